#!/bin/bash
# A/B builds of the snappy kernels: tools/snappy_variant.sh <name> <snappy.hip>
# builds tools/variants/<name>/libpsf.so (git-ignored) from the current objects
# with <snappy.hip> in place of csrc/snappy.hip; load it with
# PSF_LIBRARY_VARIANT=tools/variants/<name>/libpsf.so.
# The kernels are in csrc/snappy_common.h, snappy_compress.h and
# snappy_uncompress.h, which snappy.hip includes: a variant of a kernel is a
# directory holding a copy of snappy.hip and the changed header(s) next to it
# (the copy's includes find those first, the rest in csrc/); a snappy.hip from
# before the split is one self-contained file and builds as it is.
set -e
cd "$(dirname "$0")/.."
python -m parameter_server_amd.build > /dev/null
name=$1; src=$2
mkdir -p tools/variants/$name
OBJS=$(ls parameter_server_amd/build/*.o | grep -v "/snappy.hip.o$")
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -Iinclude \
  -Iparameter_server_amd/csrc -c "$src" -o tools/variants/$name/snappy.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/variants/$name/libpsf.so $OBJS tools/variants/$name/snappy.o
echo tools/variants/$name/libpsf.so

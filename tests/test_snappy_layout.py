"""CPU: the uncompress kernels' index arrays fit the scratch the host sizes.

The decoder's per-stream arrays are carved on the device (dscr, link_blk in
csrc/snappy_uncompress.h) and sized on the host by a formula of its own
(djob_bytes in csrc/snappy.hip).  psf_debug_snappy_dscratch runs the same
carving on the host for one stream and reports where the last array ends and
how many bytes the formula gives; if the two drifted apart the kernels would
write past the allocation.  Nothing is launched here."""
import ctypes as C

import pytest

W = 4096  # compressed bytes per parse window

CS = [1, 2, 3, 5, 4095, 4096, 4097, 4098, 4101, 8192, 65536, 65537, 65541, 2**20 + 7, 2**24 + 3,
      128 * W, 128 * W + 1, 128 * W + 5, 129 * W + 5, 2**28 + 11]
DSIZES = [0, 1, 65535, 65536, 65537, 2**20, 2**28 + 1]
CASES = [(c, hdr, d) for c in CS for hdr in range(1, 6) if hdr <= c for d in DSIZES]


@pytest.fixture(scope="module")
def dscratch():
    import parameter_server_amd as p
    fn = p.lib().psf_debug_snappy_dscratch
    fn.argtypes = [C.c_size_t, C.c_uint32, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    fn.restype = C.c_int

    def call(c, hdr, dsize):
        end, nbytes = C.c_size_t(), C.c_size_t()
        st = fn(c, hdr, dsize, C.byref(end), C.byref(nbytes))
        return st, end.value, nbytes.value
    return call


def test_index_arrays_end_inside_the_scratch(dscratch):
    assert len(CASES) == 637
    over = []
    for c, hdr, d in CASES:
        st, end, nbytes = dscratch(c, hdr, d)
        assert st == 0, (c, hdr, d)
        assert nbytes % 256 == 0
        if end > nbytes:
            over.append((c, hdr, d, end, nbytes))
    assert not over, over[:5]


def test_tightest_case_of_the_sweep(dscratch):
    """The least room the sweep leaves: 96 bytes, where the windows, the linker
    blocks and the output fragments each just passed a boundary."""
    room = {(c, hdr, d): nb - end for c, hdr, d in CASES for _, end, nb in [dscratch(c, hdr, d)]}
    worst = min(room, key=room.get)
    assert worst == (129 * W + 5, 1, 65537) and room[worst] == 96


def test_rejects_a_header_the_launch_rejects(dscratch):
    from parameter_server_amd import _lib
    for c, hdr in [(4, 5), (100, 0), (100, 6)]:
        assert dscratch(c, hdr, 10)[0] == _lib.PSF_ERR_ARG

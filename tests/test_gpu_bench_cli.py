"""GPU: bench.py's command line: what a plain run does and reports, what
--dump-outputs writes, and that --steps sets the number of timed steps.

A plain run times its steps and prints the result line, nothing else (the
diagnostic pass, the roofline, the companion lines and the CPU baseline belong
to --full; tests/test_gpu_spill.py::test_bench_default_reports_c4_spill runs
that).  --dump-outputs writes the last timed step's codes, range and decoded
values; they are checked byte for byte against the C restatement of
FIXING_FLOAT over the same input, at a size the dump keeps whole and at one it
samples.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, BUFS = 6, 3  # the last step's template, (STEPS - 1) % BUFS = 2, is not the default 20 steps' (1)


def _bench(*argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], env=env,
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    return lines[0]


@pytest.mark.parametrize("n", [(1 << 20) + 3, (1 << 22) + 5], ids=["whole", "sampled"])
def test_plain_run_line_and_dump(port, tmp_path, n):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    d = str(tmp_path / "out")
    ln = _bench("--steps", str(STEPS), "--warmup", "1", "--n", str(n), "--dump-outputs", d)
    assert ln["steps"] == STEPS and ln["warmup"] == 1 and ln["n_gpus"] == 1
    assert ln["unit"] == "GiB/s" and ln["higher_is_better"] is True and ln["dtype"] == "f64"
    assert ln["metric"].startswith("GiB/s key-value payload")
    assert ln["ms_per_step"] > 0
    # value and ms_per_step are the same measurement of STEPS steps
    assert ln["value"] == pytest.approx(4 * n / (ln["ms_per_step"] / 1e3) / 2**30, rel=2e-2)
    assert ln["roofline"] is None and ln["cpu_baseline"] is None
    assert not {"host", "config_128M", "config_c4", "config_wire"} & set(ln)

    # the last timed step's message: template (STEPS - 1) % BUFS of the seeded stream
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    xs = [torch.randn(n, device="cuda:0", generator=g, dtype=torch.float32) for _ in range(BUFS)]
    x = xs[(STEPS - 1) % BUFS].cpu().numpy()
    st, codes, mn, mx = port.ff_encode(x, 1, 12345)
    assert st == 0
    st, dec = port.ff_decode(codes, 1, mn, mx, np.float32)
    assert st == 0
    idx = bench.dump_sample_index(n)
    assert (idx is None) == (n <= bench.DUMP_MAX_ELEMS)
    if idx is not None:
        idx = idx.numpy()
        assert idx.size == bench.DUMP_MAX_ELEMS and (np.diff(idx) >= 0).all() and 0 <= idx[0] and idx[-1] < n
        codes, dec = codes[idx], dec[idx]
    got = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["decoded_values.npy", "encoded_codes.npy", "value_range.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["decoded_values.npy"].dtype == np.float32 and got["encoded_codes.npy"].dtype == np.float32
    assert got["value_range.npy"].dtype == np.float64
    assert got["value_range.npy"].tolist() == [[mn, mx]]
    assert np.array_equal(got["encoded_codes.npy"], codes.astype(np.float32))
    assert got["decoded_values.npy"].tobytes() == dec.tobytes()

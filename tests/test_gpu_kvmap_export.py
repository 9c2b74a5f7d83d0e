"""GPU: the model export, KVMap::WriteToFile's enumeration
(src/parameter/kv_map.h:99-117) as a stream compaction of the table.

The expected set comes from pull (checked against the port elsewhere): push
known keys, pull them all, keep the pairs with w != 0.  The export's pairs,
sorted by key on the host, must be exactly that set -- the same keys, the same
weight bytes, no duplicates -- at the shapes where a compaction goes wrong: an
empty table, one key, a wave's width and its neighbours, a grown table, a
count that leaves a partly kept tile, an all-zero model, the extreme keys, a
mix of zero and non-zero weights, and both entry types.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FTRL_MIXED = dict(lr_type=2, alpha=0.05, beta=1.0, lambda1=1.0, lambda2=0.5)
PLAIN = dict(lr_type=2, alpha=0.1, beta=1.0, lambda1=0.0, lambda2=0.0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keys(rng, n, hi=1 << 62):
    k = np.unique(rng.integers(0, hi, int(n * 1.2) + 8, dtype=np.uint64))
    return np.sort(rng.permutation(k)[:n])


def _push(kv, keys, rng, scale=1.0):
    g = (rng.standard_normal(keys.size) * scale).astype(np.float32)
    g[g == 0] = 1.0
    kv.push(_t(keys.view(np.int64)), _t(g))


def _expected(kv, keys):
    """(keys, w) of the pairs with w != 0 among `keys` (unique, sorted), from pull"""
    keys = np.unique(keys)
    if keys.size == 0:
        return keys, np.zeros(0, np.float32)
    w = kv.pull(_t(keys.view(np.int64))).cpu().numpy()
    keep = w != 0
    return keys[keep], w[keep]


def _exported(kv):
    k, w = kv.export()
    assert k.dtype == torch.int64 and w.dtype == torch.float32 and k.numel() == w.numel()
    k = k.cpu().numpy().view(np.uint64)
    w = w.cpu().numpy()
    o = np.argsort(k, kind="stable")
    return k[o], w[o]


def _check(kv, keys):
    ek, ew = _expected(kv, keys)
    gk, gw = _exported(kv)
    assert gk.size == ek.size
    assert np.unique(gk).size == gk.size, "a key was exported twice"
    assert gk.tobytes() == ek.tobytes()
    assert gw.tobytes() == ew.tobytes()
    return gk.size


def test_export_empty_map(ctx):
    from parameter_server_amd import filter as F
    kv = F.KVMap(ctx, capacity=1000)
    k, w = kv.export()
    assert k.numel() == 0 and w.numel() == 0
    assert kv.stats()[3] == 0


@pytest.mark.parametrize("algo", ["ftrl", "adagrad"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_export_few_keys(ctx, algo, n):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(n)
    kv = F.KVMap(ctx, capacity=1000, algo=algo, **PLAIN)
    keys = _keys(rng, n)
    _push(kv, keys, rng)
    assert _check(kv, keys) == n


@pytest.mark.parametrize("algo", ["ftrl", "adagrad"])
def test_export_after_growth(ctx, algo):
    """capacity=1000 is a 4096-slot table; 5000 keys pushed in two messages
    grow it twice before the export."""
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(50)
    kv = F.KVMap(ctx, capacity=1000, algo=algo, **PLAIN)
    keys = _keys(rng, 5_000)
    _push(kv, keys[:2_000], rng)
    _push(kv, keys, rng)
    assert _check(kv, keys) == 5_000
    assert kv.stats()[3] == 5_000


def test_export_partly_kept_tiles(ctx):
    """40 009 keys in a 2^17-slot table: every 2048-slot tile keeps some of
    its slots, none of the counts is a multiple of a wave or a tile."""
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(40)
    kv = F.KVMap(ctx, capacity=40_009, algo="adagrad", **PLAIN)
    keys = _keys(rng, 40_009)
    _push(kv, keys, rng)
    assert _check(kv, keys) == 40_009


@pytest.mark.parametrize("algo", ["ftrl", "adagrad"])
def test_export_all_zero_model(ctx, algo):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(100)
    kv = F.KVMap(ctx, capacity=1000, algo=algo, lr_type=2, alpha=0.05, beta=1.0, lambda1=100.0, lambda2=0.0)
    keys = _keys(rng, 3_000)
    _push(kv, keys, rng)
    k, w = kv.export()
    assert k.numel() == 0 and w.numel() == 0
    nnz, _, _, size = kv.stats()
    assert nnz == 0 and size == 3_000


@pytest.mark.parametrize("algo", ["ftrl", "adagrad"])
def test_export_special_keys(ctx, algo):
    """Key 0 is a valid key (only 2^64 - 1 marks a free slot); keys at and
    above 2^63 are negative in the int64 view."""
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(63)
    kv = F.KVMap(ctx, capacity=1000, algo=algo, **PLAIN)
    keys = np.unique(np.concatenate([_keys(rng, 200), np.array([0, 1, 1 << 63, (1 << 63) + 5, 2**64 - 2],
                                                               np.uint64)]))
    _push(kv, keys, rng)
    n = _check(kv, keys)
    assert n == keys.size
    gk, _ = _exported(kv)
    assert gk[0] == 0 and gk[-1] == np.uint64(2**64 - 2) and (gk >= np.uint64(1 << 63)).sum() == 3


def test_export_mixed_zero_and_nonzero(ctx):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(5)
    kv = F.KVMap(ctx, capacity=1000, **FTRL_MIXED)
    universe = _keys(rng, 12_000, 1 << 50)
    for _ in range(3):  # overlapping pushes
        _push(kv, np.sort(rng.choice(universe, 6_000, replace=False)), rng, 2.0)
    n = _check(kv, universe)
    nnz, _, _, size = kv.stats()
    assert 0 < n < size
    assert n == nnz


def test_export_capacity_contract(ctx):
    from parameter_server_amd import filter as F
    from parameter_server_amd import lib
    from parameter_server_amd._lib import PSF_ERR_ARG
    rng = np.random.default_rng(77)
    kv = F.KVMap(ctx, capacity=1000, algo="adagrad", **PLAIN)
    keys = _keys(rng, 3_000)
    _push(kv, keys, rng)
    n = C.c_size_t(12345)
    assert lib().psf_kvmap_export(kv.h, None, None, 0, C.byref(n)) == 0  # the size query
    assert n.value == 3_000
    cap, guard = 3_000 - 1, 64
    KS, WS = -0x0123456789ABCDEF, -7.25  # sentinels
    ok = torch.full((cap + guard,), KS, dtype=torch.int64, device=DEV)
    ow = torch.full((cap + guard,), WS, dtype=torch.float32, device=DEV)
    n = C.c_size_t(0)
    st = lib().psf_kvmap_export(kv.h, C.c_void_p(ok.data_ptr()), C.c_void_p(ow.data_ptr()), cap, C.byref(n))
    assert st == PSF_ERR_ARG
    assert n.value == 3_000
    assert (ok[cap:] == KS).all() and (ow[cap:] == WS).all(), "written beyond cap"
    # what was written within cap is part of the model
    ek, ew = _expected(kv, keys)
    want = dict(zip(ek.tolist(), ew.tolist()))
    gk = ok[:cap].cpu().numpy().view(np.uint64)
    gw = ow[:cap].cpu().numpy()
    done = gk != np.uint64(KS & (2**64 - 1))
    assert all(want[k] == w for k, w in zip(gk[done].tolist(), gw[done].tolist()))
    # the map still works, and a large enough buffer gets everything
    assert _check(kv, keys) == 3_000
    # null arrays are for the size query only
    assert lib().psf_kvmap_export(kv.h, None, None, 10, C.byref(n)) == PSF_ERR_ARG


@pytest.mark.parametrize("algo", ["ftrl", "adagrad"])
def test_write_file(ctx, tmp_path, algo):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(11)
    kv = F.KVMap(ctx, capacity=1000, algo=algo, **FTRL_MIXED)
    universe = _keys(rng, 6_000, 1 << 50)
    universe = np.unique(np.concatenate([universe, np.array([0, (1 << 63) + 1], np.uint64)]))
    for _ in range(2):
        _push(kv, np.sort(rng.choice(universe, 4_000, replace=False)), rng, 2.0)
    _push(kv, np.array([0, (1 << 63) + 1], np.uint64), rng, 50.0)
    gk, gw = _exported(kv)
    assert np.isfinite(gw).all() and 0 < gk.size
    want = ["%d\t%g" % (k, float(w)) for k, w in zip(gk.tolist(), gw)]
    path = tmp_path / "model" / "out_S0"  # the directory is created, as WriteToFile does
    n = kv.write_file(path, sorted=True)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[:-1] == want
    assert n == len(want) == kv.stats()[0]
    path2 = tmp_path / "unsorted"
    assert kv.write_file(path2, sorted=False) == n
    lines2 = open(path2).read().split("\n")
    assert lines2[-1] == ""
    assert sorted(lines2[:-1], key=lambda s: int(s.split("\t")[0])) == want


def test_export_is_profiled(ctx):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(2)
    kv = F.KVMap(ctx, capacity=1000, algo="adagrad", **PLAIN)
    keys = _keys(rng, 500)
    _push(kv, keys, rng)
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        n = C.c_size_t()
        ok = torch.empty(500, dtype=torch.int64, device=DEV)
        ow = torch.empty(500, dtype=torch.float32, device=DEV)
        from parameter_server_amd import lib
        assert lib().psf_kvmap_export(kv.h, C.c_void_p(ok.data_ptr()), C.c_void_p(ow.data_ptr()), 500,
                                      C.byref(n)) == 0
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert n.value == 500
    launches, ms, alg = prof["kvmap_export"]
    assert launches == 1 and ms > 0
    assert alg == 4096 * 32 + 500 * 12  # the table read + the pairs written
    assert "kvmap_push" not in prof

"""GPU: KVMap<Key, float, AdaGradEntry, SGDState> (kv_map.h:69-91,
async_sgd.h:159-176), the server's second algorithm, through the C ABI against
a numpy restatement of AdaGradEntry::Set:

* weights bit-exact after several pushes with table growth, nnz and size exact,
  the float sums within summation-order error;
* the fused push of deferred FIXING_FLOAT codes (the nb == 1 table and the
  general dequantise) feeds the new entry the decode's exact values;
* an AdaGrad map serves a router's pull like an FTRL map;
* the default entry is still FTRL.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keys(rng, n, hi):
    return np.unique(rng.integers(0, hi, int(n * 1.2) + 8).astype(np.uint64))[:n]


class AdaGradModel:
    """KVMap<Key, float, AdaGradEntry, SGDState> restated for tests: a key ->
    entry map (the reference's unordered_map, kv_map.h:65) over numpy arrays,
    AdaGradEntry::Set (async_sgd.h:160-171) vectorised over one push's keys in
    np.float32, one rounded operation per reference operation.  The keys of a
    push are unique, so the vectorised update is the serial one.

    The state is the SGDState(penalty, learning_rate) the reference's FTRL
    branch sets (async_sgd.h:47-52); its AdaGrad branch forgets set_state
    (async_sgd.h:54-56)."""

    def __init__(self, lr_type=2, alpha=0.01, beta=10.0, lambda1=0.0, lambda2=0.0):
        self.decay = lr_type != 1  # LearningRateConfig::CONSTANT = 1
        f = np.float32
        self.alpha, self.beta, self.l1, self.l2 = f(alpha), f(beta), f(lambda1), f(lambda2)
        assert self.alpha > 0 and self.beta >= 0  # learning_rate.h:10-11
        assert self.l1 >= 0 and self.l2 >= 0  # penalty.h:44-45
        self.index = {}
        self.weight = np.zeros(1 << 10, np.float32)
        self.sum_sq_grad = np.zeros(1 << 10, np.float32)
        self.nnz = 0
        self.weight_sum = np.float32(0)
        self.delta_sum = np.float32(0)

    def _entries(self, keys):
        idx = np.empty(len(keys), np.int64)
        for i, k in enumerate(keys.tolist()):
            e = self.index.get(k)
            if e is None:
                e = self.index[k] = len(self.index)
            idx[i] = e
        if len(self.index) > self.weight.size:
            cap = 1 << (len(self.index) - 1).bit_length()
            for a in ("weight", "sum_sq_grad"):
                old = getattr(self, a)
                new = np.zeros(cap, np.float32)
                new[:old.size] = old
                setattr(self, a, new)
        return idx

    def push(self, keys, grad):
        keys = np.asarray(keys, np.uint64)
        assert np.unique(keys).size == keys.size
        idx = self._entries(keys)
        one = np.float32(1)
        grad = np.ascontiguousarray(grad, np.float32)
        ss = self.sum_sq_grad[idx] + grad * grad  # sum_sq_grad += grad * grad, :164
        root = np.sqrt(ss)  # float32 in, float32 out (= the double sqrt rounded to float)
        # LearningRate::eval, learning_rate.h:15-22
        eta = self.alpha / (root + self.beta) if self.decay else np.full_like(root, self.alpha)
        w_old = self.weight[idx]  # :166
        z = w_old - eta * grad  # :167
        assert (eta > 0).all()  # CHECK_GT(eta, 0), penalty.h:52
        leta = self.l1 * eta  # penalty.h:53
        den = one + self.l2 * eta
        w = np.where(z > 0, (z - leta) / den, (z + leta) / den)  # penalty.h:55
        w = np.where((z <= leta) & (z >= -leta), np.float32(0), w).astype(np.float32)  # penalty.h:54
        assert ss.dtype == eta.dtype == z.dtype == w.dtype == np.float32
        self.sum_sq_grad[idx] = ss
        self.weight[idx] = w
        # SGDState::UpdateWeight, async_sgd.h:106-116 (the sums serially in float)
        self.nnz += int(((w != 0) & (w_old == 0)).sum()) - int(((w == 0) & (w_old != 0)).sum())
        delta = w - w_old
        self.weight_sum = np.cumsum(np.concatenate([[self.weight_sum], w * w]), dtype=np.float32)[-1]
        self.delta_sum = np.cumsum(np.concatenate([[self.delta_sum], delta * delta]), dtype=np.float32)[-1]

    def pull(self, keys):
        out = np.zeros(len(keys), np.float32)
        for i, k in enumerate(np.asarray(keys, np.uint64).tolist()):
            e = self.index.get(k)
            if e is not None:
                out[i] = self.weight[e]
        return out


CONFIGS = [(2, 0.1, 1.0, 1.0, 0.1), (2, 0.01, 10.0, 0.0, 0.0), (1, 0.1, 0.0, 0.05, 0.5), (2, 0.5, 1.0, 100.0, 0.0)]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_kvmap_adagrad_vs_reference(ctx, cfg):
    from parameter_server_amd import filter as F
    lr_type, alpha, beta, l1, l2 = cfg
    model = AdaGradModel(lr_type, alpha, beta, l1, l2)
    kv = F.KVMap(ctx, capacity=1000, lr_type=lr_type, alpha=alpha, beta=beta, lambda1=l1, lambda2=l2,
                 algo="adagrad")
    rng = np.random.default_rng(int(alpha * 1000))
    universe = _keys(rng, 60_000, 1 << 50)
    for step in range(5):  # overlapping key sets; the table grows past 1000
        keys = np.sort(rng.choice(universe, 25_000, replace=False))
        g = (rng.standard_normal(keys.size) * 2).astype(np.float32)
        model.push(keys, g)
        kv.push(_t(keys.view(np.int64)), _t(g))
    stored = model.pull(np.array(sorted(model.index), np.uint64))
    assert np.isfinite(stored).all()
    if cfg == CONFIGS[0]:  # both sides of the soft threshold
        assert 0 < (stored != 0).sum() < stored.size
    if cfg == CONFIGS[3]:  # lambda1 = 100 zeroes every weight
        assert (stored != 0).sum() == 0
    probe = np.concatenate([universe, _keys(rng, 100, 1 << 50) + np.uint64(1 << 51)])
    got = kv.pull(_t(probe.view(np.int64))).cpu().numpy()
    assert got.tobytes() == model.pull(probe).tobytes()
    nnz, ws, ds, size = kv.stats()
    print("adagrad", cfg, "nnz", nnz, "size", size, "weight_sum", ws, float(model.weight_sum), "delta_sum", ds,
          float(model.delta_sum))
    assert nnz == model.nnz == (stored != 0).sum()
    assert size == len(model.index)
    assert ws >= 0 and abs(ws - float(model.weight_sum)) <= 1e-3 * max(1.0, ws)
    assert abs(ds - float(model.delta_sum)) <= 1e-3 * max(1.0, ds)


def _push_message(F, keys, x, nb, channel):
    from parameter_server_amd import FIXING_FLOAT, KEY_CACHING
    m = F.Message(request=True, push=True, key_channel=channel, key_range=(0, 1 << 62))
    m.set_key(_t(keys.view(np.int64)))
    m.add_value(_t(x))
    m.add_filter(KEY_CACHING)
    m.add_filter(FIXING_FLOAT, num_bytes=nb)
    return m


def test_kvmap_adagrad_fused_push_messages(ctx, port):
    """Push messages [KEY_CACHING, FIXING_FLOAT] decoded with the dequantise
    deferred into KVMap::SetValue on an AdaGrad map: three at nb = 1 (the
    256-entry table) and one at nb = 2 (the general dequantise), then a pull
    message answered by KVMap::GetValue."""
    from parameter_server_amd import filter as F
    F.set_clock(777)
    try:
        cfg = dict(lr_type=2, alpha=0.1, beta=1.0, lambda1=0.5, lambda2=0.1)
        model = AdaGradModel(**cfg)
        kv = F.KVMap(ctx, capacity=1 << 14, algo="adagrad", **cfg)
        worker, server = F.RemoteNode(ctx), F.RemoteNode(ctx)
        server.set_defer_dequant(True)
        rng = np.random.default_rng(3)
        for step, nb in enumerate([1, 1, 1, 2]):
            keys = _keys(rng, 8_000, 1 << 15)  # a small universe: the pushes overlap
            x = (rng.standard_normal(keys.size) * 3).astype(np.float32)
            m = _push_message(F, keys, x, nb, channel=step)
            worker.encode(m)
            w = m.clone()
            server.decode(w)
            assert w.pending(0) is not None and w.pending(0)[0] == nb
            kv.set_value(w)
            st, codes, mn, mx = port.ff_encode(x, nb, 777)
            assert st == 0
            st, dec = port.ff_decode(codes, nb, mn, mx, np.float32)
            assert st == 0
            model.push(keys, dec)
        allk = np.array(sorted(model.index), np.uint64)
        assert allk.size < 4 * 8_000  # keys were updated more than once
        pull = F.Message(request=True, push=False)
        pull.set_key(_t(allk.view(np.int64)))
        kv.get_value(pull)
        assert pull.num_values() == 1
        got = server.value(pull, 0).cpu().numpy().view(np.float32)
        want = model.pull(allk)
        assert 0 < (want != 0).sum()
        assert got.tobytes() == want.tobytes()
        assert kv.stats()[0] == model.nnz
    finally:
        F.set_clock(None)


def test_kvmap_adagrad_serves_router_pull():
    """A world-1 router answers pulls from an AdaGrad map exactly as
    KVMap.pull reads it (the get kernels do not depend on the entry type)."""
    import oracle
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    from test_gpu_pull import SEED, _keys as stream_keys, check_pulled, expected_slices, make_requests, seed_store
    M, S = 1 << 9, 2
    F.set_clock(SEED)
    try:
        ctx = F.Context(0)
        ranges = shard.server_ranges(S)
        router = shard.PushRouter(ctx, ranges, 0, 1)
        kv = F.KVMap(ctx, capacity=2 * M, lr_type=2, alpha=0.1, beta=1.0, algo="adagrad")
        router.set_store(kv)
        reqs = make_requests(F, [0, 1], M)
        seed_store(F, kv, np.concatenate([stream_keys(s, M) for s in range(2)]))
        port = oracle.Port()
        data = {s: (stream_keys(s, M), expected_slices(kv, stream_keys(s, M), ranges, range(S), port))
                for s in range(2)}
        assert all((sl[0] != 0).any() for _, by_server in data.values() for sl in by_server.values() if sl)
        router.pull(reqs, 1)
        torch.cuda.synchronize()
        check_pulled(F, router.pulled(), data, ranges)
    finally:
        F.set_clock(None)


def test_kvmap_default_is_ftrl(ctx):
    from parameter_server_amd import filter as F
    rng = np.random.default_rng(9)
    keys = _keys(rng, 5_000, 1 << 40)
    g = rng.standard_normal(keys.size).astype(np.float32)
    cfg = dict(capacity=1000, lr_type=2, alpha=0.05, beta=1.0, lambda1=0.1, lambda2=0.5)
    pulls = []
    for kw in ({}, {"algo": "ftrl"}, {"algo": "adagrad"}):
        kv = F.KVMap(ctx, **cfg, **kw)
        for _ in range(2):
            kv.push(_t(keys.view(np.int64)), _t(g))
        pulls.append(kv.pull(_t(keys.view(np.int64))).cpu().numpy())
    assert (pulls[0] != 0).any()
    assert pulls[0].tobytes() == pulls[1].tobytes()
    assert pulls[0].tobytes() != pulls[2].tobytes()  # the keyword does select the entry
    with pytest.raises(Exception):
        F.KVMap(ctx, **cfg, algo="nope")
    # the C ABI rejects an unknown algo as well
    import ctypes as C
    from parameter_server_amd import lib
    from parameter_server_amd._lib import PSF_ERR_ARG
    h = C.c_void_p()
    assert lib().psf_kvmap_create_algo(ctx.h, 1000, 7, 2, 0.05, 1.0, 0.1, 0.5, C.byref(h)) == PSF_ERR_ARG
    assert not h.value

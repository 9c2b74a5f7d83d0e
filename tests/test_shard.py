"""CPU: the multi-server / multi-GPU split.

* Range<Key>::EvenDivide in libpsf == the restatement of range.h:100-107 (fixture)
* SliceKOFVMessage in libpsf (host keys) == the numpy restatement
* the all-to-all-v spill exchange over world_size 2 with gloo
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def test_even_divide_matches_fixture():
    from oracle import slicing
    from parameter_server_amd import shard
    rows = json.load(open(os.path.join(GOLDEN, "even_divide.json")))
    assert len(rows) > 2000
    for b, e, n, i, ob, oe in rows:
        want = (int(ob), int(oe))
        assert shard.even_divide((int(b), int(e)), n, i) == want
        assert slicing.even_divide(int(b), int(e), n, i) == want
    # the reference's defect is reproduced: 7 servers over Range::All()
    assert shard.even_divide(shard.KEY_ALL, 7, 6)[1] == 0


def _keys(n, seed, hi=1 << 64):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(0, hi - 1, size=n + 64, dtype=np.uint64))[:n]
    return k


@pytest.mark.parametrize("nserv", [1, 2, 3, 7, 8])
@pytest.mark.parametrize("mrange", ["all", "part", "narrow"])
def test_slice_host_keys_matches_restatement(nserv, mrange):
    from oracle import slicing
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    keys = _keys(5000, nserv)
    v1 = np.random.default_rng(1).standard_normal(keys.size).astype(np.float32)
    v3 = np.random.default_rng(2).standard_normal(keys.size * 3).astype(np.float32)  # dim 3 rows
    mr = {"all": shard.KEY_ALL, "part": (int(keys[100]), int(keys[4000])),
          "narrow": (int(keys[10]), int(keys[12]))}[mrange]
    ctx = F.HostContext()
    m = F.Message(request=True, push=True, key_range=mr)
    m.set_key(torch.from_numpy(keys.view(np.int64).copy()))
    m.add_value(torch.from_numpy(v1))
    m.add_value(torch.from_numpy(v3))
    ranges = shard.server_ranges(nserv)
    if nserv == 7:
        ranges[-1] = (ranges[-1][0], (1 << 64) - 1)  # contiguous stand-in for the end=0 defect
    parts = shard.slice_message(ctx, m, ranges)
    want = slicing.slice_kofv(keys, [v1, v3], mr, ranges)
    assert len(parts) == len(want) == nserv
    total = 0
    for p, w in zip(parts, want):
        if w is None:
            assert p is None
            continue
        assert p is not None
        ptr, nb, loc = p.key_ptr()
        got = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * nb).from_address(ptr)) if nb else np.zeros(0, np.uint8)
        assert got.tobytes() == w[0].tobytes()
        total += w[0].size
        for j, wv in enumerate(w[1]):
            vp, vb, _ = p.value_ptr(j)
            gv = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * vb).from_address(vp)) if vb else np.zeros(0, np.uint8)
            assert gv.tobytes() == wv.tobytes()
        assert p.key_info()[1] == 8  # key_type = UINT64 (EncodeType<K>)
    if mrange == "all":
        assert total == keys.size


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spill_msgs(rank, world):
    """the messages rank `rank` sends: (dest, server, key bytes or None, values)"""
    out = []
    for d in range(world):
        if rank == 0 and d == 1:
            continue  # a peer with nothing to send
        for j in range(d + 1 + rank):
            keys = (np.arange(10 * rank + 3 * d + j + 1, dtype=np.uint64) * 7 + j) if j % 2 == 0 else None
            vals = [np.full(5 + j, rank + d + 0.5, np.float32), np.zeros(0, np.float32),
                    np.arange(j + 1, dtype=np.float64)]
            out.append((d, 10 + d, 100 * rank + 10 * d + j, keys, vals))
    return out


def _exchange_worker(rank, world, port, q):
    import torch.distributed as dist

    from parameter_server_amd import KEY_CACHING
    from parameter_server_amd import filter as F
    from parameter_server_amd.shard import SpillExchange, w_channel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = F.HostContext()
        ex = SpillExchange(ctx)
        msgs, dest, server = [], [], []
        for d, srv, ch, keys, vals in _spill_msgs(rank, world):
            m = F.Message(request=True, push=True, key_channel=ch, key_range=(5, 1 << 40))
            if keys is not None:
                m.set_key(torch.from_numpy(keys.view(np.int64).copy()))
            for v in vals:
                m.add_value(torch.from_numpy(v.copy()))
            m.add_filter(KEY_CACHING)
            msgs.append(m)
            dest.append(d)
            server.append(srv)
        got, servers = ex.exchange(msgs, dest, server)
        want = [w for s in range(world) for w in _spill_msgs(s, world) if w[0] == rank]
        ok = len(got) == len(want)
        for m, srv, (d, wsrv, ch, keys, vals) in zip(got, servers, want):
            ok &= srv == wsrv and w_channel(m) == ch
            has_key, _ = m.key_info()
            ptr, nb, _ = m.key_ptr()
            kb = bytes((np.ctypeslib.ctypes.c_uint8 * nb).from_address(ptr)) if nb else b""
            ok &= has_key == (keys is not None) and kb == (b"" if keys is None else keys.tobytes())
            ok &= m.num_values() == len(vals)
            for i, v in enumerate(vals):
                vp, vb, _ = m.value_ptr(i)
                gb = bytes((np.ctypeslib.ctypes.c_uint8 * vb).from_address(vp)) if vb else b""
                ok &= gb == v.tobytes()
        q.put((rank, bool(ok)))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_spill_exchange_gloo_world2():
    """psf_spill_pack / fill / unpack through one gloo all-to-all-v: every
    message (Task, key frame, value frames incl. empty ones, server id) arrives
    intact, in order, at its rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}


def _router_worker(rank, world, port, q, native=False):
    import torch.distributed as dist

    from bench import splitmix64_keys
    from parameter_server_amd import KEY_CACHING
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = F.HostContext()
        ranges = shard.server_ranges(5)  # 5 servers in blocks over the ranks (2 + 3 at world 2)
        ex = shard.NativeExchange.create(ctx, transport="host") if native else shard.SpillExchange(ctx)
        router = shard.PushRouter(ctx, ranges, rank, world, ex)
        sids = [10 * r + j for r in range(world) for j in range(3)]
        data = {s: (splitmix64_keys(700 + s, 4 + s),) for s in sids}
        data = {s: (k[0], np.random.default_rng(s).standard_normal(2 * k[0].size).astype(np.float32))
                for s, k in data.items()}
        streams = {}
        for s in sids:
            if s // 10 != rank:
                continue
            keys, vals = data[s]
            m = F.Message(request=True, push=True, key_channel=s, key_range=shard.KEY_ALL)
            m.set_key(torch.from_numpy(keys.view(np.int64).copy()))
            m.add_value(torch.from_numpy(vals.copy()))
            m.add_filter(KEY_CACHING)
            streams[s] = m
        mine = [d for d in range(5) if shard.server_rank(d, 5, world) == rank]
        ok = True
        for step in range(4):  # miss (keys travel), then hits (keys elided, restored)
            if native and step == 3:
                router.run(streams, 3)  # three steps in one call: the mailbox banks alternate
            else:
                router.step(streams)
            seen = set()
            for d, w in router.results():
                s = shard.w_channel(w)
                seen.add((d, s))
                keys, vals = data[s]
                lo, hi = ranges[d]
                sel = (keys >= np.uint64(lo)) & (keys < np.uint64(hi))
                p, nb, _ = w.key_ptr()
                kb = bytes((np.ctypeslib.ctypes.c_uint8 * nb).from_address(p)) if nb else b""
                vp, vb, _ = w.value_ptr(0)
                vbytes = bytes((np.ctypeslib.ctypes.c_uint8 * vb).from_address(vp)) if vb else b""
                ok &= kb == keys[sel].tobytes() and vbytes == vals.reshape(-1, 2)[sel].tobytes()
            ok &= seen == {(d, s) for d in mine for s in sids}
        q.put((rank, bool(ok)))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,native", [(2, False), (2, True), (4, True)])
def test_push_router_gloo_world2_host(world, native):
    """The native router (psf_router_*) across two (four) ranks on CPU: 3
    streams per rank, 5 servers (in blocks over the ranks), host keys,
    [KEY_CACHING]; every server's decoded slices equal the restated slicing,
    on the miss and the hit steps.  native: libpsf's exchange (records and
    data through the node's mailbox, psf_router_step at world 2 / 4, the last
    three steps in one call) instead of gloo's all-to-all-v."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_router_worker, args=(r, world, port, q, native)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {r: True for r in range(world)}, res


def test_bench_launcher_gloo_world2():
    """`bench.py --gpus 2` starts its two ranks itself (no torchrun) and the
    process group really has two members (launch plumbing only, on CPU)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "c4",
                          "--launch-check"], env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    assert lines[0]["n_gpus"] == 2 and lines[0]["world_size"] == 2 and lines[0]["backend"] == "gloo"


def test_bench_launcher_default_carries_config_c4():
    """The default (c2) multi-GPU command with --full also runs C4's cross-range
    spill and reports it as config_c4 (its world size, backend, strong scaling)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSF_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--full",
                          "--launch-check"], env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    c4 = lines[0]["config_c4"]
    assert c4["world_size"] == 2 and c4["backend"] == "gloo" and c4["scaling"] == "strong"
    assert "all-to-all-v" in c4["parallelism"]


def test_slice_many_host_keys_matches_restatement():
    """psf_msgs_slice (many messages, one synchronisation) == the restatement."""
    from oracle import slicing
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    ctx = F.HostContext()
    ranges = shard.server_ranges(4)
    msgs, data = [], []
    for j in range(5):
        keys = _keys(1000 + 37 * j, 100 + j)
        v = np.random.default_rng(j).standard_normal(keys.size * 2).astype(np.float32)
        m = F.Message(request=True, push=True, key_range=shard.KEY_ALL)
        m.set_key(torch.from_numpy(keys.view(np.int64).copy()))
        m.add_value(torch.from_numpy(v))
        msgs.append(m)
        data.append((keys, v))
    for parts, (keys, v) in zip(shard.slice_messages(ctx, msgs, ranges), data):
        want = slicing.slice_kofv(keys, [v], shard.KEY_ALL, ranges)
        for p, w in zip(parts, want):
            assert (p is None) == (w is None)
            if w is None:
                continue
            ptr, nb, loc = p.key_ptr()
            got = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * nb).from_address(ptr)) if nb else np.zeros(0, np.uint8)
            assert got.tobytes() == w[0].tobytes()


def test_push_router_u32_keys_host():
    """SliceKOFVMessage<K> slices with the application's key type: a stream
    whose task.key_type is UINT32 is cut at 32-bit keys (message.h:107-147),
    every server gets its keys and value rows; unsupported key types and ragged
    key buffers are rejected (SArray<K>'s size CHECK), as is a step mixing
    32- and 64-bit streams."""
    from parameter_server_amd import KEY_CACHING, PsfError
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    from parameter_server_amd._lib import DT_UINT64
    DT_UINT32 = 7
    ctx = F.HostContext()
    key_range = (0, (1 << 32) - 1)  # K = uint32: range ends must fit K
    ranges = [shard.even_divide(key_range, 3, i) for i in range(3)]
    router = shard.PushRouter(ctx, ranges, 0, 1)
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, (1 << 32) - 1, 5000, dtype=np.uint64)).astype(np.uint32)
    vals = rng.standard_normal(3 * keys.size).astype(np.float32)
    m = F.Message(request=True, push=True, key_channel=3, key_range=key_range)
    m.set_key(torch.from_numpy(keys.view(np.int32).copy()), key_type=DT_UINT32)
    m.add_value(torch.from_numpy(vals.copy()))
    m.add_filter(KEY_CACHING)
    for step in range(2):  # miss, then hit
        router.step({3: m})
        got = {d: w for d, w in router.results()}
        assert sorted(got) == [0, 1, 2]
        for d, w in got.items():
            lo, hi = ranges[d]
            sel = (keys.astype(np.uint64) >= np.uint64(lo)) & (keys.astype(np.uint64) < np.uint64(hi))
            assert sel.sum() > 0
            p, nb, _ = w.key_ptr()
            kb = bytes((np.ctypeslib.ctypes.c_uint8 * nb).from_address(p)) if nb else b""
            assert kb == keys[sel].tobytes(), (step, d)
            vp, vb, _ = w.value_ptr(0)
            vbytes = bytes((np.ctypeslib.ctypes.c_uint8 * vb).from_address(vp))
            assert vbytes == vals.reshape(-1, 3)[sel].tobytes(), (step, d)
    bad = F.Message(request=True, push=True, key_channel=4, key_range=key_range)
    bad.set_key(torch.from_numpy(np.arange(10, dtype=np.int16)), key_type=2)  # INT16
    with pytest.raises(PsfError):
        router.step({4: bad})
    ragged = F.Message(request=True, push=True, key_channel=5, key_range=key_range)
    ragged.set_key(torch.from_numpy(np.arange(7, dtype=np.uint8)), key_type=DT_UINT32)
    with pytest.raises(PsfError):
        router.step({5: ragged})
    # a range end of 2^32 wraps to 0 in the (K) cast: the reference's
    # Segment CHECK (shared_array_inl.h:135) fails, so does the router
    r32 = [shard.even_divide((0, 1 << 32), 3, i) for i in range(3)]
    m32 = F.Message(request=True, push=True, key_channel=7, key_range=(0, 1 << 32))
    m32.set_key(torch.from_numpy(keys.view(np.int32).copy()), key_type=DT_UINT32)
    with pytest.raises(PsfError):
        shard.PushRouter(ctx, r32, 0, 1).step({7: m32})
    wide = F.Message(request=True, push=True, key_channel=6, key_range=key_range)
    wide.set_key(torch.from_numpy(np.arange(4, dtype=np.int64)), key_type=DT_UINT64)
    with pytest.raises(PsfError):
        router.step({3: m, 6: wide})


def _failfast_worker(rank, world, port, q):
    import time

    import torch.distributed as dist

    from bench import splitmix64_keys
    from parameter_server_amd import KEY_CACHING
    from parameter_server_amd import filter as F
    from parameter_server_amd import shard
    from parameter_server_amd._lib import PsfError
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PSF_EXCHANGE_TIMEOUT_S="60")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    try:
        ctx = F.HostContext()
        # a misconfigured rank: rank 1 splits the key space into 4 servers,
        # rank 0 into 2 -- rank 0's slices for its server 1 land on rank 1,
        # which under its own split does not host a server 1
        ranges = shard.server_ranges(2 if rank == 0 else 4)
        ex = shard.NativeExchange.create(ctx, transport="host")
        router = shard.PushRouter(ctx, ranges, rank, world, ex)
        keys = splitmix64_keys(500, 4 + rank)
        # rank 1's keys and key range in its own servers' half: it sends rank 0
        # nothing (slices whose range misses the key range are not sent)
        kr = shard.KEY_ALL
        if rank == 1:
            keys = np.unique(keys | np.uint64(1 << 63))
            kr = (1 << 63, (1 << 64) - 1)
        m = F.Message(request=True, push=True, key_channel=rank, key_range=kr)
        m.set_key(torch.from_numpy(keys.view(np.int64).copy()))
        m.add_value(torch.ones(keys.size, dtype=torch.float32))
        m.add_filter(KEY_CACHING)
        for step in range(3):
            t0 = time.perf_counter()
            try:
                router.run({rank: m}, 1)
                out.append(("ok", 0.0))
            except PsfError as e:
                out.append((str(e), time.perf_counter() - t0))
        out.append(("stats", ex.data_stats()["failed"]))
        q.put((rank, out))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def test_exchange_fails_fast_on_every_rank():
    """A step that fails between post and move (here: a record for a server
    the rank does not host) marks the exchange failed: the failing rank's
    next call and the peer's next wait raise at once, naming the cause or the
    rank, instead of hanging until PSF_EXCHANGE_TIMEOUT_S."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_failfast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    r0, r1 = res[0], res[1]
    assert isinstance(r1, list), r1
    assert "does not own" in r1[0][0], r1
    assert all("earlier step failed" in str(msg) for msg, _ in r1[1:3]), r1
    assert r1[3] == ("stats", True), r1
    assert isinstance(r0, list), r0
    # rank 0's own steps are sound: its first wait on rank 1 raises at once
    fails = [(msg, dt) for msg, dt in r0[:3] if msg != "ok"]
    assert fails and "rank 1 failed" in fails[0][0] and all(dt < 10 for _, dt in fails), r0

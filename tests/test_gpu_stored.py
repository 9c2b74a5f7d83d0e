"""GPU: FIXING_FLOAT codes written straight into the stored snappy stream
layout when COMPRESSING follows (chain [..., FIXING_FLOAT, (KEY_CACHING,)
COMPRESSING]).  The compressor leaves a stream whose fragments all come out
stored where FIXING_FLOAT wrote it (header and tags included) and places the
others as usual, so every encoded stream must be byte-identical to the snappy
1.1.8 restatement of the restatement's codes (fixing_float.h:73-88, then
compressing.h:16-19 -> shared_array_inl.h:232-245), whatever the sizes: a
stream ending on a fragment / tile / group boundary or just past one, the
last fragment's tag of 1, 2 or 3 bytes, tiny arrays, num_bytes 1 and 2, f32
and f64, one message or a batch, and streams with a compressible fragment
(the fallback placement) or compressible throughout.  Decoding gives the
restatement's values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 424242
F64 = np.float64


def _values(kind, n, dt, seed, nb):
    x = np.random.default_rng(seed).standard_normal(n).astype(dt)
    per = 65536 // nb  # values per fragment
    if kind == "onecomp" and n > 3 * per:  # fragment 2 constant: codes with matches
        x[2 * per:3 * per] = 0.25
    elif kind == "lastcomp":  # the last fragment constant
        x[(n - 1) // per * per:] = -0.5
    elif kind == "allcomp":
        x[:] = 1.0
        x[::7] = -1.0  # (a range: bin > 0)
    elif kind == "firstcomp":  # fragment 0 shrinks to a few bytes: every later one moves ~64 KiB down
        x[:per] = 0.0
    elif kind == "everyother":  # every other fragment compressible
        for f in range(0, n // per + 1, 2):
            x[f * per:(f + 1) * per] = 0.75
    return x


CASES = [  # kind, n values, nb, dtype
    ("random", 16 * 65536, 1, np.float32),
    ("random", 16 * 65536 + 1, 1, np.float32),
    ("random", 16 * 65536 + 3, 1, np.float32),
    ("random", 16 * 65536 + 4, 1, np.float32),
    ("random", 5 * 65536 + 60, 1, np.float32),
    ("random", 5 * 65536 + 61, 1, np.float32),
    ("random", 5 * 65536 + 256, 1, np.float32),
    ("random", 5 * 65536 + 257, 1, np.float32),
    ("random", 3 * 65536 + 4095, 1, np.float32),
    ("random", 3 * 65536 + 4096, 1, np.float32),
    ("random", 3 * 65536 + 4100, 1, np.float32),
    ("random", 65536, 1, np.float32),
    ("random", 65537, 1, np.float32),
    ("random", 4096, 1, np.float32),
    ("random", 1000, 1, np.float32),
    ("random", 15, 1, np.float32),
    ("random", 14, 1, np.float32),
    ("random", 1, 1, np.float32),
    ("random", 8 * 32768, 2, np.float32),
    ("random", 8 * 32768 + 1, 2, np.float32),
    ("random", 8 * 32768 + 30, 2, np.float32),
    ("random", 8 * 32768 + 31, 2, np.float32),
    ("random", 3 * 32768 + 2049, 2, np.float32),
    ("random", 7, 2, np.float32),
    ("random", 4 * 65536 + 5, 1, F64),
    ("random", 4 * 32768 + 2048, 2, F64),
    ("onecomp", 12 * 65536 + 333, 1, np.float32),
    ("onecomp", 9 * 32768 + 7, 2, np.float32),
    ("lastcomp", 6 * 65536 + 5000, 1, np.float32),
    ("allcomp", 4 * 65536 + 17, 1, np.float32),
    ("firstcomp", 10 * 65536 + 99, 1, np.float32),
    ("firstcomp", 6 * 32768 + 3, 2, np.float32),
    ("everyother", 9 * 65536 + 1234, 1, np.float32),
    ("everyother", 5 * 32768, 2, F64),
]


def _msg(F, x, nb, kc_between=False):
    from parameter_server_amd import COMPRESSING, FIXING_FLOAT, KEY_CACHING
    m = F.Message(request=True, push=True, key_channel=3, key_range=(0, 1 << 40))
    if kc_between:
        m.set_key(torch.arange(1000, device="cuda:0", dtype=torch.int64) * 3)
    m.add_value(torch.from_numpy(x).cuda())
    m.add_filter(FIXING_FLOAT, num_bytes=nb)
    if kc_between:
        m.add_filter(KEY_CACHING)
    m.add_filter(COMPRESSING)
    return m


def _want(port, x, nb):
    st, codes, mn, mx = port.ff_encode(x, nb, SEED)
    assert st == 0
    st, dec = port.ff_decode(codes, nb, mn, mx, x.dtype)
    return port.snappy_compress(codes.tobytes()), dec.tobytes()


@pytest.mark.parametrize("batched", [False, True])
def test_stored_layout_streams_vs_port(ctx, port, batched):
    from parameter_server_amd import filter as F
    F.set_clock(SEED)
    try:
        xs = [_values(kind, n, dt, 50 + k, nb) for k, (kind, n, nb, dt) in enumerate(CASES)]
        msgs = [_msg(F, x, c[2], kc_between=(k % 5 == 1)) for k, (x, c) in enumerate(zip(xs, CASES))]
        snd = [F.RemoteNode(ctx) for _ in msgs]
        if batched:
            F.RemoteNode.encode_many(snd, msgs)
        else:
            for nd, m in zip(snd, msgs):
                nd.encode(m)
        ctx.sync()
        for k, (x, c, m) in enumerate(zip(xs, CASES, msgs)):
            stream, dec = _want(port, x, c[2])
            vp, vn, vl = m.value_ptr(0)
            got = F.copy_out(vp, vn, vl, "cuda:0").cpu().numpy().tobytes()
            ok = got == stream
            assert ok, (c, len(got), len(stream))
            w = m.clone()
            rcv = F.RemoteNode(ctx)
            rcv.decode(w)
            assert rcv.value(w, 0).cpu().numpy().tobytes() == dec, c
    finally:
        F.set_clock(None)


def test_stored_layout_long_stream_scan_path(ctx, port):
    """A stream of 4100 fragments (more than kInlineScan: offsets from the
    per-stream scan launch) with compressible fragments at 1000 and 3000:
    compacted in place, byte-identical to 1.1.8's stream."""
    from parameter_server_amd import filter as F
    F.set_clock(SEED)
    try:
        n = 4100 * 65536 + 77
        x = np.random.default_rng(9).standard_normal(n).astype(np.float32)
        x[1000 * 65536:1001 * 65536] = 0.5
        x[3000 * 65536 + 100:3000 * 65536 + 40000] = -0.25
        m = _msg(F, x, 1)
        F.RemoteNode(ctx).encode(m)
        ctx.sync()
        stream, _ = _want(port, x, 1)
        vp, vn, vl = m.value_ptr(0)
        got = F.copy_out(vp, vn, vl, "cuda:0").cpu().numpy().tobytes()
        ok = got == stream
        assert ok, (len(got), len(stream))
    finally:
        F.set_clock(None)


def _skip_cum(n=384):
    """offset of the skip loop's probe k from where it starts (1.1.8: skip
    starts at 32, each probe advances by skip >> 5, then skip += skip >> 5)"""
    v, skip, cum = [], 32, 0
    for _ in range(n):
        v.append(cum)
        step = skip >> 5
        skip += step
        cum += step
    return v


def _stored_layout(payload):
    """varint(n) + per 64 KiB fragment: literal tag + bytes (1.1.8's stream of
    data without matches)"""
    n = len(payload)
    out = bytearray()
    v = n
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    for k in range(0, n, 65536):
        frag = payload[k:k + 65536]
        m = len(frag) - 1
        if m < 60:
            out.append(m << 2)
        elif m < 256:
            out += bytes([60 << 2, m])
        else:
            out += bytes([61 << 2, m & 255, m >> 8])
        out += frag
    return bytes(out)


def _planted(nfrag, plant, seed, tail=0, zeros=(), early=()):
    """random bytes; in fragment k of `plant` the 4 bytes at the skip loop's
    probe 150 copy those at probe 10 (one 4-byte match, far: the fragment
    comes out a byte longer than a literal), in fragment k of `early` those
    at probe 20 copy probe 2 (the final literal starts 25 bytes in, the
    fragment comes out 1 byte shorter); fragments in `zeros` zero"""
    cum = _skip_cum()
    b = np.random.default_rng(seed).integers(0, 256, nfrag * 65536 + tail, dtype=np.uint8)
    for k, (a, z) in [(k, (10, 150)) for k in plant] + [(k, (2, 20)) for k in early]:
        p, q = k * 65536 + 1 + cum[a], k * 65536 + 1 + cum[z]
        b[q:q + 4] = b[p:p + 4]
        b[q + 4] = b[p + 4] ^ 0x5A
    for k in zeros:
        b[k * 65536:(k + 1) * 65536] = 0
    return b.tobytes()


@pytest.mark.parametrize("case", ["grow", "grow_every", "shrink_then_grow", "grow_then_shrink", "grow_tail",
                                  "grow_early", "grow_over", "grow_short_tail1", "grow_short_tail2", "grow_one_last",
                                  "shrink_small", "shrink_grow_mixed", "shrink_over"])
def test_compress_stored_in_place(ctx, port, case):
    """psf_snappy_compress_stored: a stored-layout stream compressed, for
    streams whose fragments with tags come out longer than literals and
    shorter (down by whole fragments), byte-identical to 1.1.8.  Streams that
    grow by at most 64 bytes (and never shrink below a fragment's stored
    start) are rewritten in place by K-place, the later fragments moved right
    (snappy_compress.h kPlaceShift; "grow_early": shifts up to 55 bytes, then
    fragments whose final literal starts 25 bytes in, so the stash of each
    fragment's first bytes supplies what the left neighbour may have
    overwritten inside a final literal; "grow_short_tail*": a last
    fragment with a 1- or 2-byte tag moved); "grow_over" grows by 70 and is
    placed by the copy; "shrink_*": fragments 1 byte shorter than
    literals move left (the stash of each fragment's last bytes supplies what
    the right neighbour may have overwritten), "shrink_over" shrinks by 70
    and is placed by the copy."""
    import ctypes as C

    from parameter_server_amd._lib import check, lib
    payload = {
        "grow": lambda: _planted(12, [2, 3, 5, 8], 1),
        "grow_every": lambda: _planted(20, range(20), 2),
        "shrink_then_grow": lambda: _planted(14, [4, 5, 6, 7, 9], 3, zeros=[1]),
        "grow_then_shrink": lambda: _planted(14, [1, 2, 3, 4], 4, zeros=[8, 9]),
        "grow_tail": lambda: _planted(9, [0, 1, 2, 3, 4, 5, 6, 7], 5, tail=3000),
        "grow_early": lambda: _planted(62, range(0, 55), 6, early=range(55, 59)),
        "grow_over": lambda: _planted(72, range(0, 70), 7),
        "grow_short_tail1": lambda: _planted(4, [0, 1, 2], 8, tail=50),
        "grow_short_tail2": lambda: _planted(4, [1, 2, 3], 9, tail=200),
        "grow_one_last": lambda: _planted(6, [5], 10, tail=70000 - 65536),
        "shrink_small": lambda: _planted(20, [], 11, early=range(2, 12), tail=900),
        "shrink_grow_mixed": lambda: _planted(40, range(5, 35, 2), 12, early=[1, 2, 3, 36, 37], tail=64),
        "shrink_over": lambda: _planted(80, [], 13, early=range(0, 70)),
    }[case]()
    want = port.snappy_compress(payload)
    stored = _stored_layout(payload)
    if case.startswith("grow_") and case != "grow_then_shrink" or case == "grow":
        assert len(want) > len(stored), "the planted matches made no fragment longer"
    cap = lib().psf_snappy_stored_capacity(len(payload))
    buf = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    buf[:len(stored)] = torch.frombuffer(bytearray(stored), dtype=torch.uint8).cuda()
    out_len = C.c_size_t()
    check(lib().psf_snappy_compress_stored(ctx.h, C.c_void_p(buf.data_ptr()), len(payload), cap, C.byref(out_len)))
    got = buf[:out_len.value].cpu().numpy().tobytes()
    ok = got == want
    assert ok, (case, len(got), len(want))


def test_compress_stored_in_place_scan_path(ctx, port):
    """A stored-layout stream of 4100 fragments (offsets from the per-stream
    scan launch, more than kInlineScan) whose three matched fragments grow it
    by a few bytes: rewritten in place through K-scan's shift bounds
    (kPlaceShift), byte-identical to 1.1.8."""
    import ctypes as C

    from parameter_server_amd._lib import check, lib
    payload = _planted(4100, [3, 2000, 4090], 21, tail=777, early=[1000])
    want = port.snappy_compress(payload)
    stored = _stored_layout(payload)
    cap = lib().psf_snappy_stored_capacity(len(payload))
    buf = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    buf[:len(stored)] = torch.frombuffer(bytearray(stored), dtype=torch.uint8).cuda()
    out_len = C.c_size_t()
    check(lib().psf_snappy_compress_stored(ctx.h, C.c_void_p(buf.data_ptr()), len(payload), cap, C.byref(out_len)))
    got = buf[:out_len.value].cpu().numpy().tobytes()
    ok = got == want
    assert ok, (len(got), len(want))


def test_uncompress_tail_after_decoded_fast_path(ctx, port):
    """The uncompress's completion marker carries no system-scope fence, so the
    host may see it before the fast path's verdicts and launch the tail
    kernels for streams the fast path already decoded.  Forced here for every
    batch (psf_debug_force_snappy_tail): the tail must leave such streams as
    they are -- the fused FIXING_FLOAT decode of stored streams (with a
    compressible fragment, so one fragment sits off its assumed place) and the
    C ABI's single-stream uncompress of stored and tag-dense streams."""
    import ctypes as C
    from parameter_server_amd import lib
    from parameter_server_amd import filter as F
    L = lib()
    L.psf_debug_force_snappy_tail.argtypes = [C.c_int]
    L.psf_debug_force_snappy_tail.restype = C.c_int
    F.set_clock(SEED)
    assert L.psf_debug_force_snappy_tail(1) == 0
    try:
        cases = [("random", 6 * 65536 + 77, 1, np.float32), ("onecomp", 12 * 65536 + 333, 1, np.float32),
                 ("everyother", 9 * 65536 + 1234, 1, np.float32), ("random", 3 * 32768 + 2049, 2, np.float32)]
        xs = [_values(kind, n, dt, 900 + k, nb) for k, (kind, n, nb, dt) in enumerate(cases)]
        msgs = [_msg(F, x, c[2]) for x, c in zip(xs, cases)]
        snd = [F.RemoteNode(ctx) for _ in msgs]
        F.RemoteNode.encode_many(snd, msgs)
        ctx.sync()
        clones = [m.clone() for m in msgs]
        rcv = [F.RemoteNode(ctx) for _ in msgs]
        F.RemoteNode.decode_many(rcv, clones)
        ctx.sync()
        for x, c, m, w, r in zip(xs, cases, msgs, clones, rcv):
            stream, dec = _want(port, x, c[2])
            vp, vn, vl = m.value_ptr(0)
            assert F.copy_out(vp, vn, vl, "cuda:0").cpu().numpy().tobytes() == stream, c
            assert r.value(w, 0).cpu().numpy().tobytes() == dec, c
            # the single-stream C ABI path
            back = ctx.snappy_uncompress(torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda())
            st, codes, _, _ = port.ff_encode(x, c[2], SEED)
            assert back.cpu().numpy().tobytes() == codes.tobytes(), c
        keys = np.sort(np.random.default_rng(3).integers(0, 10**9, 300000, dtype=np.uint64)).tobytes()
        z = port.snappy_compress(keys)
        back = ctx.snappy_uncompress(torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda())
        assert back.cpu().numpy().tobytes() == keys
    finally:
        assert L.psf_debug_force_snappy_tail(0) == 0
        F.set_clock(None)

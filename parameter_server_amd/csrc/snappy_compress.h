// COMPRESSING, the compressor: snappy raw compress, byte-identical to snappy
// 1.1.8.  Three launches per batch of streams, no device-side waits.
//
// The parse of a 64 KiB fragment reads the table only at the positions it
// probes, and on data without 4-byte matches at those positions (FIXING_FLOAT
// codes, anything incompressible) 1.1.8's skip heuristic probes some 270
// positions and emits the whole fragment as one literal.  So:
//   K-parse  (snappy_parse) persistent workgroups of 12 waves, one per CU,
//            each over its stripe of the fragments in rounds of 12.  A round
//            first probes: every wave runs 1.1.8's skip loop on one fragment
//            exactly, 64 probes per step, reading the input where it probes
//            (no staging) and keeping the inserted positions in a small map
//            in LDS; a fragment whose loop ends without a match is stored
//            (one literal).  Then it parses the fragments that matched: the
//            full 1.1.8 parse, a wave per fragment (up to kParseWaves at a
//            time) reading the fragment from memory with its hash table in
//            LDS -- or, when the round has just one such fragment, that
//            fragment staged in LDS and parsed there by wave 0, its long
//            literals copied by the whole workgroup afterwards.  Tags go to
//            the fragment's scratch slot.  Nothing is loaded ahead for the
//            next round.
//   K-scan   (snappy_scan) one workgroup per stream: the stream offset of
//            every fragment (exclusive sum of the fragment lengths), the
//            varint header and the stream length (published to the host).
//            Launched only when a stream has more than kInlineScan
//            fragments; otherwise K-place's workgroups sum the lengths
//            themselves.
//   K-place  (snappy_place) one workgroup per fragment: its tags from scratch
//            and its final literal (all of a stored fragment) from the input
//            to their place.
// No workgroup ever waits for another: every dependency is a kernel boundary.
#pragma once

#include "snappy_common.h"

namespace psf {
namespace {

constexpr uint32_t kMaxTable = 16384;  // kMaxHashTableSize
constexpr uint32_t kMul = 0x1e35a7bdu;
__constant__ SkipCum kSkip = make_skip();  // (psf_internal.h)

__device__ __forceinline__ uint32_t hash(uint32_t v, int shift) { return (v * kMul) >> shift; }

// K-parse: kParseWaves waves per workgroup parse one fragment each, reading
// the fragment from memory (L1/L2) and keeping only the hash table and the
// skip loop's per-step slot words in LDS: 36 KiB per wave.
constexpr uint32_t kParseWaves = 4;
constexpr uint32_t kMinSlots = 1024;
static_assert((kParseWaves - 1) * kMaxTable * 2 >= kFrag + 16, "a staged fragment fits the other tables");
struct ParseLds {
  uint16_t table[kParseWaves][kMaxTable];  // (one fragment alone is staged in tables 1..3)
  uint32_t minlane[kParseWaves][kMinSlots + 1];  // per hash slot: lowest lane of the step that probed it (+ a spare)
};

template <uint32_t kLanes = 64>
__device__ uint32_t emit_literal(uint8_t* out, uint32_t op, const uint8_t* srcb, uint32_t lit,
                                 uint32_t len, uint32_t lane) {
  // (the tag as literal_tag writes it, spelled out: calling it here gives
  // other, if equivalent, code for K-parse)
  const uint32_t n = len - 1;
  uint32_t hl = 1;
  if (n < 60) {
    if (lane == 0) out[op] = (uint8_t)(n << 2);
  } else {
    const uint32_t count = ((31 - __builtin_clz(n)) >> 3) + 1;
    if (lane == 0) out[op] = (uint8_t)((59 + count) << 2);
    if (lane >= 1 && lane <= count) out[op + lane] = (uint8_t)(n >> (8 * (lane - 1)));
    hl += count;
  }
  // the literal bytes: byte stores up to the first aligned output position,
  // then whole dwords (16-byte chunks for long literals) composed from LDS
  // (ld32 reads unaligned), then the tail.  `out` is 16-byte aligned.
  const uint32_t d0 = op + hl, d1 = d0 + len;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(srcb);
  if (len >= 256) {
    const uint32_t a0 = (d0 + 15) & ~15u, a1 = d1 & ~15u;
    if (lane < a0 - d0) out[d0 + lane] = srcb[lit + lane];
    uint4* o16 = reinterpret_cast<uint4*>(out);
    for (uint32_t j = (a0 >> 4) + lane; j < (a1 >> 4); j += kLanes) {
      const uint32_t q = lit + (16 * j - d0);
      o16[j] = make_uint4(ld32(s32, q), ld32(s32, q + 4), ld32(s32, q + 8), ld32(s32, q + 12));
    }
    if (lane < d1 - a1) out[a1 + lane] = srcb[lit + (a1 - d0) + lane];
    return d1;
  }
  const uint32_t a0 = (d0 + 3) & ~3u, a1 = d1 & ~3u;
  if (a0 >= a1) {
    for (uint32_t i = lane; i < len; i += kLanes) out[d0 + i] = srcb[lit + i];
    return d1;
  }
  if (lane < a0 - d0) out[d0 + lane] = srcb[lit + lane];
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
  for (uint32_t j = (a0 >> 2) + lane; j < (a1 >> 2); j += kLanes) o32[j] = ld32(s32, lit + (4 * j - d0));
  if (lane < d1 - a1) out[a1 + lane] = srcb[lit + (a1 - d0) + lane];
  return d1;
}

__device__ __forceinline__ void put_copy2(uint8_t* out, uint32_t op, uint32_t offset, uint32_t len) {
  out[op] = (uint8_t)(2 + ((len - 1) << 2));
  out[op + 1] = (uint8_t)(offset & 0xff);
  out[op + 2] = (uint8_t)(offset >> 8);
}

// EmitCopy (1.1.8) by a wave.  (The lane comes first: with it last the
// compiler schedules two moves of the parse in the other order, and the
// kernels are kept bit for bit those that were measured.)
__device__ uint32_t emit_copy(uint32_t lane, uint8_t* out, uint32_t op, uint32_t offset, uint32_t len) {
  if (len >= 68) {  // while (len >= 68) { EmitCopyAtMost64(64); len -= 64; }
    const uint32_t q = (len - 68) / 64 + 1;
    for (uint32_t i = lane; i < q; i += 64) put_copy2(out, op + 3 * i, offset, 64);
    op += 3 * q;
    len -= 64 * q;
  }
  if (len > 64) {
    if (lane == 0) put_copy2(out, op, offset, 60);
    op += 3;
    len -= 60;
  }
  if (len < 12 && offset < 2048) {
    if (lane == 0) {
      out[op] = (uint8_t)(1 + ((len - 4) << 2) + ((offset >> 3) & 0xe0));
      out[op + 1] = (uint8_t)(offset & 0xff);
    }
    return op + 2;
  }
  if (lane == 0) put_copy2(out, op, offset, len);
  return op + 3;
}

// K-parse: 12 waves -- a round probes 12 fragments, so 2048 < n <= 3072
// fragments (C5 + COMPRESSING on a key cache miss: 2048 value + 128 key
// fragments) still take one round on 256 CUs; 12 waves of its 162 registers
// fit 3 per SIMD.  Staging a fragment uses the first kStageThreads.
constexpr uint32_t kCThreads = 768;
constexpr uint32_t kStageThreads = 512;

// Several streams compress in one launch chain (the COMPRESSING arrays of a
// batch of messages): fragments are numbered across the streams.
struct CJob {
  const uint8_t* in;  // the input; a stored job: the StoredLayout stream FIXING_FLOAT wrote
  uint8_t* dst;
  uint64_t n;
  uint32_t frag0, nfrag, hdr, slot, ticket, stored;  // stored: `in` is a StoredLayout stream
};
struct SnappyCJobs {
  CJob j[kSnappyBatchMax];
  PubSlot* pub;
  uint32_t njobs, nfrag;
  uint64_t* finfo;     // per fragment: op (tag bytes) << 32 | next_emit (start of the final literal)
  uint64_t* offset;    // per fragment: its offset in the stream (K-scan)
  uint32_t* in_place;  // per job (K-scan streams): a PlaceMode
  uint8_t* stash;      // per fragment of a stored job: its first and last kEdge bytes (K-parse's probe)
};
// How K-place treats a stream.  A stored job (FIXING_FLOAT wrote the stored
// layout) whose fragments all come out stored is the result as it stands.  If
// some carry tags and every fragment's new start lies within kShiftMax bytes
// of its stored one (the usual case on codes: a fragment with one 4-byte match
// comes out 2 bytes longer than a literal), the stream is rewritten in place:
// fragments before the first one with tags stay, each later one is moved by
// its own workgroup (tags from scratch, the final literal from where it lies).
// A workgroup's writes reach at most kShiftMax bytes into a neighbour's
// bytes -- the first ones of the next fragment (moved right) or the last ones
// of the previous (moved left) -- so K-parse's probe keeps every stored
// fragment's first and last kEdge bytes, and a moved fragment takes those
// from there.
// Otherwise the stream is placed into the job's dst.
enum PlaceMode : uint32_t { kPlaceCopy = 0, kPlaceStored = 1, kPlaceShift = 2 };
constexpr uint32_t kEdge = 64;
constexpr uint32_t kStash = 2 * kEdge;  // per fragment: its first kEdge bytes, then its last
constexpr int64_t kShiftMax = 64;
static_assert(kStoredSlack >= 64 + 64 + 8, "the stored stream's room for growth and the stash reads");
// fragment k's input bytes: consecutive 64 KiB blocks, or in a stored job the
// fragment's literal in the StoredLayout stream
__device__ __forceinline__ const uint8_t* frag_src(const CJob& c, uint32_t k) {
  if (!c.stored) return c.in + (size_t)k * kFrag;
  const StoredLayout L = stored_layout((uint32_t)c.n);
  return c.in + stored_frag_data(L, k);
}
__device__ __forceinline__ uint32_t cjob_index(const SnappyCJobs& J, uint32_t g) {
  uint32_t i = 0;
  while (i + 1 < J.njobs && g >= J.j[i + 1].frag0) ++i;
  return i;
}
__device__ __forceinline__ const CJob& cjob_of(const SnappyCJobs& J, uint32_t g) { return J.j[cjob_index(J, g)]; }
// bytes of the literal tag of a literal of m + 1 bytes, and of the fragment
__device__ __forceinline__ uint32_t lit_tag_len(uint32_t m) { return 1 + (m < 60 ? 0 : ((31 - __builtin_clz(m)) >> 3) + 1); }
__device__ __forceinline__ uint32_t frag_len(uint64_t info, uint32_t len) {
  const uint32_t op = (uint32_t)(info >> 32), ne = (uint32_t)info;
  return op + (ne < len ? lit_tag_len(len - ne - 1) + (len - ne) : 0);
}
__device__ __forceinline__ uint32_t hash_shift(uint32_t len) {
  uint32_t tsize = 256;
  while (tsize < kMaxTable && tsize < len) tsize <<= 1;
  return __builtin_clz(tsize) + 1;  // 32 - log2(tsize)
}

// ---- K-parse's probe
constexpr uint32_t kMapSlots = 1024;  // per wave: every inserted probe (<= 270) as {hash + 1, position, 4 bytes}
constexpr uint32_t kProbeMax = 6 * 64;  // probes a skip loop from ip = 1 can make in 64 KiB (< kSkipN)
// the 4 input bytes at p of a fragment starting at g (any alignment): one
// global_load_dword at the unaligned address -- gfx950 runs in unaligned mode,
// as the stored-layout code stores rely on (round 4 read two aligned dwords
// and shifted; the probe's ~270 scattered loads per fragment are bound by the
// texture unit's cache-line rate, so half the load instructions)
typedef uint32_t __attribute__((aligned(1))) u32u;
__device__ __forceinline__ uint32_t gld32(const uint8_t* g, uint32_t p) {
  return *gbl<u32u>(g + p);
}
// the table entry of hash h: 0 when never inserted (the table's initial 0)
__device__ __forceinline__ uint64_t map_get(const uint64_t* m, uint32_t h) {
  uint32_t s = h & (kMapSlots - 1);
  for (;;) {
    const uint64_t e = m[s];
    if (e == 0 || (uint32_t)(e >> 48) == h + 1) return e;
    s = (s + 1) & (kMapSlots - 1);
  }
}
// (no two lanes of a step insert the same hash)
__device__ __forceinline__ void map_put(uint64_t* m, uint32_t h, uint32_t pos, uint32_t v) {
  const uint64_t e = ((uint64_t)(h + 1) << 48) | ((uint64_t)pos << 32) | v;
  uint32_t s = h & (kMapSlots - 1);
  for (;;) {
    uint64_t cur = m[s];
    if (cur == 0) {
      cur = atomicCAS(reinterpret_cast<unsigned long long*>(&m[s]), 0ull, (unsigned long long)e);
      if (cur == 0) return;
    }
    if ((uint32_t)(cur >> 48) == h + 1) {
      m[s] = e;
      return;
    }
    s = (s + 1) & (kMapSlots - 1);
  }
}

// the probe's fast path: inserts the 4-byte value v into the set m (entries
// 1 << 32 | v); returns whether v was there already
__device__ __forceinline__ bool set_insert(uint64_t* m, uint32_t v) {
  const uint64_t e = (1ull << 32) | v;
  uint32_t s = (v * 0x9E3779B1u) >> 22;
  for (;;) {
    const uint64_t cur = atomicCAS(reinterpret_cast<unsigned long long*>(&m[s]), 0ull, (unsigned long long)e);
    if (cur == 0) return false;
    if (cur == e) return true;
    s = (s + 1) & (kMapSlots - 1);
  }
}

struct ProbeLds {  // the probe phase: per wave, the table as a map and every probe's bytes
  uint64_t map[kCThreads / 64][kMapSlots];
  uint32_t val[kCThreads / 64][kProbeMax];
};
union CompressPhaseLds {
  ParseLds p;
  ProbeLds q;
};

// A copy to 16-byte destination chunks from a source at any alignment, by W
// waves in rows of 63 chunks, U rows per wave at a time from chunk c0: lane l
// of wave wv loads the aligned source block under chunk l of its rows
// (load_rows; blocks from `lim` on hold no source byte) and takes each
// chunk's second block from the next lane (store_rows; chunks below nc).
typedef uint32_t V4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) V4* GblV4;
template <int U, uint32_t W>
__device__ __forceinline__ void load_rows(uint4 (&lo)[U], GblV4 s16, uint32_t c0, uint32_t wv, uint32_t lane,
                                          uint32_t lim) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = c0 + (u * W + wv) * 63 + lane;
    V4 x = {0, 0, 0, 0};
    if (c < lim) x = s16[c];
    lo[u] = make_uint4(x[0], x[1], x[2], x[3]);
  }
}
template <int U, uint32_t W>
__device__ __forceinline__ void store_rows(uint4* d16, const uint4 (&lo)[U], uint32_t c0, uint32_t wv, uint32_t lane,
                                           uint32_t nc, uint32_t sh) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = c0 + (u * W + wv) * 63 + lane;
    const uint4 hi = shfl_down1(lo[u]);
    if (lane < 63 && c < nc) d16[c] = funnel16(lo[u], hi, sh);
  }
}

// dst[0, len) = s[0, len) (global to global, any alignment of either) by T
// lanes (tid 0..T-1), in rows as above; a row's loads are all issued before
// its stores.
template <uint32_t T>
__device__ void copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ s, uint32_t len, uint32_t tid) {
  constexpr int U = 8;
  constexpr uint32_t W = T / 64;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  const uint32_t head = (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
  if (head >= len) {
    for (uint32_t i = tid; i < len; i += T) dst[i] = s[i];
    return;
  }
  if (tid < head) dst[tid] = s[tid];
  const uint32_t nc = (len - head) >> 4;
  const uintptr_t sp = reinterpret_cast<uintptr_t>(s + head);
  const GblV4 s16 = gbl<V4>(reinterpret_cast<const void*>(sp & ~(uintptr_t)15));  // global, not flat, loads
  const uint32_t sh = (uint32_t)(sp & 15);
  const uint32_t lim = nc + (sh ? 1u : 0u);  // blocks that hold source bytes
  uint4* d16 = reinterpret_cast<uint4*>(dst + head);
  for (uint32_t c0 = 0; c0 < nc; c0 += U * W * 63) {
    uint4 lo[U];
    load_rows<U, W>(lo, s16, c0, wv, lane, lim);
    store_rows<U, W>(d16, lo, c0, wv, lane, nc, sh);
  }
  const uint32_t t0 = head + 16 * nc;
  for (uint32_t i = tid; i < len - t0; i += T) dst[t0 + i] = s[t0 + i];
}

// One wave probes one fragment.  From ip = 1 the skip loop's probe positions
// are fixed (1 + kSkip[k]) until it matches, so all of their 4-byte values are
// loaded at once; the candidate a probe compares with is a position an
// earlier probe inserted (its bytes are already here) or the table's initial
// 0 (the fragment's first 4 bytes).  The loop then runs in LDS and registers,
// 64 probes per step, with exactly the full parse's rules: lanes up to the
// first one whose hash an earlier lane of the step also has see the table as
// it was, that lane sees the earlier lane's insert; later lanes wait for the
// next step.  Returns whether the loop ends without a match (one literal).
__device__ __forceinline__ bool probe_stored(const uint8_t* g, uint32_t len, const uint32_t* skip, uint64_t* m, uint32_t* pv,
                             uint32_t lane) {
  if (len < 15) return true;
  const uint32_t shift = hash_shift(len), ip_limit = len - 15, ip = 1;
  // every probe's bytes (probe k is made iff ip + skip[k + 1] <= ip_limit)
  uint32_t pre[kProbeMax / 64], vbits = 0;
#pragma unroll
  for (uint32_t r = 0; r < kProbeMax / 64; ++r) {
    const uint32_t k = r * 64 + lane;
    const bool valid = ip + skip[k + 1] <= ip_limit;
    pre[r] = valid ? gld32(g, ip + skip[k]) : 0;
    vbits |= (valid ? 1u : 0u) << r;
  }
  const uint32_t v_at0 = uni(gld32(g, 0));
  for (uint32_t i = lane; i < kMapSlots; i += 64) m[i] = 0;
#pragma unroll
  for (uint32_t r = 0; r < kProbeMax / 64; ++r) pv[r * 64 + lane] = pre[r];
  // Fast path: a probe matches only a candidate with its own 4 bytes, and
  // every candidate is position 0 or an earlier probe; when the first 4 bytes
  // and all probes' 4 bytes are distinct the loop ends without a match.
  {
    bool dup = false;
    if (lane == 0) set_insert(m, v_at0);
#pragma unroll
    for (uint32_t r = 0; r < kProbeMax / 64; ++r)
      if ((vbits >> r) & 1) dup |= set_insert(m, pre[r]);
    if (!__ballot(dup)) return true;
    for (uint32_t i = lane; i < kMapSlots; i += 64) m[i] = 0;  // the exact loop below
  }
  for (uint32_t kbase = 0;;) {
    const uint32_t k = kbase + lane;
    const uint32_t pos = ip + skip[k];
    const bool valid = ip + skip[k + 1] <= ip_limit;  // else "goto emit_remainder"
    const uint32_t v = valid ? pv[k] : 0;
    const uint32_t h = valid ? hash(v, shift) : 0;
    const uint64_t vm = __ballot(valid);
    uint64_t eq = vm;  // the valid lanes whose hash equals this lane's (14 bits)
#pragma unroll
    for (int b = 0; b < 14; ++b) {
      const bool bit = (h >> b) & 1;
      const uint64_t bm = __ballot(bit);
      eq &= bit ? bm : ~bm;
    }
    const uint32_t first = valid ? (uint32_t)__builtin_ctzll(eq) : lane;
    const uint64_t em = __ballot(valid && first < lane);
    int limit = 63, jc = 64, jm = 0;
    if (em) {
      jc = __builtin_ctzll(em);
      jm = (int)__builtin_amdgcn_readlane(first, jc);
      limit = jc;
    }
    uint32_t cv = v_at0;  // the candidate's 4 bytes
    if (valid && (int)lane <= limit) {
      const uint64_t e = map_get(m, h);
      if (e) cv = (uint32_t)e;
    }
    const uint32_t vjm = __builtin_amdgcn_readlane(v, jm & 63);
    if (em && (int)lane == jc) cv = vjm;  // lane jm's insert
    if (__ballot(valid && (int)lane <= limit && v == cv)) return false;  // a match
    // no match up to `limit`: every probe up to it inserts its position
    // (jm's insert is overwritten by jc's, same hash)
    if (valid && (int)lane <= limit && !(em && (int)lane == jm)) map_put(m, h, pos, v);
    const uint64_t lim_mask = limit >= 63 ? ~0ull : ((1ull << (limit + 1)) - 1);
    if ((vm & lim_mask) != lim_mask) return true;  // emit_remainder: one literal
    kbase += (uint32_t)limit + 1;
  }
}

// The 4 bytes at p of the fragment g[0, len) (len >= 15), without reading a
// dword that holds no byte of g[0, len): past len - 4 the word is the last
// one shifted right (its low byte is still the byte at p); p >= len reads as
// len - 1.
__device__ __forceinline__ uint32_t gw32(const uint8_t* g, uint32_t p, uint32_t len) {
  p = p < len ? p : len - 1;
  const uint32_t q = p < len - 4 ? p : len - 4;
  return gld32(g, q) >> (8 * (p - q));
}
// the same from a fragment staged in LDS (16 zero bytes after it)
__device__ __forceinline__ uint32_t ldc(const uint32_t* s, uint32_t p, uint32_t len) {
  return ld32(s, p < len ? p : len);
}
// the parse's source: the fragment in memory (g) or staged in LDS (s)
template <bool kLds>
__device__ __forceinline__ uint32_t srcw(const uint8_t* g, const uint32_t* s, uint32_t p, uint32_t len) {
  return kLds ? ldc(s, p, len) : gw32(g, p, len);
}

// The literal g[lit, lit + len) at op: for len <= 60 one tag byte (lane 0)
// and the bytes (lanes 1..len), one store instruction; else the tag and a
// wave copy.
// kDefer: the staged single-fragment parse hands literals longer than
// kDeferMin to the whole workgroup (defer[0] entries of {out offset of the
// bytes, lit, len} after it), copied from the fragment in memory after the
// parse, instead of one wave's 16-byte stores; a full list falls back to them.
constexpr uint32_t kDeferMax = 8, kDeferMin = 1024;
template <bool kLds>
__device__ __forceinline__ uint32_t emit_lit(uint8_t* out, uint32_t op, const uint8_t* g, const uint32_t* s,
                                             uint32_t glen, uint32_t lit, uint32_t len, uint32_t lane,
                                             uint32_t* defer = nullptr) {
  if (len <= 60) {
    uint32_t i = lit + (lane ? lane - 1 : 0);
    i = i < glen ? i : glen - 1;
    const uint8_t b = kLds ? reinterpret_cast<const uint8_t*>(s)[i] : gbl<uint8_t>(g)[i];
    if (lane <= len) out[op + lane] = lane ? b : (uint8_t)((len - 1) << 2);
    return op + 1 + len;
  }
  // a staged fragment: 16-byte stores composed from LDS (a wave issues them
  // back to back); from memory: the wave copy (loads before stores)
  if (kLds && defer && len >= kDeferMin && defer[0] < kDeferMax) {
    const uint32_t hl = literal_tag(out + op, len, lane);
    const uint32_t n = defer[0];
    if (lane == 0) {
      defer[1 + 3 * n] = op + hl;
      defer[2 + 3 * n] = lit;
      defer[3 + 3 * n] = len;
      defer[0] = n + 1;
    }
    return op + hl + len;
  }
  if (kLds) return emit_literal(out, op, reinterpret_cast<const uint8_t*>(s), lit, len, lane);
  const uint32_t hl = literal_tag(out + op, len, lane);
  copy_bytes<64>(out + op + hl, g + lit, len, lane);
  return op + hl + len;
}
// The literal of len <= 4 bytes that starts where a copy ended, whose bytes
// are the low ones of cur (the 4 bytes there, already in a register): no
// load on the parse's chain before the store (emit_lit would read them back
// from the fragment first, and the store waits for that read)
__device__ __forceinline__ uint32_t emit_short_lit(uint8_t* out, uint32_t op, uint32_t cur, uint32_t len,
                                                   uint32_t lane) {
  const uint8_t b = lane ? (uint8_t)(cur >> (8 * ((lane - 1) & 3))) : (uint8_t)((len - 1) << 2);
  if (lane <= len) out[op + lane] = b;
  return op + 1 + len;
}
// EmitCopy (1.1.8) of a copy that fits one tag, one store instruction; the
// rest go to emit_copy
__device__ __forceinline__ uint32_t emit_copy_fast(uint8_t* out, uint32_t op, uint32_t offset, uint32_t len,
                                                   uint32_t lane) {
  if (len < 12 && offset < 2048) {  // COPY_1_BYTE_OFFSET
    const uint8_t b = lane ? (uint8_t)offset : (uint8_t)(1 + ((len - 4) << 2) + ((offset >> 3) & 0xe0));
    if (lane < 2) out[op + lane] = b;
    return op + 2;
  }
  if (len <= 64) {  // COPY_2_BYTE_OFFSET
    const uint8_t b = lane ? (uint8_t)(offset >> (8 * (lane - 1))) : (uint8_t)(2 + ((len - 1) << 2));
    if (lane < 3) out[op + lane] = b;
    return op + 3;
  }
  return emit_copy(lane, out, op, offset, len);
}

// The exact 1.1.8 parse of one fragment g[0, len) by one wave (CompressFragment,
// snappy.cc): tags to out, returns {tag bytes, start of the final literal}.
// The fragment is read from memory (what the probe touched is in L1 / L2); the
// hash table and the skip loop's slot words are the wave's own LDS.  One wave
// issues about one vector instruction per 4 cycles, so the parse is bound by
// its instruction count and its dependent reads per tag; the common paths are
// short:
//  * copies: each lane holds the 4 bytes at ip + off + lane and at
//    cand + off + lane, so one round of reads gives 64 bytes of the match
//    length, and the bytes at the new ip - 1, ip and ip + 1 come from the
//    lanes where the match ended;
//  * after a copy, the table updates, the check whether ip matches at once
//    and the skip loop's first probe (at ip + 1, which sees those updates)
//    are issued together, with the first round of the next copy's match
//    length for both outcomes;
//  * otherwise the skip loop runs 64 probes per step (positions ip + kSkip[k];
//    the first two steps' offsets sit in registers), every probe's hash slot,
//    candidate and the slot's lowest probing lane read together; a lane whose
//    earlier same-hash lane inserted this step compares with that lane's
//    bytes; lanes past the first lane with an earlier lane in its slot wait
//    for the next step (as in probe_stored).
template <bool kLds>
__device__ __forceinline__ uint2 parse_fragment(uint16_t* __restrict__ table, uint32_t* __restrict__ minlane,
                                                const uint32_t* skip, uint32_t skA, uint32_t skB, uint32_t skC,
                                                const uint8_t* __restrict__ g, const uint32_t* s, uint32_t len,
                                                uint8_t* __restrict__ out, uint32_t lane, uint32_t* defer) {
  uint32_t op = 0, next_emit = 0;
  if (len < 15) return make_uint2(0, 0);
  const uint32_t shift = hash_shift(len), ip_limit = len - 15;
  uint32_t ip = 1, kbase = 0;  // the skip loop from ip, at its probe kbase
  for (;;) {
    // ---- skip loop steps (loading the next step's probe bytes ahead
    // measured slower: 16.6 against 15.9 ms for 128 MiB of sorted keys)
    uint32_t cand;
    for (;;) {
      const uint32_t k = kbase + lane;
      const uint32_t o0 = kbase == 0 ? skA : kbase == 1 ? skB : kbase == 2 ? skC : skip[k];
      const uint32_t o1 = kbase == 0 ? skB : kbase == 1 ? skC : skip[k + 1];
      const bool valid = ip + o1 <= ip_limit;  // else "goto emit_remainder"
      const uint32_t pos = ip + o0;
      const uint32_t v = srcw<kLds>(g, s, pos, len);
      const uint32_t h = hash(v, shift);
      const uint32_t slot = valid ? (h & (kMinSlots - 1)) : kMinSlots;  // invalid lanes: the spare slot
      const uint32_t c = table[h];
      atomicMin(&minlane[slot], lane);
      asm volatile("" ::: "memory");
      const uint32_t fl = minlane[slot];
      asm volatile("" ::: "memory");
      minlane[slot] = 0xffffffffu;  // clean for the next step
      const uint32_t wc = srcw<kLds>(g, s, c, len);
      const uint32_t first = valid ? fl : lane;
      const uint64_t vm = __ballot(valid);
      const uint64_t em = __ballot(valid && first < lane);
      int limit = 63, jc = 64, jm = 0;
      bool exact_pair = false;
      if (em) {
        jc = __builtin_ctzll(em);
        jm = (int)lane_of(first, jc);
        exact_pair = lane_of(h, jm) == lane_of(h, jc);
        limit = jc;
      }
      const uint32_t vjm = lane_of(v, jm);
      const bool pair = exact_pair && (int)lane == jc;  // sees lane jm's insert: compares with its bytes
      const bool m = valid && (int)lane <= limit && v == (pair ? vjm : wc);
      const uint64_t mm = __ballot(m);
      const int last = mm ? __builtin_ctzll(mm) : limit;
      const bool overwritten = exact_pair && (int)lane == jm && jc <= last;
      if (valid && (int)lane <= last && !overwritten) table[h] = (uint16_t)pos;
      if (mm) {
        const int ks = __builtin_ctzll(mm);
        cand = (exact_pair && ks == jc) ? lane_of(pos, jm) : lane_of(c, ks);
        ip = lane_of(pos, ks);
        break;
      }
      const uint64_t lim_mask = limit >= 63 ? ~0ull : ((1ull << (limit + 1)) - 1);
      if ((vm & lim_mask) != lim_mask) goto remainder;
      kbase += (uint32_t)limit + 1;
    }
    op = emit_lit<kLds>(out, op, g, s, len, next_emit, ip - next_emit, lane, defer);
    // ---- copies
    {
      uint32_t off = 3, wa = 0, wb = 0;  // lane 0 of the first round: byte ip + 3 (known equal)
      bool have = false;
      for (;;) {
        uint32_t k;
        for (;;) {
          const uint32_t pb = ip + off + lane;
          if (!have) {
            wb = srcw<kLds>(g, s, pb, len);
            wa = srcw<kLds>(g, s, cand + off + lane, len);
          }
          have = false;
          const uint64_t bad = __ballot(pb >= len || ((wa ^ wb) & 0xffu) != 0);
          if (bad) {
            k = (uint32_t)__builtin_ctzll(bad);  // >= 1: lane 0 is a byte known equal
            break;
          }
          off += 63;  // the next round's lane 0 is this round's lane 63
        }
        const uint32_t prev = lane_of(wb, k - 1), cur = lane_of(wb, k);
        uint32_t nxt = lane_of(wb, k < 63 ? k + 1 : 63);
        uint32_t nxt2 = lane_of(wb, k < 62 ? k + 2 : 63);
        op = emit_copy_fast(out, op, ip - cand, off + k, lane);
        ip += off + k;
        next_emit = ip;
        if (ip >= ip_limit) goto remainder;
        if (k == 63) nxt = uni(srcw<kLds>(g, s, ip + 1, len));
        if (k >= 62) nxt2 = uni(srcw<kLds>(g, s, ip + 2, len));
        const uint32_t hp = hash(prev, shift), hc = hash(cur, shift), hn = hash(nxt, shift), h2 = hash(nxt2, shift);
        if (lane == 0) table[hp] = (uint16_t)(ip - 1);
        const uint32_t c = table[hc];
        if (lane == 0) table[hc] = (uint16_t)ip;
        const uint32_t c1 = table[hn];  // the skip loop's probe 0 at ip + 1, if ip does not match
        const uint32_t c2 = table[h2];  // its probe 1 at ip + 2 (probe 0's insert aside)
        wb = srcw<kLds>(g, s, ip + lane, len);
        const uint32_t wb1 = srcw<kLds>(g, s, ip + 1 + lane, len);
        const uint32_t wb2 = srcw<kLds>(g, s, ip + 2 + lane, len);
        wa = srcw<kLds>(g, s, c + lane, len);
        const uint32_t wa1 = srcw<kLds>(g, s, c1 + lane, len);
        const uint32_t wa2 = srcw<kLds>(g, s, c2 + lane, len);
        if (lane_of(wa, 0) == cur) {  // a copy from ip at once; its first round is loaded
          cand = uni(c);
          off = 0;
          have = true;
          continue;
        }
        ip += 1;  // the skip loop from ip + 1: probe 0 is made iff ip + 1 <= ip_limit
        if (ip + 1 > ip_limit) goto remainder;
        if (lane == 0) table[hn] = (uint16_t)ip;
        if (lane_of(wa1, 0) == nxt) {  // probe 0 matches: a one-byte literal, then a copy
          cand = uni(c1);
          op = emit_short_lit(out, op, cur, 1, lane);
          wa = wa1;
          wb = wb1;
          off = 0;
          have = true;
          continue;
        }
        // probe 1 at ip + 1, made iff ip + 2 <= ip_limit; it sees probe 0's
        // insert when the hashes agree (its candidate then ip, whose bytes
        // are nxt).  On sorted keys nearly every skip loop after a copy ends
        // here (tools/bench_snappy.py --only sorted_keys_1e9, with counters
        // in the parse that are no longer in the tree: 6346 of 6395 skip
        // steps per fragment matched at probe 1), so the 64-probe step is
        // skipped.
        if (ip + 2 > ip_limit) goto remainder;
        {
          const bool same = h2 == hn;
          const uint32_t c2v = same ? ip : c2;
          if (lane == 0) table[h2] = (uint16_t)(ip + 1);
          if ((same ? nxt : lane_of(wa2, 0)) == nxt2) {  // a two-byte literal, then a copy
            cand = uni(c2v);
            op = emit_short_lit(out, op, cur, 2, lane);
            ip += 1;
            wa = same ? wb1 : wa2;
            wb = wb2;
            off = 0;
            have = true;
            continue;
          }
        }
        kbase = 2;
        break;
      }
    }
  }
remainder:
  return make_uint2(op, next_emit);
}

// LDS src[0, len) = g[0, len) (g 16-byte aligned) by T lanes: a full
// fragment's loads are all issued before its LDS stores (one memory latency
// per fragment instead of one per T x 16 bytes: 12 -> 2 us for 512 lanes);
// the lane's share is one vector value (an array of uint4 would live in
// scratch memory)
template <uint32_t T>
__device__ __forceinline__ void stage_frag(const uint8_t* __restrict__ g, uint32_t len, uint32_t* src, uint32_t tid) {
  constexpr uint32_t U = kFrag / 16 / T;
  typedef uint32_t Share __attribute__((ext_vector_type(4 * U)));
  const uint4* g4 = reinterpret_cast<const uint4*>(g);
  uint4* s4 = reinterpret_cast<uint4*>(src);
  if (len == kFrag) {
    Share v;
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint4 x = g4[u * T + tid];
      v[4 * u] = x.x;
      v[4 * u + 1] = x.y;
      v[4 * u + 2] = x.z;
      v[4 * u + 3] = x.w;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) s4[u * T + tid] = make_uint4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
    return;
  }
  const uint32_t nv = len >> 4;
  for (uint32_t i = tid; i < nv; i += T) s4[i] = g4[i];
  uint8_t* srcb = reinterpret_cast<uint8_t*>(src);
  if (tid < len - (nv << 4)) srcb[(nv << 4) + tid] = g[(nv << 4) + tid];
}

// the same for a fragment at any alignment (a stored job's literal sits at
// hdr + 65539 k + 3): each lane composes its 16-byte LDS blocks from two
// aligned source blocks (the stored stream is allocated with 64 bytes to
// spare); bytes past len are zero
template <uint32_t T>
__device__ __forceinline__ void stage_frag_shifted(const uint8_t* __restrict__ g, uint32_t len, uint32_t* src,
                                                   uint32_t tid) {
  typedef uint32_t V4 __attribute__((ext_vector_type(4)));
  const uintptr_t a = reinterpret_cast<uintptr_t>(g);
  const uint32_t sh = (uint32_t)(a & 15);
  const auto s16 = gbl<V4>(reinterpret_cast<const void*>(a & ~(uintptr_t)15));
  uint4* d4 = reinterpret_cast<uint4*>(src);
  const uint32_t nb = (len + 15) >> 4;
  constexpr uint32_t U = kFrag / 16 / T;
  for (uint32_t i0 = 0; i0 < nb; i0 += U * T) {
    V4 lo[U], hi[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t i = i0 + u * T + tid;
      if (i < nb) {
        lo[u] = s16[i];
        hi[u] = s16[i + 1];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t i = i0 + u * T + tid;
      if (i >= nb) continue;
      uint4 w = funnel16(make_uint4(lo[u][0], lo[u][1], lo[u][2], lo[u][3]),
                         make_uint4(hi[u][0], hi[u][1], hi[u][2], hi[u][3]), sh);
      if (16 * i + 16 > len) {  // the block holding the end: zero past len
        const uint32_t keep = len - 16 * i;  // 1..15
        uint32_t* wp = reinterpret_cast<uint32_t*>(&w);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t kb = keep > 4 * q ? (keep - 4 * q < 4 ? keep - 4 * q : 4) : 0;
          wp[q] &= kb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * kb)) - 1u);
        }
      }
      d4[i] = w;
    }
  }
}

// K-parse: persistent workgroups of 12 waves, each over its stripe of the
// fragments (b, b + G, b + 2G, ...) in rounds of 12: every wave probes one
// fragment; then the fragments that matched are parsed by waves
// 0..kParseWaves-1, one fragment per wave at a time (tags to the fragment's
// scratch slot).  No workgroup depends on another.
__global__ __launch_bounds__(kCThreads) void snappy_parse(const SnappyCJobs J, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t skip[kSkipN + 3];
  __shared__ CompressPhaseLds U;
  __shared__ uint32_t s_need[kCThreads / 64];
  __shared__ uint32_t s_defer[1 + 3 * kDeferMax];
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6, lane = tid & 63;
  constexpr uint32_t W = kCThreads / 64;
  for (uint32_t i = tid; i < (uint32_t)kSkipN; i += kCThreads) skip[i] = kSkip.v[i];
  const uint32_t sk0 = kSkip.v[lane], sk1 = kSkip.v[lane + 1], sk2 = kSkip.v[lane + 2];  // the first skip steps' offsets
  __syncthreads();
  const uint32_t G = gridDim.x;
  for (uint32_t r0 = 0; (size_t)r0 * G + blockIdx.x < J.nfrag; r0 += W) {
    // ---- probe: wave w takes fragment (r0 + w) G + b
    {
      const uint32_t f = (r0 + wave) * G + blockIdx.x;
      bool need = false;
      if (f < J.nfrag) {
        PSF_TRACE_T(f, 0, wave * 64);
        const CJob& c = cjob_of(J, f);
        const size_t start = (size_t)(f - c.frag0) * kFrag;
        const uint32_t len = (uint32_t)min((size_t)kFrag, c.n - start);
        const uint8_t* g = frag_src(c, f - c.frag0);
        // a stored job's fragment may be moved in place by K-place, whose
        // neighbours can overwrite its first or last bytes before it reads
        // them: keep them (reads past a short last fragment stay inside the
        // stream's kStoredSlack)
        if (c.stored && (lane < kEdge / 4 || (lane < kStash / 4 && len >= kEdge))) {
          const uint32_t p = lane < kEdge / 4 ? 4 * lane : len - kStash + 4 * lane;
          reinterpret_cast<uint32_t*>(J.stash + (size_t)f * kStash)[lane] = gld32(g, p);
        }
        need = !probe_stored(g, len, skip, U.q.map[wave], U.q.val[wave], lane);
        if (!need && lane == 0) J.finfo[f] = 0;  // no tags, the final literal from byte 0
        PSF_TRACE_T(f, 4, wave * 64);
      }
      if (lane == 0) s_need[wave] = need;
    }
    __syncthreads();
    uint32_t need = 0;
    for (uint32_t w = 0; w < W; ++w) need |= s_need[w] << w;
    __syncthreads();  // (the probe maps are overwritten by the parses)
    if (!need) continue;
    // ---- parse.  One fragment (data with few matches: a fragment of
    // FIXING_FLOAT codes now and then): staged in LDS where the other
    // tables would be and parsed there by wave 0.  More: wave p < kParseWaves
    // takes the matched fragments p, p + kParseWaves, ... from memory.
    if (wave < kParseWaves)
      for (uint32_t i = lane; i <= kMinSlots; i += 64) U.p.minlane[wave][i] = 0xffffffffu;  // each step cleans up after itself
    if (__builtin_popcount(need) == 1) {
      const uint32_t f = (r0 + __builtin_ctz(need)) * G + blockIdx.x;
      if (tid == 0) s_defer[0] = 0;
      const CJob& c = cjob_of(J, f);
      const size_t start = (size_t)(f - c.frag0) * kFrag;
      const uint32_t len = (uint32_t)min((size_t)kFrag, c.n - start);
      const uint8_t* g = frag_src(c, f - c.frag0);
      uint32_t* src = reinterpret_cast<uint32_t*>(U.p.table[1]);  // tables 1..3: 96 KiB
      uint8_t* srcb = reinterpret_cast<uint8_t*>(src);
      if (aligned16(g)) {
        if (tid < kStageThreads) stage_frag<kStageThreads>(g, len, src, tid);
      } else if (c.stored) {
        if (tid < kStageThreads) stage_frag_shifted<kStageThreads>(g, len, src, tid);
      } else {
        for (uint32_t i = tid; i < len; i += kCThreads) srcb[i] = g[i];
      }
      if (tid < 16) srcb[len + tid] = 0;
      uint4* t16 = reinterpret_cast<uint4*>(U.p.table[0]);
      for (uint32_t j = tid; j < (1u << (32 - hash_shift(len))) / 8; j += kCThreads) t16[j] = make_uint4(0, 0, 0, 0);
      __syncthreads();
      if (wave == 0) {
        const uint2 r = parse_fragment<true>(U.p.table[0], U.p.minlane[0], skip, sk0, sk1, sk2, g, src, len,
                                             scratch + (size_t)f * kSnappyFragOut, lane, s_defer);
        if (lane == 0) J.finfo[f] = ((uint64_t)r.x << 32) | r.y;
        PSF_TRACE(f, 1);
      }
    } else if (wave < kParseWaves) {
      uint16_t* table = U.p.table[wave];
      uint32_t* minlane = U.p.minlane[wave];
      uint32_t m = need;
      for (uint32_t i = 0; m; ++i) {
        const uint32_t w = __builtin_ctz(m);
        m &= m - 1;
        if (i % kParseWaves != wave) continue;
        const uint32_t f = (r0 + w) * G + blockIdx.x;
        const CJob& c = cjob_of(J, f);
        const size_t start = (size_t)(f - c.frag0) * kFrag;
        const uint32_t len = (uint32_t)min((size_t)kFrag, c.n - start);
        uint4* t16 = reinterpret_cast<uint4*>(table);
        for (uint32_t j = lane; j < (1u << (32 - hash_shift(len))) / 8; j += 64) t16[j] = make_uint4(0, 0, 0, 0);
        asm volatile("" ::: "memory");
        const uint2 r = parse_fragment<false>(table, minlane, skip, sk0, sk1, sk2, frag_src(c, f - c.frag0), nullptr, len,
                                              scratch + (size_t)f * kSnappyFragOut, lane, nullptr);
        if (lane == 0) J.finfo[f] = ((uint64_t)r.x << 32) | r.y;
        PSF_TRACE_T(f, 1, wave * 64);
      }
    }
    __syncthreads();  // (the next round's probe maps overwrite the tables)
    if (__builtin_popcount(need) == 1 && s_defer[0]) {  // the long literals it handed over
      const uint32_t f = (r0 + __builtin_ctz(need)) * G + blockIdx.x;
      const CJob& c = cjob_of(J, f);
      const uint8_t* g = frag_src(c, f - c.frag0);
      uint8_t* out = scratch + (size_t)f * kSnappyFragOut;
      for (uint32_t d = 0; d < s_defer[0]; ++d)
        copy_bytes<kCThreads>(out + s_defer[1 + 3 * d], g + s_defer[2 + 3 * d], s_defer[3 + 3 * d], tid);
      __syncthreads();  // (s_defer is reset by the next single parse)
    }
  }
}

// ---- K-scan: one workgroup per stream.  Fragment offsets = the varint
// header + the exclusive sum of the fragment lengths; the stream length is
// published to the host (the bytes are in place once K-place has run).
constexpr uint32_t kScanT = 1024;
// how far fragment k's new start lies after its stored one (a stored job)
__device__ __forceinline__ int64_t stored_shift(const CJob& c, uint32_t k, uint64_t off) {
  return (int64_t)off - (int64_t)stored_frag_tag(stored_layout((uint32_t)c.n), k);
}
__global__ __launch_bounds__(kScanT) void snappy_scan(const SnappyCJobs J) {
  __shared__ uint64_t wsum[kScanT / 64];
  __shared__ uint64_t s_base;
  __shared__ uint32_t s_any;
  __shared__ int64_t s_lo[kScanT / 64], s_hi[kScanT / 64];
  const CJob& c = J.j[blockIdx.x];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid == 0) {
    s_base = c.hdr;
    s_any = 0;
  }
  __syncthreads();
  uint32_t any = 0;  // a fragment with tags (not stored from byte 0)
  for (uint32_t k = tid; k < c.nfrag; k += kScanT) any |= J.finfo[c.frag0 + k] != 0 ? 1u : 0u;
  if (any) s_any = 1;
  __syncthreads();
  int64_t lo = 0, hi = 0;  // the fragments' shifts (kPlaceShift's bounds)
  for (uint32_t k0 = 0; k0 < c.nfrag; k0 += kScanT) {
    const uint32_t k = k0 + tid;
    uint64_t v = 0;
    if (k < c.nfrag) {
      const size_t start = (size_t)k * kFrag;
      const uint64_t info = J.finfo[c.frag0 + k];
      v = frag_len(info, (uint32_t)min((size_t)kFrag, c.n - start));
    }
    uint64_t x = v;  // inclusive scan in the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o, 64);
      if ((int)lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint64_t before = s_base;
    for (uint32_t q = 0; q < wave; ++q) before += wsum[q];
    if (k < c.nfrag) {
      J.offset[c.frag0 + k] = before + x - v;
      if (c.stored) {
        const int64_t d = stored_shift(c, k, before + x - v);
        lo = min(lo, d);
        hi = max(hi, d);
      }
    }
    __syncthreads();
    if (tid == kScanT - 1) s_base = before + x;
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, (int64_t)__shfl_xor(lo, o, 64));
    hi = max(hi, (int64_t)__shfl_xor(hi, o, 64));
  }
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  for (uint32_t w = 0; w < kScanT / 64; ++w) {
    lo = min(lo, s_lo[w]);
    hi = max(hi, s_hi[w]);
  }
  // (the stream's end: its growth must fit the stored stream's slack)
  const int64_t grow = c.stored ? (int64_t)s_base - (int64_t)stored_stream_bytes(stored_layout((uint32_t)c.n)) : 0;
  const uint32_t mode = !c.stored ? kPlaceCopy
                        : !s_any  ? kPlaceStored
                        : (lo >= -kShiftMax && hi <= kShiftMax && grow <= kShiftMax) ? kPlaceShift
                                                                                        : kPlaceCopy;
  if (tid == 0) J.in_place[blockIdx.x] = mode;
  if (mode == kPlaceCopy && tid < c.hdr) c.dst[tid] = (uint8_t)(((uint32_t)c.n >> (7 * tid)) | (tid + 1 < c.hdr ? 128u : 0u));
  if (tid == 0 && J.pub) {
    PubSlot* pub = J.pub + c.slot;
    pub_store(&pub->size, (uint64_t)s_base);
    pub_store(&pub->status, (int32_t)kOk);
    pub_store(&pub->pad, mode != kPlaceCopy ? (uint32_t)kStoredInPlace : 0u);
    publish_ticket(pub, c.ticket);
  }
}

// ---- K-place: one workgroup of 256 per fragment
constexpr uint32_t kPlaceT = 256;  // (512: C5 + COMPRESSING 1377 -> 1364, 1024: 1281 GiB/s)
constexpr int kMoveRows = 6;  // rows of 63 16-byte chunks per wave and pass (58 VGPRs: 8 waves per SIMD)
constexpr uint32_t kMovePass = kMoveRows * (kPlaceT / 64) * 63;  // chunks per pass (23.6 KiB)

// A fragment rewritten in place (kPlaceShift): at d its op tag bytes from tg,
// then the literal tag and the literal s[0, lit), which moves by D = (its new
// place - s), |D| small.  The literal goes in passes of kMovePass 16-byte
// destination chunks (lane l of a wave loads the aligned block under chunk l
// of its row of 63, as copy_bytes), each pass loaded whole before the
// workgroup's barrier and stored after it; the passes run from the end when
// D > 0 (a pass's stores then land only on bytes already read) and from the
// start when D < 0.  The tags, which may cover the literal's first D bytes,
// are stored last.
__device__ void place_moved(uint8_t* d, const uint8_t* tg, uint32_t op, const uint8_t* s, uint32_t lit, uint32_t tid) {
  constexpr uint32_t W = kPlaceT / 64;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  uint8_t* dl = d + op + (lit ? lit_tag_len(lit - 1) : 0);
  const bool right = dl >= s;
  const uint32_t head = min(lit, (uint32_t)(-reinterpret_cast<uintptr_t>(dl) & 15));
  const uint32_t nc = (lit - head) >> 4;
  const uint32_t t0 = head + 16 * nc;
  const uintptr_t sp = reinterpret_cast<uintptr_t>(s + head);
  const GblV4 s16 = gbl<V4>(reinterpret_cast<const void*>(sp & ~(uintptr_t)15));
  const uint32_t sh = (uint32_t)(sp & 15);
  const uint32_t lim = nc + (sh ? 1u : 0u);
  uint4* d16 = reinterpret_cast<uint4*>(dl + head);
  const uint32_t np = nc ? (nc + kMovePass - 1) / kMovePass : 1;
  uint8_t hb0 = 0;
  for (uint32_t i = 0; i < np; ++i) {
    const uint32_t j = right ? np - 1 - i : i;
    const uint32_t c0 = j * kMovePass;
    uint4 lo[kMoveRows];
    load_rows<kMoveRows, W>(lo, s16, c0, wv, lane, lim);
    const uint8_t hb = j == 0 && tid < head ? s[tid] : 0;
    const uint8_t tb = j + 1 == np && tid < lit - t0 ? s[t0 + tid] : 0;
    __syncthreads();  // this pass's bytes are all in registers
    store_rows<kMoveRows, W>(d16, lo, c0, wv, lane, nc, sh);
    if (j + 1 == np && tid < lit - t0) dl[t0 + tid] = tb;
    if (j == 0) hb0 = hb;
  }
  // (pass 0 has been read: last when D > 0; when D < 0 nothing stored below
  // the literal's new start is read again)
  if (tid < head) dl[tid] = hb0;
  if (lit) literal_tag(d + op, lit, tid);
  if (op) copy_bytes<kPlaceT>(d, tg, op, tid);
}

// A K-place workgroup's view of stream c (no K-scan): the offset of its
// fragment k, the stream's length and its PlaceMode.  Thread t takes fragments
// [t q, t q + q): their lengths before fragment k, whether any has tags, and
// (a stored job) how much longer than stored they come out -- whose prefix
// sums are the fragments' shifts.
struct PlaceLds {
  uint64_t part[kPlaceT / 64], all[kPlaceT / 64];
  int64_t tot[kPlaceT / 64], lo[kPlaceT / 64], hi[kPlaceT / 64];
  uint32_t any[kPlaceT / 64];
};
__device__ __forceinline__ void place_summary(const SnappyCJobs& J, const CJob& c, uint32_t k, PlaceLds& S,
                                              uint64_t& off, uint64_t& size, uint32_t& mode) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = (c.nfrag + kPlaceT - 1) / kPlaceT;
  const uint32_t i0 = min(c.nfrag, tid * q), i1 = min(c.nfrag, i0 + q);
  uint64_t part = 0, all = 0;
  uint32_t any = 0;
  int64_t tot = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint64_t fi = J.finfo[c.frag0 + i];
    const uint32_t li = (uint32_t)min((size_t)kFrag, c.n - (size_t)i * kFrag);
    const uint32_t fl = frag_len(fi, li);
    if (i < k) part += fl;
    all += fl;
    any |= fi != 0 ? 1u : 0u;
    tot += (int64_t)fl - (int64_t)frag_len(0, li);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    part += __shfl_xor(part, o, 64);
    all += __shfl_xor(all, o, 64);
    any |= __shfl_xor(any, o, 64);
  }
  if (lane == 0) {
    S.part[wave] = part;
    S.all[wave] = all;
    S.any[wave] = any;
  }
  __syncthreads();
  off = c.hdr;
  size = c.hdr;
  any = 0;
  for (uint32_t w = 0; w < kPlaceT / 64; ++w) {
    off += S.part[w];
    size += S.all[w];
    any |= S.any[w];
  }
  mode = !c.stored ? kPlaceCopy : !any ? kPlaceStored : kPlaceCopy;
  int64_t lo = 0, hi = 0;
  if (c.stored && any) {
    int64_t x = tot;  // the shift of fragment i0: the exclusive sum of the totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t y = __shfl_up(x, o, 64);
      if ((int)lane >= o) x += y;
    }
    if (lane == 63) S.tot[wave] = x;
    __syncthreads();
    int64_t run = x - tot;
    for (uint32_t w = 0; w < wave; ++w) run += S.tot[w];
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t li = (uint32_t)min((size_t)kFrag, c.n - (size_t)i * kFrag);
      run += (int64_t)frag_len(J.finfo[c.frag0 + i], li) - (int64_t)frag_len(0, li);
      lo = min(lo, run);  // (the shift of fragment i + 1, or the growth at the end)
      hi = max(hi, run);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (int64_t)__shfl_xor(lo, o, 64));
      hi = max(hi, (int64_t)__shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      S.lo[wave] = lo;
      S.hi[wave] = hi;
    }
    __syncthreads();
    for (uint32_t w = 0; w < kPlaceT / 64; ++w) {
      lo = min(lo, S.lo[w]);
      hi = max(hi, S.hi[w]);
    }
    if (lo >= -kShiftMax && hi <= kShiftMax) mode = kPlaceShift;
  }
  __syncthreads();  // (S is used again by the caller)
}

// Streams of up to kInlineScan fragments need no K-scan: the workgroup of
// fragment k sums the lengths of the stream's fragments itself (all full but
// the last); the workgroup of fragment 0 writes the varint header and
// publishes the stream length and mode -- the first workgroup of the stream
// to run, so the host, which needs them to finish the compress and launch the
// decode behind it, has them while K-place still runs (published by the last
// fragment's workgroup they arrived at its end, and the decode started 12-15
// us after it: C5 + COMPRESSING's kernel trace).
constexpr uint32_t kInlineScan = 4096;
__global__ __launch_bounds__(kPlaceT) void snappy_place(const SnappyCJobs J, const uint8_t* __restrict__ scratch) {
  __shared__ PlaceLds S;
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  // no K-scan: block j (among the first to run) publishes stream j's length
  // and mode, which the host needs to finish the compress and launch the
  // decode behind it -- it has them while K-place runs (published by the
  // stream's last, then its first fragment's workgroup, they arrived late in
  // K-place, and the decode started 12 us after it: kernel trace)
  if (!J.offset && blockIdx.x < J.njobs && J.pub) {
    const CJob& cj = J.j[blockIdx.x];
    uint64_t o, size;
    uint32_t m;
    place_summary(J, cj, cj.nfrag, S, o, size, m);
    if (tid == 0) {
      PubSlot* pub = J.pub + cj.slot;
      pub_store(&pub->size, size);
      pub_store(&pub->status, (int32_t)kOk);
      pub_store(&pub->pad, m != kPlaceCopy ? (uint32_t)kStoredInPlace : 0u);
      publish_ticket(pub, cj.ticket);
    }
  }
  const uint32_t ji = cjob_index(J, f);
  const CJob& c = J.j[ji];
  const uint32_t k = f - c.frag0;
  const size_t start = (size_t)k * kFrag;
  const uint32_t len = (uint32_t)min((size_t)kFrag, c.n - start);
  const uint64_t info = J.finfo[f];
  const uint32_t op = (uint32_t)(info >> 32), ne = (uint32_t)info;
  PSF_TRACE(f, 2);
  uint64_t off, size;
  uint32_t mode;
  if (J.offset) {
    mode = J.in_place[ji];
    if (mode == kPlaceStored) return;  // K-scan found every fragment stored: the stream is in place
    off = J.offset[f];
  } else {
    place_summary(J, c, k, S, off, size, mode);
    if (k == 0 && tid < c.hdr && mode == kPlaceCopy)
      c.dst[tid] = (uint8_t)(((uint32_t)c.n >> (7 * tid)) | (tid + 1 < c.hdr ? 128u : 0u));
    if (mode == kPlaceStored) return;  // FIXING_FLOAT wrote the stream, header and tags included
  }
  if (mode == kPlaceShift) {
    const int64_t dk = stored_shift(c, k, off);                       // this fragment's start
    const int64_t dn = dk + (int64_t)frag_len(info, len) - (int64_t)frag_len(0, len);  // the next one's
    if (!info && !dk) return;  // stored where it was written
    uint8_t* base = const_cast<uint8_t*>(c.in);
    const uint8_t* src = frag_src(c, k);
    uint8_t* dl = base + off + op + (ne < len ? lit_tag_len(len - ne - 1) : 0);
    place_moved(base + off, scratch + (size_t)f * kSnappyFragOut, op, src + ne, len - ne, tid);
    // the previous fragment's bytes end dk - (stored tag bytes) into this
    // one's (dk > 0), the next one's start -dn bytes before this one's end
    // (dn < 0): what the loads above may have seen rewritten there comes
    // from the stash
    const uint8_t* st = J.stash + (size_t)f * kStash;
    const uint32_t e = min(len, kEdge);
    const bool fix_head = dk > 0 && ne < e;
    const bool fix_tail = dn < 0 && k + 1 < c.nfrag && len >= kEdge;
    if (fix_head || fix_tail) {
      __syncthreads();
      if (fix_head && tid >= ne && tid < e) dl[tid - ne] = st[tid];
      const uint32_t p = len - kEdge + (tid - kEdge);
      if (fix_tail && tid >= kEdge && tid < kStash && p >= ne) dl[p - ne] = st[tid];
    }
    PSF_TRACE(f, 3);
    return;
  }
  uint8_t* d = c.dst + off;
  if (op) copy_bytes<kPlaceT>(d, scratch + (size_t)f * kSnappyFragOut, op, tid);
  if (ne < len) {
    d += op;
    d += literal_tag(d, len - ne, tid);
    copy_bytes<kPlaceT>(d, frag_src(c, k) + ne, len - ne, tid);
  }
  PSF_TRACE(f, 3);
}

}  // namespace
}  // namespace psf

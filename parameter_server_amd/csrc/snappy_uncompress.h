// COMPRESSING, the decompressor: any valid snappy stream, with RawUncompress's
// verdict.  K-spec (snappy_dspec, with K0 in one more workgroup per stream),
// then the tail: K1 (snappy_dscan), K2a-c (snappy_dlinka / b / c), K2
// (snappy_dlink), K3 (snappy_dindex) and K4 with K5 (snappy_dfrag); snappy.hip's
// header tells what each does.  The dq_* helpers are the FIXING_FLOAT decode
// fused into K-spec and K4.
//
// The measurements quoted in the comments below were taken with A/B scripts
// of the tuning rounds (windows, linker, ring, dequantise) that are not kept
// in the tree; the figures are kept as recorded.
#pragma once

#include "ff_dequant.h"
#include "snappy_common.h"

namespace psf {
namespace {

// compressed bytes per parse window: K1 / K3 are one wave per window whose
// chain walks are the work, so shorter windows mean more waves at once and
// shorter walks; the linker's work grows with the window count.  Sorted keys,
// 128 MiB, with the one-workgroup linker: 16 KiB windows 18.2 GB/s, 8 KiB
// 22.4, 4 KiB 22.7; with the three-launch linker (K2a-c) 8 KiB 27.5, 4 KiB
// 30.0.  (A literal that carries the
// chain past a window's first 64 bytes sends the stream to K2's serial walk;
// smaller windows have more starts to straddle.)
constexpr uint32_t kWin = 4096;
constexpr uint32_t kInWin = 4096;  // staged compressed bytes in the fragment decoder
// The fragment decoder's output window: the last kRing bytes of the fragment
// decoded so far sit in an LDS ring; older ones have been flushed to the
// output.  One decode step (a batch, or one tag; a long literal in pieces of
// kRingStep) writes at most kRingStep bytes; a step starts with at most
// kRingFlushAt bytes unflushed, so it overwrites only flushed bytes, and a copy
// source it cannot find in the ring was flushed before the step.
constexpr uint32_t kRing = 8192;
constexpr uint32_t kRingStep = 64 * 64;
constexpr uint32_t kRingFlushAt = kRing - kRingStep - 64;
constexpr uint32_t kBatchLit = 16;     // literals the fragment decoder's batches take (longer ones: one by one)
constexpr uint32_t kBatchMargin = 96;  // staged bytes past p a batch reads: 64 tag starts + a tag + kBatchLit
constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kFlagInvalid = 1, kFlagSerial = 2, kFlagScan = 4, kFlagHeader = 8;
constexpr uint64_t kFullLit = 65536 + 3;  // a 64 KiB fragment stored as one literal (tag 0xF4 + 2 length bytes)
constexpr uint32_t kStarts = 64;          // K1 parses from each of the first 64 offsets of a window
// K0's single steps before it hands the stream to K1/K2: one memory latency
// each, so a tag-dense stream costs K0 about 1 us per step until handed over
// (512: K-spec 0.59 ms on sorted keys, 64: 0.10); a stream of
// stored fragments with a few matches (C5's codes) stays well inside it
constexpr uint32_t kLitBudget = 64;

struct Tag {
  uint64_t next;  // position after the tag (literal data included)
  uint64_t len;   // output bytes
  uint32_t off;   // copy offset (0 for literals)
  uint32_t hl;    // header bytes (literal data follows)
  bool lit;
};

// Branch-free decode of the tag whose first 5 bytes are x (little endian).
__device__ __forceinline__ Tag decode_tag(uint64_t x, uint64_t p) {
  Tag t;
  const uint32_t c = (uint32_t)x & 0xff;
  const uint32_t ty = c & 3;
  const uint32_t k = (c >> 2) + 1 > 60 ? (c >> 2) + 1 - 60 : 0;  // literal length bytes
  const uint64_t litlen = k ? ((x >> 8) & ((1ull << (8 * k)) - 1)) + 1 : (c >> 2) + 1;
  const uint32_t off1 = ((c >> 5) << 8) | (uint32_t)((x >> 8) & 0xff);
  const uint32_t off2 = (uint32_t)((x >> 8) & 0xffff);
  const uint32_t off4 = (uint32_t)(x >> 8);
  t.lit = ty == 0;
  t.hl = ty == 0 ? 1 + k : ty == 1 ? 2 : ty == 2 ? 3 : 5;
  t.len = ty == 0 ? litlen : ty == 1 ? 4 + ((c >> 2) & 7) : (c >> 2) + 1;
  t.off = ty == 0 ? 0 : ty == 1 ? off1 : ty == 2 ? off2 : off4;
  t.next = p + t.hl + (ty == 0 ? litlen : 0);
  return t;
}

__device__ __forceinline__ uint64_t lane_of64(uint64_t v, uint32_t l) {
  return ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) | __builtin_amdgcn_readlane((uint32_t)v, l);
}
// The tag starts of a batch: lane l holds the (clamped) advance a of the tag
// that would start at p + l; from offset 0 the chain goes l -> l + a(l).
// Returns the bit mask of the chain's offsets below 64 that start before
// `lim` (relative to p) and lie in `ok`: a few scalar instructions per tag.
__device__ __forceinline__ uint64_t batch_mask(uint32_t a, uint64_t lim, uint64_t ok) {
  uint64_t M = 0;
  for (uint32_t q = 0; q < 64 && q < lim && ((ok >> q) & 1);) {
    M |= 1ull << q;
    q += __builtin_amdgcn_readlane(a, q);
  }
  return M;
}
// exclusive sum over the wave's lanes below this one, in DPP steps (no LDS
// round trips: a lane shuffle through ds_bpermute costs one each): the
// inclusive scan within each row of 16 lanes by row shifts 1, 2, 4, 8 (a lane
// with no source in its row adds 0), then row 15's total into the next row
// (row_bcast:15, rows 1 and 3) and lane 31's into rows 2 and 3 (row_bcast:31)
__device__ __forceinline__ uint32_t wave_excl_sum(uint32_t v, uint32_t) {
  uint32_t x = v;
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x - v;
}

// tag at LDS byte q of w (one two-dword read; q + 8 bytes must be staged)
__device__ __forceinline__ Tag lds_tag(const uint32_t* w, uint64_t q, uint64_t p) {
  const uint32_t i = (uint32_t)(q >> 2);
  const uint64_t x = (((uint64_t)w[i + 1] << 32) | w[i]) >> (8 * (q & 3));
  return decode_tag(x, p);
}

// Stage in[base, base+want) into LDS: aligned dword loads where the whole word
// lies inside the input, bytes at the edges (0 past the end).  Returns s with
// lds[s + i] == in[base + i].
__device__ __forceinline__ uint32_t stage(uint32_t* lds, const uint8_t* in, uint64_t C, uint64_t base, uint32_t want,
                                          uint32_t lane) {
  const uint32_t s = (uint32_t)(reinterpret_cast<uintptr_t>(in + base) & 3);
  const int64_t r0 = (int64_t)base - (int64_t)s;  // input offset of lds byte 0 (dword aligned)
  const uint32_t nw = (s + want + 3) >> 2;
  // 8 loads in flight per lane before their LDS stores (one memory latency
  // per 2 KiB instead of one per 256 B)
  for (uint32_t j0 = 0; j0 < nw; j0 += 8 * 64) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t j = j0 + u * 64 + lane;
      const int64_t r = r0 + 4 * (int64_t)j;
      v[u] = 0;
      if (j < nw) {
        if (r >= 0 && r + 4 <= (int64_t)C) {
          v[u] = *reinterpret_cast<const uint32_t*>(in + r);
        } else {
          for (int q = 0; q < 4; ++q)
            if (r + q >= 0 && r + q < (int64_t)C) v[u] |= (uint32_t)in[r + q] << (8 * q);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t j = j0 + u * 64 + lane;
      if (j < nw) lds[j] = v[u];
    }
  }
  return s;
}

// the 5 tag bytes at input offset p (zero past the end): three aligned dwords
__device__ __forceinline__ uint64_t tag_bytes(const uint8_t* in, uint64_t C, uint64_t p) {
  const uintptr_t ia = reinterpret_cast<uintptr_t>(in);
  const uint64_t a = (ia + p) & ~(uintptr_t)3;
  const uint64_t ai = a - ia;
  uint32_t d[3] = {0, 0, 0};
  if (ai + 12 <= C) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a);
    d[0] = q[0];
    d[1] = q[1];
    d[2] = q[2];
  } else {
    for (int i = 0; i < 12; ++i) {
      const uint64_t r = ai + i;
      if (r < C) d[i >> 2] |= (uint32_t)in[r] << (8 * (i & 3));
    }
  }
  const uint32_t sh = (uint32_t)(p - ai) * 8;
  const uint64_t lo = ((uint64_t)d[1] << 32) | d[0];
  return sh ? (lo >> sh) | ((uint64_t)d[2] << (64 - sh)) : lo;
}

// The host sized the launch from a hint (the FilterConfig's uncompressed
// size): the stream's own varint header must say the same, else the host
// redoes the call from the header (Varint::Parse32WithLimit).
__device__ __forceinline__ bool header_matches(const uint8_t* __restrict__ in, uint64_t C, uint32_t hdr,
                                               uint64_t dsize) {
  const uint64_t h = tag_bytes(in, C, 0);
  uint64_t v = 0;
  uint32_t len = 0;
  for (uint32_t i = 0; i < 5 && i < C; ++i) {
    const uint32_t b = (uint32_t)(h >> (8 * i)) & 0xff;
    if (i == 4 && b >= 16) break;
    v |= (uint64_t)(b & 127u) << (7 * i);
    if (b < 128) {
      len = i + 1;
      break;
    }
  }
  return len == hdr && v == dsize;
}

// d[0, len) = s[0, len) for any alignment of either, by 256 lanes: byte
// stores up to the first 4-aligned destination dword, then lane-contiguous
// dwords (each load and store instruction covers 256 contiguous bytes), each
// funnel-shifted from the two aligned source dwords that cover it, 16 per lane
// per step with all loads issued before the stores (a wave's memory counter
// retires in order: a load behind a store waits for it).  The loads are
// unconditional (clamped), the stores predicated, so the compiler keeps exact
// wait counts.  (Round 3: 16-byte chunks from five dword loads each ran the
// 128 MiB stored stream at 3.7 TB/s.)  U = dwords in flight
// per lane: 16 in K-spec, fewer in K4, whose occupancy its decoder sets.
template <int U = 16>
__device__ __forceinline__ void copy_g2g(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint32_t len,
                                         uint32_t tid) {
  uint32_t head = (uint32_t)(-reinterpret_cast<uintptr_t>(d) & 3);
  if (head > len) head = len;
  if (tid < head) d[tid] = s[tid];
  d += head;
  s += head;
  len -= head;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s);
  const uint32_t sh = (uint32_t)(sa & 3) * 8;
  const auto a = gbl<uint32_t>(reinterpret_cast<const void*>(sa & ~(uintptr_t)3));  // global, not flat, loads
  auto* o = reinterpret_cast<__attribute__((address_space(1))) uint32_t*>(reinterpret_cast<uintptr_t>(d));
  const uint32_t ng = len >> 2;
  for (uint32_t g0 = 0; g0 < ng; g0 += U * 256) {
    uint32_t w0[U], w1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t g = min(g0 + u * 256 + tid, ng - 1);
      w0[u] = a[g];
      w1[u] = a[sh ? g + 1 : g];  // the next dword lies inside the source only when it is needed
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t g = g0 + u * 256 + tid;
      if (g < ng) o[g] = sh ? __builtin_amdgcn_alignbit(w1[u], w0[u], sh) : w0[u];
    }
  }
  for (uint32_t i = (ng << 2) + tid; i < len; i += 256) d[i] = s[i];
}

// Last-workgroup election by one device-scope counter.  No fence: what the
// last workgroup goes on to do reads nothing the others wrote in this launch
// (an agent-scope fence on MI355X writes back the XCD's whole L2, which
// every workgroup of a streaming kernel would pay for).
__device__ __forceinline__ bool last_block(uint32_t* ctr, uint32_t total, uint32_t* s_last) {
  __syncthreads();
  if (threadIdx.x == 0) *s_last = atomicAdd(ctr, 1u) == total - 1;
  __syncthreads();
  return *s_last;
}

// Several streams decode in one launch chain (the COMPRESSING arrays of a
// batch of messages): every kernel's grid is the union of the streams' output
// fragments (or windows, or streams), and a workgroup first finds its stream
// in the job table, which rides in the kernel arguments.
struct DJob {
  const uint8_t* in;
  uint8_t* out;
  uint8_t* scratch;  // this stream's index arrays
  uint64_t C, dsize;
  uint32_t hdr, nfo, nwin;
  uint32_t fo0, win0;  // first output fragment / window of this stream in the grids
  uint32_t slot, ticket;
  // fused FIXING_FLOAT decode (SnappyDequant): values of the codes, or null
  void* fv;
  const float* frange;
  double fratio;
  float fmn, fmx;
  uint32_t fnb, fdbl;
  uint32_t blk0;  // first linker block of this stream in the linker grids
};
struct SnappyDJobs {
  DJob j[kSnappyBatchMax];
  uint32_t* ctrl;  // 8 words per stream: flags[0..3] (verdict, indexed, decoded by K-spec, linked by K2b), counters[4..7]
  PubSlot* pub;
  uint32_t njobs, nfo1, nwin;  // streams; output fragments (at least one per stream); windows
  uint32_t nblk;               // linker blocks (kLinkPer windows each)
  uint32_t* znext;  // the next launch's zeroed ctrl region (null: none), cleared by K-spec
  uint32_t zwords;
};
struct DScr {
  uint32_t *flags, *ctr;
  uint64_t *wexit, *wtotal, *wentry, *woff, *fragpos, *specpos, *specend;
  uint32_t *fdone;  // fused decode: fragment k's values written by K-spec (1) or still codes (0)
  uint32_t *bitmap, *cum;
};
// (host too: the launch layer checks the carving against the bytes it allocates)
__host__ __device__ __forceinline__ DScr dscr(const SnappyDJobs& J, const DJob& D, uint32_t i) {
  DScr S;
  S.flags = J.ctrl + 8 * i;
  S.ctr = S.flags + 4;
  S.wexit = reinterpret_cast<uint64_t*>(D.scratch);
  S.wtotal = S.wexit + (size_t)(D.nwin + 1) * kStarts;
  S.wentry = S.wtotal + (size_t)(D.nwin + 1) * kStarts;
  S.woff = S.wentry + (D.nwin + 1);
  S.fragpos = S.woff + (D.nwin + 1);
  S.specpos = S.fragpos + (D.nfo + 1);
  S.specend = S.specpos + (D.nfo + 1);
  S.fdone = reinterpret_cast<uint32_t*>(S.specend + (D.nfo + 1));
  S.bitmap = reinterpret_cast<uint32_t*>(S.specend + 2 * (D.nfo + 1));
  S.cum = S.bitmap + (size_t)(D.nwin + 1) * (kWin / 32);
  return S;
}
// the stream of output fragment / window / linker block b of the union grids,
// whose streams start at `first` (&DJob::fo0, win0 or blk0)
__device__ __forceinline__ uint32_t djob_of(const SnappyDJobs& J, uint32_t b, uint32_t DJob::*first) {
  uint32_t i = 0;
  while (i + 1 < J.njobs && b >= J.j[i + 1].*first) ++i;
  return i;
}

// ---- FIXING_FLOAT decode fused into the uncompress (SnappyDequant) ----
// A stream of FIXING_FLOAT codes whose next decode is FIXING_FLOAT is decoded
// straight to values: where the fast path copies a stored fragment, it
// dequantises it instead (the codes never reach HBM), and fragments placed any
// other way are dequantised from their codes afterwards.  The arithmetic is
// ff_decode's (ff_dequant.h), so the values are bit-identical to the unfused
// chain.
typedef float dq_f32x4 __attribute__((ext_vector_type(4)));
typedef float dq_f32x2 __attribute__((ext_vector_type(2)));
typedef double dq_f64x2 __attribute__((ext_vector_type(2)));

struct DqParams {
  double ratio, inv, bin, min_v;
};
// ff_decode's parameters for stream D (the encode's device range when it left one)
__device__ __forceinline__ DqParams dq_params(const DJob& D) {
  float mn = D.fmn, mx = D.fmx;
  if (D.frange) {
    mn = D.frange[0];
    mx = D.frange[1];
  }
  DqParams P;
  P.min_v = (double)mn;
  P.bin = (double)mx - P.min_v;
  P.ratio = D.fratio;
  P.inv = 1.0 / P.ratio;
  return P;
}

// nb = 1: the 256-entry table ff_decode builds (same formula, same bits)
template <typename V>
__device__ __forceinline__ void dq_lut(V* lut, const DqParams& P, uint32_t tid) {
  lut[tid] = dequant<V>((uint64_t)tid, P.ratio, P.bin, P.min_v);
}

// the values of one dword of codes (4 / NB of them) to o, non-temporal
template <typename V, int NB>
__device__ __forceinline__ void dq_store(V* o, uint32_t w, const V* lut, const DqParams& P) {
  if (NB == 1) {
    const V x0 = lut[w & 255], x1 = lut[(w >> 8) & 255], x2 = lut[(w >> 16) & 255], x3 = lut[w >> 24];
    if constexpr (sizeof(V) == 4) {
      const dq_f32x4 t = {(float)x0, (float)x1, (float)x2, (float)x3};
      __builtin_nontemporal_store(t, reinterpret_cast<dq_f32x4*>(o));
    } else {
      const dq_f64x2 a = {(double)x0, (double)x1}, b = {(double)x2, (double)x3};
      __builtin_nontemporal_store(a, reinterpret_cast<dq_f64x2*>(o));
      __builtin_nontemporal_store(b, reinterpret_cast<dq_f64x2*>(o) + 1);
    }
  } else {
    const V x0 = dequant_q<V>(w & 0xFFFF, P.ratio, P.inv, P.bin, P.min_v);
    const V x1 = dequant_q<V>(w >> 16, P.ratio, P.inv, P.bin, P.min_v);
    if constexpr (sizeof(V) == 4) {
      const dq_f32x2 t = {(float)x0, (float)x1};
      __builtin_nontemporal_store(t, reinterpret_cast<dq_f32x2*>(o));
    } else {
      const dq_f64x2 t = {(double)x0, (double)x1};
      __builtin_nontemporal_store(t, reinterpret_cast<dq_f64x2*>(o));
    }
  }
}

// v[0, len / NB) = the values of the codes s[0, len) (s at any alignment, v
// 16-byte aligned, len a multiple of NB), by 256 lanes: lane l takes the
// dwords of codes l, l + 256, ..., each funnel-shifted from the two aligned
// dwords that cover it (the second lies inside the source whenever it is
// needed), 8 in flight before any store.
template <typename V, int NB, int U>
__device__ void dq_bytes(const uint8_t* __restrict__ s, V* __restrict__ v, uint32_t len, const V* lut,
                         const DqParams& P, uint32_t tid) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s);
  const uint32_t sh = (uint32_t)(sa & 3) * 8;
  const auto a = gbl<uint32_t>(reinterpret_cast<const void*>(sa & ~(uintptr_t)3));  // global, not flat, loads
  const uint32_t ng = len >> 2;
  for (uint32_t g0 = 0; g0 < ng; g0 += U * 256) {
    uint32_t w0[U], w1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t g = min(g0 + u * 256 + tid, ng - 1);
      w0[u] = a[g];
      w1[u] = a[sh ? g + 1 : g];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t g = g0 + u * 256 + tid;
      const uint32_t w = sh ? __builtin_amdgcn_alignbit(w1[u], w0[u], sh) : w0[u];
      if (g < ng) dq_store<V, NB>(v + (size_t)g * (4 / NB), w, lut, P);
    }
  }
  for (uint32_t i = (ng << 2) / NB + tid; i < len / NB; i += 256) {  // the array's last len % 4 bytes
    uint32_t r = 0;
    for (int j = 0; j < NB; ++j) r |= (uint32_t)s[i * NB + j] << (8 * j);
    v[i] = NB == 1 ? lut[r] : dequant_q<V>(r, P.ratio, P.inv, P.bin, P.min_v);
  }
}

// The workgroup's LDS table (nb = 1) for stream D; called by all 256 lanes,
// ends with a barrier.
__device__ __forceinline__ void dq_prepare(const DJob& D, double* lut64, uint32_t tid) {
  const DqParams P = dq_params(D);
  if (D.fnb == 1) {
    if (D.fdbl) dq_lut<double>(lut64, P, tid);
    else dq_lut<float>(reinterpret_cast<float*>(lut64), P, tid);
  }
  __syncthreads();
}

// Output fragment bytes [o0, o0 + len) of stream D, whose codes are at s, to
// their values (after dq_prepare).  U = code dwords in flight per lane: K-spec
// (global loads, C5 + COMPRESSING) measured 4 / 8 / 12 / 16 / 32 at
// 119 / 113 / 112 / 110 / 110 us; K4 keeps 8 (its decoder's
// registers set its occupancy).
template <int U = 16>
__device__ __forceinline__ void dq_frag(const DJob& D, const uint8_t* s, uint64_t o0, uint32_t len,
                                        const double* lut64, uint32_t tid) {
  const DqParams P = dq_params(D);
  const uint64_t first = o0 / D.fnb;  // 65536 is a multiple of nb
  if (D.fdbl) {
    double* v = static_cast<double*>(D.fv) + first;
    if (D.fnb == 1) dq_bytes<double, 1, U>(s, v, len, lut64, P, tid);
    else dq_bytes<double, 2, U>(s, v, len, lut64, P, tid);
  } else {
    float* v = static_cast<float*>(D.fv) + first;
    const float* lut = reinterpret_cast<const float*>(lut64);
    if (D.fnb == 1) dq_bytes<float, 1, U>(s, v, len, lut, P, tid);
    else dq_bytes<float, 2, U>(s, v, len, lut, P, tid);
  }
}

// K0: link the chain directly when the stream is mostly 64 KiB fragments
// stored as single literals (what a snappy 1.1.8 encoder emits for
// incompressible fragments, e.g. FIXING_FLOAT codes): lane k decodes the tags
// at p + (k + 64 j) * kFullLit for j < kLitRows, and the leading run of
// positions that hold a full literal is consumed in one step (512 fragments
// per memory latency); other tags take a single step.  After kLitBudget
// single steps the stream is handed to the window scan (K1) and its linker
// (K2) through kFlagScan.  K0 also records each output fragment's first tag
// and checks the tags it steps over one at a time as K3 would (the full
// literals have no copies); if it walks the whole stream, flags[1] = 1 tells
// K3 there is nothing left to index or validate.
// (One wave; its stores to a word are issued in program order, so the
// initialisation needs no barrier.)
constexpr int kLitRows = 8;
__device__ void dlit_body(const uint8_t* __restrict__ in, uint64_t C, uint32_t hdr, uint64_t dsize, uint32_t nwin,
                          uint64_t* __restrict__ wentry, uint64_t* __restrict__ woff, uint64_t* __restrict__ fragpos,
                          uint32_t* __restrict__ flags, uint32_t lane) {
  for (uint32_t i = lane; i < nwin; i += 64) wentry[i] = kNone;
  if (lane == 0) flags[1] = 0;
  if (!header_matches(in, C, hdr, dsize)) {
    if (lane == 0) *flags = kFlagHeader;
    return;
  }
  uint64_t p = hdr, o = 0;
  int64_t last_w = -1;
  uint32_t singles = 0;
  bool bad = false, serial = false, wide = true;
  while (p < C) {
    bool full[kLitRows];
    uint64_t pk[kLitRows];
    Tag t0;
#pragma unroll
    for (int j = 0; j < kLitRows; ++j) {
      pk[j] = p + (uint64_t)(lane + 64 * j) * kFullLit;
      full[j] = false;
      if (j == 0 || wide) {  // after a single step, probe one row only
        const Tag t = decode_tag(tag_bytes(in, C, pk[j]), pk[j]);
        full[j] = pk[j] < C && t.lit && t.len == 65536 && t.hl == 3;
        if (j == 0) t0 = t;
      }
    }
    uint32_t c = 0;  // leading run of full literals over rows 0, 1, ...
    bool open = true;
#pragma unroll
    for (int j = 0; j < kLitRows; ++j) {
      const uint64_t m = __ballot(full[j]);
      if (open) {
        const uint32_t r = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
        c += r;
        open = r == 64;
      }
    }
    if (c > 0) {
      const bool aligned = (o & (kFrag - 1)) == 0;
      serial = serial || !aligned;  // full literals across output fragments
#pragma unroll
      for (int j = 0; j < kLitRows; ++j) {
        const uint32_t idx = lane + 64 * j;
        if (idx < c) {
          const int64_t wk = (int64_t)((pk[j] - hdr) / kWin);
          if (idx > 0 || wk > last_w) {  // full literals are > kWin apart: one per window
            wentry[wk] = pk[j];
            woff[wk] = o + (uint64_t)idx * 65536;
          }
          if (aligned) fragpos[o / kFrag + idx] = pk[j];
        }
      }
      last_w = (int64_t)((p + (uint64_t)(c - 1) * kFullLit - hdr) / kWin);
      p += (uint64_t)c * kFullLit;
      o += (uint64_t)c * 65536;
      wide = true;
    } else {
      wide = false;
      const uint64_t t0next = __shfl(t0.next, 0, 64), t0len = __shfl(t0.len, 0, 64);
      const bool t0lit = __shfl((int)t0.lit, 0, 64) != 0;
      const uint32_t t0off = __shfl(t0.off, 0, 64);
      const int64_t w0 = (int64_t)((p - hdr) / kWin);
      if (lane == 0) {
        if (w0 > last_w) {
          wentry[w0] = p;
          woff[w0] = o;
        }
        if ((o & (kFrag - 1)) == 0) fragpos[o / kFrag] = p;  // the tag that starts an output fragment
      }
      // what K3 checks, for the tags seen one at a time (the full literals
      // of the wide steps have no copies): a copy within the output so far,
      // and no tag or copy across output fragments (else the one-lane decoder)
      if (!t0lit) {
        if (t0off == 0 || t0off > o) bad = true;
        else if (o - t0off < (o & ~(uint64_t)(kFrag - 1))) serial = true;
      }
      if (o / kFrag != (o + t0len - 1) / kFrag) serial = true;
      if (w0 > last_w) last_w = w0;
      p = t0next;
      o += t0len;
      if (++singles > kLitBudget) {
        if (lane == 0) *flags = kFlagScan;
        return;
      }
    }
    if (o > dsize) {
      bad = true;
      break;
    }
  }
  const bool ok = !(bad || p != C || o != dsize);
  if (lane == 0) {
    *flags = !ok ? kFlagInvalid : serial ? kFlagSerial : 0u;
    flags[1] = ok ? 1u : 0u;  // every tag seen: K3 has nothing to add
  }
}

constexpr uint32_t kFewTags = 8;  // fragments of at most this many tags are decoded without LDS

struct FewLds {
  uint32_t n, o[kFewTags], len[kFewTags], off[kFewTags];
  uint64_t src[kFewTags], next;
};

// Output fragment d[0, end) from the tags at p, when they are at most
// kFewTags, end exactly at the fragment's end and copy only from inside it
// (stored data with a match or two): one lane walks the tags (checking each as
// RawUncompress would), all 256 lanes copy the literals global to global, then
// the copies run in order.  Returns the position after the fragment's last
// tag, or kNone (nothing written) when the fragment is not of that kind.
// Called by the whole workgroup.  U: copy_g2g's dwords in flight per lane.
template <int U = 16>
__device__ uint64_t decode_few(const uint8_t* __restrict__ in, uint64_t C, uint64_t p, uint32_t end,
                               uint8_t* __restrict__ d, uint32_t tid, FewLds& F) {
  if (tid == 0) {
    uint32_t o = 0, n = 0;
    bool good = p < C;
    while (good && o < end && n < kFewTags) {
      const Tag t = decode_tag(tag_bytes(in, C, p), p);
      if (t.lit ? t.next > C : (t.off == 0 || t.off > o)) good = false;
      F.o[n] = o;
      F.len[n] = (uint32_t)t.len;
      F.off[n] = t.off;
      F.src[n] = t.lit ? p + t.hl : kNone;
      o += (uint32_t)min(t.len, (uint64_t)kFrag + 1);
      p = t.next;
      ++n;
    }
    F.n = good && o == end ? n : 0;
    F.next = p;
  }
  __syncthreads();
  const uint32_t nt = F.n;
  if (nt == 0) return kNone;
  for (uint32_t i = 0; i < nt; ++i)
    if (F.src[i] != kNone) copy_g2g<U>(d + F.o[i], in + F.src[i], F.len[i], tid);
  __syncthreads();
  for (uint32_t i = 0; i < nt; ++i) {
    if (F.src[i] != kNone) continue;
    const uint32_t o = F.o[i], L = F.len[i], off = F.off[i];
    for (uint32_t j = tid; j < L; j += 256) d[o + j] = d[o - off + (off >= L ? j : j % off)];
    __syncthreads();
  }
  return F.next;
}

// K-spec: every output fragment k is first taken to be stored as one literal
// at hdr + k * (65536 + 3) -- what a 1.1.8 encoder writes for a stream of
// incompressible fragments (FIXING_FLOAT codes).  A workgroup checks its
// fragment's tag there and, if it is the literal that fills the fragment,
// copies it at once; a fragment found a few bytes off that place (after one
// with a match) is copied from there, and the first fragment with a few tags
// is decoded where assumed.  If every fragment was placed and each ends where
// the next begins (the first after the header, the last at the end of the
// stream), the stream is exactly that chain: decoded and valid, as the last
// workgroup to finish records.  One more workgroup
// runs K0 alongside (its verdict and index agree with that on such a stream);
// otherwise the kernels after this one redo every fragment whose true
// position differs from the one assumed here (specpos).
__global__ __launch_bounds__(256) void snappy_dspec(const SnappyDJobs J) {
  __shared__ uint32_t s_last, s_checked;
  __shared__ double s_lut[256];  // fused decode, nb = 1
  const uint32_t tid = threadIdx.x;
  if (J.znext)  // the next launch's control words (this launch's were cleared by the one before)
    for (uint32_t i = blockIdx.x * 256 + tid; i < J.zwords; i += gridDim.x * 256) J.znext[i] = 0;
  if (blockIdx.x < J.njobs) {  // one more workgroup per stream links it meanwhile (K0), needed or not
    const uint32_t i = blockIdx.x;  // dispatched first: its walk overlaps the copies
    const DJob& D = J.j[i];
    const DScr S = dscr(J, D, i);
    if (tid < 64) dlit_body(D.in, D.C, D.hdr, D.dsize, D.nwin, S.wentry, S.woff, S.fragpos, S.flags, tid);
    return;
  }
  const uint32_t b = blockIdx.x - J.njobs;
  const uint32_t ji = djob_of(J, b, &DJob::fo0);
  const DJob& D = J.j[ji];
  const DScr S = dscr(J, D, ji);
  const uint8_t* __restrict__ in = D.in;
  uint8_t* __restrict__ out = D.out;
  const uint64_t C = D.C, dsize = D.dsize;
  const uint32_t hdr = D.hdr, nfo = D.nfo, ticket = D.ticket;
  uint64_t* __restrict__ specpos = S.specpos;
  uint32_t* __restrict__ flags = S.flags;
  uint32_t* __restrict__ ctr = S.ctr;
  PubSlot* pub = J.pub ? J.pub + D.slot : nullptr;
  const uint32_t k = b - D.fo0, nspec = nfo ? nfo : 1;
  const uint64_t o0 = (uint64_t)k * kFrag;
  const uint32_t end = (uint32_t)min((uint64_t)kFrag, dsize - o0);  // 0 only for an empty output
  const uint64_t p = hdr + (uint64_t)k * kFullLit;
  bool ok = k > 0 || header_matches(in, C, hdr, dsize);
  uint32_t hl = 0;
  if (end == 0) {
    ok = ok && C == hdr;
  } else {
    hl = end - 1 < 60 ? 1 : ((31 - __builtin_clz(end - 1)) >> 3) + 2;
    const Tag t = decode_tag(tag_bytes(in, C, p), p);
    ok = ok && p < C && t.lit && t.len == end && t.hl == hl && t.next <= C && (k + 1 < nfo || t.next == C);
  }
  if (D.fv) dq_prepare(D, s_lut, tid);  // the range load overlaps the tag's
  // A fragment after one that is not stored (a 1.1.8 encoder found a match in
  // it) sits a few bytes off its assumed place: look for its literal within
  // +-128 bytes and copy it from there too.  That is a guess only (it does not
  // count as checked); K4 redoes the fragment unless K0/K3 find it there.
  uint64_t at = ok ? p : kNone;
  if (!ok && end && k > 0) {
    __shared__ uint32_t s_best;
    if (tid == 0) s_best = 0xffffffffu;
    __syncthreads();
    const int32_t dl = (int32_t)tid - 128;
    const uint64_t q = p + dl;
    if (dl != 0 && q < C) {
      const Tag t = decode_tag(tag_bytes(in, C, q), q);
      if (t.lit && t.len == end && t.hl == hl && t.next <= C && (k + 1 < nfo || t.next == C))
        atomicMin(&s_best, ((uint32_t)abs(dl) << 9) | tid);
    }
    __syncthreads();
    if (s_best != 0xffffffffu) at = p + (int32_t)(s_best & 511) - 128;
  }
  uint64_t e = kNone;  // where this fragment's tags end
  uint32_t vdone = 0;   // fused decode: this fragment's values written here
  if (at != kNone) {
    if (D.fv) {
      dq_frag(D, in + at + hl, o0, end, s_lut, tid);
      vdone = 1;
    } else {
      copy_g2g(out + o0, in + at + hl, end, tid);
    }
    e = at + hl + end;
  } else if (end && (k > 0 || header_matches(in, C, hdr, dsize))) {
    // not stored: a fragment with a few tags, right after stored ones that
    // all sit where assumed (the first such fragment of the stream), is
    // decoded here too
    __shared__ FewLds F;
    e = decode_few(in, C, p, end, out + o0, tid, F);
    if (e != kNone) {
      at = p;
      if (D.fv) {  // the codes just written (L2-hot) to their values (decode_few ends with a barrier)
        dq_frag(D, out + o0, o0, end, s_lut, tid);
        vdone = 1;
      }
    }
  } else if (ok) {
    e = C;  // the empty output: the header is the stream
  }
  // device-scope stores: the last workgroup reads them from another XCD
  if (tid == 0) {
    __hip_atomic_store(&specpos[k], at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&S.specend[k], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.fdone[k] = vdone;  // read by K4 (a later launch)
  }
  // one counter for both: workgroups done (high word) and fragments placed
  const bool placed = e != kNone;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long old =
        atomicAdd(reinterpret_cast<unsigned long long*>(ctr), (1ull << 32) | (placed ? 1ull : 0ull));
    s_last = (uint32_t)(old >> 32) == nspec - 1;
    s_checked = (uint32_t)old + (placed ? 1u : 0u);
  }
  __syncthreads();
  if (!s_last) return;
  // every fragment placed somewhere: the stream is that chain if each one
  // ends where the next begins, the first begins after the header and the
  // last ends the stream
  __shared__ uint32_t s_chain;
  if (tid == 0) s_chain = s_checked == nspec ? 1u : 0u;
  __syncthreads();
  if (s_chain) {
    for (uint32_t i = tid; i < nspec; i += 256) {
      const uint64_t pos = __hip_atomic_load(&specpos[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t prev = i ? __hip_atomic_load(&S.specend[i - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : (uint64_t)hdr;
      bool good = pos == prev;
      if (i + 1 == nspec)
        good = good && __hip_atomic_load(&S.specend[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == C;
      if (!good) s_chain = 0;  // any lane may clear it
    }
  }
  __syncthreads();
  if (s_chain) {
    if (tid == 0) {
      flags[0] = 0;
      flags[1] = 1;
      flags[2] = 1;  // decoded: the kernels after this one have nothing to do
      if (pub) {
        pub_store(&pub->status, (int32_t)kOk);
        pub_store(&pub->size, (uint64_t)dsize);
        publish_ticket(pub, ticket);
      }
    }
  }
}


// K2: link the windows along the true chain.  The walk is one chain (every
// lane holds the same values); K1's tables of the next kLinkAhead windows
// (exit and output count per start offset) are copied into LDS together, so a
// window entered at one of its first 64 bytes costs one LDS read and one
// memory latency per kLinkAhead windows.  Other entries step tag by tag until
// they meet lane 0's chain (bitmap word and the next tag's bytes loaded
// together).  Windows are entered in increasing order, so the first-entry
// bookkeeping stays in registers.
constexpr uint32_t kLinkAhead = 16;
__device__ void dlink_body(const uint8_t* __restrict__ in, uint64_t C, uint32_t hdr, uint64_t dsize,
                           const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ cum,
                           const uint64_t* __restrict__ wexit, const uint64_t* __restrict__ wtotal, uint32_t nwin,
                           uint64_t* __restrict__ wentry, uint64_t* __restrict__ woff, uint32_t* __restrict__ flags,
                           uint64_t* lex, uint64_t* ltot) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < nwin; i += 64) wentry[i] = kNone;
  __syncthreads();
  uint64_t p = hdr, o = 0;
  int64_t last_w = -1;  // highest window whose entry is recorded
  bool bad = false;
  const uintptr_t ia = reinterpret_cast<uintptr_t>(in);
  uint32_t tw = 0;  // first window of the tables in LDS
  bool have = false;
  while (p < C) {
    const uint64_t rel = p - hdr;
    const uint32_t w = (uint32_t)(rel / kWin);
    const uint64_t off = rel - (uint64_t)w * kWin;
    if ((int64_t)w > last_w) {
      if (lane == 0) {
        wentry[w] = p;
        woff[w] = o;
      }
      last_w = w;
    }
    if (off < kStarts) {  // parsed exactly by K1's lane `off`
      if (!have || w - tw >= kLinkAhead) {
        have = true;
        tw = w;
        uint64_t e[kLinkAhead], t[kLinkAhead];
#pragma unroll
        for (uint32_t j = 0; j < kLinkAhead; ++j) {
          const size_t r = (size_t)min(w + j, nwin - 1) * kStarts + lane;
          e[j] = wexit[r];
          t[j] = wtotal[r];
        }
#pragma unroll
        for (uint32_t j = 0; j < kLinkAhead; ++j) {
          lex[j * kStarts + lane] = e[j];
          ltot[j * kStarts + lane] = t[j];
        }
      }
      const uint32_t q = (w - tw) * kStarts + (uint32_t)off;
      o += ltot[q];
      p = lex[q];
    } else {
      // bitmap word and the 8 bytes at p, loaded together
      const uint32_t bw = bitmap[rel >> 5];
      const uint64_t a = (ia + p) & ~(uintptr_t)3;  // aligned dword address
      const uint64_t ai = a - ia;                    // its input offset (may be < p)
      uint32_t d0 = 0, d1 = 0, d2 = 0;
      if (ai + 12 <= C) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(a);
        d0 = q[0];
        d1 = q[1];
        d2 = q[2];
      } else {
        for (int i = 0; i < 12; ++i) {
          const uint64_t r = ai + i;
          const uint32_t b = r < C ? in[r] : 0;
          if (i < 4) d0 |= b << (8 * i); else if (i < 8) d1 |= b << (8 * (i - 4)); else d2 |= b << (8 * (i - 8));
        }
      }
      if ((bw >> (rel & 31)) & 1) {  // met lane 0's chain
        o += wtotal[(size_t)w * kStarts] - cum[p];
        p = wexit[(size_t)w * kStarts];
      } else {  // one tag, then look again
        const uint32_t sh = (uint32_t)(p - ai) * 8;  // 0..24
        const uint64_t lo = ((uint64_t)d1 << 32) | d0;
        const uint64_t x = sh ? (lo >> sh) | ((uint64_t)d2 << (64 - sh)) : lo;
        const Tag t = decode_tag(x, p);
        o += t.len;
        p = t.next;
      }
    }
    if (o > dsize) {
      bad = true;
      break;
    }
  }
  if (lane == 0) *flags = (bad || p != C || o != dsize) ? kFlagInvalid : 0;
}

// K1: speculative parse of each window from each of its first 64 byte offsets
// (lane l from offset l).  A window's true entry is one of them unless a literal
// carried the chain further in; for those K2 walks until it meets lane 0's chain.
constexpr uint32_t kEarly = 1024;  // bytes of a window where K1's starts are expected to meet lane 0's chain

// The chain of tags from p (relative to the staged window) to the first
// position >= wl, walked by the wave in batches: every lane decodes the tag
// that would start at p + lane, one scalar walk picks the chain's tags in
// [p, p + 64).  Adds the output to o, returns the exit position.  kRecord:
// lane 0's chain of K1 -- each tag into the bitmap, its output count before
// it into cum.
template <bool kRecord>
__device__ uint64_t scan_walk(const uint32_t* b32, uint32_t s, uint32_t wl, uint64_t p, uint64_t& o, uint32_t lane,
                              uint32_t* bm, uint32_t* __restrict__ cum) {
  while (p < wl) {
    const uint64_t pl = min(p + lane, (uint64_t)wl);
    const Tag tl = lds_tag(b32, s + pl, pl);
    const uint64_t adv = tl.next - pl;
    const uint64_t M = batch_mask((uint32_t)min(adv, (uint64_t)64), wl - p, ~0ull);
    const bool tag = (M >> lane) & 1;
    // a tag's output offset in the batch: every tag before the last has a
    // length <= 64 (it ends inside the batch)
    const uint32_t rel = wave_excl_sum(tag ? (uint32_t)min(tl.len, (uint64_t)64) : 0u, lane);
    if (kRecord && tag) {
      const uint64_t r = p + lane;
      atomicOr(&bm[r >> 5], 1u << (r & 31));
      cum[r] = (uint32_t)(o + rel);
    }
    const uint32_t last = 63 - __builtin_clzll(M);
    o += lane_of(rel, last) + lane_of64(tl.len, last);
    p += last + lane_of64(adv, last);
  }
  return p;
}

__device__ void dscan_body(const SnappyDJobs& J, uint32_t ji, uint32_t w, uint32_t* b32, uint32_t* bm) {
  const DJob& D = J.j[ji];
  const DScr S = dscr(J, D, ji);
  if (!(*S.flags & kFlagScan)) return;  // K0 linked the stream already
  const uint8_t* __restrict__ in = D.in;
  const uint64_t C = D.C;
  const uint32_t hdr = D.hdr;
  uint32_t* __restrict__ bitmap = S.bitmap;
  uint32_t* __restrict__ cum = S.cum;
  uint64_t* __restrict__ wexit = S.wexit;
  uint64_t* __restrict__ wtotal = S.wtotal;
  const uint32_t lane = threadIdx.x;
  const uint64_t base = hdr + (uint64_t)w * kWin;
  const uint32_t wl = (uint32_t)min((uint64_t)kWin, C - base);
  const uint32_t s = stage(b32, in, C, base, wl + 16, lane);
  for (uint32_t i = lane; i < kWin / 32; i += 64) bm[i] = 0;
  __syncthreads();
  // ---- lane 0's chain (from offset 0) in batches: its tags into the
  // bitmap, each tag's output count before it into cum (K2; the other starts
  // read it back where they meet the chain)
  uint64_t o = 0;
  const uint64_t exit0 = scan_walk<true>(b32, s, wl, 0, o, lane, bm, cum + base);
  const uint64_t total0 = o;
  __syncthreads();
  // ---- the other starts: each lane steps its own chain until it lands on
  // lane 0's (its exit is then lane 0's and its total follows from cum),
  // leaves the window, or passes kEarly bytes.  Starts on one chain that
  // never meets lane 0's (sorted keys: the chain that reads every copy's
  // offset byte as a 3-byte literal) stop at the same first position past
  // kEarly; each such position is walked to the end once, in batches.
  uint64_t p = lane;
  o = 0;
  bool alive = lane > 0 && p < wl;
  bool pending = false, met = false;
  uint64_t ex = lane == 0 ? exit0 : p, tot = lane == 0 ? total0 : 0;
  while (__ballot(alive)) {
    if (alive) {
      if (p < kEarly && ((bm[p >> 5] >> (p & 31)) & 1)) {
        ex = exit0;
        tot = o + total0;  // - cum[p], below
        met = true;
        alive = false;
      } else {
        const Tag t = lds_tag(b32, s + p, p);
        o += t.len;
        p = t.next;
        if (p >= wl) {
          ex = p;
          tot = o;
          alive = false;
        } else if (p >= kEarly) {
          pending = true;
          alive = false;
        }
      }
    }
  }
  // cum[p] where a start met the chain: this wave's own stores above, read
  // once they have landed in L2 (agent scope: not from a line the CU cached)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (met) tot -= __hip_atomic_load(cum + base + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint64_t pm = __ballot(pending); pm; pm = __ballot(pending)) {
    const uint64_t P = lane_of64(p, (uint32_t)__builtin_ctzll(pm));
    uint64_t oP = 0;
    const uint64_t eP = scan_walk<false>(b32, s, wl, P, oP, lane, nullptr, nullptr);
    if (pending && p == P) {
      ex = eP;
      tot = o + oP;
      pending = false;
    }
  }
  wexit[(size_t)w * kStarts + lane] = base + ex;
  wtotal[(size_t)w * kStarts + lane] = tot;
  __syncthreads();
  uint32_t* gb = bitmap + (size_t)w * (kWin / 32);
  for (uint32_t i = lane; i < kWin / 32; i += 64) gb[i] = bm[i];
}


// K3: validate copies and index the tag that starts each output fragment
__device__ void dindex_body(const SnappyDJobs& J, uint32_t ji, uint32_t w, uint32_t* b32) {
  const DJob& D = J.j[ji];
  const DScr S = dscr(J, D, ji);
  uint32_t* __restrict__ flags = S.flags;
  if (flags[1]) return;  // K0 walked and indexed the whole stream
  const uint8_t* __restrict__ in = D.in;
  const uint64_t C = D.C;
  const uint32_t hdr = D.hdr;
  const uint64_t* __restrict__ wentry = S.wentry;
  const uint64_t* __restrict__ woff = S.woff;
  uint64_t* __restrict__ fragpos = S.fragpos;
  const uint32_t lane = threadIdx.x;
  const uint64_t e = wentry[w];
  if (e == kNone || (*flags & kFlagInvalid)) return;
  const uint64_t base = hdr + (uint64_t)w * kWin;
  const uint32_t wl = (uint32_t)min((uint64_t)kWin, C - base);
  {  // the entry tag is a literal that leaves the window (a stored fragment): no staging
    const uint64_t o = woff[w];
    const Tag t = decode_tag(tag_bytes(in, C, e), e);
    if (t.lit && t.next >= base + wl) {
      if (lane == 0) {
        uint32_t fl = 0;
        if ((o & (kFrag - 1)) == 0) fragpos[o / kFrag] = e;
        if (o / kFrag != (o + t.len - 1) / kFrag) fl |= kFlagSerial;
        if (fl) atomicOr(flags, fl);
      }
      return;
    }
  }
  const uint32_t s = stage(b32, in, C, base, wl + 16, lane);
  __syncthreads();
  uint64_t p = e - base, o = woff[w];
  uint32_t fl = 0;
  while (p < wl) {
    // a batch (as in K1): lane l checks the chain's tag at p + l, if any
    const uint64_t pl = min(p + lane, (uint64_t)wl);
    const Tag tl = lds_tag(b32, s + pl, pl);
    const uint64_t adv = tl.next - pl;
    const uint64_t M = batch_mask((uint32_t)min(adv, (uint64_t)64), wl - p, ~0ull);
    const bool tag = (M >> lane) & 1;
    const uint64_t vo = o + wave_excl_sum(tag ? (uint32_t)min(tl.len, (uint64_t)64) : 0u, lane);
    bool inval = false, serial = false;
    if (tag) {
      if (!tl.lit) {
        if (tl.off == 0 || tl.off > vo) inval = true;
        else if (vo - tl.off < (vo & ~(uint64_t)(kFrag - 1))) serial = true;
      }
      if ((vo & (kFrag - 1)) == 0) fragpos[vo / kFrag] = base + pl;
      if (vo / kFrag != (vo + tl.len - 1) / kFrag) serial = true;
    }
    if (__ballot(inval)) fl |= kFlagInvalid;
    if (__ballot(serial)) fl |= kFlagSerial;
    const uint32_t last = 63 - __builtin_clzll(M);
    o = lane_of64(vo, last) + lane_of64(tl.len, last);
    p += last + lane_of64(adv, last);
  }
  if (fl && lane == 0) atomicOr(flags, fl);
}

// K1, K2 and K3 as three ordinary launches: stream order is the barrier
// between them (K1's tables feed K2, K2's window entries feed K3), so no
// workgroup ever waits for another and no co-residency is assumed.  Each
// returns at once when no stream of the batch needs it.
__device__ __forceinline__ void dslow_needs(const SnappyDJobs& J, bool& scan, bool& index) {
  scan = index = false;
  for (uint32_t i = 0; i < J.njobs; ++i) {
    const uint32_t f0 = J.ctrl[8 * i], f1 = J.ctrl[8 * i + 1];
    scan = scan || (f0 & kFlagScan);
    index = index || (!f1 && !(f0 & (kFlagInvalid | kFlagHeader)));
  }
}
// K1: windows of the streams K0 handed over
__global__ __launch_bounds__(64) void snappy_dscan(const SnappyDJobs J) {
  __shared__ uint32_t b32[(kWin + 32) / 4];
  __shared__ uint32_t bm[kWin / 32];
  bool scan, index;
  dslow_needs(J, scan, index);
  if (!scan) return;
  for (uint32_t w = blockIdx.x; w < J.nwin; w += gridDim.x) {
    const uint32_t ji = djob_of(J, w, &DJob::win0);
    dscan_body(J, ji, w - J.j[ji].win0, b32, bm);
  }
}
// K2: one workgroup per stream links its windows
__global__ __launch_bounds__(64) void snappy_dlink(const SnappyDJobs J) {
  __shared__ uint64_t lex[kLinkAhead * kStarts], ltot[kLinkAhead * kStarts];
  for (uint32_t ji = blockIdx.x; ji < J.njobs; ji += gridDim.x) {
    const DScr S = dscr(J, J.j[ji], ji);
    if (*S.flags & kFlagScan) {
      const DJob& D = J.j[ji];
      dlink_body(D.in, D.C, D.hdr, D.dsize, S.bitmap, S.cum, S.wexit, S.wtotal, D.nwin, S.wentry, S.woff, S.flags,
                 lex, ltot);
    }
  }
}
// K2p: the windows linked in parallel, for a stream whose chain enters every
// window at one of its first 64 bytes (tag-dense data: every tag is short).
// Window w's K1 tables are a function on entry offsets: F_w(l) = the next
// window's entry offset (or the stream's end), with T_w(l) output bytes; the
// chain's entries are the prefix compositions of these functions from
// window 0's offset 0.  Three launches compose them in two levels: K2a, one
// wave per block of kLinkPer windows, composes its block's function (lane l
// follows the chain entered at offset l of the block's first window: one lane
// permute per window); K2b, one workgroup per stream, composes the blocks'
// functions into at most kLinkMaxBlocks superblocks (a wave each), walks
// those along the true chain and then re-walks each superblock's blocks to
// record every block's entry; K2c, one wave per block again, re-walks the
// block's windows from its entry and records each window's entry and output
// offset -- what K2's one-chain walk records.  A chain that leaves a window
// anywhere else (a long literal, an entry past the first 64 bytes) leaves the
// stream to K2.  (Round 4: one workgroup per stream did both levels, 0.47 ms
// for 128 MiB of sorted keys in 8 KiB windows, its waves' table loads one
// memory latency per 8 windows.)
constexpr uint32_t kLinkWaves = 16;
constexpr uint32_t kLinkMaxBlocks = 128;
constexpr uint32_t kLinkPer = 16;
constexpr uint32_t kLinkEnd = 64, kLinkOdd = 65;  // F codes besides an entry offset 0..63
__device__ __forceinline__ uint32_t link_code(uint64_t x, uint32_t w, uint32_t nwin, uint32_t hdr, uint64_t C) {
  if (w + 1 == nwin) return x == C ? kLinkEnd : kLinkOdd;
  if (x < hdr) return kLinkOdd;
  const uint64_t r = x - hdr, w2 = r / kWin, off = r - w2 * kWin;
  return (w2 == (uint64_t)w + 1 && off < kStarts) ? (uint32_t)off : kLinkOdd;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)l, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)l, 64);
  return ((uint64_t)hi << 32) | lo;
}
// a stream's linker blocks: F (u8 codes) and T rows, each block's entry and
// output offset; after cum in the stream's scratch (djob_bytes)
struct LinkBlk {
  uint64_t *T, *out;
  uint32_t* entry;
  uint8_t* F;
};
__host__ __device__ __forceinline__ uint32_t link_nblk(uint32_t nwin) { return (nwin + kLinkPer - 1) / kLinkPer; }
__host__ __device__ __forceinline__ LinkBlk link_blk(const DJob& D, const DScr& S) {
  const size_t nb = link_nblk(D.nwin) + 1;
  LinkBlk B;
  B.T = reinterpret_cast<uint64_t*>(S.cum + ((D.C + 1) & ~(uint64_t)1));
  B.out = B.T + nb * kStarts;
  B.entry = reinterpret_cast<uint32_t*>(B.out + nb);
  B.F = reinterpret_cast<uint8_t*>(B.entry + nb);
  return B;
}
// The composition of windows [w0, w1)'s functions applied from entry `cur`
// (lane l: cur = l), with its output count; 8 windows' tables in flight.
__device__ __forceinline__ void link_compose(const DScr& S, uint32_t w0, uint32_t w1, uint32_t nwin, uint32_t hdr,
                                             uint64_t C, uint32_t lane, uint32_t& cur, uint64_t& acc) {
  for (uint32_t wc = w0; wc < w1; wc += 8) {
    uint64_t x[8], t[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint32_t w = min(wc + k, w1 - 1);
      x[k] = S.wexit[(size_t)w * kStarts + lane];
      t[k] = S.wtotal[(size_t)w * kStarts + lane];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      if (wc + k >= w1) break;
      const uint32_t code = link_code(x[k], wc + k, nwin, hdr, C);
      const uint32_t nc = (uint32_t)__shfl((int)code, (int)(cur & 63), 64);
      const uint64_t nt = shfl64(t[k], cur & 63);
      if (cur < kStarts) {
        acc += nt;
        cur = nc;
      } else {
        cur = kLinkOdd;  // (the end is only ever the last window's)
      }
    }
  }
}
// K2a: one wave per linker block
__global__ __launch_bounds__(64) void snappy_dlinka(const SnappyDJobs J) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t g = blockIdx.x; g < J.nblk; g += gridDim.x) {
    const uint32_t ji = djob_of(J, g, &DJob::blk0);
    const DJob& D = J.j[ji];
    const DScr S = dscr(J, D, ji);
    if (!(*S.flags & kFlagScan)) continue;
    const uint32_t b = g - D.blk0, w0 = b * kLinkPer, w1 = min(D.nwin, w0 + kLinkPer);
    if (w0 >= w1) continue;
    uint32_t cur = lane;
    uint64_t acc = 0;
    link_compose(S, w0, w1, D.nwin, D.hdr, D.C, lane, cur, acc);
    const LinkBlk B = link_blk(D, S);
    B.F[(size_t)b * kStarts + lane] = (uint8_t)cur;
    B.T[(size_t)b * kStarts + lane] = acc;
  }
}
// K2b: one workgroup per stream: the blocks' entries along the true chain
__global__ __launch_bounds__(kLinkWaves * 64) void snappy_dlinkb(const SnappyDJobs J) {
  __shared__ uint8_t sF[kLinkMaxBlocks][kStarts];
  __shared__ uint64_t sT[kLinkMaxBlocks][kStarts];
  __shared__ uint32_t s_entry[kLinkMaxBlocks];
  __shared__ uint64_t s_out[kLinkMaxBlocks];
  __shared__ uint32_t s_ok;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t ji = blockIdx.x; ji < J.njobs; ji += gridDim.x) {
    const DJob& D = J.j[ji];
    const DScr S = dscr(J, D, ji);
    if (!(*S.flags & kFlagScan)) continue;  // (uniform: every wave reads the same word)
    const uint32_t nb = link_nblk(D.nwin);
    if (nb == 0) continue;
    const LinkBlk B = link_blk(D, S);
    const uint32_t per = max(8u, (nb + kLinkMaxBlocks - 1) / kLinkMaxBlocks);
    const uint32_t ns = (nb + per - 1) / per;
    // ---- each superblock's composed function
    for (uint32_t sb = wave; sb < ns; sb += kLinkWaves) {
      const uint32_t b0 = sb * per, b1 = min(nb, b0 + per);
      uint32_t cur = lane;
      uint64_t acc = 0;
      for (uint32_t bc = b0; bc < b1; bc += 8) {
        uint32_t f[8];
        uint64_t t[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
          const uint32_t b = min(bc + k, b1 - 1);
          f[k] = B.F[(size_t)b * kStarts + lane];
          t[k] = B.T[(size_t)b * kStarts + lane];
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
          if (bc + k >= b1) break;
          const uint32_t nc = (uint32_t)__shfl((int)f[k], (int)(cur & 63), 64);
          const uint64_t nt = shfl64(t[k], cur & 63);
          if (cur < kStarts) {
            acc += nt;
            cur = nc;
          } else {
            cur = kLinkOdd;
          }
        }
      }
      sF[sb][lane] = (uint8_t)cur;
      sT[sb][lane] = acc;
    }
    __syncthreads();
    // ---- the superblocks' entries along the true chain
    if (threadIdx.x == 0) {
      uint32_t e = 0;
      uint64_t o = 0;
      for (uint32_t sb = 0; sb < ns && e < kStarts; ++sb) {
        s_entry[sb] = e;
        s_out[sb] = o;
        o += sT[sb][e];
        e = sF[sb][e];
      }
      s_ok = e == kLinkEnd ? (o == D.dsize ? 1u : 2u) : 0u;  // 0: K2 walks it
    }
    __syncthreads();
    const uint32_t ok = s_ok;
    if (ok == 1) {
      // ---- every block's entry, from its superblock's
      for (uint32_t sb = wave; sb < ns; sb += kLinkWaves) {
        const uint32_t b0 = sb * per, b1 = min(nb, b0 + per);
        uint32_t e = s_entry[sb];
        uint64_t o = s_out[sb];
        for (uint32_t bc = b0; bc < b1; bc += 8) {
          uint32_t f[8];
          uint64_t t[8];
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t b = min(bc + k, b1 - 1);
            f[k] = B.F[(size_t)b * kStarts + lane];
            t[k] = B.T[(size_t)b * kStarts + lane];
          }
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k) {
            if (bc + k >= b1) break;
            if (lane == 0) {
              B.entry[bc + k] = e;
              B.out[bc + k] = o;
            }
            o += lane_of64(t[k], e);
            e = lane_of(f[k], e);
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      S.flags[3] = ok == 1 ? 1u : 0u;  // K2c's cue
      if (ok) *S.flags = ok == 2 ? kFlagInvalid : 0;  // (K2 then skips the stream)
    }
    __syncthreads();
  }
}
// K2c: one wave per linker block of a stream K2b linked: its windows' entries
// K2c's work for linker block g of the union grid
__device__ void dlinkc_block(const SnappyDJobs& J, uint32_t g) {
  const uint32_t lane = threadIdx.x;
  const uint32_t ji = djob_of(J, g, &DJob::blk0);
  const DJob& D = J.j[ji];
  const DScr S = dscr(J, D, ji);
  if (S.flags[3] != 1) return;
  const uint32_t b = g - D.blk0, w0 = b * kLinkPer, w1 = min(D.nwin, w0 + kLinkPer);
  if (w0 >= w1) return;
  const LinkBlk B = link_blk(D, S);
  uint32_t e = B.entry[b];
  uint64_t o = B.out[b];
  const uint32_t nwin = D.nwin, hdr = D.hdr;
  for (uint32_t wc = w0; wc < w1; wc += 8) {
    uint64_t x[8], t[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint32_t w = min(wc + k, w1 - 1);
      x[k] = S.wexit[(size_t)w * kStarts + lane];
      t[k] = S.wtotal[(size_t)w * kStarts + lane];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      if (wc + k >= w1) break;
      const uint32_t w = wc + k;
      if (lane == 0) {
        S.wentry[w] = hdr + (uint64_t)w * kWin + e;
        S.woff[w] = o;
      }
      const uint32_t code = link_code(x[k], w, nwin, hdr, D.C);
      o += lane_of64(t[k], e);
      e = lane_of(code, e);
    }
  }
}

__global__ __launch_bounds__(64) void snappy_dlinkc(const SnappyDJobs J) {
  for (uint32_t g = blockIdx.x; g < J.nblk; g += gridDim.x) dlinkc_block(J, g);
}
// K3: windows indexed (streams K0 did not walk to the end)
__global__ __launch_bounds__(64) void snappy_dindex(const SnappyDJobs J) {
  __shared__ uint32_t b32[(kWin + 32) / 4];
  bool scan, index;
  dslow_needs(J, scan, index);
  if (!scan && !index) return;
  for (uint32_t w = blockIdx.x; w < J.nwin; w += gridDim.x) {
    const uint32_t ji = djob_of(J, w, &DJob::win0);
    dindex_body(J, ji, w - J.j[ji].win0, b32);
  }
}

// A literal too long for the staging window, read straight into the LDS
// fragment: 16-byte LDS stores to the aligned chunks, each composed from the
// two aligned 16-byte source blocks it straddles; 8 chunks per lane in
// flight (8 KiB per memory latency for the wave), bytes at the edges.
__device__ void literal_to_lds(uint8_t* ob, uint32_t o, const uint8_t* __restrict__ in, uint64_t src, uint32_t L,
                               uint32_t lane) {
  constexpr uint32_t M = kRing - 1;  // ob is the ring: 16-byte chunks never straddle its end
  const uint32_t head = (16 - (o & 15)) & 15;
  if (head >= L) {
    for (uint32_t i = lane; i < L; i += 64) ob[(o + i) & M] = in[src + i];
    return;
  }
  if (lane < head) ob[(o + lane) & M] = in[src + lane];
  const uint32_t nc = (L - head) >> 4;
  const uintptr_t sp = reinterpret_cast<uintptr_t>(in + src + head);
  typedef uint32_t V4 __attribute__((ext_vector_type(4)));
  const auto s16 = gbl<V4>(reinterpret_cast<const void*>(sp & ~(uintptr_t)15));  // global, not flat, loads
  const uint32_t sh = (uint32_t)(sp & 15);
  const uint32_t o16 = o + head;  // 16-aligned
  constexpr int U = 2;  // (registers: K4's occupancy)
  for (uint32_t c0 = 0; c0 < nc; c0 += U * 64) {
    uint4 lo[U], hi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t c = c0 + u * 64 + lane;
      V4 x = {0, 0, 0, 0};
      if (c < nc) x = s16[c];
      V4 y = x;
      if (c < nc && sh) y = s16[c + 1];
      lo[u] = make_uint4(x[0], x[1], x[2], x[3]);
      hi[u] = make_uint4(y[0], y[1], y[2], y[3]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t c = c0 + u * 64 + lane;
      if (c < nc) *reinterpret_cast<uint4*>(ob + ((o16 + 16 * c) & M)) = funnel16(lo[u], hi[u], sh);
    }
  }
  const uint32_t t0 = head + 16 * nc;
  if (lane < L - t0) ob[(o + t0 + lane) & M] = in[src + t0 + lane];
}

// The ring's bytes [from, to) of the fragment to d (from a multiple of 16 or
// to the fragment's end), by one wave.
__device__ __forceinline__ void ring_flush(const uint8_t* ring, uint8_t* __restrict__ d, uint32_t from, uint32_t to,
                                           uint32_t lane) {
  constexpr uint32_t M = kRing - 1;
  uint32_t i = from;
  if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
    const uint32_t c1 = to >> 4;
    for (uint32_t c = (from >> 4) + lane; c < c1; c += 64)
      reinterpret_cast<uint4*>(d)[c] = *reinterpret_cast<const uint4*>(ring + ((16 * c) & M));
    i = max(from, c1 << 4);
  }
  for (i += lane; i < to; i += 64) d[i] = ring[i & M];
}
// Byte x of the fragment d, flushed from the ring by this wave before: an
// agent-scope load after the wave's stores have landed in L2 (a plain load
// could hit a line this CU cached while the byte was not yet written).
__device__ __forceinline__ uint8_t flushed_byte(const uint8_t* d, uint32_t x) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uintptr_t a = reinterpret_cast<uintptr_t>(d + x);
  const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return (uint8_t)(w >> (8 * (a & 3)));
}

// K5 body: the verdict; one-lane decode of valid streams K4 could not split
__device__ void dserial_body(const uint8_t* __restrict__ in, uint64_t C, uint32_t hdr, uint8_t* __restrict__ out) {
  uint64_t p = hdr, o = 0;
  while (p < C) {
    const Tag t = decode_tag(tag_bytes(in, C, p), p);
    if (t.lit) {
      for (uint64_t i = 0; i < t.len; ++i) out[o + i] = in[p + t.hl + i];
    } else {
      for (uint64_t i = 0; i < t.len; ++i) out[o + i] = out[o - t.off + i];
    }
    o += t.len;
    p = t.next;
  }
}
__device__ void dverdict(uint32_t f, uint64_t dsize, PubSlot* pub, uint32_t ticket) {
  if (pub) {
    pub_store(&pub->status, (int32_t)((f & kFlagHeader) ? kErrHeaderHint : (f & kFlagInvalid) ? kErrCheck : kOk));
    pub_store(&pub->size, (uint64_t)dsize);
    publish_ticket(pub, ticket);
  }
}

// K4: one workgroup per 64 KiB output fragment whose true position differs
// from the one K-spec assumed.  A fragment stored as one literal is copied by
// all 256 lanes; any other is decoded by wave 0 through an 8 KiB LDS ring of
// its output (tags and short literals read from a staged window of the
// compressed bytes; the ring flushed to the output as it fills).  The small
// LDS footprint and 64 registers let 8 workgroups share a CU: a decode is one
// wave's dependent chain of LDS and lane operations, so the chip's 2048
// decoders (one round for 128 MiB) set the rate -- with the whole fragment in
// LDS, 2 per CU, sorted keys decoded at 11.2 GB/s, with the ring 18.3.  The
// last workgroup to finish gives the verdict (K5).
__global__ __launch_bounds__(256, 8) void snappy_dfrag(const SnappyDJobs J) {
  __shared__ uint32_t ob32[kRing / 4];
  __shared__ uint32_t ib32[(kInWin + 32) / 4];
  __shared__ uint32_t s_last;
  __shared__ FewLds F;
  __shared__ double s_lut[256];  // fused decode, nb = 1
  const uint32_t ji = djob_of(J, blockIdx.x, &DJob::fo0);
  const DJob& D = J.j[ji];
  const DScr S = dscr(J, D, ji);
  const uint32_t* __restrict__ flags = S.flags;
  const uint8_t* __restrict__ in = D.in;
  uint8_t* __restrict__ out = D.out;
  const uint64_t C = D.C, dsize = D.dsize;
  const uint32_t hdr = D.hdr, ticket = D.ticket;
  const uint32_t tid = threadIdx.x, k = blockIdx.x - D.fo0;
  const uint64_t o0 = (uint64_t)k * kFrag;
  const uint32_t end = (uint32_t)min((uint64_t)kFrag, dsize - o0);
  if (flags[2]) {  // K-spec decoded the whole stream and gave the verdict
    if (D.fv && end && !S.fdone[k]) {  // a fragment it placed as codes: their values
      dq_prepare(D, s_lut, tid);
      dq_frag<8>(D, out + o0, o0, end, s_lut, tid);
    }
    return;
  }
  const uint64_t* __restrict__ fragpos = S.fragpos;
  const uint64_t* __restrict__ specpos = S.specpos;
  PubSlot* pub = J.pub ? J.pub + D.slot : nullptr;
  const uint32_t f = flags[0];
  uint8_t* ob = reinterpret_cast<uint8_t*>(ob32);
  PSF_DTRACE(k, 0);
  const uint64_t p0 = end ? fragpos[k] : kNone;
  const bool redo = f == 0 && end && p0 != specpos[k];
  if (redo) {
    PSF_DTRACE(k, 1);
    const Tag t0 = decode_tag(tag_bytes(in, C, p0), p0);
    if (decode_few<4>(in, C, p0, end, out + o0, tid, F) != kNone) {
      // (a fragment of a few tags: done)
    } else if (t0.lit && t0.len == end) {
      copy_g2g<4>(out + o0, in + p0 + t0.hl, end, tid);
    } else {
      if (tid < 64) {
        const uint32_t lane = tid;
        constexpr uint32_t kSpan = kInWin + 16;  // staged bytes [wb, wb + kSpan)
        constexpr uint32_t RM = kRing - 1;
        uint8_t* const d = out + o0;
        uint64_t p = p0, wb = p0;
        uint32_t s = stage(ib32, in, C, wb, kSpan, lane);
        uint32_t o = 0, flushed = 0;
        const uint8_t* ibb = reinterpret_cast<const uint8_t*>(ib32);
        while (o < end) {
          if (o - flushed > kRingFlushAt) {
            ring_flush(ob, d, flushed, o & ~15u, lane);
            flushed = o & ~15u;
          }
          if (p + kBatchMargin > wb + kSpan) {
            wb = p;
            s = stage(ib32, in, C, wb, kSpan, lane);
          }
          // ---- a batch: the tags that start in [p, p + 64).  Every lane
          // decodes the tag that would start at p + lane; one scalar walk
          // marks the chain's tag starts (batch_mask) and one wave prefix sum
          // gives each its output offset; then every literal of the batch is
          // written at once (by the lane of its tag) and the copies one after
          // another in tag order (a
          // copy reads only output before it: earlier literals, done, and
          // earlier copies, done in order).  The walk stops at the
          // fragment's end and before a tag it does not take (a literal
          // longer than kBatchLit bytes); that one goes the single way below.
          {
            const uint32_t qb = s + (uint32_t)(p - wb);
            const Tag tl = lds_tag(ib32, qb + lane, p + lane);
            const uint32_t adv = (uint32_t)min(tl.next - (p + lane), (uint64_t)64);
            const uint32_t tlen = (uint32_t)min(tl.len, (uint64_t)64);
            const uint64_t M0 = batch_mask(adv, 64, __ballot(!tl.lit || tl.len <= kBatchLit));
            const bool tag0 = (M0 >> lane) & 1;
            const uint32_t vo = o + wave_excl_sum(tag0 ? tlen : 0u, lane);
            const uint64_t M = M0 & __ballot(vo < end);  // tags past the fragment's end are not its own
            if (M) {
              const bool tag = (M >> lane) & 1;
              const uint32_t last = 63 - __builtin_clzll(M);
              const uint32_t oend = lane_of(vo, last) + lane_of(tlen, last);
              if (tag && tl.lit) {
                const uint8_t* q = ibb + qb + lane + tl.hl;
                for (uint32_t j = 0; j < tlen; ++j) ob[(vo + j) & RM] = q[j];
              }
              for (uint64_t cm = __ballot(tag && !tl.lit); cm; cm &= cm - 1) {
                const uint32_t k = (uint32_t)__builtin_ctzll(cm);
                const uint32_t ko = lane_of(vo, k), L = lane_of(tlen, k), off = lane_of(tl.off, k);
                if (off >= L) {
                  if (ko - off + kRing >= oend) {
                    if (lane < L) ob[(ko + lane) & RM] = ob[(ko - off + lane) & RM];
                  } else {  // older than the ring: flushed
                    const uint8_t b = flushed_byte(d, ko - off + min(lane, L - 1));
                    if (lane < L) ob[(ko + lane) & RM] = b;
                  }
                } else if (lane < L) {
                  ob[(ko + lane) & RM] = ob[(ko - off + lane % off) & RM];
                }
              }
              o = oend;
              p += last + lane_of(adv, last);
              if (o >= end || last + lane_of(adv, last) >= 64) continue;
            }
          }
          // ---- one tag the general way (a step of its own)
          if (o - flushed > kRingFlushAt) {
            ring_flush(ob, d, flushed, o & ~15u, lane);
            flushed = o & ~15u;
          }
          const Tag t = lds_tag(ib32, s + (p - wb), p);
          const uint32_t L = (uint32_t)t.len;
          if (t.lit) {
            const uint64_t src = p + t.hl;
            if (src + L > wb + kSpan && L <= kInWin) {
              wb = src;
              s = stage(ib32, in, C, wb, kSpan, lane);
            }
            const bool staged = src + L <= wb + kSpan;
            for (uint32_t q0 = 0; q0 < L; q0 += kRingStep) {  // pieces of one step each
              const uint32_t n = min(L - q0, kRingStep), oq = o + q0;
              if (oq - flushed > kRingFlushAt) {
                ring_flush(ob, d, flushed, oq & ~15u, lane);
                flushed = oq & ~15u;
              }
              if (staged) {
                const uint8_t* q = reinterpret_cast<const uint8_t*>(ib32) + s + (src - wb) + q0;
                for (uint32_t i = lane; i < n; i += 64) ob[(oq + i) & RM] = q[i];
              } else {
                literal_to_lds(ob, oq, in, src + q0, n, lane);
              }
            }
          } else if (t.off >= L) {  // (L <= 64)
            if (o - t.off + kRing >= o + L) {
              if (lane < L) ob[(o + lane) & RM] = ob[(o - t.off + lane) & RM];
            } else {
              const uint8_t b = flushed_byte(d, o - t.off + min(lane, L - 1));
              if (lane < L) ob[(o + lane) & RM] = b;
            }
          } else if (lane < L) {
            ob[(o + lane) & RM] = ob[(o - t.off + lane % t.off) & RM];
          }
          o += L;
          p = t.next;
        }
        ring_flush(ob, d, flushed, end, lane);
      }
    }
  }
  if (D.fv && f == 0 && end && (redo || !S.fdone[k])) {  // values of the codes placed here or by K-spec
    __syncthreads();
    dq_prepare(D, s_lut, tid);
    dq_frag<8>(D, out + o0, o0, end, s_lut, tid);
  }
  PSF_DTRACE(k, 2);
  if (!last_block(S.ctr + 2, D.nfo ? D.nfo : 1, &s_last)) return;
  if (f == kFlagSerial) {
    if (tid == 0) dserial_body(in, C, hdr, out);
    if (D.fv) {
      __syncthreads();
      dq_prepare(D, s_lut, tid);
      for (uint64_t o = 0; o < dsize; o += kFrag) dq_frag<8>(D, out + o, o, (uint32_t)min((uint64_t)kFrag, dsize - o), s_lut, tid);
    }
    __syncthreads();
  }
  if (tid == 0) dverdict(f, dsize, pub, ticket);
}

}  // namespace
}  // namespace psf

// FIXING_FLOAT codec for gfx950 (CDNA4): the host launch layer of the kernels
// in ff_kernels.h, one translation unit with them.  Single arrays (nb 1..7)
// and batches of up to kFfBatchMax aligned arrays of one type and nb 1..3;
// every launch picks its kernel instantiation through ff_dispatch.h.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "ff_kernels.h"
#include "ff_dispatch.h"

namespace psf {

// an integer A/B knob of the environment; unset or not a number: dflt
// (each knob keeps the value in a function-local static: parsed once)
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  if (!e) return dflt;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  return end == e ? dflt : (int)v;
}

// ------------------------------------------------------------ LCG tables ---
static inline void lcg_affine_pow(uint64_t k, uint32_t& A, uint32_t& Cc) {
  uint32_t a = kLcgA, c = kLcgC;
  A = 1u; Cc = 0u;
  while (k) {
    if (k & 1) { A = a * A; Cc = a * Cc + c; }
    c = a * c + c;
    a = a * a;
    k >>= 1;
  }
}

// Only bit 16 of the LCG state is ever observed, and (a*s + c) mod 2^17
// depends only on s mod 2^17, so the encoder reads its bits off the LCG modulo
// 2^17, which is one cycle of length 2^17 (a = 1 mod 4, c odd).  Host side:
// the cycle x_0 = 0, x_{k+1} = a x_k + c, the position of every residue on it, and
// per device a bit table T[k] = !bit16(x_k) for k < 2^17 + 64 (wrapped), 16 KiB.
namespace {
struct LcgCycle {
  std::vector<uint32_t> pos;   // pos[x] = k with x_k = x
  std::vector<uint32_t> bits;  // T, packed 32 per word, LSB first
  LcgCycle() : pos(1u << 17), bits(((1u << 17) + 64) / 32, 0u) {
    uint32_t x = 0;
    for (uint32_t k = 0; k < (1u << 17); ++k) {
      pos[x] = k;
      x = (kLcgA * x + kLcgC) & kMask17;
    }
    x = 0;
    for (uint32_t k = 0; k < (1u << 17) + 64; ++k) {
      if (((~x) >> 16) & 1u) bits[k >> 5] |= 1u << (k & 31);
      x = (kLcgA * x + kLcgC) & kMask17;
    }
  }
};
const LcgCycle& lcg_cycle() {
  static const LcgCycle c;
  return c;
}
std::mutex g_lcg_mu;
std::map<int, uint32_t*> g_lcg_dev;  // per device, allocated once, never freed
}  // namespace

static const uint32_t* lcg_bits_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> l(g_lcg_mu);
  auto it = g_lcg_dev.find(dev);
  if (it != g_lcg_dev.end()) return it->second;
  const LcgCycle& c = lcg_cycle();
  uint32_t* d = nullptr;
  if (hipMalloc(&d, c.bits.size() * sizeof(uint32_t)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, c.bits.data(), c.bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  g_lcg_dev[dev] = d;
  return d;
}

// ----------------------------------------------------------------- grids ---
double ff_ratio(int nb) {
  // fixing_float.h:55 -- 32-bit int shift, count masked to 5 bits on x86
  int32_t one_shifted = (int32_t)(1u << ((unsigned)(nb * 8) & 31u));
  return (double)one_shifted - 2.0;
}

int ff_grid(size_t work_items) {
  size_t g = (work_items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > (size_t)kMaxGrid) g = kMaxGrid;
  return (int)g;
}

static size_t tiles_of(size_t n) { return ((n >> 2) + kTileGroups - 1) / kTileGroups; }

static int tile_grid(size_t n, int cap) {
  const size_t ntiles = tiles_of(n);
  size_t g = ntiles < 1 ? 1 : ntiles;
  if (g > (size_t)cap) g = cap;
  return (int)g;
}

// the vector kernels' alignment: 16-byte values, 4-byte (nb = 2: 8-byte) codes
static bool vec_aligned(const void* values, const void* codes, int nb) {
  return (reinterpret_cast<uintptr_t>(values) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(codes) & (nb == 2 ? 7 : 3)) == 0;
}

// ---------------------------------------------------- single-array encode ---
// PSF_ENC_PERM (A/B knob; its script and record are not kept): 0 keeps the
// min/max pass in contiguous runs per workgroup and the encode in tile order.
// On (default): the strided min/max pass sweeps the array front to back (2^28:
// 159 -> 156 us) and the encode starts from the end it read last; the Infinity
// Cache share that buys is small (encode 220 -> 222 us at 2^28, the 2^27 line
// 1743 -> 1768 GiB/s).  (Interleaving the encode over the min/max runs' last
// chunks instead cost it 219 -> 237 us.)
static bool enc_perm_mode() {
  static const bool on = env_int("PSF_ENC_PERM", 1) != 0;
  return on;
}

// the LCG jump constants of an encode launch over `grid` workgroups
static void encode_lcg_params(EncodeParams& p, int grid) {
  lcg_affine_pow((uint64_t)grid * kBlock, p.a_thr, p.c_thr);
  p.lcg_pos = lcg_cycle().pos[p.seed & kMask17];
}

template <typename V, int NB, bool kVec>
static void launch_encode(const V* x, size_t n, uint8_t* out, EncodeParams p, hipStream_t st) {
  const int grid = kVec ? tile_grid(n, kStreamGrid) : ff_grid(n);
  // after a strided min/max pass over an array larger than the Infinity
  // Cache (smaller ones stay on chip whatever the order, and the reversed
  // order cost C3's 40 MB arrays 9 %: encode 15.8 -> 17.8 us)
  p.reverse = kVec && p.partials && enc_perm_mode() && (double)n * sizeof(V) > 256.0 * (1 << 20) ? 1u : 0u;
  encode_lcg_params(p, grid);
  psf_launch((ff_encode<V, NB, kVec>), dim3(grid), dim3(kBlock), 0, st, x, n, out, p);
}

int ff_encode_launch(const void* x, size_t n, int value_type, int nb, const FixedPoint& preset,
                     uint32_t seed, void* out, void* partials, float* range_out, int* status_out,
                     hipStream_t st, Profiler* prof, PubSlot* pub, uint32_t ticket, float* range_host) {
  if (nb <= 0 || nb > kNbMax) return kErrNbytes;
  if (n == 0) return kOk;
  EncodeParams p{};
  p.range_host = range_host;
  p.pub = pub;
  p.ticket = ticket;
  p.has_min = preset.has_min;
  p.has_max = preset.has_max;
  p.preset_min = preset.min_value;
  p.preset_max = preset.max_value;
  p.seed = seed;
  p.ratio = ff_ratio(nb);
  p.range_out = range_out;
  p.status_out = status_out;
  const bool vec = vec_aligned(x, out, nb);
  return with_value_type(value_type, [&](auto v) {
    using V = decltype(v);
    const V* xv = static_cast<const V*>(x);
    if (!(preset.has_min && preset.has_max)) {
      const int grid = vec ? tile_grid(n, kMinmaxGrid) : (ff_grid(n) < kMinmaxGrid ? ff_grid(n) : kMinmaxGrid);
      ProfScope ps(prof, kKMinmax, st, (double)n * sizeof(V), true);
      if (vec)
        psf_launch((ff_minmax_partials<V, true>), dim3(grid), dim3(kBlock), 0, st, xv, n, partials,
                   1u);  // strided at every size: C3 (40 MB) 3756 -> 3837 GiB/s
      else
        psf_launch((ff_minmax_partials<V, false>), dim3(grid), dim3(kBlock), 0, st, xv, n, partials, 0u);
      p.partials = partials;
      p.nparts = grid;
      if (launch_status() != kOk) return kErrHip;
    }
    ProfScope ps(prof, kKEncode, st, (double)n * (sizeof(V) + nb), true);
    p.lcg_bits = lcg_bits_device();
    if (!p.lcg_bits) return kErrHip;
    const int s = with_bool(vec, [&](auto kv) {
      return with_nb<1, kNbMax>(nb, [&](auto N) {
        launch_encode<V, decltype(N)::value, decltype(kv)::value>(xv, n, static_cast<uint8_t*>(out), p, st);
        return kOk;
      });
    });
    return s == kOk ? launch_status() : s;
  });
}

// ---------------------------------------------------- single-array decode ---
template <typename V, int NB, bool kVec>
static void launch_decode(const uint8_t* code, size_t n, V* out, const DecodeParams& p, hipStream_t st) {
  static_assert(!kVec || ff_has_vec_decode(NB), "no vector decode at this num_bytes");
  // arrays of >= 2 x kDecodeGridBig tiles (2^28 values) decode on twice the
  // stream grid, 2 tiles per workgroup: decode 193-194 -> 189 us at 2^28
  // (r02); the encode and smaller arrays measured no gain from it (2^27 on
  // one tile per workgroup: -2.5 %)
  const int cap = tiles_of(n) >= 2 * (size_t)kDecodeGridBig ? kDecodeGridBig : kStreamGrid;
  const int grid = kVec ? tile_grid(n, cap) : ff_grid(n);
  psf_launch((ff_decode<V, NB, kVec>), dim3(grid), dim3(kBlock), 0, st, code, n, out, p);
}

int ff_decode_launch(const void* code, size_t n, int value_type, int nb, const float* range,
                     float mn, float mx, void* out, hipStream_t st, Profiler* prof) {
  if (nb <= 0 || nb > kNbMax) return kErrNbytes;
  if (n == 0) return kOk;
  return with_value_type(value_type, [&](auto v) {
    using V = decltype(v);
    const DecodeParams p{range, mn, mx, ff_ratio(nb)};
    const bool vec = vec_aligned(out, code, nb);
    const uint8_t* c = static_cast<const uint8_t*>(code);
    V* o = static_cast<V*>(out);
    ProfScope ps(prof, kKDecode, st, (double)n * (nb + sizeof(V)), true);
    const int s = with_bool(vec, [&](auto kv) {
      return with_nb<1, kNbMax>(nb, [&](auto N) {
        constexpr int NB = decltype(N)::value;
        launch_decode<V, NB, decltype(kv)::value && ff_has_vec_decode(NB)>(c, n, o, p, st);
        return kOk;
      });
    });
    return s == kOk ? launch_status() : s;
  });
}

// ------------------------------------------------------ batched launchers ---
bool ff_batchable(const void* x, const void* out, size_t n, int nb, int value_type, bool encode) {
  if (nb < 1 || nb > kBatchNbMax || n == 0 || n >= (1ull << 32)) return false;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
  const uintptr_t code_align = nb == 2 ? 7 : 3;
  // encode: values element-aligned (slices of a value array, message.h:141-143,
  // start at any element; the batched kernels load unaligned groups element
  // by element), codes aligned for the packed stores
  const uintptr_t elem_align = value_type == kDouble ? 7 : 3;
  return encode ? ((xa & elem_align) == 0 && (oa & code_align) == 0)
                : ((oa & 15) == 0 && (xa & code_align) == 0);
}

// the batched min/max pass's grid (shared by its arrays by tiles): larger than
// the single-array one -- 4096 measured 9 % faster than 1024 on C4's 512 x 1 MiB
// slices (8192: 4 % more), where 1024 is best for one 1 GiB array (r02)
#ifndef PSF_BATCH_MINMAX_GRID
#define PSF_BATCH_MINMAX_GRID 16384  // r06: 16384 against 8192 on C4, min/max 86.8 -> 83.3 us (4786 -> 4803 GiB/s; 32768: 91.6)
#endif
constexpr int kBatchMinmaxGrid = PSF_BATCH_MINMAX_GRID;
#ifndef PSF_BATCH_STREAM_GRID
#define PSF_BATCH_STREAM_GRID 16384  // the batched encode grid: 16384 measured 4 % faster than 8192 on C4
#endif
constexpr int kBatchStreamGrid = PSF_BATCH_STREAM_GRID;
static_assert(kBatchMinmaxGrid <= 0xFFFF, "FfJob::mm_nwg is 16 bits");

// fewest tiles per workgroup in the batched min/max and encode grids
#ifndef PSF_BATCH_MM_TPW
#define PSF_BATCH_MM_TPW 1
#endif
#ifndef PSF_BATCH_ENC_TPW
#define PSF_BATCH_ENC_TPW 2  // 2 measured 10 % faster than 1 on 64 x 1 MiB batches (r02)
#endif
#ifndef PSF_BATCH_DEC_TPW
#define PSF_BATCH_DEC_TPW 1  // one tile per workgroup measured best for decode
#endif
constexpr size_t kBatchMmTpw = PSF_BATCH_MM_TPW, kBatchEncTpw = PSF_BATCH_ENC_TPW, kBatchDecTpw = PSF_BATCH_DEC_TPW;
// at most this many min/max workgroups per array: every encode workgroup of
// the array folds all of its partials before it quantises, so a few large
// arrays (C5: 8 x 2^24 values, 1024 partials each from the 8192 grid) pay for
// the fold in every one of their ~2048 encode workgroups (C5: 128 per array
// gives encode 116 us against 131 at 1024, min/max 84 -- the 1024-workgroup
// total the single-array kernel uses for one 1 GiB array; C4's 512 small
// arrays get 16 each and are unaffected)
#ifndef PSF_BATCH_MM_PER_ARRAY
#define PSF_BATCH_MM_PER_ARRAY 128
#endif
constexpr uint32_t kBatchMmPerArray = PSF_BATCH_MM_PER_ARRAY;

// Workgroups of one array in a batched launch: its share (by tiles) of the
// grid the single-array kernel would use, at least one.  A batch of large
// arrays then runs several tiles per workgroup as the single kernels do
// instead of one workgroup per tile (C4: 32 x 2^21 values).
static int share_grid(size_t n, size_t tiles_total, int cap) {
  const size_t t = tiles_of(n);
  size_t c = tiles_total ? ((size_t)cap * t + tiles_total - 1) / tiles_total : (size_t)cap;
  if (c < 1) c = 1;
  if (c > (size_t)cap) c = cap;
  return tile_grid(n, (int)c);
}

// an upper bound of the min/max workgroups of ff_encode_batch_launch (each
// array's share_grid is at most its tile_grid)
size_t ff_batch_partials_bytes(const FfArray* arrs, int count) {
  size_t wgs = 0;
  for (int i = 0; i < count; ++i)
    if (!(arrs[i].preset.has_min && arrs[i].preset.has_max)) wgs += tile_grid(arrs[i].n, kBatchMinmaxGrid);
  return 2 * sizeof(uint64_t) * (wgs + 1);
}

// PSF_MM_REVERSE (A/B knob; its script is not kept): 1 runs the batched
// min/max pass back to front; 0 or unset: never
static bool mm_reverse_mode() {
  static const bool on = env_int("PSF_MM_REVERSE", 0) == 1;
  return on;
}

// PSF_FF_FUSED (A/B knob; its script is not kept): 0 keeps a small batch's
// min/max and encode in two launches
static bool fused_mode() {
  static const bool on = env_int("PSF_FF_FUSED", 1) != 0;
  return on;
}
// ff_fused_batch only for batches of at most this many encode workgroups:
// its waiting workgroups hold their slots (and poll), which a launch-bound
// batch of small arrays (C1: 832) does not notice and one of large arrays
// does (C5, 8 x 2^24 values, 16384 workgroups: 1.08 ms against 0.20 in two
// launches, r04).  1024 keeps the grid about within one round of resident
// workgroups (5 per CU at its registers); sizes between (C4's 64 slices per
// rank at N = 8: 2048) are unmeasured and keep two launches.
constexpr uint32_t kFusedMaxEncWgs = 1024;
// tiles per decode workgroup inside ff_fused_batch: 4 (C1, r04; the A/B
// script is not kept: the fused kernel 28.1-28.8 us at 1, 27.4-28.5 at 2,
// 25.6-26.7 at 4, 25.6-26.1 at 8; fewer, longer decode workgroups leave the
// encode ones their slots sooner); A/B knob PSF_FUSED_DEC_TPW, 1..16
static size_t fused_dec_tpw() {
  static const int t = env_int("PSF_FUSED_DEC_TPW", 4);
  return t >= 1 && t <= 16 ? (size_t)t : (size_t)4;
}

// Host staging of a batched launch's kernel arguments: one per batch size
// and role, used under its lock (launches are serialised per thread).  The
// pending-decode stage is taken inside the encode one, never the reverse.
enum StageRole { kStageEncode, kStageDecode, kStagePendingDecode };
template <int CAP>
struct FfStage {
  std::mutex mu;
  FfBatchT<CAP> B;
};
template <int CAP, StageRole ROLE>
static FfStage<CAP>& stage() {
  static FfStage<CAP> s;
  return s;
}

template <int CAP>
static void reset_batch(FfBatchT<CAP>& B) {
  memset(&B, 0, sizeof(B));
  for (int i = 0; i < CAP; ++i) B.first[i] = B.mm_first[i] = ~0u;
}

// a decode batch's kernel arguments, `tpw` tiles per workgroup at least
template <int CAP>
static int fill_decode_batch(FfBatchT<CAP>& B, size_t vsz, int nb, const FfDecArray* arrs, int count,
                             double* bytes_out, size_t tpw) {
  reset_batch(B);
  B.njobs = count;
  B.ratio = ff_ratio(nb);
  uint32_t wg = 0;
  double bytes = 0;
  for (int i = 0; i < count; ++i) {
    if (arrs[i].n >= (1ull << 32)) return kErrArg;
    FfJob& J = B.job[i];
    J.x = arrs[i].code;
    J.out = arrs[i].out;
    J.n = (uint32_t)arrs[i].n;
    J.mn = arrs[i].mn;
    J.mx = arrs[i].mx;
    J.u.range = arrs[i].range;
    B.first[i] = wg;
    wg += std::min<uint32_t>((uint32_t)tile_grid(arrs[i].n, kStreamGrid),
                             (uint32_t)std::max<size_t>(1, (tiles_of(arrs[i].n) + tpw - 1) / tpw));
    bytes += (double)arrs[i].n * (vsz + nb);
  }
  B.total = wg;
  *bytes_out = bytes;
  return kOk;
}

// an encode batch's kernel arguments (B.total encode and B.mm_total min/max
// workgroups), the bytes its passes move and whether any array is stored
struct EncodeBatchInfo {
  double bytes_mm = 0, bytes_enc = 0;
  bool stored = false;
};
template <int CAP>
static int fill_encode_batch(FfBatchT<CAP>& B, size_t vsz, int nb, const FfArray* arrs, int count, void* partials,
                             PubSlot* pub_base, EncodeBatchInfo* info) {
  reset_batch(B);
  B.njobs = count;
  B.partials = partials;
  B.pub = pub_base;
  B.lcg_bits = lcg_bits_device();
  if (!B.lcg_bits) return kErrHip;
  B.ratio = ff_ratio(nb);
  uint32_t mm = 0, enc = 0;
  size_t tiles_mm = 0, tiles_all = 0;
  for (int i = 0; i < count; ++i) {
    tiles_all += tiles_of(arrs[i].n);
    if (!(arrs[i].preset.has_min && arrs[i].preset.has_max)) tiles_mm += tiles_of(arrs[i].n);
  }
  // the lazy jobs' records are 16-byte entries of one device array and one
  // host-mapped ring (one RangeBatch per encode call, filters.cc): kept as a
  // base pointer each plus a per-job index
  for (int i = 0; i < count; ++i) {
    if (arrs[i].range && (!B.range_base || arrs[i].range < B.range_base)) {
      B.range_base = arrs[i].range;
      B.ring_base = arrs[i].range_host;
    }
  }
  for (int i = 0; i < count; ++i) {
    const FfArray& a = arrs[i];
    FfJob& J = B.job[i];
    if (a.n >= (1ull << 32) || a.slot < -1 || a.slot >= 0xFFFF) return kErrArg;
    J.x = a.x;
    J.out = a.out;
    J.n = (uint32_t)a.n;
    J.mn = a.preset.min_value;
    J.mx = a.preset.max_value;
    J.flags = (a.preset.has_min ? 1u : 0u) | (a.preset.has_max ? 2u : 0u) | ((uint32_t)(a.slot + 1) << 16);
    if (a.stored) {
      if (!ff_has_stored(nb) || (reinterpret_cast<uintptr_t>(a.out) & 3)) return kErrArg;
      J.flags |= kFlagStored;
      info->stored = true;
    }
    J.u.e.seed = a.seed;
    J.u.e.lcg_pos = lcg_cycle().pos[a.seed & kMask17];
    J.ticket = a.ticket;
    J.lazy = kNoLazy;
    if (a.range) {
      const ptrdiff_t k = a.range - B.range_base;
      if (k % 4 || k / 4 >= kNoLazy) return kErrArg;
      const bool ring_ok = B.ring_base ? a.range_host == B.ring_base + k : a.range_host == nullptr;
      if (!ring_ok) return kErrArg;
      J.lazy = (uint16_t)(k / 4);
    } else if (a.range_host) {
      return kErrArg;
    }
    uint32_t mm_nwg =
        (a.preset.has_min && a.preset.has_max) ? 0u : (uint32_t)share_grid(a.n, tiles_mm, kBatchMinmaxGrid);
    if (mm_nwg > 1) mm_nwg = std::min<uint32_t>(mm_nwg, (uint32_t)((tiles_of(a.n) + kBatchMmTpw - 1) / kBatchMmTpw));
    mm_nwg = std::min(mm_nwg, kBatchMmPerArray);
    J.mm_nwg = (uint16_t)mm_nwg;
    B.mm_first[i] = mm;
    mm += mm_nwg;
    B.first[i] = enc;
    enc += std::min<uint32_t>((uint32_t)share_grid(a.n, tiles_all, kBatchStreamGrid),
                              (uint32_t)std::max<size_t>(1, (tiles_of(a.n) + kBatchEncTpw - 1) / kBatchEncTpw));
    if (mm_nwg) info->bytes_mm += (double)a.n * vsz;
    info->bytes_enc += (double)a.n * (vsz + nb);
  }
  B.total = enc;
  B.mm_total = mm;
  B.mm_reverse = mm_reverse_mode() ? 1u : 0u;
  return kOk;
}

// the batched kernels' tags: kOk, or the dispatch's own error before anything is staged
static int check_batch_tags(int value_type, int nb) {
  return with_type_nb<1, kBatchNbMax>(value_type, nb, [](auto, auto) { return kOk; });
}
static size_t value_size(int value_type) { return value_type == kFloat ? 4 : 8; }

template <int CAP>
static int encode_batch_cap(int value_type, int nb, const FfArray* arrs, int count, void* partials,
                            PubSlot* pub_base, hipStream_t st, Profiler* prof, const FfDecArray* dec, int ndec,
                            int dec_nb, FfFusedCtl* fused) {
  FfStage<CAP>& S = stage<CAP, kStageEncode>();
  std::lock_guard<std::mutex> lock(S.mu);
  FfBatchT<CAP>& B = S.B;
  EncodeBatchInfo info;
  const size_t vsz = value_size(value_type);
  const int fs = fill_encode_batch(B, vsz, nb, arrs, count, partials, pub_base, &info);
  if (fs != kOk) return fs;
  if constexpr (ff_has_fused(CAP)) {
    FfStage<kBatchSmall>& P = stage<kBatchSmall, kStagePendingDecode>();
    std::lock_guard<std::mutex> plock(P.mu);
    FfBatchT<kBatchSmall>& D = P.B;
    double bytes_dec = 0;
    // min/max, encode and the pending decode (same num_bytes) in one launch
    if (fused && fused->ctl && B.mm_total > 0 && B.total <= kFusedMaxEncWgs &&
        (ndec <= 0 || (ndec <= kBatchSmall && dec_nb == nb)) && fused_mode()) {
      const int ds = fill_decode_batch(D, vsz, nb, dec, std::max(ndec, 0), &bytes_dec, fused_dec_tpw());
      if (ds != kOk) return ds;  // (no pending decode: an empty batch, D.total = 0)
      const dim3 grid(D.total + B.total);  // (the min/max items run in the encode workgroups)
      int s;
      {
        ProfScope pf(prof, kKFused, st, bytes_dec + info.bytes_mm + info.bytes_enc, true);
        s = with_type_nb<1, kBatchNbMax>(value_type, nb, [&](auto v, auto N) {
          using V = decltype(v);
          constexpr int NB = decltype(N)::value;
          return with_bool(info.stored && ff_has_stored(NB), [&](auto stored) {
            psf_launch((ff_fused_batch<V, NB, decltype(stored)::value && ff_has_stored(NB)>), grid, dim3(kBlock), 0,
                       st, D, B, fused->ctl, fused->sticky);
            return kOk;
          });
        });
      }
      return s == kOk ? launch_status() : s;
    }
    // the pending decode batch in the min/max launch when both are small (one
    // launch instead of two)
    if (ndec > 0 && ndec <= kBatchSmall && B.mm_total > 0) {
      const int ds = fill_decode_batch(D, vsz, dec_nb, dec, ndec, &bytes_dec, kBatchDecTpw);
      if (ds != kOk) return ds;
      const dim3 grid(D.total + B.mm_total);
      ProfScope pm(prof, kKDecodeMinmax, st, bytes_dec + info.bytes_mm, true);
      const int s = with_type_nb<1, kBatchNbMax>(value_type, dec_nb, [&](auto v, auto N) {
        psf_launch((ff_dec_mm_batch<decltype(v), decltype(N)::value>), grid, dim3(kBlock), 0, st, D, B);
        return kOk;
      });
      if (s != kOk) return s;
      B.mm_total_done = 1;  // the encode launch below skips the min/max pass
      ndec = 0;
    }
  }
  if (ndec > 0) {  // (not taken along above: on its own, first)
    const int ds = ff_decode_batch_launch(value_type, dec_nb, dec, ndec, st, prof);
    if (ds != kOk) return ds;
  }
  const int s = with_type_nb<1, kBatchNbMax>(value_type, nb, [&](auto v, auto N) {
    using V = decltype(v);
    constexpr int NB = decltype(N)::value;
    if (B.mm_total && !B.mm_total_done) {
      ProfScope ps(prof, kKMinmax, st, info.bytes_mm, true);
      psf_launch((ff_minmax_batch<V, CAP>), dim3(B.mm_total), dim3(kBlock), 0, st, B);
    }
    ProfScope pe(prof, kKEncode, st, info.bytes_enc, true);
    // (the kStored kernel is built at nb = 3 too, where it is never launched:
    // dropping that instantiation would change the code object)
    return with_bool(info.stored && ff_has_stored(NB), [&](auto stored) {
      psf_launch((ff_encode_batch<V, NB, CAP, decltype(stored)::value>), dim3(B.total), dim3(kBlock), 0, st, B);
      return kOk;
    });
  });
  return s == kOk ? launch_status() : s;
}

int ff_encode_batch_launch(int value_type, int nb, const FfArray* arrs, int count, void* partials,
                           PubSlot* pub_base, hipStream_t st, Profiler* prof, const FfDecArray* dec, int ndec,
                           int dec_nb, FfFusedCtl* fused) {
  if (count <= 0) return ndec > 0 ? ff_decode_batch_launch(value_type, dec_nb, dec, ndec, st, prof) : kOk;
  if (count > kFfBatchMax) return kErrArg;
  int s = check_batch_tags(value_type, nb);
  if (s == kOk && ndec > 0) s = check_batch_tags(value_type, dec_nb);
  if (s != kOk) return s;
  return count <= kBatchSmall ? encode_batch_cap<kBatchSmall>(value_type, nb, arrs, count, partials, pub_base, st, prof,
                                                              dec, ndec, dec_nb, fused)
                              : encode_batch_cap<kFfBatchMax>(value_type, nb, arrs, count, partials, pub_base, st, prof,
                                                              dec, ndec, dec_nb, nullptr);
}

template <int CAP>
static int decode_batch_cap(int value_type, int nb, const FfDecArray* arrs, int count, hipStream_t st,
                            Profiler* prof) {
  FfStage<CAP>& S = stage<CAP, kStageDecode>();
  std::lock_guard<std::mutex> lock(S.mu);
  FfBatchT<CAP>& B = S.B;
  double bytes = 0;
  const int fs = fill_decode_batch(B, value_size(value_type), nb, arrs, count, &bytes, kBatchDecTpw);
  if (fs != kOk) return fs;
  ProfScope ps(prof, kKDecode, st, bytes, true);
  const int s = with_type_nb<1, kBatchNbMax>(value_type, nb, [&](auto v, auto N) {
    psf_launch((ff_decode_batch<decltype(v), decltype(N)::value, CAP>), dim3(B.total), dim3(kBlock), 0, st, B);
    return kOk;
  });
  return s == kOk ? launch_status() : s;
}

int ff_decode_batch_launch(int value_type, int nb, const FfDecArray* arrs, int count, hipStream_t st,
                           Profiler* prof) {
  if (count <= 0) return kOk;
  if (count > kFfBatchMax) return kErrArg;
  const int s = check_batch_tags(value_type, nb);
  if (s != kOk) return s;
  return count <= kBatchSmall ? decode_batch_cap<kBatchSmall>(value_type, nb, arrs, count, st, prof)
                              : decode_batch_cap<kFfBatchMax>(value_type, nb, arrs, count, st, prof);
}

}  // namespace psf

// diagnostic: the in-launch hand-off's bound in 100 MHz ticks on the current
// device (0 = the default); a tiny bound drives ff_fused_batch's late path
extern "C" int psf_debug_set_handoff_ticks(uint64_t ticks) {
  const uint64_t v = ticks ? ticks : psf::kHandoffTicks;
  return hipMemcpyToSymbol(HIP_SYMBOL(psf::g_handoff_ticks), &v, sizeof(v)) == hipSuccess ? 0 : -1;
}

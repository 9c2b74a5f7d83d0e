// COMPRESSING on the device: what the compressor (snappy_compress.h) and the
// decompressor (snappy_uncompress.h) share -- the fragment size, the wave and
// byte-shuffling helpers, snappy's literal tag, and the phase timestamps of
// diagnostic builds.  Included by snappy.hip only (one translation unit).
#pragma once

#include "psf_internal.h"

namespace psf {
namespace {

constexpr uint32_t kFrag = 65536;     // snappy kBlockSize

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// lane l's v (l the same in every lane)
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }

__device__ __forceinline__ uint32_t ld32(const uint32_t* s, uint32_t p) {
  return __builtin_amdgcn_alignbyte(s[(p >> 2) + 1], s[p >> 2], p & 3);
}

// a pointer the caller knows is device memory, as a global-address-space one
// (plain vector loads, not flat ones, which also count against the LDS
// counter and make every LDS wait wait for them)
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gbl(const void* p) {
  return (const __attribute__((address_space(1))) T*)reinterpret_cast<uintptr_t>(p);
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the 16 bytes that start sh bytes into lo:hi (sh is the same in every lane)
__device__ __forceinline__ uint4 funnel16(const uint4& lo, const uint4& hi, uint32_t sh) {
  const uint32_t b = sh & 3;
#define AB(x, y) __builtin_amdgcn_alignbyte(x, y, b)
  switch (sh >> 2) {
    case 0: return make_uint4(AB(lo.y, lo.x), AB(lo.z, lo.y), AB(lo.w, lo.z), AB(hi.x, lo.w));
    case 1: return make_uint4(AB(lo.z, lo.y), AB(lo.w, lo.z), AB(hi.x, lo.w), AB(hi.y, hi.x));
    case 2: return make_uint4(AB(lo.w, lo.z), AB(hi.x, lo.w), AB(hi.y, hi.x), AB(hi.z, hi.y));
    default: return make_uint4(AB(hi.x, lo.w), AB(hi.y, hi.x), AB(hi.z, hi.y), AB(hi.w, hi.z));
  }
#undef AB
}

__device__ __forceinline__ uint4 shfl_down1(const uint4& v) {
  return make_uint4(__shfl_down(v.x, 1, 64), __shfl_down(v.y, 1, 64), __shfl_down(v.z, 1, 64),
                    __shfl_down(v.w, 1, 64));
}

// snappy's literal tag for a literal of len bytes at p (lanes pt 0..4)
__device__ __forceinline__ uint32_t literal_tag(uint8_t* p, uint32_t len, uint32_t pt) {
  const uint32_t m = len - 1;
  if (m < 60) {
    if (pt == 0) p[0] = (uint8_t)(m << 2);
    return 1;
  }
  const uint32_t count = ((31 - __builtin_clz(m)) >> 3) + 1;
  if (pt == 0) p[0] = (uint8_t)((59 + count) << 2);
  if (pt >= 1 && pt <= count) p[pt] = (uint8_t)(m >> (8 * (pt - 1)));
  return 1 + count;
}

// Phase timestamps of the compress kernels (diagnostic builds only,
// -DPSF_SNAPPY_TRACE, tools/snappy_trace.py): per fragment the 100 MHz clock at
// the start of the probe (0), after the probe (4), after the parse (1), at the
// start of K-place (2) and after the placement (3), plus the workgroup (5).
// The fragment decoder (K4) stamps its start, its redo and its end.
#ifdef PSF_SNAPPY_TRACE
constexpr uint32_t kTraceFrags = 1u << 14;
__device__ uint64_t g_snappy_trace[kTraceFrags * 6];
#define PSF_TRACE_T(f, k, t)                                                                \
  do {                                                                                      \
    if (threadIdx.x == (t) && (f) < kTraceFrags) {                                          \
      g_snappy_trace[(f) * 6 + (k)] = __builtin_amdgcn_s_memrealtime();                     \
      if ((k) == 0) g_snappy_trace[(f) * 6 + 5] = blockIdx.x;                               \
    }                                                                                       \
  } while (0)
#else
#define PSF_TRACE_T(f, k, t) \
  do {                       \
  } while (0)
#endif
#define PSF_TRACE(f, k) PSF_TRACE_T(f, k, 0)
#ifdef PSF_SNAPPY_TRACE
__device__ uint64_t g_dfrag_trace[kTraceFrags * 4];
#define PSF_DTRACE(f, k)                                                          \
  do {                                                                            \
    if (threadIdx.x == 0 && (f) < kTraceFrags)                                    \
      g_dfrag_trace[(f) * 4 + (k)] = __builtin_amdgcn_s_memrealtime();            \
  } while (0)
#else
#define PSF_DTRACE(f, k) \
  do {                   \
  } while (0)
#endif

}  // namespace
}  // namespace psf

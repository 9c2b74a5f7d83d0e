// C3-shape probe of the REAL single-array FIXING_FLOAT kernels: the kernels
// of ff_kernels.h (ff_minmax_partials is launched directly in mode 1) and, for
// ff_encode_launch (min/max pass + encode), ff_decode_launch and the LCG bit
// table, their launch layer ff_codec.hip, compiled into this program, on 10M
// f32 values, 3 rotating arrays, like bench.py's C3 step minus KEY_CACHING.
// Variants of the kernels are A/B'd by building this file with different -D
// flags; run under `rocprofv3 --kernel-trace --stats`.
//   argv: iters data(0 randn, 1 grid values in [-4, 4)) pub(0/1)
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I include \
//          -I parameter_server_amd/csrc -o tools/c3real_probe tools/c3real_probe.hip
#include "../parameter_server_amd/csrc/ff_kernels.h"
#include "../parameter_server_amd/csrc/ff_codec.hip"  // the launchers: this is their only other translation unit

#include <math.h>
#include <algorithm>
#include <vector>
#include <stdio.h>

namespace psf {
thread_local ExtEvents g_ext_events;
void Profiler::begin_ext() {}
void Profiler::end(KernelId, hipStream_t, double) {}
}  // namespace psf

typedef float f4v_ __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ f4v_ ld(const f4v_* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
struct P {
  const uint32_t* part;
  int nparts;
  const uint32_t* bits;
  uint32_t pos;
  double ratio;
};

// MODE 0 copy, 1 + lcg, 2 + fold, 3 full
template <int MODE, bool NT>
__global__ __launch_bounds__(256) void k_enc(const f4v_* __restrict__ x, uint32_t* __restrict__ y, size_t ntiles, P p) {
  const size_t per = (ntiles + gridDim.x - 1) / gridDim.x;
  const size_t t0 = blockIdx.x * per, t1 = min(ntiles, t0 + per);
  if (t0 >= t1) return;
  f4v_ first[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) first[u] = ld<NT>(x + t0 * 1024 + u * 256 + threadIdx.x);
  float mn = -4.f, mx = 4.f, sc = 31.75f;
  bool fast = true;
  if (MODE >= 2) {
    uint32_t lo = ~0u, hi = 0;
    for (int i = threadIdx.x; i < p.nparts; i += 256) { lo = min(lo, p.part[i]); hi = max(hi, p.part[p.nparts + i]); }
    for (int o = 32; o; o >>= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, o)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, o)); }
    __shared__ uint32_t sl[4], sh[4];
    if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = lo; sh[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = min(min(sl[0], sl[1]), min(sl[2], sl[3]));
    hi = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
    mn = unkey(lo);
    mx = (float)((double)unkey(hi) + 1e-6);
    const double bin = (double)mx - (double)mn;
    const double s = p.ratio / bin;
    sc = (float)s;
    fast = bin < __builtin_huge_val();
  }
  for (size_t t = t0; t < t1; ++t) {
    f4v_ v[4];
    if (t == t0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = first[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld<NT>(x + t * 1024 + u * 256 + threadIdx.x);
    }
    const size_t gb = t * 1024 + threadIdx.x;
    uint32_t b4[4] = {0, 0, 0, 0};
    if (MODE >= 1) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t k = (p.pos + 1u + 4u * (uint32_t)(gb + u * 256)) & 0x1FFFFu;
        const uint2 w = *reinterpret_cast<const uint2*>(p.bits + (k >> 5));
        b4[u] = __builtin_amdgcn_alignbit(w.y, w.x, k & 31u) & 0xFu;
      }
    }
    uint32_t w[4];
    uint32_t lo = 0x7F800000u, hi = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      uint32_t acc = 0;
      float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (MODE >= 3) {
          const float t = (__builtin_amdgcn_fmed3f(e[j], mn, mx) - mn) * sc;
          const float f = floorf(t);
          const uint32_t fr = __float_as_uint(t - f);
          lo = min(lo, fr);
          hi = max(hi, fr);
          acc = __builtin_amdgcn_cvt_pk_u8_f32(f, j, acc);
        } else {
          acc = __builtin_amdgcn_cvt_pk_u8_f32((e[j] - mn) * sc, j, acc);
        }
      }
      w[u] = acc;
    }
    if (MODE >= 3) {
      const bool ok = fast && lo > 0x38800000u && hi < 0x3F7FFC00u;
      if (!ok) w[0] ^= 1u;  // stand-in for the exact redo (never taken with these inputs' shape)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) y[gb + u * 256] = w[u] + ((b4[u] * 0x204081u) & 0x01010101u);
  }
}


#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

int main(int argc, char** argv) {
  const size_t n = 10000000;
  const int iters = argc > 1 ? atoi(argv[1]) : 200;
  const int data = argc > 2 ? atoi(argv[2]) : 0;
  const int use_pub = argc > 3 ? atoi(argv[3]) : 1;
  const int mode = argc > 4 ? atoi(argv[4]) : 0;  // 0 real encode, 1 real min/max + synthetic encode
  const int do_dec = argc > 5 ? atoi(argv[5]) : 1;
  const int NA = 3;
  float* h = (float*)malloc(n * 4);
  uint64_t s = 88172645463325252ull;
  for (size_t i = 0; i < n; i += 2) {
    if (data == 0) {
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;
      const double u1 = ((s >> 11) + 1) * (1.0 / 9007199254740993.0);
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;
      const double u2 = (s >> 11) * (1.0 / 9007199254740992.0);
      const double r = sqrt(-2.0 * log(u1));
      h[i] = (float)(r * cos(6.283185307179586 * u2));
      if (i + 1 < n) h[i + 1] = (float)(r * sin(6.283185307179586 * u2));
    } else {
      h[i] = (float)((int)((i * 2654435761u) >> 8) % 8000) / 1000.0f - 4.0f;
      if (i + 1 < n) h[i + 1] = (float)((int)(((i + 1) * 2654435761u) >> 8) % 8000) / 1000.0f - 4.0f;
    }
  }
  float* xs[NA];
  for (int i = 0; i < NA; ++i) { CK(hipMalloc(&xs[i], n * 4)); CK(hipMemcpy(xs[i], h, n * 4, hipMemcpyHostToDevice)); }
  uint8_t* codes[NA];
  for (int i = 0; i < NA; ++i) CK(hipMalloc(&codes[i], n));
  float* dec;
  CK(hipMalloc(&dec, n * 4));
  void* partials;
  CK(hipMalloc(&partials, 1 << 16));
  float* range;
  int* status;
  CK(hipMalloc(&range, 64));
  CK(hipMalloc(&status, 64));
  psf::PubSlot* pub = nullptr;
  CK(hipHostMalloc((void**)&pub, sizeof(psf::PubSlot) * NA, hipHostMallocMapped | hipHostMallocCoherent));
#ifdef PSF_WG_TRACE
  uint64_t* trace;
  CK(hipMalloc(&trace, 8 * 8 * 16384));
  CK(hipMemset(trace, 0, 8 * 8 * 16384));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(psf::g_wg_trace), &trace, sizeof(trace)));
#endif
  hipStream_t st;
  CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  psf::FixedPoint fp{};
  for (int it = 0; it < iters; ++it) {
    const int i = it % NA;
    int r;
    if (mode == 0) {
      r = psf::ff_encode_launch(xs[i], n, psf::kFloat, 1, fp, 12345u + it, codes[i], partials, range, status, st,
                                nullptr, use_pub ? pub + i : nullptr, (uint32_t)it + 1, nullptr);
    } else {
      psf::FixedPoint both{1, 1, -5.f, 5.f};
      (void)both;
      const int g = (int)((n / 4 + 1023) / 1024);
      hipLaunchKernelGGL((psf::ff_minmax_partials<float, true>), dim3(1024), dim3(256), 0, st, xs[i], n, partials, 0u);
      P pp{(const uint32_t*)partials, 1024, psf::lcg_bits_device(), 12345, 254.0};
      hipLaunchKernelGGL((k_enc<3, true>), dim3(g), dim3(256), 0, st, (const f4v_*)xs[i], (uint32_t*)codes[i],
                         (size_t)(n / 4096), pp);
      r = 0;
    }
    if (r) { printf("encode %d\n", r); return 1; }
    if (do_dec) r = psf::ff_decode_launch(codes[(it + NA - 1) % NA], n, psf::kFloat, 1, range, 0.f, 0.f, dec, st, nullptr);
    if (r) { printf("decode %d\n", r); return 1; }
  }
  CK(hipStreamSynchronize(st));
  printf("done data %d pub %d mode %d dec %d\n", data, use_pub, mode, do_dec);
#ifdef PSF_WG_TRACE
  // the last encode's per-workgroup stamps (10 ns ticks): when each started,
  // how long to its quantiser, to its last store; the 12 last to finish
  {
    int grid = (int)((n / 4 + 1023) / 1024);
    std::vector<uint64_t> tr8(8 * (size_t)grid), tr(4 * (size_t)grid);
    CK(hipMemcpy(tr8.data(), trace, tr8.size() * 8, hipMemcpyDeviceToHost));
    for (int b = 0; b < grid; ++b)
      for (int k = 0; k < 4; ++k) tr[4 * b + k] = tr8[8 * b + k];
    while (grid > 1 && tr[4 * (grid - 1) + 2] == 0) --grid;  // a launch of fewer workgroups
    printf("grid %d\n", grid);
    uint64_t s0 = ~0ull, e1 = 0;
    for (int b = 0; b < grid; ++b) { s0 = std::min(s0, tr[4 * b]); e1 = std::max(e1, tr[4 * b + 2]); }
    printf("kernel span %.2f us (first start -> last end)\n", (e1 - s0) * 0.01);
    auto pct = [&](int k, double q) {
      std::vector<double> v;
      for (int b = 0; b < grid; ++b) {
        const uint64_t* r = &tr[4 * b];
        v.push_back(k == 0 ? (r[0] - s0) * 0.01 : k == 1 ? (r[1] - r[0]) * 0.01 : k == 2 ? (r[2] - r[1]) * 0.01 : (r[2] - r[0]) * 0.01);
      }
      std::sort(v.begin(), v.end());
      return v[(size_t)(q * (v.size() - 1))];
    };
    const char* nm[4] = {"start", "prologue", "tiles", "total"};
    for (int k = 0; k < 4; ++k)
      printf("%-9s p0 %.2f p10 %.2f p50 %.2f p90 %.2f p99 %.2f max %.2f\n", nm[k], pct(k, 0), pct(k, .1), pct(k, .5), pct(k, .9), pct(k, .99), pct(k, 1));
    std::vector<int> ord(grid);
    for (int b = 0; b < grid; ++b) ord[b] = b;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return tr[4 * a + 2] > tr[4 * b + 2]; });
    for (int i = 0; i < 12; ++i) {
      const uint64_t* r = &tr[4 * ord[i]];
      printf("  last wg %5d start %.2f prologue %.2f tiles %.2f xcc %llu hwid %08llx\n", ord[i], (r[0] - s0) * 0.01,
             (r[1] - r[0]) * 0.01, (r[2] - r[1]) * 0.01, (unsigned long long)(r[3] >> 32), (unsigned long long)(r[3] & 0xffffffffu));
    }
    // starts over time: how many workgroups had started by t
    for (double t = 0; t <= (e1 - s0) * 0.01 + 0.5; t += 1.0) {
      int c = 0, d = 0;
      for (int b = 0; b < grid; ++b) { c += (tr[4 * b] - s0) * 0.01 <= t; d += (tr[4 * b + 2] - s0) * 0.01 <= t; }
      printf("  t %5.1f us: started %5d finished %5d\n", t, c, d);
    }
  }
#endif
  return 0;
}

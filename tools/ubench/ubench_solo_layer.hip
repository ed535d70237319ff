// ubench_solo_layer.hip -- the layer of the one-wavefront-per-item body (qsim_lean_solo.h: solo_layer, the shipped code:
// bits 4..7 as register bits of two alternating layouts, eight swaps per layer) beside the layer it replaced (bits 4 / 5
// by swap, 2 x 2, swap back per amplitude: solo_layer_swapback below),
// next to ubench_layer.hip's four-wave layer: 13 layers per "step", s_memtime around `iters` steps, one workgroup of
// W = 1, 2, 4, 8 (12, 16) wavefronts per CU on all 256 CUs (96 KiB of LDS per workgroup keep a second one off the CU), every
// wavefront on an item of its own.  Tangents read from LDS one layer ahead, as the kernel does; the phase entries
// either in registers (104 VGPRs, two wavefronts per SIMD at most: the kernel before it went wide) or in LDS as
// [layer][2][64] 16-byte units (LeanSoloLds) and read one layer ahead too, under a 1 024-thread bound (the shipped
// kernel: W up to 16, four wavefronts per SIMD).
// The four-wave layer costs 400 ticks for ONE item per CU (ubench_layer, "full layer as shipped"); W solo wavefronts
// finish W items in the time printed here.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../qiddm_amd/csrc -o ubench_solo_layer ubench_solo_layer.hip
#include "qsim_lean_solo.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qiddm;
typedef float v4f __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

constexpr int kLayers = 13;
constexpr int kBlocks = 256;
constexpr int kMaxWaves = 16;      // ... of the LDS variant; the registers variants stop at kRegWaves
constexpr int kRegWaves = 8;
constexpr size_t kLds = 96 * 1024;

// the layer before the transposing one: one layout (A) throughout, index bits 4 / 5 through ry_t_swap
__device__ __forceinline__ void solo_layer_swapback(V2<float> (&a)[4], const V2<float> (&ph)[4], const float (&ts)[4],
                                                    float t4, float t5, float t6, float t7) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float re = fmaf(-ph[r].y, a[r].y, ph[r].x * a[r].x), im = fmaf(ph[r].y, a[r].x, ph[r].x * a[r].y);
    a[r] = V2<float>{re, im};
  }
  solo_ry_dpp4(a, ts[0], ts[1], ts[2], ts[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) ry_t_swap<5, float>(a[r], t5);
#pragma unroll
  for (int r = 0; r < 4; ++r) ry_t_swap<4, float>(a[r], t4);
  solo_ry_reg(a[0], a[1], t6);
  solo_ry_reg(a[2], a[3], t6);
  solo_ry_reg(a[0], a[2], t7);
  solo_ry_reg(a[1], a[3], t7);
}

enum Variant { kSwapBack, kTransposing, kTransposingLds };
constexpr const char* kNames[] = {"swap-back      ", "transposing    ", "transposing LDS"};
constexpr size_t kPhOffset = 1024;   // the phase units behind the tangents in LDS

template <int V>
__global__ __launch_bounds__((V == kTransposingLds ? kMaxWaves : kRegWaves) * 64) void solo_layer_loop(float* out, unsigned long long* ticks, int iters,
                                                                 const float* tab) {
  using T = float;
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* s_un = reinterpret_cast<T*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < (kLayers + 1) * 8; i += blockDim.x) s_un[i] = tab[i % 509] * 0.4f;
  constexpr bool kLdsPhases = V == kTransposingLds;
  auto phase_of = [&](int l, int r, int ln) {
    const int i = (l * 4 + r) * 64 + ln;
    return C{tab[(i * 2) % 509] * 0.9f + 0.05f, tab[(i * 2 + 1) % 509] * 0.3f};
  };
  C ph[kLdsPhases ? 1 : kLayers][4];
  C* s_ph = reinterpret_cast<C*>(smem_raw + kPhOffset);   // unit (l, h, lane) = registers 2 h, 2 h + 1 of the lane
  if constexpr (kLdsPhases) {
    for (int e = tid; e < kLayers * 256; e += blockDim.x)
      s_ph[e] = phase_of(e >> 8, ((e >> 6) & 2) | (e & 1), (e >> 1) & 63);
  } else {
#pragma unroll
    for (int l = 0; l < kLayers; ++l) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ph[l][r] = phase_of(l, r, lane);
    }
  }
  T pm[4];
  const int llane = logical_lane(lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) pm[q] = ((llane >> q) & 1) ? (T)1 : (T)-1;
  C a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = C{0.01f * (float)(lane + 64 * r + 1), 0.02f};
  __syncthreads();
  const v4f* un4 = reinterpret_cast<const v4f*>(s_un);
  const v4f* ph4 = reinterpret_cast<const v4f*>(s_ph) + lane;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    asm volatile("" ::: "memory");
    v4f lo = un4[0], hi = un4[1], p01 = {}, p23 = {};
    if constexpr (kLdsPhases) {
      p01 = ph4[0];
      p23 = ph4[64];
    }
#pragma unroll
    for (int l = 0; l < kLayers; ++l) {
      const v4f nlo = un4[2 * (l + 1)], nhi = un4[2 * (l + 1) + 1];
      v4f np01 = {}, np23 = {};
      if constexpr (kLdsPhases) {
        const int ln = l + 1 < kLayers ? l + 1 : l;
        np01 = ph4[ln * 128];
        np23 = ph4[ln * 128 + 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      const T ts[4] = {lo.x * pm[0], lo.y * pm[1], lo.z * pm[2], lo.w * pm[3]};
      if constexpr (kLdsPhases) {
        const C pl[4] = {C{p01.x, p01.y}, C{p01.z, p01.w}, C{p23.x, p23.y}, C{p23.z, p23.w}};
        solo_layer(l % 2 == 0 ? kSoloLayoutB : kSoloLayoutA, a, pl, ts, hi.x, hi.y, hi.z, hi.w);
      } else if constexpr (V == kTransposing) {
        solo_layer(l % 2 == 0 ? kSoloLayoutB : kSoloLayoutA, a, ph[l], ts, hi.x, hi.y, hi.z, hi.w);
      } else {
        solo_layer_swapback(a, ph[l], ts, hi.x, hi.y, hi.z, hi.w);
      }
      lo = nlo;
      hi = nhi;
      p01 = np01;
      p23 = np23;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = a[r] * C{0.05f, 0.05f};   // keep the values bounded
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) ticks[blockIdx.x * kMaxWaves + wv] = t1 - t0;
  out[(size_t)blockIdx.x * (kMaxWaves * 64) + tid] = (a[0].x + a[1].y) + (a[2].x + a[3].y);
}

template <int V>
static double run(float* out, unsigned long long* ticks, const float* tab, int iters, int waves) {
  for (int rep = 0; rep < 2; ++rep) {
    hipLaunchKernelGGL(solo_layer_loop<V>, dim3(kBlocks), dim3(waves * 64), kLds, 0, out, ticks, iters, tab);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
  }
  std::vector<unsigned long long> h(kBlocks * kMaxWaves);
  CHECK(hipMemcpy(h.data(), ticks, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double sum = 0, mx = 0;
  for (int b = 0; b < kBlocks; ++b)
    for (int w = 0; w < waves; ++w) {
      const double v = (double)h[b * kMaxWaves + w];
      sum += v;
      mx = v > mx ? v : mx;
    }
  const double per = sum / (kBlocks * waves) / ((double)iters * kLayers);
  printf("  %s  %d solo wavefront(s) per CU: %7.1f ticks/layer (slowest wavefront %7.1f), %7.1f ticks per item-layer\n",
         kNames[V], waves, per, mx / ((double)iters * kLayers), per / waves);
  return per;
}

int main() {
  float *out, *tab;
  unsigned long long* ticks;
  CHECK(hipMalloc(&out, (size_t)kBlocks * kMaxWaves * 64 * sizeof(float)));
  CHECK(hipMalloc(&ticks, kBlocks * kMaxWaves * sizeof(unsigned long long)));
  CHECK(hipMalloc(&tab, 512 * sizeof(float)));
  std::vector<float> h(512);
  for (int i = 0; i < 512; ++i) h[i] = (float)((i * 2654435761u) % 1000) / 1000.0f;
  CHECK(hipMemcpy(tab, h.data(), 512 * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(solo_layer_loop<kSwapBack>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(solo_layer_loop<kTransposing>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(solo_layer_loop<kTransposingLds>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
  const int iters = 400;
  for (int rep = 0; rep < 3; ++rep) {
    printf("run %d\n", rep);
    for (int waves : {1, 2, 4, 8}) run<kSwapBack>(out, ticks, tab, iters, waves);
    for (int waves : {1, 2, 4, 8}) run<kTransposing>(out, ticks, tab, iters, waves);
    for (int waves : {1, 2, 4, 8, 12, 16}) run<kTransposingLds>(out, ticks, tab, iters, waves);
  }
  return 0;
}

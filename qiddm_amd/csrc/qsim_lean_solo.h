// qsim_lean_solo.h -- the "solo" body of the lean sampling loop: ONE wavefront per (sample, step) item of the 8-qubit
// net without re-upload and with a compiled-in layer count (float32; the flagship QNN_noise(784, 8, 14)).
//
// Layout: all 256 amplitudes in one wavefront, four per lane.  Amplitude k = (r << 6) | logical_lane(lane), r = 0..3:
// the register bits are index bits 6 and 7 -- the WAVE bits of the four-wave decomposition (qsim_lean.h), so entry
// r * 64 + lane of a LeanTables<T, 8> layer is this lane's entry for register r and the tables are read as they are.
// What that buys:
//   * index bits 6 / 7 are plain FMAs on register pairs: no LDS exchange, no s_barrier in a layer;
//   * every gate acts on 8 independent registers (4 amplitudes x re / im), so the wave issues back to back (~4 cycles
//     per vector instruction) instead of waiting ~11 cycles on its own previous result;
//   * the items of a launch (batch x n_steps: this instance's angles never reach the state, so its steps do not depend
//     on each other) are spread over all wavefronts of all workgroups, kSoloWaves per CU.  Every item is still
//     simulated in full.
// After the per-workgroup setup (linear_up's weights and the tangents into LDS, one __syncthreads()) there is no
// cross-wave synchronisation at all: every wave runs the same code and the only thing that depends on the wave number
// is which items it takes.
#pragma once
#include "qsim_lean.h"

namespace qiddm {

// LDS of the solo body: linear_up's weights as [4][Qp] pairs (w[pix][2 jj], w[pix][2 jj + 1]) -- a lane's 16 bytes next
// to its neighbour's: `ds_read_b128` without bank conflicts --, the bias [Qp], the tangents [layers][8].  Qp = Q rounded
// up to whole wavefronts; the rows beyond Q hold copies of the last row and are never stored.
struct LeanSoloLds {
  __host__ __device__ static constexpr int padded(int q) { return (q + kWave - 1) / kWave * kWave; }
  __host__ __device__ static constexpr size_t w_bytes(int q) { return (size_t)padded(q) * 8 * sizeof(double); }
  __host__ __device__ static constexpr size_t b_bytes(int q) { return (size_t)padded(q) * sizeof(double); }
  __host__ __device__ static constexpr size_t bytes(int q, int layers) {
    return w_bytes(q) + b_bytes(q) + (size_t)layers * 8 * sizeof(float);
  }
};

// The four DPP lane-bit gates (index bits 0..3) on eight registers: own += t_signed * partner, `v_fmac_f32_dpp` in place
// (qsim_lean.h: ry_t_dpp4).  A DPP read needs two wait states behind the vector instruction that wrote the register:
// inside the block a register is read eight instructions after it was written; `s_nop 1` in front covers whatever the
// compiler placed before the block, `s_nop 1` behind whatever it places after (a permlane swap follows).
#define QIDDM_SOLO_DPP8(ctrl, t)                                             \
  "v_fmac_f32_dpp %0, %0, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %1, %1, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %2, %2, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %3, %3, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %4, %4, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %5, %5, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %6, %6, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %7, %7, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
__device__ __forceinline__ void solo_ry_dpp4(V2<float> (&a)[4], float t0, float t1, float t2, float t3) {
  float v0 = a[0].x, v1 = a[0].y, v2 = a[1].x, v3 = a[1].y, v4 = a[2].x, v5 = a[2].y, v6 = a[3].x, v7 = a[3].y;
  asm volatile(
      "s_nop 1\n\t"
      QIDDM_SOLO_DPP8("quad_perm:[1,0,3,2]", "%8")
      QIDDM_SOLO_DPP8("quad_perm:[2,3,0,1]", "%9")
      QIDDM_SOLO_DPP8("row_half_mirror", "%10")
      QIDDM_SOLO_DPP8("row_ror:8", "%11")
      "s_nop 1"
      : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)
      : "v"(t0), "v"(t1), "v"(t2), "v"(t3));
  a[0] = V2<float>{v0, v1};
  a[1] = V2<float>{v2, v3};
  a[2] = V2<float>{v4, v5};
  a[3] = V2<float>{v6, v7};
}
#undef QIDDM_SOLO_DPP8

// RY (tangent form) on a register bit: the 2 x 2 on (member with the bit clear, member with it set)
__device__ __forceinline__ void solo_ry_reg(V2<float>& lo, V2<float>& hi, float t) {
  const V2<float> nlo = __builtin_elementwise_fma(bcast<float>(-t), hi, lo);
  const V2<float> nhi = __builtin_elementwise_fma(bcast<float>(t), lo, hi);
  lo = nlo;
  hi = nhi;
}

// One layer on the four amplitudes of a lane: phase table entry, then RY on every index bit (tangent form: the cosines
// sit in the phase entry).  ts: tangents of index bits 0..3 signed by this lane's bit; t4..t7: plain tangents.
__device__ __forceinline__ void solo_layer(V2<float> (&a)[4], const V2<float> (&ph)[4], const float (&ts)[4], float t4,
                                           float t5, float t6, float t7) {
  // (component by component, the products of cmul2: its packed form wants (ph.x, ph.x) and (ph.y, ph.y) as register
  //  pairs, which the compiler keeps across the loop for every layer -- twice the registers of the phase table)
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

// The body of dense_lean_kernel<float, 8, PPT, false, LPR, false> at kSoloThreads threads per workgroup.
// Items: (sample, step) = item / n_steps, item % n_steps for item < batch * n_steps; wave g of the launch takes items
// g, g + (waves of the launch), ...: every item is written exactly once, no wave idles while another has two to do.
template <int LPR>
__device__ void dense_lean_solo_body(const double* __restrict__ wu, const double* __restrict__ bu,
                                                     double* __restrict__ y, const unsigned char* __restrict__ tables,
                                                     const QuadScalars& d, const KScalars& p) {
  using T = float;
  using C = V2<T>;
  using QT = LeanTables<T, 8>;
  using V4 = T __attribute__((ext_vector_type(4)));
  using D2 = double __attribute__((ext_vector_type(2)));
  static_assert(LPR > 1, "a compiled-in layer count with at least one simulated layer");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int Q = d.out_features, Qp = LeanSoloLds::padded(Q);
  D2* s_w = reinterpret_cast<D2*>(smem_raw);                                   // [4][Qp]
  double* s_b = reinterpret_cast<double*>(smem_raw + LeanSoloLds::w_bytes(Q));  // [Qp]
  T* s_un = reinterpret_cast<T*>(smem_raw + LeanSoloLds::w_bytes(Q) + LeanSoloLds::b_bytes(Q));   // [LPR][8]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int llane = logical_lane(lane);
  const T* g_body = reinterpret_cast<const T*>(tables + kLeanHeaderDoubles * sizeof(double));
  const C* g_ph = reinterpret_cast<const C*>(g_body);
  const T* g_un = g_body + QT::ph_elems(LPR);
  const T* g_a0 = g_un + QT::un_elems(LPR);

  // ---- per-launch setup: weights, bias and tangents into LDS; this lane's table entries into registers -----------------
  // Every global load is issued before anything waits: the ones on their way to LDS first (loads return in order, so the
  // LDS stores wait for those alone), the table entries behind them -- one memory latency for the whole setup.
  constexpr int kWTrips = 4 * 1024 / kSoloThreads, kBTrips = 1024 / kSoloThreads;   // Q <= 1024 (the host checks)
  D2 wreg[kWTrips];
  double breg[kBTrips];
#pragma unroll
  for (int k = 0; k < kWTrips; ++k) {
    // (a row's four pairs are 64 contiguous bytes of w_up.  An entry beyond the image loads the last one -- no branch
    //  around a load, which would wait for the loads before it -- and its pixel is never stored)
    const int i = tid + k * kSoloThreads;
    wreg[k] = reinterpret_cast<const D2*>(wu)[i < 4 * Q ? i : 4 * Q - 1];
  }
#pragma unroll
  for (int k = 0; k < kBTrips; ++k) {
    const int i = tid + k * kSoloThreads;
    breg[k] = bu != nullptr ? bu[i < Q ? i : Q - 1] : 0.0;
  }
  const T unreg = g_un[tid < LPR * 8 ? tid : 0];
  C phr[LPR][4];   // (entry 0 unused: the first layer is generated)
  T a0r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a0r[r] = g_a0[r * kWave + lane];
#pragma unroll
  for (int l = 1; l < LPR; ++l) {
#pragma unroll
    for (int r = 0; r < 4; ++r) phr[l][r] = g_ph[l * QT::TL + r * kWave + lane];
  }
  __builtin_amdgcn_sched_barrier(0);   // (all loads are out)
#pragma unroll
  for (int k = 0; k < kWTrips; ++k) {
    const int i = tid + k * kSoloThreads;
    if (i < 4 * Qp) s_w[(i & 3) * Qp + (i >> 2)] = wreg[k];
  }
#pragma unroll
  for (int k = 0; k < kBTrips; ++k) {
    const int i = tid + k * kSoloThreads;
    if (i < Qp) s_b[i] = breg[k];
  }
  static_assert(LPR * 8 <= kSoloThreads, "one tangent per thread");
  if (tid < LPR * 8) s_un[tid] = unreg;
  T pm[4];   // +-1 by this lane's index bit
#pragma unroll
  for (int q = 0; q < 4; ++q) pm[q] = ((llane >> q) & 1) ? (T)1 : (T)-1;
  __syncthreads();

  // ---- the items of this wave ---------------------------------------------------------------------------------------
  const uint32_t n_steps = (uint32_t)d.n_steps;
  const uint32_t stride = (uint32_t)gridDim.x * kSoloWaves;     // waves of the launch
  const uint32_t g0 = (uint32_t)blockIdx.x * kSoloWaves + (uint32_t)wv;
  const uint32_t stride_q = stride / n_steps, stride_r = stride - stride_q * n_steps;
  int64_t sample = (int64_t)(g0 / n_steps);
  uint32_t step = g0 - (g0 / n_steps) * n_steps;
  const int groups = Qp / kWave;
  for (; sample < p.batch; ) {
    asm volatile("" ::: "memory");   // (the LDS reads below stay inside the loop: hoisted, they would not fit registers)
    C a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = C{a0r[r], (T)0};
    // a layer's tangents are read one layer ahead (the fence keeps the compiler from reading all layers' up front)
    const V4* un4 = reinterpret_cast<const V4*>(s_un);
    V4 lo = un4[2], hi = un4[3];
#pragma unroll
    for (int l = 1; l < LPR; ++l) {
      const int ln = l + 1 < LPR ? l + 1 : l;
      const V4 nlo = un4[2 * ln], nhi = un4[2 * ln + 1];
      __builtin_amdgcn_sched_barrier(0);
      const T ts[4] = {lo.x * pm[0], lo.y * pm[1], lo.z * pm[2], lo.w * pm[3]};
      solo_layer(a, phr[l], ts, hi.x, hi.y, hi.z, hi.w);
      lo = nlo;
      hi = nhi;
    }
    // ---- <Z_w>: the register-bit wires are signed in-lane sums, the lane-bit wires signed copies of the lane's total ----
    T pw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pw[r] = a[r].x * a[r].x + a[r].y * a[r].y;
    const T pt = (pw[0] + pw[1]) + (pw[2] + pw[3]);
    T ez[8];
    ez[0] = (pw[0] + pw[1]) - (pw[2] + pw[3]);   // wire 0 = index bit 7 = register bit 1
    ez[1] = (pw[0] + pw[2]) - (pw[1] + pw[3]);   // wire 1 = index bit 6 = register bit 0
#pragma unroll
    for (int w = 2; w < 8; ++w) ez[w] = ((llane >> (7 - w)) & 1) ? -pt : pt;
    const T tot = wave_reduce8<T>(ez, lane, llane);
    double ev[8];
#pragma unroll
    for (int w = 0; w < 8; ++w)
      ev[w] = (double)read_lane(tot, logical_lane(((w >> 2) & 1) | (w & 2) | ((w & 1) << 2)));
    // ---- linear_up: pixel = lane + 64 g, two partial sums with explicit fma (as dense_lean_kernel) ---------------------
    double* yrow = y + (size_t)step * d.y_step_stride + sample * d.y_ld;
#pragma unroll 4
    for (int g = 0; g < groups; ++g) {
      const int pix = lane + g * kWave;
      const D2 w01 = s_w[pix], w23 = s_w[Qp + pix], w45 = s_w[2 * Qp + pix], w67 = s_w[3 * Qp + pix];
      double o0 = s_b[pix], o1 = 0.0;
      o0 = fma(ev[0], w01.x, o0);
      o1 = fma(ev[1], w01.y, o1);
      o0 = fma(ev[2], w23.x, o0);
      o1 = fma(ev[3], w23.y, o1);
      o0 = fma(ev[4], w45.x, o0);
      o1 = fma(ev[5], w45.y, o1);
      o0 = fma(ev[6], w67.x, o0);
      o1 = fma(ev[7], w67.y, o1);
      o0 += o1;
      if (pix < Q) yrow[pix] = o0;
    }
    // next item of this wave
    sample += stride_q;
    step += stride_r;
    if (step >= n_steps) {
      step -= n_steps;
      ++sample;
    }
  }
}

}  // namespace qiddm

// qsim_traj_shots.h -- finite shots on quantum trajectories: the trajectories of qsim_traj.h, decision for decision, with a
// SAMPLER in the place of the analytic read-out.  A trajectory draws its share of the launch's shots from |psi_k|^2 and
// adds them to integer counts; a real device runs one noise realisation per shot, so shots == trajectories is the natural
// setting.  The rule (the split of the shots, the weights, the two-level CDF, the Philox word of a shot) is stated in
// include/qiddm_hip_traj_shots.h under THE SAMPLING RULE; this file follows it line by line and
// tests/_mixed_traj_shots_ref.py restates it in numpy.
//
// Neither rho nor a 2^n-entry float64 CDF fits in LDS here (psi alone takes 128 KiB at 14 wires in float32, and lives in
// the workgroup's slab of the workspace beyond that), so the CDF has two levels: 256 segment sums, scanned by one thread
// into 256 doubles of LDS, and inside the chosen segment a walk over psi itself.  Segment j holds the outcomes j, j + 256,
// j + 512, ...: the elements thread j owns in every sweep of the engine, so the sweep for the segment sums is coalesced
// and free of bank conflicts, and the CDF order is a fixed permutation of the outcomes, which sampling allows.
//
// Execution shape: mixed_traj_kernel's.  Work item (sample b, slot s), s = 0 .. min(T_run, 64) - 1: the trajectories
// t = s, s + 64, ... of the sample, one at a time, psi in dynamic LDS or in the workgroup's slab.  Counts are uint32 and
// are added with integer atomics on a zeroed region of the workspace: arrival order cannot change an integer sum, so
// reruns, any grid and any max_blocks give the same bits.  No float atomics anywhere.
// The op walk of a trajectory is repeated here, not shared with mixed_traj_kernel through a function: that kernel's four
// instantiations then keep the device code they had (see profiles/mixed_traj_shots/resource_usage.txt).
#pragma once
#include "qsim_traj.h"

namespace qiddm {

constexpr int kTrajShotsPerTraj = 1 << 16;  // most shots one trajectory draws: bounds a workgroup's sampling loop

struct TrajShotScalars {
  int32_t shots;   // S, all trajectories of a sample together
  int32_t t_run;   // min(n_traj, S): the trajectories that draw at least one shot -- the others are not run
  int32_t per;     // q = S div n_traj
  int32_t extra;   // r = S mod n_traj: trajectory t draws q + (t < r) shots, the global indices q t + min(t, r) + i
};

// p_k = max(re^2 + im^2, 0), a NaN counting as 0: two products and one sum, each rounded once, never an fma.  THE one
// place that computes a weight: the value summed, the value walked and the value handed back in per_traj are this one.
// (__dmul_rn / __dadd_rn are plain operators in the toolchain's header; the pragma is what takes the fma choice away.)
template <typename T>
__device__ __forceinline__ double traj_shot_weight(V2<T> a) {
#pragma clang fp contract(off)
  const double x = (double)a.x, y = (double)a.y;
  const double p = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
  return p > 0.0 ? p : 0.0;
}

// One shot from the two-level CDF: v in [0, W) -> the outcome.  s_cdf: C_0 .. C_{G-1}; G = 1 << gs segments of L
// elements, segment j = the outcomes j + (i << gs).
template <typename T>
__device__ __forceinline__ uint32_t traj_shot_outcome(const V2<T>* psi, const double* s_cdf, int gs, uint32_t L, double v) {
#pragma clang fp contract(off)
  const int G = 1 << gs;
  int j = 0;  // #{j : C_j <= v}, clamped to G - 1
  for (int step = G >> 1; step >= 1; step >>= 1) j += s_cdf[j + step - 1] <= v ? step : 0;
  const double u = v - (j > 0 ? s_cdf[j - 1] : 0.0);
  double c = 0.0;
  uint32_t last = (uint32_t)j, chosen = 0;  // the last k of the segment with p_k > 0: what rounding may leave
  bool found = false;
  for (uint32_t i0 = 0; i0 < L && !found; i0 += 8) {
    double p[8];  // eight loads in flight: at 15 and 16 wires every one is a trip to L2
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = i0 + e < L ? traj_shot_weight<T>(psi[(uint32_t)j + ((i0 + e) << gs)]) : 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = (uint32_t)j + ((i0 + e) << gs);
      c = __dadd_rn(c, p[e]);  // (+ 0.0 past the end changes nothing)
      last = p[e] > 0.0 ? k : last;
      if (!found && c > u) {
        found = true;
        chosen = k;
      }
    }
  }
  return found ? chosen : last;
}

// grid: any number of workgroups up to batch * n_slots (tr.n_slots = min(sh.t_run, 64)); they stride the work items.
// counts: (batch, 2^n) uint32 for PROBS, (batch, n) uint32 for EXPZ (outcomes with the wire's bit set), zeroed; flags:
// (batch) uint32, zeroed, set for a sample with a bad trajectory.  per_traj (batch, t_run, 2^n) float64, branches
// (batch, t_run, n_channels) int32 and outcomes (batch, shots) int32 may be NULL.
template <typename T, bool K2>
__global__ __launch_bounds__(256) void mixed_traj_shots_kernel(
    const MixedOp* __restrict__ prog, const double* __restrict__ angle_rows, const double* __restrict__ feats,
    const double* __restrict__ gates, uint32_t* __restrict__ counts, uint32_t* __restrict__ flags,
    V2<T>* __restrict__ slabs, double* __restrict__ per_traj, int32_t* __restrict__ branches,
    int32_t* __restrict__ outcomes, const MixedScalars m, const TrajScalars tr, const TrajShotScalars sh) {
#pragma clang fp contract(off)
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[64];
  __shared__ double s_cdf[256];   // P_j, then C_j
  __shared__ uint32_t s_ones[16];  // EXPZ: this item's outcomes with bit w set
  C* psi = tr.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : slabs + ((size_t)blockIdx.x << m.n);
  const int tid = threadIdx.x, n = m.n;
  const uint32_t D = 1u << n;
  const int gs = n < 8 ? n : 8;  // G = min(2^n, 256) segments of L = 2^n / G elements
  const int G = 1 << gs;
  const uint32_t L = D >> gs;
  const int64_t items = m.batch * tr.n_slots;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t sample = item / tr.n_slots;
    const int slot = (int)(item - sample * tr.n_slots);
    if (tid < 16) s_ones[tid] = 0u;
    __syncthreads();
    for (int t = slot; t < sh.t_run; t += tr.n_slots) {
      const size_t traj = (size_t)sample * sh.t_run + t;
      uint32_t d = 0;
      bool bad = false;
      for (int oi = 0; oi < m.n_ops; ++oi) {  // mixed_traj_kernel's walk
        const MixedOp op = prog[oi];
        if (K2 ? traj_is_channel(op.kind) : traj_is_channel1(op.kind)) {
          int chosen = -1;
          if (!bad) {
            if (K2 && op.kind == kMixKraus2) {
              if constexpr (K2) chosen = traj_channel2<T>(psi, op, gates, m, tr, sample, (uint32_t)t, d, s_red);
            } else {
              chosen = traj_channel<T>(psi, op, angle_rows, gates, m, tr, sample, (uint32_t)t, d, s_red);
            }
            bad = chosen < 0;
          }
          if (branches && tid == 0) branches[traj * tr.n_channels + d] = chosen;
          ++d;
        } else if (!bad) {
          traj_apply_op<T>(psi, op, angle_rows, feats, gates, m, sample, s_red);
        }
        __syncthreads();
      }
      // this trajectory's shots: s_t of them, the global indices first .. first + s_t - 1
      const uint32_t s_t = (uint32_t)sh.per + (t < sh.extra ? 1u : 0u);
      const size_t first = (size_t)sh.per * (size_t)t + (size_t)(t < sh.extra ? t : sh.extra);
      int32_t* __restrict__ drawn = outcomes ? outcomes + (size_t)sample * (size_t)sh.shots + first : nullptr;
      double* __restrict__ own = per_traj ? per_traj + traj * (size_t)D : nullptr;
      if (bad) {  // it stopped at a decision: psi is not a state
        if (own)
          for (uint32_t k = tid; k < D; k += 256) own[k] = __builtin_nan("");
      } else {
        if (tid < G) {  // P_j: the segment's weights in ascending i
          double P = 0.0;
          for (uint32_t i = 0; i < L; ++i) {
            const uint32_t k = (uint32_t)tid + (i << gs);
            const double p = traj_shot_weight<T>(psi[k]);
            if (own) own[k] = p;
            P = __dadd_rn(P, p);
          }
          s_cdf[tid] = P;
        }
        __syncthreads();
        if (tid == 0) {  // C_j = P_0 + ... + P_j, one thread, in ascending j
          double run = 0.0;
          for (int j = 0; j < G; ++j) {
            run = __dadd_rn(run, s_cdf[j]);
            s_cdf[j] = run;
          }
        }
        __syncthreads();
        const double W = s_cdf[G - 1];
        bad = !(W > 0.0) || !isfinite(W);
        if (!bad) {
          for (uint32_t i = tid; i < s_t; i += 256) {
            uint32_t c0 = 0x80000000u | (i >> 2), c1 = (uint32_t)t, c2 = (uint32_t)sample, c3 = tr.offset;
            philox4x32_10(c0, c1, c2, c3, tr.seed_lo, tr.seed_hi);
            const uint32_t word = (i & 3u) == 0 ? c0 : (i & 3u) == 1 ? c1 : (i & 3u) == 2 ? c2 : c3;
            const double v = ((double)word * 2.3283064365386963e-10) * W;  // 2^-32: the first product is exact
            const uint32_t k = traj_shot_outcome<T>(psi, s_cdf, gs, L, v);
            if (drawn) drawn[i] = (int32_t)k;
            if (m.measure == 0) {
              atomicAdd(counts + (size_t)sample * D + k, 1u);
            } else {
              for (int w = 0; w < n; ++w)
                if ((k >> w) & 1u) atomicAdd(&s_ones[w], 1u);  // LDS: the item's counts leave once, below
            }
          }
        }
      }
      if (bad) {
        if (tid == 0) atomicOr(flags + sample, 1u);
        if (drawn)
          for (uint32_t i = tid; i < s_t; i += 256) drawn[i] = -1;
      }
      __syncthreads();
    }
    if (m.measure != 0 && tid < n && s_ones[tid] != 0u)  // bit w is wire n-1-w
      atomicAdd(counts + (size_t)sample * n + (n - 1 - tid), s_ones[tid]);
    __syncthreads();
  }
}

// out[b][k] = count / S (PROBS) or (S - 2 ones_w) / S (EXPZ): exact integers and one float64 division per output; the
// row of a sample with a bad trajectory is NaN in every element
__global__ __launch_bounds__(256) void mixed_traj_shots_finalize(const uint32_t* __restrict__ counts,
                                                                 const uint32_t* __restrict__ flags,
                                                                 double* __restrict__ out, int64_t out_ld, int64_t batch,
                                                                 int32_t width, int32_t measure, int32_t shots) {
  const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= (size_t)batch * (size_t)width) return;
  const size_t b = idx / (size_t)width, k = idx - b * (size_t)width;
  const int64_t c = (int64_t)counts[idx];
  const int64_t num = measure == 0 ? c : (int64_t)shots - 2 * c;
  out[b * (size_t)out_ld + k] = flags[b] ? __builtin_nan("") : (double)num / (double)shots;
}

}  // namespace qiddm

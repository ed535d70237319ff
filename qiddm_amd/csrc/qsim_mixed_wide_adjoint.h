// qsim_mixed_wide_adjoint.h -- reverse sweep of the tile-fused density-matrix engine (qsim_mixed_wide.h): the exact
// vector-Jacobian product of qiddm_mixed_wide_forward at n = 7..10, with the mathematics of mixed_backward_kernel
// (qsim_mixed.h).  The reference trains such layers with backprop on default.mixed (nn/qdense.py:71-105,
// src/fashion_noise.py:210-225).
//
// The host plans the program a second time (plan_mixed_wide with split_channels): a segment holds either channels only
// or no channel.  A sample owns 2 + n_snaps slabs: rho sets 0..n_snaps and Lambda.
//   replay    the forward sweeps; a channel segment reads rho set c and writes set c + 1, so set c stays behind as the
//             snapshot (a channel is not inverted).  Channel segments after the last unitary one are not replayed:
//             nothing reads the state behind them.
//   reverse   segments backwards, one launch over (tile, sample) each.
//             unitary segment: mixed_wide_reverse_sweep holds the rho tile and the Lambda tile in LDS and walks the ops
//               backwards: U^dagger . U on both, N = sum B_rho B_Lambda^dagger of the tile in double -> one partial per
//               (slot, tile, sample).  PHASE is element-wise on any wire.  The two-wire unitary (GATE2) is un-computed the
//               same way on the 4 x 4 blocks of its wires: 32 partials, an instantiation of its own.
//             channel segment: mixed_wide_adjoint_channels applies E^dagger to the Lambda tile; rho steps back one set.
//               A segment with a native channel whose strength comes from a row (a >= 0) runs
//               mixed_wide_adjoint_channels_graded instead: it also holds the rho tile in front of each such channel
//               and writes the tile partial of dL/dstrength = <Lambda, E'(rho)> to the channel's slot.  A trailing
//               segment reads the last replayed set as its snapshot, so the host replays up to the last trailing
//               segment that holds such a channel (only programs with one are planned differently).
//               A segment with a general channel whose rows get a gradient (QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT) runs
//               mixed_wide_adjoint_channels_fit (the end of this file): the same with dL/dS of the tile in the op's 32
//               or 512 slots, summed over tiles by mixed_wide_fit_finalize.
//             The first reverse launch generates Lambda_N from grad_out instead of reading it (a measurement table and
//             the reduced density matrix's read-out: a seed launch of their own writes Lambda's slab first).
//   AMP_EMBED dL/dv from Re(Lambda_0) v: a matrix-vector pass over Lambda's slab, then one workgroup per sample.
//   finalize  a wave per parameter (angle row / gate) and sample sums the tile partials in a fixed order: no atomics,
//             reruns are bit-identical and the result does not depend on how the batch is chunked.
#pragma once
#include "qsim_mixed_wide.h"

namespace qiddm {

struct WideBwdScalars {
  int64_t gout_ld;
  int32_t n_slots, seed;  // seed: generate Lambda_N from grad_out instead of reading the slab
};

// a gradient-carrying op of the (segment-sorted) program, grouped by the parameter it feeds
struct WideParam {
  int32_t kind, a, slot, pad_;
  double scale;
};

// the Lambda tile of a reverse launch: read from its slab, or with `seed` generated as Lambda_N from grad_out
template <typename T>
__device__ __forceinline__ void wide_load_lambda(V2<T>* tile, const V2<T>* __restrict__ lam, const uint32_t (&kown)[kWidePairs],
                                                 const double* __restrict__ g, const MixedScalars& m, bool seed) {
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) {  // the test inside: hoisted, all loads are issued at once and cost registers
    if (seed) {
      const uint32_t l = 2u * (threadIdx.x + 256u * i);
      tile[l] = mixed_seed_elem<T>(g, kown[i], m);
      tile[l + 1] = mixed_seed_elem<T>(g, kown[i] + 1u, m);
    } else {
      wide_load_pair<T>(tile, lam, kown, i);
    }
  }
}

// Lambda_N of the measurement table (measure 2), written to every resident sample's Lambda slab in a launch of its own:
// the reverse launches behind it read the slab (seed = 0), so their tile walkers carry no loop over terms.  Grid
// (4^n / 1024, resident samples): a workgroup writes 1024 consecutive elements, the weights of the terms in LDS.
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_obs_seed(const MixedOp* __restrict__ prog,
                                                           const double* __restrict__ grad_out,
                                                           V2<T>* __restrict__ lam_slabs, const MixedScalars m,
                                                           const WideBwdScalars b, int64_t sample0) {
  __shared__ double s_w[256];
  const int n = m.n;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const MixedOp* __restrict__ terms = prog + m.n_ops;
  V2<T>* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  mixed_obs_seed_weights(s_w, grad_out + sample * b.gout_ld, terms, m.n_obs);
  __syncthreads();
  const uint32_t k0 = blockIdx.x * 1024u + threadIdx.x;
#pragma unroll 1
  for (int i = 0; i < 4; ++i) lam[k0 + 256u * i] = mixed_obs_seed_elem<T>(terms, m.n_obs, s_w, k0 + 256u * i, n);
}

// Lambda_N of the reduced density matrix's read-out (measure 8; mixed_rho_seed_elem of qsim_mixed.h: the Hermitian part of
// the cotangent, zero where row and column differ outside the keep-mask), written to every resident sample's Lambda slab in
// a launch of its own beside mixed_wide_obs_seed; the same grid, and the reverse launches behind it read the slab.
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_rho_seed(const double* __restrict__ grad_out,
                                                           V2<T>* __restrict__ lam_slabs, const MixedScalars m,
                                                           const WideBwdScalars b, int64_t sample0, const uint32_t mask) {
  const int n = m.n;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const double* __restrict__ g = grad_out + sample * b.gout_ld;
  V2<T>* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  const uint32_t k0 = blockIdx.x * 1024u + threadIdx.x;
#pragma unroll 1
  for (int i = 0; i < 4; ++i) lam[k0 + 256u * i] = mixed_rho_seed_elem<T>(g, k0 + 256u * i, mask, n);
}

// The kernel writes its loops over the two tiles out (the shared tile copies apart): at 256 vector registers every
// other form of them is scheduled differently, and the float64 round at 10 wires measured 1 % slower on the walkers.
// One unitary segment backwards on the rho tile and the Lambda tile of (tile, sample).  slot[oi] >= 0: the op feeds a
// parameter and writes its tile partial(s) to partials[(resident * n_slots + slot + c) * tiles + tile].
// GATE2: the instantiation that carries the two-wire unitary (32 tile partials; the segments without one run the other).
template <typename T, bool GATE2 = false>
__global__ __launch_bounds__(256) void mixed_wide_reverse_sweep(
    const MixedOp* __restrict__ prog, const int32_t* __restrict__ slot, const double* __restrict__ angle_rows,
    const double* __restrict__ gates, const double* __restrict__ grad_out, V2<T>* __restrict__ rho_slabs,
    V2<T>* __restrict__ lam_slabs, double* __restrict__ partials, const MixedScalars m, const WideSegment sg,
    const WideBwdScalars b, int64_t sample0) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
  __shared__ uint32_t s_lo[64], s_hi[64];
  __shared__ double s_part[2][4][GATE2 ? 32 : 8];
  C* rt = reinterpret_cast<C*>(smem_raw);
  C* lt = rt + kWideTile;
  const int n = m.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  C* __restrict__ rho = rho_slabs + ((size_t)resident << (2 * n));
  C* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  uint32_t kown[kWidePairs];
  wide_owned_indices(sg, s_lo, s_hi, kown);
  wide_load_tile<T>(rt, rho, kown);
  wide_load_lambda<T>(lt, lam, kown, grad_out + sample * b.gout_ld, m, b.seed != 0);
  __syncthreads();

  double* __restrict__ part = partials + (size_t)resident * b.n_slots * gridDim.x + blockIdx.x;
  int buf = 0, prep = -1;
  for (int oi = sg.op_end - 1; oi >= sg.op_begin; --oi) {
    const MixedOp op = prog[oi];
    if (op.kind == kMixZero || op.kind == kMixAmpEmbed) {  // the segment's first op: rho_0 needs no un-computing
      prep = op.kind;
      break;
    }
    const int q = n - 1 - op.wire;
    const int sl = slot[oi];
    int n_vals = 0;
    bool gate2 = false;  // tested in front of the switch: a case label there changes the code of the other instantiation
    if constexpr (GATE2) {
      if (op.kind == kMixGate2) {  // one 4 x 4 block of each tile a thread: N in 32 doubles, both tiles un-computed in place
        const MixedBlock2 bl = wide_block2(op, m, sg);
        const MixedU2<T> u = mixed_unitary2<T>(op, gates);
        double acc[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) acc[k] = 0.0;
        for (uint32_t t = tid; t < kWideTile / 16; t += 256) mixed_block_gate2_reverse<T>(u, acc, rt, lt, mixed_block2_base(t, bl), bl);
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const double s = mixed_wave_sum(acc[k]);
          if (lane == 0) s_part[buf][wave][k] = s;
        }
        n_vals = 32;
        gate2 = true;
      }
    }
    if (!gate2) switch (op.kind) {
      case kMixPhase: {
        // Im Tr(Z N) = Im N00 - Im N11 = sum_k (1 - 2 rowbit_k) Im(rho_k conj(Lambda_k)); the same before and after
        C up, dn;
        mixed_phase_factors<T>(mixed_angle(op, angle_rows, m, sample), up, dn);
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < kWidePairs; ++i) {
          const uint32_t l = 2u * (tid + 256u * i);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const uint32_t k = kown[i] + e;
            const C r = rt[l + e], lm = lt[l + e];
            const double im = (double)cmulc<T>(r, lm).y;
            acc += ((k >> (q + n)) & 1u) ? -im : im;
            rt[l + e] = mixed_phase_elem<T>(r, k, q, n, dn, up);  // the conjugate factors
            lt[l + e] = mixed_phase_elem<T>(lm, k, q, n, dn, up);
          }
        }
        if (sl >= 0) {
          const double s = mixed_wave_sum(acc);
          if (lane == 0) s_part[buf][wave][0] = s;
          n_vals = 1;
        }
        break;
      }
      case kMixRY:
      case kMixGate: {
        const int a = wide_local_rank(sg, q), bb = wide_local_rank(sg, q + n);
        const uint32_t cj = 1u << a, ci = 1u << bb;
        const MixedU<T> u = mixed_unitary<T>(op, angle_rows, gates, m, sample);
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kWideBlocks; ++i) {
          const uint32_t l = insert_two_bits(tid + 256u * i, a, bb);
          C r00 = rt[l], r01 = rt[l | cj], r10 = rt[l | ci], r11 = rt[l | ci | cj];
          C l00 = lt[l], l01 = lt[l | cj], l10 = lt[l | ci], l11 = lt[l | ci | cj];
          mixed_block_n_accumulate<T>(acc, r00, r01, r10, r11, l00, l01, l10, l11);
          mixed_udag_b_u<T>(r00, r01, r10, r11, u.u00, u.u01, u.u10, u.u11);
          mixed_udag_b_u<T>(l00, l01, l10, l11, u.u00, u.u01, u.u10, u.u11);
          rt[l] = r00; rt[l | cj] = r01; rt[l | ci] = r10; rt[l | ci | cj] = r11;
          lt[l] = l00; lt[l | cj] = l01; lt[l | ci] = l10; lt[l | ci | cj] = l11;
        }
        if (op.kind == kMixGate) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const double s = mixed_wave_sum(acc[k]);
            if (lane == 0) s_part[buf][wave][k] = s;
          }
          n_vals = 8;
        } else if (sl >= 0) {  // Im Tr(Y N) = Re N01 - Re N10
          const double s = mixed_wave_sum(acc[2] - acc[4]);
          if (lane == 0) s_part[buf][wave][0] = s;
          n_vals = 1;
        }
        break;
      }
      case kMixCZ: {
        const int qt = n - 1 - op.a;
#pragma unroll
        for (int i = 0; i < kWidePairs; ++i) {
          const uint32_t l = 2u * (tid + 256u * i);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            rt[l + e] = mixed_cz_elem<T>(rt[l + e], kown[i] + e, q, qt, n);
            lt[l + e] = mixed_cz_elem<T>(lt[l + e], kown[i] + e, q, qt, n);
          }
        }
        break;
      }
      case kMixCNOT: {
        const int qt = n - 1 - op.a;
        const int ac = wide_local_rank(sg, q), at = wide_local_rank(sg, qt);
        const int bc = wide_local_rank(sg, q + n), bt = wide_local_rank(sg, qt + n);
#pragma unroll
        for (int i = 0; i < kWideElems; ++i) {
          const uint32_t l = tid + 256u * i;
          const uint32_t pl = l ^ (((l >> ac) & 1u) << at) ^ (((l >> bc) & 1u) << bt);
          if (l < pl) {
            const C tr = rt[l], tl = lt[l];
            rt[l] = rt[pl];
            rt[pl] = tr;
            lt[l] = lt[pl];
            lt[pl] = tl;
          }
        }
        break;
      }
      default: break;
    }
    __syncthreads();
    if (n_vals) {  // uniform over the workgroup; s_part is double-buffered, so the next op may already fill the other half
      if (tid < n_vals)
        part[(size_t)(sl + tid) * gridDim.x] = s_part[buf][0][tid] + s_part[buf][1][tid] + s_part[buf][2][tid] + s_part[buf][3][tid];
      buf ^= 1;
    }
  }
  // rho_0 is not read again, and Lambda_0 only by the AMP_EMBED gradient
  if (prep < 0) wide_store_tile<T>(rho, rt, kown, 0);
  if (prep != kMixZero) wide_store_tile<T>(lam, lt, kown, 0);
}

// One channel segment backwards: E^dagger on the Lambda tile of (tile, sample), ops in reverse.  LEVEL: as in
// mixed_wide_sweep
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_wide_adjoint_channels(const MixedOp* __restrict__ prog,
                                                                   const double* __restrict__ gates,
                                                                   const double* __restrict__ grad_out,
                                                                   V2<T>* __restrict__ lam_slabs, const MixedScalars m,
                                                                   const WideSegment sg, const WideBwdScalars b,
                                                                   int64_t sample0) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
  __shared__ uint32_t s_lo[64], s_hi[64];
  C* lt = reinterpret_cast<C*>(smem_raw);
  const int n = m.n, tid = threadIdx.x;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  C* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  uint32_t kown[kWidePairs];
  wide_owned_indices(sg, s_lo, s_hi, kown);
  wide_load_lambda<T>(lt, lam, kown, grad_out + sample * b.gout_ld, m, b.seed != 0);
  bool owned = true;  // PhaseDamping works on the elements its thread owns: no barrier between two of them
  for (int oi = sg.op_end - 1; oi >= sg.op_begin; --oi) {
    const MixedOp op = prog[oi];
    const bool diag = op.kind == kMixPhaseDamp;
    if (!(diag && owned)) __syncthreads();
    owned = diag;
    const int q = n - 1 - op.wire;
    if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel2) {
      if (op.kind == kMixChannel2) {
        wide_channel2<T, true>(op, lt, gates, m, sg);
        continue;
      }
    }
    if (mixed_channels_of(LEVEL) >= kLevelChannel && op.kind == kMixChannel) {  // S^H on vec of each block
      const MixedSuper<T> su = mixed_super<T>(op, gates);
      wide_walk_blocks<T>(lt, wide_block(sg, q, n),
                          [&](C& l00, C& l01, C& l10, C& l11) { mixed_block_super_adjoint<T>(su, l00, l01, l10, l11); });
      continue;
    }
    const MixedChannel<T> ch = mixed_channel<T>(op.kind, op.p);  // a < 0 throughout: the host sends other segments below
    if (diag) {
      wide_for_owned(kown, [&](uint32_t l, uint32_t k) { lt[l] = mixed_phase_damp_elem<T>(lt[l], k, q, n, ch.off); });
    } else {
      wide_walk_blocks<T>(lt, wide_block(sg, q, n),
                          [&](C& l00, C& l01, C& l10, C& l11) { mixed_block_channel_adjoint<T>(ch, l00, l01, l10, l11); });
    }
  }
  if (!owned) __syncthreads();
  wide_store_tile<T>(lam, lt, kown, 0);
}

// A channel segment that holds a native channel with a >= 0 (strength from a row), backwards: as
// mixed_wide_adjoint_channels on the Lambda tile, with the rho tile beside it in LDS as in mixed_wide_reverse_sweep.
// `rho_slabs` is the state in front of the SEGMENT (its snapshot; read only).  In front of each graded channel (slot[oi]
// >= 0) the rho tile is loaded again and the segment's earlier ops applied to it -- quadratic in the segment's channels,
// which are few, and all in LDS --, then <Lambda, E'(rho)> of the tile goes to partials[(resident * n_slots + slot) *
// tiles + tile]: per thread in double in a fixed order, across the wave, then the four waves in order.
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_wide_adjoint_channels_graded(
    const MixedOp* __restrict__ prog, const int32_t* __restrict__ slot, const double* __restrict__ angle_rows,
    const double* __restrict__ gates, const double* __restrict__ grad_out, const V2<T>* __restrict__ rho_slabs,
    V2<T>* __restrict__ lam_slabs, double* __restrict__ partials, const MixedScalars m, const WideSegment sg,
    const WideBwdScalars b, int64_t sample0) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
  __shared__ uint32_t s_lo[64], s_hi[64];
  __shared__ double s_part[2][4];
  C* lt = reinterpret_cast<C*>(smem_raw);
  C* rt = lt + kWideTile;
  const int n = m.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const C* __restrict__ rho = rho_slabs + ((size_t)resident << (2 * n));
  C* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  uint32_t kown[kWidePairs];
  wide_owned_indices(sg, s_lo, s_hi, kown);
  wide_load_lambda<T>(lt, lam, kown, grad_out + sample * b.gout_ld, m, b.seed != 0);
  __syncthreads();

  double* __restrict__ part = partials + (size_t)resident * b.n_slots * gridDim.x + blockIdx.x;
  int buf = 0;
  for (int oi = sg.op_end - 1; oi >= sg.op_begin; --oi) {
    const MixedOp op = prog[oi];
    const int sl = slot[oi];
    if (sl >= 0) {  // uniform over the workgroup
      wide_load_tile<T>(rt, rho, kown);
      for (int oj = sg.op_begin; oj < oi; ++oj) {
        __syncthreads();
        wide_channel_op<T, LEVEL, false>(prog[oj], rt, kown, angle_rows, gates, m, sg, sample);
      }
      __syncthreads();
      const int q = n - 1 - op.wire;
      const double strength = mixed_angle(op, angle_rows, m, sample);
      double acc_off = 0.0, acc_diag = 0.0;
      if (op.kind == kMixPhaseDamp) {  // any wire: the off-diagonal elements of its blocks among the owned ones
        wide_for_owned(kown, [&](uint32_t l, uint32_t k) {
          if (((k >> (q + n)) ^ (k >> q)) & 1u) acc_off += mixed_re_dot<T>(lt[l], rt[l]);
        });
      } else {  // read only: the one walk over blocks that stores nothing
        const MixedBlock1 bl = wide_block(sg, q, n);
        const uint32_t cj = bl.cj(), ci = bl.ci();
#pragma unroll
        for (int i = 0; i < kWideBlocks; ++i) {
          const uint32_t l = bl.base(tid + 256u * i);
          acc_off += mixed_strength_grad_off<T>(rt[l | cj], rt[l | ci], lt[l | cj], lt[l | ci]);
          acc_diag += mixed_strength_grad_diag<T>(op.kind, rt[l], rt[l | ci | cj], lt[l], lt[l | ci | cj]);
        }
      }
      const double s = mixed_wave_sum(mixed_channel_doff(op.kind, strength) * acc_off + acc_diag);
      if (lane == 0) s_part[buf][wave] = s;
      __syncthreads();
      if (tid == 0) part[(size_t)sl * gridDim.x] = s_part[buf][0] + s_part[buf][1] + s_part[buf][2] + s_part[buf][3];
      buf ^= 1;
    }
    wide_channel_op<T, LEVEL, true>(op, lt, kown, angle_rows, gates, m, sg, sample);
    __syncthreads();
  }
  wide_store_tile<T>(lam, lt, kown, 0);
}

// (Re(Lambda_0) v)_i, one wave per row i of every resident sample's Lambda: lv[resident * 2^n + i]
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_embed_matvec(const V2<T>* __restrict__ lam_slabs,
                                                               const double* __restrict__ feats, double* __restrict__ lv,
                                                               const MixedScalars m, int64_t sample0) {
  const int n = m.n, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t D = 1u << n, i = blockIdx.x * 4u + wave;
  const int64_t resident = blockIdx.y;
  const double* __restrict__ row = feats + (sample0 + resident) * m.feat_ld;
  const V2<T>* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n)) + ((size_t)i << n);
  double acc = 0.0;
  for (uint32_t j = lane; j < D; j += 64) {
    const double vj = j < (uint32_t)m.n_features ? row[j] + m.enc_offset : m.pad_with;
    acc += (double)lam[j].x * vj;
  }
  acc = mixed_wave_sum(acc);
  if (lane == 0) lv[(size_t)resident * D + i] = acc;
}

// dL/dv = 2 (Re(Lambda) v - (v^T Re(Lambda) v / |v|^2) v) / |v|^2 of one sample (the AMP_EMBED step of
// mixed_backward_kernel)
__global__ __launch_bounds__(256) void mixed_wide_embed_grad(const double* __restrict__ feats, const double* __restrict__ lv,
                                                             double* __restrict__ grad_feats, const MixedScalars m,
                                                             int64_t sample0) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  const uint32_t D = 1u << m.n;
  const int64_t sample = sample0 + blockIdx.x;
  const double* __restrict__ row = feats + sample * m.feat_ld;
  const double* __restrict__ l = lv + (size_t)blockIdx.x * D;
  double vv = 0.0, vl = 0.0;
  for (uint32_t k = tid; k < D; k += 256) {
    const double v = k < (uint32_t)m.n_features ? row[k] + m.enc_offset : m.pad_with;
    vv += v * v;
    vl += v * l[k];
  }
  const double inv = 1.0 / mixed_block_sum(vv, s_red);
  const double quad = mixed_block_sum(vl, s_red) * inv;
  for (uint32_t k = tid; k < (uint32_t)m.n_features; k += 256)
    grad_feats[sample * m.n_features + k] = 2.0 * (l[k] - quad * (row[k] + m.enc_offset)) * inv;
}

// One wave per (parameter group, sample): the tile partials of every op of the group, summed lane-strided and then
// across the wave, in program order.  group_begin[g] .. group_begin[g + 1] index `params`; a group's ops share kind and a.
// GATE2: the instantiation for programs with a two-wire unitary (32 values an op where GATE has 8).
template <bool GATE2 = false>
__global__ __launch_bounds__(256) void mixed_wide_grad_finalize(const WideParam* __restrict__ params,
                                                                const int32_t* __restrict__ group_begin, int32_t n_groups,
                                                                const double* __restrict__ gates,
                                                                const double* __restrict__ partials,
                                                                double* __restrict__ grad_rows, double* __restrict__ grad_gates,
                                                                int32_t n_slots, int32_t n_gates, uint32_t tiles,
                                                                int64_t batch, int64_t sample0) {
  constexpr int kMaxVals = GATE2 ? 32 : 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + wave;
  if (g >= n_groups) return;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const double* __restrict__ part = partials + (size_t)resident * n_slots * tiles;
  const int begin = group_begin[g], end = group_begin[g + 1];
  const WideParam head = params[begin];
  double go[kMaxVals];
  for (int k = 0; k < kMaxVals; ++k) go[k] = 0.0;
  for (int pi = begin; pi < end; ++pi) {
    const WideParam p = params[pi];
    const int n_vals = GATE2 && p.kind == kMixGate2 ? 32 : p.kind == kMixGate ? 8 : 1;
    double s[kMaxVals];
    const auto tile_sum = [&](int c) {
      const double* __restrict__ src = part + (size_t)(p.slot + c) * tiles;
      double v = 0.0;
      for (uint32_t t = lane; t < tiles; t += 64) v += src[t];
      return mixed_wave_sum(v);
    };
    if constexpr (GATE2) {  // unrolled with the count tested inside: 32 sums indexed by a variable would live in scratch
#pragma unroll
      for (int c = 0; c < kMaxVals; ++c)
        if (c < n_vals) s[c] = tile_sum(c);
    } else {
      for (int c = 0; c < n_vals; ++c) s[c] = tile_sum(c);
    }
    if (GATE2 && p.kind == kMixGate2) mixed_gate2_grad_accumulate(s, gates + (size_t)p.a * 8, go);
    else if (p.kind == kMixGate) mixed_gate_grad_accumulate(s, gates + (size_t)p.a * 8, go);
    else go[0] += p.scale * s[0];
  }
  if (lane != 0) return;
  if (GATE2 && head.kind == kMixGate2) {
    double* __restrict__ dst = grad_gates + ((size_t)sample * n_gates + head.a) * 8;  // rows a .. a+3
    for (int k = 0; k < 32; ++k) dst[k] = go[k];
  } else if (head.kind == kMixGate) {
    double* __restrict__ dst = grad_gates + ((size_t)sample * n_gates + head.a) * 8;
    for (int k = 0; k < 8; ++k) dst[k] = go[k];
  } else {
    grad_rows[(size_t)head.a * batch + sample] = go[0];
  }
}

// ---- general channels whose rows get a gradient (QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT) ---------------------------------
// The host uploads them as kMixChannel / kMixChannel2, so the replay and every kernel above run them as the constant
// kinds; what marks them is slot[oi] >= 0 on a general channel.  Segments that hold one run the kernel below, programs
// without one launch nothing of this section.
//
// mixed_wide_adjoint_channels_graded with the general channels' dL/dS beside the native channels' dL/dstrength (it carries
// every channel case: one instantiation per precision).  In front of each op with a slot the rho tile is rebuilt as
// there; then, with W[r][c] = sum over the tile's blocks of conj(vec(Lambda)[r]) vec(rho)[c] (mixed_super_grad_accumulate,
// mixed_super2_grad of qsim_mixed.h), the tile partials Re W, -Im W go to the op's 32 (one wire) or 512 (two wires) slots
// in the layout of the rows.  One wire: a thread's blocks, the wave, the four waves.  Two wires: thread 16 r + c owns
// W[r][c] and walks the tile's 256 blocks in order.
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_adjoint_channels_fit(
    const MixedOp* __restrict__ prog, const int32_t* __restrict__ slot, const double* __restrict__ angle_rows,
    const double* __restrict__ gates, const double* __restrict__ grad_out, const V2<T>* __restrict__ rho_slabs,
    V2<T>* __restrict__ lam_slabs, double* __restrict__ partials, const MixedScalars m, const WideSegment sg,
    const WideBwdScalars b, int64_t sample0) {
  using C = V2<T>;
  constexpr int LEVEL = kLevelChannel2;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
  __shared__ uint32_t s_lo[64], s_hi[64];
  __shared__ double s_part[2][4][32];
  C* lt = reinterpret_cast<C*>(smem_raw);
  C* rt = lt + kWideTile;
  const int n = m.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const C* __restrict__ rho = rho_slabs + ((size_t)resident << (2 * n));
  C* __restrict__ lam = lam_slabs + ((size_t)resident << (2 * n));
  uint32_t kown[kWidePairs];
  wide_owned_indices(sg, s_lo, s_hi, kown);
  wide_load_lambda<T>(lt, lam, kown, grad_out + sample * b.gout_ld, m, b.seed != 0);
  __syncthreads();

  double* __restrict__ part = partials + (size_t)resident * b.n_slots * gridDim.x + blockIdx.x;
  int buf = 0;
  for (int oi = sg.op_end - 1; oi >= sg.op_begin; --oi) {
    const MixedOp op = prog[oi];
    const int sl = slot[oi];
    if (sl >= 0) {  // uniform over the workgroup
      wide_load_tile<T>(rt, rho, kown);
      for (int oj = sg.op_begin; oj < oi; ++oj) {
        __syncthreads();
        wide_channel_op<T, LEVEL, false>(prog[oj], rt, kown, angle_rows, gates, m, sg, sample);
      }
      __syncthreads();
      const int q = n - 1 - op.wire;
      if (op.kind == kMixChannel2) {
        double re, im;
        mixed_super2_grad<T>(lt, rt, kWideTile / 16, wide_block2(op, m, sg), re, im);
        part[(size_t)(sl + 2 * tid) * gridDim.x] = re;
        part[(size_t)(sl + 2 * tid + 1) * gridDim.x] = -im;
        __syncthreads();  // every thread has read all of the Lambda tile
      } else if (op.kind == kMixChannel) {
        const MixedBlock1 bl = wide_block(sg, q, n);
        const uint32_t cj = bl.cj(), ci = bl.ci();
        double acc[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) acc[k] = 0.0;
#pragma unroll
        for (int i = 0; i < kWideBlocks; ++i) {
          const uint32_t l = bl.base(tid + 256u * i);
          const C lv[4] = {lt[l], lt[l | cj], lt[l | ci], lt[l | ci | cj]};
          const C rv[4] = {rt[l], rt[l | cj], rt[l | ci], rt[l | ci | cj]};
          mixed_super_grad_accumulate<T>(acc, lv, rv);
        }
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const double s = mixed_wave_sum(acc[k]);
          if (lane == 0) s_part[buf][wave][k] = s;
        }
        __syncthreads();
        if (tid < 32) {
          const double s = s_part[buf][0][tid] + s_part[buf][1][tid] + s_part[buf][2][tid] + s_part[buf][3][tid];
          part[(size_t)(sl + tid) * gridDim.x] = (tid & 1) ? -s : s;
        }
        buf ^= 1;
      } else {  // a native channel with a >= 0: as in mixed_wide_adjoint_channels_graded
        const double strength = mixed_angle(op, angle_rows, m, sample);
        double acc_off = 0.0, acc_diag = 0.0;
        if (op.kind == kMixPhaseDamp) {
          wide_for_owned(kown, [&](uint32_t l, uint32_t k) {
            if (((k >> (q + n)) ^ (k >> q)) & 1u) acc_off += mixed_re_dot<T>(lt[l], rt[l]);
          });
        } else {
          const MixedBlock1 bl = wide_block(sg, q, n);
          const uint32_t cj = bl.cj(), ci = bl.ci();
#pragma unroll
          for (int i = 0; i < kWideBlocks; ++i) {
            const uint32_t l = bl.base(tid + 256u * i);
            acc_off += mixed_strength_grad_off<T>(rt[l | cj], rt[l | ci], lt[l | cj], lt[l | ci]);
            acc_diag += mixed_strength_grad_diag<T>(op.kind, rt[l], rt[l | ci | cj], lt[l], lt[l | ci | cj]);
          }
        }
        const double s = mixed_wave_sum(mixed_channel_doff(op.kind, strength) * acc_off + acc_diag);
        if (lane == 0) s_part[buf][wave][0] = s;
        __syncthreads();
        if (tid == 0) part[(size_t)sl * gridDim.x] = s_part[buf][0][0] + s_part[buf][1][0] + s_part[buf][2][0] + s_part[buf][3][0];
        buf ^= 1;
      }
    }
    wide_channel_op<T, LEVEL, true>(op, lt, kown, angle_rows, gates, m, sg, sample);
    __syncthreads();
  }
  wide_store_tile<T>(lam, lt, kown, 0);
}

// kWideFitChunks workgroups per (group of trainable channels that name the same rows, sample), 32 values each (a one-wire
// group uses the first): a wave per value sums the tile partials of every op of the group, lane-strided and then across
// the wave, in program order, and ADDS the result to the rows of grad_gates (the host has zeroed them;
// mixed_wide_grad_finalize, launched in front, may have written a GATE2 of the same four rows).  params[..].kind is
// kMixChannel (32 values) or kMixChannel2 (512).
constexpr int kWideFitChunks = 16;
__global__ __launch_bounds__(256) void mixed_wide_fit_finalize(const WideParam* __restrict__ params,
                                                               const int32_t* __restrict__ group_begin,
                                                               const double* __restrict__ partials,
                                                               double* __restrict__ grad_gates, int32_t n_slots,
                                                               int32_t n_gates, uint32_t tiles, int64_t sample0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  const double* __restrict__ part = partials + (size_t)resident * n_slots * tiles;
  const int group = blockIdx.x / kWideFitChunks, first = 32 * (blockIdx.x % kWideFitChunks);
  const int begin = group_begin[group], end = group_begin[group + 1];
  const WideParam head = params[begin];
  const int n_vals = head.kind == kMixChannel2 ? 512 : 32;
  if (first >= n_vals) return;
  double* __restrict__ dst = grad_gates + ((size_t)sample * n_gates + head.a) * 8;
  for (int c = first + wave; c < first + 32; c += 4) {
    double go = 0.0;
    for (int pi = begin; pi < end; ++pi) {
      const double* __restrict__ src = part + (size_t)(params[pi].slot + c) * tiles;
      double v = 0.0;
      for (uint32_t t = lane; t < tiles; t += 64) v += src[t];
      go += mixed_wave_sum(v);
    }
    if (lane == 0) dst[c] += go;
  }
}

}  // namespace qiddm

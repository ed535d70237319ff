// qsim_traj_adjoint.h -- the reverse sweep of the quantum-trajectory engine (qsim_traj.h): gradients of the mean read-out
// of n_traj Monte-Carlo wavefunctions per sample, for the programs of qiddm_mixed_traj_forward up to 16 wires.
//
// THE ESTIMATOR.  The exact read-out is E(theta) = sum_b <psi_0| M_b(theta)^H O M_b(theta) |psi_0>, over every branch
// sequence b (one Kraus operator per channel op), M_b the unnormalised product of gates and chosen operators.  The
// forward samples b with probability p_b = |M_b psi_0|^2, so
//     grad E = sum_b grad <.>_b = E_{b ~ p}[ grad <psi_0| M_b^H O M_b |psi_0> / p_b ].
// The forward renormalises at every decision and the product of the chosen weights w_d is p_b.  The gradient of one
// trajectory is therefore the vector-Jacobian product of a LINEAR, NON-UNITARY chain in which channel op d is the matrix
// A_d = K_{k_d}(theta) / sqrt(w_d), the branch k_d and the number w_d frozen at the values the forward took and only K's own
// dependence on theta differentiated.  The mean over the trajectories is an unbiased estimate of the gradient the
// density-matrix sweeps return; no separate score-function term is needed: it is inside the 1 / sqrt(w_d).
//
// Execution shape: the forward's.  One workgroup of 256 threads per trajectory; work items (sample, slot), S = min(T, 64),
// trajectory t in slot t mod S; workgroups stride the items.
//   replay     the forward rule unchanged (traj_channel / traj_apply_op of qsim_traj.h: the same Philox words, reductions and
//              roundings, so the branches and psi_N are the forward's bit for bit).  In front of every channel op psi is
//              copied to a snapshot in the workspace; behind the snapshot sits the decision's record (TrajDecision: the
//              2 x 2 matrix as applied, rounded to the state's dtype, w_d, the strength, the branch).
//   seed       lambda_N = (sum_j g_j O_j) psi_N, g the sample's row of grad_out.
//   walk back  for op i with psi_i = A_i psi_{i-1}: the gradient of a real parameter theta of A_i is
//              2 Re <lambda_i| dA_i/dtheta |psi_{i-1}>, then lambda_{i-1} = A_i^H lambda_i; psi_{i-1} = A_i^H psi_i for the
//              unitary ops and the snapshot for channel ops (Kraus operators are singular in general).
//              Every one-wire op reduces W_ab = sum over the wire's pairs of conj(lambda_a) psi_{i-1,b}; all its gradients
//              are real-linear in W: dL/dRe A_ab = 2 Re W_ab, dL/dIm A_ab = -2 Im W_ab.
//              A two-wire Kraus op (kMixKraus2) walks back in GATE2's case: 32 sums W_rc over the quadruples, psi_{i-1} from
//              its snapshot, the applied 4 x 4 matrix rebuilt from (gate rows, branch, w_d) by the forward's traj_kraus2_matrix;
//              rows a + 4 k_d .. a + 4 k_d + 3 get GATE2's entry gradients over sqrt(w_d).
// psi and lambda live in dynamic LDS while 2 * 2^n elements fit in 128 KiB (n <= 13 in float32, n <= 12 in float64), else
// in two slabs per workgroup in the workspace; snapshots are always in the workspace.
// Sums: traj_block_sum (float64 partials in ascending index, a wave butterfly, four partials in wave order); no atomics.
// A trajectory's gradient is collected in a float64 row of the workgroup (n_rows + 8 n_gates + n_features wide, thread 0
// adds an op's values behind the op's barrier, features belong to thread k mod 256), then added to the row of its (sample,
// slot) in ascending t (the first stored).  mixed_traj_grad_finalize adds the S rows in ascending slot, divides by n_traj and
// writes the three gradient layouts of qiddm_mixed_backward.  Reruns and any grid give the same bits.
#pragma once
#include "qsim_traj.h"

namespace qiddm {

constexpr int kTrajRecordBytes = 256;  // behind every snapshot: the decision's TrajDecision

struct TrajDecision {
  double u[8];  // the applied matrix (u00, u01, u10, u11) as (re, im), the values of the state's dtype
  double w, strength;
  int32_t chosen, pad_;
};
static_assert(sizeof(TrajDecision) <= kTrajRecordBytes, "record room");

struct TrajBwdScalars {
  int64_t gout_ld, snap_stride;  // snap_stride: bytes from one snapshot to the next, 2^n elements + kTrajRecordBytes
  int32_t n_rows, n_gates, n_features, gwidth;  // gwidth = n_rows + 8 n_gates + n_features: a gradient row
};

template <typename T>
__device__ __forceinline__ double traj_cre(V2<T> l, V2<T> p) {  // Re(conj(l) p)
  return (double)l.x * (double)p.x + (double)l.y * (double)p.y;
}
template <typename T>
__device__ __forceinline__ double traj_cim(V2<T> l, V2<T> p) {  // Im(conj(l) p)
  return (double)l.x * (double)p.y - (double)l.y * (double)p.x;
}

// A one-wire op on bit q backwards.  `snap`: psi_{i-1} (a channel op), else psi_{i-1} = U^H psi_i.  With `sums`,
// w[2 (2a + b)], w[2 (2a + b) + 1] = Re, Im of W_ab = sum over the pairs of conj(lambda_a) psi_{i-1,b}, in every thread.
// Then lambda <- U^H lambda and psi <- psi_{i-1}.  The caller's barrier follows.
template <typename T>
__device__ __forceinline__ void traj_reverse1(V2<T>* psi, V2<T>* lam, const V2<T>* snap, uint32_t half, int q,
                                              const MixedU<T>& u, bool sums, double (&w)[8], double* s_red) {
  using C = V2<T>;
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = 0.0;
  for (uint32_t t = threadIdx.x; t < half; t += 256) {
    const uint32_t i0 = traj_insert_bit(t, q), i1 = i0 | (1u << q);
    const C l0 = lam[i0], l1 = lam[i1];
    C p0, p1;
    if (snap) {
      p0 = snap[i0];
      p1 = snap[i1];
    } else {
      const C x0 = psi[i0], x1 = psi[i1];
      p0 = cmulc<T>(x0, u.u00) + cmulc<T>(x1, u.u10);
      p1 = cmulc<T>(x0, u.u01) + cmulc<T>(x1, u.u11);
    }
    if (sums) {
      w[0] += traj_cre<T>(l0, p0);
      w[1] += traj_cim<T>(l0, p0);
      w[2] += traj_cre<T>(l0, p1);
      w[3] += traj_cim<T>(l0, p1);
      w[4] += traj_cre<T>(l1, p0);
      w[5] += traj_cim<T>(l1, p0);
      w[6] += traj_cre<T>(l1, p1);
      w[7] += traj_cim<T>(l1, p1);
    }
    lam[i0] = cmulc<T>(l0, u.u00) + cmulc<T>(l1, u.u10);
    lam[i1] = cmulc<T>(l0, u.u01) + cmulc<T>(l1, u.u11);
    psi[i0] = p0;
    psi[i1] = p1;
  }
  if (sums) traj_block_sum<8>(w, s_red);
}

// A two-wire op backwards (GATE2, KRAUS2): w[2 (4 r + c)], +1 = Re, Im of W_rc = sum over the quadruples of
// conj(lambda_r) psi_{i-1,c}.  `snap`: psi_{i-1} (KRAUS2: the operator is singular), else psi_{i-1} = U^H psi_i.
template <typename T>
__device__ __forceinline__ void traj_reverse2(V2<T>* psi, V2<T>* lam, const V2<T>* snap, uint32_t quarter, int q, int q2,
                                              const MixedU2<T>& u, double (&w)[32], double* s_red) {
  using C = V2<T>;
  const int qlo = q < q2 ? q : q2, qhi = q < q2 ? q2 : q;
#pragma unroll
  for (int j = 0; j < 32; ++j) w[j] = 0.0;
  for (uint32_t t = threadIdx.x; t < quarter; t += 256) {
    const uint32_t base = insert_two_bits(t, qlo, qhi);
    const uint32_t at[4] = {base, base | (1u << q2), base | (1u << q), base | (1u << q) | (1u << q2)};
    const C x[4] = {psi[at[0]], psi[at[1]], psi[at[2]], psi[at[3]]};
    const C l[4] = {lam[at[0]], lam[at[1]], lam[at[2]], lam[at[3]]};
    C p[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      p[c] = snap ? snap[at[c]]
                  : (cmulc<T>(x[0], u.u[0][c]) + cmulc<T>(x[1], u.u[1][c])) + (cmulc<T>(x[2], u.u[2][c]) + cmulc<T>(x[3], u.u[3][c]));
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        w[2 * (4 * r + c)] += traj_cre<T>(l[r], p[c]);
        w[2 * (4 * r + c) + 1] += traj_cim<T>(l[r], p[c]);
      }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      lam[at[c]] = (cmulc<T>(l[0], u.u[0][c]) + cmulc<T>(l[1], u.u[1][c])) + (cmulc<T>(l[2], u.u[2][c]) + cmulc<T>(l[3], u.u[3][c]));
      psi[at[c]] = p[c];
    }
  }
  traj_block_sum<32>(w, s_red);
}

// lambda_N = (sum_j g_j O_j) psi_N.  s_term: 256 doubles of LDS.  The caller's barrier follows.
template <typename T>
__device__ __forceinline__ void traj_seed(const V2<T>* psi, V2<T>* lam, const double* __restrict__ g,
                                          const MixedOp* __restrict__ terms, const MixedScalars& m, double* s_term) {
  using C = V2<T>;
  const int n = m.n, tid = threadIdx.x;
  const uint32_t D = 1u << n;
  if (m.measure == 0) {
    for (uint32_t k = tid; k < D; k += 256) {
      const C a = psi[k];
      const double gk = g[k];
      lam[k] = C{(T)(gk * (double)a.x), (T)(gk * (double)a.y)};
    }
  } else if (m.measure == 1) {
    if (tid < n) s_term[tid] = g[tid];  // wire tid, at bit n-1-tid
    __syncthreads();
    for (uint32_t k = tid; k < D; k += 256) {
      double s = 0.0;
      for (int w = 0; w < n; ++w) s += ((k >> (n - 1 - w)) & 1u) ? -s_term[w] : s_term[w];
      const C a = psi[k];
      lam[k] = C{(T)(s * (double)a.x), (T)(s * (double)a.y)};
    }
  } else {  // (P psi)_j = i^ny (-1)^popcount((j ^ x) & z) psi_{j ^ x}: traj_read_out's sign and i^ny conventions
    if (tid < m.n_obs) s_term[tid] = g[terms[tid].wire2] * terms[tid].p;
    __syncthreads();
    for (uint32_t j = tid; j < D; j += 256) {
      double re = 0.0, im = 0.0;
      for (int t = 0; t < m.n_obs; ++t) {
        const uint32_t x = (uint32_t)terms[t].wire, z = (uint32_t)terms[t].a;
        const int ny = __popc(x & z) & 3;
        const C a = psi[j ^ x];
        const double c = (__popc((j ^ x) & z) & 1) ? -s_term[t] : s_term[t];
        const double ax = (double)a.x, ay = (double)a.y;
        re += c * (ny == 0 ? ax : ny == 1 ? -ay : ny == 2 ? -ax : ay);
        im += c * (ny == 0 ? ay : ny == 1 ? ax : ny == 2 ? -ay : -ax);
      }
      lam[j] = C{(T)re, (T)im};
    }
  }
}

// grid: any number of workgroups up to batch * n_slots.  acc: (batch, n_slots, gwidth) float64; rows: one gradient row per
// workgroup; snaps: n_channels snapshots of snap_stride bytes per workgroup; slabs: 2 * 2^n elements per workgroup unless
// psi and lambda are in LDS.  per_traj_grad (batch, n_traj, gwidth) float64 and branches (batch, n_traj, n_channels) int32
// may be NULL.
template <typename T, bool K2>
__global__ __launch_bounds__(256) void mixed_traj_backward_kernel(
    const MixedOp* __restrict__ prog, const double* __restrict__ angle_rows, const double* __restrict__ feats,
    const double* __restrict__ gates, const double* __restrict__ grad_out, double* __restrict__ acc,
    double* __restrict__ rows, unsigned char* __restrict__ snaps, V2<T>* __restrict__ slabs,
    double* __restrict__ per_traj_grad, int32_t* __restrict__ branches, const MixedScalars m, const TrajScalars tr,
    const TrajBwdScalars b) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[128];   // traj_block_sum<32>
  __shared__ double s_term[256];  // one per term of the measurement table
  const int n = m.n, tid = threadIdx.x;
  const uint32_t D = 1u << n, half = D >> 1;
  C* const psi = tr.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : slabs + ((size_t)blockIdx.x << (n + 1));
  C* const lam = psi + D;
  unsigned char* const my_snaps = snaps + (size_t)blockIdx.x * (size_t)tr.n_channels * (size_t)b.snap_stride;
  double* const tg = rows + (size_t)blockIdx.x * b.gwidth;  // this trajectory's gradient
  const int off_gates = b.n_rows, off_feats = b.n_rows + 8 * b.n_gates;
  const int64_t items = m.batch * tr.n_slots;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t sample = item / tr.n_slots;
    const int slot = (int)(item - sample * tr.n_slots);
    double* __restrict__ acc_row = acc + (size_t)item * b.gwidth;
    for (int t = slot; t < tr.n_traj; t += tr.n_slots) {
      const size_t traj = (size_t)sample * tr.n_traj + t;
      for (int k = tid; k < b.gwidth; k += 256) tg[k] = 0.0;
      // ---- replay: the forward, with a snapshot and a record in front of every channel op ------------------------------
      uint32_t d = 0;
      bool bad = false;
      for (int oi = 0; oi < m.n_ops; ++oi) {
        const MixedOp op = prog[oi];
        if (K2 ? traj_is_channel(op.kind) : traj_is_channel1(op.kind)) {
          int chosen = -1;
          if (!bad) {
            unsigned char* const at = my_snaps + (size_t)d * (size_t)b.snap_stride;
            C* const snap = reinterpret_cast<C*>(at);
            TrajDecision* const rec = reinterpret_cast<TrajDecision*>(at + ((size_t)D * sizeof(C)));
            for (uint32_t k = tid; k < D; k += 256) snap[k] = psi[k];
            // the copy is strided by element, the op's sweep by pair: without this barrier a wave that is done copying
            // could apply X / Y / Z of a DEPOL decision (no reduction, so no barrier of its own) to elements another wave
            // has yet to copy
            __syncthreads();
            if (K2 && op.kind == kMixKraus2) {  // the record keeps (chosen, w): the walk back rebuilds the 4 x 4 matrix from them
              if constexpr (K2)
                chosen = traj_channel2<T>(psi, op, gates, m, tr, sample, (uint32_t)t, d, s_red, [&](int k, double w) {
                  if (tid == 0) {
                    rec->w = w;
                    rec->strength = 0.0;
                    rec->chosen = k;
                  }
                });
            } else
              chosen = traj_channel<T>(psi, op, angle_rows, gates, m, tr, sample, (uint32_t)t, d, s_red,
                                       [&](int k, const MixedU<T>& u, double w, double strength) {
                                         if (tid == 0) {
                                           rec->u[0] = (double)u.u00.x; rec->u[1] = (double)u.u00.y;
                                           rec->u[2] = (double)u.u01.x; rec->u[3] = (double)u.u01.y;
                                           rec->u[4] = (double)u.u10.x; rec->u[5] = (double)u.u10.y;
                                           rec->u[6] = (double)u.u11.x; rec->u[7] = (double)u.u11.y;
                                           rec->w = w;
                                           rec->strength = strength;
                                           rec->chosen = k;
                                         }
                                       });
            bad = chosen < 0;
          }
          if (branches && tid == 0) branches[traj * tr.n_channels + d] = chosen;
          ++d;
        } else if (!bad) {
          traj_apply_op<T>(psi, op, angle_rows, feats, gates, m, sample, s_red);
        }
        __syncthreads();
      }
      if (!bad) {
        // ---- seed ------------------------------------------------------------------------------------------------------
        traj_seed<T>(psi, lam, grad_out + sample * b.gout_ld, prog + m.n_ops, m, s_term);
        __syncthreads();
        // ---- walk back -------------------------------------------------------------------------------------------------
        for (int oi = m.n_ops - 1; oi >= 0; --oi) {
          const MixedOp op = prog[oi];
          const int q = n - 1 - op.wire;
          const bool kraus2 = K2 && op.kind == kMixKraus2;  // walked back in GATE2's case
          switch (kraus2 ? (int)kMixGate2 : op.kind) {
            case kMixPhase: {  // RZ: dA = diag(-i/2 dn, +i/2 up): 2 Re(dA_00 W_00 + dA_11 W_11) = Im(dn W_00) - Im(up W_11)
              double sn, cs;
              sincos(0.5 * mixed_angle(op, angle_rows, m, sample), &sn, &cs);
              MixedU<T> u;
              u.u00 = C{(T)cs, (T)-sn};
              u.u11 = C{(T)cs, (T)sn};
              u.u01 = u.u10 = C{(T)0, (T)0};
              double w[8];
              traj_reverse1<T>(psi, lam, nullptr, half, q, u, op.a >= 0, w, s_red);
              if (op.a >= 0 && tid == 0) tg[op.a] += op.scale * ((cs * w[1] - sn * w[0]) - (cs * w[7] + sn * w[6]));
              break;
            }
            case kMixRY: {  // dU = 1/2 [[-s, -c], [c, -s]]
              double sn, cs;
              sincos(0.5 * mixed_angle(op, angle_rows, m, sample), &sn, &cs);
              double w[8];
              traj_reverse1<T>(psi, lam, nullptr, half, q, mixed_unitary<T>(op, angle_rows, gates, m, sample), op.a >= 0, w, s_red);
              if (op.a >= 0 && tid == 0) tg[op.a] += op.scale * (cs * (w[4] - w[2]) - sn * (w[0] + w[6]));
              break;
            }
            case kMixGate: {
              double w[8];
              traj_reverse1<T>(psi, lam, nullptr, half, q, mixed_unitary<T>(op, angle_rows, gates, m, sample), true, w, s_red);
              if (tid == 0) {
                double* __restrict__ go = tg + off_gates + (size_t)op.a * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) go[j] += (j & 1) ? -2.0 * w[j] : 2.0 * w[j];
              }
              break;
            }
            case kMixGate2: {  // one sweep for both: KRAUS2 is GATE2 with A = K_k / sqrt(w_d) and psi_{i-1} from the snapshot
              const C* snap = nullptr;
              size_t row = (size_t)op.a;
              double s = 2.0;
              MixedU2<T> u;
              if (kraus2) {
                --d;
                const unsigned char* const at = my_snaps + (size_t)d * (size_t)b.snap_stride;
                const TrajDecision* const rec = reinterpret_cast<const TrajDecision*>(at + ((size_t)D * sizeof(C)));
                const int chosen = rec->chosen;
                const double wd = rec->w;
                snap = reinterpret_cast<const C*>(at);
                u = traj_kraus2_matrix<T>(gates, op.a, chosen, wd);
                row += 4 * (size_t)chosen;  // the chosen operator's rows; the op's other rows keep their zeros
                s = 2.0 / sqrt(wd);
              } else {
                u = mixed_unitary2<T>(op, gates);
              }
              double w[32];
              traj_reverse2<T>(psi, lam, snap, D >> 2, q, n - 1 - op.wire2, u, w, s_red);
              if (tid == 0) {
                double* __restrict__ go = tg + off_gates + row * 8;
#pragma unroll
                for (int j = 0; j < 32; ++j) go[j] += (j & 1) ? -s * w[j] : s * w[j];
              }
              break;
            }
            case kMixCZ: {
              const uint32_t both = (1u << q) | (1u << (n - 1 - op.a));
              for (uint32_t k = tid; k < D; k += 256)
                if ((k & both) == both) {
                  psi[k] = -psi[k];
                  lam[k] = -lam[k];
                }
              break;
            }
            case kMixCNOT: {
              const int qt = n - 1 - op.a;
              const int qlo = q < qt ? q : qt, qhi = q < qt ? qt : q;
              for (uint32_t k = tid; k < (D >> 2); k += 256) {
                const uint32_t i0 = insert_two_bits(k, qlo, qhi) | (1u << q), i1 = i0 | (1u << qt);
                const C a0 = psi[i0], l0 = lam[i0];
                psi[i0] = psi[i1];
                psi[i1] = a0;
                lam[i0] = lam[i1];
                lam[i1] = l0;
              }
              break;
            }
            case kMixPhaseDamp:
            case kMixAmpDamp:
            case kMixDepol:
            case kMixKraus: {
              --d;
              const unsigned char* const at = my_snaps + (size_t)d * (size_t)b.snap_stride;
              const C* const snap = reinterpret_cast<const C*>(at);
              const TrajDecision rec = *reinterpret_cast<const TrajDecision*>(at + ((size_t)D * sizeof(C)));
              MixedU<T> u;
              u.u00 = C{(T)rec.u[0], (T)rec.u[1]};
              u.u01 = C{(T)rec.u[2], (T)rec.u[3]};
              u.u10 = C{(T)rec.u[4], (T)rec.u[5]};
              u.u11 = C{(T)rec.u[6], (T)rec.u[7]};
              const bool kraus = op.kind == kMixKraus;
              const bool graded = !kraus && op.a >= 0;
              double w[8];
              traj_reverse1<T>(psi, lam, snap, half, q, u, kraus || graded, w, s_red);
              if (tid == 0) {
                if (kraus) {  // the chosen operator's row: GATE's formula over sqrt(w_d); the other rows keep their zeros
                  const double s = 2.0 / sqrt(rec.w);
                  double* __restrict__ go = tg + off_gates + (size_t)(op.a + rec.chosen) * 8;
#pragma unroll
                  for (int j = 0; j < 8; ++j) go[j] += (j & 1) ? -s * w[j] : s * w[j];
                } else if (graded) {
                  // Re <lambda_i | psi_i> = Re sum_ab A_ab W_ab: dK_k/ds / sqrt(w_d) is a multiple of A_d in every case
                  // but k = 0 of the two damping channels
                  const double overlap = (rec.u[0] * w[0] - rec.u[1] * w[1]) + (rec.u[2] * w[2] - rec.u[3] * w[3]) +
                                         (rec.u[4] * w[4] - rec.u[5] * w[5]) + (rec.u[6] * w[6] - rec.u[7] * w[7]);
                  double g;
                  if (op.kind == kMixDepol)
                    g = rec.chosen == 0 ? -overlap / (1.0 - rec.strength) : overlap / rec.strength;
                  else
                    g = rec.chosen == 0 ? -w[6] / (sqrt(1.0 - rec.strength) * sqrt(rec.w)) : overlap / rec.strength;
                  tg[op.a] += op.scale * g;
                }
              }
              break;
            }
            case kMixAmpEmbed: {  // op 0: psi_0 = v / |v|, g = 2 Re lambda_0, dL/dv = (g - (g . psi_0) psi_0) / |v|
              const double* __restrict__ row = feats + (size_t)sample * m.feat_ld;
              double part[2] = {0.0, 0.0};
              for (uint32_t k = tid; k < D; k += 256) {
                const double v = k < (uint32_t)m.n_features ? row[k] + m.enc_offset : m.pad_with;
                part[0] += v * v;
                part[1] += 2.0 * (double)lam[k].x * v;
              }
              traj_block_sum<2>(part, s_red);
              const double inv = 1.0 / sqrt(part[0]);
              const double gdot = part[1] * inv;
              for (uint32_t k = tid; k < (uint32_t)b.n_features; k += 256) {
                const double v = row[k] + m.enc_offset;
                tg[off_feats + k] += (2.0 * (double)lam[k].x - gdot * (v * inv)) * inv;
              }
              break;
            }
            default:
              break;
          }
          __syncthreads();
        }
      }
      // ---- this trajectory's row to the item's accumulator, in ascending t ----------------------------------------------
      double* __restrict__ own = per_traj_grad ? per_traj_grad + traj * b.gwidth : nullptr;
      const bool first = t == slot;
      for (int k = tid; k < b.gwidth; k += 256) {
        const double v = bad ? __builtin_nan("") : tg[k];
        acc_row[k] = first ? v : acc_row[k] + v;
        if (own) own[k] = v;
      }
      __syncthreads();
    }
  }
}

// column j of a sample's gradient row = (acc[b][0][j] + acc[b][1][j] + ... in ascending slot) / n_traj, written where
// qiddm_mixed_backward writes it: grad_rows (n_rows, batch), grad_gates (batch, n_gates, 8), grad_feats (batch, n_features)
__global__ __launch_bounds__(256) void mixed_traj_grad_finalize(const double* __restrict__ acc, double* __restrict__ grad_rows,
                                                                double* __restrict__ grad_gates,
                                                                double* __restrict__ grad_feats, int64_t batch,
                                                                const TrajScalars tr, const TrajBwdScalars b) {
  const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= (size_t)batch * b.gwidth) return;
  const size_t s = idx / b.gwidth, j = idx - s * b.gwidth;
  const double* __restrict__ a = acc + s * (size_t)tr.n_slots * b.gwidth + j;
  double sum = 0.0;
  for (int slot = 0; slot < tr.n_slots; ++slot) sum += a[(size_t)slot * b.gwidth];
  const double v = sum / (double)tr.n_traj;
  const size_t off_feats = (size_t)b.n_rows + 8 * (size_t)b.n_gates;
  if (j < (size_t)b.n_rows)
    grad_rows[j * (size_t)batch + s] = v;
  else if (j < off_feats)
    grad_gates[s * (size_t)b.n_gates * 8 + (j - b.n_rows)] = v;
  else
    grad_feats[s * (size_t)b.n_features + (j - off_feats)] = v;
}

}  // namespace qiddm

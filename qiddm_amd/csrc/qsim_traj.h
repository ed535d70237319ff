// qsim_traj.h -- quantum trajectories (Monte-Carlo wavefunctions) for the programs of the density-matrix executor:
// default.mixed beyond the 10 wires at which one sample's rho stops fitting (8 MiB there, 32 GiB at 16).  A trajectory
// keeps a PURE state psi (2^n elements, wire w at bit n-1-w), draws one Kraus operator at every channel with probability
// |K_k psi|^2, renormalises, and reads out; the mean over n_traj trajectories estimates the density-matrix result with
// an error that falls as 1 / sqrt(n_traj).  The rule (weights, the Philox word of a decision, the operator lists of
// the native channels) is stated in include/qiddm_hip_traj.h under QIDDM_MIX_KRAUS and THE TRAJECTORY RULE; this file
// follows it line by line and tests/_mixed_traj_ref.py restates it in numpy.
//
// Execution shape: that of the one-workgroup engine (qsim_mixed.h).  A workgroup of 256 threads runs one trajectory at
// a time; psi lives in dynamic LDS while 2^n elements fit in 128 KiB (n <= 14 in float32, n <= 13 in float64: the
// launch asks for exactly 2^n elements, so small registers share a CU), else in the workgroup's slab of the workspace.
// Every op is one sweep over psi between two barriers.
//   work item (sample b, slot s), s = 0 .. S-1, S = min(n_traj, 64): the trajectories t = s, s + S, s + 2S, ... of sample
//   b in ascending t, their read-outs added into the item's own float64 accumulator row in the workspace (the first
//   one is stored: nothing is cleared).  Workgroups stride the items, so neither the grid nor its cap decides which
//   values are added in which order.  mixed_traj_finalize adds the S rows of a sample in ascending s and divides by
//   n_traj.  No float atomics anywhere: reruns and any grid give the same bits.
//   Every element of an accumulator row is owned by one thread for all trajectories of the item (element k by thread
//   k mod 256, <Z_w> by thread w, a table column by the thread of its first term).
// A two-wire channel given by its Kraus operators (kMixKraus2) is one channel op as well: traj_channel2 draws among up to
// sixteen 4 x 4 operators from the reduced matrix of the pair (two sweeps over psi: a read for the matrix, a read and a
// write for the apply).  The kernels are templates on K2, whether the program holds such an op: see traj_is_channel1.
// Sums over psi (the reduced matrix of a wire or a pair, the read-outs): float64 per-thread partials in ascending index, a wave
// butterfly, four partials in LDS added in wave order -- the shots kernel's reduction.
#pragma once
#include "qsim_mixed.h"
#include "qsim_philox.h"

namespace qiddm {

constexpr int kMixKraus = 40;       // general one-wire channel by its Kraus operators: gates[a .. a + wire2), wire2 = 1 .. 8
constexpr int kTrajMaxKraus = 8;    // ThermalRelaxationError has six
constexpr int kMixKraus2 = 48;      // general two-wire channel by its Kraus operators on (wire, wire2): p = m = 1 .. 16 of them,
                                    // operator k in gates[a + 4k .. a + 4k + 3] (GATE2's layout, one matrix after another)
constexpr int kTrajMaxKraus2 = 16;  // two-wire depolarizing has sixteen; a Choi matrix of 16 x 16 never needs more
constexpr int kTrajMaxSlots = 64;   // S = min(n_traj, 64)
constexpr int kTrajMaxTraj = 1 << 20;

struct TrajScalars {
  int32_t n_traj, n_slots, n_channels, width;  // n_channels: channel ops of the program (decisions of a trajectory)
  uint32_t seed_lo, seed_hi, offset;
  int32_t slab_in_lds;
};

// the one-wire channel ops, and every channel op.  The kernels exist twice: K2 = false is the kernel that knows no two-wire
// Kraus op -- the device code of every program without one, to the instruction what it was before the op existed -- and
// K2 = true carries it; the host launches K2 = true only for a program that holds a kMixKraus2.
__host__ __device__ constexpr bool traj_is_channel1(int kind) {
  return kind == kMixPhaseDamp || kind == kMixAmpDamp || kind == kMixDepol || kind == kMixKraus;
}
__host__ __device__ constexpr bool traj_is_channel(int kind) { return traj_is_channel1(kind) || kind == kMixKraus2; }

__device__ __forceinline__ uint32_t traj_insert_bit(uint32_t t, int q) {
  return ((t >> q) << (q + 1)) | (t & ((1u << q) - 1u));
}

// the sums of every thread's v[0 .. K), in a fixed order, handed to every thread (s_red: 4 K doubles, free on return)
template <int K>
__device__ __forceinline__ void traj_block_sum(double (&v)[K], double* s_red) {
  const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = mixed_wave_sum(v[j]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) s_red[wave * K + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = ((s_red[j] + s_red[K + j]) + s_red[2 * K + j]) + s_red[3 * K + j];
  __syncthreads();
}

template <typename T>
__device__ __forceinline__ double traj_norm2(V2<T> a) {
  return (double)a.x * (double)a.x + (double)a.y * (double)a.y;
}

// psi <- (u on bit q) psi
template <typename T>
__device__ __forceinline__ void traj_apply1(V2<T>* psi, uint32_t half, int q, const MixedU<T>& u) {
  for (uint32_t t = threadIdx.x; t < half; t += 256) {
    const uint32_t i0 = traj_insert_bit(t, q), i1 = i0 | (1u << q);
    const V2<T> a0 = psi[i0], a1 = psi[i1];
    psi[i0] = cmul<T>(u.u00, a0) + cmul<T>(u.u01, a1);
    psi[i1] = cmul<T>(u.u10, a0) + cmul<T>(u.u11, a1);
  }
}

// the reduced matrix of the wire at bit q, unnormalised: r[0] = sum |a0|^2, r[1] = sum |a1|^2, r[2] + i r[3] = sum a0 conj(a1)
// over the pairs (a0, a1) = (psi[bit clear], psi[bit set])
template <typename T>
__device__ __forceinline__ void traj_wire_rho(const V2<T>* psi, uint32_t half, int q, double* s_red, double (&r)[4]) {
  r[0] = r[1] = r[2] = r[3] = 0.0;
  for (uint32_t t = threadIdx.x; t < half; t += 256) {
    const uint32_t i0 = traj_insert_bit(t, q), i1 = i0 | (1u << q);
    const V2<T> a0 = psi[i0], a1 = psi[i1];
    const double x0 = (double)a0.x, y0 = (double)a0.y, x1 = (double)a1.x, y1 = (double)a1.y;
    r[0] += x0 * x0 + y0 * y0;
    r[1] += x1 * x1 + y1 * y1;
    r[2] += x0 * x1 + y0 * y1;
    r[3] += y0 * x1 - x0 * y1;
  }
  traj_block_sum<4>(r, s_red);
}

// w_k = |K psi|^2 from the wire's reduced matrix, K = (k00, k01, k10, k11) as (re, im); never negative
__device__ __forceinline__ double traj_kraus_weight(const double* __restrict__ g, const double (&r)[4]) {
  const double n0 = g[0] * g[0] + g[1] * g[1] + g[4] * g[4] + g[5] * g[5];
  const double n1 = g[2] * g[2] + g[3] * g[3] + g[6] * g[6] + g[7] * g[7];
  // c = k00 conj(k01) + k10 conj(k11)
  const double cx = g[0] * g[2] + g[1] * g[3] + g[4] * g[6] + g[5] * g[7];
  const double cy = g[1] * g[2] - g[0] * g[3] + g[5] * g[6] - g[4] * g[7];
  return fmax(n0 * r[0] + n1 * r[1] + 2.0 * (cx * r[2] - cy * r[3]), 0.0);
}

struct TrajNoRecord {
  template <typename U>
  __device__ __forceinline__ void operator()(int, const U&, double, double) const {}
};

// One channel op of one trajectory: weights, the decision, psi <- K psi / sqrt(w).  Returns the operator chosen, or -1
// when the total weight is not positive or not finite (psi is then left as it is).  The same value in every thread.
// `record(chosen, u, w, strength)` is told the 2 x 2 matrix as applied (rounded to T), the chosen weight and the op's
// strength before psi changes: the reverse sweep (qsim_traj_adjoint.h) keeps them; the forward passes nothing.
template <typename T, typename R = TrajNoRecord>
__device__ __forceinline__ int traj_channel(V2<T>* psi, const MixedOp& op, const double* __restrict__ angle_rows,
                                            const double* __restrict__ gates, const MixedScalars& m, const TrajScalars& tr,
                                            int64_t sample, uint32_t t, uint32_t d, double* s_red, R&& record = R{}) {
  using C = V2<T>;
  const int q = m.n - 1 - op.wire;
  const uint32_t half = 1u << (m.n - 1);
  double w[kTrajMaxKraus];
  int count;
  double strength = 0.0;
  if (op.kind == kMixKraus) {
    double r[4];
    traj_wire_rho<T>(psi, half, q, s_red, r);
    count = op.wire2;
#pragma unroll
    for (int k = 0; k < kTrajMaxKraus; ++k) w[k] = k < count ? traj_kraus_weight(gates + (size_t)(op.a + k) * 8, r) : 0.0;
  } else {
    strength = mixed_angle(op, angle_rows, m, sample);
#pragma unroll
    for (int k = 0; k < kTrajMaxKraus; ++k) w[k] = 0.0;
    if (op.kind == kMixDepol) {
      count = 4;
      w[0] = 1.0 - strength;
      w[1] = w[2] = w[3] = strength / 3.0;
    } else {
      double r[4];
      traj_wire_rho<T>(psi, half, q, s_red, r);
      count = 2;
      w[0] = r[0] + (1.0 - strength) * r[1];
      w[1] = strength * r[1];
    }
  }
  double cum[kTrajMaxKraus], total = 0.0;  // c_k, the running sum; W = c_{count - 1}
#pragma unroll
  for (int k = 0; k < kTrajMaxKraus; ++k) {
    if (k < count) total += w[k];
    cum[k] = total;
  }
  if (!(total > 0.0) || !isfinite(total)) return -1;
  uint32_t c0 = d >> 2, c1 = t, c2 = (uint32_t)sample, c3 = tr.offset;
  philox4x32_10(c0, c1, c2, c3, tr.seed_lo, tr.seed_hi);
  const uint32_t word = (d & 3u) == 0 ? c0 : (d & 3u) == 1 ? c1 : (d & 3u) == 2 ? c2 : c3;
  const double v = ((double)word * 2.3283064365386963e-10) * total;  // 2^-32: the first product is exact
  int chosen = 0;
#pragma unroll
  for (int k = 0; k < kTrajMaxKraus; ++k) chosen += (k < count && cum[k] <= v) ? 1 : 0;
  chosen = chosen < count - 1 ? chosen : count - 1;
  double wk = 0.0;
#pragma unroll
  for (int k = 0; k < kTrajMaxKraus; ++k) wk = k == chosen ? w[k] : wk;
  const double s = 1.0 / sqrt(wk);
  MixedU<T> u;
  const C zero = C{(T)0, (T)0};
  if (op.kind == kMixKraus) {
    const double* __restrict__ g = gates + (size_t)(op.a + chosen) * 8;
    u.u00 = C{(T)(g[0] * s), (T)(g[1] * s)};
    u.u01 = C{(T)(g[2] * s), (T)(g[3] * s)};
    u.u10 = C{(T)(g[4] * s), (T)(g[5] * s)};
    u.u11 = C{(T)(g[6] * s), (T)(g[7] * s)};
  } else if (op.kind == kMixDepol) {
    if (chosen == 0) {  // K_0 / sqrt(w_0) is the identity
      u.u00 = u.u11 = C{(T)1, (T)0};
      u.u01 = u.u10 = zero;
      record(0, u, wk, strength);
      return 0;
    }
    u.u00 = chosen == 3 ? C{(T)1, (T)0} : zero;
    u.u11 = chosen == 3 ? C{(T)-1, (T)0} : zero;
    u.u01 = chosen == 1 ? C{(T)1, (T)0} : chosen == 2 ? C{(T)0, (T)-1} : zero;
    u.u10 = chosen == 1 ? C{(T)1, (T)0} : chosen == 2 ? C{(T)0, (T)1} : zero;
  } else {
    u.u00 = chosen == 0 ? C{(T)s, (T)0} : zero;
    u.u10 = zero;
    if (chosen == 0) {
      u.u01 = zero;
      u.u11 = C{(T)(sqrt(1.0 - strength) * s), (T)0};
    } else if (op.kind == kMixPhaseDamp) {
      u.u01 = zero;
      u.u11 = C{(T)(sqrt(strength) * s), (T)0};
    } else {
      u.u01 = C{(T)(sqrt(strength) * s), (T)0};
      u.u11 = zero;
    }
  }
  record(chosen, u, wk, strength);
  traj_apply1<T>(psi, half, q, u);
  return chosen;
}

// ---- the two-wire Kraus op (kMixKraus2) ----------------------------------------------------------------------------------
// The reduced matrix of the pair at bits (q, q2), unnormalised, over the quadruples a_0 .. a_3 of psi (index 2 b(q) + b(q2)):
// R[r][c] = sum a_r conj(a_c), r <= c.  r[0 .. 3] the diagonal; the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) follow as (re, im).
template <typename T>
__device__ __forceinline__ void traj_pair_rho(const V2<T>* psi, uint32_t quarter, int q, int q2, double* s_red, double (&r)[16]) {
  const int qlo = q < q2 ? q : q2, qhi = q < q2 ? q2 : q;
#pragma unroll
  for (int j = 0; j < 16; ++j) r[j] = 0.0;
  for (uint32_t t = threadIdx.x; t < quarter; t += 256) {
    const uint32_t base = insert_two_bits(t, qlo, qhi);
    const V2<T> a[4] = {psi[base], psi[base | (1u << q2)], psi[base | (1u << q)], psi[base | (1u << q) | (1u << q2)]};
    double x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = (double)a[j].x;
      y[j] = (double)a[j].y;
      r[j] += x[j] * x[j] + y[j] * y[j];
    }
    int at = 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = j + 1; c < 4; ++c) {
        r[at] += x[j] * x[c] + y[j] * y[c];
        r[at + 1] += y[j] * x[c] - x[j] * y[c];
        at += 2;
      }
  }
  traj_block_sum<16>(r, s_red);
}

// w = max(0, Tr(K R K^H)) = sum_r G[r][r] R[r][r] + 2 Re sum_{r<c} G[c][r] R[r][c], G = K^H K; g: the operator's four gate rows
__device__ __forceinline__ double traj_kraus2_weight(const double* __restrict__ g, const double (&r)[16]) {
  double w = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) d += g[(4 * i + j) * 2] * g[(4 * i + j) * 2] + g[(4 * i + j) * 2 + 1] * g[(4 * i + j) * 2 + 1];
    w += d * r[j];
  }
  int at = 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = j + 1; c < 4; ++c) {
      double gre = 0.0, gim = 0.0;  // G[c][j] = sum_i conj(K[i][c]) K[i][j]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double cx = g[(4 * i + c) * 2], cy = g[(4 * i + c) * 2 + 1], jx = g[(4 * i + j) * 2], jy = g[(4 * i + j) * 2 + 1];
        gre += cx * jx + cy * jy;
        gim += cx * jy - cy * jx;
      }
      w += 2.0 * (gre * r[at] - gim * r[at + 1]);
      at += 2;
    }
  return fmax(w, 0.0);
}

// A = K_chosen / sqrt(w): formed in float64, rounded once to T, uniform like mixed_unitary2's.  The forward applies it and
// the reverse sweep rebuilds it from (gate rows, chosen, w) by this code: the same values.
template <typename T>
__device__ __forceinline__ MixedU2<T> traj_kraus2_matrix(const double* __restrict__ gates, int a, int chosen, double w) {
  const double* __restrict__ g = gates + ((size_t)a + 4 * (size_t)chosen) * 8;
  const double s = 1.0 / sqrt(w);
  MixedU2<T> u;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      u.u[r][c] = V2<T>{mixed_uniform((T)(g[(r * 4 + c) * 2] * s)), mixed_uniform((T)(g[(r * 4 + c) * 2 + 1] * s))};
  return u;
}

struct TrajNoRecord2 {
  __device__ __forceinline__ void operator()(int, double) const {}
};

// One two-wire Kraus op of one trajectory; traj_channel's contract.  The weights do not stay in registers (sixteen of them
// and their running sums would be 64): thread k < m computes w_k into LDS, every thread adds them from there in ascending
// k.  psi is swept twice: a read for R, a read and a write for the apply.  `record(chosen, w)` is called before psi changes.
template <typename T, typename R = TrajNoRecord2>
__device__ __forceinline__ int traj_channel2(V2<T>* psi, const MixedOp& op, const double* __restrict__ gates,
                                             const MixedScalars& m, const TrajScalars& tr, int64_t sample, uint32_t t,
                                             uint32_t d, double* s_red, R&& record = R{}) {
  using C = V2<T>;
  __shared__ double s_weight[kTrajMaxKraus2];
  const int tid = threadIdx.x;
  const int q = m.n - 1 - op.wire, q2 = m.n - 1 - op.wire2;
  const int qlo = q < q2 ? q : q2, qhi = q < q2 ? q2 : q;
  const uint32_t quarter = 1u << (m.n - 2);
  const int count = (int)op.p;
  {
    double r[16];
    traj_pair_rho<T>(psi, quarter, q, q2, s_red, r);
    if (tid < count) s_weight[tid] = traj_kraus2_weight(gates + ((size_t)op.a + 4 * (size_t)tid) * 8, r);
  }
  __syncthreads();
  double total = 0.0;  // W = c_{count - 1}
  for (int k = 0; k < count; ++k) total += s_weight[k];
  if (!(total > 0.0) || !isfinite(total)) return -1;
  uint32_t c0 = d >> 2, c1 = t, c2 = (uint32_t)sample, c3 = tr.offset;
  philox4x32_10(c0, c1, c2, c3, tr.seed_lo, tr.seed_hi);
  const uint32_t word = (d & 3u) == 0 ? c0 : (d & 3u) == 1 ? c1 : (d & 3u) == 2 ? c2 : c3;
  const double v = ((double)word * 2.3283064365386963e-10) * total;  // 2^-32: the first product is exact
  int chosen = 0;
  double cum = 0.0;  // c_k, the same sequential sums as `total`
  for (int k = 0; k < count; ++k) {
    cum += s_weight[k];
    chosen += cum <= v ? 1 : 0;
  }
  chosen = chosen < count - 1 ? chosen : count - 1;
  const double wk = s_weight[chosen];
  const MixedU2<T> u = traj_kraus2_matrix<T>(gates, op.a, chosen, wk);
  record(chosen, wk);
  for (uint32_t i = tid; i < quarter; i += 256) {  // GATE2's sweep
    const uint32_t base = insert_two_bits(i, qlo, qhi);
    const uint32_t at[4] = {base, base | (1u << q2), base | (1u << q), base | (1u << q) | (1u << q2)};
    const C a[4] = {psi[at[0]], psi[at[1]], psi[at[2]], psi[at[3]]};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      psi[at[r]] = (cmul<T>(u.u[r][0], a[0]) + cmul<T>(u.u[r][1], a[1])) + (cmul<T>(u.u[r][2], a[2]) + cmul<T>(u.u[r][3], a[3]));
  }
  return chosen;
}

// a unitary op or a state preparation on psi; the caller's barrier follows
template <typename T>
__device__ __forceinline__ void traj_apply_op(V2<T>* psi, const MixedOp& op, const double* __restrict__ angle_rows,
                                              const double* __restrict__ feats, const double* __restrict__ gates,
                                              const MixedScalars& m, int64_t sample, double* s_red) {
  using C = V2<T>;
  const int n = m.n, tid = threadIdx.x;
  const uint32_t D = 1u << n;
  const int q = n - 1 - op.wire;
  switch (op.kind) {
    case kMixZero:
      for (uint32_t k = tid; k < D; k += 256) psi[k] = C{(T)(k == 0 ? 1 : 0), (T)0};
      break;
    case kMixAmpEmbed: {
      const double* __restrict__ row = feats + (size_t)sample * m.feat_ld;
      double part[1] = {0.0};
      for (uint32_t k = tid; k < D; k += 256) {
        const double v = k < (uint32_t)m.n_features ? row[k] + m.enc_offset : m.pad_with;
        part[0] += v * v;
      }
      traj_block_sum<1>(part, s_red);
      const double inv = 1.0 / sqrt(part[0]);
      for (uint32_t k = tid; k < D; k += 256) {
        const double v = k < (uint32_t)m.n_features ? row[k] + m.enc_offset : m.pad_with;
        psi[k] = C{(T)(v * inv), (T)0};
      }
      break;
    }
    case kMixPhase: {  // RZ: diag(e^{-i phi / 2}, e^{+i phi / 2})
      C up, dn;
      mixed_phase_factors<T>(0.5 * mixed_angle(op, angle_rows, m, sample), up, dn);
      for (uint32_t k = tid; k < D; k += 256) psi[k] = cmul<T>(psi[k], ((k >> q) & 1u) ? up : dn);
      break;
    }
    case kMixRY:
    case kMixGate:
      traj_apply1<T>(psi, D >> 1, q, mixed_unitary<T>(op, angle_rows, gates, m, sample));
      break;
    case kMixCZ: {
      const uint32_t both = (1u << q) | (1u << (n - 1 - op.a));
      for (uint32_t k = tid; k < D; k += 256)
        if ((k & both) == both) psi[k] = -psi[k];
      break;
    }
    case kMixCNOT: {
      const int qt = n - 1 - op.a;
      const int qlo = q < qt ? q : qt, qhi = q < qt ? qt : q;
      for (uint32_t t = tid; t < (D >> 2); t += 256) {
        const uint32_t i0 = insert_two_bits(t, qlo, qhi) | (1u << q), i1 = i0 | (1u << qt);
        const C a0 = psi[i0];
        psi[i0] = psi[i1];
        psi[i1] = a0;
      }
      break;
    }
    case kMixGate2: {  // index 2 b(wire) + b(wire2), the first wire most significant
      const int q2 = n - 1 - op.wire2;
      const int qlo = q < q2 ? q : q2, qhi = q < q2 ? q2 : q;
      const MixedU2<T> u = mixed_unitary2<T>(op, gates);
      for (uint32_t t = tid; t < (D >> 2); t += 256) {
        const uint32_t base = insert_two_bits(t, qlo, qhi);
        const uint32_t at[4] = {base, base | (1u << q2), base | (1u << q), base | (1u << q) | (1u << q2)};
        const C a[4] = {psi[at[0]], psi[at[1]], psi[at[2]], psi[at[3]]};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          psi[at[r]] = (cmul<T>(u.u[r][0], a[0]) + cmul<T>(u.u[r][1], a[1])) + (cmul<T>(u.u[r][2], a[2]) + cmul<T>(u.u[r][3], a[3]));
      }
      break;
    }
    default:
      break;
  }
}

// `emit(k, value)`: element k of this trajectory's read-out, called once per element, always by the same thread
template <typename T, typename E>
__device__ __forceinline__ void traj_read_out(const V2<T>* psi, const MixedOp* __restrict__ terms, const MixedScalars& m,
                                              double* s_red, double* s_term, E&& emit) {
  const int n = m.n, tid = threadIdx.x, lane = tid & 63;
  const uint32_t D = 1u << n;
  if (m.measure == 0) {
    for (uint32_t k = tid; k < D; k += 256) emit(k, traj_norm2<T>(psi[k]));
  } else if (m.measure == 1) {
    double z[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) z[w] = 0.0;
    for (uint32_t k = tid; k < D; k += 256) {
      const double pk = traj_norm2<T>(psi[k]);
#pragma unroll
      for (int w = 0; w < 16; ++w) z[w] += ((k >> w) & 1u) ? -pk : pk;  // by bit; wire n-1-w
    }
    traj_block_sum<16>(z, s_red);
#pragma unroll
    for (int w = 0; w < 16; ++w)
      if (tid == n - 1 - w) emit((uint32_t)tid, z[w]);
  } else {  // the measurement table: rho[k][k ^ x] = psi_k conj(psi_{k ^ x}); mixed_obs_read_out's formula and order
    for (int t = mixed_obs_wave(); t < m.n_obs; t += 4) {
      const uint32_t x = (uint32_t)terms[t].wire, z = (uint32_t)terms[t].a;
      const int ny = __popc(x & z) & 3;
      const bool flip = ny == 1 || ny == 2;
      double part = 0.0;
      for (uint32_t k = lane; k < D; k += 64) {
        const V2<T> a = psi[k], b = psi[k ^ x];
        const double re = (double)a.x * (double)b.x + (double)a.y * (double)b.y;
        const double im = (double)a.y * (double)b.x - (double)a.x * (double)b.y;
        const double c = (ny & 1) ? im : re;
        part += (((__popc(k & z) & 1) != 0) != flip) ? -c : c;
      }
      const double total = mixed_wave_sum(part);
      if (lane == 0) s_term[t] = terms[t].p * total;
    }
    __syncthreads();
    if (tid < m.n_obs) {
      const int col = terms[tid].wire2;
      if (tid == 0 || terms[tid - 1].wire2 != col) {
        double s = 0.0;
        for (int u = tid; u < m.n_obs && terms[u].wire2 == col; ++u) s += s_term[u];
        emit((uint32_t)col, s);
      }
    }
    __syncthreads();
  }
}

// grid: any number of workgroups up to batch * n_slots; they stride the work items.  acc: (batch, n_slots, width) float64.
// per_traj (batch, n_traj, width) float64 and branches (batch, n_traj, n_channels) int32 may be NULL.
template <typename T, bool K2>
__global__ __launch_bounds__(256) void mixed_traj_kernel(const MixedOp* __restrict__ prog,
                                                         const double* __restrict__ angle_rows,
                                                         const double* __restrict__ feats,
                                                         const double* __restrict__ gates, double* __restrict__ acc,
                                                         V2<T>* __restrict__ slabs, double* __restrict__ per_traj,
                                                         int32_t* __restrict__ branches, const MixedScalars m,
                                                         const TrajScalars tr) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[64];
  __shared__ double s_term[256];  // one per term of the measurement table
  C* psi = tr.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : slabs + ((size_t)blockIdx.x << m.n);
  const int tid = threadIdx.x;
  const int64_t items = m.batch * tr.n_slots;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t sample = item / tr.n_slots;
    const int slot = (int)(item - sample * tr.n_slots);
    double* __restrict__ acc_row = acc + (size_t)item * tr.width;
    for (int t = slot; t < tr.n_traj; t += tr.n_slots) {
      const size_t traj = (size_t)sample * tr.n_traj + t;
      uint32_t d = 0;
      bool bad = false;
      for (int oi = 0; oi < m.n_ops; ++oi) {
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
      double* __restrict__ own = per_traj ? per_traj + traj * tr.width : nullptr;
      const bool first = t == slot;
      const auto emit = [&](uint32_t k, double v) {
        acc_row[k] = first ? v : acc_row[k] + v;
        if (own) own[k] = v;
      };
      if (bad) {  // the total weight of a decision was not positive or not finite: the row is NaN
        for (uint32_t k = tid; k < (uint32_t)tr.width; k += 256) emit(k, __builtin_nan(""));
      } else {
        traj_read_out<T>(psi, prog + m.n_ops, m, s_red, s_term, emit);
      }
      __syncthreads();
    }
  }
}

// out[b][k] = (acc[b][0][k] + acc[b][1][k] + ... in ascending slot) / n_traj
__global__ __launch_bounds__(256) void mixed_traj_finalize(const double* __restrict__ acc, double* __restrict__ out,
                                                           int64_t out_ld,
                                                           int64_t batch, const TrajScalars tr) {
  const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= (size_t)batch * tr.width) return;
  const size_t b = idx / tr.width, k = idx - b * tr.width;
  const double* __restrict__ a = acc + b * (size_t)tr.n_slots * tr.width + k;
  double s = 0.0;
  for (int slot = 0; slot < tr.n_slots; ++slot) s += a[(size_t)slot * tr.width];
  out[b * (size_t)out_ld + k] = s / (double)tr.n_traj;
}

}  // namespace qiddm

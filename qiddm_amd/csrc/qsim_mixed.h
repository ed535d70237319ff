// qsim_mixed.h -- density-matrix execution for the hardware-noise study.
//
// Reference: the `*_noise.py` drivers re-create the layers' QNodes on `default.mixed` for sampling
// (src/mnist_noise.py:214-229) and the `_circuit` bodies insert PhaseDamping / AmplitudeDamping /
// DepolarizingChannel after the encoders or in front of the read-out (nn/qdense.py:98-104, 255-261, 1410-1417).
// PennyLane's default.mixed keeps rho (2^n x 2^n, complex128) and applies U rho U^dagger / sum_k K rho K^dagger.
//
// Here one workgroup owns one sample's rho, index (i << n) | j (i: ket/row, j: bra/column; wire w is bit n-1-w of
// each half).  rho lives in LDS while it fits, else in a per-workgroup slab of the caller's workspace (L2-resident:
// 512 KiB at n = 8 in float32).  The circuit arrives as a short program (the host expands templates and rings):
// every op is one sweep over rho, separated by workgroup barriers.  Single-qubit unitaries and channels work on the
// 2 x 2 blocks M = rho[(b_i, b_j)] of their wire:
//     unitary U:            M <- U M U^dagger
//     PhaseDamping(g):      M01, M10 *= sqrt(1-g)
//     AmplitudeDamping(g):  M00 += g M11;  M11 *= 1-g;  M01, M10 *= sqrt(1-g)
//     Depolarizing(p):      M00, M11 <- (1-2p/3) own + (2p/3) other;  M01, M10 *= 1-4p/3
//     general channel S:    vec(M) <- S vec(M), vec(M) = (M00, M01, M10, M11), S = sum_k K_k (x) conj(K_k) (4 x 4 complex)
// (the Kraus sums of PennyLane's channel definitions, written out; the general one carries BitFlip, PhaseFlip,
// PauliError, GeneralizedAmplitudeDamping, ResetError, ThermalRelaxationError and QubitChannel).  The general TWO-wire
// channel works on the 4 x 4 blocks M[r][c] of its wires (r = 2 b_w1 + b_w2 from the row bits, c from the column bits):
// vec(M) <- S vec(M), vec(M)[4r + c] = M[r][c], S 16 x 16 complex (mixed_block_super2 below; two-qubit depolarizing
// behind an entangler, correlated dephasing, a two-letter PauliError, a measured two-qubit process).
// The two-wire unitary works on the same 4 x 4 blocks: M <- U M U^dagger (mixed_block_gate2 below; SWAP, controlled
// rotations, Ising gates, a learned two-qubit gate), and is un-computed in the reverse sweep like a one-wire gate.
// Diagonal gates multiply by u_i conj(u_j); CZ by
// sign(i) sign(j); CNOT permutes rows and columns (an involution: swapped in place).  Read-out: the diagonal -- or, for
// a program that ends in kMixShots, estimates from that many shots drawn from it in the launch (qsim_mixed_shots.h); for a
// program that ends in a table of kMixObs terms, Pauli-word expectation values from the off-diagonals (mixed_obs_read_out);
// for a program that ends in kMixRho, the reduced density matrix of the kept wires (mixed_rho_read_out).
// mixed_backward_kernel (below) differentiates the same programs: PennyLane trains QNodes on default.mixed with
// backprop or parameter-shift.  n <= 8.
//
// How the code is laid out (this file and the tile-fused engine, qsim_mixed_wide*.h): three layers.
//   arithmetic  what a kind does to one 2 x 2 block or one element, in registers: mixed_block_* and mixed_*_elem.
//   walking     where a wire's blocks sit (MixedBlock1) and the load / call / store of one block
//               (mixed_block_visit); mixed_walk_blocks loops over a thread's blocks of a slab, wide_walk_blocks over
//               its blocks of a tile.
//   kernels     mixed_apply_op (every op of the forward, and of the backward's replay) under mixed_replay in the two
//               forward kernels.  mixed_backward_kernel and mixed_wide_reverse_sweep write their block loops out; the
//               notes in front of them say why.
#pragma once
#include "qsim_fused.h"
#include "qsim_mixed_shots.h"

namespace qiddm {

enum MixedKind : int32_t {
  kMixZero = 0,     // rho = |0..0><0..0|
  kMixAmpEmbed,     // rho = |v><v| / |v|^2, v = features + offset padded with pad_with
  kMixPhase,        // diag(1, e^{i phi}) up to a global phase; phi = p + scale * angle_rows[a][sample] (a < 0: constant)
  kMixRY,           // RY(theta), theta as above
  kMixGate,         // fixed unitary gates[a]
  kMixCZ,           // control wire, target a
  kMixCNOT,         // control wire, target a
  kMixPhaseDamp,    // gamma = p, or with a >= 0 p + scale * angle_rows[a][sample] (not clamped; the row gets a gradient)
  kMixAmpDamp,      // gamma likewise
  kMixDepol,        // p likewise
  kMixShots = 12,   // last op only, not an op on rho: the read-out is estimated from `a` shots (qsim_mixed_shots.h);
                    // the host keeps it out of the ops the kernels walk and hands its fields over as a MixedShots
  kMixChannel = 16, // general one-wire channel: gates[a .. a+3] are the rows of the 4 x 4 superoperator S (10..15: no kind)
  kMixObs = 20,     // tail of the program, not an op on rho: one term of the measurement table (coefficient p times the
                    // Pauli word with x-mask `wire` and z-mask `a`, output column wire2); see mixed_obs_read_out
  kMixGate2 = 24,   // fixed two-wire unitary on (wire, wire2): gates[a .. a+3] are the rows of the 4 x 4 U (a unitary, not a
                    // channel: un-computed in the reverse sweeps, and its rows get a gradient)
  kMixRho = 28,     // last op only, not an op on rho: the read-out is the reduced density matrix of the wires in the keep-mask
                    // `wire` (wire w at bit n-1-w); see mixed_rho_read_out
  kMixChannel2 = 32,  // general two-wire channel on (wire, wire2): gates[a .. a+63] hold the 16 x 16 S (17, 19, 21..23, 25..27, 29..31: no kind)
  // 16 k + 2: the k-wire channel whose rows get a gradient.  The forwards and the tile-fused engine never see these two:
  // the host uploads them as kMixChannel / kMixChannel2 (and marks them by their slot); mixed_backward_kernel's kLevelFit
  // instantiations read them and take them for the constant kinds wherever rho and Lambda are concerned.
  kMixChannelFit = 18,
  kMixChannel2Fit = 34,
};

struct MixedOp {
  int32_t kind, wire, a, wire2;  // wire2: qiddm_mixed_op_t's `reserved`, read by kMixChannel2 / kMixGate2 (second wire) and kMixObs (column)
  double p, scale;
};

// Which general-channel cases an instantiation carries: each costs vector registers, so a program (tile-fused engine: a
// segment) runs the lowest level that holds its ops.  A level carries the cases below it.  kLevelGate2 is a flag beside
// the level: the two-wire unitary is no channel, and a unitary-only program that holds one carries no channel case.
enum MixedLevel : int {
  kLevelLean = 0,     // the five-scalar channels only
  kLevelChannel = 1,  // + kMixChannel
  kLevelChannel2 = 2, // + kMixChannel2 (where its S is staged: 256 V2<T> of static LDS)
  kLevelGate2 = 4,    // flag: + kMixGate2
  kLevelFit = 8,      // flag: + the gradient of the general channels' rows (kMixChannelFit, kMixChannel2Fit): reverse sweeps only
};
__host__ __device__ constexpr int mixed_level_of(int kind) {
  return kind == kMixGate2 ? kLevelGate2 : kind == kMixChannel2 ? kLevelChannel2 : kind == kMixChannel ? kLevelChannel : kLevelLean;
}
__host__ __device__ constexpr int mixed_channels_of(int level) { return level & 3; }  // the channel level without the flag
__host__ __device__ constexpr bool mixed_has_gate2(int level) { return (level & kLevelGate2) != 0; }
__host__ __device__ constexpr bool mixed_has_fit(int level) { return (level & kLevelFit) != 0; }
// the lowest level that holds the ops of both
__host__ __device__ constexpr int mixed_level_join(int a, int b) {
  return (mixed_channels_of(a) > mixed_channels_of(b) ? mixed_channels_of(a) : mixed_channels_of(b)) | ((a | b) & (kLevelGate2 | kLevelFit));
}

struct MixedScalars {
  int32_t n, n_ops, measure, n_features;  // measure 0 probs, 1 <Z_w>, 2 the measurement table behind the n_ops ops, 8 the reduced density matrix
  int64_t batch, rows_ld, feat_ld, out_ld;
  double enc_offset, pad_with;
  int32_t slab_in_lds, n_obs;  // n_obs: terms of the measurement table, prog[n_ops .. n_ops + n_obs) (measure 2; measure 8: the one kMixRho op)
};

template <typename T>
__device__ __forceinline__ V2<T> cmul(V2<T> a, V2<T> b) {
  return V2<T>{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
template <typename T>
__device__ __forceinline__ V2<T> cmulc(V2<T> a, V2<T> b) {  // a * conj(b)
  return V2<T>{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y};
}

// index of the block element (bi, bj) for block number t: insert bits at positions qj (column half) and qi = qj + n
__device__ __forceinline__ uint32_t insert_two_bits(uint32_t t, int qlo, int qhi) {
  uint32_t lo = t & ((1u << qlo) - 1u);
  uint32_t rest = t >> qlo;
  uint32_t mid_bits = qhi - qlo - 1;
  uint32_t mid = rest & ((1u << mid_bits) - 1u);
  uint32_t hi = rest >> mid_bits;
  return lo | (mid << (qlo + 1)) | (hi << (qhi + 1));
}

// Where the 2 x 2 blocks of a wire sit: its bit in the column half (lo) and in the row half (hi) -- any bit numbering:
// the one-workgroup engine passes the global q, q + n, the tile-fused engine local ranks (MixedBlock2: the same for the
// 4 x 4 blocks of two wires).  Every walk over 2 x 2 blocks takes its indices from here.
struct MixedBlock1 {
  int lo, hi;
  __device__ __forceinline__ uint32_t base(uint32_t t) const { return insert_two_bits(t, lo, hi); }  // element (0, 0)
  __device__ __forceinline__ uint32_t cj() const { return 1u << lo; }                                // column bit
  __device__ __forceinline__ uint32_t ci() const { return 1u << hi; }                                // row bit
};
// Block number t of `mem`, owned by the thread: f(m00, m01, m10, m11) works on its four elements in registers and what
// it leaves goes back.  `snap` (may be NULL): the block as it was goes there too (as in mixed_block_super2).
template <typename T, typename F>
__device__ __forceinline__ void mixed_block_visit(V2<T>* mem, V2<T>* snap, uint32_t t, const MixedBlock1& b, F&& f) {
  const uint32_t base = b.base(t), cj = b.cj(), ci = b.ci();
  V2<T> m00 = mem[base], m01 = mem[base | cj], m10 = mem[base | ci], m11 = mem[base | ci | cj];
  if (snap) {
    snap[base] = m00;
    snap[base | cj] = m01;
    snap[base | ci] = m10;
    snap[base | ci | cj] = m11;
  }
  f(m00, m01, m10, m11);
  mem[base] = m00;
  mem[base | cj] = m01;
  mem[base | ci] = m10;
  mem[base | ci | cj] = m11;
}
// A thread's blocks among the n_blocks of a slab (run-time count: fewer blocks than threads below n = 5).  The
// tile-fused engine's count is a constant and its loops are unrolled: wide_walk_blocks in qsim_mixed_wide.h.
template <typename T, typename F>
__device__ __forceinline__ void mixed_walk_blocks(V2<T>* mem, V2<T>* snap, const MixedBlock1& b, uint32_t n_blocks, F&& f) {
  for (uint32_t t = threadIdx.x; t < n_blocks; t += 256) mixed_block_visit<T>(mem, snap, t, b, f);
}

__device__ __forceinline__ double mixed_angle(const MixedOp& op, const double* __restrict__ angle_rows,
                                              const MixedScalars& m, int64_t sample) {
  return op.p + (op.a >= 0 ? op.scale * angle_rows[(size_t)op.a * m.rows_ld + sample] : 0.0);
}

// the sum of every thread's v, in a fixed order, handed to every thread (s_red is free again on return)
__device__ __forceinline__ double mixed_block_sum(double v, double* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  const double total = s_red[0];
  __syncthreads();
  return total;
}

__device__ __forceinline__ double mixed_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool mixed_needs_snapshot(int kind, int oi) {
  return kind == kMixPhaseDamp || kind == kMixAmpDamp || kind == kMixDepol || kind == kMixChannel ||
         kind == kMixChannel2 || (oi > 0 && (kind == kMixZero || kind == kMixAmpEmbed));
}

// ---- per-element / per-block arithmetic, shared by both engines and both directions --------------------------------
template <typename T>
__device__ __forceinline__ void mixed_phase_factors(double phi, V2<T>& up, V2<T>& dn) {
  double sn, cs;
  sincos(phi, &sn, &cs);
  up = V2<T>{(T)cs, (T)sn};
  dn = V2<T>{(T)cs, (T)-sn};
}
// PHASE on bit q of the column half (q + n of the row half) of element k
template <typename T>
__device__ __forceinline__ V2<T> mixed_phase_elem(V2<T> v, uint32_t k, int q, int n, V2<T> up, V2<T> dn) {
  const int bi = (k >> (q + n)) & 1, bj = (k >> q) & 1;
  return bi != bj ? cmul<T>(v, bi ? up : dn) : v;
}
// whether CZ(bits q, qt) flips the sign of element k: sign(i) sign(j) = -1
__device__ __forceinline__ bool mixed_cz_flips(uint32_t k, int q, int qt, int n) {
  const uint32_t i = k >> n, j = k & ((1u << n) - 1u);
  const int si = ((i >> q) & (i >> qt) & 1), sj = ((j >> q) & (j >> qt) & 1);
  return si != sj;
}
template <typename T>
__device__ __forceinline__ V2<T> mixed_cz_elem(V2<T> v, uint32_t k, int q, int qt, int n) {
  return mixed_cz_flips(k, q, qt, n) ? V2<T>{-v.x, -v.y} : v;
}
// where CNOT(control bit q, target bit qt) sends element k (an involution)
__device__ __forceinline__ uint32_t mixed_cnot_index(uint32_t k, int q, int qt, int n) {
  const uint32_t i = k >> n, j = k & ((1u << n) - 1u);
  const uint32_t pi = i ^ (((i >> q) & 1u) << qt), pj = j ^ (((j >> q) & 1u) << qt);
  return (pi << n) | pj;
}

template <typename T>
struct MixedU {
  V2<T> u00, u01, u10, u11;
};
// the 2 x 2 unitary of an RY / GATE op, evaluated in float64 and rounded once
template <typename T>
__device__ __forceinline__ MixedU<T> mixed_unitary(const MixedOp& op, const double* __restrict__ angle_rows,
                                                   const double* __restrict__ gates, const MixedScalars& m,
                                                   int64_t sample) {
  using C = V2<T>;
  MixedU<T> u;
  if (op.kind == kMixRY) {
    const double th = mixed_angle(op, angle_rows, m, sample);
    double sn, cs;
    sincos(0.5 * th, &sn, &cs);
    u.u00 = C{(T)cs, 0};
    u.u01 = C{(T)-sn, 0};
    u.u10 = C{(T)sn, 0};
    u.u11 = C{(T)cs, 0};
  } else {
    const double* __restrict__ g = gates + (size_t)op.a * 8;
    u.u00 = C{(T)g[0], (T)g[1]};
    u.u01 = C{(T)g[2], (T)g[3]};
    u.u10 = C{(T)g[4], (T)g[5]};
    u.u11 = C{(T)g[6], (T)g[7]};
  }
  return u;
}
// M <- U M U^dagger on one block
template <typename T>
__device__ __forceinline__ void mixed_block_unitary(const MixedU<T>& u, V2<T>& m00, V2<T>& m01, V2<T>& m10, V2<T>& m11) {
  using C = V2<T>;
  // A = U M
  const C a00 = V2<T>{0, 0} + cmul<T>(u.u00, m00) + cmul<T>(u.u01, m10);
  const C a01 = cmul<T>(u.u00, m01) + cmul<T>(u.u01, m11);
  const C a10 = cmul<T>(u.u10, m00) + cmul<T>(u.u11, m10);
  const C a11 = cmul<T>(u.u10, m01) + cmul<T>(u.u11, m11);
  // M' = A U^dagger:  M'_{xy} = sum_k A_{xk} conj(U_{yk})
  m00 = cmulc<T>(a00, u.u00) + cmulc<T>(a01, u.u01);
  m01 = cmulc<T>(a00, u.u10) + cmulc<T>(a01, u.u11);
  m10 = cmulc<T>(a10, u.u00) + cmulc<T>(a11, u.u01);
  m11 = cmulc<T>(a10, u.u10) + cmulc<T>(a11, u.u11);
}

template <typename T>
struct MixedChannel {
  T off, d_own, d_other_to_0, d_other_to_1, d11;
};
// `p`: the strength of this sample, mixed_angle(op, ...) -- op.p, or with a >= 0 op.p + op.scale * angle_rows[a][sample]
template <typename T>
__device__ __forceinline__ MixedChannel<T> mixed_channel(int kind, double p) {
  MixedChannel<T> c;
  if (kind == kMixPhaseDamp) {
    c.off = (T)sqrt(1.0 - p); c.d_own = 1; c.d11 = 1; c.d_other_to_0 = 0; c.d_other_to_1 = 0;
  } else if (kind == kMixAmpDamp) {
    c.off = (T)sqrt(1.0 - p); c.d_own = 1; c.d11 = (T)(1.0 - p); c.d_other_to_0 = (T)p; c.d_other_to_1 = 0;
  } else {
    c.off = (T)(1.0 - 4.0 * p / 3.0); c.d_own = (T)(1.0 - 2.0 * p / 3.0); c.d11 = c.d_own;
    c.d_other_to_0 = (T)(2.0 * p / 3.0); c.d_other_to_1 = c.d_other_to_0;
  }
  return c;
}
// ---- dL/dstrength of a native channel with a >= 0 (the reverse sweeps) -------------------------------------------------
// With Lambda the adjoint behind the channel and rho the state in front of it, dL/dstrength = <Lambda, E'(rho)> =
// sum over the wire's blocks of Re sum_xy conj(L_xy) E'(M)_xy, and E'(M) is
//     PhaseDamping(g):      M01, M10 -> o M01, o M10,  o = -1 / (2 sqrt(1-g));  M00, M11 -> 0
//     AmplitudeDamping(g):  M00 -> +M11, M11 -> -M11;  off-diagonals as PhaseDamping (not finite at g = 1, as PennyLane's)
//     Depolarizing(p):      M00 -> (2/3)(M11 - M00), M11 -> (2/3)(M00 - M11);  M01, M10 -> -(4/3) M01, -(4/3) M10
// The products are taken in double whatever T is: one sum per (op, sample) feeds the gradient.
__device__ __forceinline__ double mixed_channel_doff(int kind, double p) {  // d(off-diagonal factor)/dstrength
  return kind == kMixDepol ? -4.0 / 3.0 : -0.5 / sqrt(1.0 - p);
}
template <typename T>
__device__ __forceinline__ double mixed_re_dot(V2<T> l, V2<T> r) {  // Re(conj(l) r)
  return (double)l.x * (double)r.x + (double)l.y * (double)r.y;
}
// the off-diagonal elements' share, still to be multiplied by mixed_channel_doff
template <typename T>
__device__ __forceinline__ double mixed_strength_grad_off(V2<T> r01, V2<T> r10, V2<T> l01, V2<T> l10) {
  return mixed_re_dot<T>(l01, r01) + mixed_re_dot<T>(l10, r10);
}
// the diagonal elements' share (AmplitudeDamping, Depolarizing; PhaseDamping has none)
template <typename T>
__device__ __forceinline__ double mixed_strength_grad_diag(int kind, V2<T> r00, V2<T> r11, V2<T> l00, V2<T> l11) {
  const double lx = (double)l00.x - (double)l11.x, ly = (double)l00.y - (double)l11.y;
  if (kind == kMixAmpDamp) return lx * (double)r11.x + ly * (double)r11.y;
  if (kind == kMixDepol)
    return (2.0 / 3.0) * (lx * ((double)r11.x - (double)r00.x) + ly * ((double)r11.y - (double)r00.y));
  return 0.0;
}
template <typename T>
__device__ __forceinline__ void mixed_block_channel(const MixedChannel<T>& c, V2<T>& m00, V2<T>& m01, V2<T>& m10, V2<T>& m11) {
  using C = V2<T>;
  const C n00 = C{c.d_own * m00.x + c.d_other_to_0 * m11.x, c.d_own * m00.y + c.d_other_to_0 * m11.y};
  const C n11 = C{c.d11 * m11.x + c.d_other_to_1 * m00.x, c.d11 * m11.y + c.d_other_to_1 * m00.y};
  m00 = n00;
  m11 = n11;
  m01 = C{c.off * m01.x, c.off * m01.y};
  m10 = C{c.off * m10.x, c.off * m10.y};
}
// E^dagger on one block (the reverse sweeps): the transpose of E's 2 x 2 mixing of the diagonal; off-diagonals scale alike
template <typename T>
__device__ __forceinline__ void mixed_block_channel_adjoint(const MixedChannel<T>& c, V2<T>& m00, V2<T>& m01, V2<T>& m10,
                                                            V2<T>& m11) {
  using C = V2<T>;
  const C n00 = C{c.d_own * m00.x + c.d_other_to_1 * m11.x, c.d_own * m00.y + c.d_other_to_1 * m11.y};
  const C n11 = C{c.d11 * m11.x + c.d_other_to_0 * m00.x, c.d11 * m11.y + c.d_other_to_0 * m00.y};
  m00 = n00;
  m11 = n11;
  m01 = C{c.off * m01.x, c.off * m01.y};
  m10 = C{c.off * m10.x, c.off * m10.y};
}

// The general one-wire channel: S (4 x 4 complex, row-major in gates[a .. a+3]) on vec(M) = (M00, M01, M10, M11).
// The coefficients are the same for every thread of the workgroup: mixed_uniform pins each one to scalar registers, so
// the 16 complex numbers cost no vector registers in the block loops.  Its case still costs the kernels that carry it
// vector registers (a resident wave per SIMD in mixed_kernel, mixed_wide_sweep<float> and mixed_wide_adjoint_channels),
// so those kernels have an instantiation per MixedLevel; the host launches the lowest level that holds the ops of the
// program (tile-fused engine: of the segment).
__device__ __forceinline__ float mixed_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ double mixed_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
template <typename T>
struct MixedSuper {
  V2<T> s[4][4];
};
// evaluated like mixed_unitary: read in float64 and rounded once
template <typename T>
__device__ __forceinline__ MixedSuper<T> mixed_super(const MixedOp& op, const double* __restrict__ gates) {
  const double* __restrict__ g = gates + (size_t)op.a * 8;
  MixedSuper<T> su;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      su.s[r][c] = V2<T>{mixed_uniform((T)g[(r * 4 + c) * 2]), mixed_uniform((T)g[(r * 4 + c) * 2 + 1])};
  return su;
}
// vec(M) <- S vec(M) on one block
template <typename T>
__device__ __forceinline__ void mixed_block_super(const MixedSuper<T>& su, V2<T>& m00, V2<T>& m01, V2<T>& m10, V2<T>& m11) {
  const V2<T> v[4] = {m00, m01, m10, m11};
  V2<T> o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    o[r] = cmul<T>(su.s[r][0], v[0]) + cmul<T>(su.s[r][1], v[1]) + cmul<T>(su.s[r][2], v[2]) + cmul<T>(su.s[r][3], v[3]);
  m00 = o[0];
  m01 = o[1];
  m10 = o[2];
  m11 = o[3];
}
// E^dagger of the general channel for the pairing Tr(Lambda^dagger rho) of the reverse sweeps: vec(M) <- S^H vec(M)
template <typename T>
__device__ __forceinline__ void mixed_block_super_adjoint(const MixedSuper<T>& su, V2<T>& m00, V2<T>& m01, V2<T>& m10,
                                                          V2<T>& m11) {
  const V2<T> v[4] = {m00, m01, m10, m11};
  V2<T> o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    o[c] = cmulc<T>(v[0], su.s[0][c]) + cmulc<T>(v[1], su.s[1][c]) + cmulc<T>(v[2], su.s[2][c]) + cmulc<T>(v[3], su.s[3][c]);
  m00 = o[0];
  m01 = o[1];
  m10 = o[2];
  m11 = o[3];
}
// ---- the general two-wire channel ------------------------------------------------------------------------------------
// S (16 x 16 complex, row-major in gates[a .. a+63]: 256 consecutive (re, im) pairs) is the same for every thread, but
// 256 complex numbers do not fit scalar registers the way the one-wire op's 16 do.  Two ways to read it:
//   uniform  every coefficient is a uniform load from `gates` (the compiler makes scalar loads of them), converted from
//            float64 where it is used: no LDS, no barrier, no vector register for S.
//   staged   the workgroup copies S once per op to LDS, rounded once to T (2 KiB in float32, 4 KiB in float64); every
//            read in the block loops is a broadcast (all lanes one address).
// Measured on whole programs (profiles/mixed_channel2/op_cost.json): uniform is 7-17 % faster in the forward
// of both engines and 4-6 % in the one-workgroup backward, staged 5-8 % faster in the tile-fused backward only; a mix
// by direction was slower than either there.  Uniform is what is built, in both directions.
template <typename T>
struct MixedSuper2 {
  const double* __restrict__ g;  // S in `gates`
  __device__ __forceinline__ V2<T> at(int i) const { return V2<T>{(T)g[2 * i], (T)g[2 * i + 1]}; }
};
template <typename T>
__device__ __forceinline__ MixedSuper2<T> mixed_super2(const MixedOp& op, const double* __restrict__ gates) {
  return MixedSuper2<T>{gates + (size_t)op.a * 8};
}
// where the 4 x 4 block's rows and columns sit: the bits of the first and second wire in the row half (r1, r2) and in
// the column half (c1, c2) -- any bit numbering: global or tile-local -- and the four positions in ascending order
struct MixedBlock2 {
  int r1, r2, c1, c2;
  int pos[4];  // the block number's bits go around these
  // element e = 4 r + c of the block (r = 2 b_w1 + b_w2 from the row bits, c from the column bits) relative to its base
  __device__ __forceinline__ uint32_t elem(int e) const {
    return (((uint32_t)e >> 3 & 1u) << r1) | (((uint32_t)e >> 2 & 1u) << r2) | (((uint32_t)e >> 1 & 1u) << c1) |
           (((uint32_t)e & 1u) << c2);
  }
};
__device__ __forceinline__ MixedBlock2 mixed_block2(int c1, int c2, int r1, int r2) {
  MixedBlock2 b;
  b.r1 = r1; b.r2 = r2; b.c1 = c1; b.c2 = c2;
  // both numberings keep every column bit below every row bit and the order of the wires the same in both halves
  b.pos[0] = c1 < c2 ? c1 : c2;
  b.pos[1] = c1 < c2 ? c2 : c1;
  b.pos[2] = r1 < r2 ? r1 : r2;
  b.pos[3] = r1 < r2 ? r2 : r1;
  return b;
}
// block number t -> the index of its (0, 0) element: zero bits inserted at the four positions
__device__ __forceinline__ uint32_t mixed_block2_base(uint32_t t, const MixedBlock2& b) {
#pragma unroll
  for (int i = 0; i < 4; ++i) t = (t & ((1u << b.pos[i]) - 1u)) | ((t >> b.pos[i]) << (b.pos[i] + 1));
  return t;
}
// vec(M) <- S vec(M) (ADJOINT: S^H vec(M), out[c] = sum_r conj(S[r][c]) v[r]) on the block at `base` of `mem`, in place:
// all 16 elements are read before the first is written, and the thread owns the block.  `snap`: the block as it was
// goes there too.  The 16-term sums run in a fixed order.  The loop over the outputs stays rolled: unrolled, the
// compiler fetches all 256 coefficients ahead of the arithmetic and spills (2.8 KB of scratch a lane in mixed_kernel).
template <typename T, bool ADJOINT>
__device__ __forceinline__ void mixed_block_super2(const MixedSuper2<T>& su, V2<T>* __restrict__ mem, V2<T>* __restrict__ snap,
                                                   uint32_t base, const MixedBlock2& b) {
  V2<T> v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = mem[base | b.elem(e)];
  if (snap) {
#pragma unroll
    for (int e = 0; e < 16; ++e) snap[base | b.elem(e)] = v[e];
  }
#pragma unroll 1
  for (int o = 0; o < 16; ++o) {
    V2<T> acc = ADJOINT ? cmulc<T>(v[0], su.at(o)) : cmul<T>(su.at(o * 16), v[0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) acc = acc + (ADJOINT ? cmulc<T>(v[e], su.at(e * 16 + o)) : cmul<T>(su.at(o * 16 + e), v[e]));
    mem[base | b.elem(o)] = acc;
  }
}

// ---- the two-wire unitary ---------------------------------------------------------------------------------------------
// U (4 x 4 complex, row-major in gates[a .. a+3], operator index 2 b_w1 + b_w2) is read like mixed_super's S: in float64,
// rounded once to T, every coefficient pinned to scalar registers -- 16 complex numbers, as many as the one-wire
// channel's.  The block geometry is the two-wire channel's (MixedBlock2).
template <typename T>
struct MixedU2 {
  V2<T> u[4][4];
};
template <typename T>
__device__ __forceinline__ MixedU2<T> mixed_unitary2(const MixedOp& op, const double* __restrict__ gates) {
  const double* __restrict__ g = gates + (size_t)op.a * 8;
  MixedU2<T> u;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      u.u[r][c] = V2<T>{mixed_uniform((T)g[(r * 4 + c) * 2]), mixed_uniform((T)g[(r * 4 + c) * 2 + 1])};
  return u;
}
// M <- U M U^dagger (ADJOINT: U^dagger M U) on the 4 x 4 block v[4 r + c] in registers, written to the block at `base`
// of `mem`: one output row at a time -- the row of U M (four temporaries), then the row of (U M) U^dagger, stored.  The
// caller has loaded all 16 elements, so the block may be the one `v` came from.  Four-term sums in a fixed order.
template <typename T, bool ADJOINT>
__device__ __forceinline__ void mixed_block_gate2_store(const MixedU2<T>& u, const V2<T> (&v)[16], V2<T>* __restrict__ mem,
                                                        uint32_t base, const MixedBlock2& b) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    V2<T> t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      t[c] = ADJOINT ? cmulc<T>(v[c], u.u[0][r]) + cmulc<T>(v[4 + c], u.u[1][r]) + cmulc<T>(v[8 + c], u.u[2][r]) +
                           cmulc<T>(v[12 + c], u.u[3][r])
                     : cmul<T>(u.u[r][0], v[c]) + cmul<T>(u.u[r][1], v[4 + c]) + cmul<T>(u.u[r][2], v[8 + c]) +
                           cmul<T>(u.u[r][3], v[12 + c]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      mem[base | b.elem(4 * r + c)] =
          ADJOINT ? cmul<T>(t[0], u.u[0][c]) + cmul<T>(t[1], u.u[1][c]) + cmul<T>(t[2], u.u[2][c]) + cmul<T>(t[3], u.u[3][c])
                  : cmulc<T>(t[0], u.u[c][0]) + cmulc<T>(t[1], u.u[c][1]) + cmulc<T>(t[2], u.u[c][2]) + cmulc<T>(t[3], u.u[c][3]);
  }
}
// the same on the block at `base` of `mem`, in place (the thread owns the block)
template <typename T, bool ADJOINT>
__device__ __forceinline__ void mixed_block_gate2(const MixedU2<T>& u, V2<T>* __restrict__ mem, uint32_t base,
                                                  const MixedBlock2& b) {
  V2<T> v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = mem[base | b.elem(e)];
  mixed_block_gate2_store<T, ADJOINT>(u, v, mem, base, b);
}
// One 4 x 4 block of the reverse sweeps: acc += B_rho B_Lambda^dagger (N_ab = sum_c rho_ac conj(Lambda_bc), (re, im) of
// N[a][b] at acc[2 (4 a + b)]), both blocks taken behind the gate, then rho and Lambda <- U^dagger B U in place.  Lambda
// is read a row at a time beside the 16 elements of rho: the 32 sums are what fills the registers.
template <typename T>
__device__ __forceinline__ void mixed_block_gate2_reverse(const MixedU2<T>& u, double (&acc)[32], V2<T>* __restrict__ rho,
                                                          V2<T>* __restrict__ lam, uint32_t base, const MixedBlock2& b) {
  V2<T> r[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) r[e] = rho[base | b.elem(e)];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    V2<T> l[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) l[c] = lam[base | b.elem(4 * bb + c)];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const V2<T> nab = cmulc<T>(r[4 * a], l[0]) + cmulc<T>(r[4 * a + 1], l[1]) + cmulc<T>(r[4 * a + 2], l[2]) +
                        cmulc<T>(r[4 * a + 3], l[3]);
      acc[2 * (4 * a + bb)] += (double)nab.x;
      acc[2 * (4 * a + bb) + 1] += (double)nab.y;
    }
  }
  mixed_block_gate2_store<T, true>(u, r, rho, base, b);
  mixed_block_gate2<T, true>(u, lam, base, b);
}
// GATE2: go += dL/dU from the reduced N `s` and the gate `gu` (both as (re, im) of the 16 entries, row-major): the 4 x 4
// form of mixed_gate_grad_accumulate below
__device__ __forceinline__ void mixed_gate2_grad_accumulate(const double* s, const double* __restrict__ gu, double* go) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double ur = gu[(c * 4 + bb) * 2], ui = gu[(c * 4 + bb) * 2 + 1];
        const double nr = s[(c * 4 + a) * 2], ni = s[(c * 4 + a) * 2 + 1];
        re += ur * nr + ui * ni;
        im += ur * ni - ui * nr;
      }
      go[(a * 4 + bb) * 2] += 2.0 * re;
      go[(a * 4 + bb) * 2 + 1] += -2.0 * im;
    }
}

// ---- dL/dS of a general channel whose rows get a gradient (kMixChannelFit, kMixChannel2Fit; the reverse sweeps) ----------
// With Lambda' the adjoint behind the channel and M the block of rho in front of it, dL = Re sum conj(Lambda') d rho' and
// vec(M') = S vec(M) give W[r][c] = sum over blocks of conj(vec(Lambda')[r]) vec(M)[c], dL/dRe S[r][c] = Re W[r][c] and
// dL/dIm S[r][c] = -Im W[r][c].  The products are taken in double whatever T is.
// One wire: acc += (re, im) of the 16 W[r][c] of one block, at acc[2 (4 r + c)]
template <typename T>
__device__ __forceinline__ void mixed_super_grad_accumulate(double (&acc)[32], const V2<T> (&l)[4], const V2<T> (&r)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[2 * (4 * a + c)] += (double)l[a].x * (double)r[c].x + (double)l[a].y * (double)r[c].y;
      acc[2 * (4 * a + c) + 1] += (double)l[a].x * (double)r[c].y - (double)l[a].y * (double)r[c].x;
    }
}
// Two wires: 256 entries do not fit a thread's registers as sums, so thread t = 16 r + c owns W[r][c] and walks all
// `n_blocks` blocks in index order -- no reduction across threads, the order is fixed by construction.  `lam` is read
// before any thread applies S^H to it: the caller puts a barrier behind this.
template <typename T>
__device__ __forceinline__ void mixed_super2_grad(const V2<T>* __restrict__ lam, const V2<T>* __restrict__ rho,
                                                  uint32_t n_blocks, const MixedBlock2& b, double& re, double& im) {
  const uint32_t er = b.elem((int)(threadIdx.x >> 4)), ec = b.elem((int)(threadIdx.x & 15u));
  re = 0.0;
  im = 0.0;
#pragma unroll 16
  for (uint32_t t = 0; t < n_blocks; ++t) {
    const uint32_t base = mixed_block2_base(t, b);
    const V2<T> l = lam[base | er], r = rho[base | ec];
    re += (double)l.x * (double)r.x + (double)l.y * (double)r.y;
    im += (double)l.x * (double)r.y - (double)l.y * (double)r.x;
  }
}
// what the constant kinds do to rho and Lambda is what the trainable ones do: FIT instantiations take 18 for 16, 34 for 32
template <bool FIT>
__device__ __forceinline__ MixedOp mixed_constant_kind(MixedOp op) {
  if constexpr (FIT) {
    if (op.kind == kMixChannelFit || op.kind == kMixChannel2Fit) op.kind -= 2;
  }
  return op;
}

// acc += B_rho B_Lambda^dagger of one block: N_ab = sum_c rho_ac conj(Lambda_bc), (re, im) of N00, N01, N10, N11
template <typename T>
__device__ __forceinline__ void mixed_block_n_accumulate(double (&acc)[8], V2<T> r00, V2<T> r01, V2<T> r10, V2<T> r11,
                                                         V2<T> l00, V2<T> l01, V2<T> l10, V2<T> l11) {
  using C = V2<T>;
  const C n00 = cmulc<T>(r00, l00) + cmulc<T>(r01, l01), n01 = cmulc<T>(r00, l10) + cmulc<T>(r01, l11);
  const C n10 = cmulc<T>(r10, l00) + cmulc<T>(r11, l01), n11 = cmulc<T>(r10, l10) + cmulc<T>(r11, l11);
  acc[0] += (double)n00.x; acc[1] += (double)n00.y;
  acc[2] += (double)n01.x; acc[3] += (double)n01.y;
  acc[4] += (double)n10.x; acc[5] += (double)n10.y;
  acc[6] += (double)n11.x; acc[7] += (double)n11.y;
}
// GATE: go += dL/dU from the reduced N `s` and the gate `gu` (both as (re, im) of the 00, 01, 10, 11 entries):
// R_ba = sum_c conj(U_cb) N_ca;  dL/dRe U_ab = 2 Re R_ba, dL/dIm U_ab = -2 Im R_ba
__device__ __forceinline__ void mixed_gate_grad_accumulate(const double* s, const double* __restrict__ gu, double* go) {
  for (int a = 0; a < 2; ++a)
    for (int bb = 0; bb < 2; ++bb) {
      double re = 0.0, im = 0.0;
      for (int c = 0; c < 2; ++c) {
        const double ur = gu[(c * 2 + bb) * 2], ui = gu[(c * 2 + bb) * 2 + 1];
        const double nr = s[(c * 2 + a) * 2], ni = s[(c * 2 + a) * 2 + 1];
        re += ur * nr + ui * ni;
        im += ur * ni - ui * nr;
      }
      go[(a * 2 + bb) * 2] += 2.0 * re;
      go[(a * 2 + bb) * 2 + 1] += -2.0 * im;
    }
}
// an off-diagonal element of a wire's blocks under PhaseDamping (the diagonal ones stay)
template <typename T>
__device__ __forceinline__ V2<T> mixed_phase_damp_elem(V2<T> v, uint32_t k, int q, int n, T off) {
  const int bi = (k >> (q + n)) & 1, bj = (k >> q) & 1;
  return bi != bj ? V2<T>{off * v.x, off * v.y} : v;
}

// |v|^2 of a sample's padded feature row, summed in a fixed order and handed to every thread
__device__ __forceinline__ double mixed_embed_norm2(const double* __restrict__ row, double* s_red, const MixedScalars& m) {
  const int tid = threadIdx.x;
  const uint32_t D = 1u << m.n;
  double part = 0.0;
  for (uint32_t k = tid; k < D; k += 256) {
    const double v = k < (uint32_t)m.n_features ? row[k] + m.enc_offset : m.pad_with;
    part += v * v;
  }
  return mixed_block_sum(part, s_red);
}
// element k of v v^T / |v|^2
template <typename T>
__device__ __forceinline__ V2<T> mixed_embed_elem(const double* __restrict__ row, uint32_t k, double inv, const MixedScalars& m) {
  const uint32_t i = k >> m.n, j = k & ((1u << m.n) - 1u);
  const double vi = i < (uint32_t)m.n_features ? row[i] + m.enc_offset : m.pad_with;
  const double vj = j < (uint32_t)m.n_features ? row[j] + m.enc_offset : m.pad_with;
  return V2<T>{(T)(vi * vj * inv), (T)0};
}
// element k of Lambda_N = dL/drho_N, the seed of a reverse sweep: diag(g) for probs, sum_w g_w (1 - 2 bit_w) for <Z>
template <typename T>
__device__ __forceinline__ V2<T> mixed_seed_elem(const double* __restrict__ g, uint32_t k, const MixedScalars& m) {
  const int n = m.n;
  const uint32_t i = k >> n, j = k & ((1u << n) - 1u);
  double v = 0.0;
  if (i == j) {
    if (m.measure == 0) {
      v = g[i];
    } else {
      for (int w = 0; w < n; ++w) v += ((i >> (n - 1 - w)) & 1u) ? -g[w] : g[w];
    }
  }
  return V2<T>{(T)v, (T)0};
}

// the diagonal of one sample's rho -> probs / <Z_w>, float64, fixed-order sums
template <typename T>
__device__ __forceinline__ void mixed_read_out(const V2<T>* __restrict__ rho, double* __restrict__ out, double* s_red,
                                               const MixedScalars& m, int64_t sample) {
  const int n = m.n, tid = threadIdx.x;
  const uint32_t D = 1u << n;
  if (m.measure == 0) {
    for (uint32_t k = tid; k < D; k += 256) out[sample * m.out_ld + k] = (double)rho[((size_t)k << n) | k].x;
  } else {
    for (int w = 0; w < n; ++w) {
      double part = 0.0;
      for (uint32_t k = tid; k < D; k += 256) {
        const double pk = (double)rho[((size_t)k << n) | k].x;
        part += ((k >> (n - 1 - w)) & 1u) ? -pk : pk;
      }
      const double total = mixed_block_sum(part, s_red);
      if (tid == 0) out[sample * m.out_ld + w] = total;
    }
  }
}

// ---- the measurement table (measure 2): Pauli-word expectation values ---------------------------------------------------
// The program's tail is a table of kMixObs terms, each coefficient p times a Pauli word: x-mask `wire` (wires carrying X
// or Y), z-mask `a` (Z or Y), wire w at bit n-1-w; wire2 is the output column and several terms may share one (a
// Hamiltonian).  With ny = popcount(x & z) the word is P[i][j] = i^ny (-1)^popcount(j & z) where i ^ j = x, so
//     Tr(rho P) = Re( i^ny sum_k (-1)^popcount(k & z) rho[k][k ^ x] )
// (rho and P are Hermitian).  The table is the same for every thread: a term's fields are read at an index that is
// uniform over the wave (scalar loads); the seed keeps the per-sample weights of the terms in LDS.
__device__ __forceinline__ int mixed_obs_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// |Re(i^ny v)|'s component of v: Re(i^ny (re + i im)) is re, -im, -re, im for ny = 0, 1, 2, 3 (the caller has the sign)
template <typename T>
__device__ __forceinline__ double mixed_obs_part(V2<T> v, int ny) {
  return (ny & 1) ? (double)v.y : (double)v.x;
}
// One sample's rho -> out_row[column] = sum over the column's terms of p Tr(rho P), float64.  A wave owns every fourth
// term: its lanes stride the 2^n elements rho[k][k ^ x], the wave sums them in a fixed order, and the thread of a
// column's first term adds that column's terms in table order.  s_term: 256 doubles.  Ends in a barrier.
template <typename T>
__device__ __forceinline__ void mixed_obs_read_out(const V2<T>* __restrict__ rho, double* __restrict__ out_row,
                                                   double* s_term, const MixedOp* __restrict__ terms, int n_terms, int n) {
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t D = 1u << n;
  for (int t = mixed_obs_wave(); t < n_terms; t += 4) {
    const uint32_t x = (uint32_t)terms[t].wire, z = (uint32_t)terms[t].a;
    const int ny = __popc(x & z) & 3;
    const bool flip = ny == 1 || ny == 2;
    double part = 0.0;
    for (uint32_t k = lane; k < D; k += 64) {
      const double c = mixed_obs_part<T>(rho[((size_t)k << n) | (k ^ x)], ny);
      part += (((__popc(k & z) & 1) != 0) != flip) ? -c : c;
    }
    const double total = mixed_wave_sum(part);
    if (lane == 0) s_term[t] = terms[t].p * total;
  }
  __syncthreads();
  if (tid < n_terms) {
    const int col = terms[tid].wire2;
    if (tid == 0 || terms[tid - 1].wire2 != col) {
      double s = 0.0;
      for (int u = tid; u < n_terms && terms[u].wire2 == col; ++u) s += s_term[u];
      out_row[col] = s;
    }
  }
  __syncthreads();
}
// the weights of the seed, one per term: s_w[t] = g[column_t] p_t (g: this sample's row of grad_out).  The caller puts a
// barrier behind it.
__device__ __forceinline__ void mixed_obs_seed_weights(double* s_w, const double* __restrict__ g,
                                                       const MixedOp* __restrict__ terms, int n_terms) {
  for (int t = threadIdx.x; t < n_terms; t += 256) s_w[t] = g[terms[t].wire2] * terms[t].p;
}
// Element k = (i << n) | j of Lambda_N = sum_t g[column_t] p_t P_t, the seed of a reverse sweep under measure 2: the terms
// with x_t = i ^ j, in table order.  Hermitian; not real when a word holds Y, not diagonal when it holds X or Y.  The
// sweeps pair Lambda with rho as Re sum conj(Lambda_ij) rho_ij, so Lambda itself (not its transpose) is what they take:
// d/drho_ij of Re(i^ny s rho[k][k ^ x]) is conj(i^ny) s at (i, j) = (k, k ^ x), which is P[i][j] by Hermiticity.
template <typename T>
__device__ __forceinline__ V2<T> mixed_obs_seed_elem(const MixedOp* __restrict__ terms, int n_terms, const double* s_w,
                                                     uint32_t k, int n) {
  const uint32_t i = k >> n, j = k & ((1u << n) - 1u), x = i ^ j;
  double re = 0.0, im = 0.0;
  for (int t = 0; t < n_terms; ++t) {
    const uint32_t xt = (uint32_t)terms[t].wire, zt = (uint32_t)terms[t].a;  // uniform: scalar loads
    if (xt == x) {
      const int ny = __popc(xt & zt) & 3;
      const double w = (__popc(j & zt) & 1) ? -s_w[t] : s_w[t];
      if (ny == 0) re += w;
      else if (ny == 1) im += w;
      else if (ny == 2) re -= w;
      else im -= w;
    }
  }
  return V2<T>{(T)re, (T)im};
}

// ---- the reduced density matrix (measure 8): partial trace over the wires outside a keep-mask ------------------------------
// The program's last op is kMixRho; its `wire` is the keep-mask (wire w at bit n-1-w, k = popcount(mask) wires, K = 2^k).
// r and c number the kept wires' bit strings, the lowest wire most significant (the order of probs); e numbers the
// 2^(n-k) strings of the traced-out wires.  dep(r, e) puts r's bits at the mask's positions and e's at the others:
//     rho_A[r][c] = sum_e rho[dep(r, e)][dep(c, e)]        out_row[2 (r K + c)] = Re, out_row[2 (r K + c) + 1] = Im
// float64 sums in a fixed order whatever T is; k = n is rho itself, converted.
// the low bits of v, in order, to the set positions of `mask` (n <= 10 positions; the mask is uniform over the launch)
__device__ __forceinline__ uint32_t mixed_deposit(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
#pragma unroll
  for (int b = 0; b < 10; ++b)
    if (mask >> b & 1u) {
      out |= (v & 1u) << b;
      v >>= 1;
    }
  return out;
}
// its inverse: the bits of v at the set positions of `mask`, packed
__device__ __forceinline__ uint32_t mixed_extract(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
  int at = 0;
#pragma unroll
  for (int b = 0; b < 10; ++b)
    if (mask >> b & 1u) {
      out |= (v >> b & 1u) << at;
      ++at;
    }
  return out;
}
// One sample's rho -> its reduced matrix in out_row.  `part` of `n_parts` workgroups of 256 threads share the K^2 output
// elements (the one-workgroup engine: 0 of 1).  With 64 or more traced values a wave owns an element: its lanes stride
// e, mixed_wave_sum adds the 64 partials in a fixed order, waves stride the elements.  Below that a thread owns an
// element and adds its <= 32 terms in ascending e.  No LDS, no barrier; every element is written once, by one thread.
template <typename T>
__device__ __forceinline__ void mixed_rho_read_out(const V2<T>* __restrict__ rho, double* __restrict__ out_row,
                                                   uint32_t mask, int n, uint32_t part, uint32_t n_parts) {
  const uint32_t D = 1u << n, rest = (D - 1u) & ~mask;
  const int k = __popc(mask);
  const uint32_t K = 1u << k, KK = 1u << (2 * k), E = 1u << (n - k);
  if (E >= 64u) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t idx = part * 4u + (uint32_t)mixed_obs_wave(); idx < KK; idx += 4u * n_parts) {
      const uint32_t row = mixed_deposit(idx >> k, mask), col = mixed_deposit(idx & (K - 1u), mask);
      double re = 0.0, im = 0.0;
      for (uint32_t e = lane; e < E; e += 64u) {
        const uint32_t t = mixed_deposit(e, rest);
        const V2<T> v = rho[((size_t)(row | t) << n) | (col | t)];
        re += (double)v.x;
        im += (double)v.y;
      }
      re = mixed_wave_sum(re);
      im = mixed_wave_sum(im);
      if (lane == 0) {  // (two 8-byte stores: a row of `out` is 8-byte aligned, no more, when out_ld is odd)
        out_row[2 * (size_t)idx] = re;
        out_row[2 * (size_t)idx + 1] = im;
      }
    }
  } else {
    for (uint32_t idx = part * 256u + threadIdx.x; idx < KK; idx += 256u * n_parts) {
      const uint32_t row = mixed_deposit(idx >> k, mask), col = mixed_deposit(idx & (K - 1u), mask);
      double re = 0.0, im = 0.0;
      for (uint32_t e = 0; e < E; ++e) {
        const uint32_t t = mixed_deposit(e, rest);
        const V2<T> v = rho[((size_t)(row | t) << n) | (col | t)];
        re += (double)v.x;
        im += (double)v.y;
      }
      out_row[2 * (size_t)idx] = re;
      out_row[2 * (size_t)idx + 1] = im;
    }
  }
}
// Element k = (i << n) | j of Lambda_N, the seed of a reverse sweep under measure 8 (g: this sample's row of grad_out, laid
// out like out_row).  L = sum g_re[r][c] Re rho_A[r][c] + g_im[r][c] Im rho_A[r][c] pairs with rho as Re sum conj(G_ij)
// rho_ij for G_ij = g_re[r][c] + i g_im[r][c] where i and j agree outside the mask (r, c: their kept bits) and 0
// elsewhere.  G need not be Hermitian; the sweeps have only ever met Hermitian matrices, and the anti-Hermitian part of G
// pairs to zero with every Hermitian rho, so the seed is G's Hermitian part (G + G^dagger) / 2.
template <typename T>
__device__ __forceinline__ V2<T> mixed_rho_seed_elem(const double* __restrict__ g, uint32_t k, uint32_t mask, int n) {
  const uint32_t i = k >> n, j = k & ((1u << n) - 1u);
  if ((i ^ j) & ~mask) return V2<T>{(T)0, (T)0};
  const int kk = __popc(mask);
  const uint32_t r = mixed_extract(i, mask), c = mixed_extract(j, mask);
  const double* __restrict__ a = g + 2 * (((size_t)r << kk) | c);
  const double* __restrict__ b = g + 2 * (((size_t)c << kk) | r);
  return V2<T>{(T)(0.5 * (a[0] + b[0])), (T)(0.5 * (a[1] - b[1]))};
}

// Op `op` of the program on one sample's rho.  `snap` (NULL in the forward): where the backward's replay keeps rho as
// it was before a channel or a state preparation.  The caller puts a barrier after every op.
template <typename T, int LEVEL>
__device__ __forceinline__ void mixed_apply_op(const MixedOp& op, V2<T>* __restrict__ rho, V2<T>* __restrict__ snap,
                                               const double* __restrict__ angle_rows, const double* __restrict__ feats,
                                               const double* __restrict__ gates, double* s_red, const MixedScalars& m,
                                               int64_t sample) {
  using C = V2<T>;
  const int n = m.n, tid = threadIdx.x;
  const uint32_t D = 1u << n, DD = 1u << (2 * n);
  const int q = n - 1 - op.wire;  // bit of the column half; the row half's is q + n
  const MixedBlock1 blk{q, q + n};
  if (snap && (op.kind == kMixZero || op.kind == kMixAmpEmbed))
    for (uint32_t k = tid; k < DD; k += 256) snap[k] = rho[k];  // the same thread then overwrites rho[k]
  switch (op.kind) {
    case kMixZero: {
      for (uint32_t k = tid; k < DD; k += 256) rho[k] = C{k == 0 ? (T)1 : (T)0, (T)0};
      break;
    }
    case kMixAmpEmbed: {
      const double* __restrict__ row = feats + sample * m.feat_ld;
      const double inv = 1.0 / mixed_embed_norm2(row, s_red, m);
      for (uint32_t k = tid; k < DD; k += 256) rho[k] = mixed_embed_elem<T>(row, k, inv, m);
      break;
    }
    case kMixPhase: {
      C up, dn;
      mixed_phase_factors<T>(mixed_angle(op, angle_rows, m, sample), up, dn);
      for (uint32_t k = tid; k < DD; k += 256) {
        const int bi = (k >> (q + n)) & 1, bj = (k >> q) & 1;
        if (bi != bj) rho[k] = cmul<T>(rho[k], bi ? up : dn);
      }
      break;
    }
    case kMixRY:
    case kMixGate: {
      const MixedU<T> u = mixed_unitary<T>(op, angle_rows, gates, m, sample);
      mixed_walk_blocks<T>(rho, nullptr, blk, DD / 4,
                           [&](C& m00, C& m01, C& m10, C& m11) { mixed_block_unitary<T>(u, m00, m01, m10, m11); });
      break;
    }
    case kMixCZ: {
      const int qt = n - 1 - op.a;
      for (uint32_t k = tid; k < DD; k += 256)
        if (mixed_cz_flips(k, q, qt, n)) rho[k] = C{-rho[k].x, -rho[k].y};  // only the elements that change are stored
      break;
    }
    case kMixCNOT: {
      const int qt = n - 1 - op.a;
      for (uint32_t k = tid; k < DD; k += 256) {
        const uint32_t pk = mixed_cnot_index(k, q, qt, n);
        if (k < pk) {
          const C tmp = rho[k];
          rho[k] = rho[pk];
          rho[pk] = tmp;
        }
      }
      break;
    }
    case kMixPhaseDamp:
    case kMixAmpDamp:
    case kMixDepol: {
      const MixedChannel<T> ch = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample));
      mixed_walk_blocks<T>(rho, snap, blk, DD / 4,
                           [&](C& m00, C& m01, C& m10, C& m11) { mixed_block_channel<T>(ch, m00, m01, m10, m11); });
      break;
    }
    case kMixChannel2: {
      if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel2) {
        // 4^n / 16 blocks for 256 threads: fewer blocks than threads up to n = 5, one block (all of rho) at n = 2
        const int q2 = n - 1 - op.wire2;
        const MixedBlock2 b = mixed_block2(q, q2, q + n, q2 + n);
        const auto su = mixed_super2<T>(op, gates);
        for (uint32_t t = tid; t < DD / 16; t += 256) mixed_block_super2<T, false>(su, rho, snap, mixed_block2_base(t, b), b);
      }
      break;
    }
    case kMixGate2: {
      if constexpr (mixed_has_gate2(LEVEL)) {
        // the two-wire channel's walk: fewer blocks than threads up to n = 5, one block at n = 2; no snapshot (a unitary)
        const int q2 = n - 1 - op.wire2;
        const MixedBlock2 b = mixed_block2(q, q2, q + n, q2 + n);
        const MixedU2<T> u = mixed_unitary2<T>(op, gates);
        for (uint32_t t = tid; t < DD / 16; t += 256) mixed_block_gate2<T, false>(u, rho, mixed_block2_base(t, b), b);
      }
      break;
    }
    case kMixChannel: {
      if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel) {
        const MixedSuper<T> su = mixed_super<T>(op, gates);
        mixed_walk_blocks<T>(rho, snap, blk, DD / 4,
                             [&](C& m00, C& m01, C& m10, C& m11) { mixed_block_super<T>(su, m00, m01, m10, m11); });
      }
      break;
    }
    default: break;
  }
}

// The program on one sample's rho, a barrier behind every op: the body of both forward kernels
template <typename T, int LEVEL>
__device__ __forceinline__ void mixed_replay(const MixedOp* __restrict__ prog, V2<T>* __restrict__ rho,
                                             const double* __restrict__ angle_rows, const double* __restrict__ feats,
                                             const double* __restrict__ gates, double* s_red, const MixedScalars& m,
                                             int64_t sample) {
  for (int oi = 0; oi < m.n_ops; ++oi) {
    const MixedOp op = prog[oi];
    mixed_apply_op<T, LEVEL>(op, rho, nullptr, angle_rows, feats, gates, s_red, m, sample);
    __syncthreads();
  }
}

template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_kernel(const MixedOp* __restrict__ prog,
                                                    const double* __restrict__ angle_rows,
                                                    const double* __restrict__ feats,
                                                    const double* __restrict__ gates, double* __restrict__ out,
                                                    V2<T>* __restrict__ workspace, const MixedScalars m) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[256];
  C* rho = m.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : workspace + ((size_t)blockIdx.x << (2 * m.n));

  for (int64_t sample = blockIdx.x; sample < m.batch; sample += gridDim.x) {
    mixed_replay<T, LEVEL>(prog, rho, angle_rows, feats, gates, s_red, m, sample);
    mixed_read_out<T>(rho, out, s_red, m, sample);  // the diagonal
    __syncthreads();
  }
}

// mixed_kernel with the sampled read-out (the program ended in kMixShots; m.n_ops counts the ops in front of it).  An
// instantiation of its own: the analytic kernel carries none of this, neither registers nor LDS.
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_sampled_kernel(const MixedOp* __restrict__ prog,
                                                            const double* __restrict__ angle_rows,
                                                            const double* __restrict__ feats,
                                                            const double* __restrict__ gates, double* __restrict__ out,
                                                            V2<T>* __restrict__ workspace, const MixedScalars m,
                                                            const MixedShots sh) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[256];
  __shared__ double s_cdf[256];    // n <= 8: 2^n prefix sums
  __shared__ uint32_t s_cnt[256];  // and as many counts
  C* rho = m.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : workspace + ((size_t)blockIdx.x << (2 * m.n));

  for (int64_t sample = blockIdx.x; sample < m.batch; sample += gridDim.x) {
    mixed_replay<T, LEVEL>(prog, rho, angle_rows, feats, gates, s_red, m, sample);
    mixed_sample_read_out<T>(rho, out + sample * m.out_ld, s_cdf, s_cnt, m.n, m.measure, sample, sh);
    __syncthreads();
  }
}

// mixed_kernel with the measurement table's read-out (measure 2: m.n_obs terms behind the m.n_ops ops).  An instantiation
// of its own, as the sampled read-out's: the probs / <Z> kernel carries none of it.
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_obs_kernel(const MixedOp* __restrict__ prog,
                                                        const double* __restrict__ angle_rows,
                                                        const double* __restrict__ feats,
                                                        const double* __restrict__ gates, double* __restrict__ out,
                                                        V2<T>* __restrict__ workspace, const MixedScalars m) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[256];
  __shared__ double s_term[256];
  C* rho = m.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : workspace + ((size_t)blockIdx.x << (2 * m.n));

  for (int64_t sample = blockIdx.x; sample < m.batch; sample += gridDim.x) {
    mixed_replay<T, LEVEL>(prog, rho, angle_rows, feats, gates, s_red, m, sample);
    mixed_obs_read_out<T>(rho, out + sample * m.out_ld, s_term, prog + m.n_ops, m.n_obs, m.n);
  }
}

// mixed_kernel with the reduced density matrix's read-out (measure 8: the program ended in kMixRho, `mask` is its keep-mask;
// m.n_ops counts the ops in front of it).  An instantiation of its own, as the measurement table's.
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_rho_kernel(const MixedOp* __restrict__ prog,
                                                        const double* __restrict__ angle_rows,
                                                        const double* __restrict__ feats,
                                                        const double* __restrict__ gates, double* __restrict__ out,
                                                        V2<T>* __restrict__ workspace, const MixedScalars m,
                                                        const uint32_t mask) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[256];
  C* rho = m.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : workspace + ((size_t)blockIdx.x << (2 * m.n));

  for (int64_t sample = blockIdx.x; sample < m.batch; sample += gridDim.x) {
    mixed_replay<T, LEVEL>(prog, rho, angle_rows, feats, gates, s_red, m, sample);
    mixed_rho_read_out<T>(rho, out + sample * m.out_ld, mask, m.n, 0u, 1u);
    __syncthreads();
  }
}

// ---- reverse sweep ------------------------------------------------------------------------------------------------
// Per sample: replay the forward to rho_N (copying rho to a snapshot in front of every channel and every later state
// preparation), seed the adjoint Lambda_N = dL/drho_N (diagonal: diag(g) for probs, sum_w g_w (1 - 2 bit_w) for <Z>),
// then walk the program backwards with rho_k and Lambda_k side by side:
//     single-wire unitary U (generator G for RY: Y, PHASE: Z):
//         N = sum over the wire's 2 x 2 blocks of B_rho B_Lambda^dagger  (= Tr_other rho_k Lambda_k)
//         dL/dtheta = Im Tr(G N);  GATE: R = U^dagger N, dL/dRe U_ab = 2 Re R_ba, dL/dIm U_ab = -2 Im R_ba
//         rho, Lambda <- U^dagger B U  (one pass over both)
//     two-wire unitary (GATE2): the same on the 4 x 4 blocks of its wires, N and R 4 x 4
//     CZ / CNOT: applied to both (involutions)
//     channel E: Lambda <- E^dagger(Lambda) (the general channel: S^H on vec of each block), rho <- snapshot (a channel is not inverted: Depolarizing(0.9) has
//         condition number 5 per wire).  A native channel with a >= 0 (strength from a row) first reduces
//         dL/dstrength = <Lambda, E'(snapshot)> over the wire's blocks, like RY its Im Tr(G N).  A general channel whose
//         rows get a gradient (kMixChannelFit, kMixChannel2Fit; the kLevelFit instantiations) first reduces
//         W[r][c] = sum over blocks of conj(vec(Lambda)[r]) vec(snapshot)[c]: dL/dRe S = Re W, dL/dIm S = -Im W
//     AMP_EMBED: rho_0 = v v^T / |v|^2, dL/dv = 2 (Re(Lambda) v - (v^T Re(Lambda) v / |v|^2) v) / |v|^2
// Gradients go to per-sample double outputs (no atomics): every reduction runs in a fixed order, so reruns are
// bit-identical.  Thread 0 adds each parameter's reduced value after the op's barrier.
struct MixedBwdScalars {
  int64_t gout_ld;
  int32_t n_rows, n_gates, n_snaps, pad_;
};

// U^dagger B U for the 2 x 2 block (b00, b01, b10, b11), in place
template <typename T>
__device__ __forceinline__ void mixed_udag_b_u(V2<T>& b00, V2<T>& b01, V2<T>& b10, V2<T>& b11, V2<T> u00, V2<T> u01,
                                               V2<T> u10, V2<T> u11) {
  // A = U^dagger B:  A_xl = sum_k conj(U_kx) B_kl
  const V2<T> a00 = cmulc<T>(b00, u00) + cmulc<T>(b10, u10), a01 = cmulc<T>(b01, u00) + cmulc<T>(b11, u10);
  const V2<T> a10 = cmulc<T>(b00, u01) + cmulc<T>(b10, u11), a11 = cmulc<T>(b01, u01) + cmulc<T>(b11, u11);
  // B' = A U
  b00 = cmul<T>(a00, u00) + cmul<T>(a01, u10);
  b01 = cmul<T>(a00, u01) + cmul<T>(a01, u11);
  b10 = cmul<T>(a10, u00) + cmul<T>(a11, u10);
  b11 = cmul<T>(a10, u01) + cmul<T>(a11, u11);
}

// The seed, the CZ sign and the CNOT partner are the forward's helpers.  The three block loops are written out, not
// calls of the walkers: with the loops as walker calls (and nothing else changed) the state and every single
// contribution stay the same, but gradients that sum two contributions move by one unit in the last place -- the
// compiler then contracts thread 0's `+= scale * s` behind each op differently.  (Building RY / GATE with mixed_unitary
// kept the bits on the n = 6 cases of tools/mixed_bits.py; it waits for a change that runs the whole list and the
// timing.)
// OBS: the seed is the measurement table's (measure 2); an instantiation of its own, the probs / <Z> one carries none of it.
// RHO: the seed is the reduced density matrix's (measure 8, the keep-mask in the kMixRho op behind the m.n_ops ops); likewise.
template <typename T, int LEVEL, bool OBS = false, bool RHO = false>
__global__ __launch_bounds__(256) void mixed_backward_kernel(
    const MixedOp* __restrict__ prog, const double* __restrict__ angle_rows, const double* __restrict__ feats,
    const double* __restrict__ gates, const double* __restrict__ grad_out, double* __restrict__ grad_rows,
    double* __restrict__ grad_gates, double* __restrict__ grad_feats, V2<T>* __restrict__ workspace,
    const MixedScalars m, const MixedBwdScalars b) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double s_red[256];
  __shared__ double s_v[256];
  constexpr bool kGate2 = mixed_has_gate2(LEVEL);
  constexpr bool kFit = mixed_has_fit(LEVEL);  // the gradient of kMixChannelFit / kMixChannel2Fit rows: instantiations of their own
  static_assert(!kFit || (kGate2 && mixed_channels_of(LEVEL) >= kLevelChannel2), "kLevelFit rides on the full level");
  __shared__ double s_part[2][4][kGate2 ? 32 : 8];  // the four waves' partials of an op's sums, double-buffered
  const int n = m.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t D = 1u << n, DD = 1u << (2 * n);
  // workspace per workgroup: [rho, Lambda unless in LDS] then n_snaps snapshots
  const size_t per_block = (size_t)(m.slab_in_lds ? 0 : 2) + (size_t)b.n_snaps;
  C* const slabs = workspace + (size_t)blockIdx.x * per_block * DD;
  C* const rho = m.slab_in_lds ? reinterpret_cast<C*>(smem_raw) : slabs;
  C* const lam = rho + DD;
  C* const snaps = m.slab_in_lds ? slabs : slabs + 2 * (size_t)DD;
  int buf = 0;

  for (int64_t sample = blockIdx.x; sample < m.batch; sample += gridDim.x) {
    for (int r = tid; r < b.n_rows; r += 256) grad_rows[(size_t)r * m.batch + sample] = 0.0;
    for (int i = tid; i < b.n_gates * 8; i += 256) grad_gates[(size_t)sample * b.n_gates * 8 + i] = 0.0;
    if (grad_feats)  // thread k owns feature k (n_features <= 2^n <= 256) here and in AMP_EMBED below
      for (int k = tid; k < m.n_features; k += 256) grad_feats[sample * m.n_features + k] = 0.0;

    // ---- replay -------------------------------------------------------------------------------------------------
    int si = 0;
    for (int oi = 0; oi < m.n_ops; ++oi) {
      const MixedOp op = mixed_constant_kind<kFit>(prog[oi]);
      C* snap = mixed_needs_snapshot(op.kind, oi) ? snaps + (size_t)(si++) * DD : nullptr;
      mixed_apply_op<T, LEVEL>(op, rho, snap, angle_rows, feats, gates, s_red, m, sample);
      __syncthreads();
    }

    // ---- seed Lambda_N --------------------------------------------------------------------------------------------
    const double* __restrict__ g = grad_out + sample * b.gout_ld;
    if constexpr (OBS) {  // s_v is free until AMP_EMBED, the last op backwards
      const MixedOp* __restrict__ terms = prog + m.n_ops;
      mixed_obs_seed_weights(s_v, g, terms, m.n_obs);
      __syncthreads();
      for (uint32_t k = tid; k < DD; k += 256) lam[k] = mixed_obs_seed_elem<T>(terms, m.n_obs, s_v, k, n);
    } else if constexpr (RHO) {
      const uint32_t mask = (uint32_t)prog[m.n_ops].wire;  // uniform: a scalar load
      for (uint32_t k = tid; k < DD; k += 256) lam[k] = mixed_rho_seed_elem<T>(g, k, mask, n);
    } else {
      for (uint32_t k = tid; k < DD; k += 256) lam[k] = mixed_seed_elem<T>(g, k, m);
    }
    __syncthreads();

    // ---- reverse sweep --------------------------------------------------------------------------------------------
    for (int oi = m.n_ops - 1; oi >= 0; --oi) {
      const MixedOp op = mixed_constant_kind<kFit>(prog[oi]);
      bool fit = false;  // the op's rows get a gradient
      if constexpr (kFit) fit = prog[oi].kind != op.kind;
      const int q = n - 1 - op.wire;
      // a native channel that reads its strength from a row feeds that row like an angle op
      const bool graded = (op.kind == kMixPhaseDamp || op.kind == kMixAmpDamp || op.kind == kMixDepol) && op.a >= 0;
      const bool param = op.kind == kMixPhase || op.kind == kMixRY || op.kind == kMixGate || graded ||
                         (kGate2 && op.kind == kMixGate2) || (kFit && fit && op.kind == kMixChannel);
      switch (op.kind) {
        case kMixPhase:
        case kMixRY:
        case kMixGate: {
          C u00, u01, u10, u11;
          if (op.kind == kMixGate) {
            const double* __restrict__ gu = gates + (size_t)op.a * 8;
            u00 = C{(T)gu[0], (T)gu[1]};
            u01 = C{(T)gu[2], (T)gu[3]};
            u10 = C{(T)gu[4], (T)gu[5]};
            u11 = C{(T)gu[6], (T)gu[7]};
          } else {
            const double th = mixed_angle(op, angle_rows, m, sample);
            double sn, cs;
            if (op.kind == kMixRY) {
              sincos(0.5 * th, &sn, &cs);
              u00 = C{(T)cs, 0};
              u01 = C{(T)-sn, 0};
              u10 = C{(T)sn, 0};
              u11 = C{(T)cs, 0};
            } else {  // diag(1, e^{i phi}), as the forward applies it
              sincos(th, &sn, &cs);
              u00 = C{(T)1, 0};
              u01 = C{0, 0};
              u10 = C{0, 0};
              u11 = C{(T)cs, (T)sn};
            }
          }
          // N_ab = sum over blocks, c of rho_ac conj(Lambda_bc): (re, im) of N00, N01, N10, N11
          double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          for (uint32_t t = tid; t < DD / 4; t += 256) {
            const uint32_t base = insert_two_bits(t, q, q + n);
            const uint32_t cj = 1u << q, ci = 1u << (q + n);
            C r00 = rho[base], r01 = rho[base | cj], r10 = rho[base | ci], r11 = rho[base | ci | cj];
            C l00 = lam[base], l01 = lam[base | cj], l10 = lam[base | ci], l11 = lam[base | ci | cj];
            mixed_block_n_accumulate<T>(acc, r00, r01, r10, r11, l00, l01, l10, l11);
            mixed_udag_b_u<T>(r00, r01, r10, r11, u00, u01, u10, u11);
            mixed_udag_b_u<T>(l00, l01, l10, l11, u00, u01, u10, u11);
            rho[base] = r00; rho[base | cj] = r01; rho[base | ci] = r10; rho[base | ci | cj] = r11;
            lam[base] = l00; lam[base | cj] = l01; lam[base | ci] = l10; lam[base | ci | cj] = l11;
          }
          if (op.kind == kMixGate) {
            for (int k = 0; k < 8; ++k) {
              const double s = mixed_wave_sum(acc[k]);
              if (lane == 0) s_part[buf][wave][k] = s;
            }
          } else {
            // Im Tr(G N): Y -> Re N01 - Re N10, Z -> Im N00 - Im N11
            const double v = op.kind == kMixRY ? acc[2] - acc[4] : acc[1] - acc[7];
            const double s = mixed_wave_sum(v);
            if (lane == 0) s_part[buf][wave][0] = s;
          }
          break;
        }
        case kMixCZ: {
          const int qt = n - 1 - op.a;
          for (uint32_t k = tid; k < DD; k += 256)
            if (mixed_cz_flips(k, q, qt, n)) {
              rho[k] = C{-rho[k].x, -rho[k].y};
              lam[k] = C{-lam[k].x, -lam[k].y};
            }
          break;
        }
        case kMixCNOT: {
          const int qt = n - 1 - op.a;
          for (uint32_t k = tid; k < DD; k += 256) {
            const uint32_t pk = mixed_cnot_index(k, q, qt, n);
            if (k < pk) {
              const C tr = rho[k], tl = lam[k];
              rho[k] = rho[pk];
              rho[pk] = tr;
              lam[k] = lam[pk];
              lam[pk] = tl;
            }
          }
          break;
        }
        case kMixPhaseDamp:
        case kMixAmpDamp:
        case kMixDepol: {
          const double strength = mixed_angle(op, angle_rows, m, sample);
          const MixedChannel<T> ch = mixed_channel<T>(op.kind, strength);
          const C* __restrict__ sp = snaps + (size_t)(--si) * DD;
          double acc_off = 0.0, acc_diag = 0.0;  // a >= 0: <Lambda behind the channel, E'(rho in front of it)>
          for (uint32_t t = tid; t < DD / 4; t += 256) {
            const uint32_t base = insert_two_bits(t, q, q + n);
            const uint32_t cj = 1u << q, ci = 1u << (q + n);
            C l00 = lam[base], l01 = lam[base | cj], l10 = lam[base | ci], l11 = lam[base | ci | cj];
            const C r00 = sp[base], r01 = sp[base | cj], r10 = sp[base | ci], r11 = sp[base | ci | cj];
            if (graded) {
              acc_off += mixed_strength_grad_off<T>(r01, r10, l01, l10);
              acc_diag += mixed_strength_grad_diag<T>(op.kind, r00, r11, l00, l11);
            }
            mixed_block_channel_adjoint<T>(ch, l00, l01, l10, l11);
            lam[base] = l00;
            lam[base | ci | cj] = l11;
            lam[base | cj] = l01;
            lam[base | ci] = l10;
            rho[base] = r00;
            rho[base | cj] = r01;
            rho[base | ci] = r10;
            rho[base | ci | cj] = r11;
          }
          if (graded) {
            const double s = mixed_wave_sum(mixed_channel_doff(op.kind, strength) * acc_off + acc_diag);
            if (lane == 0) s_part[buf][wave][0] = s;
          }
          break;
        }
        case kMixChannel2: {  // S^H on vec of each 4 x 4 block of Lambda, rho from the snapshot; its 64 rows of grad_gates stay zero (kMixChannel2Fit: dL/dS)
          if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel2) {
            const int q2 = n - 1 - op.wire2;
            const MixedBlock2 bl = mixed_block2(q, q2, q + n, q2 + n);
            const auto su = mixed_super2<T>(op, gates);
            const C* __restrict__ sp = snaps + (size_t)(--si) * DD;
            if constexpr (kFit) {
              if (fit) {  // uniform over the workgroup.  Thread 16 r + c adds its own entry: no other thread touches it
                double re, im;
                mixed_super2_grad<T>(lam, sp, DD / 16, bl, re, im);
                double* __restrict__ go = grad_gates + ((size_t)sample * b.n_gates + op.a) * 8 + 2 * tid;
                go[0] += re;
                go[1] -= im;
                __syncthreads();
              }
            }
            for (uint32_t t = tid; t < DD / 16; t += 256) mixed_block_super2<T, true>(su, lam, nullptr, mixed_block2_base(t, bl), bl);
            for (uint32_t k = tid; k < DD; k += 256) rho[k] = sp[k];
          }
          break;
        }
        case kMixGate2: {  // N of the 4 x 4 blocks in 32 doubles a thread; rho and Lambda un-computed in place
          if constexpr (kGate2) {
            const int q2 = n - 1 - op.wire2;
            const MixedBlock2 bl = mixed_block2(q, q2, q + n, q2 + n);
            const MixedU2<T> u = mixed_unitary2<T>(op, gates);
            double acc[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) acc[k] = 0.0;
            for (uint32_t t = tid; t < DD / 16; t += 256) mixed_block_gate2_reverse<T>(u, acc, rho, lam, mixed_block2_base(t, bl), bl);
#pragma unroll
            for (int k = 0; k < 32; ++k) {
              const double s = mixed_wave_sum(acc[k]);
              if (lane == 0) s_part[buf][wave][k] = s;
            }
          }
          break;
        }
        case kMixChannel: {  // its four rows of grad_gates stay zero: channel operands get no gradient (kMixChannelFit: dL/dS)
          if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel) {
            const MixedSuper<T> su = mixed_super<T>(op, gates);
            const C* __restrict__ sp = snaps + (size_t)(--si) * DD;
            if constexpr (kFit) {
              if (fit) {  // W of the thread's blocks (the blocks it owns below), then across the workgroup like GATE2's N
                double acc[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) acc[k] = 0.0;
                for (uint32_t t = tid; t < DD / 4; t += 256) {
                  const uint32_t base = insert_two_bits(t, q, q + n);
                  const uint32_t cj = 1u << q, ci = 1u << (q + n);
                  const C l[4] = {lam[base], lam[base | cj], lam[base | ci], lam[base | ci | cj]};
                  const C r[4] = {sp[base], sp[base | cj], sp[base | ci], sp[base | ci | cj]};
                  mixed_super_grad_accumulate<T>(acc, l, r);
                }
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                  const double s = mixed_wave_sum(acc[k]);
                  if (lane == 0) s_part[buf][wave][k] = s;
                }
              }
            }
            for (uint32_t t = tid; t < DD / 4; t += 256) {
              const uint32_t base = insert_two_bits(t, q, q + n);
              const uint32_t cj = 1u << q, ci = 1u << (q + n);
              C l00 = lam[base], l01 = lam[base | cj], l10 = lam[base | ci], l11 = lam[base | ci | cj];
              mixed_block_super_adjoint<T>(su, l00, l01, l10, l11);
              lam[base] = l00;
              lam[base | cj] = l01;
              lam[base | ci] = l10;
              lam[base | ci | cj] = l11;
              rho[base] = sp[base];
              rho[base | cj] = sp[base | cj];
              rho[base | ci] = sp[base | ci];
              rho[base | ci | cj] = sp[base | ci | cj];
            }
          }
          break;
        }
        case kMixAmpEmbed: {
          const double* __restrict__ row = feats + sample * m.feat_ld;
          if (tid < (int)D) s_v[tid] = tid < m.n_features ? row[tid] + m.enc_offset : m.pad_with;
          __syncthreads();
          double v = 0.0, lv = 0.0;  // v_i and (Re(Lambda) v)_i for i = tid
          if (tid < (int)D) {
            v = s_v[tid];
            for (uint32_t j = 0; j < D; ++j) lv += (double)lam[((uint32_t)tid << n) | j].x * s_v[j];
          }
          const double inv = 1.0 / mixed_block_sum(v * v, s_red);
          const double quad = mixed_block_sum(v * lv, s_red) * inv;
          if (grad_feats && tid < m.n_features) grad_feats[sample * m.n_features + tid] += 2.0 * (lv - quad * v) * inv;
        }
          [[fallthrough]];
        case kMixZero: {
          if (oi > 0) {  // a later preparation: nothing before it reaches the output
            const C* __restrict__ sp = snaps + (size_t)(--si) * DD;
            for (uint32_t k = tid; k < DD; k += 256) {
              lam[k] = C{0, 0};
              rho[k] = sp[k];
            }
          }
          break;
        }
        default: break;
      }
      __syncthreads();
      if (param) {
        if (tid == 0) {
          if (kFit && op.kind == kMixChannel) {
            if constexpr (kFit) {  // dL/dRe S = Re W, dL/dIm S = -Im W, in the layout of the rows
              double* __restrict__ go = grad_gates + ((size_t)sample * b.n_gates + op.a) * 8;
              for (int k = 0; k < 32; ++k) {
                const double s = s_part[buf][0][k] + s_part[buf][1][k] + s_part[buf][2][k] + s_part[buf][3][k];
                go[k] += (k & 1) ? -s : s;
              }
            }
          } else if (kGate2 && op.kind == kMixGate2) {
            if constexpr (kGate2) {
              double s[32];
              for (int k = 0; k < 32; ++k) s[k] = s_part[buf][0][k] + s_part[buf][1][k] + s_part[buf][2][k] + s_part[buf][3][k];
              mixed_gate2_grad_accumulate(s, gates + (size_t)op.a * 8, grad_gates + ((size_t)sample * b.n_gates + op.a) * 8);
            }
          } else if (op.kind == kMixGate) {
            double s[8];
            for (int k = 0; k < 8; ++k) s[k] = s_part[buf][0][k] + s_part[buf][1][k] + s_part[buf][2][k] + s_part[buf][3][k];
            mixed_gate_grad_accumulate(s, gates + (size_t)op.a * 8, grad_gates + ((size_t)sample * b.n_gates + op.a) * 8);
          } else if (op.a >= 0) {
            const double s = s_part[buf][0][0] + s_part[buf][1][0] + s_part[buf][2][0] + s_part[buf][3][0];
            grad_rows[(size_t)op.a * m.batch + sample] += op.scale * s;
          }
        }
        buf ^= 1;
      }
    }
    __syncthreads();
  }
}

}  // namespace qiddm

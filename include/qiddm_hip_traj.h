/* qiddm_hip_traj.h -- extension of qiddm_hip.h: the trajectory engine of the density-matrix executor.
 * Same library (libqiddm_hip), same ABI version, same conventions (status codes, qiddm_last_error, qiddm_mixed_op_t,
 * QIDDM_MIX_* / QIDDM_MEAS_* from qiddm_hip.h, which this header includes).  It is a header of its own so that
 * qiddm_hip.h keeps declaring exactly the functions it declared before; the Python binding mirrors the split
 * (qiddm_amd/_capi.py: SIGNATURES for qiddm_hip.h, TRAJ_SIGNATURES for this header).                       */
#ifndef QIDDM_HIP_TRAJ_H
#define QIDDM_HIP_TRAJ_H

#include "qiddm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Quantum trajectories (Monte-Carlo wavefunctions): the programs of the density-matrix executor at 1 <= n_qubits <= 16
 * (else QIDDM_ERR_UNSUPPORTED), where one sample's rho no longer fits.  A trajectory keeps a PURE state psi (2^n elements,
 * wire w at bit n-1-w), draws one Kraus operator at every channel op, renormalises, and reads out; `out` is the mean of the
 * read-outs of n_traj trajectories per sample, which estimates what qiddm_mixed_forward returns with a standard error that
 * falls as 1 / sqrt(n_traj).  One workgroup of 256 threads runs one trajectory at a time; psi lives in LDS while 2^n
 * elements fit in 128 KiB (n <= 14 in float32, n <= 13 in float64), else in a slab of `workspace` per workgroup.
 * Arguments: those of qiddm_mixed_forward (qiddm_hip.h) up to `batch`, then
 *   n_traj      trajectories per sample, 1 .. 2^20 (`n_traj %d outside 1 .. 2^20`)
 *   seed        the Philox key: an integer-valued double in [0, 2^53) (`trajectory seed %g is not an integer in [0, 2^53)`)
 *   offset      the stream offset: an integer-valued double in [0, 2^32) (`trajectory offset %g is not an integer in [0, 2^32)`)
 *   max_blocks  grid cap (0: the default, 2048 workgroups with psi in LDS and 256 with psi in the workspace)
 *   out         (batch, out_ld >= width) float64 DEVICE, width = 2^n | n | columns of the table
 *   per_traj    (batch, n_traj, width) float64 DEVICE or NULL: every trajectory's own read-out
 *   branches    (batch, n_traj, n_channels) int32 DEVICE or NULL: the operator chosen at every decision, n_channels = the
 *               channel ops of the program.  Both exist for tests and diagnostics; NULL costs nothing.
 * Accepted kinds: ZERO, AMP_EMBED, PHASE (applied as RZ: diag(e^{-i phi/2}, e^{+i phi/2})), RY, GATE, CZ, CNOT, GATE2,
 * PHASE_DAMP, AMP_DAMP, DEPOL (constant or per-sample strength, the p + scale * angle_rows[a][sample] rule) and
 *   QIDDM_MIX_KRAUS (= 40)    a general one-wire channel on `wire` given by its Kraus operators: `reserved` = m of them,
 *                             1 <= m <= 8 (`op %d: %d Kraus operators (1 .. 8 are taken)`), in the m consecutive rows
 *                             a .. a+m-1 of `gates` (`op %d: Kraus rows %d..%d out of range`), row a+k = K_k as (k00, k01,
 *                             k10, k11) in (re, im): QIDDM_MIX_GATE's layout.  `p` and `scale` are not read; that
 *                             sum_k K_k^H K_k = 1 is the caller's responsibility.  Only this entry point takes the kind:
 *                             the four density-matrix entry points refuse it as `op %d: unknown kind 40`.
 *   QIDDM_MIX_KRAUS2 (= 48)   a general two-wire channel on (`wire`, `reserved`) given by its Kraus operators; GATE2's
 *                             convention: 4 x 4 index 2 b(wire) + b(reserved), the first wire most significant.  `p` = m
 *                             of them, an integer-valued double in 1 .. QIDDM_MIX_MAX_KRAUS2 = 16 (`op %d: %g Kraus
 *                             operators (1 .. 16 are taken)`; integers travel in `p` as the seed of QIDDM_MIX_SHOTS does),
 *                             in the 4m consecutive rows a .. a+4m-1 of `gates` (`op %d: Kraus rows %d..%d out of range`,
 *                             summed in 64 bits): operator k in rows a+4k .. a+4k+3, row r = K_k[r][0..3] as (re, im) --
 *                             QIDDM_MIX_GATE2's layout, one matrix after another.  Checked in this order: `wire`
 *                             (`op %d: wire %d out of range`), `reserved` (`op %d: bad second wire %d` outside 0..n-1 or
 *                             equal to `wire`), m, the rows.  `scale` is not read; sum_k K_k^H K_k = 1 is the caller's
 *                             responsibility.  The two trajectory entry points alone take the kind: the four
 *                             density-matrix entry points and the planners refuse it as `op %d: unknown kind 48`.
 *                             Kind 41 is no op anywhere.
 * Refused with QIDDM_ERR_UNSUPPORTED and a reason that names the alternative: the superoperator kinds 16 / 18 / 32 / 34
 * (`op %d: kind %d is a channel given by its superoperator ...`: hand a one-wire channel over as QIDDM_MIX_KRAUS and a
 * two-wire channel as QIDDM_MIX_KRAUS2), QIDDM_MIX_SHOTS (`op %d: a sampled read-out on
 * trajectories ...`), QIDDM_MEAS_RHO / QIDDM_MIX_RHO (`a density-matrix read-out on trajectories ...`).  Every other check
 * is qiddm_mixed_forward's, in its order; n_traj, seed, offset and max_blocks follow the ops and are refused for an empty
 * batch as well; then out / out_ld and the workspace.  batch == 0 returns QIDDM_OK.  The reverse sweep: qiddm_hip_traj_grad.h.
 *
 * THE TRAJECTORY RULE.  Channel ops are numbered d = 0, 1, ... in program order (every PHASE_DAMP, AMP_DAMP, DEPOL,
 * KRAUS and KRAUS2 op; nothing else: a KRAUS2 op is one channel op in d, in n_channels and in `branches`).  In trajectory t (0-based) of sample b (the ABSOLUTE row of the batch), channel op d on the
 * wire at bit q = n-1-wire is applied as follows, everything in float64 whatever the state's dtype:
 *   1. the wire's reduced matrix, unnormalised, over the pairs (a0, a1) = (psi[k with bit q clear], psi[k | 1 << q]):
 *        r00 = sum |a0|^2,  r11 = sum |a1|^2,  r01 = sum a0 conj(a1)
 *      (per-thread partials in ascending k, a wave butterfly, four partials in LDS added in wave order; no atomics).
 *   2. the weights w_k = |K_k psi|^2 of the op's operator list, PennyLane's order:
 *        KRAUS        K_0 .. K_{m-1} as given;
 *                     w_k = max(0, (|k00|^2 + |k10|^2) r00 + (|k01|^2 + |k11|^2) r11 + 2 Re((k00 conj(k01) + k10 conj(k11)) r01))
 *        PHASE_DAMP   K_0 = diag(1, sqrt(1-g)), K_1 = diag(0, sqrt(g));        w_0 = r00 + (1-g) r11,  w_1 = g r11
 *        AMP_DAMP     K_0 = diag(1, sqrt(1-g)), K_1 = [[0, sqrt(g)], [0, 0]];  w_0 = r00 + (1-g) r11,  w_1 = g r11
 *        DEPOL        K_0 = sqrt(1-p) 1, K_1..3 = sqrt(p/3) X, Y, Z;           w_0 = 1 - p,  w_1 = w_2 = w_3 = p / 3
 *                     (the weights of unitary operators do not depend on a normalised psi: step 1 is skipped)
 *      with g / p the strength of sample b.
 *   3. c_k = w_0 + ... + w_k, added sequentially in k; W = c_{m-1}.  W not positive or not finite: the trajectory stops,
 *      its read-out is NaN in every element (so is the sample's row of `out`), its entries of `branches` from d on are -1.
 *   4. one 32-bit word of Philox4x32-10: word (d & 3) of counter (d >> 2, t, b mod 2^32, offset) under key (seed mod 2^32,
 *      seed >> 32);  v = ((double)word * 2^-32) * W;  the chosen operator is #{k : c_k <= v}, clamped to m - 1.  An
 *      operator of weight zero is never chosen.
 *   5. psi <- K_k psi / sqrt(w_k): the 2 x 2 matrix K_k / sqrt(w_k) is formed in float64, rounded once to the state's
 *      dtype, and applied like a GATE.  DEPOL applies 1, X, Y or Z exactly (k = 0 leaves psi untouched).
 *   A KRAUS2 op on the bits q = n-1-wire and q2 = n-1-reserved follows the same five steps with the pair in the wire's place:
 *   1. the pair's reduced matrix, unnormalised, over the quadruples a_0 .. a_3 of psi (a_j = psi[k with the bits set as in
 *      j = 2 b(q) + b(q2)]):  R[r][c] = sum a_r conj(a_c) for r <= c -- 4 real and 6 complex sums, 16 doubles in one
 *      reduction (per-thread partials in ascending quadruple index, a wave butterfly, four partials added in wave order).
 *   2. w_k = max(0, Tr(K_k R K_k^H)),  Tr(K R K^H) = sum_r G[r][r] R[r][r] + 2 Re sum_{r<c} G[c][r] R[r][c],  G = K^H K.
 *      No special case for unitary operator sets: two-qubit depolarizing goes through R like anything else.
 *   3., 4. as above (sequential sums, the stop at W not positive or not finite, one Philox word, the clamp).
 *   5. psi <- K_k psi / sqrt(w_k): the 4 x 4 matrix K_k / sqrt(w_k) is formed in float64, rounded once to the state's
 *      dtype, and applied as GATE2 applies its matrix.  psi is swept twice per op: a read for R, a read and a write here.
 * Read-out of a trajectory, float64: QIDDM_MEAS_PROBS |psi_k|^2; QIDDM_MEAS_EXPZ sum_k (+-)|psi_k|^2 per wire;
 * QIDDM_MEAS_OBS the formula of QIDDM_MIX_OBS with rho[k][k ^ x] = psi_k conj(psi_{k ^ x}).
 * THE MEAN does not depend on the grid.  S = min(n_traj, 64) slots; trajectory t belongs to slot t mod S.  The read-outs
 * of the trajectories of (sample, slot) are added in ascending t into a float64 row of the workspace that belongs to that
 * pair alone (the first is stored, the others added to it); then out[b][j] = (row(b, 0)[j] + row(b, 1)[j] + ... in
 * ascending slot, starting from 0.0) / n_traj.  No float atomics: reruns and a lowered max_blocks give the same bits.
 *   qiddm_mixed_traj_workspace_bytes  host only: program head + batch * S * measure_width float64 + (psi outside LDS) one
 *                                     slab of 2^n elements per workgroup; every term rounded up to 256 B.  measure_width
 *                                     is the width of `out` (`measure_width %lld out of range` below 1).             */
int64_t qiddm_mixed_traj_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj, int32_t n_ops,
                                         int64_t measure_width, int32_t max_blocks);
int qiddm_mixed_traj_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                             const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                             int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                             const double *gates, int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj,
                             double seed, double offset, int32_t max_blocks, double *out, int64_t out_ld,
                             double *per_traj, int32_t *branches, void *workspace, int64_t workspace_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QIDDM_HIP_TRAJ_H */

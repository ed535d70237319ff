/* qiddm_hip_traj_shots.h -- extension of qiddm_hip_traj.h: finite shots on the trajectory engine.
 * Same library (libqiddm_hip), same ABI version (2), same conventions; a header of its own so that qiddm_hip.h,
 * qiddm_hip_traj.h and qiddm_hip_traj_grad.h keep declaring exactly the functions they declared before.  The Python binding
 * mirrors the split (qiddm_amd/_capi.py: TRAJ_SHOTS_SIGNATURES for this header).                                    */
#ifndef QIDDM_HIP_TRAJ_SHOTS_H
#define QIDDM_HIP_TRAJ_SHOTS_H

#include "qiddm_hip_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A shot-limited read-out of a noisy circuit beyond the wires at which a density matrix fits (1 <= n_qubits <= 16): the
 * trajectories of qiddm_mixed_traj_forward with a SAMPLER in the place of the analytic read-out.  `shots` computational-
 * basis outcomes per sample are drawn from the trajectories' |psi_k|^2 inside the launch that holds psi and counted in
 * integers; `out` is count / shots (QIDDM_MEAS_PROBS) or the wires' <Z> estimated from the same outcomes
 * (QIDDM_MEAS_EXPZ).  A real device runs one noise realisation per shot: shots == n_traj reproduces that, and every
 * element of `out` is then a mean of `shots` independent Bernoulli draws.
 *
 * THE SAMPLING RULE.  Everything is float64, whatever the state's dtype.
 *   Trajectories.  Those of qiddm_mixed_traj_forward, decision for decision: THE TRAJECTORY RULE of qiddm_hip_traj.h is
 *     unchanged, so the same (seed, offset, absolute row b, trajectory t) give the same Philox words and the same branches.
 *   Split.  With T = n_traj, S = shots, q = S div T and r = S mod T, trajectory t draws s_t = q + (t < r) shots, the global
 *     shot indices first_t + i, first_t = t q + min(t, r), i = 0 .. s_t - 1.  A trajectory with s_t = 0 is not run (S < T: only
 *     the first S are); T_run = min(T, S).  ceil(S / T) <= 65536 (`%d shots per trajectory: at most 65536 (raise n_traj)`):
 *     a design limit, which bounds one workgroup's sampling loop so that no argument can hold a shared GPU for minutes.
 *   Weights.  p_k = max(re^2 + im^2, 0) of psi_k, a NaN counting as 0; the two products and the sum are each rounded once
 *     (no fma).  One value of p_k is used wherever one is needed: summed, walked, and handed back in `per_traj`.
 *   Two levels.  G = min(2^n, 256) segments of L = 2^n / G outcomes; segment j holds k = j + G i, i = 0 .. L-1 (the CDF
 *     order is a fixed permutation of the outcomes).  P_j = p_j + p_{j+G} + ... added sequentially in ascending i;
 *     C_j = P_0 + ... + P_j added sequentially in ascending j; W = C_{G-1}.  W not positive or not finite: the trajectory
 *     is bad (below).
 *   One shot, shot i of trajectory t of absolute row b:  word (i & 3) of Philox4x32-10 at counter
 *     (0x80000000 | (i >> 2), t, b mod 2^32, offset) under the trajectory rule's key (a decision uses d >> 2 < 2^29 in counter
 *     word 0: the top bit keeps the draws disjoint);  v = ((double)word * 2^-32) * W;  j = #{j : C_j <= v} clamped to G - 1;
 *     u = v - C_{j-1} (C_{-1} = 0);  c = 0, c += p_k over segment j in ascending i: the outcome is the first k with c > u,
 *     or, if rounding leaves none, the last k of the segment with p_k > 0.  An outcome of weight zero is never chosen.
 *   Counts.  uint32, added with integer atomics on a zeroed region of the workspace -- QIDDM_MEAS_PROBS a histogram
 *     (batch, 2^n); QIDDM_MEAS_EXPZ per sample and wire the outcomes with the wire's bit set (wire w at bit n-1-w),
 *     collected per work item and added once per item.  Arrival order cannot change an integer sum: reruns, any grid and
 *     any max_blocks give the same bits.  Then out[b][k] = count / S, or (S - 2 ones_w) / S: exact integers and one float64
 *     division per output.
 *   Bad trajectories.  One that stops at a decision (THE TRAJECTORY RULE, step 3) or whose W is invalid: the sample's row
 *     of `out` is NaN in every element and the trajectory's entries of `outcomes` are -1 (its row of `per_traj` is NaN in
 *     the first case and holds the weights that gave W in the second).
 * Arguments: those of qiddm_mixed_traj_forward up to `max_blocks`, with
 *   shots       behind n_traj: shots per sample, 1 .. 2^31 - 1 (`shots %d out of range`)
 * then
 *   out         (batch, out_ld >= width) float64 DEVICE, width = 2^n | n
 *   per_traj    (batch, T_run, 2^n) float64 DEVICE or NULL: the p_k the sampler used, for either measure
 *   branches    (batch, T_run, n_channels) int32 DEVICE or NULL: as qiddm_mixed_traj_forward's, of the trajectories run
 *   outcomes    (batch, shots) int32 DEVICE or NULL: every shot's outcome in global shot order.  NULL costs nothing.
 *   workspace, workspace_bytes, stream
 * Measures: QIDDM_MEAS_PROBS and QIDDM_MEAS_EXPZ.  QIDDM_MEAS_OBS is QIDDM_ERR_UNSUPPORTED (`a measurement table on sampled
 * trajectories: words of I and Z are signed sums of the sampled probs (QIDDM_MEAS_PROBS), words with X or Y need a basis
 * rotation in front of the read-out`).  A program that holds QIDDM_MIX_SHOTS, a superoperator kind or QIDDM_MIX_RHO is
 * refused in qiddm_mixed_traj_forward's words: the validator is shared.  Checks run in that function's order up to
 * max_blocks (the refusal of QIDDM_MEAS_OBS stands beside that of QIDDM_MEAS_RHO); then shots, then shots per trajectory
 * (all refused for an empty batch as well; batch == 0 then returns QIDDM_OK); then out / out_ld and the workspace
 * (`workspace of %lld B needed (qiddm_mixed_traj_shots_workspace_bytes)`).
 *   qiddm_mixed_traj_shots_workspace_bytes  host only: program head + the counts (batch * 2^n or batch * n uint32) + one
 *       uint32 flag per sample + (psi outside LDS: n >= 15 in float32, n >= 14 in float64) one slab of 2^n elements per
 *       workgroup; every term rounded up to 256 B.  The workgroups: min(batch * min(T_run, 64), 2048 | 256, max_blocks).
 *       `measure` other than PROBS / EXPZ is refused as above (`unknown measure %d` for none of the four).        */
int64_t qiddm_mixed_traj_shots_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj,
                                               int32_t shots, int32_t n_ops, int32_t measure, int32_t max_blocks);
int qiddm_mixed_traj_shots_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                                   const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                                   int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                                   const double *gates, int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj,
                                   int32_t shots, double seed, double offset, int32_t max_blocks, double *out,
                                   int64_t out_ld, double *per_traj, int32_t *branches, int32_t *outcomes,
                                   void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QIDDM_HIP_TRAJ_SHOTS_H */

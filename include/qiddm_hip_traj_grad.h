/* qiddm_hip_traj_grad.h -- extension of qiddm_hip_traj.h: the reverse sweep of the trajectory engine.
 * Same library (libqiddm_hip), same ABI version (2), same conventions; a header of its own so that qiddm_hip.h and
 * qiddm_hip_traj.h keep declaring exactly the functions they declared before.  The Python binding mirrors the split
 * (qiddm_amd/_capi.py: TRAJ_GRAD_SIGNATURES for this header).                                                   */
#ifndef QIDDM_HIP_TRAJ_GRAD_H
#define QIDDM_HIP_TRAJ_GRAD_H

#include "qiddm_hip_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gradients through quantum trajectories: what qiddm_mixed_backward returns for a density matrix, estimated from the
 * n_traj trajectories per sample that qiddm_mixed_traj_forward runs for the same (program, seed, offset), 1 <= n_qubits <= 16.
 *
 * THE ESTIMATOR.  The exact read-out is E(theta) = sum_b <psi_0| M_b(theta)^H O M_b(theta) |psi_0>, over every branch sequence
 * b (one Kraus operator per channel op), M_b the unnormalised product of gates and chosen operators.  The forward samples
 * b with probability p_b = |M_b psi_0|^2, so grad E = E_{b ~ p}[ grad <psi_0| M_b^H O M_b |psi_0> / p_b ].  The forward
 * renormalises at every decision and the product of the chosen weights w_d is p_b, so the gradient of one trajectory is the
 * vector-Jacobian product of a LINEAR, NON-UNITARY chain in which
 *   - channel op d is the matrix A_d = K_{k_d}(theta) / sqrt(w_d);
 *   - the branch k_d and the number w_d are FROZEN at the values the forward took;
 *   - only K's own dependence on theta is differentiated.
 * The mean over the n_traj trajectories is an unbiased estimate of the gradient the density-matrix sweeps return.  No
 * separate score-function term is needed: it is inside the 1 / sqrt(w_d).
 *
 * THE SWEEP, per trajectory (one workgroup of 256 threads; work items (sample, slot) as in the forward):
 *   replay     THE TRAJECTORY RULE of qiddm_hip_traj.h unchanged -- the same Philox words from (seed, offset, absolute row,
 *              t, d), the same reductions and roundings: the branches and psi_N are the forward's bit for bit.  In front of
 *              every channel op psi is copied to a snapshot in the workspace, with the applied 2 x 2 matrix (as rounded to
 *              the state's dtype), w_d, the strength and the branch in a record of 256 B behind it.
 *   seed       lambda_N = (sum_j g_j O_j) psi_N, g = the sample's row of grad_out: QIDDM_MEAS_PROBS g_k psi_k;
 *              QIDDM_MEAS_EXPZ (sum_w +-g_w) psi_k; QIDDM_MEAS_OBS sum_t g_col(t) p_t P_t psi_N with the sign and i^ny
 *              conventions of the forward's read-out.
 *   walk back  for op i with psi_i = A_i psi_{i-1}: the gradient of a real parameter theta of A_i is
 *              2 Re <lambda_i| dA_i/dtheta |psi_{i-1}>; then lambda_{i-1} = A_i^H lambda_i.  psi_{i-1} = A_i^H psi_i for
 *              PHASE (as RZ), RY, GATE, GATE2, CZ, CNOT; for a channel op it is the snapshot.
 * Gradients (layouts of qiddm_mixed_backward; every element is written, a parameter no op reads gets 0; ops that share a
 * row add):
 *   grad_rows (n_rows, batch)       angle rows of PHASE / RY times the op's `scale`; strengths of PHASE_DAMP, AMP_DAMP, DEPOL
 *                                   with a >= 0 times `scale`, with dK_k/ds of the chosen operator over sqrt(w_d):
 *                                   PHASE_DAMP / AMP_DAMP k = 0: diag(0, -1 / (2 sqrt(1-g))), k = 1: K_1 / (2 g);
 *                                   DEPOL k = 0: -1 / (2 (1-p)) times the identity, k >= 1: the Pauli times 1 / (2 p).
 *                                   g = 1 is not special-cased.
 *   grad_gates (batch, n_gates, 8)  GATE / GATE2 rows, entries as independent reals: dL/dRe A_ab = 2 Re sum conj(lambda_a)
 *                                   psi_b, dL/dIm A_ab = -2 Im sum conj(lambda_a) psi_b over the wire's pairs / quadruples
 *                                   (psi = psi_{i-1}).  KRAUS: row a + k_d gets that times 1 / sqrt(w_d), the op's other rows
 *                                   get zero in that trajectory.  KRAUS2 (QIDDM_MIX_KRAUS2, qiddm_hip_traj.h): rows
 *                                   a + 4 k_d .. a + 4 k_d + 3 get GATE2's entry gradients times 1 / sqrt(w_d) -- with W_rc =
 *                                   sum over the quadruples of conj(lambda_r) psi_{i-1,c}, dL/dRe A_rc = 2 Re W_rc and
 *                                   dL/dIm A_rc = -2 Im W_rc -- and the op's other operators zero in that trajectory.
 *                                   The op is replayed with a snapshot in front of it like every channel op; its record
 *                                   keeps the branch and w_d alone, and the walk back rebuilds the applied 4 x 4 matrix
 *                                   K_k / sqrt(w_d) from them and the gate rows by the forward's code (the same rounding),
 *                                   takes psi_{i-1} from the snapshot and sets lambda <- A^H lambda.  The record stays
 *                                   256 B: both workspace sizes are what they are with a KRAUS op in its place.
 *   grad_features (batch, n_features)  AMP_EMBED as op 0: with g = 2 Re lambda_0 and psi_0 = v / |v|,
 *                                   dL/dv = (g - (g . psi_0) psi_0) / |v|.  Read only when the program embeds.
 * A trajectory whose forward stopped (W not positive or not finite) gives NaN in every gradient of its sample.
 * THE MEAN does not depend on the grid: a trajectory's gradient is collected in a float64 row (n_rows + 8 n_gates + n_features
 * wide; n_features counts only when the program embeds), the rows of (sample, slot) are added in ascending t (the first
 * stored), a second kernel adds the S = min(n_traj, 64) slots in ascending order from 0.0 and divides by n_traj.  Every sum
 * over psi: float64 partials in ascending index, a wave butterfly, four partials in wave order.  No atomics: reruns and a
 * lowered max_blocks give the same bits.
 * psi and lambda live in LDS while 2 * 2^n elements fit in 128 KiB (n <= 13 in float32, n <= 12 in float64), else in two
 * slabs per workgroup in the workspace.
 * Arguments: those of qiddm_mixed_traj_forward up to `max_blocks`, then
 *   grad_out, gout_ld     (batch, gout_ld >= width) float64 DEVICE
 *   grad_rows, grad_gates, grad_features   as above, float64 DEVICE
 *   per_traj_grad  (batch, n_traj, n_rows + 8 n_gates + n_features) float64 DEVICE or NULL: every trajectory's own row
 *   branches       (batch, n_traj, n_channels) int32 DEVICE or NULL: as the forward's.  Both cost nothing when NULL.
 *                  (A program without any parameter -- a gradient row of width 0 -- launches nothing, unless `branches`
 *                  is given: then the sweep runs for its sake.)
 *   max_blocks     0: the default -- as many workgroups as keep the snapshots of the launch within 1 GiB, at least one,
 *                  at most 2048 with psi and lambda in LDS and 256 otherwise.  A lower cap changes only the time.
 * Checks: those of qiddm_mixed_traj_forward, in its order and words, up to max_blocks (refused for an empty batch as well;
 * batch == 0 then returns QIDDM_OK); then QIDDM_ERR_UNSUPPORTED for a state preparation after op 0 (`op %d: a state
 * preparation after op 0 has no reverse sweep on trajectories`), the gate-row overlap refusal of qiddm_mixed_backward
 * (`op %d: gate rows %d..%d overlap those of op %d`; here a KRAUS op counts with its m rows a .. a+m-1 and a KRAUS2 op with
 * its 4m rows a .. a+4m-1: the rows of two ops that get a gate-row gradient -- GATE, GATE2, KRAUS, KRAUS2 -- are the same rows, whose gradients add, or share none), grad_out / gout_ld and the gradient pointers in its words, then the
 * workspace (`workspace of %lld B needed (qiddm_mixed_traj_backward_workspace_bytes)`).
 *   qiddm_mixed_traj_backward_workspace_bytes  host only; reads the program to count its channel ops C and whether it
 *       embeds.  With W = n_rows + 8 n_gates + (embeds ? n_features : 0), E = 2^n elements of 8 B (float32) / 16 B (float64),
 *       S = min(n_traj, 64) and G the workgroups of the launch (max_blocks as it will be passed):
 *         program head + batch * S * W float64 + G * W float64 + G * C * (E + 256 B) + (psi, lambda outside LDS) G * 2 E,
 *       every term rounded up to 256 B.  G = min(batch * S, 2048 | 256, max(1, 1 GiB / (C * (E + 256 B))), max_blocks).    */
int64_t qiddm_mixed_traj_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj,
                                                  const qiddm_mixed_op_t *program, int32_t n_ops, int32_t n_rows,
                                                  int32_t n_gates, int32_t n_features, int32_t max_blocks);
int qiddm_mixed_traj_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                              const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                              int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                              const double *gates, int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj,
                              double seed, double offset, int32_t max_blocks, const double *grad_out, int64_t gout_ld,
                              double *grad_rows, double *grad_gates, double *grad_features, double *per_traj_grad,
                              int32_t *branches, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QIDDM_HIP_TRAJ_GRAD_H */

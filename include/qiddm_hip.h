/*
 * qiddm_hip.h -- C ABI of the MI355X (gfx950) statevector engine behind the
 * QIDDM quantum layers.
 *
 * The reference (aaai2026/QIDDM) has no FFI for this path: its boundary is the
 * Python call `self.qnode(inputs[, weights])` on a PennyLane QNode
 * (reference nn/qdense.py:26-38,58 ; :237-247,279 ; :406-420,465 ; :1586-1600,1633 ;
 * nn/qconv.py:39-47) whose arithmetic lives in the third-party simulators
 * PennyLane 0.29.0 `default.qubit.torch` / PennyLane-Lightning 0.30.0
 * `lightning.qubit` (reference requirements.txt:44-45).  This header is the
 * drop-in for that simulator: every entry point below is what a QNode
 * execution (forward, parameter-shift sweep, adjoint backward) binds to.  The
 * Python binding (ctypes) is qiddm_amd/_capi.py; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t
 *     passed as void* (NULL = the null stream).
 *   - every pointer except `circ` is a DEVICE pointer owned by the caller, who
 *     keeps it alive until the stream has been synchronised.  No allocation,
 *     no synchronisation and no host<->device copies happen inside any call,
 *     so every call is hipGraph-capturable, re-entrant and thread safe.
 *   - return value: QIDDM_OK (0) or a negative qiddm_status; a human readable
 *     reason is available from qiddm_last_error() (thread local).
 *   - wire w is bit (n-1-w) of the amplitude index (wire 0 = most significant),
 *     the order qml.probs(wires=range(n)) reports.
 *   - every `*_ld` (and `y_step_stride`) is a leading dimension counted in ELEMENTS of the operand's own
 *     type: row r of the operand starts `r * ld` elements behind its pointer.  `in_ld`, `g_ld`, `gin_ld` and
 *     `out_ld` of qiddm_forward count elements of circ->dtype; `out_ld` of qiddm_forward_post counts float64
 *     elements (its output is float64 whatever the circuit's dtype).  A leading dimension below the operand's
 *     width is refused with QIDDM_ERR_INVALID.  Rows need no alignment beyond that of one element, and the
 *     elements between the end of a row and the start of the next (the padding) are never read or written.
 *
 * Circuit family (covers every `_circuit` of reference nn/qdense.py and the
 * exported QConv2d of nn/qconv.py):
 *
 *   for round in 0..n_rounds-1:                 chained QNode calls, nn/qdense.py:464-465, 1631-1635
 *     state <- AmplitudeEmbedding(x + enc_offset, pad_with, normalize)   (QIDDM_ENC_AMPLITUDE)
 *              or |0...0>
 *     for block in 0..n_blocks-1:                data re-uploading, nn/qdense.py:424-428
 *       QIDDM_ENC_RZ : RZ(enc_scale * x_j) on every wire j
 *       QIDDM_ENC_RY : RY(enc_scale * x_j) on every wire j, block 0 only (qml.AngleEmbedding)
 *       QIDDM_ENC_RY_BLOCKS : the same RY layer in front of every block
 *       StronglyEntanglingLayers(angles[round][block] : (sel_layers, n, 3), imprimitive)
 *     out <- probs (B, 2^n)  |  <Z_i> (B, n)
 *     x   <- out[:, 0:n]     (input of the next round)
 *
 * Amplitude embedding, edge rows.  Every engine divides the padded row by its L2 norm, always: a row that already
 * has unit norm is divided by 1 and its grad_inputs carries the projection term of the normalisation (PennyLane
 * skips the division within 1e-10 of unit norm, and its gradient then has no such term; the outputs agree).
 * A row whose padded norm is zero (all features + enc_offset zero and nothing padded, or pad_with = 0; PennyLane
 * raises for it) is not an error here: its output row and its grad_inputs row are NaN (0 * 1/sqrt(0)), no other
 * sample's output or grad_inputs row is affected, and the weight gradients, being sums over the batch, are NaN too.
 */
#ifndef QIDDM_HIP_H
#define QIDDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QIDDM_ABI_VERSION 2
#define QIDDM_MAX_QUBITS_FUSED 10 /* one wavefront owns the whole slab in registers */
#define QIDDM_MAX_QUBITS 16       /* 11..16: one workgroup per sample, tiled passes over a workspace slab */

typedef enum qiddm_status {
  QIDDM_OK = 0,
  QIDDM_ERR_INVALID = -1,     /* bad argument (null pointer, size, enum)            */
  QIDDM_ERR_UNSUPPORTED = -2, /* valid request this build cannot run (e.g. n > max)  */
  QIDDM_ERR_LAUNCH = -3       /* HIP reported a launch failure                       */
} qiddm_status;

typedef enum qiddm_encoding {
  QIDDM_ENC_NONE = 0,
  QIDDM_ENC_AMPLITUDE = 1, /* qml.AmplitudeEmbedding  (nn/qdense.py:41-43, nn/qconv.py:52-54) */
  QIDDM_ENC_RZ = 2,        /* qml.RZ(inputs[:, j], wires=j) (nn/qdense.py:253, 427, 1408)     */
  QIDDM_ENC_RY = 3,        /* qml.AngleEmbedding(rotation="Y"): once, before block 0 (nn/qdense.py:166-168) */
  QIDDM_ENC_RY_BLOCKS = 4  /* qml.RY(inputs[j], wires=j) re-uploaded in every block (nn/qdense.py:600-602) */
} qiddm_encoding;

typedef enum qiddm_imprimitive {
  QIDDM_IMP_CNOT = 0, /* StronglyEntanglingLayers default (nn/qdense.py:44-46)              */
  QIDDM_IMP_CZ = 1    /* imprimitive=qml.ops.CZ (nn/qdense.py:263, 428)                      */
} qiddm_imprimitive;

typedef enum qiddm_measure {
  QIDDM_MEAS_PROBS = 0, /* qml.probs(wires=range(n))                 (nn/qdense.py:47)       */
  QIDDM_MEAS_EXPZ = 1,  /* [qml.expval(qml.PauliZ(i)) for i in ...]  (nn/qdense.py:264)      */
  QIDDM_MEAS_OBS = 2,   /* density-matrix executor only: the Pauli-word table the program ends in (QIDDM_MIX_OBS) */
  QIDDM_MEAS_RHO = 8    /* density-matrix executor only: the reduced density matrix of the wires the program's last op keeps
                         * (QIDDM_MIX_RHO).  3 and 4 are deliberately no measures: they stay "unknown measure"; the pure-state
                         * entry points refuse 8 as they refuse QIDDM_MEAS_OBS */
} qiddm_measure;

typedef enum qiddm_dtype {
  QIDDM_F32 = 0, /* complex64 state, float I/O  (the production path)                        */
  QIDDM_F64 = 1  /* complex128 state, double I/O (the reference's own precision, F5)         */
} qiddm_dtype;

typedef struct qiddm_circuit {
  int32_t n_qubits;    /* 1 .. qiddm_max_qubits() (= 16)                                     */
  int32_t encoding;    /* qiddm_encoding                                                     */
  int32_t imprimitive; /* qiddm_imprimitive                                                  */
  int32_t measure;     /* qiddm_measure                                                      */
  int32_t n_rounds;    /* N >= 1                                                             */
  int32_t n_blocks;    /* L >= 1                                                             */
  int32_t sel_layers;  /* S >= 1  (ranges r_s = (s mod (n-1)) + 1 restart in every block)    */
  int32_t n_features;  /* columns of `inputs` that are read: <= 2^n (amplitude), >= n (RZ/RY) */
  int32_t dtype;       /* qiddm_dtype of inputs / outputs / gate table                       */
  int32_t reserved;    /* must be 0                                                          */
  double enc_scale;    /* multiplies the input angles (1.0; pi/2 in nn/qdense.py:2215)       */
  double enc_offset;   /* added to the features before amplitude embedding (nn/qconv.py:78)  */
  double pad_with;     /* amplitude-embedding pad constant (0.1 qdense, 0.5 qconv)           */
} qiddm_circuit_t;

/* ---- introspection ------------------------------------------------------- */
int qiddm_abi_version(void);
int qiddm_max_qubits(void);
const char *qiddm_last_error(void);

/* Diagnostics only (tools/stamp_*.py): a device buffer of n_words 64-bit words into which workgroup 0 of the
 * dense / quantum-convolution kernels writes s_memtime phase stamps (they serialise the kernel: never set it in a
 * timed run).  The pointer is checked (device memory, the words inside one allocation); NULL / 0 clears it.  There
 * is no environment-variable form: a stale value inherited from a shell would be a wild GPU write.          */
int qiddm_set_stamp_buffer(void *device_ptr, int64_t n_words);

/* number of Rot gates = n_rounds*n_blocks*sel_layers*n_qubits (= angles / 3)            */
int64_t qiddm_num_rot_gates(const qiddm_circuit_t *circ);
/* gate applications per sample per forward, counted as SURVEY.md section 8a             */
int64_t qiddm_gate_count(const qiddm_circuit_t *circ);
/* elements (of circ->dtype) in the gate table qiddm_prepare_gates writes:
 * num_rot_gates * 7 variants * 8 reals, plus (n <= 10) the folded per-layer tables the forward of a
 * CZ circuit runs on: per layer n (cos, sin)(theta/2) pairs and 2^min(n,6) + 2^max(n-6,0) phases
 * exp(i sum +-(phi^l + omega^(l-1))/2) -- RZ(phi) RZ(omega) and the CZ ring between two RY layers
 * are one diagonal; for n = 11..16 CZ circuits with no / RZ encoding, per layer and wire the pairs
 * (cos, sin)(theta/2) and (cos, sin)((phi^l + omega^(l-1))/2) the pass-structured kernels run on      */
int64_t qiddm_gate_table_elems(const qiddm_circuit_t *circ);
/* replicas of a full parameter-shift sweep: 6*num_rot_gates (+ 2*n_blocks*n for the
 * input angles of RZ/RY encodings)                                                       */
int64_t qiddm_num_shift_replicas(const qiddm_circuit_t *circ, int with_inputs);
/* bytes of device workspace qiddm_forward (n_replicas = 0) / qiddm_forward_shifted need for this
 * circuit and batch: 0 for n <= 10 (register-resident slabs); for n = 11..16 2^n-amplitude slabs for
 * the concurrently resident workgroups (up to 1024: the sweeps of a 16-qubit shard are HBM traffic).  */
int64_t qiddm_workspace_bytes(const qiddm_circuit_t *circ, int64_t batch, int64_t n_replicas);

/* ---- gate table ----------------------------------------------------------
 * angles: (n_rounds, n_blocks, sel_layers, n, 3) float64, the weights tensor of
 * StronglyEntanglingLayers AFTER any host-side map (qw_map.tanh, torch.tanh).
 * Writes for every Rot gate the 2x2 matrix RZ(omega) RY(theta) RZ(phi) (variant 0)
 * and its six +-pi/2 parameter shifts (variants 1..6 = phi+,phi-,theta+,theta-,
 * omega+,omega-), evaluated in float64 and rounded once to circ->dtype.
 * Replaces qml.StronglyEntanglingLayers' decomposition into qml.Rot
 * [PennyLane 0.29.0 templates/layers/strongly_entangling.py].                            */
int qiddm_prepare_gates(const qiddm_circuit_t *circ, const double *angles, void *gate_table,
                        void *stream);

/* ---- forward ----------------------------------------------------------------
 * Replaces one (n_rounds == 1) or N chained QNode executions
 * `self.qnode(inputs, weights)` -> default.qubit.torch / lightning.qubit
 * (reference nn/qdense.py:58, 279, 465, 1439, 1633).
 * inputs: (batch, in_ld) row-major, first n_features columns read (may be NULL
 *         for QIDDM_ENC_NONE).  out: (batch, out_ld) rows of 2^n probabilities or
 *         n expectation values.  n <= 10: one wavefront owns one sample's slab in
 *         registers for the whole circuit.  n = 11..16: one workgroup per sample, slab in
 *         `workspace` (>= qiddm_workspace_bytes(circ, batch, 0) bytes; may be NULL for
 *         n <= 10), tiled passes (qiddm_amd/csrc/qsim_tiled.h).                            */
int qiddm_forward(const qiddm_circuit_t *circ, const void *inputs, int64_t batch, int64_t in_ld,
                  const void *gate_table, void *out, int64_t out_ld, void *workspace,
                  int64_t workspace_bytes, void *stream);

/* ---- parameter-shift sweep ---------------------------------------------------
 * Replaces PennyLane's diff_method="parameter-shift" executions configured at
 * reference nn/qdense.py:246, 1400, 1596: re-invokes the forward kernel for
 * replicas [first_replica, first_replica + n_replicas) of the shift schedule and
 * contracts each replica's output with the upstream gradient on the fly:
 *     dots[r - first_replica][b] = sum_k grad_out[b][k] * out_r[b][k]
 * Replica ids: 6*g + v (v = 0..5 -> phi+,phi-,theta+,theta-,omega+,omega-) for Rot
 * gate g, then 6*G_rot + 2*(block*n + wire) + (0:+, 1:-) for the input angle of
 * `wire` re-uploaded in `block`.  d/dtheta = (dots[+] - dots[-]) / 2 summed over
 * the batch (weights) or per sample (inputs; times enc_scale).  n_rounds must be 1.      */
/* The same forward for the PROBABILITY nets with their `_post_process` fused into the store (reference
 * nn/qdense.py:49-54, 443-448: `clamp(probs[:, :pixels] * pixels, 0, 1)` on the float64 the QNode returns):
 * out (batch, post_cols) float64 = clamp((double)p[:, :post_cols] * post_scale, 0, 1) -- bit-identical to converting the
 * probabilities to float64 first; the (batch, 2^n) matrix is never written.  measure = probs, n <= 10.           */
int qiddm_forward_post(const qiddm_circuit_t *circ, const void *inputs, int64_t batch, int64_t in_ld,
                       const void *gate_table, double *out, int64_t out_ld, int32_t post_cols, double post_scale,
                       void *stream);

int qiddm_forward_shifted(const qiddm_circuit_t *circ, const void *inputs, int64_t batch,
                          int64_t in_ld, const void *gate_table, const void *grad_out,
                          int64_t g_ld, int64_t first_replica, int64_t n_replicas, void *dots,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* ---- adjoint (reverse-mode) backward ----------------------------------------------------
 * Replaces what diff_method="backprop" computes in the reference (torch autograd through
 * default.qubit.torch, nn/qdense.py:37, 419; nn/qconv.py:46) for ONE QNode round (n_rounds == 1,
 * n_qubits <= 10):  given grad_out = dL/d(out) of qiddm_forward it returns
 *   k_partials : (n_partials, n_rot, 8) of circ->dtype -- per-workgroup partial sums over the batch of
 *                K_{ab} = sum conj(lambda_a) psi_b for every Rot gate (a,b in {0,1}, as re/im pairs in the
 *                order K00 K01 K10 K11); the caller sums them over dim 0 and contracts with the analytic
 *                dRot/d(phi,theta,omega):  dL/dangle = 2 Re sum_ab (dU/dangle)_ab K_ab.
 *                n_partials = qiddm_adjoint_partials(circ, batch).  For CZ circuits without RY data encoding and
 *                n <= 9 the slabs (same size) hold per-layer sums of d/dtheta and d/d(phi^l + omega^(l-1)) instead
 *                (folded reverse sweep): treat them as opaque and hand them to qiddm_adjoint_finalize.
 *   grad_inputs: (batch, gin_ld) dL/d(inputs): n columns for RZ / RY encodings, n_features columns for
 *                the amplitude embedding (gradient through pad + normalise); may be NULL.
 * Cost: about five forward passes, independent of the number of parameters.                     */
int64_t qiddm_adjoint_partials(const qiddm_circuit_t *circ, int64_t batch);
int qiddm_backward_adjoint(const qiddm_circuit_t *circ, const void *inputs, int64_t batch,
                           int64_t in_ld, const void *gate_table, const void *grad_out, int64_t g_ld,
                           void *k_partials, void *grad_inputs, int64_t gin_ld, void *stream);
/* n = 11..16: the same gradient with psi and lambda in a per-workgroup slab pair of `workspace`
 * (qiddm_adjoint_workspace_bytes; 0 for n <= 10).  CZ circuits with no / RZ encoding and >= 2 layers: the
 * pass-structured reverse sweep (one sweep of both slabs per LAYER; the slabs of k_partials then hold per-layer
 * angle-gradient sums: opaque, hand them to qiddm_adjoint_finalize); everything else: one sweep per gate, K slabs. */
int64_t qiddm_adjoint_workspace_bytes(const qiddm_circuit_t *circ, int64_t batch);
int qiddm_backward_adjoint_wide(const qiddm_circuit_t *circ, const void *inputs, int64_t batch,
                                int64_t in_ld, const void *gate_table, const void *grad_out, int64_t g_ld,
                                void *k_partials, void *grad_inputs, int64_t gin_ld, void *workspace,
                                int64_t workspace_bytes, void *stream);
/* Sums the n_partials K slabs (fixed order: deterministic) and contracts them with the analytic
 * dRot/d(phi, theta, omega) in float64: grad_angles (n_rot, 3) float64 = dL/d(angles).              */
int qiddm_adjoint_finalize(const qiddm_circuit_t *circ, const double *angles, const void *k_partials,
                           int64_t n_partials, double *grad_angles, void *stream);

/* ---- fused dense-net forward ------------------------------------------------------
 * Replaces the whole forward of the reference's linear_down -> quantum rounds -> linear_up
 * nets in one launch: QNN_noise.forward / QNN.forward (reference nn/qdense.py:267-289,
 * 346-368) and QIDDM_LL_noise.forward (:1620-1642), i.e.
 *     h   = x @ w_down^T + b_down                      (batch, n)        float64
 *     ev  = circuit(h)  (circ: QIDDM_ENC_RZ, QIDDM_MEAS_EXPZ, any n_rounds/n_blocks/sel_layers)
 *     net = ev @ w_up^T + b_up                         (batch, out_features)  float64
 * and, with post_mode = 1, the "noise"-goal update of the sampling loop on top of it
 * (reference src/models.py:130-134):  y = clamp(x - (net - 0.5) * 0.1 * noise_factor, 0, 1)
 * (post_mode = 0: y = net).  The classical glue runs in float64 as in the reference, the
 * statevector in circ->dtype.  `angles` is the raw (n_rounds, n_blocks, sel_layers, n, 3)
 * float64 weight tensor: the Rot matrices are built inside the launch (no gate table).
 * w_down: (n, in_features) row-major, w_up: (out_features, n) row-major (torch.nn.Linear
 * layout); b_down / b_up may be NULL.  y must not alias x.  post_mode = 1 needs
 * out_features == in_features.                                                           */
int qiddm_dense_forward(const qiddm_circuit_t *circ, const double *x, int64_t batch, int64_t x_ld,
                        int64_t in_features, const double *w_down, const double *b_down,
                        const double *angles, const double *w_up, const double *b_up,
                        int64_t out_features, int32_t post_mode, double noise_factor, double *y,
                        int64_t y_ld, void *stream);

/* ---- fused sampling loop -----------------------------------------------------------------
 * `n_steps` consecutive bodies of the reference's sampling loop (src/models.py:124-136)
 *     x <- net(x)                                        (post_mode 0, "data" goal)
 *     x <- clamp(x - (net(x) - 0.5) * 0.1 * noise_factor, 0, 1)   (post_mode 1, "noise" goal)
 * in ONE launch, net = linear_down -> circuit rounds -> linear_up as in qiddm_dense_forward.
 * y: (n_steps, batch, out_features) float64, y[s] = the image after step s+1 (row stride y_ld,
 * step stride y_step_stride).  n_steps > 1 needs out_features == in_features.  Four wavefronts own
 * one sample (qsim_quad.h): supported for 2 <= n_qubits <= 10 (below 8 every wavefront runs the circuit on its own copy of the state), QIDDM_IMP_CZ, QIDDM_ENC_RZ,
 * QIDDM_MEAS_EXPZ, features <= 2048; anything else returns QIDDM_ERR_UNSUPPORTED (loop over
 * qiddm_dense_forward instead).                                                               */
int qiddm_dense_sample(const qiddm_circuit_t *circ, const double *x, int64_t batch, int64_t x_ld,
                       int64_t in_features, const double *w_down, const double *b_down,
                       const double *angles, const double *w_up, const double *b_up,
                       int64_t out_features, int32_t post_mode, double noise_factor, int32_t n_steps,
                       double *y, int64_t y_ld, int64_t y_step_stride, const void *tables, void *stream);
/* The sampler runs on per-layer tables derived from `angles` (RY coefficients, folded RZ/CZ phases).  With
 * tables == NULL every launch rebuilds them in LDS; a caller that samples many times with the same weights
 * builds them once: qiddm_dense_sample_prepare writes qiddm_dense_sample_tables_bytes(circ) bytes (circ->dtype)
 * that stay valid until the angles change.                                                              */
int64_t qiddm_dense_sample_tables_bytes(const qiddm_circuit_t *circ);
int qiddm_dense_sample_prepare(const qiddm_circuit_t *circ, const double *angles, void *tables, void *stream);

/* ---- lean sampling loop of the 8- and 6-qubit dense nets (qsim_lean.h) --------------------------------------------
 * The same n_steps bodies of Diffusion.sample (post_mode / noise_factor as for qiddm_dense_sample, reference
 * src/models.py:127-134) on 8 or 6 wires / CZ rings / RZ encoding / <Z>, with every RY in tangent form (one fused
 * cross-lane multiply-add per gate).  post_mode 0 ("data" goal, x <- net(x)): linear_down is composed with linear_up
 * into an n x n map of the previous step's <Z> (W_down is only read for the first step, and not at all when the circuit
 * has one block per round: the data angles are then a global phase).  post_mode 1 ("noise" goal): the clamp breaks that
 * composition; the image and both linears' weights stay in registers across the steps.  Tables: qiddm_dense_sample_lean_tables_bytes(circ) bytes, written once per
 * weights by _prepare (angles AND the two linears); _check synchronises the stream and returns 1 when the tables are
 * usable -- max |tan(theta/2)| <= 16 over the simulated layers -- 0 when the caller must use qiddm_dense_sample, < 0
 * on error.  Results agree with qiddm_dense_sample to rounding (not bit for bit).
 * For the instance without re-upload that has a kernel of its own (float32, 8 qubits, one block of 14 layers, one round)
 * the tables also carry the circuit's read-out, the eight <Z>: _prepare simulates the circuit once, on the same stream,
 * and the sampler executes no gate.  The read-out depends on the angles alone, so the tables are valid exactly as long
 * as the angles are -- the "once per weights" above, nothing new; _check returns 0 for such a circuit when the tables
 * carry no finite read-out for it.  w_up / b_up remain operands of every qiddm_dense_sample_lean call: the row is
 * computed from the pointers of that call.                                                                          */
int64_t qiddm_dense_sample_lean_tables_bytes(const qiddm_circuit_t *circ);
int qiddm_dense_sample_lean_prepare(const qiddm_circuit_t *circ, const double *angles, const double *w_down,
                                    const double *b_down, const double *w_up, const double *b_up, int64_t features,
                                    void *tables, void *stream);
int qiddm_dense_sample_lean_check(const qiddm_circuit_t *circ, const void *tables, void *stream);
int qiddm_dense_sample_lean(const qiddm_circuit_t *circ, const double *x, int64_t batch, int64_t x_ld,
                            int64_t features, const double *w_down, const double *b_down, const double *w_up,
                            const double *b_up, int32_t post_mode, double noise_factor, int32_t n_steps, double *y,
                            int64_t y_ld, int64_t y_step_stride, const void *tables, void *stream);

/* ---- fused quantum convolution -------------------------------------------------------
 * Replaces the (intended, SURVEY finding F3) forward of the reference's exported QConv2d
 * (`_QConv2d_FAST`, nn/qconv.py:51-87) in one launch:
 *     torch.nn.Unfold(kernel, padding) -> + enc_offset (0.1) -> AmplitudeEmbedding(pad_with 0.5,
 *     normalize) -> StronglyEntanglingLayers(angles, CNOT) -> probs -> * 2^n / 2 -> clamp [0,1] ->
 *     [:, ::2][:, :out_channels] -> (batch, out_channels, H_out, W_out)
 * x: (batch, in_channels, H, W) float64 contiguous; y: (batch, out_channels, H_out, W_out) float64
 * with H_out = H + 2*pad_h - kh + 1.  circ: QIDDM_ENC_AMPLITUDE, QIDDM_MEAS_PROBS, n_rounds =
 * n_blocks = 1, n_features = in_channels*kh*kw, n_qubits <= 10.  `angles` is the (1,1,S,n,3) float64
 * tensor AFTER the qw_map.tanh map.  out_channels beyond 2^n / 2 do not exist (the reference's slice
 * silently returns fewer channels): they are rejected here.                                  */
int qiddm_qconv_forward(const qiddm_circuit_t *circ, const double *x, int64_t batch,
                        int64_t in_channels, int64_t height, int64_t width, int64_t kh, int64_t kw,
                        int64_t pad_h, int64_t pad_w, const double *angles, int64_t out_channels,
                        double *y, void *stream);

/* Backward of qiddm_qconv_forward in two launches (replaces torch autograd through Unfold, default.qubit.torch
 * and the post-processing slices, reference nn/qconv.py:46, 58-87 with diff_method="backprop"): the adjoint
 * sweep runs one circuit per output pixel with the patch read from x and dL/dp read from grad_y
 * (B, out_channels, H_out, W_out) through the clamp / [::2] / [:out_channels] chain, never materialising the
 * (B H_out W_out, 2^n) probability gradient; then the per-pixel feature gradients are folded back onto the image.
 *   gate_table : qiddm_prepare_gates of the (1,1,S,n,3) angles (after the tanh map), circ->dtype
 *   k_partials : (qiddm_adjoint_partials(circ, batch*H_out*W_out), n_rot, 8) circ->dtype -> qiddm_adjoint_finalize
 *   grad_features : scratch (batch*H_out*W_out, in_channels*kh*kw) circ->dtype; grad_x: (batch, C, H, W) float64.
 *                   Both NULL when the input needs no gradient.
 * n_qubits <= 10.                                                                                          */
int qiddm_qconv_backward(const qiddm_circuit_t *circ, const double *x, int64_t batch, int64_t in_channels,
                         int64_t height, int64_t width, int64_t kh, int64_t kw, int64_t pad_h, int64_t pad_w,
                         const void *gate_table, const double *grad_y, int64_t out_channels, void *k_partials,
                         void *grad_features, double *grad_x, void *stream);

/* ---- fused training step (device-resident Diffusion step) ---------------------------------
 * Replaces, for nets of the linear_down -> circuit -> linear_up family (QNN_noise nn/qdense.py:267-289,
 * QIDDM_LL_noise :1620-1642), one call of Diffusion.run_training_step_data / _noise
 * (src/models.py:44-72 / :74-104) including its internal .backward(), with
 * add_normal_noise_multiple (src/noise.py:105-126) as the noising schedule:
 *     whole = x*(1-w_t) + noise*w_t, clamp      t = 0..tau        (never materialised)
 *     noisy = whole[:, 1:], clean = whole[:, :-1]                 rows i = b*tau + (t-1)
 *     out   = W_up <Z>(circuit(W_down noisy + b_down)) + b_up
 *     goal 0 ("data"):  loss = mean((out - clean)^2)
 *     goal 1 ("noise"): loss = mean(((out - 0.5)*0.1 - (noisy - clean))^2)
 * Outputs: the scalar loss and d loss / d parameter for every parameter (overwritten, not accumulated).
 * train_quantum = 0 reproduces the reference as written (SURVEY finding F1: the circuit output is
 * detached, only linear_up receives a gradient; g_w_down/g_b_down/g_angles are not touched);
 * train_quantum = 1 differentiates the circuit by the adjoint method (what diff_method="backprop"
 * yields in the reference).  recon / elem_loss (optional, (batch*tau, pixels)) are what the verbose call
 * returns: the reconstruction (goal 1: clamp(noisy - predicted, 0, 1)) and the element-wise loss.
 * circ: QIDDM_MEAS_EXPZ, any angle encoding or none, n_qubits <= 10, any n_rounds.
 * schedule: (tau+1) float32 weights with schedule[0] = 0; noise: float32 as the reference draws it.
 * All sums have a fixed order: bit-reproducible.  Three launches on `stream`, no host synchronisation. */
typedef struct qiddm_train_args {
  const double *x;        /* (batch, pixels) float64, row stride x_ld                      */
  float *noise;           /* (batch, pixels) float32, row stride noise_ld: the N(0.5, 0.2) field -- read,
                           * or, when rng_state != NULL, generated in the launch and written here        */
  const float *schedule;  /* (tau + 1)                                                     */
  int64_t x_ld, noise_ld, batch;
  int32_t pixels, tau, goal, train_quantum;
  const double *w_down, *b_down;   /* (n, pixels), (n) or NULL                              */
  const double *angles;            /* (n_rounds, n_blocks, sel_layers, n, 3)                */
  const double *w_up, *b_up;       /* (pixels, n), (pixels) or NULL                         */
  double *loss;                    /* (1)                                                   */
  double *g_w_down, *g_b_down, *g_angles, *g_w_up, *g_b_up;
  double *recon, *elem_loss;       /* optional                                              */
  uint64_t *rng_state;             /* optional: device {seed, offset}; Philox4x32-10 + Box-Muller per element,
                                    * offset advanced by one per call (graph-replayable)                 */
} qiddm_train_args_t;

/* bytes of scratch qiddm_train_step needs (negative: error code) */
int64_t qiddm_train_workspace_bytes(const qiddm_circuit_t *circ, int64_t batch, int32_t pixels, int32_t tau);
int qiddm_train_step(const qiddm_circuit_t *circ, const qiddm_train_args_t *args, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* ---- Adam for every parameter tensor in one launch ------------------------------------------------
 * torch.optim.Adam as the reference harness constructs it (src/mnist_exm.py:170; betas, eps, weight_decay
 * passed explicitly; no amsgrad, no maximize):
 *     step += 1;  g += weight_decay * p;  m.lerp_(g, 1-beta1);  v = beta2 v + (1-beta2) g^2
 *     p -= lr / (1-beta1^step) * m / (sqrt(v) / sqrt(1-beta2^step) + eps)
 * step: per-tensor device int64 counter (torch keeps one per parameter; read, then advanced by one at the
 * end of the call); sync: device uint32 scratch, zero before the first call, left zero.  dtype per tensor QIDDM_F32/QIDDM_F64
 * (grad and moments have the parameter's dtype; the arithmetic is float64).  Safe to record into a HIP graph. */
typedef struct qiddm_adam_tensor {
  void *param;
  const void *grad;
  void *exp_avg, *exp_avg_sq;
  int64_t *step;
  int64_t numel;
  int32_t dtype, reserved;
} qiddm_adam_tensor_t;
int qiddm_adam_step(const qiddm_adam_tensor_t *tensors, int32_t n_tensors, double lr, double beta1,
                    double beta2, double eps, double weight_decay, uint32_t *sync, void *stream);

/* ---- eval-mode quantum convolution: circuit unitary + GEMM on the matrix cores ------------------------
 * Reference nn/qconv.py:92-126: `_QConv2d_FAST.train(False)` caches `sample_matrix = qml.matrix(SEL(pi*tanh(w)))`
 * and evaluates AmplitudeEmbedding -> QubitUnitary(sample_matrix) -> probs.
 *
 * qiddm_circuit_unitary: u (D, D) complex float64, row-major, interleaved (re, im): u[k][j] = <k|U|j> for the
 * weight-only circuit StronglyEntanglingLayers(angles (1,1,S,n,3), imprimitive) -- circ->encoding / measure
 * are ignored; n_rounds = n_blocks = 1, n_qubits <= 10.  Wire 0 is the most significant bit of k and j
 * (qml.matrix(..., wire_order=range(n))).
 *
 * qiddm_qconv_unitary_forward: the same function of (x, weights) as qiddm_qconv_forward, computed as the
 * implicit-im2col GEMM  (batch Ho Wo) x (C kh kw)  times  (C kh kw) x 2 C_out  on v_mfma_f32_32x32x2_f32
 * (float32 products and sums) with the normalise / |.|^2 / scale / clamp epilogue; x, y float64 as there.
 * workspace: qiddm_qconv_unitary_workspace_bytes (packed operand; rewritten by every call).
 * Two neighbours of the convolution in `unet_simple` (reference nn/unet_simple.py:9-18, 40-49) can ride along:
 *   upsample2x != 0: x is (batch, C, height, width) and the convolution reads its
 *       torch.nn.Upsample(scale_factor=2, mode="bilinear") (align_corners=False) -- the `up_conv` pair;
 *   bn != NULL: eval-mode BatchNorm2d on the output, (y - running_mean) / sqrt(running_var + eps) * weight + bias
 *       (weight / bias may be NULL) -- the [QConv2d, BatchNorm2d] pair.                                */
typedef struct qiddm_batchnorm {
  const double *weight, *bias, *running_mean, *running_var; /* (out_channels) each */
  double eps;
} qiddm_batchnorm_t;
int qiddm_circuit_unitary(const qiddm_circuit_t *circ, const double *angles, double *u, void *stream);
/* n <= 12 (C4's 12-qubit layers): writes the TRANSPOSE, ut[j][k] = <k|U|j> (each column of U contiguous: the
 * workgroup of column j evolves |j> in place in row j, no workspace).  Pass u_transposed = 1 below.          */
int qiddm_circuit_unitary_wide(const qiddm_circuit_t *circ, const double *angles, double *ut, void *stream);
/* The forward first packs the rows of u it needs (and the folded BatchNorm) into `workspace`.  u == NULL skips that launch:
 * `workspace` must then still hold the packing of an earlier call for the same unitary, batch norm and geometry -- an
 * eval-mode layer whose weights have not changed keeps its own workspace and packs once.                          */
int64_t qiddm_qconv_unitary_workspace_bytes(int32_t n_qubits, int64_t in_channels, int64_t kh, int64_t kw,
                                            int64_t out_channels);
int qiddm_qconv_unitary_forward(int32_t n_qubits, const double *u, const double *x, int64_t batch,
                                int64_t in_channels, int64_t height, int64_t width, int64_t kh, int64_t kw,
                                int64_t pad_h, int64_t pad_w, int64_t out_channels, int32_t upsample2x,
                                const qiddm_batchnorm_t *bn, int32_t u_transposed, double *y, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---- training-mode BatchNorm2d, float64 NCHW ------------------------------------------------------------
 * The `torch.nn.BatchNorm2d` behind every quantum convolution of `unet_simple` (reference
 * nn/unet_simple.py:9-18, 30-39) in training mode: per-channel batch statistics (biased variance for the
 * transform, unbiased for the running estimate), running_mean / running_var moved by `momentum` in place
 * (either may be NULL), y = (x - mean) / sqrt(var + eps) * weight + bias (weight / bias may be NULL).
 * save_mean / save_invstd (channels) feed the backward: grad_x (may be NULL), grad_weight, grad_bias (may be
 * NULL).  x: (batch, channels, hw).  Two launches per direction, sums in a fixed order (deterministic).
 * workspace: qiddm_batchnorm_workspace_bytes, rewritten by every call.                                     */
int64_t qiddm_batchnorm_workspace_bytes(int64_t batch, int64_t channels, int64_t hw);
int qiddm_batchnorm_train_forward(const double *x, int64_t batch, int64_t channels, int64_t hw,
                                  const double *weight, const double *bias, double *running_mean,
                                  double *running_var, double momentum, double eps, double *y, double *save_mean,
                                  double *save_invstd, void *workspace, int64_t workspace_bytes, void *stream);
/* the statistics half of the backward only: grad_weight / grad_bias (each may be NULL) and coef (3, channels) with
 * dL/dx = coef[0][c] grad_y + coef[1][c] x + coef[2][c] -- for a producer that applies it itself
 * (qiddm_qconv_train_backward, conv_y / bn_coef).  Same workspace as qiddm_batchnorm_backward.               */
int qiddm_batchnorm_backward_stats(const double *x, const double *grad_y, int64_t batch, int64_t channels, int64_t hw,
                                   const double *weight, const double *save_mean, const double *save_invstd,
                                   double *grad_weight, double *grad_bias, double *coef, void *workspace,
                                   int64_t workspace_bytes, void *stream);
int qiddm_batchnorm_backward(const double *x, const double *grad_y, int64_t batch, int64_t channels, int64_t hw,
                             const double *weight, const double *save_mean, const double *save_invstd,
                             double *grad_x, double *grad_weight, double *grad_bias, void *workspace,
                             int64_t workspace_bytes, void *stream);

/* ---- bilinear x2, float64 (planes, H, W) -> (planes, 2H, 2W) -------------------------------------------
 * torch.nn.Upsample(scale_factor=2, mode="bilinear") in front of every `up_conv` (reference
 * nn/unet_simple.py:40-49) and its backward, for training (the eval route reads the x2 inside the GEMM).
 * ah (2H, H), aw (2W, W): the dense 1-D interpolation matrices (the caller derives them from torch's operator
 * applied to the identity, so the weights are torch's); forward y = ah x aw^T, backward grad_x = ah^T grad_y aw,
 * both as gathers over the <= 3 / 4 non-zero entries per row / column.                                      */
int qiddm_upsample2x_forward(const double *x, int64_t planes, int64_t height, int64_t width, const double *ah,
                             const double *aw, double *y, void *stream);
int qiddm_upsample2x_backward(const double *grad_y, int64_t planes, int64_t height, int64_t width,
                              const double *ah, const double *aw, double *grad_x, void *stream);

/* ---- the dense unitary route (A4 nets at inference) ----------------------------------------------------------------------
 * AmplitudeEmbedding -> weight-only layers -> probs (reference nn/qdense.py:40-47) does not depend on the data beyond the
 * embedded vector: with U = qiddm_circuit_unitary(weights), a batch is ONE real product  [Re a | Im a] = v^ [Re U^T | Im U^T]
 * (a plain library GEMM on the caller's side) between two elementwise kernels:
 *   qiddm_amp_embed_rows:  v (batch, 2^n) float32 = (x + offset | pad_with) / norm       (normalize=True)
 *   qiddm_prob_post:       out (batch, cols) float64 = clamp((Re^2 + Im^2) * scale, 0, 1) from (batch, 2 cols) float32
 * -- the move the reference itself makes for its eval-mode QConv2d (nn/qconv.py:96-113).                               */
int qiddm_amp_embed_rows(const double *x, int64_t batch, int64_t x_ld, int64_t features, int32_t n_qubits, double pad_with,
                         double offset, float *v, void *stream);
int qiddm_prob_post(const float *amplitudes, int64_t batch, int64_t cols, double scale, double *out, void *stream);

/* MaxPool2d(kernel_size=2, stride=2) of the UNets' down blocks (reference nn/unet.py:93-95), float64 (planes, H, W) ->
 * (planes, H/2, W/2), floor mode.  The backward recomputes the winner of every window from x (first maximum in row-major
 * order, as torch picks it) instead of keeping an index tensor and writes every element of grad_x once.         */
int qiddm_maxpool2_forward(const double *x, int64_t planes, int64_t height, int64_t width, double *y, void *stream);
int qiddm_maxpool2_backward(const double *x, const double *grad_y, int64_t planes, int64_t height, int64_t width,
                            double *grad_x, void *stream);

/* ---- quantum convolution backward through the circuit unitary (training) ----------------------------------
 * The circuit of QConv2d does not depend on the data (reference nn/qconv.py:51-56), so with U = U(weights):
 * a_mc = sum_j U[2c,j] v^_mj, y_mc = clamp(|a_mc|^2 D/2) for every output pixel m -- and the backward needs no
 * per-pixel circuit sweep:  with t_mc = dL/dy_mc D/2 where the clamp passes,
 *     dL/dv^_mj = 2 Re sum_c t_mc conj(a_mc) U[2c,j]   -> through the normalisation and the fold -> grad_x
 *     dL/dangle = 2 Re sum_c <e_2c| dU/dangle |h_c>,   h_c[j] = sum_m t_mc conj(a_mc) v^_mj
 * qiddm_qconv_train_backward computes a, dL/dv and partial sums of h:  h_partials (plan.n_partials, 2 row_channels,
 * C kh kw + 1) float32 with  h_c[j] = sum_p hp[p][c][j] - i sum_p hp[p][row_channels + c][j];  column C kh kw is the
 * value every pad column j >= C kh kw shares.
 *   rows: (C kh kw + 1, 2 row_channels) float32 -- rows[j][c] = Re U[2c,j], rows[j][row_channels + c] = Im U[2c,j],
 *         last row 0.5 sum_{j >= C kh kw} U[2c,j]; zero for c >= out_channels.
 * qiddm_matrix_adjoint: K slabs (-> qiddm_adjoint_finalize) of 2 Re <lambda_s| dU/dangle |psi0_s> summed over
 * `count` (psi0, lambda) pairs of complex128 vectors (count, 2^n, interleaved); circ->dtype QIDDM_F64, gate table
 * of that dtype, 2 <= n_qubits <= 16.
 *
 * One descriptor names the layer, qiddm_qconv_train_plan (host only) says what the library does with it, and
 * qiddm_qconv_train_backward launches exactly that:
 *   route         THIN: the hand-written thin-product kernels (<= 32 output channels, kernel extent <= 15, LDS tiles
 *                 that fit); GEMM: the unitary route holds (2 <= n_qubits <= 12, C kh kw <= 2^n, 2 out_channels <= 2^n)
 *                 but the layer is too wide for them -- the caller forms the products with library GEMMs and uses
 *                 qiddm_qconv_fold_features; NONE: no unitary route.  route and row_channels depend on (n_qubits,
 *                 in_channels, kh, kw, out_channels) only (one exception: a THIN layer whose C H W reaches 2^24 has no
 *                 plan at all, see below); on GEMM and NONE every other field is 0.
 *   row_channels  8, 16 or 32: the narrowest that holds out_channels (0 beyond 32); the width of `rows` / h_partials
 *   matrix_core   the three products run on the f32 matrix cores (v_mfma_f32_16x16x4_f32 / 32x32x2_f32: from 32 patch
 *                 features on, numel(x) and numel(grad_y) below 2^32), otherwise on the VALU kernel
 *   bn_fold       the kernel can apply a following training-mode BatchNorm2d's backward transform to dL/dy while it
 *                 loads it (0: the matrix-core kernel with 32 row channels has no registers left for it)
 *   pixel_rows_elems  > 0: dL/dx can come from 2 row_channels + 1 floats per output pixel and a transposed convolution
 *                 on the matrix cores (qsim_qconv_dx.h; same-size convolutions on the matrix-core kernel with at most
 *                 32 input channels) -- C kh kw / (2 row_channels + 1) times less memory traffic than the (C kh kw, M)
 *                 feature gradients + fold, and equal to them to float32 rounding (the taps are summed in float32)
 * A descriptor with an extent below 1, negative padding, a kernel larger than the padded image or 2^40 output pixels is
 * QIDDM_ERR_INVALID, and a THIN layer whose C H W reaches 2^24 QIDDM_ERR_UNSUPPORTED, from both functions alike.
 * The entry takes a THIN layer (anything else: QIDDM_ERR_UNSUPPORTED); x, grad_y, rows and h_partials are required.
 *   argument              means                                             needs
 *   x_is_f32              x is a float32 copy of the activations (same      plan.matrix_core; neither conv_y / bn_coef
 *                         results: every patch element is converted anyway) nor pixel_rows (QIDDM_ERR_UNSUPPORTED)
 *   grad_y_batch_stride   elements between two images of grad_y, 0 = dense  >= out_channels Ho Wo, batch * stride < 2^32
 *                         (a channel slice of a wider tensor read in place) (every route)
 *   conv_y, bn_coef       grad_y is dL/d(BatchNorm output): dL/dy = coef[0] both or neither; plan.bn_fold
 *                         grad_y + coef[1] conv_y + coef[2] per channel
 *                         (bn_coef: qiddm_batchnorm_backward_stats; conv_y is always the dense (batch, out_channels,
 *                         Ho, Wo) tensor: grad_y_batch_stride applies to grad_y alone)
 *   pixel_rows            (plan.pixel_rows_elems floats) dL/dx from the     grad_x, plan.pixel_rows_elems > 0, float64 x;
 *                         per-pixel rows; grad_features_t is not touched    otherwise grad_features_t is required
 *   grad_features_t       (C kh kw, M) float32 feature gradients, folded    --
 *                         into grad_x unless grad_x is NULL                                                        */
#define QIDDM_QCONV_ROUTE_NONE 0
#define QIDDM_QCONV_ROUTE_THIN 1
#define QIDDM_QCONV_ROUTE_GEMM 2
typedef struct {
  int32_t n_qubits, reserved;
  int64_t batch, in_channels, height, width, kh, kw, pad_h, pad_w, out_channels;
} qiddm_qconv_layer_t;
typedef struct {
  int32_t route;            /* QIDDM_QCONV_ROUTE_NONE / _THIN / _GEMM                                 */
  int32_t row_channels;     /* 8, 16, 32 (0: more than 32 output channels)                            */
  int32_t matrix_core;      /* thin-product kernel on the MFMA units; float32 x is accepted iff 1     */
  int32_t bn_fold;          /* the entry accepts conv_y / bn_coef                                     */
  int64_t n_partials;       /* slabs of h_partials                                                    */
  int64_t pixel_rows_elems; /* > 0: dL/dx from per-pixel rows; 0: feature gradients + fold            */
} qiddm_qconv_train_plan_t;
int qiddm_qconv_train_plan(const qiddm_qconv_layer_t *layer, qiddm_qconv_train_plan_t *plan);
int qiddm_qconv_train_backward(const qiddm_qconv_layer_t *layer, const void *x, int32_t x_is_f32, const double *grad_y,
                               int64_t grad_y_batch_stride, const double *conv_y, const double *bn_coef,
                               const float *rows, float *grad_features_t, float *pixel_rows, float *h_partials,
                               double *grad_x, void *stream);
/* the two small steps either side: `rows` from the unitary (qiddm_circuit_unitary[_wide]; u_transposed as there),
 * and h_partials -> the (out_channels, 2^n) complex128 start vectors psi0 = h_c and lambda = e_2c of
 * qiddm_matrix_adjoint                                                                                        */
int qiddm_qconv_train_rows(int32_t n_qubits, const double *u, int32_t u_transposed, int64_t features,
                           int64_t out_channels, int32_t row_channels, float *rows, void *stream);
int qiddm_qconv_train_vectors(int32_t n_qubits, const float *h_partials, int64_t n_partials, int64_t features,
                              int64_t out_channels, int32_t row_channels, double *psi0, double *lambda, void *stream);
/* the fold on its own: grad_x (batch, C, H, W) float64 from transposed feature gradients (C kh kw, batch Ho Wo)
 * float32 -- the transpose of torch.nn.Unfold as a deterministic gather (layers too wide for the thin-product
 * kernel compute the feature gradients with library GEMMs, qiddm_amd/circuit.py)                              */
int qiddm_qconv_fold_features(const float *grad_features_t, int64_t batch, int64_t in_channels, int64_t height,
                              int64_t width, int64_t kh, int64_t kw, int64_t pad_h, int64_t pad_w, double *grad_x,
                              void *stream);
int64_t qiddm_matrix_adjoint_partials(int64_t count);
int64_t qiddm_matrix_adjoint_workspace_bytes(const qiddm_circuit_t *circ, int64_t count);
int qiddm_matrix_adjoint(const qiddm_circuit_t *circ, const double *psi0, const double *lambda, int64_t count,
                         const void *gate_table, void *k_partials, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* classical 1x1 convolution, float64 NCHW (the UNets' `final_conv`, reference nn/unet.py:160-166):
 * x (batch, in_channels, hw), weight (out_channels, in_channels), bias (out_channels) or NULL.          */
int qiddm_conv1x1_forward(const double *x, const double *weight, const double *bias, int64_t batch,
                          int64_t in_channels, int64_t out_channels, int64_t hw, double *y, void *stream);
/* backward of the ONE-output-channel head (torch autograd through `final_conv`, reference nn/unet.py:160-166, 177):
 * grad_x[b, c, p] = weight[c] grad_y[b, p], grad_weight[c] = sum grad_y x, grad_bias = sum grad_y -- one pass over x and
 * grad_y, per-workgroup partial sums (`partials`: qiddm_conv1x1_head_partials() x (in_channels + 1) float64) added in a
 * fixed order.  in_channels <= 32; grad_x / grad_weight / grad_bias may each be NULL.                            */
int64_t qiddm_conv1x1_head_partials(int64_t batch, int64_t hw);
int qiddm_conv1x1_head_backward(const double *x, const double *weight, const double *grad_y, int64_t batch,
                                int64_t in_channels, int64_t hw, double *grad_x, double *grad_weight,
                                double *grad_bias, double *partials, void *stream);

/* ---- density-matrix execution (hardware-noise study) ---------------------------------------------
 * Replaces PennyLane's `default.mixed` for the circuits the `*_noise.py` drivers run at sampling time
 * (src/mnist_noise.py:214-229; channels at nn/qdense.py:98-104, 255-261, 1410-1417).  The circuit is handed over
 * as a program of single-wire / two-wire ops (the caller expands templates and entangler rings); one workgroup
 * keeps one sample's rho (2^n x 2^n) in LDS or in `workspace`.  qiddm_mixed_forward / _backward take n_qubits <= 8;
 * qiddm_mixed_wide_forward / _backward (below) run the same programs at 7 <= n_qubits <= 10.  qiddm_mixed_backward gives the
 * exact gradient of sum(grad_out * out) by a reverse sweep over the same program (PennyLane differentiates such QNodes).
 *   QIDDM_MIX_ZERO            rho = |0..0><0..0|                      (a program starts with ZERO or AMP_EMBED)
 *   QIDDM_MIX_AMP_EMBED       AmplitudeEmbedding(features + enc_offset, pad_with, normalize)
 *   QIDDM_MIX_PHASE           RZ / PhaseShift on `wire`: angle = p + scale * angle_rows[a][sample] (a < 0: p only)
 *   QIDDM_MIX_RY              RY on `wire`, angle as above
 *   QIDDM_MIX_GATE            the 2x2 unitary gates[a] = (u00, u01, u10, u11) as (re, im) float64
 *   QIDDM_MIX_CZ / _CNOT      control `wire`, target `a`
 *   QIDDM_MIX_PHASE_DAMP / _AMP_DAMP / _DEPOL   PennyLane's PhaseDamping / AmplitudeDamping /
 *                             DepolarizingChannel on `wire`.  a < 0: the strength is `p`, checked to lie in [0, 1].
 *                             a >= 0: the strength of sample s is p + scale * angle_rows[a][s], the rule of PHASE / RY
 *                             (`op %d: angle row %d out of range` when a >= n_rows; p and scale must be finite, else
 *                             QIDDM_ERR_INVALID "... not finite").  The row is device memory the library does not look
 *                             into: strengths outside [0, 1] are the caller's responsibility, the kernels do not clamp.
 *                             The reverse sweeps add scale * dL/dstrength into grad_rows[a][s].  With Lambda the adjoint
 *                             behind the channel, rho the state in front of it and o = -1 / (2 sqrt(1 - gamma)),
 *                             dL/dstrength = <Lambda, E'(rho)>, where on each 2 x 2 block M of the wire E'(M) is
 *                               PHASE_DAMP  M00' = M11' = 0;                       M01' = o M01, M10' = o M10
 *                               AMP_DAMP    M00' = +M11, M11' = -M11;              M01' = o M01, M10' = o M10
 *                               DEPOL       M00' = (2/3)(M11 - M00), M11' = -M00'; M01' = -(4/3) M01, M10' = -(4/3) M10
 *                             At gamma = 1 the derivative of the two damping channels is not finite (PennyLane's is not
 *                             either); it is not special-cased.  Several channels may read one row: their gradients add.
 *   QIDDM_MIX_CHANNEL (= 16)  a general one-wire channel on `wire`: `a` is the first of FOUR consecutive rows of `gates`,
 *                             rows a .. a+3 hold the superoperator S (4 x 4 complex, row-major; row r = S[r][0..3] as
 *                             (re, im)).  On every 2 x 2 block M of the wire vec(M') = S vec(M), vec(M) = (M00, M01,
 *                             M10, M11); for Kraus operators S = sum_k K_k (x) conj(K_k).  `p` and `scale` are not read.
 *                             `gates` is device memory the library does not look into: that S is completely positive
 *                             and trace preserving is the caller's responsibility.  The planner and every workspace
 *                             size treat it as AMP_DAMP on the same wire.  In the reverse sweeps the adjoint takes S^H
 *                             per block and the op's four rows of grad_gates are zeros for every sample (channel
 *                             operands get no gradient).  PennyLane's BitFlip, PhaseFlip, PauliError,
 *                             GeneralizedAmplitudeDamping, ResetError, ThermalRelaxationError and QubitChannel on one
 *                             wire are this op.
 *   QIDDM_MIX_CHANNEL2 (= 32) a general two-wire channel on w1 = `wire` and w2 = `reserved` -- the only kind that reads
 *                             the struct's fourth field; w1 > w2 is allowed, w1 == w2 is not.  `a` is the first of 64
 *                             consecutive rows of `gates` holding the superoperator S (16 x 16 complex, row-major): row t
 *                             of S is gate rows a+4t .. a+4t+3, four (re, im) pairs a gate row.  With the other 2n-4
 *                             index bits of rho fixed, the remaining 16 elements are a 4 x 4 block M[r][c],
 *                             r = 2 (row bit of w1) + (row bit of w2), c likewise from the column bits; the op is
 *                             vec(M') = S vec(M), vec(M)[4r + c] = M[r][c], on every block.  For Kraus operators K_k
 *                             (4 x 4, index 2 b1 + b2, the first wire most significant: PennyLane's convention)
 *                             S = sum_k K_k (x) conj(K_k), i.e. S[4r+c][4r'+c'] = sum_k K_k[r][r'] conj(K_k[c][c']).
 *                             `p` and `scale` are not read; `gates` is not looked into (complete positivity and trace
 *                             preservation are the caller's responsibility, and a channel that happens to be diagonal is
 *                             still planned as a general one).  The planner gives it CNOT's wire set {w1, w2} and treats
 *                             it as a channel that is not diagonal; every workspace size counts it as one channel.  In the
 *                             reverse sweeps the adjoint takes S^H per block (out[c] = sum_r conj(S[r][c]) v[r]) and the
 *                             op's 64 rows of grad_gates are zeros for every sample.  PennyLane's QubitChannel with 4 x 4
 *                             operators and PauliError with a two-letter word are this op.  The rule for kinds is
 *                             "general k-wire channel = 16 k".
 *   QIDDM_MIX_SHOTS (= 12)    legal only as the LAST op (`op %d: a sampled read-out must be the last op`); not an operation on
 *                             rho: it says that the read-out named by `measure` is estimated from a finite number of
 *                             computational-basis shots, drawn on the device in the launch that holds rho.  `a` is the
 *                             number of shots, 1 .. 2^31 - 1 (`op %d: shots %d out of range`); `p` is the seed and `scale`
 *                             the stream offset, both integer-valued doubles in [0, 2^53) (a non-integer, negative, too
 *                             large or non-finite value: `op %d: sampled read-out seed|offset %g is not an integer in
 *                             [0, 2^53)`); `wire` and `reserved` must be 0.  Output layout and dtype do not change:
 *                             QIDDM_MEAS_PROBS gives count[k] / shots, QIDDM_MEAS_EXPZ (n+ - n-) / shots per wire (wire w
 *                             is bit n-1-w of the outcome, sign -1 when the bit is set), each one float64 division of
 *                             exact integers.  The sampling rule, for D = 2^n outcomes of sample b (the ABSOLUTE row of
 *                             the batch: neither the sample loop of qiddm_mixed_forward nor the chunks of
 *                             qiddm_mixed_wide_forward move a stream):
 *                               p_k = fmax((double)Re rho_kk, 0)   (a NaN counts as 0),
 *                               c_k = p_0 + ... + p_k, float64, added sequentially in k (numpy.cumsum), T = c_{D-1};
 *                               shot s takes word (s & 3) of Philox4x32-10 with counter (s >> 2, b mod 2^32, offset mod
 *                               2^32, offset >> 32) and key (seed mod 2^32, seed >> 32);
 *                               v = ((double)word * 2^-32) * T;  outcome = #{k : c_k <= v}, clamped to D - 1.
 *                             T not positive or not finite: the sample's row is NaN.  Counts are accumulated with
 *                             integer adds only (LDS integer atomics, integer wave reductions): reruns are bit-identical,
 *                             no float atomics.  CDF and histogram live in LDS: no workspace size changes.  The reverse
 *                             sweeps (qiddm_mixed_backward, qiddm_mixed_wide_backward), their *_workspace_bytes and
 *                             qiddm_mixed_wide_backward_plan answer QIDDM_ERR_UNSUPPORTED for a program that ends in it
 *                             (`... a sampled read-out has no gradient`).  qiddm_mixed_wide_plan accepts it, counts it in
 *                             no sweep and not as a non-diagonal op; its op_segment entry is -1.  PennyLane's
 *                             default.mixed with shots=... is a program that ends in this op; readout_prob is a BitFlip
 *                             (QIDDM_MIX_CHANNEL) on every wire in front of it.
 *   QIDDM_MIX_OBS (= 20)      one term of the MEASUREMENT TABLE, not an operation on rho: coefficient `p` times a Pauli word.
 *                             `wire` is the word's x-mask (the wires that carry X or Y), `a` its z-mask (Z or Y), wire w at
 *                             bit n-1-w of each, both in [0, 2^n); `reserved` is the output column; `scale` is not read.
 *                             The table is the tail of the program: from the first QIDDM_MIX_OBS on every op is one
 *                             (`op %d: only measurement terms may follow the first one`), 1 .. QIDDM_MIX_MAX_OBS = 256 of
 *                             them, `p` finite, the first term's column 0 and every later one equal to the previous
 *                             term's or larger by 1.  Terms that share a column add up (a Hamiltonian).  measure =
 *                             QIDDM_MEAS_OBS reads it: with ny = popcount(x & z),
 *                               out[sample][c] = sum over the terms t of column c of
 *                                                p_t Re( i^ny_t sum_k (-1)^popcount(k & z_t) rho[k][k ^ x_t] ),
 *                             which is sum_t p_t Tr(rho P_t) with Y = [[0, -i], [i, 0]]; float64, fixed-order sums, no
 *                             atomics (reruns are bit-identical).  out / grad_out are (batch, last column + 1).  The
 *                             reverse sweeps start from Lambda_N = sum_t grad_out[sample][column_t] p_t P_t, a Hermitian
 *                             matrix that is complex when a word holds Y and not diagonal when it holds X or Y.
 *                             QIDDM_MEAS_OBS without a table, and a table under QIDDM_MEAS_PROBS / _EXPZ, are
 *                             QIDDM_ERR_INVALID; a QIDDM_MIX_SHOTS anywhere in a program with a table is
 *                             QIDDM_ERR_UNSUPPORTED (shots of a word with X or Y need a basis rotation).  The planners and
 *                             the *_workspace_bytes functions that read a program check the table in full, count it in no
 *                             sweep and no snapshot; its op_segment entries are -1.
 *   QIDDM_MIX_GATE2 (= 24)    a two-wire unitary on w1 = `wire` and w2 = `reserved` (checked like QIDDM_MIX_CHANNEL2's: `op %d:
 *                             bad second wire %d`; w1 > w2 is allowed).  `a` is the first of FOUR consecutive rows of
 *                             `gates`: row a + r holds U[r][0..3] as four (re, im) pairs, operator index 2 b1 + b2 with the
 *                             first wire most significant (QIDDM_MIX_CHANNEL2's convention, PennyLane's).  On every 4 x 4
 *                             block M of the two wires (as for QIDDM_MIX_CHANNEL2) M' = U M U^dagger, i.e. rho <- U rho
 *                             U^dagger.  `p` and `scale` are not read.  As with QIDDM_MIX_GATE the rows are device memory
 *                             and unitarity is the caller's responsibility.  a < 0 or a + 3 >= n_gates (summed in 64 bits):
 *                             `op %d: gate rows %d..%d out of range`.  The planner gives it CNOT's wire set {w1, w2}: not
 *                             diagonal, both wires in the segment's tile.  It is a unitary, not a channel: no snapshot, no
 *                             segment of its own in the reverse plan; the reverse sweeps un-compute it with U^dagger on rho
 *                             and on the adjoint and return, per sample, dL/dRe U and dL/dIm U in rows a .. a+3 of
 *                             grad_gates, in the layout of the rows themselves (entries treated as independent reals): with
 *                             N = sum over the 4 x 4 blocks of B_rho B_Lambda^dagger, both taken behind the gate, and
 *                             R = U^dagger N, dL/dRe U_ab = 2 Re R_ba and dL/dIm U_ab = -2 Im R_ba -- the 4 x 4 form of
 *                             QIDDM_MIX_GATE's.  Several ops may name the same four rows (one matrix behind every
 *                             entangler): their gradients add, as for QIDDM_MIX_GATE.  Rows that PARTLY overlap those of
 *                             another QIDDM_MIX_GATE / QIDDM_MIX_GATE2 op have no meaningful gradient: the two backward
 *                             entry points refuse them with QIDDM_ERR_INVALID, `op %d: gate rows %d..%d overlap those of
 *                             op %d` (checked behind the sampled read-out's refusal, in front of the outputs).  PennyLane's
 *                             SWAP, ISWAP, CY, CRX / CRY / CRZ / CRot, ControlledPhaseShift, IsingXX / YY / ZZ and
 *                             QubitUnitary on two wires are this op.
 *   QIDDM_MIX_RHO (= 28)      legal only as the LAST op and only once (`op %d: a density-matrix read-out must be the last op`);
 *                             not an operation on rho: it says which wires the read-out of measure = QIDDM_MEAS_RHO keeps.
 *                             `wire` is the keep-mask, wire w at bit n-1-w, in [1, 2^n) (`op %d: keep mask %d out of range`);
 *                             `a` and `reserved` must be 0 (`op %d: a density-matrix read-out takes a 0 and reserved 0`); `p`
 *                             and `scale` are not read.  With k = popcount(mask) and K = 2^k, out / grad_out are
 *                             (batch, ld >= 2 K^2) float64: element (r, c) of the reduced matrix at columns 2 (r K + c) (real
 *                             part) and 2 (r K + c) + 1 (imaginary part).  r and c number the bit strings of the kept wires in
 *                             ascending wire order, the lowest wire most significant (the bit order of probs); with e running
 *                             over the 2^(n-k) bit strings of the traced-out wires and dep(r, e) the n-bit index that holds r's
 *                             bits at the mask's positions and e's at the others,
 *                               out[sample][r][c] = sum_e rho[dep(r, e)][dep(c, e)],
 *                             float64, added in a fixed order (64 or more traced values: 64 strided partial sums in ascending
 *                             e, then a butterfly over them; fewer: ascending e), no atomics: reruns are bit-identical and
 *                             the chunking of the tile-fused engine does not show.  k = n is rho itself, converted to float64.
 *                             The reverse sweeps pair their adjoint Lambda with rho as Re sum_ij conj(Lambda_ij) rho_ij, and
 *                             every state they meet is Hermitian; they have only ever been seeded with Hermitian matrices.
 *                             With g_re[r][c] = grad_out[2 (r K + c)] and g_im[r][c] = grad_out[2 (r K + c) + 1] the loss's
 *                             differential is sum g_re Re(d rho_A) + g_im Im(d rho_A) = Re sum_ij conj(G_ij) d rho_ij for
 *                             G_ij = g_re[r][c] + i g_im[r][c] where ((i ^ j) & ~mask) == 0 (r, c: the kept bits of i, j) and
 *                             G_ij = 0 elsewhere.  G's anti-Hermitian part pairs to zero with every Hermitian matrix, so it
 *                             contributes to no gradient, and the sweeps start from the Hermitian part:
 *                               Lambda_N[i][j] = (g_re[r][c] + g_re[c][r]) / 2 + i (g_im[r][c] - g_im[c][r]) / 2.
 *                             Under any other measure the op is QIDDM_ERR_INVALID (`op %d: a density-matrix read-out needs
 *                             measure QIDDM_MEAS_RHO`), QIDDM_MEAS_RHO without it likewise (`measure QIDDM_MEAS_RHO needs a
 *                             density-matrix read-out as the last op`), as is a QIDDM_MIX_OBS table in the same program
 *                             (`op %d: a density-matrix read-out beside a measurement table`); a QIDDM_MIX_SHOTS in the same
 *                             program is QIDDM_ERR_UNSUPPORTED (`op %d: a sampled read-out beside a density-matrix read-out`).
 *                             All of this is checked where the measurement table is, by everything that reads a program.  The
 *                             planners count the op in no sweep, no snapshot and no slot; its op_segment entry is -1; no
 *                             workspace size changes.  PennyLane's qml.state() (k = n), qml.density_matrix(wires) and what
 *                             follows from them (purity, the expectation value of a Hermitian matrix) are this read-out.
 *   QIDDM_MIX_CHANNEL_FIT (= 18), QIDDM_MIX_CHANNEL2_FIT (= 34)
 *                             QIDDM_MIX_CHANNEL and QIDDM_MIX_CHANNEL2 with rows that get a gradient ("16 k + 2 is the k-wire
 *                             channel whose rows get a gradient").  Operands, checks, messages, their place in the check
 *                             order, planning and every workspace size of the forwards are those of 16 and 32, and a
 *                             forward gives, bit for bit, what the same program with the constant kinds gives.  In the
 *                             reverse sweeps they do to the adjoint and to rho what 16 and 32 do (S^H per block; rho from
 *                             the snapshot) and return, per sample, the gradient of the rows in the layout of the rows,
 *                             entries treated as independent reals as for QIDDM_MIX_GATE / _GATE2: the sweeps pair the
 *                             adjoint with rho as dL = Re sum conj(Lambda) d rho (which gives dL/dstrength = <Lambda,
 *                             E'(rho)> for the native channels and 2 Re R_ba for QIDDM_MIX_GATE), so with Lambda' the
 *                             adjoint behind the channel, M the block of rho in front of it (the snapshot) and
 *                               W[r][c] = sum over the blocks of conj(vec(Lambda')[r]) vec(M)[c],
 *                             dL/dRe S[r][c] = Re W[r][c] and dL/dIm S[r][c] = -Im W[r][c]: 16 complex sums for one wire,
 *                             256 for two.  The gradient is with respect to unconstrained entries: staying completely
 *                             positive and trace preserving is the caller's parametrisation.  Several ops may name the
 *                             same rows: their gradients add.  Rows that PARTLY overlap those of another QIDDM_MIX_GATE /
 *                             _GATE2 / _FIT op are refused by the two backward entry points like QIDDM_MIX_GATE2's (`op %d:
 *                             gate rows %d..%d overlap those of op %d`).  Every sum runs in a fixed order, without atomics:
 *                             reruns, a lowered max_blocks and a smaller tile-fused workspace give the same bits.  The
 *                             tile-fused backward keeps 32 (one wire) or 512 (two wires) tile partials per such op, and,
 *                             like a native channel with a >= 0, replays up to a trailing channel segment that holds
 *                             one; qiddm_mixed_wide_backward_workspace_bytes and _backward_plan count both, for these
 *                             kinds only.  A program without them runs the device code it ran before they existed.
 * Kinds 10, 11, 13..15, 17, 19, 21..23, 25..31 other than 28, 33, and kinds above 34 are no ops: refused as `op %d: unknown kind %d`
 * (40, QIDDM_MIX_KRAUS, and 48, QIDDM_MIX_KRAUS2, are ops of the trajectory entry points alone, qiddm_hip_traj.h: these entry
 * points and the planners refuse them in the same words; 41 is no op anywhere).
 * program: HOST array (copied to the head of `workspace` on `stream`); angle_rows (n_rows, rows_ld >= batch),
 * features (batch, feat_ld), gates (n_gates, 8), out (batch, 2^n | n | columns of the table | 2 * 4^k) float64 DEVICE arrays.
 * The four compute entry points check their arguments in one order and report the first fault: n_qubits, dtype, negative
 * batch / n_ops, measure (batch == 0 then returns QIDDM_OK with no pointer looked at), program (not empty, starts with a
 * state preparation), the density-matrix read-out or the measurement table (all of it, then against `measure`), negative n_rows / n_gates,
 * angle_rows / rows_ld, gates, the ops in front of the table one by one (kind, wire, target wire
 * or second wire -- `op %d: bad second wire %d` when it is outside 0..n-1 or equal to `wire` --; QIDDM_MIX_SHOTS instead:
 * its position, wire / reserved, shots, seed, offset --,
 * then the operand they index: features / feat_ld / n_features, angle row, gate, probability (a >= 0: angle row, then
 * finite p / scale), channel rows, gate rows), max_blocks (negative:
 * refused for an empty batch as well), in the reverse sweeps a program that ends in QIDDM_MIX_SHOTS, the outputs
 * (out, out_ld | grad_out / gout_ld, grad_rows, grad_gates, grad_features), workspace.                   */
enum {
  QIDDM_MIX_ZERO = 0, QIDDM_MIX_AMP_EMBED, QIDDM_MIX_PHASE, QIDDM_MIX_RY, QIDDM_MIX_GATE, QIDDM_MIX_CZ,
  QIDDM_MIX_CNOT, QIDDM_MIX_PHASE_DAMP, QIDDM_MIX_AMP_DAMP, QIDDM_MIX_DEPOL,
  QIDDM_MIX_SHOTS = 12,
  QIDDM_MIX_CHANNEL = 16,
  QIDDM_MIX_CHANNEL_FIT = 18,
  QIDDM_MIX_OBS = 20,
  QIDDM_MIX_GATE2 = 24,
  QIDDM_MIX_RHO = 28,
  QIDDM_MIX_CHANNEL2 = 32,
  QIDDM_MIX_CHANNEL2_FIT = 34,
  QIDDM_MIX_KRAUS = 40, /* the trajectory entry points only (qiddm_hip_traj.h) */
  QIDDM_MIX_KRAUS2 = 48 /* the trajectory entry points only: a two-wire channel by its Kraus operators (qiddm_hip_traj.h) */
};
#define QIDDM_MIX_MAX_OBS 256 /* terms of a measurement table */
#define QIDDM_MIX_MAX_KRAUS2 16 /* operators of a QIDDM_MIX_KRAUS2 op */
typedef struct qiddm_mixed_op {
  int32_t kind, wire, a, reserved; /* reserved: the second wire of QIDDM_MIX_CHANNEL2 / _GATE2, the column of QIDDM_MIX_OBS */
  double p, scale;
} qiddm_mixed_op_t;
int64_t qiddm_mixed_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_ops);
int qiddm_mixed_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                        const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                        int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                        const double *gates, int32_t n_gates, int32_t measure, int64_t batch, double *out,
                        int64_t out_ld, void *workspace, int64_t workspace_bytes, void *stream);
/* Reverse sweep (vector-Jacobian product) of qiddm_mixed_forward: the same program and inputs, plus
 *   grad_out       (batch, gout_ld >= 2^n | n | columns of the table | 2 * 4^k) float64 DEVICE: dL/d out
 *   grad_rows      (n_rows, batch) float64 DEVICE: dL/d angle_rows (required when n_rows > 0)
 *   grad_gates     (batch, n_gates, 8) float64 DEVICE: per-sample dL/d gates (the caller sums over the batch;
 *                  required when n_gates > 0)
 *   grad_features  (batch, n_features) float64 DEVICE: dL/d features (required when the program has AMP_EMBED)
 *   max_blocks     grid cap (0: the default of 256 workgroups); samples beyond the grid loop
 * The kernel replays the forward, keeping a copy of rho in front of every channel (and every state preparation
 * after op 0) in `workspace`, then walks the program backwards.  No atomics: reruns are bit-identical.  The
 * workspace holds the program, the snapshots and, when rho and the adjoint do not both fit in 128 KiB of LDS
 * (n >= 7), those two as well -- qiddm_mixed_backward_workspace_bytes(program) bytes.                    */
int64_t qiddm_mixed_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch,
                                             const qiddm_mixed_op_t *program, int32_t n_ops, int32_t max_blocks);
int qiddm_mixed_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                         const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                         int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                         const double *gates, int32_t n_gates, int32_t measure, int64_t batch,
                         const double *grad_out, int64_t gout_ld, double *grad_rows, double *grad_gates,
                         double *grad_features, int32_t max_blocks, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* Tile-fused density-matrix engine, 7 <= n_qubits <= 10 (else QIDDM_ERR_UNSUPPORTED): the 10-wire models
 * of the reference's 28 x 28 noise study (src/fashion_noise.py:42-44).  rho of a sample (index (i << n) | j) lives in a
 * slab of `workspace`; the program is cut into SEGMENTS, each run by one sweep -- one launch over (tile, sample) in which
 * a workgroup holds the 2^12 elements spanned by the index-bit pairs of six wires in LDS and applies the whole segment.
 * A segment takes PHASE / CZ / PHASE_DAMP on any wires (diagonal on vec(rho)), GATE / RY / AMP_DAMP / DEPOL / CHANNEL on its six
 * wires, CNOT, GATE2 and CHANNEL2 between two of them, and ZERO / AMP_EMBED as its first op.  Ops keep program order except where they
 * commute (no shared wire, or both diagonal).  Same arguments and results as qiddm_mixed_forward; float64 read-out with
 * fixed-order sums, no atomics: reruns are bit-identical.
 *   qiddm_mixed_wide_plan             host only (no device is touched): the number of sweeps, the number of ops that are
 *                                     not diagonal (state preparations included) and, if op_segment is not NULL, the
 *                                     segment of every op.  Any of the three outputs may be NULL.
 *   qiddm_mixed_wide_workspace_bytes  program head + one float64 per resident sample + the resident slabs.  At most
 *                                     1 GiB of slabs is resident (64 samples at n = 10 in float64); larger batches run
 *                                     in chunks inside qiddm_mixed_wide_forward.  `program` may be NULL.
 *   qiddm_mixed_wide_forward          also accepts a smaller workspace, down to one slab: fewer samples are resident
 *                                     per chunk; the results do not depend on the chunking.                          */
int64_t qiddm_mixed_wide_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch,
                                         const qiddm_mixed_op_t *program, int32_t n_ops);
int qiddm_mixed_wide_plan(int32_t n_qubits, const qiddm_mixed_op_t *program, int32_t n_ops, int32_t *n_sweeps,
                          int32_t *n_nondiag_ops, int32_t *op_segment);
int qiddm_mixed_wide_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                             const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                             int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                             const double *gates, int32_t n_gates, int32_t measure, int64_t batch, double *out,
                             int64_t out_ld, void *workspace, int64_t workspace_bytes, void *stream);
/* Reverse sweep of the tile-fused engine: the exact vector-Jacobian product of qiddm_mixed_wide_forward, with the
 * arguments and gradient layouts of qiddm_mixed_backward (no max_blocks) and its argument checks; 7 <= n_qubits <= 10
 * (else QIDDM_ERR_UNSUPPORTED).  A native channel with a >= 0 gives its row the gradient of its strength (see the kinds);
 * constant strengths (a < 0) and the general channels' rows get none.  Ops in front of the last state preparation reach
 * no output: only the ops from there on (the LIVE ops) are planned and run, other parameters get a zero gradient.  The
 * live ops are cut into segments that hold either channels only or no channel.  The call
 *   replays     the forward sweeps; a channel segment writes rho to a further slab, so the state in front of it stays
 *               behind as a snapshot (a channel is not inverted).  Channel segments behind the last unitary one are
 *               not replayed -- except, in a program where such a trailing segment other than the first holds a native
 *               channel with a >= 0, those in front of the last one that does (its gradient needs the state in front
 *               of it; the snapshots they add are counted by qiddm_mixed_wide_backward_plan).
 *   walks back  one launch over (tile, sample) per segment, the rho tile and the adjoint's tile side by side in LDS;
 *               the first one generates the adjoint from grad_out.  A unitary un-computes both tiles and writes its
 *               tile partial per (op, tile, sample); a channel segment applies E^dagger to the adjoint and rho steps
 *               back to the snapshot; one that holds a native channel with a >= 0 keeps the rho tile in front of each
 *               such channel beside the adjoint's (the snapshot's tile with the segment's earlier ops applied again)
 *               and writes a tile partial of <Lambda, E'(rho)>.  AMP_EMBED: a matrix-vector pass over the adjoint's slab.
 *   finalizes   the tile partials, summed in a fixed order per parameter and sample.
 * No atomics: reruns are bit-identical and the gradients do not depend on the chunking.
 *   qiddm_mixed_wide_backward_plan             host only: sweeps of the replay, launches of the walk back, snapshots.
 *                                              Any output may be NULL.
 *   qiddm_mixed_wide_backward_workspace_bytes  head + resident * per_sample, every term rounded up to 256 B:
 *                                              head = live ops * 32 + live ops * 4 + gradient ops * 24 + (parameter
 *                                              groups + 1) * 4; per_sample = 8 (1 + 2^n) + 8 * slots * 2^(2n-12) +
 *                                              (2 + snapshots) slabs, slots = 8 per live GATE + 32 per live GATE2 + 1 per live PHASE / RY
 *                                              / native channel with a >= 0 (gradient ops: the same ops).  resident = min(batch, 1 GiB / per_sample), at least 1;
 *                                              larger batches run in chunks inside the call.  `program` is required.
 *   qiddm_mixed_wide_backward                  also accepts a smaller workspace, down to head + per_sample.          */
int64_t qiddm_mixed_wide_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch,
                                                  const qiddm_mixed_op_t *program, int32_t n_ops);
int qiddm_mixed_wide_backward_plan(int32_t n_qubits, const qiddm_mixed_op_t *program, int32_t n_ops,
                                   int32_t *n_replay_sweeps, int32_t *n_reverse_sweeps, int32_t *n_snapshots);
int qiddm_mixed_wide_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t *program, int32_t n_ops,
                              const double *angle_rows, int64_t rows_ld, int32_t n_rows, const double *features,
                              int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                              const double *gates, int32_t n_gates, int32_t measure, int64_t batch,
                              const double *grad_out, int64_t gout_ld, double *grad_rows, double *grad_gates,
                              double *grad_features, void *workspace, int64_t workspace_bytes, void *stream);

/* Quantum trajectories (the same programs on a pure state, 1 <= n_qubits <= 16, with the op QIDDM_MIX_KRAUS): the two
 * entry points, their arguments and the trajectory rule are in the extension header include/qiddm_hip_traj.h.  This
 * header declares what it declared before they existed.                                                            */

#ifdef __cplusplus
}
#endif
#endif /* QIDDM_HIP_H */

// qiddm_mixed.hip -- extern "C" entry points of the density-matrix executor (include/qiddm_hip.h,
// "hardware-noise study"); device code in qsim_mixed.h (n <= 8, one workgroup per sample) and qsim_mixed_wide.h
// (n = 7..10, tile-fused sweeps) and qsim_mixed_wide_adjoint.h (their reverse sweep), with the planner that cuts a
// program into sweeps.
// Host side: the four compute entry points share their arguments from n_qubits to batch.  Each puts them into a
// MixedCall, has check_call() validate them (one order for all four, stated in the header), and then reads as a list of
// steps: outputs, geometry (and plan), workspace, upload(), make_scalars(), for_dtype launch.  The *_workspace_bytes
// functions check sizes with check_sizes() and the two *_plan functions validate through the planner alone.
// A program may end in QIDDM_MIX_SHOTS (the sampled read-out, qsim_mixed_shots.h): the forwards keep it out of the ops the
// kernels walk and launch the sampling kernels with its fields (shots_of); everything reverse refuses it (refuse_sampled).
// Or it ends in a table of QIDDM_MIX_OBS terms (QIDDM_MEAS_OBS: Pauli-word expectation values): check_obs_tail validates
// it wherever a program is read, the planners leave it out of every sweep, and it is uploaded behind the ops so that the
// read-out and the seed of the reverse sweeps find it at prog[n_body ..).
// Or it ends in one QIDDM_MIX_RHO op (QIDDM_MEAS_RHO: the reduced density matrix of the wires in its keep-mask): the same
// tail check validates it, it is a tail of one op to everything that plans or uploads, and the read-out kernels and the
// seed of the reverse sweeps take its mask.
// QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT are QIDDM_MIX_CHANNEL / _CHANNEL2 to every check, plan and forward (base_kind);
// the reverse sweeps return the gradient of their rows from kernels of their own (qiddm::kLevelFit in the one-workgroup
// engine; mixed_wide_adjoint_channels_fit and mixed_wide_fit_finalize in the tile-fused one), which a program without
// these kinds never launches.
// The trajectory engine (qsim_traj.h; the two qiddm_mixed_traj_* entry points at the end of this file) runs the same
// programs on a pure state up to 16 wires.  It validates through check_call with an Engine whose `traj` flag admits
// QIDDM_MIX_KRAUS / QIDDM_MIX_KRAUS2 and refuses what a trajectory cannot do (superoperator kinds, SHOTS, RHO); without the flag nothing
// above reads differently.  Its reverse sweep (qsim_traj_adjoint.h; include/qiddm_hip_traj_grad.h) follows it: the same
// checks, then the backward's own (no later state preparation, the gate-row overlap refusal, the gradient pointers).
// Its sampled read-out (qsim_traj_shots.h; include/qiddm_hip_traj_shots.h; the last two entry points of this file) shares
// that validator too: the Engine's `sampled` flag refuses a measurement table beside the density-matrix read-out.
#include "capi_common.h"
#include "../../include/qiddm_hip_traj_grad.h"
#include "../../include/qiddm_hip_traj_shots.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "qsim_mixed.h"
#include "qsim_mixed_wide.h"
#include "qsim_mixed_wide_adjoint.h"
#include "qsim_traj.h"
#include "qsim_traj_adjoint.h"
#include "qsim_traj_shots.h"

namespace {

using qiddm_capi::fail;
using qiddm_capi::for_dtype;
using qiddm_capi::kMaxLds;
using qiddm_capi::launch;
using qiddm_capi::launched;

static_assert(sizeof(qiddm::MixedOp) == sizeof(qiddm_mixed_op_t), "program layout");
static_assert((int)qiddm::kMixDepol == (int)QIDDM_MIX_DEPOL && (int)qiddm::kMixChannel == (int)QIDDM_MIX_CHANNEL &&
                  (int)qiddm::kMixChannel2 == (int)QIDDM_MIX_CHANNEL2 && (int)qiddm::kMixShots == (int)QIDDM_MIX_SHOTS &&
                  (int)qiddm::kMixObs == (int)QIDDM_MIX_OBS && (int)qiddm::kMixGate2 == (int)QIDDM_MIX_GATE2 &&
                  (int)qiddm::kMixRho == (int)QIDDM_MIX_RHO && (int)qiddm::kMixChannelFit == (int)QIDDM_MIX_CHANNEL_FIT &&
                  (int)qiddm::kMixChannel2Fit == (int)QIDDM_MIX_CHANNEL2_FIT && (int)qiddm::kMixKraus == (int)QIDDM_MIX_KRAUS &&
                  (int)qiddm::kMixKraus2 == (int)QIDDM_MIX_KRAUS2 && qiddm::kTrajMaxKraus2 == QIDDM_MIX_MAX_KRAUS2,
              "op kinds");
static_assert(offsetof(qiddm::MixedOp, wire2) == offsetof(qiddm_mixed_op_t, reserved), "the second wire travels in `reserved`");

inline int64_t round256(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t slab_bytes(int32_t n, int32_t dtype) { return ((int64_t)1 << (2 * n)) * (dtype == QIDDM_F32 ? 8 : 16); }
inline int64_t program_bytes(int32_t n_ops) { return round256((int64_t)n_ops * (int64_t)sizeof(qiddm::MixedOp)); }

// QIDDM_MIX_GATE2 (the two-wire unitary): validated like CHANNEL2's wires and GATE's rows, planned like CNOT, and in the
// reverse sweeps a unitary -- no snapshot, 32 tile partials, a refusal of rows that partly overlap another gate's.
// QIDDM_MIX_CHANNEL_FIT / _CHANNEL2_FIT (16 k + 2: the k-wire channel whose rows get a gradient): everything that
// validates, plans or sizes reads them as the constant kinds (base_kind); the forwards and the tile-fused engine upload
// them as such, so their kernels never meet the new kinds; the reverse sweeps give their rows a gradient.
inline bool is_fit(int kind) { return kind == qiddm::kMixChannelFit || kind == qiddm::kMixChannel2Fit; }
inline int base_kind(int kind) { return is_fit(kind) ? kind - 2 : kind; }
inline bool is_channel2(int kind) { return base_kind(kind) == qiddm::kMixChannel2; }
inline bool is_prep(int kind) { return kind == qiddm::kMixZero || kind == qiddm::kMixAmpEmbed; }
inline bool is_diag(int kind) {
  return kind == qiddm::kMixPhase || kind == qiddm::kMixCZ || kind == qiddm::kMixPhaseDamp;
}
// the kernels have an instantiation per qiddm::MixedLevel (which general-channel cases they carry); a program (segment)
// runs the lowest one that holds its ops: calls f(std::integral_constant<int, level>{})
// (the kernels that only ever see channel segments: a level without the two-wire unitary's flag).  None of these
// dispatchers looks at qiddm::kLevelFit: that flag selects kernels of its own where a reverse sweep is launched.
template <typename F>
int for_level(int level, F&& f) {
  return level >= qiddm::kLevelChannel2 ? f(std::integral_constant<int, qiddm::kLevelChannel2>{})
         : level == qiddm::kLevelChannel ? f(std::integral_constant<int, qiddm::kLevelChannel>{})
                                          : f(std::integral_constant<int, qiddm::kLevelLean>{});
}
// the kernels that run whole programs or unitary segments.  With the flag of the two-wire unitary (qiddm::kLevelGate2)
// two instantiations exist: beside no channel case at all, or beside all of them.
template <typename F>
int for_op_level(int level, F&& f) {
  if (!qiddm::mixed_has_gate2(level)) return for_level(level, f);
  return qiddm::mixed_channels_of(level) > qiddm::kLevelLean
             ? f(std::integral_constant<int, qiddm::kLevelChannel2 | qiddm::kLevelGate2>{})
             : f(std::integral_constant<int, qiddm::kLevelLean | qiddm::kLevelGate2>{});
}
inline int program_level(const qiddm_mixed_op_t* program, int32_t n_ops) {
  int level = qiddm::kLevelLean;
  for (int i = 0; i < n_ops; ++i) {
    level = qiddm::mixed_level_join(level, qiddm::mixed_level_of(base_kind(program[i].kind)));
    if (is_fit(program[i].kind)) level |= qiddm::kLevelFit;
  }
  return level;
}
// the program as the forward kernels (and every kernel of the tile-fused engine) read it: the constant kinds
inline qiddm_mixed_op_t constant_op(qiddm_mixed_op_t op) {
  op.kind = base_kind(op.kind);
  return op;
}
inline bool is_gate2(int kind) { return kind == qiddm::kMixGate2; }
// the rows of `gates` a GATE / GATE2 op reads and gets its gradient in: [a, a + n), n = 0 for every other kind
// (a trainable channel: the 4 or 64 rows of its superoperator)
inline int gate_rows(int kind) {
  return kind == qiddm::kMixGate ? 1 : is_gate2(kind) ? 4 : kind == qiddm::kMixChannelFit ? 4 : kind == qiddm::kMixChannel2Fit ? 64 : 0;
}
inline bool is_channel(int kind) {
  return kind == qiddm::kMixPhaseDamp || kind == qiddm::kMixAmpDamp || kind == qiddm::kMixDepol ||
         base_kind(kind) == qiddm::kMixChannel || base_kind(kind) == qiddm::kMixChannel2;
}
// a native channel that reads its strength from an angle row: the reverse sweeps give that row a gradient
inline bool is_graded(const qiddm_mixed_op_t& op) {
  return (op.kind == qiddm::kMixPhaseDamp || op.kind == qiddm::kMixAmpDamp || op.kind == qiddm::kMixDepol) && op.a >= 0;
}
// a channel whose gradient needs the state in front of it
inline bool needs_front(const qiddm_mixed_op_t& op) { return is_graded(op) || is_fit(op.kind); }

// ---- argument checks ---------------------------------------------------------------------------------------------------
struct Engine {
  const char* name;
  int min_qubits, max_qubits;
  bool traj = false;  // the trajectory engine (qsim_traj.h): a pure state, QIDDM_MIX_KRAUS, no superoperators / SHOTS / RHO
  bool sampled = false;  // its sampled read-out (qsim_traj_shots.h): PROBS and EXPZ only, no measurement table
};
constexpr Engine kOneWorkgroup{"", 1, 8}, kTileFused{"tile-fused ", 7, 10}, kTrajectories{"trajectory ", 1, 16, true};
constexpr Engine kTrajectoryShots{"trajectory ", 1, 16, true, true};

// shots count outcomes of the computational basis: a table of Pauli words has no sampled read-out on trajectories
int refuse_sampled_table() {
  return fail(QIDDM_ERR_UNSUPPORTED,
              "a measurement table on sampled trajectories: words of I and Z are signed sums of the sampled probs "
              "(QIDDM_MEAS_PROBS), words with X or Y need a basis rotation in front of the read-out");
}

int check_wires(int32_t n, const Engine& e) {
  if (e.traj && (n < e.min_qubits || n > e.max_qubits))
    return fail(QIDDM_ERR_UNSUPPORTED,
                "trajectory execution needs %d <= n_qubits <= %d (got %d): a pure state of 2^%d elements is the widest "
                "the one-workgroup engine holds; split the register or use a state-vector device",
                e.min_qubits, e.max_qubits, n, e.max_qubits);
  if (n < e.min_qubits || n > e.max_qubits)
    return fail(QIDDM_ERR_UNSUPPORTED, "%sdensity-matrix execution needs %d <= n_qubits <= %d (got %d)", e.name,
                e.min_qubits, e.max_qubits, n);
  return QIDDM_OK;
}

// what a workspace size depends on: checked by the *_workspace_bytes functions and, first of all, by check_call
int check_sizes(int32_t n, int32_t dtype, int64_t batch, int32_t n_ops, const Engine& e) {
  if (const int rc = check_wires(n, e); rc != QIDDM_OK) return rc;
  if (dtype != QIDDM_F32 && dtype != QIDDM_F64) return fail(QIDDM_ERR_INVALID, "unknown dtype %d", dtype);
  if (batch < 0 || n_ops < 0) return fail(QIDDM_ERR_INVALID, "negative batch / n_ops");
  return QIDDM_OK;
}

int check_max_blocks(int32_t max_blocks) {
  if (max_blocks < 0) return fail(QIDDM_ERR_INVALID, "negative max_blocks %d", max_blocks);
  return QIDDM_OK;
}

// a program has ops and starts by preparing the state (validator and planners)
int check_program_start(const qiddm_mixed_op_t* program, int32_t n_ops) {
  if (n_ops < 1 || !program) return fail(QIDDM_ERR_INVALID, "empty program");
  if (!is_prep(program[0].kind)) return fail(QIDDM_ERR_INVALID, "the program must start by preparing the state");
  return QIDDM_OK;
}

// a seed or stream offset of QIDDM_MIX_SHOTS: an integer-valued double in [0, 2^53)
inline bool is_counter_word(double v) { return v >= 0.0 && v < 9007199254740992.0 && v == std::floor(v); }  // NaN fails

// the sampled read-out a program ends in (all zeros: none; the ops have been checked)
qiddm::MixedShots shots_of(const qiddm_mixed_op_t* program, int32_t n_ops) {
  qiddm::MixedShots sh{};
  if (n_ops < 1 || !program || program[n_ops - 1].kind != qiddm::kMixShots) return sh;
  const qiddm_mixed_op_t& op = program[n_ops - 1];
  const uint64_t seed = (uint64_t)op.p, offset = (uint64_t)op.scale;
  sh.shots = (uint32_t)op.a;
  sh.seed_lo = (uint32_t)seed;
  sh.seed_hi = (uint32_t)(seed >> 32);
  sh.off_lo = (uint32_t)offset;
  sh.off_hi = (uint32_t)(offset >> 32);
  return sh;
}
inline bool ends_in_shots(const qiddm_mixed_op_t* program, int32_t n_ops) {
  return n_ops > 0 && program && program[n_ops - 1].kind == qiddm::kMixShots;
}

// the reverse sweeps, their workspace sizes and their plan: a program with a sampled read-out is refused (a SHOTS op
// in front of the last op is the validator's fault, reported first)
int refuse_sampled(const qiddm_mixed_op_t* program, int32_t n_ops) {
  if (!program) return QIDDM_OK;
  for (int i = 0; i + 1 < n_ops; ++i)
    if (program[i].kind == qiddm::kMixShots)
      return fail(QIDDM_ERR_INVALID, "op %d: a sampled read-out must be the last op", i);
  if (ends_in_shots(program, n_ops))
    return fail(QIDDM_ERR_UNSUPPORTED, "op %d: a sampled read-out has no gradient (finite shots have no reverse sweep)",
                n_ops - 1);
  return QIDDM_OK;
}

// The reverse sweeps: the rows of two GATE / GATE2 ops are the same rows (their gradients add) or share none -- a
// gradient for rows that partly overlap has no meaning.  Only a GATE2 op or a trainable channel (CHANNEL_FIT: 4 rows,
// CHANNEL2_FIT: 64) can overlap another's partly -- or, in the trajectory engine's reverse sweep, a KRAUS op (its m rows,
// which get a gradient there; the density-matrix entry points never see the kind) or a KRAUS2 op (its 4 m rows).
int refuse_overlapping_gate_rows(const qiddm_mixed_op_t* program, int32_t n_ops) {
  const auto rows_of = [](const qiddm_mixed_op_t& op) -> int64_t {
    return op.kind == qiddm::kMixKraus2 ? 4 * (int64_t)op.p : op.kind == qiddm::kMixKraus ? op.reserved : gate_rows(op.kind);
  };
  bool any = false;
  for (int i = 0; i < n_ops; ++i)
    any = any || is_gate2(program[i].kind) || is_fit(program[i].kind) || program[i].kind == qiddm::kMixKraus2 ||
          (program[i].kind == qiddm::kMixKraus && program[i].reserved > 1);
  if (!any) return QIDDM_OK;
  std::vector<int> gated;
  for (int i = 0; i < n_ops; ++i) {
    const int64_t ni = rows_of(program[i]), ai = program[i].a;
    if (!ni) continue;
    for (int j : gated) {
      const int64_t nj = rows_of(program[j]), aj = program[j].a;
      if (ai < aj + nj && aj < ai + ni && !(ai == aj && ni == nj))
        return fail(QIDDM_ERR_INVALID, "op %d: gate rows %d..%d overlap those of op %d", i, (int)ai, (int)(ai + ni - 1), j);
    }
    gated.push_back(i);
  }
  return QIDDM_OK;
}

// The measurement table a program may end in: QIDDM_MIX_OBS ops and nothing else from the first one on.  Checks all of it
// (position, count, masks, coefficient, columns; no QIDDM_MIX_SHOTS beside it) and counts its terms and columns; a
// program without one gives 0, 0.  `n_qubits` has been checked.
// The density-matrix read-out (one QIDDM_MIX_RHO op, the last) is checked here as well, in front of the table: position,
// keep-mask, a / reserved, no table and no QIDDM_MIX_SHOTS beside it.  It counts as a tail of one op whose columns are the
// 2 * 4^k doubles of the reduced matrix; *rho_mask is its keep-mask (0: the program has none).
int check_obs_tail(int32_t n, const qiddm_mixed_op_t* program, int32_t n_ops, int32_t* n_obs, int32_t* n_cols,
                   int32_t* rho_mask) {
  *n_obs = *n_cols = *rho_mask = 0;
  if (!program) return QIDDM_OK;
  int first = -1, shots = -1, rho = -1;
  for (int i = 0; i < n_ops; ++i) {
    if (program[i].kind == qiddm::kMixObs && first < 0) first = i;
    if (program[i].kind == qiddm::kMixShots && shots < 0) shots = i;
    if (program[i].kind == qiddm::kMixRho && rho < 0) rho = i;
  }
  if (rho >= 0) {
    const qiddm_mixed_op_t& op = program[rho];
    if (rho != n_ops - 1) return fail(QIDDM_ERR_INVALID, "op %d: a density-matrix read-out must be the last op", rho);
    if (op.wire < 1 || op.wire >= ((int64_t)1 << n))
      return fail(QIDDM_ERR_INVALID, "op %d: keep mask %d out of range [1, 2^%d)", rho, op.wire, n);
    if (op.a != 0 || op.reserved != 0)
      return fail(QIDDM_ERR_INVALID, "op %d: a density-matrix read-out takes a 0 and reserved 0 (got %d, %d)", rho, op.a,
                  op.reserved);
    if (first >= 0)
      return fail(QIDDM_ERR_INVALID, "op %d: a density-matrix read-out beside a measurement table (op %d)", rho, first);
    if (shots >= 0)
      return fail(QIDDM_ERR_UNSUPPORTED,
                  "op %d: a sampled read-out beside a density-matrix read-out (shots estimate the diagonal only)", shots);
    *n_obs = 1;
    *n_cols = 2 << (2 * __builtin_popcount((unsigned)op.wire));
    *rho_mask = op.wire;
    return QIDDM_OK;
  }
  if (first < 0) return QIDDM_OK;
  if (shots >= 0)
    return fail(QIDDM_ERR_UNSUPPORTED,
                "op %d: a sampled read-out beside a measurement table (shots of a Pauli word need a basis rotation)", shots);
  for (int i = first; i < n_ops; ++i)
    if (program[i].kind != qiddm::kMixObs)
      return fail(QIDDM_ERR_INVALID, "op %d: only measurement terms may follow the first one (op %d)", i, first);
  if (n_ops - first > QIDDM_MIX_MAX_OBS)
    return fail(QIDDM_ERR_INVALID, "op %d: more than %d measurement terms", first + QIDDM_MIX_MAX_OBS, QIDDM_MIX_MAX_OBS);
  const int64_t d = (int64_t)1 << n;
  int32_t col = 0;
  for (int i = first; i < n_ops; ++i) {
    const qiddm_mixed_op_t& op = program[i];
    if (op.wire < 0 || op.wire >= d) return fail(QIDDM_ERR_INVALID, "op %d: x-mask %d outside [0, 2^%d)", i, op.wire, n);
    if (op.a < 0 || op.a >= d) return fail(QIDDM_ERR_INVALID, "op %d: z-mask %d outside [0, 2^%d)", i, op.a, n);
    if (!std::isfinite(op.p)) return fail(QIDDM_ERR_INVALID, "op %d: measurement coefficient %g not finite", i, op.p);
    if (i == first ? op.reserved != 0 : (op.reserved != col && op.reserved != col + 1))
      return fail(QIDDM_ERR_INVALID, "op %d: output column %d (columns start at 0 and rise by at most 1; the last was %d)", i,
                  op.reserved, i == first ? -1 : col);
    col = op.reserved;
  }
  *n_obs = n_ops - first;
  *n_cols = col + 1;
  return QIDDM_OK;
}

// kind, wire and target / second wire of op i: all the planner reads of an op, and the first thing the validator checks
// of it.  QIDDM_MIX_SHOTS is checked here in full (position, wire / reserved, shots, seed, offset): it indexes no operand.
// `traj`: the trajectory engine's kinds -- QIDDM_MIX_KRAUS and QIDDM_MIX_KRAUS2 are ops, the superoperator kinds and SHOTS are refused.
int check_op_wires(int32_t n, const qiddm_mixed_op_t& op, int i, int32_t n_ops, bool traj = false) {
  if (traj) {
    if (base_kind(op.kind) == qiddm::kMixChannel || base_kind(op.kind) == qiddm::kMixChannel2)
      return fail(QIDDM_ERR_UNSUPPORTED,
                  "op %d: kind %d is a channel given by its superoperator; a trajectory draws Kraus operators: hand a "
                  "one-wire channel over as QIDDM_MIX_KRAUS and a two-wire channel as QIDDM_MIX_KRAUS2, or run the program on qiddm_mixed_forward / "
                  "qiddm_mixed_wide_forward", i, op.kind);
    if (op.kind == qiddm::kMixShots)
      return fail(QIDDM_ERR_UNSUPPORTED,
                  "op %d: a sampled read-out on trajectories; draw shots from rho with qiddm_mixed_forward / "
                  "qiddm_mixed_wide_forward", i);
  }
  if (traj && op.kind == qiddm::kMixKraus) {
    if (op.wire < 0 || op.wire >= n) return fail(QIDDM_ERR_INVALID, "op %d: wire %d out of range", i, op.wire);
    return QIDDM_OK;
  }
  if (traj && op.kind == qiddm::kMixKraus2) {  // GATE2's wires
    if (op.wire < 0 || op.wire >= n) return fail(QIDDM_ERR_INVALID, "op %d: wire %d out of range", i, op.wire);
    if (op.reserved < 0 || op.reserved >= n || op.reserved == op.wire)
      return fail(QIDDM_ERR_INVALID, "op %d: bad second wire %d", i, op.reserved);
    return QIDDM_OK;
  }
  if ((op.kind < qiddm::kMixZero || op.kind > qiddm::kMixDepol) && base_kind(op.kind) != qiddm::kMixChannel &&
      base_kind(op.kind) != qiddm::kMixChannel2 && op.kind != qiddm::kMixShots && !is_gate2(op.kind))
    return fail(QIDDM_ERR_INVALID, "op %d: unknown kind %d", i, op.kind);
  if (is_prep(op.kind)) return QIDDM_OK;
  if (op.kind == qiddm::kMixShots) {
    if (i != n_ops - 1) return fail(QIDDM_ERR_INVALID, "op %d: a sampled read-out must be the last op", i);
    if (op.wire != 0 || op.reserved != 0)
      return fail(QIDDM_ERR_INVALID, "op %d: a sampled read-out takes wire 0 and reserved 0 (got %d, %d)", i, op.wire,
                  op.reserved);
    if (op.a < 1) return fail(QIDDM_ERR_INVALID, "op %d: shots %d out of range", i, op.a);
    if (!is_counter_word(op.p))
      return fail(QIDDM_ERR_INVALID, "op %d: sampled read-out seed %g is not an integer in [0, 2^53)", i, op.p);
    if (!is_counter_word(op.scale))
      return fail(QIDDM_ERR_INVALID, "op %d: sampled read-out offset %g is not an integer in [0, 2^53)", i, op.scale);
    return QIDDM_OK;
  }
  if (op.wire < 0 || op.wire >= n) return fail(QIDDM_ERR_INVALID, "op %d: wire %d out of range", i, op.wire);
  if ((op.kind == qiddm::kMixCZ || op.kind == qiddm::kMixCNOT) && (op.a < 0 || op.a >= n || op.a == op.wire))
    return fail(QIDDM_ERR_INVALID, "op %d: bad target wire %d", i, op.a);
  if ((is_channel2(op.kind) || is_gate2(op.kind)) && (op.reserved < 0 || op.reserved >= n || op.reserved == op.wire))
    return fail(QIDDM_ERR_INVALID, "op %d: bad second wire %d", i, op.reserved);  // n_qubits = 1 cannot hold the op
  return QIDDM_OK;
}

// the arguments the four compute entry points share
struct MixedCall {
  int32_t n_qubits, dtype;
  const qiddm_mixed_op_t* program;
  int32_t n_ops;
  const double* angle_rows;
  int64_t rows_ld;
  int32_t n_rows;
  const double* features;
  int64_t feat_ld;
  int32_t n_features;
  double enc_offset, pad_with;
  const double* gates;
  int32_t n_gates, measure;
  int64_t batch;
  int32_t n_obs = 0, n_cols = 0;  // the measurement table (or the one density-matrix read-out) the program ends in: set by check_call
  int32_t rho_mask = 0;           // the keep-mask of that read-out (0: none)
  int64_t width() const {  // of out / grad_out
    return measure == QIDDM_MEAS_PROBS ? ((int64_t)1 << n_qubits)
           : measure == QIDDM_MEAS_OBS || measure == QIDDM_MEAS_RHO ? n_cols : n_qubits;
  }
  int32_t n_body() const { return n_ops - n_obs; }  // the ops in front of the measurement table / the density-matrix read-out
};

// Everything the compute entry points check about a MixedCall, in the order include/qiddm_hip.h states: wires, dtype,
// negative batch / n_ops, measure; [an empty batch is QIDDM_OK here: nothing further is looked at, the caller returns];
// program, its measurement table (against `measure` too), n_rows / n_gates, angle_rows / rows_ld, gates, then op by op
// against the arguments it indexes.  *embeds: the program has an AMP_EMBED.  Fills in c.n_obs, c.n_cols.
int check_call(MixedCall& c, const Engine& e, bool* embeds) {
  int rc = check_sizes(c.n_qubits, c.dtype, c.batch, c.n_ops, e);
  if (rc != QIDDM_OK) return rc;
  if (c.measure != QIDDM_MEAS_PROBS && c.measure != QIDDM_MEAS_EXPZ && c.measure != QIDDM_MEAS_OBS &&
      c.measure != QIDDM_MEAS_RHO)
    return fail(QIDDM_ERR_INVALID, "unknown measure %d", c.measure);
  if (c.batch == 0) return QIDDM_OK;
  if ((rc = check_program_start(c.program, c.n_ops)) != QIDDM_OK) return rc;
  if ((rc = check_obs_tail(c.n_qubits, c.program, c.n_ops, &c.n_obs, &c.n_cols, &c.rho_mask)) != QIDDM_OK) return rc;
  if (e.traj && (c.measure == QIDDM_MEAS_RHO || c.rho_mask))
    return fail(QIDDM_ERR_UNSUPPORTED,
                "a density-matrix read-out on trajectories: a trajectory holds a pure state; use qiddm_mixed_forward / "
                "qiddm_mixed_wide_forward (measure QIDDM_MEAS_RHO, QIDDM_MIX_RHO)");
  if (e.sampled && (c.measure == QIDDM_MEAS_OBS || c.n_obs > 0)) return refuse_sampled_table();
  if (c.measure == QIDDM_MEAS_RHO && !c.rho_mask)
    return fail(QIDDM_ERR_INVALID, "measure QIDDM_MEAS_RHO needs a density-matrix read-out as the last op (QIDDM_MIX_RHO)");
  if (c.measure != QIDDM_MEAS_RHO && c.rho_mask)
    return fail(QIDDM_ERR_INVALID, "op %d: a density-matrix read-out needs measure QIDDM_MEAS_RHO (got %d)", c.n_body(), c.measure);
  if (c.measure == QIDDM_MEAS_OBS && c.n_obs == 0)
    return fail(QIDDM_ERR_INVALID, "measure QIDDM_MEAS_OBS needs a measurement table: QIDDM_MIX_OBS ops at the end of the program");
  if (c.measure != QIDDM_MEAS_OBS && c.n_obs > 0 && !c.rho_mask)
    return fail(QIDDM_ERR_INVALID, "op %d: a measurement table needs measure QIDDM_MEAS_OBS (got %d)", c.n_body(), c.measure);
  if (c.n_rows < 0 || c.n_gates < 0) return fail(QIDDM_ERR_INVALID, "negative n_rows / n_gates");
  if (c.n_rows > 0 && (!c.angle_rows || c.rows_ld < c.batch)) return fail(QIDDM_ERR_INVALID, "angle_rows missing or rows_ld < batch");
  if (c.n_gates > 0 && !c.gates) return fail(QIDDM_ERR_INVALID, "gates is NULL");
  const int64_t d = (int64_t)1 << c.n_qubits;
  *embeds = false;
  for (int i = 0; i < c.n_body(); ++i) {
    const qiddm_mixed_op_t& op = c.program[i];
    if ((rc = check_op_wires(c.n_qubits, op, i, c.n_body(), e.traj)) != QIDDM_OK) return rc;
    switch (base_kind(op.kind)) {
      case qiddm::kMixKraus:  // (the trajectory engine only: refused above elsewhere) `reserved` rows of gates, one operator each
        if (op.reserved < 1 || op.reserved > qiddm::kTrajMaxKraus)
          return fail(QIDDM_ERR_INVALID, "op %d: %d Kraus operators (1 .. %d are taken)", i, op.reserved, qiddm::kTrajMaxKraus);
        if (op.a < 0 || (int64_t)op.a + op.reserved > c.n_gates)
          return fail(QIDDM_ERR_INVALID, "op %d: Kraus rows %d..%d out of range", i, op.a, (int)((int64_t)op.a + op.reserved - 1));
        break;
      case qiddm::kMixKraus2: {  // (the trajectory engine only) `p` = m operators, four rows of gates each
        if (!(op.p >= 1.0 && op.p <= (double)qiddm::kTrajMaxKraus2) || op.p != std::floor(op.p))  // NaN fails
          return fail(QIDDM_ERR_INVALID, "op %d: %g Kraus operators (1 .. %d are taken)", i, op.p, qiddm::kTrajMaxKraus2);
        const int64_t end = (int64_t)op.a + 4 * (int64_t)op.p;  // one past the last row
        if (op.a < 0 || end > c.n_gates)
          return fail(QIDDM_ERR_INVALID, "op %d: Kraus rows %d..%lld out of range", i, op.a, (long long)(end - 1));
        break;
      }
      case qiddm::kMixAmpEmbed:
        if (!c.features || c.n_features < 1 || c.n_features > d)
          return fail(QIDDM_ERR_INVALID, "Features must be of length %lld or smaller; got length %d.", (long long)d, c.n_features);
        if (c.feat_ld < c.n_features) return fail(QIDDM_ERR_INVALID, "feat_ld %lld < n_features %d", (long long)c.feat_ld, c.n_features);
        *embeds = true;
        break;
      case qiddm::kMixPhase:
      case qiddm::kMixRY:
        if (op.a >= c.n_rows) return fail(QIDDM_ERR_INVALID, "op %d: angle row %d out of range", i, op.a);
        break;
      case qiddm::kMixGate:
        if (op.a < 0 || op.a >= c.n_gates) return fail(QIDDM_ERR_INVALID, "op %d: gate %d out of range", i, op.a);
        break;
      case qiddm::kMixPhaseDamp:
      case qiddm::kMixAmpDamp:
      case qiddm::kMixDepol:
        if (op.a < 0) {
          if (!(op.p >= 0.0 && op.p <= 1.0))
            return fail(QIDDM_ERR_INVALID, "op %d: channel probability %g outside [0, 1]", i, op.p);
        } else {  // the strength is p + scale * angle_rows[a][sample]: device memory, out of the library's sight
          if (op.a >= c.n_rows) return fail(QIDDM_ERR_INVALID, "op %d: angle row %d out of range", i, op.a);
          if (!std::isfinite(op.p) || !std::isfinite(op.scale))
            return fail(QIDDM_ERR_INVALID, "op %d: channel strength p = %g, scale = %g not finite", i, op.p, op.scale);
        }
        break;
      case qiddm::kMixChannel:  // four rows of gates; what they hold is device memory, out of the library's sight
        if (op.a < 0 || (int64_t)op.a + 3 >= c.n_gates)
          return fail(QIDDM_ERR_INVALID, "op %d: channel rows %d..%d out of range", i, op.a, (int)((int64_t)op.a + 3));
        break;
      case qiddm::kMixGate2:  // four rows: the 4 x 4 unitary (device memory: unitarity is the caller's business, as for GATE)
        if (op.a < 0 || (int64_t)op.a + 3 >= c.n_gates)
          return fail(QIDDM_ERR_INVALID, "op %d: gate rows %d..%d out of range", i, op.a, (int)((int64_t)op.a + 3));
        break;
      case qiddm::kMixChannel2:  // 64 rows: the 16 x 16 superoperator
        if (op.a < 0 || (int64_t)op.a + 63 >= c.n_gates)
          return fail(QIDDM_ERR_INVALID, "op %d: channel rows %d..%d out of range", i, op.a, (int)((int64_t)op.a + 63));
        break;
      default:
        break;
    }
  }
  return QIDDM_OK;
}

int check_forward_outputs(const MixedCall& c, const double* out, int64_t out_ld) {
  if (!out) return fail(QIDDM_ERR_INVALID, "out is NULL");
  if (out_ld < c.width()) return fail(QIDDM_ERR_INVALID, "out_ld %lld < %lld", (long long)out_ld, (long long)c.width());
  return QIDDM_OK;
}

int check_backward_outputs(const MixedCall& c, bool embeds, const double* grad_out, int64_t gout_ld,
                           const double* grad_rows, const double* grad_gates, const double* grad_features) {
  if (!grad_out || gout_ld < c.width())
    return fail(QIDDM_ERR_INVALID, "grad_out missing or gout_ld < %lld", (long long)c.width());
  if (c.n_rows > 0 && !grad_rows) return fail(QIDDM_ERR_INVALID, "grad_rows is NULL");
  if (c.n_gates > 0 && !grad_gates) return fail(QIDDM_ERR_INVALID, "grad_gates is NULL");
  if (embeds && !grad_features) return fail(QIDDM_ERR_INVALID, "grad_features is NULL");
  return QIDDM_OK;
}

// ---- what the entry points share after the checks ----------------------------------------------------------------------
// `n_ops`, `n_features`: as the kernels see them (the tile-fused backward runs the live ops only; a backward without
// AMP_EMBED has no features)
qiddm::MixedScalars make_scalars(const MixedCall& c, int32_t n_ops, int32_t n_features, int64_t out_ld, bool in_lds) {
  qiddm::MixedScalars m{};
  m.n = c.n_qubits;
  m.n_ops = n_ops;
  m.n_obs = c.n_obs;  // the table sits behind the n_ops ops of the uploaded program
  m.measure = c.measure;
  m.n_features = n_features;
  m.batch = c.batch;
  m.rows_ld = c.rows_ld;
  m.feat_ld = c.feat_ld;
  m.out_ld = out_ld;
  m.enc_offset = c.enc_offset;
  m.pad_with = c.pad_with;
  m.slab_in_lds = in_lds ? 1 : 0;
  return m;
}

// the program (or the whole head) to the front of the workspace.  `src` is pageable: the copy is staged before the call
// returns, so it may go out of scope
int upload(unsigned char* ws, const void* src, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(ws, src, bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail(QIDDM_ERR_LAUNCH, "program upload failed: %s", hipGetErrorString(e));
  return QIDDM_OK;
}

// ---- one-workgroup engine (qsim_mixed.h): geometry; the arguments have been checked --------------------------------------
constexpr int64_t kMixedMaxBlocks = 256;
constexpr size_t kMixedLdsSlab = 128 * 1024;

struct MixedGeometry {
  int64_t blocks, slab_bytes, off_slabs, total;  // the program sits at offset 0
  bool in_lds;
};

MixedGeometry mixed_geometry(int32_t n, int32_t dtype, int64_t batch, int32_t n_ops) {
  MixedGeometry g;
  g.slab_bytes = slab_bytes(n, dtype);
  g.in_lds = (size_t)g.slab_bytes <= kMixedLdsSlab;
  g.blocks = batch < kMixedMaxBlocks ? batch : kMixedMaxBlocks;
  if (g.blocks < 1) g.blocks = 1;
  g.off_slabs = program_bytes(n_ops);
  g.total = g.off_slabs + (g.in_lds ? 0 : g.blocks * g.slab_bytes);
  return g;
}

// The backward's workspace per workgroup: rho and Lambda unless both fit in LDS, then one snapshot of rho for every
// channel and every state preparation after the first op.
int mixed_backward_geometry(int32_t n, int32_t dtype, int64_t batch, const qiddm_mixed_op_t* program, int32_t n_ops,
                            int32_t max_blocks, MixedGeometry* g, int32_t* n_snaps) {
  if (n_ops > 0 && !program) return fail(QIDDM_ERR_INVALID, "program is NULL");
  *g = mixed_geometry(n, dtype, batch, n_ops);
  int32_t snaps = 0;
  for (int i = 0; i < n_ops; ++i) snaps += (is_channel(program[i].kind) || (i > 0 && is_prep(program[i].kind))) ? 1 : 0;
  *n_snaps = snaps;
  g->in_lds = (size_t)(2 * g->slab_bytes) <= kMixedLdsSlab;
  if (max_blocks > 0 && g->blocks > max_blocks) g->blocks = max_blocks;
  g->total = g->off_slabs + g->blocks * ((g->in_lds ? 0 : 2) + (int64_t)snaps) * g->slab_bytes;
  return QIDDM_OK;
}

int check_workspace(const void* workspace, int64_t workspace_bytes, int64_t need, const char* sizer) {
  if (!workspace || workspace_bytes < need)
    return fail(QIDDM_ERR_INVALID, "workspace of %lld B needed (%s), got %lld", (long long)need, sizer, (long long)workspace_bytes);
  return QIDDM_OK;
}

// ---- tile-fused engine (qsim_mixed_wide.h): geometry and planner ------------------------------------------------------
constexpr int64_t kWideSlabBudget = (int64_t)1 << 30;  // resident slabs per launch: at most 1 GiB

struct WideGeometry {
  int64_t slab_bytes, resident, off_norms, off_slabs, total;
};

WideGeometry wide_geometry(int32_t n, int32_t dtype, int64_t batch, int32_t n_ops) {
  WideGeometry g;
  g.slab_bytes = slab_bytes(n, dtype);
  const int64_t cap = kWideSlabBudget / g.slab_bytes;
  g.resident = batch < cap ? batch : cap;
  if (g.resident < 1) g.resident = 1;
  g.off_norms = program_bytes(n_ops);
  g.off_slabs = g.off_norms + round256(g.resident * 8);
  g.total = g.off_slabs + g.resident * g.slab_bytes;
  return g;
}

// The samples resident in the caller's workspace: a smaller one than `total` (what `sizer` returns) is accepted down to
// one sample's worth, fewer samples are then resident per chunk.
int wide_resident(const void* workspace, int64_t workspace_bytes, int64_t head, int64_t per_sample, int64_t cap,
                  int64_t total, const char* sizer, int64_t* resident) {
  *resident = workspace ? (workspace_bytes - head) / per_sample : 0;
  if (*resident > cap) *resident = cap;
  if (*resident < 1)
    return fail(QIDDM_ERR_INVALID, "workspace of at least %lld B needed (%s: %lld), got %lld", (long long)(head + per_sample),
                sizer, (long long)total, (long long)workspace_bytes);
  return QIDDM_OK;
}

// what the planners check before they read an op
int check_plan_input(int32_t n, const qiddm_mixed_op_t* program, int32_t n_ops) {
  const int rc = check_wires(n, kTileFused);
  return rc != QIDDM_OK ? rc : check_program_start(program, n_ops);
}

struct WidePlan {
  std::vector<int32_t> order;       // program indices, segment after segment
  std::vector<int32_t> op_segment;  // segment of every op
  std::vector<qiddm::WideSegment> segments;
  std::vector<char> seg_channel;    // split_channels: the segment holds channels only
  std::vector<char> seg_level;      // the qiddm::MixedLevel the segment's ops need
  int32_t n_nondiag = 0;
};

// Cuts a program into segments, each executable by one sweep over tiles of six wires.  Two ops commute when they share
// no wire or both act diagonally on vec(rho); an op joins the open segment only if every earlier op that does not
// commute with it is placed (so executing segment after segment, each in program order, is a reordering of commuting
// neighbours only), and a non-diagonal op only if its wires fit the segment's wire set.  Wires n-1 and n-2 are in every
// set (the two lowest column bits stay local: 16-byte accesses).  ZERO / AMP_EMBED open a segment.  The first unplaced
// op always fits an empty segment, so every segment places at least one op, and at least one that is not diagonal.
// `split_channels` (the reverse sweep's plan): a segment takes channels only or no channel at all -- an op of the other
// sort waits like one whose wires do not fit -- so that the state in front of a channel is a whole slab.
// Validates what it reads (wires, program start, kind and wires of every op): the *_plan functions come here directly.
int plan_mixed_wide(int32_t n, const qiddm_mixed_op_t* program, int32_t n_ops, WidePlan* plan,
                    bool split_channels = false) {
  int rc = check_plan_input(n, program, n_ops);
  if (rc != QIDDM_OK) return rc;
  const uint32_t all = (1u << n) - 1u;
  // a sampled read-out (last op) is no op on rho: checked, then left out of every segment.  plan->order holds the
  // n_ops - 1 ops in front of it and its op_segment stays -1.
  // A measurement table (the tail of QIDDM_MIX_OBS terms) likewise: checked, in no sweep, op_segment -1.
  // The density-matrix read-out (QIDDM_MIX_RHO, last op) is a tail of one op to the same effect.
  int32_t n_obs = 0, n_cols = 0, rho_mask = 0;
  if ((rc = check_obs_tail(n, program, n_ops, &n_obs, &n_cols, &rho_mask)) != QIDDM_OK) return rc;
  n_ops -= n_obs;
  const int32_t n_table = n_ops + n_obs, n_all = n_ops;  // n_all: the ops that a sampled read-out must be the last of
  if (ends_in_shots(program, n_ops)) {
    if ((rc = check_op_wires(n, program[n_ops - 1], n_ops - 1, n_all)) != QIDDM_OK) return rc;
    --n_ops;
  }
  std::vector<uint32_t> wires(n_ops);
  plan->n_nondiag = 0;
  for (int i = 0; i < n_ops; ++i) {
    const qiddm_mixed_op_t& op = program[i];
    if ((rc = check_op_wires(n, op, i, n_all)) != QIDDM_OK) return rc;
    wires[i] = is_prep(op.kind) ? all : 1u << op.wire;
    if (op.kind == qiddm::kMixCZ || op.kind == qiddm::kMixCNOT) wires[i] |= 1u << op.a;
    if (is_channel2(op.kind) || is_gate2(op.kind)) wires[i] |= 1u << op.reserved;  // both wires in the tile, as for CNOT
    plan->n_nondiag += is_diag(op.kind) ? 0 : 1;
  }
  plan->order.clear();
  plan->order.reserve(n_ops);
  plan->op_segment.assign(n_table, -1);
  plan->segments.clear();
  plan->seg_channel.clear();
  plan->seg_level.clear();
  std::vector<char> placed(n_ops, 0);
  int first = 0;
  while (first < n_ops) {
    uint32_t set = (1u << (n - 1)) | (1u << (n - 2));
    int count = 2;
    uint32_t blocked_nondiag = 0, blocked_any = 0;  // wires with an earlier unplaced (non-diagonal / any) op
    qiddm::WideSegment sg{};
    sg.op_begin = (int32_t)plan->order.size();
    bool empty = true, channels = false;
    int level = qiddm::kLevelLean;
    for (int i = first; i < n_ops && blocked_nondiag != all; ++i) {
      if (placed[i]) continue;
      const int kind = program[i].kind;
      const uint32_t w = wires[i];
      bool ok;
      int extra = 0;
      if (is_diag(kind)) {
        ok = !(w & blocked_nondiag);
      } else if (is_prep(kind)) {
        ok = !blocked_any && empty;
      } else {
        extra = __builtin_popcount(w & ~set);
        ok = !(w & blocked_any) && count + extra <= qiddm::kWideTileWires;
      }
      if (split_channels && !empty && is_channel(kind) != channels) ok = false;
      if (ok) {
        if (empty) channels = is_channel(kind);
        level = qiddm::mixed_level_join(level, qiddm::mixed_level_of(base_kind(kind)));
        placed[i] = 1;
        plan->order.push_back(i);
        plan->op_segment[i] = (int32_t)plan->segments.size();
        if (extra) {
          set |= w;
          count += extra;
        }
        empty = false;
      } else {
        blocked_any |= w;
        if (!is_diag(kind)) blocked_nondiag |= w;
      }
    }
    while (first < n_ops && placed[first]) ++first;
    sg.op_end = (int32_t)plan->order.size();
    if (sg.op_end == sg.op_begin) return fail(QIDDM_ERR_INVALID, "planner made no progress at op %d", first);
    for (int w = n - 1; w >= 0 && count < qiddm::kWideTileWires; --w)  // fill the tile: lowest index bits first
      if (!(set >> w & 1u)) {
        set |= 1u << w;
        ++count;
      }
    sg.n_tile_bits = 2 * n - qiddm::kWideLocalBits;
    int nl = 0, ng = 0;
    for (int bit = 0; bit < 2 * n; ++bit) {
      const int q = bit % n;
      if (set >> (n - 1 - q) & 1u) sg.lpos[nl++] = (uint8_t)bit;
      else sg.gpos[ng++] = (uint8_t)bit;
    }
    if (nl != qiddm::kWideLocalBits || ng != sg.n_tile_bits || sg.lpos[0] != 0 || sg.lpos[1] != 1)
      return fail(QIDDM_ERR_INVALID, "planner built a malformed tile (%d local, %d tile bits)", nl, ng);
    plan->segments.push_back(sg);
    plan->seg_channel.push_back(channels ? 1 : 0);
    plan->seg_level.push_back((char)level);
  }
  return QIDDM_OK;
}

template <typename T>
int launch_mixed_wide(const WidePlan& plan, const WideGeometry& g, int64_t resident, unsigned char* ws, const MixedCall& c,
                      double* out, qiddm::MixedScalars m, bool embeds, const qiddm::MixedShots& sh, hipStream_t st) {
  // the workgroups that share a sample's reduced density matrix (4^k elements, 256 or -- a wave an element -- 4 a round)
  const int rho_bits = 2 * __builtin_popcount((unsigned)c.rho_mask);
  const int64_t rho_elems = (int64_t)1 << rho_bits, rho_round = (m.n - rho_bits / 2) >= 6 ? 4 : 256;
  const unsigned rho_parts = (unsigned)std::min<int64_t>((rho_elems + rho_round - 1) / rho_round, 256);
  const size_t smem = (size_t)qiddm::kWideTile * sizeof(qiddm::V2<T>);
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  double* norms = reinterpret_cast<double*>(ws + g.off_norms);
  qiddm::V2<T>* slabs = reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs);
  const unsigned tiles = 1u << (2 * m.n - qiddm::kWideLocalBits);
  for (int64_t s0 = 0; s0 < m.batch; s0 += resident) {
    const unsigned chunk = (unsigned)(m.batch - s0 < resident ? m.batch - s0 : resident);
    if (embeds) hipLaunchKernelGGL(qiddm::mixed_wide_norms, dim3(chunk), dim3(256), 0, st, c.features, norms, m, s0);
    for (size_t s = 0; s < plan.segments.size(); ++s) {   // (the sweeps ask for the LDS they use, no more)
      const int rc = for_op_level(plan.seg_level[s], [&](auto level) {
        return launch<qiddm::mixed_wide_sweep<T, decltype(level)::value>>(
            smem, dim3(tiles, chunk), dim3(256), smem, st, "mixed_wide_sweep", prog, c.angle_rows, c.features, c.gates, norms,
            slabs, m, plan.segments[s], s0, (int64_t)0);
      });
      if (rc != QIDDM_OK) return rc;
    }
    if (sh.shots)  // the sampled read-out, keyed by the absolute row s0 + block
      hipLaunchKernelGGL(qiddm::mixed_wide_sampled_read_out<T>, dim3(chunk), dim3(256), 0, st, slabs, out, m, s0, sh);
    else if (m.measure == QIDDM_MEAS_OBS)
      hipLaunchKernelGGL(qiddm::mixed_wide_obs_read_out<T>, dim3(chunk), dim3(256), 0, st, prog, slabs, out, m, s0);
    else if (m.measure == QIDDM_MEAS_RHO)
      hipLaunchKernelGGL(qiddm::mixed_wide_rho_read_out<T>, dim3(rho_parts, chunk), dim3(256), 0, st, slabs, out, m, s0,
                         (uint32_t)c.rho_mask);
    else
      hipLaunchKernelGGL(qiddm::mixed_wide_read_out<T>, dim3(chunk), dim3(256), 0, st, slabs, out, m, s0);
    if (const int rc = launched("mixed_wide"); rc != QIDDM_OK) return rc;
  }
  return QIDDM_OK;
}

// ---- reverse sweep of the tile-fused engine (qsim_mixed_wide_adjoint.h) ------------------------------------------------
// Ops in front of the last state preparation reach no output: the backward plans and runs program[live_begin ..) only,
// and their parameters keep a zero gradient.
struct WideBwdPlan {
  WidePlan plan;                          // of the live ops, channels split off into segments of their own
  int32_t live_begin = 0, n_live = 0;
  int32_t n_obs = 0;                      // terms of the measurement table behind the live ops (in no segment)
  int32_t rho_mask = 0;                   // or the keep-mask of the density-matrix read-out there (n_obs = 1)
  int32_t replay_end = 0;                 // segments [0, replay_end) are replayed: up to the last unitary one
  int32_t n_snaps = 0;                    // channel segments among them
  int32_t n_slots = 0;                    // tile partials per (tile, sample)
  bool embed_live = false;
  bool gate2 = false;                     // a live GATE2: the finalize that sums 32 partials an op
  std::vector<char> seg_graded;           // the (channel) segment holds a native channel with a >= 0 or a trainable channel
  std::vector<char> seg_fit;              // ... a trainable channel: mixed_wide_adjoint_channels_fit
  std::vector<qiddm::WideParam> fit_params;  // the trainable channels, grouped by their rows, program order within a group
  std::vector<int32_t> fit_group_begin;      // n_fit_groups + 1; empty: the program has none
  std::vector<int32_t> slot;              // per sorted live op, -1: no gradient
  std::vector<qiddm::WideParam> params;   // grouped by the parameter they feed, program order within a group
  std::vector<int32_t> group_begin;       // n_groups + 1
};

int plan_mixed_wide_backward(int32_t n, const qiddm_mixed_op_t* program, int32_t n_ops, WideBwdPlan* bp) {
  int rc = check_plan_input(n, program, n_ops);
  int32_t n_cols = 0;
  if (rc == QIDDM_OK) rc = check_obs_tail(n, program, n_ops, &bp->n_obs, &n_cols, &bp->rho_mask);
  if (rc == QIDDM_OK) rc = refuse_sampled(program, n_ops);
  if (rc != QIDDM_OK) return rc;
  n_ops -= bp->n_obs;  // the table has been checked; the plan is of the ops in front of it
  bp->live_begin = 0;
  for (int i = 0; i < n_ops; ++i)
    if (is_prep(program[i].kind)) bp->live_begin = i;
  bp->n_live = n_ops - bp->live_begin;
  const qiddm_mixed_op_t* live = program + bp->live_begin;
  if ((rc = plan_mixed_wide(n, live, bp->n_live, &bp->plan, true)) != QIDDM_OK) return rc;
  const int n_seg = (int)bp->plan.segments.size();
  bp->replay_end = n_seg;
  while (bp->replay_end > 0 && bp->plan.seg_channel[bp->replay_end - 1]) --bp->replay_end;
  // A segment with a graded channel needs the state in front of it.  A trailing segment reads the last replayed set, so
  // the replay goes on up to the last trailing segment that holds one (programs without a graded channel: as before).
  bp->seg_graded.assign(n_seg, 0);
  bp->seg_fit.assign(n_seg, 0);
  for (int i = 0; i < bp->n_live; ++i) {
    if (needs_front(live[i])) bp->seg_graded[bp->plan.op_segment[i]] = 1;
    if (is_fit(live[i].kind)) bp->seg_fit[bp->plan.op_segment[i]] = 1;
  }
  for (int s = n_seg - 1; s > bp->replay_end; --s)
    if (bp->seg_graded[s]) {
      bp->replay_end = s;
      break;
    }
  bp->n_snaps = 0;
  for (int s = 0; s < bp->replay_end; ++s) bp->n_snaps += bp->plan.seg_channel[s];
  bp->embed_live = live[0].kind == qiddm::kMixAmpEmbed;
  bp->slot.assign(bp->n_live, -1);
  bp->n_slots = 0;
  bp->gate2 = false;
  std::vector<std::pair<int64_t, int32_t>> keyed;  // (parameter, sorted position)
  std::vector<std::pair<int64_t, int32_t>> fit_keyed;  // the same for the trainable channels: a finalize of their own
  for (int i = 0; i < bp->n_live; ++i) {
    const qiddm_mixed_op_t& op = live[bp->plan.order[i]];
    const int gate = gate_rows(op.kind);  // 1: GATE (8 tile partials), 4: GATE2, CHANNEL_FIT (32), 64: CHANNEL2_FIT (512)
    if (!gate && !((op.kind == qiddm::kMixPhase || op.kind == qiddm::kMixRY) && op.a >= 0) && !is_graded(op)) continue;
    bp->slot[i] = bp->n_slots;
    bp->n_slots += gate ? 8 * gate : 1;
    if (is_fit(op.kind)) {
      fit_keyed.push_back({((int64_t)gate << 32) | (uint32_t)op.a, i});
      continue;
    }
    bp->gate2 = bp->gate2 || is_gate2(op.kind);
    keyed.push_back({((int64_t)gate << 32) | (uint32_t)op.a, i});
  }
  std::stable_sort(keyed.begin(), keyed.end(),
                   [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) { return x.first < y.first; });
  bp->params.clear();
  bp->group_begin.clear();
  for (size_t k = 0; k < keyed.size(); ++k) {
    const qiddm_mixed_op_t& op = live[bp->plan.order[keyed[k].second]];
    if (k == 0 || keyed[k].first != keyed[k - 1].first) bp->group_begin.push_back((int32_t)k);
    qiddm::WideParam p{};
    p.kind = gate_rows(op.kind) ? op.kind : qiddm::kMixPhase;  // the finalize tells GATE and GATE2 from angles
    p.a = op.a;
    p.slot = bp->slot[keyed[k].second];
    p.scale = op.scale;
    bp->params.push_back(p);
  }
  bp->group_begin.push_back((int32_t)keyed.size());
  bp->fit_params.clear();
  bp->fit_group_begin.clear();
  if (fit_keyed.empty()) return QIDDM_OK;
  std::stable_sort(fit_keyed.begin(), fit_keyed.end(),
                   [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) { return x.first < y.first; });
  for (size_t k = 0; k < fit_keyed.size(); ++k) {
    const qiddm_mixed_op_t& op = live[bp->plan.order[fit_keyed[k].second]];
    if (k == 0 || fit_keyed[k].first != fit_keyed[k - 1].first) bp->fit_group_begin.push_back((int32_t)k);
    qiddm::WideParam p{};
    p.kind = base_kind(op.kind);
    p.a = op.a;
    p.slot = bp->slot[fit_keyed[k].second];
    bp->fit_params.push_back(p);
  }
  bp->fit_group_begin.push_back((int32_t)fit_keyed.size());
  return QIDDM_OK;
}

// Workspace: [sorted live program, measurement table | slot per op | params | group_begin | with trainable channels only:
// their params | their group_begin] then, per resident sample, |v|^2 and
// Re(Lambda_0) v (AMP_EMBED), the tile partials, and 2 + n_snaps slabs.
struct WideBwdGeometry {
  int64_t slab_bytes, aux_bytes, part_bytes, per_sample, resident;
  int64_t off_slot, off_params, off_groups, off_fit_params, off_fit_groups, head, total;
};

WideBwdGeometry wide_backward_geometry(int32_t n, int32_t dtype, int64_t batch, const WideBwdPlan& bp) {
  WideBwdGeometry g;
  g.slab_bytes = slab_bytes(n, dtype);
  g.aux_bytes = round256(8 * (1 + ((int64_t)1 << n)));
  g.part_bytes = round256((int64_t)bp.n_slots * ((int64_t)1 << (2 * n - qiddm::kWideLocalBits)) * 8);
  g.per_sample = g.aux_bytes + g.part_bytes + (2 + (int64_t)bp.n_snaps) * g.slab_bytes;
  const int64_t cap = kWideSlabBudget / g.per_sample;
  g.resident = batch < cap ? batch : cap;
  if (g.resident < 1) g.resident = 1;
  g.off_slot = program_bytes(bp.n_live + bp.n_obs);
  g.off_params = g.off_slot + round256((int64_t)bp.n_live * 4);
  g.off_groups = g.off_params + round256((int64_t)bp.params.size() * (int64_t)sizeof(qiddm::WideParam));
  g.off_fit_params = g.off_groups + round256((int64_t)bp.group_begin.size() * 4);
  g.off_fit_groups = g.off_fit_params + round256((int64_t)bp.fit_params.size() * (int64_t)sizeof(qiddm::WideParam));
  g.head = g.off_fit_groups + round256((int64_t)bp.fit_group_begin.size() * 4);  // both empty: the head as it was
  g.total = g.head + g.resident * g.per_sample;
  return g;
}

template <typename T>
int launch_mixed_wide_backward(const WideBwdPlan& bp, const WideBwdGeometry& g, int64_t resident, unsigned char* ws,
                               const MixedCall& c, const double* grad_out, double* grad_rows, double* grad_gates,
                               double* grad_features, qiddm::MixedScalars m, qiddm::WideBwdScalars b, hipStream_t st) {
  using C = qiddm::V2<T>;
  const size_t tile_bytes = (size_t)qiddm::kWideTile * sizeof(C);
  const dim3 block(256);
  int rc;
  const int n = m.n;
  const size_t DD = (size_t)1 << (2 * n);
  const unsigned D = 1u << n, tiles = 1u << (2 * n - qiddm::kWideLocalBits);
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  const int32_t* slot = reinterpret_cast<const int32_t*>(ws + g.off_slot);
  const qiddm::WideParam* params = reinterpret_cast<const qiddm::WideParam*>(ws + g.off_params);
  const int32_t* group_begin = reinterpret_cast<const int32_t*>(ws + g.off_groups);
  // the per-sample regions, laid out for `resident` samples
  double* norms = reinterpret_cast<double*>(ws + g.head);
  double* lv = norms + resident;
  double* partials = reinterpret_cast<double*>(ws + g.head + resident * g.aux_bytes);
  C* slabs = reinterpret_cast<C*>(ws + g.head + resident * (g.aux_bytes + g.part_bytes));
  const size_t set_stride = (size_t)resident * DD;  // rho sets 0 .. n_snaps, then Lambda
  C* lam = slabs + (size_t)(bp.n_snaps + 1) * set_stride;
  const int n_seg = (int)bp.plan.segments.size();
  const int n_groups = (int)bp.group_begin.size() - 1;
  for (int64_t s0 = 0; s0 < m.batch; s0 += resident) {
    const unsigned chunk = (unsigned)(m.batch - s0 < resident ? m.batch - s0 : resident);
    if (bp.embed_live) hipLaunchKernelGGL(qiddm::mixed_wide_norms, dim3(chunk), dim3(256), 0, st, c.features, norms, m, s0);
    int cur = 0;
    for (int s = 0; s < bp.replay_end; ++s) {
      const bool ch = bp.plan.seg_channel[s] != 0;
      rc = for_op_level(bp.plan.seg_level[s], [&](auto level) {
        return launch<qiddm::mixed_wide_sweep<T, decltype(level)::value>>(
            tile_bytes, dim3(tiles, chunk), block, tile_bytes, st, "mixed_wide_sweep", prog, c.angle_rows, c.features, c.gates,
            norms, slabs + (size_t)cur * set_stride, m, bp.plan.segments[s], s0, (int64_t)(ch ? set_stride : 0));
      });
      if (rc != QIDDM_OK) return rc;
      cur += ch ? 1 : 0;
    }
    qiddm::WideBwdScalars bs = b;
    bs.seed = 1;
    if (m.measure == QIDDM_MEAS_OBS) {  // Lambda_N of the measurement table: a launch of its own, the sweeps read the slab
      hipLaunchKernelGGL(qiddm::mixed_wide_obs_seed<T>, dim3((unsigned)(DD / 1024), chunk), block, 0, st, prog, grad_out, lam,
                         m, bs, s0);
      bs.seed = 0;
    } else if (m.measure == QIDDM_MEAS_RHO) {  // Lambda_N of the density-matrix read-out: likewise
      hipLaunchKernelGGL(qiddm::mixed_wide_rho_seed<T>, dim3((unsigned)(DD / 1024), chunk), block, 0, st, grad_out, lam, m, bs,
                         s0, (uint32_t)bp.rho_mask);
      bs.seed = 0;
    }
    for (int s = n_seg - 1; s >= 0; --s) {
      if (!bp.plan.seg_channel[s]) {
        const auto reverse = [&](auto gate2) {  // the segment holds a two-wire unitary: the instantiation that carries it
          return launch<qiddm::mixed_wide_reverse_sweep<T, decltype(gate2)::value>>(
              2 * tile_bytes, dim3(tiles, chunk), block, 2 * tile_bytes, st, "mixed_wide_reverse_sweep", prog, slot,
              c.angle_rows, c.gates, grad_out, slabs + (size_t)cur * set_stride, lam, partials, m, bp.plan.segments[s], bs, s0);
        };
        rc = qiddm::mixed_has_gate2(bp.plan.seg_level[s]) ? reverse(std::true_type{}) : reverse(std::false_type{});
      } else if (bp.seg_fit[s]) {  // a trainable channel: the state in front of the segment as below
        const C* front = slabs + (size_t)(s < bp.replay_end ? cur - 1 : cur) * set_stride;
        rc = launch<qiddm::mixed_wide_adjoint_channels_fit<T>>(
            2 * tile_bytes, dim3(tiles, chunk), block, 2 * tile_bytes, st, "mixed_wide_adjoint_channels_fit", prog, slot,
            c.angle_rows, c.gates, grad_out, front, lam, partials, m, bp.plan.segments[s], bs, s0);
        if (s < bp.replay_end) --cur;
      } else if (bp.seg_graded[s]) {
        // the state in front of the segment: the set below the one it wrote, or (not replayed) the last replayed set
        const C* front = slabs + (size_t)(s < bp.replay_end ? cur - 1 : cur) * set_stride;
        rc = for_level(bp.plan.seg_level[s], [&](auto level) {
          return launch<qiddm::mixed_wide_adjoint_channels_graded<T, decltype(level)::value>>(
              2 * tile_bytes, dim3(tiles, chunk), block, 2 * tile_bytes, st, "mixed_wide_adjoint_channels_graded", prog, slot,
              c.angle_rows, c.gates, grad_out, front, lam, partials, m, bp.plan.segments[s], bs, s0);
        });
        if (s < bp.replay_end) --cur;
      } else {
        rc = for_level(bp.plan.seg_level[s], [&](auto level) {
          return launch<qiddm::mixed_wide_adjoint_channels<T, decltype(level)::value>>(
              tile_bytes, dim3(tiles, chunk), block, tile_bytes, st, "mixed_wide_adjoint_channels", prog, c.gates, grad_out,
              lam, m, bp.plan.segments[s], bs, s0);
        });
        if (s < bp.replay_end) --cur;
      }
      if (rc != QIDDM_OK) return rc;
      bs.seed = 0;
    }
    if (bp.embed_live) {
      hipLaunchKernelGGL(qiddm::mixed_wide_embed_matvec<T>, dim3(D / 4, chunk), dim3(256), 0, st, lam, c.features, lv, m, s0);
      hipLaunchKernelGGL(qiddm::mixed_wide_embed_grad, dim3(chunk), dim3(256), 0, st, c.features, lv, grad_features, m, s0);
    }
    if (n_groups > 0)
      hipLaunchKernelGGL(bp.gate2 ? qiddm::mixed_wide_grad_finalize<true> : qiddm::mixed_wide_grad_finalize<false>,
                         dim3((n_groups + 3) / 4, chunk), dim3(256), 0, st, params, group_begin, n_groups, c.gates, partials,
                         grad_rows, grad_gates, bp.n_slots, c.n_gates, tiles, m.batch, s0);
    if (!bp.fit_params.empty())  // behind the finalize above: it adds to the rows
      hipLaunchKernelGGL(qiddm::mixed_wide_fit_finalize,
                         dim3(((unsigned)bp.fit_group_begin.size() - 1) * qiddm::kWideFitChunks, chunk), dim3(256), 0, st,
                         reinterpret_cast<const qiddm::WideParam*>(ws + g.off_fit_params),
                         reinterpret_cast<const int32_t*>(ws + g.off_fit_groups), partials, grad_gates, bp.n_slots, c.n_gates,
                         tiles, s0);
    if (rc = launched("mixed_wide backward"); rc != QIDDM_OK) return rc;
  }
  return QIDDM_OK;
}

}  // namespace

extern "C" {

int64_t qiddm_mixed_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_ops) {
  const int rc = check_sizes(n_qubits, dtype, batch, n_ops, kOneWorkgroup);
  if (rc != QIDDM_OK) return rc;
  return mixed_geometry(n_qubits, dtype, batch, n_ops).total;
}

int qiddm_mixed_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                        const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                        int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with, const double* gates,
                        int32_t n_gates, int32_t measure, int64_t batch, double* out, int64_t out_ld, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kOneWorkgroup, &embeds);
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = check_forward_outputs(c, out, out_ld)) != QIDDM_OK) return rc;
  const MixedGeometry g = mixed_geometry(n_qubits, dtype, batch, n_ops);
  if ((rc = check_workspace(workspace, workspace_bytes, g.total, "qiddm_mixed_workspace_bytes")) != QIDDM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  std::vector<qiddm_mixed_op_t> constant(program, program + n_ops);  // the forward knows the constant kinds only
  for (qiddm_mixed_op_t& op : constant) op = constant_op(op);
  if ((rc = upload(ws, constant.data(), (size_t)n_ops * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  const qiddm::MixedShots sh = shots_of(program, n_ops);
  // the ops the kernel walks: a sampled read-out is none of them, nor is the measurement table
  const int32_t n_body = c.n_body() - (sh.shots ? 1 : 0);
  const qiddm::MixedScalars m = make_scalars(c, n_body, n_features, out_ld, g.in_lds);
  const size_t smem = g.in_lds ? (size_t)g.slab_bytes : 0;
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  const int level = program_level(program, n_body) & ~qiddm::kLevelFit;
  return for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return for_op_level(level, [&](auto lv) {
      if (sh.shots)
        return launch<qiddm::mixed_sampled_kernel<T, decltype(lv)::value>>(
            kMaxLds - 8192 /* the kernel also has 5 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
            "mixed_sampled_kernel", prog, angle_rows, features, gates, out,
            reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), m, sh);
      if (measure == QIDDM_MEAS_OBS)
        return launch<qiddm::mixed_obs_kernel<T, decltype(lv)::value>>(
            kMaxLds - 8192 /* the kernel also has 4 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
            "mixed_obs_kernel", prog, angle_rows, features, gates, out, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), m);
      if (measure == QIDDM_MEAS_RHO)
        return launch<qiddm::mixed_rho_kernel<T, decltype(lv)::value>>(
            kMaxLds - 4096 /* the kernel also has 2 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
            "mixed_rho_kernel", prog, angle_rows, features, gates, out, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), m,
            (uint32_t)c.rho_mask);
      return launch<qiddm::mixed_kernel<T, decltype(lv)::value>>(
          kMaxLds - 4096 /* the kernel also has 2 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
          "mixed_kernel", prog, angle_rows, features, gates, out, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), m);
    });
  });
}

int64_t qiddm_mixed_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch,
                                             const qiddm_mixed_op_t* program, int32_t n_ops, int32_t max_blocks) {
  MixedGeometry g;
  int32_t n_snaps = 0;
  int32_t n_obs = 0, n_cols = 0, rho_mask = 0;  // a measurement table (a density-matrix read-out) is checked and takes room in the program head only
  int rc = check_sizes(n_qubits, dtype, batch, n_ops, kOneWorkgroup);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc == QIDDM_OK) rc = check_obs_tail(n_qubits, program, n_ops, &n_obs, &n_cols, &rho_mask);
  if (rc == QIDDM_OK) rc = refuse_sampled(program, n_ops);
  if (rc == QIDDM_OK) rc = mixed_backward_geometry(n_qubits, dtype, batch, program, n_ops, max_blocks, &g, &n_snaps);
  if (rc != QIDDM_OK) return rc;
  return g.total;
}

int qiddm_mixed_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                         const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                         int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with, const double* gates,
                         int32_t n_gates, int32_t measure, int64_t batch, const double* grad_out, int64_t gout_ld,
                         double* grad_rows, double* grad_gates, double* grad_features, int32_t max_blocks,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kOneWorkgroup, &embeds);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);  // refused for an empty batch as well
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = refuse_sampled(program, n_ops)) != QIDDM_OK) return rc;
  if ((rc = refuse_overlapping_gate_rows(program, c.n_body())) != QIDDM_OK) return rc;
  if ((rc = check_backward_outputs(c, embeds, grad_out, gout_ld, grad_rows, grad_gates, grad_features)) != QIDDM_OK) return rc;
  MixedGeometry g;
  int32_t n_snaps = 0;
  if ((rc = mixed_backward_geometry(n_qubits, dtype, batch, program, n_ops, max_blocks, &g, &n_snaps)) != QIDDM_OK) return rc;
  if ((rc = check_workspace(workspace, workspace_bytes, g.total, "qiddm_mixed_backward_workspace_bytes")) != QIDDM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, program, (size_t)n_ops * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  const qiddm::MixedScalars m = make_scalars(c, c.n_body(), embeds ? n_features : 0, 0, g.in_lds);
  qiddm::MixedBwdScalars b{};
  b.gout_ld = gout_ld;
  b.n_rows = n_rows;
  b.n_gates = n_gates;
  b.n_snaps = n_snaps;
  const size_t smem = g.in_lds ? 2 * (size_t)g.slab_bytes : 0;
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  const int level = program_level(program, n_ops);
  return for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    // a program with a trainable channel: the instantiation that carries every case and the rows' gradient beside them
    const auto for_backward_level = [&](auto&& f) {
      constexpr int kAll = qiddm::kLevelChannel2 | qiddm::kLevelGate2 | qiddm::kLevelFit;
      return qiddm::mixed_has_fit(level) ? f(std::integral_constant<int, kAll>{}) : for_op_level(level, f);
    };
    return for_backward_level([&](auto lv) {
      // measure QIDDM_MEAS_OBS: the instantiation that seeds from the measurement table; QIDDM_MEAS_RHO: from the
      // density-matrix read-out's cotangent
      const auto run = [&](auto obs, auto rho) {
        return launch<qiddm::mixed_backward_kernel<T, decltype(lv)::value, decltype(obs)::value, decltype(rho)::value>>(
            kMaxLds - 8192 /* the kernel also has 4.5 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
            "mixed_backward_kernel", prog, angle_rows, features, gates, grad_out, grad_rows, grad_gates,
            embeds ? grad_features : nullptr, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), m, b);
      };
      return measure == QIDDM_MEAS_OBS   ? run(std::true_type{}, std::false_type{})
             : measure == QIDDM_MEAS_RHO ? run(std::false_type{}, std::true_type{})
                                         : run(std::false_type{}, std::false_type{});
    });
  });
}

int64_t qiddm_mixed_wide_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, const qiddm_mixed_op_t* program,
                                         int32_t n_ops) {
  (void)program;  // the workspace does not depend on the plan: program head, |v|^2 per resident sample, resident slabs
  const int rc = check_sizes(n_qubits, dtype, batch, n_ops, kTileFused);
  if (rc != QIDDM_OK) return rc;
  return wide_geometry(n_qubits, dtype, batch, n_ops).total;
}

int qiddm_mixed_wide_plan(int32_t n_qubits, const qiddm_mixed_op_t* program, int32_t n_ops, int32_t* n_sweeps,
                          int32_t* n_nondiag_ops, int32_t* op_segment) {
  WidePlan plan;
  const int rc = plan_mixed_wide(n_qubits, program, n_ops, &plan);
  if (rc != QIDDM_OK) return rc;
  if (n_sweeps) *n_sweeps = (int32_t)plan.segments.size();
  if (n_nondiag_ops) *n_nondiag_ops = plan.n_nondiag;
  if (op_segment)
    for (int i = 0; i < n_ops; ++i) op_segment[i] = plan.op_segment[i];
  return QIDDM_OK;
}

int qiddm_mixed_wide_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                             const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                             int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with, const double* gates,
                             int32_t n_gates, int32_t measure, int64_t batch, double* out, int64_t out_ld, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kTileFused, &embeds);
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = check_forward_outputs(c, out, out_ld)) != QIDDM_OK) return rc;
  const WideGeometry g = wide_geometry(n_qubits, dtype, batch, n_ops);
  WidePlan plan;
  if ((rc = plan_mixed_wide(n_qubits, program, n_ops, &plan)) != QIDDM_OK) return rc;
  int64_t resident;
  rc = wide_resident(workspace, workspace_bytes, g.off_slabs, g.slab_bytes, g.resident, g.total,
                     "qiddm_mixed_wide_workspace_bytes", &resident);
  if (rc != QIDDM_OK) return rc;
  const qiddm::MixedShots sh = shots_of(program, n_ops);
  const int32_t n_body = (int32_t)plan.order.size();  // n_ops, or n_ops - 1 in front of a sampled read-out
  std::vector<qiddm_mixed_op_t> sorted(n_body + c.n_obs);  // the measurement table stays behind the sorted ops
  for (int i = 0; i < n_body; ++i) sorted[i] = constant_op(program[plan.order[i]]);
  for (int i = 0; i < c.n_obs; ++i) sorted[n_body + i] = program[c.n_body() + i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, sorted.data(), sorted.size() * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  const qiddm::MixedScalars m = make_scalars(c, n_body, n_features, out_ld, false);
  return for_dtype(dtype, [&](auto t) {
    return launch_mixed_wide<decltype(t)>(plan, g, resident, ws, c, out, m, embeds, sh, st);
  });
}

int64_t qiddm_mixed_wide_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch,
                                                  const qiddm_mixed_op_t* program, int32_t n_ops) {
  WideBwdPlan bp;
  int rc = plan_mixed_wide_backward(n_qubits, program, n_ops, &bp);
  if (rc == QIDDM_OK) rc = check_sizes(n_qubits, dtype, batch, n_ops, kTileFused);
  if (rc != QIDDM_OK) return rc;
  return wide_backward_geometry(n_qubits, dtype, batch, bp).total;
}

int qiddm_mixed_wide_backward_plan(int32_t n_qubits, const qiddm_mixed_op_t* program, int32_t n_ops,
                                   int32_t* n_replay_sweeps, int32_t* n_reverse_sweeps, int32_t* n_snapshots) {
  WideBwdPlan bp;
  const int rc = plan_mixed_wide_backward(n_qubits, program, n_ops, &bp);
  if (rc != QIDDM_OK) return rc;
  if (n_replay_sweeps) *n_replay_sweeps = bp.replay_end;
  if (n_reverse_sweeps) *n_reverse_sweeps = (int32_t)bp.plan.segments.size();
  if (n_snapshots) *n_snapshots = bp.n_snaps;
  return QIDDM_OK;
}

int qiddm_mixed_wide_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                              const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                              int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                              const double* gates, int32_t n_gates, int32_t measure, int64_t batch,
                              const double* grad_out, int64_t gout_ld, double* grad_rows, double* grad_gates,
                              double* grad_features, void* workspace, int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kTileFused, &embeds);
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = refuse_sampled(program, n_ops)) != QIDDM_OK) return rc;
  if ((rc = refuse_overlapping_gate_rows(program, c.n_body())) != QIDDM_OK) return rc;
  if ((rc = check_backward_outputs(c, embeds, grad_out, gout_ld, grad_rows, grad_gates, grad_features)) != QIDDM_OK) return rc;
  WideBwdPlan bp;
  if ((rc = plan_mixed_wide_backward(n_qubits, program, n_ops, &bp)) != QIDDM_OK) return rc;
  const WideBwdGeometry g = wide_backward_geometry(n_qubits, dtype, batch, bp);
  int64_t resident;
  rc = wide_resident(workspace, workspace_bytes, g.head, g.per_sample, g.resident, g.total,
                     "qiddm_mixed_wide_backward_workspace_bytes", &resident);
  if (rc != QIDDM_OK) return rc;
  // the head in one upload: sorted live program, slots, params, groups
  std::vector<unsigned char> head((size_t)g.head, 0);
  qiddm_mixed_op_t* sorted = reinterpret_cast<qiddm_mixed_op_t*>(head.data());
  for (int i = 0; i < bp.n_live; ++i) sorted[i] = constant_op(program[bp.live_begin + bp.plan.order[i]]);  // trainable channels: marked by their slot
  for (int i = 0; i < bp.n_obs; ++i) sorted[bp.n_live + i] = program[c.n_body() + i];  // the measurement table
  memcpy(head.data() + g.off_slot, bp.slot.data(), bp.slot.size() * 4);
  if (!bp.params.empty()) memcpy(head.data() + g.off_params, bp.params.data(), bp.params.size() * sizeof(qiddm::WideParam));
  memcpy(head.data() + g.off_groups, bp.group_begin.data(), bp.group_begin.size() * 4);
  if (!bp.fit_params.empty()) {
    memcpy(head.data() + g.off_fit_params, bp.fit_params.data(), bp.fit_params.size() * sizeof(qiddm::WideParam));
    memcpy(head.data() + g.off_fit_groups, bp.fit_group_begin.data(), bp.fit_group_begin.size() * 4);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, head.data(), head.size(), st)) != QIDDM_OK) return rc;
  // parameters no live op feeds keep a zero gradient
  hipError_t e = hipSuccess;
  if (n_rows > 0) e = hipMemsetAsync(grad_rows, 0, (size_t)n_rows * (size_t)batch * 8, st);
  if (e == hipSuccess && n_gates > 0) e = hipMemsetAsync(grad_gates, 0, (size_t)batch * (size_t)n_gates * 64, st);
  if (e == hipSuccess && embeds && !bp.embed_live)
    e = hipMemsetAsync(grad_features, 0, (size_t)batch * (size_t)n_features * 8, st);
  if (e != hipSuccess) return fail(QIDDM_ERR_LAUNCH, "gradient reset failed: %s", hipGetErrorString(e));
  const qiddm::MixedScalars m = make_scalars(c, bp.n_live, embeds ? n_features : 0, 0, false);
  qiddm::WideBwdScalars b{};
  b.gout_ld = gout_ld;
  b.n_slots = bp.n_slots;
  return for_dtype(dtype, [&](auto t) {
    return launch_mixed_wide_backward<decltype(t)>(bp, g, resident, ws, c, grad_out, grad_rows, grad_gates, grad_features,
                                                   m, b, st);
  });
}

}  // extern "C"

// ---- trajectories (qsim_traj.h) ----------------------------------------------------------------------------------------
namespace {

constexpr int64_t kTrajLdsBlocks = 2048, kTrajSlabBlocks = 256;  // default grid caps: psi in LDS / in a slab of the workspace

struct TrajGeometry {
  int64_t slots, blocks, psi_bytes, off_acc, off_slabs, total;
  bool in_lds;
};

// S = min(n_traj, 64): a function of n_traj alone, so that the order of every sum is too
inline int64_t traj_slots(int64_t n_traj) { return n_traj < qiddm::kTrajMaxSlots ? n_traj : qiddm::kTrajMaxSlots; }

TrajGeometry traj_geometry(int32_t n, int32_t dtype, int64_t batch, int64_t n_traj, int32_t n_ops, int64_t width,
                           int32_t max_blocks) {
  TrajGeometry g;
  g.slots = traj_slots(n_traj);
  g.psi_bytes = ((int64_t)1 << n) * (dtype == QIDDM_F32 ? 8 : 16);
  g.in_lds = (size_t)g.psi_bytes <= kMixedLdsSlab;
  const int64_t items = std::max<int64_t>(batch, 1) * g.slots;
  g.blocks = std::min<int64_t>(items, g.in_lds ? kTrajLdsBlocks : kTrajSlabBlocks);
  if (max_blocks > 0 && g.blocks > max_blocks) g.blocks = max_blocks;
  g.off_acc = program_bytes(n_ops);
  g.off_slabs = g.off_acc + round256(items * width * 8);
  g.total = g.off_slabs + (g.in_lds ? 0 : g.blocks * g.psi_bytes);
  return g;
}

inline bool has_kraus2(const qiddm_mixed_op_t* program, int32_t n_ops) {
  for (int i = 0; i < n_ops; ++i)
    if (program[i].kind == qiddm::kMixKraus2) return true;
  return false;
}

int check_traj_count(int32_t n_traj) {
  if (n_traj < 1 || n_traj > qiddm::kTrajMaxTraj)
    return fail(QIDDM_ERR_INVALID, "n_traj %d outside 1 .. 2^20", n_traj);
  return QIDDM_OK;
}

}  // namespace

extern "C" {

int64_t qiddm_mixed_traj_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj, int32_t n_ops,
                                         int64_t measure_width, int32_t max_blocks) {
  int rc = check_sizes(n_qubits, dtype, batch, n_ops, kTrajectories);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);
  if (rc == QIDDM_OK && (measure_width < 1 || measure_width > ((int64_t)1 << n_qubits) + QIDDM_MIX_MAX_OBS))
    rc = fail(QIDDM_ERR_INVALID, "measure_width %lld out of range", (long long)measure_width);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc != QIDDM_OK) return rc;
  return traj_geometry(n_qubits, dtype, batch, n_traj, n_ops, measure_width, max_blocks).total;
}

int qiddm_mixed_traj_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                             const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                             int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with, const double* gates,
                             int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj, double seed, double offset,
                             int32_t max_blocks, double* out, int64_t out_ld, double* per_traj, int32_t* branches,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kTrajectories, &embeds);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);  // these four: refused for an empty batch as well
  if (rc == QIDDM_OK && !is_counter_word(seed))
    rc = fail(QIDDM_ERR_INVALID, "trajectory seed %g is not an integer in [0, 2^53)", seed);
  if (rc == QIDDM_OK && !(is_counter_word(offset) && offset < 4294967296.0))
    rc = fail(QIDDM_ERR_INVALID, "trajectory offset %g is not an integer in [0, 2^32)", offset);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = check_forward_outputs(c, out, out_ld)) != QIDDM_OK) return rc;
  const TrajGeometry g = traj_geometry(n_qubits, dtype, batch, n_traj, n_ops, c.width(), max_blocks);
  if ((rc = check_workspace(workspace, workspace_bytes, g.total, "qiddm_mixed_traj_workspace_bytes")) != QIDDM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, program, (size_t)n_ops * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  const qiddm::MixedScalars m = make_scalars(c, c.n_body(), n_features, out_ld, g.in_lds);
  qiddm::TrajScalars tr{};
  tr.n_traj = n_traj;
  tr.n_slots = (int32_t)g.slots;
  tr.width = (int32_t)c.width();
  for (int i = 0; i < c.n_body(); ++i) tr.n_channels += qiddm::traj_is_channel(program[i].kind) ? 1 : 0;
  const uint64_t seed_word = (uint64_t)seed;
  tr.seed_lo = (uint32_t)seed_word;
  tr.seed_hi = (uint32_t)(seed_word >> 32);
  tr.offset = (uint32_t)(uint64_t)offset;
  tr.slab_in_lds = g.in_lds ? 1 : 0;
  const size_t smem = g.in_lds ? (size_t)g.psi_bytes : 0;  // what this wire count needs, no more
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  double* acc = reinterpret_cast<double*>(ws + g.off_acc);
  rc = for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const auto run = [&](auto k2) {  // the kernel with the two-wire Kraus op only for a program that holds one
      return launch<qiddm::mixed_traj_kernel<T, decltype(k2)::value>>(
          kMaxLds - 4096 /* the kernel also has 2.5 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
          "mixed_traj_kernel", prog, angle_rows, features, gates, acc, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs),
          per_traj, branches, m, tr);
    };
    return has_kraus2(program, c.n_body()) ? run(std::true_type{}) : run(std::false_type{});
  });
  if (rc != QIDDM_OK) return rc;
  const int64_t elems = batch * c.width();
  hipLaunchKernelGGL(qiddm::mixed_traj_finalize, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, acc, out, out_ld,
                     batch, tr);
  return launched("mixed_traj_finalize");
}

}  // extern "C"

// ---- trajectories, the reverse sweep (qsim_traj_adjoint.h; include/qiddm_hip_traj_grad.h) ----------------------------------
namespace {

struct TrajBwdGeometry {
  int64_t slots, blocks, psi_bytes, snap_stride, gwidth, off_acc, off_rows, off_snaps, off_slabs, total;
  int32_t n_channels;
  bool in_lds, embeds;
};

// `program` may be NULL with n_ops == 0 (an empty batch)
TrajBwdGeometry traj_backward_geometry(int32_t n, int32_t dtype, int64_t batch, int64_t n_traj,
                                       const qiddm_mixed_op_t* program, int32_t n_ops, int32_t n_rows, int32_t n_gates,
                                       int32_t n_features, int32_t max_blocks) {
  TrajBwdGeometry g;
  g.slots = traj_slots(n_traj);
  g.psi_bytes = ((int64_t)1 << n) * (dtype == QIDDM_F32 ? 8 : 16);
  g.in_lds = (size_t)(2 * g.psi_bytes) <= kMixedLdsSlab;
  g.n_channels = 0;
  g.embeds = false;
  for (int i = 0; program && i < n_ops; ++i) {
    g.n_channels += qiddm::traj_is_channel(program[i].kind) ? 1 : 0;
    g.embeds = g.embeds || program[i].kind == qiddm::kMixAmpEmbed;
  }
  g.gwidth = (int64_t)n_rows + 8 * (int64_t)n_gates + (g.embeds ? n_features : 0);
  g.snap_stride = g.psi_bytes + qiddm::kTrajRecordBytes;
  const int64_t items = std::max<int64_t>(batch, 1) * g.slots;
  int64_t cap = g.in_lds ? kTrajLdsBlocks : kTrajSlabBlocks;  // never more than the forward's
  if (g.n_channels > 0)  // the snapshots of a default launch stay within 1 GiB: the tile-fused engine's residency rule
    cap = std::min<int64_t>(cap, std::max<int64_t>(1, kWideSlabBudget / (g.n_channels * g.snap_stride)));
  g.blocks = std::min<int64_t>(items, cap);
  if (max_blocks > 0 && g.blocks > max_blocks) g.blocks = max_blocks;
  g.off_acc = program_bytes(n_ops);
  g.off_rows = g.off_acc + round256(items * g.gwidth * 8);
  g.off_snaps = g.off_rows + round256(g.blocks * g.gwidth * 8);
  g.off_slabs = g.off_snaps + round256(g.blocks * g.n_channels * g.snap_stride);
  g.total = g.off_slabs + (g.in_lds ? 0 : g.blocks * 2 * g.psi_bytes);
  return g;
}

}  // namespace

extern "C" {

int64_t qiddm_mixed_traj_backward_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj,
                                                  const qiddm_mixed_op_t* program, int32_t n_ops, int32_t n_rows,
                                                  int32_t n_gates, int32_t n_features, int32_t max_blocks) {
  int rc = check_sizes(n_qubits, dtype, batch, n_ops, kTrajectories);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);
  if (rc == QIDDM_OK && (n_rows < 0 || n_gates < 0)) rc = fail(QIDDM_ERR_INVALID, "negative n_rows / n_gates");
  if (rc == QIDDM_OK && n_features < 0) rc = fail(QIDDM_ERR_INVALID, "negative n_features");
  if (rc == QIDDM_OK && n_ops > 0 && !program) rc = fail(QIDDM_ERR_INVALID, "program is NULL");
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc != QIDDM_OK) return rc;
  return traj_backward_geometry(n_qubits, dtype, batch, n_traj, program, n_ops, n_rows, n_gates, n_features, max_blocks).total;
}

int qiddm_mixed_traj_backward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                              const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                              int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with, const double* gates,
                              int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj, double seed, double offset,
                              int32_t max_blocks, const double* grad_out, int64_t gout_ld, double* grad_rows,
                              double* grad_gates, double* grad_features, double* per_traj_grad, int32_t* branches,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kTrajectories, &embeds);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);  // these four: refused for an empty batch as well
  if (rc == QIDDM_OK && !is_counter_word(seed))
    rc = fail(QIDDM_ERR_INVALID, "trajectory seed %g is not an integer in [0, 2^53)", seed);
  if (rc == QIDDM_OK && !(is_counter_word(offset) && offset < 4294967296.0))
    rc = fail(QIDDM_ERR_INVALID, "trajectory offset %g is not an integer in [0, 2^32)", offset);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc != QIDDM_OK || batch == 0) return rc;
  for (int i = 1; i < c.n_body(); ++i)
    if (is_prep(program[i].kind))
      return fail(QIDDM_ERR_UNSUPPORTED,
                  "op %d: a state preparation after op 0 has no reverse sweep on trajectories (nothing in front of it "
                  "reaches the read-out: drop those ops, or use qiddm_mixed_backward up to 8 wires)", i);
  if ((rc = refuse_overlapping_gate_rows(program, c.n_body())) != QIDDM_OK) return rc;
  if ((rc = check_backward_outputs(c, embeds, grad_out, gout_ld, grad_rows, grad_gates, grad_features)) != QIDDM_OK) return rc;
  const TrajBwdGeometry g = traj_backward_geometry(n_qubits, dtype, batch, n_traj, program, n_ops, n_rows, n_gates,
                                                   n_features, max_blocks);
  if ((rc = check_workspace(workspace, workspace_bytes, g.total, "qiddm_mixed_traj_backward_workspace_bytes")) != QIDDM_OK) return rc;
  // no parameter: no gradient to write; the replay still runs when a diagnostic asks for it (branches as the forward's)
  if (g.gwidth == 0 && !branches) return QIDDM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, program, (size_t)n_ops * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  const qiddm::MixedScalars m = make_scalars(c, c.n_body(), embeds ? n_features : 0, 0, g.in_lds);
  qiddm::TrajScalars tr{};
  tr.n_traj = n_traj;
  tr.n_slots = (int32_t)g.slots;
  tr.width = (int32_t)c.width();
  tr.n_channels = g.n_channels;
  const uint64_t seed_word = (uint64_t)seed;
  tr.seed_lo = (uint32_t)seed_word;
  tr.seed_hi = (uint32_t)(seed_word >> 32);
  tr.offset = (uint32_t)(uint64_t)offset;
  tr.slab_in_lds = g.in_lds ? 1 : 0;
  qiddm::TrajBwdScalars b{};
  b.gout_ld = gout_ld;
  b.snap_stride = g.snap_stride;
  b.n_rows = n_rows;
  b.n_gates = n_gates;
  b.n_features = embeds ? n_features : 0;
  b.gwidth = (int32_t)g.gwidth;
  const size_t smem = g.in_lds ? 2 * (size_t)g.psi_bytes : 0;  // what this wire count needs, no more
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  double* acc = reinterpret_cast<double*>(ws + g.off_acc);
  rc = for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const auto run = [&](auto k2) {  // as the forward: programs without the two-wire Kraus op run the kernel that knows none
      return launch<qiddm::mixed_traj_backward_kernel<T, decltype(k2)::value>>(
          kMaxLds - 4096 /* the kernel also has 3 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
          "mixed_traj_backward_kernel", prog, angle_rows, features, gates, grad_out, acc,
          reinterpret_cast<double*>(ws + g.off_rows), ws + g.off_snaps, reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs),
          per_traj_grad, branches, m, tr, b);
    };
    return has_kraus2(program, c.n_body()) ? run(std::true_type{}) : run(std::false_type{});
  });
  if (rc != QIDDM_OK || g.gwidth == 0) return rc;
  const int64_t elems = batch * g.gwidth;
  hipLaunchKernelGGL(qiddm::mixed_traj_grad_finalize, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, acc, grad_rows,
                     grad_gates, grad_features, batch, tr, b);
  return launched("mixed_traj_grad_finalize");
}

}  // extern "C"

// ---- trajectories, finite shots (qsim_traj_shots.h; include/qiddm_hip_traj_shots.h) ---------------------------------------
namespace {

struct TrajShotsGeometry {
  int64_t t_run, slots, blocks, psi_bytes, off_counts, off_flags, off_slabs, total;
  bool in_lds;
};

// `width`: 2^n (PROBS) or n (EXPZ).  T_run = min(n_traj, shots) trajectories draw a shot; the slots are min(T_run, 64)
TrajShotsGeometry traj_shots_geometry(int32_t n, int32_t dtype, int64_t batch, int64_t n_traj, int64_t shots, int32_t n_ops,
                                      int64_t width, int32_t max_blocks) {
  TrajShotsGeometry g;
  g.t_run = std::min<int64_t>(n_traj, shots);
  g.slots = traj_slots(g.t_run);
  g.psi_bytes = ((int64_t)1 << n) * (dtype == QIDDM_F32 ? 8 : 16);
  g.in_lds = (size_t)g.psi_bytes <= kMixedLdsSlab;
  const int64_t rows = std::max<int64_t>(batch, 1), items = rows * g.slots;
  g.blocks = std::min<int64_t>(items, g.in_lds ? kTrajLdsBlocks : kTrajSlabBlocks);
  if (max_blocks > 0 && g.blocks > max_blocks) g.blocks = max_blocks;
  g.off_counts = program_bytes(n_ops);
  g.off_flags = g.off_counts + round256(rows * width * 4);
  g.off_slabs = g.off_flags + round256(rows * 4);
  g.total = g.off_slabs + (g.in_lds ? 0 : g.blocks * g.psi_bytes);
  return g;
}

int check_traj_shots(int32_t n_traj, int32_t shots) {
  if (shots < 1) return fail(QIDDM_ERR_INVALID, "shots %d out of range", shots);
  const int64_t per = ((int64_t)shots + n_traj - 1) / n_traj;
  if (per > qiddm::kTrajShotsPerTraj)
    return fail(QIDDM_ERR_INVALID, "%d shots per trajectory: at most %d (raise n_traj)", (int)per, qiddm::kTrajShotsPerTraj);
  return QIDDM_OK;
}

}  // namespace

extern "C" {

int64_t qiddm_mixed_traj_shots_workspace_bytes(int32_t n_qubits, int32_t dtype, int64_t batch, int32_t n_traj,
                                               int32_t shots, int32_t n_ops, int32_t measure, int32_t max_blocks) {
  int rc = check_sizes(n_qubits, dtype, batch, n_ops, kTrajectoryShots);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);
  if (rc == QIDDM_OK && measure == QIDDM_MEAS_OBS) rc = refuse_sampled_table();
  if (rc == QIDDM_OK && measure != QIDDM_MEAS_PROBS && measure != QIDDM_MEAS_EXPZ)
    rc = measure == QIDDM_MEAS_RHO ? fail(QIDDM_ERR_UNSUPPORTED, "a density-matrix read-out on trajectories: a trajectory holds a pure state")
                                   : fail(QIDDM_ERR_INVALID, "unknown measure %d", measure);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc == QIDDM_OK) rc = check_traj_shots(n_traj, shots);
  if (rc != QIDDM_OK) return rc;
  const int64_t width = measure == QIDDM_MEAS_PROBS ? ((int64_t)1 << n_qubits) : n_qubits;
  return traj_shots_geometry(n_qubits, dtype, batch, n_traj, shots, n_ops, width, max_blocks).total;
}

int qiddm_mixed_traj_shots_forward(int32_t n_qubits, int32_t dtype, const qiddm_mixed_op_t* program, int32_t n_ops,
                                   const double* angle_rows, int64_t rows_ld, int32_t n_rows, const double* features,
                                   int64_t feat_ld, int32_t n_features, double enc_offset, double pad_with,
                                   const double* gates, int32_t n_gates, int32_t measure, int64_t batch, int32_t n_traj,
                                   int32_t shots, double seed, double offset, int32_t max_blocks, double* out,
                                   int64_t out_ld, double* per_traj, int32_t* branches, int32_t* outcomes, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  MixedCall c{n_qubits, dtype, program, n_ops, angle_rows, rows_ld, n_rows, features, feat_ld, n_features,
              enc_offset, pad_with, gates, n_gates, measure, batch};
  bool embeds = false;
  int rc = check_call(c, kTrajectoryShots, &embeds);
  if (rc == QIDDM_OK) rc = check_traj_count(n_traj);  // these six: refused for an empty batch as well
  if (rc == QIDDM_OK && !is_counter_word(seed))
    rc = fail(QIDDM_ERR_INVALID, "trajectory seed %g is not an integer in [0, 2^53)", seed);
  if (rc == QIDDM_OK && !(is_counter_word(offset) && offset < 4294967296.0))
    rc = fail(QIDDM_ERR_INVALID, "trajectory offset %g is not an integer in [0, 2^32)", offset);
  if (rc == QIDDM_OK) rc = check_max_blocks(max_blocks);
  if (rc == QIDDM_OK) rc = check_traj_shots(n_traj, shots);
  if (rc != QIDDM_OK || batch == 0) return rc;
  if ((rc = check_forward_outputs(c, out, out_ld)) != QIDDM_OK) return rc;
  const TrajShotsGeometry g = traj_shots_geometry(n_qubits, dtype, batch, n_traj, shots, n_ops, c.width(), max_blocks);
  if ((rc = check_workspace(workspace, workspace_bytes, g.total, "qiddm_mixed_traj_shots_workspace_bytes")) != QIDDM_OK)
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if ((rc = upload(ws, program, (size_t)n_ops * sizeof(qiddm_mixed_op_t), st)) != QIDDM_OK) return rc;
  // the counts and the flags are one stretch of the workspace: one clear, on the stream, in front of the kernel
  if (const hipError_t e = hipMemsetAsync(ws + g.off_counts, 0, (size_t)(g.off_slabs - g.off_counts), st); e != hipSuccess)
    return fail(QIDDM_ERR_LAUNCH, "count reset failed: %s", hipGetErrorString(e));
  const qiddm::MixedScalars m = make_scalars(c, c.n_body(), n_features, out_ld, g.in_lds);
  qiddm::TrajScalars tr{};
  tr.n_traj = n_traj;
  tr.n_slots = (int32_t)g.slots;
  tr.width = (int32_t)c.width();
  for (int i = 0; i < c.n_body(); ++i) tr.n_channels += qiddm::traj_is_channel(program[i].kind) ? 1 : 0;
  const uint64_t seed_word = (uint64_t)seed;
  tr.seed_lo = (uint32_t)seed_word;
  tr.seed_hi = (uint32_t)(seed_word >> 32);
  tr.offset = (uint32_t)(uint64_t)offset;
  tr.slab_in_lds = g.in_lds ? 1 : 0;
  qiddm::TrajShotScalars sh{};
  sh.shots = shots;
  sh.t_run = (int32_t)g.t_run;
  sh.per = shots / n_traj;
  sh.extra = shots % n_traj;
  const size_t smem = g.in_lds ? (size_t)g.psi_bytes : 0;
  const qiddm::MixedOp* prog = reinterpret_cast<const qiddm::MixedOp*>(ws);
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + g.off_counts);
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + g.off_flags);
  rc = for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const auto run = [&](auto k2) {  // as the analytic launch: the two-wire Kraus op only for a program that holds one
      return launch<qiddm::mixed_traj_shots_kernel<T, decltype(k2)::value>>(
          kMaxLds - 4096 /* the kernel also has 2.7 KiB of static LDS */, dim3((unsigned)g.blocks), dim3(256), smem, st,
          "mixed_traj_shots_kernel", prog, angle_rows, features, gates, counts, flags,
          reinterpret_cast<qiddm::V2<T>*>(ws + g.off_slabs), per_traj, branches, outcomes, m, tr, sh);
    };
    return has_kraus2(program, c.n_body()) ? run(std::true_type{}) : run(std::false_type{});
  });
  if (rc != QIDDM_OK) return rc;
  const int64_t elems = batch * c.width();
  hipLaunchKernelGGL(qiddm::mixed_traj_shots_finalize, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, counts, flags,
                     out, out_ld, batch, (int32_t)c.width(), measure, shots);
  return launched("mixed_traj_shots_finalize");
}

}  // extern "C"

"""The sampling rule of ``qiddm_mixed_traj_shots_forward`` (include/qiddm_hip_traj_shots.h, "THE SAMPLING RULE") in numpy
(a helper module, not a conftest): from a trajectory's float64 weights p (2^n values) to every shot's outcome.

    split       S shots over T trajectories: q = S div T, r = S mod T, s_t = q + (t < r), first_t = t q + min(t, r)
    two levels  G = min(2^n, 256) segments of L = 2^n / G; segment j holds the outcomes j + G i; P_j and C_j are sequential
                sums (``np.cumsum`` adds one element after the other), W = C_{G-1}
    a shot      word (i & 3) of Philox at counter (0x80000000 | (i >> 2), t, b mod 2^32, offset) under the trajectory key;
                v = (word * 2^-32) * W; ``searchsorted(..., side="right")`` counts the sums <= the value, on both levels

Every sum is an IEEE float64 addition in the order the header states, so the outcomes are the kernel's, shot for shot, when
``p`` is the kernel's own ``per_traj``.  Programs and the exact result come from ``_mixed_traj_ref``, Philox from
``_value_domain``; neither is edited.
"""
import numpy as np

from _value_domain import philox4x32_10

SEGMENTS = 256
PER_TRAJ = 1 << 16


def split(shots, n_traj):
    """-> (s_t, first_t) for t = 0 .. n_traj-1, int64 arrays"""
    q, r = divmod(int(shots), int(n_traj))
    t = np.arange(n_traj, dtype=np.int64)
    return q + (t < r), t * q + np.minimum(t, r)


def levels(p):
    """p (2^n,) float64 -> (cum (L, G): the running sums of every segment in ascending i, C (G,), W)"""
    d = p.shape[0]
    g = min(d, SEGMENTS)
    cum = np.cumsum(p.reshape(d // g, g), axis=0)
    c = np.cumsum(cum[-1])
    return cum, c, c[-1]


def words(i, t, row, seed, offset):
    """The 32-bit word of shots `i` (an array) of trajectory t of absolute row `row` -> uint64 array"""
    i = np.asarray(i, dtype=np.uint64)
    out = philox4x32_10((np.uint64(0x80000000) | (i >> np.uint64(2)), np.uint64(t), np.uint64(row & 0xFFFFFFFF), np.uint64(offset)),
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    out = np.stack([np.broadcast_to(np.asarray(w, dtype=np.uint64), i.shape) for w in out])
    return out[(i & np.uint64(3)).astype(np.int64), np.arange(i.shape[0])]


def outcomes_from_values(p, v):
    """The two-level rule for the values v (an array in [0, W)) -> outcomes int64"""
    cum, c, _ = levels(p)
    length, g = cum.shape
    j = np.minimum(np.searchsorted(c, v, side="right"), g - 1)
    u = v - np.where(j > 0, c[np.maximum(j - 1, 0)], 0.0)
    out = np.empty(v.shape[0], dtype=np.int64)
    seg = p.reshape(length, g)
    for s in range(v.shape[0]):
        i = int(np.searchsorted(cum[:, j[s]], u[s], side="right"))
        if i == length:                                        # rounding left none: the last outcome of positive weight
            i = int(np.nonzero(seg[:, j[s]] > 0.0)[0][-1])
        out[s] = j[s] + g * i
    return out


def flat_outcomes(p, v):
    """One ``searchsorted`` over the flat CDF in the same permuted order (exact when every sum is): the distribution the
    two-level rule must reproduce"""
    d = p.shape[0]
    g = min(d, SEGMENTS)
    length = d // g
    order = (np.arange(g)[:, None] + g * np.arange(length)[None, :]).reshape(-1)   # segment by segment, ascending i inside
    flat = np.cumsum(p[order])
    at = np.minimum(np.searchsorted(flat, v, side="right"), d - 1)
    return order[at]


def trajectory_outcomes(p, n_shots, t, row, seed, offset):
    """The outcomes of the `n_shots` shots of trajectory t from its weights p; all -1 when W is invalid or p is NaN (a
    trajectory that stopped at a decision)"""
    if n_shots == 0:
        return np.empty(0, dtype=np.int64)
    if np.isnan(p).any():
        return np.full(n_shots, -1, dtype=np.int64)
    _, _, w = levels(p)
    if not (w > 0.0 and np.isfinite(w)):
        return np.full(n_shots, -1, dtype=np.int64)
    v = (words(np.arange(n_shots), t, row, seed, offset).astype(np.float64) * 2.0 ** -32) * w
    return outcomes_from_values(p, v)


def sample_outcomes(per_traj, shots, n_traj, row, seed, offset):
    """per_traj (T_run, 2^n): one sample's weights -> (shots,) outcomes in global shot order"""
    s_t, first = split(shots, n_traj)
    out = np.empty(shots, dtype=np.int64)
    for t in range(min(n_traj, shots)):
        out[first[t]:first[t] + s_t[t]] = trajectory_outcomes(per_traj[t], int(s_t[t]), t, row, seed, offset)
    return out


# the convergence cases of the GPU test: wires -> (program seed, Philox seed, batch).  Chosen on the CPU: `cpu_convergence`
# (the restatement on its own psi) keeps its worst element below 0.75 of the bound for both settings of (T, S).
CONVERGENCE = {6: (3, 11, 3), 8: (3, 11, 2)}
CONVERGENCE_SETTINGS = ((4096, 4096), (512, 4096))


def convergence_bounds(exact_p, exact_z, n_traj, shots):
    """The derived bounds on |out - exact| for probs and <Z>.  S = T: every element is a mean of S independent Bernoulli
    draws, six standard deviations and one count; S > T: the T trajectories are independent and each one's frequency lies
    in [0, 1], so the variance is at most 1 / (4 T) and 3 / sqrt(T) is six standard deviations.  <Z> = 1 - 2 f doubles both."""
    if shots == n_traj:
        ones = (1.0 - exact_z) / 2.0
        return (6.0 * np.sqrt(np.maximum(exact_p * (1.0 - exact_p), 0.0) / shots) + 1.0 / shots,
                2.0 * (6.0 * np.sqrt(np.maximum(ones * (1.0 - ones), 0.0) / shots) + 1.0 / shots))
    return np.full_like(exact_p, 3.0 / np.sqrt(n_traj)), np.full_like(exact_z, 6.0 / np.sqrt(n_traj))


def cpu_convergence(n, n_traj, shots):
    """The restatement end to end on the CPU: ``_mixed_traj_ref.run`` for psi, this module for the shots ->
    (worst |probs - exact| / bound, worst |<Z> - exact| / bound)"""
    import _mixed_traj_ref as ref
    pseed, seed, batch = CONVERGENCE[n]
    case = ref.noisy_case(n, pseed, batch, strengths=(0.05, 0.5))
    exact_p = ref.exact(case[0], n, *case[1:], "probs")
    exact_z = ref.exact(case[0], n, *case[1:], "expz")
    t_run = min(n_traj, shots)
    _, per, _ = ref.run(case[0], n, *case[1:], "probs", t_run, seed, 0)
    got = [estimates(sample_outcomes(per[b], shots, n_traj, b, seed, 0), n, shots) for b in range(batch)]
    bound_p, bound_z = convergence_bounds(exact_p, exact_z, n_traj, shots)
    return (float((np.abs(np.stack([g[0] for g in got]) - exact_p) / bound_p).max()),
            float((np.abs(np.stack([g[1] for g in got]) - exact_z) / bound_z).max()))


def estimates(outcomes, n, shots):
    """(shots,) outcomes of one sample -> (probs (2^n,), expz (n,)): count / S and (S - 2 ones_w) / S, wire w at bit n-1-w;
    NaN rows when a trajectory was bad"""
    if (outcomes < 0).any():
        return np.full(1 << n, np.nan), np.full(n, np.nan)
    counts = np.bincount(outcomes, minlength=1 << n).astype(np.int64)
    ones = np.array([int(((outcomes >> (n - 1 - w)) & 1).sum()) for w in range(n)], dtype=np.int64)
    return counts / float(shots), (shots - 2 * ones) / float(shots)

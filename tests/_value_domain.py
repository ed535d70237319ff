"""Case tables and references for the value-domain tests (test_value_domain_host.py, test_gpu_value_domain.py).

Not collected by pytest.  Everything here is CPU numpy / torch float64: the pools of data and weight angles at the edges
of the kernels' hand-written sine / cosine, amplitude rows of every awkward kind, and an exact Philox4x32-10 with the
Box-Muller field the training launch generates.

Rule of every comparison built from these tables: the float64 oracle is fed exactly the operand the kernel sees.  For an
"f32" run the inputs are rounded to float32 first and handed to the oracle as float64; large-angle cases use
``enc_scale = 1`` so neither side rounds while forming the angle.
"""
import math

import numpy as np
import torch

PI = math.pi

# ---- tolerances of the kernels' own parity tests (nothing new) ----------------------------------------------------------
F32_TOL = dict(atol=2e-5, rtol=1e-4)                    # test_gpu_tiled.py
F64_TOL = dict(atol=1e-11, rtol=1e-10)
GRAD_TOL = {"f64": 1e-9, "f32": 2e-4}                   # x scale, test_gpu_adjoint.py
GRAD_SCALE_FLOOR = 1e-3                                 # the floor on `scale` of test_gpu_adjoint.py's cz10 / wide cases
DENSE_TOL = {"f32": 5e-5, "f64": 1e-10}                 # test_gpu_nn_parity.py::test_dense_forward_kernel (atol = rtol)
SAMPLE_TOL = {"f32": 1e-4, "f64": 1e-9}                 # test_gpu_nn_parity.py::test_dense_sample_quad_kernel
LEAN_TOL = {0: {"f32": dict(atol=2.5e-4, rtol=2.5e-4), "f64": dict(atol=1e-9, rtol=1e-9)},   # test_gpu_lean_sampler.py
            1: {"f32": dict(atol=5e-5, rtol=0), "f64": dict(atol=1e-10, rtol=0)}}
FIELD_TOL = 1e-5                                        # derived: |n| <= 6.7, sigma 0.2, float32 steps + hardware cosine


# ---- A. data angles -----------------------------------------------------------------------------------------------------
def data_pool(precision):
    """The DATA pool; nextafter(pi/2, +-inf) is taken in the run's dtype."""
    ft = np.float32 if precision == "f32" else np.float64
    h = ft(PI / 2)
    return [0.0, -0.0, 1e-30, -1e-30, PI / 2, -PI / 2, PI, -PI, 2 * PI, -2 * PI, 4 * PI,
            float(np.nextafter(h, ft(np.inf))), float(np.nextafter(h, ft(-np.inf))),
            100.5, -1234.56789, 1e5 + 0.3, 2.0 ** 20 + 0.5, 2.0 ** 29 + 64, -(2.0 ** 29 + 64)]


def as_seen(t, precision):
    """The operand as the kernel of this precision sees it, in a float64 container."""
    return t.to(torch.float32).to(torch.float64) if precision == "f32" else t.to(torch.float64)


def data_batch(n, precision, seed=0):
    """x[b, j] = DATA[(b + 3 j) % len] for b < len (every wire meets every value), plus four rows of U(-1, 1)."""
    pool = data_pool(precision)
    m = len(pool)
    x = torch.tensor([[pool[(b + 3 * j) % m] for j in range(n)] for b in range(m)], dtype=torch.float64)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.cat([x, torch.rand(4, n, generator=g, dtype=torch.float64) * 2 - 1])
    return as_seen(x, precision)


# (n, encoding, imprimitive, measure, L, S): one circuit per code path
CIRCUITS = [
    (3, "rz", "CZ", "expz", 2, 2),          # several samples per wavefront
    (5, "ry", "CNOT", "probs", 1, 2),
    (8, "rz", "CZ", "expz", 3, 2),          # folded tables and folded reverse sweep
    (8, "ry_blocks", "CZ", "probs", 2, 2),
    (10, "rz", "CZ", "probs", 2, 2),        # cz10 reverse sweep
    (10, "rz", "CNOT", "expz", 2, 1),
    (11, "rz", "CNOT", "expz", 2, 1),       # tiled forward, per-gate wide adjoint
    (11, "ry", "CNOT", "probs", 1, 2),
    (12, "rz", "CZ", "expz", 2, 2),         # pass-structured forward and reverse
]
BDOWN_POOL = [8000.25, -1234.5, 100.5, PI, -PI]


def small_weights(n, L, S, seed, N=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, L, S, n, 3, generator=g, dtype=torch.float64) * 0.8


def grad_out(batch, cols, seed):
    return torch.randn(batch, cols, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def dense_case(n, N, L, S, P, seed, batch=7, scale=0.6, bdown=True, pool=None):
    """Operands of a dense net as test_gpu_lean_sampler._case draws them, b_down cycling through ``pool`` (BDOWN_POOL:
    every entry at n >= 5): that is where large angles arise in practice."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, P, generator=g, dtype=torch.float64)
    wd = torch.randn(n, P, generator=g, dtype=torch.float64) / P ** 0.5 * 3
    bd = torch.randn(n, generator=g, dtype=torch.float64)
    wu = torch.randn(P, n, generator=g, dtype=torch.float64) * 0.3
    bu = torch.rand(P, generator=g, dtype=torch.float64)
    w = torch.randn(N, L, S, n, 3, generator=g, dtype=torch.float64) * scale
    if bdown:
        pool = BDOWN_POOL if pool is None else pool
        bd = torch.tensor([pool[j % len(pool)] for j in range(n)], dtype=torch.float64)
    return x, wd, bd, wu, bu, w


# kernel, n, imprimitive, N, L, S, P, post_mode, steps: the dense-net cases of sections A and B
DENSE_CASES = [
    ("forward", 4, "CNOT", 1, 2, 2, 64, 0, 1),        # dense_forward_kernel
    ("forward", 6, "CNOT", 2, 2, 2, 64, 1, 1),
    ("forward", 8, "CZ", 1, 2, 2, 784, 0, 1),         # the one P = 784 case
    ("sample", 3, "CZ", 1, 2, 2, 64, 0, 4),           # dense_quad_kernel
    ("sample", 8, "CZ", 2, 3, 2, 64, 1, 4),
    ("lean", 6, "CZ", 2, 3, 2, 64, 0, 4),             # re-upload
    ("lean", 6, "CZ", 2, 3, 2, 64, 1, 4),
    ("lean", 8, "CZ", 1, 1, 14, 64, 0, 4),            # L = 1
    ("lean", 8, "CZ", 1, 1, 14, 64, 1, 4),
    ("lean", 8, "CZ", 2, 3, 2, 64, 0, 4),
    ("lean", 8, "CZ", 2, 3, 2, 64, 1, 4),
]
NF = 0.8                                              # noise_factor of post_mode 1


def dense_tol(kernel, post, precision):
    """The allclose bound of the kernel's own parity test."""
    if kernel == "forward":
        return dict(atol=DENSE_TOL[precision], rtol=DENSE_TOL[precision])
    if kernel == "sample":
        return dict(atol=SAMPLE_TOL[precision], rtol=SAMPLE_TOL[precision])
    return LEAN_TOL[post][precision]


def bdown_operands(case):
    """Operands of a DENSE_CASES entry with the large b_down.  The P = 784 forward case leaves 8000.25 out: with it the
    oracle's own output moves by 1.2e-12 under +-4 ulp of h, more than 1/100 of qiddm_dense_forward's float64 bound
    (1e-10); without it by 3e-13.  8000.25 stays in the 4-qubit forward case (8e-13) and everywhere else."""
    kernel, n, imp, N, L, S, P, post, steps = case
    pool = BDOWN_POOL[1:] if (kernel, P) == ("forward", 784) else BDOWN_POOL
    return dense_case(n, N, L, S, P, seed=n + L, pool=pool)


# the training-step cases of sections A and B: QIDDM_LL-shaped nets (the data must be re-uploaded to matter)
TRAIN_STEP = dict(L=2, S=2, P=64, B=5, tau=3, shape=(8, 8))


def train_step_case(n, b_down, weights=None):
    """(state dict under the module names of oracle.training.dense_step("ll", ...), x, float32 noise)."""
    t = TRAIN_STEP
    g = torch.Generator().manual_seed(50 + n)
    x, wd, bd, wu, bu, w = dense_case(n, 1, t["L"], t["S"], t["P"], seed=70 + n, batch=t["B"], bdown=b_down)
    noise = torch.randn(t["B"], t["P"], generator=g, dtype=torch.float32) * 0.2 + 0.5
    sd = {"linear_down.weight": wd, "linear_down.bias": bd, "weights1": w if weights is None else weights,
          "linear_up.weight": wu, "linear_up.bias": bu}
    return sd, x, noise


def oracle_dense_steps(x, wd, bd, wu, bu, w, steps, post_mode=0, nf=1.0, imprimitive="CZ", h_hook=None):
    """The sampling loop around the oracle's net: post_mode 0 is x <- net(x), post_mode 1 the "noise"-goal update
    x <- clamp(x - (net(x) - 0.5) * 0.1 * nf, 0, 1).  ``h_hook`` edits the circuit's data angles (host margin test)."""
    from oracle import circuits as oc
    spec = oc.Spec(n=w.shape[-2], encoding="rz", imprimitive=imprimitive, measure="expz")
    cur, refs = x, []
    for _ in range(steps):
        h = cur @ wd.T + bd
        if h_hook is not None:
            h = h_hook(h)
        net = oc.run_circuit(spec, h, w) @ wu.T + bu
        cur = net if post_mode == 0 else torch.clamp(cur - (net - 0.5) * 0.1 * nf, 0, 1)
        refs.append(cur)
    return torch.stack(refs)


def ulp_shift(k, seed=0):
    """h -> h +- k ulp, signs drawn per element."""
    def hook(h):
        g = torch.Generator().manual_seed(seed)
        sign = torch.randint(0, 2, h.shape, generator=g).double() * 2 - 1
        return h + sign * k * torch.from_numpy(np.spacing(np.abs(h.detach().numpy())))
    return hook


# ---- B. weight angles ---------------------------------------------------------------------------------------------------
WEIGHT = [0.0, PI / 2, -PI / 2, PI, -PI, 2 * PI, -2 * PI, 3 * PI, -7 * PI / 2, 4 * PI, 1000.25, -517.5]
# theta of a lean sampler's non-first layers: the pool members whose tangent form the table check accepts
WEIGHT_LEAN_THETA = [t for t in WEIGHT if abs(math.tan(t / 2)) <= 15.9]


def pool_weights(shape, seed, theta_pool=None, theta_pi_layer=None):
    """Every gate takes each of phi, theta, omega from the pool with probability 1/2, otherwise from N(0, 1).
    ``theta_pool``: the pool for theta of every layer but a round's first (lean tables); ``theta_pi_layer`` = (l, s):
    theta = pi on every wire of that layer."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g, dtype=torch.float64)
    take = torch.rand(shape, generator=g) < 0.5
    idx = torch.randint(0, len(WEIGHT), shape, generator=g)
    w = torch.where(take, torch.tensor(WEIGHT, dtype=torch.float64)[idx], w)
    if theta_pool is not None:
        tp = torch.tensor(theta_pool, dtype=torch.float64)
        sub = torch.randint(0, len(tp), shape[:-1], generator=g)
        later = torch.ones(shape[:-1], dtype=torch.bool)
        later[:, 0, 0] = False                                     # a round's first layer takes any angle
        theta = torch.where(take[..., 1], tp[sub], torch.randn(shape[:-1], generator=g, dtype=torch.float64).clamp(-2.9, 2.9))   # tan(1.45) = 8.2
        w[..., 1] = torch.where(later, theta, w[..., 1])
    if theta_pi_layer is not None:
        w[:, theta_pi_layer[0], theta_pi_layer[1], :, 1] = PI
    return w


# ---- C. the lean sampler's accepted band ------------------------------------------------------------------------------
LEAN_BAND_T = [4.0, 8.0, 15.9]
LEAN_BAND_SHAPES = [(8, 1, 1, 14, 64), (6, 2, 3, 2, 64)]           # (n, N, L, S, P)
LEAN_BAND_PLACEMENTS = ["one_gate", "one_layer", "all_layers"]


def lean_band_weights(w, t, placement, seed):
    """theta = +-2 atan(t) on one gate / every gate of one non-first layer / every gate of every non-first layer (a
    round's first layer is generated from (cos, sin) and is not in the tangent form)."""
    g = torch.Generator().manual_seed(seed)
    N, L, S, n, _ = w.shape
    sign = torch.randint(0, 2, (N, L, S, n), generator=g).double() * 2 - 1
    theta = sign * 2 * math.atan(t)
    w = w.clone()
    flat = [(r, l, s) for r in range(N) for l in range(L) for s in range(S) if (l, s) != (0, 0)]
    if placement == "one_gate":
        r, l, s = flat[len(flat) // 2]
        w[r, l, s, n - 2, 1] = theta[r, l, s, n - 2]
    elif placement == "one_layer":
        r, l, s = flat[-1]
        w[r, l, s, :, 1] = theta[r, l, s]
    else:
        for r, l, s in flat:
            w[r, l, s, :, 1] = theta[r, l, s]
    return w


# ---- D. amplitude rows --------------------------------------------------------------------------------------------------
AMP_KINDS = ["mixed", "negative", "onehot_last", "onehot_mid", "constant", "range", "row", "row_x1e3", "row_x1e-3"]


def amp_rows(feat, seed=0):
    """One row per kind of AMP_KINDS, in that order; the last three are one row at three scales."""
    g = torch.Generator().manual_seed(7000 + seed)
    u = lambda: torch.rand(feat, generator=g, dtype=torch.float64)
    rows = [u() * 2 - 1, -(u() + 0.05)]
    for k in (feat - 1, feat // 2):
        r = torch.zeros(feat, dtype=torch.float64)
        # (not 1.0: a row of unit norm takes PennyLane's "already normalised" shortcut, whose gradient has no projection
        #  term -- a branch of the reference, not of the kernels' arithmetic; include/qiddm_hip.h.
        #  amp_unit_rows below are the unit-norm rows, compared with that difference spelled out)
        r[k] = -0.7 if k == feat - 1 else 2.5
        rows.append(r)
    rows.append(torch.full((feat,), 0.37, dtype=torch.float64))
    rows.append(10 ** (u() * 6 - 4) * (torch.randint(0, 2, (feat,), generator=g).double() * 2 - 1))
    base = u() * 2 - 1
    rows += [base, base * 1e3, base * 1e-3]
    return torch.stack(rows)


def amp_unit_rows(feat):
    """One-hot rows of exactly unit norm (+1 in the middle, -1 at index F - 1), with the index of each one."""
    ks = [feat // 2, feat - 1]
    rows = torch.zeros(2, feat, dtype=torch.float64)
    rows[0, ks[0]], rows[1, ks[1]] = 1.0, -1.0
    return rows, ks


def amp_scaled_pairs():
    i = AMP_KINDS.index("row")
    return [(i, i + 1), (i, i + 2)]


# ---- E. the generated noise field ---------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
SEEDS = [1234, 2 ** 32 + 5, 0x7F3A9C5E1B2D4F68]
OFFSETS = [0, 1, 2 ** 32 + 3]
FIELD_SHAPES = [(3, 64, 2), (2, 300, 5)]                          # (B, P, tau)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., Random123).  ctr: four uint32 arrays (broadcastable), key: two.  Returns four."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def noise_field(seed, offset, batch, pixels):
    """The N(0.5, 0.2) field of the training launch: counter = (index lo, index hi, offset lo, offset hi), key =
    (seed lo, seed hi), index = b * pixels + pix; u1 = f32(f32(c0) + 1) * 2^-32, u2 = f32(c1) * 2^-32 with those float32
    roundings, then 0.5 + 0.2 sqrt(-2 ln u1) cos(2 pi u2) in float64.  Returns (batch, pixels) float64."""
    idx = np.arange(batch * pixels, dtype=np.uint64)
    out = philox4x32_10((idx & _MASK, idx >> np.uint64(32), offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = (out[0].astype(np.float32) + np.float32(1.0)).astype(np.float64) * 2.0 ** -32
    u2 = out[1].astype(np.float32).astype(np.float64) * 2.0 ** -32
    z = 0.5 + 0.2 * np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)
    return torch.from_numpy(z.reshape(batch, pixels))


# ---- observed maxima (printed by the GPU tests, collected into profiles/value_domain/observed_maxima.txt) --------------
def report(case, **figures):
    print("[value-domain] " + case + " " + " ".join(f"{k}={v:.3e}" for k, v in figures.items()))

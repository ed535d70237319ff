"""The references of the value-domain tests, checked on the host: the Philox mirror against Random123's known-answer
vectors, the Box-Muller field's distribution and counter layout, and the float64 oracle's own margins at the edges the
GPU tests visit (test_gpu_value_domain.py).  No GPU needed."""
import math

import numpy as np
import pytest
import torch

import _value_domain as vd
from oracle import circuits as oc
from oracle import statevector as sv

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = vd.philox4x32_10([np.array([c]) for c in ctr], key)
    assert tuple(int(v[0]) for v in got) == want


def test_philox_is_vectorised_over_the_counter():
    for ctr, key, want in KAT:
        got = vd.philox4x32_10([np.array([ctr[j], ctr[j] ^ 1]) for j in range(4)], key)
        assert tuple(int(v[0]) for v in got) == want
        assert tuple(int(v[1]) for v in got) != want


def test_noise_field_layout_and_distribution():
    seed, off = vd.SEEDS[2], vd.OFFSETS[2]
    f = vd.noise_field(seed, off, 4, 300)
    assert f.shape == (4, 300) and f.dtype == torch.float64
    # index = b * P + pix: a (4, 300) field is the head of the (8, 150) field of the same key, row-major
    assert torch.equal(f.flatten(), vd.noise_field(seed, off, 8, 150).flatten())
    # one element by hand, through the scalar formula
    b, pix = 2, 17
    c = vd.philox4x32_10([np.array([v]) for v in (b * 300 + pix, 0, off & 0xFFFFFFFF, off >> 32)],
                         (seed & 0xFFFFFFFF, seed >> 32))
    u1 = float(np.float32(np.float32(c[0][0]) + np.float32(1))) * 2.0 ** -32
    u2 = float(np.float32(c[1][0])) * 2.0 ** -32
    assert f[b, pix].item() == pytest.approx(0.5 + 0.2 * math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2), abs=1e-15)
    # every word of key and counter matters: O(0.2) apart, not 1e-5
    for s, o in ((seed ^ (1 << 40), off), (seed ^ 1, off), (seed, off + 1), (seed, off ^ (1 << 32))):
        assert (vd.noise_field(s, o, 4, 300) - f).abs().mean().item() > 0.1
    big = vd.noise_field(1234, 0, 64, 4096).flatten()
    assert abs(big.mean().item() - 0.5) < 2e-3 and abs(big.std().item() - 0.2) < 2e-3
    assert torch.isfinite(big).all() and (big - 0.5).abs().max().item() <= 6.7 * 0.2


def test_pools_are_what_the_issue_lists():
    for prec, ft in (("f32", np.float32), ("f64", np.float64)):
        pool = vd.data_pool(prec)
        assert len(pool) == 19
        x = vd.data_batch(5, prec)
        assert x.shape == (23, 5) and x.dtype == torch.float64
        assert torch.equal(x, vd.as_seen(x, prec))                        # rounding to the run's dtype changes nothing
        want = vd.as_seen(torch.tensor(pool, dtype=torch.float64), prec)
        for j in range(5):                                                # every wire meets every value, signed zeros too
            col = x[:19, j]
            assert sorted(col.tolist()) == sorted(want.tolist())
            assert int((torch.signbit(col) & (col == 0)).sum()) == 1
        up, down = pool[11], pool[12]
        assert down < float(ft(math.pi / 2)) < up and float(ft(up)) == up and float(ft(down)) == down
    assert 2.0 ** 29 + 64 == float(np.float32(2.0 ** 29 + 64))            # the largest angle is a float32 number
    # tangent form: +-pi and 3 pi are outside, quarter turns and whole turns inside
    assert math.pi not in vd.WEIGHT_LEAN_THETA and 3 * math.pi not in vd.WEIGHT_LEAN_THETA
    assert {0.0, math.pi / 2, -math.pi / 2, 2 * math.pi, 4 * math.pi} <= set(vd.WEIGHT_LEAN_THETA)
    w = vd.pool_weights((2, 3, 2, 6, 3), 5, theta_pool=vd.WEIGHT_LEAN_THETA)
    t = torch.tan(w[..., 1] / 2).abs()
    t[:, 0, 0] = 0
    assert t.max().item() <= 15.9
    frac = sum(int((w == v).sum()) for v in set(vd.WEIGHT)) / w.numel()
    assert 0.3 < frac < 0.7
    w = vd.pool_weights((1, 2, 2, 4, 3), 6, theta_pi_layer=(1, 0))
    assert (w[0, 1, 0, :, 1] == math.pi).all()
    for t_ in vd.LEAN_BAND_T:
        for n, N, L, S, _ in vd.LEAN_BAND_SHAPES:
            base = torch.zeros(N, L, S, n, 3, dtype=torch.float64)
            counts = []
            for placement in vd.LEAN_BAND_PLACEMENTS:
                wb = vd.lean_band_weights(base, t_, placement, 1)
                tt = torch.tan(wb[..., 1] / 2).abs()
                assert tt[:, 0, 0].max().item() == 0.0
                assert tt.max().item() == pytest.approx(t_, rel=1e-12)
                counts.append(int((tt > 1).sum()))
            assert counts == [1, n, n * (N * L * S - N)]


@pytest.mark.parametrize("case", vd.DENSE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_oracle_margin_under_4_ulp_of_the_dense_angles(case):
    """h = W_down x + b_down is summed in another order on the device.  For every dense-net case of the GPU tests, with
    its own imprimitive, step count and post_mode: under +-4 ulp on every h of every step the oracle's output moves, element
    by element, by less than 1/100 of the float64 bound that the GPU test applies to that kernel (|h| <= 2^13: an ulp of h
    is at most 2e-12)."""
    kernel, n, imp, N, L, S, P, post, steps = case
    x, wd, bd, wu, bu, w = vd.bdown_operands(case)
    assert (x @ wd.T + bd).abs().max().item() < 2.0 ** 13 and bd.abs().max().item() > 1000
    ref = vd.oracle_dense_steps(x, wd, bd, wu, bu, w, steps, post, vd.NF, imprimitive=imp)
    moved = vd.oracle_dense_steps(x, wd, bd, wu, bu, w, steps, post, vd.NF, imprimitive=imp, h_hook=vd.ulp_shift(4, seed=3))
    tol = vd.dense_tol(kernel, post, "f64")
    room = (tol["atol"] + tol["rtol"] * ref.abs()) / 100
    worst = ((moved - ref).abs() / room).max().item()
    print(f"[value-domain] host margin {case}: moved {(moved - ref).abs().max().item():.3e}, {worst:.3f} of tol / 100")
    assert worst < 1.0, worst


@pytest.mark.parametrize("goal", ["data", "noise"])
@pytest.mark.parametrize("n", [4, 8])
def test_oracle_margin_under_4_ulp_in_the_training_step(n, goal):
    """The same for the oracle step behind the b_down cases of qiddm_train_step, against 1/100 of the float64 bounds of
    test_gpu_capi_strides.py::_check_train_step: loss rel 1e-11, gradients 1e-9 x scale + 1e-14."""
    from oracle.training import dense_step
    t = vd.TRAIN_STEP
    sd, x, noise = vd.train_step_case(n, True)
    assert sd["linear_down.bias"].abs().max().item() > 1000
    loss, grads, _ = dense_step("ll", sd, x, noise, t["tau"], t["shape"], goal, False)
    loss_m, grads_m, _ = dense_step("ll", sd, x, noise, t["tau"], t["shape"], goal, False, h_hook=vd.ulp_shift(4, seed=3))
    figs = {"loss": abs(loss_m / loss - 1) / (1e-11 / 100)}
    for name, g in grads.items():
        figs[name] = (grads_m[name] - g).abs().max().item() / ((1e-9 * g.abs().max().item() + 1e-14) / 100)
    print(f"[value-domain] host margin train_step n={n} {goal}: " + " ".join(f"{k}={v:.3f}" for k, v in figs.items()))
    assert max(figs.values()) < 1.0, figs


@pytest.mark.parametrize("n,feat,pad", [(3, 8, 0.0), (3, 5, 0.1), (8, 200, 0.5), (10, 1024, 0.0), (11, 1500, 0.1)])
def test_oracle_amplitude_rows_are_scale_free(n, feat, pad):
    """The oracle's 1e3-scaled, 1e-3-scaled and unscaled rows agree to 1e-12 (no pad: the normalised state is the same
    vector; the scaled rows are only compared where no pad constant enters), and every row kind is normalised."""
    rows = vd.amp_rows(feat)
    w = vd.small_weights(n, 1, 2, seed=n)
    spec = oc.Spec(n=n, encoding="amplitude", imprimitive="CNOT", measure="probs", pad_with=pad)
    out = oc.run_circuit(spec, rows, w)
    assert torch.isfinite(out).all()
    assert (out.sum(1) - 1).abs().max().item() < 1e-12
    st = sv.amplitude_embedding(rows, n, pad_with=pad, normalize=True)
    assert ((st.abs() ** 2).sum(1) - 1).abs().max().item() < 1e-12
    if feat == 2 ** n:
        for a, b in vd.amp_scaled_pairs():
            assert (out[a] - out[b]).abs().max().item() < 1e-12

"""The QConv2d geometry table (tests/_qconv_geometry.py) without a GPU: its plan columns against
``qiddm_qconv_train_plan``, the coverage it claims (asserted, so that a later edit of the table cannot quietly lose a
path), the conditions its seeded inputs meet, and the oracle's own patch convention against a plain triple loop."""
import ctypes

import pytest
import torch

import _qconv_geometry as qg
from qiddm_amd import _capi, circuit

IDS = [qg.case_id(c) for c in qg.CASES]


def _plan(layer):
    desc = _capi.QConvLayer(layer[0], 0, *layer[1:])
    plan = _capi.QConvTrainPlan()
    rc = _capi.lib().qiddm_qconv_train_plan(ctypes.byref(desc), ctypes.byref(plan))
    assert rc == _capi.QIDDM_OK, _capi.lib().qiddm_last_error()
    return (circuit._QCONV_ROUTES[plan.route], plan.matrix_core, plan.row_channels, plan.bn_fold,
            int(plan.pixel_rows_elems > 0))


def test_the_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS) and {c.group for c in qg.CASES} == set(qg.GROUPS)


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_plan_columns_are_what_the_library_answers(case):
    assert _plan(qg.layer_tuple(case)) == case.plan
    n, f = qg.wires(case), qg.features(case)
    assert n <= 9 and f <= 2 ** n and 2 * case.c_out <= 2 ** n
    assert circuit.qconv_unitary_route(n, case.c_in, case.k, case.c_out) == case.plan[0]
    assert circuit.qconv_bn_foldable((case.batch, case.c_in, *case.hw), n, case.c_out, case.k, case.p) == \
        (bool(case.plan[3]) if case.plan[0] == "thin" else True)


def _any(pred):
    return any(pred(c) for c in qg.CASES)


def test_the_table_covers_the_geometry_it_is_there_for():
    assert _any(lambda c: c.k[0] > c.k[1]) and _any(lambda c: c.k[0] < c.k[1])
    assert _any(lambda c: c.p[0] > c.p[1]) and _any(lambda c: c.p[0] < c.p[1])
    assert _any(lambda c: qg.out_hw(c)[0] < c.hw[0]) and _any(lambda c: qg.out_hw(c)[0] > c.hw[0])
    assert _any(lambda c: qg.out_hw(c)[1] < c.hw[1])
    assert _any(lambda c: c.hw[0] < c.k[0]) and _any(lambda c: c.hw[1] < c.k[1]) and _any(lambda c: c.hw == (1, 1))
    # fewer input channels than the matrix-core walk has waves
    assert {c.c_in for c in qg.CASES if c.plan[:2] == ("thin", 1)} >= {1, 2, 3}
    # a wave of the walk that owns no channel takes C_in < 4 with the 32-feature floor of the matrix-core kernel
    assert _any(lambda c: c.c_in < 4 and c.plan[:2] == ("thin", 1) and qg.features(c) >= 32)
    for sk, sc in qg.STATIC_SHAPES:
        assert _any(lambda c: c.k == (sk, sk) and c.c_in == sc and c.plan[:2] == ("thin", 1)
                    and c.p != ((sk - 1) // 2,) * 2), (sk, sc)
    assert _any(lambda c: c.k == (3, 3) and c.c_in == 16 and c.plan[2] == 32 and c.p != (1, 1))   # QIDDM_TM_SCASE(32, 4, 3, 16)
    assert {c.plan[0] for c in qg.CASES} == {"thin", "gemm"}
    assert {c.plan[:2] for c in qg.CASES} == {("thin", 0), ("thin", 1), ("gemm", 0)}
    assert {(c.plan[2], c.plan[3]) for c in qg.CASES if c.plan[:2] == ("thin", 1)} == {(8, 1), (16, 1), (32, 0)}
    # the extents at which the route changes: 31 taps (halo forward) against more, 32 taps (dx) against more, kw > 15
    assert _any(lambda c: c.k[0] * c.k[1] == 31 and qg.case_forward_variant(c)[0] == "halo")
    assert _any(lambda c: c.k[0] * c.k[1] > 32 and c.plan == qg.MFMA8_FOLD and qg.out_hw(c) == c.hw)
    assert _any(lambda c: max(c.k) == 15 and c.plan[0] == "thin") and _any(lambda c: max(c.k) > 15 and c.plan[0] == "gemm")
    # pixel tiles: 64 (backward, dx) and 128 (forward)
    m = {c.batch * qg.out_hw(c)[0] * qg.out_hw(c)[1] for c in qg.CASES if c.group == "edge"}
    assert m >= {65, 127, 128, 129, 130}


def test_the_table_reaches_every_kernel_variant_the_restated_rule_can_reach():
    halo, dx = set(), set()
    for c_in, c_out, k, p, hw in qg.small_layers():
        plan = _plan((qg.oc.qconv_wires(c_in, c_out, k), 2, c_in, *hw, *k, *p, c_out))
        halo.add(qg.forward_variant(c_in, c_out, k, p, hw, 2))
        got = qg.dx_variant(c_in, k, p, hw, plan)
        assert (got is not None) == bool(plan[4]), ("dx eligibility restated wrongly", c_in, c_out, k, p, hw, plan)
        dx.add(got)
    dx.discard(None)
    reached_fwd = {qg.case_forward_variant(c) for c in qg.CASES}
    reached_dx = {qg.case_dx_variant(c) for c in qg.CASES} - {None}
    for c in qg.CASES:
        assert (qg.case_dx_variant(c) is not None) == bool(c.plan[4]), qg.case_id(c)
    assert halo <= reached_fwd and dx <= reached_dx
    assert qg.HALO_VARIANTS - reached_fwd == qg.UNREACHABLE_HALO == qg.HALO_VARIANTS - halo
    assert qg.DX_VARIANTS - reached_dx == qg.UNREACHABLE_DX == qg.DX_VARIANTS - dx
    assert {v[1] for v in reached_fwd if v[0] == "gemm"} == {0, 1, 2, 3}
    # kernel extents beyond the four bits of the gathering kernels' tap table, in either coordinate: without upsampling
    # (layers the halo forward does not take) and with it (the rectangular group), narrow and 128-channel kernel
    assert {v[1] for v in reached_fwd if v[0] == "gemm" and v[3]} >= {2, 3}
    assert _any(lambda c: c.k[0] > 16 and qg.case_forward_variant(c)[0] == "gemm")
    assert _any(lambda c: c.k[1] > 16 and qg.case_forward_variant(c)[0] == "gemm")
    assert {(qg.gather_packed(c.c_out), c.k[0] > 16, c.k[1] > 16) for c in qg.CASES if c.group == "rect" and max(c.k) > 16} \
        >= {(2, True, False), (2, False, True), (3, False, True)}
    # the fold runs wherever the dx kernel does not: each of its forms on both ways into it (entry and library-GEMM route)
    assert {qg.fold_variant(c.k) for c in qg.CASES if c.plan[0] == "thin" and not c.plan[4]} == {(3, 3), (1, 1), (0, 0)}
    assert {qg.fold_variant(c.k) for c in qg.CASES if c.plan[0] == "gemm"} >= {(3, 3), (0, 0)}
    # the upsampling forward runs on the rectangular and thin-image groups
    assert _any(lambda c: c.group == "rect" and c.k[0] != c.k[1]) and _any(lambda c: c.group == "thin" and c.hw == (1, 1))


@pytest.mark.parametrize("case", qg.CASES, ids=IDS)
def test_inputs_stay_off_the_clamp_kink_and_clamp_a_share_of_the_outputs(case):
    """Conditions on the inputs, from the oracle alone: no scaled probability within 1e-3 of the clamp's kink (ten times
    the band in which float32 cannot tell the side), between 2 % and 50 % of the outputs clamped (the clamp branch runs;
    at most half of the outputs have a zero gradient), and the case's seed is the smallest that meets both."""
    dist, share = qg.input_conditions(case, case.seed)
    assert dist >= qg.KINK_BAND and qg.CLAMPED_SHARE[0] <= share <= qg.CLAMPED_SHARE[1], (dist, share)
    assert not any(qg.conditions_met(case, s) for s in range(case.seed))


@pytest.mark.parametrize("case", sorted((c for c in qg.CASES if c.group == "rect"), key=qg.features)[:2], ids=qg.case_id)
def test_oracle_patch_matrix_is_the_plain_triple_loop(case):
    """``F.unfold``'s rearrangement, as the oracle uses it, against feature (c, di, dj) = x[c, i + di - ph, j + dj - pw]
    (zero outside the image) written as loops: a convention slip in the reference would be invisible otherwise."""
    assert case.k[0] != case.k[1]
    x = qg.inputs(case)[0]
    (kh, kw), (ph, pw), (h, w) = case.k, case.p, case.hw
    ho, wo = qg.out_hw(case)
    cols = torch.nn.functional.unfold(x, kernel_size=case.k, padding=case.p)
    feats = cols.permute(0, 2, 1).reshape(case.batch * ho * wo, case.c_in * kh * kw)
    want = torch.zeros_like(feats)
    for b in range(case.batch):
        for i in range(ho):
            for j in range(wo):
                for c in range(case.c_in):
                    for di in range(kh):
                        for dj in range(kw):
                            ii, jj = i + di - ph, j + dj - pw
                            if 0 <= ii < h and 0 <= jj < w:
                                want[(b * ho + i) * wo + j, (c * kh + di) * kw + dj] = x[b, c, ii, jj]
    assert torch.equal(feats, want)

"""Leading dimensions at the C ABI: every entry point that takes a row stride refuses one that is one element below its
minimum, with QIDDM_ERR_INVALID and a reason that names the argument, before anything is launched.  Host buffers stand
in for device ones (a refused call never reads them); no test here needs a GPU."""
import ctypes

import pytest

from qiddm_amd import _capi

INVALID = -1
_BUF = (ctypes.c_double * 8192)()
PTR = ctypes.cast(_BUF, ctypes.c_void_p).value
BATCH = 3


def _circ(n, enc, imp, meas, feat=0, dtype=_capi.F32, L=1, S=2):
    return _capi.CircuitStruct(n_qubits=n, encoding=enc, imprimitive=imp, measure=meas, n_rounds=1, n_blocks=L,
                               sel_layers=S, n_features=feat or n, dtype=dtype, reserved=0, enc_scale=1.0,
                               enc_offset=0.0, pad_with=0.1)


def _refused(lib, rc, names):
    msg = lib.qiddm_last_error()
    assert rc == INVALID and any(name in msg for name in names), (rc, msg)


RZ_EXPZ = (_capi.ENC_RZ, _capi.IMP_CZ, _capi.MEAS_EXPZ)
RY_PROBS = (_capi.ENC_RY, _capi.IMP_CNOT, _capi.MEAS_PROBS)
AMP_PROBS = (_capi.ENC_AMPLITUDE, _capi.IMP_CNOT, _capi.MEAS_PROBS)


# ---- statevector engine -----------------------------------------------------------------------------------------------
# (wires, family, n_features): a register-resident and a workspace-resident width, both measures, an amplitude row
FORWARD = [(4, RZ_EXPZ, 0), (4, RY_PROBS, 0), (5, AMP_PROBS, 20), (11, RZ_EXPZ, 0), (11, RY_PROBS, 0), (11, AMP_PROBS, 1500)]


def _cols(cs):
    return (1 << cs.n_qubits) if cs.measure == _capi.MEAS_PROBS else cs.n_qubits


@pytest.mark.parametrize("n,family,feat", FORWARD)
def test_forward_refuses_short_rows(hip_lib, n, family, feat):
    cs = _circ(n, *family, feat=feat)
    ws = hip_lib.qiddm_workspace_bytes(ctypes.byref(cs), BATCH, 0)

    def call(in_ld, out_ld):
        return hip_lib.qiddm_forward(ctypes.byref(cs), PTR, BATCH, in_ld, PTR, PTR, out_ld, PTR, ws, None)

    _refused(hip_lib, call(cs.n_features - 1, _cols(cs)), [b"in_ld"])
    _refused(hip_lib, call(cs.n_features, _cols(cs) - 1), [b"out_ld"])
    _refused(hip_lib, call(cs.n_features, 0), [b"out_ld"])


def test_forward_post_refuses_short_rows(hip_lib):
    cs = _circ(5, *AMP_PROBS, feat=20)

    def call(in_ld, out_ld):
        return hip_lib.qiddm_forward_post(ctypes.byref(cs), PTR, BATCH, in_ld, PTR, PTR, out_ld, 20, 20.0, None)

    _refused(hip_lib, call(19, 20), [b"in_ld"])
    _refused(hip_lib, call(20, 19), [b"out_ld"])


@pytest.mark.parametrize("n,family,feat", FORWARD)
def test_forward_shifted_refuses_short_rows(hip_lib, n, family, feat):
    cs = _circ(n, *family, feat=feat)
    ws = hip_lib.qiddm_workspace_bytes(ctypes.byref(cs), BATCH, 2)

    def call(in_ld, g_ld):
        return hip_lib.qiddm_forward_shifted(ctypes.byref(cs), PTR, BATCH, in_ld, PTR, PTR, g_ld, 0, 2, PTR, PTR, ws, None)

    _refused(hip_lib, call(cs.n_features - 1, _cols(cs)), [b"in_ld"])
    _refused(hip_lib, call(cs.n_features, _cols(cs) - 1), [b"g_ld"])


def _adjoint(lib, cs, in_ld, g_ld, gin_ld, gin=PTR):
    if cs.n_qubits > 10:
        ws = lib.qiddm_adjoint_workspace_bytes(ctypes.byref(cs), BATCH)
        return lib.qiddm_backward_adjoint_wide(ctypes.byref(cs), PTR, BATCH, in_ld, PTR, PTR, g_ld, PTR, gin, gin_ld,
                                               PTR, ws, None)
    return lib.qiddm_backward_adjoint(ctypes.byref(cs), PTR, BATCH, in_ld, PTR, PTR, g_ld, PTR, gin, gin_ld, None)


@pytest.mark.parametrize("n,family,feat", [(4, RZ_EXPZ, 0), (5, RY_PROBS, 0), (4, AMP_PROBS, 9), (10, RZ_EXPZ, 0)])
def test_backward_adjoint_refuses_short_rows(hip_lib, n, family, feat):
    cs = _circ(n, *family, feat=feat)
    gin_cols = cs.n_features if cs.encoding == _capi.ENC_AMPLITUDE else n
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features - 1, _cols(cs), gin_cols), [b"in_ld"])
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features, _cols(cs) - 1, gin_cols), [b"g_ld"])
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features, _cols(cs), gin_cols - 1), [b"gin_ld"])


@pytest.mark.parametrize("n,family,feat", [(11, RZ_EXPZ, 0), (11, RY_PROBS, 0), (11, AMP_PROBS, 1500)])
def test_backward_adjoint_wide_refuses_short_rows(hip_lib, n, family, feat):
    """in_ld and gin_ld: the wide entry point used to accept both (it never called the shared input check)."""
    cs = _circ(n, *family, feat=feat)
    gin_cols = cs.n_features if cs.encoding == _capi.ENC_AMPLITUDE else n
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features - 1, _cols(cs), gin_cols), [b"in_ld"])
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features, _cols(cs) - 1, gin_cols), [b"g_ld"])
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features, _cols(cs), gin_cols - 1), [b"gin_ld"])
    # no input gradient asked for: gin_ld is not read, so it is not checked (as for n <= 10) -- and the call goes on to
    # the launch, which this file does not make
    _refused(hip_lib, _adjoint(hip_lib, cs, cs.n_features - 1, _cols(cs), 0, gin=None), [b"in_ld"])


def test_backward_adjoint_wide_keeps_the_null_rule_of_encoding_none(hip_lib):
    """QIDDM_ENC_NONE reads no inputs: NULL and in_ld = 0 pass the input check (the call is then refused for its
    missing workspace, the next check in line)."""
    cs = _circ(11, _capi.ENC_NONE, _capi.IMP_CZ, _capi.MEAS_EXPZ)
    rc = hip_lib.qiddm_backward_adjoint_wide(ctypes.byref(cs), None, BATCH, 0, PTR, PTR, 11, PTR, None, 0, None, 0, None)
    _refused(hip_lib, rc, [b"workspace"])
    cs = _circ(11, *RZ_EXPZ)
    rc = hip_lib.qiddm_backward_adjoint_wide(ctypes.byref(cs), None, BATCH, 11, PTR, PTR, 11, PTR, None, 0, None, 0, None)
    _refused(hip_lib, rc, [b"inputs is NULL"])


def test_amp_embed_rows_refuses_short_rows(hip_lib):
    _refused(hip_lib, hip_lib.qiddm_amp_embed_rows(PTR, BATCH, 19, 20, 5, 0.1, 0.0, PTR, None), [b"x_ld"])


# ---- dense nets, samplers, training step ------------------------------------------------------------------------------
def test_dense_forward_refuses_short_rows(hip_lib):
    for n, batch in ((4, BATCH), (6, 1100)):                # the quad route and dense_forward_kernel
        cs = _circ(n, *RZ_EXPZ)

        def call(x_ld, y_ld):
            return hip_lib.qiddm_dense_forward(ctypes.byref(cs), PTR, batch, x_ld, 20, PTR, PTR, PTR, PTR, PTR, 20, 0, 1.0,
                                               PTR + 4096, y_ld, None)

        _refused(hip_lib, call(19, 20), [b"x_ld"])
        _refused(hip_lib, call(20, 19), [b"y_ld"])


@pytest.mark.parametrize("lean", [False, True])
def test_samplers_refuse_short_strides(hip_lib, lean):
    cs = _circ(8, *RZ_EXPZ)
    feat, y_ld = 20, 23
    floor = BATCH * y_ld - (y_ld - feat)                     # the last row of a step needs no padding behind it

    def call(x_ld, y_ld, step):
        if lean:
            return hip_lib.qiddm_dense_sample_lean(ctypes.byref(cs), PTR, BATCH, x_ld, feat, PTR, PTR, PTR, PTR, 0, 1.0, 3,
                                                   PTR + 4096, y_ld, step, PTR, None)
        return hip_lib.qiddm_dense_sample(ctypes.byref(cs), PTR, BATCH, x_ld, feat, PTR, PTR, PTR, PTR, PTR, feat, 0, 1.0,
                                          3, PTR + 4096, y_ld, step, None, None)

    _refused(hip_lib, call(feat - 1, y_ld, floor), [b"x_ld"])
    _refused(hip_lib, call(feat, feat - 1, BATCH * feat), [b"y_ld"])
    _refused(hip_lib, call(feat, y_ld, floor - 1), [b"y_step_stride"])
    _refused(hip_lib, call(feat, feat, BATCH * feat - 1), [b"y_step_stride"])


def test_train_step_refuses_short_rows(hip_lib):
    cs = _circ(4, *RZ_EXPZ)
    ws = hip_lib.qiddm_train_workspace_bytes(ctypes.byref(cs), BATCH, 20, 4)
    assert ws > 0
    for over, name in ((dict(x_ld=19), b"x_ld"), (dict(noise_ld=19), b"noise_ld")):
        for goal in (0, 1):
            kw = dict(x=PTR, noise=PTR, schedule=PTR, x_ld=20, noise_ld=20, batch=BATCH, pixels=20, tau=4, goal=goal,
                      train_quantum=1, w_down=PTR, b_down=PTR, angles=PTR, w_up=PTR, b_up=PTR, loss=PTR, g_w_down=PTR,
                      g_b_down=PTR, g_angles=PTR, g_w_up=PTR, g_b_up=PTR, recon=None, elem_loss=None, rng_state=None)
            kw.update(over)
            args = _capi.TrainArgs(**kw)
            _refused(hip_lib, hip_lib.qiddm_train_step(ctypes.byref(cs), ctypes.byref(args), PTR, ws, None), [name])


# ---- density-matrix engines -------------------------------------------------------------------------------------------
def _mixed_prog():
    ops = [(_capi.MIX_AMP_EMBED, 0, -1), (_capi.MIX_PHASE, 0, 0), (_capi.MIX_RY, 1, 1), (_capi.MIX_GATE, 2, 0),
           (_capi.MIX_CZ, 0, 1), (_capi.MIX_DEPOL, 1, -1)]
    prog = (_capi.MixedOp * len(ops))()
    for dst, (kind, wire, a) in zip(prog, ops):
        dst.kind, dst.wire, dst.a, dst.reserved, dst.p, dst.scale = kind, wire, a, 0, 0.05, 1.0
    return prog


def _mixed(lib, wide, backward, n, measure, **over):
    prog = _mixed_prog()
    width = (1 << n) if measure == _capi.MEAS_PROBS else n
    feat = 5
    if backward:
        need = (lib.qiddm_mixed_wide_backward_workspace_bytes(n, _capi.F64, BATCH, prog, len(prog)) if wide else
                lib.qiddm_mixed_backward_workspace_bytes(n, _capi.F64, BATCH, prog, len(prog), 0))
    else:
        need = (lib.qiddm_mixed_wide_workspace_bytes(n, _capi.F64, BATCH, prog, len(prog)) if wide else
                lib.qiddm_mixed_workspace_bytes(n, _capi.F64, BATCH, len(prog)))
    assert need > 0
    a = dict(rows_ld=BATCH, feat_ld=feat, out_ld=width)
    a.update(over)
    head = (n, _capi.F64, prog, len(prog), PTR, a["rows_ld"], 2, PTR, a["feat_ld"], feat, 0.0, 0.1, PTR, 1, measure, BATCH,
            PTR, a["out_ld"])
    if not backward:
        fn = lib.qiddm_mixed_wide_forward if wide else lib.qiddm_mixed_forward
        return fn(*head, PTR, need, None)
    if wide:
        return lib.qiddm_mixed_wide_backward(*head, PTR, PTR, PTR, PTR, need, None)
    return lib.qiddm_mixed_backward(*head, PTR, PTR, PTR, 0, PTR, need, None)


@pytest.mark.parametrize("measure", [_capi.MEAS_PROBS, _capi.MEAS_EXPZ])
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("wide,n", [(False, 3), (False, 7), (True, 7)])
def test_mixed_refuses_short_rows(hip_lib, wide, n, backward, measure):
    """out_ld of qiddm_mixed_forward: it used to go unchecked (out_ld = 0 made every sample overwrite row 0)."""
    width = (1 << n) if measure == _capi.MEAS_PROBS else n
    out_name = [b"gout_ld"] if backward else [b"out_ld"]
    _refused(hip_lib, _mixed(hip_lib, wide, backward, n, measure, rows_ld=BATCH - 1), [b"rows_ld"])
    _refused(hip_lib, _mixed(hip_lib, wide, backward, n, measure, feat_ld=4), [b"feat_ld"])
    _refused(hip_lib, _mixed(hip_lib, wide, backward, n, measure, out_ld=width - 1), out_name)
    _refused(hip_lib, _mixed(hip_lib, wide, backward, n, measure, out_ld=0), out_name)

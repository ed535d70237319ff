"""ctypes binding of the C ABI declared in ``include/qiddm_hip.h``.

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``python -m qiddm_amd.build``) into ``qiddm_amd/lib/libqiddm_hip.so``.  There is
no CPU fallback: if the library is missing, ``lib()`` raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

# torch must come first: it ships its own HIP runtime (torch/lib/libamdhip64.so, soname
# libamdhip64.so.7).  Loading ours before torch's would bind the process to /opt/rocm's copy
# and the two runtimes then disagree about the device ("no ROCm-capable device").
import torch  # noqa: F401

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
# QIDDM_HIP_LIB: load another build of the same ABI (kernel experiments); default is the in-tree library
LIB_PATH = os.environ.get("QIDDM_HIP_LIB") or os.path.join(LIB_DIR, "libqiddm_hip.so")

QIDDM_OK = 0
ENC_NONE, ENC_AMPLITUDE, ENC_RZ, ENC_RY, ENC_RY_BLOCKS = 0, 1, 2, 3, 4
IMP_CNOT, IMP_CZ = 0, 1
MEAS_PROBS, MEAS_EXPZ, MEAS_OBS = 0, 1, 2  # MEAS_OBS (density-matrix executor): the MIX_OBS table the program ends in
MEAS_RHO = 8  # density-matrix executor: the reduced density matrix of the wires the MIX_RHO op keeps (3, 4: no measures)
F32, F64 = 0, 1


class CircuitStruct(ctypes.Structure):
    """``qiddm_circuit_t``."""

    _fields_ = [
        ("n_qubits", ctypes.c_int32),
        ("encoding", ctypes.c_int32),
        ("imprimitive", ctypes.c_int32),
        ("measure", ctypes.c_int32),
        ("n_rounds", ctypes.c_int32),
        ("n_blocks", ctypes.c_int32),
        ("sel_layers", ctypes.c_int32),
        ("n_features", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("enc_scale", ctypes.c_double),
        ("enc_offset", ctypes.c_double),
        ("pad_with", ctypes.c_double),
    ]


class QiddmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libqiddm_hip: {msg} (status {code})")
        self.code = code


class TrainArgs(ctypes.Structure):
    """``qiddm_train_args_t``."""

    _fields_ = [
        ("x", ctypes.c_void_p), ("noise", ctypes.c_void_p), ("schedule", ctypes.c_void_p),
        ("x_ld", ctypes.c_int64), ("noise_ld", ctypes.c_int64), ("batch", ctypes.c_int64),
        ("pixels", ctypes.c_int32), ("tau", ctypes.c_int32), ("goal", ctypes.c_int32),
        ("train_quantum", ctypes.c_int32),
        ("w_down", ctypes.c_void_p), ("b_down", ctypes.c_void_p), ("angles", ctypes.c_void_p),
        ("w_up", ctypes.c_void_p), ("b_up", ctypes.c_void_p),
        ("loss", ctypes.c_void_p),
        ("g_w_down", ctypes.c_void_p), ("g_b_down", ctypes.c_void_p), ("g_angles", ctypes.c_void_p),
        ("g_w_up", ctypes.c_void_p), ("g_b_up", ctypes.c_void_p),
        ("recon", ctypes.c_void_p), ("elem_loss", ctypes.c_void_p), ("rng_state", ctypes.c_void_p),
    ]


MIX_ZERO, MIX_AMP_EMBED, MIX_PHASE, MIX_RY, MIX_GATE, MIX_CZ, MIX_CNOT, MIX_PHASE_DAMP, MIX_AMP_DAMP, MIX_DEPOL = range(10)
MIX_SHOTS = 12  # last op only: the read-out is sampled; `a` = shots, `p` = seed, `scale` = stream offset
MIX_CHANNEL = 16  # general one-wire channel: `a` = first of four gate rows holding the superoperator
# tail of the program: one term of the measurement table, `p` times the Pauli word with x-mask `wire` and z-mask `a`
# (wire w at bit n-1-w), output column `reserved`; at most MIX_MAX_OBS terms
MIX_OBS, MIX_MAX_OBS = 20, 256
MIX_GATE2 = 24  # two-wire unitary: `a` = first of four gate rows (the 4 x 4 matrix), `reserved` = the second wire
MIX_RHO = 28  # last op only: the read-out keeps the wires of the mask `wire` (wire w at bit n-1-w); `a`, `reserved` = 0
MIX_CHANNEL2 = 32  # general two-wire channel: `a` = first of 64 gate rows (16 x 16), `reserved` = the second wire
# 16 k + 2: the k-wire channel whose rows get a gradient from the reverse sweeps (operands and forward as 16 / 32)
MIX_CHANNEL_FIT, MIX_CHANNEL2_FIT = 18, 34
# trajectory engine only: a one-wire channel by its Kraus operators, `reserved` = m <= MIX_MAX_KRAUS of them in the gate
# rows `a` .. `a` + m - 1
MIX_KRAUS, MIX_MAX_KRAUS = 40, 8
# trajectory engine only: a two-wire channel by its Kraus operators on (`wire`, `reserved`), `p` = m <= MIX_MAX_KRAUS2 of
# them, operator k in the gate rows `a` + 4k .. `a` + 4k + 3 (MIX_GATE2's layout)
MIX_KRAUS2, MIX_MAX_KRAUS2 = 48, 16
TRAJ_MAX, TRAJ_SLOTS = 1 << 20, 64  # most trajectories per sample; the slots of the mean are min(n_traj, TRAJ_SLOTS)


class MixedOp(ctypes.Structure):
    """``qiddm_mixed_op_t``.  ``reserved`` is 0 except for ``MIX_CHANNEL2``, ``MIX_GATE2`` and ``MIX_KRAUS2``, which read their second wire there, and ``MIX_OBS``, which reads
    its output column there."""

    _fields_ = [("kind", ctypes.c_int32), ("wire", ctypes.c_int32), ("a", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("p", ctypes.c_double), ("scale", ctypes.c_double)]


class BatchNormStruct(ctypes.Structure):
    """``qiddm_batchnorm_t``."""

    _fields_ = [("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("running_mean", ctypes.c_void_p),
                ("running_var", ctypes.c_void_p), ("eps", ctypes.c_double)]


class AdamTensor(ctypes.Structure):
    """``qiddm_adam_tensor_t``."""

    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("step", ctypes.c_void_p), ("numel", ctypes.c_int64), ("dtype", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class QConvLayer(ctypes.Structure):
    """``qiddm_qconv_layer_t``."""

    _fields_ = [("n_qubits", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [
        (name, ctypes.c_int64) for name in ("batch", "in_channels", "height", "width", "kh", "kw", "pad_h", "pad_w",
                                            "out_channels")]


class QConvTrainPlan(ctypes.Structure):
    """``qiddm_qconv_train_plan_t``."""

    _fields_ = [("route", ctypes.c_int32), ("row_channels", ctypes.c_int32), ("matrix_core", ctypes.c_int32),
                ("bn_fold", ctypes.c_int32), ("n_partials", ctypes.c_int64), ("pixel_rows_elems", ctypes.c_int64)]


_P = ctypes.POINTER(CircuitStruct)
_int, _i32, _i64, _dbl, _vp = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
_ops, _i32p = ctypes.POINTER(MixedOp), ctypes.POINTER(ctypes.c_int32)
# argument runs that several entry points share, in the header's order
_stream = [_vp]
_ws = [_vp, _i64]                                          # workspace, workspace_bytes
_image = [_i64] * 8                                        # batch, in_channels, height, width, kh, kw, pad_h, pad_w
_table_of = [_P, _vp, _vp] + _stream                       # circ, angles -> one device table
_dense = [_P, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _dbl]     # circ, x .. noise_factor
_adjoint = [_P, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64]                    # circ, inputs .. gin_ld
_layer = ctypes.POINTER(QConvLayer)
_norm_back = [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp] + _ws + _stream
_planes = [_vp, _i64, _i64, _i64]                          # x, planes, height, width
# what the four compute entry points of the density-matrix executor share: n_qubits .. batch
_mixed = [_i32, _i32, _ops, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _dbl, _dbl, _vp, _i32, _i32, _i64]
_mixed_plan = [_i32, _ops, _i32, _i32p, _i32p, _i32p]

# The one Python copy of include/qiddm_hip.h: name -> (restype, argtypes), in the header's order.
# tests/test_capi_symbols.py checks the names against the header, tests/test_capi_binding.py every parameter list.
SIGNATURES = {
    "qiddm_abi_version": (_int, []),
    "qiddm_max_qubits": (_int, []),
    "qiddm_last_error": (ctypes.c_char_p, []),
    "qiddm_set_stamp_buffer": (_int, [_vp, _i64]),
    "qiddm_num_rot_gates": (_i64, [_P]),
    "qiddm_gate_count": (_i64, [_P]),
    "qiddm_gate_table_elems": (_i64, [_P]),
    "qiddm_num_shift_replicas": (_i64, [_P, _int]),
    "qiddm_workspace_bytes": (_i64, [_P, _i64, _i64]),
    "qiddm_prepare_gates": (_int, _table_of),
    "qiddm_forward": (_int, [_P, _vp, _i64, _i64, _vp, _vp, _i64] + _ws + _stream),
    "qiddm_forward_post": (_int, [_P, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _dbl] + _stream),
    "qiddm_forward_shifted": (_int, [_P, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp] + _ws + _stream),
    "qiddm_adjoint_partials": (_i64, [_P, _i64]),
    "qiddm_backward_adjoint": (_int, _adjoint + _stream),
    "qiddm_adjoint_workspace_bytes": (_i64, [_P, _i64]),
    "qiddm_backward_adjoint_wide": (_int, _adjoint + _ws + _stream),
    "qiddm_adjoint_finalize": (_int, [_P, _vp, _vp, _i64, _vp] + _stream),
    "qiddm_dense_forward": (_int, _dense + [_vp, _i64] + _stream),
    "qiddm_dense_sample": (_int, _dense + [_i32, _vp, _i64, _i64, _vp] + _stream),
    "qiddm_dense_sample_tables_bytes": (_i64, [_P]),
    "qiddm_dense_sample_prepare": (_int, _table_of),
    "qiddm_dense_sample_lean_tables_bytes": (_i64, [_P]),
    "qiddm_dense_sample_lean_prepare": (_int, [_P, _vp, _vp, _vp, _vp, _vp, _i64, _vp] + _stream),
    "qiddm_dense_sample_lean_check": (_int, [_P, _vp] + _stream),
    "qiddm_dense_sample_lean": (_int, [_P, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _vp, _i64, _i64, _vp]
                                + _stream),
    "qiddm_qconv_forward": (_int, [_P, _vp] + _image + [_vp, _i64, _vp] + _stream),
    "qiddm_qconv_backward": (_int, [_P, _vp] + _image + [_vp, _vp, _i64, _vp, _vp, _vp] + _stream),
    "qiddm_train_workspace_bytes": (_i64, [_P, _i64, _i32, _i32]),
    "qiddm_train_step": (_int, [_P, ctypes.POINTER(TrainArgs)] + _ws + _stream),
    "qiddm_adam_step": (_int, [ctypes.POINTER(AdamTensor), _i32, _dbl, _dbl, _dbl, _dbl, _dbl, _vp] + _stream),
    "qiddm_circuit_unitary": (_int, _table_of),
    "qiddm_circuit_unitary_wide": (_int, _table_of),
    "qiddm_qconv_unitary_workspace_bytes": (_i64, [_i32, _i64, _i64, _i64, _i64]),
    "qiddm_qconv_unitary_forward": (_int, [_i32, _vp, _vp] + _image + [_i64, _i32, ctypes.POINTER(BatchNormStruct), _i32, _vp]
                                    + _ws + _stream),
    "qiddm_batchnorm_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "qiddm_batchnorm_train_forward": (_int, _planes + [_vp, _vp, _vp, _vp, _dbl, _dbl, _vp, _vp, _vp] + _ws + _stream),
    "qiddm_batchnorm_backward_stats": (_int, _norm_back),
    "qiddm_batchnorm_backward": (_int, _norm_back),
    "qiddm_upsample2x_forward": (_int, _planes + [_vp, _vp, _vp] + _stream),
    "qiddm_upsample2x_backward": (_int, _planes + [_vp, _vp, _vp] + _stream),
    "qiddm_amp_embed_rows": (_int, [_vp, _i64, _i64, _i64, _i32, _dbl, _dbl, _vp] + _stream),
    "qiddm_prob_post": (_int, [_vp, _i64, _i64, _dbl, _vp] + _stream),
    "qiddm_maxpool2_forward": (_int, _planes + [_vp] + _stream),
    "qiddm_maxpool2_backward": (_int, [_vp] + _planes + [_vp] + _stream),
    "qiddm_qconv_train_plan": (_int, [_layer, ctypes.POINTER(QConvTrainPlan)]),
    "qiddm_qconv_train_backward": (_int, [_layer, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp] + _stream),
    "qiddm_qconv_train_rows": (_int, [_i32, _vp, _i32, _i64, _i64, _i32, _vp] + _stream),
    "qiddm_qconv_train_vectors": (_int, [_i32, _vp, _i64, _i64, _i64, _i32, _vp, _vp] + _stream),
    "qiddm_qconv_fold_features": (_int, [_vp] + _image + [_vp] + _stream),
    "qiddm_matrix_adjoint_partials": (_i64, [_i64]),
    "qiddm_matrix_adjoint_workspace_bytes": (_i64, [_P, _i64]),
    "qiddm_matrix_adjoint": (_int, [_P, _vp, _vp, _i64, _vp, _vp] + _ws + _stream),
    "qiddm_conv1x1_forward": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp] + _stream),
    "qiddm_conv1x1_head_partials": (_i64, [_i64, _i64]),
    "qiddm_conv1x1_head_backward": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp] + _stream),
    "qiddm_mixed_workspace_bytes": (_i64, [_i32, _i32, _i64, _i32]),
    "qiddm_mixed_forward": (_int, _mixed + [_vp, _i64] + _ws + _stream),
    "qiddm_mixed_backward_workspace_bytes": (_i64, [_i32, _i32, _i64, _ops, _i32, _i32]),
    "qiddm_mixed_backward": (_int, _mixed + [_vp, _i64, _vp, _vp, _vp, _i32] + _ws + _stream),
    "qiddm_mixed_wide_workspace_bytes": (_i64, [_i32, _i32, _i64, _ops, _i32]),
    "qiddm_mixed_wide_plan": (_int, _mixed_plan),
    "qiddm_mixed_wide_forward": (_int, _mixed + [_vp, _i64] + _ws + _stream),
    "qiddm_mixed_wide_backward_workspace_bytes": (_i64, [_i32, _i32, _i64, _ops, _i32]),
    "qiddm_mixed_wide_backward_plan": (_int, _mixed_plan),
    "qiddm_mixed_wide_backward": (_int, _mixed + [_vp, _i64, _vp, _vp, _vp] + _ws + _stream),
}
# every symbol include/qiddm_hip.h declares
EXPORTS = tuple(SIGNATURES)
# The extension header include/qiddm_hip_traj.h (the trajectory engine): the same kind of table, kept apart as the
# header is, so that SIGNATURES stays the copy of qiddm_hip.h.  tests/test_mixed_traj_capi.py checks it against its header.
TRAJ_SIGNATURES = {
    "qiddm_mixed_traj_workspace_bytes": (_i64, [_i32, _i32, _i64, _i32, _i32, _i64, _i32]),
    "qiddm_mixed_traj_forward": (_int, _mixed + [_i32, _dbl, _dbl, _i32, _vp, _i64, _vp, _vp] + _ws + _stream),
}
# include/qiddm_hip_traj_grad.h (the trajectory engine's reverse sweep): a header and a table of its own for the same
# reason.  tests/test_mixed_traj_grad_capi.py checks it against its header.
TRAJ_GRAD_SIGNATURES = {
    "qiddm_mixed_traj_backward_workspace_bytes": (_i64, [_i32, _i32, _i64, _i32, _ops, _i32, _i32, _i32, _i32, _i32]),
    "qiddm_mixed_traj_backward": (_int, _mixed + [_i32, _dbl, _dbl, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp] + _ws + _stream),
}
# include/qiddm_hip_traj_shots.h (finite shots on the trajectory engine): again a header and a table of its own, so that
# the three tables above hold what they held.  tests/test_mixed_traj_shots_capi.py checks it against its header.
TRAJ_SHOTS_SIGNATURES = {
    "qiddm_mixed_traj_shots_workspace_bytes": (_i64, [_i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32]),
    "qiddm_mixed_traj_shots_forward": (_int, _mixed + [_i32, _i32, _dbl, _dbl, _i32, _vp, _i64, _vp, _vp, _vp] + _ws + _stream),
}
TRAJ_SHOTS_PER_TRAJ = 1 << 16  # most shots one trajectory draws: ceil(shots / trajectories) may not exceed it


_lock = threading.Lock()
_lib = None


def _declare(handle):
    """Check the ABI version of ``handle``, then set ``restype`` / ``argtypes`` of every entry of ``SIGNATURES``.  A
    library of another version, or one that lacks a symbol, is a stale build: both say so."""
    def bind(name):
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise RuntimeError(f"libqiddm_hip.so has no symbol {name}: ABI mismatch; rebuild it") from None
        fn.restype, fn.argtypes = SIGNATURES[name]
        return fn

    if bind("qiddm_abi_version")() != 2:
        raise RuntimeError("libqiddm_hip.so ABI version mismatch; rebuild it")
    for name in SIGNATURES:
        bind(name)


def _declare_extensions(handle):
    """``restype`` / ``argtypes`` of every entry of ``TRAJ_SIGNATURES``, ``TRAJ_GRAD_SIGNATURES`` and
    ``TRAJ_SHOTS_SIGNATURES`` (after ``_declare`` has accepted the library's version); a library without one of them is
    a stale build."""
    for name, (restype, argtypes) in {**TRAJ_SIGNATURES, **TRAJ_GRAD_SIGNATURES, **TRAJ_SHOTS_SIGNATURES}.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise RuntimeError(f"libqiddm_hip.so has no symbol {name}: ABI mismatch; rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes


def _preload_torch_hip_runtime():
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def lib():
    """Load (once) and return the C-ABI library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: the HIP extension has not been built. "
                    "Run `python -c 'import __graft_entry__ as g; g.build()'` (or "
                    "`python -m qiddm_amd.build`) from the repo root. "
                    "qiddm_amd has no CPU fallback for the quantum layers."
                )
            _preload_torch_hip_runtime()
            handle = ctypes.CDLL(LIB_PATH)
            _declare(handle)
            _declare_extensions(handle)
            _lib = handle
    return _lib


def check(status: int):
    if status != QIDDM_OK:
        raise QiddmError(status, lib().qiddm_last_error().decode("utf-8", "replace"))


def _addresses(name: str, args) -> list:
    """``args`` as ctypes takes them: every tensor as its device address (an int, which the entry's ``c_void_p`` argtype
    widens to a pointer), everything else as it is -- None is NULL, and a structure or array instance goes by reference
    where the argtype is a ``POINTER``.  A tensor outside the device would be a wild address inside a kernel."""
    args = list(args)
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise TypeError(f"{name}: argument {i} is a tensor on {a.device}, not on a HIP device")
            args[i] = a.data_ptr()
    return args


def launch(name: str, device, *args) -> None:
    """Call the status-returning entry ``name`` with ``args`` and, last, the current stream of ``device``; raise
    ``QiddmError`` unless it returns QIDDM_OK.  ``device=None`` appends nothing: ``args`` is the whole argument list."""
    args = _addresses(name, args)
    if device is not None:
        args.append(torch.cuda.current_stream(device).cuda_stream)
    check(getattr(lib(), name)(*args))


def query(name: str, *args, device=None) -> int:
    """The value of a size / count / predicate entry; a negative one is the library's status and raises ``QiddmError``
    with that code.  ``device``: as for ``launch`` (``qiddm_dense_sample_lean_check`` reads back on a stream)."""
    args = _addresses(name, args)
    if device is not None:
        args.append(torch.cuda.current_stream(device).cuda_stream)
    value = getattr(lib(), name)(*args)
    if value < 0:
        check(int(value))
    return value

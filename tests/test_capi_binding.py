"""The Python side of the C ABI: the signature table of qiddm_amd/_capi.py against include/qiddm_hip.h, and the
``launch`` / ``query`` gateway every call in the package goes through (no compute calls: nothing here needs a GPU)."""
import ctypes
import os
import re
import types

import pytest
import torch

from qiddm_amd import _capi
from qiddm_amd.circuit import Circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_BYTES = {"int32_t": 4, "int": 4, "int64_t": 8, "double": 8}
RETURNS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def _header_signatures():
    """name -> (return type, [("ptr", None) | ("scalar", bytes)]) for every function include/qiddm_hip.h declares."""
    text = open(os.path.join(ROOT, "include", "qiddm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for returns, name, params in re.findall(r"([A-Za-z_0-9 *]+?)\s*\b(qiddm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        kinds = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("void", ""):
                continue
            words = p.replace("*", " * ").split()
            if "*" in words or words[-1] == "stream":
                kinds.append(("ptr", None))
            else:
                ctype = [w for w in words[:-1] if w != "const"]
                assert len(ctype) == 1 and ctype[0] in SCALAR_BYTES, (name, p)
                kinds.append(("scalar", SCALAR_BYTES[ctype[0]]))
        out[name] = (" ".join(returns.split()), kinds)
    return out


def _table_kind(argtype):
    if argtype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(argtype, ctypes._Pointer):
        return ("ptr", None)
    return ("scalar", ctypes.sizeof(argtype))


def test_every_parameter_list_agrees_with_the_header():
    header = _header_signatures()
    assert len(header) == 66 and sorted(header) == sorted(_capi.SIGNATURES)
    for name, (returns, kinds) in header.items():
        restype, argtypes = _capi.SIGNATURES[name]
        assert ctypes.sizeof(restype) == ctypes.sizeof(RETURNS[returns]) and (restype is ctypes.c_char_p) == ("*" in returns), \
            (name, restype, returns)
        assert len(argtypes) == len(kinds), (name, len(argtypes), len(kinds))
        for i, (argtype, kind) in enumerate(zip(argtypes, kinds)):
            assert _table_kind(argtype) == kind, (name, i, argtype, kind)


def test_exports_and_declarations_come_from_the_table(hip_lib):
    assert _capi.EXPORTS == tuple(_capi.SIGNATURES)
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_launch_rejects_a_host_tensor_before_it_enters_the_library(hip_lib):
    cs = Circuit(4, "rz", "CZ", "expz", 1, 1, 2).c_struct("f64")
    assert hip_lib.qiddm_gate_count(ctypes.byref(Circuit(17, "rz").c_struct("f32"))) == -1
    before = hip_lib.qiddm_last_error()
    host = torch.zeros(96, dtype=torch.float64)
    # device "cuda": the stream of a device this test may not have is looked up only after the arguments passed
    with pytest.raises(TypeError, match=r"qiddm_prepare_gates: argument 1 .*cpu"):
        _capi.launch("qiddm_prepare_gates", torch.device("cuda"), cs, host, None)
    with pytest.raises(TypeError, match=r"qiddm_dense_sample_lean_check: argument 1 .*cpu"):
        _capi.query("qiddm_dense_sample_lean_check", cs, host, device=torch.device("cuda"))
    assert hip_lib.qiddm_last_error() == before and b"exceeds" in before


def test_launch_passes_none_as_null_and_raises_the_librarys_status(hip_lib):
    """The descriptors of test_capi_symbols.test_matrix_adjoint_refuses_descriptors_finalize_reads_as_folded."""
    def desc(n, imprimitive):
        return Circuit(n_qubits=n, encoding="none", imprimitive=imprimitive, measure="probs", n_rounds=1, n_blocks=1,
                       sel_layers=3).c_struct("f64")

    for cs, code, word in [(desc(n, "CZ"), -2, "folded") for n in (8, 10, 12, 16)] + [(desc(12, "CNOT"), -1, "NULL")]:
        assert hip_lib.qiddm_matrix_adjoint(ctypes.byref(cs), None, None, 2, None, None, None, 0, None) == code
        raw = hip_lib.qiddm_last_error().decode()
        with pytest.raises(_capi.QiddmError) as e:
            _capi.launch("qiddm_matrix_adjoint", None, cs, None, None, 2, None, None, None, 0, None)   # last: NULL stream
        assert e.value.code == code and word in raw and str(e.value) == f"libqiddm_hip: {raw} (status {code})"


def test_query_returns_the_value_and_raises_a_negative_one():
    cs = Circuit(8, "rz", "CZ", "expz", 2, 6, 2).c_struct("f32")
    assert _capi.query("qiddm_gate_count", cs) == 480 and _capi.query("qiddm_num_shift_replicas", cs, 1) == 6 * 192 + 96
    assert _capi.query("qiddm_workspace_bytes", cs, 4096, 0) == 0
    with pytest.raises(_capi.QiddmError, match="exceeds") as e:
        _capi.query("qiddm_gate_count", Circuit(17, "rz").c_struct("f32"))
    assert e.value.code == -1


def _stand_in(version, without=()):
    """What ``ctypes.CDLL`` hands to ``_declare``: one attribute per symbol that takes a restype and argtypes."""
    handle = types.SimpleNamespace()
    for name in _capi.SIGNATURES:
        if name not in without:
            setattr(handle, name, (lambda: version) if name == "qiddm_abi_version" else (lambda *a: 0))
    return handle


def test_a_stale_library_is_told_to_rebuild():
    _capi._declare(_stand_in(2))
    with pytest.raises(RuntimeError, match="rebuild"):
        _capi._declare(_stand_in(1))
    for missing in ("qiddm_mixed_wide_backward", "qiddm_max_qubits"):
        with pytest.raises(RuntimeError, match=f"{missing}.*rebuild") as e:
            _capi._declare(_stand_in(2, without=(missing,)))
        assert not isinstance(e.value, AttributeError)
    with pytest.raises(RuntimeError, match="rebuild"):           # the version comes first: an old library says so
        _capi._declare(_stand_in(1, without=("qiddm_mixed_wide_backward",)))

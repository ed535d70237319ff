"""A two-wire Kraus channel on ``oracle.density``'s rho, for the tests of ``QIDDM_MIX_CHANNEL2`` (the oracle has the
one-wire ``apply_kraus`` only).  complex128, differentiable torch; rho is (B, D, D), wire w is bit n-1-w of both indices.

``apply_kraus2`` reshapes rho so that the four index bits of the two wires stand alone and contracts them with
K (row side) and conj(K) (column side): no 2^n x 2^n operator is built.  ``embed2`` builds exactly that operator; it is
what ``apply_kraus2`` is checked against on the CPU (tests/test_mixed_channel2_capi.py) before any GPU test relies on it.
Also here: the Kraus sets the two test files share."""
import itertools

import numpy as np
import torch

CDT = torch.complex128
PAULIS = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
          "Y": np.array([[0, -1j], [1j, 0]], dtype=complex), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}
SWAP = np.eye(4, dtype=complex)[[0, 2, 1, 3]]
CNOT = np.eye(4, dtype=complex)[[0, 1, 3, 2]]


def apply_kraus2(rho, kraus, w1, w2, n):
    """sum_k K rho K^dagger, K (4 x 4, index 2 b_w1 + b_w2) on wires w1 != w2 of an n-wire rho (B, 2^n, 2^n)."""
    assert w1 != w2 and 0 <= w1 < n and 0 <= w2 < n
    b, d = rho.shape[0], 1 << n
    r = rho.to(CDT).reshape((b,) + (2,) * (2 * n))
    # row bits of the two wires to the front, their column bits behind them: (B, r1, r2, c1, c2, rest...)
    src = (1 + w1, 1 + w2, 1 + n + w1, 1 + n + w2)
    r = torch.movedim(r, src, (1, 2, 3, 4))
    rest = r.shape[5:]
    r = r.reshape(b, 4, 4, -1)                                   # (B, row pair, column pair, rest)
    out = torch.zeros_like(r)
    for k in kraus:
        k = torch.as_tensor(k).to(CDT)
        out = out + torch.einsum("xr,brcz,yc->bxyz", k, r, k.conj())
    out = out.reshape((b, 2, 2, 2, 2) + tuple(rest))
    return torch.movedim(out, (1, 2, 3, 4), src).reshape(b, d, d)


def embed2(k, w1, w2, n):
    """The 2^n x 2^n operator of the 4 x 4 `k` on wires (w1, w2), identity elsewhere (numpy), entry by entry."""
    k = np.asarray(k, dtype=complex)
    d = 1 << n
    out = np.zeros((d, d), dtype=complex)
    q1, q2 = n - 1 - w1, n - 1 - w2
    for i in range(d):
        for j in range(d):
            if (i ^ j) & ~((1 << q1) | (1 << q2)):
                continue                                         # the other wires must agree
            out[i, j] = k[2 * ((i >> q1) & 1) + ((i >> q2) & 1), 2 * ((j >> q1) & 1) + ((j >> q2) & 1)]
    return out


def super2(kraus):
    """S = sum K (x) conj(K), 16 x 16 (numpy)."""
    return sum(np.kron(np.asarray(k, dtype=complex), np.asarray(k, dtype=complex).conj()) for k in kraus)


def rows_to_complex(rows):
    """The (64, 8) float64 row block of the op -> the 16 x 16 complex S it holds."""
    rows = rows.numpy()
    assert rows.shape == (64, 8) and rows.dtype == np.float64
    return (rows[:, 0::2] + 1j * rows[:, 1::2]).reshape(16, 16)


def qr_kraus2(seed):
    """Three 4 x 4 operators from the reduced QR of a seeded complex Gaussian (12 x 4): K_i = Q[4i : 4i + 4].  Trace
    preserving; complex, non-unital, entangling and not symmetric under exchange of the wires (checked in the host test)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(12, 4)) + 1j * rng.normal(size=(12, 4)))
    return [np.ascontiguousarray(q[4 * i:4 * i + 4]) for i in range(3)]


def qr_kraus1(seed):
    """The one-wire analogue (6 x 2), three 2 x 2 operators."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(6, 2)) + 1j * rng.normal(size=(6, 2)))
    return [np.ascontiguousarray(q[2 * i:2 * i + 2]) for i in range(3)]


def depolarizing2(p):
    """Two-qubit depolarizing from the 16 Paulis: rho -> (1 - p) rho + p/15 sum_{P != II} P rho P."""
    words = ["".join(w) for w in itertools.product("IXYZ", repeat=2)]
    return [np.sqrt(1 - p if w == "II" else p / 15) * np.kron(PAULIS[w[0]], PAULIS[w[1]]) for w in words]

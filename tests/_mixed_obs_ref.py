"""Shared reference for the Pauli-word read-out of ``default.mixed`` (test_mixed_obs_host.py, test_gpu_mixed_obs.py).

Words are dense matrices built by Kronecker product in complex128 (wire 0 the most significant factor, as
``oracle.density`` indexes rho); an expectation value is ``Tr(rho P).real``; gradients are torch autograd through the
oracle.  That side never looks at a mask.  ``mask_rule_matrix`` / ``mask_rule_value`` restate the mask rule of
include/qiddm_hip.h in numpy, so that the host tests can hold it against the Kronecker products."""
import functools

import numpy as np
import torch

CDT = torch.complex128
PAULI = {"I": torch.eye(2, dtype=CDT), "X": torch.tensor([[0, 1], [1, 0]], dtype=CDT),
         "Y": torch.tensor([[0, -1j], [1j, 0]], dtype=CDT), "Z": torch.tensor([[1, 0], [0, -1]], dtype=CDT)}


def dense_word(word, n):
    """((wire, letter), ...) -> the 2^n x 2^n matrix of the word."""
    letters = ["I"] * n
    for wire, letter in word:
        assert letters[wire] == "I" or letter == "I", word
        letters[wire] = letter
    return functools.reduce(torch.kron, [PAULI[c] for c in letters])


def expvals(rho, columns, n):
    """rho (B, D, D) complex128, columns: one list of (coefficient, word) each -> (B, len(columns)) float64,
    sum_t c_t Tr(rho P_t).real per column.  Differentiable in rho."""
    out = []
    for column in columns:
        total = 0.0
        for coeff, word in column:
            total = total + coeff * (rho * dense_word(word, n).transpose(0, 1)).sum(dim=(1, 2)).real   # Tr(rho P) = sum_ij rho_ij P_ji
        out.append(total)
    return torch.stack(out, dim=1)


def column_weight(column):
    """max(1, sum |c_t|): the factor on the project's bounds for a column that adds several words"""
    return max(1.0, sum(abs(c) for c, _ in column))


def columns_of(measurements):
    """The (coefficient, word) lists of a list of ``qml.expval`` results."""
    return [list(m.obs.terms) for m in measurements]


def mask_rule_matrix(x, z, n):
    """The word with x-mask `x` and z-mask `z` by the header's rule, as a dense numpy matrix:
    P[i][j] = i^ny (-1)^popcount(j & z) where i ^ j = x, ny = popcount(x & z)."""
    d = 1 << n
    p = np.zeros((d, d), dtype=complex)
    ny = bin(x & z).count("1")
    for j in range(d):
        p[j ^ x, j] = (1j ** ny) * (-1) ** bin(j & z).count("1")
    return p


def mask_rule_value(rho, x, z, n):
    """Re(i^ny sum_k (-1)^popcount(k & z) rho[k][k ^ x]): what the read-out kernel sums, in numpy."""
    ny = bin(x & z).count("1")
    k = np.arange(1 << n)
    sign = np.array([(-1) ** bin(int(v) & z).count("1") for v in k])
    return float(((1j ** ny) * (sign * rho[k, k ^ x]).sum()).real)


def random_rho(n, seed):
    """A full-rank density matrix with complex off-diagonals (numpy complex128)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(1 << n, 1 << n)) + 1j * rng.normal(size=(1 << n, 1 << n))
    rho = a @ a.conj().T
    return rho / np.trace(rho).real

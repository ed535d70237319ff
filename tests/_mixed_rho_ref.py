"""Reference for the density-matrix read-out of ``default.mixed`` (``QIDDM_MEAS_RHO``): the partial trace as a reshape and
an ``einsum`` over the traced wires -- it knows nothing of masks -- and, separately, a numpy restatement of the rule in
include/qiddm_hip.h (``dep``, the output layout, the Hermitian-part seed) that the CPU tests hold against it."""
import numpy as np
import torch

_ROW, _COL = "abcdefghij", "klmnopqrst"


def partial_trace(rho, wires, n):
    """rho (B, 2^n, 2^n) complex -> (B, 2^k, 2^k): the reduced matrix of the listed wires, index bits in the listed order
    (the first listed wire most significant).  torch, differentiable in rho."""
    wires = list(wires)
    src = _ROW[:n] + "".join(_COL[w] if w in wires else _ROW[w] for w in range(n))
    dst = "".join(_ROW[w] for w in wires) + "".join(_COL[w] for w in wires)
    d = 1 << len(wires)
    return torch.einsum(f"z{src}->z{dst}", rho.reshape(rho.shape[0], *([2] * (2 * n)))).reshape(rho.shape[0], d, d)


def as_reals(rho_a):
    """(B, K, K) complex -> (B, 2 K^2) float64 in the C ABI's layout: (r, c) at columns 2 (r K + c) and 2 (r K + c) + 1."""
    return torch.view_as_real(rho_a.contiguous()).reshape(rho_a.shape[0], -1)


# ---- the rule of the header, in numpy ---------------------------------------------------------------------------------------
def keep_mask(wires, n):
    """wire w at bit n-1-w"""
    return sum(1 << (n - 1 - w) for w in wires)


def dep(v, mask, n):
    """the low bits of v, in order, at the set positions of `mask`"""
    out = 0
    for b in range(n):
        if mask >> b & 1:
            out |= (v & 1) << b
            v >>= 1
    return out


def mask_rule_read_out(rho, mask, n):
    """rho (2^n, 2^n) numpy -> the (2 K^2,) row the kernels write: out[r][c] = sum_e rho[dep(r, e)][dep(c, e)], e in
    ascending order"""
    k = bin(mask).count("1")
    K, E, rest = 1 << k, 1 << (n - k), ((1 << n) - 1) & ~mask
    out = np.zeros(2 * K * K)
    for r in range(K):
        for c in range(K):
            s = 0j
            for e in range(E):
                t = dep(e, rest, n)
                s += rho[dep(r, mask, n) | t, dep(c, mask, n) | t]
            out[2 * (r * K + c)], out[2 * (r * K + c) + 1] = s.real, s.imag
    return out


def mask_rule_seed(g, mask, n):
    """g (2 K^2,) numpy, the cotangent of the row above -> Lambda_N (2^n, 2^n): where i and j agree outside the mask,
    (g_re[r][c] + g_re[c][r]) / 2 + i (g_im[r][c] - g_im[c][r]) / 2 with r, c the kept bits of i, j; zero elsewhere."""
    k = bin(mask).count("1")
    K, D = 1 << k, 1 << n
    g_re, g_im = g[0::2].reshape(K, K), g[1::2].reshape(K, K)
    kept = lambda i: sum(((i >> b) & 1) << at for at, b in enumerate(b for b in range(n) if mask >> b & 1))
    lam = np.zeros((D, D), dtype=complex)
    for i in range(D):
        for j in range(D):
            if (i ^ j) & ~mask == 0:
                r, c = kept(i), kept(j)
                lam[i, j] = 0.5 * (g_re[r, c] + g_re[c, r]) + 0.5j * (g_im[r, c] - g_im[c, r])
    return lam

"""The sampling rule of ``QIDDM_MIX_SHOTS`` (include/qiddm_hip.h) in numpy, bit for bit (a helper module, not a
conftest): given a sample's float64 probabilities it reproduces the counts the kernels return.

    p_k = fmax(p_k, 0);  c = cumsum(p) (sequential float64);  T = c[D - 1]
    shot s of absolute row b: word (s & 3) of Philox4x32-10, counter (s >> 2, b, offset lo, offset hi),
    key (seed lo, seed hi);  v = (float64(word) * 2^-32) * T;  outcome = #{k : c_k <= v}, clamped to D - 1
    T <= 0 or not finite: no counts (the kernels return a NaN row; here the row of counts is -1)
"""
import numpy as np

from _value_domain import philox4x32_10


def outcomes(probs_row, shots, seed, offset, row):
    """The `shots` outcomes of one sample (int64), in shot order; ``None`` when T is not positive or not finite."""
    c = np.cumsum(np.fmax(np.asarray(probs_row, dtype=np.float64), 0.0))
    total = c[-1]
    if not (total > 0.0 and np.isfinite(total)):
        return None
    groups = np.arange((shots + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((groups, row & 0xFFFFFFFF, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = np.stack(words, axis=1).reshape(-1)[:shots]             # shot s = 4 g + j takes word j of group g
    v = (word.astype(np.float64) * 2.0 ** -32) * total
    return np.minimum(np.searchsorted(c, v, side="right"), len(c) - 1).astype(np.int64)


def sample(probs, shots, seed, offset, first_row=0):
    """``probs`` (B, D) float64 -> counts (B, D) int64; row b of the array is absolute row ``first_row + b``."""
    probs = np.asarray(probs, dtype=np.float64)
    counts = np.empty(probs.shape, dtype=np.int64)
    for b in range(probs.shape[0]):
        k = outcomes(probs[b], shots, seed, offset, first_row + b)
        counts[b] = -1 if k is None else np.bincount(k, minlength=probs.shape[1])
    return counts


def signed_sums(counts, n):
    """(B, 2^n) counts -> (B, n) int64: n+ - n- per wire; wire w is bit n-1-w of the outcome, -1 when the bit is set."""
    k = np.arange(counts.shape[1])
    signs = np.stack([1 - 2 * ((k >> (n - 1 - w)) & 1) for w in range(n)], axis=1)        # (D, n)
    return counts @ signs

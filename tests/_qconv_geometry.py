"""QConv2d geometry cases: rectangular kernels, unequal and over-padding, images thinner than the kernel, tile edges.

One table (``CASES``) shared by tests/test_qconv_geometry_host.py (no GPU: the plan columns, the coverage the table
claims, the conditions on the inputs) and tests/test_gpu_qconv_geometry.py (every route of every layer against the CPU
oracle, exact footprints, guard bands through the C ABI).  ``qdepth`` is 2 throughout.

The host's choice of kernel variants (qiddm_amd/csrc/qiddm_qconv.hip) is restated here in Python so that the table can be
checked, without a GPU, to reach every variant a layer of at most 9 wires can reach; a kernel trace of the GPU file
(profiles/qconv_geometry/kernels_reached.txt) is compared with the restatement.
"""
import collections
import functools
import math

import torch

from oracle import circuits as oc

QDEPTH = 2
MAX_LDS = 160 * 1024            # capi_common.h: kMaxLds
FWD_TILE, FWD_THREADS = 128, 256     # qsim_qconv_fwd.h
DX_TILE, DX_THREADS = 64, 256        # qsim_qconv_dx.h
KINK_BAND = 1e-3                # ten times the KINK of test_gpu_unet_train_at_scale.py, where float32 cannot tell the side
CLAMPED_SHARE = (0.02, 0.50)

# plan columns: (route, matrix_core, row_channels, bn_fold, pixel rows) as qiddm_qconv_train_plan answers with no
# QIDDM_QCONV_* variable set; the last three are 0 off the thin route (row_channels is reported on every route)
Case = collections.namedtuple("Case", "group c_in c_out k p hw batch seed plan")


def _c(group, c_in, c_out, k, p, hw, batch, seed, plan):
    return Case(group, c_in, c_out, k, p, hw, batch, seed, plan)


VALU8, VALU16 = ("thin", 0, 8, 1, 0), ("thin", 0, 16, 1, 0)
MFMA8_DX, MFMA16_DX, MFMA32_DX = ("thin", 1, 8, 1, 1), ("thin", 1, 16, 1, 1), ("thin", 1, 32, 0, 1)
MFMA8_FOLD, MFMA16_FOLD, MFMA32_FOLD = ("thin", 1, 8, 1, 0), ("thin", 1, 16, 1, 0), ("thin", 1, 32, 0, 0)

CASES = [
    # ---- rectangular kernels, same-size padding ----------------------------------------------------------------------
    _c("rect", 2, 4, (1, 3), (0, 1), (5, 7), 3, 1, VALU8),
    _c("rect", 2, 4, (3, 1), (1, 0), (7, 5), 3, 2, VALU8),
    _c("rect", 4, 8, (3, 5), (1, 2), (6, 9), 3, 1, MFMA8_DX),
    _c("rect", 4, 8, (5, 3), (2, 1), (9, 6), 3, 1, MFMA8_DX),
    _c("rect", 8, 16, (1, 5), (0, 2), (4, 11), 2, 4, MFMA16_DX),
    _c("rect", 3, 8, (1, 15), (0, 7), (3, 17), 2, 0, MFMA8_DX),          # C_in < 4: a wave of the walk owns no channel
    _c("rect", 1, 8, (1, 15), (0, 7), (3, 17), 2, 4, VALU8),
    _c("rect", 1, 4, (1, 31), (0, 15), (2, 33), 2, 0, ("gemm", 0, 8, 0, 0)),   # kw > 15: library-GEMM backward; 31 taps: halo forward; upsampled: the row that showed the gather's 4-bit taps
    _c("rect", 1, 4, (17, 1), (8, 0), (18, 2), 2, 0, ("gemm", 0, 8, 0, 0)),   # kh > 16: the gathering kernel's wide tap table (upsampling)
    _c("rect", 8, 100, (1, 17), (0, 8), (2, 18), 2, 0, ("gemm", 0, 0, 0, 0)),  # the same in the 128-channel gathering kernel
    # ---- fewer input channels than the four waves of the matrix-core walk -------------------------------------------
    _c("few", 3, 20, (3, 5), (1, 2), (5, 5), 2, 0, MFMA32_FOLD),         # (dx: its LDS is past half the limit)
    _c("few", 2, 8, (5, 5), (2, 2), (7, 6), 3, 0, MFMA8_DX),
    _c("few", 1, 8, (7, 7), (3, 3), (8, 8), 2, 1, MFMA8_FOLD),           # 49 taps: fold, gathering forward
    _c("few", 1, 8, (5, 7), (2, 3), (6, 8), 2, 0, MFMA8_FOLD),           # 35 taps: fold, gathering forward
    # ---- unequal padding, padding beyond "same" -----------------------------------------------------------------------
    _c("pad", 2, 4, (3, 3), (1, 0), (5, 6), 3, 0, VALU8),                # Wo < W
    _c("pad", 4, 8, (3, 3), (0, 1), (6, 5), 3, 0, MFMA8_FOLD),           # Ho < H
    _c("pad", 4, 8, (3, 3), (2, 2), (4, 5), 2, 0, MFMA8_FOLD),           # Ho > H, Wo > W
    _c("pad", 2, 4, (3, 3), (2, 1), (3, 4), 2, 0, VALU8),
    _c("pad", 1, 4, (1, 31), (0, 14), (2, 33), 2, 0, ("gemm", 0, 8, 0, 0)),    # kw > 16 outside the halo forward
    _c("pad", 1, 4, (17, 1), (7, 0), (18, 2), 2, 0, ("gemm", 0, 8, 0, 0)),     # kh > 16 outside the halo forward
    # ---- the compiled-in (kernel extent, channels) shapes with a padding they have not run with ----------------------
    _c("static", 16, 8, (1, 1), (1, 2), (3, 4), 2, 2, MFMA8_FOLD),       # border pixels whose whole patch is padding
    _c("static", 16, 8, (3, 3), (0, 0), (5, 5), 2, 0, MFMA8_FOLD),
    _c("static", 8, 16, (3, 3), (2, 2), (4, 4), 2, 1, MFMA16_FOLD),
    _c("static", 32, 16, (1, 1), (1, 1), (3, 3), 2, 0, MFMA16_FOLD),
    _c("static", 32, 16, (3, 3), (1, 0), (4, 4), 2, 0, MFMA16_FOLD),
    _c("static", 16, 32, (3, 3), (0, 1), (4, 3), 2, 0, MFMA32_FOLD),
    # ---- images thinner than the kernel ---------------------------------------------------------------------------------
    _c("thin", 4, 8, (3, 3), (1, 1), (1, 9), 3, 0, MFMA8_DX),
    _c("thin", 4, 8, (3, 3), (1, 1), (9, 1), 3, 0, MFMA8_DX),
    _c("thin", 4, 8, (3, 3), (1, 1), (1, 1), 150, 0, MFMA8_DX),          # a 128-pixel tile spans 128 images
    _c("thin", 2, 4, (5, 5), (2, 2), (2, 3), 30, 0, MFMA8_DX),
    _c("thin", 1, 4, (3, 3), (1, 1), (2, 2), 40, 2, VALU8),
    # ---- tile edges: 64 pixels backward and dx, 128 forward ----------------------------------------------------------
    _c("edge", 4, 8, (3, 3), (1, 1), (1, 127), 1, 0, MFMA8_DX),          # M = 127
    _c("edge", 4, 8, (3, 3), (1, 1), (1, 128), 1, 1, MFMA8_DX),          # M = 128
    _c("edge", 4, 8, (3, 3), (1, 1), (3, 43), 1, 0, MFMA8_DX),           # M = 129
    _c("edge", 4, 8, (3, 3), (1, 1), (5, 13), 1, 0, MFMA8_DX),           # M = 65
    _c("edge", 4, 8, (3, 3), (1, 1), (5, 13), 2, 2, MFMA8_DX),           # M = 130
    # ---- wide layers ---------------------------------------------------------------------------------------------------
    _c("wide", 32, 16, (3, 3), (1, 1), (2, 2), 17, 0, MFMA16_DX),        # dx with two channel blocks
    _c("wide", 16, 32, (3, 5), (1, 2), (4, 5), 2, 0, ("gemm", 0, 32, 0, 0)),
    _c("wide", 8, 40, (3, 3), (1, 1), (3, 3), 2, 1, ("gemm", 0, 0, 0, 0)),    # two forward channel tiles
    # ---- the remaining kernel variants a layer of at most 9 wires reaches (see ``small_layers``) ----------------
    _c("variant", 1, 16, (3, 7), (1, 3), (3, 5), 2, 0, VALU16),          # halo forward (32, 1)
    _c("variant", 4, 12, (3, 3), (1, 1), (3, 4), 2, 0, MFMA16_DX),       # halo forward (32, 4)
    _c("variant", 8, 8, (3, 3), (1, 1), (1, 20), 2, 2, MFMA8_DX),        # halo forward (16, 12)
    _c("variant", 8, 16, (3, 3), (1, 1), (1, 20), 2, 2, MFMA16_DX),      # halo forward (32, 12)
    _c("variant", 8, 32, (3, 3), (1, 1), (1, 20), 2, 2, MFMA32_DX),      # halo forward (64, 12), dx (64, 1, 6)
    _c("variant", 32, 8, (3, 3), (1, 1), (2, 2), 2, 2, MFMA8_DX),        # halo forward (16, 20), dx (16, 2, 2)
    _c("variant", 32, 32, (3, 3), (1, 1), (2, 2), 2, 0, ("gemm", 0, 32, 0, 0)),   # halo forward (64, 20)
    _c("variant", 17, 32, (1, 3), (0, 1), (2, 3), 2, 0, MFMA32_DX),      # dx (64, 2, 6): at most 6 taps fit its LDS
    _c("variant", 4, 8, (3, 3), (1, 1), (1, 40), 1, 0, MFMA8_DX),        # dx (16, 1, 4): halo 41
    _c("variant", 4, 8, (3, 3), (1, 1), (1, 97), 1, 0, MFMA8_DX),        # dx (16, 1, 6): halo 98
    _c("variant", 32, 8, (3, 3), (1, 1), (1, 40), 1, 0, MFMA8_DX),       # dx (16, 2, 4)
    _c("variant", 32, 8, (3, 3), (1, 1), (1, 97), 1, 0, MFMA8_DX),       # dx (16, 2, 6)
    _c("variant", 32, 16, (1, 1), (0, 0), (3, 3), 2, 0, MFMA16_DX),      # dx (32, 2, 2): no halo
    _c("variant", 8, 16, (3, 3), (1, 1), (1, 40), 1, 0, MFMA16_DX),      # dx (32, 1, 6): halo 41
    _c("variant", 32, 16, (3, 3), (1, 1), (1, 40), 1, 0, MFMA16_DX),     # dx (32, 2, 6)
    _c("variant", 1, 16, (3, 17), (1, 8), (3, 5), 2, 1, ("gemm", 0, 16, 0, 0)),    # 32-column gathering kernel, kw > 16
    _c("variant", 1, 32, (3, 17), (1, 8), (3, 5), 2, 1, ("gemm", 0, 32, 0, 0)),    # 64-column gathering kernel, kw > 16
    _c("variant", 44, 100, (1, 3), (0, 1), (3, 3), 2, 1, ("gemm", 0, 0, 0, 0)),   # the 128-channel gathering kernel
]
# Variants of the restated rule that no QConv2d of at most 9 wires reaches (``UNREACHABLE_*`` below):
#   halo forward (64, 1): need = 1 takes C_in = 1; at most 31 taps give at most 5 wires, hence at most 16 channels;
#   dx (32, 1, 2): K2 = 32 has slots <= 2 only without a halo, i.e. for 1 x 1 kernels; a 1 x 1 layer on the matrix-core
#       kernel has F = C_in >= 32 (the narrow 16-channel case has 8 row channels), so two channel blocks;
#   dx (64, *, 2): K2 = 64 has at least (64 + 2 halo) / 16 >= 4 slots;
#   dx (64, *, 4): K2 = 64 has 4 slots only without a halo; a 1 x 1 kernel with more than 16 output channels needs 6
#       wires, so more than 32 input channels, beyond the dx kernel.
# ``small_layers`` is the grid the rule is enumerated on; the host test holds the table and these sets to its answer.

GROUPS = ("rect", "few", "pad", "static", "thin", "edge", "wide", "variant")
STATIC_SHAPES = [(1, 16), (3, 16), (3, 8), (1, 32), (3, 32)]      # (SK, SC) of QIDDM_TM_SCASE, qiddm_qconv.hip


def case_id(case):
    return "%d-%d-k%dx%d-p%dx%d-%dx%d-b%d" % (case.c_in, case.c_out, *case.k, *case.p, *case.hw, case.batch)


def wires(case):
    return oc.qconv_wires(case.c_in, case.c_out, case.k)


def features(case):
    return case.c_in * case.k[0] * case.k[1]


def out_hw(case, hw=None):
    h, w = hw or case.hw
    return h + 2 * case.p[0] - case.k[0] + 1, w + 2 * case.p[1] - case.k[1] + 1


def layer_tuple(case):
    """(n_qubits, batch, c_in, h, w, kh, kw, ph, pw, c_out): the fields of ``_capi.QConvLayer`` behind its dtype slot."""
    return (wires(case), case.batch, case.c_in, *case.hw, *case.k, *case.p, case.c_out)


def forward_bound(case):
    """Absolute bound of the float32 forwards (test_gpu_qconv_unitary.py): outputs are probabilities times D / 2."""
    return 2e-5 * max(1.0, 2 ** wires(case) / 2) / 8


# ---- inputs and the oracle ---------------------------------------------------------------------------------------------
def draw(case, seed=None):
    """(x, weights, grad_y) float64 on the CPU from one generator seeded with ``seed`` (the case's own by default)."""
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    x = torch.rand(case.batch, case.c_in, *case.hw, generator=g, dtype=torch.float64)
    w = torch.rand(QDEPTH, wires(case), 3, generator=g, dtype=torch.float64) * math.pi - math.pi / 2
    gy = torch.randn(case.batch, case.c_out, *out_hw(case), generator=g, dtype=torch.float64)
    return x, w, gy


@functools.lru_cache(maxsize=None)
def inputs(case):
    return draw(case)


def input_conditions(case, seed):
    """(smallest distance of a scaled probability from the clamp's kink at 1, share of clamped outputs), oracle alone."""
    x, w, _ = draw(case, seed)
    p = oc.qconv2d_forward_unitary(x, w, case.c_out, case.k, case.p, clamp=False)
    return (p - 1.0).abs().min().item(), (p > 1.0).double().mean().item()


def conditions_met(case, seed):
    dist, share = input_conditions(case, seed)
    return dist >= KINK_BAND and CLAMPED_SHARE[0] <= share <= CLAMPED_SHARE[1]


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict(y, gw, gx): ``oc.qconv2d_forward`` and autograd through it with the case's ``grad_y``.  Shared: read only."""
    x, w, gy = inputs(case)
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = oc.qconv2d_forward(xo, wo, case.c_out, case.k, case.p)
    gw, gx = torch.autograd.grad((y * gy).sum(), [wo, xo])
    return {"y": y.detach(), "gw": gw, "gx": gx}


def bn_parameters(case):
    g = torch.Generator().manual_seed(1000 + case.seed + case.c_in + case.c_out)
    c = case.c_out
    return {"weight": torch.rand(c, generator=g, dtype=torch.float64) + 0.5,
            "bias": torch.rand(c, generator=g, dtype=torch.float64) * 0.6 - 0.3,
            "running_mean": torch.rand(c, generator=g, dtype=torch.float64) * 0.5,
            "running_var": torch.rand(c, generator=g, dtype=torch.float64) * 1.8 + 0.2}


@functools.lru_cache(maxsize=None)
def reference_bn_train(case):
    """dict(z, gw, gx, gbw, gbb): the oracle convolution followed by ``oracle.unet._bn(training=True)``."""
    from oracle import unet as ou
    x, w, gy = inputs(case)
    bn = bn_parameters(case)
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bw, bb = bn["weight"].clone().requires_grad_(True), bn["bias"].clone().requires_grad_(True)
    y = oc.qconv2d_forward(xo, wo, case.c_out, case.k, case.p)
    z = ou._bn(y, {"b.weight": bw, "b.bias": bb}, "b", training=True)
    gw, gx, gbw, gbb = torch.autograd.grad((z * gy).sum(), [wo, xo, bw, bb])
    return {"z": z.detach(), "gw": gw, "gx": gx, "gbw": gbw, "gbb": gbb}


def patch_footprint(case, i, j, hw=None):
    """Boolean (Ho, Wo) mask of the output pixels whose patch contains input pixel (i, j)."""
    ho, wo = out_hw(case, hw)
    oi = torch.arange(ho).view(-1, 1)
    oj = torch.arange(wo).view(1, -1)
    di, dj = i - oi + case.p[0], j - oj + case.p[1]
    return (di >= 0) & (di < case.k[0]) & (dj >= 0) & (dj < case.k[1])


def input_footprint(case, oi, oj):
    """Boolean (H, W) mask of the input pixels inside the patch of output pixel (oi, oj)."""
    h, w = case.hw
    i = torch.arange(h).view(-1, 1)
    j = torch.arange(w).view(1, -1)
    di, dj = i - oi + case.p[0], j - oj + case.p[1]
    return (di >= 0) & (di < case.k[0]) & (dj >= 0) & (dj < case.k[1])


# ---- the host's kernel selection, restated (qiddm_qconv.hip) -----------------------------------------------------------
def _halo(k, p, w):
    """fwd_halo / dx_halo: flat pixels in front of / behind a tile that its patches reach."""
    return max(p[0] * w + p[1], (k[0] - 1 - p[0]) * w + (k[1] - 1 - p[1]))


def gather_packed(c_out):
    """``packed`` of conv_geometry: 2 = one 16-column tile, 1 = one 32-column tile, 3 = 128 channels per workgroup, 0."""
    return 2 if c_out <= 8 else 1 if c_out <= 16 else 3 if c_out >= 96 else 0


def forward_variant(c_in, c_out, k, p, hw, batch, upsample=False):
    """("halo", NCOL, XPT) or ("gemm", packed, upsample, extent beyond 16) of qiddm_qconv_unitary_forward for the image
    the convolution sees (``hw``: after the upsampling).  The gathering kernels keep a kernel coordinate in four bits of
    their tap table and have a form of their own for larger extents."""
    h, w = hw
    ho, wo = h + 2 * p[0] - k[0] + 1, w + 2 * p[1] - k[1] + 1
    packed = gather_packed(c_out)
    f = c_in * k[0] * k[1]
    k_pad = (f + 31) // 32 * 32
    n_pad = {2: 16, 1: 32, 3: (c_out + 127) // 128 * 256, 0: (c_out + 31) // 32 * 64}[packed]
    xs = (FWD_TILE + 2 * _halo(k, p, w)) | 1
    m = batch * ho * wo
    if (not upsample and k[0] * k[1] > 1 and (ho, wo) == (h, w) and packed != 3 and n_pad <= 64 and c_in < 0xffff
            and k[0] * k[1] <= 31 and xs < 0xffff and batch * c_in * h * w < 2 ** 31 and m * c_out < 2 ** 31):
        need = (c_in * xs + FWD_THREADS - 1) // FWD_THREADS
        floats = c_in * xs + k_pad * n_pad + k_pad + (n_pad // 2) * (FWD_TILE + 1) + FWD_TILE
        smem = (floats * 4 + 7) // 8 * 8 + 2 * (n_pad // 2) * 8
        if need <= 40 and smem <= MAX_LDS:
            return ("halo", n_pad, 1 if need <= 1 else 4 if need <= 4 else 12 if need <= 12 else 20)
    return ("gemm", packed, bool(upsample), max(k) > 16)


def dx_variant(c_in, k, p, hw, plan):
    """(K2, CB, PF) of the per-pixel-row dL/dx kernel, or None where the layer keeps the fold.  ``plan``: the plan columns
    (the matrix-core choice is the library's own, restated nowhere)."""
    route, matrix_core, rc = plan[0], plan[1], plan[2]
    h, w = hw
    same = (h + 2 * p[0] - k[0] + 1, w + 2 * p[1] - k[1] + 1) == (h, w)
    if route != "thin" or not matrix_core or not same or c_in > 32 or k[0] * k[1] > 32:
        return None
    k2, halo = 2 * rc, _halo(k, p, w)
    cpad = 16 if c_in <= 16 else 32
    n_src = DX_TILE + 2 * halo
    smem = (n_src * (k2 + 1) + n_src + k[0] * k[1] * k2 * cpad + cpad * (DX_TILE + 1) + 2 * DX_TILE) * 4
    if smem > MAX_LDS // 2:
        return None
    slots = (n_src * (k2 // 4) + DX_THREADS - 1) // DX_THREADS
    return (k2, 1 if c_in <= 16 else 2, 2 if slots <= 2 else 4 if slots <= 4 else 6)


def fold_variant(k):
    return (3, 3) if k == (3, 3) else (1, 1) if k == (1, 1) else (0, 0)


def case_forward_variant(case):
    return forward_variant(case.c_in, case.c_out, case.k, case.p, case.hw, case.batch)


def case_dx_variant(case):
    return dx_variant(case.c_in, case.k, case.p, case.hw, case.plan)


HALO_VARIANTS = {("halo", ncol, xpt) for ncol in (16, 32, 64) for xpt in (1, 4, 12, 20)}
DX_VARIANTS = {(k2, cb, pf) for k2 in (16, 32, 64) for cb in (1, 2) for pf in (2, 4, 6)}
UNREACHABLE_HALO = {("halo", 64, 1)}
UNREACHABLE_DX = {(32, 1, 2), (64, 1, 2), (64, 2, 2), (64, 1, 4), (64, 2, 4)}


def small_layers():
    """(c_in, c_out, k, p, hw) of every same-size layer of at most 9 wires over a grid of small shapes: what the restated
    rule is enumerated on.  Same-size layers only: the halo forward and the dx kernel take no others."""
    for kh in (1, 3, 5):
        for kw in (1, 3, 5, 7, 15, 31):
            for c_in in (1, 2, 3, 4, 7, 8, 16, 17, 32, 33, 64):
                f = c_in * kh * kw
                if f > 512:
                    continue
                for c_out in (4, 8, 9, 16, 17, 32):
                    n = oc.qconv_wires(c_in, c_out, (kh, kw))
                    if n > 9 or 2 * c_out > 2 ** n:
                        continue
                    for hw in ((1, 1), (2, 2), (1, 20), (1, 40), (1, 97), (3, 60)):
                        yield c_in, c_out, (kh, kw), (kh // 2, kw // 2), hw

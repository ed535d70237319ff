"""The one-wavefront-per-item kernel at both of its widths (csrc/qsim_lean_solo.h: dense_lean_solo_kernel<LPR, WAVES>,
WAVES = 8 or 16 wavefronts per workgroup, the phase entries read from LDS one layer ahead) and its partition: wavefront
wv of workgroup b takes the items wv * grid + b, + grid * WAVES, ..; the host (csrc/qiddm_lean.hip: launch_lean) takes
WAVES = 8 while items <= 8 x CUs and 16 above that, grid = min(ceil(items / 8), CUs) at both; QIDDM_LEAN_SOLO_WAVES
forces the width.  The cases sit where that partition changes: the width boundary, wavefronts with 0 .. 3 items, grids shorter
than the chip with idle wavefronts at both barriers, rows told apart by their place in a padded, NaN-filled buffer, the
pair map's edges at width 16 on the plain-store path without a bias, and one launch through both widths.

Every row of a launch must be the same bits; a launch's row is held to the float64 oracle and to the four-wave body
within the tolerance of tests/test_gpu_lean_solo_items.py, whose operands, reference rows and launch helper are used
here as they are (float32, the solo kernel forced by QIDDM_LEAN_SOLO_MIN_ITEMS=0)."""
import functools
import os

import pytest
import torch

from test_gpu_lean_solo_items import TOL, _call, _check, _row

pytestmark = pytest.mark.gpu
SMALL = 36            # a small image: a launch of 16 x CUs items writes about a megabyte


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _split(items):
    """(batch, steps) with batch * steps == items and the most steps <= 15 that divide it."""
    steps = max(s for s in range(1, 16) if items % s == 0)
    return items // steps, steps


def _routed_width(items):
    return 8 if items <= 8 * _cus() else 16


@functools.lru_cache(maxsize=None)
def _quad_row(P, bias):
    """The row of the four-wave body for the same operands (every row of it is this one), computed once."""
    old = os.environ.get("QIDDM_LEAN_SOLO_MIN_ITEMS")
    os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = "-1"
    try:
        _, _, quad = _call(P, 2, 2, P, 2 * P, bias=bias)
    finally:
        if old is None:
            os.environ.pop("QIDDM_LEAN_SOLO_MIN_ITEMS", None)
        else:
            os.environ["QIDDM_LEAN_SOLO_MIN_ITEMS"] = old
    assert torch.equal(quad, quad[0, 0].expand_as(quad))
    return quad[0, 0].clone()


def _solo(monkeypatch, P, batch, steps, what, width=None, bias=True, aligned=None):
    """One launch of the solo kernel into a padded, NaN-filled buffer (`width`: forced, else the host's rule): pads
    untouched, every payload word written, every row the same bits, the row within TOL of the oracle and of the
    four-wave body.  aligned=False: an even y_ld and step stride from a base moved by 8 bytes -- no row is 16-byte
    aligned; None: odd strides, every other row is.  Returns the row."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    if width is None:
        monkeypatch.delenv("QIDDM_LEAN_SOLO_WAVES", raising=False)
    else:
        monkeypatch.setenv("QIDDM_LEAN_SOLO_WAVES", str(width))
    if aligned is None:
        y_ld, pad, offset = P + 5, 11, 0
    else:
        y_ld, pad, offset = P + 6 - P % 2, 12, 0 if aligned else 1
    row = _check(*_call(P, batch, steps, y_ld, batch * y_ld + pad, offset=offset, bias=bias), _row(P, bias),
                 f"{what}: P {P}, batch {batch} x {steps} steps, width {width or _routed_width(batch * steps)}")
    quad = _quad_row(P, bias)
    assert torch.allclose(row, quad, atol=TOL, rtol=TOL), (what, (row - quad).abs().max().item())
    return row


# the host's rule changes the kernel between 8 C and 8 C + 1 items; 16 C items are one per wavefront at width 16
@pytest.mark.parametrize("items", ["8C-1", "8C", "8C+1", "16C"])
def test_width_boundary(items, monkeypatch):
    c = _cus()
    n = {"8C-1": 8 * c - 1, "8C": 8 * c, "8C+1": 8 * c + 1, "16C": 16 * c}[items]
    batch, steps = _split(n)
    row = _solo(monkeypatch, SMALL, batch, steps, items)
    # (the same launch through the other width: the same bits)
    other = _solo(monkeypatch, SMALL, batch, steps, items + " other width", width=24 - _routed_width(n))
    assert torch.equal(row, other)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_items_per_wavefront_at_width_16(k, monkeypatch):
    """(k - 1) 16 C + 8 C + 3 items: the fullest wavefronts have k items, their neighbours k - 1 (none at k = 1)."""
    c = _cus()
    items = (k - 1) * 16 * c + 8 * c + 3
    assert _routed_width(items) == 16 and -(-items // (16 * c)) == k and items % (16 * c) != 0
    batch, steps = _split(items)
    _solo(monkeypatch, SMALL, batch, steps, f"{k} items per wavefront")


def test_benchmark_partition(monkeypatch):
    """256 x 15 at 784 pixels: on 256 CUs 15 items per workgroup, wavefront 15 of every workgroup idle."""
    _solo(monkeypatch, 784, 256, 15, "benchmark", width=16, aligned=True)


# fewer workgroups than CUs; 15 / 17: a workgroup whose later wavefronts have no item and meet both barriers idle
@pytest.mark.parametrize("items", [1, 15, 16, 17, 240])
def test_short_grids(items, monkeypatch):
    batch, steps = _split(items)
    rows = [_solo(monkeypatch, SMALL, batch, steps, f"{items} items", width=w) for w in (None, 8, 16)]
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@pytest.mark.parametrize("batch", [3, "C+1"])
@pytest.mark.parametrize("width", [8, 16])
def test_dealing(batch, width, monkeypatch):
    """15 step planes and the samples kept apart by y_ld = P + 5 and a step stride of batch * y_ld + 11 over NaN: an
    item dealt to the wrong (sample, step) or dealt twice leaves a row unwritten (as many rows are written as there are
    items), one dealt beyond the launch touches a pad word."""
    b = 3 if batch == 3 else _cus() + 1
    _solo(monkeypatch, SMALL, b, 15, f"dealing batch {batch}", width=width)


# the pair map's edges (tests/test_gpu_lean_solo_items.py: test_pair_map_edges) at width 16, on the plain-store path
# (no row 16-byte aligned) and with b_up = NULL
@pytest.mark.parametrize("P", [1, 3, 127, 128, 130, 784])
def test_image_sizes_at_width_16(P, monkeypatch):
    plain = _solo(monkeypatch, P, 7, 5, "plain stores, no bias", width=16, bias=False, aligned=False)
    fast = _solo(monkeypatch, P, 7, 5, "aligned, no bias", width=16, bias=False, aligned=True)
    assert torch.equal(plain, fast)


@pytest.mark.parametrize("P,batch,steps", [(784, 40, 15), (SMALL, 300, 15)])
def test_forced_widths_agree_bit_for_bit(P, batch, steps, monkeypatch):
    narrow = _solo(monkeypatch, P, batch, steps, "forced", width=8)
    wide = _solo(monkeypatch, P, batch, steps, "forced", width=16)
    assert torch.equal(narrow, wide)

"""The one-wavefront-per-item kernel once it simulates the circuit ONCE per workgroup (csrc/qsim_lean_solo.h:
dense_lean_solo_kernel<LPR, WAVES>): wavefront 0 simulates and leaves the eight <Z> in LDS while the threads of
wavefronts 1 .. WAVES - 1 load linear_up's operands, a thread the two rows of a pixel pair (thread t the pairs t,
t + 64 (WAVES - 1): one trip at width 16, a second one at width 8 beyond 896 pixels); behind a barrier those threads
compute the workgroup's one row into LDS, behind another every wavefront reads it into registers (pair = lane + 64 g)
and from there on only stores it, once per item it was dealt.

The cases sit where that can go wrong: the image sizes at the edges of the pair map and of the loaders' trips at both
widths, with and without a bias; launches of one item, around the step from one workgroup to two, with wavefronts that
have no item at the barriers and with wavefronts that have k and k - 1 items; step counts that do and do not divide the
wave stride; both store paths; both widths; and the row of the kernel that simulated every item, kept as a golden file.

Every launch goes into a padded, NaN-filled buffer: the pads stay untouched, every payload word is written, all rows are
the same bits, and the row is within TOL of the float64 oracle row.  Operands, reference rows, the launch helper and TOL
are those of tests/test_gpu_lean_solo_items.py as they are (float32, the solo kernel forced by
QIDDM_LEAN_SOLO_MIN_ITEMS=0)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_lean_solo_items import TOL, _call, _check, _row

pytestmark = pytest.mark.gpu
SMALL = 36            # a small image: a launch of 16 x CUs items writes about a megabyte
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lean_once_row_784.npy")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _split(items):
    """(batch, steps) with batch * steps == items and the most steps <= 15 that divide it."""
    steps = max(s for s in range(1, 16) if items % s == 0)
    return items // steps, steps


def _once(monkeypatch, P, batch, steps, what, width=None, bias=True, aligned=None):
    """One launch of the solo kernel into a padded, NaN-filled buffer (`width`: forced, else the host's rule), checked as
    the module's docstring says.  aligned=True: an even y_ld and step stride from a 16-byte aligned base -- every row is
    16-byte aligned; False: the same from a base moved by 8 bytes -- no row is; None: odd strides, every other row is.
    Returns the row."""
    monkeypatch.setenv("QIDDM_LEAN_SOLO_MIN_ITEMS", "0")
    if width is None:
        monkeypatch.delenv("QIDDM_LEAN_SOLO_WAVES", raising=False)
    else:
        monkeypatch.setenv("QIDDM_LEAN_SOLO_WAVES", str(width))
    if aligned is None:
        y_ld, pad, offset = P + 5, 11, 0
    else:
        y_ld, pad, offset = P + 6 - P % 2, 12, 0 if aligned else 1
    return _check(*_call(P, batch, steps, y_ld, batch * y_ld + pad, offset=offset, bias=bias), _row(P, bias),
                  f"{what}: P {P}, batch {batch} x {steps} steps, width {width or 'routed'}, bias {bias}, aligned {aligned}")


# The one row: a half pair, one pair, a pair and a half (1, 2, 3); one pair short of a wavefront's 64, exactly 64, one
# into the next wavefront (127, 128, 129); the flagship; the last image of width 8's first trip, one pixel short of it
# and the first of its second trip (896, 895, 897); every pair of the largest image and an odd last pair there (1024,
# 1023).  15 items on two workgroups with odd strides: one launch takes both stores.
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("P", [1, 2, 3, 127, 128, 129, 784, 895, 896, 897, 1023, 1024])
def test_image_sizes(P, width, bias, monkeypatch):
    _once(monkeypatch, P, 3, 5, "image sizes", width=width, bias=bias)


# 1: one workgroup whose wavefronts 1 .. WAVES - 1 have no item and meet the barriers idle; 7, 8, 9: the grid goes from
# one workgroup to two; 17: at width 16 a workgroup with one item beside one with none on its later wavefronts
@pytest.mark.parametrize("items", [1, 7, 8, 9, 17])
def test_few_items(items, monkeypatch):
    batch, steps = _split(items)
    rows = [_once(monkeypatch, SMALL, batch, steps, f"{items} items", width=w) for w in (None, 8, 16)]
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_items_per_wavefront_at_width_16(k, monkeypatch):
    """(k - 1) 16 C + 8 C + 3 items: the fullest wavefronts have k items, the others k - 1 (none at k = 1) -- the items are
    dealt round, so the counts of one launch differ by one at most, and the three launches hold 0 and 1, 1 and 2, 2 and
    3."""
    c = _cus()
    items = (k - 1) * 16 * c + 8 * c + 3
    assert items > 8 * c and -(-items // (16 * c)) == k and items % (16 * c) != 0
    batch, steps = _split(items)
    _once(monkeypatch, SMALL, batch, steps, f"{k} items per wavefront")


# the wave stride is 16 C at width 16: 1 and 4 divide it; "odd" is the first of 7, 11, 13 that does not (7 on a chip of
# 2^a CUs, where 15 does not either): a wavefront's second item then sits at another step than its first
@pytest.mark.parametrize("steps", [1, 4, 15, "odd"])
def test_step_counts(steps, monkeypatch):
    stride = 16 * _cus()
    if steps == "odd":
        steps = next(s for s in (7, 11, 13) if stride % s != 0)
    batch = -(-(stride + stride // 2 + 5) // steps)
    assert batch * steps > stride, "some wavefronts have a second item"
    _once(monkeypatch, SMALL, batch, steps, f"{steps} steps", width=16)


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("P", [SMALL, 37])
def test_both_store_paths_agree_bit_for_bit(P, width, monkeypatch):
    aligned = _once(monkeypatch, P, 5, 4, "every row aligned", width=width, aligned=True)
    moved = _once(monkeypatch, P, 5, 4, "no row aligned", width=width, aligned=False)
    mixed = _once(monkeypatch, P, 5, 4, "every other row aligned", width=width)
    assert torch.equal(aligned, moved) and torch.equal(aligned, mixed)


@pytest.mark.parametrize("P,batch,steps", [(784, 40, 15), (SMALL, 300, 15)])
def test_forced_widths_agree_bit_for_bit(P, batch, steps, monkeypatch):
    narrow = _once(monkeypatch, P, batch, steps, "forced", width=8)
    wide = _once(monkeypatch, P, batch, steps, "forced", width=16)
    assert torch.equal(narrow, wide)


@pytest.mark.parametrize("width", [8, 16])
def test_golden_row_of_the_kernel_that_simulated_every_item(width, monkeypatch):
    """tests/golden/lean_once_row_784.npy holds the 784 doubles that the library of the commit BEFORE the circuit was
    simulated once per workgroup wrote for _call's operands at 784 pixels (every row of its launch was that one): the
    same layers, read-out and linear_up arithmetic on the same operands must give the same bits.  The file is written on
    the GPU by tools/golden_lean_once_row.py, which takes the path of the library to run:
        python tools/golden_lean_once_row.py --lib <libqiddm_hip.so of that commit> --out tests/golden/lean_once_row_784.npy
    When the toolchain changes (a compiler that schedules or contracts the float32 layers differently moves the last
    bits of both kernels alike), build that commit with the new toolchain and regenerate the file with it."""
    want = torch.from_numpy(np.load(GOLDEN))
    assert want.dtype == torch.float64 and want.shape == (784,)
    row = _once(monkeypatch, 784, 3, 5, "golden", width=width, aligned=True)
    assert torch.equal(row.cpu(), want), (row.cpu() - want).abs().max().item()

"""``qiddm_amd.nn.derived.derived``: the one cache of weight-derived values, on CPU tensors (no GPU needed)."""
import pytest
import torch

from qiddm_amd.nn.derived import derived


class _Owner(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))
        self.calls = 0

    def value(self, extra=(), result="built", **kw):
        def builder():
            self.calls += 1
            return result
        return derived(self, "slot", (self.w, None), extra, builder, **kw)


@pytest.fixture(autouse=True)
def no_capture_probe(monkeypatch):
    """CPU tensors never ask for the capture state (the question raises without a GPU)."""
    def probe():
        raise AssertionError("the capture probe was consulted for CPU tensors")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", probe)


def test_second_call_hits_and_every_kind_of_weight_change_rebuilds():
    m = _Owner()
    assert m.value() == "built" and m.value() == "built" and m.calls == 1
    with torch.no_grad():
        m.w.add_(1)                                     # in place, as an optimizer step or load_state_dict
    assert m.value() == "built" and m.calls == 2
    m.w.data = m.w.data.clone()                         # same version counter, other storage
    assert m.value() == "built" and m.calls == 3
    assert m.value(extra=("f64",)) == "built" and m.calls == 4       # a changed extra key part
    assert m.value(extra=("f64",)) == "built" and m.calls == 4
    assert m.value(capture="skip") == "built" and m.calls == 5       # (extra differs again) skip builds outside a capture


def test_stamp_follows_the_value_and_a_dropped_entry_rebuilds():
    m = _Owner()
    assert "_derived" not in m.__dict__
    m.value()
    s0 = m._derived["slot"][0]
    m.value()
    assert m._derived["slot"][0] == s0
    with torch.no_grad():
        m.w.mul_(2)
    m.value()
    assert m._derived["slot"][0] != s0
    del m._derived["slot"]                              # dropping the entry (QConv2d.train) is a miss like any other
    assert m.value() == "built" and m.calls == 3


def test_a_cached_none_is_a_hit():
    m = _Owner()
    assert m.value(result=None) is None and m.value(result=None) is None and m.calls == 1


def test_only_cached_on_a_miss_returns_none_and_builds_nothing():
    m = _Owner()
    assert m.value(build=False) is None and m.calls == 0
    assert not m.__dict__.get("_derived")
    assert m.value() == "built" and m.value(build=False) == "built" and m.calls == 1


def test_a_raising_builder_leaves_the_previous_entry():
    m = _Owner()
    m.value()
    entry = m._derived["slot"]
    with torch.no_grad():
        m.w.add_(1)

    def boom():
        raise RuntimeError("builder failed")
    with pytest.raises(RuntimeError, match="builder failed"):
        derived(m, "slot", (m.w, None), (), boom)
    assert m._derived["slot"] is entry


def test_values_stay_out_of_the_state_dict_and_the_buffers():
    m = _Owner()
    derived(m, "slot", (m.w,), (), lambda: torch.ones(2))
    assert list(m.state_dict()) == ["w"] and not list(m.buffers())

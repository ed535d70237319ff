"""Values derived from a module's weights (gate tables, sampler tables, circuit unitaries), kept in the plain attribute
``_derived`` of the module (``{slot: (stamp, value)}``; no buffer, nothing in ``state_dict``) until the weights change.  One stamp rule:
``(t._version, t.data_ptr(), t.device)`` per tensor, plus whatever else selects the value (precision, shapes): an
optimizer step or ``load_state_dict`` moves the version, ``p.data = ...`` / ``.to(device)`` the address or the device."""
from __future__ import annotations

import torch


def derived(owner, slot, tensors, extra, builder, capture="build", build=True):
    """``builder()`` for the current ``tensors`` (None entries allowed) and the tuple ``extra`` of further key parts, cached
    in ``slot`` of ``owner``.  A None result is a value like any other and is cached; a builder that raises leaves the slot as it was.

    On a miss: ``build=False`` returns None (only what is cached); ``capture="skip"`` returns None, uncached, while the
    current stream records a HIP graph (for builders that read a number back); ``capture="build"`` builds regardless.
    The capture state is asked only when a tensor is on the device: without a GPU the question itself raises."""
    stamp = tuple([None if t is None else (t._version, t.data_ptr(), t.device) for t in tensors]) + extra
    try:
        slots = owner.__dict__["_derived"]
    except KeyError:
        slots = owner.__dict__["_derived"] = {}
    entry = slots.get(slot)
    if entry is not None and entry[0] == stamp:
        return entry[1]
    assert capture in ("build", "skip"), capture
    if not build or (capture == "skip" and any(t is not None and t.is_cuda for t in tensors)
                     and torch.cuda.is_current_stream_capturing()):
        return None
    slots[slot] = (stamp, builder())
    return slots[slot][1]

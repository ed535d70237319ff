"""Float64 autograd references for the training kernels' tests.

TEST INFRASTRUCTURE ONLY -- see ``oracle/__init__.py``.  Shared by the small-shape GPU tests and the ones at
training sizes: one fused ``Diffusion`` training step of the dense nets, and the circuit gradients the adjoint
backward computes.  Everything is CPU torch float64 over ``oracle.circuits`` / ``oracle.diffusion``.
"""
from __future__ import annotations

import torch

from . import circuits as oc
from . import diffusion as odf


def dense_step(kind, sd, x, noise, T, shape, goal, detach, h_hook=None):
    """Loss, parameter gradients and reconstruction of one ``Diffusion`` training step of ``QNN_noise``
    (``kind == "qnn"``) or ``QIDDM_LL_noise`` (``"ll"``) by autograd through the oracle.  ``sd`` holds the net's
    parameters under their module names; ``detach`` cuts the gradient through the circuit (``detach_quantum``);
    ``h_hook`` edits the circuit's data angles ``h = W_down x + b_down`` (margin checks of the reference itself)."""
    prm = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in sd.items()}

    def net(t):
        if kind == "qnn":
            w = prm["weights"]
            xr = t.reshape(t.shape[0], -1) @ prm["linear_down.weight"].T + prm["linear_down.bias"]
            xr = xr if h_hook is None else h_hook(xr)
            ev = oc.run_round(oc.Spec(n=w.shape[1], encoding="rz", imprimitive="CZ", measure="expz"), xr,
                              w.unsqueeze(0))
        else:
            w = prm["weights1"]
            xr = t.reshape(t.shape[0], -1) @ prm["linear_down.weight"].T + prm["linear_down.bias"]
            xr = xr if h_hook is None else h_hook(xr)
            ev = oc.run_circuit(oc.Spec(n=w.shape[3], encoding="rz", imprimitive="CZ", measure="expz"), xr, w)
        if detach:
            ev = ev.detach()
        out = ev @ prm["linear_up.weight"].T + prm["linear_up.bias"]
        return out.reshape(t.shape)

    loss, recon = odf.training_loss(net, x.cpu(), T, shape, goal, noise=noise.cpu())
    loss.backward()
    return loss.item(), {k: v.grad for k, v in prm.items()}, recon.detach()


def circuit_grads(spec, x, w, gout):
    """d/dweights and d/dinputs of ``sum(run_circuit(spec, x, w) * gout)``."""
    w = w.clone().requires_grad_(True)
    x = x.clone().requires_grad_(True)
    loss = (oc.run_circuit(spec, x, w) * gout).sum()
    return torch.autograd.grad(loss, [w, x])

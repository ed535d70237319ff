"""The route table of ``qiddm_amd.nn``: one small model call per (class, grad mode, precision, ...) that reaches a kernel.

Shared by tests/test_gpu_nn_routes.py (which launches does the call make, and when are weight-derived tables rebuilt) and
by parent-against-branch parity runs (what does it compute).  Only public names of the package are used, so the same
cases run on any commit.

Smallest shapes that exercise a route: 8 x 8 images (6 wires), 4 hidden features, 2 blocks, 1-2 rounds, batch 3.  The PCA
front-ends need at least as many samples as components (up to 8): those classes get batch 9.  Batch 64 only where
``_UNITARY_ROUTE_MIN_BATCH`` is the thing under test.
"""
import contextlib

import torch

DEV = "cuda"

# every dense class with its constructor arguments at the shapes above
DENSE = {
    "QDenseUndirected_old": (2, 8), "QDenseUndirected_old_noise": (2, 8), "QNN_A": (2, 8),
    "QNN_noise": (64, 4, 2), "QNN": (64, 4, 2),
    "differN_noise": (8, 2, 2), "differN_noise_befor": (8, 2, 2), "differN_old_pca": (8, 2, 2),
    "QIDDM_LL_noise": (64, 4, 2, 2), "QIDDM_LL_relu_noise": (64, 4, 2, 2), "QIDDM_PL_noise": (64, 4, 2, 2),
    "QIDDM_PL": (64, 4, 2, 2), "QIDDM_PL_noise1": (64, 4, 2, 2), "QIDDM_PL_old": (64, 4, 2, 2),
    "QIDDM_LL_old": (64, 4, 2, 2), "QIDDM_bias_false": (64, 4, 2, 2), "QIDDM_L_B": (64, 4, 2, 2),
    "QIDDM_CL_new": (64, 4, 2, 1), "QIDDM_CL_old": (64, 4, 2, 1), "QIDDM_PP_noise": (64, 4, 2, 1),
    "QIDDM_PP_old": (64, 4, 2, 1), "differN_new_pca": (8, 2, 2), "differN_old_conv": (8, 2, 2),
    "differN_new_conv": (8, 2, 2), "QIDDM_A_sameN": (8, 2, 2), "QIDDM_A_differN_basePL": (8, 2, 2),
    "QIDDM_A_differN_NEW": (8, 2, 2),
}
FAMILY_BASES = ("QDenseUndirected_old", "QNN_noise", "differN_noise", "QIDDM_LL_noise")
MIXED = ("QDenseUndirected_old_noise", "QNN_noise", "differN_noise_befor", "QIDDM_LL_noise")
DENSE_FAMILY = ("QNN_noise", "QNN", "QIDDM_LL_noise", "QIDDM_LL_relu_noise", "QIDDM_LL_old")
# entries that launch nothing and are asked once per process and layer shape (``functools.lru_cache``), not per module: whether
# they appear depends on what ran before in the process
HOST_ONLY = ("qiddm_qconv_train_plan",)
PP_OLD_2N = "steps_QIDDM_PP_old_2n"       # input_dim == 2 * hidden_features: the shape coincidence


@contextlib.contextmanager
def _precision(p):
    from qiddm_amd import circuit as qc
    prev = qc._default_precision
    qc.set_default_precision(p)
    try:
        yield
    finally:
        qc.set_default_precision(prev)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(DEV)


def _grads(mods):
    out = {}
    for i, m in enumerate(mods):
        out.update({f"g{i}.{k}": p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
        out.update({f"b{i}.{k}": b.detach().clone() for k, b in m.named_buffers()})
    return out


def _forward_call(mods, fn, x, grad):
    """``fn(x)``; with grad on also the backward of ``sum(y^2)``: outputs, gradients and buffers by name."""
    def call():
        for m in mods:
            m.zero_grad(set_to_none=True)
        if not grad:
            with torch.no_grad():
                return {"y": fn(x)}
        xg = x.detach().clone().requires_grad_(True)
        y = fn(xg)
        if y.requires_grad:
            y.square().sum().backward()
        out = {"y": y.detach(), **_grads(mods)}
        if xg.grad is not None:
            out["gx"] = xg.grad
        return out
    return call


def _dense(name, grad, precision="f32", mixed=False, batch=None):
    def make():
        from qiddm_amd import nn, qml
        torch.manual_seed(len(name))
        net = getattr(nn, name)(*DENSE[name]).to(DEV, dtype=torch.double)
        if mixed:       # what the noise drivers do to the layer before sampling
            net.qdev = qml.device("default.mixed", wires=getattr(net, "wires", None) or net.hidden_features)
            net.qnode = qml.QNode(net._circuit, net.qdev, interface="torch", diff_method=net.diff_method)
        b = batch or (9 if hasattr(net, "pca") else 3)
        return [net], _forward_call([net], net, _rand(b, 1, 8, 8, seed=b), grad), precision
    return make


def _steps(ctor, args, shape=(8, 8), batch=3):
    def make():
        from qiddm_amd import models, nn, noise
        torch.manual_seed(5)
        net = getattr(nn, ctor)(*args)
        diff = models.Diffusion(net, noise.add_normal_noise_multiple, "data", shape).to(DEV, dtype=torch.double).eval()
        x = _rand(batch, 1, *shape, seed=6) * 0.75 + 0.5

        def call():
            with torch.no_grad():
                return {"y": diff.denoise_steps(x, 3)}
        return [diff], call, "f32"
    return make


def _train_step(ctor, args, detach):
    def make():
        from qiddm_amd import nn, noise
        torch.manual_seed(7)
        net = getattr(nn, ctor)(*args, detach_quantum=detach).to(DEV, dtype=torch.double).train()
        x = _rand(3, 64, seed=8)
        field = torch.normal(mean=0.5, std=0.2, size=(3, 64), generator=torch.Generator().manual_seed(9)).to(DEV)
        schedule = noise.add_normal_noise_multiple.schedule(4, 3.0, torch.device(DEV)).reshape(-1)

        def call():
            net.zero_grad(set_to_none=True)
            res = net.fused_train_step(x, field, schedule, "data", want_recon=True)
            assert res is not None, "the fused training step did not engage"
            return {"loss": res["loss"], "recon": res["recon"], **_grads([net])}
        return [net], call, "f32"
    return make


def _qconv_layer(args, training):
    from qiddm_amd import nn
    torch.manual_seed(args[0])
    return nn.QConv2d(*args).to(DEV).train(training)


def _qconv(args, training, grad, precision):
    def make():
        layer = _qconv_layer(args, training)
        return [layer], _forward_call([layer], layer, _rand(2, args[0], 5, 5, seed=10), grad), precision
    return make


def _qconv_eval_forward(with_bn):
    def make():
        layer = _qconv_layer((1, 8, 3, 1, 2), False)
        bn = torch.nn.BatchNorm2d(8).to(DEV, torch.double).eval() if with_bn else None
        if with_bn:
            with torch.no_grad():
                bn.running_mean.copy_(_rand(8, seed=14) * 0.2 + 0.1)
                bn.running_var.copy_(_rand(8, seed=15) + 0.5)
        x = _rand(2, 1, 5, 5, seed=11)

        def call():
            with torch.no_grad():
                y = layer.eval_forward(x, batch_norm=bn)
            assert y is not None, "eval_forward did not engage"
            return {"y": y}
        return [layer] + ([bn] if with_bn else []), call, "f32"
    return make


def _qconv_train_bn():
    def make():
        layer = _qconv_layer((16, 8, 1, 0, 2), True)
        torch.manual_seed(12)
        bn = torch.nn.BatchNorm2d(8).to(DEV, torch.double).train()
        x = _rand(2, 16, 5, 5, seed=13)

        def fn(xg):
            y = layer.train_forward_bn(xg, bn)
            assert y is not None, "train_forward_bn did not engage"
            return y
        return [layer, bn], _forward_call([layer, bn], fn, x, True), "f32"
    return make


def _table():
    t = {}
    for name in DENSE:
        for grad in (False, True):
            t[f"dense_{name}_{'grad' if grad else 'nograd'}"] = _dense(name, grad)
    for name in FAMILY_BASES:
        for grad in (False, True):
            t[f"dense_{name}_{'grad' if grad else 'nograd'}_f64"] = _dense(name, grad, precision="f64")
    for name in MIXED:
        for grad in (False, True):
            t[f"dense_{name}_{'grad' if grad else 'nograd'}_mixed"] = _dense(name, grad, mixed=True)
    t["dense_QDenseUndirected_old_nograd_batch64"] = _dense("QDenseUndirected_old", False, batch=64)
    t["steps_QNN_noise"] = _steps("QNN_noise", (64, 4, 2))
    t["steps_QIDDM_LL_noise_lean8"] = _steps("QIDDM_LL_noise", (64, 8, 2, 2))
    t["steps_QIDDM_LL_noise_general4"] = _steps("QIDDM_LL_noise", (64, 4, 2, 2))
    t["steps_QIDDM_PP_old"] = _steps("QIDDM_PP_old", (64, 4, 2, 1), batch=9)
    t[PP_OLD_2N] = _steps("QIDDM_PP_old", (8, 4, 1, 1), shape=(2, 4), batch=9)
    for ctor, args in (("QNN_noise", (64, 4, 2)), ("QIDDM_LL_noise", (64, 4, 2, 2))):
        for detach in (True, False):
            t[f"train_step_{ctor}_{'detach' if detach else 'quantum'}"] = _train_step(ctor, args, detach)
    for args in ((1, 8, 3, 1, 2), (16, 8, 1, 0, 2)):
        for training in (False, True):
            for grad in (False, True):
                for precision in ("f32", "f64"):
                    mode = f"{'train' if training else 'eval'}_{'grad' if grad else 'nograd'}_{precision}"
                    t[f"qconv_{args[0]}_{args[1]}_{mode}"] = _qconv(args, training, grad, precision)
    t["qconv_eval_forward"] = _qconv_eval_forward(False)
    t["qconv_eval_forward_bn"] = _qconv_eval_forward(True)
    t["qconv_train_forward_bn"] = _qconv_train_bn()
    return t


CASES = _table()


def run_case(name, stepwise=False):
    """Run case ``name``: the call twice, every parameter updated in place, the call a third time.  Returns
    ``(entries, tensors)``: the three sequences of entry names that went through ``_capi.launch`` and the named tensors
    of the three calls.  ``stepwise``: take the fused sampler away first (how a step-by-step sequence is recorded on a
    commit whose sampler still accepts the net)."""
    from qiddm_amd import _capi
    mods, call, precision = CASES[name]()
    if stepwise:
        mods[0].net.fused_sample_steps = None
    real, entries, tensors = _capi.launch, [], {}

    def spy(entry, *args):
        if entry not in HOST_ONLY:
            entries[-1].append(entry)
        return real(entry, *args)
    _capi.launch = spy
    try:
        with _precision(precision):
            for i in range(3):
                if i == 2:
                    with torch.no_grad():
                        for m in mods:
                            for p in m.parameters():
                                p.add_(0.01)
                entries.append([])
                tensors.update({f"call{i}.{k}": v.detach().cpu().clone() for k, v in call().items()})
        torch.cuda.synchronize()
    finally:
        _capi.launch = real
    return entries, tensors

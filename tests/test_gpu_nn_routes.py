"""Which kernels a call of every ``qiddm_amd.nn`` quantum layer reaches, and when its weight-derived tables are rebuilt.

Every case of tests/_nn_route_cases.py runs its model call twice, updates every parameter in place and runs it a third
time, with ``_capi.launch`` (the single launch gateway) wrapped to record the entry names.  The three sequences must
equal tests/golden/nn_routes.json, recorded with the same recorder before the routing of ``nn/`` was gathered into one
decision per layer type: that pins the route (which entries) and the cache behaviour (the second call has no
prepare / tables / unitary launch, the third has them again).

The one recorded exception is ``QIDDM_PP_old`` with ``input_dim == 2 * hidden_features``: its ``forward`` is PCA +
BatchNorm1d + other linears, and only a shape comparison used to keep the fused sampler from running the stock dense
net in its place.  The golden holds the step-by-step sequence for it.
"""
import json
import os

import pytest
import torch

from _nn_route_cases import CASES, DEV, PP_OLD_2N, run_case

pytestmark = pytest.mark.gpu

# cases whose first call builds something from the weights: the second call must do with fewer launches, the third (new
# weights) needs all of them again
REBUILDS = {
    "dense_QDenseUndirected_old_nograd": "qiddm_prepare_gates",
    "dense_QDenseUndirected_old_nograd_batch64": "qiddm_circuit_unitary",
    "dense_differN_noise_nograd": "qiddm_prepare_gates",
    "steps_QIDDM_LL_noise_lean8": "qiddm_dense_sample_lean_prepare",
    "steps_QIDDM_LL_noise_general4": "qiddm_dense_sample_prepare",
    "qconv_1_8_eval_nograd_f32": "qiddm_circuit_unitary",
    "qconv_eval_forward_bn": "qiddm_circuit_unitary",
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "nn_routes.json")) as f:
        return json.load(f)


def test_golden_covers_exactly_the_route_table(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_entries_reached_and_tables_rebuilt_only_on_new_weights(name, golden):
    entries, _ = run_case(name)
    print(name, entries)
    assert all(entries), f"{name}: a call reached no launch: {entries}"      # an empty sequence is a test error
    assert entries == golden[name]
    if name in REBUILDS:
        first, second, third = entries
        assert REBUILDS[name] in first and REBUILDS[name] not in second and len(second) < len(first)
        assert third == first


def test_shape_coincidence_no_longer_reaches_the_fused_sampler():
    """``QIDDM_PP_old(8, 4, ...)`` on 2 x 4 images: ``linear_up`` has as many outputs as the image has pixels."""
    from qiddm_amd import nn
    entries, _ = run_case(PP_OLD_2N)
    assert not [e for seq in entries for e in seq if e.startswith("qiddm_dense_sample")]
    net = nn.QIDDM_PP_old(8, 4, 1, 1).to(DEV, dtype=torch.double)
    x = torch.rand(9, 1, 2, 4, dtype=torch.float64, device=DEV)
    assert net.linear_up.weight.shape[0] == x[0].numel()
    with torch.no_grad():
        assert net.fused_sample_steps(x, 3, "data") is None

"""The float64 yardsticks of tests/f64_ref.py, checked on the CPU (no GPU).

What the GPU tests rely on: a rescaled model is the same function with gradients that
normalise_grads maps back exactly; "edge" weights lie inside and "wide" weights outside the range
_split_range_ok accepts; and the float64 outputs of every input those tests use are finite and
mostly unsaturated (a saturated sigmoid would let any kernel pass)."""
import pytest
import torch

import f64_ref as R


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("weights", ["edge", "wide"])
@pytest.mark.parametrize("z,layers,hidden,B", [(4, 3, 64, 8), (4, 2, 96, 3)])
def test_rescaled_model_is_the_same_function(oracle_mod, z, layers, hidden, B, weights):
    _, H, plain, conv, types, _ = R.gnn_model(z, layers, hidden, "plain")
    _, _, dec, _, _, factors = R.gnn_model(z, layers, hidden, weights)
    llr, gt = R.inputs(B, H.shape[1], seed=7)
    p0, l0, g0 = R.grads64(oracle_mod, plain, conv, H, types, llr, gt)
    p1, l1, g1 = R.grads64(oracle_mod, dec, conv, H, types, llr, gt)
    assert float((p1 - p0).abs().max()) <= 1e-12
    assert abs(float(l1 - l0)) <= 1e-12
    g1n = R.normalise_grads(g1, factors)
    seen = 0
    for k, g in g0.items():
        if g is None:
            assert g1n[k] is None
            continue
        assert _rel(g1n[k], g) <= 1e-10, k
        seen += 1
    assert seen == 2 + 9 * layers + 2
    # the raw gradients of a rescaled W1 do differ: the normaliser is not a no-op
    k = "gnn_layers.0.var_to_check_update.0.weight"
    assert _rel(g1[k], g0[k]) > 1e-3
    # power-of-two factors: the fp32 oracle's products are the plain model's, so are its probs
    q0, _, h0 = R.grads32(oracle_mod, plain, conv, H, types, llr, gt)
    q1, _, h1 = R.grads32(oracle_mod, dec, conv, H, types, llr, gt)
    assert torch.equal(q0, q1)
    h1n = R.normalise_grads(h1, factors)
    for k, g in h0.items():  # ... and its gradients, up to the order the CPU's threads sum in
        if g is not None:
            assert _rel(h1n[k], g) <= 1e-6, k


@pytest.mark.parametrize("hidden", [64, 128])
def test_weight_sets_straddle_the_split_range(hidden):
    for weights, ok in (("plain", True), ("edge", True), ("wide", False)):
        for layers in (2, 3):
            assert R.gnn_model(4, layers, hidden, weights)[2]._split_range_ok() is ok, (weights, layers)
    for z, layers, _, _ in R.HYBRID_SHAPES:
        assert R.hybrid_model(z, layers, 64, "edge")[2]._split_range_ok() is True
        assert R.hybrid_model(z, layers, 64, "wide")[2]._split_range_ok() is False


def test_float64_loss_and_default_dtype(oracle_mod):
    """ground_truth with dtype=float64 returns a float64 loss; the default stays float32."""
    _, H, dec, conv, types, _ = R.gnn_model(4, 2, 32, "plain")
    llr, gt = R.inputs(3, H.shape[1], seed=1)
    sd = dec.state_dict()
    ev, ec = conv.edge_var, conv.edge_chk
    p64, l64 = oracle_mod.gnn_forward(sd, llr, ev, ev, ec, H.shape[1], H.shape[0], types, ground_truth=gt,
                                      dtype=torch.float64)
    p32, l32 = oracle_mod.gnn_forward(sd, llr, ev, ev, ec, H.shape[1], H.shape[0], types, ground_truth=gt)
    assert p64.dtype == l64.dtype == torch.float64 and p32.dtype == l32.dtype == torch.float32
    assert abs(float(l64) - float(l32)) < 1e-5


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("z,layers,hidden,B", R.TRAIN_SHAPES)
def test_training_inputs_are_unsaturated(oracle_mod, z, layers, hidden, B, weights):
    H, dec, conv, types, _, llr, gt = R.train_case(z, layers, hidden, B, weights)
    p64, _ = R.forward_pair(oracle_mod, dec, conv, H, types, llr)
    assert bool(torch.isfinite(p64).all()) and R.unsaturated(p64) > 0.01
    if (z, hidden) == (4, 64):  # the general-adjacency case runs on these inputs too
        q64, _, _ = R.grads64(oracle_mod, dec, conv, H, types, llr, gt, dense=R.non_clique(conv))
        assert bool(torch.isfinite(q64).all()) and R.unsaturated(q64) > 0.01


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("hidden", [64, 32])
@pytest.mark.parametrize("z,layers,B,identity", R.HYBRID_SHAPES)
def test_hybrid_inputs_are_unsaturated(oracle_mod, z, layers, B, identity, hidden, weights):
    H, dec, conv, types, llr = R.hybrid_case(z, layers, hidden, B, weights)
    p64, p32 = R.hybrid_pair(oracle_mod, dec, conv, H, types, llr, identity)
    assert p64.dtype == torch.float64 and p32.dtype == torch.float32
    assert bool(torch.isfinite(p64).all()) and R.unsaturated(p64) > 0.01


@pytest.mark.parametrize("z,hidden,layers,off,units,scale", R.NEARLY_OFF_CASES)
def test_nearly_off_inputs_are_finite_and_unsaturated(oracle_mod, z, hidden, layers, off, units, scale):
    H, dec, conv, types, llr = R.nearly_off_case(z, hidden, layers, off, units, scale)
    assert dec._split_range_ok()  # zero rows are skipped: the split / fused kernels run
    p64, p32 = R.forward_pair(oracle_mod, dec, conv, H, types, llr)
    assert bool(torch.isfinite(p64).all()) and bool(torch.isfinite(p32).all())
    assert R.unsaturated(p64) > 0.01
    if off == 0:
        return
    # what seeds the nearly-off layer's output accumulators: b2v + b2c + x, x the layer before's output
    feats = []
    ev, ec = conv.edge_var, conv.edge_chk
    oracle_mod.gnn_forward(dec.state_dict(), llr, ev, ev, ec, H.shape[1], H.shape[0], types, features=feats)
    layer = dec.gnn_layers[off]
    b2 = layer.var_to_check_update[2].bias + layer.check_to_var_update[2].bias
    seed = (feats[off - 1] + b2).detach().abs().amax(dim=2)
    if scale == 8.0:
        assert float(seed.max()) < 4.0
    else:
        assert float((seed >= 4.0).float().mean()) > 0.1

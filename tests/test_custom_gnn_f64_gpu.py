"""Hybrid GNN decoder (CustomVariableMessageGNNDecoder) against a float64 evaluation of its math (GPU).

tests/test_custom_gnn_gpu.py holds it to 2e-5 of the fp32 oracle on default weights.  Here the
yardstick is oracle.custom_variable_forward in float64 and the bar the project's fp32 contract:
max |p - p64| <= 2 max |p32 - p64| + 1e-7 (p32: the fp32 oracle), on the weight sets of
tests/f64_ref.py -- "plain", "edge" (rows spread over 2^16, inside the f16 splits' range: the split
kernels run) and "wide" (rows spread over 2^30: hidden 64 must fall back to the fp32 products, as
MessageGNNDecoder's inference does).  Hidden 32 runs the tiled fp32 kernels, which no weight range
troubles: the control."""
import pytest
import torch

import f64_ref as R

pytestmark = pytest.mark.gpu


def _run(cuda, oracle_mod, z, layers, B, identity, hidden, weights):
    H, dec, conv, types, llr = R.hybrid_case(z, layers, hidden, B, weights)
    p64, p32 = R.hybrid_pair(oracle_mod, dec, conv, H, types, llr, identity)
    dec = dec.to(cuda)
    Ac = None if identity else conv.check_to_var_adjacency
    Av = None if identity else conv.var_to_check_adjacency
    with torch.no_grad():
        probs, _ = dec(llr.to(cuda), conv.message_to_var_index().to(cuda), types.to(cuda), Av, Ac)
    assert dec._split_ok == (weights != "wide" or hidden != 64)
    p = probs.cpu().double()
    err, err32 = float((p - p64).abs().max()), float((p32.double() - p64).abs().max())
    print(f"hybrid z{z} L{layers} H{hidden} {'identity' if identity else 'clique'} {weights}: native {err:.3e}  "
          f"oracle-f32 {err32:.3e}  bar {2 * err32 + 1e-7:.3e}  (unsaturated {R.unsaturated(p64):.3f})")
    assert bool(torch.isfinite(p).all())
    assert err <= 2 * err32 + 1e-7, (err, err32)


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("z,layers,B,identity", R.HYBRID_SHAPES)
def test_hybrid_gnn_matches_float64(cuda, oracle_mod, z, layers, B, identity, weights):
    _run(cuda, oracle_mod, z, layers, B, identity, 64, weights)


@pytest.mark.parametrize("z,layers,B,identity", R.HYBRID_SHAPES)
def test_hybrid_gnn_tiled_control_matches_float64(cuda, oracle_mod, z, layers, B, identity):
    _run(cuda, oracle_mod, z, layers, B, identity, 32, "wide")

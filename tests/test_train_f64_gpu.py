"""Native GNN training (csrc/gnn.hip's training forward, csrc/gnn_train.hip's backward) against a
float64 evaluation of the same math (GPU).

tests/test_train_gpu.py compares the backward with fp32 autograd at 1e-3 of each tensor's largest
gradient; a backward that dropped a low-order split term would pass it.  Here the yardstick is
autograd through the oracle in float64, and the bars are the project's fp32 contract (tests/f64_ref.py
builds the models, inputs and references; tests/test_f64_ref_host.py checks them on the CPU):

  probs      max |p - p64| <= 2 max |p32 - p64| + 1e-7
  loss       |loss - loss64| <= 2 |loss32 - loss64| + 1e-7 max(1, |loss64|)
  gradients  per parameter tensor, in the plain parametrisation (f64_ref.normalise_grads),
             max |g - g64| <= 2 max |g32 - g64| + 1e-6 layers max |g64|

p32, loss32 and g32 are the fp32 oracle's.  The additive gradient term is what test_train_gpu.py's
docstring expects of two fp32 evaluations ("~1e-6 relative error per layer"); it keeps a tensor the
CPU happens to get almost exactly from setting an unreachable bar.  The fp32 oracle's own per-tensor
error is about 1e-7 relative (median; <= 8e-7 at worst over these configurations), so the bar is
about 3e-6 relative.

Weight sets (f64_ref): "plain"; "edge", rows spread over 2^16 inside the range the f16 splits hold
to fp32 accuracy (the split kernels run); "wide", rows spread over 2^30 (the forward must fall back
to the fp32 products, as inference does)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import f64_ref as R

pytestmark = pytest.mark.gpu

# the H = 64 backward variants tests/test_train_gpu.py toggles
VARIANTS = {
    "default": {},
    "per-message": {"LDPC_GNN_TRAIN_PROJ": "0"},
    "fp32mfma": {"LDPC_GNN_TRAIN_S6": "0"},
    "recompute": {"LDPC_GNN_SAVED_PROJ": "0"},
}
CASES = [(s, "default") for s in R.TRAIN_SHAPES] + \
        [(s, v) for s in R.TRAIN_SHAPES if s[2] == 64 for v in VARIANTS if v != "default"]


def _layer_weights(layers):
    return torch.linspace(0.5, 1.0, layers).tolist()


@functools.lru_cache(maxsize=None)
def _refs(shape, weights, kind):
    """(p64, loss64, g64, p32, loss32, g32) of one case, gradients normalised; computed once and
    shared by the variants."""
    import oracle
    oracle.build()
    z, layers, hidden, B = shape
    H, dec, conv, types, factors, llr, gt = R.train_case(z, layers, hidden, B, weights)
    kw = {}
    if kind == "all-layers":
        kw["layer_weights"] = _layer_weights(layers)
    elif kind == "non-clique":
        kw["dense"] = R.non_clique(conv)
    out = []
    for fn in (R.grads64, R.grads32):
        p, loss, g = fn(oracle, dec, conv, H, types, llr, gt, **kw)
        g = {k: (v.double() if v is not None else None) for k, v in g.items()}
        out += [p.double(), float(loss), R.normalise_grads(g, factors)]
    return tuple(out)


def _compare(tag, layers, dec, factors, probs, loss, refs):
    p64, l64, g64, p32, l32, g32 = refs
    fails = []

    def row(name, err, err32, bar):
        line = f"{tag} {name}: native {err:.3e}  oracle-f32 {err32:.3e}  bar {bar:.3e}"
        print(line)
        if not err <= bar:
            fails.append(line)

    p = probs.detach().cpu().double()
    e32 = float((p32 - p64).abs().max())
    row("probs", float((p - p64).abs().max()), e32, 2 * e32 + 1e-7)
    e32 = abs(l32 - l64)
    row("loss", abs(float(loss) - l64), e32, 2 * e32 + 1e-7 * max(1.0, abs(l64)))
    native = R.normalise_grads({k: (q.grad.detach().cpu().double() if q.grad is not None else None)
                                for k, q in dec.named_parameters()}, factors)
    seen = 0
    for name, g in native.items():
        if g64[name] is None:
            assert g is None, f"{name}: the reference has no gradient, native has one"
            continue
        assert g is not None, f"{name}: missing gradient"
        e32 = float((g32[name] - g64[name]).abs().max())
        row(name, float((g - g64[name]).abs().max()), e32, 2 * e32 + 1e-6 * layers * float(g64[name].abs().max()))
        seen += 1
    assert seen == 2 + 9 * layers + 2  # every used parameter compared
    assert not fails, "\n".join(fails)


def _env(monkeypatch, variant):
    for k in ("LDPC_GNN_TRAIN_PROJ", "LDPC_GNN_TRAIN_OVERLAP", "LDPC_GNN_TRAIN_S6", "LDPC_GNN_SAVED_PROJ"):
        monkeypatch.setenv(k, VARIANTS[variant].get(k, "1"))


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("shape,variant", CASES, ids=[f"z{s[0]}-L{s[1]}-H{s[2]}-B{s[3]}-{v}" for s, v in CASES])
def test_training_matches_float64(cuda, oracle_mod, monkeypatch, shape, variant, weights):
    _env(monkeypatch, variant)
    z, layers, hidden, B = shape
    H, dec, conv, types, factors, llr, gt = R.train_case(z, layers, hidden, B, weights)
    refs = _refs(shape, weights, "last")
    assert dec._split_range_ok() == (weights != "wide" or hidden == 32)
    dec = dec.to(cuda)
    probs, loss = dec(llr.to(cuda), conv.message_to_var_index(), types, conv.var_to_check_adjacency,
                      conv.check_to_var_adjacency, ground_truth=gt.to(cuda))
    assert probs.requires_grad and loss.requires_grad
    loss.backward()
    _compare(f"z{z} L{layers} H{hidden} {variant} {weights}", layers, dec, factors, probs, loss.item(), refs)


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
def test_deep_supervision_matches_float64(cuda, oracle_mod, weights):
    """forward_all_layers and the layer-weighted loss (ldpc_gnn_layer_probs / ldpc_gnn_backward_ds):
    every layer's probs and the gradients of the weighted sum of their BCEs."""
    shape = R.TRAIN_SHAPES[0]
    z, layers, hidden, B = shape
    H, dec, conv, types, factors, llr, gt = R.train_case(z, layers, hidden, B, weights)
    refs = _refs(shape, weights, "all-layers")
    dec = dec.to(cuda)
    p = dec.forward_all_layers(llr.to(cuda), conv.message_to_var_index(), types, conv.var_to_check_adjacency,
                               conv.check_to_var_adjacency)
    assert p.shape == (layers, B, H.shape[1])
    g = gt.to(cuda)
    loss = sum(w * F.binary_cross_entropy(p[i], g) for i, w in enumerate(_layer_weights(layers)))
    loss.backward()
    _compare(f"z{z} L{layers} H{hidden} all-layers {weights}", layers, dec, factors, p, loss.item(), refs)


@pytest.mark.parametrize("weights", list(R.WEIGHT_SETS))
def test_general_adjacency_matches_float64(cuda, oracle_mod, weights):
    """The CSR plan ("non-clique" of tests/test_train_gpu.py) against the dense bmm in float64.  Its
    unnormalised sums of up to 23 features saturate some probs to 1.0 in fp32, where torch's BCE clamps
    the log: the fp32 oracle's own loss is 0.05 and its gradients about 1 % from float64 here, so this
    case's loss and gradient bars are that loose (measured: native = fp32 oracle to the printed digits);
    its probs bar is the usual one (fp32 oracle 3.9e-7, native 8.2e-7)."""
    shape = R.TRAIN_SHAPES[0]
    z, layers, hidden, B = shape
    H, dec, conv, types, factors, llr, gt = R.train_case(z, layers, hidden, B, weights)
    refs = _refs(shape, weights, "non-clique")
    Av, Ac = R.non_clique(conv)
    dec = dec.to(cuda)
    probs, loss = dec(llr.to(cuda), conv.message_to_var_index(), types, Av, Ac, ground_truth=gt.to(cuda))
    loss.backward()
    _compare(f"z{z} L{layers} H{hidden} non-clique {weights}", layers, dec, factors, probs, loss.item(), refs)


@pytest.mark.parametrize("hidden", [64, 128, 32])
def test_device_range_check_agrees_with_host(cuda, hidden):
    """ldpc_gnn_split_range_exceeded, the kernel the training forward asks at every step, decides as
    MessageGNNDecoder._split_range_ok does (the inference path's check, once per weight version): on
    the three weight sets, with a row zeroed (zero rows do not count), and at the threshold itself --
    one row's largest weight at exactly 2^-17 of its group's largest (inside) and one ulp below."""
    from ldpc_neural_decoder import _native as N

    def exceeded(dec):
        blob = dec._weights_blob(cuda)
        T = dec.gnn_layers[0].message_type_embeddings.shape[0]
        word = torch.full((1,), -1, dtype=torch.int32, device=cuda)
        N.check(N.lib().ldpc_gnn_split_range_exceeded(dec.hidden_dim, T, len(dec.gnn_layers), N.ptr(blob),
                                                      dec.SPLIT_RANGE, N.ptr(word), N.stream_ptr(cuda)))
        return {0: False, 1: True}[int(word.item())]

    for weights in R.WEIGHT_SETS:
        dec = R.gnn_model(4, 3, hidden, weights)[2].to(cuda)
        assert exceeded(dec) == (not dec._split_range_ok()), weights
    dec = R.gnn_model(4, 2, hidden, "plain")[2].to(cuda)
    w1 = dec.gnn_layers[1].check_to_var_update[0].weight
    with torch.no_grad():
        w1[5] = 0.0
        assert dec._split_range_ok() and not exceeded(dec)
        # the projection's group (the W1 right halves): its largest |w| to 1, row 7's to 2^-17
        w1[3, hidden:] = 0.0
        w1[3, hidden] = 1.0
        w1[7, hidden:] = 0.0
        for tiny, ok in ((2.0 ** -17, True), (2.0 ** -17 * (1 - 2.0 ** -24), False)):
            w1[7, hidden + 2] = tiny
            want = ok or hidden == 32  # hidden 32: fp32 fma chains, nothing to exceed
            assert dec._split_range_ok() == want
            assert exceeded(dec) == (not want)

"""float64 yardsticks for the GNN decoders' fp32 contract (CPU; shared by the GPU tests and their
host test, tests/test_f64_ref_host.py).

The contract (README, "numerical contract"): an fp32 path's error against a float64 evaluation of
the same math stays within 2x that of the fp32 oracle (torch fp32 on the CPU).  This module builds
the models and inputs those tests use, and the three things they compare: the native result, the
fp32 oracle's and the float64 oracle's.

Weight sets.  "plain" is the decoder's default initialisation x 0.5.  "edge" and "wide" are the
plain model with hidden unit i of every MLP rescaled: row i of W1 and b1[i] times r_i = 2^k_i, column
i of W2 times 1 / r_i.  ReLU commutes with a positive scale, so the rescaled model is the same
function, and because the factors are powers of two every fp32 product and sum is the plain model's
times a power of two: the fp32 oracle's error is the same for all three sets (no value comes near
fp32's exponent limits).  The kernels' f16 splits share one power-of-two scale per weight group, so
what changes is how many bits the small rows keep.  "edge" (k in [-8, 8]) stays inside the range
MessageGNNDecoder._split_range_ok accepts (2^-17 between a group's smallest and largest row), "wide"
(k in [-24, 6]) is outside it.

Gradients of a rescaled model are mapped back to the plain parametrisation before they are
compared (normalise_grads): dL/dW1[i, :] * r_i, dL/db1[i] * r_i, dL/dW2[:, i] / r_i.  A per-tensor
max-norm then weighs every hidden unit alike; without it the rows that leave the splits' range are
invisible under max |g|."""
import functools

import torch
import torch.nn.functional as F

from conftest import code_path

from ldpc_neural_decoder.models import create_custom_variable_message_gnn_decoder, create_message_gnn_decoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

MLPS = ("var_to_check_update", "check_to_var_update")
WEIGHT_SETS = {"plain": None, "edge": (-8, 8), "wide": (-24, 6)}

# (Z, layers, hidden, B): the smallest shapes of tests/test_train_gpu.py
TRAIN_SHAPES = [(4, 3, 64, 8), (4, 2, 32, 5), (32, 2, 64, 2), (4, 2, 96, 3)]
# (Z, layers, B, identity adjacency) of the hybrid decoder at hidden 64, and its hidden-32 control
HYBRID_SHAPES = [(4, 3, 8, False), (4, 3, 8, True), (32, 2, 2, False)]
# (Z, hidden, layers, which layer is nearly off, "all" units or the var side's "first32", LLR scale),
# B = 4: the first layer (no residual) and a later one (residual; Z = 32 stays at two layers).  LLRs
# (randn * 2 + 1) * 8 leave the residual below 4 everywhere (largest |x + b2| about 2.7), and a seed
# below 4 times the largest scale 2^126 is still finite; * 32 takes it past 4 on more than a tenth of the messages, where
# an uncapped scale overflows (tests/test_f64_ref_host.py checks both statements)
NEARLY_OFF_CASES = [(4, 64, 3, 0, "all", 8.0), (4, 64, 3, 1, "all", 8.0), (32, 64, 2, 0, "all", 8.0),
                    (32, 64, 2, 1, "all", 8.0), (4, 128, 3, 0, "all", 8.0), (4, 128, 3, 1, "all", 8.0),
                    (4, 192, 3, 0, "all", 8.0), (4, 192, 3, 1, "all", 8.0), (4, 128, 3, 0, "first32", 8.0),
                    (4, 192, 3, 1, "first32", 8.0),
                    (4, 64, 3, 1, "all", 32.0), (32, 64, 2, 1, "all", 32.0), (4, 128, 3, 1, "all", 32.0),
                    (4, 192, 3, 1, "all", 32.0), (4, 128, 3, 1, "first32", 32.0), (4, 192, 3, 1, "first32", 32.0)]


def draw_exponents(dec, lo, hi, seed):
    """Integer exponents k_i, uniform in [lo, hi], one per hidden unit of every layer's two MLPs."""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randint(lo, hi + 1, (dec.hidden_dim,), generator=g) for _ in MLPS] for _ in dec.gnn_layers]


def rescale_rows(dec, ks):
    """Rescale hidden unit i of every MLP by 2^ks[layer][mlp][i] (see the module docstring), in
    place.  Returns the factors r in the same nesting."""
    factors = []
    with torch.no_grad():
        for layer, kl in zip(dec.gnn_layers, ks):
            fl = []
            for name, k in zip(MLPS, kl):
                seq = getattr(layer, name)
                r = torch.ldexp(torch.ones(k.shape[0]), k).to(seq[0].weight.device)
                seq[0].weight.mul_(r.view(-1, 1))
                seq[0].bias.mul_(r)
                seq[2].weight.div_(r.view(1, -1))
                fl.append(r)
            factors.append(fl)
    return factors


def normalise_grads(grads, factors):
    """{state_dict key: gradient or None} of a model rescaled by `factors` (None: a plain model)
    -> the plain parametrisation's gradients (new tensors; the other entries pass through)."""
    out = dict(grads)
    if factors is None:
        return out
    for l, fl in enumerate(factors):
        for name, r in zip(MLPS, fl):
            p = f"gnn_layers.{l}.{name}."
            r = r.to("cpu", torch.float64)
            for key, f in ((p + "0.weight", r.view(-1, 1)), (p + "0.bias", r), (p + "2.weight", 1.0 / r.view(1, -1))):
                if out.get(key) is not None:
                    out[key] = out[key] * f.to(out[key].dtype)
    return out


def _graph(z):
    base = load_base_matrix(code_path(z))
    return base, expand_base_matrix(base, z)


def _scaled(dec, weights, seed):
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(0.5)
    rng = WEIGHT_SETS[weights]
    if rng is None:
        return None
    # "edge" tests the threshold itself, so its exponents must leave the model inside the range; many
    # draws from [-8, 8] do not at H = 64 (its second group also holds W1v_left + W1v_right, whose rows
    # reach twice a W1 row's size, and 2^-16 / 2 is the threshold).  Rejection sampling: the first draw
    # of a fixed sequence that _split_range_ok accepts, i.e. uniform exponents conditioned on the range.
    plain = {k: v.clone() for k, v in dec.state_dict().items()}
    for attempt in range(64):
        factors = rescale_rows(dec, draw_exponents(dec, rng[0], rng[1], seed + 1000 + attempt))
        if weights != "edge" or dec._split_range_ok():
            return factors
        dec.load_state_dict(plain)
    raise AssertionError("no draw of edge exponents stays inside the splits' range")


def gnn_model(z, layers, hidden, weights, seed=0):
    """-> (base, H, decoder on the CPU, converter, message types, factors or None)."""
    base, H = _graph(z)
    torch.manual_seed(seed)
    dec, conv = create_message_gnn_decoder(H, num_iterations=layers, hidden_dim=hidden, base_graph=base, Z=z)
    factors = _scaled(dec, weights, seed)
    return base, H, dec, conv, conv.get_message_types(base, z), factors


def hybrid_model(z, layers, hidden, weights, seed=0):
    base, H = _graph(z)
    torch.manual_seed(seed)
    dec, conv = create_custom_variable_message_gnn_decoder(H, num_iterations=layers, hidden_dim=hidden,
                                                           base_graph=base, Z=z)
    factors = _scaled(dec, weights, seed)
    return base, H, dec, conv, conv.get_message_types(base, z), factors


def inputs(B, n, seed, llr_scale=1.0):
    """LLRs (randn * 2 + 1) * llr_scale and a 30 % ones ground truth, from their own generator."""
    g = torch.Generator().manual_seed(seed)
    llr = (torch.randn(B, n, generator=g) * 2 + 1.0) * llr_scale
    gt = (torch.rand(B, n, generator=g) < 0.3).float()
    return llr, gt


def nearly_off_model(z, hidden, layers, off_layer, units, seed=0):
    """A plain model whose layer `off_layer` has W1 = 0 and b1 = 1e-30 in both MLPs ("all"), or in
    the first 32 hidden units of the var side's MLP alone ("first32"): relu(h) there is 1e-30, which
    the split MLPs scale up by close to 2^126 beside a residual and output biases of ordinary size."""
    base, H, dec, conv, types, _ = gnn_model(z, layers, hidden, "plain", seed)
    layer = dec.gnn_layers[off_layer]
    with torch.no_grad():
        for name in (MLPS if units == "all" else MLPS[:1]):
            seq = getattr(layer, name)
            rows = slice(None) if units == "all" else slice(0, 32)
            seq[0].weight[rows] = 0.0
            seq[0].bias[rows] = 1e-30
    return base, H, dec, conv, types


def train_case(z, layers, hidden, B, weights):
    """The model and inputs of one training test: (H, dec, conv, types, factors, llr, gt)."""
    _, H, dec, conv, types, factors = gnn_model(z, layers, hidden, weights)
    llr, gt = inputs(B, H.shape[1], seed=z + hidden)
    return H, dec, conv, types, factors, llr, gt


def hybrid_case(z, layers, hidden, B, weights):
    _, H, dec, conv, types, _ = hybrid_model(z, layers, hidden, weights)
    return H, dec, conv, types, inputs(B, H.shape[1], seed=z + layers)[0]


def nearly_off_case(z, hidden, layers, off_layer, units, llr_scale):
    _, H, dec, conv, types = nearly_off_model(z, hidden, layers, off_layer, units)
    return H, dec, conv, types, inputs(4, H.shape[1], seed=z + hidden, llr_scale=llr_scale)[0]


def non_clique(conv):
    """The general adjacency of tests/test_train_gpu.py ("non-clique"): an unnormalized 0/1 var
    clique beside the normalized check matrix, which runs on the CSR plan."""
    import numpy as np
    ev = torch.as_tensor(conv.edge_var.astype(np.int64))
    return (ev.view(-1, 1) == ev.view(1, -1)).float(), conv.check_to_var_adjacency.clone()


def unsaturated(p64):
    """The fraction of probs within 0.49 of 0.5: what keeps a test from passing on a saturated sigmoid."""
    return float(((p64 - 0.5).abs() < 0.49).double().mean())


def _leaves(dec, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in dec.state_dict().items()}


def oracle_grads(oracle_mod, dec, conv, H, types, llr, gt, dtype, layer_weights=None, dense=None):
    """Autograd through the oracle in `dtype` on the CPU -> (probs, loss, {key: gradient or None}).
    Default: gnn_forward and the BCE of the last layer's probs.  layer_weights (one per layer): the
    probs of every layer (all_layers) and the weighted sum of their BCEs.  dense = (Av, Ac): the
    reference's dense bmm with those adjacencies (gnn_forward_dense)."""
    sd = _leaves(dec, dtype)
    llr, gt = llr.cpu().to(dtype), gt.cpu().to(dtype)
    ev, ec = conv.edge_var, conv.edge_chk
    if dense is not None:
        probs = oracle_mod.gnn_forward_dense(sd, llr, ev, H.shape[1], dense[0], dense[1], types, dtype=dtype)
    else:
        probs = oracle_mod.gnn_forward(sd, llr, ev, ev, ec, H.shape[1], H.shape[0], types,
                                       all_layers=layer_weights is not None, dtype=dtype)
    if layer_weights is not None:
        loss = sum(w * F.binary_cross_entropy(probs[i], gt) for i, w in enumerate(layer_weights))
    else:
        loss = F.binary_cross_entropy(probs, gt)
    loss.backward()
    return probs.detach(), loss.detach(), {k: v.grad for k, v in sd.items()}


grads64 = functools.partial(oracle_grads, dtype=torch.float64)
grads32 = functools.partial(oracle_grads, dtype=torch.float32)


def forward_pair(oracle_mod, dec, conv, H, types, llr):
    """(float64, fp32) oracle probs of a MessageGNNDecoder."""
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ev, ec = conv.edge_var, conv.edge_chk
    run = lambda dt: oracle_mod.gnn_forward(sd, llr.cpu(), ev, ev, ec, H.shape[1], H.shape[0], types, dtype=dt)
    return run(torch.float64), run(None)


def hybrid_pair(oracle_mod, dec, conv, H, types, llr, identity):
    """(float64, fp32) oracle probs of a CustomVariableMessageGNNDecoder."""
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    run = lambda dt: oracle_mod.custom_variable_forward(sd, llr.cpu(), conv.edge_var, conv.edge_chk, H.shape[1],
                                                        H.shape[0], types=types, check_identity=identity, dtype=dt)
    return run(torch.float64), run(None)

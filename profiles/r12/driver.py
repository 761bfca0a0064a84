"""Launch-list driver: BG2 Z = 4 and Z = 32, B = 130, 3 layers, through every GNN host path.
Static switches (LDPC_GNN_PROJ, LDPC_GNN_D1) come from the environment of the process; the per-call
ones are toggled here.  Run under the profiler's kernel trace, once per library (LDPC_AMD_LIB) and
environment; launch_list.py turns each trace into a list.  Usage: driver.py [all|fp32only]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.exists(os.path.join(ROOT, "bench.py")):  # the repository root, from wherever this lies
    ROOT = os.path.dirname(ROOT)
sys.path.insert(0, os.path.join(ROOT, "ldpc-neuralnetwork-decoder_amd"))
from ldpc_neural_decoder.models import (create_custom_variable_message_gnn_decoder,  # noqa: E402
                                        create_message_gnn_decoder)
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "all"
dev = torch.device("cuda", 0)
B, LAYERS = 130, 3


def code(z):
    base = load_base_matrix(os.path.join(ROOT, "codes", f"NR_2_0_{z}.txt"))
    return base, expand_base_matrix(base, z)


def llrs(H, seed):
    return (torch.randn(B, H.shape[1], generator=torch.Generator().manual_seed(seed)) * 2 + 1).to(dev)


def gnn(z, hidden, seed=0):
    torch.manual_seed(seed)
    base, H = code(z)
    dec, conv = create_message_gnn_decoder(H, num_iterations=LAYERS, hidden_dim=hidden, base_graph=base, Z=z)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(0.5)
    return dec.to(dev), conv, conv.get_message_types(base, z), H


def fwd(dec, conv, types, H, seed=1, Av=None, Ac=None):
    Av = conv.var_to_check_adjacency if Av is None else Av
    Ac = conv.check_to_var_adjacency if Ac is None else Ac
    with torch.no_grad():
        p = dec(llrs(H, seed), conv.message_to_var_index(), types, Av, Ac)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p).all())
    return p


def with_env(name, fn):
    os.environ[name] = "0"
    try:
        fn()
    finally:
        del os.environ[name]


for z in (4, 32):
    print("case fp32 H=64 default z", z, flush=True)
    dec, conv, types, H = gnn(z, 64)
    fwd(dec, conv, types, H)
    if mode == "fp32only":
        continue
    for sw in ("LDPC_GNN_SPLIT", "LDPC_GNN_ROWWALK", "LDPC_GNN_PCLDS"):
        print("case", sw, "= 0", flush=True)
        with_env(sw, lambda: fwd(dec, conv, types, H))
    print("case FP32_PRODUCTS", flush=True)
    dec._weights_blob(dev)
    dec._split_ok = False
    fwd(dec, conv, types, H)
    for hidden in (32, 128):
        print("case fp32 H =", hidden, flush=True)
        d2, c2, t2, H2 = gnn(z, hidden)
        fwd(d2, c2, t2, H2)
    if z == 4:  # a general adjacency (dense E x E input): the weighted CSR plan
        print("case weighted", flush=True)
        d3, c3, t3, H3 = gnn(z, 64, seed=3)
        ev = torch.as_tensor(c3.edge_var.astype(np.int64))
        fwd(d3, c3, t3, H3, Av=(ev.view(-1, 1) == ev.view(1, -1)).float(), Ac=c3.check_to_var_adjacency.clone())
    print("case bf16 early stop", flush=True)
    d4, c4, t4, H4 = gnn(z, 64)
    d4.precision = "bf16"
    d4.early_termination = True
    fwd(d4, c4, t4, H4)
    for hidden in (64, 32):
        print("case hybrid H =", hidden, flush=True)
        torch.manual_seed(5)
        base, Hm = code(z)
        hd, hc = create_custom_variable_message_gnn_decoder(Hm, num_iterations=LAYERS, hidden_dim=hidden,
                                                            base_graph=base, Z=z)
        hd = hd.to(dev)
        with torch.no_grad():
            hp, _ = hd(llrs(Hm, 2), hc.message_to_var_index().to(dev), hc.get_message_types(base, z).to(dev),
                       hc.var_to_check_adjacency, hc.check_to_var_adjacency)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(hp).all())
    print("case train step", flush=True)
    d5, c5, t5, H5 = gnn(z, 64)
    p = d5(llrs(H5, 7), c5.message_to_var_index(), t5, c5.var_to_check_adjacency, c5.check_to_var_adjacency)
    p.sum().backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(q.grad).all()) for q in d5.parameters() if q.grad is not None)
print("driver ok", flush=True)

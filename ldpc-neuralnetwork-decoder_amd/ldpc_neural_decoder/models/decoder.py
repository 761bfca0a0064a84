"""Neural min-sum decoder assembled from the index-gather layers (models/layers.py).

The reference imports ``LDPCNeuralDecoder`` from ``ldpc_neural_decoder/models/decoder.py``
(main.py:6, constructed at main.py:66-71 as ``LDPCNeuralDecoder(num_nodes=E, num_iterations,
depth_L)``) and trains/evaluates it through the protocol of training/trainer.py:93,185,251:

    soft_bits, loss = decoder(llrs, check_index_tensor, var_index_tensor, transmitted_bits)
    hard_bits = decoder.decode(llrs, check_index_tensor, var_index_tensor)

with ``llrs`` (B, N) channel LLRs, the index tensors of create_LLR_mapping (utils/ldpc_utils.py:
62-95, var-major edge numbering) and ``loss`` a per-frame vector (the trainer takes ``.mean()``).
That file is not in the reference tree, so this module DEFINES the decoder on the reference's
layers -- parity at the decoder level is unpinned; every layer it is built from is pinned to the
reference by tests/golden/layers_z4.npz.  The structure follows the notebook prototype
LDPCDecoderResidual (EE4002R_2025.ipynb cell 11): check layer -> variable layer with channel and
residual weights -> output mapping.  Iteration l = 0..I-1 runs a check layer; every iteration
but the last is followed by a variable layer with its own ResidualLayer(E, depth_L) weights, and
the last check layer's messages feed the output mapping (as the prototype's forward does):

    x0[b, e]  = llrs[b, var(e)]                                  edge view of the channel LLRs
    c_l       = CheckLayer(v_{l-1}, check_index_tensor)          (v_{-1} = x0)
    v_l       = w_ch_l * x0 + sum_{e' in var(e), e' != e} c_l[e'] + sum_i w_res_l[i] v_{l-1-i}
    app[b, j] = sum_{e in var j} c_{I-1}[e]
    soft, max_loss = OutputLayer(-app, -llrs, ground_truth)      P(bit = 1) = sigmoid(-(llr + app))

The sign: the channel's LLR is log P(0)/P(1) (channel.py:127-148), so P(bit = 1) is
sigmoid(-LLR); the negation is explicit here rather than left to training (MessageGNN keeps the
reference's sigmoid(+LLR), message_gnn_decoder.py:307).  Every gather, min-sum, sum, residual
and output op runs in csrc/layers.hip; there is no CPU path.

Inference takes one fused kernel instead (csrc/neural_ms.hip, ``ldpc_neural_forward``): when no
gradient can be asked for (grad mode off, or neither ``llrs`` nor any parameter requires grad), both
index tensors have create_LLR_mapping's group structure and a frame's messages fit one CU's LDS,
every iteration of a frame runs inside that kernel with its messages in LDS.  It evaluates exactly the
layer kernels' float32 operation sequence, so ``soft`` (and, with ``ground_truth``, the loss, which
the output layer still computes from the kernel's ``app``) is the layer path's bit for bit.  Anything
else -- training, ragged or non-group index tensors, E >= 65536, depth_L > 8, frames too large for
LDS -- runs the layers as before.  ``decoder.use_fused = False`` or ``LDPC_NEURAL_FUSED=0`` in the
environment force the layer path.
"""
import os

import torch
import torch.nn as nn

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models.layers import (
    OutputLayer, ResidualLayer, _check_groups, _check_index, _var_groups, check_minsum, gather_sum)

_STRUCT = {}
_PLANS = {}  # (index tensor identities and versions, device) -> NativeNeuralPlan, or None (no group structure)


def edge_variables(var_index_tensor):
    """Variable of every var-major LLR index, from the "other edges of my variable" table: edge
    e starts a new variable unless e - 1 is one of its neighbours (utils/ldpc_utils.py:77
    numbers the edges variable by variable)."""
    v = torch.as_tensor(var_index_tensor).cpu().long()
    E = v.shape[0]
    if E == 0:
        return torch.zeros(0, dtype=torch.long)
    same = (v[1:] == torch.arange(E - 1).unsqueeze(1)).any(dim=1) if v.shape[1] else torch.zeros(E - 1, dtype=torch.bool)
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum((~same).long(), 0)])


def _structure(var_index_tensor, n_vars, dev):
    """(x0 index (1, E), app index (dv_max, N)) in the kernels' prepared layout, cached per
    index tensor."""
    key = (id(var_index_tensor), var_index_tensor.data_ptr(), var_index_tensor._version, n_vars, str(dev))
    hit = _STRUCT.get(key)
    if hit is not None and hit[0] is var_index_tensor:
        return hit[1]
    var_of = edge_variables(var_index_tensor)
    E = var_of.numel()
    n_found = int(var_of[-1]) + 1 if E else 0
    if n_found != n_vars:
        raise RuntimeError(f"var_index_tensor describes {n_found} variables but llrs has {n_vars} columns")
    deg = torch.bincount(var_of, minlength=n_vars)
    start = torch.cumsum(deg, 0) - deg
    dmax = int(deg.max()) if E else 1
    slot = torch.arange(E) - start[var_of]
    app = torch.full((dmax, n_vars), -1, dtype=torch.int32)
    app[slot, var_of] = torch.arange(E, dtype=torch.int32)
    prepared = (var_of.to(torch.int32).unsqueeze(0).to(dev), app.to(dev))
    if len(_STRUCT) > 8:
        _STRUCT.clear()
    _STRUCT[key] = (var_index_tensor, prepared)
    return prepared


def _fused_plan(check_index_tensor, var_index_tensor, cidx, vidx, E, dev):
    """The fused kernel's plan for this pair of index tensors, or None when either lacks the group
    structure (or E needs more than 16-bit indices); cached per pair, keyed as _structure keys."""
    ct, vt = torch.as_tensor(check_index_tensor), torch.as_tensor(var_index_tensor)
    key = (id(ct), ct.data_ptr(), ct._version, id(vt), vt.data_ptr(), vt._version, str(dev))
    hit = _PLANS.get(key)
    if hit is not None and hit[0] is ct and hit[1] is vt:
        return hit[2]
    plan = None
    if 0 < E < 65536:
        cg, vptr = _check_groups(cidx, E), _var_groups(vidx, E)
        if cg is not None and vptr is not None:
            tables = (cg[0].cpu().numpy(), cg[1].cpu().numpy(), vptr.cpu().numpy(), cidx.shape[0])
            if N.neural_layout(*tables, 0) is not None:  # else no depth_L fits LDS: no plan, the layers run
                plan = N.NativeNeuralPlan(*tables, dev)
    if len(_PLANS) > 8:
        _PLANS.clear()
    _PLANS[key] = (ct, vt, plan)
    return plan


class LDPCNeuralDecoder(nn.Module):
    """Neural min-sum decoder with channel and residual weights (see module docstring)."""

    def __init__(self, num_nodes, num_iterations=5, depth_L=2):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_iterations = num_iterations
        self.depth_L = depth_L
        if num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        self.residual_layers = nn.ModuleList([ResidualLayer(num_nodes, depth_L)
                                              for _ in range(num_iterations - 1)])
        self.output_layer = OutputLayer()
        self.use_fused = True  # False: always the layer path (LDPC_NEURAL_FUSED=0 does the same)
        self._fused_w = (None, None, None)  # key, stacked w_ch (I - 1, E), stacked w_res (I - 1, depth_L)

    def _fused_weights(self, dev):
        """The residual layers' weights stacked for ldpc_neural_forward, rebuilt when a parameter's
        storage or version changes (an optimizer step, load_state_dict, an in-place edit)."""
        if not len(self.residual_layers):
            return None, None
        params = [p for res in self.residual_layers for p in (res.w_ch, res.w_res)]
        key = (str(dev),) + tuple((p.data_ptr(), p._version) for p in params)
        if key != self._fused_w[0]:
            stack = lambda ws: torch.stack([w.detach().to(dev, torch.float32) for w in ws]).contiguous()
            self._fused_w = (key, stack([res.w_ch for res in self.residual_layers]),
                             stack([res.w_res for res in self.residual_layers]))
        return self._fused_w[1], self._fused_w[2]

    def _fused(self, llr, check_index_tensor, var_index_tensor, cidx, vidx, want_app):
        """soft (or app, for the output layer's loss) from the fused kernel, or None when this call
        has to run the layers."""
        if not self.use_fused or os.environ.get("LDPC_NEURAL_FUSED", "1") == "0":
            return None
        if torch.is_grad_enabled() and (llr.requires_grad or any(p.requires_grad for p in self.parameters())):
            return None
        if not llr.shape[0]:
            return None
        plan = _fused_plan(check_index_tensor, var_index_tensor, cidx, vidx, self.num_nodes, llr.device)
        if plan is None or plan.layout(self.depth_L) is None:
            return None
        w_ch, w_res = self._fused_weights(llr.device)
        out = torch.empty_like(llr)
        plan.forward(self.num_iterations, self.depth_L, w_ch, w_res, llr,
                     app=out if want_app else None, soft=None if want_app else out)
        return out

    def forward(self, llrs, check_index_tensor, var_index_tensor, ground_truth=None):
        home = llrs.device
        dev = N.device_of(llrs)
        llr = llrs.to(dev, torch.float32).contiguous()
        B, n = llr.shape
        x0_idx, app_idx = _structure(torch.as_tensor(var_index_tensor), n, dev)
        E = x0_idx.shape[1]
        if E != self.num_nodes:
            raise RuntimeError(f"index tensors describe {E} LLR indices, decoder built for {self.num_nodes}")
        cidx = _check_index(check_index_tensor, E, dev)
        vidx = _check_index(var_index_tensor, E, dev, compact=True)
        gt = None if ground_truth is None else ground_truth.to(dev, torch.float32)
        fused = self._fused(llr, check_index_tensor, var_index_tensor, cidx, vidx, want_app=gt is not None)
        if fused is not None:
            if gt is None:
                return fused.to(home), None
            soft, loss = self.output_layer(-fused, -llr, gt)
            return soft.to(home), loss.to(home)
        x0 = gather_sum(llr, x0_idx)
        v, prevs = x0, []
        for res in self.residual_layers:
            c = check_minsum(v, cidx)
            v = res(x0, gather_sum(c, vidx), prevs)
            prevs = [v] + prevs[:max(self.depth_L - 1, 0)]
        app = gather_sum(check_minsum(v, cidx), app_idx)
        soft, loss = self.output_layer(-app, -llr, gt)
        if loss is None:
            return soft.to(home), None
        return soft.to(home), loss.to(home)

    @torch.no_grad()
    def decode(self, llrs, check_index_tensor, var_index_tensor):
        soft, _ = self.forward(llrs, check_index_tensor, var_index_tensor)
        return (soft > 0.5).float()


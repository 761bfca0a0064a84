"""The fused neural min-sum inference kernel (csrc/neural_ms.hip, ldpc_neural_forward) on the GPU.

Every comparison is bitwise (`_same`: NaN exactly where the other side has NaN, every other word equal
as an integer, so the sign of a zero counts too):
  - LDPCNeuralDecoder.forward with use_fused=True against use_fused=False (soft; with ground_truth
    under no_grad also the loss),
  - app from ldpc_neural_forward against the layer path's gather_sum(check_minsum(v), app_idx), and
    against tests/neural_ref.py (the definition in numpy float32) on every finite frame.
The plan for the direct calls is built from H by neural_ref.groups_from_H, not by the package's group
detection, so the two descriptions check each other.

Shapes are the smallest at which each thing can go wrong: the 3x4 example H (E = 7, a degree-1
variable, rows of unequal degree), a ragged 13-variable H (odd N and E, a degree-1 check: unaligned
rows and the padding cap), BG2 Z = 4 (several frames per workgroup, more work items than threads),
BG2 Z = 32 once (one frame per workgroup); iterations 1 / 2 / 5 with depth_L 0 / 1 / 3 (3 >= iterations - 1:
the ring never fills; 1 < 4: it wraps); B = 1, F + 1 and 3 F - 1 (a partial last workgroup); LLR rows that
are only 4-byte aligned."""
import pytest
import torch

from conftest import code_path

from neural_ref import groups_from_H, neural_ref

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import LDPCNeuralDecoder
from ldpc_neural_decoder.models.decoder import _structure
from ldpc_neural_decoder.models.layers import _check_index, check_minsum, gather_sum
from ldpc_neural_decoder.utils import create_LLR_mapping, expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu

EXAMPLE_ROWS = [[0, 1], [1, 2, 3], [0, 3]]
RAGGED_ROWS = [[0], [0, 1, 2, 3, 4], [2, 5, 6], [1, 6, 7, 8, 9, 10, 11], [3, 9, 12], [0, 4, 5, 7, 8, 10, 11, 12]]
_GRAPHS = {}


def _graph(which):
    """(H, cidx, vidx, (cptr, cmem, vptr, K)), built once per graph and shared."""
    if which not in _GRAPHS:
        if which in ("example", "ragged"):
            rows = EXAMPLE_ROWS if which == "example" else RAGGED_ROWS
            H = torch.zeros(len(rows), 1 + max(max(r) for r in rows))
            for i, r in enumerate(rows):
                H[i, r] = 1.0
        else:
            H = expand_base_matrix(load_base_matrix(code_path(which)), which)
        _, cidx, vidx, _ = create_LLR_mapping(H.T)
        _GRAPHS[which] = (H, cidx, vidx, groups_from_H(H.numpy()))
    return _GRAPHS[which]


def _decoder(E, iters, depth, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    dec = LDPCNeuralDecoder(E, num_iterations=iters, depth_L=depth)
    with torch.no_grad():
        for res in dec.residual_layers:
            res.w_ch.copy_(torch.rand(E, generator=g) + 0.5)
            res.w_res.copy_(torch.randn(depth, generator=g) * 0.3)
        if iters > 1:
            dec.residual_layers[0].w_ch[2] = 0.0      # a channel weight of exactly 0
    return dec.to(dev)


def _llrs(B, n, dev, seed=1):
    """(B, n) LLRs with exact zeros and a -0.0, as a view whose rows are only 4-byte aligned."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n, generator=g) * 3
    x[0, :2] = 0.0
    x[0, 2] = -0.0
    x[B - 1, n - 1] = 0.0
    flat = torch.empty(B * n + 1, device=dev)
    view = flat[1:].view(B, n)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb]))


@torch.no_grad()
def _layer_app(dec, llr, cidx_t, vidx_t):
    """The layer path of LDPCNeuralDecoder.forward up to its pre-sigmoid sum."""
    dev = llr.device
    x0_idx, app_idx = _structure(vidx_t, llr.shape[1], dev)
    E = x0_idx.shape[1]
    cidx, vidx = _check_index(cidx_t, E, dev), _check_index(vidx_t, E, dev, compact=True)
    x0 = gather_sum(llr, x0_idx)
    v, prevs = x0, []
    for res in dec.residual_layers:
        v = res(x0, gather_sum(check_minsum(v, cidx), vidx), prevs)
        prevs = [v] + prevs[:max(dec.depth_L - 1, 0)]
    return gather_sum(check_minsum(v, cidx), app_idx)


def _weights(dec):
    if not len(dec.residual_layers):
        return None, None
    return (torch.stack([r.w_ch.detach() for r in dec.residual_layers]).contiguous(),
            torch.stack([r.w_res.detach() for r in dec.residual_layers]).contiguous())


def _direct_app(plan, dec, llr):
    w_ch, w_res = _weights(dec)
    app = torch.full_like(llr, 7.0)
    plan.forward(dec.num_iterations, dec.depth_L, w_ch, w_res, llr, app=app)
    return app


def _ref_app(dec, llr, groups):
    w_ch, w_res = _weights(dec)
    return neural_ref(llr.cpu().numpy(), *groups, dec.num_iterations, dec.depth_L,
                      None if w_ch is None else w_ch.cpu().numpy(), None if w_res is None else w_res.cpu().numpy())


def _both(dec, llr, cidx, vidx, gt=None):
    """(soft, loss) with the fused kernel and with the layers, under no_grad."""
    out = []
    with torch.no_grad():
        for fused in (True, False):
            dec.use_fused = fused
            out.append(dec(llr, cidx, vidx, gt))
    dec.use_fused = True
    return out


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the launches of the fused kernel through the plan wrapper."""
    calls = []
    real = N.NativeNeuralPlan.forward

    def spy(self, *a, **k):
        calls.append(a[0])
        return real(self, *a, **k)

    monkeypatch.setattr(N.NativeNeuralPlan, "forward", spy)
    return calls


@pytest.mark.parametrize("depth", [0, 1, 3])
@pytest.mark.parametrize("iters", [1, 2, 5])
@pytest.mark.parametrize("which", ["example", "ragged", 4])
def test_fused_equals_layers_and_definition(cuda, fused_calls, which, iters, depth):
    H, cidx, vidx, groups = _graph(which)
    n, E = H.shape[1], cidx.shape[0]
    dec = _decoder(E, iters, depth, cuda)
    plan = N.NativeNeuralPlan(*groups, cuda)
    F, threads, lds = plan.layout(depth)
    assert F >= 1 and lds <= 160 * 1024
    for B in sorted({1, F + 1, 3 * F - 1}):
        llr = _llrs(B, n, cuda, seed=B)
        del fused_calls[:]
        (soft_f, none_f), (soft_l, none_l) = _both(dec, llr, cidx, vidx)
        assert fused_calls == [iters] and none_f is None and none_l is None
        assert _same(soft_f, soft_l), (which, iters, depth, B)
        app_l = _layer_app(dec, llr, cidx, vidx)
        app_f = _direct_app(plan, dec, llr)
        assert _same(app_f, app_l), (which, iters, depth, B)
        assert _same(app_f, torch.from_numpy(_ref_app(dec, llr, groups))), (which, iters, depth, B)
        # the trainer's validation: ground truth under no_grad -> the kernel's app, the layers' loss
        gt = (torch.rand(B, n, generator=torch.Generator().manual_seed(B)) < 0.5).float().to(cuda)
        (soft_f, loss_f), (soft_l, loss_l) = _both(dec, llr, cidx, vidx, gt)
        assert _same(soft_f, soft_l) and _same(loss_f, loss_l) and loss_f.shape == (B,)


def test_fused_bg2_z32(cuda, fused_calls):
    """One frame per workgroup, 1024 threads, 6 edges per thread; the ring of 3 rows never fills."""
    H, cidx, vidx, groups = _graph(32)
    dec = _decoder(cidx.shape[0], 4, 3, cuda)
    plan = N.NativeNeuralPlan(*groups, cuda)
    assert plan.layout(3)[0] == 1 and plan.layout(2)[0] == 1
    llr = _llrs(5, H.shape[1], cuda)
    (soft_f, _), (soft_l, _) = _both(dec, llr, cidx, vidx)
    assert fused_calls == [4] and _same(soft_f, soft_l)
    app_f = _direct_app(plan, dec, llr)
    assert _same(app_f, _layer_app(dec, llr, cidx, vidx))
    assert _same(app_f, torch.from_numpy(_ref_app(dec, llr, groups)))
    soft = torch.full_like(llr, 7.0)                 # both outputs in one launch
    app2 = torch.full_like(llr, 7.0)
    plan.forward(4, 3, *_weights(dec), llr, app=app2, soft=soft)
    assert _same(app2, app_f) and _same(soft, soft_l)


@pytest.mark.parametrize("which", ["ragged", 4])
def test_non_finite_frames_stay_in_their_frame(cuda, which):
    H, cidx, vidx, groups = _graph(which)
    n = H.shape[1]
    dec = _decoder(cidx.shape[0], 3, 2, cuda)
    plan = N.NativeNeuralPlan(*groups, cuda)
    B = plan.layout(2)[0] + 3
    clean = _llrs(B, n, cuda)
    dirty = clean.clone()
    dirty[1, 0], dirty[1, n - 1] = float("inf"), float("-inf")
    dirty[B - 2, n // 2] = float("nan")
    (soft_f, _), (soft_l, _) = _both(dec, dirty, cidx, vidx)
    assert _same(soft_f, soft_l)
    assert bool(torch.isnan(soft_f[B - 2]).any())
    app_f, app_l = _direct_app(plan, dec, dirty), _layer_app(dec, dirty, cidx, vidx)
    assert _same(app_f, app_l)
    # the definition agrees on the frames that stay finite, and those frames do not see the others
    ref = torch.from_numpy(_ref_app(dec, dirty, groups))
    keep = [b for b in range(B) if b not in (1, B - 2)]
    assert bool(torch.isfinite(app_f[keep]).all()) and _same(app_f[keep], ref[keep])
    (soft_clean, _), _ = _both(dec, clean, cidx, vidx)
    assert _same(soft_f[keep], soft_clean[keep])
    assert _same(app_f[keep], _direct_app(plan, dec, clean)[keep])


def test_entry_point_argument_rules(cuda):
    H, cidx, vidx, groups = _graph("example")
    plan = N.NativeNeuralPlan(*groups, cuda)
    llr = _llrs(2, H.shape[1], cuda)
    out = torch.empty_like(llr)
    lib, s = N.lib(), N.stream_ptr(cuda)
    # iterations = 1: no variable layer, both weight pointers may be NULL
    assert lib.ldpc_neural_forward(plan.handle, 1, 2, None, None, N.ptr(llr), 2, N.ptr(out), None, s) == 0
    dec = _decoder(cidx.shape[0], 1, 2, cuda)
    assert _same(out, _layer_app(dec, llr, cidx, vidx))
    # B = 0 succeeds and launches nothing; no output, no plan, iterations < 1, missing weights are refused
    assert lib.ldpc_neural_forward(plan.handle, 1, 2, None, None, None, 0, N.ptr(out), None, s) == 0
    assert lib.ldpc_neural_forward(plan.handle, 1, 2, None, None, N.ptr(llr), 2, None, None, s) == N.LDPC_EINVAL
    assert lib.ldpc_neural_forward(None, 1, 2, None, None, N.ptr(llr), 2, N.ptr(out), None, s) == N.LDPC_EINVAL
    assert lib.ldpc_neural_forward(plan.handle, 0, 2, None, None, N.ptr(llr), 2, N.ptr(out), None, s) == N.LDPC_EINVAL
    assert lib.ldpc_neural_forward(plan.handle, 2, 2, None, None, N.ptr(llr), 2, N.ptr(out), None, s) == N.LDPC_EINVAL
    rc = lib.ldpc_neural_forward(plan.handle, 1, 9, None, None, N.ptr(llr), 2, N.ptr(out), None, s)
    assert rc == N.LDPC_EUNSUPPORTED
    torch.cuda.synchronize()
    # the plan validates what it uploads
    cptr, cmem, vptr, K = groups
    bad = cmem.copy()
    bad[0] = bad[1]
    with pytest.raises(N.NativeError):
        N.NativeNeuralPlan(cptr, bad, vptr, K, cuda)


def test_training_forward_stays_on_the_layers(cuda, fused_calls):
    H, cidx, vidx, _ = _graph(4)
    n = H.shape[1]
    llr = _llrs(6, n, cuda)
    gt = (torch.rand(6, n, generator=torch.Generator().manual_seed(3)) < 0.5).float().to(cuda)
    grads = []
    for fused in (True, False):
        dec = _decoder(cidx.shape[0], 3, 2, cuda)
        dec.use_fused = fused
        with torch.enable_grad():
            soft, loss = dec(llr, cidx, vidx, gt)
            loss.mean().backward()
        grads.append([p.grad.clone() for p in dec.parameters()])
    assert fused_calls == []
    assert len(grads[0]) == 4 and all(g is not None for g in grads[0])
    # the same kernels both times; their batch reductions are float atomics, so two runs agree to
    # rounding, not bit for bit: the bar tests/test_harness_gpu.py states for these gradients
    for a, b in zip(*grads):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-6
    # frozen parameters and an LLR without grad: nothing can ask for a gradient, so the kernel runs
    dec = _decoder(cidx.shape[0], 3, 2, cuda).requires_grad_(False)
    with torch.enable_grad():
        dec(llr, cidx, vidx)
        assert fused_calls == [3]
        dec(llr.clone().requires_grad_(True), cidx, vidx)
    assert fused_calls == [3]


def test_non_group_index_runs_the_layers(cuda, fused_calls):
    H, cidx, vidx, _ = _graph(4)
    dec = _decoder(cidx.shape[0], 3, 2, cuda)
    llr = _llrs(5, H.shape[1], cuda)
    row = int((vidx >= 0).sum(1).argmax())            # a row with at least two real entries
    assert int((vidx[row] >= 0).sum()) >= 2
    perm = vidx.clone()
    perm[row, 0], perm[row, 1] = vidx[row, 1], vidx[row, 0]   # the same sets, one row out of order
    (soft_f, _), (soft_l, _) = _both(dec, llr, cidx, perm)
    assert fused_calls == [] and _same(soft_f, soft_l)
    _both(dec, llr, cidx, vidx)                       # the tensor it was made from does take the kernel
    assert fused_calls == [3]


def test_frame_too_large_for_lds_runs_the_layers(cuda, fused_calls):
    """E = 12000 on 6000 degree-2 variables: even depth_L = 0 needs (6000 + 2 * 12000) * 4 bytes of rows
    beside 66 KB of tables, so there is no plan and forward runs the layers without a word."""
    j = torch.arange(6000)
    H = torch.zeros(3000, 6000)
    H[j // 2, j] = 1.0
    H[(j // 2 + 1 + (j % 2) * 7) % 3000, j] = 1.0
    _, cidx, vidx, _ = create_LLR_mapping(H.T)
    assert cidx.shape == (12000, 3) and vidx.shape == (12000, 1)
    assert N.neural_layout(*groups_from_H(H.numpy()), 0) is None
    dec = _decoder(12000, 2, 2, cuda)
    llr = _llrs(2, 6000, cuda)
    (soft_f, _), (soft_l, _) = _both(dec, llr, cidx, vidx)
    assert fused_calls == [] and _same(soft_f, soft_l)
    dec9 = _decoder(_graph("ragged")[1].shape[0], 2, 9, cuda)     # depth_L > 8: refused by the layout
    H2, c2, v2, _ = _graph("ragged")
    assert dec9(_llrs(2, H2.shape[1], cuda), c2, v2)[0].shape == (2, H2.shape[1]) and fused_calls == []


def test_switches_and_weight_cache(cuda, fused_calls, monkeypatch):
    H, cidx, vidx, _ = _graph("ragged")
    dec = _decoder(cidx.shape[0], 3, 2, cuda)
    llr = _llrs(4, H.shape[1], cuda)
    monkeypatch.setenv("LDPC_NEURAL_FUSED", "0")
    hard_env = dec.decode(llr, cidx, vidx)
    assert fused_calls == []
    monkeypatch.delenv("LDPC_NEURAL_FUSED")
    hard = dec.decode(llr, cidx, vidx)
    assert fused_calls == [3] and _same(hard, hard_env)
    soft_before = _both(dec, llr, cidx, vidx)[0][0]
    with torch.no_grad():                             # an optimizer step is an in-place update
        dec.residual_layers[0].w_ch.mul_(-0.5)
        dec.residual_layers[1].w_res.add_(0.25)
    (soft_f, _), (soft_l, _) = _both(dec, llr, cidx, vidx)
    assert _same(soft_f, soft_l) and not _same(soft_f, soft_before)
    dec.use_fused = False
    assert _same(dec.decode(llr, cidx, vidx), (soft_l > 0.5).float())

"""The workspace queries against the documented layouts (GPU: a graph lives on a device).

ldpc_flood_workspace_size, ldpc_layered_half_workspace_size and ldpc_custom_minsum_workspace_size must equal
the sum of the buffers their carves take, in the order the comments of csrc/flood.hip (FloodWs),
csrc/flood_stream.hpp (StreamWs), csrc/flood_layered_stream_half.hip (HalfWs) and csrc/flood_stream.hip
(CustomWs) give, each rounded up to 256 bytes.  The restatement below shares nothing with the library.

Shapes: BG2 Z = 4 (LDS-resident: counter rows, redo list and, under the batch-global stop, the EsWs arrays)
and BG2 Z = 12 (streaming); B in {1, 5, 128, 129} (the half layout's row stride rounds to 128 frames and its
counter rows come one per 64 frames); max_iter in {1, 33} (the validity words per frame cross 32 iterations).
"""
import pytest

from conftest import code_path

from ldpc_neural_decoder import _native as N
from ldpc_neural_decoder.models import MinSumScaledDecoder
from ldpc_neural_decoder.utils import expand_base_matrix, load_base_matrix

pytestmark = pytest.mark.gpu
PART_ROW = 8  # uint32 per counter row
BS = [1, 5, 128, 129]
ITERS = [1, 33]


def total(sizes):
    return sum((n + 255) // 256 * 256 for n in sizes)


def cdiv(a, b):
    return (a + b - 1) // b


def flood_lds(g, B, max_iter, es):
    fg, nb = 64 // g.Z, g.N // g.Z
    nwg = cdiv(B, fg)
    sizes = [nwg * PART_ROW * 4, (nwg + 1) * 4]  # counter rows, redo list
    if es == N.LDPC_ES_BATCH:
        nvw = cdiv(max_iter, 32)
        sizes += [nwg * max_iter * nb * 8,  # decision words of every iteration
                  B * nvw * 4,              # validity words per frame
                  64 * 4,                   # their AND over the batch
                  nwg * nb * 8,             # candidate words
                  nwg * 4,                  # t_wg
                  64, 64]                   # ctl, staged
    return total(sizes)


def flood_stream(g, B, max_iter):
    return total([g.E * B * 4, g.N * B * 4, g.N * B, B, B * 4, 64, max_iter * 4, cdiv(B, 64) * PART_ROW * 4])


def layered_half(g, B):
    bs = cdiv(B, 128) * 128
    return total([g.E * bs * 2, g.N * bs * 2, g.N * B, B, B * 4, cdiv(B, 64) * PART_ROW * 4])


def custom(g, B):
    return total([g.E * B * 4, g.N * B * 4, g.N * B * 4])


@pytest.fixture(scope="module")
def graphs(cuda):
    base = load_base_matrix(code_path(32))
    out = {z: MinSumScaledDecoder(expand_base_matrix(base, z), 1).graph(cuda) for z in (4, 12)}
    assert out[4].Z == 4 and out[12].Z == 1  # 12 does not divide 64: no lifting detected, streaming
    assert (out[4].N, out[4].E, out[12].N, out[12].E) == (208, 788, 624, 2364)
    return out


@pytest.mark.parametrize("es", [N.LDPC_ES_OFF, N.LDPC_ES_BATCH, N.LDPC_ES_FRAME])
def test_flood_workspace_size(graphs, monkeypatch, es):
    monkeypatch.delenv("LDPC_FLOOD_STREAM", raising=False)
    lib = N.lib()
    for B in BS:
        for it in ITERS:
            assert lib.ldpc_flood_workspace_size(graphs[4].handle, B, it, es) == flood_lds(graphs[4], B, it, es), (B, it)
            assert lib.ldpc_flood_workspace_size(graphs[12].handle, B, it, es) == flood_stream(graphs[12], B, it), (B, it)
    monkeypatch.setenv("LDPC_FLOOD_STREAM", "1")  # the LDS-resident graph on the streaming kernels
    for B in BS:
        assert lib.ldpc_flood_workspace_size(graphs[4].handle, B, 33, es) == flood_stream(graphs[4], B, 33), B
    for g in graphs.values():
        assert lib.ldpc_flood_workspace_size(g.handle, 0, 5, es) == 0
        assert lib.ldpc_flood_workspace_size(g.handle, 5, 0, es) == 0


@pytest.mark.parametrize("z", [4, 12])
def test_layered_half_workspace_size(graphs, z):
    lib, g = N.lib(), graphs[z]
    for B in BS:
        for it in ITERS:
            for es in (N.LDPC_ES_OFF, N.LDPC_ES_FRAME):
                assert lib.ldpc_layered_half_workspace_size(g.handle, B, it, es) == layered_half(g, B), (B, it, es)
    assert lib.ldpc_layered_half_workspace_size(g.handle, 0, 5, 0) == 0
    assert lib.ldpc_layered_half_workspace_size(g.handle, 5, 0, 0) == 0


@pytest.mark.parametrize("z", [4, 12])
def test_custom_minsum_workspace_size(graphs, z):
    lib, g = N.lib(), graphs[z]
    for B in BS:
        assert lib.ldpc_custom_minsum_workspace_size(g.handle, B) == custom(g, B), B
    assert lib.ldpc_custom_minsum_workspace_size(g.handle, 0) == 0

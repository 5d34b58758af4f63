"""The fused GAT operator (fused_gat_dropout_func) in f16 / bf16 at its ORDINARY launches, forward and backward, against the
float64 oracle on the rounded inputs with the same dropout mask (oracle.gat_fwd / gat_bwd, as tests/test_gat_dropout.py).

Cases, references and bounds: tests/_gat_halfprec.py (shared with the plan launches of tests/test_halfprec_plan_gpu.py).

What the shapes reach for 2-byte elements at their own widths (PAD_FEATURES off; gat_fwd_geometry / gat_bwd_geometry,
csrc/gat_op.h; (vec, lanes per row, column tiles)):
    shape      forward        backward
    (8, 8)     (8, 8, 1)      one group (8, 8)
    (1, 41)    (1, 64, 1)     one group (1, 64)
    (3, 5)     (1, 16, 1)     tiled (1, 16, 1)
    (6, 12)    (4, 32, 1)     tiled (4, 64, 1)
    (2, 64)    (8, 16, 1)     one group (8, 16)
    (8, 64)    (8, 64, 1)     one group (8, 64)
    (4, 128)   (8, 64, 1)     one group (8, 64)
    (16, 64)   (8, 64, 2)     tiled (8, 64, 2)
    (3, 24)    (8, 16, 1)     tiled (8, 16, 1)
    (1, 300)   (4, 64, 2)     tiled (4, 64, 2)
    (3, 12)    (4, 16, 1)     tiled (4, 16, 1)
    (3, 6)     (2, 16, 1)     tiled (2, 16, 1)
    (6, 6)     (2, 32, 1)     tiled (2, 64, 1)
    (3, 7)     (1, 32, 1)     tiled (1, 64, 1)
    (4, 4)     (4, 8, 1)      one group (4, 8)
    (16, 2)    (2, 16, 1)     one group (2, 16)
    (32, 1)    (1, 32, 1)     one group (1, 32)
    (4, 64)    (8, 32, 1)     one group (8, 32)
With PAD_FEATURES on (the default) the operator pads F to whole 16-byte lanes first (fused_gat._padded_width): every width is
then a multiple of 8, forward and one-group backward at vec 8, (3, 24) and (16, 64) tiled at vec 8.
So every tiled backward instantiation for 2-byte elements (vec 1, 2, 4, 8 x 16 or 64 lanes) is launched, and every vector
width and every group size of the forward and of the one-group backward at least once.  NOT launched in 16-bit by this file:
forward (1, 8), (2, 8), (2, 64); one-group backward (1, 8), (1, 16), (2, 8), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64)
(as (vec, lanes): these need F = 1, 2 or 4 with up to 64 heads, or one head whose width is no multiple of 8)."""
import pytest
import torch

from _gat_halfprec import check
from cogdl_amd import _lib, xcdplan

pytestmark = pytest.mark.gpu
SHAPES = [(8, 8), (1, 41), (3, 5), (6, 12), (2, 64), (8, 64), (4, 128), (16, 64), (3, 24), (1, 300),
          (3, 12), (3, 6), (6, 6), (3, 7), (4, 4), (16, 2), (32, 1), (4, 64)]  # (second line: the instantiations the first leaves out)
HUB_SHAPES = [(8, 8), (1, 41), (16, 64), (6, 12), (3, 12), (3, 6)]


@pytest.fixture(autouse=True)
def ordinary_launch(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")  # (the default: these graphs are far below any plan's size)


@pytest.fixture(params=[0, 1, 2], ids=["auto", "edgewise-softmax", "chunkwise-softmax"])
def gat_kernel(request):
    _lib.hip().cogdl_hip_set_tuning(5, request.param)
    yield request.param
    _lib.hip().cogdl_hip_set_tuning(5, 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("pad", [True, False], ids=["padded-rows", "raw-width"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,f", SHAPES)
def test_fused_gat_16bit_within_half_an_ulp(gat_kernel, dtype, pad, p, h, f):
    check("random", h, f, dtype, p, pad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("pad", [True, False], ids=["padded-rows", "raw-width"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,f", HUB_SHAPES)
def test_fused_gat_16bit_hub_rows_within_half_an_ulp(gat_kernel, dtype, pad, p, h, f):
    """Rows and columns of thousands of edges: the long-row path of the forward and of both backward passes."""
    check("hubs", h, f, dtype, p, pad)

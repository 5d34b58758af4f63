"""gen_aggregate without a GPU: the CPU route against the float64 oracle under the rule of tests/_gen_cases.py (output and the
three gradients), the oracle itself against the definition written row by row, a one-edge row returns its message bit for bit and an empty row 0, the arguments are checked, the entry points
are declared in the header and resolvable through the ctypes table, and install() takes the flag."""
import inspect
import os
import re
import warnings

import pytest
import torch

import _gen_cases as C
from cogdl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cogdl_hip_gen_aggr_fwd_workspace_bytes", "cogdl_hip_gen_aggr_fwd", "cogdl_hip_gen_aggr_bwd_workspace_bytes",
           "cogdl_hip_gen_aggr_bwd")


def _ours(aggr):
    from cogdl_amd.operators import gen_aggregate

    row, col = C.graph()
    return lambda x, t, b: gen_aggregate(x, row, col, t, aggr, b, C.EPS, num_nodes=C.N)


@pytest.mark.parametrize("width", C.WIDTHS)
@pytest.mark.parametrize("with_eterm", [False, True])
def test_cpu_route_against_the_oracle(width, with_eterm):
    x, eterm, G = C.inputs(width, with_eterm)
    for aggr, beta, learn in (("softmax", 0.75, True), ("softmax", None, False), ("sum", None, False), ("mean", None, False)):
        oracle, ref32 = C.reference(width, with_eterm, aggr, beta, learn)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the CPU route is quiet
            with C.edge_order():
                got = C.run(_ours(aggr), x, eterm, beta, G, learn)
        assert got.keys() == oracle.keys() and ("g_beta" in got) == learn and ("g_eterm" in got) == with_eterm
        C.check("cpu F=%d eterm=%d %s" % (width, with_eterm, aggr), got, oracle, ref32)


@pytest.mark.parametrize("aggr", ["softmax", "sum", "mean"])
def test_oracle_is_the_row_by_row_definition(aggr):
    """The oracle shares its vectorised form with the operator's CPU route, so it is itself held to the definition written as a
    loop over the destinations with torch.softmax, in float64 (values and the three gradients through autograd)."""
    row, col = C.graph()
    x, eterm, G = C.inputs(7, True)
    beta = 0.75 if aggr == "softmax" else None
    oracle, _ = C.reference(7, True, aggr, beta, aggr == "softmax")

    def by_rows(xa, ta, ba):
        m = torch.relu(xa[col] + ta) + C.EPS
        rows = []
        for v in range(C.N):
            mv = m[row == v]
            if mv.shape[0] == 0:
                rows.append(torch.zeros(7, dtype=m.dtype))
            elif aggr == "softmax":
                rows.append((torch.softmax(ba * mv, dim=0) * mv).sum(0))
            else:
                rows.append(mv.sum(0) / (mv.shape[0] if aggr == "mean" else 1))
        return torch.stack(rows)

    want = C.run(by_rows, x, eterm, beta, G, aggr == "softmax", dtype=torch.float64)
    assert want.keys() == oracle.keys()
    for name in want:
        assert torch.allclose(oracle[name], want[name], rtol=1e-11, atol=1e-12), (name, float((oracle[name] - want[name]).abs().max()))


def test_one_edge_row_is_its_message_and_an_empty_row_is_zero():
    from cogdl_amd.operators import gen_aggregate

    row, col = C.graph()
    x, eterm, _ = C.inputs(7, True)
    one = int((row == 1).nonzero()[0])
    for aggr, beta in (("softmax", 3.0), ("softmax", None), ("sum", None), ("mean", None)):
        out = gen_aggregate(x, row, col, eterm, aggr, beta, C.EPS, num_nodes=C.N)
        m = torch.relu(x[col[one]] + eterm[one]) + C.EPS
        assert out[1].numpy().tobytes() == m.numpy().tobytes(), aggr
        assert out[0].numpy().tobytes() == bytes(4 * 7) and not out[260:].any(), aggr
    assert gen_aggregate(x, row, col, num_nodes=C.N + 5).shape == (C.N + 5, 7)


def test_arguments_are_checked():
    from cogdl_amd.operators import gen_aggregate

    x = torch.randn(5, 4)
    idx = torch.tensor([0, 1, 2])
    with pytest.raises(ValueError):
        gen_aggregate(x, idx, idx, aggr="powermean")
    with pytest.raises(ValueError):
        gen_aggregate(x, idx, idx[:2])
    with pytest.raises(ValueError):
        gen_aggregate(x, idx, idx, eterm=torch.randn(3, 5))
    with pytest.raises(ValueError):
        gen_aggregate(x, idx, idx, eterm=torch.randn(2, 4))
    with pytest.raises(ValueError):
        gen_aggregate(x, idx, idx, beta=torch.ones(2))
    with pytest.raises(ValueError):
        gen_aggregate(x[0], idx, idx)
    empty = torch.zeros(0, dtype=torch.int64)
    out = gen_aggregate(x, empty, empty)
    assert out.shape == (5, 4) and not out.any()


def test_symbols_are_declared_and_resolvable():
    text = open(os.path.join(ROOT, "include", "cogdl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.hip()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.HIP_SIGNATURES and callable(getattr(lib, name)), name
    assert lib.cogdl_hip_abi_version() == 9
    # pure host queries: the engine's workspace, zero without edges; the forward's piece records hold four floats per column
    assert lib.cogdl_hip_gen_aggr_fwd_workspace_bytes(0, 128) == 0 and lib.cogdl_hip_gen_aggr_bwd_workspace_bytes(4000, 128) > 0
    assert lib.cogdl_hip_gen_aggr_fwd_workspace_bytes(4000, 128) > lib.cogdl_hip_gen_aggr_bwd_workspace_bytes(4000, 128)
    # argument validation happens before anything is launched (EINVAL = 1)
    fwd = lambda mode, m, k, nnz: lib.cogdl_hip_gen_aggr_fwd(None, None, None, None, None, mode, None, 1.0, 1e-7, None, None,
                                                             None, m, k, nnz, None, 0, None)
    bwd = lambda mode, m, k, nnz: lib.cogdl_hip_gen_aggr_bwd(None, None, None, None, None, None, None, None, mode, None, 1.0,
                                                             1e-7, None, None, m, k, nnz, None, 0, None)
    for call in (fwd, bwd):
        assert call(0, 4, 4, 0) == 1      # null pointers
        assert call(0, -1, 4, 0) == 1     # a negative size
        assert call(3, 4, 4, 0) == 1      # an unknown mode
        assert call(0, 0, 4, 0) == 0      # no rows: nothing to do
        assert call(0, 4, 2 ** 31, 0) == 6  # ERANGE: a width the geometry cannot tile


def test_install_takes_the_flag():
    import cogdl_amd
    from cogdl_amd import genconv_compat

    sig = inspect.signature(cogdl_amd.install)
    assert "genconv" in sig.parameters and sig.parameters["genconv"].default is False
    assert "genconv=True" in cogdl_amd.install.__doc__
    assert callable(genconv_compat.forward)

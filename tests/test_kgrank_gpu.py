"""All-entity ranking on the GPU: the HIP kernels of rank_all against the float64 oracle of tests/_kgrank_cases.py and, bit for
bit in all three counts, against the host twin -- on the golden cases (tests/golden/kg_rank.npz) and on the smallest shapes
that can break a tile."""
import warnings

import numpy as np
import pytest
import torch

import _kgrank_cases as C
import _offset as O
from cogdl_amd.operators import rank_all
from cogdl_amd.operators.kgrank import slice_entities
from cogdl_amd.operators.ops import _ROUTE_NOTED, TorchRouteWarning

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS, MS = (1, 5, 63, 64, 65, 257, 1031), (1, 67, 300)
DS = {"dot": (1, 2, 3, 24, 130), "l1": (1, 2, 3, 24, 130), "cl2": (2, 24, 130)}  # 130: wider than one k slab of LDS
GAMMA = 3.0


def kernel_counts(q, table, target, kind, gamma=GAMMA, ptr=None, idx=None):
    """rank_all on the GPU on the kernels' route (a TorchRouteWarning is an error), as a CPU tensor."""
    to = lambda t: None if t is None else t.to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = rank_all(to(q), to(table), to(target), kind, gamma, to(ptr), to(idx))
    assert out.is_cuda and out.dtype == torch.int32
    return out.cpu()


def make_case(kind, m, n, d, exact, seed):
    """Tables with duplicated rows (a partner in the first and in the last slice), targets at 0, N - 1 and on either side of
    every slice boundary of the launch, and per query one of four filter lists: empty, every entity, the target alone, random
    ids each given twice."""
    gen = torch.Generator().manual_seed(seed)
    if exact:
        table = torch.randint(-8, 9, (n, d), generator=gen).float() / 4
        q = torch.randint(-8, 9, (m, d), generator=gen).float() / 4
    else:
        table, q = torch.randn(n, d, generator=gen) * 0.5, torch.randn(m, d, generator=gen)
    table[n - 1] = table[0]
    table[n // 2] = table[0]
    step = slice_entities(m, n, d, kind)
    assert step >= 1
    special = [0, n - 1, n // 2]
    for b in range(step, n, step):
        special += [b - 1, b]
    target = torch.randint(0, n, (m,), generator=gen)
    k = min(m, len(special))
    target[:k] = torch.tensor(special[:k])
    if m < len(special):  # (a single query cannot visit every boundary: the last one at least)
        target[-1] = special[-1]
    lists = []
    for i in range(m):
        which = i % 4
        if which == 0:
            lists.append(torch.zeros(0, dtype=torch.int64))
        elif which == 1:
            lists.append(torch.arange(n))
        elif which == 2:
            lists.append(target[i:i + 1].clone())
        else:
            r = torch.randint(0, n, (5,), generator=gen)
            lists.append(torch.cat([r, r.flip(0)]))
    ptr = torch.zeros(m + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor([len(x) for x in lists]).cumsum(0)
    return q, table, target, ptr, torch.cat(lists), step


def oracle_check(kind, q, table, target, ptr, idx, got, exact, chunk=4096):
    """Against the float64 oracle, in row chunks of the queries."""
    m, n, d = q.shape[0], table.shape[0], q.shape[1]
    left = np.zeros((m, n), dtype=bool)
    if ptr is not None:
        owner = np.repeat(np.arange(m), np.diff(ptr.numpy()))
        left[owner, idx.numpy()] = True
    left[np.arange(m), target.numpy()] = False
    got, tgt, qn, tn = got.numpy().astype(np.int64), target.numpy(), q.numpy(), table.numpy()
    for lo_row in range(0, m, chunk):
        rows = slice(lo_row, min(m, lo_row + chunk))
        s64 = C.scores64(kind, qn[rows], tn, GAMMA)
        if exact and kind != "cl2":  # every product and sum exact in float32: the counts are the oracle's
            assert np.array_equal(got[rows], C.counts64(s64, tgt[rows], left[rows])), (kind, m, n, d, lo_row)
            continue
        # otherwise the float32 sum of D (or D / 2) terms, each rounded a few times: (D + 4) eps of the sum of magnitudes
        mag = float((np.abs(s64).max() + abs(GAMMA)) if kind != "dot" else (np.abs(qn[rows].astype(np.float64))
                                                                              @ np.abs(tn.astype(np.float64)).T).max())
        lo, hi = C.bracket64(s64, tgt[rows], left[rows], (d + 4) * C.EPS32 * mag)
        assert (lo <= got[rows, 0]).all() and (got[rows].sum(1) <= hi).all(), (kind, m, n, d, lo_row)


@pytest.mark.parametrize("kind", ["dot", "l1", "cl2"])
@pytest.mark.parametrize("exact", [True, False])
def test_tile_shapes_against_oracle_and_host_twin(kind, exact):
    seed = 0
    ties = 0
    for n in NS:
        for m in MS:
            for d in DS[kind]:
                seed += 1
                q, table, target, ptr, idx, step = make_case(kind, m, n, d, exact, seed)
                for filt in ((None, None), (ptr, idx)):
                    got = kernel_counts(q, table, target, kind, GAMMA, *filt)
                    host = rank_all(q, table, target, kind, GAMMA, *filt)
                    assert torch.equal(got, host), (kind, exact, n, m, d, filt[0] is not None,
                                                    torch.nonzero((got != host).any(1)).flatten()[:5].tolist())
                    if m <= 67 or d in (3, 24):  # (every width, the slab-crossing 130 and the zero-padded 1 included)
                        oracle_check(kind, q, table, target, *filt, got, exact)
                    assert int(got.min()) >= 0
                    if filt[0] is None and n >= 5:
                        # rows 0, N // 2 and N - 1 are equal: a target at row 0 has two partners after it (the last one in
                        # the last slice), a target at row N - 1 two before it -- unless the score is NaN
                        for row, col in ((0, 2), (n - 1, 1)):
                            at = torch.nonzero(target == row).flatten()
                            if len(at):
                                assert int(got[at, col].min()) >= 2, (kind, n, m, d, row)
                                ties += 1
    assert ties > 10


@pytest.mark.parametrize("kind", ["dot", "l1", "cl2"])
def test_slices_of_several_entity_tiles(kind):
    """Many queries against few entities: the launch has few slices and a workgroup walks SEVERAL entity tiles (what every real
    evaluation does) -- the accumulators start again per tile while the counters carry on.  Targets and their tie partners sit
    on the tile boundaries inside a slice and on the slice boundary; all three counts bit for bit the host twin's and, the
    data being exact, the float64 oracle's."""
    m, n, d = 65536 - 61, 257, 4 if kind == "cl2" else 3  # 1024 query tiles, the last one ragged: two slices per launch
    tile = 128 if kind == "dot" else 64
    step = slice_entities(m, n, d, kind)
    assert step % tile == 0 and step >= 2 * tile and step < n  # at least two slices, each of several tiles
    gen = torch.Generator().manual_seed(11)
    table = torch.randint(-8, 9, (n, d), generator=gen).float() / 4
    q = torch.randint(-8, 9, (m, d), generator=gen).float() / 4
    special = sorted({0, n - 1} | {b + o for b in range(tile, n, tile) for o in (-1, 0)})
    table[special] = table[0].clone()  # the rows on either side of every tile boundary, the first and the last row: all equal
    target = torch.randint(0, n, (m,), generator=gen)
    target[:4 * len(special)] = torch.tensor(special).repeat(4)
    lens = torch.where(torch.arange(m) % 4 == 3, 6, 0)
    ptr = torch.zeros(m + 1, dtype=torch.int64)
    ptr[1:] = lens.cumsum(0)
    half = torch.randint(0, n, (int(ptr[-1]) // 6, 3), generator=gen)
    idx = torch.cat([half, half.flip(1)], dim=1).flatten()  # every id twice
    for filt in ((None, None), (ptr, idx)):
        got = kernel_counts(q, table, target, kind, GAMMA, *filt)
        host = rank_all(q, table, target, kind, GAMMA, *filt)
        assert torch.equal(got, host), (kind, filt[0] is not None, torch.nonzero((got != host).any(1)).flatten()[:5].tolist())
        oracle_check(kind, q, table, target, *filt, got, True, chunk=8192)
    raw = kernel_counts(q, table, target, kind)
    for i, row in enumerate(special):  # unfiltered: the partners before and after the target, in other tiles and slices
        assert raw[i, 1] >= i and raw[i, 2] >= len(special) - 1 - i, (kind, row, raw[i].tolist())


@pytest.mark.parametrize("model,family", C.CASES)
def test_golden_cases(model, family):
    """The reference's own models and positions: exact tables give the oracle's counts and bracket the recorded positions,
    float tables lie inside the float64 bracket with at most 5 % ambiguous triples and reproduce the reference's MRR within
    the ambiguous triples' share (tests/test_kgrank_cpu.py: check_case)."""
    from test_kgrank_cpu import check_case, run_case

    for mode in C.MODES:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = run_case(model, family, mode, device=DEV)
        check_case(got, model, family, mode)
        assert np.array_equal(got, run_case(model, family, mode))  # the host twin, bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        raw = run_case(model, family, "head-batch", device=DEV, filtered=False)
    check_case(raw, model, family, "head-batch", filtered=False)


@pytest.mark.parametrize("kind", ["dot", "l1", "cl2"])
def test_special_values(kind):
    """+-inf and NaN entries: inf - inf and 0 * inf give NaN scores, which are counted nowhere; the kernels agree with the
    host twin in every count, and the dot case with its hand count."""
    inf, nan = float("inf"), float("nan")
    gen = torch.Generator().manual_seed(5)
    table = torch.randint(-4, 5, (130, 4), generator=gen).float()
    table[3, 0], table[70, 1], table[129, 2], table[64, 3], table[65, 0] = inf, -inf, nan, inf, -inf
    q = torch.randint(-4, 5, (67, 4), generator=gen).float()
    q[5, 0], q[6, 1], q[7, 2] = inf, nan, -inf
    target = torch.randint(0, 130, (67,), generator=gen)
    target[:6] = torch.tensor([3, 70, 129, 64, 65, 0])
    got = kernel_counts(q, table, target, kind)
    assert torch.equal(got, rank_all(q, table, target, kind, GAMMA))
    assert got[2].tolist() == [0, 0, 0] and got[6].tolist() == [0, 0, 0]  # a NaN target score; a NaN query
    if kind == "dot":
        t = torch.tensor([[1.0, 0.0], [inf, 0.0], [-inf, 0.0], [nan, 0.0], [1.0, 0.0], [2.0, 0.0]])
        c = kernel_counts(torch.tensor([[1.0, 0.0]] * 4), t, torch.tensor([0, 1, 3, 4]), "dot")
        assert c.tolist() == [[2, 0, 1], [0, 0, 0], [0, 0, 0], [2, 1, 0]]


@pytest.mark.parametrize("kind", ["dot", "l1", "cl2"])
def test_two_runs_equal_and_operand_offsets(kind):
    q, table, target, ptr, idx, _ = make_case(kind, 300, 1031, 24, False, 77)
    first = kernel_counts(q, table, target, kind, GAMMA, ptr, idx)
    assert torch.equal(first, kernel_counts(q, table, target, kind, GAMMA, ptr, idx))
    for shift in (1, 2, 3):  # operands that start mid-allocation: every input and the int32 index arrays
        qs, _ = O.shifted(q, shift, device=DEV)
        ts, _ = O.shifted(table, shift + 1, device=DEV)
        tg, _ = O.shifted(target.int(), shift, device=DEV)
        ps, _ = O.shifted(ptr.int(), shift, device=DEV)
        xs, _ = O.shifted(idx.int(), shift + 2, device=DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert torch.equal(rank_all(qs, ts, tg, kind, GAMMA, ps, xs).cpu(), first)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(rank_all(O.strided(q.to(DEV)), O.strided(table.to(DEV)), target.to(DEV), kind, GAMMA).cpu(),
                           kernel_counts(q, table, target, kind))


def test_torch_route_says_so_and_refusals():
    from cogdl_amd import _lib

    q, table, target, ptr, idx, _ = make_case("dot", 67, 65, 4, True, 9)
    want = kernel_counts(q, table, target, "dot", GAMMA, ptr, idx)
    for key in [k for k in _ROUTE_NOTED if k[0] == "rank_all"]:
        _ROUTE_NOTED.discard(key)
    with pytest.warns(TorchRouteWarning) as rec:  # another dtype: exact data, the same counts
        got = rank_all(q.double().to(DEV), table.double().to(DEV), target.to(DEV), "dot", GAMMA, ptr.to(DEV), idx.to(DEV))
        rank_all(q.double().to(DEV), table.double().to(DEV), target.to(DEV), "dot")  # once per reason
    assert len([w for w in rec if w.category is TorchRouteWarning]) == 1 and torch.equal(got.cpu(), want)
    with pytest.warns(TorchRouteWarning):  # M == 0
        assert tuple(rank_all(q[:0].to(DEV), table.to(DEV), target[:0].to(DEV), "dot").shape) == (0, 3)
    with pytest.warns(TorchRouteWarning):  # D == 0: every candidate ties
        c = rank_all(q[:2, :0].to(DEV), table[:, :0].to(DEV), torch.tensor([1, 64], device=DEV), "l1", 1.0)
    assert c.tolist() == [[0, 1, 63], [0, 64, 0]]
    bad = (_lib.BackendError, ValueError)
    with pytest.raises(bad):
        rank_all(q.to(DEV), table.to(DEV), target.clone().index_fill_(0, torch.tensor([3]), 65).to(DEV), "dot")
    with pytest.raises(bad):
        rank_all(q.to(DEV), table.to(DEV), target.to(DEV), "dot", 0.0, ptr.to(DEV), (idx - 1).to(DEV))
    with pytest.raises(bad):
        rank_all(q.to(DEV), table.to(DEV), target.to(DEV), "dot", 0.0, ptr.flip(0).to(DEV), idx.to(DEV))
    with pytest.raises(bad):
        rank_all(q[:, :3].to(DEV), table[:, :3].to(DEV), target.to(DEV), "cl2")
    with pytest.raises(bad):
        rank_all(q.to(DEV), table, target.to(DEV), "dot")

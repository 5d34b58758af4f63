"""All-entity ranking without a GPU: the host twin of rank_all against the float64 oracle of tests/_kgrank_cases.py on the
golden cases (tests/golden/kg_rank.npz, recorded from the reference's own models and TestDataset), the torch route,
prepare_query, filter_lists against TestDataset's filter_bias rows, kg_metrics, ranks and the refusals."""
import numpy as np
import pytest
import torch

import _kgrank_cases as C
import _offset as O
from cogdl_amd import _lib
from cogdl_amd.kgrank import evaluate, filter_lists, kg_metrics, prepare_query
from cogdl_amd.operators import rank_all, ranks
from cogdl_amd.operators.kgrank import _composition

G = C.load()
TRIPLES = G["test_triples"].astype(np.int64)
CASE_MODES = [(m, f, mode) for m, f in C.CASES for mode in C.MODES]
_ORACLE = {}


def oracle(model, family, mode):
    """(s64 [M, N], target, left_out) of a golden case, computed once."""
    key = (model, family, mode)
    if key not in _ORACLE:
        ent, rel = C.tables(G, model, family)
        s64, target = C.model_scores64(model, mode, ent, rel, TRIPLES)
        _ORACLE[key] = (s64, target, C.left_out_mask(G, mode))
    return _ORACLE[key]


def run_case(model, family, mode, device="cpu", filtered=True):
    ent, rel = C.tables(G, model, family)
    ent, rel = torch.from_numpy(ent).to(device), torch.from_numpy(rel).to(device)
    filt = (None, None)
    if filtered:
        filt = filter_lists(torch.from_numpy(G["true_triples"].astype(np.int64)).to(device), torch.from_numpy(TRIPLES).to(device),
                            mode, C.N)
    return evaluate(model, ent, rel, torch.from_numpy(TRIPLES), mode, C.EMBEDDING_RANGE, C.GAMMA, *filt).cpu().numpy()


def check_case(counts, model, family, mode, filtered=True):
    """The issue's statement for one golden case; returns (lo, hi) of the bracket."""
    s64, target, left_out = oracle(model, family, mode)
    left_out = left_out if filtered else None
    key = C.tag(model, family, mode)
    total = counts.sum(1)
    if family == "exact":
        want = C.counts64(s64, target, left_out)
        assert np.array_equal(counts, want), (key, np.nonzero((counts != want).any(1))[0][:5])
        if filtered:
            pos = G["pos_f32_" + key].astype(np.int64)
            assert np.array_equal(pos, G["pos_f64_" + key]) and (counts[:, 0] <= pos).all() and (pos <= total).all(), key
        return counts[:, 0], total
    lo, hi = C.bracket64(s64, target, left_out, C.delta_of(G["ref_err_" + key], s64))
    assert (lo <= counts[:, 0]).all() and (total <= hi).all(), (key, np.nonzero((lo > counts[:, 0]) | (total > hi))[0][:5])
    assert (lo != hi).mean() <= C.AMBIGUOUS_CAP, (key, (lo != hi).mean())
    if filtered:
        mrr = float((1.0 / (1.0 + counts[:, 0] + counts[:, 1])).mean())
        ref = float((1.0 / (1.0 + G["pos_f32_" + key].astype(np.float64))).mean())
        assert abs(mrr - ref) <= C.mrr_bound(lo, hi) + 1e-15, (key, mrr, ref, C.mrr_bound(lo, hi))
    return lo, hi


@pytest.mark.parametrize("model,family,mode", CASE_MODES)
def test_host_twin_on_the_golden_cases(model, family, mode):
    check_case(run_case(model, family, mode), model, family, mode)


@pytest.mark.parametrize("model,family", C.CASES)
def test_host_twin_unfiltered(model, family):
    check_case(run_case(model, family, "tail-batch", filtered=False), model, family, "tail-batch", filtered=False)


@pytest.mark.parametrize("model,family,mode", CASE_MODES)
def test_prepare_query_against_the_recorded_scores(model, family, mode):
    """Scores from q (float32, summed in float64) equal the reference's recorded float32 scores within ref_err.  DistMult and
    ComplEx expose their intermediate -- the golden holds it as the reference's own score() returned it against unit-vector
    candidates (q_ref_*) -- and q equals it bit for bit.  TransE and RotatE expose none (a norm stands between the intermediate
    and everything score() returns): for them the recorded scores are the only independent check."""
    ent, rel = C.tables(G, model, family)
    fixed, free = C.fixed_free(mode)
    rows, rels = torch.from_numpy(ent[TRIPLES[:, fixed]]), torch.from_numpy(rel[TRIPLES[:, 1]])
    q, kind, gamma = prepare_query(model, mode, rows, rels, C.EMBEDDING_RANGE, C.GAMMA)
    assert kind == C.KIND[model] and q.dtype == torch.float32 and gamma == (0.0 if kind == "dot" else C.GAMMA)
    assert tuple(q.shape) == (len(TRIPLES), ent.shape[1])
    key = C.tag(model, family, mode)
    if kind == "dot":
        assert torch.equal(q[:C.SCORE_ROWS], torch.from_numpy(G["q_ref_" + key])), key
    rec = G["scores_f32_" + key].astype(np.float64)
    mine = C.scores64(kind, q[:C.SCORE_ROWS].numpy(), ent, C.GAMMA)
    keep = ~C.left_out_mask(G, mode)[:C.SCORE_ROWS]  # (a filtered candidate was scored as a copy of the target)
    err = np.abs(mine - rec)[keep].max()
    assert err <= float(G["ref_err_" + key]), (key, err, float(G["ref_err_" + key]))


@pytest.mark.parametrize("mode", C.MODES)
def test_filter_lists_against_testdataset(mode):
    ptr, idx = filter_lists(torch.from_numpy(G["true_triples"].astype(np.int64)), torch.from_numpy(TRIPLES), mode, C.N)
    assert ptr.dtype == torch.int32 and idx.dtype == torch.int32 and ptr.numel() == len(TRIPLES) + 1
    mask = np.zeros((len(TRIPLES), C.N), dtype=bool)
    free = C.fixed_free(mode)[1]
    for i in range(len(TRIPLES)):
        ids = idx[ptr[i]:ptr[i + 1]].numpy()
        assert (np.diff(ids) > 0).all()  # ascending, distinct
        assert TRIPLES[i, free] in ids   # (the test triple is a true one)
        mask[i, ids] = True
        mask[i, TRIPLES[i, free]] = False  # TestDataset puts the target back (tmp[head] = (0, head))
    assert np.array_equal(mask, C.left_out_mask(G, mode))
    # duplicates in all_triples change nothing; an unknown (relation, entity) pair gets an empty list
    twice = torch.from_numpy(np.concatenate([G["true_triples"], G["true_triples"][:100]]).astype(np.int64))
    ptr2, idx2 = filter_lists(twice, torch.from_numpy(TRIPLES), mode, C.N)
    assert torch.equal(ptr, ptr2) and torch.equal(idx, idx2)
    ptr3, idx3 = filter_lists(torch.tensor([[0, 0, 1]]), torch.tensor([[5, 3, 6], [0, 0, 1]]), mode, C.N)
    assert ptr3.tolist() == [0, 0, 1] and idx3.tolist() == [0 if mode == "head-batch" else 1]
    with pytest.raises(ValueError):
        filter_lists(torch.tensor([[0, 0, C.N]]), torch.tensor([[0, 0, 1]]), mode, C.N)
    with pytest.raises(ValueError):
        filter_lists(torch.tensor([[0, 0, 1]]), torch.tensor([[0, 0, 1]]), "single", C.N)


def _small(kind, m=67, n=65, d=6, seed=3):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randint(-8, 9, (n, d), generator=gen).float() / 4
    table[n // 2] = table[0]
    q = torch.randint(-8, 9, (m, d), generator=gen).float() / 4
    target = torch.randint(0, n, (m,), generator=gen)
    lens = torch.randint(0, 7, (m,), generator=gen)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    idx = torch.randint(0, n, (int(ptr[-1]),), generator=gen)
    return q, table, target, ptr, idx


def _oracle_counts(kind, q, table, target, ptr, idx, gamma):
    left = np.zeros((q.shape[0], table.shape[0]), dtype=bool)
    if ptr is not None:
        for i in range(q.shape[0]):
            left[i, idx[ptr[i]:ptr[i + 1]].numpy()] = True
    left[np.arange(q.shape[0]), target.numpy()] = False
    return C.counts64(C.scores64(kind, q.numpy(), table.numpy(), gamma), target.numpy(), left)


@pytest.mark.parametrize("kind", ["dot", "l1", "cl2"])
def test_host_twin_and_torch_route_on_exact_data(kind):
    q, table, target, ptr, idx = _small(kind)
    want = _oracle_counts(kind, q, table, target, ptr, idx, 3.0)
    got = rank_all(q, table, target, kind, 3.0, ptr, idx)
    assert got.dtype == torch.int32 and tuple(got.shape) == (67, 3) and np.array_equal(got.numpy(), want)
    assert want[:, 1:].sum() > 0  # (ties are present)
    # int32 operands, lists given in another order and with every entry twice: the same counts
    perm = torch.cat([torch.arange(int(ptr[i]), int(ptr[i + 1])).flip(0).repeat(2) for i in range(67)])
    assert torch.equal(rank_all(q, table, target.int(), kind, 3.0, (2 * ptr).int(), idx[perm].int()), got)
    # the torch composition: float64 operands on the CPU (quietly), the same counts on exact data
    assert torch.equal(rank_all(q.double(), table.double(), target, kind, 3.0, ptr, idx), got)
    assert torch.equal(_composition(q, table, target, kind, 3.0, None, None), rank_all(q, table, target, kind, 3.0))
    # operands that start mid-allocation, and non-contiguous ones
    qs, _ = O.shifted(q, 1)
    ts, _ = O.shifted(table, 3)
    assert torch.equal(rank_all(qs, ts, target, kind, 3.0, ptr, idx), got)
    assert torch.equal(rank_all(O.strided(q), O.strided(table), target, kind, 3.0, ptr, idx), got)


def test_special_values_and_empty_operands():
    inf, nan = float("inf"), float("nan")
    table = torch.tensor([[1.0, 0.0], [inf, 0.0], [-inf, 0.0], [nan, 0.0], [1.0, 0.0], [2.0, 0.0]])
    q = torch.tensor([[1.0, 0.0]] * 4)
    target = torch.tensor([0, 1, 3, 4])
    got = rank_all(q, table, target, "dot").tolist()
    # target 0 (score 1): above it inf and 2; equal to it row 4 (after); -inf below; NaN nowhere
    assert got[0] == [2, 0, 1]
    assert got[1] == [0, 0, 0]      # the target scores +inf: nothing is above, nothing else equals it
    assert got[2] == [0, 0, 0]      # the target scores NaN: compares false both ways
    assert got[3] == [2, 1, 0]      # the tie partner comes before
    # empty operands: zeros of the right shape; D == 0 ties everything
    assert tuple(rank_all(torch.zeros(0, 4), table.new_zeros(5, 4), torch.zeros(0, dtype=torch.int64), "dot").shape) == (0, 3)
    c = rank_all(torch.zeros(2, 0), torch.zeros(5, 0), torch.tensor([1, 4]), "l1", 1.0)
    assert c.tolist() == [[0, 1, 3], [0, 4, 0]]
    with pytest.raises(_lib.BackendError):  # N == 0 leaves no valid target
        rank_all(torch.zeros(2, 3), torch.zeros(0, 3), torch.tensor([0, 0]), "dot")


def test_ranks_and_metrics():
    counts = torch.tensor([[0, 0, 0], [2, 1, 3], [9, 0, 0], [0, 2, 0]], dtype=torch.int32)
    assert ranks(counts).tolist() == [1, 4, 10, 3] and ranks(counts).dtype == torch.int64
    assert ranks(counts, "optimistic").tolist() == [1, 3, 10, 1]
    assert ranks(counts, "pessimistic").tolist() == [1, 7, 10, 3]
    assert ranks(counts, "mean").tolist() == [1.0, 5.0, 10.0, 2.0]
    m = kg_metrics(counts, "stable")
    assert sorted(m) == ["HITS@1", "HITS@10", "HITS@3", "MR", "MRR"]
    assert m["MR"] == 4.5 and abs(m["MRR"] - (1 + 1 / 4 + 1 / 10 + 1 / 3) / 4) < 1e-15
    assert m["HITS@1"] == 0.25 and m["HITS@3"] == 0.5 and m["HITS@10"] == 1.0
    both = kg_metrics([counts, counts], "optimistic", hits=(2,))
    assert both["HITS@2"] == 0.5 and both["MR"] == 3.75
    with pytest.raises(ValueError):
        ranks(counts, "first")
    with pytest.raises(ValueError):
        kg_metrics(counts[:0])


def test_refusals():
    q, table, target, ptr, idx = _small("dot")
    bad = (_lib.BackendError, ValueError)
    with pytest.raises(bad):
        rank_all(q, table, target, "l2")
    with pytest.raises(bad):
        rank_all(q[:, :5], table[:, :5], target, "cl2")  # odd D
    with pytest.raises(bad):
        rank_all(q, table[:, :5], target, "dot")
    with pytest.raises(bad):
        rank_all(q, table, target[:-1], "dot")
    with pytest.raises(bad):
        rank_all(q, table, target.float(), "dot")
    for t in (target.clone().index_fill_(0, torch.tensor([5]), 65), target.clone().index_fill_(0, torch.tensor([0]), -1)):
        with pytest.raises(bad):
            rank_all(q, table, t, "dot")
    with pytest.raises(bad):
        rank_all(q, table, target, "dot", 0.0, ptr, idx.clone().index_fill_(0, torch.tensor([2]), 65))
    with pytest.raises(bad):
        rank_all(q, table, target, "dot", 0.0, ptr[:-1], idx)
    with pytest.raises(bad):
        rank_all(q, table, target, "dot", 0.0, ptr, None)
    swapped = ptr.clone()
    swapped[3], swapped[4] = ptr[4] + 1, ptr[3]
    with pytest.raises(bad):
        rank_all(q, table, target, "dot", 0.0, swapped, idx)
    with pytest.raises(bad):
        rank_all(q, table, target, "dot", 0.0, ptr, idx[:-1])
    with pytest.raises(bad):
        rank_all(q, table.double(), target, "dot")
    with pytest.raises(ValueError):
        prepare_query("conve", "tail-batch", q, q)
    with pytest.raises(ValueError):
        prepare_query("rotate", "tail-batch", q, q[:, :3])  # no embedding_range
    # the C entry points themselves: an unknown kind, odd D with cl2
    lib = _lib.host()
    out = torch.empty(67, 3, dtype=torch.int32)
    args = (q.data_ptr(), table.data_ptr(), target.int().data_ptr(), 67, 65)
    assert lib.cogdl_host_kg_rank(*args, 6, 3, 0.0, None, None, 0, out.data_ptr()) != 0
    assert lib.cogdl_host_kg_rank(*args, 5, 2, 0.0, None, None, 0, out.data_ptr()) != 0

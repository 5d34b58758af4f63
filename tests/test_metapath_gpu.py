"""The metapath walk (walk_kernel<MetapathRule>, csrc/walk.hip) on the GPU: bit-for-bit equal to the host twin, `lengths` included, over the case
graphs, the length and walker sweeps and several metapaths; stream use; the T == 1 identity with random_walk; an R-MAT run
under the brute-force checker; error flags equal to the host's instead of faults."""
import numpy as np
import pytest
import torch

import _metapath_cases as cases
from cogdl_amd import _lib, synth
from cogdl_amd.operators import metapath_walk, random_walk, typed_rows
from cogdl_amd.operators import walk as walk_mod

from test_metapath_host import LENGTHS, WALKERS, host_call, no_dead_end_graph, schemas_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEEP_SCHEMA = "0-1-0,0-2-0,1-0-2-0-1"


def both(indptr, indices, node_type, start, schema, length, which, seed):
    host = metapath_walk(indptr, indices, node_type, start, schema, length, walker_path=which, seed=seed, return_lengths=True)
    gpu = metapath_walk(indptr.to(DEV), indices.to(DEV), node_type.to(DEV), start.to(DEV), schema, length,
                        walker_path=None if which is None else which.to(DEV), seed=seed, return_lengths=True)
    assert gpu[0].is_cuda and gpu[0].dtype == torch.int64 and gpu[1].is_cuda and gpu[1].dtype == torch.int32
    assert tuple(gpu[0].shape) == (start.numel(), length)
    return host, (gpu[0].cpu(), gpu[1].cpu())


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_gpu_equals_host_on_every_graph(name):
    indptr, indices, node_type, n = cases.CASES[name]()
    for k, schema in enumerate(schemas_for(node_type)):
        paths = walk_mod.parse_schema(schema)
        start, which = cases.starts_for(node_type, paths, repeat=5)
        mixed = torch.randperm(start.numel(), generator=torch.Generator().manual_seed(k))
        start, which = start[mixed], which[mixed]
        host, gpu = both(indptr, indices, node_type, start, schema, 33, which, 40 + k)
        assert torch.equal(host[0], gpu[0]) and torch.equal(host[1], gpu[1]), (name, schema)


@pytest.fixture(scope="module")
def sweep_graph():
    indptr, indices, node_type, n = cases.random_typed()
    start, which = cases.starts_for(node_type, walk_mod.parse_schema(SWEEP_SCHEMA), repeat=2)
    return (indptr, indices, node_type), (indptr.to(DEV), indices.to(DEV), node_type.to(DEV)), start, which


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("walkers", WALKERS)
def test_gpu_equals_host_over_lengths_and_walker_counts(sweep_graph, length, walkers):
    host_g, gpu_g, start, which = sweep_graph
    start, which = start[:walkers], which[:walkers]
    want, want_len = metapath_walk(*host_g, start, SWEEP_SCHEMA, length, walker_path=which, seed=80, return_lengths=True)
    got, got_len = metapath_walk(*gpu_g, start.to(DEV), SWEEP_SCHEMA, length, walker_path=which.to(DEV), seed=80, return_lengths=True)
    assert tuple(got.shape) == (walkers, length) and torch.equal(got.cpu(), want) and torch.equal(got_len.cpu(), want_len)
    plain = metapath_walk(*gpu_g, start.to(DEV), SWEEP_SCHEMA, length, walker_path=which.to(DEV), seed=80)  # lengths = NULL
    assert torch.equal(plain, got)


def test_same_seed_on_a_side_stream_gives_the_same_array(sweep_graph):
    _, gpu_g, start, which = sweep_graph
    start, which = start.to(DEV), which.to(DEV)
    a = metapath_walk(*gpu_g, start, SWEEP_SCHEMA, 40, walker_path=which, seed=5)
    assert torch.equal(a, metapath_walk(*gpu_g, start, SWEEP_SCHEMA, 40, walker_path=which, seed=5))
    assert not torch.equal(a, metapath_walk(*gpu_g, start, SWEEP_SCHEMA, 40, walker_path=which, seed=6))
    # priority -1: torch hands high-priority streams out of a pool of their own, and the runtime gives that pool its own
    # hardware queues.  A stream of the ordinary pool would shift by one which pool stream, and with it which hardware queue,
    # every later test's side stream gets: the overlap test of test_pipeline_gpu.py needs its side stream on another queue
    # than the stream that trains.
    side = torch.cuda.Stream(priority=-1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = metapath_walk(*gpu_g, start, SWEEP_SCHEMA, 40, walker_path=which, seed=5)
    side.synchronize()
    assert torch.equal(a, b)


def test_one_type_equals_the_first_order_walk_on_the_gpu():
    indptr, indices, n = no_dead_end_graph()
    ip, ix = indptr.to(DEV), indices.to(DEV)
    start = torch.arange(n, device=DEV).repeat(3)
    zeros = torch.zeros(n, dtype=torch.long, device=DEV)
    for length in (1, 9, 40):
        want = random_walk(ip, ix, start, length, restart_p=0.0, seed=77)
        got = metapath_walk(ip, ix, zeros, start, "0-0", length, seed=77)
        assert torch.equal(got, want)
        assert torch.equal(got.cpu(), random_walk(indptr, indices, start.cpu(), length, restart_p=0.0, seed=77))


def test_rmat_walks_pass_the_brute_force_checker():
    n = 20_000
    src, dst = synth.rmat_pairs(n, 150_000, seed=3)
    g = synth.finalize(src, dst, n, symmetrise=True, self_loops=False, norm="sym")
    indptr, indices = g.rowptr.long(), g.colind.long()
    node_type = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(9))
    paths = walk_mod.parse_schema(SWEEP_SCHEMA)
    first = torch.tensor([0, 0, 1])
    which = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(10))
    which = torch.where(first[which] == node_type, which, torch.where(node_type == 1, 2, which % 2))
    keep = first[which] == node_type  # (type-2 nodes start no metapath of this schema)
    start, which = torch.arange(n)[keep], which[keep].int()
    assert start.numel() > 12_000
    seg, indices_t = typed_rows(indptr.to(DEV), indices.to(DEV), node_type.to(DEV))
    host_seg, host_t = typed_rows(indptr, indices, node_type)
    assert torch.equal(seg.cpu(), host_seg) and torch.equal(indices_t.cpu(), host_t)  # the layout built on the device
    walks, lengths = metapath_walk(indptr.to(DEV), indices.to(DEV), node_type.to(DEV), start.to(DEV), SWEEP_SCHEMA, 20,
                                   walker_path=which.to(DEV), seed=1, return_lengths=True)
    held = cases.check_walks(indptr, indices, node_type, start, paths, which, walks.cpu(), lengths.cpu())
    assert held.min() < 20 and held.max() == 20


def hip_call(seg, indices_t, n, t, types, start, which, length, pattern, path_off):
    """The HIP entry point itself on device copies -> (rc, flags, walks, lengths) on the host."""
    dev = lambda x, dt: None if x is None else torch.as_tensor(x, dtype=dt).to(DEV)  # noqa: E731
    seg, indices_t, types = dev(seg, torch.long), dev(indices_t, torch.long), dev(types, torch.int32)
    start, which = dev(start, torch.long), dev(which, torch.int32)
    pattern, path_off = dev(pattern, torch.int32), dev(path_off, torch.int32)
    w = start.numel()
    walks = torch.full((w, length), -7, dtype=torch.long, device=DEV)
    held = torch.full((w,), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rc = _lib.hip().cogdl_hip_metapath_walk(_lib.ptr(seg), _lib.ptr(indices_t), n, t, indices_t.numel(), _lib.ptr(types),
                                            _lib.ptr(start), _lib.ptr(which), w, length, _lib.ptr(pattern), _lib.ptr(path_off),
                                            path_off.numel() - 1, 9, _lib.ptr(walks), _lib.ptr(held), _lib.ptr(flags),
                                            _lib.stream_of(walks))
    torch.cuda.synchronize()
    return rc, int(flags), walks.cpu(), held.cpu()


def test_flags_equal_the_hosts_and_raise():
    indptr, indices, node_type, n = cases.random_typed()
    seg, indices_t = typed_rows(indptr, indices, node_type)
    types = node_type.int()
    zero, one = int(torch.nonzero(node_type == 0)[0]), int(torch.nonzero(node_type == 1)[0])
    gpu_g = (indptr.to(DEV), indices.to(DEV), node_type.to(DEV))
    for starts, want_flags, text in (([zero, zero], 0, None), ([zero, one], 8, "first type of its metapath"),
                                     ([zero, n], 1, "start id"), ([zero, -3], 1, "start id")):
        args = (seg, indices_t, n, 3, types, starts, [0, 0], 9, [0, 1], [0, 2])
        host, gpu = host_call(*args), hip_call(*args)
        assert host[:2] == (0, want_flags) and gpu[:2] == host[:2], (starts, host[:2], gpu[:2])
        assert torch.equal(gpu[2], host[2]) and torch.equal(gpu[3], host[3])
        if text:
            with pytest.raises(_lib.BackendError, match=text):
                metapath_walk(*gpu_g, torch.tensor(starts, device=DEV), "0-1-0", 9, seed=0)
    # a wanted type or a metapath id out of range, a malformed path_off: the host's flag, no fault
    for which, pattern, path_off in (([0], [0, 3], [0, 2]), ([1], [0, 1], [0, 2]), ([-1], [0, 1], [0, 2])):
        args = (seg, indices_t, n, 3, types, [zero], which, 9, pattern, path_off)
        host, gpu = host_call(*args), hip_call(*args)
        assert host[1] == 16 and gpu[:2] == host[:2] and torch.equal(gpu[2], host[2])
    # argument checks of the entry point
    on_dev = seg.to(DEV)
    lib, p = _lib.hip(), _lib.ptr(on_dev)
    assert lib.cogdl_hip_metapath_walk(p, p, n, 65, 1, None, p, p, 1, 4, p, p, 1, 1, p, None, p, None) == 1
    assert lib.cogdl_hip_metapath_walk(p, p, n, 0, 1, None, p, p, 1, 4, p, p, 1, 1, p, None, p, None) == 1
    assert lib.cogdl_hip_metapath_walk(p, p, n, 3, 1, None, p, p, 1, 4, p, p, 0, 1, p, None, p, None) == 1
    assert lib.cogdl_hip_metapath_walk(p, p, n, 3, 1, None, p, None, 1, 4, p, p, 1, 1, p, None, p, None) == 1
    with pytest.raises(_lib.BackendError):
        metapath_walk(gpu_g[0], gpu_g[1], node_type, torch.tensor([zero], device=DEV), "0-1-0", 5)  # mixed devices

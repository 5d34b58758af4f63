"""install(diffpool=True) without a GPU: the flag, the CPU composition of diffpool_coarsen against the float64 loop, and -- against
the REAL reference package (the copy build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE; skipped where neither is present)
in a fresh interpreter -- the rebind, its undo through the journal, the served layer on the torch composition and the inputs
that reach the reference's forward (tests/_diffpool_layer_run.py)."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

import _segmm_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


def test_the_flag_defaults_to_false_and_sits_before_actnn():
    import cogdl_amd

    params = inspect.signature(cogdl_amd.install).parameters
    assert params["diffpool"].default is False and list(params).index("diffpool") < list(params).index("actnn")


@pytest.mark.parametrize("lens,k,f", [("ragged", 33, 6), ("front", 3, 65)])
def test_cpu_composition_of_diffpool_coarsen_matches_the_float64_loop(lens, k, f):
    from cogdl_amd.operators import diffpool_coarsen

    s, (embed,), _ = C.tn_inputs(lens, k, (f,), True)
    ptr, n, s = C.ptr_of(lens), s.shape[0], torch.softmax(s, 1)
    gen = torch.Generator().manual_seed(n)
    row = torch.sort(torch.randint(0, n, (4 * n,), generator=gen))[0]
    col, weight = torch.randint(0, n, (4 * n,), generator=gen), torch.rand(4 * n, generator=gen)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(row, minlength=n), 0)]).int()
    got = diffpool_coarsen(rowptr, col.int(), weight, s, embed, ptr)
    a = torch.zeros(n, n, dtype=torch.float64).index_put((row, col), weight.double(), accumulate=True)
    want = C.loop_tn(s.double(), (embed.double(), a @ s.double(), s.double()), ptr)
    assert tuple(got[0].shape) == (len(C.LENS[lens]) * k, f)
    for g, w in zip(got, want):  # float32 sums of at most 130 products of O(1) terms: 130 eps32 = 8e-6 of the largest entry
        assert float((g.double().reshape(w.shape) - w).abs().max()) <= 1e-5 * float(w.abs().max())


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_install_serves_the_reference_layer_and_the_journal_undoes_it():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_diffpool_layer_run.py"), ROOT, REF, "cpu"],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "DIFFPOOL-LAYER-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]

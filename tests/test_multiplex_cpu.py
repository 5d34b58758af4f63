"""multiplex_embed without a GPU: CPU tensors run the torch composition, which equals the float64 oracle to float32 rounding and
passes gradcheck; argument errors; and the CPU route never loads libcogdl_hip.so."""
import subprocess
import sys

import pytest
import torch

import _multiplex_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators.multiplex import composition, multiplex_embed


@pytest.mark.parametrize("name", C.CASES)
def test_cpu_route_equals_the_oracle_to_float32_rounding(name):
    oracle, ref32 = C.reference(name)
    got = C.run(multiplex_embed, name)
    for k in C.NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
    c = C.make(name)
    u, a, t, s = c["type_emb"].shape[2], c["att_w1"].shape[2], c["type_emb"].shape[1], c["neigh"].shape[2]
    d = c["node_emb"].shape[1]
    # float32 rounding of sums of at most max(S, U, A, T, D) terms, of lists of at most B S entries for a gradient, relative to
    # the largest magnitude of the tensor or to 1 (operands and G are O(1); where D == 1 the exact gradient cancels to 0); the
    # softmax of the large_e case turns an error of eps32 |e| in a score into that relative error of att
    terms = max(s, u, a, t, d) * (1000.0 if name == "large_e" else 1.0)
    for k, (err_new, _, _) in C.errors(got, oracle, ref32).items():
        scale = float(oracle[k].abs().max())
        lists = c["inputs"].numel() * s if k.startswith("g_") else 1
        print("%s %-8s err %.3e  max|oracle| %.3e" % (name, k, err_new, scale))
        assert err_new <= 16 * C.EPS32 * terms * lists ** 0.5 * max(scale, 1.0), k
    if name == "zero_norm":
        assert bool((got["out"][0] == 0).all())


def test_gradcheck_of_the_composition_in_float64():
    c = C.make("d1_u1_a1_t1_s1_b1")
    ops = [c[k].double().requires_grad_() for k in C.FLOATS]
    assert torch.autograd.gradcheck(lambda *f: composition(*f, c["neigh"], c["inputs"], c["types"]), ops)
    c = C.make("d7_u3_a20_t2_s10_b7")
    ops = [c[k].double().requires_grad_() for k in C.FLOATS]
    assert torch.autograd.gradcheck(lambda *f: composition(*f, c["neigh"], c["inputs"], c["types"]), ops)


def test_b1_and_t1_are_served_and_rows_have_unit_norm():
    for name in ("d200_u33_a20_t1_s10_b1", "d7_u10_a1_t2_s1_b1"):
        c = C.make(name)
        out = multiplex_embed(*[c[k] for k in C.FLOATS], c["neigh"], c["inputs"], c["types"])
        assert tuple(out.shape) == (1, c["node_emb"].shape[1])
        assert abs(float(out.norm()) - 1.0) < 1e-5


def test_argument_errors():
    c = C.make("d7_u3_a20_t2_s10_b7")
    f = [c[k] for k in C.FLOATS]
    neigh, inputs, types = c["neigh"], c["inputs"], c["types"]
    with pytest.raises(ValueError):
        multiplex_embed(f[0][:, :3], *f[1:], neigh, inputs, types)  # D differs from trans_w's
    with pytest.raises(ValueError):
        multiplex_embed(f[0], f[1][:-1], *f[2:], neigh, inputs, types)  # N differs
    with pytest.raises(ValueError):
        multiplex_embed(*f[:4], f[4][:, :5], neigh, inputs, types)  # A differs
    with pytest.raises(ValueError):
        multiplex_embed(*f, neigh[:, :1], inputs, types)  # neigh is not [N, T, S]
    with pytest.raises(ValueError):
        multiplex_embed(*f, neigh.float(), inputs, types)
    with pytest.raises(ValueError):
        multiplex_embed(*f, neigh, inputs, types[:-1])
    with pytest.raises(ValueError):
        multiplex_embed(*f, neigh, inputs.float(), types)
    with pytest.raises(ValueError):
        multiplex_embed(f[0].double(), *f[1:], neigh, inputs, types)  # mixed float dtypes
    with pytest.raises(ValueError):
        multiplex_embed(*f, neigh, inputs.tolist(), types)
    for where in ("inputs", "types", "neigh"):
        bad = {"inputs": inputs.clone(), "types": types.clone(), "neigh": neigh.clone()}
        bad[where].view(-1)[2] = C.N if where != "types" else 2
        with pytest.raises(_lib.BackendError):
            multiplex_embed(*f, bad["neigh"], bad["inputs"], bad["types"])
        bad[where].view(-1)[2] = -1
        with pytest.raises(_lib.BackendError):
            multiplex_embed(*f, bad["neigh"], bad["inputs"], bad["types"])


def test_unchecked_bad_ids_give_nan_rows_and_no_gradient():
    c = C.make("d7_u3_a20_t2_s10_b7")
    f = [c[k].clone().requires_grad_() for k in C.FLOATS]
    inputs, types, neigh = c["inputs"].clone(), c["types"].clone(), c["neigh"].clone()
    inputs[1], types[3] = C.N, -1
    spoiled = int(c["inputs"][5])
    neigh[spoiled, 1, 4] = C.N + 3
    out = multiplex_embed(*f, neigh, inputs, types, check=False)
    bad_rows = torch.tensor([b in (1, 3) or int(inputs[b]) == spoiled for b in range(7)])
    assert bool(torch.isnan(out[bad_rows]).all()) and bool(torch.isfinite(out[~bad_rows]).all())
    grads = torch.autograd.grad(out[~bad_rows].sum() + torch.nan_to_num(out[bad_rows]).sum(), f)
    keep = ~bad_rows
    g = [x.clone().requires_grad_() for x in f]
    want = torch.autograd.grad(multiplex_embed(*g, c["neigh"], c["inputs"][keep], c["types"][keep]).sum(), g)
    for a, b in zip(grads, want):
        assert bool(torch.isfinite(a).all()) and torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_empty_batch():
    c = C.make("d7_u3_a20_t2_s10_b7")
    f = [c[k].clone().requires_grad_() for k in C.FLOATS]
    out = multiplex_embed(*f, c["neigh"], c["inputs"][:0], c["types"][:0])
    assert tuple(out.shape) == (0, 7)
    grads = torch.autograd.grad(out.sum(), f)
    assert all(bool((g == 0).all()) for g in grads)


def test_cpu_tensors_do_not_load_the_hip_library():
    code = ("import torch\n"
            "from cogdl_amd import _lib\n"
            "from cogdl_amd.operators.multiplex import multiplex_embed\n"
            "g = torch.Generator().manual_seed(0)\n"
            "f = [torch.randn(6, 4, generator=g), torch.randn(6, 2, 3, generator=g), torch.randn(2, 3, 4, generator=g),\n"
            "     torch.randn(2, 3, 5, generator=g), torch.randn(2, 5, generator=g)]\n"
            "f = [x.requires_grad_() for x in f]\n"
            "out = multiplex_embed(*f, torch.randint(0, 6, (6, 2, 3), generator=g), torch.tensor([0, 5, 2]), torch.tensor([1, 0, 1]))\n"
            "out.sum().backward()\n"
            "assert _lib._hip is None\n"
            "assert 'libcogdl_hip' not in open('/proc/self/maps').read()\n"
            "print('ok')\n")
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr

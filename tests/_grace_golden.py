"""Shared by tests/test_grace_loss_gpu.py and tests/test_contrast_install_cpu.py: tests/golden/grace_loss.npz (the reference's
GRACE loss on fixed inputs, tests/golden/make_golden_grace.py) against a loss function under the rule of tests/_gen_cases.py,
err_new <= 4 * ref_err + 8 * eps32 * max|float64 record|, ref_err the reference's own float32 error stored in the file."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
TAU, BATCH = 0.4, 32
NAMES = ("loss", "g_z1", "g_z2")


def batched(loss_fn, z1, z2, batch):
    """grace_mw.py:79-91 over `loss_fn(z1[idx], z2)`."""
    n = z1.shape[0]
    losses = [loss_fn(z1[i:i + batch], z2) for i in range(0, n, batch)]
    return sum(losses) / len(losses)


def run(fn, rec, device="cpu"):
    a = torch.from_numpy(rec["z1"]).to(device).requires_grad_()
    b = torch.from_numpy(rec["z2"]).to(device).requires_grad_()
    loss = fn(a, b)
    loss.backward()
    return {"loss": loss.detach().reshape(1).cpu(), "g_z1": a.grad.cpu(), "g_z2": b.grad.cpu()}


def check(tag, got, rec):
    bad = []
    for name in NAMES:
        want = torch.from_numpy(rec["%s_%s_f64" % (tag, name)])
        err_ref = float(rec["ref_err_%s_%s" % (tag, name)])
        err_new = float((got[name].double() - want).abs().max())
        bound = 4 * err_ref + 8 * EPS32 * float(want.abs().max())
        line = "%-8s %-5s err_new %.3e  err_ref %.3e  bound %.3e" % (tag, name, err_new, err_ref, bound)
        print(line)
        if not (bool(torch.isfinite(got[name]).all()) and err_new <= bound):
            bad.append(line)
    assert not bad, bad

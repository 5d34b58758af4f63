"""Writes tests/golden/grace_loss.npz: fixed inputs and what the reference's own GRACE wrapper computes on them, in float32 and
in float64.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs, and
NOT rebound: GRACEModelWrapper.contrastive_loss and batched_loss (cogdl/wrappers/model_wrapper/node_classification/
grace_mw.py:64-91) run as they are, on the CPU.  Both are functions of their arguments and self.tau alone, so the float64 run
-- the oracle -- is the same method on float64 inputs.

N = 70, d = 24, tau 0.4; z1, z2 random and unnormalised (the method normalises).  `full` is contrastive_loss(z1, z2), `batched`
is batched_loss(z1, z2, 32): three batches of 32, 32 and 6 rows.  Recorded: z1, z2 (float32), <tag>_<name>_f64 for
name in loss, g_z1, g_z2 (the gradients of the loss) and ref_err_<tag>_<name> = max |float32 run - f64|, the
yardstick of tests/test_grace_loss_gpu.py and tests/test_contrast_install_cpu.py.  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
N, D, TAU, BATCH = 70, 24, 0.4, 32


def main():
    import torch

    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(HERE, "_stubs"), scratch]
    from cogdl.wrappers.model_wrapper.node_classification.grace_mw import GRACEModelWrapper

    torch.manual_seed(20254)
    z1, z2 = torch.randn(N, D), torch.randn(N, D)
    wrapper = GRACEModelWrapper(torch.nn.Identity(), {"hidden_size": D, "lr": 0.01, "weight_decay": 0.0}, TAU, [0.3, 0.4],
                                [0.2, 0.4], BATCH, 16)
    out = {"z1": z1, "z2": z2}
    for tag, fn in (("full", wrapper.contrastive_loss), ("batched", lambda a, b: wrapper.batched_loss(a, b, BATCH))):
        for dtype, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
            a, b = z1.to(dtype).clone().requires_grad_(), z2.to(dtype).clone().requires_grad_()
            loss = fn(a, b)
            loss.backward()
            assert loss.dtype == dtype
            out.update({"%s_loss_%s" % (tag, suffix): loss.detach().reshape(1), "%s_g_z1_%s" % (tag, suffix): a.grad,
                        "%s_g_z2_%s" % (tag, suffix): b.grad})
    out = {k: v.numpy() for k, v in out.items()}
    for tag in ("full", "batched"):
        for name in ("loss", "g_z1", "g_z2"):
            f32, f64 = out["%s_%s_f32" % (tag, name)], out["%s_%s_f64" % (tag, name)]
            err = float(np.abs(f32.astype(np.float64) - f64).max())
            out["ref_err_%s_%s" % (tag, name)] = np.asarray(err)
            del out["%s_%s_f32" % (tag, name)]  # (the float32 run is kept as its error alone)
            print("%-16s ref_err %.3e  max %.3e" % (tag + " " + name, err, float(np.abs(f64).max())))
    path = os.path.join(HERE, "grace_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()

"""Activation compression, measured on the GPU (profiles/actnn_bench.txt):

  1. quantise and dequantise at [169343, 256] float32 for b in {2, 4}, G = 256: median and best device-event time of 30 launches
     after 5 warm-up launches, the bytes each kernel has to move (float32 in or out, packed codes, one (min, step) pair per
     group) per second, beside the copy roof measured in the same process (tools/papers_bench.py: measured_roofs, what
     `bench.py --full` reports); relu_mask and drop_apply at the same shape ride along;
  2. one training epoch on the arxiv-shaped graph through the reference's unchanged Trainer: its `actgcn` (hidden 256, 3
     layers) under install(actnn=True) against its `gcn` under install(): time per epoch (median of the epochs after the first
     two) and torch.cuda.max_memory_allocated, each model in a fresh interpreter.

    python tools/actnn_bench.py [--out profiles/actnn_bench.txt] [--epochs 8] [--skip-epoch]

Needs a GPU; the epoch part needs the staged reference package (oracle/_ref/pkg).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (169343, 256)


def _time(fn, warmup=5, reps=30):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def kernels(lines):
    import torch

    from cogdl_amd import _lib
    from cogdl_amd.operators import actq
    from tools.papers_bench import measured_roofs

    dev = torch.device("cuda:0")
    roofs = measured_roofs(dev)
    copy = roofs["measured_copy_GBs"]
    lines.append("device: %s" % torch.cuda.get_device_name(0))
    lines.append("copy roof: %.0f GB/s (%s)" % (copy, roofs["what"]))
    lines.append("")
    lines.append("kernel                 shape            bits  bytes moved   median ms  best ms   GB/s (median)  share of copy roof")
    x = torch.randn(SHAPE, device=dev)
    n = x.numel()
    lib = _lib.hip()
    stream = _lib.stream_of(x)
    for bits in (2, 4):
        q = actq.quantize(x, bits, 256, seed=1, call=0)
        out = torch.empty_like(x)
        packed = q.codes.numel() * 4 + q.meta.numel() * 4
        for name, fn in (
                ("actq_quantize", lambda: lib.cogdl_hip_actq_quantize(x.data_ptr(), n, bits, 256, 1, 0, q.codes.data_ptr(),
                                                                      q.meta.data_ptr(), stream)),
                ("actq_dequantize", lambda: lib.cogdl_hip_actq_dequantize(q.codes.data_ptr(), q.meta.data_ptr(), n, bits, 256,
                                                                          out.data_ptr(), stream))):
            med, best = _time(fn)
            moved = n * 4 + packed
            gbs = moved / (med * 1e-3) / 1e9
            lines.append("%-22s %-16s %-5d %-13d %-10.4f %-9.4f %-14.0f %.2f" % (name, "%dx%d" % SHAPE, bits, moved, med, best, gbs,
                                                                                gbs / copy))
    y = torch.empty_like(x)
    mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    thresh, scale = actq.drop_params(0.5)
    for name, moved, fn in (
            ("relu_mask", 2 * n * 4 + mask.numel() * 8, lambda: lib.cogdl_hip_relu_mask(x.data_ptr(), n, y.data_ptr(), mask.data_ptr(),
                                                                                       stream)),
            ("drop_apply", 2 * n * 4, lambda: lib.cogdl_hip_drop_apply(x.data_ptr(), n, 1, 0, thresh, scale, y.data_ptr(), stream))):
        med, best = _time(fn)
        gbs = moved / (med * 1e-3) / 1e9
        lines.append("%-22s %-16s %-5s %-13d %-10.4f %-9.4f %-14.0f %.2f" % (name, "%dx%d" % SHAPE, "-", moved, med, best, gbs,
                                                                            gbs / copy))


EPOCH_SCRIPT = r'''
import json, sys
import numpy as np
if not hasattr(np, "int"):
    np.int = int
ROOT, model, epochs = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, ROOT)
from tools import refpkg
refpkg.setup(install=True)
import torch
import cogdl_amd
kw = {}
if model == "actgcn":
    cogdl_amd.install(actnn=True)
    kw["actnn"] = True
ds = refpkg.arxiv_like()
torch.cuda.reset_peak_memory_stats()
res, ms = refpkg.run_experiment(ds, model=model, epochs=epochs, cpu=False, seed=0, hidden_size=256, num_layers=3, dropout=0.5, **kw)
print("RESULT " + json.dumps({"ms": ms, "peak": torch.cuda.max_memory_allocated(), "losses": res["train_losses"]}))
'''


def epoch(lines, epochs):
    import statistics as st

    rows = {}
    for model in ("gcn", "actgcn"):
        proc = subprocess.run([sys.executable, "-c", EPOCH_SCRIPT, ROOT, model, str(epochs)], capture_output=True, text=True,
                              timeout=900)
        got = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")]
        if proc.returncode != 0 or not got:
            raise SystemExit("epoch run of %s failed:\n%s" % (model, proc.stdout[-2000:] + proc.stderr[-4000:]))
        rows[model] = json.loads(got[-1][7:])
    lines.append("")
    lines.append("one training epoch, arxiv-shaped graph (169,343 nodes, 128 features, 40 classes), hidden 256, 3 layers, dropout 0.5,")
    lines.append("the reference's Trainer, %d epochs, median of the train steps after the first two; fresh interpreter per model" % epochs)
    lines.append("model     install            ms / epoch   max_memory_allocated MiB   losses (first, last)")
    for model, flag in (("gcn", "install()"), ("actgcn", "install(actnn=True)")):
        r = rows[model]
        lines.append("%-9s %-18s %-12.2f %-26.1f %.4f, %.4f" % (model, flag, st.median(r["ms"][2:]), r["peak"] / 2 ** 20,
                                                               r["losses"][0], r["losses"][-1]))
    lines.append("actgcn / gcn: time %.2fx, peak memory %.2fx" % (
        st.median(rows["actgcn"]["ms"][2:]) / st.median(rows["gcn"]["ms"][2:]), rows["actgcn"]["peak"] / rows["gcn"]["peak"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actnn_bench.txt"))
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--skip-epoch", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("actnn_bench.py measures on the GPU; none is visible")
    lines = ["activation compression (tools/actnn_bench.py)"]
    kernels(lines)
    if not args.skip_epoch:
        epoch(lines, args.epochs)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

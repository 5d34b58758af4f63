"""Times one forward + backward of hin_scores against the torch gather composition on the same GPU tensors (alternating
rounds, best-to-worst of three windows each), and hin_pairs on the GPU against its host twin; checks that the routes agree.
    python tools/hin2vec_bench.py [OUT.txt]        (needs a GPU; profiles/hin2vec_bench.txt is its output)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cogdl_amd.operators.hin2vec import composition, hin_pairs, hin_scores

dev = "cuda:0"
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(s):
    print(s)
    if out:
        out.write(s + "\n")
        out.flush()


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t) / reps)
    return sorted(best)

say("device: %s" % torch.cuda.get_device_name(0))
N, R, d = 20000, 12, 128
gen = torch.Generator().manual_seed(0)
for B in (1000, 65536):
    Wx = torch.randn(N, d, generator=gen).to(dev).requires_grad_()
    Wr = torch.randn(R, d, generator=gen).to(dev).requires_grad_()
    x, y = (torch.randint(0, N, (B,), generator=gen).to(dev) for _ in range(2))
    r = torch.randint(0, R, (B,), generator=gen).to(dev)
    g = torch.randn(B, generator=gen).to(dev)
    def step(f):
        Wx.grad = Wr.grad = None
        f(Wx, Wr, x, y, r).backward(g)
    hip = lambda: step(lambda *a: hin_scores(*a, check=False))
    ref = lambda: step(composition)
    reps = 300 if B == 1000 else 100
    a, b, a2, b2 = timed(hip, reps), timed(ref, reps), timed(hip, reps), timed(ref, reps)   # alternating
    step(lambda *a_: hin_scores(*a_, check=False)); gx, gr = Wx.grad.clone(), Wr.grad.clone()
    step(composition)
    say("hin_scores fwd+bwd N=%d R=%d d=%d B=%d: HIP %s us | torch composition %s us | max|dWx diff| %.2e max|dWr diff| %.2e"
        % (N, R, d, B, ["%.0f" % (t * 1e6) for t in a + a2], ["%.0f" % (t * 1e6) for t in b + b2],
           float((gx - Wx.grad).abs().max()), float((gr - Wr.grad).abs().max())))

Nw, L = 20000, 80
W = 40 * Nw
walks = torch.randint(0, Nw, (W, L), generator=gen)
walks[::7, 50:] = -1
types = torch.arange(Nw) % 4
wd, td = walks.to(dev), types.to(dev)
def gpu_pairs():
    return hin_pairs(wd, td, 2, 5, seed=3)
gpu_pairs(); torch.cuda.synchronize()
ts = []
for _ in range(3):
    t = time.perf_counter(); res = gpu_pairs(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
del res
t = time.perf_counter(); host = hin_pairs(walks, types, 2, 5, seed=3); th = time.perf_counter() - t
res = gpu_pairs()
same = all(torch.equal(a.cpu(), b) for a, b in zip(res, host))
say("hin_pairs W=%d L=%d hop=2 negative=5 (%d rows): GPU %s ms | host twin (16 threads) %.0f ms | equal %s"
    % (W, L, host[0].numel(), ["%.1f" % (t * 1e3) for t in ts], th * 1e3, same))

"""What the RGCN tests share: the COO generator and the float64 composition of the two laws of cogdl_amd/operators/rgcn.py."""
import torch

N, E, R, UNUSED, BIG = 600, 5000, 7, 4, 2
HUB_DST, HUB_SRC = 7, 11


def coo(seed=5):
    """Unsorted COO on N nodes: the last N / 8 rows stay empty, HUB_DST receives 2500 edges, HUB_SRC sends 1000; type UNUSED
    has no edge and type BIG more than half of them."""
    gen = torch.Generator().manual_seed(seed)
    row = torch.randint(0, N - N // 8, (E,), generator=gen)
    col = torch.randint(0, N, (E,), generator=gen)
    etype = torch.randint(0, R, (E,), generator=gen)
    where = torch.randperm(E, generator=gen)
    row[where[:2500]] = HUB_DST
    col[where[2000:3000]] = HUB_SRC
    etype[where[1000:3700]] = BIG
    etype[etype == UNUSED] = UNUSED + 1
    return row, col, etype


def basis_law(x, alpha, row, col, etype, w, n):
    """Z[v, b, :] = sum_e w_e alpha[t_e, b] x[col_e, :], one index_add_ per basis."""
    xs = x[col] if w is None else x[col] * w.unsqueeze(-1)
    return torch.stack([torch.zeros(n, x.shape[1], dtype=x.dtype).index_add_(0, row, alpha[etype, b].unsqueeze(-1) * xs)
                        for b in range(alpha.shape[1])], dim=1)


def bdd_law(x, W, row, col, etype, w, n):
    """H[v, b*bo:(b+1)*bo] = sum_e w_e x[col_e, b*bi:(b+1)*bi] @ W[t_e, b]."""
    n_blocks, bi, bo = W.shape[1:]
    msg = torch.einsum("ebi,ebio->ebo", x[col].view(-1, n_blocks, bi), W[etype]).reshape(-1, n_blocks * bo)
    if w is not None:
        msg = msg * w.unsqueeze(-1)
    return torch.zeros(n, n_blocks * bo, dtype=x.dtype).index_add_(0, row, msg)


def reference(law, a, b, row, col, etype, w, n, G):
    """float64 on the CPU: (output, grad a, grad b) of the law and of the same law on absolute values -- every term is a
    product, so the second triple is the per-element sum of |summands| that the bound scales with."""
    out = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        a64, b64 = f(a).requires_grad_(), f(b).requires_grad_()
        res = law(a64, b64, row, col, etype, None if w is None else f(w), n)
        res.backward(f(G))
        out.append((res.detach(), a64.grad, b64.grad))
    return out


def within(got, want, scale):
    """|got - want| <= 1e-5 * sum |summands| per element (tests/test_message_ops_gpu.py::test_hub_destinations)."""
    return bool((torch.abs(got.double().cpu() - want) <= 1e-5 * scale).all())

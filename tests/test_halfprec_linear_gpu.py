"""The 16-bit MFMA product tall_skinny_matmul_16 (csrc/linear_fwd16.hip; bf16 and f16 results, x in fp32 -- rounded to 16 bits in
registers -- or already 16-bit), held to "fp32 accumulation of exact products, bias added in fp32, rounded once, to nearest even".
tests/test_linear_gpu.py allows a whole ulp plus 2e-6 of the sum of magnitudes, which sees neither a truncating conversion nor
round-half-away.

  * Integer data: x and W in {-4 .. 4}, the bias a multiple of 0.5 -- every product and every fp32 partial sum is exact, whatever
    order the MFMA adds in, so the result has to EQUAL the float64 result cast once (hp.assert_exact; no slack at all).  The bias of
    the columns c % 4 == 0, 1 is +-(1100.5 + 3 c): every such output needs rounding, and in f16 (spacing 1 there) every one is a
    TIE; c % 4 == 3 has 300 + c, which puts the sums where bf16's spacing is 2 and every odd one is a tie; c % 4 == 2 has none
    (K = 602 and K = 1000 reach sums of several hundred by themselves).  Round-half-away or truncation fails on the first tie.
  * Random data: hp.bound(want, scale, k + 1, dtype) -- the standard bound of tests/_halfprec.py; its doubled `terms` also covers an
    MFMA that does not round each internal addition to nearest.  It replaces the "one ulp of slack".  For f16 at K >= 300 the fp32
    slack (2 K + 4) 2^-24 x scale outgrows half an ulp (2^-12 of the result), so there the bound by itself could not tell the store's
    rounding: those shapes are carried by the integer test.
  * The in-register rounding of fp32 x: W a 0 / 1 selection matrix, no bias -- out[:, c] has to be x[:, col(c)] cast by torch,
    on exact ties of both parities and both signs (1 + 2^-8, 1 + 3 * 2^-8 for bf16; 1 + 2^-11, 1 + 3 * 2^-11 for f16), just beside
    them, at other exponents, and on random values.
Shapes: the bf16 list of tests/test_linear_gpu.py with every edge kept -- ragged last macro-step (602), one row, one column, rows
that are no multiple of the row tile (4097, 31, 33), 16-bit rows of odd length (33: declined, the caller keeps torch's product), W as
[N, K] and as [K, N].  Not reached: K > 1024 (declined: W beyond the kernel's LDS budget), N > 64 (declined)."""
import numpy as np
import pytest
import torch

import _halfprec as hp
from cogdl_amd.linear import tall_skinny_matmul_16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
X_DTYPE = pytest.mark.parametrize("x_dtype", [torch.float32, "half"], ids=["x-f32", "x-16bit"])
SHAPES = pytest.mark.parametrize("rows,k,n,transposed_w", [
    (5000, 602, 64, False), (5000, 64, 41, False), (4097, 128, 64, True), (1000, 33, 7, False), (33, 34, 1, False),
    (31, 16, 64, False), (1, 8, 3, True), (300, 1000, 33, False), (64, 2, 2, False)])


def _declined(x, w, bias, transposed_w, half):
    """16-bit rows of an odd number of elements are not covered: the entry says so (None) and the caller uses torch's product."""
    if x.dtype == torch.float32 or x.shape[1] % 2 == 0:
        return False
    assert tall_skinny_matmul_16(x, w, bias, transposed_w, half) is None
    return True


@HALF
@X_DTYPE
@SHAPES
def test_integer_data_is_the_exact_product_rounded_once(rows, k, n, transposed_w, x_dtype, half):
    x_dtype = half if x_dtype == "half" else x_dtype
    gen = torch.Generator().manual_seed(rows + 7 * k + n)
    x = torch.randint(-4, 5, (rows, k), generator=gen).float()
    w = torch.randint(-4, 5, (n, k) if transposed_w else (k, n), generator=gen).float()
    c = torch.arange(n, dtype=torch.float32)
    bias = torch.stack([1100.5 + 3 * c, -(1100.5 + 3 * c), torch.zeros(n), 300.0 + c])[torch.arange(n) % 4, torch.arange(n)]
    xd = x.to(DEV).to(x_dtype)
    if _declined(xd, w.to(DEV), bias.to(DEV), transposed_w, half):
        return
    b64 = w.double().t() if transposed_w else w.double()
    want = (x.double() @ b64 + bias.double()).numpy()
    scale = (x.double().abs() @ b64.abs() + bias.double().abs()).numpy()
    cast = torch.from_numpy(want).to(half).double().numpy()
    rounded = cast != want
    ties = np.abs(cast - want) == 0.5 * hp.ulp(want, half)
    print("outputs that need rounding: %.3f, ties: %.3f" % (rounded.mean(), ties.mean()))
    assert rounded.mean() >= 0.05  # the check is not vacuous
    for wd in (w.to(DEV), w.to(DEV).to(half)):  # (weights already in the 16-bit type: autocast's cached cast)
        got = tall_skinny_matmul_16(xd, wd, bias.to(DEV), transposed_w, half)
        assert got is not None and got.shape == (rows, n)
        hp.assert_exact(got, want, scale, half, "(%d, %d, %d)" % (rows, k, n))


@HALF
@X_DTYPE
@SHAPES
def test_random_data_within_half_an_ulp(rows, k, n, transposed_w, x_dtype, half):
    x_dtype = half if x_dtype == "half" else x_dtype
    gen = torch.Generator().manual_seed(rows + 7 * k + n)
    x = torch.randn(rows, k, generator=gen)
    w = torch.randn((n, k) if transposed_w else (k, n), generator=gen)
    x[:, 0] += 3.0  # asymmetric: operand permutations show
    x[:, -1] -= 1.5
    bias = torch.randn(n, generator=gen)
    xd = x.to(DEV).to(x_dtype)
    if _declined(xd, w.to(DEV), bias.to(DEV), transposed_w, half):
        return
    got = tall_skinny_matmul_16(xd, w.to(DEV), bias.to(DEV), transposed_w, half)
    assert got is not None and got.dtype == half and got.shape == (rows, n)
    x64, w64 = x.to(half).double(), w.to(half).double()
    b64 = w64.t() if transposed_w else w64
    want = (x64 @ b64 + bias.double()).numpy()
    scale = (x64.abs() @ b64.abs() + bias.double().abs()).numpy()
    hp.assert_close(got, want, scale, k + 1, half, "(%d, %d, %d)" % (rows, k, n))
    assert torch.equal(tall_skinny_matmul_16(xd, w.to(DEV).to(half), bias.to(DEV), transposed_w, half), got)


@HALF
@pytest.mark.parametrize("k,n,transposed_w", [(64, 64, False), (33, 7, False), (16, 64, True), (8, 3, True), (2, 2, False)])
def test_fp32_x_is_rounded_to_nearest_even_in_registers(k, n, transposed_w, half):
    eps = [2.0 ** -8, 2.0 ** -11]  # half an ulp of 1 in bf16 / f16: 1 + eps ties to the even 1, 1 + 3 eps to the even 1 + 4 eps
    base = []
    for e in eps:
        base += [1 + e, 1 + 3 * e, 1 + 5 * e, 1 + 7 * e, 1 + e + 2.0 ** -20, 1 + e - 2.0 ** -20, 1 + 3 * e + 2.0 ** -20, 1 + 3 * e - 2.0 ** -20,
                 2 - e, 2 - e - 2.0 ** -20]
    special = torch.tensor([s * v * m for v in base for s in (1.0, -1.0) for m in (1.0, 2.0 ** 10, 2.0 ** -10, 0.25)])
    assert torch.equal(special.double(), special.float().double())  # all exact in fp32
    rows = 1024
    gen = torch.Generator().manual_seed(k + n)
    x = torch.randn(rows, k, generator=gen)
    pos = torch.randint(0, special.numel(), (rows, k), generator=gen)
    x = torch.where(torch.rand(rows, k, generator=gen) < 0.5, special.float()[pos], x)
    x[:special.numel(), 0] = special.float()  # every special value at least once
    cols = (7 * torch.arange(n) + 3) % k
    w = torch.zeros(k, n)
    w[cols, torch.arange(n)] = 1.0
    want = x[:, cols].to(half)
    assert float((want.double() != x[:, cols].double()).double().mean()) > 0.5  # most values need rounding
    got = tall_skinny_matmul_16(x.to(DEV), (w.t().contiguous() if transposed_w else w).to(DEV), None, transposed_w, half)
    assert got is not None and got.dtype == half
    assert torch.equal(got.cpu(), want), "first mismatch at %s" % (torch.nonzero(got.cpu() != want)[:1].tolist(),)

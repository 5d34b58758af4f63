"""Dense operands that start mid-allocation, for the CPU and GPU tests of operand offsets (tests/test_operand_offsets_cpu.py,
tests/test_operand_offsets_gpu.py).

A contiguous tensor whose data_ptr() is only element-aligned is ordinary torch: a slice of a flat parameter buffer, a narrow of
a packed batch, an upstream gradient that is such a view.  The kernels pick their vector width from the address, so such an
operand runs another instantiation than a fresh tensor of the same values.

    shifted(t, elems, pad=8, device=None) -> (view, guard)
        view: contiguous, t's values, view.data_ptr() % 16 == (elems * t.element_size()) % 16, inside a fresh allocation with
        at least `pad` sentinel elements in front of and behind it.
    guards_intact(guard) -> bool
        both pads still hold the sentinel, bit for bit: asserted after every call for every operand the call WRITES (the
        narrow tails of a vector store are where a kernel writes past a view).
    strided(t) -> the same values as a non-contiguous view (a column slice of a wider tensor).
"""
import torch

SENTINEL = -12345.0  # finite: a read past the view then shows as a wrong number, not as a NaN a max or a mask may swallow
# (the 16-bit formats round it; the pads are filled in the tensor's own dtype and compared with what was filled)


class Guard:
    __slots__ = ("store", "lo", "hi", "want_lo", "want_hi")

    def __init__(self, store, lo, hi):
        self.store, self.lo, self.hi = store, lo, hi
        self.want_lo, self.want_hi = store[:lo].clone(), store[hi:].clone()


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.numel() else t.new_zeros(0, dtype=torch.uint8)


def shifted(t, elems, pad=8, device=None):
    """-> (view, guard): see the module docstring.  The allocation is pad + 16 + t.numel() + pad elements long at the most: the
    view is moved up by less than 16 bytes so that its address modulo 16 is elems * element_size whatever the allocator
    returns (torch's allocators return 64 bytes and more of alignment; the rounding is there so that the assertion below
    does not depend on it)."""
    device = t.device if device is None else torch.device(device)
    es = t.element_size()
    want = (elems * es) % 16
    per16 = 16 // es
    store = torch.full((pad + per16 + t.numel() + pad + per16,), SENTINEL, dtype=t.dtype, device=device)
    start = pad
    while (store.data_ptr() + start * es) % 16 != want:
        start += 1
        assert start < pad + 2 * per16, "an allocation that is not element-aligned"
    view = store[start:start + t.numel()].view(t.shape)
    view.copy_(t.detach())
    assert view.is_contiguous() and view.data_ptr() % 16 == want and tuple(view.shape) == tuple(t.shape)
    guard = Guard(store, start, start + t.numel())
    assert guard.lo >= pad and store.numel() - guard.hi >= pad
    return view, guard


def guards_intact(guard):
    """Both pads of the allocation behind a shifted view, bit for bit what they were filled with."""
    g = guard
    return (torch.equal(_bits(g.store[:g.lo]), _bits(g.want_lo)) and torch.equal(_bits(g.store[g.hi:]), _bits(g.want_hi)))


def strided(t):
    """t's values as a non-contiguous view: the even columns of a tensor twice as wide in the last dimension (odd columns hold
    the sentinel).  A 0-d or empty tensor cannot be non-contiguous and is refused."""
    assert t.dim() >= 1 and t.numel() > 1
    wide = torch.full(tuple(t.shape[:-1]) + (2 * t.shape[-1],), SENTINEL, dtype=t.dtype, device=t.device)
    view = wide[..., ::2]
    view.copy_(t.detach())
    assert not view.is_contiguous() and torch.equal(view, t.detach())
    return view

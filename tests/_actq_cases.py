"""Shared cases of the activation-compression tests (tests/test_actq_cpu.py on the host twin, tests/test_actq_gpu.py against
it): the sizes at which the kernels take another path -- below a quadruple, below / at / above a mask word and a group, a
partial tile, more than one workgroup with a ragged end -- every width and every group size."""
import torch

SIZES = (1, 3, 63, 64, 255, 256, 257, 1000, 256 * 64 + 5)
BITS = (1, 2, 4, 8)
GROUPS = (64, 128, 256)
SEED, CALL = 0x5EED0ACD, 7

_INPUTS = {}


def tensor(n):
    """float32 [n], standard normal with a few exact zeros, a -0 and a run of equal values; one per size, never modified."""
    x = _INPUTS.get(n)
    if x is None:
        x = torch.randn(n, generator=torch.Generator().manual_seed(1000 + n))
        if n > 10:
            x[3], x[4] = 0.0, -0.0
        if n > 700:
            x[512:640] = 0.75  # a constant group at every group size up to 128
        _INPUTS[n] = x
    return x


def group_index(n, group):
    return torch.arange(n) // group


def unpack(codes, n, bits):
    """The law's storage: element i at bit bits * (i % (32 / bits)) of word i / (32 / bits) -> int64 [n]."""
    per = 32 // bits
    words = codes.cpu().to(torch.int64) & 0xFFFFFFFF
    i = torch.arange(n)
    return (words[i // per] >> (bits * (i % per))) & (2 ** bits - 1)


def mask_bits(mask, n):
    i = torch.arange(n)
    return ((mask.cpu()[i // 64] >> (i % 64)) & 1).bool()

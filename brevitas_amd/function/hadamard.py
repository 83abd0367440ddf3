"""The fast Walsh-Hadamard transform along the last dimension, in blocks: y = scale * (I (x) H_b) x.

The online rotation of QuaRot / SpinQuant style quantization, and the product of HadamardClassifier.  H_b is the
Sylvester (natural-order) +-1 matrix; the arithmetic is defined in include/bvq.h ("Hadamard transform"): float32 butterfly
stages h = 1, 2 .. b / 2 in ascending order, one multiply by float32(scale), one rounding to the tensor's dtype.  A device
tensor takes the HIP kernel (libbvq.so, bvq_hadamard), everything else the same stages composed of torch ops
(brevitas_amd._aten.hadamard); the two routes give the same bits.
"""
import math

import torch
from torch import Tensor
from torch.autograd import Function

from .. import _aten
from .. import _native as nat
from .. import config

__all__ = ['hadamard_transform', 'hadamard_matrix', 'default_block_size']

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_ROW_MAX_BYTES = 32768  # the longest row the row kernels hold (bvq_row_shifted_max_row_bytes)


def default_block_size(n: int) -> int:
    """the largest power of two dividing n"""
    n = int(n)
    return n & -n


def _check_block(block_size, n):
    b = default_block_size(n) if block_size is None else int(block_size)
    if b < 2 or b & (b - 1) or n % b:
        raise ValueError('hadamard_transform: block_size %d must be a power of two, at least 2, that divides the last '
                         'dimension %d' % (b, n))
    return b


def _row_view(n, block, itemsize):
    """c with block | c | n, c * itemsize a multiple of 16 and at most the kernel's row limit, the largest such; or None.
    The transform is block-diagonal, so [rows, n] is [rows * n / c, c] to it."""
    m = n // block
    for t in range(min(m, _ROW_MAX_BYTES // (block * itemsize)), 0, -1):
        if m % t == 0 and (block * t * itemsize) % 16 == 0:
            return block * t
    return None


def _apply(x, block, scale):
    x = x.contiguous()
    n = x.shape[-1]
    if x.is_cuda and config.FUSED_PATHS and x.numel() > 0:
        c = _row_view(n, block, x.element_size())
        if c is not None and nat.hadamard_supported(x, x.numel() // c, c, block):
            return nat.hadamard(x, x.numel() // c, c, block, scale)
    return _aten.hadamard(x, block, scale)


class _HadamardFn(Function):
    """One node for both routes.  The transform is symmetric: the backward is the forward on the incoming gradient, the
    same stages in the same order, hence the bits of a direct call."""

    @staticmethod
    def forward(ctx, x, block, scale):
        ctx.block, ctx.scale = block, scale
        return _apply(x, block, scale)

    @staticmethod
    def backward(ctx, grad_y):
        return _apply(grad_y, ctx.block, ctx.scale), None, None


def hadamard_transform(x: Tensor, block_size=None, scale=None) -> Tensor:
    """scale * (I (x) H_block_size) x along the last dimension of x (any leading shape; float32, bfloat16, float16).
    block_size: a power of two >= 2 dividing x.shape[-1]; None: the largest one.  scale: None: 1 / sqrt(block_size), the
    orthonormal transform, which is its own inverse."""
    if x.dtype not in _DTYPES:
        raise TypeError('hadamard_transform: dtype %s (float32, bfloat16, float16)' % x.dtype)
    if x.dim() < 1:
        raise ValueError('hadamard_transform: a tensor with at least one dimension')
    block = _check_block(block_size, x.shape[-1])
    scale = 1.0 / math.sqrt(block) if scale is None else float(scale)
    return _HadamardFn.apply(x, block, scale)


def hadamard_matrix(n: int, dtype=torch.float32, device=None) -> Tensor:
    """the Sylvester +-1 matrix of order n (a power of two): H_1 = [1], H_2n = [[H_n, H_n], [H_n, -H_n]]"""
    n = int(n)
    if n < 1 or n & (n - 1):
        raise ValueError('hadamard_matrix: order %d is no power of two' % n)
    h = torch.ones(1, 1, dtype=dtype, device=device)
    while h.shape[0] < n:
        h = torch.cat((torch.cat((h, h), dim=1), torch.cat((h, -h), dim=1)), dim=0)
    return h

"""Hadamard rotations as layers: the transform itself, a layer fed its rotated input (the RotatedModule of later Brevitas
releases), and the reference's HadamardClassifier (B/nn/hadamard_classifier.py) on the fast transform.
"""
import math

import torch
import torch.nn.functional as F

from brevitas_amd.function.hadamard import hadamard_transform
from brevitas_amd.function.ops import max_int
from brevitas_amd.function.ops_ste import ceil_ste

__all__ = ['HadamardRotation', 'RotatedModule', 'HadamardClassifier']


class HadamardRotation(torch.nn.Module):
    """hadamard_transform(x, block_size, scale) along the last dimension"""

    def __init__(self, block_size=None, scale=None):
        super().__init__()
        self.block_size, self.scale = block_size, scale

    def forward(self, x):
        return hadamard_transform(x, self.block_size, self.scale)

    def extra_repr(self):
        return 'block_size=%s, scale=%s' % (self.block_size, self.scale)


class RotatedModule(torch.nn.Module):
    """layer(hadamard_transform(x, block_size)): the online half of a rotation whose other half is merged into the
    layer's weight (graph/rotate.py: insert_online_rotation).  The layer stays a registered sub-module, so whatever
    walks named_modules() -- gptq_mode, gpfq_mode, awq_mode, learned_round_mode, the calibration modes -- still finds
    it, and sees the rotated input."""

    def __init__(self, layer: torch.nn.Module, block_size=None):
        super().__init__()
        self.layer = layer
        self.block_size = block_size

    def forward(self, x):
        return self.layer(hadamard_transform(x, self.block_size))

    def extra_repr(self):
        return 'block_size=%s' % (self.block_size,)


class HadamardClassifier(torch.nn.Module):
    """-scale * (H_sz[:out, :in] @ (x / (||x||_F + eps))), sz the next power of two of max(in, out) (Hoffer et al.
    2018; B/nn/hadamard_classifier.py:21-71 without its QuantTensor plumbing).  The reference multiplies by a dense
    `proj` buffer; here the input is zero-padded to sz, transformed once (unscaled) and sliced, so there is no such
    buffer and the state dict holds `scale` alone -- what the reference's state_dict() override leaves."""

    def __init__(self, in_channels, out_channels, fixed_scale=False):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.size = 1 << (max(self.in_channels, self.out_channels, 2) - 1).bit_length()
        init_scale = 1. / math.sqrt(self.out_channels)
        if fixed_scale:
            self.register_buffer('scale', torch.tensor(init_scale))
        else:
            self.scale = torch.nn.Parameter(torch.tensor(init_scale))
        self.eps = 1e-8

    def forward(self, x):
        norm = x.norm(p='fro', keepdim=True) + self.eps
        out = F.pad(x / norm, (0, self.size - self.in_channels))
        out = hadamard_transform(out, self.size, 1.0)[..., :self.out_channels]
        return -self.scale * out

    def max_output_bit_width(self, input_bit_width):
        max_input_val = max_int(bit_width=input_bit_width, narrow_range=False, signed=False)
        max_output_val = max_input_val * self.in_channels
        return ceil_ste(torch.log2(max_output_val))

"""Merging Hadamard rotations into weights (QuaRot, SpinQuant; rotation equalization of later Brevitas releases).

R = I (x) H_b / sqrt(b) is symmetric and orthogonal, so a linear layer fed R x computes the same as the layer with W R
fed x, and a layer whose weight is R W (bias R bias) emits R y.  Merged into a weight a rotation is free; what is not
merged is paid on every forward by the transform kernel (nn.RotatedModule).  A rotation spreads a few outlier channels
over all channels of a block before a quantizer sees them.

Linear layers only (QuantLinear, torch.nn.Linear), and before quantizing: a frozen layer's weight holds codes.
"""
import torch

from brevitas_amd.function.hadamard import hadamard_transform

__all__ = ['merge_input_rotation', 'merge_output_rotation', 'rotate_pair', 'insert_online_rotation']


def _check(layer, what):
    if not isinstance(layer, torch.nn.Linear):  # QuantLinear is one
        raise NotImplementedError('%s: Linear and QuantLinear layers only, not %s' % (what, type(layer).__name__))
    if getattr(layer, '_buffers', {}).get('frozen_weight_scale') is not None:
        raise RuntimeError('%s: the layer is frozen (frozen_weight_scale): its weight holds quantized codes; rotate '
                           'before quantizing' % what)


def _rotate_last(t, block_size):
    """t R along the last dimension, computed in float32 and stored in t's dtype"""
    return hadamard_transform(t.detach().to(torch.float32), block_size).to(t.dtype)


@torch.no_grad()
def merge_input_rotation(layer, block_size=None):
    """W <- W R: the layer now expects R x where it expected x"""
    _check(layer, 'merge_input_rotation')
    layer.weight.copy_(_rotate_last(layer.weight, block_size))
    return layer


@torch.no_grad()
def merge_output_rotation(layer, block_size=None):
    """W <- R W, bias <- R bias: the layer now emits R y where it emitted y"""
    _check(layer, 'merge_output_rotation')
    layer.weight.copy_(_rotate_last(layer.weight.t(), block_size).t())
    if layer.bias is not None:
        layer.bias.copy_(_rotate_last(layer.bias, block_size))
    return layer


def rotate_pair(producer, consumer, block_size=None):
    """the output side of `producer` and the input side of `consumer`: with only linear maps between the two, the
    composition is unchanged, and what flows between them is rotated"""
    _check(producer, 'rotate_pair')
    _check(consumer, 'rotate_pair')
    if producer.out_features != consumer.in_features:
        raise ValueError('rotate_pair: the producer emits %d features, the consumer takes %d'
                         % (producer.out_features, consumer.in_features))
    merge_output_rotation(producer, block_size)
    merge_input_rotation(consumer, block_size)


def insert_online_rotation(model, name, block_size=None):
    """merge the input rotation into the layer `name` of model and put RotatedModule(layer, block_size) in its place:
    the float function of the model is unchanged, the layer's input quantizer and weight quantizer see rotated
    tensors -> the RotatedModule"""
    from brevitas_amd.nn import RotatedModule
    if not name:
        raise ValueError('insert_online_rotation: the name of a sub-module of the model')
    parent_name, _, child = name.rpartition('.')
    parent = model.get_submodule(parent_name) if parent_name else model
    layer = getattr(parent, child)
    merge_input_rotation(layer, block_size)
    rotated = RotatedModule(layer, block_size)
    setattr(parent, child, rotated)
    return rotated

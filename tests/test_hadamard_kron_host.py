"""Hadamard rotations of order K * 2^n, K = 12, 20, 28, 36, without a device: the Paley matrices, the composed route against
a float64 dense product by kron(H_K, H_P), the inverse, the backward, the rotation merges and the refusals."""
import math

import pytest
import torch

from brevitas_amd import _native as nat
from brevitas_amd.function.hadamard import hadamard_matrix, hadamard_transform, paley_hadamard_matrix
from brevitas_amd.graph import insert_online_rotation, rotate_pair
from brevitas_amd.nn import QuantLinear, RotatedModule

BASES = (12, 20, 28, 36)
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
ROUND = {'f32': 2.0 ** -23, 'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}  # the output rounding: r * |y64|


@pytest.mark.parametrize('k', BASES)
def test_paley_matrix(k):
    h = paley_hadamard_matrix(k, torch.float64)
    assert h.shape == (k, k) and torch.equal(h.abs(), torch.ones(k, k, dtype=torch.float64))
    assert torch.equal(h @ h.t(), k * torch.eye(k, dtype=torch.float64))
    assert torch.equal(h, h.t()) == (k in (28, 36))
    with pytest.raises(ValueError, match='order %d' % k):
        hadamard_matrix(k)  # the Sylvester form still has no such order


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('p', [8, 64])
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('k', BASES)
def test_composed_route_against_the_dense_product(k, dt, p, transpose):
    """the bound of test_composed_route_against_the_dense_sylvester_product with log2 P + K additions and the multiply:
    1.01 * scale * (log2 P + K + 1) * 2^-24 * ||x_block||_1 + r * |y64|"""
    b = k * p
    torch.manual_seed(b)
    x = torch.randn(4, 2 * b).to(DTYPES[dt])
    scale = 1.0 / math.sqrt(b)
    h = torch.kron(paley_hadamard_matrix(k, torch.float64), hadamard_matrix(p, torch.float64))
    h = h.t() if transpose else h
    y = hadamard_transform(x, b, base=k, transpose=transpose)
    assert y.dtype == x.dtype and y.shape == x.shape
    # leading shape, default block (the largest K * 2^n dividing 2 b is 2 b)
    assert torch.equal(hadamard_transform(x.reshape(2, 2, 2 * b), base=k).reshape(4, 2 * b),
                       hadamard_transform(x, 2 * b, base=k))

    def dense(t, m):
        return (scale * (t.double().reshape(4, 2, b) @ m.t())).reshape(4, 2 * b)

    def bound(t, t64):
        l1 = t.double().abs().reshape(4, 2, b).sum(dim=-1, keepdim=True).expand(4, 2, b).reshape(4, 2 * b)
        return 1.01 * scale * (math.log2(p) + k + 1) * 2.0 ** -24 * l1 + ROUND[dt] * t64.abs()

    y64 = dense(x, h)
    assert ((y.double() - y64).abs() <= bound(x, y64)).all()
    # the inverse: the same bound on the second call, and the first call's error e carried through the orthonormal
    # inverse, every element of R' e being at most ||e_block||_2
    back = hadamard_transform(y, b, base=k, transpose=not transpose)
    back64 = dense(y, h.t())
    carried = bound(x, y64).reshape(4, 2, b).norm(dim=-1, keepdim=True).expand(4, 2, b).reshape(4, 2 * b)
    assert ((back.double() - x.double()).abs() <= bound(y, back64) + carried).all()


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('k', BASES)
def test_backward_is_the_transpose_call_on_the_gradient(k, dt):
    b = k * 16
    torch.manual_seed(k)
    x = torch.randn(3, 2 * b).to(DTYPES[dt]).requires_grad_(True)
    g = torch.randn(3, 2 * b).to(DTYPES[dt])
    hadamard_transform(x, b, base=k).backward(g)
    assert torch.equal(x.grad, hadamard_transform(g, b, base=k, transpose=True))
    x.grad = None
    hadamard_transform(x, b, base=k, transpose=True).backward(g)
    assert torch.equal(x.grad, hadamard_transform(g, b, base=k))


def test_rotation_merges_with_base_12_leave_a_float_model_unchanged():
    """with R and R' swapped in a merge the outputs differ by O(1); tolerance of the existing rotation tests' closing checks"""
    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(40, 96), torch.nn.Linear(96, 20))
    x = torch.randn(9, 40)
    want = model(x).detach()
    mid = model[0](x).detach()
    rotate_pair(model[0], model[1], 48, base=12)
    torch.testing.assert_close(model(x).detach(), want, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(model[0](x).detach(), hadamard_transform(mid, 48, base=12), rtol=1e-4, atol=1e-5)
    model = torch.nn.Sequential(torch.nn.Linear(24, 96), torch.nn.ReLU(), QuantLinear(96, 12))
    want = model(x[:, :24]).detach()
    inner = model[2]
    rot = insert_online_rotation(model, '2', base=12)
    assert isinstance(rot, RotatedModule) and rot.layer is inner and (rot.block_size, rot.base) == (None, 12)
    torch.testing.assert_close(model(x[:, :24]).detach(), want, rtol=1e-4, atol=1e-5)


def test_refusals():
    x = torch.randn(2, 192)
    for bad in (36, 72, 6, 384):  # 3 * 12, 6 * 12: no power of two; below the base; does not divide 192
        with pytest.raises(ValueError, match=r'%d\b.*\b12\b.*\b192\b' % bad):
            hadamard_transform(x, bad, base=12)
    with pytest.raises(ValueError, match='base 44'):
        hadamard_transform(x, base=44)
    with pytest.raises(ValueError, match=r'\b20\b.*\b192\b'):
        hadamard_transform(x, base=20)  # 20 does not divide 192
    with pytest.raises(ValueError, match='24'):
        hadamard_transform(torch.randn(2, 24), 6)  # without a base nothing changes
    assert torch.equal(hadamard_transform(x, base=12), hadamard_transform(x, 192, base=12))
    assert torch.equal(hadamard_transform(x, 64, transpose=True), hadamard_transform(x, 64))
    kron, sup = nat.lib.bvq_hadamard_kron, nat.lib.bvq_hadamard_kron_supported

    def refused(rc, word, dtype, xp, rows, cols, base, block, yp):
        assert kron(dtype, xp, rows, cols, base, block, 0, 1.0, yp, None) == rc and word in nat.last_error(), \
            nat.last_error()
        assert sup(dtype, rows, cols, base, block, xp, yp) == 0

    refused(-1, 'base 24', nat.BF16, None, 4, 192, 24, 192, None)
    refused(-1, 'power of two', nat.BF16, None, 4, 288, 12, 72, None)
    refused(-1, 'power of two', nat.BF16, None, 4, 192, 12, 6, None)
    refused(-1, 'divide', nat.BF16, None, 4, 288, 12, 192, None)
    refused(-2, '36864 bytes', nat.BF16, None, 4, 18432, 36, 4608, None)  # a row above 32 KiB
    refused(-2, 'sub-row of 8 bytes', nat.BF16, None, 4, 96, 12, 48, None)  # P = 4 bfloat16
    refused(-2, '16-byte', nat.BF16, 4096 + 8, 4, 96, 12, 96, 4096)  # a misaligned pointer value
    refused(-2, '16-byte', nat.BF16, 4096, 4, 96, 12, 96, 4096 + 2)
    refused(-1, 'dtype', 7, None, 4, 96, 12, 96, None)
    refused(-1, 'null', nat.F32, None, 4, 96, 12, 96, None)
    refused(-1, 'rows', nat.F32, None, 0, 96, 12, 96, None)

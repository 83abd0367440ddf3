"""The Hadamard transform kernel (bvq_hadamard) against the composed route run on the CPU: BIT equality.  Both compute
the definition of include/bvq.h ("Hadamard transform") -- float32 butterfly stages in ascending order, one multiply, one
rounding -- so no tolerance is needed on the device.  The unit-vector cases are independent of the composed route: they
compare with the rows of the Sylvester matrix and localise a wrong pairing or sign to a stage class."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# chunks (16 bytes) per row for each geometry of the row walk: a ragged row and the geometry's top
GEOMETRY = {'one_wave': (3, 96, 128), 'depth2': (384, 512), 'depth8': (1536, 2048)}
ROWS = 5  # no multiple of the four rows per workgroup of the one-wave geometry


def vec(dt):
    return 16 // torch.empty(0, dtype=dt).element_size()


def blocks_of(cols):
    top = cols & -cols
    return [1 << i for i in range(1, top.bit_length())]


def cpu_route(x, block, scale=None):
    from brevitas_amd.function.hadamard import hadamard_transform
    assert not x.is_cuda
    return hadamard_transform(x, block, scale)


def sylvester_row(k, n):
    """row k of the Sylvester matrix of order n: (-1) ** popcount(k & j)"""
    b = torch.arange(n, dtype=torch.int64) & k
    parity = torch.zeros(n, dtype=torch.int64)
    while int(b.max()) > 0:
        parity ^= b & 1
        b >>= 1
    return (1 - 2 * parity).to(torch.float32)


@pytest.fixture
def kernel_calls(monkeypatch):
    """counts the launches of bvq_hadamard made through the binding"""
    from brevitas_amd import _native as nat
    calls = []
    real = nat.hadamard

    def counted(*args, **kwargs):
        calls.append(args[1:4])
        return real(*args, **kwargs)

    monkeypatch.setattr(nat, 'hadamard', counted)
    return calls


@pytest.mark.parametrize('geometry', list(GEOMETRY))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_size_sweep(dt, geometry):
    """every power-of-two block from 2 to the largest dividing the row, rows whose last load is ragged"""
    from brevitas_amd import _native as nat
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(123456)
    for chunks in GEOMETRY[geometry]:
        cols = chunks * vec(dtype)
        x = torch.randn(ROWS, cols, generator=gen).to(dtype)
        xd = x.to(DEV)
        for b in blocks_of(cols):
            assert nat.hadamard_supported(xd, ROWS, cols, b), (cols, b)
            scale = b ** -0.5
            got = nat.hadamard(xd, ROWS, cols, b, scale).cpu()
            want = cpu_route(x, b)
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), \
                (dt, cols, b, int((got != want).sum()), (got.float() - want.float()).abs().max().item())


@pytest.mark.parametrize('geometry', list(GEOMETRY))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_unit_vectors(dt, geometry):
    """scale 1 at the geometry's largest block: e_k gives row k of the matrix exactly"""
    from brevitas_amd import _native as nat
    dtype = DTYPES[dt]
    v = vec(dtype)
    b = GEOMETRY[geometry][-1] * v
    ks = [1, v, 64 * v, b // 2, b - 1]
    x = torch.zeros(len(ks), b, dtype=dtype)
    for r, k in enumerate(ks):
        x[r, k] = 1.0
    got = nat.hadamard(x.to(DEV), len(ks), b, b, 1.0).cpu()
    for r, k in enumerate(ks):
        assert torch.equal(got[r].float(), sylvester_row(k, b)), (dt, b, k)


@pytest.mark.parametrize('dt', list(DTYPES))
def test_in_place(dt):
    from brevitas_amd import _native as nat
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(7)
    for chunks, b in ((96, 32), (512, 512 * vec(dtype)), (1536, 512 * vec(dtype))):
        cols = chunks * vec(dtype)
        x = torch.randn(ROWS, cols, generator=gen).to(dtype).to(DEV)
        out = nat.hadamard(x, ROWS, cols, b, b ** -0.5)
        y = x.clone()
        assert nat.hadamard(y, ROWS, cols, b, b ** -0.5, out=y) is y
        assert torch.equal(y.view(torch.uint8), out.view(torch.uint8))


@pytest.mark.parametrize('b', [16384, 32])
def test_last_dimension_above_the_row_limit_is_viewed_again(b, kernel_calls):
    from brevitas_amd.function.hadamard import hadamard_transform
    x = torch.randn(3, 49152, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
    got = hadamard_transform(x.to(DEV), b).cpu()
    assert len(kernel_calls) == 1 and kernel_calls[0][1] == 16384  # [9, 16384]: the kernel, not the composed route
    assert torch.equal(got.view(torch.uint8), cpu_route(x, b).view(torch.uint8))


def test_non_contiguous_misaligned_and_fused_paths_off(kernel_calls):
    from brevitas_amd import config
    from brevitas_amd.function.hadamard import hadamard_transform
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(6, 1024, generator=gen).to(torch.bfloat16)
    want = cpu_route(x[:, ::2], 128)
    got = hadamard_transform(x.to(DEV)[:, ::2], 128)  # made contiguous: the kernel
    assert len(kernel_calls) == 1 and torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))
    # a storage offset of one element breaks the 16-byte alignment: the composed route, on the device, same bits
    flat = torch.empty(6 * 512 + 1, dtype=torch.bfloat16, device=DEV)
    mis = flat[1:].view(6, 512)
    mis.copy_(x[:, ::2])
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    got = hadamard_transform(mis, 128)
    assert len(kernel_calls) == 1 and torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))
    assert config.FUSED_PATHS
    config.FUSED_PATHS = False
    try:
        got = hadamard_transform(x.to(DEV)[:, ::2], 128)
    finally:
        config.FUSED_PATHS = True
    assert len(kernel_calls) == 1 and torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize('dt', list(DTYPES))
def test_backward_is_the_forward_on_the_gradient(dt, kernel_calls):
    from brevitas_amd.function.hadamard import hadamard_transform
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(7, 1536, generator=gen).to(dtype)
    g = torch.randn(7, 1536, generator=gen).to(dtype)
    xd = x.to(DEV).requires_grad_(True)
    y = hadamard_transform(xd, 512)
    y.backward(g.to(DEV))
    assert len(kernel_calls) == 2
    assert torch.equal(y.detach().cpu().view(torch.uint8), cpu_route(x, 512).view(torch.uint8))
    assert torch.equal(xd.grad.cpu().view(torch.uint8), cpu_route(g, 512).view(torch.uint8))


def test_rotated_module_matches_the_composed_route(monkeypatch):
    """RotatedModule around a QuantLinear with a dynamic per-row input quantizer, [7, 512] bfloat16: output and input
    gradient have the bits of the same model whose transform takes the composed route (the route of CPU tensors); the
    quantizer and the matrix product are the same device code in both runs."""
    from brevitas_amd import _native as nat
    from brevitas_amd.nn import QuantLinear, RotatedModule
    from brevitas_amd.quant import Int8DynamicActPerRowFloat
    torch.manual_seed(19)
    layer = QuantLinear(512, 48, input_quant=Int8DynamicActPerRowFloat()).to(torch.bfloat16).to(DEV)
    model = RotatedModule(layer, 256)
    x = torch.randn(7, 512).to(torch.bfloat16).to(DEV)
    g = torch.randn(7, 48).to(torch.bfloat16).to(DEV)

    def run():
        xd = x.clone().requires_grad_(True)
        y = model(xd)
        y.backward(g)
        return y.detach(), xd.grad

    y_k, dx_k = run()
    monkeypatch.setattr(nat, 'hadamard_supported', lambda *a, **k: False)
    y_c, dx_c = run()
    assert torch.equal(y_k.view(torch.uint8), y_c.view(torch.uint8))
    assert torch.equal(dx_k.view(torch.uint8), dx_c.view(torch.uint8))
    # and the transform inside is the CPU's, bit for bit
    from brevitas_amd.function.hadamard import hadamard_transform
    monkeypatch.undo()
    assert torch.equal(hadamard_transform(x, 256).cpu().view(torch.uint8), cpu_route(x.cpu(), 256).view(torch.uint8))


def test_more_than_2_31_elements_in_place():
    """row bases are 64-bit: bfloat16 [R, 8192] with R * 8192 > 2^31, in place (4 GiB), the non-temporal variant; the
    first and the last four rows against the CPU"""
    from brevitas_amd import _native as nat
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip('needs 8 GB of free device memory')
    cols, rows = 8192, (1 << 18) + 4
    assert rows * cols > 2 ** 31
    x = torch.empty(rows, cols, device=DEV, dtype=torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(123456)
    step = 1 << 14
    for lo in range(0, rows, step):  # filled in pieces: a float32 randn of the whole tensor would need another 8 GiB
        n = min(step, rows - lo)
        x[lo:lo + n] = torch.randn(n, cols, device=DEV, generator=gen).to(torch.bfloat16)
    head, tail = x[:4].cpu(), x[-4:].cpu()
    nat.hadamard(x, rows, cols, cols, cols ** -0.5, out=x)
    assert torch.equal(x[:4].cpu().view(torch.uint8), cpu_route(head, cols).view(torch.uint8))
    assert torch.equal(x[-4:].cpu().view(torch.uint8), cpu_route(tail, cols).view(torch.uint8))


def test_hadamard_classifier_on_the_device():
    """the transform is bit-equal; the norm is a torch reduction whose order differs between devices, so this case takes
    the dense-product bound of tests/test_hadamard_host.py against a float64 dense product"""
    from brevitas_amd.function.hadamard import hadamard_matrix
    from brevitas_amd.nn import HadamardClassifier
    torch.manual_seed(23)
    layer = HadamardClassifier(24, 10)
    x = torch.randn(6, 24)
    got = layer.to(DEV)(x.to(DEV)).detach().cpu()
    cpu = layer.cpu()(x).detach()
    xn = x.double() / (x.double().norm() + 1e-8)
    dense = xn @ hadamard_matrix(32, torch.float64)[:10, :24].t()
    scale = float(layer.scale.detach())
    y64 = -scale * dense
    # the bound of tests/test_hadamard_host.py on the normalised, padded row: b = 32, the layer's scale, float32 output
    bound = 1.01 * scale * 6 * 2.0 ** -24 * xn.abs().sum(dim=1, keepdim=True) + 2.0 ** -23 * y64.abs()
    assert ((got.double() - y64).abs() <= bound).all()
    assert ((cpu.double() - y64).abs() <= bound).all()

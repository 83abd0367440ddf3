"""The AWQ clip-search kernel (csrc/bvq_group_clip.hip) at its edges, against the float64 reference of
tests/test_awq_clip_host.py (check_search: the derived bound on every loss, the pick, y / scale / stat bit-equal to
quantize_at_index) and against itself where the kernel's structure promises equal bits:

  row tiles          511 / 512 / 513 / 1025 rows of a 512-row workgroup at g = 128, a second tile at g = 16 and g = 64
  independence       a row's five outputs do not depend on its neighbours, its wave or its tile: row slices launched alone
  candidate count    n = 1 .. 16; the losses of a table's prefix are the prefix of the table's losses
  ties, table order  repeated and non-monotone ratios: equal thresholds give equal losses, the first one is kept
  special values     NaN / +inf / -inf groups; an all-zero and a NaN Hessian block stay inside their group column
  bit widths         2, 3 and 5
  group columns      40 and 9 of them
  refusals           candidate counts, group size, geometry, alignment, hb's dtype and shape, the ratio table
  capture            one launch captured on a side stream and replayed
  addressing         4 GiB of bfloat16: more than 2^31 elements, the last rows behind 2^32 bytes
"""
import ctypes

import pytest
import torch

from brevitas_amd import _native as nat
from brevitas_amd import quant as Q
from brevitas_amd.core.quant import _fused
from brevitas_amd.graph import awq_clip_ratios, hessian_blocks
from test_awq_clip_host import check_search, clip_inputs
from test_gpu_awq_clip import DEV, launches, searched  # noqa: F401  (launches: the fixture that records every launch)
from test_group_mse_host import same_bits

pytestmark = pytest.mark.gpu
DTYPES = ['f32', 'bf16', 'f16']


def kernel_args(x, g, bits):
    """(descriptor, min_val, thr_div) of nat.group_clip_fwd for x [R, K] in groups of g, as awq_clip_weight forms them
    for Int8WeightPerGroupFloat at this bit width"""
    quant = Q.Int8WeightPerGroupFloat(torch.nn.Parameter(torch.zeros(1, g, dtype=x.dtype)), group_size=g,
                                      bit_width=bits).to(DEV)
    tmpl = quant._group_template(quant.msb_clamp_bit_width_impl())
    desc, thr_div = _fused.unit_call(x, g, False, tmpl.int_thr, tmpl.qmin, tmpl.qmax, tmpl.clamp_ste)
    return desc, tmpl.min_val, thr_div


def launch(x, hb, g, bits, ratios):
    """one launch of the kernel on device tensors -> (y, scale, stat, idx, losses), still on the device"""
    desc, min_val, thr_div = kernel_args(x, g, bits)
    table = nat.mse_ratio_table([float(r) for r in ratios])
    assert nat.group_clip_supported(desc, x, hb, len(table))
    return nat.group_clip_fwd(desc, x, hb, table, min_val, thr_div)


def checked(w, h, g, bits, ratios, launches):  # noqa: F811
    """awq_clip_weight on the device, exactly one launch, the whole of check_search -> (idx, losses) on the host"""
    before = len(launches)
    res = searched(w, h, g, bits, ratios)
    assert len(launches) == before + 1
    y, scale, stat, idx, losses = (t.cpu() for t in launches[-1])
    assert losses.shape == (w.shape[0], w.shape[1] // g, len(ratios))
    assert same_bits(res.q.cpu(), y) and torch.equal(res.index.cpu(), idx)
    check_search(w, g, bits, hessian_blocks(h, g), ratios, idx, losses, y, scale, stat)
    return idx, losses


def all_same_bits(got, want):
    return all(same_bits(a, b) for a, b in zip(got, want))


# ---- 1. row tiles ---------------------------------------------------------------------------------------------------

TILES = [(128, 'bf16', rows) for rows in (511, 512, 513, 1025)] + \
        [(16, dn, rows) for dn in ('f32', 'f16') for rows in (512, 513)] + [(64, 'f32', 513)]


def test_row_tile_edges(launches):  # noqa: F811
    """a full last tile, a tile of one row next to three waves that leave at once, three tiles"""
    for g, dn, rows in TILES:
        print('case', g, dn, rows)
        w, h = clip_inputs(rows, 2 * g, g, dn)
        idx, _ = checked(w, h, g, 4, awq_clip_ratios(20, 0.5), launches)
        assert bool((idx == 0).any()) and bool((idx > 0).any()), (g, dn, rows)


# ---- 2. a row's result is its own -----------------------------------------------------------------------------------

@pytest.mark.parametrize('g,dn,rows', [(128, 'bf16', 1025), (16, 'f16', 517)])
def test_rows_do_not_depend_on_neighbours_wave_or_tile(g, dn, rows, launches):  # noqa: F811
    """the next row is loaded while this one is worked on: launched alone, as the first row of a one-row grid or in
    another wave of another tile, a row has the bits it has in the whole launch"""
    bits, ratios = 4, awq_clip_ratios(20, 0.5)
    w, h = clip_inputs(rows, 2 * g, g, dn)
    x, hb = w.to(DEV), hessian_blocks(h, g).to(DEV)
    whole = launch(x, hb, g, bits, ratios)
    y, scale, stat, idx, losses = (t.cpu() for t in whole)
    check_search(w, g, bits, hessian_blocks(h, g), ratios, idx, losses, y, scale, stat)
    slices = [(lo, hi) for lo, hi in ((0, 1), (510, 514), (512, 517), (1024, 1025)) if hi <= rows]
    assert len(slices) >= 3
    for lo, hi in slices:
        part = x[lo:hi]
        assert part.is_contiguous() and part.data_ptr() % 16 == 0
        got = launch(part, hb, g, bits, ratios)
        assert all_same_bits(got, [t[lo:hi] for t in whole]), (lo, hi)
    assert len(launches) == 1 + len(slices)


# ---- 3. every candidate count ---------------------------------------------------------------------------------------

def test_every_candidate_count(launches):  # noqa: F811
    """n = 1 .. 16: the live masks of both layouts, the loss store and the pick change at every n"""
    g = 64
    w, h = clip_inputs(33, 2 * g, g, 'bf16')
    for n in range(1, 17):
        print('case n =', n)
        ratios = awq_clip_ratios(2 * n, 0.5)
        assert len(ratios) == n
        idx, _ = checked(w, h, g, 4, ratios, launches)
        if n > 1:
            assert bool((idx == 0).any()) and bool((idx > 0).any()), n


def test_losses_of_a_prefix_are_the_prefix_of_the_losses(launches):  # noqa: F811
    """a row of the matrix product depends on its own row of D only and the lane sum is per candidate: the candidates
    past the table's end (zero rows of D, dead lanes of the masks) leave the live ones' losses alone"""
    g, bits = 64, 4
    w, h = clip_inputs(33, 2 * g, g, 'bf16')
    x, hb = w.to(DEV), hessian_blocks(h, g).to(DEV)
    table = awq_clip_ratios(32, 0.5)
    assert len(table) == 16
    full = launch(x, hb, g, bits, table)[4]
    assert full.shape == (33, 2, 16)
    for m in (1, 3, 4, 5, 8, 13):
        part = launch(x, hb, g, bits, table[:m])[4]
        assert part.shape == (33, 2, m) and same_bits(part, full[..., :m].contiguous()), m
    assert len(launches) == 7


# ---- 4. ties and table order ----------------------------------------------------------------------------------------

def test_repeated_and_unordered_ratios(launches):  # noqa: F811
    """equal ratios are equal thresholds and equal losses, and the first of them is the one kept"""
    g = 32
    ratios = torch.tensor([1.0, 0.8, 0.8, 0.9, 1.0, 0.6, 0.8])
    for dn in DTYPES:
        print('case', dn)
        w, h = clip_inputs(33, 2 * g, g, dn)
        idx, losses = checked(w, h, g, 4, ratios, launches)
        for first, again in ((1, 2), (1, 6), (0, 4)):
            assert same_bits(losses[..., first], losses[..., again]), dn   # the all-zero group is NaN in float16
        taken = set(idx.reshape(-1).tolist())
        assert not taken & {2, 4, 6} and len(taken) >= 3, (dn, taken)


# ---- 5. special values ----------------------------------------------------------------------------------------------

def special_inputs(dn):
    g = 32
    w, h = clip_inputs(33, 3 * g, g, dn)
    return g, w, h


def each_dtype(case, launches):  # noqa: F811
    for dn in DTYPES:
        print('case', dn)
        del launches[:]
        case(dn, launches)


def test_nan_and_inf_groups_keep_candidate_0(launches):  # noqa: F811
    each_dtype(nan_and_inf_groups, launches)


def test_a_zero_hessian_block_stays_in_its_column(launches):  # noqa: F811
    each_dtype(zero_hessian_block, launches)


def test_a_nan_in_a_hessian_block_stays_in_its_column(launches):  # noqa: F811
    each_dtype(nan_in_a_hessian_block, launches)


def nan_and_inf_groups(dn, launches):  # noqa: F811
    g, w, h = special_inputs(dn)
    planted = {(3, 0): float('nan'), (7, 1): float('inf'), (11, 2): float('-inf')}   # (row, group) -> value
    for (row, j), v in planted.items():
        w[row, j * g + 5] = v
    idx, losses = checked(w, h, g, 4, awq_clip_ratios(20, 0.5), launches)
    others = torch.zeros(33, 3, dtype=torch.bool)   # the ordinary groups of the planted rows
    for row, j in planted:
        assert not bool(torch.isfinite(losses[row, j]).any()) and int(idx[row, j]) == 0
        others[row] = True
        others[row, j] = False
    assert int(others.sum()) == 6
    assert bool(torch.isfinite(losses[others]).all()) and bool((idx[others] > 0).any())


def zero_hessian_block(dn, launches):  # noqa: F811
    g, w, h = special_inputs(dn)
    ratios = awq_clip_ratios(20, 0.5)
    x = w.to(DEV)
    plain = launch(x, hessian_blocks(h, g).to(DEV), g, 4, ratios)
    h0 = h.clone()
    h0[:g, :g] = 0.0
    got = launch(x, hessian_blocks(h0, g).to(DEV), g, 4, ratios)
    assert len(launches) == 2
    y, scale, stat, idx, losses = (t.cpu() for t in got)
    check_search(w, g, 4, hessian_blocks(h0, g), ratios, idx, losses, y, scale, stat)
    col = losses[:, 0]
    assert bool((idx[:, 0] == 0).all()) and bool((col[torch.isfinite(col)] == 0).all())
    assert bool(torch.isfinite(col).any())
    assert all_same_bits([t[:, 1:] for t in (scale, stat, idx, losses)],
                         [t.cpu()[:, 1:] for t in plain[1:]])
    assert same_bits(y[:, g:], plain[0].cpu()[:, g:])


def nan_in_a_hessian_block(dn, launches):  # noqa: F811
    g, w, h = special_inputs(dn)
    ratios = awq_clip_ratios(20, 0.5)
    x = w.to(DEV)
    plain = launch(x, hessian_blocks(h, g).to(DEV), g, 4, ratios)
    hn = h.clone()
    hn[2 * g + 5, 2 * g + 5] = float('nan')
    got = launch(x, hessian_blocks(hn, g).to(DEV), g, 4, ratios)
    assert len(launches) == 2
    y, scale, stat, idx, losses = (t.cpu() for t in got)
    check_search(w, g, 4, hessian_blocks(hn, g), ratios, idx, losses, y, scale, stat)   # y, scale: candidate 0's
    assert bool(torch.isnan(losses[:, 2]).all()) and bool((idx[:, 2] == 0).all())
    assert all_same_bits([t[:, :2] for t in (scale, stat, idx, losses)],
                         [t.cpu()[:, :2] for t in plain[1:]])
    assert same_bits(y[:, :2 * g], plain[0].cpu()[:, :2 * g])


# ---- 6. bit widths --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits', [2, 3, 5])
def test_low_and_odd_bit_widths(bits, launches):  # noqa: F811
    for g in (32, 128):
        for dn in ('bf16', 'f32'):
            print('case', g, dn)
            w, h = clip_inputs(33, 2 * g, g, dn)
            idx, _ = checked(w, h, g, bits, awq_clip_ratios(20, 0.5), launches)
            if bits == 2:   # four levels: the abs-max is rarely the best threshold
                assert int((idx > 0).sum()) > idx.numel() // 2, (g, dn)


# ---- 7. many group columns ------------------------------------------------------------------------------------------

def test_many_group_columns(launches):  # noqa: F811
    for g, groups, dn in ((16, 40, 'f16'), (128, 9, 'f32')):
        print('case', g, groups, dn)
        w, h = clip_inputs(5, groups * g, g, dn)
        idx, _ = checked(w, h, g, 4, awq_clip_ratios(20, 0.5), launches)
        assert bool((idx > 0).any()), (g, groups, dn)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------

def test_refusals_leave_no_error_behind(launches):  # noqa: F811
    g, bits = 32, 4
    w, h = clip_inputs(33, 2 * g, g, 'f32')
    x, hb = w.to(DEV), hessian_blocks(h, g).to(DEV)
    ratios = awq_clip_ratios(20, 0.5)
    desc, min_val, thr_div = kernel_args(x, g, bits)
    want = launch(x, hb, g, bits, ratios)

    def refused(desc, x, hb, values, supported=False):
        """fwd raises and names the entry; supported (which never sees the table's values) says no; a good launch
        afterwards has the right bits"""
        table = (ctypes.c_float * len(values))(*values)
        assert nat.group_clip_supported(desc, x, hb, len(values)) is supported
        with pytest.raises(nat.BvqError, match='bvq_group_clip_fwd'):
            nat.group_clip_fwd(desc, x, hb, table, min_val, thr_div)
        assert all_same_bits(launch(*good), want)

    good = (x, hb, g, bits, ratios)
    ten = ratios.tolist()
    refused(desc, x, hb, [1.0] + [0.5 + i / 32 for i in range(16)])            # 17 candidates
    refused(desc, x, hb, [])                                                    # none
    x256 = torch.randn(33, 512, device=DEV)
    refused(kernel_args(x256, 256, bits)[0], x256, torch.eye(256, device=DEV).repeat(2, 1, 1).contiguous(), ten)
    x48 = torch.randn(33, 48, device=DEV)                                       # K = 48: one group and a half
    refused(kernel_args(x48, g, bits)[0], x48, hb[:1].contiguous(), ten)
    buf = torch.empty(hb.numel() + 1, device=DEV)
    refused(desc, x, buf[1:].view(hb.shape).copy_(hb), ten)                     # hb 4 bytes off a 16-byte boundary
    refused(desc, x, hb.double(), ten)                                          # hb's dtype, shape: the Python side
    refused(desc, x, hb[:1].contiguous(), ten)
    refused(desc, x, hb.reshape(1, 2 * g, g), ten)
    refused(desc, x, hb, [0.95, 0.9], supported=True)                           # ratio 0 is the abs-max itself
    for bad in (0.0, 1.5, float('nan')):
        refused(desc, x, hb, [1.0, 0.9, bad, 0.8], supported=True)
    assert len(launches) == 1 + 12   # the refused calls returned nothing


# ---- 9. capture and side stream -------------------------------------------------------------------------------------

def test_one_launch_captured_and_replayed():
    """the argument struct with its ratio table goes into the graph by value: a weight changed in place after the
    capture is what the replay quantizes"""
    g, bits = 64, 4
    w, h = clip_inputs(33, 2 * g, g, 'bf16')
    x, hb = w.to(DEV), hessian_blocks(h, g).to(DEV)
    desc, min_val, thr_div = kernel_args(x, g, bits)
    table = nat.mse_ratio_table(awq_clip_ratios(20, 0.5).tolist())   # alive until the last replay has finished

    def one():
        return nat.group_clip_fwd(desc, x, hb, table, min_val, thr_div)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):     # a single stream: no parallel branches
        captured = one()
    with torch.no_grad():
        x.mul_(1.25)
    want = one()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all_same_bits(captured, want)
    y, scale, stat, idx, losses = (t.cpu() for t in captured)
    check_search(x.cpu(), g, bits, hessian_blocks(h, g), awq_clip_ratios(20, 0.5), idx, losses, y, scale, stat)
    del table


# ---- 10. past 2^31 elements -----------------------------------------------------------------------------------------

def test_more_than_2_31_elements(launches):  # noqa: F811
    """row, group and loss offsets are 64-bit: bfloat16 [2^18 + 4, 8192] at g = 128, x and y of 4 GiB each, the last
    rows behind 2^32 bytes; rows are independent, so the reference of a slice of rows is the reference of those rows"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip('needs 12 GB of free device memory')
    g, bits, cols, rows = 128, 4, 8192, (1 << 18) + 4
    assert rows * cols > 2 ** 31 and (rows - 4) * cols * 2 >= 2 ** 32
    ratios = torch.tensor([1.0, 0.75])
    gen = torch.Generator().manual_seed(97)
    xc = torch.randn(64, cols // g, g, generator=gen) * torch.randn(cols // g, g, generator=gen).exp()
    hb_host = ((2.0 / 64) * torch.einsum('nja,njb->jab', xc, xc)).contiguous()   # the diagonal blocks of 2 / 64 X^T X
    hb = hb_host.to(DEV)
    x = torch.empty(rows, cols, device=DEV, dtype=torch.bfloat16)
    dgen = torch.Generator(device=DEV).manual_seed(123456)
    step = 1 << 12
    for lo in range(0, rows, step):  # filled in pieces: a float32 randn of the whole tensor would need another 8 GiB
        n = min(step, rows - lo)
        piece = torch.randn(n, cols, device=DEV, generator=dgen)
        outlier = torch.rand(n, cols, device=DEV, generator=dgen) < 0.03   # as clip_inputs plants them
        x[lo:lo + n] = torch.where(outlier, piece * 6.0, piece).to(torch.bfloat16)
    del piece, outlier
    y, scale, stat, idx, losses = launch(x, hb, g, bits, ratios)
    assert len(launches) == 1
    assert int(idx.min()) == 0 and int(idx.max()) == 1
    for part in (slice(0, 4), slice(rows - 4, rows)):
        check_search(x[part].cpu(), g, bits, hb_host, ratios, idx[part].cpu(), losses[part].cpu(), y[part].cpu(),
                     scale[part].cpu(), stat[part].cpu())

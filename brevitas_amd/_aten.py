"""Pure-torch route for CPU tensors (SURVEY 8b "Errors").

The HIP engine takes device tensors only.  A layer built on the CPU, a CPU evaluation pass or a CPU unit
test must still run through the same modules -- the reference's own backend failure is a silent fall-back
to its Python ops (B/__init__.py:66-84) -- so every entry of `brevitas_amd._native` that the module
surface uses has an ATen-only counterpart here: the reference's op composition restated on torch ops,
nothing fused, nothing from oracle/ (that is test infrastructure).  `for_tensor(x)` picks the backend: a
ROCm tensor always gets the HIP library (and fails loudly if it is missing: importing
`brevitas_amd._native` without libbvq.so raises); only a CPU tensor gets this module.
"""
import torch

from . import _native as nat


def for_tensor(*tensors):
    """the backend module serving these tensors: `_native` (HIP) for device tensors, this module for CPU ones"""
    for t in tensors:
        if t is not None and t.is_cuda:
            return nat
    return _SELF


# ---- the 12 straight-through forwards (B/ops/autograd_ste_ops.py, B/function/ops.py) ------------------

def unary(op, x):
    if op == nat.OP_ROUND:
        return torch.round(x)
    if op == nat.OP_CEIL:
        return torch.ceil(x)
    if op == nat.OP_FLOOR:
        return torch.floor(x)
    if op == nat.OP_ROUND_TO_ZERO:  # B/function/ops.py:52
        return torch.sign(x) * torch.floor(torch.abs(x))
    if op == nat.OP_DPU_ROUND:      # B/function/ops.py:71
        return torch.where((x < 0.) & (x - torch.floor(x) == 0.5), torch.ceil(x), torch.round(x))
    if op == nat.OP_BINARY_SIGN:    # B/function/ops.py:31-34: +1 at 0
        return torch.ge(x, 0.0).type(x.dtype) + torch.lt(x, 0.0).type(x.dtype) * -1.0
    if op == nat.OP_TERNARY_SIGN:
        return torch.sign(x)
    if op == nat.OP_ABS:
        return torch.abs(x)
    raise nat.BvqError('brevitas_amd._aten.unary: unknown op %r' % (op,))


def scalar_clamp(x, min_val, max_val):
    if max_val is None:
        return torch.clamp_min(x, min_val)
    return torch.clamp(x, min_val, max_val)


def tensor_clamp(x, min_val, max_val, out=None):
    """where(x > max, max, x) then where(. < min, min, .)  (B/function/ops.py:98-100)"""
    y = torch.where(x > max_val, max_val.type_as(x), x)
    y = torch.where(y < min_val, min_val.type_as(y), y)
    if out is not None:
        out.copy_(y)
        return out
    return y


def tensor_clamp_bwd(grad_y, x, min_val, max_val):
    """autograd of the two torch.where w.r.t. x: the gradient passes where neither bound replaced the value"""
    hi = x > max_val
    y = torch.where(hi, max_val.type_as(x), x)
    lo = y < min_val
    return torch.where(hi | lo, torch.zeros_like(grad_y), grad_y)


def abs_binary_sign_grad_bwd(grad_y, x):
    return unary(nat.OP_BINARY_SIGN, x) * grad_y


def running_stats_update(running, stat, momentum, first_batch):
    """_RuntimeStats' in-place update (B/core/stats/stats_wrapper.py:61-66)"""
    if first_batch:
        running.mul_(stat)
    else:
        running.mul_(1 - momentum)
        running.add_(momentum * stat)
    return running


# ---- statistics (B/core/stats/stats_op.py): plain torch ops, autograd included --------------------

def _kth_rank_high(q, n):
    import math
    return int(math.floor(.01 * q * n + 0.5))  # k is 1-indexed: round away from zero (stats_op.py:56)


def _kth_rank_low(q, n):
    import math
    return int(math.ceil(.01 * q * n))  # stats_op.py:84


def _along(x, dim):
    if dim is None:
        return x.numel()
    assert len(x.size()) == 2, "Only 2-dim input is supported."
    return x.shape[dim]


def _kth(x, k, dim):
    return x.view(-1).kthvalue(k).values if dim is None else x.kthvalue(k, dim=dim).values


def abs_max(x, dim):
    return torch.max(torch.abs(x)) if dim is None else torch.max(torch.abs(x), dim=dim)[0]


def min_max(x, dim):
    """-> (max, min)"""
    if dim is None:
        return torch.max(x), torch.min(x)
    return torch.max(x, dim=dim)[0], torch.min(x, dim=dim)[0]


class _ShardedExtremum(torch.autograd.Function):
    """max |x| / max x / min x of a BATCH-SHARDED CPU tensor (brevitas_amd.distributed over gloo): the device route's
    protocol on torch ops -- all-reduce(MAX) of the float32 statistic forward; backward the summed gradient goes where
    the single-process run on the concatenated batch puts it (first attaining element of the lowest rank along a
    reduced dim, evenly over the ties of all shards for a whole-tensor reduction)."""

    @staticmethod
    def forward(ctx, x, dim, group, kind):
        import torch.distributed as dist
        key = torch.abs(x) if kind == 'abs' else (x if kind == 'max' else -x)
        rows = key.reshape(1, -1) if dim is None else key.movedim(dim, -1).reshape(-1, key.shape[dim])
        local = rows.max(dim=1).values.float()
        dist.all_reduce(local, op=dist.ReduceOp.MAX, group=group)
        stat_key = local.to(x.dtype)
        ctx.save_for_backward(x, stat_key)
        ctx.args = (dim, group, kind)
        stat = stat_key if kind != 'min' else -stat_key
        return stat.reshape(()) if dim is None else stat.reshape([s for i, s in enumerate(x.shape) if i != dim % x.dim()])

    @staticmethod
    def backward(ctx, gstat):
        from .distributed import sync_backward
        x, stat_key = ctx.saved_tensors
        dim, group, kind = ctx.args
        key = torch.abs(x) if kind == 'abs' else (x if kind == 'max' else -x)
        moved = key.reshape(1, -1) if dim is None else key.movedim(dim, -1)
        rows = moved.reshape(-1, moved.shape[-1])
        hit = rows == stat_key.reshape(-1, 1)
        ch = rows.shape[0]
        g32 = gstat.reshape(-1).float()
        if dim is None:
            info = hit.sum().reshape(1).to(torch.int64)
            gsum, _, total = sync_backward(g32, info, 1, group)
            drows = torch.where(hit, (gsum / total.to(gsum.dtype)).to(x.dtype), torch.zeros((), dtype=x.dtype))
        else:
            first = torch.where(hit.any(dim=1), hit.to(torch.int8).argmax(dim=1), torch.full((ch,), -1, dtype=torch.int64))
            gsum, info, _ = sync_backward(g32, first, ch, group, first_only=True)
            drows = torch.zeros_like(rows)
            own = info >= 0
            drows[own.nonzero().reshape(-1), info[own]] = gsum.to(x.dtype)[own]
        d = drows.reshape(moved.shape)
        d = d.reshape(x.shape) if dim is None else d.movedim(-1, dim)
        if kind == 'abs':
            d = d * torch.sgn(x)
        elif kind == 'min':
            pass  # d(min x)/dx = +1 at the arg-min: the key's sign and the statistic's cancel
        return d, None, None, None


def sharded_abs_max(x, dim, group):
    return _ShardedExtremum.apply(x, dim, group, 'abs')


def sharded_min_max(x, dim, group):
    """-> (max, min)"""
    return _ShardedExtremum.apply(x, dim, group, 'max'), _ShardedExtremum.apply(x, dim, group, 'min')


def abs_percentile(x, q, dim):
    return _kth(x.abs(), _kth_rank_high(q, _along(x, dim)), dim)


def low_percentile(x, q, dim):
    return _kth(x, _kth_rank_low(q, _along(x, dim)), dim)


def high_percentile(x, q, dim):
    return _kth(x, _kth_rank_high(q, _along(x, dim)), dim)


def abs_mean_var(x, dim):
    """-> (mean |x|, unbiased var |x|)"""
    a = torch.abs(x)
    if dim is None:
        return torch.mean(a), torch.var(a)
    return torch.mean(a, dim=dim), torch.var(a, dim=dim)


# ---- group-wise clip search (core/quant/int.py: GroupwiseMSEIntQuant), the composed route --------------------
# Both steps take the module's own sub-modules as two callables, so they run the same ops as the plain group-wise
# quantizer: scale_of(threshold [groups, 1]) -> scale [groups, 1], quantize(scale) -> y [groups, g].  They serve CPU and
# device tensors alike (the ops dispatch by themselves) and define what the one-launch kernels compute.

def group_mse_threshold(stat, ratio):
    """a candidate's threshold: the statistic times a float32 ratio (a Python float, or a float32 tensor with one ratio
    per group), the product formed in float32 and rounded once to the statistic's dtype.  Differentiable in stat."""
    if not torch.is_tensor(ratio):
        ratio = torch.tensor(float(ratio), dtype=torch.float32, device=stat.device)
    return (stat.float() * ratio).to(stat.dtype)


def group_mse_index(xg, ratios, stat, scale_of, quantize):
    """-> idx uint8 [groups]: per group the first candidate whose float32 squared error sum((y_i - x)^2) is strictly
    below every earlier one's.  NaN errors (a NaN or Inf group) are below nothing: such a group keeps 0, as a group of
    zeros does.  An explicit loop: argmin's order among ties is not defined."""
    with torch.no_grad():
        xf = xg.float()
        idx = torch.zeros(xg.shape[0], dtype=torch.uint8, device=xg.device)
        best = None
        for i, r in enumerate(ratios):
            d = quantize(scale_of(group_mse_threshold(stat, r))).float() - xf
            e = (d * d).sum(dim=1)
            if best is None:
                best = e
                continue
            better = e < best
            idx = torch.where(better, torch.full_like(idx, i), idx)
            best = torch.where(better, e, best)
    return idx


def group_mse_quantize_at(ratios, idx, stat, scale_of, quantize):
    """quantize every group at the candidate idx names -> (y [groups, g], scale [groups, 1]); idx is a constant,
    everything else is differentiated by autograd through the sub-modules"""
    table = torch.tensor([float(r) for r in ratios], dtype=torch.float32, device=stat.device)
    scale = scale_of(group_mse_threshold(stat, table[idx.long()].reshape(stat.shape)))
    return quantize(scale), scale


# ---- group-wise HQO zero-point (core/quant/int.py: GroupwiseHQOIntQuant), the composed route ------------------
# The search takes the module's own integer conversion as a callable, to_int(zero_point [groups, 1]) -> q [groups, g], so
# it runs the same ops as the plain asymmetric quantizer.  It serves CPU and device tensors alike and defines what the
# one-launch kernels compute ("Group-wise HQO zero-point").

def tree_sum(v, chunk):
    """the sum over dim 1 of v [groups, g] in the fixed order of the group walk's kernels -> [groups].  Within each run
    of `chunk` consecutive elements (a 16-byte chunk of the weight's dtype) the even-indexed elements are added in order
    into one accumulator and the odd-indexed into another, the two are added, and the per-chunk values are reduced by
    halves, t[:h] + t[h:], until one is left (g / chunk is a power of two)."""
    c = v.reshape(v.shape[0], -1, chunk)
    even, odd = c[:, :, 0], c[:, :, 1]
    for k in range(2, chunk, 2):
        even = even + c[:, :, k]
        odd = odd + c[:, :, k + 1]
    t = even + odd
    while t.shape[1] > 1:
        h = t.shape[1] // 2
        if 2 * h != t.shape[1]:
            raise ValueError('tree_sum: %d chunks per group is no power of two' % (v.shape[1] // chunk))
        t = t[:, :h] + t[:, h:]
    return t[:, 0]


def group_hqo_search(xg, inv_beta, p, scale, zp0, to_int):
    """Half-quadratic optimisation of the zero-point of every group of xg [groups, g] at the fixed scale [groups, 1],
    from the integer zero-point zp0 [groups, 1] on -> (zero_point [groups, 1] in xg's dtype T, idx uint8 [groups], the
    kept candidate's float32 error [groups], candidate 0's [groups]).  No gradient.

    inv_beta: the n + 1 float32 values 1 / (beta * kappa^i); p: the norm, in (0, 1].  Candidates i = 0 .. n, every
    float32 op rounded on its own:
        zp_i = T(z_i), q_i = to_int(zp_i), y_i = T(T(q_i - zp_i) * scale), r = float32(x) - float32(y_i), e_i = tree(|r|)
        the first candidate is the best so far; a later one is if the group is live and e_i < e_best (strict; a NaN
        error is below nothing), and a group whose error did not fall is finished for good.  A constant group (every
        element equal to the first: its scale is the lower bound, the grid has collapsed) is finished after candidate 0
        thr = inv_beta[i] * |r|^(p - 1): inv_beta[i] for p = 1, inv_beta[i] / sqrt(|r|) for p = 0.5 (the correctly rounded
        root), torch.pow otherwise
        w_e = sign(r) * max(|r| - thr, 0);  z_{i+1} = tree(float32(q_i) - (float32(x) - w_e) * (1 / scale)) * (1 / g)
    An explicit loop over all candidates: the groups that are finished are carried along and masked."""
    with torch.no_grad():
        g, dt = xg.shape[1], xg.dtype
        chunk = 16 // xg.element_size()
        xf = xg.float()
        inv_s = 1.0 / scale.float()
        z = zp0.float()
        n = len(inv_beta) - 1
        for i in range(n + 1):
            zp = z.to(dt)
            q = to_int(zp)
            y = (q - zp) * scale
            r = xf - y.float()
            ar = r.abs()
            e = tree_sum(ar, chunk)
            if i == 0:
                e0 = e_best = e
                zp_best = zp
                idx = torch.zeros(xg.shape[0], dtype=torch.uint8, device=xg.device)
                live = ~(xg == xg[:, :1]).all(dim=1)  # a constant group is not searched
            else:
                better = live & (e < e_best)
                e_best = torch.where(better, e, e_best)
                zp_best = torch.where(better.reshape(-1, 1), zp, zp_best)
                idx = torch.where(better, torch.full_like(idx, i), idx)
                live = better
            if i == n:
                break
            ib = torch.tensor(float(inv_beta[i]), dtype=torch.float32, device=xg.device)
            if p == 1.0:
                thr = ib
            elif p == 0.5:
                # the correctly rounded float32 root: torch's vectorized float32 sqrt on the CPU is not, the float64 root
                # rounded once is (53 >= 2 * 24 + 2 bits: the second rounding cannot change the result)
                thr = ib / torch.sqrt(ar.double()).float()
            else:
                thr = ib * torch.pow(ar, p - 1.0)
            sign = (r > 0).float() - (r < 0).float()
            w_e = sign * torch.clamp_min(ar - thr, 0.0)
            z = (tree_sum(q.float() - (xf - w_e) * inv_s, chunk) * (1.0 / g)).reshape(-1, 1)
    return zp_best, idx, e_best, e0


# ---- Hadamard transform (include/bvq.h, "Hadamard transform") ----------------------------------------------

def hadamard(x, block, scale):
    """scale * (I (x) H_block) x along the last dimension of x, the definition restated on torch ops: float32 from the
    widening to the multiply, butterfly stages h = 1, 2 .. block / 2 in ascending order, one multiply by float32(scale),
    one rounding to x.dtype.  Every stage is a float32 addition and a float32 subtraction of the same operands the
    kernel pairs, so the two routes give the same bits, on a CPU tensor and on a device one."""
    y = x.to(torch.float32)
    h = 1
    while h < block:
        y = y.reshape(-1, block // (2 * h), 2, h)
        a, c = y[:, :, 0], y[:, :, 1]
        y = torch.stack((a + c, a - c), dim=2)
        h *= 2
    scale32 = torch.tensor(float(scale), dtype=torch.float64).to(torch.float32).item()
    return (y.reshape(x.shape) * scale32).to(x.dtype)


import sys  # noqa: E402

_SELF = sys.modules[__name__]

"""Restatements of the weight-norm quantizer's semantics ("Weight-norm and accumulator-aware weights") for
the tests: the float32 chain on torch CPU ops, the closed-form gradients in float64, and the error bounds.

Bounds, stated once (u = 2^-24, the unit roundoff of float32; K the row length).

Sums.  A float32 sum of K terms, added in ANY order, differs from the exact sum of the same terms by at most
(K - 1) u sum |term_i| to first order (every partial sum is rounded once and is at most sum |term_i|); the second-order
part is below K^2 u^2 sum |term_i|, under 4 u sum |term_i| for K <= 8192.

Norm.  Every term of the norm's sum is non-negative, so sum |term_i| is the sum itself and the bound is relative:
L1, whose terms |v_i| are exact: (K - 1) u + 4 u.  L2: each v_i^2 is rounded once (u, relative, on every term), the sum
adds (K - 1) u + 4 u, the square root halves the relative error and adds its own u: below (K + 4) u as well.  Hence
|n - n64| <= (K + 4) u n64, for both norms and any summation order.

A, B, ds, dg.  The terms gy_i m_i t_i and gy_i q_i are float32 products that kernel and reference share bit for bit
(t, q and m are the forward's bits), so only the order of the additions differs: |A - A64| <= (K + 3) u SA and
|B - B64| <= (K + 3) u SB with SA = sum |gy m t|, SB = sum |gy q|.  ds = B - A adds one rounding, and where g was capped
T dg' = T (s A / g') adds three more on a quantity equal to A in real arithmetic (g' = T s): |ds - ds64| <=
(K + 6) u (SA + SB).  dg' = (s A) / g' has two roundings of its own: |dg - dg64| <= (s / g') (K + 6) u SA.

dv.  dv_i = gy_i m_i c1 - c2 dn_i with c1 = g' / n and c2 = s A / n (L2: c2 / n, times v_i).  A enters through c2 alone:
|dv_i - dv64_i| <= |dn_i| (s / n) (K + 6) u SA  +  6 u (|gy_i m_i c1| + |c2 dn_i|)  +  half an ulp of the dtype at dv64_i,
the middle term covering the roundings of c1, c2, c2 / n, the two products and the subtraction.
"""
import math

import torch

U = 2.0 ** -24
NORM_MIN = 1e-10
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def round_fn(norm):
    if norm == 'l1':
        return lambda t: torch.sign(t) * torch.floor(torch.abs(t))
    return torch.round


def t_bound(acc_bits, in_bits, signed):
    return float(2 ** (acc_bits - 1) - 1) * 2.0 ** ((1 if signed else 0) - in_bits)


def norm64(v, norm):
    v = v.double()
    return v.abs().sum(1) if norm == 'l1' else torch.sqrt((v * v).sum(1))


def chain(v, s, g, n, T, qmax, norm):
    """the forward from a given n on torch CPU ops, every operation in v's compute dtype (float32, or float64 for a
    float64 v): -> (t, r, q, gp, capped, p); v [rows, K], s, g, n [rows]"""
    ct = torch.promote_types(v.dtype, torch.float32)
    v = v.to(ct)
    s, g, n = s.to(ct).reshape(-1, 1), g.to(ct).reshape(-1, 1), n.to(ct).reshape(-1, 1)
    ts = s * torch.full_like(s, T)
    capped = ~(g <= ts)
    gp = torch.where(capped, ts, g)
    p = (s * n) / gp
    t = v / p
    r = round_fn(norm)(t)
    q = torch.where(r > qmax, torch.full_like(r, qmax), r)
    q = torch.where(q < -qmax, torch.full_like(q, -qmax), q)
    return t, r, q, gp, capped, p


def forward_from_n(v, s, g, n, T, qmax, norm):
    """y with the bits the kernel must give for its own n: the float32 chain, cast once to v's dtype"""
    t, r, q, gp, capped, p = chain(v, s, g, n, T, qmax, norm)
    return (q * s.float().reshape(-1, 1)).to(v.dtype)


def closed_forms(v, s, g, gy, n, T, qmax, norm, clamp_ste):
    """the issue's backward in float64, from the float32 (or float64) terms of `chain` at the given n ->
    dict(A, B, SA, SB, ds, dg, dv, c1gm, c2dn, dn, s_over_n, s_over_gp)"""
    t, r, q, gp, capped, p = chain(v, s, g, n, T, qmax, norm)
    ct = t.dtype
    gyc = gy.to(ct)
    m = torch.ones_like(t) if clamp_ste else (~((r > qmax) | (r < -qmax))).to(ct)
    gm = gyc * m
    ta, tb = (gm * t).double(), (gyc * q).double()   # the products in the compute dtype, the sums in float64
    A, B = ta.sum(1), tb.sum(1)
    SA, SB = ta.abs().sum(1), tb.abs().sum(1)
    s64, n64, gp64 = s.double().reshape(-1), n.double().reshape(-1), gp.double().reshape(-1)
    cap = capped.reshape(-1)
    dgp = s64 * A / gp64
    ds = B - A + torch.where(cap, float(T) * dgp if math.isfinite(T) else torch.zeros_like(dgp), torch.zeros_like(dgp))
    dg = torch.where(cap, torch.zeros_like(dgp), dgp)
    v64 = v.double()
    # c2 = n > norm_min ? s A / n : 0 is a choice, not a product with 0 or 1: where n was clamped, an A that is not finite
    # (a NaN in the row) stays out of dv
    kept = n64 > float(torch.tensor(NORM_MIN, dtype=torch.float32))
    dn = torch.sign(v64) if norm == 'l1' else v64 / n64.reshape(-1, 1)
    c1 = (gp64 / n64).reshape(-1, 1)
    c2 = torch.where(kept, s64 * A / n64, torch.zeros_like(A)).reshape(-1, 1)
    c1gm, c2dn = gm.double() * c1, c2 * dn
    return dict(A=A, B=B, SA=SA, SB=SB, ds=ds, dg=dg, dv=c1gm - c2dn, c1gm=c1gm, c2dn=c2dn,
                dn=dn * kept.double().reshape(-1, 1), s_over_n=s64 / n64, s_over_gp=s64 / gp64, kept=kept)


def half_ulp(x64, dtype):
    """half the spacing of `dtype` at the binade of each |x64|"""
    _, e = torch.frexp(x64.abs().clamp_min(2.0 ** -300))
    e = torch.clamp(e.double() - 1.0, min=float(EMIN[dtype]))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def sum_bound(k):
    return (k + 6) * U


def dv_bound(ref, k, dtype):
    sa = ref['SA'].reshape(-1, 1)
    # (A reaches dv through c2 alone: a row whose n was clamped has no such term, whatever its A)
    through_a = torch.where(ref['kept'].reshape(-1, 1), ref['dn'].abs() * ref['s_over_n'].reshape(-1, 1) * sum_bound(k) * sa,
                            torch.zeros_like(ref['c1gm']))
    rest = through_a + 6 * U * (ref['c1gm'].abs() + ref['c2dn'].abs())
    # (the value that is rounded lies within `rest` of dv64: the spacing at the farther end covers a binade crossed)
    return rest + half_ulp(ref['dv'].abs() + rest, dtype)

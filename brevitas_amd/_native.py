"""ctypes binding of libbvq.so -- the C-ABI HIP library (include/bvq.h).

This is the only backend of device tensors: a call here never falls back to torch ops.  If the
library is missing, or a tensor does not live on a ROCm device, the call fails loudly.  (CPU tensors
never get here: the modules send them down their composed routes, brevitas_amd/_aten.py.)

PyTorch is used here as plumbing only: device memory (torch.empty), the current HIP stream and the
device guard.  Signatures carry raw pointers and sizes.
"""
import ctypes
import functools
import operator
import os
from typing import NamedTuple, Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# BREVITAS_AMD_LIB: developer override to load an experimental build of the same ABI (tools/microbench.py)
LIB_PATH = os.environ.get('BREVITAS_AMD_LIB') or os.path.join(_PKG, 'libbvq.so')

F32, BF16, F16 = 0, 1, 2
ROUND, FLOOR, CEIL, ROUND_TO_ZERO, DPU_ROUND = range(5)
(OP_ROUND, OP_FLOOR, OP_CEIL, OP_ROUND_TO_ZERO, OP_DPU_ROUND, OP_BINARY_SIGN, OP_TERNARY_SIGN,
 OP_ABS) = range(8)
STAT_ABSMAX, STAT_MINMAX = 0, 1
SCALAR_OPMATH, SCALAR_CAST = 0, 1
OUT_DEQUANT, OUT_INT = 0, 1
MATCH_ABS, MATCH_VALUE = 0, 1
MATCH_FIRST = 16  # OR-ed: only the first attaining element, even for a whole-tensor reduction
PRE_NONE, PRE_RELU, PRE_SIGMOID, PRE_TANH = 0, 1, 2, 3
CODES_I32, CODES_I8, CODES_U8 = 0, 1, 2
CLUSTER_FORCE_FALLBACK = 1  # BVQ_CLUSTER_FORCE_FALLBACK: tests only
# the `form` of bvq_absmax_fakequant_cluster_form (developers, tests)
CLUSTER_AUTO, CLUSTER_WALK, CLUSTER_ONESHOT = range(3)
# bvq_mx_format, bvq_mx_scale_rule
MX_E4M3, MX_E5M2, MX_E3M2, MX_E2M3, MX_E2M1, MX_INT8 = range(6)
MX_FLOOR, MX_CEIL = 0, 1
LR_HARD_SIGMOID, LR_SIGMOID = 0, 1  # bvq_learned_round_impl
NORM_L1, NORM_L2 = 0, 1  # bvq_norm_kind
_CODES_TORCH = {CODES_I32: torch.int32, CODES_I8: torch.int8, CODES_U8: torch.uint8}
ABI_VERSION = 12

_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}

class QuantDesc(ctypes.Structure):
    """bvq_quant_desc of include/bvq.h"""
    _fields_ = [
        ('outer', ctypes.c_int64), ('channels', ctypes.c_int64), ('inner', ctypes.c_int64),
        ('x_dtype', ctypes.c_int32), ('ct_dtype', ctypes.c_int32), ('scale_dtype', ctypes.c_int32),
        ('zp_dtype', ctypes.c_int32), ('scale_per_channel', ctypes.c_int32),
        ('zp_per_channel', ctypes.c_int32), ('qmin', ctypes.c_float), ('qmax', ctypes.c_float),
        ('round_mode', ctypes.c_int32), ('scalar_mode', ctypes.c_int32), ('clamp_ste', ctypes.c_int32),
        ('out_kind', ctypes.c_int32), ('pre_op', ctypes.c_int32), ('codes_dtype', ctypes.c_int32)]

    # the integer fields as the C++ autograd node takes and hands back a descriptor (csrc/bvq_autograd.cpp, desc_ints /
    # desc_from: `dv`, in this order; qmin and qmax travel apart, as doubles)
    DV_FIELDS = ('outer', 'channels', 'inner', 'x_dtype', 'ct_dtype', 'scale_dtype', 'zp_dtype', 'scale_per_channel',
                 'zp_per_channel', 'round_mode', 'scalar_mode', 'clamp_ste', 'out_kind', 'pre_op', 'codes_dtype')

    def to_dv(self):
        return _DV_OF(self)

    @classmethod
    def from_dv(cls, dv, qmin, qmax):
        """inverse of to_dv; entries of dv behind the descriptor's 15 are the node's own"""
        return cls(qmin=qmin, qmax=qmax, **dict(zip(cls.DV_FIELDS, dv)))


_DV_OF = operator.attrgetter(*QuantDesc.DV_FIELDS)


class VariantDesc(ctypes.Structure):
    """bvq_variant_desc of include/bvq.h"""
    _fields_ = [
        ('outer', ctypes.c_int64), ('channels', ctypes.c_int64), ('inner', ctypes.c_int64), ('kind', ctypes.c_int32),
        ('x_dtype', ctypes.c_int32), ('ct_dtype', ctypes.c_int32), ('scale_dtype', ctypes.c_int32),
        ('zp_dtype', ctypes.c_int32), ('scale_per_channel', ctypes.c_int32), ('round_mode', ctypes.c_int32),
        ('clamp_ste', ctypes.c_int32), ('scalar_mode', ctypes.c_int32), ('qmin', ctypes.c_float),
        ('qmax', ctypes.c_float), ('threshold', ctypes.c_float), ('trunc_scale', ctypes.c_float)]


VAR_BINARY, VAR_CLAMPED_BINARY, VAR_TERNARY, VAR_DECOUPLED, VAR_TRUNC = range(5)

WEIGHT_LIST_MAX = 16  # BVQ_WEIGHT_LIST_MAX: items per bvq_weight_quant_list_* call


class WeightItem(ctypes.Structure):
    """bvq_weight_item of include/bvq.h"""
    _fields_ = [
        ('x', ctypes.c_void_p), ('y', ctypes.c_void_p), ('stat', ctypes.c_void_p), ('scale', ctypes.c_void_p),
        ('g', ctypes.c_void_p), ('dx', ctypes.c_void_p), ('dscale', ctypes.c_void_p), ('channels', ctypes.c_int64),
        ('inner', ctypes.c_int64), ('min_val', ctypes.c_double), ('int_threshold', ctypes.c_double),
        ('qmin', ctypes.c_float), ('qmax', ctypes.c_float), ('use_min', ctypes.c_int32), ('clamp_ste', ctypes.c_int32)]


class BvqError(RuntimeError):
    pass


# The signature of every entry of include/bvq.h that takes arguments: name -> (restype, argtypes).
# tests/test_cabi_symbols.py holds it against the header's prototypes.
_vp, _i64, _i32, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_qd, _vd = ctypes.POINTER(QuantDesc), ctypes.POINTER(VariantDesc)
_SIG = {
    'bvq_nt_threshold_bytes': (_i64, []),
    'bvq_unary': (_i32, [_i32, _i32, _vp, _vp, _i64, _vp]),
    'bvq_scalar_clamp': (_i32, [_i32, _vp, _vp, _i64, _dbl, _i32, _dbl, _i32, _vp]),
    'bvq_tensor_clamp': (_i32, [_i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    'bvq_tensor_clamp_bwd': (_i32, [_i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    'bvq_abs_binary_sign_grad_bwd': (_i32, [_i32, _vp, _vp, _vp, _i64, _vp]),
    'bvq_stats_workspace_bytes': (_i64, [_i32, _i32, _i64, _i64, _i64]),
    'bvq_stats': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp]),
    'bvq_stats_pre': (_i32, [_i32, _i32, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp]),
    'bvq_stat_bwd': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp]),
    'bvq_fakequant_fwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_stats_fakequant_fwd_workspace_bytes': (_i64, [_qd, _vp, _vp]),
    'bvq_stats_fakequant_fwd': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _i64, _vp]),
    'bvq_fakequant_bwd_workspace_bytes': (_i64, [_qd]),
    'bvq_fakequant_bwd_stats_workspace_bytes': (_i64, [_qd]),
    'bvq_fakequant_bwd_stats': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _vp, _i64, _vp]),
    'bvq_fakequant_bwd_stats_onepass_supported': (_i32, [_qd]),
    'bvq_fakequant_bwd_stats_onepass': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _vp, _i64, _vp, _i64, _vp]),
    'bvq_absmax_scale': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _vp, _dbl, _i32, _dbl, _i32, _vp, _vp, _i64, _vp]),
    'bvq_absmax_scale_running': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _vp, _dbl, _i32, _dbl, _i32, _vp, _i32, _vp, _dbl, _i32, _vp, _i64, _vp]),
    'bvq_absmax_onepass_supported': (_i32, [_i32, _vp, _i64, _i64, _i64]),
    'bvq_absmax_scale_onepass': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _dbl, _i32, _dbl, _i32, _vp, _i32, _vp, _dbl, _i32, _vp, _i64, _vp]),
    'bvq_absmax_list_supported': (_i32, [_i32, _i32, _vp, _vp, _i64, _vp]),
    'bvq_absmax_scale_list': (_i32, [_i32, _i32, _vp, _vp, _i64, _vp, _vp, _dbl, _i32, _dbl, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    'bvq_running_stats_update': (_i32, [_i32, _vp, _i32, _vp, _i64, _dbl, _i32, _vp]),
    'bvq_scale_from_stat': (_i32, [_vp, _i64, _i32, _vp, _dbl, _i32, _dbl, _i32, _vp, _vp]),
    'bvq_scale_from_stat_running': (_i32, [_vp, _i64, _i32, _vp, _dbl, _i32, _dbl, _i32, _vp, _i32, _vp, _dbl, _i32, _vp]),
    'bvq_fakequant_bwd_shard': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _vp]),
    'bvq_shard_unpack_deposit': (_i32, [_i32, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _i64, _i32, _dbl, _i32, _i32, _vp, _vp]),
    'bvq_shard_pack': (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    'bvq_shard_unpack': (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    'bvq_abs_moments_workspace_bytes': (_i64, [_i32, _i64, _i64, _i64]),
    'bvq_abs_moments': (_i32, [_i32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    'bvq_abs_affine_bwd': (_i32, [_i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    'bvq_kth_workspace_bytes': (_i64, [_i32, _i64, _i64, _i64]),
    'bvq_kth_value': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    'bvq_kth_pair': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    'bvq_kth_passes': (_i32, [_i32]),
    'bvq_kth_hist_offset': (_i64, [_i32, _i64, _i32]),
    'bvq_kth_begin': (_i32, [_i32, _i64, _i32, _i64, _dbl, _vp, _i64, _vp]),
    'bvq_kth_hist': (_i32, [_i32, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp]),
    'bvq_kth_pick': (_i32, [_i32, _i64, _i32, _i32, _dbl, _vp, _i64, _vp]),
    'bvq_kth_finish': (_i32, [_i32, _i32, _i64, _vp, _vp, _i64, _vp]),
    'bvq_kthw_plan': (_i32, [_i32, _i32, _i32, _vp, _vp]),
    'bvq_kthw_begin': (_i32, [_i32, _i32, _vp, _i64, _vp]),
    'bvq_kthw_hist': (_i32, [_i32, _i32, _vp, _i64, _i32, _vp, _i64, _vp]),
    'bvq_kthw_pick': (_i32, [_i32, _i32, _i32, _i32, _i64, _dbl, _vp, _i64, _vp]),
    'bvq_kthw_finish': (_i32, [_i32, _i32, _vp, _vp, _i64, _vp]),
    'bvq_tie_info_bytes': (_i64, [_i64]),
    'bvq_stat_tie_scan': (_i32, [_i32, _i32, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    'bvq_stat_tie_apply': (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp]),
    'bvq_stat_tie_apply_dscale': (_i32, [_i32, _i32, _vp, _vp, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    'bvq_fakequant_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'bvq_learned_scale': (_i32, [_i32, _vp, _i64, _dbl, _i32, _dbl, _i32, _vp, _vp]),
    'bvq_histc': (_i32, [_i32, _vp, _i64, _vp, _i32, _vp, _vp]),
    'bvq_selftest_div_f16r': (_i32, [_vp, _i32, _vp, _i32, _vp, _vp]),
    'bvq_selftest_pre_op': (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    'bvq_fakequant_fwd_bounds': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_fakequant_bwd_bounds': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'bvq_variant_fwd': (_i32, [_vd, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_variant_bwd_workspace_bytes': (_i64, [_vd]),
    'bvq_variant_bwd': (_i32, [_vd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'bvq_weight_list_supported': (_i32, [_i32, _i32, _i32, _vp, _i64]),
    'bvq_weight_quant_list_fwd': (_i32, [_i32, _i32, _i32, _i32, _vp, _vp]),
    'bvq_weight_quant_list_bwd_workspace_bytes': (_i64, [_i32, _i32, _vp]),
    'bvq_weight_quant_list_bwd': (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    'bvq_absmax_fakequant_cluster_supported': (_i64, [_qd, _vp, _vp]),
    'bvq_absmax_fakequant_cluster': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _i32, _vp, _dbl, _i32, _vp,
                                            _vp, _i64, _i32, _vp, _vp]),
    'bvq_absmax_fakequant_cluster_form': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _i32, _vp, _dbl, _i32,
                                                 _vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    'bvq_group_quant_supported': (_i32, [_qd, _vp]),
    'bvq_group_quant_fwd': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp]),
    'bvq_group_quant_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _vp, _vp]),
    'bvq_group_mse_supported': (_i32, [_qd, _vp, _i32]),
    'bvq_group_mse_fwd': (_i32, [_qd, _vp, _vp, _i32, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp]),
    'bvq_group_mse_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _dbl, _vp, _vp]),
    'bvq_group_shifted_supported': (_i32, [_qd, _vp]),
    'bvq_group_shifted_fwd': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp]),
    'bvq_group_shifted_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _vp, _vp]),
    'bvq_group_hqo_supported': (_i32, [_qd, _vp, _i32, _i32]),
    'bvq_group_hqo_fwd': (_i32, [_qd, _vp, _vp, _i32, _i32, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_group_hqo_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _vp, _vp]),
    'bvq_group_awq_supported': (_i32, [_qd, _vp, _vp, _vp, _i64, _i32]),
    'bvq_group_awq_fwd': (_i32, [_qd, _vp, _vp, _i64, _i32, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp]),
    'bvq_row_shifted_max_row_bytes': (_i64, []),
    'bvq_row_shifted_supported': (_i32, [_qd, _vp]),
    'bvq_row_shifted_fwd': (_i32, [_qd, _vp, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp]),
    'bvq_row_shifted_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _dbl, _vp, _vp]),
    'bvq_weight_norm_supported': (_i32, [_qd, _i32, _dbl, _dbl, _vp]),
    'bvq_weight_norm_fwd': (_i32, [_qd, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_weight_norm_bwd': (_i32, [_qd, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bvq_gptq_block_supported': (_i32, [_qd, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    'bvq_gptq_block': (_i32, [_qd, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp]),
    'bvq_gpfq_block_supported': (_i32, [_qd, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    'bvq_gpfq_block': (_i32, [_qd, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    'bvq_learned_round_supported': (_i32, [_qd, _vp, _vp, _vp]),
    'bvq_learned_round_fwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _i32, _dbl, _dbl, _i32, _vp, _vp]),
    'bvq_learned_round_bwd': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _vp]),
    'bvq_mx_quant_supported': (_i32, [_i32, _i64, _i32, _i32, _vp]),
    'bvq_mx_quant_fwd': (_i32, [_i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    'bvq_mx_quant_bwd': (_i32, [_i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    'bvq_mx_encode_supported': (_i32, [_i32, _i64, _i32, _i32, _vp]),
    'bvq_mx_encode': (_i32, [_i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    'bvq_mx_decode': (_i32, [_i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    'bvq_hadamard_supported': (_i32, [_i32, _i64, _i64, _i64, _vp, _vp]),
    'bvq_hadamard': (_i32, [_i32, _vp, _i64, _i64, _i64, _dbl, _vp, _vp]),
    'bvq_fakequant_bwd_learned': (_i32, [_qd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _dbl, _i32, _dbl, _vp, _vp, _vp, _i64, _vp]),
}

EXPORTS = ('bvq_abi_version', 'bvq_last_error') + tuple(_SIG)

TORCH_DTYPES = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


def _load(path=None, strict=True):
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            'brevitas_amd: %s is missing. Build it with `python -m brevitas_amd.csrc.build` '
            '(needs hipcc, gfx950). There is no fallback backend.' % path)
    lib = ctypes.CDLL(path)
    lib.bvq_abi_version.restype = _i32
    lib.bvq_last_error.restype = ctypes.c_char_p
    for name, (res, args) in _SIG.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if strict:
                raise ImportError('brevitas_amd: %s does not export %s' % (path, name))
            continue  # developer A/B runs against an older build (tools/variant_bench.py)
        fn.restype = res
        fn.argtypes = args
    ver = lib.bvq_abi_version()
    if ver != ABI_VERSION:
        raise ImportError('brevitas_amd: libbvq.so has ABI %d, this package needs %d' % (ver, ABI_VERSION))
    return lib


lib = _load()


def last_error():
    return lib.bvq_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise BvqError('%s failed (%d): %s' % (what, rc, last_error()))


def dtype_code(dtype):
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise BvqError('brevitas_amd: unsupported dtype %s (float32, bfloat16, float16)' % dtype)


def require_device(*tensors):
    """every tensor must live on the same ROCm device; no CPU path exists"""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise BvqError(
                'brevitas_amd: got a %s tensor; the fake-quantization engine only runs on a ROCm '
                'device (there is no CPU fallback)' % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise BvqError('brevitas_amd: tensors on different devices (%s, %s)' % (dev, t.device))
    return dev


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device):
    """the current HIP stream of `device` as the void* the C ABI takes"""
    if _raw_stream is not None:  # no Stream object construction on the hot path
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    """raw device address (ctypes converts the int for the c_void_p parameters)"""
    return t.data_ptr() if t is not None else None


class _DeviceGuard:
    """`with torch.cuda.device(dev)` only when dev is not already current (the common case costs one call); yields the
    current stream of dev, for a wrapper that needs it before its launch: `with _DeviceGuard(dev) as st:`, the arrival
    buffer asked for and `_call(..., st)` made inside"""
    __slots__ = ('ctx', 'dev')

    def __init__(self, dev):
        idx = dev.index
        self.ctx = None if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(dev)
        self.dev = dev

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
        return stream_ptr(self.dev)

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# Optional measurement hook (bench.py): an object with before(name) / after(name), called around the
# C-ABI calls that name a bracket (_launch / _call) on the launching thread, e.g. to record HIP events on the current
# stream.
_timer = None


def set_kernel_timer(timer):
    global _timer
    _timer = timer


def _call(name, bracket, *args):
    """One C-ABI call on the current device: lib.<name>(*args), the stream already last in args; a non-zero return
    raises BvqError naming the entry.  bracket: the name the kernel timer, if one is set, sees before and after the
    call (a failing call raises before after()); None: the call is not timed.  Called by _launch, and directly by the
    wrappers that hold a guard and its stream for their arrival buffer: `with _DeviceGuard(dev) as st:`."""
    if bracket is not None and _timer is not None:
        _timer.before(bracket)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        check(rc, name)
    if bracket is not None and _timer is not None:
        _timer.after(bracket)


def _launch(dev, name, bracket, *args):
    """One launching C-ABI call, the whole protocol: _call on dev with dev's current stream as the last argument, where
    every launching entry of include/bvq.h takes it.  (dev already current, the common case, costs one query.)"""
    idx = dev.index
    if idx is not None and idx != torch.cuda.current_device():
        with _DeviceGuard(dev) as stream:
            return _call(name, bracket, *args, stream)
    _call(name, bracket, *args, stream_ptr(dev))


def _workspace(dev, query, *args, floor=0):
    """ask lib.<query>(*args) for a workspace size -> (uint8 tensor of max(size, floor) bytes, size)"""
    wsb = int(getattr(lib, query)(*args))
    if wsb < 0:
        raise BvqError('%s: %s' % (query, last_error()))
    return torch.empty(max(wsb, floor), dtype=torch.uint8, device=dev), wsb


def _scale_args(min_val, int_threshold):
    """(min_val, use_min, int_threshold) of a scale epilogue: no clamp_min for a min_val of None or 0"""
    if min_val:
        return float(min_val), 1, float(int_threshold)
    return 0.0, 0, float(int_threshold)


def _running_args(running, momentum, first_batch):
    """(run_dtype, running, momentum, first_batch) of a running statistic; running None: none is kept"""
    return dtype_code(running.dtype) if running is not None else 0, ptr(running), float(momentum), int(first_batch)


# ---- arrival buffers of the one-launch kernels --------------------------------------------------------------------
# include/bvq.h, bvq_absmax_scale_onepass: per-channel key / counter words that are zero when a launch starts and that
# the launch hands back as zeros.  One buffer per (device, stream), zero-filled once when it is allocated; launches
# on one stream are ordered, so they can share it.  Not allocated while a stream is capturing (the capture would
# own the memory): those calls take the two-launch route.
ARRIVE_WORDS = 1 << 16
_arrive = {}
ONEPASS = True       # the one-launch routes (tests and tools/onepass_ab.py switch them off for A/B runs)
ONEPASS_BWD = True   # the one-launch backward alone


def arrival_buffer(dev, stream, words):
    """-> int32 tensor of >= words zeros for this device and stream, or None (capturing / switched off)"""
    if not ONEPASS or words > ARRIVE_WORDS:
        return None
    key = (dev.index, stream)
    buf = _arrive.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        buf = _arrive[key] = torch.zeros(ARRIVE_WORDS, dtype=torch.int32, device=dev)
    return buf


# ---- thin wrappers: allocate outputs with torch, pass raw pointers --------------------------------

def unary(op, x):
    dev = require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _launch(dev, 'bvq_unary', None, op, dtype_code(x.dtype), ptr(x), ptr(y), x.numel())
    return y


def scalar_clamp(x, lo, hi):
    dev = require_device(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _launch(dev, 'bvq_scalar_clamp', None, dtype_code(x.dtype), ptr(x), ptr(y), x.numel(),
            0.0 if lo is None else float(lo), int(lo is not None), 0.0 if hi is None else float(hi),
            int(hi is not None))
    return y


def _bounds(x, lo, hi):
    """bring clamp bounds to x's dtype/device; returns (lo, hi, bounds_full)"""
    lo = lo.to(device=x.device, dtype=x.dtype)
    hi = hi.to(device=x.device, dtype=x.dtype)
    if lo.numel() == 1 and hi.numel() == 1:
        return lo.reshape(1), hi.reshape(1), 0
    return lo.expand_as(x).contiguous(), hi.expand_as(x).contiguous(), 1


def tensor_clamp(x, lo, hi, out=None):
    dev = require_device(x)
    xc = x.contiguous()
    lo, hi, full = _bounds(xc, lo, hi)
    y = out if out is not None else torch.empty_like(xc)
    _launch(dev, 'bvq_tensor_clamp', None, dtype_code(xc.dtype), ptr(xc), ptr(lo), ptr(hi), full, ptr(y), xc.numel())
    return y


def tensor_clamp_bwd(g, x, lo, hi):
    dev = require_device(g, x)
    xc = x.contiguous()
    g = g.to(xc.dtype).contiguous()
    lo, hi, full = _bounds(xc, lo, hi)
    dx = torch.empty_like(xc)
    _launch(dev, 'bvq_tensor_clamp_bwd', None, dtype_code(xc.dtype), ptr(g), ptr(xc), ptr(lo), ptr(hi), full, ptr(dx),
            xc.numel())
    return dx


def abs_binary_sign_grad_bwd(g, x):
    dev = require_device(g, x)
    xc = x.contiguous()
    g = g.to(xc.dtype).contiguous()
    dx = torch.empty_like(xc)
    _launch(dev, 'bvq_abs_binary_sign_grad_bwd', None, dtype_code(xc.dtype), ptr(g), ptr(xc), ptr(dx), xc.numel())
    return dx


def _absmax_onepass(dev, pre_op, x, outer, channels, inner, stat, min_val=None, int_threshold=1.0, scale=None,
                    running=None, momentum=0.0, first_batch=False):
    """the one-launch abs-max (the statistic kernel's last-arriving wave per channel finishes it) into `stat`, where
    the layout is covered and an arrival buffer is to be had -> whether it was launched; if not, the caller takes the
    two-launch route.  scale: None, or the tensor that takes clamp_min(stat, min_val) / int_threshold; running: None,
    or the running statistic folded with `stat` in the same launch"""
    dt = dtype_code(x.dtype)
    if pre_op not in (PRE_NONE, PRE_RELU) or not lib.bvq_absmax_onepass_supported(dt, ptr(x), outer, channels, inner):
        return False
    with _DeviceGuard(dev) as st:
        arrive = arrival_buffer(dev, st, max(2 * channels, 18))
        if arrive is None:
            return False
        _call('bvq_absmax_scale_onepass', 'bvq_stats', pre_op, dt, ptr(x), outer, channels, inner,
              dtype_code(stat.dtype), ptr(stat), *_scale_args(min_val, int_threshold),
              dtype_code(scale.dtype) if scale is not None else 0, ptr(scale),
              *_running_args(running, momentum, first_batch), ptr(arrive), arrive.numel(), st)
    return True


def stats(kind, x, outer, channels, inner, out_f32=False, pre_op=PRE_NONE):
    """x contiguous, viewed as [outer, channels, inner] -> [channels] (ABSMAX) or [2, channels]"""
    dev = require_device(x)
    assert x.is_contiguous() and x.numel() == outer * channels * inner
    dt = dtype_code(x.dtype)
    nout = channels * (2 if kind == STAT_MINMAX else 1)
    out = torch.empty(nout, dtype=torch.float32 if out_f32 else x.dtype, device=dev)
    if kind == STAT_ABSMAX and _absmax_onepass(dev, pre_op, x, outer, channels, inner, out):
        return out
    ws, _ = _workspace(dev, 'bvq_stats_workspace_bytes', kind, dt, outer, channels, inner, floor=8)
    _launch(dev, 'bvq_stats_pre', 'bvq_stats', kind, pre_op, dt, ptr(x), outer, channels, inner, dtype_code(out.dtype),
            ptr(out), ptr(ws), ws.numel())
    return out


def stat_bwd(match, x, stat, gstat, outer, channels, inner, dx=None):
    """dense (dx None) or in-place additive (dx given) backward of a max/min statistic"""
    dev = require_device(x, stat, gstat, dx)
    assert x.is_contiguous()
    dt = dtype_code(x.dtype)
    stat = stat.to(x.dtype).contiguous()
    gstat = gstat.to(x.dtype).contiguous()
    mode_add = int(dx is not None)
    if dx is None:
        dx = torch.empty_like(x)
    assert dx.is_contiguous() and dx.dtype == x.dtype
    ws, _ = _workspace(dev, 'bvq_stats_workspace_bytes', STAT_ABSMAX, dt, outer, channels, inner, floor=8)
    _launch(dev, 'bvq_stat_bwd', None, match, dt, ptr(x), ptr(stat), ptr(gstat), ptr(dx), outer, channels, inner,
            mode_add, ptr(ws), ws.numel())
    return dx


def fakequant_fwd(desc, x, scale, zp, want_codes=False, want_y=True):
    """-> y, (y, codes) or codes alone; codes have the element type of desc.codes_dtype"""
    dev = require_device(x, scale, zp)
    y = torch.empty(x.shape, dtype=TORCH_DTYPES[desc.ct_dtype], device=dev) if want_y else None
    codes = torch.empty(x.shape, dtype=_CODES_TORCH[desc.codes_dtype], device=dev) if want_codes else None
    _launch(dev, 'bvq_fakequant_fwd', 'bvq_fakequant_fwd', ctypes.byref(desc), ptr(x), ptr(scale), ptr(zp), ptr(y),
            ptr(codes))
    if not want_y:
        return codes
    return (y, codes) if want_codes else y


def stats_fakequant_fwd(desc, x, min_val, int_threshold, scale_dtype):
    """abs-max statistic, scale and quantize-dequantize in ONE launch (x read once) -> (stat, scale, y), or
    None when the shape is not covered by that kernel (the caller takes the two-call route)"""
    dev = require_device(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    wsb = int(lib.bvq_stats_fakequant_fwd_workspace_bytes(ctypes.byref(desc), ptr(x), ptr(y)))
    if wsb <= 0:
        return None
    channels = int(desc.channels) if (desc.scale_per_channel and desc.channels > 1) else 1
    stat = torch.empty(channels, dtype=x.dtype, device=dev)
    scale = torch.empty(channels, dtype=scale_dtype, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _launch(dev, 'bvq_stats_fakequant_fwd', 'bvq_stats_fakequant_fwd', ctypes.byref(desc), ptr(x),
            *_scale_args(min_val, int_threshold), ptr(stat), ptr(scale), ptr(y), ptr(ws), wsb)
    return stat, scale, y


# ---- the per-unit families: one value per group or per row, one launch each way ---------------------------------
# A unit is a group of consecutive elements or a row; the descriptor has outer 1, channels = units, inner = the unit's
# length.  Every family has three entries, bvq_<stem>_supported / _fwd / _bwd, with one argument order (include/bvq.h):
#   fwd: desc, x, [extra], min_val, use_min, int_threshold, y, the per-unit outputs
#   bwd: desc, g, x, the saved per-unit outputs, the side gradients, [extra], min_val, use_min, int_threshold, dx
# The public wrappers take their arguments in that order too, so the plain ones ARE the generic wrapper with the
# family bound (functools.partial: no frame of their own on the path of every layer and step).  DESIGN.md §9 has the
# table in words.

class UnitOut(NamedTuple):
    name: str
    per_unit: int = 1                      # elements per unit
    dtype: Optional[torch.dtype] = None    # None: x's


class UnitFamily(NamedTuple):
    supported: str        # the three entries, spelled out so that a search for an entry finds its family; the
    fwd: str              # wrappers of this module have their names without the bvq_
    bwd: str
    outs: tuple           # UnitOuts the forward writes after y, in header order
    saved: tuple          # names of those the backward takes after x, in header order
    side: tuple           # the gradients that follow them, each None or [units] in x's dtype
    extra: tuple = ()     # host arguments in front of the scale arguments, both ways
    bwd_extra: Optional[tuple] = None   # the backward's, where they differ from the forward's (None: `extra`)
    # what the Functions of core/quant/_fused.py read
    zp_per_unit: bool = False   # the descriptor has one zero-point per unit, in x's dtype
    align_side: bool = False    # the .hip file's group_aligned: side gradients must sit on 16-byte boundaries


_SHIFTED_OUTS = (UnitOut('scale'), UnitOut('zp'), UnitOut('stat', 2))  # stat: the maxima, then the minima
GROUP_QUANT = UnitFamily('bvq_group_quant_supported', 'bvq_group_quant_fwd', 'bvq_group_quant_bwd',
                         (UnitOut('scale'), UnitOut('stat')), ('scale', 'stat'), ('gscale',))
GROUP_MSE = UnitFamily('bvq_group_mse_supported', 'bvq_group_mse_fwd', 'bvq_group_mse_bwd',
                       (UnitOut('scale'), UnitOut('stat'), UnitOut('idx', 1, torch.uint8)), ('stat', 'idx'), ('gscale',),
                       extra=('ratios', 'n_ratios'))
GROUP_SHIFTED = UnitFamily('bvq_group_shifted_supported', 'bvq_group_shifted_fwd', 'bvq_group_shifted_bwd',
                           _SHIFTED_OUTS, ('stat',), ('gscale', 'gzp'), zp_per_unit=True)
ROW_SHIFTED = UnitFamily('bvq_row_shifted_supported', 'bvq_row_shifted_fwd', 'bvq_row_shifted_bwd',
                         _SHIFTED_OUTS, ('stat',), ('gscale', 'gzp'), zp_per_unit=True, align_side=True)
UNIT_FAMILIES = (GROUP_QUANT, GROUP_MSE, GROUP_SHIFTED, ROW_SHIFTED)
# GROUP_SHIFTED with a searched zero-point.  The same record type, served by the same unit_fwd / unit_bwd, but kept out
# of UNIT_FAMILIES: that tuple is the set of families whose public wrappers ARE the generic ones and whose Functions
# return every per-unit output shaped [units, 1] and differentiable, which tests/test_unit_families_host.py walks; this
# family's zero-point and index are constants of the backward and its backward takes none of the forward's host
# arguments (bwd_extra), so tests/test_group_hqo_host.py holds its record on its own.
GROUP_HQO = UnitFamily('bvq_group_hqo_supported', 'bvq_group_hqo_fwd', 'bvq_group_hqo_bwd',
                       _SHIFTED_OUTS + (UnitOut('idx', 1, torch.uint8),), ('stat', 'zp'), ('gscale',),
                       extra=('inv_beta', 'n_iters', 'lp'), bwd_extra=(), zp_per_unit=True)


def unit_supported(fam, desc, x, *extra):
    """the family's kernels cover this descriptor, tensor and extra arguments"""
    return bool(getattr(lib, fam.supported)(ctypes.byref(desc), ptr(x), *extra))


def unit_fwd(fam, desc, x, *rest):
    """statistic per unit, scale (zero-point) and quantize-dequantize in ONE launch -> (y like x, *fam.outs), an output
    of `per_unit` elements per unit flat.  rest: fam.extra, min_val, thr_div"""
    dev = require_device(x)
    assert x.is_contiguous() and len(rest) == len(fam.extra) + 2
    units, dt = int(desc.channels), x.dtype
    res = [torch.empty_like(x)]
    for _, per_unit, dtype in fam.outs:
        res.append(torch.empty(per_unit * units, dtype=dtype or dt, device=dev))
    _launch(dev, fam.fwd, fam.fwd, ctypes.byref(desc), ptr(x), *rest[:-2], *_scale_args(rest[-2], rest[-1]),
            *map(ptr, res))
    return tuple(res)


def unit_bwd(fam, desc, g, x, *rest):
    """backward of unit_fwd in ONE launch -> dx (each statistic's gradient of every unit deposited on the first element
    attaining it).  rest: the tensors of fam.saved, the gradients of fam.side that arrived through the per-unit outputs
    (None: none did), fam.extra, min_val, thr_div"""
    n = len(fam.saved) + len(fam.side)
    assert len(rest) == n + len(fam.extra if fam.bwd_extra is None else fam.bwd_extra) + 2
    tensors = rest[:n]
    dev = require_device(g, x, *tensors)
    assert g.is_contiguous() and x.is_contiguous()
    for t in tensors:
        assert t is None or t.is_contiguous()
    dx = torch.empty_like(x)
    _launch(dev, fam.bwd, fam.bwd, ctypes.byref(desc), ptr(g), ptr(x), *map(ptr, tensors), *rest[n:-2],
            *_scale_args(rest[-2], rest[-1]), ptr(dx))
    return dx


# (desc, x): outer 1, channels = groups, inner = group size
group_quant_supported = functools.partial(unit_supported, GROUP_QUANT)
# (desc, x, min_val, thr_div): abs-max per group -> (y, scale [groups], stat [groups])
group_quant_fwd = functools.partial(unit_fwd, GROUP_QUANT)
# (desc, g, x, scale, stat, gscale, min_val, thr_div) -> dx
group_quant_bwd = functools.partial(unit_bwd, GROUP_QUANT)


def mse_ratio_table(ratios):
    """the host array of float32 candidate ratios that the bvq_group_mse_* entries take (keep it alive over the call)"""
    return (ctypes.c_float * len(ratios))(*[float(r) for r in ratios])


def group_mse_supported(desc, x, n_ratios):
    """as group_quant_supported, and the candidate count"""
    return unit_supported(GROUP_MSE, desc, x, int(n_ratios))


def group_mse_fwd(desc, x, table, min_val, thr_div):
    """abs-max per group and the search over the candidate thresholds abs-max * table[i] -> (y, scale [groups],
    stat [groups], idx uint8 [groups]: the chosen candidate)"""
    return unit_fwd(GROUP_MSE, desc, x, ctypes.addressof(table), len(table), min_val, thr_div)


def group_mse_bwd(desc, g, x, stat, idx, gscale, table, min_val, thr_div):
    """idx is a constant; the statistic's gradient is scaled by the chosen ratio"""
    assert idx.dtype == torch.uint8
    return unit_bwd(GROUP_MSE, desc, g, x, stat, idx, gscale, ctypes.addressof(table), len(table), min_val, thr_div)


# as group_quant_*, with one zero-point per group in x's dtype: max and min per group, integer zero-point
# fwd -> (y, scale [groups], zp [groups], stat [2 * groups]);  bwd (desc, g, x, stat, gscale, gzp, min_val, thr_div)
group_shifted_supported = functools.partial(unit_supported, GROUP_SHIFTED)
group_shifted_fwd = functools.partial(unit_fwd, GROUP_SHIFTED)
group_shifted_bwd = functools.partial(unit_bwd, GROUP_SHIFTED)


HQO_LP = {1.0: 0, 0.5: 1}   # the `lp` codes of the bvq_group_hqo_* entries: the norms their kernels are built for
HQO_MAX_ITERS = 63


def hqo_beta_table(beta, kappa, n_iters):
    """the host array float32(1 / (beta * kappa^i)), i = 0 .. n_iters, that bvq_group_hqo_fwd takes: each entry formed
    in double precision and rounded once (keep it alive over the call)"""
    return (ctypes.c_float * (int(n_iters) + 1))(*[1.0 / (float(beta) * float(kappa) ** i)
                                                   for i in range(int(n_iters) + 1)])


def group_hqo_supported(desc, x, n_iters, lp):
    """as group_shifted_supported, and the iteration count and the norm's code"""
    return unit_supported(GROUP_HQO, desc, x, int(n_iters), int(lp))


def group_hqo_fwd(desc, x, table, lp, min_val, thr_div):
    """the statistics of group_shifted_fwd and the zero-point search of len(table) - 1 proximal steps -> (y, scale
    [groups], zp [groups]: the kept zero-point, stat [2 * groups], idx uint8 [groups]: the kept candidate)"""
    return unit_fwd(GROUP_HQO, desc, x, ctypes.addressof(table), len(table) - 1, int(lp), min_val, thr_div)


def group_hqo_bwd(desc, g, x, stat, zp, gscale, min_val, thr_div):
    """zp is a constant: dx and the scale statistics' gradients at (scale, zp)"""
    return unit_bwd(GROUP_HQO, desc, g, x, stat, zp, gscale, min_val, thr_div)


AWQ_MAX_CANDIDATES = 64


def group_awq_supported(desc, x, table, y=None):
    """the AWQ candidates kernel covers this descriptor (that of group_quant_* or of group_shifted_*), the weight x
    [R, K] and the column factors table [n, K]; y: the output, where it exists already"""
    if table.dim() != 2 or not (x.is_contiguous() and table.is_contiguous()) or table.dtype != x.dtype:
        return False
    n, k = table.shape
    return bool(lib.bvq_group_awq_supported(ctypes.byref(desc), ptr(x), ptr(table), ptr(y), int(k), int(n)))


def group_awq_fwd(desc, x, table, min_val, thr_div):
    """every candidate of table [n, K] in ONE launch: scale the columns of x [R, K], group-quantize, unscale ->
    (y [n, *x.shape], scale [n, groups], zp [n, groups] or None where the descriptor has no zero-point per group)"""
    dev = require_device(x, table)
    assert x.is_contiguous() and table.is_contiguous() and table.dim() == 2 and table.dtype == x.dtype
    n, k = table.shape
    groups = int(desc.channels)
    y = torch.empty((n,) + tuple(x.shape), dtype=x.dtype, device=dev)
    scale = torch.empty(n, groups, dtype=x.dtype, device=dev)
    zp = torch.empty(n, groups, dtype=x.dtype, device=dev) if desc.zp_per_channel else None
    _launch(dev, 'bvq_group_awq_fwd', 'bvq_group_awq_fwd', ctypes.byref(desc), ptr(x), ptr(table), int(k), int(n),
            *_scale_args(min_val, thr_div), ptr(y), ptr(scale), ptr(zp))
    return y, scale, zp


def row_shifted_max_row_bytes():
    """the longest row, in bytes, the asymmetric per-row kernels hold"""
    return int(lib.bvq_row_shifted_max_row_bytes())


# group_shifted_* with a row in the place of a group: outer 1, channels = rows, inner = H
row_shifted_supported = functools.partial(unit_supported, ROW_SHIFTED)
row_shifted_fwd = functools.partial(unit_fwd, ROW_SHIFTED)
row_shifted_bwd = functools.partial(unit_bwd, ROW_SHIFTED)


def weight_norm_supported(desc, norm_kind, t_bound, norm_min, x):
    """the weight-norm kernels cover this descriptor (outer 1, channels = rows, inner = K, float32 arithmetic and
    scales, a narrow signed range, round-to-zero with NORM_L1 and half-even with NORM_L2), scalars and tensor"""
    return bool(lib.bvq_weight_norm_supported(ctypes.byref(desc), int(norm_kind), float(t_bound), float(norm_min),
                                              ptr(x)))


def weight_norm_fwd(desc, norm_kind, t_bound, norm_min, x, scale, g):
    """norm per row, pre-scale, quantize-dequantize in ONE launch -> (y like x, norm float32 [rows]); scale, g: float32
    [rows]"""
    dev = require_device(x, scale, g)
    assert x.is_contiguous() and scale.is_contiguous() and g.is_contiguous()
    assert scale.dtype == g.dtype == torch.float32 and scale.numel() == g.numel() == int(desc.channels)
    y = torch.empty_like(x)
    norm = torch.empty(int(desc.channels), dtype=torch.float32, device=dev)
    _launch(dev, 'bvq_weight_norm_fwd', 'bvq_weight_norm_fwd', ctypes.byref(desc), int(norm_kind), float(t_bound),
            float(norm_min), ptr(x), ptr(scale), ptr(g), ptr(y), ptr(norm))
    return y, norm


def weight_norm_bwd(desc, norm_kind, t_bound, norm_min, gy, x, scale, g, norm):
    """backward of weight_norm_fwd in ONE launch -> (dx like x, dscale, dg: float32 [rows])"""
    dev = require_device(gy, x, scale, g, norm)
    assert gy.is_contiguous() and x.is_contiguous() and gy.dtype == x.dtype
    assert scale.is_contiguous() and g.is_contiguous() and norm.is_contiguous()
    assert scale.dtype == g.dtype == norm.dtype == torch.float32
    assert scale.numel() == g.numel() == norm.numel() == int(desc.channels)
    dx = torch.empty_like(x)
    dscale = torch.empty(int(desc.channels), dtype=torch.float32, device=dev)
    dg = torch.empty(int(desc.channels), dtype=torch.float32, device=dev)
    _launch(dev, 'bvq_weight_norm_bwd', 'bvq_weight_norm_bwd', ctypes.byref(desc), int(norm_kind), float(t_bound),
            float(norm_min), ptr(gy), ptr(x), ptr(scale), ptr(g), ptr(norm), ptr(dx), ptr(dscale), ptr(dg))
    return dx, dscale, dg


def hadamard_supported(x, rows, cols, block, out=None):
    """the Hadamard kernel covers x viewed [rows, cols] (contiguous) with blocks of `block`, written to out (x: in place)"""
    out = x if out is None else out
    return x.dtype in _DTYPES and out.dtype == x.dtype and \
        bool(lib.bvq_hadamard_supported(dtype_code(x.dtype), int(rows), int(cols), int(block), ptr(x), ptr(out)))


def hadamard(x, rows, cols, block, scale, out=None):
    """out = float32(scale) * (I (x) H_block) x along the rows of x viewed [rows, cols], ONE launch -> out (a new tensor
    like x when None; out may be x: a row is whole in registers between its load and its store)"""
    dev = require_device(x, out)
    if out is None:
        out = torch.empty_like(x)
    assert x.is_contiguous() and out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
    assert x.numel() == int(rows) * int(cols)
    _launch(dev, 'bvq_hadamard', 'bvq_hadamard', dtype_code(x.dtype), ptr(x), int(rows), int(cols), int(block),
            float(scale), ptr(out))
    return out


COLUMN_BLOCK = 128  # columns of one launch of a column-loop kernel (bvq_gptq_block, bvq_gpfq_block)


def _column_block(entry, desc, wf, mats, col0, block_cols, scalars, q, scale, zp):
    """what gptq_block and gpfq_block share: wf and `mats` (float32, contiguous; the last one [cols, cols], those before
    it shaped like wf) go in in that order, `scalars` between the block and the outputs -> err float32 [rows, block_cols]"""
    dev = require_device(wf, *mats, q, scale, zp)
    rows, cols = wf.shape
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (wf, *mats))
    assert all(t.shape == wf.shape for t in mats[:-1]) and mats[-1].shape == (cols, cols)
    assert q.is_contiguous() and q.shape == wf.shape and scale.is_contiguous() and (zp is None or zp.is_contiguous())
    err = torch.empty(rows, block_cols, dtype=torch.float32, device=dev)
    _launch(dev, entry, entry, ctypes.byref(desc), ptr(wf), *map(ptr, mats), rows, cols, int(col0), int(block_cols),
            *scalars, ptr(q), ptr(err), ptr(scale), ptr(zp))
    return err


def gptq_block_supported(desc, wf, u, q, col0, block_cols, computed):
    """the GPTQ column-loop kernel covers this descriptor (that of the group-wise entries for the weight [rows, cols]
    regrouped by the group size), block and tensors"""
    rows, cols = wf.shape
    return bool(lib.bvq_gptq_block_supported(ctypes.byref(desc), rows, cols, int(col0), int(block_cols), int(computed),
                                             ptr(wf), ptr(u), ptr(q)))


def gptq_block(desc, wf, u, col0, block_cols, computed, min_val, thr_div, q, scale, zp):
    """the GPTQ column loop of the block [col0, col0 + block_cols) in ONE launch (include/bvq.h, "GPTQ"): reads wf
    (float32 [rows, cols]) and u (float32 [cols, cols]), writes the block's columns of q (like wf, in the quantizer's
    dtype) and, computed, the block's entries of scale / zp ([rows, cols / group size]; given, they are read; zp None for
    a symmetric quantizer) -> err float32 [rows, block_cols]"""
    return _column_block('bvq_gptq_block', desc, wf, (u,), col0, block_cols,
                         (int(computed), *_scale_args(min_val, thr_div)), q, scale, zp)


def gpfq_block_supported(desc, wf, c, h, q, col0, block_cols):
    """the GPFQ column-loop kernel covers this descriptor (that of gptq_block with given parameters), block and
    tensors"""
    rows, cols = wf.shape
    return bool(lib.bvq_gpfq_block_supported(ctypes.byref(desc), rows, cols, int(col0), int(block_cols), ptr(wf),
                                             ptr(c), ptr(h), ptr(q)))


def gpfq_block(desc, wf, c, h, col0, block_cols, q, scale, zp):
    """the GPFQ column loop of the block [col0, col0 + block_cols) in ONE launch (include/bvq.h, "GPFQ"): reads wf and c
    (float32 [rows, cols]), h (float32 [cols, cols]) and scale / zp ([rows, cols / group size]; zp None for a symmetric
    quantizer), writes the block's columns of q (like wf, in the quantizer's dtype) -> err float32 [rows, block_cols]"""
    return _column_block('bvq_gpfq_block', desc, wf, (c, h), col0, block_cols, (), q, scale, zp)


def learned_round_supported(desc, x, value):
    """the learned-round kernels cover this descriptor (that of fakequant_fwd) and these tensors"""
    return bool(lib.bvq_learned_round_supported(ctypes.byref(desc), ptr(x), ptr(value), None))


def learned_round_fwd(desc, x, value, scale, zp, impl, consts, hard):
    """IntQuant with floor(t) + h(value) in ONE launch (include/bvq.h, "Learned rounding") -> y like x; hard: h is 0 or 1
    (eval mode); consts: (c0, c1) of the impl"""
    dev = require_device(x, value, scale, zp)
    assert x.is_contiguous() and value.is_contiguous() and value.dtype == x.dtype and value.numel() == x.numel()
    y = torch.empty_like(x)
    _launch(dev, 'bvq_learned_round_fwd', 'bvq_learned_round_fwd', ctypes.byref(desc), ptr(x), ptr(value), ptr(scale),
            ptr(zp), int(impl), float(consts[0]), float(consts[1]), int(bool(hard)), ptr(y))
    return y


def learned_round_bwd(desc, g, x, value, scale, zp, impl, consts, want_dx):
    """backward of learned_round_fwd (soft h) in ONE launch -> (dvalue like value, dx like x or None)"""
    dev = require_device(g, x, value, scale, zp)
    assert g.is_contiguous() and x.is_contiguous() and value.is_contiguous() and g.dtype == x.dtype == value.dtype
    dvalue = torch.empty_like(value)
    dx = torch.empty_like(x) if want_dx else None
    _launch(dev, 'bvq_learned_round_bwd', 'bvq_learned_round_bwd', ctypes.byref(desc), ptr(g), ptr(x), ptr(value),
            ptr(scale), ptr(zp), int(impl), float(consts[0]), float(consts[1]), ptr(dvalue), ptr(dx))
    return dvalue, dx


def mx_quant_supported(x, group_size, fmt):
    """the MX kernels cover this tensor (dtype, whole groups, 16-byte aligned), group size and format"""
    code = _DTYPES.get(x.dtype)
    if code is None or x.numel() == 0 or x.numel() % group_size:
        return False
    return bool(lib.bvq_mx_quant_supported(code, x.numel() // group_size, int(group_size), int(fmt), ptr(x)))


def mx_quant_fwd(x, group_size, fmt, scale_rule):
    """MX block-scaled quantize-dequantize in ONE launch -> (y like x, float32 scale [groups])"""
    dev = require_device(x)
    assert x.is_contiguous() and x.numel() % group_size == 0
    groups = x.numel() // group_size
    y = torch.empty_like(x)
    scale = torch.empty(groups, dtype=torch.float32, device=dev)
    _launch(dev, 'bvq_mx_quant_fwd', 'bvq_mx_quant_fwd', dtype_code(x.dtype), groups, int(group_size), int(fmt),
            int(scale_rule), ptr(x), ptr(y), ptr(scale))
    return y, scale


def mx_quant_bwd(g, x, gscale, group_size, fmt, scale_rule, clamp_ste):
    """backward of mx_quant_fwd in ONE launch -> dx; gscale: None, or the float32 [groups] gradient arriving through the
    returned scale.  The group's abs-max and exponent are recomputed from x."""
    dev = require_device(g, x, gscale)
    assert g.is_contiguous() and x.is_contiguous() and g.dtype == x.dtype
    assert gscale is None or (gscale.is_contiguous() and gscale.dtype == torch.float32)
    dx = torch.empty_like(x)
    _launch(dev, 'bvq_mx_quant_bwd', 'bvq_mx_quant_bwd', dtype_code(x.dtype), x.numel() // group_size, int(group_size),
            int(fmt), int(scale_rule), int(bool(clamp_ste)), ptr(g), ptr(x), ptr(gscale), ptr(dx))
    return dx


MX_CODE_BITS = (8, 8, 6, 6, 4, 8)  # per bvq_mx_format


def mx_encode(x, group_size, fmt, scale_rule, codes=None, scale_e8m0=None):
    """packed MX element codes and E8M0 scale bytes of x in ONE launch -> (uint8 codes [numel * bits / 8], uint8 scale
    bytes [groups]); codes / scale_e8m0: contiguous uint8 outputs of exactly those sizes to write into"""
    dev = require_device(x, codes, scale_e8m0)
    assert x.is_contiguous() and x.numel() % group_size == 0
    groups = x.numel() // group_size
    nbytes = x.numel() * MX_CODE_BITS[fmt] // 8
    if codes is None:
        codes = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if scale_e8m0 is None:
        scale_e8m0 = torch.empty(groups, dtype=torch.uint8, device=dev)
    for t, n in ((codes, nbytes), (scale_e8m0, groups)):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n
    _launch(dev, 'bvq_mx_encode', 'bvq_mx_encode', dtype_code(x.dtype), groups, int(group_size), int(fmt),
            int(scale_rule), ptr(x), ptr(codes), ptr(scale_e8m0))
    return codes, scale_e8m0


def mx_decode(codes, scale_e8m0, group_size, fmt, dtype):
    """the values of packed MX codes and E8M0 scale bytes in ONE launch -> y of `dtype`, [groups * group_size]"""
    dev = require_device(codes, scale_e8m0)
    groups = scale_e8m0.numel()
    n = groups * group_size
    for t, m in ((codes, n * MX_CODE_BITS[fmt] // 8), (scale_e8m0, groups)):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == m
    y = torch.empty(n, dtype=dtype, device=dev)
    _launch(dev, 'bvq_mx_decode', 'bvq_mx_decode', dtype_code(dtype), groups, int(group_size), int(fmt), ptr(codes),
            ptr(scale_e8m0), ptr(y))
    return y


def absmax_fakequant_cluster(desc, x, min_val, int_threshold, scale_dtype, running=None, momentum=0.0,
                             first_batch=False, flags=0, fallbacks=None, form=CLUSTER_AUTO, stamps=None):
    """abs-max statistic, scale, running statistic and quantize-dequantize in ONE launch for channels held by a cluster
    of workgroups (x read once) -> (stat, scale, y), the bits of absmax_scale + fakequant_fwd; or None when the shape is
    not covered or there is no arrival buffer (capturing, ONEPASS off): the caller takes the two-call route.
    fallbacks: optional int32 device counter of the workgroups that read their channel themselves.
    form (developers, tests): CLUSTER_AUTO, or the form of the kernel to run instead of the library's choice for the
    shape; stamps: int64 [channels * members * 6] for a library built with -DBVQ_CLUSTER_STAMPS."""
    dev = require_device(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    words = int(lib.bvq_absmax_fakequant_cluster_supported(ctypes.byref(desc), ptr(x), ptr(y)))
    if words <= 0:
        return None
    with _DeviceGuard(dev) as st:
        arrive = arrival_buffer(dev, st, words)
        if arrive is None:
            return None
        stat = torch.empty(desc.channels, dtype=x.dtype, device=dev)
        scale = torch.empty(desc.channels, dtype=scale_dtype, device=dev)
        args = (ctypes.byref(desc), ptr(x), *_scale_args(min_val, int_threshold), ptr(stat), ptr(scale),
                *_running_args(running, momentum, first_batch), ptr(y), ptr(arrive), arrive.numel(), int(flags),
                ptr(fallbacks))
        if form == CLUSTER_AUTO and stamps is None:
            _call('bvq_absmax_fakequant_cluster', 'bvq_stats_fakequant_fwd', *args, st)
        else:
            _call('bvq_absmax_fakequant_cluster_form', 'bvq_stats_fakequant_fwd', *args, int(form), ptr(stamps), st)
    return stat, scale, y


def _absmax_list_args(xs, outers, channels, inners):
    """the leading arguments bvq_absmax_list_supported and bvq_absmax_scale_list share"""
    n = len(xs)
    return (dtype_code(xs[0].dtype), n, (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs]),
            (ctypes.c_int64 * n)(*outers), channels, (ctypes.c_int64 * n)(*inners))


def absmax_list_supported(xs, outers, channels, inners) -> bool:
    """the list kernel covers these tensors (absmax_scale_list returns None only for want of an arrival buffer)"""
    return bool(lib.bvq_absmax_list_supported(*_absmax_list_args(xs, outers, channels, inners)))


def absmax_scale_list(xs, outers, channels, inners, min_val, int_threshold, scale_dtype):
    """abs-max statistic of a LIST of contiguous tensors [outers[i], channels, inners[i]] (the concatenation the
    reference builds is never materialised) and the scale derived from it, ONE launch:
    -> (stat [channels], scale [channels]), or None when the list is not covered / no arrival buffer"""
    dev = require_device(*xs)
    for x, o, i in zip(xs, outers, inners):
        assert x.is_contiguous() and x.dtype == xs[0].dtype and x.numel() == o * channels * i
    args = _absmax_list_args(xs, outers, channels, inners)
    if not lib.bvq_absmax_list_supported(*args):
        return None
    with _DeviceGuard(dev) as st:
        arrive = ws = None
        if channels > 1:
            arrive = arrival_buffer(dev, st, max(2 * channels, 18))
            if arrive is None:
                return None
        else:  # a whole-tensor statistic: one partial per unit (<= 4096) and a finishing launch
            ws = torch.empty(1 << 14, dtype=torch.uint8, device=dev)
        stat = torch.empty(channels, dtype=xs[0].dtype, device=dev)
        scale = torch.empty(channels, dtype=scale_dtype, device=dev)
        _call('bvq_absmax_scale_list', None, *args, ptr(stat),
              *_scale_args(min_val, int_threshold), dtype_code(scale_dtype), ptr(scale), ptr(arrive),
              arrive.numel() if arrive is not None else 0, ptr(ws), ws.numel() if ws is not None else 0, st)
    return stat, scale


def absmax_scale(x, outer, channels, inner, min_val, int_threshold, scale_dtype, pre_op=PRE_NONE, running=None,
                 momentum=0.0, first_batch=False):
    """abs-max statistic and the scale derived from it, one call: -> (stat [channels], scale [channels]);
    running (contiguous [channels] buffer): also folded with the statistic in the same finishing launch"""
    dev = require_device(x)
    assert x.is_contiguous() and x.numel() == outer * channels * inner
    dt = dtype_code(x.dtype)
    stat = torch.empty(channels, dtype=x.dtype, device=dev)
    scale = torch.empty(channels, dtype=scale_dtype, device=dev)
    if _absmax_onepass(dev, pre_op, x, outer, channels, inner, stat, min_val, int_threshold, scale, running, momentum,
                       first_batch):
        return stat, scale
    scale_args = (*_scale_args(min_val, int_threshold), dtype_code(scale_dtype), ptr(scale))
    ws, _ = _workspace(dev, 'bvq_stats_workspace_bytes', STAT_ABSMAX, dt, outer, channels, inner, floor=8)
    if running is not None:
        _launch(dev, 'bvq_absmax_scale_running', 'bvq_stats', pre_op, dt, ptr(x), outer, channels, inner, ptr(stat),
                *scale_args, *_running_args(running, momentum, first_batch), ptr(ws), ws.numel())
    else:
        _launch(dev, 'bvq_absmax_scale', 'bvq_stats', pre_op, dt, ptr(x), outer, channels, inner, ptr(stat),
                *scale_args, ptr(ws), ws.numel())
    return stat, scale


def _kth(entry, bracket, x, ks, outer, channels, inner, abs_key):
    """ranks ks of |x| or x per channel of x[outer, channels, inner] -> [len(ks), channels]"""
    dev = require_device(x)
    assert x.is_contiguous() and x.numel() == outer * channels * inner
    dt = dtype_code(x.dtype)
    out = torch.empty(len(ks), channels, dtype=x.dtype, device=dev)
    ws, wsb = _workspace(dev, 'bvq_kth_workspace_bytes', dt, outer, channels, inner)
    _launch(dev, entry, bracket, int(abs_key), dt, ptr(x), outer, channels, inner, *map(int, ks), ptr(out), ptr(ws),
            wsb)
    return out


def kth_value(x, k, outer, channels, inner, abs_key):
    """exact k-th smallest (1-indexed) of |x| or x per channel of x[outer, channels, inner] -> [channels]"""
    return _kth('bvq_kth_value', 'bvq_kth_value', x, (k,), outer, channels, inner, abs_key)[0]


def kth_pair(x, k_first, k_second, outer, channels, inner, abs_key):
    """two ranks of the same tensor, one histogram read where the per-tensor route applies -> [2, channels]"""
    return _kth('bvq_kth_pair', None, x, (k_first, k_second), outer, channels, inner, abs_key)


KTH_EXPLICIT, KTH_HIGH, KTH_LOW = 0, 1, 2


def scale_from_stat(stat32, stat_dtype, min_val, int_threshold, scale_dtype, running=None, momentum=0.0,
                    first_batch=False):
    """all-reduced float32 statistic [channels] -> (stat in stat_dtype, scale in scale_dtype), one launch; running
    (contiguous [channels] buffer): _RuntimeStats' running average updated in the same launch"""
    dev = require_device(stat32, running)
    assert stat32.dtype == torch.float32 and stat32.is_contiguous()
    n = stat32.numel()
    stat = torch.empty(n, dtype=stat_dtype, device=dev)
    scale = torch.empty(n, dtype=scale_dtype, device=dev)
    _launch(dev, 'bvq_scale_from_stat_running', None, ptr(stat32), n, dtype_code(stat_dtype), ptr(stat),
            *_scale_args(min_val, int_threshold), dtype_code(scale_dtype), ptr(scale),
            *_running_args(running, momentum, first_batch))
    return stat, scale


def fakequant_bwd_shard(desc, g, x, scale, zp, stat, rank):
    """backward of the stats-scaled per-channel graph on ONE BATCH SHARD: -> (dx without the deposit, this shard's
    float64 [2 * channels] all-gather message, first arg-max position per channel), or None if the layout is not
    covered (include/bvq.h, bvq_fakequant_bwd_shard)"""
    dev = require_device(g, x, scale, zp, stat)
    wsb = int(lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(desc)))
    if wsb <= 0 or (x.data_ptr() | g.data_ptr()) & 15:
        return None
    ch = int(desc.channels)
    dx = torch.empty_like(x)
    msg = torch.empty(2 * ch, dtype=torch.float64, device=dev)
    pos = torch.empty(ch, dtype=torch.int64, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stat = stat.to(x.dtype).contiguous()
    with _DeviceGuard(dev) as st:
        arrive = arrival_buffer(dev, st, ch) if ONEPASS_BWD else None
        _call('bvq_fakequant_bwd_shard', 'bvq_fakequant_bwd', ctypes.byref(desc), ptr(g), ptr(x), ptr(scale),
              ptr(zp), ptr(stat), ptr(dx), ptr(msg), ptr(pos), int(rank), ptr(ws), wsb, ptr(arrive),
              arrive.numel() if arrive is not None else 0, st)
    return dx, msg, pos


def shard_unpack_deposit(x, dx, gathered, world, channels, rank, first_pos, inner, scale_dtype, int_threshold,
                         quot_dtype, pre_op=PRE_NONE, want_dscale=False):
    """after the all-gather: the shards' dscale sums added in double, the owner's deposit on dx in place (include/bvq.h);
    -> float32 dscale_total [channels] if asked"""
    dev = require_device(x, dx, gathered, first_pos)
    assert gathered.dtype == torch.float64 and gathered.is_contiguous() and gathered.numel() == world * 2 * channels
    ds = torch.empty(channels, dtype=torch.float32, device=dev) if want_dscale else None
    _launch(dev, 'bvq_shard_unpack_deposit', None, dtype_code(x.dtype), ptr(x), ptr(dx), ptr(gathered), int(world),
            channels, int(rank), ptr(first_pos), inner, dtype_code(scale_dtype), float(int_threshold),
            dtype_code(quot_dtype), pre_op, ptr(ds))
    return ds


def shard_pack(ds, tie_info, channels, rank, per_channel):
    """this shard's float64 [2 * channels] message for the backward all-gather (include/bvq.h)"""
    dev = require_device(ds, tie_info)
    assert ds.dtype == torch.float32 and ds.is_contiguous() and tie_info.dtype == torch.int64
    msg = torch.empty(2 * channels, dtype=torch.float64, device=dev)
    _launch(dev, 'bvq_shard_pack', None, ptr(ds), ptr(tie_info), channels, int(rank), int(per_channel), ptr(msg))
    return msg


def shard_unpack(gathered, world, channels, rank, per_channel, tie_info):
    """-> (dscale_total float32 [channels], total_ties int64 [1] or None); tie_info is updated in place"""
    dev = require_device(gathered, tie_info)
    assert gathered.dtype == torch.float64 and gathered.is_contiguous() and gathered.numel() == world * 2 * channels
    ds_total = torch.empty(channels, dtype=torch.float32, device=dev)
    total = None if per_channel else torch.empty(1, dtype=torch.int64, device=dev)
    _launch(dev, 'bvq_shard_unpack', None, ptr(gathered), int(world), channels, int(rank), int(per_channel),
            ptr(ds_total), ptr(tie_info), ptr(total))
    return ds_total, total


def abs_moments(x, outer, channels, inner):
    """-> float32 [3 * channels] of x[outer, channels, inner]: per channel sum d, sum d^2 with d = |x| - p, and the
    pivot p (include/bvq.h): mean |x| = p + sum d / n, var |x| = (sum d^2 - (sum d)^2 / n) / (n - 1)"""
    dev = require_device(x)
    assert x.is_contiguous() and x.numel() == outer * channels * inner
    dt = dtype_code(x.dtype)
    sums = torch.empty(3 * channels, dtype=torch.float32, device=dev)
    ws, wsb = _workspace(dev, 'bvq_abs_moments_workspace_bytes', dt, outer, channels, inner, floor=8)
    _launch(dev, 'bvq_abs_moments', None, dt, ptr(x), outer, channels, inner, ptr(sums), ptr(ws), wsb)
    return sums


def abs_affine_bwd(x, a, b, outer, channels, inner):
    """dx = sgn(x) * (a[c] + b[c] * |x|); a, b float32 [channels]"""
    dev = require_device(x, a, b)
    assert x.is_contiguous() and a.dtype == torch.float32 and b.dtype == torch.float32
    assert a.numel() == channels and b.numel() == channels
    dx = torch.empty_like(x)
    _launch(dev, 'bvq_abs_affine_bwd', None, dtype_code(x.dtype), ptr(x), ptr(a.contiguous()), ptr(b.contiguous()),
            ptr(dx), outer, channels, inner)
    return dx


class _KthSteps:
    """A select in steps on one shard: begin / hist(p) / pick(p) / finish over the entries `prefix`_begin .. _finish of
    include/bvq.h.  A route gives the prefix, the leading arguments of its entries and where the counters of a pass
    lie; `passes`, `per_channel` (elements per channel on THIS shard) and the workspace come from its constructor."""

    def __init__(self, x, abs_key, rule, q, k, channels):
        self.dev = require_device(x)
        assert x.is_contiguous()
        self.x, self.abs_key, self.channels = x, int(abs_key), channels
        self.rule, self.q, self.k = int(rule), float(q), int(k)
        self.dt = dtype_code(x.dtype)

    def _step(self, step, *args):
        _launch(self.dev, '%s_%s' % (self.prefix, step), None, *args, ptr(self.ws), self.wsb)

    def begin(self):
        self._step('begin', *self._begin_args())

    def hist(self, p):
        """histogram this shard's elements for pass p -> the counters to be summed over the shards (int32 view of the
        unsigned counters: a two's-complement sum over the shards is their unsigned sum)"""
        self._step('hist', self.abs_key, self.dt, ptr(self.x) if self.x.numel() else None, *self._shape, p)
        off, words = self._counters(p)
        return self.ws[off:off + 4 * words].view(torch.int32)

    def pick(self, p):
        self._step('pick', *self._pick_args(p))

    def finish(self):
        out = torch.empty(self.channels, dtype=self.x.dtype, device=self.dev)
        self._step('finish', *self._lead, ptr(out))
        return out


class KthSelectSteps(_KthSteps):
    """bvq_kth_value in steps (include/bvq.h) for a batch-sharded tensor: between hist(p) and pick(p)
    the caller sums the returned counters over the shards (brevitas_amd.distributed.sharded_kth_value).
    rule / q: the rank is derived on the device from the global element count (KTH_HIGH / KTH_LOW), or
    KTH_EXPLICIT with k."""
    prefix = 'bvq_kth'

    def __init__(self, x, outer, channels, inner, abs_key, rule, q, k=0):
        super().__init__(x, abs_key, rule, q, k, channels)
        assert x.numel() == outer * channels * inner
        self.layout = self._shape = (outer, channels, inner)
        self.per_channel = outer * inner if channels > 1 else x.numel()
        self.passes = int(lib.bvq_kth_passes(self.dt))
        self._lead = (self.abs_key, self.dt, channels)
        self.ws, self.wsb = _workspace(self.dev, 'bvq_kth_workspace_bytes', self.dt, outer, channels, inner)

    def _begin_args(self):
        return self.dt, self.channels, self.rule, self.k, self.q

    def _pick_args(self, p):
        return self.dt, self.channels, p, self.rule, self.q

    def _counters(self, p):
        # (the counters of a pass end where the next pass's begin; every dtype has at least two passes)
        at = [int(lib.bvq_kth_hist_offset(self.dt, self.channels, i)) for i in (0, 1, p)]
        return at[2], (at[1] - at[0]) // 4


class KthWideSteps(_KthSteps):
    """the sharded selection of a whole-tensor statistic with the 15-bit first digit (include/bvq.h, bvq_kthw_*):
    same interface as KthSelectSteps -- begin / hist(p) / pick(p) / finish, `passes`, `per_channel` -- for
    brevitas_amd.distributed.sharded_kth_value; one pass for |x| of a 16-bit type, two otherwise"""
    prefix = 'bvq_kthw'

    def __init__(self, x, abs_key, rule, q, k=0):
        super().__init__(x.reshape(-1), abs_key, rule, q, k, 1)
        self._shape = (x.numel(),)
        self.per_channel = x.numel()
        self.passes = int(lib.bvq_kthw_plan(self.abs_key, self.dt, -1, None, None))
        if self.passes < 1:
            raise BvqError('bvq_kthw_plan: bad arguments')
        self._lead = (self.abs_key, self.dt)
        self.ws, self.wsb = _workspace(self.dev, 'bvq_kth_workspace_bytes', self.dt, 1, 1, max(x.numel(), 1))

    def _begin_args(self):
        return self._lead

    def _pick_args(self, p):
        return self.abs_key, self.dt, p, self.rule, self.k, self.q

    def _counters(self, p):
        off, words = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.bvq_kthw_plan(self.abs_key, self.dt, p, ctypes.byref(off), ctypes.byref(words))
        return off.value, words.value


def running_stats_update(running, stat, momentum, first_batch):
    """in-place batch-norm style update of a running statistic (one launch)"""
    dev = require_device(running, stat)
    assert running.is_contiguous() and running.numel() == stat.numel()
    stat = stat.contiguous()
    _launch(dev, 'bvq_running_stats_update', None, dtype_code(running.dtype), ptr(running), dtype_code(stat.dtype),
            ptr(stat), running.numel(), float(momentum), int(first_batch))
    return running


def tie_info_buffer(channels, device):
    nbytes = int(lib.bvq_tie_info_bytes(int(channels)))
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def stat_tie_scan(match, x, stat, outer, channels, inner, dx_zero_fill=None):
    """record which elements of x attain `stat`; returns the tie_info buffer (int64, device)"""
    dev = require_device(x, stat, dx_zero_fill)
    assert x.is_contiguous()
    stat = stat.to(x.dtype).contiguous()
    info = tie_info_buffer(channels, dev)
    _launch(dev, 'bvq_stat_tie_scan', None, match, dtype_code(x.dtype), ptr(x), ptr(stat), outer, channels, inner,
            ptr(dx_zero_fill), ptr(info))
    return info


def stat_tie_apply(match, x, stat, gstat, info, dx, outer, channels, inner, mode_add, total_ties=None,
                   pre_op=PRE_NONE):
    dev = require_device(x, stat, gstat, info, dx, total_ties)
    assert x.is_contiguous() and dx.is_contiguous() and dx.dtype == x.dtype
    stat = stat.to(x.dtype).contiguous()
    gstat = gstat.to(x.dtype).contiguous()
    _launch(dev, 'bvq_stat_tie_apply', None, match, pre_op, dtype_code(x.dtype), ptr(x), ptr(stat), ptr(gstat),
            ptr(info), ptr(total_ties), ptr(dx), outer, channels, inner, int(mode_add))
    return dx


def stat_tie_apply_dscale(x, stat, dscale, scale_dtype, int_threshold, quot_dtype, info, dx, outer, channels,
                          inner, total_ties=None, pre_op=PRE_NONE):
    """deposit the statistic's gradient derived from float32 dscale sums (fused quantizer backward)"""
    dev = require_device(x, stat, dscale, info, dx, total_ties)
    assert x.is_contiguous() and dx.is_contiguous() and dx.dtype == x.dtype and dscale.dtype == torch.float32
    stat = stat.to(x.dtype).contiguous()
    _launch(dev, 'bvq_stat_tie_apply_dscale', None, pre_op, dtype_code(x.dtype), ptr(x), ptr(stat), ptr(dscale),
            dtype_code(scale_dtype), float(int_threshold), dtype_code(quot_dtype), ptr(info), ptr(total_ties), ptr(dx),
            outer, channels, inner)
    return dx


def fakequant_bwd_stats(desc, g, x, scale, zp, stat, scale_dtype, int_threshold, quot_dtype, want_dscale=False):
    """backward of the stats-scaled per-channel graph in two launches: dx with the statistic's gradient already
    deposited on the arg-max elements (and the float32 dscale sums if asked); None if the layout is not covered"""
    dev = require_device(g, x, scale, zp, stat)
    wsb = int(lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(desc)))
    if wsb <= 0 or (x.data_ptr() | g.data_ptr()) & 15:  # (views into the middle of a buffer: the general route)
        return None
    dx = torch.empty_like(x)
    ds = torch.empty(int(desc.channels), dtype=torch.float32, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stat = stat.to(x.dtype).contiguous()
    with _DeviceGuard(dev) as st:
        arrive = None
        if ONEPASS_BWD and lib.bvq_fakequant_bwd_stats_onepass_supported(ctypes.byref(desc)):
            arrive = arrival_buffer(dev, st, int(desc.channels))
        if arrive is not None:  # one launch: the wave that completes a channel finishes it
            _call('bvq_fakequant_bwd_stats_onepass', 'bvq_fakequant_bwd', ctypes.byref(desc), ptr(g), ptr(x),
                  ptr(scale), ptr(zp), ptr(stat), ptr(dx), ptr(ds), dtype_code(scale_dtype), float(int_threshold),
                  dtype_code(quot_dtype), ptr(ws), wsb, ptr(arrive), arrive.numel(), st)
        else:
            _call('bvq_fakequant_bwd_stats', 'bvq_fakequant_bwd', ctypes.byref(desc), ptr(g), ptr(x), ptr(scale),
                  ptr(zp), ptr(stat), ptr(dx), ptr(ds), dtype_code(scale_dtype), float(int_threshold),
                  dtype_code(quot_dtype), ptr(ws), wsb, st)
    return (dx, ds) if want_dscale else dx


def variant_fwd(desc, x, scale, pre_scale=None, zp=None, pre_zp=None):
    """forward of the sign / decoupled / truncating quantizers (include/bvq.h, bvq_variant_fwd) -> y in desc.ct_dtype"""
    dev = require_device(x, scale, pre_scale, zp, pre_zp)
    y = torch.empty(x.shape, dtype=TORCH_DTYPES[desc.ct_dtype], device=dev)
    _launch(dev, 'bvq_variant_fwd', None, ctypes.byref(desc), ptr(x), ptr(scale), ptr(pre_scale), ptr(zp), ptr(pre_zp),
            ptr(y))
    return y


def variant_bwd(desc, g, x, scale, pre_scale=None, zp=None, pre_zp=None, need_dscale=False, need_dpre=False):
    """-> (dx, dscale float32 or None, dpre_scale float32 or None)"""
    dev = require_device(g, x, scale, pre_scale, zp, pre_zp)
    dx = torch.empty_like(x)
    nsum = int(desc.channels) if (desc.scale_per_channel and desc.channels > 1) else 1
    ds = torch.empty(nsum, dtype=torch.float32, device=dev) if need_dscale else None
    dp = torch.empty(nsum, dtype=torch.float32, device=dev) if need_dpre else None
    ws, wsb = None, 0
    if need_dscale or need_dpre:
        ws, wsb = _workspace(dev, 'bvq_variant_bwd_workspace_bytes', ctypes.byref(desc), floor=8)
    _launch(dev, 'bvq_variant_bwd', None, ctypes.byref(desc), ptr(g), ptr(x), ptr(scale), ptr(pre_scale), ptr(zp),
            ptr(pre_zp), ptr(dx), ptr(ds), ptr(dp), ptr(ws), wsb)
    return dx, ds, dp


def fakequant_fwd_bounds(desc, x, scale, zp, bounds):
    """bvq_fakequant_fwd with the integer range [qmin, qmax] read from the device (float32 [2]) -> y"""
    dev = require_device(x, scale, zp, bounds)
    assert bounds.dtype == torch.float32 and bounds.numel() == 2 and bounds.is_contiguous()
    y = torch.empty(x.shape, dtype=TORCH_DTYPES[desc.ct_dtype], device=dev)
    _launch(dev, 'bvq_fakequant_fwd_bounds', None, ctypes.byref(desc), ptr(x), ptr(scale), ptr(zp), ptr(bounds), ptr(y))
    return y


def fakequant_bwd_bounds(desc, g, x, scale, zp, bounds, need_dbounds):
    """-> (dx, dscale float32 [n], dbounds float32 [2, n] or None): n = channels when the scale OR the zero-point is
    per-channel, else 1 -- the kernel sums per channel in either case (like bvq_fakequant_bwd)"""
    dev = require_device(g, x, scale, zp, bounds)
    dx = torch.empty_like(x)
    nsum = int(desc.channels) if ((desc.scale_per_channel or desc.zp_per_channel) and desc.channels > 1) else 1
    ds = torch.empty(nsum, dtype=torch.float32, device=dev)
    db = torch.empty(2, nsum, dtype=torch.float32, device=dev) if need_dbounds else None
    ws, wsb = _workspace(dev, 'bvq_fakequant_bwd_workspace_bytes', ctypes.byref(desc), floor=8)
    _launch(dev, 'bvq_fakequant_bwd_bounds', None, ctypes.byref(desc), ptr(g), ptr(x), ptr(scale), ptr(zp), ptr(bounds),
            ptr(dx), ptr(ds), ptr(db), ptr(ws), wsb)
    return dx, ds, db


def histc(x, absmax, bins):
    """torch.histc(x, bins, min=-absmax, max=absmax) with the bounds read from the device -> int32 [bins]"""
    dev = require_device(x, absmax)
    x = x.contiguous()
    counts = torch.empty(bins, dtype=torch.int32, device=dev)
    _launch(dev, 'bvq_histc', None, dtype_code(x.dtype), ptr(x), x.numel(), ptr(absmax.to(x.dtype).reshape(1)),
            int(bins), ptr(counts))
    return counts


def selftest_div_f16r(a, scales):
    """diagnostic: the quotient the float16 kernels compute for every (scale, numerator) pair -> float32 [n_s, n_a]"""
    dev = require_device(a, scales)
    assert a.dtype == torch.float32 and scales.dtype == torch.float32 and a.is_contiguous() and scales.is_contiguous()
    out = torch.empty(scales.numel(), a.numel(), dtype=torch.float32, device=dev)
    _launch(dev, 'bvq_selftest_div_f16r', None, ptr(a), a.numel(), ptr(scales), scales.numel(), ptr(out))
    return out


def selftest_pre_op(pre_op, x, g):
    """diagnostic: (act(x), act_backward(g, act(x))) as the quantizer kernels compute the fused activation pre_op
    (PRE_SIGMOID / PRE_TANH), element by element, in x's dtype"""
    dev = require_device(x, g)
    assert x.dtype == g.dtype and x.shape == g.shape and x.is_contiguous() and g.is_contiguous()
    a = torch.empty_like(x)
    da = torch.empty_like(x)
    _launch(dev, 'bvq_selftest_pre_op', None, pre_op, dtype_code(x.dtype), ptr(x), ptr(g), ptr(a), ptr(da), x.numel())
    return a, da


def learned_scale(value, min_val, int_threshold, scale_dtype):
    """scale = |clamp_min(value, min_val)| / int_threshold, one launch -> [value.numel()] in scale_dtype"""
    dev = require_device(value)
    v = value.detach().reshape(-1).contiguous()
    scale = torch.empty(v.numel(), dtype=scale_dtype, device=dev)
    _launch(dev, 'bvq_learned_scale', None, dtype_code(v.dtype), ptr(v), v.numel(),
            *_scale_args(min_val, int_threshold), dtype_code(scale_dtype), ptr(scale))
    return scale


def fakequant_bwd_learned(desc, g, x, scale, zp, value, min_val, int_threshold, gscale=None):
    """quantizer backward + the learned scale's backward in its last launch -> (dx, dscale float32, dvalue flat)"""
    dev = require_device(g, x, scale, zp, value, gscale)
    dx = torch.empty_like(x)
    pc = desc.scale_per_channel and desc.channels > 1
    nsum = int(desc.channels) if pc else 1
    v = value.detach().reshape(-1).contiguous()
    assert v.numel() == nsum and (gscale is None or (gscale.numel() == nsum and gscale.is_contiguous()))
    ds = torch.empty(nsum, dtype=torch.float32, device=dev)
    dv = torch.empty(nsum, dtype=v.dtype, device=dev)
    ws, wsb = _workspace(dev, 'bvq_fakequant_bwd_workspace_bytes', ctypes.byref(desc), floor=8)
    _launch(dev, 'bvq_fakequant_bwd_learned', 'bvq_fakequant_bwd', ctypes.byref(desc), ptr(g), ptr(x), ptr(scale),
            ptr(zp), ptr(dx), ptr(ds), ptr(v), dtype_code(v.dtype), *_scale_args(min_val, int_threshold), ptr(gscale),
            ptr(dv), ptr(ws), wsb)
    return dx, ds, dv


def fakequant_bwd(desc, g, x, scale, zp, need_dscale, need_dzp, tie_stat=None):
    """-> (dx, dscale, dzp[, tie_info]); tie_stat: abs-max statistic whose ties are recorded on the fly"""
    dev = require_device(g, x, scale, zp, tie_stat)
    dx = torch.empty_like(x)
    pc = (desc.scale_per_channel or desc.zp_per_channel) and desc.channels > 1
    nsum = int(desc.channels) if pc else 1
    ds = torch.empty(nsum, dtype=torch.float32, device=dev) if need_dscale else None
    dz = torch.empty(nsum, dtype=torch.float32, device=dev) if need_dzp else None
    info = None
    if tie_stat is not None:
        tie_stat = tie_stat.to(x.dtype).contiguous()
        info = tie_info_buffer(desc.channels, dev)
    ws, wsb = None, 0
    if need_dscale or need_dzp:
        ws, wsb = _workspace(dev, 'bvq_fakequant_bwd_workspace_bytes', ctypes.byref(desc), floor=8)
    _launch(dev, 'bvq_fakequant_bwd', 'bvq_fakequant_bwd', ctypes.byref(desc), ptr(g), ptr(x), ptr(scale), ptr(zp),
            ptr(dx), ptr(ds), ptr(dz), ptr(tie_stat), ptr(info), ptr(ws), wsb)
    if tie_stat is not None:
        return dx, ds, dz, info
    return dx, ds, dz


# ---- many weights in one launch each way (include/bvq.h, bvq_weight_quant_list_*) -------------------------------------
# The caller keeps a WeightItem array with the static fields filled (x, channels, inner, min_val, int_threshold, qmin,
# qmax, use_min, clamp_ste); a call takes the len(xs) items from index `first` on, sets their per-call pointers and
# launches.

_ITEM = ctypes.sizeof(WeightItem)


def weight_list_supported(items, first, n, dtype, round_mode):
    """the n items from `first` on (static fields and x) are covered by both one-launch forms"""
    return bool(lib.bvq_weight_list_supported(dtype_code(dtype), round_mode, n,
                                              ctypes.addressof(items) + first * _ITEM, ARRIVE_WORDS))


def weight_quant_list_fwd(items, first, xs, scale_dtype, round_mode):
    """statistic, scale and quantize-dequantize of every weight of `xs` (items[first + i] describes xs[i]), ONE launch
    -> (ys, stat, scale): ys fresh tensors like xs, stat [sum of channels] in xs' dtype, scale [sum of channels] in
    scale_dtype, tensor i's channels after tensor i - 1's"""
    n = len(xs)
    dev = xs[0].device
    dtype = xs[0].dtype
    channels = 0
    for i in range(first, first + n):
        channels += items[i].channels
    if scale_dtype == dtype:  # one buffer for both per-channel vectors
        both = torch.empty(2 * channels, dtype=dtype, device=dev)
        stat, scale = both[:channels], both[channels:]
    else:
        stat = torch.empty(channels, dtype=dtype, device=dev)
        scale = torch.empty(channels, dtype=scale_dtype, device=dev)
    ys = [torch.empty_like(x) for x in xs]
    ps, ss = stat.data_ptr(), scale.data_ptr()
    es, esc = stat.element_size(), scale.element_size()
    for i in range(n):
        it = items[first + i]
        it.y = ys[i].data_ptr()
        it.stat = ps
        it.scale = ss
        ps += it.channels * es
        ss += it.channels * esc
    _launch(dev, 'bvq_weight_quant_list_fwd', 'bvq_weight_quant_list_fwd', dtype_code(dtype), dtype_code(scale_dtype),
            round_mode, n, ctypes.addressof(items) + first * _ITEM)
    return ys, stat, scale


def weight_quant_list_bwd(items, first, gs, xs, stat_ptrs, scale_ptrs, scale_dtype, quot_dtype, round_mode):
    """backward of weight_quant_list_fwd for the gradients `gs` (contiguous, 16-byte aligned, xs' dtype) with the
    forward's statistics and scales at stat_ptrs / scale_ptrs, ONE launch -> dxs (the statistics' gradients
    deposited), or None when no arrival buffer is available -- a stream capturing its first step (arrival buffers are
    allocated outside captures: capture on the stream the eager warm-up ran on), or the one-launch backward switched off
    (ONEPASS_BWD) -- and the caller takes the per-tensor route"""
    n = len(xs)
    dev = xs[0].device
    dtype = xs[0].dtype
    channels = 0
    for i in range(first, first + n):
        channels += items[i].channels
    with _DeviceGuard(dev) as st:
        arrive = arrival_buffer(dev, st, channels) if ONEPASS_BWD else None
        if arrive is None:
            return None
        dxs = [torch.empty_like(x) for x in xs]
        ds = torch.empty(channels, dtype=torch.float32, device=dev)
        pd = ds.data_ptr()
        for i in range(n):
            it = items[first + i]
            it.g = gs[i].data_ptr()
            it.dx = dxs[i].data_ptr()
            it.stat = stat_ptrs[i]
            it.scale = scale_ptrs[i]
            it.dscale = pd
            pd += it.channels * 4
        addr = ctypes.addressof(items) + first * _ITEM
        ws, wsb = _workspace(dev, 'bvq_weight_quant_list_bwd_workspace_bytes', dtype_code(dtype), n, addr)
        _call('bvq_weight_quant_list_bwd', 'bvq_weight_quant_list_bwd', dtype_code(dtype),
              dtype_code(scale_dtype), dtype_code(quot_dtype), round_mode, n, addr, ptr(ws), wsb, ptr(arrive),
              arrive.numel(), st)
    return dxs

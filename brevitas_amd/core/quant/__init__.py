from .binary import BinaryQuant, ClampedBinaryQuant
from .delay import DelayWrapper
from .dynamic import DynamicActIntQuant
from .int import (DecoupledRescalingIntQuant, GroupwiseHQOIntQuant, GroupwiseMSEIntQuant, GroupwiseRescalingIntQuant,
                  PrescaledRestrictIntQuant, PrescaledRestrictIntQuantWithInputBitWidth, RescalingIntQuant,
                  TruncIntQuant, WeightNormIntQuant)
from .int_base import DecoupledIntQuant, IntQuant
from .mx import MXPacked, MXQuant, mx_dequantize
from .ternary import TernaryQuant

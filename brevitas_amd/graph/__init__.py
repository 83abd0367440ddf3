from .awq import (AWQResult, awq_candidates, awq_losses, awq_mode, awq_scale_weight, awq_table, freeze_awq_weight)
from .calibrate import DisableEnableQuantization, calibration_mode, finalize_collect_stats
from .gpfq import GPFQResult, gpfq_mode, gpfq_quantize_weight
from .gptq import GPTQResult, freeze_weight_quant, gptq_mode, gptq_quantize_weight, unfreeze_weight_quant
from .learned_round import insert_learned_round, learned_round_mode, remove_learned_round
from .rotate import insert_online_rotation, merge_input_rotation, merge_output_rotation, rotate_pair

__all__ = ['calibration_mode', 'finalize_collect_stats', 'DisableEnableQuantization', 'gptq_mode',
           'gptq_quantize_weight', 'GPTQResult', 'freeze_weight_quant', 'unfreeze_weight_quant',
           'learned_round_mode', 'insert_learned_round', 'remove_learned_round', 'awq_mode', 'awq_scale_weight',
           'awq_candidates', 'awq_losses', 'awq_table', 'AWQResult', 'freeze_awq_weight', 'gpfq_mode',
           'gpfq_quantize_weight', 'GPFQResult', 'merge_input_rotation', 'merge_output_rotation', 'rotate_pair',
           'insert_online_rotation']

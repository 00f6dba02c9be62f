"""Inputs of the TeaCache fixture tests/golden/g19_teacache.npz, shared by its generator (tests/golden/make_teacache_golden.py) and
the tests: the g13 call (gen_inputs.PIPELINE_CALL_KWARGS, same models / image / control video / prompts) with 20 steps and TeaCache on."""
import torch

import gen_inputs as gi

CALL_KWARGS = dict(gi.PIPELINE_CALL_KWARGS, num_inference_steps=20, tea_cache_l1_thresh=0.26,
                   tea_cache_model_id="Wan2.1-I2V-14B-480P")
EXPERT_SEEDS = (41, 43)        # dit, dit2 of g13
OFFSET_SCALE = 8.0
BIAS = "time_projection.1.bias"


def smooth_time_projection(sd, expert):
    """Adds OFFSET_SCALE * randn(seed 700 + expert) to `time_projection.1.bias` of an fp32 state dict, in place, BEFORE the dtype
    cast.  A random-init time embedding is chaotic from step to step (relative L1 distance of consecutive t_mod around 0.9) and
    nothing is ever skipped; a large constant part, as a trained projection has, makes consecutive steps close."""
    assert sd[BIAS].dtype == torch.float32
    g = torch.Generator().manual_seed(700 + expert)
    sd[BIAS] += OFFSET_SCALE * torch.randn(sd[BIAS].shape, generator=g)
    return sd


def expert_sd(expert):
    """The fp32 state dict of expert 0 / 1 (gen_inputs.dit_sd, seeds of g13) with the smoothed time projection."""
    return smooth_time_projection(gi.dit_sd(gi.TINY, seed=EXPERT_SEEDS[expert], dtype=torch.float32), expert)

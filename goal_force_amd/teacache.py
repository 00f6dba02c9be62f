"""TeaCache — skip the whole block stack of a denoising step whose timestep modulation has moved little since the last computed
one, and add that step's cached residual `x_after_blocks - x_patchified` instead (the reference's `TeaCache`, GF:1243-1292, behind
`pipe(..., tea_cache_l1_thresh=, tea_cache_model_id=)` and `model_fn_wan_video(tea_cache=)`).

Same constructor, attribute names and three methods as the reference's class; model_fn_wan_video talks to the object through
`check` / `store` / `update` only, so any object with those three works in its place.

The state machine is host arithmetic and has no GPU in it:
  * `ratio_from_sums` — mean|t_mod - prev| / mean|prev| with the three bf16 roundings torch makes on bf16 tensors,
  * `decide`          — step counter, accumulator, polynomial, threshold, forced first / last step, wrap.
The device side is two kernels (`ops.rel_l1`, `ops.sub`; the update is `ops.add`) and one 8-byte read-back per checked step.
"""
from __future__ import annotations

import struct

import numpy as np

from . import ops
from ._lib import GoalForceError

# Rescaling polynomials of the relative L1 distance, highest power first (what numpy.poly1d takes), per model id.  They were fitted
# by the TeaCache authors on the Wan2.1 checkpoints named; none is fitted for Wan2.2-A14B.
COEFFICIENTS = {
    "Wan2.1-T2V-1.3B":     (-52186.2437, 9230.41404, -528.275948, 13.6987616, -0.0499875664),
    "Wan2.1-T2V-14B":      (-303318.725, 49053.7029, -2655.30556, 58.7365115, -0.315583525),
    "Wan2.1-I2V-14B-480P": (257151.496, -35422.9917, 1402.86849, -13.5890334, 0.132517977),
    "Wan2.1-I2V-14B-720P": (8107.0546, 2133.93892, -372.934672, 16.6203073, -0.0417769401),
}


def coefficients_for(model_id):
    """The polynomial of `model_id`; ValueError naming the supported ids otherwise (GF:1259-1261)."""
    if model_id not in COEFFICIENTS:
        raise ValueError(f"{model_id} is not a supported TeaCache model id. Please choose a valid model id in "
                         f"({', '.join(COEFFICIENTS)}).")
    return list(COEFFICIENTS[model_id])


def _bf16(v) -> np.float32:
    """An fp32 value rounded to the nearest bf16 (ties to even), as fp32; inf and NaN pass through."""
    v = np.float32(v)
    if not np.isfinite(v):
        return v
    bits = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return np.float32(struct.unpack("<f", struct.pack("<I", bits))[0])


def ratio_from_sums(s_diff, s_prev, n) -> float:
    """`((cur - prev).abs().mean() / prev.abs().mean()).item()` as torch evaluates it on bf16 tensors, from the two sums of
    ops.rel_l1 (whose terms |bf16(cur_i - prev_i)| already carry the per-element rounding): each mean is the fp32 sum / n rounded
    to bf16, the quotient of the two bf16 means is an fp32 division rounded to bf16."""
    with np.errstate(divide="ignore", invalid="ignore"):       # an all-zero prev gives inf / nan like torch, never an exception
        m_diff = _bf16(np.float32(s_diff) / np.float32(n))
        m_prev = _bf16(np.float32(s_prev) / np.float32(n))
        return float(_bf16(m_diff / m_prev))


class TeaCache:
    """One per CFG branch and `pipe(...)` call; both experts share it across the `switch_DiT_boundary` switch (GF:1114-1125)."""

    def __init__(self, num_inference_steps, rel_l1_thresh, model_id):
        self.num_inference_steps = num_inference_steps
        self.step = 0
        self.accumulated_rel_l1_distance = 0
        self.previous_modulated_input = None
        self.rel_l1_thresh = rel_l1_thresh
        self.previous_residual = None
        self.previous_hidden_states = None
        self.coefficients_dict = {k: list(v) for k, v in COEFFICIENTS.items()}
        self.coefficients = coefficients_for(model_id)

    # ---- host only
    def decide(self, ratio) -> bool:
        """Skip this step?  `ratio` is the relative L1 distance of this step's t_mod to the previous step's; it is not looked
        at on the first and the last step of a pass, which always compute (GF:1266-1281)."""
        if self.step == 0 or self.step == self.num_inference_steps - 1:
            skip = False
            self.accumulated_rel_l1_distance = 0
        else:
            self.accumulated_rel_l1_distance += np.poly1d(self.coefficients)(ratio)
            skip = bool(self.accumulated_rel_l1_distance < self.rel_l1_thresh)
            if not skip:
                self.accumulated_rel_l1_distance = 0
        self.step += 1
        if self.step == self.num_inference_steps:
            self.step = 0
        return skip

    # ---- the three calls of model_fn_wan_video
    def check(self, dit, x, t_mod) -> bool:
        """After patchify and RoPE: True = skip the blocks (then `update`), False = run them (then `store`)."""
        ratio = None
        if not (self.step == 0 or self.step == self.num_inference_steps - 1):
            prev = self.previous_modulated_input
            if prev is None:
                raise GoalForceError("TeaCache.check: no previous t_mod at step %d — one object per pass, from step 0" % self.step)
            ratio = ratio_from_sums(*ops.rel_l1(t_mod.contiguous(), prev), t_mod.numel())
        skip = self.decide(ratio)
        self.previous_modulated_input = t_mod.clone()
        if not skip:
            self.previous_hidden_states = x.clone()
        return skip

    def store(self, hidden_states):
        """After the last block and the ControlNet injection of a computed step: keep bf16(x - the copy `check` took)."""
        if self.previous_hidden_states is None:
            raise GoalForceError("TeaCache.store without a computing `check` before it")
        self.previous_residual = ops.sub(hidden_states.contiguous(), self.previous_hidden_states, out=self.previous_hidden_states)
        self.previous_hidden_states = None

    def update(self, hidden_states):
        """On a skipped step: bf16(x + residual), a new tensor."""
        if self.previous_residual is None:
            raise GoalForceError("TeaCache.update before any `store`")
        return ops.add(hidden_states.contiguous(), self.previous_residual)

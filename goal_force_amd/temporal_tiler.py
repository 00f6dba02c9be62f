"""TemporalTiler_BCTHW — sliding-window sampling (src/goal_force/wan_video_new.py:1296-1345): the model is evaluated on overlapping
windows of latent frames and the predictions are cross-faded.  The reference's name and `run(...)` signature (B3 drop-in).

The schedule, the mask and the three bf16 roundings are the reference's; the accumulation runs on the device
(ops.window_blend / ops.window_finalize, gf_window.hip) with the reference's bf16 accumulators — no tensor leaves HBM and no torch
arithmetic is on the path.  Windows are blended in ascending order on the current stream: bf16 accumulation depends on the order.

Refused by name (GoalForceError) where the reference crashes, divides by a zero weight or silently does something else:
a stride larger than the size, non-positive or non-integer values, only one of the two given, a merged-CFG batch."""
from __future__ import annotations

import torch

from . import ops
from ._lib import GoalForceError


def check_window(sliding_window_size, sliding_window_stride):
    """(size, stride) of a sliding-window request, or None when neither is given."""
    if sliding_window_size is None and sliding_window_stride is None:
        return None
    if sliding_window_size is None or sliding_window_stride is None:
        # the reference takes the windowed branch only when BOTH are set (GF:1381) and otherwise runs the dense pass without a word
        raise GoalForceError(f"sliding window: sliding_window_size={sliding_window_size!r} and sliding_window_stride="
                             f"{sliding_window_stride!r} must be given together")
    for name, v in (("sliding_window_size", sliding_window_size), ("sliding_window_stride", sliding_window_stride)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise GoalForceError(f"sliding window: {name} must be an integer number of latent frames, got {v!r}")
        if v <= 0:
            raise GoalForceError(f"sliding window: {name} must be positive, got {v}")
    if sliding_window_stride > sliding_window_size:
        # border = size - stride < 0: the reference fails in build_1d_mask or leaves frames with weight zero
        raise GoalForceError(f"sliding window: sliding_window_stride={sliding_window_stride} exceeds sliding_window_size="
                             f"{sliding_window_size}: frames between the windows would be covered by none")
    return sliding_window_size, sliding_window_stride


class TemporalTiler_BCTHW:
    def __init__(self):
        pass

    @staticmethod
    def windows(T, sliding_window_size, sliding_window_stride):
        """[(t, t_)]: the windows [t, t_) the reference's loop visits over T latent frames, in its order (GF:1327-1330).  A start
        whose predecessor already reached the end of the clip is skipped."""
        out = []
        for t in range(0, T, sliding_window_stride):
            if t - sliding_window_stride >= 0 and t - sliding_window_stride + sliding_window_size >= T:
                continue
            out.append((t, min(t + sliding_window_size, T)))
        return out

    def run(self, model_fn, sliding_window_size, sliding_window_stride, computation_device, computation_dtype, model_kwargs,
            tensor_names, batch_size=None, window_kwargs=None):
        """GF:1318-1345.  `tensor_names`: the entries of model_kwargs cut along T ([1, C, T, H, W] each; None entries are left
        alone); every window calls `model_fn(**model_kwargs)` with its slices.  Returns the blended prediction, the shape of the first
        named tensor; model_kwargs holds the whole tensors again afterwards.
        `window_kwargs` (optional, not in the reference): `window_kwargs(t, t_)` -> further keywords for the call of window [t, t_)."""
        size, stride = check_window(sliding_window_size, sliding_window_stride)
        if batch_size not in (None, 1):
            raise GoalForceError(f"TemporalTiler_BCTHW.run: batch_size={batch_size!r} (a merged CFG batch) is not built: run the cond "
                                 "and the uncond forward separately")
        tensor_names = [n for n in tensor_names if model_kwargs.get(n) is not None]
        if not tensor_names:
            raise GoalForceError("TemporalTiler_BCTHW.run: none of tensor_names is set in model_kwargs")
        tensor_dict = {n: model_kwargs[n] for n in tensor_names}
        first = tensor_dict[tensor_names[0]]
        for n, x in tensor_dict.items():
            if not x.is_cuda or x.dtype != torch.bfloat16:
                raise GoalForceError(f"TemporalTiler_BCTHW.run: {n} must be a bf16 tensor on the GPU (no CPU fallback exists)")
            if x.dim() != 5 or x.shape[0] != 1 or x.shape[2:] != first.shape[2:]:
                raise GoalForceError(f"TemporalTiler_BCTHW.run: {n} must be [1, C, T, H, W] with the T, H, W of {tensor_names[0]} "
                                     f"{tuple(first.shape)}, got {tuple(x.shape)}")
        dev = torch.device(computation_device)
        if dev.type != first.device.type or dev.index not in (None, first.device.index) or computation_dtype != first.dtype:
            raise GoalForceError(f"TemporalTiler_BCTHW.run: computation on {computation_device} / {computation_dtype} with data on "
                                 f"{first.device} / {first.dtype}: the windows are computed where the data lives")
        _, C, T, H, W = first.shape
        value = torch.zeros((1, C, T, H, W), device=first.device, dtype=first.dtype)
        weight = torch.zeros((T,), device=first.device, dtype=first.dtype)
        try:
            for t, t_ in self.windows(T, size, stride):
                model_kwargs.update({n: x[:, :, t:t_].contiguous() for n, x in tensor_dict.items()})
                extra = {} if window_kwargs is None else window_kwargs(t, t_)
                model_output = model_fn(**model_kwargs, **extra)
                ops.window_blend(value, weight, model_output.contiguous(), t, (t == 0, t_ == T), size - stride)
        finally:
            model_kwargs.update(tensor_dict)
        return ops.window_finalize(value, weight)

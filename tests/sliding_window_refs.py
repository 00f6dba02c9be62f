"""Shared by tests/golden/make_sliding_window_golden.py and the sliding-window tests: the cases of g20_sliding_window.npz, their seeded
inputs, the toy model of the tiler cases, and a torch restatement of the temporal tiler (schedule, mask, the three bf16 roundings)
that runs on the CPU — what the device kernels gf_window_blend / gf_window_finalize are specified to compute, element by element.

The restatement takes `fault=`: one deliberate deviation, which the CPU tests show to break the equality with the golden (a
restatement that cannot fail pins nothing)."""
import numpy as np
import torch

BF = torch.bfloat16

# (T, size, stride) of golden part (a); C = 2, H x W = 2 x 3.  In every case but the last a window with both ramps has them overlap
# in its centre frame only, where the two ramps agree; (6, 4, 1) has a 4-frame window with border 3, whose two middle frames get
# different values from the two ramps — the one case on which the order of the two ramp assignments shows.
TILER_CASES = ((3, 2, 1), (5, 3, 2), (5, 3, 1), (11, 5, 2), (9, 4, 3), (7, 3, 3), (5, 8, 4), (25, 21, 10), (23, 21, 2), (41, 21, 10),
               (41, 21, 20), (6, 4, 1))
TILER_C, TILER_HW = 2, (2, 3)
# (T, size, stride) of golden part (b): the tiny expert of g5 at TINY_LATENT (T = 3) and at a T = 5 latent
MODEL_FN_CASES = ((3, 2, 1), (5, 3, 2), (5, 3, 1))
MODEL_FN_TIMESTEP = 995.9
# golden part (c): the keyword arguments of the pipeline call (T = 5 latent frames)
PIPELINE_KWARGS = dict(seed=0, height=64, width=96, num_frames=17, num_inference_steps=3, cfg_scale=5.0, tiled=True, tile_size=(6, 8),
                       tile_stride=(3, 4), controlnet=False, sliding_window_size=3, sliding_window_stride=2)
FAULTS = ("left_ramp_last", "shift_one", "one_rounding", "descending")


def case_key(T, size, stride):
    return f"T{T}_s{size}_d{stride}"


def tiler_inputs(T, seed=2000):
    """latents, y [1, 2, T, 2, 3] bf16 of a tiler case."""
    g = torch.Generator().manual_seed(seed + T)
    shape = (1, TILER_C, T) + TILER_HW
    return torch.randn(shape, generator=g).to(BF), torch.randn(shape, generator=g).to(BF)


def toy_model_fn(latents=None, y=None, **_):
    """The stand-in model of the tiler cases: elementwise in latents, y and the frame index INSIDE the window (so a window's
    output is not a slice of the dense output), in bf16 with torch's eager roundings."""
    idx = torch.arange(latents.shape[2], dtype=torch.float32).view(1, 1, -1, 1, 1)
    return latents * (0.75 + 0.25 * idx).to(latents.dtype) + y * 0.5


def model_fn_inputs(T):
    """latents [1,16,T,8,12], y [1,20,T,8,12], control [1,16,T,8,12], ctx_posi, ctx_nega: gen_inputs.tiny_inputs() at T = 3, the same
    recipe from another seed at other lengths (the contexts are tiny_inputs()' own)."""
    import gen_inputs as gi
    inp = gi.tiny_inputs()
    if T == gi.TINY_LATENT[2]:
        return inp
    g = torch.Generator().manual_seed(4321 + T)
    b, c, _, h, w = gi.TINY_LATENT
    latents = torch.randn((b, c, T, h, w), generator=g).to(BF)
    y = torch.randn((b, 20, T, h, w), generator=g).to(BF)
    y[:, :4] = (y[:, :4] > 0).to(BF)
    control = torch.randn((b, 16, T, h, w), generator=g).to(BF)
    return dict(latents=latents, y=y, control=control, ctx_posi=inp["ctx_posi"], ctx_nega=inp["ctx_nega"])


# ---------------------------------------------------------------------------------------------- the restatement
def windows(T, size, stride):
    """[(t, t_)] in the order the windows are blended."""
    out = []
    for t in range(0, T, stride):
        if t - stride >= 0 and t - stride + size >= T:
            continue
        out.append((t, min(t + size, T)))
    return out


def mask_1d(n, left_bound, right_bound, border, fault=None):
    """The fp32 mask of an n-frame window, position by position as gf_window_blend forms it: 1, then the left ramp, then the right
    ramp (which therefore wins where the two overlap)."""
    shift = np.float32(1.0 if fault == "shift_one" else 0.5)
    m = np.ones(n, dtype=np.float32)
    b = np.float32(border)

    def left(i):
        if not left_bound and i < border:
            m[i] = (np.float32(i) + shift) / b                    # one correctly rounded fp32 division

    def right(i):
        if not right_bound and i >= n - border:
            m[i] = (np.float32(n - 1 - i) + shift) / b
    for i in range(n):
        for ramp in ((right, left) if fault == "left_ramp_last" else (left, right)):
            ramp(i)
    return torch.from_numpy(m)


def blend(outputs, T, size, stride, fault=None):
    """value [1, C, T, H, W] bf16 from the per-window outputs (in schedule order): value += bf16(out * mask) in bf16, weight += mask
    in bf16, value = bf16(value / weight)."""
    wins = list(zip(windows(T, size, stride), outputs))
    _, C, _, H, W = outputs[0].shape
    value = torch.zeros((1, C, T, H, W), dtype=torch.float32)       # holds bf16 values: every update below is rounded to bf16
    weight = torch.zeros((T,), dtype=torch.float32)
    rb = lambda x: x.to(BF).float()                                # noqa: E731
    for (t, t_), out in (reversed(wins) if fault == "descending" else wins):
        m = rb(mask_1d(t_ - t, t == 0, t_ == T, size - stride, fault))
        mm = m.view(1, 1, -1, 1, 1)
        if fault == "one_rounding":
            value[:, :, t:t_] = rb(out.float() * mm + value[:, :, t:t_])
        else:
            value[:, :, t:t_] = rb(value[:, :, t:t_] + rb(out.float() * mm))
        weight[t:t_] = rb(weight[t:t_] + m)
    return rb(value / weight.view(1, 1, -1, 1, 1)).to(BF)


def run(model_fn, size, stride, latents, y, fault=None):
    """The tiler around `model_fn` on CPU tensors -> (per-window outputs, value)."""
    T = latents.shape[2]
    outs = [model_fn(latents=latents[:, :, t:t_], y=y[:, :, t:t_]) for t, t_ in windows(T, size, stride)]
    return outs, blend(outs, T, size, stride, fault)

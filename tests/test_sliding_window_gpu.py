"""Sliding-window sampling on the GPU: gf_window_blend / gf_window_finalize through the raw C ABI against what the REFERENCE's own
TemporalTiler_BCTHW returned (tests/golden/g20_sliding_window.npz, made by tests/golden/make_sliding_window_golden.py), bit for bit;
model_fn_wan_video and pipe(...) with a window against the reference's windowed forward and call, and against the manual composition
of plain forwards with the two kernels.

One departure from the reference is pinned here as a property: its windowed forward drops the ControlNet (the golden script asserts
that); here the ControlNet follows its window, so the result with a live ControlNet equals the manual composition WITH it and differs
from the result without."""
import os

import numpy as np
import pytest
import torch

import gen_inputs as gi
import sliding_window_refs as sw
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g20_sliding_window.npz"))


def _lib():
    from goal_force_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().gf_last_error().decode()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _blend(value, weight, win, t0, left, right, border, C=None, T=None, HW=None, sc=None, st=None, n=None):
    """gf_window_blend on value [C, T, HW] (any strides of C and T), every argument overridable (the refusals)."""
    return _lib().gf_window_blend(_ptr(value), _ptr(weight), _ptr(win), value.shape[0] if C is None else C, value.shape[1] if T is None else T,
                                  value.shape[2] if HW is None else HW, value.stride(0) if sc is None else sc,
                                  value.stride(1) if st is None else st, t0, win.shape[1] if n is None else n, left, right, border, _stream())


def _finalize(value, weight, C=None, T=None, HW=None, sc=None, st=None):
    return _lib().gf_window_finalize(_ptr(value), _ptr(weight), value.shape[0] if C is None else C, value.shape[1] if T is None else T,
                                     value.shape[2] if HW is None else HW, value.stride(0) if sc is None else sc,
                                     value.stride(1) if st is None else st, _stream())


class _Framed:
    """Zeroed accumulators inside guarded storage: value [C, T, HW] is a slice (strided in C and T, its pixel rows padded) of a
    NaN-filled parent, weight [T] the head of a buffer whose tail holds sentinels."""

    def __init__(self, C, T, HW):
        self.parent = torch.full((C + 1, T + 3, HW + 5), float("nan"), dtype=BF, device="cuda")
        self.value = self.parent[:C, 1:T + 1, :HW]
        self.value.zero_()
        self.inside = torch.zeros(self.parent.shape, dtype=torch.bool, device="cuda")
        self.inside[:C, 1:T + 1, :HW] = True
        self.wbuf = torch.full((T + 4,), 7.0, dtype=BF, device="cuda")
        self.weight = self.wbuf[:T]
        self.weight.zero_()
        assert not self.value.is_contiguous() and self.value.stride(2) == 1

    def check_guards(self):
        assert bool(torch.isnan(self.parent[~self.inside]).all()), "a store landed outside value"
        assert bool((self.wbuf[self.weight.numel():] == 7.0).all()), "a store landed behind weight"


def _windows_of(g, T, size, stride):
    k = sw.case_key(T, size, stride)
    wins = gi.from_u16(g[f"a_{k}_windows"])[0]                     # [C, sum of lengths, H, W]
    outs, at = [], 0
    for t, t_ in sw.windows(T, size, stride):
        outs.append((t, t_, wins[:, at:at + t_ - t].reshape(wins.shape[0], t_ - t, -1).contiguous().cuda()))
        at += t_ - t
    return outs, gi.from_u16(g[f"a_{k}_value"])[0].reshape(wins.shape[0], T, -1)


# ---------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("T,size,stride", sw.TILER_CASES)
def test_kernels_reproduce_the_reference_tiler_bit_for_bit(golden, T, size, stride):
    outs, want = _windows_of(golden, T, size, stride)
    f = _Framed(want.shape[0], T, want.shape[2])
    for t, t_, win in outs:
        assert _blend(f.value, f.weight, win, t, int(t == 0), int(t_ == T), size - stride) == 0, _err()
    assert bool((f.weight.float() > 0).all())
    assert _finalize(f.value, f.weight) == 0, _err()
    torch.cuda.synchronize()
    assert torch.equal(f.value.cpu(), want), (T, size, stride)
    f.check_guards()


def test_kernels_over_more_than_one_block_and_grid_stride_trip():
    """3 x 4 x 50021 window elements: more than the 2048 x 256 lanes of a full grid, an odd pixel count; against the CPU restatement
    (tests/sliding_window_refs.py, itself pinned to the reference bit for bit by the CPU tests)."""
    C, T, HW, size, stride = 3, 7, 50021, 4, 2
    g = torch.Generator().manual_seed(5)
    outs = [torch.randn((1, C, t_ - t, HW, 1), generator=g).to(BF) for t, t_ in sw.windows(T, size, stride)]
    assert outs[0].numel() > 2048 * 256
    want = sw.blend(outs, T, size, stride)[0, :, :, :, 0]
    f = _Framed(C, T, HW)
    for (t, t_), o in zip(sw.windows(T, size, stride), outs):
        assert _blend(f.value, f.weight, o[0, :, :, :, 0].contiguous().cuda(), t, int(t == 0), int(t_ == T), size - stride) == 0, _err()
    assert _finalize(f.value, f.weight) == 0, _err()
    torch.cuda.synchronize()
    assert torch.equal(f.value.cpu(), want)
    f.check_guards()


def test_a_window_that_touches_both_ends_is_the_identity():
    g = torch.Generator().manual_seed(6)
    win = torch.randn((2, 5, 6), generator=g).to(BF).cuda()
    for border in (0, 1, 4, 9):                                  # no ramp is requested: any border passes, and none is applied
        f = _Framed(2, 5, 6)
        assert _blend(f.value, f.weight, win, 0, 1, 1, border) == 0, _err()
        assert torch.equal(f.value, win) and bool((f.weight == 1).all())
        assert _finalize(f.value, f.weight) == 0, _err()
        assert torch.equal(f.value, win)
        f.check_guards()
    f = _Framed(2, 7, 6)                                         # ... and border 0 with ramps requested is all ones as well
    assert _blend(f.value, f.weight, win, 1, 0, 0, 0) == 0, _err()
    assert torch.equal(f.value[:, 1:6], win) and f.weight.tolist() == [0, 1, 1, 1, 1, 1, 0]
    f.check_guards()


def test_entry_points_refuse_by_message_and_touch_nothing():
    g = torch.Generator().manual_seed(7)
    win = torch.randn((2, 3, 6), generator=g).to(BF).cuda()
    f = _Framed(2, 5, 6)
    f.value.copy_(torch.randn((2, 5, 6), generator=g).to(BF))
    f.weight.copy_(torch.rand((5,), generator=g).to(BF) + 1)
    parent0, wbuf0 = f.parent.clone(), f.wbuf.clone()
    v, w = f.value, f.weight
    blend_cases = [
        (lambda: _lib().gf_window_blend(None, _ptr(w), _ptr(win), 2, 5, 6, v.stride(0), v.stride(1), 1, 3, 0, 0, 1, _stream()), "null pointer"),
        (lambda: _lib().gf_window_blend(_ptr(v), None, _ptr(win), 2, 5, 6, v.stride(0), v.stride(1), 1, 3, 0, 0, 1, _stream()), "null pointer"),
        (lambda: _lib().gf_window_blend(_ptr(v), _ptr(w), None, 2, 5, 6, v.stride(0), v.stride(1), 1, 3, 0, 0, 1, _stream()), "null pointer"),
        (lambda: _blend(v, w, win, 1, 0, 0, 1, n=0), "len must be positive"),
        (lambda: _blend(v, w, win, 1, 0, 0, 1, n=-3), "len must be positive"),
        (lambda: _blend(v, w, win, -1, 0, 0, 1), "window outside the T frames"),
        (lambda: _blend(v, w, win, 3, 0, 0, 1), "window outside the T frames"),                 # t0 + len = 6 > T
        (lambda: _blend(v, w, win, 0, 0, 0, 1, n=6), "window outside the T frames"),
        (lambda: _blend(v, w, win, 1, 0, 0, -1), "border must not be negative"),
        (lambda: _blend(v, w, win, 1, 1, 1, -1), "border must not be negative"),
        (lambda: _blend(v, w, win, 1, 0, 0, 3), "border must be smaller than len"),             # border == len
        (lambda: _blend(v, w, win, 1, 1, 0, 4), "border must be smaller than len"),
        (lambda: _blend(v, w, win, 1, 0, 1, 3), "border must be smaller than len"),
        (lambda: _blend(v, w, win, 1, 0, 0, 1, C=0), "positive sizes"),
        (lambda: _blend(v, w, win, 1, 0, 0, 1, HW=0), "positive sizes"),
        (lambda: _blend(v, w, win, 1, 0, 0, 1, st=5), "non-overlapping planes"),                # T stride below HW
        (lambda: _blend(v, w, win, 1, 0, 0, 1, sc=4 * v.stride(1)), "non-overlapping planes"),   # C stride below the plane
    ]
    finalize_cases = [
        (lambda: _lib().gf_window_finalize(None, _ptr(w), 2, 5, 6, v.stride(0), v.stride(1), _stream()), "null pointer"),
        (lambda: _lib().gf_window_finalize(_ptr(v), None, 2, 5, 6, v.stride(0), v.stride(1), _stream()), "null pointer"),
        (lambda: _finalize(v, w, T=0), "positive sizes"),
        (lambda: _finalize(v, w, C=-1), "positive sizes"),
        (lambda: _finalize(v, w, st=5), "non-overlapping planes"),
    ]
    for name, cases in (("gf_window_blend", blend_cases), ("gf_window_finalize", finalize_cases)):
        for call, msg in cases:
            rc = call()
            assert rc != 0 and _err().startswith(name + ":") and msg in _err(), (rc, _err(), msg)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))     # noqa: E731  (bit patterns: the parent holds NaN)
    assert same(f.parent, parent0) and same(f.wbuf, wbuf0), "a refused call wrote"
    # what the refusals border on is accepted: border = len - 1 with both ramps, the last window position
    assert _blend(v, w, win, 2, 0, 0, 2) == 0, _err()
    assert not same(f.parent, parent0)
    f.check_guards()


def test_ops_wrappers_validate_and_take_the_five_dim_tensors():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    g = torch.Generator().manual_seed(8)
    out = torch.randn((1, 2, 3, 2, 3), generator=g).to(BF).cuda()
    value, weight = torch.zeros((1, 2, 5, 2, 3), dtype=BF, device="cuda"), torch.zeros((5,), dtype=BF, device="cuda")
    ops.window_blend(value, weight, out, 1, (True, True), 1)
    assert torch.equal(value[:, :, 1:4], out) and weight.tolist() == [0, 1, 1, 1, 0]
    assert ops.window_finalize(value[:, :, 1:4], weight[1:4].contiguous()) is not None          # a T slice: strided value
    assert torch.equal(value[:, :, 1:4], out)
    for bad, msg in ((dict(value=value.float()), "expected dtype"), (dict(value=value.cpu()), "must be on the GPU"),
                     (dict(weight=weight[:4]), r"expected contiguous \[5\]"), (dict(win=out[:, :, :, :, :2]), "window_blend.win"),
                     (dict(win=out.transpose(3, 4)), "window_blend.win"), (dict(value=value.transpose(3, 4)), "must be contiguous"),
                     (dict(value=value[:, :, :, :1].expand(1, 2, 5, 2, 3)), "must be contiguous")):
        kw = dict(value=value, weight=weight, win=out)
        kw.update(bad)
        with pytest.raises(GoalForceError, match=msg):
            ops.window_blend(kw["value"], kw["weight"], kw["win"], 1, (True, True), 1)
    with pytest.raises(GoalForceError, match="window outside the T frames"):
        ops.window_blend(value, weight, out, 3, (False, True), 1)


# ---------------------------------------------------------------------------------------------- model_fn
def _tiny(zero_cn=False, dit_seed=41):
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    cfg = gi.TINY
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(gi.dit_sd(cfg, seed=dit_seed), strict=True)
    cn = ControlNet(gi.TINY_CONTROLNET_LAYERS, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
    cn.load_state_dict(gi.controlnet_sd(cfg, gi.TINY_CONTROLNET_LAYERS, seed=42, zero_convs_zero=zero_cn), strict=True)
    return dit.to(BF).cuda(), cn.to(BF).cuda()


@pytest.fixture(scope="module")
def tiny():
    return _tiny()


def _inputs(T):
    return {k: v.cuda() for k, v in sw.model_fn_inputs(T).items()}


def _ts():
    return torch.tensor([sw.MODEL_FN_TIMESTEP], dtype=BF).cuda()


def _manual(dit, inp, size, stride, context, cn=None, **kw):
    """Plain forwards on the slices, blended with the two ops wrappers."""
    from goal_force_amd import ops
    from goal_force_amd.model_fn import model_fn_wan_video
    lat = inp["latents"]
    T = lat.shape[2]
    value, weight = torch.zeros_like(lat), torch.zeros((T,), dtype=BF, device="cuda")
    for t, t_ in sw.windows(T, size, stride):
        more = {} if cn is None else dict(controlnet=cn, control_signal_video_latents=inp["control"][:, :, t:t_].contiguous(),
                                          elide_zero_controlnet=False)
        out = model_fn_wan_video(dit, latents=lat[:, :, t:t_].contiguous(), y=inp["y"][:, :, t:t_].contiguous(), timestep=_ts(),
                                 context=context, **more, **kw)
        ops.window_blend(value, weight, out, t, (t == 0, t_ == T), size - stride)
    return ops.window_finalize(value, weight)


@pytest.mark.parametrize("T,size,stride", sw.MODEL_FN_CASES)
def test_windowed_model_fn_vs_the_reference_golden(golden, tiny, T, size, stride):
    from goal_force_amd.model_fn import model_fn_wan_video
    dit, _ = tiny
    k = sw.case_key(T, size, stride)
    assert gi.same_checksum(gi.checksum(gi.dit_sd(gi.TINY, seed=41)), golden["ck_dit"])
    assert gi.same_checksum(gi.checksum(sw.model_fn_inputs(T)), golden[f"b_{k}_ck_inputs"])
    inp = _inputs(T)
    out = model_fn_wan_video(dit, latents=inp["latents"], timestep=_ts(), context=inp["ctx_posi"], y=inp["y"],
                             sliding_window_size=size, sliding_window_stride=stride)
    f32 = torch.from_numpy(golden[f"b_{k}_f32"])
    e, e_ref = rel_l2(out.cpu().float(), f32), rel_l2(gi.from_u16(golden[f"b_{k}_bf16"]).float(), f32)
    print(f"g20 (b) {k}: vs fp32 {e:.3e} (reference bf16 {e_ref:.3e})")
    assert out.shape == inp["latents"].shape and out.dtype == BF
    assert e < 1e-2 and e < 2 * e_ref + 1e-4, f"{k}: vs fp32 {e:.3e} (reference bf16 {e_ref:.3e})"


@pytest.mark.parametrize("T,size,stride", sw.MODEL_FN_CASES)
def test_windowed_model_fn_is_the_manual_composition_with_and_without_a_live_controlnet(tiny, T, size, stride):
    from goal_force_amd.model_fn import model_fn_wan_video
    dit, cn = tiny
    inp = _inputs(T)
    kw = dict(latents=inp["latents"], timestep=_ts(), context=inp["ctx_posi"], y=inp["y"], sliding_window_size=size,
              sliding_window_stride=stride)
    plain = model_fn_wan_video(dit, **kw)
    assert torch.equal(plain, _manual(dit, inp, size, stride, inp["ctx_posi"]))
    assert not cn.all_zero()
    with_cn = model_fn_wan_video(dit, controlnet=cn, control_signal_video_latents=inp["control"], elide_zero_controlnet=False, **kw)
    assert torch.equal(with_cn, _manual(dit, inp, size, stride, inp["ctx_posi"], cn=cn))
    assert not torch.equal(with_cn, plain), "the ControlNet did not follow its window"
    # (a window is not a slice of the dense forward: attention sees only the window's frames)
    dense = model_fn_wan_video(dit, **{k: v for k, v in kw.items() if not k.startswith("sliding")})
    assert not torch.equal(dense, plain)
    assert torch.equal(inp["latents"], _inputs(T)["latents"])          # the inputs are left as they were


def test_a_clip_no_longer_than_the_window_is_the_plain_forward(tiny):
    from goal_force_amd.model_fn import model_fn_wan_video
    dit, cn = tiny
    inp = _inputs(3)
    kw = dict(latents=inp["latents"], timestep=_ts(), context=inp["ctx_posi"], y=inp["y"])
    want = model_fn_wan_video(dit, **kw)
    want_cn = model_fn_wan_video(dit, controlnet=cn, control_signal_video_latents=inp["control"], elide_zero_controlnet=False, **kw)
    for size, stride in ((3, 2), (3, 3), (8, 4), (21, 10), (4, 1)):
        assert torch.equal(model_fn_wan_video(dit, sliding_window_size=size, sliding_window_stride=stride, **kw), want)
        assert torch.equal(model_fn_wan_video(dit, controlnet=cn, control_signal_video_latents=inp["control"], elide_zero_controlnet=False,
                                              sliding_window_size=size, sliding_window_stride=stride, **kw), want_cn)


def test_cfg_shared_under_windows_is_bit_identical_and_drained(tiny):
    """The uncond window t takes the block-0 halves of the cond window t: same bits as without the memo, for both branch orders."""
    from goal_force_amd.model_fn import model_fn_wan_video
    dit, cn = tiny
    inp = _inputs(5)
    for size, stride in ((3, 2), (3, 1)):
        kw = dict(latents=inp["latents"], timestep=_ts(), y=inp["y"], controlnet=cn, control_signal_video_latents=inp["control"],
                  elide_zero_controlnet=False, sliding_window_size=size, sliding_window_stride=stride)
        want_p = model_fn_wan_video(dit, context=inp["ctx_posi"], **kw)
        want_n = model_fn_wan_video(dit, context=inp["ctx_nega"], **kw)
        assert not torch.equal(want_p, want_n)
        starts = {("window", t) for t, _ in sw.windows(5, size, stride)}
        for first, second, w1, w2 in (("ctx_posi", "ctx_nega", want_p, want_n), ("ctx_nega", "ctx_posi", want_n, want_p)):
            pair = {}
            got1 = model_fn_wan_video(dit, context=inp[first], cfg_shared=pair, **kw)
            assert set(pair) == starts and all(set(sub) == {"cn0", "dit0"} and all("x" in m for m in sub.values()) for sub in pair.values())
            got2 = model_fn_wan_video(dit, context=inp[second], cfg_shared=pair, **kw)
            assert torch.equal(got1, w1) and torch.equal(got2, w2)
            assert set(pair) == starts and all(len(m) == 0 for sub in pair.values() for m in sub.values())


def test_frame_window_sparse_attention_under_windows_is_its_manual_composition():
    """A 3-frame window of 28 x 26 tokens is 2184 keys — above ops.VT_MIN_KV, where a switched block runs the sparse kernel."""
    from goal_force_amd import dit as dit_mod, ops
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.sparse_attention import FrameWindow
    dit, _ = _tiny()
    g = torch.Generator().manual_seed(99)
    T, H, W = 5, 56, 52
    assert 3 * (H // 2) * (W // 2) >= ops.VT_MIN_KV
    inp = dict(latents=torch.randn((1, 16, T, H, W), generator=g).to(BF).cuda(), y=torch.randn((1, 20, T, H, W), generator=g).to(BF).cuda(),
               ctx_posi=gi.tiny_inputs()["ctx_posi"].cuda())
    kw = dict(latents=inp["latents"], timestep=_ts(), context=inp["ctx_posi"], y=inp["y"], sliding_window_size=3, sliding_window_stride=2)
    dense = model_fn_wan_video(dit, **kw)
    fw = FrameWindow(0, 0)
    assert fw((3, H // 2, W // 2)).density < 1.0
    try:
        dit_mod.enable_sparse_attention(dit, fw)
        sparse = model_fn_wan_video(dit, **kw)
        assert torch.equal(sparse, _manual(dit, inp, 3, 2, inp["ctx_posi"]))
        assert not torch.equal(sparse, dense) and bool(torch.isfinite(sparse.float()).all())
        assert torch.equal(model_fn_wan_video(dit, sparse_dense=True, **kw), dense)      # `sparse_dense` reaches every window
    finally:
        dit_mod.enable_sparse_attention(dit, None)
    assert torch.equal(model_fn_wan_video(dit, **kw), dense)


def test_tea_cache_and_sequence_parallelism_are_refused_with_a_window(tiny):
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.teacache import TeaCache
    dit, _ = tiny
    inp = _inputs(5)
    kw = dict(latents=inp["latents"], timestep=_ts(), context=inp["ctx_posi"], y=inp["y"], sliding_window_size=3, sliding_window_stride=2)
    with pytest.raises(GoalForceError, match="tea_cache with a sliding window"):
        model_fn_wan_video(dit, tea_cache=TeaCache(3, rel_l1_thresh=0.26, model_id="Wan2.1-I2V-14B-480P"), **kw)
    with pytest.raises(GoalForceError, match="sequence parallelism with a sliding window"):
        model_fn_wan_video(dit, use_unified_sequence_parallel=True, **kw)
    with pytest.raises(GoalForceError, match="sequence parallelism with a sliding window"):
        model_fn_wan_video(dit, sequence_parallel=object(), **kw)


# ---------------------------------------------------------------------------------------------- the pipeline
class FixedPrompter:
    """What the golden run used in place of WanPrompter (tests/test_pipeline_call_gpu.py)."""

    def __init__(self, inp):
        self.inp = inp

    def encode_prompt(self, prompt, positive=True, device="cuda"):
        return (self.inp["ctx_posi"] if prompt == gi.PIPELINE_PROMPTS[0] else self.inp["ctx_nega"]).to(device)


def test_pipeline_call_with_a_window_vs_the_reference_call(golden, monkeypatch):
    """`pipe(prompt, negative_prompt, input_image, **sliding_window_refs.PIPELINE_KWARGS)` on the tiny experts of g13 against the
    reference's own `__call__` with these arguments: the same window forwards in the same order (expert, frames, timestep), and final
    latents under test_pipeline_call_gpu.py's bar."""
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    from goal_force_amd.temporal_tiler import TemporalTiler_BCTHW
    from goal_force_amd.vae import WanVideoVAE
    g, cfg = golden, gi.TINY

    def expert(seed):
        m = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
        m.load_state_dict(gi.dit_sd(cfg, seed=seed), strict=True)
        return m.to(BF).cuda()
    g6 = np.load(os.path.join(GOLDEN, "g6_vae.npz"))
    vae = WanVideoVAE()
    vae.load_state_dict({"model." + k: t for k, t in gi.vae_decoder_sd(list(g6["names"]), g6["shapes"], seed=61).items()}, strict=True)
    pipe = WanVideoPipeline.from_modules(expert(41), expert(43), None, None, vae=vae.to(BF).cuda())
    image, _ = gi.preloop_inputs()
    inp = gi.tiny_inputs()
    assert gi.same_checksum(gi.checksum([torch.from_numpy(np.array(image)).float(), inp["ctx_posi"], inp["ctx_nega"]]), g["c_ck_inputs"])
    assert str(g["c_kwargs_repr"]) == repr(sorted(sw.PIPELINE_KWARGS.items())), "the golden was made with these keyword arguments"
    pipe.prompter = FixedPrompter(inp)
    calls = []
    real_run = TemporalTiler_BCTHW.run

    def spy_run(self, model_fn, *a, **k):
        whole = k["model_kwargs"]["latents"]

        def spy_fn(**kw):
            lat = kw["latents"]
            n = lat.shape[2]
            at = [t for t in range(whole.shape[2] - n + 1) if torch.equal(lat, whole[:, :, t:t + n])]
            assert len(at) == 1, at
            calls.append((float(kw["dit"] is pipe.dit2), float(at[0]), float(at[0] + n), float(kw["timestep"].float())))
            return model_fn(**kw)
        return real_run(self, spy_fn, *a, **k)
    monkeypatch.setattr(TemporalTiler_BCTHW, "run", spy_run)
    lat = pipe(prompt=gi.PIPELINE_PROMPTS[0], negative_prompt=gi.PIPELINE_PROMPTS[1], input_image=image, output_type="latent",
               **sw.PIPELINE_KWARGS)
    want_calls = [tuple(r) for r in g["c_calls_bf16"].tolist()]
    assert calls == want_calls, (calls, want_calls)
    lat = lat.float().cpu()
    f32, ref_bf = torch.from_numpy(g["c_latents_f32"]), gi.from_u16(g["c_latents_bf16"]).float()
    e, e_ref, e_bf = rel_l2(lat, f32), rel_l2(ref_bf, f32), rel_l2(lat, ref_bf)
    print(f"g20 (c): latents vs fp32 {e:.3e} (reference bf16 {e_ref:.3e}), vs ref-bf16 {e_bf:.3e}")
    assert tuple(lat.shape) == (1, 16, 5, 8, 12)
    assert e < 1.25 * e_ref + 1e-3 and e_bf < 2 * e_ref, f"latents vs fp32 {e:.3e}, vs ref-bf16 {e_bf:.3e} (reference bf16 vs fp32 {e_ref:.3e})"


def test_denoise_with_a_window_same_bits_with_the_shared_prefix_and_on_two_streams():
    from goal_force_amd.pipeline import WanVideoPipeline
    inp = _inputs(5)
    dit1, cn1 = _tiny(False)
    dit2, cn2 = _tiny(True, dit_seed=43)
    pipe = WanVideoPipeline.from_modules(dit1, dit2, cn1, cn2)
    run = lambda **kw: pipe.denoise(inp["latents"], inp["ctx_posi"], inp["ctx_nega"], inp["y"], inp["control"], num_inference_steps=3,   # noqa: E731
                                    cfg_scale=5.0, controlnet=True, **kw)
    win = dict(sliding_window_size=3, sliding_window_stride=2)
    assert pipe.share_cfg_prefix and not pipe.cfg_streams
    a = run(**win)
    assert a.shape == inp["latents"].shape and bool(torch.isfinite(a.float()).all()) and not torch.equal(a, run())
    pipe.share_cfg_prefix = False
    assert torch.equal(a, run(**win))
    pipe.share_cfg_prefix = True
    pipe.cfg_streams = True
    for _ in range(2):
        assert torch.equal(a, run(**win))
    assert pipe._cfg_side_stream is not None
    torch.cuda.synchronize()

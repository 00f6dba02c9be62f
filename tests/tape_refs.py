"""fp64 references, fp32 restatements and the row statistic of the training TAPE (goal_force_amd/training.py): the GEMM backward, the
small autograd functions, DiTBlockFn.backward and model_fn_train.  Plain helper: CPU tensors in, CPU tensors out; it imports the
oracle and the other *_refs helpers, nothing from goal_force_amd, and needs no GPU.

* `block_grads_ref` / `model_grads_ref`: fp64 autograd of oracle.wan_oracle.dit_block / oracle.train_oracle.loss_and_grads on the
  bf16 inputs upcast.  (The oracle's two norms compute in fp32 whatever they are given: 2^-24 relative, four thousand times below the
  bf16 noise the statistic measures.)
* `block_chain` (= `block_fwd` + `block_bwd`): the tape of DiTBlockFn.backward restated in torch from DIT:197-230 and the calculus —
  fp32 arithmetic with ONE bf16 rounding wherever the tape's kernels round (every GEMM output, every row kernel's output, every add),
  fp32 where they accumulate in fp32 (column sums, the norm weights' sums).  The stages are the restatements the kernels' own tests
  already hold: gemm_refs.gemm_f32, forward_refs.layernorm_f32 / rmsnorm_rope_f32 / act_f32, backward_refs.*_f32,
  attention_bwd_refs.chain_f32.  `order` picks the GEMMs' summation order (0: K tiles of 64 from tile 0; 1: K tiles of 32, column tile j
  started at tile j), so the two restatements are two draws of the rounding noise.  `prescale=True` restates dit.q_rotation under
  attn_q_prescale: q's table is (c cos, c sin), c = fp32(fp32(1 / sqrt 128) fp32(log2 e)), and the attention's scale is ln 2.
* `glue_chain`: linear_dx / linear_dw / bias_grad (LinearFn, PatchEmbedFn on the gathered columns, InjectFn); `loss_chain`: MseLossFn;
  `model_chain`: model_fn_train + the loss, forward and backward, on those pieces.

THE ROW STATISTIC.  For a gradient tensor T and a slice s of it
      ratio(s) = dev_rms(got, s) / max(dev_rms(chain order 0, s), floor_T),
  dev_rms(t, s) the rms over the slice of t - ref64, floor_T a quarter of the median of the chain's dev_rms over T's slices (a slice the
  chain happens to hit almost exactly must not make a right result look bad).  Slices: every row and every column of a 2-D weight (conv
  and zero-conv weights flattened behind their first dim), the 6 rows of `modulation`, every token row of dx, a 1-D tensor as one
  slice.  A slice whose reference is identically zero must be exactly zero in `got`.
  1.0 means "as far from fp64 as a right restatement is".  The threshold is MEASURED on the CPU, never on the device: ROW_WORST is the
  worst ratio of the order-1 restatement over every case the GPU tests run (tests/test_tape_refs_cpu.py measures and asserts it), per
  tensor group, and the device's bar is ROW_BAR = 1.25 x that (summation order and the hardware exp2: attention_bwd_refs' margin).
  The two orders differ where a right kernel may: the GEMMs' K order and the attention forward's softmax (every key at once / online
  over key tiles of 64 with a running maximum).  Everything downstream of a flipped rounding is then redrawn, so most of the noise of
  the self-attention branch and behind it is independent between the two; a stage both restatements evaluate alike (the row kernels,
  a cross-attention over <= 64 keys) is common to both and cancels from the ratio.
  Groups, measured over cases() and the two whole-tape cases (the block cases alone / the whole tape alone in brackets):
      weight       2.03  (1.74 / 2.03)  2-D weight gradients not listed below, the patch embedding's and the zero convs' included
      attn_weight  3.89  (3.89 / 3.34)  self_attn.v / o, cross_attn.k / v / o: the token-side operand of these five GEMMs is the
                                        attention's own output or gradient (a, a2, dv, dk) — the stage the two orders draw apart — and a row
                                        of dW = dY^T X is ONE sum over the tokens, dominated by the few tokens (with 7 context rows: by
                                        all seven) whose dy is largest: a row's deviations are a handful of random variables, not 256,
                                        and the worst of ~1500 rows lies near 3 - 4 standard deviations (attention_bwd_refs' far_* classes
                                        show the same).  Their own, wider figure keeps the other weights' sharp
      vector       1.17  1-D: biases, norm weights — one slice each
      modulation   1.075
      dx           1.22
  If the device later exceeds a bar, that is a finding to explain from the code, not a figure to raise.
"""
import math
import types

import torch

import attention_bwd_refs as AB
import backward_refs as BR
import forward_refs as FR
import gemm_refs as GR
from oracle import train_oracle as to
from oracle import wan_oracle as wo

BF = torch.bfloat16
HD = 128
EPS = 1e-6
PARAM_NAMES = (
    "modulation",
    "self_attn.q.weight", "self_attn.q.bias", "self_attn.k.weight", "self_attn.k.bias", "self_attn.v.weight",
    "self_attn.v.bias", "self_attn.o.weight", "self_attn.o.bias", "self_attn.norm_q.weight", "self_attn.norm_k.weight",
    "norm3.weight", "norm3.bias",
    "cross_attn.q.weight", "cross_attn.q.bias", "cross_attn.k.weight", "cross_attn.k.bias", "cross_attn.v.weight",
    "cross_attn.v.bias", "cross_attn.o.weight", "cross_attn.o.bias", "cross_attn.norm_q.weight", "cross_attn.norm_k.weight",
    "ffn.0.weight", "ffn.0.bias", "ffn.2.weight", "ffn.2.bias",
)
BLOCK_FAULTS = ("dx2b_no_residual", "dgate2_from_o", "mod_rows_swapped", "mod1_from_dh3", "dh1_no_k", "dh1_no_v", "cross_kv_from_x",
                "norm3w_from_x1", "q_bwd_plain_table", "bias_drops_last_row", "pad_row_garbage", "ffn0_dw_from_f", "row_eps")
MODEL_FAULTS = ("fanout_g1_only", "inject_dstate_for_dout")
FAULTS = BLOCK_FAULTS + MODEL_FAULTS

# measured by tests/test_tape_refs_cpu.py::test_row_worst_reproduces (the worst ratio of the order-1 restatement per group over
# cases() and the whole-tape cases: 2.0254, 3.892, 1.168, 1.0748, 1.2236); the bars are 1.25 x these and nothing else
ROW_WORST = {"weight": 2.03, "attn_weight": 3.89, "vector": 1.17, "modulation": 1.075, "dx": 1.22}
ROW_BAR = {k: 1.25 * v for k, v in ROW_WORST.items()}
LOSS_MARGIN = 1.25
# fault `row_eps` (one row of a weight gradient times 1 + eps, eps = 2 ROW_BAR x the tensor's relative row noise: 2.9e-2 .. 4.1e-2 for the
# FFN, 3.8e-2 for cross_attn.q, 5.4e-2 .. 5.7e-2 for self_attn.q / k, 5.8e-2 .. 8.9e-2 for the attn_weight group) is outside at the stated
# eps for every tensor and case but self_attn.o.weight at 72 and 64 tokens, whose middle row carries 1.5 - 2 x the median noise: there the
# smallest eps outside is 1.5 x (64 tokens) and 2 x (72 tokens) the stated one.  The CPU test searches EPS_FACTORS and holds EPS_FACTOR.
EPS_FACTORS = (1, 1.5, 2, 3, 4, 6, 8)
EPS_FACTOR = {"weight": 1, "attn_weight": 2}


def pad64(n):
    return -(-n // 64) * 64


def q_prescale():
    return AB.q_prescale()


# ---------------------------------------------------------------------------------------------------------------------
# the cases shared by the CPU and the GPU test
def cases():
    """dicts: name, cfg ('TINY' | 'MID'), grid (f, h, w), ctx_len, prescale, seed."""
    out = [dict(name="tiny-72-7", cfg="TINY", grid=(3, 4, 6), ctx_len=7, prescale=True, seed=101),
           dict(name="tiny-72-7-plainq", cfg="TINY", grid=(3, 4, 6), ctx_len=7, prescale=False, seed=101),
           dict(name="tiny-64-64", cfg="TINY", grid=(1, 8, 8), ctx_len=64, prescale=True, seed=102),
           dict(name="tiny-65-65", cfg="TINY", grid=(1, 5, 13), ctx_len=65, prescale=True, seed=103),
           dict(name="tiny-130-7", cfg="TINY", grid=(1, 10, 13), ctx_len=7, prescale=True, seed=104),
           dict(name="mid-130-65", cfg="MID", grid=(1, 10, 13), ctx_len=65, prescale=True, seed=105)]
    return out


BASE_CASE = "tiny-72-7"
SUBSETS = {"all": PARAM_NAMES, "none": (), "modulation": ("modulation",), "ffn2w": ("ffn.2.weight",),
           "sa_qw_kb": ("self_attn.q.weight", "self_attn.k.bias"), "ca_kw_vb": ("cross_attn.k.weight", "cross_attn.v.bias"),
           "n3b_canq": ("norm3.bias", "cross_attn.norm_q.weight"), "sa_ow": ("self_attn.o.weight",)}
MODEL_CASES = (False, True)               # zero_convs_zero


def case_inputs(case, gi):
    """(cfg, sd, x [S, D], ctx [L, D], t_mod [1, 6, D], dout [S, D]) bf16 of a case; `gi` is tests/golden/gen_inputs."""
    cfg = getattr(gi, case["cfg"])
    tokens = case["grid"][0] * case["grid"][1] * case["grid"][2]
    sd = gi.block_sd(torch.Generator().manual_seed(case["seed"]), cfg["dim"], cfg["ffn_dim"], "", BF)
    x, ctx, t_mod = gi.block_inputs(cfg["dim"], tokens, case["ctx_len"], seed=case["seed"] + 1000)
    dout = torch.randn(x.shape, generator=torch.Generator().manual_seed(case["seed"] + 2000)).to(BF)
    return cfg, sd, x[0], ctx[0], t_mod, dout[0]


def zero_gate(sd, t_mod, row):
    """t_mod with row `row` the negative of the block's modulation row: bf16(modulation + t_mod) is exactly +0 there."""
    t = t_mod.clone()
    t[0, row] = -sd["modulation"][0, row]
    return t


def rope_tables(head_dim, grid):
    """fp32 (cos, sin) [S, head_dim/2] of the oracle's complex table, and the table itself."""
    fr = wo.rope_freqs_3d(head_dim, *grid)
    return fr.real.float().contiguous(), fr.imag.float().contiguous(), fr


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references
def block_grads_ref(cfg, sd, x, ctx, t_mod, dout, grid):
    """(dx [S, D], {name: gradient}) in fp64: autograd of the oracle's block on the bf16 inputs upcast."""
    with torch.enable_grad():
        sdd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xd = x.double()[None].requires_grad_(True)
        fr = wo.rope_freqs_3d(cfg["dim"] // cfg["num_heads"], *grid)
        y = wo.dit_block(xd, ctx.double()[None], t_mod.double(), fr, sdd, "", cfg["num_heads"], cfg["eps"])
        y.backward(dout.double()[None])
    return xd.grad[0], {k: v.grad for k, v in sdd.items()}


def model_grads_ref(cfg, dit_sd, cn_sd, n_cn, inputs, timestep_id):
    """(loss, {name: gradient}) in fp64 through oracle.train_oracle.loss_and_grads; the timestep is the bf16-rounded one the device
    draws (GF:184), or the yardstick would measure another step."""
    loss, grads = to.loss_and_grads(dit_sd, cn_sd, cfg, n_cn, inputs, timestep_id, dtype=torch.float64, timestep_dtype=BF)
    return float(loss), grads


# ---------------------------------------------------------------------------------------------------------------------
# the stages
def _gemm(a, w, bias, order, epi=GR.EPI_BIAS, resid=None):
    """bf16 [M, N] = epilogue(a w^T + bias); K is padded with zeros to the order's K tile (what a padded operand is to the kernel)."""
    ktile = 64 if order == 0 else 32
    K = a.shape[1]
    kp = -(-K // 64) * 64
    if kp != K:
        a = torch.nn.functional.pad(a, (0, kp - K))
        w = torch.nn.functional.pad(w, (0, kp - K))
    return GR.gemm_f32(a, w, bias, epi, resid, None, None, ktile, order)


def _tpad(t, mp, garbage=False):
    """transpose_pad: [M, C] -> [C, mp], zeros behind M (fault: one NaN in the first pad row)."""
    out = torch.zeros((t.shape[1], mp), dtype=t.dtype)
    out[:, :t.shape[0]] = t.t()
    if garbage and mp > t.shape[0]:
        out[t.shape[1] // 2, t.shape[0]] = math.nan
    return out


def linear_dx(dy, w, order=0):
    return _gemm(dy, w.t().contiguous(), None, order)


def linear_dw(dy, x, order=0, fault=None):
    mp = pad64(dy.shape[0])
    return _gemm(_tpad(dy, mp), _tpad(x, mp, garbage=fault == "pad_row_garbage"), None, order)


def bias_grad(dy, fault=None):
    return BR.colsum_f32(dy[:-1] if fault == "bias_drops_last_row" else dy).to(BF)


def glue_chain(x, w, dy, order=0, fault=None):
    """{dx, dw, db} bf16 of y = x w^T + b under the upstream gradient dy — LinearFn; PatchEmbedFn with x the gathered columns (dw's pad
    columns come out exactly zero); InjectFn with x the ControlNet state (its fourth result, the residual's gradient, is dy itself)."""
    return dict(dx=linear_dx(dy, w, order), dw=linear_dw(dy, x, order, fault), db=bias_grad(dy, fault))


def loss_chain(pred, target, weight, g=1.0):
    """(loss, dpred bf16) of MseLossFn: the kernel's gradient, times the upstream scalar in fp32 and rounded again unless it is 1."""
    loss, dpred = BR.mse_f32(pred, target, weight)
    if g != 1.0:
        dpred = (dpred.float() * torch.tensor(g, dtype=torch.float32)).to(BF)
    return loss * g, dpred


def attn_fwd_f32(q, k, v, heads, scale, order=0):
    """(o bf16 [Sq, D], lse2 fp32 [Sq, heads]): the flash forward — scores and the softmax in fp32 in the log2 domain, P rounded once to
    bf16 for P V, the row sum from the unrounded P.  order 0: every key at once against the row's maximum; order 1: the online form, key
    tiles of 64 against the RUNNING maximum with the accumulators rescaled in fp32 (P is then rounded at another scale: the same
    function, another draw of its rounding)."""
    qh, kh, vh = (AB._heads(t.float(), heads) for t in (q, k, v))
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(AB.LOG2E, dtype=torch.float32)
    s = (qh @ kh.transpose(1, 2)) * c
    tile = s.shape[-1] if order == 0 else 64
    m = torch.full_like(s[..., :1], -math.inf)
    den = torch.zeros_like(m)
    acc = torch.zeros_like(qh)
    for j in range(0, s.shape[-1], tile):
        sj = s[..., j:j + tile]
        m_new = torch.maximum(m, sj.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(sj - m_new)
        den = den * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + p.to(BF).float() @ vh[:, j:j + tile]
        m = m_new
    lse = (m + torch.log2(den)).squeeze(-1).transpose(0, 1).contiguous()
    return AB._flat(acc / den).to(BF), lse


def _add(a, b):
    return (a.float() + b.float()).to(BF)


def _gated(a, gate):
    return BR.gated_ref(a, gate)


def _lin(xin, sd, pre, order):
    return _gemm(xin, sd[pre + ".weight"], sd[pre + ".bias"], order)


def block_fwd(cfg, sd, x, ctx, t_mod, grid, order=0, prescale=True):
    """The block's forward, un-fused, with every intermediate the backward reads (DIT:214-230; DiTBlockFn.backward's recompute)."""
    heads = cfg["num_heads"]
    hd = cfg["dim"] // heads
    cos, sin, _ = rope_tables(hd, grid)
    s = types.SimpleNamespace(cfg=cfg, sd=sd, x=x, ctx=ctx, heads=heads, hd=hd, cos=cos, sin=sin, order=order, prescale=prescale)
    s.mod = FR.modulation_ref(sd["modulation"][0], t_mod[0], 0b010010)
    mod = s.mod
    if prescale:
        c = torch.tensor(q_prescale(), dtype=torch.float32)
        s.qcos, s.qsin, s.sa_scale = cos * c, sin * c, math.log(2.0)
    else:
        s.qcos, s.qsin, s.sa_scale = cos, sin, 1.0 / math.sqrt(hd)
    s.h1 = FR.layernorm_f32(x, scale1p=mod[1], shift=mod[0], eps=EPS)
    s.qp, s.kp, s.v = (_lin(s.h1, sd, "self_attn." + n, order) for n in "qkv")
    s.qn = FR.rmsnorm_rope_f32(s.qp, sd["self_attn.norm_q.weight"], s.qcos, s.qsin, hd, EPS)
    s.kn = FR.rmsnorm_rope_f32(s.kp, sd["self_attn.norm_k.weight"], cos, sin, hd, EPS)
    s.a, s.lse = attn_fwd_f32(s.qn, s.kn, s.v, heads, s.sa_scale, order)
    s.o = _lin(s.a, sd, "self_attn.o", order)
    s.x1 = _add(x, _gated(s.o, mod[2]))
    s.h2 = FR.layernorm_f32(s.x1, weight=sd["norm3.weight"], bias=sd["norm3.bias"], eps=EPS)
    s.q2p, s.k2p, s.v2 = _lin(s.h2, sd, "cross_attn.q", order), _lin(ctx, sd, "cross_attn.k", order), _lin(ctx, sd, "cross_attn.v", order)
    s.q2n = FR.rmsnorm_rope_f32(s.q2p, sd["cross_attn.norm_q.weight"], None, None, hd, EPS)
    s.k2n = FR.rmsnorm_rope_f32(s.k2p, sd["cross_attn.norm_k.weight"], None, None, hd, EPS)
    s.ca_scale = 1.0 / math.sqrt(hd)
    s.a2, s.lse2 = attn_fwd_f32(s.q2n, s.k2n, s.v2, heads, s.ca_scale, order)
    s.x2b = _gemm(s.a2, sd["cross_attn.o.weight"], sd["cross_attn.o.bias"], order, GR.EPI_RESID, s.x1)
    s.h3 = FR.layernorm_f32(s.x2b, scale1p=mod[4], shift=mod[3], eps=EPS)
    s.u = _lin(s.h3, sd, "ffn.0", order)
    s.f = FR.act_f32(s.u, "gelu_tanh")
    s.y = _lin(s.f, sd, "ffn.2", order)
    s.out = _add(s.x2b, _gated(s.y, mod[5]))
    return s


def block_bwd(s, dout, fault=None):
    """(dx bf16, {name: gradient bf16}) of the tape, walked backwards over block_fwd's intermediates; `fault`: one wrong line."""
    assert fault is None or fault in BLOCK_FAULTS, fault
    sd, mod, order, hd, heads = s.sd, s.mod, s.order, s.hd, s.heads
    g = {}

    def lin_bwd(dy, xin, pre, want_dx=True):
        g[pre + ".weight"] = linear_dw(dy, xin, order, fault)
        g[pre + ".bias"] = bias_grad(dy, fault)
        return linear_dx(dy, sd[pre + ".weight"], order) if want_dx else None

    # ---- FFN branch: out = x2b + gate_mlp y
    dgate2 = BR.colsum_f32(dout, s.o if fault == "dgate2_from_o" else s.y)
    dy = _gated(dout, mod[5])
    df = lin_bwd(dy, s.f, "ffn.2")
    du = BR.act_bwd_f32(s.u, df, "gelu_tanh")
    dh3 = lin_bwd(du, s.h3, "ffn.0")
    if fault == "ffn0_dw_from_f":
        g["ffn.0.weight"] = linear_dw(du, s.f[:, :s.h3.shape[1]].contiguous(), order)
    dln, dscale2, dshift2 = BR.layernorm_bwd_f32(s.x2b, dh3, g=mod[4], eps=EPS)
    d_x2b = dln if fault == "dx2b_no_residual" else _add(dout, dln)
    # ---- cross-attention branch: x2b = x1 + o2
    da2 = lin_bwd(d_x2b, s.a2, "cross_attn.o")
    dq2n, dk2n, dv2 = AB.chain_f32(s.q2n, s.k2n, s.v2, s.a2, da2, s.lse2, heads, s.ca_scale)
    dq2p, wq = BR.rmsnorm_rope_bwd_f32(s.q2p, dq2n, sd["cross_attn.norm_q.weight"], None, None, hd, EPS)
    dh2 = lin_bwd(dq2p, s.h2, "cross_attn.q")
    dk2p, wk = BR.rmsnorm_rope_bwd_f32(s.k2p, dk2n, sd["cross_attn.norm_k.weight"], None, None, hd, EPS)
    kv_in = s.x[:s.ctx.shape[0]].contiguous() if fault == "cross_kv_from_x" else s.ctx
    lin_bwd(dk2p, kv_in, "cross_attn.k", want_dx=False)
    lin_bwd(dv2, kv_in, "cross_attn.v", want_dx=False)
    g["cross_attn.norm_q.weight"], g["cross_attn.norm_k.weight"] = wq.to(BF), wk.to(BF)
    dln, n3w, n3b = BR.layernorm_bwd_f32(s.x1, dh2, g=sd["norm3.weight"], eps=EPS)
    if fault == "norm3w_from_x1":
        n3w = BR.colsum_f32(dh2, s.x1)
    g["norm3.weight"], g["norm3.bias"] = n3w.to(BF), n3b.to(BF)
    d_x1 = _add(d_x2b, dln)
    # ---- self-attention branch: x1 = x + gate_msa o
    dgate1 = BR.colsum_f32(d_x1, s.o)
    do = _gated(d_x1, mod[2])
    da = lin_bwd(do, s.a, "self_attn.o")
    dqn, dkn, dvv = AB.chain_f32(s.qn, s.kn, s.v, s.a, da, s.lse, heads, s.sa_scale)
    qc, qs = (s.cos, s.sin) if fault == "q_bwd_plain_table" else (s.qcos, s.qsin)
    dqp, wq = BR.rmsnorm_rope_bwd_f32(s.qp, dqn, sd["self_attn.norm_q.weight"], qc, qs, hd, EPS)
    dkp, wk = BR.rmsnorm_rope_bwd_f32(s.kp, dkn, sd["self_attn.norm_k.weight"], s.cos, s.sin, hd, EPS)
    g["self_attn.norm_q.weight"], g["self_attn.norm_k.weight"] = wq.to(BF), wk.to(BF)
    dh1 = lin_bwd(dqp, s.h1, "self_attn.q")
    dk_x = lin_bwd(dkp, s.h1, "self_attn.k")
    if fault != "dh1_no_k":
        dh1 = _add(dh1, dk_x)
    dv_x = lin_bwd(dvv, s.h1, "self_attn.v")
    if fault != "dh1_no_v":
        dh1 = _add(dh1, dv_x)
    dln, dscale1, dshift1 = BR.layernorm_bwd_f32(s.x, dh1, g=mod[1], eps=EPS)
    if fault == "mod1_from_dh3":
        _, dscale1, dshift1 = BR.layernorm_bwd_f32(s.x, dh3, g=mod[1], eps=EPS)
    dx = _add(d_x1, dln)
    rows = [dshift1, dscale1, dgate1, dshift2, dscale2, dgate2]         # the forward's order: shift, scale, gate (d(1 + s) = ds)
    if fault == "mod_rows_swapped":
        rows = [dscale1, dshift1, dgate1, dscale2, dshift2, dgate2]
    g["modulation"] = torch.stack(rows).to(BF).view(sd["modulation"].shape)
    return dx, g


def block_chain(cfg, sd, x, ctx, t_mod, dout, grid, order=0, prescale=True, fault=None):
    return block_bwd(block_fwd(cfg, sd, x, ctx, t_mod, grid, order, prescale), dout, fault)


# ---------------------------------------------------------------------------------------------------------------------
# the whole tape
def im2col(lat):
    """[c, F, H, W] -> [F (H/2) (W/2), 4 c]: the patches in the Conv3d weight's column order (c, ky, kx)."""
    c, F, H, W = lat.shape
    return lat.reshape(c, F, H // 2, 2, W // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(F * (H // 2) * (W // 2), 4 * c).contiguous()


def unpatchify_bwd_ref(dout, c, f, h, w):
    """dtokens [f h w, 4 c] of oracle.wan_oracle.unpatchify under dout [c, f, 2 h, 2 w], by fp64 autograd."""
    with torch.enable_grad():
        tok = torch.zeros((1, f * h * w, 4 * c), dtype=torch.float64, requires_grad=True)
        wo.unpatchify(tok, (f, h, w), c).backward(dout.double()[None])
    return tok.grad[0]


def _sub_sd(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


FWD_FAULTS = ("inject_prev_state", "inject_before_block", "last_cn_not_injected", "cat_y_latents", "head_shift_scale_swapped")


def model_fwd(cfg, dit_sd, cn_sd, n_cn, latents, y, control, context, timestep, order=0, block=None, fault=None):
    """The forward of model_fn (GF:1349-1591) on the pieces above, shared by model_chain (the training tape) and tests/inference_refs.py
    (the inference forward): time / text embedding, the patch GEMM on cat([latents, y]), the ControlNet patch embedding, ControlNet
    block i before DiT block i, the injection GEMM with its residual epilogue, the head, unpatchify.  `block(sd, x, ctx, t_mod, grid,
    stack, i)` -> an object with `.out` (default: block_fwd; stack "cn" | "dit").  -> a namespace: `taps[i]` the residual stream after
    DiT block i BEFORE the injection, `x` the stream the head reads, `tok` the head's output [S, 4 out_dim], `pred` [out_dim, f, 2h, 2w].
    `fault`: one of FWD_FAULTS (a wrong line of the forward)."""
    assert fault is None or fault in FWD_FAULTS, fault
    if block is None:
        block = lambda sd, x, ctx, t_mod, grid, stack, i: block_fwd(cfg, sd, x, ctx, t_mod, grid, order)          # noqa: E731
    d, eps = cfg["dim"], cfg["eps"]
    m = types.SimpleNamespace()
    m.t, m.t_mod = wo.time_embed(timestep, dit_sd, cfg["freq_dim"], d)               # bf16 linears: fp32 sums rounded once
    m.ctx = wo.text_embed(context, dit_sd)[0]
    parts = [latents] if y is None else ([y, latents] if fault == "cat_y_latents" else [latents, y])
    m.cols = im2col(torch.cat(parts, dim=1)[0])
    x = _gemm(m.cols, dit_sd["patch_embedding.weight"].reshape(d, -1), dit_sd["patch_embedding.bias"], order)
    f_, h_, w_ = latents.shape[2], latents.shape[3] // 2, latents.shape[4] // 2
    m.grid = grid = (f_, h_, w_)
    c = None
    if n_cn:
        pe = "controlnet_patch_embedding.patch_embedding."
        m.ccols = im2col(control[0])
        c = _gemm(m.ccols, cn_sd[pe + "weight"].reshape(d, -1), cn_sd[pe + "bias"], order)
    m.cn_fwd, m.dit_fwd, m.states, m.taps = [], [], [], []

    def inject(i, x):
        j = max(i - 1, 0) if fault == "inject_prev_state" else i
        zw = cn_sd[f"controlnet_zero_convs_after.{i}.weight"]
        return _gemm(m.states[j], zw.reshape(d, d), cn_sd[f"controlnet_zero_convs_after.{i}.bias"], order, GR.EPI_RESID, x)

    injected = n_cn - 1 if fault == "last_cn_not_injected" else n_cn
    for i in range(cfg["num_layers"]):
        if i < n_cn:
            m.cn_fwd.append(block(_sub_sd(cn_sd, f"controlnet_dit.blocks.{i}."), c, m.ctx, m.t_mod, grid, "cn", i))
            c = m.cn_fwd[-1].out
            m.states.append(c)
            if fault == "inject_before_block" and i < injected:
                x = inject(i, x)
        m.dit_fwd.append(block(_sub_sd(dit_sd, f"blocks.{i}."), x, m.ctx, m.t_mod, grid, "dit", i))
        x = m.dit_fwd[-1].out
        m.taps.append(x)
        if i < injected and fault != "inject_before_block":
            x = inject(i, x)
    m.x = x
    m.hmod = FR.modulation_ref(dit_sd["head.modulation"][0], m.t, 0b10)
    shift, scale1p = (m.hmod[1], m.hmod[0]) if fault == "head_shift_scale_swapped" else (m.hmod[0], m.hmod[1])
    hx = FR.layernorm_f32(x, scale1p=scale1p, shift=shift, eps=eps)
    m.tok = _gemm(hx, dit_sd["head.head.weight"], dit_sd["head.head.bias"], order)
    co = cfg["out_dim"]
    m.pred = m.tok.reshape(f_, h_, w_, 2, 2, co).permute(5, 0, 1, 3, 2, 4).reshape(co, f_, 2 * h_, 2 * w_)
    return m


def model_chain(cfg, dit_sd, cn_sd, n_cn, inputs, timestep_id, order=0, fault=None):
    """(loss, {ControlNet parameter: gradient bf16}) of training_loss + backward (model_fn_train, GF:1349-1591 with the tape)."""
    assert fault is None or fault in MODEL_FAULTS, fault
    d, eps = cfg["dim"], cfg["eps"]
    sigmas, timesteps, weights = to.training_schedule()
    timestep = timesteps[timestep_id:timestep_id + 1].to(BF)
    tid = int(torch.argmin((timesteps - timestep.float()).abs()))
    sigma = sigmas[tid]
    x0, noise = inputs["input_latents"], inputs["noise"]
    latents = (1 - sigma) * x0 + sigma * noise                                     # bf16 eager arithmetic, as the scheduler's
    target = noise - x0
    m = model_fwd(cfg, dit_sd, cn_sd, n_cn, latents, inputs["y"], inputs["control"], inputs["context"], timestep, order)
    f_, h_, w_ = m.grid
    x, hmod, states, cn_fwd, dit_fwd, ccols, pred, co = m.x, m.hmod, m.states, m.cn_fwd, m.dit_fwd, m.ccols, m.pred, cfg["out_dim"]
    pe = "controlnet_patch_embedding.patch_embedding."
    loss, dpred = loss_chain(pred.contiguous(), target[0].contiguous(), float(weights[tid]))
    # ---- backward
    grads = {}
    dtok = dpred.reshape(co, f_, h_, 2, w_, 2).permute(1, 2, 4, 3, 5, 0).reshape(f_ * h_ * w_, 4 * co).contiguous()
    dhx = linear_dx(dtok, dit_sd["head.head.weight"], order)
    dx = BR.layernorm_bwd_f32(x, dhx, g=hmod[1], eps=eps)[0]
    dstates = [None] * n_cn
    for i in reversed(range(cfg["num_layers"])):
        if i < n_cn:
            zn = f"controlnet_zero_convs_after.{i}."
            gl = glue_chain(states[i], cn_sd[zn + "weight"].reshape(d, d), dx, order)
            dstates[i] = gl["dx"]
            grads[zn + "weight"], grads[zn + "bias"] = gl["dw"].reshape(cn_sd[zn + "weight"].shape), gl["db"]
            if fault == "inject_dstate_for_dout":                          # the residual stream is handed dstate where dout belongs
                dx = gl["dx"]
        dx = block_bwd(dit_fwd[i], dx)[0]
    gc = None                                                              # g1: what the next ControlNet block returns for its input
    for i in reversed(range(n_cn)):
        if gc is None:
            gs = dstates[i]
        else:
            gs = gc if fault == "fanout_g1_only" else _add(gc, dstates[i])
        gc, gb = block_bwd(cn_fwd[i], gs)
        grads.update({f"controlnet_dit.blocks.{i}.{k}": v for k, v in gb.items()})
    gl = glue_chain(ccols, cn_sd[pe + "weight"].reshape(d, -1), gc, order)
    grads[pe + "weight"], grads[pe + "bias"] = gl["dw"].reshape(cn_sd[pe + "weight"].shape), gl["db"]
    return loss, grads


# ---------------------------------------------------------------------------------------------------------------------
# the row statistic
ATTN_WEIGHTS = ("self_attn.v.weight", "self_attn.o.weight", "cross_attn.k.weight", "cross_attn.v.weight", "cross_attn.o.weight")


def group(name, model=False):
    if name == "dx":
        return "dx"
    if name.endswith("modulation"):
        return "modulation"
    if name.endswith(ATTN_WEIGHTS):
        return "attn_weight"
    return "weight" if (name.endswith(".weight") and "norm" not in name) else "vector"


def _as2d(name, t):
    t = t.double()
    if name == "dx":
        return t.reshape(t.shape[0], -1), ("row",)
    if name.endswith("modulation"):
        return t.reshape(6, -1), ("row",)
    if t.dim() >= 2:
        return t.reshape(t.shape[0], -1), ("row", "col")
    return t.reshape(1, -1), ("all",)


def row_stat(name, got, chain0, ref, axes=None):
    """dict(worst, where, zero_bad, noise): the worst ratio over the tensor's slices and which slice; the number of slices whose
    reference is identically zero but `got` is not; the chain's median dev_rms over the rows (fault `row_eps` is built from it).
    `axes` (tests/inference_refs.py): the slices of a 2-D tensor, ("row",), ("col",) or both, instead of what the name says."""
    assert got.shape == ref.shape == chain0.shape, (name, got.shape, chain0.shape, ref.shape)
    g, named_axes = _as2d(name, got)
    axes = named_axes if axes is None else axes
    c, r = _as2d(name, chain0)[0], _as2d(name, ref)[0]
    worst, where, zero_bad, noise = 0.0, None, 0, 0.0
    for ax in axes:
        dim = 0 if ax == "col" else 1
        dg, dc = (g - r).pow(2).mean(dim).sqrt(), (c - r).pow(2).mean(dim).sqrt()
        zero = (r == 0).all(dim)
        zb = zero & ~((g == 0).all(dim))                                   # NaN != 0: a NaN in a zero slice is caught here
        zero_bad += int(zb.sum())
        live = ~zero
        if not bool(live.any()):
            continue
        floor = 0.25 * float(dc[live].median())
        den = dc.clamp_min(floor)
        ratio = torch.where(den > 0, dg / den, torch.where(dg > 0, torch.full_like(dg, math.inf), torch.zeros_like(dg)))
        ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
        ratio = torch.where(live, ratio, torch.zeros_like(ratio))
        i = int(ratio.argmax())
        if float(ratio[i]) > worst or where is None:
            worst, where = float(ratio[i]), f"{ax} {i}"
        if ax != "col":
            noise = float(dc[live].median())
    return dict(worst=worst, where=where, zero_bad=zero_bad, noise=noise)


def measure(got, chain0, ref, model=False):
    """{name: row_stat} over every tensor of `got` (dicts of the same keys; `got` may hold a subset)."""
    return {n: row_stat(n, got[n].reshape(ref[n].shape), chain0[n].reshape(ref[n].shape), ref[n]) for n in got}


def worst_by_group(stats, model=False):
    out = {}
    for n, s in stats.items():
        k = group(n, model)
        out[k] = max(out.get(k, 0.0), s["worst"])
    return out


def failures(stats, model=False, bars=None):
    """The failure messages of a measure() result against ROW_BAR: tensor, slice, ratio and the bar; and the non-zero zero slices."""
    bars = ROW_BAR if bars is None else bars
    out = []
    for n, s in stats.items():
        bar = bars[group(n, model)]
        if not s["worst"] <= bar:
            out.append(f"{n}: {s['where']} is {s['worst']:.3f} x the restatement's distance from fp64 (bar {bar:.3f}, group {group(n, model)})")
        if s["zero_bad"]:
            out.append(f"{n}: {s['zero_bad']} slice(s) whose reference is identically zero are not exactly zero")
    return out


def assert_rows(got, chain0, ref, what, model=False):
    stats = measure(got, chain0, ref, model)
    for k, v in sorted(worst_by_group(stats, model).items()):
        print(f"ROW {what} {k}: worst ratio {v:.3f} (restatement {ROW_WORST[k]:.3f}, bar {ROW_BAR[k]:.3f})")
    fails = failures(stats, model)
    assert not fails, f"{what}: " + "; ".join(fails)
    return stats


def with_dx(dx, grads):
    out = dict(grads)
    out["dx"] = dx
    return out


def row_eps(name, chain0, ref, bar):
    """The epsilon of fault `row_eps` for a 2-D gradient: 2 x bar x (the chain's median row dev_rms / the reference's median row rms)."""
    r = _as2d(name, ref)[0]
    noise = row_stat(name, chain0, chain0, ref)["noise"]
    return 2.0 * bar * noise / float(r.pow(2).mean(1).sqrt().median())


def apply_row_eps(t, eps):
    """Row rows/2 of a 2-D gradient scaled by 1 + eps (fp32 product, rounded once)."""
    out = t.clone()
    v = out.reshape(out.shape[0], -1)
    v[v.shape[0] // 2] = (v[v.shape[0] // 2].float() * (1.0 + eps)).to(t.dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the whole-tensor bars the suite had before (tests/test_training_gpu.py)
def old_bars(got, ref):
    """{name: (passes, rel-L2, bar)} under test_dit_block_backward_vs_oracle's thresholds: 2.5e-2 per parameter gradient, 8e-2 for
    attn.k.bias, 1.5e-2 for dx."""
    out = {}
    for n in got:
        e = BR.rel_l2(got[n].reshape(ref[n].shape), ref[n])
        bar = 1.5e-2 if n == "dx" else 8e-2 if n.endswith("attn.k.bias") else 2.5e-2
        out[n] = (e < bar, e, bar)
    return out


def old_bars_pass(got, ref):
    return all(v[0] for v in old_bars(got, ref).values())


# ---------------------------------------------------------------------------------------------------------------------
# the glue's cases and data classes (linear_dx / linear_dw / bias_grad, LinearFn, PatchEmbedFn, InjectFn)
LIN_M = (1, 63, 64, 65, 127, 129, 513)        # 513: dX's GEMM (M rows) and dW's (LIN_N rows, K = 576) both run on the 4-wave kernel
LIN_N, LIN_K = 576, 136                       # out_features (a multiple of 64, and >= every M: the selector class), in_features
LIN_CLASSES = ("integers", "selector", "gauss")
BIAS_ROWS, BIAS_COLS = (1, 63, 64, 65, 1031), (8, 64, 520)
PATCH_GRIDS = ((1, 1, 1), (3, 4, 6), (2, 5, 7))
PATCH_IN, PATCH_OUT = 36, 128                 # in_dim 36: k = 144, kpad = 192


def linear_inputs(cls, M, N=LIN_N, K=LIN_K, seed=0):
    """bf16 (x [M, K], w [N, K], dy [M, N]) of a data class:
    integers   entries in {-1, 0, 1}: every sum is an integer below 256, exactly representable, whatever the order;
    selector   dy's row m holds ONE value +-2^k (k in -2..2) at column n(m) = (7 m + 3) mod N (distinct for M <= N, 7 a unit), x and w
               random bf16 bit patterns: dW's row n(m) is +-2^k x[m] exactly and every other row is zero; dX's row m is +-2^k w[n(m)];
    gauss      x, dy ~ N(0, 1), w ~ N(0, 1) / sqrt(K).  Where dX or dW has fewer than gemm_refs.SMALL elements — gemm_refs' bar (a) asks for
               equal bits there, and ONE element within a few fp32 ulps of a rounding boundary is a right kernel's to differ on — the
               data are drawn again until the restatement gives the chain's bits in every summation order it can state, as
               gemm_refs.gauss_inputs does.  The selection looks at the chain and the restatement alone."""
    if cls == "gauss":
        for attempt in range(256):
            x, w, dy = _linear_draw(cls, M, N, K, seed + 101 * attempt)
            if _order_proof(x, w, dy):
                return x, w, dy
        raise RuntimeError(f"linear_inputs({M}, {N}, {K}): no draw is clear of the rounding boundaries")
    return _linear_draw(cls, M, N, K, seed)


def _order_proof(x, w, dy):
    mp = pad64(dy.shape[0])
    for a, wt in ((dy, w.t().contiguous()), (_tpad(dy, mp), _tpad(x, mp))):
        if a.shape[0] * wt.shape[0] >= GR.SMALL:
            continue
        want = FR.bits(FR.rb(a.double() @ wt.double().t()))
        for ktile in (8, 16, 32, 64):                  # (8 and 16 as well: an element that cancels to a small sum flips under SOME order)
            for order in (0, 1, 2, 3):
                if not torch.equal(FR.bits(GR.gemm_f32(a, wt, None, GR.EPI_BIAS, None, None, None, ktile, order)), want):
                    return False
    return True


def _linear_draw(cls, M, N, K, seed):
    g = torch.Generator().manual_seed(5000011 * seed + 7919 * M + 31 * N + K + LIN_CLASSES.index(cls))
    if cls == "integers":
        x, w, dy = (torch.randint(-1, 2, shp, generator=g).float() for shp in ((M, K), (N, K), (M, N)))
    elif cls == "selector":
        assert M <= N
        x, w = GR._band_bf16((M, K), g).float(), GR._band_bf16((N, K), g).float()
        dy = torch.zeros((M, N))
        sign = torch.randint(0, 2, (M,), generator=g).float() * 2 - 1
        dy[torch.arange(M), selector_col(M, N)] = sign * torch.exp2(torch.randint(-2, 3, (M,), generator=g).float())
    else:
        x, dy = torch.randn((M, K), generator=g), torch.randn((M, N), generator=g)
        w = torch.randn((N, K), generator=g) / math.sqrt(K)
    return x.to(BF), w.to(BF), dy.to(BF)


def selector_col(M, N):
    return (7 * torch.arange(M) + 3) % N


def linear_refs(x, w, dy):
    """(dx Ref, dw Ref, db fp64) against the fp64 products: gemm_refs' bars with K = N for dX and K = pad64(M) for dW."""
    (ax, sx), (aw, sw) = _prod(dy, w.t()), _prod(dy.t(), x.t())
    dx = GR.Ref(*GR.chain(ax, None, GR.EPI_BIAS, None, None, None, sx), None, None)
    dw = GR.Ref(*GR.chain(aw, None, GR.EPI_BIAS, None, None, None, sw), None, None)
    return dx, dw, dy.double().sum(0)


def _prod(a, wt):
    """(acc, S) of a [M, K] times wt^T given wt [N, K]; chain()'s first argument and its S keyword."""
    av, wv = a.double(), wt.double()
    return av @ wv.t(), av.abs() @ wv.abs().t()


def bias_grad_bound(dy):
    """(want, lo, hi) as fp64 holding bf16 values: want = bf16(fp64 column sum); the fp32 column sum is held to backward_refs' colsum bar
    (1e-5, here asked of every column against its sum of magnitudes: ~170 fp32 epsilons, an order above what 1031 additions in any
    order cost), and rounding is monotone, so a right bias gradient lies in [bf16(sum - 1e-5 sum|dy|), bf16(sum + 1e-5 sum|dy|)] — the
    one value `want`, or its neighbour where the exact sum sits that close to a rounding boundary."""
    s, sa = dy.double().sum(0), dy.double().abs().sum(0)
    want = FR.rb(s)
    slop = 1e-5 * sa                                    # the fp32 column sum's distance from the exact one
    lo, hi = FR.rb(s - slop), FR.rb(s + slop)           # rounding is monotone: the result lies between these two bf16 values
    return want, lo, hi

/*
 * goalforce.h — C ABI of libgoalforce_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary underneath the reference's Python call sites
 * (level B5).  The reference (brown-palm/goal-force) has no
 * FFI of its own: every entry point below replaces a *Python* interface, cited
 * as file:line relative to the reference tree.  Abbreviations:
 *   DIT  = diffsynth/models/wan_video_dit.py
 *   GF   = src/goal_force/wan_video_new.py
 *   FM   = diffsynth/schedulers/flow_match.py
 *   VAE  = diffsynth/models/wan_video_vae.py
 *   VRAM = diffsynth/vram_management/layers.py
 *   DS   = src/goal_force/unified_dataset.py
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless a parameter says "host".
 *   - bf16 tensors are passed as `const void*` / `void*` (raw 16-bit storage).
 *   - The caller owns all memory; the library never allocates or frees
 *     user-visible buffers and never synchronises: kernels are enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - Return value: 0 on success, negative gf_status on error; the message is
 *     available from gf_last_error() (thread-local).
 *   - Row-major everywhere; `ld*`/`*_stride` are in ELEMENTS.
 */
#ifndef GOALFORCE_H
#define GOALFORCE_H

#include <stdint.h>

#if defined(GF_BUILD)
#define GF_API __attribute__((visibility("default")))
#else
#define GF_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GF_OK = 0,
    GF_ERR_INVALID_ARG = -1,   /* bad shape / alignment / null pointer */
    GF_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels are built for */
    GF_ERR_LAUNCH = -3         /* hipLaunchKernel / hipFuncSetAttribute failed */
} gf_status;

/* library identity ------------------------------------------------------- */
GF_API const char* gf_version(void);      /* "goalforce-hip <semver> gfx950" */
GF_API const char* gf_last_error(void);   /* thread-local message of the last failure */
/* The C ABI revision: the ONE number bumped on any signature change, and on any change of what an entry point expects of a
 * caller-owned buffer under an unchanged signature.  gf_abi_version() returns it; the Python bindings read this line and refuse
 * a library built from another revision. */
#define GF_ABI_VERSION 20
GF_API int gf_abi_version(void);          /* GF_ABI_VERSION of the build */
/* Dispatch overrides.  Every kernel in the library ships, each for the shapes its launcher sends it; the parity tests cross-check
 * two kernels on the same operands, which needs a way to route a shape to the one that would not get it by default.  Names:
 * "prefer_8wave" (0/1), "a4_stagger" (>= 0), "a4_group_m" (0 = by K), "conv_nb" (0 = by Cout, 1, 2), "conv_gather" (0/1),
 * "conv_direct" (0/1), "vae_rms3" (0/1), "attn_fixed_max" (0/1, default 1; 0: gf_flash_attn_fwd_vt32_fm / _sparse_fm make the one exact
 * launch of the plain entry points — the A/B switch and the escape hatch of the fixed-maximum softmax).  Values are clamped to their range; an unknown name returns GF_ERR_INVALID_ARG.
 * The library reads NO environment variable: only these calls change the dispatch.  Process-wide, relaxed atomics. */
GF_API int gf_set_option(const char* name, int value);
GF_API int gf_get_option(const char* name, int* value);   /* the value in force (after clamping); a caller that overrides one reads it first to restore it */
GF_API void gf_reset_options(void);   /* back to the shipped dispatch */

/* ------------------------------------------------------------------------
 * gf_layernorm_modulate — LayerNorm over the last dim (fp32 math, one
 * rounding to bf16), optionally affine, optionally followed by the AdaLN
 * modulate y*(1+scale)+shift with the reference's bf16 rounding after each op.
 * Replaces: nn.LayerNorm norm1/norm2/norm3 + modulate() (DIT:64-65, 206-208,
 * 225-228), WanAutoCastLayerNorm.forward (VRAM:78-92), Head.norm (DIT:258,268).
 *   x, out     [rows, dim] bf16 (out may alias x)
 *   weight,bias[dim] bf16 or NULL  (norm3 affine)
 *   scale1p    [dim] bf16 or NULL  — the already-formed (1+scale) vector
 *   shift      [dim] bf16 or NULL
 * dim % 8 == 0, dim <= 8192.
 */
GF_API int gf_layernorm_modulate(const void* x, void* out, const void* weight, const void* bias,
                          const void* scale1p, const void* shift,
                          int64_t rows, int64_t dim, int64_t x_stride, int64_t out_stride,
                          float eps, void* stream);

/* ------------------------------------------------------------------------
 * gf_modulation — forms the AdaLN vectors of one block in bf16 exactly as the
 * reference's eager ops do: out[i,:] = bf16(param[i,:] + t[i % t_rows,:]) and,
 * for rows whose bit is set in onep_mask, out[i,:] = bf16(1 + out[i,:]).
 * Replaces `(self.modulation + t_mod).chunk(6)` and the `1 + scale` of
 * modulate() (DIT:64-65, 218-219) and Head's `(modulation + t).chunk(2)` (DIT:264-268).
 *   param [k, dim] bf16, t [t_rows, dim] bf16, out [k, dim] bf16; k <= 32.
 */
GF_API int gf_modulation(const void* param, const void* t, void* out, int64_t k, int64_t dim,
                         int64_t t_rows, uint32_t onep_mask, void* stream);

/* ------------------------------------------------------------------------
 * gf_rmsnorm_rope — in place: RMSNorm over the FULL row (all heads jointly;
 * fp32 math, round to bf16, then bf16 multiply by weight) followed by 3-D RoPE
 * on adjacent element pairs.  Replaces RMSNorm.forward (DIT:100-111) and
 * rope_apply (DIT:92-97) as used by SelfAttention.forward (DIT:141-145) and
 * CrossAttention.forward (DIT:177-178; cos/sin NULL => no RoPE).
 *   x       [rows, dim] bf16, row stride x_stride
 *   weight  [dim] bf16
 *   cos,sin [rows, head_dim/2] fp32 or NULL
 * dim % 8 == 0, dim <= 8192, head_dim % 8 == 0.
 */
GF_API int gf_rmsnorm_rope(void* x, const void* weight, const float* cos_tab, const float* sin_tab,
                    int64_t rows, int64_t dim, int64_t head_dim, int64_t x_stride,
                    float eps, void* stream);

/* ------------------------------------------------------------------------
 * gf_gemm_bf16 — C[M,N] = epilogue(A[M,K] · W[N,K]^T + bias[N]); bf16 in/out,
 * fp32 MFMA accumulate (v_mfma_f32_16x16x32_bf16).  Replaces nn.Linear /
 * F.linear at DIT:131-134,146 (q,k,v,o), DIT:209-210 (ffn), DIT:309-320
 * (text/time embeddings), DIT:263 (head), the Conv3d patch embeddings
 * (DIT:307-308,342; GF:85,92 — after gf_patchify_im2col) and the ControlNet
 * zero-conv Conv1d(k=1) (GF:113-116, 1565-1570).
 *   epilogue: see gf_epilogue.  resid [M,N] (ldr) and gate [N] are bf16.
 *   C may alias resid (in-place residual update).
 * K % 64 == 0, N % 8 == 0, lda/ldw/ldc/ldr % 8 == 0, 16-byte aligned bases.
 */
typedef enum {
    GF_EPI_BIAS = 0,           /* bf16(acc + bias)                               */
    GF_EPI_BIAS_GELU_TANH = 1, /* bf16(gelu_tanh(bf16(acc + bias)))              */
    GF_EPI_BIAS_GATE_RESID = 2,/* bf16(resid + bf16(gate * bf16(acc + bias)))    */
    GF_EPI_BIAS_RESID = 3,     /* bf16(resid + bf16(acc + bias))                 */
    GF_EPI_BIAS_SILU = 4,      /* bf16(silu(bf16(acc + bias)))                   */
    GF_EPI_BIAS_MUL = 5        /* bf16(bf16(acc + bias) * resid)  — GEGLU: fc1(x) * gelu(gate(x)),
                                  wan_video_text_encoder.py:106                  */
} gf_epilogue;
/* The activations of epilogues 1 and 4 are the plain fp32 formula v / (1 + exp(-z)): in the far negative tail (the bf16 values -97 <= v <= -89
 * for SiLU, -10.3125 <= v <= -10.0625 for GELU-tanh) 1 + exp(-z) overflows (z < -88.72) and they return -0 where bf16(function) is not yet zero (below
 * 3e-37, the last values denormal).  gf_act does not (see there); on every other finite bf16 value the two agree bit for bit. */

GF_API int gf_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias,
                 void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                 int epilogue, const void* resid, int64_t ldr, const void* gate,
                 void* stream);

/* gf_gemm_bf16_batched — `batch` independent products C_b = A_b W_b^T (no bias, no epilogue) in ONE launch: problem b reads
 * A + b*strideA ([M, K], row pitch lda), W + b*strideW ([N, K], row pitch ldw) and writes C + b*strideC ([M, N], row pitch ldc); strides in
 * elements, and a stride may be smaller than a matrix (heads side by side in one [L, H*d] tensor: strideA = d, lda = H*d).  The small
 * per-head / per-frame products of the umT5 encoder's attention (wan_video_text_encoder.py:61-93: q k^T and attn v per head) and of the
 * VAE AttentionBlock (VAE:304-342, per frame).  K a multiple of 64, N of 8.  Runs on the 8-wave kernel: bit-identical to `batch`
 * gf_gemm_bf16 calls on that kernel (M < 512, or gf_set_option("prefer_8wave", 1)); the 4-wave kernel gf_gemm_bf16 takes for M >= 512 rotates the K
 * loop's start per column tile, i.e. sums the same products in another order. */
GF_API int gf_gemm_bf16_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw, int64_t strideW, void* C,
                                int64_t ldc, int64_t strideC, int64_t M, int64_t N, int64_t K, int64_t batch, void* stream);

/* ------------------------------------------------------------------------
 * gf_flash_attn_fwd — softmax(Q K^T * scale) V per head, non-causal, no mask,
 * no dropout, head_dim 128.  Replaces flash_attention() (DIT:28-61) /
 * AttentionModule (DIT:114-121).  q,k,v,o are [len, heads*128] bf16 with the
 * head h at columns [h*128, (h+1)*128) ("b s (n d)" layout, DIT:56-60); row
 * strides in elements (so q/k/v may be slices of one fused buffer).
 */
GF_API int gf_flash_attn_fwd(const void* q, const void* k, const void* v, void* o,
                      int64_t q_len, int64_t kv_len, int64_t heads, int64_t head_dim,
                      int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride,
                      float scale, void* stream);

/* gf_transpose_v + gf_flash_attn_fwd_vt — the same attention with V handed over pre-transposed: vt [heads][128][kv_pad] bf16
 * (kv_pad a multiple of 64, keys >= kv_len zero, keys permuted 0-3,8-11,4-7,12-15 inside every group of 16 — written by
 * gf_transpose_v).  One LDS read per PV MFMA instead of two; what the self-attention of the DiT blocks uses.  lse may be NULL. */
GF_API int gf_transpose_v(const void* v, int64_t v_stride, void* vt, int64_t kv_len, int64_t kv_pad, int64_t heads, void* stream);
GF_API int gf_flash_attn_fwd_vt(const void* q, const void* k, const void* vt, void* o, float* lse,
                         int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t heads, int64_t head_dim,
                         int64_t q_stride, int64_t k_stride, int64_t o_stride, float scale, void* stream);

/* gf_transpose_v32 + gf_flash_attn_fwd_vt32 — the self-attention of the DiT blocks (round 2; kv_len >= 128): the same attention
 * (DIT:28-61) on v_mfma_f32_16x16x32_bf16, the MFMA shape the chip sustains a higher clock on under random data.  Same
 * arguments as the pair above; the two V^T copies differ in the key order inside a 64-key tile and are NOT interchangeable
 * (vt32: inside every group of 32 keys position 8 g + i holds key 4 g + i for i < 4, 16 + 4 g + i - 4 for i >= 4). */
GF_API int gf_transpose_v32(const void* v, int64_t v_stride, void* vt, int64_t kv_len, int64_t kv_pad, int64_t heads, void* stream);
GF_API int gf_flash_attn_fwd_vt32(const void* q, const void* k, const void* vt, void* o, float* lse,
                                  int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t heads, int64_t head_dim,
                                  int64_t q_stride, int64_t k_stride, int64_t o_stride, float scale, void* stream);

/* gf_flash_attn_fwd_vt32_sparse — gf_flash_attn_fwd_vt32 over a block map: the workgroup of query block b (256 rows) of head h
 * visits only the 64-key tiles listed for it, softmax and output are taken over those keys alone.  Operands and their checks
 * are gf_flash_attn_fwd_vt32's (V^T from gf_transpose_v32 / gf_linear_vt32 / gf_linear_vt32_fp8; lse may be NULL).  The map is
 * CSR in device memory, read-only during the launch:
 *   row_ptr  int32 [n_maps * n_qblocks + 1], n_qblocks = ceil(q_len / 256);
 *   tile_idx int32, the tiles of row r at [row_ptr[r], row_ptr[r + 1]);
 *   head_map int32 [heads] or NULL (every head uses map 0); head h reads row head_map[h] * n_qblocks + b.
 * Contract: inside a row the indices ascend, there are at least 2 of them (the two-tile pipeline is the validated one: the dense
 * entry's kv_len >= 128), each is < ceil(kv_len / 64), head_map[h] < n_maps.  The library cannot inspect device memory: it checks
 * the pointers and n_maps >= 1 only.  The kernel clamps every index it reads to the tiles that exist, so a map that breaks the
 * contract gives wrong numbers but no read outside k / vt — that clamp is the only protection against a bad map.
 * A row that lists every tile computes bit for bit what gf_flash_attn_fwd_vt32 does; any row computes bit for bit what
 * gf_flash_attn_fwd_vt32 does on the listed tiles' keys gathered in order.  Forward only (no backward takes a map). */
GF_API int gf_flash_attn_fwd_vt32_sparse(const void* q, const void* k, const void* vt, void* o, float* lse,
                                         const int32_t* row_ptr, const int32_t* tile_idx, const int32_t* head_map, int64_t n_maps,
                                         int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t heads, int64_t head_dim,
                                         int64_t q_stride, int64_t k_stride, int64_t o_stride, float scale, void* stream);

/* gf_flash_attn_fwd_vt32_fm / gf_flash_attn_fwd_vt32_sparse_fm — the two entry points above with the softmax maximum FIXED at the
 * first visited tile's row maximum m0 (dense: tile 0; sparse: the first list entry) instead of a running maximum: two launches on
 * `stream`.  The first computes p = bf16(exp2(s - m0)) for every later tile with no maximum, no rescale decision and no rescale of
 * O — fp32 and bf16 carry the full exponent range, and the row sum holds the exact term 1, so the result has the exact path's
 * accuracy unless a later score lies ~100 - 128 log2 units above m0 and a row sum or an O accumulator overflows.  Each wave tests
 * its accumulators for non-finite values and writes flags[(head * n_qblocks + b) * 8 + wave] = 0 / 1 (n_qblocks = ceil(q_len /
 * 256); every word is written on every call: no memset needed).  The second launch returns at once in every workgroup whose eight
 * flags are zero and recomputes the others' 256 rows with the running maximum (bit for bit what the plain entry point writes for
 * them), overwriting o and lse.  After the call flags tells which blocks were repaired.
 *   flags int32 [heads * n_qblocks * 8], caller-owned, 4-byte aligned, one per stream in flight.
 * Option "attn_fixed_max" = 0: one exact launch, flags zeroed. */
GF_API int gf_flash_attn_fwd_vt32_fm(const void* q, const void* k, const void* vt, void* o, float* lse, int32_t* flags,
                                     int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t heads, int64_t head_dim,
                                     int64_t q_stride, int64_t k_stride, int64_t o_stride, float scale, void* stream);
GF_API int gf_flash_attn_fwd_vt32_sparse_fm(const void* q, const void* k, const void* vt, void* o, float* lse, int32_t* flags,
                                            const int32_t* row_ptr, const int32_t* tile_idx, const int32_t* head_map, int64_t n_maps,
                                            int64_t q_len, int64_t kv_len, int64_t kv_pad, int64_t heads, int64_t head_dim,
                                            int64_t q_stride, int64_t k_stride, int64_t o_stride, float scale, void* stream);

/* gf_linear_vt32 — the V projection of SelfAttention.forward (`v = self.v(x)`, DIT:131-146) written DIRECTLY in the layout
 * gf_flash_attn_fwd_vt32 reads: vt[n * kv_pad + pos(s)] = bf16(sum_k x[s,k] * w[n,k] + bias[n]) for n < N, s < kv_len, positions
 * kv_len .. kv_pad-1 zero, pos() = the key order of gf_transpose_v32.  Bit-identical to gf_gemm_bf16(x, w, bias) followed by
 * gf_transpose_v32 (same MFMA kernel with the operands swapped, same summation order); saves the plain V tensor's round trip.
 *   x [kv_len, ldx] bf16, w [N, ldw] bf16 (nn.Linear layout), bias [N] bf16 or NULL, vt [N * kv_pad] bf16;
 *   kv_pad = kv_len rounded up to 64, N >= 512 and a multiple of 128, K a multiple of 64. */
GF_API int gf_linear_vt32(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* vt,
                          int64_t kv_len, int64_t kv_pad, int64_t N, int64_t K, void* stream);

/* gf_flash_attn_fwd_lastmult — gf_flash_attn_fwd in which the LAST key (row kv_len - 1 of k / v) counts `last_key_multiplicity`
 * times in the softmax: softmax over [k_0 .. k_{n-2}, k_{n-1} x m] evaluated on n keys (the key's score gets + log2 m in the exp2
 * domain).  Cross-attention over a prompt whose padded tail is a run of identical context rows (wan_prompter.py:99-109 zeroes the
 * text-encoder output past the prompt: every padded row is text_embedding(0), so its K and V rows are identical, DIT:177-186) is
 * the same function of q evaluated on the distinct keys only.  Key lengths below the V^T threshold only (the 512-token context). */
GF_API int gf_flash_attn_fwd_lastmult(const void* q, const void* k, const void* v, void* o, int64_t q_len, int64_t kv_len,
                                      int64_t heads, int64_t head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                      int64_t o_stride, float scale, float last_key_multiplicity, void* stream);

/* gf_cross_probs — the normalised softmax probabilities of a cross-attention over n_keys < 64 keys, instead of its output:
 * p[s, h*n_pad + j] = bf16(w_hj), w_hj = softmax_j(scale * q_h . k_hj), the last key (row n_keys - 1) counting `last_key_multiplicity`
 * times as in gf_flash_attn_fwd_lastmult, the same fp32 score arithmetic.  Column n_keys holds the last key's rounding residue
 * bf16(w - bf16(w)) (its partner is column n_keys of the table, a copy of column n_keys - 1); columns n_keys < j < n_pad (n_pad > n_keys,
 * a multiple of 16, <= 64) are written as zeros.  With U from gf_cross_fold_table the attention output times W_o^T is ONE GEMM p @ U^T (K = heads * n_pad):
 * the cross-attention's output projection folded into the cached values.  q [q_len, heads*128], k [n_keys, heads*128] row-strided,
 * 16-byte aligned; p [q_len, p_stride >= heads*n_pad] bf16, 8-byte aligned, p_stride a multiple of 4. */
GF_API int gf_cross_probs(const void* q, const void* k, void* p, int64_t q_len, int64_t n_keys, int64_t n_pad, int64_t heads,
                          int64_t head_dim, int64_t q_stride, int64_t k_stride, int64_t p_stride, float scale,
                          float last_key_multiplicity, void* stream);

/* gf_cross_fold_table — the value table of gf_cross_probs: u[n, h*n_pad + j] = bf16(sum_d v[j, h*128 + d] * w_o[n, h*128 + d]) for
 * n < n_out and j < n_keys (fp32 accumulation, one rounding), column n_keys = column n_keys - 1, zeros for n_keys < j < n_pad.  v [n_keys, heads*128], w_o [n_out, heads*128] (the
 * o projection's weight) row-strided, 16-byte aligned; u [n_out, u_stride >= heads*n_pad] bf16 — the [N, K] weight layout of
 * gf_gemm_bf16. */
GF_API int gf_cross_fold_table(const void* v, const void* w_o, void* u, int64_t n_keys, int64_t n_pad, int64_t heads, int64_t head_dim,
                               int64_t n_out, int64_t v_stride, int64_t w_stride, int64_t u_stride, void* stream);

/* ------------------------------------------------------------------------
 * Training (ControlNet training step): training_loss (GF:180-193) calls loss.backward() through
 * F.scaled_dot_product_attention (DIT:28-61) in every block.
 * gf_flash_attn_fwd_lse — gf_flash_attn_fwd that also returns lse [q_len, heads] fp32, the log2-domain log-sum-exp
 *   of the scaled scores: softmax row = exp2(scale*log2(e)*S - lse).
 * gf_flash_attn_bwd — dq, dk, dv from (q, k, v, o, dout, lse).  Same layouts / strides as the forward; fp32 accumulation,
 *   bf16 results.  `workspace` is caller-owned, 16-byte aligned, gf_flash_attn_bwd_workspace_bytes(q_len, kv_len, heads) bytes:
 *   rowsum(dout*o) [q_len, heads] fp32 and the dK/dV kernel's per-granule (-lse | -delta) records (a -DGF_BWD_QSCALE=1 build adds
 *   a pre-scaled copy of q: always size the buffer with the function); scratch, its contents need not survive the call.  The
 *   log-sum-exp must come from gf_flash_attn_fwd_lse (or gf_flash_attn_fwd_vt32 / _vt with a non-NULL lse) with the same `scale`.
 *   dk and dv may be NULL together: only dq is computed (a frozen block's cross-attention: nobody reads the context gradients).
 */
GF_API int gf_flash_attn_fwd_lse(const void* q, const void* k, const void* v, void* o, float* lse,
                          int64_t q_len, int64_t kv_len, int64_t heads, int64_t head_dim,
                          int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride,
                          float scale, void* stream);
GF_API int64_t gf_flash_attn_bwd_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads);
GF_API int gf_flash_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                      const float* lse, void* workspace, void* dq, void* dk, void* dv,
                      int64_t q_len, int64_t kv_len, int64_t heads, int64_t head_dim,
                      int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t do_stride,
                      int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, float scale, void* stream);

/* Backward of the row / elementwise ops of a block and the loss / optimiser of the training step (gf_backward.hip).
 * Gradients: fp32 math on the bf16 forward operands, one rounding to bf16.  *_acc are caller-zeroed fp32 [dim] column
 * accumulators (parameter gradients summed over the token rows; NULL = not wanted).
 * gf_layernorm_bwd   — LayerNorm (DIT:206-208, VRAM:78-92) with y = xhat*g (+b): g = affine weight or (1+scale) or NULL;
 *                      dx; dg_acc += dy*xhat, db_acc += dy.
 * gf_rmsnorm_rope_bwd — RMSNorm (DIT:100-111) (+ RoPE DIT:92-97): x is the PRE-norm tensor; dx; dw_acc.
 * gf_colsum          — acc[n] += sum_r a[r,n]*(b ? b[r,n] : 1); optionally out[r,n] = bf16(a[r,n]*gate[n]) (bias gradients;
 *                      the gated residual out = resid + gate*y: a = dout, b = y gives dgate and dy in one pass).
 * gf_act_bwd         — du = df * act'(u), kind 0 = GELU-tanh (DIT:209), 1 = SiLU.
 * gf_mse_loss        — loss[0] = weight * mean((pred-target)^2), dpred = weight*2(pred-target)/n  (GF:190-191).
 * gf_adamw_step      — torch.optim.AdamW update of a bf16 parameter with fp32 moments (utils.py:755); grad_scale
 *                      multiplies the gradient first (gradient clipping).
 * gf_f32_to_bf16     — rounds an accumulator buffer to the bf16 gradient.                                             */
GF_API int gf_layernorm_bwd(const void* x, int64_t x_stride, const void* dy, int64_t dy_stride, const void* g, void* dx,
                            int64_t dx_stride, float* dg_acc, float* db_acc, int64_t rows, int64_t dim, float eps, void* stream);
GF_API int gf_rmsnorm_rope_bwd(const void* x, int64_t x_stride, const void* dy, int64_t dy_stride, const void* weight,
                               const float* cos_tab, const float* sin_tab, void* dx, int64_t dx_stride, float* dw_acc,
                               int64_t rows, int64_t dim, int64_t head_dim, float eps, void* stream);
GF_API int gf_colsum(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gate, void* out, int64_t ldo,
                     float* acc, int64_t rows, int64_t cols, void* stream);
GF_API int gf_act_bwd(const void* u, const void* df, void* du, int64_t n, int kind, void* stream);
GF_API int gf_mse_loss(const void* pred, const void* target, void* dpred, float* loss, int64_t n, float weight, void* stream);
GF_API int gf_adamw_step(void* param, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream);
GF_API int gf_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* gf_sumsq — acc[0] += sum of squares of a bf16 buffer (fp32): the global gradient norm of clip_grad_norm_ (utils.py:806-808). */
GF_API int gf_sumsq(const void* x, int64_t n, float* acc, void* stream);

/* ------------------------------------------------------------------------
 * Mass-cover block maps (gf_block_map.hip; the reference has no counterpart): the CSR map of gf_flash_attn_fwd_vt32_sparse built
 * on the device from that call's own q and k, per head, with no host read.  Operands as there: q [q_len][ldq], k [kv_len][ldk]
 * bf16, heads * 128 columns used (head_dim 128), row strides multiples of 8 elements, 16-byte aligned; n_qb = ceil(q_len / 256),
 * n_t = ceil(kv_len / 64); kv_len >= 128 and n_t <= 1024 (else GF_ERR_INVALID_ARG, by name).  The recipe (this project's own, in the
 * line of SpargeAttn / XAttention / MInference):
 *   1. pooling   qm[h][b][:] = fp32 mean of the rows of query block b that exist (a ragged last block divides by its own count);
 *                km[h][t][:] = the same over the keys of tile t.  Sum order: a lane's rows 16 apart ascending, then a fixed tree.
 *   1b. coherence (gf_block_means_coh, the gated entries only) of the same runs, from the same loads: rho = |m|^2 / e with m the
 *                pooled mean above (the same sum order, the same bits as gf_block_means) and e = (sum_i |x_i|^2) / count, fp32.
 *                0 <= rho <= 1 (Cauchy-Schwarz), rho = 1 iff the run's rows are equal, 1 - rho = the mean squared deviation from
 *                the mean relative to the rows' energy — what makes <q_i, km> differ from <qm, km>.  e == 0 (all rows zero, hence
 *                equal) gives rho = 1.  Sum order of e: per lane the chain e = fma(x, x, e) over the row's 8 channels, rows 16 apart
 *                ascending; the 16 channel-group lanes by xor 1, 2, 4, 8; then the means' tree (row groups xor 1, 2; waves 0 .. 3);
 *                / count.  |m|^2: lane l forms fma(m[l + 64], m[l + 64], m[l] * m[l]), then xor 1, 2, .. 32.  No atomics.
 *                Non-finite input gives NaN; so does FINITE input whose squares overflow fp32 (|x| beyond ~1e19) — conservative:
 *                NaN counts as incoherent below.
 *   2. scores    s[h][b][t] = fma(c, dot, log2(n_keys(t))), dot = fma chain over d = 0 .. 127, c = fp32(double(scale) * log2(e))
 *                (the package's pre-scaled q with scale = ln 2 gives c = 1); n_keys(t) = 64, or the ragged last tile's count.
 *                By Jensen's inequality n_keys 2^dot-term is a LOWER bound of the tile's true unnormalised mass seen from the pooled
 *                query — for the block's actual rows it is an ESTIMATE, not a guarantee.
 *   3. selection per row (h, b): M = max_t s, w_t = exp2(s_t - M), W = sum_t w_t; `forced` (uint32 [n_qb][ceil(n_t / 32)], bit t % 32
 *                of word t / 32, shared by all heads, NULL = none; bits >= n_t ignored) names tiles that are always kept, F = their
 *                mass.  theta* = the largest value among the w_t with F + sum{w_u : u not forced, w_u >= theta*} >= mass * W; selected =
 *                forced U {u : w_u >= theta*}; forced only when F >= mass * W.  A threshold on the value: ties are taken together.
 *                Fewer than 2 selected: the largest unselected w is added (lowest index on ties) until there are 2.  mass >= 1
 *                selects every tile.  A row with ANY non-finite score selects every tile — so every emitted row is valid (>= 2
 *                ascending indices < n_t) for any input bits.  All sums are fp32 in one fixed order.
 *                The gate (gf_block_map_select_gated): a row (h, b) with !(q_coh[h][b] >= q_min) selects every tile, as a row with a
 *                non-finite score does (kept = 1); a tile t with !(k_coh[h][t] >= k_min) is forced for every row of head h — OR-ed
 *                with `forced`, counted in F, under the same rules (forced only when F >= mass * W, the two-tile floor).  Written
 *                `!(rho >= min)` so that a NaN coherence fires.  q_coh fp32 [heads][n_qb], k_coh fp32 [heads][n_t]; NULL switches
 *                that side off, both NULL are the bits of gf_block_map_select.  q_min, k_min in (0, 1] (else refused by name).
 *   4. emit      row_ptr int32 [heads * n_qb + 1] (row_ptr[0] = 0, a scan of the counts on the device), tile_idx int32 ascending
 *                inside a row, caller-owned with capacity heads * n_qb * n_t (the worst case), head_map int32 [heads] = 0 .. heads-1;
 *                the sparse kernel takes them with n_maps = heads.
 * Optional outputs (NULL to skip): scores fp32 [heads][n_qb][n_t]; kept fp32 [heads * n_qb], the ESTIMATED kept share
 * sum_selected w / W (1 for a row that selects everything).  The true retained mass of a run is 2^(lse_sparse - lse_dense).
 * No atomics: two calls on the same operands write the same bits; gf_block_map_from_qk writes the bits of the staged calls
 * (gf_block_means x 2, gf_block_map_scores, gf_block_map_select), which it runs on `stream` in that order.
 *   ws of gf_block_map_from_qk: gf_block_map_workspace_bytes bytes, 256-byte aligned (qm, km, scores, the selection's scratch);
 *   ws of gf_block_map_select: gf_block_map_select_workspace_bytes bytes (counts and selection bitmasks).  One per stream in flight.
 * The gated entries (coherence, step 1b, and the gate of step 3) change none of the above: the ungated entries write the bits they
 * wrote before.  gf_block_map_from_qk_gated runs gf_block_means_coh x 2 (in place of the pooling pass: q and k are still read once
 * each), gf_block_map_scores, gf_block_map_select_gated on `stream`, checks every argument before the first launch and writes the
 * bits of those staged calls; q_coh_out fp32 [heads][n_qb] / k_coh_out fp32 [heads][n_t] receive the coherences (NULL to skip);
 * q_min <= 0 / k_min <= 0 switches that side of the gate off there (NaN and values above 1 are refused); ws:
 * gf_block_map_gated_workspace_bytes bytes, 256-byte aligned; gf_block_map_select_gated takes gf_block_map_select's workspace.
 * What the gate GUARANTEES.  Assume every ungated query block has equal rows and every unforced key tile has equal keys.  Then for a
 * row of an ungated block the pooled query IS the row, the estimate n 2^dot-term is exact on the unforced tiles and a lower bound
 * (Jensen) on the forced ones.  With S the exact mass of the selected unforced tiles, U that of the unselected tiles, F_true >= F_est
 * the true and the estimated mass of the forced tiles, the retained share is (F_true + S) / (F_true + S + U) >= (F_est + S) /
 * (F_est + S + U) >= mass, because x / (x + U) increases in x; gated rows retain 1.  So thresholds near 1 predict only for constant
 * blocks and the promise holds; no gate uses the pooled estimate everywhere; in between the true retained mass is MEASURED
 * (2^(lse_sparse - lse_dense)), not promised. */
GF_API int64_t gf_block_map_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads);     /* 0: a shape the entry refuses */
GF_API int64_t gf_block_map_select_workspace_bytes(int64_t n_qblocks, int64_t n_tiles, int64_t heads);
/* mean fp32 [heads][ceil(rows / block)][128]; block = 256 (query blocks) or 64 (key tiles) */
GF_API int gf_block_means(const void* x, int64_t ldx, float* mean, int64_t rows, int64_t heads, int64_t block, void* stream);
GF_API int gf_block_map_scores(const float* q_mean, const float* k_mean, float* scores, int64_t q_len, int64_t kv_len, int64_t heads,
                               float scale, void* stream);
GF_API int gf_block_map_select(const float* scores, const uint32_t* forced, int32_t* row_ptr, int32_t* tile_idx, int32_t* head_map,
                               float* kept, void* ws, int64_t n_qblocks, int64_t n_tiles, int64_t heads, float mass, void* stream);
GF_API int gf_block_map_from_qk(const void* q, int64_t ldq, const void* k, int64_t ldk, const uint32_t* forced, int32_t* row_ptr,
                                int32_t* tile_idx, int32_t* head_map, float* scores, float* kept, void* ws, int64_t q_len,
                                int64_t kv_len, int64_t heads, float scale, float mass, void* stream);
GF_API int64_t gf_block_map_gated_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads);       /* 0: a shape the entry refuses */
/* gf_block_means plus coh fp32 [heads][ceil(rows / block)]; refuses what gf_block_means refuses, and a null coh */
GF_API int gf_block_means_coh(const void* x, int64_t ldx, float* mean, float* coh, int64_t rows, int64_t heads, int64_t block,
                              void* stream);
GF_API int gf_block_map_select_gated(const float* scores, const uint32_t* forced, const float* q_coh, const float* k_coh,
                                     int32_t* row_ptr, int32_t* tile_idx, int32_t* head_map, float* kept, void* ws, int64_t n_qblocks,
                                     int64_t n_tiles, int64_t heads, float mass, float q_min, float k_min, void* stream);
GF_API int gf_block_map_from_qk_gated(const void* q, int64_t ldq, const void* k, int64_t ldk, const uint32_t* forced, int32_t* row_ptr,
                                      int32_t* tile_idx, int32_t* head_map, float* scores, float* kept, float* q_coh_out,
                                      float* k_coh_out, void* ws, int64_t q_len, int64_t kv_len, int64_t heads, float scale, float mass,
                                      float q_min, float k_min, void* stream);

/* ------------------------------------------------------------------------
 * gf_patchify_im2col — gathers the (1,2,2) patches of an NCTHW latent into a
 * token-major matrix for the patch-embedding GEMM.  Replaces the data movement
 * of WanModel.patchify (DIT:341-349) / ControlNet_PatchEmbedding.forward
 * (GF:85-94) for the concatenated input x = cat([latents, y]) (GF:1458).
 *   src0 [c0,F,H,W], src1 [c1,F,H,W] (src1 may be NULL with c1 = 0), bf16
 *   out  [F*(H/2)*(W/2), kpad] bf16, column = c*4 + dy*2 + dx (Conv3d weight
 *   order), columns >= (c0+c1)*4 zero-filled.
 */
GF_API int gf_patchify_im2col(const void* src0, int64_t c0, const void* src1, int64_t c1,
                       void* out, int64_t F, int64_t H, int64_t W, int64_t kpad, void* stream);

/* ------------------------------------------------------------------------
 * gf_unpatchify — 'b (f h w) (x y z c) -> b c (f x) (h y) (w z)' with patch
 * (1,2,2).  Replaces WanModel.unpatchify (DIT:351-356).
 *   tokens [f*h*w, 4*c] bf16  ->  out [c, f, 2h, 2w] bf16
 */
GF_API int gf_unpatchify(const void* tokens, void* out, int64_t c, int64_t f, int64_t h, int64_t w,
                  void* stream);

/* ------------------------------------------------------------------------
 * gf_cfg_euler_step — classifier-free guidance + flow-match Euler update in
 * one pass, with the reference's bf16 rounding after every op:
 *   pred = nega + cfg*(posi - nega)            (GF:716)
 *   latents = latents + pred * dsigma          (FM:72-82; dsigma = sigma_next - sigma)
 * nega may be NULL (cfg_scale == 1: pred = posi, GF:717-718).  In place on latents.
 */
GF_API int gf_cfg_euler_step(void* latents, const void* posi, const void* nega,
                      float cfg_scale, float dsigma, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * gf_act — elementwise activation bf16 -> bf16 (fp32 math, one rounding):
 * kind 0 = SiLU (DIT:316,320), 1 = GELU-tanh (DIT:311).
 * Every finite input is within one bf16 value of bf16(the function in fp64), the far negative tail included (where
 * x / (1 + exp(-z)) alone overflows to -0: SiLU below -88.7, GELU-tanh below -10.06); -inf gives NaN, as torch's does.
 */
GF_API int gf_act(const void* x, void* out, int64_t n, int kind, void* stream);

/* ------------------------------------------------------------------------
 * gf_add_bf16 — out = bf16(a + b), elementwise (x + controlnet_state,
 * GF:1570).  out may alias a.
 */
GF_API int gf_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * TeaCache (GF:1243-1292): the two kernels of the step-skipping cache; its
 * update on a skipped step is gf_add_bf16.
 * gf_sub_bf16    — out = bf16(a - b), the fp32 difference rounded once
 *                  (the residual x_after_blocks - x_patchified, GF:1287).
 *                  out may alias a or b.
 * gf_rel_l1_bf16 — sums[0] = sum_i |bf16(cur_i - prev_i)|, sums[1] = sum_i |prev_i|,
 *                  fp32 accumulation, for the relative L1 distance of two
 *                  timestep modulations (GF:1272).  One launch of one block,
 *                  every addition in an order fixed by the code (no atomics):
 *                  the same bits on every call.  n > 0, n % 8 == 0 (n = 6*dim);
 *                  sums is fp32[2] on the device, overwritten.
 */
GF_API int gf_sub_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);
GF_API int gf_rel_l1_bf16(const void* cur, const void* prev, int64_t n, void* sums, void* stream);

/* ------------------------------------------------------------------------
 * gf_force_map — renders the Goal-Force control-signal video on the GPU.
 * Replaces the pixel work of ControlSignalDataset_Balls._generate_control_video
 * / get_gaussian_blob / get_blob_for_mass (DS:775-940): every blob contributes
 * amp * exp(-((x-cx)^2 + (y-cy)^2) / denom) to its channel (fp32, summed in blob
 * order, optional clamp to [0,1] as DS:887, one rounding to bf16).
 *   out      [frames, H, W, 3] bf16 (THWC, DS:842)
 *   channels [n_blobs] int32      0 direct force, 1 goal force, 2 mass
 *   params   [n_blobs, 2] fp32    {denom = 2*radius^2, amp}
 *   centers  [n_blobs, frames, 2] fp32  {cx, cy} per frame (host computes them
 *            in float64 exactly as DS:817-823 and rounds once to fp32)
 */
GF_API int gf_force_map(void* out, int64_t frames, int64_t H, int64_t W,
                 const int32_t* channels, const float* params, const float* centers,
                 int64_t n_blobs, int clamp01, void* stream);

/* ========================================================================
 * Wan 3-D causal VAE decoder (VAE = diffsynth/models/wan_video_vae.py).
 * Decoder activations are channels-last [T, H, W, C] bf16; every convolution is
 * gf_vae_im2col (patch gather, temporal halo from the 2-frame feature cache)
 * followed by gf_gemm_bf16 on the weight pre-permuted to [Cout, (dt,dy,dx,cin)].
 * ======================================================================== */

/* gf_vae_prep_latent — un-normalise a latent tile and make it channels-last:
 * out[t,y,x,c] = bf16(bf16(z[c,t,y,x] / inv_std[c]) + mean[c]), c >= C zero-filled.
 * Replaces VideoVAE_.decode's scale step (VAE:1014-1020); z is addressed with
 * element strides (sc,st,sy,sx) so a tile slice needs no copy (VAE:1125).     */
GF_API int gf_vae_prep_latent(const void* z, int64_t sc, int64_t st, int64_t sy, int64_t sx,
                              const void* mean, const void* inv_std, void* out,
                              int64_t C, int64_t T, int64_t H, int64_t W, int64_t cpad, void* stream);

/* gf_vae_im2col — patch gather for CausalConv3d (VAE:33-52; kt in {1,3}, ks in {1,3},
 * causal temporal padding kt-1 taken from `cache` [2,H,W,C] = the reference's
 * feat_cache entry, all-zero when there is no history).  Output frame j is the conv at
 * input frame t_off + j*t_stride (t_stride 2 = the encoder's strided time_conv, VAE:107-112, 160-170).
 *   mode 0: zero spatial padding ks/2, stride 1;
 *   mode 1: Upsample(nearest-exact 2x) folded into a 3x3 conv (decoder Resample, VAE:91-99);
 *   mode 2: ZeroPad2d((0,1,0,1)) + 3x3 conv stride 2 (encoder Resample, VAE:101-106).
 * src [T,H,W,C] -> out [T_out*Ho*Wo, kpad], column ((dt*ks+dy)*ks+dx)*C+c. */
GF_API int gf_vae_im2col(const void* src, const void* cache, void* out, int64_t T_out, int64_t H, int64_t W,
                         int64_t C, int64_t kt, int64_t ks, int mode, int64_t t_stride, int64_t t_off,
                         int64_t kpad, void* stream);

/* gf_conv3d_bf16 — the same convolution as ONE implicit GEMM: gf_vae_im2col's patch matrix is never written; the GEMM's
 * LDS-DMA fetches every 16-byte piece (8 channels of one tap of one output pixel) straight from src / cache (padding taps
 * and the K padding columns from a zero page).  Replaces CausalConv3d.forward (VAE:33-52) and the convs inside Resample
 * (VAE:82-174) end to end; arguments as gf_vae_im2col (T_in = frames in src) + gf_gemm_bf16 (Wm [N, ldw] with columns
 * ((dt*ks+dy)*ks+dx)*C+c, zero from kt*ks*ks*C up to K; K a multiple of 64; epilogue GF_EPI_BIAS or GF_EPI_BIAS_RESID).
 * out [T_out*Ho*Wo, ldc].  Bit-identical to gf_vae_im2col + gf_gemm_bf16.
 * kt == 3 with cache == NULL: the two history frames lie directly IN FRONT of src (src points two frames into one
 * [2 + T_in, H, W, C] buffer) — with mode 0 this selects the pointer-per-row gather (one 64-bit pointer + 4 border flags per
 * output pixel, one offset per tap), 20 % faster than the general one. */
GF_API int gf_conv3d_bf16(const void* src, const void* cache, const void* Wm, int64_t ldw, const void* bias,
                          void* out, int64_t ldc, int64_t T_in, int64_t T_out, int64_t H, int64_t W, int64_t C,
                          int kt, int ks, int mode, int t_stride, int t_off, int64_t N, int64_t K, int epilogue,
                          const void* resid, int64_t ldr, void* stream);

/* gf_vae_finish_latent — encoder tail: out[r,c] = bf16(bf16(x[r,c] - mean[c]) * inv_std[c]) for the first C
 * (mu) channels of the 1x1x1 conv1 output (VideoVAE_.encode, VAE:1002-1010). */
GF_API int gf_vae_finish_latent(const void* x, int64_t ldx, const void* mean, const void* inv_std, void* out,
                                int64_t rows, int64_t C, void* stream);

/* gf_vae_rmsnorm_silu — RMS_norm over channels (F.normalize * sqrt(C) * gamma, bf16
 * rounding after each eager op, VAE:55-70) optionally followed by SiLU
 * (ResidualBlock VAE:277-281, Decoder3d.head VAE:785).  x,out [rows, C], C <= 512.  */
GF_API int gf_vae_rmsnorm_silu(const void* x, const void* gamma, void* out, int64_t rows, int64_t C,
                               int silu, void* stream);

/* gf_softmax_rows — out[r,:ncols] = softmax(bf16(x[r,:]*scale + bias[r,:])) over the first nvalid columns
 * (columns >= nvalid: probability 0, = masked_fill(finfo.min)), out[r,ncols:ldo] = 0; bias may be NULL.
 * The single-head SDPA of the VAE AttentionBlock (VAE:326-333) and the umT5 attention with its relative
 * position bias and key mask (wan_video_text_encoder.py:72-84), between their two GEMMs.                  */
GF_API int gf_softmax_rows(const void* x, int64_t ldx, const void* bias, int64_t ldb, void* out, int64_t ldo,
                           int64_t rows, int64_t ncols, int64_t nvalid, float scale, void* stream);

/* gf_rowmax_neg_bf16 — out[r * ldo] = bf16(-max_c x[r, c]) (exact: a maximum of bf16 values).  The per-row offset of the
 * AttentionBlock's score GEMM (VAE:326-333): written into an extra K column of the Q operand whose counterpart in the K operand
 * is 1, it makes the GEMM accumulate q.k - rowmax in fp32, so that the bf16 rounding of the scores is small where the softmax
 * weight is large (F.scaled_dot_product_attention, which the reference calls, keeps its scores in fp32).  x [rows, ncols] bf16 (ldx). */
GF_API int gf_rowmax_neg_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int64_t ncols, void* stream);

/* gf_transpose_pad — dst[c, r] = src[r, c], r >= R zero-filled up to rpad (V^T operand
 * of the AttentionBlock's P·V GEMM).                                                   */
GF_API int gf_transpose_pad(const void* src, int64_t ld_src, void* dst, int64_t R, int64_t C, int64_t rpad,
                            void* stream);

/* gf_transpose_pad_batched — `batch` transposes in one launch: matrix b = src + b*stride_src ([R, C], row pitch ld_src; heads lying side by
 * side in one [R, H*C] tensor have stride_src = C) -> dst + b*stride_dst ([C, rpad], zero columns past R); strides in elements. */
GF_API int gf_transpose_pad_batched(const void* src, int64_t ld_src, int64_t stride_src, void* dst, int64_t stride_dst, int64_t R,
                                    int64_t C, int64_t rpad, int64_t batch, void* stream);

/* gf_vae_tile_blend / gf_vae_tile_finalize — WanVideoVAE.tiled_decode's weighted tile
 * accumulation (VAE:1128-1150, build_mask VAE:1081-1100) with bf16 accumulators:
 *   values[c,t,y0+y,x0+x] += tile[t,y,x,c]*mask(y,x); weight[y0+y,x0+x] += mask(y,x)
 * then values = clamp(values/weight, -1, 1).  tile is channels-last [T,th,tw,tc>=nch] (nch = 3 RGB / 16 latent);
 * top/bottom/left/right = the tile touches that frame border (no ramp on that side).   */
GF_API int gf_vae_tile_blend(void* values, void* weight, const void* tile, int64_t nch, int64_t T, int64_t th,
                             int64_t tw, int64_t tc, int64_t H, int64_t W, int64_t y0, int64_t x0,
                             int top, int bottom, int left, int right, int64_t border_h, int64_t border_w,
                             void* stream);
/* clamp1 != 0: clamp to [-1,1] (decode); 0: no clamp (tiled_encode, VAE:1155-1203). */
GF_API int gf_vae_tile_finalize(void* values, const void* weight, int64_t planes, int64_t hw, int clamp1, void* stream);

/* gf_window_blend / gf_window_finalize — TemporalTiler_BCTHW.run's weighted accumulation of one temporal window (GF:1336-1343,
 * build_1d_mask GF:1300-1310) with bf16 accumulators: the sibling in time of gf_vae_tile_blend / gf_vae_tile_finalize.
 *   value  [C, T, HW] bf16, HW contiguous, value_stride_c / value_stride_t in elements (a slice of a larger tensor is fine as long
 *          as its planes do not overlap); weight [T] bf16.  Both are accumulators, zeroed by the caller before the first window.
 *   win    [C, len, HW] bf16 contiguous: the window's prediction as gf_unpatchify leaves it; it covers frames t0 .. t0+len-1.
 * The mask of window frame i, built in this order (the right ramp is written last and wins where both apply, len < 2*border):
 *   m = 1
 *   if (!left_bound  && i < border)        m = bf16(fp32(i + 0.5) / fp32(border))
 *   if (!right_bound && i >= len - border) m = bf16(fp32(len - 1 - i + 0.5) / fp32(border))
 * (the fp32 division correctly rounded; border = 0: all ones), and the update, the reference's two bf16 roundings of
 * `value += out * mask`:
 *   value[c, t0+i, p] = bf16(fp32(value[c, t0+i, p]) + fp32(bf16(fp32(win[c, i, p]) * fp32(m))))
 *   weight[t0+i]      = bf16(fp32(weight[t0+i]) + fp32(m))
 * Windows of one accumulator are blended on one stream in ascending t0: bf16 accumulation depends on the order.
 * Refused (outputs untouched): null pointers, C / T / HW / len <= 0, strides that let planes overlap, t0 < 0, t0 + len > T,
 * border < 0, and border >= len when a ramp is requested (!left_bound || !right_bound, border > 0). */
GF_API int gf_window_blend(void* value, void* weight, const void* win, int64_t C, int64_t T, int64_t HW, int64_t value_stride_c,
                           int64_t value_stride_t, int64_t t0, int64_t len, int left_bound, int right_bound, int64_t border,
                           void* stream);
/* value[c, t, p] = bf16(fp32(value[c, t, p]) / fp32(weight[t])), no clamp (GF:1343); a frame no window covered divides by zero
 * as the reference does. */
GF_API int gf_window_finalize(void* value, const void* weight, int64_t C, int64_t T, int64_t HW, int64_t value_stride_c,
                              int64_t value_stride_t, void* stream);

/* gf_modulate — the reference's module-level `modulate(x, shift, scale)` (DIT:64-65) in its eager bf16 rounding sequence:
 * out = bf16(bf16(x * bf16(1 + scale)) + shift); scale / shift [dim] bf16; x, out [rows, dim] bf16.  (On the hot path the
 * modulation is fused into gf_layernorm_modulate; this entry point backs the B3 drop-in name.) */
GF_API int gf_modulate(const void* x, void* out, const void* scale, const void* shift, int64_t rows, int64_t dim,
                       int64_t x_stride, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------------
 * LoRA adapters (gf_lora.hip).  Replaces GeneralLoRALoader.load (diffsynth/lora/__init__.py; GF:171-174) and peft's unmerged
 * forward.  Both sum the rank in fp32 — chunks of 32 rank columns in ascending order, one v_mfma_f32_16x16x32_bf16 per chunk and
 * output element (four per wave: its four accumulator fragments), the rank zero-padded to a multiple of 32 inside the kernel — and
 * round to bf16 only after the last product.  A shape of more than 2^31 tiles of 64 x 64 is refused.
 *
 * gf_lora_merge — in place, W [n_out, ldw] bf16:
 *     W[n,k] <- bf16( W[n,k] + bf16( alpha * bf16( sum_j up[n,j] * down[j,k] ) ) )
 * the reference's three bf16 roundings (torch.mm, the scalar multiply by fp32(alpha), the add).  up [n_out, ld_up], down
 * [rank, ld_down] bf16 with any row pitch that covers the row; 1 <= rank <= 256; alpha finite (0 still runs the chain).
 * k_in % 8 == 0, ldw % 8 == 0, W 16-byte aligned.  Every refusal leaves W untouched.
 *
 * gf_lora_up — one attached adapter on a layer's output y0 = bf16(acc + bias) [M, ldy], t = bf16(x down^T) [M, ldt]:
 *     out[m,n] = epi( bf16( y0[m,n] + bf16( scale * bf16( sum_j t[m,j] * up[n,j] ) ) ), resid, gate )
 * with epi = gf_epilogue as gf_gemm_bf16 applies it to bf16(acc + bias).  up [N, ld_up] with columns true rank .. rank_pad - 1 zero;
 * rank_pad a multiple of 32, <= 256; N % 8 == 0; every leading dimension a multiple of 8; 16-byte aligned bases.  out may alias
 * y0 or resid.  resid / ldr / gate as gf_gemm_bf16. */
GF_API int gf_lora_merge(void* W, int64_t ldw, const void* up, int64_t ld_up, const void* down, int64_t ld_down, int64_t n_out,
                         int64_t k_in, int64_t rank, float alpha, void* stream);
GF_API int gf_lora_up(const void* y0, int64_t ldy, const void* t, int64_t ldt, const void* up, int64_t ld_up, void* out, int64_t ldo,
                      int64_t M, int64_t N, int64_t rank_pad, float scale, int epilogue, const void* resid, int64_t ldr,
                      const void* gate, void* stream);

/* gf_lora_grad (gf_lora_grad.hip) — a trainable adapter's parameter gradients, the sum over the tokens:
 *     out[c, j] = bf16( fp32(scale) * sum_{m < M} Y[m, c] * T[m, j] )        c < C, j < rank_pad;  transposed = 1: stored at out[j, c]
 * dUp [n_out, r] = gf_lora_grad(dy, t = bf16(x down^T), scale); dDown [r, k_in] = gf_lora_grad(x, dt = bf16(dy up), scale, transposed).
 * Y [M, ldy] and T [M, ldt] bf16, read row-major as they are (no transposed copy is written); out bf16 [C, ldo] or, transposed,
 * [rank_pad, ldo].  fp32 accumulation on v_mfma_f32_16x16x32_bf16, nothing rounded before the last token, scale applied to the fp32
 * sum, ONE bf16 rounding per element: at scale 1 (the reference's lora_alpha = r) torch's bf16 autograd chain, at any other scale
 * one rounding tighter than it.  A zero sum is stored as +0 for every scale, so columns of T that are zero (the rank's padding) give
 * +0, and M = 0 writes +0 everywhere.
 * The tokens are split into gf_lora_grad_slabs(M, C, rank_pad) slabs — slab s is rows s * gf_lora_grad_slab_rows(...) up to the
 * next slab's first row or M — each summed in ascending tiles of 64 tokens into an fp32 partial in `workspace`
 * (gf_lora_grad_workspace_bytes bytes, 16-byte aligned, caller-owned, one per stream in flight; may be null when that is 0); a
 * second kernel adds the partials in ascending slab order.  No atomics: two calls on the same operands give the same bits.  All
 * three are pure functions of (M, C, rank_pad) and return 0 for a shape gf_lora_grad refuses (and for M = 0).
 * M >= 0; C % 8 == 0; rank_pad a multiple of 32, <= 256; every leading dimension a multiple of 8 that covers its row; 16-byte
 * aligned bases; scale finite.  Every refusal leaves out untouched. */
GF_API int64_t gf_lora_grad_slabs(int64_t M, int64_t C, int64_t rank_pad);
GF_API int64_t gf_lora_grad_slab_rows(int64_t M, int64_t C, int64_t rank_pad);
GF_API int64_t gf_lora_grad_workspace_bytes(int64_t M, int64_t C, int64_t rank_pad);
GF_API int gf_lora_grad(const void* Y, int64_t ldy, const void* T, int64_t ldt, void* out, int64_t ldo, int64_t M, int64_t C,
                        int64_t rank_pad, float scale, int transposed, void* workspace, void* stream);

/* ---- Canny-edge control signal (ControlSignalDataset_CannyEdge._generate_control_video, src/goal_force/unified_dataset.py:559-578;
 * the reference calls cv2 / controlnet_aux per frame on the host — absent here: OpenCV's published algorithm restated, "parity unpinned").
 * All images are uint8 [frames, H, W, 3] (HWC), all tables device arrays built by goal_force_amd/canny.py.
 * gf_resize_lanczos4_u8 — cv2.resize(INTER_LANCZOS4) on 8-bit pixels: xofs/yofs = floor source coordinate per destination column / row,
 *   xcoef/ycoef [n][8] = the 8 tap weights in 11-bit fixed point; replicated border; one rounding shift by 22. */
GF_API int gf_resize_lanczos4_u8(const void* src, void* dst, const int* xofs, const short* xcoef, const int* yofs, const short* ycoef,
                                 int64_t frames, int64_t H, int64_t W, int64_t Hd, int64_t Wd, void* stream);
/* gf_resize_area_u8 — cv2.resize(INTER_AREA), shrinking by a non-integer ratio: CSR tables (start [n+1], source index, fp32 weight) per
 *   axis.  mode 0: uint8 [frames,H,W,3] -> uint8 [frames,Hd,Wd,3].  mode 1: src is gf_canny_u8's state map [frames,H,W] (2 = edge -> 255,
 *   else 0) and dst the dataset's control video: bf16 [frames,Hd,Wd,3], three equal channels of x / 127.5 - 1. */
GF_API int gf_resize_area_u8(const void* src, void* dst, const int* xstart, const int* xsrc, const float* xalpha, const int* ystart,
                             const int* ysrc, const float* yalpha, int64_t frames, int64_t H, int64_t W, int64_t Hd, int64_t Wd, int mode,
                             void* stream);
/* gf_canny_u8 — cv2.Canny(img, low, high), aperture 3, L1 gradient, on uint8 [frames,H,W,3]: Sobel (replicated border), strongest
 *   channel per pixel, non-maximum suppression, double threshold, hysteresis to the fixpoint -> state uint8 [frames,H,W]
 *   (2 = edge).  mag_ws / dxy_ws: int32 [frames*H*W] scratch each; changed: one device int.  Synchronises the stream once per
 *   hysteresis pass (a dataset loader, not the sampling loop); fails if max_passes are not enough. */
GF_API int gf_canny_u8(const void* img, void* state, void* mag_ws, void* dxy_ws, int* changed, int64_t frames, int64_t H, int64_t W,
                       int low, int high, int max_passes, void* stream);

/* gf_gate_residual — `GateModule.forward(x, gate, residual)` (DIT:189-194): out = bf16(x + bf16(gate * residual)), gate [dim]
 * bf16 (batch 1), x / residual / out [rows, dim] bf16 with row strides.  (Hot path: the GEMM epilogue GF_EPI_BIAS_GATE_RESID.) */
GF_API int gf_gate_residual(const void* x, const void* gate, const void* residual, void* out, int64_t rows, int64_t dim,
                            int64_t x_stride, int64_t r_stride, int64_t out_stride, void* stream);

/* gf_rope_apply — the reference's module-level `rope_apply(x, freqs, num_heads)` (DIT:92-97) alone: adjacent pairs of every
 * head rotated by cos / sin [rows, head_dim/2] fp32.  (Hot path: fused into gf_rmsnorm_rope.) */
GF_API int gf_rope_apply(const void* x, void* out, const float* cos_tab, const float* sin_tab, int64_t rows, int64_t dim,
                         int64_t head_dim, int64_t x_stride, int64_t out_stride, void* stream);

/* ========================================================================
 * fp8 Linear — the contract of AutoWrappedLinear.fp8_linear (VRAM:115-151):
 *   scale_a = clamp(rowmax|x| / 448, min=1);  x8 = e4m3(x / (scale_a + 1e-8));  W8 = e4m3(W) (unit scale)
 *   out = bf16((x8 · W8^T) * scale_a + bias)          [torch._scaled_mm, out_dtype bf16]
 * e4m3 is OCP e4m3fn (gfx950 native; the reference halves fp8_max only for MI300's fnuz).
 * ======================================================================== */

/* gf_quant_fp8_rowscale — per-row dynamic activation quantisation (VRAM:124-137).
 * x [rows, dim] bf16 -> out8 [rows, dim] e4m3 bytes, scale [rows] fp32; dim % 8 == 0, dim <= 14336. */
GF_API int gf_quant_fp8_rowscale(const void* x, void* out8, float* scale, int64_t rows, int64_t dim,
                                 int64_t x_stride, int64_t out_stride, void* stream);

/* gf_layernorm_modulate_fp8 — gf_layernorm_modulate whose consumer is an fp8 Linear: the normalised (+affine, +modulate) bf16
 * row stays in registers, its row maximum gives scale_a and only the e4m3 bytes + scale are written — bit-identical to
 * gf_layernorm_modulate followed by gf_quant_fp8_rowscale (DIT:206-208, 225-228 feeding VRAM:124-137).
 * dim must be one of the wave-per-row widths 5120 / 4096 / 1536; other widths: call the two functions. */
GF_API int gf_layernorm_modulate_fp8(const void* x, void* out8, float* scale, const void* weight, const void* bias,
                                     const void* scale1p, const void* shift, int64_t rows, int64_t dim,
                                     int64_t x_stride, int64_t out_stride, float eps, void* stream);

/* gf_linear_vt32_fp8 — gf_linear_vt32 on the fp8_linear contract: the V projection of a self-attention under config 5 written
 * directly as attention kernel 3's V^T operand.  x8 [kv_len, K] / w8 [N, K] e4m3 bytes, x_scale [kv_len] fp32 (the tokens'
 * activation scales); bit-identical to gf_gemm_fp8 + gf_transpose_v32.  N >= 512, N % 128 == 0, K % 128 == 0. */
GF_API int gf_linear_vt32_fp8(const void* x8, int64_t ldx, const float* x_scale, const void* w8, int64_t ldw, const void* bias,
                              void* vt, int64_t kv_len, int64_t kv_pad, int64_t N, int64_t K, void* stream);

/* gf_cast_fp8 — bf16 -> e4m3 elementwise (weight.to(float8_e4m3fn), VRAM:138); n % 8 == 0.  torch's codes on every input: round to
 * nearest even, |x| <= 464 -> at most 448, |x| > 464, +-inf and NaN -> the NaN code (sign | 0x7F): no saturation. */
GF_API int gf_cast_fp8(const void* x, void* out8, int64_t n, void* stream);

/* Training through FROZEN fp8 layers (training.set_fp8_frozen; no weight gradient): dX = dY · W8 on gf_gemm_fp8, from the two below.
 *
 * gf_quant_fp8_grad — the per-row quantiser of a GRADIENT, with a power-of-two scale (gf_quant_fp8_rowscale's clamp(min=1) would turn a
 * row of magnitude 1e-5 into zeros).  x [rows, dim] bf16 (rows may be strided) -> out8 [rows, dim] e4m3 bytes, scale [rows] fp32;
 * dim % 8 == 0, dim <= 14336, strides >= dim and % 8 == 0.  Per row, with amax = max|x|:
 *   e      the smallest integer with amax 2^-e <= 448, clamped to [-126, 127]
 *   scale  2^e;   out8 = e4m3(x 2^-e), round to nearest even as gf_cast_fp8 rounds.  The product is exact in fp32 (a power of two; what
 *          underflows fp32 is far below e4m3's half step and rounds to +-0 either way), so there is ONE rounding, the codes are the
 *          e4m3 rounding of the gradient itself in a shifted exponent window, |x 2^-e| <= 448 never gives the NaN code, and the GEMM
 *          epilogue's `* row_scale` adds no rounding.
 *   zero row (amax == 0)                e = 0, the cast's codes of +-0 (0x00 / 0x80)
 *   a row holding an inf or a NaN       scale = NaN and all codes 0x00: that row of the GEMM comes out NaN, never silently zero
 * Nothing outside [rows, dim] of either output is written. */
GF_API int gf_quant_fp8_grad(const void* x, void* out8, float* scale, int64_t rows, int64_t dim,
                             int64_t x_stride, int64_t out_stride, void* stream);

/* gf_cast_fp8_t — the transposed e4m3 weight copy, made once per weight: w [N, K] bf16 (row pitch ldw) -> out8 [K, N] e4m3 bytes (row
 * pitch ldo), out8[k, n] bit for bit what gf_cast_fp8 makes of w[n, k] (the NaN code above 464 included) — the [N', K'] operand of
 * gf_gemm_fp8 with the layer's out_features as the reduction dimension.  N % 128 == 0 (N becomes the GEMM's K), K % 8 == 0,
 * ldw % 8 == 0, ldw >= K, ldo % 16 == 0, ldo >= N, both pointers 16-byte aligned.  Bytes [N, ldo) of an output row are not written. */
GF_API int gf_cast_fp8_t(const void* w, int64_t ldw, void* out8, int64_t ldo, int64_t N, int64_t K, void* stream);

/* gf_gemm_fp8 — C = epilogue((A8 · W8^T) * row_scale[m] + bias); A8 [M,K], W8 [N,K] e4m3 bytes (K contiguous),
 * fp32 accumulate on v_mfma_f32_16x16x128_f8f6f4 (2x the bf16 MFMA rate; M >= 512: the 4-wave asm K loop).  As MEASURED through
 * these kernels on an MI355X (no vendor statement; model: tests/gemm_refs.py::mfma_fp8, held by tests/test_gemm_pinned_gpu.py::
 * test_fp8_mfma_model), the sum is not that of exact products in fp32: inside every group of 8 consecutive k the products are aligned to
 * the group's largest exponent and truncated 13 bits below it, so each group is within 7 * 2^-13 of its largest product of exact;
 * same epilogues / residual / gate semantics as gf_gemm_bf16 (torch._scaled_mm, VRAM:141-148).
 * K % 128 == 0, lda/ldw % 16 == 0. */
GF_API int gf_gemm_fp8(const void* A8, int64_t lda, const void* W8, int64_t ldw, const float* row_scale,
                       const void* bias, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                       int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* gf_gemm_fp8_lora — an fp8 Linear with ONE attached LoRA adapter added in the GEMM's epilogue (the reference's
 * AutoWrappedLinear.forward, VRAM:168-187: out = fp8_linear(x), then out + x @ lora_A.T @ lora_B.T on the bf16 x):
 *     y0       = bf16( (A8 · W8^T)[m,n] * row_scale[m] + bias[n] )
 *     out[m,n] = epi( bf16( y0 + bf16( scale * bf16( sum_j t[m,j] * up[n,j] ) ) ), resid, gate )
 * by definition the bits of gf_gemm_fp8(..., GF_EPI_BIAS) followed by gf_lora_up(..., epilogue, resid, gate): the same K loop, the
 * same three bf16 roundings taken in registers, the rank summed as gf_lora_up sums it (a zero fp32 accumulator, one
 * v_mfma_f32_16x16x32_bf16 per chunk of 32 rank columns, chunks ascending); y0 is never written.  The first eleven operands and
 * M .. stream are gf_gemm_fp8's (out [M, ldo] = its C); t [M, ldt] bf16 = bf16(x down^T), up [N, ld_up] bf16 with columns true rank ..
 * rank_pad - 1 zero, rank_pad and scale follow gf_lora_up's contract (ldt / ld_up multiples of 8 that cover rank_pad, 16-byte aligned
 * bases, scale finite).  out may alias resid.  It runs exactly where gf_gemm_fp8_lora_ok returns 1 — the 4-wave kernel's shapes
 * (M >= 512, K % 128 == 0, N % 8 == 0, 256 rows of K bytes within 2^31), rank_pad 32 or 64, option prefer_8wave off; a pure function
 * of its arguments and that option — and refuses everything else by message with out untouched: there the two launches are the route
 * (ops.gemm_fp8_lora takes it). */
GF_API int gf_gemm_fp8_lora_ok(int64_t M, int64_t N, int64_t K, int64_t rank_pad);
GF_API int gf_gemm_fp8_lora(const void* A8, int64_t lda, const void* W8, int64_t ldw, const float* row_scale, const void* bias,
                            const void* t, int64_t ldt, const void* up, int64_t ld_up, int64_t rank_pad, float scale, void* out,
                            int64_t ldo, int64_t M, int64_t N, int64_t K, int epilogue, const void* resid, int64_t ldr,
                            const void* gate, void* stream);

/* ========================================================================
 * MXFP4 Linear — OCP Microscaling FP4 (no counterpart in the reference; off by default, dit.enable_fp4).  The format, stated once:
 *   element  e2m1, code s|ee|m: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 (codes 0..7), bit 3 the sign
 *   packing  byte i of a row holds element 2i in bits 3:0 and element 2i+1 in bits 7:4
 *   scale    one E8M0 byte per 32 consecutive k: value 2^(code - 127), code 255 = NaN; stored row-major [rows, K/32] with a stride
 * Quantiser recipe (bf16 in, blocks of 32 along the contiguous dimension; every step exact arithmetic on power-of-two scalings):
 *   amax = the largest |x| of the block (exact: bf16 subnormals are not flushed);  amax = 0 -> code 127, all elements +0
 *   else e = floor(log2 amax) - 2, code = clamp(e + 127, 0, 254)  (bf16's exponent range reaches codes 0 .. 252 only)
 *   element = x * 2^-(code - 127) rounded to the nearest e2m1 value, ties to the even mantissa code (5 -> 4, 2.5 -> 2, 0.25 -> 0),
 *   the magnitude saturating at 6 (7 -> 6), the sign kept (-0 and values that round to zero keep their sign bit)
 *   a block holding any NaN or +-inf -> code 255, all elements +0
 * ======================================================================== */

/* gf_quant_mxfp4 — x [rows, dim] bf16 (row stride x_stride elements) -> out4 [rows, dim/2] packed bytes (row stride out_stride bytes)
 * and scales [rows, dim/32] E8M0 bytes (row stride scale_stride bytes), one pass; serves activations and weights alike.
 * dim % 32 == 0; x 16-byte aligned with x_stride % 8 == 0; out4 4-byte aligned with out_stride % 4 == 0; rows = 0 is a no-op. */
GF_API int gf_quant_mxfp4(const void* x, int64_t x_stride, void* out4, int64_t out_stride, void* scales, int64_t scale_stride,
                          int64_t rows, int64_t dim, void* stream);

/* gf_gemm_mxfp4 — C = epilogue(bf16(sum_k A^[m,k] W^[n,k] + bias)), A^ / W^ the dequantised operands: A4 [M, K/2] / W4 [N, K/2] packed
 * e2m1 (lda / ldw in BYTES, multiples of 16), a_scale [M, K/32] / w_scale [N, K/32] E8M0 with their row strides in bytes.  The block
 * scales are applied inside v_mfma_scale_f32_16x16x128_f8f6f4 (both operands e2m1: 4x the bf16 MFMA rate); no row scale in the
 * epilogue.  Epilogues, bf16 rounding sequence, residual / gate semantics and C-aliases-resid are gf_gemm_bf16's.
 * Any M >= 0, N % 8 == 0, K % 256 == 0 (one 128-byte LDS row = 256 elements = two MFMA k-steps).
 * NaN: a row of A whose scale row holds code 255 comes out NaN in all its columns, a row of W with one makes its column NaN.
 * OBSERVED on an MI355X (one instruction per wave, no vendor statement): the instruction itself returns NaN for every output of a lane's
 * row / column whose scale byte is 255, also over a block of zeros and whatever the other operand holds.  The kernel does not rely on
 * it: its epilogue sets those rows / columns to NaN from the scale bytes it fetched.
 * Accumulation, as measured (tests/fp4_refs.py::MODEL_NOTE): products inside a block are summed exactly; with the four
 * blocks' scale sums within 2^+-4 and a zero accumulator the result is the exact sum rounded to fp32; beyond that it is a fixed-point
 * adder — a block 22 - 23 binades below the instruction's largest scale sum is dropped, bits about 23 below it are cut — so an output
 * is within K 2^-23 S + T of the exact product (T: fp4_refs.mfma_mxfp4; about one fp32 ulp of S on operands from gf_quant_mxfp4). */
GF_API int gf_gemm_mxfp4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw,
                         const void* w_scale, int64_t w_scale_stride, const void* bias, void* C, int64_t ldc, int64_t M, int64_t N,
                         int64_t K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* The two producers of an fp4 Linear's activation that quantise in the registers that hold the finished bf16 values, so that the bf16
 * intermediate never reaches memory.  The block quantiser is one function (csrc/gf_mxfp4_quant.h) and works on bit patterns: both give
 * the BYTES of the two-call path they replace (tests/test_fp4_fused_gpu.py: torch.equal on codes and scales).
 *
 * gf_layernorm_modulate_mxfp4 — gf_layernorm_modulate (its arithmetic and roundings, every subset of weight / bias / scale1p / shift)
 * whose consumer is an fp4 Linear: out4 [rows, dim/2] packed e2m1 (row stride out_stride BYTES) and scales [rows, dim/32] E8M0 (row
 * stride scale_stride bytes) = gf_quant_mxfp4 of the bf16 row gf_layernorm_modulate would have written.  dim must be one of the
 * wave-per-row widths 5120 / 4096 / 1536; other widths: call the two functions.  x 16-byte aligned with x_stride % 8 == 0, the vectors
 * 16-byte aligned, out4 4-byte aligned with out_stride % 4 == 0 (16 / 16 to serve as gf_gemm_mxfp4's A4); rows = 0 is a no-op. */
GF_API int gf_layernorm_modulate_mxfp4(const void* x, void* out4, void* scales, const void* weight, const void* bias,
                                       const void* scale1p, const void* shift, int64_t rows, int64_t dim, int64_t x_stride,
                                       int64_t out_stride, int64_t scale_stride, float eps, void* stream);

/* gf_gemm_mxfp4_q4 — C4 / c_scale = gf_quant_mxfp4(gf_gemm_mxfp4(...)) without C existing in memory: the epilogue's read-back quantises
 * the finished bf16 values (activation and NaN-scale handling applied) 32 output columns at a time.  C4 [M, N/2] packed e2m1, 16-byte
 * aligned, ldc4 in BYTES with ldc4 % 16 == 0 and ldc4 >= N/2 (a legal A4 of the next GEMM); c_scale [M, N/32] E8M0 with
 * c_scale_stride >= N/32.  N % 32 == 0; the epilogues without a second operand only (GF_EPI_BIAS, GF_EPI_BIAS_GELU_TANH,
 * GF_EPI_BIAS_SILU); every other operand rule is gf_gemm_mxfp4's.  A NaN output (a NaN scale in its row of A or of W) makes its block
 * code 255 with zero elements, as gf_quant_mxfp4 does.  M = 0 is a no-op. */
GF_API int gf_gemm_mxfp4_q4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw,
                            const void* w_scale, int64_t w_scale_stride, const void* bias, void* C4, int64_t ldc4, void* c_scale,
                            int64_t c_scale_stride, int64_t M, int64_t N, int64_t K, int epilogue, void* stream);

/* ------------------------------------------------------------------------
 * gf_conv3d_padded_bf16 — CausalConv3d 3x3x3, stride 1 (VAE:33-52) of the 192- and 384-channel levels of Decoder3d / Encoder3d
 * (VAE:736-838, 517-617) as a direct convolution on the 4-wave GEMM loop (gf_conv_a4.hip).
 *   xp   : zero-bordered activation [kt - 1 + T][H + 2][W + 2][C] bf16 — kt = 3: frames 0, 1 = the two cached history frames (zeros =
 *          no history), real pixel (t, y, x) at [2 + t][1 + y][1 + x]; kt = 1 (a 3x3 convolution per frame, e.g. the resample
 *          convolution behind the nearest-exact 2x upsample, VAE:82-96): no history frames; one pixel of zeros around every frame
 *   Wm   : [N, ldw] bf16, K order (dt, dy, dx, cin), ldw >= 9 kt C
 *   out  : [T H W, ldo] bf16 = conv + bias (GF_EPI_BIAS) or resid + bf16(conv + bias) (GF_EPI_BIAS_RESID, resid [T H W, ldr])
 * C = 192 or 384; results bit-identical to gf_conv3d_bf16 on the same values.  The caller owns every buffer; no workspace.
 * gf_vae_rmsnorm_silu_padded — gf_vae_rmsnorm_silu writing into the interior of such a buffer: out_interior = &xp[f][1][1][0].
 * gf_vae_upsample2x_padded — nearest-exact 2x upsample of [T, H, W, C] into the interior of a [T][2 H + 2][2 W + 2][C] buffer. */
GF_API int gf_conv3d_padded_bf16(const void* xp, const void* Wm, int64_t ldw, const void* bias, void* out, int64_t ldo, int64_t T,
                                 int64_t H, int64_t W, int64_t C, int64_t N, int64_t kt, int epilogue, const void* resid, int64_t ldr,
                                 void* stream);
GF_API int gf_vae_rmsnorm_silu_padded(const void* x, const void* gamma, void* out_interior, int64_t T, int64_t H, int64_t W, int64_t C,
                                      int silu, void* stream);
GF_API int gf_vae_upsample2x_padded(const void* x, void* out_interior, int64_t T, int64_t H, int64_t W, int64_t C, void* stream);

/* ------------------------------------------------------------------------
 * SageAttention backend (the reference's `sageattn(q, k, v)` branch of flash_attention, DIT:22-26, 50-54): int8 QK^T with
 * smoothed K, e4m3 P·V, fp32 accumulation; head_dim 128, non-causal, no mask.  The recipe (granularities are this project's own):
 *   mu[h][c]     = fp32 mean of k over the kv_len keys (fp64 sums);  k~ = fp32(k) - mu
 *   q8, q_scale  : int8 codes, one scale per (head, 32 query rows from row 0): scale = amax / 127, code = rne(x * (127 / amax))
 *                  clamped to +-127; an all-zero block has scale 0 and codes 0.  k8, k_scale: the same on k~ per (head, 64 keys)
 *   vt8, v_scale : e4m3fn codes of V^T, one scale per (head, channel) over all keys: scale = amax / 448, code = e4m3(v * (448 / amax))
 *   tiny blocks  : where the reciprocal 127 / amax (448 / amax) is not finite in fp32 — a non-zero amax below about 3.7e-37 (1.3e-36);
 *                  bf16 reaches down to 9.2e-41 — the block is quantised with the reciprocal FLT_MAX and gets the scale 2^-128 =
 *                  fp32(1 / FLT_MAX): every code is finite, a zero element has code 0, code x scale is the element to within the
 *                  code's own rounding.  Every other block is as stated above, bit for bit.  (Two such scales, s_q s_k = 2^-256,
 *                  underflow to w = 0: a tiny Q or K block against another attends uniformly — as scores of 1e-74 would.)
 *   s            = float(int32 dot) * fp32(fp32(s_q s_k) * c), c = scale * log2(e)
 *   per 128-key tile in key order: m = running row maximum of s, P = e4m3(exp2(s - m + 8)), l = sum of that P, acc = sum P V_code
 *   (fp32, rescaled by exp2(m_old - m_new) when m moves); O = bf16(acc / l * v_scale)
 * Layouts (caller-owned; the library never allocates):
 *   q8 [q_len][heads*128] int8;  q_scale [heads][ceil(q_len / 32)] fp32
 *   k8 [kv_pad8][heads*128] int8 (kv_pad8 = kv_len rounded up to 128, rows >= kv_len zero);  k_scale [heads][kv_pad8 / 64] fp32
 *   vt8 [heads*128][kv_pad8] e4m3, inside every 128-key slice key k at position 32 ((k >> 2) & 3) + 4 (k >> 4) + (k & 3) (the PV
 *       MFMA operand order), keys >= kv_len zero;  v_scale [heads][128] fp32;  mu [heads][128] fp32
 *   scratch: heads * 64 * 128 * 8 bytes (row-chunk partial sums of gf_sage_k_mean / maxima of gf_sage_quant_vt)
 * Inputs are bf16 with a row stride (a column slice of a wider tensor is fine), 16-byte aligned, strides multiples of 8. */
GF_API int64_t gf_sage_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads);   /* bytes gf_sage_attn needs */
GF_API int gf_sage_k_mean(const void* k, int64_t ldk, float* mu, void* scratch, int64_t kv_len, int64_t heads, void* stream);
GF_API int gf_sage_quant_q(const void* q, int64_t ldq, void* q8, float* q_scale, int64_t q_len, int64_t heads, void* stream);
GF_API int gf_sage_quant_k(const void* k, int64_t ldk, const float* mu, void* k8, float* k_scale, int64_t kv_len, int64_t heads,
                           void* stream);
/* vt_in = 0: v is V [kv_len][ldv];  vt_in = 1: v is the bf16 V^T of gf_linear_vt32 / gf_linear_vt32_fp8 / gf_transpose_v32 with
 * ldv = its kv_pad (a multiple of 64). */
GF_API int gf_sage_quant_vt(const void* v, int64_t ldv, int vt_in, void* vt8, float* v_scale, void* scratch, int64_t kv_len,
                            int64_t heads, void* stream);
GF_API int gf_sage_attn_fwd(const void* q8, const float* q_scale, const void* k8, const float* k_scale, const void* vt8,
                            const float* v_scale, void* o, int64_t ldo, int64_t q_len, int64_t kv_len, int64_t heads, float scale,
                            void* stream);
/* gf_sage_attn — the four quantisation passes and the attention in one call; ws = gf_sage_workspace_bytes bytes, laid out as
 * q8, k8, vt8, q_scale, k_scale, v_scale, mu, scratch, each starting on a 256-byte boundary.  It is its five staged calls in the
 * order k_mean, quant_q, quant_k, quant_vt, attn_fwd; a refusal of a later stage may follow the earlier stages' writes into ws —
 * only o is untouched by every refusal. */
GF_API int gf_sage_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int vt_in, void* o,
                        int64_t ldo, int64_t q_len, int64_t kv_len, int64_t heads, float scale, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOALFORCE_H */

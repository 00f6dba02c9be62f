// gf_cross_fold.hip — the cross-attention with its output projection folded into the cached values.
//
// Per head h the cross-attention output is a mix of at most n_keys fixed value rows: o = sum_h P_h V_h W_o,h^T + b.  With the
// table U_h = V_h W_o,h^T ([n_keys x N], constant per (expert, prompt, block), memoised like the K/V) the projection becomes ONE
// GEMM [S x heads*n_pad] x [heads*n_pad x N] on the normalised probabilities, K = heads * n_pad instead of heads * 128.
//   * gf_cross_probs: P^[s, h*n_pad + j] = bf16(w_hj), w_hj = exp2(c s_hj + log2 m_j - c max) / l_h, for n_keys < 64 — one key tile,
//     so the max, the sum and the normalisation happen in one pass (no online rescale).  Score arithmetic as kernel 2
//     (gf_attention.hip) on the same operands: the 32x32x16 bf16 MFMA S^T = K Q^T in fp32, scaled in fp32 (fmaf(s, c, -c max)), the
//     last key's multiplicity as + log2(m) / c on its raw score.
//     Column n_keys carries the rounding residue of the LAST key's weight, bf16(w - bf16(w)): that key (the prompt's padding, m of
//     the 512 context rows) usually holds most of a row's mass, and its weight rounded to bf16 alone would scale the whole head's
//     output by up to 2^-9 — an error the unfolded path does not make (its largest unnormalised weight is exactly 1).  Columns
//     n_keys < j < n_pad are exact zeros.
//   * gf_cross_fold_table: U[n, h*n_pad + j] = bf16(sum_d V[j, h*128 + d] W_o[n, h*128 + d]), fp32 accumulation in d order, one
//     rounding; column n_keys repeats column n_keys - 1 (the residue's partner), the columns after it are exact zeros.
// Kept out of gf_attention.hip: profiles/pmc_static.json keys the self-attention's counters on that file's sha256.
#include "gf_common.h"

namespace {

constexpr int CF_HD = 128;        // head dim
constexpr int CF_MAXK = 64;       // keys per row: one tile
constexpr int CF_THREADS = 256;   // 4 waves x 32 query rows
constexpr int CF_QB = 128;        // query rows per workgroup

__device__ __forceinline__ void cf_mfma32(f32x16& acc, const bf16x8& a, const bf16x8& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// one workgroup = (128 query rows, one head).  The key tile (rows >= n_keys zero) is staged in LDS with kernel 2's K image:
// 256-byte rows, 16-byte chunk c of row r at chunk c ^ sK(r), sK(r) = ((r & 3) << 2) | ((r >> 2) & 3).
// MFMA layout (as kernel 2): A = K[32 keys x 16 d] (lane: key r, d 16 kd + 8 h .. +7), B = Q^T (lane: query r, same d),
// D: lane (r, h) element e = query r, key 32 half + 4 h + (e & 3) + 8 (e >> 2); the other half of a row's keys is in lane ^ 32.
__global__ __launch_bounds__(CF_THREADS) void cross_probs_kernel(const u16* __restrict__ q, const u16* __restrict__ k, u16* __restrict__ pout,
                                                                 int q_len, int n_keys, int n_pad, int heads, long q_stride, long k_stride,
                                                                 long p_stride, float c, float last_key_bias) {
    __shared__ __attribute__((aligned(16))) char lds[CF_MAXK * 256];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int q0 = blockIdx.x * CF_QB + wave * 32;
    const int halves = n_keys > 32 ? 2 : 1;

#pragma unroll
    for (int i = 0; i < (CF_MAXK * 16) / CF_THREADS; ++i) {
        const int idx = tid + CF_THREADS * i;
        const int row = idx >> 4, ch = idx & 15;
        u16x8 v8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < n_keys) v8 = *reinterpret_cast<const u16x8*>(k + (long)row * k_stride + head * CF_HD + ch * 8);
        const int sk = ((row & 3) << 2) | ((row >> 2) & 3);
        *(u16x8*)(lds + row * 256 + ((ch ^ sk) << 4)) = v8;
    }

    bf16x8 qf[8];
    {
        const int qr = min(q0 + r, q_len - 1);
        const u16* qp = q + (long)qr * q_stride + head * CF_HD + 8 * h;
#pragma unroll
        for (int kd = 0; kd < 8; ++kd) qf[kd] = *reinterpret_cast<const bf16x8*>(qp + 16 * kd);
    }
    __syncthreads();

    f32x16 sc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sc[0][e] = 0.f;
        sc[1][e] = 0.f;
    }
    const int sK = ((r & 3) << 2) | ((r >> 2) & 3);
#pragma unroll
    for (int kd = 0; kd < 8; ++kd) {
        const int off = 256 * r + 16 * ((2 * kd + h) ^ sK);
        cf_mfma32(sc[0], *(const bf16x8*)(lds + off), qf[kd]);
        if (halves == 2) cf_mfma32(sc[1], *(const bf16x8*)(lds + off + 32 * 256), qf[kd]);
    }

    // mask + multiplicity, max, exp2, sum: the arithmetic of kernel 2's softmax on its only tile
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int key = 4 * h + (e & 3) + 8 * (e >> 2);
        if (key >= n_keys) sc[0][e] = -INFINITY;
        if (key + 32 >= n_keys) sc[1][e] = -INFINITY;
        if (key == n_keys - 1) sc[0][e] += last_key_bias;
        if (key + 32 == n_keys - 1) sc[1][e] += last_key_bias;
    }
    float mx = sc[0][0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, sc[0][e]);
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sc[1][e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mc = mx * c;
    float rs = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sc[0][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[0][e], c, -mc));
        sc[1][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[1][e], c, -mc));
        rs += sc[0][e] + sc[1][e];
    }
    const float l_tot = rs + __shfl_xor(rs, 32);
    const float inv = 1.0f / l_tot;
    // the last key's weight: held by one lane of the pair (r, r + 32), the other contributes an exact 0
    float pl = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int key = 4 * h + (e & 3) + 8 * (e >> 2);
        if (key == n_keys - 1) pl = sc[0][e];
        if (key + 32 == n_keys - 1) pl = sc[1][e];
    }
    pl += __shfl_xor(pl, 32);
    const float wl = pl * inv;
    const float wl_lo = wl - bf2f(f2bf(wl));

    // lane (r, h) owns keys 32 half + 8 g + 4 h .. +3 of row q0 + r: one 8-byte store per (half, g) inside [0, n_pad); key n_keys
    // (masked, 0 so far) takes the residue
    const int qrow = q0 + r;
    if (qrow < q_len) {
        u16* prow = pout + (long)qrow * p_stride + (long)head * n_pad;
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int key = 32 * half + 8 * g + 4 * h;
                if (key < n_pad) {
                    float w4[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) w4[i] = key + i == n_keys ? wl_lo : sc[half][4 * g + i] * inv;
                    u32x2 pk;
                    pk[0] = pack2bf(w4[0], w4[1]);
                    pk[1] = pack2bf(w4[2], w4[3]);
                    *reinterpret_cast<u32x2*>(prow + key) = pk;
                }
            }
    }
}

// one workgroup = (64 output rows n, one head): V_h in LDS (n_pad rows: row n_keys repeats row n_keys - 1, zero after it); thread
// (n = tid >> 2, jg = tid & 3) owns columns j = jg + 4 i of row n and walks d = 0 .. 127 in order (fp32 FMAs), one bf16 rounding.
constexpr int CFT_ROWS = 64;
__global__ __launch_bounds__(CF_THREADS) void cross_fold_table_kernel(const u16* __restrict__ v, const u16* __restrict__ w, u16* __restrict__ u,
                                                                      int n_keys, int n_pad, int n_out, long v_stride, long w_stride,
                                                                      long u_stride) {
    __shared__ __attribute__((aligned(16))) u16 vs[CF_MAXK * CF_HD];
    const int tid = threadIdx.x;
    const int head = blockIdx.y;
    for (int idx = tid; idx < n_pad * 16; idx += CF_THREADS) {
        const int row = idx >> 4, ch = idx & 15;
        u16x8 v8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row <= n_keys) v8 = *reinterpret_cast<const u16x8*>(v + (long)min(row, n_keys - 1) * v_stride + head * CF_HD + ch * 8);
        *reinterpret_cast<u16x8*>(vs + row * CF_HD + ch * 8) = v8;
    }
    __syncthreads();
    const int n = blockIdx.x * CFT_ROWS + (tid >> 2), jg = tid & 3;
    if (n >= n_out) return;
    const int nj = n_pad >> 2;   // columns of this thread (n_pad is a multiple of 16)
    float acc[CF_MAXK / 4];
#pragma unroll
    for (int i = 0; i < CF_MAXK / 4; ++i) acc[i] = 0.f;
    const u16* wr = w + (long)n * w_stride + head * CF_HD;
    for (int d0 = 0; d0 < CF_HD; d0 += 8) {
        const u16x8 w8 = *reinterpret_cast<const u16x8*>(wr + d0);
        float wf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wf[e] = bf2f(w8[e]);
#pragma unroll
        for (int i = 0; i < CF_MAXK / 4; ++i) {
            if (i < nj) {
                const u16x8 v8 = *reinterpret_cast<const u16x8*>(vs + (jg + 4 * i) * CF_HD + d0);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i] = __builtin_fmaf(bf2f(v8[e]), wf[e], acc[i]);
            }
        }
    }
    u16* ur = u + (long)n * u_stride + (long)head * n_pad;
#pragma unroll
    for (int i = 0; i < CF_MAXK / 4; ++i) {
        const int j = jg + 4 * i;
        if (i < nj) ur[j] = j <= n_keys ? f2bf(acc[i]) : (u16)0;
    }
}

}  // namespace

extern "C" GF_API int gf_cross_probs(const void* q, const void* k, void* p, int64_t q_len, int64_t n_keys, int64_t n_pad, int64_t heads,
                                     int64_t head_dim, int64_t q_stride, int64_t k_stride, int64_t p_stride, float scale,
                                     float last_key_multiplicity, void* stream) {
    GF_CHECK_ARG(q && k && p, "gf_cross_probs: null pointer");
    if (head_dim != CF_HD) {
        gf_set_error("gf_cross_probs: head_dim=%ld unsupported (kernel is built for 128)", (long)head_dim);
        return GF_ERR_UNSUPPORTED;
    }
    GF_CHECK_ARG(q_len >= 0 && q_len < (1 << 30) && heads > 0 && heads < 65536, "gf_cross_probs: bad sizes q=%ld heads=%ld", (long)q_len,
                 (long)heads);
    GF_CHECK_ARG(n_keys >= 1 && n_pad % 16 == 0 && n_pad > n_keys && n_pad <= CF_MAXK,
                 "gf_cross_probs: 1 <= n_keys=%ld < n_pad=%ld <= 64, n_pad a multiple of 16", (long)n_keys, (long)n_pad);
    GF_CHECK_ARG(q_stride % 8 == 0 && k_stride % 8 == 0 && p_stride % 4 == 0 && q_stride >= heads * CF_HD && k_stride >= heads * CF_HD &&
                     p_stride >= heads * n_pad,
                 "gf_cross_probs: strides must cover the rows (q, k: multiples of 8; p: of 4, >= heads * n_pad)");
    GF_CHECK_ARG(gf_aligned16(q) && gf_aligned16(k) && ((uintptr_t)p & 7u) == 0, "gf_cross_probs: alignment (q, k 16 bytes, p 8 bytes)");
    GF_CHECK_ARG(scale > 0.f && last_key_multiplicity >= 1.0f, "gf_cross_probs: scale > 0, multiplicity >= 1");
    if (q_len == 0) return GF_OK;
    const float c = scale * 1.4426950408889634f;
    const float bias = last_key_multiplicity != 1.0f ? log2f(last_key_multiplicity) / c : 0.f;
    const dim3 grid((unsigned)((q_len + CF_QB - 1) / CF_QB), (unsigned)heads);
    hipLaunchKernelGGL(cross_probs_kernel, grid, dim3(CF_THREADS), 0, (hipStream_t)stream, (const u16*)q, (const u16*)k, (u16*)p,
                       (int)q_len, (int)n_keys, (int)n_pad, (int)heads, (long)q_stride, (long)k_stride, (long)p_stride, c, bias);
    GF_CHECK_LAUNCH("gf_cross_probs");
    return GF_OK;
}

extern "C" GF_API int gf_cross_fold_table(const void* v, const void* w_o, void* u, int64_t n_keys, int64_t n_pad, int64_t heads,
                                          int64_t head_dim, int64_t n_out, int64_t v_stride, int64_t w_stride, int64_t u_stride,
                                          void* stream) {
    GF_CHECK_ARG(v && w_o && u, "gf_cross_fold_table: null pointer");
    if (head_dim != CF_HD) {
        gf_set_error("gf_cross_fold_table: head_dim=%ld unsupported (kernel is built for 128)", (long)head_dim);
        return GF_ERR_UNSUPPORTED;
    }
    GF_CHECK_ARG(heads > 0 && heads < 65536 && n_out > 0 && n_out < (1 << 30), "gf_cross_fold_table: bad sizes heads=%ld N=%ld", (long)heads,
                 (long)n_out);
    GF_CHECK_ARG(n_keys >= 1 && n_pad % 16 == 0 && n_pad > n_keys && n_pad <= CF_MAXK,
                 "gf_cross_fold_table: 1 <= n_keys=%ld < n_pad=%ld <= 64, n_pad a multiple of 16", (long)n_keys, (long)n_pad);
    GF_CHECK_ARG(v_stride % 8 == 0 && w_stride % 8 == 0 && v_stride >= heads * CF_HD && w_stride >= heads * CF_HD && u_stride >= heads * n_pad,
                 "gf_cross_fold_table: strides must cover the rows (v, w_o: multiples of 8; u >= heads * n_pad)");
    GF_CHECK_ARG(gf_aligned16(v) && gf_aligned16(w_o) && ((uintptr_t)u & 1u) == 0, "gf_cross_fold_table: alignment");
    const dim3 grid((unsigned)((n_out + CFT_ROWS - 1) / CFT_ROWS), (unsigned)heads);
    hipLaunchKernelGGL(cross_fold_table_kernel, grid, dim3(CF_THREADS), 0, (hipStream_t)stream, (const u16*)v, (const u16*)w_o, (u16*)u,
                       (int)n_keys, (int)n_pad, (int)n_out, (long)v_stride, (long)w_stride, (long)u_stride);
    GF_CHECK_LAUNCH("gf_cross_fold_table");
    return GF_OK;
}

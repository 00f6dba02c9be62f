// gf_sage_attention.hip — SageAttention-style self-attention (SageAttention2's qk_int8_pv_fp8 structure), head_dim 128,
// non-causal, no mask: the backend the reference's flash_attention() takes when the `sageattention` package is installed
// (diffsynth/models/wan_video_dit.py:22-26, 50-54).  The arithmetic is this project's own restatement (the package pins none):
//   * K smoothing: mu_h = fp32 mean of k over all keys per channel, k~ = k - mu_h (softmax unchanged);
//   * Q -> int8, one fp32 scale per (head, 32 query rows);  K~ -> int8, one per (head, 64 keys):
//     scale = amax / 127, code = rne(x * (127 / amax)) clamped to +-127 (an all-zero block: scale 0, codes 0);
//   * V -> OCP e4m3fn, one scale per (head, channel) over all keys: scale = amax / 448, code = e4m3fn_rne(v * (448 / amax));
//   * scores s = float(int32 dot) * w with w = fp32(fp32(s_q s_k) c), c = softmax scale x log2(e) (exp2 domain);
//   * online softmax over tiles of SAGE_T = 128 keys in index order, the running maximum m updated on every tile (tau = 0):
//     P = e4m3fn(exp2(s - m + SAGE_E)), SAGE_E = 8, so P <= 256 stays inside e4m3fn; l = the sum of that same quantised P,
//     acc = sum P V_code in fp32; O = bf16(acc / l * v_scale[channel]).
// tests/sage_oracle.py restates all of it in torch (fp64 sums of exact products).
//
// Kernel layout (gf_sage_attn_fwd; one workgroup = 4 waves = 128 query rows of one head, 32 rows per wave = ONE Q scale block;
// two workgroups per CU, so the two waves of a SIMD belong to different workgroups and are not held in phase by the per-tile
// barrier: one runs its MFMAs while the other runs its softmax; r = lane & 15, g = lane >> 4):
//   S^T = K~ Q^T on v_mfma_i32_16x16x64_i8: A = K~ codes [16 keys x 64 d] (lane: key 16 kb + r, bytes 64 ks + 16 g .. +16),
//        B = Q codes (same byte map, query 16 qb + r), D = sc[kb][qb] (i32x4): query 16 qb + r, keys 16 kb + 4 g + j.  The
//        int32 dot is exact, so the hardware's k order inside a step does not matter as long as A and B share the byte map.
//   O^T += V^T P^T on the K = 128 f8f6f4 MFMA (e4m3 x e4m3, unit block scales): B = P^T, lane (r, g) byte jj = 4 kb + j holds
//        P of key 16 kb + 4 g + j — the lane's own scores, converted in place; A = V^T codes [16 channels x 128 keys], lane byte
//        jj of channel 16 db + r is the same key: gf_sage_quant_vt stores every 128-key slice in that order (position 32 g + jj).
//   Row sums l on the matrix pipe: a ninth channel block whose A fragment is e4m3 1.0 in row 0.
//   K~ and V^T tiles (16 KiB each) arrive by LDS-DMA into a 2-deep ring; the blockIdx map is kernel 3's XCD-aware one.
#include <cfloat>

#include "gf_mfma_frame.h"

namespace {

constexpr int SAGE_T = 128;        // keys per tile
constexpr int SAGE_E = 8;          // exponent offset: P <= 2^8
constexpr int SAGE_NW = 4;         // waves per workgroup (32 query rows each); two workgroups per CU
constexpr int SAGE_QB = 32 * SAGE_NW;   // query rows per workgroup
constexpr int SAGE_QBLK = 32;      // query rows per Q scale
constexpr int SAGE_KBLK = 64;      // keys per K scale
constexpr int SAGE_NCH = 64;       // row chunks of the column reductions (mean of K, amax of V)
constexpr int HD = 128;
constexpr int TILE_BYTES = SAGE_T * HD;   // 16 KiB of int8 K~ or of e4m3 V^T
constexpr int SAGE_LDS = 4 * TILE_BYTES;  // K ring + V^T ring (64 KiB: two workgroups per CU); the epilogue reuses it for O

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4s;

long pad_to(long n, long m) { return (n + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------------ column reductions
// partial[h][chunk][c] over the rows of chunk `chunk` (SAGE_NCH chunks of ceil(rows / SAGE_NCH) rows): the fp64 sum of
// the bf16 values (AMAX = false, the mean of K) or their largest magnitude (AMAX = true, the V scale).
template <bool AMAX>
__global__ __launch_bounds__(256) void sage_colreduce_kernel(const u16* __restrict__ x, long ld, int rows, double* __restrict__ partial) {
    __shared__ double red[16][HD];
    const int chunk = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int c8 = tid & 15, rs = tid >> 4;
    const int per = (rows + SAGE_NCH - 1) / SAGE_NCH;
    const int r0 = chunk * per, r1 = min(rows, r0 + per);
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int row = r0 + rs; row < r1; row += 16) {
        const u16x8 v = *reinterpret_cast<const u16x8*>(x + (long)row * ld + h * HD + 8 * c8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = bf2f(v[e]);
            if constexpr (AMAX)
                acc[e] = fmax(acc[e], (double)fabsf(f));
            else
                acc[e] += (double)f;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rs][8 * c8 + e] = acc[e];
    __syncthreads();
    if (tid < HD) {
        double t = red[0][tid];
        for (int i = 1; i < 16; ++i) t = AMAX ? fmax(t, red[i][tid]) : t + red[i][tid];
        partial[((long)h * SAGE_NCH + chunk) * HD + tid] = t;
    }
}

// mu[h][c] = fp32(sum over the chunks in order / rows)
__global__ __launch_bounds__(HD) void sage_mean_finish_kernel(const double* __restrict__ partial, int rows, float* __restrict__ mu) {
    const int h = blockIdx.x, c = threadIdx.x;
    double t = 0.0;
    for (int i = 0; i < SAGE_NCH; ++i) t += partial[((long)h * SAGE_NCH + i) * HD + c];
    mu[h * HD + c] = (float)(t / (double)rows);
}

// V^T input (gf_linear_vt32 / gf_transpose_v32 layout: [heads*128][kv_pad_in], inside every 32-key group position 8 g + i holds
// key 4 g + i (i < 4) or 16 + 4 g + i - 4): the amax of one channel is a row reduction, written as chunk 0 of partial.
__global__ __launch_bounds__(256) void sage_vt_amax_kernel(const u16* __restrict__ vt, long kv_pad_in, int kv_len, double* __restrict__ partial) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // row = h * 128 + channel
    float m = 0.f;
    for (long p0 = 8L * lane; p0 < kv_pad_in; p0 += 512) {
        const u16x8 v = *reinterpret_cast<const u16x8*>(vt + (long)row * kv_pad_in + p0);
        const int grp = (int)(p0 >> 5), gq = (int)((p0 & 31) >> 3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = 32 * grp + (i < 4 ? 4 * gq + i : 16 + 4 * gq + i - 4);
            if (key < kv_len) m = fmaxf(m, fabsf(bf2f(v[i])));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) partial[((long)(row >> 7) * SAGE_NCH) * HD + (row & 127)] = (double)m;
}

// ------------------------------------------------------------------------------------------------ Q / K~ to int8
// One workgroup per (block of BR rows, head).  Rows >= rows_valid do not enter the amax; rows in [rows_valid, rows_out) get
// code 0 (the padded keys of K~).  mu (K only) is subtracted in fp32 before the amax.
template <int BR>
__global__ __launch_bounds__(256) void sage_quant_rows_kernel(const u16* __restrict__ x, long ld, const float* __restrict__ mu,
                                                             signed char* __restrict__ out, long ldo, float* __restrict__ scale,
                                                             int rows_valid, int rows_out, int nblk) {
    constexpr int PER = BR * 16 / 256;   // 8-element chunks per thread
    __shared__ float wred[4];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    float f[PER][8];
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int ci = tid + 256 * i, row = b * BR + (ci >> 4), c8 = ci & 15;
        if (row < rows_valid) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(x + (long)row * ld + h * HD + 8 * c8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                f[i][e] = mu ? bf2f(v[e]) - mu[h * HD + 8 * c8 + e] : bf2f(v[e]);
                m = fmaxf(m, fabsf(f[i][e]));
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[i][e] = 0.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) wred[tid >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    // a block whose amax is so small that 127 / amax overflows (below ~3.7e-37): inv = FLT_MAX, scale = 2^-128 = fp32(1 / FLT_MAX)
    // (include/goalforce.h); 0 x inf would be NaN, and fmaxf(NaN, -127) code -127
    const bool tiny = amax > 0.f && !(127.0f / amax <= FLT_MAX);
    const float inv = amax > 0.f ? (tiny ? FLT_MAX : 127.0f / amax) : 0.f;
    if (tid == 0 && b < nblk) scale[(long)h * nblk + b] = tiny ? 0x1p-128f : amax / 127.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int ci = tid + 256 * i, row = b * BR + (ci >> 4), c8 = ci & 15;
        if (row < rows_out) {
            unsigned w[2] = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float c = fminf(fmaxf(__builtin_rintf(f[i][e] * inv), -127.f), 127.f);
                w[e >> 2] |= ((unsigned)(int)c & 0xffu) << (8 * (e & 3));
            }
            *reinterpret_cast<u32x2*>(out + (long)row * ldo + h * HD + 8 * c8) = u32x2{w[0], w[1]};
        }
    }
}

// ------------------------------------------------------------------------------------------------ V -> e4m3 V^T
// One workgroup per (128-key tile, head): vt8[h*128 + c][kv_pad8], key k of the tile at position 32 ((k >> 2) & 3) + 4 (k >> 4)
// + (k & 3) (the PV MFMA's operand order, see the file header).  Keys >= kv_len are code 0.  The channel amax comes from nch
// chunks of partial.  VT_IN: the input is the bf16 V^T of gf_linear_vt32 (see sage_vt_amax_kernel), else V [kv_len][ld].
template <bool VT_IN>
__global__ __launch_bounds__(256) void sage_quant_vt_kernel(const u16* __restrict__ v, long ld, const double* __restrict__ partial, int nch,
                                                           unsigned char* __restrict__ vt8, long kv_pad8, float* __restrict__ vscale, int kv_len) {
    __shared__ float s_inv[HD];
    __shared__ __attribute__((aligned(16))) unsigned char tile[HD * SAGE_T];
    const int t = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    if (tid < HD) {
        double a = 0.0;
        for (int i = 0; i < nch; ++i) a = fmax(a, partial[((long)h * SAGE_NCH + i) * HD + tid]);
        const float amax = (float)a;
        // a channel whose amax is so small that 448 / amax overflows (below ~1.3e-36): inv = FLT_MAX, scale = 2^-128 (include/goalforce.h);
        // 0 x inf would be the e4m3 NaN code
        const bool tiny = amax > 0.f && !(448.0f / amax <= FLT_MAX);
        s_inv[tid] = amax > 0.f ? (tiny ? FLT_MAX : 448.0f / amax) : 0.f;
        if (t == 0) vscale[h * HD + tid] = tiny ? 0x1p-128f : amax / 448.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ci = tid + 256 * i;
        if constexpr (VT_IN) {
            // channel row c, input positions 8 m16 .. +8 of the tile = keys 32 G + 4 m + (0..3) and 32 G + 16 + 4 m + (0..3),
            // G = m16 >> 2, m = m16 & 3: output positions 32 m + 8 G + (0..7), contiguous
            const int c = ci >> 4, m16 = ci & 15, G = m16 >> 2, mm = m16 & 3;
            const int kbase = t * SAGE_T + 32 * G;
            u16x8 x = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (kbase < kv_len) x = *reinterpret_cast<const u16x8*>(v + (long)(h * HD + c) * ld + t * SAGE_T + 8 * m16);
            const float inv = s_inv[c];
            unsigned w[2] = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const int k0 = kbase + (e < 4 ? 4 * mm + e : 16 + 4 * mm + e - 4);
                const float a0 = k0 < kv_len ? bf2f(x[e]) * inv : 0.f, a1 = k0 + 1 < kv_len ? bf2f(x[e + 1]) * inv : 0.f;
                const unsigned pk = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false) & 0xffffu;
                w[e >> 2] |= pk << (8 * (e & 3));
            }
            *reinterpret_cast<u32x2*>(tile + c * SAGE_T + 32 * mm + 8 * G) = u32x2{w[0], w[1]};
        } else {
            const int kl = ci >> 4, c8 = ci & 15, key = t * SAGE_T + kl;
            const int pos = 32 * ((kl >> 2) & 3) + 4 * (kl >> 4) + (kl & 3);
            u16x8 x = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (key < kv_len) x = *reinterpret_cast<const u16x8*>(v + (long)key * ld + h * HD + 8 * c8);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const unsigned pk = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[e]) * s_inv[8 * c8 + e],
                                                                              bf2f(x[e + 1]) * s_inv[8 * c8 + e + 1], 0, false);
                tile[(8 * c8 + e) * SAGE_T + pos] = (unsigned char)(pk & 0xffu);
                tile[(8 * c8 + e + 1) * SAGE_T + pos] = (unsigned char)((pk >> 8) & 0xffu);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = tid + 256 * i, c = ci >> 3, ch = ci & 7;
        *reinterpret_cast<u32x4*>(vt8 + (long)(h * HD + c) * kv_pad8 + t * SAGE_T + 16 * ch) =
            *reinterpret_cast<const u32x4*>(tile + c * SAGE_T + 16 * ch);
    }
}

// ------------------------------------------------------------------------------------------------ attention
struct SageArgs {
    const signed char* q8;        // [q_len][heads*128]
    const float* q_scale;         // [heads][nqs]
    const signed char* k8;        // [kv_pad8][heads*128]
    const float* k_scale;         // [heads][kv_pad8 / 64]
    const unsigned char* vt8;     // [heads*128][kv_pad8]
    const float* v_scale;         // [heads][128]
    u16* o;
    long ldo, kv_pad8;
    int q_len, kv_len, heads, n_qblocks, nqs;
    float c;                      // softmax scale x log2(e)
};

__device__ __forceinline__ void mfma_i8(i32x4& acc, const i32x4& a, const i32x4& b) {
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_f8(f32x4& acc, const i32x8& a, const i32x8& b) {
    // e4m3 x e4m3 (format 0 / 0), E8M0 block scales 127 = 2^0
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, 127, 0, 127);
}

__global__ __launch_bounds__(64 * SAGE_NW, 2) void sage_attn_fwd_kernel(const SageArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    GF_LDS char* lds = (GF_LDS char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    int head, qb0;   // XCD-aware (kernel 3's map): the CUs of one XCD walk the query blocks of ONE head, its K~ / V^T stream shared in their L2
    gf_xcd_head_block(blockIdx.x, p.heads, p.n_qblocks, head, qb0);
    const int q0 = qb0 * SAGE_QB + wave * 32;

    // Q codes: qf[qb][ks] = bytes 64 ks + 16 g .. +16 of query q0 + 16 qb + r
    i32x4 qf[2][2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int qr = min(q0 + 16 * qb + r, p.q_len - 1);
        const signed char* qp = p.q8 + (long)qr * p.heads * HD + head * HD + 16 * g;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[qb][ks] = *reinterpret_cast<const i32x4*>(qp + 64 * ks);
    }
    const float sq = p.q_scale[(long)head * p.nqs + min(q0 / SAGE_QBLK, p.nqs - 1)];

    // ---- staging: a tile is 16 pieces of 1 KiB (8 rows of 128 B); wave w stages pieces w and w + 8.  Lane L: row 8 P + (L >> 3),
    // physical 16-byte chunk L & 7 = logical chunk ^ (row & 7)
    auto make_srd = [](const void* base) {
        const unsigned long b = (unsigned long)base;
        u32x4s s;
        s[0] = (unsigned)b;
        s[1] = (unsigned)(b >> 32) & 0xffffu;
        s[2] = 0xffffffffu;
        s[3] = 0x00020000u;
        return s;
    };
    const u32x4s srd_k = make_srd(p.k8 + head * HD), srd_v = make_srd(p.vt8 + (long)head * HD * p.kv_pad8);
    const int drow = lane >> 3, dlch = (lane & 7) ^ (drow & 7);
    const unsigned k_lane = (unsigned)(drow * p.heads * HD + 16 * dlch), v_lane = (unsigned)(drow * p.kv_pad8 + 16 * dlch);
    auto dma16b = [&](const u32x4s& srd, unsigned voff, unsigned soff, GF_LDS char* l) __attribute__((always_inline)) {
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)l);
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                     :
                     : "v"(voff), "s"(srd), "s"(dst), "s"(soff)
                     : "memory");
    };
    auto stage = [&](int t, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < 16 / SAGE_NW; ++jj) {
            const int piece = wave + SAGE_NW * jj;
            dma16b(srd_k, k_lane, (unsigned)((t * SAGE_T + 8 * piece) * p.heads * HD), lds + buf * TILE_BYTES + piece * 1024);
            dma16b(srd_v, v_lane, (unsigned)(8 * piece * p.kv_pad8 + t * SAGE_T), lds + 2 * TILE_BYTES + buf * TILE_BYTES + piece * 1024);
        }
    };
    // fragment offsets inside a buffer: K~ (kb, ks): row 16 kb + r, logical chunk 4 ks + g;  V^T (db): row 16 db + r, chunks 2 g, 2 g + 1
    int koff[2], voff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) koff[ks] = 128 * r + 16 * ((4 * ks + g) ^ (r & 7));
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) voff[hh] = 2 * TILE_BYTES + 128 * r + 16 * ((2 * g + hh) ^ (r & 7));

    constexpr int NDB = 9;   // 8 channel blocks of O^T + the row sums
    f32x4 oacc[NDB][2];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) oacc[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    i32x8 ones;   // e4m3 1.0 (0x38) in row 0 of the A operand
    {
        const int o1 = r == 0 ? 0x38383838 : 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = o1;
    }
    float mrun[2] = {-INFINITY, -INFINITY};
    const int nt = (p.kv_len + SAGE_T - 1) / SAGE_T;
    const int nks = (int)(p.kv_pad8 / SAGE_KBLK);

    stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                       // tile t landed for every wave; every wave is done with buffer 1 - buf
        if (t + 1 < nt) stage(t + 1, 1 - buf);
        // ---- S^T = K~ Q^T (int32, exact)
        i32x4 sc[8][2];
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const i32x4 kf = *(GF_LDS i32x4*)(lds + buf * TILE_BYTES + koff[ks] + kb * 2048);
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    if (ks == 0) sc[kb][qb] = i32x4{0, 0, 0, 0};
                    mfma_i8(sc[kb][qb], kf, qf[qb][ks]);
                }
            }
        }
        // ---- dequant scale per 64-key half (wave-uniform), masking of a ragged last tile
        float w[2];
        bool hvalid[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            w[hf] = (sq * p.k_scale[(long)head * nks + 2 * t + hf]) * p.c;
            hvalid[hf] = t * SAGE_T + 64 * hf < p.kv_len;
        }
        const bool ragged = (t + 1) * SAGE_T > p.kv_len;
        if (ragged) {
#pragma unroll
            for (int kb = 0; kb < 8; ++kb)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t * SAGE_T + 16 * kb + 4 * g + j >= p.kv_len) {
#pragma unroll
                        for (int qb = 0; qb < 2; ++qb) sc[kb][qb][j] = INT_MIN;
                    }
        }
        // ---- row maxima: the int32 maximum of each half, dequantised (monotone: the same as the maximum of the fp32 scores)
        bool moved = false;
        float mnew[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float mt = -INFINITY;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                int im = INT_MIN;
#pragma unroll
                for (int kb = 4 * hf; kb < 4 * hf + 4; ++kb)
#pragma unroll
                    for (int j = 0; j < 4; ++j) im = max(im, sc[kb][qb][j]);
                im = max(im, __shfl_xor(im, 16));
                im = max(im, __shfl_xor(im, 32));
                if (hvalid[hf]) mt = fmaxf(mt, (float)im * w[hf]);
            }
            mnew[qb] = fmaxf(mrun[qb], mt);
            moved |= mnew[qb] > mrun[qb];
        }
        if (__any(moved)) {
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                const float alpha = mnew[qb] > mrun[qb] ? __builtin_amdgcn_exp2f(mrun[qb] - mnew[qb]) : 1.0f;
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int e = 0; e < 4; ++e) oacc[db][qb][e] *= alpha;
                mrun[qb] = mnew[qb];
            }
        }
        // ---- P = e4m3(exp2(s - m + E)), packed in place as the B operand (byte 4 kb + j)
        i32x8 pf[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const float off = (float)SAGE_E - mrun[qb];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const float wh = w[kb >> 2];
                float e4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e4[j] = __builtin_amdgcn_exp2f(__builtin_fmaf((float)sc[kb][qb][j], wh, off));
                int pk = __builtin_amdgcn_cvt_pk_fp8_f32(e4[0], e4[1], 0, false);
                pk = __builtin_amdgcn_cvt_pk_fp8_f32(e4[2], e4[3], pk, true);
                pf[qb][kb] = pk;
            }
        }
        // keys past kv_len of a ragged tile: their P bytes are cleared here, in that tile only (a compare and a select per score
        // in every tile cost a third of the softmax's vector issue)
        if (ragged) {
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                unsigned keep = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t * SAGE_T + 16 * kb + 4 * g + j < p.kv_len) keep |= 0xffu << (8 * j);
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) pf[qb][kb] &= (int)keep;
            }
        }
        // ---- O^T += V^T P^T, l += 1^T P^T
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const u32x4 v0 = *(GF_LDS u32x4*)(lds + buf * TILE_BYTES + voff[0] + db * 2048);
            const u32x4 v1 = *(GF_LDS u32x4*)(lds + buf * TILE_BYTES + voff[1] + db * 2048);
            const i32x8 vf = __builtin_bit_cast(i32x8, (__attribute__((ext_vector_type(8))) unsigned){v0[0], v0[1], v0[2], v0[3],
                                                                                                     v1[0], v1[1], v1[2], v1[3]});
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) mfma_f8(oacc[db][qb], vf, pf[qb]);
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) mfma_f8(oacc[NDB - 1][qb], ones, pf[qb]);
    }

    // ---- epilogue: O = bf16(acc / l * v_scale), through LDS as whole 256-byte rows (kernel 3's image)
    float inv[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) inv[qb] = 1.0f / __shfl(oacc[NDB - 1][qb][0], r);
    __syncthreads();
    GF_LDS char* ob = lds + wave * (32 * 256);
#pragma unroll
    for (int db = 0; db < 8; ++db) {
        const f32x4 vs = *reinterpret_cast<const f32x4*>(p.v_scale + head * HD + 16 * db + 4 * g);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            u32x2 pk;
            pk[0] = pack2bf(oacc[db][qb][0] * inv[qb] * vs[0], oacc[db][qb][1] * inv[qb] * vs[1]);
            pk[1] = pack2bf(oacc[db][qb][2] * inv[qb] * vs[2], oacc[db][qb][3] * inv[qb] * vs[3]);
            const int row = 16 * qb + r;
            *(GF_LDS u32x2*)(ob + row * 256 + (((2 * db + (g >> 1)) ^ (row & 15)) << 4) + 8 * (g & 1)) = pk;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int row = 4 * it + (lane >> 4), ch = lane & 15;
        const u16x8 v8 = *(GF_LDS u16x8*)(ob + row * 256 + ((ch ^ (row & 15)) << 4));
        if (q0 + row < p.q_len) *reinterpret_cast<u16x8*>(p.o + (long)(q0 + row) * p.ldo + head * HD + 8 * ch) = v8;
    }
}

// ------------------------------------------------------------------------------------------------ workspace layout
struct SageWs {
    long q8, k8, vt8, q_scale, k_scale, v_scale, mu, scratch, total;
};
SageWs sage_layout(long q_len, long kv_len, long heads) {
    const long kv_pad8 = pad_to(kv_len, SAGE_T), nqs = (q_len + SAGE_QBLK - 1) / SAGE_QBLK;
    SageWs w;
    long o = 0;
    auto take = [&](long bytes) { const long at = o; o += pad_to(bytes, 256); return at; };
    w.q8 = take(q_len * heads * HD);
    w.k8 = take(kv_pad8 * heads * HD);
    w.vt8 = take(heads * HD * kv_pad8);
    w.q_scale = take(heads * nqs * 4);
    w.k_scale = take(heads * (kv_pad8 / SAGE_KBLK) * 4);
    w.v_scale = take(heads * HD * 4);
    w.mu = take(heads * HD * 4);
    w.scratch = take(heads * SAGE_NCH * HD * 8);
    w.total = o;
    return w;
}

bool sage_sizes_ok(long rows, long heads) { return rows > 0 && heads > 0 && pad_to(rows, SAGE_T) * heads * HD < (1L << 31); }

}  // namespace

extern "C" GF_API int64_t gf_sage_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads) {
    if (q_len < 0 || kv_len <= 0 || heads <= 0) return 0;
    return sage_layout(q_len, kv_len, heads).total;
}

extern "C" GF_API int gf_sage_k_mean(const void* k, int64_t ldk, float* mu, void* scratch, int64_t kv_len, int64_t heads, void* stream) {
    GF_CHECK_ARG(k && mu && scratch, "gf_sage_k_mean: null pointer");
    GF_CHECK_ARG(sage_sizes_ok(kv_len, heads) && ldk >= heads * HD && ldk % 8 == 0 && gf_aligned16(k),
                 "gf_sage_k_mean: bad shape (kv_len=%ld heads=%ld ldk=%ld) or k not 16-byte aligned", (long)kv_len, (long)heads, (long)ldk);
    hipLaunchKernelGGL(sage_colreduce_kernel<false>, dim3(SAGE_NCH, (unsigned)heads), dim3(256), 0, (hipStream_t)stream, (const u16*)k, (long)ldk,
                       (int)kv_len, (double*)scratch);
    hipLaunchKernelGGL(sage_mean_finish_kernel, dim3((unsigned)heads), dim3(HD), 0, (hipStream_t)stream, (const double*)scratch, (int)kv_len, mu);
    GF_CHECK_LAUNCH("gf_sage_k_mean");
    return GF_OK;
}

static int sage_quant_rows(const char* what, int br, const void* x, int64_t ld, const float* mu, void* out, float* scale, int64_t rows,
                           int64_t rows_out, int64_t heads, void* stream) {
    GF_CHECK_ARG(x && out && scale, "%s: null pointer", what);
    GF_CHECK_ARG(sage_sizes_ok(rows, heads) && ld >= heads * HD && ld % 8 == 0 && gf_aligned16(x) && gf_aligned16(out),
                 "%s: bad shape (rows=%ld heads=%ld ld=%ld) or a pointer not 16-byte aligned", what, (long)rows, (long)heads, (long)ld);
    const int nblk = (int)((rows_out + br - 1) / br);
    if (br == SAGE_QBLK)
        hipLaunchKernelGGL(sage_quant_rows_kernel<SAGE_QBLK>, dim3(nblk, (unsigned)heads), dim3(256), 0, (hipStream_t)stream, (const u16*)x,
                           (long)ld, mu, (signed char*)out, (long)(heads * HD), scale, (int)rows, (int)rows_out, nblk);
    else
        hipLaunchKernelGGL(sage_quant_rows_kernel<SAGE_KBLK>, dim3(nblk, (unsigned)heads), dim3(256), 0, (hipStream_t)stream, (const u16*)x,
                           (long)ld, mu, (signed char*)out, (long)(heads * HD), scale, (int)rows, (int)rows_out, nblk);
    GF_CHECK_LAUNCH(what);
    return GF_OK;
}

extern "C" GF_API int gf_sage_quant_q(const void* q, int64_t ldq, void* q8, float* q_scale, int64_t q_len, int64_t heads, void* stream) {
    return sage_quant_rows("gf_sage_quant_q", SAGE_QBLK, q, ldq, nullptr, q8, q_scale, q_len, q_len, heads, stream);
}

extern "C" GF_API int gf_sage_quant_k(const void* k, int64_t ldk, const float* mu, void* k8, float* k_scale, int64_t kv_len, int64_t heads,
                                      void* stream) {
    GF_CHECK_ARG(mu, "gf_sage_quant_k: null mu");
    return sage_quant_rows("gf_sage_quant_k", SAGE_KBLK, k, ldk, mu, k8, k_scale, kv_len, pad_to(kv_len, SAGE_T), heads, stream);
}

extern "C" GF_API int gf_sage_quant_vt(const void* v, int64_t ldv, int vt_in, void* vt8, float* v_scale, void* scratch, int64_t kv_len,
                                       int64_t heads, void* stream) {
    GF_CHECK_ARG(v && vt8 && v_scale && scratch, "gf_sage_quant_vt: null pointer");
    GF_CHECK_ARG(sage_sizes_ok(kv_len, heads) && gf_aligned16(v) && gf_aligned16(vt8) && ldv % 8 == 0,
                 "gf_sage_quant_vt: bad shape (kv_len=%ld heads=%ld ldv=%ld) or a pointer not 16-byte aligned", (long)kv_len, (long)heads, (long)ldv);
    const long kv_pad8 = pad_to(kv_len, SAGE_T);
    const dim3 grid((unsigned)(kv_pad8 / SAGE_T), (unsigned)heads);
    if (vt_in) {
        // ldv = kv_pad of the bf16 V^T (a multiple of 64, >= kv_len); the quant pass reads whole 32-key groups below kv_len
        GF_CHECK_ARG(ldv >= kv_len && ldv % 64 == 0, "gf_sage_quant_vt: V^T input needs kv_pad (ldv=%ld) a multiple of 64 >= kv_len", (long)ldv);
        hipLaunchKernelGGL(sage_vt_amax_kernel, dim3((unsigned)(heads * HD / 4)), dim3(256), 0, (hipStream_t)stream, (const u16*)v, (long)ldv,
                           (int)kv_len, (double*)scratch);
        hipLaunchKernelGGL(sage_quant_vt_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const u16*)v, (long)ldv,
                           (const double*)scratch, 1, (unsigned char*)vt8, kv_pad8, v_scale, (int)kv_len);
    } else {
        GF_CHECK_ARG(ldv >= heads * HD, "gf_sage_quant_vt: ldv=%ld below heads*128", (long)ldv);
        hipLaunchKernelGGL(sage_colreduce_kernel<true>, dim3(SAGE_NCH, (unsigned)heads), dim3(256), 0, (hipStream_t)stream, (const u16*)v,
                           (long)ldv, (int)kv_len, (double*)scratch);
        hipLaunchKernelGGL(sage_quant_vt_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const u16*)v, (long)ldv,
                           (const double*)scratch, SAGE_NCH, (unsigned char*)vt8, kv_pad8, v_scale, (int)kv_len);
    }
    GF_CHECK_LAUNCH("gf_sage_quant_vt");
    return GF_OK;
}

extern "C" GF_API int gf_sage_attn_fwd(const void* q8, const float* q_scale, const void* k8, const float* k_scale, const void* vt8,
                                       const float* v_scale, void* o, int64_t ldo, int64_t q_len, int64_t kv_len, int64_t heads, float scale,
                                       void* stream) {
    GF_CHECK_ARG(q8 && q_scale && k8 && k_scale && vt8 && v_scale && o, "gf_sage_attn_fwd: null pointer");
    GF_CHECK_ARG(q_len >= 0 && sage_sizes_ok(kv_len, heads) && pad_to(q_len, SAGE_T) * heads * HD < (1L << 31) && ldo >= heads * HD &&
                     ldo % 8 == 0 && gf_aligned16(q8) && gf_aligned16(k8) && gf_aligned16(vt8) && gf_aligned16(o) && gf_aligned16(v_scale),
                 "gf_sage_attn_fwd: bad shape (q=%ld kv=%ld heads=%ld ldo=%ld) or a pointer not 16-byte aligned", (long)q_len, (long)kv_len,
                 (long)heads, (long)ldo);
    // the row maximum is taken on the int32 dots and dequantised once: that is the maximum of the scores only for w = s_q s_k c >= 0
    GF_CHECK_ARG(scale > 0.f && scale < INFINITY, "gf_sage_attn_fwd: the softmax scale must be positive and finite (got %g)", (double)scale);
    if (q_len == 0) return GF_OK;
    SageArgs a;
    a.q8 = (const signed char*)q8;
    a.q_scale = q_scale;
    a.k8 = (const signed char*)k8;
    a.k_scale = k_scale;
    a.vt8 = (const unsigned char*)vt8;
    a.v_scale = v_scale;
    a.o = (u16*)o;
    a.ldo = ldo;
    a.kv_pad8 = pad_to(kv_len, SAGE_T);
    a.q_len = (int)q_len;
    a.kv_len = (int)kv_len;
    a.heads = (int)heads;
    a.n_qblocks = (int)((q_len + SAGE_QB - 1) / SAGE_QB);
    a.nqs = (int)((q_len + SAGE_QBLK - 1) / SAGE_QBLK);
    a.c = scale * 1.4426950408889634f;   // the factor kernel 3 uses (gf_attention.hip: scale_log2e)
    return gf_launch_lds<sage_attn_fwd_kernel>("gf_sage_attn_fwd", GF_ATTR_MSG_PLAIN, "gf_sage_attn_fwd", dim3((unsigned)(a.n_qblocks * a.heads)), dim3(64 * SAGE_NW),
                                               SAGE_LDS, (hipStream_t)stream, a);
}

extern "C" GF_API int gf_sage_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int vt_in, void* o,
                                   int64_t ldo, int64_t q_len, int64_t kv_len, int64_t heads, float scale, void* ws, void* stream) {
    GF_CHECK_ARG(ws, "gf_sage_attn: null workspace");
    GF_CHECK_ARG(scale > 0.f && scale < INFINITY, "gf_sage_attn: the softmax scale must be positive and finite (got %g)", (double)scale);
    if (q_len == 0) return GF_OK;
    GF_CHECK_ARG(sage_sizes_ok(kv_len, heads) && q_len > 0, "gf_sage_attn: bad lengths q=%ld kv=%ld heads=%ld", (long)q_len, (long)kv_len,
                 (long)heads);
    const SageWs L = sage_layout(q_len, kv_len, heads);
    char* w = (char*)ws;
    int s;
    if ((s = gf_sage_k_mean(k, ldk, (float*)(w + L.mu), w + L.scratch, kv_len, heads, stream)) != GF_OK) return s;
    if ((s = gf_sage_quant_q(q, ldq, w + L.q8, (float*)(w + L.q_scale), q_len, heads, stream)) != GF_OK) return s;
    if ((s = gf_sage_quant_k(k, ldk, (const float*)(w + L.mu), w + L.k8, (float*)(w + L.k_scale), kv_len, heads, stream)) != GF_OK) return s;
    if ((s = gf_sage_quant_vt(v, ldv, vt_in, w + L.vt8, (float*)(w + L.v_scale), w + L.scratch, kv_len, heads, stream)) != GF_OK) return s;
    return gf_sage_attn_fwd(w + L.q8, (const float*)(w + L.q_scale), w + L.k8, (const float*)(w + L.k_scale), w + L.vt8,
                            (const float*)(w + L.v_scale), o, ldo, q_len, kv_len, heads, scale, stream);
}

// gf_lora_grad.hip — the parameter gradients of a LoRA adapter (gfx950): a tall-skinny product that sums over the tokens,
//     out[c, j] = bf16( fp32(scale) * sum_{m < M} Y[m, c] * T[m, j] )          c < C, j < rank_pad  (transposed: stored at out[j, c])
// read straight from the row-major operands: Y [M, C] is the wide activation (dy for dUp, x for dDown), T [M, rank_pad] the
// narrow one (t = bf16(x down^T) for dUp, dt = bf16(dy up) for dDown).  No transposed copy of either is written.
//
// Arithmetic: fp32 accumulation on v_mfma_f32_16x16x32_bf16, nothing rounded to bf16 before the last token is in, `scale`
// multiplied into the fp32 sum, ONE bf16 rounding per element.  At scale 1 (the reference trains with lora_alpha = r) that is torch's
// bf16 autograd chain; at any other scale torch rounds the scaled dy (or the product) once more, so this is one rounding tighter.
// A sum that is zero is stored as +0 whatever the sign of `scale`.
//
// The token split: the tokens are cut into gf_lora_grad_slabs(M, C, rank_pad) slabs of gf_lora_grad_slab_rows(...) rows (the last
// one ragged); workgroup (column tile of 64, slab) sums its slab in ascending token tiles of 64 and writes the fp32 partial
// ws[slab][c][j] (c padded to the column tile).  A second kernel adds the slabs in ASCENDING slab order, applies scale, rounds and
// stores in the asked orientation: no floating-point atomics, the same bits on every call.
//
// Frame: 256 threads = 4 waves; wave w owns the 16 columns 16 w .. 16 w + 15 of the tile and all rank_pad / 16 accumulator
// fragments.  A stage is 64 tokens: coalesced 16-byte pieces of Y [64][64] and T [64][rank_pad] go through registers into one LDS
// image each (the next stage's pieces are in flight during the MFMAs).  Both MFMA operands are walked along the tokens, the slow
// index of both images, so both are read with ds_read_b64_tr_b16: lane (g = lane >> 4, i = lane & 15) supplies the address of row
// 4 g + (i >> 2) (second read: + 16), columns 4 (i & 3) .. + 3 of its 16-column block and receives column i of the four rows; the
// MFMA's k position 8 g + e is thus token 4 g + e (e < 4) / 16 + 4 g + (e - 4) of the 32-token half in BOTH operands.  Row pitch =
// row bytes + 32, an odd multiple of 32 bytes: the eight rows a 32-lane half reads start 8 banks apart, no conflicts.  Rows
// beyond the slab and columns beyond C are staged as +0 (pad, don't mask: the transposing read needs EXEC all ones).
#include "gf_mfma_frame.h"

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_CT = 64;          // columns of Y per workgroup
constexpr int LG_KT = 64;          // tokens per stage
constexpr int LG_MAX_RANK = 256;
constexpr int LG_MIN_TILES = 4;    // at most one slab per 4 stages (256 tokens), rounded up
constexpr int LG_TARGET_WG = 1024; // 4 workgroups per CU
constexpr int LG_PY = LG_CT * 2 + 32;   // LDS row pitch of the Y image, bytes

struct LoraGradArgs {
    const u16* Y;
    const u16* T;
    float* ws;
    long ldy, ldt;
    int M, C, cpad, ctiles, slab_rows;
};

struct LoraGradSumArgs {
    const float* ws;
    u16* out;
    long ldo;
    int C, cpad, rank_pad, slabs;
    float scale;
};

typedef __attribute__((ext_vector_type(4))) short lg_s16x4;
typedef __attribute__((ext_vector_type(8))) short lg_s16x8;

// the 16 (columns) x 32 (tokens) operand of block `blk` = image + column offset, rows 32 h ..: two transposing reads
__device__ __forceinline__ bf16x8 lg_frag(GF_LDS char* p, int pitch) {
    const lg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((GF_LDS lg_s16x4*)p);
    const lg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((GF_LDS lg_s16x4*)(p + 16 * pitch));
    const lg_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// NJ = rank_pad / 16 accumulator fragments per wave
template <int NJ>
__global__ __launch_bounds__(LG_THREADS) void lora_grad_kernel(const LoraGradArgs p) {
    constexpr int RP = NJ * 16;
    constexpr int PT = RP * 2 + 32;                    // LDS row pitch of the T image, bytes
    constexpr int TPIECES = RP / 8;                    // 16-byte pieces per T row
    constexpr int TN = (LG_KT * TPIECES + LG_THREADS - 1) / LG_THREADS;   // T pieces per thread and stage
    extern __shared__ __attribute__((aligned(16))) char lg_lds[];
    GF_LDS char* yimg = (GF_LDS char*)lg_lds;
    GF_LDS char* timg = yimg + LG_KT * LG_PY;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctile = blockIdx.x % p.ctiles, slab = blockIdx.x / p.ctiles;
    const int c0 = ctile * LG_CT;
    const int m0 = slab * p.slab_rows;
    const int m1 = min(p.M, m0 + p.slab_rows);
    const int ntiles = (m1 - m0 + LG_KT - 1) / LG_KT;

    // staging: Y piece q of this thread = row 32 q + (tid >> 3), columns 8 (tid & 7) ..; T piece q = item tid + 256 q of [row][piece]
    const int yrow = tid >> 3, ycol = (tid & 7) * 8;
    const bool ycol_ok = c0 + ycol < p.C;              // C % 8 == 0: a piece is inside or outside as a whole
    const u16* ysrc = p.Y + (long)c0 + ycol;
    u16x8 yreg[2], treg[TN];
    const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int tile) {
        const int mt = m0 + tile * LG_KT;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = mt + 32 * q + yrow;
            yreg[q] = zero8;
            if (ycol_ok && m < m1) yreg[q] = *reinterpret_cast<const u16x8*>(ysrc + (long)m * p.ldy);
        }
#pragma unroll
        for (int q = 0; q < TN; ++q) {
            const int idx = tid + LG_THREADS * q;
            const int m = mt + idx / TPIECES;
            treg[q] = zero8;
            if (idx < LG_KT * TPIECES && m < m1) treg[q] = *reinterpret_cast<const u16x8*>(p.T + (long)m * p.ldt + (idx % TPIECES) * 8);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < 2; ++q) *(GF_LDS u16x8*)(yimg + (32 * q + yrow) * LG_PY + ycol * 2) = yreg[q];
#pragma unroll
        for (int q = 0; q < TN; ++q) {
            const int idx = tid + LG_THREADS * q;
            if (idx < LG_KT * TPIECES) *(GF_LDS u16x8*)(timg + (idx / TPIECES) * PT + (idx % TPIECES) * 16) = treg[q];
        }
    };

    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's address in a 16-column block: row 4 g + (i >> 2), columns 4 (i & 3) ..
    const int trow = 4 * (lane >> 4) + ((lane & 15) >> 2), tcol = 4 * (lane & 3);
    GF_LDS char* ya = yimg + trow * LG_PY + (16 * wave + tcol) * 2;
    GF_LDS char* ta = timg + trow * PT + tcol * 2;

    if (ntiles > 0) fetch(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        __syncthreads();                               // the previous stage's reads are done
        stage();
        __syncthreads();
        if (tile + 1 < ntiles) fetch(tile + 1);
#pragma unroll
        for (int h = 0; h < LG_KT / 32; ++h) {
            const bf16x8 a = lg_frag(ya + 32 * h * LG_PY, LG_PY);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const bf16x8 b = lg_frag(ta + 32 * h * PT + 32 * j, PT);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
            }
        }
    }

    // accumulator element r of fragment j: column c0 + 16 wave + 4 g + r of Y, rank column 16 j + i
    float* w = p.ws + ((long)slab * p.cpad + c0 + 16 * wave + 4 * (lane >> 4)) * RP + (lane & 15);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) w[(long)r * RP + 16 * j] = acc[j][r];
}

// one thread = eight consecutive elements of an `out` row
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void lora_grad_sum_kernel(const LoraGradSumArgs p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long items = (long)p.C * p.rank_pad / 8;
    if (idx >= items) return;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    u16* dst;
    if constexpr (TRANSPOSED) {
        const int j = (int)(idx % p.rank_pad);
        const long c = idx / p.rank_pad * 8;
        for (int sl = 0; sl < p.slabs; ++sl) {
            const float* w = p.ws + ((long)sl * p.cpad + c) * p.rank_pad + j;
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += w[(long)e * p.rank_pad];
        }
        dst = p.out + (long)j * p.ldo + c;
    } else {
        const int pieces = p.rank_pad / 8;
        const int j = (int)(idx % pieces) * 8;
        const long c = idx / pieces;
        for (int sl = 0; sl < p.slabs; ++sl) {
            const float* w = p.ws + ((long)sl * p.cpad + c) * p.rank_pad + j;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(w), hi = *reinterpret_cast<const f32x4*>(w + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += lo[e], s[4 + e] += hi[e];
        }
        dst = p.out + c * p.ldo + j;
    }
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(p.scale * s[e] + 0.f);     // + 0: a zero sum times a negative scale is stored as +0
    *reinterpret_cast<u16x8*>(dst) = o;
}

// ---- the slab rule, a pure function of (M, C, rank_pad): stages of 64 tokens, enough slabs that column tiles x slabs reaches
// LG_TARGET_WG workgroups, at most one slab per LG_MIN_TILES stages (rounded up), equal slabs but for the last
struct LoraGradPlan {
    long ctiles, slabs, slab_rows;
};
bool lora_grad_shape_ok(int64_t M, int64_t C, int64_t rank_pad) {
    return M >= 0 && M < (1 << 30) && C > 0 && C < (1 << 30) && C % 8 == 0 && rank_pad >= 32 && rank_pad <= LG_MAX_RANK && rank_pad % 32 == 0;
}
LoraGradPlan lora_grad_plan(int64_t M, int64_t C) {
    LoraGradPlan pl;
    pl.ctiles = (C + LG_CT - 1) / LG_CT;
    const long mtiles = (M + LG_KT - 1) / LG_KT;
    if (mtiles == 0) {
        pl.slabs = 0, pl.slab_rows = 0;
        return pl;
    }
    const long want = (LG_TARGET_WG + pl.ctiles - 1) / pl.ctiles;
    long target = (mtiles + LG_MIN_TILES - 1) / LG_MIN_TILES;
    if (target > want) target = want;
    const long per = (mtiles + target - 1) / target;
    pl.slabs = (mtiles + per - 1) / per;
    pl.slab_rows = per * LG_KT;
    return pl;
}

}  // namespace

extern "C" {

int64_t gf_lora_grad_slabs(int64_t M, int64_t C, int64_t rank_pad) {
    return lora_grad_shape_ok(M, C, rank_pad) ? lora_grad_plan(M, C).slabs : 0;
}

int64_t gf_lora_grad_slab_rows(int64_t M, int64_t C, int64_t rank_pad) {
    return lora_grad_shape_ok(M, C, rank_pad) ? lora_grad_plan(M, C).slab_rows : 0;
}

int64_t gf_lora_grad_workspace_bytes(int64_t M, int64_t C, int64_t rank_pad) {
    if (!lora_grad_shape_ok(M, C, rank_pad)) return 0;
    const LoraGradPlan pl = lora_grad_plan(M, C);
    return pl.slabs * pl.ctiles * LG_CT * rank_pad * (int64_t)sizeof(float);
}

int gf_lora_grad(const void* Y, int64_t ldy, const void* T, int64_t ldt, void* out, int64_t ldo, int64_t M, int64_t C, int64_t rank_pad,
                 float scale, int transposed, void* workspace, void* stream) {
    const char* fn = "gf_lora_grad";
    GF_CHECK_ARG(Y && T && out, "%s: null pointer", fn);
    GF_CHECK_ARG(M >= 0 && C > 0, "%s: bad shape M=%lld C=%lld", fn, (long long)M, (long long)C);
    GF_CHECK_ARG(rank_pad >= 32 && rank_pad <= LG_MAX_RANK && rank_pad % 32 == 0, "%s: rank_pad=%lld must be a multiple of 32 in 32..%d",
                 fn, (long long)rank_pad, LG_MAX_RANK);
    GF_CHECK_ARG(C % 8 == 0, "%s: C=%lld must be a multiple of 8", fn, (long long)C);
    GF_CHECK_ARG(transposed == 0 || transposed == 1, "%s: transposed=%d must be 0 or 1", fn, transposed);
    GF_CHECK_ARG(ldy % 8 == 0 && ldt % 8 == 0 && ldo % 8 == 0 && ldy >= C && ldt >= rank_pad && ldo >= (transposed ? C : rank_pad),
                 "%s: leading dimensions must be multiples of 8 and cover the row", fn);
    GF_CHECK_ARG(gf_aligned16(Y) && gf_aligned16(T) && gf_aligned16(out) && gf_aligned16(workspace), "%s: 16-byte alignment required", fn);
    GF_CHECK_ARG(M < (1 << 30) && C < (1 << 30), "%s: M/C too large", fn);
    GF_CHECK_ARG(scale == scale && scale - scale == 0.f, "%s: scale must be finite", fn);
    const LoraGradPlan pl = lora_grad_plan(M, C);
    GF_CHECK_ARG(M == 0 || workspace, "%s: null workspace (gf_lora_grad_workspace_bytes bytes)", fn);
    GF_CHECK_ARG(pl.ctiles * (pl.slabs ? pl.slabs : 1) < (1L << 31), "%s: %ld column tiles x %ld slabs exceed the grid", fn, pl.ctiles,
                 pl.slabs);
    hipStream_t s = (hipStream_t)stream;
    if (pl.slabs > 0) {
        LoraGradArgs a{};
        a.Y = (const u16*)Y, a.T = (const u16*)T, a.ws = (float*)workspace;
        a.ldy = ldy, a.ldt = ldt;
        a.M = (int)M, a.C = (int)C, a.cpad = (int)(pl.ctiles * LG_CT), a.ctiles = (int)pl.ctiles, a.slab_rows = (int)pl.slab_rows;
        const int nj = (int)rank_pad / 16;
        const int lds = LG_KT * LG_PY + LG_KT * ((int)rank_pad * 2 + 32);      // <= 45 056 B: below the 64 KiB a launch gets unasked
        const dim3 grid((unsigned)(pl.ctiles * pl.slabs)), block(LG_THREADS);
        const int rc = gf_dispatch<2, 4, 6, 8, 10, 12, 14, 16>(nj, [&](auto n) {
            hipLaunchKernelGGL((lora_grad_kernel<decltype(n)::value>), grid, block, lds, s, a);
            GF_CHECK_LAUNCH(fn);
            return GF_OK;
        });
        if (rc) return rc;
    }
    LoraGradSumArgs r{};
    r.ws = (const float*)workspace, r.out = (u16*)out, r.ldo = ldo;
    r.C = (int)C, r.cpad = (int)(pl.ctiles * LG_CT), r.rank_pad = (int)rank_pad, r.slabs = (int)pl.slabs;
    r.scale = scale;
    const long items = C * rank_pad / 8;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (transposed) hipLaunchKernelGGL(lora_grad_sum_kernel<true>, grid, block, 0, s, r);
    else hipLaunchKernelGGL(lora_grad_sum_kernel<false>, grid, block, 0, s, r);
    GF_CHECK_LAUNCH(fn);
    return GF_OK;
}

}  // extern "C"

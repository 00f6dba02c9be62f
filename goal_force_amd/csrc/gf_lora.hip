// gf_lora.hip — LoRA adapters (gfx950): gf_lora_merge folds one adapter into a bf16 weight in place (the reference's
// GeneralLoRALoader.load: diffsynth/lora/__init__.py), gf_lora_up adds one attached adapter's update to a layer's output (peft's
// unmerged forward, result + lora_B(lora_A(x)) * scaling, in bf16).
//
// Both are ONE pass over a [rows, cols] bf16 matrix Y (the weight W [n_out, k_in]; the layer's output y0 [M, N]) plus a product of
// rank <= 256 terms per element:
//     merge:  W[n,k]   <- bf16( W[n,k]  + bf16( alpha * bf16( sum_j up[n,j] * down[j,k] ) ) )
//     up   :  out[m,n] <- epi( bf16( y0[m,n] + bf16( scale * bf16( sum_j t[m,j] * up[n,j] ) ) ), resid, gate )
// i.e. Y[r,c] += R[r,:] . Ct[c,:] with a "row factor" R [rows, rank] (up; t) and a "column factor" Ct [cols, rank] (down^T; up).
//
// Summation order (the tests' fp32 restatement follows it): the rank is zero-padded to rank_pad = a multiple of 32; the sum runs over
// the chunks of 32 rank columns in ascending order; every output element belongs to ONE accumulator fragment, to which each chunk's 32
// products are added by one v_mfma_f32_16x16x32_bf16 (a wave holds four such fragments, so it issues four MFMAs per chunk; the
// accumulators start at +0), and nothing is rounded to bf16 before the last product is in.  Then the three
// bf16 roundings of the formula above, alpha / scale multiplied as fp32.
//
// Frame: 256 threads = 4 waves, a tile of 64 rows x 64 columns of Y per workgroup; wave w owns rows 16 w .. 16 w + 15.  The column
// factor of the tile is staged ONCE in LDS as Ct[64][rank_pad] (row pitch rank_pad + 8 elements: 16-byte fragment reads of 16
// different rows land in different banks); merge transposes `down` on the way in.  The row factor is read from global memory as the
// MFMA's B fragments, once per wave and chunk.  The MFMA runs TRANSPOSED (its 16 "rows" are columns of Y, its 16 "columns" are rows
// of Y) and the two MFMAs of a 32-column block take the columns 8 q + e (e < 4) and 8 q + 4 + e: lane l then holds the eight
// CONSECUTIVE columns 32 cb + 8 (l >> 4) .. + 7 of row (l & 15) — one 16-byte load of Y and one 16-byte store per lane and block, no
// LDS round trip for the result.
#include "gf_mfma_frame.h"

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_TILE = 64;        // rows and columns of Y per workgroup
constexpr int LR_MAX_RANK = 256;
constexpr int LR_PAD = 8;          // elements added to the LDS row pitch

struct LoraArgs {
    const u16* Y;      // W (merge) / y0 (up): [rows, ldy]
    u16* O;            // W / out: [rows, ldo]
    const u16* R;      // row factor [rows, ldrf]: up (merge) / t (up)
    const u16* Cf;     // column factor: down [rank, ldcf] (merge) / up [cols, ldcf] (up)
    const u16* resid;  // [rows, ldres] or null
    const u16* gate;   // [cols] or null
    long ldy, ldo, ldrf, ldcf, ldres;
    int rows, cols, rank, rank_pad;
    int r_vec, c_vec;  // the factor may be read in 16-byte pieces (aligned base, pitch a multiple of 8)
    float scale;
};

// eight consecutive elements p[0..7] of which the first `valid` (<= 8, may be <= 0) exist; the rest are +0
__device__ __forceinline__ u16x8 lr_load8(const u16* p, int valid, bool vec) {
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (valid >= 8 && vec) return *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < valid) v[e] = p[e];
    return v;
}

// MERGE: Cf is down [rank, cols] (transposed into LDS), no epilogue operands.  EPI: the gf_epilogue applied to y (gf_lora_up).
template <bool MERGE, int EPI>
__global__ __launch_bounds__(LR_THREADS) void lora_kernel(const LoraArgs p) {
    extern __shared__ __attribute__((aligned(16))) char lr_lds[];
    u16* ct = reinterpret_cast<u16*>(lr_lds);
    const int pitch = p.rank_pad + LR_PAD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctiles = (p.cols + LR_TILE - 1) / LR_TILE;
    const int r0 = (blockIdx.x / ctiles) * LR_TILE, c0 = (blockIdx.x % ctiles) * LR_TILE;
    const int nchunk = p.rank_pad >> 5;

    // this lane's pieces of Y (and resid): row r0 + 16 wave + (lane & 15), columns c0 + 32 cb + 8 (lane >> 4) .. + 7
    const int row = r0 + wave * 16 + (lane & 15);
    const bool row_ok = row < p.rows;
    u16x8 y8[2], res8[2], g8[2];
    constexpr bool HAS_R = !MERGE && (EPI == GF_EPI_BIAS_GATE_RESID || EPI == GF_EPI_BIAS_RESID || EPI == GF_EPI_BIAS_MUL);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int col = c0 + cb * 32 + (lane >> 4) * 8;
        const bool ok = row_ok && col < p.cols;      // cols % 8 == 0: a piece is inside or outside as a whole
        y8[cb] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) y8[cb] = *reinterpret_cast<const u16x8*>(p.Y + (long)row * p.ldy + col);
        if constexpr (HAS_R)
            if (ok) res8[cb] = *reinterpret_cast<const u16x8*>(p.resid + (long)row * p.ldres + col);
        if constexpr (!MERGE && EPI == GF_EPI_BIAS_GATE_RESID)
            if (ok) g8[cb] = *reinterpret_cast<const u16x8*>(p.gate + col);
    }

    // ---- stage the column factor: ct[c][j] = Ct[c0 + c][j], +0 where c0 + c >= cols or j >= rank
    if constexpr (MERGE) {
        // down [rank, cols]: item = (rank row j, 8-column piece q); each element goes to its own LDS row
        for (int idx = tid; idx < p.rank_pad * 8; idx += LR_THREADS) {
            const int q = idx & 7, j = idx >> 3;
            const int col = c0 + q * 8;
            const int valid = (j < p.rank && col < p.cols) ? 8 : 0;
            const u16x8 v = lr_load8(p.Cf + (long)j * p.ldcf + col, valid, p.c_vec);
#pragma unroll
            for (int e = 0; e < 8; ++e) ct[(q * 8 + e) * pitch + j] = v[e];
        }
    } else {
        // up [cols, rank]: item = (column c, 8-rank piece q)
        const int pieces = p.rank_pad >> 3;
        for (int idx = tid; idx < LR_TILE * pieces; idx += LR_THREADS) {
            const int q = idx % pieces, c = idx / pieces;
            const int valid = (c0 + c < p.cols) ? p.rank - q * 8 : 0;
            const u16x8 v = lr_load8(p.Cf + (long)(c0 + c) * p.ldcf + q * 8, valid, p.c_vec);
            *reinterpret_cast<u16x8*>(ct + c * pitch + q * 8) = v;
        }
    }

    // the row factor's first fragment: row (lane & 15) of the wave, rank columns 32 chunk + 8 (lane >> 4) .. + 7
    const u16* rrow = p.R + (long)row * p.ldrf;
    const int jl = (lane >> 4) * 8;
    u16x8 bnext = lr_load8(rrow + jl, row_ok ? p.rank - jl : 0, p.r_vec);
    __syncthreads();

    f32x4 acc[2][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[cb][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    // MFMA row i of block cb, half h = tile column 32 cb + 8 (i >> 2) + 4 h + (i & 3)
    const int i = lane & 15;
    const u16* arow = ct + (8 * (i >> 2) + (i & 3)) * pitch + jl;
    for (int ch = 0; ch < nchunk; ++ch) {
        const bf16x8 b = __builtin_bit_cast(bf16x8, bnext);
        if (ch + 1 < nchunk) {
            const int j = (ch + 1) * 32 + jl;
            bnext = lr_load8(rrow + j, row_ok ? p.rank - j : 0, p.r_vec);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + (cb * 32 + h * 4) * pitch + ch * 32);
                acc[cb][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[cb][h], 0, 0, 0);
            }
    }

    // ---- the three roundings, the epilogue, one 16-byte store per block
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int col = c0 + cb * 32 + (lane >> 4) * 8;
        if (!(row_ok && col < p.cols)) continue;
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = rbf(acc[cb][e >> 2][e & 3]);
            const float s = rbf(p.scale * d);
            const float y = rbf(bf2f(y8[cb][e]) + s);
            if constexpr (MERGE) o[e] = f2bf(y);
            else {
                float t = gf_epi_act<EPI>(y);
                if constexpr (EPI == GF_EPI_BIAS_GATE_RESID) t = rbf(bf2f(g8[cb][e]) * t);
                if constexpr (EPI == GF_EPI_BIAS_MUL) o[e] = f2bf(t * bf2f(res8[cb][e]));
                else if constexpr (HAS_R) o[e] = f2bf(bf2f(res8[cb][e]) + t);
                else o[e] = f2bf(t);
            }
        }
        *reinterpret_cast<u16x8*>(p.O + (long)row * p.ldo + col) = o;
    }
}

template <bool MERGE, int EPI>
int lora_launch(const char* fn, const LoraArgs& a, hipStream_t s) {
    const long rt = (a.rows + LR_TILE - 1) / LR_TILE, ctl = (a.cols + LR_TILE - 1) / LR_TILE;
    GF_CHECK_ARG(rt * ctl < (1L << 31), "%s: %ld x %ld tiles of 64 x 64 exceed the grid (2^31 workgroups)", fn, rt, ctl);
    const int lds = LR_TILE * (a.rank_pad + LR_PAD) * (int)sizeof(u16);   // <= 33 792 B: below the 64 KiB a launch gets unasked
    hipLaunchKernelGGL((lora_kernel<MERGE, EPI>), dim3((unsigned)(rt * ctl)), dim3(LR_THREADS), lds, s, a);
    GF_CHECK_LAUNCH(fn);
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_lora_merge(void* W, int64_t ldw, const void* up, int64_t ld_up, const void* down, int64_t ld_down, int64_t n_out,
                  int64_t k_in, int64_t rank, float alpha, void* stream) {
    const char* fn = "gf_lora_merge";
    GF_CHECK_ARG(W && up && down, "%s: null pointer", fn);
    GF_CHECK_ARG(n_out >= 0 && k_in > 0, "%s: bad shape n_out=%lld k_in=%lld", fn, (long long)n_out, (long long)k_in);
    GF_CHECK_ARG(rank >= 1 && rank <= LR_MAX_RANK, "%s: rank=%lld outside 1..%d", fn, (long long)rank, LR_MAX_RANK);
    GF_CHECK_ARG(k_in % 8 == 0, "%s: k_in=%lld must be a multiple of 8", fn, (long long)k_in);
    GF_CHECK_ARG(ldw % 8 == 0 && ldw >= k_in, "%s: ldw=%lld must be a multiple of 8 and cover the row", fn, (long long)ldw);
    GF_CHECK_ARG(ld_up >= rank && ld_down >= k_in, "%s: ld_up / ld_down must cover the row", fn);
    GF_CHECK_ARG(gf_aligned16(W), "%s: 16-byte alignment of W required", fn);
    GF_CHECK_ARG((((uintptr_t)up) & 1u) == 0 && (((uintptr_t)down) & 1u) == 0, "%s: up / down must be 2-byte aligned", fn);
    GF_CHECK_ARG(n_out < (1 << 30) && k_in < (1 << 30), "%s: n_out / k_in too large", fn);
    GF_CHECK_ARG(alpha == alpha && alpha - alpha == 0.f, "%s: alpha must be finite", fn);
    if (n_out == 0) return GF_OK;
    LoraArgs a{};
    a.Y = (const u16*)W, a.O = (u16*)W, a.R = (const u16*)up, a.Cf = (const u16*)down;
    a.ldy = a.ldo = ldw, a.ldrf = ld_up, a.ldcf = ld_down;
    a.rows = (int)n_out, a.cols = (int)k_in, a.rank = (int)rank, a.rank_pad = (int)((rank + 31) / 32 * 32);
    a.r_vec = gf_aligned16(up) && ld_up % 8 == 0, a.c_vec = gf_aligned16(down) && ld_down % 8 == 0;
    a.scale = alpha;
    return lora_launch<true, GF_EPI_BIAS>(fn, a, (hipStream_t)stream);
}

int gf_lora_up(const void* y0, int64_t ldy, const void* t, int64_t ldt, const void* up, int64_t ld_up, void* out, int64_t ldo,
               int64_t M, int64_t N, int64_t rank_pad, float scale, int epilogue, const void* resid, int64_t ldr, const void* gate,
               void* stream) {
    const char* fn = "gf_lora_up";
    GF_CHECK_ARG(y0 && t && up && out, "%s: null pointer", fn);
    GF_CHECK_ARG(M >= 0 && N > 0, "%s: bad shape M=%lld N=%lld", fn, (long long)M, (long long)N);
    GF_CHECK_ARG(rank_pad >= 32 && rank_pad <= LR_MAX_RANK && rank_pad % 32 == 0, "%s: rank_pad=%lld must be a multiple of 32 in 32..%d",
                 fn, (long long)rank_pad, LR_MAX_RANK);
    GF_CHECK_ARG(N % 8 == 0, "%s: N=%lld must be a multiple of 8", fn, (long long)N);
    GF_CHECK_ARG(ldy % 8 == 0 && ldo % 8 == 0 && ldt % 8 == 0 && ld_up % 8 == 0 && ldy >= N && ldo >= N && ldt >= rank_pad &&
                     ld_up >= rank_pad,
                 "%s: leading dimensions must be multiples of 8 and cover the row", fn);
    GF_CHECK_ARG(gf_aligned16(y0) && gf_aligned16(t) && gf_aligned16(up) && gf_aligned16(out), "%s: 16-byte alignment required", fn);
    GF_CHECK_ARG(M < (1 << 30) && N < (1 << 30), "%s: M/N too large", fn);
    GF_CHECK_ARG(scale == scale && scale - scale == 0.f, "%s: scale must be finite", fn);
    GF_CHECK_ARG(epilogue >= GF_EPI_BIAS && epilogue <= GF_EPI_BIAS_MUL, "%s: unknown epilogue %d", fn, epilogue);
    const bool need_r = epilogue == GF_EPI_BIAS_GATE_RESID || epilogue == GF_EPI_BIAS_RESID || epilogue == GF_EPI_BIAS_MUL;
    GF_CHECK_ARG(!need_r || (resid && ldr % 8 == 0 && ldr >= N && gf_aligned16(resid)),
                 "%s: residual epilogue needs an aligned resid with ldr >= N", fn);
    GF_CHECK_ARG(epilogue != GF_EPI_BIAS_GATE_RESID || (gate && gf_aligned16(gate)), "%s: gate epilogue needs an aligned gate vector", fn);
    if (M == 0) return GF_OK;
    LoraArgs a{};
    a.Y = (const u16*)y0, a.O = (u16*)out, a.R = (const u16*)t, a.Cf = (const u16*)up, a.resid = (const u16*)resid,
    a.gate = (const u16*)gate;
    a.ldy = ldy, a.ldo = ldo, a.ldrf = ldt, a.ldcf = ld_up, a.ldres = ldr;
    a.rows = (int)M, a.cols = (int)N, a.rank = (int)rank_pad, a.rank_pad = (int)rank_pad;
    a.r_vec = a.c_vec = 1;
    a.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    return gf_dispatch<GF_EPI_BIAS, GF_EPI_BIAS_GELU_TANH, GF_EPI_BIAS_GATE_RESID, GF_EPI_BIAS_RESID, GF_EPI_BIAS_SILU, GF_EPI_BIAS_MUL>(
        epilogue, [&](auto e) { return lora_launch<false, decltype(e)::value>(fn, a, s); });
}

}  // extern "C"

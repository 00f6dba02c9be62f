// gf_gemm_mxfp4.hip — OCP MXFP4 linears (include/goalforce.h, "MXFP4 Linear"): the quantiser gf_quant_mxfp4 (bf16 -> packed e2m1
// codes + one E8M0 scale per 32 k) and the block-scaled GEMM gf_gemm_mxfp4 on v_mfma_scale_f32_16x16x128_f8f6f4 with both operands
// e2m1 (cbsz = blgp = 4) and the blocks' scales in the instruction's scale operands; gf_gemm_mxfp4_q4 is that GEMM with its output
// quantised in the epilogue, for a consumer that is another fp4 Linear.
//
// The GEMM is the 8-wave one-barrier kernel of the fp8 small shapes (gf_gemm.hip, gemm_kernel<EPI, true>) with another element:
//   * 256x256 output tile per 512-thread workgroup (8 waves as 2(M) x 4(N), 128x64 per wave), fp32 accumulators;
//   * a K tile is one 128-byte LDS row = 256 e2m1 elements = 8 MX blocks = TWO MFMA k-steps of 128;
//   * tiles are staged HBM -> LDS with global_load_lds_dwordx4, double buffered, one barrier per K tile, rows clamped at the M / N tails;
//   * LDS image: 128-byte rows, 16-byte chunk index XOR (row & 7), applied to the DMA's source address and on the ds_read_b128;
//   * lane (row = lane & 15, kb = lane >> 4) reads chunk 2 kb + s in sub-step s: one 16-byte chunk = 32 k = ONE MX block, placed in the
//     low four dwords of the operand.  Both operands follow the same rule, so slot e of lane group kb pairs the same k on both;
//   * the K tile's scales (8 bytes per row) are fetched one K tile ahead, one row per thread, rows clamped like the operand rows, and handed
//     on through LDS; the lane's two E8M0 bytes (blocks 2 kb, 2 kb + 1 of its row) are ONE 16-bit LDS read per fragment row and sub-step s
//     selects byte s through opsel;
//   * operands swapped (D = W_frag x A_frag), the epilogue transposes through wave-private LDS and touches HBM with 16-byte pieces.
// NaN: an E8M0 code 255 anywhere in a row's scales makes that row of A (column of W) NaN in the output.  The instruction was observed to
// do that by itself (goalforce.h); no document says so, so the epilogue also does it from the scale bytes the K loop fetched.
// The K loop holds no branch but the one around the DMA: with the scale hand-over under an `if` the compiler rotated the accumulators
// through v_mov and spilled 29 - 63 VGPRs, and every reload waited (vmcnt) for the next tile's DMA as well: 0.77 -> 0.51 ms at
// 32760 x 5120 x 5120 once it was gone (197 VGPRs, no scratch).
#include "gf_mfma_frame.h"
#include "gf_mxfp4_quant.h"

namespace {

constexpr int BM = 256, BN = 256;
constexpr int FP4_THREADS = 512;
constexpr int TILE_BYTES = BM * 128;          // 32 KiB per operand tile: 256 rows x 256 e2m1
constexpr int STAGE_BYTES = 2 * TILE_BYTES;   // A + W
constexpr int FP4_LDS_TILES = 2 * STAGE_BYTES;           // 128 KiB
constexpr int FP4_LDS = FP4_LDS_TILES + 2 * 4096 + 512;  // + two buffers of a K tile's scales (256 + 256 rows x 8 B) + the rows' NaN flags
constexpr int GROUP_M = 8;

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct Fp4Args {
    const char* A = nullptr;
    const char* W = nullptr;
    const unsigned char* sa = nullptr;
    const unsigned char* sw = nullptr;
    const u16* bias = nullptr;
    u16* C = nullptr;
    const u16* R = nullptr;
    const u16* gate = nullptr;
    int M = 0, N = 0, K = 0;
    long lda = 0, ldw = 0, lsa = 0, lsw = 0, ldc = 0, ldr = 0;
    int tiles_m = 0, tiles_n = 0;
    // Q4 (gf_gemm_mxfp4_q4): the output as the next GEMM's A operand instead of C — packed codes [M, N/2] and scales [M, N/32], strides in bytes
    unsigned char* C4 = nullptr;
    unsigned char* sc = nullptr;
    long ldc4 = 0, lsc = 0;
};

// Q4: the finished bf16 output is quantised to MXFP4 in the read-back loop (gf_mxfp4_quant.h) and only its codes and scales are stored:
// a lane of that loop holds 8 consecutive columns of one row and lanes cc = 0..3 / 4..7 are the two 32-aligned MX blocks of the wave's
// 64 columns — the quantiser's own arrangement.  Epilogues without a second operand only.
template <int EPI, bool Q4 = false>
__global__ __launch_bounds__(FP4_THREADS, 2) void gemm_mxfp4_kernel(const Fp4Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    GF_LDS char* lds = (GF_LDS char*)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- XCD-aware tile mapping (bijective for any grid size) ------------------------------
    const int v = gf_xcd_tile_order(p.tiles_m * p.tiles_n);
    const int per_group = GROUP_M * p.tiles_n;
    const int group = v / per_group;
    const int first_m = group * GROUP_M;
    const int gsz = min(p.tiles_m - first_m, GROUP_M);
    const int in_group = v - group * per_group;
    const int tile_m = first_m + in_group % gsz;
    const int tile_n = in_group / gsz;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int m_last = p.M - 1 - m0, n_last = p.N - 1 - n0;   // the last row of either operand that exists, relative to the tile

    // ---- staging addresses: wave w issues row-groups g = 4w..4w+3 (8 rows x 128 B each) -------
    // lane l of a DMA instruction fills LDS chunk (l&7) of row (l>>3); it must hold the logical chunk (l&7) ^ (row&7) of that row.
    // Offsets are relative to the tile's first row and 32 bits wide (gf_gemm_mxfp4 refuses operands they cannot cover).
    const char* a_tile = p.A + (long)m0 * p.lda;
    const char* w_tile = p.W + (long)n0 * p.ldw;
    const int srow = lane >> 3;
    const int schunk = (lane & 7) ^ srow;
    unsigned a_off[4], b_off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + srow;
        a_off[i] = (unsigned)min(row, m_last) * (unsigned)p.lda + (unsigned)(schunk * 16);
        b_off[i] = (unsigned)min(row, n_last) * (unsigned)p.ldw + (unsigned)(schunk * 16);
    }
    auto stage = [&](int buf, int kt) {
        GF_LDS char* sa = lds + buf * STAGE_BYTES + wave * 4096;
        GF_LDS char* sb = sa + TILE_BYTES;
        const unsigned koff = (unsigned)kt * 128u;  // bytes along K
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            glds16(a_tile + (a_off[i] + koff), sa + i * 1024);
            glds16(w_tile + (b_off[i] + koff), sb + i * 1024);
        }
    };

    // ---- fragment read addresses ---------------------------------------------------------------
    const int wm = wave >> 2, wn = wave & 3;
    const int frow = lane & 15;   // row inside a 16-row fragment
    const int fq = lane >> 4;     // k group of the row: MX blocks 2 fq, 2 fq + 1 of the K tile
    const int sw = frow & 7;      // row & 7 of every fragment row of this lane (the fragment bases are multiples of 16)
    const int a_base = (wm * 128 + frow) * 128;
    const int b_base = TILE_BYTES + (wn * 64 + frow) * 128;

    // ---- scales: 8 E8M0 bytes per row and K tile.  Thread t fetches them for one row (t < 256: row t of the A tile, else row t - 256
    // of the W tile; rows clamped like the operand rows), one K tile ahead and into registers, and hands them on through LDS:
    // image [2 buffers][A rows 0..255 | W rows 0..255][8 bytes] behind the operand stages.  It also watches them for code 255.
    const bool s_is_a = wave < 4;     // wave-uniform
    const int s_row = tid & 255;
    const unsigned char* s_src = s_is_a ? p.sa + ((long)m0 + min(s_row, m_last)) * p.lsa : p.sw + ((long)n0 + min(s_row, n_last)) * p.lsw;
    GF_LDS char* sc_lds = lds + FP4_LDS_TILES;
    const int s_dst = (s_is_a ? 0 : 2048) + s_row * 8;
    auto ld_scale8 = [&](int kt) {   // any alignment
        u32x2 r;
        __builtin_memcpy(&r, s_src + (long)kt * 8, 8);
        return r;
    };
    unsigned row_nan_seen = 0;
    auto watch = [&](u32x2 r) {      // a byte 0xFF in r <=> a zero byte in ~r
        const unsigned y0 = ~r[0], y1 = ~r[1];
        row_nan_seen |= ((y0 - 0x01010101u) & ~y0 & 0x80808080u) | ((y1 - 0x01010101u) & ~y1 & 0x80808080u);
    };
    // this lane's two bytes of a fragment row: blocks 2 fq, 2 fq + 1
    const int sa_rd = (wm * 128 + frow) * 8 + 2 * fq;
    const int sw_rd = 2048 + (wn * 64 + frow) * 8 + 2 * fq;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / 256;
    {
        const u32x2 s0 = ld_scale8(0);
        watch(s0);
        *(GF_LDS u32x2*)(sc_lds + s_dst) = s0;
    }
    // the scales run two K tiles ahead in a register pair and one ahead in LDS, without a branch: past the last tile the last one is
    // fetched and handed on again, which nobody reads
    u32x2 s_nxt = ld_scale8(min(1, nk - 1));
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // tile kt and its scales landed for every wave; everyone is done reading the other buffers
        watch(s_nxt);
        *(GF_LDS u32x2*)(sc_lds + ((kt + 1) & 1) * 4096 + s_dst) = s_nxt;      // tile kt + 1's, read after the next barrier
        s_nxt = ld_scale8(min(kt + 2, nk - 1));
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        GF_LDS char* sbuf = lds + (kt & 1) * STAGE_BYTES;
        GF_LDS char* scb = sc_lds + (kt & 1) * 4096;
        unsigned sca[8], scw[4];      // the K tile's scale pairs of this lane's fragment rows
#pragma unroll
        for (int i = 0; i < 8; ++i) sca[i] = *(GF_LDS unsigned short*)(scb + sa_rd + i * 128);
#pragma unroll
        for (int j = 0; j < 4; ++j) scw[j] = *(GF_LDS unsigned short*)(scb + sw_rd + j * 128);
        gf_static_for<0, 2>([&](auto s_) {
            constexpr int S = decltype(s_)::value;      // sub-step: MX block 2 fq + S of the row, scale byte S of the pair
            const int c = ((2 * fq + S) ^ sw) << 4;
            i32x8 bfr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 lo = *(GF_LDS u32x4*)(sbuf + b_base + j * 2048 + c);
                bfr[j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], 0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const u32x4 lo = *(GF_LDS u32x4*)(sbuf + a_base + i * 2048 + c);
                const i32x8 af = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], 0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j)   // swapped operands: D[n-local][m-local]; lane holds 4 consecutive n of one m
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bfr[j], af, acc[i][j], 4, 4, S, (int)scw[j], S, (int)sca[i]);
            }
            // a fence for the compiler's memory operations: the second sub-step's 12 fragment reads are not hoisted in front of the
            // first one's (24 fragments = 96 VGPRs beside the 128 accumulators)
            if constexpr (S == 0) asm volatile("" ::: "memory");
        });
    }

    // ---- NaN scales: one flag byte per row of the A tile and of the W tile, behind the scale buffers
    GF_LDS unsigned char* nanf = (GF_LDS unsigned char*)(sc_lds + 8192);
    nanf[(s_is_a ? 0 : 256) + s_row] = row_nan_seen ? 1 : 0;

    // ---- epilogue -----------------------------------------------------------------------------
    // acc[i][j][r] = C[m = m0 + wm*128 + i*16 + (lane&15)][n = n0 + wn*64 + j*16 + (lane>>4)*4 + r]
    __syncthreads();  // all waves finished reading the stage buffers; the NaN flags are written
    GF_LDS char* ep = lds + wave * 16384;  // private 128 rows x 128 B (64 bf16) per wave
    {
        const float qnan = __builtin_nanf("");
        unsigned nan_a = 0;      // bit i: fragment row i of this lane
#pragma unroll
        for (int i = 0; i < 8; ++i) nan_a |= (unsigned)nanf[wm * 128 + i * 16 + frow] << i;
        unsigned nan_col[4];     // [j] byte r: column j*16 + fq*4 + r of this wave's 64
#pragma unroll
        for (int j = 0; j < 4; ++j) nan_col[j] = *(GF_LDS unsigned*)(nanf + 256 + wn * 64 + j * 16 + fq * 4);
        const int nb = n0 + wn * 64 + fq * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            const int n = nb + j * 16;
            if (p.bias && n < p.N) {  // N % 8 == 0 so n..n+3 are all valid
                const u16x4 b4 = *reinterpret_cast<const u16x4*>(p.bias + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) bv[r] = bf2f(b4[r]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float y[4];
                const bool row_nan = (nan_a >> i) & 1u;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool is_nan = row_nan || ((nan_col[j] >> (8 * r)) & 1u);
                    y[r] = gf_epi_act<EPI>(is_nan ? qnan : acc[i][j][r] + bv[r]);
                }
                u32x2 pk;
                pk[0] = pack2bf(y[0], y[1]);
                pk[1] = pack2bf(y[2], y[3]);
                const int row = i * 16 + frow;
                const int slot = (j * 4 + fq) ^ ((row & 7) << 1);  // 8-byte slot, pairs stay together
                *(GF_LDS u32x2*)(ep + row * 128 + slot * 8) = pk;
            }
        }
    }
    // each wave reads back only its own region: no workgroup barrier needed, only the LDS wait
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    {
        const int rr = lane >> 3, cc = lane & 7;
        const int n = n0 + wn * 64 + cc * 8;
        const bool n_ok = n < p.N;
        u16x8 g8;
        if (EPI == GF_EPI_BIAS_GATE_RESID && n_ok) g8 = *reinterpret_cast<const u16x8*>(p.gate + n);
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            const int row = it * 8 + rr;
            const int m = m0 + wm * 128 + row;
            const u16x8 yv = *(GF_LDS u16x8*)(ep + row * 128 + ((cc ^ (row & 7)) << 4));
            if constexpr (Q4) {
                int code;       // the block step shuffles: in front of the tail branch; N % 32 == 0, so a block's four lanes share n_ok
                const unsigned packed = mxfp4_block_step(yv, code);
                if (m < p.M && n_ok) {
                    *reinterpret_cast<unsigned*>(p.C4 + (long)m * p.ldc4 + (n >> 1)) = packed;
                    if ((cc & 3) == 0) p.sc[(long)m * p.lsc + (n >> 5)] = (unsigned char)code;
                }
            } else if (m < p.M && n_ok) {
                u16x8 o = yv;
                if (EPI == GF_EPI_BIAS_GATE_RESID || EPI == GF_EPI_BIAS_RESID || EPI == GF_EPI_BIAS_MUL) {
                    const u16x8 r8 = *reinterpret_cast<const u16x8*>(p.R + (long)m * p.ldr + n);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float t = bf2f(yv[e]);
                        if (EPI == GF_EPI_BIAS_GATE_RESID) t = rbf(bf2f(g8[e]) * t);  // gate * residual
                        o[e] = (EPI == GF_EPI_BIAS_MUL) ? f2bf(t * bf2f(r8[e]))       // fc1(x) * gelu(gate(x))
                                                        : f2bf(bf2f(r8[e]) + t);      // x + ...
                    }
                }
                *reinterpret_cast<u16x8*>(p.C + (long)m * p.ldc + n) = o;
            }
        }
    }
}

// ---- the quantiser: thread = 8 consecutive elements (one 16-byte load), four neighbouring lanes = one MX block ---------------------
// The block step itself is gf_mxfp4_quant.h's, shared with the two producers that quantise in registers.
__global__ __launch_bounds__(256) void quant_mxfp4_kernel(const u16* __restrict__ x, long x_stride, unsigned char* __restrict__ out4,
                                                          long out_stride, unsigned char* __restrict__ scales, long scale_stride,
                                                          long total, int cpr) {
    const long g0 = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = g0 < total;           // total is a multiple of 4: the four lanes of a block are live together
    const long g = live ? g0 : total - 1;
    const long row = g / cpr;
    const int c = (int)(g - row * cpr);
    const u16x8 xv = *reinterpret_cast<const u16x8*>(x + row * x_stride + (long)c * 8);
    int code;
    const unsigned packed = mxfp4_block_step(xv, code);      // every lane: a dead one re-does the last piece
    if (live) {
        *reinterpret_cast<unsigned*>(out4 + row * out_stride + (long)c * 4) = packed;
        if ((c & 3) == 0) scales[row * scale_stride + (c >> 2)] = (unsigned char)code;
    }
}

template <int EPI, bool Q4>
int launch_mxfp4(const char* fn, const Fp4Args& a, hipStream_t stream) {
    return gf_launch_lds<gemm_mxfp4_kernel<EPI, Q4>>(fn, GF_ATTR_MSG_BYTES, fn, dim3((unsigned)(a.tiles_m * a.tiles_n)), dim3(FP4_THREADS),
                                                      FP4_LDS, stream, a);
}

// The operand rules gf_gemm_mxfp4 and gf_gemm_mxfp4_q4 share, in the order both have always answered in.  The output is the one operand
// that differs (q4: packed codes C4 [M, N/2] with ldo in bytes and scales c_scale [M, N/32]; else bf16 C [M, N] with ldo in elements), and
// its rules sit between the shared ones, so they are stated here too; what follows the operands (resid / gate, the epilogue) is the caller's.
int mxfp4_check(const char* fn, bool q4, const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw,
                const void* w_scale, int64_t w_scale_stride, const void* bias, const void* out, int64_t ldo, const void* c_scale,
                int64_t c_scale_stride, int64_t M, int64_t N, int64_t K) {
    GF_CHECK_ARG(A4 && W4 && out && (!q4 || c_scale) && a_scale && w_scale, "%s: null A/W/C/scales", fn);
    GF_CHECK_ARG(M >= 0 && N > 0 && K > 0, "%s: bad sizes M=%ld N=%ld K=%ld", fn, (long)M, (long)N, (long)K);
    GF_CHECK_ARG(K % 256 == 0, "%s: K=%ld must be a multiple of %d", fn, (long)K, 256);
    GF_CHECK_ARG(N % (q4 ? 32 : 8) == 0, "%s: N=%ld must be a multiple of %s", fn, (long)N, q4 ? "32 (one E8M0 scale per 32 output columns)" : "8");
    GF_CHECK_ARG(lda % 16 == 0 && ldw % 16 == 0 && lda >= K / 2 && ldw >= K / 2 && (q4 ? ldo % 16 == 0 && ldo >= N / 2 : ldo % 8 == 0 && ldo >= N),
                 "%s: leading dimensions must be multiples of %d %s and cover the row", fn, 16, q4 ? "(A/W/C4, in bytes)" : "(A/W) / 8 (C)");
    GF_CHECK_ARG(a_scale_stride >= K / 32 && w_scale_stride >= K / 32, "%s: scale strides must cover K/32 = %ld blocks", fn, (long)(K / 32));
    GF_CHECK_ARG(!q4 || c_scale_stride >= N / 32, "%s: c_scale_stride must cover N/32 = %ld blocks", fn, (long)(N / 32));
    GF_CHECK_ARG(gf_aligned16(A4) && gf_aligned16(W4) && gf_aligned16(out) && (!bias || gf_aligned16(bias)),
                 "%s: 16-byte alignment required", fn);
    GF_CHECK_ARG(M < (1 << 30) && N < (1 << 30), "%s: M/N too large", fn);
    GF_CHECK_ARG(256L * lda + K / 2 < (1L << 31) && 256L * ldw + K / 2 < (1L << 31) && 256L * a_scale_stride + K / 32 < (1L << 31) &&
                     256L * w_scale_stride + K / 32 < (1L << 31),
                 "%s: operand too large for 32-bit staging offsets", fn);
    return GF_OK;
}

// The one place an Fp4Args is filled: the operands both entries share; the output (C / R / gate, or C4 / sc) is set by the caller.
Fp4Args mxfp4_args(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw, const void* w_scale,
                   int64_t w_scale_stride, const void* bias, int64_t M, int64_t N, int64_t K) {
    Fp4Args a;
    a.A = (const char*)A4;
    a.W = (const char*)W4;
    a.sa = (const unsigned char*)a_scale;
    a.sw = (const unsigned char*)w_scale;
    a.bias = (const u16*)bias;
    a.M = (int)M;
    a.N = (int)N;
    a.K = (int)K;
    a.lda = lda;
    a.ldw = ldw;
    a.lsa = a_scale_stride;
    a.lsw = w_scale_stride;
    a.tiles_m = (int)((M + BM - 1) / BM);
    a.tiles_n = (int)((N + BN - 1) / BN);
    return a;
}

}  // namespace

extern "C" GF_API int gf_quant_mxfp4(const void* x, int64_t x_stride, void* out4, int64_t out_stride, void* scales, int64_t scale_stride,
                                     int64_t rows, int64_t dim, void* stream) {
    GF_CHECK_ARG(x && out4 && scales && rows >= 0, "gf_quant_mxfp4: null pointer");
    GF_CHECK_ARG(dim > 0 && dim % 32 == 0, "gf_quant_mxfp4: dim=%ld must be a multiple of 32", (long)dim);
    GF_CHECK_ARG(x_stride % 8 == 0 && x_stride >= dim && out_stride % 4 == 0 && out_stride >= dim / 2 && scale_stride >= dim / 32,
                 "gf_quant_mxfp4: strides must be multiples of 8 (x) / 4 (out4) and cover the row");
    GF_CHECK_ARG(gf_aligned16(x) && (((uintptr_t)out4) & 3u) == 0, "gf_quant_mxfp4: alignment");
    GF_CHECK_ARG(rows < (1LL << 31) && rows * (dim / 8) < (1LL << 39), "gf_quant_mxfp4: rows x dim too large");
    if (rows == 0) return GF_OK;
    const long total = rows * (dim / 8);
    hipLaunchKernelGGL(quant_mxfp4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u16*)x,
                       (long)x_stride, (unsigned char*)out4, (long)out_stride, (unsigned char*)scales, (long)scale_stride, total,
                       (int)(dim / 8));
    GF_CHECK_LAUNCH("gf_quant_mxfp4");
    return GF_OK;
}

extern "C" GF_API int gf_gemm_mxfp4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw,
                                    const void* w_scale, int64_t w_scale_stride, const void* bias, void* C, int64_t ldc, int64_t M,
                                    int64_t N, int64_t K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream) {
    const char* fn = "gf_gemm_mxfp4";
    if (const int rc = mxfp4_check(fn, false, A4, lda, a_scale, a_scale_stride, W4, ldw, w_scale, w_scale_stride, bias, C, ldc, nullptr, 0, M, N, K))
        return rc;
    const bool need_r = epilogue == GF_EPI_BIAS_GATE_RESID || epilogue == GF_EPI_BIAS_RESID || epilogue == GF_EPI_BIAS_MUL;
    GF_CHECK_ARG(!need_r || (resid && ldr % 8 == 0 && ldr >= N && gf_aligned16(resid)),
                 "%s: residual epilogue needs an aligned resid with ldr >= N", fn);
    GF_CHECK_ARG(epilogue != GF_EPI_BIAS_GATE_RESID || (gate && gf_aligned16(gate)),
                 "%s: gate epilogue needs an aligned gate vector", fn);
    GF_CHECK_ARG(epilogue >= GF_EPI_BIAS && epilogue <= GF_EPI_BIAS_MUL, "%s: unknown epilogue %d", fn, epilogue);
    if (M == 0) return GF_OK;
    Fp4Args a = mxfp4_args(A4, lda, a_scale, a_scale_stride, W4, ldw, w_scale, w_scale_stride, bias, M, N, K);
    a.C = (u16*)C;
    a.R = (const u16*)resid;
    a.gate = (const u16*)gate;
    a.ldc = ldc;
    a.ldr = ldr;
    return gf_dispatch<GF_EPI_BIAS, GF_EPI_BIAS_GELU_TANH, GF_EPI_BIAS_GATE_RESID, GF_EPI_BIAS_RESID, GF_EPI_BIAS_SILU, GF_EPI_BIAS_MUL>(
        epilogue, [&](auto e) { return launch_mxfp4<decltype(e)::value, false>(fn, a, (hipStream_t)stream); });
}

extern "C" GF_API int gf_gemm_mxfp4_q4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw,
                                       const void* w_scale, int64_t w_scale_stride, const void* bias, void* C4, int64_t ldc4, void* c_scale,
                                       int64_t c_scale_stride, int64_t M, int64_t N, int64_t K, int epilogue, void* stream) {
    const char* fn = "gf_gemm_mxfp4_q4";
    if (const int rc = mxfp4_check(fn, true, A4, lda, a_scale, a_scale_stride, W4, ldw, w_scale, w_scale_stride, bias, C4, ldc4, c_scale,
                                   c_scale_stride, M, N, K))
        return rc;
    GF_CHECK_ARG(epilogue >= GF_EPI_BIAS && epilogue <= GF_EPI_BIAS_MUL, "%s: unknown epilogue %d", fn, epilogue);
    GF_CHECK_ARG(epilogue == GF_EPI_BIAS || epilogue == GF_EPI_BIAS_GELU_TANH || epilogue == GF_EPI_BIAS_SILU,
                 "%s: epilogue %d takes a second operand; the quantising epilogue serves GF_EPI_BIAS, GF_EPI_BIAS_GELU_TANH and "
                 "GF_EPI_BIAS_SILU (use gf_gemm_mxfp4 + gf_quant_mxfp4)", fn, epilogue);
    if (M == 0) return GF_OK;
    Fp4Args a = mxfp4_args(A4, lda, a_scale, a_scale_stride, W4, ldw, w_scale, w_scale_stride, bias, M, N, K);
    a.C4 = (unsigned char*)C4;
    a.sc = (unsigned char*)c_scale;
    a.ldc4 = ldc4;
    a.lsc = c_scale_stride;
    return gf_dispatch<GF_EPI_BIAS, GF_EPI_BIAS_GELU_TANH, GF_EPI_BIAS_SILU>(
        epilogue, [&](auto e) { return launch_mxfp4<decltype(e)::value, true>(fn, a, (hipStream_t)stream); });
}

// gf_block_map.hip — mass-cover block maps built on the device from q and k (the recipe is stated in include/goalforce.h):
// pooled means per query block / key tile, pooled scores in the log2 domain, per (head, query block) the smallest top set of tiles
// whose estimated softmax mass reaches tau, written as the CSR map gf_flash_attn_fwd_vt32_sparse reads.  Five small kernels on the
// caller's stream, no host read, no atomics: every sum has ONE order (a lane's own elements in index order, the wave's xor
// butterfly, the waves in wave order), so two calls on the same operands give the same bits.  The gated entries add the coherence of
// every block (step 1b, on the pooling pass's own loads) and refuse to predict for incoherent query blocks and key tiles (step 3).
#include "gf_common.h"

namespace {

constexpr int BM_QB = 256, BM_KB = 64;      // query rows per map row, keys per map column (kernel 3's workgroup and key tile)
constexpr int BM_MAX_TILES = 1024;          // the selection keeps a row's tiles in the registers of one 256-thread workgroup
constexpr int BM_THREADS = 256;

static inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }
__device__ __forceinline__ bool bm_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------------------------------------------------------- 1. pooling
// mean[h][b][c] = (sum over the rows of block b that exist of x[row][h*128 + c]) / their count.  One workgroup per (block, head):
// 16 lanes read one row's 128 channels as 8 bf16 each, the 16 row groups of the workgroup walk the block's rows 16 apart.
// Order of the sum: a lane's rows in ascending order; row groups g ^ 1, g ^ 2 (xor butterfly inside the wave); waves 0, 1, 2, 3.
template <int BLOCK>
__global__ __launch_bounds__(BM_THREADS) void block_means_kernel(const u16* __restrict__ x, int64_t ldx, float* __restrict__ mean,
                                                                 int rows, int n_blocks) {
    __shared__ float red[4][16][8];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    const int r0 = b * BLOCK, n = min(BLOCK, rows - r0);
    const u16* src = x + (int64_t)r0 * ldx + h * 128 + cg * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = rg; i < n; i += 16) {
        const u16x8 v = *reinterpret_cast<const u16x8*>(src + (int64_t)i * ldx);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += bf2f(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc[j] += __shfl_xor(acc[j], 16);
        acc[j] += __shfl_xor(acc[j], 32);
    }
    if ((tid & 63) < 16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[tid >> 6][cg][j] = acc[j];
    }
    __syncthreads();
    if (tid < 128) {
        const int g = tid >> 3, j = tid & 7;
        const float s = ((red[0][g][j] + red[1][g][j]) + red[2][g][j]) + red[3][g][j];
        mean[((int64_t)h * n_blocks + b) * 128 + tid] = s / (float)n;
    }
}

// ------------------------------------------------------------------------------------------------------------ 1b. coherence
// block_means_kernel with one more accumulator per lane on the same loads: rho = |mean|^2 / e, e = (sum over the block's rows of
// |x_i|^2) / their count — 1 when the rows are equal, 1 / n for orthogonal rows of one norm, 0 when they cancel.  The means are
// summed in block_means_kernel's order and have its bits.  Order of e's sum: per lane the fma chain e = fma(x, x, e) over the row's 8
// channels, rows ascending; the 16 channel-group lanes cg ^ 1, ^ 2, ^ 4, ^ 8; row groups g ^ 1, g ^ 2; waves 0, 1, 2, 3; / count.
// |mean|^2 from the finished fp32 means: lane l of wave 0 forms fma(m[l + 64], m[l + 64], m[l] * m[l]), then l ^ 1, ^ 2, .. ^ 32.
// e == 0 (every row zero: all rows are equal) gives 1; a non-finite e or quotient (non-finite input, or finite input whose squares
// overflow fp32 — conservative) is written as NaN, which the gate's `!(rho >= min)` counts as incoherent.
template <int BLOCK>
__global__ __launch_bounds__(BM_THREADS) void block_means_coh_kernel(const u16* __restrict__ x, int64_t ldx, float* __restrict__ mean,
                                                                     float* __restrict__ coh, int rows, int n_blocks) {
    __shared__ float red[4][16][8];
    __shared__ float ered[4];
    __shared__ float ml[128];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    const int r0 = b * BLOCK, n = min(BLOCK, rows - r0);
    const u16* src = x + (int64_t)r0 * ldx + h * 128 + cg * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float e = 0.f;
#pragma unroll 4
    for (int i = rg; i < n; i += 16) {
        const u16x8 v = *reinterpret_cast<const u16x8*>(src + (int64_t)i * ldx);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = bf2f(v[j]);
            acc[j] += f;
            e = __builtin_fmaf(f, f, e);
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) e += __shfl_xor(e, o);
    e += __shfl_xor(e, 16);
    e += __shfl_xor(e, 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc[j] += __shfl_xor(acc[j], 16);
        acc[j] += __shfl_xor(acc[j], 32);
    }
    if ((tid & 63) < 16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[tid >> 6][cg][j] = acc[j];
    }
    if ((tid & 63) == 0) ered[tid >> 6] = e;
    __syncthreads();
    if (tid < 128) {
        const int g = tid >> 3, j = tid & 7;
        const float s = ((red[0][g][j] + red[1][g][j]) + red[2][g][j]) + red[3][g][j];
        const float m = s / (float)n;
        mean[((int64_t)h * n_blocks + b) * 128 + tid] = m;
        ml[tid] = m;
    }
    __syncthreads();
    if (tid < 64) {
        const float lo = ml[tid], hi = ml[tid + 64];
        float p = __builtin_fmaf(hi, hi, lo * lo);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) p += __shfl_xor(p, o);
        if (tid == 0) {
            const float en = (((ered[0] + ered[1]) + ered[2]) + ered[3]) / (float)n;
            float rho = 1.0f;
            if (en != 0.f) {
                rho = p / en;
                if (!bm_finite(en) || !bm_finite(rho)) rho = __builtin_nanf("");
            }
            coh[(int64_t)h * n_blocks + b] = rho;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- 2. scores
// s[h][b][t] = fma(c, dot, log2(n_keys(t))), dot = the fma chain over d = 0 .. 127 from 0.  One workgroup per (64 tiles, head): the
// tiles' means sit in LDS (row pitch 129 floats: lane t reads bank (t + d) % 64), wave w takes the query blocks w, w + 4, ...
constexpr int SC_TILES = 64, SC_PITCH = 129;
__global__ __launch_bounds__(BM_THREADS) void block_scores_kernel(const float* __restrict__ qm, const float* __restrict__ km,
                                                                  float* __restrict__ scores, int n_qb, int n_t, int kv_len, float c) {
    __shared__ float kl[SC_TILES * SC_PITCH];
    const int t0 = blockIdx.x * SC_TILES, h = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < SC_TILES * 128; i += BM_THREADS) {
        const int tl = i >> 7, d = i & 127;
        kl[tl * SC_PITCH + d] = t0 + tl < n_t ? km[((int64_t)h * n_t + t0 + tl) * 128 + d] : 0.f;
    }
    __syncthreads();
    const int tl = tid & 63, t = t0 + tl;
    if (t >= n_t) return;
    const int nk = min(BM_KB, kv_len - t * BM_KB);
    const float lg = nk == BM_KB ? 6.0f : log2f((float)nk);
    const float* kp = kl + tl * SC_PITCH;
    for (int b = tid >> 6; b < n_qb; b += 4) {
        const float* qp = qm + ((int64_t)h * n_qb + b) * 128;
        float dot = 0.f;
#pragma unroll 16
        for (int d = 0; d < 128; ++d) dot = __builtin_fmaf(qp[d], kp[d], dot);
        scores[((int64_t)h * n_qb + b) * n_t + t] = __builtin_fmaf(c, dot, lg);
    }
}

// -------------------------------------------------------------------------------------------------------------- 3. selection
// block-wide integer sum, fp32 maximum and 64-bit maximum in the shape of gf_common.h's block_sum (256 threads)
__device__ __forceinline__ int bm_block_isum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float bm_block_fmax(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ unsigned long long bm_block_umax(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) m = red[i] > m ? red[i] : m;
    return m;
}

// One workgroup per row r = h * n_qb + b; thread i holds the tiles 4 i .. 4 i + 3.  Writes counts[r], the selection as a bitmask
// bits[r][n_words] (bit t % 32 of word t / 32) and, when asked, the estimated kept share.
// GATED (gf_block_map_select_gated; the ungated instantiation is the code it was): a row whose query block is incoherent,
// !(q_coh[r] >= q_min), takes the path of a non-finite score; a tile with !(k_coh[h][t] >= k_min) is one more forced tile of every row
// of head h — each thread reads the coherences of its own four tiles.  `!(>=)`: a NaN coherence fires.  A null q_coh / k_coh: no gate.
template <bool GATED>
__global__ __launch_bounds__(BM_THREADS) void block_select_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ forced,
                                                                  int32_t* __restrict__ counts, uint32_t* __restrict__ bits,
                                                                  float* __restrict__ kept, int n_qb, int n_t, int n_words, float mass,
                                                                  const float* __restrict__ q_coh, const float* __restrict__ k_coh,
                                                                  float q_min, float k_min) {
    __shared__ float fred[4];
    __shared__ int ired[4];
    __shared__ unsigned long long ured[4];
    const int r = blockIdx.x, tid = threadIdx.x, b = r % n_qb;
    const float* sp = scores + (int64_t)r * n_t;
    float s[4], w[4];
    bool valid[4], forc[4], sel[4];
    uint32_t fword = 0;
    if (forced != nullptr && (tid >> 3) < n_words) fword = forced[(int64_t)b * n_words + (tid >> 3)];
    bool bad = false;
    float m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = tid * 4 + j;
        valid[j] = t < n_t;
        s[j] = valid[j] ? sp[t] : 0.f;
        forc[j] = valid[j] && ((fword >> ((tid & 7) * 4 + j)) & 1u);
        bad = bad || !bm_finite(s[j]);
        if (valid[j]) m = fmaxf(m, s[j]);
    }
    if constexpr (GATED) {
        if (k_coh != nullptr) {
            const float* kc = k_coh + (int64_t)(r / n_qb) * n_t;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (valid[j] && !(kc[tid * 4 + j] >= k_min)) forc[j] = true;
        }
        if (q_coh != nullptr && !(q_coh[r] >= q_min)) bad = true;      // the same value in every thread of the row
    }
    const bool full = __syncthreads_or(bad) || !(mass < 1.0f);      // a non-finite score, or tau >= 1 (a NaN tau too): every tile
    float share = 1.0f;
    int count = n_t;
    if (full) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sel[j] = valid[j];
    } else {
        // the row maximum (all scores finite here; the order of a maximum does not matter)
        const float M = bm_block_fmax(m, fred);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = valid[j] ? exp2f(s[j] - M) : 0.f;
        const float W = block_sum<BM_THREADS>(((w[0] + w[1]) + w[2]) + w[3], fred);
        const float target = mass * W;
        // G(theta) = the sum, in that one order, of w over the forced tiles and the tiles with w >= theta: not increasing in theta
        // (fp32 addition is monotone in each term), so the largest theta with G >= target is found by bisection on w's bit pattern
        auto G = [&](uint32_t theta) {
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = (forc[j] || (valid[j] && __float_as_uint(w[j]) >= theta)) ? w[j] : 0.f;
            return block_sum<BM_THREADS>(((p[0] + p[1]) + p[2]) + p[3], fred);
        };
        uint32_t lo = 0u, hi = 0x3f800001u;                         // w <= 1: nothing but the forced tiles passes hi
        if (G(hi) >= target) {
            lo = hi;                                                // the forced tiles alone reach the mass
        } else {
            while (hi - lo > 1u) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (G(mid) >= target) lo = mid; else hi = mid;
            }
        }
        int mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sel[j] = forc[j] || (valid[j] && __float_as_uint(w[j]) >= lo);
            mine += sel[j] ? 1 : 0;
        }
        count = bm_block_isum(mine, ired);
        // the two-tile floor: the largest unselected w, the lowest index on ties (n_t >= 2, so there is one)
        while (count < 2) {
            unsigned long long best = 0ull;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (valid[j] && !sel[j]) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(w[j]) << 32) | (uint32_t)(0x7fffffff - (tid * 4 + j));
                    best = key > best ? key : best;
                }
            best = bm_block_umax(best, ured);
            const int pick = 0x7fffffff - (int)(uint32_t)best;
            if ((pick >> 2) == tid) sel[pick & 3] = true;
            ++count;
        }
        if (kept != nullptr) {
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = sel[j] ? w[j] : 0.f;
            share = block_sum<BM_THREADS>(((p[0] + p[1]) + p[2]) + p[3], fred) / W;
        }
    }
    // 8 threads x 4 tiles = one 32-bit word
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= (sel[j] ? 1u : 0u) << ((tid & 7) * 4 + j);
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    if ((tid & 7) == 0 && (tid >> 3) < n_words) bits[(int64_t)r * n_words + (tid >> 3)] = word;
    if (tid == 0) {
        counts[r] = count;
        if (kept != nullptr) kept[r] = share;
    }
}

// --------------------------------------------------------------------------------------------------------------- 4. CSR emit
// row_ptr[0] = 0, row_ptr[i + 1] = counts[0] + .. + counts[i]: one workgroup of 1024 threads walks the counts 1024 at a time with a
// running carry; head_map[h] = h.
__global__ __launch_bounds__(1024) void block_scan_kernel(const int32_t* __restrict__ counts, int32_t* __restrict__ row_ptr,
                                                          int32_t* __restrict__ head_map, int n_rows, int heads) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n_rows; base += 1024) {
        const int i = base + tid;
        int v = i < n_rows ? counts[i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            before += k < wave ? wsum[k] : 0;
            total += wsum[k];
        }
        if (i < n_rows) row_ptr[i + 1] = carry + before + v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) row_ptr[0] = 0;
    for (int h = tid; h < heads; h += 1024) head_map[h] = h;
}

// tile_idx of row r from its bitmask, ascending: one wave per row, lane l owns word l
__global__ __launch_bounds__(BM_THREADS) void block_emit_kernel(const uint32_t* __restrict__ bits, const int32_t* __restrict__ row_ptr,
                                                                int32_t* __restrict__ tile_idx, int n_rows, int n_words) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    uint32_t word = lane < n_words ? bits[(int64_t)r * n_words + lane] : 0u;
    const int c = __popc(word);
    int v = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    int32_t* dst = tile_idx + row_ptr[r] + (v - c);
    while (word) {
        *dst++ = lane * 32 + (__ffs(word) - 1);
        word &= word - 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct Shape {
    int64_t n_qb, n_t, n_rows, n_words;
};

static int check_shape(const char* who, int64_t q_len, int64_t kv_len, int64_t heads, Shape* sh) {
    GF_CHECK_ARG(q_len >= 1 && heads >= 1, "%s: expected q_len >= 1 and heads >= 1, got %lld / %lld", who, (long long)q_len, (long long)heads);
    GF_CHECK_ARG(kv_len >= 2 * BM_KB, "%s: expected kv_len >= 128 (two key tiles: the sparse kernel's two-tile pipeline), got %lld", who,
                 (long long)kv_len);
    sh->n_qb = (q_len + BM_QB - 1) / BM_QB;
    sh->n_t = (kv_len + BM_KB - 1) / BM_KB;
    GF_CHECK_ARG(sh->n_t <= BM_MAX_TILES, "%s: expected at most 1024 key tiles (kv_len <= 65536), got %lld for kv_len %lld", who,
                 (long long)sh->n_t, (long long)kv_len);
    sh->n_rows = heads * sh->n_qb;
    sh->n_words = (sh->n_t + 31) / 32;
    GF_CHECK_ARG(heads <= 65535 && sh->n_rows * sh->n_t < ((int64_t)1 << 31), "%s: expected heads <= 65535 and heads * n_qblocks * n_tiles below 2^31", who);
    return GF_OK;
}

static int check_means(const char* who, const void* x, int64_t ldx, const float* mean, int64_t rows, int64_t heads, int64_t block) {
    GF_CHECK_ARG(x && mean, "%s: null pointer", who);
    GF_CHECK_ARG(block == BM_QB || block == BM_KB, "%s: expected block 256 (query blocks) or 64 (key tiles), got %lld", who, (long long)block);
    GF_CHECK_ARG(rows >= 1 && rows < ((int64_t)1 << 31) && heads >= 1 && heads <= 65535, "%s: expected 1 <= rows < 2^31 and 1 <= heads <= 65535", who);
    GF_CHECK_ARG(ldx >= heads * 128 && ldx % 8 == 0 && gf_aligned16(x), "%s: expected a row stride >= heads*128 that is a multiple of 8 elements and 16-byte aligned data", who);
    return GF_OK;
}

static int launch_means(const char* who, const void* x, int64_t ldx, float* mean, int64_t rows, int64_t heads, int64_t block, hipStream_t st) {
    if (int e = check_means(who, x, ldx, mean, rows, heads, block)) return e;
    const int nb = (int)((rows + block - 1) / block);
    const dim3 grid(nb, (unsigned)heads);
    if (block == BM_QB)
        block_means_kernel<BM_QB><<<grid, BM_THREADS, 0, st>>>((const u16*)x, ldx, mean, (int)rows, nb);
    else
        block_means_kernel<BM_KB><<<grid, BM_THREADS, 0, st>>>((const u16*)x, ldx, mean, (int)rows, nb);
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}

static int launch_means_coh(const char* who, const void* x, int64_t ldx, float* mean, float* coh, int64_t rows, int64_t heads, int64_t block,
                           hipStream_t st) {
    if (int e = check_means(who, x, ldx, mean, rows, heads, block)) return e;
    GF_CHECK_ARG(coh, "%s: null pointer (coh)", who);
    const int nb = (int)((rows + block - 1) / block);
    const dim3 grid(nb, (unsigned)heads);
    if (block == BM_QB)
        block_means_coh_kernel<BM_QB><<<grid, BM_THREADS, 0, st>>>((const u16*)x, ldx, mean, coh, (int)rows, nb);
    else
        block_means_coh_kernel<BM_KB><<<grid, BM_THREADS, 0, st>>>((const u16*)x, ldx, mean, coh, (int)rows, nb);
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}

static int launch_scores(const char* who, const float* qm, const float* km, float* scores, const Shape& sh, int64_t kv_len, int64_t heads,
                         float scale, hipStream_t st) {
    GF_CHECK_ARG(qm && km && scores, "%s: null pointer", who);
    GF_CHECK_ARG(scale > 0.f && scale < __builtin_inff(), "%s: the softmax scale must be positive and finite, got %g", who, (double)scale);
    const float c = (float)((double)scale * 1.4426950408889634);
    block_scores_kernel<<<dim3((unsigned)((sh.n_t + SC_TILES - 1) / SC_TILES), (unsigned)heads), BM_THREADS, 0, st>>>(
        qm, km, scores, (int)sh.n_qb, (int)sh.n_t, (int)kv_len, c);
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}

static int64_t select_ws_bytes(int64_t n_rows, int64_t n_words) { return align256(n_rows * 4) + align256(n_rows * n_words * 4); }

// the gate of the gated entries: null coherences = that side off; the thresholds are checked by the entries
struct Gate {
    const float *q_coh, *k_coh;
    float q_min, k_min;
};

static int launch_select(const char* who, const float* scores, const uint32_t* forced, int32_t* row_ptr, int32_t* tile_idx, int32_t* head_map,
                         float* kept, void* ws, const Shape& sh, int64_t heads, float mass, hipStream_t st, const Gate* gate = nullptr) {
    GF_CHECK_ARG(scores && row_ptr && tile_idx && head_map && ws, "%s: null pointer", who);
    GF_CHECK_ARG(mass > 0.f, "%s: expected a mass share in (0, 1] (values above 1 select every tile), got %g", who, (double)mass);
    int32_t* counts = (int32_t*)ws;
    uint32_t* bits = (uint32_t*)((char*)ws + align256(sh.n_rows * 4));
    if (gate != nullptr && (gate->q_coh != nullptr || gate->k_coh != nullptr))
        block_select_kernel<true><<<(unsigned)sh.n_rows, BM_THREADS, 0, st>>>(scores, forced, counts, bits, kept, (int)sh.n_qb, (int)sh.n_t,
                                                                             (int)sh.n_words, mass, gate->q_coh, gate->k_coh, gate->q_min,
                                                                             gate->k_min);
    else
        block_select_kernel<false><<<(unsigned)sh.n_rows, BM_THREADS, 0, st>>>(scores, forced, counts, bits, kept, (int)sh.n_qb, (int)sh.n_t,
                                                                              (int)sh.n_words, mass, nullptr, nullptr, 1.f, 1.f);
    GF_CHECK_LAUNCH(who);
    block_scan_kernel<<<1, 1024, 0, st>>>(counts, row_ptr, head_map, (int)sh.n_rows, (int)heads);
    GF_CHECK_LAUNCH(who);
    block_emit_kernel<<<(unsigned)((sh.n_rows + 3) / 4), BM_THREADS, 0, st>>>(bits, row_ptr, tile_idx, (int)sh.n_rows, (int)sh.n_words);
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}

}  // namespace

extern "C" GF_API int64_t gf_block_map_select_workspace_bytes(int64_t n_qblocks, int64_t n_tiles, int64_t heads) {
    if (n_qblocks < 1 || n_tiles < 2 || n_tiles > BM_MAX_TILES || heads < 1) return 0;
    return select_ws_bytes(heads * n_qblocks, (n_tiles + 31) / 32);
}

extern "C" GF_API int64_t gf_block_map_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads) {
    Shape sh;
    if (check_shape("gf_block_map_workspace_bytes", q_len, kv_len, heads, &sh) != GF_OK) return 0;
    return align256(sh.n_rows * 128 * 4) + align256(heads * sh.n_t * 128 * 4) + align256(sh.n_rows * sh.n_t * 4) +
           select_ws_bytes(sh.n_rows, sh.n_words);
}

extern "C" GF_API int gf_block_means(const void* x, int64_t ldx, float* mean, int64_t rows, int64_t heads, int64_t block, void* stream) {
    return launch_means("gf_block_means", x, ldx, mean, rows, heads, block, (hipStream_t)stream);
}

extern "C" GF_API int gf_block_map_scores(const float* q_mean, const float* k_mean, float* scores, int64_t q_len, int64_t kv_len,
                                          int64_t heads, float scale, void* stream) {
    Shape sh;
    if (int e = check_shape("gf_block_map_scores", q_len, kv_len, heads, &sh)) return e;
    return launch_scores("gf_block_map_scores", q_mean, k_mean, scores, sh, kv_len, heads, scale, (hipStream_t)stream);
}

extern "C" GF_API int gf_block_map_select(const float* scores, const uint32_t* forced, int32_t* row_ptr, int32_t* tile_idx,
                                          int32_t* head_map, float* kept, void* ws, int64_t n_qblocks, int64_t n_tiles, int64_t heads,
                                          float mass, void* stream) {
    const char* who = "gf_block_map_select";
    GF_CHECK_ARG(n_qblocks >= 1 && heads >= 1 && heads <= 65535, "%s: expected n_qblocks >= 1 and 1 <= heads <= 65535", who);
    GF_CHECK_ARG(n_tiles >= 2 && n_tiles <= BM_MAX_TILES, "%s: expected 2 .. 1024 key tiles, got %lld", who, (long long)n_tiles);
    Shape sh{n_qblocks, n_tiles, heads * n_qblocks, (n_tiles + 31) / 32};
    GF_CHECK_ARG(sh.n_rows * sh.n_t < ((int64_t)1 << 31), "%s: expected heads * n_qblocks * n_tiles below 2^31", who);
    return launch_select(who, scores, forced, row_ptr, tile_idx, head_map, kept, ws, sh, heads, mass, (hipStream_t)stream);
}

extern "C" GF_API int gf_block_map_from_qk(const void* q, int64_t ldq, const void* k, int64_t ldk, const uint32_t* forced, int32_t* row_ptr,
                                           int32_t* tile_idx, int32_t* head_map, float* scores, float* kept, void* ws, int64_t q_len,
                                           int64_t kv_len, int64_t heads, float scale, float mass, void* stream) {
    const char* who = "gf_block_map_from_qk";
    Shape sh;
    if (int e = check_shape(who, q_len, kv_len, heads, &sh)) return e;
    GF_CHECK_ARG(ws && (((uintptr_t)ws) & 255u) == 0, "%s: expected a 256-byte aligned workspace of gf_block_map_workspace_bytes bytes", who);
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)ws;
    float* qm = (float*)p;
    p += align256(sh.n_rows * 128 * 4);
    float* km = (float*)p;
    p += align256(heads * sh.n_t * 128 * 4);
    float* sc = scores ? scores : (float*)p;
    p += align256(sh.n_rows * sh.n_t * 4);
    // every argument is checked before the first launch: a refused call enqueues nothing
    GF_CHECK_ARG(q && k && row_ptr && tile_idx && head_map, "%s: null pointer", who);
    GF_CHECK_ARG(ldq >= heads * 128 && ldq % 8 == 0 && gf_aligned16(q) && ldk >= heads * 128 && ldk % 8 == 0 && gf_aligned16(k),
                 "%s: expected row strides >= heads*128 that are multiples of 8 elements and 16-byte aligned data", who);
    GF_CHECK_ARG(scale > 0.f && scale < __builtin_inff(), "%s: the softmax scale must be positive and finite, got %g", who, (double)scale);
    GF_CHECK_ARG(mass > 0.f, "%s: expected a mass share in (0, 1] (values above 1 select every tile), got %g", who, (double)mass);
    if (int e = launch_means(who, q, ldq, qm, q_len, heads, BM_QB, st)) return e;
    if (int e = launch_means(who, k, ldk, km, kv_len, heads, BM_KB, st)) return e;
    if (int e = launch_scores(who, qm, km, sc, sh, kv_len, heads, scale, st)) return e;
    return launch_select(who, sc, forced, row_ptr, tile_idx, head_map, kept, p, sh, heads, mass, st);
}

// ---------------------------------------------------------------------------------------------------- the coherence-gated entries
static int check_gate_min(const char* who, const char* name, float v) {
    GF_CHECK_ARG(v > 0.f && v <= 1.f, "%s: expected %s in (0, 1] (the least coherence a block is predicted for), got %g", who, name, (double)v);
    return GF_OK;
}

extern "C" GF_API int64_t gf_block_map_gated_workspace_bytes(int64_t q_len, int64_t kv_len, int64_t heads) {
    Shape sh;
    if (check_shape("gf_block_map_gated_workspace_bytes", q_len, kv_len, heads, &sh) != GF_OK) return 0;
    return align256(sh.n_rows * 128 * 4) + align256(heads * sh.n_t * 128 * 4) + align256(sh.n_rows * sh.n_t * 4) + align256(sh.n_rows * 4) +
           align256(heads * sh.n_t * 4) + select_ws_bytes(sh.n_rows, sh.n_words);
}

extern "C" GF_API int gf_block_means_coh(const void* x, int64_t ldx, float* mean, float* coh, int64_t rows, int64_t heads, int64_t block,
                                         void* stream) {
    return launch_means_coh("gf_block_means_coh", x, ldx, mean, coh, rows, heads, block, (hipStream_t)stream);
}

extern "C" GF_API int gf_block_map_select_gated(const float* scores, const uint32_t* forced, const float* q_coh, const float* k_coh,
                                                int32_t* row_ptr, int32_t* tile_idx, int32_t* head_map, float* kept, void* ws,
                                                int64_t n_qblocks, int64_t n_tiles, int64_t heads, float mass, float q_min, float k_min,
                                                void* stream) {
    const char* who = "gf_block_map_select_gated";
    GF_CHECK_ARG(n_qblocks >= 1 && heads >= 1 && heads <= 65535, "%s: expected n_qblocks >= 1 and 1 <= heads <= 65535", who);
    GF_CHECK_ARG(n_tiles >= 2 && n_tiles <= BM_MAX_TILES, "%s: expected 2 .. 1024 key tiles, got %lld", who, (long long)n_tiles);
    Shape sh{n_qblocks, n_tiles, heads * n_qblocks, (n_tiles + 31) / 32};
    GF_CHECK_ARG(sh.n_rows * sh.n_t < ((int64_t)1 << 31), "%s: expected heads * n_qblocks * n_tiles below 2^31", who);
    if (int e = check_gate_min(who, "q_min", q_min)) return e;
    if (int e = check_gate_min(who, "k_min", k_min)) return e;
    const Gate gate{q_coh, k_coh, q_min, k_min};
    return launch_select(who, scores, forced, row_ptr, tile_idx, head_map, kept, ws, sh, heads, mass, (hipStream_t)stream, &gate);
}

extern "C" GF_API int gf_block_map_from_qk_gated(const void* q, int64_t ldq, const void* k, int64_t ldk, const uint32_t* forced,
                                                 int32_t* row_ptr, int32_t* tile_idx, int32_t* head_map, float* scores, float* kept,
                                                 float* q_coh_out, float* k_coh_out, void* ws, int64_t q_len, int64_t kv_len, int64_t heads,
                                                 float scale, float mass, float q_min, float k_min, void* stream) {
    const char* who = "gf_block_map_from_qk_gated";
    Shape sh;
    if (int e = check_shape(who, q_len, kv_len, heads, &sh)) return e;
    GF_CHECK_ARG(ws && (((uintptr_t)ws) & 255u) == 0, "%s: expected a 256-byte aligned workspace of gf_block_map_gated_workspace_bytes bytes", who);
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)ws;
    float* qm = (float*)p;
    p += align256(sh.n_rows * 128 * 4);
    float* km = (float*)p;
    p += align256(heads * sh.n_t * 128 * 4);
    float* sc = scores ? scores : (float*)p;
    p += align256(sh.n_rows * sh.n_t * 4);
    // a coherence output the caller asked for is written in place of the workspace's copy: the same kernel, the same bits
    float* qc = q_coh_out ? q_coh_out : (float*)p;
    p += align256(sh.n_rows * 4);
    float* kc = k_coh_out ? k_coh_out : (float*)p;
    p += align256(heads * sh.n_t * 4);
    // every argument is checked before the first launch: a refused call enqueues nothing
    GF_CHECK_ARG(q && k && row_ptr && tile_idx && head_map, "%s: null pointer", who);
    GF_CHECK_ARG(ldq >= heads * 128 && ldq % 8 == 0 && gf_aligned16(q) && ldk >= heads * 128 && ldk % 8 == 0 && gf_aligned16(k),
                 "%s: expected row strides >= heads*128 that are multiples of 8 elements and 16-byte aligned data", who);
    GF_CHECK_ARG(scale > 0.f && scale < __builtin_inff(), "%s: the softmax scale must be positive and finite, got %g", who, (double)scale);
    GF_CHECK_ARG(mass > 0.f, "%s: expected a mass share in (0, 1] (values above 1 select every tile), got %g", who, (double)mass);
    // a threshold <= 0 switches its side of the gate off; NaN and values above 1 are refused
    GF_CHECK_ARG(q_min <= 1.f, "%s: expected q_min in (0, 1], or <= 0 for no query gate, got %g", who, (double)q_min);
    GF_CHECK_ARG(k_min <= 1.f, "%s: expected k_min in (0, 1], or <= 0 for no key gate, got %g", who, (double)k_min);
    const Gate gate{q_min > 0.f ? qc : nullptr, k_min > 0.f ? kc : nullptr, q_min > 0.f ? q_min : 1.f, k_min > 0.f ? k_min : 1.f};
    if (int e = launch_means_coh(who, q, ldq, qm, qc, q_len, heads, BM_QB, st)) return e;
    if (int e = launch_means_coh(who, k, ldk, km, kc, kv_len, heads, BM_KB, st)) return e;
    if (int e = launch_scores(who, qm, km, sc, sh, kv_len, heads, scale, st)) return e;
    return launch_select(who, sc, forced, row_ptr, tile_idx, head_map, kept, p, sh, heads, mass, st, &gate);
}

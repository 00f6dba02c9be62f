// gf_mxfp4_quant.h — the MXFP4 block quantiser (include/goalforce.h, "MXFP4 Linear"), stated once for its three users: the stand-alone
// pass quant_mxfp4_kernel, the LayerNorm that feeds an fp4 Linear (gf_rowops.hip) and the quantising epilogue of gemm_mxfp4_kernel.
// Thread = 8 consecutive bf16 elements (one 16-byte piece), four neighbouring lanes (lane & ~3 .. lane | 3) = one MX block of 32.
// Everything is integer work on the bf16 bit patterns and exact power-of-two scalings: no step depends on the denormal mode, and the
// same bf16 values give the same bytes wherever they are quantised.
#pragma once
#include "gf_common.h"

__device__ __forceinline__ unsigned e2m1_code(unsigned bits, int code) {
    // |x| = sig * 2^ex (bf16: normal sig = 128 + mantissa, ex = exponent field - 134; subnormal sig = mantissa, ex = -133)
    const unsigned a = bits & 0x7FFFu;
    const int ef = (int)(a >> 7);
    const int sig = ef ? (int)(128u | (a & 127u)) : (int)(a & 127u);
    // v = |x| * 2^-(code - 127) = sig * 2^t, below 8 by the choice of the code; far below 1/4 (t < -40) it rounds to 0 like anything there
    const int t = max((ef ? ef : 1) - 134 - code + 127, -40);
    const float v = sig ? __uint_as_float(__float_as_uint((float)sig) + ((unsigned)t << 23)) : 0.0f;   // a normal fp32, exact
    // e2m1's grid: steps of 1/2 below 2, of 1 below 4, of 2 above; v_rndne rounds ties to the even multiple = the even mantissa code
    int c;
    if (v < 2.0f) c = (int)__builtin_rintf(v * 2.0f);                 // 0, .5, 1, 1.5, (2)   -> codes 0..4
    else if (v < 4.0f) c = 2 + (int)__builtin_rintf(v);               // 2, 3, (4)            -> codes 4..6
    else c = min(4 + (int)__builtin_rintf(v * 0.5f), 7);              // 4, 6, saturating     -> codes 6, 7
    return (unsigned)c | ((bits >> 12) & 8u);
}

// The block step on this lane's 8 bf16 patterns: -> the packed dword of its 8 e2m1 codes (element 2i in bits 3:0 of byte i, 2i+1 in
// bits 7:4) and, in `code`, the block's E8M0 byte (the same in all four lanes).  It holds two shuffles: ALL FOUR lanes of a block must
// execute it, so call it in front of any m < M / n < N branch, never inside one.
__device__ __forceinline__ unsigned mxfp4_block_step(const u16x8 xv, int& code) {
    unsigned amax = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = max(amax, (unsigned)(xv[e] & 0x7FFFu));   // |x| orders like its bits; NaN / inf are >= 0x7F80
    amax = max(amax, (unsigned)__shfl_xor((int)amax, 1));
    amax = max(amax, (unsigned)__shfl_xor((int)amax, 2));
    unsigned packed = 0;
    if (amax >= 0x7F80u) code = 255;                                  // a NaN or an infinity in the block: NaN scale, elements +0
    else if (amax == 0) code = 127;
    else {
        const int ef = (int)(amax >> 7);
        // floor(log2 amax): exponent field - 127, subnormals by their leading mantissa bit; code = that - 2 + 127, clamped to 0 .. 254
        const int fl = ef ? ef - 127 : -133 + (31 - __builtin_clz(amax & 127u));
        code = min(max(fl - 2 + 127, 0), 254);
#pragma unroll
        for (int e = 0; e < 8; ++e) packed |= e2m1_code(xv[e], code) << (4 * e);   // element 2i in bits 3:0 of byte i, 2i+1 in bits 7:4
    }
    return packed;
}

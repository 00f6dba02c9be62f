// gf_window.hip — sliding-window sampling (TemporalTiler_BCTHW, GF:1296-1345): the weighted accumulation of one temporal
// window's prediction into the bf16 accumulators, and the final division.  The sibling in time of gf_vae.hip's tile blend.
// Both kernels move a few MB once per window (16 x 21 x 6240 elements at 480 x 832) beside a forward of seconds: they are
// plain grid-stride loops, one element per lane and trip.
#include "gf_common.h"

namespace {

constexpr int WT = 256;
static inline unsigned wgrid(long work_items) {
    long b = (work_items + WT - 1) / WT;
    if (b < 1) b = 1;
    if (b > 256 * 8) b = 256 * 8;
    return (unsigned)b;
}

// build_1d_mask (GF:1300-1310) at window frame i, already rounded to bf16 (`.to(dtype=data_dtype)`, GF:1340).  The right ramp
// is assigned after the left one there, so it wins where the two overlap (len < 2*border).
__device__ __forceinline__ float window_mask(int i, int len, int left_bound, int right_bound, int border) {
    float m = 1.f;
    if (!left_bound && i < border) m = ((float)i + 0.5f) / (float)border;
    if (!right_bound && i >= len - border) m = ((float)(len - 1 - i) + 0.5f) / (float)border;
    return rbf(m);
}

// value[c, t0+i, p] += win[c, i, p] * mask(i);  weight[t0+i] += mask(i)   (GF:1341-1342, every op rounded to bf16)
__global__ __launch_bounds__(WT) void window_blend_kernel(u16* __restrict__ value, u16* __restrict__ weight,
                                                          const u16* __restrict__ win, long C, long HW, long sc, long st,
                                                          int t0, int len, int left_bound, int right_bound, int border) {
    const long total = C * len * HW;
    const long stride = (long)gridDim.x * WT;
    for (long e = (long)blockIdx.x * WT + threadIdx.x; e < total; e += stride) {
        const long p = e % HW;
        const long ci = e / HW;
        const int i = (int)(ci % len);
        const long c = ci / len;
        const float m = window_mask(i, len, left_bound, right_bound, border);
        u16* vp = value + c * sc + (long)(t0 + i) * st + p;
        *vp = f2bf(bf2f(*vp) + rbf(bf2f(win[e]) * m));
        if (c == 0 && p == 0) weight[t0 + i] = f2bf(bf2f(weight[t0 + i]) + m);
    }
}

// value /= weight   (GF:1343)
__global__ __launch_bounds__(WT) void window_finalize_kernel(u16* __restrict__ value, const u16* __restrict__ weight, long C,
                                                             long T, long HW, long sc, long st) {
    const long total = C * T * HW;
    const long stride = (long)gridDim.x * WT;
    for (long e = (long)blockIdx.x * WT + threadIdx.x; e < total; e += stride) {
        const long p = e % HW;
        const long ct = e / HW;
        const long t = ct % T;
        u16* vp = value + (ct / T) * sc + t * st + p;
        *vp = f2bf(bf2f(*vp) / bf2f(weight[t]));
    }
}

// what both entry points ask of the accumulator: [C, T, HW] with HW contiguous and planes that do not overlap
static inline bool value_layout_ok(int64_t C, int64_t T, int64_t HW, int64_t sc, int64_t st) {
    return C > 0 && T > 0 && HW > 0 && T < (1 << 30) && st >= HW && sc >= (T - 1) * st + HW;
}

}  // namespace

extern "C" GF_API int gf_window_blend(void* value, void* weight, const void* win, int64_t C, int64_t T, int64_t HW,
                                      int64_t value_stride_c, int64_t value_stride_t, int64_t t0, int64_t len, int left_bound,
                                      int right_bound, int64_t border, void* stream) {
    GF_CHECK_ARG(value && weight && win, "gf_window_blend: null pointer");
    GF_CHECK_ARG(value_layout_ok(C, T, HW, value_stride_c, value_stride_t),
                 "gf_window_blend: value must be [C, T, HW] with positive sizes, HW contiguous and non-overlapping planes");
    GF_CHECK_ARG(len > 0, "gf_window_blend: len must be positive");
    GF_CHECK_ARG(t0 >= 0 && t0 + len <= T, "gf_window_blend: window outside the T frames of value");
    GF_CHECK_ARG(border >= 0, "gf_window_blend: border must not be negative");
    GF_CHECK_ARG(border == 0 || (left_bound && right_bound) || border < len,
                 "gf_window_blend: border must be smaller than len where a ramp is requested");
    const int ramp = (left_bound && right_bound) ? 0 : (int)border;   // no ramp requested: any border passes and none is applied
    hipLaunchKernelGGL(window_blend_kernel, dim3(wgrid(C * len * HW)), dim3(WT), 0, (hipStream_t)stream, (u16*)value,
                       (u16*)weight, (const u16*)win, (long)C, (long)HW, (long)value_stride_c, (long)value_stride_t, (int)t0,
                       (int)len, left_bound ? 1 : 0, right_bound ? 1 : 0, ramp);
    GF_CHECK_LAUNCH("gf_window_blend");
    return GF_OK;
}

extern "C" GF_API int gf_window_finalize(void* value, const void* weight, int64_t C, int64_t T, int64_t HW, int64_t value_stride_c,
                                         int64_t value_stride_t, void* stream) {
    GF_CHECK_ARG(value && weight, "gf_window_finalize: null pointer");
    GF_CHECK_ARG(value_layout_ok(C, T, HW, value_stride_c, value_stride_t),
                 "gf_window_finalize: value must be [C, T, HW] with positive sizes, HW contiguous and non-overlapping planes");
    hipLaunchKernelGGL(window_finalize_kernel, dim3(wgrid(C * T * HW)), dim3(WT), 0, (hipStream_t)stream, (u16*)value,
                       (const u16*)weight, (long)C, (long)T, (long)HW, (long)value_stride_c, (long)value_stride_t);
    GF_CHECK_LAUNCH("gf_window_finalize");
    return GF_OK;
}

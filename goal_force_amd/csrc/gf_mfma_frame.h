// gf_mfma_frame.h — what the MFMA kernels share, stated once: the workgroup orders, the 4-wave frame's per-lane addresses
// (gemm_a4_kernel, conv_a4_kernel), the AGPR hand-off read, LDS-DMA, and the launch of a kernel with dynamic LDS.
// Every device helper restates the expression its kernels had inline, literally: the kernels' instruction streams are the
// ones they had before this header existed (profiles/r10/asm_identity.txt).
#pragma once
#include "gf_common.h"
#include <type_traits>

template <int I, int N, class F>
__device__ __forceinline__ void gf_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        gf_static_for<I + 1, N>(f);
    }
}

// accumulator I of a K loop that leaves its results in AGPRs (tools/check_a4_agpr.py checks the hand-off on the assembly)
template <int I>
__device__ __forceinline__ float gf_agpr_read() {
    float x;
    asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "n"(I));
    return x;
}

// LDS-DMA: 16 bytes per lane, lane-linear in LDS from `l`
__device__ __forceinline__ void glds16(const void* g, GF_LDS char* l) {
    __builtin_amdgcn_global_load_lds((const GF_GLOBAL void*)g, (GF_LDS void*)l, 16, 0, 0);
}

// XCD-aware workgroup order (bijective for any grid size): XCD blockIdx % 8 owns a contiguous range of the `nwg` positions
// of the caller's tile order; returns this workgroup's position.  What a kernel does with it (groups of row tiles, row-major)
// is its own.
__device__ __forceinline__ int gf_xcd_tile_order(int nwg) {
    const int pid = blockIdx.x;
    const int xcd = pid & 7, local = pid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

// Attention family: the blocks of ONE head run on one XCD, whose L2 then holds that head's streamed operands (heads a multiple
// of 8; otherwise head-major)
__device__ __forceinline__ void gf_xcd_head_block(int pid, int heads, int nblk, int& head, int& blk) {
    if ((heads & 7) == 0) {
        const int xcd = pid & 7, idx = pid >> 3;
        head = xcd + 8 * (idx / nblk);
        blk = idx % nblk;
    } else {
        head = pid / nblk;
        blk = pid % nblk;
    }
}

// ---- the 4-wave frame (gemm_a4_kernel, conv_a4_kernel): 256 threads = 4 waves (wm, wn) in 2 x 2, two LDS stages of (A tile 256 rows |
// W tile) x 128-byte rows with 16-byte chunk c of row r at chunk c ^ (r & 7), staged by `buffer_load_dwordx4 ... offen lds` in 1-KiB
// pieces of 8 rows: piece q of wave w = rows 32 q + 8 w .. + 7 of the tile.
// Source byte offset of lane l in a piece: it fills LDS chunk (l & 7) of row (l >> 3) and must fetch logical chunk (l & 7) ^ (row & 7)
// of that row; `ld` elements of ESZ bytes per source row.
// The rest of the per-lane setup (descriptor halves, the pieces' row-group offsets, the LDS write base, the four swizzled fragment read
// addresses) stays written out in the two kernels: one call returning all of it, a call per group and a helper for the swizzled chunk
// term alone each changed the instruction stream of gemm_a4_kernel (profiles/r10/asm_identity.txt lists what was tried).
template <unsigned ESZ>
__device__ __forceinline__ unsigned gf_a4_voff(int lane, unsigned ld) {
    const int srow = lane >> 3;
    return (unsigned)srow * ld * ESZ + (unsigned)(((lane & 7) ^ srow) << 4);
}

// ---- host: set the dynamic-LDS limit of `Kernel` once per device (one GfDeviceOnce per kernel function, whichever launcher
// reaches it), launch it, check the launch.  `who` names the caller in the attribute error, whose text either carries the byte
// count or does not (each entry point keeps the message it always had); `name` names it in the launch error.
enum GfAttrMsg { GF_ATTR_MSG_PLAIN, GF_ATTR_MSG_BYTES };   // "%s: hipFuncSetAttribute failed: %s" / "%s: hipFuncSetAttribute(%d B LDS) failed: %s"
template <auto Kernel>
static inline int gf_arm_lds(const char* who, GfAttrMsg msg, int lds) {
    static GfDeviceOnce once;
    const hipError_t e = gf_once_per_device(once, [lds] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    });
    if (e == hipSuccess) return GF_OK;
    if (msg == GF_ATTR_MSG_BYTES) gf_set_error("%s: hipFuncSetAttribute(%d B LDS) failed: %s", who, lds, hipGetErrorString(e));
    else gf_set_error("%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(e));
    return GF_ERR_LAUNCH;
}
template <auto Kernel, class... Args>
static inline int gf_launch_lds(const char* who, GfAttrMsg msg, const char* name, dim3 grid, dim3 block, int lds, hipStream_t stream,
                                const Args&... args) {
    if (const int rc = gf_arm_lds<Kernel>(who, msg, lds)) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    GF_CHECK_LAUNCH(name);
    return GF_OK;
}

// ---- host: from a run-time value to a template argument.  gf_dispatch<V0, V1, ...>(v, f) returns f(std::integral_constant<int, Vi>{})
// for the Vi that equals v; the LAST value also answers every other v, like the `default:` of a switch (callers have checked v).
// Nested calls select among a product of values; f is instantiated once per listed value and for nothing else.
template <int V0, int... Vs, class F>
static inline int gf_dispatch(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else return v == V0 ? f(std::integral_constant<int, V0>{}) : gf_dispatch<Vs...>(v, f);
}

// wave_ops.h — cross-lane primitives of a wave64 without the LDS pipe, one copy each: DPP moves, the gfx950
// v_permlane{16,32}_swap pairs, wave / group sums, a double read from a lane, the reciprocal square root of the pivot chains.
// Needs nothing but the HIP runtime.
#pragma once
#include <hip/hip_runtime.h>

namespace sadvio {

// ds_bpermute / ds_swizzle shuffles and ds_add_f64 cost ~100-170 cycles per wave-instruction here (measured),
// DPP modifiers and the gfx950 v_permlane{16,32}_swap are plain VALU. dpp_ctrl: quad_perm 0x00-0xFF,
// row_shl:n 0x100+n, row_shr:n 0x110+n, row_ror:n 0x120+n, row_mirror 0x140, row_half_mirror 0x141.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }

// v_permlane16_swap / v_permlane32_swap of a register with itself: (even-row member, odd-row member) of the lane pair {l, l ^ 16}
// in both lanes; likewise (lower, upper) of {l, l ^ 32}. Symmetric combinations (sum, max) need not know which is which.
__device__ __forceinline__ void swap16_pair_f64(double v, double& x0, double& x1) {
    unsigned lo = __double2loint(v), hi = __double2hiint(v);
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x0 = __hiloint2double(b[0], a[0]); x1 = __hiloint2double(b[1], a[1]);
}
__device__ __forceinline__ void swap32_pair_f64(double v, double& x0, double& x1) {
    unsigned lo = __double2loint(v), hi = __double2hiint(v);
    auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    x0 = __hiloint2double(b[0], a[0]); x1 = __hiloint2double(b[1], a[1]);
}
// v[lane] + v[lane ^ 16] / v[lane ^ 32] in every lane
__device__ __forceinline__ double xor16_sum(double v) { double x0, x1; swap16_pair_f64(v, x0, x1); return x0 + x1; }
__device__ __forceinline__ double xor32_sum(double v) { double x0, x1; swap32_pair_f64(v, x0, x1); return x0 + x1; }
__device__ __forceinline__ int xor16_other(int v) {  // the value held by lane ^ 16 (SADVIO_KERNEL_TS builds: the tile-sum counters of k_build)
    auto a = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((threadIdx.x & 16) ? a[0] : a[1]);
}
__device__ __forceinline__ int xor32_other(int v) {
    auto a = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((threadIdx.x & 32) ? a[0] : a[1]);
}

// Wave-wide sum / max with DPP + the permlane swaps: every lane receives the result. The __shfl_down forms go through
// ds_bpermute, ~100 cycles per step on the LDS pipe: six steps per value were ~1 us of every kernel tail that reduces a
// handful of partials.
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_f64<0xB1>(v);   // xor 1
    v += dpp_f64<0x4E>(v);   // xor 2
    v += dpp_f64<0x141>(v);  // row_half_mirror
    v += dpp_f64<0x140>(v);  // row_mirror
    double x0, x1;
    swap16_pair_f64(v, x0, x1); v = x0 + x1;
    swap32_pair_f64(v, x0, x1); v = x0 + x1;
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    double x0, x1;
    swap16_pair_f64(v, x0, x1); v = fmax(x0, x1);
    swap32_pair_f64(v, x0, x1); v = fmax(x0, x1);
    return v;
}

// Sum over the G lanes of a landmark group (G = power of two, 8 <= G <= 64, groups aligned to G lanes);
// every lane of the group receives the total.
__device__ __forceinline__ double group_sum(double v, int G) {
    v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]  (xor 1)
    v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]  (xor 2)
    v += dpp_f64<0x141>(v);  // row_half_mirror: the other quad of the 8-lane group
    if (G >= 16) v += dpp_f64<0x140>(v);  // row_mirror: the other half of the 16-lane row
    if (G >= 32) v = xor16_sum(v);
    if (G >= 64) v = xor32_sum(v);
    return v;
}

// the value lane `lane` (wave-uniform) holds, in every lane: two v_readlane
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane);
    hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}

// 1 / sqrt(d) for the pivot chains: v_rsq_f64 (2^-24) + ONE third-order (Halley) step, e = 1 - d y^2, y <- y (1 + e / 2 + 3 e^2 / 8):
// error O(e^3) ~ 1e-22 before rounding; five dependent operations instead of the six of two Newton steps
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
    const double t = d * y;
    const double e = __builtin_fma(-t, y, 1.0);
    const double p = __builtin_fma(0.375, e, 0.5);
    const double q = e * p;
    return __builtin_fma(y, q, y);
}

}  // namespace sadvio

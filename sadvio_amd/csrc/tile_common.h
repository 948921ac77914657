// tile_common.h — the landmark-group machinery shared by the two tile kernels (k_build, k_backsub) and the long-track kernels:
// lane-local linearisation, the per-landmark elimination, the LDS tables of a tile.
#pragma once
#include "device_math.h"
#include "step_args.h"
#include "wave_ops.h"

namespace sadvio {

// ceres::HuberLoss(a) + Corrector (rho'' <= 0 branch): returns rho(|r|^2) and the scale sqrt(rho') for r and J.
__device__ __forceinline__ double huber_rho(double a, double s, double& scale) {
    scale = 1.0;
    if (a > 0.0 && s > a * a) {
        const double rr = sqrt(s);
        scale = sqrt(fmax(2.2250738585072014e-308, a / rr));
        return 2.0 * a * rr - a * a;
    }
    return s;
}

struct ObsLin {
    double r[2], Jp[12], Jl[6];
    double rho;   // loss-corrected cost of the block (= |r|^2 without a loss function)
    int row;      // row of the observing key-frame in the tile's LDS system, -1 if constant
    int slot;     // index into the tile's key-frame list
    bool valid;   // this lane owns an observation
    bool counted; // the residual block belongs to the reduced program (some parameter block is free)
};

// Lane-local linearisation of observation `o` of landmark `gl` from LDS tables.
// RARE = false compiles the robust loss out (plain window BA: huber_a = 0, no prior-kept landmarks).
// The constants of one observation, loaded ahead of use (k_build fetches its first landmark round while the LM decision of
// the previous slot is still being summed).
struct ObsPre {
    int slot, craw;
    double m[3];
};
template <int FACTOR>
__device__ __forceinline__ ObsPre obs_prefetch(const DevPtrs& P, int o) {
    ObsPre q;
    q.slot = P.obs_slot[o];
    q.craw = P.obs_cam[o];
    if (FACTOR == 0) { const double* m = P.obs_meas + 2 * (long long)o; q.m[0] = m[0]; q.m[1] = m[1]; q.m[2] = 0.0; }
    else { const double* m = P.obs_meas + 3 * (long long)o; q.m[0] = m[0]; q.m[1] = m[1]; q.m[2] = m[2]; }
    return q;
}

template <int FACTOR, bool RARE>
__device__ __forceinline__ void lane_linearize(const DevPtrs& P, const double* poseTab, const double* camTab,
                                               const int* rowTab, int cam_base, const ObsPre& ob, const double* pw, bool keep_jl,
                                               bool lcounted, ObsLin& L) {
    const int slot = ob.slot;
    const int craw = ob.craw;
    const int cam = craw < 0 ? 0 : craw - cam_base;
    const double* tab = poseTab + slot * POSE_TAB;
    const double* ct = camTab + cam * 17;  // K[4] Tsf[12] isig
    L.slot = slot;
    L.row = rowTab[slot];
    if (RARE && craw < 0) {
        // pseudo-observation: one half of a PoseToLandmarkFactor of the sparsified prior (no loss function on it)
        const int code = -1 - craw;
        const SparseDev& f = P.sparse[code >> 1];
        p2l_pseudo_obs<true>(tab, pw, f.delta, f.W, code & 1, L.r, L.Jp, L.Jl);
        L.rho = L.r[0] * L.r[0] + L.r[1] * L.r[1];
        if (L.row < 0) {
#pragma unroll
            for (int i = 0; i < 12; i++) L.Jp[i] = 0.0;
        }
        if (!keep_jl) {
#pragma unroll
            for (int i = 0; i < 6; i++) L.Jl[i] = 0.0;
        }
        L.counted = (L.row >= 0) || lcounted;
        return;
    }
    if (FACTOR == 0) {
        pixel_factor<true>(tab, ct, ct + 4, pw, ob.m[0], ob.m[1], ct[16], L.r, L.Jp, L.Jl);
    } else {
        double b[3] = {ob.m[0], ob.m[1], ob.m[2]};
        angular_factor<true>(tab, ct + 4, pw, b, ct[16], L.r, L.Jp, L.Jl);
    }
    L.rho = L.r[0] * L.r[0] + L.r[1] * L.r[1];
    if (RARE) {
        double sc;
        L.rho = huber_rho(P.o.huber_a, L.rho, sc);
        if (sc != 1.0) {
            L.r[0] *= sc; L.r[1] *= sc;
#pragma unroll
            for (int i = 0; i < 12; i++) L.Jp[i] *= sc;
#pragma unroll
            for (int i = 0; i < 6; i++) L.Jl[i] *= sc;
        }
    }
    if (L.row < 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) L.Jp[i] = 0.0;
    }
    if (!keep_jl) {
#pragma unroll
        for (int i = 0; i < 6; i++) L.Jl[i] = 0.0;
    }
    L.counted = (L.row >= 0) || lcounted;
    if (!L.counted) { /* fixed cost: caller accounts r, then it leaves the program */ }
}

// Inverse Cholesky factor Li (sym3_chol_inverse: packed lower 6-vector) of a landmark's H_ll (packed lower, 6) under the LM damping of
// radius `radius`, s = the landmark's three Jacobi scales
__device__ __forceinline__ void damped_inverse(const DevPtrs& P, const double* H, const double* s, double radius, double* Mi) {
    const double ir = 1.0 / radius;
    const double s0 = s[0] * s[0], s1 = s[1] * s[1], s2 = s[2] * s[2];
    double M[6] = {H[0], H[1], H[2], H[3], H[4], H[5]};
    M[0] += fmin(fmax(s0 * H[0], P.o.min_lm_diagonal), P.o.max_lm_diagonal) * ir / s0;
    M[3] += fmin(fmax(s1 * H[3], P.o.min_lm_diagonal), P.o.max_lm_diagonal) * ir / s1;
    M[5] += fmin(fmax(s2 * H[5], P.o.min_lm_diagonal), P.o.max_lm_diagonal) * ir / s2;
    sym3_chol_inverse(M, Mi);
}

// Per-landmark elimination, every lane of the group redundantly: H_ll, g_l (group sums), LM damping, the inverse Cholesky
// factor Li of the damped block (sym3_chol_inverse: packed lower 6-vector; named Mi below). Returns whether the landmark has a
// parameter block in the program. s_pre: the landmark's three Jacobi scales (DevPtrs::s_lmk) where the caller fetched them with
// the round's other inputs (k_build), or null: they are loaded here, behind the group sums. Unused with write_scale.
__device__ __forceinline__ bool group_eliminate(const DevPtrs& P, const ObsLin& L, int G, int gl, bool lmk_valid,
                                                bool lfree, int nobs, double radius, bool write_scale, bool leader,
                                                double* Mi, double* g, const double* s_pre) {
    double H[6];
    H[0] = L.Jl[0] * L.Jl[0] + L.Jl[3] * L.Jl[3];
    H[1] = L.Jl[0] * L.Jl[1] + L.Jl[3] * L.Jl[4];
    H[2] = L.Jl[0] * L.Jl[2] + L.Jl[3] * L.Jl[5];
    H[3] = L.Jl[1] * L.Jl[1] + L.Jl[4] * L.Jl[4];
    H[4] = L.Jl[1] * L.Jl[2] + L.Jl[4] * L.Jl[5];
    H[5] = L.Jl[2] * L.Jl[2] + L.Jl[5] * L.Jl[5];
    g[0] = L.Jl[0] * L.r[0] + L.Jl[3] * L.r[1];
    g[1] = L.Jl[1] * L.r[0] + L.Jl[4] * L.r[1];
    g[2] = L.Jl[2] * L.r[0] + L.Jl[5] * L.r[1];
#pragma unroll
    for (int i = 0; i < 6; i++) H[i] = group_sum(H[i], G);
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = group_sum(g[i], G);
    const bool active = lmk_valid && lfree && nobs > 0;
    if (!active) {
#pragma unroll
        for (int i = 0; i < 6; i++) Mi[i] = 0.0;
        return false;
    }
    double s[3];
    if (write_scale) {
        s[0] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[0])) : 1.0;
        s[1] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[3])) : 1.0;
        s[2] = P.o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[5])) : 1.0;
        if (leader) {
            P.s_lmk[3 * (long long)gl] = s[0]; P.s_lmk[3 * (long long)gl + 1] = s[1]; P.s_lmk[3 * (long long)gl + 2] = s[2];
        }
    } else if (s_pre) {
        s[0] = s_pre[0]; s[1] = s_pre[1]; s[2] = s_pre[2];
    } else {
        s[0] = P.s_lmk[3 * (long long)gl]; s[1] = P.s_lmk[3 * (long long)gl + 1]; s[2] = P.s_lmk[3 * (long long)gl + 2];
    }
    damped_inverse(P, H, s, radius, Mi);
    return true;
}

// Camera table of a window in LDS: per camera K[4] | Tsf[12] | 1 / sigma (n_cam cameras from global camera cam_base on)
__device__ __forceinline__ void stage_cams(const DevPtrs& P, int cam_base, int n_cam, double* camTab) {
    for (int i = threadIdx.x; i < n_cam * 17; i += blockDim.x) {
        const int c = i / 17, e = i - 17 * c;
        const int gc = cam_base + c;
        camTab[i] = e < 4 ? P.cam_K[4 * (long long)gc + e] : (e < 16 ? P.cam_T[12 * (long long)gc + e - 4] : P.cam_isig[gc]);
    }
}
// Row table of a tile in LDS: the row of each listed key-frame in the tile's system, -1 if constant
__device__ __forceinline__ void stage_rows(const DevPtrs& P, const Tile& T, int* rowTab) {
    for (int i = threadIdx.x; i < T.n_kf; i += blockDim.x) rowTab[i] = P.tile_row[T.kf_off + i];
}

// Stage the tile's key-frame pose tables (buffer `buf`) and the window's cameras into LDS.
__device__ __forceinline__ void stage_tables(const DevPtrs& P, const Tile& T, int buf, double* poseTab, double* camTab,
                                             int* rowTab) {
    const int tid = threadIdx.x;
    const double* src = P.ptab + (long long)buf * P.ptab_stride;
    for (int i = tid; i < T.n_kf * POSE_TAB; i += blockDim.x) {
        const int k = i / POSE_TAB, e = i - k * POSE_TAB;
        poseTab[i] = src[(long long)P.tile_kf[T.kf_off + k] * POSE_TAB + e];
    }
    stage_cams(P, T.cam_base, T.n_cam, camTab);
    stage_rows(P, T, rowTab);
}

__device__ __forceinline__ void wave_lds_fence() {
    // LDS traffic between lanes of ONE wave: order this wave's stores before its later loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ inline size_t tile_tables_bytes(int n_kf) {
    // pose tables + camera tables + row table; a global-atomics tile may list up to 64 key-frames (> MAX_TILE_KF)
    size_t b = sizeof(double) * ((size_t)n_kf * POSE_TAB + MAX_WIN_CAM * 17) + sizeof(int) * (size_t)(n_kf > MAX_TILE_KF ? n_kf : MAX_TILE_KF);
    return (b + 15) & ~(size_t)15;
}

// global landmark in slot i of a tile: listed (packed tiles) or consecutive
__device__ __forceinline__ int tile_landmark(const Tile& T, const int* __restrict__ tile_lmk, int i) { return T.lmk_off >= 0 ? tile_lmk[T.lmk_off + i] : T.lmk0 + i; }

}  // namespace sadvio

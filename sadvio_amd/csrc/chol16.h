// chol16.h — in-LDS Cholesky solve of the reduced pose system (N <= 174) on 16x16 tiles, one 512-thread workgroup.
//
// Layout ("tile-packed"): the lower block triangle of the (N + 1) x (N + 1) matrix [S ; rhs^T] in 16 x 16 tiles,
// tile (I, J), I >= J, at ((I (I + 1) / 2 + J) * 256 doubles, COLUMN-major inside the tile (element (r, c) at c * 16 + r).
// A wave holds a tile as 4 registers per lane: lane l = 16 k + i, register s <-> element (i, 4 s + k) ("X layout") — the
// register s of a tile is 64 consecutive doubles (conflict-free ds_read_b64 / ds_write_b64), and it is at the same time
//   * the A / B operand of v_mfma_f64_16x16x4_f64 for the 4 columns 4 s .. 4 s + 3 of the tile, and
//   * the accumulator layout of the TRANSPOSED tile (D[row = k + 4 s][col = i], measured: scripts/probe/uarch_probe.hip),
// so  X(C) += mfma(A = X(P)[s], B = X(Q)[s])  accumulates  C += Q P^T  with no data movement between products, and a
// SYMMETRIC tile's register s is directly the operand of its own rank-4 update.
//
// Factorisation (right-looking, block columns of 16, 4-column steps inside a block):
//   pivot wave (wave 0)  one diagonal tile D in registers. Per 4-column step: the 4 x 4 pivot block goes to SGPRs
//                        (v_readlane), its Cholesky factor is computed uniformly (v_rsq_f64 + 2 Newton steps per column:
//                        65 cycles, the dependency floor), every lane gets the 4 entries of its row with three
//                        v_permlane{16,32}_swap pairs and forward-substitutes them (y = a L_ss^-T), D -= y y^T is ONE MFMA.
//                        The step's y (= 4 columns of L_kk) is published in LDS (the back-substitution reads the rhs row's).
//                        The same steps run on an identity tile: after the block W = L_kk^-T, which goes into the dead
//                        diagonal tile (X layout) and, transposed and padded, into `wt`.
//   phase A, all waves   panel tiles below the block: L_Ik = A_Ik L_kk^-T, four MFMAs per tile with `wt` as the operand. The
//                        pivot wave takes tile (k + 1, k) and updates the next diagonal tile with it.
//   phase B              the pivot wave factors the next diagonal tile (look-ahead) while the bulk waves run the trailing
//                        update C_IJ -= L_Ik L_Jk^T, 4 MFMAs per tile, and turn the panel of the PREVIOUS block column, dead
//                        as L by then, into H_IJ = L_IJ L_JJ^-1 (stored transposed). In the phase B of the last block column
//                        but one, the wave that ran the only trailing tile left converts that column's panel as well, after
//                        its own reads of it: the last block column then has nothing but the panel of the right-hand side's
//                        tile row (N a multiple of 16; the pivot wave's, which also converts it) and runs without a barrier.
// Two workgroup barriers per block column but the last. The right-hand side is row N of the matrix (forward substitution for
// free); columns >= N of the last tile are dummy pivots (inverse 0: no effect).
// Back-substitution on the H tiles: x_J = z_J - sum_{I > J} H_IJ^T x_I with z = the right-hand-side row of H, no triangular
// solve per block. Thread c owns z_c; per block I from the last one down: its 16 owners put x_I into LDS, one workgroup barrier,
// every thread c < 16 I subtracts H_I,J(c)^T x_I. (A chain through the four blocks of a wave without the barrier, barriers
// between waves only, gives the same bits and was measured 0.55 us SLOWER at N = 114: docs/KERNEL_HISTORY.md "The tail of chol16".)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ba_types.h"
#include "wave_ops.h"

// SADVIO_C16_PARENT_ORDER (compile time; tests/cpp/chol16_order_check.hip and A/B measurements): the back-substitution with the H
// column of a step requested in front of that step's barrier, as it was before the column was requested one step ahead — the same
// floating-point operations in the same order either way. Not a runtime switch: a binary that carries two back-substitution loops ran
// every panel slower (docs/KERNEL_HISTORY.md, "The tail of chol16").

namespace sadvio {

typedef double c16_d4 __attribute__((ext_vector_type(4)));

constexpr int C16_STEP = 64;             // published per 4-column step: y = the step's 4 columns of L_kk (the back-substitution reads the rhs row's)
constexpr int C16_PUB = 4 * C16_STEP;    // per block column; double-buffered by block parity
constexpr int C16_WT = 16 * 17;          // L_kk^-T of the current block, element (r, c) at c * 17 + r (read transposed without bank conflicts)
constexpr int C16_WORK = 2 * C16_PUB + 64 + C16_WT;   // doubles of the exchange area (`pub`)

__host__ __device__ constexpr int c16_tile(int I, int J) { return ((I * (I + 1)) >> 1) + J; }
// element (i, j), i >= j, of the tile-packed lower triangle (diagonal tiles: the lower half; see c16_symmetrize)
__host__ __device__ constexpr int c16_index(int i, int j) { return (c16_tile(i >> 4, j >> 4) << 8) + ((j & 15) << 4) + (i & 15); }
// c16_blocks, c16_size: ba_types.h (the host's layout sizes the image with them)

__device__ __forceinline__ c16_d4 c16_load(const double* t, int ln) {
    c16_d4 v;
    v[0] = t[ln]; v[1] = t[64 + ln]; v[2] = t[128 + ln]; v[3] = t[192 + ln];
    return v;
}
__device__ __forceinline__ void c16_store(double* t, int ln, c16_d4 v) {
    t[ln] = v[0]; t[64 + ln] = v[1]; t[128 + ln] = v[2]; t[192 + ln] = v[3];
}

// Mirror the lower halves of the diagonal tiles into their upper halves (the assembly only writes i >= j).
__device__ __forceinline__ void c16_symmetrize(double* A, int nb) {
    for (int e = threadIdx.x; e < nb * 120; e += blockDim.x) {
        const int I = e / 120;
        int q = e - I * 120;
        const int c = (int)((1.0f + __builtin_sqrtf((float)(1 + 8 * q))) * 0.5f);   // q = c (c - 1) / 2 + r, r < c <= 15 (exact: 1 + 8 q <= 953)
        q -= (c * (c - 1)) >> 1;
        double* t = A + (c16_tile(I, I) << 8);
        t[c * 16 + q] = t[q * 16 + c];
    }
}

// The same for the diagonal tiles I0 <= I < I1 alone, on the nt threads t = 0 .. nt - 1 (a caller that lets the pivot wave mirror
// tile (0, 0) by itself and start on it while the other waves mirror the rest).
__device__ __forceinline__ void c16_symmetrize_tiles(double* A, int I0, int I1, int t0, int nt) {
    for (int e = t0; e < (I1 - I0) * 120; e += nt) {
        const int I = e / 120;
        int q = e - I * 120;
        const int c = (int)((1.0f + __builtin_sqrtf((float)(1 + 8 * q))) * 0.5f);
        q -= (c * (c - 1)) >> 1;
        double* t = A + (c16_tile(I0 + I, I0 + I) << 8);
        t[c * 16 + q] = t[q * 16 + c];
    }
}

// One diagonal tile mirrored by one wave, in front of its own c16_load of that tile: lane (i, k) reads the elements (i, 4 s + k)
// (the X layout: conflict-free) and stores those below the diagonal to their mirror places. No index arithmetic to speak of:
// the e -> (row, column) decoding above is some 45 instructions per element, which here would stand in front of the first pivot.
__device__ __forceinline__ void c16_symmetrize_wave(double* t, int ln) {
    const int i = ln & 15, k = ln >> 4;
    const c16_d4 v = c16_load(t, ln);
#pragma unroll
    for (int s = 0; s < 4; s++)
        if (i > 4 * s + k) t[i * 16 + 4 * s + k] = v[s];
}

// ---- one 4-column step ------------------------------------------------------------------------------------------------
// The 4 x 4 pivot block P = D[4S .. 4S+3][4S .. 4S+3] is made uniform (v_readlane or an LDS broadcast), its Cholesky factor
// L_ss and M = L_ss^-1 are computed in every lane; M goes into an MFMA A operand "Mpad" (lane (r < 4, k): M[r][k]) so that
//     y = (tile register of the step) L_ss^-T  =  first accumulator register of  mfma(A = Mpad, B = register)
// for the diagonal tile AND for every panel tile: the replay is two MFMAs per step, no cross-lane VALU work.
// No sign test on the pivots: a non-positive pivot turns into NaN / inf (v_rsq_f64) and reaches the solution, which the
// caller tests; columns >= nreal are dummies (inverse 0: they neither change nor produce anything).
struct C16Lane {          // per-lane constants
    int e;                // Mpad select: index into the 10 entries of M (row-major lower: 00 10 11 20 21 22 30 31 32 33) or -1
    double k0, k1, k2, k3;   // 1.0 where lane / 16 == q: the lane's own column of a step, selected by multiplication
    double w[10];            // 1.0 for the lane's entry of M (Mpad), else 0
    long long* dbg;          // probe builds: timestamps inside the first pivot steps (null in the library)
};
__device__ __forceinline__ void c16_stamp(const C16Lane& lc, int slot, double& tie) {
    if (lc.dbg) {
        asm volatile("s_nop 0" : "+v"(tie) :: "memory");
        long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        asm volatile("s_nop 0" : "+v"(tie) :: "memory");
        if ((threadIdx.x & 63) == 0) lc.dbg[slot] = t;
    }
}
__device__ __forceinline__ C16Lane c16_lane(int ln) {
    const int r = ln & 15, k = ln >> 4;
    C16Lane c;
    c.e = (r < 4 && k <= r) ? (r * (r + 1) / 2 + k) : -1;
    c.k0 = k == 0 ? 1.0 : 0.0; c.k1 = k == 1 ? 1.0 : 0.0; c.k2 = k == 2 ? 1.0 : 0.0; c.k3 = k == 3 ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 10; q++) c.w[q] = c.e == q ? 1.0 : 0.0;
    c.dbg = nullptr;
    return c;
}

template <int S, int GATHER>
__device__ __forceinline__ void c16_gather(double u, double* gbuf, int ln, double (&a)[10]) {
    if (GATHER == 0) {
        // D[4S + r][4S + c] (r >= c) = D[4S + c][4S + r] sits in lane 16 r + 4 S + c
        a[0] = readlane_f64(u, 4 * S);
        a[1] = readlane_f64(u, 16 + 4 * S); a[2] = readlane_f64(u, 16 + 4 * S + 1);
        a[3] = readlane_f64(u, 32 + 4 * S); a[4] = readlane_f64(u, 32 + 4 * S + 1); a[5] = readlane_f64(u, 32 + 4 * S + 2);
        a[6] = readlane_f64(u, 48 + 4 * S); a[7] = readlane_f64(u, 48 + 4 * S + 1); a[8] = readlane_f64(u, 48 + 4 * S + 2);
        a[9] = readlane_f64(u, 48 + 4 * S + 3);
    } else {
        gbuf[ln] = u;      // wave-private 64 doubles; same-wave LDS accesses complete in order
        const double2 r1 = *(const double2*)(gbuf + 16 + 4 * S), r2 = *(const double2*)(gbuf + 32 + 4 * S);
        const double2 r3 = *(const double2*)(gbuf + 48 + 4 * S), r3b = *(const double2*)(gbuf + 48 + 4 * S + 2);
        a[0] = gbuf[4 * S]; a[1] = r1.x; a[2] = r1.y; a[3] = r2.x; a[4] = r2.y; a[5] = gbuf[32 + 4 * S + 2];
        a[6] = r3.x; a[7] = r3.y; a[8] = r3b.x; a[9] = r3b.y;
    }
}

template <int S, int GATHER>
__device__ __forceinline__ void c16_pivot_step(c16_d4& D, c16_d4& E, c16_d4& W, double& mp_io, double& y_io, int nreal, double* pub, double* gbuf, int ln, const C16Lane& lc) {
    double u = D[S];
    c16_stamp(lc, 8 * S + 0, u);
    double a0, a1, a2, a3;   // the 4 entries of the lane's row (independent of the factor)
    double a[10];
    c16_d4 zw = {0.0, 0.0, 0.0, 0.0};
    if (GATHER == 0) {
        double ev, od;
        swap16_pair_f64(u, ev, od);
        swap32_pair_f64(ev, a0, a2);
        swap32_pair_f64(od, a1, a3);
        c16_stamp(lc, 8 * S + 1, a3);
        c16_gather<S, 0>(u, gbuf, ln, a);
    } else {
        gbuf[ln] = u;          // wave-private; same-wave LDS accesses complete in order
        const double* row = gbuf + (ln & 15);
        if (S > 0) zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp_io, E[S - 1], zw, 0, 0, 0);   // the previous step on the identity tile, see below
        a0 = row[0]; a1 = row[16]; a2 = row[32]; a3 = row[48];
        const double2 r1 = *(const double2*)(gbuf + 16 + 4 * S), r2 = *(const double2*)(gbuf + 32 + 4 * S);
        const double2 r3 = *(const double2*)(gbuf + 48 + 4 * S), r3b = *(const double2*)(gbuf + 48 + 4 * S + 2);
        a[0] = gbuf[4 * S]; a[1] = r1.x; a[2] = r1.y; a[3] = r2.x; a[4] = r2.y; a[5] = gbuf[32 + 4 * S + 2];
        a[6] = r3.x; a[7] = r3.y; a[8] = r3b.x; a[9] = r3b.y;
        c16_stamp(lc, 8 * S + 1, a3);
    }
    c16_stamp(lc, 8 * S + 2, a[9]);
    const double i0 = nreal > 0 ? rsqrt_nr(a[0]) : 0.0;
    const double l10 = a[1] * i0, l20 = a[3] * i0, l30 = a[6] * i0;
    const double i1 = nreal > 1 ? rsqrt_nr(__builtin_fma(-l10, l10, a[2])) : 0.0;
    const double l21 = __builtin_fma(-l20, l10, a[4]) * i1, l31 = __builtin_fma(-l30, l10, a[7]) * i1;
    const double i2 = nreal > 2 ? rsqrt_nr(__builtin_fma(-l21, l21, __builtin_fma(-l20, l20, a[5]))) : 0.0;
    const double l32 = __builtin_fma(-l31, l21, __builtin_fma(-l30, l20, a[8])) * i2;
    double i3 = nreal > 3 ? rsqrt_nr(__builtin_fma(-l32, l32, __builtin_fma(-l31, l31, __builtin_fma(-l30, l30, a[9])))) : 0.0;
    c16_stamp(lc, 8 * S + 3, i3);
    if (GATHER == 1 && S > 0) {   // the matrix pipe finished zw during the factor chain
        W[S - 1] = zw[0];
        E = __builtin_amdgcn_mfma_f64_16x16x4f64(-y_io, zw[0], E, 0, 0, 0);
    }
    // y = (row's 4 entries) L_ss^-T by forward substitution; the lane keeps its own column
    const double y0 = a0 * i0;
    const double y1 = __builtin_fma(-l10, y0, a1) * i1;
    const double y2 = __builtin_fma(-l21, y1, __builtin_fma(-l20, y0, a2)) * i2;
    const double y3 = __builtin_fma(-l32, y2, __builtin_fma(-l31, y1, __builtin_fma(-l30, y0, a3))) * i3;
    double y = __builtin_fma(lc.k3, y3, __builtin_fma(lc.k2, y2, __builtin_fma(lc.k1, y1, lc.k0 * y0)));
    c16_stamp(lc, 8 * S + 4, y);
    if (S < 3) D = __builtin_amdgcn_mfma_f64_16x16x4f64(-y, y, D, 0, 0, 0);
    if (S < 3) { double t = D[S + 1]; c16_stamp(lc, 8 * S + 5, t); D[S + 1] = t; }
    // for the other waves (in the shadow of the MFMA): M = L_ss^-1 as an MFMA A operand
    const double m10 = -(l10 * i0) * i1;
    const double m21 = -(l21 * i1) * i2;
    const double m32 = -(l32 * i2) * i3;
    const double m20 = -__builtin_fma(l21, m10, l20 * i0) * i2;
    const double m31 = -__builtin_fma(l32, m21, l31 * i1) * i3;
    const double m30 = -__builtin_fma(l32, m20, __builtin_fma(l31, m10, l30 * i0)) * i3;
    double mp;   // the lane's entry of M by multiplication with 0 / 1 weights (half the instructions of a select chain)
    mp = lc.w[0] * i0;
    mp = __builtin_fma(lc.w[1], m10, mp); mp = __builtin_fma(lc.w[2], i1, mp); mp = __builtin_fma(lc.w[3], m20, mp);
    mp = __builtin_fma(lc.w[4], m21, mp); mp = __builtin_fma(lc.w[5], i2, mp); mp = __builtin_fma(lc.w[6], m30, mp);
    mp = __builtin_fma(lc.w[7], m31, mp); mp = __builtin_fma(lc.w[8], m32, mp); mp = __builtin_fma(lc.w[9], i3, mp);
    c16_stamp(lc, 8 * S + 6, mp);
    pub[S * C16_STEP + ln] = y;
    // The same step on the identity tile E (after the four steps W = I L_kk^-T) is two MFMAs, zw = M E[S] and E -= y zw^T.
    // They are issued one step LATE, inside the next step (zw before its factor chain, the update after it), so that the
    // matrix pipe works under VALU instructions the wave has to issue anyway instead of stalling it; the last step's is
    // finished by c16_pivot_block.
    if (GATHER == 0) {
        c16_d4 zw = {0.0, 0.0, 0.0, 0.0};
        zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp, E[S], zw, 0, 0, 0);
        W[S] = zw[0];
        if (S < 3) E = __builtin_amdgcn_mfma_f64_16x16x4f64(-y, zw[0], E, 0, 0, 0);
    }
    mp_io = mp; y_io = y;
}

// Factor the diagonal tile D (nreal real pivot columns): publishes the steps' y, returns X(L_kk^-T).
// A 4-column step whose columns are ALL dummies (4 S >= nreal: the last block column of a system whose size is not a multiple
// of 16) would compute y = 0, M = 0, W[S] = 0 and leave D alone: it is skipped (a step is ~1 000 cycles of pivot chain;
// N = 114 has three of them in its last block column).
template <int GATHER>
__device__ __forceinline__ c16_d4 c16_pivot_block(c16_d4 D, int nreal, double* pub, double* gbuf, int ln, const C16Lane& lc) {
    c16_d4 E, W = {0.0, 0.0, 0.0, 0.0};
    const int i = ln & 15, k = ln >> 4;
#pragma unroll
    for (int s = 0; s < 4; s++) E[s] = (i == 4 * s + k) ? 1.0 : 0.0;
    double mp = 0.0, y = 0.0;
    c16_d4 zw = {0.0, 0.0, 0.0, 0.0};
    c16_pivot_step<0, GATHER>(D, E, W, mp, y, nreal, pub, gbuf, ln, lc);
    if (nreal > 4) {
        c16_pivot_step<1, GATHER>(D, E, W, mp, y, nreal - 4, pub, gbuf, ln, lc);
        if (nreal > 8) {
            c16_pivot_step<2, GATHER>(D, E, W, mp, y, nreal - 8, pub, gbuf, ln, lc);
            if (nreal > 12) {
                c16_pivot_step<3, GATHER>(D, E, W, mp, y, nreal - 12, pub, gbuf, ln, lc);
                if (GATHER == 1) { zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp, E[3], zw, 0, 0, 0); W[3] = zw[0]; }
            } else {
                if (GATHER == 1) { zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp, E[2], zw, 0, 0, 0); W[2] = zw[0]; }
                W[3] = 0.0; pub[3 * C16_STEP + ln] = 0.0;
            }
        } else {
            if (GATHER == 1) { zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp, E[1], zw, 0, 0, 0); W[1] = zw[0]; }
            W[2] = 0.0; W[3] = 0.0; pub[2 * C16_STEP + ln] = 0.0; pub[3 * C16_STEP + ln] = 0.0;
        }
    } else {
        if (GATHER == 1) { zw = __builtin_amdgcn_mfma_f64_16x16x4f64(mp, E[0], zw, 0, 0, 0); W[0] = zw[0]; }
        W[1] = 0.0; W[2] = 0.0; W[3] = 0.0;
        pub[1 * C16_STEP + ln] = 0.0; pub[2 * C16_STEP + ln] = 0.0; pub[3 * C16_STEP + ln] = 0.0;
    }
    return W;
}

// X(L_kk^-T) -> its tile (for the back-substitution, X layout) and the padded transposed buffer (for the panel products)
__device__ __forceinline__ void c16_publish_w(double* tile, double* wt, int ln, c16_d4 W) {
    c16_store(tile, ln, W);
    const int i = ln & 15, k = ln >> 4;
#pragma unroll
    for (int s = 0; s < 4; s++) wt[(4 * s + k) * 17 + i] = W[s];    // element (r = i, c = 4 s + k)
}

// L_Ik = A_Ik L_kk^-T: X(Q P^T) = sum_s mfma(A = X(P)[s], B = X(Q)[s]) with Q = A_Ik and P = L_kk^-1, whose X layout
// (lane (i, k), register s: L_kk^-1[i][4 s + k] = L_kk^-T[4 s + k][i]) is the transposed read of the buffer
__device__ __forceinline__ c16_d4 c16_panel(c16_d4 X, const double* wt, int ln) {
    const int i = ln & 15, k = ln >> 4;
    const double* w = wt + i * 17 + k;
    c16_d4 Y = {0.0, 0.0, 0.0, 0.0}, Y2 = {0.0, 0.0, 0.0, 0.0};
    Y = __builtin_amdgcn_mfma_f64_16x16x4f64(w[0], X[0], Y, 0, 0, 0);
    Y2 = __builtin_amdgcn_mfma_f64_16x16x4f64(w[4], X[1], Y2, 0, 0, 0);
    Y = __builtin_amdgcn_mfma_f64_16x16x4f64(w[8], X[2], Y, 0, 0, 0);
    Y2 = __builtin_amdgcn_mfma_f64_16x16x4f64(w[12], X[3], Y2, 0, 0, 0);
    return Y + Y2;
}

// H = L_IJ L_JJ^-1 (stored transposed) in place of a panel tile (the diagonal tile holds X(L_JJ^-T)): with it the back-substitution is
// x_J = z_J - sum_{I > J} H_IJ^T x_I with z = the right-hand-side row of H — no triangular solve per block.
__device__ __forceinline__ void c16_to_h(double* A, int I, int J, int ln) {
    double* t = A + (c16_tile(I, J) << 8);
    const c16_d4 L = c16_load(t, ln);
    const c16_d4 W = c16_load(A + (c16_tile(J, J) << 8), ln);
    // operands swapped: the accumulator then holds H^T, i.e. the tile is stored TRANSPOSED (H[i][c] at i * 16 + c): the
    // back-substitution reads, for a fixed row i, the 16 columns of a tile with unit stride across lanes (no bank conflicts;
    // the column-major tile put the 64 lanes' 16-byte reads 128 bytes apart)
    c16_d4 H = {0.0, 0.0, 0.0, 0.0}, H2 = {0.0, 0.0, 0.0, 0.0};
    H = __builtin_amdgcn_mfma_f64_16x16x4f64(L[0], W[0], H, 0, 0, 0);
    H2 = __builtin_amdgcn_mfma_f64_16x16x4f64(L[1], W[1], H2, 0, 0, 0);
    H = __builtin_amdgcn_mfma_f64_16x16x4f64(L[2], W[2], H, 0, 0, 0);
    H2 = __builtin_amdgcn_mfma_f64_16x16x4f64(L[3], W[3], H2, 0, 0, 0);
    c16_store(t, ln, H + H2);
}

// ---- back-substitution, one block: the 16 owners of x_I publish it, one workgroup barrier, every thread c < 16 I subtracts
// H_I,J(c)^T x_I. hc: the thread's 16 values of H_I,J(c) (requested a step ago); hn receives those of step I - 1 ----
__device__ __forceinline__ void c16_back_hcol(const double* A, int I, int tid, double (&h)[16]) {
    const double* ht = A + (c16_tile(I, tid >> 4) << 8) + (tid & 15);
#pragma unroll
    for (int i = 0; i < 16; i++) h[i] = ht[i * 16];
}
__device__ __forceinline__ bool c16_back_step(const double* A, double* yv, double* xs, int N, int I, int tid, const double (&hc)[16], double (&hn)[16], double& z, bool& bad) {
    if ((tid >> 4) == I) {
        yv[tid] = z;
        if (tid < N) { xs[tid] = z; if (!(fabs(z) < 1e300)) bad = true; }
    }
    if (I == 0) return false;
    __syncthreads();
    if (tid < 16 * I) {
        double xv[16];
#pragma unroll
        for (int i = 0; i < 16; i++) xv[i] = yv[16 * I + i];
        // the owners of x_{I-1} (16 (I - 1) <= tid < 16 I) have no column at step I - 1: they read the diagonal tile
        // (I - 1, I - 1), inside the image, and drop it — one instruction stream for the whole wave, no branch around the loads
        c16_back_hcol(A, I - 1, tid, hn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 16; i++) z = __builtin_fma(-hc[i], xv[i], z);
    }
    return true;
}

// Solve [S] x = rhs for the tile-packed image A (N columns, rhs = row N; diagonal tiles already symmetric). On return
// xs[0 .. N) = S^-1 rhs. Every thread of the 512-thread workgroup must call it. pub: C16_WORK doubles; yv: 16 * nb
// doubles. Returns false if the solution is not finite (a non-positive pivot). ts (may be null): phase timestamps.
// SOLVE = false stops after the factorisation: the panel tiles hold L_IJ, the diagonal tiles L_JJ^-T, the tiles of row N the
// forward-substituted right-hand side (L^-1 rhs)^T in their first rows — what the wide-panel dense solver takes (dense_chol.h).
// old_tail (uniform; SADVIO_C16_OLD_TAIL, A/B): the last block column keeps both of its barriers and converts the panel of the
// column before it, as every other block column does. Same bits either way. ts[1 + 2 kb], ts[2 + 2 kb]: end of the phases of
// block column kb < 8 (a skipped phase repeats the stamp before it), ts[18] .. ts[19]: the back-substitution from the barrier in
// front of it to its last step, ts[20]: the end.
//
// c16_solve_hooked: the same with a caller's hook, for work that wants to run in the shadow of the first block column instead of in
// front of the first pivot block (k_solve's end-of-solve test):
//   hook.under_first_panel()   every thread calls it behind the first workgroup barrier, in front of phase A of block column 0;
//   hook.ended()               every thread calls it behind the barrier in front of the back-substitution and must get the same answer;
//                              on true every thread returns true at once. (Asked behind the barrier that closes the first panel
//                              instead, an exit inside the loop, every panel phase ran ~100 cycles longer and the gain was gone:
//                              docs/KERNEL_HISTORY.md "k_solve's front half under the first pivot block".)
// No barrier is added, none is skipped by one wave alone, the loop over the block columns is untouched. C16NoHook does nothing:
// c16_solve is the code it was.
struct C16NoHook {
    __device__ __forceinline__ void under_first_panel() {}
    __device__ __forceinline__ bool ended() { return false; }
};
template <int GATHER = 1, bool SOLVE = true, class HOOK>
__device__ __forceinline__ bool c16_solve_hooked(double* A, int N, double* xs, double* pub, double* yv, long long* ts, long long* dbg, bool old_tail, HOOK& hook) {
    const int tid = threadIdx.x, ln = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = blockDim.x >> 6;
    const int nb = c16_blocks(N + 1);     // tile rows incl. the right-hand-side row
    const int nbc = c16_blocks(N);        // block columns with real pivots
    C16Lane lc = c16_lane(ln);
    lc.dbg = dbg;
    double* gbuf = pub + 2 * C16_PUB;     // the pivot wave's gather buffer
    double* wt = gbuf + 64;               // L_kk^-T of the block just factored, transposed read
    __shared__ int s_bad;
    if (tid == 0) s_bad = 0;
    c16_d4 D = {0.0, 0.0, 0.0, 0.0};      // pivot wave: the next diagonal tile
    if (wv == 0) c16_publish_w(A, wt, ln, c16_pivot_block<GATHER>(c16_load(A, ln), N < 16 ? N : 16, pub, gbuf, ln, lc));
    __syncthreads();
    long long tlast = 0;                  // the last stamp written (repeated for a skipped phase)
    if (ts && tid == 0) ts[0] = tlast = clock64();
    static_assert(SOLVE || std::is_same<HOOK, C16NoHook>::value, "a hook needs SOLVE = true: the barrier that closes SOLVE = false does not ask it");
    hook.under_first_panel();
    for (int kb = 0; kb < nbc; kb++) {
        const int m = nb - kb - 1;        // tile rows below the diagonal tile
        // ---- phase A: L_Ik = A_Ik L_kk^-T, one product per panel tile. The pivot wave takes the tile it needs next,
        //      (kb + 1, kb), and updates the next diagonal tile with it ----
        if (wv == 0) {
            if (m >= 1) {
                double* tp = A + (c16_tile(kb + 1, kb) << 8);
                const c16_d4 Y = c16_panel(c16_load(tp, ln), wt, ln);
                c16_store(tp, ln, Y);
                if (kb + 1 < nbc) {
                    D = c16_load(A + (c16_tile(kb + 1, kb + 1) << 8), ln);
                    c16_d4 D2 = {0.0, 0.0, 0.0, 0.0};     // two accumulators: two dependent MFMAs instead of four
                    D = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[0], Y[0], D, 0, 0, 0);
                    D2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[1], Y[1], D2, 0, 0, 0);
                    D = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[2], Y[2], D, 0, 0, 0);
                    D2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[3], Y[3], D2, 0, 0, 0);
                    D += D2;
                }
            }
        } else {
            for (int I = kb + 1 + wv; I < nb; I += nwv - 1) {
                double* tp = A + (c16_tile(I, kb) << 8);
                c16_store(tp, ln, c16_panel(c16_load(tp, ln), wt, ln));
            }
        }
        if (!old_tail && kb == nbc - 1) {
            // the last block column: its panel is at most the right-hand side's tile (m = 1), the pivot wave's above, which no
            // other wave touches before the barrier in front of the back-substitution; phase B has nothing (the panel of block
            // column kb - 1 became H one phase early, below)
            if (ts && tid == 0 && kb < 8) { ts[1 + 2 * kb] = tlast; ts[2 + 2 * kb] = tlast; }
            break;
        }
        __syncthreads();
        if (ts && tid == 0 && kb < 8) ts[1 + 2 * kb] = tlast = clock64();
        // ---- phase B: factorisation of the next diagonal tile (look-ahead) | trailing update of everything else, and the
        //      panel of the PREVIOUS block column (no longer needed as L) turned into H = L L_JJ^-1 ----
        if (wv == 0) {
            if (kb + 1 < nbc) {
                const int left = N - 16 * (kb + 1);
                const c16_d4 W = c16_pivot_block<GATHER>(D, left < 16 ? left : 16, pub + ((kb + 1) & 1) * C16_PUB, gbuf, ln, lc);
                c16_publish_w(A + (c16_tile(kb + 1, kb + 1) << 8), wt, ln, W);   // wt: every wave is past its phase-A reads (barrier)
            }
        } else {
            // tiles (I, J), kb < J <= I, J < nbc, minus the pivot wave's (kb + 1, kb + 1), dealt round-robin in row order.
            // The wave that shares the pivot wave's SIMD (wave nwv / 2 with waves placed round-robin on the 4 SIMDs) stays
            // out of it: whatever it issues is taken from the pivot chain (+40 % on a pivot step, measured)
            // ... unless the trailing update is the longer side (many tile rows left: N > ~130)
            const bool all = (nb - kb) * (nb - kb - 1) / 2 > 4 * (nwv - 2) + 2;
            const int nbw = all ? nwv - 1 : nwv - 2;                   // bulk waves of this phase
            const int bw = (all || wv < nwv / 2) ? wv - 1 : wv - 2;    // index among them
            if (all || wv != nwv / 2) {
                int I = kb + 1, J = kb + 2 + bw;
                while (true) {
                    int jmax = I < nbc ? I : nbc - 1;
                    while (I < nb && J > jmax) { J -= jmax - kb; I++; jmax = I < nbc ? I : nbc - 1; }   // row I holds jmax - kb tiles
                    if (I >= nb) break;
                    double* ct = A + (c16_tile(I, J) << 8);
                    c16_d4 C = c16_load(ct, ln);
                    const c16_d4 LI = c16_load(A + (c16_tile(I, kb) << 8), ln);
                    const c16_d4 LJ = c16_load(A + (c16_tile(J, kb) << 8), ln);
                    c16_d4 C2 = {0.0, 0.0, 0.0, 0.0};
                    C = __builtin_amdgcn_mfma_f64_16x16x4f64(-LJ[0], LI[0], C, 0, 0, 0);
                    C2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-LJ[1], LI[1], C2, 0, 0, 0);
                    C = __builtin_amdgcn_mfma_f64_16x16x4f64(-LJ[2], LI[2], C, 0, 0, 0);
                    C2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-LJ[3], LI[3], C2, 0, 0, 0);
                    c16_store(ct, ln, C + C2);
                    J += nbw;
                }
                if (SOLVE && kb >= 1)
                    for (int Ic = kb + (nbw - 1 - bw); Ic < nb; Ic += nbw) c16_to_h(A, Ic, kb - 1, ln);   // last waves first: they got fewer tiles above
                // The last block column but one: the only trailing tile left to the bulk waves is (nbc, nbc - 1), the first
                // bulk wave's (none when the right-hand side shares the last diagonal tile), and the pivot wave read (kb + 1, kb)
                // in phase A. That wave turns THIS column's panel into H after its own reads of it (c16_to_h reads and writes
                // the addresses the same lane read as LI / LJ): nothing is left for the last block column's phase B
                if (SOLVE && !old_tail && kb == nbc - 2 && bw == 0)
                    for (int Ic = kb + 1; Ic < nb; Ic++) c16_to_h(A, Ic, kb, ln);
            }
        }
        __syncthreads();
        if (ts && tid == 0 && kb < 8) ts[2 + 2 * kb] = tlast = clock64();
    }
    if (!SOLVE) { __syncthreads(); return true; }
    // the last block column's panel (at most the tile row of the right-hand side when N is a multiple of 16): the pivot wave's,
    // as its phase A was
    if (wv == 0 && nbc < nb) c16_to_h(A, nbc, nbc - 1, ln);
    // ---- back-substitution. z_c = H[N][c] = (L_JJ^-T y_J)[c]; x_I = z_I once the blocks above are in; then every thread
    //      c < 16 I subtracts H_I,J(c)^T x_I (16 consecutive doubles of tile (I, c / 16)): I descending, i ascending ----
    const int IB = N >> 4, r = N & 15;
    __syncthreads();
    if (hook.ended()) return true;
    if (ts && tid == 0) ts[18] = clock64();
    double z = 0.0;
    if (tid < N) {
        const int J = tid >> 4, cl = tid & 15;
        if (J < IB) z = A[(c16_tile(IB, J) << 8) + r * 16 + cl];   // H tiles are stored transposed (c16_to_h)
    }
    if (r > 0 && (tid >> 4) == IB) {       // the block that shares its diagonal tile with the right-hand side: z = L_JJ^-T y_J
        const int cl = tid & 15;
        yv[tid] = tid < N ? pub[(IB & 1) * C16_PUB + (cl >> 2) * C16_STEP + 16 * (cl & 3) + r] : 0.0;   // lane (row r, k = cl & 3) of step cl / 4
        const double* lt = A + (c16_tile(IB, IB) << 8) + cl;
        const double* v = yv + 16 * IB;
        double xi = 0.0;
#pragma unroll
        for (int c = 0; c < 16; c++) xi = __builtin_fma(lt[c * 16], v[c], xi);
        z = tid < N ? xi : 0.0;
    }
    bool bad = false;
#ifdef SADVIO_C16_PARENT_ORDER
    for (int I = nbc - 1; I >= 0; I--) {
        double hcol[16];
        if (tid < 16 * I) {                // issued before the barrier: independent of x_I
            const double* ht = A + (c16_tile(I, tid >> 4) << 8) + (tid & 15);
#pragma unroll
            for (int i = 0; i < 16; i++) hcol[i] = ht[i * 16];
        }
        if ((tid >> 4) == I) {
            yv[tid] = z;
            if (tid < N) { xs[tid] = z; if (!(fabs(z) < 1e300)) bad = true; }
        }
        if (I == 0) break;
        __syncthreads();
        if (tid < 16 * I) {
            // all of x_I on the way before the first FMA: left to itself the compiler loads it four values at a time between
            // the FMAs that use them and exposes the LDS latency five times per block instead of once
            double xv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) xv[i] = yv[16 * I + i];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; i++) z = __builtin_fma(-hcol[i], xv[i], z);
        }
    }
#else
    // The H column of a step is requested ONE STEP AHEAD, behind the reads of x of the step before it: LDS reads retire in order, so
    // the FMAs wait for x_I alone, the column of step I - 1 lands under them, and the owners' store of x_{I-1} follows the last FMA
    // with no wait in front of it. Two register buffers, the loop body twice.
    double h0[16], h1[16];
    if (nbc >= 1 && tid < 16 * (nbc - 1)) c16_back_hcol(A, nbc - 1, tid, h0);
    for (int I = nbc - 1; I >= 0; I -= 2) {
        if (!c16_back_step(A, yv, xs, N, I, tid, h0, h1, z, bad)) break;
        if (!c16_back_step(A, yv, xs, N, I - 1, tid, h1, h0, z, bad)) break;
    }
#endif
    if (ts && tid == 0) ts[19] = clock64();
    if (bad) s_bad = 1;
    __syncthreads();
    if (ts && tid == 0) ts[20] = clock64();
    return s_bad == 0;
}
template <int GATHER = 1, bool SOLVE = true>
__device__ __forceinline__ bool c16_solve(double* A, int N, double* xs, double* pub, double* yv, long long* ts, long long* dbg = nullptr, bool old_tail = false) {
    C16NoHook none;
    return c16_solve_hooked<GATHER, SOLVE>(A, N, xs, pub, yv, ts, dbg, old_tail, none);
}

}  // namespace sadvio

// step_args.h — what every kernel of the LM step is handed: the DevPtrs argument block, the in-kernel phase-timestamp macros,
// index helpers of the reduced system and the two global atomics.
#pragma once
#include "ba_types.h"
#include "chol16.h"

namespace sadvio {

struct DevPtrs {
    const WinDev* win;
    const Tile* tiles;
    const double* kf_T0;
    const int* kf_fidx;
    double* xp; double* xv; double* xba; double* xbg;  // [2][...]
    long long xp_stride, xv_stride, xl_stride;
    const double* kf_vel; const double* kf_ba; const double* kf_bg;
    const double* cam_K; const double* cam_T; const double* cam_isig;
    const double* lmk_p; double* xl; double* s_lmk;
    const unsigned char* lmk_const;
    const int* lmk_ob; const int* lmk_oe;
    const int* obs_kf; const int* obs_cam; const double* obs_meas;
    const unsigned char* obs_slot;  // index of the observation's key-frame in its tile's list
    const int* tile_kf;             // per-tile key-frame lists (global indices)
    const int* tile_lmk;            // landmark lists of the packed tiles (Tile::lmk_off)
    const int* tile_row;            // matching row in the tile's LDS system (6 * rank among free) or -1
    // first-round packets (k_pre_packets; null for submissions of more than PRE_MAX_TILES tiles): per (tile, 8 consecutive lanes — a landmark's
    // lane group is 8 .. 64 wide) | landmark | its first observation | its observation count + (1 << 16 if the landmark exists) | position of the
    // 8 lanes' first one inside the group |,
    // per (tile, k < PRE_KF) | global key-frame or -1 | its free index |: the opening loads of k_build / k_backsub hang on blockIdx alone
    const int4* pre_lane;
    const int2* pre_kf;
    double* ptab;                   // [2][n_kf_tot][POSE_TAB] pose tables of the two delta buffers
    long long ptab_stride;
    const PriorDev* priors;
    double* prior_lin;              // [2][n_prior_tot][PRIOR_LIN] g = J^T r (6) | H = J^T J lower (21) | |r|^2 of every pose prior at the x of
    long long prior_lin_stride;     // each delta buffer: written at x = 0 by k_init_tables, at the candidate by k_solve's back half
    int n_prior_tot;
    const ImuDev* imus;
    double* imu_scratch;  // [2][n_imu_tot][IMU_ROW], see ba_types.h: the linearisation of every IMU factor pair at the deltas of buffer 0 | 1
    long long imu_scratch_stride;
    double* S; double* gred; double* gfull; double* hdiag; double* delta; double* s_pose;
    LmState* states;  // [n_win][slots+2]
    IterAcc* acc;     // [n_win][slots+1] window totals (written by single workgroups only)
    TileAcc* tacc;    // [2][n_tiles] per-tile partials, double-buffered by slot parity (no atomics)
    FinalRec* final_out;  // [n_win]
    int* big_info;        // [n_win] potrf info of the windows solved out of LDS
    // a window sharded over `world` GPUs (landmark partition): per-rank partial sums, exchanged with the reduced
    // system by one all-reduce per phase; rank r writes slot r and zeroes the others (sum == gather)
    int imu_direct;       // 1: imu_pair_lin_wg adds the IMU pairs' entries to the reduced system itself (one device); 0: k_solve's item loop
    int decide_kernel;    // 1: the LM decision of a slot is taken by k_decide (many tiles); 0: by every k_build workgroup
    int world, rank;
    double* rank_b;       // [n_win][world][4] lin_cost, fixed_cost, gmax, -      (after k_build)
    double* rank_s;       // [n_win][world][4] cand_cost, mcc, step_norm2, cand_norm2 (after k_backsub)
    const int* lmk_red;   // [n_lmk_tot] offset of a prior-kept landmark in its window's reduced vector, else -1 (may be null)
    const int* kept_obs;  // [n_kept][3] (device observation index, global landmark, window)
    int n_kept;
    double* dp_data;      // dense priors, see WinDev::dp_off
    const SparseDev* sparse;  // sparse prior factors
    const int* sp_list;       // indices (into sparse) of the factors the solve evaluates itself, per window slice
    double* sp_scratch;       // [2][n_sparse][SPARSE_J] r, J of the listed factors at the deltas of buffer 0 | 1 (as imu_scratch)
    long long sp_scratch_stride;
    int n_imu_tot, n_sp_list;  // extra workgroups of k_build / k_backsub: IMU factor pairs, then the listed sparse-prior factors
    const int* dp_ints;
    const int* chunk_ob;      // [n_chunks + 1] first observation of each chunk (lm_kernels.h)
    const int* chunk_lm;      // [n_chunks + 1] first landmark of each chunk
    const int* tile_perm;     // [n_tiles] launch order of the throughput kernels: tiles by decreasing chunk count
    const unsigned char* obs_lslot;  // [n_obs_tot] index of the observation's landmark inside its chunk
    double* lm_hg;            // [2][n_lmk_tot][9] H_ll | g_l of every landmark at the point of each delta buffer (k_lm_pass)
    double* lm_dt;            // [2][n_tiles][LM_DT] per tile: key-frame sums (sum Jp^T Jp, sum Jp^T r) + cost totals at each buffer's point
    long long lm_hg_stride, lm_dt_stride;
    const int* lm_sub;        // [n_sub][2] work list of k_lm_pass: tile | sub-block (LM_PASS_THREADS landmarks) of the tile, largest tiles first
    int lm_sub_per_item;      // sub-blocks one work item (workgroup) of k_lm_pass runs through
    int lm_ksub;              // record slots per tile (= the largest tile's sub-block count): lm_dt / lm_sacc are indexed tile * lm_ksub + sub-block
    double* lm_sacc;          // [2][n_tiles * lm_ksub][4] per sub-block and slot parity: cand_cost | mcc | step_norm2 | cand_norm2 (unused slots stay zero)
    const LineDev* lines;     // linexd landmarks: few, kept in the reduced system
    const LineObsDev* lobs;
    double* xline;            // [2][n_line_tot][6] line deltas, double-buffered like xp
    double* line_scratch;     // [n_lobs_tot][LINE_ROW]
    long long xline_stride;
    long long n_xp, n_xv, n_xl;  // doubles in the (double-buffered) delta arrays, zeroed by k_reset
    int n_tiles;
    int state_stride;
    int n_win;
    long long* t_start; // wall_clock64 at the first kernel of the solve (k_reset)
    double* trace;      // [n_win][state_stride][8] per-iteration log (sadvio_ba_get_trace), written by the slot's single decider
    long long* dbg_ts;  // [DBG_SLOTS] phase timestamps (wall_clock64, 100 MHz) of workgroup 0 when debug & 4096
    int debug;  // SADVIO_DEBUG env: bit 12 (4096) = in-kernel phase timestamps of workgroup 0 into dbg_ts (results unaffected)
    int c16_old_tail;   // 1 (SADVIO_C16_OLD_TAIL, A/B): chol16.h's last block column with both of its barriers
    SolveOpts o;
};

// In-kernel phase timestamps (SADVIO_DEBUG & 4096) exist only in a build with -DSADVIO_KERNEL_TS: even as not-taken
// branches they cost the latency-bound kernels ~1-2 us per launch (measured A/B on k_solve).
#ifdef SADVIO_KERNEL_TS
#define SADVIO_TS(slot_, idx_) do { if ((P.debug & 4096) && blockIdx.x == 0 && threadIdx.x == 0 && slot == (slot_)) P.dbg_ts[idx_] = wall_clock64(); } while (0)
#define SADVIO_TS_PTR(cond_) ((cond_) ? P.dbg_ts : nullptr)
// Per-workgroup record of one k_build launch (slot 3): | start | end | XCC id << 32 | HW_ID (gfx9 layout: SIMD 5:4, CU 11:8, SH 12,
// SE 15:13) | waves whose 8 landmarks list the same key-frames in the same lanes (`uniform`) << 32, most head lanes in a wave | behind the 128 phase slots. Shows which workgroups share a CU and when each of them ends (scripts/gpu_time_tiles.py).
constexpr int DBG_WG_MAX = 1024, DBG_WG_BASE = 128, DBG_SLOTS = DBG_WG_BASE + 4 * DBG_WG_MAX;
#define SADVIO_WG_TS(slot_, which_) do { if ((P.debug & 4096) && blockIdx.x < DBG_WG_MAX && threadIdx.x == 0 && slot == (slot_)) { \
        P.dbg_ts[DBG_WG_BASE + 4 * blockIdx.x + (which_)] = wall_clock64(); \
        if ((which_) == 0) P.dbg_ts[DBG_WG_BASE + 4 * blockIdx.x + 3] = 0; \
        if ((which_) == 0) P.dbg_ts[DBG_WG_BASE + 4 * blockIdx.x + 2] = ((long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) | (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)); } } while (0)
#else
#define SADVIO_TS(slot_, idx_) do { } while (0)
#define SADVIO_TS_PTR(cond_) nullptr
#define SADVIO_WG_TS(slot_, which_) do { } while (0)
constexpr int DBG_SLOTS = 128;
#endif

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j
// element (i >= j) of a window's reduced matrix in HBM: packed lower triangle (ld == 0) or full row-major
// ld == 0: the 16 x 16 tile-packed lower triangle of chol16.h (= the LDS image of k_solve<0>, so that its gather is a linear copy)
__device__ __forceinline__ long long s_index(int ld, int i, int j) { return ld ? (long long)i * ld + j : (long long)c16_index(i, j); }

__device__ __forceinline__ void atomic_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }

__device__ __forceinline__ void atomic_max_u64(unsigned long long* p, unsigned long long v) { atomicMax(p, v); }

}  // namespace sadvio

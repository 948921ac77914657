// ba_handle.h — the handle behind the C ABI (sadvio_ba_handle) and its helper structs: device buffers, the staged upload batch,
// the host copies of the caller's windows, the environment switches, the long-track switches, the state guard of the entry points
// (entry_state) and the kernel-class timers.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/sadvio_ba.h"
#include "kernels.h"
#include "layout_plan.h"
#include "dense_chol.h"
#include "marg_kernels.h"
#include "lm_kernels.h"
#include "long_kernels.h"
#include "viinit_kernels.h"
#include "nofov_kernels.h"
#include "cov_border_plan.h"

using namespace sadvio;

namespace {

#define HIP_TRY(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            h->err = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
            return SADVIO_E_HIP;                                                              \
        }                                                                                     \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        if (count <= n && p && !view) return hipSuccess;
        if (p && !view) (void)hipFree(p);
        view = false;
        p = nullptr; n = 0;
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    bool view = false;  // non-owning window into another buffer
    void set_view(T* ptr, size_t count) { if (p && !view) (void)hipFree(p); p = ptr; n = count; view = true; }
    void release() { if (p && !view) (void)hipFree(p); p = nullptr; n = 0; view = false; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(view, o.view); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
};

struct KernelClass {
    const char* name;
    double total_ms = 0;
    long long launches = 0;
};

}  // namespace

// RCCL (all-reduce of the reduced system over xGMI), loaded on first use: single-GPU solves never touch it.
struct NcclId { char internal[128]; };
struct RcclLib {
    void* lib = nullptr;
    void* comm = nullptr;
    int (*get_id)(NcclId*) = nullptr;
    int (*init_rank)(void**, int, NcclId, int) = nullptr;
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*destroy)(void*) = nullptr;
    const char* (*err_string)(int) = nullptr;
    int (*comm_count)(void*, int*) = nullptr;
    int (*comm_user_rank)(void*, int*) = nullptr;
    int (*comm_cu_device)(void*, int*) = nullptr;
};

// Host -> device uploads of one layout build are packed into ONE pinned staging buffer, copied with one
// hipMemcpyAsync and scattered to their destinations by one kernel: ~25 small pageable copies cost ~15 us each.
struct UploadItem { unsigned long long dst; unsigned long long off; unsigned long long bytes; };
__global__ void k_scatter_uploads(const char* stage, const UploadItem* items, int n_items) {
    for (int it = blockIdx.y; it < n_items; it += gridDim.y) {
        const UploadItem u = items[it];
        char* dst = (char*)u.dst;
        const char* src = stage + u.off;
        const unsigned long long words = u.bytes >> 3;  // staging offsets and device allocations are 8-byte aligned
        for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (unsigned long long)gridDim.x * blockDim.x)
            ((unsigned long long*)dst)[i] = ((const unsigned long long*)src)[i];
        if (blockIdx.x == 0 && threadIdx.x < (u.bytes & 7)) dst[(words << 3) + threadIdx.x] = src[(words << 3) + threadIdx.x];
    }
}
struct UploadBatch {
    std::vector<UploadItem> items;
    char* pinned = nullptr; size_t pinned_cap = 0, used = 0;   // sources are packed straight into pinned memory
    char* dev = nullptr; size_t dev_cap = 0;
    bool failed = false;
    bool trace = false;   // SADVIO_DEBUG & 8192: flush prints the size and FNV-1a hash of every item's payload (scripts/layout_same_uploads.py)
    // flush() does not wait: the staged copy + scatter are stream work like the kernels that read their output. The pinned buffer is
    // only touched again (next add / grow) after the event recorded behind the copy has fired — by then it normally has
    hipEvent_t ev = nullptr;
    bool in_flight = false;
    void wait() { if (in_flight) { (void)hipEventSynchronize(ev); in_flight = false; } }
    void reset() { wait(); items.clear(); used = 0; failed = false; }   // drop what an earlier, failed layout build left queued
    void reserve(size_t bytes) {
        if (bytes <= pinned_cap) return;
        wait();
        char* np = nullptr;
        const size_t cap = bytes + bytes / 2 + 4096;
        if (hipHostMalloc((void**)&np, cap, hipHostMallocDefault) != hipSuccess) { failed = true; return; }
        if (pinned) { memcpy(np, pinned, used); (void)hipHostFree(pinned); }
        pinned = np; pinned_cap = cap;
    }
    void add(void* dst, const void* src, size_t bytes) {
        if (!bytes) return;
        wait();
        const size_t off = (used + 7) & ~(size_t)7;
        reserve(off + bytes);
        if (failed) return;
        memcpy(pinned + off, src, bytes);
        used = off + bytes;
        items.push_back({(unsigned long long)dst, (unsigned long long)off, (unsigned long long)bytes});
    }
    hipError_t flush(hipStream_t stream) {
        if (failed) { failed = false; items.clear(); used = 0; return hipErrorOutOfMemory; }
        if (items.empty()) return hipSuccess;
        const size_t data_bytes = (used + 7) & ~(size_t)7;
        const size_t total = data_bytes + items.size() * sizeof(UploadItem);
        reserve(total);
        if (failed) { failed = false; items.clear(); used = 0; return hipErrorOutOfMemory; }
        if (trace)
            for (const UploadItem& u : items) {
                unsigned long long f = 0xcbf29ce484222325ULL;
                for (unsigned long long i = 0; i < u.bytes; i++) f = (f ^ (unsigned char)pinned[u.off + i]) * 0x100000001b3ULL;
                fprintf(stderr, "[sadvio dbg] upload %llu bytes fnv1a %016llx\n", u.bytes, f);
            }
        hipError_t e = hipSuccess;
        // every error return drops the queue: callers that do not reset() afterwards (marginalize, sparsify) must not re-send it
        auto drop = [&](hipError_t err) { items.clear(); used = 0; return err; };
        if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return drop(e);
        if (dev_cap < total) {
            if (dev) { (void)hipStreamSynchronize(stream); (void)hipFree(dev); }   // an earlier scatter may still read it
            dev = nullptr; dev_cap = 0;
            if ((e = hipMalloc((void**)&dev, total + total / 2)) != hipSuccess) return drop(e);
            dev_cap = total + total / 2;
        }
        memcpy(pinned + data_bytes, items.data(), items.size() * sizeof(UploadItem));
        if ((e = hipMemcpyAsync(dev, pinned, total, hipMemcpyHostToDevice, stream)) != hipSuccess) return drop(e);
        hipLaunchKernelGGL(k_scatter_uploads, dim3(64, (unsigned)std::min<size_t>(items.size(), 64)), dim3(256), 0, stream, dev, (const UploadItem*)(dev + data_bytes), (int)items.size());
        e = hipEventRecord(ev, stream);
        in_flight = e == hipSuccess;
        if (!in_flight) e = hipStreamSynchronize(stream);
        items.clear(); used = 0;
        return e;
    }
    ~UploadBatch() { wait(); if (ev) (void)hipEventDestroy(ev); if (pinned) (void)hipHostFree(pinned); if (dev) (void)hipFree(dev); }
};

// The handle's marginalisation prior: what the reference keeps in `_marginalization_last` inside the optimizer between
// marginalize() and the next window solve / the next marginalize() (AOptimizer.h:88-90, …Analytic.cpp:627-660). Device
// resident; the variables its columns refer to are named by the caller per window (it owns the id bookkeeping).
struct PriorState {
    bool valid = false;
    int n_full = 0, n = 0, form = 0, cut_mode = 0;   // cut_mode: the SADVIO_EIG_CUT_* it was built with (sparsify applies the same cut)
    DevBuf<double> J, r0;        // n_full x n row-major packed, n_full
    DevBuf<double> Z;            // n_full x n with Z^T Z = Sigma_k (built by the first sparsify of this prior)
    bool z_valid = false;
    DevBuf<int> step_of;         // Cholesky form: pivot step of every column
    DevBuf<double> H, g;         // J^T J = Ak and -J^T r0 = bk as the marginalisation that built the prior had them (full-rank Cholesky form only):
    bool hg_valid = false;       // the next marginalize / the next window's dense prior take them instead of re-forming J^T J (n^3 flops)
    unsigned long long serial = 0;   // bumped whenever the prior changes: a window that attached it checks it is still the same one
};

// Work buffers of marginalize / sparsify, kept in the handle: both run once per key-frame, and ~20 hipMalloc / hipFree pairs
// per call cost more than the kernels between them.
struct TriLevel { int first, count, max_m, max_n; };
struct MargScratch {
    DevBuf<double> A, b, G, V, ev, Vs, Ainv, T, Ak, bk, newJ, newr, lastJ, lastr, L, Tb, Zt, S, mi, jsel, lam, wtmp, Hl;
    DevBuf<int> ditems, flag, sel, lastcol, piv_of, lc, piv_mm;
    DevBuf<MargSmall> small;
    DevBuf<NfrSpecC> spec;
    std::vector<int> lcol, items, items_l, col;
    std::vector<double> hev, hsel, hS;
    struct TriPlan { DevBuf<TriNode> nodes; std::vector<TriLevel> levels; int leaves = 0; };
    std::map<int, TriPlan> tri_plans;   // node tables of the triangular inverse, by padded size (m of Amm and n of the prior alternate)
};

// Work buffers of sadvio_ba_covariance (cov_driver.h), kept in the handle like MargScratch: an odometry consumer calls it once per key-frame.
struct CovScratch {
    DevBuf<double> ptab, hll, hinv, ent_w, ent_hpp, S, Sig, lout, V, Lx, G, Z;
    DevBuf<int> status, ent_n, ent_col, step_of;
    DevBuf<int> is_long;   // windows with long tracks: the landmarks k_cov_long filled (cov_long_kernels.h)
    std::vector<double> h_sig, h_lout;
    // the band route (cov_band_kernels.h): L's band and the inverse pivot blocks | the solved columns of the out-of-band pairs | the
    // gathered blocks; the in-band pair table of k_cov_schur | the gather table | the pivot flag
    DevBuf<double> Lb, Linv, X, gout;
    DevBuf<int> pair_tab, gtab, xcol, bflag;
    // the border route (cov_border_kernels.h): the compacted band of B and of B^-1 | C, D | W, Z, T^-1 | [core | border] -> natural column;
    // the windows' plans (cov_border_plan.h), made by the first covariance call after a solve (border_known[w]) and dropped by the next
    // solve: every change of the layout passes a solve before a covariance call is served again
    DevBuf<double> bSb, bSigc, bCt, bDm, bW, bZ, bTinv;
    DevBuf<int> bperm;
    std::vector<int> h_bperm;
    std::vector<CovBorderPlan> border_plan;
    std::vector<char> border_known;
    std::vector<int> h_pair_tab, h_gtab, h_xcol;
    // the square-root assembly (cov_kernels.h: k_cov_assemble_sqrt): J_p and Q1 rows and the entry of every observation | the
    // key-frame -> landmark lists (cov_kf_lists.h)
    DevBuf<double> sq_jp, sq_q;
    DevBuf<int> sq_ent, kf_ptr, kf_lmk;
    std::vector<int> h_kf_ptr, h_kf_lmk;
};

// Work buffers of sadvio_ba_covariance_cross (cov_cross_driver.h), grown on demand: the call's tables in one int upload (plan order |
// workgroup table | request kf, lmk | global camera | block row of each candidate | band route: first column of each block row), the
// candidate measurements, the band route's solved block rows, and the results (cross | innov | maha2; status).
struct CovCrossScratch {
    DevBuf<int> ints, status;
    DevBuf<double> meas, rows, out;
    std::vector<int> h_ints, h_status;
    std::vector<double> h_out;
};

// Work buffers of sadvio_ba_covariance_batch (cov_batch_driver.h). The pools hold the work arrays (pool, ipool) and the results (rpool)
// of one group of windows and only ever grow; the pinned block holds the unit tables and receives every group's results, one copy
// per group, read after the call's one wait.
struct CovBatchScratch {
    DevBuf<double> pool, rpool, ptab;
    DevBuf<int> ipool;
    DevBuf<char> units;
    char* pinned = nullptr; size_t pinned_cap = 0;
    size_t tab_bytes = 0;   // of the current call's tables (units and long-track rows) in `units` and at the head of `pinned`
    hipError_t pin(size_t bytes) {
        if (bytes <= pinned_cap) return hipSuccess;
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinned_cap = 0;
        hipError_t e = hipHostMalloc((void**)&pinned, bytes + bytes / 2, hipHostMallocDefault);
        if (e == hipSuccess) pinned_cap = bytes + bytes / 2;
        return e;
    }
    CovBatchScratch() = default;
    CovBatchScratch(const CovBatchScratch&) = delete;
    CovBatchScratch& operator=(const CovBatchScratch&) = delete;
    ~CovBatchScratch() { if (pinned) (void)hipHostFree(pinned); }
};

// Work buffers of sadvio_ba_marginalize_relative_batch (rel_driver.h), grown on demand, and the per-key-frame landmark lists of one
// window: built by the first batch call on a layout, dropped with the layout (layout_build).
struct RelScratch {
    DevBuf<int> pairs, kf_ptr, kf_lmk, n_shared, status;   // pairs: [2][n_pair] kf_a | kf_b
    DevBuf<double> inf, Ak, Tab;
    std::vector<int> h_pairs, h_ptr, h_lmk, h_last;
    int csr_win = -1;      // window the lists on the device describe (-1: none)
    int n_kf_lmk = 0;
};

// The diagnostic switches of DESIGN.md 4 (environment), read ONCE when the handle is created: none is needed in production, and none is
// looked up again on a per-key-frame path (round 4 called getenv 39 times across set_windows / marginalize / solve).
struct EnvCfg {
    int debug = 0;
    int lm = -1, pf_wg = -1;            // -1: not set
    int tile_rounds = 0, lm_subs = 0, band_c = 0;   // 0: not set
    int cov_batch_lds = 1, cov_batch_scratch_mb = 1024;   // sadvio_ba_covariance_batch: the in-LDS inverse (0: every item down the dense route, A/B) | scratch budget of one group
    int cov_band = -1;   // covariance, the band route (cov_band_kernels.h): -1 not set: only where the call was refused before (N_p >= 2047) | 1: every bandable window | 0: never
    int cov_sqrt = -1;   // covariance, the square-root assembly (cov_kernels.h): -1 not set: only after the pivot tests refused the plain form | 1: from the start | 0: never
    int cov_border = -1; // covariance, the border route (cov_border_kernels.h): -1 not set: only where the call was refused before (N_p >= 2047) | 1: every borderable window that is not plainly bandable | 0: never
    int cov_border_hb = 0;   // ... its hb_lim (cov_border_plan.h), tests: a value in [1, the band kernels' limit) lowers it; 0: not set
    int cov_cross_stage = -1;   // covariance_cross: doubles of a block row k_cov_cross stages in LDS (tests: both sides of the limit); -1 not set: COVX_STAGE_MAX
    int long_min_env = 0;   // SADVIO_LONG_MIN as read (0: not set or out of range): LongCfg::from_create applies it
    double jacobi_tol = 1e-14;
    bool marg_pivoted = false, marg_unpivoted = false, pchol_strict = false, no_lpt = false, no_pre = false, no_fork = false, no_bcr = false, imu_items = false, contig_tiles = false, c16_old_tail = false, no_one_round = false;
    void read() {
        auto on = [](const char* k) { return getenv(k) != nullptr; };
        auto num = [](const char* k, int unset) { const char* e = getenv(k); return e ? atoi(e) : unset; };
        debug = num("SADVIO_DEBUG", 0); lm = num("SADVIO_LM", -1); pf_wg = num("SADVIO_PF_WG", -1);
        tile_rounds = num("SADVIO_TILE_ROUNDS", 0); lm_subs = num("SADVIO_LM_SUBS", 0); band_c = num("SADVIO_BAND_C", 0);
        cov_batch_lds = num("SADVIO_COV_BATCH_LDS", 1); cov_batch_scratch_mb = num("SADVIO_COV_BATCH_SCRATCH_MB", 1024);
        cov_band = num("SADVIO_COV_BAND", -1); cov_sqrt = num("SADVIO_COV_SQRT", -1);
        cov_cross_stage = num("SADVIO_COV_CROSS_STAGE", -1);
        cov_border = num("SADVIO_COV_BORDER", -1); cov_border_hb = std::max(num("SADVIO_COV_BORDER_HB", 0), 0);
        long_min_env = num("SADVIO_LONG_MIN", 0);
        if (long_min_env < 2 || long_min_env > MAX_LMK_OBS + 1) long_min_env = 0;
        if (const char* e = getenv("SADVIO_JACOBI_TOL")) jacobi_tol = atof(e);
        marg_pivoted = on("SADVIO_MARG_PIVOTED"); marg_unpivoted = on("SADVIO_MARG_UNPIVOTED"); pchol_strict = on("SADVIO_PCHOL_STRICT");
        no_lpt = on("SADVIO_NO_LPT"); no_pre = on("SADVIO_NO_PRE"); no_fork = on("SADVIO_NO_FORK");
        no_bcr = on("SADVIO_NO_BCR");
        { const char* e = getenv("SADVIO_NO_ONE_ROUND"); no_one_round = e && atoi(e) != 0; }   // A/B: single-round tiles on the kernels that loop over landmark rounds
        contig_tiles = on("SADVIO_CONTIG_TILES");   // A/B: single-round tiles as runs of consecutive landmarks (no packing, tile_pack.h)
        c16_old_tail = on("SADVIO_C16_OLD_TAIL");   // A/B: k_solve's in-LDS solve with both barriers of its last block column (chol16.h)
        imu_items = on("SADVIO_IMU_ITEMS");   // A/B: the IMU pairs' entries through k_solve's item loop (the pre-0.5 path) on one device too
    }
};

// What sadvio_ba_create's long-track flags (sadvio_ba_config::reserved) ask of the handle.
struct LongCfg {
    int min = 0;   // 0: created without SADVIO_CFG_LONG_TRACKS (no long path: a 65th observation is refused as it always was); else 65, or SADVIO_LONG_MIN in
                   // [2, 65] (tests, A/B timing): a landmark with at least this many observations takes the long path (long_kernels.h)
    bool priors = false;   // SADVIO_CFG_LONG_TRACK_PRIORS: marginalize, sparsify and the prior setters serve long tracks
    bool cov = false;      // SADVIO_CFG_LONG_TRACK_COVARIANCE: covariance and covariance_cross serve a window with long tracks (independent of `priors`)
    bool batch = false;    // SADVIO_CFG_LONG_TRACK_BATCH: marginalize_relative(_batch) serve a window with long tracks, and with `cov` covariance_batch
    // Fills the struct; false with the refusal in `err`: a flag that needs SADVIO_CFG_LONG_TRACKS and came without it
    bool from_create(unsigned reserved, int long_min_env, std::string& err) {
        static const struct { unsigned flag; const char* name; const char* reason; } needs[] = {
            {SADVIO_CFG_LONG_TRACK_PRIORS, "SADVIO_CFG_LONG_TRACK_PRIORS", "to carry a prior on"},
            {SADVIO_CFG_LONG_TRACK_COVARIANCE, "SADVIO_CFG_LONG_TRACK_COVARIANCE", "to form a covariance of"},
            {SADVIO_CFG_LONG_TRACK_BATCH, "SADVIO_CFG_LONG_TRACK_BATCH", "for a batch call to serve"}};
        for (const auto& n : needs)
            if ((reserved & n.flag) && !(reserved & SADVIO_CFG_LONG_TRACKS)) {
                err = std::string("create: ") + n.name + " needs SADVIO_CFG_LONG_TRACKS (a handle without the long path has no long track " + n.reason + ")";
                return false;
            }
        min = (reserved & SADVIO_CFG_LONG_TRACKS) ? (long_min_env ? long_min_env : MAX_LMK_OBS + 1) : 0;
        priors = (reserved & SADVIO_CFG_LONG_TRACK_PRIORS) != 0; cov = (reserved & SADVIO_CFG_LONG_TRACK_COVARIANCE) != 0;
        batch = (reserved & SADVIO_CFG_LONG_TRACK_BATCH) != 0;
        return true;
    }
};

struct sadvio_ba_handle {
    EnvCfg env;
    LongCfg lt;
    sadvio_ba_config cfg{};
    LayoutPlan plan;   // the current layout as host tables (layout_plan.h); layout_driver.h puts it on the device
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // host mirrors
    std::vector<PriorDev> priors;
    std::vector<std::vector<PriorDev>> priors_per_win;
    std::vector<std::vector<ImuDev>> imus_per_win;
    std::vector<ImuDev> imus;
    DevBuf<int> d_big_info;
    DevBuf<double> d_big_M;     // inverse diagonal blocks of the wide-panel dense solver, 96 x 96 per 96 columns (+ the factors' tiles)
    DevBuf<double> d_big_Lx;    // its out-of-place panels
    DevBuf<double> d_big_linv;  // inverse pivot blocks of the banded solver, N * NB doubles per out-of-LDS window
    DevBuf<double> d_coll_band; // band-packed copy of the reduced system for the sharded all-reduce
    DevBuf<double> d_bcr;       // block-cyclic-reduction workspace of the long banded systems
    DevBuf<double> d_big_mid;   // the two Schur complements on the middle block of the twisted banded factorisation
    bool uploaded = false, solved = false;
    bool defer = false, pending = false;   // begin_update .. commit_update: set_* calls only record, ONE layout build + staged upload at commit
    UploadBatch up;   // pending host -> device uploads of the current layout build
    // window sharded over several GPUs: collective hook (user callback or the built-in RCCL one)
    int world = 1, rank = 0;
    sadvio_allreduce_fn coll_fn = nullptr;
    void* coll_ctx = nullptr;
    RcclLib rccl;
    DevBuf<double> d_rank_b, d_rank_s;
    // dense marginalisation priors (host copies, one per window) and the layout they induce
    std::vector<DensePriorHost> dprior_per_win;
    PriorState prior;   // the handle's own prior (sadvio_ba_marginalize leaves it here)
    MargScratch mg;
    CovScratch cv;
    CovBatchScratch cvb;
    CovCrossScratch cx;
    RelScratch rel;
    double cov_huber_a = 0.0;   // huber_a of the last solve: sadvio_ba_covariance corrects the visual factors as that solve did
    bool cov_use_lm = false;    // ... and whether the throughput kernels ran it (covariance is then refused)
    std::vector<SrcWin> src;                       // caller windows (deep copies)
    std::vector<std::vector<sadvio_sparse_prior>> sparse_per_win;
    std::vector<LineSetHost> lines_per_win;        // linexd landmarks
    DevBuf<LineDev> d_lines;
    DevBuf<LineObsDev> d_lobs;
    DevBuf<double> d_xline, d_line_scratch;
    int n_line_tot = 0, n_lobs_tot = 0;
    DevBuf<SparseDev> d_sparse;
    DevBuf<int> d_sp_list;
    int n_sp_list = 0;   // sparse prior factors evaluated by sparse_factor_eval (all windows)
    size_t n_sparse_tot = 0;
    DevBuf<double> d_sp_scratch;
    DevBuf<int> d_lmk_red, d_kept_obs, d_dp_ints;
    DevBuf<double> d_dp_data;
    int last_slots = 0;
    bool last_one_round = false;   // the last solve's SolvePlan::one_round (sadvio_ba_one_round)
    // device buffers
    DevBuf<WinDev> d_win;
    DevBuf<Tile> d_tiles;
    DevBuf<double> d_kf_T0, d_xp, d_xv, d_xba, d_xbg, d_kf_vel, d_kf_ba, d_kf_bg;
    DevBuf<int> d_kf_fidx;
    DevBuf<double> d_cam_K, d_cam_T, d_cam_isig;
    DevBuf<double> d_lmk_p, d_xl, d_s_lmk;
    DevBuf<unsigned char> d_lmk_const;
    DevBuf<int> d_lmk_ob, d_lmk_oe, d_obs_kf, d_obs_cam, d_tile_kf, d_tile_row, d_tile_lmk;
    DevBuf<int> d_long_rec, d_long_kf, d_long_slot;   // tables of the long tracks (long_kernels.h, LayoutPlan::long_rec)
    DevBuf<int> d_pre_lane, d_pre_kf;     // first-round packets of the latency kernels (step_args.h: DevPtrs::pre_lane), few-tile submissions only
    bool pre_dirty = false;
    DevBuf<int> d_rank_col; DevBuf<double> d_rank_x;       // refine_rank_by_eigenvalue (guarded calls only): pivot column per step, the solved vectors
    DevBuf<unsigned char> d_obs_slot, d_obs_lslot;
    DevBuf<int> d_chunk_ob, d_chunk_lm, d_tile_perm;   // chunk tables of the throughput kernels (lm_kernels.h)
    DevBuf<int> d_jac_ints;               // pivoting / rank of the Cholesky-preconditioned Jacobi
    DevBuf<double> d_jac_dbl;             // its remaining diagonal + threshold
    DevBuf<double> d_lm_hg, d_lm_dt, d_lm_sacc;   // throughput path: per-landmark H_ll | g_l, per-tile key-frame sums and cost sums (each per delta buffer)
    DevBuf<int> d_lm_sub;                 // work list of k_lm_pass (tile, sub-block), see DevPtrs
    int hidden_eig_count = 0;             // sparsify: priors of full rank by their pivots whose inverse showed an eigenvalue that may lie below the cut (SADVIO_DEBUG prints it)
    int marg_stats[4] = {0, 0, 0, 0};     // Cholesky-form marginalisations: calls | took the unpivoted route | tried it and fell back | calls whose rank the eigenvalue refinement lowered
    DevBuf<double> d_ptab;
    DevBuf<double> d_obs_meas;
    DevBuf<PriorDev> d_priors;
    DevBuf<double> d_prior_lin;   // [2][n_prior][PRIOR_LIN], see DevPtrs::prior_lin
    DevBuf<ImuDev> d_imus;
    DevBuf<double> d_imu_scratch;
    DevBuf<double> d_S, d_gred, d_gfull, d_hdiag, d_delta, d_s_pose;
    DevBuf<LmState> d_states;
    DevBuf<double> d_trace;
    DevBuf<long long> d_tstart;
    DevBuf<IterAcc> d_acc;
    DevBuf<FinalRec> d_final;
    FinalRec* h_final = nullptr;  // pinned
    double* h_deltas = nullptr; size_t h_deltas_cap = 0; bool deltas_cached = false;   // pinned copy of BOTH delta buffers, fetched by the first get_deltas after a solve
    size_t h_final_n = 0;
    std::vector<FinalRec> fin;    // last solve's records
    DevBuf<TileAcc> d_tacc;
    DevBuf<long long> d_dbg;
    // hipGraph of one complete solve (all slots), re-captured whenever the launch parameters change
    hipGraphExec_t graph_exec = nullptr;
    std::vector<unsigned char> graph_key;
    DevBuf<double> d_probe;
    // profiling
    std::vector<KernelClass> kclasses;
    hipStream_t side = nullptr;            // IMU factor evaluation runs here, concurrently with k_build / k_backsub
    hipEvent_t ev_fork = nullptr, ev_lin = nullptr, ev_solved = nullptr, ev_cost = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<std::pair<int, int>> ev_used;  // (class, pool index)
    size_t ev_next = 0;
};

namespace {

int kclass_id(sadvio_ba_handle* h, const char* name) {
    for (size_t i = 0; i < h->kclasses.size(); i++)
        if (!strcmp(h->kclasses[i].name, name)) return (int)i;
    KernelClass k; k.name = name;
    h->kclasses.push_back(k);
    return (int)h->kclasses.size() - 1;
}

// The state an entry point needs of its handle, checked in this order; `what` opens the refusal's text
enum { NEED_UPLOADED = 1, NOT_DEFERRED = 2, NEED_SOLVED = 4 };
int entry_state(sadvio_ba_handle* h, const char* what, int need) {
    if ((need & NEED_UPLOADED) && !h->uploaded) { h->err = std::string(what) + " before set_windows"; return SADVIO_E_STATE; }
    if ((need & NOT_DEFERRED) && h->defer) { h->err = std::string(what) + " between begin_update and commit_update"; return SADVIO_E_STATE; }
    if ((need & NEED_SOLVED) && !h->solved) { h->err = std::string(what) + " before solve"; return SADVIO_E_STATE; }
    return SADVIO_OK;
}

// Long tracks (long_kernels.h) are served by the window solve and the per-landmark probes; the entry points that walk a landmark's
// observations in lane groups of their own refuse a window that has one (DESIGN.md "Long tracks": follow-ups).
bool window_has_long(const sadvio_ba_handle* h, int w) {
    return w >= 0 && w < (int)h->plan.wins.size() && h->plan.wins[w].long_end > h->plan.wins[w].long_begin;
}
int refuse_long(sadvio_ba_handle* h, int w, const char* what) {
    if (!h->uploaded || h->defer || !window_has_long(h, w)) return SADVIO_OK;
    h->err = std::string(what) + ": the window has long tracks (landmarks with more than 64 observations), which this call does not serve";
    return SADVIO_E_INVALID_ARG;
}
// landmark l of window w as the NEXT layout will see it (the caller's copy: valid between begin_update and commit_update too)
bool lmk_is_long(const sadvio_ba_handle* h, int w, int l) {
    return w >= 0 && w < (int)h->src.size() && src_lmk_is_long(h->src[w], l, h->lt.min, h->world, h->coll_fn != nullptr);
}
// ... and is it one that this handle's back-end calls (marginalize, sparsify, the prior setters) refuse: every long track, unless the
// handle was created with SADVIO_CFG_LONG_TRACK_PRIORS
bool lmk_is_refused_long(const sadvio_ba_handle* h, int w, int l) { return !h->lt.priors && lmk_is_long(h, w, l); }

struct ScopedTimer {
    sadvio_ba_handle* h;
    int pool = -1;
    ScopedTimer(sadvio_ba_handle* h_, const char* name) : h(h_) {
        if (!h->cfg.profile_kernels || !name) return;   // (a null name: no timer)
        if (h->ev_next == h->ev_pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            h->ev_pool.push_back({a, b});
        }
        pool = (int)h->ev_next++;
        h->ev_used.push_back({kclass_id(h, name), pool});
        (void)hipEventRecord(h->ev_pool[pool].first, h->stream);
    }
    ~ScopedTimer() {
        if (pool >= 0) (void)hipEventRecord(h->ev_pool[pool].second, h->stream);
    }
};

void collect_timers(sadvio_ba_handle* h) {
    for (auto& u : h->ev_used) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->ev_pool[u.second].first, h->ev_pool[u.second].second) == hipSuccess) {
            h->kclasses[u.first].total_ms += ms;
            h->kclasses[u.first].launches += 1;
        }
    }
    h->ev_used.clear();
    h->ev_next = 0;
}

}  // namespace

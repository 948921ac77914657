// layout_plan.h — the device layout of a batch of windows as a function from the caller's windows and factor lists to host tables
// (host only: integer arithmetic and copied doubles; nothing here touches the device — layout_driver.h allocates and uploads what this
// plans). Every kernel trusts these tables without bounds checks; tests/cpp/test_layout_plan.cpp holds them to hand-derived values.
//
// Steps of a full build, in order (layout_plan): layout_views (camera de-duplication, pseudo-observations of eliminable
// pose-to-landmark factors), layout_windows (window records and bases), layout_long (which landmarks are long tracks: more
// observations than a lane group holds; they stay out of the tiles), then per window layout_concat, layout_sort (per-landmark
// key-frame order, obs_perm), layout_long_lists (key-frame lists of the long tracks) and layout_tiles (contiguous or packed cut), then layout_chunks (chunk tables and work lists of the
// throughput kernels) and layout_reduced_plan (reduced systems: Np, ld, S_off, kept landmarks, dense-prior column maps, lines).
// A change of the factor lists that leaves the tiles alone re-runs layout_reduced_plan only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sadvio_ba.h"
#include "ba_types.h"
#include "tile_pack.h"

namespace sadvio {

// Deep copy of a caller's window (set_windows) + the observation arrays actually tiled: pose-to-landmark NFR factors
// whose landmark can be eliminated are appended to the landmark's observation list as two pseudo-observations
// (rows 0-1 and row 2 of the 3-row factor), so that they ride the ordinary Schur elimination.
struct SrcWin {
    sadvio_flat_window v{};   // view into the vectors below
    std::vector<int64_t> kf_id, lmk_id;
    std::vector<double> kf_T, kf_vel, kf_ba, kf_bg, cam_K, cam_T, cam_sigma, lmk_p, obs_meas;
    std::vector<uint8_t> kf_const, lmk_const;
    std::vector<int32_t> lmk_obs_ptr, obs_kf, obs_cam;
    // augmented observation list (what layout_tiles cuts) and its map to the caller's observation index (-1 = pseudo): layout_views
    std::vector<int32_t> a_ptr, a_kf, a_cam, a_src;
    std::vector<double> a_meas;
    // cameras with identical (K, T_s_f, sigma) are stored once: SaDVIO has one ImageSensor object per (frame, camera),
    // i.e. 2 x N_kf table entries that are all copies of the rig's two cameras
    std::vector<double> u_cam_K, u_cam_T, u_cam_sigma;
    std::vector<int32_t> u_obs_cam;
    std::vector<int> cam_map;   // caller's camera index -> stored camera index
};

struct HostWin {
    WinDev d;
    std::vector<int64_t> kf_id, lmk_id;
    int hb_lmk = 0;  // max distance (in free key-frame index) between two key-frames observing one landmark
    int long_begin = 0, long_end = 0;   // the window's slice of the long list (LayoutPlan::long_rec)
};

struct DensePriorHost {
    int n_full = 0, n = 0, kf_keep = -1, kf_col = 0;
    bool resident = false;      // J, r0 = the handle's prior (PriorState), copied device to device
    unsigned long long serial = 0;   // ... as it was when set_dense_prior named it
    std::vector<double> J, r0;
    std::vector<int> lmk_index, lmk_col;
};

struct LineSetHost {   // deep copy of a sadvio_line_set
    std::vector<int64_t> id;
    std::vector<double> T, model, meas;
    std::vector<unsigned char> is_const;
    std::vector<int> ptr, obs_kf, obs_cam;
    int n() const { return (int)id.size(); }
};

// Work arrays of the steps, kept between calls like the plan's own vectors: a sliding-window back end calls set_windows once per
// key-frame, and ~2 MB of fresh std::vectors per call are ~500 page faults (more than the layout arithmetic itself).
struct LayoutScratch {
    std::vector<int> pack_order, pack_cut, pkf, run_max, mark, add, kfs, slot_of;
    std::vector<int> rem, rem_ptr, rem_kf, rem_run;   // a window with long tracks: the landmarks left to the tiles and their compact CSR (tile_pack)
    std::vector<long long> long_key;
    std::vector<char> held;
};

// What the plan depends on, and nothing else.
struct LayoutIn {
    std::vector<SrcWin>* src = nullptr;   // the caller's windows; layout_views fills their a_*, u_* and cam_map
    const std::vector<std::vector<sadvio_sparse_prior>>* sparse_per_win = nullptr;
    const std::vector<DensePriorHost>* dprior_per_win = nullptr;
    const std::vector<LineSetHost>* lines_per_win = nullptr;
    // the handle's resident prior, as a window that attached it must still find it
    bool prior_valid = false;
    unsigned long long prior_serial = 0;
    int prior_n_full = 0, prior_n = 0;
    int world = 1;
    bool has_coll = false;   // a collective hook is set (a sharded window keeps the contiguous cut)
    int tile_rounds = 0, lm = -1, lm_subs = 0;   // SADVIO_TILE_ROUNDS, SADVIO_LM, SADVIO_LM_SUBS (0 / -1: not set)
    bool contig_tiles = false, no_lpt = false, no_pre = false;   // no_pre decides pre_ok only
    int long_min = 0;   // 0: no long path (a landmark with more than 64 observations is refused); else a landmark with at least this many observations
                        // is a long track (SADVIO_CFG_LONG_TRACKS: 65, or SADVIO_LONG_MIN)
    bool long_priors = false;   // SADVIO_CFG_LONG_TRACK_PRIORS: a prior may keep a long track in the reduced system (false: such a prior is refused)
};

struct DensePrep { long long off; int nf, n, w; };   // a window's dense prior in dp_data: offset, rows, columns, window

// Everything the planning produces. Kept in the handle: the vectors keep their capacity between calls.
struct LayoutPlan {
    // layout_views
    std::vector<sadvio_flat_window> views;         // the windows as tiled: stored cameras, augmented observation lists
    std::vector<std::vector<char>> sp_elim;        // per window, per sparse factor: handled as pseudo-observations
    std::vector<int> n_obs_user;                   // caller's observation count per window
    // layout_windows
    std::vector<HostWin> wins;
    int factor_type = 0;
    int n_kf_tot = 0, n_cam_tot = 0, n_lmk_tot = 0, n_obs_tot = 0;
    int max_n_kf = 0, max_npose = 0;
    bool user_lmk_const = false;                   // a window came with lmk_const
    // layout_long, layout_long_lists: the long tracks (long_kernels.h), windows in order. long_rec: per track | global landmark |
    // window | first entry of long_kf | distinct observing key-frames | first entry of long_slot | observations |; long_kf: those
    // key-frames (global, ascending); long_slot: per observation of the track, in device order, its index into that list
    std::vector<int> long_rec, long_kf, long_slot;
    std::vector<char> is_long;                     // [n_lmk_tot]
    int n_long = 0, long_max_kf = 0;
    // layout_concat, layout_sort: the concatenated arrays
    std::vector<double> kf_T0, kf_vel, kf_ba, kf_bg, cam_K, cam_T, cam_isig, lmk_p, obs_meas;
    std::vector<int> kf_fidx, lmk_ob, lmk_oe, obs_kf, obs_cam;
    std::vector<unsigned char> lmk_const;          // as given by the caller
    std::vector<int> obs_perm;                     // device observation position -> caller's observation index (within window), -1 = pseudo
    // layout_tiles
    std::vector<Tile> tiles;
    std::vector<int> tile_kf, tile_row, tile_lmk;
    std::vector<unsigned char> obs_slot;
    int max_tile_kf = 1, max_tile_free = 0, max_gemm_free = 0;
    bool gemm_run4 = false;               // a tile on the MFMA path holds runs of 3 - 4 observations on one key-frame (k_build<.., RARE = true> only)
    // layout_chunks
    std::vector<int> chunk_ob, chunk_lm, perm, sub;   // chunk starts + one sentinel | launch order of the tiles | work list of k_lm_pass (tile, sub-block)
    std::vector<unsigned char> obs_lslot;
    bool want_lm = false;                 // the throughput path's tables are built
    bool lm_ok = false;                   // every tile is on the MFMA path and chunked: k_build_obs / k_lm_pass may run
    long long lm_landmarks = 0;
    int lm_sub_obs = 0;                   // most observations of LM_PASS_THREADS consecutive landmarks of a tile (LDS staging of k_lm_pass)
    int lm_ksub = 1, lm_max_cam = 1, lm_n_sub = 0;
    int lm_sub_per_item = 8;              // sub-blocks per work item of k_lm_pass (8 = the whole tile: MAX tile = 512 landmarks)
    bool pre_ok = false;                  // few enough tiles for the first-round packets
    bool single_round = false;            // every tile holds at most BUILD_WAVES * (64 / G) landmarks: each wave of k_build / k_backsub runs one landmark round
    // layout_reduced_plan
    std::vector<int> lmk_red, kept, dp_ints, sp_list;
    std::vector<unsigned char> lmk_const_red;      // lmk_const with 2 = kept in the reduced system
    std::vector<SparseDev> sparse;
    std::vector<LineDev> lines;
    std::vector<LineObsDev> lobs;
    std::vector<DensePrep> preps;
    long long dp_total = 0;               // doubles of dp_data: per window [J | J^T | J^T J | r0 | dx | r | cost slot]
    long long s_tot = 0, red_total = 0, n_rank_b = 0;   // red_total: doubles in [S | gred | gfull | hdiag | rank_b], the buffer of the per-step all-reduce
    int np_tot = 0, n_kept = 0, max_np = 0, n_big = 0;
    bool has_lmk_const = false;
    LayoutScratch ls;
};

// One caller's window, before it is copied: everything later steps index with is present and in range.
inline int check_flat_window(const sadvio_flat_window& F, int w, std::string& err) {
    // a pose-graph window (relative-pose factors only) has no cameras, landmarks or observations
    if (F.n_kf <= 0 || F.n_cam < 0 || F.n_lmk < 0 || F.n_obs < 0 || !F.kf_T_f_w || (F.n_cam > 0 && (!F.cam_K || !F.cam_T_s_f)) ||
        (F.n_obs > 0 && F.n_cam == 0) ||
        (F.n_lmk > 0 && (!F.lmk_p || !F.lmk_obs_ptr)) || (F.n_obs > 0 && (!F.obs_kf || !F.obs_cam || !F.obs_meas))) {
        err = "set_windows: missing array in window " + std::to_string(w);
        return SADVIO_E_INVALID_ARG;
    }
    if (F.n_lmk > 0 && (F.lmk_obs_ptr[0] != 0 || F.lmk_obs_ptr[F.n_lmk] != F.n_obs)) {
        err = "set_windows: lmk_obs_ptr is not a CSR over n_obs";
        return SADVIO_E_INVALID_ARG;
    }
    for (int l = 0; l < F.n_lmk; l++)
        if (F.lmk_obs_ptr[l + 1] < F.lmk_obs_ptr[l]) { err = "set_windows: CSR not monotone"; return SADVIO_E_INVALID_ARG; }
    for (int o = 0; o < F.n_obs; o++)
        if (F.obs_kf[o] < 0 || F.obs_kf[o] >= F.n_kf || F.obs_cam[o] < 0 || F.obs_cam[o] >= F.n_cam) {
            err = "set_windows: observation index out of range";
            return SADVIO_E_INVALID_ARG;
        }
    return SADVIO_OK;
}

inline bool src_lmk_is_long(const SrcWin& S, int l, int long_min, int world, bool has_coll);   // below, with layout_long

// Views of the windows as they are tiled. Cameras with equal (K, T, sigma) are stored once. Which sparse factors ride the Schur
// elimination as pseudo-observations: PoseToLandmark factors whose landmark is free and not held in the reduced system for another
// reason (dense prior, landmark prior / landmark chain factor).
inline void layout_views(const LayoutIn& in, LayoutPlan& P) {
    const int n_windows = (int)in.src->size();
    P.views.resize(n_windows);
    P.sp_elim.assign(n_windows, {});
    P.n_obs_user.assign(n_windows, 0);
    int sp_global = 0;
    for (int w = 0; w < n_windows; w++) {
        SrcWin& S = (*in.src)[w];
        const auto& sp = (*in.sparse_per_win)[w];
        sadvio_flat_window& V = P.views[w];
        P.sp_elim[w].assign(sp.size(), 0);
        P.n_obs_user[w] = S.v.n_obs;
        V = S.v;
        std::vector<int>& cmap = S.cam_map;
        cmap.assign(S.v.n_cam, -1);
        S.u_cam_K.clear(); S.u_cam_T.clear(); S.u_cam_sigma.clear();
        for (int c = 0; c < S.v.n_cam; c++) {
            const double sg = S.cam_sigma.empty() ? 1.0 : S.cam_sigma[c];
            const int nu = (int)S.u_cam_sigma.size();
            for (int u = 0; u < nu && cmap[c] < 0; u++)
                if (!memcmp(&S.u_cam_K[4 * u], &S.cam_K[4 * c], 32) && !memcmp(&S.u_cam_T[12 * u], &S.cam_T[12 * c], 96) && S.u_cam_sigma[u] == sg) cmap[c] = u;
            if (cmap[c] < 0) {
                cmap[c] = nu;
                S.u_cam_K.insert(S.u_cam_K.end(), &S.cam_K[4 * c], &S.cam_K[4 * c] + 4);
                S.u_cam_T.insert(S.u_cam_T.end(), &S.cam_T[12 * c], &S.cam_T[12 * c] + 12);
                S.u_cam_sigma.push_back(sg);
            }
        }
        S.u_obs_cam.resize(S.obs_cam.size());
        for (size_t o = 0; o < S.obs_cam.size(); o++) S.u_obs_cam[o] = cmap[S.obs_cam[o]];
        V.n_cam = (int32_t)S.u_cam_sigma.size();
        V.cam_K = S.u_cam_K.data(); V.cam_T_s_f = S.u_cam_T.data(); V.cam_sigma = S.u_cam_sigma.data();
        V.obs_cam = S.u_obs_cam.data();
        S.a_src.clear();
        if (sp.empty()) continue;   // no sparse factors: nothing rides the elimination as a pseudo-observation
        auto& held = P.ls.held;
        held.assign(std::max(S.v.n_lmk, 1), 0);
        const DensePriorHost& D = (*in.dprior_per_win)[w];
        for (size_t i = 0; i < D.lmk_index.size(); i++) if (D.n_full > 0 && D.lmk_col[i] >= 0) held[D.lmk_index[i]] = 1;
        for (const auto& s : sp) {
            if (s.type == SADVIO_SPARSE_LMK_PRIOR) held[s.lmk0] = 1;
            if (s.type == SADVIO_SPARSE_LMK_TO_LMK) { held[s.lmk0] = 1; held[s.lmk1] = 1; }
            // a long track carries real observations only: a pose-to-landmark factor on one holds it in the reduced system and becomes
            // a listed factor whose second block is a reduced column (without long_priors layout_long refuses the factor, as it did)
            if (s.type == SADVIO_SPARSE_POSE_TO_LMK && in.long_priors && src_lmk_is_long(S, s.lmk0, in.long_min, in.world, in.has_coll)) held[s.lmk0] = 1;
        }
        std::vector<std::vector<int>> extra(S.v.n_lmk);  // per landmark: the window's sparse factors to append
        bool any = false;
        for (size_t k = 0; k < sp.size(); k++) {
            const auto& s = sp[k];
            if (s.type != SADVIO_SPARSE_POSE_TO_LMK || held[s.lmk0]) continue;
            if (!S.lmk_const.empty() && S.lmk_const[s.lmk0]) continue;
            P.sp_elim[w][k] = 1;
            extra[s.lmk0].push_back((int)k);
            any = true;
        }
        if (any) {
            const int ms = S.v.factor_type == SADVIO_FACTOR_PIXEL ? 2 : 3;
            S.a_ptr.assign(1, 0); S.a_kf.clear(); S.a_cam.clear(); S.a_meas.clear();
            for (int l = 0; l < S.v.n_lmk; l++) {
                for (int o = S.lmk_obs_ptr[l]; o < S.lmk_obs_ptr[l + 1]; o++) {
                    S.a_kf.push_back(S.obs_kf[o]); S.a_cam.push_back(S.u_obs_cam[o]); S.a_src.push_back(o);
                    for (int q = 0; q < ms; q++) S.a_meas.push_back(S.obs_meas[(size_t)ms * o + q]);
                }
                for (int k : extra[l])
                    for (int half = 0; half < 2; half++) {
                        S.a_kf.push_back(sp[k].kf); S.a_cam.push_back(-1 - (2 * (sp_global + k) + half)); S.a_src.push_back(-1);   // the factor's index in the batch
                        for (int q = 0; q < ms; q++) S.a_meas.push_back(0.0);
                    }
                S.a_ptr.push_back((int32_t)S.a_kf.size());
            }
            V.n_obs = (int32_t)S.a_kf.size();
            V.lmk_obs_ptr = S.a_ptr.data(); V.obs_kf = S.a_kf.data(); V.obs_cam = S.a_cam.data();
            V.obs_meas = S.a_meas.data();
        }
        sp_global += (int)sp.size();
    }
}

// Window records and their bases in the concatenated arrays. set_windows calls this inside begin_update .. commit_update as well:
// the factor setters that follow validate against the windows' sizes and convert indices with these offsets.
inline void layout_windows(int n_windows, const sadvio_flat_window* wins, LayoutPlan& P) {
    int kf_b = 0, cam_b = 0, lmk_b = 0, obs_b = 0;
    P.wins.resize(n_windows);
    P.factor_type = wins[0].factor_type;
    P.max_n_kf = P.max_npose = 0;
    P.user_lmk_const = false;
    for (int w = 0; w < n_windows; w++) {
        const sadvio_flat_window& F = wins[w];
        if (F.lmk_const) P.user_lmk_const = true;
        HostWin& H = P.wins[w];
        H.hb_lmk = 0;
        WinDev& d = H.d;
        memset(&d, 0, sizeof(d));
        d.n_kf = F.n_kf; d.n_cam = F.n_cam; d.n_lmk = F.n_lmk; d.n_obs = F.n_obs;
        d.kf_base = kf_b; d.cam_base = cam_b; d.lmk_base = lmk_b; d.obs_base = obs_b;
        d.factor_type = F.factor_type; d.has_imu = F.has_imu;
        d.dpf = F.has_imu ? 15 : 6;
        int nfree = 0;
        for (int k = 0; k < F.n_kf; k++)
            if (!(F.kf_const && F.kf_const[k])) nfree++;
        d.n_free_kf = nfree;
        d.Npose = nfree * 6;
        d.Np = nfree * d.dpf;
        H.kf_id.assign(F.n_kf, 0); H.lmk_id.assign(F.n_lmk, 0);
        for (int k = 0; k < F.n_kf; k++) H.kf_id[k] = F.kf_id ? F.kf_id[k] : k;
        for (int l = 0; l < F.n_lmk; l++) H.lmk_id[l] = F.lmk_id ? F.lmk_id[l] : l;
        kf_b += F.n_kf; cam_b += F.n_cam; lmk_b += F.n_lmk; obs_b += F.n_obs;
        P.max_n_kf = std::max(P.max_n_kf, F.n_kf);
        P.max_npose = std::max(P.max_npose, d.Npose);
    }
    P.n_kf_tot = kf_b; P.n_cam_tot = cam_b; P.n_lmk_tot = lmk_b; P.n_obs_tot = obs_b;
}

// Is landmark l of caller's window S a long track: by its REAL observations, so that a factor list never moves a landmark between
// the two paths. A window sharded over several GPUs has no long path.
inline bool src_lmk_is_long(const SrcWin& S, int l, int long_min, int world, bool has_coll) {
    if (long_min <= 0 || world > 1 || has_coll || l < 0 || l + 1 >= (int)S.lmk_obs_ptr.size()) return false;
    return S.lmk_obs_ptr[l + 1] - S.lmk_obs_ptr[l] >= long_min;
}

// The long list: landmarks with at least long_min observations are linearised, eliminated and back-substituted by kernels of their
// own (long_kernels.h), one workgroup each, and stay out of the tiles. Their index, their CSR entries and their place in every
// output array are untouched. Such a landmark carries real observations only; a landmark that passes MAX_LMK_OBS through
// pseudo-observations alone fits neither path. Fills HostWin::long_begin / long_end, is_long and the first two fields of long_rec.
inline int layout_long(const LayoutIn& in, LayoutPlan& P, std::string& err) {
    const int n_windows = (int)P.wins.size();
    P.long_rec.clear(); P.long_kf.clear(); P.long_slot.clear();
    P.is_long.assign(std::max(P.n_lmk_tot, 1), 0);
    P.n_long = 0; P.long_max_kf = 0;
    for (int w = 0; w < n_windows; w++) {
        const sadvio_flat_window& F = P.views[w];
        const SrcWin& S = (*in.src)[w];
        HostWin& H = P.wins[w];
        H.long_begin = P.n_long;
        for (int l = 0; l < F.n_lmk; l++) {
            const int n_aug = F.lmk_obs_ptr[l + 1] - F.lmk_obs_ptr[l];
            if (!src_lmk_is_long(S, l, in.long_min, in.world, in.has_coll)) {
                if (n_aug <= MAX_LMK_OBS) continue;
                if (in.long_min <= 0 || in.world > 1 || in.has_coll || n_aug == S.lmk_obs_ptr[l + 1] - S.lmk_obs_ptr[l]) err = "set_windows: a landmark has more than 64 observations";
                else err = "long tracks: the pseudo-observations of pose-to-landmark factors take a landmark past 64 observations";
                return SADVIO_E_INVALID_ARG;
            }
            if (n_aug != S.lmk_obs_ptr[l + 1] - S.lmk_obs_ptr[l]) { err = "long tracks: a pose-to-landmark factor of the sparse prior touches a landmark on the long path"; return SADVIO_E_INVALID_ARG; }
            if (n_aug > MAX_LONG_OBS) { err = "set_windows: a long track has more than " + std::to_string(MAX_LONG_OBS) + " observations"; return SADVIO_E_INVALID_ARG; }
            P.is_long[H.d.lmk_base + l] = 1;
            const int rec[LONG_REC] = {H.d.lmk_base + l, w, 0, 0, 0, n_aug};
            P.long_rec.insert(P.long_rec.end(), rec, rec + LONG_REC);
            P.n_long++;
        }
        H.long_end = P.n_long;
    }
    return SADVIO_OK;
}

// Key-frame lists of window w's long tracks, from the sorted observations (layout_sort left the window-local key-frames in ls.pkf)
inline int layout_long_lists(LayoutPlan& P, int w, std::string& err) {
    const HostWin& H = P.wins[w];
    const WinDev& d = H.d;
    const auto& pkf = P.ls.pkf;
    for (int i = H.long_begin; i < H.long_end; i++) {
        int* rec = &P.long_rec[(size_t)LONG_REC * i];
        const int gl = rec[0], o0 = P.lmk_ob[gl] - d.obs_base, o1 = P.lmk_oe[gl] - d.obs_base;
        rec[2] = (int)P.long_kf.size(); rec[4] = (int)P.long_slot.size();
        int prev = -1, n = 0;
        for (int o = o0; o < o1; o++) {
            if (pkf[o] != prev) { P.long_kf.push_back(d.kf_base + pkf[o]); prev = pkf[o]; n++; }
            P.long_slot.push_back(n - 1);
        }
        rec[3] = n;
        if (n > MAX_LONG_KF) { err = "set_windows: a long track is observed from more than " + std::to_string(MAX_LONG_KF) + " key-frames"; return SADVIO_E_INVALID_ARG; }
        P.long_max_kf = std::max(P.long_max_kf, n);
    }
    return SADVIO_OK;
}

// Sizes of the concatenated arrays (once per build) ...
inline void layout_concat_begin(LayoutPlan& P) {
    const int kf_b = P.n_kf_tot, cam_b = P.n_cam_tot, lmk_b = P.n_lmk_tot, obs_b = P.n_obs_tot;
    P.kf_T0.resize(12 * (size_t)kf_b); P.kf_vel.assign(3 * (size_t)kf_b, 0.0); P.kf_ba.assign(3 * (size_t)kf_b, 0.0); P.kf_bg.assign(3 * (size_t)kf_b, 0.0);
    P.kf_fidx.resize(kf_b);
    P.cam_K.resize(4 * (size_t)cam_b); P.cam_T.resize(12 * (size_t)cam_b); P.cam_isig.resize(cam_b);
    P.lmk_p.resize(3 * (size_t)lmk_b);
    P.lmk_const.assign(std::max(lmk_b, 1), 0);
    P.lmk_ob.resize(std::max(lmk_b, 1)); P.lmk_oe.resize(std::max(lmk_b, 1)); P.obs_kf.resize(std::max(obs_b, 1)); P.obs_cam.resize(std::max(obs_b, 1));
    const int ms = P.factor_type == SADVIO_FACTOR_PIXEL ? 2 : 3;
    P.obs_meas.resize((size_t)ms * std::max(obs_b, 1));
    P.tile_kf.clear(); P.tile_row.clear(); P.tile_lmk.clear(); P.tiles.clear();
    P.obs_slot.assign(std::max(obs_b, 1), 0);
    P.obs_perm.assign(std::max(obs_b, 1), 0);
    P.max_tile_kf = 1; P.max_tile_free = 0; P.max_gemm_free = 0; P.gemm_run4 = false;
}

// ... and window w's key-frames, cameras and landmarks at its bases (its observations: layout_sort)
inline void layout_concat(LayoutPlan& P, int w) {
    const sadvio_flat_window& F = P.views[w];
    const WinDev& d = P.wins[w].d;
    memcpy(&P.kf_T0[12 * (size_t)d.kf_base], F.kf_T_f_w, sizeof(double) * 12 * F.n_kf);
    if (F.kf_vel) memcpy(&P.kf_vel[3 * (size_t)d.kf_base], F.kf_vel, sizeof(double) * 3 * F.n_kf);
    if (F.kf_ba) memcpy(&P.kf_ba[3 * (size_t)d.kf_base], F.kf_ba, sizeof(double) * 3 * F.n_kf);
    if (F.kf_bg) memcpy(&P.kf_bg[3 * (size_t)d.kf_base], F.kf_bg, sizeof(double) * 3 * F.n_kf);
    int fi = 0;
    for (int k = 0; k < F.n_kf; k++) P.kf_fidx[d.kf_base + k] = (F.kf_const && F.kf_const[k]) ? -1 : fi++;
    if (F.n_cam) {
        memcpy(&P.cam_K[4 * (size_t)d.cam_base], F.cam_K, sizeof(double) * 4 * F.n_cam);
        memcpy(&P.cam_T[12 * (size_t)d.cam_base], F.cam_T_s_f, sizeof(double) * 12 * F.n_cam);
    }
    for (int c = 0; c < F.n_cam; c++) P.cam_isig[d.cam_base + c] = 1.0 / (F.cam_sigma ? F.cam_sigma[c] : 1.0);
    if (F.n_lmk) memcpy(&P.lmk_p[3 * (size_t)d.lmk_base], F.lmk_p, sizeof(double) * 3 * F.n_lmk);
    for (int l = 0; l < F.n_lmk; l++) {
        P.lmk_const[d.lmk_base + l] = F.lmk_const ? F.lmk_const[l] : 0;
        P.lmk_ob[d.lmk_base + l] = d.obs_base + F.lmk_obs_ptr[l];
        P.lmk_oe[d.lmk_base + l] = d.obs_base + F.lmk_obs_ptr[l + 1];
    }
}

// Observations of a landmark are stored sorted by key-frame (stable), so that the (at most two) cameras of one key-frame sit in
// adjacent lanes; the landmark / key-frame order of the window is untouched and obs_perm maps device position -> caller position
// for the per-observation probe. Leaves the window's sorted key-frames in ls.pkf and every landmark's
// longest same-key-frame run in ls.run_max for layout_tiles.
inline int layout_sort(const LayoutIn& in, LayoutPlan& P, int w, std::string& err) {
    const sadvio_flat_window& F = P.views[w];
    const WinDev& d = P.wins[w].d;
    auto& pkf = P.ls.pkf; auto& run_max = P.ls.run_max;
    pkf.resize(std::max(F.n_obs, 1));
    run_max.assign(std::max(F.n_lmk, 1), 0);
    const std::vector<int32_t>& a_src = (*in.src)[w].a_src;
    const bool has_asrc = !a_src.empty();
    const int32_t* asrc = has_asrc ? a_src.data() : nullptr;
    const int ms = P.factor_type == SADVIO_FACTOR_PIXEL ? 2 : 3;
    // first pass (integers only): is every landmark's list already key-frame sorted (what a flattening in frame order
    // produces)? Its longest same-key-frame run either way.
    bool all_sorted = true;
    int hb_win = 0;   // largest spread of free key-frame indices one landmark couples (half bandwidth of the reduced system)
    const int* fidx_w = P.kf_fidx.data() + d.kf_base;
    for (int l = 0; l < F.n_lmk; l++) {
        const int o0 = F.lmk_obs_ptr[l], o1 = F.lmk_obs_ptr[l + 1];
        // (more than MAX_LMK_OBS observations: a long track, or refused by layout_long)
        int run = 0, rm = 0, prev = -1, lo = 1 << 30, hi = -1;
        for (int o = o0; o < o1; o++) {
            const int kf = F.obs_kf[o];
            if (kf < prev) { all_sorted = false; }
            run = (kf == prev) ? run + 1 : 1;
            rm = std::max(rm, run);
            prev = kf;
            const int fi = fidx_w[kf];
            if (fi >= 0) { lo = std::min(lo, fi); hi = std::max(hi, fi); }
        }
        run_max[l] = rm;
        if (hi >= 0) hb_win = std::max(hb_win, hi - lo);
    }
    P.wins[w].hb_lmk = hb_win;
    const int kb = d.kf_base, cb = d.cam_base, ob = d.obs_base;
    if (all_sorted) {
        // bulk path: the device order IS the caller's order — whole-array copies
        const int n = F.n_obs;
        for (int o = 0; o < n; o++) { pkf[o] = F.obs_kf[o]; P.obs_kf[ob + o] = kb + F.obs_kf[o]; }
        for (int o = 0; o < n; o++) { const int c = F.obs_cam[o]; P.obs_cam[ob + o] = c < 0 ? c : cb + c; }
        if (has_asrc) for (int o = 0; o < n; o++) P.obs_perm[ob + o] = asrc[o];
        else for (int o = 0; o < n; o++) P.obs_perm[ob + o] = o;
        if (n) memcpy(&P.obs_meas[(size_t)ms * ob], F.obs_meas, sizeof(double) * (size_t)ms * n);
        return SADVIO_OK;
    }
    static_assert(MAX_LMK_OBS <= 256, "the sort key carries a landmark's observation position in 8 bits");
    for (int l = 0; l < F.n_lmk; l++) {
        const int o0 = F.lmk_obs_ptr[l], o1 = F.lmk_obs_ptr[l + 1], k_n = o1 - o0;
        // tracks are short: insertion sort (stable) on packed keys (key-frame << 8 | position) held in a local array —
        // no indirection through the caller's arrays inside the sort
        long long key_short[MAX_LMK_OBS];
        long long* key = key_short;
        int shift = 8;
        const int32_t* okf = F.obs_kf + o0;
        if (k_n > MAX_LMK_OBS) {
            // a long track (at most MAX_LONG_OBS observations: layout_long): a 16-bit position field, and the keys, all distinct, through std::sort
            static_assert(MAX_LONG_OBS <= 65536, "the sort key of a long track carries the observation position in 16 bits");
            P.ls.long_key.resize(k_n);
            key = P.ls.long_key.data(); shift = 16;
            for (int k = 0; k < k_n; k++) key[k] = ((long long)okf[k] << 16) | k;
            std::sort(key, key + k_n);
        } else {
            for (int k = 0; k < k_n; k++) key[k] = ((long long)okf[k] << 8) | k;
            for (int a = 1; a < k_n; a++) {
                const long long v = key[a];
                int b = a - 1;
                while (b >= 0 && key[b] > v) { key[b + 1] = key[b]; b--; }
                key[b + 1] = v;
            }
        }
        int run = 0, rm = 0, prev = -1;
        for (int k = 0; k < k_n; k++) {
            const int rel = (int)(key[k] & ((1 << shift) - 1));
            const int src = o0 + rel, dst = o0 + k;
            const int kf = okf[rel], c = F.obs_cam[src];
            pkf[dst] = kf;
            P.obs_perm[ob + dst] = has_asrc ? asrc[src] : src;  // -1: pseudo-observation
            P.obs_kf[ob + dst] = kb + kf;
            P.obs_cam[ob + dst] = c < 0 ? c : cb + c;
            const double* m = F.obs_meas + (size_t)ms * src;
            double* md = &P.obs_meas[(size_t)ms * (ob + dst)];
            md[0] = m[0]; md[1] = m[1]; if (ms == 3) md[2] = m[2];
            run = (kf == prev) ? run + 1 : 1;
            rm = std::max(rm, run);
            prev = kf;
        }
        run_max[l] = rm;
    }
    return SADVIO_OK;
}

// Is the throughput path wanted: its chunk tables cost host time (a second, sorted copy of the observation constants), so they are
// only built where it can run; its tiles are runs of consecutive landmarks throughout
// (a batch with long tracks is solved by the latency kernels: the chunk tables hold at most 64 observations per landmark)
inline bool layout_want_lm(const LayoutIn& in, const LayoutPlan& P) { return P.n_long == 0 && (in.lm >= 0 ? in.lm != 0 : P.n_lmk_tot >= 65536); }

// Tiles of window w. Every landmark gets a group of G lanes (G = pow2 >= the tile's largest observation count); a workgroup of
// BUILD_WAVES waves holds BUILD_WAVES * 64 / G landmarks per round. Contiguous cut: runs of consecutive landmarks, a tile is cut
// when its key-frame list would exceed the LDS tile capacity. Single-round tiles of the latency kernels are packed instead
// (tile_pack.h): a tile lists its landmarks, so that a few outlier tracks do not cut the runs around them. Multi-round tiles,
// sharded ranks and layouts that build the throughput path's chunk tables keep the contiguous cut.
inline int layout_tiles(const LayoutIn& in, LayoutPlan& P, int w, std::string& err) {
    const int n_windows = (int)P.views.size();
    const sadvio_flat_window& F = P.views[w];
    WinDev& d = P.wins[w].d;
    LayoutScratch& ls = P.ls;
    const auto& pkf = ls.pkf; const auto& run_max = ls.run_max;
    const bool has_asrc = !(*in.src)[w].a_src.empty();
    if (F.n_cam > MAX_WIN_CAM) { err = "set_windows: more than 8 distinct cameras per window"; return SADVIO_E_INVALID_ARG; }
    // rounds per tile: one for a single window (most workgroups = lowest latency); a large batch gets fewer, larger tiles
    // (~2048 = 4 per resident workgroup slot) so that table staging, merge and flush are paid once per several rounds
    int tile_rounds = (int)std::min<long long>(16, std::max<long long>(1, (P.n_lmk_tot + 32LL * 2048 - 1) / (32LL * 2048)));
    if (in.tile_rounds > 0) tile_rounds = in.tile_rounds;
    d.tile_begin = (int)P.tiles.size();
    const bool packed = n_windows == 1 && tile_rounds == 1 && F.n_lmk > 0 && in.world == 1 && !in.has_coll && !layout_want_lm(in, P) && !in.contig_tiles;
    auto& order = ls.pack_order; auto& cut = ls.pack_cut;
    // Long tracks (layout_long) pass through the cut as landmarks without observations and are left out of the tiles' landmark lists:
    // the tiles are those of the same window with these landmarks emptied. Their tiles list their landmarks (lmk_off >= 0) either way.
    const bool has_long = P.wins[w].long_end > P.wins[w].long_begin;
    const char* is_long = P.is_long.data() + d.lmk_base;
    const bool listed = packed || has_long;
    if (packed && has_long) {
        auto& rp = ls.rem_ptr; auto& rk = ls.rem_kf; auto& rr = ls.rem_run;
        rp.assign(1, 0); rk.clear(); rr.assign(F.n_lmk, 0);
        for (int gl = 0; gl < F.n_lmk; gl++) {
            if (!is_long[gl]) { rk.insert(rk.end(), pkf.begin() + F.lmk_obs_ptr[gl], pkf.begin() + F.lmk_obs_ptr[gl + 1]); rr[gl] = run_max[gl]; }
            rp.push_back((int)rk.size());
        }
        if (rk.empty()) rk.push_back(0);
        const TilePackIn tp{F.n_lmk, F.n_kf, rp.data(), rk.data(), F.kf_const, rr.data(), BUILD_WAVES * 64, MAX_TILE_KF, MAX_TILE_FREE_KF, MAX_GEMM_FREE_KF};
        tile_pack(tp, order, cut);
    } else if (packed) {
        const TilePackIn tp{F.n_lmk, F.n_kf, F.lmk_obs_ptr, pkf.data(), F.kf_const, run_max.data(), BUILD_WAVES * 64, MAX_TILE_KF, MAX_TILE_FREE_KF, MAX_GEMM_FREE_KF};
        tile_pack(tp, order, cut);
    }
    int l = 0;   // position in the window's landmark sequence: the landmark itself, or its place in order (packed)
    size_t next_cut = 0;
    auto lm_at = [&](int i) { return packed ? order[i] : i; };
    auto& mark = ls.mark; auto& add = ls.add; auto& kfs = ls.kfs; auto& slot_of = ls.slot_of;
    mark.assign(F.n_kf, -1); slot_of.assign(F.n_kf, -1);
    while (l < F.n_lmk || (int)P.tiles.size() == d.tile_begin) {
        Tile t{};
        t.w = w; t.lmk0 = d.lmk_base + (l < F.n_lmk ? lm_at(l) : l); t.kmax = 1; t.G = 8;
        t.lmk_off = listed ? (int)P.tile_lmk.size() : -1;
        t.dpf = d.dpf;  // Np, red_off, S_off, ld: layout_reduced_plan
        t.cam_base = d.cam_base; t.n_cam = F.n_cam;
        t.first_of_window = ((int)P.tiles.size() == d.tile_begin) ? 1 : 0;
        kfs.clear();
        int nfree = 0, tile_run_max = 0, n_skipped = 0;
        const int l_begin = l;
        while (l < F.n_lmk) {
            const int gl = lm_at(l);
            if (packed && l == cut[next_cut]) break;
            const bool lg = has_long && is_long[gl];
            const int k = lg ? 0 : F.lmk_obs_ptr[gl + 1] - F.lmk_obs_ptr[gl];
            int G = t.G;
            while (G < k) G <<= 1;
            const int cap = tile_rounds * BUILD_WAVES * (64 / G);  // landmarks per tile (tile_rounds rounds per wave)
            if (!packed && l - l_begin + 1 > cap && l > l_begin) break;
            // key-frames this landmark would add
            add.clear();
            int add_free = 0;
            for (int o = F.lmk_obs_ptr[gl]; o < F.lmk_obs_ptr[gl] + k; o++) {
                const int kf = pkf[o];
                if (mark[kf] != (int)P.tiles.size()) {
                    mark[kf] = (int)P.tiles.size();
                    add.push_back(kf);
                    if (!(F.kf_const && F.kf_const[kf])) add_free++;
                }
            }
            const bool fits_hard = (int)(kfs.size() + add.size()) <= MAX_TILE_KF && nfree + add_free <= MAX_TILE_FREE_KF;
            // soft limit: keep tiles on the MFMA path (<= MAX_GEMM_FREE_KF free key-frames) whenever a cut achieves it
            const bool fits = fits_hard && (nfree + add_free <= MAX_GEMM_FREE_KF || l == l_begin);
            if (!packed && !fits && l > l_begin) {
                for (int kf : add) mark[kf] = -1;  // roll back
                break;
            }
            for (int kf : add) kfs.push_back(kf);
            nfree += add_free;
            t.G = G;
            t.kmax = std::max(t.kmax, k);
            if (lg) n_skipped++;
            else {
                tile_run_max = std::max(tile_run_max, run_max[gl]);
                if (listed) P.tile_lmk.push_back(d.lmk_base + gl);
            }
            l++;
            if (!packed && !fits_hard) break;  // a single landmark exceeding the capacity: global-atomics tile
        }
        if (packed) next_cut++;
        t.n_lmk = l - l_begin - n_skipped;
        t.lmk1 = t.lmk0 + t.n_lmk;   // (a tile that lists its landmarks: the count only; they are tile_lmk's)
        std::sort(kfs.begin(), kfs.end());
        t.lds_mode = ((int)kfs.size() <= MAX_TILE_KF && nfree <= MAX_TILE_FREE_KF) ? ((nfree <= MAX_GEMM_FREE_KF && tile_run_max <= (has_asrc ? 4 : 2) && t.G == 8) ? 2 : 1) : 0;
        if (t.lds_mode == 2 && tile_run_max > 2) P.gemm_run4 = true;   // needs the RARE variant of k_build (pseudo-observations: it is taken)
        if (t.lds_mode == 2) P.max_gemm_free = std::max(P.max_gemm_free, nfree);
        // (a guard, not reachable today: a landmark of a tile has at most 64 observations, and a tile of several landmarks lists at most
        // MAX_TILE_KF key-frames; long tracks are not in the tiles' lists)
        if ((int)kfs.size() > 64) { err = "set_windows: a landmark is observed from more than 64 key-frames"; return SADVIO_E_INVALID_ARG; }
        t.kf_off = (int)P.tile_kf.size(); t.n_kf = (int)kfs.size(); t.n_free = t.lds_mode ? nfree : 0;
        int rank = 0;
        for (size_t i = 0; i < kfs.size(); i++) {
            const int kf = kfs[i];
            slot_of[kf] = (int)i;
            P.tile_kf.push_back(d.kf_base + kf);
            const bool is_const = F.kf_const && F.kf_const[kf];
            if (is_const) P.tile_row.push_back(-1);
            else if (t.lds_mode) P.tile_row.push_back(6 * rank++);
            else P.tile_row.push_back(6 * P.kf_fidx[d.kf_base + kf]);  // global mode: 6 * free index of the window
        }
        for (int li = l_begin; li < l; li++) {
            if (has_long && is_long[lm_at(li)]) continue;   // (its observations carry no tile slot: long_slot)
            for (int o = F.lmk_obs_ptr[lm_at(li)]; o < F.lmk_obs_ptr[lm_at(li) + 1]; o++)
                P.obs_slot[d.obs_base + o] = (unsigned char)slot_of[pkf[o]];
        }
        P.max_tile_kf = std::max(P.max_tile_kf, t.n_kf);
        P.max_tile_free = std::max(P.max_tile_free, t.n_free);
        P.tiles.push_back(t);
        if (F.n_lmk == 0) break;
    }
    d.tile_end = (int)P.tiles.size();
    for (int ti = d.tile_begin; ti < d.tile_end; ti++) { P.tiles[ti].win_tile0 = d.tile_begin; P.tiles[ti].win_ntiles = d.tile_end - d.tile_begin; }
    return SADVIO_OK;
}

// Chunk tables of the throughput kernels: a tile's consecutive landmarks in chunks of <= LM_CHUNK landmarks and <= 64 observations;
// obs_lslot = index of the observation's landmark inside its chunk. Then the launch order of the tiles and k_lm_pass's work list.
inline void layout_chunks(const LayoutIn& in, LayoutPlan& P) {
    const int lmk_b = P.n_lmk_tot, obs_b = P.n_obs_tot;
    const auto& lmk_ob = P.lmk_ob; const auto& lmk_oe = P.lmk_oe;
    auto& chunk_ob = P.chunk_ob; auto& chunk_lm = P.chunk_lm;   // chunk starts + one sentinel (landmarks and observations are globally consecutive)
    chunk_ob.clear(); chunk_lm.clear();
    P.obs_lslot.assign(std::max(obs_b, 1), 0);
    const bool want_lm = P.want_lm = layout_want_lm(in, P);
    P.lm_ok = want_lm && !P.tiles.empty();
    P.lm_landmarks = 0;
    P.lm_sub_obs = 0;
    for (auto& t : P.tiles) {
        if (!want_lm) { t.chunk0 = t.chunk1 = 0; continue; }
        t.chunk0 = (int)chunk_lm.size();
        if (t.lds_mode != 2) P.lm_ok = false;
        int l = t.lmk0;
        while (l < t.lmk1) {   // (every landmark has <= 64 observations: a chunk holds at least one)
            chunk_lm.push_back(l); chunk_ob.push_back(lmk_ob[l]);
            int nl = 0, no = 0;
            while (l < t.lmk1 && nl < LM_CHUNK && no + (lmk_oe[l] - lmk_ob[l]) <= 64) {
                for (int o = lmk_ob[l]; o < lmk_oe[l]; o++) P.obs_lslot[o] = (unsigned char)nl;
                no += lmk_oe[l] - lmk_ob[l]; nl++; l++;
            }
        }
        t.chunk1 = (int)chunk_lm.size();
        P.lm_landmarks += t.lmk1 - t.lmk0;
    }
    chunk_lm.push_back(lmk_b); chunk_ob.push_back(obs_b);
    if (want_lm) {
        // k_lm_pass stages the observation constants of LM_PASS_THREADS consecutive landmarks of a tile in LDS: the largest such block
        P.lm_max_cam = 1; P.lm_ksub = 1;
        for (const auto& t : P.tiles) {
            for (int l0 = t.lmk0; l0 < t.lmk1; l0 += LM_PASS_THREADS) {
                const int l1 = std::min(l0 + LM_PASS_THREADS, t.lmk1);
                P.lm_sub_obs = std::max(P.lm_sub_obs, lmk_oe[l1 - 1] - lmk_ob[l0]);
            }
            P.lm_max_cam = std::max(P.lm_max_cam, t.n_cam);
            P.lm_ksub = std::max(P.lm_ksub, (t.lmk1 - t.lmk0 + LM_PASS_THREADS - 1) / LM_PASS_THREADS);
        }
        P.lm_sub_obs = (P.lm_sub_obs + 3) & ~3;
    }
    // launch order of the throughput kernels: longest tiles first (LPT), so that the last workgroups to start are short ones
    auto& perm = P.perm;
    perm.resize(P.tiles.size());
    for (size_t i = 0; i < perm.size(); i++) perm[i] = (int)i;
    if (want_lm && !in.no_lpt)
        std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) {
            return P.tiles[a].chunk1 - P.tiles[a].chunk0 > P.tiles[b].chunk1 - P.tiles[b].chunk0; });
    // work list of k_lm_pass: the sub-blocks (LM_PASS_THREADS landmarks) of every tile, in the same order
    P.sub.clear();
    if (in.lm_subs > 0) P.lm_sub_per_item = in.lm_subs;
    if (want_lm)
        for (int ti : perm) {
            const Tile& t = P.tiles[ti];
            for (int q = 0, l0 = t.lmk0; l0 < t.lmk1; l0 += LM_PASS_THREADS * P.lm_sub_per_item, q += P.lm_sub_per_item) { P.sub.push_back(ti); P.sub.push_back(q); }
        }
    P.lm_n_sub = (int)P.sub.size() / 2;
    if (P.tile_kf.empty()) { P.tile_kf.push_back(0); P.tile_row.push_back(-1); }   // (no table is uploaded empty)
    if (P.tile_lmk.empty()) P.tile_lmk.push_back(0);
    if (P.long_rec.empty()) P.long_rec.assign(LONG_REC, 0);
    if (P.long_kf.empty()) P.long_kf.push_back(0);
    if (P.long_slot.empty()) P.long_slot.push_back(0);
    // first-round packets of the latency kernels (k_pre_packets): few-tile submissions only, the single-window / small-batch regime
    P.pre_ok = !P.tiles.empty() && P.tiles.size() <= PRE_MAX_TILES && !in.no_pre;
    P.single_round = !P.tiles.empty();
    for (const Tile& t : P.tiles) P.single_round = P.single_round && t.n_lmk <= BUILD_WAVES * (64 / t.G);
}

// Layout of the reduced systems of all windows: [free key-frames (dpf each) | prior-kept landmarks (3 each) | lines (6 each)].
// Planned with the tiles and again whenever a factor list that holds landmarks or lines in the reduced system changes.
// A resident prior that changed after it was attached is refused before anything of the plan changes: what the device holds
// then still matches the plan.
inline int layout_reduced_plan(const LayoutIn& in, LayoutPlan& P, std::string& err) {
    const int n_windows = (int)P.wins.size();
    const auto& dpriors = *in.dprior_per_win;
    for (int w = 0; w < n_windows && w < (int)dpriors.size(); w++) {
        const DensePriorHost& D = dpriors[w];
        if (D.n_full > 0 && D.resident && (!in.prior_valid || in.prior_serial != D.serial || in.prior_n_full != D.n_full || in.prior_n != D.n)) {
            err = "the handle's prior changed after set_dense_prior(SADVIO_PRIOR_RESIDENT) attached it to a window: attach it again"; return SADVIO_E_STATE;
        }
    }
    // without long_priors a long track cannot be held in the reduced system (refused before anything of the plan changes). With it
    // keep_landmark below takes a long track as it takes any landmark: lmk_red, lmk_const_red = 2 and ALL its observations on the kept
    // list (k_build_kept: one thread each, no per-landmark cap); it stays on the long list, whose kernels sum its pose-pose part and
    // take its step from the reduced solution (long_kernels.h, lcode == 2)
    if (P.n_long > 0 && !in.long_priors)
        for (int w = 0; w < n_windows && w < (int)dpriors.size(); w++) {
            const int lb = P.wins[w].d.lmk_base;
            const DensePriorHost& D = dpriors[w];
            bool bad = false;
            for (size_t i = 0; i < D.lmk_index.size(); i++) bad |= D.n_full > 0 && D.lmk_col[i] >= 0 && P.is_long[lb + D.lmk_index[i]];
            for (const sadvio_sparse_prior& sp : (*in.sparse_per_win)[w]) {
                if (sp.type != SADVIO_SPARSE_IMU_PRIOR && sp.type != SADVIO_SPARSE_RELATIVE_POSE) bad |= P.is_long[lb + sp.lmk0] != 0;
                if (sp.type == SADVIO_SPARSE_LMK_TO_LMK) bad |= P.is_long[lb + sp.lmk1] != 0;
            }
            if (bad) { err = "long tracks: a prior factor keeps or touches a landmark on the long path"; return SADVIO_E_INVALID_ARG; }
        }
    int red_b = 0; long long s_b = 0;
    P.max_np = 0; P.n_big = 0;
    auto& lmk_red = P.lmk_red; auto& lmk_const = P.lmk_const_red; auto& kept = P.kept; auto& dp_ints = P.dp_ints;
    auto& sparse = P.sparse; auto& sp_list = P.sp_list; auto& lines = P.lines; auto& lobs = P.lobs;
    lmk_red.assign(std::max(P.n_lmk_tot, 1), -1);
    lmk_const = P.lmk_const;
    kept.clear(); dp_ints.clear(); sparse.clear(); sp_list.clear(); lines.clear(); lobs.clear(); P.preps.clear();
    long long dp_total = 0;
    bool any_red = false;
    std::vector<int> kind, index, col;
    for (int w = 0; w < n_windows; w++) {
        WinDev& d = P.wins[w].d;
        const DensePriorHost& D = dpriors[w];
        int n_red = 0;
        d.dp_n_full = d.dp_n = 0; d.dp_off = 0; d.dp_int_off = 0;
        d.kept_begin = (int)kept.size() / 3;
        auto keep_landmark = [&](int gl) {   // 3 reduced columns behind the poses, and its observations into the kept list
            lmk_red[gl] = d.dpf * d.n_free_kf + 3 * n_red; n_red++;
            lmk_const[gl] = 2; any_red = true;
            for (int o = P.lmk_ob[gl]; o < P.lmk_oe[gl]; o++) { kept.push_back(o); kept.push_back(gl); kept.push_back(w); }
        };
        if (D.n_full > 0) {
            const int n = D.n, nf = D.n_full;
            kind.assign(n, -1); index.assign(n, 0); col.assign(n, -1);
            if (D.kf_keep >= 0) {
                const int g = d.kf_base + D.kf_keep, fi = P.kf_fidx[g];
                for (int q = 0; q < 15; q++) {
                    const int a = D.kf_col + q;
                    if (q < 6) { kind[a] = 0; index[a] = 6 * g + q; }
                    else { kind[a] = 1 + (q - 6) / 3; index[a] = 3 * g + (q - 6) % 3; }
                    col[a] = (fi >= 0 && q < d.dpf) ? fi * d.dpf + q : -1;
                }
            }
            for (size_t i = 0; i < D.lmk_index.size(); i++) {
                if (D.lmk_col[i] < 0) continue;
                const int gl = d.lmk_base + D.lmk_index[i];
                const bool is_const = lmk_const[gl] == 1;
                if (!is_const) keep_landmark(gl);
                for (int a = 0; a < 3; a++) {
                    kind[D.lmk_col[i] + a] = 4; index[D.lmk_col[i] + a] = 3 * gl + a;
                    col[D.lmk_col[i] + a] = is_const ? -1 : lmk_red[gl] + a;
                }
            }
            d.dp_n_full = nf; d.dp_n = n;
            d.dp_int_off = (int)dp_ints.size();
            dp_ints.insert(dp_ints.end(), kind.begin(), kind.end());
            dp_ints.insert(dp_ints.end(), index.begin(), index.end());
            dp_ints.insert(dp_ints.end(), col.begin(), col.end());
            d.dp_off = dp_total;
            P.preps.push_back({d.dp_off, nf, n, w});
            dp_total += (long long)nf * n + (long long)n * nf + (long long)n * n + nf + n + nf + 2 + 3LL * ((nf + 3) / 4);   // J, Jt, H (device-filled), r0, dx, r scratch, cost slot, -, row-block partial sums (sharded windows)
            dp_total += dp_total & 1;
        }
        // landmarks touched by sparse prior factors stay in the reduced system as well
        d.sp_begin = (int)sparse.size();
        d.spl_begin = (int)sp_list.size();
        const auto& sps = (*in.sparse_per_win)[w];
        for (size_t sk = 0; sk < sps.size(); sk++) {
            const sadvio_sparse_prior& s = sps[sk];
            SparseDev o{};
            o.type = s.type; o.win = w;
            const bool elim = w < (int)P.sp_elim.size() && sk < P.sp_elim[w].size() && P.sp_elim[w][sk];
            if (elim) {
                // rides the Schur elimination as two pseudo-observations of its landmark: only its constants are needed
                o.type = 4; o.kf = d.kf_base + s.kf; o.lmk0 = d.lmk_base + s.lmk0; o.lmk1 = -1;
                memcpy(o.delta, s.delta, 24); memcpy(o.W, s.sqrt_inf, sizeof(o.W));
                sparse.push_back(o);
                continue;
            }
            o.kf = s.kf >= 0 ? d.kf_base + s.kf : -1;
            const bool rel = s.type == SADVIO_SPARSE_RELATIVE_POSE;
            if (rel) { o.type = 5; o.kf2 = d.kf_base + s.kf_b; }   // internal type 4 is the pseudo-observation form above
            const int ls[2] = {(s.type == SADVIO_SPARSE_IMU_PRIOR || rel) ? -1 : s.lmk0, s.type == SADVIO_SPARSE_LMK_TO_LMK ? s.lmk1 : -1};
            int gls[2] = {-1, -1};
            for (int q = 0; q < 2; q++) {
                if (ls[q] < 0) continue;
                const int gl = d.lmk_base + ls[q];
                gls[q] = gl;
                if (lmk_const[gl] == 1 || lmk_red[gl] >= 0) continue;
                keep_landmark(gl);
            }
            o.lmk0 = gls[0]; o.lmk1 = gls[1];
            memcpy(o.T_prior, s.T_prior, sizeof(o.T_prior)); memcpy(o.v_prior, s.v_prior, 24); memcpy(o.ba_prior, s.ba_prior, 24);
            memcpy(o.bg_prior, s.bg_prior, 24); memcpy(o.delta, s.delta, 24); memcpy(o.W, s.sqrt_inf, sizeof(o.W));
            sp_list.push_back((int)sparse.size());
            sparse.push_back(o);
        }
        d.sp_end = (int)sparse.size();
        d.spl_end = (int)sp_list.size();
        d.kept_end = (int)kept.size() / 3;
        d.n_red = n_red;
        d.Np = d.n_free_kf * d.dpf + 3 * n_red;
        // linexd landmarks: 6 columns each after the kept landmarks
        d.line_begin = (int)lines.size(); d.lobs_begin = (int)lobs.size();
        if (w < (int)in.lines_per_win->size()) {
            const LineSetHost& LS = (*in.lines_per_win)[w];
            for (int l = 0; l < LS.n(); l++) {
                LineDev o{};
                memcpy(o.T, &LS.T[12 * (size_t)l], 96); memcpy(o.model, &LS.model[6 * (size_t)l], 48);
                o.win = w; o.col = -1;
                if (!(LS.is_const.size() && LS.is_const[l])) { o.col = d.Np; d.Np += 6; }
                const int ms = d.factor_type == SADVIO_FACTOR_PIXEL ? 4 : 6;
                for (int ob = LS.ptr[l]; ob < LS.ptr[l + 1]; ob++) {
                    LineObsDev q{};
                    q.line = (int)lines.size(); q.kf = d.kf_base + LS.obs_kf[ob]; q.cam = d.cam_base + (*in.src)[w].cam_map[LS.obs_cam[ob]]; q.win = w;
                    memcpy(q.meas, &LS.meas[(size_t)ms * ob], sizeof(double) * ms);
                    lobs.push_back(q);
                }
                lines.push_back(o);
            }
        }
        d.line_end = (int)lines.size(); d.lobs_end = (int)lobs.size();
        // reduced systems that fit LDS are kept as a packed lower triangle (16-byte aligned); larger ones as a
        // full row-major matrix (lower triangle used) that the library factorisation works on in place
        d.ld = d.Np > MAX_LDS_NP ? d.Np : 0;
        d.S_off = s_b; d.red_off = red_b;
        red_b += d.Np; s_b += d.ld ? (((long long)d.Np * d.Np + 1) & ~1LL) : (long long)c16_size(d.Np);   // LDS-sized systems: the tile-packed image of chol16.h
        if (d.ld) P.n_big++; else P.max_np = std::max(P.max_np, d.Np);
        for (int ti = d.tile_begin; ti < d.tile_end; ti++) {
            Tile& t = P.tiles[ti];
            t.Np = d.Np; t.red_off = d.red_off; t.S_off = d.S_off; t.ld = d.ld;
        }
    }
    P.np_tot = red_b; P.s_tot = s_b; P.dp_total = dp_total;
    P.n_kept = (int)kept.size() / 3;
    P.has_lmk_const = P.user_lmk_const || any_red;
    // one allocation [S | gred | gfull | hdiag | rank_b]: a window sharded over several GPUs all-reduces it whole
    P.n_rank_b = (long long)n_windows * in.world * 4;
    P.red_total = s_b + 3LL * red_b + P.n_rank_b;
    if (kept.empty()) kept.assign(3, 0);   // (no table is uploaded empty)
    if (dp_ints.empty()) dp_ints.push_back(0);
    return SADVIO_OK;
}

// The whole plan of a batch whose windows passed check_flat_window. lap(name) is called behind the steps (SADVIO_DEBUG=8192).
template <typename Lap>
inline int layout_plan(const LayoutIn& in, LayoutPlan& P, std::string& err, Lap&& lap) {
    const int n_windows = (int)in.src->size();
    layout_views(in, P);
    lap("views");
    for (int w = 0; w < n_windows; w++) {
        const sadvio_flat_window& F = P.views[w];
        if (F.factor_type != P.views[0].factor_type || (F.factor_type != SADVIO_FACTOR_PIXEL && F.factor_type != SADVIO_FACTOR_ANGULAR)) {
            err = "set_windows: all windows of a batch must share one factor_type";
            return SADVIO_E_INVALID_ARG;
        }
    }
    layout_windows(n_windows, P.views.data(), P);
    if (const int rc = layout_long(in, P, err)) return rc;
    lap("  validate");
    layout_concat_begin(P);
    for (int w = 0; w < n_windows; w++) {
        layout_concat(P, w);
        lap("  concat");
        int rc = layout_sort(in, P, w, err);
        if (rc != SADVIO_OK) return rc;
        rc = layout_long_lists(P, w, err);
        if (rc != SADVIO_OK) return rc;
        lap("  sort+permute");
        rc = layout_tiles(in, P, w, err);
        if (rc != SADVIO_OK) return rc;
    }
    lap("concat+tiles");
    layout_chunks(in, P);
    lap("chunks");
    const int rc = layout_reduced_plan(in, P, err);
    lap("layout_reduced");
    return rc;
}

}  // namespace sadvio

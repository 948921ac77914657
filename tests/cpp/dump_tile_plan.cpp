// Prints what the host-only planner (sadvio_amd/csrc/layout_plan.h) makes of the track structure of a batch of windows, so that
// tests/test_tile_plan_cpu.py can hold every window of the first-step tests to the tile variant it is meant to reach. Host only.
// Reads from stdin (whitespace separated integers):
//   lm tile_rounds lm_subs contig_tiles no_pre            the LayoutIn switches (lm: -1 = not set)
//   n_windows, then per window:
//     n_kf n_cam has_imu n_lmk
//     kf_const[n_kf]
//     lmk_const[n_lmk]
//     per landmark: n_obs, then n_obs pairs (key-frame, camera) in caller order
// Prints:
//   P lm_ok lm_ksub lm_n_sub pre_ok gemm_run4 n_tiles
//   T tile window lds_mode G n_lmk n_free n_kf packed n_chunks, then per chunk: landmarks observations
#include <cstdio>
#include <cstdlib>

#include "../../sadvio_amd/csrc/layout_plan.h"

using namespace sadvio;

static int next_int() {
    int v = 0;
    if (scanf("%d", &v) != 1) { fprintf(stderr, "dump_tile_plan: input ends early\n"); exit(2); }
    return v;
}

// What set_windows stores of a caller's window: the deep copy (geometry is irrelevant to the planner: identity poses, one distinct
// set of intrinsics per camera so that none is de-duplicated)
static SrcWin read_window(int& has_imu) {
    SrcWin S;
    const int n_kf = next_int(), n_cam = next_int();
    has_imu = next_int();
    const int n_lmk = next_int();
    S.kf_T.assign(12 * (size_t)n_kf, 0.0);
    for (int k = 0; k < n_kf; k++) { S.kf_T[12 * k] = S.kf_T[12 * k + 5] = S.kf_T[12 * k + 10] = 1.0; S.kf_T[12 * k + 3] = k; }
    S.kf_const.resize(n_kf);
    for (int k = 0; k < n_kf; k++) S.kf_const[k] = (uint8_t)next_int();
    for (int c = 0; c < n_cam; c++) {
        const double K[4] = {400.0 + c, 400.0 + c, 320.0, 240.0};
        S.cam_K.insert(S.cam_K.end(), K, K + 4);
        for (int q = 0; q < 12; q++) S.cam_T.push_back(q % 5 == 0 ? 1.0 : 0.0);
        S.cam_sigma.push_back(1.0);
    }
    S.lmk_const.resize(n_lmk);
    bool any_const = false;
    for (int l = 0; l < n_lmk; l++) { S.lmk_const[l] = (uint8_t)next_int(); any_const |= S.lmk_const[l] != 0; }
    if (!any_const) S.lmk_const.clear();
    S.lmk_obs_ptr.assign(1, 0);
    for (int l = 0; l < n_lmk; l++) {
        const int n = next_int();
        for (int o = 0; o < n; o++) {
            S.obs_kf.push_back(next_int()); S.obs_cam.push_back(next_int());
            S.obs_meas.push_back(0.0); S.obs_meas.push_back(0.0);
        }
        S.lmk_obs_ptr.push_back((int32_t)S.obs_kf.size());
        for (int q = 0; q < 3; q++) S.lmk_p.push_back(l + 0.25 * q);
    }
    return S;
}

static void set_view(SrcWin& S, int has_imu) {
    sadvio_flat_window& v = S.v;
    memset(&v, 0, sizeof(v));
    v.n_kf = (int32_t)S.kf_const.size(); v.n_cam = (int32_t)S.cam_sigma.size(); v.n_lmk = (int32_t)S.lmk_obs_ptr.size() - 1; v.n_obs = (int32_t)S.obs_kf.size();
    v.factor_type = SADVIO_FACTOR_PIXEL; v.has_imu = has_imu;
    v.kf_T_f_w = S.kf_T.data(); v.kf_const = S.kf_const.data();
    v.cam_K = S.cam_K.data(); v.cam_T_s_f = S.cam_T.data(); v.cam_sigma = S.cam_sigma.data();
    v.lmk_p = S.lmk_p.data(); v.lmk_obs_ptr = S.lmk_obs_ptr.data(); v.lmk_const = S.lmk_const.empty() ? nullptr : S.lmk_const.data();
    v.obs_kf = S.obs_kf.data(); v.obs_cam = S.obs_cam.data(); v.obs_meas = S.obs_meas.data();
}

int main() {
    LayoutIn in;
    in.lm = next_int(); in.tile_rounds = next_int(); in.lm_subs = next_int();
    in.contig_tiles = next_int() != 0; in.no_pre = next_int() != 0;
    const int n_windows = next_int();
    std::vector<SrcWin> src;
    std::vector<int> has_imu(n_windows, 0);
    for (int w = 0; w < n_windows; w++) src.push_back(read_window(has_imu[w]));
    std::vector<std::vector<sadvio_sparse_prior>> sparse(n_windows);
    std::vector<DensePriorHost> dprior(n_windows);
    std::vector<LineSetHost> lines(n_windows);
    std::string err;
    for (int w = 0; w < n_windows; w++) {
        set_view(src[w], has_imu[w]);
        if (check_flat_window(src[w].v, w, err) != SADVIO_OK) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    }
    in.src = &src; in.sparse_per_win = &sparse; in.dprior_per_win = &dprior; in.lines_per_win = &lines;
    LayoutPlan P;
    if (layout_plan(in, P, err, [](const char*) {}) != SADVIO_OK) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    printf("P %d %d %d %d %d %d\n", P.lm_ok ? 1 : 0, P.lm_ksub, P.lm_n_sub, P.pre_ok ? 1 : 0, P.gemm_run4 ? 1 : 0, (int)P.tiles.size());
    for (size_t ti = 0; ti < P.tiles.size(); ti++) {
        const Tile& t = P.tiles[ti];
        printf("T %d %d %d %d %d %d %d %d %d", (int)ti, t.w, t.lds_mode, t.G, t.n_lmk, t.n_free, t.n_kf, t.lmk_off >= 0 ? 1 : 0, t.chunk1 - t.chunk0);
        for (int c = t.chunk0; c < t.chunk1; c++) printf(" %d %d", P.chunk_lm[c + 1] - P.chunk_lm[c], P.chunk_ob[c + 1] - P.chunk_ob[c]);
        printf("\n");
    }
    return 0;
}

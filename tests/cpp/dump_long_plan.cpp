// Prints what the host-only planner (sadvio_amd/csrc/layout_plan.h) makes of a batch of windows that may hold long tracks (landmarks
// with at least long_min observations: long_kernels.h), for tests/test_long_plan_cpu.py. Host only; a sanitizer build of this
// program is the place to check the planner's new tables.
// Reads from stdin (whitespace separated integers):
//   long_min                                              LayoutIn::long_min (0: no long path; 65 on a handle that asked for long tracks; SADVIO_LONG_MIN)
//   then dump_tile_plan's input: the switches, n_windows, per window its sizes, flags and tracks
// Prints:
//   P n_tiles n_long long_max_kf lm_ok
//   L index window landmark n_obs n_kf | the track's key-frames | the slot of each of its observations (device order)
//   T tile window lds_mode G n_lmk n_free n_kf kmax listed | the tile's key-frames | its rows | its landmarks (window-local)
//   O window | obs_kf of every observation in device order | obs_perm
// or, when the planner refuses the batch: E <its text>
#include <cstdio>
#include <cstdlib>

#include "../../sadvio_amd/csrc/layout_plan.h"

using namespace sadvio;

static int next_int() {
    int v = 0;
    if (scanf("%d", &v) != 1) { fprintf(stderr, "dump_long_plan: input ends early\n"); exit(2); }
    return v;
}

// (as dump_tile_plan.cpp: geometry is irrelevant to the planner)
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
    in.long_min = next_int();
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
        if (check_flat_window(src[w].v, w, err) != SADVIO_OK) { printf("E %s\n", err.c_str()); return 0; }
    }
    in.src = &src; in.sparse_per_win = &sparse; in.dprior_per_win = &dprior; in.lines_per_win = &lines;
    LayoutPlan P;
    if (layout_plan(in, P, err, [](const char*) {}) != SADVIO_OK) { printf("E %s\n", err.c_str()); return 0; }
    printf("P %d %d %d %d\n", (int)P.tiles.size(), P.n_long, P.long_max_kf, P.lm_ok ? 1 : 0);
    for (int i = 0; i < P.n_long; i++) {
        const int* r = &P.long_rec[(size_t)LONG_REC * i];
        const WinDev& d = P.wins[r[1]].d;
        printf("L %d %d %d %d %d |", i, r[1], r[0] - d.lmk_base, r[5], r[3]);
        for (int k = 0; k < r[3]; k++) printf(" %d", P.long_kf[r[2] + k] - d.kf_base);
        printf(" |");
        for (int o = 0; o < r[5]; o++) printf(" %d", P.long_slot[r[4] + o]);
        printf("\n");
    }
    for (size_t ti = 0; ti < P.tiles.size(); ti++) {
        const Tile& t = P.tiles[ti];
        const WinDev& d = P.wins[t.w].d;
        printf("T %d %d %d %d %d %d %d %d %d |", (int)ti, t.w, t.lds_mode, t.G, t.n_lmk, t.n_free, t.n_kf, t.kmax, t.lmk_off >= 0 ? 1 : 0);
        for (int k = 0; k < t.n_kf; k++) printf(" %d", P.tile_kf[t.kf_off + k] - d.kf_base);
        printf(" |");
        for (int k = 0; k < t.n_kf; k++) printf(" %d", P.tile_row[t.kf_off + k]);
        printf(" |");
        for (int k = 0; k < t.n_lmk; k++) printf(" %d", (t.lmk_off >= 0 ? P.tile_lmk[t.lmk_off + k] : t.lmk0 + k) - d.lmk_base);
        printf("\n");
    }
    for (int w = 0; w < n_windows; w++) {
        const WinDev& d = P.wins[w].d;
        printf("O %d |", w);
        for (int o = 0; o < d.n_obs; o++) printf(" %d", P.obs_kf[d.obs_base + o] - d.kf_base);
        printf(" |");
        for (int o = 0; o < d.n_obs; o++) printf(" %d", P.obs_perm[d.obs_base + o]);
        printf("\n");
    }
    return 0;
}

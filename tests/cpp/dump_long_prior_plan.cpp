// Prints what the host-only planner (sadvio_amd/csrc/layout_plan.h) makes of windows whose long tracks (landmarks with at least long_min
// observations: long_kernels.h) are held in the reduced system by priors, for tests/test_long_prior_plan_cpu.py. Host only.
// Reads from stdin (whitespace separated integers):
//   long_min long_priors                                  LayoutIn::long_min, LayoutIn::long_priors (SADVIO_CFG_LONG_TRACK_PRIORS)
//   then dump_tile_plan's input: the switches, n_windows, per window its sizes, flags and tracks
//   then per window: n_keep and the landmarks a dense prior keeps (columns 3 i, an identity J) | n_p2l and (key-frame, landmark) of
//   pose-to-landmark factors of the sparse prior
// Prints:
//   P n_long n_kept
//   W window Np n_red n_obs_planned n_obs_given           (n_obs_planned - n_obs_given: the pseudo-observations appended)
//   L index window landmark n_obs on_kept_list lmk_const_red lmk_red
//   K window landmark on_kept_list lmk_const_red lmk_red  for every landmark with lmk_red >= 0 that is not a long track
//   S window factor type lmk0                             the sparse factors as planned (type 4: rides the elimination as pseudo-observations)
// or, when the planner refuses the batch: E <its text>
#include <cstdio>
#include <cstdlib>

#include "../../sadvio_amd/csrc/layout_plan.h"

using namespace sadvio;

static int next_int() {
    int v = 0;
    if (scanf("%d", &v) != 1) { fprintf(stderr, "dump_long_prior_plan: input ends early\n"); exit(2); }
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
    in.long_min = next_int(); in.long_priors = next_int() != 0;
    in.lm = next_int(); in.tile_rounds = next_int(); in.lm_subs = next_int();
    in.contig_tiles = next_int() != 0; in.no_pre = next_int() != 0;
    const int n_windows = next_int();
    std::vector<SrcWin> src;
    std::vector<int> has_imu(n_windows, 0);
    for (int w = 0; w < n_windows; w++) src.push_back(read_window(has_imu[w]));
    std::vector<std::vector<sadvio_sparse_prior>> sparse(n_windows);
    std::vector<DensePriorHost> dprior(n_windows);
    std::vector<LineSetHost> lines(n_windows);
    for (int w = 0; w < n_windows; w++) {
        const int n_keep = next_int();
        DensePriorHost& D = dprior[w];
        for (int i = 0; i < n_keep; i++) { D.lmk_index.push_back(next_int()); D.lmk_col.push_back(3 * i); }
        if (n_keep > 0) {
            D.n = D.n_full = 3 * n_keep;
            D.J.assign((size_t)D.n * D.n, 0.0); D.r0.assign(D.n, 0.0);
            for (int i = 0; i < D.n; i++) D.J[(size_t)i * D.n + i] = 1.0;
        }
        const int n_p2l = next_int();
        for (int i = 0; i < n_p2l; i++) {
            sadvio_sparse_prior s;
            memset(&s, 0, sizeof(s));
            s.type = SADVIO_SPARSE_POSE_TO_LMK; s.kf = next_int(); s.lmk0 = next_int(); s.lmk1 = -1;
            s.sqrt_inf[0] = s.sqrt_inf[4] = s.sqrt_inf[8] = 1.0;
            sparse[w].push_back(s);
        }
    }
    std::string err;
    for (int w = 0; w < n_windows; w++) {
        set_view(src[w], has_imu[w]);
        if (check_flat_window(src[w].v, w, err) != SADVIO_OK) { printf("E %s\n", err.c_str()); return 0; }
    }
    in.src = &src; in.sparse_per_win = &sparse; in.dprior_per_win = &dprior; in.lines_per_win = &lines;
    LayoutPlan P;
    if (layout_plan(in, P, err, [](const char*) {}) != SADVIO_OK) { printf("E %s\n", err.c_str()); return 0; }
    std::vector<int> on_list(std::max(P.n_lmk_tot, 1), 0);
    for (int e = 0; e < P.n_kept; e++) {
        const int o = P.kept[3 * e], gl = P.kept[3 * e + 1];
        if (o < P.lmk_ob[gl] || o >= P.lmk_oe[gl]) { printf("E kept entry %d: observation %d is not one of landmark %d\n", e, o, gl); return 0; }
        on_list[gl]++;
    }
    printf("P %d %d\n", P.n_long, P.n_kept);
    for (int w = 0; w < n_windows; w++) {
        const WinDev& d = P.wins[w].d;
        printf("W %d %d %d %d %d\n", w, d.Np, d.n_red, d.n_obs, P.n_obs_user[w]);
    }
    for (int i = 0; i < P.n_long; i++) {
        const int* r = &P.long_rec[(size_t)LONG_REC * i];
        const WinDev& d = P.wins[r[1]].d;
        printf("L %d %d %d %d %d %d %d\n", i, r[1], r[0] - d.lmk_base, r[5], on_list[r[0]], (int)P.lmk_const_red[r[0]], P.lmk_red[r[0]]);
    }
    for (int w = 0; w < n_windows; w++) {
        const WinDev& d = P.wins[w].d;
        for (int l = 0; l < d.n_lmk; l++) {
            const int gl = d.lmk_base + l;
            if (P.lmk_red[gl] >= 0 && !P.is_long[gl]) printf("K %d %d %d %d %d\n", w, l, on_list[gl], (int)P.lmk_const_red[gl], P.lmk_red[gl]);
        }
        for (int k = d.sp_begin; k < d.sp_end; k++) printf("S %d %d %d %d\n", w, k - d.sp_begin, P.sparse[k].type, P.sparse[k].lmk0 - d.lmk_base);
    }
    return 0;
}

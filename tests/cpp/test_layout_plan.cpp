// The host-only layout planner (sadvio_amd/csrc/layout_plan.h) against hand-derived tables. The expected numbers follow from the
// constants of ba_types.h (256 lanes per workgroup, 8 .. 64 lanes per landmark, 24 / 20 / 5 key-frame limits of a tile, 174 columns
// in LDS, chunks of 12 landmarks and 64 observations) and are written as literals: nothing here calls the planner's own expressions.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>

#include "../../sadvio_amd/csrc/layout_plan.h"

using namespace sadvio;

static int g_fail = 0;
static const char* g_case = "";
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { printf("FAILED [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

typedef std::vector<std::pair<int, int>> Track;   // (key-frame, camera) of a landmark's observations, in caller order

struct Cam { double k, sigma; };   // distinct k = distinct intrinsics

// What set_windows stores of a caller's window: the deep copy with its view
static SrcWin make_src(int n_kf, const std::vector<int>& const_kfs, const std::vector<Cam>& cams, const std::vector<Track>& tracks,
                       const std::vector<int>& const_lmks = {}) {
    SrcWin S;
    S.kf_T.assign(12 * (size_t)n_kf, 0.0);
    for (int k = 0; k < n_kf; k++) { S.kf_T[12 * k] = S.kf_T[12 * k + 5] = S.kf_T[12 * k + 10] = 1.0; S.kf_T[12 * k + 3] = k; }
    S.kf_const.assign(n_kf, 0);
    for (int k : const_kfs) S.kf_const[k] = 1;
    for (const Cam& c : cams) {
        const double K[4] = {c.k, c.k, 320.0, 240.0};
        S.cam_K.insert(S.cam_K.end(), K, K + 4);
        for (int q = 0; q < 12; q++) S.cam_T.push_back(q % 5 == 0 ? 1.0 : 0.0);
        S.cam_sigma.push_back(c.sigma);
    }
    S.lmk_obs_ptr.assign(1, 0);
    for (size_t l = 0; l < tracks.size(); l++) {
        for (const auto& ob : tracks[l]) {
            S.obs_kf.push_back(ob.first); S.obs_cam.push_back(ob.second);
            S.obs_meas.push_back(1000.0 * l + 10.0 * ob.first + ob.second); S.obs_meas.push_back(0.5 + 1000.0 * l + 10.0 * ob.first + ob.second);
        }
        S.lmk_obs_ptr.push_back((int32_t)S.obs_kf.size());
        for (int q = 0; q < 3; q++) S.lmk_p.push_back(l + 0.25 * q);
    }
    if (!const_lmks.empty()) { S.lmk_const.assign(tracks.size(), 0); for (int l : const_lmks) S.lmk_const[l] = 1; }
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

struct Case {
    std::vector<SrcWin> src;
    std::vector<int> has_imu;
    std::vector<std::vector<sadvio_sparse_prior>> sparse;
    std::vector<DensePriorHost> dprior;
    std::vector<LineSetHost> lines;
    LayoutIn in;
    LayoutPlan P;
    std::string err;
    int rc = 0;
    void add(SrcWin S, int imu = 0) { src.push_back(std::move(S)); has_imu.push_back(imu); }
    void wire() {
        const size_t n = src.size();
        sparse.resize(n); dprior.resize(n); lines.resize(n);
        for (size_t w = 0; w < n; w++) set_view(src[w], has_imu[w]);
        in.src = &src; in.sparse_per_win = &sparse; in.dprior_per_win = &dprior; in.lines_per_win = &lines;
    }
    int run() {
        wire();
        for (size_t w = 0; w < src.size(); w++)
            if ((rc = check_flat_window(src[w].v, (int)w, err)) != SADVIO_OK) return rc;
        return rc = layout_plan(in, P, err, [](const char*) {});
    }
};

static long long s_doubles(int Np) {   // doubles of a window's S: full square (rounded up to even) above 174 columns, else 16 x 16 tiles of the lower block triangle of Np + 1 rows
    if (Np > 174) return ((long long)Np * Np + 1) / 2 * 2;
    const int b = (Np + 1 + 15) / 16;
    return (long long)b * (b + 1) / 2 * 256;
}

// The properties every plan has, whatever the windows
static void check_plan(Case& c, int tile_rounds = 1) {
    const LayoutPlan& P = c.P;
    CHECK(c.rc == SADVIO_OK);
    if (c.rc != SADVIO_OK) return;
    const int n_windows = (int)c.src.size();
    int kf_b = 0, cam_b = 0, lmk_b = 0, obs_b = 0, red_b = 0;
    long long s_b = 0;
    std::vector<int> in_tiles(std::max(P.n_lmk_tot, 1), 0);
    for (int w = 0; w < n_windows; w++) {
        const WinDev& d = P.wins[w].d;
        const SrcWin& S = c.src[w];
        CHECK(d.kf_base == kf_b && d.cam_base == cam_b && d.lmk_base == lmk_b && d.obs_base == obs_b);
        CHECK(d.n_kf == S.v.n_kf && d.n_lmk == S.v.n_lmk && d.n_obs >= S.v.n_obs && d.n_cam <= S.v.n_cam);
        kf_b += d.n_kf; cam_b += d.n_cam; lmk_b += d.n_lmk; obs_b += d.n_obs;
        // obs_perm: a permutation of the caller's observations, -1 for pseudo-observations
        std::vector<int> seen(std::max(S.v.n_obs, 1), 0);
        int n_pseudo = 0;
        for (int o = d.obs_base; o < d.obs_base + d.n_obs; o++) {
            const int p = P.obs_perm[o];
            if (p < 0) { CHECK(p == -1 && P.obs_cam[o] < 0); n_pseudo++; continue; }
            CHECK(p < S.v.n_obs);
            if (p < S.v.n_obs) {
                seen[p]++;
                CHECK(P.obs_kf[o] == d.kf_base + S.obs_kf[p] && P.obs_cam[o] == d.cam_base + S.cam_map[S.obs_cam[p]]);
                CHECK(P.obs_meas[2 * (size_t)o] == S.obs_meas[2 * (size_t)p] && P.obs_meas[2 * (size_t)o + 1] == S.obs_meas[2 * (size_t)p + 1]);
            }
        }
        for (int p = 0; p < S.v.n_obs; p++) CHECK(seen[p] == 1);
        CHECK(n_pseudo == d.n_obs - S.v.n_obs && P.n_obs_user[w] == S.v.n_obs);
        // a landmark's device observations: non-decreasing in key-frame, equal key-frames in caller order, caller's landmark
        for (int l = 0; l < d.n_lmk; l++) {
            const int gl = d.lmk_base + l;
            CHECK(P.lmk_ob[gl] >= d.obs_base && P.lmk_oe[gl] <= d.obs_base + d.n_obs && P.lmk_ob[gl] <= P.lmk_oe[gl]);
            if (l + 1 < d.n_lmk) CHECK(P.lmk_oe[gl] == P.lmk_ob[gl + 1]);
            for (int o = P.lmk_ob[gl]; o < P.lmk_oe[gl]; o++) {
                if (P.obs_perm[o] >= 0) CHECK(P.obs_perm[o] >= S.lmk_obs_ptr[l] && P.obs_perm[o] < S.lmk_obs_ptr[l + 1]);
                if (o == P.lmk_ob[gl]) continue;
                CHECK(P.obs_kf[o - 1] <= P.obs_kf[o]);
                if (P.obs_kf[o - 1] == P.obs_kf[o] && P.obs_perm[o - 1] >= 0 && P.obs_perm[o] >= 0) CHECK(P.obs_perm[o - 1] < P.obs_perm[o]);
            }
        }
        // tiles of the window
        CHECK(d.tile_end > d.tile_begin && (w == 0 ? d.tile_begin == 0 : d.tile_begin == P.wins[w - 1].d.tile_end));
        int free_of_win = 0;
        std::vector<int> fidx(d.n_kf);
        for (int k = 0; k < d.n_kf; k++) fidx[k] = S.kf_const[k] ? -1 : free_of_win++;
        CHECK(d.n_free_kf == free_of_win);
        for (int k = 0; k < d.n_kf; k++) CHECK(P.kf_fidx[d.kf_base + k] == fidx[k]);
        for (int ti = d.tile_begin; ti < d.tile_end; ti++) {
            const Tile& t = P.tiles[ti];
            CHECK(t.w == w && t.win_tile0 == d.tile_begin && t.win_ntiles == d.tile_end - d.tile_begin && t.first_of_window == (ti == d.tile_begin));
            CHECK(t.cam_base == d.cam_base && t.n_cam == d.n_cam && t.dpf == d.dpf);
            CHECK(t.Np == d.Np && t.red_off == d.red_off && t.S_off == d.S_off && t.ld == d.ld);
            CHECK(t.G >= 8 && t.G <= 64 && (t.G & (t.G - 1)) == 0 && t.kmax <= t.G && t.n_lmk <= tile_rounds * 256 / t.G);
            CHECK(t.lmk1 - t.lmk0 == t.n_lmk);
            std::set<int> kfs;
            int kmax = 1;
            std::vector<int> members;
            for (int i = 0; i < t.n_lmk; i++) members.push_back(t.lmk_off >= 0 ? P.tile_lmk[t.lmk_off + i] : t.lmk0 + i);
            for (int gl : members) {
                CHECK(gl >= d.lmk_base && gl < d.lmk_base + d.n_lmk);
                if (gl < 0 || gl >= P.n_lmk_tot) continue;
                in_tiles[gl]++;
                kmax = std::max(kmax, P.lmk_oe[gl] - P.lmk_ob[gl]);
                for (int o = P.lmk_ob[gl]; o < P.lmk_oe[gl]; o++) {
                    kfs.insert(P.obs_kf[o]);
                    CHECK(P.obs_slot[o] < t.n_kf && P.tile_kf[t.kf_off + P.obs_slot[o]] == P.obs_kf[o]);
                }
            }
            CHECK(t.kmax == kmax);
            CHECK((int)kfs.size() == t.n_kf);
            int i = 0, rank = 0;
            for (int kf : kfs) {   // (a std::set iterates in increasing order)
                if (i >= t.n_kf) break;
                CHECK(P.tile_kf[t.kf_off + i] == kf);
                const int fi = fidx[kf - d.kf_base];
                CHECK(P.tile_row[t.kf_off + i] == (fi < 0 ? -1 : t.lds_mode ? 6 * rank : 6 * fi));
                if (fi >= 0) rank++;
                i++;
            }
            CHECK(t.lds_mode >= 0 && t.lds_mode <= 2);
            CHECK(t.n_free == (t.lds_mode ? rank : 0));
            if (t.lds_mode == 2) CHECK(t.n_free <= 5);
            if (t.lds_mode == 1) CHECK(t.n_free <= 20 && t.n_kf <= 24);
            CHECK(t.n_kf <= P.max_tile_kf && t.n_free <= P.max_tile_free);
        }
        // reduced layout
        CHECK(d.red_off == red_b && d.S_off == s_b);
        CHECK(d.ld == (d.Np > 174 ? d.Np : 0));
        red_b += d.Np; s_b += s_doubles(d.Np);
    }
    for (int gl = 0; gl < P.n_lmk_tot; gl++) CHECK(in_tiles[gl] == 1);
    CHECK(P.n_kf_tot == kf_b && P.n_cam_tot == cam_b && P.n_lmk_tot == lmk_b && P.n_obs_tot == obs_b);
    CHECK(P.np_tot == red_b && P.s_tot == s_b && P.red_total == s_b + 3LL * red_b + 4LL * n_windows * c.in.world);
    CHECK(P.dp_total % 2 == 0);
}

// ---- the windows of the cases ----

// 40 landmarks x 2 - 4 observations over 4 key-frames (0 constant), every list sorted by key-frame, cameras alternating
static std::vector<Track> tracks40(bool reversed) {
    std::vector<Track> tr;
    for (int l = 0; l < 40; l++) {
        const int n = 2 + l % 3, start = l % (4 - n + 1);
        Track t;
        for (int i = 0; i < n; i++) t.push_back({start + i, (l + i) % 2});
        if (reversed) std::reverse(t.begin(), t.end());
        tr.push_back(t);
    }
    return tr;
}

static void case_contiguous_sorted_and_unsorted() {
    g_case = "1 contiguous cut, sorted input";
    Case a;
    a.add(make_src(4, {0}, {{400.0, 1.0}, {400.0, 1.0}}, tracks40(false)));
    a.in.contig_tiles = true;
    a.run(); check_plan(a);
    CHECK(a.P.n_cam_tot == 1 && a.src[0].cam_map == std::vector<int>({0, 0}));
    CHECK(a.P.tiles.size() == 2 && a.P.tiles[0].n_lmk == 32 && a.P.tiles[1].n_lmk == 8 && a.P.tiles[0].lmk_off == -1 && a.P.tiles[1].lmk0 == 32);
    CHECK(a.P.tiles[0].lds_mode == 2 && a.P.tiles[0].n_kf == 4 && a.P.tiles[0].n_free == 3 && a.P.tiles[0].G == 8);
    CHECK(a.P.n_obs_tot == 14 * 2 + 13 * 3 + 13 * 4);   // l % 3 == 0: 14 landmarks of 2, then 13 of 3 and 13 of 4
    for (int o = 0; o < a.P.n_obs_tot; o++) CHECK(a.P.obs_perm[o] == o);
    CHECK(a.P.wins[0].d.Np == 18 && a.P.wins[0].hb_lmk == 2 && a.P.pre_ok && !a.P.lm_ok);
    Case b;   // another sigma on the second camera: two stored cameras
    b.add(make_src(4, {0}, {{400.0, 1.0}, {400.0, 2.0}}, tracks40(false)));
    b.in.contig_tiles = true;
    b.run(); check_plan(b);
    CHECK(b.P.n_cam_tot == 2 && b.src[0].cam_map == std::vector<int>({0, 1}) && b.P.cam_isig[1] == 0.5);

    g_case = "2 unsorted input";
    Case r;
    r.add(make_src(4, {0}, {{400.0, 1.0}, {400.0, 1.0}}, tracks40(true)));
    r.in.contig_tiles = true;
    r.run(); check_plan(r);
    const LayoutPlan &A = a.P, &R = r.P;
    CHECK(A.obs_kf == R.obs_kf && A.obs_cam == R.obs_cam && A.obs_meas == R.obs_meas && A.lmk_ob == R.lmk_ob && A.lmk_oe == R.lmk_oe);
    CHECK(A.tile_kf == R.tile_kf && A.tile_row == R.tile_row && A.tile_lmk == R.tile_lmk && A.obs_slot == R.obs_slot && A.tiles.size() == R.tiles.size());
    for (size_t i = 0; i < A.tiles.size() && i < R.tiles.size(); i++) CHECK(!memcmp(&A.tiles[i], &R.tiles[i], sizeof(Tile)));
    CHECK(A.kf_T0 == R.kf_T0 && A.kf_fidx == R.kf_fidx && A.cam_K == R.cam_K && A.lmk_p == R.lmk_p && A.chunk_lm == R.chunk_lm && A.perm == R.perm);
    CHECK(A.wins[0].hb_lmk == R.wins[0].hb_lmk && A.s_tot == R.s_tot && A.np_tot == R.np_tot);
    for (int l = 0; l < 40; l++)
        for (int o = R.lmk_ob[l]; o < R.lmk_oe[l]; o++) CHECK(R.obs_perm[o] == R.lmk_ob[l] + (R.lmk_oe[l] - 1 - o));   // the reversal
    Case s;   // two observations of one key-frame from two cameras keep the caller's order
    s.add(make_src(3, {0}, {{400.0, 1.0}, {500.0, 1.0}}, {{{2, 0}, {1, 1}, {1, 0}}}));
    s.run(); check_plan(s);
    CHECK(s.P.obs_perm[0] == 1 && s.P.obs_perm[1] == 2 && s.P.obs_perm[2] == 0 && s.P.obs_cam[0] == 1 && s.P.obs_cam[1] == 0 && s.P.obs_cam[2] == 0);
}

static void case_observation_counts() {
    g_case = "3 observation counts";
    {   // 20 landmarks of 2 observations, landmark 3 with 9: 16 lanes per landmark from there on, 256 / 16 landmarks in the tile
        std::vector<Track> tr(20, Track{{6, 0}, {7, 0}});
        tr[3] = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}, {6, 0}, {7, 0}, {8, 0}};
        Case c;
        c.add(make_src(9, {0, 1, 2, 3, 4, 5}, {{400.0, 1.0}}, tr));
        c.in.contig_tiles = true;
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 2 && c.P.tiles[0].G == 16 && c.P.tiles[0].n_lmk == 16 && c.P.tiles[0].kmax == 9 && c.P.tiles[1].G == 8 && c.P.tiles[1].n_lmk == 4);
        CHECK(c.P.tiles[0].lds_mode == 1 && c.P.tiles[1].lds_mode == 2);   // 16 lanes per landmark: not on the MFMA path
    }
    std::vector<Cam> cams8, cams9;
    for (int i = 0; i < 9; i++) { if (i < 8) cams8.push_back({400.0 + i, 1.0}); cams9.push_back({400.0 + i, 1.0}); }
    Track t64;
    for (int k = 0; k < 8; k++) for (int cm = 0; cm < 8; cm++) t64.push_back({k, cm});
    {
        Case c;
        c.add(make_src(8, {0}, cams8, {t64}));
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 1 && c.P.tiles[0].G == 64 && c.P.tiles[0].kmax == 64 && c.P.tiles[0].lds_mode == 1);
    }
    {
        Track t65 = t64; t65.push_back({7, 0});
        Case c;
        c.add(make_src(8, {0}, cams8, {t65}));
        CHECK(c.run() == SADVIO_E_INVALID_ARG && c.err == "set_windows: a landmark has more than 64 observations");
        Case u;   // the same, unsorted
        std::reverse(t65.begin(), t65.end());
        u.add(make_src(8, {0}, cams8, {t65}));
        CHECK(u.run() == SADVIO_E_INVALID_ARG && u.err == "set_windows: a landmark has more than 64 observations");
    }
    {
        Track t9;
        for (int cm = 0; cm < 9; cm++) t9.push_back({1, cm});
        Case c;
        c.add(make_src(2, {0}, cams9, {t9}));
        CHECK(c.run() == SADVIO_E_INVALID_ARG && c.err == "set_windows: more than 8 distinct cameras per window");
    }
}

static Track over(int k0, int k1) { Track t; for (int k = k0; k <= k1; k++) t.push_back({k, 0}); return t; }

static void case_free_keyframe_limits() {
    g_case = "4 free key-frame limits";
    {   // tracks over (0,1), (2,3), (4,5), (6,7), 4 landmarks each: the third pair would bring the sixth free key-frame
        std::vector<Track> tr;
        for (int p = 0; p < 4; p++) for (int i = 0; i < 4; i++) tr.push_back(over(2 * p, 2 * p + 1));
        Case c;
        c.add(make_src(8, {}, {{400.0, 1.0}}, tr));
        c.in.contig_tiles = true;
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 2 && c.P.tiles[0].n_lmk == 8 && c.P.tiles[1].n_lmk == 8 && c.P.tiles[1].lmk0 == 8);
        for (const Tile& t : c.P.tiles) CHECK(t.lds_mode == 2 && t.n_free == 4);
        CHECK(c.P.max_gemm_free == 4 && c.P.wins[0].hb_lmk == 1);
    }
    {   // a landmark over 6 free key-frames: alone in its tile, LDS tile without the MFMA contraction
        Case c;
        c.add(make_src(8, {}, {{400.0, 1.0}}, {over(0, 1), over(0, 5), over(0, 1)}));
        c.in.contig_tiles = true;
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 3 && c.P.tiles[1].n_lmk == 1 && c.P.tiles[1].lds_mode == 1 && c.P.tiles[1].n_free == 6 && c.P.tiles[0].lds_mode == 2 && c.P.tiles[2].lds_mode == 2);
    }
    {   // 21 of the window's 23 free key-frames: global-atomics tile, rows from the WINDOW's free index — key-frames 1 and 2 are free
        // and not observed, so the tile's first key-frame (3) has free index 2 and row 12, where its rank in the tile would give 0
        Case c;
        c.add(make_src(24, {0}, {{400.0, 1.0}}, {over(3, 23)}));
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 1 && c.P.tiles[0].lds_mode == 0 && c.P.tiles[0].n_free == 0 && c.P.tiles[0].n_kf == 21 && c.P.tiles[0].G == 32);
        const int* row = &c.P.tile_row[c.P.tiles[0].kf_off];
        CHECK(row[0] == 12 && row[1] == 18 && row[2] == 24 && row[20] == 132);
        for (int i = 0; i < 21; i++) CHECK(row[i] == 12 + 6 * i && c.P.tile_kf[c.P.tiles[0].kf_off + i] == i + 3);
    }
    {   // a track over 25 key-frames (1 .. 20 constant, 21 .. 25 free): over the 24 a tile lists. Key-frame 0 is free and not observed:
        // the free index of key-frame 21 is 1
        std::vector<int> ck;
        for (int k = 1; k <= 20; k++) ck.push_back(k);
        Case c;
        c.add(make_src(26, ck, {{400.0, 1.0}}, {over(1, 25)}));
        c.run(); check_plan(c);
        CHECK(c.P.tiles.size() == 1 && c.P.tiles[0].lds_mode == 0 && c.P.tiles[0].n_kf == 25 && c.P.tiles[0].n_free == 0);
        const int* row = &c.P.tile_row[c.P.tiles[0].kf_off];
        CHECK(row[0] == -1 && row[19] == -1 && row[20] == 6 && row[21] == 12 && row[22] == 18 && row[23] == 24 && row[24] == 30);
    }
    {   // more than 64 key-frames need more than 64 observations: that refusal comes first
        Case c;
        c.add(make_src(65, {0}, {{400.0, 1.0}}, {over(0, 64)}));
        CHECK(c.run() == SADVIO_E_INVALID_ARG && c.err == "set_windows: a landmark has more than 64 observations");
    }
}

static void case_packed_cut() {
    g_case = "5 packed cut";
    // 96 narrow tracks (5 observations over 3 key-frames, newest first) and 5 tracks over key-frames 1 .. 5 between them
    std::vector<Track> tr;
    for (int l = 0; l < 96; l++) {
        if (l == 10 || l == 20 || l == 40 || l == 50) tr.push_back(over(1, 5));
        if (l == 40) tr.push_back(over(1, 5));
        const int k0 = 5 - (l * 5) / 96;
        tr.push_back({{k0, 0}, {k0, 1}, {k0 + 1, 0}, {k0 + 1, 1}, {k0 + 2, 0}});
    }
    Case p, q;
    p.add(make_src(8, {0}, {{400.0, 1.0}, {401.0, 1.0}}, tr));
    q.add(make_src(8, {0}, {{400.0, 1.0}, {401.0, 1.0}}, tr));
    q.in.contig_tiles = true;
    p.run(); check_plan(p);
    q.run(); check_plan(q);
    CHECK(p.P.n_lmk_tot == 101);
    int at = 0;
    for (const Tile& t : p.P.tiles) { CHECK(t.lmk_off == at); at += t.n_lmk; }   // the slices partition tile_lmk (check_plan: every landmark once)
    CHECK(at == 101 && p.P.tile_lmk.size() == 101);
    for (const Tile& t : q.P.tiles) CHECK(t.lmk_off == -1);
    printf("packed cut: %zu tiles, contiguous cut: %zu tiles\n", p.P.tiles.size(), q.P.tiles.size());
    CHECK(p.P.tiles.size() < q.P.tiles.size());
    CHECK(p.P.obs_kf == q.P.obs_kf && p.P.obs_perm == q.P.obs_perm);   // the cut moves no observation
}

static void case_empty_and_batch() {
    g_case = "6 empty window";
    Case e;
    e.add(make_src(3, {0}, {}, {}));
    e.run(); check_plan(e);
    CHECK(e.P.tiles.size() == 1 && e.P.tiles[0].n_lmk == 0 && e.P.tiles[0].first_of_window == 1 && e.P.tiles[0].n_kf == 0);
    CHECK(e.P.tile_kf.size() == 1 && e.P.obs_kf.size() == 1 && e.P.chunk_lm == std::vector<int>({0}) && e.P.wins[0].d.Np == 12);

    g_case = "7 batch";
    Case b;
    b.add(make_src(4, {0}, {{400.0, 1.0}, {400.0, 1.0}}, tracks40(false)));
    b.add(make_src(6, {0, 1}, {{300.0, 1.0}, {301.0, 1.0}, {300.0, 1.0}}, {over(2, 4), {{5, 2}, {3, 1}}}));
    b.run(); check_plan(b);
    const WinDev& d1 = b.P.wins[1].d;
    CHECK(d1.kf_base == 4 && d1.cam_base == 1 && d1.lmk_base == 40 && d1.obs_base == 119 && d1.n_cam == 2 && d1.tile_begin == 2 && d1.tile_end == 3);
    CHECK(b.P.tiles.size() == 3 && b.P.tiles[2].w == 1 && b.P.tiles[2].win_tile0 == 2 && b.P.tiles[2].win_ntiles == 1 && b.P.tiles[0].win_ntiles == 2 && b.P.tiles[2].lmk0 == 40);
    CHECK(b.P.tiles[0].lmk_off == -1);   // a batch keeps the contiguous cut
    CHECK(b.P.obs_kf[119] == 4 + 2 && b.P.obs_kf[122] == 4 + 3 && b.P.obs_cam[122] == 1 + 1 && b.P.obs_cam[123] == 1 + 0 && b.P.obs_perm[122] == 4);
    CHECK(d1.red_off == 18 && d1.Np == 24 && d1.S_off == 768 && b.P.s_tot == 768 + 768 && b.P.max_n_kf == 6 && b.P.max_npose == 24);   // 19 and 25 rows: 2 block rows of 16, 3 tiles of 256 doubles each
    Case m;   // one factor type per batch
    m.add(make_src(3, {0}, {{400.0, 1.0}}, {over(0, 1)}));
    m.add(make_src(3, {0}, {{400.0, 1.0}}, {over(0, 1)}));
    m.wire();
    m.src[1].v.factor_type = SADVIO_FACTOR_ANGULAR;
    CHECK(layout_plan(m.in, m.P, m.err, [](const char*) {}) == SADVIO_E_INVALID_ARG && m.err == "set_windows: all windows of a batch must share one factor_type");
}

static sadvio_sparse_prior sparse_factor(int type, int kf, int l0, int l1 = -1) {
    sadvio_sparse_prior s;
    memset(&s, 0, sizeof(s));
    s.type = type; s.kf = kf; s.lmk0 = l0; s.lmk1 = l1;
    s.delta[0] = 0.1; s.delta[1] = 0.2; s.delta[2] = 0.3; s.sqrt_inf[0] = 2.0;
    return s;
}

static void case_pseudo_observations() {
    g_case = "8 pseudo-observations";
    const std::vector<Track> tr = {over(1, 2), over(1, 3), over(2, 3)};
    Case c;
    c.add(make_src(4, {0}, {{400.0, 1.0}}, tr));
    c.add(make_src(4, {0}, {{400.0, 1.0}}, tr));
    c.wire();
    c.sparse[0] = {sparse_factor(SADVIO_SPARSE_IMU_PRIOR, 1, -1)};
    c.sparse[1] = {sparse_factor(SADVIO_SPARSE_IMU_PRIOR, 1, -1), sparse_factor(SADVIO_SPARSE_POSE_TO_LMK, 3, 1)};   // factor 2 of the batch
    c.run(); check_plan(c);
    const WinDev& d = c.P.wins[1].d;
    CHECK(d.n_obs == 9 && c.P.n_obs_user[1] == 7 && c.P.sp_elim[1] == std::vector<char>({0, 1}) && c.P.sp_elim[0] == std::vector<char>({0}));
    const int o1 = c.P.lmk_oe[d.lmk_base + 1];   // the two entries end landmark 1's list: key-frame 3 is its last
    CHECK(o1 - c.P.lmk_ob[d.lmk_base + 1] == 5);
    CHECK(c.P.obs_cam[o1 - 2] == -1 - (2 * 2 + 0) && c.P.obs_cam[o1 - 1] == -1 - (2 * 2 + 1) && c.P.obs_perm[o1 - 2] == -1 && c.P.obs_perm[o1 - 1] == -1);
    CHECK(c.P.obs_kf[o1 - 1] == d.kf_base + 3 && c.P.obs_meas[2 * (size_t)(o1 - 1)] == 0.0);
    CHECK(c.P.sparse.size() == 3 && c.P.sparse[2].type == 4 && c.P.sparse[2].lmk0 == d.lmk_base + 1 && c.P.sparse[2].kf == d.kf_base + 3 && c.P.sp_list == std::vector<int>({0, 1}));
    CHECK(d.n_red == 0 && c.P.lmk_red[d.lmk_base + 1] == -1 && d.sp_begin == 1 && d.sp_end == 3 && d.spl_begin == 1 && d.spl_end == 2);
    CHECK(c.P.tiles[d.tile_begin].lds_mode == 2 && c.P.gemm_run4);   // a run of three on key-frame 3
    // with a landmark prior on the same landmark it is held in the reduced system: nothing is eliminated
    c.sparse[1].push_back(sparse_factor(SADVIO_SPARSE_LMK_PRIOR, -1, 1));
    c.run(); check_plan(c);
    CHECK(d.n_obs == 7 && c.P.sp_elim[1] == std::vector<char>({0, 0, 0}) && c.P.sp_list == std::vector<int>({0, 1, 2, 3}) && c.P.sparse[2].type == SADVIO_SPARSE_POSE_TO_LMK);
    CHECK(d.n_red == 1 && c.P.lmk_red[d.lmk_base + 1] == 18 && d.Np == 21 && c.P.lmk_const_red[d.lmk_base + 1] == 2 && c.P.has_lmk_const);
    CHECK(d.kept_end - d.kept_begin == 3 && c.P.kept[0] == c.P.lmk_ob[d.lmk_base + 1] && c.P.kept[1] == d.lmk_base + 1 && c.P.kept[2] == 1);
    for (int o = d.obs_base; o < d.obs_base + d.n_obs; o++) CHECK(c.P.obs_cam[o] >= 0);
}

static void case_chunk_tables() {
    g_case = "9 chunk tables";
    const std::vector<Cam> two = {{400.0, 1.0}, {401.0, 1.0}};
    Track t10;
    for (int k = 1; k <= 5; k++) { t10.push_back({k, 0}); t10.push_back({k, 1}); }
    Case c;
    c.add(make_src(6, {0}, two, std::vector<Track>(8, over(1, 5))));    // one chunk
    c.add(make_src(6, {0}, two, std::vector<Track>(32, over(1, 5))));   // 12 + 12 + 8
    c.add(make_src(6, {0}, two, std::vector<Track>(7, t10)));           // 6 + 1: 64 observations per chunk
    c.add(make_src(6, {0}, two, std::vector<Track>(32, over(1, 5))));
    c.in.lm = 1;
    c.run(); check_plan(c);
    CHECK(c.P.tiles.size() == 4 && c.P.want_lm);
    CHECK(c.P.chunk_lm == std::vector<int>({0, 8, 20, 32, 40, 46, 47, 59, 71, 79}));
    CHECK(c.P.chunk_ob == std::vector<int>({0, 40, 100, 160, 200, 260, 270, 330, 390, 430}));
    const int c0[4] = {0, 1, 4, 6}, c1[4] = {1, 4, 6, 9};
    for (int i = 0; i < 4; i++) CHECK(c.P.tiles[i].chunk0 == c0[i] && c.P.tiles[i].chunk1 == c1[i]);
    for (int l = 0; l < 79; l++) {
        const int in_chunk = l < 8 ? l : l < 40 ? (l - 8) % 12 : l < 47 ? (l - 40) % 6 : (l - 47) % 12;
        for (int o = c.P.lmk_ob[l]; o < c.P.lmk_oe[l]; o++) CHECK(c.P.obs_lslot[o] == in_chunk);
    }
    CHECK(c.P.perm == std::vector<int>({1, 3, 2, 0}));   // longest first, equal lengths in tile order
    CHECK(c.P.sub == std::vector<int>({1, 0, 3, 0, 2, 0, 0, 0}) && c.P.lm_n_sub == 4 && c.P.lm_ksub == 1 && c.P.lm_max_cam == 2 && c.P.lm_landmarks == 79);
    CHECK(c.P.lm_sub_obs == 160 && !c.P.lm_ok);   // 32 landmarks x 5 | the 10-observation tile is not on the MFMA path
    c.in.no_lpt = true;
    c.run(); check_plan(c);
    CHECK(c.P.perm == std::vector<int>({0, 1, 2, 3}) && c.P.sub == std::vector<int>({0, 0, 1, 0, 2, 0, 3, 0}));
    Case e;   // 8 landmarks of 8 observations fill a chunk to exactly 64; a ninth with a single observation would be the 65th: it opens the next
    Track t8;
    for (int k = 1; k <= 4; k++) { t8.push_back({k, 0}); t8.push_back({k, 1}); }
    std::vector<Track> tr9(8, t8);
    tr9.push_back({{1, 0}});
    e.add(make_src(5, {0}, two, tr9));
    e.in.lm = 1;
    e.run(); check_plan(e);
    CHECK(e.P.chunk_lm == std::vector<int>({0, 8, 9}) && e.P.chunk_ob == std::vector<int>({0, 64, 65}) && e.P.lm_ok && e.P.lm_sub_obs == 68);   // 65 observations staged, in fours
    for (int o = 0; o < 65; o++) CHECK(e.P.obs_lslot[o] == (o < 64 ? o / 8 : 0));
    Case d;   // every tile on the MFMA path
    d.add(make_src(6, {0}, two, std::vector<Track>(32, over(1, 5))));
    d.in.lm = 1;
    d.run(); check_plan(d);
    CHECK(d.P.lm_ok && d.P.tiles[0].lmk_off == -1 && d.P.chunk_lm == std::vector<int>({0, 12, 24, 32}));
    d.in.lm = 0;
    d.run(); check_plan(d);
    CHECK(!d.P.lm_ok && !d.P.want_lm && d.P.chunk_lm == std::vector<int>({32}) && d.P.tiles[0].lmk_off == 0 && d.P.tiles[0].chunk1 == 0);
}

static void case_reduced_layout() {
    g_case = "10 reduced layout";
    const std::vector<Track> tr = {over(1, 2), over(1, 3), over(2, 3), over(0, 1)};
    {
        Case c;
        c.add(make_src(4, {0}, {{400.0, 1.0}}, tr));
        c.add(make_src(12, {0}, {{400.0, 1.0}}, tr), 1);
        c.add(make_src(13, {0}, {{400.0, 1.0}}, tr), 1);
        c.run(); check_plan(c);
        const WinDev &v = c.P.wins[0].d, &i11 = c.P.wins[1].d, &i12 = c.P.wins[2].d;
        CHECK(v.Np == 18 && v.dpf == 6 && v.ld == 0 && v.S_off == 0);
        CHECK(i11.Np == 165 && i11.dpf == 15 && i11.ld == 0 && i11.S_off == 768 && i11.Npose == 66);      // 19 rows: 3 tiles of 256
        CHECK(i12.Np == 180 && i12.ld == 180 && i12.S_off == 768 + 16896 && c.P.s_tot == 768 + 16896 + 32400);   // 166 rows: 11 block rows, 66 tiles
        CHECK(c.P.max_np == 165 && c.P.n_big == 1 && c.P.np_tot == 18 + 165 + 180 && c.P.red_total == c.P.s_tot + 3 * 363 + 12);
    }
    Case c;
    c.add(make_src(4, {0}, {{400.0, 1.0}, {400.0, 1.0}}, tr, {2}));
    c.wire();
    DensePriorHost& D = c.dprior[0];   // 20 rows; columns: landmark 2 (constant) | key-frame 1 | landmark 0
    D.n_full = 20; D.n = 21; D.kf_keep = 1; D.kf_col = 3; D.lmk_index = {2, 0, 3}; D.lmk_col = {0, 18, -1};
    D.J.assign(20 * 21, 1.0); D.r0.assign(20, 0.5);
    c.run(); check_plan(c);
    const WinDev& d = c.P.wins[0].d;
    CHECK(d.dp_n_full == 20 && d.dp_n == 21 && d.dp_off == 0 && d.dp_int_off == 0 && c.P.dp_ints.size() == 63);
    CHECK(c.P.dp_total == 1360);   // 420 + 420 + 441 + 20 + 21 + 20 + 2 + 3 * 5 = 1359, kept even
    CHECK(c.P.preps.size() == 1 && c.P.preps[0].nf == 20 && c.P.preps[0].n == 21 && c.P.preps[0].w == 0);
    const int *kind = c.P.dp_ints.data(), *index = kind + 21, *col = index + 21;
    for (int a = 0; a < 3; a++) CHECK(kind[a] == 4 && index[a] == 3 * 2 + a && col[a] == -1);              // the constant landmark: no column
    for (int q = 0; q < 6; q++) CHECK(kind[3 + q] == 0 && index[3 + q] == 6 * 1 + q && col[3 + q] == q);   // key-frame 1 = free index 0
    for (int q = 6; q < 15; q++) CHECK(kind[3 + q] == 1 + (q - 6) / 3 && index[3 + q] == 3 * 1 + (q - 6) % 3 && col[3 + q] == -1);   // no IMU states in this window
    for (int a = 0; a < 3; a++) CHECK(kind[18 + a] == 4 && index[18 + a] == a && col[18 + a] == 18 + a);
    CHECK(d.n_red == 1 && d.Np == 21 && c.P.lmk_red[0] == 18 && c.P.lmk_red[2] == -1 && c.P.lmk_const_red[0] == 2 && c.P.lmk_const_red[2] == 1 && c.P.lmk_const[0] == 0);
    CHECK(c.P.n_kept == 2 && c.P.kept == std::vector<int>({0, 0, 0, 1, 0, 0}));
    // landmark-to-landmark factors: each landmark once (0 is kept already, 1 twice, 2 is constant)
    c.sparse[0] = {sparse_factor(SADVIO_SPARSE_LMK_TO_LMK, -1, 0, 1), sparse_factor(SADVIO_SPARSE_LMK_TO_LMK, -1, 1, 3), sparse_factor(SADVIO_SPARSE_LMK_TO_LMK, -1, 3, 2)};
    c.run(); check_plan(c);
    CHECK(d.n_red == 3 && d.Np == 27 && c.P.lmk_red[0] == 18 && c.P.lmk_red[1] == 21 && c.P.lmk_red[3] == 24 && c.P.lmk_red[2] == -1);
    CHECK(c.P.sparse.size() == 3 && c.P.sparse[2].lmk0 == 3 && c.P.sparse[2].lmk1 == 2 && c.P.sp_list == std::vector<int>({0, 1, 2}) && c.P.n_kept == 2 + 3 + 2);
    // two lines, the first constant: 6 columns behind the kept landmarks
    LineSetHost& L = c.lines[0];
    L.id = {7, 8}; L.T.assign(24, 0.0); L.model.assign(12, 1.0); L.is_const = {1, 0}; L.ptr = {0, 1, 3}; L.obs_kf = {1, 2, 3}; L.obs_cam = {1, 0, 1}; L.meas.assign(12, 2.0);
    c.run(); check_plan(c);
    CHECK(d.Np == 33 && c.P.lines.size() == 2 && c.P.lines[0].col == -1 && c.P.lines[1].col == 27 && d.line_end == 2 && d.lobs_end == 3);
    CHECK(c.P.lobs[2].line == 1 && c.P.lobs[2].kf == 3 && c.P.lobs[2].cam == 0 && c.P.tiles[0].Np == 33);   // the two cameras are one
    // a resident prior that is no longer the handle's: refused, and nothing the driver would queue has changed
    c.in.prior_valid = true; c.in.prior_serial = 5; c.in.prior_n_full = 20; c.in.prior_n = 21;
    D.resident = true; D.serial = 5;
    CHECK(layout_reduced_plan(c.in, c.P, c.err) == SADVIO_OK && c.P.wins[0].d.Np == 33);
    c.in.prior_serial = 6;
    c.lines[0] = LineSetHost();   // (what a refused set_lines would have left behind)
    const std::vector<int> lmk_red = c.P.lmk_red, kept = c.P.kept, dp_ints = c.P.dp_ints, sp_list = c.P.sp_list;
    const std::vector<unsigned char> lcr = c.P.lmk_const_red;
    const std::vector<Tile> tiles = c.P.tiles;
    const WinDev d0 = c.P.wins[0].d;
    const size_t n_sparse = c.P.sparse.size(), n_lines = c.P.lines.size(), n_lobs = c.P.lobs.size();
    c.err.clear();
    CHECK(layout_reduced_plan(c.in, c.P, c.err) == SADVIO_E_STATE);
    CHECK(c.err == "the handle's prior changed after set_dense_prior(SADVIO_PRIOR_RESIDENT) attached it to a window: attach it again");
    CHECK(c.P.lmk_red == lmk_red && c.P.kept == kept && c.P.dp_ints == dp_ints && c.P.sp_list == sp_list && c.P.lmk_const_red == lcr);
    CHECK(c.P.sparse.size() == n_sparse && c.P.lines.size() == n_lines && c.P.lobs.size() == n_lobs && c.P.dp_total == 1360 && c.P.np_tot == 33);
    CHECK(!memcmp(&d0, &c.P.wins[0].d, sizeof(WinDev)) && tiles.size() == c.P.tiles.size() && !memcmp(tiles.data(), c.P.tiles.data(), tiles.size() * sizeof(Tile)));
}

static void case_flat_window_checks() {
    g_case = "check_flat_window";
    Case c;
    c.add(make_src(3, {0}, {{400.0, 1.0}}, {over(0, 1), over(1, 2)}));
    c.wire();
    std::string err;
    sadvio_flat_window F = c.src[0].v;
    CHECK(check_flat_window(F, 0, err) == SADVIO_OK);
    F.obs_meas = nullptr;
    CHECK(check_flat_window(F, 2, err) == SADVIO_E_INVALID_ARG && err == "set_windows: missing array in window 2");
    F = c.src[0].v; F.n_obs = 3;
    CHECK(check_flat_window(F, 0, err) == SADVIO_E_INVALID_ARG && err == "set_windows: lmk_obs_ptr is not a CSR over n_obs");
    c.src[0].lmk_obs_ptr = {0, 5, 4}; c.wire();
    CHECK(check_flat_window(c.src[0].v, 0, err) == SADVIO_E_INVALID_ARG && err == "set_windows: CSR not monotone");
    c.src[0].lmk_obs_ptr = {0, 2, 4}; c.src[0].obs_kf[3] = 3; c.wire();
    CHECK(check_flat_window(c.src[0].v, 0, err) == SADVIO_E_INVALID_ARG && err == "set_windows: observation index out of range");
}

int main() {
    case_contiguous_sorted_and_unsorted();
    case_observation_counts();
    case_free_keyframe_limits();
    case_packed_cut();
    case_empty_and_batch();
    case_pseudo_observations();
    case_chunk_tables();
    case_reduced_layout();
    case_flat_window_checks();
    if (g_fail) { printf("%d check(s) FAILED\n", g_fail); return 1; }
    printf("PASSED\n");
    return 0;
}

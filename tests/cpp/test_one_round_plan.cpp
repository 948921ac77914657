// LayoutPlan::single_round (layout_plan.h), the layout's half of the gate of the single-round tile kernels (SolvePlan::one_round): true
// exactly when every tile holds at most 4 waves x (64 / G) landmarks. Hand-derived from the constants of ba_types.h, on the helpers
// of test_layout_plan.cpp (its main is not run). Built as it stands and with -fsanitize=address,undefined (tests/test_one_round_plan_cpu.py).
#define main test_layout_plan_main
#include "test_layout_plan.cpp"
#undef main

static std::vector<Track> tracks_of(int n_lmk, int n_obs, int n_kf) {
    std::vector<Track> t;
    for (int l = 0; l < n_lmk; l++) { Track tr; for (int q = 0; q < n_obs; q++) tr.push_back({(l + q) % n_kf, 0}); t.push_back(tr); }
    return t;
}

int main() {
    const std::vector<Cam> cams = {{450.0, 1.0}};
    {   // one window, 40 landmarks of 4 observations: packed tiles of at most 32 landmarks, one round each
        g_case = "one window";
        Case c; c.add(make_src(6, {0}, cams, tracks_of(40, 4, 6)));
        c.run(); check_plan(c);
        CHECK(c.P.single_round && c.P.tiles.size() >= 2);
        for (const Tile& t : c.P.tiles) CHECK(t.G == 8 && t.n_lmk <= 32);
    }
    {   // the same window with two rounds per tile: one tile of 40 landmarks
        g_case = "two rounds";
        Case c; c.add(make_src(6, {0}, cams, tracks_of(40, 4, 6)));
        c.in.tile_rounds = 2;
        c.run(); check_plan(c, 2);
        CHECK(!c.P.single_round && c.P.tiles.size() == 1 && c.P.tiles[0].n_lmk == 40);
    }
    {   // two rounds allowed, 30 landmarks: the one tile still runs a single round
        g_case = "two rounds allowed, one used";
        Case c; c.add(make_src(6, {0}, cams, tracks_of(30, 4, 6)));
        c.in.tile_rounds = 2;
        c.run(); check_plan(c, 2);
        CHECK(c.P.single_round && c.P.tiles.size() == 1 && c.P.tiles[0].n_lmk == 30);
    }
    {   // a landmark of 9 observations: 16 lanes per landmark, 16 landmarks per round
        g_case = "wide groups";
        Case c; c.add(make_src(12, {0, 1, 2, 3, 4, 5, 6}, cams, tracks_of(20, 9, 12)));
        c.run(); check_plan(c);
        CHECK(c.P.single_round);
        for (const Tile& t : c.P.tiles) CHECK(t.G == 16 && t.n_lmk <= 16);
    }
    {   // a batch of two windows (contiguous cut): single-round by the default of one round per tile
        g_case = "batch";
        Case c; c.add(make_src(6, {0}, cams, tracks_of(40, 4, 6))); c.add(make_src(5, {0}, cams, tracks_of(10, 3, 5)));
        c.run(); check_plan(c);
        CHECK(c.P.single_round && c.P.tiles.size() >= 3);
    }
    {   // a window without landmarks: its one empty tile runs no round at all
        g_case = "no landmarks";
        Case c; c.add(make_src(3, {0}, cams, {}));
        c.run(); check_plan(c);
        CHECK(c.P.single_round && c.P.tiles.size() == 1 && c.P.tiles[0].n_lmk == 0);
    }
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("PASSED\n");
    return 0;
}

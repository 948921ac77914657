// Stand-alone check of sadvio_amd/csrc/covb_long_plan.h (no HIP): the work table of k_covb_long / k_covb_lmk_long for one group of
// three units of sadvio_ba_covariance_batch. Long tracks in the first and in the last unit only, none in the middle one; the last
// unit is window 2 of its batch, whose slice of the long list does not start at 0. Prints OK and exits 0 when every check holds.
#include <cstdio>
#include <vector>

#include "../../sadvio_amd/csrc/covb_long_plan.h"

static int fails = 0;
static void check(bool ok, const char* what) {
    if (!ok) { fails++; std::printf("FAILED: %s\n", what); }
}

int main() {
    constexpr int REC = 6;   // LONG_REC: landmark | window | first entry of kf | key-frames | first entry of slot | observations
    // the batch's long list: window 0 owns tracks 0, 1; window 1 none; window 2 tracks 2, 3, 4 (long_begin = 2 > 0)
    const int n_kf[5] = {66, 300, 70, 512, 65};
    std::vector<int> rec;
    for (int i = 0; i < 5; i++) {
        const int r[REC] = {100 + i, i < 2 ? 0 : 2, 1000 * i, n_kf[i], 5000 * i, 2 * n_kf[i]};
        rec.insert(rec.end(), r, r + REC);
    }
    {   // the group [window 0, window 1, window 2]
        const int lb[3] = {0, 2, 2}, le[3] = {2, 2, 5};
        sadvio::CovbLongPlan P;
        sadvio::covb_long_plan(3, lb, le, rec.data(), REC, P);
        const int want[5][2] = {{0, 0}, {0, 1}, {2, 2}, {2, 3}, {2, 4}};
        check(P.n_rows() == 5 && (int)P.rows.size() == 5 * sadvio::COVB_LONG_ROW, "five rows of two ints");
        for (int r = 0; r < 5 && r < P.n_rows(); r++)
            check(P.rows[2 * r] == want[r][0] && P.rows[2 * r + 1] == want[r][1], "a row names its unit inside the group and its index on the long list");
        for (int r = 1; r < P.n_rows(); r++)
            check(P.rows[2 * r] > P.rows[2 * r - 2] || (P.rows[2 * r] == P.rows[2 * r - 2] && P.rows[2 * r + 1] > P.rows[2 * r - 1]), "units ascending, tracks ascending");
        for (int r = 0; r < P.n_rows(); r++) check(P.rows[2 * r] != 1, "the unit without long tracks has no row");
        check(P.max_kf == 512, "the LDS is sized by the largest n_kf of the table");
    }
    {   // the same units in another call: [window 2, window 0]; the table follows the units, the LDS the tracks named
        const int lb[2] = {2, 0}, le[2] = {5, 1};
        sadvio::CovbLongPlan P;
        sadvio::covb_long_plan(2, lb, le, rec.data(), REC, P);
        const int want[4][2] = {{0, 2}, {0, 3}, {0, 4}, {1, 0}};
        check(P.n_rows() == 4, "four rows");
        for (int r = 0; r < 4 && r < P.n_rows(); r++) check(P.rows[2 * r] == want[r][0] && P.rows[2 * r + 1] == want[r][1], "rows of the second call");
        check(P.max_kf == 512, "largest n_kf, second call");
    }
    {   // window 0 alone: track 3's 512 key-frames are not in the table; a plan object is reused
        const int lb[1] = {0}, le[1] = {2};
        sadvio::CovbLongPlan P;
        P.rows.assign(8, 9); P.max_kf = 77;
        sadvio::covb_long_plan(1, lb, le, rec.data(), REC, P);
        check(P.n_rows() == 2 && P.max_kf == 300, "a reused plan is rebuilt; max_kf is the table's own");
        const int none_b[2] = {2, 2}, none_e[2] = {2, 2};
        sadvio::covb_long_plan(2, none_b, none_e, rec.data(), REC, P);
        check(P.n_rows() == 0 && P.max_kf == 0, "no long track: an empty table");
    }
    if (fails) { std::printf("FAILED (%d)\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}

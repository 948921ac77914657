// covb_long_plan.h — the work table of k_covb_long / k_covb_lmk_long (cov_batch_kernels.h): the long tracks of one group of units of
// sadvio_ba_covariance_batch (cov_batch_driver.h: covb_assemble builds it and uploads it with the unit table). Host only, no HIP:
// tests/cpp/test_covb_long_plan.cpp compiles it on its own.
#pragma once
#include <vector>

namespace sadvio {

constexpr int COVB_LONG_ROW = 2;   // ints of a row: unit inside the group | index on the batch's long list

struct CovbLongPlan {
    std::vector<int> rows;   // [n_rows][COVB_LONG_ROW], units ascending, a unit's tracks ascending: one workgroup per row
    int max_kf = 0;          // most distinct key-frames observing one track of the table: sizes the dynamic LDS (cov_long_lds_bytes)
    int n_rows() const { return (int)rows.size() / COVB_LONG_ROW; }
};

// n_unit units; unit u's window owns the tracks long_begin[u] .. long_end[u] - 1 of the long list (HostWin::long_begin / long_end).
//   long_rec, rec_ints   the list's records (LayoutPlan::long_rec, LONG_REC ints each); field 3 of a record: its distinct key-frames
// The order of the rows is fixed by the units and the list alone, so a track's workgroup never depends on what else the call asked for.
inline void covb_long_plan(int n_unit, const int* long_begin, const int* long_end, const int* long_rec, int rec_ints, CovbLongPlan& out) {
    out.rows.clear();
    out.max_kf = 0;
    for (int u = 0; u < n_unit; u++)
        for (int i = long_begin[u]; i < long_end[u]; i++) {
            out.rows.push_back(u);
            out.rows.push_back(i);
            const int n_kf = long_rec[(size_t)rec_ints * i + 3];
            if (n_kf > out.max_kf) out.max_kf = n_kf;
        }
}

}  // namespace sadvio

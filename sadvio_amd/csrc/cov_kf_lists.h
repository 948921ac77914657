// cov_kf_lists.h — the key-frame -> landmark lists of the square-root covariance assembly (cov_driver.h: cov_assemble;
// cov_kernels.h: k_cov_schur_sqrt walks them). Host only, no HIP: tests/cpp/test_cov_kf_lists.cpp compiles it on its own.
#pragma once
#include <vector>

namespace sadvio {

// CSR over the free key-frames of one window: ptr [n_free_kf + 1], lst the window indices of the landmarks with at least one
// observation (pseudo-observations included: they are rows of the landmark's Jacobian) in the key-frame, each once, ascending.
//   lmk_ob / lmk_oe   observation range of the window's landmark l at [l] (the caller passes the plan's arrays at lmk_base)
//   obs_kf            key-frame of every observation, the index kf_fidx takes
//   kf_fidx           free index of a key-frame inside its window, -1: constant
// An observation whose key-frame is constant or whose free index is outside [0, n_free_kf) is skipped.
inline void cov_kf_lmk_lists(int n_free_kf, int n_lmk, const int* lmk_ob, const int* lmk_oe, const int* obs_kf, const int* kf_fidx,
                             std::vector<int>& ptr, std::vector<int>& lst) {
    const int nf = n_free_kf > 0 ? n_free_kf : 0;
    ptr.assign((size_t)nf + 1, 0);
    std::vector<int> last((size_t)nf, -1);
    auto visit = [&](bool fill) {
        for (int l = 0; l < n_lmk; l++)
            for (int o = lmk_ob[l]; o < lmk_oe[l]; o++) {
                const int f = kf_fidx[obs_kf[o]];
                if (f < 0 || f >= nf || last[f] == l) continue;
                last[f] = l;
                if (fill) lst[ptr[f]++] = l; else ptr[f + 1]++;
            }
    };
    visit(false);
    for (int f = 0; f < nf; f++) ptr[f + 1] += ptr[f];
    lst.assign((size_t)(ptr[nf] > 0 ? ptr[nf] : 1), 0);
    last.assign((size_t)nf, -1);
    visit(true);
    for (int f = nf; f > 0; f--) ptr[f] = ptr[f - 1];   // the fill advanced every start to its end
    ptr[0] = 0;
}

}  // namespace sadvio

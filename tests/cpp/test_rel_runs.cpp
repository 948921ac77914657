// Stand-alone check of sadvio_amd/csrc/rel_runs.h (no HIP): on observation ranges sorted by key-frame, visiting the two runs that
// rel_runs returns must visit exactly the positions the linear walk of the relative marginalisations stops at (key-frame == ga or
// == gb), in the walk's order. Built a second time with -DPLANT_SHORT_RUN (the helper's upper bound drops the last observation of a
// run) the comparison must fail: the program then prints MISMATCH and exits 1. Prints OK and exits 0 otherwise.
#include <cstdio>
#include <vector>

#include "../../sadvio_amd/csrc/rel_runs.h"

using sadvio::RelRuns;
using sadvio::rel_runs;

static int n_cases = 0, n_bad = 0;

static void compare(const std::vector<int>& kf, int ob, int oe, int ga, int gb, const char* what) {
    std::vector<int> walk, runs;
    for (int o = ob; o < oe; o++)
        if (kf[o] == ga || kf[o] == gb) walk.push_back(o);
    const RelRuns R = rel_runs(kf.data(), ob, oe, ga, gb);
    for (int r = 0; r < 2; r++)
        for (int o = R.lo[r]; o < R.hi[r]; o++) runs.push_back(o);
    bool in_range = true;
    for (int r = 0; r < 2; r++) in_range = in_range && ob <= R.lo[r] && R.lo[r] <= R.hi[r] && R.hi[r] <= oe;
    in_range = in_range && R.hi[0] <= R.lo[1];
    n_cases++;
    if (walk != runs || !in_range) {
        n_bad++;
        if (n_bad <= 5) std::printf("MISMATCH %s: range [%d, %d) ga %d gb %d: walk visits %zu, runs visit %zu\n", what, ob, oe, ga, gb, walk.size(), runs.size());
    }
}

// a range of `len` observations at offset `pad` of a larger array (the neighbours' key-frames around it must not be read as its own):
// key-frame k contributes run_of(k) observations, key-frames first_kf, first_kf + step, ...
template <class RunOf>
static std::vector<int> make(int pad, int len, int first_kf, int step, RunOf run_of, int& ob, int& oe) {
    std::vector<int> kf(pad, first_kf);   // a neighbour landmark seen from the same key-frames
    ob = pad;
    for (int k = first_kf; (int)kf.size() - pad < len; k += step)
        for (int r = 0; r < run_of(k) && (int)kf.size() - pad < len; r++) kf.push_back(k);
    oe = (int)kf.size();
    for (int i = 0; i < pad; i++) kf.push_back(kf[oe - 1]);
    return kf;
}

int main() {
    const int lens[] = {65, 66, 129, 4096};
    for (int len : lens) {
        for (int run : {1, 2}) {
            int ob, oe;
            const std::vector<int> kf = make(7, len, 10, 3, [&](int) { return run; }, ob, oe);
            const int first = kf[ob], last = kf[oe - 1], mid = kf[ob + len / 2];
            const int absent_in = first + 1, below = first - 1, above = last + 1;   // (step 3: first + 1 is no key-frame of the range)
            const int cand[] = {first, last, mid, absent_in, below, above};
            for (int ga : cand)
                for (int gb : cand)
                    if (ga != gb) compare(kf, ob, oe, ga, gb, "regular");   // every (ga, gb), gb < ga included; one or both absent
        }
        {   // runs of 64 equal key-frames, at the start, inside and at the end; 1 and 2 elsewhere
            int ob, oe;
            for (int heavy : {0, 1, 2}) {
                const std::vector<int> kf = make(5, len, 100, 1, [&](int k) {
                    const int at = heavy == 0 ? 100 : (heavy == 1 ? 100 + 3 : -1);
                    return k == at ? 64 : 1 + (k & 1);
                }, ob, oe);
                std::vector<int> k2 = kf;
                if (heavy == 2) {   // the last 64 observations of the range: one key-frame
                    const int lastk = k2[oe - 1] + 1;
                    for (int o = oe - 64; o < oe; o++) k2[o] = lastk;
                    for (size_t o = oe; o < k2.size(); o++) k2[o] = lastk;
                }
                const int first = k2[ob], last = k2[oe - 1], heavy_kf = heavy == 0 ? first : (heavy == 1 ? 103 : last);
                const int cand[] = {first, last, heavy_kf, k2[ob + len / 2], first - 1, last + 1};
                for (int ga : cand)
                    for (int gb : cand)
                        if (ga != gb) compare(k2, ob, oe, ga, gb, "run of 64");
            }
        }
        {   // a range that consists of one key-frame only
            std::vector<int> kf(len + 6, 42);
            for (int i = 0; i < 3; i++) { kf[i] = 41; kf[len + 3 + i] = 43; }
            for (int gb : {41, 43, 7}) { compare(kf, 3, 3 + len, 42, gb, "one key-frame"); compare(kf, 3, 3 + len, gb, 42, "one key-frame"); }
            compare(kf, 3, 3 + len, 41, 43, "one key-frame, both absent");
        }
    }
    std::printf("%d cases, %d mismatches\n", n_cases, n_bad);
    if (n_bad) return 1;
    std::printf("OK\n");
    return 0;
}

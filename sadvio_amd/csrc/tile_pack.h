// Tiles as landmark lists: which landmarks of one window share a tile when every tile runs a single round (host only).
#pragma once
#include <algorithm>
#include <vector>

// The contiguous cut ends a tile at every landmark whose key-frames would push the tile past the MFMA limit (gemm_free free
// key-frames). A few outlier tracks in a run of narrow ones then cost two extra tiles each, and a single window sits right at the
// chip's CU count: one tile more than CUs makes two workgroups share a CU. Here such a landmark is SET ASIDE instead (at most
// TILE_PACK_ASIDE per tile, and only when the landmark behind it still fits), the run goes on, and the set-aside landmarks are placed
// afterwards: into a tile with a free slot whose key-frame list already covers them, else into tiles of their own, cut greedily in
// the order of their first key-frame. Everything a tile derives from its members (key-frame list, G, kmax, the lds_mode rule) is
// computed by the caller from the lists as it was from the ranges; the hard limits and the lone over-wide landmark are unchanged.
constexpr int TILE_PACK_ASIDE = 4;

struct TilePackIn {
    int n_lmk, n_kf;
    const int* obs_ptr;        // [n_lmk + 1]
    const int* obs_kf;         // window-local key-frame of every observation
    const unsigned char* kf_const; // may be null
    const int* run_max;        // [n_lmk] longest same-key-frame run of a landmark
    int lanes;                 // lanes of a workgroup: a tile holds lanes / G landmarks
    int max_kf, max_free, gemm_free;
};

// order: every landmark of the window once, tile after tile; cut: end position (in order) of every tile
inline void tile_pack(const TilePackIn& in, std::vector<int>& order, std::vector<int>& cut) {
    order.clear(); cut.clear();
    struct Open { std::vector<int> kfs; int begin = 0, n = 0, nfree = 0, G = 8, run = 0, aside = 0; bool hard = false; };
    std::vector<int> mark(in.n_kf, -1);   // tile (by its index in cut) that lists the key-frame
    std::vector<int> aside;
    std::vector<Open> done;               // per finished tile: what placing a set-aside landmark needs
    auto is_free = [&](int kf) { return !(in.kf_const && in.kf_const[kf]); };
    auto lanes_of = [&](int l, int G) { while (G < in.obs_ptr[l + 1] - in.obs_ptr[l]) G <<= 1; return G; };
    // would landmark l join tile t (index ti)? 1: yes, 0: no. add_kf / add_free: what it would add
    auto probe = [&](const Open& t, int ti, int l, int& G, int& add_kf, int& add_free) {
        G = lanes_of(l, t.G);
        add_kf = add_free = 0;
        if (t.n + 1 > in.lanes / G && t.n > 0) return false;
        for (int o = in.obs_ptr[l]; o < in.obs_ptr[l + 1]; o++) {
            const int kf = in.obs_kf[o];
            bool seen = mark[kf] == ti;
            for (int p = in.obs_ptr[l]; p < o && !seen; p++) seen = in.obs_kf[p] == kf;
            if (!seen) { add_kf++; add_free += is_free(kf); }
        }
        const bool fits_hard = (int)t.kfs.size() + add_kf <= in.max_kf && t.nfree + add_free <= in.max_free;
        return t.n == 0 || (fits_hard && t.nfree + add_free <= in.gemm_free);
    };
    auto admit = [&](Open& t, int ti, int l, int G) {
        for (int o = in.obs_ptr[l]; o < in.obs_ptr[l + 1]; o++) {
            const int kf = in.obs_kf[o];
            if (mark[kf] != ti) { mark[kf] = ti; t.kfs.push_back(kf); t.nfree += is_free(kf); }
        }
        t.G = G; t.n++; t.run = std::max(t.run, in.run_max[l]);
        t.hard = (int)t.kfs.size() > in.max_kf || t.nfree > in.max_free;   // a lone over-wide landmark: the tile ends with it
        order.push_back(l);
    };
    // greedy cut over seq; may_set_aside: the first pass
    auto run_cut = [&](const std::vector<int>* seq, int n, bool may_set_aside) {
        int i = 0;
        while (i < n) {
            Open t; t.begin = (int)order.size();
            const int ti = (int)done.size();
            while (i < n) {
                const int l = seq ? (*seq)[i] : i;
                int G, ak, af;
                if (probe(t, ti, l, G, ak, af)) { admit(t, ti, l, G); i++; if (t.hard) break; continue; }
                // does not fit: set it aside when that keeps the run going, else the tile ends here
                int G2, ak2, af2;
                const bool cap_cut = t.n + 1 > in.lanes / G;
                if (may_set_aside && !cap_cut && t.aside < TILE_PACK_ASIDE && i + 1 < n && probe(t, ti, seq ? (*seq)[i + 1] : i + 1, G2, ak2, af2)) {
                    aside.push_back(l); t.aside++; i++;
                    continue;
                }
                break;
            }
            done.push_back(std::move(t));
        }
    };
    run_cut(nullptr, in.n_lmk, true);
    // set-aside landmarks: a free slot in a tile that already lists their key-frames (G, run length and so the tile's mode unchanged)
    std::vector<std::vector<int>> extra(done.size());
    std::vector<int> rest;
    for (int l : aside) {
        int home = -1;
        for (int ti = 0; ti < (int)done.size() && home < 0; ti++) {
            const Open& t = done[ti];
            if (t.hard || lanes_of(l, t.G) != t.G || t.n + (int)extra[ti].size() + 1 > in.lanes / t.G || in.run_max[l] > t.run) continue;
            bool covered = true;
            for (int o = in.obs_ptr[l]; o < in.obs_ptr[l + 1] && covered; o++) covered = mark[in.obs_kf[o]] == ti || std::find(t.kfs.begin(), t.kfs.end(), in.obs_kf[o]) != t.kfs.end();
            if (covered) home = ti;
        }
        if (home >= 0) extra[home].push_back(l); else rest.push_back(l);
    }
    // tiles in the order they were cut, each with the landmarks placed into it
    std::vector<int> first_pass;
    first_pass.swap(order);
    for (size_t ti = 0; ti < done.size(); ti++) {
        order.insert(order.end(), first_pass.begin() + done[ti].begin, first_pass.begin() + done[ti].begin + done[ti].n);
        order.insert(order.end(), extra[ti].begin(), extra[ti].end());
        cut.push_back((int)order.size());
    }
    // the rest: tiles of their own, by first key-frame (observations are key-frame sorted)
    std::stable_sort(rest.begin(), rest.end(), [&](int a, int b) {
        const int ka = in.obs_ptr[a + 1] > in.obs_ptr[a] ? in.obs_kf[in.obs_ptr[a]] : -1, kb = in.obs_ptr[b + 1] > in.obs_ptr[b] ? in.obs_kf[in.obs_ptr[b]] : -1;
        return ka < kb; });
    const size_t n_first = done.size();
    run_cut(&rest, (int)rest.size(), false);
    for (size_t ti = n_first; ti < done.size(); ti++) cut.push_back(done[ti].begin + done[ti].n);
}

#!/usr/bin/env python
"""Does a single window's k_build / k_backsub launch end late because two tile workgroups share a CU?

  python scripts/gpu_time_tiles.py solve SEED [SOLVES]   GN-10 solves of make_window(seed=SEED) through one graph; run it under
                                                         rocprofv3 --kernel-trace --stats for the per-kernel times. In a build with
                                                         -DSADVIO_KERNEL_TS and SADVIO_DEBUG=4096 the library prints one line per
                                                         k_build workgroup (start, end, CU) to stderr after every solve.
  python scripts/gpu_time_tiles.py wg LOG                summary of the LAST solve's workgroup lines in LOG (that stderr)
"""
import os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def solve(seed, solves):
    from sadvio_amd import capi, synthetic
    w = synthetic.make_window(seed=seed)
    opts = capi.gn_options(10); opts.max_num_consecutive_invalid_steps = 1000
    be = capi.Backend(device=0, use_graph=True)
    be.set_windows([w])
    for _ in range(3): be.solve(opts)
    t = time.perf_counter()
    for _ in range(solves): s = be.solve(opts)
    dt = (time.perf_counter() - t) / solves
    print(f"seed {seed}: {solves} GN-10 solves, wall/solve {dt * 1e6:.1f} us, final cost {s[0].final_cost!r}", flush=True)
    be.close()


def wg_summary(path):
    pat = re.compile(r"k_build wg (\d+) start (\S+) end (\S+) xcc (\d+) se (\d+) sh (\d+) cu (\d+) simd (\d+)")
    runs, cur = [], None
    for line in open(path):
        m = pat.search(line)
        if not m: continue
        if int(m.group(1)) == 0: cur = []; runs.append(cur)
        cur.append((int(m.group(1)), float(m.group(2)), float(m.group(3)), tuple(int(m.group(i)) for i in (4, 5, 6, 7))))
    if not runs: sys.exit("no workgroup lines in " + path)
    wgs = runs[-1]
    by_cu = {}
    for b, s, e, cu in wgs: by_cu.setdefault(cu, []).append(b)
    shared = {b for v in by_cu.values() if len(v) > 1 for b in v}
    ends = sorted(e for _, _, e, _ in wgs)
    med = ends[len(ends) // 2]
    alone = [e for b, _, e, _ in wgs if b not in shared]
    print(f"{len(wgs)} workgroups on {len(by_cu)} CUs; {sum(len(v) > 1 for v in by_cu.values())} CUs host more than one ({len(shared)} workgroups)")
    print(f"end after workgroup 0's start (us): median {med:.2f}, max {ends[-1]:.2f}; workgroups alone on their CU: max {max(alone):.2f}" if alone else "no workgroup alone on its CU")
    print(f"start (us): max {max(s for _, s, _, _ in wgs):.2f}")
    for cu, v in sorted(by_cu.items()):
        if len(v) > 1:
            print(f"  xcc {cu[0]} se {cu[1]} sh {cu[2]} cu {cu[3]}: " + ", ".join(f"wg {b} [{wgs[b][1]:.2f} .. {wgs[b][2]:.2f}]" for b in v))
    late = sorted(wgs, key=lambda r: -r[2])[:8]
    print("latest 8: " + ", ".join(f"wg {b} {e:.2f}{' (shared CU)' if b in shared else ''}" for b, _, e, _ in late))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "solve": solve(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
    elif len(sys.argv) == 3 and sys.argv[1] == "wg": wg_summary(sys.argv[2])
    else: sys.exit(__doc__)

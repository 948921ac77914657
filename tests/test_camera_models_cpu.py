"""CPU checks behind tests/test_gpu_model_gate.py (sadvio_ba_landmark_chi2_models):
  - the Python restatement of the camera models (tests/camera_models.py) equals include/sadvio_cameras.hpp, the header that
    tests/cpp/test_cameras.cpp already pins to the reference's own vectors;
  - the inputs of the GPU tests are well conditioned for their 1e-9 bar: a 50-digit evaluation agrees with the double one to
    1e-10 in every per-observation term; every fisheye observation sits at least 0.05 rad off the axis, except one at 1e-3 rad
    whose projection has its own bar 64 eps f rmax / theta;
  - at most 2 % of the landmarks lie within 1e-6 of the gate's threshold in the reference alone;
  - the decoys of the window-index test move the answer when the model table is indexed without the window's camera base;
  - sadvio_camera_model has the layout of its ctypes mirror, and the library exports the entry point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_helpers as bh
import camera_models as cm
import model_gate_helpers as mg
from sadvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TOL = 1e-13
MP_TOL = 1e-10
BAND, BAND_SHARE = 1e-6, 0.02          # CHI2_THRESHOLD_BAND of tests/test_gpu_window_index.py
FACTORS = [bh.PIXEL, bh.ANGULAR]


def test_restatement_matches_the_header(tmp_path):
    exe = str(tmp_path / "dump_cameras")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "dump_cameras.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    models, n_p, n_r, worst, kinds = {}, 0, 0, 0.0, set()

    def close(got, want):
        got, want = np.array([float(x) for x in got]), np.array(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
        ok = ~np.isnan(want)
        if not ok.any():
            return 0.0
        assert np.array_equal(np.isinf(got[ok]), np.isinf(want[ok]))
        fin = ok & np.isfinite(want)
        return float(np.abs(got[fin] - want[fin]).max() / max(np.abs(want[fin]).max(), 1e-300)) if fin.any() and np.abs(want[fin]).max() > 0 else float(np.abs(got[fin]).max(initial=0.0))

    for ln in out.splitlines():
        t = ln.split()
        if t[0] == "M":
            v = [float(x) for x in t[3:]]
            models[int(t[1])] = (v[0:4], {"kind": int(t[2]), "width": v[4], "height": v[5], "rmax": v[6], "xi": v[7], "alpha": v[8],
                                          "distortion": int(t[12]), "D": v[10:14]})
            kinds.add(int(t[2]))
        elif t[0] == "P":
            K, m = models[int(t[1])]
            x, y, z, u, v = (float(q) for q in t[2:7])
            gu, gv, ok = cm.project_camera(m, K, [x, y, z])
            assert int(ok) == int(t[7]), ln                                   # verdicts: exactly
            worst = max(worst, close([gu, gv], [u, v]))
            n_p += 1
        else:
            K, m = models[int(t[1])]
            u, v, rx, ry, rz = (float(q) for q in t[2:7])
            worst = max(worst, close(cm.ray_camera(m, K, u, v), [rx, ry, rz]))
            n_r += 1
    print(f"[camera models] {n_p} projections, {n_r} rays, {len(models)} models: worst relative difference to the header {worst:.3e}; bar {HEADER_TOL:.0e}")
    assert kinds == set(range(6)) and n_p >= 100 and n_r >= 40
    assert worst <= HEADER_TOL


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
def gpu_cases():
    """(name, window, models, uv) of every window the GPU tests evaluate."""
    out = []
    for f in FACTORS:
        for rig in mg.RIGS:
            out.append((f"{rig} factor {f}",) + mg.rig_window(rig, f))
        a, b = mg.decoys(f)
        out += [(f"decoy a factor {f}",) + a, (f"decoy b factor {f}",) + b]
    return out


def states(w):
    return [(None, None), mg.fixed_deltas(w)]


def test_gpu_inputs_hold_every_branch_and_stay_off_the_fisheye_axis():
    """Every (kind, verdict) pair the issue lists is present, and theta >= 0.05 on the fisheye cameras outside the role landmarks."""
    seen = set()
    for name, w, models, uv in gpu_cases():
        lmk_of = np.repeat(np.arange(w.n_lmk), np.diff(w.lmk_obs_ptr))
        for pd, ld in states(w):
            for o in range(w.n_obs):
                m = models[w.obs_cam[o]]
                pc = np.array(cm.camera_point(w, o, lmk_of[o], pd, ld))
                u, v, ok = cm.project_camera(m, w.cam_K[w.obs_cam[o]], pc)
                tag = (m["kind"], m["alpha"], m["distortion"])
                depth = 0.01 if m["kind"] in cm.FISHEYE else 0.1
                seen.add(tag + ("valid" if ok else "depth" if pc[2] < depth else "outside",))
                if 0.01 <= pc[2] < 0.1:
                    seen.add(tag + ("z=0.05 passes" if ok else "z=0.05 fails",))
                if m["kind"] in cm.FISHEYE and o not in w.truth["role_obs"]:
                    assert mg._theta(pc) >= mg.MIN_THETA, (name, o)
            if w.truth["near_axis_obs"] is not None and pd is None and models[w.obs_cam[w.truth["near_axis_obs"]]]["kind"] in cm.FISHEYE:
                o = w.truth["near_axis_obs"]
                assert abs(mg._theta(np.array(cm.camera_point(w, o, lmk_of[o]))) - 1e-3) < 1e-5
        assert w.n_lmk == mg.N_LMK or "decoy" in name
        assert set(np.diff(w.lmk_obs_ptr)) == {1, 2, 5}
        assert any((np.diff(w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]) < 0).any() for l in range(w.n_lmk)), "a track out of key-frame order"
    tags = {(k, a, d) for k, a, d, _ in seen}
    assert {t[0] for t in tags} == set(range(6))
    assert {(cm.OMNI, 0.3, 0), (cm.OMNI, 0.7, 1), (cm.DOUBLE_SPHERE, 0.3, 0), (cm.DOUBLE_SPHERE, 0.7, 0)} <= tags
    for t in tags:
        for verdict in ("valid", "depth", "outside"):
            assert t + (verdict,) in seen, (t, verdict)
        assert t + ("z=0.05 passes" if t[0] in cm.FISHEYE else "z=0.05 fails",) in seen, t
        assert t[0] in cm.FISHEYE or t + ("z=0.05 passes",) not in seen, t


def test_gpu_inputs_are_well_conditioned_at_50_digits():
    MP = cm.mp_namespace(50)
    eps = np.finfo(np.float64).eps
    worst, worst_axis, n = (0.0, ""), 0.0, 0
    for name, w, models, uv in gpu_cases():
        near = w.truth["near_axis_obs"]
        lmk_of = np.repeat(np.arange(w.n_lmk), np.diff(w.lmk_obs_ptr))
        for pd, ld in states(w):
            for obs_uv in (uv, None):
                _, inl, t = cm.chi2_gate(w, models, pd, ld, obs_uv, 1.0)
                _, inl50, t50 = cm.chi2_gate(w, models, pd, ld, obs_uv, 1.0, mx=MP)
                assert (inl == inl50).all(), name
                for o in range(w.n_obs):
                    if o == near and pd is None:
                        continue
                    a, b = float(t[o]), float(t50[o])
                    assert (a == 1000.0) == (b == 1000.0), (name, o)
                    d = abs(a - b) / max(1.0, abs(b))
                    worst = max(worst, (d, f"{name} observation {o}"))
                    n += 1
        if near is not None and models[w.obs_cam[near]]["kind"] in cm.FISHEYE:    # its own bar, on the projection
            m, K = models[w.obs_cam[near]], w.cam_K[w.obs_cam[near]]
            pc = cm.camera_point(w, near, lmk_of[near])
            u, v, ok = cm.project_camera(m, K, pc)
            u50, v50, ok50 = cm.project_camera(m, K, cm.camera_point(w, near, lmk_of[near], mx=MP), MP)
            bar = 64 * eps * K[0] * m["rmax"] / mg._theta(np.array(pc))
            d = max(abs(float(u50 - u)), abs(float(v50 - v)))
            print(f"[camera models] {name}: near-axis projection differs from 50 digits by {d:.3e} px; bar {bar:.3e} px")
            assert ok and ok50 and d <= bar
            worst_axis = max(worst_axis, d / bar)
    print(f"[camera models] {n} per-observation terms: worst |double - 50 digits| / max(1, |term|) = {worst[0]:.3e} ({worst[1]}); bar {MP_TOL:.0e}")
    assert worst[0] <= MP_TOL and worst_axis > 0.0


def test_reference_stays_clear_of_the_threshold():
    for name, w, models, uv in gpu_cases():
        for pd, ld in states(w):
            for obs_uv in (uv, None):
                for sigma in (0.0, 1.0):
                    avg = cm.as_array(cm.chi2_gate(w, models, pd, ld, obs_uv, sigma)[0])
                    share = (np.abs(avg - 2.0) <= BAND).mean()
                    assert share <= BAND_SHARE, (name, share)


@pytest.mark.parametrize("factor", FACTORS)
def test_a_forgotten_camera_base_on_the_model_table_shows(factor):
    """The handle stores the model table per stored camera of the BATCH; the target's camera c is entry cam_base + c. Reading
    entry c instead (the models of decoy a) must change what the gate returns for the target, by far more than the GPU bar."""
    (a, ma, _), (b, mb, _), (t, mt, uv) = mg.decoys(factor) + (mg.target(factor),)
    table = ma + mb + mt
    base = a.n_cam + b.n_cam
    assert a.n_cam != t.n_cam and b.n_cam != t.n_cam and base != t.n_cam
    assert all(table[c]["kind"] != table[base + c]["kind"] for c in range(t.n_cam))
    good = cm.chi2_gate(t, mt, obs_uv=uv, pixel_sigma=1.0, model_of=lambda c: table[base + c])
    plain = cm.chi2_gate(t, mt, obs_uv=uv, pixel_sigma=1.0)
    bad = cm.chi2_gate(t, mt, obs_uv=uv, pixel_sigma=1.0, model_of=lambda c: table[c])
    assert cm.as_array(good[0]).tolist() == cm.as_array(plain[0]).tolist()
    d = np.abs(cm.as_array(bad[2]) - cm.as_array(good[2])) / (1.0 + np.abs(cm.as_array(good[2])))
    print(f"[camera models] factor {factor}: a forgotten cam_base moves {np.mean(d > 1e-6):.0%} of the observation terms, the median by {np.median(d):.2e}")
    assert np.mean(d > 1e-6) > 0.9 and (bad[1] != good[1]).any()


def test_camera_model_struct_layout(tmp_path):
    fields = [f[0] for f in capi.CameraModelC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sadvio_ba.h"\nint main(void) {\n'
                   'printf("size %zu\\n", sizeof(sadvio_camera_model));\n'
                   + "".join(f'printf("{f} %zu\\n", offsetof(sadvio_camera_model, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lay = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert fields == ["kind", "distortion", "width", "height", "rmax", "xi", "alpha", "D"]
    assert C.sizeof(capi.CameraModelC) == int(lay["size"]) == 80
    for f in fields:
        assert getattr(capi.CameraModelC, f).offset == int(lay[f]), f
    hdr = open(os.path.join(ROOT, "include", "sadvio_ba.h")).read()
    for k, name in enumerate(("PINHOLE", "FISHEYE_EQUIDISTANT", "FISHEYE_EQUISOLID", "FISHEYE_STEREOGRAPHIC", "OMNI", "DOUBLE_SPHERE")):
        assert f"#define SADVIO_CAM_{name} {k}\n" in hdr and getattr(capi, "CAM_" + name) == k


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build_hip()
    lib = capi.load_library()
    assert hasattr(lib, "sadvio_ba_landmark_chi2_models")
    assert lib.sadvio_ba_landmark_chi2_models.argtypes[4] == C.POINTER(capi.CameraModelC)

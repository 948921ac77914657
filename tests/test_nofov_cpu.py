"""CPU: the NoFov scale solve's reference (tests/nofov_helpers.py) and its C-ABI mirrors. AngularErrorScaleCam0's Jacobians
against central differences and the 50-digit back end, the vectorised arrowhead LM against twin.lm_solve on the dense problem,
and the ctypes mirrors of sadvio_nofov_problem / sadvio_nofov_result against the C compiler's layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import twin
from sadvio_amd import capi
import nofov_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _factor_args(seed=0):
    pb = H.make_nofov(seed=seed, n_points=200, px_noise=0.3, lmk_noise=0.05)
    T_cam0_w, T_cc0 = H._tables(pb)
    return [(pb["scale_bearing"][l], pb["lmk_p"][l], T_cam0_w, pb["T_cam0_cam0p"], T_cc0[int(pb["scale_cam"][l])])
            for l in range(0, len(pb["lmk_p"]), max(1, len(pb["lmk_p"]) // 12))], pb


def test_scale_factor_jacobians_match_central_differences_and_mp():
    B, M = twin.Backend("f64"), twin.Backend("mp", 50)
    args, _ = _factor_args()
    for (b, p, Tw, Tm, Tc) in args:
        lam, dl = 0.93, np.array([0.01, -0.02, 0.015])
        r, Jlam, Jl = H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, lam, dl)
        h = 1e-6
        num_lam = (H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, lam + h, dl)[0] - H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, lam - h, dl)[0]) / (2 * h)
        num_l = np.stack([(H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, lam, dl + h * e)[0] -
                           H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, lam, dl - h * e)[0]) / (2 * h) for e in np.eye(3)], axis=1)
        assert np.abs(Jlam - num_lam).max() < 1e-7 * max(1.0, np.abs(Jlam).max())
        assert np.abs(Jl - num_l).max() < 1e-7 * max(1.0, np.abs(Jl).max())
        rm, Jlam_m, Jl_m = H.scale_factor(M, b, p, Tw, Tm, Tc, 1.0, M.s(lam), dl)
        assert np.abs(r - M.f(rm)).max() < 1e-14
        assert np.abs(Jlam - M.f(Jlam_m)).max() < 1e-12 and np.abs(Jl - M.f(Jl_m)).max() < 1e-12


def test_scale_factor_weight_is_one_over_sigma_squared():
    B = twin.Backend("f64")
    (b, p, Tw, Tm, Tc), _ = _factor_args()[0][0], None
    r1 = H.scale_factor(B, b, p, Tw, Tm, Tc, 1.0, 0.9, np.zeros(3))[0]
    r2 = H.scale_factor(B, b, p, Tw, Tm, Tc, 2.0, 0.9, np.zeros(3))[0]
    assert np.allclose(r2, r1 / 4.0, rtol=1e-15, atol=0)


def test_residual_is_zero_at_the_ground_truth():
    B = twin.Backend("f64")
    pb = H.make_nofov(seed=3, n_points=300, scale0=1.0, n_extra=2)
    lam = 1.0                                              # T_cam0_cam0p is the truth itself
    T_cam0_w, T_cc0 = H._tables(pb)
    for l in range(len(pb["lmk_p"])):
        r, _, _ = H.scale_factor(B, pb["scale_bearing"][l], pb["lmk_p"][l], T_cam0_w, pb["T_cam0_cam0p"], T_cc0[int(pb["scale_cam"][l])],
                                 1.0, lam, np.zeros(3))
        assert np.abs(r).max() < 1e-12
    A = H.Arrowhead(H.abi(pb))
    assert A.cost(1.0, np.zeros((A.n, 3))) < 1e-20


@pytest.mark.parametrize("seed,kw", [
    (11, dict(px_noise=0.3, lmk_noise=0.03, n_extra=2)),
    (12, dict(px_noise=0.2, n_outliers=6, n_extra=3, info_scale=10.0)),
    (13, dict(lmk_noise=0.05, n_outliers=4, n_extra=2, scale0=0.9)),
])
def test_arrowhead_lm_matches_the_dense_twin(seed, kw):
    pb = H.abi(H.make_nofov(seed=seed, n_points=400, max_lmk=60, **kw))
    assert 30 <= len(pb["lmk_p"]) <= 100
    a = H.arrowhead_lm(pb)
    b = H.twin_solve(pb)
    assert (a["iterations"], a["termination"], a["n_success"], a["n_unsuccess"]) == \
           (b["iterations"], b["termination"], b["n_success"], b["n_unsuccess"])
    assert abs(a["lambda"] - b["lambda"]) < 1e-10
    assert np.abs(a["lmk_delta"] - b["lmk_delta"]).max() < 1e-9
    assert np.isclose(a["initial_cost"], b["initial_cost"], rtol=1e-12)


def test_arrowhead_lm_with_constant_scale_matches_the_dense_twin():
    fx = H.fixture()
    M = fx["T_f_fp"].copy(); M[:3, :3] = np.eye(3)
    pb = H.abi(H.make_nofov(seed=14, n_points=300, max_lmk=50, motion=M, px_noise=0.3, lmk_noise=0.03, n_extra=2, info_scale=10.0))
    a, b = H.arrowhead_lm(pb), H.twin_solve(pb)
    assert a["scale_fixed"] and a["lambda"] == 1.0 and b["lambda"] == 1.0
    assert (a["iterations"], a["termination"], a["n_success"]) == (b["iterations"], b["termination"], b["n_success"])
    assert np.abs(a["lmk_delta"] - b["lmk_delta"]).max() < 1e-9


def test_fix_scale_rule():
    assert H.reference_fix_scale(H.T12(np.eye(4)))
    M = np.eye(4); M[:3, 3] = [0.2, 0, 0]
    assert H.reference_fix_scale(H.T12(M))                 # no rotation
    M[:3, :3] = twin.exp_so3(twin.Backend("f64"), np.array([0.0, 0.06, 0.0]))
    assert not H.reference_fix_scale(H.T12(M))
    M[:3, 3] = [0.005, 0, 0]
    assert H.reference_fix_scale(H.T12(M))                 # no translation


def _c_layout(tmp_path, names):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sadvio_ba.h")).read(), flags=re.S)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sadvio_ba.h"', "int main(void) {"]
    for name in names:
        m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", hdr, flags=re.S)
        assert m, name
        fields = []
        for decl in m.group(1).split(";"):
            decl = re.sub(r"\[[^\]]*\]", "", decl.strip())
            if not decl:
                continue
            parts = decl.split(",")
            fields.append(parts[0].split()[-1].lstrip("*"))
            fields += [e.strip().lstrip("*") for e in parts[1:]]
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    pairs = {"sadvio_nofov_problem": capi.NoFovProblemC, "sadvio_nofov_result": capi.NoFovResultC}
    lay = _c_layout(tmp_path, pairs)
    for name, mirror in pairs.items():
        assert C.sizeof(mirror) == lay[name], name
        c_fields = [k.split(".")[1] for k in lay if k.startswith(name + ".")]
        assert [{"lambda": "lambda_"}.get(f, f) for f in c_fields] == [f[0] for f in mirror._fields_], name
        for f in c_fields:
            assert getattr(mirror, {"lambda": "lambda_"}.get(f, f)).offset == lay[f"{name}.{f}"], (name, f)


def test_nofov_options_are_the_reference_solver_settings():
    o = capi.nofov_options()
    assert o.max_num_iterations == 20 and o.function_tolerance == 1e-3 and o.huber_a == 1.345 ** 0.5


def test_library_exports_nofov_scale():
    import __graft_entry__ as g
    g.build_hip()
    assert hasattr(capi.load_library(), "sadvio_ba_nofov_scale")

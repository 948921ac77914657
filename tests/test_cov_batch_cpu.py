"""CPU side of sadvio_ba_covariance_batch: the float64 yardsticks of the new windows of tests/test_gpu_cov_batch.py, the ctypes
mirror of sadvio_cov_batch_item, and the C++ program on the plain C ABI (compile + link; it runs in tests/test_cpp_covariance_batch.py).

e_ref per window as in tests/test_cov_cpu.py: the largest relative block difference between np.linalg.inv of the full information
matrix and the 50-digit inverse of the same matrix (every key-frame block, one cross pair, every landmark block) at the oracle's
solution. Measured values (recorded, rounded up, in cov_batch_helpers.E_REF):

    w7         9.54e-13  (n = 1230, N_p = 30)        np174  3.27e-12  (n = 1074, N_p = 174)
    w42        3.03e-13  (n = 924,  N_p = 24)        np180  7.09e-12  (n = 1080, N_p = 180)
    w7_angular 1.51e-12  (n = 1230, N_p = 30)

The test asserts that today's measurement lies in (E_REF / 4, E_REF], and that the information matrix of every window is positive
definite (30- and 31-key-frame windows of shorter tracks are not: they would be no parity windows)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cov_batch_helpers as cb
import cov_helpers as ch
from sadvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(cb.WINDOWS))
def test_float64_inverse_against_50_digits(oracle_lib, case):
    build, pair = cb.WINDOWS[case]
    w = build()
    assert cb.n_p(w) == cb.N_P[case]
    sol = oracle_lib.solve(w, capi.reference_options())
    info = ch.Information(w, sol, 0.0)
    assert not info.singular
    lam = np.linalg.eigvalsh(info.H)[0]
    f64 = ch.reference_blocks(info)
    mp, residual = ch.mp_blocks(info, want_residual=True)
    e = ch.worst_block_difference(f64, mp, info, [pair])
    print(f"[cov batch] {case}: n {info.n}, N_p {cb.N_P[case]}, smallest eigenvalue {lam:.3e}, e_ref {e:.3e} (recorded {cb.E_REF[case]:.1e}), "
          f"50-digit residual |H X - I| {residual:.1e}")
    assert lam > 0.0
    assert residual < 1e-40
    assert cb.E_REF[case] / 4 < e <= cb.E_REF[case], (case, e)


def test_recorded_yardsticks_of_the_known_windows_are_kept():
    for k, v in ch.E_REF.items():
        assert cb.E_REF[k] == v
    assert cb.N_P["np174"] <= 176 < cb.N_P["np180"]            # the pair straddles the cap of the in-LDS inverse


def test_cov_batch_item_mirror_matches_the_c_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sadvio_ba.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef struct sadvio_cov_batch_item\s*\{(.*?)\}\s*sadvio_cov_batch_item;", hdr, flags=re.S)
    assert m
    fields = [d.strip().split()[-1].lstrip("*") for d in m.group(1).split(";") if d.strip()]
    assert fields == [f for f, _ in capi.CovBatchItemC._fields_]
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "sadvio_ba.h"', "int main() {",
             'std::printf("sizeof %zu\\n", sizeof(sadvio_cov_batch_item));']
    lines += [f'std::printf("{f} %zu\\n", offsetof(sadvio_cov_batch_item, {f}));' for f in fields]
    lines += [f'std::printf("{name} %d\\n", {name});' for name in ("SADVIO_COV_ROUTE_NONE", "SADVIO_COV_ROUTE_LDS", "SADVIO_COV_ROUTE_DENSE")]
    lines.append("return 0; }")
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lay = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(lay["sizeof"]) == C.sizeof(capi.CovBatchItemC)
    for f in fields:
        assert int(lay[f]) == getattr(capi.CovBatchItemC, f).offset, f
    assert (int(lay["SADVIO_COV_ROUTE_NONE"]), int(lay["SADVIO_COV_ROUTE_LDS"]), int(lay["SADVIO_COV_ROUTE_DENSE"])) == \
        (capi.COV_ROUTE_NONE, capi.COV_ROUTE_LDS, capi.COV_ROUTE_DENSE)
    decl = re.search(r"int sadvio_ba_covariance_batch\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == 3


def test_the_library_exports_the_entry_point_and_the_binding_declares_it():
    lib = capi.load_library()
    assert hasattr(lib, "sadvio_ba_covariance_batch")
    assert lib.sadvio_ba_covariance_batch.argtypes[2] == C.POINTER(capi.CovBatchItemC)


def test_cpp_program_compiles_with_werror_and_links(tmp_path):
    from test_cpp_covariance_batch import build
    assert os.path.exists(build(tmp_path))

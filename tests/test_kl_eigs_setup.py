"""The matrix-free Matern eigensolver without a GPU: the boundary (symbols, header, argument checks that fail before any
device call) and matern_eigs_filtered, the numpy twin of the device algorithm, against the dense host solve.  The cases,
mode counts and their gaps are in tests/kl_eigs_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import kl_eigs_cases as cases

PMC_ERR_INVALID = -1


def test_symbols_are_exported_and_bound():
    from parelagmc_amd import capi
    lib = capi.load_library()
    for name in ("pmc_kl_eigs_opts_default", "pmc_kl_matern_apply", "pmc_kl_matern_eigs"):
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    o = capi.pmc_kl_eigs_opts()
    lib.pmc_kl_eigs_opts_default(C.byref(o))
    assert (o.tol, o.max_iter, o.guard, o.degree, o.seed) == (1e-8, 100, 16, 8, 0)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_with_the_new_structs(tmp_path, compiler, std, ext):
    src = tmp_path / f"use_kl_eigs.{ext}"
    src.write_text("""
#include "pmc.h"
int main(void) {
    pmc_kl_eigs_opts o;
    pmc_kl_eigs_info i;
    o.tol = 1e-8; o.max_iter = 1; o.guard = 16; o.degree = 8; o.seed = 7u;
    i.iterations = i.block_products = i.converged = 0; i.max_residual_rel = i.gap_rel = i.seconds = 0.0;
    int (*apply)(pmc_ctx*, int, int, const double*, const double*, double, int, const double*, double*) = pmc_kl_matern_apply;
    int (*eigs)(pmc_ctx*, int, int, const double*, const double*, double, int, const pmc_kl_eigs_opts*, double*, double*,
                pmc_kl_eigs_info*) = pmc_kl_matern_eigs;
    void (*dflt)(pmc_kl_eigs_opts*) = pmc_kl_eigs_opts_default;
    return (apply && eigs && dflt && o.max_iter + i.converged == 1) ? 0 : 1;
}
""")
    r = subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use_kl_eigs.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _call_eigs(lib, ctx=None, dim=3, n=8, corlen=0.1, nmodes=2, guard=None, x=True, w=True, out=True):
    from parelagmc_amd import capi
    xs = np.random.default_rng(0).random((n, 3))
    ws = np.ones(n)
    ev, V = np.zeros(max(1, nmodes)), np.zeros(n * max(1, nmodes))
    o = capi.pmc_kl_eigs_opts()
    lib.pmc_kl_eigs_opts_default(C.byref(o))
    if guard is not None:
        o.guard = guard
    dp = C.POINTER(C.c_double)
    rc = lib.pmc_kl_matern_eigs(ctx, dim, n, xs.ctypes.data_as(dp) if x else None, ws.ctypes.data_as(dp) if w else None,
                                corlen, nmodes, C.byref(o), ev.ctypes.data_as(dp) if out else None,
                                V.ctypes.data_as(dp) if out else None, None)
    return rc, lib.pmc_last_error().decode()


def test_arguments_refused_before_any_device_call():
    """no context exists here (ctx = NULL is itself refused), so every call must fail; the message tells which check did"""
    from parelagmc_amd import capi
    lib = capi.load_library()
    rc, msg = _call_eigs(lib, dim=2)
    assert rc == PMC_ERR_INVALID and "dim == 3" in msg
    rc, msg = _call_eigs(lib, corlen=0.0)
    assert rc == PMC_ERR_INVALID and "corlen" in msg
    rc, msg = _call_eigs(lib, corlen=-1.0)
    assert rc == PMC_ERR_INVALID and "corlen" in msg
    rc, msg = _call_eigs(lib, nmodes=0)
    assert rc == PMC_ERR_INVALID and "nmodes" in msg
    rc, msg = _call_eigs(lib, n=600, nmodes=500, guard=16)
    assert rc == PMC_ERR_INVALID and "512" in msg
    rc, msg = _call_eigs(lib, n=600, nmodes=496, guard=16)          # 512 exactly passes that check and stops at ctx = NULL
    assert rc == PMC_ERR_INVALID and "NULL" in msg
    rc, msg = _call_eigs(lib, out=False)
    assert rc == PMC_ERR_INVALID and "NULL" in msg
    for kw in (dict(x=False), dict(w=False), dict()):
        rc, msg = _call_eigs(lib, **kw)
        assert rc == PMC_ERR_INVALID and "NULL" in msg
    dp = C.POINTER(C.c_double)
    a = np.ones(24)
    rc = lib.pmc_kl_matern_apply(None, 2, 8, a.ctypes.data_as(dp), a.ctypes.data_as(dp), 0.1, 1, a.ctypes.data_as(dp),
                                 a.ctypes.data_as(dp))
    assert rc == PMC_ERR_INVALID and "dim == 3" in lib.pmc_last_error().decode()


@pytest.mark.parametrize("name,corlen,m", cases.CASE_IDS)
def test_filtered_twin_matches_the_dense_solve(name, corlen, m):
    from parelagmc_amd.fe.kl import matern_eigs_filtered
    x, w = cases.points(name)
    lam, V, info = matern_eigs_filtered(x, w, corlen, m, tol=cases.TOL)
    print(info)
    assert info["converged"] == 1 and info["max_residual_rel"] <= cases.TOL
    cases.check_against_dense(name, corlen, m, lam, V, info["gap_rel"])


def test_filtered_twin_with_a_wide_block():
    """m = 120 on hex16 (b = 136): the narrowest of cases.WIDE_CASES; the wider ones run on the device only"""
    from parelagmc_amd.fe.kl import matern_eigs_filtered
    name, corlen, m, guard = cases.WIDE_CASES[0]
    assert (name, corlen, m, guard) == ("hex16", 0.1, 120, 16)
    x, w = cases.points(name)
    lam, V, info = matern_eigs_filtered(x, w, corlen, m, tol=cases.TOL, guard=guard)
    print(info)
    assert info["converged"] == 1 and info["max_residual_rel"] <= cases.TOL
    cases.check_against_dense(name, corlen, m, lam, V, info["gap_rel"])


@pytest.mark.parametrize("name,corlen,nmodes", cases.SMALL_CASES)
def test_filtered_twin_on_small_problems(name, corlen, nmodes):
    """b = n (hex4) and m = n (the others): the block spans the whole space, so the twin stops without a filter step"""
    from parelagmc_amd.fe.kl import matern_eigs_filtered
    x, w = cases.points(name)
    lam, V, info = matern_eigs_filtered(x, w, corlen, nmodes, tol=cases.TOL)
    print(info)
    assert info["converged"] == 1 and info["iterations"] == 0
    cases.check_small_against_dense(name, corlen, nmodes, lam, V)


@pytest.mark.parametrize("opts", [dict(guard=0), dict(degree=1), dict(degree=2)], ids=["guard0", "degree1", "degree2"])
def test_filtered_twin_option_extremes(opts):
    """cube_tet_embed, m = 24 (gap 0.0221), default max_iter = 100.  guard = 0: b == m, so the smallest Ritz value of the
    block is a wanted one; with the filter interval ending there the twin stopped at residual 4.8e-5 after 100 filters."""
    from parelagmc_amd.fe.kl import matern_eigs_filtered
    x, w = cases.points("cube_tet_embed")
    lam, V, info = matern_eigs_filtered(x, w, 0.1, 24, tol=cases.TOL, **opts)
    print(info)
    assert info["converged"] == 1 and info["iterations"] <= 100
    if "guard" in opts:
        assert info["gap_rel"] == 0.0
        cases.check_against_dense("cube_tet_embed", 0.1, 24, lam, V)
    else:
        cases.check_against_dense("cube_tet_embed", 0.1, 24, lam, V, info["gap_rel"])


@pytest.mark.parametrize("n", [1, 33, 1000, 4100])
def test_integer_fixture_through_the_twin(n):
    """cases.integer_clusters fed to matern_apply_blocked returns the int64 product exactly: the fixture is what its
    docstring says, and the twin has the device's conventions (c = 1 where kr < 1e-10, exp underflowing to 0, K_ii = w_i;
    DESIGN section 10)"""
    from parelagmc_amd.fe.kl import matern_apply_blocked
    x, w, cl, s = cases.integer_clusters(n)
    assert np.array_equal(np.sqrt(w), s) and s.min() >= 1 and s.max() <= 8
    assert np.all((x == 0.0) | (x == 1000.0 * cases.INT_CORLEN)) and np.all((x != 0.0).sum(1) <= 1)
    for p in (4, 16, 32, 128):
        if n >= 8 * p:
            assert not np.array_equal(cl[:-p], cl[p:]) and not np.array_equal(s[:-p], s[p:]), f"periodic in {p}"
    if n >= 1000:
        assert np.bincount(cl, minlength=4).min() >= n // 8 and np.bincount(s, minlength=9)[1:].min() >= n // 16
    X = cases.integer_block(n, 129)
    assert np.abs(X).max() <= 3 and (n < 4 or np.unique(X, axis=1).shape[1] == 129)
    ref = cases.integer_product(cl, s, X)
    if n <= 1000:
        K = cases.integer_k(cl, s)
        assert np.array_equal(np.diag(K), (s * s)) and np.array_equal(K @ X, ref)
        assert np.array_equal(cases.dense_k(x, w, cases.INT_CORLEN), K)
    Y = matern_apply_blocked(x, w, cases.INT_CORLEN, X.astype(np.float64))
    assert np.array_equal(Y, ref)


def test_eigensolver_keyword():
    """default stays dense; "filtered" goes through the twin; unknown names and a device solve without ctx are refused"""
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_kl_sampler_problem
    from parelagmc_amd.fe.kl import matern_eigs
    h = build_hierarchy(box_mesh([6, 6, 6], [2, 2, 2], "hex"), 0)
    lam_d, V_d = matern_eigs(h, 0.3, 4)
    lam_e, V_e = matern_eigs(h, 0.3, 4, eigensolver="dense")
    assert np.array_equal(lam_d, lam_e) and np.array_equal(V_d, V_e)
    prob = build_kl_sampler_problem(h, "matern", nmodes=4, corlen=0.3, eigensolver="filtered", tol=1e-12)
    assert np.abs(prob.evals - lam_d).max() <= 1e-11 * lam_d[-1]
    with pytest.raises(ValueError):
        matern_eigs(h, 0.3, 4, eigensolver="lobpcg")
    with pytest.raises(ValueError):
        matern_eigs(h, 0.3, 4, eigensolver="device")

"""Gauss-Newton Hessian-vector products on the device (pmc_darcy_mass_tangent / _gn_hessvec: csrc/darcy_hessian.hip;
pmc_sampler_eval_tangent: csrc/sampler_adjoint.hip; pmc_bayes_logpost_gn_hessvec of the host layer) against their numpy twins
with sparse direct solves (parelagmc_amd/fe/darcy_adjoint.py, parelagmc_amd/fe/sampler_adjoint.py, themselves checked against
central differences in tests/test_darcy_gn_hessian.py).  Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import darcy_gradient_cases as cases
import sampler_adjoint_cases as scases
from conftest import ROOT

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
NOISE = 0.01
# Measured on an MI355X at rel_tol = abs_tol = 1e-12 over every case of this file, relative L2 error against the twins' direct
# solves: hv of pmc_darcy_gn_hessvec at most 1.5e-10 (MEASURED_HV) and dG = J dk at most 1.7e-10 (MEASURED_DG; both on hex
# 8^3 with fp32 storage of the preconditioned vectors, 2.7e-11 with fp64), pmc_sampler_eval_tangent at most 9.7e-12
# (MEASURED_TANGENT; the hybridized handle on hex 8^3; the KL handles 3.5e-16), hv of pmc_bayes_logpost_gn_hessvec at most
# 2.2e-11 (MEASURED_LOGPOST); hv at the default 1e-6 options against the tight result at most 2.1e-4 (MEASURED_LOOSE; two
# solves at rel_tol 1e-6 chained).  The kernel alone stays below 0.18 of its summation bound, the transpose pair below 0.015 of
# the sum of the two bounds.  The bounds are 10 x the measured values (box-to-box differences in where a column stops; the
# rule at the top of tests/test_gpu_darcy_gradient.py), those at 1e-12 never looser than 1e-7.
MEASURED_HV = 1.5e-10
MEASURED_DG = 1.7e-10
MEASURED_TANGENT = 9.7e-12
MEASURED_LOGPOST = 2.2e-11
MEASURED_LOOSE = 2.1e-4
TOL_HV = min(10 * MEASURED_HV, 1e-7)
TOL_DG = min(10 * MEASURED_DG, 1e-7)
TOL_TANGENT = min(10 * MEASURED_TANGENT, 1e-7)
TOL_LOGPOST = min(10 * MEASURED_LOGPOST, 1e-7)
TOL_LOOSE = 10 * MEASURED_LOOSE
# The same figures on the element families of tests/derivative_family_cases.py (triangles, quadrilaterals, agglomerated levels;
# the samplers: the agglomerated levels with unit and non-unit P_s weights, the 2-D hierarchy), measured on an MI355X with the
# *_on_other_families tests and the family cases of test_pde_eval_tangent below; the lines they come from are quoted in those
# docstrings.  One constant per family and quantity, the same rule.  The default-options figure keeps TOL_LOOSE: a comparison
# of the device with itself sets no bound.
MEASURED_HV_FAMILY = {"tri": 6.1e-11, "quad": 2.4e-11, "agg": 8.6e-11}
MEASURED_DG_FAMILY = {"tri": 3.8e-11, "quad": 3.0e-11, "agg": 1.4e-10}
MEASURED_TANGENT_FAMILY = {"tri": 4.0e-13, "agg": 3.2e-12}
MEASURED_LOGPOST_TRI = 5.2e-12
TOL_HV_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_HV_FAMILY.items()}
TOL_DG_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_DG_FAMILY.items()}
TOL_TANGENT_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_TANGENT_FAMILY.items()}
TOL_LOGPOST_TRI = min(10 * MEASURED_LOGPOST_TRI, 1e-7)
PMC_ERR_INVALID = -1


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _widths(bw):
    w, out = 1, []
    while w <= bw:
        out.append(w)
        w *= 2
    return out


# ---- the kernel alone ---------------------------------------------------------------------------------------------------
def _check_mass_tangent(gpu_ctx, dp, level, n_fe_expected, nside_expected, label, same_bits_as=None):
    """every launch width 1, 2, 4, ... BatchWidth and a ragged batch of 11 (8 + 2 + 1); host and device memory.  Every entry
    within the first-order summation bound (nside n_fe + 3) 2^-52 sum |dc| |M_aa'| |x_a'| of a reference summed in extended
    precision (n_fe: the padded width, nside: the largest number of elements of a face); essential rows and p-rows exactly
    +0; column b bitwise the same for every width and split; <lam, t> against <dk, g> of the device's own mass sensitivity
    within the sum of the two bounds; the bytes of a launch as documented with n_fe and nside - the handle derived the
    twin's padded width and side count, and with them the kernel form it launches (two sides and 3, 4 or 6 faces: the
    register forms; anything else: the general form).  same_bits_as: a one-level problem whose handle must return the same
    bits (derivative_family_cases.widened)."""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import darcy_adjoint
    k_divides = dp.k_divides
    L = dp.levels[level]
    n = L.n_u + L.n_p
    ess = L.ess_mask.astype(bool)
    assert ess.any()
    ds = capi.DarcySolver(gpu_ctx, dp)
    other = None if same_bits_as is None else capi.DarcySolver(gpu_ctx, same_bits_as)
    bw = ds.BatchWidth(level)
    rng = np.random.default_rng(59)
    k = np.exp(rng.standard_normal((bw, L.n_p)))
    dk = rng.standard_normal((bw, L.n_p))
    x = rng.standard_normal((bw, n))
    lam = rng.standard_normal((bw, n))
    lam[:, :L.n_u][:, ess] = 0.0
    n_fe = darcy_adjoint.element_matrices(L)[0].shape[1]
    assert n_fe == n_fe_expected
    nside = nside_expected
    ld = lambda a: a.astype(np.longdouble)      # noqa: E731
    for wrt_log in (False, True):
        ref, scale = darcy_adjoint.mass_tangent(L, k, x, dk, k_divides, wrt_log, return_abs=True, dtype=np.longdouble)
        bound = (nside * n_fe + 3) * 2.0 ** -52 * scale
        full = ds.mass_tangent(level, k, x, dk, wrt_log)
        assert full.shape == (bw, n)
        err = np.abs(ld(full) - ref)
        free = np.zeros(n, bool)
        free[:L.n_u] = ~ess
        worst = float(np.max(err[:, free] / bound[:, free]))
        print(f"{label} k_divides={k_divides} wrt_log={wrt_log}: width {bw}, max error / bound {worst:.3f}")
        assert np.all(err <= bound)
        assert np.all(full[:, ~free] == 0.0) and not np.any(np.signbit(full[:, ~free]))
        for w in _widths(bw)[:-1] + [11]:
            part = ds.mass_tangent(level, k[:w], x[:w], dk[:w], wrt_log)
            assert np.array_equal(part, full[:w]), f"width {w}"
        for w in (bw, 11):
            kd, xd, dd = (gpu_ctx.array(a[:w]) for a in (k, x, dk))
            td = gpu_ctx.empty(w * n)
            ds.mass_tangent(level, kd, xd, dd, wrt_log, nbatch=w, t_out=td)
            assert np.array_equal(td.download().reshape(w, n), full[:w])
            for a in (kd, xd, dd, td):
                a.free()
        if other is not None:
            assert other.BatchWidth(0) == bw
            for w in (bw, 11, 1):
                assert np.array_equal(other.mass_tangent(0, k[:w], x[:w], dk[:w], wrt_log), full[:w]), f"width {w}"
        # the transpose pair on the device: <lam, t(dk)> == <dk, g(lam)>
        g = ds.mass_sensitivity(level, k, x, lam, wrt_log)
        g_scale = darcy_adjoint.mass_sensitivity(L, k, x, lam, k_divides, wrt_log, return_abs=True, dtype=np.longdouble)[1]
        g_bound = (n_fe * n_fe + 3) * 2.0 ** -52 * g_scale
        lhs = np.sum(ld(lam) * ld(full), axis=1)
        rhs = np.sum(ld(dk) * ld(g), axis=1)
        slack = np.sum(np.abs(ld(lam)) * bound, axis=1) + np.sum(np.abs(ld(dk)) * g_bound, axis=1)
        print(f"    transpose pair: max defect / bound {float(np.max(np.abs(lhs - rhs) / slack)):.3f}")
        assert np.all(np.abs(lhs - rhs) <= slack)
    # bytes of one launch, as documented
    assert ds.mass_tangent_bytes(level, 16) == L.n_u * nside * (4 + 12 * n_fe) + 16 * (2 * 8 * L.n_p + 2 * 8 * L.n_u)
    ds.close()
    if other is not None:       # derivative_family_cases.widened: one element of 5 faces, three sides on a face
        assert other.mass_tangent_bytes(0, 16) == L.n_u * 3 * (4 + 12 * 5) + 16 * (2 * 8 * L.n_p + 2 * 8 * L.n_u)
        other.close()


@pytest.mark.parametrize("k_divides", [True, False])
@pytest.mark.parametrize("mesh", ["hex4", "hex543", "hex5", "hex8", "tet1"])
def test_mass_tangent_kernel(gpu_ctx, mesh, k_divides):
    """240 faces (hex4), 60 elements and a partial last face slice (hex543), 450 faces = seven full slices and a partial one
    (hex5), hex8, tetrahedra; every launch width 1, 2, 4, ... BatchWidth and a ragged batch of 11 (8 + 2 + 1); host and
    device memory.  Every entry within the first-order summation bound (nside n_fe + 3) 2^-52 sum |dc| |M_aa'| |x_a'| of a
    reference summed in extended precision; essential rows and p-rows exactly zero; column b bitwise the same for every
    width and split; <lam, t> against <dk, g> of the device's own mass sensitivity within the sum of the two bounds."""
    h, dp = cases.problem(mesh, k_divides)
    if mesh == "hex5":
        assert dp.levels[0].n_u == 450
    _check_mass_tangent(gpu_ctx, dp, 0, 4 if mesh == "tet1" else 6, 2, mesh)


FAMILY_KERNEL_CASES = [("tri", 0, 3, 2), ("tri", 1, 3, 2), ("quad", 0, 4, 2), ("agg2", 1, 12, 2), ("agg2s", 2, 22, 5),
                       ("agg3", 1, 15, 2), ("agg3s", 2, 57, 11)]


@pytest.mark.parametrize("case,level,n_fe,nside", FAMILY_KERNEL_CASES)
def test_mass_tangent_kernel_on_other_families(gpu_ctx, case, level, n_fe, nside):
    """The instantiations no older test launches (cases: tests/derivative_family_cases.py, both k_divides spread over them):
    mass_tangent_kernel<NB, 3> on tri (2008 faces = 31 slices + 24; 512 = exactly 8 slices), <NB, 4> on quadrilaterals (136
    faces), the general form <NB, 0> on the agglomerated levels: with two sides on agg2 level 1 (197 faces, 12 to 5 faces
    per element) and agg3 level 1 (1630 faces = 25 slices + 30); with nside > 2 - the sides of Darcy::ensure_gradient that a
    face does not have (selem == -1, their padding columns the face itself) - on agg2s level 2 (29 faces, up to 5 sides, 22
    to 15 faces per element) and agg3s level 2 (234 faces, up to 11 sides, 57 to 10 faces per element).  The padded faces of
    the narrower elements carry weight zero in every side's row.
    The general form against the fixed form: as in test_mass_sensitivity_kernel_on_other_families of
    tests/test_gpu_darcy_gradient.py, through derivative_family_cases.widened (its handle reports 5 faces and three sides
    in its bytes) - bit for bit at every width.
    Seeded faults (each built once into a copy of the library and run on an MI355X, none committed): the a2 loop of the
    general form stopping at nfe - 1 fails all seven cases here (tri and quad in the widened comparison) and the five
    agglomerated cases of test_gn_hessvec_on_other_families; its side loop stopping at min(nside, 2) fails agg2s and agg3s
    here (nside 5 and 11), tri and quad in the widened comparison (three sides) and the agg2s / agg3s cases of
    test_gn_hessvec_on_other_families.  Every older test passes with either fault."""
    import derivative_family_cases as fcases
    dp = fcases.problem(case)
    assert fcases.structure(dp.levels[level])[::2] == (n_fe, nside)
    wide = fcases.widened(case, level) if case in ("tri", "quad") else None
    _check_mass_tangent(gpu_ctx, dp, level, n_fe, nside, f"{case} level {level}", same_bits_as=wide)


# ---- the Hessian action -------------------------------------------------------------------------------------------------
def _twin_hv(dp, level, k, dk, Gobs, wrt_log, cols):
    from parelagmc_amd.fe import darcy_adjoint
    out = {b: darcy_adjoint.gn_hessvec(dp, level, k[b], dk[b], Gobs, NOISE, wrt_log, return_all=True) for b in cols}
    return out                                                                   # b -> (hv, dG, x)


def _check_hessvec_level(gpu_ctx, ds, ds_loose, dp, h, level, rng, worst, Gobs=None, tol_hv=None):
    tol_hv = TOL_HV if tol_hv is None else tol_hv
    L = dp.levels[level]
    n = L.n_u + L.n_p
    Gobs = cases.two_cell_observations(h, level) if Gobs is None else Gobs
    ds.SetObservations(level, Gobs)
    ds_loose.SetObservations(level, Gobs)
    bw = ds.BatchWidth(level)
    for wrt_log in (False, True):
        for nb in ((3, bw + 3) if (level == 0 and not wrt_log) else (3,)):
            k = np.exp(rng.standard_normal((nb, L.n_p)))
            dk = rng.standard_normal((nb, L.n_p))
            hv, dG, x, st_t, st_a = ds.gn_hessvec(level, k, dk, NOISE, wrt_log, want_solution=True, return_stats=True)
            assert hv.shape == (nb, L.n_p) and dG.shape == (nb, 2) and x.shape == (nb, n)
            assert all(t[1] == 1 for t in st_t + st_a), (st_t, st_a)
            cols = range(nb) if nb == 3 else (0, 1, bw - 1, bw, bw + 1, bw + 2)      # every launch of the split call
            ref = _twin_hv(dp, level, k, dk, Gobs, wrt_log, cols)
            for b in cols:
                worst["hv"] = max(worst["hv"], rel(hv[b], ref[b][0]))
                worst["dG"] = max(worst["dG"], rel(dG[b], ref[b][1]))
                assert rel(x[b], ref[b][2]) < 1e-9
            assert np.all(np.sum(dk * hv, axis=1) >= 0.0)
            # the forward solution handed back in: no forward solve, the same bits
            hv2, dG2 = ds.gn_hessvec(level, k, dk, NOISE, wrt_log, x_in=x)
            assert np.array_equal(hv2, hv) and np.array_equal(dG2, dG)
            if nb != 3:
                continue
            # symmetry against a second direction on the same state
            w = rng.standard_normal((nb, L.n_p))
            Hw = ds.gn_hessvec(level, k, w, NOISE, wrt_log, x_in=x)[0]
            for b in range(nb):
                defect = abs(float(w[b] @ hv[b]) - float(dk[b] @ Hw[b]))
                assert defect <= 2 * tol_hv * np.linalg.norm(w[b]) * np.linalg.norm(hv[b])
            # device memory: the same bits, with the solution out and back in
            kd, dd = gpu_ctx.array(k), gpu_ctx.array(dk)
            hd, xd = gpu_ctx.empty(hv.size), gpu_ctx.empty(x.size)
            out = ds.gn_hessvec(level, kd, dd, NOISE, wrt_log, nbatch=nb, hv_out=hd, x_out=xd)
            assert np.array_equal(hd.download().reshape(hv.shape), hv) and np.array_equal(out[1], dG)
            assert np.array_equal(xd.download().reshape(x.shape), x)
            hd2 = gpu_ctx.empty(hv.size)
            ds.gn_hessvec(level, kd, dd, NOISE, wrt_log, x_in=xd, nbatch=nb, hv_out=hd2)
            assert np.array_equal(hd2.download().reshape(hv.shape), hv)
            for a in (kd, dd, hd, xd, hd2):
                a.free()
            # the default 1e-6 options against the tight result
            hl = ds_loose.gn_hessvec(level, k, dk, NOISE, wrt_log)[0]
            worst["loose"] = max(worst["loose"], max(rel(hl[b], hv[b]) for b in range(nb)))


@pytest.mark.parametrize("mesh,k_divides,storage,hybrid", [
    ("hex842", True, "fp32", False),
    ("hex842", False, "fp64", False),
    ("hex842", True, "fp32", True),
    ("tet2", True, "fp64", False),
    ("tet2", False, "fp32", False),
    ("tet2", True, "fp32", True),
])
def test_gn_hessvec_matches_the_direct_solve_twin(gpu_ctx, mesh, k_divides, storage, hybrid):
    """every level of the 8^3 / 4^3 / 2^3 hierarchy and of cube_tet refined twice (a hybridized handle: its two finest levels),
    nonzero essential data, both storages of the preconditioned vectors, both wrt_log, nb = 3 and BatchWidth + 3, host and
    device memory"""
    from parelagmc_amd import capi
    h, dp = cases.problem(mesh, k_divides, n_mc_levels=2 if hybrid else None)
    st = capi.PMC_STORAGE_FP32 if storage == "fp32" else capi.PMC_STORAGE_FP64
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st, **TIGHT), hybrid=hybrid)
    ds_loose = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st), hybrid=hybrid)
    rng = np.random.default_rng(61)
    worst = dict(hv=0.0, dG=0.0, loose=0.0)
    for level in range(dp.n_mc_levels):
        _check_hessvec_level(gpu_ctx, ds, ds_loose, dp, h, level, rng, worst)
    print(f"{mesh} k_divides={k_divides} {storage} hybrid={hybrid}: hv rel. error {worst['hv']:.2e}, dG {worst['dG']:.2e}, "
          f"default options against tight {worst['loose']:.2e}")
    ds.close()
    ds_loose.close()
    assert worst["hv"] < TOL_HV and worst["dG"] < TOL_DG
    assert worst["loose"] < TOL_LOOSE


@pytest.mark.parametrize("case,storage,mg", [("tri", "fp64", 0), ("quad", "fp32", 0), ("agg2", "fp64", 0), ("agg2", "fp32", 1),
                                             ("agg2s", "fp32", 0), ("agg2s", "fp64", 1), ("agg3s", "fp64", 1)])
def test_gn_hessvec_on_other_families(gpu_ctx, case, storage, mg):
    """pmc_darcy_gn_hessvec on EVERY level of the cases of tests/derivative_family_cases.py against the twin's direct
    solves: the tangent right-hand side in its <NB, 3> form (tri), on quadrilaterals, in its general form with two sides
    (levels 1 and 2 of agg2) and with up to 5 / 11 sides (level 2 of agg2s / agg3s), and the mass sensitivity behind the
    adjoint solve.  Two observations with unit weights on the agglomerated levels; nb = 3 and BatchWidth + 3 on the finest
    level; both wrt_log, both storages, both V-cycle modes on the agglomerated levels, both k_divides (the cases' own); host
    and device memory.
    Measured on an MI355X (printed by this test):
        tri k_divides=True fp64 mg_coarsening=0: hv rel. error 6.02e-11, dG 3.80e-11, default options against tight 1.79e-05
        quad k_divides=False fp32 mg_coarsening=0: hv rel. error 2.34e-11, dG 2.93e-11, default options against tight 1.03e-05
        agg2 k_divides=False fp64 mg_coarsening=0: hv rel. error 3.98e-11, dG 4.47e-11, default options against tight 7.29e-05
        agg2 k_divides=False fp32 mg_coarsening=1: hv rel. error 3.22e-11, dG 2.48e-11, default options against tight 1.80e-05
        agg2s k_divides=True fp32 mg_coarsening=0: hv rel. error 8.58e-11, dG 1.33e-10, default options against tight 4.63e-05
        agg2s k_divides=True fp64 mg_coarsening=1: hv rel. error 4.77e-11, dG 4.53e-11, default options against tight 2.02e-05
        agg3s k_divides=False fp64 mg_coarsening=1: hv rel. error 1.22e-11, dG 1.00e-11, default options against tight 2.25e-05"""
    import derivative_family_cases as fcases
    from test_gpu_darcy_gradient import family_solvers
    dp, ds, ds_loose, family = family_solvers(gpu_ctx, case, storage, mg)
    rng = np.random.default_rng(61)
    worst = dict(hv=0.0, dG=0.0, loose=0.0)
    for level in range(dp.n_mc_levels):
        _check_hessvec_level(gpu_ctx, ds, ds_loose, dp, None, level, rng, worst, Gobs=fcases.observations(case, level),
                             tol_hv=TOL_HV_FAMILY[family])
    print(f"{case} k_divides={dp.k_divides} {storage} mg_coarsening={mg}: hv rel. error {worst['hv']:.2e}, dG {worst['dG']:.2e}, "
          f"default options against tight {worst['loose']:.2e}")
    ds.close()
    ds_loose.close()
    assert worst["hv"] < TOL_HV_FAMILY[family] and worst["dG"] < TOL_DG_FAMILY[family]
    assert worst["loose"] < TOL_LOOSE


def test_hessvec_under_graph_replay(gpu_ctx):
    """gradient, Hessian action, gradient, Hessian action with different directions on one handle with captured MINRES
    iterations: a graph of one solve replayed for another right-hand side would show in either"""
    from parelagmc_amd import capi
    h, dp = cases.problem("hex8")
    L = dp.levels[0]
    rng = np.random.default_rng(67)
    k = np.exp(rng.standard_normal((4, L.n_p)))
    v, w = rng.standard_normal((2, 4, L.n_p))
    Gobs = cases.two_cell_observations(h)
    eager = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    graph = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(use_graph=1, check_every=2, **TIGHT))
    for ds in (eager, graph):
        ds.SetObservations(0, Gobs)
    g0 = graph.solve_gradient(0, k)[2]
    hv = graph.gn_hessvec(0, k, v, NOISE)
    g1 = graph.solve_gradient(0, k)[2]
    hw = graph.gn_hessvec(0, k, w, NOISE)
    ge = eager.solve_gradient(0, k)[2]
    hve, hwe = eager.gn_hessvec(0, k, v, NOISE), eager.gn_hessvec(0, k, w, NOISE)
    assert rel(g0, ge) < 1e-9 and rel(g1, ge) < 1e-9
    for got, want in ((hv, hve), (hw, hwe)):
        assert rel(got[0], want[0]) < 1e-9 and rel(got[1], want[1]) < 1e-9
    eager.close()
    graph.close()


# ---- the tangent of Eval ------------------------------------------------------------------------------------------------
def _pde_case(kind, mesh, lognormal):
    """(problem for the handle, problem for the twin, projection name, per-level projections for the twin, l2_ops): the cases
    of tests/test_gpu_sampler_adjoint.py"""
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    if kind in ("agg-unit", "agg-nonunit", "tri"):
        import derivative_family_cases as fcases
        sp = fcases.sampler_problem(kind, lognormal)
        return sp, sp, "none", None, None
    if kind in ("saddle", "hybrid"):
        h = scases.hierarchy(mesh)
        sp = build_sampler_problem(h, corlen=scases.CORLEN, lognormal=lognormal)
        if kind == "saddle":
            return sp, sp, "none", None, None
        return (build_hybrid_sampler_problem(h, corlen=scases.CORLEN, lognormal=lognormal, n_mc_levels=min(2, h.nlevels)), sp,
                "none", None, None)
    if kind.endswith("gather"):
        sp, proj = scases.gather_problem(mesh, lognormal)
        hp = sp if kind == "gather" else build_hybrid_sampler_problem(scases.embedded_hierarchy(mesh), corlen=scases.CORLEN,
                                                                      lognormal=lognormal, embedded=True)
        return hp, sp, "gather", proj, None
    sp, proj, ops = scases.l2_problem(mesh, lognormal)
    hp = sp if kind == "l2" else build_hybrid_sampler_problem(scases.hierarchy(mesh), corlen=scases.CORLEN, lognormal=lognormal)
    return hp, sp, "l2", proj, ops


PDE_CASES = [("saddle", "hex842"), ("saddle", "tet2"), ("hybrid", "hex842"), ("hybrid", "tet2"), ("gather", "ragged"),
             ("l2", "ragged"), ("hybrid-gather", "ragged"), ("hybrid-l2", "ragged"), ("agg-unit", "tet2"), ("agg-nonunit", "tet2"),
             ("tri", "square")]


@pytest.mark.parametrize("kind,mesh", PDE_CASES)
def test_pde_eval_tangent(gpu_ctx, kind, mesh):
    """every (level, xi_level) pair; nb = 3 (launches of 2 + 1) and BatchWidth + 3 on the finest level; the lognormal handle
    with s_out against the twin; bitwise Eval of the same vector on the Gaussian handle, and s_out times that on the lognormal
    one; host and device memory.
    agg-unit / agg-nonunit / tri (tests/derivative_family_cases.py; the pairs (0, 0), (1, 0), (2, 0), (2, 2), on tri (0, 0),
    (1, 0), (1, 1)): the restriction chain of the tangent with 5 to 14 children per parent and weights of 0.5 to 1, and the
    2-D SPDE (g = 50.13).
    Measured on an MI355X (printed by this test):
        agg-unit tet2: eval_tangent rel. error against the twin 2.80e-12
        agg-nonunit tet2: eval_tangent rel. error against the twin 3.16e-12
        tri square: eval_tangent rel. error against the twin 4.00e-13"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import sampler_adjoint
    from test_gpu_sampler_adjoint import _family_of
    family, pairs, tight = _family_of(kind)
    prob, twin_prob, projection, projs, ops = _pde_case(kind, mesh, True)
    gprob = _pde_case(kind, mesh, False)[0]
    logn = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(**tight), projection=projection, l2_ops=ops)
    gauss = capi.PDESampler(gpu_ctx, gprob, capi.solver_opts(**tight), projection=projection, l2_ops=ops)
    rng = np.random.default_rng(71)
    cache = {}
    worst = 0.0
    for level in range(prob.n_mc_levels):
        for xi_level in range(level + 1):
            if pairs is not None and (level, xi_level) not in pairs:
                continue
            widths = (3, logn.BatchWidth(level) + 3) if (level, xi_level) == (0, 0) else (3,)
            for nb in widths:
                xi = rng.standard_normal((nb, logn.xi_size(xi_level)))
                v = rng.standard_normal((nb, logn.xi_size(xi_level)))
                s = logn.Eval(level, xi, xi_level=xi_level)
                t, st = logn.EvalTangent(level, v, s_out=s, xi_level=xi_level, return_stats=True)
                assert t.shape == s.shape and all(q[1] == 1 for q in st), st
                proj = None if projs is None else projs[level]
                cols = range(nb) if nb == 3 else (0, 1, nb - 4, nb - 3, nb - 2, nb - 1)
                for b in cols:
                    ref = sampler_adjoint.eval_tangent(twin_prob, level, xi_level, v[b], s[b], proj, cache)
                    worst = max(worst, rel(t[b], ref))
                lv = gauss.Eval(level, v, xi_level=xi_level)
                assert np.array_equal(gauss.EvalTangent(level, v, xi_level=xi_level), lv)
                assert np.array_equal(logn.EvalTangent(level, v, xi_level=xi_level), lv)      # s_out None: d(log s_out)
                assert np.array_equal(t, s * lv)
                if nb == 3:
                    vd, sd, td = gpu_ctx.array(v), gpu_ctx.array(s), gpu_ctx.empty(t.size)
                    logn.EvalTangent(level, vd, s_out=sd, xi_level=xi_level, ds_out=td, nbatch=nb)
                    assert np.array_equal(td.download().reshape(t.shape), t)
                    for a in (vd, sd, td):
                        a.free()
    print(f"{kind} {mesh}: eval_tangent rel. error against the twin {worst:.2e}")
    for smp in (logn, gauss):
        smp.close()
    assert worst < (TOL_TANGENT if family is None else TOL_TANGENT_FAMILY[family])


@pytest.mark.parametrize("mesh,nm", [("hex16", (3, 3, 3)), ("ragged", (4, 4, 4))])
def test_kl_eval_tangent(gpu_ctx, mesh, nm):
    """KL handles: nb = 3 (the VALU kernel) and 129 (the MFMA kernel, two column groups), every (level, xi_level)"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import sampler_adjoint
    kp = scases.kl_problem(mesh, nm, lognormal=True)
    logn = capi.KLSampler(gpu_ctx, kp)
    gauss = capi.KLSampler(gpu_ctx, scases.kl_problem(mesh, nm))
    rng = np.random.default_rng(73)
    worst = 0.0
    for level in range(kp.n_mc_levels):
        for xi_level in range(level + 1):
            for nb in (3, 129):
                xi = 0.3 * rng.standard_normal((nb, logn.xi_size(xi_level)))
                v = rng.standard_normal((nb, logn.xi_size(xi_level)))
                s = logn.Eval(level, xi, xi_level=xi_level)
                t = logn.EvalTangent(level, v, s_out=s, xi_level=xi_level)
                for b in (0, 1, nb - 1):
                    worst = max(worst, rel(t[b], sampler_adjoint.eval_tangent(kp, level, xi_level, v[b], s[b])))
                lv = gauss.Eval(level, v, xi_level=xi_level)
                assert np.array_equal(gauss.EvalTangent(level, v, xi_level=xi_level), lv)
                assert np.array_equal(t, s * lv)
                vd, sd, td = gpu_ctx.array(v), gpu_ctx.array(s), gpu_ctx.empty(t.size)
                logn.EvalTangent(level, vd, s_out=sd, xi_level=xi_level, ds_out=td, nbatch=nb)
                assert np.array_equal(td.download().reshape(t.shape), t)
                for a in (vd, sd, td):
                    a.free()
    print(f"KL {mesh} {nm}: eval_tangent rel. error against the twin {worst:.2e}")
    logn.close()
    gauss.close()
    assert worst < TOL_TANGENT


# ---- the log-posterior --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bayes_setup(gpu_ctx):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    h, dp = cases.problem("hex842", True)
    sp = build_sampler_problem(h, corlen=scases.CORLEN, lognormal=True, n_mc_levels=2)
    smp = capi.PDESampler(gpu_ctx, sp, capi.solver_opts(**TIGHT))
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    Gobs = [cases.two_cell_observations(h, level) for level in (0, 1)]
    for level in (0, 1):
        ds.SetObservations(level, Gobs[level])
    yield h, dp, sp, smp, ds, Gobs
    ds.close()
    smp.close()


def test_logpost_gn_hessvec_matches_the_twin(gpu_ctx, bayes_setup):
    """BayesianInverseProblem::ApplyGNHessian through pmc_bayes_logpost_gn_hessvec: hex 8^3 / 4^3 / 2^3, a lognormal sampler,
    two observations, both levels and a finer xi, host and device vectors; a reused state reproduces the first call bit for
    bit"""
    from parelagmc_amd import host_api
    from parelagmc_amd.fe import sampler_adjoint
    h, dp, sp, smp, ds, Gobs = bayes_setup
    rng = np.random.default_rng(79)
    cache = {}
    worst = 0.0
    for level, xi_level in ((0, 0), (1, 1), (1, 0)):
        n_xi = sp.levels[xi_level].n_s
        xi = 0.5 * rng.standard_normal((3, n_xi))
        v = rng.standard_normal((3, n_xi))
        hv, state = host_api.bayes_logpost_gn_hessvec(smp, ds, level, xi, v, NOISE, xi_level=xi_level)
        assert np.array_equal(state[0], smp.Eval(level, xi, xi_level=xi_level))
        for b in range(3):
            ref = sampler_adjoint.logpost_gn_hessvec(sp, dp, level, xi[b], v[b], Gobs[level], NOISE, xi_level, cache=cache)
            e = rel(hv[b], ref)
            worst = max(worst, e)
            print(f"H_GN level {level} from xi on level {xi_level} column {b}: rel. error {e:.2e}")
        hv2, _ = host_api.bayes_logpost_gn_hessvec(smp, ds, level, None, v, NOISE, xi_level=xi_level, state=state)
        assert np.array_equal(hv2, hv)
        # device vectors: the same bits, first call and reused state
        n_p, n = dp.levels[level].n_p, dp.levels[level].n_u + dp.levels[level].n_p
        xd, vd, hd = gpu_ctx.array(xi), gpu_ctx.array(v), gpu_ctx.empty(v.size)
        kd, sd = gpu_ctx.empty(3 * n_p), gpu_ctx.empty(3 * n)
        host_api.bayes_logpost_gn_hessvec(smp, ds, level, xd, vd, NOISE, xi_level=xi_level, state=(kd, sd, False), nbatch=3,
                                          hv_out=hd)
        assert np.array_equal(hd.download().reshape(v.shape), hv)
        assert np.array_equal(kd.download().reshape(3, n_p), state[0]) and np.array_equal(sd.download().reshape(3, n), state[1])
        hd2 = gpu_ctx.empty(v.size)
        host_api.bayes_logpost_gn_hessvec(smp, ds, level, None, vd, NOISE, xi_level=xi_level, state=(kd, sd), nbatch=3, hv_out=hd2)
        assert np.array_equal(hd2.download().reshape(v.shape), hv)
        for a in (xd, vd, hd, kd, sd, hd2):
            a.free()
    print(f"H_GN: largest rel. error {worst:.2e}")
    assert worst < TOL_LOGPOST


def test_logpost_gn_hessvec_on_triangles(gpu_ctx):
    """pmc_bayes_logpost_gn_hessvec on the 2-D hierarchy of tests/derivative_family_cases.py (1312 / 328 triangles, lognormal
    sampler at corlen 0.1, two observations): mass_tangent_kernel<NB, 3>, mass_sensitivity_kernel<NB, 3> and the 2-D Eval
    tangent and adjoint in one chain; both levels and a finer xi; a reused state reproduces the first call bit for bit.
    Measured on an MI355X (printed by this test):
        H_GN on triangles: largest rel. error 5.13e-12"""
    import derivative_family_cases as fcases
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import sampler_adjoint
    dp, sp = fcases.problem("tri"), fcases.sampler_problem("tri", True)
    smp = capi.PDESampler(gpu_ctx, sp, capi.solver_opts(**TIGHT))
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    rng = np.random.default_rng(79)
    cache = {}
    worst = 0.0
    for level, xi_level in fcases.level_pairs("tri"):
        Gobs = fcases.observations("tri", level)
        ds.SetObservations(level, Gobs)
        n_xi = sp.levels[xi_level].n_s
        xi = 0.5 * rng.standard_normal((3, n_xi))
        v = rng.standard_normal((3, n_xi))
        hv, state = host_api.bayes_logpost_gn_hessvec(smp, ds, level, xi, v, NOISE, xi_level=xi_level)
        assert np.array_equal(state[0], smp.Eval(level, xi, xi_level=xi_level))
        for b in range(3):
            ref = sampler_adjoint.logpost_gn_hessvec(sp, dp, level, xi[b], v[b], Gobs, NOISE, xi_level, cache=cache)
            worst = max(worst, rel(hv[b], ref))
        hv2, _ = host_api.bayes_logpost_gn_hessvec(smp, ds, level, None, v, NOISE, xi_level=xi_level, state=state)
        assert np.array_equal(hv2, hv)
    print(f"H_GN on triangles: largest rel. error {worst:.2e}")
    ds.close()
    smp.close()
    assert worst < TOL_LOGPOST_TRI


def test_newton_cg_step_through_the_entry(gpu_ctx, bayes_setup):
    """up to ten CG steps on H_GN d = -grad(-log pi) driven from Python, the linearization computed once: every p . H p is
    positive, the quadratic model never increases (the error decreases monotonically in the H_GN norm), and d is a descent
    direction.  With two observations H_GN is the identity plus a matrix of rank two: CG ends after three steps, and the
    loop stops once the residual has dropped by 1e-10 (further steps would divide rounding noise by rounding noise)."""
    from parelagmc_amd import host_api
    h, dp, sp, smp, ds, Gobs = bayes_setup
    rng = np.random.default_rng(83)
    xi = 0.5 * rng.standard_normal((1, sp.levels[0].n_s))
    data = ds.ComputeG(0, np.exp(0.3 * rng.standard_normal((1, dp.levels[0].n_p))))[0][0]
    g = -host_api.bayes_logpost_gradient(smp, ds, 0, xi, data, NOISE)[1]           # gradient of -log pi
    d = np.zeros_like(xi)
    r = -g.copy()
    p = r.copy()
    state = None
    model = [0.0]
    for it in range(10):
        Hp, state = host_api.bayes_logpost_gn_hessvec(smp, ds, 0, xi if state is None else None, p, NOISE, state=state)
        pHp = float(np.sum(p * Hp))
        assert pHp > 0.0, (it, pHp)
        rr = float(np.sum(r * r))
        a = rr / pHp
        d += a * p
        r -= a * Hp
        p = r + (float(np.sum(r * r)) / rr) * p
        model.append(0.5 * float(np.sum(d * g)) - 0.5 * float(np.sum(d * r)))     # 1/2 d.Hd + g.d with H d = -g - r
        assert model[-1] <= model[-2] + 1e-12 * abs(model[-2]), (it, model)
        if np.linalg.norm(r) <= 1e-10 * np.linalg.norm(g):
            break
    assert 2 <= len(model) - 1 <= 10 and model[-1] < model[1] < 0.0
    print(f"CG: model values {model[1]:.4e} ... {model[-1]:.4e}, |r| / |g| {np.linalg.norm(r) / np.linalg.norm(g):.2e}")
    assert float(np.sum(d * g)) < 0.0


def test_host_classes_return_the_c_abi_values(tmp_path, hex_hierarchy_small, seeded_rng):
    """tests/c/gn_hessian_smoke.cpp: PDESampler::EvalTangent, DarcySolver::SolveFwd_GNHessVec and
    BayesianInverseProblem::ApplyGNHessian (host and device vectors, fresh and reused state) and pmc_bayes_logpost_gn_hessvec
    against the chain composed from the C ABI, compared with memcmp"""
    from parelagmc_amd.fe import build_darcy_problem, build_sampler_problem
    from test_abi_binaries import write_problem_file
    r = subprocess.run(["make", "-C", ROOT, "test-gn-hessian"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sp_ = build_sampler_problem(hex_hierarchy_small, corlen=0.1, lognormal=True)
    dp = build_darcy_problem(hex_hierarchy_small, cases.ESS, cases.OBS, cases.INFLOW)
    nb = 3
    xi = 0.5 * seeded_rng.standard_normal((nb, sp_.levels[0].n_s))
    s_expect = [np.zeros((nb, sp_.levels[l].n_s)) for l in range(2)]        # not read here
    k = [np.exp(0.5 * seeded_rng.standard_normal((nb, dp.levels[l].n_p))) for l in range(2)]
    path = str(tmp_path / "problem.bin")
    write_problem_file(path, sp_, dp, xi, s_expect, k, [np.zeros(nb), np.zeros(nb)])
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "gn_hessian_smoke"), path], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("gn_hessian_smoke OK"), r.stdout + r.stderr


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_hessian_calls_refuse_bad_arguments(gpu_ctx):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    h, dp = cases.problem("hex4")
    L = dp.levels[0]
    ds = capi.DarcySolver(gpu_ctx, dp)
    lib = gpu_ctx.lib
    k = np.ones((1, L.n_p))
    x = np.ones((1, L.n_u + L.n_p))
    hv, t = np.empty((1, L.n_p)), np.empty((1, L.n_u + L.n_p))
    pk, px, ph, pt = k.ctypes.data, x.ctypes.data, hv.ctypes.data, t.ctypes.data
    H = capi.PMC_MEM_HOST

    def refused(rc, word):
        assert rc == PMC_ERR_INVALID
        assert word in lib.pmc_last_error().decode(), lib.pmc_last_error().decode()

    def hess(level=0, nb=1, kk=pk, xin=None, dk=pk, noise=NOISE, out=ph, xout=None):
        return lib.pmc_darcy_gn_hessvec(ds.h, level, nb, kk, xin, dk, noise, 0, out, None, xout, H, None, None)

    def tang(level=0, nb=1, kk=pk, xx=px, dk=pk, out=pt):
        return lib.pmc_darcy_mass_tangent(ds.h, level, nb, kk, xx, dk, 0, out, H)

    refused(hess(), "observation")                       # no observation functionals yet
    ds.SetObservations(0, cases.two_cell_observations(h))
    for fn in (hess, tang):
        refused(fn(level=-1), "level")
        refused(fn(level=dp.n_mc_levels), "level")
        refused(fn(nb=0), "nbatch")
        refused(fn(kk=None), "k is NULL")
        refused(fn(dk=None), "dk is NULL")
        refused(fn(out=None), "hv is NULL" if fn is hess else "t_out is NULL")
    refused(tang(xx=None), "x is NULL")
    for noise in (0.0, -1.0):
        refused(hess(noise=noise), "noise")
    refused(hess(xin=px, xout=pt), "x_out")
    assert hess() == 0 and hess(xout=pt) == 0 and hess(xin=pt) == 0 and tang() == 0
    b = C.c_double(0.0)
    refused(lib.pmc_darcy_mass_tangent_bytes(ds.h, dp.n_mc_levels, 16, C.byref(b)), "mass_tangent_bytes")
    ds.close()
    # the tangent of Eval: as the adjoint refuses
    hs = scases.hierarchy("ragged")
    gauss = capi.PDESampler(gpu_ctx, build_sampler_problem(hs, corlen=scases.CORLEN))
    logn = capi.PDESampler(gpu_ctx, build_sampler_problem(hs, corlen=scases.CORLEN, lognormal=True))
    klg = capi.KLSampler(gpu_ctx, scases.kl_problem("ragged"))
    for smp in (gauss, logn, klg):
        n = smp.SampleSize(0)
        v, d = np.ones((1, n)), np.empty((1, n))
        pv, pd = v.ctypes.data, d.ctypes.data
        for level, xi_level, nb, vv, dd, word in ((-1, 0, 1, pv, pd, "level"), (smp.nlevels, 0, 1, pv, pd, "level"),
                                                  (0, -1, 1, pv, pd, "xi_level"), (0, 1, 1, pv, pd, "xi_level"),
                                                  (0, 0, 0, pv, pd, "EvalTangent"), (0, 0, 1, None, pd, "EvalTangent"),
                                                  (0, 0, 1, pv, None, "EvalTangent")):
            refused(lib.pmc_sampler_eval_tangent(smp.h, level, xi_level, nb, vv, None, dd, H, None), word)
        if smp is not logn:
            refused(lib.pmc_sampler_eval_tangent(smp.h, 0, 0, 1, pv, pv, pd, H, None), "s_out")
        assert lib.pmc_sampler_eval_tangent(smp.h, 0, 0, 1, pv, pv if smp is logn else None, pd, H, None) == 0
        assert lib.pmc_sampler_is_lognormal(smp.h) == (1 if smp is logn else 0)      # the flag is back in place
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    n = gauss.SampleSize(0)
    H0 = point_observations(n, pick_observation_elements(hs, 2, 5))
    for smp in (gauss, klg):
        cond = capi.Conditioner(smp, H0, np.array([0.3, -0.2]))
        smp.SetConditioner(cond)
        v, d = np.ones((1, n)), np.empty((1, n))
        refused(lib.pmc_sampler_eval_tangent(smp.h, 0, 0, 1, v.ctypes.data, None, d.ctypes.data, H, None), "conditioner")
        smp.SetConditioner(None)
        assert lib.pmc_sampler_eval_tangent(smp.h, 0, 0, 1, v.ctypes.data, None, d.ctypes.data, H, None) == 0
        cond.close()
    # the prior's part of the Hessian action: hv += v; refusals
    v = np.random.default_rng(89).standard_normal((5, n))
    hv = np.ones((5, n))
    assert lib.pmc_sampler_logprior_hessvec(gauss.h, n, 5, v.ctypes.data, hv.ctypes.data, H) == 0
    assert np.array_equal(hv, 1.0 + v)
    for nn, nb, pv, ph in ((0, 5, v.ctypes.data, hv.ctypes.data), (n, 0, v.ctypes.data, hv.ctypes.data), (n, 5, None, hv.ctypes.data),
                           (n, 5, v.ctypes.data, None)):
        refused(lib.pmc_sampler_logprior_hessvec(gauss.h, nn, nb, pv, ph, H), "logprior_hessvec")
    for smp in (gauss, logn, klg):
        smp.close()

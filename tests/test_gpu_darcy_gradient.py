"""Adjoint gradients of the Darcy solve on the device (pmc_darcy_mass_sensitivity / _solve_gradient / _loglik_gradient,
csrc/darcy_gradient.hip) against their numpy twin with sparse direct solves (parelagmc_amd/fe/darcy_adjoint.py, itself checked
against central differences of the oracle in tests/test_darcy_adjoint.py).  Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import darcy_gradient_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
# Relative L2 error of the device gradient at rel_tol = abs_tol = 1e-12 against the twin's direct-solve gradient, measured on
# an MI355X over every case of this file: at most 2.3e-11 (solve_gradient) and 3.5e-11 (loglik_gradient).  The bounds are
# 10 x the measured values and never looser than 1e-7 (the gradient is bilinear in two fields that the project holds to 1e-9 at
# this tolerance).
TOL_GRAD = min(10 * 2.3e-11, 1e-7)
TOL_LOGLIK = min(10 * 3.5e-11, 1e-7)
# The same two figures on the element families of tests/derivative_family_cases.py (triangles, quadrilaterals, agglomerated
# levels), measured on an MI355X with test_gradients_on_other_families below; the lines they come from are quoted in its
# docstring.  One constant per family and quantity, the same rule.
MEASURED_GRAD_FAMILY = {"tri": 2.7e-11, "quad": 7.0e-12, "agg": 2.6e-11}
MEASURED_LOGLIK_FAMILY = {"tri": 1.9e-11, "quad": 6.9e-12, "agg": 2.1e-11}
TOL_GRAD_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_GRAD_FAMILY.items()}
TOL_LOGLIK_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_LOGLIK_FAMILY.items()}
TIGHT_AGG = dict(TIGHT, max_iter=600)          # the iteration limit of tests/test_gpu_agglomerated.py
PMC_ERR_INVALID = -1


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def _widths(bw):
    w, out = 1, []
    while w <= bw:
        out.append(w)
        w *= 2
    return out


# ---- 4. the kernel alone ------------------------------------------------------------------------------------------------
def _check_mass_sensitivity(gpu_ctx, dp, level, n_fe_expected, label, same_bits_as=None):
    """every launch width 1, 2, 4, ... BatchWidth and a ragged batch of 11 (8 + 2 + 1); host and device memory.  Every entry
    within the first-order summation bound (n_fe^2 + 3) 2^-52 sum |c'| |lam_a M_aa' x_a'| of a reference summed in extended
    precision (n_fe: the padded width); column b bitwise the same for every width and split; the bytes of a launch as
    documented with n_fe - the handle derived the twin's padded width, and with it the kernel form it launches (3, 4, 6:
    the register forms; anything else: the general form).  same_bits_as: a one-level problem whose handle must return the
    same bits (derivative_family_cases.widened).  Returns the full-width results per wrt_log."""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import darcy_adjoint
    k_divides = dp.k_divides
    L = dp.levels[level]
    n = L.n_u + L.n_p
    ds = capi.DarcySolver(gpu_ctx, dp)
    other = None if same_bits_as is None else capi.DarcySolver(gpu_ctx, same_bits_as)
    bw = ds.BatchWidth(level)
    rng = np.random.default_rng(41)
    k = np.exp(rng.standard_normal((bw, L.n_p)))
    x = rng.standard_normal((bw, n))
    lam = rng.standard_normal((bw, n))
    n_fe = darcy_adjoint.element_matrices(L)[0].shape[1]
    assert n_fe == n_fe_expected
    assert ds.mass_sensitivity_bytes(level, 16) == L.n_p * (4 * n_fe + 8 * n_fe * n_fe + 2 * 8 * 16) + 2 * 8 * 16 * L.n_u
    out = {}
    for wrt_log in (False, True):
        ref, scale = darcy_adjoint.mass_sensitivity(L, k, x, lam, k_divides, wrt_log, return_abs=True, dtype=np.longdouble)
        bound = (n_fe * n_fe + 3) * 2.0 ** -52 * scale
        full = ds.mass_sensitivity(level, k, x, lam, wrt_log)
        assert full.shape == (bw, L.n_p)
        err = np.abs(full.astype(np.longdouble) - ref)
        worst = float(np.max(err / bound))
        print(f"{label} k_divides={k_divides} wrt_log={wrt_log}: width {bw}, max error / bound {worst:.3f}")
        assert np.all(err <= bound)
        for w in _widths(bw)[:-1] + [11]:
            part = ds.mass_sensitivity(level, k[:w], x[:w], lam[:w], wrt_log)
            assert np.array_equal(part, full[:w]), f"width {w}"
        # device memory: the full width and the ragged batch
        for w in (bw, 11):
            kd, xd, ld = (gpu_ctx.array(a[:w]) for a in (k, x, lam))
            gd = gpu_ctx.empty(w * L.n_p)
            ds.mass_sensitivity(level, kd, xd, ld, wrt_log, nbatch=w, grad_out=gd)
            assert np.array_equal(gd.download().reshape(w, L.n_p), full[:w])
            for a in (kd, xd, ld, gd):
                a.free()
        if other is not None:
            assert other.BatchWidth(0) == bw
            for w in (bw, 11, 1):
                assert np.array_equal(other.mass_sensitivity(0, k[:w], x[:w], lam[:w], wrt_log), full[:w]), f"width {w}"
        out[wrt_log] = full
    ds.close()
    if other is not None:
        n_w = 5                  # derivative_family_cases.widened: none of the register forms
        assert other.mass_sensitivity_bytes(0, 16) == L.n_p * (4 * n_w + 8 * n_w * n_w + 2 * 8 * 16) + 2 * 8 * 16 * L.n_u
        other.close()
    return out


@pytest.mark.parametrize("k_divides", [True, False])
@pytest.mark.parametrize("mesh", ["hex4", "hex543", "hex5", "hex8", "tet1"])
def test_mass_sensitivity_kernel(gpu_ctx, mesh, k_divides):
    """64 elements (exactly one slice), 60 (ragged), 125 (two slices, the second ragged), 512, 48 tetrahedra; every launch
    width 1, 2, 4, ... BatchWidth and a ragged batch of 11 (8 + 2 + 1); host and device memory.  Every entry within the
    first-order summation bound (n_fe^2 + 3) 2^-52 sum |c'| |lam_a M_aa' x_a'| of a reference summed in extended precision;
    column b bitwise the same for every width and split."""
    h, dp = cases.problem(mesh, k_divides)
    _check_mass_sensitivity(gpu_ctx, dp, 0, 4 if mesh == "tet1" else 6, mesh)


FAMILY_KERNEL_CASES = [("tri", 0, 3, 2), ("tri", 1, 3, 2), ("quad", 0, 4, 2), ("agg2", 1, 12, 2), ("agg2s", 2, 22, 5),
                       ("agg3", 1, 15, 2), ("agg3s", 2, 57, 11)]


@pytest.mark.parametrize("case,level,n_fe,nside", FAMILY_KERNEL_CASES)
def test_mass_sensitivity_kernel_on_other_families(gpu_ctx, case, level, n_fe, nside):
    """The instantiations no older test launches (cases: tests/derivative_family_cases.py, both k_divides spread over them):
    mass_sensitivity_kernel<NB, 3> on tri (1312 elements = 20 slices + 32; 328 = 5 slices + 8), <NB, 4> on quadrilaterals
    (60 elements, one ragged slice), the general form <NB, 0> on the agglomerated levels: agg2 level 1 (41 elements of 12 to
    5 faces), agg2s level 2 (5 elements of 22 to 15 faces: one nearly empty slice), agg3 level 1 (334 elements = 5 slices +
    14, 15 to 4 faces), agg3s level 2 (37 elements of 57 to 10 faces).  On every agglomerated level the elements with fewer
    faces than the widest run through the zero-weight padding of Darcy::ensure_gradient.
    The general form against the fixed form: no entry point selects the form - the launch switches on the face count alone
    - so the test changes the data instead: derivative_family_cases.widened gives one element of tri / quad further faces
    of weight 0.0; that handle reports 5 faces in its bytes (the general form, every other element padded) and has to
    return the bits of the fixed form at every width ("the same order, the same bits" of the kernel's comment).
    Seeded faults (each built once into a copy of the library and run on an MI355X, none committed): the general form
    skipping a == 0 fails all seven cases here (tri and quad in the widened comparison), the five agglomerated cases of
    test_gradients_on_other_families and the four agglomerated cases of test_mass_tangent_kernel_on_other_families (its
    transpose pair); Darcy::ensure_gradient padding with the element's last face at the neighbouring weight instead of
    weight zero fails the same tests and all seven tangent kernel cases.  Every older test passes with either fault."""
    import derivative_family_cases as fcases
    dp = fcases.problem(case)
    assert fcases.structure(dp.levels[level])[::2] == (n_fe, nside)
    wide = fcases.widened(case, level) if case in ("tri", "quad") else None
    _check_mass_sensitivity(gpu_ctx, dp, level, n_fe, f"{case} level {level}", same_bits_as=wide)


# ---- 5. the full gradient -----------------------------------------------------------------------------------------------
def _twin(dp, level, k, adj_rhs, wrt_log):
    from parelagmc_amd.fe import darcy_adjoint
    out = [darcy_adjoint.gradient(dp, level, k[b], None if adj_rhs is None else adj_rhs[b], wrt_log, return_all=True)
           for b in range(k.shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))   # grad, Q, x, lam


def _check_level(ds, ds_loose, dp, level, rng, hybrid, nb=3, tol=None):
    """both right-hand sides and both wrt_log on one level: gradient against the twin, Q bitwise against solve_fwd, the two
    solutions through the operator, the default tolerance against the tight one.  tol: the bound on the gradient's error
    (None: TOL_GRAD).  Returns the largest gradient error."""
    tol = TOL_GRAD if tol is None else tol
    from parelagmc_amd.fe import darcy_adjoint
    L = dp.levels[level]
    n = L.n_u + L.n_p
    ess = np.zeros(n, bool)
    ess[:L.n_u] = L.ess_mask.astype(bool)
    k = np.exp(rng.standard_normal((nb, L.n_p)))
    worst = 0.0
    for adj_rhs in (None, rng.standard_normal((nb, n))):
        for wrt_log in (False, True):
            g_ref, Q_ref, x_ref, lam_ref = _twin(dp, level, k, adj_rhs, wrt_log)
            Q, Cc, g, x, lam, st_f, st_a = ds.solve_gradient(level, k, adj_rhs, wrt_log, want_solution=True, return_stats=True)
            assert all(t[1] == 1 for t in st_f + st_a), (st_f, st_a)
            assert np.all(Cc == n)
            e = max(rel(g[b], g_ref[b]) for b in range(nb))
            worst = max(worst, e)
            assert e < tol, e
            assert rel(x, x_ref) < 1e-9 and rel(lam, lam_ref) < 1e-9
            if wrt_log or adj_rhs is not None:
                continue
            assert np.allclose(Q, Q_ref, rtol=1e-9, atol=0.0)
            if hybrid:          # SolveFwd of a hybridized handle goes through the multiplier system; the gradient does not
                continue
            # Q: bitwise the value of solve_fwd with the solution requested
            Qf, _, xf = ds.SolveFwd(level, k, want_solution=True)
            assert np.array_equal(Q, Qf) and np.array_equal(x, xf)
    # A(k) x = rhs_bc and A(k) lam = adj_rhs (essential rows zero) through the operator, on a launch width (2 columns)
    adj_rhs = rng.standard_normal((nb, n))
    Q, Cc, g, x, lam = ds.solve_gradient(level, k, adj_rhs, want_solution=True)
    rhs_bc = np.stack([darcy_adjoint.assemble(dp, level, k[b])[1] for b in range(2)])
    b_adj = np.where(ess[None, :], 0.0, adj_rhs[:2])
    if not hybrid:              # (pmc_darcy_apply_operator of a hybridized handle is the multiplier operator)
        assert rel(ds.ApplyOperator(level, k[:2], x[:2]), rhs_bc) < 1e-9
        assert rel(ds.ApplyOperator(level, k[:2], lam[:2]), b_adj) < 1e-9
    assert np.all(lam[:, ess] == 0.0)
    # the default 1e-6 rule against the 1e-12 one: the project's QoI figure at that rule
    g_tight = ds.solve_gradient(level, k)[2]
    g_loose = ds_loose.solve_gradient(level, k)[2]
    assert max(rel(g_loose[b], g_tight[b]) for b in range(nb)) < 1e-4
    return worst


@pytest.mark.parametrize("mesh,qoi,k_divides,storage,hybrid", [
    ("hex842", "eff_perm", True, "fp32", False),
    ("hex842", "p_int", True, "fp64", False),
    ("hex842", "p_int", False, "fp32", False),
    ("hex842", "eff_perm", False, "fp64", False),
    ("hex842", "eff_perm", True, "fp32", True),
    ("tet2", "eff_perm", True, "fp32", False),
    ("tet2", "p_int", True, "fp64", False),
    ("tet2", "p_int", False, "fp32", True),
])
def test_solve_gradient_matches_the_direct_solve_twin(gpu_ctx, mesh, qoi, k_divides, storage, hybrid):
    """every level of the 8^3 / 4^3 / 2^3 hierarchy and of cube_tet refined twice (a hybridized handle: its two finest levels),
    nonzero essential data, adj_rhs NULL and random, both storages of the preconditioned vectors"""
    from parelagmc_amd import capi
    n_mc = 2 if hybrid else None
    h, dp = cases.problem(mesh, k_divides, qoi, n_mc_levels=n_mc)
    st = capi.PMC_STORAGE_FP32 if storage == "fp32" else capi.PMC_STORAGE_FP64
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st, **TIGHT), hybrid=hybrid)
    ds_loose = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st), hybrid=hybrid)
    rng = np.random.default_rng(43)
    for level in range(dp.n_mc_levels):
        worst = _check_level(ds, ds_loose, dp, level, rng, hybrid)
        print(f"{mesh} {qoi} k_divides={k_divides} {storage} hybrid={hybrid} level {level}: gradient rel. error {worst:.2e}")
    ds.close()
    ds_loose.close()


# ---- 6. the log-likelihood ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_divides", [True, False])
def test_loglik_gradient_matches_the_twin(gpu_ctx, k_divides):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import darcy_adjoint
    h, dp = cases.problem("hex842", k_divides)
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    rng = np.random.default_rng(47)
    noise = 0.01
    for level in (0, 1):
        L = dp.levels[level]
        Gobs = cases.two_cell_observations(h, level)
        ds.SetObservations(level, Gobs)
        k = np.exp(rng.standard_normal((5, L.n_p)))
        data = ds.ComputeG(level, np.exp(rng.standard_normal((1, L.n_p))))[0][0]     # observations of another field
        for wrt_log in (False, True):
            ll, G, g = ds.loglik_gradient(level, k, data, noise, wrt_log)
            Gc = ds.ComputeG(level, k)[0]
            ll_c = (-1.0 / (noise * 2)) * np.sum((Gc - data) ** 2, axis=1)
            assert np.allclose(G, Gc, rtol=1e-12, atol=0.0) and np.allclose(ll, ll_c, rtol=1e-12, atol=0.0)
            for b in range(5):
                ll_r, G_r, g_r = darcy_adjoint.loglik_gradient(dp, level, k[b], Gobs, data, noise, wrt_log)
                e = rel(g[b], g_r)
                print(f"loglik k_divides={k_divides} level {level} wrt_log={wrt_log} column {b}: rel. error {e:.2e}")
                assert e < TOL_LOGLIK
                assert abs(ll[b] - ll_r) <= 1e-9 * abs(ll_r)
            # the host class behind the C entry of pmc_host.h: the C ABI's values, bit for bit
            from parelagmc_amd import host_api
            ll_h, g_h = host_api.bayes_loglik_gradient(ds, level, k, data, noise, wrt_log)
            assert np.array_equal(ll_h, ll) and np.array_equal(g_h, g)
    ds.close()


FAMILY_SOLVE_CASES = [("tri", "fp32", 0), ("quad", "fp64", 0), ("agg2", "fp32", 0), ("agg2", "fp64", 1), ("agg2s", "fp64", 0),
                      ("agg2s", "fp32", 1), ("agg3s", "fp32", 1)]


def family_solvers(gpu_ctx, case, storage, mg):
    """(problem, handle at the 1e-12 options, handle at the default options, family): saddle-point handles"""
    import derivative_family_cases as fcases
    from parelagmc_amd import capi
    dp = fcases.problem(case)
    st = capi.PMC_STORAGE_FP32 if storage == "fp32" else capi.PMC_STORAGE_FP64
    agg = case.startswith("agg")
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st, mg_coarsening=mg, **(TIGHT_AGG if agg else TIGHT)))
    ds_loose = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(precond_storage=st, mg_coarsening=mg))
    return dp, ds, ds_loose, "agg" if agg else case


@pytest.mark.parametrize("case,storage,mg", FAMILY_SOLVE_CASES)
def test_gradients_on_other_families(gpu_ctx, case, storage, mg):
    """solve_gradient (adj_rhs NULL and random, both wrt_log) and loglik_gradient on EVERY level of the cases of
    tests/derivative_family_cases.py against the twins' direct solves: the mass sensitivity in its <NB, 3> form (tri), on
    quadrilaterals, and in its general form with the padding of Darcy::ensure_gradient (levels 1 and 2 of the agglomerated
    cases; level 2 of agg2s / agg3s with flux dofs of up to 5 / 11 agglomerates), behind the solves it serves.  nb = 3, and
    one call of BatchWidth + 3 on the finest level; both storages of the preconditioned vectors, both V-cycle modes on the
    agglomerated levels, both k_divides (the cases' own).
    Measured on an MI355X (printed by this test):
        tri k_divides=True fp32 mg_coarsening=0: gradient rel. error 2.67e-11, loglik gradient 1.87e-11
        quad k_divides=False fp64 mg_coarsening=0: gradient rel. error 6.97e-12, loglik gradient 6.81e-12
        agg2 k_divides=False fp32 mg_coarsening=0: gradient rel. error 5.44e-12, loglik gradient 1.86e-11
        agg2 k_divides=False fp64 mg_coarsening=1: gradient rel. error 5.00e-12, loglik gradient 6.93e-12
        agg2s k_divides=True fp64 mg_coarsening=0: gradient rel. error 2.26e-11, loglik gradient 2.10e-11
        agg2s k_divides=True fp32 mg_coarsening=1: gradient rel. error 2.56e-11, loglik gradient 1.25e-11
        agg3s k_divides=False fp32 mg_coarsening=1: gradient rel. error 8.79e-12, loglik gradient 5.53e-12"""
    import derivative_family_cases as fcases
    from parelagmc_amd.fe import darcy_adjoint
    dp, ds, ds_loose, family = family_solvers(gpu_ctx, case, storage, mg)
    rng = np.random.default_rng(43)
    worst_g = worst_ll = 0.0
    for level in range(dp.n_mc_levels):
        worst_g = max(worst_g, _check_level(ds, ds_loose, dp, level, rng, False, tol=TOL_GRAD_FAMILY[family]))
        L = dp.levels[level]
        Gobs = fcases.observations(case, level)
        ds.SetObservations(level, Gobs)
        k = np.exp(rng.standard_normal((3, L.n_p)))
        data = ds.ComputeG(level, np.exp(rng.standard_normal((1, L.n_p))))[0][0]
        for wrt_log in (False, True):
            ll, G, g = ds.loglik_gradient(level, k, data, 0.01, wrt_log)
            for b in range(3):
                ll_r, G_r, g_r = darcy_adjoint.loglik_gradient(dp, level, k[b], Gobs, data, 0.01, wrt_log)
                worst_ll = max(worst_ll, rel(g[b], g_r))
                assert abs(ll[b] - ll_r) <= 1e-9 * abs(ll_r) and np.allclose(G[b], G_r, rtol=1e-9, atol=0.0)
    # one call wider than a launch on the finest level: the first and the last columns of every piece
    L = dp.levels[0]
    bw = ds.BatchWidth(0)
    k = np.exp(rng.standard_normal((bw + 3, L.n_p)))
    g = ds.solve_gradient(0, k)[2]
    assert g.shape == (bw + 3, L.n_p)
    for b in (0, bw - 1, bw, bw + 1, bw + 2):
        worst_g = max(worst_g, rel(g[b], darcy_adjoint.gradient(dp, 0, k[b])))
    print(f"{case} k_divides={dp.k_divides} {storage} mg_coarsening={mg}: gradient rel. error {worst_g:.2e}, loglik gradient "
          f"{worst_ll:.2e}")
    ds.close()
    ds_loose.close()
    assert worst_g < TOL_GRAD_FAMILY[family] and worst_ll < TOL_LOGLIK_FAMILY[family]


def test_gradient_calls_refuse_bad_arguments(gpu_ctx):
    from parelagmc_amd import capi
    h, dp = cases.problem("hex4")
    L = dp.levels[0]
    ds = capi.DarcySolver(gpu_ctx, dp)
    lib = gpu_ctx.lib
    k = np.ones((1, L.n_p))
    v = np.ones((1, L.n_u + L.n_p))
    g = np.empty((1, L.n_p))
    ll, G, data = np.empty(1), np.empty(2), np.zeros(2)
    pk, pv, pg = k.ctypes.data, v.ctypes.data, g.ctypes.data
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    H = capi.PMC_MEM_HOST

    def refused(rc):
        assert rc == PMC_ERR_INVALID
        assert lib.pmc_last_error().decode() != ""

    for level, nb, kk, gg in ((-1, 1, pk, pg), (dp.n_mc_levels, 1, pk, pg), (0, 0, pk, pg), (0, 1, None, pg), (0, 1, pk, None)):
        refused(lib.pmc_darcy_mass_sensitivity(ds.h, level, nb, kk, pv, pv, 0, gg, H))
        refused(lib.pmc_darcy_solve_gradient(ds.h, level, nb, kk, None, 0, None, None, gg, None, None, H, None, None))
        refused(lib.pmc_darcy_loglik_gradient(ds.h, level, nb, kk, dptr(data), 0.01, 0, dptr(ll), dptr(G), gg, H, None))
    # no observation functionals yet; then a non-positive noise variance
    refused(lib.pmc_darcy_loglik_gradient(ds.h, 0, 1, pk, dptr(data), 0.01, 0, dptr(ll), dptr(G), pg, H, None))
    ds.SetObservations(0, cases.two_cell_observations(h))
    for noise in (0.0, -1.0):
        refused(lib.pmc_darcy_loglik_gradient(ds.h, 0, 1, pk, dptr(data), noise, 0, dptr(ll), dptr(G), pg, H, None))
    assert lib.pmc_darcy_loglik_gradient(ds.h, 0, 1, pk, dptr(data), 0.01, 0, dptr(ll), dptr(G), pg, H, None) == 0
    ds.close()


# ---- 7. graph replay ----------------------------------------------------------------------------------------------------
def test_gradient_under_graph_replay(gpu_ctx):
    """forward, gradient, forward on one handle with captured MINRES iterations: a graph of the forward solve replayed for the
    adjoint right-hand side (or the reverse) would show in either"""
    from parelagmc_amd import capi
    h, dp = cases.problem("hex8")
    L = dp.levels[0]
    rng = np.random.default_rng(53)
    k = np.exp(rng.standard_normal((4, L.n_p)))
    eager = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    graph = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(use_graph=1, check_every=2, **TIGHT))
    g_ref, Q_ref, _, _ = _twin(dp, 0, k, None, False)
    Q0, _, x0 = graph.SolveFwd(0, k, want_solution=True)
    Q1, _, g, x1, lam1 = graph.solve_gradient(0, k, want_solution=True)
    Q2, _, x2 = graph.SolveFwd(0, k, want_solution=True)
    Qe, _, ge, xe, lame = eager.solve_gradient(0, k, want_solution=True)
    e = max(rel(g[b], g_ref[b]) for b in range(4))
    print(f"graph replay: gradient rel. error {e:.2e}, eager {max(rel(ge[b], g_ref[b]) for b in range(4)):.2e}")
    assert e < TOL_GRAD and max(rel(ge[b], g_ref[b]) for b in range(4)) < TOL_GRAD
    for Q, x in ((Q0, x0), (Q1, x1), (Q2, x2)):
        assert np.allclose(Q, Qe, rtol=1e-9, atol=0.0) and rel(x, xe) < 1e-9
    assert rel(lam1, lame) < 1e-9
    eager.close()
    graph.close()


# ---- 8. the host classes ------------------------------------------------------------------------------------------------
def test_host_classes_return_the_c_abi_values(tmp_path, hex_hierarchy_small, seeded_rng):
    """tests/c/gradient_smoke.cpp: DarcySolver::SolveFwd_Gradient and BayesianInverseProblem::ComputeGradLogLikelihood (host and
    device vectors) against pmc_darcy_solve_gradient / pmc_darcy_loglik_gradient, compared with memcmp"""
    from parelagmc_amd.fe import build_darcy_problem, build_sampler_problem
    from test_abi_binaries import write_problem_file
    r = subprocess.run(["make", "-C", ROOT, "test-gradient"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sp_ = build_sampler_problem(hex_hierarchy_small, corlen=0.1, lognormal=True)
    dp = build_darcy_problem(hex_hierarchy_small, cases.ESS, cases.OBS, cases.INFLOW)
    nb = 3
    xi = np.zeros((nb, sp_.levels[0].n_s))
    s_expect = [np.zeros((nb, sp_.levels[l].n_s)) for l in range(2)]        # the sampler part of the file is not read here
    k = [np.exp(0.5 * seeded_rng.standard_normal((nb, dp.levels[l].n_p))) for l in range(2)]
    path = str(tmp_path / "problem.bin")
    write_problem_file(path, sp_, dp, xi, s_expect, k, [np.zeros(nb), np.zeros(nb)])
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "gradient_smoke"), path], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("gradient_smoke OK"), r.stdout + r.stderr

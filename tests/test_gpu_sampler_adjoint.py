"""The adjoint of the samplers' Eval on the device (pmc_sampler_eval_adjoint: csrc/sampler_adjoint.hip, csrc/kl_adjoint.hip)
and the log-posterior gradient of the host layer against their numpy twin with sparse direct solves
(parelagmc_amd/fe/sampler_adjoint.py, itself checked against the oracle in tests/test_sampler_adjoint.py).  Run with -m gpu on
an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import darcy_gradient_cases as dcases
import sampler_adjoint_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
# Measured on an MI355X at rel_tol = abs_tol = 1e-12 over every case of this file: the relative L2 error of the device adjoint
# against the twin's direct solves is at most 2.3e-12 (MEASURED_TWIN; the hybridized handle on cube_tet r = 2), the defect of
# the adjoint identity against the device's own Eval, |<Eval(xi), v> - <xi, EvalAdjoint(v)>| / (|Eval(xi)| |v|), at most 2.3e-13
# (MEASURED_IDENTITY), the relative L2 error of ComputeGradLogPosterior against the twin at most 1.7e-11 (MEASURED_LOGPOST).  The
# KL kernel alone stays below 0.05 of its summation bound.  The bounds are 10 x the measured values and never looser
# than 1e-7 (the rule at the top of tests/test_gpu_darcy_gradient.py).
MEASURED_TWIN = 2.3e-12
MEASURED_IDENTITY = 2.3e-13
MEASURED_LOGPOST = 1.7e-11
TOL_TWIN = min(10 * MEASURED_TWIN, 1e-7)
TOL_IDENTITY = min(10 * MEASURED_IDENTITY, 1e-7)
TOL_LOGPOST = min(10 * MEASURED_LOGPOST, 1e-7)
# The same figures on the sampler problems of tests/derivative_family_cases.py - "agg": the agglomerated levels of cube_tet
# refined twice (P_s with 5 to 14 children per parent, unit and non-unit weights), "tri": the 2-D hierarchy - measured on an
# MI355X with the family cases of test_pde_adjoint_matches_the_twin_and_its_own_eval and test_logpost_gradient_on_triangles;
# the lines they come from are quoted in those docstrings.  One constant per family and quantity, the same rule.
MEASURED_TWIN_FAMILY = {"tri": 1.0e-12, "agg": 2.3e-12}
MEASURED_IDENTITY_FAMILY = {"tri": 1.8e-14, "agg": 1.7e-13}
MEASURED_LOGPOST_TRI = 9.5e-12
TOL_TWIN_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_TWIN_FAMILY.items()}
TOL_IDENTITY_FAMILY = {f: min(10 * m, 1e-7) for f, m in MEASURED_IDENTITY_FAMILY.items()}
TOL_LOGPOST_TRI = min(10 * MEASURED_LOGPOST_TRI, 1e-7)
TIGHT_AGG = dict(TIGHT, max_iter=600)          # the iteration limit of tests/test_gpu_agglomerated.py
FAMILY_KINDS = ("agg-unit", "agg-nonunit", "tri")
PMC_ERR_INVALID = -1
NB_KL = (1, 2, 4, 5, 11, 16, 17, 64, 129)      # VALU widths, one tile, ragged tiles, 129: a second column group of the grid


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


# ---- the KL kernel alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kl_handles(gpu_ctx):
    """Gaussian and lognormal KL handles per (mesh, modes), and the device's own modes Phi_l Lambda^1/2 of every level, read
    back exactly through Eval of unit vectors (each entry is one product with 1.0 and sums of zeros)"""
    from parelagmc_amd import capi
    out = {}
    for mesh, nm in (("hex16", (3, 3, 3)), ("hex16", (4, 4, 4)), ("ragged", (3, 3, 3)), ("ragged", (4, 4, 4))):
        kp = cases.kl_problem(mesh, nm)
        gauss = capi.KLSampler(gpu_ctx, kp)
        logn = capi.KLSampler(gpu_ctx, cases.kl_problem(mesh, nm, lognormal=True))
        m = kp.nmodes
        phis = []
        for lvl in range(kp.n_mc_levels):
            unit = np.zeros((m, gauss.xi_size(lvl)))
            unit[np.arange(m), np.arange(m)] = 1.0
            phis.append(np.ascontiguousarray(gauss.Eval(lvl, unit, xi_level=lvl).T))      # n_s(lvl) x m
            assert np.allclose(phis[-1], np.asarray(kp.evects[lvl]) * np.sqrt(kp.evals), rtol=1e-9, atol=1e-12)
        out[(mesh, m)] = (kp, gauss, logn, phis)
    yield out
    for _, gauss, logn, _ in out.values():
        gauss.close()
        logn.close()


@pytest.mark.parametrize("mesh,m,level", [("hex16", 27, 0), ("hex16", 27, 1), ("hex16", 64, 0), ("hex16", 64, 1),
                                          ("ragged", 27, 0), ("ragged", 27, 1), ("ragged", 64, 0)])
def test_kl_adjoint_kernel(gpu_ctx, kl_handles, mesh, m, level):
    """n_s = 4096 (four reduction chunks), 512, 240 and 30 (ragged stages); 27 modes (no multiple of 4 or 16) and 64; every
    width of NB_KL; host and device memory.  Every entry within the first-order summation bound (n_s + 3) 2^-52 sum_i |v_i
    Phi_ik| of a reference summed in extended precision; column b bitwise the same for every nb > 4 and for the pieces wider
    than 4 of the call split 129 = 64 + 64 + 1; the one-column piece takes the VALU kernel (whose bits may differ from the
    MFMA kernel's, as for the forward pair): within the bound, and bitwise the VALU kernel's value at every width <= 4.  The
    entries m.. are exactly 0."""
    kp, gauss, logn, phis = kl_handles[(mesh, m)]
    assert kp.nmodes == m and level < kp.n_mc_levels
    n = gauss.SampleSize(level)
    assert n == {"hex16": (4096, 512), "ragged": (240, 30)}[mesh][level]
    Phi = phis[level]
    rng = np.random.default_rng(83)
    V = rng.standard_normal((129, n))
    ref = V.astype(np.longdouble) @ Phi.astype(np.longdouble)
    bound = (n + 3) * 2.0 ** -52 * (np.abs(V) @ np.abs(Phi))
    n_xi = gauss.xi_size(level)
    full = gauss.EvalAdjoint(level, V)
    assert full.shape == (129, n_xi)
    valu = gauss.EvalAdjoint(level, V[:4])
    worst = 0.0
    for nb in NB_KL:
        g = gauss.EvalAdjoint(level, V[:nb])
        err = np.abs(g[:, :m].astype(np.longdouble) - ref[:nb])
        worst = max(worst, float(np.max(err / bound[:nb])))
        assert np.all(err <= bound[:nb]), f"nb {nb}"
        assert np.all(g[:, m:] == 0.0)
        assert np.array_equal(g, full[:nb] if nb > 4 else valu[:nb]), f"nb {nb}"
    print(f"{mesh} m={m} level {level} (n_s {n}): max error / bound {worst:.3f}")
    # the call split 129 = 64 + 64 + 1
    assert np.array_equal(gauss.EvalAdjoint(level, V[:64]), full[:64])
    assert np.array_equal(gauss.EvalAdjoint(level, V[64:128]), full[64:128])
    last = gauss.EvalAdjoint(level, V[128:129])
    assert np.all(np.abs(last[:, :m].astype(np.longdouble) - ref[128:]) <= bound[128:]) and np.all(last[:, m:] == 0.0)
    assert np.array_equal(last[0], gauss.EvalAdjoint(level, V[[128, 0, 1]])[0])
    # a call wider than one launch (256): 260 = 256 + 4, the remainder of 4 still through the MFMA kernel
    wide = gauss.EvalAdjoint(level, np.concatenate([V, V, V[:2]]))
    assert wide.shape == (260, n_xi)
    assert np.array_equal(wide[:129], full) and np.array_equal(wide[129:258], full) and np.array_equal(wide[258:], full[:2])
    # device memory
    for nb in (129, 4):
        vd, gd = gpu_ctx.array(V[:nb]), gpu_ctx.empty(nb * n_xi)
        gauss.EvalAdjoint(level, vd, grad_out=gd, nbatch=nb)
        assert np.array_equal(gd.download().reshape(nb, n_xi), full[:nb] if nb > 4 else valu[:nb])
        vd.free()
        gd.free()
    # a finer xi: the same values in the first m entries of the longer vector, zeros behind
    if level == 1:
        g0 = gauss.EvalAdjoint(1, V[:17], xi_level=0)
        assert g0.shape == (17, gauss.xi_size(0)) and np.array_equal(g0[:, :m], full[:17, :m]) and np.all(g0[:, m:] == 0.0)
    # the lognormal handle with s_out equals the Gaussian handle fed v * s_out (one rounding, formed in the load)
    S = np.exp(0.3 * rng.standard_normal((17, n)))
    for nb in (3, 17):
        assert np.array_equal(logn.EvalAdjoint(level, V[:nb], s_out=S[:nb]), gauss.EvalAdjoint(level, V[:nb] * S[:nb]))
    assert np.array_equal(logn.EvalAdjoint(level, V[:17]), full[:17])          # s_out None: v is dJ/dlog s_out already


# ---- the PDE samplers ---------------------------------------------------------------------------------------------------
def _pde_case(kind, mesh, lognormal):
    """(problem for the handle, problem for the twin, projection name, per-level projections for the twin, l2_ops)"""
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    if kind in FAMILY_KINDS:
        import derivative_family_cases as fcases
        sp = fcases.sampler_problem(kind, lognormal)
        return sp, sp, "none", None, None
    if kind in ("saddle", "hybrid"):
        h = cases.hierarchy(mesh)
        sp = build_sampler_problem(h, corlen=cases.CORLEN, lognormal=lognormal)
        if kind == "saddle":
            return sp, sp, "none", None, None
        # (the hybridized handles of the three-level hierarchies: their two finest levels, as in tests/test_gpu_darcy_gradient.py)
        return (build_hybrid_sampler_problem(h, corlen=cases.CORLEN, lognormal=lognormal, n_mc_levels=min(2, h.nlevels)), sp,
                "none", None, None)
    if kind.endswith("gather"):
        sp, proj = cases.gather_problem(mesh, lognormal)
        hp = sp if kind == "gather" else build_hybrid_sampler_problem(cases.embedded_hierarchy(mesh), corlen=cases.CORLEN,
                                                                      lognormal=lognormal, embedded=True)
        return hp, sp, "gather", proj, None
    sp, proj, ops = cases.l2_problem(mesh, lognormal)
    hp = sp if kind == "l2" else build_hybrid_sampler_problem(cases.hierarchy(mesh), corlen=cases.CORLEN, lognormal=lognormal)
    return hp, sp, "l2", proj, ops


PDE_CASES = [("saddle", "hex842"), ("saddle", "tet2"), ("hybrid", "hex842"), ("hybrid", "tet2"), ("hybrid", "ragged"),
             ("gather", "hex842"), ("gather", "ragged"), ("l2", "hex842"), ("l2", "ragged"), ("hybrid-gather", "ragged"),
             ("hybrid-l2", "ragged"), ("agg-unit", "tet2"), ("agg-nonunit", "tet2"), ("tri", "square")]


def _family_of(kind):
    """(family for the tolerances or None, the (level, xi_level) pairs to run or None for all, solver options)"""
    if kind not in FAMILY_KINDS:
        return None, None, TIGHT
    import derivative_family_cases as fcases
    return ("tri", fcases.level_pairs(kind), TIGHT) if kind == "tri" else ("agg", fcases.level_pairs(kind), TIGHT_AGG)


@pytest.mark.parametrize("kind,mesh", PDE_CASES)
def test_pde_adjoint_matches_the_twin_and_its_own_eval(gpu_ctx, kind, mesh):
    """every (level, xi_level) pair of the hierarchy; nb = 3 (launches of 2 + 1) and BatchWidth + 3 on the finest level;
    lognormal handles with s_out against the twin, Gaussian handles for the adjoint identity against the device's own Eval;
    the default 1e-6 options within 1e-4 of the tight ones (100 x rel_tol, the rule of DESIGN.md section 16).
    agg-unit / agg-nonunit / tri (tests/derivative_family_cases.py; the pairs (0, 0), (1, 0), (2, 0), (2, 2), on tri (0, 0),
    (1, 0), (1, 1)): the restriction chain R = P_s[level-1]^T ... P_s[xi_level]^T of the adjoint with 5 to 14 children per
    parent and weights of 0.5 to 1 (agg-nonunit) - the 8-children unit injections of the other cases hide a transposed,
    unweighted or mis-sized P_s - and the 2-D SPDE (g = 50.13 in the factor -g sqrt(w)).  Seeded fault (built once into a
    copy of the library and run on an MI355X, not committed): eval_adjoint_chunk applying P_s^T with unit weights fails
    agg-nonunit here and no other test of this file or of the Eval tangent.
    Measured on an MI355X (printed by this test):
        agg-unit tet2: rel. error against the twin 1.71e-12, identity defect 1.36e-13
        agg-nonunit tet2: rel. error against the twin 2.22e-12, identity defect 1.67e-13
        tri square: rel. error against the twin 9.94e-13, identity defect 1.75e-14"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import sampler_adjoint
    family, pairs, tight = _family_of(kind)
    tol_twin = TOL_TWIN if family is None else TOL_TWIN_FAMILY[family]
    tol_identity = TOL_IDENTITY if family is None else TOL_IDENTITY_FAMILY[family]
    prob, twin_prob, projection, projs, ops = _pde_case(kind, mesh, True)
    gprob = _pde_case(kind, mesh, False)[0]
    logn = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(**tight), projection=projection, l2_ops=ops)
    loose = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(), projection=projection, l2_ops=ops)
    gauss = capi.PDESampler(gpu_ctx, gprob, capi.solver_opts(**tight), projection=projection, l2_ops=ops)
    rng = np.random.default_rng(89)
    cache = {}
    worst_twin = worst_id = 0.0
    for level in range(prob.n_mc_levels):
        for xi_level in range(level + 1):
            if pairs is not None and (level, xi_level) not in pairs:
                continue
            widths = (3, logn.BatchWidth(level) + 3) if (level, xi_level) == (0, 0) else (3,)
            for nb in widths:
                xi = rng.standard_normal((nb, logn.xi_size(xi_level)))
                v = rng.standard_normal((nb, logn.SampleSize(level)))
                s = logn.Eval(level, xi, xi_level=xi_level)
                g, st = logn.EvalAdjoint(level, v, s_out=s, xi_level=xi_level, return_stats=True)
                assert g.shape == xi.shape and all(t[1] == 1 for t in st), st
                proj = None if projs is None else projs[level]
                ref = np.stack([sampler_adjoint.eval_adjoint(twin_prob, level, xi_level, v[b], s[b], proj, cache)
                                for b in range(nb)])
                e = max(rel(g[b], ref[b]) for b in range(nb))
                worst_twin = max(worst_twin, e)
                assert e < tol_twin, (level, xi_level, nb, e)
                # the identity on the Gaussian handle: the device's own forward map
                sg = gauss.Eval(level, xi, xi_level=xi_level)
                gg = gauss.EvalAdjoint(level, v, xi_level=xi_level)
                d = max(abs(float(sg[b] @ v[b]) - float(xi[b] @ gg[b])) / (np.linalg.norm(sg[b]) * np.linalg.norm(v[b]))
                        for b in range(nb))
                worst_id = max(worst_id, d)
                assert d < tol_identity, (level, xi_level, nb, d)
                if nb == 3:
                    gl = loose.EvalAdjoint(level, v, s_out=s, xi_level=xi_level)
                    assert max(rel(gl[b], g[b]) for b in range(nb)) < 1e-4
                    # device memory: the same bits
                    vd, sd, gd = gpu_ctx.array(v), gpu_ctx.array(s), gpu_ctx.empty(g.size)
                    logn.EvalAdjoint(level, vd, s_out=sd, xi_level=xi_level, grad_out=gd, nbatch=nb)
                    assert np.array_equal(gd.download().reshape(g.shape), g)
                    for a in (vd, sd, gd):
                        a.free()
    print(f"{kind} {mesh}: rel. error against the twin {worst_twin:.2e}, identity defect {worst_id:.2e}")
    for smp in (logn, loose, gauss):
        smp.close()


def test_adjoint_under_graph_replay(gpu_ctx):
    """Eval, EvalAdjoint, Eval on one handle with captured MINRES iterations: a graph of the forward solve replayed for the
    adjoint right-hand side (or the reverse) would show in either"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    h = cases.hierarchy("hex842")
    rng = np.random.default_rng(97)
    for build in (build_sampler_problem, build_hybrid_sampler_problem):
        prob = build(h, corlen=cases.CORLEN)
        eager = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(**TIGHT))
        graph = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(use_graph=1, check_every=2, **TIGHT))
        xi = rng.standard_normal((4, eager.xi_size(0)))
        v = rng.standard_normal((4, eager.SampleSize(0)))
        s0 = graph.Eval(0, xi)
        g = graph.EvalAdjoint(0, v)
        s1 = graph.Eval(0, xi)
        g1 = graph.EvalAdjoint(0, v)
        se, ge = eager.Eval(0, xi), eager.EvalAdjoint(0, v)
        assert rel(s0, se) < 1e-9 and rel(s1, se) < 1e-9
        assert rel(g, ge) < 1e-9 and rel(g1, ge) < 1e-9
        eager.close()
        graph.close()


# ---- the log-posterior --------------------------------------------------------------------------------------------------
def test_logpost_gradient_matches_the_twin(gpu_ctx):
    """BayesianInverseProblem::ComputeGradLogPosterior through pmc_bayes_logpost_gradient: hex 8^3 / 4^3, a lognormal sampler,
    two observations, both levels and a finer xi, host and device vectors"""
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_sampler_problem, sampler_adjoint
    h, dp = dcases.problem("hex842", True)
    sp = build_sampler_problem(h, corlen=cases.CORLEN, lognormal=True, n_mc_levels=2)
    smp = capi.PDESampler(gpu_ctx, sp, capi.solver_opts(**TIGHT))
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    rng = np.random.default_rng(101)
    noise = 0.01
    cache = {}
    worst = 0.0
    for level, xi_level in ((0, 0), (1, 1), (1, 0)):
        Gobs = dcases.two_cell_observations(h, level)
        ds.SetObservations(level, Gobs)
        data = ds.ComputeG(level, np.exp(0.3 * rng.standard_normal((1, dp.levels[level].n_p))))[0][0]
        xi = 0.5 * rng.standard_normal((3, sp.levels[xi_level].n_s))
        lp, g = host_api.bayes_logpost_gradient(smp, ds, level, xi, data, noise, xi_level=xi_level)
        for b in range(3):
            lp_r, g_r = sampler_adjoint.logpost_gradient(sp, dp, level, xi[b], Gobs, data, noise, xi_level=xi_level, cache=cache)
            e = rel(g[b], g_r)
            worst = max(worst, e)
            print(f"logpost level {level} from xi on level {xi_level} column {b}: rel. error {e:.2e}")
            assert e < TOL_LOGPOST
            assert abs(lp[b] - lp_r) <= 1e-9 * abs(lp_r)
        xd, gd = gpu_ctx.array(xi), gpu_ctx.empty(xi.size)
        lp_d, _ = host_api.bayes_logpost_gradient(smp, ds, level, xd, data, noise, xi_level=xi_level, nbatch=3, grad_out=gd)
        assert np.array_equal(lp_d, lp) and np.array_equal(gd.download().reshape(xi.shape), g)
        xd.free()
        gd.free()
    print(f"logpost: largest rel. error {worst:.2e}")
    ds.close()
    smp.close()


def test_logpost_gradient_on_triangles(gpu_ctx):
    """pmc_bayes_logpost_gradient on the 2-D hierarchy of tests/derivative_family_cases.py (1312 / 328 triangles, lognormal
    sampler at corlen 0.1, two observations): mass_sensitivity_kernel<NB, 3> and the 2-D Eval adjoint in one chain; both
    levels and a finer xi, host and device vectors.
    Measured on an MI355X (printed by this test):
        logpost on triangles: largest rel. error 9.43e-12"""
    import derivative_family_cases as fcases
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import sampler_adjoint
    dp, sp = fcases.problem("tri"), fcases.sampler_problem("tri", True)
    smp = capi.PDESampler(gpu_ctx, sp, capi.solver_opts(**TIGHT))
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    rng = np.random.default_rng(101)
    noise = 0.01
    cache = {}
    worst = 0.0
    for level, xi_level in fcases.level_pairs("tri"):
        Gobs = fcases.observations("tri", level)
        ds.SetObservations(level, Gobs)
        data = ds.ComputeG(level, np.exp(0.3 * rng.standard_normal((1, dp.levels[level].n_p))))[0][0]
        xi = 0.5 * rng.standard_normal((3, sp.levels[xi_level].n_s))
        lp, g = host_api.bayes_logpost_gradient(smp, ds, level, xi, data, noise, xi_level=xi_level)
        for b in range(3):
            lp_r, g_r = sampler_adjoint.logpost_gradient(sp, dp, level, xi[b], Gobs, data, noise, xi_level=xi_level, cache=cache)
            worst = max(worst, rel(g[b], g_r))
            assert abs(lp[b] - lp_r) <= 1e-9 * abs(lp_r)
        xd, gd = gpu_ctx.array(xi), gpu_ctx.empty(xi.size)
        lp_d, _ = host_api.bayes_logpost_gradient(smp, ds, level, xd, data, noise, xi_level=xi_level, nbatch=3, grad_out=gd)
        assert np.array_equal(lp_d, lp) and np.array_equal(gd.download().reshape(xi.shape), g)
        xd.free()
        gd.free()
    print(f"logpost on triangles: largest rel. error {worst:.2e}")
    ds.close()
    smp.close()
    assert worst < TOL_LOGPOST_TRI


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_eval_adjoint_refuses_bad_arguments(gpu_ctx):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    h = cases.hierarchy("ragged")
    gauss = capi.PDESampler(gpu_ctx, build_sampler_problem(h, corlen=cases.CORLEN))
    logn = capi.PDESampler(gpu_ctx, build_sampler_problem(h, corlen=cases.CORLEN, lognormal=True))
    klg = capi.KLSampler(gpu_ctx, cases.kl_problem("ragged"))
    lib = gpu_ctx.lib
    H = capi.PMC_MEM_HOST

    def refused(rc):
        assert rc == PMC_ERR_INVALID
        assert lib.pmc_last_error().decode() != ""

    for smp in (gauss, logn, klg):
        n = smp.SampleSize(0)
        v, g = np.ones((1, n)), np.empty((1, n))
        pv, pg = v.ctypes.data, g.ctypes.data
        for level, xi_level, nb, vv, gg in ((-1, 0, 1, pv, pg), (smp.nlevels, 0, 1, pv, pg), (0, -1, 1, pv, pg), (0, 1, 1, pv, pg),
                                            (0, 0, 0, pv, pg), (0, 0, 1, None, pg), (0, 0, 1, pv, None)):
            refused(lib.pmc_sampler_eval_adjoint(smp.h, level, xi_level, nb, vv, None, gg, H, None))
        if smp is not logn:           # s_out on a handle that is not lognormal
            refused(lib.pmc_sampler_eval_adjoint(smp.h, 0, 0, 1, pv, pv, pg, H, None))
        assert lib.pmc_sampler_eval_adjoint(smp.h, 0, 0, 1, pv, pv if smp is logn else None, pg, H, None) == 0
    # a conditioned handle: out of scope, refused; accepted again once the conditioner is detached
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    n = gauss.SampleSize(0)
    H0 = point_observations(n, pick_observation_elements(h, 2, 5))
    for smp in (gauss, klg):
        cond = capi.Conditioner(smp, H0, np.array([0.3, -0.2]))
        smp.SetConditioner(cond)
        v, g = np.ones((1, n)), np.empty((1, n))
        refused(lib.pmc_sampler_eval_adjoint(smp.h, 0, 0, 1, v.ctypes.data, None, g.ctypes.data, H, None))
        smp.SetConditioner(None)
        assert lib.pmc_sampler_eval_adjoint(smp.h, 0, 0, 1, v.ctypes.data, None, g.ctypes.data, H, None) == 0
        cond.close()
    # the prior's part: grad -= xi, -|xi|^2 / 2; refusals
    xi = np.random.default_rng(103).standard_normal((5, n))
    g = np.ones((5, n))
    lp = np.empty(5)
    dptr = lp.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.pmc_sampler_logprior_gradient(gauss.h, n, 5, xi.ctypes.data, g.ctypes.data, dptr, H) == 0
    assert np.array_equal(g, 1.0 - xi) and np.allclose(lp, -0.5 * np.sum(xi * xi, axis=1), rtol=1e-14, atol=0.0)
    for nn, nb, px, pgr in ((0, 5, xi.ctypes.data, g.ctypes.data), (n, 0, xi.ctypes.data, g.ctypes.data), (n, 5, None, g.ctypes.data),
                            (n, 5, xi.ctypes.data, None)):
        refused(lib.pmc_sampler_logprior_gradient(gauss.h, nn, nb, px, pgr, dptr, H))
    assert lib.pmc_sampler_is_lognormal(gauss.h) == 0 and lib.pmc_sampler_is_lognormal(logn.h) == 1
    for smp in (gauss, logn, klg):
        smp.close()


# ---- the C caller -------------------------------------------------------------------------------------------------------
def test_c_caller(tmp_path, hex_hierarchy_small, seeded_rng):
    """tests/c/sampler_adjoint_smoke.c (plain C, include/pmc.h only) builds with -Wall -Wextra -Werror and passes: the
    saddle-point sampler and pmc_sampler_create_hybrid_from_elements, every (level, xi_level), host and device buffers"""
    from parelagmc_amd.fe import build_darcy_problem, build_sampler_problem
    from test_abi_binaries import write_problem_file
    r = subprocess.run(["make", "-C", ROOT, "test-sampler-adjoint"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sp_ = build_sampler_problem(hex_hierarchy_small, corlen=0.1, lognormal=True)
    dp = build_darcy_problem(hex_hierarchy_small, dcases.ESS, dcases.OBS, dcases.INFLOW)
    nb = 3
    xi = np.zeros((nb, sp_.levels[0].n_s))                                   # the program draws its own xi
    s_expect = [np.zeros((nb, sp_.levels[l].n_s)) for l in range(2)]
    k = [np.exp(0.5 * seeded_rng.standard_normal((nb, dp.levels[l].n_p))) for l in range(2)]
    path = str(tmp_path / "problem.bin")
    write_problem_file(path, sp_, dp, xi, s_expect, k, [np.zeros(nb), np.zeros(nb)])
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "sampler_adjoint_smoke"), path], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("sampler_adjoint_smoke OK"), r.stdout + r.stderr

"""The numpy twins of the tangent directions and of the Gauss-Newton Hessian action (parelagmc_amd/fe/darcy_adjoint.py:
mass_tangent / tangent / gn_hessvec; parelagmc_amd/fe/sampler_adjoint.py: eval_tangent / logpost_gn_hessvec) against central
differences of the oracles' direct solves and of the first-derivative twins, and their structural identities.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.darcy_oracle import DarcyOracle  # noqa: E402
from oracle.sampler_oracle import SamplerOracle  # noqa: E402
from parelagmc_amd.fe import (box_mesh, build_darcy_problem, build_hierarchy, build_sampler_problem, darcy_adjoint,  # noqa: E402
                              sampler_adjoint)

import darcy_gradient_cases as dcases  # noqa: E402
import sampler_adjoint_cases as cases  # noqa: E402

STEP = 1e-5          # relative step: k -> k (1 +- STEP d) per entry; xi -> xi +- STEP d
NOISE = 0.01
# Largest relative L2 error |fd - value| / |value| of a directional derivative measured over all cases below:
#   J dk against central differences of the oracle's G                                   2.3e-9   (MEAS_JDK)
#   gn_hessvec against central differences of loglik_gradient at zero misfit             3.2e-9   (MEAS_HV)
#   eval_tangent against central differences of Eval                                     5.3e-10  (MEAS_EVT)
#   logpost_gn_hessvec against central differences of logpost_gradient at zero misfit    7.0e-10  (MEAS_LP)
# Each bound is 100 x the measured value and never looser than 1e-5 (the margin covers the O(STEP^2) truncation on other
# seeds).  The structural identities are asserted at 1e-12 (measured: at most 2.2e-16 for the two
# transpose pairs and 1.6e-15 for the symmetry of H).
MEAS_JDK, MEAS_HV, MEAS_EVT, MEAS_LP = 2.3e-9, 3.2e-9, 5.3e-10, 7.0e-10
TOL_JDK, TOL_HV, TOL_EVT, TOL_LP = (min(100 * m, 1e-5) for m in (MEAS_JDK, MEAS_HV, MEAS_EVT, MEAS_LP))
TOL_IDENT = 1e-12
LEVELS = [(0, 0), (1, 0), (1, 1)]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _setup(mesh, k_divides, seed):
    h, dp = dcases.problem(mesh, k_divides)
    L = dp.levels[0]
    assert np.abs(L.ess_data).max() > 0.0
    rng = np.random.default_rng(seed)
    k = np.exp(rng.standard_normal(L.n_p))
    return h, dp, L, dcases.two_cell_observations(h), rng, k


CASES = pytest.mark.parametrize("mesh,k_divides,wrt_log", [(m, kd, wl) for m in ("hex4", "hex543", "tet1")
                                                           for kd in (True, False) for wl in (False, True)])


@CASES
def test_tangent_matches_central_differences_of_the_oracle(mesh, k_divides, wrt_log):
    """J dk = dG of the tangent solve against (G(k + dk) - G(k - dk)) / 2 from the oracle's pressure.  A wrong sign, a
    missing c', a missing essential-value term or a wrong row of M_e is an O(1) error here."""
    h, dp, L, Gobs, rng, k = _setup(mesh, k_divides, 29)
    norm = 1.0 / np.asarray(Gobs.sum(axis=1)).ravel()
    orc = DarcyOracle(dp)

    def G_of(kk):
        return norm * (Gobs @ orc.solve_fwd(0, kk, return_solution=True)[2][L.n_u:])

    errs = []
    for _ in range(5):
        d = rng.standard_normal(L.n_p)
        dk = STEP * k * d
        fd = (G_of(k + dk) - G_of(k - dk)) / 2.0
        dG = darcy_adjoint.tangent(dp, 0, k, STEP * d if wrt_log else dk, Gobs, wrt_log)
        errs.append(rel(fd, dG))
    print(f"{mesh} k_divides={k_divides} wrt_log={wrt_log}: J dk max rel err {max(errs):.2e}")
    assert max(errs) < TOL_JDK


@CASES
def test_gn_hessvec_matches_central_differences_of_the_gradient_at_zero_misfit(mesh, k_divides, wrt_log):
    """with data = G(k) the Gauss-Newton action is the full Hessian of -loglik: -(g(k + dk) - g(k - dk)) / 2 of
    darcy_adjoint.loglik_gradient (itself checked against the oracle in tests/test_darcy_adjoint.py)"""
    h, dp, L, Gobs, rng, k = _setup(mesh, k_divides, 31)
    data = darcy_adjoint.loglik_gradient(dp, 0, k, Gobs, np.zeros(2), NOISE)[1]

    def grad(kk):
        return darcy_adjoint.loglik_gradient(dp, 0, kk, Gobs, data, NOISE, wrt_log)[2]

    errs = []
    for _ in range(5):
        d = rng.standard_normal(L.n_p)
        dk = STEP * k * d
        fd = -(grad(k + dk) - grad(k - dk)) / 2.0
        hv = darcy_adjoint.gn_hessvec(dp, 0, k, STEP * d if wrt_log else dk, Gobs, NOISE, wrt_log)
        errs.append(rel(fd, hv))
    print(f"{mesh} k_divides={k_divides} wrt_log={wrt_log}: gn_hessvec max rel err {max(errs):.2e}")
    assert max(errs) < TOL_HV


@CASES
def test_structural_identities(mesh, k_divides, wrt_log):
    """the tangent right-hand side is the transpose of the mass sensitivity in (dk, lam); H is symmetric and positive
    semi-definite"""
    h, dp, L, Gobs, rng, k = _setup(mesh, k_divides, 37)
    n = L.n_u + L.n_p
    ess = np.zeros(n, bool)
    ess[:L.n_u] = L.ess_mask.astype(bool)
    x = rng.standard_normal(n)
    worst_t = worst_s = 0.0
    for _ in range(5):
        dk, lam = rng.standard_normal(L.n_p), rng.standard_normal(n)
        lam[ess] = 0.0
        t = darcy_adjoint.mass_tangent(L, k, x, dk, k_divides, wrt_log)[0]
        g = darcy_adjoint.mass_sensitivity(L, k, x, lam, k_divides, wrt_log)[0]
        assert np.all(t[ess] == 0.0) and np.all(t[L.n_u:] == 0.0)
        worst_t = max(worst_t, abs(float(lam @ t) - float(dk @ g)) / (np.linalg.norm(lam) * np.linalg.norm(t)))
        v, w = rng.standard_normal(L.n_p), rng.standard_normal(L.n_p)
        Hv = darcy_adjoint.gn_hessvec(dp, 0, k, v, Gobs, NOISE, wrt_log)
        Hw = darcy_adjoint.gn_hessvec(dp, 0, k, w, Gobs, NOISE, wrt_log)
        worst_s = max(worst_s, abs(float(w @ Hv) - float(v @ Hw)) / (np.linalg.norm(w) * np.linalg.norm(Hv)))
        assert float(v @ Hv) >= 0.0 and float(w @ Hw) >= 0.0
    print(f"{mesh} k_divides={k_divides} wrt_log={wrt_log}: transpose defect {worst_t:.2e}, symmetry defect {worst_s:.2e}")
    assert worst_t <= TOL_IDENT and worst_s <= TOL_IDENT


def test_mass_tangent_extended_precision_and_scale():
    """return_abs / dtype as mass_sensitivity has them: the longdouble sum agrees with the float64 one inside the bound its
    scale gives"""
    h, dp, L, Gobs, rng, k = _setup("hex543", True, 39)
    x, dk = rng.standard_normal((2, L.n_u + L.n_p)), rng.standard_normal((2, L.n_p))
    kk = np.stack([k, k[::-1]])
    t = darcy_adjoint.mass_tangent(L, kk, x, dk, True)
    ref, scale = darcy_adjoint.mass_tangent(L, kk, x, dk, True, return_abs=True, dtype=np.longdouble)
    assert t.shape == ref.shape == scale.shape == (2, L.n_u + L.n_p) and ref.dtype == np.longdouble
    assert np.all(np.abs(t - ref) <= (2 * 6 + 3) * 2.0 ** -52 * scale)
    assert np.all(scale[:, :L.n_u][:, ~L.ess_mask.astype(bool)] > 0.0)


# ---- in the white noise -------------------------------------------------------------------------------------------------
def _sampler_case(kind, lognormal=False):
    """(problem, projections per level or None)"""
    if kind == "kl":
        return cases.kl_problem("ragged", lognormal=lognormal), None
    if kind.startswith("plain"):
        return build_sampler_problem(cases.hierarchy(kind.split("-")[1]), corlen=cases.CORLEN, lognormal=lognormal), None
    return cases.gather_problem("ragged", lognormal) if kind == "gather" else cases.l2_problem("ragged", lognormal)[:2]


KINDS = ["plain-ragged", "plain-tet1", "gather", "l2", "kl"]


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_eval_tangent_is_the_transpose_of_eval_adjoint(kind, level, xi_level):
    """<eval_tangent(v), u> == <v, eval_adjoint(u)>, with and without the f' of a lognormal problem"""
    for lognormal in (False, True):
        prob, projs = _sampler_case(kind, lognormal)
        proj = None if projs is None else projs[level]
        rng = np.random.default_rng(83)
        xi = rng.standard_normal(prob.levels[xi_level].n_s)
        v = rng.standard_normal(xi.size)
        s = sampler_adjoint.eval_forward(prob, level, xi_level, xi, proj) if lognormal else None
        tv = sampler_adjoint.eval_tangent(prob, level, xi_level, v, s, proj)
        u = rng.standard_normal(tv.size)
        adj = sampler_adjoint.eval_adjoint(prob, level, xi_level, u, s, proj)
        d = abs(float(tv @ u) - float(v @ adj)) / (np.linalg.norm(tv) * np.linalg.norm(u))
        print(f"{kind} ({level}, {xi_level}) lognormal={lognormal}: transpose defect {d:.2e}")
        assert d <= TOL_IDENT


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_eval_tangent_matches_central_differences_of_eval(kind, level, xi_level):
    """the lognormal chain: (Eval(xi + h d) - Eval(xi - h d)) / 2 against s_out o L (h d); Eval from the oracle where it
    has one (the KL twin: eval_forward)"""
    prob, projs = _sampler_case(kind, True)
    proj = None if projs is None else projs[level]
    if kind == "kl":
        fun = lambda x: sampler_adjoint.eval_forward(prob, level, xi_level, x)      # noqa: E731
    else:
        so = SamplerOracle(prob)
        fun = lambda x: so.eval(level, xi_level, x, projection=proj)[0]             # noqa: E731
    rng = np.random.default_rng(89)
    xi = rng.standard_normal(prob.levels[xi_level].n_s)
    s = fun(xi)
    errs = []
    for _ in range(5):
        d = STEP * rng.standard_normal(xi.size)
        fd = (fun(xi + d) - fun(xi - d)) / 2.0
        errs.append(rel(fd, sampler_adjoint.eval_tangent(prob, level, xi_level, d, s, proj)))
    print(f"{kind} ({level}, {xi_level}): eval_tangent max rel err {max(errs):.2e}")
    assert max(errs) < TOL_EVT


def _darcy_for(kind):
    """a Darcy problem whose elements number as many as the entries of the sampler's output on every level (the gather and
    the L2 map: the original box)"""
    if kind == "plain-tet1":
        h, dp = dcases.problem("tet1")
        return dp, h
    n, size = {"gather": ([3, 3, 2], [1.2, 2, 2]), "l2": ([3, 2, 2], [1.2, 2, 2])}.get(kind, ([5, 3, 2], [2, 2, 2]))
    h = build_hierarchy(box_mesh(n, size, "hex"), 1)
    dp = build_darcy_problem(h, dcases.ESS, dcases.OBS, dcases.INFLOW)
    rng = np.random.default_rng(3)
    for L in dp.levels:
        L.ess_data[:] = np.where(L.ess_mask.astype(bool), rng.standard_normal(L.n_u), 0.0)
    return dp, h


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_logpost_gn_hessvec_matches_central_differences_of_the_gradient_at_zero_misfit(kind, level, xi_level):
    """H_GN v against -(grad(xi + h d) - grad(xi - h d)) / 2 of sampler_adjoint.logpost_gradient with data = G(k(xi)):
    lognormal problems, the chain in log k; symmetric and positive definite"""
    prob, projs = _sampler_case(kind, True)
    proj = None if projs is None else projs[level]
    dp, h = _darcy_for(kind)
    rng = np.random.default_rng(97)
    xi = 0.5 * rng.standard_normal(prob.levels[xi_level].n_s)
    k = sampler_adjoint.eval_forward(prob, level, xi_level, xi, proj)
    assert k.size == dp.levels[level].n_p
    Gobs = dcases.two_cell_observations(h, level)
    data = darcy_adjoint.loglik_gradient(dp, level, k, Gobs, np.zeros(2), NOISE)[1]
    cache = {}

    def grad(x):
        return sampler_adjoint.logpost_gradient(prob, dp, level, x, Gobs, data, NOISE, xi_level, proj, cache)[1]

    def H(v):
        return sampler_adjoint.logpost_gn_hessvec(prob, dp, level, xi, v, Gobs, NOISE, xi_level, proj, cache)

    errs = []
    for _ in range(3):
        d = STEP * rng.standard_normal(xi.size)
        fd = -(grad(xi + d) - grad(xi - d)) / 2.0
        errs.append(rel(fd, H(d)))
    v, w = rng.standard_normal(xi.size), rng.standard_normal(xi.size)
    Hv, Hw = H(v), H(w)
    sym = abs(float(w @ Hv) - float(v @ Hw)) / (np.linalg.norm(w) * np.linalg.norm(Hv))
    print(f"{kind} ({level}, {xi_level}): logpost_gn_hessvec max rel err {max(errs):.2e}, symmetry defect {sym:.2e}")
    assert max(errs) < TOL_LP
    assert sym <= TOL_IDENT and float(v @ Hv) > 0.0 and float(w @ Hw) > 0.0


def test_twins_refuse_what_the_library_refuses():
    sp = build_sampler_problem(cases.hierarchy("ragged"), corlen=cases.CORLEN)
    v = np.zeros(sp.levels[0].n_s)
    with pytest.raises(ValueError):
        sampler_adjoint.eval_tangent(sp, 0, 0, v, s_out=v)       # s_out on a Gaussian problem
    with pytest.raises(ValueError):
        sampler_adjoint.eval_tangent(sp, 0, 1, v)                # xi_level coarser than level

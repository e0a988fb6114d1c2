"""The numpy twin of the adjoint of the samplers' Eval (parelagmc_amd/fe/sampler_adjoint.py) against the oracle's direct
solves (oracle/sampler_oracle.py): the adjoint identity for the Gaussian map, central differences for the lognormal chain and
for the log-posterior.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.darcy_oracle import DarcyOracle  # noqa: E402
from oracle.sampler_oracle import SamplerOracle  # noqa: E402
from parelagmc_amd.fe import build_sampler_problem, sampler_adjoint  # noqa: E402

import darcy_gradient_cases as dcases  # noqa: E402
import sampler_adjoint_cases as cases  # noqa: E402

STEP = 1e-5          # xi -> xi +- STEP d
# Largest relative error of a directional derivative measured over all cases below, relative to |g . d| + 1e-3 |g| |d|:
# 2.3e-9 (the sampler's lognormal chain), 6.5e-9 (the log-posterior).  The bound is 100 x that, and never looser than 1e-5.
TOL_CHAIN = min(100 * 2.3e-9, 1e-5)
TOL_LOGPOST = min(100 * 6.5e-9, 1e-5)
LEVELS = [(0, 0), (1, 0), (1, 1)]


def _identity_defect(g, v, xi, adj):
    """|<g, v> - <xi, adj>| / (|g| |v|)"""
    return abs(float(g @ v) - float(xi @ adj)) / (np.linalg.norm(g) * np.linalg.norm(v))


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("mesh", ["ragged", "tet1"])
def test_adjoint_identity_plain(mesh, level, xi_level):
    """<Eval(xi), v> == <xi, EvalAdjoint(v)> for the Gaussian map.  Measured over this file's identity cases: at most
    1.8e-16 |g| |v|."""
    sp = build_sampler_problem(cases.hierarchy(mesh), corlen=cases.CORLEN)
    so = SamplerOracle(sp)
    rng = np.random.default_rng(61)
    xi = rng.standard_normal(sp.levels[xi_level].n_s)
    v = rng.standard_normal(sp.levels[level].n_s)
    g = so.eval_gaussian(level, xi_level, xi)
    adj = sampler_adjoint.eval_adjoint(sp, level, xi_level, v)
    assert adj.shape == xi.shape
    d = _identity_defect(g, v, xi, adj)
    print(f"{mesh} ({level}, {xi_level}): identity defect {d:.2e}")
    assert d <= 1e-12


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("kind", ["gather", "l2"])
def test_adjoint_identity_projected(kind, level, xi_level):
    """the same through the gather and the L2 output map (ragged hierarchy; the L2 map from fe/transfer)"""
    sp, proj = (cases.gather_problem("ragged") if kind == "gather" else cases.l2_problem("ragged")[:2])
    so = SamplerOracle(sp)
    rng = np.random.default_rng(67)
    xi = rng.standard_normal(sp.levels[xi_level].n_s)
    s = so.eval(level, xi_level, xi, projection=proj[level])[0]
    assert s.size != sp.levels[level].n_s                       # the output space is another one
    v = rng.standard_normal(s.size)
    adj = sampler_adjoint.eval_adjoint(sp, level, xi_level, v, projection=proj[level])
    d = _identity_defect(s, v, xi, adj)
    print(f"{kind} ({level}, {xi_level}): identity defect {d:.2e}")
    assert d <= 1e-12
    assert np.allclose(sampler_adjoint.eval_forward(sp, level, xi_level, xi, proj[level]), s, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("mesh", ["ragged", "tet1"])
def test_adjoint_identity_kl(mesh, level, xi_level):
    """the KL twin on the modes of `level`: s = Phi_level Lambda^1/2 xi[:m]; the entries of the gradient behind m vanish"""
    kp = cases.kl_problem(mesh, (3, 3, 3) if mesh == "ragged" else (2, 1, 1))
    m = kp.nmodes
    rng = np.random.default_rng(71)
    xi = rng.standard_normal(kp.levels[xi_level].n_s)
    v = rng.standard_normal(kp.levels[level].n_s)
    g = (np.asarray(kp.evects[level]) * np.sqrt(kp.evals)) @ xi[:m]
    adj = sampler_adjoint.eval_adjoint(kp, level, xi_level, v)
    assert adj.shape == xi.shape and np.all(adj[m:] == 0.0) and np.any(adj[:m] != 0.0)
    assert _identity_defect(g, v, xi, adj) <= 1e-12
    assert np.allclose(sampler_adjoint.eval_forward(kp, level, xi_level, xi), g, rtol=1e-13, atol=0.0)


def _directional_errors(fun, g, xi, rng):
    out = []
    for _ in range(5):
        d = rng.standard_normal(xi.size)
        fd = (fun(xi + STEP * d) - fun(xi - STEP * d)) / 2.0
        gd = float(g @ (STEP * d))
        out.append(abs(fd - gd) / (abs(gd) + 1e-3 * np.linalg.norm(g) * np.linalg.norm(STEP * d)))
    return out


@pytest.mark.parametrize("level,xi_level", LEVELS)
@pytest.mark.parametrize("kind", ["plain-ragged", "plain-tet1", "gather", "l2", "kl"])
def test_lognormal_chain_matches_central_differences_of_the_oracle(kind, level, xi_level):
    """J(xi) = <c, exp(...)>: a missing s_out, a wrong sign of g or a transposed P is an O(1) error here.  Measured: at most
    2.3e-9 over the 15 cases x 5 directions (cube_tet, level 1 from xi on level 0)."""
    rng = np.random.default_rng(73)
    proj = None
    if kind == "kl":
        kp = cases.kl_problem("ragged", lognormal=True)
        Phi = np.asarray(kp.evects[level]) * np.sqrt(kp.evals)
        prob, fun_s = kp, (lambda x: np.exp(Phi @ x[:kp.nmodes]))
    else:
        if kind.startswith("plain"):
            prob = build_sampler_problem(cases.hierarchy(kind.split("-")[1]), corlen=cases.CORLEN, lognormal=True)
        else:
            prob, projs = (cases.gather_problem("ragged", True) if kind == "gather" else cases.l2_problem("ragged", True)[:2])
            proj = projs[level]
        so = SamplerOracle(prob)
        fun_s = lambda x: so.eval(level, xi_level, x, projection=proj)[0]      # noqa: E731
    xi = rng.standard_normal(prob.levels[xi_level].n_s)
    s = fun_s(xi)
    c = rng.standard_normal(s.size)
    g = sampler_adjoint.eval_adjoint(prob, level, xi_level, c, s_out=s, projection=proj)
    errs = _directional_errors(lambda x: float(c @ fun_s(x)), g, xi, rng)
    print(f"{kind} ({level}, {xi_level}): max rel err {max(errs):.2e}")
    assert max(errs) < TOL_CHAIN


@pytest.mark.parametrize("lognormal", [True, False])
@pytest.mark.parametrize("k_divides", [True, False])
def test_logpost_gradient_matches_central_differences_of_the_oracle(k_divides, lognormal):
    """log pi(xi) = loglik(Eval(xi)) - |xi|^2 / 2 from the two oracles and this test's own observation functionals (a Gaussian
    field is shifted to stay positive: k = 3 + 0.2 s).  Measured: at most 6.5e-9."""
    h, dp = dcases.problem("hex4", k_divides, "eff_perm")
    L = dp.levels[0]
    sp = build_sampler_problem(h, corlen=cases.CORLEN, lognormal=lognormal)
    so, orc = SamplerOracle(sp), DarcyOracle(dp)
    Gobs = dcases.two_cell_observations(h)
    norm = 1.0 / np.asarray(Gobs.sum(axis=1)).ravel()
    rng = np.random.default_rng(79)
    noise = 0.01

    def G_of(kk):
        return norm * (Gobs @ orc.solve_fwd(0, kk, return_solution=True)[2][L.n_u:])

    data = G_of(np.exp(0.3 * rng.standard_normal(L.n_p)))        # observations of another field: a nonzero misfit
    xi = rng.standard_normal(sp.levels[0].n_s)
    if lognormal:
        def logpost(x):
            r = G_of(so.eval(0, 0, x)[0]) - data
            return -float(r @ r) / (2.0 * noise) - 0.5 * float(x @ x)
        lp, g = sampler_adjoint.logpost_gradient(sp, dp, 0, xi, Gobs, data, noise)
    else:
        # the Gaussian handle's field is no permeability by itself: the chain through an affine map, composed by hand
        from parelagmc_amd.fe import darcy_adjoint

        def logpost(x):
            r = G_of(3.0 + 0.2 * so.eval(0, 0, x)[0]) - data
            return -float(r @ r) / (2.0 * noise) - 0.5 * float(x @ x)
        k = 3.0 + 0.2 * sampler_adjoint.eval_forward(sp, 0, 0, xi)
        ll, _, gk = darcy_adjoint.loglik_gradient(dp, 0, k, Gobs, data, noise)
        lp, g = ll - 0.5 * float(xi @ xi), -xi + sampler_adjoint.eval_adjoint(sp, 0, 0, 0.2 * gk)
    assert abs(lp - logpost(xi)) <= 1e-10 * abs(lp)
    errs = _directional_errors(logpost, g, xi, rng)
    print(f"logpost k_divides={k_divides} lognormal={lognormal}: max rel err {max(errs):.2e}")
    assert max(errs) < TOL_LOGPOST


def test_twin_refuses_what_the_library_refuses():
    sp = build_sampler_problem(cases.hierarchy("ragged"), corlen=cases.CORLEN)
    v = np.zeros(sp.levels[0].n_s)
    with pytest.raises(ValueError):
        sampler_adjoint.eval_adjoint(sp, 0, 0, v, s_out=v)       # s_out on a Gaussian problem
    with pytest.raises(ValueError):
        sampler_adjoint.eval_adjoint(sp, 0, 1, v)                # xi_level coarser than level

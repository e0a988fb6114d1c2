"""The numpy twin of BayesianInverseProblem::ComputeMAP (parelagmc_amd/fe/map_estimate.py): inexact
Gauss-Newton-CG on lognormal problems with two observations, against scipy's L-BFGS-B as an independent optimiser, and the CG
loop on an explicit matrix against numpy.linalg.solve.  No GPU.

Measured here (printed by the tests): the twin's maximiser against L-BFGS-B (ftol = gtol = 1e-15-class settings, which stops
on its own line search) differs by 6.2e-8, 1.6e-6 and 2.9e-7 relative in the three converging cases (MEASURED_SCIPY; limited by
L-BFGS-B: the twin's two starts agree to 2.2e-6 or better at |g| <= 1e-8 |g0|).  The bound is 100 x that, never looser than
1e-4.  The two starts are compared through the gradient norms they stopped at: with the prior's identity in the Hessian,
|xi_a - xi_b| <= (|g_a| + |g_b|) / mu with mu the smallest eigenvalue of the true Hessian between them; mu >= 1e-3 is
assumed (the Gauss-Newton part is exact only at zero residual), which every case meets with room."""
import numpy as np
import pytest
import scipy.optimize

import map_cases as mc
from parelagmc_amd.fe import map_estimate, sampler_adjoint

MEASURED_SCIPY = 1.6e-6
TOL_SCIPY = min(100 * MEASURED_SCIPY, 1e-4)
TIGHT = dict(max_newton=40, grad_rtol=1e-8)


def _monotone(res):
    for b in range(res["status"].size):
        lp = res["hist_logpost"][:, b]
        lp = lp[np.isfinite(lp)]
        assert np.all(np.diff(lp) >= 0.0), (b, lp)


def _armijo_holds(res, c1=1e-4):
    for b in range(res["status"].size):
        for i in range(int(res["newton_iterations"][b])):
            lp0, lp1 = res["hist_logpost"][i, b], res["hist_logpost"][i + 1, b]
            assert res["hist_t"][i, b] > 0.0
            assert lp1 >= lp0 + c1 * res["hist_t"][i, b] * res["hist_gd"][i, b], (b, i)


@pytest.mark.parametrize("name", ["ragged-00", "ragged-10", "tet1-00"])
def test_converging_cases(name):
    dp, sp, Gobs, level, xi_level, noise, data, n_xi = mc.case(name)
    xi, res = map_estimate.map_estimate(sp, dp, level, mc.starts(name, 2), Gobs, data, noise, xi_level, **TIGHT)
    print(f"{name}: outer iterations {res['newton_iterations']}, Hessian actions {res['hessian_actions']}, "
          f"CG steps per iteration at most {res['hist_cg'].max()}, steps {sorted(set(res['hist_t'][res['hist_t'] > 0]))}")
    assert np.all(res["status"] == map_estimate.CONVERGED)
    assert np.all(res["grad_norm"] <= 1e-8 * res["grad_norm0"])
    assert res["hist_cg"].max() <= 3                     # the identity plus a matrix of rank two
    assert np.all(res["nonpos_curvature"] == 0)
    _monotone(res)
    _armijo_holds(res)
    gap = np.linalg.norm(xi[0] - xi[1])
    print(f"{name}: the two starts differ by {gap / np.linalg.norm(xi[0]):.2e} relative, |g| {res['grad_norm']}")
    assert gap <= 1e3 * res["grad_norm"].sum()
    cache = {}

    def neg(x):
        lp, g = sampler_adjoint.logpost_gradient(sp, dp, level, x, Gobs, data, noise, xi_level, cache=cache)
        return -lp, -g
    ref = scipy.optimize.minimize(neg, np.zeros(n_xi), jac=True, method="L-BFGS-B",
                                  options=dict(maxiter=2000, maxfun=4000, ftol=1e-15, gtol=1e-12, maxcor=30))
    e = np.linalg.norm(xi[0] - ref.x) / np.linalg.norm(ref.x)
    print(f"{name}: against L-BFGS-B ({ref.nit} iterations, logpost {-ref.fun:.12e} vs {res['logpost'][0]:.12e}): {e:.2e}")
    assert e <= TOL_SCIPY
    assert res["logpost"][0] >= -ref.fun - 1e-9 * abs(ref.fun)


def test_backtracking_case():
    """small noise, a far start: steps below 1 occur, and the iteration still converges"""
    name = "tet1-11-small-noise"
    dp, sp, Gobs, level, xi_level, noise, data, n_xi = mc.case(name)
    assert n_xi == 6
    xi, res = map_estimate.map_estimate(sp, dp, level, mc.starts(name, 2, scale=2.0), Gobs, data, noise, xi_level, **TIGHT)
    t = res["hist_t"][res["hist_t"] > 0]
    print(f"{name}: outer iterations {res['newton_iterations']}, steps taken {sorted(set(t))}")
    assert np.any(t < 1.0)
    assert np.all(res["status"] == map_estimate.CONVERGED)
    _monotone(res)
    _armijo_holds(res)
    assert np.all(res["gradient_evaluations"] >= res["newton_iterations"] + 1)


def test_max_newton_status():
    """Gauss-Newton is slow where the residual is large against the noise: 30 iterations do not reach 1e-8"""
    name = "ragged-00-small-noise"
    dp, sp, Gobs, level, xi_level, noise, data, n_xi = mc.case(name)
    xi, res = map_estimate.map_estimate(sp, dp, level, mc.starts(name, 2), Gobs, data, noise, xi_level, max_newton=30,
                                        grad_rtol=1e-8)
    assert np.all(res["status"] == map_estimate.MAX_NEWTON) and np.all(res["newton_iterations"] == 30)
    assert np.all(np.isfinite(res["hist_logpost"]))
    _monotone(res)


def _quadratic(n=65, rank=3, nb=3, seed=107):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, rank))
    H = np.eye(n) + U @ U.T
    rhs = rng.standard_normal((nb, n))
    return H, rhs, rng


def test_cg_columns_against_a_dense_solve():
    """H = I + U U^T, n = 65, rank 3: CG ends after four steps; an inactive column stays zero and counts nothing"""
    H, rhs, rng = _quadratic()
    calls = []

    def hv(P):
        calls.append(P.copy())
        return P @ H
    d, count, npc = map_estimate.cg_columns(hv, rhs, np.full(3, 1e-13), np.array([True, False, True]), 20)
    ref = np.linalg.solve(H, rhs.T).T
    for b in (0, 2):
        assert np.linalg.norm(d[b] - ref[b]) <= 1e-12 * np.linalg.norm(ref[b])
    assert list(count) == [4, 0, 4] and not npc.any() and not d[1].any()
    assert all(not P[1].any() for P in calls)            # the inactive column enters every action as zeros
    # a loose column finishes first and enters the later actions as zeros
    calls.clear()
    d2, count2, _ = map_estimate.cg_columns(hv, rhs, np.array([0.5, 0.5, 1e-13]), np.ones(3, bool), 20)
    assert count2[0] < 4 and count2[2] == 4 and np.array_equal(d2[2], d[2])
    assert not calls[-1][0].any()


def test_newton_cg_on_a_quadratic_with_a_converged_column():
    """logpost = b.x - x.Hx / 2: one full Newton step per column; a column that starts at the solution takes no iteration and
    keeps its bits"""
    H, rhs, rng = _quadratic()
    sol = np.linalg.solve(H, rhs.T).T
    x0 = rng.standard_normal(rhs.shape)
    x0[1] = sol[1]

    def lpg(X):
        return np.einsum("ij,ij->i", rhs, X) - 0.5 * np.einsum("ij,ij->i", X @ H, X), rhs - X @ H
    xi, res = map_estimate.map_newton_cg(lpg, lambda X, V: V @ H, x0, grad_rtol=1e-10, grad_atol=1e-9, max_newton=20)
    assert np.all(res["status"] == map_estimate.CONVERGED)
    assert res["newton_iterations"][1] == 0 and res["hessian_actions"][1] == 0 and np.array_equal(xi[1], sol[1])
    assert res["gradient_evaluations"][1] == 1
    for b in (0, 2):
        assert np.linalg.norm(xi[b] - sol[b]) <= 1e-8 * np.linalg.norm(sol[b])
        assert np.all(res["hist_t"][:res["newton_iterations"][b], b] == 1.0)
    _monotone(res)


def test_non_positive_curvature_takes_the_gradient():
    """a Hessian action that returns -v: every CG run ends at its first step with d = g, the event is counted, and the line
    search still climbs"""
    H, rhs, rng = _quadratic()
    x0 = rng.standard_normal(rhs.shape)

    def lpg(X):
        return np.einsum("ij,ij->i", rhs, X) - 0.5 * np.einsum("ij,ij->i", X @ H, X), rhs - X @ H
    xi, res = map_estimate.map_newton_cg(lpg, lambda X, V: -V, x0, max_newton=4, grad_rtol=1e-12)
    assert np.all(res["status"] == map_estimate.MAX_NEWTON)
    assert np.all(res["nonpos_curvature"] == 4) and np.all(res["hessian_actions"] == 4) and np.all(res["hist_cg"][:4] == 1)
    g0 = rhs - x0 @ H
    assert np.allclose(res["hist_gd"][0], np.einsum("ij,ij->i", g0, g0), rtol=1e-14)     # d = g
    _monotone(res)
    _armijo_holds(res)


def test_options_are_checked():
    H, rhs, _ = _quadratic()
    for bad in (dict(max_newton=0), dict(max_cg=0), dict(max_backtracks=0), dict(eta_max=1.0), dict(c1=0.0),
                dict(grad_rtol=0.0), dict(grad_atol=-1.0)):
        with pytest.raises(ValueError):
            map_estimate.map_newton_cg(lambda X: (np.zeros(len(X)), X), lambda X, V: V, rhs, **bad)
    with pytest.raises(TypeError):
        map_estimate.map_newton_cg(lambda X: (np.zeros(len(X)), X), lambda X, V: V, rhs, tolerance=1.0)

"""The fp64 reference of the MINRES preconditioner (oracle/precond_oracle.py) checked against closed forms and textbook
identities (no GPU needed)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.precond_oracle import (DarcyPrecondOracle, chebyshev, cheb2_coefficients, vcycle, GALERKIN_SCALE,
                                   LMAX_SCHUR)


def _spd(rng, n=40):
    Q = rng.standard_normal((n, n))
    return sp.csr_matrix(Q @ Q.T + n * np.eye(n))


@pytest.mark.parametrize("lmax,ratio", [(1.0, 8.0), (2.0002, 8.0), (1.0, 3.5), (2.0002, 100.0)])
def test_degree_two_polynomial_is_the_closed_form(lmax, ratio):
    """chebyshev(degree 2) = D^-1 (c0 r - c1 A D^-1 r), and (c0, c1) equal the recurrence form of csrc/solver.hpp's
    cheb2_coefficients: c0 = (1 + rho1 rho0) / theta + 2 rho1 / delta, c1 = 2 rho1 / (delta theta)"""
    rng = np.random.default_rng(1)
    A = _spd(rng)
    dinv = 1.0 / A.diagonal()
    r = rng.standard_normal(A.shape[0])
    c0, c1 = cheb2_coefficients(lmax, ratio)
    ref = dinv * (c0 * r - c1 * (A @ (dinv * r)))
    assert np.linalg.norm(chebyshev(A, dinv, r, 2, lmax, ratio) - ref) <= 1e-13 * np.linalg.norm(ref)
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    rho0 = delta / theta
    rho1 = 1.0 / (2.0 * theta / delta - rho0)
    assert c0 == pytest.approx((1.0 + rho1 * rho0) / theta + 2.0 * rho1 / delta, rel=1e-14)
    assert c1 == pytest.approx(2.0 * rho1 / (delta * theta), rel=1e-14)


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 7, 12])
@pytest.mark.parametrize("ratio", [4.0, 8.0, 100.0])
def test_chebyshev_residual_polynomial_is_optimal(degree, ratio):
    """max over [lmax/ratio, lmax] of |1 - l p(l)| = 1 / T_d(sigma), attained at the interval's ends; the guess form
    x0 + p(r - A x0) is the same polynomial on the initial residual"""
    lmax = 2.0002
    lam = np.linspace(lmax / ratio, lmax, 4001)
    A = sp.diags(lam).tocsr()
    one = np.ones_like(lam)
    res = 1.0 - lam * chebyshev(A, one, one, degree, lmax, ratio)
    lmin = lmax / ratio
    sigma = (lmax + lmin) / (lmax - lmin)
    bound = 1.0 / np.cosh(degree * np.arccosh(sigma))
    assert np.max(np.abs(res)) == pytest.approx(bound, rel=1e-9)
    assert abs(res[0]) == pytest.approx(bound, rel=1e-9) and abs(res[-1]) == pytest.approx(bound, rel=1e-9)
    rng = np.random.default_rng(degree)
    x0, r = rng.standard_normal((2, lam.size))
    x = chebyshev(A, one, r, degree, lmax, ratio, x0=x0)
    assert np.allclose(r - A @ x, (1.0 - lam * chebyshev(A, one, one, degree, lmax, ratio)) * (r - A @ x0), atol=1e-13)


@pytest.fixture(scope="module")
def darcy_small(hex_hierarchy_small):
    from parelagmc_amd.fe import build_darcy_problem
    return build_darcy_problem(hex_hierarchy_small, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])


def _matrix(apply, n):
    return np.column_stack([apply(e) for e in np.eye(n)])


def test_vcycle_is_spd_and_a_contraction(darcy_small):
    """on the Darcy Schur hierarchy of hex_hierarchy_small (log-normal k): the reference V-cycle is symmetric positive
    definite and I - V S contracts in the S-norm (spec(V S) in (0, 2))"""
    po = DarcyPrecondOracle(darcy_small)
    k = np.exp(np.random.default_rng(3).standard_normal(darcy_small.levels[0].n_p))
    levels = po.schur_levels(0, k)
    S = levels[0][0].toarray()
    V = _matrix(lambda e: vcycle(levels, e, *po.smooth), S.shape[0])
    assert np.abs(V - V.T).max() <= 1e-12 * np.abs(V).max()
    assert np.linalg.eigvalsh(0.5 * (V + V.T)).min() > 0
    ev = np.linalg.eigvals(V @ S).real
    assert ev.min() > 0 and ev.max() < 2
    # the coarse level is the scaled Galerkin product and diagonally scaled spectra stay under lmax
    S1 = levels[1][0].toarray()
    P = darcy_small.levels[0].P.toarray()
    assert np.allclose(S1, GALERKIN_SCALE * P.T @ S @ P, rtol=0, atol=1e-14 * np.abs(S1).max())
    for Sl, lmax, _ in levels:
        d = Sl.diagonal()
        assert np.abs(np.linalg.eigvalsh(Sl.toarray() / np.sqrt(np.outer(d, d)))).max() <= lmax == LMAX_SCHUR


def test_two_grid_with_exact_coarse_solve_is_the_textbook_formula(darcy_small):
    """two levels, exact coarse solve: I - V S = (I - M S)(I - P S_c^-1 P^T S)(I - M S) with M = p(D^-1 S) D^-1 the
    smoother's matrix"""
    po = DarcyPrecondOracle(darcy_small)
    k = np.exp(0.7 * np.random.default_rng(4).standard_normal(darcy_small.levels[0].n_p))
    levels = po.schur_levels(0, k)[:2]
    S, lmax, Pm = levels[0]
    levels[1] = (levels[1][0], levels[1][1], None)
    Sc = levels[1][0].toarray()
    n = S.shape[0]
    sd, sr, _, _ = po.smooth
    V = _matrix(lambda e: vcycle(levels, e, *po.smooth, coarse_solve=lambda rc: np.linalg.solve(Sc, rc)), n)
    Sd = S.toarray()
    dinv = 1.0 / Sd.diagonal()
    Msm = _matrix(lambda e: chebyshev(S, dinv, e, sd, lmax, sr), n)
    P = Pm.toarray()
    I = np.eye(n)
    E = (I - Msm @ Sd) @ (I - P @ np.linalg.solve(Sc, P.T @ Sd)) @ (I - Msm @ Sd)
    assert np.allclose(I - V @ Sd, E, rtol=0, atol=1e-11)

"""The fp64 reference of the MINRES preconditioner (oracle/precond_oracle.py) checked against closed forms and textbook
identities (no GPU needed)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.precond_oracle import (DarcyPrecondOracle, SamplerPrecondOracle, bottom_exact, bottom_polynomial, chebyshev,
                                   cheb2_coefficients, sampler_schur, vcycle, GALERKIN_SCALE, LMAX_SCHUR)


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


def _aggregate(A):
    """indicator prolongator of a greedy aggregation: each unaggregated row takes its unaggregated neighbours"""
    A = A.tocsr()
    n = A.shape[0]
    agg = -np.ones(n, dtype=np.int64)
    nc = 0
    for i in range(n):
        if agg[i] >= 0:
            continue
        nbrs = A.indices[A.indptr[i]:A.indptr[i + 1]]
        agg[nbrs[agg[nbrs] < 0]] = nc
        agg[i] = nc
        nc += 1
    return sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))


def _gershgorin_lmax(S):
    return float((np.asarray(abs(S).sum(axis=1)).ravel() / S.diagonal()).max()) * 1.0001


@pytest.fixture(scope="module")
def hybrid_small(hex_hierarchy_small):
    from parelagmc_amd.fe import build_hybrid_sampler_problem
    return build_hybrid_sampler_problem(hex_hierarchy_small, corlen=0.3)


def _setup(kind, lmax, roles_wide, roles_narrow=None, smooth_ratio=16.0, scale=1.0, last=(12, 100.0)):
    """pmc_sampler_vcycle_level's dicts for a hand-built hierarchy"""
    roles_narrow = roles_wide if roles_narrow is None else roles_narrow
    return [dict(hierarchy=kind, lmax=l, role_wide=w, role_narrow=q, smooth_degree=2, smooth_ratio=smooth_ratio,
                 galerkin_scale=scale, last_degree=last[0], last_ratio=last[1], ratio_M=0.0, degree_M=0)
            for l, w, q in zip(lmax, roles_wide, roles_narrow)]


def test_two_grid_with_exact_bottom_on_aggregation_is_the_textbook_formula(hybrid_small):
    """two levels over an aggregation P, the bottom an exact solve (bottom_exact):
    I - V H = (I - M H)(I - P H_c^-1 P^T H)(I - M H), M = p(D^-1 H) D^-1 the smoother's matrix on [lmax / 16, lmax]"""
    H = hybrid_small.levels[1].H.tocsr()
    P = _aggregate(H)
    Hc = (P.T @ H @ P).tocsr()
    lmax = _gershgorin_lmax(H)
    levels = [(H, lmax, P, None), (Hc, _gershgorin_lmax(Hc), None, bottom_exact(Hc))]
    n = H.shape[0]
    V = _matrix(lambda e: vcycle(levels, e, 2, 16.0), n)
    Hd = H.toarray()
    Msm = _matrix(lambda e: chebyshev(H, 1.0 / H.diagonal(), e, 2, lmax, 16.0), n)
    I = np.eye(n)
    E = (I - Msm @ Hd) @ (I - P.toarray() @ np.linalg.solve(Hc.toarray(), P.T.toarray() @ Hd)) @ (I - Msm @ Hd)
    assert np.allclose(I - V @ Hd, E, rtol=0, atol=1e-11)
    # the oracle of a hybridized handle runs exactly this cycle (kind 2: S_0 = H, Galerkin below with the exported P)
    class _Prob:
        levels = [hybrid_small.levels[1]]
    po = SamplerPrecondOracle(_Prob, 0, _setup(2, [lmax, levels[1][1]], [0, 2]), [P])
    r = np.random.default_rng(5).standard_normal(n)
    assert np.allclose(po.apply(r), V @ r, rtol=0, atol=1e-12 * np.abs(V @ r).max())


@pytest.mark.parametrize("schur_scale", [1.0, 0.7])
def test_kind0_schur_level_is_the_dense_block_elimination(darcy_small, hex_hierarchy_small, schur_scale):
    """S_l of the caller's levels = the Schur complement of the block matrix [D B^T; B -alpha W] with D = diag(M) /
    schur_scale, by dense elimination of the first block, on every level (each rediscretized, no Galerkin product)"""
    from parelagmc_amd.fe import build_sampler_problem
    sp_ = build_sampler_problem(hex_hierarchy_small, corlen=0.3)
    po = SamplerPrecondOracle(sp_, 0, _setup(0, [2.0] * len(sp_.levels), [0] * len(sp_.levels)),
                              [L.P for L in sp_.levels[:-1]], schur_scale)
    for v, L in enumerate(sp_.levels):
        D = np.diag(L.M.diagonal() / schur_scale)
        Bd = L.B.toarray()
        A = np.block([[D, Bd.T], [Bd, -sp_.alpha * np.diag(L.w_diag)]])
        nu = L.n_u
        elim = A[nu:, nu:] - A[nu:, :nu] @ np.linalg.solve(A[:nu, :nu], A[:nu, nu:])
        S = sampler_schur(L, sp_.alpha, schur_scale).toarray()
        assert np.allclose(S, -elim, rtol=0, atol=1e-13 * np.abs(elim).max())
        assert np.allclose(po.S[v].toarray(), S, rtol=0, atol=0)
        if v + 1 < len(sp_.levels):   # not the Galerkin product of the finer level
            Sg = (L.P.T @ po.S[v] @ L.P).toarray()
            assert not np.allclose(po.S[v + 1].toarray(), Sg)


@pytest.mark.parametrize("narrow", [False, True])
def test_vcycle_on_an_aggregation_hierarchy_is_spd_and_contracting(hybrid_small, narrow):
    """a three-level cycle over greedy aggregations of a hybridized problem's H (kind 2): wide - smoothing down to a
    polynomial bottom on its Gershgorin interval; narrow - ending on level 1 with an exact solve.  V is SPD and
    spec(V H) lies in (0, 2)"""
    H = hybrid_small.levels[0].H.tocsr()
    P0 = _aggregate(H)
    H1 = (P0.T @ H @ P0).tocsr()
    P1 = _aggregate(H1)
    H2 = (P1.T @ H1 @ P1).tocsr()
    d2 = 1.0 / np.sqrt(H2.diagonal())
    ev2 = np.linalg.eigvalsh((H2.toarray() * d2).T * d2)
    lmax = [_gershgorin_lmax(H), _gershgorin_lmax(H1), _gershgorin_lmax(H2)]
    setup = _setup(2, lmax, [0, 0, 1], [0, 2, 3], last=(8, lmax[2] / (0.999 * ev2[0])))
    class _Prob:
        levels = [hybrid_small.levels[0]]
    po = SamplerPrecondOracle(_Prob, 0, setup, [P0, P1])
    assert all(np.allclose(po.S[v].toarray(), Sv.toarray()) for v, Sv in enumerate((H, H1, H2)))
    n = H.shape[0]
    V = _matrix(lambda e: po.apply(e, narrow), n)
    assert np.abs(V - V.T).max() <= 1e-12 * np.abs(V).max()
    assert np.linalg.eigvalsh(0.5 * (V + V.T)).min() > 0
    ev = np.linalg.eigvals(V @ H.toarray()).real
    assert ev.min() > 0 and ev.max() < 2
    # the polynomial bottom's interval contains the spectrum of its level
    assert ev2[-1] <= lmax[2] and ev2[0] >= lmax[2] / setup[2]["last_ratio"]


# ---- internal hierarchies of the Darcy handle (DarcyChainPrecondOracle) ----

@pytest.fixture(scope="module")
def darcy_hybrid_small(hex_hierarchy_small, darcy_small):
    from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
    return darcy_hybrid_level(hex_hierarchy_small.spaces[0], darcy_small.levels[0])


def _chain_setup(kind, nlev, smooth_ratio, scale, degree=2, last=(12, 100.0)):
    """pmc_darcy_vcycle_level's dicts of an internal hierarchy (lmax 1: the Gershgorin bound is folded into D^-1)"""
    return [dict(hierarchy=kind, lmax=1.0, bottom=float(v == nlev - 1), smooth_degree=degree, smooth_ratio=smooth_ratio,
                 last_degree=last[0], last_ratio=last[1], galerkin_scale=scale, ratio_M=4.0, degree_M=2)
            for v in range(nlev)]


def _kappa(dp, k):
    return k if dp.k_divides else 1.0 / k


@pytest.mark.parametrize("degree", [1, 2, 3, 5])
@pytest.mark.parametrize("ratio", [8.0, 16.0])
def test_gershgorin_folded_chebyshev_is_the_scaled_interval(darcy_small, darcy_hybrid_small, degree, ratio):
    """what an internal hierarchy runs - D^-1 / lambda as the diagonal, lmax 1 - is chebyshev(S, 1 / diag S, r, d, lambda,
    ratio), the form the oracle uses; and lambda bounds spec(D^-1 S) on the Schur level and on H(kappa)"""
    from oracle.precond_oracle import gershgorin_lmax
    rng = np.random.default_rng(degree)
    k = np.exp(1.5 * rng.standard_normal(darcy_small.levels[0].n_p))
    for S in (DarcyPrecondOracle(darcy_small).schur(0, k), darcy_hybrid_small.operator(_kappa(darcy_small, k))):
        lam = gershgorin_lmax(S)
        d = S.diagonal()
        dinv = 1.0 / d
        ref = (np.asarray(abs(S).sum(axis=1)).ravel() / d).max() * 1.0001
        assert lam == pytest.approx(ref, rel=1e-15)
        r = rng.standard_normal(S.shape[0])
        a = chebyshev(S, dinv / lam, r, degree, 1.0, ratio)
        b = chebyshev(S, dinv, r, degree, lam, ratio)
        assert np.linalg.norm(a - b) <= 1e-13 * np.linalg.norm(b)
        if degree == 2:   # ... and the one-pass closed form the element-grouped finest level runs
            c0, c1 = cheb2_coefficients(1.0, ratio)
            dl = dinv / lam
            assert np.linalg.norm(dl * (c0 * r - c1 * (S @ (dl * r))) - b) <= 1e-13 * np.linalg.norm(b)


def test_gershgorin_bound_holds_on_every_level_of_an_internal_hierarchy(darcy_small, darcy_hybrid_small):
    """lambda_v >= lambda_max(D^-1 S_v) (eigsh) on every level of both internal hierarchy kinds, for k == 1 and a
    high-contrast k"""
    from scipy.sparse.linalg import eigsh
    from oracle.precond_oracle import DarcyChainPrecondOracle, KIND_HYBRID, KIND_SA, gershgorin_lmax
    n_p = darcy_small.levels[0].n_p
    H1 = darcy_hybrid_small.operator(np.ones(n_p))
    Pa = _aggregate(H1)
    Pb = _aggregate((Pa.T @ H1 @ Pa).tocsr())
    S1 = DarcyPrecondOracle(darcy_small).schur(0, np.ones(n_p))
    Ps = _aggregate(S1)
    Ps = (sp.eye(n_p) - 0.5 * sp.diags(1.0 / S1.diagonal()) @ S1) @ Ps          # a smoothed (non-injection) prolongator
    cases = [(KIND_SA, [Ps.tocsr()], 1.0, None), (KIND_HYBRID, [Pa, Pb], 0.5, darcy_hybrid_small)]
    rng = np.random.default_rng(11)
    for kind, P, s, hl in cases:
        po = DarcyChainPrecondOracle(darcy_small, 0, _chain_setup(kind, len(P) + 1, 8.0, s), P, hl)
        for k in (np.ones(n_p), np.where(rng.random(n_p) < 0.3, 1e3, 1.0)):
            for v, (Sv, lam, _, _) in enumerate(po.levels(k)):
                d = 1.0 / np.sqrt(Sv.diagonal())
                A = (sp.diags(d) @ Sv @ sp.diags(d)).tocsr()
                hi = eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-10)[0]
                assert lam == gershgorin_lmax(Sv) and hi <= lam, (kind, v, hi, lam)
                if v > 0:
                    Sg = s * (P[v - 1].T @ po.operators(k)[v - 1] @ P[v - 1])
                    assert abs(Sv - Sg).max() <= 1e-14 * abs(Sg).max()


def test_element_grouped_cycle_is_the_oracle_vcycle(darcy_small, darcy_hybrid_small):
    """the finest level of a hybridized handle with degree-2 smoothing written out the way Darcy::hybrid_ops sequences it -
    x = p2(H) r;  x += P V_1(P^T (r - H x));  x += p2(H)(r - H x),  p2 the one-pass polynomial with (c0, c1) of
    cheb2_coefficients(1, 2 mg_smooth_ratio) on D^-1 / lambda_0 - equals the oracle's V(1,1) cycle to rounding"""
    from oracle.precond_oracle import DarcyChainPrecondOracle, KIND_HYBRID
    n_p = darcy_small.levels[0].n_p
    H1 = darcy_hybrid_small.operator(np.ones(n_p))
    P0 = _aggregate(H1)
    P1 = _aggregate((P0.T @ H1 @ P0).tocsr())
    ratio = 2 * 8.0
    po = DarcyChainPrecondOracle(darcy_small, 0, _chain_setup(KIND_HYBRID, 3, ratio, 0.5), [P0, P1], darcy_hybrid_small)
    rng = np.random.default_rng(12)
    c0, c1 = cheb2_coefficients(1.0, ratio)
    for k in (np.ones(n_p), np.exp(2.0 * rng.standard_normal(n_p))):
        levels = po.levels(k)
        H, lam0 = levels[0][0], levels[0][1]
        dl = 1.0 / (lam0 * H.diagonal())
        p2 = lambda v: dl * (c0 * v - c1 * (H @ (dl * v)))
        r = rng.standard_normal(H.shape[0])
        x = p2(r)
        x = x + P0 @ vcycle(levels, P0.T @ (r - H @ x), 2, ratio, l=1)
        x = x + p2(r - H @ x)
        ref = po.apply(k, r)
        assert np.linalg.norm(x - ref) <= 1e-13 * np.linalg.norm(ref)


def test_hybrid_chain_with_over_corrected_coarse_levels_is_spd_and_contracting(darcy_small, darcy_hybrid_small):
    """a three-level multiplier hierarchy as the hybridized handle builds it - indicator aggregations, S_{v+1} = 0.5 P^T S_v P,
    smoothing on [lambda_v / 16, lambda_v] - is SPD and spec(V H) lies in (0, 2) for a log-normal kappa"""
    from oracle.precond_oracle import DarcyChainPrecondOracle, KIND_HYBRID
    n_p = darcy_small.levels[0].n_p
    H1 = darcy_hybrid_small.operator(np.ones(n_p))
    P0 = _aggregate(H1)
    P1 = _aggregate((P0.T @ H1 @ P0).tocsr())
    for P in (P0, P1):
        assert np.array_equal(np.diff(P.indptr), np.ones(P.shape[0])) and np.all(P.data == 1.0)
    po = DarcyChainPrecondOracle(darcy_small, 0, _chain_setup(KIND_HYBRID, 3, 16.0, 0.5), [P0, P1], darcy_hybrid_small)
    k = np.exp(np.random.default_rng(13).standard_normal(n_p))
    H = po.operators(k)[0].toarray()
    V = _matrix(lambda e: po.apply(k, e), H.shape[0])
    assert np.abs(V - V.T).max() <= 1e-12 * np.abs(V).max()
    assert np.linalg.eigvalsh(0.5 * (V + V.T)).min() > 0
    ev = np.linalg.eigvals(V @ H).real
    assert ev.min() > 0 and ev.max() < 2


def test_chain_oracle_of_a_saddle_point_handle_keeps_the_m_block(darcy_small):
    """kind 1: the u-rows are DarcyPrecondOracle's M-block polynomial, the p-rows the cycle on S_0(k) of the same level"""
    from oracle.precond_oracle import DarcyChainPrecondOracle, KIND_SA
    L = darcy_small.levels[0]
    S1 = DarcyPrecondOracle(darcy_small).schur(0, np.ones(L.n_p))
    P = _aggregate(S1)
    po = DarcyChainPrecondOracle(darcy_small, 0, _chain_setup(KIND_SA, 2, 8.0, 1.0), [P])
    rng = np.random.default_rng(14)
    k = np.exp(rng.standard_normal(L.n_p))
    r = rng.standard_normal(L.n_u + L.n_p)
    z = po.apply(k, r)
    base = DarcyPrecondOracle(darcy_small)
    assert np.array_equal(z[:L.n_u], base.mblock(0, k, r[:L.n_u], 4.0, 2))
    assert np.array_equal(z[L.n_u:], po.vcycle(k, r[L.n_u:]))
    assert abs(po.operators(k)[0] - base.schur(0, k)).max() == 0.0

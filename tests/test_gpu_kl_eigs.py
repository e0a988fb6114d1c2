"""The matrix-free Matern eigensolver on the device (pmc_kl_matern_apply / pmc_kl_matern_eigs, csrc/kl_eigs.hip) against numpy:
the block product against the dense K @ X, the eigenpairs against the dense host solve (cases, mode counts and gaps:
tests/kl_eigs_cases.py), a size the dense solve cannot reach, and the pairs fed through pmc_sampler_create_kl."""
import ctypes as C
import time

import numpy as np
import pytest

import kl_eigs_cases as cases

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
PMC_ERR_INVALID = -1


def _dense_k(x, w, corlen):
    """K = W^1/2 C W^1/2 with the conventions of fe/kl.py (matern_kernel, unit diagonal of C), distances from differences"""
    from parelagmc_amd.fe.kl import matern_kernel
    d2 = np.zeros((x.shape[0], x.shape[0]))
    for d in range(3):
        diff = x[:, d:d + 1] - x[None, :, d]
        d2 += diff * diff
    Cm = matern_kernel(np.sqrt(d2), corlen, 3)
    np.fill_diagonal(Cm, 1.0)
    sw = np.sqrt(w)
    return sw[:, None] * Cm * sw[None, :]


@pytest.mark.parametrize("name", ["hex16", "cube_tet", "cube_tet_embed"])
def test_block_product_matches_the_dense_product(gpu_ctx, name):
    from parelagmc_amd import capi
    x, w = cases.points(name)
    n = w.size
    K = _dense_k(x, w, 0.1)
    rng = np.random.default_rng(5)
    for ncols in (1, 4, 16, 17, 80):
        X = rng.standard_normal((n, ncols))
        Y = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, X)
        ref = K @ X
        err = (np.abs(Y - ref).max(0) / np.abs(ref).max(0)).max()
        print(f"{name} ncols {ncols}: worst column ||y_dev - y_np||_inf / ||y_np||_inf = {err:.2e}")
        assert err <= 1e-12
        assert np.array_equal(Y, capi.kl_matern_apply(gpu_ctx, x, w, 0.1, X)), "two calls must agree bitwise"
    # the diagonal convention: K e_j has exactly w_j at entry j
    E = np.zeros((n, 16))
    E[np.arange(16), np.arange(16)] = 1.0
    Y = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, E)
    assert np.array_equal(Y[np.arange(16), np.arange(16)], w[:16])
    assert np.abs(Y - K[:, :16]).max() <= 4 * EPS * np.abs(K[:, :16]).max()
    y1 = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, X[:, 0])
    assert y1.shape == (n,) and np.array_equal(y1, capi.kl_matern_apply(gpu_ctx, x, w, 0.1, X[:, :1])[:, 0])


@pytest.mark.parametrize("name,corlen,m", cases.CASE_IDS)
def test_eigenpairs_match_the_dense_solve(gpu_ctx, name, corlen, m):
    from parelagmc_amd import capi
    x, w = cases.points(name)
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, corlen, m, tol=cases.TOL, seed=3)
    print(info)
    assert info["converged"] == 1
    assert info["max_residual_rel"] <= cases.TOL
    assert info["block_products"] >= 1 and info["iterations"] >= 1 and info["seconds"] > 0.0
    cases.check_against_dense(name, corlen, m, lam, V, info["gap_rel"])
    lam2, V2, info2 = capi.kl_matern_eigs(gpu_ctx, x, w, corlen, m, tol=cases.TOL, seed=3)
    assert np.array_equal(lam, lam2) and np.array_equal(V, V2), "same seed, same options: bitwise the same output"
    assert (info2["iterations"], info2["block_products"], info2["max_residual_rel"], info2["gap_rel"]) == \
        (info["iterations"], info["block_products"], info["max_residual_rel"], info["gap_rel"])


def test_degenerate_cut_is_reported_not_refused(gpu_ctx):
    """nmodes = 64 on the uniform cube cuts the pair lambda_64 = lambda_65: gap_rel says so"""
    from parelagmc_amd import capi
    x, w = cases.points("hex16")
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 64, tol=cases.TOL)
    print(info)
    assert info["converged"] == 1 and lam.shape == (64,)
    assert abs(info["gap_rel"]) < 1e-9


def test_size_the_dense_solve_cannot_reach(gpu_ctx):
    """hex 32^3 (n = 32 768), corlen 0.1, m = 64, default options (tol 1e-8).  numpy recomputes K V in row blocks for ALL 64
    columns, never holding more than 1024 x n entries of K; timed on two hosts with 16 CPU threads each, that check took
    13.5 s and 68 s (under the two minutes allowed); it prints its wall time."""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.kl import matern_apply_blocked
    x, w = cases.points("hex32")
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 64)
    print(info)
    assert info["converged"] == 1 and info["max_residual_rel"] <= 1e-8
    t0 = time.time()
    Yv = V * np.sqrt(w)[:, None]
    R = matern_apply_blocked(x, w, 0.1, Yv) - Yv * lam[None, :]
    res = np.sqrt((R * R).sum(0)) / lam[-1]
    orth = np.abs(V.T @ (w[:, None] * V) - np.eye(64)).max()
    print(f"worst ||K y - lambda y|| / lambda_1 = {res.max():.2e}, |V^T W V - I|_max = {orth:.2e}, "
          f"numpy check {time.time() - t0:.1f} s")
    assert res.max() <= 10 * 1e-8
    assert orth <= 1e-10
    assert np.all(np.diff(lam) >= 0.0)


def test_pairs_feed_the_kl_sampler(gpu_ctx):
    """build_kl_sampler_problem(..., eigensolver="device") -> pmc_sampler_create_kl unchanged; Eval is the expansion of the
    returned pairs (bound of tests/test_gpu_kl.py), and the marginal variances match the dense-built sampler's"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_kl_sampler_problem
    h = cases.hierarchy("hex16")
    m = 60
    prob = build_kl_sampler_problem(h, "matern", nmodes=m, corlen=0.1, eigensolver="device", ctx=gpu_ctx, tol=cases.TOL)
    assert prob.nmodes == m and prob.evect0.shape == (4096, m)
    smp = capi.KLSampler(gpu_ctx, prob)
    try:
        xi = np.random.default_rng(2).standard_normal((7, 4096))
        s, emb = smp.Eval(0, xi, want_embed=True)
        z = xi[:, :m] * np.sqrt(prob.evals)[None, :]
        g = z @ prob.evect0.T
        bound = 8.0 * m * EPS * (np.abs(z) @ np.abs(prob.evect0).T)
        assert np.all(np.abs(emb - g) <= bound)
        assert np.array_equal(s, emb)
    finally:
        smp.close()
    lam_d, V_d, _ = cases.dense("hex16", 0.1, m)
    var, var_d = (prob.evect0 ** 2) @ prob.evals, (V_d ** 2) @ lam_d
    verr = np.abs(var - var_d).max() / var_d.max()
    print(f"marginal variances of the device-built against the dense-built sampler: {verr:.2e}")
    assert verr <= 1e-6


def test_failure_paths(gpu_ctx):
    from parelagmc_amd import capi
    x, w = cases.points("cube_tet_embed")
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 24, tol=1e-14, max_iter=1)
    print(info)
    assert info["converged"] == 0 and info["iterations"] == 1 and info["max_residual_rel"] > 0.0
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V)) and np.all(lam > 0.0) and np.all(np.diff(lam) >= 0.0)
    with pytest.raises(capi.PmcError) as e:
        capi.kl_matern_eigs(gpu_ctx, np.ascontiguousarray(x[:, :2]), w, 0.1, 24)
    assert e.value.code == PMC_ERR_INVALID and "dim == 3" in str(e.value)
    for bad in (dict(w=-w), dict(corlen=0.0), dict(nmodes=0), dict(nmodes=500, guard=16)):
        kw = dict(w=w, corlen=0.1, nmodes=24)
        kw.update(bad)
        with pytest.raises(capi.PmcError) as e:
            capi.kl_matern_eigs(gpu_ctx, x, kw["w"], kw["corlen"], kw["nmodes"], guard=kw.get("guard"))
        assert e.value.code == PMC_ERR_INVALID
    xn = x.copy()
    xn[3, 1] = np.nan
    with pytest.raises(capi.PmcError):
        capi.kl_matern_eigs(gpu_ctx, xn, w, 0.1, 24)

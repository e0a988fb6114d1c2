"""The matrix-free Matern eigensolver on the device (csrc/kl_eigs.hip) at every tile count, column-group count and ragged
size the interface admits (ncols <= 512, m + guard <= 512, any n >= 1); tests/test_gpu_kl_eigs.py reaches NT = 1..5, one
column group and four sizes only.

1. Exact arithmetic.  On cases.integer_clusters every entry of K is a small integer (s_i s_j inside a cluster, exactly 0
   across), X holds integers in [-3, 3], so every partial sum is an integer below 2^53 in any order and Y must EQUAL the
   int64 product: a wrong lane, column offset, pad tile or pairing is a wrong entry, not a rounding figure.  The full cross
   product of INT_SIZES x INT_WIDTHS runs; test_the_lists_reach_every_path asserts from the launch formulas of MaternOp that
   it reaches NT = 1..8, 1..4 column groups and both split regimes with a ragged n.
2. Real geometry at the same edges against fp64 numpy (dense K for n <= 4096, matern_apply_blocked above), bound 1e-12 of
   tests/test_gpu_kl_eigs.py, two calls bitwise equal; the diagonal rule on the last 16 rows; translation by 2^20.
3. Eigenpairs with blocks of 2 and 3 column groups (cases.WIDE_CASES) through cases.check_against_dense.
4. b = n, m = n (whole spectrum), n = 1, guard = 0, degree 1 and 2, two seeds.

Every bound is the one the existing files use for the same quantity (kl_eigs_cases.py, test_gpu_kl_eigs.py); the references
are integer arithmetic or numpy / LAPACK in fp64.  Every figure is printed before it is asserted.

Measured on the MI355X (the printed lines):
- exact arithmetic: the 121 cases of all sizes with the widths other than 33 and 64 equal the int64 product entry for
  entry (33 and 64 joined the list after that run, for the coverage assertion);
- block product against fp64 numpy (bound 1e-12): hex 26^3 2.0e-14 at 17 and at 129 columns (the numpy reference of 145
  columns took 4.1 s), columns of K for its last 16 rows 0.54 eps; cube_tet_embed at 96 .. 512 columns 2.0e-15 .. 2.5e-15;
  boxes of 27, 8, 1 and 6 elements at most 3.0e-16; corlen 0.01 3.4e-16, corlen 10 1.6e-14; the translated product is
  bitwise the untranslated one;
- wide eigenpairs (tol 1e-10): 4 .. 9 filters, |lambda - lambda_dense| / lambda_1 at most 9.0e-16, |V^T W V - I|_max at most
  1.1e-15, marginal variances within 2.4e-10, gap_rel equal to the dense one to all printed digits; m = 365 (b = 381)
  takes 0.86 s, of which the Jacobi sweeps on the host are most;
- b = n and m = n: 0 filters, eigenvalues within 9.1e-16 lambda_1, residuals at most 1.2e-15 lambda_1, |V^T W V - I|_max at
  most 1.7e-14;
- guard = 0: 22 filters (it did not converge before the filter interval was moved off theta_m: the numpy twin stood at
  4.8e-5 after 100 filters); degree 1: 75 filters, degree 2: 24; seeds 3 and 4: eigenvalues 8.6e-16 lambda_1 apart.
"""
import time

import numpy as np
import pytest

import kl_eigs_cases as cases

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps

INT_SIZES = [1, 15, 16, 17, 31, 33, 127, 129, 1000, 4100, 17576]
# (groups, NT): 1, 15, 16 -> (1, 1); 17 -> (1, 2); 33 -> (1, 3); 64 -> (1, 4); 96, 112, 128 -> (1, 6), (1, 7), (1, 8);
# 129, 176, 300, 512 -> (2, 5), (2, 6), (3, 7), (4, 8).  33 and 64 are there for NT = 3 and 4 alone.
INT_WIDTHS = [1, 15, 16, 17, 33, 64, 96, 112, 128, 129, 176, 300, 512]


def launch_shape(n, ncols):
    """(groups, nt, jsplit, last row block, last chunk) of the block product.  These formulas MIRROR MaternOp (its
    constructor and apply_t in csrc/kl_eigs.hip: kApWaves = 8 waves of 16 rows, kJc = 32 columns of K per stage,
    kMaxTiles = 8 tiles of 16 columns per group, split over at most 16 workgroup rows while fewer than 256 row blocks);
    they are restated so that the coverage below is asserted, not assumed."""
    bt = (ncols + 15) // 16
    groups = (bt + 7) // 8
    nt = (bt + groups - 1) // groups
    nchunks = (n + 31) // 32
    row_blocks = (n + 127) // 128
    jsplit = max(1, min(16, 256 // row_blocks, nchunks))
    cps = (nchunks + jsplit - 1) // jsplit
    jsplit = (nchunks + cps - 1) // cps
    return groups, nt, jsplit, n % 128, n % 32


def test_the_lists_reach_every_path():
    """a later change of INT_SIZES / INT_WIDTHS cannot silently drop a path"""
    by_width = {c: launch_shape(128, c)[:2] for c in INT_WIDTHS}
    print("ncols -> (groups, NT):", by_width)
    assert {nt for _, nt in by_width.values()} == set(range(1, 9))
    assert {g for g, _ in by_width.values()} == {1, 2, 3, 4}
    assert [by_width[c] for c in (96, 112, 128, 129, 176, 300, 512)] == [(1, 6), (1, 7), (1, 8), (2, 5), (2, 6), (3, 7), (4, 8)]
    # a last group whose final tile lies wholly past bp, and pad columns inside a stored tile
    assert any(g * nt * 16 > (c + 15) // 16 * 16 for c, (g, nt) in by_width.items())
    assert any(c % 16 for c in INT_WIDTHS)
    by_size = {n: launch_shape(n, 16)[2:] for n in INT_SIZES}
    print("n -> (jsplit, n % 128, n % 32):", by_size)
    assert any(js == 1 and r128 and r32 for js, r128, r32 in by_size.values()), "no split, ragged row block and chunk"
    assert any(js > 1 and r128 and r32 for js, r128, r32 in by_size.values()), "split, ragged row block and chunk"
    assert by_size[17576] == (1, 40, 8)
    assert min(INT_SIZES) == 1 and any(n < 16 for n in INT_SIZES) and any(16 < n < 32 for n in INT_SIZES) \
        and any(32 < n < 128 for n in INT_SIZES)


@pytest.mark.parametrize("ncols", INT_WIDTHS)
@pytest.mark.parametrize("n", INT_SIZES)
def test_integer_block_product_is_exact(gpu_ctx, n, ncols):
    from parelagmc_amd import capi
    x, w, cl, s = cases.integer_clusters(n)
    X = cases.integer_block(n, ncols)
    ref = cases.integer_product(cl, s, X)
    assert np.abs(ref).max() < 2 ** 53
    if n >= 4:
        assert np.unique(X, axis=1).shape[1] == ncols, "no two columns alike"
    Y = capi.kl_matern_apply(gpu_ctx, x, w, cases.INT_CORLEN, X.astype(np.float64))
    bad = np.argwhere(Y != ref)
    print(f"n {n} ncols {ncols} (groups, NT, jsplit, n % 128, n % 32) = {launch_shape(n, ncols)}: {bad.shape[0]} wrong entries"
          + (f", first (row, col) {bad[:8].tolist()}" if bad.size else ""))
    assert Y.shape == ref.shape and np.array_equal(Y, ref)


# ---- real geometry --------------------------------------------------------------------------------------------------------
def _product_check(gpu_ctx, tag, x, w, corlen, X, ref):
    from parelagmc_amd import capi
    Y = capi.kl_matern_apply(gpu_ctx, x, w, corlen, X)
    scale = np.abs(ref).max(0)
    assert np.all(scale > 0.0)
    err = (np.abs(Y - ref).max(0) / scale).max()
    print(f"{tag} ncols {X.shape[1]} (groups, NT, jsplit, n % 128, n % 32) = {launch_shape(w.size, X.shape[1])}: "
          f"worst column ||y_dev - y_np||_inf / ||y_np||_inf = {err:.2e}")
    assert err <= 1e-12
    assert np.array_equal(Y, capi.kl_matern_apply(gpu_ctx, x, w, corlen, X)), "two calls must agree bitwise"
    return Y


def test_hex26_block_product_and_ragged_diagonal(gpu_ctx):
    """hex 26^3 (n = 17 576 = 137 * 128 + 40 = 549 * 32 + 8): no column split, ragged last row block and last chunk.  One
    pass of matern_apply_blocked over 129 random columns and the identity columns of the last 16 rows is the reference for
    ncols = 17, 129 and for the diagonal rule; it prints its wall time."""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.kl import matern_apply_blocked
    x, w = cases.points("hex26")
    n = w.size
    assert n == 17576 and launch_shape(n, 17)[2:] == (1, 40, 8)
    X = np.random.default_rng(11).standard_normal((n, 129))
    E = np.zeros((n, 16))
    E[n - 16 + np.arange(16), np.arange(16)] = 1.0
    t0 = time.time()
    ref = matern_apply_blocked(x, w, 0.1, np.hstack([X, E]))
    print(f"numpy reference, 145 columns: {time.time() - t0:.1f} s")
    for ncols in (17, 129):
        _product_check(gpu_ctx, "hex26", x, w, 0.1, X[:, :ncols], ref[:, :ncols])
    Y = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, E)
    assert np.array_equal(Y[n - 16 + np.arange(16), np.arange(16)], w[n - 16:]), "K e_j has exactly w_j at entry j"
    derr = np.abs(Y - ref[:, 129:]).max() / np.abs(ref[:, 129:]).max()
    print(f"hex26 columns of K for the last 16 rows: max error / max entry = {derr / EPS:.2f} eps")
    assert derr <= 4 * EPS


@pytest.mark.parametrize("ncols", [96, 112, 128, 129, 176, 300, 512])
def test_wide_blocks_on_non_uniform_weights(gpu_ctx, ncols):
    x, w = cases.points("cube_tet_embed")
    X = np.random.default_rng(12).standard_normal((w.size, ncols))
    _product_check(gpu_ctx, "cube_tet_embed", x, w, 0.1, X, cases.dense_k(x, w, 0.1) @ X)


def test_ragged_diagonal_on_non_uniform_weights(gpu_ctx):
    """identity columns on the last 16 rows of n = 1624 = 12 * 128 + 88 = 50 * 32 + 24"""
    from parelagmc_amd import capi
    x, w = cases.points("cube_tet_embed")
    n = w.size
    assert n == 1624
    K = cases.dense_k(x, w, 0.1)
    E = np.zeros((n, 16))
    E[n - 16 + np.arange(16), np.arange(16)] = 1.0
    Y = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, E)
    assert np.array_equal(Y[n - 16 + np.arange(16), np.arange(16)], w[n - 16:]), "K e_j has exactly w_j at entry j"
    assert np.abs(Y - K[:, n - 16:]).max() <= 4 * EPS * np.abs(K[:, n - 16:]).max()


@pytest.mark.parametrize("name", ["hex3", "hex2", "hex1", "cube_tet0"])
def test_small_boxes(gpu_ctx, name):
    x, w = cases.points(name)
    assert w.size == {"hex3": 27, "hex2": 8, "hex1": 1, "cube_tet0": 6}[name]
    K = cases.dense_k(x, w, 0.1)
    for ncols in (1, 16, 17):
        X = np.random.default_rng(13).standard_normal((w.size, ncols))
        _product_check(gpu_ctx, name, x, w, 0.1, X, K @ X)


@pytest.mark.parametrize("corlen", [0.01, 10.0])
def test_extreme_correlation_lengths(gpu_ctx, corlen):
    """corlen 0.01: most entries below e^-100; corlen 10: all entries near 1"""
    x, w = cases.points("cube_tet_embed")
    X = np.random.default_rng(14).standard_normal((w.size, 17))
    _product_check(gpu_ctx, f"cube_tet_embed corlen {corlen}", x, w, corlen, X, cases.dense_k(x, w, corlen) @ X)


@pytest.mark.parametrize("ncols", [17, 129])
def test_translation_leaves_the_product_bitwise_unchanged(gpu_ctx, ncols):
    """hex16 centroids are odd multiples of 1/16 and stay exact after adding 2^20; the kernel works from differences"""
    from parelagmc_amd import capi
    x, w = cases.points("hex16")
    xt = x + 2.0 ** 20
    assert np.array_equal(x * 16.0, np.round(x * 16.0)) and np.array_equal(xt - 2.0 ** 20, x)
    X = np.random.default_rng(15).standard_normal((w.size, ncols))
    Y = capi.kl_matern_apply(gpu_ctx, x, w, 0.1, X)
    assert np.array_equal(Y, capi.kl_matern_apply(gpu_ctx, xt, w, 0.1, X))


# ---- eigenpairs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,corlen,m,guard", cases.WIDE_CASES)
def test_wide_eigenpairs_match_the_dense_solve(gpu_ctx, name, corlen, m, guard):
    from parelagmc_amd import capi
    x, w = cases.points(name)
    t0 = time.time()
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, corlen, m, tol=cases.TOL, guard=guard, seed=3)
    print(f"b = {m + guard}, (groups, NT) = {launch_shape(w.size, m + guard)[:2]}, {time.time() - t0:.1f} s:", info)
    assert info["converged"] == 1
    assert info["max_residual_rel"] <= cases.TOL
    cases.check_against_dense(name, corlen, m, lam, V, info["gap_rel"])
    lam2, V2, info2 = capi.kl_matern_eigs(gpu_ctx, x, w, corlen, m, tol=cases.TOL, guard=guard, seed=3)
    assert np.array_equal(lam, lam2) and np.array_equal(V, V2), "same seed, same options: bitwise the same output"
    assert (info2["iterations"], info2["block_products"], info2["max_residual_rel"], info2["gap_rel"]) == \
        (info["iterations"], info["block_products"], info["max_residual_rel"], info["gap_rel"])


@pytest.mark.parametrize("name,corlen,nmodes", cases.SMALL_CASES)
def test_small_problems_and_the_whole_spectrum(gpu_ctx, name, corlen, nmodes):
    """hex4: b = min(76, 64) = n; the others: m = min(60, n) = n"""
    from parelagmc_amd import capi
    x, w = cases.points(name)
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, corlen, nmodes, tol=cases.TOL)
    print(info)
    assert info["converged"] == 1
    assert lam.shape == (min(nmodes, w.size),)
    cases.check_small_against_dense(name, corlen, nmodes, lam, V)


def test_guard_zero(gpu_ctx):
    from parelagmc_amd import capi
    x, w = cases.points("cube_tet_embed")
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 24, tol=cases.TOL, guard=0)
    print(info)
    assert info["converged"] == 1
    assert info["gap_rel"] == 0.0
    cases.check_against_dense("cube_tet_embed", 0.1, 24, lam, V)


@pytest.mark.parametrize("degree", [1, 2])
def test_lowest_filter_degrees(gpu_ctx, degree):
    """degree 1 skips the three-term loop, degree 2 runs one trip of it; default max_iter = 100"""
    from parelagmc_amd import capi
    x, w = cases.points("cube_tet_embed")
    lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 24, tol=cases.TOL, degree=degree)
    print(info)
    assert info["converged"] == 1 and info["iterations"] <= 100
    assert info["block_products"] == 1 + info["iterations"] * degree
    cases.check_against_dense("cube_tet_embed", 0.1, 24, lam, V, info["gap_rel"])


def test_two_seeds_agree_through_the_dense_solve(gpu_ctx):
    from parelagmc_amd import capi
    x, w = cases.points("cube_tet_embed")
    out = []
    for seed in (3, 4):
        lam, V, info = capi.kl_matern_eigs(gpu_ctx, x, w, 0.1, 24, tol=cases.TOL, seed=seed)
        print(seed, info)
        assert info["converged"] == 1
        cases.check_against_dense("cube_tet_embed", 0.1, 24, lam, V, info["gap_rel"])
        out.append((lam, V))
    assert not np.array_equal(out[0][1], out[1][1]), "the seed must reach the start block"
    lam1 = out[0][0][-1]
    print(f"seeds 3 and 4: |lambda_3 - lambda_4| / lambda_1 = {np.abs(out[0][0] - out[1][0]).max() / lam1:.2e}")
    assert np.abs(out[0][0] - out[1][0]).max() / lam1 <= 20 * cases.TOL

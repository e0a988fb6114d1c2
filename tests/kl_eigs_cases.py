"""Cases shared by tests/test_kl_eigs_setup.py (numpy twin) and tests/test_gpu_kl_eigs.py (device): the meshes, mode counts
and checks of the Matern eigenpairs against the dense host solve.

Mode counts.  The truncation must not cut a cluster, or eigenvectors cannot be compared at all; every m below sits at the
largest relative gap (lambda_m - lambda_{m+1}) / lambda_1 of its range in the dense spectrum (fp64 LAPACK, CPU):
  hex 16^3 on [0,2]^3 (n = 4096), range 40..80:   m = 60, gap 0.0314 (corlen 0.1) and 0.0104 (corlen 0.3);
                                                  m = 64 cuts the degenerate pair lambda_64 = lambda_65
  cube_tet refined 3 times (n = 3072), 24..48:    m = 26, gap 0.0284 (corlen 0.1) and 0.0043 (corlen 0.3)
  cube_tet_embed refined once (n = 1624), 24..48: m = 24, gap 0.0221 (corlen 0.1); m = 45, gap 0.0093 (corlen 0.3)
The cube_tet fixture refines into tetrahedra of EQUAL volume (max w / min w = 1 exactly), so on its own it would not test
the W^1/2 scalings; cube_tet_embed (max w / min w = 82.6) is the case with non-uniform w.

Wide blocks (WIDE_CASES, hex 16^3, guard 16 unless stated; the block of b = m + guard columns is padded to bp, a multiple of
16, and multiplied in `groups` column groups of NT tiles of 16).  Largest relative gap of the range, dense spectrum as above:
  corlen 0.1:  m = 120, gap 0.01331, b = 136, bp = 144, 2 x 5      m = 196, gap 0.01148, b = 212, bp = 224, 2 x 7
               m = 284, gap 0.00673, b = 300, bp = 304, 3 x 7      m = 365, gap 0.00443, b = 381, bp = 384, 3 x 8
               m = 120 with guard 56: b = 176 = bp, 2 x 6
  corlen 0.3:  m = 120, gap 0.00297 (m = 139 has 0.00105, barely above MIN_GAP: not used)

Small problems (SMALL_CASES): hex 4^3 with nmodes = 60 has b = min(76, 64) = n; hex 3^3, 2^3, 1^3 and the unrefined cube_tet
(6 tetrahedra) with nmodes = 60 have m = n, the cap, and return the whole spectrum.  The uniform cubes have degenerate
eigenvalues, so check_small_against_dense compares no eigenvector column by column.

integer_clusters: point sets on which every entry of K is a small integer, for exact comparisons of the block product."""
import functools

import numpy as np

from conftest import golden_path

TOL = 1e-10
MIN_GAP = 1e-3
# name -> (corlen, m)
CASES = {
    "hex16": [(0.1, 60), (0.3, 60)],
    "cube_tet": [(0.1, 26), (0.3, 26)],
    "cube_tet_embed": [(0.1, 24), (0.3, 45)],
}
CASE_IDS = [(name, corlen, m) for name, lst in CASES.items() for corlen, m in lst]
# (name, corlen, m, guard)
WIDE_CASES = [("hex16", 0.1, 120, 16), ("hex16", 0.1, 196, 16), ("hex16", 0.1, 284, 16), ("hex16", 0.1, 365, 16),
              ("hex16", 0.1, 120, 56), ("hex16", 0.3, 120, 16)]
# (name, corlen, nmodes): nmodes = 60 throughout, m = min(60, n)
SMALL_CASES = [("hex4", 0.3, 60), ("hex3", 0.3, 60), ("hex2", 0.3, 60), ("hex1", 0.3, 60), ("cube_tet0", 0.3, 60)]
HEX_BOXES = {"hex16": 16, "hex32": 32, "hex26": 26, "hex4": 4, "hex3": 3, "hex2": 2, "hex1": 1}


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if name in HEX_BOXES:
        return build_hierarchy(box_mesh([HEX_BOXES[name]] * 3, [2, 2, 2], "hex"), 0)
    if name == "cube_tet0":
        return build_hierarchy(mesh_from_json(golden_path("meshes", "cube_tet.json")), 0)
    nref = {"cube_tet": 3, "cube_tet_embed": 1}[name]
    h = build_hierarchy(mesh_from_json(golden_path("meshes", name + ".json")), nref)
    assert h.spaces[0].n_s >= 1500
    return h


def points(name):
    from parelagmc_amd.fe.mesh import element_centroids
    sp0 = hierarchy(name).spaces[0]
    return np.ascontiguousarray(element_centroids(sp0.mesh)), np.ascontiguousarray(sp0.vol)


@functools.lru_cache(maxsize=None)
def dense(name, corlen, m):
    """(lambda ascending (m), V, gap_rel) of the dense solve; m + 1 pairs are computed for the gap"""
    from parelagmc_amd.fe.kl import matern_eigs
    lam, V = matern_eigs(hierarchy(name), corlen, m + 1)
    return lam[1:], V[:, 1:], (lam[1] - lam[0]) / lam[-1]


def check_against_dense(name, corlen, m, lam, V, gap_rel=None):
    """the comparisons both solvers must pass; prints every figure before it asserts"""
    _, w = points(name)
    lam_d, V_d, gap_d = dense(name, corlen, m)
    assert gap_d >= MIN_GAP, f"{name} corlen {corlen}: the dense spectrum has gap_rel {gap_d:.2e} at m = {m}"
    lam1 = lam_d[-1]
    err = np.abs(lam - lam_d).max() / lam1
    orth = np.abs(V.T @ (w[:, None] * V) - np.eye(m)).max()
    var, var_d = (V * V) @ lam, (V_d * V_d) @ lam_d
    verr = np.abs(var - var_d).max() / np.abs(var_d).max()
    idx = np.argmax(np.abs(V), axis=0)
    print(f"{name} corlen {corlen} m {m}: dense gap_rel {gap_d:.4e}, |lambda - lambda_dense| / lambda_1 {err:.2e}, "
          f"|V^T W V - I|_max {orth:.2e}, marginal variance rel. error {verr:.2e}"
          + ("" if gap_rel is None else f", gap_rel {gap_rel:.6e}"))
    assert lam.shape == (m,) and V.shape == (w.size, m)
    assert err <= 10 * TOL
    assert orth <= 1e-10
    assert verr <= 1e-6
    assert np.all(np.diff(lam) >= 0.0), "eigenvalues must ascend"
    assert np.all(V[idx, np.arange(m)] > 0.0), "the entry of largest magnitude of every column must be positive"
    if gap_rel is not None:
        assert abs(gap_rel - gap_d) <= 1e-6


@functools.lru_cache(maxsize=None)
def dense_all(name, corlen):
    """(lambda ascending (n), V) of the dense solve, the whole spectrum"""
    from parelagmc_amd.fe.kl import matern_eigs
    h = hierarchy(name)
    return matern_eigs(h, corlen, h.spaces[0].n_s)


def dense_k(x, w, corlen):
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


def check_small_against_dense(name, corlen, nmodes, lam, V):
    """the subspace-independent comparisons for problems with b = n or m = n (degenerate clusters allowed); prints every
    figure before it asserts"""
    x, w = points(name)
    n = w.size
    m = min(nmodes, n)
    lam_d = dense_all(name, corlen)[0][n - m:]
    lam1 = lam_d[-1]
    assert lam.shape == (m,) and V.shape == (n, m)
    err = np.abs(lam - lam_d).max() / lam1
    orth = np.abs(V.T @ (w[:, None] * V) - np.eye(m)).max()
    Yv = V * np.sqrt(w)[:, None]
    R = dense_k(x, w, corlen) @ Yv - Yv * lam[None, :]
    res = np.sqrt((R * R).sum(0)).max() / lam1
    idx = np.argmax(np.abs(V), axis=0)
    print(f"{name} (n = {n}) corlen {corlen} m {m}: |lambda - lambda_dense| / lambda_1 {err:.2e}, |V^T W V - I|_max "
          f"{orth:.2e}, worst ||K y - lambda y|| / lambda_1 {res:.2e}")
    assert err <= 10 * TOL
    assert orth <= 1e-10
    assert res <= 10 * TOL
    assert np.all(np.diff(lam) >= 0.0), "eigenvalues must ascend"
    assert np.all(V[idx, np.arange(m)] > 0.0), "the entry of largest magnitude of every column must be positive"


# ---- exact-arithmetic block product ---------------------------------------------------------------------------------------
INT_CORLEN = 0.125
INT_NMAX = 17576


def integer_clusters(n):
    """(x, w, cl, s): n points, each exactly on one of the four centres (0,0,0), (L,0,0), (0,L,0), (0,0,L) with
    L = 1000 corlen, and weights w_i = s_i^2 with integer s_i in 1..8.  Then kr = 0 < 1e-10 inside a cluster (c = 1 exactly)
    and kr >= 1000 across clusters (exp(-1000) underflows to exactly 0), so K_ij = s_i s_j inside a cluster, 0 across, and
    K_ii = w_i = s_i^2 agrees with that.  Cluster and s are drawn from a fixed Philox stream (point i has the same cluster
    and weight for every n), so they are periodic in nothing; the quadratic residues one might use instead, such as
    (7 i^2 + 3 i) % 4, have period 4."""
    assert 1 <= n <= INT_NMAX
    rng = np.random.Generator(np.random.Philox(20261017))
    cl = rng.integers(0, 4, INT_NMAX)[:n]
    s = rng.integers(1, 9, INT_NMAX)[:n]
    L = 1000.0 * INT_CORLEN
    centres = np.array([[0.0, 0.0, 0.0], [L, 0.0, 0.0], [0.0, L, 0.0], [0.0, 0.0, L]])
    return np.ascontiguousarray(centres[cl]), (s * s).astype(np.float64), cl, s.astype(np.int64)


def integer_block(n, ncols):
    """X (n, ncols) int64 with entries in [-3, 3].  Rows 0..3 of column c hold the base-7 digits of c (minus 3), so no two
    columns are alike once n >= 4 (7^4 > 512); with n < 4 rows there are only 7^n distinct columns and they repeat with
    period 7^n.  The other rows come from a fixed Philox stream."""
    rng = np.random.Generator(np.random.Philox(20261018))
    X = rng.integers(-3, 4, (n, ncols))
    c = np.arange(ncols)
    for r in range(min(n, 4)):
        X[r] = (c // 7 ** r) % 7 - 3
    return X.astype(np.int64)


def integer_product(cl, s, X):
    """K_int @ X in int64 without forming K_int: K_int is s s^T restricted to each cluster"""
    Y = np.zeros_like(X)
    for k in range(4):
        idx = np.flatnonzero(cl == k)
        Y[idx] = s[idx, None] * (s[idx] @ X[idx])[None, :]
    return Y


def integer_k(cl, s):
    """the dense K_int (small n only)"""
    return np.where(cl[:, None] == cl[None, :], s[:, None] * s[None, :], 0)

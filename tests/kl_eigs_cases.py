"""Cases shared by tests/test_kl_eigs_setup.py (numpy twin) and tests/test_gpu_kl_eigs.py (device): the meshes, mode counts
and checks of the Matern eigenpairs against the dense host solve.

Mode counts.  The truncation must not cut a cluster, or eigenvectors cannot be compared at all; every m below sits at the
largest relative gap (lambda_m - lambda_{m+1}) / lambda_1 of its range in the dense spectrum (fp64 LAPACK, CPU):
  hex 16^3 on [0,2]^3 (n = 4096), range 40..80:   m = 60, gap 0.0314 (corlen 0.1) and 0.0104 (corlen 0.3);
                                                  m = 64 cuts the degenerate pair lambda_64 = lambda_65
  cube_tet refined 3 times (n = 3072), 24..48:    m = 26, gap 0.0284 (corlen 0.1) and 0.0043 (corlen 0.3)
  cube_tet_embed refined once (n = 1624), 24..48: m = 24, gap 0.0221 (corlen 0.1); m = 45, gap 0.0093 (corlen 0.3)
The cube_tet fixture refines into tetrahedra of EQUAL volume (max w / min w = 1 exactly), so on its own it would not test
the W^1/2 scalings; cube_tet_embed (max w / min w = 82.6) is the case with non-uniform w."""
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


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if name == "hex16":
        return build_hierarchy(box_mesh([16, 16, 16], [2, 2, 2], "hex"), 0)
    if name == "hex32":
        return build_hierarchy(box_mesh([32, 32, 32], [2, 2, 2], "hex"), 0)
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

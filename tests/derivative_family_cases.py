"""Problems on triangles, quadrilaterals and algebraically agglomerated levels shared by tests/test_derivative_families.py and
the device tests of the derivative stack (tests/test_gpu_darcy_gradient.py, test_gpu_darcy_gn_hessian.py,
test_gpu_sampler_adjoint.py).  No tests here.

    case     levels: n_u / n_p, faces per element (max-min), elements per face (nside)
    tri      L0 2008 / 1312, L1 512 / 328; 3 faces, nside 2 (golden square.json refined once)
    quad     L0 136 / 60, L1 38 / 15; 4 faces, nside 2 (5 x 3 quadrilaterals refined once)
    agg2     L0 864 / 384 (tetrahedra); L1 197 / 41, 12-5 faces; L2 29 / 5, 10-6 faces; nside 2
    agg2s    as agg2, the coarsest prolongator smoothed (smooth_pu = 0.5): L2 29 / 5, 22-15 faces, nside 5
    agg3     L0 6528 / 3072; L1 1630 / 334, 15-4 faces; L2 234 / 37, 19-5 faces; nside 2
    agg3s    as agg3 with smooth_pu = 0.5: L2 234 / 37, 57-10 faces, nside 11

(cube_tet refined twice / three times, agglomerated with sizes (5, 9, 14, 7, 11) and seed 3, the generators' defaults.)
The problems are cached: the tests read them and leave them unchanged."""
import functools
import os

import numpy as np
import scipy.sparse as sp

from parelagmc_amd.fe import (box_mesh, build_darcy_problem, build_hierarchy, build_sampler_problem, build_spaces, mesh_from_json,
                              refine_uniform)
from parelagmc_amd.fe.agglomerate import build_agglomerated_darcy_problem, build_agglomerated_sampler_problem
from parelagmc_amd.fe.problems import DarcyProblem

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BC_2D = ([1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1])
BC_3D = ([0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
NLEVELS_AGG = 3
CORLEN_AGG, CORLEN_TRI = 0.3, 0.1
# both k_divides spread over the cases
K_DIVIDES = {"tri": True, "quad": False, "agg2": False, "agg2s": True, "agg3": True, "agg3s": False}
CASES = tuple(K_DIVIDES)


@functools.lru_cache(maxsize=None)
def hierarchy(case):
    """'tri' / 'quad': the nested two-level hierarchies"""
    if case == "tri":
        return build_hierarchy(mesh_from_json(os.path.join(GOLD, "meshes", "square.json")), 1)
    assert case == "quad"
    return build_hierarchy(box_mesh([5, 3], [1.0, 1.0], "quad"), 1)


@functools.lru_cache(maxsize=None)
def tet_spaces(refinements):
    """cube_tet refined `refinements` times with six boundary attributes by position, as tests/test_gpu_agglomerated.py sets
    them: 1 z=0, 2 y=0, 3 x=1, 4 y=1, 5 x=0, 6 z=1"""
    m = mesh_from_json(os.path.join(GOLD, "meshes", "cube_tet.json"))
    for _ in range(refinements):
        m = refine_uniform(m)[0]
    c = m.verts[m.bdr].mean(axis=1)
    attr = np.zeros(len(m.bdr), np.int32)
    for a, (ax, val) in enumerate([(2, 0.0), (1, 0.0), (0, 1.0), (1, 1.0), (0, 0.0), (2, 1.0)], start=1):
        attr[np.abs(c[:, ax] - val) < 1e-12] = a
    assert attr.min() == 1
    m.bdr_attr = attr
    return build_spaces(m)


@functools.lru_cache(maxsize=None)
def problem(case, k_divides=None, seed=3):
    """DarcyProblem of `case` with NONZERO seeded essential fluxes on every level, as darcy_gradient_cases.problem sets
    them.  k_divides None: the case's own (K_DIVIDES)."""
    kd = K_DIVIDES[case] if k_divides is None else k_divides
    if case in ("tri", "quad"):
        dp = build_darcy_problem(hierarchy(case), *BC_2D, k_divides=kd)
    else:
        dp = build_agglomerated_darcy_problem(tet_spaces(int(case[3])), NLEVELS_AGG, *BC_3D, k_divides=kd,
                                              smooth_pu=0.5 if case.endswith("s") else 0.0)
    rng = np.random.default_rng(seed)
    for L in dp.levels:
        L.ess_data[:] = np.where(L.ess_mask.astype(bool), rng.standard_normal(L.n_u), 0.0)
    return dp


def observations(case, level):
    """two observation functionals on the elements of `level`, the shape of darcy_gradient_cases.two_cell_observations: one
    cell, and a pair of cells - weighted by their volumes on the nested hierarchies, by one on the agglomerated levels
    (they have no volumes)"""
    n = problem(case).levels[level].n_p
    vol = hierarchy(case).spaces[level].vol if case in ("tri", "quad") else np.ones(n)
    a, b, c = n // 3, (2 * n) // 3, (2 * n) // 3 + 1
    return sp.csr_matrix(([vol[a], vol[b], vol[c]], ([0, 1, 1], [a, b, c])), shape=(2, n))


@functools.lru_cache(maxsize=None)
def widened(case, level):
    """A one-level DarcyProblem with the data of `level` of `case` ('tri' / 'quad') and further contributions of value 0.0:
    the middle element also 'contributes' to the diagonal entries of interior free faces of two other elements each - two
    such faces on tri, one on quad, which makes it an element of 5 faces.  Every other element is padded and those faces
    have three sides, so the device takes the general form of both mass kernels (5 is none of the widths 3, 4, 6 of the
    register forms) - on data whose every added product is an exact zero: the general form has to return the bits of the
    fixed form on the original level.  M(k) itself is unchanged."""
    import dataclasses
    L = problem(case).levels[level]
    faces_of = L.B.tocsr()
    e = L.n_p // 2
    own = set(faces_of.indices[faces_of.indptr[e]:faces_of.indptr[e + 1]].tolist())
    sides = np.bincount(faces_of.indices, minlength=L.n_u)
    found = [int(j) for j in range(L.n_u // 2, L.n_u) if sides[j] == 2 and not L.ess_mask[j] and j not in own]
    pat = L.M_pattern.tocsr()
    c_ptr, c_elem, c_val = L.c_ptr.copy(), L.c_elem, L.c_val
    for f in found[:5 - len(own)]:
        p = pat.indptr[f] + int(np.flatnonzero(pat.indices[pat.indptr[f]:pat.indptr[f + 1]] == f)[0])
        at = int(c_ptr[p + 1])                                 # behind the entry's own contributions
        c_ptr[p + 1:] += 1
        c_elem, c_val = np.insert(c_elem, at, e).astype(L.c_elem.dtype), np.insert(c_val, at, 0.0)
    wide = dataclasses.replace(L, c_ptr=c_ptr, c_elem=c_elem, c_val=c_val, P=None)
    return DarcyProblem([wide], 1, problem(case).k_divides)


def structure(level):
    """(n_fe_max, n_fe_min, nside) of a DarcyLevel: faces per element (the padded width of the device's element matrices
    and the smallest count) and the largest number of elements a face belongs to - counted as Darcy::ensure_gradient counts
    them, from the contributions to the diagonal of M"""
    pat = level.M_pattern.tocsr()
    rows = np.repeat(np.arange(level.n_u), np.diff(pat.indptr))
    diag = np.repeat(rows == pat.indices, np.diff(level.c_ptr))
    t_row = np.repeat(rows, np.diff(level.c_ptr))[diag]
    pairs = np.unique(np.stack([level.c_elem[diag], t_row]), axis=1)
    per_elem = np.bincount(pairs[0], minlength=level.n_p)
    per_face = np.bincount(pairs[1], minlength=level.n_u)
    return int(per_elem.max()), int(per_elem.min()), int(per_face.max())


@functools.lru_cache(maxsize=None)
def sampler_problem(kind, lognormal):
    """'agg-unit' / 'agg-nonunit': the agglomerated levels of cube_tet refined twice (variable children per parent, unit or
    non-unit weights in P_s), corlen 0.3; 'tri': the 2-D hierarchy at corlen 0.1 (g = 50.13, another SPDE exponent)"""
    if kind == "tri":
        return build_sampler_problem(hierarchy("tri"), corlen=CORLEN_TRI, lognormal=lognormal)
    return build_agglomerated_sampler_problem(tet_spaces(2), NLEVELS_AGG, corlen=CORLEN_AGG, ps_weights=kind.split("-")[1],
                                              lognormal=lognormal)


SAMPLER_KINDS = ("agg-unit", "agg-nonunit", "tri")


def level_pairs(kind):
    """the (level, xi_level) pairs the derivative tests run"""
    return ((0, 0), (1, 0), (1, 1)) if kind == "tri" else ((0, 0), (1, 0), (2, 0), (2, 2))

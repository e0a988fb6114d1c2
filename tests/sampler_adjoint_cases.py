"""Problems shared by tests/test_sampler_adjoint.py and tests/test_gpu_sampler_adjoint.py (no tests here)."""
import functools
import os

import numpy as np

from parelagmc_amd.fe import (box_mesh, build_hierarchy, build_kl_sampler_problem, build_sampler_problem,
                              l2_projection_hierarchy, mesh_from_json)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORLEN = 0.3


@functools.lru_cache(maxsize=None)
def hierarchy(mesh):
    """'ragged' (5x3x2 hexes refined once: n_s = 240 / 30), 'tet1' / 'tet2' (cube_tet refined once / twice), 'hex842' (8^3 / 4^3 /
    2^3), 'hex84' (8^3 / 4^3), 'hex16' (16^3 / 8^3)"""
    if mesh == "ragged":
        return build_hierarchy(box_mesh([5, 3, 2], [2, 2, 2], "hex"), 1)
    if mesh == "hex842":
        return build_hierarchy(box_mesh([2, 2, 2], [1, 1, 1], "hex"), 2)
    if mesh == "hex84":
        return build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1)
    if mesh == "hex16":
        return build_hierarchy(box_mesh([8, 8, 8], [1, 1, 1], "hex"), 1)
    return build_hierarchy(mesh_from_json(os.path.join(GOLD, "meshes", "cube_tet.json")), {"tet1": 1, "tet2": 2}[mesh])


@functools.lru_cache(maxsize=None)
def embedded_hierarchy(mesh):
    """the enlarged mesh of the gather cases: the original elements (attribute 1) are those with centroid x below 0.6 of its
    extent (no multiple of anything)"""
    if mesh == "ragged":
        m = box_mesh([5, 3, 2], [2, 2, 2], "hex")
        refine = 1
    else:
        m = box_mesh([2, 2, 2], [1, 1, 1], "hex")
        refine = 2
    cen = m.verts[m.elems].mean(1)
    m.elem_attr[:] = np.where(cen[:, 0] < 0.6 * m.verts[:, 0].max(), 1, 2)
    return build_hierarchy(m, refine)


@functools.lru_cache(maxsize=None)
def gather_problem(mesh, lognormal=False):
    """(SamplerProblem on the enlarged mesh, [("gather", idx_l)] per level)"""
    sp = build_sampler_problem(embedded_hierarchy(mesh), corlen=CORLEN, lognormal=lognormal, embedded=True)
    return sp, [("gather", idx) for idx in sp.orig_index]


@functools.lru_cache(maxsize=None)
def l2_problem(mesh, lognormal=False):
    """(SamplerProblem on the enlarged mesh, [("l2", Gt_l, inv_w_l)] per level, the l2_ops list): an original box whose cells do
    not line up with the enlarged mesh's, so that Gt has rows with several entries"""
    if mesh == "ragged":
        he = hierarchy("ragged")
        ho = build_hierarchy(box_mesh([3, 2, 2], [1.2, 2, 2], "hex"), 1)
    else:
        he = hierarchy("hex842")
        ho = build_hierarchy(box_mesh([1, 3, 2], [0.5, 1, 1], "hex"), 2)
    ops = l2_projection_hierarchy(ho, he)
    sp = build_sampler_problem(he, corlen=CORLEN, lognormal=lognormal)
    return sp, [("l2",) + tuple(o) for o in ops], ops


def kl_problem(mesh, nmodes=(3, 3, 3), lognormal=False):
    h = hierarchy(mesh)
    return build_kl_sampler_problem(h, "analytic", nmodes=list(nmodes), corlen=CORLEN, lognormal=lognormal)

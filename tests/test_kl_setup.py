"""Setup of the Karhunen-Loeve sampler (parelagmc_amd/fe/kl.py) against the reference's algebra (no GPU):
AnalyticExponentialCovariance (computeOmega's bisection, 1D eigenpairs, i-major tensor products), MaternCovariance (dense
generalised eigenproblem A v = lambda W v, ascending), and KLSampler::BuildHierarchy's projection Phi_{l+1} = D^-1 P^T W Phi_l."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from parelagmc_amd.fe import box_mesh, build_hierarchy, kuhn_cube_tet, refine_uniform
from parelagmc_amd.fe.kl import (OMEGA_TOL, analytic_exponential_eigs, build_kl_sampler_problem, compute_omega,
                                 kl_projector, matern_covariance, matern_eigs, omega_brackets, project_kl_levels)


def _residual(x, lt):
    return math.tan(x) - 2.0 * lt * x / (lt * lt * x * x - 1.0)


@pytest.mark.parametrize("lt", [0.05, 0.3, 0.9, 2.0])
def test_omega_lies_in_its_bracket_and_solves_the_transcendental_equation(lt):
    om = compute_omega(25, lt)
    br = omega_brackets(25, lt)
    for j, w in enumerate(om):
        xl, xr = 1.001 * br[j], 0.999 * br[j + 1]
        assert xl <= w <= xr
        if _residual(xl, lt) * _residual(xr, lt) < 0:
            assert abs(_residual(w, lt)) <= OMEGA_TOL
        else:
            # no sign change between the bracket ends (next to the spliced asymptote the root can lie beyond 0.999 x_{j+1}):
            # the reference's bisection then moves its left end up to the right one and stops after maxit - restated as is
            assert w == pytest.approx(xr, rel=1e-12)
    assert np.all(np.diff(om) > 0)
    # the asymptote 1/l~ is one of the bracket ends whenever it falls inside the covered range
    if 1.0 / lt < br[-1]:
        assert np.any(np.isclose(br, 1.0 / lt, rtol=0, atol=0))


def test_tensor_modes_are_i_major_products_of_the_1d_pairs():
    """hand-worked 2 x 2 x 2 case on a box with three different axis lengths"""
    L = [1.0, 2.0, 0.5]
    corlen = 0.4
    h = build_hierarchy(box_mesh([6, 5, 4], L, "hex"), 0)
    lam, phi = analytic_exponential_eigs(h, [2, 2, 2], L, corlen)
    x = h.spaces[0].mesh.verts[h.spaces[0].mesh.elems].mean(axis=1)
    vol = h.spaces[0].vol
    ev, fn = [], []
    for d in range(3):
        lt = corlen / L[d]
        om = compute_omega(2, lt)
        ev.append([2.0 * L[d] * lt / (lt * lt * w * w + 1.0) for w in om])
        fn.append([(np.sin(x[:, d] * w / L[d]) + lt * w * np.cos(x[:, d] * w / L[d])) / L[d] for w in om])
    k = 0
    for i in range(2):
        for j in range(2):
            for l in range(2):
                assert lam[k] == pytest.approx(ev[0][i] * ev[1][j] * ev[2][l], rel=1e-14)
                v = fn[0][i] * fn[1][j] * fn[2][l]
                v = v / math.sqrt(np.sum(vol * v * v))
                assert np.allclose(phi[:, k], v, rtol=0, atol=1e-12 * np.abs(v).max())
                k += 1
    assert not np.all(np.diff(lam) <= 0), "the order is the loop order, not sorted by eigenvalue"


@pytest.mark.parametrize("mesh", ["quad", "hex"])
def test_analytic_columns_are_p0_mass_normalised(mesh):
    if mesh == "quad":
        h = build_hierarchy(box_mesh([12, 8], [1.5, 1.0], "quad"), 0)
        nm, L = [4, 3], [1.5, 1.0]
    else:
        h = build_hierarchy(box_mesh([6, 6, 6], [2, 2, 2], "hex"), 0)
        nm, L = [3, 4, 2], [2.0, 2.0, 2.0]
    lam, phi = analytic_exponential_eigs(h, nm, L, 0.3)
    assert lam.shape == (int(np.prod(nm)),) and phi.shape == (h.spaces[0].n_s, lam.size)
    assert np.all(lam > 0)
    assert np.allclose(np.einsum("i,ik,ik->k", h.spaces[0].vol, phi, phi), 1.0, rtol=0, atol=1e-13)


def test_the_1d_eigenvalues_sum_to_the_trace_of_the_kernel():
    """sum_k lambda_k -> int_0^L C(x, x) dx = L for the exponential kernel; the tail after N modes is ~ 2 L / (l~ pi^2 N)"""
    for L, corlen in ((1.0, 0.5), (3.0, 0.6)):
        lt = corlen / L
        om = compute_omega(3000, lt)
        lam = 2.0 * L * lt / (lt * lt * om * om + 1.0)
        tail = 2.0 * L / (lt * math.pi ** 2 * om.size)
        assert abs(lam.sum() + tail - L) < 0.1 * tail


def test_analytic_refuses_more_modes_than_elements():
    h = build_hierarchy(box_mesh([3, 3], [1, 1], "quad"), 0)
    with pytest.raises(ValueError):
        analytic_exponential_eigs(h, [4, 3], [1, 1], 0.2)


def _matern_meshes():
    return {"inline_quad": build_hierarchy(box_mesh([12, 10], [1.0, 1.0], "quad"), 0),
            "hex": build_hierarchy(box_mesh([6, 6, 6], [2, 2, 2], "hex"), 0),
            "tet": build_hierarchy(refine_uniform(kuhn_cube_tet())[0], 0)}


@pytest.mark.parametrize("mesh", ["inline_quad", "hex", "tet"])
def test_matern_solves_the_generalised_problem_in_ascending_order(mesh):
    h = _matern_meshes()[mesh]
    w = h.spaces[0].vol
    A = matern_covariance(h, 0.2) * w[:, None] * w[None, :]
    lam, V = matern_eigs(h, 0.2, 30)
    assert lam.shape == (30,) and V.shape == (h.spaces[0].n_s, 30)
    assert np.linalg.norm(A @ V - (w[:, None] * V) * lam[None, :]) <= 1e-10 * np.linalg.norm(A)
    assert np.allclose(V.T @ (w[:, None] * V), np.eye(30), rtol=0, atol=1e-10)
    assert np.all(np.diff(lam) >= 0) and lam[0] > 0
    # the top 30 of the whole spectrum
    full = np.linalg.eigvalsh(A / np.sqrt(w)[:, None] / np.sqrt(w)[None, :])
    assert np.allclose(lam, full[-30:], rtol=1e-9)


@pytest.mark.parametrize("mesh", ["inline_quad", "hex", "tet"])
def test_matern_with_every_mode_reproduces_the_covariance(mesh):
    h = _matern_meshes()[mesh]
    n = h.spaces[0].n_s
    assert n <= 512
    C = matern_covariance(h, 0.2)
    lam, V = matern_eigs(h, 0.2, 10 ** 6)     # capped at NE
    assert lam.size == n
    assert np.abs(V @ np.diag(lam) @ V.T - C).max() <= 1e-10


def test_matern_kernel_known_values():
    from parelagmc_amd.fe.kl import matern_kernel
    import scipy.special
    r = np.array([0.0, 1e-13, 0.1, 0.35])
    assert np.allclose(matern_kernel(r, 0.2, 3), [1.0, 1.0, math.exp(-0.5), math.exp(-1.75)], rtol=1e-15)
    t = math.sqrt(2.0) * 0.5
    assert matern_kernel(np.array([0.1]), 0.2, 2)[0] == pytest.approx(t * scipy.special.k1(t), rel=1e-15)


def test_projection_reproduces_a_coarse_field_and_keeps_weighted_sums():
    h = build_hierarchy(box_mesh([3, 2, 2], [1.5, 1.0, 1.0], "hex"), 2)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((h.spaces[1].n_s, 7))
    phi = project_kl_levels(h, h.P[0] @ X)
    assert np.abs(phi[1] - X).max() <= 1e-14 * np.abs(X).max()
    Y = rng.standard_normal((h.spaces[0].n_s, 7))
    phi = project_kl_levels(h, Y)
    assert len(phi) == 3
    for lvl in range(3):
        assert phi[lvl].shape == (h.spaces[lvl].n_s, 7)
        assert np.allclose(h.spaces[lvl].vol @ phi[lvl], h.spaces[0].vol @ Y, rtol=1e-13, atol=1e-13)


def test_projector_refuses_overlapping_agglomerates():
    P = sp.csr_matrix(np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]]))
    with pytest.raises(ValueError):
        kl_projector(P, np.ones(3))


def test_problem_levels_stop_where_the_modes_exceed_the_elements():
    h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 2)      # 4096 / 512 / 64 elements
    p = build_kl_sampler_problem(h, "analytic", nmodes=[5, 5, 5], corlen=0.1)
    assert p.nmodes == 125 and p.n_mc_levels == 2 and len(p.levels) == 2
    assert p.levels[0].P is h.P[0] and p.levels[1].P is None
    p = build_kl_sampler_problem(h, "analytic", corlen=0.1)            # the CreateSamplerParameterList default, 4 x 4 x 4
    assert p.nmodes == 64 and p.n_mc_levels == 3
    assert [e.shape for e in p.evects] == [(4096, 64), (512, 64), (64, 64)]
    with pytest.raises(ValueError):
        build_kl_sampler_problem(h, "exponential")

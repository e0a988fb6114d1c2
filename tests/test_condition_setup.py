"""Conditioning on observed field values: the setup algebra and the numpy twin (parelagmc_amd/fe/condition.py) against the
CPU oracle's direct solves, and the new entry points of libpmc.so.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

CORLEN = 0.5


@pytest.fixture(scope="module")
def ragged_hierarchy():
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    return build_hierarchy(box_mesh([5, 3, 2], [2, 2, 2], "hex"), 1)     # n_s = 240 / 30


def _observations(h, nobs, seed, averaging=False):
    """unit rows on fine elements with distinct coarsest ancestors (the last one an average over its 8 siblings' parent
    when `averaging`) and data y"""
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    elems = pick_observation_elements(h, nobs, seed)
    extra = []
    if averaging:
        # replace the last point value by the mean of the fine elements sharing its level-1 parent
        parent = sp.csr_matrix(h.P[0]).indices
        sib = np.nonzero(parent == parent[elems[-1]])[0]
        extra = [(sib, np.full(sib.size, 1.0 / sib.size))]
        elems = elems[:-1]
    H0 = point_observations(h.spaces[0].n_s, elems, extra)
    y = np.random.default_rng(seed + 100).normal(0.0, 1.0, H0.shape[0])
    return H0, y


def _dense_schur_K(oracle, problem, level, H):
    """g^2 S^-1 W S^-1 H^T with the dense Schur complement S = alpha W + B M^-1 B^T of the oracle's block operator"""
    L = problem.levels[level]
    A = oracle.block_operator(level).toarray()
    M, Bt, B = A[:L.n_u, :L.n_u], A[:L.n_u, L.n_u:], A[L.n_u:, :L.n_u]
    S = -A[L.n_u:, L.n_u:] + B @ np.linalg.solve(M, Bt)
    Sinv = np.linalg.inv(S)
    return problem.matern_g ** 2 * Sinv @ (L.w_diag[:, None] * (Sinv @ H.T.toarray()))


@pytest.mark.parametrize("mesh,nobs", [("hex", 1), ("hex", 5), ("hex", 16), ("hex", 33), ("hex", 64),
                                       ("ragged", 1), ("ragged", 5), ("ragged", 30)])
def test_twin_against_the_oracle(hex_hierarchy, ragged_hierarchy, mesh, nobs):
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd.fe import build_sampler_problem
    from parelagmc_amd.fe.condition import Conditioner
    h = hex_hierarchy if mesh == "hex" else ragged_hierarchy
    prob = build_sampler_problem(h, corlen=CORLEN)
    H0, y = _observations(h, nobs, seed=nobs, averaging=(nobs == 5))
    twin = Conditioner(prob, H0, y)
    oracle = SamplerOracle(prob)
    last = prob.n_mc_levels - 1
    Kref = _dense_schur_K(oracle, prob, last, twin.H[last])
    err = np.max(np.abs(twin.K[last] - Kref)) / np.max(np.abs(Kref))
    conds = [np.linalg.cond(A) for A in twin.A]
    print(f"[{mesh} nobs {nobs}] K vs dense Schur {err:.2e}; cond(A_l) {['%.2e' % c for c in conds]}")
    assert err <= 1e-11
    xi = np.random.default_rng(7).standard_normal((3, prob.levels[0].n_s))
    for lvl in range(prob.n_mc_levels):
        g = np.stack([oracle.eval_gaussian(lvl, 0, x) for x in xi])     # xi drawn on level 0, evaluated on every level
        gc = twin.apply(lvl, g)
        miss = np.max(np.abs((twin.H[lvl] @ gc.T).T - y[None, :]))
        print(f"    level {lvl}: max |H g_c - y| {miss:.2e}")
        assert miss <= 1e-12
        assert np.allclose(twin.apply(lvl, g, exp=True), np.exp(gc), rtol=0, atol=0)


def test_twin_on_the_hybridized_problem_matches_the_saddle_point_one(hex_hierarchy):
    """the two formulations solve the same system: the same K_l and A_l"""
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    from parelagmc_amd.fe.condition import Conditioner
    H0, y = _observations(hex_hierarchy, 16, seed=16)
    a = Conditioner(build_sampler_problem(hex_hierarchy, corlen=CORLEN), H0, y)
    b = Conditioner(build_hybrid_sampler_problem(hex_hierarchy, corlen=CORLEN), H0, y)
    for lvl in range(3):
        assert np.max(np.abs(a.K[lvl] - b.K[lvl])) <= 1e-10 * np.max(np.abs(a.K[lvl]))


@pytest.mark.parametrize("noise", [False, True])
def test_affine_map_reproduces_the_posterior_covariance(hex_hierarchy, noise):
    """(I - G H) C (I - G H)^T + G R G^T = C - K A^-1 K^T with G = K A^-1, dense on the 64-element level"""
    from parelagmc_amd.fe import build_sampler_problem
    from parelagmc_amd.fe.condition import Conditioner
    prob = build_sampler_problem(hex_hierarchy, corlen=CORLEN)
    H0, y = _observations(hex_hierarchy, 16, seed=16, averaging=True)
    sigma2 = np.random.default_rng(3).uniform(0.01, 0.2, 16) if noise else None
    twin = Conditioner(prob, H0, y, sigma2)
    lvl = 2
    C = twin.covariance(lvl)
    G, H = twin.gain(lvl), twin.H[lvl].toarray()
    R = np.diag(sigma2) if noise else np.zeros((16, 16))
    T = np.eye(C.shape[0]) - G @ H
    lhs = T @ C @ T.T + G @ R @ G.T
    rhs = C - twin.K[lvl] @ np.linalg.solve(twin.A[lvl], twin.K[lvl].T)
    err = np.linalg.norm(lhs - rhs) / np.linalg.norm(C)
    print(f"[noise {noise}] posterior covariance identity {err:.2e}")
    assert err <= 1e-11
    if noise:     # zeta is required iff some sigma2 > 0
        g = np.zeros((2, C.shape[0]))
        with pytest.raises(ValueError):
            twin.apply(lvl, g)
        twin.apply(lvl, g, zeta=np.zeros((2, 16)))


def test_duplicate_coarse_ancestors(hex_hierarchy):
    """two exact observations inside one coarse element make A of that level singular: an error naming the level; the same
    set with noise is accepted"""
    from parelagmc_amd.fe import build_sampler_problem
    from parelagmc_amd.fe.condition import Conditioner, point_observations
    prob = build_sampler_problem(hex_hierarchy, corlen=CORLEN)
    parent = sp.csr_matrix(hex_hierarchy.P[0]).indices
    grand = sp.csr_matrix(hex_hierarchy.P[1]).indices[parent]
    e0 = 0
    e1 = int(np.nonzero((grand == grand[e0]) & (parent != parent[e0]))[0][0])     # same level-2 element, other level-1 element
    H0 = point_observations(prob.levels[0].n_s, [e0, e1, 4000])
    y = np.array([0.3, -0.2, 0.1])
    with pytest.raises(ValueError, match="level 2"):
        Conditioner(prob, H0, y)
    twin = Conditioner(prob, H0, y, sigma2=np.full(3, 0.05))
    assert len(twin.A) == 3
    for bad in (dict(y=[0.0, np.nan, 0.0]), dict(sigma2=[0.1, -0.1, 0.1]), dict(H0=sp.csr_matrix((3, 4096)))):
        args = dict(H0=H0, y=y, sigma2=None)
        args.update(bad)
        with pytest.raises(ValueError):
            Conditioner(prob, args["H0"], args["y"], args["sigma2"])


def test_library_exports_the_conditioner():
    import ctypes
    from parelagmc_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("pmc_conditioner_create", "pmc_conditioner_destroy", "pmc_conditioner_num_obs", "pmc_conditioner_level",
                 "pmc_conditioner_apply", "pmc_sampler_set_conditioner"):
        assert hasattr(lib, name), f"libpmc.so does not export {name}"
        assert name in capi.SYMBOLS

"""tests/layout_cases.py against itself and the oracles (CPU): a re-laid problem holds the same matrices and the same M(k),
the direct-solve oracles return the same bits for it - they do not care about the layout, only the device library can - and
a renumbered problem is the same problem under other names.  The device side: tests/test_gpu_input_layouts.py."""
import dataclasses

import numpy as np
import pytest

import layout_cases as lc
from oracle.darcy_oracle import DarcyOracle
from oracle.sampler_oracle import SamplerOracle

KINDS = ("sampler", "hybrid", "darcy", "darcy-agg2", "elements")
SEED = 11


@pytest.fixture(scope="module")
def problems(hex_hierarchy_small):
    import derivative_family_cases as dfc
    from parelagmc_amd.fe import build_darcy_problem, build_hybrid_sampler_problem, build_sampler_problem
    h = hex_hierarchy_small
    sp_ = build_sampler_problem(h, corlen=0.1, lognormal=True)
    return {"sampler": sp_, "hybrid": build_hybrid_sampler_problem(h, corlen=0.1, lognormal=True),
            "darcy": build_darcy_problem(h, *dfc.BC_3D), "darcy-agg2": dfc.problem("agg2"),
            "elements": lc.hybrid_elements(h.spaces[0], sp_.alpha, h.P[0])}


@pytest.mark.parametrize("layout", lc.LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_relaid_members_are_the_same_matrices(problems, kind, layout):
    p = problems[kind]
    q = lc.relayout_problem(p, layout, SEED)
    padded = 0
    for (l, name, A), (_, _, A2) in zip(lc.csr_members(p), lc.csr_members(q)):
        assert A.has_sorted_indices and A2.shape == A.shape
        assert (A != A2).nnz == 0, (kind, layout, l, name)
        added = lc.zeros_added(p, name, A) if layout == "zeros" else 0
        if added:
            assert A2.nnz == A.nnz + added and np.count_nonzero(A2.data == 0.0) >= added
            padded += 1
        else:
            assert A2.nnz == A.nnz
        if np.diff(A2.indptr).max() >= 2:
            assert not A2.has_sorted_indices, (kind, layout, l, name)
        if layout == "diag_first" and A.shape[0] == A.shape[1]:
            assert np.array_equal(A2.indices[A2.indptr[:-1]], np.arange(A.shape[0])), "the diagonal entry comes first"
    assert (padded > 0) == (layout == "zeros")
    # a relayout leaves the caller's problem alone
    assert all(A.has_sorted_indices for _, _, A in lc.csr_members(p))


@pytest.mark.parametrize("layout", lc.LAYOUTS)
@pytest.mark.parametrize("kind", ("darcy", "darcy-agg2"))
def test_relaid_lists_assemble_the_same_mass_matrix(problems, kind, layout):
    """M(k) from the moved lists = the canonical one exactly (the order inside a list is kept, so each sum has the same
    bits), for a random k; a stored zero of the pattern has an empty list"""
    p = problems[kind]
    q = lc.relayout_problem(p, layout, SEED)
    rng = np.random.default_rng(5)
    for lvl, (L, L2) in enumerate(zip(p.levels, q.levels)):
        k = np.exp(rng.standard_normal(L.n_p))
        M, M2 = DarcyOracle(p).mass(lvl, k), DarcyOracle(q).mass(lvl, k)
        assert (M != M2).nnz == 0 and abs(M - M2).max() == 0.0
        assert len(L2.c_ptr) == L2.M_pattern.nnz + 1 and L2.c_ptr[-1] == len(L2.c_elem) == len(L.c_elem)
        if layout == "zeros":
            assert np.count_nonzero(np.diff(L2.c_ptr) == 0) == lc.zeros_added(p, "M_pattern", L.M_pattern)
        A, rhs = DarcyOracle(p).assemble(lvl, k)
        A2, rhs2 = DarcyOracle(q).assemble(lvl, k)
        assert abs(A - A2).max() == 0.0 and np.array_equal(rhs, rhs2)


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_oracles_return_the_same_bits_for_a_relaid_problem(problems, layout):
    """bit for bit under another order of the entries.  Stored zeros are structural nonzeros to the sparse LU - other
    fill, other pivots - so under `zeros` the results agree as those of a renumbered problem do: to 1e-12 relative."""
    same = np.array_equal if layout != "zeros" else (lambda a, b: np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(a))
    rng = np.random.default_rng(6)
    sp_, dp = problems["sampler"], problems["darcy"]
    sq, dq = lc.relayout_problem(sp_, layout, SEED), lc.relayout_problem(dp, layout, SEED)
    xi = rng.standard_normal(sp_.levels[0].n_s)
    for lvl in (0, 1):
        s, g = SamplerOracle(sp_).eval(lvl, 0, xi)
        s2, g2 = SamplerOracle(sq).eval(lvl, 0, xi)
        assert same(s, s2) and same(g, g2)
        Q, _, x = DarcyOracle(dp).solve_fwd(lvl, s, return_solution=True)
        Q2, _, x2 = DarcyOracle(dq).solve_fwd(lvl, s, return_solution=True)
        assert same(np.array([Q]), np.array([Q2])) and same(x, x2)


def test_oracles_of_a_renumbered_problem_return_the_permuted_result(problems):
    """to 1e-12 relative: the direct solve sees another ordering"""
    rng = np.random.default_rng(7)
    sp_, dp = problems["sampler"], problems["darcy"]
    (sq, sperm), (dq, dperm) = lc.renumber_problem(sp_, SEED), lc.renumber_problem(dp, SEED + 1)
    assert all(A.has_sorted_indices for _, _, A in lc.csr_members(sq) + lc.csr_members(dq))
    xi = rng.standard_normal(sp_.levels[0].n_s)
    for lvl in (0, 1):
        s = SamplerOracle(sp_).eval(lvl, 0, xi)[0]
        s2 = SamplerOracle(sq).eval(lvl, 0, xi[sperm[0][0]])[0]
        assert np.linalg.norm(s2 - s[sperm[lvl][0]]) <= 1e-12 * np.linalg.norm(s)
        L = dp.levels[lvl]
        ps, pu = dperm[lvl]
        Q, _, x = DarcyOracle(dp).solve_fwd(lvl, s, return_solution=True)
        Q2, _, x2 = DarcyOracle(dq).solve_fwd(lvl, s[ps], return_solution=True)
        assert abs(Q2 - Q) <= 1e-12 * abs(Q)
        xp = np.concatenate([x[:L.n_u][pu], x[L.n_u:][ps]])
        assert np.linalg.norm(x2 - xp) <= 1e-12 * np.linalg.norm(x)
    # the hybridized sampler problem: H lambda = G f, s = z f - G^T lambda gives the permuted field
    import scipy.sparse.linalg as spla
    hp = problems["hybrid"]
    hq, hperm = lc.renumber_problem(hp, SEED + 2)
    f = rng.standard_normal(hp.levels[0].n_s)
    field = lambda L, f: L.z_diag * f - L.G.T @ spla.splu(L.H.tocsc()).solve(L.G @ f)
    s, s2 = field(hp.levels[0], f), field(hq.levels[0], f[hperm[0][0]])
    assert np.linalg.norm(s2 - s[hperm[0][0]]) <= 1e-12 * np.linalg.norm(s)


def test_renumbering_leaves_the_injection_path(problems):
    """every refinement hierarchy numbers children consecutively: its P is what csr_is_oct_injection accepts (hexes), and
    stays a one-entry-per-row injection under every relayout but `zeros`; a renumbered P is no octree injection any more"""
    for kind in ("sampler", "darcy"):
        p = problems[kind]
        assert lc.is_oct_injection(p.levels[0].P)
        for layout in lc.ORDERS:
            assert lc.is_oct_injection(lc.relayout_problem(p, layout, SEED).levels[0].P)
        Pz = lc.relayout_problem(p, "zeros", SEED).levels[0].P
        assert not lc.is_oct_injection(Pz) and (Pz != p.levels[0].P).nnz == 0
        q, perms = lc.renumber_problem(p, SEED)
        P2 = q.levels[0].P
        assert not lc.is_oct_injection(P2)
        assert np.array_equal(np.diff(P2.indptr), np.ones(P2.shape[0])) and np.all(P2.data == 1.0), "still an injection"
        assert (P2 != p.levels[0].P[perms[0][0]][:, perms[1][0]]).nnz == 0


def test_duplicated_entry_is_the_same_matrix(problems):
    dp = problems["darcy"]
    L = dp.levels[1]
    for A in (problems["sampler"].levels[1].M, problems["sampler"].levels[1].B, L.P if L.P is not None else dp.levels[0].P):
        A2 = lc.duplicated_entry(A)
        assert A2.nnz == A.nnz + 1 and abs(A - A2).max() <= 1e-16 * abs(A).max()      # the halves sum up to rounding
    pat, lists = lc.duplicated_entry(L.M_pattern, lists=(L.c_ptr, L.c_elem, L.c_val))
    L2 = dataclasses.replace(L, M_pattern=pat, c_ptr=lists[0], c_elem=lists[1], c_val=lists[2])
    k = np.exp(np.random.default_rng(8).standard_normal(L.n_p))
    M = DarcyOracle(dp).mass(1, k)
    M2 = DarcyOracle(dataclasses.replace(dp, levels=[dp.levels[0], L2])).mass(1, k)
    assert pat.nnz == L.M_pattern.nnz + 1 and abs(M - M2).max() <= 1e-15 * abs(M).max()


# --------------------------------------------------------------------------- host code of the library (runs without a GPU)
@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_library_elimination_of_a_relaid_element_input(problems, layout):
    """pmc_hybrid_build returns the same H and G as matrices, to 1e-14 of their largest entry"""
    from parelagmc_amd import capi
    el = problems["elements"]
    H, G, z = capi.hybrid_build(*el.args())
    H2, G2, z2 = capi.hybrid_build(*lc.relayout_problem(el, layout, SEED).args())
    assert abs(H - H2).max() <= 1e-14 * abs(H).max() and abs(G - G2).max() <= 1e-14 * abs(G).max()
    assert np.max(np.abs(z - z2)) <= 1e-14 * np.max(np.abs(z))


def test_library_refuses_a_column_stored_twice_in_a_row(problems):
    """include/pmc.h: a column may appear once per row; csr_from_c refuses anything else with PMC_ERR_INVALID"""
    from parelagmc_amd import capi
    el = problems["elements"]
    pat, lists = lc.duplicated_entry(el.M_pattern, lists=(el.c_ptr, el.c_elem, el.c_val))
    for bad in (dataclasses.replace(el, M_pattern=pat, c_ptr=lists[0], c_elem=lists[1], c_val=lists[2]),
                dataclasses.replace(el, B=lc.duplicated_entry(el.B)), dataclasses.replace(el, P=lc.duplicated_entry(el.P))):
        with pytest.raises(capi.PmcError) as e:
            capi.hybrid_build(*bad.args())
        assert e.value.code == -1 and "appears twice in row" in str(e.value)

"""The Darcy solver's MINRES preconditioner on its INTERNAL hierarchies (pmc_darcy_apply_preconditioner) against the fp64
restatement oracle/precond_oracle.py:DarcyChainPrecondOracle.  Run with -m gpu on an MI355X.

A solve converges with ANY fixed SPD preconditioner, so a Gershgorin bound over the wrong rows, a wrong refresh list, a
Galerkin factor dropped or a wrong coefficient in the element-grouped cycle costs only iterations; comparing converged fields
or QoIs cannot see it.  These tests compare B(k)^-1 r itself, column by column with the column's own k, with the reference
built from the caller's data plus what pmc_darcy_vcycle_level / pmc_darcy_vcycle_prolongator export:
- a. every handle in both storages at every launch width 1 .. BatchWidth against the reference (columns 0, 1, 4 - the
  1e3-contrast field -, nb - 1 and the ends of every 32-column group; column 1 has k == 1);
- b. the setup values with a closed form (kind, lmax 1, smoothing interval, bottom polynomial, Galerkin scale s), the level
  sizes against the prolongator shapes, indicator aggregations with connected aggregates in the caller's multiplier
  numbering on the hybridized handles, a non-injection P on level 0 of the smoothed-aggregation chains;
- c. that the parametrization reaches every path the internal hierarchies run, so that a later mesh or threshold change
  cannot move everything into one of them unnoticed.

The two hierarchies (csrc/darcy.hip: build_chain, build_hybrid, hybrid_ops):
- smoothed aggregation of a saddle-point handle (mg_coarsening = 1, or the auto mode 2 on cells with anisotropy above 10):
  S_0(k) = B diag(M(k))^-1 B^T, S_{j+1} = P_j^T S_j P_j refreshed per realization through contribution lists;
- the multiplier hierarchy of a hybridized handle: S_0 = H(kappa), S_{j+1} = 0.5 P_j^T S_j P_j over indicator aggregations,
  smoothing ratio 2 mg_smooth_ratio; with mg_smooth_degree = 2 the finest level is smoothed in element-grouped form
  (eg_poly2 / eg_pair_spmm), with degree 3 the generic cycle runs on its explicit per-realization values.
Both fold the per-realization Gershgorin bound 1.0001 max_i sum_j |S_ij| / |S_ii| into D^-1 (exported lmax 1).

The handles (Monte Carlo levels: all of the problem's):
- hex-sa: hex 16^3 / 8^3 / 4^3, mg_coarsening = 1 (each MC level its own chain; level 0 inside the LDS tail, P not an
  injection);
- hex32-sa: 32^3, one MC level, mg_coarsening = 1: level 0 (32 768 rows) outside the tail, the generic per-realization path
  with a non-injection P;
- spe10-auto: the stretched box of test_stretched_cells_algebraic_coarsening, default options (the auto mode must choose the
  chain);
- hex-hybrid (degree 2 and 3), tet-hybrid, spe10-hybrid (the box of test_hybrid_darcy_on_stretched_cells);
- hex32-hybrid (degree 2 and 3): 32^3, one MC level, a chain level 1 above 8 192 rows.

Tolerances: REF_TOL of test_gpu_precond.py.

Measured on the MI355X (the printed lines), widths 1 .. BatchWidth on every MC level, against the fp64 reference:
- fp64 storage: at most 1.1e-13 (tet-hybrid level 0: the library inverts the element matrices itself, which on tetrahedra
  differs from numpy's by up to a few hundred eps of an entry; see test_darcy_operator_matches_assembled_matrix), 5.5e-14 on
  spe10-hybrid, 3.6e-14 / 2.8e-14 on hex-sa / hex32-sa, 1.4e-15 on hex32-hybrid;
- fp32 storage: at most 1.3e-7 (hex32-hybrid-d3; hex32-sa 1.1e-7, hex-hybrid-d3 1.1e-7: the iterate and residuals of levels
  outside the tail in fp32), 3.1e-8 on hex32-hybrid (element-grouped finest level), 1.5e-8 on hex-sa; levels whose whole
  cycle runs in the tail 1.9e-13 or less.
Each of five seeded mutations of a scratch build fails test a on the handles that run the mutated code, while
test_gpu_precond.py and test_gpu_sampler_precond.py pass: the Gershgorin margin 1.0001 -> 1.01 in gersh_scale_kernel, the
element-grouped smoother's interval ratio halved in hybrid_ops, the Galerkin factor dropped from build_chain's refresh lists
(export unchanged), vres -> r and c0 <-> c1 in hybrid_ops' post-smoothing eg_poly2 (the last two also break the converged
solves of test_gpu_darcy_hybrid.py).
"""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from conftest import golden_path
from test_gpu_precond import REF_TOL, _fields, _rel, _widths

pytestmark = pytest.mark.gpu

STORAGES = ("fp64", "fp32")
# Multigrid::enable_bv_tail: per-realization levels of at most this many rows carry the LDS tail's transposed copies
TAIL_ROWS = 8192
TAIL_LDS_DOUBLES = (160 * 1024 - 1024) // 8     # kTailLdsDoubles: 3 vectors per level of a tail
TAIL_MAX_LEVELS = 8

# name -> (problem, hybridized, solver options beyond the storage)
HANDLES = {
    "hex-sa": ("hex", False, dict(mg_coarsening=1)),
    "hex32-sa": ("hex32", False, dict(mg_coarsening=1)),
    "spe10-auto": ("spe10-saddle", False, {}),
    "hex-hybrid": ("hex", True, dict(mg_smooth_degree=2)),
    "hex-hybrid-d3": ("hex", True, dict(mg_smooth_degree=3)),
    "tet-hybrid": ("tet", True, {}),
    "spe10-hybrid": ("spe10-hybrid", True, {}),
    "hex32-hybrid": ("hex32", True, dict(mg_smooth_degree=2)),
    "hex32-hybrid-d3": ("hex32", True, dict(mg_smooth_degree=3)),
}

_PROBLEMS = {}


def _problem(name):
    """name -> (hierarchy, Darcy problem)"""
    if name not in _PROBLEMS:
        from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy, mesh_from_json
        if name == "hex":
            h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 2)
            dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
        elif name == "hex32":
            h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 3)
            dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
        elif name == "tet":
            m = mesh_from_json(golden_path("meshes", "cube_tet.json"))
            cen = m.verts[m.bdr].mean(axis=1)
            lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
            m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1,
                                  np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
            h = build_hierarchy(m, 2)
            dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=2)
        elif name == "spe10-saddle":
            h = build_hierarchy(box_mesh([4, 12, 6], [1200.0, 2200.0, 170.0], "hex"), 1)
            dp = build_darcy_problem(h, [1, 0, 1, 0, 1, 1], [0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0])
        else:
            assert name == "spe10-hybrid"
            h = build_hierarchy(box_mesh([7, 27, 10], [1200.0, 2200.0, 170.0], "hex"), 1)
            dp = build_darcy_problem(h, [1, 0, 1, 0, 1, 1], [0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0], n_mc_levels=1)
        _PROBLEMS[name] = (h, dp)
    return _PROBLEMS[name]


class _Handle:
    """one Darcy handle with its exported setup and a reference per MC level"""

    def __init__(self, ctx, name, storage):
        from parelagmc_amd import capi
        from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
        from oracle.precond_oracle import DarcyChainPrecondOracle
        pname, self.hybrid, extra = HANDLES[name]
        self.h, self.dp = _problem(pname)
        st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
        self.opts = capi.solver_opts(precond_storage=st, **extra)
        self.ds = capi.DarcySolver(ctx, self.dp, self.opts, hybrid=self.hybrid)
        self.setup, self.P, self.hl, self.oracle = [], [], [], []
        for lvl in range(self.dp.n_mc_levels):
            setup = self.ds.vcycle_levels(lvl)
            P = [self.ds.vcycle_prolongator(lvl, v) for v in range(len(setup) - 1)]
            hl = darcy_hybrid_level(self.h.spaces[lvl], self.dp.levels[lvl]) if self.hybrid else None
            self.setup.append(setup)
            self.P.append(P)
            self.hl.append(hl)
            self.oracle.append(DarcyChainPrecondOracle(self.dp, lvl, setup, P, hl))

    def rows(self, lvl):
        L = self.dp.levels[lvl]
        return self.hl[lvl].n_lambda if self.hybrid else L.n_u + L.n_p


_HANDLES = {}


@pytest.fixture(scope="module")
def handles(gpu_ctx):
    """(name, storage) -> _Handle, built once per module"""
    def get(name, storage):
        if (name, storage) not in _HANDLES:
            _HANDLES[(name, storage)] = _Handle(gpu_ctx, name, storage)
        return _HANDLES[(name, storage)]
    yield get
    for hd in _HANDLES.values():
        hd.ds.close()
    _HANDLES.clear()


def _cols(nb):
    """both ends of the launch and of every column group of 32 inside it, and column 4 (the 1e3-contrast field)"""
    return sorted({c for c in (0, 1, 4, nb - 1, 31, 32, 63, 64, 127, 128) if c < nb})


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(HANDLES))
def test_darcy_internal_preconditioner_matches_fp64_reference(handles, seeded_rng, name, storage):
    """B(k_j)^-1 r_j of the compared columns at every launch width 1 .. BatchWidth against DarcyChainPrecondOracle, each
    column with its own k (one oracle call per column)"""
    hd = handles(name, storage)
    for lvl in range(hd.dp.n_mc_levels):
        n, n_p = hd.rows(lvl), hd.dp.levels[lvl].n_p
        top = hd.ds.BatchWidth(lvl)
        k = _fields(seeded_rng, top, n_p)
        r = seeded_rng.standard_normal((top, n))
        ref, worst = {}, 0.0
        for nb in _widths(top):
            z = hd.ds.ApplyPreconditioner(lvl, k[:nb], r[:nb])
            assert z.shape == (nb, n)
            for j in _cols(nb):
                if j not in ref:
                    ref[j] = hd.oracle[lvl].apply(k[j], r[j])
                e = _rel(z[j], ref[j])
                worst = max(worst, e)
                assert e <= REF_TOL[storage], (lvl, nb, j, e)
        print(f"reference {name} {storage} level {lvl} ({len(hd.setup[lvl])} vlevels, rows "
              f"{[int(m['rows']) for m in hd.setup[lvl]]}) widths 1..{top}: max rel L2 = {worst:.2e}")


def _is_injection(P):
    """one unit entry per row"""
    return np.array_equal(np.diff(P.indptr), np.ones(P.shape[0])) and np.all(P.data == 1.0)


@pytest.mark.parametrize("name", list(HANDLES))
def test_darcy_internal_vcycle_setup_values(handles, name):
    """the exported setup values with a closed form, the level sizes against the prolongators, and the prolongators'
    structure (the setup does not depend on the storage: fp64 handles)"""
    from oracle.precond_oracle import KIND_HYBRID, KIND_SA
    hd = handles(name, "fp64")
    o = hd.opts
    kind = KIND_HYBRID if hd.hybrid else KIND_SA
    for lvl in range(hd.dp.n_mc_levels):
        setup, P = hd.setup[lvl], hd.P[lvl]
        nv = len(setup)
        for v, m in enumerate(setup):
            assert int(m["hierarchy"]) == kind, (lvl, v, m["hierarchy"])   # spe10-auto: the auto mode chose the chain
            assert m["lmax"] == 1.0                                         # the Gershgorin bound lives in D^-1
            assert m["smooth_degree"] == o.mg_smooth_degree
            assert m["smooth_ratio"] == (2.0 if hd.hybrid else 1.0) * o.mg_smooth_ratio
            assert m["galerkin_scale"] == (0.5 if hd.hybrid else 1.0)
            assert m["bottom"] == (1.0 if v == nv - 1 else 0.0)
            if v == nv - 1:
                assert (m["last_degree"], m["last_ratio"]) == (o.mg_coarse_degree, o.mg_coarse_ratio)
        assert setup[0]["rows"] == (hd.hl[lvl].n_lambda if hd.hybrid else hd.dp.levels[lvl].n_p)
        for v, Pv in enumerate(P):
            assert Pv.shape == (setup[v]["rows"], setup[v + 1]["rows"]), (lvl, v, Pv.shape)
            assert np.all(np.isfinite(Pv.data))
            if hd.hybrid:
                assert _is_injection(Pv), (lvl, v)
                assert np.array_equal(np.unique(Pv.indices), np.arange(Pv.shape[1])), "every aggregate has a member"
        if hd.hybrid and P:
            # level 0 in the caller's multiplier numbering: every aggregate of P_0 is connected in the graph of H(1)
            # (the aggregation follows the couplings of H(1); a renumbering would scatter the aggregates)
            H1 = hd.hl[lvl].operator(np.ones(hd.dp.levels[lvl].n_p)).tocoo()
            agg = P[0].indices
            same = agg[H1.row] == agg[H1.col]
            G = sp.csr_matrix((np.ones(int(same.sum())), (H1.row[same], H1.col[same])), shape=H1.shape)
            ncomp, _ = connected_components(G, directed=False)
            assert ncomp == P[0].shape[1], (lvl, ncomp, P[0].shape[1])
        if not hd.hybrid and P:
            assert not _is_injection(P[0]), "smoothed aggregation: P_0 is not an injection"
        print(f"setup {name} level {lvl}: rows {[int(m['rows']) for m in setup]}, P nnz {[Pv.nnz for Pv in P]}")


def _tail_start(rows):
    """the first level of the LDS tail of a per-realization hierarchy (Multigrid::enable_bv_tail / build_tails): every
    level from there on has at most TAIL_ROWS rows, at most TAIL_MAX_LEVELS of them and 3 vectors each in the LDS budget"""
    for l0 in range(len(rows)):
        rest = rows[l0:]
        if max(rest) <= TAIL_ROWS and len(rest) <= TAIL_MAX_LEVELS and 3 * sum(rest) <= TAIL_LDS_DOUBLES:
            return l0
    return len(rows)


def test_darcy_internal_preconditioner_paths_are_covered(handles):
    """the handles of this file reach every path of the internal hierarchies at least once"""
    from oracle.precond_oracle import KIND_HYBRID, KIND_SA
    seen = set()
    for name in HANDLES:
        hd = handles(name, "fp64")
        for lvl in range(hd.dp.n_mc_levels):
            setup, P = hd.setup[lvl], hd.P[lvl]
            kind = int(setup[0]["hierarchy"])
            rows = [int(m["rows"]) for m in setup]
            t0 = _tail_start(rows)
            for v, n in enumerate(rows):
                if n > TAIL_ROWS:
                    seen.add(f"kind {kind} level above the tail")
                    if kind == KIND_HYBRID and v >= 1:
                        seen.add("hybrid chain level >= 1 above the tail")
                if v >= t0 and v < len(P) and not _is_injection(P[v]):
                    seen.add("non-injection P inside the tail")
            if kind == KIND_HYBRID and len(rows) >= 2:
                seen.add("element-grouped finest level" if hd.opts.mg_smooth_degree == 2 else "generic hybrid cycle")
    want = {f"kind {KIND_SA} level above the tail", f"kind {KIND_HYBRID} level above the tail",
            "hybrid chain level >= 1 above the tail", "non-injection P inside the tail", "element-grouped finest level",
            "generic hybrid cycle"}
    assert want <= seen, f"paths no handle reaches: {sorted(want - seen)}"

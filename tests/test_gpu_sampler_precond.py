"""The sampler's MINRES preconditioner (pmc_sampler_apply_preconditioner) against the fp64 restatement
oracle/precond_oracle.py:SamplerPrecondOracle, on the hierarchies and launch widths where its kernels choose different paths.
Run with -m gpu on an MI355X.

A solve converges with ANY fixed SPD preconditioner, so a wrong segment table, a smoother on the wrong interval, an exact solve
on the wrong level or an off-by-one in a row-split piece costs only iterations; comparing fields after convergence cannot see
it.  These tests compare B^-1 r itself, column by column, with the reference built from the caller's data plus what
pmc_sampler_vcycle_level / pmc_sampler_vcycle_prolongator export (setup values, the internal prolongators):
- a. every handle kind in both storages at every launch width against the reference of its regime: launches of at most
  dense_nb (8) realizations of a hybridized handle end their cycle early with an exact dense solve, wider ones run the whole
  cycle down to the dense inverse at its bottom;
- b. the setup values with a closed form, and the conditions that make the cycle an SPD preconditioner: lmax bounds
  spec(D^-1 S_l) (eigsh), a polynomial bottom's interval contains the spectrum, the multiplier hierarchy's prolongators are
  indicator aggregations, and a kind-0 hierarchy's prolongators are the caller's;
- c. that the parametrization reaches every kernel path of Multigrid::cycle at least once (below), so that a later change of
  a mesh or of a threshold cannot move everything back into the LDS tail unnoticed;
- d. every column at every width against the same column in the narrowest launch of its regime.

The handles (MC level 0 of each; n_mc_levels = 1):
- hex32-saddle: hex 4^3 refined 3 times (32^3, Schur levels 32 768 / 4 096 / 512 / 64), corlen 0.3 - level 0 leaves the tail
  and is not reaction-dominated; fp32 storage: the fp32-intermediate kernels with the octree restriction fused
  (vc_presmooth32, vc_residual_restrict8_32, vc_residual_coarse32, vc_postsmooth32_z); fp64 storage: cheb_apply and
  residual_restrict8 (the generic fp64 path);
- tet-saddle: cube_tet refined twice (384 / 48 / 6 elements).  Its P0 prolongators are octree injections as well (the
  children of a tetrahedron are numbered consecutively), so it runs the cycle of hex32-saddle inside the LDS tail;
- hex32-sa: hex32 with mg_coarsening = 1: internal smoothed aggregation (P not an injection), the generic fp64 path in
  both storages outside the tail;
- hex12-hybrid: hybridized, hex 3^3 refined twice (5 616 multipliers): the whole cycle fits the tail for wide launches; narrow
  launches start it one level later (level 0 has more than 4 096 rows: fused aggregate restriction on kernels) and end on
  level 1 with the exact dense solve (dense_apply); the tail ends with the dense inverse ainv;
- hex24-hybrid: hybridized, hex 3^3 refined 3 times (43 200 multipliers): level 0 outside the tail at every width (fused
  aggregate restriction after agg_pack_rows), level 1 row-split (S_split, SP_split) for narrow launches.

Not covered here, because only a solve reaches them: the preconditioner inside mini_sampler_kernel and the r32_top input of the
hybridized cycle (the fp32 copy the Lanczos update of the MINRES loop writes).  test_gpu_minres_trajectory.py covers both: it
compares the iterates of whole solves on tet-saddle, hex12-hybrid and hex24-hybrid with single-vector MINRES over THIS file's
reference preconditioner.  The Darcy internal hierarchies: test_gpu_darcy_internal_precond.py.

Tolerances: REF_TOL / WIDTH_TOL of test_gpu_precond.py.  Outside the tail the fp32 storage keeps the level's iterate and
residuals in fp32 (the matrix values of these shared-value levels stay fp64): 1e-5 holds with more than two orders of margin.

Measured on the MI355X (the printed lines), widths 1 .. 64 (32^3, 24^3) or 1 .. 256:
- against the fp64 reference, fp64 storage: at most 7.9e-16 on the kind-0 handles, 1.7e-14 on hex32-sa, 7.1e-15 on the
  hybridized handles (narrow launches 5.5e-15);
- fp32 storage: hex32-saddle 9.3e-9, tet-saddle 5.4e-16 (inside the tail), hex32-sa 1.4e-14 (fp64 path), hex12-hybrid
  2.3e-15 wide (tail) / 1.9e-8 narrow, hex24-hybrid 2.5e-8 wide / 2.8e-8 narrow;
- width consistency: bit for bit within each regime, except the wide fp32 launches of hex32-saddle (4.0e-17) and hex24-hybrid
  (5.4e-17).
"""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import eigsh

from precond_cases import HANDLES, REF_TOL, Handle as _Handle, rel as _rel   # shared with test_gpu_minres_trajectory.py

pytestmark = pytest.mark.gpu

# relative L2 bound of a column against the same column in another launch, per storage (REF_TOL: against the fp64 reference)
WIDTH_TOL = {"fp64": 1e-12, "fp32": 1e-5}
STORAGES = ("fp64", "fp32")


def _widths(top):
    w, out = 1, []
    while w <= top:
        out.append(w)
        w *= 2
    return out


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
        hd.smp.close()
    _HANDLES.clear()


def _cols(nb):
    """both ends of the launch and of every column group of 32 inside it"""
    return sorted({c for c in (0, 1, nb - 1, 7, 8, 31, 32, 63, 64, 127, 128) if c < nb})


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(HANDLES))
def test_sampler_preconditioner_matches_fp64_reference(handles, seeded_rng, name, storage):
    """B^-1 r_j of the compared columns at every launch width 1 .. BatchWidth against the fp64 reference of the launch's
    regime (one oracle call per column and regime)"""
    hd = handles(name, storage)
    r = seeded_rng.standard_normal((hd.top, hd.n))
    ref, worst = {}, {False: 0.0, True: 0.0}
    for nb in _widths(hd.top):
        z = hd.smp.ApplyPreconditioner(0, r[:nb])
        narrow = hd.narrow(nb)
        for j in _cols(nb):
            if (j, narrow) not in ref:
                ref[(j, narrow)] = hd.oracle.apply(r[j], narrow)
            e = _rel(z[j], ref[(j, narrow)])
            worst[narrow] = max(worst[narrow], e)
            assert e <= REF_TOL[storage], (nb, j, e)
    for narrow in (True, False):
        if (hd.dense_nb > 0) or not narrow:
            print(f"reference {name} {storage} level 0 {'narrow' if narrow else 'wide'} widths 1..{hd.top}: "
                  f"max rel L2 = {worst[narrow]:.2e}")


def _scaled_extremes(S, lo=False):
    """largest (and, lo, smallest) eigenvalue of D^-1 S via the symmetric D^-1/2 S D^-1/2"""
    d = 1.0 / np.sqrt(S.diagonal())
    A = (sp.diags(d) @ S @ sp.diags(d)).tocsr()
    if A.shape[0] <= 6000:
        ev = np.linalg.eigvalsh(A.toarray())
        return ev[-1], ev[0]
    hi = eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-10)[0]
    return hi, (eigsh(A, k=1, which="SA", return_eigenvectors=False, tol=1e-10)[0] if lo else None)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(HANDLES))
def test_sampler_vcycle_setup_values(handles, name, storage):
    """closed-form setup values, lmax >= lambda_max(D^-1 S_l), spec(D^-1 S) inside the interval of a polynomial bottom, the
    exported prolongators (the caller's on kind 0, indicator aggregations on kind 2)"""
    from oracle.precond_oracle import KIND_CALLER, KIND_HYBRID, KIND_SA, ROLE_DESCEND, ROLE_POLY, ROLE_UNREACHED
    hd = handles(name, storage)
    o = hd.opts
    cfg = HANDLES[name]
    kind = KIND_HYBRID if hd.hybrid else (KIND_SA if cfg["coarsening"] == 1 else KIND_CALLER)
    for v, m in enumerate(hd.setup):
        assert int(m["hierarchy"]) == kind
        assert m["rows"] == hd.info[v]["rows"]
        assert m["smooth_degree"] == o.mg_smooth_degree
        # the aggregation hierarchy of H smooths on twice the interval ratio of the Schur hierarchies
        assert m["smooth_ratio"] == (2.0 if hd.hybrid else 1.0) * o.mg_smooth_ratio
        assert m["galerkin_scale"] == (0.0 if kind == KIND_CALLER else 1.0)
        assert m["dense_nb"] == (8 if hd.hybrid else 0)
        if hd.hybrid:
            assert m["degree_M"] == 0 and m["ratio_M"] == 0
        else:
            assert m["ratio_M"] > 1.0
            assert m["degree_M"] == (o.cheb_degree_M or (4 if m["ratio_M"] > 16.0 else 2))
        if hd.dense_nb == 0:
            assert m["role_narrow"] == m["role_wide"] and m["tail_narrow"] == m["tail_wide"]
    # the cycle ends exactly once per regime, and no level is smoothed after it
    for key in ("role_wide", "role_narrow"):
        roles = [int(m[key]) for m in hd.setup]
        ends = [v for v, q in enumerate(roles) if q not in (ROLE_DESCEND, ROLE_UNREACHED)]
        assert len(ends) == 1 and all(q == ROLE_DESCEND for q in roles[:ends[0]]), (key, roles)
        assert all(q == ROLE_UNREACHED for q in roles[ends[0] + 1:]), (key, roles)
    # level 0 is not where the cycle ends (a reaction-dominated level 0 would make it a single polynomial)
    assert int(hd.setup[0]["role_wide"]) == ROLE_DESCEND
    if kind == KIND_CALLER:
        for v in range(len(hd.P)):
            Pc = hd.prob.levels[v].P
            assert hd.setup[v]["rows"] == hd.prob.levels[v].n_s
            assert (hd.P[v] != Pc).nnz == 0 and hd.P[v].shape == Pc.shape
    if kind == KIND_HYBRID:
        assert hd.setup[0]["rows"] == hd.prob.levels[0].n_lambda
        for P in hd.P:
            assert np.array_equal(np.diff(P.indptr), np.ones(P.shape[0])) and np.all(P.data == 1.0)
            assert np.array_equal(np.unique(P.indices), np.arange(P.shape[1])), "every aggregate has a member"
    for v, m in enumerate(hd.setup):
        if int(m["role_wide"]) == ROLE_UNREACHED and int(m["role_narrow"]) == ROLE_UNREACHED:
            break
        S = hd.oracle.S[v]
        assert S.shape[0] == m["rows"]
        poly = int(m["role_wide"]) == ROLE_POLY or int(m["role_narrow"]) == ROLE_POLY
        hi, lo = _scaled_extremes(S, lo=poly)
        assert hi <= m["lmax"], (v, hi, m["lmax"])
        if poly:
            assert lo >= m["lmax"] / m["last_ratio"], (v, lo, m["lmax"], m["last_ratio"])
        print(f"setup {name} {storage} vlevel {v}: rows {int(m['rows'])} lambda_max(D^-1 S) {hi:.4f} <= lmax {m['lmax']:.4f}"
              + (f", lambda_min {lo:.4f} >= lmax / ratio {m['lmax'] / m['last_ratio']:.4f}" if poly else ""))


def _is_oct(P):
    """csr_is_oct_injection's rule: rows 8 i .. 8 i + 7 are the children of coarse row i, unit weights"""
    P = P.tocsr()
    return (P.shape[0] == 8 * P.shape[1] and np.array_equal(np.diff(P.indptr), np.ones(P.shape[0]))
            and np.array_equal(P.indices, np.arange(P.shape[0]) // 8) and np.all(P.data == 1.0))


def test_sampler_preconditioner_paths_are_covered(handles):
    """the handles of this file reach every path of Multigrid::cycle at least once (from pmc_sampler_vcycle_info's flags and
    pmc_sampler_vcycle_level's roles)"""
    from oracle.precond_oracle import KIND_CALLER, KIND_HYBRID, KIND_SA, ROLE_DESCEND, ROLE_EXACT
    seen = set()
    for name in HANDLES:
        for storage in STORAGES:
            hd = handles(name, storage)
            for v, (m, f) in enumerate(zip(hd.setup, hd.info)):
                kind = int(m["hierarchy"])
                wide_kernels = int(m["role_wide"]) == ROLE_DESCEND and not m["tail_wide"]
                narrow_kernels = int(m["role_narrow"]) == ROLE_DESCEND and not m["tail_narrow"]
                if storage == "fp32" and kind == KIND_CALLER and wide_kernels and f["fused_restriction"] and _is_oct(hd.P[v]):
                    seen.add("octree fp32 out of the tail")
                if storage == "fp32" and kind == KIND_HYBRID and wide_kernels and f["fused_restriction"]:
                    seen.add("fused aggregate restriction")
                if wide_kernels and (storage == "fp64" or kind == KIND_SA):
                    seen.add("generic fp64")
                if int(m["role_narrow"]) == ROLE_EXACT and int(m["role_wide"]) == ROLE_DESCEND:
                    seen.add("narrow exact dense solve")
                if storage == "fp32" and narrow_kernels and v > 0 and f["narrow_pieces"] > 1:
                    seen.add("row split")
                if v == 0 and m["rows"] > 4096 and hd.dense_nb >= 1 and m["tail_wide"] and not m["tail_narrow"]:
                    seen.add("late tail start")
                if int(m["role_wide"]) == ROLE_EXACT:
                    seen.add("ainv bottom")
    want = {"octree fp32 out of the tail", "fused aggregate restriction", "generic fp64", "narrow exact dense solve",
            "row split", "late tail start", "ainv bottom"}
    assert want <= seen, f"paths no handle reaches: {sorted(want - seen)}"


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(HANDLES))
def test_sampler_preconditioner_is_the_same_at_every_width(handles, seeded_rng, name, storage):
    """within each regime every column equals the same column in the narrowest launch of that regime: width 1 for launches
    of at most dense_nb realizations, width 2 dense_nb (its column group) for the wider ones"""
    hd = handles(name, storage)
    r = seeded_rng.standard_normal((hd.top, hd.n))
    alone = np.stack([hd.smp.ApplyPreconditioner(0, r[j:j + 1])[0] for j in range(hd.top)])
    assert np.all(np.isfinite(alone)) and np.all(np.linalg.norm(alone, axis=1) > 0)
    base = {True: alone, False: alone}
    w0 = 2 * hd.dense_nb
    if hd.dense_nb > 0 and w0 <= hd.top:
        base[False] = np.concatenate([hd.smp.ApplyPreconditioner(0, r[c:c + w0]) for c in range(0, hd.top, w0)])
    worst = {True: 0.0, False: 0.0}
    for nb in _widths(hd.top)[1:]:
        narrow = hd.narrow(nb)
        for c0 in sorted({0, hd.top - nb}):
            z = hd.smp.ApplyPreconditioner(0, r[c0:c0 + nb])
            for j in range(nb):
                e = _rel(z[j], base[narrow][c0 + j])
                worst[narrow] = max(worst[narrow], e)
                assert e <= WIDTH_TOL[storage], (nb, c0 + j, e)
    print(f"width-consistency {name} {storage} level 0 widths 1..{hd.top}: max rel L2 narrow {worst[True]:.2e}, "
          f"wide {worst[False]:.2e}")

"""The MINRES operator and preconditioner of the Darcy solvers, applied on their own through pmc_darcy_apply_operator /
pmc_darcy_apply_preconditioner (the same per-realization setup and the same closures as pmc_darcy_solve_fwd), and the
column independence of the sampler's preconditioner.  Run with -m gpu on an MI355X.

Solves converge to the direct-solve answer with ANY fixed SPD preconditioner, so a smoother on the wrong interval, a wrong
Galerkin scale or a per-realization hierarchy in which column j read another column's values would only cost iterations.
These tests pin what a solve cannot:
- B(k)^-1 of saddle-point handles on the caller's hierarchy against the fp64 restatement oracle/precond_oracle.py, every
  compared column with its own k, at every launch width, and the setup values with a closed form against
  pmc_darcy_vcycle_level;
- the operator against the assembled CSR matrix of every column (its own k), at every launch width;
- the preconditioner of every column at every launch width against the same column launched alone (the Darcy hierarchies
  choose no path by width: dense_nb = 0 and no later LDS tail), on saddle-point and hybridized handles;
- column independence, bit for bit: a zero column gives exactly 0, a duplicated column (same r, same k) its twin's result,
  permuting the columns of (r, k) permutes z, and swapping k between two columns with equal r swaps their results;
- the block structure (u- and p-rows preconditioned independently) and the symmetry of B(k)^-1 per column.

The hex32 handle (32^3, one MC level) puts the finest level (32 768 rows) outside the LDS tail, which takes per-realization
levels of at most 8 192 rows: with PMC_STORAGE_FP32 it runs the fp32-value kernels vc_presmooth32_bv, vc_restrict8_32_bv,
vc_prolong8_32, vc_residual32_bv and vc_postsmooth32_bv_z, with PMC_STORAGE_FP64 the bv Chebyshev polynomial and
residual_restrict8.  The sampler's preconditioner (every hierarchy kind, both width regimes) is compared with a reference in
test_gpu_sampler_precond.py.

The Darcy internal hierarchies (mg_coarsening and the hybridized Darcy handle) are compared with a reference in
test_gpu_darcy_internal_precond.py; here hex-sa (mg_coarsening = 1) and spe10-hybrid join the width-consistency and
column-independence tests.

Not covered by this file: the preconditioner inside mini_sampler_kernel and the r32_top input of the hybridized sampler's
cycle, which only the MINRES loop provides - test_gpu_minres_trajectory.py compares the iterates of whole solves on those
paths (and of the Darcy solves of this file's `hex` problem) with single-vector MINRES over the reference preconditioners.

Measured on the MI355X (the printed lines), widths 1 .. 256 on every level:
- against the fp64 reference: at most 2.8e-15 with PMC_STORAGE_FP64, 2.6e-9 with PMC_STORAGE_FP32 (these levels keep the
  fp64 values inside the LDS tail; z is returned in fp64); hex32: 5.1e-16 (fp64) and 8.1e-8 (fp32: the finest level's values,
  iterate and residuals in fp32 - REF_TOL's 1e-5 holds with two orders of margin);
- operator, saddle-point (hex, tet with and without the element-grouped M-block): max |y - Ax| / (|A||x|) 1.9 .. 2.8 eps;
  hybridized: 2.7 .. 3.4 eps on hexahedra, relative L2 error at most 1.1e-15 on tetrahedra;
- preconditioner at width nb against the column alone: bit for bit equal on every path (hex32 included) and in both
  storages, except the
  materialised M-block (cheb_degree_M = 3), where the polynomial's rounding depends on the width: 1.5e-16 (fp64) and 2.5e-16
  (fp32 storage);
- every bitwise column-independence check held on every path, both storages;
- hex-sa and spe10-hybrid (the internal hierarchies): bit for bit equal to the column alone at every width, both storages.
"""
import dataclasses

import numpy as np
import pytest

from conftest import golden_path
from precond_cases import REF_TOL, darcy_fields as _fields   # shared with test_gpu_minres_trajectory.py

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
# relative L2 bound of a column against the same column at width 1, per preconditioner storage
WIDTH_TOL = {"fp64": 1e-12, "fp32": 1e-5}


def _widths(top):
    w, out = 1, []
    while w <= top:
        out.append(w)
        w *= 2
    return out


def _tet_hierarchy(nref):
    from parelagmc_amd.fe import build_hierarchy, mesh_from_json
    m = mesh_from_json(golden_path("meshes", "cube_tet.json"))
    cen = m.verts[m.bdr].mean(axis=1)
    lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
    m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1, np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
    return build_hierarchy(m, nref)


@pytest.fixture(scope="module")
def problems(hex_hierarchy):
    """name -> (hierarchy, Darcy problem): the octree hierarchy (hexahedra) and tetrahedra"""
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy
    out = {"hex": (hex_hierarchy, build_darcy_problem(hex_hierarchy, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]))}
    ht = _tet_hierarchy(2)
    out["tet"] = (ht, build_darcy_problem(ht, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=2))
    # 32^3 hexahedra, one MC level: a per-realization level above 8 192 rows (outside the LDS tail)
    h32 = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 3)
    out["hex32"] = (h32, build_darcy_problem(h32, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1))
    # the hex problem on the internal smoothed-aggregation hierarchy (EXTRA_OPTS), and SPE10-shaped cells hybridized
    out["hex-sa"] = out["hex"]
    hs = build_hierarchy(box_mesh([7, 27, 10], [1200.0, 2200.0, 170.0], "hex"), 1)
    out["spe10"] = (hs, build_darcy_problem(hs, [1, 0, 1, 0, 1, 1], [0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0], n_mc_levels=1))
    return out


# handle kinds: (problem, hybridized, cheb_degree_M) - degree 2 takes the element-grouped M-block, 3 the materialised M(k)
HANDLES = [("hex", False, 0), ("tet", False, 0), ("tet", False, 3), ("hex", True, 0), ("tet", True, 0)]
HANDLE_IDS = ["hex-saddle", "tet-saddle-eg", "tet-saddle-noeg", "hex-hybrid", "tet-hybrid"]
# ... and the saddle-point handle whose finest level (32^3: 32 768 rows) runs the per-realization V-cycle kernels outside the
# LDS tail: fp32 storage vc_presmooth32_bv / vc_restrict8_32_bv / vc_prolong8_32 / vc_residual32_bv / vc_postsmooth32_bv_z,
# fp64 storage the bv Chebyshev polynomial and residual_restrict8
# ... and the internal hierarchies: smoothed aggregation of the Schur block (mg_coarsening = 1, every MC level its own chain)
# and the hybridized handle's multiplier aggregation on SPE10-shaped cells (tests/test_gpu_darcy_internal_precond.py)
PRECOND_HANDLES = HANDLES + [("hex32", False, 0), ("hex-sa", False, 0), ("spe10", True, 0)]
PRECOND_IDS = HANDLE_IDS + ["hex32-saddle", "hex-sa", "spe10-hybrid"]
# solver options of a problem name beyond the storage and cheb_degree_M
EXTRA_OPTS = {"hex-sa": dict(mg_coarsening=1)}


def _solver(ctx, problems, name, hybrid, degM, storage="fp32"):
    from parelagmc_amd import capi
    h, dp = problems[name]
    st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
    return capi.DarcySolver(ctx, dp, capi.solver_opts(precond_storage=st, cheb_degree_M=degM, **EXTRA_OPTS.get(name, {})),
                            hybrid=hybrid)


def _rows(problems, name, hybrid, lvl):
    h, dp = problems[name]
    L = dp.levels[lvl]
    if not hybrid:
        return L.n_u + L.n_p
    from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
    return darcy_hybrid_level(h.spaces[lvl], L).n_lambda


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


@pytest.mark.parametrize("name,hybrid,degM", HANDLES, ids=HANDLE_IDS)
def test_darcy_operator_matches_assembled_matrix(gpu_ctx, problems, seeded_rng, name, hybrid, degM):
    """y = A(k_j) x_j for every column at every launch width against scipy's product with the oracle's assembled matrix of
    that column (DarcyOracle.assemble; the host restatement H(kappa) on a hybridized handle): |y - A x| <= 8 eps |A| |x|
    (hybridized tetrahedra: relative L2 error <= 1e-13, see below)"""
    from oracle.darcy_oracle import DarcyOracle
    from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
    h, dp = problems[name]
    do = DarcyOracle(dp)
    ds = _solver(gpu_ctx, problems, name, hybrid, degM)
    for lvl in range(dp.n_mc_levels):
        L = dp.levels[lvl]
        hl = darcy_hybrid_level(h.spaces[lvl], L) if hybrid else None
        # H(kappa) is applied element by element (shared element entries times kappa_e): its rounding is bounded by the sum of
        # the absolute element contributions, which the entries of H (sums with cancellation between elements) undercount
        hl_abs = dataclasses.replace(hl, h_val=np.abs(hl.h_val)) if hybrid else None
        # ... and its element entries X_e come from the library's own inversion of the element matrices, not numpy's: on
        # tetrahedra single entries then differ by up to 350 eps of the row scale, so there the bound is on the column's relative
        # L2 error instead (1e-13; a wrong coefficient or a dropped row is O(1)); hexahedra keep 8 eps
        n = hl.n_lambda if hybrid else L.n_u + L.n_p
        worst = worst_l2 = 0.0
        for nb in _widths(ds.BatchWidth(lvl)):
            k = _fields(seeded_rng, nb, L.n_p)
            x = seeded_rng.standard_normal((nb, n))
            y = ds.ApplyOperator(lvl, k, x)
            assert y.shape == (nb, n)
            for j in range(nb):
                if hybrid:
                    kappa = k[j] if dp.k_divides else 1.0 / k[j]
                    A, absA = hl.operator(kappa), hl_abs.operator(kappa)
                else:
                    A = do.assemble(lvl, k[j])[0].tocsr()
                    absA = abs(A)
                ref = A @ x[j]
                err = float((np.abs(y[j] - ref) / (absA @ np.abs(x[j]))).max())
                worst = max(worst, err)
                worst_l2 = max(worst_l2, _rel(y[j], ref))
                if hybrid and name == "tet":
                    assert _rel(y[j], ref) < 1e-13, (lvl, nb, j, _rel(y[j], ref))
                else:
                    assert err < 8 * EPS, (lvl, nb, j, err)
        print(f"operator {name} hybrid={hybrid} degM={degM} level {lvl}: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps, "
              f"max rel L2 = {worst_l2:.2e}")
    ds.close()


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("name,hybrid,degM", PRECOND_HANDLES, ids=PRECOND_IDS)
def test_darcy_preconditioner_is_the_same_at_every_width(gpu_ctx, problems, seeded_rng, name, hybrid, degM, storage):
    """every column of a launch of width 1, 2, 4, ... BatchWidth equals the same (r, k) launched alone; the column's own k is
    what it is preconditioned with (a width-1 launch has no other column to read)"""
    _, dp = problems[name]
    ds = _solver(gpu_ctx, problems, name, hybrid, degM, storage)
    for lvl in range(dp.n_mc_levels):
        n, n_p = _rows(problems, name, hybrid, lvl), dp.levels[lvl].n_p
        top = ds.BatchWidth(lvl)
        k = _fields(seeded_rng, top, n_p)
        r = seeded_rng.standard_normal((top, n))
        alone = np.stack([ds.ApplyPreconditioner(lvl, k[j:j + 1], r[j:j + 1])[0] for j in range(top)])
        assert np.all(np.isfinite(alone)) and np.all(np.linalg.norm(alone, axis=1) > 0)
        worst = 0.0
        for nb in _widths(top)[1:]:
            for c0 in sorted({0, top - nb}):         # the first and the last nb columns (every column group of the widest)
                z = ds.ApplyPreconditioner(lvl, k[c0:c0 + nb], r[c0:c0 + nb])
                for j in range(nb):
                    e = _rel(z[j], alone[c0 + j])
                    worst = max(worst, e)
                    assert e <= WIDTH_TOL[storage], (lvl, nb, c0 + j, e)
        print(f"width-consistency {name} hybrid={hybrid} degM={degM} {storage} level {lvl} widths 1..{top}: "
              f"max rel L2 = {worst:.2e}")
    ds.close()


def _independence_batch(rng, nb, n, n_p):
    """columns of r with magnitudes 1e-6 .. 1e6, column 2 zero, the last column a copy of column 0 (r and k); columns 1 and
    2 of r_eq are equal (for the k swap)"""
    k = _fields(rng, nb, n_p)
    r = rng.standard_normal((nb, n)) * np.logspace(-6, 6, nb)[:, None]
    if nb >= 3:
        r[2] = 0.0
    if nb >= 4:
        r[-1], k[-1] = r[0], k[0]
    return k, r


def _check_independence(apply, rng, nb, n, n_p):
    k, r = _independence_batch(rng, nb, n, n_p)
    z = apply(k, r)
    assert np.all(np.isfinite(z))
    assert np.array_equal(z[2], np.zeros(n)), "a zero column must give exactly zero"
    assert np.array_equal(z[-1], z[0]), "a duplicated column must give its twin's result bit for bit"
    perm = rng.permutation(nb)
    zp = apply(k[perm], r[perm])
    assert np.array_equal(zp, z[perm]), "permuting the columns of (r, k) must permute z bit for bit"
    # equal r in columns 0 and 1, different k: swapping the two k swaps the two results
    r2 = r.copy()
    r2[1] = r2[0]
    za = apply(k, r2)
    k2 = k.copy()
    k2[[0, 1]] = k2[[1, 0]]
    zb = apply(k2, r2)
    assert np.array_equal(zb[[1, 0]], za[[0, 1]]), "swapping k between two columns must swap their results bit for bit"
    assert np.array_equal(zb[2:], za[2:]), "the other columns must not change"
    assert not np.array_equal(za[0], za[1]), "columns with different k must not give the same result"


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("name,hybrid,degM", PRECOND_HANDLES, ids=PRECOND_IDS)
def test_darcy_preconditioner_columns_are_independent(gpu_ctx, problems, seeded_rng, name, hybrid, degM, storage):
    """zero / duplicate / permuted / k-swapped columns at the widest launch of every level (bit for bit)"""
    _, dp = problems[name]
    ds = _solver(gpu_ctx, problems, name, hybrid, degM, storage)
    for lvl in range(dp.n_mc_levels):
        n, n_p = _rows(problems, name, hybrid, lvl), dp.levels[lvl].n_p
        for nb in sorted({4, ds.BatchWidth(lvl)}):
            _check_independence(lambda k, r: ds.ApplyPreconditioner(lvl, k, r), seeded_rng, nb, n, n_p)
    ds.close()


@pytest.mark.parametrize("name", ["hex", "tet"])
def test_darcy_preconditioner_is_block_diagonal_and_symmetric(gpu_ctx, problems, seeded_rng, name):
    """saddle-point handles, fp64 storage: the u- and p-rows are preconditioned independently (a zero block gives exactly zero
    there), and <B^-1 r1, r2> = <r1, B^-1 r2> > 0 per column with its own k"""
    _, dp = problems[name]
    ds = _solver(gpu_ctx, problems, name, False, 0, "fp64")
    for lvl in range(dp.n_mc_levels):
        L = dp.levels[lvl]
        n, nu = L.n_u + L.n_p, L.n_u
        nb = min(8, ds.BatchWidth(lvl))
        k = _fields(seeded_rng, nb, L.n_p)
        r1, r2 = seeded_rng.standard_normal((2, nb, n))
        z1, z2 = ds.ApplyPreconditioner(lvl, k, r1), ds.ApplyPreconditioner(lvl, k, r2)
        ru, rp = r1.copy(), r1.copy()
        ru[:, nu:] = 0.0
        rp[:, :nu] = 0.0
        zu, zp = ds.ApplyPreconditioner(lvl, k, ru), ds.ApplyPreconditioner(lvl, k, rp)
        assert np.array_equal(zu[:, nu:], np.zeros((nb, n - nu))) and np.array_equal(zp[:, :nu], np.zeros((nb, nu)))
        assert np.allclose(zu + zp, z1, rtol=0, atol=1e-13 * np.abs(z1).max())
        for j in range(nb):
            a, b = z1[j] @ r2[j], r1[j] @ z2[j]
            assert abs(a - b) <= 1e-12 * np.sqrt((z1[j] @ r1[j]) * (z2[j] @ r2[j])), (lvl, j, a, b)
            assert z1[j] @ r1[j] > 0
    ds.close()


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["saddle", "hybrid"])
def test_sampler_preconditioner_columns_are_independent(gpu_ctx, hex_hierarchy, seeded_rng, kind, storage):
    """the sampler's preconditioner (shared values, pmc_sampler_apply_preconditioner): a zero column gives exactly zero, a
    duplicated column its twin's result, a permutation of the columns the permuted result - bit for bit, at 4 columns and
    at the widest launch of every level"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    build = build_hybrid_sampler_problem if kind == "hybrid" else build_sampler_problem
    sp = build(hex_hierarchy, corlen=0.1, lognormal=True)
    st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
    smp = capi.PDESampler(gpu_ctx, sp, capi.solver_opts(precond_storage=st))
    for lvl in range(smp.nlevels):
        L = sp.levels[lvl]
        n = L.n_lambda if kind == "hybrid" else L.n_u + L.n_s
        for nb in sorted({4, smp.BatchWidth(lvl)}):
            r = seeded_rng.standard_normal((nb, n)) * np.logspace(-6, 6, nb)[:, None]
            r[2] = 0.0
            r[-1] = r[0]
            z = smp.ApplyPreconditioner(lvl, r)
            assert np.all(np.isfinite(z))
            assert np.array_equal(z[2], np.zeros(n)) and np.array_equal(z[-1], z[0])
            perm = seeded_rng.permutation(nb)
            assert np.array_equal(smp.ApplyPreconditioner(lvl, r[perm]), z[perm])
    smp.close()


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("name,degM", [("hex", 0), ("tet", 0), ("tet", 3), ("hex32", 0)],
                         ids=["hex-eg", "tet-eg", "tet-noeg", "hex32-eg"])
def test_darcy_preconditioner_matches_fp64_reference(gpu_ctx, problems, seeded_rng, name, degM, storage):
    """B(k_j)^-1 r_j of every compared column at every launch width 1 .. BatchWidth against the fp64 restatement
    (oracle/precond_oracle.py: M-block polynomial, Schur V-cycle over the caller's P with S_{l+1} = 1/2 P^T S_l P), each column
    with its own k.  The setup values with a closed form (lmax = 2 * 1.0001, the Galerkin scale 1/2, the smoothing and
    coarsest-level parameters of the options, where the cycle ends) are asserted equal to what pmc_darcy_vcycle_level exports;
    ratio_M (a Lanczos estimate at k == 1) is taken from it."""
    from parelagmc_amd import capi
    from oracle.precond_oracle import GALERKIN_SCALE, LMAX_SCHUR, DarcyPrecondOracle
    _, dp = problems[name]
    o = capi.solver_opts()
    po = DarcyPrecondOracle(dp, o.mg_smooth_degree, o.mg_smooth_ratio, o.mg_coarse_degree, o.mg_coarse_ratio)
    ds = _solver(gpu_ctx, problems, name, False, degM, storage)
    nlev = len(dp.levels)
    if name == "hex32":
        # the finest level really takes the kernels outside the tail: more than 8 192 rows (Multigrid::enable_bv_tail) and
        # the 8-children injection csr_is_oct_injection accepts (the fused restriction / prolongation of the bv kernels)
        L0 = dp.levels[0]
        P = L0.P.tocsr()
        assert L0.n_p > 8192 and P.shape == (L0.n_p, dp.levels[1].n_p) and P.shape[0] == 8 * P.shape[1]
        assert np.array_equal(np.diff(P.indptr), np.ones(P.shape[0])) and np.all(P.data == 1.0)
        assert np.array_equal(P.indices, np.arange(P.shape[0]) // 8)
    for lvl in range(dp.n_mc_levels):
        info = ds.vcycle_levels(lvl)
        assert len(info) == nlev - lvl
        for v, m in enumerate(info):
            assert m["hierarchy"] == 0 and m["rows"] == dp.levels[lvl + v].n_p
            assert m["lmax"] == LMAX_SCHUR and m["galerkin_scale"] == GALERKIN_SCALE
            assert (m["smooth_degree"], m["smooth_ratio"]) == po.smooth[:2]
            assert m["bottom"] == (1.0 if lvl + v == nlev - 1 else 0.0)
            if m["bottom"]:
                assert (m["last_degree"], m["last_ratio"]) == po.smooth[2:]
        ratio_M, deg_M = info[0]["ratio_M"], int(info[0]["degree_M"])
        assert deg_M == (degM or 2) and ratio_M > 1.0
        n, n_p = _rows(problems, name, False, lvl), dp.levels[lvl].n_p
        top = ds.BatchWidth(lvl)
        k = _fields(seeded_rng, top, n_p)
        r = seeded_rng.standard_normal((top, n))
        ref = {}
        worst = 0.0
        for nb in _widths(top):
            z = ds.ApplyPreconditioner(lvl, k[:nb], r[:nb])
            # both ends of the launch and of every column group of 32 inside it
            cols = sorted({c for c in (0, 1, nb - 1, 31, 32, 63, 64, 127, 128) if c < nb})
            for j in cols:
                if j not in ref:
                    ref[j] = po.apply(lvl, k[j], r[j], ratio_M, deg_M)
                e = _rel(z[j], ref[j])
                worst = max(worst, e)
                assert e <= REF_TOL[storage], (lvl, nb, j, e)
        print(f"reference {name} degM={degM} {storage} level {lvl} widths 1..{top}: max rel L2 = {worst:.2e}")
    ds.close()

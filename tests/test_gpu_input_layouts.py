"""Handles created on the matrices real callers hand over: rows in descending, random and diagonal-first order, stored
zeros, renumbered dofs (tests/layout_cases.py).  Run with -m gpu on an MI355X.

include/pmc.h takes pmc_csr with "sorted or unsorted column indices", MFEM sorts nothing, hypre stores the diagonal first,
EliminateRowCol leaves stored zeros and METIS numbers the children of an agglomerate anyhow - and every builder of this
repository ends in sort_indices().  A relayout is exact on the reference side (tests/test_layout_cases.py: the oracles
return the same bits), so every check here takes the canonical problem's reference and the bound of the test it mirrors:

- a. operators (PDESampler.Mult, DarcySolver.ApplyOperator; widths 1, 8, BatchWidth): |y - A x| <= 8 eps |A| |x| per
  entry against scipy on the canonical matrix (test_gpu_parity.py, test_gpu_precond.py); hybridized Darcy on tetrahedra:
  relative L2 1e-13, for the reason test_gpu_precond.py gives;
- b. preconditioners (both storages, widths 1 and BatchWidth) against SamplerPrecondOracle / DarcyPrecondOracle built from
  the CANONICAL problem plus what the re-laid handle exports, within precond_cases.REF_TOL - what sees a P row whose stored
  zero changed the kernel path, or a diagonal taken from the wrong slot;
- c. solves at test_gpu_parity.py's TIGHT options against the oracles' direct solves: fields 1e-9 (Eval on level 1, then
  level 0 warm-started from it), Darcy Q 1e-9 and solution 1e-8, converged == 1; iteration counts printed, not asserted;
- d. mass_sensitivity / mass_tangent (per-entry summation bounds of test_gpu_darcy_gradient.py / _gn_hessian.py against the
  long-double twins), solve_gradient and gn_hessvec (those files' TOL_*), both k_divides, saddle and hybridized handles;
- e. the entry points that take a CSR of their own: SetObservations + ComputeG (Gobs), set_projection L2 (Gt),
  SetOutputHierarchy + ComputeL2Error (P_orig), Conditioner (H0), KLSampler (P), LevelFields.parents() (P with stored
  zeros), pmc_hybrid_build (the element input) - each against its canonical twin;
- f. bit for bit: the sampler sorts M, B (H, G) at create, so handles that differ only in the order of those return
  np.array_equal operators, preconditioners, fields, solver statistics and field statistics;
- g. renumbered problems (hex): a, b, c against oracles built from the RENUMBERED problem plus the handle's own exports
  (pairwise matching, SELL slices and the tail layout depend on the row order: the preconditioner is not the permuted
  canonical one).  A renumbered P is a one-entry injection that csr_is_oct_injection refuses.  Saddle-point sampler and
  Darcy handles and the hybridized sampler; not the hybridized Darcy handle, whose multiplier numbering is its own.
- duplicates: a column stored twice in a row is refused by every create function (PMC_ERR_INVALID, include/pmc.h).

Problems: hex (conftest.hex_hierarchy_small, 8^3 / 4^3), tet (tracer_cases.hierarchy("tet1"), 48 / 6 tetrahedra), agg
(derivative_family_cases agg2 / agg-unit: 384 / 41 / 5 elements, rows of 5 to 12 entries).

What these tests found (fixed in the same change): pmc_hybrid_build, and with it the hybridized Darcy handle, refused an
M_pattern with stored zeros ("fewer contributions than stored entries" in element_inverses):
tests/test_layout_cases.py::test_library_elimination_of_a_relaid_element_input[zeros] and its copy here failed, and no
`zeros` case of a hybridized Darcy handle could be created.  The oracles' M(k) (np.add.reduceat) returned the neighbouring
entry's value for an entry with an empty list.  Nothing else: every other assertion held on the first run.

Duplicates before this change, from the code: csr_diag summed them, sell_build took the last one as the diagonal, the
injection tests read the first entry of the row, Darcy's dM1 took the last list - no single rule, so csr_from_c now refuses
them for every matrix (test_create_functions_refuse_a_column_stored_twice).

Measured on the MI355X (the printed lines; the same figure for every layout unless noted):
- a. sampler operators at most 2.51 eps, Darcy operators at most 2.69 eps (hybridized tetrahedra 5.84 eps per entry,
  relative L2 3.8e-16), bound 8 eps;
- b. sampler preconditioners, both storages (these levels lie inside the LDS tail, which keeps fp64): saddle at most
  8.1e-16, hybridized 6.5e-15; Darcy 1.7e-15 (fp64) and 5.0e-9 (fp32).  Level 0 of the hex saddle handle reports
  (role_wide, in_tail, fused_restriction) = (0, 1, 1) for the canonical and the three reordered problems and (0, 1, 0)
  under `zeros` and under the renumbering: the stored zero / the other numbering moves it off the fused octree restriction;
- c. fields at most 8.9e-13 (bound 1e-9), Darcy Q 7.0e-11 (bound 1e-9), solutions 2.3e-12 (bound 1e-8); iteration counts
  canonical | re-laid, hex: sampler level 1 [35, 35, 35] | the same under all four layouts, level 0 warm-started
  [49, 47, 49] | the same; Darcy saddle [[59, 59, 59], [54, 54, 55]] | the same; renumbered: sampler the same, Darcy
  [[59, 60, 59], [55, 54, 54]];
- d. mass_sensitivity at most 0.044 of its bound, mass_tangent 0.113; gradient 7.7e-11 (bounds 2.3e-10 / 2.6e-10), hv
  3.3e-11 (1.5e-9 / 8.6e-10), dG 4.0e-11 (1.7e-9 / 1.4e-9);
- e. ComputeG 1.1e-12 / 1.5e-12 absolute; L2 projection 2.3e-13 (bound 1e-9), ComputeL2Error 2.5e-15 (bound 1e-12);
  Conditioner K 7.3e-13, A 2.6e-13 (bound 1e-8), bit for bit the canonical K, A under reverse and random;
- f. 14 results per handle (21 on the three agglomerated levels) bit for bit equal under reverse / random / diag_first of
  M, B (H, G); 10 per Darcy handle under reverse / random of B;
- g. renumbered hex: operators 1.85 / 1.95 eps, preconditioners 3.2e-16 (sampler), 5.1e-16 / 1.9e-9 (Darcy), fields 5.2e-13;
  hybridized sampler: operator 2.23 eps, preconditioner 2.7e-14, fields 6.0e-13, iterations [11, 11, 11] / [24, 23, 24].
The whole file takes 6.5 s, no test more than 0.4 s.

Mutation check (each change built once into a copy of the library and this file run against it on an MI355X, none
committed).  Removing a csr_sort_rows call changes no result beyond rounding - the setup works on any order - so what
catches it is the bitwise claim of f, failing first at the named result:
- sampler.hip M (:258), B (:259): test_sampler_results_do_not_depend_on_the_order_of_sorted_members[hex- / tet- /
  agg-sampler], 'reverse', level 0, Mult;
- sampler.hip H (:383): the same test [hex-hybrid, tet-hybrid], level 0, Mult; G (:384): [hex-hybrid] level 1 Eval,
  [tet-hybrid] level 0 Eval statistics;
- darcy.hip Bfull (:333): test_darcy_results_do_not_depend_on_the_order_of_B[hex-False, tet-False], level 0,
  ApplyOperator; B of build_hybrid (:844): [hex-True] level 0 solution, [tet-True] level 0 Q;
- condition.hip H0 (:506): test_conditioner_with_observations_in_other_layouts (K, A bit for bit);
- darcy.hip PL (:931): NOT caught, and cannot be - behind the sorted B of :844 the rows of PL are filled in ascending face
  order and the multiplier numbering is monotone in the face number, so the rows are sorted before the call;
- sell_build taking the first instead of the last matching entry as dpos: cannot differ - a row holds its diagonal column
  once, since csr_from_c refuses a second one.
"""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import layout_cases as lc
from precond_cases import REF_TOL, Handle as _Handle, darcy_fields as _fields, rel as _rel

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SEED = 23
TIGHT = dict(rel_tol=1e-12, abs_tol=1e-30, max_iter=400)          # test_gpu_parity.py
TIGHT_GRAD = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)     # test_gpu_darcy_gradient.py / _gn_hessian.py
MAX_ITER_AGG = 600                                                 # ... and their iteration limit on agglomerated levels
NOISE = 0.01
CORLEN = 0.5
KINDS = ("hex", "tet", "agg")
BC = ([0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])


@pytest.fixture(scope="module")
def cases(hex_hierarchy_small):
    """kind -> dict(h: the hierarchy or None, sampler, hybrid (or None), darcy): the canonical problems"""
    import derivative_family_cases as dfc
    import tracer_cases
    from parelagmc_amd.fe import build_darcy_problem, build_hybrid_sampler_problem, build_sampler_problem
    out = {}
    for kind, h in (("hex", hex_hierarchy_small), ("tet", tracer_cases.hierarchy("tet1"))):
        dp = build_darcy_problem(h, *BC)
        rng = np.random.default_rng(3)
        levels = [dataclasses.replace(L, ess_data=np.where(L.ess_mask.astype(bool), rng.standard_normal(L.n_u), 0.0))
                  for L in dp.levels]                      # nonzero essential fluxes, as the derivative tests set them
        # corlen 0.5: level 0 of the saddle-point handles is not reaction-dominated (Gershgorin ratio 73 / 58 against the 40
        # below which a small level ends the cycle with a polynomial), so the preconditioner runs the V-cycle through P
        out[kind] = dict(h=h, sampler=build_sampler_problem(h, corlen=CORLEN), darcy=dataclasses.replace(dp, levels=levels),
                         hybrid=build_hybrid_sampler_problem(h, corlen=CORLEN))
    out["agg"] = dict(h=None, sampler=dfc.sampler_problem("agg-unit", False), hybrid=None, darcy=dfc.problem("agg2"))
    return out


def _variants(p, renumber=False):
    """[(label, problem for the handle, problem for the reference, perms)]: the canonical problem and its four layouts
    (reference: the canonical problem), or the renumbered problem (reference: itself)"""
    if renumber:
        q, perms = lc.renumber_problem(p, SEED)
        return [("canonical", p, p, None), ("renumbered", q, q, perms)]
    return [("canonical", p, p, None)] + [(lay, lc.relayout_problem(p, lay, SEED), p, None) for lay in lc.LAYOUTS]


def _widths(top):
    return sorted({1, min(8, top), top})


def _cols(nb):
    return sorted({c for c in (0, 1, nb - 1, 7, 8, 31, 32, 63, 64, 127, 128) if c < nb})


def _opts(storage="fp32", **kw):
    from parelagmc_amd import capi
    st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
    return capi.solver_opts(precond_storage=st, **kw)


def _tight(kind, base=TIGHT):
    return dict(base, max_iter=MAX_ITER_AGG) if kind == "agg" else base


# ------------------------------------------------------------------------------------------------------------ a. operators
def _check_sampler_operator(ctx, label, q, ref):
    """Mult of a handle on q against scipy on the block operator (H) of `ref`; returns the largest error / (|A||x|)"""
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd import capi
    hybrid = hasattr(ref.levels[0], "n_lambda")
    smp = capi.PDESampler(ctx, q)
    worst = 0.0
    for lvl in range(smp.nlevels):
        A = ref.levels[lvl].H.tocsr() if hybrid else SamplerOracle(ref).block_operator(lvl).tocsr()
        top = smp.BatchWidth(lvl)
        x = np.random.default_rng(SEED + lvl).standard_normal((top, A.shape[0]))
        for nb in _widths(top):
            y = smp.Mult(lvl, x[:nb])[0]
            err = float(np.max(np.abs(y - (A @ x[:nb].T).T) / (abs(A) @ np.abs(x[:nb].T)).T))
            worst = max(worst, err)
            assert err < 8 * EPS, (label, lvl, nb, err / EPS)
        assert hybrid or smp.GetNNZ(lvl) == q.levels[lvl].nnz        # stored zeros count: they are stored
    smp.close()
    return worst


def _check_darcy_operator(ctx, kind, label, q, ref, h, hybrid, cache):
    """ApplyOperator of a handle on q against the assembled matrix of every compared column (its own k) of `ref`"""
    from oracle.darcy_oracle import DarcyOracle
    from parelagmc_amd import capi
    from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
    do = DarcyOracle(ref)
    ds = capi.DarcySolver(ctx, q, hybrid=hybrid)
    worst = worst_l2 = 0.0
    for lvl in range(ds.nlevels):
        L = ref.levels[lvl]
        hl = darcy_hybrid_level(h.spaces[lvl], L) if hybrid else None
        hl_abs = dataclasses.replace(hl, h_val=np.abs(hl.h_val)) if hybrid else None
        n = hl.n_lambda if hybrid else L.n_u + L.n_p
        top = ds.BatchWidth(lvl)
        rng = np.random.default_rng(SEED + lvl)
        k, x = _fields(rng, top, L.n_p), rng.standard_normal((top, n))
        for nb in _widths(top):
            y = ds.ApplyOperator(lvl, k[:nb], x[:nb])
            for j in _cols(nb):
                if (id(ref), lvl, j) not in cache:
                    if hybrid:
                        kappa = k[j] if ref.k_divides else 1.0 / k[j]
                        A, absA = hl.operator(kappa), hl_abs.operator(kappa)
                    else:
                        A = do.assemble(lvl, k[j])[0].tocsr()
                        absA = abs(A)
                    cache[(id(ref), lvl, j)] = (A @ x[j], absA @ np.abs(x[j]))
                want, scale = cache[(id(ref), lvl, j)]
                err = float(np.max(np.abs(y[j] - want) / scale))
                worst, worst_l2 = max(worst, err), max(worst_l2, _rel(y[j], want))
                if hybrid and kind == "tet":
                    assert _rel(y[j], want) < 1e-13, (label, lvl, nb, j, _rel(y[j], want))
                else:
                    assert err < 8 * EPS, (label, lvl, nb, j, err / EPS)
    ds.close()
    return worst, worst_l2


@pytest.mark.parametrize("kind", KINDS)
def test_sampler_operators_of_relaid_handles(gpu_ctx, cases, kind):
    for name in ("sampler", "hybrid"):
        p = cases[kind][name]
        if p is None:
            continue
        for label, q, ref, _ in _variants(p):
            worst = _check_sampler_operator(gpu_ctx, label, q, ref)
            print(f"a. sampler operator {kind} {name} {label}: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps (bound 8)")


@pytest.mark.parametrize("kind", KINDS)
def test_darcy_operators_of_relaid_handles(gpu_ctx, cases, kind):
    p, h = cases[kind]["darcy"], cases[kind]["h"]
    for hybrid in ((False, True) if h is not None else (False,)):
        cache = {}
        for label, q, ref, _ in _variants(p):
            worst, l2 = _check_darcy_operator(gpu_ctx, kind, label, q, ref, h, hybrid, cache)
            print(f"a. darcy operator {kind} hybrid={hybrid} {label}: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps (bound 8),"
                  f" max rel L2 = {l2:.2e}")


# ------------------------------------------------------------------------------------------------------ b. preconditioners
def _check_sampler_precond(ctx, label, q, ref, storage):
    """ApplyPreconditioner of MC level 0 against SamplerPrecondOracle(ref, the handle's setup values and prolongators)"""
    from oracle.precond_oracle import ROLE_DESCEND, SamplerPrecondOracle
    hd = _Handle(ctx, label, storage, problem=q)
    oracle = SamplerPrecondOracle(ref, 0, hd.setup, hd.P, hd.opts.schur_scale)
    r = np.random.default_rng(SEED).standard_normal((hd.top, hd.n))
    worst = 0.0
    for nb in sorted({1, hd.top}):
        z = hd.smp.ApplyPreconditioner(0, r[:nb])
        for j in _cols(nb):
            e = _rel(z[j], oracle.apply(r[j], hd.narrow(nb)))
            worst = max(worst, e)
            assert e <= REF_TOL[storage], (label, storage, nb, j, e)
    role = (int(hd.setup[0]["role_wide"]), hd.info[0]["in_tail"], hd.info[0]["fused_restriction"])
    if not hd.hybrid:
        assert role[0] == ROLE_DESCEND, "level 0 ends the cycle: the preconditioner would not read P at all"
    hd.smp.close()
    return worst, role


@pytest.mark.parametrize("kind", KINDS)
def test_sampler_preconditioners_of_relaid_handles(gpu_ctx, cases, kind):
    for name in ("sampler", "hybrid"):
        p = cases[kind][name]
        if p is None:
            continue
        for storage in ("fp64", "fp32"):
            for label, q, ref, _ in _variants(p):
                worst, role = _check_sampler_precond(gpu_ctx, label, q, ref, storage)
                print(f"b. sampler preconditioner {kind} {name} {storage} {label}: max rel L2 = {worst:.2e} (bound "
                      f"{REF_TOL[storage]:.0e}), level 0 (role_wide, in_tail, fused_restriction) = {role}")


def _check_darcy_precond(ctx, label, q, ref, storage):
    """ApplyPreconditioner of every MC level against DarcyPrecondOracle(ref), every compared column with its own k; the
    closed-form setup values as test_gpu_precond.py asserts them, ratio_M from the handle"""
    from oracle.precond_oracle import GALERKIN_SCALE, LMAX_SCHUR, DarcyPrecondOracle
    from parelagmc_amd import capi
    o = _opts(storage)
    po = DarcyPrecondOracle(ref, o.mg_smooth_degree, o.mg_smooth_ratio, o.mg_coarse_degree, o.mg_coarse_ratio)
    ds = capi.DarcySolver(ctx, q, o)
    worst = 0.0
    for lvl in range(ds.nlevels):
        info = ds.vcycle_levels(lvl)
        assert len(info) == len(ref.levels) - lvl
        for v, m in enumerate(info):
            assert m["hierarchy"] == 0 and m["rows"] == ref.levels[lvl + v].n_p
            assert m["lmax"] == LMAX_SCHUR and m["galerkin_scale"] == GALERKIN_SCALE
        ratio_M, deg_M = info[0]["ratio_M"], int(info[0]["degree_M"])
        L = ref.levels[lvl]
        top = ds.BatchWidth(lvl)
        rng = np.random.default_rng(SEED + lvl)
        k, r = _fields(rng, top, L.n_p), rng.standard_normal((top, L.n_u + L.n_p))
        for nb in sorted({1, top}):
            z = ds.ApplyPreconditioner(lvl, k[:nb], r[:nb])
            for j in _cols(nb)[:6]:
                e = _rel(z[j], po.apply(lvl, k[j], r[j], ratio_M, deg_M))
                worst = max(worst, e)
                assert e <= REF_TOL[storage], (label, storage, lvl, nb, j, e)
    ds.close()
    return worst


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_darcy_preconditioners_of_relaid_handles(gpu_ctx, cases, kind, storage):
    for label, q, ref, _ in _variants(cases[kind]["darcy"]):
        worst = _check_darcy_precond(gpu_ctx, label, q, ref, storage)
        print(f"b. darcy preconditioner {kind} {storage} {label}: max rel L2 = {worst:.2e} (bound {REF_TOL[storage]:.0e})")


# --------------------------------------------------------------------------------------------------------------- c. solves
def _check_sampler_solves(ctx, kind, label, q, ref, perms, cache):
    """Eval on level 1 from level-0 xi, then level 0 warm-started from that field, against SamplerOracle(ref); returns
    (largest relative L2 error, iteration counts)"""
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd import capi
    sref = cache.get(("so", id(ref)))
    if sref is None:
        hyb = hasattr(ref.levels[0], "n_lambda")
        # the hybridized problem is an exact reformulation of the saddle-point one: same oracle (the canonical saddle problem)
        sref = cache[("so", id(ref))] = SamplerOracle(cache["saddle"] if hyb else ref)
    smp = capi.PDESampler(ctx, q, capi.solver_opts(**_tight(kind)))
    xi = np.random.default_rng(SEED).standard_normal((3, ref.levels[0].n_s))
    if perms is not None:
        xi = xi[:, perms[0][0]]
    s1, e1, st1 = smp.Eval(1, xi, xi_level=0, want_embed=True, return_stats=True)
    s0, st0 = smp.Eval(0, xi, xi_level=0, init_s=e1, init_level=1, use_init=True, return_stats=True)
    worst = 0.0
    for lvl, s, st in ((1, s1, st1), (0, s0, st0)):
        key = ("s", id(ref), lvl)
        if key not in cache:
            cache[key] = np.stack([sref.eval(lvl, 0, x)[0] for x in xi])
        e = _rel(s, cache[key])
        worst = max(worst, e)
        assert e < 1e-9, (label, lvl, e)
        assert all(t[1] == 1 for t in st), (label, lvl, st)
    smp.close()
    return worst, [t[0] for t in st1], [t[0] for t in st0]


@pytest.mark.parametrize("kind", KINDS)
def test_sampler_solves_of_relaid_handles(gpu_ctx, cases, kind):
    for name in ("sampler", "hybrid"):
        p = cases[kind][name]
        if p is None:
            continue
        cache = {"saddle": cases[kind]["sampler"]}
        for label, q, ref, perms in _variants(p):
            worst, it1, it0 = _check_sampler_solves(gpu_ctx, kind, label, q, ref, perms, cache)
            print(f"c. sampler Eval {kind} {name} {label}: max rel L2 = {worst:.2e} (bound 1e-9), iterations level 1 {it1}, "
                  f"level 0 warm-started {it0}")


def _check_darcy_solves(ctx, kind, label, q, ref, perms, hybrid, cache):
    from oracle.darcy_oracle import DarcyOracle
    from parelagmc_amd import capi
    do = DarcyOracle(ref)
    ds = capi.DarcySolver(ctx, q, capi.solver_opts(**_tight(kind)), hybrid=hybrid)
    worst_q = worst_x = 0.0
    its = []
    for lvl in range(ds.nlevels):
        L = ref.levels[lvl]
        k = np.exp(np.random.default_rng(SEED + lvl).standard_normal((3, L.n_p)))
        Q, C, sol, st = ds.SolveFwd(lvl, k, want_solution=True, return_stats=True)
        for b in range(3):
            if (id(ref), lvl, b) not in cache:
                cache[(id(ref), lvl, b)] = do.solve_fwd(lvl, k[b], return_solution=True)
            Qr, Cr, xr = cache[(id(ref), lvl, b)]
            worst_q, worst_x = max(worst_q, abs(Q[b] - Qr) / abs(Qr)), max(worst_x, _rel(sol[b], xr))
            assert abs(Q[b] - Qr) < 1e-9 * abs(Qr) and C[b] == Cr, (label, lvl, b, Q[b], Qr)
            assert _rel(sol[b], xr) < 1e-8, (label, lvl, b, _rel(sol[b], xr))
        assert all(t[1] == 1 for t in st), (label, lvl, st)
        its.append([t[0] for t in st])
    ds.close()
    return worst_q, worst_x, its


@pytest.mark.parametrize("kind", KINDS)
def test_darcy_solves_of_relaid_handles(gpu_ctx, cases, kind):
    p, h = cases[kind]["darcy"], cases[kind]["h"]
    for hybrid in ((False, True) if h is not None else (False,)):
        cache = {}
        for label, q, ref, perms in _variants(p):
            wq, wx, its = _check_darcy_solves(gpu_ctx, kind, label, q, ref, perms, hybrid, cache)
            print(f"c. darcy SolveFwd {kind} hybrid={hybrid} {label}: max rel error Q {wq:.2e} (bound 1e-9), solution {wx:.2e} "
                  f"(bound 1e-8), iterations per level {its}")


# --------------------------------------------------------------------------------------------------- d. derivative kernels
def _derivative_tols(kind):
    import test_gpu_darcy_gn_hessian as th
    import test_gpu_darcy_gradient as tg
    if kind == "agg":
        return tg.TOL_GRAD_FAMILY["agg"], th.TOL_HV_FAMILY["agg"], th.TOL_DG_FAMILY["agg"]
    return tg.TOL_GRAD, th.TOL_HV, th.TOL_DG


@pytest.mark.parametrize("k_divides", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_derivative_kernels_of_relaid_handles(gpu_ctx, cases, kind, k_divides):
    """the kernels that read the moved contribution lists most directly, on the level with the widest rows (agg: level 1,
    elements of 12 to 5 faces; else level 0)"""
    import derivative_family_cases as dfc
    from parelagmc_amd import capi
    from parelagmc_amd.fe import darcy_adjoint as da
    p = dataclasses.replace(cases[kind]["darcy"], k_divides=k_divides)
    level = 1 if kind == "agg" else 0
    L = p.levels[level]
    n, nb = L.n_u + L.n_p, 4
    ess = L.ess_mask.astype(bool)
    n_fe = da.element_matrices(L)[0].shape[1]
    nside = dfc.structure(L)[2]
    assert nside == 2
    tol_g, tol_hv, tol_dg = _derivative_tols(kind)
    rng = np.random.default_rng(SEED)
    k, dk = np.exp(rng.standard_normal((nb, L.n_p))), rng.standard_normal((nb, L.n_p))
    x, lam = rng.standard_normal((nb, n)), rng.standard_normal((nb, n))
    a, b, c = L.n_p // 3, (2 * L.n_p) // 3, (2 * L.n_p) // 3 + 1
    Gobs = sp.csr_matrix(([1.0, 0.5, 2.0], ([0, 1, 1], [a, b, c])), shape=(2, L.n_p))
    # references, once: the long-double twins of the kernels, the direct-solve twins of the two solves
    ld = np.longdouble
    g_ref = {w: da.mass_sensitivity(L, k, x, lam, k_divides, w, return_abs=True, dtype=ld) for w in (False, True)}
    t_ref = {w: da.mass_tangent(L, k, x, dk, k_divides, w, return_abs=True, dtype=ld) for w in (False, True)}
    grad_ref = np.stack([da.gradient(p, level, k[j]) for j in range(nb)])
    hv_ref = [da.gn_hessvec(p, level, k[j], dk[j], Gobs, NOISE, return_all=True) for j in range(nb)]
    free = np.zeros(n, bool)
    free[:L.n_u] = ~ess
    h = cases[kind]["h"]
    for hybrid in ((False, True) if h is not None else (False,)):
        for label, q, _, _ in _variants(p):
            ds = capi.DarcySolver(gpu_ctx, q, capi.solver_opts(**_tight(kind, TIGHT_GRAD)), hybrid=hybrid)
            worst = dict(g=0.0, t=0.0)
            for w in (False, True):
                g = ds.mass_sensitivity(level, k, x, lam, w)
                bound = (n_fe * n_fe + 3) * 2.0 ** -52 * g_ref[w][1]
                err = np.abs(g.astype(ld) - g_ref[w][0])
                worst["g"] = max(worst["g"], float(np.max(err / bound)))
                assert np.all(err <= bound), (label, hybrid, w, float(np.max(err / bound)))
                t = ds.mass_tangent(level, k, x, dk, w)
                bound = (nside * n_fe + 3) * 2.0 ** -52 * t_ref[w][1]
                err = np.abs(t.astype(ld) - t_ref[w][0])
                worst["t"] = max(worst["t"], float(np.max(err[:, free] / bound[:, free])))
                assert np.all(err <= bound), (label, hybrid, w, worst["t"])
                assert np.all(t[:, ~free] == 0.0)
            Q, Cc, grad, st_f, st_a = ds.solve_gradient(level, k, return_stats=True)
            assert all(s[1] == 1 for s in st_f + st_a), (label, hybrid, st_f, st_a)
            e_g = max(_rel(grad[j], grad_ref[j]) for j in range(nb))
            assert e_g < tol_g, (label, hybrid, e_g)
            ds.SetObservations(level, Gobs)
            hv, dG, st_t, st_h = ds.gn_hessvec(level, k, dk, NOISE, return_stats=True)
            assert all(s[1] == 1 for s in st_t + st_h), (label, hybrid, st_t, st_h)
            e_hv = max(_rel(hv[j], hv_ref[j][0]) for j in range(nb))
            e_dg = max(_rel(dG[j], hv_ref[j][1]) for j in range(nb))
            assert e_hv < tol_hv and e_dg < tol_dg, (label, hybrid, e_hv, e_dg)
            print(f"d. derivatives {kind} k_divides={k_divides} hybrid={hybrid} {label}: mass_sensitivity error / bound "
                  f"{worst['g']:.3f}, mass_tangent {worst['t']:.3f}, gradient rel {e_g:.2e} (bound {tol_g:.1e}), hv {e_hv:.2e} "
                  f"(bound {tol_hv:.1e}), dG {e_dg:.2e} (bound {tol_dg:.1e})")
            ds.close()


# --------------------------------------------------------------------------------------------------------------- f. bitwise
def _order_only(p, layout):
    """p with M, B (H, G) of every level in `layout` and P as the caller's: what the sampler sorts at create, nothing else"""
    q = lc.relayout_problem(p, layout, SEED)
    return dataclasses.replace(q, levels=[dataclasses.replace(Lq, P=L.P) for Lq, L in zip(q.levels, p.levels)])


@pytest.mark.parametrize("kind,name", [("hex", "sampler"), ("hex", "hybrid"), ("tet", "sampler"), ("tet", "hybrid"),
                                       ("agg", "sampler")])
def test_sampler_results_do_not_depend_on_the_order_of_sorted_members(gpu_ctx, cases, kind, name):
    """the sampler sorts M, B (H, G) at create: handles that differ only in the order of those four return the same bits -
    operator, preconditioner, fields, solver statistics, field statistics.  If this fails, something reads the caller's
    order that should not."""
    from parelagmc_amd import capi
    p = cases[kind][name]

    def results(q):
        smp = capi.PDESampler(gpu_ctx, q)
        out = []
        for lvl in range(smp.nlevels):
            L = q.levels[lvl]
            n = L.n_lambda if smp.hybrid else L.n_u + L.n_s
            nb = smp.BatchWidth(lvl)
            r = np.random.default_rng(SEED + lvl).standard_normal((nb, n))
            out += [smp.Mult(lvl, r)[0], smp.ApplyPreconditioner(lvl, r), smp.ApplyPreconditioner(lvl, r[:1])]
            xi = np.random.default_rng(SEED).standard_normal((5, q.levels[0].n_s))
            s, st = smp.Eval(lvl, xi, xi_level=0, return_stats=True)
            out += [s, np.array(st, dtype=np.float64)]
            fs = capi.FieldStatistics(smp, lvl)
            e, m2, _, cnt = fs.run(0, 12).read()
            assert cnt == 12
            out += [e, m2]
            fs.close()
        smp.close()
        return out

    base = results(p)
    assert all(np.all(np.isfinite(v)) for v in base)
    names = ("Mult", "ApplyPreconditioner", "ApplyPreconditioner width 1", "Eval", "Eval statistics", "expectation",
             "second moment")
    for layout in lc.ORDERS:
        got = results(_order_only(p, layout))
        for i, (u, v) in enumerate(zip(got, base)):
            assert np.array_equal(u, v), (kind, name, layout, f"level {i // len(names)}", names[i % len(names)])
    print(f"f. bitwise {kind} {name}: {len(base)} results equal under {lc.ORDERS}")


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_darcy_results_do_not_depend_on_the_order_of_B(gpu_ctx, cases, kind, hybrid):
    """the Darcy handles sort B at create (the saddle-point setup and the hybridized one), and everything they derive from it
    - the eliminated B and B^T, the symbolic Schur lists, the element-local face order of the hybridized form - comes from
    the sorted copy: handles that differ only in the order of B return the same bits"""
    from parelagmc_amd import capi
    p = cases[kind]["darcy"]

    def results(q):
        ds = capi.DarcySolver(gpu_ctx, q, capi.solver_opts(**TIGHT), hybrid=hybrid)
        out = []
        for lvl in range(ds.nlevels):
            L = q.levels[lvl]
            nb = ds.BatchWidth(lvl)
            rng = np.random.default_rng(SEED + lvl)
            k = _fields(rng, nb, L.n_p)
            Q, _, sol, st = ds.SolveFwd(lvl, k[:3], want_solution=True, return_stats=True)
            out += [Q, sol, np.array(st, dtype=np.float64)]
            n = _rows_of(q, lvl, hybrid)
            r = rng.standard_normal((nb, n))
            out += [ds.ApplyOperator(lvl, k, r), ds.ApplyPreconditioner(lvl, k, r)]
        ds.close()
        return out

    base = results(p)
    assert all(np.all(np.isfinite(v)) for v in base)
    names = ("Q", "solution", "solver statistics", "ApplyOperator", "ApplyPreconditioner")
    for order in lc.ORDERS[:2]:
        rng = np.random.default_rng(SEED)
        q = dataclasses.replace(p, levels=[dataclasses.replace(L, B=lc.relayout_csr(L.B, order, rng)) for L in p.levels])
        for i, (u, v) in enumerate(zip(results(q), base)):
            assert np.array_equal(u, v), (kind, hybrid, order, f"level {i // len(names)}", names[i % len(names)])
    print(f"f. bitwise darcy {kind} hybrid={hybrid}: {len(base)} results equal under {lc.ORDERS[:2]} of B")


def _rows_of(q, lvl, hybrid):
    """rows of the operator of a Darcy handle: n_u + n_p, or the multipliers (interior and essential faces)"""
    L = q.levels[lvl]
    if not hybrid:
        return L.n_u + L.n_p
    sides = np.bincount(L.B.tocsr().indices, minlength=L.n_u)
    return int(np.count_nonzero((sides == 2) | L.ess_mask.astype(bool)))


# ----------------------------------------------------------------------------------------------------------- g. renumbering
def test_renumbered_sampler_handles(gpu_ctx, cases):
    """a, b, c on the renumbered hex sampler problem, saddle-point handles, against oracles of the renumbered problem"""
    p = cases["hex"]["sampler"]
    (_, _, _, _), (label, q, ref, perms) = _variants(p, renumber=True)
    assert lc.is_oct_injection(p.levels[0].P) and not lc.is_oct_injection(q.levels[0].P)
    worst = _check_sampler_operator(gpu_ctx, label, q, ref)
    print(f"g. sampler operator hex {label}: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps (bound 8)")
    for storage in ("fp64", "fp32"):
        for lab, qq, rr in (("canonical", p, p), (label, q, ref)):
            w, role = _check_sampler_precond(gpu_ctx, lab, qq, rr, storage)
            print(f"g. sampler preconditioner hex {storage} {lab}: max rel L2 = {w:.2e} (bound {REF_TOL[storage]:.0e}), "
                  f"level 0 (role_wide, in_tail, fused_restriction) = {role}")
    for lab, qq, rr, pp in (("canonical", p, p, None), (label, q, ref, perms)):
        w, it1, it0 = _check_sampler_solves(gpu_ctx, "hex", lab, qq, rr, pp, {})
        print(f"g. sampler Eval hex {lab}: max rel L2 = {w:.2e} (bound 1e-9), iterations level 1 {it1}, level 0 {it0}")


def test_renumbered_hybridized_sampler_handle(gpu_ctx, cases):
    """the same for the hybridized sampler: H and the preconditioner against the renumbered problem, the fields against the
    canonical saddle-point oracle's, permuted (the direct solve of the other ordering agrees to 1e-12:
    tests/test_layout_cases.py)"""
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd import capi
    p = cases["hex"]["hybrid"]
    q, perms = lc.renumber_problem(p, SEED)
    worst = _check_sampler_operator(gpu_ctx, "renumbered", q, q)
    print(f"g. sampler operator hex hybrid renumbered: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps (bound 8)")
    for storage in ("fp64", "fp32"):
        w, role = _check_sampler_precond(gpu_ctx, "renumbered", q, q, storage)
        print(f"g. sampler preconditioner hex hybrid {storage} renumbered: max rel L2 = {w:.2e} (bound {REF_TOL[storage]:.0e})")
    so = SamplerOracle(cases["hex"]["sampler"])
    xi = np.random.default_rng(SEED).standard_normal((3, p.levels[0].n_s))
    smp = capi.PDESampler(gpu_ctx, q, capi.solver_opts(**TIGHT))
    for lvl in (1, 0):
        s, st = smp.Eval(lvl, xi[:, perms[0][0]], xi_level=0, return_stats=True)
        ref = np.stack([so.eval(lvl, 0, x)[0] for x in xi])[:, perms[lvl][0]]
        assert _rel(s, ref) < 1e-9 and all(t[1] == 1 for t in st), (lvl, _rel(s, ref), st)
        print(f"g. sampler Eval hex hybrid renumbered level {lvl}: rel L2 = {_rel(s, ref):.2e} (bound 1e-9), iterations "
              f"{[t[0] for t in st]}")
    smp.close()


def test_renumbered_darcy_handles(gpu_ctx, cases):
    p = cases["hex"]["darcy"]
    (_, _, _, _), (label, q, ref, perms) = _variants(p, renumber=True)
    assert lc.is_oct_injection(p.levels[0].P) and not lc.is_oct_injection(q.levels[0].P)
    worst, l2 = _check_darcy_operator(gpu_ctx, "hex", label, q, ref, None, False, {})
    print(f"g. darcy operator hex {label}: max |y - Ax| / (|A||x|) = {worst / EPS:.2f} eps (bound 8)")
    for storage in ("fp64", "fp32"):
        w = _check_darcy_precond(gpu_ctx, label, q, ref, storage)
        print(f"g. darcy preconditioner hex {storage} {label}: max rel L2 = {w:.2e} (bound {REF_TOL[storage]:.0e})")
    for lab, qq, rr, pp in (("canonical", p, p, None), (label, q, ref, perms)):
        wq, wx, its = _check_darcy_solves(gpu_ctx, "hex", lab, qq, rr, pp, False, {})
        print(f"g. darcy SolveFwd hex {lab}: max rel error Q {wq:.2e} (bound 1e-9), solution {wx:.2e} (bound 1e-8), "
              f"iterations per level {its}")


# ------------------------------------------------------------------------------------------------------------- duplicates
def test_create_functions_refuse_a_column_stored_twice(gpu_ctx, cases):
    """include/pmc.h: a column may appear once per row.  One duplicated entry (the value split in two halves; the list of an
    M_pattern entry split in two) in M, B, P, H, G, M_pattern: PMC_ERR_INVALID with a message, from every create function"""
    from parelagmc_amd import capi
    sp_, hp, dp = (cases["hex"][n] for n in ("sampler", "hybrid", "darcy"))

    def with_member(p, lvl, **new):
        levels = list(p.levels)
        levels[lvl] = dataclasses.replace(levels[lvl], **new)
        return dataclasses.replace(p, levels=levels)

    L = dp.levels[1]
    pat, lists = lc.duplicated_entry(L.M_pattern, lists=(L.c_ptr, L.c_elem, L.c_val))
    bad = [("sampler M", capi.PDESampler, with_member(sp_, 1, M=lc.duplicated_entry(sp_.levels[1].M)), {}),
           ("sampler B", capi.PDESampler, with_member(sp_, 0, B=lc.duplicated_entry(sp_.levels[0].B)), {}),
           ("sampler P", capi.PDESampler, with_member(sp_, 0, P=lc.duplicated_entry(sp_.levels[0].P)), {}),
           ("hybrid H", capi.PDESampler, with_member(hp, 0, H=lc.duplicated_entry(hp.levels[0].H)), {}),
           ("hybrid G", capi.PDESampler, with_member(hp, 1, G=lc.duplicated_entry(hp.levels[1].G)), {}),
           ("darcy M_pattern", capi.DarcySolver,
            with_member(dp, 1, M_pattern=pat, c_ptr=lists[0], c_elem=lists[1], c_val=lists[2]), {}),
           ("darcy M_pattern", capi.DarcySolver,
            with_member(dp, 1, M_pattern=pat, c_ptr=lists[0], c_elem=lists[1], c_val=lists[2]), dict(hybrid=True)),
           ("darcy B", capi.DarcySolver, with_member(dp, 0, B=lc.duplicated_entry(dp.levels[0].B)), {}),
           ("darcy P", capi.DarcySolver, with_member(dp, 0, P=lc.duplicated_entry(dp.levels[0].P)), {})]
    for what, create, q, kw in bad:
        with pytest.raises(capi.PmcError) as e:
            create(gpu_ctx, q, **kw)
        assert e.value.code == -1 and what in str(e.value) and "appears twice in row" in str(e.value), (what, str(e.value))


# -------------------------------------------------------------------------- e. entry points that take a CSR of their own
def _csr_layouts(A):
    """[(label, A')] of one bare matrix: every order it can take, and stored zeros (one per row) in random order"""
    rng = np.random.default_rng(SEED)
    orders = lc.ORDERS if A.shape[0] == A.shape[1] else lc.ORDERS[:2]
    out = [(o, lc.relayout_csr(A, o, rng)) for o in orders]
    return out + [("zeros", lc.relayout_csr(lc.with_stored_zeros(A, rng, 1), "random", rng))]


def test_observation_functionals_in_other_layouts(gpu_ctx, cases, hex_hierarchy_small):
    """SetObservations + ComputeG with a re-laid Gobs (rows of several elements) against the oracle, at the bound of
    test_gpu_parity.py::test_bayesian_observation_operator_and_likelihood"""
    from oracle.bayes_oracle import compute_G, observation_functionals
    from oracle.darcy_oracle import DarcyOracle
    from parelagmc_amd import capi
    dp = cases["hex"]["darcy"]
    do = DarcyOracle(dp)
    Gobs = observation_functionals(hex_hierarchy_small, np.array([[0.5, 0.5, 0.5], [1.5, 1.0, 0.4], [1.0, 1.6, 1.7]]), eps=0.3)
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(**TIGHT))
    for lvl in range(2):
        assert np.diff(Gobs[lvl].tocsr().indptr).max() >= 2
        k = np.exp(0.5 * np.random.default_rng(SEED + lvl).standard_normal((5, dp.levels[lvl].n_p)))
        ref = [compute_G(do, Gobs, lvl, kk) for kk in k]
        for label, G2 in [("canonical", Gobs[lvl].tocsr())] + _csr_layouts(Gobs[lvl].tocsr()):
            ds.SetObservations(lvl, G2)
            G, C, Q = ds.ComputeG(lvl, k)
            assert np.allclose(G, np.stack([r[0] for r in ref]), rtol=1e-8, atol=1e-10), (lvl, label)
            assert np.allclose(Q, [r[2] for r in ref], rtol=1e-8) and np.all(C == dp.levels[lvl].ndofs), (lvl, label)
            print(f"e. ComputeG level {lvl} Gobs {label}: max |G - ref| = {np.max(np.abs(G - np.stack([r[0] for r in ref]))):.2e}")
    ds.close()


def test_projection_and_output_hierarchy_in_other_layouts(gpu_ctx):
    """set_projection (L2) with a re-laid Gt on a non-matching pair (cube_hex_enlarge 10^3 / 5^3 projected to cube_hex 8^3 /
    4^3: rows of Gt hold up to 8 overlaps) against the oracle's projection at 1e-9 (test_gpu_parity.py), then
    SetOutputHierarchy + ComputeL2Error with the re-laid prolongators of the original mesh against numpy at rtol 1e-12
    (test_gpu_field_stats.py)"""
    from conftest import golden_path
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_hierarchy, build_sampler_problem, l2_projection_hierarchy, mesh_from_json
    ho = build_hierarchy(mesh_from_json(golden_path("meshes", "cube_hex.json")), 1)
    he = build_hierarchy(mesh_from_json(golden_path("meshes", "cube_hex_enlarge.json")), 1)
    sp_ = build_sampler_problem(he, corlen=0.1, lognormal=True)
    ops = l2_projection_hierarchy(ho, he)
    assert np.diff(ops[0][0].tocsr().indptr).max() >= 2
    so = SamplerOracle(sp_)
    xi = np.random.default_rng(SEED).standard_normal((3, sp_.levels[0].n_s))
    ref = [np.stack([so.eval(lvl, 0, x, projection=("l2",) + tuple(ops[lvl]))[0] for x in xi]) for lvl in range(2)]
    w0 = ho.spaces[0].vol
    layouts = list(zip(*[[("canonical", op[0].tocsr())] + _csr_layouts(op[0].tocsr()) for op in ops]))
    P_layouts = dict([("canonical", ho.P[0].tocsr())] + _csr_layouts(ho.P[0].tocsr()))
    for per_level in layouts:
        label = per_level[0][0]
        l2 = [(G2, ops[lvl][1]) for lvl, (_, G2) in enumerate(per_level)]
        smp = capi.PDESampler(gpu_ctx, sp_, capi.solver_opts(**TIGHT), projection="l2", l2_ops=l2)
        worst = 0.0
        for lvl in range(2):
            s = smp.Eval(lvl, xi, xi_level=0)
            worst = max(worst, _rel(s, ref[lvl]))
            assert _rel(s, ref[lvl]) < 1e-9, (label, lvl, _rel(s, ref[lvl]))
        smp.SetOutputHierarchy([P_layouts[label]], w0)
        coeff = np.random.default_rng(SEED + 1).standard_normal((4, smp.SampleSize(1)))
        want = (((ho.P[0] @ coeff.T) - 0.3) ** 2 * w0[:, None]).sum(axis=0)
        got = smp.ComputeL2Error(1, coeff, 0.3)
        assert np.allclose(got, want, rtol=1e-12, atol=0), (label, got, want)
        print(f"e. L2 projection Gt / output P {label}: max rel L2 = {worst:.2e} (bound 1e-9), L2 error rel "
              f"{np.max(np.abs(got - want) / want):.2e} (bound 1e-12)")
        smp.close()


def test_conditioner_with_observations_in_other_layouts(gpu_ctx, cases, hex_hierarchy_small):
    """Conditioner with a re-laid H0 (point rows and two averaging rows of 8 siblings) against the numpy twin, at the bounds
    of test_gpu_condition.py::test_setup_matches_the_twin; the exported K, A of the re-laid handles equal the canonical
    ones bit for bit - condition.hip sorts H0"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.condition import Conditioner, point_observations
    h, prob = hex_hierarchy_small, cases["hex"]["hybrid"]
    parent = sp.csr_matrix(h.P[0]).indices
    sib = [np.nonzero(parent == c)[0] for c in (5, 40)]
    H0 = point_observations(h.spaces[0].n_s, [3, 77, 200, 451], [(s, np.full(s.size, 1.0 / s.size)) for s in sib])
    y = np.random.default_rng(SEED).standard_normal(H0.shape[0])
    twin = Conditioner(prob, H0, y, None)
    smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(rel_tol=1e-12, max_iter=1000))
    base = None
    for label, H2 in [("canonical", H0)] + _csr_layouts(H0)[:2]:
        cond = capi.Conditioner(smp, H2, y)
        got = []
        for lvl in range(prob.n_mc_levels):
            K, A, H = cond.level(lvl)
            assert (abs(H - twin.H[lvl])).max() <= 1e-15, (label, lvl)
            eK = (np.linalg.norm(K.T - twin.K[lvl].T, axis=-1) / np.linalg.norm(twin.K[lvl].T, axis=-1)).max()
            eA = (np.linalg.norm(A.T - twin.A[lvl].T, axis=-1) / np.linalg.norm(twin.A[lvl].T, axis=-1)).max()
            assert eK <= 1e-8 and eA <= 1e-8, (label, lvl, eK, eA)
            got += [K, A]
            print(f"e. Conditioner H0 {label} level {lvl}: K {eK:.2e} A {eA:.2e} (bound 1e-8)")
        if base is None:
            base = got
        assert all(np.array_equal(u, v) for u, v in zip(got, base)), label
        cond.close()
    smp.close()


def test_kl_sampler_and_level_fields_with_relaid_prolongators(gpu_ctx, cases, hex_hierarchy_small):
    """KLSampler with a re-laid P (it projects the modes to the coarser levels through P) against the expansion at the
    per-entry bound of test_gpu_kl.py; LevelFields.parents() of a Darcy handle whose P carries stored zeros"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_kl_sampler_problem
    prob = build_kl_sampler_problem(hex_hierarchy_small, "analytic", corlen=0.1)
    assert prob.n_mc_levels == 2
    m = prob.nmodes
    xi = np.random.default_rng(SEED).standard_normal((5, prob.levels[0].n_s))
    z = xi[:, :m] * np.sqrt(prob.evals)[None, :]
    for label, P2 in [("canonical", prob.levels[0].P.tocsr())] + _csr_layouts(prob.levels[0].P.tocsr()):
        q = dataclasses.replace(prob, levels=[dataclasses.replace(prob.levels[0], P=P2), prob.levels[1]])
        smp = capi.KLSampler(gpu_ctx, q)
        for lvl in range(2):
            phi = prob.evects[lvl]
            emb = smp.Eval(lvl, xi, xi_level=0, want_embed=True)[1]
            assert np.all(np.abs(emb - z @ phi.T) <= 8.0 * m * EPS * (np.abs(z) @ np.abs(phi).T)), (label, lvl)
        smp.close()
    dp = cases["hex"]["darcy"]
    want = dp.levels[0].P.tocsr().indices.astype(np.int64)
    for label in ("canonical", "zeros"):
        q = dp if label == "canonical" else lc.relayout_problem(dp, "zeros", SEED)
        assert label == "canonical" or q.levels[0].P.nnz > dp.levels[0].P.nnz
        ds = capi.DarcySolver(gpu_ctx, q)
        f = capi.LevelFields(gpu_ctx, ds, 0, True)
        assert np.array_equal(f.parents(), want), label
        f.close()
        ds.close()


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_library_elimination_of_a_relaid_element_input(cases, hex_hierarchy_small, layout):
    """pmc_hybrid_build (host code of the library) on the re-laid element input: H and G equal the canonical ones as
    matrices to 1e-14 of their largest entry"""
    from parelagmc_amd import capi
    h = hex_hierarchy_small
    el = lc.hybrid_elements(h.spaces[0], cases["hex"]["sampler"].alpha, h.P[0])
    H, G, z = capi.hybrid_build(*el.args())
    H2, G2, z2 = capi.hybrid_build(*lc.relayout_problem(el, layout, SEED).args())
    assert abs(H - H2).max() <= 1e-14 * abs(H).max() and abs(G - G2).max() <= 1e-14 * abs(G).max()
    assert np.max(np.abs(z - z2)) <= 1e-14 * np.max(np.abs(z))

"""The MINRES preconditioners away from the defaults of pmc_solver_opts: smoother degrees 1, 3, 4, other smoothing and
coarse intervals, another M-block polynomial, another schur_scale - B^-1 r itself against the fp64 restatements of
oracle/precond_oracle.py, which follow all of these options.  Run with -m gpu on an MI355X.

Every other comparison of a preconditioner application with the oracles creates its handles with the default options (a few
cheb_degree_M = 3 / 4 cases and the hybridized Darcy handles at mg_smooth_degree = 3 aside), and the one test that sets other
degrees compares converged fields - which any fixed SPD preconditioner reaches.  The options do not only change numbers, they
change which code runs (csrc/vcycle_plan.hpp, csrc/solver.hip, csrc/k_tail.hip, csrc/sampler.hip):
- level_step takes the fp32 paths only at smooth_degree == 2: any other degree sends shared-value sampler levels and the
  per-realization Darcy levels outside the LDS tail through cycle_generic / cycle_bottom in BOTH storages;
- cheb_apply's unfused loop (cheb_first, cheb_step with the rho / rho_old recurrence, cheb_step_z for the typed last step, the
  convert_z rounding pass at degree 1), pick_buffers' parity (2 degree - 1 flips on a smoothed level, degree - 1 on a bottom),
  and cycle_generic's unfused branch after the coarse solve (spmm(P, xc, x, accumulate), then cheb_apply from a non-zero guess),
  which is dead on has_sp sampler levels at degree 2;
- the hybridized sampler on the generic path: a level renumbered by agg_pack_rows restricted through Pt;
- inside the LDS tail: tail_cheb's general loop as a pre-smoother, its one-pass branch as a bottom of last_degree 2,
  tail_cheb_cached at a degree other than 12;
- schur_scale, mg_smooth_ratio, mg_coarse_degree / mg_coarse_ratio and cheb_ratio_M, which never left their defaults on the
  device.

The option sets (precond_cases.OPTION_SETS): deg1 (every polynomial of one step), deg3 (odd parity, bottom of degree 2, M-block
of degree 3 on [1/6, 1]), deg4 (even parity, bottom of degree 5, schur_scale 0.7), ratio (degree 2 kept: the fused kernels with
other coefficients, schur_scale 1.3).  The Darcy handles ignore schur_scale and run deg1, deg3, deg4.

The handles.  Sampler (MC level 0, n_mc_levels = 1): tet-saddle (whole cycle in the tail), hex12-hybrid (wide launches in the
tail, narrow ones level 0 on kernels - a p_agg level - and dense_apply on level 1), hex20-saddle and hex20-sa (hex 5^3 refined
twice: 8 000 / 1 000 / 125 Schur rows, three vectors each exceed the tail's LDS, so level 0 runs on kernels), hex24-hybrid
(level 0 on kernels at every width) and hex8-long.  The last one is there because on every other saddle-point handle the cycle
ends on a reaction-dominated level (MgLevel::is_last) with the polynomial of that level's own Gershgorin interval, so
mg_coarse_degree / mg_coarse_ratio would not be exercised by any sampler: hex8-long (512 / 64 rows, corlen 2) ends on its last
level with the polynomial of the options.  Which of the two a polynomial bottom must carry is decided here from the level
operator (the closed form of sampler.hip: interval [lo, lmax] of the Gershgorin discs of D^-1 S, reaction-dominated when
lmax / lo <= 3.5, or <= 40 on at most 4 096 rows) and asserted either way.
hex20-reaction (20^3 at corlen 0.03) is the opposite case: level 0 itself is reaction-dominated and too large for the tail, so
the cycle is one polynomial of degree 3 (schur_scale 0.7) or 4 (1.3) through cycle_bottom on kernels; only schur_scale and
the M-block options reach it, so it runs deg4 and ratio.
Darcy (saddle-point): hex (16^3 / 8^3 / 4^3 of the preconditioner tests, in the per-realization tail), hex24 (24^3 = 13 824 rows,
above the tail's 8 192), hex-sa (mg_coarsening = 1, the chain oracle) and flat24 (the 24^3 cells as ONE level: the polynomial of
mg_coarse_degree / mg_coarse_ratio alone through cycle_bottom on kernels - no other handle of the suite ends a cycle outside
the tail).

Asserted per (handle, set, storage): a. B^-1 r of columns 0, nb - 1 and 32 (Darcy: 0, nb - 1, 4 - the 1e3-contrast field) at
widths 1, 8, 16, 32 and BatchWidth (Darcy: 1, 8, BatchWidth) against the reference of the launch's regime within REF_TOL; b. the
sensitivity of that comparison, on the reference alone: a second reference with the degrees and ratios put back to the defaults
(schur_scale 1) differs from it by at least 100 REF_TOL["fp32"] of the column's norm on every compared column, and in every
block of the column whose options changed on at least one compared column of every launch - so that a device that ignored an
option, of one block alone too, would fail a; c. the exported setup values against the options (and
lmax, last_degree, last_ratio against their closed forms); d. the path preconditions from the exports, and that the
parametrization reaches every path named above at a degree other than 2; e. every compared column against the same column in
the narrowest launch of its regime within WIDTH_TOL.

Measured on the MI355X (the printed lines).  Every case passed on the library as it was: the device follows every option, and
this file found no defect.
- against the fp64 reference, fp64 storage, largest over the sets: tet-saddle 1.1e-15, hex12-hybrid 2.9e-15, hex20-saddle
  5.4e-16, hex20-sa 1.1e-15, hex24-hybrid 9.8e-15, hex8-long 4.0e-16, hex20-reaction 3.2e-16; Darcy hex 4.9e-16, hex24 1.1e-15,
  hex-sa 3.0e-14, flat24 4.0e-16;
- fp32 storage: the same figures to both digits wherever the degree is not 2 on shared-value levels - off the fp32 paths
  nothing of a sampler cycle is kept in fp32 - and under `ratio`, which keeps the fused fp32 kernels, hex12-hybrid 1.9e-8
  (narrow), hex20-saddle 2.0e-8, hex24-hybrid 2.2e-8 narrow / 1.7e-8 wide; Darcy (fp32 VALUES of the per-realization levels
  outside the tail and of the materialised M-block): hex 1.4e-9 (deg3), hex24 3.7e-8 / 6.0e-8 / 7.0e-8 (deg1 / deg3 / deg4),
  hex-sa 7.7e-9 (deg3), flat24 9.8e-9 / 5.4e-8 (deg3 / deg4);
- smallest distance between the reference and the default-option reference: whole column 4.4e-2 (tet-saddle deg3), Darcy
  6.2e-2 (hex24 deg4); weakest changed block on the best column of a launch 1.9e-2 (hex20-saddle deg4, the u-block), Darcy
  1.1e-2 (hex24 deg4) - against the required 1e-3;
- width consistency: at most 1.7e-16 (bit for bit at degrees 1 and 2);
- durations: every test below 0.3 s (the first one 0.7 s with the module's set-up), the file 8 s, the four new trajectory
  tests of test_gpu_minres_trajectory.py 0.2 to 0.9 s each.  Reference iteration counts of the new trajectory cases: hex8-mini-deg3
  35 36 31 22 7 0 36 0 (36), hex16-saddle-deg3 32 32 27 17 7 0 31 0 (32), no borderline column; the device stops where the
  reference does, iterates within 2.1e-14 | 2.0e-12 (mini, both storages) and 4.2e-9 | 2.7e-7 (hex16, fp32 storage).

Mutation check.  Each change was built once into a scratch copy of the library (none is committed) and run against this file,
the new trajectory cases and the pre-existing reference comparisons (test_gpu_sampler_precond.py, test_gpu_precond.py,
test_gpu_darcy_internal_precond.py, test_fp32_krylov_vectors_on_every_preconditioner_path of test_gpu_round3.py):
- `rho_old = rho` dropped from cheb_apply's loop: test a fails on every deg3 and deg4 case that runs a polynomial on kernels or
  a materialised M-block (24 sampler and 16 Darcy cases, hex20-reaction included) and the four hex16-saddle-deg3 trajectory
  tests.  Pre-existing: 6 Darcy cases fail (tet-noeg, hex-hybrid-d3, hex32-hybrid-d3), no sampler test;
- the same line dropped from tail_cheb: every deg3 / deg4 case with a level in the tail (18 sampler, 12 Darcy) and all eight
  new trajectory tests.  Pre-existing: hex32-sa of the sampler and 17 cases of test_gpu_darcy_internal_precond.py fail (a
  bottom of degree 12 that does not fit tail_cheb_cached), none on the caller's hierarchies;
- 1 / theta -> 1 / lmax in cheb_first: every deg1, deg3, deg4 case (32 sampler - hex20-reaction under `ratio` too, its bottom
  has degree 4 - and all 24 Darcy cases) and the four hex16-saddle-deg3 trajectory tests.  Pre-existing: the same 6 Darcy
  cases, no sampler test;
- smooth_ratio where last_ratio / coarse_ratio belongs in cycle_bottom: hex20-reaction (4 cases) and flat24 (6 cases) of test a.
  Pre-existing: none fails - no other handle ends its cycle outside the tail;
- the division by schur_scale removed in sampler.hip: the 16 deg4 / ratio cases of the saddle-point sampler handles in test a
  and in test c (lmax of the level operator), and test d (the roles of hex20-saddle change).  Pre-existing: none can fail (every
  other handle divides by 1);
- the fused dot of the convert_z fallback taken from the unrounded vector: not built.  It changes <r, z> by at most 6e-8
  relative, only where z is stored in fp32 and a polynomial has degree 1, and only a solve reads that dot; initial_norm is held
  to 0.5 REF_TOL |b| |z| / <b, z> (about 5e-6) by the trajectory tests, so no test of the project's tolerances can see it, new
  or pre-existing.  B^-1 r through pmc_sampler_apply_preconditioner does not return the dot.
"""
import zlib

import numpy as np
import pytest

from precond_cases import (OPTION_SETS, REF_TOL, Handle, darcy_fields, darcy_flat24_problem, darcy_hex24_problem,
                           darcy_hex_problem, darcy_options, rel as _rel)

pytestmark = pytest.mark.gpu

WIDTH_TOL = {"fp64": 1e-12, "fp32": 1e-5}         # as test_gpu_sampler_precond.py
STORAGES = ("fp64", "fp32")
SENSITIVITY = 100.0 * REF_TOL["fp32"]
ALL_SETS = tuple(OPTION_SETS)

SAMPLER_CASES = ([("tet-saddle", s) for s in ALL_SETS] + [("hex12-hybrid", s) for s in ALL_SETS] +
                 [("hex20-saddle", s) for s in ALL_SETS] + [("hex20-sa", "deg3"), ("hex24-hybrid", "deg3"),
                                                            ("hex24-hybrid", "ratio")] +
                 [("hex8-long", s) for s in ALL_SETS] + [("hex20-reaction", "deg4"), ("hex20-reaction", "ratio")])
SAMPLER_IDS = [f"{h}-{s}" for h, s in SAMPLER_CASES]
# handles whose level 0 must run on kernels / whose wide launches must run wholly inside the tail
ON_KERNELS = ("hex20-saddle", "hex20-sa", "hex24-hybrid")
IN_TAIL = ("tet-saddle", "hex12-hybrid", "hex8-long")
BOTTOM_ON_KERNELS = ("hex20-reaction",)           # ... whose cycle is one polynomial on level 0, outside the tail

DARCY_SETS = ("deg1", "deg3", "deg4")
DARCY_CASES = [(h, s) for h in ("hex", "hex24", "hex-sa", "flat24") for s in DARCY_SETS]
DARCY_IDS = [f"{h}-{s}" for h, s in DARCY_CASES]
# Multigrid::enable_bv_tail / build_tails, as test_gpu_darcy_internal_precond.py restates them
TAIL_ROWS = 8192
TAIL_LDS_DOUBLES = (160 * 1024 - 1024) // 8
TAIL_THREADS = 1024                                # kTailThreads: tail_cheb_cached holds 3 x 5 or 2 x 7 entries per thread


def _rng(label):
    return np.random.Generator(np.random.PCG64(zlib.crc32(label.encode())))


# ---------------------------------------------------------------------------------------------------------------------------
# sampler handles

_HANDLES = {}
_RHS = {}        # handle name -> right-hand sides (the same for every set and storage)
_REFS = {}       # (name, set) -> (the setup they were built from, {(column, narrow): (reference, default one)}, default oracle)


@pytest.fixture(scope="module")
def handles(gpu_ctx):
    """(name, set, storage) -> Handle, built once per module"""
    def get(name, oset, storage):
        key = (name, oset, storage)
        if key not in _HANDLES:
            _HANDLES[key] = Handle(gpu_ctx, name, storage, **OPTION_SETS[oset])
        return _HANDLES[key]
    yield get
    for hd in _HANDLES.values():
        hd.smp.close()
    _HANDLES.clear()
    _REFS.clear()
    _RHS.clear()


def _rhs(name, hd):
    if name not in _RHS:
        _RHS[name] = _rng(name).standard_normal((hd.top, hd.n))
    return _RHS[name]


def _sampler_widths(top):
    return sorted({w for w in (1, 8, 16, 32, top) if w <= top})


def _cols(nb):
    return sorted({c for c in (0, nb - 1, 32) if c < nb})


def _default_degree_M(ratio_M):
    return 4 if ratio_M > 16.0 else 2


def _default_oracle(hd):
    """the reference of a device that ignored the options: the same exported setup (roles, lmax, prolongators, ratio_M) with
    the smoothing degree and ratio, a bottom polynomial that carries the options, and the M-block degree put back to the
    defaults of pmc_solver_opts, schur_scale 1"""
    from parelagmc_amd import capi
    from oracle.precond_oracle import SamplerPrecondOracle
    d, o = capi.solver_opts(), hd.opts
    setup = []
    for m in hd.setup:
        q = dict(m)
        q["smooth_degree"] = d.mg_smooth_degree
        q["smooth_ratio"] = (2.0 if hd.hybrid else 1.0) * d.mg_smooth_ratio
        if (q["last_degree"], q["last_ratio"]) == (o.mg_coarse_degree, o.mg_coarse_ratio):
            q["last_degree"], q["last_ratio"] = d.mg_coarse_degree, d.mg_coarse_ratio
        if not hd.hybrid:
            q["degree_M"] = _default_degree_M(q["ratio_M"])
        setup.append(q)
    return SamplerPrecondOracle(hd.prob, 0, setup, hd.P, 1.0)


def _changed_blocks(hd):
    """the row ranges of a column whose reference the options of the handle change: the u-block when the M-block polynomial
    has another degree than the default rule gives at the exported ratio_M; the Schur block (or the multiplier system) when
    the cycle smooths a level - every set changes the smoothing -, ends with the polynomial of the options, or runs on another
    schur_scale (hex20-reaction: nothing else reaches its one polynomial)"""
    from oracle.precond_oracle import ROLE_DESCEND
    if hd.hybrid:
        return {"lambda": slice(0, hd.n)}
    n_u = hd.prob.levels[0].n_u
    out = {}
    o = hd.opts
    if (int(hd.setup[0]["role_wide"]) == ROLE_DESCEND or o.schur_scale != 1.0 or
            (hd.setup[0]["last_degree"], hd.setup[0]["last_ratio"]) == (o.mg_coarse_degree, o.mg_coarse_ratio)):
        out["s"] = slice(n_u, hd.n)
    m = hd.setup[0]
    if int(m["degree_M"]) != _default_degree_M(m["ratio_M"]):
        out["u"] = slice(0, n_u)
    return out


def _references(hd, name, oset, r, j, narrow):
    """(reference, default-option reference) of column j in the regime, one oracle call each, shared by the storages"""
    if (name, oset) not in _REFS or _REFS[(name, oset)][0] != hd.setup:
        _REFS[(name, oset)] = (hd.setup, {}, _default_oracle(hd))
    _, refs, dflt = _REFS[(name, oset)]
    if (j, narrow) not in refs:
        refs[(j, narrow)] = (hd.oracle.apply(r[j], narrow), dflt.apply(r[j], narrow))
    return refs[(j, narrow)]


def _sensitivity(ref, dflt, blocks):
    """distance between the two references relative to the column: of the whole column, and the smallest over the blocks
    whose options changed.  The first is asserted on every compared column.  The second on the best column of every launch:
    a device that ignored the options of ONE block fails there (in the 1e3-contrast column of the Darcy batches the u-block
    carries the norm, and the p-block's share of it is 7e-4 to 4e-3)"""
    n = np.linalg.norm(ref)
    return np.linalg.norm(ref - dflt) / n, min(np.linalg.norm(ref[b] - dflt[b]) for b in blocks) / n


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name,oset", SAMPLER_CASES, ids=SAMPLER_IDS)
def test_sampler_preconditioner_under_options_matches_fp64_reference(handles, name, oset, storage):
    hd = handles(name, oset, storage)
    r = _rhs(name, hd)
    blocks = list(_changed_blocks(hd).values())
    worst, sens, sens_block = {False: 0.0, True: 0.0}, np.inf, np.inf
    for nb in _sampler_widths(hd.top):
        z = hd.smp.ApplyPreconditioner(0, r[:nb])
        narrow = hd.narrow(nb)
        best = 0.0
        for j in _cols(nb):
            ref, dflt = _references(hd, name, oset, r, j, narrow)
            s, sb = _sensitivity(ref, dflt, blocks)
            sens, best = min(sens, s), max(best, sb)
            assert s >= SENSITIVITY, (nb, j, s, "the default-option reference is too close: strengthen the set")
            e = _rel(z[j], ref)
            worst[narrow] = max(worst[narrow], e)
            print(f"  {name} {oset} {storage} width {nb} column {j}: rel L2 {e:.2e}, to the default reference {s:.2e} "
                  f"(weakest block {sb:.2e})")
            assert e <= REF_TOL[storage], (nb, j, e)
        sens_block = min(sens_block, best)
        assert best >= SENSITIVITY, (nb, best, "no compared column of the launch separates every block: strengthen the set")
    print(f"options {name} {oset} {storage} widths {_sampler_widths(hd.top)}: max rel L2 "
          + (f"narrow {worst[True]:.2e}, " if hd.dense_nb > 0 else "") + f"wide {worst[False]:.2e}; "
          f"smallest distance to the default reference {sens:.2e}, per block {sens_block:.2e}")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name,oset", SAMPLER_CASES, ids=SAMPLER_IDS)
def test_sampler_preconditioner_under_options_is_the_same_at_every_width(handles, name, oset, storage):
    """every compared column equals the same column in the narrowest launch of its regime: alone, or - the wide launches of a
    hybridized handle - in its own group of 2 dense_nb columns"""
    hd = handles(name, oset, storage)
    r = _rhs(name, hd)
    w0 = 2 * hd.dense_nb
    base, worst = {}, 0.0
    for nb in _sampler_widths(hd.top):
        z = hd.smp.ApplyPreconditioner(0, r[:nb])
        narrow = hd.narrow(nb)
        for j in _cols(nb):
            if (j, narrow) not in base:
                if narrow or hd.dense_nb == 0:
                    base[(j, narrow)] = hd.smp.ApplyPreconditioner(0, r[j:j + 1])[0]
                else:
                    c = j - j % w0
                    base[(j, narrow)] = hd.smp.ApplyPreconditioner(0, r[c:c + w0])[j - c]
            b = base[(j, narrow)]
            assert np.all(np.isfinite(b)) and np.linalg.norm(b) > 0
            e = _rel(z[j], b)
            worst = max(worst, e)
            assert e <= WIDTH_TOL[storage], (nb, j, e)
    print(f"options width-consistency {name} {oset} {storage}: max rel L2 = {worst:.2e}")


def _gershgorin(S):
    """(lmax, lo) of sampler.hip / build_chain: 1.0001 max_i and min_i of the Gershgorin interval of row i of D^-1 S"""
    S = S.tocsr()
    s = np.asarray(abs(S).sum(axis=1)).ravel() / S.diagonal()
    return 1.0001 * float(s.max()), float((2.0 - s).min())


def _reaction_bottom(S):
    """None, or the (last_degree, last_ratio) of a reaction-dominated level (MgLevel::is_last): the polynomial on the level's
    own Gershgorin interval that reduces the error by 0.02"""
    lmax, lo = _gershgorin(S)
    if not (lo > 0.0 and (lmax / lo <= 3.5 or (S.shape[0] <= 4096 and lmax / lo <= 40.0))):
        return None
    ratio = lmax / (lo * 0.999)
    sk = np.sqrt(ratio)
    return min(16, max(2, int(np.ceil(np.log(2.0 / 0.02) / np.log((sk + 1.0) / (sk - 1.0)))))), ratio


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name,oset", SAMPLER_CASES, ids=SAMPLER_IDS)
def test_sampler_setup_values_follow_the_options(handles, name, oset, storage):
    """the exported setup against the options; lmax and a reaction-dominated bottom against their closed forms on the level
    operator (which carries schur_scale); the path preconditions of the handle"""
    from oracle.precond_oracle import ROLE_DESCEND, ROLE_EXACT, ROLE_POLY, ROLE_UNREACHED
    hd = handles(name, oset, storage)
    o, want = hd.opts, OPTION_SETS[oset]
    for key, val in want.items():
        assert getattr(o, key) == val
    bottoms = []
    for v, m in enumerate(hd.setup):
        assert m["smooth_degree"] == o.mg_smooth_degree
        assert m["smooth_ratio"] == (2.0 if hd.hybrid else 1.0) * o.mg_smooth_ratio
        if hd.hybrid:
            assert m["degree_M"] == 0 and m["ratio_M"] == 0
        else:
            assert m["ratio_M"] > 1.0
            assert m["degree_M"] == (o.cheb_degree_M or _default_degree_M(m["ratio_M"]))
            if "cheb_ratio_M" in want:
                assert m["ratio_M"] == want["cheb_ratio_M"]
        roles = (int(m["role_wide"]), int(m["role_narrow"]))
        if roles == (ROLE_UNREACHED, ROLE_UNREACHED):
            continue
        S = hd.oracle.S[v]
        assert S.shape[0] == m["rows"]
        assert abs(m["lmax"] - _gershgorin(S)[0]) <= 1e-10 * m["lmax"], (v, m["lmax"], _gershgorin(S)[0])
        if ROLE_POLY in roles:
            rb = _reaction_bottom(S)
            if rb is None:
                assert v == len(hd.setup) - 1
                assert (m["last_degree"], m["last_ratio"]) == (o.mg_coarse_degree, o.mg_coarse_ratio), (v, m)
                bottoms.append("options")
            else:
                assert m["last_degree"] == rb[0] and abs(m["last_ratio"] - rb[1]) <= 1e-10 * rb[1], (v, m, rb)
                bottoms.append("reaction")
    m0 = hd.setup[0]
    if name in BOTTOM_ON_KERNELS:
        assert int(m0["role_wide"]) == ROLE_POLY and not m0["tail_wide"] and bottoms == ["reaction"]
        assert int(m0["last_degree"]) > 2, "a bottom of degree 2 takes the fused polynomial, not cheb_apply's loop"
    else:
        assert int(m0["role_wide"]) == ROLE_DESCEND
    if name in ON_KERNELS:
        assert not m0["tail_wide"], "level 0 of a wide launch must run on kernels"
    if name in IN_TAIL:
        assert m0["tail_wide"], "the whole cycle of a wide launch must run inside the tail"
    if name == "hex12-hybrid":
        assert not m0["tail_narrow"] and int(m0["role_narrow"]) == ROLE_DESCEND
        assert int(hd.setup[1]["role_narrow"]) == ROLE_EXACT
    if name == "hex8-long":
        assert bottoms == ["options"], "the cycle must end with the polynomial of mg_coarse_degree / mg_coarse_ratio"
    print(f"options setup {name} {oset} {storage}: rows {[int(m['rows']) for m in hd.setup]} roles wide "
          f"{[int(m['role_wide']) for m in hd.setup]} narrow {[int(m['role_narrow']) for m in hd.setup]} tail wide "
          f"{[int(m['tail_wide']) for m in hd.setup]} narrow {[int(m['tail_narrow']) for m in hd.setup]} last "
          f"{[(int(m['last_degree']), round(m['last_ratio'], 2)) for m in hd.setup]} bottoms {bottoms} degree_M "
          f"{int(m0['degree_M'])} ratio_M {m0['ratio_M']:.3f}")


def _fits_cached(S):
    """tail_cheb_cached's own condition: 3 rows of at most 5 entries, or 2 rows of at most 7, per thread"""
    S = S.tocsr()
    width = int(np.diff(S.indptr).max())
    return (S.shape[0] <= 3 * TAIL_THREADS and width <= 5) or (S.shape[0] <= 2 * TAIL_THREADS and width <= 7)


# ---------------------------------------------------------------------------------------------------------------------------
# Darcy handles (saddle-point)

_DARCY = {}
_DARCY_DATA = {}     # handle name -> (k, r)
_DARCY_REFS = {}     # (name, set or None, column, ratio_M, degree_M) -> reference


class _DarcyHandle:
    def __init__(self, ctx, hex_hierarchy, name, oset, storage):
        from parelagmc_amd import capi
        self.name, self.oset = name, oset
        self.dp = (darcy_hex24_problem() if name == "hex24" else darcy_flat24_problem() if name == "flat24" else
                   darcy_hex_problem(hex_hierarchy))
        st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
        extra = dict(mg_coarsening=1) if name == "hex-sa" else {}
        self.opts = capi.solver_opts(precond_storage=st, **extra, **darcy_options(oset))
        self.ds = capi.DarcySolver(ctx, self.dp, self.opts)
        self.setup = self.ds.vcycle_levels(0)
        self.P = [self.ds.vcycle_prolongator(0, v) for v in range(len(self.setup) - 1)] if name == "hex-sa" else None
        L = self.dp.levels[0]
        self.n, self.n_p, self.n_u = L.n_u + L.n_p, L.n_p, L.n_u
        self.top = self.ds.BatchWidth(0)

    def reference(self, k, r, default):
        """B(k)^-1 r under the handle's options, or (default) under the defaults of pmc_solver_opts with everything else of
        the exported setup kept"""
        from parelagmc_amd import capi
        from oracle.precond_oracle import DarcyChainPrecondOracle, DarcyPrecondOracle
        o = capi.solver_opts() if default else self.opts
        m0 = self.setup[0]
        deg_M = 2 if default else int(m0["degree_M"])
        if self.P is None:
            po = DarcyPrecondOracle(self.dp, o.mg_smooth_degree, o.mg_smooth_ratio, o.mg_coarse_degree, o.mg_coarse_ratio)
            return po.apply(0, k, r, m0["ratio_M"], deg_M)
        setup = [dict(m) for m in self.setup]
        if default:
            for m in setup:
                m.update(smooth_degree=o.mg_smooth_degree, smooth_ratio=o.mg_smooth_ratio, degree_M=deg_M)
            setup[-1].update(last_degree=o.mg_coarse_degree, last_ratio=o.mg_coarse_ratio)
        return DarcyChainPrecondOracle(self.dp, 0, setup, self.P).apply(k, r)


@pytest.fixture(scope="module")
def darcy(gpu_ctx, hex_hierarchy):
    def get(name, oset, storage):
        key = (name, oset, storage)
        if key not in _DARCY:
            _DARCY[key] = _DarcyHandle(gpu_ctx, hex_hierarchy, name, oset, storage)
        return _DARCY[key]
    yield get
    for hd in _DARCY.values():
        hd.ds.close()
    _DARCY.clear()
    _DARCY_DATA.clear()
    _DARCY_REFS.clear()


def _darcy_data(hd):
    if hd.name not in _DARCY_DATA:
        rng = _rng("darcy/" + hd.name)
        _DARCY_DATA[hd.name] = (darcy_fields(rng, hd.top, hd.n_p), rng.standard_normal((hd.top, hd.n)))
    return _DARCY_DATA[hd.name]


def _darcy_reference(hd, k, r, j, default):
    m0 = hd.setup[0]
    key = (hd.name, None if default else hd.oset, j, m0["ratio_M"], int(m0["degree_M"]) if not default else 2)
    if key not in _DARCY_REFS:
        _DARCY_REFS[key] = hd.reference(k[j], r[j], default)
    return _DARCY_REFS[key]


def _tail_start(rows):
    """the first level of the LDS tail of a per-realization hierarchy (Multigrid::enable_bv_tail / build_tails)"""
    for l0 in range(len(rows)):
        rest = rows[l0:]
        if max(rest) <= TAIL_ROWS and len(rest) <= 8 and 3 * sum(rest) <= TAIL_LDS_DOUBLES:
            return l0
    return len(rows)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name,oset", DARCY_CASES, ids=DARCY_IDS)
def test_darcy_preconditioner_under_options_matches_fp64_reference(darcy, name, oset, storage):
    """B(k_j)^-1 r_j, every compared column with its own k, on MC level 0; the setup values against the options; where level 0
    runs (the tail's own size rule, restated); the sensitivity of the comparison in the u- and in the p-block"""
    from oracle.precond_oracle import KIND_CALLER, KIND_SA
    hd = darcy(name, oset, storage)
    o, want = hd.opts, darcy_options(oset)
    for v, m in enumerate(hd.setup):
        assert int(m["hierarchy"]) == (KIND_SA if name == "hex-sa" else KIND_CALLER)
        assert (m["smooth_degree"], m["smooth_ratio"]) == (o.mg_smooth_degree, o.mg_smooth_ratio)
        assert m["bottom"] == (1.0 if v == len(hd.setup) - 1 else 0.0)
        if m["bottom"]:
            assert (m["last_degree"], m["last_ratio"]) == (o.mg_coarse_degree, o.mg_coarse_ratio)
    m0 = hd.setup[0]
    assert int(m0["degree_M"]) == want["cheb_degree_M"] and m0["ratio_M"] > 1.0
    if "cheb_ratio_M" in want:
        assert m0["ratio_M"] == want["cheb_ratio_M"]
    rows = [int(m["rows"]) for m in hd.setup]
    assert rows[0] == hd.n_p
    if name == "hex24":
        assert rows[0] > TAIL_ROWS and _tail_start(rows) == 1, rows
    elif name == "flat24":
        assert rows == [13824] and rows[0] > TAIL_ROWS, rows
    else:
        assert _tail_start(rows) == 0, rows
    k, r = _darcy_data(hd)
    blocks = [slice(0, hd.n_u), slice(hd.n_u, hd.n)]      # every set changes the M-block's degree and the cycle
    worst, sens, sens_block = 0.0, np.inf, np.inf
    for nb in sorted({1, 8, hd.top}):
        z = hd.ds.ApplyPreconditioner(0, k[:nb], r[:nb])
        best = 0.0
        for j in sorted({c for c in (0, nb - 1, 4) if c < nb}):
            ref = _darcy_reference(hd, k, r, j, False)
            dflt = _darcy_reference(hd, k, r, j, True)
            s, sb = _sensitivity(ref, dflt, blocks)
            sens, best = min(sens, s), max(best, sb)
            assert s >= SENSITIVITY, (nb, j, s, "the default-option reference is too close: strengthen the set")
            e = _rel(z[j], ref)
            worst = max(worst, e)
            print(f"  darcy {name} {oset} {storage} width {nb} column {j}: rel L2 {e:.2e}, to the default reference {s:.2e} "
                  f"(weakest block {sb:.2e})")
            assert e <= REF_TOL[storage], (nb, j, e)
        sens_block = min(sens_block, best)
        assert best >= SENSITIVITY, (nb, best, "no compared column of the launch separates every block: strengthen the set")
    print(f"options darcy {name} {oset} {storage} rows {rows} widths {sorted({1, 8, hd.top})}: max rel L2 = {worst:.2e}; "
          f"smallest distance to the default reference {sens:.2e}, per block {sens_block:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------

def test_option_sets_reach_every_path_at_another_degree(handles, darcy):
    """from the exports of the handles above.  At a degree other than 2 the storage does not choose the path, but the
    hybridized handles pack level 0 (agg_pack_rows) in fp32 storage only; the per-realization roles and the tail do not depend
    on it (Darcy: fp64 handles)"""
    from oracle.precond_oracle import KIND_HYBRID, ROLE_DESCEND, ROLE_POLY
    seen = set()
    for name, oset, storage in [(n, s, st) for n, s in SAMPLER_CASES for st in STORAGES]:
        hd = handles(name, oset, storage)
        deg = hd.opts.mg_smooth_degree
        for v, (m, f) in enumerate(zip(hd.setup, hd.info)):
            for regime in ("wide", "narrow"):
                role, tail = int(m["role_" + regime]), bool(m["tail_" + regime])
                if role == ROLE_DESCEND and not tail and deg != 2:
                    seen.add("generic on kernels")
                    if int(m["hierarchy"]) == KIND_HYBRID and v == 0 and f["fused_restriction"]:
                        seen.add("generic on an aggregate level")
                    if deg == 1 and v == 0:
                        seen.add("degree-1 rounding pass")
                if role == ROLE_DESCEND and tail and deg != 2:
                    seen.add("tail general loop")
                if role == ROLE_POLY and not tail and int(m["last_degree"]) > 2:
                    seen.add(f"polynomial bottom on kernels, {'odd' if (int(m['last_degree']) - 1) % 2 else 'even'} flips")
                if role == ROLE_POLY and tail and deg != 2 and int(m["last_degree"]) == 2:
                    seen.add("tail fused bottom")
                if role == ROLE_POLY and tail and deg != 2 and int(m["last_degree"]) == 5 and _fits_cached(hd.oracle.S[v]):
                    seen.add("tail cached bottom at degree 5")
        if not hd.hybrid and int(hd.setup[0]["degree_M"]) == 1:
            seen.add("degree-1 rounding pass of the M-block")
    for name, oset in DARCY_CASES:
        hd = darcy(name, oset, "fp64")
        rows = [int(m["rows"]) for m in hd.setup]
        t0 = _tail_start(rows)
        if len(rows) == 1 and t0 == 1:
            seen.add(f"per-realization bottom of degree {int(hd.setup[0]['last_degree'])} on kernels")
        elif t0 > 0:
            seen.add("per-realization generic on kernels")
        if t0 < len(rows) - 1:
            seen.add("per-realization tail general loop")
        last = hd.setup[-1]
        # the caller's octree hierarchy: 7-point rows on the last level (tail_cheb_cached<2, 7>)
        if name != "hex-sa" and t0 < len(rows) and int(last["last_degree"]) == 2:
            seen.add("per-realization tail fused bottom")
        if name != "hex-sa" and t0 < len(rows) and int(last["last_degree"]) == 5 and rows[-1] <= 2 * TAIL_THREADS:
            seen.add("per-realization tail cached bottom at degree 5")
    want = {"generic on kernels", "generic on an aggregate level", "tail general loop", "tail fused bottom",
            "tail cached bottom at degree 5", "degree-1 rounding pass", "degree-1 rounding pass of the M-block",
            "per-realization generic on kernels", "per-realization tail general loop", "per-realization tail fused bottom",
            "per-realization tail cached bottom at degree 5", "polynomial bottom on kernels, odd flips",
            "polynomial bottom on kernels, even flips", "per-realization bottom of degree 1 on kernels",
            "per-realization bottom of degree 2 on kernels", "per-realization bottom of degree 5 on kernels"}
    assert want <= seen, f"paths no option set reaches: {sorted(want - seen)}"

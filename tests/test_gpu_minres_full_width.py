"""The MINRES loops at the width the managers and the benchmark run them at - pmc_sampler_batch_width, 64 to 256 columns in
column groups of 32 - iteration by iteration against the single-vector fp64 reference, with the machinery, the tolerance scheme
and the constants of test_gpu_minres_trajectory.py (which stops at 32 columns; read its docstring first).  Run with -m gpu on
an MI355X.

Why: many launchers switch to another form of their kernel on the size of the operands alone (csrc/klaunch.hpp: nt_flat,
nt_poly, nt_streams, grid_bounded; more than one column group: blockIdx.y).  The suite below this file compares those kernels
with fp64 references at shapes under the gates; a wrong instantiation in an `if (nt)` ladder or a fault in the group
arithmetic would show only as slow convergence.  Every case therefore reads the counters of the gated forms
(pmc_solve_path_count, PMC_COUNT_NT_OPERATOR ... PMC_COUNT_TRACER_SPLIT) around its solve: the ones it names in `needs` must
move at full width and must not move in the narrow twin - the same handle, the first `twin` columns of the same batch - so
that a retuned threshold fails the case instead of quietly returning it to the small form.

Cases (width = pmc_sampler_batch_width of level 0, asserted):
  hex16-saddle / -late / -graph   256   the options of the three hex16 cases of the trajectory file (the eager one with
                                        two_streams = 2: at 4.4 M rows x realizations the automatic choice depends on what
                                        else lives on the device); non-temporal lincomb3 / minres_wx / minres_wx_deferred
                                        (NT_FLAT), 8 column groups
  hex8-mini, tet-mini             256   256 workgroups of the mini kernel; no gated form runs, at either width
  hex12-hybrid                    256   whole cycle in the tail, 8 groups; NT_FLAT
  hex24-hybrid                     64   fused Lanczos forms with two column groups; NT_FLAT (narrow twin: 8 columns)
  hex32-saddle                     64   134 144 rows, default cheb_degree_M: the M block's one-pass polynomial in its
                                        non-temporal form (NT_POLY; narrow twin: 8 columns); fp32 input in fp32 storage
  hex32-cheb4                      64   ... with cheb_degree_M = 4 (cheb_first + cheb_step instead of the polynomial)
  darcy-hex                       256   every column its own field (darcy_fields cycles over six kinds), the full solution
                                        and the Q-only solve; NT_FLAT

The gates are evaluated per column group: PMC_DISPATCH_NB hands the launchers NB = 32 for every width from 32 on, and
nt_poly / nt_streams / the k_darcy.hip callers of nt_flat compute their byte counts with NB.  With 32 columns per group the
operator stream of hex32-saddle is 78 MB (in-loop gate 128 MiB), the multiplier level of hex24-hybrid 25 MB (gate 32 MiB) and
the Darcy M block 13 056 x 32 x 2 = 835 584 entries (gate 1 048 576): none of the three is crossed at any width, so NT_OPERATOR
is asserted to stay put everywhere in this file.  cheb_first carries a fused dot - and with it a bounded grid - only at
polynomial degree 1 without a typed result, which no registered option set selects: BOUNDED_GRID stays put too.

Compared columns: the eight scales of SCALES at 0, 1, 31, 32, width - 33, width - 32, width - 2, width - 1 (both ends of the
launch, both sides of the first and of the last group boundary; 64 columns have one boundary: 30, 31 | 32, 33, then 63 and
62), the ninth column (scale 1e-3) inside a middle group, the bitwise copy of column 0 in another group than column 0.  The
hex32 cases compare six of them - 0, 31, 32, 63, the abs_tol column 33 and the zero column 62 - for the time of the
reference.  Darcy: columns 0, 1, 31, 32, 254, 255.

Runs, as in the trajectory file: mixed batch, capped solves (1, 2, 9), warm starts (hex16-saddle, hex8-mini, hex12-hybrid),
the blind second solve (hex16-saddle in both storages, hex24-hybrid fp32).  Tolerances: REF_TOL, PERTURBATION by storage,
MARGIN 10 over four perturbed reruns, FLOOR 1e-13 - nothing new is chosen; the Darcy case uses the tolerances of the Darcy
case of the trajectory file.  _check_reference_spread is asserted on the reference alone, exactly as there.

Measured on the MI355X (the printed lines; largest over the compared columns, device against reference | tolerance).  Every
compared column of every case stopped at the reference's iteration, and no column of any batch is borderline.  Reference
counts of the mixed batches: hex16 29 29 25 16 7 0 29 0 (29), hex8 19 19 15 10 3 0 19 0 (19), tet 39 39 32 21 7 0 39 0 (39),
hex12-hybrid 12 12 10 6 2 0 12 0 (12), hex24-hybrid 17 17 14 9 3 0 18 0 (18), hex32-saddle 30 25 16 0 30 0, hex32-cheb4
28 24 15 0 28 0; Darcy 30 26 26 53 71 40.
- fp64 storage: iterates at most 1.2e-15 | 3.0e-13 mixed (hex24-hybrid), 5.3e-15 | 6.4e-13 capped, 5.9e-16 | 1.0e-13 warm;
  final_norm at most 3.2e-14 | 4.5e-13; initial_norm at most 1.8e-14 | 1.0e-12 (hex12-hybrid warm; 3.4e-16 elsewhere); Darcy
  2.2e-14 | 1.3e-11 (iterate), 2.8e-14 | 2.5e-10 (final_norm), Q of the compact solve within 3.0e-5 of its bound;
- fp32 storage: iterates at most 1.5e-8 | 3.1e-7 mixed, 2.5e-8 | 5.6e-7 capped (hex24-hybrid at 1), 3.1e-10 | 1.3e-8 warm;
  final_norm at most 4.8e-8 | 4.1e-6; initial_norm at most 9.4e-10 | 1.3e-5; the mini kernel stays at 3.8e-16 ... 9.1e-16 in
  both storages; Darcy 3.5e-10 | 1.4e-5 (iterate), 9.0e-7 | 3.1e-5 (final_norm), Q within 1.1e-3 of its bound;
- the largest share of a tolerance any quantity used: 0.28 (final_norm, hex32-saddle fp32 capped at 1: 5.0e-10 | 1.8e-9);
- blind iterations: unit batch 29 (18) iterations, the mixed batch froze at 7, 16, 25 (3, 9, 14, 17): bit for bit the fresh
  handle's result with 5 polls where the fresh handle makes 16 (10);
- gated launches of one mixed solve, full width / narrow twin: NT_FLAT 31 / 0 (hex16-saddle, -graph), 60 / 0 (hex16-late),
  13 / 0 (hex12-hybrid), 19 / 0 and 1 / 0 (hex24-hybrid fp64 / fp32: the fused Lanczos passes replace lincomb3), 31 / 31
  (hex32), 137 / 0 (Darcy); NT_POLY 31 / 0 (hex32-saddle), 0 / 0 with cheb_degree_M = 4; every other counter 0;
- time: the reference of a batch takes 0.1 ... 1.2 s, 2.7 s on hex32 (six columns); the slowest cases are the hex32 mixed
  batches at 3.2 s each, host time nearly all of it; this file, test_gpu_million_rows.py and test_gpu_tracer_split.py take
  50 s together.

Seeded one at a time in a scratch copy of the library (never committed); "existing" = test_gpu_minres_trajectory.py,
test_gpu_wx_window.py, test_gpu_solve_edges.py, test_gpu_fused_lanczos.py, test_gpu_tracer.py, test_gpu_round4.py and
test_gpu_parity.py, the files nearest to the faults (the whole suite was not rerun per fault):
- lincomb3_kernel<NB, true> reading b where it should read a: 34 tests of this file fail (every case but the mini ones), and
  test_gpu_million_rows.py; 8 existing tests notice it too (hex24-hybrid-32 fp64 of the trajectory file, whose 1.38 M entries
  cross the gate, and the full-size tests of test_gpu_round4.py / test_gpu_parity.py);
- minres_wx_deferred_kernel<NB, true, float> launched with g64 in place of g32: an EQUIVALENT change - g64 is twice g32
  (WxShape<float>::R = 4 rows per thread, <double>::R = 2) and the surplus workgroups return at `i0 >= nflat` - nothing can
  notice it by value and nothing does.  The mix-up the other way round, <NB, true, double> on g32, leaves half the entries
  without their update: 13 fp64 tests of this file and test_gpu_million_rows.py fail (3 existing ones);
- the tail `if (b < nblocks) ...` of compress_partials_kernel dropped: test_gpu_million_rows.py (both capped solves); no
  existing test notices - the two-stage dot otherwise runs at nb = 2 in converged solves;
- in spmm_launch, the non-temporal branch's diagonal-last instantiation swapped with the plain fused-dot one: an EQUIVALENT
  change - the plain form loads dot_with[row], the diagonal-last form takes the same x_i from the row's last gathered column
  and adds the products in the same order; all tests pass, as they must;
- the grid-stride increment of cheb_first_kernel: cheb_first receives a dot buffer only at polynomial degree 1 without a typed
  result, and both callers of cheb_apply_z pass a typed result, so its grid is never bounded in the library as it stands and
  its workgroups never make a second trip: not seeded;
- the output offset dropped from launch_walk's second launch: test_gpu_tracer_split.py."""
import time

import numpy as np
import pytest

from precond_cases import Handle
from test_gpu_minres_trajectory import (EXTRA_SCALE, REL_TOL, SCALES, STORAGES, _Batch, _check_column,
                                        _check_reference_spread, _check_replays, _DarcyBatch, _darcy_solve, _expected_path,
                                        _open, _solve, _Worst)

pytestmark = pytest.mark.gpu

GATES = ("NT_OPERATOR", "NT_POLY", "NT_FLAT", "BOUNDED_GRID", "TWO_STAGE_DOT", "TRACER_SPLIT")
HEX32_ONLY = (0, 2, 3, 5, 6, 7)       # indices into the places: columns 0, 31, 32, 33 (abs_tol), 63, 62 (zero)

# case -> handle, solver options (precond: the ones that change the preconditioner, part of the reference's key), loop, width,
# gated forms that must run at full width, width of the narrow twin, gated forms that may run in the twin too
FULL_CASES = {
    "hex16-saddle": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0, two_streams=2), path="WINDOW", width=256,
                         needs=("NT_FLAT",), twin=32),
    "hex16-late": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0, two_streams=1), path="LATE", width=256,
                       needs=("NT_FLAT",), twin=32),
    "hex16-graph": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0, use_graph=1, check_every=2, two_streams=2),
                        path="GRAPH", width=256, needs=("NT_FLAT",), twin=32),
    "hex8-mini": dict(handle="hex8-saddle", opts={}, path="MINI", width=256, needs=(), twin=32),
    "tet-mini": dict(handle="tet-saddle", opts={}, path="MINI", width=256, needs=(), twin=32),
    "hex12-hybrid": dict(handle="hex12-hybrid", opts={}, path="WINDOW", width=256, needs=("NT_FLAT",), twin=32),
    "hex24-hybrid": dict(handle="hex24-hybrid", opts={}, path="WINDOW", width=64, needs=("NT_FLAT",), twin=8),
    # 134 144 rows x 8 columns are 1 073 152 entries: the flat forms stream non-temporally in the twin as well
    "hex32-saddle": dict(handle="hex32-saddle", opts=dict(two_streams=2), path="WINDOW", width=64, needs=("NT_POLY", "NT_FLAT"),
                         twin=8, twin_may=("NT_FLAT",), only=HEX32_ONLY),
    "hex32-cheb4": dict(handle="hex32-saddle", opts=dict(two_streams=2), precond=dict(cheb_degree_M=4), path="WINDOW", width=64,
                        needs=("NT_FLAT",), twin=8, twin_may=("NT_FLAT",), only=HEX32_ONLY),
}
for _cfg in FULL_CASES.values():
    _cfg["opts"] = {**_cfg["opts"], **_cfg.get("precond", {})}
CASES = list(FULL_CASES)


def _gates(ctx):
    from parelagmc_amd import capi
    return np.array([ctx.lib.pmc_solve_path_count(getattr(capi, "PMC_COUNT_" + g)) for g in GATES], dtype=np.int64)


def _gated(ctx, fn):
    """fn() and the launches of each gated form it issued"""
    before = _gates(ctx)
    out = fn()
    return out, dict(zip(GATES, (int(v) for v in _gates(ctx) - before)))


def _check_gates(case, cfg, wide, narrow):
    """the gated forms the case needs ran at full width - and no other - and did not run in the narrow twin"""
    print(f"gates {case}: width {cfg['width']} {wide}, width {cfg['twin']} {narrow}")
    for g in GATES:
        if g in cfg["needs"]:
            assert wide[g] > 0, (case, g, "the shape no longer reaches its gate", wide)
        else:
            assert wide[g] == 0, (case, g, "a gated form this case does not name ran", wide)
        if g not in cfg.get("twin_may", ()):
            assert narrow[g] == 0, (case, g, "the narrow twin took the gated form", narrow)


def _places(width):
    """(places of the eight scaled columns and the ninth, place of the copy of column 0)"""
    if width == 64:
        pos = [0, 1, 31, 32, 30, 33, 63, 62]
    else:
        pos = [0, 1, 31, 32, width - 33, width - 32, width - 2, width - 1]
    mid = (width // 32 // 2) * 32                      # first column of a middle group (the second of two)
    copy_at = 32 + 5 if width == 64 else mid // 2 + 5  # another group than column 0's and than the ninth column's where there is one
    return pos + [mid + 6], copy_at


class _FullBatch(_Batch):
    """the mixed batch of a full launch; only: the indices into the places that get a reference (None: all nine)"""

    def __init__(self, hd, handle, storage, width, only=None, seed=None):
        pos, copy_at = _places(width)
        assert len(set(pos)) == 9 and copy_at not in pos and copy_at // 32 != 0 and all(0 <= p < width for p in pos)
        super().__init__(hd, handle, storage, width, pos=pos, copy_at=copy_at, seed=seed)
        self.only = tuple(range(9)) if only is None else tuple(only)
        self.seconds = 0.0

    def column(self, p, x0, rel_tol, abs_tol, max_iter, keep):
        if self.pos.index(p) not in self.only:
            return None
        t0 = time.perf_counter()
        col = super().column(p, x0, rel_tol, abs_tol, max_iter, keep)
        self.seconds += time.perf_counter() - t0
        return col


_BASE = {}
_REFS = {}


def _precond_key(case):
    return tuple(sorted(FULL_CASES[case].get("precond", {}).items()))


@pytest.fixture(scope="module")
def base(gpu_ctx):
    """base(case) -> the getter _open expects: the handle with default options (and the case's preconditioner options) the
    reference is built from"""
    def for_case(case):
        pk = _precond_key(case)

        def get(handle, storage):
            key = (handle, storage, pk)
            if key not in _BASE:
                _BASE[key] = Handle(gpu_ctx, handle, storage, **dict(pk))
            return _BASE[key]
        return get
    yield for_case
    for hd in _BASE.values():
        hd.smp.close()
    _BASE.clear()
    _REFS.clear()


def _batch(base, case, storage):
    cfg = FULL_CASES[case]
    key = (cfg["handle"], storage, cfg["width"], _precond_key(case))
    if key not in _REFS:
        hd = base(case)(cfg["handle"], storage)
        assert hd.smp.BatchWidth(0) == cfg["width"], (case, hd.smp.BatchWidth(0))
        assert not hd.narrow(cfg["width"])
        _REFS[key] = _FullBatch(hd, cfg["handle"], storage, cfg["width"], cfg.get("only"))
    return _REFS[key]


def _open_case(ctx, base, case, storage, **opts):
    hd = _open(ctx, base(case), case, storage, cases=FULL_CASES, **opts)
    assert hd.smp.BatchWidth(0) == FULL_CASES[case]["width"], (case, hd.smp.BatchWidth(0))
    return hd


def _scale(bt, i):
    return (SCALES + (EXTRA_SCALE,))[i]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES)
def test_full_width_mixed_batch_stops_column_by_column_where_the_reference_stops(gpu_ctx, base, case, storage):
    cfg = FULL_CASES[case]
    width = cfg["width"]
    bt = _batch(base, case, storage)
    cols = bt.mixed
    sel = [i for i, c in enumerate(cols) if c is not None]
    counts = dict(zip(sel, _check_reference_spread([cols[i] for i in sel], (case, width, storage), 4, True)))
    assert counts[5] == 0 and counts[7] == 0 and min(n for i, n in counts.items() if i not in (5, 7)) > 0, counts
    hd = _open_case(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    try:
        (x, st, took), wide = _gated(gpu_ctx, lambda: _solve(gpu_ctx, hd, bt.rhs))
        events = hd.events
        assert took == _expected_path(case, hd, storage, width, FULL_CASES), took
        longest = max(t[0] for t in st)
        _check_replays(case, events[0], longest + longest % 2, FULL_CASES)
        worst = _Worst()
        zero = np.zeros(hd.n)
        for i in sel:
            p = bt.pos[i]
            _check_column(cols[i], x[p], st[p], zero, worst, f"{case}-{width} {storage} column {p} (scale {_scale(bt, i):g})")
        assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0], "the copy of column 0 differs from it"
        assert all(t[1] == 1 for t in st)              # the unit columns nobody compares still converged
        # the narrow twin: the first columns of the same batch on the same handle
        (_, st_n, took_n), narrow = _gated(gpu_ctx, lambda: _solve(gpu_ctx, hd, bt.rhs[:cfg["twin"]]))
        assert all(t[1] == 1 for t in st_n) and sum(took_n.values()) >= 1
        _check_gates(case, cfg, wide, narrow)
        print(worst.line(f"mixed {case}-{width} {storage} (reference {list(counts.values())}, {bt.seconds:.1f} s of reference)"))
    finally:
        hd.smp.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES)
def test_full_width_capped_solves_return_the_iterate_of_the_cap(gpu_ctx, base, case, storage):
    cfg = FULL_CASES[case]
    width, caps = cfg["width"], (1, 2, 9)
    bt = _batch(base, case, storage)
    cols = bt.capped(caps)
    sel = [i for i, c in enumerate(cols) if c is not None]
    assert all(cols[i].run.iterations == max(caps) and not cols[i].run.converged for i in sel if i != 7), "the cap must be what stops the reference"
    assert cols[7].run.iterations == 0 and cols[7].run.converged
    zero = np.zeros(bt.hd.n)
    for cap in caps:
        hd = _open_case(gpu_ctx, base, case, storage, rel_tol=1e-14, abs_tol=1e-300, max_iter=cap)
        try:
            (x, st, took), wide = _gated(gpu_ctx, lambda: _solve(gpu_ctx, hd, bt.rhs))
            events = hd.events
            assert took == _expected_path(case, hd, storage, width, FULL_CASES), took
            _check_replays(case, events[0], cap, FULL_CASES)
            # (a solve capped at 1 or 2 applies no deferred update before its end, but lincomb3 runs in every iteration)
            for g in cfg["needs"]:
                assert wide[g] > 0, (case, cap, g, wide)
            worst = _Worst()
            for i in sel:
                p, c = bt.pos[i], cols[i]
                if i == 7:
                    _check_column(c, x[p], st[p], zero, worst, f"{case}-{width} {storage} cap {cap} zero column")
                    continue
                it_dev, conv, ini, fin = st[p]
                where = f"{case}-{width} {storage} cap {cap} column {p}"
                assert (it_dev, conv) == (cap, 0), (where, st[p])
                e_x = np.linalg.norm(x[p] - c.x[cap]) / c.scale
                e_eta = abs(fin - c.run.history[cap]) / c.run.history[cap]
                e_ini = abs(ini - c.run.initial_norm) / c.run.initial_norm
                worst.counts.append(it_dev)
                worst.add("x", e_x, c.tol_x[cap])
                worst.add("eta", e_eta, c.tol_eta[cap])
                worst.add("ini", e_ini, c.tol_ini)
                assert e_ini <= c.tol_ini, (where, "initial_norm", e_ini, c.tol_ini)
                assert e_eta <= c.tol_eta[cap], (where, "final_norm", e_eta, c.tol_eta[cap])
                assert e_x <= c.tol_x[cap], (where, "iterate", e_x, c.tol_x[cap])
            assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0]
            print(worst.line(f"capped at {cap} {case}-{width} {storage}"))
        finally:
            hd.smp.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ["hex16-saddle", "hex8-mini", "hex12-hybrid"])
def test_full_width_warm_start_follows_the_reference_from_its_guess(gpu_ctx, base, case, storage):
    cfg = FULL_CASES[case]
    width = cfg["width"]
    bt = _batch(base, case, storage)
    guess, cols = bt.warm
    counts = [c.run.iterations for c in cols]
    assert len([i for i, c in enumerate(cols) if c.borderline()]) <= 1, counts
    assert counts[4] == 0 and counts[5] == 0 and counts[7] == 0 and min(counts[:4] + counts[6:7] + counts[8:]) > 0, counts
    hd = _open_case(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    try:
        (x, st, took), wide = _gated(gpu_ctx, lambda: _solve(gpu_ctx, hd, bt.rhs, guess=guess))
        assert took == _expected_path(case, hd, storage, width, FULL_CASES), took
        for g in cfg["needs"]:
            assert wide[g] > 0, (case, g, wide)
        worst = _Worst()
        for i, (p, c) in enumerate(zip(bt.pos, cols)):
            _check_column(c, x[p], st[p], guess[p], worst, f"warm {case}-{width} {storage} column {p} (scale {_scale(bt, i):g})")
        assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0]
        print(worst.line(f"warm {case}-{width} {storage} (reference {counts})"))
    finally:
        hd.smp.close()


@pytest.mark.parametrize("case,storage", [("hex16-saddle", "fp64"), ("hex16-saddle", "fp32"), ("hex24-hybrid", "fp32")],
                         ids=["hex16-saddle-fp64", "hex16-saddle-fp32", "hex24-hybrid-fp32"])
def test_full_width_blind_iterations_change_nothing(gpu_ctx, base, case, storage):
    """the blind second solve of the trajectory file at full width: after a batch of unit columns the handle polls the mixed
    batch late, and returns bit for bit what a fresh handle returns"""
    bt = _batch(base, case, storage)
    fresh = _open_case(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    used = _open_case(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    try:
        x_f, st_f, _ = _solve(gpu_ctx, fresh, bt.rhs)
        polls_fresh = int(fresh.events[1])
        _, st_u, _ = _solve(gpu_ctx, used, bt.unit_rhs)
        longest = max(t[0] for t in st_u)
        shortest_active = min(t[0] for t in st_f if t[0] > 0)
        assert longest - 4 > shortest_active + 2, "no blind iteration after the first freeze"
        x_b, st_b, _ = _solve(gpu_ctx, used, bt.rhs)
        polls_blind = int(used.events[1])
        issued = max(t[0] for t in st_f)
        issued += issued % 2
        assert polls_fresh == 1 + issued // 2 and 2 <= polls_blind <= 2 + (issued - (longest - 4)) // 2 + 1 < polls_fresh, \
            (polls_fresh, polls_blind, issued, longest)
        assert np.array_equal(x_b, x_f) and st_b == st_f
        print(f"blind {case}-{bt.width} {storage}: unit batch {longest} iterations, mixed batch {sorted({t[0] for t in st_f})}, "
              f"polls {polls_fresh} fresh, {polls_blind} blind")
    finally:
        fresh.smp.close()
        used.smp.close()


# ---------------------------------------------------------------------------------------------------------------------------
# Darcy at full width: every column its own field

DARCY_WIDTH = 256
DARCY_COMPARED = (0, 1, 31, 32, DARCY_WIDTH - 2, DARCY_WIDTH - 1)
DARCY_TWIN = 32
_DARCY = {}


@pytest.fixture(scope="module")
def darcy(gpu_ctx, hex_hierarchy):
    def get(storage):
        if storage not in _DARCY:
            t0 = time.perf_counter()
            _DARCY[storage] = _DarcyBatch(gpu_ctx, hex_hierarchy, False, storage, ncols=DARCY_WIDTH, compared=DARCY_COMPARED)
            _DARCY[storage].seconds = time.perf_counter() - t0
        return _DARCY[storage]
    yield get
    _DARCY.clear()


@pytest.mark.parametrize("storage", STORAGES)
def test_full_width_darcy_realizations_stop_where_their_own_reference_stops(gpu_ctx, darcy, storage):
    bt = darcy(storage)
    t0 = time.perf_counter()
    cols = bt.columns(1e-6, 1e-12, 300, ())
    seconds = bt.seconds + time.perf_counter() - t0
    label = f"darcy-hex-{DARCY_WIDTH} {storage}"
    counts = _check_reference_spread(cols, label, 3, False)
    assert all(c.run.converged for c in cols)
    cfg = dict(width=DARCY_WIDTH, twin=DARCY_TWIN, needs=("NT_FLAT",))
    ds = bt.make(two_streams=2)      # (at 4.4 M rows x realizations the automatic choice depends on what else lives on the device)
    try:
        assert ds.BatchWidth(0) == DARCY_WIDTH
        ((Q, _, sol, st), took), wide = _gated(gpu_ctx, lambda: _darcy_solve(gpu_ctx, ds, bt.k, True))
        assert took == {"WINDOW": 1}, took
        worst = _Worst()
        zero = np.zeros(sol.shape[1])
        for j, c in zip(bt.compared, cols):
            _check_column(c, sol[j], st[j], zero, worst, f"{label} column {j}")
        assert all(t[1] == 1 for t in st)
        print(worst.line(f"{label} full solution (reference {counts}, {seconds:.1f} s of reference)"))
        # Q only: the update touches the rows of supp(obs) alone
        ((Q2, _, st2), took), wide_q = _gated(gpu_ctx, lambda: _darcy_solve(gpu_ctx, ds, bt.k, False))
        assert took == {"INDEXED": 1}, took
        obs = bt.L.obs
        worst_q = 0.0
        for j, c in zip(bt.compared, cols):
            it_dev = st2[j][0]
            assert st2[j][:2] == st[j][:2], (label, j, st2[j], st[j])
            k_tol = c.run.iterations
            q_ref = float(obs @ c.iterate(it_dev))
            assert abs(st2[j][2] - c.run.initial_norm) <= c.tol_ini * c.run.initial_norm
            assert abs(st2[j][3] - c.eta(it_dev)) <= c.tol_eta[k_tol] * c.eta(it_dev)
            bound = c.tol_x[k_tol] * c.scale * np.linalg.norm(obs)
            worst_q = max(worst_q, abs(Q2[j] - q_ref) / bound)
            assert abs(Q2[j] - q_ref) <= bound, (label, "Q", j, Q2[j], q_ref, bound)
            assert abs(Q[j] - q_ref) <= bound, (label, "Q of the full solve", j, Q[j], q_ref, bound)
        print(f"trajectory {label} Q only: |Q - <obs, x_it>| at most {worst_q:.1e} of its bound")
        (_, took_n), narrow = _gated(gpu_ctx, lambda: _darcy_solve(gpu_ctx, ds, bt.k[:DARCY_TWIN], True))
        assert took_n == {"WINDOW": 1}, took_n
        _check_gates(label, cfg, wide, narrow)
        assert wide_q["NT_FLAT"] > 0 and all(wide_q[g] == 0 for g in GATES if g != "NT_FLAT"), wide_q
    finally:
        ds.close()

"""The MINRES loops of the library, iteration by iteration, against oracle/minres_oracle.py (single-vector preconditioned
MINRES in fp64, pinned on its own in test_minres_oracle.py) run on every compared column ALONE, with the operator from scipy
and B^-1 from the fp64 preconditioner oracles (oracle/precond_oracle.py) built from what the handle exports.  Run with -m gpu
on an MI355X.

What the other solver tests cannot see: they compare the CONVERGED field with a direct solve, or one path of the library with
another bit for bit.  A loop that converges but not optimally, that stops an iteration late, or that evaluates
max(rel_tol * beta, abs_tol) wrongly passes the former; an error common to scal1_body / scal2_body, minres_init and the
freeze logic passes the latter.  Here every compared column must stop at exactly the iteration single-vector MINRES stops at
(DESIGN 3), with the iterate of that iteration - and the columns of a batch stop at DIFFERENT iterations:

- the batch: N(0,1) right-hand sides scaled by 1, 1, 1e-4, 1e-6, 1e-8, 1e-10, 1e+8 and an exact zero column (positions 0, 1,
  7, 8, 15, 16, 30, 31 of 32; all 8 of a narrow launch), a bitwise copy of column 0, unit columns elsewhere; rel_tol = 1e-6
  and abs_tol = 1e-9 beta_ref (beta_ref: the reference's median initial norm of the unit columns), so that the columns need a
  relative reduction of max(1e-6, 1e-9 / scale): full length, three shorter ones, and two columns that are never active (the
  abs_tol branch of the goal; the zero column).  Asserted on the reference alone: at least four distinct counts, 0 among them.
  Wide launches carry a ninth compared column, scale 1e-3 at position 6: its relative goal equals the absolute one, so that
  max(rel_tol * beta, abs_tol) and their sum differ by a factor of two there (in the eight others by a thousandth at most, which
  no stop notices: a seeded `goal = rel_tol * beta + abs_tol` passed without it);
- per column: iterations, converged, initial_norm, final_norm against |eta_it|, the solution against the reference iterate of
  the column's own stopping iteration; never-active columns return exactly x0 with final_norm == initial_norm; the copy of
  column 0 equals column 0 bit for bit in solution and statistics (a narrow launch has no ninth column: a second launch
  carries the copy in place of the never-active column, and every other column of it must not change);
- capped solves (max_iter 1 and 9, and 33 = one past the update window on hex16-saddle; rel_tol 1e-14): x_k, |eta_k|,
  iterations == k, converged 0;
- warm starts: the guess is the reference's x_5 in every other compared column (in the scale-1e-8 column its final iterate:
  that column starts converged and must return its guess untouched), zero in the others;
- blind iterations: a batch of unit columns first, then the mixed batch on the same handle - it starts polling at the hinted
  count, long after its short columns froze - equals the mixed batch on a fresh handle bit for bit;
- Darcy: eight realizations of test_gpu_precond.py's fields (their counts differ by themselves: at least three distinct
  ones), each against the reference with its own A(k_j), B(k_j)^-1 and eliminated right-hand side; the full solution
  (want_solution) and the Q-only solve whose update touches the rows of supp(obs) only (minres_wx_idx) against <obs, x_it>;
  the hybridized handle (the back-substituted (u, p) of the reference's multipliers) converged to rel_tol = 1e-3 - its
  default-tolerance solves are not reproducible, which test_hybridized_darcy_realizations_... asserts on the reference - and
  in the capped solves.

The loops (each case asserts the one it SELECTED from pmc_solve_path_count / pmc_fused_lanczos_solves and the roles of
pmc_sampler_vcycle_level, and the number of graph replays from PMC_COUNT_GRAPH_REPLAYS: none outside hex16-graph, and none in
its solve capped at 1, which runs the eager tail alone; the blind runs read PMC_COUNT_POLLS):
  hex16-saddle   hex 4^3 refined twice (17 152 rows), mini_max_rows = 0: eager loop, deferred w / x window
  hex16-late     ... two_streams = 1: update one iteration late, three z vectors
  hex16-graph    ... use_graph = 1, check_every = 2: graph replay, per-iteration minres_wx, eager tail of an odd max_iter
  hex8-mini      hex 4^3 refined once (2 240 rows): mini_sampler_kernel (the second copy of the recurrences)
  tet-mini       tet-saddle of the preconditioner tests: mini_sampler_kernel on tetrahedra
  hex8-mini-deg3     hex 4^3 refined once at corlen 2 under the deg3 options of precond_cases.py (smoothers of degree 3 on
                     [lmax / 5, lmax], bottom of degree 2): mini_sampler_kernel with the tail's general loop
  hex16-saddle-deg3  hex16-saddle under the full deg3 set: the window loop, the same tail, M-block of degree 3 (cheb_step_z)
  hex12-hybrid   8 columns: level 0 on kernels, fused Lanczos update + r32 (fp32 storage), dense_apply; 32: cycle in the tail, stored q
  hex24-hybrid   43 200 multipliers: fused Lanczos update, r32_top, fused aggregate restriction, row-split narrow levels
  darcy-hex      per-realization operators; window update (solution wanted) and minres_wx_idx (Q only)
  darcy-hex-hybrid   per-realization H(kappa) and multiplier hierarchy, frozen columns back-substituted (rel_tol 1e-3; capped)

Tolerances.  Iteration counts are equal, except for a borderline column (reference history within the measured norm
tolerance d of its goal: |eta_it| > goal (1 - d) or |eta_it-1| < goal (1 + d)), which may differ by one; at most one compared
column per case may be borderline (asserted on the reference).  initial_norm: eta_0^2 = <b, z>, a relative L2 error e of
z = B^-1 b moves it by at most e |b| |z| / <b, z>, hence 0.5 REF_TOL[storage] |b| |z| / <b, z>.  Iterates (relative to
|x_final|) and final_norm (relative to itself) are measured on the reference by perturbing the reference: four reruns of the
oracle with every preconditioner application perturbed by a fresh random vector of relative L2 size p (1e-13 fp64 storage,
1e-7 fp32 storage: the largest preconditioner errors the preconditioner tests print for the sampler and saddle-point Darcy
handles - 1.7e-14, 8.1e-8 - rounded up to a power of ten; 1e-12 and 1e-6 for the hybridized Darcy handle, whose kind prints up
to 1.1e-13 and 1.3e-7 in test_gpu_darcy_internal_precond.py; fp32 storage also rounds z to fp32, as the solver does by
design); the tolerance is 10 times the largest deviation the four runs show for that column and quantity, floor 1e-13.  A
borderline column that the device stops one iteration off is held to the reference's iterate of the device's iteration, with
the tolerances of perturbed reruns to that iteration.

Measured on the MI355X (the printed lines; largest over the compared columns of a case, device against reference |
tolerance).  Every compared column of every case stopped at the reference's iteration; no column of any committed batch is
borderline.  Reference counts of the mixed batches: hex16 29 29 25 16 7 0 29 0 (29), hex8 18 18 15 10 3 0 19 0 (18), tet 39
39 32 20 7 0 39 0 (39), hex12-hybrid 12 12 10 6 2 0 12 0 (12), hex24-hybrid 17 17 14 8 3 0 17 0 narrow, 17 17 15 9 3 0 18 0
(18) wide; Darcy 30 26 57 37 121 35 29 26.
- fp64 storage: iterates at most 4.7e-15 | 3.3e-13 in the mixed batches (hex24-hybrid-32), 5.9e-15 | 6.7e-13 capped, 5.9e-16 |
  1.0e-13 warm; final_norm at most 2.7e-14 | 3.6e-13; initial_norm at most 6.7e-15 | 1.0e-12; Darcy 9.0e-15 | 7.9e-12 (iterate),
  6.6e-14 | 4.4e-10 (final_norm), Q of the compact solve within 2.9e-5 of its bound; hybridized Darcy at rel_tol 1e-3 (counts
  9 9 18 14 19 11 9 9, equal): 8.8e-13 | 4.9e-9 (iterate), 1.5e-13 | 2.2e-8 (final_norm), capped at 9: 1.5e-13 | 7.7e-10;
- fp32 storage: iterates at most 1.5e-8 | 4.2e-7 mixed, 3.0e-8 | 7.7e-7 capped at 1, 4.8e-9 | 2.6e-7 at 9, 8.8e-11 | 3.7e-9 at
  33, 3.1e-10 | 8.4e-9 warm; final_norm at most 9.6e-8 | 2.2e-6; initial_norm at most 1.4e-9 | 7.6e-6; the mini kernel keeps
  everything in fp64 and stays at 4.2e-16 ... 6.3e-16 in both storages; Darcy 2.0e-9 | 7.8e-6 (iterate), 9.0e-7 | 5.2e-5
  (final_norm), 4.0e-7 | 1.6e-5 capped at 1; hybridized Darcy at rel_tol 1e-3 (counts equal; column 2 is the one borderline
  column of the fp32 reference): 1.2e-5 | 5.1e-3 (iterate, the 1e3-contrast column; the others 1.5e-10 ... 1.5e-7), 7.0e-8 |
  2.2e-2 (final_norm), capped 1.2e-5 | 4.4e-2 at 1 and 2.3e-7 | 7.7e-4 at 9;
- hybridized Darcy at the default rel_tol 1e-6, printed and not compared (the reference has 2 borderline columns in fp64
  storage, 7 in fp32; its perturbed reruns are off by 2.5e-2 and 5.1e-2 in |eta| on the rough columns, 4.0e-1 with the fp32
  model): reference counts 18 17 140 45 109 30 18 17; the device's are the same in fp64 storage, with final_norm off by 9.2e-7
  and 1.5e-4 on the two rough columns (1.2e-14 and less elsewhere) - its structured error moves the trajectory far less than
  the isotropic model does - and 18 17 142 45 111 30 18 17 in fp32 storage: two columns two iterations late;
- the largest share of a tolerance any quantity used: 0.12 (final_norm, hex12-hybrid-8 fp32 capped at 9: 3.9e-8 | 3.3e-7);
- blind iterations: unit batch 29 (18) iterations, the mixed batch's columns froze at 7, 16, 25 (3, 9, 15, 17): bit for bit
  the fresh handle's result, with 5 convergence polls where the fresh handle makes 16 (10).
Seeded one at a time in a scratch copy, each of these fails this file: the stop test on the previous eta (all mixed, warm
and Darcy cases), goal = rel_tol beta + abs_tol (the 12 wide mixed cases), the inactive branch of scal2_body leaving its
coefficients in place (mixed, warm, blind, Darcy), final_norm taken before the update (every comparison of a norm), abs_tol
dropped from the mini kernel's goal (the four mini cases and their warm starts), rho3 from sigma1 (everything but the blind
runs).  test_gpu_wx_window.py, test_gpu_solve_edges.py and test_gpu_fused_lanczos.py together noticed the third (16 tests) and
the last (one test) of the six."""
import zlib

import numpy as np
import pytest

from oracle.minres_oracle import minres
from precond_cases import REF_TOL, Handle, darcy_fields, darcy_hex_problem

pytestmark = pytest.mark.gpu

STORAGES = ("fp64", "fp32")
REL_TOL = 1e-6
SCALES = (1.0, 1.0, 1e-4, 1e-6, 1e-8, 1e-10, 1e8, 0.0)
# relative size of the perturbation of every preconditioner application in the reruns of the reference: the largest error the
# preconditioner tests print for the handle kind and storage, rounded up to a power of ten - 1.7e-14 / 8.1e-8 on the sampler
# and saddle-point Darcy handles (test_gpu_sampler_precond.py, test_gpu_precond.py), 1.1e-13 / 1.3e-7 on the hybridized Darcy
# handles (test_gpu_darcy_internal_precond.py)
PERTURBATION = {"fp64": 1e-13, "fp32": 1e-7}
PERTURBATION_DARCY_HYBRID = {"fp64": 1e-12, "fp32": 1e-6}
PERTURBED_RUNS = 4
MARGIN, FLOOR = 10.0, 1e-13

# case -> handle of precond_cases.SOLVE_HANDLES, solver options, the loop it must take, launch widths
SAMPLER_CASES = {
    "hex16-saddle": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0), path="WINDOW", widths=(32,)),
    "hex16-late": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0, two_streams=1), path="LATE", widths=(32,)),
    "hex16-graph": dict(handle="hex16-saddle", opts=dict(mini_max_rows=0, use_graph=1, check_every=2, two_streams=2),
                        path="GRAPH", widths=(32,)),
    "hex8-mini": dict(handle="hex8-saddle", opts={}, path="MINI", widths=(32,)),
    "tet-mini": dict(handle="tet-saddle", opts={}, path="MINI", widths=(32,)),
    "hex12-hybrid": dict(handle="hex12-hybrid", opts={}, path="WINDOW", widths=(8, 32)),
    "hex24-hybrid": dict(handle="hex24-hybrid", opts={}, path="WINDOW", widths=(8, 32)),
    # whole solves under the deg3 option set of precond_cases.OPTION_SETS (the handles carry the options, so that the
    # reference preconditioner is exported under them): the tail's general smoothing loop and one-pass bottom inside
    # mini_sampler_kernel (degree-2 M-block, which that kernel requires; hex 4^3 refined once at corlen 2, where the cycle
    # descends), and in the window loop the same tail beside an M-block of degree 3 through cheb_apply_z's unfused loop
    # (cheb_step_z into the typed z)
    "hex8-mini-deg3": dict(handle="hex8-long-deg3", opts={}, path="MINI", widths=(32,)),
    "hex16-saddle-deg3": dict(handle="hex16-saddle-deg3", opts=dict(mini_max_rows=0), path="WINDOW", widths=(32,)),
}
CASE_WIDTHS = [(c, w) for c, cfg in SAMPLER_CASES.items() for w in cfg["widths"]]
CASE_IDS = [f"{c}-{w}" for c, w in CASE_WIDTHS]


def _paths(ctx):
    from parelagmc_amd import capi
    names = ("MINI", "GRAPH", "LATE", "INDEXED", "WINDOW", "PLAIN")
    out = {nm: ctx.lib.pmc_solve_path_count(getattr(capi, "PMC_PATH_" + nm)) for nm in names}
    out["FUSED"] = ctx.lib.pmc_fused_lanczos_solves()
    return out


def _events(ctx):
    """(graph replays, convergence polls) so far"""
    from parelagmc_amd import capi
    return np.array([ctx.lib.pmc_solve_path_count(capi.PMC_COUNT_GRAPH_REPLAYS),
                     ctx.lib.pmc_solve_path_count(capi.PMC_COUNT_POLLS)], dtype=np.int64)


def _took(before, after):
    return {nm: after[nm] - before[nm] for nm in after if after[nm] != before[nm]}


def _check_replays(case, replays, issued, cases=None):
    """pmc_solve_path_count says which loop a solve SELECTED; that the graph path really replayed is read from the replay
    count: `issued` iterations (an even number, or max_iter) = one eager pair, the replays, the eager tail of an odd max_iter.
    cases: another case table than SAMPLER_CASES (test_gpu_minres_full_width.py)"""
    if (cases or SAMPLER_CASES)[case]["path"] == "GRAPH":
        assert replays == max(issued // 2 - 1, 0), (case, replays, issued)
    else:
        assert replays == 0, (case, replays)


def _positions(width):
    """where the eight compared columns sit: both ends of the launch and of its quarters (0, 1, 7, 8, 15, 16, 30, 31 of 32)"""
    if width == 8:
        return list(range(8))
    return [0, 1, width // 4 - 1, width // 4, width // 2 - 1, width // 2, width - 2, width - 1]


COPY_AT = 5       # wide launches: the bitwise copy of column 0 (a unit column's place)
# wide launches: a ninth compared column whose relative goal EQUALS the absolute one (rel_tol * scale = 1e-9): the only column
# that tells max(rel_tol * beta, abs_tol) from their sum - in every other one the two differ by three orders or more
EXTRA_AT, EXTRA_SCALE = 6, 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the reference of one column, with its measured tolerances

class _Column:
    """reference run of one column and what its perturbed reruns say about the attainable accuracy"""

    def __init__(self, A, Binv, b, x0, rel_tol, abs_tol, max_iter, keep, storage, rng, out=None, pert=None):
        self.storage, self.rng, self.pert = storage, rng, pert
        self.out = out if out is not None else (lambda x: x)     # what the device returns of an iterate
        x0 = np.zeros_like(b) if x0 is None else x0
        r0 = b - A @ x0 if np.any(x0) else b
        z0 = Binv(r0)
        bz = float(r0 @ z0)
        self.tol_ini = 0.5 * REF_TOL[storage] * np.linalg.norm(r0) * np.linalg.norm(z0) / bz if bz > 0 else 0.0
        self.run = run = minres(A, Binv, b, x0, rel_tol, abs_tol, max_iter, keep=keep)
        self.A, self.Binv, self.b, self.x0 = A, Binv, b, x0
        it = run.iterations
        self.ks = sorted({k for k in keep if 0 < k <= it} | ({it} if it else set()))
        self.x = {k: self.out(run.iterates[k]) for k in self.ks if k in run.iterates}
        self.x[it] = self.out(run.x)
        self.scale = np.linalg.norm(self.x[it])
        self.tol_x, self.tol_eta = {}, {}
        if it == 0:
            return
        dev_x = dict.fromkeys(self.ks, 0.0)
        dev_e = dict.fromkeys(self.ks, 0.0)
        p, f32 = (pert or PERTURBATION)[storage], storage == "fp32"

        def rough(r):
            z = Binv(r)
            g = rng.standard_normal(z.shape)
            z = z + (p * np.linalg.norm(z) / np.linalg.norm(g)) * g
            return z.astype(np.float32).astype(np.float64) if f32 else z

        for _ in range(PERTURBED_RUNS):
            pr = minres(A, rough, b, x0, 0.0, 0.0, it, keep=self.ks)
            for k in self.ks:
                if k > pr.iterations:
                    continue
                xk = self.out(pr.iterates[k])
                dev_x[k] = max(dev_x[k], np.linalg.norm(xk - self.x[k]) / self.scale)
                dev_e[k] = max(dev_e[k], abs(pr.history[k] - run.history[k]) / run.history[k])
        self.tol_x = {k: max(MARGIN * dev_x[k], FLOOR) for k in self.ks}
        self.tol_eta = {k: max(MARGIN * dev_e[k], FLOOR) for k in self.ks}

    def borderline(self):
        """the reference history comes within the norm tolerance of the goal at the stop (or one iteration before it)"""
        run, it = self.run, self.run.iterations
        h, goal = run.history, run.goal
        if it == 0:
            return bool(run.converged and h[0] > goal * (1.0 - 1e-6))      # never active: eta_0 against the goal
        if not run.converged:
            return False                                                    # stopped by max_iter
        d = self.tol_eta[it]
        return bool(h[it] > goal * (1.0 - d) or h[it - 1] < goal * (1.0 + d))

    def iterate(self, k):
        """x_k and |eta_k| past the reference's own stop (a borderline column the device stopped elsewhere)"""
        if k not in self.x:
            run = minres(self.A, self.Binv, self.b, self.x0, 0.0, 0.0, k)
            assert run.iterations == k
            self.x[k] = self.out(run.x)
            self._eta = {**getattr(self, "_eta", {}), k: run.history[k]}
        return self.x[k]

    def eta(self, k):
        h = self.run.history
        return h[k] if k < len(h) else self._eta[k]


class _Worst:
    """largest device-against-reference deviations of a case and the tolerances they were held to"""

    def __init__(self):
        self.v = {"x": (0.0, 0.0), "eta": (0.0, 0.0), "ini": (0.0, 0.0)}
        self.counts = []

    def add(self, key, dev, tol):
        if dev >= self.v[key][0]:
            self.v[key] = (dev, tol)

    def line(self, label):
        return (f"trajectory {label}: iterations {self.counts}  " +
                "  ".join(f"{k} {d:.1e} | {t:.1e}" for k, (d, t) in self.v.items()))


def _check_column(col, x_dev, stat, x0_dev, worst, where, k_cap=None):
    """one device column against its reference column; x0_dev: the guess the device was given (exact-return cases)"""
    run = col.run
    it_dev, conv, ini, fin = stat
    it = run.iterations
    worst.counts.append(it_dev)
    if it == 0:
        assert not col.borderline(), (where, "a never-active column too close to its goal: pick another seed")
        assert (it_dev, conv) == (0, 1 if run.converged else 0), (where, stat)
        assert fin == ini, (where, stat)
        assert np.array_equal(x_dev, x0_dev), (where, "a never-active column must return its guess exactly")
        assert abs(ini - run.initial_norm) <= col.tol_ini * run.initial_norm, (where, ini, run.initial_norm)
        return
    if it_dev != it:
        assert col.borderline() and abs(it_dev - it) == 1, (where, f"stopped at {it_dev}, the reference at {it}",
                                                            list(run.history[max(it - 2, 0):]), run.goal)
        # the device stopped by its own goal one iteration off: held to the reference's iterate of THAT iteration, with the
        # tolerances its own perturbed reruns give
        assert conv == 1, (where, stat)
        alt = _Column(col.A, col.Binv, col.b, col.x0, 0.0, 0.0, it_dev, (), col.storage, col.rng, col.out, col.pert)
        assert alt.run.iterations == it_dev
        alt.tol_ini, alt.scale = col.tol_ini, col.scale
        col, it = alt, it_dev
        x_ref = col.x[it]
    else:
        x_ref = col.x[it]
        assert conv == (1 if run.converged else 0), (where, stat)
    if k_cap is not None:
        assert (it_dev, conv) == (k_cap, 0), (where, stat)
    k_tol = it
    e_ini = abs(ini - run.initial_norm) / run.initial_norm
    e_eta = abs(fin - col.eta(it)) / col.eta(it)
    e_x = np.linalg.norm(x_dev - x_ref) / col.scale
    worst.add("ini", e_ini, col.tol_ini)
    worst.add("eta", e_eta, col.tol_eta[k_tol])
    worst.add("x", e_x, col.tol_x[k_tol])
    print(f"  {where}: it {it_dev} (ref {run.iterations}) conv {conv}  x {e_x:.2e} | {col.tol_x[k_tol]:.2e}  "
          f"eta {e_eta:.2e} | {col.tol_eta[k_tol]:.2e}  ini {e_ini:.2e} | {col.tol_ini:.2e}")
    assert e_ini <= col.tol_ini, (where, "initial_norm", e_ini, col.tol_ini)
    assert e_eta <= col.tol_eta[k_tol], (where, "final_norm", it, e_eta, col.tol_eta[k_tol])
    assert e_x <= col.tol_x[k_tol], (where, "iterate", it, e_x, col.tol_x[k_tol])


# ---------------------------------------------------------------------------------------------------------------------------
# sampler handles

_BASE = {}        # (handle, storage) -> Handle with default options: setup values, prolongators, the preconditioner oracle
_REFS = {}        # (kind, handle, storage, width) -> reference of a batch


@pytest.fixture(scope="module")
def base(gpu_ctx):
    def get(handle, storage):
        if (handle, storage) not in _BASE:
            _BASE[(handle, storage)] = Handle(gpu_ctx, handle, storage)
        return _BASE[(handle, storage)]
    yield get
    for hd in _BASE.values():
        hd.smp.close()
    _BASE.clear()
    _REFS.clear()


def _operator(hd):
    if hd.hybrid:
        return hd.prob.levels[0].H.tocsr()
    from oracle.sampler_oracle import SamplerOracle
    return SamplerOracle(hd.prob).block_operator(0).tocsr()


class _Batch:
    """the mixed batch of a (handle, storage, width) with the reference of its compared columns.  pos: the places of the
    eight scaled columns and the ninth one, copy_at: the place of the copy of column 0, seed: the label the generator is
    seeded from (defaults: the places and the seed of this file's cases; test_gpu_minres_full_width.py passes its own)"""

    def __init__(self, hd, handle, storage, width, pos=None, copy_at=None, seed=None):
        self.hd, self.width, self.storage = hd, width, storage
        self.narrow = hd.narrow(width)
        self.A = _operator(hd)
        self.Binv = lambda r: hd.oracle.apply(r, self.narrow)
        self.rng = np.random.Generator(np.random.PCG64(zlib.crc32((seed or f"{handle}/{width}").encode())))
        self.pos = list(pos) if pos is not None else _positions(width) + ([EXTRA_AT] if width > 8 else [])
        self.scales = SCALES + ((EXTRA_SCALE,) if width > 8 else ())
        rhs = self.rng.standard_normal((width, hd.n))
        unit = [j for j in range(width) if j not in self.pos[2:]]
        z = [self.Binv(rhs[j]) for j in unit]
        self.beta_ref = float(np.median([np.sqrt(rhs[j] @ zj) for j, zj in zip(unit, z)]))
        self.abs_tol = 1e-9 * self.beta_ref
        for p, s in zip(self.pos, self.scales):
            rhs[p] *= s
        self.copy_at = (COPY_AT if copy_at is None else copy_at) if width > 8 else None
        if self.copy_at is not None:
            assert self.copy_at not in self.pos and len(set(self.pos)) == len(self.pos)
            rhs[self.copy_at] = rhs[0]
        self.rhs = rhs
        self.unit_rhs = self.rng.standard_normal((width, hd.n))
        self._mixed = self._capped = self._warm = None

    def column(self, p, x0, rel_tol, abs_tol, max_iter, keep):
        return _Column(self.A, self.Binv, self.rhs[p], x0, rel_tol, abs_tol, max_iter, keep, self.storage, self.rng)

    @property
    def mixed(self):
        if self._mixed is None:
            self._mixed = [self.column(p, None, REL_TOL, self.abs_tol, 300, (5,)) for p in self.pos]
        return self._mixed

    def capped(self, caps):
        if self._capped is None or self._capped[0] != caps:
            cols = [self.column(p, None, 1e-14, 0.0, max(caps), caps) for p in self.pos]
            self._capped = (caps, cols)
        return self._capped[1]

    @property
    def warm(self):
        """(guess, columns): x_5 of the mixed reference in every other compared column, the final iterate in the scale-1e-8 one"""
        if self._warm is None:
            guess = np.zeros_like(self.rhs)
            for i, (p, c) in enumerate(zip(self.pos, self.mixed)):
                if i == 4:
                    guess[p] = c.run.x                 # the short column starts converged: never active, nonzero guess
                elif i % 2 == 0:
                    guess[p] = c.run.iterates[5]
            if self.copy_at is not None:
                guess[self.copy_at] = guess[0]
            cols = [self.column(p, guess[p], REL_TOL, self.abs_tol, 300, ()) for p in self.pos]
            self._warm = (guess, cols)
        return self._warm


def _batch(base, case, storage, width):
    handle = SAMPLER_CASES[case]["handle"]
    key = (handle, storage, width)
    if key not in _REFS:
        _REFS[key] = _Batch(base(handle, storage), handle, storage, width)
    return _REFS[key]


def _open(ctx, base, case, storage, cases=None, **opts):
    """a fresh handle of the case with the given tolerances; its setup must be the one the reference was built from"""
    cfg = (cases or SAMPLER_CASES)[case]
    hd = Handle(ctx, cfg["handle"], storage, **cfg["opts"], **opts)
    b = base(cfg["handle"], storage)
    assert hd.setup == b.setup and all((p != q).nnz == 0 for p, q in zip(hd.P, b.P)), "the options changed the preconditioner"
    return hd


def _expected_path(case, hd, storage, width, cases=None):
    """the counters one solve of the case must move, from the case table and the handle's own report of its cycle"""
    from oracle.precond_oracle import ROLE_DESCEND, ROLE_EXACT
    cases = cases or SAMPLER_CASES
    want = {cases[case]["path"]: 1}
    if hd.hybrid:
        narrow = hd.narrow(width)
        m0 = hd.setup[0]
        top_on_kernels = not (m0["tail_narrow"] if narrow else m0["tail_wide"])
        assert int(m0["role_wide"]) == ROLE_DESCEND
        if cases[case]["handle"] == "hex12-hybrid":
            # narrow: level 0 on kernels, the exact dense solve on level 1; wide: the whole cycle inside the tail
            assert top_on_kernels == narrow and int(hd.setup[1]["role_narrow"]) == ROLE_EXACT
        else:
            assert top_on_kernels
            assert storage == "fp64" or (hd.info[0]["fused_restriction"] and hd.info[1]["narrow_pieces"] > 1)
        if top_on_kernels and storage == "fp32":
            want["FUSED"] = 1          # the two operator passes need the fp32 copy of the Lanczos vector (r32)
    elif cases[case]["path"] == "MINI":
        assert hd.n <= hd.opts.mini_max_rows and hd.info[0]["in_tail"]
    else:
        assert hd.n > hd.opts.mini_max_rows
    return want


def _solve(ctx, hd, rhs, guess=None):
    """solution, statistics, the path counters the solve moved; hd.events: its (graph replays, convergence polls)"""
    before, ev = _paths(ctx), _events(ctx)
    x, st = hd.smp.Solve(0, rhs, guess=guess, return_stats=True)
    hd.events = _events(ctx) - ev
    return x, st, _took(before, _paths(ctx))


def _check_reference_spread(cols, label, distinct, need_zero):
    counts = [c.run.iterations for c in cols]
    assert len(set(counts)) >= distinct and (not need_zero or 0 in counts), (label, counts)
    border = [i for i, c in enumerate(cols) if c.borderline()]
    near = [(i, c.run.iterations, f"{c.run.history[max(c.run.iterations - 1, 0)] / c.run.goal:.4f}",
             f"{c.run.history[-1] / c.run.goal:.4f}", f"{c.tol_eta.get(c.run.iterations, 0.0):.1e}") for i, c in enumerate(cols)
            if c.run.goal > 0]
    assert len(border) <= 1, (label, "more than one borderline column: pick another seed", border, near)
    return counts


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case,width", CASE_WIDTHS, ids=CASE_IDS)
def test_mixed_batch_stops_column_by_column_where_the_reference_stops(gpu_ctx, base, case, width, storage):
    bt = _batch(base, case, storage, width)
    cols = bt.mixed
    counts = _check_reference_spread(cols, (case, width, storage), 4, True)
    assert counts[5] == 0 and counts[7] == 0 and min(counts[:5] + counts[6:7] + counts[8:]) > 0, counts
    hd = _open(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    try:
        x, st, took = _solve(gpu_ctx, hd, bt.rhs)
        assert took == _expected_path(case, hd, storage, width), took
        longest = max(t[0] for t in st)
        _check_replays(case, hd.events[0], longest + longest % 2)      # polled after every pair: an even number is issued
        worst = _Worst()
        zero = np.zeros(hd.n)
        for i, (p, c) in enumerate(zip(bt.pos, cols)):
            _check_column(c, x[p], st[p], zero, worst, f"{case}-{width} {storage} column {p} (scale {bt.scales[i]:g})")
        if bt.copy_at is not None:
            assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0], "the copy of column 0 differs from it"
        else:
            # a narrow launch has no ninth column: the copy takes the place of the never-active column of a second launch
            rhs2 = bt.rhs.copy()
            rhs2[5] = rhs2[0]
            x2, st2, _ = _solve(gpu_ctx, hd, rhs2)
            assert np.array_equal(x2[5], x2[0]) and st2[5] == st2[0], "the copy of column 0 differs from it"
            keep = [j for j in range(width) if j != 5]
            assert np.array_equal(x2[keep], x[keep]) and [st2[j] for j in keep] == [st[j] for j in keep]
        # the unit columns nobody compares still converged
        assert all(t[1] == 1 for t in st)
        print(worst.line(f"mixed {case}-{width} {storage} (reference {counts})"))
    finally:
        hd.smp.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case,width", CASE_WIDTHS, ids=CASE_IDS)
def test_capped_solves_return_the_iterate_of_the_cap(gpu_ctx, base, case, width, storage):
    caps = (1, 9, 33) if case == "hex16-saddle" else (1, 9)
    bt = _batch(base, case, storage, width)
    cols = bt.capped(caps)
    assert all(c.run.iterations == max(caps) and not c.run.converged for c in cols[:7] + cols[8:]), "the cap must be what stops the reference"
    assert cols[7].run.iterations == 0 and cols[7].run.converged
    zero = np.zeros(bt.hd.n)
    for cap in caps:
        hd = _open(gpu_ctx, base, case, storage, rel_tol=1e-14, abs_tol=1e-300, max_iter=cap)
        try:
            x, st, took = _solve(gpu_ctx, hd, bt.rhs)
            assert took == _expected_path(case, hd, storage, width), took
            _check_replays(case, hd.events[0], cap)      # cap 1: the eager tail alone; 9: one eager pair, 3 replays, the tail
            worst = _Worst()
            for i, (p, c) in enumerate(zip(bt.pos, cols)):
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
            if bt.copy_at is not None:
                assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0]
            print(worst.line(f"capped at {cap} {case}-{width} {storage}"))
        finally:
            hd.smp.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case,width", [("hex16-saddle", 32), ("hex8-mini", 32), ("hex12-hybrid", 8)],
                         ids=["hex16-saddle-32", "hex8-mini-32", "hex12-hybrid-8"])
def test_warm_start_follows_the_reference_from_its_guess(gpu_ctx, base, case, width, storage):
    bt = _batch(base, case, storage, width)
    guess, cols = bt.warm
    counts = [c.run.iterations for c in cols]
    assert len([i for i, c in enumerate(cols) if c.borderline()]) <= 1, counts
    # the column that starts converged never starts; the others run (the goal is relative to the residual of the guess)
    assert counts[4] == 0 and counts[5] == 0 and counts[7] == 0 and min(counts[:4] + counts[6:7] + counts[8:]) > 0, counts
    hd = _open(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    try:
        x, st, took = _solve(gpu_ctx, hd, bt.rhs, guess=guess)
        want = _expected_path(case, hd, storage, width)
        assert took == want, took
        worst = _Worst()
        for i, (p, c) in enumerate(zip(bt.pos, cols)):
            _check_column(c, x[p], st[p], guess[p], worst, f"warm {case}-{width} {storage} column {p} (scale {bt.scales[i]:g})")
        if bt.copy_at is not None:
            assert np.array_equal(x[bt.copy_at], x[0]) and st[bt.copy_at] == st[0]
        print(worst.line(f"warm {case}-{width} {storage} (reference {counts})"))
    finally:
        hd.smp.close()


@pytest.mark.parametrize("case,width,storage", [("hex16-saddle", 32, "fp64"), ("hex16-saddle", 32, "fp32"),
                                                ("hex24-hybrid", 32, "fp32")],
                         ids=["hex16-saddle-fp64", "hex16-saddle-fp32", "hex24-hybrid-fp32"])
def test_blind_iterations_change_nothing(gpu_ctx, base, case, width, storage):
    """after a batch of unit columns the handle polls the mixed batch (same width, same guess mode: the same hint key) first
    at the hinted count less 4 and once half way: its short columns freeze long before anybody looks.  That the second
    solve really ran blind is read from the library's poll count (PMC_COUNT_POLLS): fewer polls than the fresh handle's"""
    bt = _batch(base, case, storage, width)
    fresh = _open(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
    used = _open(gpu_ctx, base, case, storage, rel_tol=REL_TOL, abs_tol=bt.abs_tol)
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
        # a fresh handle polls before the first iteration and after every pair; the hinted one before the first iteration,
        # once half way and from the hint on - not once while the short columns freeze
        assert polls_fresh == 1 + issued // 2 and 2 <= polls_blind <= 2 + (issued - (longest - 4)) // 2 + 1 < polls_fresh, \
            (polls_fresh, polls_blind, issued, longest)
        assert np.array_equal(x_b, x_f) and st_b == st_f
        print(f"blind {case} {storage}: unit batch {longest} iterations, mixed batch {sorted({t[0] for t in st_f})}, "
              f"polls {polls_fresh} fresh, {polls_blind} blind")
    finally:
        fresh.smp.close()
        used.smp.close()


# ---------------------------------------------------------------------------------------------------------------------------
# Darcy handles: per-realization operators and preconditioners

DARCY_COLUMNS = 8


class _DarcyBatch:
    """ncols realizations of darcy_fields with the systems of the `compared` ones (default: DARCY_COLUMNS, all compared, the
    last a twin of column 1; test_gpu_minres_full_width.py passes a full launch and the columns it compares)"""

    def __init__(self, ctx, hex_hierarchy, hybrid, storage, ncols=DARCY_COLUMNS, compared=None):
        from oracle.darcy_oracle import DarcyOracle
        from oracle.precond_oracle import DarcyChainPrecondOracle, DarcyPrecondOracle, chebyshev, vcycle
        from parelagmc_amd import capi
        from parelagmc_amd.fe.darcy_hybrid import darcy_hybrid_level
        self.hybrid, self.storage = hybrid, storage
        self.dp = dp = darcy_hex_problem(hex_hierarchy)
        L = dp.levels[0]
        self.L = L
        self.rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"darcy/{hybrid}".encode())))
        self.k = darcy_fields(self.rng, ncols, L.n_p)
        if compared is None:
            self.k[7] = self.k[1]      # (both are k == 1 already: columns 1 and 7 are bitwise twins)
        self.compared = list(range(ncols)) if compared is None else list(compared)
        st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
        self.make = lambda **kw: capi.DarcySolver(ctx, dp, capi.solver_opts(precond_storage=st, cheb_degree_M=0, **kw),
                                                  hybrid=hybrid)
        ds = self.make()
        setup = ds.vcycle_levels(0)
        o = capi.solver_opts()
        self.systems = []
        if hybrid:
            hl = darcy_hybrid_level(hex_hierarchy.spaces[0], L)
            P = [ds.vcycle_prolongator(0, v) for v in range(len(setup) - 1)]
            oc = DarcyChainPrecondOracle(dp, 0, setup, P, hl)
            deg, ratio = int(setup[0]["smooth_degree"]), setup[0]["smooth_ratio"]
            for j in self.compared:
                kappa = self.k[j] if dp.k_divides else 1.0 / self.k[j]
                lv = oc.levels(self.k[j])
                self.systems.append((hl.operator(kappa).tocsr(), (lambda r, lv=lv: vcycle(lv, r, deg, ratio)), hl.rhs(kappa),
                                     (lambda lam, kappa=kappa: np.concatenate(hl.back_substitute(kappa, lam)))))
        else:
            do = DarcyOracle(dp)
            po = DarcyPrecondOracle(dp, o.mg_smooth_degree, o.mg_smooth_ratio, o.mg_coarse_degree, o.mg_coarse_ratio)
            ratio_M, deg_M = setup[0]["ratio_M"], int(setup[0]["degree_M"])
            for j in self.compared:
                A, rhs = do.assemble(0, self.k[j])
                M, _ = po.mass(0, self.k[j])
                l1inv = 1.0 / np.asarray(abs(M).sum(axis=1)).ravel()
                lv = po.schur_levels(0, self.k[j])

                def Binv(r, M=M, l1inv=l1inv, lv=lv):
                    return np.concatenate([chebyshev(M, l1inv, r[:L.n_u], deg_M, 1.0, ratio_M),
                                           vcycle(lv, r[L.n_u:], *po.smooth)])
                self.systems.append((A.tocsr(), Binv, rhs, None))
        ds.close()
        self._cols = {}

    def columns(self, rel_tol, abs_tol, max_iter, keep):
        key = (rel_tol, abs_tol, max_iter, tuple(keep))
        if key not in self._cols:
            pert = PERTURBATION_DARCY_HYBRID if self.hybrid else None
            self._cols[key] = [_Column(A, Binv, b, None, rel_tol, abs_tol, max_iter, keep, self.storage, self.rng, out, pert)
                               for A, Binv, b, out in self.systems]
        return self._cols[key]


_DARCY = {}


@pytest.fixture(scope="module")
def darcy(gpu_ctx, hex_hierarchy):
    def get(hybrid, storage):
        if (hybrid, storage) not in _DARCY:
            _DARCY[(hybrid, storage)] = _DarcyBatch(gpu_ctx, hex_hierarchy, hybrid, storage)
        return _DARCY[(hybrid, storage)]
    yield get
    _DARCY.clear()


def _darcy_solve(ctx, ds, k, want_solution):
    before = _paths(ctx)
    out = ds.SolveFwd(0, k, want_solution=want_solution, return_stats=True)
    return out, _took(before, _paths(ctx))


@pytest.mark.parametrize("storage", STORAGES)
def test_darcy_realizations_stop_where_their_own_reference_stops(gpu_ctx, darcy, storage):
    """the saddle-point handle at the default stopping rule (the hybridized one: the next test)"""
    bt = darcy(False, storage)
    cols = bt.columns(1e-6, 1e-12, 300, ())
    label = f"darcy-hex {storage}"
    counts = _check_reference_spread(cols, label, 3, False)
    assert all(c.run.converged for c in cols)
    ds = bt.make()
    try:
        (Q, _, sol, st), took = _darcy_solve(gpu_ctx, ds, bt.k, True)
        assert took == {"WINDOW": 1}, took
        worst = _Worst()
        zero = np.zeros(sol.shape[1])
        for j, c in enumerate(cols):
            _check_column(c, sol[j], st[j], zero, worst, f"{label} column {j}")
        assert np.array_equal(sol[7], sol[1]) and st[7] == st[1] and Q[7] == Q[1], "the twin realizations differ"
        print(worst.line(f"{label} full solution (reference {counts})"))
        # Q only: the update touches the rows of supp(obs) alone
        (Q2, _, st2), took = _darcy_solve(gpu_ctx, ds, bt.k, False)
        assert took == {"INDEXED": 1}, took
        obs = bt.L.obs
        worst_q = 0.0
        for j, c in enumerate(cols):
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
        assert Q2[7] == Q2[1] and st2[7] == st2[1]
        print(f"trajectory {label} Q only: |Q - <obs, x_it>| at most {worst_q:.1e} of its bound")
    finally:
        ds.close()


HYBRID_REL_TOL = 1e-3


@pytest.mark.parametrize("storage", STORAGES)
def test_hybridized_darcy_realizations_stop_where_their_own_reference_stops(gpu_ctx, darcy, storage):
    """the hybridized handle - per-realization H(kappa), a multiplier hierarchy refreshed per realization, the back-substitution
    of frozen columns - converged to rel_tol = 1e-3, where its eight realizations stop at 9 ... 19 iterations.

    Why not at the default 1e-6: there the trajectories of the rough realizations (variance 2.25, 4 and 9, the 1e3-contrast
    field: 30 ... 140 iterations) are not reproducible - their residual sits on a plateau from about k = 33 on while Ritz
    values converge, and finite-precision Lanczos amplifies any perturbation; the reference's own perturbed reruns deviate from
    it by 3e-12 in |eta| at k = 22 but by 2.6e-2 at k = 45.  With such a norm tolerance d a column is borderline whatever the
    seed, and the cap of one borderline column per case is not raised.  That is asserted below ON THE REFERENCE (more than
    one borderline column at 1e-6), so that this test says so if a later preconditioner makes those solves comparable; what
    the device does there is printed (counts beside the reference's) and asserted only to converge."""
    bt = darcy(True, storage)
    cols = bt.columns(HYBRID_REL_TOL, 1e-12, 300, ())
    label = f"darcy-hex-hybrid {storage} rel_tol {HYBRID_REL_TOL:g}"
    counts = _check_reference_spread(cols, label, 3, False)
    assert all(c.run.converged for c in cols)
    ds = bt.make(rel_tol=HYBRID_REL_TOL)
    try:
        (Q, _, sol, st), took = _darcy_solve(gpu_ctx, ds, bt.k, True)
        assert took == {"WINDOW": 1}, took
        worst = _Worst()
        zero = np.zeros(sol.shape[1])
        for j, c in enumerate(cols):
            _check_column(c, sol[j], st[j], zero, worst, f"{label} column {j}")
        assert np.array_equal(sol[7], sol[1]) and st[7] == st[1] and Q[7] == Q[1], "the twin realizations differ"
        # every column froze at its own iteration and the batch ran on to the longest: Q = <obs, the frozen iterate>
        obs = bt.L.obs
        for j, c in enumerate(cols):
            x_ref = c.x[st[j][0]] if st[j][0] in c.x else c.iterate(st[j][0])
            bound = c.tol_x[c.run.iterations] * c.scale * np.linalg.norm(obs)
            assert abs(Q[j] - float(obs @ x_ref)) <= bound, (label, "Q", j, Q[j], float(obs @ x_ref), bound)
        print(worst.line(f"{label} (reference {counts})"))
    finally:
        ds.close()
    # the default stopping rule, on the reference: not comparable under the cap ...
    tight = bt.columns(1e-6, 1e-12, 300, ())
    border = [j for j, c in enumerate(tight) if c.borderline()]
    devs = [f"{c.tol_eta[c.run.iterations] / MARGIN:.1e}" for c in tight]
    print(f"trajectory darcy-hex-hybrid {storage} rel_tol 1e-6, reference alone: counts {[c.run.iterations for c in tight]}, "
          f"|eta| of the perturbed reruns off by {devs}, borderline columns {border}")
    assert len(border) > 1, "the default-tolerance solves have become comparable: compare them"
    # ... and the device there, for the record
    ds = bt.make()
    try:
        (_, _, _, st6), _ = _darcy_solve(gpu_ctx, ds, bt.k, True)
        assert all(t[1] == 1 for t in st6)
        print(f"trajectory darcy-hex-hybrid {storage} rel_tol 1e-6, device: counts {[t[0] for t in st6]}, final_norm off by "
              f"{[f'{abs(t[3] - c.eta(t[0])) / c.eta(t[0]):.1e}' if t[0] <= c.run.iterations else 'n/a' for t, c in zip(st6, tight)]}")
    finally:
        ds.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("hybrid", [False, True], ids=["darcy-hex", "darcy-hex-hybrid"])
def test_darcy_capped_solves_return_the_iterate_of_the_cap(gpu_ctx, darcy, hybrid, storage):
    bt = darcy(hybrid, storage)
    caps = (1, 9)
    cols = bt.columns(1e-14, 0.0, max(caps), caps)
    assert all(c.run.iterations == max(caps) and not c.run.converged for c in cols)
    label = f"darcy-hex{'-hybrid' if hybrid else ''} {storage}"
    for cap in caps:
        ds = bt.make(rel_tol=1e-14, abs_tol=1e-300, max_iter=cap)
        try:
            (_, _, sol, st), took = _darcy_solve(gpu_ctx, ds, bt.k, True)
            assert took == {"WINDOW": 1}, took
            worst = _Worst()
            for j, c in enumerate(cols):
                it_dev, conv, ini, fin = st[j]
                assert (it_dev, conv) == (cap, 0), (label, cap, j, st[j])
                e_x = np.linalg.norm(sol[j] - c.x[cap]) / c.scale
                e_eta = abs(fin - c.run.history[cap]) / c.run.history[cap]
                worst.counts.append(it_dev)
                worst.add("x", e_x, c.tol_x[cap])
                worst.add("eta", e_eta, c.tol_eta[cap])
                worst.add("ini", abs(ini - c.run.initial_norm) / c.run.initial_norm, c.tol_ini)
                assert abs(ini - c.run.initial_norm) <= c.tol_ini * c.run.initial_norm
                assert e_eta <= c.tol_eta[cap], (label, cap, j, "final_norm", e_eta, c.tol_eta[cap])
                assert e_x <= c.tol_x[cap], (label, cap, j, "iterate", e_x, c.tol_x[cap])
            print(worst.line(f"capped at {cap} {label}"))
        finally:
            ds.close()

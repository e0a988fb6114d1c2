"""The multiplier solve that never stores q = H u (two operator passes per MINRES iteration: the dot-only pass for alpha, then
the pass whose epilogue forms the next Lanczos vector and its fp32 copy) against the path that stores q and runs
k::lincomb3 (use_graph = 1, check_every = 2: the captured pair keeps the separate kernels).  The second pass recomputes the
row sums in the same order and combines them with the very expression of lincomb3, so every comparison here is
np.array_equal, on fields and on the solver's statistics.  mini_max_rows = 0 and two_streams = 2 in both, as in
test_gpu_wx_window.py.  Run with -m gpu on an MI355X.

Which path a solve took is read from pmc_fused_lanczos_solves(), the library's count of solves that ran the two passes; every
case asserts it: one per launch where the path must be taken, none on the graph path, with operator timing on, with fp64
storage and for the saddle-point system.

Where the fused path runs: on a level whose V-cycle keeps the fp32 copy of the Lanczos vector - a multi-level aggregation
hierarchy whose top level is outside the LDS tail.  That holds for the finest level of cube_tet r = 3 (V-cycle levels 6 528 /
697 / 74, the tail from the second on), of the hex hierarchy (13 056 / 1 562 / 184) and of the box below (12 272 / 1 474 /
170); FUSED_LEVELS lists, per hierarchy, the sampler levels that take it - the small coarse levels solve inside the tail and
pass through on the storing path.  The multiplier counts of cube_tet r = 3 and of the finest hex level are multiples of 64;
the 5 x 4 x 3 box (12 272 = 191 x 64 + 48) has a last slice with rows past the end, and widths, short solves and the timing
toggle use it."""
import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

MODES = {"fused": dict(use_graph=0), "stored": dict(use_graph=1, check_every=2)}


@pytest.fixture(scope="module")
def tet_hierarchies():
    """cube_tet refined twice and three times (864 and 6 528 multipliers on the finest level)"""
    from parelagmc_amd.fe import build_hierarchy, mesh_from_json
    mesh = mesh_from_json(golden_path("meshes", "cube_tet.json"))
    return {r: build_hierarchy(mesh, r) for r in (2, 3)}


@pytest.fixture(scope="module")
def ragged_box():
    """5 x 4 x 3 hexes refined twice: 12 272 multipliers on the finest level, 48 rows in the last slice"""
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    return build_hierarchy(box_mesh([5, 4, 3], [2, 2, 2], "hex"), 2)


def _problem(h, hybrid=True, corlen=0.1, **kw):
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    return (build_hybrid_sampler_problem if hybrid else build_sampler_problem)(h, corlen=corlen, **kw)


def _fused_solves(ctx):
    return ctx.lib.pmc_fused_lanczos_solves()


def _both(ctx, prob, calls, **opts):
    """every call(sampler) in the eager loop and on the graph path, which stores q: per mode a list of (result, solves
    that took the fused path during the call)"""
    from parelagmc_amd import capi
    out = []
    for mode in ("fused", "stored"):
        smp = capi.PDESampler(ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, **MODES[mode], **opts))
        res = []
        for call in calls:
            n0 = _fused_solves(ctx)
            r = call(smp)
            res.append((r, _fused_solves(ctx) - n0))
        out.append(res)
        smp.close()
    return out


def _same(a, b):
    (s1, st1), (s2, st2) = a, b
    assert np.array_equal(s1, s2)
    assert st1 == st2          # iterations, converged, initial and final norm of every realization, exactly


def _check(f, s, fused_solves, converged=True):
    """eager against graph path, call by call: equal results; the eager loop took the fused path `fused_solves[i]` times in
    call i, the graph path never"""
    assert len(f) == len(s) == len(fused_solves)
    for (a, na), (b, nb), want in zip(f, s, fused_solves):
        _same(a, b)
        assert nb == 0
        assert na == want
        if converged:
            assert all(t[1] == 1 for t in a[1])


def _timed_and_untimed(ctx, prob, level, xi, **opts):
    """the same handle without and with operator timing: (untimed result, fused solves of it), (timed result, fused solves)"""
    from parelagmc_amd import capi
    smp = capi.PDESampler(ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, use_graph=0, **opts))

    def run():
        n0 = _fused_solves(ctx)
        r = smp.Eval(level, xi, xi_level=0, return_stats=True)
        return r, _fused_solves(ctx) - n0

    plain = run()
    smp.set_operator_timing(True)
    timed = run()
    smp.set_operator_timing(False)
    again = run()
    smp.close()
    _same(plain[0], again[0])
    assert again[1] == plain[1]
    return plain, timed


def _eval(lvl, xi):
    return lambda smp: smp.Eval(lvl, xi, xi_level=0, return_stats=True)


# sampler levels whose multiplier solve takes the fused path (the others solve inside the LDS tail)
FUSED_LEVELS = {"tet2": (), "tet3": (0,), "hex": (0,), "box": (0,)}


@pytest.mark.parametrize("r", [2, 3])
def test_fused_equals_stored_on_tetrahedra(gpu_ctx, tet_hierarchies, seeded_rng, r):
    prob = _problem(tet_hierarchies[r], n_mc_levels=2)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(lvl, xi) for lvl in range(2)])
    _check(f, s, [int(lvl in FUSED_LEVELS[f"tet{r}"]) for lvl in range(2)])


def test_fused_equals_stored_on_the_hex_hierarchy(gpu_ctx, hex_hierarchy, seeded_rng):
    """every level of the hex hierarchy at the default tolerance, 16 realizations"""
    prob = _problem(hex_hierarchy, lognormal=True)
    xi = seeded_rng.standard_normal((16, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(lvl, xi) for lvl in range(3)])
    _check(f, s, [int(lvl in FUSED_LEVELS["hex"]) for lvl in range(3)])


def test_the_ragged_box_on_every_level(gpu_ctx, ragged_box, seeded_rng):
    prob = _problem(ragged_box, lognormal=True)
    xi = seeded_rng.standard_normal((16, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(lvl, xi) for lvl in range(3)])
    _check(f, s, [int(lvl in FUSED_LEVELS["box"]) for lvl in range(3)])


@pytest.mark.parametrize("ncols,launches", [(1, 1), (8, 1), (16, 1), (32, 1), (33, 2), (64, 1)])
def test_launch_widths(gpu_ctx, ragged_box, seeded_rng, ncols, launches):
    """the instantiations with 1, 2 and 4 values per thread; this level carries up to 256 realizations per launch (asserted),
    so 64 columns are ONE launch of two column groups.  The binding accepts 33 realizations but cuts them into launches of
    32 and 1 (the widths of a launch are powers of two: no launch has a ragged column group), so 33 checks that cut - two
    fused solves - and 64 the second column group."""
    from parelagmc_amd import capi
    prob = _problem(ragged_box, n_mc_levels=1)
    smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2))
    assert smp.BatchWidth(0) >= 64
    smp.close()
    xi = seeded_rng.standard_normal((ncols, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(0, xi)])
    _check(f, s, [launches])


@pytest.mark.parametrize("ncols", [8, 64])
@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_solves_that_stop_after_the_first_update_passes(gpu_ctx, ragged_box, seeded_rng, max_iter, ncols):
    """rel_tol = 1e-14 is out of reach: the solve stops by max_iter.  One iteration runs only the update pass without v0
    (v0 is never filled on this path), two and three follow it with the pass that reads what the earlier ones wrote"""
    prob = _problem(ragged_box, n_mc_levels=1)
    xi = seeded_rng.standard_normal((ncols, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(0, xi)], rel_tol=1e-14, abs_tol=1e-300, max_iter=max_iter)
    _check(f, s, [1], converged=False)
    assert all(t[0] == max_iter and t[1] == 0 for t in f[0][0][1])


def test_repeated_solves_reuse_the_work_vectors(gpu_ctx, ragged_box, seeded_rng):
    """a second solve on the same handle starts from whatever the first left in v0: the first update pass must not read it"""
    prob = _problem(ragged_box, n_mc_levels=1)
    xi = seeded_rng.standard_normal((2, 8, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(0, x) for x in (xi[0], xi[1], xi[0])])
    _check(f, s, [1, 1, 1])


@pytest.mark.parametrize("mesh", ["tet3", "box"])
def test_operator_timing_takes_the_storing_path_with_the_same_bits(gpu_ctx, tet_hierarchies, ragged_box, seeded_rng, mesh):
    """with operator timing on, the bracket measures the product that stores q, so the solve runs lincomb3; the untimed
    solve of the same handle is the fused one and gives exactly the same result"""
    prob = _problem(tet_hierarchies[3] if mesh == "tet3" else ragged_box, n_mc_levels=1)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    (plain, n_plain), (timed, n_timed) = _timed_and_untimed(gpu_ctx, prob, 0, xi)
    _same(plain, timed)
    assert all(t[1] == 1 for t in plain[1])
    assert (n_plain, n_timed) == (1, 0)


def test_fp64_storage_keeps_the_storing_path(gpu_ctx, ragged_box, seeded_rng):
    from parelagmc_amd import capi
    prob = _problem(ragged_box, n_mc_levels=1)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(0, xi)], precond_storage=capi.PMC_STORAGE_FP64)
    _check(f, s, [0])
    (plain, n_plain), (timed, n_timed) = _timed_and_untimed(gpu_ctx, prob, 0, xi, precond_storage=capi.PMC_STORAGE_FP64)
    _same(plain, timed)
    assert (n_plain, n_timed) == (0, 0)


def test_the_saddle_point_solve_keeps_the_storing_path(gpu_ctx, ragged_box, seeded_rng):
    prob = _problem(ragged_box, hybrid=False, n_mc_levels=1)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    f, s = _both(gpu_ctx, prob, [_eval(0, xi)])
    _check(f, s, [0])
    (plain, n_plain), (timed, n_timed) = _timed_and_untimed(gpu_ctx, prob, 0, xi)
    _same(plain, timed)
    assert (n_plain, n_timed) == (0, 0)

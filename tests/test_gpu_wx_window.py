"""The deferred w / x update of MINRES (k::minres_wx_deferred: the updates of a whole window of up to 32 iterations in one
pass, first pass from literal zeros, last pass without storing w0 / w1) against the path that applies one update per
iteration (use_graph = 1, check_every = 2: minres_wx inside the captured pair).  The recurrences run per entry in iteration
order on both paths - the same operations in the same order - so every comparison here is np.array_equal, on fields and on
the solver's statistics.  mini_max_rows = 0 and two_streams = 2 in both: small saddle-point levels go through minres_solve,
and on one stream, where the deferred path is the default.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

MODES = {"deferred": dict(use_graph=0), "per_iteration": dict(use_graph=1, check_every=2)}


def _problem(h, hybrid, corlen=0.1, **kw):
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    return (build_hybrid_sampler_problem if hybrid else build_sampler_problem)(h, corlen=corlen, **kw)


def _long_problem(h, hybrid):
    """a system whose solve to rel_tol = 1e-14 needs more than 33 iterations: the hybridized system of the hex hierarchy
    takes 18 at the correlation length 0.1 of the other tests and 40 at 0.5 (the saddle-point form is long enough at 0.1)"""
    return _problem(h, hybrid, corlen=0.5 if hybrid else 0.1)


def _both(ctx, prob, run, **opts):
    """run(sampler) with the deferred and with the per-iteration update"""
    from parelagmc_amd import capi
    out = []
    for mode in ("deferred", "per_iteration"):
        smp = capi.PDESampler(ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, **MODES[mode], **opts))
        out.append(run(smp))
        smp.close()
    return out


def _same(a, b):
    (s1, st1), (s2, st2) = a, b
    assert np.array_equal(s1, s2)
    assert st1 == st2          # iterations, converged, initial and final norm of every realization, exactly


@pytest.mark.parametrize("hybrid", [True, False], ids=["hybridized", "saddle"])
def test_deferred_update_equals_the_update_per_iteration(gpu_ctx, hex_hierarchy, seeded_rng, hybrid):
    """every level of the hex hierarchy at the default tolerance, 16 realizations"""
    prob = _problem(hex_hierarchy, hybrid, lognormal=True)
    xi = seeded_rng.standard_normal((16, prob.levels[0].n_s))
    d, p = _both(gpu_ctx, prob, lambda smp: [smp.Eval(lvl, xi, xi_level=0, return_stats=True) for lvl in range(3)])
    for a, b in zip(d, p):
        _same(a, b)
        assert all(t[1] == 1 for t in a[1])


def test_deferred_update_on_tetrahedra(gpu_ctx, seeded_rng):
    """cube_tet refined three times, hybridized (the mesh family of the headline)"""
    from parelagmc_amd.fe import build_hierarchy, mesh_from_json
    h = build_hierarchy(mesh_from_json(golden_path("meshes", "cube_tet.json")), 3)
    prob = _problem(h, True, n_mc_levels=2)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    d, p = _both(gpu_ctx, prob, lambda smp: [smp.Eval(lvl, xi, xi_level=0, return_stats=True) for lvl in range(2)])
    for a, b in zip(d, p):
        _same(a, b)
        assert all(t[1] == 1 for t in a[1])


@pytest.mark.parametrize("hybrid", [True, False], ids=["hybridized", "saddle"])
@pytest.mark.parametrize("max_iter", [1, 7, 8, 9, 31, 32, 33])
def test_solves_that_stop_at_the_window_edges(gpu_ctx, hex_hierarchy, seeded_rng, hybrid, max_iter):
    """rel_tol = 1e-14 is out of reach in so few iterations: the solve stops by max_iter (converged == 0) after exactly
    max_iter updates - one short of a trip of 8, a full trip, one into the next; one short of the window of 32, the full
    window (flushed inside the loop, nothing left for the pass after it), one into the second window"""
    prob = _long_problem(hex_hierarchy, hybrid)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    d, p = _both(gpu_ctx, prob, lambda smp: smp.Eval(0, xi, xi_level=0, return_stats=True), rel_tol=1e-14, abs_tol=1e-300,
                 max_iter=max_iter)
    _same(d, p)
    assert all(t[0] == max_iter and t[1] == 0 for t in d[1])


@pytest.mark.parametrize("hybrid", [True, False], ids=["hybridized", "saddle"])
def test_a_solve_that_converges_beyond_the_window(gpu_ctx, hex_hierarchy, seeded_rng, hybrid):
    prob = _long_problem(hex_hierarchy, hybrid)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    d, p = _both(gpu_ctx, prob, lambda smp: smp.Eval(0, xi, xi_level=0, return_stats=True), rel_tol=1e-14, abs_tol=1e-300,
                 max_iter=400)
    _same(d, p)
    assert all(t[1] == 1 for t in d[1]) and min(t[0] for t in d[1]) > 32


def test_warm_start_is_read_by_the_first_pass(gpu_ctx, hex_hierarchy, seeded_rng):
    """saddle-point sampler with use_init: x holds the prolongated coarse field when the first pass runs, so that pass
    must load it (only w0 / w1 start from literal zeros).  A first pass that ignored x would lose the initial guess."""
    prob = _problem(hex_hierarchy, False)
    n0, n1 = prob.levels[0].n_s, prob.levels[1].n_s
    xi = seeded_rng.standard_normal((8, n0))

    def run(smp):
        coarse = smp.Eval(1, xi, xi_level=0)
        cold = smp.Eval(0, xi, xi_level=0, return_stats=True)
        warm = smp.Eval(0, xi, xi_level=0, init_s=coarse, init_level=1, use_init=True, return_stats=True)
        return cold, warm

    (dc, dw), (pc, pw) = _both(gpu_ctx, prob, run)
    _same(dc, pc)
    _same(dw, pw)
    assert all(t[1] == 1 for t in dw[1])
    assert not np.array_equal(dw[0], dc[0])                       # the guess took part ...
    # ... and both solve the same system: each stops at a preconditioned residual of 1e-6 relative to its start, which
    # bounds the error of either by 1e-6 times the condition of the preconditioned operator (below 100 here)
    assert np.linalg.norm(dw[0] - dc[0]) < 1e-3 * np.linalg.norm(dc[0])


@pytest.mark.parametrize("hybrid", [True, False], ids=["hybridized", "saddle"])
@pytest.mark.parametrize("ncols", [1, 8, 64])
def test_launch_widths(gpu_ctx, hex_hierarchy, seeded_rng, hybrid, ncols):
    """launches of 1, 8 and 64 columns: the instantiations with 1, 2 and 4 values per thread, the last one with two column
    groups of 32"""
    prob = _problem(hex_hierarchy, hybrid)
    xi = seeded_rng.standard_normal((ncols, prob.levels[0].n_s))
    d, p = _both(gpu_ctx, prob, lambda smp: smp.Eval(0, xi, xi_level=0, return_stats=True))
    _same(d, p)
    assert all(t[1] == 1 for t in d[1])

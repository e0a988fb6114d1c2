"""The edges of the hybridized multiplier solve that no longer pass through a stored copy: the right-hand side b = Gz fz that
the solve adopts (its producing kernel writes the first Lanczos vector and the fp32 copy itself, k::spmm_store32, instead
of b and k::copy_r32) and the field that the back-substitution writes sample-major itself (k::residual_samples instead of
k::residual and k::deinterleave).  Both store the very values the two-kernel paths store, so every comparison here is
np.array_equal, on fields and on the solver's statistics, new path against old path in the same library:

  eager     use_graph = 0, no embedded copy     adopted right-hand side, fused field
  embed     use_graph = 0, want_embed           adopted right-hand side, residual + deinterleave (the embedded copy reads
                                                the interleaved field)
  stored    use_graph = 1, check_every = 2,     b stored and copied, q stored, residual + deinterleave: the parent's path
            want_embed

Which path a launch took is read from pmc_adopted_rhs_solves() and pmc_fused_field_evals() and asserted in every case.  The
deferred w / x pass (k::minres_wx_deferred, several entries per thread) runs in `eager` and `embed` only - the graph path
keeps one update launch per iteration - so the same comparisons hold it to the per-iteration kernel: solve lengths 1, 8, 9
and 33 end inside the first trip, on a trip boundary, one past it, and one past the window of 32.

The right-hand side is adopted where the solve keeps the fp32 copy of its Lanczos vectors: the finest level of the 5 x 4 x 3
box (12 272 = 191 x 64 + 48 multipliers, a ragged last slice), of cube_tet r = 3 (6 528) and of the hex hierarchy; coarser
levels solve inside the LDS tail and keep b, but still write their field directly.  A conditioned sampler adopts its
right-hand side (the conditioner only touches the output) and keeps the two output kernels; a warm-started solve and the
saddle-point system take neither path.  mini_max_rows = 0 and two_streams = 2 in all, as in test_gpu_fused_lanczos.py.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

MODES = {"eager": (dict(use_graph=0), False), "embed": (dict(use_graph=0), True),
         "stored": (dict(use_graph=1, check_every=2), True)}


@pytest.fixture(scope="module")
def tet3():
    from parelagmc_amd.fe import build_hierarchy, mesh_from_json
    return build_hierarchy(mesh_from_json(golden_path("meshes", "cube_tet.json")), 3)


@pytest.fixture(scope="module")
def ragged_box():
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    return build_hierarchy(box_mesh([5, 4, 3], [2, 2, 2], "hex"), 2)


def _problem(h, hybrid=True, corlen=0.1, **kw):
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    return (build_hybrid_sampler_problem if hybrid else build_sampler_problem)(h, corlen=corlen, **kw)


def _counts(ctx):
    return np.array([ctx.lib.pmc_adopted_rhs_solves(), ctx.lib.pmc_fused_field_evals()], dtype=np.int64)


def _sampler(ctx, prob, mode, **opts):
    from parelagmc_amd import capi
    return capi.PDESampler(ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, **MODES[mode][0], **opts))


def _eval(ctx, smp, mode, level, xi):
    """(field, stats, embedded copy or None, (adopted right-hand sides, fused fields) of the call)"""
    n0 = _counts(ctx)
    if MODES[mode][1]:
        s, emb, st = smp.Eval(level, xi, xi_level=0, want_embed=True, return_stats=True)
    else:
        (s, st), emb = smp.Eval(level, xi, xi_level=0, return_stats=True), None
    return s, st, emb, tuple(int(v) for v in _counts(ctx) - n0)


def _three_ways(ctx, prob, level, xi, adopted=1, lognormal=False, **opts):
    """the three modes agree bit for bit and each took the path it must; returns the eager result"""
    res = {}
    for mode in MODES:
        smp = _sampler(ctx, prob, mode, **opts)
        res[mode] = _eval(ctx, smp, mode, level, xi)
        smp.close()
    want = {"eager": (adopted, 1), "embed": (adopted, 0), "stored": (0, 0)}
    for mode, (s, st, emb, took) in res.items():
        print(f"{mode}: adopted right-hand sides {took[0]}, fused fields {took[1]}, iterations {max(t[0] for t in st)}")
        assert took == want[mode], mode
        assert np.array_equal(s, res["stored"][0]), mode
        assert st == res["stored"][1], mode
        if emb is not None:      # the Gaussian field: the returned one before exp()
            assert np.array_equal(emb, res["stored"][2]), mode
            if not lognormal:
                assert np.array_equal(s, emb), mode
    return res["eager"]


@pytest.mark.parametrize("lognormal", [False, True])
@pytest.mark.parametrize("mesh", ["box", "tet3"])
def test_adopted_rhs_and_fused_field_equal_the_stored_paths(gpu_ctx, ragged_box, tet3, seeded_rng, mesh, lognormal):
    prob = _problem(ragged_box if mesh == "box" else tet3, lognormal=lognormal, n_mc_levels=1)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    s, st, _, _ = _three_ways(gpu_ctx, prob, 0, xi, lognormal=lognormal)
    assert all(t[1] == 1 for t in st)
    assert np.all(np.isfinite(s)) and (not lognormal or np.all(s > 0.0))


@pytest.mark.parametrize("ncols", [1, 8, 32, 64])
def test_launch_widths(gpu_ctx, ragged_box, seeded_rng, ncols):
    """1, 2 and 4 values per thread, and two column groups in one launch (64)"""
    prob = _problem(ragged_box, lognormal=True, n_mc_levels=1)
    smp = _sampler(gpu_ctx, prob, "eager")
    assert smp.BatchWidth(0) >= 64
    smp.close()
    xi = seeded_rng.standard_normal((ncols, prob.levels[0].n_s))
    _, st, _, _ = _three_ways(gpu_ctx, prob, 0, xi, lognormal=True)
    assert all(t[1] == 1 for t in st)


@pytest.mark.parametrize("max_iter", [1, 8, 9, 33])
def test_solve_lengths(gpu_ctx, ragged_box, hex_hierarchy, seeded_rng, max_iter):
    """rel_tol = 1e-14 is out of reach in so few iterations: every column runs max_iter iterations and stops unconverged.
    1, 8 and 9 on the box (whose solves end after 18 at any tolerance); 33 on the hex hierarchy at correlation length 0.5,
    which needs about 40 to reach 1e-14"""
    prob = _problem(ragged_box, n_mc_levels=1) if max_iter <= 9 else _problem(hex_hierarchy, corlen=0.5)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    _, st, _, _ = _three_ways(gpu_ctx, prob, 0, xi, rel_tol=1e-14, abs_tol=1e-300, max_iter=max_iter)
    assert all(t[0] == max_iter and t[1] == 0 for t in st)


@pytest.mark.parametrize("ncols", [32, 64])
@pytest.mark.parametrize("max_iter", [4, 5, 33])
def test_solve_lengths_at_four_values_per_thread(gpu_ctx, hex_hierarchy, seeded_rng, max_iter, ncols):
    """the instantiation the large levels run (column groups of 32: four entries per thread, trips of four iterations): a
    full trip, one into the next, and one past the window of 32; one and two column groups"""
    prob = _problem(hex_hierarchy, corlen=0.5, n_mc_levels=1)
    xi = seeded_rng.standard_normal((ncols, prob.levels[0].n_s))
    _, st, _, _ = _three_ways(gpu_ctx, prob, 0, xi, rel_tol=1e-14, abs_tol=1e-300, max_iter=max_iter)
    assert all(t[0] == max_iter and t[1] == 0 for t in st)


def test_a_solve_longer_than_the_window_on_the_hex_hierarchy(gpu_ctx, hex_hierarchy, seeded_rng):
    """correlation length 0.5 solved to rel_tol = 1e-14: about 40 iterations, more than one window of 32"""
    prob = _problem(hex_hierarchy, corlen=0.5, lognormal=True)
    xi = seeded_rng.standard_normal((16, prob.levels[0].n_s))
    _, st, _, _ = _three_ways(gpu_ctx, prob, 0, xi, lognormal=True, rel_tol=1e-14, abs_tol=1e-300, max_iter=400)
    assert max(t[0] for t in st) > 32


def test_a_level_inside_the_tail_keeps_b_and_writes_its_field(gpu_ctx, ragged_box, seeded_rng):
    prob = _problem(ragged_box, lognormal=True)
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    _three_ways(gpu_ctx, prob, 1, xi, adopted=0, lognormal=True)


def test_a_warm_start_takes_neither_path(gpu_ctx, ragged_box, seeded_rng):
    """pmc_sampler_mult with an initial guess on the multiplier system, and a warm-started saddle-point Eval: no producer, no
    fused field, the same solution eagerly and on the graph path"""
    prob = _problem(ragged_box, n_mc_levels=1)
    n = prob.levels[0].n_lambda
    rhs = seeded_rng.standard_normal((8, n))
    out = []
    for mode in ("eager", "stored"):
        smp = _sampler(gpu_ctx, prob, mode)
        cold = smp.Solve(0, rhs)
        n0 = _counts(gpu_ctx)
        out.append(smp.Solve(0, rhs, guess=0.5 * cold, return_stats=True))
        assert tuple(_counts(gpu_ctx) - n0) == (0, 0)
        smp.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    sprob = _problem(ragged_box, hybrid=False, n_mc_levels=1)
    xi = seeded_rng.standard_normal((8, sprob.levels[0].n_s))
    res = []
    for mode in ("eager", "stored"):
        smp = _sampler(gpu_ctx, sprob, mode)
        s0 = smp.Eval(0, xi, xi_level=0)
        n0 = _counts(gpu_ctx)
        res.append(smp.Eval(0, xi, xi_level=0, init_s=0.5 * s0, init_level=0, use_init=True, return_stats=True))
        assert tuple(_counts(gpu_ctx) - n0) == (0, 0)
        smp.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


@pytest.mark.parametrize("lognormal", [False, True])
def test_a_conditioned_sampler_keeps_the_two_output_kernels(gpu_ctx, hex_hierarchy, seeded_rng, lognormal):
    """the conditioner updates the sample-major Gaussian field in place (exp fused into its store): the field is never fused
    into the back-substitution, and detaching brings the fused field back with the bits of the two-kernel path"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    prob = _problem(hex_hierarchy, lognormal=lognormal)
    H0 = point_observations(hex_hierarchy.spaces[0].n_s, pick_observation_elements(hex_hierarchy, 16, 16), [])
    y = np.random.default_rng(116).normal(0.0, 1.0, H0.shape[0])
    xi = seeded_rng.standard_normal((8, prob.levels[0].n_s))
    res = {}
    for mode in ("eager", "stored"):
        smp = _sampler(gpu_ctx, prob, mode)
        cond = capi.Conditioner(smp, H0, y)
        smp.SetConditioner(cond)
        n0 = _counts(gpu_ctx)
        s, st = smp.Eval(0, xi, xi_level=0, return_stats=True)
        took = tuple(int(v) for v in _counts(gpu_ctx) - n0)
        smp.SetConditioner(None)
        n0 = _counts(gpu_ctx)
        free = smp.Eval(0, xi, xi_level=0)
        took_free = tuple(int(v) for v in _counts(gpu_ctx) - n0)
        res[mode] = (s, st, took, free, took_free)
        cond.close()
        smp.close()
    assert res["eager"][2] == (1, 0) and res["stored"][2] == (0, 0)
    assert res["eager"][4] == (1, 1) and res["stored"][4] == (0, 1)
    assert np.array_equal(res["eager"][0], res["stored"][0]) and res["eager"][1] == res["stored"][1]
    assert np.array_equal(res["eager"][3], res["stored"][3])

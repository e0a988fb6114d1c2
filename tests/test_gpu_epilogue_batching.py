"""The row-local epilogues of the finest-level kernels of the hybridized sampler at 32 columns per group: the Lanczos update
passes (sell_spmm_kernel, LZ = 2 / 3) keep the lane's coefficients in registers and read the own rows of v1 / v0 for a batch
of row steps together; the one-pass smoother (vc_poly2_kernel) knows its optional operands at compile time and reads the
parent indices of the coarse correction ahead of the gather loop.  Rows past the end of the last slice re-read the last row
and store nothing, in batches, so the tests choose the multiplier counts by what the last slice holds.  Run with -m gpu on an
MI355X.

Meshes: a x b x c hexes refined once carry 24abc + 4(ab + bc + ca) multipliers (every face of the fine mesh):
- 6 x 6 x 7: 6 528 = 102 x 64 - no row past the end;
- 5 x 6 x 9: 6 996 = 109 x 64 + 20 - the third row step of the last slice (8 rows at NB = 32) holds 4 rows and 4 past the
  end, the fourth and the pairs behind it lie wholly past the end;
- 5 x 7 x 9: 8 132 = 127 x 64 + 4 - the first row step is partly past the end, the second wholly, and so are the three pairs
  (and the one batch of four of the first update pass) behind them.
(The 5 x 4 x 3 box of test_gpu_fused_lanczos.py, refined twice, has 48 = six whole row steps.)  All three keep their finest
V-cycle level outside the LDS tail (3 x the rows of all levels exceed its 20 352 doubles from 6 784 rows on), which every
solve here asserts through pmc_fused_lanczos_solves() and the preconditioner tests through the setup export.

What is compared:
- the eager loop (fused Lanczos passes) against the hipGraph path (stored q, k::lincomb3) with np.array_equal on field and
  statistics, widths 1, 8, 32 and 64, max_iter 1, 2 and 3: one iteration runs only the pass without v0 (LZ = 3), two and three
  follow it with the pass that reads v0 (LZ = 2), so each form is once the first and once the last pass of a solve;
- one launch of 64 realizations against two launches of 32 with the same white noise, columns 0-31 and 32-63, bit for bit: the
  second column group reads its coefficients, parents and own rows at a column offset of 32 (the dots of a solve enter too:
  their per-block partials are added in the same order in both launch widths, see the test's docstring).  The same for
  pmc_sampler_apply_preconditioner on a random multi-vector (pre-smoothing: nothing added; post-smoothing: iterate and
  coarse correction added);
- pmc_sampler_apply_preconditioner of the default (fp32) storage against the fp64 reference oracle/precond_oracle.py on the
  two ragged sizes, bound REF_TOL of precond_cases.py (the bound of test_gpu_sampler_precond.py)."""
import numpy as np
import pytest

from precond_cases import REF_TOL, rel as _rel

pytestmark = pytest.mark.gpu

# coarse hexes (refined once) -> multipliers on the finest level, rows in the last slice
MESHES = {"full": ((6, 6, 7), 6528, 0), "rem20": ((5, 6, 9), 6996, 20), "rem4": ((5, 7, 9), 8132, 4)}
MODES = {"fused": dict(use_graph=0), "stored": dict(use_graph=1, check_every=2)}

_PROBLEMS = {}


def _problem(name):
    """the hybridized problem of a mesh (one Monte Carlo level), built once on the CPU"""
    if name not in _PROBLEMS:
        from parelagmc_amd.fe import box_mesh, build_hierarchy, build_hybrid_sampler_problem
        n, rows, rem = MESHES[name]
        prob = build_hybrid_sampler_problem(build_hierarchy(box_mesh(list(n), [2, 2, 2], "hex"), 1), corlen=0.1,
                                            n_mc_levels=1)
        assert prob.levels[0].n_lambda == rows and rows % 64 == rem
        _PROBLEMS[name] = prob
    return _PROBLEMS[name]


def _fused_solves(ctx):
    return ctx.lib.pmc_fused_lanczos_solves()


def _eval_counted(ctx, smp, xi):
    n0 = _fused_solves(ctx)
    r = smp.Eval(0, xi, xi_level=0, return_stats=True)
    return r, _fused_solves(ctx) - n0


def _same(a, b):
    (s1, st1), (s2, st2) = a, b
    assert np.array_equal(s1, s2)
    assert st1 == st2          # iterations, converged, initial and final norm of every realization, exactly


def test_the_sizes_are_what_the_docstring_says():
    assert [m[1] % 64 for m in MESHES.values()] == [0, 20, 4]
    assert MESHES["rem20"][2] % 8 != 0 and MESHES["rem4"][2] < 16


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_eager_loop_equals_graph_path(gpu_ctx, seeded_rng, mesh, max_iter):
    """rel_tol = 1e-14 is out of reach: every solve stops by max_iter"""
    from parelagmc_amd import capi
    prob = _problem(mesh)
    xi = seeded_rng.standard_normal((64, prob.levels[0].n_s))
    res = {}
    for mode in MODES:
        smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, rel_tol=1e-14, abs_tol=1e-300,
                                                              max_iter=max_iter, **MODES[mode]))
        assert smp.BatchWidth(0) >= 64
        res[mode] = [_eval_counted(gpu_ctx, smp, xi[:w]) for w in (1, 8, 32, 64)]
        smp.close()
    for (a, na), (b, nb) in zip(res["fused"], res["stored"]):
        _same(a, b)
        assert (na, nb) == (1, 0)
        assert all(t[0] == max_iter and t[1] == 0 for t in a[1])


@pytest.mark.parametrize("mesh", list(MESHES))
def test_one_launch_of_64_equals_two_of_32(gpu_ctx, seeded_rng, mesh):
    """five iterations each (a launch iterates until its last column has converged, so the three launches are given the same
    length: rel_tol = 1e-14 is out of reach); the statistics of a realization do not depend on its column either.

    Every dot of these solves is fused into a slice kernel, whose per-block partials do not depend on the number of column
    groups; the scalar kernels that add them deal a column's blocks over the same number of threads at 32 and at 64 columns
    (reduce_width), so the sums - initial norm, Lanczos coefficients, final norm - are the same bits.  Before that a launch
    of 32 added them over twice as many threads and the fields differed by 3.6e-15 after one iteration, 2.8e-11 after five."""
    from parelagmc_amd import capi
    prob = _problem(mesh)
    xi = seeded_rng.standard_normal((64, prob.levels[0].n_s))
    smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, use_graph=0, rel_tol=1e-14,
                                                          abs_tol=1e-300, max_iter=5))
    assert smp.BatchWidth(0) >= 64
    (s, st), n = _eval_counted(gpu_ctx, smp, xi)
    (s0, st0), n0 = _eval_counted(gpu_ctx, smp, xi[:32])
    (s1, st1), n1 = _eval_counted(gpu_ctx, smp, xi[32:])
    smp.close()
    assert (n, n0, n1) == (1, 1, 1)
    assert all(t[0] == 5 for t in st)
    assert np.array_equal(s[:32], s0) and np.array_equal(s[32:], s1)
    assert list(st[:32]) == list(st0) and list(st[32:]) == list(st1)


class _Precond:
    """a default-storage handle of a mesh with its setup export"""

    def __init__(self, ctx, mesh):
        from parelagmc_amd import capi
        self.prob = _problem(mesh)
        self.opts = capi.solver_opts()
        self.smp = capi.PDESampler(ctx, self.prob, self.opts)
        self.setup = self.smp.vcycle_setup(0)
        assert self.smp.BatchWidth(0) >= 64
        # wide launches smooth and descend on the finest level, on kernels: the epilogues under test
        assert int(self.setup[0]["role_wide"]) == 0 and int(self.setup[0]["tail_wide"]) == 0
        assert int(self.setup[0]["rows"]) == MESHES[mesh][1]


@pytest.mark.parametrize("mesh", list(MESHES))
def test_preconditioner_column_groups(gpu_ctx, seeded_rng, mesh):
    hd = _Precond(gpu_ctx, mesh)
    r = seeded_rng.standard_normal((64, MESHES[mesh][1]))
    z = hd.smp.ApplyPreconditioner(0, r)
    z0 = hd.smp.ApplyPreconditioner(0, r[:32])
    z1 = hd.smp.ApplyPreconditioner(0, r[32:])
    hd.smp.close()
    assert np.all(np.isfinite(z)) and np.all(np.linalg.norm(z, axis=1) > 0)
    assert np.array_equal(z[:32], z0) and np.array_equal(z[32:], z1)


@pytest.mark.parametrize("mesh", ["rem20", "rem4"])
def test_preconditioner_matches_fp64_reference_on_ragged_sizes(gpu_ctx, seeded_rng, mesh):
    """both ends of each column group of a launch of 64 and of a launch of 32 against the reference of the wide regime"""
    from oracle.precond_oracle import SamplerPrecondOracle
    hd = _Precond(gpu_ctx, mesh)
    P = [hd.smp.vcycle_prolongator(0, v) for v in range(len(hd.setup) - 1)]
    oracle = SamplerPrecondOracle(hd.prob, 0, hd.setup, P, hd.opts.schur_scale)
    assert 32 > int(hd.setup[0]["dense_nb"])
    r = seeded_rng.standard_normal((64, MESHES[mesh][1]))
    z64 = hd.smp.ApplyPreconditioner(0, r)
    z32 = hd.smp.ApplyPreconditioner(0, r[:32])
    hd.smp.close()
    worst = 0.0
    for j in (0, 31, 32, 63):
        ref = oracle.apply(r[j], False)
        errs = [_rel(z64[j], ref)] + ([_rel(z32[j], ref)] if j < 32 else [])
        worst = max(worst, *errs)
        print(f"reference {mesh} fp32 storage column {j}: rel L2 = {max(errs):.2e}")
        assert max(errs) <= REF_TOL["fp32"], (j, errs)
    print(f"reference {mesh} fp32 storage, launches of 64 and 32: max rel L2 = {worst:.2e}")

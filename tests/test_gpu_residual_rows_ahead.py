"""The residual kernels of the finest V-cycle level of the hybridized sampler at 32 columns per group (vc_residual_kernel: the
residual with the fused aggregate restriction, and res - (S P) xc in place) read the own rows of r AHEAD of their gather loop -
all eight row steps in the in-place form, four ahead and four behind the loop with the fused restriction - and the fused
restriction reads its slice's segment range and first (position, coarse row) pair ahead as well.  Rows past the end of the
last slice re-read the last row and store nothing, so the multiplier counts are chosen by what the last slice holds.  Run with
-m gpu on an MI355X.

Meshes (those of test_gpu_epilogue_batching.py): a x b x c hexes refined once carry 24abc + 4(ab + bc + ca) multipliers:
- 6 x 6 x 7: 6 528 = 102 x 64 - no row past the end;
- 5 x 6 x 9: 6 996 = 109 x 64 + 20 - the end of the matrix lies inside the third row step (8 rows each at NB = 32), i.e.
  inside the batch of four that is read ahead; the second batch lies wholly past the end;
- 5 x 7 x 9: 8 132 = 127 x 64 + 4 - the end lies inside the first row step.
All three keep their finest V-cycle level outside the LDS tail with the coarse correction folded into S P.  On the first two
the restriction is fused into the residual kernel; for the third agg_pack_rows finds no exact packing of the aggregates into
slices (nor for any other box below 10 000 rows whose last slice holds fewer than eight rows), so its level 0 runs the plain
residual - all eight row steps ahead - and the separate restriction.  Every case asserts through the setup exports
(pmc_sampler_vcycle_info) which of the two a mesh takes.

What is compared:
(a) pmc_sampler_apply_preconditioner on a seeded random multi-vector, one launch of 64 against two launches of 32 (columns
    0-31 and 32-63), bit for bit: the second column group reads its own rows and writes its coarse rows at a column offset;
(b) one launch of 32 against two launches of 16, bit for bit: the 16-wide instantiations keep the loads behind the gather
    loop and take the same route through the levels (16 > dense_nb), so this is the new code against the old code.  (The
    equality holds with the library of the commit before this change as well - checked on the MI355X - so it is a property
    of the cycle, not of this change);
(c) the default (fp32) storage against the fp64 reference oracle/precond_oracle.py on the two ragged sizes, bound REF_TOL of
    precond_cases.py;
(d) a full Eval of 64 realizations with max_iter 1, 2 and 3, eager loop against hipGraph path, np.array_equal on fields and
    statistics."""
import numpy as np
import pytest

from precond_cases import REF_TOL, rel as _rel

pytestmark = pytest.mark.gpu

# coarse hexes (refined once) -> multipliers on the finest level, rows in the last slice
MESHES = {"full": ((6, 6, 7), 6528, 0), "rem20": ((5, 6, 9), 6996, 20), "rem4": ((5, 7, 9), 8132, 4)}
# whether agg_pack_rows could renumber the finest level (every aggregate inside one slice), i.e. the restriction is fused
FUSED = {"full": 1, "rem20": 1, "rem4": 0}

_PROBLEMS = {}
_RHS = {}


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


def _rhs(name):
    """the multi-vector every preconditioner case of a mesh applies the cycle to (seeded, never written)"""
    if name not in _RHS:
        r = np.random.default_rng(20321 + MESHES[name][1]).standard_normal((64, MESHES[name][1]))
        r.setflags(write=False)
        _RHS[name] = r
    return _RHS[name]


class _Precond:
    """a default-storage handle of a mesh; level 0 of its cycle runs the kernels under test"""

    def __init__(self, ctx, mesh):
        from parelagmc_amd import capi
        self.prob = _problem(mesh)
        self.opts = capi.solver_opts()
        self.smp = capi.PDESampler(ctx, self.prob, self.opts)
        self.setup = self.smp.vcycle_setup(0)
        info = self.smp.vcycle_levels(0)
        assert self.smp.BatchWidth(0) >= 64
        # the finest level smooths and descends on kernels (not in the LDS tail), fp32 shared-value path: its restriction is
        # fused into the residual kernel (RAGG) and the coarse correction goes through S P (res - (S P) xc, in place)
        assert info[0]["rows"] == MESHES[mesh][1] and info[0]["in_tail"] == 0
        assert info[0]["fused_restriction"] == FUSED[mesh] and info[0]["sp_nnz"] > 0
        assert int(self.setup[0]["role_wide"]) == 0 and int(self.setup[0]["tail_wide"]) == 0
        assert int(self.setup[0]["rows"]) == MESHES[mesh][1]
        assert 16 > int(self.setup[0]["dense_nb"])       # launches of 16 and of 32 take the same route


def test_the_sizes_put_the_end_where_the_docstring_says():
    assert [m[1] % 64 for m in MESHES.values()] == [0, 20, 4]
    assert 16 < MESHES["rem20"][2] < 24 and MESHES["rem4"][2] < 8      # row steps of 8 rows at NB = 32


@pytest.mark.parametrize("mesh", list(MESHES))
def test_launch_of_64_equals_two_of_32(gpu_ctx, mesh):
    hd = _Precond(gpu_ctx, mesh)
    r = _rhs(mesh)
    z = hd.smp.ApplyPreconditioner(0, r)
    z0 = hd.smp.ApplyPreconditioner(0, r[:32])
    z1 = hd.smp.ApplyPreconditioner(0, r[32:])
    hd.smp.close()
    assert np.all(np.isfinite(z)) and np.all(np.linalg.norm(z, axis=1) > 0)
    assert np.array_equal(z[:32], z0) and np.array_equal(z[32:], z1)


@pytest.mark.parametrize("mesh", list(MESHES))
def test_launch_of_32_equals_two_of_16(gpu_ctx, mesh):
    """rows read ahead (32 wide) against rows read behind the gather loop (16 wide)"""
    hd = _Precond(gpu_ctx, mesh)
    r = _rhs(mesh)[:32]
    z = hd.smp.ApplyPreconditioner(0, r)
    z0 = hd.smp.ApplyPreconditioner(0, r[:16])
    z1 = hd.smp.ApplyPreconditioner(0, r[16:])
    hd.smp.close()
    assert np.all(np.isfinite(z)) and np.all(np.linalg.norm(z, axis=1) > 0)
    print(f"32 against 2 x 16, {mesh}: max |diff| = {max(np.max(np.abs(z[:16] - z0)), np.max(np.abs(z[16:] - z1))):.3e}")
    assert np.array_equal(z[:16], z0) and np.array_equal(z[16:], z1)


@pytest.mark.parametrize("mesh", ["rem20", "rem4"])
def test_matches_fp64_reference_on_ragged_sizes(gpu_ctx, mesh):
    """both ends of each column group of a launch of 64 against the reference of the wide regime"""
    from oracle.precond_oracle import SamplerPrecondOracle
    hd = _Precond(gpu_ctx, mesh)
    P = [hd.smp.vcycle_prolongator(0, v) for v in range(len(hd.setup) - 1)]
    oracle = SamplerPrecondOracle(hd.prob, 0, hd.setup, P, hd.opts.schur_scale)
    r = _rhs(mesh)
    z64 = hd.smp.ApplyPreconditioner(0, r)
    hd.smp.close()
    for j in (0, 31, 32, 63):
        err = _rel(z64[j], oracle.apply(np.array(r[j]), False))
        print(f"reference {mesh} fp32 storage column {j}: rel L2 = {err:.2e}")
        assert err <= REF_TOL["fp32"], (j, err)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_eval_of_64_eager_equals_graph(gpu_ctx, seeded_rng, mesh, max_iter):
    """rel_tol = 1e-14 is out of reach: every solve stops by max_iter; the eager loop counts one fused-Lanczos solve, the
    graph path none"""
    from parelagmc_amd import capi
    prob = _problem(mesh)
    xi = seeded_rng.standard_normal((64, prob.levels[0].n_s))
    res = []
    for use_graph in (0, 1):
        extra = dict(check_every=2) if use_graph else {}
        smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(mini_max_rows=0, two_streams=2, rel_tol=1e-14, abs_tol=1e-300,
                                                              max_iter=max_iter, use_graph=use_graph, **extra))
        assert smp.BatchWidth(0) >= 64
        n0 = gpu_ctx.lib.pmc_fused_lanczos_solves()
        out = smp.Eval(0, xi, xi_level=0, return_stats=True)
        res.append((out, gpu_ctx.lib.pmc_fused_lanczos_solves() - n0))
        smp.close()
    ((s0, st0), n_eager), ((s1, st1), n_graph) = res
    assert (n_eager, n_graph) == (1, 0)
    assert np.array_equal(s0, s1)
    assert st0 == st1          # iterations, converged, initial and final norm of every realization, exactly
    assert all(t[0] == max_iter and t[1] == 0 for t in st0)

"""The vectors BETWEEN the levels of the multiplier / Schur V-cycle (coarse right-hand side, coarse correction) are fp32 with
the default preconditioner storage (Multigrid::inner_f32, LAB_NOTES 2c and 10.24), fp64 with PMC_STORAGE_FP64.  They live only
inside one application of the preconditioner, so - like the fp32 iterates and residuals of a level - they may perturb the
preconditioner by fp32 rounding and nothing else:

  * cube_tet r = 3 and r = 4, hybridized (aggregation hierarchy, fused aggregate restriction on the finest level, separate
    restriction below it) and saddle-point (octree hierarchy, restriction over groups of 8 rows): the fields of the default
    storage equal those of PMC_STORAGE_FP64 to 1e-9 when both solve to rel 1e-12 - the bound the storage tests use
    (tests/test_gpu_round4.py, tests/test_gpu_hybrid.py) - and at the default tolerance every realization needs the same
    number of iterations in both storages;
  * launches of 1, 8 and 64 realizations (the row-split kernels, the dense inverse and the late LDS tail of narrow launches;
    one and two column groups) return the members of a full launch to the same 1e-9."""
import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-300, max_iter=300)
BOUND = 1e-9


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def _problem(nref, solver):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_hierarchy, build_hybrid_sampler_problem, build_sampler_problem, mesh_from_json
    h = build_hierarchy(mesh_from_json(golden_path("meshes", "cube_tet.json")), nref)
    kw = dict(corlen=0.1, n_mc_levels=1)
    if solver == "hybridization":
        return build_hybrid_sampler_problem(h, builder=capi.library_hybrid_builder, **kw)
    return build_sampler_problem(h, **kw)


@pytest.mark.parametrize("solver", ["hybridization", "saddle-point"])
@pytest.mark.parametrize("nref", [3, 4])
def test_default_storage_against_fp64_storage(gpu_ctx, nref, solver):
    from parelagmc_amd import capi
    prob = _problem(nref, solver)
    fields, its = {}, {}
    xi = None
    for storage in (capi.PMC_STORAGE_FP32, capi.PMC_STORAGE_FP64):
        tight = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(precond_storage=storage, **TIGHT))
        assert tight.z_bytes() == (4 if storage == capi.PMC_STORAGE_FP32 else 8)
        if xi is None:
            xi = tight.Sample(0, first_id=31 + nref, nbatch=tight.BatchWidth(0))
        s, st = tight.Eval(0, xi, return_stats=True)
        assert all(t[1] == 1 for t in st), [t for t in st if t[1] != 1][:4]
        fields[storage] = s
        tight.close()
        dflt = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(precond_storage=storage))
        _, st = dflt.Eval(0, xi, return_stats=True)
        assert all(t[1] == 1 for t in st)
        its[storage] = [t[0] for t in st]
        dflt.close()
    a, b = fields[capi.PMC_STORAGE_FP32], fields[capi.PMC_STORAGE_FP64]
    err = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    print(f"cube_tet r={nref} {solver}: {len(err)} realizations, worst column fp32 against fp64 storage {err.max():.2e}, "
          f"iterations at the default tolerance {sorted(set(its[capi.PMC_STORAGE_FP32]))}")
    assert err.max() < BOUND, (err.max(), int(err.argmax()))
    assert its[capi.PMC_STORAGE_FP32] == its[capi.PMC_STORAGE_FP64]


@pytest.mark.parametrize("solver", ["hybridization", "saddle-point"])
@pytest.mark.parametrize("nref", [3, 4])
def test_narrow_launches_return_the_members_of_a_full_launch(gpu_ctx, nref, solver):
    from parelagmc_amd import capi
    prob = _problem(nref, solver)
    smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(**TIGHT))
    w = smp.BatchWidth(0)
    assert w >= 64
    xi = smp.Sample(0, first_id=57 + nref, nbatch=w)
    full, st = smp.Eval(0, xi, return_stats=True)
    assert all(t[1] == 1 for t in st)
    worst = {}
    for m in (1, 8, 64):
        part = smp.Eval(0, xi[w - m:])                     # the LAST members: not the columns a narrow launch would pick first
        err = np.linalg.norm(part - full[w - m:], axis=1) / np.linalg.norm(full[w - m:], axis=1)
        worst[m] = float(err.max())
    print(f"cube_tet r={nref} {solver}: full launch of {w}; worst column of a launch of m against it {worst}")
    smp.close()
    assert max(worst.values()) < BOUND, worst

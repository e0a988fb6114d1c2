"""Conditioning on observed field values on the device (csrc/condition.hip, pmc_conditioner_*) against its numpy twin
(parelagmc_amd/fe/condition.py): setup, apply, the Eval hook, the layers above it, refusals and the C caller."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

CORLEN = 0.5
NBATCH = (1, 3, 4, 5, 16, 17, 64, 130, 257)     # VALU path, one tile, a ragged last tile, more than one workgroup column


def _opts():
    from parelagmc_amd import capi
    return capi.solver_opts(rel_tol=1e-12, max_iter=1000)


@pytest.fixture(scope="module")
def ragged_hierarchy():
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    return build_hierarchy(box_mesh([5, 3, 2], [2, 2, 2], "hex"), 1)     # n_s = 240 / 30; 240 is no multiple of 64


def _observations(h, nobs, seed, averaging=False):
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    elems = pick_observation_elements(h, nobs, seed)
    extra = []
    if averaging:     # the last row: the mean over the fine elements that share its level-1 parent
        parent = sp.csr_matrix(h.P[0]).indices
        sib = np.nonzero(parent == parent[elems[-1]])[0]
        extra = [(sib, np.full(sib.size, 1.0 / sib.size))]
        elems = elems[:-1]
    H0 = point_observations(h.spaces[0].n_s, elems, extra)
    y = np.random.default_rng(seed + 100).normal(0.0, 1.0, H0.shape[0])
    return H0, y


def _problem(kind, h, lognormal=False):
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_kl_sampler_problem, build_sampler_problem
    if kind == "saddle":
        return build_sampler_problem(h, corlen=CORLEN, lognormal=lognormal)
    if kind == "hybrid":
        return build_hybrid_sampler_problem(h, corlen=CORLEN, lognormal=lognormal)
    return build_kl_sampler_problem(h, "analytic", corlen=CORLEN, lognormal=lognormal, n_mc_levels=h.nlevels)


def _sampler(ctx, kind, prob):
    from parelagmc_amd import capi
    return capi.KLSampler(ctx, prob) if kind == "kl" else capi.PDESampler(ctx, prob, _opts())


@pytest.fixture(scope="module")
def hybrid_handles(gpu_ctx, hex_hierarchy, ragged_hierarchy):
    """Gaussian hybridized handles on the two meshes, shared by the apply tests"""
    out = {}
    for name, h in (("hex", hex_hierarchy), ("ragged", ragged_hierarchy)):
        prob = _problem("hybrid", h)
        out[name] = (h, prob, _sampler(gpu_ctx, "hybrid", prob))
    yield out
    for _, _, smp in out.values():
        smp.close()


def _rel_cols(a, b):
    """relative L2 distance per column (realization / observation)"""
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.mark.parametrize("kind,nobs,noise", [("saddle", 16, False), ("hybrid", 33, False), ("hybrid", 5, True),
                                             ("kl", 5, False), ("kl", 16, True)])
def test_setup_matches_the_twin(gpu_ctx, hex_hierarchy, kind, nobs, noise):
    """K_l and A_l of every level: 1e-8 relative per column for the handles that solve (two chained solves at the project's
    1e-9-at-1e-12 field tolerance, plus margin), 1e-12 for the KL handle, which multiplies its modes"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.condition import Conditioner
    prob = _problem(kind, hex_hierarchy)
    H0, y = _observations(hex_hierarchy, nobs, seed=nobs, averaging=(nobs == 5))
    sigma2 = np.random.default_rng(5).uniform(0.01, 0.2, nobs) if noise else None
    twin = Conditioner(prob, H0, y, sigma2)
    smp = _sampler(gpu_ctx, kind, prob)
    cond = capi.Conditioner(smp, H0, y, sigma2)
    tol = 1e-12 if kind == "kl" else 1e-8
    for lvl in range(prob.n_mc_levels):
        K, A, H = cond.level(lvl)
        assert (abs(H - twin.H[lvl])).max() <= 1e-15
        eK, eA = _rel_cols(K.T, twin.K[lvl].T).max(), _rel_cols(A.T, twin.A[lvl].T).max()
        print(f"[{kind} nobs {nobs} noise {noise}] level {lvl}: K {eK:.2e} A {eA:.2e} cond(A) {np.linalg.cond(A):.2e}")
        assert eK <= tol and eA <= tol
        assert np.array_equal(A, A.T)
    cond.close()
    smp.close()


APPLY_CASES = [("hex", n, z) for n in (1, 5, 16, 33, 64) for z in (False, True)] + \
              [("ragged", n, z) for n in (1, 5, 30) for z in (False, True)]


@pytest.mark.parametrize("mesh,nobs,noise", APPLY_CASES)
def test_apply_matches_the_twin_on_the_exported_setup(gpu_ctx, hybrid_handles, mesh, nobs, noise):
    """device apply against the twin's affine map fed the device's own K, A: 1e-12 relative L2 per realization, for every
    launch shape, host and device memory, exp on and off, in place, and bitwise repeatable"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.condition import apply_affine
    h, prob, smp = hybrid_handles[mesh]
    H0, y = _observations(h, nobs, seed=nobs, averaging=(nobs == 5))
    sigma2 = np.random.default_rng(5).uniform(0.01, 0.2, nobs) if noise else None
    if noise and nobs > 1:
        sigma2[0] = 0.0      # a mix of exact and noisy rows
    cond = capi.Conditioner(smp, H0, y, sigma2)
    rng = np.random.default_rng(1000 + nobs)
    worst = 0.0
    for lvl in range(prob.n_mc_levels):
        K, A, H = cond.level(lvl)
        n = K.shape[0]
        for nb in NBATCH:
            g = rng.standard_normal((nb, n))
            zeta = rng.standard_normal((nb, nobs)) if noise else None
            ref = apply_affine(K, A, H, y, sigma2, g, zeta)
            out = cond.apply(lvl, g, zeta)
            err = _rel_cols(out, ref).max()
            worst = max(worst, err)
            assert err <= 1e-12, (lvl, nb, err)
            assert np.array_equal(out, cond.apply(lvl, g, zeta)), "two identical calls differ"
            if nb in (3, 17, 130):
                oe = cond.apply(lvl, g, zeta, exp=True)
                assert _rel_cols(oe, np.exp(ref)).max() <= 1e-12
                # device memory, out aliasing g
                gd = gpu_ctx.array(g)
                zd = gpu_ctx.array(zeta) if noise else None
                cond.apply(lvl, gd, zd)
                assert np.array_equal(gd.download().reshape(nb, n), out), "device / in-place result differs from the host call"
                gd.upload(g)
                cond.apply(lvl, gd, zd, exp=True)
                assert np.array_equal(gd.download().reshape(nb, n), oe)
                gd.free()
                if zd is not None:
                    zd.free()
                inplace = g.copy()
                cond.apply(lvl, inplace, zeta, out=inplace)
                assert np.array_equal(inplace, out)
        if not noise:     # exact data are honoured
            gc = cond.apply(lvl, rng.standard_normal((5, n)))
            assert np.max(np.abs((H @ gc.T).T - y[None, :])) <= 1e-9
    print(f"[{mesh} nobs {nobs} noise {noise}] worst relative L2 {worst:.2e}")
    cond.close()


@pytest.mark.parametrize("kind", ["saddle", "hybrid"])
def test_eval_hook(gpu_ctx, hex_hierarchy, kind):
    """Sample + Eval on a lognormal handle with a conditioner attached: the data are honoured, s = exp(affine map of the
    prior field embed_s_out) with the device's exported K, A, embed_s_out is bitwise the prior field, and detaching restores
    Eval bit for bit"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe.condition import apply_affine
    prob = _problem(kind, hex_hierarchy, lognormal=True)
    smp = _sampler(gpu_ctx, kind, prob)
    nobs = 16
    H0, y = _observations(hex_hierarchy, nobs, seed=nobs, averaging=True)
    cond = capi.Conditioner(smp, H0, y)
    for lvl in (1, 2):
        K, A, H = cond.level(lvl)
        for xi_level in (lvl, lvl - 1):
            xi = smp.Sample(xi_level, first_id=40, nbatch=6)
            s0, e0 = smp.Eval(lvl, xi, xi_level=xi_level, want_embed=True)
            smp.SetConditioner(cond)
            s1, e1 = smp.Eval(lvl, xi, xi_level=xi_level, want_embed=True)
            smp.SetConditioner(None)
            s2, e2 = smp.Eval(lvl, xi, xi_level=xi_level, want_embed=True)
            assert np.array_equal(e1, e0), "embed_s_out is not the prior field"
            assert np.array_equal(s2, s0) and np.array_equal(e2, e0), "Eval changed after detaching"
            miss = np.max(np.abs((H @ np.log(s1).T).T - y[None, :]))
            err = _rel_cols(s1, apply_affine(K, A, H, y, None, e1, exp=True)).max()
            print(f"[{kind}] level {lvl} xi_level {xi_level}: |H log s - y| {miss:.2e}, s vs twin {err:.2e}")
            assert miss <= 1e-9
            assert err <= 1e-12
    cond.close()
    smp.close()


def test_field_statistics_and_mlmc_over_a_conditioned_sampler(gpu_ctx, hex_hierarchy):
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_darcy_problem
    prob = _problem("hybrid", hex_hierarchy)
    smp = _sampler(gpu_ctx, "hybrid", prob)
    H0, y = _observations(hex_hierarchy, 16, seed=16)
    cond = capi.Conditioner(smp, H0, y)
    smp.SetConditioner(cond)
    fs = capi.FieldStatistics(smp, 0).run(0, 256)
    e, m2, _, N = fs.read()
    fs.close()
    obs = H0.indices
    var = m2 - e * e
    assert N == 256
    print(f"at the data: |E - y| {np.max(np.abs(e[obs] - y)):.2e}, |var| {np.max(np.abs(var[obs])):.2e}")
    assert np.max(np.abs(e[obs] - y)) <= 1e-9
    assert np.max(np.abs(var[obs])) <= 1e-8
    rest = np.setdiff1d(np.arange(e.size), obs)
    assert np.all(var[rest] > 0.0)
    smp.close()
    # MLMC over a conditioned lognormal sampler and the Darcy handle
    lprob = _problem("hybrid", hex_hierarchy, lognormal=True)
    dp = build_darcy_problem(hex_hierarchy, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
    smp = _sampler(gpu_ctx, "hybrid", lprob)
    ds = capi.DarcySolver(gpu_ctx, dp, _opts())
    runs = []
    for attach in (False, True):
        if attach:
            cond = capi.Conditioner(smp, H0, 0.3 * y)
            smp.SetConditioner(cond)
        mgr = host_api.MLMCManager(3, sampler=smp, solver=ds, wall_time=False)
        runs.append(mgr.InitRun([8, 8, 8]))
        mgr.close()
    assert all(list(r["nsamples"]) == [8, 8, 8] and np.all(np.isfinite(r["sums"])) for r in runs)
    assert not np.allclose(runs[0]["sums"], runs[1]["sums"], rtol=1e-6, atol=0.0)
    ds.close()
    smp.close()


def test_refusals(gpu_ctx, hex_hierarchy, hex_hierarchy_small):
    """every refusal returns PMC_ERR_INVALID with a message and leaves the handle usable"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    from parelagmc_amd.fe.condition import point_observations
    prob = _problem("hybrid", hex_hierarchy)
    smp = _sampler(gpu_ctx, "hybrid", prob)
    n0 = prob.levels[0].n_s
    H0, y = _observations(hex_hierarchy, 5, seed=5)
    xi = smp.Sample(2, first_id=3, nbatch=2)
    before = smp.Eval(2, xi, xi_level=2)

    def refused(fn, match=None):
        with pytest.raises(capi.PmcError) as ei:
            fn()
        assert ei.value.code == -1 and len(gpu_ctx.lib.pmc_last_error()) > 0, str(ei.value)
        if match:
            assert match in str(ei.value), str(ei.value)
        assert np.array_equal(smp.Eval(2, xi, xi_level=2), before)

    big = point_observations(n0, np.arange(513))
    refused(lambda: capi.Conditioner(smp, big, np.zeros(513)))                          # nobs > 512
    refused(lambda: capi.Conditioner(smp, sp.csr_matrix((0, n0)), np.zeros(0)))         # nobs < 1
    empty = sp.csr_matrix(H0.copy())
    empty.data[2] = 0.0
    empty.eliminate_zeros()
    refused(lambda: capi.Conditioner(smp, empty, y))                                    # an empty row
    refused(lambda: capi.Conditioner(smp, sp.csr_matrix(H0[:, :n0 - 1]), y))            # wrong column count
    bad = y.copy()
    bad[1] = np.inf
    refused(lambda: capi.Conditioner(smp, H0, bad))                                     # non-finite y
    refused(lambda: capi.Conditioner(smp, H0, y, [0.1, np.nan, 0.1, 0.1, 0.1]))         # non-finite sigma2
    refused(lambda: capi.Conditioner(smp, H0, y, [0.1, -0.1, 0.1, 0.1, 0.1]))           # negative sigma2
    parent = sp.csr_matrix(hex_hierarchy.P[0]).indices
    grand = sp.csr_matrix(hex_hierarchy.P[1]).indices[parent]
    e1 = int(np.nonzero((grand == grand[0]) & (parent != parent[0]))[0][0])
    dup = point_observations(n0, [0, e1, 4000])
    refused(lambda: capi.Conditioner(smp, dup, [0.3, -0.2, 0.1]), match="level 2")      # A of level 2 singular
    noisy = capi.Conditioner(smp, dup, [0.3, -0.2, 0.1], [0.05, 0.05, 0.05])            # ... accepted with noise
    g = np.zeros((2, n0))
    refused(lambda: noisy.apply(0, g))                                                  # zeta missing
    refused(lambda: smp.SetConditioner(noisy))                                          # noise inside the Eval hook
    noisy.apply(0, g, np.zeros((2, 3)))
    # a conditioner of another handle
    other = _sampler(gpu_ctx, "hybrid", prob)
    theirs = capi.Conditioner(other, H0, y)
    refused(lambda: smp.SetConditioner(theirs))
    theirs.close()
    other.close()
    # projections: refused at create on a handle that has one, and on a handle with a conditioner attached
    sprob = build_sampler_problem(hex_hierarchy_small, corlen=CORLEN, embedded=True)
    emb = capi.PDESampler(gpu_ctx, sprob, _opts(), projection="gather")
    Hs = point_observations(sprob.levels[0].n_s, [1, 300])
    with pytest.raises(capi.PmcError) as ei:
        capi.Conditioner(emb, Hs, [0.0, 0.1])
    assert ei.value.code == -1 and "projection" in str(ei.value)
    emb.close()
    mine = capi.Conditioner(smp, H0, y)
    smp.SetConditioner(mine)
    idx = np.arange(8, dtype=np.int32)
    rc = gpu_ctx.lib.pmc_sampler_set_projection(smp.h, 2, capi.PMC_PROJ_GATHER, None,
                                                idx.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)), None, 8)
    assert rc == -1 and len(gpu_ctx.lib.pmc_last_error()) > 0
    cs = smp.Eval(2, xi, xi_level=2)
    assert np.max(np.abs((mine.level(2)[2] @ cs.T).T - y[None, :])) <= 1e-9            # still attached and working
    mine.close()                                                                        # destroy detaches
    assert np.array_equal(smp.Eval(2, xi, xi_level=2), before)
    noisy.close()
    smp.close()


def _write_problem(path, prob):
    """tests/c/kl_io.h layout with no realizations (nbatch 0)"""
    with open(path, "wb") as f:
        np.array([0x4b4c3031, len(prob.levels), prob.nmodes, 1 if prob.lognormal else 0, 0], np.int32).tofile(f)
        for L in prob.levels:
            np.array([L.n_s], np.int32).tofile(f)
            L.w_diag.astype(np.float64).tofile(f)
            np.array([0 if L.P is None else 1], np.int32).tofile(f)
            if L.P is not None:
                P = sp.csr_matrix(L.P)
                np.array([P.shape[0], P.shape[1], P.nnz], np.int32).tofile(f)
                P.indptr.astype(np.int32).tofile(f)
                P.indices.astype(np.int32).tofile(f)
                P.data.astype(np.float64).tofile(f)
        prob.evals.astype(np.float64).tofile(f)
        np.asfortranarray(prob.evect0).ravel(order="F").astype(np.float64).tofile(f)


def test_c_caller(hex_hierarchy, tmp_path):
    """tests/c/condition_smoke.c (plain C, include/pmc.h only) builds with -Wall -Wextra -Werror and passes"""
    import os
    import subprocess
    from conftest import ROOT
    r = subprocess.run(["make", "-C", ROOT, "test-condition"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    prob = _problem("kl", hex_hierarchy, lognormal=True)
    path = str(tmp_path / "kl.bin")
    _write_problem(path, prob)
    H0, y = _observations(hex_hierarchy, 5, seed=5)
    args = [a for e, v in zip(H0.indices, y) for a in (str(int(e)), repr(float(v)))]
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "condition_smoke"), path, "11"] + args, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("condition_smoke OK"), r.stdout + r.stderr

"""KL sampler on the device (pmc_sampler_create_kl, csrc/kl.hip) against numpy restatements of KLSampler::Eval
(/root/reference/src/KLSampler.cpp:199-223): s = Phi_level Lambda^1/2 xi[:m], exp() if lognormal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
WIDTHS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]


def _problems():
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_kl_sampler_problem, kuhn_cube_tet
    hex_h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 2)      # the conftest hex_hierarchy
    quad_h = build_hierarchy(box_mesh([12, 10], [1.2, 1.0], "quad"), 1)
    tet_h = build_hierarchy(kuhn_cube_tet(), 2)
    return {
        "hex_analytic": lambda logn: build_kl_sampler_problem(hex_h, "analytic", corlen=0.1, lognormal=logn),
        "hex_matern": lambda logn: build_kl_sampler_problem(hex_h, "matern", nmodes=37, corlen=0.1, lognormal=logn),
        "quad_analytic": lambda logn: build_kl_sampler_problem(quad_h, "analytic", nmodes=[5, 3], corlen=0.2, lognormal=logn),
        "tet_matern": lambda logn: build_kl_sampler_problem(tet_h, "matern", nmodes=20, corlen=0.3, lognormal=logn),
    }


def _gauss_ref(prob, level, xi):
    """numpy Phi_l Lambda^1/2 xi[:m] and the per-entry bound 8 m eps sum_k |Phi_ik sqrt(lambda_k) xi_k|"""
    m = prob.nmodes
    z = xi[:, :m] * np.sqrt(prob.evals)[None, :]
    phi = prob.evects[level]
    return z @ phi.T, 8.0 * m * EPS * (np.abs(z) @ np.abs(phi).T)


@pytest.mark.parametrize("memspace", ["host", "device"])
@pytest.mark.parametrize("lognormal", [False, True])
@pytest.mark.parametrize("name", ["hex_analytic", "hex_matern", "quad_analytic", "tet_matern"])
def test_eval_matches_the_expansion(gpu_ctx, name, lognormal, memspace):
    from parelagmc_amd import capi
    prob = _problems()[name](lognormal)
    smp = capi.KLSampler(gpu_ctx, prob)
    rng = np.random.default_rng(11)
    try:
        assert smp.is_kl()
        for level in range(prob.n_mc_levels):
            n = prob.levels[level].n_s
            for xi_level in range(level + 1):
                for nb in WIDTHS:
                    if xi_level < level and nb not in (1, 5, 64, 257):
                        continue
                    xi = rng.standard_normal((nb, prob.levels[xi_level].n_s))
                    g, bound = _gauss_ref(prob, level, xi)
                    if memspace == "host":
                        s, emb = smp.Eval(level, xi, xi_level=xi_level, want_embed=True)
                    else:
                        dxi, ds, de = gpu_ctx.array(xi), gpu_ctx.empty(nb * n), gpu_ctx.empty(nb * n)
                        smp.Eval(level, dxi, xi_level=xi_level, s_out=ds, embed_out=de)
                        s, emb = ds.download().reshape(nb, n), de.download().reshape(nb, n)
                        for a in (dxi, ds, de):
                            a.free()
                    what = f"{name} level {level} xi_level {xi_level} nb {nb}"
                    assert np.all(np.abs(emb - g) <= bound), what
                    if lognormal:
                        assert np.all(np.abs(s - np.exp(emb)) <= 2 * EPS * np.abs(s)), what
                    else:
                        assert np.array_equal(s, emb), what
    finally:
        smp.close()


def test_device_projection_matches_the_host_projection(gpu_ctx):
    """Eval on unit xi returns the columns of Phi_l sqrt(lambda) as projected on the device at create"""
    from parelagmc_amd import capi
    for name in ("hex_analytic", "hex_matern", "tet_matern"):
        prob = _problems()[name](False)
        smp = capi.KLSampler(gpu_ctx, prob)
        m = prob.nmodes
        for level in range(prob.n_mc_levels):
            xi = np.zeros((m, prob.levels[0].n_s))
            xi[np.arange(m), np.arange(m)] = 1.0
            s = smp.Eval(level, xi, xi_level=0)
            ref = (prob.evects[level] * np.sqrt(prob.evals)[None, :]).T
            assert np.abs(s - ref).max() <= 1e-13 * np.abs(ref).max(), (name, level)
        smp.close()


def test_mfma_operand_maps_with_exact_integer_data(gpu_ctx):
    """small integers in Phi and xi: every product and sum is exact in fp64, so any lane-map error shows as a wrong entry"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import KLLevel, KLProblem
    rng = np.random.default_rng(3)
    n, m = 83, 45
    phi = rng.integers(-4, 5, size=(n, m)).astype(np.float64)
    phi[np.arange(m), np.arange(m)] += np.arange(1, m + 1)       # asymmetric, no two columns alike
    prob = KLProblem([KLLevel(n, np.ones(n), None)], 1, np.ones(m), phi, False, "integers", [phi])
    smp = capi.KLSampler(gpu_ctx, prob)
    for nb in (1, 4, 5, 17, 100, 300):
        xi = rng.integers(-3, 4, size=(nb, n)).astype(np.float64)
        assert np.array_equal(smp.Eval(0, xi), xi[:, :m] @ phi.T), nb
    smp.close()


def test_sizes_true_p_and_the_handle_kind(gpu_ctx, hex_hierarchy):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    prob = _problems()["hex_analytic"](False)
    smp = capi.KLSampler(gpu_ctx, prob)
    lib = gpu_ctx.lib
    assert lib.pmc_sampler_num_levels(smp.h) == 3
    for level in range(3):
        n = hex_hierarchy.spaces[level].n_s
        assert smp.xi_size(level) == n and smp.SampleSize(level) == n and smp.GetNNZ(level) == 0
        assert smp.BatchWidth(level) >= 1
        if level < 2:
            assert abs(smp.GetTrueP(level) - hex_hierarchy.P[level]).max() == 0
        xi = smp.Sample(level, first_id=3, nbatch=4)
        assert xi.shape == (4, n) and abs(xi.mean()) < 0.2
    assert lib.pmc_sampler_is_kl(smp.h) == 1 and lib.pmc_sampler_is_hybrid(smp.h) == 0
    assert lib.pmc_sampler_is_kl(None) == -1
    s, emb, st = smp.Eval(1, smp.Sample(0, nbatch=3), xi_level=0, want_embed=True, return_stats=True)
    assert [t[:2] for t in st] == [(0, 1)] * 3
    pde = capi.PDESampler(gpu_ctx, build_sampler_problem(hex_hierarchy, corlen=0.1))
    assert lib.pmc_sampler_is_kl(pde.h) == 0
    pde.close()
    smp.close()


def test_entry_points_without_a_linear_system_are_refused(gpu_ctx):
    from parelagmc_amd import capi
    prob = _problems()["quad_analytic"](False)
    smp = capi.KLSampler(gpu_ctx, prob)
    lib = gpu_ctx.lib
    n = prob.levels[0].n_s
    x = np.zeros(2 * n)
    y = np.zeros(2 * n)
    nv = C.c_int(0)
    info = (C.c_int64 * 7)()
    dinfo = (C.c_double * 15)()
    nc, nnz = C.c_int(0), C.c_int64(0)
    t, b = C.c_double(), C.c_double()
    calls = {
        "pmc_sampler_mult": lambda: lib.pmc_sampler_mult(smp.h, 0, 1, x.ctypes.data, y.ctypes.data, 0, 0, None),
        "pmc_sampler_apply_preconditioner": lambda: lib.pmc_sampler_apply_preconditioner(smp.h, 0, 1, x.ctypes.data,
                                                                                         y.ctypes.data, 0),
        "pmc_sampler_apply_operator": lambda: lib.pmc_sampler_apply_operator(smp.h, 0, 1, x.ctypes.data, y.ctypes.data, 0, 1,
                                                                             C.byref(t), C.byref(b)),
        "pmc_sampler_vcycle_info": lambda: lib.pmc_sampler_vcycle_info(smp.h, 0, 0, C.byref(nv), info),
        "pmc_sampler_vcycle_level": lambda: lib.pmc_sampler_vcycle_level(smp.h, 0, 0, C.byref(nv), dinfo),
        "pmc_sampler_vcycle_prolongator": lambda: lib.pmc_sampler_vcycle_prolongator(smp.h, 0, 0, C.byref(nv), C.byref(nc),
                                                                                     C.byref(nnz), None, None, None),
        "pmc_sampler_set_projection": lambda: lib.pmc_sampler_set_projection(smp.h, 0, capi.PMC_PROJ_GATHER, None,
                                                                             np.arange(n, dtype=np.int32).ctypes.data_as(
                                                                                 C.POINTER(C.c_int32)), None, n),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.pmc_last_error().decode()
        assert name in msg and "KL" in msg, msg
    smp.close()


def _create(ctx, prob, nmodes=None, evals=None, evect0=None, levels=None, nlevels=None, w_null=False):
    from parelagmc_amd import capi
    keep = capi._Keep()
    lv = prob.levels if levels is None else levels
    arr = (capi.pmc_kl_level * len(lv))()
    for i, L in enumerate(lv):
        arr[i] = capi.pmc_kl_level(L.n_s, None if w_null else keep.f64(L.w_diag), keep.csr(L.P))
    ev = prob.evals if evals is None else evals
    phi = np.asfortranarray(prob.evect0 if evect0 is None else evect0)
    h = C.c_void_p()
    rc = ctx.lib.pmc_sampler_create_kl(ctx.h, len(lv) if nlevels is None else nlevels, arr,
                                       prob.nmodes if ev is False else (ev.size if nmodes is None else nmodes),
                                       None if ev is False else keep.f64(ev),
                                       None if evect0 is False else phi.ravel(order="K").ctypes.data_as(C.POINTER(C.c_double)),
                                       0, C.byref(h))
    if rc == 0:
        ctx.lib.pmc_sampler_destroy(h)
    return rc, ctx.lib.pmc_last_error().decode()


def test_create_refuses_bad_arguments(gpu_ctx):
    from parelagmc_amd.fe import KLLevel
    prob = _problems()["hex_analytic"](False)
    m = prob.nmodes
    assert _create(gpu_ctx, prob)[0] == 0
    # nmodes > n_s of a level (64 modes, a 4^3 level: one mode more than the last level has elements)
    wide = np.concatenate([prob.evect0, prob.evect0[:, :1]], axis=1)
    rc, msg = _create(gpu_ctx, prob, evals=np.append(prob.evals, 0.001), evect0=wide)
    assert rc == -1 and "nmodes exceeds" in msg
    bad = prob.evals.copy()
    bad[5] = -1e-3
    assert _create(gpu_ctx, prob, evals=bad)[0] == -1
    bad[5] = np.nan
    assert _create(gpu_ctx, prob, evals=bad)[0] == -1
    bad[5] = np.inf
    assert _create(gpu_ctx, prob, evals=bad)[0] == -1
    assert _create(gpu_ctx, prob, evals=False)[0] == -1
    assert _create(gpu_ctx, prob, evect0=False)[0] == -1
    assert _create(gpu_ctx, prob, w_null=True)[0] == -1
    assert _create(gpu_ctx, prob, nmodes=0)[0] == -1
    assert _create(gpu_ctx, prob, nlevels=0)[0] == -1
    assert gpu_ctx.lib.pmc_sampler_create_kl(gpu_ctx.h, 1, None, m, None, None, 0, C.byref(C.c_void_p())) == -1
    # P^T W P not diagonal: one fine element shared by two coarse ones
    L0, L1 = prob.levels[0], prob.levels[1]
    P = L0.P.tolil()
    P[0, (P.rows[0][0] + 1) % L1.n_s] = 0.5
    rc, msg = _create(gpu_ctx, prob, levels=[KLLevel(L0.n_s, L0.w_diag, sp.csr_matrix(P)), L1], nlevels=2)
    assert rc == -1 and "not diagonal" in msg
    # wrong shape of P
    rc, _ = _create(gpu_ctx, prob, levels=[KLLevel(L0.n_s, L0.w_diag, L0.P[:, :-1]), L1], nlevels=2)
    assert rc == -1


def test_field_statistics(gpu_ctx):
    """N = 16384 device draws on the 4^3 level (64 elements, all 64 modes): sample covariance against Phi Lambda Phi^T in
    Frobenius norm, mean ~ 0; lognormal: E[exp s_i] = exp(1/2 sum_k lambda_k Phi_ik^2)"""
    from parelagmc_amd import capi
    N, level = 16384, 2
    for lognormal in (False, True):
        prob = _problems()["hex_analytic"](lognormal)
        smp = capi.KLSampler(gpu_ctx, prob)
        xi = smp.Sample(level, first_id=0, nbatch=N)
        s, g = smp.Eval(level, xi, xi_level=level, want_embed=True)
        smp.close()
        phi = prob.evects[level]
        Cov = (phi * prob.evals[None, :]) @ phi.T
        var = np.diag(Cov)
        if not lognormal:
            assert np.all(np.abs(g.mean(0)) <= 5 * np.sqrt(var / N))
            Chat = g.T @ g / N
            sigma_f = np.sqrt(np.sum(np.outer(var, var) + Cov ** 2) / N)
            assert np.linalg.norm(Chat - Cov) <= 3 * sigma_f, (np.linalg.norm(Chat - Cov), sigma_f)
        else:
            mean = np.exp(0.5 * var)
            sd = np.sqrt((np.exp(var) - 1.0) * np.exp(var) / N)
            assert np.all(np.abs(s.mean(0) - mean) <= 4 * sd)


def test_mlmc_manager_over_the_kl_handle_equals_the_numpy_callbacks(gpu_ctx, hex_hierarchy):
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_darcy_problem
    prob = _problems()["hex_analytic"](True)
    dp = build_darcy_problem(hex_hierarchy, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
    smp = capi.KLSampler(gpu_ctx, prob)
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(rel_tol=1e-12, abs_tol=1e-14))
    counts = [40, 70, 130]
    mgr = host_api.MLMCManager(3, sampler=smp, solver=ds, wall_time=False, batch=32)
    dev = mgr.InitRun(counts)
    mgr.close()

    def f_eval(level, xi_level, xi, init, init_level):
        g, _ = _gauss_ref(prob, level, xi)
        return np.exp(g), g

    cb = dict(sample=lambda level, first_id, nb: smp.Sample(level, first_id=first_id, nbatch=nb), eval=f_eval,
              solve=lambda level, k: ds.SolveFwd(level, np.ascontiguousarray(k))[:2],
              xi_size=[L.n_s for L in prob.levels], sample_size=[L.n_s for L in prob.levels],
              ndofs=[ds.GetGlobalNumberOfDofs(lvl) for lvl in range(3)])
    mgr = host_api.MLMCManager(3, callbacks=cb, wall_time=False, batch=32)
    ref = mgr.InitRun(counts)
    mgr.close()
    assert list(dev["nsamples"]) == list(ref["nsamples"]) == counts
    assert np.allclose(dev["sums"], ref["sums"], rtol=1e-8, atol=1e-12)
    ds.close()
    smp.close()


def test_ratio_manager_takes_the_kl_handle(gpu_ctx, hex_hierarchy_small):
    from oracle.bayes_oracle import observation_functionals
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_darcy_problem, build_kl_sampler_problem
    h = hex_hierarchy_small
    prob = build_kl_sampler_problem(h, "analytic", corlen=0.1, lognormal=True)
    assert prob.n_mc_levels == 2
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
    smp = capi.KLSampler(gpu_ctx, prob)
    ds = capi.DarcySolver(gpu_ctx, dp, capi.solver_opts(rel_tol=1e-12, abs_tol=1e-300))
    Gobs = observation_functionals(h, np.array([[0.5, 0.5, 0.5], [1.4, 1.2, 0.6]]), eps=0.3)
    for lvl in range(2):
        ds.SetObservations(lvl, Gobs[lvl])
    G_obs = ds.ComputeG(0, smp.Eval(0, smp.Sample(0, first_id=12345)))[0][0]
    mgr = host_api.RatioManager(2, sampler=smp, solver=ds, G_obs=G_obs, noise=0.05, wall_time=False)
    r = mgr.InitRun([20, 40])
    mgr.close()
    assert list(r["nsamples"]) == [20, 40] and np.all(np.isfinite(r["sums"]))
    ds.close()
    smp.close()


def _write_kl_file(path, prob, xi):
    with open(path, "wb") as f:
        np.array([0x4b4c3031, len(prob.levels), prob.nmodes, 1 if prob.lognormal else 0, xi.shape[0]], np.int32).tofile(f)
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
        xi.astype(np.float64).tofile(f)
        for lvl in range(len(prob.levels)):
            g, _ = _gauss_ref(prob, lvl, xi)
            (np.exp(g) if prob.lognormal else g).astype(np.float64).tofile(f)


def test_c_and_cpp_callers(tmp_path):
    r = subprocess.run(["make", "-C", ROOT, "test-kl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    prob = _problems()["hex_matern"](True)
    xi = np.random.default_rng(9).standard_normal((3, prob.levels[0].n_s))
    path = str(tmp_path / "kl.bin")
    _write_kl_file(path, prob, xi)
    for exe in ("kl_smoke", "kl_adapter_smoke"):
        r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", exe), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith(f"{exe} OK"), r.stdout + r.stderr

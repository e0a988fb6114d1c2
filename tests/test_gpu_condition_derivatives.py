"""Tangent and adjoint of the conditioning map on the device (csrc/condition.hip: pmc_conditioner_apply_tangent /
_apply_adjoint), the hooked pmc_sampler_eval_tangent / _eval_adjoint of a conditioner with derivatives enabled, and the
pmc_bayes_* chain over conditioned handles, against long-double references and the numpy twins
(parelagmc_amd/fe/condition.py, fe/sampler_adjoint.py, fe/map_estimate.py with conditioner=).

The adjoint's bound (test_adjoint_kernels).  With eps = 2^-53, u = fl(v o s_out), |K|, |A^-1|, |H| the entrywise moduli, to
first order in eps and for ANY order of the sums (so for both kernels and every chunking):

    t = K^T u, n products per entry:                       |dt| <= (n + 3) eps |K|^T |u|
        (n - 1 additions and the products' roundings are n eps; the rounding of u and the slack for the zero start of the
        accumulators and the ascending sum over the chunk partials are the + 3)
    c = A^-1 t with the inverse rounded from long double:  |dc| <= |A^-1| |dt| + (nobs + 3) eps |A^-1| |t|
        (nobs eps for the sum, the + 3 for the entries of the rounded inverse: DESIGN.md section 15a)
    w = u - H^T c, at most m_H entries per column of H:    |dw| <= eps |u| + |H|^T (|dc| + (m_H + 1) eps |c|) + eps |w|
        (the rounding of u = v o s_out, the fma chain over the column, the one subtraction)

The reference takes u = v o s_out, K^T u, the solve with A (a Cholesky factorization, not an inverse) and H^T c in long
double; |A^-1| of the bound is the double inverse of A (a bound needs no more).

Tolerances against the twins with direct solves (handles at rel_tol = abs_tol = 1e-12) are 10 x the values measured on an
MI355X over every case of this file, never looser than 1e-7 (the rule at the top of tests/test_gpu_darcy_gradient.py):

    MEASURED_PAIR        transposition defect |<T dg, u> - <dg, T^T u>| / (|dg| |u o s|) of the device pair apply_tangent /
                         apply_adjoint
    MEASURED_HOOK_PAIR   the same for the hooked EvalTangent / EvalAdjoint, relative to |EvalTangent v| |u| + |v| |EvalAdjoint u|
    MEASURED_HOOK_TWIN   relative L2 deviation of the hooked EvalTangent / EvalAdjoint from the conditioned twins
    MEASURED_CHAIN       relative deviation of bayes_logpost_gradient (logpost and gradient) and bayes_logpost_gn_hessvec
    MEASURED_MAP_LOGPOST, MEASURED_MAP_XI   as MEASURED_TWIN_LOGPOST / _XI of tests/test_gpu_map_estimate.py

The tangent is compared as tests/test_gpu_condition.py compares the forward apply (1e-12 relative L2 per column, the same
kernels).  On a level where H_l is square and invertible (as many exact point observations as elements: hex level 2 with 64,
ragged level 1 with 30) Gamma_l = 0, the exact tangent is zero and both results are rounding errors: there the 1e-12 is
taken relative to |dg|."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import condition_derivative_cases as cdc
import map_cases as mc
from conftest import ROOT
from test_gpu_condition import _observations, _problem, _sampler, _write_problem
from test_gpu_map_estimate import Handles, RTOL, rel

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
WIDTHS = (1, 2, 4, 5, 16, 17, 64, 129, 260)
NBMAX = max(WIDTHS)
MEASURED_PAIR = 5.4e-15         # ragged, 30 observations; the others 1.7e-16 .. 3.8e-15
MEASURED_HOOK_PAIR = 1.1e-13    # saddle-point handle; hybridized 3.5e-14, KL 7.7e-17
MEASURED_HOOK_TWIN = 1.5e-12    # hybridized handle; saddle-point 7.4e-13, KL 8.9e-16
MEASURED_CHAIN = 1.2e-11        # hybridized handle; saddle-point 1.1e-11, KL 2.6e-12
MEASURED_MAP_LOGPOST = 4.3e-10  # ragged-10 on the saddle-point handle; the others 3.5e-11 .. 3.9e-11
MEASURED_MAP_XI = 2.5e-11       # ragged-00 on the KL handle; the SPDE handles 3.5e-12 .. 9.7e-12
TOL_PAIR = min(10 * MEASURED_PAIR, 1e-7)
TOL_HOOK_PAIR = min(10 * MEASURED_HOOK_PAIR, 1e-7)
TOL_HOOK_TWIN = min(10 * MEASURED_HOOK_TWIN, 1e-7)
TOL_CHAIN = min(10 * MEASURED_CHAIN, 1e-7)
TOL_MAP_LOGPOST = min(10 * MEASURED_MAP_LOGPOST, 1e-7)
TOL_MAP_XI = min(10 * MEASURED_MAP_XI, 1e-7)


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def ragged_hierarchy():
    return mc.problems("ragged")[0]      # n_s = 240 / 30


@pytest.fixture(scope="module")
def hybrid_handles(gpu_ctx, hex_hierarchy, ragged_hierarchy):
    """Gaussian hybridized handles on the two meshes, shared by the kernel tests"""
    out = {}
    for name, h in (("hex", hex_hierarchy), ("ragged", ragged_hierarchy)):
        prob = _problem("hybrid", h)
        out[name] = (h, prob, _sampler(gpu_ctx, "hybrid", prob))
    yield out
    for _, _, smp in out.values():
        smp.close()


def _chol_solve_ld(A, T):
    """A^-1 T in long double by Cholesky (A (m, m) symmetric positive definite, T (m, k))"""
    m = A.shape[0]
    L = np.zeros((m, m), np.longdouble)
    A = np.asarray(A, np.longdouble)
    for j in range(m):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    X = np.array(T, np.longdouble)
    for j in range(m):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    for j in range(m - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def _adjoint_reference(K, A, H, V):
    """(w in long double rounded to double, the entrywise bound) for the columns V (nb, n), no s_out"""
    n, nobs = K.shape
    Hd = H.toarray()
    U = np.asarray(V, np.longdouble)
    T = np.asarray(K, np.longdouble).T @ U.T                          # (nobs, nb)
    Cc = _chol_solve_ld(A, T)
    W = U - (np.asarray(Hd, np.longdouble).T @ Cc).T
    aK, aH, aU = np.abs(K), np.abs(Hd), np.abs(V)
    aAinv = np.abs(np.linalg.inv(A))
    dt = (n + 3) * EPS * (aK.T @ aU.T)
    dc = aAinv @ dt + (nobs + 3) * EPS * (aAinv @ np.abs(np.asarray(T, np.float64)))
    m_h = int(np.max(np.diff(sp.csc_matrix(H).indptr)))
    Wd = np.asarray(W, np.float64)
    bound = EPS * aU + (aH.T @ (dc + (m_h + 1) * EPS * np.abs(np.asarray(Cc, np.float64)))).T + EPS * np.abs(Wd)
    return Wd, bound


def _overlap_observations(h):
    """5 point rows and an averaging row over the siblings of the FIRST point: its column of H holds two entries"""
    from parelagmc_amd.fe.condition import pick_observation_elements, point_observations
    elems = pick_observation_elements(h, 5, 5)
    parent = sp.csr_matrix(h.P[0]).indices
    sib = np.nonzero(parent == parent[elems[0]])[0]
    H0 = point_observations(h.spaces[0].n_s, elems, [(sib, np.full(sib.size, 1.0 / sib.size))])
    return H0, np.random.default_rng(105).normal(0.0, 1.0, 6), np.full(6, 0.05)


# ("deep", 129): 129 noisy observations of tests/gemm_depth_cases.py on its KL handle (n = 1920 / 240) - three mode blocks of
# the adjoint's reduction, where a workgroup carries 4 (nb = 64) and 8 (nb >= 81) realization tiles instead of 1 or 2
KERNEL_CASES = [("hex", n) for n in (1, 5, 16, 17, 33, 64)] + [("ragged", n) for n in (1, 5, 30)] + [("hex", "overlap"),
                                                                                                    ("deep", 129)]


@pytest.fixture(scope="module", params=KERNEL_CASES, ids=[f"{m}-{n}" for m, n in KERNEL_CASES])
def kernel_case(request, gpu_ctx, hybrid_handles):
    """(mesh, nobs, conditioner, per level: K, A, H, V, S, the long-double adjoint of V and its bound), computed once"""
    from parelagmc_amd import capi
    mesh, nobs = request.param
    own = None
    if mesh == "deep":
        import gemm_depth_cases as gdc
        prob = gdc.real_problem(False)
        own = smp = capi.KLSampler(gpu_ctx, prob)
        H0, y, sigma2 = gdc.observations(nobs, "noisy")
    elif nobs == "overlap":
        h, prob, smp = hybrid_handles[mesh]
        H0, y, sigma2 = _overlap_observations(h)
    else:
        h, prob, smp = hybrid_handles[mesh]
        H0, y = _observations(h, nobs, seed=nobs, averaging=(nobs == 5))
        sigma2 = None
    cond = capi.Conditioner(smp, H0, y, sigma2)
    rng = np.random.default_rng(2000 + H0.shape[0])
    levels = []
    for lvl in range(prob.n_mc_levels):
        K, A, H = cond.level(lvl)
        n = K.shape[0]
        V = rng.standard_normal((NBMAX, n))
        S = np.exp(0.3 * rng.standard_normal((NBMAX, n)))
        levels.append((K, A, H, V, S) + _adjoint_reference(K, A, H, V))
    yield mesh, nobs, cond, levels
    cond.close()
    if own is not None:
        own.close()


def test_adjoint_kernels(gpu_ctx, kernel_case):
    """every entry of apply_adjoint within the first-order bound of the module docstring, at every width; the bitwise rules"""
    mesh, nobs, cond, levels = kernel_case
    worst = 0.0
    for lvl, (K, A, H, V, S, ref, bound) in enumerate(levels):
        n = K.shape[0]
        outs = {}
        for nb in WIDTHS:
            out = cond.apply_adjoint(lvl, V[:nb])
            ratio = float(np.max(np.abs(out - ref[:nb]) / bound[:nb]))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (lvl, nb, ratio)
            assert _bits(out, cond.apply_adjoint(lvl, V[:nb])), "two identical calls differ"
            outs[nb] = out
        wide = [nb for nb in WIDTHS if nb > 4]
        for nb in wide[:-1]:     # a column's bits do not depend on nbatch: MFMA kernel ...
            assert _bits(outs[nb], outs[NBMAX][:nb]), (lvl, nb)
        assert _bits(outs[1], outs[4][:1]) and _bits(outs[2], outs[4][:2])     # ... and VALU kernel
        # 129 = 64 + 64 + 1: the wide pieces keep their bits, the last piece takes the VALU kernel and stays within the bound
        assert _bits(np.concatenate([cond.apply_adjoint(lvl, V[:64]), cond.apply_adjoint(lvl, V[64:128])]), outs[129][:128])
        last = cond.apply_adjoint(lvl, V[128:129])
        assert np.all(np.abs(last - ref[128:129]) <= bound[128:129])
        for nb in (3, 17, 129):
            # s_out given equals the Gaussian call fed v * s_out (u is one rounding, formed in the load)
            assert _bits(cond.apply_adjoint(lvl, V[:nb], S[:nb]), cond.apply_adjoint(lvl, V[:nb] * S[:nb])), (lvl, nb)
            vd, sd, od = gpu_ctx.array(V[:nb]), gpu_ctx.array(S[:nb]), gpu_ctx.array(np.zeros((nb, n)))
            cond.apply_adjoint(lvl, vd, out=od)
            assert _bits(od.download().reshape(nb, n), cond.apply_adjoint(lvl, V[:nb])), "device and host memory differ"
            cond.apply_adjoint(lvl, vd, sd, out=od)
            assert _bits(od.download().reshape(nb, n), cond.apply_adjoint(lvl, V[:nb], S[:nb]))
            assert _bits(vd.download().reshape(nb, n), V[:nb]) and _bits(sd.download().reshape(nb, n), S[:nb])
            for a in (vd, sd, od):
                a.free()
    print(f"[{mesh} nobs {nobs}] adjoint: worst error / bound {worst:.3f}")


def test_tangent_kernels_and_the_pair(gpu_ctx, kernel_case):
    """apply_tangent within 1e-12 relative L2 per column of the twin fed the device's own K, A; its bitwise rules; the
    transposition identity of the device pair"""
    from parelagmc_amd.fe.condition import apply_tangent
    mesh, nobs, cond, levels = kernel_case
    worst, defect = 0.0, 0.0
    for lvl, (K, A, H, V, S, ref, bound) in enumerate(levels):
        n = K.shape[0]
        DG = np.random.default_rng(3000 + lvl).standard_normal((NBMAX, n))
        tref = apply_tangent(K, A, H, DG)
        degenerate = H.shape[0] == n and not cond.noisy      # Gamma_l = 0: see the module docstring
        den = np.linalg.norm(DG if degenerate else tref, axis=1)
        outs = {}
        for nb in WIDTHS:
            out = cond.apply_tangent(lvl, DG[:nb])
            err = float(np.max(np.linalg.norm(out - tref[:nb], axis=1) / den[:nb]))
            worst = max(worst, err)
            assert err <= 1e-12, (lvl, nb, err)
            assert _bits(out, cond.apply_tangent(lvl, DG[:nb])), "two identical calls differ"
            outs[nb] = out
        for nb in (5, 16, 17, 64, 129):
            assert _bits(outs[nb], outs[NBMAX][:nb]), (lvl, nb)
        assert _bits(outs[1], outs[4][:1]) and _bits(outs[2], outs[4][:2])
        for nb in (3, 17):
            ts = cond.apply_tangent(lvl, DG[:nb], S[:nb])
            assert _bits(ts, cond.apply_tangent(lvl, DG[:nb]) * S[:nb])
            gd, sd = gpu_ctx.array(DG[:nb]), gpu_ctx.array(S[:nb])
            cond.apply_tangent(lvl, gd, sd)                                   # device memory, in place
            assert _bits(gd.download().reshape(nb, n), ts), "device / in-place result differs from the host call"
            gd.free()
            sd.free()
            inplace = DG[:nb].copy()
            cond.apply_tangent(lvl, inplace, out=inplace)
            assert _bits(inplace, outs[NBMAX][:nb] if nb > 4 else cond.apply_tangent(lvl, DG[:nb]))
        if not cond.noisy:     # a tangent cannot move exact data
            assert np.max(np.abs(H @ outs[17].T)) <= 1e-9
        # <T dg, u> = <dg, T^T u>, with and without s_out
        for nb in (4, 17):
            for s in (None, S[:nb]):
                t, a = cond.apply_tangent(lvl, DG[:nb], s), cond.apply_adjoint(lvl, V[:nb], s)
                us = V[:nb] if s is None else V[:nb] * s
                d = np.abs(np.einsum("ij,ij->i", t, V[:nb]) - np.einsum("ij,ij->i", DG[:nb], a)) / \
                    (np.linalg.norm(DG[:nb], axis=1) * np.linalg.norm(us, axis=1))
                defect = max(defect, float(d.max()))
    print(f"[{mesh} nobs {nobs}] tangent: worst relative L2 {worst:.2e}; transposition defect of the pair {defect:.2e}")
    assert defect <= TOL_PAIR


def _refused(fn, match="conditioner"):
    from parelagmc_amd import capi
    with pytest.raises(capi.PmcError) as ei:
        fn()
    assert ei.value.code == -1 and match in str(ei.value), str(ei.value)


def test_new_entries_refuse_bad_arguments(gpu_ctx, hybrid_handles):
    """PMC_ERR_INVALID with a message, and the output untouched"""
    import ctypes as C
    from parelagmc_amd import capi
    h, prob, smp = hybrid_handles["ragged"]
    H0, y = _observations(h, 5, seed=5)
    cond = capi.Conditioner(smp, H0, y)
    lib = gpu_ctx.lib
    n = prob.levels[0].n_s
    v, s, out = np.ones((2, n)), np.ones((2, n)), np.full((2, n), 7.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    H, D = capi.PMC_MEM_HOST, capi.PMC_MEM_DEVICE
    assert D != 5 and H != 5
    for fn in (lib.pmc_conditioner_apply_tangent, lib.pmc_conditioner_apply_adjoint):
        for args in ((-1, 2, p(v), p(s), p(out), H), (prob.n_mc_levels, 2, p(v), p(s), p(out), H), (0, 0, p(v), p(s), p(out), H),
                     (0, 2, None, p(s), p(out), H), (0, 2, p(v), p(s), None, H), (0, 2, p(v), p(s), p(out), 5),
                     (0, 2, p(v), p(out), p(out), H)):
            assert fn(cond.h, *args) == -1 and len(lib.pmc_last_error()) > 0, args
        assert fn(None, 0, 2, p(v), p(s), p(out), H) == -1
    assert lib.pmc_conditioner_apply_adjoint(cond.h, 0, 2, p(out), None, p(out), H) == -1      # out aliasing v
    assert lib.pmc_conditioner_enable_derivatives(None, 1) == -1 and lib.pmc_conditioner_derivatives_enabled(None) == -1
    assert np.all(out == 7.0) and np.all(v == 1.0)
    assert lib.pmc_conditioner_apply_tangent(cond.h, 0, 2, p(v), None, p(v), H) == 0           # the tangent may alias dg
    cond.close()


# ---- the hook ------------------------------------------------------------------------------------------------------------------
HOOK_PAIRS = [(0, 0), (1, 0), (1, 1)]


class Conditioned(Handles):
    """Handles of tests/test_gpu_map_estimate.py (lognormal prior on the mesh of `name`) with the hard data of
    condition_derivative_cases attached and derivatives enabled; .twin_cond is the conditioned twin"""

    def __init__(self, ctx, name, kind):
        from parelagmc_amd import capi
        super().__init__(ctx, name, kind)
        mesh = mc.CASES[name][0]
        H0, y = cdc.hard_data(mesh)
        self.cond = capi.Conditioner(self.smp, H0, y).enable_derivatives()
        self.smp.SetConditioner(self.cond)
        self.twin_cond = cdc.twin_conditioner(mesh, "kl" if kind == "kl" else "spde")

    def close(self):
        self.smp.SetConditioner(None)
        self.cond.close()
        super().close()


@pytest.fixture(scope="module", params=["saddle", "hybrid", "kl"])
def hooked(request, gpu_ctx):
    h = Conditioned(gpu_ctx, "ragged-10", request.param)
    yield h
    h.close()


def test_hook_is_the_composition_of_the_public_pieces(hooked):
    """enabled EvalTangent / EvalAdjoint equal detach + EvalTangent / EvalAdjoint + apply_tangent / apply_adjoint bit for bit;
    the pair is transposed; two successive adjoint calls with different v (default graph setting) both match"""
    h, smp, cond = hooked, hooked.smp, hooked.cond
    rng = np.random.default_rng(41)
    defect = 0.0
    for level, xi_level in HOOK_PAIRS:
        n, n_xi = smp.SampleSize(level), smp.xi_size(xi_level)
        for nb in (3, 6):
            assert nb <= smp.BatchWidth(level)
            xi, v = 0.5 * rng.standard_normal((nb, n_xi)), rng.standard_normal((nb, n_xi))
            u, u2 = rng.standard_normal((nb, n)), rng.standard_normal((nb, n))
            s = smp.Eval(level, xi, xi_level=xi_level)                     # the conditional lognormal field
            assert np.max(np.abs((cond.level(level)[2] @ np.log(s).T).T - cdc.hard_data("ragged")[1][None, :])) <= 1e-9
            t = smp.EvalTangent(level, v, s, xi_level=xi_level)
            t0 = smp.EvalTangent(level, v, None, xi_level=xi_level)
            a = smp.EvalAdjoint(level, u, s, xi_level=xi_level)
            a2 = smp.EvalAdjoint(level, u2, None, xi_level=xi_level)
            a_again = smp.EvalAdjoint(level, u, s, xi_level=xi_level)
            smp.SetConditioner(None)
            try:
                lt = smp.EvalTangent(level, v, None, xi_level=xi_level)
                assert _bits(t, cond.apply_tangent(level, lt, s)) and _bits(t0, cond.apply_tangent(level, lt))
                assert _bits(a, smp.EvalAdjoint(level, cond.apply_adjoint(level, u, s), None, xi_level=xi_level))
                assert _bits(a2, smp.EvalAdjoint(level, cond.apply_adjoint(level, u2), None, xi_level=xi_level))
                assert _bits(a_again, a)
            finally:
                smp.SetConditioner(cond)
            d = np.abs(np.einsum("ij,ij->i", t, u) - np.einsum("ij,ij->i", v, a)) / \
                (np.linalg.norm(t, axis=1) * np.linalg.norm(u, axis=1) + np.linalg.norm(v, axis=1) * np.linalg.norm(a, axis=1))
            defect = max(defect, float(d.max()))
    print(f"[{h.kind}] hooked pair: transposition defect {defect:.2e}")
    assert defect <= TOL_HOOK_PAIR


def test_hook_matches_the_conditioned_twins(hooked):
    from parelagmc_amd.fe import sampler_adjoint
    h, smp = hooked, hooked.smp
    rng = np.random.default_rng(43)
    worst = 0.0
    cache = {}
    for level, xi_level in HOOK_PAIRS:
        n, n_xi = smp.SampleSize(level), smp.xi_size(xi_level)
        for nb in (3, 6):
            xi, v, u = 0.5 * rng.standard_normal((nb, n_xi)), rng.standard_normal((nb, n_xi)), rng.standard_normal((nb, n))
            s = smp.Eval(level, xi, xi_level=xi_level)
            for s_out in (s, None):
                t = smp.EvalTangent(level, v, s_out, xi_level=xi_level)
                a = smp.EvalAdjoint(level, u, s_out, xi_level=xi_level)
                for b in range(nb):
                    sb = None if s_out is None else s_out[b]
                    tt = sampler_adjoint.eval_tangent(h.sp, level, xi_level, v[b], sb, None, cache, h.twin_cond)
                    ta = sampler_adjoint.eval_adjoint(h.sp, level, xi_level, u[b], sb, None, cache, h.twin_cond)
                    worst = max(worst, rel(t[b], tt), rel(a[b], ta))
            sf = np.array([sampler_adjoint.eval_forward(h.sp, level, xi_level, x, None, cache, h.twin_cond) for x in xi])
            worst = max(worst, max(rel(s[b], sf[b]) for b in range(nb)))
    print(f"[{h.kind}] hooked EvalTangent / EvalAdjoint against the conditioned twins: {worst:.2e}")
    assert worst <= TOL_HOOK_TWIN


def test_a_tangent_cannot_move_exact_data(gpu_ctx, ragged_hierarchy):
    """H . EvalTangent(v) = 0 to 1e-9 on a Gaussian handle"""
    from parelagmc_amd import capi
    prob = _problem("saddle", ragged_hierarchy)
    smp = capi.PDESampler(gpu_ctx, prob, capi.solver_opts(rel_tol=1e-12, abs_tol=1e-12, max_iter=400))
    H0, y = cdc.hard_data("ragged")
    cond = capi.Conditioner(smp, H0, y).enable_derivatives()
    assert cond.derivatives_enabled
    smp.SetConditioner(cond)
    rng = np.random.default_rng(47)
    for level, xi_level in HOOK_PAIRS:
        for nb in (3, 6):
            t = smp.EvalTangent(level, rng.standard_normal((nb, smp.xi_size(xi_level))), xi_level=xi_level)
            moved = float(np.max(np.abs(cond.level(level)[2] @ t.T)))
            assert np.max(np.abs(t)) > 1e-3 and moved <= 1e-9, (level, xi_level, nb, moved)
    cond.close()
    smp.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def test_bayes_gradient_and_gn_hessian_over_conditioned_handles(hooked):
    from parelagmc_amd import host_api
    from parelagmc_amd.fe import sampler_adjoint
    h = hooked
    rng = np.random.default_rng(53)
    nb = 3
    xi, v = 0.5 * rng.standard_normal((nb, h.n_xi)), rng.standard_normal((nb, h.n_xi))
    lp, g = h.gradient(xi)
    hv, _ = host_api.bayes_logpost_gn_hessvec(h.smp, h.ds, h.level, xi, v, h.noise, xi_level=h.xi_level)
    cache = {}
    worst = 0.0
    for b in range(nb):
        tlp, tg = sampler_adjoint.logpost_gradient(h.sp, h.dp, h.level, xi[b], h.Gobs, h.data, h.noise, h.xi_level, None, cache,
                                                   h.twin_cond)
        thv = sampler_adjoint.logpost_gn_hessvec(h.sp, h.dp, h.level, xi[b], v[b], h.Gobs, h.noise, h.xi_level, None, cache,
                                                 h.twin_cond)
        worst = max(worst, abs(lp[b] - tlp) / abs(tlp), rel(g[b], tg), rel(hv[b], thv))
    print(f"[{h.kind}] conditioned logpost, gradient and GN Hessian action against the twins: {worst:.2e}")
    assert worst <= TOL_CHAIN


# the twin's smallest decision margin of each case, computed on the CPU: above the 1e-6 the integer comparison requires.
# ragged-00 on the SPDE prior decides by 1.8e-7 and is not a case.
MAP_CASES = [("ragged-10", "saddle", 1.9e-4), ("tet1-00", "hybrid", 7.7e-5), ("ragged-00", "kl", 4.3e-6)]


@pytest.mark.parametrize("name,kind,cpu_margin", MAP_CASES, ids=[f"{c[0]}-{c[1]}" for c in MAP_CASES])
def test_map_over_conditioned_handles(gpu_ctx, name, kind, cpu_margin):
    """as test_trajectory_and_values_match_the_twin of tests/test_gpu_map_estimate.py; at the result H log k_MAP = y"""
    from parelagmc_amd.fe import map_estimate
    h = Conditioned(gpu_ctx, name, kind)
    try:
        x0 = mc.starts(name, 3, 0.5)
        kw = dict(grad_rtol=RTOL, max_newton=40)
        xt, rt = map_estimate.map_estimate(h.sp, h.dp, h.level, x0, h.Gobs, h.data, h.noise, h.xi_level, conditioner=h.twin_cond,
                                           **kw)
        margin = min(rt["cg_margins"].min(), rt["armijo_margins"].min(), rt["conv_margins"].min())
        assert margin >= 1e-6, f"{name}: the twin decides by {margin:.1e}: not a case for the integer comparison"
        assert np.all(rt["status"] == 0)
        xi, res = h.map(x0, **kw)
        for key in ("status", "newton_iterations", "hessian_actions", "gradient_evaluations", "nonpos_curvature", "hist_cg"):
            assert np.array_equal(res[key], rt[key]), (key, res[key], rt[key])
        assert np.array_equal(np.nan_to_num(res["hist_t"], nan=-1.0), np.nan_to_num(rt["hist_t"], nan=-1.0))
        ok = np.isfinite(rt["hist_logpost"])
        assert np.array_equal(ok, np.isfinite(res["hist_logpost"]))
        e_lp = float(np.max(np.abs(res["hist_logpost"][ok] - rt["hist_logpost"][ok]) / np.abs(rt["hist_logpost"][ok])))
        e_xi = max(rel(xi[b], xt[b]) for b in range(3))
        k = h.smp.Eval(h.level, xi, xi_level=h.xi_level)
        miss = float(np.max(np.abs((h.cond.level(h.level)[2] @ np.log(k).T).T - cdc.hard_data(mc.CASES[name][0])[1][None, :])))
        print(f"{name} {kind}: outer iterations {res['newton_iterations']}, smallest twin margin {margin:.1e} (CPU: "
              f"{cpu_margin:.1e}); logpost history {e_lp:.2e}, xi_MAP {e_xi:.2e} from the twin; |H log k_MAP - y| {miss:.2e}")
        assert miss <= 1e-9
        assert e_lp <= TOL_MAP_LOGPOST and e_xi <= TOL_MAP_XI
    finally:
        h.close()


# ---- opt-in and refusals -------------------------------------------------------------------------------------------------------
def test_opt_in_and_refusals(gpu_ctx):
    from parelagmc_amd import capi, host_api
    h = Handles(gpu_ctx, "ragged-10", "saddle")
    try:
        H0, y = cdc.hard_data("ragged")
        cond = capi.Conditioner(h.smp, H0, y)
        assert not cond.derivatives_enabled
        h.smp.SetConditioner(cond)
        n, n_xi = h.smp.SampleSize(h.level), h.n_xi
        xi, v, u = np.zeros((2, n_xi)), np.ones((2, n_xi)), np.ones((2, n))

        def all_refuse():
            _refused(lambda: h.smp.EvalAdjoint(h.level, u, xi_level=h.xi_level))
            _refused(lambda: h.smp.EvalTangent(h.level, v, xi_level=h.xi_level))
            _refused(lambda: h.gradient(xi))
            _refused(lambda: host_api.bayes_logpost_gn_hessvec(h.smp, h.ds, h.level, xi, v, h.noise, xi_level=h.xi_level))
            _refused(lambda: h.map(xi))

        all_refuse()
        _refused(lambda: h.smp.EvalAdjoint(h.level, u, xi_level=h.xi_level), match="pmc_conditioner_enable_derivatives")
        cond.enable_derivatives()
        assert cond.derivatives_enabled
        h.smp.EvalAdjoint(h.level, u, xi_level=h.xi_level)
        h.smp.EvalTangent(h.level, v, xi_level=h.xi_level)
        h.gradient(xi)
        cond.enable_derivatives(False)
        assert not cond.derivatives_enabled
        all_refuse()
        h.smp.SetConditioner(None)
        # a noisy conditioner still cannot be attached, with or without the opt-in; its two apply entries work
        noisy = capi.Conditioner(h.smp, H0, y, np.full(y.size, 0.05)).enable_derivatives()
        _refused(lambda: h.smp.SetConditioner(noisy))
        n0 = h.smp.SampleSize(0)
        assert np.all(np.isfinite(noisy.apply_tangent(0, np.ones((2, n0)))))
        assert np.all(np.isfinite(noisy.apply_adjoint(0, np.ones((2, n0)))))
        noisy.close()
        cond.close()
    finally:
        h.close()


# ---- a C caller ----------------------------------------------------------------------------------------------------------------
def test_c_caller(hex_hierarchy, tmp_path):
    """tests/c/condition_derivatives_smoke.c (plain C, include/pmc.h only) builds with -Wall -Wextra -Werror and passes"""
    r = subprocess.run(["make", "-C", ROOT, "test-condition-derivatives"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    prob = _problem("kl", hex_hierarchy, lognormal=True)
    path = str(tmp_path / "kl.bin")
    _write_problem(path, prob)
    H0, y = _observations(hex_hierarchy, 5, seed=5)
    args = [a for e, v in zip(H0.indices, y) for a in (str(int(e)), repr(float(v)))]
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "condition_derivatives_smoke"), path, "11"] + args,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("condition_derivatives_smoke OK"), r.stdout + r.stderr

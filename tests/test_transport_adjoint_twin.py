"""The numpy twin of the transport adjoint (fe.transport.advance_adjoint / advance_tangent): the adjoint
identity, finite differences in log k through the oracle's direct solve, rounding against np.longdouble, the invariance of
the gradient in k under the branch of r_e on tied elements, the independence of the checkpoint segment, the columns that are
not differentiated, the refusals, and the header.  No GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import transport_adjoint_cases as ta
import transport_cases as tc
from conftest import ROOT
from parelagmc_amd.fe import transport as tw

NEW_SYMBOLS = ("pmc_transport_run_adjoint", "pmc_transport_set_adjoint_segment", "pmc_darcy_transport_gradient",
               "pmc_darcy_transport_loglik_gradient")
EPS = np.finfo(np.float64).eps


def test_header_and_bindings():
    from parelagmc_amd import capi
    header = open(os.path.join(ROOT, "include", "pmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "#define PMC_ABI_VERSION 3 " in header
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in capi.SYMBOLS, s
    for cls, names in ((capi.Transport, ("run_adjoint", "set_adjoint_segment")),
                       (capi.DarcySolver, ("TransportGradient", "TransportLoglikGradient"))):
        assert all(hasattr(cls, n) for n in names)
    hpp = open(os.path.join(ROOT, "parelagmc_amd", "host", "parelagmc.hpp")).read()
    for name in ("RunAdjoint(", "SolveFwd_TransportGradient(", "ComputeGradTransportLogLikelihood("):
        assert name in hpp, name
    from parelagmc_amd import fe
    assert fe.advance_adjoint is tw.advance_adjoint and fe.advance_tangent is tw.advance_tangent


@pytest.mark.parametrize("name", ta.NAMES)
def test_forward_results_are_those_of_advance(name):
    r, f = ta.twin(name), tc.twin(name)
    for key in ("c", "curve", "stored", "rate", "nsteps", "dt", "t_reached", "status"):
        assert np.array_equal(r[key], f[key]), key
    assert (r["g_margin"][:4] > 1e-7).all() and np.isinf(r["g_margin"][4])        # smallest nonzero |g| / max |g|
    assert (r["u_bar"][4] == 0).all()                                             # zero flux: every g == 0 contributes nothing


@pytest.mark.parametrize("name", ta.NAMES)
def test_adjoint_identity(name):
    """<advance_tangent(du), seeds> == <du, u_bar> for random du: linear algebra under fixed decisions, so du is arbitrary.
    Bound: 64 eps times the sum of the absolute values of the terms of both inner products."""
    c, r = tc.case(name), ta.twin(name)
    sd = ta.all_seeds(name)
    rng = np.random.Generator(np.random.PCG64(3 + ta.NAMES.index(name)))
    du = rng.standard_normal(c.u.shape)
    t = tw.advance_tangent(c.mesh, c.u, du, c.t_end, tc.CFL, ta.NREPORT)
    nf = c.mesh.n_face
    for b in range(5):
        left = np.concatenate([t["dcurve"][b] * sd["curve_bar"][b], [t["dstored"][b] * sd["stored_bar"][b]], t["dc"][b] * sd["c_bar"][b]])
        right = du[b, :nf] * r["u_bar"][b]
        bound = 64 * EPS * (np.abs(left).sum() + np.abs(right).sum())
        assert abs(left.sum() - right.sum()) <= bound, (b, left.sum(), right.sum(), bound)
        if b < 4:
            assert abs(left.sum()) > 1e3 * bound                                   # the identity is not 0 == 0


@pytest.mark.parametrize("name", ta.FD_CASES)
def test_finite_differences_in_log_k(name):
    """the chain (direct solve, advance_adjoint, adjoint solve, mass sensitivity) against central differences of the oracle's
    direct solve plus the forward twin along a random direction in log k, h = 1e-5, the seeds on the curve, on stored and on c
    separately.  A column is left out only if a step count or a sign of g changed between k exp(+-h dk)."""
    worst = 0.0
    for combo in (("curve_bar",), ("stored_bar",), ("c_bar",)):
        checks = [ta.fd_check(name, b, combo) for b in range(4)]
        assert sum(not kept for _, kept in checks) <= 1
        worst = max([worst] + [rel for rel, kept in checks if kept])
    print(f"{name}: largest relative difference from central differences {worst:.3g} (FD_RAW {ta.FD_RAW:.3g})")
    assert worst <= 10 * ta.FD_RAW


def test_recorded_tolerances():
    """ADJ_ROUNDING_RAW and GRAD_PERTURBATION_RAW of transport_adjoint_cases.py are what their method measures: not below
    it, and not more than 4 x above"""
    rounding = max(ta.rounding_deviation(n) for n in ta.NAMES)
    change = max(ta.gradient_perturbation_change(name, b, ("curve_bar", "stored_bar"), wrt_log)
                 for name, _ in ta.GRAD_CASES[:3] for wrt_log in (False, True) for b in range(4))
    print(f"float64 vs long double twin {rounding:.3g}; gradient in k under a 1e-9 flux perturbation {change:.3g}")
    assert ta.ADJ_ROUNDING_RAW / 4 <= rounding <= ta.ADJ_ROUNDING_RAW
    assert ta.GRAD_PERTURBATION_RAW / 4 <= change <= ta.GRAD_PERTURBATION_RAW
    assert ta.TOL_KA == 16 * ta.ADJ_ROUNDING_RAW and ta.TOL_G == 10 * ta.GRAD_PERTURBATION_RAW


@pytest.mark.parametrize("name", ["hex1", "quad0", "tri1", "agg2_1"])
def test_sigma_flip_invariance(name):
    """On a divergence-free flux out_e == in_e up to rounding, and exactly on some elements.  Forcing the other branch of r_e
    on every exactly tied element changes u_bar by -+ w_e P_e B[e, :]^T: in the range of B^T (projection residual at
    rounding, on the dofs that are not essential - an essential dof of zero flux has g == 0 and takes no part), and the
    gradient in k does not change: the adjoint solve maps the range of B^T to lam_u = 0."""
    c = tc.case(name)
    dp = tc.problem(c.kind)
    L = dp.levels[c.level]
    free = ~L.ess_mask.astype(bool)
    Bt = sp.csr_matrix(L.B).T.tocsr()[free].toarray()
    for b in range(4):
        g0, r0 = ta.chain_gradient(name, b, ("curve_bar", "stored_bar"), True)
        n, sgn, sigma = r0["decisions"][0]
        tied = r0["tied"][0]
        assert tied.sum() >= 1
        g1, r1 = ta.chain_gradient(name, b, ("curve_bar", "stored_bar"), True, decisions=[(n, sgn, sigma ^ tied)])
        diff = (r1["u_bar"][0] - r0["u_bar"][0])[free]
        scale = np.abs(r0["u_bar"][0]).max()
        assert np.abs(diff).max() > 1e3 * ta.TOL_KA * scale                      # u_bar itself does change
        y = np.linalg.lstsq(Bt, diff, rcond=None)[0]
        resid = np.abs(Bt @ y - diff).max()
        assert resid <= ta.TOL_KA * scale, (b, resid / scale)
        # the gradient in k, relative to its largest entry, at the rounding scale the kernel is held to (seen: at most 2.2e-14,
        # tri1, while u_bar changes by 0.4 to 0.98 of its largest entry and the residual stays below 3.4e-15)
        assert np.abs(g1 - g0).max() <= ta.TOL_KA * np.abs(g0).max(), (b, np.abs(g1 - g0).max() / np.abs(g0).max())


@pytest.mark.parametrize("name", ["quad1", "hex1", "agg2_2"])
def test_checkpoint_independence(name):
    c, r = tc.case(name), ta.twin(name)
    sd = ta.seeds(name, ta.SEED_NAMES)
    for K in (1, 2, int(r["nsteps"].max())):
        s = tw.advance_adjoint(c.mesh, c.u, c.t_end, tc.CFL, ta.NREPORT, **sd, segment=K)
        for key in ("u_bar", "c0_bar", "c", "curve", "stored"):
            assert np.array_equal(s[key], r[key]), (K, key)


def test_columns_that_are_not_differentiated():
    c = tc.case("hex1")
    sd = ta.seeds("hex1", ta.SEED_NAMES)
    clean = ta.twin("hex1")
    u = c.u.copy()
    u[1, 7] = np.nan
    r = tw.advance_adjoint(c.mesh, u, c.t_end, tc.CFL, ta.NREPORT, **sd)
    assert r["status"][1] == tw.BAD_FLUX and r["nsteps"][1] == 0 and r["decisions"][1] is None
    assert (r["u_bar"][1] == 0).all() and (r["c0_bar"][1] == 0).all()
    for b in (0, 2, 3, 4):
        assert np.array_equal(r["u_bar"][b], clean["u_bar"][b]) and np.array_equal(r["c0_bar"][b], clean["c0_bar"][b])
    r = tw.advance_adjoint(c.mesh, c.u, c.t_end, tc.CFL, ta.NREPORT, **sd, max_steps=20)
    f = tw.advance(c.mesh, c.u, c.t_end, tc.CFL, ta.NREPORT, max_steps=20)
    lim = r["status"] == tw.STEP_LIMIT
    assert lim.sum() == 2 and np.array_equal(r["status"], f["status"]) and np.array_equal(r["curve"], f["curve"])
    assert (r["u_bar"][lim] == 0).all() and (r["c0_bar"][lim] == 0).all()
    assert np.array_equal(r["u_bar"][~lim], clean["u_bar"][~lim])
    t = tw.advance_tangent(c.mesh, c.u, np.ones_like(c.u), c.t_end, tc.CFL, ta.NREPORT, max_steps=20)
    assert (t["dcurve"][lim] == 0).all() and (t["dstored"][lim] == 0).all() and (t["dc"][lim] == 0).all()


def test_refusals():
    c = tc.case("quad1")
    sd = ta.seeds("quad1", ta.SEED_NAMES)
    args = (c.mesh, c.u, c.t_end, tc.CFL, ta.NREPORT)
    for bad in (dict(), dict(curve_bar=sd["curve_bar"][:, :3]), dict(stored_bar=sd["stored_bar"][:4]),
                dict(c_bar=sd["c_bar"][:, 1:]), dict(sd, segment=0), dict(sd, decisions=[None]), dict(sd, max_steps=-1)):
        with pytest.raises(ValueError):
            tw.advance_adjoint(*args, **bad)
    for bad_args in ((c.mesh, None) + args[2:], (c.mesh, c.u[:, :-1]) + args[2:], (c.mesh, c.u, 0.0) + args[3:],
                     (c.mesh, c.u, c.t_end, 1.5, ta.NREPORT), (c.mesh, c.u, c.t_end, tc.CFL, 0)):
        with pytest.raises(ValueError):
            tw.advance_adjoint(*bad_args, **sd)
    with pytest.raises(ValueError):
        tw.advance_tangent(c.mesh, c.u, c.u[:3], c.t_end, tc.CFL, ta.NREPORT)
    with pytest.raises(ValueError):
        tw.advance_tangent(c.mesh, c.u, None, c.t_end, tc.CFL, ta.NREPORT)
    assert tw.advance_adjoint(*args, stored_bar=sd["stored_bar"])["u_bar"].shape == (5, c.mesh.n_face)      # one seed is enough

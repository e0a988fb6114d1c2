"""The tangent and the adjoint of the particle tracer's numpy twin (fe.tracer.trace_tangent / trace_adjoint; DESIGN.md section
25): forward bits, the adjoint identity, finite differences in the flux, in the start points and through the Darcy chain, the
long-double reference, particles that do not exit, the seed of the reduction, and the text of the header.  No GPU."""
import os
import re

import numpy as np
import pytest

import tracer_adjoint_cases as ta
import tracer_cases as tc
from conftest import ROOT
from parelagmc_amd.fe import tracer as tr

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", ta.NAMES)
def test_forward_outputs_are_those_of_trace(name):
    c = ta.case(name)
    fwd, adj = tr.trace(c.mesh, ta.flux(name), c.x0, c.elem0), ta.twin(name)
    for key in ta.FWD_KEYS + ("x_exit",):
        assert np.array_equal(fwd[key], adj[key]), key
    one = tr.trace_adjoint(c.mesh, ta.flux(name)[2], c.x0, c.elem0, **ta.seeds(name, ta.BOTH, 2))       # a one-dimensional u
    assert all(np.array_equal(one[key], adj[key][2]) for key in ta.FWD_KEYS + ("x_exit", "u_bar", "x0_bar"))


@pytest.mark.parametrize("name", ta.NAMES)
def test_adjoint_identity(name):
    """<tangent(du, dx0), seeds> = <du, u_bar> + <dx0, x0_bar> within 64 eps of the sum of the absolute terms"""
    c, u = ta.case(name), ta.flux(name)
    rng = np.random.Generator(np.random.PCG64(5 + ta.NAMES.index(name)))
    du, dx0 = u * rng.standard_normal(u.shape), 1e-2 * rng.standard_normal(c.x0.shape)
    tan = tr.trace_tangent(c.mesh, u, du, c.x0, c.elem0, dx0=dx0)
    zT, zx = np.zeros_like(tan["dT"]), np.zeros_like(tan["dx_exit"])
    for combo in ta.COMBOS:
        sd = ta.seeds(name, combo)
        Tb, xb = sd.get("T_bar", zT), sd.get("x_exit_bar", zx)
        adj = ta.twin(name, combo)
        lhs_terms = np.concatenate([(tan["dT"] * Tb).reshape(4, -1), (tan["dx_exit"] * xb).reshape(4, -1)], axis=1)
        rhs_terms = np.concatenate([du * adj["u_bar"], (dx0[None] * adj["x0_bar"]).reshape(4, -1)], axis=1)
        lhs, rhs = lhs_terms.sum(axis=1), rhs_terms.sum(axis=1)
        bound = 64 * EPS * (np.abs(lhs_terms).sum(axis=1) + np.abs(rhs_terms).sum(axis=1))
        assert (np.abs(lhs) > 0).all() and (np.abs(lhs - rhs) <= bound).all(), (combo, lhs, rhs, bound)


@pytest.mark.parametrize("name", ta.NAMES)
def test_tangent_against_central_differences(name):
    dT, dx = ta.tangent_fd(name)
    print(f"{name}: tangent differs from central differences (h = {ta.FD_STEP:g}) by {dT:.3g} (T), {dx:.3g} (x_exit) of the "
          f"largest derivative (tolerance {10 * ta.TANGENT_FD_RAW:.3g})")
    assert max(dT, dx) <= 10 * ta.TANGENT_FD_RAW


@pytest.mark.parametrize("name", ta.NAMES)
def test_start_point_adjoint_against_central_differences(name):
    d = ta.start_fd(name)
    print(f"{name}: <x0_bar, dx0> differs from central differences by {d:.3g} (tolerance {10 * ta.START_FD_RAW:.3g})")
    assert d <= 10 * ta.START_FD_RAW


@pytest.mark.parametrize("name", ta.NAMES)
def test_float64_against_long_double(name):
    worst = max(ta.rounding_deviation(name, combo) for combo in ta.COMBOS)
    f64, f80 = ta.twin(name), ta.twin(name, longdouble=True)
    for key in ("status", "exit_face", "nsteps"):
        assert np.array_equal(f64[key], f80[key]), key                   # the float64 decisions
    assert f80["u_bar"].dtype == np.longdouble and np.abs(f64["T"] / f80["T"] - 1).max() <= tc.ROUNDING_RAW
    print(f"{name}: float64 twin differs from the long-double twin by {worst:.3g} (recorded {ta.ADJ_ROUNDING_RAW:.3g})")
    assert worst <= ta.ADJ_ROUNDING_RAW


@pytest.mark.parametrize("name", ta.CHAIN_CASES)
def test_chain_against_central_differences(name):
    worst = max(ta.chain_fd(name, b) for b in range(4))
    print(f"{name}: chain gradient in log k differs from central differences (h = {ta.CHAIN_STEP:g}) by {worst:.3g} "
          f"(tolerance {10 * ta.CHAIN_FD_RAW:.3g})")
    assert worst <= 10 * ta.CHAIN_FD_RAW


def test_recorded_tolerances():
    """the constants of tracer_adjoint_cases.py, re-measured: each holds, and none is more than twice what is measured"""
    lp, ep = ta.derivative_branch_agreement()
    print(f"L' and E' at their switch: {lp:.3g} and {ep:.3g} ulp")
    assert max(lp, ep) <= ta.BRANCH_ULP
    rounding = max(ta.rounding_deviation(n, c) for n in ta.NAMES for c in ta.COMBOS)
    tangent = max(max(ta.tangent_fd(n)) for n in ta.NAMES)
    start = max(ta.start_fd(n) for n in ta.NAMES)
    chain = max(ta.chain_fd(n, b) for n in ta.CHAIN_CASES for b in range(4))
    pert = max(ta.gradient_perturbation_change(n, b, w) for n in ta.CHAIN_CASES for b in range(4) for w in (False, True))
    for what, got, rec in (("rounding", rounding, ta.ADJ_ROUNDING_RAW), ("tangent", tangent, ta.TANGENT_FD_RAW),
                           ("start", start, ta.START_FD_RAW), ("chain", chain, ta.CHAIN_FD_RAW),
                           ("perturbation", pert, ta.GRAD_PERTURBATION_RAW)):
        print(f"{what}: measured {got:.3g}, recorded {rec:.3g}")
        assert rec / 2 <= got <= rec, what
    assert ta.TOL_KT == 16 * ta.ADJ_ROUNDING_RAW and ta.TOL_G == 10 * ta.GRAD_PERTURBATION_RAW


def test_derivative_series_lengths():
    """the truncated tails of the two series at the switch are below 2^-55 of the value; one term fewer would not be"""
    s = tr._DSERIES
    n = tr._LP_TERMS
    assert (n + 1) / (n + 2) * s ** n <= 0.5 * 2.0 ** -55 < n / (n + 1) * s ** (n - 1)
    n = tr._EP_TERMS
    fact = lambda k: float(np.prod(np.arange(1, k + 1, dtype=np.float64)))
    assert (n + 1) / fact(n + 2) * s ** n <= 0.5 * 2.0 ** -55 < n / fact(n + 1) * s ** (n - 1)
    ld = np.longdouble
    for x in (-s / 2, 1e-3, -1e-9, s / 3, np.nextafter(s, 0.0)):       # against 60 terms in long double
        lp = sum(ld((-1) ** k * k) / ld(k + 1) * ld(x) ** (k - 1) for k in range(1, 61))
        ep = sum(ld(k) / ld(fact(k + 1)) * ld(x) ** (k - 1) for k in range(1, 25))
        assert abs(float(tr._Lp(np.float64(x)) / lp - 1)) <= 4 * EPS and abs(float(tr._Ep(np.float64(x)) / ep - 1)) <= 4 * EPS
    assert tr._Lp(np.float64(0.0)) == -0.5 and tr._Ep(np.float64(0.0)) == 0.5


def test_particles_that_do_not_exit():
    for name in ("hex1", "tet1"):
        c, u, free = ta.case(name), ta.flux(name), ta.twin(name)
        cut = int(np.median(free["nsteps"]))
        sd = ta.seeds(name, ta.BOTH)
        r = tr.trace_adjoint(c.mesh, u, c.x0, c.elem0, **sd, max_steps=cut)
        cens = r["status"] != tr.EXITED
        assert cens.any() and (~cens).any() and (r["status"][cens] == tr.MAX_STEPS).all()
        assert (r["x0_bar"][cens] == 0).all()
        assert np.array_equal(r["x0_bar"][~cens], free["x0_bar"][~cens])            # the others are unchanged
        zeroed = tr.trace_adjoint(c.mesh, u, c.x0, c.elem0, sd["T_bar"] * ~cens, sd["x_exit_bar"] * ~cens[:, :, None])
        assert np.array_equal(r["u_bar"], zeroed["u_bar"])                          # the censored ones contribute nothing
        tan = tr.trace_tangent(c.mesh, u, u, c.x0, c.elem0, max_steps=cut)
        assert (tan["dT"][cens] == 0).all() and (tan["dx_exit"][cens] == 0).all()
    # a one-element stagnant box: all fluxes inward
    m = tc.single_box()
    u = -np.ones(6)                                                       # outward = global normal: every face flows in
    r = tr.trace_adjoint(m, u, np.array([[0.3, 0.4, 0.5], [0.5, 0.5, 0.5]]), np.zeros(2, np.int32), np.ones(2), np.ones((2, 3)))
    assert (r["status"] == tr.STAGNANT).all() and (r["u_bar"] == 0).all() and (r["x0_bar"] == 0).all() and (r["T"] == 0).all()


def test_exact_one_step_derivatives():
    """the unit box with v_lo = 1, v_hi = 2 along z: T = ln(2 / v(z0)), v(z) = 1 + z"""
    m = tc.single_box()
    u = np.zeros(6)
    u[0], u[5] = -1.0, 2.0
    z0 = 0.25
    r = tr.trace_adjoint(m, u, np.array([[0.5, 0.5, z0]]), np.zeros(1, np.int32), np.ones(1))
    # T = ln(vhi / v0) / g, g = vhi - vlo, v0 = vlo + g z0; dT/dz0 = -1 / v0
    vlo, vhi = 1.0, 2.0
    g, v0 = vhi - vlo, vlo + (vhi - vlo) * z0
    T = np.log(vhi / v0) / g
    dvhi = (1 / vhi - z0 / v0) / g - T / g
    dvlo = (-(1 - z0) / v0) / g + T / g
    assert abs(r["T"][0] - T) <= 4 * EPS * T
    assert abs(r["x0_bar"][0, 2] + 1 / v0) <= 8 * EPS and (r["x0_bar"][0, :2] == 0).all()
    assert abs(r["u_bar"][5] - dvhi) <= 16 * EPS and abs(r["u_bar"][0] + dvlo) <= 16 * EPS          # u_0 = -v_lo


def test_reduce_seed():
    rng = np.random.Generator(np.random.PCG64(9))
    T = rng.uniform(1.0, 2.0, (3, 17))
    status = np.zeros((3, 17), np.int32)
    status[1, 4] = tr.MAX_STEPS
    T[2, 5] = T[2, 9] = 0.5                                               # a tie: the lower index
    status[0, int(T[0].argmin())] = tr.STAGNANT                           # the minimum did not exit
    mean = tr.reduce_seed(T, status, tr.MEAN)
    exited = status == tr.EXITED
    assert (mean[exited] == 1 / 17).all() and (mean[~exited] == 0).all()
    # against a finite difference of reduce (linear in T): on the particles that exited
    h = 1e-3
    dT = rng.standard_normal(T.shape) * exited
    fd = (tr.reduce(T + h * dT, status)[0] - tr.reduce(T - h * dT, status)[0]) / (2 * h)
    assert np.abs(fd - (mean * dT).sum(axis=1)).max() <= 1e-12
    mn = tr.reduce_seed(T, status, tr.MIN)
    assert mn[2, 5] == 1 and mn[2].sum() == 1 and mn[0].sum() == 0 and mn[1, int(T[1].argmin())] == 1 and mn[1].sum() == 1
    fd = (tr.reduce(T + h * mn, status, tr.MIN)[0] - tr.reduce(T - h * mn, status, tr.MIN)[0]) / (2 * h)
    assert abs(fd[1] - 1) <= 1e-12                                         # away from a tie the minimum moves with its particle


def test_refusals_and_header_text():
    c = ta.case("hex1")
    with pytest.raises(ValueError):
        tr.trace_adjoint(c.mesh, ta.flux("hex1"), c.x0, c.elem0, np.zeros((3, len(c.x0))))        # a seed of another shape
    text = open(os.path.join(ROOT, "include", "pmc.h")).read()
    for fn in ("pmc_tracer_run_adjoint", "pmc_tracer_reduce_seed", "pmc_tracer_set_adjoint_scratch", "pmc_tracer_adjoint_chunks",
               "pmc_darcy_tracer_gradient", "pmc_darcy_tracer_loglik_gradient"):
        assert len(re.findall(r"\bint " + fn + r"\(", text)) == 1, fn
    block = text[text.index("The adjoint of the particle tracer"):text.index("MLMC accumulators across GPUs")]
    for phrase in ("ascending (particle index in the caller's order, step)", "from 0.0", "both seeds NULL", "ld or ld_bar < n_face",
                   "nbatch < 1", "a bad memspace", "noise <= 0", "created on another device", "not_exited[b] > 0",
                   "is not differentiated", "DESIGN.md section 25", "pmc_tracer_run bit for"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", block), phrase
    from parelagmc_amd import capi
    for fn in ("pmc_tracer_run_adjoint", "pmc_tracer_reduce_seed", "pmc_darcy_tracer_gradient", "pmc_darcy_tracer_loglik_gradient"):
        assert fn in capi.SYMBOLS
    assert all(hasattr(capi.Tracer, m) for m in ("run_adjoint", "reduce_seed")) and all(
        hasattr(capi.DarcySolver, m) for m in ("tracer_gradient", "tracer_loglik_gradient"))
    hpp = open(os.path.join(ROOT, "parelagmc_amd", "host", "parelagmc.hpp")).read()
    for m in ("RunAdjoint(const Vector& u, const double* T_bar", "SolveFwd_TracerGradient", "ComputeGradTravelTimeLogLikelihood"):
        assert m in hpp, m

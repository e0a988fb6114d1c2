"""Numpy twin of BayesianInverseProblem::ComputeMAP / pmc_bayes_map (host/host.cpp, csrc/newton_cg.hip; DESIGN.md section
19): batched MAP estimation by inexact Gauss-Newton-CG with Armijo backtracking.  The reference has no optimiser; the twin
restates the library's loop decision for decision, so that the integer trajectory (outer iterations, CG steps per
iteration, accepted steps) of the two can be compared - and it returns, for every decision it takes, the relative margin to
the other branch, so that a comparison can be restricted to cases no rounding error decides.

    map_newton_cg(logpost_grad, hessvec, xi0, **opts)      over callables on whole batches
    map_estimate(sampler_problem, darcy_problem, ...)       over sampler_adjoint.logpost_gradient / logpost_gn_hessvec
"""
from __future__ import annotations

import numpy as np

from . import sampler_adjoint

CONVERGED, MAX_NEWTON, LINE_SEARCH_FAILED, NON_FINITE = range(4)
_RUNNING = -1

DEFAULTS = dict(max_newton=50, max_cg=100, max_backtracks=10, eta_max=0.5, c1=1e-4, grad_atol=0.0, grad_rtol=1e-4)


def _check_opts(o):
    if o["max_newton"] <= 0 or o["max_cg"] <= 0 or o["max_backtracks"] <= 0 or not o["grad_rtol"] > 0 or not o["grad_atol"] >= 0 \
            or not 0 < o["eta_max"] < 1 or not 0 < o["c1"] < 1:
        raise ValueError("max_newton, max_cg, max_backtracks and grad_rtol must be positive, eta_max and c1 inside (0, 1), "
                         "grad_atol not negative")


def cg_columns(hessvec, g, eta, active, max_cg, margins=None):
    """The pmc_ncg loop: CG on H d = g per column from d = 0, ended per column at <r, r> <= (eta |g|)^2, on <p, Hp> <= 0 (d kept,
    or d = g at the first step) or after max_cg steps; hessvec(P) maps the whole batch of search directions, finished and
    inactive columns entering as zeros.  Returns (d, count, npc)."""
    nb, n = g.shape
    d, r, p = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
    rr, tol2 = np.zeros(nb), np.zeros(nb)
    count, npc = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    done = np.ones(nb, bool)
    for b in range(nb):
        if active[b]:
            r[b], p[b] = g[b], g[b]
            rr[b] = float(g[b] @ g[b])
            tol2[b] = eta[b] * eta[b] * rr[b]
            done[b] = not rr[b] > 0.0
    for _ in range(max_cg):
        if done.all():
            break
        hp = hessvec(p)
        for b in range(nb):
            if done[b]:
                continue
            php = float(p[b] @ hp[b])
            count[b] += 1
            if not php > 0.0:
                if count[b] == 1:
                    d[b] = p[b]
                npc[b], done[b] = 1, True
                p[b] = 0.0
                continue
            alpha = rr[b] / php
            d[b] = d[b] + alpha * p[b]
            r[b] = r[b] - alpha * hp[b]
            rr_new = float(r[b] @ r[b])
            if margins is not None and tol2[b] > 0.0:
                margins.append(abs(np.sqrt(rr_new) - np.sqrt(tol2[b])) / np.sqrt(tol2[b]))
            if not rr_new > tol2[b]:
                done[b] = True
                p[b] = 0.0
            else:
                p[b] = r[b] + (rr_new / rr[b]) * p[b]
            rr[b] = rr_new
    return d, count, npc


def map_newton_cg(logpost_grad, hessvec, xi0, **opts):
    """logpost_grad(X) -> (logpost (nb,), grad (nb, n)) and hessvec(X, V) -> (nb, n) act on whole batches (nb, n), as
    pmc_bayes_logpost_gradient and pmc_bayes_logpost_gn_hessvec do.  Returns (xi, result): result holds the per-column
    arrays and histories of pmc_map_result under the same names, plus
        hist_gd         <g, d> of the direction taken from iterate i
        cg_margins      | |r| - eta |g| | / (eta |g|) of every tolerance test taken
        armijo_margins  |logpost(xi + t d) - logpost(xi) - c1 t <g, d>| / |logpost(xi)| of every Armijo test taken
        conv_margins    | |g| - tol | / tol of every convergence test taken
    - the relative distance of each decision to its other branch."""
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise TypeError(f"unknown MAP option {k!r}")
        o[k] = v
    _check_opts(o)
    xi = np.array(np.atleast_2d(xi0), np.float64)
    nb, n = xi.shape
    rows = o["max_newton"] + 1
    status = np.full(nb, _RUNNING, np.int32)
    iters, nhess, ngrad, nnpc = (np.zeros(nb, np.int32) for _ in range(4))
    hist_lp, hist_gn, hist_t = (np.full((rows, nb), np.nan) for _ in range(3))
    hist_cg = np.full((rows, nb), -1, np.int32)
    hist_gd = np.full((rows, nb), np.nan)
    cg_m, arm_m, conv_m = [], [], []

    lp, g = logpost_grad(xi)
    lp, g = np.array(lp, np.float64), np.array(g, np.float64)
    ngrad[:] = 1
    gn = np.sqrt(np.einsum("ij,ij->i", g, g))
    lp0, gn0 = lp.copy(), gn.copy()
    status[~(np.isfinite(lp) & np.isfinite(gn))] = NON_FINITE
    it = 0
    while True:
        for b in range(nb):
            if status[b] != _RUNNING:
                continue
            tol = max(o["grad_rtol"] * gn0[b], o["grad_atol"])
            if tol > 0.0:
                conv_m.append(abs(gn[b] - tol) / tol)
            if gn[b] <= tol:
                status[b] = CONVERGED
            elif it == o["max_newton"]:
                status[b] = MAX_NEWTON
            hist_lp[it, b], hist_gn[it, b], hist_cg[it, b], hist_t[it, b] = lp[b], gn[b], 0, 0.0
        mask = status == _RUNNING
        if not mask.any():
            break
        eta = np.where(mask, np.minimum(o["eta_max"], np.sqrt(gn / np.where(gn0 > 0, gn0, 1.0))), 0.0)
        d, cgc, npc = cg_columns(lambda P: hessvec(xi, P), g, eta, mask, o["max_cg"], cg_m)
        nhess[mask] += cgc[mask]
        nnpc[mask] += npc[mask]
        gd = np.einsum("ij,ij->i", g, d)
        t = np.where(mask, 1.0, 0.0)
        searching, accepted = mask.copy(), np.zeros(nb, bool)
        for ls in range(o["max_backtracks"] + 1):
            trial = np.where((t != 0.0)[:, None], xi + t[:, None] * d, xi)
            lpt, gt = logpost_grad(trial)
            ngrad[mask] += 1
            again = False
            for b in range(nb):
                if not searching[b]:
                    continue
                if np.isfinite(lpt[b]):
                    arm_m.append(abs(lpt[b] - lp[b] - o["c1"] * t[b] * gd[b]) / abs(lp[b]) if lp[b] != 0 else np.inf)
                if np.isfinite(lpt[b]) and lpt[b] >= lp[b] + o["c1"] * t[b] * gd[b]:
                    searching[b], accepted[b] = False, True
                elif ls == o["max_backtracks"]:
                    searching[b] = False
                else:
                    t[b] *= 0.5
                    again = True
            if not again:
                break
        for b in range(nb):
            if not mask[b]:
                continue
            hist_cg[it, b], hist_gd[it, b] = cgc[b], gd[b]
            if accepted[b]:
                xi[b], g[b], lp[b] = trial[b], gt[b], lpt[b]
                gn[b] = np.sqrt(float(g[b] @ g[b]))
                iters[b] += 1
                hist_t[it, b] = t[b]
                if not np.isfinite(gn[b]):
                    status[b] = NON_FINITE
            else:
                status[b] = LINE_SEARCH_FAILED
        it += 1
    res = dict(status=status, newton_iterations=iters, hessian_actions=nhess, gradient_evaluations=ngrad,
               nonpos_curvature=nnpc, logpost0=lp0, logpost=lp, grad_norm0=gn0, grad_norm=gn, hist_logpost=hist_lp,
               hist_grad_norm=hist_gn, hist_cg=hist_cg, hist_t=hist_t, hist_gd=hist_gd, cg_margins=np.array(cg_m),
               armijo_margins=np.array(arm_m), conv_margins=np.array(conv_m))
    return xi, res


def map_estimate(sampler_problem, darcy_problem, level, xi0, Gobs, data, noise, xi_level=None, projection=None, conditioner=None,
                 **opts):
    """map_newton_cg over the twins of the library's two entries, with direct solves: logpost_gradient and
    logpost_gn_hessvec of sampler_adjoint, column by column (Gobs: the observation functionals, data: the observed values).
    conditioner: an fe.condition.Conditioner with exact data - the MAP point of the conditional prior."""
    cache = {}

    def logpost_grad(X):
        out = [sampler_adjoint.logpost_gradient(sampler_problem, darcy_problem, level, x, Gobs, data, noise, xi_level,
                                                projection, cache, conditioner) for x in X]
        return np.array([a for a, _ in out]), np.array([g for _, g in out])

    def hessvec(X, V):
        return np.array([sampler_adjoint.logpost_gn_hessvec(sampler_problem, darcy_problem, level, x, v, Gobs, noise, xi_level,
                                                            projection, cache, conditioner) if np.any(v) else np.zeros_like(v)
                         for x, v in zip(X, V)])

    return map_newton_cg(logpost_grad, hessvec, xi0, **opts)

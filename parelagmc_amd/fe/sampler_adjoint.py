"""Adjoint of the samplers' Eval in the white noise, in numpy / scipy with sparse direct solves: the twin of
pmc_sampler_eval_adjoint (csrc/sampler_adjoint.hip, csrc/kl_adjoint.hip) and of the log-posterior gradient of the host layer
(BayesianInverseProblem::ComputeGradLogPosterior), DESIGN.md section 17.  The reference has no gradients; everything here
follows from the level data of a SamplerProblem / KLProblem alone.

Eval(level, xi_level) of an SPDE sampler is s_out = f(O S R D xi):

    D = -g diag(sqrt(w[xi_level])),     R = P[level-1]^T ... P[xi_level]^T,     S = the s-block of [M B^T; B -alpha W]^-1
    O = the output map (identity | the gather idx | diag(inv_w) Gt),            f = exp (lognormal) or the identity.

The block operator is symmetric, so S is, and for v = dJ/ds_out

    dJ/dxi = D R^T S O^T (v o f'),      f' = s_out (lognormal) or 1.

Eval of a KL sampler is s = f(Phi_level Lambda^1/2 xi[:m]); its adjoint is (Phi_level Lambda^1/2)^T (v o f') in the first m
entries and zero in the others.

Second order: the tangent of Eval is ds_out = f' o (L v) with L = O S R D the linear part (Eval of v
without exp), and the Gauss-Newton Hessian of -log pi is H_GN v = v + L^T J^T (1/noise) J L v (in log k on a lognormal
problem): pmc_sampler_eval_tangent and BayesianInverseProblem::ApplyGNHessian.

Conditioned fields: every entry takes conditioner=, an fe.condition.Conditioner with exact data built
on the same problem.  The Gaussian field g = O S R D xi then becomes g_c = Gamma g + K A^-1 y, Gamma = I - K A^-1 H, before
f: the tangent gains Gamma behind L (Conditioner.apply_tangent), the adjoint Gamma^T in front of L^T
(Conditioner.apply_adjoint, after v o f').  A conditioner excludes a projection, as on the device.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import darcy_adjoint


def _is_kl(problem):
    return hasattr(problem, "evects")


def _check_conditioner(conditioner, projection):
    if conditioner is None:
        return
    if projection is not None:
        raise ValueError("a conditioner and a projection exclude each other")
    if conditioner.noisy:
        raise ValueError("the conditioner must hold exact data (every sigma2 == 0)")


def _block_solver(problem, level, cache):
    if cache is not None and level in cache:
        return cache[level]
    L = problem.levels[level]
    A = sp.bmat([[L.M, L.B.T], [L.B, -problem.alpha * sp.diags(L.w_diag)]], format="csc")
    lu = spla.splu(A)
    if cache is not None:
        cache[level] = lu
    return lu


def output_map_transpose(n_s, projection, q):
    """O^T q on the sampler's own mesh (n_s entries) for q on the output space"""
    if projection is None:
        return np.array(q, dtype=np.float64)
    if projection[0] == "gather":
        out = np.zeros(n_s)
        np.add.at(out, np.asarray(projection[1]), q)
        return out
    if projection[0] == "l2":
        return sp.csr_matrix(projection[1]).T @ (np.asarray(projection[2]) * q)
    raise ValueError(projection[0])


def kl_modes(problem, level):
    """Phi_level Lambda^1/2, n_s(level) x m"""
    return np.asarray(problem.evects[level]) * np.sqrt(problem.evals)[None, :]


def eval_adjoint(problem, level, xi_level, v, s_out=None, projection=None, cache=None, conditioner=None):
    """dJ/dxi (xi_size(xi_level) entries) of one realization for v = dJ/ds_out (sample_size(level) entries).  s_out: None, or
    Eval's output on a lognormal problem (v is multiplied by it).  projection: as SamplerOracle.eval takes it (ignored for a
    KLProblem).  cache: a dict that keeps the factorizations between calls.  conditioner: Eval's field is the conditional one
    (s_out then is the conditional field)."""
    _check_conditioner(conditioner, projection)
    v = np.asarray(v, dtype=np.float64)
    if s_out is not None:
        if not problem.lognormal:
            raise ValueError("s_out given for a problem that is not lognormal")
        v = v * np.asarray(s_out, dtype=np.float64)
    if not 0 <= xi_level <= level < problem.n_mc_levels:
        raise ValueError("need 0 <= xi_level <= level < n_mc_levels")
    if conditioner is not None:
        v = conditioner.apply_adjoint(level, v)[0]
    if _is_kl(problem):
        m = problem.nmodes
        g = np.zeros(problem.levels[xi_level].n_s)
        g[:m] = kl_modes(problem, level).T @ v
        return g
    L = problem.levels[level]
    rhs = np.zeros(L.n_u + L.n_s)
    rhs[L.n_u:] = output_map_transpose(L.n_s, projection, v)
    y = _block_solver(problem, level, cache).solve(rhs)[L.n_u:]           # S q: the operator is symmetric
    for lvl in range(level - 1, xi_level - 1, -1):
        y = problem.levels[lvl].P @ y
    return -problem.matern_g * np.sqrt(problem.levels[xi_level].w_diag) * y


def eval_forward(problem, level, xi_level, xi, projection=None, cache=None, conditioner=None):
    """Eval itself with the same pieces (s_out of one realization): what logpost_gradient differentiates"""
    _check_conditioner(conditioner, projection)
    xi = np.asarray(xi, dtype=np.float64)
    if _is_kl(problem):
        g = kl_modes(problem, level) @ xi[:problem.nmodes]
    else:
        r = -problem.matern_g * np.sqrt(problem.levels[xi_level].w_diag) * xi
        for lvl in range(xi_level, level):
            r = problem.levels[lvl].P.T @ r
        L = problem.levels[level]
        g = _block_solver(problem, level, cache).solve(np.concatenate([np.zeros(L.n_u), r]))[L.n_u:]
        if projection is not None:
            g = g[np.asarray(projection[1])] if projection[0] == "gather" else (projection[1] @ g) * projection[2]
    if conditioner is not None:
        g = conditioner.apply(level, g)[0]
    return np.exp(g) if problem.lognormal else g


def logpost_gradient(sampler_problem, darcy_problem, level, xi, Gobs, data, noise, xi_level=None, projection=None, cache=None,
                     conditioner=None):
    """(logpost, grad) of  log pi(xi) = loglik(k) - |xi|^2 / 2,  k = Eval(level, xi),
    loglik = -|G(k) - data|^2 / (2 noise)  (darcy_adjoint.loglik_gradient).  On a lognormal problem the Darcy gradient is
    taken with respect to log k, which already carries the factor k of the exp chain."""
    xi = np.asarray(xi, dtype=np.float64)
    xi_level = level if xi_level is None else xi_level
    k = eval_forward(sampler_problem, level, xi_level, xi, projection, cache, conditioner)
    logn = bool(sampler_problem.lognormal)
    loglik, _, gk = darcy_adjoint.loglik_gradient(darcy_problem, level, k, Gobs, data, noise, wrt_log=logn)
    grad = -xi + eval_adjoint(sampler_problem, level, xi_level, gk, None, projection, cache, conditioner)
    return loglik - 0.5 * float(xi @ xi), grad


def eval_tangent(problem, level, xi_level, v, s_out=None, projection=None, cache=None, conditioner=None):
    """ds_out = (d Eval / d xi) v of one realization: L v, the Gaussian part of Eval applied to v (no exp), times s_out when
    given (Eval's output on a lognormal problem: the f' of the exp).  <eval_tangent(v), u> = <v, eval_adjoint(u)>."""
    _check_conditioner(conditioner, projection)
    if s_out is not None and not problem.lognormal:
        raise ValueError("s_out given for a problem that is not lognormal")
    if not 0 <= xi_level <= level < problem.n_mc_levels:
        raise ValueError("need 0 <= xi_level <= level < n_mc_levels")
    v = np.asarray(v, dtype=np.float64)
    if _is_kl(problem):
        g = kl_modes(problem, level) @ v[:problem.nmodes]
    else:
        r = -problem.matern_g * np.sqrt(problem.levels[xi_level].w_diag) * v
        for lvl in range(xi_level, level):
            r = problem.levels[lvl].P.T @ r
        L = problem.levels[level]
        g = _block_solver(problem, level, cache).solve(np.concatenate([np.zeros(L.n_u), r]))[L.n_u:]
        if projection is not None:
            g = g[np.asarray(projection[1])] if projection[0] == "gather" else (projection[1] @ g) * projection[2]
    if conditioner is not None:
        g = conditioner.apply_tangent(level, g)[0]
    return g if s_out is None else g * np.asarray(s_out, dtype=np.float64)


def logpost_gn_hessvec(sampler_problem, darcy_problem, level, xi, v, Gobs, noise, xi_level=None, projection=None, cache=None,
                       conditioner=None):
    """H_GN v = v + (dk/dxi)^T J^T (1/noise) J (dk/dxi) v of -log pi at xi (logpost_gradient's log pi): symmetric positive
    definite, the full Hessian where G(k) = data.  On a lognormal problem the chain runs in log k (wrt_log, no s_out), as
    logpost_gradient chains the first derivatives; on a Gaussian one k is the field itself."""
    xi = np.asarray(xi, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    xi_level = level if xi_level is None else xi_level
    k = eval_forward(sampler_problem, level, xi_level, xi, projection, cache, conditioner)
    logn = bool(sampler_problem.lognormal)
    dk = eval_tangent(sampler_problem, level, xi_level, v, None, projection, cache, conditioner)
    hk = darcy_adjoint.gn_hessvec(darcy_problem, level, k, dk, Gobs, noise, wrt_log=logn)
    return v + eval_adjoint(sampler_problem, level, xi_level, hk, None, projection, cache, conditioner)

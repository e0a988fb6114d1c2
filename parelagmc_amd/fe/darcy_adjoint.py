"""Adjoint gradients of the mixed Darcy solve with respect to the permeability field, in numpy / scipy with sparse direct
solves: the twin of pmc_darcy_mass_sensitivity / _solve_gradient / _loglik_gradient (csrc/darcy_gradient.hip, DESIGN.md
section 16) and of pmc_darcy_mass_tangent / _gn_hessvec (csrc/darcy_hessian.hip, section 18).  The reference has no
derivatives; everything here follows from the level data of a DarcyProblem alone.

With the essential rows and columns of A(k) = [M(k) B^T; B 0] eliminated (unit diagonal, the essential values in the
right-hand side) the system stays symmetric, so for a functional J(x)

    A(k) x = rhs_bc,        A(k) lam = dJ/dx  (essential rows zero),
    dJ/dc_e = -lam_u^T M_e x_u,        dJ/dk_e = c'(k_e) dJ/dc_e,    c = 1/k (k_divides) or c = k.

x_u holds the essential values and lam_u vanishes on the essential rows, so the derivative of the eliminated right-hand side
-M(k)[:, ess] ess_data is part of the same bilinear form.  M_e is the unit-coefficient element matrix of the level's
contribution lists.

Second order (Gauss-Newton): for a direction dk the coefficient changes by dc_e = c'(k_e) dk_e and the solution by dx with

    A(k) dx = t,    t_u[f] = -sum_{e has f} dc_e sum_a' M_e[a(f), a'] x_u[f_e(a')]  (0 on the essential rows),   t_p = 0,

so J dk = dG with dG_i = <g_i, dp> / sum(g_i), and J^T (1/noise) J dk = mass_sensitivity(k, x, lam) with
A(k) lam = [0; (1/noise) sum_i dG_i g_i / sum(g_i)]: the Hessian of the NEGATIVE log-likelihood where the misfit vanishes.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def element_matrices(level):
    """(faces, Me) of a DarcyLevel from its contribution lists: faces (n_p, n_fe) int32 - the faces of every element in
    ascending order, the rows whose diagonal entry the element contributes to - and Me (n_p, n_fe, n_fe), the dense
    unit-coefficient element matrices on those faces.  An element with fewer than n_fe faces repeats its first face with
    zero rows and columns."""
    L = level
    pat = L.M_pattern.tocsr()
    nnz = pat.indices.size
    rows = np.repeat(np.arange(L.n_u), np.diff(pat.indptr))
    cols = pat.indices
    cnt = np.diff(L.c_ptr)
    t_row = np.repeat(rows, cnt)
    t_col = np.repeat(cols, cnt)
    assert t_row.size == L.c_elem.size and nnz + 1 == L.c_ptr.size
    diag = t_row == t_col
    order = np.lexsort((t_row[diag], L.c_elem[diag]))
    de, df = L.c_elem[diag][order], t_row[diag][order]
    keep = np.ones(de.size, bool)
    keep[1:] = (de[1:] != de[:-1]) | (df[1:] != df[:-1])
    de, df = de[keep], df[keep]
    nf = np.bincount(de, minlength=L.n_p)
    assert nf.min() >= 1, "an element contributes to no diagonal entry of M"
    n_fe = int(nf.max())
    start = np.concatenate([[0], np.cumsum(nf)])
    faces = np.empty((L.n_p, n_fe), np.int32)
    local = np.arange(de.size) - start[de]
    faces[:] = df[start[:-1]][:, None]
    faces[de, local] = df
    # local index of every contribution's row and column inside its element
    key = de.astype(np.int64) * L.n_u + df
    pos_r = np.searchsorted(key, L.c_elem.astype(np.int64) * L.n_u + t_row)
    pos_c = np.searchsorted(key, L.c_elem.astype(np.int64) * L.n_u + t_col)
    assert np.all(key[pos_r] == L.c_elem.astype(np.int64) * L.n_u + t_row)
    assert np.all(key[pos_c] == L.c_elem.astype(np.int64) * L.n_u + t_col)
    Me = np.zeros((L.n_p, n_fe, n_fe))
    np.add.at(Me, (L.c_elem, local[pos_r], local[pos_c]), L.c_val)
    return faces, Me


def _minus_dc(k, k_divides, wrt_log):
    """-c'(k), times k for the gradient with respect to log k"""
    f = 1.0 / (k * k) if k_divides else -np.ones_like(k)
    return f * k if wrt_log else f


def mass_sensitivity(level, k, x, lam, k_divides, wrt_log=False, return_abs=False, dtype=np.float64):
    """g_e = -c'(k_e) lam_u^T M_e x_u for full vectors x, lam of n_u + n_p entries (one realization, or rows of 2-D arrays).
    return_abs: also sum |c'| |lam_a M_aa' x_a'| per element (the scale of a summation error bound).  dtype: the precision
    the sums are formed in (np.longdouble: a reference whose own rounding does not count against such a bound)."""
    faces, Me = element_matrices(level)
    Me = Me.astype(dtype)
    k, x, lam = (np.atleast_2d(np.asarray(a, dtype=dtype)) for a in (k, x, lam))
    xu, lu = x[:, faces], lam[:, faces]                       # (nb, n_p, n_fe)
    f = _minus_dc(k, k_divides, wrt_log)
    g = f * np.einsum("bea,eac,bec->be", lu, Me, xu)
    if return_abs:
        return g, np.abs(f) * np.einsum("bea,eac,bec->be", np.abs(lu), np.abs(Me), np.abs(xu))
    return g


def assemble(problem, level, k):
    """(A, rhs_bc, ess) of the eliminated system: essential rows and columns replaced by the identity, the essential values
    moved to the right-hand side."""
    L = problem.levels[level]
    k = np.asarray(k, dtype=np.float64)
    c = (1.0 / k) if problem.k_divides else k
    full = np.flatnonzero(np.diff(L.c_ptr) > 0)                 # entries with an empty list are stored zeros
    data = np.zeros(len(L.c_ptr) - 1)
    data[full] = np.add.reduceat(c[L.c_elem] * L.c_val, L.c_ptr[:-1][full])
    M = sp.csr_matrix((data, L.M_pattern.indices, L.M_pattern.indptr), shape=L.M_pattern.shape)
    A = sp.bmat([[M, L.B.T], [L.B, None]], format="csr")
    n = L.n_u + L.n_p
    ess = np.zeros(n, bool)
    ess[:L.n_u] = L.ess_mask.astype(bool)
    d = np.zeros(n)
    d[:L.n_u] = np.where(ess[:L.n_u], L.ess_data, 0.0)
    rhs = L.rhs - A @ d
    rhs[ess] = d[ess]
    keep = sp.diags((~ess).astype(np.float64))
    return (keep @ A @ keep + sp.diags(ess.astype(np.float64))).tocsc(), rhs, ess


def gradient(problem, level, k, adj_rhs=None, wrt_log=False, return_all=False):
    """dJ/dk (or dJ/dlog k) of J = <adj_rhs, x> - adj_rhs None: the level's obs, J = Q - for one realization k by two direct
    solves.  return_all: (grad, Q, x, lam)."""
    L = problem.levels[level]
    A, rhs, ess = assemble(problem, level, k)
    lu = spla.splu(A)
    x = lu.solve(rhs)
    b = np.array(L.obs if adj_rhs is None else adj_rhs, dtype=np.float64)
    b[ess] = 0.0
    lam = lu.solve(b)                                         # A is symmetric
    g = mass_sensitivity(L, k, x, lam, problem.k_divides, wrt_log)[0]
    if return_all:
        return g, float(L.obs @ x), x, lam
    return g


def loglik_gradient(problem, level, k, Gobs, data, noise, wrt_log=False):
    """(loglik, G, grad) of loglik = -|G(k) - data|^2 / (2 noise), G_i = <g_i, p> / sum(g_i) with g_i the rows of Gobs
    (nobs x n_p)."""
    L = problem.levels[level]
    A, rhs, ess = assemble(problem, level, k)
    lu = spla.splu(A)
    x = lu.solve(rhs)
    Gobs = sp.csr_matrix(Gobs)
    norm = 1.0 / np.asarray(Gobs.sum(axis=1)).ravel()
    G = norm * (Gobs @ x[L.n_u:])
    r = G - np.asarray(data, dtype=np.float64)
    loglik = (-1.0 / (noise * 2)) * float(np.sum(r * r))
    b = np.zeros(L.n_u + L.n_p)
    b[L.n_u:] = -(1.0 / noise) * (Gobs.T @ (norm * r))
    lam = lu.solve(b)
    return loglik, G, mass_sensitivity(L, k, x, lam, problem.k_divides, wrt_log)[0]


def mass_tangent(level, k, x, dk, k_divides, wrt_log=False, return_abs=False, dtype=np.float64):
    """t = -dA/dk[dk] x on the free u-rows (0 on the essential rows and on the p-rows) for full vectors x of n_u + n_p
    entries and directions dk of n_p entries (one realization, or rows of 2-D arrays): the transpose of mass_sensitivity in
    the pair (dk, lam), <lam, mass_tangent(dk)> = <dk, mass_sensitivity(lam)> for lam zero on the essential rows.
    return_abs: also sum |dc| |M_aa' x_a'| per row (the scale of a summation error bound).  dtype: the precision the sums
    are formed in."""
    faces, Me = element_matrices(level)
    L = level
    k, x, dk = (np.atleast_2d(np.asarray(a, dtype=dtype)) for a in (k, x, dk))
    ndc = _minus_dc(k, k_divides, wrt_log) * dk                       # -dc, (nb, n_p)
    # an element with fewer than n_fe faces repeats its first face with zero rows: the scatter below adds zeros there
    Me = Me.astype(dtype)
    xu = x[:, faces]                                                  # (nb, n_p, n_fe)
    free = ~L.ess_mask.astype(bool)
    nb, n = x.shape[0], L.n_u + L.n_p

    def scatter(contrib):                                             # (nb, n_p, n_fe) -> (nb, n)
        t = np.zeros((nb, n), dtype=dtype)
        for b in range(nb):
            np.add.at(t[b], faces.ravel(), contrib[b].ravel())
        t[:, :L.n_u] *= free
        return t

    t = scatter(ndc[:, :, None] * np.einsum("eac,bec->bea", Me, xu))
    if return_abs:
        return t, scatter(np.abs(ndc)[:, :, None] * np.einsum("eac,bec->bea", np.abs(Me), np.abs(xu)))
    return t


def _observations(Gobs):
    Gobs = sp.csr_matrix(Gobs)
    return Gobs, 1.0 / np.asarray(Gobs.sum(axis=1)).ravel()


def tangent(problem, level, k, dk, Gobs=None, wrt_log=False, return_all=False):
    """dx = (dx/dk) dk of the forward solution of one realization by two direct solves; with Gobs: dG = J dk instead.
    return_all: (dG or dx, x, dx, lu)."""
    L = problem.levels[level]
    A, rhs, ess = assemble(problem, level, k)
    lu = spla.splu(A)
    x = lu.solve(rhs)
    dx = lu.solve(mass_tangent(L, k, x, dk, problem.k_divides, wrt_log)[0])
    out = dx
    if Gobs is not None:
        Gobs, norm = _observations(Gobs)
        out = norm * (Gobs @ dx[L.n_u:])
    if return_all:
        return out, x, dx, lu
    return out


def gn_hessvec(problem, level, k, dk, Gobs, noise, wrt_log=False, return_all=False):
    """hv = J^T (1/noise) J dk of the negative log-likelihood of loglik_gradient, J = dG/dk (dG/dlog k with wrt_log, dk then
    a direction in log k): symmetric positive semi-definite, the full Hessian where G(k) = data.  return_all: (hv, dG, x)."""
    L = problem.levels[level]
    dG, x, _, lu = tangent(problem, level, k, dk, Gobs, wrt_log, return_all=True)
    Gobs, norm = _observations(Gobs)
    b = np.zeros(L.n_u + L.n_p)
    b[L.n_u:] = (1.0 / noise) * (Gobs.T @ (norm * dG))
    lam = lu.solve(b)
    hv = mass_sensitivity(L, k, x, lam, problem.k_divides, wrt_log)[0]
    if return_all:
        return hv, dG, x
    return hv

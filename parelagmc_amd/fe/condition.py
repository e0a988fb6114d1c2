"""Conditioning of the samplers' Gaussian fields on linear observations (kriging / Matheron's rule): setup algebra and the
numpy twin of the device conditioner (csrc/condition.hip, pmc_conditioner_*).  An extension of this project; the reference
has no counterpart.

With C_l the covariance of the Gaussian field Eval produces on level l and H_l the observation operator of the level,

    g_c = g + K_l A_l^-1 (y + R^1/2 zeta - H_l g),     K_l = C_l H_l^T,     A_l = H_l K_l + R,     R = diag(sigma2),

is a draw of the field conditioned on H_l g + noise = y whenever g is a prior draw and zeta ~ N(0, I) is independent of it.
H_{l+1} = H_l P_l: an observation on a coarser level sees the coarse element(s) that contain it.  The nested P0 levels give
P^T W_l P = W_{l+1}, so C_l does not depend on the level xi was drawn on.

  SPDE samplers (saddle-point and hybridized): C_l = g^2 T_l W_l T_l with T_l the map from the right-hand side of the level's
      system to its s-block (T_l = -S_l^-1, S_l = alpha W_l + B M^-1 B^T); sparse direct solves here.
  KL sampler: C_l = Phi_l Lambda Phi_l^T with the projected, NOT renormalised Phi_l the handle uses.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

MAX_OBS = 512
# A_l counts as positive definite when every Cholesky pivot exceeds this fraction of its diagonal entry (the device setup
# applies the same rule): two exact observations inside one coarse element leave a pivot of rounding size, either sign
PIVOT_RTOL = 1e-12


def check_observations(H0, y, sigma2, n0: int):
    """validated (H0 csr, y, sigma2 or None); the rules pmc_conditioner_create enforces"""
    H0 = sp.csr_matrix(H0, dtype=np.float64)
    H0.sum_duplicates()
    H0.sort_indices()
    nobs = H0.shape[0]
    if not 1 <= nobs <= MAX_OBS:
        raise ValueError(f"conditioner: nobs = {nobs} outside [1, {MAX_OBS}]")
    if H0.shape[1] != n0:
        raise ValueError(f"conditioner: H0 has {H0.shape[1]} columns, level 0 has {n0} elements")
    if np.any(np.diff(H0.indptr) == 0):
        raise ValueError("conditioner: H0 has an empty row")
    y = np.asarray(y, dtype=np.float64).ravel()
    if y.size != nobs or not np.all(np.isfinite(y)):
        raise ValueError("conditioner: y must hold nobs finite values")
    if sigma2 is not None:
        sigma2 = np.asarray(sigma2, dtype=np.float64).ravel()
        if sigma2.size != nobs or not np.all(np.isfinite(sigma2)) or np.any(sigma2 < 0.0):
            raise ValueError("conditioner: sigma2 must hold nobs finite values >= 0")
    return H0, y, sigma2


def spd_factor(A: np.ndarray, level: int):
    """Cholesky factor of A_l; ValueError naming the level when A_l is not (numerically) positive definite"""
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        L = None
    if L is None or not np.all(np.diag(L) ** 2 > PIVOT_RTOL * np.diag(A)):
        raise ValueError(f"conditioner: A of level {level} is not positive definite (with exact data: two observations "
                         f"inside one element of level {level})")
    return L


def apply_affine(K, A, H, y, sigma2, g, zeta=None, exp=False):
    """g + K A^-1 (y + sqrt(sigma2) zeta - H g) for a batch g (nbatch, n); K (n, nobs), A (nobs, nobs), H scipy (nobs, n)"""
    g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    noisy = sigma2 is not None and np.any(np.asarray(sigma2) > 0.0)
    if noisy != (zeta is not None):
        raise ValueError("conditioner: zeta is required iff some sigma2 > 0")
    d = np.asarray(y)[None, :] - (H @ g.T).T
    if noisy:
        d = d + np.sqrt(sigma2)[None, :] * np.atleast_2d(zeta)
    out = g + (K @ _refined_solve(A, d.T)).T
    return np.exp(out) if exp else out


def _refined_solve(A, d):
    """A^-1 d for columns d (nobs, nbatch): Cholesky and one step of iterative refinement with the residual in long double.  A
    plain float64 Cholesky solve carries cond(A) eps, which at cond(A) = 3.5e3 is 2e-12 in exp() of fields of size 25
    (tests/gemm_depth_cases.py)"""
    chol = (np.linalg.cholesky(A), True)
    c = sla.cho_solve(chol, d)
    r = np.asarray(d, dtype=np.longdouble) - np.asarray(A, dtype=np.longdouble) @ np.asarray(c, dtype=np.longdouble)
    return c + sla.cho_solve(chol, np.asarray(r, dtype=np.float64))


def apply_tangent(K, A, H, dg, s_out=None):
    """The derivative of apply_affine in g applied to a batch dg (nbatch, n): f' o (dg - K A^-1 H dg), f' = s_out (the
    conditional lognormal field of the linearization point) or 1.  Independent of y, sigma2 and zeta."""
    dg = np.atleast_2d(np.asarray(dg, dtype=np.float64))
    out = dg - (K @ _refined_solve(A, np.asarray(H @ dg.T))).T
    return out if s_out is None else out * np.atleast_2d(np.asarray(s_out, dtype=np.float64))


def apply_adjoint(K, A, H, v, s_out=None):
    """The transpose of apply_tangent applied to a batch v (nbatch, n): u - H^T A^-1 K^T u, u = v o s_out (u = v without
    s_out).  <apply_tangent(dg, s), v> = <dg, apply_adjoint(v, s)>."""
    u = np.atleast_2d(np.asarray(v, dtype=np.float64))
    if s_out is not None:
        u = u * np.atleast_2d(np.asarray(s_out, dtype=np.float64))
    return u - np.asarray(H.T @ _refined_solve(A, K.T @ u.T)).T


class _Gaussian:
    """EvalGaussian of one level as a linear map of xi (drawn on that level), by sparse direct solves"""

    def __init__(self, problem, level):
        L = problem.levels[level]
        self.g, self.w = problem.matern_g, np.asarray(L.w_diag, dtype=np.float64)
        self.L = L
        if hasattr(L, "n_lambda"):     # hybridized: s = z f - G^T H^-1 G f
            self.lu = spla.splu(sp.csc_matrix(L.H))
        else:                          # saddle point: [M B^T; B -alpha W] [u; s] = [0; f]
            W = sp.diags(self.w)
            self.lu = spla.splu(sp.bmat([[L.M, L.B.T], [L.B, -problem.alpha * W]], format="csc"))

    def __call__(self, xi):
        """columns of xi (n_s, k) -> Gaussian fields (n_s, k)"""
        L = self.L
        f = -self.g * np.sqrt(self.w)[:, None] * xi
        if hasattr(L, "n_lambda"):
            return L.z_diag[:, None] * f - L.G.T @ self.lu.solve(np.asarray(L.G @ f))
        return self.lu.solve(np.vstack([np.zeros((L.n_u, f.shape[1])), f]))[L.n_u:]


class Conditioner:
    """Setup (H_l, K_l, A_l per Monte Carlo level) and apply of the conditioning map for a SamplerProblem, a
    HybridSamplerProblem or a KLProblem."""

    def __init__(self, problem, H0, y, sigma2=None):
        self.problem = problem
        H0, self.y, self.sigma2 = check_observations(H0, y, sigma2, problem.levels[0].n_s)
        self.nobs = H0.shape[0]
        self.noisy = self.sigma2 is not None and bool(np.any(self.sigma2 > 0.0))
        self.H: List[sp.csr_matrix] = [H0]
        for lvl in range(problem.n_mc_levels - 1):
            Hn = sp.csr_matrix(self.H[-1] @ problem.levels[lvl].P)
            Hn.sort_indices()
            self.H.append(Hn)
        self.K: List[np.ndarray] = []
        self.A: List[np.ndarray] = []
        self._chol = []
        R = np.zeros(self.nobs) if self.sigma2 is None else self.sigma2
        for lvl, H in enumerate(self.H):
            K = self.cross_covariance(lvl, H.T.toarray())
            HK = np.asarray(H @ K)
            A = 0.5 * (HK + HK.T) + np.diag(R)
            self._chol.append(spd_factor(A, lvl))
            self.K.append(K)
            self.A.append(A)

    def cross_covariance(self, level, V):
        """C_level V for dense columns V (n_s(level), k)"""
        p = self.problem
        if hasattr(p, "evects"):
            phi = p.evects[level]
            return phi @ (p.evals[:, None] * (phi.T @ V))
        ev = _Gaussian(p, level)
        sw = np.sqrt(ev.w)[:, None]
        return ev(sw * ev(V / sw))     # column j: t = EvalGaussian(W^-1/2 v_j), then EvalGaussian(W^1/2 t)

    def covariance(self, level) -> np.ndarray:
        """dense C_level (small levels only)"""
        return self.cross_covariance(level, np.eye(self.problem.levels[level].n_s))

    def gain(self, level) -> np.ndarray:
        """K_l A_l^-1 (n_s(level), nobs)"""
        return sla.cho_solve((self._chol[level], True), self.K[level].T).T

    def apply(self, level, g, zeta=None, exp=False):
        """g + K_l A_l^-1 (y + sqrt(sigma2) * zeta - H_l g) for a batch g (nbatch, n_s(level)); zeta (nbatch, nobs) standard
        normals, required iff some sigma2 > 0; exp: return exp() of it"""
        return apply_affine(self.K[level], self.A[level], self.H[level], self.y, self.sigma2 if self.noisy else None, g, zeta,
                            exp)

    def apply_tangent(self, level, dg, s_out=None):
        """f' o (dg - K_l A_l^-1 H_l dg) for a batch dg (nbatch, n_s(level)): the derivative of apply in g; f' = s_out or 1"""
        return apply_tangent(self.K[level], self.A[level], self.H[level], dg, s_out)

    def apply_adjoint(self, level, v, s_out=None):
        """u - H_l^T A_l^-1 K_l^T u, u = v o s_out, for a batch v (nbatch, n_s(level)): the transpose of apply_tangent"""
        return apply_adjoint(self.K[level], self.A[level], self.H[level], v, s_out)


def pick_observation_elements(hierarchy, nobs: int, seed: int = 0) -> np.ndarray:
    """nobs fine elements with pairwise distinct ancestors on the coarsest level of `hierarchy` (sorted)"""
    anc = np.arange(hierarchy.spaces[0].n_s)
    for P in hierarchy.P:
        anc = _parents(P)[anc]
    nc = hierarchy.spaces[-1].n_s
    if nobs > nc:
        raise ValueError(f"{nobs} observations need {nobs} coarse elements, the coarsest level has {nc}")
    rng = np.random.default_rng(seed)
    coarse = rng.choice(nc, size=nobs, replace=False)
    elems = [rng.choice(np.nonzero(anc == c)[0]) for c in coarse]
    return np.sort(np.asarray(elems, dtype=np.int64))


def _parents(P) -> np.ndarray:
    """parent[i]: the single coarse element of fine element i (P0 injection prolongator)"""
    P = sp.csr_matrix(P)
    if np.any(np.diff(P.indptr) != 1):
        raise ValueError("prolongator rows must hold one entry")
    return P.indices.copy()


def point_observations(n0: int, elems, extra_rows: Optional[list] = None) -> sp.csr_matrix:
    """unit rows at `elems`; extra_rows: [(columns, weights)] appended as averaging rows"""
    rows = [([int(e)], [1.0]) for e in elems] + list(extra_rows or [])
    ci = np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in rows])
    va = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows])
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    return sp.csr_matrix((va, ci, rp), shape=(len(rows), n0))

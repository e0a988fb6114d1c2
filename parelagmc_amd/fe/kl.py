"""Setup of the truncated Karhunen-Loeve sampler (the reference's KLSampler and its two covariance functions).

Restates, on the host and in numpy/scipy, what the reference computes once before sampling:
  * AnalyticExponentialCovariance::computeEigs   /root/reference/src/AnalyticExponentialCovariance.cpp:117-361
  * MaternCovariance::GenerateCovarianceMatrix / solveEigenvalueSymEigensolver
                                                 /root/reference/src/MaternCovariance.cpp:114-142,312-355,432-449
  * KLSampler::BuildHierarchy                    /root/reference/src/KLSampler.cpp:144-191
The per-realization work, s = Phi_level Lambda^1/2 xi[:m] (KLSampler::Eval, :199-223), runs on the device
(pmc_sampler_create_kl).  Every field is piecewise constant (P0): one value per element, level 0 finest.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List, Optional, Sequence

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.special

from .mesh import element_centroids
from .problems import Hierarchy

# computeOmega's bisection (AnalyticExponentialCovariance.cpp:223-287)
OMEGA_TOL = 1e-5
OMEGA_MAXIT = 1000


def _omega_residual(x, lt):
    return math.tan(x) - (2.0 * lt * x) / (lt * lt * x * x - 1.0)


def omega_brackets(nmodes: int, scaled_corlen: float) -> np.ndarray:
    """xlvec of computeOmega: pi/2 + j pi, with the asymptote 1/l~ of the right-hand side spliced in.  Root j lies in
    [1.001 xlvec[j], 0.999 xlvec[j+1]].  (The reference's array holds nmodes + 2 entries and the splice can write one past
    it; here it is long enough.)"""
    asyx = 1.0 / scaled_corlen
    xl = np.zeros(nmodes + 4)
    ctr = 0
    xl[0] = math.pi / 2.0
    if asyx < math.pi / 2.0:
        xl[0] = asyx
        xl[1] = math.pi / 2.0
        ctr += 1
    while ctr < nmodes + 1:
        ctr += 1
        xl[ctr] = xl[ctr - 1] + math.pi
        if xl[ctr - 1] < asyx < xl[ctr]:
            xl[ctr] = asyx
            ctr += 1
            xl[ctr] = xl[ctr - 2] + math.pi
    return xl[:nmodes + 1]


def compute_omega(nmodes: int, scaled_corlen: float) -> np.ndarray:
    """The roots omega_j of tan(w) = 2 l~ w / (l~^2 w^2 - 1) exactly as computeOmega's bisection returns them (residual
    tolerance 1e-5 at the midpoint, at most 1000 halvings): the same iterate, not a more accurate root."""
    lt = scaled_corlen
    xlvec = omega_brackets(nmodes, lt)
    omega = np.zeros(nmodes)
    for j in range(nmodes):
        xl = 1.001 * xlvec[j]
        xr = 0.999 * xlvec[j + 1]
        xm = (xl + xr) / 2.0
        fl = _omega_residual(xl, lt)
        fm = _omega_residual(xm, lt)
        it = 0
        while abs(fm) > OMEGA_TOL and it < OMEGA_MAXIT:
            xm = (xl + xr) / 2.0
            fm = _omega_residual(xm, lt)
            if fl * fm < 0:
                xr = xm
            else:
                xl = xm
            fl = _omega_residual(xl, lt)
            it += 1
        omega[j] = xm
    return omega


def _p0_normalise(v: np.ndarray, vol: np.ndarray) -> np.ndarray:
    """scale the columns of v to unit P0 mass norm: v^T diag(vol) v = 1 per column"""
    return v / np.sqrt(np.einsum("i,i...->...", vol, v * v))


def analytic_exponential_eigs(h: Hierarchy, nmodes: Sequence[int], domain_lengths: Sequence[float], corlen):
    """(lambda, Phi0) of AnalyticExponentialCovariance on the finest level of `h`: the separable exponential kernel
    exp(-|x_d - y_d| / corlen) per axis on [0, L_d], modes the tensor products of the 1D eigenpairs in i-major loop order
    ("Number of modes" = {n_x, n_y[, n_z]}, NOT sorted by eigenvalue), each product renormalised in the P0 mass inner
    product.  `corlen`: one correlation length or one per axis.  Phi0: (n_s(0), m), column k = mode k."""
    sp0 = h.spaces[0]
    dim = sp0.mesh.dim
    nmodes = [int(n) for n in nmodes]
    if len(nmodes) != dim or len(domain_lengths) != dim:
        raise ValueError("analytic_exponential_eigs: one mode count and one domain length per axis")
    corl = np.broadcast_to(np.asarray(corlen, dtype=np.float64), (dim,))
    m = int(np.prod(nmodes))
    if m > sp0.n_s:
        raise ValueError(f"analytic_exponential_eigs: {m} modes exceed the {sp0.n_s} elements (m <= NE is asserted)")
    x = element_centroids(sp0.mesh)       # P0 ProjectCoefficient: the coefficient at the element centre
    vol = sp0.vol
    ev1, vec1 = [], []
    for d in range(dim):
        L = float(domain_lengths[d])
        lt = float(corl[d]) / L
        om = compute_omega(nmodes[d], lt)
        ev1.append(2.0 * L * lt / (lt * lt * om * om + 1.0))          # computeEigenvalues1d
        xc = x[:, d:d + 1] * om[None, :] / L
        v = (np.sin(xc) + lt * om[None, :] * np.cos(xc)) / L           # AnalyticExponentialEvect1dCoefficient::Eval
        vec1.append(_p0_normalise(v, vol))
    if dim == 2:
        lam = (ev1[0][:, None] * ev1[1][None, :]).ravel()
        phi = (vec1[0][:, :, None] * vec1[1][:, None, :]).reshape(sp0.n_s, m)
    else:
        lam = (ev1[0][:, None, None] * ev1[1][None, :, None] * ev1[2][None, None, :]).ravel()
        phi = (vec1[0][:, :, None, None] * vec1[1][:, None, :, None] * vec1[2][:, None, None, :]).reshape(sp0.n_s, m)
    return lam, np.ascontiguousarray(_p0_normalise(phi, vol))


def matern_kernel(r: np.ndarray, corlen: float, dim: int) -> np.ndarray:
    """MaternCovariance::Compute with nu = 2 - d/2, kappa = 1/corlen: exp(-kappa r) in 3D, (sqrt2 kappa r) K1(sqrt2 kappa r)
    in 2D, 1 where kappa r < 1e-10.  K1 is scipy's; the reference evaluates it with the polynomial bessk1 of Utilities.hpp
    (about 1e-7 relative error), so 2D covariances differ from the reference's at that level."""
    kr = np.asarray(r, dtype=np.float64) / corlen
    out = np.ones_like(kr)
    far = kr >= 1e-10
    if dim == 3:
        out[far] = np.exp(-kr[far])
    elif dim == 2:
        t = math.sqrt(2.0) * kr[far]
        out[far] = t * scipy.special.k1(t)      # scale = 1 / (Gamma(1) 2^0) = 1
    else:
        raise ValueError("matern_kernel: 2D or 3D meshes only")
    return out


def matern_covariance(h: Hierarchy, corlen: float) -> np.ndarray:
    """C_ij = Compute(x_i, x_j) at the element centres of the finest level (dense n_s x n_s)"""
    sp0 = h.spaces[0]
    x = element_centroids(sp0.mesh)
    d2 = np.maximum((x * x).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * x @ x.T, 0.0)
    C = matern_kernel(np.sqrt(d2), corlen, sp0.mesh.dim)
    np.fill_diagonal(C, 1.0)
    return C


def matern_eigs(h: Hierarchy, corlen: float, nmodes: int, eigensolver: str = "dense", ctx=None, **solver_opts):
    """(lambda, Phi0) of MaternCovariance: the top m = min(nmodes, NE) eigenpairs of the generalised problem
    A v = lambda W v, A = W C W, W = diag(P0 mass), in ascending order and with V^T W V = I.
      eigensolver="dense"     LAPACK (dsygvx, RANGE='I', indices n - m + 1 .. n).  Dense O(NE^2) memory and O(NE^3) work:
                              meant for NE up to about 16k.
      eigensolver="filtered"  matern_eigs_filtered, the numpy twin of the device solver (O(NE (m + guard)) memory).
      eigensolver="device"    pmc_kl_matern_eigs on the device of `ctx` (capi.Context): matrix-free, 3D only.
    solver_opts (filtered / device): tol, max_iter, guard, degree, seed."""
    sp0 = h.spaces[0]
    n = sp0.n_s
    m = min(int(nmodes), n)
    w = sp0.vol
    if eigensolver == "filtered":
        lam, V, _ = matern_eigs_filtered(element_centroids(sp0.mesh), w, corlen, m, **solver_opts)
        return lam, V
    if eigensolver == "device":
        if ctx is None:
            raise ValueError("matern_eigs: eigensolver='device' needs ctx (a capi.Context)")
        from .. import capi
        lam, V, _ = capi.kl_matern_eigs(ctx, element_centroids(sp0.mesh), w, corlen, m, **solver_opts)
        return lam, V
    if eigensolver != "dense":
        raise ValueError(f"unknown eigensolver {eigensolver!r} (dense | filtered | device)")
    if solver_opts:
        raise ValueError("matern_eigs: the dense solver takes no options")
    A = matern_covariance(h, corlen)
    A *= w[:, None]
    A *= w[None, :]
    lam, V = sla.eigh(A, np.diag(w), subset_by_index=[n - m, n - 1], driver="gvx")
    return lam, np.ascontiguousarray(V)


def matern_apply_blocked(x: np.ndarray, w: np.ndarray, corlen: float, X: np.ndarray, rows: int = 1024) -> np.ndarray:
    """Y = K X with K = W^1/2 C W^1/2, K_ij = sqrt(w_i) c(|x_i - x_j|) sqrt(w_j), K_ii = w_i, in row blocks of `rows`: never
    holds more than rows x n entries of K.  Distances from sum (x_i - x_j)^2, as the device kernel takes them."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = x.shape
    sw = np.sqrt(w)
    X = np.asarray(X, dtype=np.float64).reshape(n, -1)
    Y = np.empty_like(X)
    swX = sw[:, None] * X
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        d2 = np.zeros((r1 - r0, n))
        for d in range(dim):
            diff = x[r0:r1, d:d + 1] - x[None, :, d]
            d2 += diff * diff
        C = matern_kernel(np.sqrt(d2), corlen, dim)
        C[np.arange(r1 - r0), np.arange(r0, r1)] = 1.0
        Y[r0:r1] = sw[r0:r1, None] * (C @ swX)
    return Y


def normalise_signs(V: np.ndarray) -> np.ndarray:
    """the entry of largest magnitude of every column (the first one on ties) made positive"""
    idx = np.argmax(np.abs(V), axis=0)
    s = np.where(V[idx, np.arange(V.shape[1])] < 0.0, -1.0, 1.0)
    return V * s[None, :]


def _cholqr(X: np.ndarray) -> np.ndarray:
    """unit columns, then Cholesky-QR until two passes ran without a shift"""
    clean = 0
    b = X.shape[1]
    for _ in range(6):
        X = X / np.sqrt((X * X).sum(0))[None, :]
        G = X.T @ X
        G = 0.5 * (G + G.T)
        shifted = False
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            shifted = True
            shift = 1e-13 * b
            while True:
                try:
                    L = np.linalg.cholesky(G + shift * np.eye(b))
                    break
                except np.linalg.LinAlgError:
                    shift *= 100.0
        X = sla.solve_triangular(L, X.T, lower=True).T
        clean += not shifted
        if clean >= 2:
            return X
    raise RuntimeError("matern_eigs_filtered: the block could not be orthonormalised")


def matern_eigs_filtered(x: np.ndarray, w: np.ndarray, corlen: float, nmodes: int, tol: float = 1e-8, max_iter: int = 100,
                         guard: int = 16, degree: int = 8, seed: int = 0, rows: int = 1024):
    """numpy twin of pmc_kl_matern_eigs: Chebyshev-filtered subspace iteration on K y = lambda y (y = W^1/2 v) with a block
    of m + guard columns, filter of `degree` on [0, smallest Ritz value] (0.9 of it when guard = 0) scaled to 1 at the
    largest, Cholesky-QR twice and Rayleigh-Ritz after every filter; stops when max_k ||K y_k - theta_k y_k|| <= tol theta_1 over the m wanted columns.
    K is applied in row blocks (matern_apply_blocked).  Returns (lambda ascending (m), V (n, m) with V^T W V = I and the
    sign rule of normalise_signs, info dict as pmc_kl_eigs_info).  The start block is numpy's Philox stream of `seed`, not the
    device's: the two solvers agree to the tolerance, not bitwise."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = x.shape[0]
    if x.shape[1] != 3:
        raise ValueError("matern_eigs_filtered: 3D only (as the device solver)")
    m = min(int(nmodes), n)
    if m + guard > 512:
        raise ValueError("matern_eigs_filtered: m + guard exceeds 512")
    b = min(m + guard, n)
    products = 0

    def apply(X):
        nonlocal products
        products += 1
        return matern_apply_blocked(x, w, corlen, X, rows)

    def ritz(X):
        Y = apply(X)
        H = X.T @ Y
        th, S = np.linalg.eigh(0.5 * (H + H.T))
        th, S = th[::-1], S[:, ::-1]
        return X @ S, Y @ S, th

    X = np.random.Generator(np.random.Philox(seed)).standard_normal((n, b))
    X, Y, th = ritz(_cholqr(X))
    res = np.sqrt(((Y - X * th[None, :])[:, :m] ** 2).sum(0)).max() / th[0]
    it = 0
    while res > tol and it < max_iter:
        it += 1
        # no guard column (b == m < n): th[-1] is a wanted value and must lie outside the damped interval (see kl_eigs.hip)
        lo = max((0.9 if b == m and b < n else 1.0) * th[-1], 1e-14 * th[0])
        e = c = 0.5 * lo
        sigma = e / (th[0] - c)
        tau = 2.0 / sigma
        P0, P1 = X, (Y - c * X) * (sigma / e)
        for _ in range(2, degree + 1):
            sigma2 = 1.0 / (tau - sigma)
            P0, P1 = P1, (apply(P1) - c * P1) * (2.0 * sigma2 / e) - (sigma * sigma2) * P0
            sigma = sigma2
        X, Y, th = ritz(_cholqr(P1))
        res = np.sqrt(((Y - X * th[None, :])[:, :m] ** 2).sum(0)).max() / th[0]
    V = normalise_signs(np.ascontiguousarray((X[:, :m] / np.sqrt(w)[:, None])[:, ::-1]))
    info = dict(iterations=it, block_products=products, converged=int(res <= tol), max_residual_rel=float(res),
                gap_rel=float((th[m - 1] - th[m]) / th[0]) if b > m else 0.0)
    return np.ascontiguousarray(th[:m][::-1]), V, info


def kl_projector(P: sp.csr_matrix, w_fine: np.ndarray) -> sp.csr_matrix:
    """Pi = D^-1 P^T W of a P0 prolongator P (fine x coarse), D = P^T W P: ParELAG's L2 projector onto the coarser space.
    D must be diagonal (every fine element in at most one agglomerate)."""
    P = sp.csr_matrix(P)
    D = (P.T @ sp.diags(w_fine) @ P).tocsr()
    off = D - sp.diags(D.diagonal())
    off.eliminate_zeros()
    if off.nnz:
        raise ValueError("kl_projector: P^T W P is not diagonal")
    return (sp.diags(1.0 / D.diagonal()) @ P.T @ sp.diags(w_fine)).tocsr()


def project_kl_levels(h: Hierarchy, phi0: np.ndarray, nlevels: Optional[int] = None) -> List[np.ndarray]:
    """[Phi_l] of KLSampler::BuildHierarchy: Phi_{l+1} = Pi_l Phi_l, the coarse columns NOT renormalised"""
    nl = h.nlevels if nlevels is None else nlevels
    out = [np.asarray(phi0, dtype=np.float64)]
    for lvl in range(nl - 1):
        out.append(np.asarray(kl_projector(h.P[lvl], h.spaces[lvl].vol) @ out[-1]))
    return out


@dataclasses.dataclass
class KLLevel:
    n_s: int
    w_diag: np.ndarray                 # diag(W) = element volumes
    P: Optional[sp.csr_matrix]         # n_s(l) x n_s(l+1) P0 prolongator, None on the last level


@dataclasses.dataclass
class KLProblem:
    levels: List[KLLevel]
    n_mc_levels: int                   # = len(levels): every level of a KL sampler is a Monte Carlo level
    evals: np.ndarray                  # (m,) CovarianceFunction::Eigenvalues()
    evect0: np.ndarray                 # (n_s(0), m) CovarianceFunction::Eigenvectors() on the finest level
    lognormal: bool
    covariance: str
    evects: List[np.ndarray]           # host Phi_l of every level (project_kl_levels), for checks

    @property
    def nmodes(self) -> int:
        return int(self.evals.size)


def build_kl_sampler_problem(h: Hierarchy, covariance: str = "analytic", nmodes=None, domain_lengths=None, corlen=0.1,
                             lognormal: bool = False, n_mc_levels: Optional[int] = None, eigensolver: str = "dense",
                             ctx=None, **solver_opts) -> KLProblem:
    """Everything pmc_sampler_create_kl takes.  analytic: nmodes = modes per axis (default 4 per axis, the
    CreateSamplerParameterList default), domain_lengths = the box (default: the finest mesh's extent from the origin);
    matern: nmodes = total number of modes (default 64), eigensolver / ctx / solver_opts as matern_eigs takes them
    ("device": the matrix-free solver on the GPU of ctx).  n_mc_levels defaults to the levels with at least m elements
    (the reference would read past xi on a level with fewer)."""
    dim = h.spaces[0].mesh.dim
    if covariance == "analytic":
        nm = [4] * dim if nmodes is None else list(nmodes)
        dl = list(h.spaces[0].mesh.verts.max(axis=0)) if domain_lengths is None else list(domain_lengths)
        lam, phi0 = analytic_exponential_eigs(h, nm, dl, corlen)
    elif covariance == "matern":
        lam, phi0 = matern_eigs(h, corlen, 64 if nmodes is None else int(nmodes), eigensolver=eigensolver, ctx=ctx,
                                **solver_opts)
    else:
        raise ValueError(f"unknown covariance {covariance!r} (analytic | matern)")
    m = lam.size
    if n_mc_levels is None:
        n_mc_levels = 0
        while n_mc_levels < h.nlevels and h.spaces[n_mc_levels].n_s >= m:
            n_mc_levels += 1
    if not 1 <= n_mc_levels <= h.nlevels:
        raise ValueError("build_kl_sampler_problem: n_mc_levels out of range")
    levels = [KLLevel(h.spaces[i].n_s, h.spaces[i].vol.copy(), h.P[i] if i < n_mc_levels - 1 else None)
              for i in range(n_mc_levels)]
    return KLProblem(levels, n_mc_levels, lam, phi0, lognormal, covariance, project_kl_levels(h, phi0, n_mc_levels))

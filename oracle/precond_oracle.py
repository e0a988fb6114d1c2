"""ORACLE (test infrastructure): fp64 restatement of the MINRES preconditioner B(k)^-1 of the mixed Darcy solver on the
caller's level hierarchy, written from the mathematics (include/pmc.h: pmc_solver_opts; csrc/solver.hpp: ChebParams,
Multigrid), not from the kernels.

    B(k)^-1 = diag( p_M(D_l1^-1 M(k)) D_l1^-1 ,  V(S(k)) )

- M-block: Chebyshev polynomial of degree `degree_M` in D_l1^-1 M(k) on [1 / ratio_M, 1] (lmax 1: the l1 row sums bound the
  spectrum), D_l1 = the l1 row sums of M(k) after the elimination of the essential rows (DarcyOracle.assemble);
- S-block: one V-cycle on S_0(k) = B diag(M(k))^-1 B^T (essential u-dofs eliminated) and S_{l+1} = s P_l^T S_l P_l with
  s = 1/2, Jacobi-scaled Chebyshev smoothers of degree `smooth_degree` on [lmax / smooth_ratio, lmax], lmax = 2 * 1.0001
  (a weakly diagonally dominant M-matrix has spec(D^-1 S) in (0, 2]), pre-smoothing from zero, post-smoothing from the
  corrected iterate, and a Chebyshev polynomial of degree `coarse_degree` on [lmax / coarse_ratio, lmax] on the last level.

DarcyChainPrecondOracle: B(k)^-1 of a Darcy handle on its INTERNAL hierarchy - the smoothed-aggregation chain of a
saddle-point handle (mg_coarsening) or the multiplier aggregation of a hybridized handle - from the prolongators and setup
values pmc_darcy_vcycle_prolongator / pmc_darcy_vcycle_level export: S_{v+1} = s P_v^T S_v P_v per realization, and on every
level the per-realization Gershgorin bound lambda_v = 1.0001 max_i sum_j |S_v,ij| / |S_v,ii| as the smoothers' lmax.

SamplerPrecondOracle: the same for the SPDE sampler's handles (csrc/sampler.hip), whose cycles may also end with an exact
solve (the dense inverse of the bottom level, or of an inner level for narrow launches), and whose hierarchies are either the
caller's levels, each rediscretized, or internal Galerkin hierarchies over a prolongator the library exports.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from .darcy_oracle import DarcyOracle

GALERKIN_SCALE = 0.5            # S_{l+1} = 1/2 P^T S_l P on the caller's hierarchy
LMAX_SCHUR = 2.0 * 1.0001       # Gershgorin bound of D^-1 S with a 1e-4 margin
# pmc_sampler_vcycle_level: role of a level in a cycle; pmc_sampler_ / pmc_darcy_vcycle_level: the kinds of hierarchy
ROLE_DESCEND, ROLE_POLY, ROLE_EXACT, ROLE_UNREACHED = 0, 1, 2, 3
KIND_CALLER, KIND_SA, KIND_HYBRID = 0, 1, 2
GERSH_MARGIN = 1.0001          # internal hierarchies: lmax of every level and realization = this times its Gershgorin bound


def gershgorin_lmax(S):
    """1.0001 max_i sum_j |S_ij| / |S_ii|: an upper bound of spec(D^-1 S) with a 1e-4 margin"""
    S = S.tocsr()
    return GERSH_MARGIN * float((np.asarray(abs(S).sum(axis=1)).ravel() / np.abs(S.diagonal())).max())


def cheb2_coefficients(lmax, ratio):
    """closed form of the degree-2 Chebyshev polynomial: p(D^-1 A) D^-1 r = D^-1 (c0 r - c1 A D^-1 r).  From
    1 - l p(l) = T_2((theta - l) / delta) / T_2(sigma): p(l) = (4 theta / delta^2) / T_2(sigma) - (2 / delta^2) / T_2(sigma) l."""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    t2 = 2.0 * (theta / delta) ** 2 - 1.0
    return 4.0 * theta / (delta * delta * t2), 2.0 / (delta * delta * t2)


def chebyshev(A, dinv, r, degree, lmax, ratio, x0=None):
    """Chebyshev semi-iteration of `degree` steps for A x = r preconditioned by diag(dinv), spectrum of D^-1 A assumed in
    [lmax / ratio, lmax] (Saad, Iterative Methods, Alg. 12.1).  x0 None: from a zero guess (x = p(D^-1 A) D^-1 r); else
    x0 + p(D^-1 A) D^-1 (r - A x0)."""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho_old = 1.0 / sigma
    if x0 is None:
        d = dinv * r / theta
        x = d.copy()
    else:
        d = dinv * (r - A @ x0) / theta
        x = x0 + d
    for _ in range(1, degree):
        rho = 1.0 / (2.0 * sigma - rho_old)
        d = rho * rho_old * d + (2.0 * rho / delta) * dinv * (r - A @ x)
        x = x + d
        rho_old = rho
    return x


def vcycle(levels, r, smooth_degree, smooth_ratio, coarse_degree=None, coarse_ratio=None, l=0, coarse_solve=None):
    """One V(1,1)-cycle from level l.  levels[i] = (S_i, lmax_i, P_i) with P_i: level i+1 -> i (None on the last level), or
    (S_i, lmax_i, P_i, bottom_i) with bottom_i None (smooth and descend) or a callable r -> x that ends the cycle on level i
    (bottom_polynomial / bottom_exact).  A 3-tuple last level runs the polynomial of degree coarse_degree on
    [lmax / coarse_ratio, lmax], or coarse_solve (optional: an exact solve, the textbook two-grid method)."""
    S, lmax, P = levels[l][:3]
    bottom = levels[l][3] if len(levels[l]) > 3 else None
    if bottom is not None:
        return bottom(r)
    dinv = 1.0 / S.diagonal()
    if l == len(levels) - 1:
        if coarse_solve is not None:
            return coarse_solve(r)
        return chebyshev(S, dinv, r, coarse_degree, lmax, coarse_ratio)
    x = chebyshev(S, dinv, r, smooth_degree, lmax, smooth_ratio)
    xc = vcycle(levels, P.T @ (r - S @ x), smooth_degree, smooth_ratio, coarse_degree, coarse_ratio, l + 1, coarse_solve)
    x = x + P @ xc
    return chebyshev(S, dinv, r, smooth_degree, lmax, smooth_ratio, x0=x)


def bottom_polynomial(S, lmax, degree, ratio):
    """the cycle ends with a Chebyshev polynomial of `degree` in D^-1 S on [lmax / ratio, lmax]"""
    dinv = 1.0 / S.diagonal()
    return lambda r: chebyshev(S, dinv, r, degree, lmax, ratio)


def bottom_exact(S):
    """the cycle ends with an exact solve S^-1 r (Cholesky of the dense level operator)"""
    c = sla.cho_factor(S.toarray() if sp.issparse(S) else S)
    return lambda r: sla.cho_solve(c, r)


class DarcyPrecondOracle:
    """B(k)^-1 of a saddle-point Darcy handle on the caller's hierarchy, one realization at a time."""

    def __init__(self, problem, smooth_degree=2, smooth_ratio=8.0, coarse_degree=12, coarse_ratio=100.0):
        self.p = problem
        self.do = DarcyOracle(problem)
        self.smooth = (smooth_degree, smooth_ratio, coarse_degree, coarse_ratio)

    def mass(self, level, k):
        """M(k) with the essential rows / columns eliminated (unit diagonal there), and the essential mask"""
        L = self.p.levels[level]
        A = self.do.assemble(level, np.asarray(k, dtype=np.float64))[0].tocsr()
        return A[:L.n_u, :L.n_u].tocsr(), L.ess_mask.astype(bool)

    def schur(self, level, k):
        """S_0(k) = B diag(M(k))^-1 B^T of `level`, the essential u-dofs eliminated"""
        L = self.p.levels[level]
        M, ess = self.mass(level, k)
        Bk = (L.B @ sp.diags((~ess).astype(np.float64))).tocsr()
        return (Bk @ sp.diags(1.0 / M.diagonal()) @ Bk.T).tocsr()

    def schur_levels(self, level, k):
        """[(S_l, lmax, P_l)] from `level` down to the last level of the problem"""
        S = self.schur(level, k)
        out = []
        for l in range(level, len(self.p.levels)):
            P = self.p.levels[l].P if l + 1 < len(self.p.levels) else None
            out.append((S, LMAX_SCHUR, P))
            if P is not None:
                S = (GALERKIN_SCALE * (P.T @ S @ P)).tocsr()
        return out

    def mblock(self, level, k, r_u, ratio_M, degree_M):
        """p_M(D_l1^-1 M(k)) D_l1^-1 r_u"""
        M, _ = self.mass(level, k)
        l1inv = 1.0 / np.asarray(abs(M).sum(axis=1)).ravel()
        return chebyshev(M, l1inv, r_u, degree_M, 1.0, ratio_M)

    def apply(self, level, k, r, ratio_M, degree_M):
        L = self.p.levels[level]
        zu = self.mblock(level, k, r[:L.n_u], ratio_M, degree_M)
        zp = vcycle(self.schur_levels(level, k), r[L.n_u:], *self.smooth)
        return np.concatenate([zu, zp])


class DarcyChainPrecondOracle:
    """B(k)^-1 of ONE Monte Carlo level of a Darcy handle whose cycle runs on an internal hierarchy, one realization at a
    time, from the problem, the setup values of pmc_darcy_vcycle_level (`setup`: CAPI DarcySolver.vcycle_levels) and the
    prolongators of pmc_darcy_vcycle_prolongator (`prolongators[v]`: vlevel v + 1 -> v).

    - kind 1 (smoothed aggregation of a saddle-point handle): diag(p_M(D_l1^-1 M(k)) D_l1^-1, V(S(k))) with
      S_0(k) = B diag(M(k))^-1 B^T as on the caller's hierarchy (DarcyPrecondOracle.schur) and the M-block unchanged;
    - kind 2 (hybridized handle): V(H(kappa)) alone, S_0 = H(kappa) of `hybrid_level` (fe/darcy_hybrid.py:DarcyHybridLevel),
      kappa = k when M(k) divides by k, else 1 / k;
    - S_{v+1} = s P_v^T S_v P_v with the exported s; every level smooths with Jacobi-scaled Chebyshev of smooth_degree on
      [lambda_v / smooth_ratio, lambda_v], lambda_v = gershgorin_lmax(S_v) of this realization; the last level runs the
      polynomial of (last_degree, last_ratio) on [lambda / last_ratio, lambda]."""

    def __init__(self, problem, level, setup, prolongators, hybrid_level=None):
        self.p, self.level, self.setup, self.P = problem, level, setup, prolongators
        self.kind = int(setup[0]["hierarchy"])
        assert self.kind in (KIND_SA, KIND_HYBRID) and (hybrid_level is not None) == (self.kind == KIND_HYBRID)
        assert len(prolongators) == len(setup) - 1
        self.hl = hybrid_level
        self.base = DarcyPrecondOracle(problem)

    def operators(self, k):
        """[S_v(k)] of every level of the cycle"""
        k = np.asarray(k, dtype=np.float64)
        if self.kind == KIND_HYBRID:
            S = [self.hl.operator(k if self.p.k_divides else 1.0 / k).tocsr()]
        else:
            S = [self.base.schur(self.level, k)]
        for v in range(len(self.setup) - 1):
            S.append((self.setup[v]["galerkin_scale"] * (self.P[v].T @ S[v] @ self.P[v])).tocsr())
        return S

    def levels(self, k):
        """[(S_v, lambda_v, P_v, bottom_v)] for vcycle"""
        out = []
        S = self.operators(k)
        for v, (Sv, m) in enumerate(zip(S, self.setup)):
            lam = gershgorin_lmax(Sv)
            if v + 1 < len(S):
                out.append((Sv, lam, self.P[v], None))
            else:
                out.append((Sv, lam, None, bottom_polynomial(Sv, lam, int(m["last_degree"]), m["last_ratio"])))
        return out

    def vcycle(self, k, r):
        m = self.setup[0]
        return vcycle(self.levels(k), r, int(m["smooth_degree"]), m["smooth_ratio"])

    def apply(self, k, r):
        if self.kind == KIND_HYBRID:
            return self.vcycle(k, r)
        L = self.p.levels[self.level]
        m = self.setup[0]
        zu = self.base.mblock(self.level, k, r[:L.n_u], m["ratio_M"], int(m["degree_M"]))
        return np.concatenate([zu, self.vcycle(k, r[L.n_u:])])




def sampler_schur(level, alpha, schur_scale):
    """S = B (diag(M) / schur_scale)^-1 B^T + alpha W of one caller's sampler level (B with its essential columns removed)"""
    d = level.M.diagonal() / schur_scale
    return (level.B @ sp.diags(1.0 / d) @ level.B.T + alpha * sp.diags(level.w_diag)).tocsr()


class SamplerPrecondOracle:
    """B^-1 of ONE Monte Carlo level of a sampler handle (pmc_sampler_apply_preconditioner) in fp64, from the problem the
    handle was created with, the setup values of pmc_sampler_vcycle_level (`setup`: a list of dicts, CAPI
    PDESampler.vcycle_setup) and the prolongators of pmc_sampler_vcycle_prolongator (`prolongators[v]`: vlevel v + 1 -> v).

    - saddle-point handles: diag(p_M(D_l1^-1 M) D_l1^-1, V(S)), p_M of degree_M on [1 / ratio_M, 1] (D_l1: l1 row sums of M);
      hybridized handles: V(H) alone;
    - kind 0 (the caller's levels): S_v of level `level` + v rediscretized from its own level struct (sampler_schur), not a
      Galerkin product; kind 1 (mg_coarsening): S_0 the same Schur complement, S_{v+1} = s P_v^T S_v P_v with the exported P;
      kind 2 (hybridized): S_0 = the caller's H, Galerkin below;
    - per level: Chebyshev smoothing of smooth_degree on [lmax / smooth_ratio, lmax] before and after the coarse correction;
      the cycle ends where `role_wide` (launches of more than dense_nb realizations) or `role_narrow` says, with the polynomial
      of (last_degree, last_ratio) or an exact solve."""

    def __init__(self, problem, level, setup, prolongators, schur_scale=1.0):
        self.p, self.level, self.setup, self.P = problem, level, setup, prolongators
        kind = int(setup[0]["hierarchy"])
        self.kind = kind
        self.hybrid = kind == KIND_HYBRID
        if kind == KIND_CALLER:
            S = [sampler_schur(problem.levels[level + v], problem.alpha, schur_scale) for v in range(len(setup))]
        else:
            S0 = problem.levels[level].H.tocsr() if self.hybrid else sampler_schur(problem.levels[level], problem.alpha,
                                                                                     schur_scale)
            S = [S0]
            for v in range(len(setup) - 1):
                s = setup[v]["galerkin_scale"]
                S.append((s * (prolongators[v].T @ S[v] @ prolongators[v])).tocsr())
        self.S = S
        self._levels = {}

    def levels(self, narrow):
        """[(S_v, lmax_v, P_v, bottom_v)] of the cycle a narrow (at most dense_nb realizations) or wide launch runs"""
        if narrow not in self._levels:
            out = []
            for v, m in enumerate(self.setup):
                role = int(m["role_narrow" if narrow else "role_wide"])
                if role == ROLE_DESCEND:
                    out.append((self.S[v], m["lmax"], self.P[v], None))
                    continue
                assert role in (ROLE_POLY, ROLE_EXACT), (v, role)
                bottom = (bottom_exact(self.S[v]) if role == ROLE_EXACT else
                          bottom_polynomial(self.S[v], m["lmax"], int(m["last_degree"]), m["last_ratio"]))
                out.append((self.S[v], m["lmax"], None, bottom))
                break
            self._levels[narrow] = out
        return self._levels[narrow]

    def vcycle(self, r, narrow=False):
        m = self.setup[0]
        return vcycle(self.levels(narrow), r, int(m["smooth_degree"]), m["smooth_ratio"])

    def apply(self, r, narrow=False):
        if self.hybrid:
            return self.vcycle(r, narrow)
        L = self.p.levels[self.level]
        m = self.setup[0]
        l1inv = 1.0 / np.asarray(abs(L.M).sum(axis=1)).ravel()
        zu = chebyshev(L.M, l1inv, r[:L.n_u], int(m["degree_M"]), 1.0, m["ratio_M"])
        return np.concatenate([zu, self.vcycle(r[L.n_u:], narrow)])

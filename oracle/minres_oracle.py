"""ORACLE (test infrastructure): preconditioned MINRES for ONE right-hand side in fp64, numpy only, written from the
literature (Paige & Saunders, SIAM J. Numer. Anal. 12 (1975); Greenbaum, Iterative Methods for Solving Linear Systems (1997),
ch. 2.5 and 8) and not from the device's scalar kernels or oracle/c/pmc_ref.c: it is what the solver loops are compared with,
iteration by iteration (tests/test_gpu_minres_trajectory.py), and is itself pinned against a dense minimiser and scipy
(tests/test_minres_oracle.py).

The method.  A symmetric, B SPD (B^-1 = the preconditioner).  With r_0 = b - A x_0 the Lanczos process in the B^-1 inner
product builds vectors q_1, q_2, ... (q_1 = r_0 / ||r_0||_{B^-1}) with <q_i, B^-1 q_j> = delta_ij and

    A B^-1 Q_k = Q_{k+1} T_k,      T_k (k + 1) x k tridiagonal: diagonal a_j, off-diagonals t_{j+1}.

x_k = x_0 + B^-1 Q_k y_k minimises ||b - A x||_{B^-1} over x_0 + K_k(B^-1 A, B^-1 r_0) when y_k solves the least-squares
problem min || ||r_0|| e_1 - T_k y ||_2.  Its QR factorization by Givens rotations advances one column per iteration; the
directions D_k = B^-1 Q_k R_k^-1 obey a three-term recurrence, and the last entry of the rotated right-hand side is the
residual norm: |eta_k| = ||b - A x_k||_{B^-1}.

The stopping rule is the library's (include/pmc.h): goal = max(rel_tol * eta_0, abs_tol); no iteration when
eta_0 <= goal (a zero residual - the zero right-hand side from a zero guess - among them: x_0 is returned, converged, after 0
iterations); otherwise stop after the first iteration k with |eta_k| <= goal, or after max_iter iterations, or when the
Krylov space is exhausted (t_{k+1} = 0: x_k is exact)."""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class MinresRun:
    x: np.ndarray               # the iterate at exit
    iterations: int
    converged: bool             # |eta_iterations| <= goal
    initial_norm: float         # eta_0 = ||b - A x_0||_{B^-1}
    goal: float
    history: np.ndarray         # |eta_0|, ..., |eta_iterations|
    iterates: dict              # k -> x_k for the k in `keep` that were reached (0: x_0)

    @property
    def final_norm(self):
        return float(self.history[-1])


def _rotation(f, g):
    """c, s, h with [c s; -s c] [f; g] = [h; 0], h >= 0"""
    h = float(np.hypot(f, g))
    if h == 0.0:
        return 1.0, 0.0, 0.0
    return f / h, g / h, h


def minres(A, Binv, b, x0, rel_tol, abs_tol, max_iter, keep=()):
    """A: anything with A @ x (symmetric); Binv: callable r -> B^-1 r (B SPD); b, x0: vectors (x0 None: zero).
    keep: iteration numbers whose iterates are returned in MinresRun.iterates."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    keep = set(int(k) for k in keep)
    iterates = {0: x.copy()} if 0 in keep else {}

    resid = b - A @ x if np.any(x) else b.copy()
    p = Binv(resid)
    nrm2 = float(resid @ p)
    if nrm2 < 0.0 or nrm2 != nrm2:
        raise ValueError("minres: <r, B^-1 r> < 0 - the preconditioner is not SPD")
    eta0 = np.sqrt(nrm2)
    goal = max(rel_tol * eta0, abs_tol)
    history = [eta0]
    if eta0 <= goal or max_iter <= 0:
        return MinresRun(x, 0, bool(eta0 <= goal), eta0, goal, np.array(history), iterates)

    # Lanczos vectors, B^-1-orthonormal: q (and its preconditioned twin p = B^-1 q), the one before, the coupling t_j
    q_prev = np.zeros_like(b)
    q, p = resid / eta0, p / eta0
    t = 0.0                       # t_1: no vector before the first
    # the two most recent rotations (c, s) and direction vectors; rhs_last = last entry of the rotated right-hand side
    c_old, s_old, c_cur, s_cur = 1.0, 0.0, 1.0, 0.0
    d_old = np.zeros_like(b)
    d_cur = np.zeros_like(b)
    rhs_last = eta0
    k = 0
    while k < max_iter:
        k += 1
        # one Lanczos step: column k of T is (t_k, a_k, t_{k+1})
        Ap = A @ p
        a = float(p @ Ap)
        q_next = Ap - a * q - t * q_prev
        p_next = Binv(q_next)
        t2 = float(q_next @ p_next)
        if t2 < 0.0 or t2 != t2:
            raise ValueError("minres: <v, B^-1 v> < 0 - the preconditioner is not SPD")
        t_next = np.sqrt(t2)
        # the rotations of the columns k - 2 and k - 1 act on (0, t_k, a_k): entries r_{k-2,k}, r_{k-1,k} and the pivot
        r_far = s_old * t
        mid = c_old * t
        r_near = c_cur * mid + s_cur * a
        pivot = -s_cur * mid + c_cur * a
        # the new rotation removes t_{k+1}
        c_new, s_new, r_diag = _rotation(pivot, t_next)
        if r_diag == 0.0:         # singular least-squares problem: A B^-1 singular on the Krylov space; nothing to add
            history.append(abs(rhs_last))
            break
        d_new = (p - r_near * d_cur - r_far * d_old) / r_diag
        x = x + (c_new * rhs_last) * d_new
        rhs_last = -s_new * rhs_last
        history.append(abs(rhs_last))
        if k in keep:
            iterates[k] = x.copy()
        if abs(rhs_last) <= goal or t_next == 0.0:
            break
        q_prev, q, p = q, q_next / t_next, p_next / t_next
        t = t_next
        c_old, s_old, c_cur, s_cur = c_cur, s_cur, c_new, s_new
        d_old, d_cur = d_cur, d_new
    return MinresRun(x, k, bool(history[-1] <= goal), eta0, goal, np.array(history), iterates)

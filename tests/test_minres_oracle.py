"""oracle/minres_oracle.py (the fp64 single-vector MINRES the solver loops are compared with in
test_gpu_minres_trajectory.py) against statements that trust no recurrence:

- x_k and |eta_k| for k = 1, 2, 5, 9 against the dense minimiser of <b - A x, B^-1 (b - A x)> over
  x_0 + span{B^-1 r_0, (B^-1 A) B^-1 r_0, ...}: an orthonormalised basis of the Krylov space, the normal equations solved in
  fp64; on the saddle-point system of hex 8^3 (indefinite) and on the hybridized H of the same mesh (SPD), from a zero and
  from a nonzero x_0, with an SPD preconditioner that is not the identity (diag(M)^-1 and an exact solve of the Schur
  complement B diag(M)^-1 B^T + alpha W; Jacobi on H);
- scipy.sparse.linalg.minres with M = B^-1 at the same truncations;
- the stopping rule at its edges: abs_tol above eta_0, abs_tol between two history values, a zero right-hand side,
  max_iter = 0.

Tolerance 1e-12 relative to ||x_final|| and to eta_0: the formulations agree to 1.6e-15 on the saddle-point system (K_5);
three orders of margin are left for the conditioning of the normal equations on the SPD case (Jacobi on H).  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.minres_oracle import minres

TOL = 1e-12
KS = (1, 2, 5, 9)


@pytest.fixture(scope="module")
def systems(hex_hierarchy_small):
    """name -> (A, Binv, n)"""
    from oracle.precond_oracle import sampler_schur
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
    prob = build_sampler_problem(hex_hierarchy_small, corlen=0.1, lognormal=True)
    L = prob.levels[0]
    A = SamplerOracle(prob).block_operator(0).tocsr()
    dM = 1.0 / L.M.diagonal()
    lu = spla.splu(sampler_schur(L, prob.alpha, 1.0).tocsc())

    def saddle_prec(r):
        return np.concatenate([dM * r[:L.n_u], lu.solve(r[L.n_u:])])

    H = build_hybrid_sampler_problem(hex_hierarchy_small, corlen=0.1, lognormal=True).levels[0].H.tocsr()
    dH = 1.0 / H.diagonal()
    return {"saddle": (A, saddle_prec, A.shape[0]), "spd": (H, lambda r: dH * r, H.shape[0])}


def _dense_minimiser(A, Binv, b, x0, kmax):
    """k -> (x_k, eta_k) for k = 1 .. kmax from an orthonormal basis of K_k(B^-1 A, B^-1 r_0) (Gram-Schmidt twice) and the
    normal equations of min_y <r_0 - A Q y, B^-1 (r_0 - A Q y)>"""
    r0 = b - A @ x0
    Q = np.zeros((len(b), kmax))
    AQ = np.zeros_like(Q)
    BAQ = np.zeros_like(Q)
    v = Binv(r0)
    out = {}
    for k in range(1, kmax + 1):
        for _ in range(2):
            v = v - Q[:, :k - 1] @ (Q[:, :k - 1].T @ v)
        Q[:, k - 1] = v / np.linalg.norm(v)
        AQ[:, k - 1] = A @ Q[:, k - 1]
        BAQ[:, k - 1] = Binv(AQ[:, k - 1])
        G = AQ[:, :k].T @ BAQ[:, :k]
        y = np.linalg.solve(0.5 * (G + G.T), BAQ[:, :k].T @ r0)
        rk = r0 - AQ[:, :k] @ y
        out[k] = (x0 + Q[:, :k] @ y, np.sqrt(rk @ Binv(rk)))
        v = BAQ[:, k - 1]          # B^-1 A q_k extends the space by (B^-1 A)^k B^-1 r_0
    return out


def _case(systems, name, warm, seed=0):
    A, Binv, n = systems[name]
    rng = np.random.Generator(np.random.PCG64(20261019 + seed))
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) if warm else np.zeros(n)
    return A, Binv, b, x0


@pytest.mark.parametrize("warm", [False, True], ids=["zero-guess", "nonzero-guess"])
@pytest.mark.parametrize("name", ["saddle", "spd"])
def test_iterates_are_the_dense_minimisers(systems, name, warm):
    A, Binv, b, x0 = _case(systems, name, warm)
    run = minres(A, Binv, b, x0, 0.0, 0.0, max(KS), keep=KS)
    assert run.iterations == max(KS) and not run.converged and len(run.history) == max(KS) + 1
    dense = _dense_minimiser(A, Binv, b, x0, max(KS))
    r0 = b - A @ x0
    assert abs(run.initial_norm - np.sqrt(r0 @ Binv(r0))) <= TOL * run.initial_norm
    scale = np.linalg.norm(run.x)
    for k in KS:
        xk, ek = dense[k]
        ex = np.linalg.norm(run.iterates[k] - xk) / scale
        ee = abs(run.history[k] - ek) / run.initial_norm
        print(f"dense minimiser {name} warm={warm} k={k}: x {ex:.2e}  eta {ee:.2e}")
        assert ex <= TOL and ee <= TOL, (k, ex, ee)
    # the norms decrease, and each is the norm of the true residual of its iterate
    assert np.all(np.diff(run.history) <= 0)
    for k in KS:
        rk = b - A @ run.iterates[k]
        assert abs(np.sqrt(rk @ Binv(rk)) - run.history[k]) <= TOL * run.initial_norm


@pytest.mark.parametrize("warm", [False, True], ids=["zero-guess", "nonzero-guess"])
@pytest.mark.parametrize("name", ["saddle", "spd"])
def test_iterates_equal_scipy_minres(systems, name, warm):
    A, Binv, b, x0 = _case(systems, name, warm, seed=1)
    n = len(b)
    M = spla.LinearOperator((n, n), matvec=Binv, dtype=np.float64)
    run = minres(A, Binv, b, x0, 0.0, 0.0, max(KS), keep=KS)
    scale = np.linalg.norm(run.x)
    for k in KS:
        try:
            xs, _ = spla.minres(A, b, x0=x0.copy(), M=M, rtol=1e-300, maxiter=k)
        except TypeError:          # scipy before 1.12 calls it tol
            xs, _ = spla.minres(A, b, x0=x0.copy(), M=M, tol=1e-300, maxiter=k)
        e = np.linalg.norm(run.iterates[k] - xs) / scale
        print(f"scipy {name} warm={warm} k={k}: {e:.2e}")
        assert e <= TOL, (k, e)


def test_stopping_rule_edges(systems):
    A, Binv, b, x0 = _case(systems, "saddle", False, seed=2)
    full = minres(A, Binv, b, x0, 1e-6, 0.0, 300, keep=range(301))
    h = full.history
    it = full.iterations
    assert full.converged and 5 < it < 300 and len(h) == it + 1
    assert h[it] <= 1e-6 * h[0] < h[it - 1], "stops at the FIRST iteration at or below the goal"
    assert np.array_equal(full.x, full.iterates[it]) and full.final_norm == h[it] and full.goal == 1e-6 * h[0]

    # abs_tol above eta_0: no iteration, converged, x0 returned untouched, final norm = initial norm
    warm = minres(A, Binv, b, full.iterates[3], 1e-6, 0.0, 300)
    for guess in (x0, full.iterates[3]):
        run = minres(A, Binv, b, guess, 1e-6, 2.0 * h[0], 300, keep=(0, 1))
        assert run.iterations == 0 and run.converged and np.array_equal(run.x, guess)
        assert len(run.history) == 1 and run.final_norm == run.initial_norm and set(run.iterates) == {0}
    assert abs(warm.initial_norm - h[3]) <= TOL * h[0], "restarting from x_3 starts at |eta_3|"
    # eta_0 == goal exactly: still no iteration (the rule is eta_0 <= goal)
    run = minres(A, Binv, b, x0, 1e-6, h[0], 300)
    assert run.iterations == 0 and run.converged

    # abs_tol between two history values wins over the smaller relative goal: stop exactly there, with the same iterate
    for k in (1, 4, it - 1):
        run = minres(A, Binv, b, x0, 1e-6, np.sqrt(h[k] * h[k - 1]), 300)
        assert h[k] < run.goal < h[k - 1]
        assert run.iterations == k and run.converged and np.array_equal(run.x, full.iterates[k])
        assert np.array_equal(run.history, h[:k + 1])
    # ... and abs_tol below the relative goal has no say
    run = minres(A, Binv, b, x0, 1e-6, 1e-9 * h[0], 300)
    assert run.iterations == it and np.array_equal(run.x, full.x)
    # a goal that equals a history value exactly stops AT that iteration (<=, not <)
    run = minres(A, Binv, b, x0, 0.0, h[4], 300)
    assert run.iterations == 4 and run.converged

    # a zero right-hand side (zero guess): x0, 0 iterations, converged - also with both tolerances zero
    for rel, ab in ((1e-6, 1e-12), (0.0, 0.0)):
        run = minres(A, Binv, np.zeros_like(b), None, rel, ab, 300)
        assert run.iterations == 0 and run.converged and not np.any(run.x) and run.initial_norm == 0.0

    # max_iter = 0: x0 back, not converged; max_iter = k: x_k, not converged
    run = minres(A, Binv, b, full.iterates[3], 1e-6, 0.0, 0)
    assert run.iterations == 0 and not run.converged and np.array_equal(run.x, full.iterates[3])
    run = minres(A, Binv, b, x0, 1e-6, 0.0, 7)
    assert run.iterations == 7 and not run.converged and np.array_equal(run.x, full.iterates[7])

    # scaling b scales everything and changes no count (what the mixed batches of the GPU test rely on)
    run = minres(A, Binv, 1e-8 * b, x0, 1e-6, 0.0, 300)
    assert run.iterations == it and np.linalg.norm(run.x - 1e-8 * full.x) <= TOL * np.linalg.norm(1e-8 * full.x)


def test_an_indefinite_preconditioner_is_refused(systems):
    A, Binv, b, x0 = _case(systems, "spd", False)
    with pytest.raises(ValueError):
        minres(A, lambda r: -Binv(r), b, x0, 1e-6, 0.0, 10)

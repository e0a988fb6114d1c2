"""The numpy twin of the adjoint gradients (parelagmc_amd/fe/darcy_adjoint.py) against central differences of the oracle's
direct solves (oracle/darcy_oracle.py).  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.darcy_oracle import DarcyOracle  # noqa: E402
from parelagmc_amd.fe import darcy_adjoint  # noqa: E402

import darcy_gradient_cases as cases  # noqa: E402

STEP = 1e-5          # relative step: k -> k (1 +- STEP d) per entry
# Largest relative error of a directional derivative measured over all cases below: 8.5e-9 (QoI), 7.9e-9 (log-likelihood),
# relative to |g . d| + 1e-3 |g| |d|.  The bound is 100 x that, and never looser than 1e-5.
TOL_Q = min(100 * 8.5e-9, 1e-5)
TOL_LL = min(100 * 7.9e-9, 1e-5)


def _directional_errors(fun, g, k, wrt_log, rng):
    """relative errors of g against central differences of fun along five seeded random directions"""
    out = []
    for _ in range(5):
        d = rng.standard_normal(k.size)
        dk = STEP * k * d
        fd = (fun(k + dk) - fun(k - dk)) / 2.0
        v = STEP * d if wrt_log else dk          # d log k = dk / k
        gd = float(g @ v)
        out.append(abs(fd - gd) / (abs(gd) + 1e-3 * np.linalg.norm(g) * np.linalg.norm(v)))
    return out


@pytest.mark.parametrize("wrt_log", [False, True])
@pytest.mark.parametrize("qoi", ["eff_perm", "p_int"])
@pytest.mark.parametrize("k_divides", [True, False])
@pytest.mark.parametrize("mesh", ["hex4", "hex543", "tet1"])
def test_gradient_matches_central_differences_of_the_oracle(mesh, k_divides, qoi, wrt_log):
    """A wrong sign, a missing c', a missing essential-value term or a transposed M_e is an O(1) error here.  Measured:
    at most 8.5e-9 relative over the 24 cases x 5 directions."""
    h, dp = cases.problem(mesh, k_divides, qoi)
    assert np.abs(dp.levels[0].ess_data).max() > 0.0
    rng = np.random.default_rng(17)
    k = np.exp(rng.standard_normal(dp.levels[0].n_p))
    orc = DarcyOracle(dp)
    g, Q, _, lam = darcy_adjoint.gradient(dp, 0, k, wrt_log=wrt_log, return_all=True)
    assert abs(Q - orc.solve_fwd(0, k)[0]) <= 1e-11 * abs(Q)
    assert np.all(lam[:dp.levels[0].n_u][dp.levels[0].ess_mask.astype(bool)] == 0.0)
    errs = _directional_errors(lambda kk: orc.solve_fwd(0, kk)[0], g, k, wrt_log, rng)
    print(f"{mesh} k_divides={k_divides} {qoi} wrt_log={wrt_log}: max rel err {max(errs):.2e}")
    assert max(errs) < TOL_Q


@pytest.mark.parametrize("wrt_log", [False, True])
@pytest.mark.parametrize("k_divides", [True, False])
def test_loglik_gradient_matches_central_differences_of_the_oracle(k_divides, wrt_log):
    """log-likelihood from the oracle's pressure and this test's own observation functionals.  Measured: at most 7.9e-9."""
    h, dp = cases.problem("hex4", k_divides, "eff_perm")
    L = dp.levels[0]
    Gobs = cases.two_cell_observations(h)
    norm = 1.0 / np.asarray(Gobs.sum(axis=1)).ravel()
    rng = np.random.default_rng(23)
    k = np.exp(rng.standard_normal(L.n_p))
    orc = DarcyOracle(dp)
    noise = 0.01

    def G_of(kk):
        return norm * (Gobs @ orc.solve_fwd(0, kk, return_solution=True)[2][L.n_u:])

    data = G_of(np.exp(rng.standard_normal(L.n_p)))          # observations of another field: a nonzero misfit

    def loglik(kk):
        r = G_of(kk) - data
        return -float(r @ r) / (2.0 * noise)

    ll, G, g = darcy_adjoint.loglik_gradient(dp, 0, k, Gobs, data, noise, wrt_log=wrt_log)
    assert abs(ll - loglik(k)) <= 1e-10 * abs(ll)
    assert np.allclose(G, G_of(k), rtol=1e-11, atol=0.0)
    errs = _directional_errors(loglik, g, k, wrt_log, rng)
    print(f"loglik k_divides={k_divides} wrt_log={wrt_log}: max rel err {max(errs):.2e}")
    assert max(errs) < TOL_LL


@pytest.mark.parametrize("k_divides", [True, False])
@pytest.mark.parametrize("mesh", ["hex4", "hex543", "tet1"])
def test_element_matrices_assemble_to_the_oracles_mass_matrix(mesh, k_divides):
    """sum_e c_e P_e^T M_e P_e == DarcyOracle.mass, entry by entry"""
    import scipy.sparse as sp
    h, dp = cases.problem(mesh, k_divides)
    L = dp.levels[0]
    faces, Me = darcy_adjoint.element_matrices(L)
    assert faces.shape == (L.n_p, 6 if mesh.startswith("hex") else 4)
    B = L.B.tocsr()
    for e in range(L.n_p):                                    # the faces of an element: the columns of its row of B
        assert np.array_equal(faces[e], np.sort(B.indices[B.indptr[e]:B.indptr[e + 1]]))
    assert np.array_equal(Me, Me.transpose(0, 2, 1))
    rng = np.random.default_rng(5)
    k = np.exp(rng.standard_normal(L.n_p))
    c = 1.0 / k if k_divides else k
    n_fe = faces.shape[1]
    rows = np.repeat(faces, n_fe, axis=1).ravel()
    cols = np.tile(faces, (1, n_fe)).ravel()
    M = sp.csr_matrix(((c[:, None, None] * Me).ravel(), (rows, cols)), shape=(L.n_u, L.n_u))
    ref = DarcyOracle(dp).mass(0, k)
    diff = (M - ref).tocoo()
    assert ref.nnz > 0
    refd = ref.toarray()
    assert np.all(np.abs(diff.data) <= 1e-14 * np.abs(refd[diff.row, diff.col]))

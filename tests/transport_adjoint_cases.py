"""Shared cases of the transport-adjoint tests (test_transport_adjoint_twin.py, test_gpu_transport_adjoint.py): the seeds, the
cached twin results of fe.transport.advance_adjoint on the cases of transport_cases.py, the chain to a gradient in k (direct
solve, advance_adjoint, adjoint solve, mass sensitivity) and the measured tolerances.  No tests here."""
import functools
import itertools

import numpy as np
import scipy.sparse.linalg as spla

import transport_cases as tc
from parelagmc_amd.fe import darcy_adjoint as dad
from parelagmc_amd.fe import transport as tw

NAMES = tc.NAMES
NREPORT = tc.NREPORT
SEED_NAMES = ("curve_bar", "stored_bar", "c_bar")
COMBOS = tuple(c for n in (1, 2, 3) for c in itertools.combinations(SEED_NAMES, n))     # every seed combination: 7
FD_CASES = ("hex1", "quad1", "agg2_2", "tri1", "agg3_1")        # 6, 4, ragged, 3, ragged row entries; 3 to 89 steps
FD_STEP = 1e-5
GRAD_CASES = (("hex1", False), ("quad0", False), ("agg2_1", False), ("hex1", True))      # (case, hybridized handle)


@functools.lru_cache(maxsize=None)
def all_seeds(name):
    """one random seed of every kind for the case's five columns"""
    c = tc.case(name)
    rng = np.random.Generator(np.random.PCG64(20261021 + NAMES.index(name)))
    s = dict(curve_bar=rng.standard_normal((5, NREPORT)), stored_bar=rng.standard_normal(5),
             c_bar=rng.standard_normal((5, c.mesh.n_elem)))
    for a in s.values():
        a.setflags(write=False)
    return s


def seeds(name, combo, cols=slice(None)):
    return {k: np.ascontiguousarray(all_seeds(name)[k][cols]) for k in combo}


@functools.lru_cache(maxsize=None)
def twin(name, combo=SEED_NAMES, longdouble=False):
    """advance_adjoint on the case's five columns; the np.longdouble run takes the float64 run's decisions"""
    c = tc.case(name)
    if not longdouble:
        return tw.advance_adjoint(c.mesh, c.u, c.t_end, tc.CFL, NREPORT, **seeds(name, combo))
    return tw.advance_adjoint(c.mesh, c.u, c.t_end, tc.CFL, NREPORT, **seeds(name, combo), dtype=np.longdouble,
                              decisions=twin(name, combo)["decisions"])


def adjoint_deviation(got, ref, cols=slice(None)):
    """largest difference of u_bar and c0_bar of two results, per column relative to the column's largest |u_bar| of ref.  A
    column whose u_bar is zero (zero flux, a status that is not OK) must have a zero u_bar; its c0_bar (lam^N carried
    through unchanged) is compared relative to its own largest entry"""
    worst = 0.0
    gu, gc = np.asarray(got["u_bar"]), np.asarray(got["c0_bar"])
    ru, rc = np.asarray(ref["u_bar"])[cols], np.asarray(ref["c0_bar"])[cols]
    nf = ru.shape[1]
    for b in range(len(ru)):
        scale = float(np.abs(ru[b]).max())
        du, dc = float(np.abs(gu[b, :nf] - ru[b]).max()), float(np.abs(gc[b] - rc[b]).max())
        if scale > 0:
            worst = max(worst, max(du, dc) / scale)
        else:
            assert du == 0.0, (b, du)
            worst = max(worst, dc / max(float(np.abs(rc[b]).max()), np.finfo(np.float64).tiny))
    return worst


def rounding_deviation(name, combo=SEED_NAMES):
    return adjoint_deviation(twin(name, combo), twin(name, combo, longdouble=True))


# ---- the chain to a gradient in k ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(kind):
    from oracle.darcy_oracle import DarcyOracle
    return DarcyOracle(tc.problem(kind))


def chain_gradient(name, b, combo, wrt_log, flux_noise=None, decisions=None, nreport=NREPORT):
    """(grad, the advance_adjoint result) of J = <curve_bar, curve> + stored_bar stored [+ <c_bar, c>] for column b of the
    case: a direct solve with k[b], the twin's adjoint on its flux (times 1 + flux_noise), a direct adjoint solve with
    [u_bar; 0] (essential rows zero), the mass sensitivity"""
    c = tc.case(name)
    dp = tc.problem(c.kind)
    L = dp.levels[c.level]
    A, rhs, ess = dad.assemble(dp, c.level, c.k[b])
    lu = spla.splu(A)
    x = lu.solve(rhs)
    if flux_noise is not None:
        x[:L.n_u] *= 1 + flux_noise
    sd = {k: v[:, :nreport] if k == "curve_bar" else v for k, v in seeds(name, combo, [b]).items()}
    r = tw.advance_adjoint(c.mesh, x[None, :L.n_u], c.t_end, tc.CFL, nreport, **sd, decisions=decisions)
    rhs_adj = np.zeros(L.n_u + L.n_p)
    rhs_adj[:L.n_u] = r["u_bar"][0]
    rhs_adj[ess] = 0.0
    lam = lu.solve(rhs_adj)
    return dad.mass_sensitivity(L, c.k[b], x, lam, dp.k_divides, wrt_log)[0], r


def gradient_perturbation_change(name, b, combo, wrt_log, size=1e-9, reps=3):
    """largest relative change (of the largest entry) of the chain's gradient when every flux is multiplied by
    1 + size N(0, 1); draws that change a step count are left out"""
    g0, r0 = chain_gradient(name, b, combo, wrt_log)
    rng = np.random.Generator(np.random.PCG64(11 + b))
    worst = 0.0
    for _ in range(reps):
        g, r = chain_gradient(name, b, combo, wrt_log, flux_noise=size * rng.standard_normal(tc.case(name).mesh.n_face))
        if r["nsteps"][0] == r0["nsteps"][0]:
            worst = max(worst, float(np.abs(g - g0).max() / np.abs(g0).max()))
    return worst


def fd_check(name, b, combo, h=FD_STEP):
    """(relative difference, kept) of the chain's gradient in log k along a random direction against central differences of
    J through the oracle's direct solve and the forward twin at k exp(+-h dk); kept False: a step count or a sign of g
    changed between the two"""
    c = tc.case(name)
    orc = oracle(c.kind)
    n_u = c.mesh.n_face
    rng = np.random.Generator(np.random.PCG64(31 * NAMES.index(name) + b))
    dk = rng.standard_normal(c.k.shape[1])
    sd = seeds(name, combo, [b])

    def J(sign):
        u = orc.solve_fwd(c.level, c.k[b] * np.exp(sign * h * dk), True)[2][:n_u]
        r = tw.advance_adjoint(c.mesh, u[None], c.t_end, tc.CFL, NREPORT, **sd)
        val = sum(float((np.atleast_1d(v[0]) * np.atleast_1d(r[k[:-4]][0])).sum()) for k, v in sd.items())
        return val, r["decisions"][0]

    (jp, dp_), (jm, dm) = J(+1), J(-1)
    kept = dp_ is not None and dm is not None and dp_[0] == dm[0] and np.array_equal(dp_[1], dm[1])
    fd = (jp - jm) / (2 * h)
    an = float(chain_gradient(name, b, combo, True)[0] @ dk)
    return abs(fd - an) / max(abs(fd), abs(an)), kept


# ---- measured tolerances (re-measured by test_transport_adjoint_twin.py::test_recorded_tolerances) ------
# Largest deviation of the float64 twin's u_bar and c0_bar from the np.longdouble twin on the float64 twin's decisions, over
# all nine cases, five columns and all three seeds at once, relative to the column's largest |u_bar|.  The kernel may differ
# from the twin by 16 x that (the section 21 convention: the factor covers the device's divisions).  Measured: 3.9e-15 (hex0).
ADJ_ROUNDING_RAW = 4.0e-15
TOL_KA = 16 * ADJ_ROUNDING_RAW
# Largest relative difference between the chain's gradient in log k and central differences (h = 1e-5) through the oracle,
# over FD_CASES, the four lognormal columns and the seeds on the curve, on stored and on c separately.  The test allows 10 x.
# Measured: 4.6e-9 (agg3_1, column 0, the seed on stored); no column changed a step count or a sign of g between k exp(+-h dk).
FD_RAW = 5.0e-9
# Largest relative change of the chain's gradient (in k and in log k, GRAD_CASES, the four columns) under a relative flux
# perturbation of 1e-9 - the accuracy at which a 1e-12 solve holds x.  A 1e-12 device solve may differ from the chain by 10 x.
# Measured: 6.2e-9 (quad0, log k); seeds on the curve and on stored together, three draws per column.
GRAD_PERTURBATION_RAW = 6.5e-9
TOL_G = 10 * GRAD_PERTURBATION_RAW
# Largest change of grad of pmc_darcy_transport_gradient, relative to its largest entry, when a column moves between launches
# of 1, 2 and 4 columns (hex1, 1e-12 solves).  The change is that of the two Darcy solves, whose paths depend on the launch
# width - the entry is bit for bit the composition of pmc_transport_run_adjoint and pmc_darcy_solve_gradient at every width,
# and x and lam of the latter move by 5.6e-16 and 1.3e-15.  Measured on the MI355X: 2.3e-15; the test allows 16 x.
WIDTH_RAW = 2.5e-15

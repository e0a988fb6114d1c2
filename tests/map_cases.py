"""Problems shared by tests/test_map_estimate.py and tests/test_gpu_map_estimate.py (no tests here): lognormal SPDE priors on
the small meshes, two observations (two_cell_observations), data from a known xi_true plus noise."""
import functools

import numpy as np

import darcy_gradient_cases as dcases
import sampler_adjoint_cases as scases
from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy, build_sampler_problem, darcy_adjoint, sampler_adjoint

# (name) -> (mesh, level, xi_level, noise)
CASES = {
    "ragged-00": ("ragged", 0, 0, 1e-2),
    "ragged-10": ("ragged", 1, 0, 1e-3),
    "tet1-00": ("tet1", 0, 0, 1e-2),
    "tet1-11-small-noise": ("tet1", 1, 1, 1e-4),        # the backtracking case, from 2 * randn
    "ragged-00-small-noise": ("ragged", 0, 0, 1e-4),    # Gauss-Newton with a large residual: the max_newton case
    "hex84-00": ("hex84", 0, 0, 1e-2),
}


@functools.lru_cache(maxsize=None)
def problems(mesh):
    """(hierarchy, DarcyProblem with seeded essential fluxes, lognormal SamplerProblem, [Gobs per level])"""
    if mesh == "tet1":
        h, dp = dcases.problem("tet1")
    else:
        h = (build_hierarchy(box_mesh([5, 3, 2], [2, 2, 2], "hex"), 1) if mesh == "ragged"
             else build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1))
        dp = build_darcy_problem(h, dcases.ESS, dcases.OBS, dcases.INFLOW)
        rng = np.random.default_rng(3)
        for L in dp.levels:
            L.ess_data[:] = np.where(L.ess_mask.astype(bool), rng.standard_normal(L.n_u), 0.0)
    sp = build_sampler_problem(h, corlen=scases.CORLEN, lognormal=True)
    Gobs = [dcases.two_cell_observations(h, level) for level in range(dp.n_mc_levels)]
    return h, dp, sp, Gobs


@functools.lru_cache(maxsize=None)
def kl_prior(mesh):
    """a lognormal KL prior (3 x 3 x 3 analytic modes) on the mesh of problems(mesh)"""
    from parelagmc_amd.fe import build_kl_sampler_problem
    return build_kl_sampler_problem(problems(mesh)[0], "analytic", nmodes=[3, 3, 3], corlen=scases.CORLEN, lognormal=True)


@functools.lru_cache(maxsize=None)
def case(name, prior="spde"):
    """(dp, sp, Gobs of the level, level, xi_level, noise, data, n_xi): data = G(Eval(xi_true)) + sqrt(noise) * randn;
    prior "kl": the KL prior of the mesh in place of the SPDE one"""
    mesh, level, xi_level, noise = CASES[name]
    h, dp, sp, Gobs = problems(mesh)
    if prior == "kl":
        sp = kl_prior(mesh)
    rng = np.random.default_rng(101)
    n_xi = sp.levels[xi_level].n_s
    xi_true = rng.standard_normal(n_xi)
    k = sampler_adjoint.eval_forward(sp, level, xi_level, xi_true)
    G = darcy_adjoint.loglik_gradient(dp, level, k, Gobs[level], np.zeros(2), noise, wrt_log=True)[1]
    data = np.asarray(G) + np.sqrt(noise) * rng.standard_normal(2)
    return dp, sp, Gobs[level], level, xi_level, noise, data, n_xi


def starts(name, nb, scale=0.5, seed=103):
    """column 0 is the zero start, the others scale * randn"""
    n_xi = case(name)[7]        # (a KL prior's xi has the SPDE prior's length)
    x = scale * np.random.default_rng(seed).standard_normal((nb, n_xi))
    x[0] = 0.0
    return x

"""Data shared by tests/test_condition_derivatives.py and tests/test_gpu_condition_derivatives.py (no tests here): the hard data
of the conditioned inverse problems - 5 point observations of log k on the meshes of tests/map_cases.py - and their twins."""
import functools

import numpy as np

import map_cases as mc
from parelagmc_amd.fe.condition import Conditioner, pick_observation_elements, point_observations

NOBS = 5


@functools.lru_cache(maxsize=None)
def hard_data(mesh):
    """(H0, y): NOBS point observations with distinct coarse ancestors, y ~ N(0, 0.5^2)"""
    h = mc.problems(mesh)[0]
    H0 = point_observations(h.spaces[0].n_s, pick_observation_elements(h, NOBS, 5))
    return H0, np.random.default_rng(7).normal(0.0, 0.5, NOBS)


@functools.lru_cache(maxsize=None)
def twin_conditioner(mesh, prior="spde"):
    """fe.condition.Conditioner of the lognormal prior of map_cases (prior "kl": the KL prior of the mesh)"""
    sp = mc.kl_prior(mesh) if prior == "kl" else mc.problems(mesh)[2]
    H0, y = hard_data(mesh)
    return Conditioner(sp, H0, y)

"""ctypes binding of libpmc.so (include/pmc.h) - the reference-side stub a ParELAGMC maintainer
would write in C++ is shown in INTEGRATION.md; this is the same binding for the Python test
harness and launcher.  There is NO CPU fallback: if the library cannot be loaded, or no GPU is
visible when a context is created, the call raises.
"""
from __future__ import annotations

import ctypes as C
import weakref
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpmc.so")

PMC_MEM_HOST, PMC_MEM_DEVICE = 0, 1
PMC_PROJ_NONE, PMC_PROJ_GATHER, PMC_PROJ_L2 = 0, 1, 2


class PmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libpmc error {code}: {msg}")
        self.code = code


class pmc_csr(C.Structure):
    _fields_ = [("nrows", C.c_int32), ("ncols", C.c_int32), ("rowptr", C.POINTER(C.c_int32)),
                ("colind", C.POINTER(C.c_int32)), ("vals", C.POINTER(C.c_double))]


class pmc_solver_opts(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("max_iter", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double),
                ("cheb_degree_M", C.c_int32), ("cheb_ratio_M", C.c_double),
                ("mg_smooth_degree", C.c_int32), ("mg_smooth_ratio", C.c_double),
                ("mg_coarse_degree", C.c_int32), ("mg_coarse_ratio", C.c_double), ("check_every", C.c_int32),
                ("use_graph", C.c_int32), ("schur_scale", C.c_double), ("mg_coarsening", C.c_int32), ("mini_max_rows", C.c_int32),
                ("two_streams", C.c_int32), ("precond_storage", C.c_int32)]


PMC_ABI_VERSION = 3          # include/pmc.h: layout of pmc_solver_opts / pmc_stats these classes restate
PMC_STORAGE_FP32, PMC_STORAGE_FP64 = 0, 1
# enum pmc_solve_path: the loops pmc_solve_path_count counts
PMC_PATH_MINI, PMC_PATH_GRAPH, PMC_PATH_LATE, PMC_PATH_INDEXED, PMC_PATH_WINDOW, PMC_PATH_PLAIN = range(6)
PMC_COUNT_GRAPH_REPLAYS, PMC_COUNT_POLLS = 6, 7     # ... events, not solves: graph launches, convergence polls
# ... launches that took a size-gated form: non-temporal operator / polynomial / flat kernels, a fused-dot grid the bound cut,
# the block operator's two-stage dot, a tracer walk or upload in more than one piece
(PMC_COUNT_NT_OPERATOR, PMC_COUNT_NT_POLY, PMC_COUNT_NT_FLAT, PMC_COUNT_BOUNDED_GRID, PMC_COUNT_TWO_STAGE_DOT,
 PMC_COUNT_TRACER_SPLIT) = range(8, 14)


class pmc_stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("initial_norm", C.c_double),
                ("final_norm", C.c_double), ("solve_ms", C.c_double), ("setup_ms", C.c_double)]


class pmc_sampler_level(C.Structure):
    _fields_ = [("n_u", C.c_int32), ("n_s", C.c_int32), ("M", pmc_csr), ("B", pmc_csr),
                ("w_diag", C.POINTER(C.c_double)), ("P", pmc_csr)]


class pmc_hybrid_level(C.Structure):
    _fields_ = [("n_lambda", C.c_int32), ("n_s", C.c_int32), ("H", pmc_csr), ("G", pmc_csr),
                ("z_diag", C.POINTER(C.c_double)), ("w_diag", C.POINTER(C.c_double)), ("P", pmc_csr)]


class pmc_hybrid_elements(C.Structure):
    _fields_ = [("n_u", C.c_int32), ("n_s", C.c_int32), ("M_pattern", pmc_csr), ("c_ptr", C.POINTER(C.c_int32)),
                ("c_elem", C.POINTER(C.c_int32)), ("c_val", C.POINTER(C.c_double)), ("B", pmc_csr),
                ("w_diag", C.POINTER(C.c_double)), ("P", pmc_csr)]


class pmc_kl_level(C.Structure):
    _fields_ = [("n_s", C.c_int32), ("w_diag", C.POINTER(C.c_double)), ("P", pmc_csr)]


class pmc_kl_eigs_opts(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int32), ("guard", C.c_int32), ("degree", C.c_int32),
                ("seed", C.c_uint64)]


class pmc_kl_eigs_info(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("block_products", C.c_int32), ("converged", C.c_int32),
                ("max_residual_rel", C.c_double), ("gap_rel", C.c_double), ("seconds", C.c_double)]


class pmc_darcy_level(C.Structure):
    _fields_ = [("n_u", C.c_int32), ("n_p", C.c_int32), ("M_pattern", pmc_csr), ("c_ptr", C.POINTER(C.c_int32)),
                ("c_elem", C.POINTER(C.c_int32)), ("c_val", C.POINTER(C.c_double)), ("B", pmc_csr),
                ("rhs", C.POINTER(C.c_double)), ("ess_mask", C.POINTER(C.c_uint8)),
                ("ess_data", C.POINTER(C.c_double)), ("obs", C.POINTER(C.c_double)), ("P", pmc_csr)]


class pmc_tracer_mesh(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_elem", C.c_int32), ("n_face", C.c_int32), ("elem_face", C.POINTER(C.c_int32)),
                ("elem_sign", C.POINTER(C.c_int8)), ("face_elem", C.POINTER(C.c_int32)), ("geom", C.POINTER(C.c_double)),
                ("porosity", C.POINTER(C.c_double))]


class pmc_transport_mesh(C.Structure):
    _fields_ = [("n_elem", C.c_int32), ("n_face", C.c_int32), ("rowptr", C.POINTER(C.c_int32)), ("col", C.POINTER(C.c_int32)),
                ("val", C.POINTER(C.c_double)), ("pore_volume", C.POINTER(C.c_double)), ("c0", C.POINTER(C.c_double)),
                ("c_in", C.POINTER(C.c_double)), ("outlet", C.POINTER(C.c_uint8)), ("weight", C.POINTER(C.c_double))]


class pmc_transport_params(C.Structure):
    _fields_ = [("t_end", C.c_double), ("cfl", C.c_double), ("nreport", C.c_int32), ("max_steps", C.c_int32)]


# every symbol include/pmc.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
_DP = C.c_void_p   # double* that may be a host or a device address
SYMBOLS = {
    "pmc_version": (C.c_int, []),
    "pmc_last_error": (C.c_char_p, []),
    "pmc_solver_opts_default": (None, [C.POINTER(pmc_solver_opts)]),
    "pmc_abi_version": (C.c_int, []),
    "pmc_krylov_z_bytes": (C.c_int, []),
    "pmc_sampler_krylov_z_bytes": (C.c_int, [_VP]),
    "pmc_darcy_krylov_z_bytes": (C.c_int, [_VP]),
    "pmc_kernel_launches": (C.c_uint64, []),
    "pmc_fused_lanczos_solves": (C.c_uint64, []),
    "pmc_adopted_rhs_solves": (C.c_uint64, []),
    "pmc_fused_field_evals": (C.c_uint64, []),
    "pmc_solve_path_count": (C.c_uint64, [C.c_int]),
    "pmc_ctx_create": (C.c_int, [C.c_int, C.POINTER(_VP)]),
    "pmc_ctx_create_abi": (C.c_int, [C.c_int, C.c_int, C.POINTER(_VP)]),
    "pmc_ctx_destroy": (None, [_VP]),
    "pmc_ctx_synchronize": (C.c_int, [_VP]),
    "pmc_ctx_stream": (_VP, [_VP]),
    "pmc_ctx_device": (C.c_int, [_VP]),
    "pmc_timer_start": (C.c_int, [_VP]),
    "pmc_timer_stop": (C.c_int, [_VP, C.POINTER(C.c_double)]),
    "pmc_malloc": (C.c_int, [_VP, C.c_size_t, C.POINTER(_VP)]),
    "pmc_free": (C.c_int, [_VP, _VP]),
    "pmc_memcpy_h2d": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "pmc_memcpy_d2h": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "pmc_rng_seed": (C.c_int, [_VP, C.c_uint64, C.c_int, C.c_int]),
    "pmc_normal_fill": (C.c_int, [_VP, C.c_double, C.c_double, C.c_uint64, C.c_uint32, C.c_int, C.c_int, _DP, C.c_int]),
    "pmc_sampler_create": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(pmc_sampler_level), C.c_double, C.c_double,
                                     C.c_int, C.POINTER(pmc_solver_opts), C.POINTER(_VP)]),
    "pmc_sampler_create_hybrid": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_hybrid_level), C.c_double, C.c_double, C.c_int,
                                            C.POINTER(pmc_solver_opts), C.POINTER(_VP)]),
    "pmc_sampler_is_hybrid": (C.c_int, [_VP]),
    "pmc_sampler_create_kl": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_kl_level), C.c_int, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.c_int, C.POINTER(_VP)]),
    "pmc_sampler_is_kl": (C.c_int, [_VP]),
    "pmc_kl_eigs_opts_default": (None, [C.POINTER(pmc_kl_eigs_opts)]),
    "pmc_kl_matern_apply": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pmc_kl_matern_eigs": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                     C.POINTER(pmc_kl_eigs_opts), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(pmc_kl_eigs_info)]),
    "pmc_hybrid_build": (C.c_int, [C.POINTER(pmc_hybrid_elements), C.c_double, C.POINTER(_VP)]),
    "pmc_hybrid_system_level": (C.c_int, [_VP, C.POINTER(pmc_hybrid_level)]),
    "pmc_hybrid_system_destroy": (None, [_VP]),
    "pmc_sampler_create_hybrid_from_elements": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_hybrid_elements), C.c_double, C.c_double,
                                                          C.c_int, C.POINTER(pmc_solver_opts), C.POINTER(_VP)]),
    "pmc_sampler_smoother_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pmc_sampler_smoother_bytes": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pmc_sampler_vcycle_info": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "pmc_sampler_vcycle_level": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "pmc_sampler_vcycle_prolongator": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_double)]),
    "pmc_sampler_destroy": (None, [_VP]),
    "pmc_sampler_set_projection": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(pmc_csr), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double), C.c_int]),
    "pmc_sampler_num_levels": (C.c_int, [_VP]),
    "pmc_sampler_xi_size": (C.c_int, [_VP, C.c_int]),
    "pmc_sampler_sample_size": (C.c_int, [_VP, C.c_int]),
    "pmc_sampler_batch_width": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_batch_width": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_set_operator_timing": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_operator_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pmc_darcy_operator_bytes": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pmc_darcy_poly_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pmc_darcy_poly_bytes": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pmc_sampler_nnz": (C.c_int64, [_VP, C.c_int]),
    "pmc_sampler_true_p": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_csr)]),
    "pmc_sampler_sample": (C.c_int, [_VP, C.c_int, C.c_uint64, C.c_int, _DP, C.c_int]),
    "pmc_sampler_eval": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, C.c_int, _DP, C.c_int,
                                   C.POINTER(pmc_stats)]),
    "pmc_sampler_mult": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.c_int, C.c_int, C.POINTER(pmc_stats)]),
    "pmc_sampler_eval_adjoint": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, C.POINTER(pmc_stats)]),
    "pmc_sampler_eval_tangent": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, C.POINTER(pmc_stats)]),
    "pmc_sampler_is_lognormal": (C.c_int, [_VP]),
    "pmc_sampler_logprior_gradient": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.POINTER(C.c_double), C.c_int]),
    "pmc_sampler_logprior_hessvec": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.c_int]),
    "pmc_sampler_apply_preconditioner": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.c_int]),
    "pmc_sampler_apply_operator": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.c_int, C.c_int, C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]),
    "pmc_sampler_set_operator_timing": (C.c_int, [_VP, C.c_int]),
    "pmc_sampler_operator_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pmc_sampler_operator_event_overhead": (C.c_int, [_VP, C.POINTER(C.c_double)]),
    "pmc_conditioner_create": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_csr), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(_VP)]),
    "pmc_conditioner_destroy": (None, [_VP]),
    "pmc_conditioner_num_obs": (C.c_int, [_VP]),
    "pmc_conditioner_level": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_double)]),
    "pmc_conditioner_apply": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, C.c_int]),
    "pmc_conditioner_apply_tangent": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int]),
    "pmc_conditioner_apply_adjoint": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int]),
    "pmc_conditioner_enable_derivatives": (C.c_int, [_VP, C.c_int]),
    "pmc_conditioner_derivatives_enabled": (C.c_int, [_VP]),
    "pmc_sampler_set_conditioner": (C.c_int, [_VP, _VP]),
    "pmc_field_stats_create": (C.c_int, [_VP, C.c_int, _DP, C.c_int, C.POINTER(_VP)]),
    "pmc_field_stats_destroy": (None, [_VP]),
    "pmc_field_stats_reset": (C.c_int, [_VP]),
    "pmc_field_stats_accumulate": (C.c_int, [_VP, C.c_int, _DP, C.c_int]),
    "pmc_field_stats_run": (C.c_int, [_VP, C.c_uint64, C.c_int64]),
    "pmc_field_stats_read": (C.c_int, [_VP, _DP, _DP, _DP, C.POINTER(C.c_int64), C.c_int]),
    "pmc_field_stats_read_sums": (C.c_int, [_VP, _DP, C.POINTER(C.c_int64), C.c_int]),
    "pmc_field_stats_chi_dot": (C.c_int, [_VP, C.c_int, _DP, _DP, C.c_int]),
    "pmc_sampler_l2_error": (C.c_int, [_VP, C.c_int, C.c_int, _DP, C.c_double, _DP, C.c_int]),
    "pmc_sampler_max_error": (C.c_int, [_VP, C.c_int, C.c_int, _DP, C.c_double, _DP, C.c_int]),
    "pmc_sampler_set_output_hierarchy": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_csr), C.POINTER(C.c_double)]),
    "pmc_darcy_create": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(pmc_darcy_level), C.c_int,
                                   C.POINTER(pmc_solver_opts), C.POINTER(_VP)]),
    "pmc_darcy_create_hybrid": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(pmc_darcy_level), C.c_int,
                                          C.POINTER(pmc_solver_opts), C.POINTER(_VP)]),
    "pmc_darcy_destroy": (None, [_VP]),
    "pmc_darcy_num_dofs": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_num_pressure_dofs": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_nnz": (C.c_int64, [_VP, C.c_int]),
    "pmc_darcy_solve_fwd": (C.c_int, [_VP, C.c_int, C.c_int, _DP, C.POINTER(C.c_double), C.POINTER(C.c_double), _DP,
                                      C.c_int, C.POINTER(pmc_stats)]),
    "pmc_darcy_solve_fwd_pressure": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(pmc_stats)]),
    "pmc_level_fields_create": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "pmc_level_fields_destroy": (None, [_VP]),
    "pmc_level_fields_reset": (C.c_int, [_VP]),
    "pmc_level_fields_accumulate": (C.c_int, [_VP, C.c_int, _DP, _DP, C.c_int]),
    "pmc_level_fields_accumulate_weighted": (C.c_int, [_VP, C.c_int, _DP, _DP, _DP, _DP, C.c_int]),
    "pmc_level_fields_read_sums": (C.c_int, [_VP, _DP, C.POINTER(C.c_int64), C.c_int]),
    "pmc_level_fields_size": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pmc_level_fields_parents": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "pmc_darcy_apply_preconditioner": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int]),
    "pmc_darcy_apply_operator": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int]),
    "pmc_darcy_vcycle_level": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "pmc_darcy_vcycle_prolongator": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_double)]),
    "pmc_darcy_set_observations": (C.c_int, [_VP, C.c_int, C.POINTER(pmc_csr)]),
    "pmc_darcy_num_observations": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_compute_G": (C.c_int, [_VP, C.c_int, C.c_int, _DP, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_int, C.POINTER(pmc_stats)]),
    "pmc_darcy_mass_sensitivity_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pmc_darcy_mass_sensitivity_bytes": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pmc_darcy_mass_sensitivity": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, _DP, C.c_int]),
    "pmc_darcy_mass_tangent_time": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pmc_darcy_mass_tangent_bytes": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pmc_darcy_mass_tangent": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, _DP, C.c_int]),
    "pmc_darcy_gn_hessvec": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, _DP, C.c_double, C.c_int, _DP, C.POINTER(C.c_double),
                                       _DP, C.c_int, C.POINTER(pmc_stats), C.POINTER(pmc_stats)]),
    "pmc_darcy_solve_gradient": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _DP, C.c_int, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), _DP, _DP, _DP, C.c_int, C.POINTER(pmc_stats),
                                           C.POINTER(pmc_stats)]),
    "pmc_darcy_loglik_gradient": (C.c_int, [_VP, C.c_int, C.c_int, _DP, C.POINTER(C.c_double), C.c_double, C.c_int,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), _DP, C.c_int,
                                            C.POINTER(pmc_stats)]),
    "pmc_ncg_create": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "pmc_ncg_destroy": (None, [_VP]),
    "pmc_ncg_begin": (C.c_int, [_VP, C.c_int, _DP, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]),
    "pmc_ncg_step": (C.c_int, [_VP, C.c_int, _DP, C.c_int]),
    "pmc_ncg_direction": (_VP, [_VP]),
    "pmc_ncg_search_direction": (_VP, [_VP]),
    "pmc_ncg_residual": (_VP, [_VP]),
    "pmc_ncg_status": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32)]),
    "pmc_ncg_axpy_cols": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_double), _DP, _DP, _DP, C.c_int]),
    "pmc_ncg_dot_cols": (C.c_int, [_VP, C.c_int, _DP, _DP, C.POINTER(C.c_double), C.c_int]),
    "pmc_tracer_create": (C.c_int, [_VP, C.POINTER(pmc_tracer_mesh), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                    C.c_int, C.POINTER(_VP)]),
    "pmc_tracer_destroy": (None, [_VP]),
    "pmc_tracer_num_particles": (C.c_int, [_VP]),
    "pmc_tracer_run": (C.c_int, [_VP, C.c_int, _DP, C.c_int64, _DP, _VP, _VP, _VP, _DP, C.c_int]),
    "pmc_tracer_reduce": (C.c_int, [_VP, C.c_int, _DP, _VP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]),
    "pmc_darcy_set_tracer": (C.c_int, [_VP, C.c_int, _VP, C.c_int]),
    "pmc_transport_create": (C.c_int, [_VP, C.POINTER(pmc_transport_mesh), C.POINTER(pmc_transport_params), C.POINTER(_VP)]),
    "pmc_transport_destroy": (None, [_VP]),
    "pmc_transport_size": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pmc_transport_run": (C.c_int, [_VP, C.c_int, _DP, C.c_int64, _DP, _DP, _DP, _DP, _DP, _VP, _VP, C.c_int]),
    "pmc_transport_reduce": (C.c_int, [_VP, C.c_int, _DP, _DP, C.c_int, C.POINTER(C.c_double), C.c_int]),
    "pmc_darcy_set_transport": (C.c_int, [_VP, C.c_int, _VP, C.c_int]),
    "pmc_transport_run_adjoint": (C.c_int, [_VP, C.c_int, _DP, C.c_int64, _DP, _DP, _DP, _DP, C.c_int64, _DP, _DP, _DP, _VP, _VP,
                                            C.c_int]),
    "pmc_transport_set_adjoint_segment": (C.c_int, [_VP, C.c_int]),
    "pmc_darcy_transport_gradient": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _DP, _DP, _DP, C.c_int, _DP, _DP,
                                               C.POINTER(C.c_int32), _DP, _DP, _DP, C.c_int, C.POINTER(pmc_stats),
                                               C.POINTER(pmc_stats)]),
    "pmc_darcy_transport_loglik_gradient": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _DP, C.POINTER(C.c_double), C.c_double, C.c_int,
                                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), _DP,
                                                      C.c_int, C.POINTER(pmc_stats)]),
    "pmc_tracer_run_adjoint": (C.c_int, [_VP, C.c_int, _DP, C.c_int64, _DP, _DP, _DP, C.c_int64, _DP, _DP, _VP, _VP, _VP, C.c_int]),
    "pmc_tracer_reduce_seed": (C.c_int, [_VP, C.c_int, _DP, _VP, C.c_int, _DP, C.c_int]),
    "pmc_tracer_set_adjoint_scratch": (C.c_int, [_VP, C.c_int64]),
    "pmc_tracer_adjoint_chunks": (C.c_int, [_VP]),
    "pmc_darcy_tracer_gradient": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _DP, _DP, C.c_int, _DP, _VP, _DP, _DP, _DP, C.c_int,
                                            C.POINTER(pmc_stats), C.POINTER(pmc_stats)]),
    "pmc_darcy_tracer_loglik_gradient": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _DP, C.POINTER(C.c_double), C.c_double, C.c_int,
                                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), _DP,
                                                   C.c_int, C.POINTER(pmc_stats)]),
    "pmc_comm_unique_id": (C.c_int, [_VP]),
    "pmc_comm_init": (C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    "pmc_comm_destroy": (C.c_int, [_VP]),
    "pmc_allreduce_sum_f64": (C.c_int, [_VP, C.POINTER(C.c_double), C.c_int]),
}

# path diagnostics added after the boundary settled: a library built from an older commit (the parent in a same-box A/B,
# scripts/ab_libs.sh) lacks them and still loads; calling one on such a library raises AttributeError
_LATE_DIAGNOSTICS = ("pmc_adopted_rhs_solves", "pmc_fused_field_evals", "pmc_solve_path_count")

_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libpmc.so and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # PMC_LIB (harness only - the library itself reads no PMC_* variable): another build of the library, e.g. the laboratory
    # one for a profiling pass, selected WITHOUT overwriting the product's file
    p = path or os.environ.get("PMC_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise PmcError(-2, f"{p} not found - build it with `make` / __graft_entry__.build() (no CPU fallback)")
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        if name in _LATE_DIAGNOSTICS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)     # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise PmcError(rc, load_library().pmc_last_error().decode("utf-8", "replace"))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class _Keep:
    """Holds numpy arrays alive while a C struct points into them."""

    def __init__(self):
        self.refs = []

    def csr(self, m) -> pmc_csr:
        if m is None:
            return pmc_csr(0, 0, None, None, None)
        m = m.tocsr()
        rp, ci, v = _i32(m.indptr), _i32(m.indices), _f64(m.data)
        self.refs += [rp, ci, v]
        return pmc_csr(m.shape[0], m.shape[1], _ptr(rp, C.c_int32), _ptr(ci, C.c_int32), _ptr(v, C.c_double))

    def f64(self, a):
        a = _f64(a)
        self.refs.append(a)
        return _ptr(a, C.c_double)

    def i32(self, a):
        a = _i32(a)
        self.refs.append(a)
        return _ptr(a, C.c_int32)

    def u8(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        self.refs.append(a)
        return _ptr(a, C.c_uint8)


def hybrid_build(pattern, c_ptr, c_elem, c_val, B, w_diag, alpha, P=None):
    """pmc_hybrid_build (host code of libpmc.so, no GPU needed): the element-local elimination of one sampler level from the
    element decomposition of the u-mass matrix (fe.rt0.mass_contributions), B without boundary elimination and diag(W).
    Returns (H, G, z_diag) as scipy CSR / numpy COPIES of what pmc_hybrid_system_level exposes."""
    import scipy.sparse as sp
    lib = load_library()
    keep = _Keep()
    n_s, n_u = B.shape
    lv = pmc_hybrid_elements(n_u, n_s, keep.csr(pattern), keep.i32(c_ptr), keep.i32(c_elem), keep.f64(c_val), keep.csr(B),
                             keep.f64(w_diag), keep.csr(P))
    h = _VP()
    _check(lib.pmc_hybrid_build(C.byref(lv), float(alpha), C.byref(h)))
    try:
        v = pmc_hybrid_level()
        _check(lib.pmc_hybrid_system_level(h, C.byref(v)))

        def mat(c):
            rp = np.ctypeslib.as_array(c.rowptr, (c.nrows + 1,)).copy()
            nnz = int(rp[-1])
            return sp.csr_matrix((np.ctypeslib.as_array(c.vals, (nnz,)).copy(), np.ctypeslib.as_array(c.colind, (nnz,)).copy(), rp),
                                 shape=(c.nrows, c.ncols))
        return mat(v.H), mat(v.G), np.ctypeslib.as_array(v.z_diag, (n_s,)).copy()
    finally:
        lib.pmc_hybrid_system_destroy(h)


def library_hybrid_builder(space, alpha):
    """fe.hybrid's `builder` hook: the library's own elimination (pmc_hybrid_build) instead of the numpy stand-in"""
    from .fe.rt0 import mass_contributions
    pat, c_ptr, c_elem, c_val = mass_contributions(space.emass)
    return hybrid_build(pat, c_ptr, c_elem, c_val, space.B, space.vol, alpha)


def solver_opts(**kw) -> pmc_solver_opts:
    o = pmc_solver_opts()
    load_library().pmc_solver_opts_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k!r}")
        setattr(o, k, v)
    return o


class DeviceArray:
    """fp64 array in HBM owned by a Context (pmc_malloc / pmc_free)."""

    def __init__(self, ctx: "Context", n: int):
        self.ctx, self.n = ctx, int(n)
        p = _VP()
        _check(ctx.lib.pmc_malloc(ctx.h, self.n * 8, C.byref(p)))
        self.ptr = p.value or 0
        ctx._adopt(self)

    def upload(self, a):
        a = _f64(a).ravel()
        assert a.size == self.n
        _check(self.ctx.lib.pmc_memcpy_h2d(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.n, np.float64)
        _check(self.ctx.lib.pmc_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx.lib.pmc_free(self.ctx.h, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceInt32Array(DeviceArray):
    """int32 array in HBM (the integer outputs of Tracer.Run on device memory): n entries in a DeviceArray of (n + 1) // 2"""

    def __init__(self, ctx: "Context", n: int):
        super().__init__(ctx, (int(n) + 1) // 2)
        self.n_int = int(n)

    def upload(self, a):
        raise TypeError("DeviceInt32Array is an output buffer")

    def download(self) -> np.ndarray:
        out = np.empty(self.n_int, np.int32)
        _check(self.ctx.lib.pmc_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out


def _batch_of(x, n):
    """realizations of n entries a DeviceArray / torch tensor holds (its length must be a multiple of n)"""
    total = x.n if isinstance(x, DeviceArray) else int(x.numel())
    if n <= 0 or total == 0 or total % n:
        raise PmcError(-1, f"a buffer of {total} entries does not hold whole fields of {n}")
    return total // n


def _addr(x):
    """(address, memspace) of a numpy array, a DeviceArray or a torch tensor."""
    if x is None:
        return None, None
    if isinstance(x, DeviceArray):
        return x.ptr, PMC_MEM_DEVICE
    if isinstance(x, np.ndarray):
        assert x.dtype == np.float64 and x.flags["C_CONTIGUOUS"]
        return x.ctypes.data, PMC_MEM_HOST
    if hasattr(x, "data_ptr"):   # torch tensor: plumbing only (device memory owner)
        assert str(x.dtype) == "torch.float64" and x.is_contiguous()
        return x.data_ptr(), (PMC_MEM_DEVICE if x.is_cuda else PMC_MEM_HOST)
    raise TypeError(type(x))


class Context:
    def __init__(self, device_id: int = 0, seed: int = 0):
        self.lib = load_library()
        h = _VP()
        # the versioned entry point: a library with another pmc_solver_opts / pmc_stats layout refuses this binding
        _check(self.lib.pmc_ctx_create_abi(int(device_id), PMC_ABI_VERSION, C.byref(h)))
        self.h = h
        self.device_id = device_id
        self._children = []     # weakrefs to handles that must die before the context does
        self.seed(seed)

    def _adopt(self, obj):
        import weakref
        self._children.append(weakref.ref(obj))

    def seed(self, seed: int, nparts: int = 1, mypart: int = 0):
        _check(self.lib.pmc_rng_seed(self.h, C.c_uint64(seed), nparts, mypart))

    def synchronize(self):
        _check(self.lib.pmc_ctx_synchronize(self.h))

    def stream(self) -> int:
        return self.lib.pmc_ctx_stream(self.h) or 0

    def timer_start(self):
        _check(self.lib.pmc_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_double()
        _check(self.lib.pmc_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def empty(self, n) -> DeviceArray:
        return DeviceArray(self, n)

    def array(self, a) -> DeviceArray:
        a = _f64(a)
        return DeviceArray(self, a.size).upload(a)

    def normal_fill(self, n, nbatch=1, first_id=0, stream=0, mean=0.0, sigma2=1.0, out=None):
        """NormalDistributionSampler::operator()(Vector&)."""
        if out is None:
            out = np.empty((nbatch, n))
        p, ms = _addr(out)
        _check(self.lib.pmc_normal_fill(self.h, mean, sigma2, C.c_uint64(first_id), stream, nbatch, n, p, ms))
        return out

    # communicator
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        _check(self.lib.pmc_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = C.create_string_buffer(uid, 128)
        _check(self.lib.pmc_comm_init(self.h, buf, nranks, rank))

    def allreduce_sum(self, a: np.ndarray) -> np.ndarray:
        a = _f64(a)
        _check(self.lib.pmc_allreduce_sum_f64(self.h, _ptr(a, C.c_double), a.size))
        return a

    def close(self):
        if getattr(self, "h", None):
            for ref in self._children:      # samplers / solvers / device arrays hold a reference to this ctx
                obj = ref()
                if obj is not None:
                    (obj.close if hasattr(obj, "close") else obj.free)()
            self._children = []
            self.lib.pmc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PDESampler:
    """Device SPDE sampler; mirrors parelagmc::PDESampler / EmbeddedPDESampler /
    L2ProjectionPDESampler (Sample, Eval, SampleSize, GetNNZ)."""

    def __init__(self, ctx: Context, problem, opts: Optional[pmc_solver_opts] = None, projection: str = "none",
                 l2_ops=None):
        self.ctx, self.problem = ctx, problem
        lib = ctx.lib
        keep = _Keep()
        nl = len(problem.levels)
        h = _VP()
        o = opts if opts is not None else solver_opts()
        self.hybrid = hasattr(problem.levels[0], "n_lambda")     # fe.HybridSamplerProblem: the hybridized solver
        if self.hybrid:
            harr = (pmc_hybrid_level * nl)()
            for i, L in enumerate(problem.levels):
                harr[i] = pmc_hybrid_level(L.n_lambda, L.n_s, keep.csr(L.H), keep.csr(L.G), keep.f64(L.z_diag),
                                           keep.f64(L.w_diag), keep.csr(L.P))
            _check(lib.pmc_sampler_create_hybrid(ctx.h, nl, harr, problem.alpha, problem.matern_g,
                                                 1 if problem.lognormal else 0, C.byref(o), C.byref(h)))
        else:
            arr = (pmc_sampler_level * nl)()
            for i, L in enumerate(problem.levels):
                arr[i] = pmc_sampler_level(L.n_u, L.n_s, keep.csr(L.M), keep.csr(L.B), keep.f64(L.w_diag), keep.csr(L.P))
            _check(lib.pmc_sampler_create(ctx.h, nl, problem.n_mc_levels, arr, problem.alpha, problem.matern_g,
                                          1 if problem.lognormal else 0, C.byref(o), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.nlevels = problem.n_mc_levels
        if projection == "gather":
            for lvl, idx in enumerate(problem.orig_index):
                k2 = _Keep()
                _check(lib.pmc_sampler_set_projection(h, lvl, PMC_PROJ_GATHER, None, k2.i32(idx), None, len(idx)))
        elif projection == "l2":
            for lvl, (Gt, inv_w) in enumerate(l2_ops):
                k2 = _Keep()
                g = k2.csr(Gt)
                _check(lib.pmc_sampler_set_projection(h, lvl, PMC_PROJ_L2, C.byref(g), None, k2.f64(inv_w), Gt.shape[0]))
        elif projection != "none":
            raise ValueError(projection)

    def xi_size(self, level):
        return self.ctx.lib.pmc_sampler_xi_size(self.h, level)

    def SampleSize(self, level):
        return self.ctx.lib.pmc_sampler_sample_size(self.h, level)

    def BatchWidth(self, level):
        """realizations of `level` one launch of the solver kernels carries (pmc_sampler_batch_width)"""
        return self.ctx.lib.pmc_sampler_batch_width(self.h, level)

    def vcycle_levels(self, level):
        """[{rows, nnz, slots, sp_nnz, sp_slots, in_tail, fused_restriction, narrow_dense, narrow_pieces}] of the V-cycle
        hierarchy of `level` (narrow_*: what launches of at most 8 realizations do on the level, see include/pmc.h)"""
        out, nv, info = [], C.c_int(0), (C.c_int64 * 7)()
        v = 0
        while True:
            _check(self.ctx.lib.pmc_sampler_vcycle_info(self.h, level, v, C.byref(nv), info))
            d = dict(zip(("rows", "nnz", "slots", "sp_nnz", "sp_slots", "in_tail", "fused_restriction"), [int(x) for x in info]))
            flags = d["in_tail"]
            d.update(in_tail=flags & 1, narrow_dense=(flags >> 1) & 1, narrow_pieces=1 << (flags >> 4))
            out.append(d)
            v += 1
            if v >= nv.value:
                return out

    def vcycle_setup(self, level):
        """setup values of every level of the V-cycle of `level` (pmc_sampler_vcycle_level): a list of dicts.  role_wide /
        role_narrow: what launches of more than / at most dense_nb realizations do on the level (0 smooth and descend,
        1 end with a polynomial, 2 end with an exact solve, 3 not reached); tail_wide / tail_narrow: inside the LDS tail"""
        keys = ("rows", "lmax", "role_wide", "smooth_degree", "smooth_ratio", "last_degree", "last_ratio", "galerkin_scale",
                "ratio_M", "degree_M", "hierarchy", "dense_nb", "role_narrow", "tail_wide", "tail_narrow")
        out, nv, v = [], C.c_int(0), 0
        while True:
            info = (C.c_double * 15)()
            _check(self.ctx.lib.pmc_sampler_vcycle_level(self.h, level, v, C.byref(nv), info))
            out.append(dict(zip(keys, list(info))))
            v += 1
            if v >= nv.value:
                return out

    def vcycle_prolongator(self, level, vlevel):
        """P from V-cycle level vlevel + 1 to vlevel of `level` (pmc_sampler_vcycle_prolongator) as a scipy CSR matrix; the
        rows of vlevel 0 in the caller's numbering"""
        import scipy.sparse as sp
        nr, nc, nnz = C.c_int(0), C.c_int(0), C.c_int64(0)
        _check(self.ctx.lib.pmc_sampler_vcycle_prolongator(self.h, level, vlevel, C.byref(nr), C.byref(nc), C.byref(nnz),
                                                           None, None, None))
        rp = np.empty(nr.value + 1, dtype=np.int32)
        ci = np.empty(nnz.value, dtype=np.int32)
        va = np.empty(nnz.value, dtype=np.float64)
        _check(self.ctx.lib.pmc_sampler_vcycle_prolongator(self.h, level, vlevel, C.byref(nr), C.byref(nc), C.byref(nnz),
                                                           rp.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           va.ctypes.data_as(C.POINTER(C.c_double))))
        return sp.csr_matrix((va, ci, rp), shape=(nr.value, nc.value))

    def z_bytes(self):
        """bytes per entry of the preconditioned Krylov vectors of this handle (4: PMC_STORAGE_FP32, 8: PMC_STORAGE_FP64)"""
        return self.ctx.lib.pmc_sampler_krylov_z_bytes(self.h)

    def GetNNZ(self, level):
        return self.ctx.lib.pmc_sampler_nnz(self.h, level)

    def GetTrueP(self, level):
        """MLSampler::GetTrueP: the s-space prolongator from level+1 to level as a scipy CSR matrix (a copy)."""
        import scipy.sparse as sp
        c = pmc_csr()
        _check(self.ctx.lib.pmc_sampler_true_p(self.h, level, C.byref(c)))
        nnz = c.rowptr[c.nrows]
        rp = np.ctypeslib.as_array(c.rowptr, shape=(c.nrows + 1,)).copy()
        ci = np.ctypeslib.as_array(c.colind, shape=(nnz,)).copy()
        v = np.ctypeslib.as_array(c.vals, shape=(nnz,)).copy()
        return sp.csr_matrix((v, ci, rp), shape=(c.nrows, c.ncols))

    def Sample(self, level, first_id=0, nbatch=1, out=None):
        n = self.xi_size(level)
        if out is None:
            out = np.empty((nbatch, n))
        p, ms = _addr(out)
        _check(self.ctx.lib.pmc_sampler_sample(self.h, level, C.c_uint64(first_id), nbatch, p, ms))
        return out

    def Eval(self, level, xi, xi_level=None, init_s=None, init_level=None, use_init=False, s_out=None,
             embed_out=None, want_embed=False, return_stats=False):
        """xi: (nbatch, n_xi) numpy (host) or DeviceArray/torch tensor (device, with nbatch=...).
        Returns s (and embed_s, stats) as numpy arrays for host inputs."""
        lib = self.ctx.lib
        if not (0 <= level < self.nlevels):
            raise PmcError(-1, f"Eval: level {level} out of range")
        if isinstance(xi, np.ndarray):
            xi = _f64(np.atleast_2d(xi))
            nbatch = xi.shape[0]
            if xi_level is None:     # reference behaviour: infer from the length (PDESampler.cpp:419)
                sizes = [self.xi_size(l) for l in range(self.nlevels)]
                xi_level = sizes.index(xi.shape[1])
            if s_out is None:
                s_out = np.empty((nbatch, self.SampleSize(level)))
            if want_embed and embed_out is None:
                embed_out = np.empty((nbatch, self.xi_size(level)))
            if init_s is not None:
                init_s = _f64(np.atleast_2d(init_s))
        else:
            nbatch = xi.n // self.xi_size(xi_level)
        stats = (pmc_stats * nbatch)()
        pxi, ms = _addr(xi)
        ps, _ = _addr(s_out)
        pinit, _ = _addr(init_s)
        pemb, _ = _addr(embed_out)
        _check(lib.pmc_sampler_eval(self.h, level, xi_level, nbatch, pxi, ps, pinit,
                                    -1 if init_level is None else init_level, 1 if use_init else 0, pemb, ms, stats))
        # device milliseconds of this call (HIP events on the handle's stream): (right-hand sides / initial guesses, solves)
        self.last_phase_ms = (sum(s.setup_ms for s in stats), sum(s.solve_ms for s in stats))
        out = [s_out]
        if want_embed or embed_out is not None:
            out.append(embed_out)
        if return_stats:
            out.append([(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in stats])
        return out[0] if len(out) == 1 else tuple(out)

    def EvalAdjoint(self, level, v, s_out=None, xi_level=None, grad_out=None, nbatch=None, return_stats=False):
        """dJ/dxi = (d Eval / d xi)^T v (pmc_sampler_eval_adjoint).  v: (nbatch, SampleSize(level)) numpy (host) or a device
        array (then with nbatch=... and grad_out=...); s_out: None, or Eval's output on a lognormal handle (v is multiplied
        by it).  Returns grad_xi (nbatch, xi_size(xi_level)); xi_level defaults to level."""
        if not (0 <= level < self.nlevels):
            raise PmcError(-1, f"EvalAdjoint: level {level} out of range")
        if xi_level is None:
            xi_level = level
        single = False
        if isinstance(v, np.ndarray):
            single = v.ndim == 1
            v = _f64(np.atleast_2d(v))
            nbatch = v.shape[0]
            if v.shape[1] != self.SampleSize(level):
                raise PmcError(-1, "EvalAdjoint: v does not match SampleSize(level)")
            if s_out is not None:
                s_out = _f64(np.atleast_2d(s_out))
                if s_out.shape != v.shape:
                    raise PmcError(-1, "EvalAdjoint: s_out does not match v")
            if grad_out is None and 0 <= xi_level < self.nlevels:
                grad_out = np.empty((nbatch, self.xi_size(xi_level)))
        elif nbatch is None:
            nbatch = v.n // self.SampleSize(level)
        stats = (pmc_stats * max(1, nbatch))()
        pv, ms = _addr(v)
        ps, _ = _addr(s_out)
        pg, _ = _addr(grad_out)
        _check(self.ctx.lib.pmc_sampler_eval_adjoint(self.h, level, xi_level, nbatch, pv, ps, pg, ms, stats))
        self.last_phase_ms = (sum(s.setup_ms for s in stats), sum(s.solve_ms for s in stats))
        g = grad_out[0] if single else grad_out
        if return_stats:
            return g, [(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in stats]
        return g

    def EvalTangent(self, level, v, s_out=None, xi_level=None, ds_out=None, nbatch=None, return_stats=False):
        """ds_out = (d Eval / d xi) v (pmc_sampler_eval_tangent): Eval of v without exp(), times s_out when given.  v: (nbatch,
        xi_size(xi_level)) numpy (host) or a device array (then with nbatch=... and ds_out=...); s_out: None, or Eval's
        output on a lognormal handle.  Returns ds_out (nbatch, SampleSize(level)); xi_level defaults to level."""
        if not (0 <= level < self.nlevels):
            raise PmcError(-1, f"EvalTangent: level {level} out of range")
        if xi_level is None:
            xi_level = level
        single = False
        if isinstance(v, np.ndarray):
            single = v.ndim == 1
            v = _f64(np.atleast_2d(v))
            nbatch = v.shape[0]
            if 0 <= xi_level < self.nlevels and v.shape[1] != self.xi_size(xi_level):
                raise PmcError(-1, "EvalTangent: v does not match xi_size(xi_level)")
            if s_out is not None:
                s_out = _f64(np.atleast_2d(s_out))
                if s_out.shape != (nbatch, self.SampleSize(level)):
                    raise PmcError(-1, "EvalTangent: s_out does not match SampleSize(level)")
            if ds_out is None:
                ds_out = np.empty((nbatch, self.SampleSize(level)))
        assert nbatch is not None
        stats = (pmc_stats * max(1, nbatch))()
        pv, ms = _addr(v)
        ps, _ = _addr(s_out)
        pd, _ = _addr(ds_out)
        _check(self.ctx.lib.pmc_sampler_eval_tangent(self.h, level, xi_level, nbatch, pv, ps, pd, ms, stats))
        self.last_phase_ms = (sum(s.setup_ms for s in stats), sum(s.solve_ms for s in stats))
        d = ds_out[0] if single else ds_out
        if return_stats:
            return d, [(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in stats]
        return d

    def set_operator_timing(self, on: bool):
        """Bracket every K5 launch of the MINRES loop with HIP events (in-situ kernel time for the roofline)."""
        _check(self.ctx.lib.pmc_sampler_set_operator_timing(self.h, 1 if on else 0))

    def _error(self, fn, level, coeff, exact):
        n = self.SampleSize(level)
        if n < 0:
            raise PmcError(-1, f"level {level} out of range")
        if isinstance(coeff, np.ndarray):
            single = coeff.ndim == 1
            coeff = _f64(np.atleast_2d(coeff))
            nbatch = coeff.shape[0]
            if coeff.shape[1] != n:
                raise PmcError(-1, "coefficient vectors do not match SampleSize(level)")
        else:
            single, nbatch = False, _batch_of(coeff, n)
        err = np.empty(nbatch)
        p, ms = _addr(coeff)
        _check(fn(self.h, level, nbatch, p, float(exact), err.ctypes.data, PMC_MEM_HOST) if ms == PMC_MEM_HOST else
               self._error_dev(fn, level, nbatch, p, exact, err))
        return float(err[0]) if single else err

    def _error_dev(self, fn, level, nbatch, p, exact, err):
        out = self.ctx.empty(nbatch)
        rc = fn(self.h, level, nbatch, p, float(exact), out.ptr, PMC_MEM_DEVICE)
        if rc == 0:
            err[:] = out.download()
        out.free()
        return rc

    def ComputeL2Error(self, level, coeff, exact):
        """MLSampler::ComputeL2Error: || P_0 .. P_{level-1} coeff - exact ||^2_L2 (squared, as the reference returns) of one
        field (a float) or of each row of a (nbatch, SampleSize(level)) array / device array (an array)."""
        return self._error(self.ctx.lib.pmc_sampler_l2_error, level, coeff, exact)

    def ComputeMaxError(self, level, coeff, exact):
        """MLSampler::ComputeMaxError: max(max coeff - exact, exact - min coeff), per field."""
        return self._error(self.ctx.lib.pmc_sampler_max_error, level, coeff, exact)

    def SetOutputHierarchy(self, P_orig, w0_orig):
        """the original mesh's prolongators (P_orig[l]: SampleSize(l) x SampleSize(l + 1)) and level-0 P0 mass behind the
        output of an embedded / L2-projected handle (pmc_sampler_set_output_hierarchy)"""
        keep = _Keep()
        arr = (pmc_csr * max(1, len(P_orig)))()
        for i, P in enumerate(P_orig):
            arr[i] = keep.csr(P)
        _check(self.ctx.lib.pmc_sampler_set_output_hierarchy(self.h, len(P_orig) + 1, arr, keep.f64(w0_orig)))

    def operator_time(self):
        """(total ms, launches) of the timed K5 launches since the last call."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        _check(self.ctx.lib.pmc_sampler_operator_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def operator_event_overhead(self):
        """total ms of the empty event brackets recorded behind the timed launches since the last call."""
        ms = C.c_double(0.0)
        _check(self.ctx.lib.pmc_sampler_operator_event_overhead(self.h, C.byref(ms)))
        return ms.value

    def smoother_time(self):
        """(total ms, launches, event overhead ms) of the bracketed post-smoothing launches (hybridized samplers) since the
        last call"""
        ms, n, g = C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx.lib.pmc_sampler_smoother_time(self.h, C.byref(ms), C.byref(n), C.byref(g)))
        return ms.value, n.value, g.value

    def smoother_bytes(self, level, nbatch):
        b = C.c_double(0.0)
        _check(self.ctx.lib.pmc_sampler_smoother_bytes(self.h, level, nbatch, C.byref(b)))
        return b.value

    def Mult(self, level, x, repeat=1):
        """y = [M Bt; B -aW] x (the block operator's Mult).  x: (nbatch, n_u+n_s) numpy or a
        DeviceArray (then pass nbatch via x.n).  Returns (y, avg_kernel_ms, algorithmic_bytes)."""
        L = self.problem.levels[level]
        n = L.n_lambda if self.hybrid else L.n_u + L.n_s     # hybrid: y = H x
        if isinstance(x, np.ndarray):
            x = _f64(np.atleast_2d(x))
            nb = x.shape[0]
            y = np.empty_like(x)
        else:
            nb = x.n // n
            y = self.ctx.empty(x.n)
        px, ms = _addr(x)
        py, _ = _addr(y)
        t, b = C.c_double(), C.c_double()
        _check(self.ctx.lib.pmc_sampler_apply_operator(self.h, level, nb, px, py, ms, repeat, C.byref(t), C.byref(b)))
        return y, t.value, b.value

    def ApplyPreconditioner(self, level, r):
        """z = B^-1 r, one application of the MINRES preconditioner of `level` (pmc_sampler_apply_preconditioner); r: (nbatch,
        n_u+n_s) numpy, nbatch one of 1, 2, 4, ... up to the level's launch width"""
        r = _f64(np.atleast_2d(r))
        z = np.empty_like(r)
        pr, ms = _addr(r)
        pz, _ = _addr(z)
        _check(self.ctx.lib.pmc_sampler_apply_preconditioner(self.h, level, r.shape[0], pr, pz, ms))
        return z

    def Solve(self, level, rhs, guess=None, return_stats=False):
        """invA[level]->Mult(rhs, sol) (pmc_sampler_mult): the full solution [u; s] of A x = rhs.  rhs: (nbatch, n_u+n_s)
        numpy or a DeviceArray; guess (same kind): initial guess (iterative_mode)."""
        L = self.problem.levels[level]
        n = L.n_lambda if self.hybrid else L.n_u + L.n_s     # hybrid: H lambda = rhs on the multipliers
        if isinstance(rhs, np.ndarray):
            rhs = _f64(np.atleast_2d(rhs))
            nb = rhs.shape[0]
            sol = np.empty_like(rhs) if guess is None else _f64(np.atleast_2d(guess)).copy()
        else:
            nb = rhs.n // n
            sol = self.ctx.empty(rhs.n) if guess is None else guess
        pr, ms = _addr(rhs)
        px, _ = _addr(sol)
        st = (pmc_stats * nb)()
        _check(self.ctx.lib.pmc_sampler_mult(self.h, level, nb, pr, px, 0 if guess is None else 1, ms, st))
        if return_stats:
            return sol, [(t.iterations, t.converged, t.initial_norm, t.final_norm) for t in st]
        return sol

    def SetConditioner(self, conditioner):
        """Eval returns fields conditioned on the data of `conditioner` (a Conditioner created on this handle with exact
        data); None detaches (pmc_sampler_set_conditioner)"""
        _check(self.ctx.lib.pmc_sampler_set_conditioner(self.h, None if conditioner is None else conditioner.h))
        self._conditioner = conditioner

    def close(self):
        if getattr(self, "h", None):
            for ref in getattr(self, "_stats", []):     # FieldStatistics and Conditioners of this handle die first
                obj = ref()
                if obj is not None:
                    obj.close()
            self.ctx.lib.pmc_sampler_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sampler_alive(sampler) -> bool:
    """False once the sampler's handle is destroyed.  FieldStatistics and Conditioners hold a reference into it on the C side
    and their destroy calls touch it: PDESampler.close() closes them first, but when the garbage collector finalizes a
    sampler and its dependants together (a test that failed before its close() calls) the weak references are already cleared
    and the sampler may go first - destroying the dependant afterwards would read freed memory, so it is abandoned instead."""
    return getattr(sampler, "h", None) is not None


class FieldStatistics:
    """Accumulators of one sampler level's output on the device (pmc_field_stats_*): the expectation, the second moment
    about zero (the drivers' "marginal variance") and the covariance with an indicator chi of PDESamplerTest's loop."""

    def __init__(self, sampler: PDESampler, level: int, chi=None):
        self.sampler, self.level, self.ctx = sampler, level, sampler.ctx
        self.n = sampler.SampleSize(level)
        self.has_chi = chi is not None
        h = _VP()
        if chi is None:
            p, ms = None, PMC_MEM_HOST
        else:
            if isinstance(chi, np.ndarray):
                chi = _f64(chi).ravel()
                if chi.size != self.n:
                    raise PmcError(-1, "chi does not match SampleSize(level)")
            p, ms = _addr(chi)
        _check(self.ctx.lib.pmc_field_stats_create(sampler.h, level, p, ms, C.byref(h)))
        self.h = h
        if not hasattr(sampler, "_stats"):
            sampler._stats = []
        sampler._stats.append(weakref.ref(self))

    def run(self, first_id, nsamples):
        """Sample + Eval + accumulate the realizations first_id .. first_id + nsamples - 1 on the device"""
        _check(self.ctx.lib.pmc_field_stats_run(self.h, C.c_uint64(first_id), C.c_int64(nsamples)))
        return self

    def accumulate(self, s, nbatch=None):
        """add realizations the caller holds: (nbatch, n) numpy, or a DeviceArray / torch tensor (nbatch=...)"""
        if isinstance(s, np.ndarray):
            s = _f64(np.atleast_2d(s))
            nbatch = s.shape[0]
        else:
            nb = _batch_of(s, self.n)
            if nbatch is None:
                nbatch = nb
            elif not 1 <= nbatch <= nb:
                raise PmcError(-1, f"nbatch {nbatch} exceeds the {nb} realizations the buffer holds")
        p, ms = _addr(s)
        _check(self.ctx.lib.pmc_field_stats_accumulate(self.h, int(nbatch), p, ms))
        return self

    def reset(self):
        _check(self.ctx.lib.pmc_field_stats_reset(self.h))
        return self

    def read(self, chi_cov=None):
        """(expectation, second_moment, chi_cov or None, N); chi_cov defaults to whether chi was given"""
        want = self.has_chi if chi_cov is None else chi_cov
        e, m2 = np.empty(self.n), np.empty(self.n)
        cc = np.empty(self.n) if want else None
        cnt = C.c_int64(0)
        _check(self.ctx.lib.pmc_field_stats_read(self.h, e.ctypes.data, m2.ctypes.data, None if cc is None else cc.ctypes.data,
                                                 C.byref(cnt), PMC_MEM_HOST))
        return e, m2, cc, cnt.value

    def read_sums(self):
        """((4 or 6), n) raw accumulators [sum s, comp, sum s^2, comp, sum <chi,s> s, comp] and N"""
        out = np.empty(((6 if self.has_chi else 4), self.n))
        cnt = C.c_int64(0)
        _check(self.ctx.lib.pmc_field_stats_read_sums(self.h, out.ctypes.data, C.byref(cnt), PMC_MEM_HOST))
        return out, cnt.value

    def chi_dot(self, s):
        """<chi, s_c> of each row of s exactly as the accumulation forms them"""
        s = _f64(np.atleast_2d(s))
        out = np.empty(s.shape[0])
        _check(self.ctx.lib.pmc_field_stats_chi_dot(self.h, s.shape[0], s.ctypes.data, out.ctypes.data, PMC_MEM_HOST))
        return out

    def close(self):
        if getattr(self, "h", None):
            if _sampler_alive(self.sampler):
                self.ctx.lib.pmc_field_stats_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Conditioner:
    """Conditioning of a sampler's Gaussian fields on linear observations H0 g (+ noise of variance sigma2) = y
    (pmc_conditioner_*; fe.condition is its numpy twin).  H0: scipy sparse nobs x n_s(0); sigma2 None = exact data."""

    def __init__(self, sampler: PDESampler, H0, y, sigma2=None):
        self.sampler, self.ctx = sampler, sampler.ctx
        keep = _Keep()
        H = keep.csr(H0)
        y = _f64(y).ravel()
        self.nobs = int(H.nrows)
        if y.size != self.nobs or (sigma2 is not None and np.size(sigma2) != self.nobs):
            raise PmcError(-1, "Conditioner: y / sigma2 must hold one value per row of H0")
        self.noisy = sigma2 is not None and bool(np.any(np.asarray(sigma2) > 0.0))
        h = _VP()
        _check(self.ctx.lib.pmc_conditioner_create(sampler.h, self.nobs, C.byref(H), keep.f64(y),
                                                   None if sigma2 is None else keep.f64(np.ravel(sigma2)), C.byref(h)))
        self.h = h
        if not hasattr(sampler, "_stats"):
            sampler._stats = []
        sampler._stats.append(weakref.ref(self))

    def level(self, level):
        """(K (n_s(level), nobs), A (nobs, nobs), H_level scipy CSR) of the device setup"""
        import scipy.sparse as sp
        lib = self.ctx.lib
        n, nnz = C.c_int(0), C.c_int64(0)
        _check(lib.pmc_conditioner_level(self.h, level, C.byref(n), C.byref(nnz), None, None, None, None, None))
        K = np.empty((self.nobs, n.value))      # column-major n x nobs
        A = np.empty((self.nobs, self.nobs))
        rp, ci, va = np.empty(self.nobs + 1, np.int32), np.empty(nnz.value, np.int32), np.empty(nnz.value)
        _check(lib.pmc_conditioner_level(self.h, level, None, None, _ptr(K, C.c_double), _ptr(A, C.c_double),
                                         _ptr(rp, C.c_int32), _ptr(ci, C.c_int32), _ptr(va, C.c_double)))
        return np.ascontiguousarray(K.T), A, sp.csr_matrix((va, ci, rp), shape=(self.nobs, n.value))

    def apply(self, level, g, zeta=None, exp=False, out=None):
        """g + K A^-1 (y + sqrt(sigma2) zeta - H g) (exp() of it with exp=True) for (nbatch, n_s(level)) numpy fields, or for
        a DeviceArray / torch tensor g (zeta and out of the same kind; out defaults to g itself: in place)"""
        if isinstance(g, np.ndarray):
            g = _f64(np.atleast_2d(g))
            nbatch = g.shape[0]
            if zeta is not None:
                zeta = _f64(np.atleast_2d(zeta))
                if zeta.shape != (nbatch, self.nobs):
                    raise PmcError(-1, "Conditioner.apply: zeta must be (nbatch, nobs)")
            if out is None:
                out = np.empty_like(g)
        else:
            nbatch = _batch_of(g, self.sampler.xi_size(level))
            if out is None:
                out = g
        pg, ms = _addr(g)
        pz, _ = _addr(zeta)
        po, _ = _addr(out)
        _check(self.ctx.lib.pmc_conditioner_apply(self.h, level, nbatch, pg, pz, po, 1 if exp else 0, ms))
        return out

    def _derivative(self, fn, level, x, s_out, out, in_place):
        if isinstance(x, np.ndarray):
            x = _f64(np.atleast_2d(x))
            nbatch = x.shape[0]
            if s_out is not None:
                s_out = _f64(np.atleast_2d(s_out))
                if s_out.shape != x.shape:
                    raise PmcError(-1, "Conditioner: s_out must have the shape of the input")
            if out is None:
                out = np.empty_like(x)
        else:
            nbatch = _batch_of(x, self.sampler.xi_size(level))
            if out is None:
                if not in_place:
                    raise PmcError(-1, "Conditioner.apply_adjoint: device arrays need out (it must not alias v)")
                out = x
        px, ms = _addr(x)
        ps, _ = _addr(s_out)
        po, _ = _addr(out)
        _check(fn(self.h, level, nbatch, px, ps, po, ms))
        return out

    def apply_tangent(self, level, dg, s_out=None, out=None):
        """f' o (dg - K A^-1 H dg), f' = s_out or 1: the derivative of apply in g (pmc_conditioner_apply_tangent).  Arrays as
        for apply; out defaults to a new array (numpy) or to dg itself (device arrays)"""
        return self._derivative(self.ctx.lib.pmc_conditioner_apply_tangent, level, dg, s_out, out, True)

    def apply_adjoint(self, level, v, s_out=None, out=None):
        """u - H^T A^-1 K^T u, u = v o s_out: the transpose of apply_tangent (pmc_conditioner_apply_adjoint).  out must not
        alias v or s_out; device arrays must pass it"""
        return self._derivative(self.ctx.lib.pmc_conditioner_apply_adjoint, level, v, s_out, out, False)

    def enable_derivatives(self, on=True):
        """while attached, EvalTangent / EvalAdjoint and what is built on them differentiate the conditional field"""
        _check(self.ctx.lib.pmc_conditioner_enable_derivatives(self.h, 1 if on else 0))
        return self

    @property
    def derivatives_enabled(self):
        return bool(self.ctx.lib.pmc_conditioner_derivatives_enabled(self.h))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.sampler, "_conditioner", None) is self:
                self.sampler._conditioner = None
            if _sampler_alive(self.sampler):
                self.ctx.lib.pmc_conditioner_destroy(self.h)      # detaches itself from the sampler
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LevelFields:
    """Pressure accumulators of one Darcy level for the multilevel field estimates (pmc_level_fields_*): the compensated
    sums of d = p - p_c[parent], d^2 and p^2 - p_c[parent]^2 per fine element.  coupled: the level has a coarse partner
    level + 1 (p_c = 0 otherwise).  Work runs on ctx's stream."""

    def __init__(self, ctx: Context, solver, level: int, coupled: bool):
        self.ctx, self.solver, self.level, self.coupled = ctx, solver, level, bool(coupled)
        h = _VP()
        _check(ctx.lib.pmc_level_fields_create(ctx.h, solver.h, level, 1 if coupled else 0, C.byref(h)))
        self.h = h
        ctx._adopt(self)
        nf, nc = C.c_int(0), C.c_int(0)
        _check(ctx.lib.pmc_level_fields_size(self.h, C.byref(nf), C.byref(nc)))
        self.n, self.nc = nf.value, nc.value

    def accumulate(self, p_fine, p_coarse=None):
        """add (nbatch, n_p(level)) pressure blocks, with (nbatch, n_p(level + 1)) coarse blocks on a coupled level"""
        pf = _f64(np.atleast_2d(p_fine))
        pc = None if p_coarse is None else _f64(np.atleast_2d(p_coarse))
        if pf.shape[1] != self.n or (pc is not None and (pc.shape[1] != self.nc or pc.shape[0] != pf.shape[0])):
            raise PmcError(-1, "pressure blocks do not match the level sizes")
        _check(self.ctx.lib.pmc_level_fields_accumulate(self.h, pf.shape[0], pf.ctypes.data,
                                                        None if pc is None else pc.ctypes.data, PMC_MEM_HOST))
        return self

    def accumulate_weighted(self, x_fine, w_fine, x_coarse=None, w_coarse=None):
        """add (nbatch, n) fields weighted per realization: d = w_fine[b] x_fine - w_coarse[b] x_coarse[parent], d^2 and
        w_fine[b] x_fine^2 - w_coarse[b] x_coarse[parent]^2 (pmc_level_fields_accumulate_weighted)"""
        xf = _f64(np.atleast_2d(x_fine))
        xc = None if x_coarse is None else _f64(np.atleast_2d(x_coarse))
        wf = _f64(np.atleast_1d(w_fine))
        wc = None if w_coarse is None else _f64(np.atleast_1d(w_coarse))
        nb = xf.shape[0]
        if xf.shape[1] != self.n or wf.shape != (nb,) or (xc is not None and (xc.shape != (nb, self.nc))) or \
                (wc is not None and wc.shape != (nb,)):
            raise PmcError(-1, "fields / weights do not match the level sizes")
        addr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        _check(self.ctx.lib.pmc_level_fields_accumulate_weighted(self.h, nb, addr(xf), addr(wf), addr(xc), addr(wc),
                                                                 PMC_MEM_HOST))
        return self

    def reset(self):
        _check(self.ctx.lib.pmc_level_fields_reset(self.h))
        return self

    def read_sums(self):
        """(6, n) raw accumulators [sum d, comp, sum d^2, comp, sum p^2 - p_c^2, comp] and N"""
        out = np.empty((6, self.n))
        cnt = C.c_int64(0)
        _check(self.ctx.lib.pmc_level_fields_read_sums(self.h, out.ctypes.data, C.byref(cnt), PMC_MEM_HOST))
        return out, cnt.value

    def parents(self):
        out = np.empty(self.n, np.int32)
        _check(self.ctx.lib.pmc_level_fields_parents(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pmc_level_fields_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kl_matern_apply(ctx, centroids, w_diag, corlen, X) -> np.ndarray:
    """Y = K X on the device (pmc_kl_matern_apply): K = W^1/2 C W^1/2 of the 3D Matern kernel exp(-r / corlen), never stored.
    centroids (n, dim), X (n,) or (n, ncols); returns Y of X's shape."""
    x = _f64(centroids)
    w = _f64(w_diag)
    n, dim = x.shape
    X = np.asarray(X, dtype=np.float64)
    Xc = np.asfortranarray(X.reshape(n, -1))
    Y = np.empty_like(Xc, order="F")
    _check(ctx.lib.pmc_kl_matern_apply(ctx.h, dim, n, _ptr(x, C.c_double), _ptr(w, C.c_double), float(corlen), Xc.shape[1],
                                       Xc.ctypes.data_as(C.POINTER(C.c_double)), Y.ctypes.data_as(C.POINTER(C.c_double))))
    return np.ascontiguousarray(Y).reshape(X.shape)


def kl_matern_eigs(ctx, centroids, w_diag, corlen, nmodes, tol=None, max_iter=None, guard=None, degree=None, seed=None):
    """The top min(nmodes, n) eigenpairs of the Matern covariance on the device (pmc_kl_matern_eigs).  Returns
    (evals ascending (m,), evect0 (n, m) with V^T W V = I, info dict of pmc_kl_eigs_info).  info["converged"] == 0 is not an
    error: the pairs are the best reached after max_iter."""
    x = _f64(centroids)
    w = _f64(w_diag)
    n, dim = x.shape
    o = pmc_kl_eigs_opts()
    ctx.lib.pmc_kl_eigs_opts_default(C.byref(o))
    for name, val in (("tol", tol), ("max_iter", max_iter), ("guard", guard), ("degree", degree), ("seed", seed)):
        if val is not None:
            setattr(o, name, val)
    m = max(1, min(int(nmodes), n))
    evals = np.empty(m)
    V = np.empty((n, m), order="F")
    info = pmc_kl_eigs_info()
    _check(ctx.lib.pmc_kl_matern_eigs(ctx.h, dim, n, _ptr(x, C.c_double), _ptr(w, C.c_double), float(corlen), int(nmodes),
                                      C.byref(o), _ptr(evals, C.c_double), V.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(info)))
    return evals, np.ascontiguousarray(V), {f: getattr(info, f) for f, _ in pmc_kl_eigs_info._fields_}


class KLSampler(PDESampler):
    """Device truncated Karhunen-Loeve sampler (pmc_sampler_create_kl); mirrors parelagmc::KLSampler (Sample, Eval,
    SampleSize, GetNNZ, GetTrueP).  problem: fe.KLProblem - the eigenpairs of the covariance on the finest level and the
    level hierarchy; the handle projects the modes to the coarser levels itself."""

    def __init__(self, ctx: Context, problem):
        self.ctx, self.problem = ctx, problem
        self.hybrid = False
        keep = _Keep()
        nl = len(problem.levels)
        arr = (pmc_kl_level * nl)()
        for i, L in enumerate(problem.levels):
            arr[i] = pmc_kl_level(L.n_s, keep.f64(L.w_diag), keep.csr(L.P))
        evect0 = np.asfortranarray(problem.evect0, dtype=np.float64)     # column-major n_s(0) x m (DenseMatrix::Data())
        h = _VP()
        _check(ctx.lib.pmc_sampler_create_kl(ctx.h, nl, arr, int(problem.evals.size), keep.f64(problem.evals),
                                             _ptr(evect0.ravel(order="K"), C.c_double), 1 if problem.lognormal else 0,
                                             C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.nlevels = nl

    def is_kl(self):
        return self.ctx.lib.pmc_sampler_is_kl(self.h) == 1


class DarcySolver:
    """Device mixed Darcy solver; mirrors parelagmc::DarcySolver (SolveFwd, GetNNZ, ...)."""

    def __init__(self, ctx: Context, problem, opts: Optional[pmc_solver_opts] = None, hybrid: bool = False):
        """hybrid: SolveFwd through the hybridized form (pmc_darcy_create_hybrid, the reference's "Hybridization" option)"""
        self.ctx, self.problem = ctx, problem
        keep = _Keep()
        nl = len(problem.levels)
        arr = (pmc_darcy_level * nl)()
        for i, L in enumerate(problem.levels):
            arr[i] = pmc_darcy_level(L.n_u, L.n_p, keep.csr(L.M_pattern), keep.i32(L.c_ptr), keep.i32(L.c_elem),
                                     keep.f64(L.c_val), keep.csr(L.B), keep.f64(L.rhs), keep.u8(L.ess_mask),
                                     keep.f64(L.ess_data), keep.f64(L.obs), keep.csr(L.P))
        h = _VP()
        o = opts if opts is not None else solver_opts()
        create = ctx.lib.pmc_darcy_create_hybrid if hybrid else ctx.lib.pmc_darcy_create
        _check(create(ctx.h, nl, problem.n_mc_levels, arr, 1 if problem.k_divides else 0, C.byref(o), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.nlevels = problem.n_mc_levels

    def GetGlobalNumberOfDofs(self, level):
        return self.ctx.lib.pmc_darcy_num_dofs(self.h, level)

    GetNumberOfDofs = GetGlobalNumberOfDofs

    def GetNNZ(self, level):
        return self.ctx.lib.pmc_darcy_nnz(self.h, level)

    def BatchWidth(self, level):
        return self.ctx.lib.pmc_darcy_batch_width(self.h, level)

    def z_bytes(self):
        return self.ctx.lib.pmc_darcy_krylov_z_bytes(self.h)

    def set_operator_timing(self, on: bool):
        """Bracket every in-loop launch of the u-rows [M(k) | B^T] x (eg_pair_spmm) with HIP events."""
        _check(self.ctx.lib.pmc_darcy_set_operator_timing(self.h, 1 if on else 0))

    def operator_time(self):
        """(total bracket ms, launches, total empty-bracket ms) since the last call."""
        ms, n, gap = C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_operator_time(self.h, C.byref(ms), C.byref(n), C.byref(gap)))
        return ms.value, n.value, gap.value

    def operator_bytes(self, level, nbatch):
        b = C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_operator_bytes(self.h, level, nbatch, C.byref(b)))
        return b.value

    def poly_time(self):
        """the same for the M-block polynomial of the preconditioner (eg_poly2): (bracket ms, launches, empty-bracket ms)"""
        ms, n, gap = C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_poly_time(self.h, C.byref(ms), C.byref(n), C.byref(gap)))
        return ms.value, n.value, gap.value

    def poly_bytes(self, level, nbatch):
        b = C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_poly_bytes(self.h, level, nbatch, C.byref(b)))
        return b.value

    def SolveFwd(self, level, k, nbatch=None, want_solution=False, sol_out=None, return_stats=False):
        """Returns (Q, C) arrays of length nbatch (plus solution / stats on request)."""
        lib = self.ctx.lib
        if isinstance(k, np.ndarray):
            k = _f64(np.atleast_2d(k))
            nbatch = k.shape[0]
            if want_solution and sol_out is None:
                sol_out = np.empty((nbatch, self.GetGlobalNumberOfDofs(level)))
        assert nbatch is not None
        Q = np.empty(nbatch)
        Cc = np.empty(nbatch)
        stats = (pmc_stats * nbatch)()
        pk, ms = _addr(k)
        psol, _ = _addr(sol_out)
        _check(lib.pmc_darcy_solve_fwd(self.h, level, nbatch, pk, _ptr(Q, C.c_double), _ptr(Cc, C.c_double), psol, ms,
                                       stats))
        # device milliseconds of this call: ("Darcy: Build Solver" = M(k), elimination, Schur hierarchy refresh; "Darcy: Mult")
        self.last_phase_ms = (sum(s.setup_ms for s in stats), sum(s.solve_ms for s in stats))
        out = [Q, Cc]
        if want_solution or sol_out is not None:
            out.append(sol_out)
        if return_stats:
            out.append([(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in stats])
        return tuple(out)

    def _apply(self, fn, level, k, v):
        k = _f64(np.atleast_2d(k))
        v = _f64(np.atleast_2d(v))
        if k.shape[0] != v.shape[0]:
            raise ValueError("k and the vectors must have the same number of columns")
        out = np.empty_like(v)
        _check(fn(self.h, level, v.shape[0], _ptr(k, C.c_double), _ptr(v, C.c_double), _ptr(out, C.c_double),
                  PMC_MEM_HOST))
        return out

    def ApplyPreconditioner(self, level, k, r):
        """z = B(k)^-1 r, one application of the MINRES preconditioner of `level` (pmc_darcy_apply_preconditioner): column j
        with its own permeability k[j].  k: (nbatch, n_p), r: (nbatch, n_u + n_p) - hybridized handle: (nbatch, n_lambda),
        multipliers in the numbering of parelagmc_amd.fe.darcy_hybrid - nbatch one of 1, 2, 4, ... up to BatchWidth(level)."""
        return self._apply(self.ctx.lib.pmc_darcy_apply_preconditioner, level, k, r)

    def ApplyOperator(self, level, k, x):
        """y = A(k) x, the operator of the MINRES solve of `level` (pmc_darcy_apply_operator): [M(k) B^T; B 0] after the
        elimination of the essential rows, or H(kappa) on a hybridized handle; shapes as ApplyPreconditioner."""
        return self._apply(self.ctx.lib.pmc_darcy_apply_operator, level, k, x)

    def vcycle_levels(self, level):
        """setup values of every level of the Schur-block V-cycle of `level` (pmc_darcy_vcycle_level): a list of dicts"""
        keys = ("rows", "lmax", "bottom", "smooth_degree", "smooth_ratio", "last_degree", "last_ratio", "galerkin_scale",
                "ratio_M", "degree_M", "hierarchy")
        out, nv, v = [], C.c_int(0), 0
        while True:
            info = (C.c_double * 11)()
            _check(self.ctx.lib.pmc_darcy_vcycle_level(self.h, level, v, C.byref(nv), info))
            out.append(dict(zip(keys, list(info))))
            v += 1
            if v >= nv.value:
                return out

    def vcycle_prolongator(self, level, vlevel):
        """P from V-cycle level vlevel + 1 to vlevel of `level` (pmc_darcy_vcycle_prolongator) as a scipy CSR matrix; the
        rows of vlevel 0 in the caller's numbering"""
        import scipy.sparse as sp
        nr, nc, nnz = C.c_int(0), C.c_int(0), C.c_int64(0)
        _check(self.ctx.lib.pmc_darcy_vcycle_prolongator(self.h, level, vlevel, C.byref(nr), C.byref(nc), C.byref(nnz),
                                                         None, None, None))
        rp = np.empty(nr.value + 1, dtype=np.int32)
        ci = np.empty(nnz.value, dtype=np.int32)
        va = np.empty(nnz.value, dtype=np.float64)
        _check(self.ctx.lib.pmc_darcy_vcycle_prolongator(self.h, level, vlevel, C.byref(nr), C.byref(nc), C.byref(nnz),
                                                         rp.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         va.ctypes.data_as(C.POINTER(C.c_double))))
        return sp.csr_matrix((va, ci, rp), shape=(nr.value, nc.value))

    def SetObservations(self, level, Gobs):
        """Gobs: scipy sparse (nobs, n_p): rows are the observation functionals g_obs_i of the level."""
        keep = _Keep()
        g = keep.csr(Gobs)
        _check(self.ctx.lib.pmc_darcy_set_observations(self.h, level, C.byref(g)))

    def SetTracer(self, level, tracer, kind=0):
        """Make the travel-time QoI of `tracer` (kind: Tracer.MEAN | Tracer.MIN) the Q of SolveFwd / SolveFwd_RtnPressure on
        `level` (pmc_darcy_set_tracer); None detaches.  ComputeG, the gradients and the Hessian actions keep <obs, x>."""
        _check(self.ctx.lib.pmc_darcy_set_tracer(self.h, level, None if tracer is None else tracer.h, int(kind)))
        self._tracers = getattr(self, "_tracers", {})
        self._tracers[level] = tracer          # keeps an attached tracer alive

    def SetTransport(self, level, transport, kind=0):
        """Make the solute-transport QoI of `transport` (kind: Transport.MASS_OUT | Transport.STORED) the Q of SolveFwd /
        SolveFwd_RtnPressure on `level` (pmc_darcy_set_transport); None detaches.  ComputeG, the gradients and the Hessian
        actions keep <obs, x>.  A level holds a tracer or a transport, not both."""
        _check(self.ctx.lib.pmc_darcy_set_transport(self.h, level, None if transport is None else transport.h, int(kind)))
        self._transports = getattr(self, "_transports", {})
        self._transports[level] = transport    # keeps an attached handle alive

    def ComputeG(self, level, k, nbatch=None):
        """BayesianInverseProblem::ComputeG: returns (G (nbatch, nobs), C, Q)."""
        if isinstance(k, np.ndarray):
            k = _f64(np.atleast_2d(k))
            nbatch = k.shape[0]
        nobs = self.ctx.lib.pmc_darcy_num_observations(self.h, level)
        G = np.empty((nbatch, nobs))
        Q = np.empty(nbatch)
        Cc = np.empty(nbatch)
        pk, ms = _addr(k)
        _check(self.ctx.lib.pmc_darcy_compute_G(self.h, level, nbatch, pk, _ptr(G, C.c_double), _ptr(Cc, C.c_double),
                                                _ptr(Q, C.c_double), ms, None))
        return G, Cc, Q

    def SolveFwd_RtnPressure(self, level, k, compute_Q=True):
        """Returns (P, C, Q): pressure block (nbatch, n_p), dof counts, QoI (None unless compute_Q)."""
        k = _f64(np.atleast_2d(k))
        nb = k.shape[0]
        n_p = self.problem.levels[level].n_p
        P = np.empty((nb, n_p))
        Q = np.empty(nb)
        Cc = np.empty(nb)
        stats = (pmc_stats * nb)()
        _check(self.ctx.lib.pmc_darcy_solve_fwd_pressure(self.h, level, nb, k.ctypes.data, P.ctypes.data,
                                                         _ptr(Cc, C.c_double), _ptr(Q, C.c_double),
                                                         1 if compute_Q else 0, PMC_MEM_HOST, stats))
        return P, Cc, (Q if compute_Q else None)

    # ---- adjoint gradients with respect to k --------------------------------------------------
    def _grad_out(self, level, k, nbatch, grad_out):
        """(k, nbatch, grad): numpy k -> a new numpy gradient; device k -> grad_out (a DeviceArray / tensor) is required"""
        if isinstance(k, np.ndarray):
            k = _f64(np.atleast_2d(k))
            nbatch = k.shape[0]
            if grad_out is None:
                grad_out = np.empty((nbatch, self.problem.levels[level].n_p))
        assert nbatch is not None and grad_out is not None
        if _addr(k)[1] != _addr(grad_out)[1]:
            raise ValueError("k and the gradient must share a memory space")
        return k, nbatch, grad_out

    def _same_space(self, ms, *arrays):
        out = []
        for a in arrays:
            if isinstance(a, np.ndarray):
                a = _f64(np.atleast_2d(a))
            p, m = _addr(a)
            if a is not None and m != ms:
                raise ValueError("all arrays of a call must share a memory space")
            out.append((a, p))
        return out

    def mass_sensitivity_time(self):
        """the gradient's mass-sensitivity kernel under set_operator_timing: (bracket ms, launches, empty-bracket ms)"""
        ms, n, gap = C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_mass_sensitivity_time(self.h, C.byref(ms), C.byref(n), C.byref(gap)))
        return ms.value, n.value, gap.value

    def mass_sensitivity_bytes(self, level, nbatch):
        b = C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_mass_sensitivity_bytes(self.h, level, nbatch, C.byref(b)))
        return b.value

    def mass_sensitivity(self, level, k, x, lam, wrt_log=False, nbatch=None, grad_out=None):
        """g[b, e] = -c'(k) lam_u^T M_e x_u for caller-supplied full vectors x, lam (nbatch, n_u + n_p); no solve
        (pmc_darcy_mass_sensitivity).  numpy arrays, or DeviceArrays / device tensors with nbatch and grad_out."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        (x, px), (lam, pl) = self._same_space(ms, x, lam)
        _check(self.ctx.lib.pmc_darcy_mass_sensitivity(self.h, level, nbatch, pk, px, pl, 1 if wrt_log else 0,
                                                       _addr(grad)[0], ms))
        return grad

    def solve_gradient(self, level, k, adj_rhs=None, wrt_log=False, nbatch=None, grad_out=None, want_solution=False,
                       sol_out=None, adj_out=None, return_stats=False):
        """Forward solve, adjoint solve, gradient (pmc_darcy_solve_gradient): returns (Q, C, grad) - plus (x, lam) with
        want_solution or given sol_out / adj_out, plus the (forward, adjoint) stats lists with return_stats.  adj_rhs None:
        J = Q (the level's obs)."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        if want_solution and ms == PMC_MEM_HOST:
            n = self.GetGlobalNumberOfDofs(level)
            sol_out = np.empty((nbatch, n)) if sol_out is None else sol_out
            adj_out = np.empty((nbatch, n)) if adj_out is None else adj_out
        (adj_rhs, pr), (sol_out, ps), (adj_out, pa) = self._same_space(ms, adj_rhs, sol_out, adj_out)
        Q, Cc = np.empty(nbatch), np.empty(nbatch)
        sf, sa = (pmc_stats * nbatch)(), (pmc_stats * nbatch)()
        _check(self.ctx.lib.pmc_darcy_solve_gradient(self.h, level, nbatch, pk, pr, 1 if wrt_log else 0,
                                                     _ptr(Q, C.c_double), _ptr(Cc, C.c_double), _addr(grad)[0], ps, pa, ms,
                                                     sf, sa))
        out = [Q, Cc, grad]
        if sol_out is not None or adj_out is not None:
            out += [sol_out, adj_out]
        if return_stats:
            out += [[(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in st] for st in (sf, sa)]
        return tuple(out)

    def loglik_gradient(self, level, k, data, noise, wrt_log=False, nbatch=None, grad_out=None):
        """Gradient of the Gaussian log-likelihood of the observation functionals set with SetObservations
        (pmc_darcy_loglik_gradient): returns (loglik (nbatch,), G (nbatch, nobs), grad)."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        nobs = max(self.ctx.lib.pmc_darcy_num_observations(self.h, level), 0)
        data = _f64(np.asarray(data, dtype=np.float64).ravel())
        if nobs and data.size != nobs:
            raise ValueError("data must hold one value per observation functional")
        ll, G = np.empty(nbatch), np.empty((nbatch, nobs))
        _check(self.ctx.lib.pmc_darcy_loglik_gradient(self.h, level, nbatch, pk, _ptr(data, C.c_double), float(noise),
                                                      1 if wrt_log else 0, _ptr(ll, C.c_double), _ptr(G, C.c_double),
                                                      _addr(grad)[0], ms, None))
        return ll, G, grad

    # ---- gradients of breakthrough data through a transport's adjoint ---------------------------
    def TransportGradient(self, level, transport, k, curve_bar=None, stored_bar=None, wrt_log=False, nbatch=None, grad_out=None,
                          want_solution=False, return_stats=False):
        """dJ/dk (dJ/dlog k) of J = <curve_bar, curve> + stored_bar stored of `transport` (a capi.Transport of the level's
        sizes) on the flux of the Darcy solution (pmc_darcy_transport_gradient).  k and the seeds numpy, or all on the device
        with nbatch and grad_out.  Returns a dict of grad, curve (nbatch x nreport), stored and status (numpy int32) - plus sol
        and adj with want_solution, plus stats (forward, adjoint) with return_stats."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        host = ms == PMC_MEM_HOST
        nr, n = (transport.nreport if transport is not None else 1), self.GetGlobalNumberOfDofs(level)   # None: the library refuses
        if host and transport is not None:
            curve_bar = None if curve_bar is None else _f64(np.atleast_2d(curve_bar))
            stored_bar = None if stored_bar is None else _f64(np.atleast_1d(stored_bar))
            if (curve_bar is not None and curve_bar.shape != (nbatch, nr)) or (stored_bar is not None and stored_bar.shape != (nbatch,)):
                raise ValueError("curve_bar must be nbatch x nreport and stored_bar nbatch")
        new = (lambda *shape: np.empty(shape)) if host else (lambda *shape: DeviceArray(self.ctx, int(np.prod(shape))))
        curve, stored = new(nbatch, nr), new(nbatch)
        sol, adj = (new(nbatch, n), new(nbatch, n)) if want_solution else (None, None)
        for a in (curve_bar, stored_bar):
            if a is not None and _addr(a)[1] != ms:
                raise ValueError("all arrays of a call must share a memory space")
        status = np.empty(nbatch, np.int32)
        sf, sa = (pmc_stats * nbatch)(), (pmc_stats * nbatch)()
        _check(self.ctx.lib.pmc_darcy_transport_gradient(
            self.h, level, None if transport is None else transport.h, nbatch, pk, _addr(curve_bar)[0], _addr(stored_bar)[0],
            1 if wrt_log else 0, _addr(curve)[0], _addr(stored)[0], _ptr(status, C.c_int32), _addr(grad)[0], _addr(sol)[0],
            _addr(adj)[0], ms, sf, sa))
        out = dict(grad=grad, curve=curve, stored=stored, status=status)
        if want_solution:
            out.update(sol=sol, adj=adj)
        if return_stats:
            out["stats"] = [[(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in st] for st in (sf, sa)]
        return out

    def TransportLoglikGradient(self, level, transport, k, data, noise, wrt_log=False, nbatch=None, grad_out=None):
        """loglik = -|curve - data|^2 / (2 noise) of the breakthrough curve of `transport` and its gradient in k
        (pmc_darcy_transport_loglik_gradient): returns (loglik (nbatch,), curve (nbatch, nreport), status, grad)."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        data = None if data is None else _f64(np.asarray(data, dtype=np.float64).ravel())
        if data is not None and data.size != transport.nreport:
            raise ValueError("data must hold one value per report time")
        ll, curve, status = np.empty(nbatch), np.empty((nbatch, transport.nreport)), np.empty(nbatch, np.int32)
        _check(self.ctx.lib.pmc_darcy_transport_loglik_gradient(
            self.h, level, transport.h, nbatch, pk, None if data is None else _ptr(data, C.c_double), float(noise),
            1 if wrt_log else 0, _ptr(ll, C.c_double), _ptr(curve, C.c_double), _ptr(status, C.c_int32), _addr(grad)[0], ms, None))
        return ll, curve, status, grad

    # ---- gradients of travel times through a tracer's adjoint -------------------------------------
    def tracer_gradient(self, level, tracer, k, T_bar, wrt_log=False, nbatch=None, grad_out=None, want_solution=False,
                        return_stats=False):
        """dJ/dk (dJ/dlog k) of J = <T_bar, T> of `tracer` (a capi.Tracer of the level's sizes) on the flux of the Darcy solution
        (pmc_darcy_tracer_gradient).  k and T_bar (nbatch x nparticles) numpy, or both on the device with nbatch and grad_out.
        Returns a dict of grad, T and status (nbatch x nparticles) - plus sol and adj with want_solution, plus stats (forward,
        adjoint) with return_stats."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        host = ms == PMC_MEM_HOST
        npart, n = (tracer.nparticles if tracer is not None else 1), self.GetGlobalNumberOfDofs(level)   # None: the library refuses
        if host and T_bar is not None:
            T_bar = _f64(np.atleast_2d(T_bar))
            if tracer is not None and T_bar.shape != (nbatch, npart):
                raise ValueError("T_bar must be nbatch x nparticles")
        if T_bar is not None and _addr(T_bar)[1] != ms:
            raise ValueError("all arrays of a call must share a memory space")
        new = (lambda *shape: np.empty(shape)) if host else (lambda *shape: DeviceArray(self.ctx, int(np.prod(shape))))
        T = new(nbatch, npart)
        status = np.empty((nbatch, npart), np.int32) if host else DeviceInt32Array(self.ctx, nbatch * npart)
        sol, adj = (new(nbatch, n), new(nbatch, n)) if want_solution else (None, None)
        sf, sa = (pmc_stats * nbatch)(), (pmc_stats * nbatch)()
        _check(self.ctx.lib.pmc_darcy_tracer_gradient(
            self.h, level, None if tracer is None else tracer.h, nbatch, pk, _addr(T_bar)[0], 1 if wrt_log else 0, _addr(T)[0],
            status.ctypes.data if host else status.ptr, _addr(grad)[0], _addr(sol)[0], _addr(adj)[0], ms, sf, sa))
        out = dict(grad=grad, T=T, status=status)
        if want_solution:
            out.update(sol=sol, adj=adj)
        if return_stats:
            out["stats"] = [[(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in st] for st in (sf, sa)]
        return out

    def tracer_loglik_gradient(self, level, tracer, k, data, noise, wrt_log=False, nbatch=None, grad_out=None):
        """loglik = -|T - data|^2 / (2 noise) of the travel times of `tracer` and its gradient in k
        (pmc_darcy_tracer_loglik_gradient): returns (loglik (nbatch,), T (nbatch, nparticles), not_exited (nbatch,), grad).  A
        column with not_exited > 0 has a zero gradient."""
        k, nbatch, grad = self._grad_out(level, k, nbatch, grad_out)
        pk, ms = _addr(k)
        data = None if data is None else _f64(np.asarray(data, dtype=np.float64).ravel())
        if data is not None and data.size != tracer.nparticles:
            raise ValueError("data must hold one value per particle")
        ll, T, nex = np.empty(nbatch), np.empty((nbatch, tracer.nparticles)), np.empty(nbatch, np.int32)
        _check(self.ctx.lib.pmc_darcy_tracer_loglik_gradient(
            self.h, level, tracer.h, nbatch, pk, None if data is None else _ptr(data, C.c_double), float(noise),
            1 if wrt_log else 0, _ptr(ll, C.c_double), _ptr(T, C.c_double), _ptr(nex, C.c_int32), _addr(grad)[0], ms, None))
        return ll, T, nex, grad

    # ---- Gauss-Newton Hessian-vector products in k ----------------------------------------------
    def mass_tangent_time(self):
        """the tangent right-hand side kernel under set_operator_timing: (bracket ms, launches, empty-bracket ms)"""
        ms, n, gap = C.c_double(0.0), C.c_int64(0), C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_mass_tangent_time(self.h, C.byref(ms), C.byref(n), C.byref(gap)))
        return ms.value, n.value, gap.value

    def mass_tangent_bytes(self, level, nbatch):
        b = C.c_double(0.0)
        _check(self.ctx.lib.pmc_darcy_mass_tangent_bytes(self.h, level, nbatch, C.byref(b)))
        return b.value

    def mass_tangent(self, level, k, x, dk, wrt_log=False, nbatch=None, t_out=None):
        """t[b, :] = the tangent right-hand side -dA/dk[dk] x on the free u-rows, 0 elsewhere, for caller-supplied full
        vectors x (nbatch, n_u + n_p) and directions dk (nbatch, n_p); no solve (pmc_darcy_mass_tangent).  numpy arrays, or
        DeviceArrays / device tensors with nbatch and t_out."""
        if isinstance(k, np.ndarray):
            k = _f64(np.atleast_2d(k))
            nbatch = k.shape[0]
            if t_out is None:
                t_out = np.empty((nbatch, self.GetGlobalNumberOfDofs(level)))
        assert nbatch is not None and t_out is not None
        pk, ms = _addr(k)
        (x, px), (dk, pd), (t_out, pt) = self._same_space(ms, x, dk, t_out)
        _check(self.ctx.lib.pmc_darcy_mass_tangent(self.h, level, nbatch, pk, px, pd, 1 if wrt_log else 0, pt, ms))
        return t_out

    def gn_hessvec(self, level, k, dk, noise, wrt_log=False, x_in=None, nbatch=None, hv_out=None, want_solution=False,
                   x_out=None, return_stats=False):
        """hv = J^T (1/noise) J dk of the observation functionals set with SetObservations (pmc_darcy_gn_hessvec): returns
        (hv, dG (nbatch, nobs)) - plus x with want_solution or a given x_out (only without x_in: the forward solve then runs
        inside), plus the (tangent, adjoint) stats lists with return_stats."""
        k, nbatch, hv = self._grad_out(level, k, nbatch, hv_out)
        pk, ms = _addr(k)
        if want_solution and ms == PMC_MEM_HOST and x_out is None:
            x_out = np.empty((nbatch, self.GetGlobalNumberOfDofs(level)))
        (dk, pd), (x_in, pi), (x_out, po) = self._same_space(ms, dk, x_in, x_out)
        nobs = max(self.ctx.lib.pmc_darcy_num_observations(self.h, level), 0)
        dG = np.empty((nbatch, nobs))
        st, sa = (pmc_stats * nbatch)(), (pmc_stats * nbatch)()
        _check(self.ctx.lib.pmc_darcy_gn_hessvec(self.h, level, nbatch, pk, pi, pd, float(noise), 1 if wrt_log else 0,
                                                 _addr(hv)[0], _ptr(dG, C.c_double), po, ms, st, sa))
        out = [hv, dG]
        if x_out is not None:
            out.append(x_out)
        if return_stats:
            out += [[(s.iterations, s.converged, s.initial_norm, s.final_norm) for s in t] for t in (st, sa)]
        return tuple(out)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pmc_darcy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NewtonCG:
    """Batched CG vector algebra for Newton-CG (pmc_ncg_*, csrc/newton_cg.hip): nb <= nbatch_max independent CG iterations
    on columns of length n.  The caller applies the operator to search_direction() and hands the product to step().  Array
    arguments: numpy (host), DeviceArray or torch tensors (device), sample-major nb x n."""

    def __init__(self, ctx: Context, n: int, nbatch_max: int):
        self.ctx, self.n, self.nbatch_max = ctx, int(n), int(nbatch_max)
        h = _VP()
        _check(ctx.lib.pmc_ncg_create(ctx.h, self.n, self.nbatch_max, C.byref(h)))
        self.h = h
        ctx._adopt(self)

    @staticmethod
    def _space(*arrays):
        spaces = {_addr(a)[1] for a in arrays if a is not None and not isinstance(a, int)}
        assert len(spaces) <= 1, "arguments in different memory spaces"
        return spaces.pop() if spaces else PMC_MEM_DEVICE

    @staticmethod
    def _p(a):
        return a if a is None or isinstance(a, int) else _addr(a)[0]

    def begin(self, nb, g, eta, active=None):
        eta = _f64(eta)
        assert eta.size == nb
        act = None if active is None else _i32(active)
        _check(self.ctx.lib.pmc_ncg_begin(self.h, nb, self._p(g), _ptr(eta, C.c_double),
                                          None if act is None else _ptr(act, C.c_int32), self._space(g)))

    def step(self, nb, Hp):
        _check(self.ctx.lib.pmc_ncg_step(self.h, nb, self._p(Hp), self._space(Hp)))

    def status(self, nb):
        """(rr, cg_count, done, nonpos_curvature): numpy arrays of nb"""
        rr = np.empty(nb)
        cnt, done, npc = (np.empty(nb, np.int32) for _ in range(3))
        _check(self.ctx.lib.pmc_ncg_status(self.h, nb, _ptr(rr, C.c_double), _ptr(cnt, C.c_int32), _ptr(done, C.c_int32),
                                           _ptr(npc, C.c_int32)))
        return rr, cnt, done, npc

    # the workspace's own vectors: device addresses (ints), accepted by axpy_cols / dot_cols in either memory space
    def direction_ptr(self) -> int:
        return self.ctx.lib.pmc_ncg_direction(self.h) or 0

    def search_direction_ptr(self) -> int:
        return self.ctx.lib.pmc_ncg_search_direction(self.h) or 0

    def residual_ptr(self) -> int:
        return self.ctx.lib.pmc_ncg_residual(self.h) or 0

    def _download(self, ptr, nb):
        out = np.empty((nb, self.n))
        _check(self.ctx.lib.pmc_memcpy_d2h(self.ctx.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def direction(self, nb) -> np.ndarray:
        return self._download(self.direction_ptr(), nb)

    def search_direction(self, nb) -> np.ndarray:
        return self._download(self.search_direction_ptr(), nb)

    def residual(self, nb) -> np.ndarray:
        return self._download(self.residual_ptr(), nb)

    def axpy_cols(self, nb, t, x, d, out):
        """out_b = x_b + t_b d_b on the columns with t_b != 0 (d None: a masked copy); the others are not written"""
        t = _f64(t)
        assert t.size == nb
        _check(self.ctx.lib.pmc_ncg_axpy_cols(self.h, nb, _ptr(t, C.c_double), self._p(x), self._p(d), self._p(out),
                                              self._space(x, d, out)))
        return out

    def dot_cols(self, nb, a, b) -> np.ndarray:
        out = np.empty(nb)
        _check(self.ctx.lib.pmc_ncg_dot_cols(self.h, nb, self._p(a), self._p(b), _ptr(out, C.c_double), self._space(a, b)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pmc_ncg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tracer:
    """Particle travel times on the RT0 Darcy flux (pmc_tracer_*, csrc/tracer.hip).

    mesh: a parelagmc_amd.fe.tracer.TracerMesh (fe.tracer.tracer_mesh of a level); x0: (nparticles, 3) start points;
    elem0: their elements (None: found geometrically, fe.tracer.locate); max_steps 0: 64 + 32 ceil(cbrt(n_elem))."""

    EXITED, STAGNANT, MAX_STEPS = 0, 1, 2
    MEAN, MIN = 0, 1

    def __init__(self, ctx: Context, mesh, x0, elem0=None, max_steps: int = 0):
        self.ctx = ctx
        x0 = _f64(np.atleast_2d(x0))
        if elem0 is None:
            from .fe.tracer import locate
            elem0 = locate(mesh, x0)
        elem0 = _i32(elem0)
        if x0.shape != (elem0.size, 3):
            raise ValueError("x0 must be nparticles x 3 and elem0 nparticles")
        keep = _Keep()
        sign = np.ascontiguousarray(mesh.elem_sign, dtype=np.int8)
        m = pmc_tracer_mesh(int(mesh.kind), int(mesh.n_elem), int(mesh.n_face), keep.i32(mesh.elem_face),
                            sign.ctypes.data_as(C.POINTER(C.c_int8)), keep.i32(mesh.face_elem), keep.f64(mesh.geom),
                            None if mesh.porosity is None else keep.f64(mesh.porosity))
        h = _VP()
        _check(ctx.lib.pmc_tracer_create(ctx.h, C.byref(m), int(elem0.size), _ptr(x0, C.c_double), _ptr(elem0, C.c_int32),
                                         int(max_steps), C.byref(h)))
        self.h = h
        self.n_face, self.nparticles = int(mesh.n_face), int(elem0.size)
        ctx._adopt(self)

    def Run(self, u, nbatch=None, ld=None, want_x=True):
        """Walk every particle through nbatch flux fields.  u: numpy (nbatch, ld >= n_face) - e.g. sol_out of SolveFwd - or a
        DeviceArray / torch tensor on the device with nbatch (and ld, default n_face) given.  Returns a dict of T, exit_face,
        status, nsteps (nbatch x nparticles) and x_exit (nbatch x nparticles x 3, unless want_x is False): numpy arrays for
        a numpy u, flat DeviceArray / DeviceInt32Array buffers on the device otherwise."""
        npart = self.nparticles
        if isinstance(u, np.ndarray):
            u = _f64(np.atleast_2d(u))
            nbatch, ld = u.shape
            T = np.empty((nbatch, npart))
            ints = [np.empty((nbatch, npart), np.int32) for _ in range(3)]
            x = np.empty((nbatch, npart, 3)) if want_x else None
            pu, ms = u.ctypes.data, PMC_MEM_HOST
            addr = lambda a: None if a is None else a.ctypes.data
        else:
            assert nbatch is not None
            ld = self.n_face if ld is None else int(ld)
            pu, ms = _addr(u)
            assert ms == PMC_MEM_DEVICE
            T = DeviceArray(self.ctx, nbatch * npart)
            ints = [DeviceInt32Array(self.ctx, nbatch * npart) for _ in range(3)]
            x = DeviceArray(self.ctx, nbatch * npart * 3) if want_x else None
            addr = lambda a: None if a is None else a.ptr
        _check(self.ctx.lib.pmc_tracer_run(self.h, int(nbatch), pu, int(ld), addr(T), addr(ints[0]), addr(ints[1]),
                                           addr(ints[2]), addr(x), ms))
        out = dict(T=T, exit_face=ints[0], status=ints[1], nsteps=ints[2])
        if want_x:
            out["x_exit"] = x
        return out

    def run_adjoint(self, u, T_bar=None, x_exit_bar=None, nbatch=None, ld=None, ld_bar=None, want_x0_bar=True):
        """u_bar = dJ/du and x0_bar = dJ/dx0 of J = <T_bar, T> + <x_exit_bar, x_exit> per column, the decisions of the walk held
        (pmc_tracer_run_adjoint).  u and the seeds: numpy (u: nbatch x ld >= n_face), or DeviceArrays /
        device tensors with nbatch (and ld, default n_face).  Returns a dict of u_bar (nbatch x ld_bar, default n_face; only the
        first n_face entries of a row are written), x0_bar (nbatch x nparticles x 3, unless want_x0_bar is False), T,
        exit_face, status and nsteps.  Particles that did not exit contribute nothing."""
        npart = self.nparticles
        seeds = [T_bar, x_exit_bar]
        if isinstance(u, np.ndarray):
            u = _f64(np.atleast_2d(u))
            nbatch, ld = u.shape
            ld_bar = self.n_face if ld_bar is None else int(ld_bar)
            for i, (a, shape) in enumerate(zip(seeds, [(nbatch, npart), (nbatch, npart, 3)])):
                if a is not None:
                    seeds[i] = _f64(a).reshape(shape)
            out = dict(u_bar=np.zeros((nbatch, max(ld_bar, 0))), x0_bar=np.empty((nbatch, npart, 3)) if want_x0_bar else None,
                       T=np.empty((nbatch, npart)), exit_face=np.empty((nbatch, npart), np.int32),
                       status=np.empty((nbatch, npart), np.int32), nsteps=np.empty((nbatch, npart), np.int32))
            pu, ms = u.ctypes.data, PMC_MEM_HOST
            addr = lambda a: None if a is None else a.ctypes.data
        else:
            assert nbatch is not None
            ld = self.n_face if ld is None else int(ld)
            ld_bar = self.n_face if ld_bar is None else int(ld_bar)
            pu, ms = _addr(u)
            assert ms == PMC_MEM_DEVICE and all(a is None or _addr(a)[1] == ms for a in seeds)
            dev = lambda n: DeviceArray(self.ctx, n)
            idev = lambda: DeviceInt32Array(self.ctx, nbatch * npart)
            out = dict(u_bar=dev(nbatch * max(ld_bar, 1)), x0_bar=dev(nbatch * npart * 3) if want_x0_bar else None,
                       T=dev(nbatch * npart), exit_face=idev(), status=idev(), nsteps=idev())
            addr = lambda a: None if a is None else (a.ptr if isinstance(a, (DeviceArray, DeviceInt32Array)) else _addr(a)[0])
        _check(self.ctx.lib.pmc_tracer_run_adjoint(self.h, int(nbatch), pu, int(ld), addr(seeds[0]), addr(seeds[1]),
                                                   addr(out["u_bar"]), int(ld_bar), *[addr(out[k]) for k in
                                                                                      ("x0_bar", "T", "exit_face", "status", "nsteps")], ms))
        if not want_x0_bar:
            del out["x0_bar"]
        return out

    def reduce_seed(self, T, status, kind=0):
        """T_bar = dQ/dT of the Q of Reduce (pmc_tracer_reduce_seed): numpy (nbatch x nparticles) for numpy inputs, a DeviceArray
        for the device buffers of Run"""
        if isinstance(T, np.ndarray):
            T = _f64(np.atleast_2d(T))
            status = _i32(np.atleast_2d(status))
            nbatch = T.shape[0]
            out = np.empty(T.shape)
            pT, ps, po, ms = T.ctypes.data, status.ctypes.data, out.ctypes.data, PMC_MEM_HOST
        else:
            nbatch = T.n // self.nparticles
            out = DeviceArray(self.ctx, nbatch * self.nparticles)
            pT, ps, po, ms = T.ptr, status.ptr, out.ptr, PMC_MEM_DEVICE
        _check(self.ctx.lib.pmc_tracer_reduce_seed(self.h, nbatch, pT, ps, int(kind), po, ms))
        return out

    def set_adjoint_scratch(self, nbytes=0):
        """the cap in bytes on the records of one chunk of columns of run_adjoint; 0: 256 MiB.  The results do not depend on
        it."""
        _check(self.ctx.lib.pmc_tracer_set_adjoint_scratch(self.h, int(nbytes)))

    def adjoint_chunks(self):
        """column chunks of the last adjoint launch"""
        return int(self.ctx.lib.pmc_tracer_adjoint_chunks(self.h))

    def Reduce(self, T, status, kind=0):
        """(Q, not_exited) per realization: the mean (MEAN) or minimum (MIN) travel time and the particles that did not exit"""
        if isinstance(T, np.ndarray):
            T = _f64(np.atleast_2d(T))
            status = _i32(np.atleast_2d(status))
            nbatch = T.shape[0]
            pT, ps, ms = T.ctypes.data, status.ctypes.data, PMC_MEM_HOST
        else:
            nbatch = T.n // self.nparticles
            pT, ps, ms = T.ptr, status.ptr, PMC_MEM_DEVICE
        Q = np.empty(nbatch)
        nex = np.empty(nbatch, np.int32)
        _check(self.ctx.lib.pmc_tracer_reduce(self.h, nbatch, pT, ps, int(kind), _ptr(Q, C.c_double), _ptr(nex, C.c_int32), ms))
        return Q, nex

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pmc_tracer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Transport:
    """First-order upwind transport of a passive solute on the Darcy flux (pmc_transport_*, csrc/transport.hip; DESIGN.md
    section 21).

    mesh: a parelagmc_amd.fe.transport.TransportMesh (fe.transport.transport_mesh of a Darcy level and its element volumes);
    t_end: the time to advance to; cfl in (0, 1]; nreport: points of the breakthrough curve; max_steps 0: 65536."""

    OK, STEP_LIMIT, BAD_FLUX = 0, 1, 2
    MASS_OUT, STORED = 0, 1

    def __init__(self, ctx: Context, mesh, t_end: float, cfl: float = 0.9, nreport: int = 1, max_steps: int = 0):
        self.ctx = ctx
        keep = _Keep()
        opt = lambda a: None if a is None else keep.f64(a)
        outlet = None
        if mesh.outlet is not None:
            flags = np.ascontiguousarray(mesh.outlet, dtype=np.uint8)
            keep.refs.append(flags)
            outlet = flags.ctypes.data_as(C.POINTER(C.c_uint8))
        m = pmc_transport_mesh(int(mesh.n_elem), int(mesh.n_face), keep.i32(mesh.rowptr), keep.i32(mesh.col), keep.f64(mesh.val),
                               keep.f64(mesh.pore_volume), opt(mesh.c0), opt(mesh.c_in), outlet, opt(mesh.weight))
        prm = pmc_transport_params(float(t_end), float(cfl), int(nreport), int(max_steps))
        h = _VP()
        _check(ctx.lib.pmc_transport_create(ctx.h, C.byref(m), C.byref(prm), C.byref(h)))
        self.h = h
        size = [C.c_int() for _ in range(4)]
        _check(ctx.lib.pmc_transport_size(h, *[C.byref(x) for x in size]))
        self.n_elem, self.n_face, self.n_outlet, self.nreport = (x.value for x in size)
        ctx._adopt(self)

    def Run(self, u, nbatch=None, ld=None, want_c=True):
        """Advance nbatch flux fields to t_end.  u: numpy (nbatch, ld >= n_face) - e.g. sol_out of SolveFwd - or a DeviceArray /
        torch tensor on the device with nbatch (and ld, default n_face) given.  Returns a dict of c (nbatch x n_elem, unless
        want_c is False), curve (nbatch x nreport), stored, rate, t_reached, nsteps and status (nbatch): numpy arrays for a
        numpy u, flat DeviceArray / DeviceInt32Array buffers on the device otherwise."""
        ne, nr = self.n_elem, self.nreport
        if isinstance(u, np.ndarray):
            u = _f64(np.atleast_2d(u))
            nbatch, ld = u.shape
            out = dict(c=np.empty((nbatch, ne)) if want_c else None, curve=np.empty((nbatch, nr)), stored=np.empty(nbatch),
                       rate=np.empty(nbatch), t_reached=np.empty(nbatch), nsteps=np.empty(nbatch, np.int32),
                       status=np.empty(nbatch, np.int32))
            pu, ms = u.ctypes.data, PMC_MEM_HOST
            addr = lambda a: None if a is None else a.ctypes.data
        else:
            assert nbatch is not None
            ld = self.n_face if ld is None else int(ld)
            pu, ms = _addr(u)
            assert ms == PMC_MEM_DEVICE
            dev = lambda n: DeviceArray(self.ctx, n)
            out = dict(c=dev(nbatch * ne) if want_c else None, curve=dev(nbatch * nr), stored=dev(nbatch), rate=dev(nbatch),
                       t_reached=dev(nbatch), nsteps=DeviceInt32Array(self.ctx, nbatch), status=DeviceInt32Array(self.ctx, nbatch))
            addr = lambda a: None if a is None else a.ptr
        _check(self.ctx.lib.pmc_transport_run(self.h, int(nbatch), pu, int(ld), *[addr(out[k]) for k in
                                              ("c", "curve", "stored", "rate", "t_reached", "nsteps", "status")], ms))
        if not want_c:
            del out["c"]
        return out

    def run_adjoint(self, u, curve_bar=None, stored_bar=None, c_bar=None, nbatch=None, ld=None, ld_bar=None, want_c0_bar=True):
        """u_bar = dJ/du and c0_bar = dJ/dc0 of J = <curve_bar, curve> + stored_bar stored + <c_bar, c> per column
        (pmc_transport_run_adjoint).  u and the seeds: numpy (u: nbatch x ld >= n_face), or DeviceArrays /
        device tensors with nbatch (and ld, default n_face).  Returns a dict of u_bar (nbatch x ld_bar, default n_face; only the
        first n_face entries of a row are written), c0_bar (unless want_c0_bar is False), curve, stored, nsteps and status."""
        ne, nr = self.n_elem, self.nreport
        seeds = [curve_bar, stored_bar, c_bar]
        if isinstance(u, np.ndarray):
            u = _f64(np.atleast_2d(u))
            nbatch, ld = u.shape
            ld_bar = self.n_face if ld_bar is None else int(ld_bar)
            shapes = [(nbatch, nr), (nbatch,), (nbatch, ne)]
            for i, (a, shape) in enumerate(zip(seeds, shapes)):
                if a is not None:
                    seeds[i] = _f64(a).reshape(shape)
            out = dict(u_bar=np.zeros((nbatch, max(ld_bar, 0))), c0_bar=np.empty((nbatch, ne)) if want_c0_bar else None,
                       curve=np.empty((nbatch, nr)), stored=np.empty(nbatch), nsteps=np.empty(nbatch, np.int32),
                       status=np.empty(nbatch, np.int32))
            pu, ms = u.ctypes.data, PMC_MEM_HOST
            addr = lambda a: None if a is None else a.ctypes.data
        else:
            assert nbatch is not None
            ld = self.n_face if ld is None else int(ld)
            ld_bar = self.n_face if ld_bar is None else int(ld_bar)
            pu, ms = _addr(u)
            assert ms == PMC_MEM_DEVICE and all(a is None or _addr(a)[1] == ms for a in seeds)
            dev = lambda n: DeviceArray(self.ctx, n)
            out = dict(u_bar=dev(nbatch * max(ld_bar, 1)), c0_bar=dev(nbatch * ne) if want_c0_bar else None, curve=dev(nbatch * nr),
                       stored=dev(nbatch), nsteps=DeviceInt32Array(self.ctx, nbatch), status=DeviceInt32Array(self.ctx, nbatch))
            addr = lambda a: None if a is None else (a.ptr if isinstance(a, DeviceArray) else _addr(a)[0])
        _check(self.ctx.lib.pmc_transport_run_adjoint(self.h, int(nbatch), pu, int(ld), *[addr(a) for a in seeds], addr(out["u_bar"]),
                                                      int(ld_bar), *[addr(out[k]) for k in ("c0_bar", "curve", "stored", "nsteps",
                                                                                            "status")], ms))
        if not want_c0_bar:
            del out["c0_bar"]
        return out

    def set_adjoint_segment(self, K=0):
        """the number of steps between two kept states of run_adjoint; 0: ceil(sqrt(largest step count)).  The results do
        not depend on it."""
        _check(self.ctx.lib.pmc_transport_set_adjoint_segment(self.h, int(K)))

    def Reduce(self, curve, stored, kind=0):
        """Q per realization: the mass that left through the outlet (MASS_OUT) or the weighted mass in place (STORED)"""
        if isinstance(curve, np.ndarray):
            curve, stored = _f64(np.atleast_2d(curve)), _f64(np.atleast_1d(stored))
            nbatch = curve.shape[0]
            pc, ps, ms = curve.ctypes.data, stored.ctypes.data, PMC_MEM_HOST
        else:
            nbatch = curve.n // self.nreport
            pc, ps, ms = curve.ptr, stored.ptr, PMC_MEM_DEVICE
        Q = np.empty(nbatch)
        _check(self.ctx.lib.pmc_transport_reduce(self.h, nbatch, pc, ps, int(kind), _ptr(Q, C.c_double), ms))
        return Q

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pmc_transport_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

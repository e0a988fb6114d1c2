/* pmc_host.h - C ABI of libpmc_host.so: the host-side Monte Carlo managers.
 *
 * Restates, in C++ behind a C surface, the two outer loops that drive the hot path in the
 * reference (paths relative to /root/reference):
 *     MLMC_Manager::Run / InitRun / computeNSamplesMSE   src/MLMC_Manager.cpp:103-214,300-401
 *     MC_Manager::Run / InitRun / computeNSamplesMSE     src/MC_Manager.cpp:82-146,194-239
 * They call ONLY the MLSampler / PhysicalMLSolver plugin surface (src/MLSampler.hpp:33-52,
 * src/PhysicalMLSolver.hpp:33-47), here either the device objects of pmc.h or user callbacks
 * (any other sampler/solver, and CPU-side tests of the managers).
 *
 * New relative to the reference ("serial multi-level MC manager", src/MLMC_Manager.hpp:24):
 * realizations of one InitRun round are sharded over ranks (one rank per GPU) in blocks of
 * `batch` consecutive sample ids and the nlevels x 9 sums table is SUM-all-reduced once per
 * round before computeNSamplesMSE.
 */
#ifndef PMC_HOST_H_
#define PMC_HOST_H_

#include "pmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PMC_MLMC_NVAR 9 /* Y2,Y,ABSY,Q2,Q,ABSQ,C,Y3,Y4 - enum order of src/MLMC_Manager.hpp:65 */

typedef struct pmc_mlmc pmc_mlmc;

/* in-place SUM all-reduce of a host buffer over the sample-farm ranks */
typedef int (*pmc_reduce_fn)(double* buf, int n, void* user);

/* plugin callbacks (host pointers, batched sample-major like pmc.h) */
typedef int (*pmc_cb_sample)(void* user, int level, uint64_t first_id, int nbatch, double* xi);
typedef int (*pmc_cb_eval)(void* user, int level, int xi_level, int nbatch, const double* xi, double* s,
                           const double* init_s, int init_level, int use_init, double* embed_s_out);
typedef int (*pmc_cb_solve)(void* user, int level, int nbatch, const double* k, double* Q, double* C);

typedef struct pmc_plugin_callbacks {
    void* user;
    pmc_cb_sample sample;
    pmc_cb_eval eval;
    pmc_cb_solve solve_fwd;
    const int32_t* xi_size;     /* nlevels: size Sample() fills      */
    const int32_t* sample_size; /* nlevels: size of Eval's s         */
    const int32_t* ndofs;       /* nlevels: GetGlobalNumberOfDofs()  */
} pmc_plugin_callbacks;

/* "Problem parameters" read by the managers (src/MLMC_Manager.cpp:30-36) */
typedef struct pmc_mlmc_params {
    double eps2;              /* "Mean square error", default 0.001; < 0 = automatic        */
    double ratio;             /* "MSE splitting ratio", default 0.5                         */
    int32_t init_nsamples;    /* "Number of samples", default 10                            */
    const int32_t* array_nsamples; /* "Array number of samples" (nlevels) or NULL           */
    int32_t wall_time;        /* public member wallTime (src/MLMC_Manager.hpp:61), default 1 */
    int32_t batch;            /* upper limit of realizations per plugin call (1..256), default 256.  The managers cut a level's realizations into calls of at most this many, at most what the plugins prefer for the level (pmc_sampler_batch_width: 16 on large levels ... 256 on the smallest), cut so that every rank of a farm gets a share - independent of the lane count, so a realization's result does not depend on how many lanes share a GPU */
    int32_t max_rounds;       /* safety bound on the adaptive loop, default 1000            */
    const char* log_file;     /* "Output filename for MC managers" or NULL                  */
} pmc_mlmc_params;
void pmc_mlmc_params_default(pmc_mlmc_params* p);

typedef struct pmc_mlmc_result {
    int32_t nlevels;
    double estimate, eps2, actual_mse, estimator_variance, bias2, alpha, alpha_abs, beta, gamma;
    /* arrays of nlevels, owned by the manager, valid until the next call */
    const double *eY, *eABSY, *eQ, *eABSQ, *eC, *varY, *varQ, *consistency, *kurtosis, *VC, *cost;
    const double* sums;            /* nlevels x PMC_MLMC_NVAR, row-major */
    const int64_t* nsamples;       /* per level, global                   */
    const int64_t* nsamples_missing;
    const double* level_seconds;   /* wall time spent per level on this rank */
} pmc_mlmc_result;

/* manager over the device sampler + solver of pmc.h (device-resident vectors, no PCIe traffic) */
int pmc_mlmc_create(pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver, int nlevels,
                    const pmc_mlmc_params* params, pmc_mlmc** out);
/* add a lane: another (ctx, sampler, solver) triple built from the same operators, i.e. another HIP stream
 * that processes this rank's realizations concurrently (device-handle managers only) */
int pmc_mlmc_add_lane(pmc_mlmc* m, pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver);
/* manager over arbitrary plugins */
int pmc_mlmc_create_callbacks(int nlevels, const pmc_plugin_callbacks* cb, const pmc_mlmc_params* params,
                              pmc_mlmc** out);
void pmc_mlmc_destroy(pmc_mlmc* m);
/* sample-farm layout; reduce == NULL with nranks > 1 uses pmc_allreduce_sum_f64 (RCCL) of the ctx */
int pmc_mlmc_set_farm(pmc_mlmc* m, int nranks, int rank, pmc_reduce_fn reduce, void* user);
int pmc_mlmc_run(pmc_mlmc* m);                               /* MLMC_Manager::Run      */
int pmc_mlmc_reset(pmc_mlmc* m);                             /* zero sums and counters */
/* resume: add the realizations recorded in a per-sample log (params.log_file of an earlier run; columns level, Y, Q,
 * Q_c, cost as in the reference's MLMC.dat, src/MLMC_Manager.cpp:106-108) to the sums table and counters */
int pmc_mlmc_replay_log(pmc_mlmc* m, const char* path, int64_t* nread);
int pmc_mlmc_init_run(pmc_mlmc* m, const int32_t* nsamples); /* MLMC_Manager::InitRun  */
int pmc_mlmc_result_get(pmc_mlmc* m, pmc_mlmc_result* out);
/* Multilevel estimates of the Darcy pressure field.  Opt-in, on managers from pmc_mlmc_create only
 * (lanes and farms included): from now on every level pair the manager runs also accumulates, on the device, the sums of
 * d_l = p_l - p_{l+1}[parent] (d_{L-1} = p_{L-1}), d_l^2 and p_l^2 - p_{l+1}[parent]^2 (pmc_level_fields_*).  The scalar
 * sums and every statistic derived from them are unchanged.  Call before the first InitRun or after Reset, after the last
 * pmc_mlmc_add_lane; w0: the level-0 P0 mass, n_p(0) entries > 0 in `memspace`.  Refused (PMC_ERR_INVALID): a callbacks
 * manager, a manager that holds samples, a bad w0, a pressure prolongator that is not a 0/1 injection. */
int pmc_mlmc_enable_pressure_stats(pmc_mlmc* m, const double* w0, int memspace);
/* Level-0 maps, n_p(0) entries each in `memspace` (each may be NULL), with N_l = the manager's global level_nsamples[l]
 * and I_l the injection along the parent chain to level 0:
 *   mean               = sum_l I_l mean_l(d_l)
 *   second_moment      = sum_l I_l mean_l(p_l^2 - p_{l+1}^2)   (about zero: Var p = second_moment - mean^2, which is
 *                        returned neither centred nor clipped at 0)
 *   estimator_variance = sum_l I_l var_l(d_l) / N_l            (unbiased sample variance: the MSE map of mean)
 * and per level (nlevels entries in `memspace`, may be NULL) l2_mean_corr = ||mean_l(d_l)||_L2 and int_var_corr =
 * int var_l(d_l), with the weights (P chain)^T w0 - the field counterparts of eY / varY.  With nranks > 1 the raw sums are
 * reduced once through the farm's reduction: a collective every rank calls.  Refused (PMC_ERR_INVALID): not enabled, a
 * level whose accumulated count differs from level_nsamples (e.g. after pmc_mlmc_replay_log, whose log carries scalars
 * only), a level without realizations, estimator_variance or int_var_corr with some N_l < 2. */
int pmc_mlmc_pressure_stats(pmc_mlmc* m, double* mean, double* second_moment, double* estimator_variance,
                            double* l2_mean_corr, double* int_var_corr, int memspace);
/* the farm's one collective: wall milliseconds this rank has spent inside the SUM all-reduce of the accumulators (waiting
 * for the slowest rank included) and the number of reductions so far - one per InitRun round (the place the serial
 * reference would need it: src/MLMC_Manager.cpp:178, before computeNSamplesMSE) */
int pmc_mlmc_farm_times(pmc_mlmc* m, double* allreduce_ms, int64_t* reductions);
/* the table MLMC_Manager::ShowMe prints after every InitRun (src/MLMC_Manager.cpp:216-297), same labels / widths /
 * precision, into buf (NUL-terminated, truncated to cap); *needed (may be NULL) receives the full size incl. the NUL */
int pmc_mlmc_show_me(pmc_mlmc* m, char* buf, size_t cap, size_t* needed);
/* the per-level timers the reference keeps in parelag::TimeManager and prints at the end of a run (examples/MLMC.cpp:275):
 * "Sampler: Mult -- Level i" (src/PDESampler.cpp:328-333), "Darcy: Build Solver -- Level i", "Darcy: Mult -- Level i"
 * (src/DarcySolver.cpp:231-243) - device milliseconds (HIP events, pmc_stats.solve_ms / setup_ms) summed over the lanes of
 * this rank since the manager was created, as text (same calling convention as pmc_mlmc_show_me) and as numbers */
int pmc_mlmc_print_timers(pmc_mlmc* m, char* buf, size_t cap, size_t* needed);
int pmc_mlmc_phase_times(pmc_mlmc* m, int level, double* sampler_mult_ms, double* darcy_setup_ms, double* darcy_mult_ms,
                         int64_t* sampler_realizations, int64_t* darcy_realizations);
const char* pmc_host_last_error(void);

/* BayesianInverseProblem::ComputeLikelihood / ComputeLikelihoodAndQ / ComputeR (src/BayesianInverseProblem.cpp:188-218)
 * for nbatch realizations:  G = ComputeG(k) on the device (pmc_darcy_compute_G),
 *   likelihood = exp(-|G - G_obs|^2 / (2 noise)),   R = Q * likelihood.
 * likelihood, C: host arrays of nbatch; Q, R: host arrays or NULL. */
int pmc_bayes_likelihood(pmc_darcy* solver, int level, int nbatch, const double* k, int memspace, const double* G_obs,
                         int nobs, double noise, double* likelihood, double* C, double* Q, double* R);
/* BayesianInverseProblem::ComputeGradLogLikelihood (an extension: the reference has no gradients): loglik = log of the
 * likelihood above and its adjoint gradient with respect to k (wrt_log != 0: log k) for nbatch realizations, through
 * pmc_darcy_loglik_gradient.  loglik: host array of nbatch or NULL; grad: nbatch x n_p(level) in `memspace`, as k. */
int pmc_bayes_loglik_gradient(pmc_darcy* solver, int level, int nbatch, const double* k, int memspace, const double* G_obs,
                              int nobs, double noise, int wrt_log, double* loglik, double* grad);
/* BayesianInverseProblem::ComputeGradLogPosterior (an extension): for nbatch realizations of the
 * white noise xi (nbatch x xi_size(xi_level), xi_level <= level),
 *     logpost = loglik(k) - |xi|^2 / 2,  k = Eval(level, xi),      grad = dlogpost/dxi = -xi + (dk/dxi)^T dloglik/dk,
 * through pmc_sampler_eval, pmc_darcy_loglik_gradient (with respect to log k on a lognormal sampler) and
 * pmc_sampler_eval_adjoint.  logpost: host array of nbatch or NULL; grad: nbatch x xi_size(xi_level) in `memspace`, as xi.
 * With device memory only the scalars cross to the host.  ctx: the context both handles were created on. */
int pmc_bayes_logpost_gradient(pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver, int level, int xi_level, int nbatch,
                               const double* xi, int memspace, const double* G_obs, int nobs, double noise, double* logpost,
                               double* grad);
/* BayesianInverseProblem::ApplyGNHessian (an extension): the Gauss-Newton Hessian of -logpost at xi
 * applied to nbatch directions v (both nbatch x xi_size(xi_level)),
 *     hv = v + (dk/dxi)^T J^T (1/noise) J (dk/dxi) v,     J = dG/dk at k = Eval(level, xi),
 * symmetric positive definite and equal to the full Hessian where G(k) = data, through pmc_sampler_eval_tangent,
 * pmc_darcy_gn_hessvec (in log k on a lognormal sampler) and pmc_sampler_eval_adjoint; the prior's v is added on the device.
 * k_state (nbatch x n_p(level)) and x_state (nbatch x (n_u + n_p)) are caller-owned buffers in `memspace`, the linearization
 * state: have_state == 0: filled from xi (Eval, then the forward solve) and written; have_state != 0: read (xi is not, and
 * may be NULL), and the call costs two sampler solves and two Darcy solves - a CG loop at a fixed xi pays for the
 * linearization once.  The observed data do not enter.  xi, v, hv and the state share `memspace`. */
int pmc_bayes_logpost_gn_hessvec(pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver, int level, int xi_level, int nbatch,
                                 const double* xi, const double* v, int memspace, double noise, double* k_state,
                                 double* x_state, int have_state, double* hv);

/* BayesianInverseProblem::ComputeMAP (an extension): the maximiser of pmc_bayes_logpost_gradient's
 * logpost in the white noise, by inexact Gauss-Newton-CG, for nbatch independent columns that share the data G_obs.
 * Per outer iteration, all columns together: a column is converged once |g| <= max(grad_rtol |g0|, grad_atol) and is frozen
 * from then on (its xi keeps its bits, it enters later Hessian actions with a zero direction); CG on H_GN d = g from d = 0
 * through pmc_bayes_logpost_gn_hessvec and the pmc_ncg kernels of pmc.h, the linearization state computed by the first action
 * of the iteration, with the per-column forcing term eta = min(eta_max, sqrt(|g| / |g0|)), ended per column at
 * |r| <= eta |g|, after max_cg actions or on p.Hp <= 0 (possible through inexact solves only: the column keeps its d, or
 * takes d = g at its first step, and the event is counted); Armijo backtracking from t = 1 by halving, at most max_backtracks
 * halvings, accepting logpost(xi + t d) >= logpost(xi) + c1 t <g, d>, each trial one pmc_bayes_logpost_gradient of the whole
 * batch (accepted columns recompute their point, so the accepted gradient is the next iteration's).  A column whose
 * backtracks are exhausted stops at its last accepted xi.
 * grad_rtol's default belongs to the default solver options: under the 1e-6 MINRES rule gradients are accurate to about 1e-4
 * (DESIGN.md section 16), so a tighter gradient tolerance needs tighter solver options on both handles. */
typedef struct pmc_map_opts {
    int32_t max_newton;      /* outer iterations (default 50) */
    int32_t max_cg;          /* Hessian actions per outer iteration (default 100) */
    int32_t max_backtracks;  /* halvings of the step (default 10) */
    double eta_max;          /* cap of the forcing term, in (0, 1) (default 0.5) */
    double c1;               /* Armijo constant, in (0, 1) (default 1e-4) */
    double grad_atol;        /* >= 0 (default 0) */
    double grad_rtol;        /* > 0 (default 1e-4) */
} pmc_map_opts;
void pmc_map_opts_default(pmc_map_opts* o);
enum pmc_map_status {
    PMC_MAP_CONVERGED = 0,
    PMC_MAP_MAX_NEWTON = 1,
    PMC_MAP_LINE_SEARCH_FAILED = 2,
    PMC_MAP_NON_FINITE = 3   /* logpost or its gradient is not finite at the column's iterate */
};
/* Caller-owned HOST arrays; the per-column ones hold nbatch entries, the history ones (max_newton + 1) x nbatch, row i =
 * outer iterate i.  Every pointer may be NULL.  History rows a column never reached hold NaN / -1. */
typedef struct pmc_map_result {
    int32_t* status;                /* enum pmc_map_status */
    int32_t* newton_iterations;     /* accepted steps */
    int32_t* hessian_actions;       /* CG steps of the column over all iterations */
    int32_t* gradient_evaluations;  /* pmc_bayes_logpost_gradient calls while the column was running */
    int32_t* nonpos_curvature;      /* CG runs ended on p.Hp <= 0 */
    double* logpost0;
    double* logpost;
    double* grad_norm0;
    double* grad_norm;
    double* hist_logpost;           /* logpost at iterate i */
    double* hist_grad_norm;         /* |g| at iterate i */
    int32_t* hist_cg;               /* CG steps taken from iterate i (0: none, the column stopped there) */
    double* hist_t;                 /* step accepted from iterate i (0: none) */
} pmc_map_result;
/* xi_inout: nbatch x xi_size(xi_level) in `memspace`, the starting points on entry and the results on exit; with device
 * memory only scalars cross to the host.  opts NULL: the defaults.  Refused with PMC_ERR_INVALID: whatever
 * pmc_bayes_logpost_gradient refuses (a conditioned sampler handle among it), NULL xi_inout or res, max_newton / max_cg /
 * max_backtracks / grad_rtol <= 0, eta_max or c1 outside (0, 1), grad_atol < 0. */
int pmc_bayes_map(pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver, int level, int xi_level, int nbatch,
                  double* xi_inout, int memspace, const double* G_obs, int nobs, double noise, const pmc_map_opts* opts,
                  pmc_map_result* res);

/* ---- ML_BayesRatio_Manager / SL_BayesRatio_Manager (src/ML_BayesRatio_Manager.hpp:315-728, src/SL_BayesRatio_Manager.hpp)
 * Multilevel ratio estimator E[Q * likelihood] / E[likelihood]: per realization two INDEPENDENT prior draws, one for
 * Z = likelihood and one for R = Q * likelihood, each evaluated on level l and (same xi) on level l+1; the same
 * variance / bias / sample-allocation statistics as MLMC_Manager, computed for R and Z and combined by max.  nlevels == 1
 * is the single-level manager.  Sums use the reference's enum order (:66-69), 20 columns per level. */
#define PMC_RATIO_NVAR 20
typedef struct pmc_ratio pmc_ratio;
/* likelihood and R = Q*likelihood of nbatch realizations of k (host pointers) */
typedef int (*pmc_cb_likelihood)(void* user, int level, int nbatch, const double* k, double* likelihood, double* R,
                                 double* C);
typedef struct pmc_ratio_result {
    int32_t nlevels;
    double R_estimate, Z_estimate, ratio_estimate, eps2, actual_mse, estimator_variance, estimator_variance_R,
        estimator_variance_Z, bias2, bias2_R, bias2_Z, alpha_R, alpha_abs_R, beta_R, alpha_Z, alpha_abs_Z, beta_Z, gamma;
    const double *eR, *varR, *eYR, *varYR, *eABS_YR, *eZ, *varZ, *eYZ, *varYZ, *eABS_YZ, *eC, *cost;
    const double* sums;          /* nlevels x PMC_RATIO_NVAR */
    const int64_t *nsamples, *nsamples_missing;
    /* Ratio columns (q = r/z, y = q - q_c): what the *_Splitting managers estimate and allocate samples by */
    double alpha, alpha_abs, beta;
    const double *eRatio, *varRatio, *eYRatio, *varYRatio, *eABS_YRatio;
} pmc_ratio_result;
/* device version: prior = sampler, forward problem = solver with observation functionals set on every level */
int pmc_ratio_create(pmc_ctx* ctx, pmc_sampler* sampler, pmc_darcy* solver, int nlevels, const double* G_obs, int nobs,
                     double noise, const pmc_mlmc_params* params, pmc_ratio** out);
/* plugin version: cb->sample / cb->eval give the prior, `like` the likelihood and ratio integrand */
int pmc_ratio_create_callbacks(int nlevels, const pmc_plugin_callbacks* cb, pmc_cb_likelihood like,
                               const pmc_mlmc_params* params, pmc_ratio** out);
void pmc_ratio_destroy(pmc_ratio* m);
int pmc_ratio_set_farm(pmc_ratio* m, int nranks, int rank, pmc_reduce_fn reduce, void* user);
/* on != 0: ML_BayesRatio_Splitting_Manager / SL_BayesRatio_Splitting_Manager (src/ML_BayesRatio_Splitting_Manager.hpp:
 * 297-432 InitRun, :595-737 computeNSamplesMSE): estimate E[R/Z] by the level differences r/z - r_c/z_c; variance,
 * bias and sample allocation follow the Ratio columns; ratio_estimate = sum_l E[Y_Ratio,l] */
int pmc_ratio_set_splitting(pmc_ratio* m, int on);
int pmc_ratio_run(pmc_ratio* m);
int pmc_ratio_init_run(pmc_ratio* m, const int32_t* nsamples);
int pmc_ratio_result_get(pmc_ratio* m, pmc_ratio_result* out);
/* Posterior field estimates.  Opt-in, on managers from pmc_ratio_create only: from now on every
 * level also accumulates on the device (pmc_level_fields_accumulate_weighted, on ctx's stream - the one the sampler's Eval
 * writes on) the sums of d_l = w k_l - w_c k_{l+1}[parent], d_l^2 and w k_l^2 - w_c k_{l+1}[parent]^2, where k is the R-draw's
 * prior field (Eval's output on the Darcy level: n_p(l) entries) and w, w_c the likelihoods of its evaluations on l and l+1
 * (plain), or those divided by the Z-draw's likelihoods (splitting); w_c = 0 on the coarsest level.  parent() comes from the
 * Darcy handle's pressure prolongator, which must be a 0/1 injection.  The scalar sums are unchanged.  Call before the first
 * InitRun or after Reset; w0: the level-0 P0 mass, n_p(0) entries > 0 in `memspace`.  Refused (PMC_ERR_INVALID): a callbacks
 * manager, a manager that holds samples, a bad w0, a prior field that is not on the Darcy mesh, a prolongator that is not an
 * injection. */
int pmc_ratio_enable_field_stats(pmc_ratio* m, const double* w0, int memspace);
/* Level-0 maps, n_p(0) entries each in `memspace` (each may be NULL), with N_l = level_nsamples[l], I_l the injection along
 * the parent chain to level 0, Zhat = Z_estimate, V_Z = estimator_variance_Z and s = Zhat (plain) or 1 (splitting):
 *   mean               = sum_l I_l mean_l(d_l) / s                           the posterior mean of k
 *   second_moment      = sum_l I_l mean_l(w k^2 - w_c k_c^2) / s             about zero: Var_post k = second_moment - mean^2
 *   estimator_variance = (V_R + mean^2 V_Z) / Zhat^2 (plain), V_R (splitting), V_R = sum_l I_l var_l(d_l) / N_l
 * and per level (nlevels entries in `memspace`, may be NULL) l2_mean_corr = ||mean_l(d_l) / s||_L2 and int_var_corr =
 * int var_l(d_l) / (N_l s^2), with the weights (P chain)^T w0.  Outputs not requested are not computed.  The raw sums are
 * reduced once through the farm's reduction: a collective every rank calls.  Refused (PMC_ERR_INVALID): not enabled, a
 * level whose accumulated count differs from level_nsamples, a level without realizations, estimator_variance or
 * int_var_corr with some N_l < 2, sums accumulated in a mode other than the current one (pmc_ratio_set_splitting while
 * samples were held), a plain-mode read with Zhat 0 or not finite. */
int pmc_ratio_field_stats(pmc_ratio* m, double* mean, double* second_moment, double* estimator_variance,
                          double* l2_mean_corr, double* int_var_corr, int memspace);

/* ---- P0 x P0 mortar matrix between two NON-MATCHING meshes:  G[i,j] = | A_i  n  B_j |  (setup side, host only).
 * Replaces ParMortarAssembler::Assemble (src/transfer/ParMortarAssembler.cpp:1127-1144) as used for Gt by
 * L2ProjectionPDESampler::BuildHierarchy (src/L2ProjectionPDESampler.cpp:488-505) with A = original mesh, B = enlarged
 * mesh; the coarser levels follow by RAP(orig_Ps, Gt, Ps) (:512-513).  Elements: triangles / quadrilaterals (dim 2),
 * tetrahedra / hexahedra in MFEM vertex order (dim 3); they are split into simplices and intersected exactly. */
typedef struct pmc_mesh_view {
    int32_t dim, nverts, nelems, verts_per_elem;
    const double* verts;   /* nverts x dim, row-major         */
    const int32_t* elems;  /* nelems x verts_per_elem          */
} pmc_mesh_view;
typedef struct pmc_mortar pmc_mortar;
/* rel_tol: intersections below rel_tol * min(|A_i|, |B_j|) are dropped (<= 0: 1e-12) */
int pmc_mortar_assemble(const pmc_mesh_view* a, const pmc_mesh_view* b, double rel_tol, pmc_mortar** out);
int64_t pmc_mortar_nnz(const pmc_mortar* m);
/* copies the CSR arrays (rowptr: nelems_a + 1) and the element measures of both meshes; NULL pointers are skipped */
int pmc_mortar_get(const pmc_mortar* m, int32_t* rowptr, int32_t* colind, double* vals, double* measure_a,
                   double* measure_b);
void pmc_mortar_destroy(pmc_mortar* m);
const char* pmc_mortar_last_error(void);

/* expWRegression (src/Utilities.cpp:257-283), exported for the host-logic tests */
double pmc_exp_w_regression(const double* y, const double* x, int n, int skip_n_last);

#ifdef __cplusplus
}
#endif
#endif /* PMC_HOST_H_ */

/* pmc.h - C ABI of the MI355X-native ParELAGMC hot path (libpmc.so).
 *
 * Drop-in boundary for the per-realization work that ParELAGMC performs behind its two
 * plugin interfaces (all paths relative to /root/reference):
 *     MLSampler::Sample / Eval               src/MLSampler.hpp:33-52
 *     PhysicalMLSolver::SolveFwd             src/PhysicalMLSolver.hpp:33-47
 * as called, and only called, from MLMC_Manager::InitRun (src/MLMC_Manager.cpp:113-173) and
 * MC_Manager::InitRun (src/MC_Manager.cpp:82-116).
 *
 * Conventions
 *   - plain C types only: opaque handles, pointers + sizes, int32 indices, fp64 values;
 *   - every function returns PMC_OK (0) or a negative error code; no exception crosses the
 *     boundary; pmc_last_error() returns a thread-local message for the last failure;
 *   - operators are passed as host CSR arrays (exactly what ParELAG's SparseMatrix /
 *     HypreParMatrix diag blocks hold) and are copied/re-laid-out on the device at create
 *     time; callers keep ownership of everything they pass in;
 *   - level 0 is the FINEST level (ParELAG convention); P of level i maps level i+1 -> i;
 *   - vectors may live in host or device memory (`memspace`); batched vectors are
 *     sample-major: sample b occupies [b*n, (b+1)*n);
 *   - one handle per GPU; calls on one ctx are serialised by the caller (the reference's
 *     objects are not re-entrant either: src/DarcySolver.hpp:238).
 */
#ifndef PMC_H_
#define PMC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMC_OK 0
#define PMC_ERR_INVALID (-1)  /* bad argument (PARELAG_ASSERT / PARELAG_TEST_FOR_EXCEPTION sites) */
#define PMC_ERR_DEVICE (-2)   /* HIP runtime error, no GPU, out of memory */
#define PMC_ERR_COMM (-3)     /* RCCL failure */
#define PMC_ERR_INTERNAL (-4)

enum pmc_memspace { PMC_MEM_HOST = 0, PMC_MEM_DEVICE = 1 };
enum pmc_projection { PMC_PROJ_NONE = 0, PMC_PROJ_GATHER = 1, PMC_PROJ_L2 = 2 };
/* pmc_solver_opts.precond_storage: how data that lives INSIDE one application of the preconditioner z = B^-1 v is stored -
 * the preconditioned vectors z themselves, the V-cycle's iterates / residuals on a level, the per-realization values of the
 * Darcy Schur-complement hierarchy.  Operators, Lanczos vectors, products A z, directions, solution, every inner product and
 * ALL arithmetic are fp64 either way (the reference is fp64 end to end, src/PDESampler.cpp:279-333); with FP32 the solver is
 * MINRES with the fixed symmetric preconditioner fl32(B^-1 .), converges to the same solution at the same tolerance and
 * moves a quarter fewer bytes per iteration. */
enum pmc_storage { PMC_STORAGE_FP32 = 0, PMC_STORAGE_FP64 = 1 };

typedef struct pmc_ctx pmc_ctx;
typedef struct pmc_sampler pmc_sampler;
typedef struct pmc_darcy pmc_darcy;

/* CSR matrix, host pointers, sorted or unsorted column indices.  The entries of a row may come in any order (ascending,
 * the diagonal first, unordered) and may include stored zeros - an eliminated coupling left in the pattern, or an entry of
 * M_pattern with an empty contribution list.  A column may appear only ONCE in a row: every call that takes a pmc_csr
 * returns PMC_ERR_INVALID (-1) with a message naming the matrix and the row if one appears twice; sum duplicates first. */
typedef struct pmc_csr {
    int32_t nrows, ncols;
    const int32_t* rowptr; /* nrows+1 */
    const int32_t* colind; /* nnz */
    const double* vals;    /* nnz */
} pmc_csr;

/* Linear-solver options.  Defaults restate the reference's "MINRES-BJ-GS" entry
 * (examples/example_helpers/CreateSamplerParameterList.hpp:54-66): MINRES, 300 iterations,
 * rel 1e-6, abs 1e-12, block-diagonal preconditioner.  The two diagonal blocks are
 * GPU-native replacements inside the reference's own configuration space:
 * a fixed Chebyshev/l1-Jacobi polynomial on M (instead of 3 sequential l1-GS sweeps) and one
 * V-cycle over the caller's level hierarchy on S = aW + B diag(M)^-1 B^T (instead of
 * BoomerAMG), both fixed SPD linear operators as MINRES requires. */
typedef struct pmc_solver_opts {
    int32_t abi_version;      /* = PMC_ABI_VERSION; written by pmc_solver_opts_default, checked by the create functions: a caller
                                 compiled against another layout of this struct / pmc_stats is refused instead of misread   */
    int32_t max_iter;
    double rel_tol;
    double abs_tol;
    int32_t cheb_degree_M;    /* polynomial degree on the M block; 0 (default) = automatic: 2, or 4 on sampler levels whose
                                 measured Chebyshev interval exceeds 16 (badly shaped cells)                                */
    double cheb_ratio_M;      /* Chebyshev interval lambda_max/lambda_min of the l1-scaled M-block; <= 0 (default): measured at
                                 create time by a host Lanczos run on M (Darcy: on M(k == 1))                              */
    int32_t mg_smooth_degree; /* Chebyshev pre/post smoothing degree per level (default 2) */
    double mg_smooth_ratio;   /* smoothing interval [lmax/ratio, lmax] (default 8) */
    int32_t mg_coarse_degree; /* polynomial degree on the coarsest level (default 12) */
    double mg_coarse_ratio;   /* (default 100) */
    int32_t check_every;      /* iterations between host convergence polls (default 2) */
    int32_t use_graph;        /* replay pairs of MINRES iterations as one hipGraph (default 0; needs check_every 2) */
    double schur_scale;       /* gamma in S = aW + gamma * B diag(M)^-1 B^T (default 1): diag(M) under-/over-estimates M by
                                 the spectrum of diag(M)^-1 M, gamma recentres that interval                              */
    int32_t mg_coarsening;    /* hierarchy of the Schur-complement V-cycle: 0 = the caller's levels (P of the level structs),
                                 1 = smoothed aggregation built internally from S itself (what BoomerAMG does in the reference:
                                 strength-based, robust on stretched cells), 2 = choose 1 when the cells are strongly anisotropic
                                 (median strongest/weakest coupling per row > 10), else 0 (default 2)                       */
    int32_t mini_max_rows;    /* sampler levels of at most this many rows (n_u + n_s) whose Schur V-cycle fits the LDS tail are
                                 solved by ONE persistent workgroup per realization - the whole MINRES solve in a single
                                 kernel launch - instead of ~7 launches per iteration (default 6000; 0 = never)           */
    int32_t two_streams;      /* the two diagonal blocks of the preconditioner on two HIP streams of the handle: 0 = automatic
                                 (default: only when the handle is the only one on its device and the level has at least
                                 ~1.5 M rows x realizations; with several handles per GPU their kernels already fill the
                                 gaps), 1 = always, 2 = never.  Results do not depend on it.                                 */
    int32_t precond_storage;  /* enum pmc_storage (ABI 3): PMC_STORAGE_FP32 (default) or PMC_STORAGE_FP64 = everything fp64    */
} pmc_solver_opts;

/* Per-realization solver report; the reference returns -1 for iteration counts
 * (src/PDESampler.hpp:142-145, src/DarcySolver.hpp:104-107) and is silent on non-convergence. */
typedef struct pmc_stats {
    int32_t iterations;  /* iterations until THIS realization met the tolerance (the batch keeps iterating until its last one has) */
    int32_t converged;   /* 1 converged, 0 iteration cap reached, -1 breakdown (non-finite data / indefinite preconditioner) */
    double initial_norm; /* preconditioned residual norm before the first iteration */
    double final_norm;   /* |eta| at exit */
    /* Device time (HIP events on the handle's stream) of the launch group this realization was solved in, divided by the
     * realizations of that group, so that summing over realizations gives device milliseconds.  The reference's per-level
     * timers: solve_ms = "Sampler: Mult" (src/PDESampler.cpp:328-333) / "Darcy: Mult" (src/DarcySolver.cpp:231-236) - the
     * Krylov solve; setup_ms = what precedes it per realization: right-hand side and initial guess (sampler), M(k),
     * elimination and the Schur-complement hierarchy refresh = "Darcy: Build Solver" (src/DarcySolver.cpp:238-242). */
    double solve_ms;
    double setup_ms;
} pmc_stats;

/* One level of the SPDE sampler hierarchy = the blocks PDESampler::BuildHierarchy assembles
 * (src/PDESampler.cpp:232-284): A = [M B^T; B -alpha*W]. */
typedef struct pmc_sampler_level {
    int32_t n_u, n_s;
    pmc_csr M;            /* n_u x n_u, SPD, essential rows/cols -> identity (:236-241)     */
    pmc_csr B;            /* n_s x n_u, = W*D with essential columns zeroed (:243-246)       */
    const double* w_diag; /* n_s, diag(W) > 0; w_sqrt = sqrt(w_diag) (:248-254)              */
    pmc_csr P;            /* n_s(level) x n_s(level+1) = ComputeTrueP(sform) (:189-193);
                             ignored (may be zeroed) on the last level                        */
} pmc_sampler_level;

/* One level of the HYBRIDIZED sampler: the reference's alternative solver of the same system ("Hybridization" in the
 * sampler's parameter list, src/PDESampler.cpp:291,307-311,383-389; ParELAG's HybridHdivL2 does the element-local
 * elimination).  Eliminating (u, s) element by element from [M B^T; B -alpha*W][u; s] = [0; f] leaves one Lagrange
 * multiplier per face:   H lambda = G f,   s = z_diag .* f - G^T lambda   (exact, not an approximation). */
typedef struct pmc_hybrid_level {
    int32_t n_lambda, n_s;
    pmc_csr H;             /* n_lambda x n_lambda, SPD                                              */
    pmc_csr G;             /* n_lambda x n_s                                                        */
    const double* z_diag;  /* n_s, the (s, s) entry of the local inverses (negative)                */
    const double* w_diag;  /* n_s, diag(W) > 0 as in pmc_sampler_level                              */
    pmc_csr P;             /* n_s(level) x n_s(level+1) = ComputeTrueP(sform); ignored on the last  */
} pmc_hybrid_level;

/* What PDESampler::BuildHierarchy holds for one level BEFORE it eliminates boundary rows - the input of the element-local
 * elimination (pmc_hybrid_build).  The reference hands A[i] plus the level's de Rham sequence to
 * prec_factory->BuildSolver(A[i], state) (src/PDESampler.cpp:302-318; extra parameter "L2MassWeight" = alpha, :307-311) and
 * ParELAG's HybridHdivL2 reads the element matrices from the sequence; here they arrive as the same element decomposition of
 * the u-mass matrix that pmc_darcy_level carries for ComputeMassOperator(uform, k). */
typedef struct pmc_hybrid_elements {
    int32_t n_u, n_s;
    pmc_csr M_pattern;       /* n_u x n_u, sparsity of the u-mass matrix (vals ignored, may be NULL)                */
    const int32_t* c_ptr;    /* nnz(M)+1: contributions of stored entry p are c_ptr[p] .. c_ptr[p+1]                */
    const int32_t* c_elem;   /* element of each contribution                                                         */
    const double* c_val;     /* element-matrix value (global face orientation)                                       */
    pmc_csr B;               /* n_s x n_u as assembled, NO boundary elimination: row e lists every face of element e
                                with the sign of its outward normal against the face's global normal (:232-234)     */
    const double* w_diag;    /* n_s, diag(W) > 0                                                                     */
    pmc_csr P;               /* n_s(level) x n_s(level+1) = ComputeTrueP(sform); ignored (may be zeroed) on the last */
} pmc_hybrid_elements;
typedef struct pmc_hybrid_system pmc_hybrid_system;

/* One level of the Darcy hierarchy = what DarcySolver precomputes (src/DarcySolver.cpp:
 * 194-227 B/Bt/P, :297-319 obs, :360-384 ess_data, :386-414 rhs) plus the element
 * decomposition of the mass matrix that ComputeMassOperator(uform,k) re-assembles per sample
 * (:479):  M(k).vals[p] = sum_{t in c_ptr[p]..c_ptr[p+1]} coef(k[c_elem[t]]) * c_val[t]. */
typedef struct pmc_darcy_level {
    int32_t n_u, n_p;
    pmc_csr M_pattern;       /* n_u x n_u, sparsity of M(k) (vals ignored, may be NULL)       */
    const int32_t* c_ptr;    /* nnz(M)+1                                                      */
    const int32_t* c_elem;   /* element (entry of k) of each contribution                      */
    const double* c_val;     /* unit-coefficient element-matrix value                          */
    pmc_csr B;               /* n_p x n_u, no boundary elimination (:203-207)                 */
    const double* rhs;       /* n_u+n_p                                                       */
    const uint8_t* ess_mask; /* n_u, 1 = essential u-dof (:487-492)                           */
    const double* ess_data;  /* n_u, essential values (only read where ess_mask)              */
    const double* obs;       /* n_u+n_p, observation functional (:297-319)                    */
    pmc_csr P;               /* n_p(level) x n_p(level+1), P0 prolongator; ignored on last    */
} pmc_darcy_level;

/* ---- library / context ---------------------------------------------------------------- */
int pmc_version(void);
#define PMC_ABI_VERSION 3 /* layout of pmc_solver_opts / pmc_stats; 2: abi_version field, solve_ms / setup_ms; 3: precond_storage */
int pmc_abi_version(void); /* the library's PMC_ABI_VERSION */
/* bytes per entry of the PRECONDITIONED Krylov vectors inside the MINRES solves of a handle (4: PMC_STORAGE_FP32, 8:
 * PMC_STORAGE_FP64; pmc_krylov_z_bytes: of the default options).  The byte counts pmc_sampler_apply_operator reports are for
 * fp64 input; the launches inside the solver loop read their input vector at this width. */
int pmc_krylov_z_bytes(void);
int pmc_sampler_krylov_z_bytes(const pmc_sampler* s);
int pmc_darcy_krylov_z_bytes(const pmc_darcy* d);
/* kernels launched by this process through the library so far (all handles, all host threads): launch-rate diagnostics */
uint64_t pmc_kernel_launches(void);
/* MINRES solves of this process that ran the operator twice per iteration and never stored q = A u (the hybridized multiplier
 * solve in its eager loop; DESIGN.md section 3, paragraph "The multiplier solve without q"): path diagnostics, as
 * pmc_kernel_launches */
uint64_t pmc_fused_lanczos_solves(void);
/* ... whose right-hand side was written by its producer straight into the first Lanczos vector and its fp32 copy (the
 * hybridized sampler's G product from a zero guess), and batch evaluations of the hybridized sampler whose back-substitution
 * wrote the field sample-major itself (identity output map, no embedded copy, no conditioner): path diagnostics */
uint64_t pmc_adopted_rhs_solves(void);
uint64_t pmc_fused_field_evals(void);
/* MINRES solves of this process by the loop that ran them (all handles, all host threads): path diagnostics.  A solve counts
 * once, for the first of these that applies: the persistent one-workgroup kernel of small sampler levels (mini_max_rows); pairs
 * of iterations replayed as a captured graph (use_graph with check_every 2); the two-stream schedule with the w / x update one
 * iteration late; the eager loop that updates the rows of a compact index list once per iteration (the Darcy solves); the
 * eager loop that applies the w / x updates of a whole window of iterations in one pass; the eager loop with one plain update
 * per iteration (laboratory builds with the window switched off only).  The path is counted when the solve SELECTS its loop: a
 * solve on PMC_PATH_GRAPH that ends within its first, eager pair of iterations (or whose max_iter is 1: only the eager tail
 * runs) never replays a graph.  Two further values count events, not solves: PMC_COUNT_GRAPH_REPLAYS the graph launches, and
 * PMC_COUNT_POLLS the convergence polls (device-to-host reads of the active-column count) of all solves - a solve that starts
 * polling late, at the iteration count its predecessor on the handle needed, shows fewer.  Six more count launches that took a
 * size-gated form, bumped on the host next to the launch (under graph capture: the capture, not its replays), so that a test can
 * tell that its shape reached the gate: PMC_COUNT_NT_OPERATOR block-operator products with non-temporal matrix / result streams;
 * PMC_COUNT_NT_POLY one-pass polynomial (smoother) launches with them; PMC_COUNT_NT_FLAT flat vector kernels (lincomb3, the w / x
 * updates, the Darcy element-gather operator and polynomial) with them; PMC_COUNT_BOUNDED_GRID fused-dot launches whose grid the
 * workgroup bound actually cut (their workgroups loop); PMC_COUNT_TWO_STAGE_DOT block-operator products whose partial blocks
 * were folded by a second kernel; PMC_COUNT_TRACER_SPLIT tracer walks or flux uploads issued in more than one piece.  Another
 * value returns 0. */
enum pmc_solve_path {
    PMC_PATH_MINI = 0,
    PMC_PATH_GRAPH = 1,
    PMC_PATH_LATE = 2,
    PMC_PATH_INDEXED = 3,
    PMC_PATH_WINDOW = 4,
    PMC_PATH_PLAIN = 5,
    PMC_COUNT_GRAPH_REPLAYS = 6,
    PMC_COUNT_POLLS = 7,
    PMC_COUNT_NT_OPERATOR = 8,
    PMC_COUNT_NT_POLY = 9,
    PMC_COUNT_NT_FLAT = 10,
    PMC_COUNT_BOUNDED_GRID = 11,
    PMC_COUNT_TWO_STAGE_DOT = 12,
    PMC_COUNT_TRACER_SPLIT = 13
};
uint64_t pmc_solve_path_count(int path);
const char* pmc_last_error(void);
void pmc_solver_opts_default(pmc_solver_opts* opts);

/* pmc_ctx_create_abi refuses a caller compiled against another PMC_ABI_VERSION (another layout of pmc_solver_opts /
 * pmc_stats) before any handle exists - also callers that pass opts == NULL (defaults) and a pmc_stats array later.  C and
 * C++ callers get it through the macro below; binders that cannot use macros (ctypes, cgo) call it directly.  The plain
 * pmc_ctx_create symbol stays exported and performs no such check: the create functions then check pmc_solver_opts only. */
int pmc_ctx_create(int device_id, pmc_ctx** out);
int pmc_ctx_create_abi(int device_id, int abi_version, pmc_ctx** out);
#ifndef PMC_NO_ABI_CHECK_MACRO
#define pmc_ctx_create(device_id, out) pmc_ctx_create_abi((device_id), PMC_ABI_VERSION, (out))
#endif
void pmc_ctx_destroy(pmc_ctx* ctx);
int pmc_ctx_synchronize(pmc_ctx* ctx);
/* hipStream_t all work of this ctx is enqueued on (for callers that record their own events) */
void* pmc_ctx_stream(pmc_ctx* ctx);
/* the device the ctx was created on (-1 for NULL) */
int pmc_ctx_device(const pmc_ctx* ctx);
/* elapsed device milliseconds between two points on the ctx stream (HIP events) */
int pmc_timer_start(pmc_ctx* ctx);
int pmc_timer_stop(pmc_ctx* ctx, double* ms);

/* device memory helpers so non-HIP callers can keep xi / s / k resident in HBM */
int pmc_malloc(pmc_ctx* ctx, size_t bytes, void** dptr);
int pmc_free(pmc_ctx* ctx, void* dptr);
int pmc_memcpy_h2d(pmc_ctx* ctx, void* dst, const void* src, size_t bytes);
int pmc_memcpy_d2h(pmc_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- NormalDistributionSampler (src/NormalDistributionSampler.cpp:17-37) ---------------- */
/* Seed the counter-based generator.  (nparts, mypart) restate NormalDistributionSampler::Split
 * (src/NormalDistributionSampler.cpp:21-24, a leap-frog of the stream): part `mypart` owns the generator's
 * realizations mypart, mypart + nparts, ...; the ids handed to pmc_*_sample / pmc_normal_fill are LOCAL to the part
 * (local id i = generator realization i * nparts + mypart), so parts with the same seed and different mypart never
 * share a realization, and the union over the parts is exactly the unsplit stream.  (1, 0) = no split. */
int pmc_rng_seed(pmc_ctx* ctx, uint64_t seed, int nparts, int mypart);
/* out[b*n + i] = mean + sqrt(sigma2) * Phi^-1(u),  b < nbatch, realization id first_id+b */
int pmc_normal_fill(pmc_ctx* ctx, double mean, double sigma2, uint64_t first_sample_id, uint32_t stream,
                    int nbatch, int n, double* out, int memspace);

/* ---- PDESampler / EmbeddedPDESampler / L2ProjectionPDESampler -------------------------- */
/* nlevels >= n_mc_levels >= 1: levels [n_mc_levels, nlevels) are never sampled on, they only
 * deepen the V-cycle of the Schur-complement preconditioner. */
int pmc_sampler_create(pmc_ctx* ctx, int nlevels, int n_mc_levels, const pmc_sampler_level* levels,
                       double alpha, double matern_g, int lognormal, const pmc_solver_opts* opts,
                       pmc_sampler** out);
/* The same sampler with the hybridized solver (pmc_hybrid_level): MINRES on H with one V-cycle of an internal aggregation
 * multigrid as preconditioner.  Every level is a Monte Carlo level.  The handle behaves like any other pmc_sampler
 * (Sample / Eval / projections / batch width); init_s / use_init are accepted and ignored (the multiplier has no
 * counterpart of a coarse field), pmc_sampler_mult / _apply_preconditioner / _apply_operator act on multiplier vectors
 * of n_lambda entries, pmc_sampler_nnz reports nnz(H).  Of pmc_solver_opts the Krylov fields, precond_storage,
 * mg_smooth_degree / mg_coarse_* apply; the smoothing interval of the aggregation hierarchy is [lmax / (2 mg_smooth_ratio),
 * lmax] (default 16); cheb_*_M, schur_scale, mg_coarsening and mini_max_rows have no role. */
int pmc_sampler_create_hybrid(pmc_ctx* ctx, int nlevels, const pmc_hybrid_level* levels, double alpha, double matern_g,
                              int lognormal, const pmc_solver_opts* opts, pmc_sampler** out);
int pmc_sampler_is_hybrid(const pmc_sampler* s);
/* The element-local elimination itself (host code, setup): one dense (n_fe + 1)^2 inverse per element,
 * [[X, y], [y^T, z]]_e = [[M_e, b_e^T], [b_e, -alpha w_e]]^-1, H = sum_e C_e X_e C_e^T, G = sum_e C_e y_e, C_e = sign(B[e, f]).
 * pmc_hybrid_system_level fills `view` with pointers into the system (valid until pmc_hybrid_system_destroy) - the arrays
 * pmc_sampler_create_hybrid takes.  pmc_sampler_create_hybrid_from_elements = build every level, create, destroy: the one call
 * that stands where the reference's `if (if_solver_hybridization)` branch builds its solver (src/PDESampler.cpp:302-318). */
int pmc_hybrid_build(const pmc_hybrid_elements* level, double alpha, pmc_hybrid_system** out);
int pmc_hybrid_system_level(const pmc_hybrid_system* sys, pmc_hybrid_level* view);
void pmc_hybrid_system_destroy(pmc_hybrid_system* sys);
int pmc_sampler_create_hybrid_from_elements(pmc_ctx* ctx, int nlevels, const pmc_hybrid_elements* levels, double alpha,
                                            double matern_g, int lognormal, const pmc_solver_opts* opts, pmc_sampler** out);
/* ---- KLSampler (src/KLSampler.cpp:144-223) ------------------------------------------------ */
/* One level of the truncated Karhunen-Loeve sampler: the P0 space of the level, its mass diagonal and the prolongator to the
 * next coarser level (ParELAG's L2 projector onto the coarser P0 space is D^-1 P^T W with D = P^T W P, which must be
 * diagonal: every fine element in at most one agglomerate). */
typedef struct pmc_kl_level {
    int32_t n_s;          /* elements of the level                                               */
    const double* w_diag; /* n_s, diag(W) > 0 (P0 mass)                                          */
    pmc_csr P;            /* n_s(level) x n_s(level+1); ignored (may be zeroed) on the last level */
} pmc_kl_level;
/* KLSampler over what CovarianceFunction::Eigenvalues() / Eigenvectors() hold after SolveEigenvalue() (the caller runs its
 * own eigensolver on the host, as the reference does, or pmc_kl_matern_eigs below): evals (nmodes, each finite and >= 0) and evect0 (n_s(0) x nmodes,
 * column-major = mfem::DenseMatrix::Data()).  The handle projects Phi to the coarser levels itself at create,
 * Phi_{l+1} = D^-1 P^T W_l Phi_l, without renormalising the coarse columns (KLSampler::BuildHierarchy).  Every level is a
 * Monte Carlo level.  nmodes > n_s of a level is refused: the reference reads past xi there (Sample draws n_s normals,
 * Eval reads the first nmodes of them).
 * pmc_sampler_sample / _xi_size (= n_s) / _sample_size / _nnz (0) / _true_p / _batch_width / _num_levels and the managers
 * take the handle like any other.  pmc_sampler_eval computes s = Phi_level Lambda^1/2 xi[:nmodes] (exp() if lognormal) for
 * every realization in one fp64 launch, whichever level xi was drawn on; embed_s_out receives the Gaussian field;
 * init_s / init_level / use_init are ignored; pmc_stats: iterations 0, converged 1.  pmc_sampler_mult, _apply_preconditioner,
 * _apply_operator, _vcycle_info, _vcycle_level, _vcycle_prolongator and _set_projection return PMC_ERR_INVALID on a KL
 * handle. */
int pmc_sampler_create_kl(pmc_ctx* ctx, int nlevels, const pmc_kl_level* levels, int nmodes, const double* evals,
                          const double* evect0, int lognormal, pmc_sampler** out);
int pmc_sampler_is_kl(const pmc_sampler* s);
/* ---- MaternCovariance::SolveEigenvalue on the device (src/MaternCovariance.cpp:357-420) -------------------------- */
/* The top m = min(nmodes, n) eigenpairs of A v = lambda W v, A = W C W, W = diag(w_diag), C_ij = c(|x_i - x_j|) at the element
 * centres, c(r) = exp(-r / corlen) (the 3D Matern kernel with nu = 1/2; c = 1 where r / corlen < 1e-10), without ever
 * storing C: with y = W^1/2 v the problem is K y = lambda y, K = W^1/2 C W^1/2, and every product with K evaluates its entries
 * on the fly (fp64 MFMA; O(n (m + guard)) memory).  Chebyshev-filtered subspace iteration on a block of m + guard columns
 * (at most 512), filter degree `degree` on [0, smallest Ritz value], Rayleigh-Ritz after every filter; it stops when
 * max_k ||K y_k - theta_k y_k||_2 <= tol theta_1 over the m wanted columns, or after max_iter filters.  The start block comes
 * from the library's Philox generator with `seed`: the same seed, device and options give bitwise the same output.
 * Output as pmc_sampler_create_kl takes it: evals ascending (m), evect0 n x m column-major with V^T W V = I, the entry of
 * largest magnitude of every column (the first one on ties) positive.
 * Not converged after max_iter is NOT an error: the call returns PMC_OK with the best pairs, info.converged = 0 and the
 * residual reached, so pass `info` and read it.  gap_rel = (lambda_m - lambda_{m+1}) / lambda_1 from the guard Ritz values
 * (0 when guard = 0 or m = n): near zero means the truncation cuts through a cluster and the last modes are an arbitrary
 * rotation inside it.
 * PMC_ERR_INVALID: dim != 3 (the 2D kernel needs the Bessel function K1; 2D meshes fit a dense host solve), w_diag not
 * positive, coordinates not finite, corlen <= 0, nmodes < 1, m + guard > 512, a NULL pointer. */
typedef struct pmc_kl_eigs_opts {
    double tol;       /* 1e-8                                                        */
    int32_t max_iter; /* 100 filter applications                                     */
    int32_t guard;    /* 16 extra columns of the block                               */
    int32_t degree;   /* 8, degree of the Chebyshev filter; keep it modest           */
    uint64_t seed;    /* 0, seed of the start block                                  */
} pmc_kl_eigs_opts;
typedef struct pmc_kl_eigs_info {
    int32_t iterations;      /* filters applied                                      */
    int32_t block_products;  /* products of K with the whole block                   */
    int32_t converged;       /* 1: the stop rule was met                             */
    double max_residual_rel; /* max_k ||K y_k - theta_k y_k||_2 / theta_1, k < m      */
    double gap_rel;          /* (lambda_m - lambda_{m+1}) / lambda_1                 */
    double seconds;          /* wall time of the call                                */
} pmc_kl_eigs_info;
void pmc_kl_eigs_opts_default(pmc_kl_eigs_opts* opts);
/* Y = K X: X and Y n x ncols column-major HOST arrays, centroids n x dim row-major, 1 <= ncols <= 512 (tests, benchmarks) */
int pmc_kl_matern_apply(pmc_ctx* ctx, int dim, int n, const double* centroids, const double* w_diag, double corlen,
                        int ncols, const double* X, double* Y);
int pmc_kl_matern_eigs(pmc_ctx* ctx, int dim, int n, const double* centroids, const double* w_diag, double corlen,
                       int nmodes, const pmc_kl_eigs_opts* opts /* NULL = defaults */, double* evals /* m */,
                       double* evect0 /* n x m */, pmc_kl_eigs_info* info /* may be NULL */);
void pmc_sampler_destroy(pmc_sampler* s);
/* Output map of the embedded variants.  PMC_PROJ_GATHER: s = sbar[gather_idx]
 * (src/EmbeddedPDESampler.cpp:552-556); PMC_PROJ_L2: s = inv_w_orig .* (Gt sbar)
 * (src/L2ProjectionPDESampler.cpp:738-750). */
int pmc_sampler_set_projection(pmc_sampler* s, int level, int kind, const pmc_csr* Gt,
                               const int32_t* gather_idx, const double* inv_w_orig, int orig_size);
int pmc_sampler_num_levels(const pmc_sampler* s);
int pmc_sampler_xi_size(const pmc_sampler* s, int level);     /* size Sample() fills            */
int pmc_sampler_sample_size(const pmc_sampler* s, int level); /* SampleSize(): size of Eval's s */
int64_t pmc_sampler_nnz(const pmc_sampler* s, int level);     /* GetNNZ()                       */
/* Realizations of `level` ONE launch of the solver kernels carries (16 on large levels, 32 on small ones, 64 / 128 / 256 -
 * column groups of 32 - on the smallest): pmc_sampler_eval cuts any nbatch into chunks of this width, so callers that
 * can choose (the managers' realizations per plugin call) should hand over multiples of it. */
int pmc_sampler_batch_width(const pmc_sampler* s, int level);
/* GetTrueP(level) (src/MLSampler.hpp:85-87, src/PDESampler.hpp:153-156): the prolongator of the s-space from level+1 to
 * level as handed over at create time; the pointers stay valid for the life of the handle.  Error on the last level. */
int pmc_sampler_true_p(const pmc_sampler* s, int level, pmc_csr* out);
/* Sample(level, xi): xi ~ N(0, 1) of pmc_sampler_xi_size(level) entries per realization */
int pmc_sampler_sample(pmc_sampler* s, int level, uint64_t first_sample_id, int nbatch, double* xi,
                       int memspace);
/* Eval(level, xi, s, embed_s, use_init) (src/PDESampler.cpp:411-535).
 *   xi_level <= level : level xi was drawn on (the reference infers it from xi.Size(), :419)
 *   s                 : out, nbatch x sample_size(level); exp() applied if lognormal
 *   init_s/init_level : in, Gaussian field on a coarser-or-equal level used as the initial
 *                       guess when use_init != 0 (:498-510); ignored otherwise (may be NULL)
 *   embed_s_out       : out (may be NULL), Gaussian field on the sampler mesh at `level`
 *                       (:527); may alias init_s
 *   stats             : out (may be NULL), nbatch entries */
int pmc_sampler_eval(pmc_sampler* s, int level, int xi_level, int nbatch, const double* xi, double* s_out,
                     const double* init_s, int init_level, int use_init, double* embed_s_out, int memspace,
                     pmc_stats* stats);
/* The adjoint (transpose of the derivative) of Eval in the white noise (an extension of this project):
 * for J a function of Eval's output s_out and v = dJ/ds_out,
 *     grad_xi = (d s_out / d xi)^T v = dJ/dxi,
 * per realization, sample-major like Eval and cut into the same launch widths.  SPDE handles (saddle-point and hybridized,
 * every output map of pmc_sampler_set_projection): the level's own solve from a zero guess with O^T (v o f') in the s-rows
 * of the right-hand side, prolongated from `level` to xi_level and scaled by -g w_sqrt[xi_level]; stats (may be NULL)
 * reports that solve.  KL handles: grad_xi[:nmodes] = (Phi_level Lambda^1/2)^T (v o f'), the other xi_size(xi_level) - nmodes
 * entries 0; calls of more than 4 realizations run the fp64 MFMA kernel, narrower ones a VALU kernel (a column's bits may
 * differ between the two); within either, a column's bits do not depend on nbatch or on how a call was split.
 *   v       : in, nbatch x sample_size(level)
 *   s_out   : in, NULL or Eval's output for the same xi: v is multiplied by it (f' of the exp() of a lognormal handle).
 *             NULL for callers that hold dJ/dlog s_out already (wrt_log of the Darcy gradients) and on Gaussian handles
 *   grad_xi : out, nbatch x xi_size(xi_level)
 * Conditioned handles: with a conditioner attached that has pmc_conditioner_enable_derivatives on, the
 * entry differentiates the CONDITIONAL field: per launch, w = pmc_conditioner_apply_adjoint(v, s_out) in a buffer of the
 * conditioner, then the path above with v := w, s_out := NULL (the same solve, reported in stats as before; s_out is the
 * conditional field Eval returned).  For nbatch <= pmc_sampler_batch_width(level) the result is bit for bit the composition
 * of the public pieces: detach, w = pmc_conditioner_apply_adjoint(v, s_out) at the same nbatch, pmc_sampler_eval_adjoint(w,
 * NULL).
 * PMC_ERR_INVALID: level outside [0, number of Monte Carlo levels), xi_level outside [0, level], nbatch < 1, NULL v or
 * grad_xi, s_out != NULL on a handle that is not lognormal, a handle with a conditioner attached that has not been opted in
 * with pmc_conditioner_enable_derivatives. */
int pmc_sampler_eval_adjoint(pmc_sampler* s, int level, int xi_level, int nbatch, const double* v, const double* s_out,
                             double* grad_xi, int memspace, pmc_stats* stats);
/* Tangent of Eval (an extension): ds_out = (d Eval(level, xi_level) / d xi) v = f' o (L v), with L the
 * linear part of Eval - Eval of v without the exp() of a lognormal handle, through the same output map, the same solve from a
 * zero guess and the same launch widths, on every handle kind Eval serves (saddle-point, hybridized, KL; identity, gather and
 * L2 output maps).  <ds_out, u> = <v, pmc_sampler_eval_adjoint(u)> with the same s_out.
 *   v       : in, nbatch x xi_size(xi_level)
 *   s_out   : in, NULL or Eval's output for the xi of the linearization: L v is multiplied by it (f' of the exp()).  NULL
 *             for callers that want the direction in log s_out (wrt_log of the Darcy entries) and on Gaussian handles,
 *             where the result is Eval of v bit for bit
 *   ds_out  : out, nbatch x sample_size(level)
 * Conditioned handles, with pmc_conditioner_enable_derivatives on: Eval's linear part of v, then per
 * launch the homogeneous conditioning update dg - K A^-1 H dg (y = 0, no exp), then o s_out.  For nbatch <=
 * pmc_sampler_batch_width(level) bit for bit the composition: detach, pmc_sampler_eval_tangent(v, NULL),
 * pmc_conditioner_apply_tangent(., s_out) at the same nbatch.
 * PMC_ERR_INVALID: as pmc_sampler_eval_adjoint (NULL v or ds_out, s_out on a handle that is not lognormal, a conditioner
 * without pmc_conditioner_enable_derivatives). */
int pmc_sampler_eval_tangent(pmc_sampler* s, int level, int xi_level, int nbatch, const double* v, const double* s_out,
                             double* ds_out, int memspace, pmc_stats* stats);
/* 1 if Eval applies exp() (the lognormal flag of the create call), 0 if not */
int pmc_sampler_is_lognormal(const pmc_sampler* s);
/* The prior's part of a log-posterior gradient in the white noise xi ~ N(0, I), on the handle's stream:
 *     grad -= xi (in place; xi, grad: nbatch x n in `memspace`),     logprior[b] = -|xi_b|^2 / 2 (host array, may be NULL).
 * The sum has a fixed order: a realization's value does not depend on how its call was split.  PMC_ERR_INVALID: n < 1,
 * nbatch < 1, NULL xi or grad. */
int pmc_sampler_logprior_gradient(pmc_sampler* s, int n, int nbatch, const double* xi, double* grad, double* logprior,
                                  int memspace);
/* The prior's part of a Hessian action of -log pi in the white noise xi ~ N(0, I), on the handle's stream: hv += v (in
 * place; v, hv: nbatch x n in `memspace`).  PMC_ERR_INVALID: n < 1, nbatch < 1, NULL v or hv. */
int pmc_sampler_logprior_hessvec(pmc_sampler* s, int n, int nbatch, const double* v, double* hv, int memspace);

/* ---- Field statistics and errors of the sampler drivers (examples/PDESamplerTest.cpp:205-274) ---------------------- */
/* Accumulators of ONE level's Eval output s (pmc_sampler_sample_size(level) entries per realization) on the device:
 * per element the sums of s, s^2 and <chi, s> s as (sum, compensation) pairs (Neumaier), added in ascending sample id.
 * The result is bit-identical however the N realizations were split into calls and launches.
 * chi (may be NULL: no chi_cov): sample_size(level) entries in `memspace`, already on `level` (the drivers restrict the
 * level-0 indicator by P^T level by level); <chi, s> is the plain Euclidean dot of the drivers (no mass weighting). */
typedef struct pmc_field_stats pmc_field_stats;
int pmc_field_stats_create(pmc_sampler* s, int level, const double* chi, int memspace, pmc_field_stats** out);
void pmc_field_stats_destroy(pmc_field_stats* fs);   /* before the sampler it was created on */
int pmc_field_stats_reset(pmc_field_stats* fs);
/* add nbatch realizations the caller holds (sample-major, as pmc_sampler_eval writes them) */
int pmc_field_stats_accumulate(pmc_field_stats* fs, int nbatch, const double* s, int memspace);
/* the drivers' loop on the device: Sample(level) + Eval(level) of the ids first_sample_id .. first_sample_id + nsamples - 1,
 * each launch accumulated in place; nothing crosses to the host.  Launches cover the fixed id ranges
 * [t W, (t + 1) W), W = pmc_sampler_batch_width(level), so that every realization is evaluated beside the same others
 * whatever the split into calls; a range that does not start and end on multiples of W evaluates the whole launches at its
 * ends and accumulates only its own ids. */
int pmc_field_stats_run(pmc_field_stats* fs, uint64_t first_sample_id, int64_t nsamples);
/* expectation = (1/N) sum s, second_moment = (1/N) sum s^2, chi_cov = (1/N) sum <chi, s> s, count = N; any pointer may be
 * NULL.  second_moment is what the drivers call the "marginal variance": the moment about ZERO, not about the mean
 * (PDESamplerTest.cpp:240,251; compared with exp(s2) (exp(s2) - 1) for a lognormal field).  Centre it yourself:
 * Var = second_moment - expectation^2.  chi_cov from accumulators created without chi, and N = 0, are refused. */
int pmc_field_stats_read(const pmc_field_stats* fs, double* expectation, double* second_moment, double* chi_cov,
                         int64_t* count, int memspace);
/* the raw accumulators, (4 or 6) x sample_size(level) doubles: [sum s | comp | sum s^2 | comp | sum <chi,s> s | comp]
 * (the last two only with chi); sum + comp is the compensated sum.  Readable so that ranks can combine them. */
int pmc_field_stats_read_sums(const pmc_field_stats* fs, double* sums, int64_t* count, int memspace);
/* <chi, s_c> of nbatch realizations exactly as accumulate forms them (a fixed reduction tree: the same bits for a column
 * alone or inside any launch) */
int pmc_field_stats_chi_dot(const pmc_field_stats* fs, int nbatch, const double* s, double* dots, int memspace);
/* MLSampler::ComputeL2Error / ComputeMaxError for nbatch fields of sample_size(level) entries at once (coeff, err in
 * `memspace`).  l2: err[c] = || P_0 .. P_{level-1} coeff_c - exact ||^2_L2 with the level-0 P0 mass (the squared error,
 * as the reference returns; src/PDESampler.cpp:613-623).  max: err[c] = max(max coeff_c - exact, exact - min coeff_c)
 * (:625-633) on the level itself.  EmbeddedPDESampler's abs() in EmbedComputeMaxError changes nothing: the two terms sum
 * to max - min >= 0.  The output of an embedded / L2-projected level lives on the ORIGINAL mesh: both calls are refused
 * there until pmc_sampler_set_output_hierarchy has handed over that mesh's hierarchy. */
int pmc_sampler_l2_error(pmc_sampler* s, int level, int nbatch, const double* coeff, double exact, double* err,
                         int memspace);
int pmc_sampler_max_error(pmc_sampler* s, int level, int nbatch, const double* coeff, double exact, double* err,
                          int memspace);
/* the original mesh's P0 hierarchy behind the output of the projected variants: P_orig[l] (l < nlevels - 1) maps
 * sample_size(l + 1) -> sample_size(l) in the output numbering, w0_orig the P0 mass diagonal of its level 0
 * (sample_size(0) entries, > 0).  Copied; nlevels in [1, number of Monte Carlo levels]. */
int pmc_sampler_set_output_hierarchy(pmc_sampler* s, int nlevels, const pmc_csr* P_orig, const double* w0_orig);

/* ---- Conditioning on observed field values (an extension of this project; nothing in the reference
 *      does this) ---------------------------------------------------------------------------------------------------------- */
/* Kriging / Matheron's rule for LINEAR observations of the Gaussian field: with C_l the covariance of the Gaussian field Eval
 * produces on level l, H_l the observation operator (H_{l+1} = H_l P_l) and R = diag(sigma2),
 *     g_c = g + K_l A_l^-1 (y + R^1/2 zeta - H_l g),   K_l = C_l H_l^T,   A_l = 1/2 (H_l K_l + (H_l K_l)^T) + R,
 * is a draw of the field conditioned on the data whenever g is a prior draw and zeta ~ N(0, I) is independent of it.
 * pmc_conditioner_create does everything expensive once per handle and Monte Carlo level: K_l by two applications of the
 * handle's own Eval per observation (a KL handle: from its device modes), A_l^-1 by a host Cholesky.  H0: nobs x n_s(0), point
 * values or averages, every row non-empty; y: nobs values; sigma2: nobs values >= 0, NULL = exact data.
 * PMC_ERR_INVALID: a handle with a projection set (pmc_sampler_set_projection), nobs < 1 or nobs > 512, an empty row or a
 * wrong column count of H0, a non-finite y / sigma2 / entry of H0, a negative sigma2, an A_l that is not positive definite (a
 * Cholesky pivot below 1e-12 of its diagonal entry; with exact data: two observations inside one element of a coarse level -
 * the message names the level). */
typedef struct pmc_conditioner pmc_conditioner;
int pmc_conditioner_create(pmc_sampler* s, int nobs, const pmc_csr* H0, const double* y,
                           const double* sigma2 /* NULL = exact */, pmc_conditioner** out);
void pmc_conditioner_destroy(pmc_conditioner* c);   /* before the sampler it was created on; detaches itself */
int pmc_conditioner_num_obs(const pmc_conditioner* c);
/* Setup export (tests): *n = n_s(level), *nnz = entries of H_level; K: n x nobs column-major; A: nobs x nobs as inverted;
 * rowptr (nobs + 1) / colind (nnz) / vals (nnz): H_level in CSR, columns ascending.  Every pointer may be NULL: call once for
 * the sizes, then with arrays.  Host arrays. */
int pmc_conditioner_level(const pmc_conditioner* c, int level, int* n, int64_t* nnz, double* K, double* A, int32_t* rowptr,
                          int32_t* colind, double* vals);
/* out = f(g + K_l A_l^-1 (y + sqrt(sigma2) zeta - H_l g)) for nbatch >= 1 Gaussian fields g (nbatch x n_s(level), sample-major)
 * in `memspace`; zeta: nbatch x nobs standard normals in the same memspace, NULL iff the data are exact (every sigma2 == 0),
 * e.g. from pmc_normal_fill on a stream of the caller's own; f = exp when apply_exp != 0, else the identity; out may alias g.
 * Every sum has a fixed order: a realization's result does not depend on how its call was split and two identical calls agree
 * bit for bit.  Calls of more than 4 realizations run the fp64 MFMA kernel, narrower ones a VALU kernel: a column's bits may
 * differ between the two (as for pmc_sampler_create_kl handles).  PMC_ERR_INVALID: zeta == NULL with some sigma2 > 0 (and zeta
 * given for exact data), a level out of range, nbatch < 1, a NULL g / out. */
int pmc_conditioner_apply(pmc_conditioner* c, int level, int nbatch, const double* g, const double* zeta, double* out,
                          int apply_exp, int memspace);
/* The derivative of that map in g and its transpose, Gamma_l = I - K_l A_l^-1 H_l, for nbatch >= 1
 * columns of n_s(level) entries in `memspace`.  Both work on any conditioner, attached or not, derivatives enabled or not.
 * Every sum has a fixed order: a column's bits do not depend on nbatch or on how a call was split among pieces wider than 4;
 * calls of more than 4 columns run fp64 MFMA kernels, narrower ones VALU kernels (a column's bits may differ between the two).
 * PMC_ERR_INVALID: a level out of range, nbatch < 1, a NULL dg / v / out, a bad memspace, out aliasing s_out, and for the
 * adjoint out aliasing v.  Nothing is written then. */
/* out = f' o (dg - K_l A_l^-1 H_l dg); f' = s_out, or 1 when s_out == NULL.  Independent of y, sigma2 and zeta, so it is
 * valid for noisy conditioners too.  out may alias dg. */
int pmc_conditioner_apply_tangent(pmc_conditioner* c, int level, int nbatch, const double* dg, const double* s_out,
                                  double* out, int memspace);
/* out = u - H_l^T A_l^-1 K_l^T u,  u = v o s_out (u = v when s_out == NULL).  out must not alias v or s_out. */
int pmc_conditioner_apply_adjoint(pmc_conditioner* c, int level, int nbatch, const double* v, const double* s_out,
                                  double* out, int memspace);
/* on != 0: while c is attached, pmc_sampler_eval_tangent / _eval_adjoint (and with them the pmc_bayes_* derivative entries
 * and pmc_bayes_map) differentiate the CONDITIONAL field instead of refusing the handle.  Default off. */
int pmc_conditioner_enable_derivatives(pmc_conditioner* c, int on);
int pmc_conditioner_derivatives_enabled(const pmc_conditioner* c);
/* Eval hook: with a conditioner set, pmc_sampler_eval (and with it the managers, pmc_field_stats_run and the farm) returns
 * conditional fields - exp() AFTER conditioning on a lognormal handle; embed_s_out keeps the PRIOR Gaussian field (it is the
 * finer level's warm start).  NULL detaches; without a conditioner Eval takes exactly the path it took before.
 * PMC_ERR_INVALID: a conditioner with any sigma2 > 0 (Eval receives no realization id, so it has no independent noise to
 * draw: such callers use pmc_conditioner_apply), a conditioner created on another handle.  While one is attached
 * pmc_sampler_set_projection is refused, and so are pmc_sampler_eval_tangent / _eval_adjoint and everything built on them
 * unless the conditioner has pmc_conditioner_enable_derivatives on. */
int pmc_sampler_set_conditioner(pmc_sampler* s, pmc_conditioner* c);

/* invA[level]->Mult(rhs, sol) (src/PDESampler.cpp:397,521), the narrowest seam of the reference: the whole linear solve
 * A [u; s] = rhs on FULL vectors of n_u + n_s entries per realization (sample-major), every row of the solution maintained.
 * use_sol_as_guess != 0 = mfem::Solver::iterative_mode (:510): sol holds the initial guess on entry.  pmc_sampler_eval is this
 * solve with the right-hand side, warm start and output maps of Eval around it (and only the s-rows maintained); this entry
 * exists for callers that keep the reference's Eval and replace just the solver, and for true-residual checks. */
int pmc_sampler_mult(pmc_sampler* s, int level, int nbatch, const double* rhs, double* sol, int use_sol_as_guess,
                     int memspace, pmc_stats* stats);

/* z = B^-1 r: ONE application of the block-diagonal preconditioner the MINRES solves of `level` use (the reference's
 * "BJ-GS" block, examples/example_helpers/CreateSamplerParameterList.hpp:68-113), fp64 in and out, full vectors, nbatch one
 * of the level's launch widths.  Diagnostics: sqrt(<r, B^-1 r>) of a TRUE residual r = b - A x is the quantity whose
 * recurrence estimate pmc_stats.final_norm reports. */
int pmc_sampler_apply_preconditioner(pmc_sampler* s, int level, int nbatch, const double* r, double* z, int memspace);

/* y = A x with A = [M B^T; B -alpha W] of `level` (src/PDESampler.cpp:279-284; the oper->Mult inside the
 * Krylov loop, kernel K5) for nbatch in {1,2,4,8,16,32,64,128,256} vectors of n_u+n_s entries each.  The SpMM kernel is
 * launched `repeat` >= 1 times between two HIP events on the ctx stream; avg_ms (may be NULL) receives the
 * mean kernel duration, bytes (may be NULL) the algorithmic bytes of ONE launch:
 * 12 nnz + 4 nrows + nbatch * 8 * (nrows + ncols). */
int pmc_sampler_apply_operator(pmc_sampler* s, int level, int nbatch, const double* x, double* y, int memspace,
                               int repeat, double* avg_ms, double* bytes);

/* In-situ timing of the K5 launches inside the MINRES loop of pmc_sampler_eval: with on != 0 every operator launch is
 * bracketed by HIP events on the solve's own stream (adds two event records per iteration; hipGraph replay is not
 * timed).  pmc_sampler_operator_time returns and clears the accumulated kernel time [ms] and launch count. */
int pmc_sampler_set_operator_timing(pmc_sampler* s, int on);
int pmc_sampler_operator_time(pmc_sampler* s, double* total_ms, int64_t* launches);
/* Behind every timed launch an EMPTY event bracket is recorded as well: returns and clears the sum of those [ms] - what
 * the event pair itself adds to a bracket on that stream (call before pmc_sampler_operator_time clears the count). */
int pmc_sampler_operator_event_overhead(pmc_sampler* s, double* total_ms);
/* Hybridized samplers, while pmc_sampler_set_operator_timing is on: the post-smoothing kernel of the finest level of the
 * multiplier V-cycle (k::vc_postsmooth32: the largest single kernel of an iteration) is bracketed the same way.
 * pmc_sampler_smoother_bytes: algorithmic bytes of one such launch = 12 B per entry of H + 12 B per row + nbatch x
 * ((4 + 4 + 8 + z) n_lambda + 8 n_coarse): residual and pre-smoothed iterate (fp32) and r read, z written, the coarse
 * correction read once.  Both report 0 for a saddle-point sampler. */
int pmc_sampler_smoother_time(pmc_sampler* s, double* total_ms, int64_t* launches, double* event_overhead_ms);
int pmc_sampler_smoother_bytes(const pmc_sampler* s, int level, int nbatch, double* bytes);
/* Sizes of the V-cycle hierarchy the sampler runs on `level` (diagnostics: what scripts/collect_profiles.py prices the
 * per-kernel roofline table with): info[0] = rows, [1] = entries of the level operator, [2] = its stored SELL slots,
 * [3] = entries of S P (0 when the coarse correction is not folded), [4] = slots of S P, [5] = flags: bit 0 = the level runs
 * inside the LDS tail kernel (launches of more than 8 realizations), bit 1 = launches of at most 8 realizations end their
 * cycle on this level with an exact dense solve, bits 4.. = log2 of the pieces its rows are cut into for such launches (0: not
 * split), [6] = 1 when its restriction is fused into the residual kernel.
 * Returns the number of V-cycle levels through *nvlevels; vlevel out of range is an error. */
int pmc_sampler_vcycle_info(const pmc_sampler* s, int level, int vlevel, int* nvlevels, int64_t info[7]);
/* Setup values of level `vlevel` (0 = the first) of the Schur-block (hybridized: multiplier) V-cycle the solves of `level`
 * run - what a reference of the preconditioner cannot derive from the caller's data.  Reads setup only.
 * info[0] = rows, [1] = lmax of the diagonally scaled level operator, [2] = what a launch of more than dense_nb realizations
 * does on the level: 0 = smooths and descends, 1 = ends its cycle with a polynomial of degree [5] on [lmax / [6], lmax],
 * 2 = ends it with an exact solve (the level's dense inverse), 3 = does not reach it; [3] / [4] = smoothing degree / ratio
 * (interval [lmax / ratio, lmax]); [5] / [6] = degree / ratio of the polynomial a cycle ending here runs (the level's own
 * values when its spectrum is provably narrow, else mg_coarse_*); [7] = s of an internal hierarchy S_{l+1} = s P^T S_l P
 * (0: the caller's levels, each rediscretized from its level struct); [8] = ratio_M and [9] = degree of the l1-scaled
 * Chebyshev polynomial of the M-block (lmax 1; 0 on a hybridized handle); [10] = 0: the caller's levels, 1: internal smoothed
 * aggregation (mg_coarsening), 2: the multiplier aggregation of a hybridized handle; [11] = dense_nb (0: launches of every
 * width run the same cycle); [12] = [2] for launches of at most dense_nb realizations (2 there: the exact solve that ends
 * their cycle early); [13] / [14] = 1 when launches of more than / at most dense_nb realizations run the level inside the LDS
 * tail kernel.  Returns the number of V-cycle levels through *nvlevels; vlevel out of range is an error. */
int pmc_sampler_vcycle_level(const pmc_sampler* s, int level, int vlevel, int* nvlevels, double info[15]);
/* The prolongator P from V-cycle level vlevel + 1 to vlevel (0 <= vlevel < nvlevels - 1) as CSR: *nrows x *ncols with *nnz
 * entries.  Call with rowptr, colind and vals NULL for the sizes, then with arrays of nrows + 1 / nnz / nnz entries and *nnz
 * set to their capacity.  The rows of vlevel 0 are in the caller's numbering (a hybridized handle's internal renumbering of
 * the multipliers undone); coarser levels are numbered by the library, consistently from one level to the next. */
int pmc_sampler_vcycle_prolongator(const pmc_sampler* s, int level, int vlevel, int* nrows, int* ncols, int64_t* nnz,
                                   int32_t* rowptr, int32_t* colind, double* vals);

/* ---- DarcySolver ------------------------------------------------------------------------ */
int pmc_darcy_create(pmc_ctx* ctx, int nlevels, int n_mc_levels, const pmc_darcy_level* levels,
                     int k_divides, const pmc_solver_opts* opts, pmc_darcy** out);
/* The same handle with SolveFwd through the HYBRIDIZED form of the mixed system - the reference's "Hybridization" branch of
 * DarcySolver (src/DarcySolver.cpp:586,619: the solver factory eliminates flux and pressure element by element).  Same level
 * structs: the element-local inverses are formed inside the library from the contribution lists of M (as pmc_hybrid_build does
 * for the sampler), one Lagrange multiplier per interior / essential face, H(k) lambda = rhs(k) with H linear in the
 * realization's coefficients solved by MINRES + one V-cycle of a per-realization aggregation hierarchy, then the element-local
 * back-substitution; Q, the returned solution and the pressure block are those of the saddle-point solve to the solver
 * tolerance.  Needs every face to belong to at most two elements and essential dofs on boundary faces only.  ComputeG keeps
 * the saddle-point path. */
int pmc_darcy_create_hybrid(pmc_ctx* ctx, int nlevels, int n_mc_levels, const pmc_darcy_level* levels,
                            int k_divides, const pmc_solver_opts* opts, pmc_darcy** out);
void pmc_darcy_destroy(pmc_darcy* d);
int pmc_darcy_num_dofs(const pmc_darcy* d, int level); /* GetGlobalNumberOfDofs() */
int pmc_darcy_num_pressure_dofs(const pmc_darcy* d, int level); /* GetSizeOfStochasticData(): entries of k */
int64_t pmc_darcy_nnz(const pmc_darcy* d, int level);  /* GetNNZ()                */
int pmc_darcy_batch_width(const pmc_darcy* d, int level);  /* as pmc_sampler_batch_width */
/* In-situ timing of the dominant kernel of the Darcy operator inside the MINRES loop of SolveFwd (solver->Mult,
 * src/DarcySolver.cpp:629-631): the u-rows y_u = M(k) x_u + B^T x_p with the fused <x, Ax> (eg_pair_spmm_kernel).  With
 * on != 0 every such launch is bracketed by HIP events on the solve's stream and an empty bracket is recorded behind it;
 * while timing, the p-rows (B x_u) follow on the same stream instead of running beside it.  pmc_darcy_operator_time returns
 * and clears the accumulated bracket time, the launch count and the sum of the empty brackets [ms];
 * pmc_darcy_operator_bytes gives the ALGORITHMIC bytes of one such launch for nbatch realizations: element-grouped M(k)
 * 12 B per stored slot + 8 B per dof (coefficient rows) + the coefficient table (n_p + 1) x nbatch x 8, B^T 12 B per nonzero,
 * 4 B per row, vectors nbatch (z (n_u + n_p) + 8 n_u) with z = pmc_krylov_z_bytes(). */
int pmc_darcy_set_operator_timing(pmc_darcy* d, int on);
int pmc_darcy_operator_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms);
int pmc_darcy_operator_bytes(const pmc_darcy* d, int level, int nbatch, double* bytes);
/* The same for the other large gather kernel of a Darcy iteration, the M-block polynomial of the preconditioner
 * z_u = D^-1 (c0 r - c1 M(k) D^-1 r) (eg_poly2_kernel; the reference's A00^-1 block, three l1-Gauss-Seidel sweeps on M(k),
 * CreateSamplerParameterList.hpp:80-93): timed by the same pmc_darcy_set_operator_timing switch (the launch then runs on
 * the solve's main stream instead of beside the V-cycle's bottom).  Algorithmic bytes: 12 B per stored slot of the
 * element-grouped matrix + 12 B per dof + the coefficient table + nbatch ((8 + 8 + z) n_u): r and the per-realization l1
 * diagonal read, z written. */
int pmc_darcy_poly_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms);
int pmc_darcy_poly_bytes(const pmc_darcy* d, int level, int nbatch, double* bytes);
/* SolveFwd(level, k, Q, C) (src/DarcySolver.cpp:416-437).  k: nbatch x n_p(level) in
 * `memspace`; Q, C: host arrays of nbatch; sol_out (may be NULL): nbatch x (n_u+n_p) in
 * `memspace` (SolveFwd_RtnPressure, :439-470, reads its p-block). */
int pmc_darcy_solve_fwd(pmc_darcy* d, int level, int nbatch, const double* k, double* Q, double* C,
                        double* sol_out, int memspace, pmc_stats* stats);

/* SolveFwd_RtnPressure(level, k, P, C, Q, compute_Q) (src/DarcySolver.cpp:439-470): the pressure block of the
 * solution, nbatch x n_p(level) in `memspace`; Q (host, may be NULL) is only written when compute_Q != 0, and is the Q
 * pmc_darcy_solve_fwd returns for the same call, bit for bit. */
int pmc_darcy_solve_fwd_pressure(pmc_darcy* d, int level, int nbatch, const double* k, double* p_out, double* C,
                                 double* Q, int compute_Q, int memspace, pmc_stats* stats);

/* ---- Pressure accumulators of the multilevel field estimates ----------------------------------- */
/* Accumulators of ONE Darcy level's pressure block for the MLMC telescoping sum, on the device: per fine element i the
 * sums of d = p - p_c[parent(i)], d^2 and p^2 - p_c[parent(i)]^2 as (sum, compensation) pairs (Neumaier), added in
 * ascending realization id.  parent() is derived at create from the handle's own pressure prolongator P(level), which must
 * be a 0/1 injection (every row a single 1.0).  coupled != 0: the level has a coarse partner level + 1 (requires
 * level + 1 < n_mc_levels); coupled == 0: p_c = 0 (the coarsest level of an estimator).  Work is enqueued on ctx's stream
 * (ctx on the device of d); device-memory accumulates are asynchronous there.  The sums are bit-identical however the
 * realizations are split into calls.  Refused with PMC_ERR_INVALID: a row of P that is not a single 1.0, a level out of
 * range, coupled on the last Monte Carlo level, NULL pointers, nbatch < 1, a p_coarse that does not match coupled. */
typedef struct pmc_level_fields pmc_level_fields;
int pmc_level_fields_create(pmc_ctx* ctx, const pmc_darcy* d, int level, int coupled, pmc_level_fields** out);
void pmc_level_fields_destroy(pmc_level_fields* f);   /* before the Darcy handle and the ctx */
int pmc_level_fields_reset(pmc_level_fields* f);
/* nbatch pressure blocks, sample-major as pmc_darcy_solve_fwd_pressure writes them: p_fine nbatch x n_p(level), p_coarse
 * nbatch x n_p(level + 1) (NULL iff !coupled); realizations in ascending id */
int pmc_level_fields_accumulate(pmc_level_fields* f, int nbatch, const double* p_fine, const double* p_coarse,
                                int memspace);
/* The weighted form (the ratio managers' posterior field estimates): per realization b the terms
 * a = w_fine[b] x_fine, c = w_coarse[b] x_coarse[parent] and the sums of a - c, (a - c)^2 and a x_fine - c x_coarse[parent]
 * in the same six pairs, products rounded before they are summed.  w_fine, w_coarse: HOST arrays of nbatch, read before
 * the call returns (w_coarse NULL iff !coupled).  With every weight 1.0 the sums equal pmc_level_fields_accumulate's bit for
 * bit; they are bit-identical however the realizations are split into calls.  The same refusals as
 * pmc_level_fields_accumulate, and NULL weights where they are required. */
int pmc_level_fields_accumulate_weighted(pmc_level_fields* f, int nbatch, const double* x_fine, const double* w_fine,
                                         const double* x_coarse, const double* w_coarse, int memspace);
/* the raw accumulators, 6 x n_p(level) doubles [sum d | comp | sum d^2 | comp | sum p^2 - p_c^2 | comp] (sum + comp is the
 * compensated sum), and the number of realizations accumulated */
int pmc_level_fields_read_sums(const pmc_level_fields* f, double* sums, int64_t* count, int memspace);
/* n_p(level) and n_p(level + 1) (0 when not coupled); parent(): n_p(level) entries (coupled levels only) */
int pmc_level_fields_size(const pmc_level_fields* f, int* n_fine, int* n_coarse);
int pmc_level_fields_parents(const pmc_level_fields* f, int32_t* parent);

/* z = B(k)^-1 r: ONE application of the block-diagonal preconditioner the MINRES solve of `level` uses, column b with its
 * own permeability k[b*n_p .. (b+1)*n_p) (the same per-realization setup and the same kernels as pmc_darcy_solve_fwd).
 * r, z: nbatch x (n_u + n_p) sample-major, fp64 in and out; on a handle from pmc_darcy_create_hybrid they are multiplier
 * vectors (the V-cycle of H(kappa)), nbatch x n_lambda.  nbatch: one of the level's launch widths (1, 2, 4, ... up to
 * pmc_darcy_batch_width).  All arrays in `memspace`.  With PMC_STORAGE_FP32 the solver additionally rounds z to fp32. */
int pmc_darcy_apply_preconditioner(pmc_darcy* d, int level, int nbatch, const double* k, const double* r, double* z,
                                   int memspace);
/* y = A(k) x, the operator of the same solve: [M(k) B^T; B 0] with the essential rows and columns eliminated (unit
 * diagonal), or H(kappa) on a hybridized handle.  Arguments as pmc_darcy_apply_preconditioner. */
int pmc_darcy_apply_operator(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, double* y, int memspace);
/* Setup values of level `vlevel` (0 = the first) of the Schur-block (hybridized: multiplier) V-cycle the solves of `level`
 * run (what a reference of B(k)^-1 cannot derive from the caller's data): info[0] = rows, [1] = lmax of the diagonally scaled
 * level operator (1 on an internal hierarchy: there the per-realization Gershgorin bound 1.0001 max_i sum_j |S_ij| / |S_ii| is
 * folded into D^-1), [2] = 1 when the cycle ends on this level, [3] / [4] = smoothing degree / ratio (interval
 * [lmax / ratio, lmax]), [5] / [6] = degree / ratio of the polynomial solve that ends the cycle, [7] = s of
 * S_{l+1}(k) = s P^T S_l(k) P (1/2 on the caller's hierarchy, 1 on an internal aggregation hierarchy, 0.5 on the multiplier
 * hierarchy of a hybridized handle), [8] = ratio_M and [9] = degree of the l1-scaled Chebyshev polynomial of the M-block
 * (lmax 1), [10] = 0: the caller's hierarchy (P of the level structs), 1: an internal aggregation hierarchy, 2: the
 * multiplier hierarchy of a hybridized handle.  Returns the number of V-cycle levels through *nvlevels; vlevel out of range
 * is an error. */
int pmc_darcy_vcycle_level(const pmc_darcy* d, int level, int vlevel, int* nvlevels, double info[11]);
/* The prolongator P from V-cycle level vlevel + 1 to vlevel (0 <= vlevel < nvlevels - 1) of that cycle as CSR, for every
 * hierarchy kind (the caller's P on the caller's hierarchy).  Sizes and errors as pmc_sampler_vcycle_prolongator: call with
 * rowptr, colind and vals NULL for *nrows, *ncols and *nnz, then with arrays of nrows + 1 / nnz / nnz entries and *nnz set to
 * their capacity.  The rows of vlevel 0 are in the caller's numbering (P0 elements; the multipliers of a hybridized handle:
 * interior and essential faces in face order); coarser levels are numbered by the library, consistently from one level to the
 * next.  Reads setup only. */
int pmc_darcy_vcycle_prolongator(const pmc_darcy* d, int level, int vlevel, int* nrows, int* ncols, int64_t* nnz,
                                 int32_t* rowptr, int32_t* colind, double* vals);

/* Bayesian observation operator (src/BayesianInverseProblem.cpp:178-186, ComputeG): Gobs is nobs x n_p(level), row i
 * = the observation functional g_obs_i (e.g. the indicator of the cells around an observation point, restricted to the
 * level).  pmc_darcy_compute_G solves like SolveFwd and returns G[b*nobs + i] = <g_i, p_b> / sum(g_i) (host array) plus
 * Q and C (host, may be NULL); only the rows of the solution that Q and G read are maintained by the Krylov solver.  Q is
 * <obs, x> also on a level with a tracer attached (pmc_darcy_set_tracer). */
int pmc_darcy_set_observations(pmc_darcy* d, int level, const pmc_csr* Gobs);
int pmc_darcy_num_observations(const pmc_darcy* d, int level);
int pmc_darcy_compute_G(pmc_darcy* d, int level, int nbatch, const double* k, double* G, double* C, double* Q,
                        int memspace, pmc_stats* stats);

/* ---- Adjoint gradients with respect to the permeability field (an extension: the reference has none)
 * The mixed system is symmetric: with A(k) x = rhs_bc (essential rows of x hold the essential data) and A(k) lam = dJ/dx
 * (essential rows of lam zero), dJ/dc_e = -lam_u^T M_e x_u with M_e the unit-coefficient element matrix of the level's
 * contribution lists, and dJ/dk_e = c'(k_e) dJ/dc_e, c = 1/k (k_divides) or k.  wrt_log != 0: the gradient with respect to
 * log k (times k).  k, grad: nbatch x n_p(level); full vectors: nbatch x (n_u + n_p), sample-major; arrays in `memspace`
 * unless stated.  Column b of every result is the same, bit for bit, however nbatch is split into calls and launches.  All
 * three functions take the saddle-point path, also on a handle from pmc_darcy_create_hybrid (as pmc_darcy_compute_G does),
 * and their Q and J = Q are <obs, x> also on a level with a tracer attached (pmc_darcy_set_tracer).
 * Refused with PMC_ERR_INVALID: a level outside [0, n_mc_levels), nbatch < 1, NULL k / grad; non-positive k is the caller's
 * problem, as in pmc_darcy_solve_fwd. */
/* In-situ timing of the mass-sensitivity kernel (the one new kernel of a gradient), on the pmc_darcy_set_operator_timing switch
 * and with the meaning of pmc_darcy_operator_time; ALGORITHMIC bytes of one launch for nbatch realizations: per element n_fe
 * face indices (4 B) + n_fe^2 matrix entries (8 B) + nbatch x 16 (k read, gradient written), and every row of x_u and lam_u
 * once (nbatch x 16 n_u).  The bytes call builds the level's gradient data when no gradient has been asked for yet. */
int pmc_darcy_mass_sensitivity_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms);
int pmc_darcy_mass_sensitivity_bytes(pmc_darcy* d, int level, int nbatch, double* bytes);
/* grad[b*n_p + e] = -c'(k) lam_u^T M_e x_u for caller-supplied vectors x, lam.  No solve. */
int pmc_darcy_mass_sensitivity(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, const double* lam,
                               int wrt_log, double* grad, int memspace);
/* Forward solve, adjoint solve, gradient: one per-realization setup serves both solves (same operator, preconditioner and
 * options; the adjoint solve starts from zero).  adj_rhs: nbatch x (n_u + n_p) = dJ/dx per realization, or NULL = the level's
 * obs (J = Q); its essential rows are ignored.  Q, C (host, may be NULL) as pmc_darcy_solve_fwd - Q bit-identical to
 * pmc_darcy_solve_fwd(..., sol_out != NULL) of the same call; sol_out / adj_out (may be NULL): x and lam; stats_fwd /
 * stats_adj (may be NULL): nbatch entries for the two solves. */
int pmc_darcy_solve_gradient(pmc_darcy* d, int level, int nbatch, const double* k, const double* adj_rhs, int wrt_log,
                             double* Q, double* C, double* grad, double* sol_out, double* adj_out, int memspace,
                             pmc_stats* stats_fwd, pmc_stats* stats_adj);
/* Gradient of the Gaussian log-likelihood loglik = -|G(k) - data|^2 / (2 noise) of the handle's observation functionals
 * (pmc_darcy_set_observations; the logarithm of BayesianInverseProblem::ComputeLikelihood, src/BayesianInverseProblem.cpp:196):
 * forward solve -> G -> adjoint right-hand side -(1/noise) sum_i (G_i - data_i) g_i / sum(g_i) on the p-rows, formed on the
 * device -> adjoint solve -> gradient.  data: HOST array of nobs; loglik (nbatch), G (nbatch x nobs): host arrays, may be NULL.
 * Also refused: no observation functionals on the level, noise <= 0, NULL data. */
int pmc_darcy_loglik_gradient(pmc_darcy* d, int level, int nbatch, const double* k, const double* data, double noise,
                              int wrt_log, double* loglik, double* G, double* grad, int memspace, pmc_stats* stats_adj);

/* ---- Gauss-Newton Hessian-vector products of the negative log-likelihood in k (an extension)
 * With J = dG/dk of the handle's observation functionals: hv = J^T (1/noise) J dk, symmetric positive semi-definite.  For a
 * direction dk per element (wrt_log != 0: a direction in log k, and hv with respect to log k) the coefficient changes by
 * dc_e = c'(k_e) dk_e (times k_e), the tangent right-hand side is t_u[f] = -sum_{e has f} dc_e sum_a' M_e[a(f), a'] x_u[f_e(a')]
 * on the free rows (0 on the essential rows, t_p = 0), A(k) dx = t gives dG_i = <g_i, dp> / sum(g_i) = (J dk)_i, and
 * A(k) lam = [0; (1/noise) sum_i dG_i g_i / sum(g_i)] gives hv = pmc_darcy_mass_sensitivity(k, x, lam).  Array shapes, memory
 * spaces, the saddle-point path on hybridized handles and the bitwise independence of a column from the launch width and the
 * split of a call: as for the gradients above.  A tracer attached to the level (pmc_darcy_set_tracer) changes nothing here:
 * these entries read the observation functionals and <obs, x> only. */
/* In-situ timing of the tangent right-hand side kernel (the one new kernel), on the pmc_darcy_set_operator_timing switch and
 * with the meaning of pmc_darcy_operator_time; ALGORITHMIC bytes of one launch for nbatch realizations: per face and side an
 * element id (4 B), n_fe face indices (4 B) and n_fe matrix entries (8 B) - n_u nside (4 + 12 n_fe) -, k and dk read once
 * (nbatch x 16 n_p), every row of x_u read and of t_u written once (nbatch x 16 n_u).  The bytes call builds the level's
 * face-major data when no tangent has been asked for yet. */
int pmc_darcy_mass_tangent_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms);
int pmc_darcy_mass_tangent_bytes(pmc_darcy* d, int level, int nbatch, double* bytes);
/* t_out[b*(n_u+n_p) + f] = the tangent right-hand side for caller-supplied x and dk; the p-rows are zero.  No solve.
 * Refused with PMC_ERR_INVALID: a level outside [0, n_mc_levels), nbatch < 1, a NULL array. */
int pmc_darcy_mass_tangent(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, const double* dk,
                           int wrt_log, double* t_out, int memspace);
/* hv = J^T (1/noise) J dk.  x_in NULL: the forward solve A(k) x = rhs_bc runs inside, as in pmc_darcy_solve_gradient, and
 * x_out (may be NULL) returns x; x_in given (sol_out of pmc_darcy_solve_gradient, or x_out of an earlier call): no forward
 * solve runs, and the result is the same bit for bit.  dG: HOST array nbatch x nobs, may be NULL: J dk.  One per-realization
 * setup serves all solves; the tangent and the adjoint solve use the operator, preconditioner and options of the forward
 * solve from a zero guess.  stats_tan / stats_adj (may be NULL): nbatch entries for the two solves.  Refused with
 * PMC_ERR_INVALID: a level out of range, nbatch < 1, NULL k / dk / hv, no observation functionals on the level, noise <= 0,
 * x_out together with x_in. */
int pmc_darcy_gn_hessvec(pmc_darcy* d, int level, int nbatch, const double* k, const double* x_in, const double* dk,
                         double noise, int wrt_log, double* hv, double* dG, double* x_out, int memspace, pmc_stats* stats_tan,
                         pmc_stats* stats_adj);

/* ---- Batched conjugate-gradient vector algebra for Newton-CG (an extension)
 * A workspace for nb <= nbatch_max independent CG iterations H_b d_b = g_b on columns of length n, vectors sample-major
 * nb x n.  The caller owns the operator: it applies H to pmc_ncg_search_direction (p) for the whole batch and hands Hp to
 * pmc_ncg_step; everything between two applications (<p, Hp>, alpha, d += alpha p, r -= alpha Hp, <r, r>, the tolerance test,
 * beta, p = r + beta p) runs on the device in three launches, and the per-column scalars never leave it: pmc_ncg_status is
 * the one small copy a CG step needs.
 *   begin: on the columns with active_mask[b] != 0 (NULL: all) d = 0, r = p = g and the column ends once <r, r> <=
 *          (eta_b |g_b|)^2; on the others p = 0 and nothing else is written.  eta, active_mask: HOST arrays of nb.
 *   step:  one CG step of every unfinished column with Hp = H p.  A column whose <p, Hp> is not positive ends with its
 *          non-positive-curvature flag set and keeps its d (d = g when this was its first step).  A column that ends gets
 *          p = 0, once; after that none of its vectors is written.  The cap on the steps is the caller's loop.
 *   status (host arrays of nb, each may be NULL): <r, r>, steps taken, finished, ended on non-positive curvature.
 *   axpy_cols: out_b = x_b + t_b d_b on the columns with t_b != 0 (d NULL: out_b = x_b, a masked copy); a column with
 *          t_b == 0 is masked and not written.  t: HOST array of nb.  out may be x.
 *   dot_cols: out_host[b] = <a_b, b_b> for all nb columns.
 * Every sum has a fixed order that depends on n alone (chunks of 4096 entries, a fixed tree inside a chunk, the chunk sums
 * added in ascending order, no atomics): a column's vectors and scalars have the same bits at every nb, beside any other
 * columns, in either memory space and in repeated calls.  With PMC_MEM_HOST the arrays are staged through the workspace; the
 * workspace's own vectors (the three pointers below, device memory) may be passed as arguments in either memory space.
 * Refused with PMC_ERR_INVALID: n or nbatch_max < 1, nb outside [1, nbatch_max], a NULL array, a negative eta, a step whose
 * nb differs from its begin. */
typedef struct pmc_ncg pmc_ncg;
int pmc_ncg_create(pmc_ctx* ctx, int n, int nbatch_max, pmc_ncg** out);
void pmc_ncg_destroy(pmc_ncg* w);
int pmc_ncg_begin(pmc_ncg* w, int nb, const double* g, const double* eta, const int32_t* active_mask, int memspace);
int pmc_ncg_step(pmc_ncg* w, int nb, const double* Hp, int memspace);
double* pmc_ncg_direction(pmc_ncg* w);          /* d: nbatch_max x n on the device */
double* pmc_ncg_search_direction(pmc_ncg* w);   /* p */
double* pmc_ncg_residual(pmc_ncg* w);           /* r */
int pmc_ncg_status(pmc_ncg* w, int nb, double* rr, int32_t* cg_count, int32_t* done, int32_t* nonpos_curvature);
int pmc_ncg_axpy_cols(pmc_ncg* w, int nb, const double* t, const double* x, const double* d, double* out, int memspace);
int pmc_ncg_dot_cols(pmc_ncg* w, int nb, const double* a, const double* b, double* out_host, int memspace);

/* ---- Particle travel times on the Darcy flux as a QoI (an extension: the reference has none)
 * How long a particle released at a point takes to leave the domain in the RT0 velocity field of a solve, u / porosity.  A
 * u-dof is the total flux through a face along the face's global normal, so inside an element every coordinate - a box axis,
 * a barycentric coordinate of a tetrahedron - obeys a scalar linear ODE, and the time to the next face is closed-form
 * (Pollock's method): no time stepper, no step-size parameter.  One thread walks one particle of one realization.
 *   create: the mesh arrays are copied and packed; the particles are sorted by start element (the outputs are in the caller's
 *           order).  A start point may lie outside its elem0 by at most 1e-12 of the element's extent and is clamped into it.
 *   run:    u: nbatch rows of n_face fluxes, row b at u + b * ld (sol_out of pmc_darcy_solve_fwd passes as it is with
 *           ld = n_u + n_p).  Outputs, nbatch x nparticles each, in `memspace` like u: T the travel time (the time
 *           accumulated so far when the path did not exit), exit_face the global id of the boundary face (-1: none), status,
 *           nsteps the elements crossed, x_exit (may be NULL) nbatch x nparticles x 3 the last position.
 *   status: PMC_TRACER_EXITED through a boundary face; PMC_TRACER_STAGNANT: no face of the current element can be reached
 *           (all candidate velocities zero or inward); PMC_TRACER_MAX_STEPS: the step counter reached max_steps.
 *   reduce: Q[b] (host) = mean of T over all particles of realization b, censored times included (PMC_TRACER_MEAN), or their
 *           minimum (PMC_TRACER_MIN); not_exited[b] (host, may be NULL) = particles whose status is not EXITED.  T, status in
 *           `memspace`.  The sum has a fixed order (ascending particles per thread, a fixed tree across the workgroup).
 * A particle's outputs have the same bits at every nbatch, beside any other realizations, in either memory space, in repeated
 * calls, and when the walk runs inside a solve (pmc_darcy_set_tracer).
 * Scope: 3-D meshes of axis-aligned hexahedra or of tetrahedra with element geometry.  2-D meshes and agglomerated levels
 * (no element geometry) are not supported.
 * Refused with PMC_ERR_INVALID (nothing is written, the handle stays usable): a kind other than the two, a NULL array
 * (porosity and x_exit excepted), nparticles < 1, max_steps < 0 or > 2^22, porosity <= 0, elem_face / elem_sign and face_elem
 * that disagree, boxes that are not axis-aligned and conforming (lo >= hi; a neighbour across local face l that does not meet
 * the box with its opposite face in the same plane and cross-section), a simplex of non-positive volume, an elem0 out of
 * range or a start point outside its elem0, nbatch < 1, ld < n_face, a bad memspace. */
enum pmc_tracer_kind { PMC_TRACER_BOX = 0, PMC_TRACER_SIMPLEX = 1 };
enum pmc_tracer_status { PMC_TRACER_EXITED = 0, PMC_TRACER_STAGNANT = 1, PMC_TRACER_MAX_STEPS = 2 };
enum pmc_tracer_qoi { PMC_TRACER_MEAN = 0, PMC_TRACER_MIN = 1 };
typedef struct pmc_tracer_mesh {      /* host arrays, copied at create */
    int32_t kind;                     /* PMC_TRACER_BOX (axis-aligned hexahedra) | PMC_TRACER_SIMPLEX (tetrahedra) */
    int32_t n_elem, n_face;
    const int32_t* elem_face;         /* n_elem x n_fe (6 | 4); hexahedra: z-, y-, x+, y+, x-, z+; face i of a tetrahedron is opposite vertex i */
    const int8_t*  elem_sign;         /* n_elem x n_fe, +1: outward = the face's global normal */
    const int32_t* face_elem;         /* n_face x 2, second -1 on the boundary */
    const double*  geom;              /* BOX: n_elem x 6 (lo, hi); SIMPLEX: n_elem x 4 x 3 vertex coordinates, positively oriented */
    const double*  porosity;          /* n_elem, > 0; NULL = 1 */
} pmc_tracer_mesh;
typedef struct pmc_tracer pmc_tracer;
int pmc_tracer_create(pmc_ctx* ctx, const pmc_tracer_mesh* mesh, int nparticles, const double* x0 /* nparticles x 3 */,
                      const int32_t* elem0, int max_steps /* 0: 64 + 32 ceil(cbrt(n_elem)) */, pmc_tracer** out);
void pmc_tracer_destroy(pmc_tracer* t);   /* detach it first (pmc_darcy_set_tracer with NULL); before the ctx */
int pmc_tracer_num_particles(const pmc_tracer* t);
int pmc_tracer_run(pmc_tracer* t, int nbatch, const double* u, int64_t ld, double* T, int32_t* exit_face,
                   int32_t* status, int32_t* nsteps, double* x_exit /* may be NULL */, int memspace);
int pmc_tracer_reduce(pmc_tracer* t, int nbatch, const double* T, const int32_t* status, int kind,
                      double* Q /* host */, int32_t* not_exited /* host, may be NULL */, int memspace);
/* Makes the travel-time QoI (kind: PMC_TRACER_MEAN | PMC_TRACER_MIN) the Q of pmc_darcy_solve_fwd and of
 * pmc_darcy_solve_fwd_pressure (compute_Q) on `level`: it is computed on the solver's internal solution before any copy-out,
 * equals pmc_tracer_reduce of pmc_tracer_run on sol_out bit for bit, and is what the managers, lanes and farms then see.  The
 * solve maintains the full solution also when sol_out is NULL.  Every other entry keeps Q = <obs, x>: pmc_darcy_compute_G,
 * the gradients (pmc_darcy_solve_gradient, pmc_darcy_loglik_gradient) and the Hessian actions (pmc_darcy_gn_hessvec) - the
 * Q of pmc_darcy_solve_gradient is then no longer that of pmc_darcy_solve_fwd.  t == NULL detaches and restores <obs, x>.
 * The tracer is not owned, serves one Darcy handle at a time (each lane its own), and must outlive the attachment.
 * Refused with PMC_ERR_INVALID: a level outside [0, n_mc_levels), n_face != n_u(level) or n_elem != n_p(level), a tracer
 * created on another context's device, a kind other than the two. */
int pmc_darcy_set_tracer(pmc_darcy* d, int level, pmc_tracer* t, int kind);

/* ---- Upwind solute transport on the Darcy flux as a QoI (an extension: the reference has none)
 * First-order upwind finite-volume advection of a passive solute on the P0 elements of a level: the breakthrough curve at an
 * outlet and the mass still in place at t_end.  It needs no geometry - only the rows of the level's divergence matrix B
 * (n_elem x n_face CSR, not eliminated), the flux block of a solve and one pore volume per element - so it serves triangles,
 * quadrilaterals, hexahedra, tetrahedra and unsmoothed agglomerated levels alike.
 *   mesh:   every column of B has one entry (a boundary dof) or two entries in two elements, of opposite sign and with
 *           |a + b| <= 1e-12 max(|a|, |b|) (an interior dof).  a_f = |B[e_first, f]| of the dof's lowest element, and the
 *           outward rate of element e through its l-th row entry is g_l = sign(B[e, f]) * (a_f * u_f).
 *   scheme: out_e = sum_l max(g_l, 0), in_e = sum_l max(-g_l, 0), r_e = max(out_e, in_e), rate = max_e r_e / V_e;
 *           x = (t_end * rate) / cfl, nsteps = max(1, ceil(x)), dt = t_end / nsteps; per step
 *           c_e' = (1 - (dt / V_e) r_e) c_e + (dt / V_e) sum_l max(-g_l, 0) cn_l with cn_l the neighbour's old concentration,
 *           c_in[f] on a boundary dof.  A source dilutes with clean water, a sink extracts at c_e.
 *   run:    u: nbatch rows of n_face fluxes, row b at u + b * ld (sol_out of pmc_darcy_solve_fwd passes as it is with
 *           ld = n_u + n_p).  Outputs in `memspace` like u: c_out (nbatch x n_elem, may be NULL) the concentrations at
 *           t_reached; curve (nbatch x nreport) the mass that left through the outlet dofs by r t_reached / nreport,
 *           r = 1 .. nreport (linear within a step); stored = sum_e weight_e c_e; rate, t_reached, nsteps, status per column.
 *   status: PMC_TRANSPORT_OK; PMC_TRANSPORT_STEP_LIMIT: nsteps would exceed max_steps - the column runs max_steps steps of
 *           dt = cfl / rate and reaches t_reached = max_steps dt < t_end; PMC_TRANSPORT_BAD_FLUX: a flux of the column is not
 *           finite (rate = +inf) - no step, nsteps = 0, t_reached = 0, c = c0, a zero curve.
 *   reduce: Q[b] (host) = curve[b][nreport - 1] (PMC_TRANSPORT_MASS_OUT) or stored[b] (PMC_TRANSPORT_STORED).
 * The sums over outlet dofs and over elements have a fixed order (that of pmc_tracer_reduce).  A column's outputs have the
 * same bits at every nbatch, beside any other columns, in either memory space, in repeated calls, and when the transport runs
 * inside a solve (pmc_darcy_set_transport).
 * Refused with PMC_ERR_INVALID (nothing is written, the handle stays usable): a NULL required argument, n_elem < 1 or
 * n_face < 1, a bad rowptr, a column index out of range, a zero or non-finite entry of val, a column of B that breaks the rule
 * above, a pore volume that is not positive and finite, a non-finite entry of c0, c_in or weight, an outlet flag on an
 * interior dof, t_end <= 0, cfl outside (0, 1], nreport outside [1, 4096], max_steps < 0 or > 2^24, nbatch < 1, ld < n_face,
 * a bad memspace, a kind other than the two. */
enum pmc_transport_status { PMC_TRANSPORT_OK = 0, PMC_TRANSPORT_STEP_LIMIT = 1, PMC_TRANSPORT_BAD_FLUX = 2 };
enum pmc_transport_qoi { PMC_TRANSPORT_MASS_OUT = 0, PMC_TRANSPORT_STORED = 1 };
typedef struct pmc_transport_mesh {   /* host arrays, copied at create */
    int32_t n_elem, n_face;
    const int32_t* rowptr;            /* B of the level, CSR: n_elem + 1 */
    const int32_t* col;
    const double*  val;
    const double*  pore_volume;       /* n_elem, > 0 */
    const double*  c0;                /* n_elem, NULL = 0 */
    const double*  c_in;              /* n_face, NULL = 1; read on boundary dofs only */
    const uint8_t* outlet;            /* n_face, NULL = every boundary dof; set only on boundary dofs */
    const double*  weight;            /* n_elem, NULL = pore_volume */
} pmc_transport_mesh;
typedef struct pmc_transport_params {
    double t_end, cfl;
    int32_t nreport, max_steps;       /* max_steps 0: 65536 */
} pmc_transport_params;
typedef struct pmc_transport pmc_transport;
int pmc_transport_create(pmc_ctx* ctx, const pmc_transport_mesh* mesh, const pmc_transport_params* params, pmc_transport** out);
void pmc_transport_destroy(pmc_transport* t);   /* detach it first (pmc_darcy_set_transport with NULL); before the ctx */
int pmc_transport_size(const pmc_transport* t, int* n_elem, int* n_face, int* n_outlet, int* nreport);
int pmc_transport_run(pmc_transport* t, int nbatch, const double* u, int64_t ld, double* c_out /* may be NULL */, double* curve,
                      double* stored, double* rate, double* t_reached, int32_t* nsteps, int32_t* status, int memspace);
int pmc_transport_reduce(pmc_transport* t, int nbatch, const double* curve, const double* stored, int kind, double* Q /* host */,
                         int memspace);
/* Makes the transport QoI (kind: PMC_TRANSPORT_MASS_OUT | PMC_TRANSPORT_STORED) the Q of pmc_darcy_solve_fwd and of
 * pmc_darcy_solve_fwd_pressure on `level`, as pmc_darcy_set_tracer does for the travel time: computed on the solver's internal
 * solution before any copy-out, equal to pmc_transport_reduce of pmc_transport_run on sol_out bit for bit; the solve maintains
 * the full solution.  pmc_darcy_compute_G, the gradients and the Hessian actions keep Q = <obs, x>.  t == NULL detaches.  A
 * level holds a tracer or a transport, not both: attaching one while the other is attached is refused, here and in
 * pmc_darcy_set_tracer.  The handle is not owned, serves one Darcy handle at a time and must outlive the attachment.
 * Refused with PMC_ERR_INVALID: a level outside [0, n_mc_levels), n_face != n_u(level) or n_elem != n_p(level), a handle
 * created on another context's device, a kind other than the two, a tracer attached to the level. */
int pmc_darcy_set_transport(pmc_darcy* d, int level, pmc_transport* t, int kind);

/* ---- The adjoint of the solute transport: gradients of breakthrough data (an extension)
 * For J = <curve_bar, curve> + stored_bar stored + <c_bar, c> per column, pmc_transport_run_adjoint returns u_bar = dJ/du
 * (the first n_face entries of the row at u_bar + b * ld_bar; nothing else of the row is written) and c0_bar = dJ/dc0 (nbatch
 * x n_elem, may be NULL), the discrete adjoint of the scheme above with three decisions of the forward pass held fixed: the
 * step count, the sign of every g_l (g_l == 0 contributes nothing) and the branch out_e >= in_e of r_e.  Seeds: curve_bar
 * (nbatch x nreport), stored_bar (nbatch), c_bar (nbatch x n_elem); each may be NULL and then counts as zero, at least one must
 * be given.  The forward outputs curve, stored, nsteps (each may be NULL) and status are those of pmc_transport_run bit for
 * bit.  A column whose status is not PMC_TRANSPORT_OK is not differentiated: its u_bar and c0_bar are zero.  All arrays in
 * `memspace`.
 *   history: the sweep needs every state c^n.  The forward pass keeps every K-th one and the sweep recomputes a segment of K
 *            states at a time, with the forward bits.  K = ceil(sqrt(largest step count of the launch)) unless
 *            pmc_transport_set_adjoint_segment sets one (0: automatic again); scratch about (N / K + K) n_elem nbatch doubles.
 * A column's results have the same bits at every nbatch, in every split into calls, in either memory space, at every K and
 * in repeated calls; pmc_transport_run is not disturbed.
 * Refused with PMC_ERR_INVALID (nothing is written, the handle stays usable): all three seeds NULL; NULL u, u_bar or status;
 * ld or ld_bar < n_face; nbatch < 1; a bad memspace; K < 0. */
int pmc_transport_run_adjoint(pmc_transport* t, int nbatch, const double* u, int64_t ld,
                              const double* curve_bar /* nbatch x nreport | NULL */, const double* stored_bar /* nbatch | NULL */,
                              const double* c_bar /* nbatch x n_elem | NULL */, double* u_bar, int64_t ld_bar /* >= n_face */,
                              double* c0_bar /* nbatch x n_elem | NULL */, double* curve /* | NULL */, double* stored /* | NULL */,
                              int32_t* nsteps /* | NULL */, int32_t* status, int memspace);
int pmc_transport_set_adjoint_segment(pmc_transport* t, int K);   /* 0: automatic */
/* dJ/dk (wrt_log: dJ/dlog k) of J = <curve_bar, curve> + stored_bar stored of the transport t on the flux of the level's
 * Darcy solution, per realization: forward solve, the transport and its adjoint on the solver's internal solution, u_bar as the
 * u rows of the adjoint right-hand side (p rows and essential rows zero), adjoint solve, pmc_darcy_mass_sensitivity - the
 * pipeline of pmc_darcy_solve_gradient, saddle-point path on every handle, whose sol_out / adj_out / stats these are.  t is
 * given with the call: what pmc_darcy_set_transport or pmc_darcy_set_tracer attached is neither read nor changed.  k,
 * curve_bar (nbatch x nreport | NULL), stored_bar (nbatch | NULL; one of the two must be given), grad (nbatch x n_p), curve
 * (nbatch x nreport | NULL), stored (nbatch | NULL), sol_out and adj_out (| NULL) in `memspace`; status (nbatch) on the host.  A
 * column whose status is not PMC_TRANSPORT_OK has a zero gradient.
 * pmc_darcy_transport_loglik_gradient: loglik[b] = -|curve_b - data|^2 / (2 noise) (host) and its gradient, the seed
 * curve_bar = -(curve - data) / noise formed on the device; data (nreport), loglik, curve (| NULL) and status on the host.
 * Refused with PMC_ERR_INVALID: a level out of range, t NULL, of other sizes than the level (n_face != n_u or n_elem != n_p) or
 * created on another device, nbatch < 1, NULL k, grad, status or data, both seeds NULL, noise <= 0, a bad memspace. */
int pmc_darcy_transport_gradient(pmc_darcy* d, int level, pmc_transport* t, int nbatch, const double* k,
                                 const double* curve_bar, const double* stored_bar, int wrt_log, double* curve, double* stored,
                                 int32_t* status, double* grad, double* sol_out, double* adj_out, int memspace,
                                 pmc_stats* stats_fwd, pmc_stats* stats_adj);
int pmc_darcy_transport_loglik_gradient(pmc_darcy* d, int level, pmc_transport* t, int nbatch, const double* k,
                                        const double* data /* host, nreport */, double noise, int wrt_log, double* loglik /* host */,
                                        double* curve /* host, nbatch x nreport | NULL */, int32_t* status, double* grad, int memspace,
                                        pmc_stats* stats_adj);

/* ---- The adjoint of the particle tracer: gradients of travel times (an extension)
 * For J = <T_bar, T> + <x_exit_bar, x_exit> per column, pmc_tracer_run_adjoint returns u_bar = dJ/du (the first n_face entries
 * of the row at u_bar + b * ld_bar; nothing else of the row is written) and x0_bar = dJ/dx0 (nbatch x nparticles x 3, may be
 * NULL): the derivative of the walk above with its decisions held at their forward values - the element sequence and the
 * step count, the chosen exit of every step (for a box the side of its axis) and the series / closed-form branch of L and E.
 * Clamps count as the identity; a coordinate that the walk sets exactly (the exit plane, the entry face's barycentric
 * coordinate) has a zero derivative.  Seeds: T_bar (nbatch x nparticles), x_exit_bar (nbatch x nparticles x 3); each may be
 * NULL and then counts as zero, at least one must be given.  The forward outputs T, exit_face, nsteps (each may be NULL) and
 * status are those of pmc_tracer_run bit for bit.  A particle whose status is not PMC_TRACER_EXITED is not differentiated:
 * it adds nothing to u_bar and its x0_bar is zero (its T is a censored time so far).  All arrays in `memspace`.
 *   order:   u_bar[f] is summed from 0.0 over the (at most two) elements of face_elem[f] in that order and, within an element,
 *            over the visits of the column's particles in ascending (particle index in the caller's order, step).
 *   records: the sweep needs, per (column, particle, step), the element, the entry coordinates and the chosen exit; a second
 *            walk stores them, sized by the largest step count of the call, about (16 + 8 (n_c + n_fe)) bytes each (n_c = 3 |
 *            4 coordinates, n_fe = 6 | 4 faces).  Columns are processed in chunks whose records stay under 256 MiB (at least
 *            one column); pmc_tracer_set_adjoint_scratch sets another cap in bytes (0: the default) and
 *            pmc_tracer_adjoint_chunks returns the chunks of the last launch.  No result depends on the chunking.
 * A column's u_bar, x0_bar and forward outputs have the same bits at every nbatch, beside any other columns, in every split
 * into calls, in either memory space, at every ld / ld_bar, under any chunking and in repeated calls; pmc_tracer_run is not
 * disturbed.
 * pmc_tracer_reduce_seed: T_bar = dQ/dT of the Q of pmc_tracer_reduce, in `memspace` like T and status - PMC_TRACER_MEAN:
 * 1 / nparticles on the particles that exited, 0 elsewhere; PMC_TRACER_MIN: 1 on the lowest-index particle attaining the
 * minimum, if it exited, 0 elsewhere.
 * Refused with PMC_ERR_INVALID (nothing is written, the handle stays usable): both seeds NULL; NULL u, u_bar or status (T,
 * status or T_bar of the seed); ld or ld_bar < n_face; nbatch < 1; a bad memspace; a kind other than the two; bytes < 0. */
int pmc_tracer_run_adjoint(pmc_tracer* t, int nbatch, const double* u, int64_t ld,
                           const double* T_bar /* nbatch x nparticles | NULL */,
                           const double* x_exit_bar /* nbatch x nparticles x 3 | NULL; at least one seed */,
                           double* u_bar, int64_t ld_bar /* >= n_face; only the first n_face of each row written */,
                           double* x0_bar /* nbatch x nparticles x 3 | NULL */, double* T /* | NULL */,
                           int32_t* exit_face /* | NULL */, int32_t* status, int32_t* nsteps /* | NULL */, int memspace);
int pmc_tracer_reduce_seed(pmc_tracer* t, int nbatch, const double* T, const int32_t* status, int kind, double* T_bar,
                           int memspace);
int pmc_tracer_set_adjoint_scratch(pmc_tracer* t, int64_t bytes);   /* 0: 256 MiB */
int pmc_tracer_adjoint_chunks(const pmc_tracer* t);
/* dJ/dk (wrt_log: dJ/dlog k) of J = <T_bar, T> of the tracer t on the flux of the level's Darcy solution, per realization:
 * forward solve, the walk and its adjoint on the solver's internal solution, u_bar as the u rows of the adjoint right-hand
 * side (p rows and essential rows zero), adjoint solve, pmc_darcy_mass_sensitivity - the pipeline of
 * pmc_darcy_solve_gradient, saddle-point path on every handle, whose sol_out / adj_out / stats these are.  t is given with the
 * call: what pmc_darcy_set_tracer or pmc_darcy_set_transport attached is neither read nor changed.  k, T_bar (nbatch x
 * nparticles), grad (nbatch x n_p), T (nbatch x nparticles | NULL), status (nbatch x nparticles), sol_out and adj_out (| NULL)
 * in `memspace`.  Particles that did not exit add nothing to the gradient.
 * pmc_darcy_tracer_loglik_gradient: loglik[b] = -|T_b - data|^2 / (2 noise) over all particles (host) and its gradient, the
 * seed T_bar = -(T - data) / noise formed on the device; data (nparticles), loglik, T (| NULL) and not_exited (nbatch, the
 * particles of the column that did not exit) on the host.  A column with not_exited[b] > 0 has a zero gradient.
 * Refused with PMC_ERR_INVALID: a level out of range, t NULL, of other sizes than the level (n_face != n_u or n_elem != n_p) or
 * created on another device, nbatch < 1, NULL k, grad, T_bar, status, not_exited or data, noise <= 0, a bad memspace. */
int pmc_darcy_tracer_gradient(pmc_darcy* d, int level, pmc_tracer* t, int nbatch, const double* k,
                              const double* T_bar /* nbatch x nparticles */, int wrt_log, double* T,
                              int32_t* status /* nbatch x nparticles */, double* grad, double* sol_out, double* adj_out,
                              int memspace, pmc_stats* stats_fwd, pmc_stats* stats_adj);
int pmc_darcy_tracer_loglik_gradient(pmc_darcy* d, int level, pmc_tracer* t, int nbatch, const double* k,
                                     const double* data /* host, nparticles */, double noise, int wrt_log,
                                     double* loglik /* host */, double* T /* host | NULL */,
                                     int32_t* not_exited /* host, nbatch */, double* grad, int memspace, pmc_stats* stats_adj);

/* ---- MLMC accumulators across GPUs (new: the reference's manager is serial,
 *      src/MLMC_Manager.hpp:24) ----------------------------------------------------------- */
int pmc_comm_unique_id(void* id128);                                        /* 128 bytes    */
int pmc_comm_init(pmc_ctx* ctx, const void* id128, int nranks, int rank);   /* RCCL over xGMI */
int pmc_comm_destroy(pmc_ctx* ctx);
/* in-place SUM all-reduce of a small host buffer (the nlevels x 9 sums table + counts) */
int pmc_allreduce_sum_f64(pmc_ctx* ctx, double* host_buf, int n);

#ifdef __cplusplus
}
#endif
#endif /* PMC_H_ */

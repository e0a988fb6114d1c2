// Device-side objects behind the opaque C handles.
#pragma once
#include "chunks.hpp"
#include "solver.hpp"

namespace pmc {

HostCsr schur_host(const HostCsr& B, const HostCsr& Bt, const std::vector<double>& dM, const double* diag_add);
// device V-cycle hierarchy (shared values) from a host smoothed-aggregation hierarchy of diag(w) + K
std::unique_ptr<Multigrid> build_sa_chain(const HostCsr& K, const std::vector<double>& w, const pmc_solver_opts& o,
                                          hipStream_t st);

// inv = S^-1 (dense, row-major, exactly symmetric) of a small SPD operator by Cholesky; false when S is not numerically SPD
bool spd_dense_inverse(const HostCsr& S, std::vector<double>& inv);

struct Conditioner;

struct SamplerLevel {
    double ratio_M = 8.0;            // Chebyshev interval lambda_max/lambda_min of the l1-scaled M-block
    int n_u = 0, n_s = 0;
    int64_t nnz = 0;
    Sell A;                 // [M Bt; B -aW]
    Sell M;
    DevBuf<double> dinvM;   // 1 / l1 row sums of M
    DevBuf<double> M_scaled; // M D^-1 on M's SELL pattern
    DevBuf<double> w_sqrt;
    int proj = PMC_PROJ_NONE;
    int out_size = 0;
    Sell Gt;
    DevBuf<int> gather;
    DevBuf<double> inv_w;
    HostCsr P_host;         // ComputeTrueP(sform) as handed over (MLSampler::GetTrueP); empty on the last level
    // hybridized sampler (Sampler::hybrid): A = H on the multipliers (n_u = n_lambda), rhs = Gz (z f), s = z f - Gl lambda
    Sell Gz;                // G diag(1 / z): n_lambda x n_s
    Sell Gl;                // G^T: n_s x n_lambda
    Sell Ptz;               // diag(z) P^T of the next finer level: restriction of a finer xi that lands on z f directly
    DevBuf<double> zw_sqrt; // z .* sqrt(w)
    // internal numbering of the multipliers (aggregates of the V-cycle's finest level contiguous, agg_pack_rows): internal
    // row i is the caller's row lam_new2old[i]; empty = the caller's numbering
    DevBuf<int> lam_new2old, lam_old2new;
    std::vector<int> lam_n2o_host;   // lam_new2old on the host (setup export of the V-cycle's finest prolongator)
    // Adjoint of Eval (sampler_adjoint.hip), built at the first pmc_sampler_eval_adjoint of the level
    // from gather / Gt / inv_w / zw_sqrt / w_sqrt read back from the device: adj_Ot = (output map)^T as a SELL matrix (n_s x
    // out_size: the gather's 0/1 matrix or Gt^T diag(inv_w); on a hybridized handle its rows times z) and, on a hybridized
    // handle, z alone (the solve's right-hand side is Gz (z q); setup keeps z only folded into zw_sqrt and Ptz)
    bool has_adj = false;
    Sell adj_Ot;
    DevBuf<double> adj_z;
};

// evaluations (launches of one batch) of this process whose back-substitution wrote the field sample-major itself
// (k::residual_samples) instead of the interleaved field and its k::deinterleave (all handles, all threads)
uint64_t fused_field_eval_count();

struct Sampler {
    Ctx& ctx;
    int nlevels, n_mc;
    double alpha, g;
    bool lognormal;
    pmc_solver_opts opts;
    std::vector<SamplerLevel> lv;
    Multigrid mg;                                  // caller's levels: transfers between MC levels + geometric V-cycle
    std::vector<std::unique_ptr<Multigrid>> amg;   // per MC level: internal smoothed-aggregation hierarchy (if selected)
    double anisotropy = 1.0;
    bool hybrid = false;                           // pmc_sampler_create_hybrid: multiplier system, amg[l] its V-cycle
    // pmc_sampler_create_kl (kl.hip): truncated Karhunen-Loeve expansion, no linear system.  kl_phi[l] = Phi_l diag(sqrt(lambda)),
    // column-major n_s x kl_m (Phi_0 as handed over, the coarser levels projected on the device at create)
    bool kl = false;
    int kl_m = 0;
    std::vector<DevBuf<double>> kl_phi;
    // pmc_sampler_set_conditioner (condition.hip): when set, Eval conditions its Gaussian field before the output map (the
    // exp() of a lognormal handle then happens in the conditioner's store); embed_s_out keeps the prior field
    Conditioner* cond = nullptr;
    // set by eval_tangent around its Eval when the conditioner has derivatives enabled: the hook then applies the
    // homogeneous map (y = 0), its kernel chosen by the width of the whole call (0 outside such a call)
    int cond_tangent_width = 0;
    // ComputeL2Error / ComputeMaxError (field_stats.hip): diag(W) of level 0 as handed over, and the hierarchy of the output
    // space of the embedded / L2-projected variants (pmc_sampler_set_output_hierarchy: out_P[l] maps sample_size(l + 1) ->
    // sample_size(l), out_w0 the P0 mass of the original mesh's level 0; empty = not set)
    std::vector<double> w0_host;
    std::vector<HostCsr> out_P;
    std::vector<double> out_w0;
    // device copies of the two chains (the handle's own uploaded at the first error call, the output one by the setter)
    struct ErrChain {
        std::vector<int> nrows, ncols;
        std::vector<DevBuf<int>> rp, ci;
        std::vector<DevBuf<double>> v;
        DevBuf<double> w0;
        bool ready = false;
        void upload(const std::vector<const HostCsr*>& P, const std::vector<double>& w, hipStream_t st);
    };
    ErrChain err_own, err_out;
    OpTimer vc_timer;                              // hybrid: the finest level's post-smoothing launches (with work.op_timer.on)
    MinresWork work;
    DevBuf<double> rhs, sol, tA, tB, cx, cd, cx2, stage_in, stage_out, stage_emb, mini_scratch;
    DevBuf<pmc_stats> mini_stats;
    DevBuf<double> adj_part;                       // KL handles: partials of the adjoint's split reduction (kl_adjoint.hip)
    DevBuf<double> adj_lp;                         // prior_gradient: -|xi_b|^2 / 2 per realization

    Sampler(Ctx& c, int nlevels, int n_mc, const pmc_sampler_level* in, double alpha, double g, bool lognormal,
            const pmc_solver_opts& o);
    Sampler(Ctx& c, int nlevels, const pmc_hybrid_level* in, double alpha, double g, bool lognormal, const pmc_solver_opts& o);
    Sampler(Ctx& c, int nlevels, const pmc_kl_level* in, int nmodes, const double* evals, const double* evect0, bool lognormal);
    // rows of the vectors the Krylov solver of `level` iterates on
    // algorithmic bytes of one launch of the timed post-smoothing kernel (level 0 of the hybrid V-cycle of `level`)
    double smoother_bytes(int level, int nb) const;
    // setup values / prolongator of level `vlevel` of the V-cycle `level`'s solves run (pmc_sampler_vcycle_level / _prolongator)
    void vcycle_level(int level, int vlevel, int* nvlevels, double* info) const;
    const HostCsr& vcycle_prolongator(int level, int vlevel, HostCsr& scratch) const;
    // sizes and kernel-selection flags of that level (pmc_sampler_vcycle_info)
    void vcycle_info(int level, int vlevel, int* nvlevels, int64_t* info) const;
    size_t system_rows(int level) const { return hybrid ? (size_t)lv[level].n_u : (size_t)lv[level].n_u + lv[level].n_s; }
    void set_projection(int level, int kind, const pmc_csr* Gt, const int32_t* idx, const double* inv_w, int orig_size);
    void sample(int level, uint64_t first_id, int nbatch, double* xi, int memspace);
    void eval(int level, int xi_level, int nbatch, const double* xi, double* s_out, const double* init_s, int init_level,
              bool use_init, double* emb_out, int memspace, pmc_stats* stats);
    // dJ/dxi = (d Eval / d xi)^T v (pmc_sampler_eval_adjoint): v, s_out nbatch x sample_size(level), grad_xi nbatch x
    // xi_size(xi_level), sample-major; s_out (lognormal handles, may be NULL) multiplies v
    void eval_adjoint(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* grad_xi, int memspace,
                      pmc_stats* stats);
    // ds_out = (d Eval / d xi) v (pmc_sampler_eval_tangent): Eval of v without exp(), times s_out (lognormal handles, may be
    // NULL); v nbatch x xi_size(xi_level), s_out / ds_out nbatch x sample_size(level)
    void eval_tangent(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* ds_out, int memspace,
                      pmc_stats* stats);
    // the white-noise prior's part of a log-posterior gradient (pmc_sampler_logprior_gradient): grad -= xi in place (nbatch x
    // n, `memspace`), logprior[b] = -|xi_b|^2 / 2 (host, may be NULL)
    void prior_gradient(int n, int nbatch, const double* xi, double* grad, double* logprior, int memspace);
    // ... and of a Hessian action of -log pi (pmc_sampler_logprior_hessvec): hv += v in place (nbatch x n, `memspace`)
    void prior_hessvec(int n, int nbatch, const double* v, double* hv, int memspace);
    void apply_operator(int level, int nb, const double* x, double* y, int memspace, int repeat, double* avg_ms,
                        double* bytes);
    // invA[level]->Mult(rhs, sol) on full vectors of n_u + n_s entries per realization (sample-major)
    void mult(int level, int nbatch, const double* rhs, double* sol, bool use_guess, int memspace, pmc_stats* stats);
    // z = B^-1 r: one application of the MINRES preconditioner (diagnostics: true preconditioned residual norms)
    void apply_preconditioner(int level, int nbatch, const double* r, double* z, int memspace);

    void set_output_hierarchy(int nlev, const pmc_csr* P_orig, const double* w0_orig);
    // err[c] of nbatch fields of sample_size(level) entries (coeff, err in `memspace`): the squared L2 distance to `exact`
    // after prolongation to level 0 (max_err false) or max(max c - exact, exact - min c) (max_err true)
    void field_error(int level, int nbatch, const double* coeff, double exact, double* err, int memspace, bool max_err);
    // realizations of `level` one launch carries (pmc_sampler_batch_width)
    int launch_width(int level) const;

  private:
    CycleHierarchy cycle_hierarchy(int level) const;
    void ensure(int level, int nb);
    // rhs (hybridized solver): the kernel that would write the multiplier right-hand side, handed to the solve (RhsFn)
    // key_salt != 0: a solver configuration (graph key) apart from Eval's with the same level / width / rows
    void solve_system(int level, int nb, bool zero_guess, int x_row0, int x_nrows, pmc_stats* stats, const RhsFn* rhs = nullptr,
                      uint64_t key_salt = 0);
    PrecFn preconditioner(int level, int nb);
    // ... that hierarchy for the solves themselves, which set per-solve state on it (the handle's own amg[level] or mg)
    Multigrid& cycle_mg(int level) { return const_cast<Multigrid&>(cycle_hierarchy(level).g); }
    int degree_M(int level) const;
    const double* level_walk(int nb, int from, int to, const double* src, double* dst, const Sell* last = nullptr);
    RhsFn multiplier_rhs(int level, const double* fz);
    void eval_chunk(int level, int xi_level, int nb, const double* xi_d, double* s_d, const double* init_d,
                    int init_level, bool use_init, double* emb_d, pmc_stats* stats);
    // Eval of a KL handle: every realization in one launch
    void eval_kl(int level, int xi_level, int nbatch, const double* xi, double* s_out, double* emb_out, int memspace,
                 pmc_stats* stats);
    // sampler_adjoint.hip / kl_adjoint.hip
    void ensure_adjoint(int level);
    void eval_adjoint_chunk(int level, int xi_level, int nb, const double* v_d, const double* s_d, double* grad_d,
                            pmc_stats* stats);
    void eval_adjoint_kl(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* grad_xi,
                         int memspace, pmc_stats* stats);
};

// Conditioning on linear observations of the Gaussian field (condition.hip, pmc_conditioner_*): per
// Monte Carlo level H_l (CSR), K_l = C_l H_l^T and A_l^-1 on the device.  K_l is column-major with leading dimension ld (n
// rounded up to 16) and mp columns (nobs rounded up to 16, the padding zero).
constexpr int kCondMaxObs = 512;
struct Conditioner {
    Sampler& smp;
    int nobs, mp;
    bool noisy = false;               // some sigma2 > 0: apply needs zeta
    struct Level {
        int n = 0, ld = 0;
        HostCsr H;
        DevBuf<int> hrp, hci;
        DevBuf<double> hv, K, Ainv;
        std::vector<double> A;        // nobs x nobs, as inverted
        // H_l^T in compressed-column form, the touched columns only (the adjoint's correction): column tcol[q] holds the
        // entries tptr[q] .. tptr[q + 1], (trow, tval) in ascending row order
        int tcols = 0;
        DevBuf<int> tcol, tptr, trow;
        DevBuf<double> tval;
    };
    std::vector<Level> lv;
    DevBuf<double> y, sqrt_sigma2, coef, stage_g, stage_z;
    // derivatives of the map: partials of the adjoint's split reduction, the staging of a host call's
    // s_out and result, and w = Gamma^T (v o f') of the EvalAdjoint hook; grown at the first use, never shrunk
    DevBuf<double> adj_part, stage_s, stage_w, hook_w;
    bool derivs = false;              // pmc_conditioner_enable_derivatives
    Conditioner(Sampler& s, int nobs, const pmc_csr* H0, const double* y, const double* sigma2);
    ~Conditioner() { if (smp.cond == this) smp.cond = nullptr; }
    // out = f(g + K_l A_l^-1 (y + sqrt(sigma2) zeta - H_l g)), f = exp or the identity; out may alias g
    void apply(int level, int nbatch, const double* g, const double* zeta, double* out, bool apply_exp, int memspace);
    // the same on device arrays, enqueued on the handle's stream (the Eval hook).  homogeneous: y = 0 and no noise, the linear
    // part of the map (its tangent); call_width: the realizations of the CALL this launch is a piece of (0 = nbatch) - more
    // than 4 select the MFMA kernel
    void apply_device(int level, int nbatch, const double* g_d, const double* zeta_d, double* out_d, bool apply_exp,
                      bool homogeneous = false, int call_width = 0);
    // out = f' o (dg - K_l A_l^-1 H_l dg), f' = s_out or 1; out may alias dg
    void apply_tangent(int level, int nbatch, const double* dg, const double* s_out, double* out, int memspace);
    // out = u - H_l^T A_l^-1 K_l^T u, u = v o s_out (s_out may be NULL); out aliases neither v nor s_out
    void apply_adjoint(int level, int nbatch, const double* v, const double* s_out, double* out, int memspace);
    // the same on device arrays, enqueued on the handle's stream (the EvalAdjoint hook); call_width as for apply_device
    void apply_adjoint_device(int level, int nbatch, const double* v_d, const double* s_d, double* out_d, int call_width = 0);
    void export_level(int level, int* n, int64_t* nnz, double* K, double* A, int32_t* rowptr, int32_t* colind,
                      double* vals) const;

  private:
    void build_K_solves(int level);
    void build_K_kl(int level);
};

// Accumulators of one sampler level's output (field_stats.hip, pmc_field_stats_*): (sum, compensation) pairs of s, s^2 and
// <chi, s> s per element, in device memory between calls
struct FieldStats {
    Sampler& smp;
    int level, n;
    bool has_chi;
    int64_t count = 0;
    DevBuf<double> chi, acc, dots, part, xi, sbuf;
    FieldStats(Sampler& s, int level, const double* chi, int memspace);
    void reset();
    void accumulate(int nbatch, const double* s, int memspace);
    void run(uint64_t first_id, int64_t nsamples);
    void read(double* expectation, double* second_moment, double* chi_cov, int64_t* count, int memspace);
    void read_sums(double* sums, int64_t* count, int memspace);
    void chi_dots(int nbatch, const double* s, double* out, int memspace);

  private:
    void check_size() const;
    void accumulate_device(int nbatch, const double* s_d);
};

// Accumulators of one Darcy level's pressure for the multilevel field estimates (level_fields.hip, pmc_level_fields_*):
// (sum, compensation) pairs of d = p - p_c[parent], d^2 and p^2 - p_c[parent]^2 per element (p_c = 0 without a coarse
// partner), added in ascending realization id; work on ctx's stream
struct Darcy;
struct LevelFields {
    Ctx& ctx;
    int level, n, nc;              // n_p(level), n_p(level + 1) (0 when not coupled)
    bool coupled;
    int64_t count = 0;
    std::vector<int> parent_host;  // parent[i]: the coarse element of fine element i (coupled only)
    DevBuf<int> parent;
    DevBuf<double> acc, pbuf, cbuf;
    LevelFields(Ctx& c, const Darcy& d, int level, bool coupled);
    void reset();
    void accumulate(int nbatch, const double* p_fine, const double* p_coarse, int memspace);
    // per-column weights (host arrays of nbatch): w_fine[b] p_fine - w_coarse[b] p_coarse[parent]
    void accumulate_weighted(int nbatch, const double* p_fine, const double* w_fine, const double* p_coarse,
                             const double* w_coarse, int memspace);
    void read_sums(double* sums, int64_t* count, int memspace);

  private:
    void accumulate_device(int nbatch, const double* pf, const double* pc);
    void accumulate_weighted_device(int nbatch, const double* pf, const double* wf, const double* pc, const double* wc);
};

// kl_eigs.hip: the Matern covariance operator K = W^1/2 C W^1/2 applied matrix-free (Y = K X, host pointers, column-major
// n x ncols) and its top eigenpairs by Chebyshev-filtered subspace iteration (pmc_kl_matern_apply / pmc_kl_matern_eigs).
// Both validate their arguments themselves and throw Error.
void kl_matern_apply(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int ncols,
                     const double* X, double* Y);
void kl_matern_eigs(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int nmodes,
                    const pmc_kl_eigs_opts* opts, double* evals, double* evect0, pmc_kl_eigs_info* info);

// kl.hip: s[b n + i] = sum_k phi[k n + i] xi[b n_xi + k] (exp() if lognormal, the Gaussian value to emb when non-NULL) for
// b < nb, i < n, k < m, in fp64 (MFMA for nb > 4, a bandwidth GEMV below); phi column-major n x m.
void kl_eval(hipStream_t st, int n, int m, int nb, const double* phi, const double* xi, int n_xi, double* s, double* emb,
             bool lognormal);
// kl_adjoint.hip: grad[b n_xi + k] = sum_i phi[k n + i] v[b n + i] (sv ? sv[b n + i] : 1) for k < m, 0 for m <= k < n_xi, in
// fp64 (MFMA for nb > 4, a bandwidth kernel below); part: kl_adjoint_partials(n, m, nb) doubles of scratch.  The reduction
// over i is split into chunks that depend on n alone and summed in a fixed order: column b has the same bits for every
// nb > 4 and every split of a call into pieces wider than 4 (narrower calls take the VALU kernel, whose bits may differ).
size_t kl_adjoint_partials(int n, int m, int nb);
// rows of one reduction chunk of a field of n rows (the conditioner's adjoint cuts its reduction by the same rule)
int kl_adjoint_chunk_rows(int n);
void kl_eval_adjoint(hipStream_t st, int n, int m, int nb, const double* phi, const double* v, const double* sv, int n_xi,
                     double* grad, double* part);

// Particle travel times on the RT0 flux (tracer.hip, pmc_tracer_*): per element one packed record
// (faces with the sign folded in, neighbours, porosity, geometry), the particles sorted by start element, and the output
// buffers of the hooked SolveFwd / the staging of host-memory callers.  Work on ctx's stream, except qoi_interleaved and
// adjoint_launch, which run on the stream the Darcy handle passes: a tracer serves one handle at a time.
struct Tracer {
    Ctx& ctx;
    int kind, n_elem, n_face, npart, max_steps = 0;
    DevBuf<char> recs;
    DevBuf<double> x0;
    DevBuf<int32_t> e0, orig;      // start elements in sorted order; orig[p]: the caller's index of sorted particle p
    DevBuf<double> out_T, out_x, stage_u, red_T, q;
    DevBuf<int32_t> out_i, red_s, nex;
    Tracer(Ctx& c, const pmc_tracer_mesh& m, int nparticles, const double* x0, const int32_t* elem0, int max_steps);
    static int default_max_steps(int n_elem);      // 64 + 32 ceil(cbrt(n_elem))
    void run(int nbatch, const double* u, int64_t ld, double* T, int32_t* exit_face, int32_t* status, int32_t* nsteps,
             double* x_exit, int memspace);
    void reduce(int nbatch, const double* T, const int32_t* status, int kind, double* Q, int32_t* not_exited, int memspace);
    // Q of a launch of the Darcy solver: walk on its interleaved solution sol[row * nb + col], reduce into q_d (device, nb)
    void qoi_interleaved(hipStream_t st, int nb, const double* sol, int kind, double* q_d);
    // the adjoint (pmc_tracer_run_adjoint): per face its elements, local faces and signs; the records
    // of a launch - per (step, thread) the element, the chosen exit, the entry coordinates, the adjoints of the outward
    // fluxes and the link of the element's visit list - the list heads per (element, column), and the staging of a host
    // call.  Scratch of its own: a pmc_tracer_run after an adjoint call finds its buffers as it left them.
    DevBuf<int32_t> side, adj_elem, adj_code, adj_link, adj_head, adj_i;
    DevBuf<double> adj_c, adj_fbar, adj_T, adj_stage_u, adj_stage_ubar, adj_stage_tb, adj_stage_xb, adj_stage_x0b, seed_tb;
    std::vector<int32_t> h_steps;
    int64_t adj_cap = 0;           // bytes of records per chunk of columns (pmc_tracer_set_adjoint_scratch); 0: 256 MiB
    int adj_chunks = 0;            // column chunks of the last adjoint_launch
    void run_adjoint(int nbatch, const double* u, int64_t ld, const double* T_bar, const double* x_exit_bar, double* u_bar,
                     int64_t ld_bar, double* x0_bar, double* T, int32_t* exit_face, int32_t* status, int32_t* nsteps, int memspace);
    void reduce_seed(int nbatch, const double* T, const int32_t* status, int kind, double* T_bar, int memspace);
    void set_adjoint_scratch(int64_t bytes);
    // nb columns on stream st, the flux read through (stride_face, stride_batch): the forward outputs (device, nb x npart,
    // the caller's particle order), u_bar written through (stride_face_out, stride_batch_out), x0_bar (nb x npart x 3 | NULL)
    // from the seeds (device, sample-major, each may be NULL)
    void adjoint_launch(hipStream_t st, int nb, bool by_batch, const double* u_d, int64_t stride_face, int64_t stride_batch,
                        const double* Tbar_d, const double* xbar_d, double* ubar_d, int64_t stride_face_out,
                        int64_t stride_batch_out, double* x0bar_d, double* T_d, int32_t* face_d, int32_t* status_d,
                        int32_t* steps_d, const double* data_d = nullptr, double noise = 1.0);
    // T_bar = -(T - data) / noise, zero on the columns with nex > 0, into seed_tb (data: device, npart); returns seed_tb.p.
    // adjoint_launch forms it after its walk when data_d is given (Tbar_d is then ignored) and leaves the counts in nex.
    const double* loglik_seed(hipStream_t st, int nb, const double* T_d, const double* data_d, double noise);

  private:
    void launch_walk(hipStream_t st, int nb, bool by_batch, const double* u_d, int64_t stride_face, int64_t stride_batch,
                     double* T_d, int32_t* face_d, int32_t* status_d, int32_t* steps_d, double* x_d);
    void launch_reduce(hipStream_t st, int nb, const double* T_d, const int32_t* status_d, int kind, double* q_d,
                       int32_t* nex_d);
};

// Upwind transport of a passive solute on the Darcy flux (transport.hip, pmc_transport_*): the rows of
// B packed as (dof with the sign folded in, neighbour element) pairs, one magnitude per dof, and the scratch of a call - two
// concentration buffers, the outlet accumulators and their snapshots at the report times.  Work on ctx's stream, except
// qoi_interleaved, which runs on the stream of the Darcy handle it is attached to: attach it to one handle at a time.
struct Transport {
    Ctx& ctx;
    int n_elem, n_face, n_outlet = 0, nreport, max_steps = 0;
    int width = 0;                 // 3 | 4 | 6: every row has that many entries (register form); 0: the general form
    double t_end, cfl;
    DevBuf<int32_t> rec, rowptr;
    DevBuf<double> a, cin, vol, c0, wgt;
    DevBuf<double> cbuf, acc, snap, col_rate, col_dt, stage_u, out_c, out_curve, out_stored;
    DevBuf<int32_t> col_steps;
    std::vector<double> h_rate, h_dt, h_treached;   // the plan of the last launch, per column
    std::vector<int32_t> h_steps, h_status, h_steps_adj;
    // the adjoint (pmc_transport_run_adjoint): per dof its one or two elements and its outlet index;
    // the checkpoints, one recomputed segment, the final states, the (lam, w lam) pairs, beta per (step, column), the time
    // sums P, X, O and the branch of r_e; the staging of a host call.  Scratch of their own: a pmc_transport_run after an
    // adjoint call finds its buffers as it left them.
    DevBuf<int32_t> side, col_steps_adj;
    DevBuf<double> adj_ck, adj_seg, adj_tmp, adj_fin, adj_lam, adj_wlam, adj_beta, adj_P, adj_X, adj_O;
    DevBuf<unsigned char> adj_sig;
    DevBuf<double> stage_cb, stage_sb, stage_eb, stage_ubar, stage_c0bar, seed_cb;
    int adj_segment = 0;           // K of pmc_transport_set_adjoint_segment; 0: ceil(sqrt(longest step count))
    int adj_K = 1, adj_nck = 1, adj_longest = 0, adj_longest_fwd = 0;   // of the last adjoint_forward
    Transport(Ctx& c, const pmc_transport_mesh& m, const pmc_transport_params& p);
    void run_adjoint(int nbatch, const double* u, int64_t ld, const double* curve_bar, const double* stored_bar, const double* c_bar,
                     double* u_bar, int64_t ld_bar, double* c0_bar, double* curve, double* stored, int32_t* nsteps, int32_t* status,
                     int memspace);
    void set_adjoint_segment(int K);
    // The two halves of an adjoint launch of nb columns on stream st, the flux read through (stride_face, stride_batch):
    // the forward pass with checkpoints (curve_d nb x nreport, stored_d nb; the plan in h_*), then the sweep from the
    // seeds (device, sample-major, each may be NULL) to u_bar, written through (stride_face_out, stride_batch_out), and
    // c0_bar (nb x n_elem, may be NULL).  Columns whose status is not PMC_TRANSPORT_OK get zeros.
    void adjoint_forward(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch, double* curve_d,
                         double* stored_d);
    void adjoint_backward(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch,
                          const double* curve_bar_d, const double* stored_bar_d, const double* c_bar_d, double* ubar_d,
                          int64_t stride_face_out, int64_t stride_batch_out, double* c0_bar_d);
    // curve_bar = -(curve - data) / noise into seed_cb (data: device, nreport); returns seed_cb.p
    const double* loglik_seed(hipStream_t st, int nb, const double* curve_d, const double* data_d, double noise);
    void run(int nbatch, const double* u, int64_t ld, double* c_out, double* curve, double* stored, double* rate,
             double* t_reached, int32_t* nsteps, int32_t* status, int memspace);
    void reduce(int nbatch, const double* curve, const double* stored, int kind, double* Q, int memspace);
    // Q of a launch of the Darcy solver: the transport on its interleaved solution sol[row * nb + col] into q_d (device, nb)
    void qoi_interleaved(hipStream_t st, int nb, const double* sol, int kind, double* q_d);

  private:
    int nnz_ = 0;
    template <class F>
    void by_width(F&& launch) const;   // transport.hip only
    int plan_columns(hipStream_t st, int nb, const double* q_d);
    void compute(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch, double* curve_d,
                 double* stored_d, int kind, double* q_d);
};

struct DarcyLevel {
    int n_u = 0, n_p = 0, n_coef = 0;
    double ratio_M = 8.0;            // Chebyshev interval of the l1-scaled M-block (from M(k == 1) unless given)
    int64_t nnz = 0;
    Sell M;                          // pattern only; values are per-realization
    DevBuf<int> slot_src, c_ptr, c_elem;
    DevBuf<double> c_val;
    // element-grouped form of M(k) (EgView): shared element-matrix entries + two coefficient rows per dof; when present
    // (every dof belongs to at most two elements) the solve never materialises per-realization values of M
    Sell Meg;
    DevBuf<int> eg_e12;
    int eg_gw = 0;
    bool has_eg = false;
    Sell B, Bt;                      // shared +-1 values (essential columns/rows removed)
    DevBuf<unsigned char> ess;
    DevBuf<double> ess_data, rhs_u0, rhs_p, obs;
    // Schur complement refresh: S(k) = B diag(M(k))^-1 B^T on the fixed pattern of mg.L[level].S
    DevBuf<int> s_ptr, s_idx;        // per SELL slot of S: faces contributing
    DevBuf<double> s_w;
    DevBuf<int> s_diag_slot;         // per row: SELL slot of the diagonal entry
    // Galerkin coarse operator refresh: S_{l+1} = 1/2 P^T S_l P (lists of fine SELL slots per coarse slot)
    DevBuf<int> g_ptr, g_idx;
    DevBuf<double> g_w;
    // per-realization values
    DevBuf<double> coef, mvals, mvals_scaled, diagM, l1invM, rhs_bc;
    // support of the observation functional (rows with obs != 0) and its weights: when the caller does not ask for
    // the solution vector, MINRES only maintains these rows of it
    DevBuf<int> obs_rows;
    DevBuf<double> obs_w;
    int n_obs = 0;
    // Bayesian observation functionals g_i (src/BayesianInverseProblem.cpp:178-186): rows of Gobs act on the pressure
    // block.  MINRES then maintains the union of supp(obs) and supp(g_i); Gobs is stored on that compact numbering.
    int n_gobs = 0, n_grows = 0;
    Sell Gobs;
    DevBuf<int> g_rows;
    DevBuf<double> g_obs_w, g_norm;
    // Adjoint gradients (darcy_gradient.hip), built at the first gradient call of the level: per
    // element its faces and the dense unit-coefficient matrix M_e, element-major in slices of 64 elements, column-major
    // inside a slice - faces [slice][a][64], M_e [slice][a n_fe + a'][64]
    bool has_grad = false;
    int grad_nfe = 0, grad_nslices = 0;
    DevBuf<int> grad_faces;
    DevBuf<double> grad_me;
    // ... and, from the first tangent / Hessian call on (darcy_hessian.hip), the same data face-major
    // in slices of 64 faces: per face its tan_nside elements in ascending order (-1: none), and per side the element's
    // faces and the row of M_e that belongs to the face - tan_elem [slice][s][64], tan_cols / tan_w [slice][s n_fe + a'][64]
    bool has_tan = false;
    int tan_nside = 0, tan_nslices = 0;
    DevBuf<int> tan_elem, tan_cols;
    DevBuf<double> tan_w;
    // the observation functionals as handed over and, for the log-likelihood gradient, diag(1 / sum g_i) Gobs transposed
    // (CSR over the elements, uploaded at the first pmc_darcy_loglik_gradient after a set_observations)
    HostCsr Gobs_host;
    bool has_gt = false;
    DevBuf<int> gt_ptr, gt_obs;
    DevBuf<double> gt_val;
};

// Internal algebraic hierarchy of one Monte Carlo level (mg_coarsening): smoothed-aggregation prolongators frozen at
// k == 1, operators S_0(k) = B diag(M(k))^-1 B^T and S_{j+1}(k) = P_j^T S_j(k) P_j refreshed per realization on fixed
// patterns through contribution lists (the same refresh kernel as the geometric hierarchy).
struct DarcyChainLevel {
    DevBuf<int> ptr, idx, diag_slot;   // per SELL slot: list into diag(M) (level 0, reciprocal) or the finer level's slots
    DevBuf<double> w;
};
struct DarcyChain {
    Multigrid mg;
    std::vector<DarcyChainLevel> cl;
    double galerkin_scale = 1.0;       // S_{j+1}(k) = galerkin_scale P_j^T S_j(k) P_j (folded into the refresh weights)
};

// Hybridized form of one Monte Carlo level (pmc_darcy_create_hybrid: the reference's "Hybridization" branch of DarcySolver,
// src/DarcySolver.cpp:586,619; algebra: parelagmc_amd/fe/darcy_hybrid.py).  One multiplier per interior / essential face,
//     H(kappa) lambda = R kappa + b_0,     H(kappa) = sum_e kappa_e C_e X_e C_e^T     (kappa = 1 / c(k), SPD, linear in kappa)
//     u = kappa_owner (U_0 - U_L lambda) + u_g,     p = P_0 - P_L lambda - z_g / kappa.
// chain: level 0 holds H(kappa) on its fixed pattern through contribution lists over the coefficient table, the coarser
// levels the OVER-CORRECTED Galerkin products s P^T H P of a plain-aggregation hierarchy frozen at kappa == 1 (LAB_NOTES
// 10.15: s = 0.5 makes the iteration count nearly level-independent), all refreshed per realization.
struct DarcyHybrid {
    int n_lambda = 0;
    std::unique_ptr<DarcyChain> chain;
    Sell R, UL, PL;
    // element-grouped form of H(kappa) (EgView, as DarcyLevel::Meg for M(k)): the operator of the MINRES loop never reads the
    // explicit per-realization values of level 0 (1.1 GB per pass at 0.8 M multipliers x 16)
    Sell Heg;
    DevBuf<int> eg_e12, no_rows;       // no_rows: slice offsets of an operator without entries (the kernel's second operand)
    int eg_gw = 0;
    DevBuf<double> b0, U0, ug, P0, zg;
    DevBuf<int> owner;
    DevBuf<double> coef, rhs, lam, tu, tp;     // per launch: kappa [n_p][nb], right-hand side, multipliers, U_L lambda, P_L lambda
    // finest level of the V-cycle in element-grouped form (solve_chunk_hybrid): -kappa (the residual r - H x is ONE launch of
    // the operator kernel with the negated coefficients and the identity as its second operand), iterate, residual, update
    Sell ident;
    DevBuf<double> negcoef, vx, vres, vd, vxc;
};

struct Darcy {
    Ctx& ctx;
    int nlevels, n_mc;
    bool k_divides;
    bool hybrid = false;             // SolveFwd through the hybridized form (ComputeG keeps the saddle-point path)
    std::vector<std::unique_ptr<DarcyHybrid>> hyb;   // per MC level
    pmc_solver_opts opts;
    std::vector<DarcyLevel> lv;
    Multigrid mg;                    // batched values
    std::vector<std::unique_ptr<DarcyChain>> chains;   // per MC level, empty unless algebraic coarsening is selected
    double anisotropy = 1.0;
    DevBuf<double> gwork;
    MinresWork work;
    // in-loop timing of the dominant kernel of the Darcy operator: the u-rows [M(k) | B^T] (k::eg_pair_spmm with the fused
    // <x, Ax>; k::pair_spmm when the element-grouped form is not available)
    OpTimer op_timer;
    double operator_bytes(int level, int nb) const;   // algorithmic bytes of ONE such launch
    // ... and of the M-block polynomial of the preconditioner (k::eg_poly2, the other large gather kernel of an iteration):
    // timed on the same switch, on the main stream instead of beside the V-cycle's bottom
    OpTimer poly_timer;
    double poly_bytes(int level, int nb) const;
    // ... and of the gradient's mass-sensitivity kernel (darcy_gradient.hip), on the same switch
    OpTimer grad_timer;
    double mass_sensitivity_bytes(int level, int nb);   // builds the level's gradient data when it is not there yet
    // ... and of the tangent right-hand side kernel (darcy_hessian.hip), on the same switch
    OpTimer tan_timer;
    double mass_tangent_bytes(int level, int nb);       // builds the level's face-major data when it is not there yet
    DevBuf<double> sol, sol_compact, cx, cd, cx2, stage_k, stage_sol, qpartial, qout, gtmp, gout;
    // adjoint solve (darcy_gradient.hip): right-hand side and second full solution, host staging (stage_out: the adjoint
    // solution on its way out); allocated at first use
    DevBuf<double> adj_rhs, adj_sol, stage_adj, stage_grad, stage_out, obs_data;
    // tangent solve (darcy_hessian.hip): third full solution, host staging of the direction; allocated at first use
    DevBuf<double> tan_sol, stage_dk;
    // travel-time QoI (pmc_darcy_set_tracer): with a tracer on a level, the Q of solve_fwd there is the tracer's reduction of
    // the particles' travel times on the solve's flux block instead of <obs, x>.  compute_G, the gradients and the Hessian
    // actions keep <obs, x>.  Not owned.
    std::vector<Tracer*> tracers;
    std::vector<int> tracer_kind;
    void set_tracer(int level, Tracer* t, int kind);
    Tracer* tracer_of(int level) const { return level < (int)tracers.size() ? tracers[level] : nullptr; }
    // solute-transport QoI (pmc_darcy_set_transport): as the tracer's hook, with the mass that left through the outlet or the
    // mass in place as Q.  A level holds a tracer or a transport, not both.  Not owned.
    std::vector<Transport*> transports;
    std::vector<int> transport_kind;
    void set_transport(int level, Transport* t, int kind);
    Transport* transport_of(int level) const { return level < (int)transports.size() ? transports[level] : nullptr; }
    bool use_eg(const DarcyLevel& d) const;
    void set_observations(int level, const pmc_csr* Gobs);
    void compute_G(int level, int nbatch, const double* k, double* G, double* C, double* Q, int memspace, pmc_stats* stats);

    Darcy(Ctx& c, int nlevels, int n_mc, const pmc_darcy_level* in, bool k_divides, const pmc_solver_opts& o,
          bool hybrid = false);
    // sol_kind: 0 none, 1 full solution (n_u+n_p per realization), 2 pressure block only (n_p per realization)
    void solve_fwd(int level, int nbatch, const double* k, double* Q, double* C, double* sol_out, int memspace,
                   pmc_stats* stats, int sol_kind = 1);
    // one application of the MINRES preconditioner / operator of a launch of nbatch realizations with permeabilities k
    // (pmc_darcy_apply_preconditioner / _apply_operator): the same setup and the same closures as solve_fwd
    void apply_preconditioner(int level, int nbatch, const double* k, const double* r, double* z, int memspace);
    void apply_operator(int level, int nbatch, const double* k, const double* x, double* y, int memspace);
    // Adjoint gradients with respect to k (pmc_darcy_mass_sensitivity / _solve_gradient / _loglik_gradient,
    // darcy_gradient.hip).  All three take the saddle-point path, also on a hybridized handle (as compute_G).
    void mass_sensitivity(int level, int nbatch, const double* k, const double* x, const double* lam, bool wrt_log,
                          double* grad, int memspace);
    void solve_gradient(int level, int nbatch, const double* k, const double* adj_rhs, bool wrt_log, double* Q, double* C,
                        double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                        pmc_stats* stats_adj);
    void loglik_gradient(int level, int nbatch, const double* k, const double* data, double noise, bool wrt_log,
                         double* loglik, double* G, double* grad, int memspace, pmc_stats* stats_adj);
    // Gradients in k of the breakthrough data of a transport on the level's flux (pmc_darcy_transport_gradient /
    // _transport_loglik_gradient): gradient_chunk with the transport's adjoint in front of the adjoint
    // solve.  t is given with the call; what set_transport / set_tracer attached is neither read nor changed.
    void transport_gradient(int level, Transport* t, int nbatch, const double* k, const double* curve_bar, const double* stored_bar,
                            bool wrt_log, double* curve, double* stored, int32_t* status, double* grad, double* sol_out,
                            double* adj_out, int memspace, pmc_stats* stats_fwd, pmc_stats* stats_adj);
    // Gradients in k of the travel times of a tracer on the level's flux (pmc_darcy_tracer_gradient / _tracer_loglik_gradient;
    // DESIGN.md section 25): gradient_chunk with the tracer's adjoint in front of the adjoint solve.  t is given with the call.
    void tracer_gradient(int level, Tracer* t, int nbatch, const double* k, const double* T_bar, bool wrt_log, double* T,
                         int32_t* status, double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                         pmc_stats* stats_adj);
    void tracer_loglik_gradient(int level, Tracer* t, int nbatch, const double* k, const double* data, double noise, bool wrt_log,
                                double* loglik, double* T, int32_t* not_exited, double* grad, int memspace, pmc_stats* stats_adj);
    void transport_loglik_gradient(int level, Transport* t, int nbatch, const double* k, const double* data, double noise,
                                   bool wrt_log, double* loglik, double* curve, int32_t* status, double* grad, int memspace,
                                   pmc_stats* stats_adj);
    // Tangent right-hand side and Gauss-Newton Hessian action (pmc_darcy_mass_tangent / _gn_hessvec, darcy_hessian.hip);
    // the saddle-point path on every handle, as the gradients
    void mass_tangent(int level, int nbatch, const double* k, const double* x, const double* dk, bool wrt_log, double* t_out,
                      int memspace);
    void gn_hessvec(int level, int nbatch, const double* k, const double* x_in, const double* dk, double noise, bool wrt_log,
                    double* hv, double* dG, double* x_out, int memspace, pmc_stats* stats_tan, pmc_stats* stats_adj);
    // setup values of one level of the V-cycle `level`'s solves run (pmc_darcy_vcycle_level)
    void vcycle_level(int level, int vlevel, int* nvlevels, double* info) const;
    // P from V-cycle level vlevel + 1 to vlevel of that cycle (pmc_darcy_vcycle_prolongator), rows of vlevel 0 in the caller's
    // numbering
    const HostCsr& vcycle_prolongator(int level, int vlevel) const;
    // caller's hierarchy: S_{l+1}(k) = galerkin_scale P^T S_l(k) P
    double galerkin_scale = 0.5;
    // the pressure prolongators P_l (n_p(l) x n_p(l + 1)) as handed over, for the level accumulators (level_fields.hip)
    std::vector<HostCsr> P_host;

  private:
    CycleHierarchy cycle_hierarchy(int level) const;
    void ensure(int level, int nb);
    void setup_chunk(int level, int nb, const double* k_d);
    void chunk_ops(int level, int nb, bool timing_ok, LinOp& A, PrecFn& prec);
    // The launches of a batched entry: ChunkArg, Chunk and the driver are in chunks.hpp.  This forwards with the level's
    // launch width and a synchronisation behind every launch.
    void for_chunks(int level, int nbatch, int memspace, const std::vector<ChunkArg>& args, const std::function<void(const Chunk&)>& body) {
        pmc::for_chunks(ctx, batch_width((size_t)lv[level].n_u + lv[level].n_p, true, ctx.device), nbatch, memspace, true, args, body);
    }
    // One launch configuration for the saddle-point solves of a launch.  SolveMode is the last word of the key under which
    // a MINRES loop is captured and replayed as a graph: a solve finds its graph again only under the same level, width
    // and mode, and solves that share a mode (the forward solve of solve_fwd, gradient_chunk and gn_hessvec_chunk) share
    // the graph.
    enum SolveMode : uint64_t {
        kSolveObsRows = 1,     // forward solve that maintains only the rows in supp(obs) (solve_fwd without a solution)
        kSolveFull = 2,        // forward solve on all rows (solve_fwd with a solution, gradient_chunk, gn_hessvec_chunk)
        kSolveGRows = 3,       // forward solve that maintains the rows of the observation functionals (compute_G)
        kSolveAdjoint = 5,     // adjoint solve of gradient_chunk
        kSolveTangent = 6,     // tangent solve of gn_hessvec_chunk
        kSolveGnAdjoint = 7,   // Gauss-Newton adjoint solve of gn_hessvec_chunk
    };
    struct SaddleLaunch {
        LinOp A;
        PrecFn prec;
        uint64_t key0 = 0;     // level and width; the mode completes a key
        GraphHint hint;        // of the forward solve: right-hand side rhs_bc, the mode asked for
        // a further solve of the launch with the same operator and preconditioner
        GraphHint follow_up(SolveMode mode, const void* rhs, const void* x) const {
            return GraphHint{hash_mix(key0, mode), hash_ptr(hash_ptr(hint.sig, rhs), x)};
        }
    };
    // ensure, phase mark 0 (timed), setup_chunk, phase mark 1 (timed and setup_ends: "Build Solver" ends with the setup; a
    // caller whose setup phase goes on marks 1 itself), chunk_ops and the forward hint
    SaddleLaunch saddle_launch(int level, int nb, const double* k_d, SolveMode mode, bool timed, bool setup_ends);
    // behind a minres_solve: phase mark 2, the columns' results and the phase times into stats (NULL: none), the in-loop timers
    void solve_done(const MinresResult& res, int nb, pmc_stats* stats);
    void solve_chunk(int level, int nb, const double* k_d, double* Q_host, double* sol_d, pmc_stats* stats, int row0,
                     int nrows, double* G_host);
    void build_hybrid(int level, const pmc_darcy_level& L);
    bool hybrid_eg_cycle(int level) const;
    void ensure_hybrid(int level, int nb);
    void setup_chunk_hybrid(int level, int nb, const double* k_d);
    void hybrid_ops(int level, LinOp& A, PrecFn& prec);
    // one launch of the seams below: applies the preconditioner (true) or the operator to the [nb][rows] vectors in
    void apply_one(int level, int nb, const double* k, const double* in, double* out, int memspace, bool precond);
    void solve_chunk_hybrid(int level, int nb, const double* k_d, double* Q_host, double* sol_d, pmc_stats* stats, int row0,
                            int nrows);
    // darcy_gradient.hip.  gradient_chunk is one launch of every gradient entry; what differs between them is the adjoint
    // right-hand side, which the entry hands over as a callable: it runs once per launch behind the forward solve (st: the
    // stream, nb, the level) and leaves the right-hand side in adj_rhs, essential rows zero, from the solution in sol.
    // There are four, and an entry binds its own operands to one of them: rhs_seed (the caller's dJ/dx, or obs), rhs_loglik
    // (the observation functionals; also delivers G), rhs_transport and rhs_tracer (the adjoint of a transport / of a tracer
    // on the flux block, with given seeds or with data).  rhs_finish is their common end.
    using AdjointRhs = std::function<void(hipStream_t st, int nb, int level)>;
    void gradient_chunk(int level, int nb, const double* k_d, const AdjointRhs& form_rhs, bool wrt_log, double* Q_host,
                        double* grad_d, double* sol_d, double* adj_d, pmc_stats* stats_fwd, pmc_stats* stats_adj);
    void rhs_seed(hipStream_t st, int nb, int level, const double* rhs_d);
    void rhs_loglik(hipStream_t st, int nb, int level, const double* data, double noise, double* G_host);
    void rhs_transport(hipStream_t st, int nb, int level, Transport& T, const double* curve_bar_d, const double* stored_bar_d,
                       const double* tdata_d, double noise, double* curve_d, double* stored_d, int32_t* status_h);
    void rhs_tracer(hipStream_t st, int nb, int level, Tracer& T, const double* tbar_d, const double* trdata_d, double noise,
                    double* T_d, int32_t* status_d);
    void rhs_finish(hipStream_t st, int nb, int level, bool zero_p);
    template <class T>
    void check_flux_user(int level, const T* t, const std::string& noun, const std::string& who) const;
    DevBuf<double> tr_curve, tr_stored, tr_cb, tr_sb, tr_data;
    DevBuf<double> trc_T, trc_tb, trc_data;
    DevBuf<int32_t> trc_i;
    void ensure_gradient(int level, bool tangent = false);   // tangent: the face-major copy as well
    void ensure_loglik(int level);
    // darcy_hessian.hip
    void gn_hessvec_chunk(int level, int nb, const double* k_d, const double* x_in_d, const double* dk_d, double noise,
                          bool wrt_log, double* hv_d, double* dG_host, double* x_out_d, pmc_stats* stats_tan,
                          pmc_stats* stats_adj);
};

// Batched CG vector algebra for Newton-CG (pmc_ncg_*; newton_cg.hip)
constexpr int kNcgThreads = 256;                   // workgroup of every pmc_ncg kernel
constexpr int kNcgPer = 16;                        // entries per thread: eight 16-byte accesses per vector
constexpr int kNcgChunk = kNcgThreads * kNcgPer;   // entries per workgroup = the unit of the fixed summation order
struct NcgCol {                                    // one column's scalars, kept on the device
    double rr, gg, tol2, pHp;                      // <r, r>, <g, g>, (eta |g|)^2, the last <p, Hp>
    int32_t count, done, npc, active;              // steps taken, finished, ended on <p, Hp> <= 0, active at pmc_ncg_begin
};
struct Ncg {
    Ctx& ctx;
    int n, nbmax, nch;                             // column length, widest batch, chunks per column
    DevBuf<double> d, r, p, part_a, part_b, scal, dots;
    DevBuf<int32_t> mask;
    DevBuf<NcgCol> cols;                           // 2 x nbmax, double-buffered by step parity
    DevBuf<double> stage[3];                       // host-memory callers: staged operands (allocated at first use)
    NcgCol* h_cols = nullptr;                      // pinned
    double* h_dots = nullptr;                      // pinned
    int cur = 0, nb_cur = 0;
    static constexpr int kNcgSlots = 8;
    struct Slot {                                  // pinned staging of one call's per-column host arrays (16 B per column)
        char* h = nullptr;
        hipEvent_t ev = nullptr;
        bool used = false;
    };
    Slot slots[kNcgSlots];
    int slot_at = 0;
    Ncg(Ctx& c, int n, int nbmax);
    ~Ncg();
    Ncg(const Ncg&) = delete;
    Ncg& operator=(const Ncg&) = delete;
    void begin(int nb, const double* g, const double* eta, const int32_t* active, int memspace);
    void step(int nb, const double* hp, int memspace);
    void status(int nb, double* rr, int32_t* count, int32_t* done, int32_t* npc);
    void axpy(int nb, const double* t, const double* x, const double* dd, double* out, int memspace);
    void dot(int nb, const double* a, const double* b, double* out_host, int memspace);

private:
    const double* in(const double* a, int nb, int memspace, int slot);
    Slot& next_slot();
    void check(int nb, int memspace, const char* what) const;
};

}  // namespace pmc

struct pmc_sampler { pmc::Sampler impl; template <class... A> explicit pmc_sampler(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_conditioner { pmc::Conditioner impl; template <class... A> explicit pmc_conditioner(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_field_stats { pmc::FieldStats impl; template <class... A> explicit pmc_field_stats(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_level_fields { pmc::LevelFields impl; template <class... A> explicit pmc_level_fields(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_tracer { pmc::Tracer impl; template <class... A> explicit pmc_tracer(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_transport { pmc::Transport impl; template <class... A> explicit pmc_transport(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_darcy { pmc::Darcy impl; template <class... A> explicit pmc_darcy(A&&... a) : impl(std::forward<A>(a)...) {} };
struct pmc_ncg { pmc::Ncg impl; template <class... A> explicit pmc_ncg(A&&... a) : impl(std::forward<A>(a)...) {} };

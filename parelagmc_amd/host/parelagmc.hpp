// Host-side C++ mirror of ParELAGMC's plugin surface and Monte Carlo managers.
//
// Same class and method names, argument meaning and error behaviour (exceptions) as the
// reference (paths relative to /root/reference):
//   MLSampler                 src/MLSampler.hpp:33-52
//   PhysicalMLSolver          src/PhysicalMLSolver.hpp:33-62
//   NormalDistributionSampler src/NormalDistributionSampler.hpp:27-64
//   PDESampler                src/PDESampler.hpp (Sample/Eval/SampleSize/GetNNZ)
//   KLSampler                 src/KLSampler.hpp (the same methods over a pmc_sampler_create_kl handle)
//   MaternCovariance          src/MaternCovariance.hpp (SolveEigenvalue / Eigenvalues / Eigenvectors over pmc_kl_matern_eigs)
//   DarcySolver               src/DarcySolver.hpp (SolveFwd/GetNumberOfDofs/GetNNZ)
//   MLMC_Manager              src/MLMC_Manager.hpp:24-181
//   MC_Manager                src/MC_Manager.hpp
// mfem::Vector is replaced by parelagmc::Vector, a (pointer, size, memory space) view that can
// live in HBM, so a whole realization (xi -> s -> Q) never crosses PCIe.  The numerical work is
// delegated to libpmc.so through include/pmc.h; nothing here touches a GPU API directly.
#pragma once

#include <cstdint>
#include <fstream>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <ostream>
#include <vector>

#include "../../include/pmc.h"
#include "../../include/pmc_host.h"

namespace parelagmc {

// A batch of `nbatch` vectors of `size` doubles each, sample-major, in host or device memory.
class Vector {
  public:
    Vector() = default;
    Vector(pmc_ctx* ctx, int memspace) : ctx_(ctx), memspace_(memspace) {}
    Vector(const Vector&) = delete;
    Vector& operator=(const Vector&) = delete;
    ~Vector();
    void SetSize(int size, int nbatch = 1);   // reallocates when the capacity is too small
    void Swap(Vector& o);                     // exchange storage (same context and memory space)
    void Adopt(double* p, int size, int nbatch) { data_ = p; size_ = size; nbatch_ = nbatch; cap_ = (size_t)size * nbatch; }
    void Release() { data_ = nullptr; cap_ = 0; }   // forget adopted storage without freeing it
    int Size() const { return size_; }
    int Batch() const { return nbatch_; }
    int MemSpace() const { return memspace_; }
    double* GetData() { return data_; }
    const double* GetData() const { return data_; }

  private:
    pmc_ctx* ctx_ = nullptr;
    int memspace_ = PMC_MEM_HOST;
    double* data_ = nullptr;
    size_t cap_ = 0;
    int size_ = 0, nbatch_ = 1;
};

/// Accumulated device time of one plugin on one level: the reference's TimeManager entries "Sampler: Mult -- Level i"
/// (src/PDESampler.cpp:328-333), "Darcy: Mult -- Level i" and "Darcy: Build Solver -- Level i" (src/DarcySolver.cpp:231-243),
/// measured with HIP events on the plugin's stream (pmc_stats.solve_ms / setup_ms).
struct PhaseTimes {
    double mult_ms = 0.0;    // Krylov solves
    double setup_ms = 0.0;   // per-realization work ahead of them (rhs / M(k), elimination, Schur hierarchy refresh)
    int64_t realizations = 0;
    void add(const pmc_stats* st, int n) {
        for (int i = 0; i < n; ++i) { mult_ms += st[i].solve_ms; setup_ms += st[i].setup_ms; }
        realizations += n;
    }
};

class MLSampler {
  public:
    virtual ~MLSampler() = default;
    /// Fill xi with nbatch realizations of white noise for `level`; ids first_id .. first_id+nbatch-1
    virtual void Sample(const int level, Vector& xi, uint64_t first_id = 0, int nbatch = 1) = 0;
    /// Evaluate random field at level with random sample xi
    virtual void Eval(const int level, const Vector& xi, Vector& s) = 0;
    /// ... storing the Gaussian field in u and optionally warm-starting from it (use_init)
    virtual void Eval(const int level, const Vector& xi, Vector& s, Vector& u, bool use_init) = 0;
    virtual int SampleSize(int level) const = 0;
    virtual size_t GetNNZ(int level) const = 0;
    /// Build the hierarchy of the sampler (src/MLSampler.hpp:64-66).  The operators arrive assembled through the C ABI,
    /// so for handle-backed samplers this only checks that the handle exists; plugins may do real work here.
    virtual void BuildHierarchy() {}
    /// Prolongator of the sample space from level+1 to level (src/MLSampler.hpp:85-87; a HypreParMatrix there, a CSR
    /// view with host pointers owned by the sampler here).  Default: not available.
    virtual pmc_csr GetTrueP(int /*level*/) const { throw std::runtime_error("GetTrueP: not provided by this sampler"); }
    /// Realizations of `level` the plugin processes at once most efficiently (0 = no preference).  The managers cut a
    /// level's realizations into plugin calls of at most this many (device plugins: 16 on large levels, up to 256 on the
    /// smallest - pmc_sampler_batch_width).
    virtual int PreferredBatch(int /*level*/) const { return 0; }
    /// Device time spent on `level` since construction / ResetPhaseTimes (zero for plugins that do not measure)
    virtual PhaseTimes GetPhaseTimes(int /*level*/) const { return PhaseTimes(); }
    virtual void ResetPhaseTimes() {}
};

class PhysicalMLSolver {
  public:
    virtual ~PhysicalMLSolver() = default;
    /// Solve and update quantity of interest Q, cost C (arrays of k.Batch() entries)
    virtual void SolveFwd(int ilevel, Vector& k_over_k_ref, double* Q, double* C) = 0;
    /// The reference's signature (src/PhysicalMLSolver.hpp:33-39): one realization, Q and C by reference
    void SolveFwd(int ilevel, Vector& k_over_k_ref, double& Q, double& C) {
        if (k_over_k_ref.Batch() != 1) throw std::invalid_argument("SolveFwd(double&, double&): one realization expected");
        SolveFwd(ilevel, k_over_k_ref, &Q, &C);
    }
    /// Solve and return the pressure block P (k.Batch() x pressure dofs), cost C and, when compute_Q, the QoI Q
    /// (src/PhysicalMLSolver.hpp:41-47).  Arrays of k.Batch() entries.
    virtual void SolveFwd_RtnPressure(int /*ilevel*/, Vector& /*k_over_k_ref*/, Vector& /*P*/, double* /*C*/, double* /*Q*/,
                                      bool /*compute_Q*/) {
        throw std::runtime_error("SolveFwd_RtnPressure: not provided by this solver");
    }
    void SolveFwd_RtnPressure(int ilevel, Vector& k_over_k_ref, Vector& P, double& C, double& Q, bool compute_Q) {
        if (k_over_k_ref.Batch() != 1) throw std::invalid_argument("SolveFwd_RtnPressure(double&, double&): one realization expected");
        SolveFwd_RtnPressure(ilevel, k_over_k_ref, P, &C, &Q, compute_Q);
    }
    virtual int GetNumberOfDofs(int ilevel) const = 0;
    virtual int GetGlobalNumberOfDofs(int ilevel) const = 0;
    virtual int GetNNZ(int ilevel) const = 0;
    /// see MLSampler::PreferredBatch
    virtual int PreferredBatch(int /*ilevel*/) const { return 0; }
    virtual PhaseTimes GetPhaseTimes(int /*ilevel*/) const { return PhaseTimes(); }
    virtual void ResetPhaseTimes() {}
};

/// Uncorrelated N(mu, sigma2) variates (counter-based generator on the device).
class NormalDistributionSampler {
  public:
    NormalDistributionSampler(pmc_ctx* ctx, double mu, double sigma2) : ctx_(ctx), mu_(mu), sigma2_(sigma2) {}
    NormalDistributionSampler(NormalDistributionSampler const&) = delete;
    NormalDistributionSampler& operator=(NormalDistributionSampler const&) = delete;
    /// Provides statistically independent random numbers to each part
    void Split(int nparts, int mypart);
    void Seed(uint64_t seed) { seed_ = seed; Split(nparts_, mypart_); }
    /// Fill v (all batch entries) with realizations first_id...
    void operator()(Vector& v, uint64_t first_id = 0, uint32_t stream = 0);

  private:
    pmc_ctx* ctx_;
    double mu_, sigma2_;
    uint64_t seed_ = 0;
    int nparts_ = 1, mypart_ = 0;
};

/// Device SPDE sampler (plain, matching-embedded or L2-projected: decided by the handle's projection).
class PDESampler : public MLSampler {
  public:
    PDESampler(pmc_ctx* ctx, pmc_sampler* handle) : ctx_(ctx), h_(handle) {}
    void Sample(const int level, Vector& xi, uint64_t first_id = 0, int nbatch = 1) override;
    void Eval(const int level, const Vector& xi, Vector& s) override;
    void Eval(const int level, const Vector& xi, Vector& s, Vector& u, bool use_init) override;
    /// Eval with the level xi was drawn on named instead of inferred from xi.Size()
    void EvalAt(const int level, const int xi_level, const Vector& xi, Vector& s);
    int SampleSize(int level) const override;
    size_t GetNNZ(int level) const override;
    void BuildHierarchy() override;
    pmc_csr GetTrueP(int level) const override;
    int PreferredBatch(int level) const override { return pmc_sampler_batch_width(h_, level); }
    PhaseTimes GetPhaseTimes(int level) const override { return level < (int)times_.size() ? times_[level] : PhaseTimes(); }
    void ResetPhaseTimes() override { times_.clear(); adj_times_.clear(); }
    int GetNumIters() const { return last_iters_; }   // the reference returns -1 (PDESampler.hpp:142-145)
    /// MLSampler::ComputeL2Error / ComputeMaxError of ONE field (coeff.Batch() == 1; pmc_sampler_l2_error / _max_error).
    /// L2: the squared error, as the reference returns.
    double ComputeL2Error(int level, const Vector& coeff, double exact) const;
    double ComputeMaxError(int level, const Vector& coeff, double exact) const;
    /// the batched forms: err[c] of each of coeff.Batch() fields (err: coeff.Batch() host doubles)
    void ComputeL2Error(int level, const Vector& coeff, double exact, double* err) const;
    void ComputeMaxError(int level, const Vector& coeff, double exact, double* err) const;
    /// The adjoint of Eval in the white noise (pmc_sampler_eval_adjoint): grad_xi = (d Eval / d xi)^T v for every
    /// realization of v (v.Batch() x SampleSize(level)); s_or_null: nullptr, or Eval's output on a lognormal handle (v is
    /// multiplied by it).  grad_xi is sized to v.Batch() x xi_size(xi_level) in v's memory space; xi_level < 0: level.
    /// The adjoint solves are timed apart from Eval's: GetPhaseTimes / GetNumIters keep meaning the forward solves.
    void EvalAdjoint(const int level, const Vector& v, const Vector* s_or_null, Vector& grad_xi, int xi_level = -1);
    /// The tangent of Eval in the white noise (pmc_sampler_eval_tangent): ds = (d Eval / d xi) v for every realization of v
    /// (v.Batch() x xi_size(xi_level)): Eval of v without exp(), times s_or_null when given (Eval's output on a lognormal
    /// handle).  ds is sized to v.Batch() x SampleSize(level) in v's memory space; xi_level < 0: level.  Timed with the adjoint
    /// solves, apart from Eval's.
    void EvalTangent(const int level, const Vector& v, const Vector* s_or_null, Vector& ds, int xi_level = -1);
    PhaseTimes GetAdjointPhaseTimes(int level) const { return level < (int)adj_times_.size() ? adj_times_[level] : PhaseTimes(); }
    int GetNumAdjointIters() const { return last_adj_iters_; }
    bool IsLognormal() const { return pmc_sampler_is_lognormal(h_) == 1; }
    /// Eval returns fields conditioned on the data of `c` (pmc_conditioner_create on this handle, exact data); nullptr
    /// detaches (pmc_sampler_set_conditioner).  The caller keeps ownership of `c`.  EvalAdjoint / EvalTangent, the
    /// BayesianInverseProblem derivative entries and ComputeMAP refuse the handle while `c` is attached unless the caller
    /// has opted in with pmc_conditioner_enable_derivatives(c, 1): they then differentiate the conditional field.
    void SetConditioner(pmc_conditioner* c);
    pmc_sampler* Handle() const { return h_; }
    pmc_ctx* Context() const { return ctx_; }

  private:
    int level_of_xi(int size) const;
    int level_of_field(int size) const;
    void record(int level, const std::vector<pmc_stats>& st) {
        if ((int)times_.size() <= level) times_.resize(level + 1);
        times_[level].add(st.data(), (int)st.size());
        last_iters_ = st.empty() ? -1 : st[0].iterations;
    }
    pmc_ctx* ctx_;
    pmc_sampler* h_;
    int last_iters_ = -1, last_adj_iters_ = -1;
    std::vector<PhaseTimes> times_, adj_times_;
};

/// Device truncated Karhunen-Loeve sampler: a handle from pmc_sampler_create_kl behind the same calls (GetNumIters() = 0).
class KLSampler : public PDESampler {
  public:
    using PDESampler::PDESampler;
};

/// MaternCovariance on the finest level, solved on the device without storing the covariance matrix (pmc_kl_matern_eigs;
/// 3D only).  centroids: n x 3 row-major element centres, w_diag: the P0 mass diagonal; both are read by SolveEigenvalue()
/// and must live until then.  Eigenvalues() ascend, Eigenvectors() is n x NumberOfModes() column-major with V^T W V = I:
/// what pmc_sampler_create_kl (KLSampler) and mfem_adapter::DeviceKLSampler take.  Not converged within max_iter is not
/// an exception: read Info().converged.
class MaternCovariance {
  public:
    MaternCovariance(pmc_ctx* ctx, int n, const double* centroids, const double* w_diag, double corlen, int nmodes)
        : ctx_(ctx), n_(n), x_(centroids), w_(w_diag), corlen_(corlen), m_(nmodes < n ? nmodes : n) {
        pmc_kl_eigs_opts_default(&opts_);
    }
    pmc_kl_eigs_opts& Options() { return opts_; }
    void SolveEigenvalue() {
        if (m_ < 1) throw std::runtime_error("MaternCovariance: need at least one mode");
        evals_.assign((size_t)m_, 0.0);
        evect_.assign((size_t)n_ * m_, 0.0);
        if (pmc_kl_matern_eigs(ctx_, 3, n_, x_, w_, corlen_, m_, &opts_, evals_.data(), evect_.data(), &info_) != PMC_OK)
            throw std::runtime_error(std::string("MaternCovariance::SolveEigenvalue: ") + pmc_last_error());
    }
    int NumberOfModes() const { return m_; }
    const std::vector<double>& Eigenvalues() const { return evals_; }
    const std::vector<double>& Eigenvectors() const { return evect_; }
    const pmc_kl_eigs_info& Info() const { return info_; }

  private:
    pmc_ctx* ctx_;
    int n_;
    const double *x_, *w_;
    double corlen_;
    int m_;
    pmc_kl_eigs_opts opts_;
    pmc_kl_eigs_info info_{};
    std::vector<double> evals_, evect_;
};

/// The drivers' per-level statistics (PDESamplerTest.cpp:205-274) on the device: an owning wrapper of pmc_field_stats.
/// Destroy it before the sampler it was created on.
class FieldStatistics {
  public:
    /// chi: SampleSize(level) entries (host or device, chi.MemSpace()), or nullptr for no chi_cov
    FieldStatistics(PDESampler& sampler, int level, const Vector* chi = nullptr);
    ~FieldStatistics() { pmc_field_stats_destroy(fs_); }
    FieldStatistics(const FieldStatistics&) = delete;
    FieldStatistics& operator=(const FieldStatistics&) = delete;
    void Run(uint64_t first_id, int64_t nsamples);          // Sample + Eval + accumulate on the device
    void Accumulate(const Vector& s);                        // s.Batch() realizations the caller holds
    void Reset();
    /// (1/N) sum s, (1/N) sum s^2 (about zero), (1/N) sum <chi, s> s into host arrays of SampleSize(level); any may be NULL
    int64_t Read(double* expectation, double* second_moment, double* chi_cov) const;
    int Size() const { return n_; }

  private:
    pmc_field_stats* fs_ = nullptr;
    int n_ = 0;
};

/// Particle travel times on the RT0 Darcy flux (an extension): an owning wrapper of pmc_tracer.
/// Attach it to a level with DarcySolver::SetTracer to make the travel-time QoI the Q the managers see; detach it (or destroy
/// the solver) before destroying it.  One tracer serves one DarcySolver at a time.
class ParticleTracer {
  public:
    /// x0: nparticles x 3 start points, elem0: their elements; max_steps 0: 64 + 32 ceil(cbrt(n_elem))
    ParticleTracer(pmc_ctx* ctx, const pmc_tracer_mesh& mesh, int nparticles, const double* x0, const int32_t* elem0,
                   int max_steps = 0);
    ~ParticleTracer() { pmc_tracer_destroy(h_); }
    ParticleTracer(const ParticleTracer&) = delete;
    ParticleTracer& operator=(const ParticleTracer&) = delete;
    int NumParticles() const { return pmc_tracer_num_particles(h_); }
    /// u: the flux rows of u.Batch() realizations (row stride u.Size() >= n_face, e.g. full solution vectors); the outputs are
    /// u.Batch() x NumParticles() in u's memory space, x_exit (x 3) may be NULL
    void Run(const Vector& u, double* T, int32_t* exit_face, int32_t* status, int32_t* nsteps, double* x_exit = nullptr);
    /// Q (host, nbatch): mean (PMC_TRACER_MEAN) or minimum (PMC_TRACER_MIN) of T per realization; not_exited (host) may be NULL
    void Reduce(int nbatch, const double* T, const int32_t* status, int kind, double* Q, int32_t* not_exited, int memspace);
    /// The adjoint of the walk, its decisions held (pmc_tracer_run_adjoint): u_bar = dJ/du and x0_bar =
    /// dJ/dx0 (u.Batch() x NumParticles() x 3, may be NULL) of J = <T_bar, T> + <x_exit_bar, x_exit> per realization.  Seeds
    /// (u.Batch() x NumParticles() and x 3; each may be NULL, not both) and outputs in u's memory space; u_bar is sized to
    /// u.Size() x u.Batch() and only the first n_face entries of a row are written.  T, exit_face, nsteps may be NULL; status
    /// may not.  Particles that did not exit contribute nothing.
    void RunAdjoint(const Vector& u, const double* T_bar, const double* x_exit_bar, Vector& u_bar, double* x0_bar, double* T,
                    int32_t* exit_face, int32_t* status, int32_t* nsteps);
    /// T_bar = dQ/dT of the Q of Reduce (pmc_tracer_reduce_seed), in the memory space of T and status
    void ReduceSeed(int nbatch, const double* T, const int32_t* status, int kind, double* T_bar, int memspace);
    /// cap in bytes on the records of one chunk of columns of RunAdjoint; 0: 256 MiB.  The results do not depend on it.
    void SetAdjointScratch(int64_t bytes);
    pmc_tracer* Handle() const { return h_; }

  private:
    pmc_tracer* h_ = nullptr;
};

/// First-order upwind transport of a passive solute on the Darcy flux (an extension): an owning wrapper
/// of pmc_transport.  Attach it to a level with DarcySolver::SetTransport to make the mass that left through the outlet, or
/// the mass in place, the Q the managers see; detach it (or destroy the solver) before destroying it.  One handle serves one
/// DarcySolver at a time.
class SoluteTransport {
  public:
    SoluteTransport(pmc_ctx* ctx, const pmc_transport_mesh& mesh, const pmc_transport_params& params);
    ~SoluteTransport() { pmc_transport_destroy(h_); }
    SoluteTransport(const SoluteTransport&) = delete;
    SoluteTransport& operator=(const SoluteTransport&) = delete;
    int NumElements() const { return n_elem_; }
    int NumFluxDofs() const { return n_face_; }
    int NumOutletDofs() const { return n_outlet_; }
    int NumReports() const { return nreport_; }
    /// u: the flux rows of u.Batch() realizations (row stride u.Size() >= n_face, e.g. full solution vectors); the outputs are
    /// in u's memory space: c_out u.Batch() x NumElements() (may be NULL), curve u.Batch() x NumReports(), the rest u.Batch()
    void Run(const Vector& u, double* c_out, double* curve, double* stored, double* rate, double* t_reached, int32_t* nsteps,
             int32_t* status);
    /// Q (host, nbatch): curve[.][NumReports() - 1] (PMC_TRANSPORT_MASS_OUT) or stored (PMC_TRANSPORT_STORED)
    void Reduce(int nbatch, const double* curve, const double* stored, int kind, double* Q, int memspace);
    /// The discrete adjoint (pmc_transport_run_adjoint): u_bar = dJ/du and c0_bar = dJ/dc0 (may be NULL) of
    /// J = <curve_bar, curve> + stored_bar stored + <c_bar, c> per realization.  Seeds (each may be NULL, not all) and outputs in
    /// u's memory space; u_bar is sized to u.Size() x u.Batch() and only the first NumFluxDofs() entries of a row are written.
    /// curve, stored, nsteps may be NULL; status may not.
    void RunAdjoint(const Vector& u, const double* curve_bar, const double* stored_bar, const double* c_bar, Vector& u_bar,
                    double* c0_bar, double* curve, double* stored, int32_t* nsteps, int32_t* status);
    /// steps between two kept states of RunAdjoint; 0: automatic.  The results do not depend on it.
    void SetAdjointSegment(int K);
    pmc_transport* Handle() const { return h_; }

  private:
    pmc_transport* h_ = nullptr;
    int n_elem_ = 0, n_face_ = 0, n_outlet_ = 0, nreport_ = 0;
};

class DarcySolver : public PhysicalMLSolver {
  public:
    DarcySolver(pmc_ctx* ctx, pmc_darcy* handle) : ctx_(ctx), h_(handle) {}
    /// Q of SolveFwd / SolveFwd_RtnPressure on ilevel becomes the transport QoI (kind: PMC_TRANSPORT_MASS_OUT | _STORED;
    /// pmc_darcy_set_transport); nullptr detaches.  The gradient and Hessian entries keep <obs, x>.  A level holds a tracer or
    /// a transport, not both.
    void SetTransport(int ilevel, SoluteTransport* transport, int kind = PMC_TRANSPORT_MASS_OUT);
    /// Q of SolveFwd / SolveFwd_RtnPressure on ilevel becomes the tracer's travel-time QoI (kind: PMC_TRACER_MEAN | _MIN;
    /// pmc_darcy_set_tracer); nullptr detaches.  The gradient and Hessian entries keep <obs, x>.
    void SetTracer(int ilevel, ParticleTracer* tracer, int kind = PMC_TRACER_MEAN);
    using PhysicalMLSolver::SolveFwd;
    using PhysicalMLSolver::SolveFwd_RtnPressure;
    void SolveFwd(int ilevel, Vector& k_over_k_ref, double* Q, double* C) override;
    void SolveFwd_RtnPressure(int ilevel, Vector& k_over_k_ref, Vector& P, double* C, double* Q, bool compute_Q) override;
    /// SolveFwd plus the adjoint gradient dQ/dk (wrt_log: dQ/dlog k) of every realization: grad is sized to
    /// GetSizeOfStochasticData(ilevel) x k.Batch() in k's memory space (pmc_darcy_solve_gradient; an extension, the
    /// reference has no gradients).  Q, C: host arrays of k.Batch(), may be NULL.
    void SolveFwd_Gradient(int ilevel, Vector& k_over_k_ref, double* Q, double* C, Vector& grad, bool wrt_log = false);
    /// Forward solve plus the gradient in k (wrt_log: in log k) of J = <curve_bar, curve> + stored_bar stored of `transport` on
    /// the solution's flux (pmc_darcy_transport_gradient; an extension).  The transport is given with the call: what
    /// SetTransport / SetTracer attached is neither read nor changed.  curve_bar (k.Batch() x NumReports()), stored_bar
    /// (k.Batch()), one of them may be NULL, and the outputs curve, stored (may be NULL) in k's memory space; status: host,
    /// k.Batch().  grad is sized like k.
    void SolveFwd_TransportGradient(int ilevel, SoluteTransport& transport, Vector& k_over_k_ref, const double* curve_bar,
                                    const double* stored_bar, double* curve, double* stored, int32_t* status, Vector& grad,
                                    bool wrt_log = false);
    /// loglik = -|curve - data|^2 / (2 noise) of the breakthrough curve of `transport` and its gradient in k
    /// (pmc_darcy_transport_loglik_gradient).  data: host, NumReports(); loglik, curve (may be NULL) and status: host.
    void ComputeGradTransportLogLikelihood(int ilevel, SoluteTransport& transport, Vector& k_over_k_ref, const double* data,
                                           double noise, double* loglik, double* curve, int32_t* status, Vector& grad,
                                           bool wrt_log = false);
    /// Forward solve plus the gradient in k (wrt_log: in log k) of J = <T_bar, T> of the travel times of `tracer` on the
    /// solution's flux (pmc_darcy_tracer_gradient; an extension).  The tracer is given with the call: what SetTracer /
    /// SetTransport attached is neither read nor changed.  T_bar, T (may be NULL) and status, k.Batch() x NumParticles(), in
    /// k's memory space.  grad is sized like k.
    void SolveFwd_TracerGradient(int ilevel, ParticleTracer& tracer, Vector& k_over_k_ref, const double* T_bar, double* T,
                                 int32_t* status, Vector& grad, bool wrt_log = false);
    /// loglik = -|T - data|^2 / (2 noise) of the travel times of `tracer` and its gradient in k
    /// (pmc_darcy_tracer_loglik_gradient).  data: host, NumParticles(); loglik, T (may be NULL) and not_exited (k.Batch()): host.
    /// A realization with not_exited > 0 has a zero gradient.
    void ComputeGradTravelTimeLogLikelihood(int ilevel, ParticleTracer& tracer, Vector& k_over_k_ref, const double* data,
                                            double noise, double* loglik, double* T, int32_t* not_exited, Vector& grad,
                                            bool wrt_log = false);
    /// Gauss-Newton Hessian action hv = J^T (1/noise) J dk of the negative log-likelihood of the handle's observation
    /// functionals, J = dG/dk (wrt_log: in log k), for every realization (pmc_darcy_gn_hessvec; an extension).  x: the forward
    /// solutions, GetNumberOfDofs(ilevel) x k.Batch() - x_given false: solved inside and written to x; true: read, and no
    /// forward solve runs.  hv is sized like k; k, dk, x, hv share a memory space.  dG: host array k.Batch() x nobs = J dk,
    /// may be NULL.
    void SolveFwd_GNHessVec(int ilevel, Vector& k_over_k_ref, const Vector& dk, double noise, Vector& x, bool x_given, Vector& hv,
                            double* dG = nullptr, bool wrt_log = false);
    int GetSizeOfStochasticData(int ilevel) const;   // entries of k (src/DarcySolver.hpp:127-130)
    int GetNumberOfDofs(int ilevel) const override;
    int GetGlobalNumberOfDofs(int ilevel) const override;
    int GetNNZ(int ilevel) const override;
    int PreferredBatch(int ilevel) const override { return pmc_darcy_batch_width(h_, ilevel); }
    pmc_darcy* Handle() const { return h_; }
    PhaseTimes GetPhaseTimes(int ilevel) const override { return ilevel < (int)times_.size() ? times_[ilevel] : PhaseTimes(); }
    void ResetPhaseTimes() override { times_.clear(); }

  private:
    void record(int level, const std::vector<pmc_stats>& st) {
        if ((int)times_.size() <= level) times_.resize(level + 1);
        times_[level].add(st.data(), (int)st.size());
    }
    pmc_ctx* ctx_;
    pmc_darcy* h_;
    std::vector<PhaseTimes> times_;
};

/// Plugins backed by C callbacks (host memory).
class CallbackSampler : public MLSampler {
  public:
    CallbackSampler(int nlevels, const pmc_plugin_callbacks& cb);
    void Sample(const int level, Vector& xi, uint64_t first_id = 0, int nbatch = 1) override;
    void Eval(const int level, const Vector& xi, Vector& s) override;
    void Eval(const int level, const Vector& xi, Vector& s, Vector& u, bool use_init) override;
    int SampleSize(int level) const override { return ssize_.at(level); }
    size_t GetNNZ(int) const override { return 0; }

  private:
    pmc_plugin_callbacks cb_;
    std::vector<int> xsize_, ssize_;
};
class CallbackSolver : public PhysicalMLSolver {
  public:
    CallbackSolver(int nlevels, const pmc_plugin_callbacks& cb);
    void SolveFwd(int ilevel, Vector& k, double* Q, double* C) override;
    int GetNumberOfDofs(int l) const override { return ndofs_.at(l); }
    int GetGlobalNumberOfDofs(int l) const override { return ndofs_.at(l); }
    int GetNNZ(int) const override { return 0; }

  private:
    pmc_plugin_callbacks cb_;
    std::vector<int> ndofs_;
};

/// Bayesian inverse problem on top of the forward solver (src/BayesianInverseProblem.hpp): observation operator G,
/// Gaussian likelihood with noise variance `noise`, ratio integrand R = Q * likelihood.  The observation functionals
/// live in the solver handle (pmc_darcy_set_observations).
class BayesianInverseProblem {
  public:
    BayesianInverseProblem(pmc_darcy* solver, double noise, std::vector<double> G_obs)
        : solver_(solver), noise_(noise), G_obs_(std::move(G_obs)) {}
    /// G (k.Batch() x size_obs_data), C and optionally Q
    void ComputeG(int ilevel, Vector& k_over_k_ref, std::vector<double>& G, double* C, double* Q, bool compute_Q);
    void ComputeLikelihood(int ilevel, Vector& k_over_k_ref, double* likelihood, double* C);
    void ComputeLikelihoodAndQ(int ilevel, Vector& k_over_k_ref, double* likelihood, double* C, double* Q);
    void ComputeR(int ilevel, Vector& k_over_k_ref, double* R, double* C);
    /// log of ComputeLikelihood and its adjoint gradient with respect to k (wrt_log: log k) for every realization: loglik
    /// host array of k.Batch() (may be NULL), grad sized to n_p x k.Batch() in k's memory space (pmc_darcy_loglik_gradient)
    void ComputeGradLogLikelihood(int ilevel, Vector& k_over_k_ref, double* loglik, Vector& grad, bool wrt_log = false);
    /// log pi(xi) = loglik(Eval(ilevel, xi)) - |xi|^2 / 2 and its gradient in the white noise xi for every realization of xi
    /// (drawn on ilevel or finer): Eval, pmc_darcy_loglik_gradient (with respect to log k on a lognormal sampler, which
    /// carries the factor k of the exp chain), pmc_sampler_eval_adjoint, the prior.  logpost: host array of xi.Batch() (may
    /// be NULL); grad sized like xi, in xi's memory space.  With device vectors only the scalars cross to the host.
    /// xi_level: the level xi was drawn on; < 0 infers it from xi.Size() (the first level up to ilevel of that size - name it
    /// for samplers whose levels share a size, such as KL handles).  The two work vectors (k and dloglik/dk) are kept between
    /// calls.
    void ComputeGradLogPosterior(int ilevel, PDESampler& sampler, const Vector& xi, double* logpost, Vector& grad,
                                 int xi_level = -1);
    /// Gauss-Newton Hessian of -log pi at xi applied to v for every realization: hv = v + (dk/dxi)^T J^T (1/noise) J (dk/dxi) v,
    /// symmetric positive definite, the full Hessian where G(k) = data (pmc_sampler_eval_tangent, pmc_darcy_gn_hessvec - in log k
    /// on a lognormal sampler, as ComputeGradLogPosterior chains the first derivatives -, pmc_sampler_eval_adjoint; the prior's
    /// v is added on the device).  v and hv are sized like xi, in xi's memory space; xi_level as in ComputeGradLogPosterior.
    /// reuse_state false: the linearization state - k = Eval(xi) and the forward solution - is computed from xi and kept;
    /// true: the state of the previous call is used (same ilevel, batch and memory space; xi is not read), and the call
    /// costs two sampler solves and two Darcy solves: a CG loop at a fixed xi pays for the linearization once.
    void ApplyGNHessian(int ilevel, PDESampler& sampler, const Vector& xi, const Vector& v, Vector& hv, int xi_level = -1,
                        bool reuse_state = false);
    /// the same on caller-owned state vectors k (n_p x batch) and x (n_u + n_p x batch)
    void ApplyGNHessian(int ilevel, PDESampler& sampler, const Vector& xi, const Vector& v, Vector& hv, int xi_level,
                        Vector& k_state, Vector& x_state, bool have_state);
    /// The maximiser of log pi in the white noise by inexact Gauss-Newton-CG, for every column of xi (the starting points on
    /// entry, the results on exit; host or device memory): the algorithm, options and result arrays of pmc_bayes_map
    /// (include/pmc_host.h).  ComputeGradLogPosterior and ApplyGNHessian do the solves; the CG algebra between two Hessian
    /// actions runs in the pmc_ncg kernels.  xi_level as in ComputeGradLogPosterior.  The work vectors and the CG workspace
    /// are kept between calls.
    void ComputeMAP(int ilevel, PDESampler& sampler, Vector& xi, const pmc_map_opts& opts, pmc_map_result& result,
                    int xi_level = -1);
    int SizeOfObservationalData() const { return (int)G_obs_.size(); }

  private:
    pmc_darcy* solver_;
    double noise_;
    std::vector<double> G_obs_;
    // ComputeMAP: iterate (host callers), trial point, gradients at both, H p, linearization state; the CG workspace
    std::unique_ptr<Vector> map_xi_, map_trial_, map_g_, map_gt_, map_hp_, map_k_, map_x_;
    std::unique_ptr<pmc_ncg, void (*)(pmc_ncg*)> map_ncg_{nullptr, pmc_ncg_destroy};
    int map_ncg_n_ = 0, map_ncg_nb_ = 0;
    std::unique_ptr<Vector> work_k_, work_gk_;   // ComputeGradLogPosterior
    std::unique_ptr<Vector> state_k_, state_x_, work_dk_, work_hk_;   // ApplyGNHessian: linearization state, dk, J^T J dk
};

double expWRegression(const std::vector<double>& y, const std::vector<double>& x, int skip_n_last);

/// Multi-level Monte Carlo manager: the reference's serial loop, sharded over a sample farm.
class MLMC_Manager {
  public:
    enum { Y2 = 0, Y = 1, ABSY = 2, Q2 = 3, Q = 4, ABSQ = 5, C = 6, Y3 = 7, Y4 = 8, NVAR = 9 };

    MLMC_Manager(pmc_ctx* ctx, int memspace, int nlevels, PhysicalMLSolver& pSolver, MLSampler& sampler,
                 const pmc_mlmc_params& params);
    void SetFarm(int nranks, int rank, std::function<void(double*, int)> reduce);
    /// Additional plugin pair (own context / HIP stream) working on this rank's realizations concurrently:
    /// the launch-latency-bound kernels of the small levels of one lane overlap the other lanes' work.
    void AddLane(pmc_ctx* ctx, PhysicalMLSolver& solver, MLSampler& sampler);
    /// the farm's collective: seconds this rank spent in the SUM all-reduce of the accumulators and the number of
    /// reductions (one per InitRun round, src/MLMC_Manager.cpp:178 is where the serial reference would need it)
    void FarmTimes(double* allreduce_seconds, int64_t* reductions) const {
        if (allreduce_seconds) *allreduce_seconds = reduce_seconds_;
        if (reductions) *reductions = reduce_count_;
    }
    /// Run ML simulation by sampling v_init_nsamples then the missing samples until the estimator variance target is met
    void Run();
    /// Run ML simulation using level_nsamples_init[i] samples on level i
    void InitRun(std::vector<int>& level_nsamples_init);
    void Reset();
    /// Resume: rebuild the sums table and sample counters from a per-sample log of an earlier run
    int64_t ReplayLog(const std::string& path);
    void ShowMe(std::ostream& os) const;
    /// The reference's TimeManager::Print (examples/MLMC.cpp:275) for the per-realization path: "Sampler: Mult", "Darcy: Build
    /// Solver" and "Darcy: Mult" per level, device milliseconds summed over all lanes of this rank, with realization counts
    void PrintTimers(std::ostream& os) const;
    void PhaseTimesOfLevel(int level, double* sampler_mult_ms, double* darcy_setup_ms, double* darcy_mult_ms,
                           int64_t* sampler_realizations, int64_t* darcy_realizations) const;
    /// Multilevel estimates of the Darcy pressure field: from now on every level pair also
    /// accumulates the pressure statistics on the device.  Device-handle managers only, before the first InitRun or after
    /// Reset, after the last AddLane.  w0: the level-0 P0 mass, GetSizeOfStochasticData(0) entries > 0 (host or device).
    void EnablePressureStatistics(const Vector& w0);
    bool PressureStatisticsEnabled() const { return !pfields_.empty(); }
    /// Level-0 maps (each may be NULL, else GetSizeOfStochasticData(0) entries in its own memory space):
    /// mean = sum_l I_l mean_l(p_l - p_{l+1}), second_moment = sum_l I_l mean_l(p_l^2 - p_{l+1}^2) (about zero, uncentred),
    /// estimator_variance = sum_l I_l var_l(p_l - p_{l+1}) / N_l; per level (host arrays of nlevels, may be NULL)
    /// ||mean_l||_L2 and int var_l with the weights (P chain)^T w0.  Collective when the farm has several ranks.
    void PressureStatistics(Vector* mean, Vector* second_moment, Vector* estimator_variance, double* l2_mean_corr,
                            double* int_var_corr);
    ~MLMC_Manager();

    bool wallTime;   // public switch, src/MLMC_Manager.hpp:61

    // results (read by pmc_mlmc_result_get)
    int nlevels;
    double eps2, ratio;
    double ml_estimator_variance, expected_discretization_error2, actualMSE;
    double alpha = 0, alphaABS = 0, beta = 0, gamma = 0;
    std::vector<double> sums, eY, eABSY, eQ, eABSQ, eC, varY, varQ, consistency, kurtosis, M, VC, cost, level_seconds;
    std::vector<int64_t> level_nsamples, level_nsamples_missing;

  private:
    void computeNSamplesMSE();
    void run_level(int ilevel, int nsamples);
    // several lanes: all levels of one InitRun round go through one task queue (finest level first), so the
    // launch-latency-bound batches of the coarse levels overlap the bandwidth-bound batches of the fine ones
    void run_round_overlapped(const std::vector<int>& level_nsamples_init);
    // realizations per plugin call on `ilevel`: at most `batch`, at most what the plugins prefer for that level
    // (PreferredBatch: 16 on large levels ... 256 on the smallest), and small enough that every RANK of a farm gets a share.
    // Independent of the number of lanes: on a given farm the blocks of realization ids - and with them every realization's
    // bits - do not depend on how many lanes share a GPU.  Identical on all ranks.
    int level_batch(int ilevel, int nsamples) const;
    double& S(int l, int v) { return sums[(size_t)l * NVAR + v]; }

    pmc_ctx* ctx_;
    int memspace_;
    PhysicalMLSolver& pSolver;
    MLSampler& sampler;
    int auto_eps2;
    std::vector<int> v_init_nsamples;
    int batch_, max_rounds_;
    int nranks_ = 1, rank_ = 0;
    std::function<void(double*, int)> reduce_;
    double reduce_seconds_ = 0.0;          // wall time this rank spent inside the farm's all-reduce (incl. waiting for the
    int64_t reduce_count_ = 0;             // slowest rank), and how many there were: one per InitRun round
    std::vector<double> pending_;          // this round's local contributions (sums + counts + seconds)
    struct Lane {
        pmc_ctx* ctx;
        MLSampler* sampler;
        PhysicalMLSolver* solver;
        Vector xi, sparam, init_s;
        Vector p_fine, p_coarse;   // pressure blocks of the level pair (pressure statistics only)
        Lane(pmc_ctx* c, int ms, MLSampler* s, PhysicalMLSolver* p)
            : ctx(c), sampler(s), solver(p), xi(c, ms), sparam(c, ms), init_s(c, ms), p_fine(c, ms), p_coarse(c, ms) {}
    };
    std::vector<std::unique_ptr<Lane>> lanes_;
    // pressure statistics: one accumulator per level (on lane 0's stream with one lane, else on stats_ctx_, a stream of
    // their own on the lanes' device), the parent maps of the coupled levels and the weights (P chain)^T w0 per level
    std::vector<pmc_level_fields*> pfields_;
    pmc_ctx* stats_ctx_ = nullptr;
    std::vector<std::vector<int32_t>> parents_;
    std::vector<std::vector<double>> weights_;
    void release_pressure_stats();
    // one level pair's solves of a block of m realizations on lane L, with the pressure blocks kept when enabled
    void solve_block(Lane& L, int ilevel, int m, double* q, double* c, double* qc, double* cc);
    std::ofstream logger;
    std::string log_path_;
    bool append_log_ = false;
};

/// What the ratio managers call (the reference's BayesianInverseProblem seen from ML_BayesRatio_Manager):
/// prior draws plus likelihood and ratio integrand.
class BayesRatioProblem {
  public:
    virtual ~BayesRatioProblem() = default;
    virtual void SamplePrior(int level, Vector& xi, uint64_t first_id, int nbatch) = 0;
    virtual void EvalPrior(int level, const Vector& xi, Vector& s) = 0;
    /// likelihood[b] and R[b] = Q[b] * likelihood[b]; C[b] = cost (dofs)
    virtual void ComputeLikelihoodAndR(int level, Vector& s, double* likelihood, double* R, double* C) = 0;
    virtual int GetGlobalNumberOfDofs(int level) const = 0;
    /// realizations of `level` one launch of the device plugins carries (0: no preference), see MLSampler::PreferredBatch
    virtual int PreferredBatch(int /*level*/) const { return 0; }
    /// for the posterior field estimates: the device forward-problem handle and the entries of EvalPrior's output on
    /// `level` (nullptr / -1: the prior's fields never reach the device)
    virtual pmc_darcy* DarcyHandle() const { return nullptr; }
    virtual int PriorFieldSize(int /*level*/) const { return -1; }
};

/// Multilevel (nlevels > 1) / single-level (nlevels == 1) ratio estimator, src/ML_BayesRatio_Manager.hpp.
/// SetSplitting(true) turns it into ML_BayesRatio_Splitting_Manager / SL_BayesRatio_Splitting_Manager
/// (src/ML_BayesRatio_Splitting_Manager.hpp): the same draws, but the estimated quantity is E[R/Z] with the
/// level difference r/z - r_c/z_c ("divide, then subtract"), and the variance / bias / sample allocation follow the
/// Ratio columns of the sums table instead of max(R, Z).
class ML_BayesRatio_Manager {
  public:
    enum { YZ2 = 0, YZ = 1, ABS_YZ = 2, Z2 = 3, Z = 4, ABS_Z = 5, YR2 = 6, YR = 7, ABS_YR = 8, R2 = 9, R = 10,
           ABS_R = 11, YRatio2 = 12, YRatio = 13, ABS_YRatio = 14, Ratio2 = 15, Ratio = 16, ABS_Ratio = 17, C = 18,
           T = 19, NVAR = 20 };
    ML_BayesRatio_Manager(pmc_ctx* ctx, int memspace, int nlevels, BayesRatioProblem& problem,
                          const pmc_mlmc_params& params);
    void SetFarm(int nranks, int rank, std::function<void(double*, int)> reduce);
    void SetSplitting(bool on) { splitting = on; }
    void Run();
    void InitRun(std::vector<int>& level_nsamples_init);
    void Reset();
    /// Posterior field estimates: from now on every level also accumulates, on the device, the
    /// likelihood-weighted sums of the R-draws' prior field k (w k - w_c k_c[parent] with w = L, or L / Z when splitting).
    /// The scalar sums are unchanged.  Device-handle managers only, before the first InitRun or after Reset.  w0: the
    /// level-0 P0 mass, n_p(0) entries > 0 (host or device).
    void EnableFieldStatistics(const Vector& w0);
    bool FieldStatisticsEnabled() const { return !ffields_.empty(); }
    /// Level-0 maps (each may be NULL, else n_p(0) entries in its own memory space) of the posterior mean of k, its second
    /// moment about zero and the estimator variance of the mean; per level (host arrays of nlevels, may be NULL) the level's
    /// contribution to the mean in the L2 norm and the integral of its variance term, with the weights (P chain)^T w0.
    /// The maps follow the mode (plain / splitting) the sums were accumulated in.  Collective when the farm has several ranks.
    void FieldStatistics(Vector* mean, Vector* second_moment, Vector* estimator_variance, double* l2_mean_corr,
                         double* int_var_corr);
    ~ML_BayesRatio_Manager();

    bool wallTime;
    bool splitting = false;
    int nlevels;
    double eps2, ratio;
    double alpha = 0, alphaABS = 0, beta = 0;   // rates of the Ratio columns (splitting manager)
    std::vector<double> eRatio, varRatio, eYRatio, varYRatio, eABS_YRatio;
    double ml_estimator_variance, ml_estimator_variance_R, ml_estimator_variance_Z;
    double expected_discretization_error2, expected_discretization_error2_R, expected_discretization_error2_Z, actualMSE;
    double alpha_R = 0, alphaABS_R = 0, beta_R = 0, alpha_Z = 0, alphaABS_Z = 0, beta_Z = 0, gamma = 0;
    std::vector<double> sums, eR, varR, eYR, varYR, eABS_YR, eZ, varZ, eYZ, varYZ, eABS_YZ, eC, M, cost, level_seconds;
    std::vector<int64_t> level_nsamples, level_nsamples_missing;

  private:
    void computeNSamplesMSE();
    void run_level(int ilevel, int nsamples);
    /// plugin-call size of a level: min(batch, what the plugins prefer there, a rank's share) - as MLMC_Manager::level_batch
    int level_batch(int ilevel, int nsamples) const;
    double& S(int l, int v) { return sums[(size_t)l * NVAR + v]; }
    BayesRatioProblem& problem;
    int auto_eps2, init_nsamples_, batch_, max_rounds_;
    int nranks_ = 1, rank_ = 0;
    std::function<void(double*, int)> reduce_;
    std::vector<double> pending_;
    pmc_ctx* ctx_;
    Vector zxi, xi, zparam, sparam;
    // posterior field estimates: one accumulator per level on ctx_'s stream, the parent maps of the coupled levels, the
    // weights (P chain)^T w0 per level, the coarse R-draw field (the fine one stays in sparam) and the mode the sums were
    // accumulated in (-1 none yet, 0 plain, 1 splitting, 2 both)
    std::vector<pmc_level_fields*> ffields_;
    std::vector<std::vector<int32_t>> fparents_;
    std::vector<std::vector<double>> fweights_;
    Vector sparam_c;
    int fields_mode_ = -1;
    void release_field_stats();
};

/// Single-level Monte Carlo manager (src/MC_Manager.hpp): the nlevels == 1 case of the above.
class MC_Manager : public MLMC_Manager {
  public:
    MC_Manager(pmc_ctx* ctx, int memspace, PhysicalMLSolver& pSolver, MLSampler& sampler, const pmc_mlmc_params& params)
        : MLMC_Manager(ctx, memspace, 1, pSolver, sampler, params) {}
};

}  // namespace parelagmc

// extern "C" surface of libpmc.so (see include/pmc.h).  No exception leaves this file.
#include <dlfcn.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "handles.hpp"

namespace pmc {

static thread_local std::string g_last_error;
void set_last_error(const std::string& m) { g_last_error = m; }

void Ctx::activate() const { PMC_HIP(hipSetDevice(device)); }
void Ctx::phase_mark(int i) const { PMC_HIP(hipEventRecord(ev_phase[i], stream)); }
void Ctx::phase_report(pmc_stats* stats, int nb) const {
    PMC_HIP(hipEventSynchronize(ev_phase[2]));
    float setup = 0.f, solve = 0.f;
    PMC_HIP(hipEventElapsedTime(&setup, ev_phase[0], ev_phase[1]));
    PMC_HIP(hipEventElapsedTime(&solve, ev_phase[1], ev_phase[2]));
    for (int k = 0; k < nb; ++k) {
        stats[k].setup_ms = (double)setup / nb;
        stats[k].solve_ms = (double)solve / nb;
    }
}

static std::atomic<int> g_live_ctx[64];
int Ctx::contexts_on_device(int device) { return g_live_ctx[device & 63].load(); }

Lanes Ctx::lanes(bool split) {
    if (split && !stream2) {
        PMC_HIP(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
        PMC_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        PMC_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    return Lanes{stream, split ? stream2 : stream, ev_fork, ev_join, split};
}

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return PMC_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return PMC_ERR_INTERNAL;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return PMC_ERR_INTERNAL;
    } catch (...) {
        set_last_error("unknown exception");
        return PMC_ERR_INTERNAL;
    }
}

// ---- RCCL, resolved lazily so that single-GPU use never needs the library ---------------------
struct UniqueId { char internal[128]; };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char* n : names) {
            r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    });
    if (!r.lib || !r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy)
        throw Error(PMC_ERR_COMM, "RCCL (librccl.so) could not be loaded");
    return r;
}
static void rccl_check(int rc, const char* what) {
    if (rc != 0) {
        Rccl& r = rccl();
        throw Error(PMC_ERR_COMM, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error"));
    }
}

}  // namespace pmc

using namespace pmc;

extern "C" {

int pmc_version(void) { return 100; }
int pmc_abi_version(void) { return PMC_ABI_VERSION; }
int pmc_krylov_z_bytes(void) { return 4; }   // of the default options (PMC_STORAGE_FP32)
uint64_t pmc_kernel_launches(void) { return kernel_launch_count(); }
uint64_t pmc_fused_lanczos_solves(void) { return fused_lanczos_solve_count(); }
uint64_t pmc_adopted_rhs_solves(void) { return adopted_rhs_solve_count(); }
uint64_t pmc_fused_field_evals(void) { return fused_field_eval_count(); }
uint64_t pmc_solve_path_count(int path) { return solve_path_count(path); }
const char* pmc_last_error(void) { return g_last_error.c_str(); }

static void check_abi(const pmc_solver_opts& o) {
    if (o.abi_version != PMC_ABI_VERSION)
        throw Error(PMC_ERR_INVALID, "pmc_solver_opts.abi_version is " + std::to_string(o.abi_version) + ", this library has " +
                                         std::to_string(PMC_ABI_VERSION) +
                                         ": fill the struct with pmc_solver_opts_default() of the header you compile against");
}

void pmc_solver_opts_default(pmc_solver_opts* o) {
    if (!o) return;
    o->max_iter = 300;
    o->rel_tol = 1e-6;
    o->abs_tol = 1e-12;
    o->abi_version = PMC_ABI_VERSION;
    // tuned on MI355X (scripts/sweep.py, cube_tet r=5): degree 2 on M needs no more MINRES iterations than
    // degree 3; smoothing interval [lmax/8, lmax]
    o->cheb_degree_M = 0;
    o->cheb_ratio_M = 0.0;
    o->mg_smooth_degree = 2;
    o->mg_smooth_ratio = 8.0;
    o->mg_coarse_degree = 12;
    o->mg_coarse_ratio = 100.0;
    o->check_every = 2;
    o->schur_scale = 1.0;
    o->mg_coarsening = 2;
    o->mini_max_rows = 6000;
    o->two_streams = 0;
    o->use_graph = 0;   // measured: no gain single-stream (kernels are latency-, not launch-bound), slower with 4 lanes
    o->precond_storage = PMC_STORAGE_FP32;
}

#undef pmc_ctx_create   // the header redirects the name to pmc_ctx_create_abi for C / C++ callers
int pmc_ctx_create(int device_id, pmc_ctx** out);
int pmc_ctx_create_abi(int device_id, int abi_version, pmc_ctx** out) {
    if (abi_version != PMC_ABI_VERSION) {
        if (out) *out = nullptr;
        set_last_error("caller was compiled against PMC_ABI_VERSION " + std::to_string(abi_version) + ", this library has " +
                       std::to_string(PMC_ABI_VERSION) + " (layout of pmc_solver_opts / pmc_stats): rebuild against include/pmc.h");
        return PMC_ERR_INVALID;
    }
    return pmc_ctx_create(device_id, out);
}
int pmc_ctx_create(int device_id, pmc_ctx** out) {
    return guarded([&] {
        PMC_REQUIRE(out != nullptr, "pmc_ctx_create: out is NULL");
        *out = nullptr;
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0)
            throw Error(PMC_ERR_DEVICE, "no HIP device available (libpmc has no CPU fallback)");
        PMC_REQUIRE(device_id >= 0 && device_id < ndev, "pmc_ctx_create: device id out of range");
        std::unique_ptr<pmc_ctx> c(new pmc_ctx());
        c->device = device_id;
        PMC_HIP(hipSetDevice(device_id));
        PMC_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        PMC_HIP(hipEventCreate(&c->ev0));
        PMC_HIP(hipEventCreate(&c->ev1));
        for (hipEvent_t& e : c->ev_phase) PMC_HIP(hipEventCreate(&e));
        PMC_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_flag), sizeof(int) * 16, hipHostMallocDefault));
        PMC_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_scal), sizeof(double) * pmc::Ctx::kHostScratch, hipHostMallocDefault));
        g_live_ctx[device_id & 63].fetch_add(1);
        *out = c.release();
    });
}

void pmc_ctx_destroy(pmc_ctx* c) {
    if (!c) return;
    g_live_ctx[c->device & 63].fetch_sub(1);
    (void)hipSetDevice(c->device);
    if (c->nccl) {
        try { rccl().CommDestroy(c->nccl); } catch (...) {}
        c->nccl = nullptr;
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->h_flag) (void)hipHostFree(c->h_flag);
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->ev_phase)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->ev_fork, c->ev_join})
        if (e) (void)hipEventDestroy(e);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int pmc_ctx_synchronize(pmc_ctx* c) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        c->activate();
        PMC_HIP(hipStreamSynchronize(c->stream));
    });
}

void* pmc_ctx_stream(pmc_ctx* c) { return c ? (void*)c->stream : nullptr; }
int pmc_ctx_device(const pmc_ctx* c) { return c ? c->device : -1; }

int pmc_timer_start(pmc_ctx* c) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        c->activate();
        PMC_HIP(hipEventRecord(c->ev0, c->stream));
    });
}
int pmc_timer_stop(pmc_ctx* c, double* ms) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && ms != nullptr, "ctx/ms is NULL");
        c->activate();
        PMC_HIP(hipEventRecord(c->ev1, c->stream));
        PMC_HIP(hipEventSynchronize(c->ev1));
        float f = 0.f;
        PMC_HIP(hipEventElapsedTime(&f, c->ev0, c->ev1));
        *ms = (double)f;
    });
}

int pmc_malloc(pmc_ctx* c, size_t bytes, void** dptr) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && dptr != nullptr, "pmc_malloc: NULL argument");
        c->activate();
        *dptr = nullptr;
        if (bytes) PMC_HIP(hipMalloc(dptr, bytes));
    });
}
int pmc_free(pmc_ctx* c, void* dptr) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        c->activate();
        if (dptr) PMC_HIP(hipFree(dptr));
    });
}
int pmc_memcpy_h2d(pmc_ctx* c, void* dst, const void* src, size_t bytes) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        c->activate();
        if (bytes) {
            PMC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
            PMC_HIP(hipStreamSynchronize(c->stream));
        }
    });
}
int pmc_memcpy_d2h(pmc_ctx* c, void* dst, const void* src, size_t bytes) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        c->activate();
        if (bytes) {
            PMC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
            PMC_HIP(hipStreamSynchronize(c->stream));
        }
    });
}

int pmc_rng_seed(pmc_ctx* c, uint64_t seed, int nparts, int mypart) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        PMC_REQUIRE(nparts >= 1 && mypart >= 0 && mypart < nparts, "pmc_rng_seed: need 0 <= mypart < nparts");
        c->seed = seed;
        c->nparts = nparts;
        c->mypart = mypart;
    });
}

int pmc_normal_fill(pmc_ctx* c, double mean, double sigma2, uint64_t first_id, uint32_t stream, int nbatch, int n,
                    double* out, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && out != nullptr, "pmc_normal_fill: NULL argument");
        PMC_REQUIRE(n >= 0 && nbatch >= 0 && sigma2 >= 0.0, "pmc_normal_fill: bad size / variance");
        c->activate();
        const double sigma = std::sqrt(sigma2);   // NormalDistributionSampler ctor, cpp:17-19
        if (memspace == PMC_MEM_DEVICE) {
            k::normal_fill(c->stream, n, nbatch, c->seed, c->stream_id(first_id), stream, mean, sigma, out, (uint64_t)c->nparts);
        } else {
            DevBuf<double> tmp((size_t)n * nbatch);
            k::normal_fill(c->stream, n, nbatch, c->seed, c->stream_id(first_id), stream, mean, sigma, tmp.p, (uint64_t)c->nparts);
            PMC_HIP(hipMemcpyAsync(out, tmp.p, sizeof(double) * n * nbatch, hipMemcpyDeviceToHost, c->stream));
            PMC_HIP(hipStreamSynchronize(c->stream));
        }
    });
}

// ---- sampler -----------------------------------------------------------------------------------
int pmc_sampler_create(pmc_ctx* c, int nlevels, int n_mc_levels, const pmc_sampler_level* levels, double alpha,
                       double matern_g, int lognormal, const pmc_solver_opts* opts, pmc_sampler** out) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && out != nullptr, "pmc_sampler_create: NULL argument");
        *out = nullptr;
        pmc_solver_opts o;
        pmc_solver_opts_default(&o);
        if (opts) {
            check_abi(*opts);
            o = *opts;
        }
        PMC_REQUIRE(o.max_iter >= 1 && o.cheb_degree_M >= 0 && o.mg_smooth_degree >= 1 && o.mg_coarse_degree >= 1 &&
                        (o.cheb_ratio_M <= 0.0 || o.cheb_ratio_M > 1.0) && o.mg_smooth_ratio > 1.0 && o.mg_coarse_ratio > 1.0 &&
                        (o.precond_storage == PMC_STORAGE_FP32 || o.precond_storage == PMC_STORAGE_FP64),
                    "solver options out of range");
        *out = new pmc_sampler(*c, nlevels, n_mc_levels, levels, alpha, matern_g, lognormal != 0, o);
        for (int l = 0; l < (*out)->impl.nlevels; ++l) (*out)->impl.lv[l].out_size = (*out)->impl.lv[l].n_s;
    });
}
int pmc_sampler_create_hybrid(pmc_ctx* c, int nlevels, const pmc_hybrid_level* levels, double alpha, double matern_g,
                              int lognormal, const pmc_solver_opts* opts, pmc_sampler** out) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && out != nullptr, "pmc_sampler_create_hybrid: NULL argument");
        *out = nullptr;
        pmc_solver_opts o;
        pmc_solver_opts_default(&o);
        if (opts) {
            check_abi(*opts);
            o = *opts;
        }
        PMC_REQUIRE(o.max_iter >= 1 && o.mg_smooth_degree >= 1 && o.mg_coarse_degree >= 1 && o.mg_smooth_ratio > 1.0 &&
                        o.mg_coarse_ratio > 1.0 && (o.precond_storage == PMC_STORAGE_FP32 || o.precond_storage == PMC_STORAGE_FP64),
                    "solver options out of range");
        *out = new pmc_sampler(*c, nlevels, levels, alpha, matern_g, lognormal != 0, o);
        for (int l = 0; l < (*out)->impl.nlevels; ++l) (*out)->impl.lv[l].out_size = (*out)->impl.lv[l].n_s;
    });
}
int pmc_sampler_is_hybrid(const pmc_sampler* s) { return s ? (s->impl.hybrid ? 1 : 0) : PMC_ERR_INVALID; }
int pmc_sampler_create_kl(pmc_ctx* c, int nlevels, const pmc_kl_level* levels, int nmodes, const double* evals,
                          const double* evect0, int lognormal, pmc_sampler** out) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && out != nullptr, "pmc_sampler_create_kl: NULL argument");
        *out = nullptr;
        *out = new pmc_sampler(*c, nlevels, levels, nmodes, evals, evect0, lognormal != 0);
    });
}
int pmc_sampler_is_kl(const pmc_sampler* s) { return s ? (s->impl.kl ? 1 : 0) : PMC_ERR_INVALID; }
void pmc_kl_eigs_opts_default(pmc_kl_eigs_opts* o) {
    if (!o) return;
    o->tol = 1e-8;
    o->max_iter = 100;
    o->guard = 16;
    o->degree = 8;
    o->seed = 0;
}
int pmc_kl_matern_apply(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int ncols,
                        const double* X, double* Y) {
    return guarded([&] { kl_matern_apply(c, dim, n, centroids, w_diag, corlen, ncols, X, Y); });
}
int pmc_kl_matern_eigs(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int nmodes,
                       const pmc_kl_eigs_opts* opts, double* evals, double* evect0, pmc_kl_eigs_info* info) {
    return guarded([&] { kl_matern_eigs(c, dim, n, centroids, w_diag, corlen, nmodes, opts, evals, evect0, info); });
}
// entry points that act on the linear system of an SPDE sampler: a KL handle has none
static void refuse_kl(const pmc_sampler* s, const char* what) {
    PMC_REQUIRE(!s->impl.kl, std::string(what) + " is not defined on a KL sampler handle (pmc_sampler_create_kl)");
}
void pmc_sampler_destroy(pmc_sampler* s) {
    if (!s) return;
    (void)hipSetDevice(s->impl.ctx.device);
    (void)hipStreamSynchronize(s->impl.ctx.stream);
    delete s;
}
int pmc_sampler_set_projection(pmc_sampler* s, int level, int kind, const pmc_csr* Gt, const int32_t* idx,
                               const double* inv_w, int orig_size) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        refuse_kl(s, "pmc_sampler_set_projection");
        s->impl.set_projection(level, kind, Gt, idx, inv_w, orig_size);
    });
}
int pmc_sampler_num_levels(const pmc_sampler* s) { return s ? s->impl.n_mc : PMC_ERR_INVALID; }
int pmc_sampler_xi_size(const pmc_sampler* s, int level) {
    if (!s || level < 0 || level >= s->impl.nlevels) return PMC_ERR_INVALID;
    return s->impl.lv[level].n_s;
}
int pmc_sampler_sample_size(const pmc_sampler* s, int level) {
    if (!s || level < 0 || level >= s->impl.nlevels) return PMC_ERR_INVALID;
    return s->impl.lv[level].out_size;
}
int pmc_sampler_krylov_z_bytes(const pmc_sampler* s) {
    return s ? (s->impl.opts.precond_storage == PMC_STORAGE_FP64 ? 8 : 4) : PMC_ERR_INVALID;
}
int pmc_darcy_krylov_z_bytes(const pmc_darcy* d) {
    return d ? (d->impl.opts.precond_storage == PMC_STORAGE_FP64 ? 8 : 4) : PMC_ERR_INVALID;
}
int pmc_sampler_mult(pmc_sampler* s, int level, int nbatch, const double* rhs, double* sol, int use_sol_as_guess,
                     int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        refuse_kl(s, "pmc_sampler_mult");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        s->impl.mult(level, nbatch, rhs, sol, use_sol_as_guess != 0, memspace, stats);
    });
}
int pmc_sampler_apply_preconditioner(pmc_sampler* s, int level, int nbatch, const double* r, double* z, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        refuse_kl(s, "pmc_sampler_apply_preconditioner");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        s->impl.apply_preconditioner(level, nbatch, r, z, memspace);
    });
}
int pmc_sampler_batch_width(const pmc_sampler* s, int level) {
    if (!s || level < 0 || level >= s->impl.nlevels) return PMC_ERR_INVALID;
    return s->impl.launch_width(level);
}
int pmc_sampler_true_p(const pmc_sampler* s, int level, pmc_csr* out) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && out != nullptr, "pmc_sampler_true_p: NULL argument");
        PMC_REQUIRE(level >= 0 && level + 1 < s->impl.nlevels, "pmc_sampler_true_p: level has no coarser level");
        const HostCsr& P = s->impl.lv[level].P_host;
        *out = pmc_csr{P.nrows, P.ncols, P.rowptr.data(), P.colind.data(), P.vals.data()};
    });
}

int64_t pmc_sampler_nnz(const pmc_sampler* s, int level) {
    if (!s || level < 0 || level >= s->impl.nlevels) return PMC_ERR_INVALID;
    return s->impl.lv[level].nnz;
}
int pmc_sampler_sample(pmc_sampler* s, int level, uint64_t first_id, int nbatch, double* xi, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.sample(level, first_id, nbatch, xi, memspace);
    });
}
int pmc_sampler_eval(pmc_sampler* s, int level, int xi_level, int nbatch, const double* xi, double* s_out,
                     const double* init_s, int init_level, int use_init, double* embed_s_out, int memspace,
                     pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.eval(level, xi_level, nbatch, xi, s_out, init_s, init_level, use_init != 0, embed_s_out, memspace, stats);
    });
}

int pmc_sampler_eval_adjoint(pmc_sampler* s, int level, int xi_level, int nbatch, const double* v, const double* s_out,
                             double* grad_xi, int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.eval_adjoint(level, xi_level, nbatch, v, s_out, grad_xi, memspace, stats);
    });
}

int pmc_sampler_logprior_hessvec(pmc_sampler* s, int n, int nbatch, const double* v, double* hv, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.prior_hessvec(n, nbatch, v, hv, memspace);
    });
}
int pmc_sampler_eval_tangent(pmc_sampler* s, int level, int xi_level, int nbatch, const double* v, const double* s_out,
                             double* ds_out, int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.eval_tangent(level, xi_level, nbatch, v, s_out, ds_out, memspace, stats);
    });
}

int pmc_sampler_is_lognormal(const pmc_sampler* s) { return s ? (s->impl.lognormal ? 1 : 0) : PMC_ERR_INVALID; }
int pmc_sampler_logprior_gradient(pmc_sampler* s, int n, int nbatch, const double* xi, double* grad, double* logprior,
                                  int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.prior_gradient(n, nbatch, xi, grad, logprior, memspace);
    });
}

int pmc_conditioner_create(pmc_sampler* s, int nobs, const pmc_csr* H0, const double* y, const double* sigma2,
                           pmc_conditioner** out) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && out != nullptr, "pmc_conditioner_create: NULL argument");
        *out = nullptr;
        *out = new pmc_conditioner(s->impl, nobs, H0, y, sigma2);
    });
}
void pmc_conditioner_destroy(pmc_conditioner* c) {
    if (!c) return;
    (void)hipSetDevice(c->impl.smp.ctx.device);
    (void)hipStreamSynchronize(c->impl.smp.ctx.stream);
    delete c;
}
int pmc_conditioner_num_obs(const pmc_conditioner* c) { return c ? c->impl.nobs : PMC_ERR_INVALID; }
int pmc_conditioner_level(const pmc_conditioner* c, int level, int* n, int64_t* nnz, double* K, double* A, int32_t* rowptr,
                          int32_t* colind, double* vals) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "conditioner is NULL");
        c->impl.export_level(level, n, nnz, K, A, rowptr, colind, vals);
    });
}
int pmc_conditioner_apply(pmc_conditioner* c, int level, int nbatch, const double* g, const double* zeta, double* out,
                          int apply_exp, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "conditioner is NULL");
        c->impl.apply(level, nbatch, g, zeta, out, apply_exp != 0, memspace);
    });
}
int pmc_conditioner_apply_tangent(pmc_conditioner* c, int level, int nbatch, const double* dg, const double* s_out,
                                  double* out, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "conditioner is NULL");
        c->impl.apply_tangent(level, nbatch, dg, s_out, out, memspace);
    });
}
int pmc_conditioner_apply_adjoint(pmc_conditioner* c, int level, int nbatch, const double* v, const double* s_out,
                                  double* out, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "conditioner is NULL");
        c->impl.apply_adjoint(level, nbatch, v, s_out, out, memspace);
    });
}
int pmc_conditioner_enable_derivatives(pmc_conditioner* c, int on) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "conditioner is NULL");
        c->impl.derivs = on != 0;
    });
}
int pmc_conditioner_derivatives_enabled(const pmc_conditioner* c) { return c ? (c->impl.derivs ? 1 : 0) : PMC_ERR_INVALID; }
int pmc_sampler_set_conditioner(pmc_sampler* s, pmc_conditioner* c) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        if (c) {
            PMC_REQUIRE(&c->impl.smp == &s->impl, "pmc_sampler_set_conditioner: the conditioner was created on another handle");
            PMC_REQUIRE(!c->impl.noisy, "pmc_sampler_set_conditioner: the conditioner has sigma2 > 0; Eval receives no realization "
                                        "id to draw independent noise from - use pmc_conditioner_apply with pmc_normal_fill");
            for (int l = 0; l < s->impl.n_mc; ++l)
                PMC_REQUIRE(s->impl.lv[l].proj == PMC_PROJ_NONE, "pmc_sampler_set_conditioner: the handle has a projection set");
        }
        s->impl.cond = c ? &c->impl : nullptr;
    });
}

int pmc_field_stats_create(pmc_sampler* s, int level, const double* chi, int memspace, pmc_field_stats** out) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && out != nullptr, "pmc_field_stats_create: NULL argument");
        *out = new pmc_field_stats(s->impl, level, chi, memspace);
    });
}
void pmc_field_stats_destroy(pmc_field_stats* fs) {
    if (!fs) return;
    (void)hipSetDevice(fs->impl.smp.ctx.device);
    (void)hipStreamSynchronize(fs->impl.smp.ctx.stream);
    delete fs;
}
int pmc_field_stats_reset(pmc_field_stats* fs) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        fs->impl.reset();
    });
}
int pmc_field_stats_accumulate(pmc_field_stats* fs, int nbatch, const double* s, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        fs->impl.accumulate(nbatch, s, memspace);
    });
}
int pmc_field_stats_run(pmc_field_stats* fs, uint64_t first_sample_id, int64_t nsamples) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        fs->impl.run(first_sample_id, nsamples);
    });
}
int pmc_field_stats_read(const pmc_field_stats* fs, double* expectation, double* second_moment, double* chi_cov,
                         int64_t* count, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        const_cast<pmc_field_stats*>(fs)->impl.read(expectation, second_moment, chi_cov, count, memspace);
    });
}
int pmc_field_stats_read_sums(const pmc_field_stats* fs, double* sums, int64_t* count, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        const_cast<pmc_field_stats*>(fs)->impl.read_sums(sums, count, memspace);
    });
}
int pmc_field_stats_chi_dot(const pmc_field_stats* fs, int nbatch, const double* s, double* dots, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(fs != nullptr, "field stats is NULL");
        const_cast<pmc_field_stats*>(fs)->impl.chi_dots(nbatch, s, dots, memspace);
    });
}
int pmc_sampler_l2_error(pmc_sampler* s, int level, int nbatch, const double* coeff, double exact, double* err,
                         int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.field_error(level, nbatch, coeff, exact, err, memspace, false);
    });
}
int pmc_sampler_max_error(pmc_sampler* s, int level, int nbatch, const double* coeff, double exact, double* err,
                          int memspace) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.field_error(level, nbatch, coeff, exact, err, memspace, true);
    });
}
int pmc_sampler_set_output_hierarchy(pmc_sampler* s, int nlevels, const pmc_csr* P_orig, const double* w0_orig) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.set_output_hierarchy(nlevels, P_orig, w0_orig);
    });
}
int pmc_sampler_apply_operator(pmc_sampler* s, int level, int nbatch, const double* x, double* y, int memspace,
                               int repeat, double* avg_ms, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        refuse_kl(s, "pmc_sampler_apply_operator");
        s->impl.apply_operator(level, nbatch, x, y, memspace, repeat, avg_ms, bytes);
    });
}

int pmc_sampler_set_operator_timing(pmc_sampler* s, int on) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        s->impl.work.op_timer.on = on != 0;
    });
}

int pmc_sampler_operator_time(pmc_sampler* s, double* total_ms, int64_t* launches) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        if (total_ms) *total_ms = s->impl.work.op_timer.ms;
        if (launches) *launches = s->impl.work.op_timer.launches;
        s->impl.work.op_timer.ms = 0.0;
        s->impl.work.op_timer.launches = 0;
    });
}

int pmc_sampler_smoother_time(pmc_sampler* s, double* total_ms, int64_t* launches, double* event_overhead_ms) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr, "sampler is NULL");
        if (total_ms) *total_ms = s->impl.vc_timer.ms;
        if (launches) *launches = s->impl.vc_timer.launches;
        if (event_overhead_ms) *event_overhead_ms = s->impl.vc_timer.gap_ms;
        s->impl.vc_timer.clear();
    });
}
int pmc_sampler_smoother_bytes(const pmc_sampler* s, int level, int nbatch, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && bytes != nullptr, "pmc_sampler_smoother_bytes: NULL argument");
        *bytes = s->impl.smoother_bytes(level, nbatch);
    });
}

// The two-call CSR export of the prolongator entry points: sizes always (*nnz holds the arrays' capacity on entry), the arrays
// when all three are given
static void export_csr(const HostCsr& P, int* nrows, int* ncols, int64_t* nnz, int32_t* rowptr, int32_t* colind, double* vals,
                       const char* too_small) {
    const int64_t cap = *nnz;
    *nrows = P.nrows;
    *ncols = P.ncols;
    *nnz = (int64_t)P.colind.size();
    if (rowptr == nullptr && colind == nullptr && vals == nullptr) return;   // size query
    PMC_REQUIRE(rowptr != nullptr && colind != nullptr && vals != nullptr && cap >= *nnz, too_small);
    std::copy(P.rowptr.begin(), P.rowptr.end(), rowptr);
    std::copy(P.colind.begin(), P.colind.end(), colind);
    std::copy(P.vals.begin(), P.vals.end(), vals);
}

int pmc_sampler_vcycle_info(const pmc_sampler* s, int level, int vlevel, int* nvlevels, int64_t info[7]) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && nvlevels != nullptr && info != nullptr, "pmc_sampler_vcycle_info: NULL argument");
        refuse_kl(s, "pmc_sampler_vcycle_info");
        s->impl.vcycle_info(level, vlevel, nvlevels, info);
    });
}

int pmc_sampler_vcycle_level(const pmc_sampler* s, int level, int vlevel, int* nvlevels, double info[15]) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && nvlevels != nullptr && info != nullptr, "pmc_sampler_vcycle_level: NULL argument");
        refuse_kl(s, "pmc_sampler_vcycle_level");
        s->impl.vcycle_level(level, vlevel, nvlevels, info);
    });
}
int pmc_sampler_vcycle_prolongator(const pmc_sampler* s, int level, int vlevel, int* nrows, int* ncols, int64_t* nnz,
                                   int32_t* rowptr, int32_t* colind, double* vals) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && nrows != nullptr && ncols != nullptr && nnz != nullptr,
                    "pmc_sampler_vcycle_prolongator: NULL argument");
        refuse_kl(s, "pmc_sampler_vcycle_prolongator");
        HostCsr scratch;
        const HostCsr& P = s->impl.vcycle_prolongator(level, vlevel, scratch);
        export_csr(P, nrows, ncols, nnz, rowptr, colind, vals, "pmc_sampler_vcycle_prolongator: arrays missing or smaller than nnz");
    });
}

int pmc_sampler_operator_event_overhead(pmc_sampler* s, double* total_ms) {
    return guarded([&] {
        PMC_REQUIRE(s != nullptr && total_ms != nullptr, "operator_event_overhead: bad arguments");
        *total_ms = s->impl.work.op_timer.gap_ms;
        s->impl.work.op_timer.gap_ms = 0.0;
    });
}

// ---- Darcy ------------------------------------------------------------------------------------
static int darcy_create(pmc_ctx* c, int nlevels, int n_mc_levels, const pmc_darcy_level* levels, int k_divides,
                        const pmc_solver_opts* opts, pmc_darcy** out, bool hybrid) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && out != nullptr, "pmc_darcy_create: NULL argument");
        *out = nullptr;
        pmc_solver_opts o;
        pmc_solver_opts_default(&o);
        if (opts) {
            check_abi(*opts);
            o = *opts;
        }
        PMC_REQUIRE(o.max_iter >= 1 && o.cheb_degree_M >= 0 && o.mg_smooth_degree >= 1 && o.mg_coarse_degree >= 1 &&
                        (o.cheb_ratio_M <= 0.0 || o.cheb_ratio_M > 1.0) && o.mg_smooth_ratio > 1.0 && o.mg_coarse_ratio > 1.0 &&
                        (o.precond_storage == PMC_STORAGE_FP32 || o.precond_storage == PMC_STORAGE_FP64),
                    "solver options out of range");
        *out = new pmc_darcy(*c, nlevels, n_mc_levels, levels, k_divides != 0, o, hybrid);
    });
}
int pmc_darcy_create(pmc_ctx* c, int nlevels, int n_mc_levels, const pmc_darcy_level* levels, int k_divides,
                     const pmc_solver_opts* opts, pmc_darcy** out) {
    return darcy_create(c, nlevels, n_mc_levels, levels, k_divides, opts, out, false);
}
int pmc_darcy_create_hybrid(pmc_ctx* c, int nlevels, int n_mc_levels, const pmc_darcy_level* levels, int k_divides,
                            const pmc_solver_opts* opts, pmc_darcy** out) {
    return darcy_create(c, nlevels, n_mc_levels, levels, k_divides, opts, out, true);
}
void pmc_darcy_destroy(pmc_darcy* d) {
    if (!d) return;
    (void)hipSetDevice(d->impl.ctx.device);
    (void)hipStreamSynchronize(d->impl.ctx.stream);
    delete d;
}
// ---- batched CG vector algebra (newton_cg.hip) ----
int pmc_ncg_create(pmc_ctx* ctx, int n, int nbatch_max, pmc_ncg** out) {
    return guarded([&] {
        PMC_REQUIRE(ctx != nullptr && out != nullptr, "pmc_ncg_create: NULL argument");
        *out = nullptr;
        *out = new pmc_ncg(*ctx, n, nbatch_max);
    });
}
void pmc_ncg_destroy(pmc_ncg* w) { delete w; }
int pmc_ncg_begin(pmc_ncg* w, int nb, const double* g, const double* eta, const int32_t* active_mask, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(w != nullptr, "pmc_ncg_begin: workspace is NULL");
        w->impl.begin(nb, g, eta, active_mask, memspace);
    });
}
int pmc_ncg_step(pmc_ncg* w, int nb, const double* Hp, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(w != nullptr, "pmc_ncg_step: workspace is NULL");
        w->impl.step(nb, Hp, memspace);
    });
}
double* pmc_ncg_direction(pmc_ncg* w) { return w ? w->impl.d.p : nullptr; }
double* pmc_ncg_search_direction(pmc_ncg* w) { return w ? w->impl.p.p : nullptr; }
double* pmc_ncg_residual(pmc_ncg* w) { return w ? w->impl.r.p : nullptr; }
int pmc_ncg_status(pmc_ncg* w, int nb, double* rr, int32_t* cg_count, int32_t* done, int32_t* nonpos_curvature) {
    return guarded([&] {
        PMC_REQUIRE(w != nullptr, "pmc_ncg_status: workspace is NULL");
        w->impl.status(nb, rr, cg_count, done, nonpos_curvature);
    });
}
int pmc_ncg_axpy_cols(pmc_ncg* w, int nb, const double* t, const double* x, const double* d, double* out, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(w != nullptr, "pmc_ncg_axpy_cols: workspace is NULL");
        w->impl.axpy(nb, t, x, d, out, memspace);
    });
}
int pmc_ncg_dot_cols(pmc_ncg* w, int nb, const double* a, const double* b, double* out_host, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(w != nullptr, "pmc_ncg_dot_cols: workspace is NULL");
        w->impl.dot(nb, a, b, out_host, memspace);
    });
}

// ---- particle travel times (tracer.hip) ----
int pmc_tracer_create(pmc_ctx* ctx, const pmc_tracer_mesh* mesh, int nparticles, const double* x0, const int32_t* elem0,
                      int max_steps, pmc_tracer** out) {
    return guarded([&] {
        PMC_REQUIRE(ctx != nullptr && mesh != nullptr && out != nullptr, "pmc_tracer_create: NULL argument");
        *out = nullptr;
        *out = new pmc_tracer(*ctx, *mesh, nparticles, x0, elem0, max_steps);
    });
}
void pmc_tracer_destroy(pmc_tracer* t) {
    if (!t) return;
    (void)hipSetDevice(t->impl.ctx.device);
    (void)hipStreamSynchronize(t->impl.ctx.stream);
    delete t;
}
int pmc_tracer_num_particles(const pmc_tracer* t) { return t ? t->impl.npart : PMC_ERR_INVALID; }
int pmc_tracer_run(pmc_tracer* t, int nbatch, const double* u, int64_t ld, double* T, int32_t* exit_face, int32_t* status,
                   int32_t* nsteps, double* x_exit, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_tracer_run: tracer is NULL");
        t->impl.run(nbatch, u, ld, T, exit_face, status, nsteps, x_exit, memspace);
    });
}
int pmc_tracer_reduce(pmc_tracer* t, int nbatch, const double* T, const int32_t* status, int kind, double* Q,
                      int32_t* not_exited, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_tracer_reduce: tracer is NULL");
        t->impl.reduce(nbatch, T, status, kind, Q, not_exited, memspace);
    });
}
int pmc_darcy_set_tracer(pmc_darcy* d, int level, pmc_tracer* t, int kind) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_set_tracer: darcy is NULL");
        d->impl.set_tracer(level, t ? &t->impl : nullptr, kind);
    });
}
int pmc_tracer_run_adjoint(pmc_tracer* t, int nbatch, const double* u, int64_t ld, const double* T_bar, const double* x_exit_bar,
                           double* u_bar, int64_t ld_bar, double* x0_bar, double* T, int32_t* exit_face, int32_t* status,
                           int32_t* nsteps, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_tracer_run_adjoint: tracer is NULL");
        t->impl.run_adjoint(nbatch, u, ld, T_bar, x_exit_bar, u_bar, ld_bar, x0_bar, T, exit_face, status, nsteps, memspace);
    });
}
int pmc_tracer_reduce_seed(pmc_tracer* t, int nbatch, const double* T, const int32_t* status, int kind, double* T_bar, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_tracer_reduce_seed: tracer is NULL");
        t->impl.reduce_seed(nbatch, T, status, kind, T_bar, memspace);
    });
}
int pmc_tracer_set_adjoint_scratch(pmc_tracer* t, int64_t bytes) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_tracer_set_adjoint_scratch: tracer is NULL");
        t->impl.set_adjoint_scratch(bytes);
    });
}
int pmc_tracer_adjoint_chunks(const pmc_tracer* t) { return t ? t->impl.adj_chunks : PMC_ERR_INVALID; }
int pmc_darcy_tracer_gradient(pmc_darcy* d, int level, pmc_tracer* t, int nbatch, const double* k, const double* T_bar, int wrt_log,
                              double* T, int32_t* status, double* grad, double* sol_out, double* adj_out, int memspace,
                              pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_tracer_gradient: darcy is NULL");
        d->impl.tracer_gradient(level, t ? &t->impl : nullptr, nbatch, k, T_bar, wrt_log != 0, T, status, grad, sol_out, adj_out,
                                memspace, stats_fwd, stats_adj);
    });
}
int pmc_darcy_tracer_loglik_gradient(pmc_darcy* d, int level, pmc_tracer* t, int nbatch, const double* k, const double* data,
                                     double noise, int wrt_log, double* loglik, double* T, int32_t* not_exited, double* grad,
                                     int memspace, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_tracer_loglik_gradient: darcy is NULL");
        d->impl.tracer_loglik_gradient(level, t ? &t->impl : nullptr, nbatch, k, data, noise, wrt_log != 0, loglik, T, not_exited,
                                       grad, memspace, stats_adj);
    });
}

// ---- upwind solute transport (transport.hip) ----
int pmc_transport_create(pmc_ctx* ctx, const pmc_transport_mesh* mesh, const pmc_transport_params* params, pmc_transport** out) {
    return guarded([&] {
        PMC_REQUIRE(ctx != nullptr && mesh != nullptr && params != nullptr && out != nullptr, "pmc_transport_create: NULL argument");
        *out = nullptr;
        *out = new pmc_transport(*ctx, *mesh, *params);
    });
}
void pmc_transport_destroy(pmc_transport* t) {
    if (!t) return;
    (void)hipSetDevice(t->impl.ctx.device);
    (void)hipStreamSynchronize(t->impl.ctx.stream);
    delete t;
}
int pmc_transport_size(const pmc_transport* t, int* n_elem, int* n_face, int* n_outlet, int* nreport) {
    if (!t) return PMC_ERR_INVALID;
    if (n_elem) *n_elem = t->impl.n_elem;
    if (n_face) *n_face = t->impl.n_face;
    if (n_outlet) *n_outlet = t->impl.n_outlet;
    if (nreport) *nreport = t->impl.nreport;
    return PMC_OK;
}
int pmc_transport_run(pmc_transport* t, int nbatch, const double* u, int64_t ld, double* c_out, double* curve, double* stored,
                      double* rate, double* t_reached, int32_t* nsteps, int32_t* status, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_transport_run: transport is NULL");
        t->impl.run(nbatch, u, ld, c_out, curve, stored, rate, t_reached, nsteps, status, memspace);
    });
}
int pmc_transport_reduce(pmc_transport* t, int nbatch, const double* curve, const double* stored, int kind, double* Q, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_transport_reduce: transport is NULL");
        t->impl.reduce(nbatch, curve, stored, kind, Q, memspace);
    });
}
int pmc_darcy_set_transport(pmc_darcy* d, int level, pmc_transport* t, int kind) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_set_transport: darcy is NULL");
        d->impl.set_transport(level, t ? &t->impl : nullptr, kind);
    });
}
int pmc_transport_run_adjoint(pmc_transport* t, int nbatch, const double* u, int64_t ld, const double* curve_bar,
                              const double* stored_bar, const double* c_bar, double* u_bar, int64_t ld_bar, double* c0_bar,
                              double* curve, double* stored, int32_t* nsteps, int32_t* status, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_transport_run_adjoint: transport is NULL");
        t->impl.run_adjoint(nbatch, u, ld, curve_bar, stored_bar, c_bar, u_bar, ld_bar, c0_bar, curve, stored, nsteps, status, memspace);
    });
}
int pmc_transport_set_adjoint_segment(pmc_transport* t, int K) {
    return guarded([&] {
        PMC_REQUIRE(t != nullptr, "pmc_transport_set_adjoint_segment: transport is NULL");
        t->impl.set_adjoint_segment(K);
    });
}
int pmc_darcy_transport_gradient(pmc_darcy* d, int level, pmc_transport* t, int nbatch, const double* k, const double* curve_bar,
                                 const double* stored_bar, int wrt_log, double* curve, double* stored, int32_t* status, double* grad,
                                 double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_transport_gradient: darcy is NULL");
        d->impl.transport_gradient(level, t ? &t->impl : nullptr, nbatch, k, curve_bar, stored_bar, wrt_log != 0, curve, stored, status,
                                   grad, sol_out, adj_out, memspace, stats_fwd, stats_adj);
    });
}
int pmc_darcy_transport_loglik_gradient(pmc_darcy* d, int level, pmc_transport* t, int nbatch, const double* k, const double* data,
                                        double noise, int wrt_log, double* loglik, double* curve, int32_t* status, double* grad,
                                        int memspace, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "pmc_darcy_transport_loglik_gradient: darcy is NULL");
        d->impl.transport_loglik_gradient(level, t ? &t->impl : nullptr, nbatch, k, data, noise, wrt_log != 0, loglik, curve, status,
                                          grad, memspace, stats_adj);
    });
}

int pmc_darcy_num_dofs(const pmc_darcy* d, int level) {
    if (!d || level < 0 || level >= d->impl.nlevels) return PMC_ERR_INVALID;
    return d->impl.lv[level].n_u + d->impl.lv[level].n_p;
}
int pmc_darcy_num_pressure_dofs(const pmc_darcy* d, int level) {
    if (!d || level < 0 || level >= d->impl.nlevels) return PMC_ERR_INVALID;
    return d->impl.lv[level].n_p;
}
int pmc_darcy_set_operator_timing(pmc_darcy* d, int on) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy handle is NULL");
        d->impl.op_timer.on = on != 0;
        d->impl.poly_timer.on = on != 0;
        d->impl.grad_timer.on = on != 0;
        d->impl.tan_timer.on = on != 0;
    });
}
int pmc_darcy_operator_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy handle is NULL");
        if (total_ms) *total_ms = d->impl.op_timer.ms;
        if (launches) *launches = d->impl.op_timer.launches;
        if (event_overhead_ms) *event_overhead_ms = d->impl.op_timer.gap_ms;
        d->impl.op_timer.clear();
    });
}
int pmc_darcy_operator_bytes(const pmc_darcy* d, int level, int nbatch, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && bytes != nullptr && level >= 0 && level < d->impl.nlevels && valid_batch(nbatch),
                    "pmc_darcy_operator_bytes: bad arguments");
        *bytes = d->impl.operator_bytes(level, nbatch);
    });
}
int pmc_darcy_poly_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy handle is NULL");
        if (total_ms) *total_ms = d->impl.poly_timer.ms;
        if (launches) *launches = d->impl.poly_timer.launches;
        if (event_overhead_ms) *event_overhead_ms = d->impl.poly_timer.gap_ms;
        d->impl.poly_timer.clear();
    });
}
int pmc_darcy_poly_bytes(const pmc_darcy* d, int level, int nbatch, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && bytes != nullptr && level >= 0 && level < d->impl.nlevels && valid_batch(nbatch),
                    "pmc_darcy_poly_bytes: bad arguments");
        *bytes = d->impl.poly_bytes(level, nbatch);
    });
}
int pmc_darcy_mass_sensitivity_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy handle is NULL");
        if (total_ms) *total_ms = d->impl.grad_timer.ms;
        if (launches) *launches = d->impl.grad_timer.launches;
        if (event_overhead_ms) *event_overhead_ms = d->impl.grad_timer.gap_ms;
        d->impl.grad_timer.clear();
    });
}
int pmc_darcy_mass_sensitivity_bytes(pmc_darcy* d, int level, int nbatch, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && bytes != nullptr && level >= 0 && level < d->impl.n_mc && valid_batch(nbatch),
                    "pmc_darcy_mass_sensitivity_bytes: bad arguments");
        *bytes = d->impl.mass_sensitivity_bytes(level, nbatch);
    });
}
int pmc_darcy_mass_tangent_time(pmc_darcy* d, double* total_ms, int64_t* launches, double* event_overhead_ms) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy handle is NULL");
        if (total_ms) *total_ms = d->impl.tan_timer.ms;
        if (launches) *launches = d->impl.tan_timer.launches;
        if (event_overhead_ms) *event_overhead_ms = d->impl.tan_timer.gap_ms;
        d->impl.tan_timer.clear();
    });
}
int pmc_darcy_mass_tangent_bytes(pmc_darcy* d, int level, int nbatch, double* bytes) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && bytes != nullptr && level >= 0 && level < d->impl.n_mc && valid_batch(nbatch),
                    "pmc_darcy_mass_tangent_bytes: bad arguments");
        *bytes = d->impl.mass_tangent_bytes(level, nbatch);
    });
}
int pmc_darcy_batch_width(const pmc_darcy* d, int level) {
    if (!d || level < 0 || level >= d->impl.nlevels) return PMC_ERR_INVALID;
    return batch_width((size_t)d->impl.lv[level].n_u + d->impl.lv[level].n_p, true, d->impl.ctx.device);
}
int64_t pmc_darcy_nnz(const pmc_darcy* d, int level) {
    if (!d || level < 0 || level >= d->impl.nlevels) return PMC_ERR_INVALID;
    return d->impl.lv[level].nnz;
}
int pmc_darcy_solve_fwd(pmc_darcy* d, int level, int nbatch, const double* kf, double* Q, double* C, double* sol_out,
                        int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        d->impl.solve_fwd(level, nbatch, kf, Q, C, sol_out, memspace, stats);
    });
}

int pmc_darcy_solve_fwd_pressure(pmc_darcy* d, int level, int nbatch, const double* kf, double* p_out, double* C,
                                 double* Q, int compute_Q, int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && p_out != nullptr, "SolveFwd_RtnPressure: NULL argument");
        PMC_REQUIRE(nbatch >= 1, "SolveFwd_RtnPressure: bad batch");
        std::vector<double> q(nbatch);
        d->impl.solve_fwd(level, nbatch, kf, q.data(), C, p_out, memspace, stats, 2);
        if (compute_Q && Q)
            for (int b = 0; b < nbatch; ++b) Q[b] = q[b];
    });
}

int pmc_level_fields_create(pmc_ctx* ctx, const pmc_darcy* d, int level, int coupled, pmc_level_fields** out) {
    return guarded([&] {
        PMC_REQUIRE(ctx != nullptr && d != nullptr && out != nullptr, "pmc_level_fields_create: NULL argument");
        *out = new pmc_level_fields(*ctx, d->impl, level, coupled != 0);
    });
}
void pmc_level_fields_destroy(pmc_level_fields* f) {
    if (!f) return;
    (void)hipSetDevice(f->impl.ctx.device);
    (void)hipStreamSynchronize(f->impl.ctx.stream);
    delete f;
}
int pmc_level_fields_reset(pmc_level_fields* f) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr, "level fields is NULL");
        f->impl.reset();
    });
}
int pmc_level_fields_accumulate(pmc_level_fields* f, int nbatch, const double* p_fine, const double* p_coarse, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr, "level fields is NULL");
        f->impl.accumulate(nbatch, p_fine, p_coarse, memspace);
    });
}
int pmc_level_fields_accumulate_weighted(pmc_level_fields* f, int nbatch, const double* x_fine, const double* w_fine,
                                         const double* x_coarse, const double* w_coarse, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr, "level fields is NULL");
        f->impl.accumulate_weighted(nbatch, x_fine, w_fine, x_coarse, w_coarse, memspace);
    });
}
int pmc_level_fields_read_sums(const pmc_level_fields* f, double* sums, int64_t* count, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr, "level fields is NULL");
        const_cast<pmc_level_fields*>(f)->impl.read_sums(sums, count, memspace);
    });
}
int pmc_level_fields_size(const pmc_level_fields* f, int* n_fine, int* n_coarse) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr, "level fields is NULL");
        if (n_fine) *n_fine = f->impl.n;
        if (n_coarse) *n_coarse = f->impl.nc;
    });
}
int pmc_level_fields_parents(const pmc_level_fields* f, int32_t* parent) {
    return guarded([&] {
        PMC_REQUIRE(f != nullptr && parent != nullptr, "pmc_level_fields_parents: NULL argument");
        PMC_REQUIRE(f->impl.coupled, "pmc_level_fields_parents: the level was created without a coarse partner");
        for (int i = 0; i < f->impl.n; ++i) parent[i] = f->impl.parent_host[i];
    });
}

int pmc_darcy_apply_preconditioner(pmc_darcy* d, int level, int nbatch, const double* k, const double* r, double* z,
                                   int memspace) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.apply_preconditioner(level, nbatch, k, r, z, memspace);
    });
}
int pmc_darcy_apply_operator(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, double* y, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.apply_operator(level, nbatch, k, x, y, memspace);
    });
}
int pmc_darcy_vcycle_level(const pmc_darcy* d, int level, int vlevel, int* nvlevels, double info[11]) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && nvlevels != nullptr && info != nullptr, "pmc_darcy_vcycle_level: NULL argument");
        d->impl.vcycle_level(level, vlevel, nvlevels, info);
    });
}
int pmc_darcy_vcycle_prolongator(const pmc_darcy* d, int level, int vlevel, int* nrows, int* ncols, int64_t* nnz,
                                 int32_t* rowptr, int32_t* colind, double* vals) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr && nrows != nullptr && ncols != nullptr && nnz != nullptr,
                    "pmc_darcy_vcycle_prolongator: NULL argument");
        const HostCsr& P = d->impl.vcycle_prolongator(level, vlevel);
        export_csr(P, nrows, ncols, nnz, rowptr, colind, vals, "pmc_darcy_vcycle_prolongator: arrays missing or smaller than nnz");
    });
}
int pmc_darcy_set_observations(pmc_darcy* d, int level, const pmc_csr* Gobs) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        d->impl.set_observations(level, Gobs);
    });
}
int pmc_darcy_num_observations(const pmc_darcy* d, int level) {
    if (!d || level < 0 || level >= d->impl.nlevels) return PMC_ERR_INVALID;
    return d->impl.lv[level].n_gobs;
}
int pmc_darcy_compute_G(pmc_darcy* d, int level, int nbatch, const double* kf, double* G, double* C, double* Q,
                        int memspace, pmc_stats* stats) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        d->impl.compute_G(level, nbatch, kf, G, C, Q, memspace, stats);
    });
}
int pmc_darcy_mass_sensitivity(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, const double* lam,
                               int wrt_log, double* grad, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.mass_sensitivity(level, nbatch, k, x, lam, wrt_log != 0, grad, memspace);
    });
}
int pmc_darcy_solve_gradient(pmc_darcy* d, int level, int nbatch, const double* k, const double* adj_rhs, int wrt_log,
                             double* Q, double* C, double* grad, double* sol_out, double* adj_out, int memspace,
                             pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.solve_gradient(level, nbatch, k, adj_rhs, wrt_log != 0, Q, C, grad, sol_out, adj_out, memspace, stats_fwd,
                               stats_adj);
    });
}
int pmc_darcy_loglik_gradient(pmc_darcy* d, int level, int nbatch, const double* k, const double* data, double noise,
                              int wrt_log, double* loglik, double* G, double* grad, int memspace, pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.loglik_gradient(level, nbatch, k, data, noise, wrt_log != 0, loglik, G, grad, memspace, stats_adj);
    });
}
int pmc_darcy_mass_tangent(pmc_darcy* d, int level, int nbatch, const double* k, const double* x, const double* dk,
                           int wrt_log, double* t_out, int memspace) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.mass_tangent(level, nbatch, k, x, dk, wrt_log != 0, t_out, memspace);
    });
}
int pmc_darcy_gn_hessvec(pmc_darcy* d, int level, int nbatch, const double* k, const double* x_in, const double* dk,
                         double noise, int wrt_log, double* hv, double* dG, double* x_out, int memspace, pmc_stats* stats_tan,
                         pmc_stats* stats_adj) {
    return guarded([&] {
        PMC_REQUIRE(d != nullptr, "darcy is NULL");
        PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "bad memspace");
        d->impl.gn_hessvec(level, nbatch, k, x_in, dk, noise, wrt_log != 0, hv, dG, x_out, memspace, stats_tan, stats_adj);
    });
}

// ---- communicator -----------------------------------------------------------------------------
int pmc_comm_unique_id(void* id128) {
    return guarded([&] {
        PMC_REQUIRE(id128 != nullptr, "id buffer is NULL");
        UniqueId id;
        rccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(id128, &id, sizeof(id));
    });
}
int pmc_comm_init(pmc_ctx* c, const void* id128, int nranks, int rank) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && id128 != nullptr, "pmc_comm_init: NULL argument");
        PMC_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "pmc_comm_init: bad rank");
        c->activate();
        UniqueId id;
        std::memcpy(&id, id128, sizeof(id));
        rccl_check(rccl().CommInitRank(&c->nccl, nranks, id, rank), "ncclCommInitRank");
        c->nranks = nranks;
        c->rank = rank;
    });
}
int pmc_comm_destroy(pmc_ctx* c) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr, "ctx is NULL");
        if (c->nccl) {
            c->activate();
            rccl_check(rccl().CommDestroy(c->nccl), "ncclCommDestroy");
            c->nccl = nullptr;
        }
        c->nranks = 1;
        c->rank = 0;
    });
}
int pmc_allreduce_sum_f64(pmc_ctx* c, double* host_buf, int n) {
    return guarded([&] {
        PMC_REQUIRE(c != nullptr && (host_buf != nullptr || n == 0) && n >= 0, "pmc_allreduce_sum_f64: bad argument");
        if (n == 0) return;
        if (c->nccl == nullptr) {
            PMC_REQUIRE(c->nranks == 1, "pmc_allreduce_sum_f64: communicator not initialised");
            return;   // single rank without a communicator: the sum is the buffer itself
        }
        c->activate();
        c->comm_buf.ensure((size_t)n);
        PMC_HIP(hipMemcpyAsync(c->comm_buf.p, host_buf, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        rccl_check(rccl().AllReduce(c->comm_buf.p, c->comm_buf.p, (size_t)n, /*ncclDouble*/ 8, /*ncclSum*/ 0, c->nccl,
                                    c->stream),
                   "ncclAllReduce");
        PMC_HIP(hipMemcpyAsync(host_buf, c->comm_buf.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        PMC_HIP(hipStreamSynchronize(c->stream));
    });
}

}  // extern "C"

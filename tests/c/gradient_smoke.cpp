// The adjoint gradients through the mirror classes of parelagmc.hpp: DarcySolver::SolveFwd_Gradient and
// BayesianInverseProblem::ComputeGradLogLikelihood (and the C entry pmc_bayes_loglik_gradient) return the values of
// pmc_darcy_solve_gradient / pmc_darcy_loglik_gradient bit for bit, in host and in device memory.
// Usage: gradient_smoke problem.bin      exit code 0 and a final line "gradient_smoke OK" on success.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../parelagmc_amd/host/parelagmc.hpp"

extern "C" {
#include "prob_io.h"
}

using namespace parelagmc;

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        int rc_ = (call);                                                                                    \
        if (rc_ != PMC_OK) { std::fprintf(stderr, "%s -> %d: %s / %s\n", #call, rc_, pmc_last_error(), pmc_host_last_error()); return 1; } \
    } while (0)

static pmc_csr as_csr(const t_csr* a) {
    pmc_csr c;
    c.nrows = a->nrows; c.ncols = a->ncols; c.rowptr = a->rp; c.colind = a->ci; c.vals = a->v;
    return c;
}
static bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: gradient_smoke problem.bin\n"); return 2; }
    t_problem p = t_load(argv[1]);
    pmc_ctx* ctx = nullptr;
    CHECK(pmc_ctx_create(0, &ctx));
    pmc_solver_opts opts;
    pmc_solver_opts_default(&opts);
    std::vector<pmc_darcy_level> dl((size_t)p.d_nlevels);
    for (int l = 0; l < p.d_nlevels; ++l) {
        const t_dlevel* L = &p.dl[l];
        std::memset(&dl[l], 0, sizeof(pmc_darcy_level));
        dl[l].n_u = L->n_u; dl[l].n_p = L->n_p;
        dl[l].M_pattern = as_csr(&L->M);
        dl[l].c_ptr = L->c_ptr; dl[l].c_elem = L->c_elem; dl[l].c_val = L->c_val;
        dl[l].B = as_csr(&L->B);
        dl[l].rhs = L->rhs; dl[l].ess_mask = L->ess; dl[l].ess_data = L->ess_data; dl[l].obs = L->obs;
        if (L->has_p) dl[l].P = as_csr(&L->P);
    }
    pmc_darcy* dar = nullptr;
    CHECK(pmc_darcy_create(ctx, p.d_nlevels, p.d_nlevels, dl.data(), p.k_divides, &opts, &dar));
    const int np = p.dl[0].n_p, nb = p.nbatch;
    // two observation functionals: one cell, and a pair of cells
    int32_t rp[3] = {0, 1, 3}, ci[3] = {np / 3, 2 * np / 3, 2 * np / 3 + 1};
    double gv[3] = {1.0, 0.5, 1.5};
    pmc_csr G;
    G.nrows = 2; G.ncols = np; G.rowptr = rp; G.colind = ci; G.vals = gv;
    CHECK(pmc_darcy_set_observations(dar, 0, &G));
    const std::vector<double> data = {0.25, -0.5};
    const double noise = 0.01;
    int rc = 1;
    try {
        DarcySolver ds(ctx, dar);
        BayesianInverseProblem bip(dar, noise, data);
        for (int wrt_log = 0; wrt_log < 2; ++wrt_log) {
            std::vector<double> Q(nb), C(nb), g((size_t)nb * np), Qc(nb), Cc(nb), ll(nb), llc(nb), llh(nb), gh((size_t)nb * np);
            CHECK(pmc_darcy_solve_gradient(dar, 0, nb, p.k[0], nullptr, wrt_log, Q.data(), C.data(), g.data(), nullptr, nullptr,
                                           PMC_MEM_HOST, nullptr, nullptr));
            Vector k(ctx, PMC_MEM_HOST), grad(ctx, PMC_MEM_HOST);
            k.SetSize(np, nb);
            std::memcpy(k.GetData(), p.k[0], sizeof(double) * (size_t)np * nb);
            ds.SolveFwd_Gradient(0, k, Qc.data(), Cc.data(), grad, wrt_log != 0);
            if (grad.Size() != np || grad.Batch() != nb || !same_bits(grad.GetData(), g.data(), g.size()) ||
                !same_bits(Qc.data(), Q.data(), Q.size()) || !same_bits(Cc.data(), C.data(), C.size())) {
                std::fprintf(stderr, "DarcySolver::SolveFwd_Gradient differs from pmc_darcy_solve_gradient (host)\n");
                return 1;
            }
            Vector kd(ctx, PMC_MEM_DEVICE), gd(ctx, PMC_MEM_DEVICE);
            kd.SetSize(np, nb);
            CHECK(pmc_memcpy_h2d(ctx, kd.GetData(), p.k[0], sizeof(double) * (size_t)np * nb));
            ds.SolveFwd_Gradient(0, kd, Qc.data(), Cc.data(), gd, wrt_log != 0);
            CHECK(pmc_memcpy_d2h(ctx, gh.data(), gd.GetData(), sizeof(double) * gh.size()));
            if (!same_bits(gh.data(), g.data(), g.size()) || !same_bits(Qc.data(), Q.data(), Q.size())) {
                std::fprintf(stderr, "DarcySolver::SolveFwd_Gradient differs from pmc_darcy_solve_gradient (device)\n");
                return 1;
            }
            CHECK(pmc_darcy_loglik_gradient(dar, 0, nb, p.k[0], data.data(), noise, wrt_log, ll.data(), nullptr, g.data(),
                                            PMC_MEM_HOST, nullptr));
            bip.ComputeGradLogLikelihood(0, k, llc.data(), grad, wrt_log != 0);
            CHECK(pmc_bayes_loglik_gradient(dar, 0, nb, p.k[0], PMC_MEM_HOST, data.data(), (int)data.size(), noise, wrt_log,
                                            llh.data(), gh.data()));
            if (!same_bits(grad.GetData(), g.data(), g.size()) || !same_bits(llc.data(), ll.data(), ll.size()) ||
                !same_bits(gh.data(), g.data(), g.size()) || !same_bits(llh.data(), ll.data(), ll.size())) {
                std::fprintf(stderr, "ComputeGradLogLikelihood differs from pmc_darcy_loglik_gradient\n");
                return 1;
            }
            std::printf("wrt_log %d: Q[0] %.17g loglik[0] %.17g grad[0] %.17g\n", wrt_log, Q[0], ll[0], g[0]);
        }
        rc = 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
    }
    pmc_darcy_destroy(dar);
    pmc_ctx_destroy(ctx);
    if (rc == 0) std::printf("gradient_smoke OK\n");
    return rc;
}

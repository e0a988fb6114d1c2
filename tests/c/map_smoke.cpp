// MAP estimation through the mirror classes of parelagmc.hpp: BayesianInverseProblem::ComputeMAP returns what the C entry
// pmc_bayes_map returns, bit for bit, in host and in device memory and on a reused object; the result is a stationary point
// by pmc_bayes_logpost_gradient's own gradient.
// Usage: map_smoke problem.bin      exit code 0 and a final line "map_smoke OK" on success.
#include <cmath>
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
#define FAIL(msg)                                \
    do {                                         \
        std::fprintf(stderr, "%s\n", msg);       \
        return 1;                                \
    } while (0)

static pmc_csr as_csr(const t_csr* a) {
    pmc_csr c;
    c.nrows = a->nrows; c.ncols = a->ncols; c.rowptr = a->rp; c.colind = a->ci; c.vals = a->v;
    return c;
}
static bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

struct Result {
    std::vector<int32_t> status, iters, nhess, ngrad, npc;
    std::vector<double> lp0, lp, gn0, gn;
    pmc_map_result r;
    explicit Result(int nb) : status(nb), iters(nb), nhess(nb), ngrad(nb), npc(nb), lp0(nb), lp(nb), gn0(nb), gn(nb) {
        std::memset(&r, 0, sizeof(r));
        r.status = status.data(); r.newton_iterations = iters.data(); r.hessian_actions = nhess.data();
        r.gradient_evaluations = ngrad.data(); r.nonpos_curvature = npc.data();
        r.logpost0 = lp0.data(); r.logpost = lp.data(); r.grad_norm0 = gn0.data(); r.grad_norm = gn.data();
    }
    bool same(const Result& o) const {
        return status == o.status && iters == o.iters && nhess == o.nhess && ngrad == o.ngrad && npc == o.npc &&
               same_bits(lp.data(), o.lp.data(), lp.size()) && same_bits(gn.data(), o.gn.data(), gn.size()) &&
               same_bits(lp0.data(), o.lp0.data(), lp.size()) && same_bits(gn0.data(), o.gn0.data(), gn.size());
    }
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: map_smoke problem.bin\n"); return 2; }
    t_problem p = t_load(argv[1]);
    pmc_ctx* ctx = nullptr;
    CHECK(pmc_ctx_create(0, &ctx));
    pmc_solver_opts opts;
    pmc_solver_opts_default(&opts);
    opts.rel_tol = 1e-10;
    std::vector<pmc_sampler_level> sl((size_t)p.s_nlevels);
    for (int l = 0; l < p.s_nlevels; ++l) {
        std::memset(&sl[l], 0, sizeof(pmc_sampler_level));
        sl[l].n_u = p.sl[l].n_u; sl[l].n_s = p.sl[l].n_s;
        sl[l].M = as_csr(&p.sl[l].M); sl[l].B = as_csr(&p.sl[l].B); sl[l].w_diag = p.sl[l].w;
        if (p.sl[l].has_p) sl[l].P = as_csr(&p.sl[l].P);
    }
    pmc_sampler* smp = nullptr;
    CHECK(pmc_sampler_create(ctx, p.s_nlevels, p.s_nlevels, sl.data(), p.alpha, p.g, p.lognormal, &opts, &smp));
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
    const int np = p.dl[0].n_p, nb = p.nbatch, nxi = p.sl[0].n_s;
    if (np != nxi) FAIL("the sampler's field is not the solver's k");
    int32_t rp[3] = {0, 1, 3}, ci[3] = {np / 3, 2 * np / 3, 2 * np / 3 + 1};
    double gv[3] = {1.0, 0.5, 1.5};
    pmc_csr G;
    G.nrows = 2; G.ncols = np; G.rowptr = rp; G.colind = ci; G.vals = gv;
    CHECK(pmc_darcy_set_observations(dar, 0, &G));
    const double noise = 0.01;
    const size_t cnt = (size_t)nb * nxi;
    int rc = 1;
    try {
        // data: the observations of the first start's field, so that the misfit of the other starts is not zero
        std::vector<double> k((size_t)nb * np), Gall((size_t)nb * 2);
        CHECK(pmc_sampler_eval(smp, 0, 0, nb, p.xi, k.data(), nullptr, -1, 0, nullptr, PMC_MEM_HOST, nullptr));
        CHECK(pmc_darcy_compute_G(dar, 0, nb, k.data(), Gall.data(), nullptr, nullptr, PMC_MEM_HOST, nullptr));
        const std::vector<double> data{Gall[0], Gall[1]};
        pmc_map_opts mo;
        pmc_map_opts_default(&mo);
        mo.grad_rtol = 1e-3;
        // ---- the C entry, host memory
        std::vector<double> xc(p.xi, p.xi + cnt);
        Result rcapi(nb);
        CHECK(pmc_bayes_map(ctx, smp, dar, 0, 0, nb, xc.data(), PMC_MEM_HOST, data.data(), 2, noise, &mo, &rcapi.r));
        for (int b = 0; b < nb; ++b) {
            std::printf("column %d: status %d, %d outer iterations, %d Hessian actions, %d gradients, logpost %.12g -> %.12g, "
                        "|g| %.3e -> %.3e\n", b, rcapi.status[b], rcapi.iters[b], rcapi.nhess[b], rcapi.ngrad[b], rcapi.lp0[b],
                        rcapi.lp[b], rcapi.gn0[b], rcapi.gn[b]);
            if (rcapi.status[b] != PMC_MAP_CONVERGED) FAIL("pmc_bayes_map did not converge");
            if (!(rcapi.lp[b] >= rcapi.lp0[b])) FAIL("logpost decreased");
        }
        // the gradient entry at the result agrees with the stopping rule
        std::vector<double> lp((size_t)nb), g(cnt);
        CHECK(pmc_bayes_logpost_gradient(ctx, smp, dar, 0, 0, nb, xc.data(), PMC_MEM_HOST, data.data(), 2, noise, lp.data(), g.data()));
        for (int b = 0; b < nb; ++b) {
            double s = 0.0;
            for (int i = 0; i < nxi; ++i) s += g[(size_t)b * nxi + i] * g[(size_t)b * nxi + i];
            if (!(std::sqrt(s) <= 1.01 * mo.grad_rtol * rcapi.gn0[b])) FAIL("the gradient at the result misses the stopping rule");
            if (!(std::fabs(lp[b] - rcapi.lp[b]) <= 1e-9 * std::fabs(lp[b]))) FAIL("logpost at the result differs from the reported one");
        }
        // ---- the class, host memory, twice on one object (the work vectors are kept)
        PDESampler ps(ctx, smp);
        BayesianInverseProblem bip(dar, noise, data);
        for (int rep = 0; rep < 2; ++rep) {
            Vector xi(ctx, PMC_MEM_HOST);
            xi.SetSize(nxi, nb);
            std::memcpy(xi.GetData(), p.xi, sizeof(double) * cnt);
            Result rr(nb);
            bip.ComputeMAP(0, ps, xi, mo, rr.r);
            if (!same_bits(xi.GetData(), xc.data(), cnt) || !rr.same(rcapi)) FAIL("ComputeMAP differs from pmc_bayes_map (host)");
        }
        // ---- the class, device memory
        Vector xd(ctx, PMC_MEM_DEVICE);
        xd.SetSize(nxi, nb);
        CHECK(pmc_memcpy_h2d(ctx, xd.GetData(), p.xi, sizeof(double) * cnt));
        Result rd(nb);
        bip.ComputeMAP(0, ps, xd, mo, rd.r);
        std::vector<double> back(cnt);
        CHECK(pmc_memcpy_d2h(ctx, back.data(), xd.GetData(), sizeof(double) * cnt));
        if (!same_bits(back.data(), xc.data(), cnt) || !rd.same(rcapi)) FAIL("ComputeMAP differs from pmc_bayes_map (device)");
        // a refused option stays a refused argument
        mo.max_cg = 0;
        Result rbad(nb);
        if (pmc_bayes_map(ctx, smp, dar, 0, 0, nb, xc.data(), PMC_MEM_HOST, data.data(), 2, noise, &mo, &rbad.r) != PMC_ERR_INVALID)
            FAIL("max_cg = 0 was not refused");
        rc = 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
    }
    pmc_darcy_destroy(dar);
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    if (rc == 0) std::printf("map_smoke OK\n");
    return rc;
}

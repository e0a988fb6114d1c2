/* The adjoint of Eval through the C ABI from plain C (include/pmc.h only; prob_io.h reads the problem file of
 * tests/test_abi_binaries.py): the saddle-point sampler and the hybridized one built by pmc_sampler_create_hybrid_from_elements,
 * every (level, xi_level) pair, host and device buffers.  With g = log(s) on a lognormal file (s itself otherwise) and
 * w = v o s (v otherwise) the identity <g, w> = <xi, grad_xi> must hold to the tolerance of the solves.
 * Usage: sampler_adjoint_smoke problem.bin      a final line "sampler_adjoint_smoke OK" on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pmc.h"
#include "prob_io.h"

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc_ = (call);                                                                  \
        if (rc_ != PMC_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmc_last_error()); return 1; } \
    } while (0)

static pmc_csr as_csr(const t_csr* a) {
    pmc_csr c;
    c.nrows = a->nrows; c.ncols = a->ncols; c.rowptr = a->rp; c.colind = a->ci; c.vals = a->v;
    return c;
}

static int check_handle(pmc_ctx* ctx, pmc_sampler* smp, const t_problem* p, const char* name) {
    const int nb = p->nbatch;
    for (int l = 0; l < p->s_nlevels; ++l) {
        for (int xl = 0; xl <= l; ++xl) {
            const int ns = pmc_sampler_sample_size(smp, l), nxi = pmc_sampler_xi_size(smp, xl);
            double* xi = (double*)malloc(8 * (size_t)nb * nxi);
            double* s = (double*)malloc(8 * (size_t)nb * ns);
            double* v = (double*)malloc(8 * (size_t)nb * ns);
            double* g = (double*)malloc(8 * (size_t)nb * nxi);
            double* g2 = (double*)malloc(8 * (size_t)nb * nxi);
            pmc_stats* st = (pmc_stats*)calloc((size_t)nb, sizeof(pmc_stats));
            CHECK(pmc_sampler_sample(smp, xl, 3, nb, xi, PMC_MEM_HOST));
            CHECK(pmc_sampler_eval(smp, l, xl, nb, xi, s, NULL, -1, 0, NULL, PMC_MEM_HOST, NULL));
            for (size_t i = 0; i < (size_t)nb * ns; ++i) v[i] = cos(0.7 * (double)i + 0.3 * l);
            CHECK(pmc_sampler_eval_adjoint(smp, l, xl, nb, v, p->lognormal ? s : NULL, g, PMC_MEM_HOST, st));
            double worst = 0.0;
            for (int b = 0; b < nb; ++b) {
                double lhs = 0.0, rhs = 0.0, ng = 0.0, nw = 0.0;
                for (int i = 0; i < ns; ++i) {
                    const double si = s[(size_t)b * ns + i], vi = v[(size_t)b * ns + i];
                    const double gi = p->lognormal ? log(si) : si, wi = p->lognormal ? vi * si : vi;
                    lhs += gi * wi; ng += gi * gi; nw += wi * wi;
                }
                for (int i = 0; i < nxi; ++i) rhs += xi[(size_t)b * nxi + i] * g[(size_t)b * nxi + i];
                worst = fmax(worst, fabs(lhs - rhs) / sqrt(ng * nw));
                if (st[b].converged != 1) { fprintf(stderr, "%s: adjoint solve of column %d not converged\n", name, b); return 1; }
            }
            printf("%s level %d from xi on level %d: identity defect %.2e, %d iterations\n", name, l, xl, worst, st[0].iterations);
            if (!(worst < 1e-9)) { fprintf(stderr, "the adjoint identity fails\n"); return 1; }
            /* the same through device buffers: the same bits */
            void *dv = NULL, *ds = NULL, *dg = NULL;
            CHECK(pmc_malloc(ctx, 8 * (size_t)nb * ns, &dv));
            CHECK(pmc_malloc(ctx, 8 * (size_t)nb * ns, &ds));
            CHECK(pmc_malloc(ctx, 8 * (size_t)nb * nxi, &dg));
            CHECK(pmc_memcpy_h2d(ctx, dv, v, 8 * (size_t)nb * ns));
            CHECK(pmc_memcpy_h2d(ctx, ds, s, 8 * (size_t)nb * ns));
            CHECK(pmc_sampler_eval_adjoint(smp, l, xl, nb, (const double*)dv, p->lognormal ? (const double*)ds : NULL, (double*)dg,
                                           PMC_MEM_DEVICE, NULL));
            CHECK(pmc_memcpy_d2h(ctx, g2, dg, 8 * (size_t)nb * nxi));
            if (memcmp(g, g2, 8 * (size_t)nb * nxi) != 0) { fprintf(stderr, "%s: host and device paths differ\n", name); return 1; }
            CHECK(pmc_free(ctx, dv)); CHECK(pmc_free(ctx, ds)); CHECK(pmc_free(ctx, dg));
            free(xi); free(s); free(v); free(g); free(g2); free(st);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: sampler_adjoint_smoke problem.bin\n"); return 2; }
    t_problem p = t_load(argv[1]);
    pmc_ctx* ctx = NULL;
    CHECK(pmc_ctx_create(0, &ctx));
    CHECK(pmc_rng_seed(ctx, 29, 1, 0));
    pmc_solver_opts opts;
    pmc_solver_opts_default(&opts);
    opts.rel_tol = 1e-12;
    opts.abs_tol = 1e-12;
    opts.max_iter = 400;
    pmc_sampler_level* sl = (pmc_sampler_level*)calloc((size_t)p.s_nlevels, sizeof(pmc_sampler_level));
    pmc_hybrid_elements* he = (pmc_hybrid_elements*)calloc((size_t)p.s_nlevels, sizeof(pmc_hybrid_elements));
    if (p.d_nlevels < p.s_nlevels) { fprintf(stderr, "problem file: fewer Darcy than sampler levels\n"); return 1; }
    for (int l = 0; l < p.s_nlevels; ++l) {
        const t_dlevel* D = &p.dl[l];
        sl[l].n_u = p.sl[l].n_u; sl[l].n_s = p.sl[l].n_s;
        sl[l].M = as_csr(&p.sl[l].M); sl[l].B = as_csr(&p.sl[l].B); sl[l].w_diag = p.sl[l].w;
        he[l].n_u = D->n_u; he[l].n_s = D->n_p;
        he[l].M_pattern = as_csr(&D->M);
        he[l].c_ptr = D->c_ptr; he[l].c_elem = D->c_elem; he[l].c_val = D->c_val;
        he[l].B = as_csr(&D->B);
        he[l].w_diag = p.sl[l].w;
        if (p.sl[l].has_p) { sl[l].P = as_csr(&p.sl[l].P); he[l].P = as_csr(&p.sl[l].P); }
    }
    pmc_sampler *smp = NULL, *hyb = NULL;
    CHECK(pmc_sampler_create(ctx, p.s_nlevels, p.s_nlevels, sl, p.alpha, p.g, p.lognormal, &opts, &smp));
    CHECK(pmc_sampler_create_hybrid_from_elements(ctx, p.s_nlevels, he, p.alpha, p.g, p.lognormal, &opts, &hyb));
    if (check_handle(ctx, smp, &p, "saddle-point sampler") || check_handle(ctx, hyb, &p, "hybridized sampler")) return 1;
    {   /* refused, with a message: level / xi_level out of range, no realization, NULL v / grad_xi */
        const int ns = pmc_sampler_sample_size(smp, 0);
        double* v = (double*)calloc((size_t)ns, 8);
        double* g = (double*)calloc((size_t)ns, 8);
        if (pmc_sampler_eval_adjoint(smp, p.s_nlevels, 0, 1, v, NULL, g, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            pmc_sampler_eval_adjoint(smp, 0, 1, 1, v, NULL, g, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            pmc_sampler_eval_adjoint(smp, 0, 0, 0, v, NULL, g, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            pmc_sampler_eval_adjoint(smp, 0, 0, 1, NULL, NULL, g, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            pmc_sampler_eval_adjoint(smp, 0, 0, 1, v, NULL, NULL, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            (!p.lognormal && pmc_sampler_eval_adjoint(smp, 0, 0, 1, v, v, g, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID) ||
            pmc_last_error()[0] == '\0') {
            fprintf(stderr, "an invalid call was accepted\n");
            return 1;
        }
        free(v); free(g);
    }
    pmc_sampler_destroy(hyb);
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    free(sl); free(he);
    printf("sampler_adjoint_smoke OK\n");
    return 0;
}

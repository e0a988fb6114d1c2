/* Tangent and adjoint of the conditioning map through the C ABI from plain C (include/pmc.h only), on a KL sampler read from
 * a problem file of tests/test_gpu_condition_derivatives.py (kl_io.h format, nbatch 0): unit-row observations at the given
 * fine elements; per level one call of pmc_conditioner_apply_tangent and one of pmc_conditioner_apply_adjoint on NB columns,
 * <tangent(dg), u> = <dg, adjoint(u)> per column, H_l tangent(dg) = 0; then the opt-in: pmc_sampler_eval_adjoint refuses the
 * attached conditioner, accepts it after pmc_conditioner_enable_derivatives, and refuses it again after switching it off.
 * Usage: condition_derivatives_smoke problem.bin seed elem_0 y_0 [elem_1 y_1 ...]
 * Prints one line per level and a final line "condition_derivatives_smoke OK" on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kl_io.h"
#include "pmc.h"

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc_ = (call);                                                                  \
        if (rc_ != PMC_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmc_last_error()); return 1; } \
    } while (0)

#define NB 6

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 3) % 2) {
        fprintf(stderr, "usage: condition_derivatives_smoke problem.bin seed elem_0 y_0 [elem_1 y_1 ...]\n");
        return 2;
    }
    kl_file k = kl_load(argv[1]);
    const uint64_t seed = strtoull(argv[2], NULL, 10);
    const int nobs = (argc - 3) / 2;
    int32_t* rp = (int32_t*)malloc(4 * ((size_t)nobs + 1));
    int32_t* ci = (int32_t*)malloc(4 * (size_t)nobs);
    double* hv = (double*)malloc(8 * (size_t)nobs);
    double* y = (double*)malloc(8 * (size_t)nobs);
    for (int j = 0; j < nobs; ++j) {
        rp[j] = j;
        ci[j] = atoi(argv[3 + 2 * j]);
        hv[j] = 1.0;
        y[j] = atof(argv[4 + 2 * j]);
    }
    rp[nobs] = nobs;
    pmc_ctx* ctx = NULL;
    CHECK(pmc_ctx_create(0, &ctx));
    CHECK(pmc_rng_seed(ctx, seed, 1, 0));
    pmc_kl_level* lv = (pmc_kl_level*)calloc((size_t)k.nlevels, sizeof(pmc_kl_level));
    for (int l = 0; l < k.nlevels; ++l) {
        lv[l].n_s = k.lv[l].n_s;
        lv[l].w_diag = k.lv[l].w;
        if (k.lv[l].has_p) {
            lv[l].P.nrows = k.lv[l].P.nrows; lv[l].P.ncols = k.lv[l].P.ncols;
            lv[l].P.rowptr = k.lv[l].P.rp; lv[l].P.colind = k.lv[l].P.ci; lv[l].P.vals = k.lv[l].P.v;
        }
    }
    pmc_sampler* smp = NULL;
    CHECK(pmc_sampler_create_kl(ctx, k.nlevels, lv, k.nmodes, k.evals, k.evect0, k.lognormal, &smp));
    pmc_csr H0 = {nobs, k.lv[0].n_s, rp, ci, hv};
    pmc_conditioner* cond = NULL;
    CHECK(pmc_conditioner_create(smp, nobs, &H0, y, NULL, &cond));
    if (pmc_conditioner_derivatives_enabled(cond) != 0) { fprintf(stderr, "derivatives are on by default\n"); return 1; }
    const int nlevels = pmc_sampler_num_levels(smp);
    for (int l = 0; l < nlevels; ++l) {
        int n = 0;
        int64_t nnz = 0;
        CHECK(pmc_conditioner_level(cond, l, &n, &nnz, NULL, NULL, NULL, NULL, NULL));
        int32_t* lrp = (int32_t*)malloc(4 * ((size_t)nobs + 1));
        int32_t* lci = (int32_t*)malloc(4 * (size_t)nnz);
        double* lv_ = (double*)malloc(8 * (size_t)nnz);
        CHECK(pmc_conditioner_level(cond, l, NULL, NULL, NULL, NULL, lrp, lci, lv_));
        const size_t cnt = (size_t)n * NB;
        double* dg = (double*)malloc(8 * cnt);
        double* u = (double*)malloc(8 * cnt);
        double* t = (double*)malloc(8 * cnt);
        double* a = (double*)malloc(8 * cnt);
        CHECK(pmc_sampler_sample(smp, l, 0, NB, dg, PMC_MEM_HOST));      /* two sets of standard normals as test vectors */
        CHECK(pmc_sampler_sample(smp, l, NB, NB, u, PMC_MEM_HOST));
        /* refused and nothing written: a level out of range, nbatch 0, out aliasing v */
        memset(a, 0, 8 * cnt);
        if (pmc_conditioner_apply_adjoint(cond, nlevels, NB, u, NULL, a, PMC_MEM_HOST) != PMC_ERR_INVALID ||
            pmc_conditioner_apply_tangent(cond, l, 0, dg, NULL, a, PMC_MEM_HOST) != PMC_ERR_INVALID ||
            pmc_conditioner_apply_adjoint(cond, l, NB, u, NULL, u, PMC_MEM_HOST) != PMC_ERR_INVALID || pmc_last_error()[0] == '\0') {
            fprintf(stderr, "an invalid call was accepted\n");
            return 1;
        }
        for (size_t i = 0; i < cnt; ++i)
            if (a[i] != 0.0) { fprintf(stderr, "a refused call wrote its output\n"); return 1; }
        CHECK(pmc_conditioner_apply_tangent(cond, l, NB, dg, NULL, t, PMC_MEM_HOST));
        CHECK(pmc_conditioner_apply_adjoint(cond, l, NB, u, NULL, a, PMC_MEM_HOST));
        double defect = 0.0, moved = 0.0;
        for (int b = 0; b < NB; ++b) {
            double tu = 0.0, da = 0.0, ndg = 0.0, nu = 0.0;
            for (int i = 0; i < n; ++i) {
                const size_t o = (size_t)b * n + i;
                tu += t[o] * u[o];
                da += dg[o] * a[o];
                ndg += dg[o] * dg[o];
                nu += u[o] * u[o];
            }
            defect = fmax(defect, fabs(tu - da) / sqrt(ndg * nu));
            for (int j = 0; j < nobs; ++j) {
                double ht = 0.0;
                for (int p = lrp[j]; p < lrp[j + 1]; ++p) ht += lv_[p] * t[(size_t)b * n + lci[p]];
                moved = fmax(moved, fabs(ht));
            }
        }
        printf("level %d: n %d transposition defect %.3e max |H tangent| %.3e\n", l, n, defect, moved);
        /* both bounds: rounding of sums of n products, n <= 1e6 here, with two decades of margin */
        if (!(defect <= 1e-9) || !(moved <= 1e-9)) { fprintf(stderr, "the pair is not a transposed pair\n"); return 1; }
        /* the opt-in of the sampler entry */
        double* gx = (double*)malloc(8 * (size_t)pmc_sampler_xi_size(smp, l) * NB);
        CHECK(pmc_sampler_set_conditioner(smp, cond));
        if (pmc_sampler_eval_adjoint(smp, l, l, NB, u, NULL, gx, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID ||
            strstr(pmc_last_error(), "conditioner") == NULL) {
            fprintf(stderr, "EvalAdjoint accepted a conditioner without the opt-in\n");
            return 1;
        }
        CHECK(pmc_conditioner_enable_derivatives(cond, 1));
        if (pmc_conditioner_derivatives_enabled(cond) != 1) return 1;
        CHECK(pmc_sampler_eval_adjoint(smp, l, l, NB, u, NULL, gx, PMC_MEM_HOST, NULL));
        CHECK(pmc_conditioner_enable_derivatives(cond, 0));
        if (pmc_sampler_eval_adjoint(smp, l, l, NB, u, NULL, gx, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID) {
            fprintf(stderr, "EvalAdjoint accepted a conditioner after the opt-in was withdrawn\n");
            return 1;
        }
        CHECK(pmc_sampler_set_conditioner(smp, NULL));
        free(lrp); free(lci); free(lv_); free(dg); free(u); free(t); free(a); free(gx);
    }
    pmc_conditioner_destroy(cond);
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    free(rp); free(ci); free(hv); free(y); free(lv);
    printf("condition_derivatives_smoke OK\n");
    return 0;
}

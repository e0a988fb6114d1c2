/* Conditioning on observed field values through the C ABI from plain C (include/pmc.h only), on a KL sampler read from a
 * problem file of tests/test_gpu_condition.py (kl_io.h format, nbatch 0): unit-row observations at the given fine elements,
 * setup on every level, then Sample + conditioned Eval of 6 realizations per level through the Eval hook; the observed
 * combinations H_l log(s) (the handle is lognormal or not as the file says) must reproduce y.
 * Usage: condition_smoke problem.bin seed elem_0 y_0 [elem_1 y_1 ...]
 * Prints one line per level and a final line "condition_smoke OK" on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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
        fprintf(stderr, "usage: condition_smoke problem.bin seed elem_0 y_0 [elem_1 y_1 ...]\n");
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
    /* refused: no observation, a wrong column count */
    pmc_csr Hbad = H0;
    Hbad.ncols += 1;
    if (pmc_conditioner_create(smp, 0, &H0, y, NULL, &cond) != PMC_ERR_INVALID ||
        pmc_conditioner_create(smp, nobs, &Hbad, y, NULL, &cond) != PMC_ERR_INVALID || pmc_last_error()[0] == '\0') {
        fprintf(stderr, "an invalid call was accepted\n");
        return 1;
    }
    CHECK(pmc_conditioner_create(smp, nobs, &H0, y, NULL, &cond));
    if (pmc_conditioner_num_obs(cond) != nobs) return 1;
    CHECK(pmc_sampler_set_conditioner(smp, cond));
    const int nlevels = pmc_sampler_num_levels(smp);
    for (int l = 0; l < nlevels; ++l) {
        int n = 0;
        int64_t nnz = 0;
        CHECK(pmc_conditioner_level(cond, l, &n, &nnz, NULL, NULL, NULL, NULL, NULL));
        if (n != pmc_sampler_sample_size(smp, l)) return 1;
        int32_t* lrp = (int32_t*)malloc(4 * ((size_t)nobs + 1));
        int32_t* lci = (int32_t*)malloc(4 * (size_t)nnz);
        double* lv_ = (double*)malloc(8 * (size_t)nnz);
        CHECK(pmc_conditioner_level(cond, l, NULL, NULL, NULL, NULL, lrp, lci, lv_));
        double* xi = (double*)malloc(8 * (size_t)n * NB);
        double* s = (double*)malloc(8 * (size_t)n * NB);
        CHECK(pmc_sampler_sample(smp, l, 0, NB, xi, PMC_MEM_HOST));
        CHECK(pmc_sampler_eval(smp, l, l, NB, xi, s, NULL, -1, 0, NULL, PMC_MEM_HOST, NULL));
        double worst = 0.0;
        for (int b = 0; b < NB; ++b)
            for (int j = 0; j < nobs; ++j) {
                double hg = 0.0;
                for (int p = lrp[j]; p < lrp[j + 1]; ++p) {
                    const double v = s[(size_t)b * n + lci[p]];
                    hg += lv_[p] * (k.lognormal ? log(v) : v);
                }
                worst = fmax(worst, fabs(hg - y[j]));
            }
        printf("level %d: n %d nnz(H) %lld max |H g_c - y| %.3e\n", l, n, (long long)nnz, worst);
        if (!(worst <= 1e-9)) { fprintf(stderr, "the conditioned fields miss the data\n"); return 1; }
        free(lrp); free(lci); free(lv_); free(xi); free(s);
    }
    CHECK(pmc_sampler_set_conditioner(smp, NULL));
    pmc_conditioner_destroy(cond);
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    free(rp); free(ci); free(hv); free(y); free(lv);
    printf("condition_smoke OK\n");
    return 0;
}

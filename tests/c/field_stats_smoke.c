/* PDESamplerTest's result table (examples/PDESamplerTest.cpp:186-274) through the C ABI from plain C (include/pmc.h only),
 * on a KL sampler read from a problem file of tests/test_gpu_field_stats.py (kl_io.h format, nbatch 0): chi restricted level
 * by level with P^T, then per level Sample + Eval + statistics on the device (pmc_field_stats_run) and the errors of the
 * expectation and the second moment against the exact moments.
 * Usage: field_stats_smoke problem.bin seed chi_index nsamples exact_expectation exact_variance
 * Prints one table line per level and a final line "field_stats_smoke OK" on success. */
#include <stdio.h>
#include <stdlib.h>

#include "kl_io.h"
#include "pmc.h"

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc_ = (call);                                                                  \
        if (rc_ != PMC_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmc_last_error()); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: field_stats_smoke problem.bin seed chi_index nsamples exact_expectation exact_variance\n");
        return 2;
    }
    kl_file k = kl_load(argv[1]);
    const uint64_t seed = strtoull(argv[2], NULL, 10);
    const int chi_index = atoi(argv[3]);
    const int64_t nsamples = strtoll(argv[4], NULL, 10);
    const double exact_e = atof(argv[5]), exact_v = atof(argv[6]);
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
    const int nlevels = pmc_sampler_num_levels(smp);
    /* chi[0] = indicator of chi_index; chi[l + 1] = P_l^T chi[l] (PDESamplerTest.cpp:186-192) */
    double** chi = (double**)calloc((size_t)k.nlevels, sizeof(double*));
    chi[0] = (double*)calloc((size_t)k.lv[0].n_s, sizeof(double));
    if (chi_index < 0 || chi_index >= k.lv[0].n_s) { fprintf(stderr, "chi_index out of range\n"); return 2; }
    chi[0][chi_index] = 1.0;
    for (int l = 0; l + 1 < k.nlevels; ++l) {
        chi[l + 1] = (double*)calloc((size_t)k.lv[l + 1].n_s, sizeof(double));
        const kl_csr* P = &k.lv[l].P;
        for (int r = 0; r < P->nrows; ++r)
            for (int p = P->rp[r]; p < P->rp[r + 1]; ++p) chi[l + 1][P->ci[p]] += P->v[p] * chi[l][r];
    }
    for (int l = 0; l < nlevels; ++l) {
        const int n = pmc_sampler_sample_size(smp, l);
        pmc_field_stats* fs = NULL;
        CHECK(pmc_field_stats_create(smp, l, chi[l], PMC_MEM_HOST, &fs));
        CHECK(pmc_field_stats_run(fs, 0, nsamples));
        double* e = (double*)malloc(8 * (size_t)n);
        double* m2 = (double*)malloc(8 * (size_t)n);
        double* cc = (double*)malloc(8 * (size_t)n);
        int64_t N = 0;
        CHECK(pmc_field_stats_read(fs, e, m2, cc, &N, PMC_MEM_HOST));
        double exp_err = 0.0, var_err = 0.0, max_err = 0.0;
        CHECK(pmc_sampler_l2_error(smp, l, 1, e, exact_e, &exp_err, PMC_MEM_HOST));
        CHECK(pmc_sampler_l2_error(smp, l, 1, m2, exact_v, &var_err, PMC_MEM_HOST));
        CHECK(pmc_sampler_max_error(smp, l, 1, e, exact_e, &max_err, PMC_MEM_HOST));
        int ichi = 0;
        for (int i = 1; i < n; ++i)
            if (chi[l][i] > chi[l][ichi]) ichi = i;
        printf("level %d: N %lld exp_l2 %.17g var_l2 %.17g exp_max %.17g chi_cov %.17g\n", l, (long long)N, exp_err, var_err,
               max_err, cc[ichi]);
        if (N != nsamples) return 1;
        /* refused: nbatch < 1, nsamples < 1 */
        if (pmc_sampler_l2_error(smp, l, 0, e, exact_e, &exp_err, PMC_MEM_HOST) != PMC_ERR_INVALID ||
            pmc_field_stats_run(fs, 0, 0) != PMC_ERR_INVALID) {
            fprintf(stderr, "an invalid call was accepted\n");
            return 1;
        }
        pmc_field_stats_destroy(fs);
        free(e);
        free(m2);
        free(cc);
    }
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    printf("field_stats_smoke OK\n");
    return 0;
}

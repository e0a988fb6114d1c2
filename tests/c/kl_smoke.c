/* KL sampler through the C ABI from plain C (include/pmc.h only): create from the eigenpairs of a problem file written by
 * tests/test_gpu_kl.py, check the sizes and the refused entry points, Sample, and Eval on every level against the expected
 * fields.  Usage: kl_smoke problem.bin      exit code 0 and a final line "kl_smoke OK" on success. */
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

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kl_smoke problem.bin\n"); return 2; }
    kl_file k = kl_load(argv[1]);
    pmc_ctx* ctx = NULL;
    CHECK(pmc_ctx_create(0, &ctx));
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
    if (pmc_sampler_is_kl(smp) != 1 || pmc_sampler_is_hybrid(smp) != 0) { fprintf(stderr, "handle kind\n"); return 1; }
    if (pmc_sampler_num_levels(smp) != k.nlevels) { fprintf(stderr, "level count\n"); return 1; }
    if (pmc_sampler_mult(smp, 0, 1, k.xi, k.xi, 0, PMC_MEM_HOST, NULL) != PMC_ERR_INVALID) {
        fprintf(stderr, "pmc_sampler_mult accepted a KL handle\n");
        return 1;
    }
    const int n0 = k.lv[0].n_s;
    double* xi = (double*)malloc(8 * (size_t)k.nbatch * n0);
    CHECK(pmc_sampler_sample(smp, 0, 0, k.nbatch, xi, PMC_MEM_HOST));
    for (int l = 0; l < k.nlevels; ++l) {
        const int ns = k.lv[l].n_s;
        if (pmc_sampler_xi_size(smp, l) != ns || pmc_sampler_sample_size(smp, l) != ns || pmc_sampler_nnz(smp, l) != 0) {
            fprintf(stderr, "sizes on level %d\n", l);
            return 1;
        }
        double* s = (double*)malloc(8 * (size_t)k.nbatch * ns);
        pmc_stats* st = (pmc_stats*)calloc((size_t)k.nbatch, sizeof(pmc_stats));
        CHECK(pmc_sampler_eval(smp, l, 0, k.nbatch, k.xi, s, NULL, -1, 0, NULL, PMC_MEM_HOST, st));
        double err = 0.0, ref = 0.0;
        for (size_t i = 0; i < (size_t)k.nbatch * ns; ++i) {
            err = fmax(err, fabs(s[i] - k.s_expect[l][i]));
            ref = fmax(ref, fabs(k.s_expect[l][i]));
        }
        printf("level %d: n_s %d, max |s - s_expect| / max |s_expect| = %.3e, iterations %d, converged %d\n", l, ns,
               err / ref, st[0].iterations, st[0].converged);
        if (!(err <= 1e-12 * ref) || st[0].iterations != 0 || st[0].converged != 1) return 1;
        free(s);
        free(st);
    }
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    printf("kl_smoke OK\n");
    return 0;
}

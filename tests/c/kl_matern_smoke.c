/* The device Matern eigensolver through the C ABI from plain C (include/pmc.h only): the top 8 eigenpairs of the covariance
 * on an 8 x 8 x 8 grid of cells on [0,2]^3, checked by the block product (K y = lambda y with y = W^1/2 v), by V^T W V = I,
 * and fed to pmc_sampler_create_kl.  Exit code 0 and a final line "kl_matern_smoke OK" on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "pmc.h"

#define CHECK(call)                                                                        \
    do {                                                                                   \
        int rc_ = (call);                                                                  \
        if (rc_ != PMC_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmc_last_error()); return 1; } \
    } while (0)

enum { NX = 8, N = NX * NX * NX, M = 8 };

int main(void) {
    const double h = 2.0 / NX, corlen = 0.3;
    double* x = (double*)malloc(sizeof(double) * 3 * N);
    double* w = (double*)malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) {
        x[3 * i] = (i % NX + 0.5) * h;
        x[3 * i + 1] = (i / NX % NX + 0.5) * h;
        x[3 * i + 2] = (i / (NX * NX) + 0.5) * h;
        w[i] = h * h * h * (1.0 + 0.5 * (i % 3));   /* not uniform: the W^1/2 scalings matter */
    }
    pmc_ctx* ctx = NULL;
    CHECK(pmc_ctx_create(0, &ctx));
    pmc_kl_eigs_opts o;
    pmc_kl_eigs_opts_default(&o);
    o.tol = 1e-10;
    o.seed = 5;
    pmc_kl_eigs_info info;
    double evals[M];
    double* V = (double*)malloc(sizeof(double) * N * M);
    if (pmc_kl_matern_eigs(ctx, 2, N, x, w, corlen, M, &o, evals, V, &info) != PMC_ERR_INVALID) {
        fprintf(stderr, "dim = 2 was accepted\n");
        return 1;
    }
    printf("dim = 2 refused: %s\n", pmc_last_error());
    CHECK(pmc_kl_matern_eigs(ctx, 3, N, x, w, corlen, M, &o, evals, V, &info));
    printf("iterations %d, block products %d, converged %d, residual %.2e, gap_rel %.3e, %.3f s\n", info.iterations,
           info.block_products, info.converged, info.max_residual_rel, info.gap_rel, info.seconds);
    if (info.converged != 1 || !(info.max_residual_rel <= o.tol)) return 1;
    double* Y = (double*)malloc(sizeof(double) * N * M);
    double* KY = (double*)malloc(sizeof(double) * N * M);
    for (int k = 0; k < M; ++k)
        for (int i = 0; i < N; ++i) Y[k * N + i] = sqrt(w[i]) * V[k * N + i];
    CHECK(pmc_kl_matern_apply(ctx, 3, N, x, w, corlen, M, Y, KY));
    for (int k = 0; k < M; ++k) {
        double r2 = 0.0;
        for (int i = 0; i < N; ++i) r2 += pow(KY[k * N + i] - evals[k] * Y[k * N + i], 2);
        if (k > 0 && evals[k] < evals[k - 1]) { fprintf(stderr, "eigenvalues do not ascend\n"); return 1; }
        if (!(sqrt(r2) <= 10.0 * o.tol * evals[M - 1])) { fprintf(stderr, "residual of mode %d: %.3e\n", k, sqrt(r2)); return 1; }
        for (int l = 0; l <= k; ++l) {
            double d = 0.0;
            for (int i = 0; i < N; ++i) d += Y[k * N + i] * Y[l * N + i];
            if (!(fabs(d - (k == l ? 1.0 : 0.0)) <= 1e-10)) { fprintf(stderr, "V^T W V (%d, %d) = %.3e\n", k, l, d); return 1; }
        }
    }
    /* the pairs as pmc_sampler_create_kl takes them: xi = e_k returns sqrt(lambda_k) v_k */
    pmc_kl_level lv = {0};
    lv.n_s = N;
    lv.w_diag = w;
    pmc_sampler* smp = NULL;
    CHECK(pmc_sampler_create_kl(ctx, 1, &lv, M, evals, V, 0, &smp));
    double* xi = (double*)calloc(N, sizeof(double));
    double* s = (double*)malloc(sizeof(double) * N);
    xi[M - 1] = 1.0;
    CHECK(pmc_sampler_eval(smp, 0, 0, 1, xi, s, NULL, -1, 0, NULL, PMC_MEM_HOST, NULL));
    double err = 0.0, big = 0.0;
    for (int i = 0; i < N; ++i) {
        const double ref = sqrt(evals[M - 1]) * V[(M - 1) * N + i];
        err = fmax(err, fabs(s[i] - ref));
        big = fmax(big, fabs(ref));
    }
    printf("sampler field of the largest mode: max |s - sqrt(lambda) v| / max |sqrt(lambda) v| = %.3e\n", err / big);
    if (!(err <= 1e-12 * big)) return 1;
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    printf("kl_matern_smoke OK\n");
    return 0;
}

/* Posterior field estimates from plain C: include/pmc.h + include/pmc_host.h only.  Builds the sampler and the Darcy solver
 * of a problem file (tests/c/prob_io.h layout, as tests/test_abi_binaries.py writes it), observes the P0-mass-weighted
 * mean pressure of every level, runs a 2-level device ratio manager with field statistics on, and prints the maps'
 * checksums (serial sums in element order) and the per-level norms with 17 significant digits.
 * Usage: posterior_fields_smoke problem.bin seed n0 n1 batch splitting g_obs noise
 * final line "posterior_fields_smoke OK" on success. */
#include <stdio.h>
#include <stdlib.h>

#include "pmc.h"
#include "pmc_host.h"
#include "prob_io.h"

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        int rc_ = (call);                                                                                    \
        if (rc_ != PMC_OK) { fprintf(stderr, "%s -> %d: %s / %s\n", #call, rc_, pmc_last_error(), pmc_host_last_error()); return 1; } \
    } while (0)

static pmc_csr as_csr(const t_csr* a) {
    pmc_csr c;
    c.nrows = a->nrows; c.ncols = a->ncols; c.rowptr = a->rp; c.colind = a->ci; c.vals = a->v;
    return c;
}

int main(int argc, char** argv) {
    if (argc < 9) {
        fprintf(stderr, "usage: posterior_fields_smoke problem.bin seed n0 n1 batch splitting g_obs noise\n");
        return 2;
    }
    t_problem p = t_load(argv[1]);
    const uint64_t seed = strtoull(argv[2], NULL, 10);
    const int32_t ns[2] = {atoi(argv[3]), atoi(argv[4])};
    const int splitting = atoi(argv[6]);
    const double g_obs = strtod(argv[7], NULL), noise = strtod(argv[8], NULL);
    if (p.s_nlevels < 2 || p.d_nlevels < 2) { fprintf(stderr, "two levels expected\n"); return 2; }
    pmc_ctx* ctx = NULL;
    CHECK(pmc_ctx_create(0, &ctx));
    CHECK(pmc_rng_seed(ctx, seed, 1, 0));
    pmc_solver_opts opts;
    pmc_solver_opts_default(&opts);
    opts.rel_tol = 1e-12;
    opts.abs_tol = 1e-30;
    opts.max_iter = 400;
    pmc_sampler_level* sl = (pmc_sampler_level*)calloc((size_t)p.s_nlevels, sizeof(pmc_sampler_level));
    for (int l = 0; l < p.s_nlevels; ++l) {
        sl[l].n_u = p.sl[l].n_u; sl[l].n_s = p.sl[l].n_s;
        sl[l].M = as_csr(&p.sl[l].M); sl[l].B = as_csr(&p.sl[l].B); sl[l].w_diag = p.sl[l].w;
        if (p.sl[l].has_p) sl[l].P = as_csr(&p.sl[l].P);
    }
    pmc_sampler* smp = NULL;
    CHECK(pmc_sampler_create(ctx, p.s_nlevels, p.s_nlevels, sl, p.alpha, p.g, p.lognormal, &opts, &smp));
    pmc_darcy_level* dl = (pmc_darcy_level*)calloc((size_t)p.d_nlevels, sizeof(pmc_darcy_level));
    for (int l = 0; l < p.d_nlevels; ++l) {
        const t_dlevel* L = &p.dl[l];
        dl[l].n_u = L->n_u; dl[l].n_p = L->n_p;
        dl[l].M_pattern = as_csr(&L->M);
        dl[l].c_ptr = L->c_ptr; dl[l].c_elem = L->c_elem; dl[l].c_val = L->c_val;
        dl[l].B = as_csr(&L->B);
        dl[l].rhs = L->rhs; dl[l].ess_mask = L->ess; dl[l].ess_data = L->ess_data; dl[l].obs = L->obs;
        if (L->has_p) dl[l].P = as_csr(&L->P);
    }
    pmc_darcy* dar = NULL;
    CHECK(pmc_darcy_create(ctx, p.d_nlevels, p.d_nlevels, dl, p.k_divides, &opts, &dar));
    /* one observation per level: the P0-mass-weighted mean pressure, g = diag(W) of the level (the same P0 space) */
    for (int l = 0; l < 2; ++l) {
        const int n = pmc_darcy_num_pressure_dofs(dar, l);
        int32_t* rp = (int32_t*)malloc(sizeof(int32_t) * 2);
        int32_t* ci = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
        rp[0] = 0; rp[1] = n;
        for (int i = 0; i < n; ++i) ci[i] = i;
        pmc_csr g;
        g.nrows = 1; g.ncols = n; g.rowptr = rp; g.colind = ci; g.vals = p.sl[l].w;
        CHECK(pmc_darcy_set_observations(dar, l, &g));
        free(rp);
        free(ci);
    }

    pmc_mlmc_params prm;
    pmc_mlmc_params_default(&prm);
    prm.wall_time = 0;
    prm.batch = atoi(argv[5]);
    pmc_ratio* m = NULL;
    CHECK(pmc_ratio_create(ctx, smp, dar, 2, &g_obs, 1, noise, &prm, &m));
    CHECK(pmc_ratio_set_splitting(m, splitting));
    const int n0 = pmc_darcy_num_pressure_dofs(dar, 0);
    CHECK(pmc_ratio_enable_field_stats(m, p.sl[0].w, PMC_MEM_HOST));
    CHECK(pmc_ratio_init_run(m, ns));
    double* maps = (double*)malloc(sizeof(double) * 3 * (size_t)n0);
    double l2[2], iv[2];
    CHECK(pmc_ratio_field_stats(m, maps, maps + n0, maps + 2 * (size_t)n0, l2, iv, PMC_MEM_HOST));
    const char* names[3] = {"mean", "second_moment", "estimator_variance"};
    for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (int i = 0; i < n0; ++i) s += maps[(size_t)k * n0 + i];
        printf("%s %.17g\n", names[k], s);
    }
    for (int l = 0; l < 2; ++l) printf("level %d %.17g %.17g\n", l, l2[l], iv[l]);
    pmc_ratio_destroy(m);
    pmc_darcy_destroy(dar);
    pmc_sampler_destroy(smp);
    pmc_ctx_destroy(ctx);
    free(maps);
    free(sl);
    free(dl);
    printf("posterior_fields_smoke OK\n");
    return 0;
}

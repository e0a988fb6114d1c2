/* Reader of the KL sampler problem files tests/test_gpu_kl.py writes for kl_smoke.c / kl_adapter_smoke.cpp (test
 * infrastructure).  Layout, little-endian: int32 magic 0x4b4c3031, nlevels, nmodes, lognormal, nbatch; per level int32 n_s,
 * double w[n_s], int32 has_P and, if set, int32 nrows, ncols, nnz, rowptr[nrows+1], colind[nnz], double vals[nnz]; then
 * double evals[nmodes], evect0[n_s(0) * nmodes] (column-major), xi[nbatch * n_s(0)], and per level the expected fields
 * s[nbatch * n_s] of Eval(level, xi drawn on level 0). */
#ifndef KL_IO_H_
#define KL_IO_H_
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct kl_csr { int32_t nrows, ncols, nnz; int32_t *rp, *ci; double* v; } kl_csr;
typedef struct kl_lvl { int32_t n_s, has_p; double* w; kl_csr P; } kl_lvl;
typedef struct kl_file {
    int32_t nlevels, nmodes, lognormal, nbatch;
    kl_lvl* lv;
    double *evals, *evect0, *xi;
    double** s_expect;
} kl_file;

static void* kl_read(FILE* f, size_t size, size_t n) {
    void* p = malloc(size * (n ? n : 1));
    if (!p || fread(p, size, n, f) != n) { fprintf(stderr, "kl_io: short read\n"); exit(2); }
    return p;
}
static int32_t kl_i32(FILE* f) {
    int32_t v;
    if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "kl_io: short read\n"); exit(2); }
    return v;
}
static kl_file kl_load(const char* path) {
    kl_file k;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "kl_io: cannot open %s\n", path); exit(2); }
    if (kl_i32(f) != 0x4b4c3031) { fprintf(stderr, "kl_io: bad magic\n"); exit(2); }
    k.nlevels = kl_i32(f); k.nmodes = kl_i32(f); k.lognormal = kl_i32(f); k.nbatch = kl_i32(f);
    k.lv = (kl_lvl*)calloc((size_t)k.nlevels, sizeof(kl_lvl));
    for (int l = 0; l < k.nlevels; ++l) {
        kl_lvl* L = &k.lv[l];
        L->n_s = kl_i32(f);
        L->w = (double*)kl_read(f, 8, (size_t)L->n_s);
        L->has_p = kl_i32(f);
        if (L->has_p) {
            L->P.nrows = kl_i32(f); L->P.ncols = kl_i32(f); L->P.nnz = kl_i32(f);
            L->P.rp = (int32_t*)kl_read(f, 4, (size_t)L->P.nrows + 1);
            L->P.ci = (int32_t*)kl_read(f, 4, (size_t)L->P.nnz);
            L->P.v = (double*)kl_read(f, 8, (size_t)L->P.nnz);
        }
    }
    k.evals = (double*)kl_read(f, 8, (size_t)k.nmodes);
    k.evect0 = (double*)kl_read(f, 8, (size_t)k.lv[0].n_s * k.nmodes);
    k.xi = (double*)kl_read(f, 8, (size_t)k.nbatch * k.lv[0].n_s);
    k.s_expect = (double**)calloc((size_t)k.nlevels, sizeof(double*));
    for (int l = 0; l < k.nlevels; ++l) k.s_expect[l] = (double*)kl_read(f, 8, (size_t)k.nbatch * k.lv[l].n_s);
    fclose(f);
    return k;
}
#endif

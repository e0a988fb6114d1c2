// Random fields and layout changes: Philox4x32-10 + AS241 normal deviates (K1), the sample-major <-> interleaved layout
// changes fused with the sampler's pointwise maps (K2, K9, K10), the broadcast of a shared vector into a batch.
#include "klaunch.hpp"

namespace pmc {

// ------------------------------------------------------------------------------------------
// Philox4x32-10 + AS241 inverse normal CDF (bit-level twin: oracle/rng_oracle.py)
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
}

__device__ __forceinline__ double u01_open(uint32_t hi, uint32_t lo) {
    // 52 bits: (m + 1/2) / 2^52 is exact, strictly inside (0,1)
    const uint64_t m = ((uint64_t)(hi >> 6) << 26) + (uint64_t)(lo >> 6);
    return ((double)m + 0.5) * (1.0 / 4503599627370496.0);
}

#pragma clang fp contract(off)
__device__ double inv_normal_cdf(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
                                 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                               1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
                                 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                               5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r +
                                 2.41780725177450611770e-1) * r + 1.27045825245236838258e0) * r +
                               3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
                             4.63033784615654529590e0) * r + 1.42343711074968357734e0);
        const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r +
                                 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                               6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
                             2.05319162663775882187e0) * r + 1.0);
        val = num / den;
    } else {
        r -= 5.0;
        const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
                                 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                               2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
                             5.46378491116411436990e0) * r + 6.65790464350110377720e0);
        const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r +
                                 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                               1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                             5.99832206555887937690e-1) * r + 1.0);
        val = num / den;
    }
    return q < 0.0 ? -val : val;
}
#pragma clang fp contract(fast)

// out[b*n + i], sample-major.  One thread per (pair of elements, realization).
// Realization b of the launch is the generator's realization first_id + b * id_stride (id_stride = nparts of a split
// generator: part p owns the ids p, p + nparts, ...).
__global__ __launch_bounds__(kBlock) void normal_fill_kernel(int n, int nbatch, uint64_t seed, uint64_t first_id,
                                                             uint64_t id_stride, uint32_t stream, double mean, double sigma,
                                                             double* __restrict__ out) {
    const int npair = (n + 1) >> 1;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= npair || b >= nbatch) return;
    const uint64_t sid = first_id + (uint64_t)b * id_stride;
    uint32_t c[4] = {(uint32_t)j, (uint32_t)sid, (uint32_t)(sid >> 32), stream};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    double* o = out + (size_t)b * n + 2 * (size_t)j;
    o[0] = mean + sigma * inv_normal_cdf(u01_open(c[0], c[1]));
    if (2 * j + 1 < n) o[1] = mean + sigma * inv_normal_cdf(u01_open(c[2], c[3]));
}

// ------------------------------------------------------------------------------------------
// layout changes fused with the sampler's pointwise maps
// out[i*NB + k] = scale * in[k*n + i] * (w ? w[i] : 1)        (K2: rhs_s = -g W^{1/2} xi)
// src (optional): row i of the result takes row src[i] of the input (a renumbering of the rows)
template <int NB>
__global__ __launch_bounds__(kBlock) void interleave_kernel(int n, const double* __restrict__ in,
                                                            const double* __restrict__ w, double scale,
                                                            double* __restrict__ out, int ld, const int* __restrict__ src) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    const double f = w ? scale * w[i] : scale;
    const int is = src ? src[i] : i;
    double v[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = f * in[(size_t)(c0 + k) * n + is];
    store_row<NB>(out + (size_t)i * LD + c0, v);
}

// out[i*NB + k] = scale * v[k*n + i] * (s ? s[k*n + i] : 1) * (rowscale ? rowscale[i] : 1): the seed of Eval's adjoint
// (Sampler::eval_adjoint_chunk), dJ/ds_out through the exp() of a lognormal handle, sample-major in and interleaved out
template <int NB>
__global__ __launch_bounds__(kBlock) void seed_interleave_kernel(int n, const double* __restrict__ v,
                                                                 const double* __restrict__ s,
                                                                 const double* __restrict__ rowscale, double scale,
                                                                 double* __restrict__ out, int ld) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    const double f = rowscale ? scale * rowscale[i] : scale;
    double t[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const size_t o = (size_t)(c0 + k) * n + i;
        t[k] = f * (s ? v[o] * s[o] : v[o]);
    }
    store_row<NB>(out + (size_t)i * LD + c0, t);
}

// out[k*m + i] = post( rowscale[i] * in[idx ? idx[i] : i][k] ),  post = exp if do_exp   (K9, K10)
template <int NB>
__global__ __launch_bounds__(kBlock) void deinterleave_kernel(int m, const double* __restrict__ in,
                                                              const int* __restrict__ idx,
                                                              const double* __restrict__ rowscale, int do_exp,
                                                              double* __restrict__ out, int ld) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    const int src = idx ? idx[i] : i;
    double v[NB];
    load_row<NB>(in + (size_t)src * LD + c0, v);
    const double f = rowscale ? rowscale[i] : 1.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        double t = f * v[k];
        if (do_exp) t = exp(t);
        out[(size_t)(c0 + k) * m + i] = t;
    }
}

// out[i*NB+k] = a[i] (broadcast a shared vector into an interleaved batch)
template <int NB>
__global__ __launch_bounds__(kBlock) void broadcast_kernel(int n, const double* __restrict__ a, double* __restrict__ out,
                                                           int ld) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double v[NB];
    const double t = a[i];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = t;
    store_row<NB>(out + (size_t)i * row_ld<NB>(ld) + col0<NB>(), v);
}

// ==========================================================================================
// launchers
namespace k {

void normal_fill(hipStream_t st, int n, int nbatch, uint64_t seed, uint64_t first_id, uint32_t stream, double mean,
                 double sigma, double* out, uint64_t id_stride) {
    if (n == 0 || nbatch == 0) return;
    const int npair = (n + 1) / 2;
    dim3 g((unsigned)((npair + kBlock - 1) / kBlock), (unsigned)nbatch);
    normal_fill_kernel<<<g, kBlock, 0, st>>>(n, nbatch, seed, first_id, id_stride, stream, mean, sigma, out);
    check_launch();
}

void interleave(hipStream_t st, int nb, int n, const double* in, const double* w, double scale, double* out, const int* src) {
    PMC_DISPATCH_NB(nb, { interleave_kernel<NB><<<groups(grid_rows(n), nb), kBlock, 0, st>>>(n, in, w, scale, out, nb, src); });
    check_launch();
}

void seed_interleave(hipStream_t st, int nb, int n, const double* v, const double* s, const double* rowscale, double scale,
                     double* out) {
    if (n == 0) return;
    PMC_DISPATCH_NB(nb, { seed_interleave_kernel<NB><<<groups(grid_rows(n), nb), kBlock, 0, st>>>(n, v, s, rowscale, scale, out, nb); });
    check_launch();
}

void deinterleave(hipStream_t st, int nb, int m, const double* in, const int* idx, const double* rowscale, bool do_exp,
                  double* out) {
    if (m == 0) return;
    PMC_DISPATCH_NB(nb, { deinterleave_kernel<NB><<<groups(grid_rows(m), nb), kBlock, 0, st>>>(m, in, idx, rowscale, do_exp ? 1 : 0, out, nb); });
    check_launch();
}

void broadcast(hipStream_t st, int nb, int n, const double* a, double* out) {
    PMC_DISPATCH_NB(nb, { broadcast_kernel<NB><<<groups(grid_rows(n), nb), kBlock, 0, st>>>(n, a, out, nb); });
    check_launch();
}

}  // namespace k
}  // namespace pmc

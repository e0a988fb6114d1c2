// Small levels in one workgroup's LDS: the V-cycle tail, the persistent per-realization MINRES solver of small sampler
// levels, the dense exact solve of narrow launches, and the transposition of per-realization values the tail reads.
#include "klaunch.hpp"

#include <atomic>

namespace pmc {

// ------------------------------------------------------------------------------------------
// V-cycle tail in LDS.  Small levels are launch-latency bound as separate kernels (a few us each, ~20
// launches per V-cycle); here one workgroup per realization sweeps all of them with __syncthreads()
// between phases.  Vectors live in LDS ([r | x | d] per level), matrices are read from global memory (L2).
static constexpr int kTailThreads = 1024;
// The tail's device functions are inlined into their two kernels: as real calls they cost ~50 callee-saved registers spilled
// at every entry and a register allocation split at the call boundary (Darcy iteration on a 16^3 level 168 -> 147 us,
// config 3 +5 %).
#define PMC_TAIL_INLINE __device__ __forceinline__
static constexpr size_t kTailLdsBytes = 160 * 1024 - 1024;   // dynamic LDS budget (static reduction scratch on top)

#ifndef PMC_TAIL_WIDE
#define PMC_TAIL_WIDE 0
#endif
__device__ __forceinline__ double tail_row_dot(const int* __restrict__ off, const int* __restrict__ cols,
                                               const double* __restrict__ vals, int vstride, size_t vk, int row,
                                               const double* xl) {
    const int slice = row >> 6, lane = row & 63;
    const int o = off[slice];
    const int width = (off[slice + 1] - o) >> 6;
    double acc = 0.0;
    int slot = o + lane;
#if PMC_TAIL_WIDE
    // wide slices (aggregation hierarchies of the hybridized sampler: 17-27 entries per row): 16 pairs per trip - a sweep over
    // such a level is a chain of trips to L2 (one workgroup per realization, ~1 us each), and the chain is what a pass
    // costs (LAB_NOTES 10.4).  Same summation order as the 8-wide loop: bit-identical.
    if (width > 12) {
        for (int j0 = 0; j0 < width; j0 += 16, slot += 16 * kWave) {
            int c[16];
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const bool ok = j0 + u < width;
                const int at = ok ? slot + u * kWave : slot;
                c[u] = cols[at];
                v[u] = ok ? vals[(size_t)at * vstride + vk] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 16; ++u) acc = fma(v[u], xl[c[u]], acc);
        }
        return acc;
    }
#endif
    // 8 (index, value) pairs are requested together, then the 8 LDS gathers: two memory latencies per 8 entries
    // instead of one dependent chain per entry (rows have 1..8 entries on these levels)
    for (int j0 = 0; j0 < width; j0 += 8, slot += 8 * kWave) {
        int c[8];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool ok = j0 + u < width;
            const int at = ok ? slot + u * kWave : slot;
            c[u] = cols[at];
            v[u] = ok ? vals[(size_t)at * vstride + vk] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fma(v[u], xl[c[u]], acc);
    }
    return acc;
}

// Many-step Chebyshev solve on the LAST tail level with the thread's matrix rows held in registers.  In tail_cheb every
// step re-reads the (index, value) pairs of its rows from L2 - two dependent round trips per step, ~3 us, while the
// arithmetic of a step on a few thousand rows takes a fraction of that; a degree-14 solve costs ~80 us that way.  Here a
// thread loads the pairs of its R rows (at most W entries each) once and all steps run on registers + LDS.
// Same recurrences and summation order as tail_cheb: bit-identical results.  Returns false (nothing done) when the
// level does not fit R rows per thread x W entries per row.
template <int R, int W>
PMC_TAIL_INLINE bool tail_cheb_cached(const TailLevelDev& L, int bv, int nb, int k, int degree, double ratio, const double* r,
                                 double* x, double* d) {
    const int n = L.n;
    if (n > R * kTailThreads) return false;
    const int vstride = bv == 1 ? nb : 1;
    const size_t vk = bv == 1 ? (size_t)k : bv == 2 ? (size_t)k * L.nslots : 0;
    const size_t dk = bv == 1 ? (size_t)k : bv == 2 ? (size_t)k * L.n : 0;
    // widths are uniform per slice; reject the level if any slice is wider than W (uniform decision: every thread scans
    // the same few slice offsets)
    for (int s = 0; s < L.nslices; ++s)
        if (((L.slice_off[s + 1] - L.slice_off[s]) >> 6) > W) return false;
    int c[R][W];
    double v[R][W], di[R], rr[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int i = threadIdx.x + q * kTailThreads;
        const bool live = i < n;
        const int row = live ? i : 0;
        const int slice = row >> 6, lane = row & 63;
        const int o = L.slice_off[slice];
        const int width = (L.slice_off[slice + 1] - o) >> 6;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const bool ok = live && j < width;
            const int at = o + (ok ? j : 0) * kWave + lane;
            c[q][j] = L.cols[at];
            const double val = L.vals[(size_t)at * vstride + vk];
            v[q][j] = ok ? val : 0.0;
        }
        di[q] = L.dinv[(size_t)row * vstride + dk];
        rr[q] = live ? r[row] : 0.0;
    }
    const double lmax = L.lmax, lmin = lmax / ratio;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho_old = 1.0 / sigma;
    // step 0 from a zero guess: d = x = dinv r / theta
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int i = threadIdx.x + q * kTailThreads;
        if (i < n) {
            const double t = di[q] * rr[q] / theta;
            d[i] = t;
            x[i] = t;
        }
    }
    __syncthreads();
    for (int step = 1; step < degree; ++step) {
        const double rho = 1.0 / (2.0 * sigma - rho_old);
        const double a = rho * rho_old, b = 2.0 * rho / delta;
        rho_old = rho;
        double dn[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = threadIdx.x + q * kTailThreads;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < W; ++j) acc = fma(v[q][j], x[c[q][j]], acc);
            dn[q] = i < n ? a * d[i] + b * di[q] * (rr[q] - acc) : 0.0;
        }
        __syncthreads();       // every gather of x is done before anyone updates it
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = threadIdx.x + q * kTailThreads;
            if (i < n) {
                d[i] = dn[q];
                x[i] += dn[q];
            }
        }
        __syncthreads();
    }
    return true;
}

// Chebyshev iteration on one tail level, in place: x (zero or given) -> x.  All threads participate.  The matrix is re-read
// from L2 every step; the many-step solve of the LAST tail level runs on register-cached rows instead (tail_cheb_cached).
PMC_TAIL_INLINE void tail_cheb(const TailLevelDev& L, int bv, int nb, int k, int degree, double ratio, bool zero_guess,
                          const double* r, double* x, double* d) {
    const int n = L.n;
    // value / diagonal addressing: shared, interleaved per realization, or transposed per realization
    const int vstride = bv == 1 ? nb : 1;
    const size_t vk = bv == 1 ? (size_t)k : bv == 2 ? (size_t)k * L.nslots : 0;
    const size_t dk = bv == 1 ? (size_t)k : bv == 2 ? (size_t)k * L.n : 0;
    const double lmax = L.lmax, lmin = lmax / ratio;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho_old = 1.0 / sigma;
    int step = 0;
    if (zero_guess && degree == 2 && L.vals_scaled) {
        const double rho1 = 1.0 / (2.0 * sigma - rho_old);
        const double c0 = (1.0 + rho1 * rho_old) / theta + 2.0 * rho1 / delta, c1 = 2.0 * rho1 / (delta * theta);
        for (int i = threadIdx.x; i < n; i += kTailThreads) {
            const double acc = tail_row_dot(L.slice_off, L.cols, L.vals_scaled, vstride, vk, i, r);
            x[i] = L.dinv[(size_t)i * vstride + dk] * (c0 * r[i] - c1 * acc);
        }
        __syncthreads();
        return;
    }
    if (zero_guess) {
        for (int i = threadIdx.x; i < n; i += kTailThreads) {
            const double v = L.dinv[(size_t)i * vstride + dk] * r[i] / theta;
            d[i] = v;
            x[i] = v;
        }
        __syncthreads();
        step = 1;
    }
    for (; step < degree; ++step) {
        double a, b;
        if (step == 0) {
            a = 0.0;
            b = 1.0 / theta;
        } else {
            const double rho = 1.0 / (2.0 * sigma - rho_old);
            a = rho * rho_old;
            b = 2.0 * rho / delta;
            rho_old = rho;
        }
        for (int i = threadIdx.x; i < n; i += kTailThreads) {
            const double acc = tail_row_dot(L.slice_off, L.cols, L.vals, vstride, vk, i, x);
            const double dold = (a != 0.0) ? d[i] : 0.0;
            d[i] = a * dold + b * L.dinv[(size_t)i * vstride + dk] * (r[i] - acc);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kTailThreads) x[i] += d[i];
        __syncthreads();
    }
}

// V-cycle over the tail levels for realization k: the right-hand side is in LDS at lev[0]'s r block on entry, the
// result in its x block on return.  All kTailThreads threads of the workgroup participate.
PMC_TAIL_INLINE void tail_vcycle_lds(const TailParams& P, int nb, int k, double* lds) {
    const int nlev = P.nlev;
    // down sweep
    int l = 0;
    for (;; ++l) {
        const TailLevelDev& L = P.lev[l];
        double* r = lds + L.lds_off;
        double* x = r + L.n;
        double* d = x + L.n;
        if (l == nlev - 1 && L.ainv) {   // exact coarse solve with the precomputed dense inverse (symmetric: read column-wise)
            const int n = L.n;
            for (int i = threadIdx.x; i < n; i += kTailThreads) {
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                int j = 0;
                for (; j + 3 < n; j += 4) {
                    s0 = fma(L.ainv[(size_t)j * n + i], r[j], s0);
                    s1 = fma(L.ainv[(size_t)(j + 1) * n + i], r[j + 1], s1);
                    s2 = fma(L.ainv[(size_t)(j + 2) * n + i], r[j + 2], s2);
                    s3 = fma(L.ainv[(size_t)(j + 3) * n + i], r[j + 3], s3);
                }
                for (; j < n; ++j) s0 = fma(L.ainv[(size_t)j * n + i], r[j], s0);
                x[i] = (s0 + s1) + (s2 + s3);
            }
            __syncthreads();
            break;
        }
        if (l == nlev - 1) {     // host guarantees last_degree > 0 on the final tail level
            // rows in registers: 3 rows x 5 entries (tets: 4 neighbours + diagonal) or 2 rows x 7 (hexahedra) per thread
            if (!(L.last_degree > 2 && (tail_cheb_cached<3, 5>(L, P.bv, nb, k, L.last_degree, L.last_ratio, r, x, d) ||
                                        tail_cheb_cached<2, 7>(L, P.bv, nb, k, L.last_degree, L.last_ratio, r, x, d))))
                tail_cheb(L, P.bv, nb, k, L.last_degree, L.last_ratio, true, r, x, d);
            break;
        }
        tail_cheb(L, P.bv, nb, k, P.smooth_degree, P.smooth_ratio, true, r, x, d);
        const int vstride = P.bv == 1 ? nb : 1;
        const size_t vk = P.bv == 1 ? (size_t)k : P.bv == 2 ? (size_t)k * L.nslots : 0;
        for (int i = threadIdx.x; i < L.n; i += kTailThreads)          // residual into d
            d[i] = r[i] - tail_row_dot(L.slice_off, L.cols, L.vals, vstride, vk, i, x);
        __syncthreads();
        const TailLevelDev& Lc = P.lev[l + 1];
        double* rc = lds + Lc.lds_off;
        for (int i = threadIdx.x; i < Lc.n; i += kTailThreads)         // restriction r_c = P^T res
            rc[i] = tail_row_dot(L.pt_off, L.pt_cols, L.pt_vals, 1, 0, i, d);
        __syncthreads();
    }
    // up sweep
    for (--l; l >= 0; --l) {
        const TailLevelDev& L = P.lev[l];
        double* r = lds + L.lds_off;
        double* x = r + L.n;
        double* d = x + L.n;
        const double* xc = lds + P.lev[l + 1].lds_off + P.lev[l + 1].n;
        for (int i = threadIdx.x; i < L.n; i += kTailThreads) x[i] += tail_row_dot(L.p_off, L.p_cols, L.p_vals, 1, 0, i, xc);
        __syncthreads();
        tail_cheb(L, P.bv, nb, k, P.smooth_degree, P.smooth_ratio, false, r, x, d);
    }
}

// out32: xout points at fp32 storage (the preconditioned Krylov vectors in fp32 storage, or the coarse correction of a cycle
// with fp32 inter-level vectors); in32: so does rin (the coarse right-hand side of such a cycle)
__global__ __launch_bounds__(kTailThreads) void mg_tail_kernel(const TailParams* __restrict__ pp, int nb,
                                                               const double* __restrict__ rin, double* __restrict__ xout,
                                                               double* __restrict__ partial, int out32, int in32) {
    extern __shared__ __align__(16) double lds[];
    __shared__ double red[kTailThreads / kWave];
    const TailParams& P = *pp;
    const int k = blockIdx.x;
    const TailLevelDev& L0 = P.lev[0];
    {
        double* r0 = lds + L0.lds_off;
        if (in32) {
            const float* rf = reinterpret_cast<const float*>(rin);
            for (int i = threadIdx.x; i < L0.n; i += kTailThreads) r0[i] = (double)rf[(size_t)i * nb + k];
        } else {
            for (int i = threadIdx.x; i < L0.n; i += kTailThreads) r0[i] = rin[(size_t)i * nb + k];
        }
    }
    __syncthreads();
    tail_vcycle_lds(P, nb, k, lds);
    const double* r0 = lds + L0.lds_off;
    const double* x0 = r0 + L0.n;
    double p = 0.0;
    for (int i = threadIdx.x; i < L0.n; i += kTailThreads) {
        double xi = x0[i];
        if (out32) {
            const float xf = (float)xi;
            reinterpret_cast<float*>(xout)[(size_t)i * nb + k] = xf;
            xi = (double)xf;
        } else {
            xout[(size_t)i * nb + k] = xi;
        }
        p = fma(r0[i], xi, p);
    }
    if (partial) {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) p += __shfl_down(p, off, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = p;
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (int w = 0; w < kTailThreads / kWave; ++w) sum += red[w];
            partial[k] = sum;     // one partial block: partial[0*nb + k]
        }
    }
}

// ------------------------------------------------------------------------------------------
// Persistent per-realization solver for SMALL levels (shared matrix values: the SPDE sampler).  As separate kernels a
// MINRES iteration on a ~17 k-row level is 7 launches of a few microseconds each - the GPU's dispatch rate, not its
// bandwidth, bounds the throughput.  Here ONE workgroup runs the whole preconditioned MINRES solve of ONE realization:
// operator, M-block polynomial, S-block V-cycle (the LDS tail above), dots and scalar recurrences, separated only by
// __syncthreads(); vectors live in a per-realization scratch area that stays in L2, no host round trip until the solve
// has finished.  Same recurrences, stopping rule and per-realization results as the batched kernels.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    __syncthreads();                                   // red may still be read from the previous call
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / kWave; ++w) s += red[w];   // same order in every thread: deterministic, no broadcast
    return s;
}

__global__ __launch_bounds__(kTailThreads) void mini_sampler_kernel(MiniSamplerParams P, int nb, const double* __restrict__ b,
                                                                     double* __restrict__ x, int zero_guess,
                                                                     double* __restrict__ scratch, pmc_stats* __restrict__ stats) {
    extern __shared__ __align__(16) double lds[];
    __shared__ double red[kTailThreads / kWave];
    const int k = blockIdx.x;
    const int n_u = P.n_u, n_s = P.n_s, n = n_u + n_s;
    const int tid = threadIdx.x;
    double* v0 = scratch + (size_t)k * P.scratch_per_col;
    double* v1 = v0 + n;
    double* u0 = v1 + n;
    double* u1 = u0 + n;
    double* q = u1 + n;
    double* w0 = q + n;
    double* w1 = w0 + P.x_nrows;
    double* xs = w1 + P.x_nrows;
    const TailParams& T = *P.tail;
    const TailLevelDev& L0 = T.lev[0];
    double* r0 = lds + L0.lds_off;
    const double* x0 = r0 + L0.n;

    // z = B^-1 r: u-block one-pass degree-2 polynomial in D^-1 M, s-block V-cycle in LDS; returns <r, z>
    auto prec = [&](const double* r, double* z) {
        double p = 0.0;
        for (int i = tid; i < n_u; i += kTailThreads) {
            const double acc = tail_row_dot(P.m_off, P.m_cols, P.m_scaled, 1, 0, i, r);
            const double zi = P.m_dinv[i] * (P.mc0 * r[i] - P.mc1 * acc);
            z[i] = zi;
            p = fma(r[i], zi, p);
        }
        for (int i = tid; i < n_s; i += kTailThreads) r0[i] = r[n_u + i];
        __syncthreads();
        tail_vcycle_lds(T, nb, k, lds);
        for (int i = tid; i < n_s; i += kTailThreads) {
            const double zi = x0[i];
            z[n_u + i] = zi;
            p = fma(r0[i], zi, p);
        }
        return block_sum(p, red);     // its barriers also order the z writes before the next phase reads them
    };

    // v1 = b - A x0
    if (zero_guess) {
        for (int i = tid; i < n; i += kTailThreads) v1[i] = b[(size_t)i * nb + k];
        for (int i = tid; i < P.x_nrows; i += kTailThreads) xs[i] = 0.0;
    } else {
        for (int i = tid; i < n; i += kTailThreads) u1[i] = x[(size_t)i * nb + k];
        __syncthreads();
        for (int i = tid; i < n; i += kTailThreads)
            v1[i] = b[(size_t)i * nb + k] - tail_row_dot(P.a_off, P.a_cols, P.a_vals, 1, 0, i, u1);
        for (int i = tid; i < P.x_nrows; i += kTailThreads) xs[i] = u1[P.x_row0 + i];
    }
    for (int i = tid; i < n; i += kTailThreads) v0[i] = 0.0;
    for (int i = tid; i < P.x_nrows; i += kTailThreads) { w0[i] = 0.0; w1[i] = 0.0; }
    __syncthreads();
    const double d0 = prec(v1, u1);
    double beta = d0 > 0.0 ? sqrt(d0) : 0.0, beta_old = 1.0, eta = beta;
    double gamma0 = 1.0, gamma1 = 1.0, sigma0 = 0.0, sigma1 = 0.0;
    const double eta0 = beta;
    const double goal = fmax(P.rel_tol * beta, P.abs_tol);
    int flag = (d0 < 0.0 || d0 != d0) ? -1 : 0;
    bool active = beta > goal && flag == 0;
    int it = 0;
    while (active && it < P.max_iter) {
        // q = A u1, <u1, q>
        double p = 0.0;
        for (int i = tid; i < n; i += kTailThreads) {
            const double qi = tail_row_dot(P.a_off, P.a_cols, P.a_vals, 1, 0, i, u1);
            q[i] = qi;
            p = fma(u1[i], qi, p);
        }
        const double d1 = block_sum(p, red);
        const double ib = 1.0 / beta;
        const double alpha = d1 * ib * ib;
        const double cV0 = ib, cV1 = -alpha * ib, cV2 = -beta / beta_old;
        const double delta = gamma1 * alpha - gamma0 * sigma1 * beta;
        const double rho3 = sigma0 * beta;
        const double rho2 = sigma1 * alpha + gamma0 * gamma1 * beta;
        for (int i = tid; i < n; i += kTailThreads) v0[i] = cV0 * q[i] + cV1 * v1[i] + cV2 * v0[i];
        __syncthreads();
        const double d2 = prec(v0, u0);
        if (d2 < 0.0 || d2 != d2) flag = -1;
        const double beta_new = d2 > 0.0 ? sqrt(d2) : 0.0;
        const double rho1 = hypot(delta, beta_new);
        const double ir = rho1 > 0.0 ? 1.0 / rho1 : 0.0;
        const double cW0 = ir / beta, cW1 = -rho3 * ir, cW2 = -rho2 * ir;
        gamma0 = gamma1;
        gamma1 = delta * ir;
        const double cW3 = gamma1 * eta;
        sigma0 = sigma1;
        sigma1 = beta_new * ir;
        eta = -sigma1 * eta;
        beta_old = beta;
        beta = beta_new;
        for (int i = tid; i < P.x_nrows; i += kTailThreads) {
            const double w = cW0 * u1[P.x_row0 + i] + cW1 * w0[i] + cW2 * w1[i];
            w0[i] = w;
            xs[i] += cW3 * w;
        }
        ++it;
        if (fabs(eta) <= goal || beta_new == 0.0 || flag != 0) active = false;
        // role swap (every thread holds the same pointers)
        double* t;
        t = u0; u0 = u1; u1 = t;
        t = v0; v0 = v1; v1 = t;
        t = w0; w0 = w1; w1 = t;
        __syncthreads();
    }
    for (int i = tid; i < P.x_nrows; i += kTailThreads) x[(size_t)(P.x_row0 + i) * nb + k] = xs[i];
    if (tid == 0) {
        stats[k].iterations = it;
        stats[k].converged = flag != 0 ? -1 : (fabs(eta) <= goal ? 1 : 0);   // -1: indefinite preconditioner / NaN
        stats[k].initial_norm = eta0;
        stats[k].final_norm = fabs(eta);
        stats[k].solve_ms = 0.0;      // filled on the host from the launch's events
        stats[k].setup_ms = 0.0;
    }
}

// ==========================================================================================
// launchers
namespace k {

void mini_sampler_solve(hipStream_t st, int nb, const MiniSamplerParams& P, size_t lds_doubles, const double* b, double* x,
                        bool zero_guess, double* scratch, pmc_stats* stats) {
    const size_t bytes = lds_doubles * sizeof(double);
    if (bytes > kTailLdsBytes) throw Error(PMC_ERR_INTERNAL, "mini solver: LDS request too large");
    static std::atomic<unsigned long long> attr_mask{0};
    int dev = 0;
    PMC_HIP(hipGetDevice(&dev));
    if (!(attr_mask.load() & (1ull << (dev & 63)))) {
        PMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mini_sampler_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)kTailLdsBytes));
        attr_mask.fetch_or(1ull << (dev & 63));
    }
    mini_sampler_kernel<<<nb, kTailThreads, bytes, st>>>(P, nb, b, x, zero_guess ? 1 : 0, scratch, stats);
    check_launch();
}

__global__ __launch_bounds__(kBlock) void transpose_bv_kernel(size_t count, int nb, const double* __restrict__ in,
                                                              double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;   // coalesced reads; the writes of a small array stay in L2
    if (e >= count * nb) return;
    const size_t i = e / nb;
    const int k = (int)(e % nb);
    out[(size_t)k * count + i] = in[e];
}

__global__ __launch_bounds__(kBlock) void transpose_bv32_kernel(size_t count, int nb, const float* __restrict__ in,
                                                                double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count * nb) return;
    const size_t i = e / nb;
    const int k = (int)(e % nb);
    out[(size_t)k * count + i] = (double)in[e];
}

void transpose_bv32(hipStream_t st, int nb, size_t count, const float* in, double* out) {
    if (count == 0) return;
    const size_t total = count * nb;
    transpose_bv32_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, st>>>(count, nb, in, out);
    check_launch();
}

void transpose_bv(hipStream_t st, int nb, size_t count, const double* in, double* out) {
    if (count == 0) return;
    const size_t total = count * nb;
    transpose_bv_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, st>>>(count, nb, in, out);
    check_launch();
}

// x[i][k] = sum_j ainv[i][j] r[j][k] for a launch of at most 8 realizations: one wavefront per row, lanes over the columns of the
// (symmetric, row-major) dense inverse, so the matrix is read once, coalesced, by n wavefronts spread over the chip - the exact
// solve of a level of a few hundred rows that a narrow launch would otherwise cycle through in ONE workgroup's LDS tail
// VT: storage of r and x (fp32 inside a cycle with fp32 inter-level vectors; the sums are fp64, rounded once on store)
template <typename VT>
__global__ __launch_bounds__(kBlock) void dense_apply_kernel(int n, int nb, const double* __restrict__ ainv,
                                                              const VT* __restrict__ r, VT* __restrict__ x) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (i >= n) return;
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    const double* row = ainv + (size_t)i * n;
    for (int j = lane; j < n; j += kWave) {
        const double a = row[j];
        const VT* rj = r + (size_t)j * nb;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nb) acc[k] = fma(a, (double)rj[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= nb) break;
        double v = acc[k];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (lane == 0) x[(size_t)i * nb + k] = (VT)v;
    }
}

void dense_apply(hipStream_t st, int nb, int n, const double* ainv, zvec r, zvec x) {
    if (r.f32 != x.f32) throw Error(PMC_ERR_INTERNAL, "dense_apply: right-hand side and result in different storage");
    if (nb < 1 || nb > 8) throw Error(PMC_ERR_INTERNAL, "dense_apply: serves launches of at most 8 realizations");
    if (n <= 0) return;
    const int rows_per_block = kBlock / kWave;
    const unsigned g = (unsigned)((n + rows_per_block - 1) / rows_per_block);
    if (r.f32) dense_apply_kernel<float><<<g, kBlock, 0, st>>>(n, nb, ainv, r.as<float>(), x.as<float>());
    else dense_apply_kernel<double><<<g, kBlock, 0, st>>>(n, nb, ainv, r.as<double>(), x.as<double>());
    check_launch();
}

int mg_tail(hipStream_t st, int nb, const TailParams* dev_params, size_t lds_doubles, const double* r, double* xout,
            double* dot_partial, bool out32, bool in32) {
    const size_t bytes = lds_doubles * sizeof(double);
    if (bytes > kTailLdsBytes) throw Error(PMC_ERR_INTERNAL, "mg_tail: LDS request too large");
    // the dynamic-LDS limit is a per-device function attribute: raise it once per device (idempotent if two lanes race)
    static std::atomic<unsigned long long> attr_mask{0};
    int dev = 0;
    PMC_HIP(hipGetDevice(&dev));
    if (!(attr_mask.load() & (1ull << (dev & 63)))) {
        PMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mg_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)kTailLdsBytes));
        attr_mask.fetch_or(1ull << (dev & 63));
    }
    mg_tail_kernel<<<nb, kTailThreads, bytes, st>>>(dev_params, nb, r, xout, dot_partial, out32 ? 1 : 0, in32 ? 1 : 0);
    check_launch();
    return dot_partial ? 1 : 0;
}

}  // namespace k
}  // namespace pmc

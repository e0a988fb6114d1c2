// MINRES vector and scalar kernels (K6): the flat element-wise kernels (first Chebyshev step, dots, conversions, Lanczos
// combination, w / x updates) and the single-block scalar recurrences with their partial-sum reductions; the library's
// launch counter.
#include "klaunch.hpp"

#include <cstddef>

#include <atomic>

namespace pmc {

static std::atomic<uint64_t> g_kernel_launches{0};
uint64_t kernel_launch_count() { return g_kernel_launches.load(std::memory_order_relaxed); }
void count_kernel_launches(int n) { g_kernel_launches.fetch_add((uint64_t)n, std::memory_order_relaxed); }

// MINRES w / x update restricted to an index list of rows: w, x are compact [nsel][NB], u is full
template <int NB, typename UT>
__global__ __launch_bounds__(kBlock) void minres_wx_idx_kernel(size_t nflat, const int* __restrict__ rows,
                                                               const double* __restrict__ c0, const UT* __restrict__ u,
                                                               const double* __restrict__ c1, double* __restrict__ w0,
                                                               const double* __restrict__ c2, const double* __restrict__ w1,
                                                               const double* __restrict__ c3, double* __restrict__ x, int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nflat) return;
    const size_t e = i * C;
    const size_t sel = e / W;
    const int k0 = (int)(e % W);
    double uv[C], w0v[C], w1v[C], xv[C];
    load_v<C>(u + (size_t)rows[sel] * W + k0, uv);
    load_c<C>(w0 + e, w0v);
    load_c<C>(w1 + e, w1v);
    load_c<C>(x + e, xv);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        w0v[c] = c0[k0 + c] * uv[c] + c1[k0 + c] * w0v[c] + c2[k0 + c] * w1v[c];
        xv[c] += c3[k0 + c] * w0v[c];
    }
    store_c<C>(w0 + e, w0v);
    store_c<C>(x + e, xv);
}

// ---- flat element-wise kernels: thread i owns the C doubles at flat index i*C, i.e. row (i*C)/NB and
// columns ((i*C) % NB) + c; consecutive lanes touch consecutive 16 B -> fully coalesced.  Grid-stride:
// the stride gridDim*256 is a multiple of T, so a thread keeps its column pair.
template <int NB, bool BV, bool DOT>
__global__ __launch_bounds__(kBlock) void cheb_first_kernel(size_t nflat, const double* __restrict__ dinv,
                                                            const double* __restrict__ r, double* __restrict__ d,
                                                            double* __restrict__ x, double b,
                                                            double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        const size_t e = i * C;
        double rv[C], di[C], xv[C];
        load_c<C>(r + e, rv);
        if constexpr (BV) {
            load_c<C>(dinv + e, di);
        } else {
            const double s = dinv[e / W];
#pragma unroll
            for (int c = 0; c < C; ++c) di[c] = s;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xv[c] = b * di[c] * rv[c];
            if constexpr (DOT) p[c] = fma(rv[c], xv[c], p[c]);
        }
        store_c<C>(d + e, xv);
        store_c<C>(x + e, xv);
    }
    if constexpr (DOT) reduce_flat_store<NB>(p, partial, W);
}

template <int NB, typename BT = double>
__global__ __launch_bounds__(kBlock) void dot_kernel(size_t nflat, const double* __restrict__ a,
                                                     const BT* __restrict__ b, double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    // grid-stride: the stride gridDim*256 is a multiple of T, so a thread keeps its column pair
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        double av[C], bv[C];
        load_c<C>(a + i * C, av);
        load_v<C>(b + i * C, bv);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = fma(av[c], bv[c], p[c]);
    }
    reduce_flat_store<NB>(p, partial, row_ld<NB>(ld));
}

// z = storage-rounded copy of a preconditioner result that a kernel without a typed output left in fp64, with the fused
// <r, z> of the rounded values (the paths off the hot configurations: higher-degree smoothers, algebraic transfers)
template <int NB, bool DOT, typename OT>
__global__ __launch_bounds__(kBlock) void convert_dot_kernel(size_t nflat, const double* __restrict__ in,
                                                             OT* __restrict__ out, const double* __restrict__ r,
                                                             double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        double v[C];
        load_c<C>(in + i * C, v);
        round_to<OT>(v);
        if constexpr (DOT) {
            double rv[C];
            load_c<C>(r + i * C, rv);
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = fma(rv[c], v[c], p[c]);
        }
        store_v<C>(out + i * C, v);
    }
    if constexpr (DOT) reduce_flat_store<NB>(p, partial, row_ld<NB>(ld));
}

// out = in and out32 = its fp32 copy in one pass (the first Lanczos vector of a solve from a zero guess: k::copy + k::convert_z)
template <int NB>
__global__ __launch_bounds__(kBlock) void copy_r32_kernel(size_t nflat, const double* __restrict__ in,
                                                          double* __restrict__ out, float* __restrict__ out32) {
    constexpr int C = Lay<NB>::C;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        double v[C];
        load_c<C>(in + i * C, v);
        store_c<C>(out + i * C, v);
        store_v<C>(out32 + i * C, v);
    }
}

// y32 (optional): the result is also written in fp32 - the copy the V-cycle's first two kernels gather and read (k::vc_*_r32)
template <int NB, bool NT = false>
__global__ __launch_bounds__(kBlock) void lincomb3_kernel(size_t nflat, const double* __restrict__ c0,
                                                          const double* __restrict__ a, const double* __restrict__ c1,
                                                          const double* __restrict__ b, const double* __restrict__ c2,
                                                          double* __restrict__ y, int ld, float* __restrict__ y32 = nullptr) {
    constexpr int C = Lay<NB>::C;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nflat) return;
    const size_t e = i * C;
    const int k0 = (int)(e % row_ld<NB>(ld));
    double av[C], bv[C], yv[C];
    load_c_nt<NT, C>(a + e, av);   // the three inputs are read once; the result is gathered by the next kernels
    load_c_nt<NT, C>(b + e, bv);
    load_c_nt<NT, C>(y + e, yv);
    lanczos_combine<C>(c0, c1, c2, k0, av, bv, yv);
    store_c<C>(y + e, yv);
    if (y32) store_v<C>(y32 + e, yv);
}

template <int NB, bool NT, typename UT>
__global__ __launch_bounds__(kBlock) void minres_wx_kernel(size_t nflat, const double* __restrict__ c0,
                                                           const UT* __restrict__ u, const double* __restrict__ c1,
                                                           double* __restrict__ w0, const double* __restrict__ c2,
                                                           const double* __restrict__ w1, const double* __restrict__ c3,
                                                           double* __restrict__ x, int ld) {
    constexpr int C = Lay<NB>::C;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nflat) return;
    const size_t e = i * C;
    const int k0 = (int)(e % row_ld<NB>(ld));
    double uv[C], w0v[C], w1v[C], xv[C];
    load_v_nt<NT, C>(u + e, uv);
    load_c_nt<NT, C>(w0 + e, w0v);
    load_c_nt<NT, C>(w1 + e, w1v);
    load_c_nt<NT, C>(x + e, xv);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        w0v[c] = c0[k0 + c] * uv[c] + c1[k0 + c] * w0v[c] + c2[k0 + c] * w1v[c];
        xv[c] += c3[k0 + c] * w0v[c];
    }
    store_c_nt<NT, C>(w0 + e, w0v);
    store_c_nt<NT, C>(x + e, xv);
}

// a flat vector entry in its storage type (fp32-stored vectors are widened only where they are consumed)
template <bool NT, typename UT, int C>
__device__ __forceinline__ void load_raw_nt(const UT* __restrict__ p, RawVec<UT, C>& r) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) r.v[i] = __builtin_nontemporal_load(p + i);
    } else {
        load_raw<C>(p, r);
    }
}

// The w / x updates of B.cnt <= kWxWindow iterations in one pass (see kWxWindow): the pending iterations are walked in
// trips - the u vectors of a trip are requested first (and stay in their storage type until their FMA), the recurrences
// then run in registers in iteration order, w0 / w1 / x stay in registers from trip to trip - the same operations in the
// same order as cnt successive minres_wx launches.  B.first: w0 and w1 are zero, and with B.x_zero so is x: they start as
// literal zeros (the same bits as a loaded +0.0); B.last: w0 / w1 are never read again and not stored.
//
// A thread owns R entries kBlock flat indices apart: kBlock * C is a multiple of every row stride, so the R entries lie in
// the same columns and one load of an iteration's four coefficient rows serves all of them.  With one entry per thread the
// coefficient loads - eight 16-byte loads per lane and iteration, against one of u - kept the vector memory pipeline busy
// six times as long as the payload did, and the pass ran at 0.42 of the HBM rate (LAB_NOTES 10.27).  A workgroup walks
// R * kBlock consecutive entries; entries past the end alias the thread's first one and are not stored.
template <typename UT, int C>
struct WxShape {
    static constexpr int R = sizeof(UT) == 4 ? 4 : 2;
    // u values in flight per lane: about 64 registers' worth, at most kWxDefer iterations
    static constexpr int Dfit = 64 / (R * C * (int)(sizeof(UT) / 4));
    static constexpr int D = Dfit < 1 ? 1 : (Dfit > k::kWxDefer ? k::kWxDefer : Dfit);
};
template <int NB, bool NT, typename UT>
__global__ __launch_bounds__(kBlock) void minres_wx_deferred_kernel(size_t nflat, k::WxDeferred B,
                                                                    const double* __restrict__ cW, double* __restrict__ w0,
                                                                    double* __restrict__ w1, double* __restrict__ x, int ld) {
    constexpr int C = Lay<NB>::C;
    constexpr int R = WxShape<UT, C>::R, D = WxShape<UT, C>::D;
    const size_t i0 = (size_t)blockIdx.x * (R * kBlock) + threadIdx.x;
    if (i0 >= nflat) return;
    const int k0 = (int)((i0 * C) % row_ld<NB>(ld));
    size_t e[R];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t i = i0 + (size_t)r * kBlock;
        live[r] = i < nflat;
        e[r] = (live[r] ? i : i0) * C;
    }
    double a[R][C], b[R][C], xv[R][C];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (B.first) {
#pragma unroll
            for (int c = 0; c < C; ++c) a[r][c] = b[r][c] = 0.0;
        } else {
            load_c_nt<NT, C>(w0 + e[r], a[r]);
            load_c_nt<NT, C>(w1 + e[r], b[r]);
        }
        if (B.first && B.x_zero) {
#pragma unroll
            for (int c = 0; c < C; ++c) xv[r][c] = 0.0;
        } else {
            load_c_nt<NT, C>(x + e[r], xv[r]);
        }
    }
    for (int t = 0; t < B.cnt; t += D) {
        RawVec<UT, C> uv[D][R];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (t + j < B.cnt) {
                const UT* up = static_cast<const UT*>(B.u[t + j]);
#pragma unroll
                for (int r = 0; r < R; ++r) load_raw_nt<NT>(up + e[r], uv[j][r]);
            }
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (t + j < B.cnt) {
                const double* cj = cW + (size_t)B.slot[t + j] * 4 * kMaxBatch + k0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const double wn = cj[c] * (double)uv[j][r].v[c] + cj[kMaxBatch + c] * a[r][c] + cj[2 * kMaxBatch + c] * b[r][c];
                        xv[r][c] += cj[3 * kMaxBatch + c] * wn;
                        a[r][c] = b[r][c];
                        b[r][c] = wn;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!live[r]) continue;
        if (!B.last) {
            store_c_nt<NT, C>(w0 + e[r], a[r]);
            store_c_nt<NT, C>(w1 + e[r], b[r]);
        }
        store_c_nt<NT, C>(x + e[r], xv[r]);
    }
}

// partial sums of <w, x[:,k]> with a shared (non-batched) weight vector w   (K15 QoI)
template <int NB>
__global__ __launch_bounds__(kBlock) void wdot_kernel(size_t nflat, const double* __restrict__ w,
                                                      const double* __restrict__ x, double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        double xv[C];
        load_c<C>(x + i * C, xv);
        const double ww = w[(i * C) / W];
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = fma(ww, xv[c], p[c]);
    }
    reduce_flat_store<NB>(p, partial, W);
}

__global__ void fill_kernel(size_t n, double* __restrict__ x, double v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) x[i] = v;
}

// ------------------------------------------------------------------------------------------
// MINRES scalar recurrences.  One block of 256 threads; thread k < nb owns column k.  Restates the
// preconditioned MINRES of Paige & Saunders in the form MFEM's MINRESSolver uses (normalised Lanczos
// vectors); the vectors are kept UNnormalised here and the 1/beta factors are folded into the
// update coefficients.
//
// Column sums of the per-block partials: thread t reads column t % nb of blocks t / nb, t / nb + 256/nb, ...
// (coalesced), then thread k adds the 256/nb group sums of its column in a fixed order (deterministic).
static constexpr int kScalBlock = 1024;
// Two segments (partial: nblocks blocks, partial2: nblocks2 blocks) are summed as one concatenated list: kernels that
// run side by side on two streams each write their own segment.
__device__ __forceinline__ double reduce_partials(const double* __restrict__ partial, int nblocks, int nb,
                                                  const double* __restrict__ partial2 = nullptr, int nblocks2 = 0) {
    __shared__ double lds[kScalBlock];
    const int k = threadIdx.x % nb, q = threadIdx.x / nb, nq = kScalBlock / reduce_width(nb);
    if (q >= nq) nblocks = nblocks2 = 0;   // nb = kGroup: the upper half of the threads adds nothing (see reduce_width)
    // eight independent chains keep the loads in flight (the partials of a 2 000-block launch are 36 values per thread)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    int b = q;
    for (; b + 7 * nq < nblocks; b += 8 * nq) {
        s0 += partial[(size_t)b * nb + k];
        s1 += partial[(size_t)(b + nq) * nb + k];
        s2 += partial[(size_t)(b + 2 * nq) * nb + k];
        s3 += partial[(size_t)(b + 3 * nq) * nb + k];
        s4 += partial[(size_t)(b + 4 * nq) * nb + k];
        s5 += partial[(size_t)(b + 5 * nq) * nb + k];
        s6 += partial[(size_t)(b + 6 * nq) * nb + k];
        s7 += partial[(size_t)(b + 7 * nq) * nb + k];
    }
    for (; b < nblocks; b += nq) s0 += partial[(size_t)b * nb + k];
    for (b = q; b + 3 * nq < nblocks2; b += 4 * nq) {
        s4 += partial2[(size_t)b * nb + k];
        s5 += partial2[(size_t)(b + nq) * nb + k];
        s6 += partial2[(size_t)(b + 2 * nq) * nb + k];
        s7 += partial2[(size_t)(b + 3 * nq) * nb + k];
    }
    for (; b < nblocks2; b += nq) s1 += partial2[(size_t)b * nb + k];
    s0 += s4;
    s1 += s5;
    s2 += s6;
    s3 += s7;
    const double s = (s0 + s1) + (s2 + s3);
    __syncthreads();
    lds[threadIdx.x] = s;
    __syncthreads();
    // narrow batches (nb < 32: the one-realization-per-call path hands over ONE column) leave 64 ... 1 024 groups per
    // column: fold them pairwise down to 32 before the serial sum - at nb = 1 thread 0 otherwise walks 1 024 dependent LDS
    // reads, 26 us per MINRES iteration of a 215 us iteration (round 5).  nb >= 32 takes the loop below unchanged.
    int groups = nq;
    for (int stride = nq >> 1; stride >= 32; stride >>= 1) {
        if (q < stride) lds[threadIdx.x] += lds[threadIdx.x + stride * nb];
        __syncthreads();
        groups = stride;
    }
    double t = 0.0;
    if ((int)threadIdx.x < nb)
        for (int g = 0; g < groups; ++g) t += lds[g * nb + threadIdx.x];
    return t;   // valid for threadIdx.x < nb
}

__device__ __forceinline__ void count_active(k::MinresState* st, int nb, bool bump) {
    __syncthreads();
    const int na = __syncthreads_count((int)threadIdx.x < nb && st->active[threadIdx.x] != 0);
    if (threadIdx.x == 0) {
        st->n_active = na;
        st->it = bump ? st->it + 1 : 0;
    }
}

__global__ __launch_bounds__(kScalBlock) void minres_init_kernel(k::MinresState* st, const double* __restrict__ partial,
                                                             int nblocks, int nb, double rel_tol, double abs_tol,
                                                             const double* __restrict__ partial2, int nblocks2, int ring) {
    if (threadIdx.x == 0) st->ring = ring;
    const double d = reduce_partials(partial, nblocks, nb, partial2, nblocks2);
    const int k = threadIdx.x;
    if (k < nb) {
        const double beta = d > 0.0 ? sqrt(d) : 0.0;
        st->beta[k] = beta;
        st->beta_old[k] = 1.0;
        st->eta[k] = beta;
        st->eta0[k] = beta;
        st->gamma0[k] = st->gamma1[k] = 1.0;
        st->sigma0[k] = st->sigma1[k] = 0.0;
        st->goal[k] = fmax(rel_tol * beta, abs_tol);
        st->iters[k] = 0;
        st->flag[k] = (d < 0.0 || d != d) ? -1 : 0;   // preconditioner not SPD / NaN
        st->active[k] = (beta > st->goal[k] && st->flag[k] == 0) ? 1 : 0;
    }
    count_active(st, nb, false);
}

// after q = A u1 and d1 = <u1, q>   (thread k < nb owns column k)
__device__ __forceinline__ void scal1_body(k::MinresState* st, int k, double d1) {
    if (st->active[k]) {
        const double beta = st->beta[k];
        const double ib = 1.0 / beta;
        const double alpha = d1 * ib * ib;
        st->alpha[k] = alpha;
        st->cV[0][k] = ib;                       // q / beta
        st->cV[1][k] = -alpha * ib;              // - alpha v1
        st->cV[2][k] = -beta / st->beta_old[k];  // - beta v0
        st->delta[k] = st->gamma1[k] * alpha - st->gamma0[k] * st->sigma1[k] * beta;
        st->rho3[k] = st->sigma0[k] * beta;
        st->rho2[k] = st->sigma1[k] * alpha + st->gamma0[k] * st->gamma1[k] * beta;
    } else {
        st->cV[0][k] = st->cV[1][k] = st->cV[2][k] = 0.0;
    }
}
// after z_new = prec(v_new) and d2 = <v_new, z_new>
__device__ __forceinline__ void scal2_body(k::MinresState* st, int k, double d2) {
    if (st->active[k]) {
        if (d2 < 0.0 || d2 != d2) st->flag[k] = -1;
        const double beta_new = d2 > 0.0 ? sqrt(d2) : 0.0;
        const double delta = st->delta[k];
        const double rho1 = hypot(delta, beta_new);
        const double ir = rho1 > 0.0 ? 1.0 / rho1 : 0.0;
        double (*cW)[kMaxBatch] = st->cW[st->it % st->ring];   // this iteration's coefficient set
        cW[0][k] = ir / st->beta[k];
        cW[1][k] = -st->rho3[k] * ir;
        cW[2][k] = -st->rho2[k] * ir;
        st->gamma0[k] = st->gamma1[k];
        st->gamma1[k] = delta * ir;
        cW[3][k] = st->gamma1[k] * st->eta[k];
        st->sigma0[k] = st->sigma1[k];
        st->sigma1[k] = beta_new * ir;
        st->eta[k] = -st->sigma1[k] * st->eta[k];
        st->beta_old[k] = st->beta[k];
        st->beta[k] = beta_new;
        st->iters[k] = st->it + 1;
        if (fabs(st->eta[k]) <= st->goal[k] || beta_new == 0.0 || st->flag[k] != 0) st->active[k] = 0;
    } else {
        double (*cW)[kMaxBatch] = st->cW[st->it % st->ring];
        cW[0][k] = cW[1][k] = cW[2][k] = cW[3][k] = 0.0;
    }
}

__global__ __launch_bounds__(kScalBlock) void minres_scal1_kernel(k::MinresState* st, const double* __restrict__ partial,
                                                              int nblocks, int nb, const double* __restrict__ partial2,
                                                              int nblocks2) {
    const double d1 = reduce_partials(partial, nblocks, nb, partial2, nblocks2);
    if ((int)threadIdx.x < nb) scal1_body(st, threadIdx.x, d1);
}

__global__ __launch_bounds__(kScalBlock) void minres_scal2_kernel(k::MinresState* st, const double* __restrict__ partial,
                                                              int nblocks, int nb, const double* __restrict__ partial2,
                                                              int nblocks2) {
    const double d2 = reduce_partials(partial, nblocks, nb, partial2, nblocks2);
    if ((int)threadIdx.x < nb) scal2_body(st, threadIdx.x, d2);
    count_active(st, nb, true);
}

// Both scalar steps in one launch: the recurrences of iteration i (from <v_new, z_new>) and, with the operator product
// of iteration i + 1 already done, the first half of iteration i + 1 (from <z_new, A z_new>).  One single-block launch
// per iteration instead of two.
__global__ __launch_bounds__(kScalBlock) void minres_scal21_kernel(k::MinresState* st, const double* __restrict__ pa,
                                                               int na, const double* __restrict__ pa2, int na2,
                                                               const double* __restrict__ pb, int nbk,
                                                               const double* __restrict__ pb2, int nbk2, int nb) {
    const double d2 = reduce_partials(pa, na, nb, pa2, na2);
    const double d1 = reduce_partials(pb, nbk, nb, pb2, nbk2);
    if ((int)threadIdx.x < nb) {
        scal2_body(st, threadIdx.x, d2);
        scal1_body(st, threadIdx.x, d1);          // same thread, same column: sees the state scal2 has just written
    }
    count_active(st, nb, true);
}

// First stage for long partial lists (a fine-level iteration hands ~4 600 blocks x nb values to the single-block scalar
// kernel, which then spends ~19 us on load latency alone): kStageBlocks workgroups sum contiguous chunks of the two dot
// products' lists into stage[list][g][nb]; the scalar kernel adds the kStageBlocks chunk sums in index order.  Fixed chunking
// and fixed order: deterministic.
static constexpr int kStageBlocks = 64;
__global__ __launch_bounds__(256) void stage_partials_kernel(const double* __restrict__ pa, int na,
                                                             const double* __restrict__ pa2, int na2,
                                                             const double* __restrict__ pb, int nbk,
                                                             const double* __restrict__ pb2, int nbk2, int nb,
                                                             double* __restrict__ stage) {
    __shared__ double lds[2][256];
    const int g = blockIdx.x, k = threadIdx.x % nb, q = threadIdx.x / nb, nq = 256 / reduce_width(nb);
    auto chunk = [&](const double* __restrict__ p, int n) {
        const int per = (n + kStageBlocks - 1) / kStageBlocks;
        const int lo = min(n, g * per), hi = q < nq ? min(n, lo + per) : lo;   // q >= nq: idle (see reduce_width)
        double a = 0.0, b = 0.0;
        int i = lo + q;
        for (; i + nq < hi; i += 2 * nq) {
            a += p[(size_t)i * nb + k];
            b += p[(size_t)(i + nq) * nb + k];
        }
        if (i < hi) a += p[(size_t)i * nb + k];
        return a + b;
    };
    lds[0][threadIdx.x] = chunk(pa, na) + chunk(pa2, na2);
    lds[1][threadIdx.x] = chunk(pb, nbk) + chunk(pb2, nbk2);
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * nb; e += 256) {   // nb up to 256: two entries per thread
        const int list = e / nb, c = e % nb;
        double t = 0.0;
        for (int j = 0; j < nq; ++j) t += lds[list][j * nb + c];
        stage[((size_t)list * kStageBlocks + g) * nb + c] = t;
    }
}

// out[k] = sum_b partial[b*nb+k]   (single block)
__global__ __launch_bounds__(kScalBlock) void reduce_final_kernel(const double* __restrict__ partial, int nblocks, int nb,
                                                              double* __restrict__ out) {
    const double s = reduce_partials(partial, nblocks, nb);
    if ((int)threadIdx.x < nb) out[threadIdx.x] = s;
}

// ==========================================================================================
// launchers
namespace k {

void minres_wx_idx(hipStream_t st, int nb, int nsel, const int* rows, const double* c0, zvec u, const double* c1,
                   double* w0, const double* c2, const double* w1, const double* c3, double* x) {
    if (nsel == 0) return;
    PMC_DISPATCH_NB(nb, dispatch_storage(u, [&](auto* up) {
        minres_wx_idx_kernel<NB><<<grid_flat(nsel, nb), kBlock, 0, st>>>(flat_count(nsel, nb), rows, c0, up, c1, w0, c2, w1, c3, x, nb);
    }));
    check_launch();
}

int cheb_first(hipStream_t st, int nb, int n, const double* dinv, bool dinv_bv, const double* r, double* d, double* x,
               double b, double* dot_partial) {
    if (n == 0) return 0;
    const size_t nf = flat_count(n, nb);
    const dim3 g = grid_bounded(grid_flat(n, nb), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, dispatch_bool(dinv_bv, [&](auto bv) {
        dispatch_bool(dot_partial != nullptr, [&](auto dot) {
            constexpr bool DOT = decltype(dot)::value;
            cheb_first_kernel<NB, decltype(bv)::value, DOT><<<g, kBlock, 0, st>>>(nf, dinv, r, d, x, b, DOT ? dot_partial : nullptr, nb);
        });
    }));
    check_launch();
    return dot_partial ? (int)g.x : 0;
}

int dot_z(hipStream_t st, int nb, int n, const double* a, zvec b, double* partial) {
    const dim3 g = grid_dot(n, nb);
    PMC_DISPATCH_NB(nb, dispatch_storage(b, [&](auto* bp) { dot_kernel<NB><<<g, kBlock, 0, st>>>(flat_count(n, nb), a, bp, partial, nb); }));
    check_launch();
    return (int)g.x;
}

int convert_z(hipStream_t st, int nb, int n, const double* in, zvec out, const double* r, double* dot_partial) {
    if (n == 0) return 0;
    const dim3 g = grid_dot(n, nb);
    PMC_DISPATCH_NB(nb, dispatch_storage(out, [&](auto* op) {
        dispatch_bool(dot_partial != nullptr, [&](auto dot) {
            constexpr bool DOT = decltype(dot)::value;
            convert_dot_kernel<NB, DOT><<<g, kBlock, 0, st>>>(flat_count(n, nb), in, op, DOT ? r : nullptr, DOT ? dot_partial : nullptr, nb);
        });
    }));
    check_launch();
    return dot_partial ? (int)g.x : 0;
}

void copy_r32(hipStream_t st, int nb, int n, const double* in, double* out, float* out32) {
    if (n == 0) return;
    PMC_DISPATCH_NB(nb, { copy_r32_kernel<NB><<<grid_dot(n, nb), kBlock, 0, st>>>(flat_count(n, nb), in, out, out32); });
    check_launch();
}

int wdot(hipStream_t st, int nb, int n, const double* w, const double* x, double* partial) {
    const dim3 g = grid_dot(n, nb);
    PMC_DISPATCH_NB(nb, { wdot_kernel<NB><<<g, kBlock, 0, st>>>(flat_count(n, nb), w, x, partial, nb); });
    check_launch();
    return (int)g.x;
}

void reduce_final(hipStream_t st, int nb, int nblocks, const double* partial, double* out) {
    reduce_final_kernel<<<1, kScalBlock, 0, st>>>(partial, nblocks, nb, out);
    check_launch();
}

void lincomb3(hipStream_t st, int nb, int n, const double* c0, const double* a, const double* c1, const double* b,
              const double* c2, double* y, float* y32) {
    // non-temporal loads on large levels (one lane 1104 -> 1129, four lanes 1400 -> 1412 samples/s); PMC_NT_LINCOMB=0: off
    static const bool nt_on = [] { const char* e = lab_env("PMC_NT_LINCOMB"); return !e || atoi(e) != 0; }();
    const bool nt = nt_on && nt_flat((size_t)n * nb);
    if (nt) count_solve_path(PMC_COUNT_NT_FLAT);
    PMC_DISPATCH_NB(nb, dispatch_bool(nt, [&](auto nt_c) {
        lincomb3_kernel<NB, decltype(nt_c)::value><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, a, c1, b, c2, y, nb, y32);
    }));
    check_launch();
}

void minres_wx(hipStream_t st, int nb, int n, const double* c0, zvec u, const double* c1, double* w0,
               const double* c2, const double* w1, const double* c3, double* x) {
    const bool nt = nt_flat((size_t)n * nb);
    if (nt) count_solve_path(PMC_COUNT_NT_FLAT);
    PMC_DISPATCH_NB(nb, dispatch_storage(u, [&](auto* up) {
        dispatch_bool(nt, [&](auto nt_c) {
            minres_wx_kernel<NB, decltype(nt_c)::value><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, up, c1, w0, c2, w1, c3, x, nb);
        });
    }));
    check_launch();
}

void minres_wx_deferred(hipStream_t st, int nb, int n, const MinresState* s, const WxDeferred& B, double* w0, double* w1,
                        double* x) {
    if (n == 0 || B.cnt == 0) return;
    if (B.cnt < 0 || B.cnt > kWxWindow) throw Error(PMC_ERR_INTERNAL, "minres_wx_deferred: bad count");
    const double* cW = reinterpret_cast<const double*>(reinterpret_cast<const char*>(s) + offsetof(MinresState, cW));
    const bool nt = nt_flat((size_t)n * nb);
    if (nt) count_solve_path(PMC_COUNT_NT_FLAT);
    // the entries of one thread share their columns (see the kernel): kBlock * C flat values are whole rows
    if ((kBlock * lay_c(nb)) % nb != 0) throw Error(PMC_ERR_INTERNAL, "minres_wx_deferred: row stride does not divide a workgroup's step");
    const size_t nf = flat_count(n, nb);
    PMC_DISPATCH_NB(nb, dispatch_f32(B.f32, [&](auto t) {   // (the u vectors travel inside B)
        dispatch_bool(nt, [&](auto nt_c) {
            using UT = typename decltype(t)::type;
            const dim3 g(wx_deferred_blocks(nf, WxShape<UT, Lay<NB>::C>::R));
            minres_wx_deferred_kernel<NB, decltype(nt_c)::value, UT><<<g, kBlock, 0, st>>>(nf, B, cW, w0, w1, x, nb);
        });
    }));
    check_launch();
}

void fill(hipStream_t st, size_t n, double* x, double v) {
    if (n == 0) return;
    if (v == 0.0) {
        PMC_HIP(hipMemsetAsync(x, 0, n * sizeof(double), st));
        return;
    }
    const unsigned g = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 2048);
    fill_kernel<<<g, kBlock, 0, st>>>(n, x, v);
    check_launch();
}

__global__ __launch_bounds__(kBlock) void scale_kernel(size_t n, const double* __restrict__ in, double a, double* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) out[i] = a * in[i];
}
void scale(hipStream_t st, size_t n, const double* in, double a, double* out) {
    if (n == 0) return;
    const unsigned g = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 2048);
    scale_kernel<<<g, kBlock, 0, st>>>(n, in, a, out);
    check_launch();
}

void copy(hipStream_t st, size_t n, const double* src, double* dst) {
    if (n && src != dst) PMC_HIP(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, st));
}

void minres_init(hipStream_t st, int nb, MinresState* s, const DotParts& d, double rel_tol, double abs_tol, int ring) {
    minres_init_kernel<<<1, kScalBlock, 0, st>>>(s, d.p1, d.n1, nb, rel_tol, abs_tol, d.p2, d.n2, ring);
    check_launch();
}
void minres_scal1(hipStream_t st, int nb, MinresState* s, const DotParts& d) {
    minres_scal1_kernel<<<1, kScalBlock, 0, st>>>(s, d.p1, d.n1, nb, d.p2, d.n2);
    check_launch();
}
void minres_scal2(hipStream_t st, int nb, MinresState* s, const DotParts& d) {
    minres_scal2_kernel<<<1, kScalBlock, 0, st>>>(s, d.p1, d.n1, nb, d.p2, d.n2);
    check_launch();
}
size_t scal_stage_doubles() { return (size_t)2 * kStageBlocks * kMaxBatch; }
void minres_scal21(hipStream_t st, int nb, MinresState* s, const DotParts& d2, const DotParts& d1, double* stage) {
    if (stage && d2.total() + d1.total() >= 8 * kStageBlocks) {
        stage_partials_kernel<<<kStageBlocks, 256, 0, st>>>(d2.p1, d2.n1, d2.p2, d2.n2, d1.p1, d1.n1, d1.p2, d1.n2, nb, stage);
        check_launch();
        minres_scal21_kernel<<<1, kScalBlock, 0, st>>>(s, stage, kStageBlocks, nullptr, 0,
                                                        stage + (size_t)kStageBlocks * nb, kStageBlocks, nullptr, 0, nb);
    } else {
        minres_scal21_kernel<<<1, kScalBlock, 0, st>>>(s, d2.p1, d2.n1, d2.p2, d2.n2, d1.p1, d1.n1, d1.p2, d1.n2, nb);
    }
    check_launch();
}

}  // namespace k
}  // namespace pmc

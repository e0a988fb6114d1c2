// Conditioning of the samplers' Gaussian fields on linear observations (kriging / Matheron's rule; an extension of this
// project, DESIGN.md section 15 - the reference has no counterpart):
//     g_c = g + K_l c,   c = A_l^-1 (y + R^1/2 zeta - H_l g),   K_l = C_l H_l^T,   A_l = 1/2 (H_l K_l + (H_l K_l)^T) + R.
// Setup (once per handle and level) runs the handle's own Eval twice per observation - t = EvalGaussian(W^-1/2 H_l^T e_j),
// K e_j = EvalGaussian(W^1/2 t) - or, on a KL handle, multiplies the device modes; A_l^-1 is a host Cholesky in long double.
// Per realization:
//   cond_coef_kernel    one workgroup per realization: the gather d = y + R^1/2 zeta - H_l g and c = A_l^-1 d, every sum in a
//                       fixed order, no atomics: a realization's coefficients do not depend on the others of the call.
//   cond_update_mfma    nb > 4: out = f(g + K c) as an fp64 GEMM on v_mfma_f64_16x16x4f64 with the operand maps of kl.hip; the
//                       accumulator starts from g, K streams from HBM once per workgroup column of up to 128 realizations,
//                       the coefficients are staged through a double-buffered LDS tile, the next chunk in registers while
//                       one is multiplied.  A lane reads exactly the entries of g it later writes: out may alias g.
//   cond_update_gemv    nb <= 4: one field row per lane, the observations split over the 4 waves of a workgroup.
// A column's bits may differ between the two update kernels (different summation order), as for the KL sampler.
//
// Derivatives of the map in g, Gamma = I - K A^-1 H:
//   tangent  f' o (Gamma dg): the kernels above with y = 0 (cond_coef_kernel's homogeneous mode) and exp() off, then o s_out.
//   adjoint  w = Gamma^T u = u - H^T A^-1 K^T u, u = v o s_out formed in the load (one rounding):
//     cond_adjoint_mfma / _gemv   t = K^T u as partials over chunks of kl_adjoint_chunk_rows(n) field rows, a function of n
//                       alone; the operand maps and LDS staging of kl_adjoint_mfma_kernel with K's leading dimension.  The
//                       workgroups of the first mode block store u to w while they stage it: u is read once.
//     cond_adjoint_finish_kernel  one workgroup per realization: the partials summed in ascending chunk order, c = A^-1 t
//                       (the mirror of cond_coef_kernel), then w -= H^T c at the touched columns only, each column's entries
//                       in ascending row order.  No atomics anywhere.
#include "handles.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <cmath>

namespace pmc {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kKc = 32;          // observations per LDS stage of the MFMA kernel
constexpr int kPad = 2;          // row stride kKc + 2 doubles = 68 dwords: the 16 rows x 2 k-quarters a 32-lane half reads with
                                 // ds_read_b64 (bank = dword address mod 64) land on banks 4 r + 2 kq, all distinct
constexpr int kWaves = 4;        // waves per workgroup (both update kernels); 16 field rows per wave in the MFMA kernel
constexpr int kMaxTiles = 8;     // realization tiles of 16 per MFMA workgroup: 128 realizations
constexpr int kCoefThreads = 256;
constexpr int kLaunchCols = 4096;   // realizations per launch (bounds the coefficient scratch; long calls are cut)
constexpr double kPivotRtol = 1e-12;   // fe/condition.py PIVOT_RTOL

// c[b mp + j] = sum_k Ainv[j][k] d[k],  d[k] = y[k] + sig[k] zeta[b nobs + k] - sum_p hv[p] g[b n + hci[p]]  (p in row k of H);
// c[b mp + j] = 0 for nobs <= j < mp.  Ainv is exactly symmetric: thread j reads column j, consecutive threads consecutive words.
__global__ __launch_bounds__(kCoefThreads) void cond_coef_kernel(int n, int nobs, int mp, const int* __restrict__ hrp,
                                                                 const int* __restrict__ hci, const double* __restrict__ hv,
                                                                 const double* __restrict__ y, const double* __restrict__ sig,
                                                                 const double* __restrict__ ainv, const double* __restrict__ g,
                                                                 const double* __restrict__ zeta, double* __restrict__ c) {
    __shared__ double d[kCondMaxObs];
    const size_t b = blockIdx.x;
    const double* gb = g + b * n;
    for (int j = threadIdx.x; j < nobs; j += kCoefThreads) {
        double hg = 0.0;
        for (int p = hrp[j]; p < hrp[j + 1]; ++p) hg = fma(hv[p], gb[hci[p]], hg);
        double v = y ? y[j] : 0.0;   // y == NULL: the homogeneous map (the tangent)
        if (zeta) v = fma(sig[j], zeta[b * nobs + j], v);
        d[j] = v - hg;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < mp; j += kCoefThreads) {
        double v = 0.0;
        if (j < nobs)
            for (int k = 0; k < nobs; ++k) v = fma(ainv[(size_t)k * nobs + j], d[k], v);
        c[b * mp + j] = v;
    }
}

// out[b n + i] = f(g[b n + i] + sum_k K[k ld + i] c[b mp + k]), k < mp (the columns nobs .. mp of K and c are zero).
// Operand maps as kl_mfma_kernel (kl.hip): A = c (rows: realizations), B = K^T (columns: field rows); lane l, register r of
// tile t holds realization b0 + 16 t + (l >> 4) + 4 r of field row i, so the accumulators load from g and store to out as 16
// consecutive doubles of one realization.  g and out carry no __restrict__: they may be the same array.
template <int NT>
__global__ __launch_bounds__(64 * kWaves, 2) void cond_update_mfma(int n, int ld, int mp, int nb, const double* __restrict__ K,
                                                                 const double* __restrict__ c, const double* g, double* out,
                                                                 int apply_exp) {
    constexpr int kStage = 16 * NT * kKc / (64 * kWaves);   // coefficients each thread stages per chunk
    __shared__ double xs[2][16 * NT][kKc + kPad];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (blockIdx.x * kWaves + wave) * 16 + (lane & 15);
    const int kq = lane >> 4;
    const int b0 = blockIdx.y * 16 * NT;
    const bool row_ok = i < n;
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 16 * t + kq + 4 * r;
            acc[t][r] = (row_ok && b < nb) ? g[(size_t)b * n + i] : 0.0;
        }
    }
    double bcur[kKc / 4], bnxt[kKc / 4], xr[kStage];
    auto load_chunk = [&](int ch, double* bq, double* xq) {
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) {
            const int k = ch * kKc + 4 * kk + kq;
            bq[kk] = (row_ok && k < mp) ? K[(size_t)k * ld + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kStage; ++j) {
            const int e = threadIdx.x + j * 64 * kWaves;
            const int b = b0 + e / kKc, k = ch * kKc + e % kKc;
            xq[j] = (b < nb && k < mp) ? c[(size_t)b * mp + k] : 0.0;
        }
    };
    load_chunk(0, bcur, xr);
    const int nchunks = (mp + kKc - 1) / kKc;
    for (int ch = 0; ch < nchunks; ++ch) {
        double (*x)[kKc + kPad] = xs[ch & 1];
#pragma unroll
        for (int j = 0; j < kStage; ++j) {
            const int e = threadIdx.x + j * 64 * kWaves;
            x[e / kKc][e % kKc] = xr[j];
        }
        // buffer ch & 1 was last read in chunk ch - 2; every wave has passed the barrier of chunk ch - 1 since
        __syncthreads();
        if (ch + 1 < nchunks) load_chunk(ch + 1, bnxt, xr);   // in flight while this chunk is multiplied
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t * 16 + (lane & 15)][4 * kk + kq], bcur[kk], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) bcur[kk] = bnxt[kk];
    }
    if (!row_ok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 16 * t + kq + 4 * r;
            if (b < nb) {
                const double v = acc[t][r];
                out[(size_t)b * n + i] = apply_exp ? exp(v) : v;
            }
        }
    }
}

constexpr int kGemvUnroll = 16;

template <int NB>
__global__ __launch_bounds__(64 * kWaves) void cond_update_gemv(int n, int ld, int m, int mp, const double* __restrict__ K,
                                                                const double* __restrict__ c, const double* g, double* out,
                                                                int apply_exp) {
    __shared__ double part[kWaves - 1][NB][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: c is read with scalar loads
    const int i = blockIdx.x * 64 + lane;
    const int per = (m + kWaves - 1) / kWaves;
    const int k_lo = wave * per, k_hi = min(m, k_lo + per);
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    if (i < n) {
        int k = k_lo;
        for (; k + kGemvUnroll <= k_hi; k += kGemvUnroll) {
            double p[kGemvUnroll];
#pragma unroll
            for (int u = 0; u < kGemvUnroll; ++u) p[u] = K[(size_t)(k + u) * ld + i];
#pragma unroll
            for (int u = 0; u < kGemvUnroll; ++u)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = fma(p[u], c[(size_t)b * mp + k + u], acc[b]);
        }
        for (; k < k_hi; ++k) {
            const double p = K[(size_t)k * ld + i];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = fma(p, c[(size_t)b * mp + k], acc[b]);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) part[wave - 1][b][lane] = acc[b];
    }
    __syncthreads();
    if (wave != 0 || i >= n) return;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double v = acc[b];
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) v += part[w][b][lane];
        const size_t o = (size_t)b * n + i;
        v += g[o];
        out[o] = apply_exp ? exp(v) : v;
    }
}

// ---- adjoint -------------------------------------------------------------------------------------------------------------------
constexpr int kAdjModes = 16 * kWaves;   // observations per MFMA workgroup: 16 per wave
constexpr int kAdjRows = 32;             // field rows per LDS stage
constexpr int kAdjLd = kAdjRows + 2;     // row stride of the LDS tiles in doubles: conflict-free as kLd of kl_adjoint.hip
constexpr int kAdjMaxLaunch = 256;       // realizations per launch (bounds the partials: chunks x 256 x nobs doubles)

// part[(chunk nb + b) m + k] = sum over the chunk's rows i of K[k ld + i] u[b n + i], u = v o sv (u = v when sv == NULL).
// A = U (rows: realizations, reduction: field rows), B = K (columns: observations): lane l, register r of tile t holds
// D[realization 16 t + (l >> 4) + 4 r][observation l & 15].  Rows past the chunk, observations past m and realizations past nb
// are staged as zeros: they add +0 products.  The workgroups of mode block 0 write u to w as they load it.
template <int NT>
__global__ __launch_bounds__(64 * kWaves) void cond_adjoint_mfma(int n, int ld, int m, int nb, int chunk_rows,
                                                                  const double* __restrict__ K, const double* __restrict__ v,
                                                                  const double* __restrict__ sv, double* __restrict__ w,
                                                                  double* __restrict__ part) {
    constexpr int kThreads = 64 * kWaves;
    constexpr int kP = kAdjModes * kAdjRows / kThreads;   // K entries each thread stages per step
    constexpr int kV = 16 * NT * kAdjRows / kThreads;     // U entries
    __shared__ double ps[kAdjModes][kAdjLd];
    __shared__ double vs[16 * NT][kAdjLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kq = lane >> 4;
    const int k0 = blockIdx.x * kAdjModes;
    const int chunk = blockIdx.y;
    const int b0 = blockIdx.z * 16 * NT;
    const int r0 = chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);
    const bool store_u = blockIdx.x == 0;
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double pr[kP], vr[kV];
    auto load_tile = [&](int i0) {
        const int i = i0 + (threadIdx.x & (kAdjRows - 1));
        const bool row_ok = i < r1;
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int k = k0 + (threadIdx.x + j * kThreads) / kAdjRows;
            pr[j] = (row_ok && k < m) ? K[(size_t)k * ld + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kV; ++j) {
            const int b = b0 + (threadIdx.x + j * kThreads) / kAdjRows;
            double x = 0.0;
            if (row_ok && b < nb) {
                const size_t o = (size_t)b * n + i;
                x = sv ? v[o] * sv[o] : v[o];
            }
            vr[j] = x;
        }
    };
    load_tile(r0);
    for (int i0 = r0; i0 < r1; i0 += kAdjRows) {
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int e = threadIdx.x + j * kThreads;
            ps[e / kAdjRows][e % kAdjRows] = pr[j];
        }
        // u goes to w here, where the staged values are consumed anyway: a store inside load_tile would wait for the loads
        // that are meant to stay in flight while the previous stage is multiplied
        const int iu = i0 + (threadIdx.x & (kAdjRows - 1));
#pragma unroll
        for (int j = 0; j < kV; ++j) {
            const int e = threadIdx.x + j * kThreads;
            vs[e / kAdjRows][e % kAdjRows] = vr[j];
            const int b = b0 + e / kAdjRows;
            if (store_u && iu < r1 && b < nb) w[(size_t)b * n + iu] = vr[j];
        }
        __syncthreads();
        if (i0 + kAdjRows < r1) load_tile(i0 + kAdjRows);   // in flight while this stage is multiplied
#pragma unroll
        for (int kk = 0; kk < kAdjRows / 4; ++kk) {
            const double b = ps[wave * 16 + (lane & 15)][4 * kk + kq];
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[t * 16 + (lane & 15)][4 * kk + kq], b, acc[t], 0, 0, 0);
        }
        __syncthreads();   // every wave has read the tiles before the next stage overwrites them
    }
    const int k = k0 + wave * 16 + (lane & 15);
    if (k >= m) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 16 * t + kq + 4 * r;
            if (b < nb) part[((size_t)chunk * nb + b) * m + k] = acc[t][r];
        }
    }
}

// nb <= 4: one observation per wave, the chunk's rows over the lanes, a fixed butterfly; the wave of observation 0 stores u
template <int NB>
__global__ __launch_bounds__(64 * kWaves) void cond_adjoint_gemv(int n, int ld, int m, int chunk_rows,
                                                                  const double* __restrict__ K, const double* __restrict__ v,
                                                                  const double* __restrict__ sv, double* __restrict__ w,
                                                                  double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= m) return;   // whole waves; the kernel has no barrier
    const int chunk = blockIdx.y;
    const int r0 = chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);
    const double* __restrict__ col = K + (size_t)k * ld;
    const bool store_u = k == 0;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
#pragma unroll 4
    for (int i = r0 + lane; i < r1; i += 64) {
        const double p = col[i];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const size_t o = (size_t)b * n + i;
            const double x = sv ? v[o] * sv[o] : v[o];
            if (store_u) w[o] = x;
            acc[b] = fma(p, x, acc[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double a = acc[b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
        if (lane == 0) part[((size_t)chunk * NB + b) * m + k] = a;
    }
}

// realization b = blockIdx.x: t[j] = sum over the chunks, ascending, of part[(chunk nb + b) nobs + j]; c = Ainv t (Ainv is
// exactly symmetric: thread j reads column j); w[b n + tcol[q]] -= sum_p tval[p] c[trow[p]], p in column q of H^T's
// compressed form, ascending.  Only the touched entries of w are read and written again.
__global__ __launch_bounds__(kCoefThreads) void cond_adjoint_finish_kernel(int n, int nobs, int nb, int nchunks, int tcols,
                                                                           const double* __restrict__ part,
                                                                           const double* __restrict__ ainv,
                                                                           const int* __restrict__ tcol, const int* __restrict__ tptr,
                                                                           const int* __restrict__ trow,
                                                                           const double* __restrict__ tval, double* __restrict__ w) {
    __shared__ double t[kCondMaxObs];
    __shared__ double c[kCondMaxObs];
    const size_t b = blockIdx.x;
    for (int j = threadIdx.x; j < nobs; j += kCoefThreads) {
        double a = part[b * nobs + j];
        for (int ch = 1; ch < nchunks; ++ch) a += part[((size_t)ch * nb + b) * nobs + j];
        t[j] = a;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nobs; j += kCoefThreads) {
        double a = 0.0;
        for (int k = 0; k < nobs; ++k) a = fma(ainv[(size_t)k * nobs + j], t[k], a);
        c[j] = a;
    }
    __syncthreads();
    double* wb = w + b * n;
    for (int q = threadIdx.x; q < tcols; q += kCoefThreads) {
        double a = 0.0;
        for (int p = tptr[q]; p < tptr[q + 1]; ++p) a = fma(tval[p], c[trow[p]], a);
        wb[tcol[q]] -= a;
    }
}

template <int NT>
void launch_adjoint_mfma(hipStream_t st, int n, int ld, int m, int nb, int chunk_rows, int nchunks, const double* K,
                         const double* v, const double* sv, double* w, double* part) {
    const dim3 grid((unsigned)((m + kAdjModes - 1) / kAdjModes), (unsigned)nchunks, (unsigned)((nb + 16 * NT - 1) / (16 * NT)));
    cond_adjoint_mfma<NT><<<grid, 64 * kWaves, 0, st>>>(n, ld, m, nb, chunk_rows, K, v, sv, w, part);
}

template <int NB>
void launch_adjoint_gemv(hipStream_t st, int n, int ld, int m, int chunk_rows, int nchunks, const double* K, const double* v,
                         const double* sv, double* w, double* part) {
    const dim3 grid((unsigned)((m + kWaves - 1) / kWaves), (unsigned)nchunks);
    cond_adjoint_gemv<NB><<<grid, 64 * kWaves, 0, st>>>(n, ld, m, chunk_rows, K, v, sv, w, part);
}

// out[i] *= s[i]: the f' = s_out of a lognormal field on the tangent
__global__ void cond_mul_inplace_kernel(size_t total, const double* __restrict__ s, double* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) out[t] *= s[t];
}

// ---- setup kernels ----------------------------------------------------------------------------------------------------------
// KL handle: mt[j m + k] = sum_p hv[p] phi[k n + hci[p]], p in row j of H  (row j of H_l Phi_l Lambda^1/2)
__global__ void cond_gather_modes_kernel(int n, int m, int nobs, const int* __restrict__ hrp, const int* __restrict__ hci,
                                         const double* __restrict__ hv, const double* __restrict__ phi, double* __restrict__ mt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * nobs) return;
    const int j = e / m, k = e % m;
    double acc = 0.0;
    for (int p = hrp[j]; p < hrp[j + 1]; ++p) acc = fma(hv[p], phi[(size_t)k * n + hci[p]], acc);
    mt[e] = acc;
}

// hk[r nobs + j] = sum_p hv[p] K[j ld + hci[p]], p in row r of H
__global__ void cond_hk_kernel(int nobs, int ld, const int* __restrict__ hrp, const int* __restrict__ hci,
                               const double* __restrict__ hv, const double* __restrict__ K, double* __restrict__ hk) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nobs * nobs) return;
    const int r = e / nobs, j = e % nobs;
    double acc = 0.0;
    for (int p = hrp[r]; p < hrp[r + 1]; ++p) acc = fma(hv[p], K[(size_t)j * ld + hci[p]], acc);
    hk[e] = acc;
}

template <int NT>
void launch_mfma(hipStream_t st, int n, int ld, int mp, int nb, const double* K, const double* c, const double* g, double* out,
                 bool apply_exp) {
    const dim3 grid((unsigned)((n + 16 * kWaves - 1) / (16 * kWaves)), (unsigned)((nb + 16 * NT - 1) / (16 * NT)));
    cond_update_mfma<NT><<<grid, 64 * kWaves, 0, st>>>(n, ld, mp, nb, K, c, g, out, apply_exp ? 1 : 0);
}

template <int NB>
void launch_gemv(hipStream_t st, int n, int ld, int m, int mp, const double* K, const double* c, const double* g, double* out,
                 bool apply_exp) {
    cond_update_gemv<NB><<<(unsigned)((n + 63) / 64), 64 * kWaves, 0, st>>>(n, ld, m, mp, K, c, g, out, apply_exp ? 1 : 0);
}

// smallest Cholesky pivot of the dense symmetric a (n x n) relative to its diagonal entry; -1 when a pivot is not finite
double min_relative_pivot(std::vector<double> a, int n) {
    double worst = 1.0;
    for (int j = 0; j < n; ++j) {
        const double ajj = a[(size_t)j * n + j];
        double dj = ajj;
        for (int k = 0; k < j; ++k) dj -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
        if (!std::isfinite(dj) || !(ajj > 0.0)) return -1.0;
        worst = std::min(worst, dj / ajj);
        if (!(dj > 0.0)) return worst;
        const double l = std::sqrt(dj);
        a[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double v = a[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) v -= a[(size_t)i * n + k] * a[(size_t)j * n + k];
            a[(size_t)i * n + j] = v / l;
        }
    }
    return worst;
}

// inv = a^-1 for the dense symmetric positive definite a (n x n), Cholesky and both triangular solves in long double on the
// host, rounded to double once and made exactly symmetric (cond_coef_kernel reads it either way round).  The coefficients are
// c = a^-1 d per realization: an inverse formed in double carries cond(a) eps, which at cond(a) = 3.5e3 showed as 2e-12 in
// exp() of fields of size 25; formed in extended precision its entries are correctly rounded to about
// one ulp and the product loses eps sum_k |a^-1_jk d_k| only.  Once per level at create: n <= 512.
bool spd_inverse_extended(const std::vector<double>& a_in, int n, std::vector<double>& inv) {
    typedef long double real;
    std::vector<real> a(a_in.begin(), a_in.end()), x((size_t)n * n, 0.0L), y((size_t)n);
    for (int j = 0; j < n; ++j) {   // a = L L^T (lower, in place)
        real dj = a[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) dj -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
        if (!(dj > 0.0L) || !std::isfinite((double)dj)) return false;
        const real l = std::sqrt(dj);
        a[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            real v = a[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) v -= a[(size_t)i * n + k] * a[(size_t)j * n + k];
            a[(size_t)i * n + j] = v / l;
        }
    }
    for (int c = 0; c < n; ++c) {   // column c of the inverse: L y = e_c, L^T x = y
        for (int i = c; i < n; ++i) {
            real v = i == c ? 1.0L : 0.0L;
            for (int k = c; k < i; ++k) v -= a[(size_t)i * n + k] * y[k];
            y[i] = v / a[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            real v = i >= c ? y[i] : 0.0L;
            for (int k = i + 1; k < n; ++k) v -= a[(size_t)k * n + i] * x[(size_t)k * n + c];
            x[(size_t)i * n + c] = v / a[(size_t)i * n + i];
        }
    }
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            inv[(size_t)i * n + j] = inv[(size_t)j * n + i] = (double)(0.5L * (x[(size_t)i * n + j] + x[(size_t)j * n + i]));
    return true;
}

}  // namespace

Conditioner::Conditioner(Sampler& s, int nobs_, const pmc_csr* H0, const double* y_in, const double* sigma2)
    : smp(s), nobs(nobs_), mp((nobs_ + 15) / 16 * 16) {
    PMC_REQUIRE(nobs >= 1 && nobs <= kCondMaxObs, "conditioner: nobs must be in [1, 512]");
    PMC_REQUIRE(H0 != nullptr && y_in != nullptr, "conditioner: H0 / y is NULL");
    for (int l = 0; l < smp.n_mc; ++l)
        PMC_REQUIRE(smp.lv[l].proj == PMC_PROJ_NONE, "conditioner: the handle has a projection set (pmc_sampler_set_projection); "
                                                     "embedded / L2-projected handles are not supported");
    HostCsr H = csr_from_c(*H0, true, "conditioner H0");
    PMC_REQUIRE(H.nrows == nobs, "conditioner: H0 must have nobs rows");
    PMC_REQUIRE(H.ncols == smp.lv[0].n_s, "conditioner: H0 must have n_s(0) columns");
    for (int r = 0; r < nobs; ++r)
        PMC_REQUIRE(H.rowptr[r + 1] > H.rowptr[r], "conditioner: row " + std::to_string(r) + " of H0 is empty");
    for (double v : H.vals) PMC_REQUIRE(std::isfinite(v), "conditioner: H0 has a non-finite entry");
    std::vector<double> sig((size_t)nobs, 0.0), R((size_t)nobs, 0.0);
    for (int j = 0; j < nobs; ++j) {
        PMC_REQUIRE(std::isfinite(y_in[j]), "conditioner: y is not finite");
        if (sigma2) {
            PMC_REQUIRE(std::isfinite(sigma2[j]) && sigma2[j] >= 0.0, "conditioner: sigma2 must be finite and >= 0");
            R[j] = sigma2[j];
            sig[j] = std::sqrt(sigma2[j]);
            noisy = noisy || sigma2[j] > 0.0;
        }
    }
    smp.ctx.activate();
    hipStream_t st = smp.ctx.stream;
    y.upload(y_in, (size_t)nobs, st);
    sqrt_sigma2.upload(sig, st);
    lv.resize((size_t)smp.n_mc);
    for (int l = 0; l < smp.n_mc; ++l) {
        Level& L = lv[l];
        L.n = smp.lv[l].n_s;
        L.ld = (L.n + 15) / 16 * 16;   // every 16-row segment of a column of K is one aligned 128-byte line
        if (l > 0) {
            H = csr_spgemm(H, smp.lv[l - 1].P_host);
            PMC_REQUIRE(H.ncols == L.n, "conditioner: the prolongator of level " + std::to_string(l - 1) + " has the wrong shape");
        }
        csr_sort_rows(H);
        L.H = H;
        L.hrp.upload(H.rowptr, st);
        L.hci.upload(H.colind, st);
        L.hv.upload(H.vals, st);
        {   // H_l^T compressed: the touched columns ascending, each column's entries in ascending row order
            std::vector<int> order((size_t)H.nnz()), rowof((size_t)H.nnz());
            for (int r = 0; r < nobs; ++r)
                for (int p = H.rowptr[r]; p < H.rowptr[r + 1]; ++p) rowof[(size_t)p] = r;
            for (size_t p = 0; p < order.size(); ++p) order[p] = (int)p;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return H.colind[a] < H.colind[b]; });
            std::vector<int> tcol, tptr, trow;
            std::vector<double> tval;
            for (int p : order) {
                if (tcol.empty() || tcol.back() != H.colind[p]) {
                    tcol.push_back(H.colind[p]);
                    tptr.push_back((int)trow.size());
                }
                trow.push_back(rowof[(size_t)p]);
                tval.push_back(H.vals[p]);
            }
            tptr.push_back((int)trow.size());
            L.tcols = (int)tcol.size();
            L.tcol.upload(tcol, st);
            L.tptr.upload(tptr, st);
            L.trow.upload(trow, st);
            L.tval.upload(tval, st);
            PMC_HIP(hipStreamSynchronize(st));   // the host vectors end here
        }
        L.K.alloc((size_t)L.ld * mp);
        L.K.zero(st);
        if (smp.kl) build_K_kl(l);
        else build_K_solves(l);
        // A = 1/2 (H K + (H K)^T) + R, inverted on the host
        DevBuf<double> hk_d((size_t)nobs * nobs);
        cond_hk_kernel<<<(unsigned)((nobs * nobs + 255) / 256), 256, 0, st>>>(nobs, L.ld, L.hrp.p, L.hci.p, L.hv.p, L.K.p, hk_d.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
        std::vector<double> hk((size_t)nobs * nobs);
        PMC_HIP(hipMemcpyAsync(hk.data(), hk_d.p, sizeof(double) * hk.size(), hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        L.A.assign((size_t)nobs * nobs, 0.0);
        for (int i = 0; i < nobs; ++i)
            for (int j = 0; j < nobs; ++j)
                L.A[(size_t)i * nobs + j] = 0.5 * (hk[(size_t)i * nobs + j] + hk[(size_t)j * nobs + i]) + (i == j ? R[i] : 0.0);
        std::vector<double> inv;
        const std::string bad = "conditioner: A of level " + std::to_string(l) + " is not positive definite (with exact data: two "
                                "observations inside one element of level " + std::to_string(l) + ")";
        PMC_REQUIRE(min_relative_pivot(L.A, nobs) > kPivotRtol, bad);
        PMC_REQUIRE(spd_inverse_extended(L.A, nobs, inv), bad);
        L.Ainv.upload(inv, st);
        PMC_HIP(hipStreamSynchronize(st));
    }
}

// column j of K_l by two applications of the handle's own Eval (Gaussian output, xi on `level`, zero initial guess, the
// handle's solver options), in batches of the level's launch width
void Conditioner::build_K_solves(int level) {
    Level& L = lv[level];
    hipStream_t st = smp.ctx.stream;
    const int n = L.n, W = smp.launch_width(level);
    std::vector<double> wsq((size_t)n);
    PMC_HIP(hipMemcpyAsync(wsq.data(), smp.lv[level].w_sqrt.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    std::vector<double> xi((size_t)n * W), t((size_t)n * W), dummy((size_t)n * W);
    for (int j0 = 0; j0 < nobs; j0 += W) {
        const int nb = std::min(W, nobs - j0);
        std::fill(xi.begin(), xi.begin() + (size_t)n * nb, 0.0);
        for (int b = 0; b < nb; ++b)
            for (int p = L.H.rowptr[j0 + b]; p < L.H.rowptr[j0 + b + 1]; ++p) {
                const int e = L.H.colind[p];
                xi[(size_t)b * n + e] += L.H.vals[p] / wsq[e];
            }
        smp.eval(level, level, nb, xi.data(), dummy.data(), nullptr, -1, false, t.data(), PMC_MEM_HOST, nullptr);
        for (int b = 0; b < nb; ++b)
            for (int e = 0; e < n; ++e) xi[(size_t)b * n + e] = wsq[e] * t[(size_t)b * n + e];
        smp.eval(level, level, nb, xi.data(), dummy.data(), nullptr, -1, false, t.data(), PMC_MEM_HOST, nullptr);
        PMC_HIP(hipMemcpy2DAsync(L.K.p + (size_t)j0 * L.ld, sizeof(double) * L.ld, t.data(), sizeof(double) * n, sizeof(double) * n,
                                 (size_t)nb, hipMemcpyHostToDevice, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

// K_l = (Phi_l Lambda^1/2) (Phi_l Lambda^1/2)^T H_l^T from the device modes
void Conditioner::build_K_kl(int level) {
    Level& L = lv[level];
    hipStream_t st = smp.ctx.stream;
    const int n = L.n, m = smp.kl_m;
    DevBuf<double> mt((size_t)m * nobs), tmp((size_t)n * nobs);
    cond_gather_modes_kernel<<<(unsigned)((m * nobs + 255) / 256), 256, 0, st>>>(n, m, nobs, L.hrp.p, L.hci.p, L.hv.p,
                                                                               smp.kl_phi[level].p, mt.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    kl_eval(st, n, m, nobs, smp.kl_phi[level].p, mt.p, m, tmp.p, nullptr, false);
    PMC_HIP(hipMemcpy2DAsync(L.K.p, sizeof(double) * L.ld, tmp.p, sizeof(double) * n, sizeof(double) * n, (size_t)nobs,
                             hipMemcpyDeviceToDevice, st));
    PMC_HIP(hipStreamSynchronize(st));
}

void Conditioner::apply_device(int level, int nbatch, const double* g_d, const double* zeta_d, double* out_d, bool apply_exp,
                               bool homogeneous, int call_width) {
    const Level& L = lv[level];
    hipStream_t st = smp.ctx.stream;
    const int n = L.n;
    coef.ensure((size_t)std::min(nbatch, kLaunchCols) * mp);
    // chosen per call, not per launch: the last launch of a long call stays on the MFMA path
    const bool wide = (call_width > 0 ? call_width : nbatch) > 4;
    for (int done = 0; done < nbatch; done += kLaunchCols) {
        const int nb = std::min(kLaunchCols, nbatch - done);
        const double* g = g_d + (size_t)done * n;
        double* out = out_d + (size_t)done * n;
        cond_coef_kernel<<<(unsigned)nb, kCoefThreads, 0, st>>>(n, nobs, mp, L.hrp.p, L.hci.p, L.hv.p, homogeneous ? nullptr : y.p,
                                                               sqrt_sigma2.p, L.Ainv.p, g,
                                                               zeta_d ? zeta_d + (size_t)done * nobs : nullptr, coef.p);
        if (wide) {
            const int tiles = (std::min(nb, 16 * kMaxTiles) + 15) / 16;
            if (tiles <= 1) launch_mfma<1>(st, n, L.ld, mp, nb, L.K.p, coef.p, g, out, apply_exp);
            else if (tiles <= 2) launch_mfma<2>(st, n, L.ld, mp, nb, L.K.p, coef.p, g, out, apply_exp);
            else if (tiles <= 4) launch_mfma<4>(st, n, L.ld, mp, nb, L.K.p, coef.p, g, out, apply_exp);
            else launch_mfma<8>(st, n, L.ld, mp, nb, L.K.p, coef.p, g, out, apply_exp);
        } else {
            switch (nb) {
                case 1: launch_gemv<1>(st, n, L.ld, nobs, mp, L.K.p, coef.p, g, out, apply_exp); break;
                case 2: launch_gemv<2>(st, n, L.ld, nobs, mp, L.K.p, coef.p, g, out, apply_exp); break;
                case 3: launch_gemv<3>(st, n, L.ld, nobs, mp, L.K.p, coef.p, g, out, apply_exp); break;
                default: launch_gemv<4>(st, n, L.ld, nobs, mp, L.K.p, coef.p, g, out, apply_exp); break;
            }
        }
        PMC_HIP(hipGetLastError());
        count_kernel_launches(2);
    }
}

void Conditioner::apply(int level, int nbatch, const double* g, const double* zeta, double* out, bool apply_exp, int memspace) {
    PMC_REQUIRE(level >= 0 && level < (int)lv.size(), "conditioner apply: level out of range");
    PMC_REQUIRE(nbatch >= 1 && g != nullptr && out != nullptr, "conditioner apply: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "conditioner apply: bad memspace");
    PMC_REQUIRE(!noisy || zeta != nullptr, "conditioner apply: zeta is NULL but some sigma2 > 0");
    PMC_REQUIRE(noisy || zeta == nullptr, "conditioner apply: zeta given for exact data (every sigma2 is 0)");
    smp.ctx.activate();
    hipStream_t st = smp.ctx.stream;
    if (memspace == PMC_MEM_DEVICE) {
        apply_device(level, nbatch, g, zeta, out, apply_exp);
        return;
    }
    const int n = lv[level].n;
    stage_g.ensure((size_t)nbatch * n);
    PMC_HIP(hipMemcpyAsync(stage_g.p, g, sizeof(double) * n * nbatch, hipMemcpyHostToDevice, st));
    if (zeta) {
        stage_z.ensure((size_t)nbatch * nobs);
        PMC_HIP(hipMemcpyAsync(stage_z.p, zeta, sizeof(double) * nobs * nbatch, hipMemcpyHostToDevice, st));
    }
    apply_device(level, nbatch, stage_g.p, zeta ? stage_z.p : nullptr, stage_g.p, apply_exp);
    PMC_HIP(hipMemcpyAsync(out, stage_g.p, sizeof(double) * n * nbatch, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
}

void Conditioner::apply_tangent(int level, int nbatch, const double* dg, const double* s_out, double* out, int memspace) {
    PMC_REQUIRE(level >= 0 && level < (int)lv.size(), "conditioner apply_tangent: level out of range");
    PMC_REQUIRE(nbatch >= 1 && dg != nullptr && out != nullptr, "conditioner apply_tangent: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "conditioner apply_tangent: bad memspace");
    PMC_REQUIRE(out != s_out, "conditioner apply_tangent: out must not alias s_out");
    smp.ctx.activate();
    hipStream_t st = smp.ctx.stream;
    const size_t total = (size_t)lv[level].n * nbatch;
    if (memspace == PMC_MEM_DEVICE) {
        apply_device(level, nbatch, dg, nullptr, out, false, true);
        if (s_out) {
            cond_mul_inplace_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(total, s_out, out);
            PMC_HIP(hipGetLastError());
            count_kernel_launches(1);
        }
        return;
    }
    stage_g.ensure(total);
    PMC_HIP(hipMemcpyAsync(stage_g.p, dg, sizeof(double) * total, hipMemcpyHostToDevice, st));
    apply_device(level, nbatch, stage_g.p, nullptr, stage_g.p, false, true);
    PMC_HIP(hipMemcpyAsync(out, stage_g.p, sizeof(double) * total, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    if (s_out)   // host arrays are staged, so the product is the host's (the same single rounding)
        for (size_t i = 0; i < total; ++i) out[i] *= s_out[i];
}

void Conditioner::apply_adjoint_device(int level, int nbatch, const double* v_d, const double* s_d, double* out_d,
                                       int call_width) {
    const Level& L = lv[level];
    hipStream_t st = smp.ctx.stream;
    const int n = L.n;
    const int cr = kl_adjoint_chunk_rows(n);
    const int nchunks = (n + cr - 1) / cr;
    adj_part.ensure((size_t)nchunks * (size_t)std::min(nbatch, kAdjMaxLaunch) * (size_t)nobs);
    const bool wide = (call_width > 0 ? call_width : nbatch) > 4;   // decided by the CALL, as everywhere in this file
    for (int done = 0; done < nbatch; done += kAdjMaxLaunch) {
        const int nb = std::min(kAdjMaxLaunch, nbatch - done);
        const double* v = v_d + (size_t)done * n;
        const double* sv = s_d ? s_d + (size_t)done * n : nullptr;
        double* w = out_d + (size_t)done * n;
        if (wide) {
            // Realization tiles per workgroup: 2 per mode block of kAdjModes observations, at most kMaxTiles.  The grid is
            // (mode blocks) x (chunks, at most 32) x (tiles / NT): with up to 64 observations, 8 tiles per workgroup leave
            // 32 - 64 workgroups for 256 CUs (measured at n = 262 144, nobs = 64: 0.99 ms for 256 realizations against 0.47 ms
            // with 2 tiles); K is re-read once per workgroup row of tiles, which more mode blocks (a larger K) make rarer.
            // A column's bits do not depend on NT.
            const int cap = std::min(kMaxTiles, 2 * ((nobs + kAdjModes - 1) / kAdjModes));
            const int tiles = (std::min(nb, 16 * cap) + 15) / 16;
            if (tiles <= 1) launch_adjoint_mfma<1>(st, n, L.ld, nobs, nb, cr, nchunks, L.K.p, v, sv, w, adj_part.p);
            else if (tiles <= 2) launch_adjoint_mfma<2>(st, n, L.ld, nobs, nb, cr, nchunks, L.K.p, v, sv, w, adj_part.p);
            else if (tiles <= 4) launch_adjoint_mfma<4>(st, n, L.ld, nobs, nb, cr, nchunks, L.K.p, v, sv, w, adj_part.p);
            else launch_adjoint_mfma<8>(st, n, L.ld, nobs, nb, cr, nchunks, L.K.p, v, sv, w, adj_part.p);
        } else {
            switch (nb) {
                case 1: launch_adjoint_gemv<1>(st, n, L.ld, nobs, cr, nchunks, L.K.p, v, sv, w, adj_part.p); break;
                case 2: launch_adjoint_gemv<2>(st, n, L.ld, nobs, cr, nchunks, L.K.p, v, sv, w, adj_part.p); break;
                case 3: launch_adjoint_gemv<3>(st, n, L.ld, nobs, cr, nchunks, L.K.p, v, sv, w, adj_part.p); break;
                default: launch_adjoint_gemv<4>(st, n, L.ld, nobs, cr, nchunks, L.K.p, v, sv, w, adj_part.p); break;
            }
        }
        PMC_HIP(hipGetLastError());
        cond_adjoint_finish_kernel<<<(unsigned)nb, kCoefThreads, 0, st>>>(n, nobs, nb, nchunks, L.tcols, adj_part.p, L.Ainv.p,
                                                                         L.tcol.p, L.tptr.p, L.trow.p, L.tval.p, w);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(2);
    }
}

void Conditioner::apply_adjoint(int level, int nbatch, const double* v, const double* s_out, double* out, int memspace) {
    PMC_REQUIRE(level >= 0 && level < (int)lv.size(), "conditioner apply_adjoint: level out of range");
    PMC_REQUIRE(nbatch >= 1 && v != nullptr && out != nullptr, "conditioner apply_adjoint: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "conditioner apply_adjoint: bad memspace");
    PMC_REQUIRE(out != v && out != s_out, "conditioner apply_adjoint: out must not alias v or s_out");
    smp.ctx.activate();
    hipStream_t st = smp.ctx.stream;
    if (memspace == PMC_MEM_DEVICE) {
        apply_adjoint_device(level, nbatch, v, s_out, out);
        return;
    }
    const size_t total = (size_t)lv[level].n * nbatch;
    stage_g.ensure(total);
    stage_w.ensure(total);
    PMC_HIP(hipMemcpyAsync(stage_g.p, v, sizeof(double) * total, hipMemcpyHostToDevice, st));
    if (s_out) {
        stage_s.ensure(total);
        PMC_HIP(hipMemcpyAsync(stage_s.p, s_out, sizeof(double) * total, hipMemcpyHostToDevice, st));
    }
    apply_adjoint_device(level, nbatch, stage_g.p, s_out ? stage_s.p : nullptr, stage_w.p);
    PMC_HIP(hipMemcpyAsync(out, stage_w.p, sizeof(double) * total, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
}

void Conditioner::export_level(int level, int* n_out, int64_t* nnz_out, double* K_out, double* A_out, int32_t* rowptr,
                               int32_t* colind, double* vals) const {
    PMC_REQUIRE(level >= 0 && level < (int)lv.size(), "pmc_conditioner_level: level out of range");
    const Level& L = lv[level];
    if (n_out) *n_out = L.n;
    if (nnz_out) *nnz_out = L.H.nnz();
    if (K_out) {
        smp.ctx.activate();
        hipStream_t st = smp.ctx.stream;
        PMC_HIP(hipMemcpy2DAsync(K_out, sizeof(double) * L.n, L.K.p, sizeof(double) * L.ld, sizeof(double) * L.n, (size_t)nobs,
                                 hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
    if (A_out) std::copy(L.A.begin(), L.A.end(), A_out);
    if (rowptr) std::copy(L.H.rowptr.begin(), L.H.rowptr.end(), rowptr);
    if (colind) std::copy(L.H.colind.begin(), L.H.colind.end(), colind);
    if (vals) std::copy(L.H.vals.begin(), L.H.vals.end(), vals);
}

}  // namespace pmc

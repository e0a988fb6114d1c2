// Darcy kernels (K12-K15): the element-grouped per-realization mass matrix M(k) (pair product, one-pass polynomial), column
// scaling of per-realization values, per-sample assembly with BC elimination, Schur refresh, diagonals, Gershgorin scaling,
// back-substitution of the hybridized system.
#include "klaunch.hpp"
#include "sell_rows.hpp"

namespace pmc {

// row steps per pass of the element-grouped kernels
template <int NB>
struct EgPass {
    static constexpr int TH = NB >= 32 ? 4 : Lay<NB>::T;   // only the widest instantiation (256 VGPRs, one wave per SIMD otherwise)
};

// Element-grouped per-realization mass matrix (EgView): acc = c1 * (group 1 row sums) + c2 * (group 2 row sums), for the row
// steps rs0 .. rs0 + TH - 1 of the slice.  The two coefficient rows are requested before the sweeps they scale.
// kEgNt: non-temporal matrix / result streams on large levels (hex 64^3, one lane: 28.2 -> 27.3 ms per 16 Darcy solves).
template <int NB, bool CS, bool kEgNt, int TH, typename XT = double>
__device__ __forceinline__ void eg_row_product(const int* __restrict__ cols, const double* __restrict__ w,
                                               const int* __restrict__ e12, const double* __restrict__ coef, int gw,
                                               const XT* __restrict__ x, const double* __restrict__ cs, int nrows,
                                               int slice, int lane, int LD, int rs0, double (&y)[TH][Lay<NB>::C]) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int g = lane / T, t = lane % T;
    const int off = slice * 2 * gw * kWave;
    double a[TH][C], c1[TH][C];
    // lean variant (fp32 x, three waves per SIMD instead of two): only the coefficient-row INDICES are fetched ahead of a
    // sweep, the rows themselves after it - 2 TH C registers fewer live while the gathers are in flight
    constexpr bool LATE = lean_part<NB, CS, XT>() && kEgLateCoef;
    int e1[TH];
#pragma unroll
    for (int q = 0; q < TH; ++q) {
        const int row = min(slice * kWave + (rs0 + q) * G + g, nrows - 1);
        if constexpr (LATE) e1[q] = e12[2 * row];
        else load_c<C>(coef + (size_t)e12[2 * row] * LD + t * C, c1[q]);
    }
    sell_row_part<NB, CS, true, kEgNt, TH, XT>(cols, w, x, cs, off, gw, lane, LD, rs0, a);
    if constexpr (LATE) {
#pragma unroll
        for (int q = 0; q < TH; ++q) load_c<C>(coef + (size_t)e1[q] * LD + t * C, c1[q]);
    }
#pragma unroll
    for (int q = 0; q < TH; ++q)
#pragma unroll
        for (int c = 0; c < C; ++c) y[q][c] = c1[q][c] * a[q][c];
#pragma unroll
    for (int q = 0; q < TH; ++q) {
        const int row = min(slice * kWave + (rs0 + q) * G + g, nrows - 1);
        if constexpr (LATE) e1[q] = e12[2 * row + 1];
        else load_c<C>(coef + (size_t)e12[2 * row + 1] * LD + t * C, c1[q]);
    }
    sell_row_part<NB, CS, true, kEgNt, TH, XT>(cols, w, x, cs, off + gw * kWave, gw, lane, LD, rs0, a);
    if constexpr (LATE) {
#pragma unroll
        for (int q = 0; q < TH; ++q) load_c<C>(coef + (size_t)e1[q] * LD + t * C, c1[q]);
    }
#pragma unroll
    for (int q = 0; q < TH; ++q)
#pragma unroll
        for (int c = 0; c < C; ++c) y[q][c] = fma(c1[q][c], a[q][c], y[q][c]);
}

template <int NB, bool DOT, bool kEgNt = false, typename XT = double>
__global__ __launch_bounds__(kBlock) void eg_pair_spmm_kernel(
    int nrows, int nslices, int gw, const int* __restrict__ cols1, const double* __restrict__ w1,
    const int* __restrict__ e12, const double* __restrict__ coef, const int* __restrict__ off2,
    const int* __restrict__ cols2, const double* __restrict__ vals2, const XT* __restrict__ x1,
    const typename ident<XT>::type* __restrict__ x2, double* __restrict__ y,
    const typename ident<XT>::type* __restrict__ dot_with, double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        coef += c0; x1 += c0; x2 += c0; y += c0;
        if constexpr (DOT) { dot_with += c0; partial += c0; }
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    constexpr int TH = EgPass<NB>::TH;
    const SliceWalk sw = slice_walk(nslices);
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        const int o2 = off2[slice];
        const int w2 = (off2[slice + 1] - o2) >> 6;
#pragma unroll 1
        for (int rs0 = 0; rs0 < T; rs0 += TH) {
            double acc[TH][C];
            eg_row_product<NB, false, kEgNt, TH, XT>(cols1, w1, e12, coef, gw, x1, nullptr, nrows, slice, lane, LD, rs0, acc);
            sell_row_part<NB, false, false, kEgNt, TH, XT>(cols2, vals2, x2, nullptr, o2, w2, lane, LD, rs0, acc);
            // the dot operand of all TH row steps is requested at once (rows past the end re-read the last row): the guarded
            // per-row-step form left the compiler one load - wait - fma chain per row step
            double wv[DOT ? TH : 1][C];
            if constexpr (DOT) {
#pragma unroll
                for (int q = 0; q < TH; ++q) {
                    const int rowc = min(slice * kWave + (rs0 + q) * G + g, nrows - 1);
                    load_v<C>(dot_with + (size_t)rowc * LD + t * C, wv[q]);
                }
                pin_block(wv);
            }
#pragma unroll
            for (int q = 0; q < TH; ++q) {
                const int row = slice * kWave + (rs0 + q) * G + g;
                if (row >= nrows) continue;
                const size_t at = (size_t)row * LD + t * C;
                store_c_stream<kEgNt, C>(y + at, acc[q]);
                if constexpr (DOT) {
#pragma unroll
                    for (int c = 0; c < C; ++c) p[c] = fma(wv[q][c], acc[q][c], p[c]);
                }
            }
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

template <int NB, bool DOT, bool kEgNt = false, typename OT = double>
__global__ __launch_bounds__(kBlock) void eg_poly2_kernel(int nrows, int nslices, int gw, const int* __restrict__ cols,
                                                          const double* __restrict__ w, const int* __restrict__ e12,
                                                          const double* __restrict__ coef,
                                                          const double* __restrict__ dinv, const double* __restrict__ r,
                                                          OT* __restrict__ xout, double c0, double c1,
                                                          double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int g0 = col0<NB>();
        coef += g0; dinv += g0; r += g0; xout += g0;
        if constexpr (DOT) partial += g0;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    constexpr int TH = EgPass<NB>::TH;
    const SliceWalk sw = slice_walk(nslices);
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
#pragma unroll 1
        for (int rs0 = 0; rs0 < T; rs0 += TH) {
            double acc[TH][C];
            eg_row_product<NB, true, kEgNt, TH>(cols, w, e12, coef, gw, r, dinv, nrows, slice, lane, LD, rs0, acc);
            // own-row reads of all TH row steps at once (see eg_pair_spmm_kernel)
            double rv[TH][C], di[TH][C];
#pragma unroll
            for (int q = 0; q < TH; ++q) {
                const size_t atc = (size_t)min(slice * kWave + (rs0 + q) * G + g, nrows - 1) * LD + t * C;
                load_c<C>(r + atc, rv[q]);
                load_c<C>(dinv + atc, di[q]);
            }
            pin_block(rv);
            pin_block(di);
#pragma unroll
            for (int q = 0; q < TH; ++q) {
                const int row = slice * kWave + (rs0 + q) * G + g;
                if (row >= nrows) continue;
                const size_t at = (size_t)row * LD + t * C;
                double xv[C];
#pragma unroll
                for (int c = 0; c < C; ++c) xv[c] = di[q][c] * (c0 * rv[q][c] - c1 * acc[q][c]);
                round_to<OT>(xv);
                if constexpr (DOT) {
#pragma unroll
                    for (int c = 0; c < C; ++c) p[c] = fma(rv[q][c], xv[c], p[c]);
                }
                store_v_stream<kEgNt, C>(xout + at, xv);
            }
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

// out[slot][k] = vals[slot][k] * colscale[cols[slot]][k]   (per-realization column scaling A(k) D(k)^-1)
template <int NB>
__global__ __launch_bounds__(kBlock) void scale_cols_bv_kernel(size_t nflat, const int* __restrict__ cols,
                                                               const double* __restrict__ vals,
                                                               const double* __restrict__ colscale,
                                                               double* __restrict__ out, int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);   // flat kernel: a wide batch is simply a wider row
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        const size_t e = i * C;
        const size_t slot = e / W;
        const int k0 = (int)(e % W);
        double v[C], sc[C];
        load_c<C>(vals + e, v);
        load_c<C>(colscale + (size_t)cols[slot] * W + k0, sc);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] *= sc[c];
        store_c<C>(out + e, v);
    }
}

// fp32 copies for the preconditioner kernels: out_scaled[slot][k] = (float)(vals[slot][k] * colscale[cols[slot]][k]),
// out_vals[slot][k] = (float)vals[slot][k]
template <int NB>
__global__ __launch_bounds__(kBlock) void scale_cols_bv32_kernel(size_t nflat, const int* __restrict__ cols,
                                                                 const double* __restrict__ vals,
                                                                 const double* __restrict__ colscale,
                                                                 float* __restrict__ out_scaled, float* __restrict__ out_vals,
                                                                 int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nflat; i += (size_t)gridDim.x * kBlock) {
        const size_t e = i * C;
        const size_t slot = e / W;
        const int k0 = (int)(e % W);
        double v[C], sc[C];
        load_c<C>(vals + e, v);
        load_c<C>(colscale + (size_t)cols[slot] * W + k0, sc);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            out_vals[e + c] = (float)v[c];
            out_scaled[e + c] = (float)(v[c] * sc[c]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Darcy per-sample numeric refresh (K12-K14), batched values: arrays are [slot][NB].
// coef[e*NB+k] = 1/k or k.
template <int NB>
__global__ __launch_bounds__(kBlock) void darcy_coef_kernel(int n, const double* __restrict__ kfield, int k_divides,
                                                            double* __restrict__ coef, int ld) {
    // kfield sample-major [nb][n] -> interleaved coefficient
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    double v[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const double t = kfield[(size_t)(c0 + k) * n + i];
        v[k] = k_divides ? 1.0 / t : t;
    }
    store_row<NB>(coef + (size_t)i * LD + c0, v);
}

// One lane per row of the SELL-stored M: raw values from element contributions, essential
// row/col elimination (DarcySolver.cpp:487-498), rhs fix-up, diagonal and l1 row sums.
template <int NB>
__global__ __launch_bounds__(kBlock) void darcy_assemble_kernel(
    int nrows, int nslices, const int* __restrict__ slice_off, const int* __restrict__ cols,
    const int* __restrict__ slot_src, const int* __restrict__ c_ptr, const int* __restrict__ c_elem,
    const double* __restrict__ c_val, const double* __restrict__ coef, const unsigned char* __restrict__ ess,
    const double* __restrict__ ess_data, const double* __restrict__ rhs0, double* __restrict__ mvals,
    double* __restrict__ diag, double* __restrict__ l1inv, double* __restrict__ rhs_bc, int ld) {
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        coef += c0; diag += c0; l1inv += c0; rhs_bc += c0;
        if (mvals) mvals += c0;
    }
    const int row = blockIdx.x * kBlock + threadIdx.x;
    const int slice = row >> 6, lane = row & 63;
    if (slice >= nslices) return;
    const int off = slice_off[slice];
    const int width = (slice_off[slice + 1] - off) >> 6;
    const bool live = row < nrows;
    const bool row_ess = live && ess[row];
    double dg[NB], l1[NB], fix[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) dg[k] = l1[k] = fix[k] = 0.0;
    int slot = off + lane;
    for (int j = 0; j < width; ++j, slot += kWave) {
        const int p = slot_src[slot];
        double v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = 0.0;
        const int c = cols[slot];
        if (p >= 0) {
            for (int t = c_ptr[p]; t < c_ptr[p + 1]; ++t) {
                const double cv = c_val[t];
                double ce[NB];
                load_row<NB>(coef + (size_t)c_elem[t] * LD, ce);
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k] = fma(ce[k], cv, v[k]);
            }
            const bool col_ess = ess[c];
            if (row_ess || col_ess) {
                if (col_ess && !row_ess) {
                    const double dval = ess_data[c];
#pragma unroll
                    for (int k = 0; k < NB; ++k) fix[k] = fma(v[k], dval, fix[k]);
                }
                const double e = (c == row) ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k] = e;
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                l1[k] += fabs(v[k]);
                if (c == row) dg[k] = v[k];
            }
        }
        if (mvals) store_row<NB>(mvals + (size_t)slot * LD, v);
    }
    if (!live) return;
    double rb[NB];
    const double r0 = row_ess ? ess_data[row] : rhs0[row];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        rb[k] = row_ess ? r0 : r0 - fix[k];
        l1[k] = 1.0 / l1[k];
    }
    store_row<NB>(diag + (size_t)row * LD, dg);
    store_row<NB>(l1inv + (size_t)row * LD, l1);
    store_row<NB>(rhs_bc + (size_t)row * LD, rb);
}

// Generic numeric refresh of a derived matrix on a fixed pattern:
//   out[slot][k] = sum_{t in ptr[slot]..ptr[slot+1]} w[t] * f(src[idx[t]][k]),  f = 1/x if recip else x
// used for S = B diag(M)^-1 B^T (recip, src = diag(M)) and for coarse S_c = 1/2 P^T S P.
// Also produces 1/diag of the derived matrix when dinv != nullptr (is_diag[slot] marks diagonal slots).
template <int NB>
__global__ __launch_bounds__(kBlock) void refresh_kernel(int64_t nslots, const int* __restrict__ ptr,
                                                         const int* __restrict__ idx, const double* __restrict__ w,
                                                         const double* __restrict__ src, int recip,
                                                         double* __restrict__ out, int ld) {
    const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= nslots) return;
    const int LD = row_ld<NB>(ld);
    src += col0<NB>();
    out += col0<NB>();
    double acc[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = 0.0;
    for (int t = ptr[slot]; t < ptr[slot + 1]; ++t) {
        double s[NB];
        load_row<NB>(src + (size_t)idx[t] * LD, s);
        const double wt = w[t];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = fma(wt, recip ? 1.0 / s[k] : s[k], acc[k]);
    }
    store_row<NB>(out + (size_t)slot * LD, acc);
}

// dinv[row][k] = 1 / vals[diag_slot[row]][k]
template <int NB>
__global__ __launch_bounds__(kBlock) void diag_inv_kernel(int n, const int* __restrict__ diag_slot,
                                                          const double* __restrict__ vals, double* __restrict__ dinv, int ld) {
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= n) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    double v[NB];
    load_row<NB>(vals + (size_t)diag_slot[row] * LD + c0, v);
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = 1.0 / v[k];
    store_row<NB>(dinv + (size_t)row * LD + c0, v);
}

// Per-realization Gershgorin bound of D^-1 S on batched values:  g[k] = max_i dinv[i][k] * sum_j |S_ij(k)|  (atomic max
// on the bit pattern of the non-negative doubles; g zeroed by the launcher), then dinv[i][k] /= 1.0001 g[k] so that the
// Chebyshev smoothers run on (0, 1] for every realization of the batch.
template <int NB>
__global__ __launch_bounds__(kBlock) void gersh_bv_kernel(int nrows, const int* __restrict__ slice_off,
                                                          const double* __restrict__ vals, const double* __restrict__ dinv,
                                                          unsigned long long* __restrict__ g, int ld) {
    const int row = blockIdx.x * kBlock + threadIdx.x;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        vals += c0; dinv += c0; g += c0;
    }
    double acc[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = 0.0;
    if (row < nrows) {
        const int slice = row >> 6, lane = row & 63;
        const int off = slice_off[slice];
        const int width = (slice_off[slice + 1] - off) >> 6;
        for (int j = 0; j < width; ++j) {
            double v[NB];
            load_row<NB>(vals + ((size_t)off + (size_t)j * 64 + lane) * LD, v);
#pragma unroll
            for (int k = 0; k < NB; ++k) acc[k] += fabs(v[k]);
        }
        double d[NB];
        load_row<NB>(dinv + (size_t)row * LD, d);
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] *= fabs(d[k]);
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        double v = acc[k];
        for (int o = kWave / 2; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
        if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(g + k, (unsigned long long)__double_as_longlong(v));
    }
}

template <int NB>
__global__ __launch_bounds__(kBlock) void gersh_scale_kernel(int nrows, const unsigned long long* __restrict__ g,
                                                             double* __restrict__ dinv, int ld) {
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nrows) return;
    const int LD = row_ld<NB>(ld), c0 = col0<NB>();
    double d[NB];
    load_row<NB>(dinv + (size_t)row * LD + c0, d);
#pragma unroll
    for (int k = 0; k < NB; ++k) d[k] /= 1.0001 * __longlong_as_double((long long)g[c0 + k]);
    store_row<NB>(dinv + (size_t)row * LD + c0, d);
}

// ==========================================================================================
// launchers
namespace k {

template <typename XT>
static int eg_pair_spmm_t(hipStream_t st, int nb, const EgView& M, const double* coef, const XT* x1, const SellView& A2,
                          const XT* x2, double* y, double* dot_partial, const XT* dot_with) {
    if (M.nrows == 0) return 0;
    if (A2.bv || A2.nrows != M.nrows || A2.nslices != M.nslices)
        throw Error(PMC_ERR_INTERNAL, "eg_pair_spmm: second operator must share the rows and carry shared values");
    // the kernels address their gathers with 32-bit element offsets (sell_row_part)
    if ((uint64_t)std::max(M.nrows, A2.ncols_hint) * (uint64_t)nb >= (1ull << 32))
        throw Error(PMC_ERR_INVALID, "eg_pair_spmm: rows x batch width exceed 32-bit gather offsets");
    const dim3 g = grid_bounded(grid_slices(M.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        const bool nt = nt_flat((size_t)M.nrows * NB * 2);   // from 4 MiB per vector on
        if (nt) count_solve_path(PMC_COUNT_NT_FLAT);
        dispatch_bool(nt, [&](auto nt_c) {
            dispatch_bool(dot_partial != nullptr, [&](auto dot) {
                constexpr bool DOT = decltype(dot)::value;
                eg_pair_spmm_kernel<NB, DOT, decltype(nt_c)::value, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(
                    M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, A2.slice_off, A2.cols, A2.vals, x1, x2, y,
                    DOT ? dot_with : nullptr, DOT ? dot_partial : nullptr, nb);
            });
        });
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int eg_pair_spmm(hipStream_t st, int nb, const EgView& M, const double* coef, const double* x1, const SellView& A2,
                 const double* x2, double* y, double* dot_partial, const double* dot_with) {
    return eg_pair_spmm_t<double>(st, nb, M, coef, x1, A2, x2, y, dot_partial, dot_with);
}
int eg_pair_spmm_z(hipStream_t st, int nb, const EgView& M, const double* coef, zvec x1, const SellView& A2,
                   zvec x2, double* y, double* dot_partial, zvec dot_with) {
    return dispatch_storage(x1, [&](auto* p1, auto* p2, auto* dw) { return eg_pair_spmm_t(st, nb, M, coef, p1, A2, p2, y, dot_partial, dw); }, x2, dot_with);
}

template <typename OT>
static int eg_poly2_t(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, OT* xout,
                      double c0, double c1, double* dot_partial) {
    if (M.nrows == 0) return 0;
    if ((uint64_t)M.nrows * (uint64_t)nb >= (1ull << 32))
        throw Error(PMC_ERR_INVALID, "eg_poly2: rows x batch width exceed 32-bit gather offsets");
    const dim3 g = grid_bounded(grid_slices(M.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        const bool nt = nt_flat((size_t)M.nrows * NB * 2);
        if (nt) count_solve_path(PMC_COUNT_NT_FLAT);
        dispatch_bool(nt, [&](auto nt_c) {
            dispatch_bool(dot_partial != nullptr, [&](auto dot) {
                constexpr bool DOT = decltype(dot)::value;
                eg_poly2_kernel<NB, DOT, decltype(nt_c)::value, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(
                    M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, dinv, r, xout, c0, c1, DOT ? dot_partial : nullptr, nb);
            });
        });
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int eg_poly2(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, double* xout,
             double c0, double c1, double* dot_partial) {
    return eg_poly2_t<double>(st, nb, M, coef, dinv, r, xout, c0, c1, dot_partial);
}
int eg_poly2_z(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, zvec xout,
               double c0, double c1, double* dot_partial) {
    return dispatch_storage(xout, [&](auto* out) { return eg_poly2_t(st, nb, M, coef, dinv, r, out, c0, c1, dot_partial); });
}

void scale_cols_bv(hipStream_t st, int nb, int64_t nslots, const int* cols, const double* vals, const double* colscale,
                   double* out) {
    if (nslots == 0) return;
    const size_t nf = (size_t)nslots * nb / lay_c(nb);
    const unsigned g = (unsigned)std::min<size_t>((nf + kBlock - 1) / kBlock, 8192);
    PMC_DISPATCH_NB(nb, { scale_cols_bv_kernel<NB><<<g, kBlock, 0, st>>>(nf, cols, vals, colscale, out, nb); });
    check_launch();
}

void scale_cols_bv32(hipStream_t st, int nb, int64_t nslots, const int* cols, const double* vals, const double* colscale,
                     float* out_scaled, float* out_vals) {
    if (nslots == 0) return;
    const size_t nf = (size_t)nslots * nb / lay_c(nb);
    const unsigned g = (unsigned)std::min<size_t>((nf + kBlock - 1) / kBlock, 8192);
    PMC_DISPATCH_NB(nb, { scale_cols_bv32_kernel<NB><<<g, kBlock, 0, st>>>(nf, cols, vals, colscale, out_scaled, out_vals, nb); });
    check_launch();
}

void darcy_coef(hipStream_t st, int nb, int n, const double* kfield, bool k_divides, double* coef) {
    PMC_DISPATCH_NB(nb, { darcy_coef_kernel<NB><<<groups(grid_rows(n), nb), kBlock, 0, st>>>(n, kfield, k_divides ? 1 : 0, coef, nb); });
    check_launch();
}

void darcy_assemble(hipStream_t st, int nb, const SellView& Mp, const int* slot_src, const int* c_ptr, const int* c_elem,
                    const double* c_val, const double* coef, const unsigned char* ess, const double* ess_data,
                    const double* rhs0, double* mvals, double* diag, double* l1inv, double* rhs_bc) {
    const dim3 g = grid_rows(Mp.nslices * kWave);
    PMC_DISPATCH_NB(nb, {
        darcy_assemble_kernel<NB><<<groups(g, nb), kBlock, 0, st>>>(Mp.nrows, Mp.nslices, Mp.slice_off, Mp.cols, slot_src, c_ptr,
                                                                   c_elem, c_val, coef, ess, ess_data, rhs0, mvals, diag, l1inv,
                                                                   rhs_bc, nb);
    });
    check_launch();
}

void gersh_scale_bv(hipStream_t st, int nb, const SellView& S, double* dinv, double* gwork) {
    unsigned long long* g = reinterpret_cast<unsigned long long*>(gwork);
    PMC_HIP(hipMemsetAsync(g, 0, sizeof(unsigned long long) * kMaxBatch, st));
    const int grid = (S.nrows + kBlock - 1) / kBlock;
    PMC_DISPATCH_NB(nb, {
        gersh_bv_kernel<NB><<<groups(grid, nb), kBlock, 0, st>>>(S.nrows, S.slice_off, S.vals, dinv, g, nb);
        gersh_scale_kernel<NB><<<groups(grid, nb), kBlock, 0, st>>>(S.nrows, g, dinv, nb);
    });
    check_launch(2);
}

void refresh(hipStream_t st, int nb, int64_t nslots, const int* ptr, const int* idx, const double* w, const double* src,
             bool recip, double* out) {
    if (nslots == 0) return;
    const dim3 g((unsigned)((nslots + kBlock - 1) / kBlock));
    PMC_DISPATCH_NB(nb, { refresh_kernel<NB><<<groups(g, nb), kBlock, 0, st>>>(nslots, ptr, idx, w, src, recip ? 1 : 0, out, nb); });
    check_launch();
}

void diag_inv(hipStream_t st, int nb, int n, const int* diag_slot, const double* vals, double* dinv) {
    PMC_DISPATCH_NB(nb, { diag_inv_kernel<NB><<<groups(grid_rows(n), nb), kBlock, 0, st>>>(n, diag_slot, vals, dinv, nb); });
    check_launch();
}

// Back-substitution of the hybridized Darcy system (DarcyHybrid): interleaved [row][nb] vectors, one thread per entry.
//   flux:     out[f][k] = kappa[owner[f]][k] * (U0[f] - t[f][k]) + ug[f]          t = U_L lambda
//   pressure: out[e][k] = P0[e] - t[e][k] - zg[e] / kappa[e][k]                  t = P_L lambda
__global__ __launch_bounds__(kBlock) void darcy_backsub_u_kernel(size_t total, int nb, const int* __restrict__ owner,
                                                                  const double* __restrict__ kappa, const double* __restrict__ U0,
                                                                  const double* __restrict__ ug, const double* __restrict__ t,
                                                                  double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / (size_t)nb;
    const int k = (int)(i % (size_t)nb);
    out[i] = kappa[(size_t)owner[f] * nb + k] * (U0[f] - t[i]) + ug[f];
}
__global__ __launch_bounds__(kBlock) void darcy_backsub_p_kernel(size_t total, int nb, const double* __restrict__ kappa,
                                                                  const double* __restrict__ P0, const double* __restrict__ zg,
                                                                  const double* __restrict__ t, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t e = i / (size_t)nb;
    out[i] = P0[e] - t[i] - zg[e] / kappa[i];
}

void darcy_backsub_u(hipStream_t st, int nb, int n_u, const int* owner, const double* kappa, const double* U0, const double* ug,
                     const double* t, double* out) {
    const size_t total = (size_t)n_u * nb;
    if (total == 0) return;
    darcy_backsub_u_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, st>>>(total, nb, owner, kappa, U0, ug, t, out);
    check_launch();
}
void darcy_backsub_p(hipStream_t st, int nb, int n_p, const double* kappa, const double* P0, const double* zg, const double* t,
                     double* out) {
    const size_t total = (size_t)n_p * nb;
    if (total == 0) return;
    darcy_backsub_p_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, st>>>(total, nb, kappa, P0, zg, t, out);
    check_launch();
}

}  // namespace k
}  // namespace pmc

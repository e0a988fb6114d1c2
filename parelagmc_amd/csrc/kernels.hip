// CDNA4 (gfx950) kernels of the ParELAGMC hot path.  fp64 values, int32 indices, HBM-bound:
// no MFMA (<= 0.17 flop/byte), 64-wide wavefronts, SELL-64 operators so that every matrix load
// of a wavefront is one contiguous 512 B (values) / 256 B (columns) segment.
//
// Kernel <-> reference operation:
//   sell_spmm / sell_residual / sell_cheb_step : K5 block saddle-point SpMV, K7 smoother on M,
//        K8 V-cycle smoothing/residual/transfer, K3/K4 restriction/prolongation, K11 projection
//   minres_* / lincomb3 / dot                  : K6 MINRES vector operations
//   normal_fill                                : K1 NormalDistributionSampler
//   interleave / deinterleave                  : K2 white-noise RHS scaling, K9 exp, K10 gather (fused with the layout change)
//   darcy_*                                    : K12-K15 per-sample M(k), BC elimination, Schur refresh, QoI
#include "sell_rows.hpp"

#include <cstddef>
#include <cstdlib>

#include <algorithm>
#include <atomic>

namespace pmc {

static unsigned dot_grid_bound();
int dot_capacity(int nrows, int nb) {
    // upper bound on the partial blocks (of nb doubles each) any fused dot over nrows rows of a batch of nb writes: slice
    // kernels one block per 4 slices, flat kernels one per kBlock threads, both bounded by dot_grid_bound() - except the
    // block operator's two-stage reduction, which keeps every slice block behind kCompressBlocks compressed ones (k::spmm)
    const size_t slice_blocks = ((size_t)nrows + 63) / 64 / (kBlock / kWave) + 1;
    const size_t flat_blocks = ((size_t)nrows * nb / (nb >= 32 ? 4 : (nb >= 2 ? 2 : 1)) + kBlock - 1) / kBlock;
    const size_t bounded = std::min<size_t>(std::max(slice_blocks, flat_blocks), dot_grid_bound());
    return (int)std::max<size_t>(bounded, 256 + slice_blocks) + 2;
}

template <int NB, int BV, typename XT = double>
__device__ __forceinline__ void sell_row_product(const int* __restrict__ slice_off, const int* __restrict__ cols,
                                                 const double* __restrict__ vals, const XT* __restrict__ x,
                                                 int slice, int lane, int LD, double (&acc)[Lay<NB>::T][Lay<NB>::C]) {
    const int off = slice_off[slice];
    const int width = (slice_off[slice + 1] - off) >> 6;
    sell_row_range<NB, BV, false, true, false, XT>(cols, vals, x, nullptr, off, width, lane, LD, acc);
}

// MODE 0: y = Ax   1: y += Ax   2: y = r - Ax ; DOT: partial sums of <dot_with, result>.
// Wavefronts stride over the slices (grid may be smaller than the slice count: bounded partial-sum count).
// TAG only names the instantiation: 1 = the block saddle-point operator (K5) inside the solver, 2 = the same operator
// launched by pmc_sampler_apply_operator (the isolated roofline measurement), so that profiles show the
// hot operator's launches on their own row; 0 = every other matrix (transfers, residuals, ...).
// R8 (with MODE 2, no DOT): the rows of the result are also summed in groups of 8 consecutive rows into
// partial[(row / 8) * NB + k] - the restriction P^T res of a prolongator whose parent i has exactly the children
// 8 i .. 8 i + 7 with unit weights (uniformly refined tetrahedra / hexahedra): a slice holds 8 whole groups, the sum is
// a fixed xor tree over the lanes of a row step, and the separate restriction kernel (13 us of dependent latency for a
// few MB) disappears from the V-cycle.
// XT: storage type of x and dot_with (fp32 or fp64 for the preconditioned Krylov vectors, zvec)
// YT: storage type of y (fp32: the coarse right-hand side of a V-cycle level with fp32 inter-level vectors, plain products only)
// LZ: the two operator passes of a MINRES iteration that never stores q = A u (shared values, MODE 0; k::LanczosUpdate):
//   1 = the product is not stored, only the fused dot leaves the kernel (alpha = <u, Au>: the same partials, bit for bit,
//       as the storing form);
//   2 = no dot; the epilogue forms the next Lanczos vector from the row sums (the same bits as the stored q) and the own
//       rows of v1 (lz.v1) and v0 (y): y = c0 (A x) + c1 v1 + c2 y, written over v0 together with its fp32 copy lz.y32;
//   3 = as 2 in the first iteration, where v0 is zero: y is not read (the c2 term is kept with a literal +0.0, so even the
//       sign of a zero result is that of the flat kernel);
//   4 = a plain product that also leaves the fp32 copy of its result in lz.y32 (k::spmm_store32: the right-hand side a MINRES
//       solve adopts as its first Lanczos vector - what k::copy_r32 made of the stored product, from the registers)
// SM (MODE 2, shared values): the result leaves the kernel sample-major, y[k * nrows + row], as k::deinterleave would write it
//   from the interleaved one (k::residual_samples); 2 = through exp().  Each value is computed as in the interleaved form and
//   stored once; a wavefront writes, per column, the 64 rows of its slice in T runs of G consecutive rows.
template <int NB, int BV, int MODE, bool DOT, int TAG, bool NT = false, bool R8 = false, bool DL = false, typename XT = double,
          typename YT = double, int LZ = 0, int SM = 0>
__global__ __launch_bounds__(kBlock, (NB >= 32 && BV == 0 && sizeof(XT) == 4 ? 3 : 1)) void sell_spmm_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
                                                           const int* __restrict__ sched,
                                                           const int* __restrict__ cols,
                                                           const double* __restrict__ vals,
                                                           const XT* __restrict__ x, typename ident<YT>::type* __restrict__ y,
                                                           const double* __restrict__ r,
                                                           const typename ident<XT>::type* __restrict__ dot_with,
                                                           double* __restrict__ partial, int ld,
                                                           k::LanczosUpdate lz = k::LanczosUpdate{}) {
    static_assert(!R8 || (MODE == 2 && !DOT), "fused restriction goes with the residual");
    static_assert(LZ == 0 || (BV == 0 && MODE == 0 && !R8 && sizeof(YT) == 8 && DOT == (LZ == 1)),
                  "Lanczos passes: shared values, plain product; the dot-only pass has the dot, the update passes none");
    static_assert(sizeof(YT) == 8 || (MODE == 0 && !DOT && !NT), "fp32 result: plain products only");
    static_assert(SM == 0 || (MODE == 2 && BV == 0 && !DOT && !R8 && LZ == 0 && sizeof(YT) == 8),
                  "sample-major result: the plain residual of a shared-value matrix");
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();   // this group's columns of every interleaved operand
        x += c0;
        if constexpr (SM) y += (size_t)c0 * nrows;   // column k of the result starts at k * nrows
        else if constexpr (LZ != 1) y += c0;         // (the dot-only pass has no y)
        if constexpr (BV) vals = shift_bv<BV>(vals, c0);
        if constexpr (MODE == 2) r += c0;
        if constexpr (DOT && !DL) dot_with += c0;
        if constexpr (DOT || R8) partial += c0;
        if constexpr (LZ == 2 || LZ == 3) {
            lz.v1 += c0;
            lz.c0 += c0; lz.c1 += c0; lz.c2 += c0;
        }
        if constexpr (LZ >= 2) lz.y32 += c0;
    }
    static_assert(!DL || (DOT && !BV && Lay<NB>::T > 1), "diagonal-last serves the fused <x, Ax> of shared-value operators");
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    const SliceWalk sw = slice_walk(nslices);
    for (int si = sw.begin; si < sw.end; si += sw.stride) {
        const int slice = sched ? sched[si] : si;   // optional processing order (locality), see Sell::sched
        double acc[T][C];
        constexpr bool LEAN_DL = DL && lean_range<NB>();   // the dot is taken inside the gather loop
        double xd[DL && !LEAN_DL ? T : 1][C];
        if constexpr (LEAN_DL) {
            const int off = slice_off[slice];
            sell_row_range<NB, false, false, true, NT, XT>(cols, vals, x, nullptr, off, (slice_off[slice + 1] - off) >> 6,
                                                             lane, LD, acc, nullptr, p);
        } else if constexpr (DL) {
            const int off = slice_off[slice];
            sell_row_range<NB, false, false, true, NT, XT>(cols, vals, x, nullptr, off, (slice_off[slice + 1] - off) >> 6,
                                                             lane, LD, acc, xd);
        } else if constexpr (NT) {
            const int off = slice_off[slice];
            sell_row_range<NB, BV, false, true, true, XT>(cols, vals, x, nullptr, off, (slice_off[slice + 1] - off) >> 6, lane, LD, acc);
        } else {
            sell_row_product<NB, BV, XT>(slice_off, cols, vals, x, slice, lane, LD, acc);
        }
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int row = slice * kWave + rs * G + g;
            if (row < nrows) {
                const size_t at = (size_t)row * LD + t * C;
                if constexpr (MODE == 1) {
                    double old[C];
                    load_c<C>(y + at, old);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[rs][c] += old[c];
                } else if constexpr (MODE == 2) {
                    double rv[C];
                    load_c<C>(r + at, rv);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[rs][c] = rv[c] - acc[rs][c];
                }
                if constexpr (LZ == 4) {
                    store_c<C>(y + at, acc[rs]);
                    store_v<C>(lz.y32 + at, acc[rs]);
                } else if constexpr (SM) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        double tv = acc[rs][c];
                        if constexpr (SM == 2) tv = exp(tv);
                        y[(size_t)(t * C + c) * nrows + row] = tv;
                    }
                } else if constexpr (LZ >= 2) {
                    double bv[C], yv[C];
                    load_c_nt<NT, C>(lz.v1 + at, bv);
                    if constexpr (LZ == 2) {
                        load_c_nt<NT, C>(y + at, yv);
                    } else {
#pragma unroll
                        for (int c = 0; c < C; ++c) yv[c] = 0.0;
                    }
                    lanczos_combine<C>(lz.c0, lz.c1, lz.c2, t * C, acc[rs], bv, yv);
                    store_c<C>(y + at, yv);          // gathered by the next kernels
                    store_v<C>(lz.y32 + at, yv);
                } else if constexpr (LZ == 1) {      // the product only feeds the dot
                } else if constexpr (sizeof(YT) == 8) store_c_stream<NT, C>(y + at, acc[rs]);
                else store_v<C>(y + at, acc[rs]);
                if constexpr (LEAN_DL) {
                } else if constexpr (DL) {
#pragma unroll
                    for (int c = 0; c < C; ++c) p[c] = fma(xd[rs][c], acc[rs][c], p[c]);
                } else if constexpr (DOT) {
                    double w[C];
                    load_v<C>(dot_with + at, w);
#pragma unroll
                    for (int c = 0; c < C; ++c) p[c] = fma(w[c], acc[rs][c], p[c]);
                }
            } else if constexpr (R8) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[rs][c] = 0.0;     // rows past the end add nothing to their group
            }
            if constexpr (R8) {
                // lanes (g, t): the 8 rows of a group differ in the low three bits of g = lane / T
                double s[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    double v = acc[rs][c];
                    v += __shfl_xor(v, T, kWave);
                    v += __shfl_xor(v, 2 * T, kWave);
                    v += __shfl_xor(v, 4 * T, kWave);
                    s[c] = v;
                }
                if ((g & 7) == 0 && row < nrows) store_c<C>(partial + (size_t)(row >> 3) * LD + t * C, s);
            }
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

// Chebyshev / Jacobi step: d = a d + b dinv (r - A xin); xout = xin + d ; DOT: partials of <r, xout>
// OT != double: the LAST step of a polynomial whose result is a preconditioned Krylov vector (zvec storage): d is not
// written back, the iterate is rounded to its storage before the fused dot
template <int NB, int BV, bool DOT, typename OT = double>
__global__ __launch_bounds__(kBlock) void sell_cheb_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
                                                           const int* __restrict__ sched,
                                                           const int* __restrict__ cols,
                                                           const double* __restrict__ vals,
                                                           const double* __restrict__ dinv,
                                                           const double* __restrict__ r,
                                                           const double* __restrict__ xin, double* __restrict__ d,
                                                           OT* __restrict__ xout, double a, double b,
                                                           double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        r += c0; xin += c0; d += c0; xout += c0;
        if constexpr (BV) { vals = shift_bv<BV>(vals, c0); dinv += c0; }
        if constexpr (DOT) partial += c0;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    const SliceWalk sw = slice_walk(nslices);
    for (int si = sw.begin; si < sw.end; si += sw.stride) {
        const int slice = sched ? sched[si] : si;
        double acc[T][C];
        sell_row_product<NB, BV>(slice_off, cols, vals, xin, slice, lane, LD, acc);
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int row = slice * kWave + rs * G + g;
            if (row >= nrows) continue;
            const size_t at = (size_t)row * LD + t * C;
            double rv[C], dv[C], xv[C], di[C];
            load_c<C>(r + at, rv);
            load_c<C>(xin + at, xv);
            if (a != 0.0) {
                load_c<C>(d + at, dv);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) dv[c] = 0.0;
            }
            if constexpr (BV) {
                load_c<C>(dinv + at, di);
            } else {
                const double s = dinv[row];
#pragma unroll
                for (int c = 0; c < C; ++c) di[c] = s;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                dv[c] = a * dv[c] + b * di[c] * (rv[c] - acc[rs][c]);
                xv[c] += dv[c];
            }
            round_to<OT>(xv);
            if constexpr (DOT) {
#pragma unroll
                for (int c = 0; c < C; ++c) p[c] = fma(rv[c], xv[c], p[c]);
            }
            if constexpr (std::is_same<OT, double>::value) store_c<C>(d + at, dv);
            store_v<C>(xout + at, xv);
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

// Degree-2 Chebyshev polynomial from a ZERO initial guess in ONE pass.  With t = D^-1 r the two steps
//   x1 = t/theta ;  x2 = x1 + rho1 rho0 x1 + (2 rho1/delta) D^-1 (r - A x1)
// collapse to  x2_i = dinv_i (c0 r_i - c1 (A D^-1 r)_i),  so with the column-scaled values As = A D^-1
// (precomputed at create time) a single SpMM over r gives the result: 1 gather pass instead of the
// 3 + 5 vector passes of cheb_first + cheb_step.  DOT: partials of <r, x2>.
// From a NONZERO guess x0 the same polynomial acts on the residual: x2 = x0 + p2(r - A x0); then r is that residual,
// xadd = x0 (may alias xout: no gathers on it) and the dot is taken with dot_with (the right-hand side).
template <int NB, int BV, bool DOT, bool NT = false, typename OT = double>
__global__ __launch_bounds__(kBlock, (NB >= 32 && BV == 0 ? 3 : 1)) void sell_poly2_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
                                                            const int* __restrict__ sched,
                                                            const int* __restrict__ cols,
                                                            const double* __restrict__ vals_scaled,
                                                            const double* __restrict__ dinv,
                                                            const double* __restrict__ r, OT* xout,
                                                            double c0, double c1, double* __restrict__ partial,
                                                            const double* xadd, const double* __restrict__ dot_with,
                                                            const int* __restrict__ padd_idx,
                                                            const double* __restrict__ padd_x, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        r += c0; xout += c0;
        if constexpr (BV) { vals_scaled = shift_bv<BV>(vals_scaled, c0); dinv += c0; }
        if (xadd) xadd += c0;
        if (dot_with) dot_with += c0;
        if (padd_x) padd_x += c0;
        if constexpr (DOT) partial += c0;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    const SliceWalk sw = slice_walk(nslices);
    for (int si = sw.begin; si < sw.end; si += sw.stride) {
        const int slice = sched ? sched[si] : si;
        double acc[T][C];
        if constexpr (NT) {
            const int off = slice_off[slice];
            sell_row_range<NB, BV, false, true, true>(cols, vals_scaled, r, nullptr, off, (slice_off[slice + 1] - off) >> 6,
                                                        lane, LD, acc);
        } else {
            sell_row_product<NB, BV>(slice_off, cols, vals_scaled, r, slice, lane, LD, acc);
        }
        // own-row reads in batches of H row steps (shared values only: the per-realization instantiations have no registers
        // to spare); rows past the end re-read the last row and store nothing
        constexpr int H = (BV == 0 && T >= 4) ? 2 : 1;   // (4 spills in the fp64-output instantiations: 168 registers are the cap)
        double rvb[H][C], dib[H];
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int row = slice * kWave + rs * G + g;
            if constexpr (H > 1) {
                if (rs % H == 0) {
#pragma unroll
                    for (int u = 0; u < H; ++u) {
                        const int rc = min(row + u * G, nrows - 1);
                        load_c<C>(r + (size_t)rc * LD + t * C, rvb[u]);
                        dib[u] = dinv[rc];
                    }
                    pin_block(rvb);
                }
            }
            if (row >= nrows) continue;
            const size_t at = (size_t)row * LD + t * C;
            double rv[C], xv[C], di[C];
            if constexpr (H > 1) {
#pragma unroll
                for (int c = 0; c < C; ++c) { rv[c] = rvb[rs % H][c]; di[c] = dib[rs % H]; }
            } else {
                load_c<C>(r + at, rv);
                if constexpr (BV) {
                    load_c<C>(dinv + at, di);
                } else {
                    const double s = dinv[row];
#pragma unroll
                    for (int c = 0; c < C; ++c) di[c] = s;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) xv[c] = di[c] * (c0 * rv[c] - c1 * acc[rs][c]);
            if (xadd) {
                double x0[C];
                load_c<C>(xadd + at, x0);
#pragma unroll
                for (int c = 0; c < C; ++c) xv[c] += x0[c];
            }
            if (padd_idx) {   // + (P xc)_row for an injection-type prolongator: xc[parent[row]]
                double pc[C];
                load_c<C>(padd_x + (size_t)padd_idx[row] * LD + t * C, pc);
#pragma unroll
                for (int c = 0; c < C; ++c) xv[c] += pc[c];
            }
            round_to<OT>(xv);
            if constexpr (DOT) {
                if (dot_with) load_c<C>(dot_with + at, rv);
#pragma unroll
                for (int c = 0; c < C; ++c) p[c] = fma(rv[c], xv[c], p[c]);
            }
            store_v_stream<NT, C>(xout + at, xv);
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

// ------------------------------------------------------------------------------------------
// V-cycle kernels with fp32 INTERMEDIATES (shared-value hierarchies: the sampler).  The vectors that live only inside one
// application of the preconditioner - the pre-smoothed iterate and the residuals of a level - are stored in fp32; the
// preconditioner's input and output, every coarse right-hand side / correction and all arithmetic stay fp64.  A
// preconditioner whose result carries fp32-sized rounding does not limit what MINRES attains: its search directions are
// the preconditioned vectors themselves, q = A z is formed from the z actually delivered, so the residual recurrence stays
// consistent - measured (z rounded to fp32 after every application, cube_tet r = 4): identical iteration counts at 1e-6 ...
// 1e-12 and fields equal to the unrounded run's to 7e-16.  What it saves is 87 MB of the 1 089 MB an iteration moves at r = 5.

// out = dinv (c0 r - c1 As r) (+ xadd) (+ padd_x[padd_idx]) with r of type XT (gathered and read at the own row), out of
// type OT, xadd of type AT; DOT: partials of <dot_with, out> (dot_with fp64).  See sell_poly2_kernel.
#ifndef PMC_VC_MIN_WAVES
#define PMC_VC_MIN_WAVES 3   // post-smoothing of the 400 k-row multiplier level: 172 -> 168 registers, 83.6 -> 79.7 us (LAB_NOTES 10.3)
#endif
#ifndef PMC_VC_MIN_WAVES_D
#define PMC_VC_MIN_WAVES_D 1
#endif
// wavefronts per SIMD the fp32-gather V-cycle kernels of the 32-wide layout are compiled for (laboratory macro)
template <int NB, typename XT, int BV, int DEEP>
constexpr int vc_min_waves() {
    return (NB >= 32 && BV == 0 && DEEP == 1) ? (sizeof(XT) == 4 ? PMC_VC_MIN_WAVES : PMC_VC_MIN_WAVES_D) : 1;
}
// SPL (launches of at most 8 realizations on the small levels of an aggregation hierarchy, whose rows hold 20-40 entries): the
// matrix stores every row as 2^sl consecutive pieces (csr_split_rows), nrows counts the ROWS; the pieces of a row sit in
// neighbouring lane groups and are added with a shuffle tree, the first piece's lanes finish the row.  A 5 k-row level then
// runs 2^sl times the wavefronts over slices 2^sl times shorter - these launches are one chain of dependent gathers per slice.
template <int NB, int C, int T>
__device__ __forceinline__ void split_row_sums(double (&acc)[T][C], int sl) {
#pragma unroll
    for (int rs = 0; rs < T; ++rs)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double v = acc[rs][c];
            for (int o = 0; o < sl; ++o) v += __shfl_xor(v, T << o, kWave);
            acc[rs][c] = v;
        }
}
// GIB (launches of 64 realizations = two column groups): ONE workgroup sweeps a slice for both groups back to back - the slice's
// (index, value) pairs come from L1 / L2 the second time instead of being fetched again by another workgroup at another time
// (what `traffic` showed as 1.34 x the algorithmic bytes) - gridDim.y is 1 and the partial sums keep their layout.
// PT: storage type of padd_x (the coarse correction: fp64, or fp32 with fp32 inter-level vectors), widened on load
template <int NB, typename XT, typename OT, typename AT, bool DOT, bool NT = false, int BV = 0, int DEEP = 1, bool SPL = false,
          bool GIB = false, typename PT = double>
__global__ __launch_bounds__(kBlock, (vc_min_waves<NB, XT, BV, DEEP>())) void vc_poly2_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
                                                          const int* __restrict__ cols, const double* __restrict__ vals_scaled,
                                                          const double* __restrict__ dinv, const XT* __restrict__ r, OT* xout,
                                                          double c0, double c1, double* __restrict__ partial, const AT* xadd,
                                                          const double* __restrict__ dot_with,
                                                          const int* __restrict__ padd_idx,
                                                          const typename ident<PT>::type* __restrict__ padd_x,
                                                          int ld, int sl = 0) {
    static_assert(!SPL || (NB <= 8 && BV == 0 && DEEP == 1), "row-split instantiations: narrow launches, shared values");
    static_assert(!GIB || (NB == kGroup && BV == 0 && DEEP == 1 && !SPL), "both column groups in one workgroup: 64 wide, shared values");
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    constexpr int NG = GIB ? 2 : 1;
    const int LD = row_ld<NB>(ld);
    if constexpr (!GIB) {
        const int g0 = col0<NB>();
        r += g0; xout += g0;
        if constexpr (BV != 0) { vals_scaled = shift_bv<BV>(vals_scaled, g0); dinv += g0; }
        if (xadd) xadd += g0;
        if (dot_with) dot_with += g0;
        if (padd_x) padd_x += g0;
        if constexpr (DOT) partial += g0;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    const SliceWalk sw = slice_walk(nslices);
    // (the group loop is the OUTER one and not unrolled: inside the slice loop the two groups' gathers interleave and 84-188
    // registers spill; a workgroup walks one or two slices per wavefront, so the second sweep still finds them in L1 / L2)
#pragma unroll 1
    for (int grp = 0; grp < NG; ++grp) {
      const int go = grp * NB;                         // 0 unless GIB
      const XT* rg = r + go;
      OT* xg = xout + go;
      const AT* xa = xadd ? xadd + go : nullptr;
      const double* dw = dot_with ? dot_with + go : nullptr;
      const PT* px = padd_x ? padd_x + go : nullptr;
      double p[C];
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = 0.0;
      for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        double acc[T][C];
        const int off = slice_off[slice];
        sell_row_range_t<NB, XT, NT, BV, DEEP>(cols, vals_scaled, rg, off, (slice_off[slice + 1] - off) >> 6, lane, LD, acc);
        if constexpr (SPL) split_row_sums<NB, C, T>(acc, sl);
        // row steps in pairs: the own-row reads of both (and the parent indices of the coarse correction) are issued before
        // either is consumed - rows past the end re-read the last row and store nothing
        // (pairs only where the gathers above leave the registers for it - the fp32-gather instantiations; the fp64-gather
        // ones, with sixteen 16-byte gathers in flight, would drop from three to two waves per SIMD)
        constexpr int H = (T >= 2 && sizeof(XT) == 4) ? 2 : 1;
#pragma unroll
        for (int h0 = 0; h0 < T; h0 += H) {
            double rv[H][C], di[H][C], x0[H][C], pc[H][C], wv[H][C];
            size_t at[H];
            int par[H];
            bool ok[H];
#pragma unroll
            for (int u = 0; u < H; ++u) {
                const int piece = slice * kWave + (h0 + u) * G + g;
                const int row = SPL ? piece >> sl : piece;
                ok[u] = row < nrows && (!SPL || (piece & ((1 << sl) - 1)) == 0);
                const int rowc = row < nrows ? row : nrows - 1;
                at[u] = (size_t)rowc * LD + t * C;
                load_v<C>(rg + at[u], rv[u]);
                if constexpr (BV != 0) {
                    load_c<C>(dinv + at[u], di[u]);
                } else {
                    const double sdi = dinv[rowc];
#pragma unroll
                    for (int c = 0; c < C; ++c) di[u][c] = sdi;
                }
                if (xa) load_v<C>(xa + at[u], x0[u]);
                if (padd_idx) par[u] = padd_idx[rowc];
                if constexpr (DOT) load_c<C>(dw + at[u], wv[u]);
            }
            if (padd_idx) {
#pragma unroll
                for (int u = 0; u < H; ++u) load_v<C>(px + (size_t)par[u] * LD + t * C, pc[u]);
            }
#pragma unroll
            for (int u = 0; u < H; ++u) {
                double xv[C];
#pragma unroll
                for (int c = 0; c < C; ++c) xv[c] = di[u][c] * (c0 * rv[u][c] - c1 * acc[h0 + u][c]);
                if (xa) {
#pragma unroll
                    for (int c = 0; c < C; ++c) xv[c] += x0[u][c];
                }
                if (padd_idx) {
#pragma unroll
                    for (int c = 0; c < C; ++c) xv[c] += pc[u][c];
                }
                round_to<OT>(xv);
                if (ok[u]) {
                    if constexpr (DOT) {
#pragma unroll
                        for (int c = 0; c < C; ++c) p[c] = fma(wv[u][c], xv[c], p[c]);
                    }
                    store_v_stream<NT, C>(xg + at[u], xv);
                }
            }
        }
      }
      if constexpr (DOT) {
          reduce_cols_store<NB>(p, partial + go, LD);
          if (grp + 1 < NG) __syncthreads();            // the reduction's LDS scratch is reused by the next group
      }
    }
}

// y = r - A x with x of type XT (gathered), r of type RT, y of type YT; R8: rows also summed in groups of 8 into `coarse`
// (fp64), see sell_spmm_kernel
// BV: 0 shared fp64 values, 2 per-realization fp32 values; STORE = false: only the restricted sums are wanted (y unused)
// RAGG (aggregation levels renumbered by agg_pack_rows: every aggregate a run of consecutive rows inside one slice): the
// wavefront keeps its 64 x NB residual tile - the fp32 values it has just stored - in LDS and sums its own aggregates from it
// in increasing row order: coarse[cid] = sum of the rows of segment (cid, first row, rows).  No other wavefront touches those
// coarse rows: deterministic, no atomics, and the separate product with P^T (one more pass over the residual) is gone.
// SPL: rows stored in 2^sl pieces, see vc_poly2_kernel
// CT: storage type of `coarse` (fp64, or fp32 with fp32 inter-level vectors: the fp64 sums are rounded once, on store)
// TAG only names the instantiation: 1 = res - (S P) xc (in place), so that profiles show that pass on a row of its own
template <int NB, typename XT, typename RT, typename YT, bool R8, int BV = 0, bool STORE = true, int DEEP = 1, bool RAGG = false,
          bool SPL = false, typename CT = double, int TAG = 0>
__global__ __launch_bounds__(kBlock) void vc_residual_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
                                                             const int* __restrict__ cols, const double* __restrict__ vals,
                                                             const XT* __restrict__ x, const RT* r, YT* y,
                                                             typename ident<CT>::type* __restrict__ coarse, int ld,
                                                             const int* __restrict__ seg_ptr = nullptr,
                                                             const int* __restrict__ seg_cid = nullptr,
                                                             const int* __restrict__ seg_pos = nullptr, int sl = 0) {
    static_assert(!SPL || (NB <= 8 && BV == 0 && DEEP == 1 && !R8 && !RAGG && STORE), "row-split instantiations: narrow launches, plain residual");
    static_assert(STORE || R8, "a residual that is neither stored nor restricted");
    static_assert(!RAGG || (!R8 && STORE && BV == 0 && sizeof(YT) == 4), "fused aggregate restriction: shared values, fp32 residual");
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int g0 = col0<NB>();
        x += g0; r += g0;
        if constexpr (STORE) y += g0;
        if constexpr (BV != 0) vals = shift_bv<BV>(vals, g0);
        if constexpr (R8 || RAGG) coarse += g0;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    __shared__ float tile_all[RAGG ? (kBlock / kWave) * kWave * NB : 1];
    float* tile = tile_all + (RAGG ? (threadIdx.x / kWave) * kWave * NB : 0);
    const SliceWalk sw = slice_walk(nslices);
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        double acc[T][C];
        const int off = slice_off[slice];
        sell_row_range_t<NB, XT, false, BV, DEEP>(cols, vals, x, off, (slice_off[slice + 1] - off) >> 6, lane, LD, acc);
        if constexpr (SPL) split_row_sums<NB, C, T>(acc, sl);
        // the own-row reads of H row steps are issued together (rows past the end re-read the last row): one latency per
        // batch instead of one per row step - these launches are single occupancy rounds of dependent loads
        constexpr int H = T >= 4 ? 4 : T;
        double rvb[H][C];
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int piece = slice * kWave + rs * G + g;
            const int row = SPL ? piece >> sl : piece;
            if (rs % H == 0) {
#pragma unroll
                for (int u = 0; u < H; ++u) {
                    const int ru = SPL ? (piece + u * G) >> sl : row + u * G;
                    load_v<C>(r + (size_t)(ru < nrows ? ru : nrows - 1) * LD + t * C, rvb[u]);
                }
            }
            if (row < nrows && (!SPL || (piece & ((1 << sl) - 1)) == 0)) {
                const size_t at = (size_t)row * LD + t * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[rs][c] = rvb[rs % H][c] - acc[rs][c];
                if constexpr (STORE) store_v<C>(y + at, acc[rs]);
                if constexpr (RAGG) {
#pragma unroll
                    for (int c = 0; c < C; ++c) tile[(rs * G + g) * NB + t * C + c] = (float)acc[rs][c];
                }
            } else if constexpr (R8) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[rs][c] = 0.0;
            }
            if constexpr (R8) {
                double s[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    double v = acc[rs][c];
                    v += __shfl_xor(v, T, kWave);
                    v += __shfl_xor(v, 2 * T, kWave);
                    v += __shfl_xor(v, 4 * T, kWave);
                    s[c] = v;
                }
                if ((g & 7) == 0 && row < nrows) store_v<C>(coarse + (size_t)(row >> 3) * LD + t * C, s);
            }
        }
        if constexpr (RAGG) {
            // the tile is private to this wavefront: its own LDS writes are complete once the wait below has passed
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int s0 = seg_ptr[slice], s1 = seg_ptr[slice + 1];
            for (int sg = s0 + g; sg < s1; sg += G) {
                const int pos = seg_pos[sg], first = pos >> 8, len = pos & 255;
                double sum[C];
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] = 0.0;
                for (int q = 0; q < len; ++q)
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[c] += (double)tile[(first + q) * NB + t * C + c];
                store_v<C>(coarse + (size_t)seg_cid[sg] * LD + t * C, sum);
            }
            __builtin_amdgcn_wave_barrier();    // the next slice overwrites the tile
        }
    }
}

// x (fp32) += xc[row >> 3] (fp64): the coarse correction of a prolongator over groups of 8 consecutive rows
template <int NB>
__global__ __launch_bounds__(kBlock) void vc_prolong8_kernel(size_t nflat, float* __restrict__ x, const double* __restrict__ xc,
                                                             int ld) {
    constexpr int C = Lay<NB>::C;
    const int W = row_ld<NB>(ld);
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nflat) return;
    const size_t e = i * C;
    const size_t row = e / W;
    const int k0 = (int)(e % W);
    double xv[C], cv[C];
    load_cf<C>(x + e, xv);
    load_c<C>(xc + (row >> 3) * W + k0, cv);
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] += cv[c];
    store_v<C>(x + e, xv);
}

// y = A1 x1 + A2 x2 over the SAME rows: A1 with per-realization values, A2 with shared values (the u-rows
// [M(k) | B^T] of the Darcy operator in one pass); DOT: partials of <dot_with, y>.
template <int NB, bool DOT, typename XT = double>
__global__ __launch_bounds__(kBlock) void sell_pair_spmm_kernel(
    int nrows, int nslices, const int* __restrict__ off1, const int* __restrict__ cols1, const double* __restrict__ vals1,
    const int* __restrict__ off2, const int* __restrict__ cols2, const double* __restrict__ vals2,
    const XT* __restrict__ x1, const typename ident<XT>::type* __restrict__ x2, double* __restrict__ y,
    const typename ident<XT>::type* __restrict__ dot_with, double* __restrict__ partial, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        vals1 += c0; x1 += c0; x2 += c0; y += c0;
        if constexpr (DOT) { dot_with += c0; partial += c0; }
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    double p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = 0.0;
    const SliceWalk sw = slice_walk(nslices);
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        double acc[T][C], acc2[T][C];
        sell_row_product<NB, true, XT>(off1, cols1, vals1, x1, slice, lane, LD, acc);
        sell_row_product<NB, false, XT>(off2, cols2, vals2, x2, slice, lane, LD, acc2);
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int row = slice * kWave + rs * G + g;
            if (row >= nrows) continue;
            const size_t at = (size_t)row * LD + t * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[rs][c] += acc2[rs][c];
            store_c<C>(y + at, acc[rs]);
            if constexpr (DOT) {
                double w[C];
                load_v<C>(dot_with + at, w);
#pragma unroll
                for (int c = 0; c < C; ++c) p[c] = fma(w[c], acc[rs][c], p[c]);
            }
        }
    }
    if constexpr (DOT) reduce_cols_store<NB>(p, partial, LD);
}

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
    const int k = threadIdx.x % nb, q = threadIdx.x / nb, nq = kScalBlock / nb;
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
    const int g = blockIdx.x, k = threadIdx.x % nb, q = threadIdx.x / nb, nq = 256 / nb;
    auto chunk = [&](const double* __restrict__ p, int n) {
        const int per = (n + kStageBlocks - 1) / kStageBlocks;
        const int lo = min(n, g * per), hi = min(n, lo + per);
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

// First stage of a two-stage reduction for launches with many partial blocks: block j of kCompressBlocks sums the input
// blocks j, j + kCompressBlocks, ... (fixed order: deterministic) into out[j][k].
static constexpr int kCompressBlocks = 256;   // dot_capacity() reserves this many blocks ahead of the uncompressed ones
__global__ __launch_bounds__(256) void compress_partials_kernel(const double* __restrict__ in, int nblocks, int nb,
                                                                double* __restrict__ out) {
    __shared__ double lds[256];
    const int k = threadIdx.x % nb, q = threadIdx.x / nb, nq = 256 / nb;
    double s0 = 0.0, s1 = 0.0;
    int b = blockIdx.x + kCompressBlocks * q;
    for (; b + kCompressBlocks * nq < nblocks; b += 2 * kCompressBlocks * nq) {
        s0 += in[(size_t)b * nb + k];
        s1 += in[(size_t)(b + kCompressBlocks * nq) * nb + k];
    }
    if (b < nblocks) s0 += in[(size_t)b * nb + k];
    lds[threadIdx.x] = s0 + s1;
    __syncthreads();
    if ((int)threadIdx.x < nb) {
        double t = 0.0;
        for (int g = 0; g < nq; ++g) t += lds[g * nb + threadIdx.x];
        out[(size_t)blockIdx.x * nb + threadIdx.x] = t;
    }
}

// out[k] = sum_b partial[b*nb+k]   (single block)
__global__ __launch_bounds__(kScalBlock) void reduce_final_kernel(const double* __restrict__ partial, int nblocks, int nb,
                                                              double* __restrict__ out) {
    const double s = reduce_partials(partial, nblocks, nb);
    if ((int)threadIdx.x < nb) out[threadIdx.x] = s;
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
// the row-split instantiations (SellView::split_log2) exist for launches of at most 8 realizations
#define PMC_DISPATCH_NARROW(nb, ...)                                      \
    switch (nb) {                                                         \
        case 1: { constexpr int NB = 1; __VA_ARGS__; } break;             \
        case 2: { constexpr int NB = 2; __VA_ARGS__; } break;             \
        case 4: { constexpr int NB = 4; __VA_ARGS__; } break;             \
        case 8: { constexpr int NB = 8; __VA_ARGS__; } break;             \
        default: throw Error(PMC_ERR_INTERNAL, "row-split level kernels serve launches of 1, 2, 4 or 8 realizations"); \
    }

// grid of a group-capable kernel: y = number of column groups of a batch of nb realizations (1 up to kGroup)
static inline dim3 groups(dim3 g, int nb) { return dim3(g.x, nb > kGroup ? (unsigned)(nb / kGroup) : 1u); }
// the slice kernels' grid (see vblock()): column groups of the same slices adjacent on the same XCD
static inline bool xcd_layout(dim3 g, int nb) {
    // off in the product: one lane gains 2.4 % from it, four lanes lose 1 % (LAB_NOTES 10.11); laboratory switch PMC_XCD_GROUPS=1
    static const bool on = [] { const char* e = lab_env("PMC_XCD_GROUPS"); return e && atoi(e) != 0; }();
    return on && nb > kGroup && g.x >= 16;
}
static inline dim3 groups_xcd(dim3 g, int nb) {
    if (!xcd_layout(g, nb)) return groups(g, nb);
    return dim3(8u, (unsigned)(nb / kGroup), (g.x + 7u) / 8u);
}
// number of per-block dot partials such a launch writes (its virtual grid extent)
static inline int dot_blocks(dim3 g, int nb) { return xcd_layout(g, nb) ? (int)((g.x + 7u) / 8u * 8u) : (int)g.x; }
static inline dim3 groups(unsigned g, int nb) { return groups(dim3(g), nb); }
static inline dim3 groups(int g, int nb) { return groups(dim3((unsigned)g), nb); }
static inline dim3 grid_rows(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
static inline dim3 grid_slices(int nslices) { return dim3((unsigned)((nslices + kBlock / kWave - 1) / (kBlock / kWave))); }
static inline int lay_c(int nb) { return nb >= 32 ? 4 : (nb >= 2 ? 2 : 1); }   // = Lay<nb>::C
static inline size_t flat_count(int n, int nb) { return (size_t)n * nb / lay_c(nb); }
// workgroups of k::minres_wx_deferred: each walks `rows` * kBlock consecutive flat entries
static inline unsigned wx_deferred_blocks(size_t nflat, int rows) {
    const size_t per = (size_t)rows * kBlock;
    return (unsigned)((nflat + per - 1) / per);
}
static inline dim3 grid_flat(int n, int nb) { return dim3((unsigned)((flat_count(n, nb) + kBlock - 1) / kBlock)); }
static std::atomic<uint64_t> g_kernel_launches{0};
uint64_t kernel_launch_count() { return g_kernel_launches.load(std::memory_order_relaxed); }
void count_kernel_launches(int n) { g_kernel_launches.fetch_add((uint64_t)n, std::memory_order_relaxed); }
static inline void check_launch(int n = 1) {
    PMC_HIP(hipGetLastError());
    count_kernel_launches(n);
}
// the lean gather loops address rows with 32-bit element offsets: rows x row stride of every gathered vector must fit
static inline void check_offsets32(const SellView& A, int nb) {
    if ((uint64_t)std::max(A.nrows, A.ncols_hint) * (uint64_t)nb >= (1ull << 32))
        throw Error(PMC_ERR_INVALID, "operand exceeds the 32-bit gather offsets of the SpMM kernels (rows x batch width >= 2^32)");
}
// flat vector kernels stream non-temporally once one vector exceeds PMC_NT_FLAT_MB MiB (default 8; 0 = never)
static inline bool nt_flat(size_t doubles) {
    static const double limit = [] {
        const char* e = lab_env("PMC_NT_FLAT_MB");
        return (e ? atof(e) : 8.0) * 1024.0 * 1024.0;
    }();
    return limit > 0.0 && (double)doubles * 8.0 > limit;
}

// kernels with a fused dot write one partial per block; the bound trades occupancy of the SpMM against the length of
// the single-block final reduction (PMC_DOT_GRID overrides it for tuning runs)
static unsigned dot_grid_bound() {
    static const unsigned v = [] {
        const char* e = lab_env("PMC_DOT_GRID");
        const long x = e ? atol(e) : 0;
        return x >= 8 ? (unsigned)x : 4096u;
    }();
    return v;
}

namespace k {

static inline dim3 grid_bounded(dim3 g, bool bounded) { return bounded ? dim3(std::min(g.x, dot_grid_bound())) : g; }

// non-temporal matrix / result streams for the block operator once its operands no longer fit the Infinity Cache.  Inside
// the MINRES loop (in_loop: the launch with the fused dot) they never are cache-resident from half that size on - the rest
// of the iteration moves ~5 x the operator's bytes in between - and the hints pay earlier (0.6 M rows, 195 MB: one lane
// 1057 -> 1063, four lanes 1417 -> 1434 samples/s); PMC_NT_MIN_MB overrides the in-loop threshold.
static inline bool nt_streams(const SellView& A, int nb, bool in_loop) {
    const double bytes = 12.0 * (double)A.nslices * 64.0 * 6.0 + 16.0 * nb * (double)A.nrows;   // ~6 entries per row
    static const double loop_limit = [] {
        const char* e = lab_env("PMC_NT_MIN_MB");
        return (e ? atof(e) : 128.0) * 1024.0 * 1024.0;
    }();
    return bytes > (in_loop ? loop_limit : 256.0 * 1024.0 * 1024.0);
}

// The same hints for the one-pass polynomial kernels (smoothers) of large levels: their matrix and result streams no longer
// displace the gathered rows from L2 (0.6 M rows: one lane 1048 -> 1081 samples/s, four lanes 1367 -> 1380).  Not for the
// residual kernels: their result is read again two launches later (one lane 1103 -> 1084 with the hints).
// PMC_NT_POLY_MB: threshold in MiB of operands, 0 = never.
static inline bool nt_poly(const SellView& A, int nb) {
    static const double limit = [] {
        const char* e = lab_env("PMC_NT_POLY_MB");
        return (e ? atof(e) : 32.0) * 1024.0 * 1024.0;
    }();
    const double bytes = 12.0 * (double)A.nslices * 64.0 * 6.0 + 16.0 * nb * (double)A.nrows;
    return limit > 0.0 && bytes > limit;
}

// one Lanczos pass of the operator (sell_spmm_kernel's LZ forms) with the matrix streams and the dot of the in-loop product
#define PMC_SPMM_LZ(NTF, DLF, LZF)                                                                                          \
    sell_spmm_kernel<NB, false, 0, (LZF) == 1, TAG, NTF, false, DLF, XT, double, LZF><<<groups_xcd(g, nb), kBlock, 0, st>>>( \
        A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb, *lz)

template <int NB, int TAG, typename XT>
static void spmm_launch(hipStream_t st, int nb, dim3 g, const SellView& A, const XT* x, double* y, bool accumulate,
                        double* dot_partial, const XT* dot_with, int lz_mode = 0, const LanczosUpdate* lz = nullptr) {
    // <x, Ax> with a diagonal-last matrix: x_i is what the row's last slice column gathers
    const bool dl = TAG == 1 && Lay<NB>::T > 1 && A.diag_last && dot_with == x;
    if constexpr (!std::is_same<XT, double>::value) {
        // fp32-stored input (the preconditioned Krylov vectors): the operator products of the solver loop only
        if (A.bv || accumulate) throw Error(PMC_ERR_INTERNAL, "spmm: fp32 input with per-realization values / accumulation");
        if constexpr (TAG == 1) {
            if (lz_mode) {
                // the matrix streams of both passes are those of the in-loop product (its launch carries the dot)
                const bool ntl = nt_streams(A, NB, true);
                constexpr bool kDl = Lay<NB>::T > 1;
                if (lz_mode == 1) {
                    if (ntl) { if (dl) PMC_SPMM_LZ(true, kDl, 1); else PMC_SPMM_LZ(true, false, 1); }
                    else { if (dl) PMC_SPMM_LZ(false, kDl, 1); else PMC_SPMM_LZ(false, false, 1); }
                } else if (lz_mode == 2) {
                    if (ntl) PMC_SPMM_LZ(true, false, 2); else PMC_SPMM_LZ(false, false, 2);
                } else {
                    if (ntl) PMC_SPMM_LZ(true, false, 3); else PMC_SPMM_LZ(false, false, 3);
                }
                return;
            }
        }
        const bool nt = TAG != 0 && nt_streams(A, NB, dot_partial != nullptr);
        if (nt) {
            if (dot_partial && dl)
                sell_spmm_kernel<NB, false, 0, true, TAG, true, false, (Lay<NB>::T > 1), XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
            else if (dot_partial)
                sell_spmm_kernel<NB, false, 0, true, TAG, true, false, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
            else
                sell_spmm_kernel<NB, false, 0, false, TAG, true, false, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        } else {
            if (dot_partial && dl)
                sell_spmm_kernel<NB, false, 0, true, TAG, false, false, (Lay<NB>::T > 1), XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
            else if (dot_partial)
                sell_spmm_kernel<NB, false, 0, true, TAG, false, false, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
            else
                sell_spmm_kernel<NB, false, 0, false, TAG, false, false, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        }
        return;
    } else
    if (A.bv && A.f32) {
        if (dot_partial)
            sell_spmm_kernel<NB, 2, 0, true, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (accumulate)
            sell_spmm_kernel<NB, 2, 1, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, 2, 0, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
    } else if (A.bv) {
        if (dot_partial)
            sell_spmm_kernel<NB, true, 0, true, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (accumulate)
            sell_spmm_kernel<NB, true, 1, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, true, 0, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
    } else if (TAG != 0 && nt_streams(A, NB, dot_partial != nullptr)) {
        if (dot_partial && dl)
            sell_spmm_kernel<NB, false, 0, true, TAG, true, false, (Lay<NB>::T > 1)><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (dot_partial)
            sell_spmm_kernel<NB, false, 0, true, TAG, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (accumulate)
            sell_spmm_kernel<NB, false, 1, false, TAG, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, false, 0, false, TAG, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
    } else {
        if (dot_partial && dl)
            sell_spmm_kernel<NB, false, 0, true, TAG, false, false, (Lay<NB>::T > 1)><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (dot_partial)
            sell_spmm_kernel<NB, false, 0, true, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, dot_with, dot_partial, nb);
        else if (accumulate)
            sell_spmm_kernel<NB, false, 1, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, false, 0, false, TAG><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb);
    }
}

template <typename XT>
static int spmm_t(hipStream_t st, int nb, const SellView& A, const XT* x, double* y, bool accumulate, double* dot_partial,
                  const XT* dot_with, int lz_mode = 0, const LanczosUpdate* lz = nullptr) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return 0;
    if (dot_partial && !dot_with) throw Error(PMC_ERR_INTERNAL, "spmm: fused dot without its second vector");
    dim3 g = grid_bounded(grid_slices(A.nslices), dot_partial != nullptr);
    // The block operator keeps one slice per wavefront also with a fused dot (a bounded grid of looping workgroups cost
    // 22 us of 450 at 4.7 M rows); its partial blocks - more than the single-block consumers should read - are first
    // compressed to kCompressBlocks.  They are written behind the compressed ones: dot_capacity() leaves the room.
    const bool two_stage = dot_partial && A.tag != 0 && !A.bv && grid_slices(A.nslices).x > g.x;
    double* kernel_partial = dot_partial;
    if (two_stage) {
        g = grid_slices(A.nslices);
        kernel_partial = dot_partial + (size_t)kCompressBlocks * nb;
    }
    PMC_DISPATCH_NB(nb, {
        if (A.tag == 1) spmm_launch<NB, 1, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with, lz_mode, lz);
        else if (A.tag == 2) spmm_launch<NB, 2, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with);
        else spmm_launch<NB, 0, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with);
    });
    check_launch();
    if (two_stage) {
        compress_partials_kernel<<<kCompressBlocks, 256, 0, st>>>(kernel_partial, dot_blocks(g, nb), nb, dot_partial);
        check_launch();
        return kCompressBlocks;
    }
    return dot_partial ? dot_blocks(g, nb) : 0;
}
int spmm(hipStream_t st, int nb, const SellView& A, const double* x, double* y, bool accumulate, double* dot_partial,
         const double* dot_with) {
    return spmm_t<double>(st, nb, A, x, y, accumulate, dot_partial, dot_with);
}
int spmm_z(hipStream_t st, int nb, const SellView& A, zvec x, double* y, double* dot_partial, zvec dot_with) {
    if (x.f32) return spmm_t<float>(st, nb, A, x.as<float>(), y, false, dot_partial, dot_with.as<float>());
    return spmm_t<double>(st, nb, A, x.as<double>(), y, false, dot_partial, dot_with.as<double>());
}

static void check_lanczos_pass(const SellView& A, zvec x) {
    if (!x.f32 || A.bv || A.tag != 1)
        throw Error(PMC_ERR_INTERNAL, "Lanczos operator passes: shared values, fp32-stored input, the solver's operator");
}
int spmm_z_dot(hipStream_t st, int nb, const SellView& A, zvec x, double* dot_partial) {
    check_lanczos_pass(A, x);
    const LanczosUpdate none{};
    return spmm_t<float>(st, nb, A, x.as<float>(), nullptr, false, dot_partial, x.as<float>(), 1, &none);
}
void spmm_z_update(hipStream_t st, int nb, const SellView& A, zvec x, const LanczosUpdate& lz, double* v, bool v_zero) {
    check_lanczos_pass(A, x);
    if (!lz.c0 || !lz.c1 || !lz.c2 || !lz.v1 || !lz.y32 || !v)
        throw Error(PMC_ERR_INTERNAL, "Lanczos update pass: operand missing");
    spmm_t<float>(st, nb, A, x.as<float>(), v, false, nullptr, nullptr, v_zero ? 3 : 2, &lz);
}

void residual_restrict8(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, double* out,
                        double* coarse) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.nrows % 8 != 0) throw Error(PMC_ERR_INTERNAL, "residual_restrict8: rows are not groups of 8");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, {
        if (A.bv && A.f32)
            sell_spmm_kernel<NB, 2, 2, false, 0, false, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, coarse, nb);
        else if (A.bv)
            sell_spmm_kernel<NB, true, 2, false, 0, false, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, coarse, nb);
        else
            sell_spmm_kernel<NB, false, 2, false, 0, false, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, coarse, nb);
    });
    check_launch();
}

void spmm_store32(hipStream_t st, int nb, const SellView& A, const double* x, double* y, float* y32) {
    check_offsets32(A, nb);
    if (A.bv || A.tag != 0 || !y || !y32) throw Error(PMC_ERR_INTERNAL, "spmm_store32: shared values, an untagged matrix, both results");
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    LanczosUpdate lz{};
    lz.y32 = y32;
    PMC_DISPATCH_NB(nb, {
        sell_spmm_kernel<NB, false, 0, false, 0, false, false, false, double, double, 4><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, nullptr, nullptr, nullptr, nb, lz);
    });
    check_launch();
}

void residual_samples(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, bool do_exp, double* out) {
    check_offsets32(A, nb);
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "residual_samples: shared values only");
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, {
        if (do_exp)
            sell_spmm_kernel<NB, false, 2, false, 0, false, false, false, double, double, 0, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, false, 2, false, 0, false, false, false, double, double, 0, 1><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, nullptr, nb);
    });
    check_launch();
}

void residual(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, double* out) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, {
        if (A.bv && A.f32)
            sell_spmm_kernel<NB, 2, 2, false, 0><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, nullptr, nb);
        else if (A.bv)
            sell_spmm_kernel<NB, true, 2, false, 0><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, nullptr, nb);
        else
            sell_spmm_kernel<NB, false, 2, false, 0><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, out, r, nullptr, nullptr, nb);
    });
    check_launch();
}

template <typename OT>
static int cheb_step_t(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
                       const double* xin, double* d, OT* xout, double a, double b, double* dot_partial) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return 0;
    if (A.bv != dinv_bv) throw Error(PMC_ERR_INTERNAL, "cheb_step: value/diagonal batching mismatch");
    const dim3 g = grid_bounded(grid_slices(A.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (A.bv && A.f32) {
            if (dot_partial)
                sell_cheb_kernel<NB, 2, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, dot_partial, nb);
            else
                sell_cheb_kernel<NB, 2, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, nullptr, nb);
        } else if (A.bv) {
            if (dot_partial)
                sell_cheb_kernel<NB, 1, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, dot_partial, nb);
            else
                sell_cheb_kernel<NB, 1, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, nullptr, nb);
        } else {
            if (dot_partial)
                sell_cheb_kernel<NB, 0, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, dot_partial, nb);
            else
                sell_cheb_kernel<NB, 0, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, nullptr, nb);
        }
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int cheb_step(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
              const double* xin, double* d, double* xout, double a, double b, double* dot_partial) {
    return cheb_step_t<double>(st, nb, A, dinv, dinv_bv, r, xin, d, xout, a, b, dot_partial);
}

// fp64 storage: the iterate of the last step goes straight to zout, d is left as it was (as the typed kernel does)
int cheb_step_z(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
                const double* xin, double* d, zvec zout, double a, double b, double* dot_partial) {
    if (zout.f32) return cheb_step_t<float>(st, nb, A, dinv, dinv_bv, r, xin, d, zout.as<float>(), a, b, dot_partial);
    return cheb_step_t<double>(st, nb, A, dinv, dinv_bv, r, xin, d, zout.as<double>(), a, b, dot_partial);
}

template <typename OT>
static int poly2_t(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, OT* xout,
                   double c0, double c1, double* dot_partial, const double* xadd, const double* dot_with, const int* padd_idx,
                   const double* padd_x) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return 0;
    if (As.bv != dinv_bv) throw Error(PMC_ERR_INTERNAL, "poly2: value/diagonal batching mismatch");
    const dim3 g = grid_bounded(grid_slices(As.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (As.bv && As.f32) {
            if (dot_partial)
                sell_poly2_kernel<NB, 2, true, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x, nb);
            else
                sell_poly2_kernel<NB, 2, false, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, xadd, dot_with, padd_idx, padd_x, nb);
        } else if (As.bv) {
            if (dot_partial)
                sell_poly2_kernel<NB, 1, true, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x, nb);
            else
                sell_poly2_kernel<NB, 1, false, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, xadd, dot_with, padd_idx, padd_x, nb);
        } else if (nt_poly(As, NB)) {
            if (dot_partial)
                sell_poly2_kernel<NB, 0, true, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x, nb);
            else
                sell_poly2_kernel<NB, 0, false, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, xadd, dot_with, padd_idx, padd_x, nb);
        } else {
            if (dot_partial)
                sell_poly2_kernel<NB, 0, true, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x, nb);
            else
                sell_poly2_kernel<NB, 0, false, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, xadd, dot_with, padd_idx, padd_x, nb);
        }
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int poly2(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, double* xout,
          double c0, double c1, double* dot_partial, const double* xadd, const double* dot_with, const int* padd_idx,
          const double* padd_x) {
    return poly2_t<double>(st, nb, As, dinv, dinv_bv, r, xout, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x);
}

int poly2_z(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, zvec xout,
            double c0, double c1, double* dot_partial, const double* xadd, const double* dot_with, const int* padd_idx,
            const double* padd_x) {
    if (xout.f32)
        return poly2_t<float>(st, nb, As, dinv, dinv_bv, r, xout.as<float>(), c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x);
    return poly2_t<double>(st, nb, As, dinv, dinv_bv, r, xout.as<double>(), c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x);
}

// a level runs the deep gather loop (sell_row_range_deep) when its launch has at most this many wavefronts - about two per
// SIMD of the chip (PMC_DEEP_WAVES in laboratory builds; 0 = never)
static inline bool deep_level(const SellView& A, int nb) {
    static const long limit = [] {
        const char* e = lab_env("PMC_DEEP_WAVES");
        return e ? atol(e) : 0L;   // off in the product: measured neutral on config 2 (LAB_NOTES 10), kept for laboratory runs
    }();
    return nb >= kGroup && !A.bv && (long)A.nslices * (nb / kGroup) <= limit;
}

// the launchers below take the right-hand side and the inter-level vectors (coarse right-hand side, coarse correction) of a
// shared-value level in either storage: T names the element type inside the braces
#define PMC_DISPATCH_F32(is_f32, T, ...)                \
    if (is_f32) { using T = float; __VA_ARGS__; }       \
    else { using T = double; __VA_ARGS__; }

// r in fp32: the copy of the Lanczos vector the MINRES loop keeps for the top level of a cycle (k::lincomb3) - gathered, and
// read at the own row, as 128-byte rows instead of 256-byte ones - or the coarse right-hand side the level above wrote
template <typename RT>
static void vc_presmooth32_t(hipStream_t st, int nb, const SellView& As, const double* dinv, const RT* r, float* xout, double c0,
                             double c1) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return;
    if (As.bv) throw Error(PMC_ERR_INTERNAL, "vc_presmooth32: shared values expected");
    const dim3 g = grid_slices(As.nslices);
    if (As.split_log2) {
        PMC_DISPATCH_NARROW(nb, {
            vc_poly2_kernel<NB, RT, float, float, false, false, 0, 1, true><<<g, kBlock, 0, st>>>(As.nrows >> As.split_log2, As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, nullptr, nb, As.split_log2);
        });
        check_launch();
        return;
    }
    if (deep_level(As, nb)) {
        vc_poly2_kernel<kGroup, RT, float, float, false, false, 0, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, nullptr, nb);
        check_launch();
        return;
    }
    PMC_DISPATCH_NB(nb, {
        if (nt_poly(As, NB))
            vc_poly2_kernel<NB, RT, float, float, false, true><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, nullptr, nb);
        else
            vc_poly2_kernel<NB, RT, float, float, false><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, nullptr, nb);
    });
    check_launch();
}
void vc_presmooth32(hipStream_t st, int nb, const SellView& As, const double* dinv, zvec r, float* xout, double c0, double c1) {
    PMC_DISPATCH_F32(r.f32, RT, vc_presmooth32_t<RT>(st, nb, As, dinv, r.as<RT>(), xout, c0, c1));
}

void vc_residual_restrict8_32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv || A.nrows % 8 != 0) throw Error(PMC_ERR_INTERNAL, "vc_residual_restrict8_32: shared values and groups of 8 rows expected");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_F32(r.f32, RT, PMC_DISPATCH_F32(coarse.f32, CT, PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, float, RT, float, true, 0, true, 1, false, false, CT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r.as<RT>(), out, coarse.as<CT>(), nb);
    })));
    check_launch();
}

template <typename RT>
static void vc_residual32_t(hipStream_t st, int nb, const SellView& A, const RT* r, const float* x, float* out) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual32: shared values expected");
    const dim3 g = grid_slices(A.nslices);
    if (A.split_log2) {
        PMC_DISPATCH_NARROW(nb, {
            vc_residual_kernel<NB, float, RT, float, false, 0, true, 1, false, true><<<g, kBlock, 0, st>>>(A.nrows >> A.split_log2, A.nslices, A.slice_off, A.cols, A.vals, x, r, out, nullptr, nb, nullptr, nullptr, nullptr, A.split_log2);
        });
        check_launch();
        return;
    }
    if (deep_level(A, nb)) {
        vc_residual_kernel<kGroup, float, RT, float, false, 0, true, 4><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r, out, nullptr, nb);
        check_launch();
        return;
    }
    PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, float, RT, float, false><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r, out, nullptr, nb);
    });
    check_launch();
}
void vc_residual32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out) {
    PMC_DISPATCH_F32(r.f32, RT, vc_residual32_t<RT>(st, nb, A, r.as<RT>(), x, out));
}

void vc_residual_restrict_agg32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse,
                                const int* seg_ptr, const int* seg_cid, const int* seg_pos) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual_restrict_agg32: shared values expected");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_F32(r.f32, RT, PMC_DISPATCH_F32(coarse.f32, CT, PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, float, RT, float, false, 0, true, 1, true, false, CT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r.as<RT>(), out, coarse.as<CT>(), nb, seg_ptr, seg_cid, seg_pos);
    })));
    check_launch();
}

// coarse = Pt res (the restriction of a level without a fused one): fp64 through the product every caller uses, fp32 through
// the same kernel with a typed result
void vc_restrict32(hipStream_t st, int nb, const SellView& Pt, const float* res, zvec coarse) {
    if (!coarse.f32) {
        spmm_z(st, nb, Pt, zvec(const_cast<float*>(res), true), coarse.as<double>(), nullptr, zvec());
        return;
    }
    check_offsets32(Pt, nb);
    if (Pt.nrows == 0) return;
    if (Pt.bv) throw Error(PMC_ERR_INTERNAL, "vc_restrict32: shared values expected");
    const dim3 g = grid_slices(Pt.nslices);
    PMC_DISPATCH_NB(nb, {
        sell_spmm_kernel<NB, false, 0, false, 0, false, false, false, float, float><<<groups_xcd(g, nb), kBlock, 0, st>>>(Pt.nrows, Pt.nslices, Pt.slice_off, Pt.sched, Pt.cols, Pt.vals, res, coarse.as<float>(), nullptr, nullptr, nullptr, nb);
    });
    check_launch();
}

template <typename XT>
static void vc_residual_coarse32_t(hipStream_t st, int nb, const SellView& SP, float* res, const XT* xc) {
    check_offsets32(SP, nb);
    if (SP.nrows == 0) return;
    if (SP.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual_coarse32: shared values expected");
    const dim3 g = grid_slices(SP.nslices);
    if (SP.split_log2) {
        PMC_DISPATCH_NARROW(nb, {
            vc_residual_kernel<NB, XT, float, float, false, 0, true, 1, false, true, double, 1><<<g, kBlock, 0, st>>>(SP.nrows >> SP.split_log2, SP.nslices, SP.slice_off, SP.cols, SP.vals, xc, res, res, nullptr, nb, nullptr, nullptr, nullptr, SP.split_log2);
        });
        check_launch();
        return;
    }
    if (deep_level(SP, nb)) {
        vc_residual_kernel<kGroup, XT, float, float, false, 0, true, 2, false, false, double, 1><<<groups_xcd(g, nb), kBlock, 0, st>>>(SP.nrows, SP.nslices, SP.slice_off, SP.cols, SP.vals, xc, res, res, nullptr, nb);
        check_launch();
        return;
    }
    PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, XT, float, float, false, 0, true, 1, false, false, double, 1><<<groups_xcd(g, nb), kBlock, 0, st>>>(SP.nrows, SP.nslices, SP.slice_off, SP.cols, SP.vals, xc, res, res, nullptr, nb);
    });
    check_launch();
}
void vc_residual_coarse32(hipStream_t st, int nb, const SellView& SP, float* res, zvec xc) {
    PMC_DISPATCH_F32(xc.f32, XT, vc_residual_coarse32_t<XT>(st, nb, SP, res, xc.as<XT>()));
}

template <typename OT, typename PT>
static int vc_postsmooth32_t(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                             OT* xout, double c0, double c1, const double* r, const int* parent, const PT* xc,
                             double* dot_partial) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return 0;
    if (As.bv) throw Error(PMC_ERR_INTERNAL, "vc_postsmooth32: shared values expected");
    const dim3 g = grid_bounded(grid_slices(As.nslices), dot_partial != nullptr);
    if (As.split_log2) {
        if (dot_partial) throw Error(PMC_ERR_INTERNAL, "vc_postsmooth32: the row-split form serves inner levels (no fused dot)");
        PMC_DISPATCH_NARROW(nb, {
            vc_poly2_kernel<NB, float, OT, float, false, false, 0, 1, true, false, PT><<<g, kBlock, 0, st>>>(As.nrows >> As.split_log2, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc, nb, As.split_log2);
        });
        check_launch();
        return 0;
    }
    if (deep_level(As, nb)) {
        if (dot_partial)
            vc_poly2_kernel<kGroup, float, OT, float, true, false, 0, 4, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc, nb);
        else
            vc_poly2_kernel<kGroup, float, OT, float, false, false, 0, 4, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc, nb);
        check_launch();
        return dot_partial ? dot_blocks(g, nb) : 0;
    }
    // 64 per launch on a large level: both column groups of a slice in one workgroup (vc_poly2_kernel, GIB).  Off in the
    // product: one lane 2 870 -> 2 815 samples/s, four lanes 3 745 -> 3 757 (LAB_NOTES 10.19); laboratory switch PMC_GIB=1
    static const bool gib = [] { const char* e = lab_env("PMC_GIB"); return e && atoi(e) != 0; }();
    if (gib && nb == 2 * kGroup && nt_poly(As, kGroup) && !xcd_layout(g, nb)) {
        if (dot_partial)
            vc_poly2_kernel<kGroup, float, OT, float, true, true, 0, 1, false, true, PT><<<g, kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc, nb);
        else
            vc_poly2_kernel<kGroup, float, OT, float, false, true, 0, 1, false, true, PT><<<g, kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc, nb);
        check_launch();
        return dot_partial ? (int)g.x : 0;
    }
    PMC_DISPATCH_NB(nb, {
        if (nt_poly(As, NB)) {
            if (dot_partial)
                vc_poly2_kernel<NB, float, OT, float, true, true, 0, 1, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc, nb);
            else
                vc_poly2_kernel<NB, float, OT, float, false, true, 0, 1, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc, nb);
        } else if (dot_partial)
            vc_poly2_kernel<NB, float, OT, float, true, false, 0, 1, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc, nb);
        else
            vc_poly2_kernel<NB, float, OT, float, false, false, 0, 1, false, false, PT><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc, nb);
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int vc_postsmooth32_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                      zvec xout, double c0, double c1, const double* r, const int* parent, zvec xc, double* dot_partial) {
    int nblk = 0;
    PMC_DISPATCH_F32(xout.f32, OT, PMC_DISPATCH_F32(xc.f32, PT, {
        nblk = vc_postsmooth32_t<OT, PT>(st, nb, As, dinv, res, x, xout.as<OT>(), c0, c1, r, parent, xc.as<PT>(), dot_partial);
    }));
    return nblk;
}

// ---- the same level with per-realization fp32 values (Darcy; SellView::f32) and per-realization diagonals
void vc_presmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const double* r, float* xout, double c0,
                       double c1) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return;
    if (!(As.bv && As.f32)) throw Error(PMC_ERR_INTERNAL, "vc_presmooth32_bv: per-realization fp32 values expected");
    const dim3 g = grid_slices(As.nslices);
    PMC_DISPATCH_NB(nb, {
        vc_poly2_kernel<NB, double, float, float, false, false, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, nullptr, nb);
    });
    check_launch();
}

void vc_restrict8_32_bv(hipStream_t st, int nb, const SellView& A, const double* r, const float* x, double* coarse) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (!(A.bv && A.f32) || A.nrows % 8 != 0) throw Error(PMC_ERR_INTERNAL, "vc_restrict8_32_bv: operand mismatch");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, float, double, float, true, 2, false><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r, nullptr, coarse, nb);
    });
    check_launch();
}

void vc_prolong8_32(hipStream_t st, int nb, int n, float* x, const double* xc) {
    if (n == 0) return;
    PMC_DISPATCH_NB(nb, { vc_prolong8_kernel<NB><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), x, xc, nb); });
    check_launch();
}

void vc_residual32_bv(hipStream_t st, int nb, const SellView& A, const double* r, const float* x, float* out) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (!(A.bv && A.f32)) throw Error(PMC_ERR_INTERNAL, "vc_residual32_bv: per-realization fp32 values expected");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, {
        vc_residual_kernel<NB, float, double, float, false, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(A.nrows, A.nslices, A.slice_off, A.cols, A.vals, x, r, out, nullptr, nb);
    });
    check_launch();
}

template <typename OT>
static int vc_postsmooth32_bv_t(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                                OT* xout, double c0, double c1, const double* r, double* dot_partial) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return 0;
    if (!(As.bv && As.f32)) throw Error(PMC_ERR_INTERNAL, "vc_postsmooth32_bv: per-realization fp32 values expected");
    const dim3 g = grid_bounded(grid_slices(As.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (dot_partial)
            vc_poly2_kernel<NB, float, OT, float, true, false, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, dot_partial, x, r, nullptr, nullptr, nb);
        else
            vc_poly2_kernel<NB, float, OT, float, false, false, 2><<<groups_xcd(g, nb), kBlock, 0, st>>>(As.nrows, As.nslices, As.slice_off, As.cols, As.vals, dinv, res, xout, c0, c1, nullptr, x, nullptr, nullptr, nullptr, nb);
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int vc_postsmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                       double* xout, double c0, double c1, const double* r, double* dot_partial) {
    return vc_postsmooth32_bv_t<double>(st, nb, As, dinv, res, x, xout, c0, c1, r, dot_partial);
}
int vc_postsmooth32_bv_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                         zvec xout, double c0, double c1, const double* r, double* dot_partial) {
    if (xout.f32) return vc_postsmooth32_bv_t<float>(st, nb, As, dinv, res, x, xout.as<float>(), c0, c1, r, dot_partial);
    return vc_postsmooth32_bv_t<double>(st, nb, As, dinv, res, x, xout.as<double>(), c0, c1, r, dot_partial);
}

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
        if (nt_flat((size_t)M.nrows * NB * 2)) {   // from 4 MiB per vector on
            if (dot_partial)
                eg_pair_spmm_kernel<NB, true, true, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, A2.slice_off, A2.cols, A2.vals, x1, x2, y, dot_with, dot_partial, nb);
            else
                eg_pair_spmm_kernel<NB, false, true, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, A2.slice_off, A2.cols, A2.vals, x1, x2, y, nullptr, nullptr, nb);
        } else if (dot_partial)
            eg_pair_spmm_kernel<NB, true, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, A2.slice_off, A2.cols, A2.vals, x1, x2, y, dot_with, dot_partial, nb);
        else
            eg_pair_spmm_kernel<NB, false, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, A2.slice_off, A2.cols, A2.vals, x1, x2, y, nullptr, nullptr, nb);
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
    if (x1.f32)
        return eg_pair_spmm_t<float>(st, nb, M, coef, x1.as<float>(), A2, x2.as<float>(), y, dot_partial, dot_with.as<float>());
    return eg_pair_spmm_t<double>(st, nb, M, coef, x1.as<double>(), A2, x2.as<double>(), y, dot_partial, dot_with.as<double>());
}

template <typename OT>
static int eg_poly2_t(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, OT* xout,
                      double c0, double c1, double* dot_partial) {
    if (M.nrows == 0) return 0;
    if ((uint64_t)M.nrows * (uint64_t)nb >= (1ull << 32))
        throw Error(PMC_ERR_INVALID, "eg_poly2: rows x batch width exceed 32-bit gather offsets");
    const dim3 g = grid_bounded(grid_slices(M.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (nt_flat((size_t)M.nrows * NB * 2)) {
            if (dot_partial)
                eg_poly2_kernel<NB, true, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, dinv, r, xout, c0, c1, dot_partial, nb);
            else
                eg_poly2_kernel<NB, false, true, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, dinv, r, xout, c0, c1, nullptr, nb);
        } else if (dot_partial)
            eg_poly2_kernel<NB, true, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, dinv, r, xout, c0, c1, dot_partial, nb);
        else
            eg_poly2_kernel<NB, false, false, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(M.nrows, M.nslices, M.gw, M.cols, M.w, M.e12, coef, dinv, r, xout, c0, c1, nullptr, nb);
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
    if (xout.f32) return eg_poly2_t<float>(st, nb, M, coef, dinv, r, xout.as<float>(), c0, c1, dot_partial);
    return eg_poly2_t<double>(st, nb, M, coef, dinv, r, xout.as<double>(), c0, c1, dot_partial);
}

template <typename XT>
static int pair_spmm_t(hipStream_t st, int nb, const SellView& A1, const XT* x1, const SellView& A2, const XT* x2, double* y,
                       double* dot_partial, const XT* dot_with) {
    check_offsets32(A1, nb);
    if (A1.nrows == 0) return 0;
    if (!A1.bv || A2.bv || A1.nrows != A2.nrows || A1.nslices != A2.nslices)
        throw Error(PMC_ERR_INTERNAL, "pair_spmm: operand mismatch");
    const dim3 g = grid_bounded(grid_slices(A1.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (dot_partial)
            sell_pair_spmm_kernel<NB, true, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A1.nrows, A1.nslices, A1.slice_off, A1.cols, A1.vals, A2.slice_off, A2.cols, A2.vals, x1, x2, y, dot_with, dot_partial, nb);
        else
            sell_pair_spmm_kernel<NB, false, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(A1.nrows, A1.nslices, A1.slice_off, A1.cols, A1.vals, A2.slice_off, A2.cols, A2.vals, x1, x2, y, nullptr, nullptr, nb);
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int pair_spmm_z(hipStream_t st, int nb, const SellView& A1, zvec x1, const SellView& A2, zvec x2, double* y,
                double* dot_partial, zvec dot_with) {
    if (x1.f32) return pair_spmm_t<float>(st, nb, A1, x1.as<float>(), A2, x2.as<float>(), y, dot_partial, dot_with.as<float>());
    return pair_spmm_t<double>(st, nb, A1, x1.as<double>(), A2, x2.as<double>(), y, dot_partial, dot_with.as<double>());
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

void minres_wx_idx(hipStream_t st, int nb, int nsel, const int* rows, const double* c0, zvec u, const double* c1,
                   double* w0, const double* c2, const double* w1, const double* c3, double* x) {
    if (nsel == 0) return;
    PMC_DISPATCH_NB(nb, {
        if (u.f32) minres_wx_idx_kernel<NB, float><<<grid_flat(nsel, nb), kBlock, 0, st>>>(flat_count(nsel, nb), rows, c0, u.as<float>(), c1, w0, c2, w1, c3, x, nb);
        else minres_wx_idx_kernel<NB, double><<<grid_flat(nsel, nb), kBlock, 0, st>>>(flat_count(nsel, nb), rows, c0, u.as<double>(), c1, w0, c2, w1, c3, x, nb);
    });
    check_launch();
}

int cheb_first(hipStream_t st, int nb, int n, const double* dinv, bool dinv_bv, const double* r, double* d, double* x,
               double b, double* dot_partial) {
    if (n == 0) return 0;
    const size_t nf = flat_count(n, nb);
    const dim3 g = grid_bounded(grid_flat(n, nb), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, {
        if (dinv_bv) {
            if (dot_partial) cheb_first_kernel<NB, true, true><<<g, kBlock, 0, st>>>(nf, dinv, r, d, x, b, dot_partial, nb);
            else cheb_first_kernel<NB, true, false><<<g, kBlock, 0, st>>>(nf, dinv, r, d, x, b, nullptr, nb);
        } else {
            if (dot_partial) cheb_first_kernel<NB, false, true><<<g, kBlock, 0, st>>>(nf, dinv, r, d, x, b, dot_partial, nb);
            else cheb_first_kernel<NB, false, false><<<g, kBlock, 0, st>>>(nf, dinv, r, d, x, b, nullptr, nb);
        }
    });
    check_launch();
    return dot_partial ? (int)g.x : 0;
}

static inline dim3 grid_dot(int n, int nb) { return dim3(std::min(grid_flat(n, nb).x, 1024u)); }

int dot_z(hipStream_t st, int nb, int n, const double* a, zvec b, double* partial) {
    const dim3 g = grid_dot(n, nb);
    PMC_DISPATCH_NB(nb, {
        if (b.f32) dot_kernel<NB, float><<<g, kBlock, 0, st>>>(flat_count(n, nb), a, b.as<float>(), partial, nb);
        else dot_kernel<NB, double><<<g, kBlock, 0, st>>>(flat_count(n, nb), a, b.as<double>(), partial, nb);
    });
    check_launch();
    return (int)g.x;
}

int convert_z(hipStream_t st, int nb, int n, const double* in, zvec out, const double* r, double* dot_partial) {
    if (n == 0) return 0;
    const dim3 g = grid_dot(n, nb);
    PMC_DISPATCH_NB(nb, {
        if (out.f32) {
            if (dot_partial) convert_dot_kernel<NB, true, float><<<g, kBlock, 0, st>>>(flat_count(n, nb), in, out.as<float>(), r, dot_partial, nb);
            else convert_dot_kernel<NB, false, float><<<g, kBlock, 0, st>>>(flat_count(n, nb), in, out.as<float>(), nullptr, nullptr, nb);
        } else {
            if (dot_partial) convert_dot_kernel<NB, true, double><<<g, kBlock, 0, st>>>(flat_count(n, nb), in, out.as<double>(), r, dot_partial, nb);
            else convert_dot_kernel<NB, false, double><<<g, kBlock, 0, st>>>(flat_count(n, nb), in, out.as<double>(), nullptr, nullptr, nb);
        }
    });
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
    PMC_DISPATCH_NB(nb, {
        if (nt) lincomb3_kernel<NB, true><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, a, c1, b, c2, y, nb, y32);
        else lincomb3_kernel<NB><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, a, c1, b, c2, y, nb, y32);
    });
    check_launch();
}

template <typename UT>
static void minres_wx_t(hipStream_t st, int nb, int n, const double* c0, const UT* u, const double* c1, double* w0,
                        const double* c2, const double* w1, const double* c3, double* x) {
    const bool nt = nt_flat((size_t)n * nb);
    PMC_DISPATCH_NB(nb, {
        if (nt) minres_wx_kernel<NB, true, UT><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, u, c1, w0, c2, w1, c3, x, nb);
        else minres_wx_kernel<NB, false, UT><<<grid_flat(n, nb), kBlock, 0, st>>>(flat_count(n, nb), c0, u, c1, w0, c2, w1, c3, x, nb);
    });
}
void minres_wx(hipStream_t st, int nb, int n, const double* c0, zvec u, const double* c1, double* w0,
               const double* c2, const double* w1, const double* c3, double* x) {
    if (u.f32) minres_wx_t<float>(st, nb, n, c0, u.as<float>(), c1, w0, c2, w1, c3, x);
    else minres_wx_t<double>(st, nb, n, c0, u.as<double>(), c1, w0, c2, w1, c3, x);
    check_launch();
}

void minres_wx_deferred(hipStream_t st, int nb, int n, const MinresState* s, const WxDeferred& B, double* w0, double* w1,
                        double* x) {
    if (n == 0 || B.cnt == 0) return;
    if (B.cnt < 0 || B.cnt > kWxWindow) throw Error(PMC_ERR_INTERNAL, "minres_wx_deferred: bad count");
    const double* cW = reinterpret_cast<const double*>(reinterpret_cast<const char*>(s) + offsetof(MinresState, cW));
    const bool nt = nt_flat((size_t)n * nb);
    // the entries of one thread share their columns (see the kernel): kBlock * C flat values are whole rows
    if ((kBlock * lay_c(nb)) % nb != 0) throw Error(PMC_ERR_INTERNAL, "minres_wx_deferred: row stride does not divide a workgroup's step");
    const size_t nf = flat_count(n, nb);
    PMC_DISPATCH_NB(nb, {
        constexpr int C = Lay<NB>::C;
        const dim3 g32(wx_deferred_blocks(nf, WxShape<float, C>::R)), g64(wx_deferred_blocks(nf, WxShape<double, C>::R));
        if (B.f32) {
            if (nt) minres_wx_deferred_kernel<NB, true, float><<<g32, kBlock, 0, st>>>(nf, B, cW, w0, w1, x, nb);
            else minres_wx_deferred_kernel<NB, false, float><<<g32, kBlock, 0, st>>>(nf, B, cW, w0, w1, x, nb);
        } else {
            if (nt) minres_wx_deferred_kernel<NB, true, double><<<g64, kBlock, 0, st>>>(nf, B, cW, w0, w1, x, nb);
            else minres_wx_deferred_kernel<NB, false, double><<<g64, kBlock, 0, st>>>(nf, B, cW, w0, w1, x, nb);
        }
    });
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

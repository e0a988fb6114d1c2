// Kernels in which a wavefront sweeps the slices of a SELL-64 matrix through sell_row_range, with their launchers: the
// operator products (K5, K3/K4, K11) with their Lanczos forms, residuals with fused restriction / sample-major stores,
// Chebyshev steps and the one-pass degree-2 polynomial (K7, K8), the V-cycle level kernels with fp32 intermediates, the pair
// product of the Darcy u-rows, and the first stage of the two-stage dot reduction.  fp64 values, int32 indices, HBM-bound:
// no MFMA (<= 0.17 flop/byte), 64-wide wavefronts, SELL-64 operators so that every matrix load of a wavefront is one
// contiguous 512 B (values) / 256 B (columns) segment.
//
// Why the V-cycle kernels are not a unit of their own: sell_row_range takes its optional results (xlast, pdot) as run-time
// pointers, and the compiler specialises a device function for the arguments ALL callers in its translation unit agree on
// before it inlines it.  The diagonal-last forms of sell_spmm_kernel pass xlast; every other caller of the same
// specialisations (NB = 4, 8, 16, shared values: sell_cheb / sell_poly2 / sell_pair_spmm / vc_*) passes nullptr and, in a unit
// without sell_spmm_kernel, comes out with other machine code (measured for the vc_* kernels: 108 of them, LAB_NOTES 10.28).
// They stay in one unit until those arguments are template parameters.
#include "klaunch.hpp"
#include "sell_rows.hpp"

namespace pmc {

template <int NB, int BV, typename XT = double>
__device__ __forceinline__ void sell_row_product(const int* __restrict__ slice_off, const int* __restrict__ cols,
                                                 const double* __restrict__ vals, const XT* __restrict__ x,
                                                 int slice, int lane, int LD, double (&acc)[Lay<NB>::T][Lay<NB>::C]) {
    const int off = slice_off[slice];
    const int width = (slice_off[slice + 1] - off) >> 6;
    sell_row_range<NB, BV, false, true, false, XT>(cols, vals, x, nullptr, off, width, lane, LD, acc);
}

// Row steps whose own-row reads an update pass (LZ 2 / 3) issues together: 64 B per lane and row step with v0 (LZ 2), 32 B
// without (LZ 3), so both keep 128 B per lane in flight - what the gather loop does.  (gfx950, NB = 32, fp32 x: 150 VGPRs, no
// scratch, 3 waves per SIMD; four row steps with v0 need 168 + 40 B of scratch)
template <int NB, int LZ>
constexpr int lz_batch() {
    constexpr int H = LZ == 3 ? 4 : 2;
    return Lay<NB>::T >= H ? H : Lay<NB>::T;
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
    // update passes: the lane's coefficients depend on the column group and t only - read once per wavefront, not behind
    // every row step's stores (which the compiler must assume to alias them)
    constexpr bool LZU = LZ == 2 || LZ == 3;
    double cz0[LZU ? C : 1], cz1[LZU ? C : 1], cz2[LZU ? C : 1];
    if constexpr (LZU) {
        load_c<C>(lz.c0 + t * C, cz0);
        load_c<C>(lz.c1 + t * C, cz1);
        load_c<C>(lz.c2 + t * C, cz2);
    }
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
        if constexpr (LZU) {
            // row steps in batches of H: the own rows of v1 and v0 of the whole batch are in flight together, then the batch
            // is combined and stored - rows past the end re-read the last row and store nothing
            constexpr int H = lz_batch<NB, LZ>();
#pragma unroll
            for (int h0 = 0; h0 < T; h0 += H) {
                double bv[H][C], yv[H][C];
                size_t at[H];
                bool ok[H];
#pragma unroll
                for (int u = 0; u < H; ++u) {
                    const int row = slice * kWave + (h0 + u) * G + g;
                    ok[u] = row < nrows;
                    at[u] = (size_t)(ok[u] ? row : nrows - 1) * LD + t * C;
                    load_c_nt<NT, C>(lz.v1 + at[u], bv[u]);
                    if constexpr (LZ == 2) {
                        load_c_nt<NT, C>(y + at[u], yv[u]);
                    } else {
#pragma unroll
                        for (int c = 0; c < C; ++c) yv[u][c] = 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < H; ++u) {
                    lanczos_combine<C>(cz0, cz1, cz2, acc[h0 + u], bv[u], yv[u]);
                    if (ok[u]) {
                        store_c<C>(y + at[u], yv[u]);          // gathered by the next kernels
                        store_v<C>(lz.y32 + at[u], yv[u]);
                    }
                }
            }
            continue;
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
// EPS: the optional operands of the epilogue are compile-time facts - xadd is there iff XA, the coarse correction (padd_idx,
// padd_x) iff PA, dot_with iff DOT - so that a pair of row steps is one basic block: with run-time pointers every
// `if (ptr)` is a branch the compiler moves no load across, and the pair drained the memory counter three times
template <int NB, typename XT, typename OT, typename AT, bool DOT, bool NT = false, int BV = 0, int DEEP = 1, bool SPL = false,
          bool GIB = false, typename PT = double, bool EPS = false, bool XA = false, bool PA = false>
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
    static_assert(!EPS || (BV == 0 && DEEP == 1 && !SPL && !GIB), "static epilogue: the plain shared-value form");
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    constexpr int NG = GIB ? 2 : 1;
    const int LD = row_ld<NB>(ld);
    if constexpr (!GIB) {
        const int g0 = col0<NB>();
        r += g0; xout += g0;
        if constexpr (BV != 0) { vals_scaled = shift_bv<BV>(vals_scaled, g0); dinv += g0; }
        if (EPS ? XA : xadd != nullptr) xadd += g0;
        if (EPS ? DOT : dot_with != nullptr) dot_with += g0;
        if (EPS ? PA : padd_x != nullptr) padd_x += g0;
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
      const AT* xa = (EPS ? XA : xadd != nullptr) ? xadd + go : nullptr;
      const double* dw = (EPS ? DOT : dot_with != nullptr) ? dot_with + go : nullptr;
      const PT* px = (EPS ? PA : padd_x != nullptr) ? padd_x + go : nullptr;
      double p[C];
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = 0.0;
      for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        double acc[T][C];
        // static epilogue with a coarse correction: the slice's parent indices are read ahead of the gather loop (T registers),
        // so that xc[parent] is gathered together with the own-row reads and not one round trip behind them
        constexpr bool PAR_AHEAD = EPS && PA;
        int parv[PAR_AHEAD ? T : 1];
        if constexpr (PAR_AHEAD) {
#pragma unroll
            for (int rs = 0; rs < T; ++rs) parv[rs] = padd_idx[min(slice * kWave + rs * G + g, nrows - 1)];
        }
        const int off = slice_off[slice];
        sell_row_range_t<NB, XT, NT, BV, DEEP>(cols, vals_scaled, rg, off, (slice_off[slice + 1] - off) >> 6, lane, LD, acc);
        if constexpr (SPL) split_row_sums<NB, C, T>(acc, sl);
        // row steps in pairs: the own-row reads of both (and the parent indices of the coarse correction) are issued before
        // either is consumed - rows past the end re-read the last row and store nothing
        // (pairs only where the gathers above leave the registers for it - the fp32-gather instantiations; the fp64-gather
        // ones, with sixteen 16-byte gathers in flight, would drop from three to two waves per SIMD)
        // (the static form that adds nothing - pre-smoothing - reads 24 B per lane and row step and takes four at a time: 124
        // registers and four waves per SIMD either way at NB = 32)
        constexpr int H = (T >= 2 && sizeof(XT) == 4) ? ((EPS && !XA && !PA && T >= 4) ? 4 : 2) : 1;
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
                if (EPS ? XA : xa != nullptr) load_v<C>(xa + at[u], x0[u]);
                if constexpr (PAR_AHEAD) par[u] = parv[h0 + u];
                else if (EPS ? PA : padd_idx != nullptr) par[u] = padd_idx[rowc];
                if constexpr (DOT) load_c<C>(dw + at[u], wv[u]);
            }
            if (EPS ? PA : padd_idx != nullptr) {
#pragma unroll
                for (int u = 0; u < H; ++u) load_v<C>(px + (size_t)par[u] * LD + t * C, pc[u]);
            }
#pragma unroll
            for (int u = 0; u < H; ++u) {
                double xv[C];
#pragma unroll
                for (int c = 0; c < C; ++c) xv[c] = di[u][c] * (c0 * rv[u][c] - c1 * acc[h0 + u][c]);
                if (EPS ? XA : xa != nullptr) {
#pragma unroll
                    for (int c = 0; c < C; ++c) xv[c] += x0[u][c];
                }
                if (EPS ? PA : padd_idx != nullptr) {
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
// ROWS AHEAD (vc_rows_ahead: the 32-wide shared-value forms with an fp32 gathered vector and an fp32 r, not row-split, not
// deep, no groups of 8 - the finest levels of a cycle): a wavefront handles one slice and its life was a chain - slice_off, the
// first (index, value) pair, the gather columns, and only then the own rows of r in two batches of four row steps, two more
// round trips with nothing else in flight.  The own rows depend on nothing the gather loop produces: they are requested BEFORE
// the loop (rows past the end re-read the last row and store nothing) and pinned as one point of use behind it - all T row
// steps (32 registers) in the plain forms, T / 2 ahead and T / 2 behind the loop with RAGG, where all T spill.  With RAGG the
// slice's segment range and the lane group's first (position, coarse row) pair travel with them, so that behind the wave
// barrier only LDS reads and the coarse store remain.  The in-place form (TAG 1, r == y) keeps every load of a slice ahead
// of that slice's stores; a wavefront owns its rows.  Same operations in the same order (LAB_NOTES 10.32).
#ifndef PMC_RES_ROWS_AHEAD
#define PMC_RES_ROWS_AHEAD 1   // laboratory macro: 0 = the own rows behind the gather loop, as every other form reads them
#endif
#ifndef PMC_RES_SEG_AHEAD
#define PMC_RES_SEG_AHEAD 1    // laboratory macro: 0 = the segment tables behind the wave barrier
#endif
template <int NB, typename XT, typename RT, bool R8, int BV, int DEEP, bool SPL>
constexpr bool vc_rows_ahead() {
    return PMC_RES_ROWS_AHEAD != 0 && NB == kGroup && sizeof(XT) == 4 && sizeof(RT) == 4 && !R8 && BV == 0 && DEEP == 1 && !SPL;
}
// (0: no occupancy request, as before; the forms with 32 more registers in flight are held to three waves per SIMD)
template <int NB, typename XT, typename RT, bool R8, int BV, int DEEP, bool SPL>
constexpr int vc_res_min_waves() {
    return vc_rows_ahead<NB, XT, RT, R8, BV, DEEP, SPL>() ? 3 : 0;
}
__device__ __forceinline__ void pin_rows(pmc_f4 (&q)[8]) {
    asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]));
}
__device__ __forceinline__ void pin_rows(pmc_f4 (&q)[4]) { asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3])); }
__device__ __forceinline__ void pin_rows(pmc_f4 (&)[1]) {}
template <int NB, typename XT, typename RT, typename YT, bool R8, int BV = 0, bool STORE = true, int DEEP = 1, bool RAGG = false,
          bool SPL = false, typename CT = double, int TAG = 0>
__global__ __launch_bounds__(kBlock, (vc_res_min_waves<NB, XT, RT, R8, BV, DEEP, SPL>())) void vc_residual_kernel(int nrows, int nslices, const int* __restrict__ slice_off,
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
    constexpr bool AHEAD = vc_rows_ahead<NB, XT, RT, R8, BV, DEEP, SPL>();
    constexpr bool SEGA = AHEAD && RAGG && PMC_RES_SEG_AHEAD != 0;
    // row steps read ahead: all T; T / 2 with the fused restriction, whose tile addressing and segment pair leave no room for
    // 32 registers at three waves per SIMD (all T: 168 VGPRs and 20-24 B of scratch)
    constexpr int AH = RAGG ? T / 2 : T;
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        double acc[T][C];
        pmc_f4 own[AHEAD ? AH : 1];
        int s0 = 0, s1 = 0, pos0 = 0, cid0 = 0;
        if constexpr (AHEAD) {
#pragma unroll
            for (int u = 0; u < AH; ++u)
                own[u] = *reinterpret_cast<const pmc_f4*>(r + (size_t)min(slice * kWave + u * G + g, nrows - 1) * LD + t * C);
            if constexpr (SEGA) {
                s0 = seg_ptr[slice];
                s1 = seg_ptr[slice + 1];
            }
        }
        const int off = slice_off[slice], width = (slice_off[slice + 1] - off) >> 6;
        if constexpr (SEGA) {
            // (behind the request for slice_off: the segment range's round trip then runs beside that one, not ahead of it)
            if (s0 + g < s1) {
                pos0 = seg_pos[s0 + g];
                cid0 = seg_cid[s0 + g];
            }
        }
        sell_row_range_t<NB, XT, false, BV, DEEP>(cols, vals, x, off, width, lane, LD, acc);
        if constexpr (SPL) split_row_sums<NB, C, T>(acc, sl);
        if constexpr (AHEAD) {
#pragma unroll
            for (int h0 = 0; h0 < T; h0 += AH) {
                if (h0 > 0) {
                    // (the rest, where all T ahead do not fit: one batch, once the rows read ahead are consumed)
#pragma unroll
                    for (int u = 0; u < AH; ++u)
                        own[u] = *reinterpret_cast<const pmc_f4*>(r + (size_t)min(slice * kWave + (h0 + u) * G + g, nrows - 1) * LD + t * C);
                }
                pin_rows(own);
#pragma unroll
                for (int u = 0; u < AH; ++u) {
                    const int rs = h0 + u, row = slice * kWave + rs * G + g;
                    if (row < nrows) {
                        const size_t at = (size_t)row * LD + t * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[rs][c] = (double)own[u][c] - acc[rs][c];
                        if constexpr (STORE) store_v<C>(y + at, acc[rs]);
                        if constexpr (RAGG) {
#pragma unroll
                            for (int c = 0; c < C; ++c) tile[(rs * G + g) * NB + t * C + c] = (float)acc[rs][c];
                        }
                    }
                }
            }
        } else {
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
        }
        if constexpr (RAGG) {
            // the tile is private to this wavefront: its own LDS writes are complete once the wait below has passed
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if constexpr (SEGA) {
                // the first trip's pair was read ahead of the gather loop; later trips (sg += G) load theirs here
                int pos = pos0, cid = cid0;
                for (int sg = s0 + g; sg < s1;) {
                    const int first = pos >> 8, len = pos & 255;
                    double sum[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[c] = 0.0;
                    for (int q = 0; q < len; ++q)
#pragma unroll
                        for (int c = 0; c < C; ++c) sum[c] += (double)tile[(first + q) * NB + t * C + c];
                    store_v<C>(coarse + (size_t)cid * LD + t * C, sum);
                    sg += G;
                    if (sg < s1) {
                        pos = seg_pos[sg];
                        cid = seg_cid[sg];
                    }
                }
            } else {
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

// First stage of a two-stage reduction for launches with many partial blocks: block j of kCompressBlocks sums the input
// blocks j, j + kCompressBlocks, ... (fixed order: deterministic) into out[j][k].
static constexpr int kCompressBlocks = 256;   // dot_capacity() reserves this many blocks ahead of the uncompressed ones
__global__ __launch_bounds__(256) void compress_partials_kernel(const double* __restrict__ in, int nblocks, int nb,
                                                                double* __restrict__ out) {
    __shared__ double lds[256];
    const int k = threadIdx.x % nb, q = threadIdx.x / nb, nq = 256 / reduce_width(nb);
    if (q >= nq) nblocks = 0;   // nb = kGroup: the upper half of the threads adds nothing (see reduce_width)
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

int dot_capacity(int nrows, int nb) {
    // upper bound on the partial blocks (of nb doubles each) any fused dot over nrows rows of a batch of nb writes: slice
    // kernels one block per 4 slices, flat kernels one per kBlock threads, both bounded by dot_grid_bound() - except the
    // block operator's two-stage reduction, which keeps every slice block behind kCompressBlocks compressed ones (k::spmm)
    const size_t slice_blocks = ((size_t)nrows + 63) / 64 / (kBlock / kWave) + 1;
    const size_t flat_blocks = ((size_t)nrows * nb / (nb >= 32 ? 4 : (nb >= 2 ? 2 : 1)) + kBlock - 1) / kBlock;
    const size_t bounded = std::min<size_t>(std::max(slice_blocks, flat_blocks), dot_grid_bound());
    return (int)std::max<size_t>(bounded, kCompressBlocks + slice_blocks) + 2;
}

// ==========================================================================================
// launchers
namespace k {

// How these launchers are built (the dispatch helpers: klaunch.hpp).  Every kernel template above has ONE <<< site.  A kernel
// that several public launchers start (sell_spmm_kernel, vc_poly2_kernel, vc_residual_kernel) has a launch_* function: it
// takes the grid, the matrix view and the operands, fills the matrix arguments from the view and passes an optional operand
// only if the form reads it, nullptr otherwise - a flag and its pointer cannot disagree.  The other kernels are started in
// place by their one launcher, under the same rule.  A public launcher is the checks, the grid, the decision and a call;
// the run-time facts of the decision become template arguments through dispatch_bool / dispatch_values / dispatch_storage /
// dispatch_narrow and PMC_DISPATCH_NB.  The instantiations of the unit are exactly those the dispatches span, so each
// dispatch names the forms that do not exist.

// what one launch of sell_spmm_kernel computes: its MODE, R8, LZ and SM arguments, of which at most one differs from the
// plain product
enum class Spmm {
    product,               // y = A x                                            MODE 0
    accumulate,            // y += A x                                           MODE 1
    residual,              // y = r - A x                                        MODE 2
    residual_restrict8,    // ... with the fused restriction over groups of 8    MODE 2, R8
    residual_samples,      // ... stored sample-major                            MODE 2, SM 1
    residual_samples_exp,  // ... through exp()                                  MODE 2, SM 2
    dot_only,              // <x, A x> alone (first Lanczos pass)                LZ 1
    update,                // the next Lanczos vector from A x, v1 and v0        LZ 2
    update_first,          // ... in the first iteration (v0 = 0)                LZ 3
    product_store32        // y = A x with its fp32 copy                         LZ 4
};
// sell_spmm_kernel's TAG (SellView::tag)
constexpr int kTagNone = 0, kTagOperator = 1, kTagApply = 2;

template <int NB, int BV, Spmm OP, int TAG = kTagNone, bool DOT = false, bool NT = false, bool DL = false, typename XT, typename YT>
static void launch_spmm(hipStream_t st, int nb, dim3 g, const SellView& A, const XT* x, YT* y, const double* r,
                        const typename ident<XT>::type* dot_with, double* partial, const LanczosUpdate* lz = nullptr) {
    constexpr bool RES = OP == Spmm::residual || OP == Spmm::residual_restrict8 || OP == Spmm::residual_samples ||
                         OP == Spmm::residual_samples_exp;
    constexpr int MODE = OP == Spmm::accumulate ? 1 : (RES ? 2 : 0);
    constexpr bool R8 = OP == Spmm::residual_restrict8;
    constexpr int SM = OP == Spmm::residual_samples ? 1 : (OP == Spmm::residual_samples_exp ? 2 : 0);
    constexpr int LZ = OP == Spmm::dot_only ? 1 : OP == Spmm::update ? 2 : OP == Spmm::update_first ? 3 : OP == Spmm::product_store32 ? 4 : 0;
    sell_spmm_kernel<NB, BV, MODE, DOT, TAG, NT, R8, DL, XT, YT, LZ, SM><<<groups_xcd(g, nb), kBlock, 0, st>>>(
        A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, x, y, RES ? r : nullptr, DOT ? dot_with : nullptr,
        DOT || R8 ? partial : nullptr, nb, LZ != 0 ? *lz : LanczosUpdate{});
}

// the operator products: y = A x, y += A x, with a fused dot, and the Lanczos passes of the solver's operator (lz_mode 1 - 3)
template <int NB, int TAG, typename XT>
static void spmm_launch(hipStream_t st, int nb, dim3 g, const SellView& A, const XT* x, double* y, bool accumulate,
                        double* dot_partial, const XT* dot_with, int lz_mode = 0, const LanczosUpdate* lz = nullptr) {
    constexpr bool F32 = !std::is_same<XT, double>::value;   // fp32-stored input: the preconditioned Krylov vectors
    constexpr bool LANCZOS = F32 && TAG == kTagOperator;      // where the Lanczos passes exist (lz_mode != 0 comes with both)
    constexpr bool DL_ROWS = Lay<NB>::T > 1;
    if (!LANCZOS && lz_mode != 0) throw Error(PMC_ERR_INTERNAL, "spmm: Lanczos pass outside the solver's fp32 operator product");
    // <x, Ax> with a diagonal-last matrix: x_i is what the row's last slice column gathers
    const bool dl = TAG == kTagOperator && DL_ROWS && A.diag_last && dot_with == x;
    if constexpr (F32) {
        // the operator products of the solver loop only
        if (A.bv || accumulate) throw Error(PMC_ERR_INTERNAL, "spmm: fp32 input with per-realization values / accumulation");
    }
    // non-temporal streams: the matrix streams of the Lanczos passes are those of the in-loop product (its launch carries the dot)
    const bool nt = !A.bv && TAG != kTagNone && nt_streams(A, NB, lz_mode != 0 || dot_partial != nullptr);
    if (nt) count_solve_path(PMC_COUNT_NT_OPERATOR);
    dispatch_values<!F32>(A, [&](auto bv) {
        constexpr int BV = decltype(bv)::value;
        constexpr bool SHARED = BV == kSharedValues;   // non-temporal and diagonal-last forms: shared values only
        dispatch_bool<SHARED>(nt, [&](auto nt_c) {
            constexpr bool NT = decltype(nt_c)::value;
            if constexpr (LANCZOS) {
                if (lz_mode != 0 && lz_mode != 1) {   // the update passes: 2, and 3 in the first iteration
                    dispatch_bool(lz_mode != 2, [&](auto first) {
                        constexpr Spmm OP = decltype(first)::value ? Spmm::update_first : Spmm::update;
                        launch_spmm<NB, BV, OP, TAG, false, NT>(st, nb, g, A, x, y, nullptr, nullptr, nullptr, lz);
                    });
                    return;
                }
            }
            if (dot_partial || lz_mode == 1) {
                dispatch_bool<SHARED && DL_ROWS>(dl, [&](auto dl_c) {
                    dispatch_bool<LANCZOS>(lz_mode == 1, [&](auto only) {
                        constexpr Spmm OP = decltype(only)::value ? Spmm::dot_only : Spmm::product;
                        launch_spmm<NB, BV, OP, TAG, true, NT, decltype(dl_c)::value>(st, nb, g, A, x, y, nullptr, dot_with, dot_partial, lz);
                    });
                });
                return;
            }
            if constexpr (!F32) {
                if (accumulate) {
                    launch_spmm<NB, BV, Spmm::accumulate, TAG, false, NT>(st, nb, g, A, x, y, nullptr, nullptr, nullptr);
                    return;
                }
            }
            launch_spmm<NB, BV, Spmm::product, TAG, false, NT>(st, nb, g, A, x, y, nullptr, nullptr, nullptr);
        });
    });
}

template <typename XT>
static int spmm_t(hipStream_t st, int nb, const SellView& A, const XT* x, double* y, bool accumulate, double* dot_partial,
                  const XT* dot_with, int lz_mode = 0, const LanczosUpdate* lz = nullptr) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return 0;
    if (dot_partial && !dot_with) throw Error(PMC_ERR_INTERNAL, "spmm: fused dot without its second vector");
    // The block operator keeps one slice per wavefront also with a fused dot (a bounded grid of looping workgroups cost
    // 22 us of 450 at 4.7 M rows); its partial blocks - more than the single-block consumers should read - are first
    // compressed to kCompressBlocks.  They are written behind the compressed ones: dot_capacity() leaves the room.
    const bool two_stage = dot_partial && A.tag != 0 && !A.bv && grid_slices(A.nslices).x > dot_grid_bound();
    const dim3 g = two_stage ? grid_slices(A.nslices) : grid_bounded(grid_slices(A.nslices), dot_partial != nullptr);
    double* kernel_partial = dot_partial;
    if (two_stage) {
        kernel_partial = dot_partial + (size_t)kCompressBlocks * nb;
        count_solve_path(PMC_COUNT_TWO_STAGE_DOT);
    }
    PMC_DISPATCH_NB(nb, {
        if (A.tag == kTagOperator) spmm_launch<NB, kTagOperator, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with, lz_mode, lz);
        else if (A.tag == kTagApply) spmm_launch<NB, kTagApply, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with);
        else spmm_launch<NB, kTagNone, XT>(st, nb, g, A, x, y, accumulate, kernel_partial, dot_with);
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
    return dispatch_storage(x, [&](auto* xp, auto* dw) { return spmm_t(st, nb, A, xp, y, false, dot_partial, dw); }, dot_with);
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
    PMC_DISPATCH_NB(nb, dispatch_values(A, [&](auto bv) {
        launch_spmm<NB, decltype(bv)::value, Spmm::residual_restrict8>(st, nb, g, A, x, out, r, nullptr, coarse);
    }));
    check_launch();
}

void spmm_store32(hipStream_t st, int nb, const SellView& A, const double* x, double* y, float* y32) {
    check_offsets32(A, nb);
    if (A.bv || A.tag != 0 || !y || !y32) throw Error(PMC_ERR_INTERNAL, "spmm_store32: shared values, an untagged matrix, both results");
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    LanczosUpdate lz{};
    lz.y32 = y32;
    PMC_DISPATCH_NB(nb, { launch_spmm<NB, kSharedValues, Spmm::product_store32>(st, nb, g, A, x, y, nullptr, nullptr, nullptr, &lz); });
    check_launch();
}

void residual_samples(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, bool do_exp, double* out) {
    check_offsets32(A, nb);
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "residual_samples: shared values only");
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, dispatch_bool(do_exp, [&](auto e) {
        constexpr Spmm OP = decltype(e)::value ? Spmm::residual_samples_exp : Spmm::residual_samples;
        launch_spmm<NB, kSharedValues, OP>(st, nb, g, A, x, out, r, nullptr, nullptr);
    }));
    check_launch();
}

void residual(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, double* out) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, dispatch_values(A, [&](auto bv) {
        launch_spmm<NB, decltype(bv)::value, Spmm::residual>(st, nb, g, A, x, out, r, nullptr, nullptr);
    }));
    check_launch();
}

template <typename OT>
static int cheb_step_t(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
                       const double* xin, double* d, OT* xout, double a, double b, double* dot_partial) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return 0;
    if (A.bv != dinv_bv) throw Error(PMC_ERR_INTERNAL, "cheb_step: value/diagonal batching mismatch");
    const dim3 g = grid_bounded(grid_slices(A.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, dispatch_values(A, [&](auto bv) {
        dispatch_bool(dot_partial != nullptr, [&](auto dot) {
            constexpr bool DOT = decltype(dot)::value;
            sell_cheb_kernel<NB, decltype(bv)::value, DOT, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(
                A.nrows, A.nslices, A.slice_off, A.sched, A.cols, A.vals, dinv, r, xin, d, xout, a, b, DOT ? dot_partial : nullptr, nb);
        });
    }));
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
    return dispatch_storage(zout, [&](auto* out) { return cheb_step_t(st, nb, A, dinv, dinv_bv, r, xin, d, out, a, b, dot_partial); });
}

template <typename OT>
static int poly2_t(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, OT* xout,
                   double c0, double c1, double* dot_partial, const double* xadd, const double* dot_with, const int* padd_idx,
                   const double* padd_x) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return 0;
    if (As.bv != dinv_bv) throw Error(PMC_ERR_INTERNAL, "poly2: value/diagonal batching mismatch");
    const dim3 g = grid_bounded(grid_slices(As.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, dispatch_values(As, [&](auto bv) {
        constexpr int BV = decltype(bv)::value;
        constexpr bool SHARED = BV == kSharedValues;   // the non-temporal form: shared values only
        const bool nt = SHARED && nt_poly(As, NB);
        if (nt) count_solve_path(PMC_COUNT_NT_POLY);
        dispatch_bool<SHARED>(nt, [&](auto nt_c) {
            dispatch_bool(dot_partial != nullptr, [&](auto dot) {
                constexpr bool DOT = decltype(dot)::value;
                sell_poly2_kernel<NB, BV, DOT, decltype(nt_c)::value, OT><<<groups_xcd(g, nb), kBlock, 0, st>>>(
                    As.nrows, As.nslices, As.slice_off, As.sched, As.cols, As.vals, dinv, r, xout, c0, c1,
                    DOT ? dot_partial : nullptr, xadd, dot_with, padd_idx, padd_x, nb);
            });
        });
    }));
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
    return dispatch_storage(xout, [&](auto* out) {
        return poly2_t(st, nb, As, dinv, dinv_bv, r, out, c0, c1, dot_partial, xadd, dot_with, padd_idx, padd_x);
    });
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

// how a V-cycle kernel walks a level: its NT, DEEP, SPL and GIB arguments, of which at most one path is taken
enum class Walk {
    lean,        // the lean gather loop
    lean_nt,     // ... with non-temporal matrix / result streams                                   NT
    deep2,       // sell_row_range_deep, 2 slice columns per trip (small 32-wide levels)            DEEP 2
    deep4,       // ... 4 slice columns per trip                                                    DEEP 4
    split,       // rows stored as 2^split_log2 pieces: narrow launches, grid and row count differ  SPL
    both_groups  // both column groups of a 64-wide launch in one workgroup, non-temporal           GIB, NT
};
template <Walk W>
struct WalkArgs {
    static constexpr bool NT = W == Walk::lean_nt || W == Walk::both_groups;
    static constexpr int DEEP = W == Walk::deep2 ? 2 : (W == Walk::deep4 ? 4 : 1);
    static constexpr bool SPL = W == Walk::split, GIB = W == Walk::both_groups;
    // the row-split and the two-group forms carry the column groups inside the workgroup
    static dim3 grid(dim3 g, int nb) { return SPL || GIB ? g : groups_xcd(g, nb); }
    static int nrows(const SellView& A) { return SPL ? A.nrows >> A.split_log2 : A.nrows; }
    static int sl(const SellView& A) { return SPL ? A.split_log2 : 0; }
};

// the epilogue of vc_poly2_kernel (EPS, XA, PA): operands found at run time by their pointers, or known at compile time
enum class Epilogue {
    dynamic,  // xadd / the coarse correction are added where their pointers are set
    nothing,  // compile time: nothing is added (pre-smoothing)                       EPS
    full      // compile time: the iterate and the coarse correction are added        EPS, XA, PA
};

// xadd is the level's fp32 iterate; a launch without coarse correction passes a typed null (PT = double)
template <int NB, Walk W, bool DOT, int BV = kSharedValues, Epilogue E = Epilogue::dynamic, typename XT, typename OT, typename PT>
static void launch_vc_poly2(hipStream_t st, int nb, dim3 g, const SellView& As, const double* dinv, const XT* r, OT* xout,
                            double c0, double c1, double* partial, const float* xadd, const double* dot_with,
                            const int* padd_idx, const PT* padd_x) {
    using WA = WalkArgs<W>;
    constexpr bool EPS = E != Epilogue::dynamic, ADD = E != Epilogue::nothing;
    vc_poly2_kernel<NB, XT, OT, float, DOT, WA::NT, BV, WA::DEEP, WA::SPL, WA::GIB, PT, EPS, EPS && ADD, EPS && ADD>
        <<<WA::grid(g, nb), kBlock, 0, st>>>(
        WA::nrows(As), As.nslices, As.slice_off, As.cols, As.vals, dinv, r, xout, c0, c1, DOT ? partial : nullptr,
        ADD ? xadd : nullptr, DOT ? dot_with : nullptr, ADD ? padd_idx : nullptr, ADD ? padd_x : nullptr, nb, WA::sl(As));
}
constexpr const double* kNoCoarse = nullptr;

// what leaves vc_residual_kernel besides (or instead of) the residual: its R8, STORE and RAGG arguments
enum class Restrict {
    none,         // the residual alone
    groups8,      // ... and its sums over groups of 8 consecutive rows                    R8
    groups8_only, // the sums alone, the residual is not stored                            R8, no STORE
    aggregates    // ... and its sums over the aggregates of the segment tables            RAGG
};

// IN_PLACE (the kernel's TAG 1): r == y, the correction of a residual by the coarse iterate
template <int NB, Walk W, Restrict R, int BV = kSharedValues, bool IN_PLACE = false, typename XT, typename RT, typename CT>
static void launch_vc_residual(hipStream_t st, int nb, dim3 g, const SellView& A, const XT* x, const RT* r, float* y, CT* coarse,
                               const int* seg_ptr = nullptr, const int* seg_cid = nullptr, const int* seg_pos = nullptr) {
    using WA = WalkArgs<W>;
    static_assert(!WA::NT && !WA::GIB, "the residual kernels have no non-temporal and no two-group form");
    constexpr bool R8 = R == Restrict::groups8 || R == Restrict::groups8_only, RAGG = R == Restrict::aggregates;
    constexpr bool STORE = R != Restrict::groups8_only;
    vc_residual_kernel<NB, XT, RT, float, R8, BV, STORE, WA::DEEP, RAGG, WA::SPL, CT, IN_PLACE ? 1 : 0>
        <<<WA::grid(g, nb), kBlock, 0, st>>>(
        WA::nrows(A), A.nslices, A.slice_off, A.cols, A.vals, x, r, STORE ? y : nullptr, R8 || RAGG ? coarse : nullptr, nb,
        RAGG ? seg_ptr : nullptr, RAGG ? seg_cid : nullptr, RAGG ? seg_pos : nullptr, WA::sl(A));
}
constexpr double* kNoRestriction = nullptr;

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
        dispatch_narrow(nb, [&](auto w) {
            launch_vc_poly2<decltype(w)::value, Walk::split, false>(st, nb, g, As, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, kNoCoarse);
        });
    } else if (deep_level(As, nb)) {
        launch_vc_poly2<kGroup, Walk::deep2, false>(st, nb, g, As, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, kNoCoarse);
    } else PMC_DISPATCH_NB(nb, {
        // (the 32-wide fp32 forms - the finest level of a cycle - know at compile time that the epilogue adds nothing)
        constexpr Epilogue E = NB == kGroup && sizeof(RT) == 4 ? Epilogue::nothing : Epilogue::dynamic;
        const bool nt = nt_poly(As, NB);
        if (nt) count_solve_path(PMC_COUNT_NT_POLY);
        dispatch_bool(nt, [&](auto nt_c) {
            constexpr Walk W = decltype(nt_c)::value ? Walk::lean_nt : Walk::lean;
            launch_vc_poly2<NB, W, false, kSharedValues, E>(st, nb, g, As, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, kNoCoarse);
        });
    });
    check_launch();
}
void vc_presmooth32(hipStream_t st, int nb, const SellView& As, const double* dinv, zvec r, float* xout, double c0, double c1) {
    dispatch_storage(r, [&](auto* rp) { vc_presmooth32_t(st, nb, As, dinv, rp, xout, c0, c1); });
}

void vc_residual_restrict8_32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv || A.nrows % 8 != 0) throw Error(PMC_ERR_INTERNAL, "vc_residual_restrict8_32: shared values and groups of 8 rows expected");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, dispatch_storage(r, [&](auto* rp) {
        dispatch_storage(coarse, [&](auto* cp) { launch_vc_residual<NB, Walk::lean, Restrict::groups8>(st, nb, g, A, x, rp, out, cp); });
    }));
    check_launch();
}

template <typename RT>
static void vc_residual32_t(hipStream_t st, int nb, const SellView& A, const RT* r, const float* x, float* out) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual32: shared values expected");
    const dim3 g = grid_slices(A.nslices);
    if (A.split_log2) {
        dispatch_narrow(nb, [&](auto w) {
            launch_vc_residual<decltype(w)::value, Walk::split, Restrict::none>(st, nb, g, A, x, r, out, kNoRestriction);
        });
    } else if (deep_level(A, nb)) {
        launch_vc_residual<kGroup, Walk::deep4, Restrict::none>(st, nb, g, A, x, r, out, kNoRestriction);
    } else PMC_DISPATCH_NB(nb, { launch_vc_residual<NB, Walk::lean, Restrict::none>(st, nb, g, A, x, r, out, kNoRestriction); });
    check_launch();
}
void vc_residual32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out) {
    dispatch_storage(r, [&](auto* rp) { vc_residual32_t(st, nb, A, rp, x, out); });
}

void vc_residual_restrict_agg32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse,
                                const int* seg_ptr, const int* seg_cid, const int* seg_pos) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (A.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual_restrict_agg32: shared values expected");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, dispatch_storage(r, [&](auto* rp) {
        dispatch_storage(coarse, [&](auto* cp) {
            launch_vc_residual<NB, Walk::lean, Restrict::aggregates>(st, nb, g, A, x, rp, out, cp, seg_ptr, seg_cid, seg_pos);
        });
    }));
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
    PMC_DISPATCH_NB(nb, { launch_spmm<NB, kSharedValues, Spmm::product>(st, nb, g, Pt, res, coarse.as<float>(), nullptr, nullptr, nullptr); });
    check_launch();
}

template <typename XT>
static void vc_residual_coarse32_t(hipStream_t st, int nb, const SellView& SP, float* res, const XT* xc) {
    check_offsets32(SP, nb);
    if (SP.nrows == 0) return;
    if (SP.bv) throw Error(PMC_ERR_INTERNAL, "vc_residual_coarse32: shared values expected");
    const dim3 g = grid_slices(SP.nslices);
    constexpr bool IN_PLACE = true;   // res -= SP xc
    if (SP.split_log2) {
        dispatch_narrow(nb, [&](auto w) {
            launch_vc_residual<decltype(w)::value, Walk::split, Restrict::none, kSharedValues, IN_PLACE>(st, nb, g, SP, xc, res, res, kNoRestriction);
        });
    } else if (deep_level(SP, nb)) {
        launch_vc_residual<kGroup, Walk::deep2, Restrict::none, kSharedValues, IN_PLACE>(st, nb, g, SP, xc, res, res, kNoRestriction);
    } else PMC_DISPATCH_NB(nb, { launch_vc_residual<NB, Walk::lean, Restrict::none, kSharedValues, IN_PLACE>(st, nb, g, SP, xc, res, res, kNoRestriction); });
    check_launch();
}
void vc_residual_coarse32(hipStream_t st, int nb, const SellView& SP, float* res, zvec xc) {
    dispatch_storage(xc, [&](auto* xp) { vc_residual_coarse32_t(st, nb, SP, res, xp); });
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
        dispatch_narrow(nb, [&](auto w) {
            launch_vc_poly2<decltype(w)::value, Walk::split, false>(st, nb, g, As, dinv, res, xout, c0, c1, nullptr, x, nullptr, parent, xc);
        });
        check_launch();
        return 0;
    }
    if (deep_level(As, nb)) {
        dispatch_bool(dot_partial != nullptr, [&](auto dot) {
            launch_vc_poly2<kGroup, Walk::deep4, decltype(dot)::value>(st, nb, g, As, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc);
        });
        check_launch();
        return dot_partial ? dot_blocks(g, nb) : 0;
    }
    // 64 per launch on a large level: both column groups of a slice in one workgroup (vc_poly2_kernel, GIB).  Off in the
    // product: one lane 2 870 -> 2 815 samples/s, four lanes 3 745 -> 3 757 (LAB_NOTES 10.19); laboratory switch PMC_GIB=1
    static const bool gib = [] { const char* e = lab_env("PMC_GIB"); return e && atoi(e) != 0; }();
    if (gib && nb == 2 * kGroup && nt_poly(As, kGroup) && !xcd_layout(g, nb)) {
        count_solve_path(PMC_COUNT_NT_POLY);
        dispatch_bool(dot_partial != nullptr, [&](auto dot) {
            launch_vc_poly2<kGroup, Walk::both_groups, decltype(dot)::value>(st, nb, g, As, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc);
        });
        check_launch();
        return dot_partial ? (int)g.x : 0;
    }
    // (the 32-wide forms - the finest level of a cycle - know their epilogue at compile time: the iterate and the coarse
    // correction are added, the dot is taken with r iff there is one)
    if (!x || !parent || !xc || (dot_partial && !r))
        throw Error(PMC_ERR_INTERNAL, "vc_postsmooth32: iterate, parent table, coarse correction and the dot's vector expected");
    PMC_DISPATCH_NB(nb, {
        constexpr Epilogue E = NB == kGroup ? Epilogue::full : Epilogue::dynamic;
        const bool nt = nt_poly(As, NB);
        if (nt) count_solve_path(PMC_COUNT_NT_POLY);
        dispatch_bool(nt, [&](auto nt_c) {
            dispatch_bool(dot_partial != nullptr, [&](auto dot) {
                constexpr Walk W = decltype(nt_c)::value ? Walk::lean_nt : Walk::lean;
                launch_vc_poly2<NB, W, decltype(dot)::value, kSharedValues, E>(st, nb, g, As, dinv, res, xout, c0, c1, dot_partial, x, r, parent, xc);
            });
        });
    });
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int vc_postsmooth32_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                      zvec xout, double c0, double c1, const double* r, const int* parent, zvec xc, double* dot_partial) {
    return dispatch_storage(xout, [&](auto* out) {
        return dispatch_storage(xc, [&](auto* xp) {
            return vc_postsmooth32_t(st, nb, As, dinv, res, x, out, c0, c1, r, parent, xp, dot_partial);
        });
    });
}

// ---- the same level with per-realization fp32 values (Darcy; SellView::f32) and per-realization diagonals
void vc_presmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const double* r, float* xout, double c0,
                       double c1) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return;
    if (!(As.bv && As.f32)) throw Error(PMC_ERR_INTERNAL, "vc_presmooth32_bv: per-realization fp32 values expected");
    const dim3 g = grid_slices(As.nslices);
    PMC_DISPATCH_NB(nb, {
        launch_vc_poly2<NB, Walk::lean, false, kValues32>(st, nb, g, As, dinv, r, xout, c0, c1, nullptr, nullptr, nullptr, nullptr, kNoCoarse);
    });
    check_launch();
}

void vc_restrict8_32_bv(hipStream_t st, int nb, const SellView& A, const double* r, const float* x, double* coarse) {
    check_offsets32(A, nb);
    if (A.nrows == 0) return;
    if (!(A.bv && A.f32) || A.nrows % 8 != 0) throw Error(PMC_ERR_INTERNAL, "vc_restrict8_32_bv: operand mismatch");
    const dim3 g = grid_slices(A.nslices);
    PMC_DISPATCH_NB(nb, { launch_vc_residual<NB, Walk::lean, Restrict::groups8_only, kValues32>(st, nb, g, A, x, r, nullptr, coarse); });
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
    PMC_DISPATCH_NB(nb, { launch_vc_residual<NB, Walk::lean, Restrict::none, kValues32>(st, nb, g, A, x, r, out, kNoRestriction); });
    check_launch();
}

template <typename OT>
static int vc_postsmooth32_bv_t(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                                OT* xout, double c0, double c1, const double* r, double* dot_partial) {
    check_offsets32(As, nb);
    if (As.nrows == 0) return 0;
    if (!(As.bv && As.f32)) throw Error(PMC_ERR_INTERNAL, "vc_postsmooth32_bv: per-realization fp32 values expected");
    const dim3 g = grid_bounded(grid_slices(As.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, dispatch_bool(dot_partial != nullptr, [&](auto dot) {
        launch_vc_poly2<NB, Walk::lean, decltype(dot)::value, kValues32>(st, nb, g, As, dinv, res, xout, c0, c1, dot_partial, x, r, nullptr, kNoCoarse);
    }));
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int vc_postsmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                       double* xout, double c0, double c1, const double* r, double* dot_partial) {
    return vc_postsmooth32_bv_t<double>(st, nb, As, dinv, res, x, xout, c0, c1, r, dot_partial);
}
int vc_postsmooth32_bv_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                         zvec xout, double c0, double c1, const double* r, double* dot_partial) {
    return dispatch_storage(xout, [&](auto* out) { return vc_postsmooth32_bv_t(st, nb, As, dinv, res, x, out, c0, c1, r, dot_partial); });
}

template <typename XT>
static int pair_spmm_t(hipStream_t st, int nb, const SellView& A1, const XT* x1, const SellView& A2, const XT* x2, double* y,
                       double* dot_partial, const XT* dot_with) {
    check_offsets32(A1, nb);
    if (A1.nrows == 0) return 0;
    if (!A1.bv || A2.bv || A1.nrows != A2.nrows || A1.nslices != A2.nslices)
        throw Error(PMC_ERR_INTERNAL, "pair_spmm: operand mismatch");
    const dim3 g = grid_bounded(grid_slices(A1.nslices), dot_partial != nullptr);
    PMC_DISPATCH_NB(nb, dispatch_bool(dot_partial != nullptr, [&](auto dot) {
        constexpr bool DOT = decltype(dot)::value;
        sell_pair_spmm_kernel<NB, DOT, XT><<<groups_xcd(g, nb), kBlock, 0, st>>>(
            A1.nrows, A1.nslices, A1.slice_off, A1.cols, A1.vals, A2.slice_off, A2.cols, A2.vals, x1, x2, y,
            DOT ? dot_with : nullptr, DOT ? dot_partial : nullptr, nb);
    }));
    check_launch();
    return dot_partial ? dot_blocks(g, nb) : 0;
}

int pair_spmm_z(hipStream_t st, int nb, const SellView& A1, zvec x1, const SellView& A2, zvec x2, double* y,
                double* dot_partial, zvec dot_with) {
    return dispatch_storage(x1, [&](auto* p1, auto* p2, auto* dw) { return pair_spmm_t(st, nb, A1, p1, A2, p2, y, dot_partial, dw); }, x2, dot_with);
}

}  // namespace k
}  // namespace pmc

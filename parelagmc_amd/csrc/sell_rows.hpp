// The SELL-64 gather loops: what a wavefront does with one slice.  Every kernel that multiplies by a SELL-64 matrix goes
// through one of
//   sell_row_range       all row steps of a slice, `width` slice columns         (operator, smoothers, V-cycle levels)
//   sell_row_range_deep  the same with J slice columns per trip, NB = 32         (V-cycle levels too small to fill the chip)
//   sell_row_range_t     picks one of the two above by its DEEP argument         (V-cycle kernels)
//   sell_row_part        TH row steps of a slice only                            (element-grouped Darcy kernels)
#pragma once
#include "kdev.hpp"

namespace pmc {

// ------------------------------------------------------------------------------------------
// SELL-64 sparse matrix times interleaved multi-vector.  One wavefront per 64-row slice.  Every lane
// loads the value / column of "its" row for slice column j (one fully coalesced 512 B + 256 B access
// per wavefront), then the wavefront sweeps the slice in T steps of G rows: lane (g, t) takes row
// rs*G+g and the 16 B column pair t, fetching that row's value / column index with a cross-lane
// shuffle, so each x gather and each y store is one contiguous NB*8-byte segment per row.
// sell_row_range works on `width` slice columns starting at slot `off`.  CS: every gathered x[col] is multiplied by a
// second gathered per-realization vector cs[col] (column scaling A D^-1 without stored scaled values).  ZERO: acc is
// cleared first, otherwise accumulated into.
// xlast (optional): receives the x rows gathered by the LAST slice column.  A matrix built diagonal-last (Sell::diag_last:
// every row ends with its diagonal entry and is padded with zero-weight copies of it) gathers x[row] there, so a fused
// <x, Ax> needs no second read of x - which by the end of a slice has long left the L2 (measured at 0.6 M rows: 25 MB of
// 280 MB per launch).
template <int NB>
__device__ __forceinline__ constexpr bool lean_range() {
    return Lay<NB>::T > 1 && NB >= kLeanRangeMinNb;
}
template <int NB, int BV, bool CS, bool ZERO, bool NT = false, typename XT = double>
__device__ __forceinline__ void sell_row_range(const int* __restrict__ cols, const double* __restrict__ vals,
                                               const XT* __restrict__ x, const double* __restrict__ cs, int off,
                                               int width, int lane, int LD, double (&acc)[Lay<NB>::T][Lay<NB>::C],
                                               double (*xlast)[Lay<NB>::C] = nullptr, double* pdot = nullptr) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int g = lane / T, t = lane % T;
    if constexpr (ZERO) {
#pragma unroll
        for (int rs = 0; rs < T; ++rs)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[rs][c] = 0.0;
    }
    int slot = off + lane;

    if constexpr (T == 1) {
        // one lane per row (NB = 1, 2): take JU slice columns at a time so that JU (index, value) pairs and then
        // JU gathers are in flight together instead of one dependent chain per column
        constexpr int JU = 4;
        for (int j = 0; j < width; j += JU, slot += JU * kWave) {
            int cc[JU];
            double aa[JU];
#pragma unroll
            for (int u = 0; u < JU; ++u) {
                const bool ok = j + u < width;
                const int at = ok ? slot + u * kWave : slot;   // out-of-range columns re-read column j, weight 0
                cc[u] = cols[at];
                if constexpr (BV) aa[u] = ok ? 1.0 : 0.0;
                else aa[u] = ok ? vals[at] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
            double xv[JU][C], av[JU][C], sv[JU][C];
#pragma unroll
            for (int u = 0; u < JU; ++u) {
                load_v<C>(x + (size_t)cc[u] * LD, xv[u]);
                if constexpr (CS) load_c<C>(cs + (size_t)cc[u] * LD, sv[u]);
                if constexpr (BV) load_bv<BV, C>(vals, (size_t)(j + u < width ? slot + u * kWave : slot) * LD, av[u]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < JU; ++u)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if constexpr (CS) xv[u][c] *= sv[u][c];
                    if constexpr (BV) acc[0][c] = fma(aa[u] * av[u][c], xv[u][c], acc[0][c]);
                    else acc[0][c] = fma(aa[u], xv[u][c], acc[0][c]);
                }
        }
        return;
    }

    int cj = 0;
    double vj = 0.0;
    if (width > 0) {
        cj = load_stream<NT>(cols + slot);
        if constexpr (!BV) vj = load_stream<NT>(vals + slot);
    }
    if constexpr (lean_range<NB>()) {
        // lean loop (as sell_row_part): 32-bit element offsets, gathered rows and fp32 per-realization values stay in their
        // storage type until the FMA, shared values are fetched across lanes after the gathers have been issued; with pdot
        // the fused <x, A x> of a diagonal-last matrix is taken right at the row's last column (rows past the end carry
        // zero values)
        for (int j = 0; j < width; ++j, slot += kWave) {
            int cn = cj;
            double vn = vj;
            if (j + 1 < width) {
                cn = load_stream<NT>(cols + slot + kWave);
                if constexpr (!BV) vn = load_stream<NT>(vals + slot + kWave);
            }
            unsigned at[T];
#pragma unroll
            for (int rs = 0; rs < T; ++rs) at[rs] = (unsigned)__shfl(cj, rs * G + g, kWave) * (unsigned)LD + (unsigned)(t * C);
            RawVec<XT, C> xr[T];
            RawVec<float, C> avf[BV == 2 ? T : 1];
            double avd[BV == 1 ? T : 1][C];
            double sv[CS ? T : 1][C];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rs = 0; rs < T; ++rs) {
                load_raw<C>(x + at[rs], xr[rs]);
                if constexpr (CS) load_c<C>(cs + at[rs], sv[rs]);
                if constexpr (BV == 2)
                    load_raw<C>(reinterpret_cast<const float*>(vals) + ((size_t)(slot - lane + rs * G + g) * LD + t * C), avf[rs]);
                if constexpr (BV == 1) load_c<C>(vals + ((size_t)(slot - lane + rs * G + g) * LD + t * C), avd[rs]);
            }
            if (!pdot && !xlast) pin_gathers(xr);   // (with pdot / xlast the values live past the FMAs and stay grouped)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rs = 0; rs < T; ++rs) {
                double a = 0.0;
                if constexpr (!BV) a = __shfl(vj, rs * G + g, kWave);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    double xv = (double)xr[rs].v[c];
                    if constexpr (CS) xv *= sv[rs][c];
                    if constexpr (BV == 2) acc[rs][c] = fma((double)avf[rs].v[c], xv, acc[rs][c]);
                    else if constexpr (BV == 1) acc[rs][c] = fma(avd[rs][c], xv, acc[rs][c]);
                    else acc[rs][c] = fma(a, xv, acc[rs][c]);
                }
            }
            if (j + 1 == width) {
                if (pdot) {
#pragma unroll
                    for (int rs = 0; rs < T; ++rs)
#pragma unroll
                        for (int c = 0; c < C; ++c) pdot[c] = fma((double)xr[rs].v[c], acc[rs][c], pdot[c]);
                } else if (xlast) {
#pragma unroll
                    for (int rs = 0; rs < T; ++rs)
#pragma unroll
                        for (int c = 0; c < C; ++c) xlast[rs][c] = (double)xr[rs].v[c];
                }
            }
            cj = cn;
            vj = vn;
        }
        return;
    }
    for (int j = 0; j < width; ++j, slot += kWave) {
        // software pipeline: the next slice column's (value, index) pair is requested before this
        // column's gathers, so its latency overlaps them
        int cn = cj;
        double vn = vj;
        if (j + 1 < width) {
            cn = load_stream<NT>(cols + slot + kWave);
            if constexpr (!BV) vn = load_stream<NT>(vals + slot + kWave);
        }
        // phase 1: all cross-lane fetches, phase 2: all gathers (independent registers, so the T loads of a
        // slice column are in flight together), phase 3: FMAs
        int cc[T];
        double aa[T];
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            const int src = rs * G + g;
            cc[rs] = (T == 1) ? cj : __shfl(cj, src, kWave);
            if constexpr (!BV) aa[rs] = (T == 1) ? vj : __shfl(vj, src, kWave);
        }
        double xv[T][C];
        double av[T][C];
        double sv[T][C];
        if constexpr (T > 1) __builtin_amdgcn_sched_barrier(0);   // hipcc otherwise re-serialises load -> wait -> fma
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
            load_v<C>(x + (size_t)cc[rs] * LD + t * C, xv[rs]);
            if constexpr (CS) load_c<C>(cs + (size_t)cc[rs] * LD + t * C, sv[rs]);
            if constexpr (BV) load_bv<BV, C>(vals, (size_t)(slot - lane + rs * G + g) * LD + t * C, av[rs]);
        }
        if constexpr (T > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rs = 0; rs < T; ++rs) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if constexpr (CS) xv[rs][c] *= sv[rs][c];
                if constexpr (BV) acc[rs][c] = fma(av[rs][c], xv[rs][c], acc[rs][c]);
                else acc[rs][c] = fma(aa[rs], xv[rs][c], acc[rs][c]);
            }
        }
        if (xlast && j + 1 == width) {
#pragma unroll
            for (int rs = 0; rs < T; ++rs)
#pragma unroll
                for (int c = 0; c < C; ++c) xlast[rs][c] = xv[rs][c];
        }
        cj = cn;
        vj = vn;
    }
}

// DEEP gather loop for levels too small to fill the chip (NB = 32, shared values): J slice columns - J x 8 gathers per lane -
// are in flight together.  A launch of a few hundred to a few thousand wavefronts (one per 64-row slice) runs less than one
// wavefront per SIMD; each walks its slice's columns as a chain of dependent round trips to L2, so the launch lasts
// `slice width` x latency whatever its size (round 5: the five V-cycle kernels of the 4 964-row level of the hybridized
// hierarchy - 78 wavefronts, 17-27 columns - took ~38 us each, those of the 43 622-row level ~30 us).  With J columns per
// trip the chain is J times shorter; registers (J x 32 for the raw fp32 rows) are no concern at that occupancy.  Same FMA
// order per accumulator as the one-column loop (column after column), out-of-range columns re-read the last column with
// weight zero: bit-identical results.
typedef float pmc_f4x __attribute__((ext_vector_type(4)));
template <int J>
__device__ __forceinline__ void pin_deep(pmc_f4x (&q)[J][8]) {
    if constexpr (J == 2)
        asm volatile("" : "+v"(q[0][0]), "+v"(q[0][1]), "+v"(q[0][2]), "+v"(q[0][3]), "+v"(q[0][4]), "+v"(q[0][5]), "+v"(q[0][6]),
                     "+v"(q[0][7]), "+v"(q[1][0]), "+v"(q[1][1]), "+v"(q[1][2]), "+v"(q[1][3]), "+v"(q[1][4]), "+v"(q[1][5]),
                     "+v"(q[1][6]), "+v"(q[1][7]));
    else if constexpr (J == 4)
        asm volatile("" : "+v"(q[0][0]), "+v"(q[0][1]), "+v"(q[0][2]), "+v"(q[0][3]), "+v"(q[0][4]), "+v"(q[0][5]), "+v"(q[0][6]),
                     "+v"(q[0][7]), "+v"(q[1][0]), "+v"(q[1][1]), "+v"(q[1][2]), "+v"(q[1][3]), "+v"(q[1][4]), "+v"(q[1][5]),
                     "+v"(q[1][6]), "+v"(q[1][7]), "+v"(q[2][0]), "+v"(q[2][1]), "+v"(q[2][2]), "+v"(q[2][3]), "+v"(q[2][4]),
                     "+v"(q[2][5]), "+v"(q[2][6]), "+v"(q[2][7]), "+v"(q[3][0]), "+v"(q[3][1]), "+v"(q[3][2]), "+v"(q[3][3]),
                     "+v"(q[3][4]), "+v"(q[3][5]), "+v"(q[3][6]), "+v"(q[3][7]));
}
typedef double pmc_d2x __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pin_deep_d(pmc_d2x (&q)[2][8][2]) {
    asm volatile("" : "+v"(q[0][0][0]), "+v"(q[0][0][1]), "+v"(q[0][1][0]), "+v"(q[0][1][1]), "+v"(q[0][2][0]), "+v"(q[0][2][1]),
                 "+v"(q[0][3][0]), "+v"(q[0][3][1]), "+v"(q[0][4][0]), "+v"(q[0][4][1]), "+v"(q[0][5][0]), "+v"(q[0][5][1]),
                 "+v"(q[0][6][0]), "+v"(q[0][6][1]), "+v"(q[0][7][0]), "+v"(q[0][7][1]), "+v"(q[1][0][0]), "+v"(q[1][0][1]),
                 "+v"(q[1][1][0]), "+v"(q[1][1][1]), "+v"(q[1][2][0]), "+v"(q[1][2][1]), "+v"(q[1][3][0]), "+v"(q[1][3][1]),
                 "+v"(q[1][4][0]), "+v"(q[1][4][1]), "+v"(q[1][5][0]), "+v"(q[1][5][1]), "+v"(q[1][6][0]), "+v"(q[1][6][1]),
                 "+v"(q[1][7][0]), "+v"(q[1][7][1]));
}
template <int NB, typename XT, int J>
__device__ __forceinline__ void sell_row_range_deep(const int* __restrict__ cols, const double* __restrict__ vals,
                                                    const XT* __restrict__ x, int off, int width, int lane, int LD,
                                                    double (&acc)[Lay<NB>::T][Lay<NB>::C]) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    static_assert(C == 4 && T == 8, "the deep loop is written for the 32-wide layout");
    static_assert((sizeof(XT) == 4 && (J == 2 || J == 4)) || (sizeof(XT) == 8 && J == 2), "columns per trip");
    const int g = lane / T, t = lane % T;
#pragma unroll
    for (int rs = 0; rs < T; ++rs)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[rs][c] = 0.0;
    int slot = off + lane;
    int cj[J];
    double vj[J];
#pragma unroll
    for (int u = 0; u < J; ++u) {
        const bool ok = u < width;
        const int at = ok ? slot + u * kWave : slot;
        cj[u] = width > 0 ? cols[at] : 0;
        vj[u] = (ok && width > 0) ? vals[at] : 0.0;
    }
    for (int j = 0; j < width; j += J, slot += J * kWave) {
        int cn[J];
        double vn[J];
#pragma unroll
        for (int u = 0; u < J; ++u) {   // the next trip's (index, value) pairs: requested before this trip's gathers
            const bool ok = j + J + u < width;
            const int at = ok ? slot + (J + u) * kWave : slot;
            cn[u] = cols[at];
            vn[u] = ok ? vals[at] : 0.0;
        }
        unsigned at[J][T];
#pragma unroll
        for (int u = 0; u < J; ++u)
#pragma unroll
            for (int rs = 0; rs < T; ++rs) at[u][rs] = (unsigned)__shfl(cj[u], rs * G + g, kWave) * (unsigned)LD + (unsigned)(t * C);
        if constexpr (sizeof(XT) == 4) {
            pmc_f4x q[J][8];
#pragma unroll
            for (int u = 0; u < J; ++u)
#pragma unroll
                for (int rs = 0; rs < T; ++rs) q[u][rs] = *reinterpret_cast<const pmc_f4x*>(x + at[u][rs]);
            pin_deep<J>(q);
#pragma unroll
            for (int u = 0; u < J; ++u)
#pragma unroll
                for (int rs = 0; rs < T; ++rs) {
                    const double a = __shfl(vj[u], rs * G + g, kWave);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[rs][c] = fma(a, (double)q[u][rs][c], acc[rs][c]);
                }
        } else {
            pmc_d2x q[2][8][2];
#pragma unroll
            for (int u = 0; u < J; ++u)
#pragma unroll
                for (int rs = 0; rs < T; ++rs) {
                    q[u][rs][0] = reinterpret_cast<const pmc_d2x*>(x + at[u][rs])[0];
                    q[u][rs][1] = reinterpret_cast<const pmc_d2x*>(x + at[u][rs])[1];
                }
            pin_deep_d(q);
#pragma unroll
            for (int u = 0; u < J; ++u)
#pragma unroll
                for (int rs = 0; rs < T; ++rs) {
                    const double a = __shfl(vj[u], rs * G + g, kWave);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[rs][c] = fma(a, q[u][rs][c >> 1][c & 1], acc[rs][c]);
                }
        }
#pragma unroll
        for (int u = 0; u < J; ++u) {
            cj[u] = cn[u];
            vj[u] = vn[u];
        }
    }
}

// acc = A x for one slice, shared fp64 values, gathered vector of type XT (the T > 1 schedule of sell_row_range; T == 1
// walks the slice columns one by one)
// DEEP > 1 (NB = 32, shared values): sell_row_range_deep with that many slice columns per trip
template <int NB, typename XT, bool NT = false, int BV = 0, int DEEP = 1>
__device__ __forceinline__ void sell_row_range_t(const int* __restrict__ cols, const double* __restrict__ vals,
                                                 const XT* __restrict__ x, int off, int width, int lane, int LD,
                                                 double (&acc)[Lay<NB>::T][Lay<NB>::C]) {
    if constexpr (DEEP > 1 && NB == 32 && BV == 0)
        sell_row_range_deep<NB, XT, DEEP>(cols, vals, x, off, width, lane, LD, acc);
    else
        sell_row_range<NB, BV, false, true, NT, XT>(cols, vals, x, nullptr, off, width, lane, LD, acc);
}

// sell_row_range for the TH row steps rs0 .. rs0 + TH - 1 of a slice only (shared values).  A kernel that sweeps a slice in
// T / TH such passes keeps TH instead of T rows' accumulators, gathers and shuffled slot data alive - the element-grouped
// kernels below, which carry two accumulators and up to three gathered vectors per row, drop from 206-246 VGPRs (two waves per
// SIMD) to four waves per SIMD; the (index, value) pairs of the later passes come from L1.
template <int NB, bool CS, typename XT>
__device__ __forceinline__ constexpr bool lean_part() {
    return Lay<NB>::T > 1 && ((!CS && sizeof(XT) == 4) ? kLeanGather : kLeanCs);
}
template <int NB, bool CS, bool ZERO, bool NT, int TH, typename XT = double>
__device__ __forceinline__ void sell_row_part(const int* __restrict__ cols, const double* __restrict__ vals,
                                              const XT* __restrict__ x, const double* __restrict__ cs, int off, int width,
                                              int lane, int LD, int rs0, double (&acc)[TH][Lay<NB>::C]) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int g = lane / T, t = lane % T;
    if constexpr (ZERO) {
#pragma unroll
        for (int q = 0; q < TH; ++q)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[q][c] = 0.0;
    }
    int slot = off + lane;
    int cj = 0;
    double vj = 0.0;
    if (width > 0) {
        cj = load_stream<NT>(cols + slot);
        vj = load_stream<NT>(vals + slot);
    }
    if constexpr (lean_part<NB, CS, XT>()) {
        // Lean loop: 32-bit element offsets address the gathers, gathered rows stay in their storage type until their FMA
        // (fp32 rows of the preconditioned Krylov vectors: half the registers), and the matrix values are fetched across
        // lanes only AFTER the gathers have been issued - fewer registers live while the loads are in flight, and the
        // cross-lane traffic overlaps the gather latency.  Hex 64^3 x 16, rocprofv3 averages: Darcy operator u-rows
        // 96.9 -> 85.1 us, M-block polynomial 119.5 -> 114.8 us (compiled for three waves per SIMD instead the operator
        // spills and takes 90.5 us; the same loop in the block operator K5 - 92 instead of 114 registers, five waves - changed
        // nothing measurable).
        for (int j = 0; j < width; ++j, slot += kWave) {
            int cn = cj;
            double vn = vj;
            if (j + 1 < width) {
                cn = load_stream<NT>(cols + slot + kWave);
                vn = load_stream<NT>(vals + slot + kWave);
            }
            unsigned at[TH];
#pragma unroll
            for (int q = 0; q < TH; ++q) at[q] = (unsigned)__shfl(cj, (rs0 + q) * G + g, kWave) * (unsigned)LD + (unsigned)(t * C);
            RawVec<XT, C> xr[TH];
            double sv[CS ? TH : 1][C];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < TH; ++q) {
                load_raw<C>(x + at[q], xr[q]);
                if constexpr (CS) load_c<C>(cs + at[q], sv[q]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < TH; ++q) {
                const double a = __shfl(vj, (rs0 + q) * G + g, kWave);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    double xv = (double)xr[q].v[c];
                    if constexpr (CS) xv *= sv[q][c];
                    acc[q][c] = fma(a, xv, acc[q][c]);
                }
            }
            cj = cn;
            vj = vn;
        }
        return;
    }
    for (int j = 0; j < width; ++j, slot += kWave) {
        int cn = cj;
        double vn = vj;
        if (j + 1 < width) {
            cn = load_stream<NT>(cols + slot + kWave);
            vn = load_stream<NT>(vals + slot + kWave);
        }
        int cc[TH];
        double aa[TH];
#pragma unroll
        for (int q = 0; q < TH; ++q) {
            const int src = (rs0 + q) * G + g;
            cc[q] = (T == 1) ? cj : __shfl(cj, src, kWave);
            aa[q] = (T == 1) ? vj : __shfl(vj, src, kWave);
        }
        double xv[TH][C], sv[TH][C];
        if constexpr (T > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < TH; ++q) {
            load_v<C>(x + (size_t)cc[q] * LD + t * C, xv[q]);
            if constexpr (CS) load_c<C>(cs + (size_t)cc[q] * LD + t * C, sv[q]);
        }
        if constexpr (T > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < TH; ++q)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if constexpr (CS) xv[q][c] *= sv[q][c];
                acc[q][c] = fma(aa[q], xv[q][c], acc[q][c]);
            }
        cj = cn;
        vj = vn;
    }
}

}  // namespace pmc

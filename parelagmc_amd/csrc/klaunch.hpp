// Host-side launch helpers shared by the kernel units (k_*.hip): grids, column groups, the bounds of the fused dots, the
// non-temporal thresholds, the launch check.  Included by the kernel sources only.
// Every unit holds its own copy of the statics that cache a lab_env() lookup: lab_env() is constant for the life of a process.
#pragma once
#include "kdev.hpp"

#include <cstdlib>

#include <algorithm>

namespace pmc {

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
static inline unsigned dot_grid_bound() {
    static const unsigned v = [] {
        const char* e = lab_env("PMC_DOT_GRID");
        const long x = e ? atol(e) : 0;
        return x >= 8 ? (unsigned)x : 4096u;
    }();
    return v;
}

namespace k {

// (called once per launch, next to it: a grid the bound actually cuts is counted as PMC_COUNT_BOUNDED_GRID)
static inline dim3 grid_bounded(dim3 g, bool bounded) {
    if (!bounded || g.x <= dot_grid_bound()) return g;
    count_solve_path(PMC_COUNT_BOUNDED_GRID);
    return dim3(dot_grid_bound());
}

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

static inline dim3 grid_dot(int n, int nb) { return dim3(std::min(grid_flat(n, nb).x, 1024u)); }

}  // namespace k
}  // namespace pmc

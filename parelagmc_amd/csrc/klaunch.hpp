// Host-side launch helpers shared by the kernel units (k_*.hip): grids, column groups, the bounds of the fused dots, the
// non-temporal thresholds, the launch check, and the dispatch helpers that turn a run-time fact of a launch into a template
// argument of its kernel.  Included by the kernel sources only.
//
// How a launcher chooses its kernel.  Every kernel template has ONE launch site per unit.  A launcher decides the form at run
// time (fused dot or not, value storage, non-temporal streams, ...) and hands each such fact to a dispatch_* helper below,
// which calls a generic lambda with the fact as a compile-time constant:
//     dispatch_bool(dot_partial != nullptr, [&](auto dot) { constexpr bool DOT = decltype(dot)::value; ... });
// A lambda called for both values of a flag instantiates the kernel for both.  The set of instantiations is part of a unit's
// machine code (see the head of k_sell.hip), so a form that must not exist is pruned where the flag is dispatched - the
// helpers' EXISTS argument - not by leaving the launch unreachable.  The helpers and the lambdas they call are forced inline
// (PMC_DISPATCH_INLINE): a dispatch compiles to the if / switch one would write by hand, no call is left on the launch path.
// PMC_DISPATCH_NB (kdev.hpp) does the same for the batch width.
// Every unit holds its own copy of the statics that cache a lab_env() lookup: lab_env() is constant for the life of a process.
#pragma once
#include "kdev.hpp"

#include <cstdlib>

#include <algorithm>
#include <type_traits>

namespace pmc {

// ---- run-time fact -> compile-time constant
#define PMC_DISPATCH_INLINE __attribute__((always_inline, flatten)) inline
// a flag as std::bool_constant.  EXISTS = false: the kernel has no such form here - only the `false` instantiation is made,
// and a set flag takes it too (the launcher has ruled it out, or the form without the flag serves the launch as well)
template <bool EXISTS = true, typename F>
PMC_DISPATCH_INLINE auto dispatch_bool(bool v, F&& f) {
    if constexpr (EXISTS) {
        if (v) return f(std::true_type{});
    }
    return f(std::false_type{});
}
// the kernels' BV argument - how a SellView stores its values - as std::integral_constant<int, BV>
constexpr int kSharedValues = 0;   // one fp64 value per entry for all realizations
constexpr int kValues64 = 1;       // per-realization fp64 values
constexpr int kValues32 = 2;       // per-realization fp32 values (SellView::f32)
// PER_REALIZATION = false: the launcher serves shared values only (it has thrown otherwise)
template <bool PER_REALIZATION = true, typename F>
PMC_DISPATCH_INLINE auto dispatch_values(const SellView& A, F&& f) {
    if constexpr (PER_REALIZATION) {
        if (A.bv && A.f32) return f(std::integral_constant<int, kValues32>{});
        if (A.bv) return f(std::integral_constant<int, kValues64>{});
    }
    return f(std::integral_constant<int, kSharedValues>{});
}
// a stored vector (zvec) as the typed pointer to its elements, float* or double*; `same` are further vectors of that storage
template <typename F, typename... Z>
PMC_DISPATCH_INLINE auto dispatch_storage(zvec z, F&& f, Z... same) {
    if (z.f32) return f(z.as<float>(), same.template as<float>()...);
    return f(z.as<double>(), same.template as<double>()...);
}
// a bare storage flag (no vector at hand) as a tag of the element type: `typename decltype(t)::type` is float or double
template <typename T>
struct type_tag { using type = T; };
template <typename F>
PMC_DISPATCH_INLINE auto dispatch_f32(bool f32, F&& f) {
    if (f32) return f(type_tag<float>{});
    return f(type_tag<double>{});
}
// the widths of the row-split instantiations (SellView::split_log2), which exist for launches of at most 8 realizations
template <typename F>
PMC_DISPATCH_INLINE auto dispatch_narrow(int nb, F&& f) {
    switch (nb) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: throw Error(PMC_ERR_INTERNAL, "row-split level kernels serve launches of 1, 2, 4 or 8 realizations");
    }
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

// Device-side helpers of the kernels (the units k_*.hip): tuning constants, batch layout, typed loads / stores, block reductions,
// the XCD-aware slice walk.  Included by the kernel sources only; kernels.hpp stays the interface the rest of the library sees.
#pragma once
#include "kernels.hpp"

#include <cstddef>

namespace pmc {

#ifndef PMC_KBLOCK
#define PMC_KBLOCK 256
#endif
static constexpr int kBlock = PMC_KBLOCK;   // workgroup size of the streaming / SpMM kernels (tuning builds may override)
static constexpr int kWave = 64;
#ifndef PMC_LEAN_GATHER
#define PMC_LEAN_GATHER 1
#endif
static constexpr bool kLeanGather = PMC_LEAN_GATHER != 0;   // see sell_row_part: fp32 gathers without column scaling
#ifndef PMC_LEAN_CS
#define PMC_LEAN_CS 1
#endif
static constexpr bool kLeanCs = PMC_LEAN_CS != 0;           // ... fp64 gathers / column scaling (eg_poly2_kernel)
#ifndef PMC_EG_LATE_COEF
#define PMC_EG_LATE_COEF 1
#endif
static constexpr bool kEgLateCoef = PMC_EG_LATE_COEF != 0;  // see eg_row_product
#ifndef PMC_LEAN_RANGE_MIN_NB
#define PMC_LEAN_RANGE_MIN_NB 32
#endif
// sell_row_range takes the lean gather loop (see sell_row_part) from this batch width on: at NB = 32 the one-column loop
// needs 170-184 registers (two waves per SIMD), the lean one fits three; at NB = 16 (four waves either way) it changed nothing
static constexpr int kLeanRangeMinNb = PMC_LEAN_RANGE_MIN_NB;

// Batch layout helper.  A row of NB interleaved values is handled by T lanes, C = 2 doubles (one 16 B
// access) each, so a group of T lanes touches NB*8 contiguous bytes and a wavefront G = 64/T rows.
template <int NB>
struct Lay {
    static constexpr int C = NB >= 32 ? 4 : (NB >= 2 ? 2 : 1);   // NB = 32: two 16 B accesses per lane, still 8 lanes per row
    static constexpr int T = NB / C;
    static constexpr int G = kWave / T;
};

// Column groups (super-batches).  A batch wider than kGroup realizations is ONE interleaved vector with row stride
// ld = nb doubles, worked on as nb / kGroup groups of kGroup columns: group g owns the columns [g kGroup, (g + 1) kGroup) of
// every row, blockIdx.y names the group, and every launch carries all groups - a level too small to fill the chip with 32
// realizations is solved 64 ... 256 at a time.  Only the widest instantiation (NB == kGroup) is group-capable; the
// narrower ones keep the compile-time row stride NB (ld is ignored, gridDim.y == 1).
template <int NB>
__device__ __forceinline__ int row_ld(int ld) {
    if constexpr (NB == kGroup) return ld;
    else return NB;
}
template <int NB>
__device__ __forceinline__ int col0() {
    if constexpr (NB == kGroup) return (int)blockIdx.y * NB;
    else return 0;
}

template <int C>
__device__ __forceinline__ void load_c(const double* __restrict__ p, double (&v)[C]) {
    if constexpr (C == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int i = 0; i < C / 2; ++i) {
            const double2 t = reinterpret_cast<const double2*>(p)[i];
            v[2 * i] = t.x;
            v[2 * i + 1] = t.y;
        }
    }
}
template <int C>
__device__ __forceinline__ void store_c(double* __restrict__ p, const double (&v)[C]) {
    if constexpr (C == 1) {
        p[0] = v[0];
    } else {
#pragma unroll
        for (int i = 0; i < C / 2; ++i) reinterpret_cast<double2*>(p)[i] = make_double2(v[2 * i], v[2 * i + 1]);
    }
}

// Per-realization matrix values of the PRECONDITIONER (Darcy: the Schur-complement hierarchy S(k)) may be stored in fp32
// (BV == 2; BV == 1: fp64): the preconditioner stays a fixed symmetric linear operator - MINRES converges to the same
// solution at the same tolerance - while the dominant stream of its kernels halves.  Arithmetic stays fp64.
template <int C>
__device__ __forceinline__ void load_cf(const float* __restrict__ p, double (&v)[C]) {
    if constexpr (C == 1) {
        v[0] = (double)p[0];
    } else if constexpr (C == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = (double)t.x;
        v[1] = (double)t.y;
    } else {
#pragma unroll
        for (int i = 0; i < C / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            v[4 * i] = (double)t.x;
            v[4 * i + 1] = (double)t.y;
            v[4 * i + 2] = (double)t.z;
            v[4 * i + 3] = (double)t.w;
        }
    }
}
// values of batched matrix entry `idx` (in units of one value): fp64 or fp32 storage
template <int BV, int C>
__device__ __forceinline__ void load_bv(const double* __restrict__ vals, size_t idx, double (&v)[C]) {
    if constexpr (BV == 2) load_cf<C>(reinterpret_cast<const float*>(vals) + idx, v);
    else load_c<C>(vals + idx, v);
}
// advance a batched-value pointer by c columns
template <int BV>
__device__ __forceinline__ const double* shift_bv(const double* vals, int c) {
    if constexpr (BV == 2) return reinterpret_cast<const double*>(reinterpret_cast<const float*>(vals) + c);
    else return vals + c;
}

// typed vector accesses: fp64 or fp32 storage, fp64 in registers
template <typename T>
struct ident { using type = T; };   // keeps a parameter out of template argument deduction (nullptr arguments)
template <int C>
__device__ __forceinline__ void load_v(const double* __restrict__ p, double (&v)[C]) { load_c<C>(p, v); }
template <int C>
__device__ __forceinline__ void load_v(const float* __restrict__ p, double (&v)[C]) { load_cf<C>(p, v); }
template <int C>
__device__ __forceinline__ void store_v(double* __restrict__ p, const double (&v)[C]) { store_c<C>(p, v); }
template <int C>
__device__ __forceinline__ void store_v(float* __restrict__ p, const double (&v)[C]) {
    if constexpr (C == 1) {
        p[0] = (float)v[0];
    } else if constexpr (C == 2) {
        *reinterpret_cast<float2*>(p) = make_float2((float)v[0], (float)v[1]);
    } else {
#pragma unroll
        for (int i = 0; i < C / 4; ++i)
            reinterpret_cast<float4*>(p)[i] = make_float4((float)v[4 * i], (float)v[4 * i + 1], (float)v[4 * i + 2], (float)v[4 * i + 3]);
    }
}
// values an fp32 store will keep: rounding BEFORE a fused dot keeps <., out> consistent with what is stored
template <typename T, int C>
__device__ __forceinline__ void round_to(double (&v)[C]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = (double)(float)v[i];
    }
}

// What a gather leaves in registers until its FMA: fp32-stored vectors stay fp32 (half the registers per gather in flight)
// and are widened only when they are consumed.
template <typename XT, int C>
struct RawVec {
    XT v[C];
};
template <int C>
__device__ __forceinline__ void load_raw(const double* __restrict__ p, RawVec<double, C>& r) { load_c<C>(p, r.v); }
template <int C>
__device__ __forceinline__ void load_raw(const float* __restrict__ p, RawVec<float, C>& r) {
    if constexpr (C == 1) {
        r.v[0] = p[0];
    } else if constexpr (C == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r.v[0] = t.x;
        r.v[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < C / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            r.v[4 * i] = t.x;
            r.v[4 * i + 1] = t.y;
            r.v[4 * i + 2] = t.z;
            r.v[4 * i + 3] = t.w;
        }
    }
}

// The T = 8 gathers of one slice column (fp32 rows, four columns per lane) as ONE point of use.  hipcc sinks loads from
// __restrict__ pointers past __builtin_amdgcn_sched_barrier (they carry no ordering against it) down to their first use; in
// the kernels whose gathered fp32 values die in their own FMA group that turned "eight gathers in flight" into load - wait -
// convert - fma, eight times per slice column (ISA of vc_residual_kernel<32, float, ...> and vc_poly2_kernel<32, float, ...>,
// round 4: a level of 44 k rows took 67-74 us per launch where the fp64-gather kernel on the same matrix took 30).  An empty
// asm that takes all eight results as operands cannot be split: every load is issued before it.
typedef float pmc_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pin_gathers(RawVec<float, 4> (&xr)[8]) {
    pmc_f4 q0 = {xr[0].v[0], xr[0].v[1], xr[0].v[2], xr[0].v[3]}, q1 = {xr[1].v[0], xr[1].v[1], xr[1].v[2], xr[1].v[3]};
    pmc_f4 q2 = {xr[2].v[0], xr[2].v[1], xr[2].v[2], xr[2].v[3]}, q3 = {xr[3].v[0], xr[3].v[1], xr[3].v[2], xr[3].v[3]};
    pmc_f4 q4 = {xr[4].v[0], xr[4].v[1], xr[4].v[2], xr[4].v[3]}, q5 = {xr[5].v[0], xr[5].v[1], xr[5].v[2], xr[5].v[3]};
    pmc_f4 q6 = {xr[6].v[0], xr[6].v[1], xr[6].v[2], xr[6].v[3]}, q7 = {xr[7].v[0], xr[7].v[1], xr[7].v[2], xr[7].v[3]};
    asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5), "+v"(q6), "+v"(q7));
    const pmc_f4 q[8] = {q0, q1, q2, q3, q4, q5, q6, q7};
#pragma unroll
    for (int rs = 0; rs < 8; ++rs)
#pragma unroll
        for (int c = 0; c < 4; ++c) xr[rs].v[c] = q[rs][c];
}
template <typename XT, int C, int T>
__device__ __forceinline__ void pin_gathers(RawVec<XT, C> (&)[T]) {}
// the same for sixteen widened values (8 row steps x 2 columns or 4 x 4): the own-row reads of an epilogue, issued together
template <int R, int C>
__device__ __forceinline__ void pin_block(double (&a)[R][C]) {
    if constexpr (R == 8 && C == 2)
        asm volatile("" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]),
                     "+v"(a[3][1]), "+v"(a[4][0]), "+v"(a[4][1]), "+v"(a[5][0]), "+v"(a[5][1]), "+v"(a[6][0]), "+v"(a[6][1]),
                     "+v"(a[7][0]), "+v"(a[7][1]));
    else if constexpr (R == 4 && C == 4)
        asm volatile("" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]),
                     "+v"(a[1][3]), "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[2][2]), "+v"(a[2][3]), "+v"(a[3][0]), "+v"(a[3][1]),
                     "+v"(a[3][2]), "+v"(a[3][3]));
    else if constexpr (R == 2 && C == 4)
        asm volatile("" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]),
                     "+v"(a[1][3]));
}

// Vector streams without reuse inside the iteration (MINRES w / x updates of large levels): non-temporal variants, so that a
// flat kernel running beside a gather kernel (second stream, other lanes) does not sweep that kernel's rows out of L2.
// Measured at 0.6 M rows x 16: one lane 1096 -> 1112, four lanes 1446 -> 1454 samples/s; small levels keep the cached
// accesses (their vectors live in the caches from one iteration to the next).
template <bool NT, int C>
__device__ __forceinline__ void load_c_nt(const double* __restrict__ p, double (&v)[C]) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = __builtin_nontemporal_load(p + i);
    } else {
        load_c<C>(p, v);
    }
}
template <bool NT, int C>
__device__ __forceinline__ void load_v_nt(const double* __restrict__ p, double (&v)[C]) { load_c_nt<NT, C>(p, v); }
template <bool NT, int C>
__device__ __forceinline__ void load_v_nt(const float* __restrict__ p, double (&v)[C]) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = (double)__builtin_nontemporal_load(p + i);
    } else {
        load_cf<C>(p, v);
    }
}
template <bool NT, int C>
__device__ __forceinline__ void store_c_nt(double* __restrict__ p, const double (&v)[C]) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) __builtin_nontemporal_store(v[i], p + i);
    } else {
        store_c<C>(p, v);
    }
}

// Streaming accesses (matrix values / indices read once, result rows written once) with NT = true are non-temporal, so
// that they do not displace the gathered x rows - the only data with reuse - from the XCD's L2.  Worth it only when the
// operands exceed the 256 MiB Infinity Cache, which non-temporal accesses bypass: measured on the block operator at
// 4.7 M rows (1.65 GB per launch) 460-475 -> 435-448 us inside the solver loop; at 0.6 M rows (206 MB, cache-resident when
// launched back to back) 43 -> 55 us, and no change inside the loop.  The launcher picks NT by operand size.
template <bool NT, int C>
__device__ __forceinline__ void store_c_stream(double* __restrict__ p, const double (&v)[C]) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) __builtin_nontemporal_store(v[i], p + i);
    } else {
        store_c<C>(p, v);
    }
}
template <bool NT>
__device__ __forceinline__ int load_stream(const int* __restrict__ p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ double load_stream(const double* __restrict__ p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// The Lanczos update y = c0 a + c1 b + c2 y of MINRES, columns k0 .. k0 + C - 1: ONE expression for the flat kernel
// (lincomb3_kernel) and for the operator pass that forms the vector in its epilogue (sell_spmm_kernel, LZ >= 2), so that
// both contract to the same instructions and give the same bits.
template <int C>
__device__ __forceinline__ void lanczos_combine(const double* __restrict__ c0, const double* __restrict__ c1,
                                                const double* __restrict__ c2, int k0, const double (&a)[C],
                                                const double (&b)[C], double (&y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = c0[k0 + c] * a[c] + c1[k0 + c] * b[c] + c2[k0 + c] * y[c];
}

// the same with the lane's coefficients in registers (read once per wavefront: the operator pass, whose stores the compiler
// must assume to alias c0 / c1 / c2 and would reload them behind).  The contraction is written out: the expression above
// compiles to c1 b, then fma(c0, a, .), then fma(c2, y, .), but which product stays the plain multiply is the backend's choice
// per call site - with a (the row sums) ready before b arrives it took c0 a here, one rounding apart from the flat kernel.
template <int C>
__device__ __forceinline__ void lanczos_combine(const double (&c0)[C], const double (&c1)[C], const double (&c2)[C],
                                                const double (&a)[C], const double (&b)[C], double (&y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = fma(c2[c], y[c], fma(c0[c], a[c], c1[c] * b[c]));
}

template <bool NT, int C>
__device__ __forceinline__ void store_v_stream(double* __restrict__ p, const double (&v)[C]) { store_c_stream<NT, C>(p, v); }
template <bool NT, int C>
__device__ __forceinline__ void store_v_stream(float* __restrict__ p, const double (&v)[C]) {
    if constexpr (NT) {
#pragma unroll
        for (int i = 0; i < C; ++i) __builtin_nontemporal_store((float)v[i], p + i);
    } else {
        store_v<C>(p, v);
    }
}

template <int NB>
__device__ __forceinline__ void load_row(const double* __restrict__ p, double (&v)[NB]) {
    if constexpr (NB == 1) {
        v[0] = p[0];
    } else {
        const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int i = 0; i < NB / 2; ++i) {
            double2 t = q[i];
            v[2 * i] = t.x;
            v[2 * i + 1] = t.y;
        }
    }
}
template <int NB>
__device__ __forceinline__ void store_row(double* __restrict__ p, const double (&v)[NB]) {
    if constexpr (NB == 1) {
        p[0] = v[0];
    } else {
        double2* q = reinterpret_cast<double2*>(p);
#pragma unroll
        for (int i = 0; i < NB / 2; ++i) q[i] = make_double2(v[2 * i], v[2 * i + 1]);
    }
}

// Virtual block index / grid extent of the slice kernels.  A launch of several column groups (nb > kGroup) is laid out as
// dim3(8, groups, chunks) (groups_xcd): the hardware deals workgroups to the 8 XCDs by their linear id x + 8 y + 8 groups z, so
// the blocks (x, 0, z) and (x, 1, z) - the SAME slices for column group 0 and 1 - run on the same XCD right after each other and
// the second one finds the slices' (index, value) pairs in that XCD's L2 instead of reading the matrix from HBM once more.
// Ordinary launches are dim3(blocks, groups, 1): vblock() == blockIdx.x.
__device__ __forceinline__ int vblock() { return (int)(blockIdx.z * gridDim.x + blockIdx.x); }
__device__ __forceinline__ int vgrid() { return (int)(gridDim.z * gridDim.x); }

// Column-wise block reduction.  Every lane holds partial sums p[0..C) for columns (lane % T)*C + c.
// Deterministic: fixed xor tree over the lanes that share a column, fixed order over the 4 wavefronts.
// Writes partial[vblock()*LD + k] (partial already points at the group's first column).
template <int NB>
__device__ __forceinline__ void reduce_cols_store(double (&p)[Lay<NB>::C], double* __restrict__ partial, int LD = NB) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T;
    __shared__ double lds[kBlock / kWave][NB];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double v = p[c];
#pragma unroll
        for (int off = kWave / 2; off >= T; off >>= 1) v += __shfl_xor(v, off, kWave);
        p[c] = v;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane < T) {
#pragma unroll
        for (int c = 0; c < C; ++c) lds[wave][lane * C + c] = p[c];
    }
    __syncthreads();
    if (threadIdx.x < NB) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s += lds[w][threadIdx.x];
        partial[(size_t)vblock() * LD + threadIdx.x] = s;
    }
}

// The same for the flat kernels on a batch of W = ld > kGroup columns (runtime width, W divides 4 * kBlock): thread t owns the
// columns (4 t) % W + c of the rows it visits; LDS holds every thread's four sums, thread j < W adds the 4 kBlock / W
// entries of column j in index order (deterministic).  Writes partial[blockIdx.x * W + j].
__device__ __forceinline__ void reduce_cols_store_wide(const double (&p)[4], double* __restrict__ partial, int W) {
    __shared__ double lds[kBlock * 4];
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[threadIdx.x * 4 + c] = p[c];
    __syncthreads();
    if ((int)threadIdx.x < W) {
        double s = 0.0;
        for (int m = threadIdx.x; m < kBlock * 4; m += W) s += lds[m];
        partial[(size_t)blockIdx.x * W + threadIdx.x] = s;
    }
}
template <int NB>
__device__ __forceinline__ void reduce_flat_store(double (&p)[Lay<NB>::C], double* __restrict__ partial, int W) {
    if constexpr (NB == kGroup) {
        if (W > NB) {
            reduce_cols_store_wide(p, partial, W);
            return;
        }
    }
    reduce_cols_store<NB>(p, partial);
}

// Second-stage sums of the per-block partials (the scalar kernels, their staging and compression kernels) deal the blocks
// of a column over blockDim / nb threads.  A launch of kGroup columns deals them as a launch of two column groups does (half
// of its threads stay idle), so a realization's dots - and with them its solve - are the same bits in one launch of 64 and
// in a launch of 32.  The first-stage partials of the slice kernels do not depend on the number of groups.
__device__ __forceinline__ int reduce_width(int nb) { return nb == kGroup ? 2 * kGroup : nb; }

// XCD-aware slice assignment.  The dispatcher deals workgroups round-robin over the 8 XCDs (block b runs on XCD b % 8),
// and each XCD has its own 4 MiB L2.  XCD x owns one CONTIGUOUS eighth of the slices (in processing order), so the x
// entries its gathers touch (mesh neighbours = nearby indices) stay in that XCD's L2 instead of being fetched by all
// eight.  Inside the eighth the slices are dealt CYCLICALLY over the XCD's workgroups (block i of the XCD takes the
// slices 4 i .. 4 i + 3, then those one full round of workgroups further on, ...): whatever the grid size, the slices
// in flight on an XCD at any time form one compact window of the rows.  (With one contiguous chunk per workgroup - the
// round-1 layout - a bounded grid of 4096 workgroups at 4.7 M rows had concurrently running workgroups 19 slices apart:
// the window of x rows in flight was 5x wider than the L2 and x was fetched 3 times, 2.87 GB per launch against
// 1.65 GB algorithmic.)  Placement only affects speed, never results.
struct SliceWalk {
    int begin, end, stride;
};
__device__ __forceinline__ SliceWalk slice_walk(int nslices) {
    constexpr int WPB = kBlock / kWave;                     // wavefronts = slices per workgroup and round
    const int nblk = vgrid(), bid = vblock(), wave = threadIdx.x / kWave;
    if (nblk < 8) return SliceWalk{bid * WPB + wave, nslices, nblk * WPB};
    const int xcd = bid % 8, idx = bid / 8;
    const int nb_x = nblk / 8 + (xcd < nblk % 8 ? 1 : 0);   // workgroups of this XCD
    const int per = (nslices + 7) / 8;                      // slices of an XCD (the last one may get fewer)
    const int lo = min(xcd * per, nslices), hi = min(lo + per, nslices);
    return SliceWalk{lo + idx * WPB + wave, hi, nb_x * WPB};
}

// Launch-side dispatch on the batch width: the body sees the compile-time interleave NB of a launch of nb realizations
// (the units k_*.hip and every other translation unit that starts a batched kernel).
#define PMC_DISPATCH_NB(nb, ...)                                          \
    switch (nb) {                                                         \
        case 1: { constexpr int NB = 1; __VA_ARGS__; } break;             \
        case 2: { constexpr int NB = 2; __VA_ARGS__; } break;             \
        case 4: { constexpr int NB = 4; __VA_ARGS__; } break;             \
        case 8: { constexpr int NB = 8; __VA_ARGS__; } break;             \
        case 16: { constexpr int NB = 16; __VA_ARGS__; } break;           \
        case 32: case 64: case 128: case 256: { constexpr int NB = 32; __VA_ARGS__; } break;   /* column groups of 32 */ \
        default: throw Error(PMC_ERR_INTERNAL, "unsupported batch width"); \
    }

}  // namespace pmc

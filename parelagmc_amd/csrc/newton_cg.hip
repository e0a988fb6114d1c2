// Batched conjugate-gradient vector algebra for Newton-CG (pmc_ncg_*).
//
// nb independent columns of length n, sample-major.  The caller applies the operator (Hp = H p, e.g. pmc_bayes_logpost_gn_hessvec
// on pmc_ncg_search_direction) and calls pmc_ncg_step; everything between two applications - <p, Hp>, alpha, d += alpha p,
// r -= alpha Hp, <r, r>, the tolerance test, beta, p = r + beta p - stays on the device in three launches:
//     ncg_dot_kernel     partial <p, Hp> per chunk
//     ncg_update_kernel  alpha from the partials; d, r updated; partial <r, r> per chunk
//     ncg_dir_kernel     rr from the partials; tolerance test; p updated (or zeroed, once, when the column ends); scalars written
// The per-column scalars live in NcgCol records, double-buffered: the kernels of step s read buffer s & 1, and chunk 0 of
// ncg_dir_kernel writes buffer (s + 1) & 1, so no workgroup reads a scalar another one of the same launch writes.
//
// Summation order.  A column is cut into chunks of kNcgChunk entries, one workgroup each; inside a chunk thread t owns the
// entries j * 2 * kNcgThreads + 2 t + {0, 1}, j = 0 .. kNcgPer / 2 - 1, accumulated in that order with fma; the workgroup's 256
// partial sums go through a fixed shuffle tree per wave and the four wave sums are added in ascending order; the chunk
// partials are added in ascending order by every workgroup that needs the total.  All of it depends on n alone - never on nb,
// on the neighbouring columns or on whether the 16-byte path is taken -, so a column's bits are the same in every batch.
// No atomics, no LDS beyond the four wave sums, no scratch.
#include "handles.hpp"

#include <cstring>

namespace pmc {

namespace {

template <bool VEC>
__device__ __forceinline__ void ncg_ld2(const double* __restrict__ p, int i, int n, double& a, double& b) {
    if (VEC) {
        const double2 v = *reinterpret_cast<const double2*>(p + i);
        a = v.x;
        b = v.y;
    } else {
        a = p[i];
        b = i + 1 < n ? p[i + 1] : 0.0;
    }
}
template <bool VEC>
__device__ __forceinline__ void ncg_st2(double* __restrict__ p, int i, int n, double a, double b) {
    if (VEC) {
        *reinterpret_cast<double2*>(p + i) = make_double2(a, b);
    } else {
        p[i] = a;
        if (i + 1 < n) p[i + 1] = b;
    }
}

// sum of the workgroup's per-thread values, the same in every thread: xor-shuffle tree inside each wave, wave sums ascending
__device__ __forceinline__ double ncg_block_sum(double v) {
    __shared__ double wsum[kNcgThreads / 64];
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // a previous call's readers are done with wsum
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = wsum[0];
    for (int w = 1; w < kNcgThreads / 64; ++w) s += wsum[w];
    return s;
}

// total of a column's chunk partials, ascending; every thread computes the same value from the same (uniform) loads
__device__ __forceinline__ double ncg_total(const double* __restrict__ part, int nch) {
    double s = part[0];
    for (int c = 1; c < nch; ++c) s += part[c];
    return s;
}

// entry offset of pair j of this thread inside its column
__device__ __forceinline__ int ncg_at(int j) { return (int)blockIdx.x * kNcgChunk + j * 2 * kNcgThreads + 2 * (int)threadIdx.x; }

// pmc_ncg_begin: r = p = g, d = 0 and the partial <g, g> on the active columns; p = 0 on the others (nothing else of theirs)
template <bool VEC>
__global__ __launch_bounds__(kNcgThreads) void ncg_begin_kernel(int n, int nch, const double* __restrict__ g,
                                                                const int32_t* __restrict__ active, double* __restrict__ d,
                                                                double* __restrict__ r, double* __restrict__ p,
                                                                double* __restrict__ part) {
    const int b = blockIdx.y;
    const size_t o = (size_t)b * n;
    const bool on = active[b] != 0;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kNcgPer / 2; ++j) {
        const int i = ncg_at(j);
        if (i >= n) break;
        if (!on) {
            ncg_st2<VEC>(p + o, i, n, 0.0, 0.0);
            continue;
        }
        double a0, a1;
        ncg_ld2<VEC>(g + o, i, n, a0, a1);
        ncg_st2<VEC>(r + o, i, n, a0, a1);
        ncg_st2<VEC>(p + o, i, n, a0, a1);
        ncg_st2<VEC>(d + o, i, n, 0.0, 0.0);
        acc = fma(a0, a0, acc);
        acc = fma(a1, a1, acc);
    }
    if (!on) return;                                   // uniform over the workgroup
    const double s = ncg_block_sum(acc);
    if (threadIdx.x == 0) part[(size_t)b * nch + blockIdx.x] = s;
}

// the columns' scalars after pmc_ncg_begin: one thread per column
__global__ void ncg_begin_cols_kernel(int nb, int nch, const double* __restrict__ part, const double* __restrict__ eta,
                                      const int32_t* __restrict__ active, NcgCol* __restrict__ cols) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    NcgCol c;
    c.active = active[b] != 0 ? 1 : 0;
    c.gg = c.active ? ncg_total(part + (size_t)b * nch, nch) : 0.0;
    c.rr = c.gg;
    c.tol2 = eta[b] * eta[b] * c.gg;
    c.pHp = 0.0;
    c.count = 0;
    c.npc = 0;
    c.done = (c.active && c.gg > 0.0) ? 0 : 1;         // a zero (or non-finite) right-hand side has nothing to iterate on
    cols[b] = c;
}

// partial <a, b> per chunk; cols != nullptr: finished columns are skipped
template <bool VEC>
__global__ __launch_bounds__(kNcgThreads) void ncg_dot_kernel(int n, int nch, const NcgCol* __restrict__ cols,
                                                              const double* __restrict__ x, const double* __restrict__ y,
                                                              double* __restrict__ part) {
    const int b = blockIdx.y;
    if (cols && cols[b].done) return;
    const size_t o = (size_t)b * n;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kNcgPer / 2; ++j) {
        const int i = ncg_at(j);
        if (i >= n) break;
        double x0, x1, y0, y1;
        ncg_ld2<VEC>(x + o, i, n, x0, x1);
        ncg_ld2<VEC>(y + o, i, n, y0, y1);
        acc = fma(x0, y0, acc);
        acc = fma(x1, y1, acc);
    }
    const double s = ncg_block_sum(acc);
    if (threadIdx.x == 0) part[(size_t)b * nch + blockIdx.x] = s;
}

__global__ void ncg_dot_final_kernel(int nb, int nch, const double* __restrict__ part, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) out[b] = ncg_total(part + (size_t)b * nch, nch);
}

// alpha = rr / <p, Hp>; d += alpha p, r -= alpha Hp, partial <r, r>.  <p, Hp> <= 0 (or not a number): the column ends here -
// d = p = g when this was its first step, d kept otherwise; r is left alone
template <bool VEC>
__global__ __launch_bounds__(kNcgThreads) void ncg_update_kernel(int n, int nch, const NcgCol* __restrict__ cols,
                                                                 const double* __restrict__ part_php,
                                                                 const double* __restrict__ p, const double* __restrict__ hp,
                                                                 double* __restrict__ d, double* __restrict__ r,
                                                                 double* __restrict__ part_rr) {
    const int b = blockIdx.y;
    const NcgCol c = cols[b];
    if (c.done) return;
    const size_t o = (size_t)b * n;
    const double php = ncg_total(part_php + (size_t)b * nch, nch);
    if (!(php > 0.0)) {
        if (c.count != 0) return;
#pragma unroll
        for (int j = 0; j < kNcgPer / 2; ++j) {
            const int i = ncg_at(j);
            if (i >= n) break;
            double p0, p1;
            ncg_ld2<VEC>(p + o, i, n, p0, p1);
            ncg_st2<VEC>(d + o, i, n, p0, p1);
        }
        return;
    }
    const double alpha = c.rr / php;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kNcgPer / 2; ++j) {
        const int i = ncg_at(j);
        if (i >= n) break;
        double p0, p1, h0, h1, d0, d1, r0, r1;
        ncg_ld2<VEC>(p + o, i, n, p0, p1);
        ncg_ld2<VEC>(hp + o, i, n, h0, h1);
        ncg_ld2<VEC>(d + o, i, n, d0, d1);
        ncg_ld2<VEC>(r + o, i, n, r0, r1);
        d0 = fma(alpha, p0, d0);
        d1 = fma(alpha, p1, d1);
        r0 = fma(-alpha, h0, r0);
        r1 = fma(-alpha, h1, r1);
        ncg_st2<VEC>(d + o, i, n, d0, d1);
        ncg_st2<VEC>(r + o, i, n, r0, r1);
        acc = fma(r0, r0, acc);
        if (i + 1 < n) acc = fma(r1, r1, acc);
    }
    const double s = ncg_block_sum(acc);
    if (threadIdx.x == 0) part_rr[(size_t)b * nch + blockIdx.x] = s;
}

// rr = <r, r>; the column ends when rr <= tol2 (p = 0, once), else p = r + (rr / rr_old) p; chunk 0 writes the next record
template <bool VEC>
__global__ __launch_bounds__(kNcgThreads) void ncg_dir_kernel(int n, int nch, const NcgCol* __restrict__ cols,
                                                              NcgCol* __restrict__ next, const double* __restrict__ part_php,
                                                              const double* __restrict__ part_rr, const double* __restrict__ r,
                                                              double* __restrict__ p) {
    const int b = blockIdx.y;
    NcgCol c = cols[b];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (c.done) {
        if (writer) next[b] = c;
        return;
    }
    const size_t o = (size_t)b * n;
    const double php = ncg_total(part_php + (size_t)b * nch, nch);
    const bool npc = !(php > 0.0);
    const double rr = npc ? c.rr : ncg_total(part_rr + (size_t)b * nch, nch);
    const bool fin = npc || !(rr > c.tol2);
    const double beta = rr / c.rr;
#pragma unroll
    for (int j = 0; j < kNcgPer / 2; ++j) {
        const int i = ncg_at(j);
        if (i >= n) break;
        if (fin) {
            ncg_st2<VEC>(p + o, i, n, 0.0, 0.0);
            continue;
        }
        double r0, r1, p0, p1;
        ncg_ld2<VEC>(r + o, i, n, r0, r1);
        ncg_ld2<VEC>(p + o, i, n, p0, p1);
        ncg_st2<VEC>(p + o, i, n, fma(beta, p0, r0), fma(beta, p1, r1));
    }
    if (writer) {
        c.pHp = php;
        c.rr = rr;
        c.count += 1;
        c.done = fin ? 1 : 0;
        c.npc = npc ? 1 : 0;
        next[b] = c;
    }
}

// out_b = x_b + t_b d_b (d == nullptr: out_b = x_b) on the columns with t_b != 0; the others are not written.  out may be x.
template <bool VEC>
__global__ __launch_bounds__(kNcgThreads) void ncg_axpy_kernel(int n, const double* __restrict__ t, const double* x,
                                                               const double* __restrict__ d, double* out) {
    const int b = blockIdx.y;
    const double tb = t[b];
    if (tb == 0.0) return;
    const size_t o = (size_t)b * n;
#pragma unroll
    for (int j = 0; j < kNcgPer / 2; ++j) {
        const int i = ncg_at(j);
        if (i >= n) break;
        double x0, x1;
        ncg_ld2<VEC>(x + o, i, n, x0, x1);
        if (d) {
            double d0, d1;
            ncg_ld2<VEC>(d + o, i, n, d0, d1);
            x0 = fma(tb, d0, x0);
            x1 = fma(tb, d1, x1);
        }
        ncg_st2<VEC>(out + o, i, n, x0, x1);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

Ncg::Ncg(Ctx& c, int n_, int nbmax_) : ctx(c), n(n_), nbmax(nbmax_), nch((n_ + kNcgChunk - 1) / kNcgChunk) {
    PMC_REQUIRE(n >= 1 && nbmax >= 1, "pmc_ncg_create: n and nbatch_max must be at least 1");
    PMC_REQUIRE((uint64_t)n + kNcgChunk < (1ull << 31), "pmc_ncg_create: n exceeds the 32-bit offsets inside a column");
    PMC_REQUIRE(nbmax <= 65535, "pmc_ncg_create: nbatch_max exceeds the grid's second dimension");
    ctx.activate();
    const size_t cnt = (size_t)n * nbmax;
    d.alloc(cnt);
    r.alloc(cnt);
    p.alloc(cnt);
    d.zero(ctx.stream);
    r.zero(ctx.stream);
    p.zero(ctx.stream);
    part_a.alloc((size_t)nch * nbmax);
    part_b.alloc((size_t)nch * nbmax);
    scal.alloc((size_t)nbmax);
    dots.alloc((size_t)nbmax);
    mask.alloc((size_t)nbmax);
    cols.alloc(2 * (size_t)nbmax);
    PMC_HIP(hipMemsetAsync(cols.p, 0, sizeof(NcgCol) * 2 * (size_t)nbmax, ctx.stream));
    PMC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_cols), sizeof(NcgCol) * (size_t)nbmax, hipHostMallocDefault));
    PMC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_dots), sizeof(double) * (size_t)nbmax, hipHostMallocDefault));
    for (Slot& s : slots) {
        PMC_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h), 16 * (size_t)nbmax, hipHostMallocDefault));
        PMC_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    PMC_HIP(hipStreamSynchronize(ctx.stream));
}

Ncg::~Ncg() {
    (void)hipSetDevice(ctx.device);
    (void)hipStreamSynchronize(ctx.stream);
    if (h_cols) (void)hipHostFree(h_cols);
    if (h_dots) (void)hipHostFree(h_dots);
    for (Slot& s : slots) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

// The per-column host arrays of a call (eta, mask, t) go to the device through a ring of pinned slots: a slot is reused only
// after the copies that read it have completed, so no call waits for the stream unless kNcgSlots calls are in flight.
Ncg::Slot& Ncg::next_slot() {
    Slot& s = slots[slot_at];
    slot_at = (slot_at + 1) % kNcgSlots;
    if (s.used) PMC_HIP(hipEventSynchronize(s.ev));
    s.used = true;
    return s;
}

// a caller's array on the device: itself, the workspace's own vectors included, or a staged copy of a host array
const double* Ncg::in(const double* a, int nb, int memspace, int slot) {
    if (memspace == PMC_MEM_DEVICE || a == d.p || a == r.p || a == p.p) return a;
    const size_t cnt = (size_t)n * nb;
    stage[slot].ensure((size_t)n * nbmax);
    PMC_HIP(hipMemcpyAsync(stage[slot].p, a, sizeof(double) * cnt, hipMemcpyHostToDevice, ctx.stream));
    return stage[slot].p;
}

void Ncg::check(int nb, int memspace, const char* what) const {
    PMC_REQUIRE(nb >= 1 && nb <= nbmax, std::string(what) + ": nb outside [1, nbatch_max]");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, std::string(what) + ": bad memspace");
}

void Ncg::begin(int nb, const double* g, const double* eta, const int32_t* active, int memspace) {
    check(nb, memspace, "pmc_ncg_begin");
    PMC_REQUIRE(g != nullptr && eta != nullptr, "pmc_ncg_begin: NULL argument");
    for (int b = 0; b < nb; ++b) PMC_REQUIRE(eta[b] >= 0.0, "pmc_ncg_begin: eta must not be negative");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const double* g_d = in(g, nb, memspace, 0);
    Slot& up = next_slot();
    double* h_eta = reinterpret_cast<double*>(up.h);
    int32_t* h_on = reinterpret_cast<int32_t*>(up.h + 8 * (size_t)nbmax);
    for (int b = 0; b < nb; ++b) {
        h_eta[b] = eta[b];
        h_on[b] = (!active || active[b] != 0) ? 1 : 0;
    }
    PMC_HIP(hipMemcpyAsync(mask.p, h_on, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
    PMC_HIP(hipMemcpyAsync(scal.p, h_eta, sizeof(double) * nb, hipMemcpyHostToDevice, st));
    PMC_HIP(hipEventRecord(up.ev, st));
    const dim3 grid((unsigned)nch, (unsigned)nb);
    if (n % 2 == 0 && aligned16(g_d))
        ncg_begin_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, nch, g_d, mask.p, d.p, r.p, p.p, part_a.p);
    else
        ncg_begin_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, nch, g_d, mask.p, d.p, r.p, p.p, part_a.p);
    PMC_HIP(hipGetLastError());
    cur = 0;
    ncg_begin_cols_kernel<<<(unsigned)((nb + 63) / 64), 64, 0, st>>>(nb, nch, part_a.p, scal.p, mask.p, cols.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(2);
    nb_cur = nb;
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipStreamSynchronize(st));     // the staged copy of g has been read
}

void Ncg::step(int nb, const double* hp, int memspace) {
    check(nb, memspace, "pmc_ncg_step");
    PMC_REQUIRE(hp != nullptr, "pmc_ncg_step: Hp is NULL");
    PMC_REQUIRE(nb == nb_cur, "pmc_ncg_step: nb differs from the pmc_ncg_begin this step continues");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const double* h_d = in(hp, nb, memspace, 0);
    const NcgCol* c0 = cols.p + (size_t)cur * nbmax;
    NcgCol* c1 = cols.p + (size_t)(cur ^ 1) * nbmax;
    const dim3 grid((unsigned)nch, (unsigned)nb);
    if (n % 2 == 0 && aligned16(h_d)) {
        ncg_dot_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, p.p, h_d, part_a.p);
        ncg_update_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, part_a.p, p.p, h_d, d.p, r.p, part_b.p);
        ncg_dir_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, c1, part_a.p, part_b.p, r.p, p.p);
    } else {
        ncg_dot_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, p.p, h_d, part_a.p);
        ncg_update_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, part_a.p, p.p, h_d, d.p, r.p, part_b.p);
        ncg_dir_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, nch, c0, c1, part_a.p, part_b.p, r.p, p.p);
    }
    PMC_HIP(hipGetLastError());
    count_kernel_launches(3);
    cur ^= 1;
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipStreamSynchronize(st));
}

void Ncg::status(int nb, double* rr, int32_t* count, int32_t* done, int32_t* npc) {
    PMC_REQUIRE(nb >= 1 && nb <= nbmax, "pmc_ncg_status: nb outside [1, nbatch_max]");
    ctx.activate();
    hipStream_t st = ctx.stream;
    PMC_HIP(hipMemcpyAsync(h_cols, cols.p + (size_t)cur * nbmax, sizeof(NcgCol) * nb, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < nb; ++b) {
        if (rr) rr[b] = h_cols[b].rr;
        if (count) count[b] = h_cols[b].count;
        if (done) done[b] = h_cols[b].done;
        if (npc) npc[b] = h_cols[b].npc;
    }
}

void Ncg::axpy(int nb, const double* t, const double* x, const double* dd, double* out, int memspace) {
    check(nb, memspace, "pmc_ncg_axpy_cols");
    PMC_REQUIRE(t != nullptr && x != nullptr && out != nullptr, "pmc_ncg_axpy_cols: NULL argument");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const bool out_own = out == d.p || out == r.p || out == p.p;
    const bool host_out = memspace == PMC_MEM_HOST && !out_own;
    const double* x_d = in(x, nb, memspace, 0);
    const double* d_d = dd ? in(dd, nb, memspace, 1) : nullptr;
    double* o_d = out;
    if (host_out) {       // the columns that are not written keep the caller's values
        o_d = x == out ? stage[0].p : const_cast<double*>(in(out, nb, memspace, 2));
    }
    Slot& up = next_slot();
    std::memcpy(up.h, t, sizeof(double) * nb);
    PMC_HIP(hipMemcpyAsync(scal.p, up.h, sizeof(double) * nb, hipMemcpyHostToDevice, st));
    PMC_HIP(hipEventRecord(up.ev, st));
    const dim3 grid((unsigned)nch, (unsigned)nb);
    if (n % 2 == 0 && aligned16(x_d) && aligned16(o_d) && (!d_d || aligned16(d_d)))
        ncg_axpy_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, scal.p, x_d, d_d, o_d);
    else
        ncg_axpy_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, scal.p, x_d, d_d, o_d);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    if (host_out) PMC_HIP(hipMemcpyAsync(out, o_d, sizeof(double) * (size_t)n * nb, hipMemcpyDeviceToHost, st));
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipStreamSynchronize(st));
}

void Ncg::dot(int nb, const double* a, const double* b, double* out_host, int memspace) {
    check(nb, memspace, "pmc_ncg_dot_cols");
    PMC_REQUIRE(a != nullptr && b != nullptr && out_host != nullptr, "pmc_ncg_dot_cols: NULL argument");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const double* a_d = in(a, nb, memspace, 0);
    const double* b_d = b == a ? a_d : in(b, nb, memspace, 1);
    const dim3 grid((unsigned)nch, (unsigned)nb);
    if (n % 2 == 0 && aligned16(a_d) && aligned16(b_d))
        ncg_dot_kernel<true><<<grid, kNcgThreads, 0, st>>>(n, nch, nullptr, a_d, b_d, part_a.p);
    else
        ncg_dot_kernel<false><<<grid, kNcgThreads, 0, st>>>(n, nch, nullptr, a_d, b_d, part_a.p);
    PMC_HIP(hipGetLastError());
    ncg_dot_final_kernel<<<(unsigned)((nb + 63) / 64), 64, 0, st>>>(nb, nch, part_a.p, dots.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(2);
    PMC_HIP(hipMemcpyAsync(h_dots, dots.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < nb; ++i) out_host[i] = h_dots[i];
}

}  // namespace pmc

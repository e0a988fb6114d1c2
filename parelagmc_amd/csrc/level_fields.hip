// Field accumulators of one level of a multilevel estimator (pmc_level_fields_*, DESIGN.md sections 12 and 13).
//
//   accumulate_kernel: one thread per fine element i walks the launch's columns in ascending realization id, gathers the
//     coarse partner's pressure p_c[b n_c + parent[i]] (a P0 injection: every fine element has exactly one parent) and adds
//     d = p - p_c, d^2 and p^2 - p_c^2 into (sum, compensation) pairs with Neumaier's two-sum (neumaier.hpp, shared with
//     field_stats.hip).  Every element sees the same sequence of additions however the realizations were split into calls,
//     so the accumulators are bit-identical for every split.  Products are rounded before they are summed (fp contraction
//     off).  On the coarsest level (no partner) p_c = 0: d = p and the third pair equals the second.
//   accumulate_weighted_kernel: the same walk with per-column weights (the ratio managers' posterior field estimates,
//     DESIGN.md section 13).
// fp64 and bandwidth-bound: per realization the fine column, the coarse column (gathered, n_c distinct entries), and the six
// pairs once per launch.
#include "handles.hpp"
#include "kernels.hpp"
#include "neumaier.hpp"

#include <cmath>
#include <string>

namespace pmc {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 8;   // columns whose loads are issued together

// acc = [sum d | comp | sum d^2 | comp | sum p^2 - p_c^2 | comp] (n each); pc == nullptr: no coarse partner
__global__ __launch_bounds__(kThreads) void accumulate_kernel(int n, int nc, int nb, const double* __restrict__ pf,
                                                              const double* __restrict__ pc, const int* __restrict__ parent,
                                                              double* __restrict__ acc) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    double s1 = acc[i], c1 = acc[N + i], s2 = acc[2 * N + i], c2 = acc[3 * N + i], s3 = acc[4 * N + i], c3 = acc[5 * N + i];
    const int j = pc ? parent[i] : 0;
    for (int c0 = 0; c0 < nb; c0 += kUnroll) {
        double x[kUnroll], y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool in = c0 + u < nb;
            x[u] = in ? pf[(size_t)(c0 + u) * n + i] : 0.0;
            y[u] = in && pc ? pc[(size_t)(c0 + u) * nc + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (c0 + u >= nb) break;
            const double d = x[u] - y[u];
            two_sum(s1, c1, d);
            const double d2 = d * d;
            two_sum(s2, c2, d2);
            const double pp = x[u] * x[u];
            const double cc = y[u] * y[u];
            const double q = pp - cc;
            two_sum(s3, c3, q);
        }
    }
    acc[i] = s1;
    acc[N + i] = c1;
    acc[2 * N + i] = s2;
    acc[3 * N + i] = c2;
    acc[4 * N + i] = s3;
    acc[5 * N + i] = c3;
}

// The same walk with per-column weights w[b], w_c[b] (the posterior field estimates of the ratio managers, DESIGN.md
// section 13): a = w x, b = w_c y, d = a - b, d^2 and a x - b y.  The weights of a launch travel by value in the kernel
// arguments (uniform across the launch, so they are read as scalars), which leaves no host staging buffer that a later
// chunk could overwrite under an in-flight copy.  With every weight 1.0 each product is exact (a = x, a x = x x), so the
// sums equal accumulate_kernel's bit for bit.
constexpr int kWeightedCols = 64;   // columns (and weight pairs) per launch: 1 KiB of weights in the kernel arguments
struct ColumnWeights {
    double w[kWeightedCols], wc[kWeightedCols];
};
__global__ __launch_bounds__(kThreads) void accumulate_weighted_kernel(int n, int nc, int nb, const double* __restrict__ pf,
                                                                       const double* __restrict__ pc,
                                                                       const int* __restrict__ parent,
                                                                       double* __restrict__ acc, const ColumnWeights cw) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    double s1 = acc[i], c1 = acc[N + i], s2 = acc[2 * N + i], c2 = acc[3 * N + i], s3 = acc[4 * N + i], c3 = acc[5 * N + i];
    const int j = pc ? parent[i] : 0;
    for (int c0 = 0; c0 < nb; c0 += kUnroll) {
        double x[kUnroll], y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool in = c0 + u < nb;
            x[u] = in ? pf[(size_t)(c0 + u) * n + i] : 0.0;
            y[u] = in && pc ? pc[(size_t)(c0 + u) * nc + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (c0 + u >= nb) break;
            const double a = cw.w[c0 + u] * x[u];
            const double b = cw.wc[c0 + u] * y[u];
            const double d = a - b;
            two_sum(s1, c1, d);
            const double d2 = d * d;
            two_sum(s2, c2, d2);
            const double pp = a * x[u];
            const double cc = b * y[u];
            const double q = pp - cc;
            two_sum(s3, c3, q);
        }
    }
    acc[i] = s1;
    acc[N + i] = c1;
    acc[2 * N + i] = s2;
    acc[3 * N + i] = c2;
    acc[4 * N + i] = s3;
    acc[5 * N + i] = c3;
}

void copy_in(DevBuf<double>& dst, const double* src, size_t cnt, hipStream_t st) {
    dst.ensure(cnt);
    PMC_HIP(hipMemcpyAsync(dst.p, src, cnt * sizeof(double), hipMemcpyHostToDevice, st));
}

}  // namespace

LevelFields::LevelFields(Ctx& c, const Darcy& d, int level_, bool coupled_)
    : ctx(c), level(level_), n(0), nc(0), coupled(coupled_) {
    PMC_REQUIRE(level >= 0 && level < d.n_mc, "level fields: level out of range");
    PMC_REQUIRE(!coupled || level + 1 < d.n_mc,
                "level fields: coupled requires a coarse partner level + 1 < number of Monte Carlo levels");
    PMC_REQUIRE(ctx.device == d.ctx.device, "level fields: ctx and the Darcy handle are on different devices");
    n = d.lv[level].n_p;
    if (coupled) {
        PMC_REQUIRE(level < (int)d.P_host.size() && d.P_host[level].nrows == n,
                    "level fields: the Darcy handle holds no pressure prolongator for the level");
        const HostCsr& P = d.P_host[level];
        nc = P.ncols;
        parent_host.assign(n, -1);
        for (int i = 0; i < n; ++i) {
            for (int p = P.rowptr[i]; p < P.rowptr[i + 1]; ++p) {
                if (P.vals[p] == 0.0) continue;   // explicitly stored zeros are no coupling
                PMC_REQUIRE(P.vals[p] == 1.0 && parent_host[i] < 0 && P.colind[p] >= 0 && P.colind[p] < nc,
                            "level fields: row " + std::to_string(i) + " of P(" + std::to_string(level) +
                                ") is not a single 1.0 (the pressure estimates need a P0 injection)");
                parent_host[i] = P.colind[p];
            }
            PMC_REQUIRE(parent_host[i] >= 0, "level fields: row " + std::to_string(i) + " of P(" + std::to_string(level) +
                                                 ") is not a single 1.0 (the pressure estimates need a P0 injection)");
        }
    }
    ctx.activate();
    hipStream_t st = ctx.stream;
    if (coupled) parent.upload(parent_host, st);
    acc.alloc((size_t)6 * n);
    acc.zero(st);
    PMC_HIP(hipStreamSynchronize(st));
}

void LevelFields::reset() {
    ctx.activate();
    acc.zero(ctx.stream);
    PMC_HIP(hipStreamSynchronize(ctx.stream));
    count = 0;
}

void LevelFields::accumulate_device(int nbatch, const double* pf, const double* pc) {
    accumulate_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, ctx.stream>>>(n, nc, nbatch, pf, pc,
                                                                                             parent.p, acc.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

void LevelFields::accumulate(int nbatch, const double* p_fine, const double* p_coarse, int memspace) {
    PMC_REQUIRE(nbatch >= 1 && p_fine != nullptr, "level fields accumulate: bad arguments");
    PMC_REQUIRE(coupled == (p_coarse != nullptr),
                coupled ? "level fields accumulate: p_coarse is NULL on a coupled level"
                        : "level fields accumulate: p_coarse given on a level created without a coarse partner");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "level fields accumulate: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    if (memspace == PMC_MEM_DEVICE) {   // asynchronous on ctx's stream
        accumulate_device(nbatch, p_fine, p_coarse);
    } else {
        const int cols = 64;   // host input: staged 64 realizations at a time (the additions are the same for every split)
        for (int done = 0; done < nbatch;) {
            const int nb = std::min(cols, nbatch - done);
            copy_in(pbuf, p_fine + (size_t)done * n, (size_t)nb * n, st);
            if (coupled) copy_in(cbuf, p_coarse + (size_t)done * nc, (size_t)nb * nc, st);
            accumulate_device(nb, pbuf.p, coupled ? cbuf.p : nullptr);
            PMC_HIP(hipStreamSynchronize(st));   // the staging buffers are overwritten by the next chunk's copies
            done += nb;
        }
    }
    count += nbatch;
}

void LevelFields::accumulate_weighted_device(int nbatch, const double* pf, const double* wf, const double* pc,
                                             const double* wc) {
    for (int done = 0; done < nbatch;) {
        const int nb = std::min(kWeightedCols, nbatch - done);
        ColumnWeights cw;
        for (int b = 0; b < kWeightedCols; ++b) {
            cw.w[b] = b < nb ? wf[done + b] : 0.0;
            cw.wc[b] = b < nb && wc ? wc[done + b] : 0.0;   // no coarse partner: b = 0 * 0
        }
        accumulate_weighted_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, ctx.stream>>>(
            n, nc, nb, pf + (size_t)done * n, pc ? pc + (size_t)done * nc : nullptr, parent.p, acc.p, cw);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
        done += nb;
    }
}

void LevelFields::accumulate_weighted(int nbatch, const double* p_fine, const double* w_fine, const double* p_coarse,
                                      const double* w_coarse, int memspace) {
    PMC_REQUIRE(nbatch >= 1 && p_fine != nullptr && w_fine != nullptr, "level fields accumulate_weighted: bad arguments");
    PMC_REQUIRE(coupled == (p_coarse != nullptr) && coupled == (w_coarse != nullptr),
                coupled ? "level fields accumulate_weighted: p_coarse / w_coarse is NULL on a coupled level"
                        : "level fields accumulate_weighted: p_coarse / w_coarse given on a level created without a coarse "
                          "partner");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "level fields accumulate_weighted: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    if (memspace == PMC_MEM_DEVICE) {   // asynchronous on ctx's stream; the weights are consumed at launch
        accumulate_weighted_device(nbatch, p_fine, w_fine, p_coarse, w_coarse);
    } else {
        const int cols = kWeightedCols;   // host input: staged as accumulate() stages it
        for (int done = 0; done < nbatch;) {
            const int nb = std::min(cols, nbatch - done);
            copy_in(pbuf, p_fine + (size_t)done * n, (size_t)nb * n, st);
            if (coupled) copy_in(cbuf, p_coarse + (size_t)done * nc, (size_t)nb * nc, st);
            accumulate_weighted_device(nb, pbuf.p, w_fine + done, coupled ? cbuf.p : nullptr,
                                       coupled ? w_coarse + done : nullptr);
            PMC_HIP(hipStreamSynchronize(st));   // the staging buffers are overwritten by the next chunk's copies
            done += nb;
        }
    }
    count += nbatch;
}

void LevelFields::read_sums(double* sums, int64_t* cnt, int memspace) {
    PMC_REQUIRE(sums != nullptr, "level fields read_sums: sums is NULL");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "level fields read_sums: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    PMC_HIP(hipMemcpyAsync(sums, acc.p, sizeof(double) * acc.n,
                           memspace == PMC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    PMC_HIP(hipStreamSynchronize(st));
    if (cnt) *cnt = count;
}

}  // namespace pmc

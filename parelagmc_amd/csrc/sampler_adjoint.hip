// Adjoint of the SPDE samplers' Eval (pmc_sampler_eval_adjoint).
//
// Eval(level, xi_level) is s_out = f(O S R D xi): D = -g diag(w_sqrt[xi_level]), R = Ps[level-1]^T ... Ps[xi_level]^T, S the
// s-block of A_level^-1 (symmetric; the saddle-point and the hybridized solver compute the same S), O the output map
// (identity, gather, diag(inv_w) Gt), f = exp on a lognormal handle.  So
//     dJ/dxi = D R^T S O^T (v o f'),   f' = s_out,
// i.e. the level's own solve with O^T (v o s_out) in the s-rows of the right-hand side, prolongated to xi_level and scaled.
// The solve IS Eval's (Sampler::solve_system, zero guess) under a graph key of its own.  The factor -g is applied in the
// seed: everything after it is linear.
//
// Tangent of Eval (pmc_sampler_eval_tangent): ds_out = f' o (O S R D v), the linear part of Eval applied
// to the direction - Eval itself with the exp() of its stores switched off, so the same solve from a zero guess at the same
// launch widths on every handle kind - times s_out, the f' of a lognormal handle, when the caller hands it over.
//
// Conditioned handles: with a conditioner attached that has derivatives enabled, Gamma = I - K A^-1 H
// stands between L = O S R D and f.  The tangent runs Eval's hook on its homogeneous map (Sampler::cond_tangent_width); the
// adjoint forms w = Gamma^T (v o f') per launch (Conditioner::apply_adjoint_device) and takes the path above with v := w,
// s_out := NULL.  Without the opt-in both entries refuse the handle, as they always did.
#include "handles.hpp"

namespace pmc {

namespace {
constexpr uint64_t kAdjointKey = 0xad;   // graph-key salt: a captured graph of a forward Eval is never replayed here

// grad[b][:] -= xi[b][:] and logprior[b] = -|xi_b|^2 / 2: one workgroup per realization, a fixed summation order (strided
// partial sums per thread, then a tree over the workgroup), so the value does not depend on how a call was split
constexpr int kPriorThreads = 256;
__global__ __launch_bounds__(kPriorThreads) void prior_gradient_kernel(int n, const double* __restrict__ xi,
                                                                       double* __restrict__ grad, double* __restrict__ logprior) {
    __shared__ double red[kPriorThreads];
    const size_t o = (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kPriorThreads) {
        const double x = xi[o + i];
        grad[o + i] -= x;
        acc = fma(x, x, acc);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kPriorThreads / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) logprior[blockIdx.x] = -0.5 * red[0];
}
}

namespace {
// out[i] *= s[i]: the f' = s_out of a lognormal handle on the tangent
__global__ void mul_inplace_kernel(size_t total, const double* __restrict__ s, double* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) out[t] *= s[t];
}
}

void Sampler::eval_tangent(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* ds_out,
                           int memspace, pmc_stats* stats) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "EvalTangent: level out of range");
    PMC_REQUIRE(xi_level >= 0 && xi_level <= level, "EvalTangent: xi_level must satisfy 0 <= xi_level <= level");
    PMC_REQUIRE(nbatch >= 1 && v != nullptr && ds_out != nullptr, "EvalTangent: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "EvalTangent: bad memspace");
    PMC_REQUIRE(s_out == nullptr || lognormal, "EvalTangent: s_out given on a handle that is not lognormal");
    PMC_REQUIRE(cond == nullptr || cond->derivs,
                "EvalTangent: a conditioner is attached (pmc_sampler_set_conditioner) without derivatives enabled; call "
                "pmc_conditioner_enable_derivatives for the tangent of the conditional field");
    // Eval of v with the exp() of the stores off: the flag is a plain argument of every store Eval ends in
    struct FlagOff {
        bool& f;
        const bool keep;
        explicit FlagOff(bool& flag) : f(flag), keep(flag) { f = false; }
        ~FlagOff() { f = keep; }
    };
    // ... and with the conditioner's hook on its homogeneous map dg - K A^-1 H dg, launch by launch as in Eval
    struct WidthSet {
        int& w;
        WidthSet(int& width, int value) : w(width) { w = value; }
        ~WidthSet() { w = 0; }
    };
    {
        FlagOff off(lognormal);
        WidthSet hom(cond_tangent_width, cond ? nbatch : 0);
        eval(level, xi_level, nbatch, v, ds_out, nullptr, 0, false, nullptr, memspace, stats);
    }
    if (!s_out) return;
    const size_t total = (size_t)lv[level].out_size * nbatch;
    if (memspace == PMC_MEM_HOST) {           // Eval has synchronised; host arrays are staged, so the product is the host's
        for (size_t i = 0; i < total; ++i) ds_out[i] *= s_out[i];
        return;
    }
    hipStream_t st = ctx.stream;
    mul_inplace_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(total, s_out, ds_out);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

void Sampler::prior_gradient(int n, int nbatch, const double* xi, double* grad, double* logprior, int memspace) {
    PMC_REQUIRE(n >= 1 && nbatch >= 1 && xi != nullptr && grad != nullptr, "logprior_gradient: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "logprior_gradient: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t cnt = (size_t)n * nbatch;
    // the handle's own buffers (grown, never shrunk): a call per MCMC step allocates nothing
    adj_lp.ensure((size_t)nbatch);
    const double* xi_d = xi;
    double* g_d = grad;
    if (memspace == PMC_MEM_HOST) {
        stage_in.ensure(cnt);
        stage_out.ensure(cnt);
        PMC_HIP(hipMemcpyAsync(stage_in.p, xi, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        PMC_HIP(hipMemcpyAsync(stage_out.p, grad, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        xi_d = stage_in.p;
        g_d = stage_out.p;
    }
    prior_gradient_kernel<<<(unsigned)nbatch, kPriorThreads, 0, st>>>(n, xi_d, g_d, adj_lp.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipMemcpyAsync(grad, stage_out.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
    // the scalars cross to the host only when asked for; a device-memory call without them does not synchronise
    if (logprior) PMC_HIP(hipMemcpyAsync(logprior, adj_lp.p, sizeof(double) * nbatch, hipMemcpyDeviceToHost, st));
    if (logprior || memspace == PMC_MEM_HOST) PMC_HIP(hipStreamSynchronize(st));
}

namespace {
// hv[i] += v[i]: the N(0, I) prior's part of a Hessian action in the white noise
__global__ void add_inplace_kernel(size_t total, const double* __restrict__ v, double* __restrict__ hv) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) hv[t] += v[t];
}
}

void Sampler::prior_hessvec(int n, int nbatch, const double* v, double* hv, int memspace) {
    PMC_REQUIRE(n >= 1 && nbatch >= 1 && v != nullptr && hv != nullptr, "logprior_hessvec: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "logprior_hessvec: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t cnt = (size_t)n * nbatch;
    const double* v_d = v;
    double* h_d = hv;
    if (memspace == PMC_MEM_HOST) {
        stage_in.ensure(cnt);
        stage_out.ensure(cnt);
        PMC_HIP(hipMemcpyAsync(stage_in.p, v, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        PMC_HIP(hipMemcpyAsync(stage_out.p, hv, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        v_d = stage_in.p;
        h_d = stage_out.p;
    }
    add_inplace_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, st>>>(cnt, v_d, h_d);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    if (memspace == PMC_MEM_HOST) {
        PMC_HIP(hipMemcpyAsync(hv, stage_out.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

namespace {
template <class T>
std::vector<T> read_back(const DevBuf<T>& b, size_t cnt, hipStream_t st) {
    std::vector<T> h(cnt);
    if (cnt) PMC_HIP(hipMemcpyAsync(h.data(), b.p, sizeof(T) * cnt, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    return h;
}
// A^T diag(rowscale) of a shared-value SELL matrix as host CSR, read back from the device (padding slots carry the value 0)
HostCsr sell_transpose_host(const Sell& A, const std::vector<double>& rowscale, hipStream_t st) {
    const std::vector<int> off = read_back(A.slice_off, (size_t)A.nslices + 1, st);
    const std::vector<int> cols = read_back(A.cols, (size_t)A.nslots, st);
    const std::vector<double> vals = read_back(A.vals, (size_t)A.nslots, st);
    HostCsr O;   // A diag-scaled, row by row, then transposed
    O.nrows = A.nrows;
    O.ncols = A.ncols;
    O.rowptr.assign((size_t)A.nrows + 1, 0);
    for (int r = 0; r < A.nrows; ++r) {
        const int s = r / 64, lane = r % 64;
        const int w = (off[(size_t)s + 1] - off[(size_t)s]) / 64;
        for (int j = 0; j < w; ++j) {
            const size_t slot = (size_t)off[(size_t)s] + (size_t)j * 64 + lane;
            if (vals[slot] == 0.0) continue;
            O.colind.push_back(cols[slot]);
            O.vals.push_back(vals[slot] * rowscale[(size_t)r]);
        }
        O.rowptr[(size_t)r + 1] = (int)O.colind.size();
    }
    return csr_transpose(O);
}
}

// device side of the adjoint of `level`, built at the first adjoint call from what setup left on the device (a handle that
// never asks allocates nothing, on the host or on the device)
void Sampler::ensure_adjoint(int level) {
    SamplerLevel& d = lv[level];
    if (d.has_adj) return;
    hipStream_t st = ctx.stream;
    std::vector<double> z;
    if (hybrid) {   // z = zw_sqrt / w_sqrt, the two exactly as setup uploaded them
        std::vector<double> zw((size_t)d.n_s), wsq((size_t)d.n_s);
        PMC_HIP(hipMemcpyAsync(zw.data(), d.zw_sqrt.p, sizeof(double) * d.n_s, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(wsq.data(), d.w_sqrt.p, sizeof(double) * d.n_s, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        z.resize((size_t)d.n_s);
        for (int i = 0; i < d.n_s; ++i) z[(size_t)i] = zw[(size_t)i] / wsq[(size_t)i];
        d.adj_z.upload(z, st);
    }
    if (d.proj != PMC_PROJ_NONE) {
        HostCsr Ot;
        if (d.proj == PMC_PROJ_GATHER) {   // O (out_size x n_s): row j is e_idx[j]
            HostCsr O;
            O.nrows = d.out_size;
            O.ncols = d.n_s;
            O.rowptr.resize((size_t)d.out_size + 1);
            for (int j = 0; j <= d.out_size; ++j) O.rowptr[(size_t)j] = j;
            O.colind = read_back(d.gather, (size_t)d.out_size, st);
            O.vals.assign((size_t)d.out_size, 1.0);
            Ot = csr_transpose(O);
        } else {                           // O = diag(inv_w) Gt, both as set_projection uploaded them
            Ot = sell_transpose_host(d.Gt, read_back(d.inv_w, (size_t)d.out_size, st), st);
        }
        if (hybrid)
            for (int i = 0; i < Ot.nrows; ++i)
                for (int p = Ot.rowptr[(size_t)i]; p < Ot.rowptr[(size_t)i + 1]; ++p) Ot.vals[(size_t)p] *= z[(size_t)i];
        sell_build(d.adj_Ot, Ot, true, false, st);
    }
    PMC_HIP(hipStreamSynchronize(st));
    d.has_adj = true;
}

void Sampler::eval_adjoint_chunk(int level, int xi_level, int nb, const double* v_d, const double* s_d, double* grad_d,
                                 pmc_stats* stats) {
    hipStream_t st = ctx.stream;
    SamplerLevel& d = lv[level];
    const int n_u = d.n_u, n_s = d.n_s;
    ensure(level, nb);
    if (stats) ctx.phase_mark(0);
    // s-rows of the right-hand side: q = -g O^T (v o s_out); the hybridized solve wants z q there (fz of eval_chunk)
    double* rhs_s = rhs.p + (size_t)n_u * nb;
    if (d.proj == PMC_PROJ_NONE) {
        k::seed_interleave(st, nb, n_s, v_d, s_d, hybrid ? d.adj_z.p : nullptr, -g, rhs_s);
    } else {
        k::seed_interleave(st, nb, d.out_size, v_d, s_d, nullptr, -g, tA.p);
        k::spmm(st, nb, view(d.adj_Ot), tA.p, rhs_s, false, nullptr, nullptr);
    }
    if (hybrid) {
        // rhs = Gz (z q) = G q; lambda = H^-1 rhs; S q = z q - G^T lambda: eval_chunk's solve and back-substitution
        const RhsFn make_rhs = multiplier_rhs(level, rhs_s);
        if (stats) ctx.phase_mark(1);
        solve_system(level, nb, true, 0, n_u, stats, &make_rhs, kAdjointKey);
        k::residual(st, nb, view(d.Gl), rhs_s, sol.p, sol.p + (size_t)n_u * nb);
    } else {
        k::fill(st, (size_t)n_u * nb, rhs.p, 0.0);
        if (stats) ctx.phase_mark(1);
        solve_system(level, nb, true, n_u, n_s, stats, nullptr, kAdjointKey);
    }
    // R^T: down the levels with the prolongators, then the row scale of D
    const double* fine = level_walk(nb, level, xi_level, sol.p + (size_t)n_u * nb, nullptr);
    k::deinterleave(st, nb, lv[xi_level].n_s, fine, nullptr, lv[xi_level].w_sqrt.p, false, grad_d);
}

void Sampler::eval_adjoint(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* grad_xi,
                           int memspace, pmc_stats* stats) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "EvalAdjoint: level out of range");
    PMC_REQUIRE(xi_level >= 0 && xi_level <= level, "EvalAdjoint: xi_level must satisfy 0 <= xi_level <= level");
    PMC_REQUIRE(nbatch >= 1 && v != nullptr && grad_xi != nullptr, "EvalAdjoint: bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "EvalAdjoint: bad memspace");
    PMC_REQUIRE(s_out == nullptr || lognormal, "EvalAdjoint: s_out given on a handle that is not lognormal");
    PMC_REQUIRE(cond == nullptr || cond->derivs,
                "EvalAdjoint: a conditioner is attached (pmc_sampler_set_conditioner) without derivatives enabled; call "
                "pmc_conditioner_enable_derivatives for the adjoint of the conditional field");
    if (kl) {
        eval_adjoint_kl(level, xi_level, nbatch, v, s_out, grad_xi, memspace, stats);
        return;
    }
    ctx.activate();
    ensure_adjoint(level);
    const int n_xi = lv[xi_level].n_s, n_out = lv[level].out_size;
    const int width = launch_width(level);   // the launch widths of Sampler::eval
    ensure(level, first_chunk(width, nbatch));   // the staging buffers are among what it sizes
    enum { V, S, GRAD, STATS };
    for_chunks(ctx, width, nbatch, memspace, memspace == PMC_MEM_HOST,
               {ChunkArg::in(v, (size_t)n_out, stage_in), ChunkArg::in(s_out, (size_t)n_out, stage_emb),
                ChunkArg::out(grad_xi, (size_t)n_xi, stage_out), ChunkArg::stats(stats)},
               [&](const Chunk& c) {
                   const double* v_d = c.at<double>(V);
                   const double* s_d = c.at<double>(S);
                   if (cond) {   // w = Gamma^T (v o f') per launch, then the unconditioned path with v := w, s_out := NULL
                       cond->hook_w.ensure((size_t)n_out * c.nb);
                       cond->apply_adjoint_device(level, c.nb, v_d, s_d, cond->hook_w.p, nbatch);
                       v_d = cond->hook_w.p;
                       s_d = nullptr;
                   }
                   eval_adjoint_chunk(level, xi_level, c.nb, v_d, s_d, c.at<double>(GRAD), c.at<pmc_stats>(STATS));
               });
}

}  // namespace pmc

// Truncated Karhunen-Loeve sampler (the reference's KLSampler, src/KLSampler.cpp:144-223): s = Phi_level Lambda^1/2 xi[:m].
//
// A launch of nb realizations is one fp64 GEMM  S^T (nb x n) = (Lambda^1/2 Xi)^T (nb x m) . Phi^T (m x n), Phi column-major.
// Setup folds sqrt(lambda) into Phi (kl_phi = Phi diag(sqrt(lambda))) and projects it to the coarser levels on the device.
//   nb > 4: kl_mfma_kernel, v_mfma_f64_16x16x4f64.  A workgroup owns 64 field rows and up to 128 realizations; Phi streams
//           from HBM once per 128 realizations (each workgroup reads its row block once), Xi is staged through a
//           double-buffered LDS tile in chunks of kKc modes, the next chunk of Phi and Xi in registers while one is multiplied.
//   nb <= 4: kl_gemv_kernel, pure bandwidth: one field row per lane, the modes split over the 4 waves of a workgroup.
#include "handles.hpp"
#include "kernels.hpp"

#include <cmath>

namespace pmc {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kKc = 32;          // modes per LDS stage of the MFMA kernel
constexpr int kWaves = 4;        // waves per workgroup (both kernels); 16 field rows per wave in the MFMA kernel
constexpr int kMaxTiles = 8;     // realization tiles of 16 per MFMA workgroup: 128 realizations

// f64 16x16x4 MFMA operand / result maps (cdna_hip_programming.md §3, checked in tests/test_gpu_kl.py with exact integer data):
//   A (16 x 4): lane l holds A[l & 15][l >> 4];   B (4 x 16): lane l holds B[l >> 4][l & 15];
//   D (16 x 16): lane l, register r holds D[(l >> 4) + 4 r][l & 15].
// Here A = (Lambda^1/2 Xi)^T (rows: realizations), B = Phi^T (columns: field rows), so a lane's results are 4 realizations
// of ONE field row and each store of a register is 16 consecutive doubles of one realization.
template <int NT>
__global__ __launch_bounds__(64 * kWaves, 2) void kl_mfma_kernel(int n, int m, int nb, const double* __restrict__ phi,
                                                               const double* __restrict__ xi, int n_xi, double* __restrict__ s,
                                                               double* __restrict__ emb, int lognormal) {
    constexpr int kStage = 16 * NT * kKc / (64 * kWaves);   // xi entries each thread stages per chunk
    __shared__ double xs[2][16 * NT][kKc + 1];              // double-buffered: one barrier per chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (blockIdx.x * kWaves + wave) * 16 + (lane & 15);
    const int kq = lane >> 4;
    const int b0 = blockIdx.y * 16 * NT;
    const bool row_ok = i < n;
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double bcur[kKc / 4], bnxt[kKc / 4], xr[kStage];
    // chunk c: Phi rows k = c kKc + 4 kk + kq of this lane's field row; xi entries e = threadIdx.x + j 64 kWaves of the
    // [16 NT realizations][kKc modes] tile (consecutive threads read consecutive modes of one realization)
    auto load_chunk = [&](int c, double* bq, double* xq) {
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) {
            const int k = c * kKc + 4 * kk + kq;
            bq[kk] = (row_ok && k < m) ? phi[(size_t)k * n + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kStage; ++j) {
            const int e = threadIdx.x + j * 64 * kWaves;
            const int b = b0 + e / kKc, k = c * kKc + e % kKc;
            xq[j] = (b < nb && k < m) ? xi[(size_t)b * n_xi + k] : 0.0;
        }
    };
    load_chunk(0, bcur, xr);
    const int nchunks = (m + kKc - 1) / kKc;
    for (int c = 0; c < nchunks; ++c) {
        double (*x)[kKc + 1] = xs[c & 1];
#pragma unroll
        for (int j = 0; j < kStage; ++j) {
            const int e = threadIdx.x + j * 64 * kWaves;
            x[e / kKc][e % kKc] = xr[j];
        }
        // buffer c & 1 was last read in chunk c - 2; every wave has passed the barrier of chunk c - 1 since
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1, bnxt, xr);   // in flight while this chunk is multiplied
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t * 16 + (lane & 15)][4 * kk + kq], bcur[kk], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int kk = 0; kk < kKc / 4; ++kk) bcur[kk] = bnxt[kk];
    }
    if (!row_ok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 16 * t + kq + 4 * r;
            if (b < nb) {
                const double g = acc[t][r];
                const size_t o = (size_t)b * n + i;
                if (emb) emb[o] = g;
                s[o] = lognormal ? exp(g) : g;
            }
        }
    }
}

constexpr int kGemvUnroll = 16;

template <int NB>
__global__ __launch_bounds__(64 * kWaves) void kl_gemv_kernel(int n, int m, const double* __restrict__ phi,
                                                              const double* __restrict__ xi, int n_xi, double* __restrict__ s,
                                                              double* __restrict__ emb, int lognormal) {
    __shared__ double part[kWaves - 1][NB][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: xi is read with scalar loads
    const int i = blockIdx.x * 64 + lane;
    const int per = (m + kWaves - 1) / kWaves;
    const int k_lo = wave * per, k_hi = min(m, k_lo + per);
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    if (i < n) {
        int k = k_lo;
        for (; k + kGemvUnroll <= k_hi; k += kGemvUnroll) {
            double p[kGemvUnroll];
#pragma unroll
            for (int u = 0; u < kGemvUnroll; ++u) p[u] = phi[(size_t)(k + u) * n + i];
#pragma unroll
            for (int u = 0; u < kGemvUnroll; ++u)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = fma(p[u], xi[(size_t)b * n_xi + k + u], acc[b]);
        }
        for (; k < k_hi; ++k) {
            const double p = phi[(size_t)k * n + i];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = fma(p, xi[(size_t)b * n_xi + k], acc[b]);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) part[wave - 1][b][lane] = acc[b];
    }
    __syncthreads();
    if (wave != 0 || i >= n) return;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double g = acc[b];
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) g += part[w][b][lane];
        const size_t o = (size_t)b * n + i;
        if (emb) emb[o] = g;
        s[o] = lognormal ? exp(g) : g;
    }
}

// phi_c[k nc + c] = sum_p v[p] phi_f[k nf + ci[p]], p in row c of Pi = D^-1 P^T W
__global__ void kl_project_kernel(int nc, int nf, int m, const int* __restrict__ rp, const int* __restrict__ ci,
                                  const double* __restrict__ v, const double* __restrict__ phi_f, double* __restrict__ phi_c) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    for (int k = blockIdx.y; k < m; k += gridDim.y) {
        double acc = 0.0;
        for (int p = rp[c]; p < rp[c + 1]; ++p) acc += v[p] * phi_f[(size_t)k * nf + ci[p]];
        phi_c[(size_t)k * nc + c] = acc;
    }
}

template <int NT>
void launch_mfma(hipStream_t st, int n, int m, int nb, const double* phi, const double* xi, int n_xi, double* s, double* emb,
                 bool lognormal) {
    const dim3 grid((unsigned)((n + 16 * kWaves - 1) / (16 * kWaves)), (unsigned)((nb + 16 * NT - 1) / (16 * NT)));
    kl_mfma_kernel<NT><<<grid, 64 * kWaves, 0, st>>>(n, m, nb, phi, xi, n_xi, s, emb, lognormal ? 1 : 0);
}

template <int NB>
void launch_gemv(hipStream_t st, int n, int m, const double* phi, const double* xi, int n_xi, double* s, double* emb,
                 bool lognormal) {
    kl_gemv_kernel<NB><<<(unsigned)((n + 63) / 64), 64 * kWaves, 0, st>>>(n, m, phi, xi, n_xi, s, emb, lognormal ? 1 : 0);
}

}  // namespace

void kl_eval(hipStream_t st, int n, int m, int nb, const double* phi, const double* xi, int n_xi, double* s, double* emb,
             bool lognormal) {
    switch (nb) {
        case 1: launch_gemv<1>(st, n, m, phi, xi, n_xi, s, emb, lognormal); break;
        case 2: launch_gemv<2>(st, n, m, phi, xi, n_xi, s, emb, lognormal); break;
        case 3: launch_gemv<3>(st, n, m, phi, xi, n_xi, s, emb, lognormal); break;
        case 4: launch_gemv<4>(st, n, m, phi, xi, n_xi, s, emb, lognormal); break;
        default: {
            // realization tiles of 16 per workgroup: the smallest power of two that covers nb, at most 8 (128 realizations;
            // wider launches take several workgroup columns, each reading Phi again: 16 tiles need 135 KB of LDS and 330
            // registers per lane, one workgroup per CU, and ran slower per flop than 8)
            const int tiles = (std::min(nb, 16 * kMaxTiles) + 15) / 16;
            if (tiles <= 1) launch_mfma<1>(st, n, m, nb, phi, xi, n_xi, s, emb, lognormal);
            else if (tiles <= 2) launch_mfma<2>(st, n, m, nb, phi, xi, n_xi, s, emb, lognormal);
            else if (tiles <= 4) launch_mfma<4>(st, n, m, nb, phi, xi, n_xi, s, emb, lognormal);
            else launch_mfma<8>(st, n, m, nb, phi, xi, n_xi, s, emb, lognormal);
        }
    }
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

// ---- handle --------------------------------------------------------------------------------------------------------------
Sampler::Sampler(Ctx& c, int nlevels_, const pmc_kl_level* in, int nmodes, const double* evals, const double* evect0,
                 bool logn)
    : ctx(c), nlevels(nlevels_), n_mc(nlevels_), alpha(0.0), g(0.0), lognormal(logn), kl(true), kl_m(nmodes) {
    PMC_REQUIRE(nlevels >= 1, "KL sampler: need at least one level");
    PMC_REQUIRE(in != nullptr && evals != nullptr && evect0 != nullptr, "KL sampler: levels / evals / evect0 is NULL");
    PMC_REQUIRE(nmodes >= 1, "KL sampler: need at least one mode");
    pmc_solver_opts_default(&opts);
    for (int k = 0; k < nmodes; ++k)
        PMC_REQUIRE(std::isfinite(evals[k]) && evals[k] >= 0.0, "KL sampler: eigenvalue " + std::to_string(k) +
                                                                    " is negative or not finite");
    lv.resize(nlevels);
    for (int l = 0; l < nlevels; ++l) {
        const pmc_kl_level& L = in[l];
        SamplerLevel& d = lv[l];
        PMC_REQUIRE(L.n_s > 0, "KL sampler level: no elements");
        PMC_REQUIRE(L.w_diag != nullptr, "KL sampler level: w_diag is NULL");
        PMC_REQUIRE(nmodes <= L.n_s, "KL sampler: nmodes exceeds n_s of level " + std::to_string(l) +
                                         " (KLSampler::Eval would read past xi)");
        for (int e = 0; e < L.n_s; ++e)
            PMC_REQUIRE(std::isfinite(L.w_diag[e]) && L.w_diag[e] > 0.0, "KL sampler level: w_diag must be positive");
        if (l == 0) w0_host.assign(L.w_diag, L.w_diag + L.n_s);
        d.n_u = 0;
        d.n_s = L.n_s;
        d.out_size = L.n_s;
        d.nnz = 0;   // KLSampler::BuildHierarchy: nnz[i] = 0
    }
    ctx.activate();
    hipStream_t st = ctx.stream;
    kl_phi.resize(nlevels);
    {
        const int n0 = lv[0].n_s;
        std::vector<double> h((size_t)n0 * nmodes);
        for (int k = 0; k < nmodes; ++k) {
            const double sq = std::sqrt(evals[k]);
            const double* src = evect0 + (size_t)k * n0;
            double* dst = h.data() + (size_t)k * n0;
            for (int i = 0; i < n0; ++i) dst[i] = sq * src[i];
        }
        kl_phi[0].upload(h, st);
        PMC_HIP(hipStreamSynchronize(st));
    }
    for (int l = 0; l + 1 < nlevels; ++l) {
        const int nf = lv[l].n_s, nc = lv[l + 1].n_s;
        HostCsr P = csr_from_c(in[l].P, true, "KL sampler P");
        PMC_REQUIRE(P.nrows == nf && P.ncols == nc, "KL sampler P: wrong shape (n_s(level) x n_s(level+1))");
        // D = P^T W P must be diagonal: the nonzero entries of a row of P all lie in one column
        std::vector<double> D((size_t)nc, 0.0);
        for (int r = 0; r < nf; ++r) {
            int col = -1;
            for (int p = P.rowptr[r]; p < P.rowptr[r + 1]; ++p) {
                if (P.vals[p] == 0.0) continue;
                PMC_REQUIRE(col < 0 || col == P.colind[p], "KL sampler: P^T W P is not diagonal (row " + std::to_string(r) +
                                                               " of P has entries in two columns)");
                col = P.colind[p];
            }
            double pr = 0.0;
            for (int p = P.rowptr[r]; p < P.rowptr[r + 1]; ++p) pr += P.vals[p];
            if (col >= 0) D[(size_t)col] += pr * in[l].w_diag[r] * pr;
        }
        for (int j = 0; j < nc; ++j)
            PMC_REQUIRE(D[(size_t)j] > 0.0, "KL sampler: P^T W P has a zero diagonal entry (empty coarse element)");
        // Pi = D^-1 P^T W (nc x nf)
        HostCsr Pi = csr_transpose(P);
        for (int j = 0; j < nc; ++j)
            for (int p = Pi.rowptr[j]; p < Pi.rowptr[j + 1]; ++p) Pi.vals[p] *= in[l].w_diag[Pi.colind[p]] / D[(size_t)j];
        lv[l].P_host = std::move(P);
        DevBuf<int> rp, ci;
        DevBuf<double> v;
        rp.upload(Pi.rowptr, st);
        ci.upload(Pi.colind, st);
        v.upload(Pi.vals, st);
        kl_phi[l + 1].alloc((size_t)nc * nmodes);
        const dim3 grid((unsigned)((nc + 255) / 256), (unsigned)std::min(nmodes, 4096));
        kl_project_kernel<<<grid, 256, 0, st>>>(nc, nf, nmodes, rp.p, ci.p, v.p, kl_phi[l].p, kl_phi[l + 1].p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
        PMC_HIP(hipStreamSynchronize(st));
    }
}

void Sampler::eval_kl(int level, int xi_level, int nbatch, const double* xi, double* s_out, double* emb_out, int memspace,
                      pmc_stats* stats) {
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "Eval: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const int n = lv[level].n_s, n_xi = lv[xi_level].n_s;
    const double* xi_d = xi;
    double* s_d = s_out;
    double* emb_d = emb_out;
    if (memspace == PMC_MEM_HOST) {
        stage_in.ensure((size_t)n_xi * nbatch);
        stage_out.ensure((size_t)n * nbatch);
        if (emb_out) stage_emb.ensure((size_t)n * nbatch);
        PMC_HIP(hipMemcpyAsync(stage_in.p, xi, sizeof(double) * n_xi * nbatch, hipMemcpyHostToDevice, st));
        xi_d = stage_in.p;
        s_d = stage_out.p;
        emb_d = emb_out ? stage_emb.p : nullptr;
    }
    if (stats) {
        ctx.phase_mark(0);
        ctx.phase_mark(1);
    }
    kl_eval(st, n, kl_m, nbatch, kl_phi[level].p, xi_d, n_xi, s_d, emb_d, lognormal && !cond);
    // exp() in the conditioner's store; inside EvalTangent the homogeneous map
    if (cond) cond->apply_device(level, nbatch, s_d, nullptr, s_d, lognormal, cond_tangent_width > 0, cond_tangent_width);
    if (stats) {
        ctx.phase_mark(2);
        ctx.phase_report(stats, nbatch);
        for (int b = 0; b < nbatch; ++b) {
            stats[b].iterations = 0;
            stats[b].converged = 1;
            stats[b].initial_norm = 0.0;
            stats[b].final_norm = 0.0;
        }
    }
    if (memspace == PMC_MEM_HOST) {
        PMC_HIP(hipMemcpyAsync(s_out, s_d, sizeof(double) * n * nbatch, hipMemcpyDeviceToHost, st));
        if (emb_out) PMC_HIP(hipMemcpyAsync(emb_out, emb_d, sizeof(double) * n * nbatch, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

}  // namespace pmc

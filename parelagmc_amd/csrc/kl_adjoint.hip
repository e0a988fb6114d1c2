// Adjoint of the KL sampler's Eval (pmc_sampler_eval_adjoint on a pmc_sampler_create_kl handle):
//     dJ/dxi[:m] = (Phi_level Lambda^1/2)^T (v o f'),   f' = s_out on a lognormal handle, 1 otherwise;   dJ/dxi[m:] = 0.
//
// A launch of nb realizations is one fp64 GEMM  G (nb x m) = V (nb x n) . Phi (n x m), V = v o s_out formed in the load, Phi
// column-major with sqrt(lambda) folded in (Sampler::kl_phi).  The reduction runs over the FIELD: it is cut into chunks of
// adjoint_chunk_rows(n) rows - a function of n alone - each chunk's product written as a partial, and the partials summed
// in ascending chunk order by kl_adjoint_reduce_kernel.  No atomics: column b of the result is the same bits for every
// nb > 4 and every split of a call into pieces wider than 4 (a piece of at most 4 takes the VALU kernel below).
//   nb > 4: kl_adjoint_mfma_kernel, v_mfma_f64_16x16x4f64 (operand maps: the comment at the top of kl.hip).  The first design
//           note of kl_mfma_kernel applies mirrored: neither Phi (stride n between modes) nor V (stride n between
//           realizations) is laid out for the operand maps, so both are staged through LDS - loaded along the field
//           (256-byte runs), read back along modes / realizations.
//   nb <= 4: kl_adjoint_gemv_kernel, pure bandwidth: one mode per wave, the chunk's rows over the lanes.
#include "handles.hpp"
#include "kernels.hpp"

namespace pmc {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;            // waves per workgroup (both kernels)
constexpr int kThreads = 64 * kWaves;
constexpr int kModes = 16 * kWaves;  // modes per MFMA workgroup: 16 per wave
constexpr int kRows = 32;            // field rows per LDS stage
// row stride of the LDS tiles in doubles.  A 32-lane half of a wave reads rows j = 0..15, columns kq and kq + 1: dword
// addresses 2 (kLd j + kq) = 4 j + 2 kq (mod 64) with kLd = 34 - all 64 banks once, no conflict for ds_read_b64.
constexpr int kLd = kRows + 2;
constexpr int kMaxTiles = 8;         // realization tiles of 16 per MFMA workgroup: 128 realizations
constexpr int kMaxLaunch = 256;      // realizations per launch (bounds the partials: chunks x 256 x m doubles)

// rows of one reduction chunk: 1024, and from 32 768 rows on as many as keep the chunks at 32 (a multiple of kRows)
int adjoint_chunk_rows(int n) {
    const int per32 = ((n + 31) / 32 + kRows - 1) / kRows * kRows;
    return std::max(1024, per32);
}

// Here A = V (rows: realizations, reduction: field rows), B = Phi (columns: modes), so lane l, register r holds
// D[realization (l >> 4) + 4 r][mode l & 15] and each store of a register is 16 consecutive modes of one realization.
// Rows past the chunk, modes past m and realizations past nb are staged as zeros: they add +0 products.
template <int NT>
__global__ __launch_bounds__(kThreads) void kl_adjoint_mfma_kernel(int n, int m, int nb, int chunk_rows,
                                                                   const double* __restrict__ phi, const double* __restrict__ v,
                                                                   const double* __restrict__ sv, double* __restrict__ part) {
    constexpr int kP = kModes * kRows / kThreads;     // Phi entries each thread stages per step
    constexpr int kV = 16 * NT * kRows / kThreads;    // V entries
    __shared__ double ps[kModes][kLd];
    __shared__ double vs[16 * NT][kLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kq = lane >> 4;
    const int k0 = blockIdx.x * kModes;
    const int chunk = blockIdx.y;
    const int b0 = blockIdx.z * 16 * NT;
    const int r0 = chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double pr[kP], vr[kV];
    // entry e = threadIdx.x + j kThreads of a [modes | realizations][kRows] tile: consecutive threads read consecutive rows
    auto load_tile = [&](int i0) {
        const int i = i0 + (threadIdx.x & (kRows - 1));
        const bool row_ok = i < r1;
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int k = k0 + (threadIdx.x + j * kThreads) / kRows;
            pr[j] = (row_ok && k < m) ? phi[(size_t)k * n + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kV; ++j) {
            const int b = b0 + (threadIdx.x + j * kThreads) / kRows;
            double x = 0.0;
            if (row_ok && b < nb) {
                const size_t o = (size_t)b * n + i;
                x = sv ? v[o] * sv[o] : v[o];
            }
            vr[j] = x;
        }
    };
    load_tile(r0);
    for (int i0 = r0; i0 < r1; i0 += kRows) {
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int e = threadIdx.x + j * kThreads;
            ps[e / kRows][e % kRows] = pr[j];
        }
#pragma unroll
        for (int j = 0; j < kV; ++j) {
            const int e = threadIdx.x + j * kThreads;
            vs[e / kRows][e % kRows] = vr[j];
        }
        __syncthreads();
        if (i0 + kRows < r1) load_tile(i0 + kRows);   // in flight while this stage is multiplied
#pragma unroll
        for (int kk = 0; kk < kRows / 4; ++kk) {
            const double b = ps[wave * 16 + (lane & 15)][4 * kk + kq];
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[t * 16 + (lane & 15)][4 * kk + kq], b, acc[t], 0, 0, 0);
        }
        __syncthreads();   // every wave has read the tiles before the next stage overwrites them
    }
    const int k = k0 + wave * 16 + (lane & 15);
    if (k >= m) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 16 * t + kq + 4 * r;
            if (b < nb) part[((size_t)chunk * nb + b) * m + k] = acc[t][r];
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kThreads) void kl_adjoint_gemv_kernel(int n, int m, int chunk_rows, const double* __restrict__ phi,
                                                                   const double* __restrict__ v, const double* __restrict__ sv,
                                                                   double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= m) return;   // whole waves; the kernel has no barrier
    const int chunk = blockIdx.y;
    const int r0 = chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);
    const double* __restrict__ col = phi + (size_t)k * n;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
#pragma unroll 4
    for (int i = r0 + lane; i < r1; i += 64) {
        const double p = col[i];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const size_t o = (size_t)b * n + i;
            acc[b] = fma(p, sv ? v[o] * sv[o] : v[o], acc[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double a = acc[b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);   // a fixed butterfly
        if (lane == 0) part[((size_t)chunk * NB + b) * m + k] = a;
    }
}

// grad[b n_xi + k] = sum over the chunks, ascending, of part[chunk][b][k] for k < m; 0 for m <= k < n_xi
__global__ __launch_bounds__(kThreads) void kl_adjoint_reduce_kernel(int m, int n_xi, int nb, int nchunks,
                                                                     const double* __restrict__ part, double* __restrict__ grad) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= n_xi) return;
    double g = 0.0;
    if (k < m) {
        g = part[(size_t)b * m + k];
        for (int c = 1; c < nchunks; ++c) g += part[((size_t)c * nb + b) * m + k];
    }
    grad[(size_t)b * n_xi + k] = g;
}

template <int NT>
void launch_mfma(hipStream_t st, int n, int m, int nb, int chunk_rows, int nchunks, const double* phi, const double* v,
                 const double* sv, double* part) {
    const dim3 grid((unsigned)((m + kModes - 1) / kModes), (unsigned)nchunks, (unsigned)((nb + 16 * NT - 1) / (16 * NT)));
    kl_adjoint_mfma_kernel<NT><<<grid, kThreads, 0, st>>>(n, m, nb, chunk_rows, phi, v, sv, part);
}

template <int NB>
void launch_gemv(hipStream_t st, int n, int m, int chunk_rows, int nchunks, const double* phi, const double* v,
                 const double* sv, double* part) {
    const dim3 grid((unsigned)((m + kWaves - 1) / kWaves), (unsigned)nchunks);
    kl_adjoint_gemv_kernel<NB><<<grid, kThreads, 0, st>>>(n, m, chunk_rows, phi, v, sv, part);
}

}  // namespace

int kl_adjoint_chunk_rows(int n) { return adjoint_chunk_rows(n); }

size_t kl_adjoint_partials(int n, int m, int nb) {
    const int cr = adjoint_chunk_rows(n);
    return (size_t)((n + cr - 1) / cr) * (size_t)std::min(nb, kMaxLaunch) * (size_t)m;
}

void kl_eval_adjoint(hipStream_t st, int n, int m, int nb, const double* phi, const double* v, const double* sv, int n_xi,
                     double* grad, double* part) {
    const int cr = adjoint_chunk_rows(n);
    const int nchunks = (n + cr - 1) / cr;
    const bool mfma = nb > 4;   // decided by the CALL: the pieces of a wide call all take the MFMA kernel
    for (int done = 0; done < nb; done += kMaxLaunch) {
        const int w = std::min(kMaxLaunch, nb - done);
        const double* vp = v + (size_t)done * n;
        const double* sp = sv ? sv + (size_t)done * n : nullptr;
        if (!mfma) {
            switch (w) {
                case 1: launch_gemv<1>(st, n, m, cr, nchunks, phi, vp, sp, part); break;
                case 2: launch_gemv<2>(st, n, m, cr, nchunks, phi, vp, sp, part); break;
                case 3: launch_gemv<3>(st, n, m, cr, nchunks, phi, vp, sp, part); break;
                default: launch_gemv<4>(st, n, m, cr, nchunks, phi, vp, sp, part); break;
            }
        } else {
            const int tiles = (std::min(w, 16 * kMaxTiles) + 15) / 16;
            if (tiles <= 1) launch_mfma<1>(st, n, m, w, cr, nchunks, phi, vp, sp, part);
            else if (tiles <= 2) launch_mfma<2>(st, n, m, w, cr, nchunks, phi, vp, sp, part);
            else if (tiles <= 4) launch_mfma<4>(st, n, m, w, cr, nchunks, phi, vp, sp, part);
            else launch_mfma<8>(st, n, m, w, cr, nchunks, phi, vp, sp, part);
        }
        PMC_HIP(hipGetLastError());
        const dim3 rgrid((unsigned)((n_xi + kThreads - 1) / kThreads), (unsigned)w);
        kl_adjoint_reduce_kernel<<<rgrid, kThreads, 0, st>>>(m, n_xi, w, nchunks, part, grad + (size_t)done * n_xi);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(2);
    }
}

void Sampler::eval_adjoint_kl(int level, int xi_level, int nbatch, const double* v, const double* s_out, double* grad_xi,
                              int memspace, pmc_stats* stats) {
    ctx.activate();
    hipStream_t st = ctx.stream;
    const int n = lv[level].n_s, n_xi = lv[xi_level].n_s;
    const double* v_d = v;
    const double* s_d = s_out;
    double* g_d = grad_xi;
    if (memspace == PMC_MEM_HOST) {
        stage_in.ensure((size_t)n * nbatch);
        stage_out.ensure((size_t)n_xi * nbatch);
        PMC_HIP(hipMemcpyAsync(stage_in.p, v, sizeof(double) * n * nbatch, hipMemcpyHostToDevice, st));
        v_d = stage_in.p;
        if (s_out) {
            stage_emb.ensure((size_t)n * nbatch);
            PMC_HIP(hipMemcpyAsync(stage_emb.p, s_out, sizeof(double) * n * nbatch, hipMemcpyHostToDevice, st));
            s_d = stage_emb.p;
        }
        g_d = stage_out.p;
    }
    adj_part.ensure(kl_adjoint_partials(n, kl_m, nbatch));
    if (cond) {   // w = Gamma^T (v o f') of the whole call, then the unconditioned product with v := w, s_out := NULL
        cond->hook_w.ensure((size_t)n * nbatch);
        cond->apply_adjoint_device(level, nbatch, v_d, s_d, cond->hook_w.p);
        v_d = cond->hook_w.p;
        s_d = nullptr;
    }
    if (stats) {
        ctx.phase_mark(0);
        ctx.phase_mark(1);
    }
    kl_eval_adjoint(st, n, kl_m, nbatch, kl_phi[level].p, v_d, s_d, n_xi, g_d, adj_part.p);
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
        PMC_HIP(hipMemcpyAsync(grad_xi, g_d, sizeof(double) * n_xi * nbatch, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

}  // namespace pmc

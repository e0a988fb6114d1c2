// Adjoint gradients of the Darcy quantity of interest and of the Gaussian log-likelihood with respect to the permeability
// field (numpy twin: parelagmc_amd/fe/darcy_adjoint.py).  The reference has no gradients: this is an
// extension.  The mixed system is symmetric, so one adjoint solve with the operator and the per-realization preconditioner
// of the forward solve gives the whole gradient:
//     A(k) x = rhs_bc,   A(k) lam = dJ/dx (essential rows zero),   dJ/dk_e = -c'(k_e) lam_u^T M_e x_u.
// x_u carries the essential values and lam_u vanishes on the essential rows, so the derivative of the eliminated right-hand
// side needs no term of its own.
#include <algorithm>
#include <cmath>

#include "handles.hpp"
#include "kdev.hpp"

namespace pmc {

namespace {

// One wavefront per slice of 64 elements, swept in T steps of G elements: lane (g, t) takes element rs G + g and the 16 B
// column pair t of its NB realizations.  The 2 n_fe gathered rows of x_u / lam_u (NB x 8 contiguous bytes each) are requested
// back to back, then a fixed double loop forms s_a = sum_a' M_e[a][a'] x[a'] and acc += lam[a] s_a with explicit FMAs (the
// same rounding sequence per column whatever NB).  Face indices and M_e entries of a step are G consecutive words of the
// slice's columns; no LDS.  NFE == 0: any number of faces per element - the rows are gathered again per (a, a') instead of
// being held in registers (same order, same bits).
template <int NB, int NFE>
__global__ __launch_bounds__(kBlock) void mass_sensitivity_kernel(int n_elem, int nslices, int nfe_rt,
                                                                  const int* __restrict__ faces,
                                                                  const double* __restrict__ me,
                                                                  const double* __restrict__ kfield,
                                                                  const double* __restrict__ x,
                                                                  const double* __restrict__ lam, int k_divides, int wrt_log,
                                                                  double* __restrict__ out, int ld) {
    constexpr int C = Lay<NB>::C, T = Lay<NB>::T, G = Lay<NB>::G;
    const int LD = row_ld<NB>(ld);
    {
        const int c0 = col0<NB>();
        x += c0;
        lam += c0;
        kfield += (size_t)c0 * n_elem;      // sample-major: column b starts at b n_elem
        out += (size_t)c0 * n_elem;
    }
    const int nfe = NFE > 0 ? NFE : nfe_rt;
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / T, t = lane % T;
    const SliceWalk sw = slice_walk(nslices);
    for (int slice = sw.begin; slice < sw.end; slice += sw.stride) {
        const int* __restrict__ fs = faces + (size_t)slice * nfe * kWave;
        const double* __restrict__ ms = me + (size_t)slice * nfe * nfe * kWave;
#pragma unroll 1
        for (int rs = 0; rs < T; ++rs) {
            const int le = rs * G + g;
            const int e = slice * kWave + le;
            if (e >= n_elem) continue;          // elements past the end of the last slice write nothing
            double acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.0;
            if constexpr (NFE > 0) {
                size_t at[NFE];
#pragma unroll
                for (int a = 0; a < NFE; ++a) at[a] = (size_t)fs[a * kWave + le] * LD + t * C;
                double xv[NFE][C], lv[NFE][C];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < NFE; ++a) {
                    load_c<C>(x + at[a], xv[a]);
                    load_c<C>(lam + at[a], lv[a]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < NFE; ++a) {
                    double s[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) s[c] = 0.0;
#pragma unroll
                    for (int a2 = 0; a2 < NFE; ++a2) {
                        const double m = ms[(a * NFE + a2) * kWave + le];
#pragma unroll
                        for (int c = 0; c < C; ++c) s[c] = fma(m, xv[a2][c], s[c]);
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = fma(lv[a][c], s[c], acc[c]);
                }
            } else {
                for (int a = 0; a < nfe; ++a) {
                    double s[C], lv[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) s[c] = 0.0;
                    load_c<C>(lam + (size_t)fs[a * kWave + le] * LD + t * C, lv);
                    for (int a2 = 0; a2 < nfe; ++a2) {
                        const double m = ms[(a * nfe + a2) * kWave + le];
                        double xv[C];
                        load_c<C>(x + (size_t)fs[a2 * kWave + le] * LD + t * C, xv);
#pragma unroll
                        for (int c = 0; c < C; ++c) s[c] = fma(m, xv[c], s[c]);
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = fma(lv[c], s[c], acc[c]);
                }
            }
            // -c'(k) and the sample-major store: per column the G elements of a step are consecutive
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const size_t o = (size_t)(t * C + c) * n_elem + e;
                const double kv = kfield[o];
                double f;
                if (k_divides) f = wrt_log ? 1.0 / kv : 1.0 / (kv * kv);
                else f = wrt_log ? -kv : -1.0;
                out[o] = f * acc[c];
            }
        }
    }
}

// v[i nb + b] = 0 on the essential rows i < n_u of an interleaved vector
__global__ void zero_ess_rows_kernel(size_t total, int nb, const unsigned char* __restrict__ ess, double* __restrict__ v) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    if (ess[t / nb]) v[t] = 0.0;
}

// y[j nb + b] = x[rows[j] nb + b]
__global__ void gather_rows_kernel(size_t total, int nb, const int* __restrict__ rows, const double* __restrict__ x,
                                   double* __restrict__ y) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t j = t / nb;
    y[t] = x[(size_t)rows[j] * nb + (t - j * nb)];
}

// p-rows of the adjoint right-hand side of the log-likelihood: rhs[e][b] = -(1 / noise) sum_i (G_ib - data_i) g_i[e] / sum(g_i)
// with G_ib = norm_i gsum[i][b] (the value pmc_darcy_compute_G reports); gt_*: CSR over the elements of diag(norm) Gobs
// transposed, entries of a row in ascending observation index (fixed summation order)
__global__ void loglik_rhs_kernel(size_t total, int nb, const int* __restrict__ gt_ptr, const int* __restrict__ gt_obs,
                                  const double* __restrict__ gt_val, const double* __restrict__ gsum,
                                  const double* __restrict__ norm, const double* __restrict__ data, double neg_inv_noise,
                                  double* __restrict__ rhs_p) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t e = t / nb;
    const int b = (int)(t - e * nb);
    double s = 0.0;
    for (int p = gt_ptr[e]; p < gt_ptr[e + 1]; ++p) {
        const int i = gt_obs[p];
        s = fma(norm[i] * gsum[(size_t)i * nb + b] - data[i], gt_val[p], s);
    }
    rhs_p[t] = neg_inv_noise * s;
}

inline unsigned flat_blocks(size_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

namespace k {

void darcy_mass_sensitivity(hipStream_t st, int nb, const ElemMassView& E, const double* kfield, const double* x,
                            const double* lam, bool k_divides, bool wrt_log, double* out) {
    if (E.n_elem <= 0) return;
    const dim3 grid((unsigned)((E.nslices + kBlock / kWave - 1) / (kBlock / kWave)), nb > kGroup ? (unsigned)(nb / kGroup) : 1u);
    const int kd = k_divides ? 1 : 0, wl = wrt_log ? 1 : 0;
#define PMC_MS_LAUNCH(NFE)                                                                                              \
    PMC_DISPATCH_NB(nb, {                                                                                               \
        mass_sensitivity_kernel<NB, NFE><<<grid, kBlock, 0, st>>>(E.n_elem, E.nslices, E.nfe, E.faces, E.me, kfield, x, \
                                                                   lam, kd, wl, out, nb);                                \
    })
    switch (E.nfe) {      // faces of a triangle, a quadrilateral / tetrahedron, a hexahedron; anything else: the general form
        case 3: PMC_MS_LAUNCH(3); break;
        case 4: PMC_MS_LAUNCH(4); break;
        case 6: PMC_MS_LAUNCH(6); break;
        default: PMC_MS_LAUNCH(0); break;
    }
#undef PMC_MS_LAUNCH
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

}  // namespace k

// Faces and dense unit-coefficient matrix of every element from the contribution lists the handle already holds on the device
// (pattern of M in SELL order, c_ptr / c_elem / c_val): the faces of element e are the rows whose DIAGONAL entry e contributes
// to - the columns of row e of the uneliminated B - in ascending order.  Built once per level, at its first gradient call.
// tangent: also the face-major copy of the same data the tangent right-hand side reads (darcy_hessian.hip), at the level's
// first tangent / Hessian call; a handle that never asks for one allocates nothing for it.
void Darcy::ensure_gradient(int level, bool tangent) {
    DarcyLevel& d = lv[level];
    if (d.has_grad && (!tangent || d.has_tan)) return;
    hipStream_t st = ctx.stream;
    const Sell& M = d.M;
    const size_t nslots = (size_t)M.nslots;
    std::vector<int> soff((size_t)M.nslices + 1), cols(nslots), src(nslots), c_ptr(d.c_ptr.n), c_elem(d.c_elem.n);
    std::vector<double> c_val(d.c_val.n);
    auto fetch = [&](void* dst, const void* from, size_t bytes) {
        if (bytes) PMC_HIP(hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToHost, st));
    };
    fetch(soff.data(), M.slice_off.p, sizeof(int) * soff.size());
    fetch(cols.data(), M.cols.p, sizeof(int) * nslots);
    fetch(src.data(), d.slot_src.p, sizeof(int) * nslots);
    fetch(c_ptr.data(), d.c_ptr.p, sizeof(int) * c_ptr.size());
    fetch(c_elem.data(), d.c_elem.p, sizeof(int) * c_elem.size());
    fetch(c_val.data(), d.c_val.p, sizeof(double) * c_val.size());
    PMC_HIP(hipStreamSynchronize(st));
    const int n_u = d.n_u, n_p = d.n_p;
    // walk the stored entries (row, col, nnz index) of M in SELL order
    auto for_entries = [&](auto&& fn) {
        for (int sl = 0; sl < M.nslices; ++sl) {
            const int off = soff[sl], width = (soff[sl + 1] - off) / kWave;
            for (int j = 0; j < width; ++j)
                for (int lane = 0; lane < kWave; ++lane) {
                    const size_t s = (size_t)off + (size_t)j * kWave + lane;
                    const int row = sl * kWave + lane;
                    if (row < n_u && src[s] >= 0) fn(row, cols[s], src[s]);
                }
        }
    };
    std::vector<std::vector<int>> ef(n_p);
    for_entries([&](int row, int col, int p) {
        if (row != col) return;
        for (int t = c_ptr[p]; t < c_ptr[p + 1]; ++t) ef[c_elem[t]].push_back(row);
    });
    int nfe = 0;
    for (int e = 0; e < n_p; ++e) {
        std::sort(ef[e].begin(), ef[e].end());
        ef[e].erase(std::unique(ef[e].begin(), ef[e].end()), ef[e].end());
        PMC_REQUIRE(!ef[e].empty(), "darcy gradient: an element contributes to no diagonal entry of M");
        nfe = std::max(nfe, (int)ef[e].size());
    }
    PMC_REQUIRE(nfe <= 64, "darcy gradient: more than 64 faces per element");
    const int nslices = (n_p + kWave - 1) / kWave;
    std::vector<int> faces((size_t)nslices * nfe * kWave, 0);
    std::vector<double> me((size_t)nslices * nfe * nfe * kWave, 0.0);
    for (int e = 0; e < n_p; ++e) {
        const size_t sl = (size_t)e / kWave, le = (size_t)e % kWave;
        for (int a = 0; a < nfe; ++a)      // padding: the element's first face, weight zero
            faces[(sl * nfe + a) * kWave + le] = ef[e][a < (int)ef[e].size() ? a : 0];
    }
    auto local = [&](int e, int f) {
        const auto it = std::lower_bound(ef[e].begin(), ef[e].end(), f);
        PMC_REQUIRE(it != ef[e].end() && *it == f, "darcy gradient: an element matrix entry outside the element's faces");
        return (int)(it - ef[e].begin());
    };
    for_entries([&](int row, int col, int p) {
        for (int t = c_ptr[p]; t < c_ptr[p + 1]; ++t) {
            const int e = c_elem[t];
            const size_t sl = (size_t)e / kWave, le = (size_t)e % kWave;
            me[(sl * nfe * nfe + (size_t)local(e, row) * nfe + local(e, col)) * kWave + le] += c_val[t];
        }
    });
    if (!d.has_grad) {
        d.grad_faces.upload(faces, st);
        d.grad_me.upload(me, st);
        PMC_HIP(hipStreamSynchronize(st));
        d.grad_nfe = nfe;
        d.grad_nslices = nslices;
        d.has_grad = true;
    }
    if (!tangent || d.has_tan) return;
    // face-major: the sides of face f are the elements that have f among their faces, in ascending element id (the loop
    // below visits them in that order); side s of f holds the element's faces and row a(f) of its M_e
    std::vector<int> cnt((size_t)n_u, 0);
    for (int e = 0; e < n_p; ++e)
        for (int f : ef[e]) cnt[f]++;
    int nside = 1;
    for (int f = 0; f < n_u; ++f) nside = std::max(nside, cnt[f]);
    const int fslices = (n_u + kWave - 1) / kWave;
    std::vector<int> selem((size_t)fslices * nside * kWave, -1), scols((size_t)fslices * nside * nfe * kWave, 0);
    std::vector<double> sw((size_t)fslices * nside * nfe * kWave, 0.0);
    // padding (a missing side, a slot past the last face): the face itself or the slice's first face, with weight zero
    for (size_t sl = 0; sl < (size_t)fslices; ++sl)
        for (size_t j = 0; j < (size_t)nside * nfe; ++j)
            for (size_t lf = 0; lf < (size_t)kWave; ++lf) {
                const size_t f = sl * kWave + lf;
                scols[(sl * nside * nfe + j) * kWave + lf] = (int)(f < (size_t)n_u ? f : sl * kWave);
            }
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int e = 0; e < n_p; ++e) {
        const size_t esl = (size_t)e / kWave, ele = (size_t)e % kWave;
        for (int a = 0; a < (int)ef[e].size(); ++a) {
            const int f = ef[e][a], s = cnt[f]++;
            const size_t sl = (size_t)f / kWave, lf = (size_t)f % kWave;
            selem[(sl * nside + s) * kWave + lf] = e;
            for (int a2 = 0; a2 < nfe; ++a2) {
                const size_t at = ((sl * nside + s) * nfe + a2) * kWave + lf;
                scols[at] = faces[(esl * nfe + a2) * kWave + ele];
                sw[at] = me[(esl * nfe * nfe + (size_t)a * nfe + a2) * kWave + ele];
            }
        }
    }
    d.tan_elem.upload(selem, st);
    d.tan_cols.upload(scols, st);
    d.tan_w.upload(sw, st);
    PMC_HIP(hipStreamSynchronize(st));
    d.tan_nside = nside;
    d.tan_nslices = fslices;
    d.has_tan = true;
}

double Darcy::mass_sensitivity_bytes(int level, int nb) {
    // ALGORITHMIC bytes of one launch: per element n_fe face indices (4 B) and n_fe^2 matrix entries (8 B), its k read and its
    // gradient written per realization; every row of x_u and lam_u once
    ctx.activate();
    ensure_gradient(level);
    const DarcyLevel& d = lv[level];
    const double V = 8.0 * nb, nfe = d.grad_nfe;
    return (double)d.n_p * (4.0 * nfe + 8.0 * nfe * nfe + 2.0 * V) + 2.0 * V * d.n_u;
}

void Darcy::ensure_loglik(int level) {
    DarcyLevel& d = lv[level];
    if (d.has_gt) return;
    hipStream_t st = ctx.stream;
    const HostCsr& G = d.Gobs_host;
    std::vector<int> ptr((size_t)d.n_p + 1, 0), obs(G.colind.size());
    std::vector<double> val(G.colind.size());
    for (int c : G.colind) ptr[(size_t)c + 1]++;
    for (int e = 0; e < d.n_p; ++e) ptr[e + 1] += ptr[e];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int i = 0; i < G.nrows; ++i) {
        double s = 0.0;
        for (int p = G.rowptr[i]; p < G.rowptr[i + 1]; ++p) s += G.vals[p];
        for (int p = G.rowptr[i]; p < G.rowptr[i + 1]; ++p) {
            const int at = fill[G.colind[p]]++;
            obs[at] = i;
            val[at] = G.vals[p] * (1.0 / s);      // 1 / s: the g_norm of set_observations
        }
    }
    d.gt_ptr.upload(ptr, st);
    d.gt_obs.upload(obs, st);
    d.gt_val.upload(val, st);
    PMC_HIP(hipStreamSynchronize(st));
    d.has_gt = true;
}

// ---- the adjoint right-hand sides: each forms adj_rhs (interleaved, essential rows zero) from the launch's solution sol ------
// what the arms that write only the u rows end with: zero p rows (zero_p), zero essential rows
void Darcy::rhs_finish(hipStream_t st, int nb, int level, bool zero_p) {
    const DarcyLevel& d = lv[level];
    if (zero_p) k::fill(st, (size_t)d.n_p * nb, adj_rhs.p + (size_t)d.n_u * nb, 0.0);
    const size_t tu = (size_t)d.n_u * nb;
    zero_ess_rows_kernel<<<flat_blocks(tu), 256, 0, st>>>(tu, nb, d.ess.p, adj_rhs.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

// the caller's dJ/dx (rhs_d: device, sample-major), or the level's obs broadcast (NULL): J = Q
void Darcy::rhs_seed(hipStream_t st, int nb, int level, const double* rhs_d) {
    const DarcyLevel& d = lv[level];
    if (rhs_d) k::interleave(st, nb, d.n_u + d.n_p, rhs_d, nullptr, 1.0, adj_rhs.p);
    else k::broadcast(st, nb, d.n_u + d.n_p, d.obs.p, adj_rhs.p);
    rhs_finish(st, nb, level, false);
}

// the Gaussian log-likelihood of the observation functionals; data: host, n_gobs.  G_host (nb x n_gobs) has arrived once
// the stream is synchronised.
void Darcy::rhs_loglik(hipStream_t st, int nb, int level, const double* data, double noise, double* G_host) {
    DarcyLevel& d = lv[level];
    const int n_u = d.n_u, n_p = d.n_p;
    ensure_loglik(level);
    gtmp.ensure((size_t)d.n_gobs * nb);
    gout.ensure((size_t)d.n_gobs * nb);
    sol_compact.ensure((size_t)std::max(d.n_grows, 1) * nb);
    obs_data.upload(data, (size_t)d.n_gobs, st);
    // G_i = <g_i, p> / sum(g_i) on the rows compute_G maintains
    const size_t tg = (size_t)d.n_grows * nb;
    gather_rows_kernel<<<flat_blocks(tg), 256, 0, st>>>(tg, nb, d.g_rows.p, sol.p, sol_compact.p);
    PMC_HIP(hipGetLastError());
    k::spmm(st, nb, view(d.Gobs), sol_compact.p, gtmp.p, false, nullptr, nullptr);
    k::deinterleave(st, nb, d.n_gobs, gtmp.p, nullptr, d.g_norm.p, false, gout.p);
    PMC_HIP(hipMemcpyAsync(G_host, gout.p, sizeof(double) * d.n_gobs * nb, hipMemcpyDeviceToHost, st));
    k::fill(st, (size_t)n_u * nb, adj_rhs.p, 0.0);
    const size_t tp = (size_t)n_p * nb;
    loglik_rhs_kernel<<<flat_blocks(tp), 256, 0, st>>>(tp, nb, d.gt_ptr.p, d.gt_obs.p, d.gt_val.p, gtmp.p, d.g_norm.p,
                                                       obs_data.p, -1.0 / noise, adj_rhs.p + (size_t)n_u * nb);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(2);
}

// J of the breakthrough data: the transport and its adjoint on the interleaved solution (minres_solve has synchronised the
// stream, as Transport::qoi_interleaved requires), u_bar straight into the u rows.  Seeds curve_bar_d / stored_bar_d (device,
// sample-major; NULL: zero), or with tdata_d (device, nreport) curve_bar = -(curve - data) / noise.  curve_d / stored_d: the
// forward outputs of the launch (device, nb x nreport and nb); status_h: host, nb.
void Darcy::rhs_transport(hipStream_t st, int nb, int level, Transport& T, const double* curve_bar_d, const double* stored_bar_d,
                          const double* tdata_d, double noise, double* curve_d, double* stored_d, int32_t* status_h) {
    T.adjoint_forward(st, nb, sol.p, nb, 1, curve_d, stored_d);
    for (int kcol = 0; kcol < nb; ++kcol) status_h[kcol] = T.h_status[kcol];
    const double* cb_d = tdata_d ? T.loglik_seed(st, nb, curve_d, tdata_d, noise) : curve_bar_d;
    T.adjoint_backward(st, nb, sol.p, nb, 1, cb_d, tdata_d ? nullptr : stored_bar_d, nullptr, adj_rhs.p, nb, 1, nullptr);
    rhs_finish(st, nb, level, true);
}

// J of the travel times: the walk and its adjoint on the interleaved solution, u_bar straight into the
// u rows.  Seed tbar_d (device, nb x nparticles), or with trdata_d (device, nparticles) T_bar = -(T - data) / noise.
// T_d / status_d: the forward outputs of the launch (device, nb x nparticles).
void Darcy::rhs_tracer(hipStream_t st, int nb, int level, Tracer& T, const double* tbar_d, const double* trdata_d, double noise,
                       double* T_d, int32_t* status_d) {
    const size_t cnt = (size_t)nb * T.npart;
    trc_i.ensure(2 * cnt);
    T.adjoint_launch(st, nb, true, sol.p, nb, 1, tbar_d, nullptr, adj_rhs.p, nb, 1, nullptr, T_d, trc_i.p, status_d, trc_i.p + cnt,
                     trdata_d, noise);
    rhs_finish(st, nb, level, true);
}

// One launch: forward solve (all rows), adjoint right-hand side (form_rhs, one of the four above bound to the entry's
// operands), adjoint solve on the same operator and preconditioner, gradient kernel.  grad_d / sol_d / adj_d: device,
// sample-major.
void Darcy::gradient_chunk(int level, int nb, const double* k_d, const AdjointRhs& form_rhs, bool wrt_log, double* Q_host,
                           double* grad_d, double* sol_d, double* adj_d, pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const int n_p = d.n_p, n = d.n_u + n_p;
    ensure_gradient(level);
    adj_rhs.ensure((size_t)n * nb);
    adj_sol.ensure((size_t)n * nb);
    // forward solve on all rows: the configuration (and the captured graph) of solve_fwd with a solution requested
    const SaddleLaunch L = saddle_launch(level, nb, k_d, kSolveFull, stats_fwd != nullptr, true);
    solve_done(minres_solve(ctx, nb, L.A, L.prec, d.rhs_bc.p, sol.p, true, opts, work, 0, n, nullptr, L.hint), nb, stats_fwd);
    // Q = <obs, sol> over all rows, as solve_fwd forms it when the solution is requested - also on a level with a tracer
    // attached (pmc_darcy_set_tracer): the gradient is that of <obs, x>, so its Q stays <obs, x>
    const int qblocks = k::wdot(st, nb, n, d.obs.p, sol.p, qpartial.p);
    k::reduce_final(st, nb, qblocks, qpartial.p, qout.p);
    PMC_HIP(hipMemcpyAsync(ctx.h_scal, qout.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    if (sol_d) k::deinterleave(st, nb, n, sol.p, nullptr, nullptr, false, sol_d);
    if (stats_adj) ctx.phase_mark(0);
    form_rhs(st, nb, level);
    PMC_HIP(hipStreamSynchronize(st));           // Q (and G) have arrived; the data of the right-hand side was read
    for (int kcol = 0; kcol < nb; ++kcol) Q_host[kcol] = ctx.h_scal[kcol];
    if (stats_adj) ctx.phase_mark(1);
    // adjoint solve: same A, prec and options, zero guess, a configuration (graph key) of its own
    solve_done(minres_solve(ctx, nb, L.A, L.prec, adj_rhs.p, adj_sol.p, true, opts, work, 0, n, nullptr,
                            L.follow_up(kSolveAdjoint, adj_rhs.p, adj_sol.p)),
               nb, stats_adj);
    const k::ElemMassView E{n_p, d.grad_nslices, d.grad_nfe, d.grad_faces.p, d.grad_me.p};
    if (grad_timer.on) grad_timer.begin(st);
    k::darcy_mass_sensitivity(st, nb, E, k_d, sol.p, adj_sol.p, k_divides, wrt_log, grad_d);
    if (grad_timer.on) grad_timer.end(st);
    if (adj_d) k::deinterleave(st, nb, n, adj_sol.p, nullptr, nullptr, false, adj_d);
    PMC_HIP(hipStreamSynchronize(st));
    if (grad_timer.on) grad_timer.harvest();
}

namespace {
// Gaussian log-likelihood of nb columns of len values against data (len): loglik_out[b] = -(1 / (2 noise)) sum_i (v_bi - data_i)^2,
// the log of BayesianInverseProblem::ComputeLikelihood; values_out: the values themselves.  Either output may be NULL.
void gauss_loglik(int nb, size_t len, const double* values, const double* data, double noise, double* loglik_out,
                  double* values_out) {
    for (int b = 0; b < nb; ++b) {
        double s = 0.0;
        for (size_t i = 0; i < len; ++i) {
            const double dd = values[(size_t)b * len + i] - data[i];
            s += dd * dd;
            if (values_out) values_out[(size_t)b * len + i] = values[(size_t)b * len + i];
        }
        if (loglik_out) loglik_out[b] = (-1. / (noise * 2)) * s;
    }
}
}  // namespace

// ---- the batched entries: argument checks, the operands of for_chunks (chunks.hpp), one launch as the body -------------------
void Darcy::mass_sensitivity(int level, int nbatch, const double* kf, const double* x, const double* lam, bool wrt_log,
                             double* grad, int memspace) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "mass_sensitivity: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && x != nullptr && lam != nullptr && grad != nullptr,
                "mass_sensitivity: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p;
    ensure_gradient(level);
    const k::ElemMassView E{d.n_p, d.grad_nslices, d.grad_nfe, d.grad_faces.p, d.grad_me.p};
    enum { K, X, LAM, GRAD };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::in(x, n, stage_sol), ChunkArg::in(lam, n, stage_adj),
                ChunkArg::out(grad, np, stage_grad)},
               [&](const Chunk& c) {
                   sol.ensure(n * c.nb);
                   adj_sol.ensure(n * c.nb);
                   k::interleave(st, c.nb, (int)n, c.at<double>(X), nullptr, 1.0, sol.p);
                   k::interleave(st, c.nb, (int)n, c.at<double>(LAM), nullptr, 1.0, adj_sol.p);
                   if (grad_timer.on) grad_timer.begin(st);
                   k::darcy_mass_sensitivity(st, c.nb, E, c.at<double>(K), sol.p, adj_sol.p, k_divides, wrt_log, c.at<double>(GRAD));
                   if (grad_timer.on) grad_timer.end(st);
               });
    if (grad_timer.on) grad_timer.harvest();      // every launch's bracket: the stream is synchronised
}

void Darcy::solve_gradient(int level, int nbatch, const double* kf, const double* adj_rhs_in, bool wrt_log, double* Q,
                           double* C, double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                           pmc_stats* stats_adj) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "solve_gradient: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr, "solve_gradient: bad arguments");
    ctx.activate();
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p;
    std::vector<double> q(kMaxBatch);
    enum { K, RHS, GRAD, SOL, ADJ, SF, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::in(adj_rhs_in, n, stage_adj), ChunkArg::out(grad, np, stage_grad),
                ChunkArg::out(sol_out, n, stage_sol), ChunkArg::out(adj_out, n, stage_out), ChunkArg::stats(stats_fwd),
                ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) { rhs_seed(st, nb, lvl, c.at<double>(RHS)); }, wrt_log,
                                  q.data(), c.at<double>(GRAD), c.at<double>(SOL), c.at<double>(ADJ), c.at<pmc_stats>(SF),
                                  c.at<pmc_stats>(SA));
                   for (int b = 0; b < c.nb; ++b) {
                       if (Q) Q[c.done + b] = q[b];
                       if (C) C[c.done + b] = (double)n;
                   }
               });
}

void Darcy::loglik_gradient(int level, int nbatch, const double* kf, const double* data, double noise, bool wrt_log,
                            double* loglik, double* G, double* grad, int memspace, pmc_stats* stats_adj) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "loglik_gradient: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr, "loglik_gradient: bad arguments");
    PMC_REQUIRE(noise > 0.0, "loglik_gradient: the noise variance must be positive");
    DarcyLevel& d = lv[level];
    PMC_REQUIRE(d.n_gobs > 0, "loglik_gradient: no observation functionals set on this level");
    ctx.activate();
    const size_t np = (size_t)d.n_p, nobs = (size_t)d.n_gobs;
    std::vector<double> q(kMaxBatch), gh(nobs * nbatch);
    enum { K, GH, GRAD, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::host(gh.data(), nobs), ChunkArg::out(grad, np, stage_grad),
                ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) { rhs_loglik(st, nb, lvl, data, noise, c.at<double>(GH)); },
                                  wrt_log, q.data(), c.at<double>(GRAD), nullptr, nullptr, nullptr, c.at<pmc_stats>(SA));
               });
    gauss_loglik(nbatch, nobs, gh.data(), data, noise, loglik, G);
}

// a Transport or a Tracer handed over with a call (noun: what the messages call it)
template <class T>
void Darcy::check_flux_user(int level, const T* t, const std::string& noun, const std::string& who) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, who + ": level out of range");
    PMC_REQUIRE(t != nullptr, who + ": " + noun + " is NULL");
    PMC_REQUIRE(t->n_face == lv[level].n_u && t->n_elem == lv[level].n_p,
                who + ": the " + noun + "'s mesh does not match the level (n_face != n_u or n_elem != n_p)");
    PMC_REQUIRE(t->ctx.device == ctx.device, who + ": the " + noun + " was created on another device");
}

void Darcy::transport_gradient(int level, Transport* t, int nbatch, const double* kf, const double* curve_bar,
                               const double* stored_bar, bool wrt_log, double* curve, double* stored, int32_t* status, double* grad,
                               double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    const std::string who = "pmc_darcy_transport_gradient";
    check_flux_user(level, t, "transport", who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && status != nullptr, who + ": bad arguments");
    PMC_REQUIRE(curve_bar != nullptr || stored_bar != nullptr, who + ": curve_bar or stored_bar must be given");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, who + ": bad memspace");
    ctx.activate();
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p, nr = (size_t)t->nreport;
    std::vector<double> q(kMaxBatch);
    enum { K, CB, SB, CURVE, STORED, GRAD, SOL, ADJ, STATUS, SF, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::in(curve_bar, nr, tr_cb), ChunkArg::in(stored_bar, 1, tr_sb),
                ChunkArg::made(curve, nr), ChunkArg::made(stored, 1), ChunkArg::out(grad, np, stage_grad),
                ChunkArg::out(sol_out, n, stage_sol), ChunkArg::out(adj_out, n, stage_out), ChunkArg::host(status, 1),
                ChunkArg::stats(stats_fwd), ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   tr_curve.ensure(nr * c.nb);
                   tr_stored.ensure(c.nb);
                   c.dev[CURVE] = tr_curve.p;
                   c.dev[STORED] = tr_stored.p;
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) {
                                      rhs_transport(st, nb, lvl, *t, c.at<double>(CB), c.at<double>(SB), nullptr, 1.0, tr_curve.p,
                                                    tr_stored.p, c.at<int32_t>(STATUS));
                                  },
                                  wrt_log, q.data(), c.at<double>(GRAD), c.at<double>(SOL), c.at<double>(ADJ), c.at<pmc_stats>(SF),
                                  c.at<pmc_stats>(SA));
               });
}

void Darcy::transport_loglik_gradient(int level, Transport* t, int nbatch, const double* kf, const double* data, double noise,
                                      bool wrt_log, double* loglik, double* curve, int32_t* status, double* grad, int memspace,
                                      pmc_stats* stats_adj) {
    const std::string who = "pmc_darcy_transport_loglik_gradient";
    check_flux_user(level, t, "transport", who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr && status != nullptr, who + ": bad arguments");
    PMC_REQUIRE(noise > 0.0, who + ": the noise variance must be positive");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, who + ": bad memspace");
    ctx.activate();
    DarcyLevel& d = lv[level];
    const size_t np = (size_t)d.n_p, nr = (size_t)t->nreport;
    std::vector<double> q(kMaxBatch), ch(nr * nbatch);
    tr_data.upload(data, nr, ctx.stream);
    enum { K, CH, GRAD, STATUS, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::made_host(ch.data(), nr), ChunkArg::out(grad, np, stage_grad),
                ChunkArg::host(status, 1), ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   tr_curve.ensure(nr * c.nb);
                   tr_stored.ensure(c.nb);
                   c.dev[CH] = tr_curve.p;
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) {
                                      rhs_transport(st, nb, lvl, *t, nullptr, nullptr, tr_data.p, noise, tr_curve.p, tr_stored.p,
                                                    c.at<int32_t>(STATUS));
                                  },
                                  wrt_log, q.data(), c.at<double>(GRAD), nullptr, nullptr, nullptr, c.at<pmc_stats>(SA));
               });
    gauss_loglik(nbatch, nr, ch.data(), data, noise, loglik, curve);
}

void Darcy::tracer_gradient(int level, Tracer* t, int nbatch, const double* kf, const double* T_bar, bool wrt_log, double* T,
                            int32_t* status, double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                            pmc_stats* stats_adj) {
    const std::string who = "pmc_darcy_tracer_gradient";
    check_flux_user(level, t, "tracer", who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && status != nullptr && T_bar != nullptr, who + ": bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, who + ": bad memspace");
    ctx.activate();
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p, npt = (size_t)t->npart;
    std::vector<double> q(kMaxBatch);
    enum { K, TB, T_, STATUS, GRAD, SOL, ADJ, SF, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::in(T_bar, npt, trc_tb), ChunkArg::made(T, npt),
                ChunkArg::made(status, npt), ChunkArg::out(grad, np, stage_grad), ChunkArg::out(sol_out, n, stage_sol),
                ChunkArg::out(adj_out, n, stage_out), ChunkArg::stats(stats_fwd), ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   trc_T.ensure(npt * c.nb);
                   trc_i.ensure(3 * npt * c.nb);
                   int32_t* status_d = trc_i.p + 2 * npt * c.nb;
                   c.dev[T_] = trc_T.p;
                   c.dev[STATUS] = status_d;
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) {
                                      rhs_tracer(st, nb, lvl, *t, c.at<double>(TB), nullptr, 1.0, trc_T.p, status_d);
                                  },
                                  wrt_log, q.data(), c.at<double>(GRAD), c.at<double>(SOL), c.at<double>(ADJ), c.at<pmc_stats>(SF),
                                  c.at<pmc_stats>(SA));
               });
}

void Darcy::tracer_loglik_gradient(int level, Tracer* t, int nbatch, const double* kf, const double* data, double noise,
                                   bool wrt_log, double* loglik, double* T, int32_t* not_exited, double* grad, int memspace,
                                   pmc_stats* stats_adj) {
    const std::string who = "pmc_darcy_tracer_loglik_gradient";
    check_flux_user(level, t, "tracer", who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr && not_exited != nullptr, who + ": bad arguments");
    PMC_REQUIRE(noise > 0.0, who + ": the noise variance must be positive");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, who + ": bad memspace");
    ctx.activate();
    DarcyLevel& d = lv[level];
    const size_t np = (size_t)d.n_p, npt = (size_t)t->npart;
    std::vector<double> q(kMaxBatch), th(npt * nbatch);
    trc_data.upload(data, npt, ctx.stream);
    enum { K, TH, NEX, GRAD, SA };
    for_chunks(level, nbatch, memspace,
               {ChunkArg::in(kf, np, stage_k), ChunkArg::made_host(th.data(), npt), ChunkArg::made_host(not_exited, 1),
                ChunkArg::out(grad, np, stage_grad), ChunkArg::stats(stats_adj)},
               [&](const Chunk& c) {
                   trc_T.ensure(npt * c.nb);
                   trc_i.ensure(3 * npt * c.nb);
                   gradient_chunk(level, c.nb, c.at<double>(K),
                                  [&](hipStream_t st, int nb, int lvl) {
                                      rhs_tracer(st, nb, lvl, *t, nullptr, trc_data.p, noise, trc_T.p, trc_i.p + 2 * npt * c.nb);
                                  },
                                  wrt_log, q.data(), c.at<double>(GRAD), nullptr, nullptr, nullptr, c.at<pmc_stats>(SA));
                   c.dev[TH] = trc_T.p;
                   c.dev[NEX] = t->nex.p;                // the tracer's count of particles that did not exit, per column
               });
    gauss_loglik(nbatch, npt, th.data(), data, noise, loglik, T);
}

}  // namespace pmc

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

// One launch: forward solve (all rows), adjoint right-hand side, adjoint solve on the same operator and preconditioner,
// gradient kernel.  grad_d / sol_d / adj_d: device, sample-major.
void Darcy::gradient_chunk(int level, int nb, const double* k_d, const AdjointSpec& adj, bool wrt_log, double* Q_host,
                           double* G_host, double* grad_d, double* sol_d, double* adj_d, pmc_stats* stats_fwd,
                           pmc_stats* stats_adj) {
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const int n_u = d.n_u, n_p = d.n_p, n = n_u + n_p;
    ensure(level, nb);
    ensure_gradient(level);
    adj_rhs.ensure((size_t)n * nb);
    adj_sol.ensure((size_t)n * nb);
    if (stats_fwd) ctx.phase_mark(0);
    setup_chunk(level, nb, k_d);             // M(k), Schur hierarchy, l1 diagonals: serves both solves
    if (stats_fwd) ctx.phase_mark(1);
    LinOp A;
    PrecFn prec;
    chunk_ops(level, nb, opts.use_graph == 0, A, prec);
    DarcyChain* chain = (level < (int)chains.size()) ? chains[level].get() : nullptr;
    Multigrid* mgp = chain ? &chain->mg : &mg;
    const int mg_l0 = chain ? 0 : level;
    work.want_r32 = false;
    // forward solve on all rows: the configuration (and the captured graph) of solve_fwd with a solution requested
    GraphHint hint;
    hint.key = hash_mix(hash_mix(hash_mix(0xda, (uint64_t)level + 1), (uint64_t)nb), 2);
    hint.sig = mgp->signature(mg_l0);
    for (const void* p : {(const void*)cx.p, (const void*)cd.p, (const void*)cx2.p, (const void*)d.mvals.p, (const void*)d.mvals_scaled.p,
                          (const void*)d.l1invM.p, (const void*)d.rhs_bc.p})
        hint.sig = hash_ptr(hint.sig, p);
    MinresResult res = minres_solve(ctx, nb, A, prec, d.rhs_bc.p, sol.p, true, opts, work, 0, n, nullptr, hint);
    if (stats_fwd) {
        ctx.phase_mark(2);
        for (int kcol = 0; kcol < nb; ++kcol) stats_fwd[kcol] = res.col[kcol];
        ctx.phase_report(stats_fwd, nb);
    }
    if (op_timer.on) op_timer.harvest();
    if (poly_timer.on) poly_timer.harvest();
    // Q = <obs, sol> over all rows, as solve_fwd forms it when the solution is requested - also on a level with a tracer
    // attached (pmc_darcy_set_tracer): the gradient is that of <obs, x>, so its Q stays <obs, x>
    const int qblocks = k::wdot(st, nb, n, d.obs.p, sol.p, qpartial.p);
    k::reduce_final(st, nb, qblocks, qpartial.p, qout.p);
    PMC_HIP(hipMemcpyAsync(ctx.h_scal, qout.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    if (sol_d) k::deinterleave(st, nb, n, sol.p, nullptr, nullptr, false, sol_d);
    if (stats_adj) ctx.phase_mark(0);
    // adjoint right-hand side, essential rows zero
    if (adj.loglik) {
        ensure_loglik(level);
        gtmp.ensure((size_t)d.n_gobs * nb);
        gout.ensure((size_t)d.n_gobs * nb);
        sol_compact.ensure((size_t)std::max(d.n_grows, 1) * nb);
        obs_data.upload(adj.data, (size_t)d.n_gobs, st);
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
                                                           obs_data.p, -1.0 / adj.noise, adj_rhs.p + (size_t)n_u * nb);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(2);
    } else if (adj.transport) {
        // J of the breakthrough data: the transport and its adjoint on the interleaved solution (minres_solve has synchronised
        // the stream, as Transport::qoi_interleaved requires), u_bar straight into the u rows, zero p rows and essential rows
        Transport& T = *adj.transport;
        T.adjoint_forward(st, nb, sol.p, nb, 1, adj.curve_d, adj.stored_d);
        for (int kcol = 0; kcol < nb; ++kcol) adj.status_h[kcol] = T.h_status[kcol];
        const double* cb_d = adj.tdata_d ? T.loglik_seed(st, nb, adj.curve_d, adj.tdata_d, adj.noise) : adj.curve_bar_d;
        T.adjoint_backward(st, nb, sol.p, nb, 1, cb_d, adj.tdata_d ? nullptr : adj.stored_bar_d, nullptr, adj_rhs.p, nb, 1, nullptr);
        k::fill(st, (size_t)n_p * nb, adj_rhs.p + (size_t)n_u * nb, 0.0);
        const size_t tu = (size_t)n_u * nb;
        zero_ess_rows_kernel<<<flat_blocks(tu), 256, 0, st>>>(tu, nb, d.ess.p, adj_rhs.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    } else if (adj.tracer) {
        // J of the travel times: the walk and its adjoint on the interleaved solution, u_bar straight into the u rows, zero
        // p rows and essential rows
        Tracer& T = *adj.tracer;
        const size_t cnt = (size_t)nb * T.npart;
        trc_i.ensure(2 * cnt);
        T.adjoint_launch(st, nb, true, sol.p, nb, 1, adj.tbar_d, nullptr, adj_rhs.p, nb, 1, nullptr, adj.trT_d, trc_i.p,
                         adj.trstatus_d, trc_i.p + cnt, adj.trdata_d, adj.noise);
        k::fill(st, (size_t)n_p * nb, adj_rhs.p + (size_t)n_u * nb, 0.0);
        const size_t tu = (size_t)n_u * nb;
        zero_ess_rows_kernel<<<flat_blocks(tu), 256, 0, st>>>(tu, nb, d.ess.p, adj_rhs.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    } else {
        if (adj.rhs_d) k::interleave(st, nb, n, adj.rhs_d, nullptr, 1.0, adj_rhs.p);
        else k::broadcast(st, nb, n, d.obs.p, adj_rhs.p);
        const size_t tu = (size_t)n_u * nb;
        zero_ess_rows_kernel<<<flat_blocks(tu), 256, 0, st>>>(tu, nb, d.ess.p, adj_rhs.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
    PMC_HIP(hipStreamSynchronize(st));           // Q (and G) have arrived; the data of the right-hand side was read
    for (int kcol = 0; kcol < nb; ++kcol) Q_host[kcol] = ctx.h_scal[kcol];
    if (stats_adj) ctx.phase_mark(1);
    // adjoint solve: same A, prec and options, zero guess, a configuration (graph key) of its own
    GraphHint hint_adj;
    hint_adj.key = hash_mix(hash_mix(hash_mix(0xda, (uint64_t)level + 1), (uint64_t)nb), 5);
    hint_adj.sig = hash_ptr(hash_ptr(hint.sig, adj_rhs.p), adj_sol.p);
    MinresResult res_adj = minres_solve(ctx, nb, A, prec, adj_rhs.p, adj_sol.p, true, opts, work, 0, n, nullptr, hint_adj);
    if (stats_adj) {
        ctx.phase_mark(2);
        for (int kcol = 0; kcol < nb; ++kcol) stats_adj[kcol] = res_adj.col[kcol];
        ctx.phase_report(stats_adj, nb);
    }
    if (op_timer.on) op_timer.harvest();
    if (poly_timer.on) poly_timer.harvest();
    const k::ElemMassView E{n_p, d.grad_nslices, d.grad_nfe, d.grad_faces.p, d.grad_me.p};
    if (grad_timer.on) grad_timer.begin(st);
    k::darcy_mass_sensitivity(st, nb, E, k_d, sol.p, adj_sol.p, k_divides, wrt_log, grad_d);
    if (grad_timer.on) grad_timer.end(st);
    if (adj_d) k::deinterleave(st, nb, n, adj_sol.p, nullptr, nullptr, false, adj_d);
    PMC_HIP(hipStreamSynchronize(st));
    if (grad_timer.on) grad_timer.harvest();
}

void Darcy::mass_sensitivity(int level, int nbatch, const double* kf, const double* x, const double* lam, bool wrt_log,
                             double* grad, int memspace) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "mass_sensitivity: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && x != nullptr && lam != nullptr && grad != nullptr,
                "mass_sensitivity: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p;
    ensure_gradient(level);
    const k::ElemMassView E{d.n_p, d.grad_nslices, d.grad_nfe, d.grad_faces.p, d.grad_me.p};
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        const double* k_d = kf + (size_t)done * d.n_p;
        const double* x_d = x + (size_t)done * n;
        const double* l_d = lam + (size_t)done * n;
        double* g_d = grad + (size_t)done * d.n_p;
        sol.ensure(n * nb);
        adj_sol.ensure(n * nb);
        if (memspace == PMC_MEM_HOST) {
            stage_k.ensure((size_t)d.n_p * nb);
            stage_sol.ensure(n * nb);
            stage_adj.ensure(n * nb);
            stage_grad.ensure((size_t)d.n_p * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, k_d, sizeof(double) * d.n_p * nb, hipMemcpyHostToDevice, st));
            PMC_HIP(hipMemcpyAsync(stage_sol.p, x_d, sizeof(double) * n * nb, hipMemcpyHostToDevice, st));
            PMC_HIP(hipMemcpyAsync(stage_adj.p, l_d, sizeof(double) * n * nb, hipMemcpyHostToDevice, st));
            k_d = stage_k.p;
            x_d = stage_sol.p;
            l_d = stage_adj.p;
            g_d = stage_grad.p;
        }
        k::interleave(st, nb, (int)n, x_d, nullptr, 1.0, sol.p);
        k::interleave(st, nb, (int)n, l_d, nullptr, 1.0, adj_sol.p);
        if (grad_timer.on) grad_timer.begin(st);
        k::darcy_mass_sensitivity(st, nb, E, k_d, sol.p, adj_sol.p, k_divides, wrt_log, g_d);
        if (grad_timer.on) grad_timer.end(st);
        if (memspace == PMC_MEM_HOST)
            PMC_HIP(hipMemcpyAsync(grad + (size_t)done * d.n_p, stage_grad.p, sizeof(double) * d.n_p * nb,
                                   hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        if (grad_timer.on) grad_timer.harvest();
        done += nb;
    }
}

void Darcy::solve_gradient(int level, int nbatch, const double* kf, const double* adj_rhs_in, bool wrt_log, double* Q,
                           double* C, double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                           pmc_stats* stats_adj) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "solve_gradient: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr, "solve_gradient: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch);
    DevBuf<double> stage_out;                 // host memspace: the adjoint solution on its way out
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        struct { const double *k_d, *rhs_d; double *grad_d, *sol_d, *adj_d; } s{
            kf + done * np, adj_rhs_in ? adj_rhs_in + done * n : nullptr, grad + done * np,
            sol_out ? sol_out + done * n : nullptr, adj_out ? adj_out + done * n : nullptr};
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, s.k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            s.k_d = stage_k.p;
            if (s.rhs_d) {
                stage_adj.ensure(n * nb);
                PMC_HIP(hipMemcpyAsync(stage_adj.p, s.rhs_d, sizeof(double) * n * nb, hipMemcpyHostToDevice, st));
                s.rhs_d = stage_adj.p;
            }
            s.grad_d = stage_grad.p;
            if (s.sol_d) s.sol_d = stage_sol.p;
            if (s.adj_d) {
                stage_out.ensure(n * nb);
                s.adj_d = stage_out.p;
            }
        }
        AdjointSpec adj;
        adj.rhs_d = s.rhs_d;
        gradient_chunk(level, nb, s.k_d, adj, wrt_log, q.data(), nullptr, s.grad_d, s.sol_d, s.adj_d,
                       stats_fwd ? stats_fwd + done : nullptr, stats_adj ? stats_adj + done : nullptr);
        if (host) {
            PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
            if (sol_out) PMC_HIP(hipMemcpyAsync(sol_out + done * n, stage_sol.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
            if (adj_out) PMC_HIP(hipMemcpyAsync(adj_out + done * n, stage_out.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
            PMC_HIP(hipStreamSynchronize(st));
        }
        for (int b = 0; b < nb; ++b) {
            if (Q) Q[done + b] = q[b];
            if (C) C[done + b] = (double)n;
        }
        done += nb;
    }
}

void Darcy::loglik_gradient(int level, int nbatch, const double* kf, const double* data, double noise, bool wrt_log,
                            double* loglik, double* G, double* grad, int memspace, pmc_stats* stats_adj) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "loglik_gradient: level out of range");
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr, "loglik_gradient: bad arguments");
    PMC_REQUIRE(noise > 0.0, "loglik_gradient: the noise variance must be positive");
    DarcyLevel& d = lv[level];
    PMC_REQUIRE(d.n_gobs > 0, "loglik_gradient: no observation functionals set on this level");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p;
    const int nobs = d.n_gobs;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch), gh((size_t)nobs * kMaxBatch);
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        const double* k_d = kf + done * np;
        double* grad_d = grad + done * np;
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            k_d = stage_k.p;
            grad_d = stage_grad.p;
        }
        AdjointSpec adj;
        adj.loglik = true;
        adj.data = data;
        adj.noise = noise;
        gradient_chunk(level, nb, k_d, adj, wrt_log, q.data(), gh.data(), grad_d, nullptr, nullptr, nullptr,
                       stats_adj ? stats_adj + done : nullptr);
        if (host) {
            PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
            PMC_HIP(hipStreamSynchronize(st));
        }
        for (int b = 0; b < nb; ++b) {
            double s = 0.0;
            for (int i = 0; i < nobs; ++i) {
                const double dd = gh[(size_t)b * nobs + i] - data[i];
                s += dd * dd;
                if (G) G[(size_t)(done + b) * nobs + i] = gh[(size_t)b * nobs + i];
            }
            if (loglik) loglik[done + b] = (-1. / (noise * 2)) * s;      // log of BayesianInverseProblem::ComputeLikelihood
        }
        done += nb;
    }
}

void Darcy::check_transport(int level, const Transport* t, const char* who) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, std::string(who) + ": level out of range");
    PMC_REQUIRE(t != nullptr, std::string(who) + ": transport is NULL");
    PMC_REQUIRE(t->n_face == lv[level].n_u && t->n_elem == lv[level].n_p,
                std::string(who) + ": the transport's mesh does not match the level (n_face != n_u or n_elem != n_p)");
    PMC_REQUIRE(t->ctx.device == ctx.device, std::string(who) + ": the transport was created on another device");
}

void Darcy::transport_gradient(int level, Transport* t, int nbatch, const double* kf, const double* curve_bar,
                               const double* stored_bar, bool wrt_log, double* curve, double* stored, int32_t* status, double* grad,
                               double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd, pmc_stats* stats_adj) {
    const char* who = "pmc_darcy_transport_gradient";
    check_transport(level, t, who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && status != nullptr, std::string(who) + ": bad arguments");
    PMC_REQUIRE(curve_bar != nullptr || stored_bar != nullptr, std::string(who) + ": curve_bar or stored_bar must be given");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, std::string(who) + ": bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p, nr = (size_t)t->nreport;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch);
    DevBuf<double> stage_out;
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        struct { const double *k_d, *cb_d, *sb_d; double *grad_d, *sol_d, *adj_d; } s{
            kf + done * np, curve_bar ? curve_bar + done * nr : nullptr, stored_bar ? stored_bar + done : nullptr, grad + done * np,
            sol_out ? sol_out + done * n : nullptr, adj_out ? adj_out + done * n : nullptr};
        tr_curve.ensure(nr * nb);
        tr_stored.ensure(nb);
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, s.k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            s.k_d = stage_k.p;
            if (s.cb_d) {
                tr_cb.upload(s.cb_d, nr * nb, st);
                s.cb_d = tr_cb.p;
            }
            if (s.sb_d) {
                tr_sb.upload(s.sb_d, nb, st);
                s.sb_d = tr_sb.p;
            }
            s.grad_d = stage_grad.p;
            if (s.sol_d) s.sol_d = stage_sol.p;
            if (s.adj_d) {
                stage_out.ensure(n * nb);
                s.adj_d = stage_out.p;
            }
        }
        AdjointSpec adj;
        adj.transport = t;
        adj.curve_bar_d = s.cb_d;
        adj.stored_bar_d = s.sb_d;
        adj.curve_d = tr_curve.p;
        adj.stored_d = tr_stored.p;
        adj.status_h = status + done;
        gradient_chunk(level, nb, s.k_d, adj, wrt_log, q.data(), nullptr, s.grad_d, s.sol_d, s.adj_d,
                       stats_fwd ? stats_fwd + done : nullptr, stats_adj ? stats_adj + done : nullptr);
        const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (curve) PMC_HIP(hipMemcpyAsync(curve + done * nr, tr_curve.p, sizeof(double) * nr * nb, back, st));
        if (stored) PMC_HIP(hipMemcpyAsync(stored + done, tr_stored.p, sizeof(double) * nb, back, st));
        if (host) {
            PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
            if (sol_out) PMC_HIP(hipMemcpyAsync(sol_out + done * n, stage_sol.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
            if (adj_out) PMC_HIP(hipMemcpyAsync(adj_out + done * n, stage_out.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
        }
        PMC_HIP(hipStreamSynchronize(st));
        done += nb;
    }
}

void Darcy::transport_loglik_gradient(int level, Transport* t, int nbatch, const double* kf, const double* data, double noise,
                                      bool wrt_log, double* loglik, double* curve, int32_t* status, double* grad, int memspace,
                                      pmc_stats* stats_adj) {
    const char* who = "pmc_darcy_transport_loglik_gradient";
    check_transport(level, t, who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr && status != nullptr, std::string(who) + ": bad arguments");
    PMC_REQUIRE(noise > 0.0, std::string(who) + ": the noise variance must be positive");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, std::string(who) + ": bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p;
    const int nr = t->nreport;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch), ch((size_t)nr * kMaxBatch);
    tr_data.upload(data, (size_t)nr, st);
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        const double* k_d = kf + done * np;
        double* grad_d = grad + done * np;
        tr_curve.ensure((size_t)nr * nb);
        tr_stored.ensure(nb);
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            k_d = stage_k.p;
            grad_d = stage_grad.p;
        }
        AdjointSpec adj;
        adj.transport = t;
        adj.tdata_d = tr_data.p;
        adj.noise = noise;
        adj.curve_d = tr_curve.p;
        adj.stored_d = tr_stored.p;
        adj.status_h = status + done;
        gradient_chunk(level, nb, k_d, adj, wrt_log, q.data(), nullptr, grad_d, nullptr, nullptr, nullptr,
                       stats_adj ? stats_adj + done : nullptr);
        PMC_HIP(hipMemcpyAsync(ch.data(), tr_curve.p, sizeof(double) * nr * nb, hipMemcpyDeviceToHost, st));
        if (host) PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < nb; ++b) {
            double s = 0.0;
            for (int i = 0; i < nr; ++i) {
                const double dd = ch[(size_t)b * nr + i] - data[i];
                s += dd * dd;
                if (curve) curve[(size_t)(done + b) * nr + i] = ch[(size_t)b * nr + i];
            }
            if (loglik) loglik[done + b] = (-1. / (noise * 2)) * s;
        }
        done += nb;
    }
}

void Darcy::check_tracer(int level, const Tracer* t, const char* who) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, std::string(who) + ": level out of range");
    PMC_REQUIRE(t != nullptr, std::string(who) + ": tracer is NULL");
    PMC_REQUIRE(t->n_face == lv[level].n_u && t->n_elem == lv[level].n_p,
                std::string(who) + ": the tracer's mesh does not match the level (n_face != n_u or n_elem != n_p)");
    PMC_REQUIRE(t->ctx.device == ctx.device, std::string(who) + ": the tracer was created on another device");
}

void Darcy::tracer_gradient(int level, Tracer* t, int nbatch, const double* kf, const double* T_bar, bool wrt_log, double* T,
                            int32_t* status, double* grad, double* sol_out, double* adj_out, int memspace, pmc_stats* stats_fwd,
                            pmc_stats* stats_adj) {
    const char* who = "pmc_darcy_tracer_gradient";
    check_tracer(level, t, who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && status != nullptr && T_bar != nullptr,
                std::string(who) + ": bad arguments");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, std::string(who) + ": bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p, npt = (size_t)t->npart;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch);
    DevBuf<double> stage_out;
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        struct { const double *k_d, *tb_d; double *grad_d, *sol_d, *adj_d; } s{
            kf + done * np, T_bar + done * npt, grad + done * np, sol_out ? sol_out + done * n : nullptr,
            adj_out ? adj_out + done * n : nullptr};
        trc_T.ensure(npt * nb);
        trc_i.ensure(3 * npt * nb);
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, s.k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            s.k_d = stage_k.p;
            trc_tb.upload(s.tb_d, npt * nb, st);
            s.tb_d = trc_tb.p;
            s.grad_d = stage_grad.p;
            if (s.sol_d) s.sol_d = stage_sol.p;
            if (s.adj_d) {
                stage_out.ensure(n * nb);
                s.adj_d = stage_out.p;
            }
        }
        AdjointSpec adj;
        adj.tracer = t;
        adj.tbar_d = s.tb_d;
        adj.trT_d = trc_T.p;
        adj.trstatus_d = trc_i.p + 2 * npt * nb;
        gradient_chunk(level, nb, s.k_d, adj, wrt_log, q.data(), nullptr, s.grad_d, s.sol_d, s.adj_d,
                       stats_fwd ? stats_fwd + done : nullptr, stats_adj ? stats_adj + done : nullptr);
        const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (T) PMC_HIP(hipMemcpyAsync(T + done * npt, trc_T.p, sizeof(double) * npt * nb, back, st));
        PMC_HIP(hipMemcpyAsync(status + done * npt, adj.trstatus_d, sizeof(int32_t) * npt * nb, back, st));
        if (host) {
            PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
            if (sol_out) PMC_HIP(hipMemcpyAsync(sol_out + done * n, stage_sol.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
            if (adj_out) PMC_HIP(hipMemcpyAsync(adj_out + done * n, stage_out.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
        }
        PMC_HIP(hipStreamSynchronize(st));
        done += nb;
    }
}

void Darcy::tracer_loglik_gradient(int level, Tracer* t, int nbatch, const double* kf, const double* data, double noise,
                                   bool wrt_log, double* loglik, double* T, int32_t* not_exited, double* grad, int memspace,
                                   pmc_stats* stats_adj) {
    const char* who = "pmc_darcy_tracer_loglik_gradient";
    check_tracer(level, t, who);
    PMC_REQUIRE(nbatch >= 1 && kf != nullptr && grad != nullptr && data != nullptr && not_exited != nullptr,
                std::string(who) + ": bad arguments");
    PMC_REQUIRE(noise > 0.0, std::string(who) + ": the noise variance must be positive");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, std::string(who) + ": bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    DarcyLevel& d = lv[level];
    const size_t n = (size_t)d.n_u + d.n_p, np = (size_t)d.n_p, npt = (size_t)t->npart;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<double> q(kMaxBatch), th(npt * kMaxBatch);
    trc_data.upload(data, npt, st);
    int done = 0;
    while (done < nbatch) {
        int nb = batch_width(n, true, ctx.device);
        while (nb > nbatch - done) nb >>= 1;
        const double* k_d = kf + done * np;
        double* grad_d = grad + done * np;
        trc_T.ensure(npt * nb);
        trc_i.ensure(3 * npt * nb);
        if (host) {
            ensure(level, nb);
            stage_grad.ensure(np * nb);
            PMC_HIP(hipMemcpyAsync(stage_k.p, k_d, sizeof(double) * np * nb, hipMemcpyHostToDevice, st));
            k_d = stage_k.p;
            grad_d = stage_grad.p;
        }
        AdjointSpec adj;
        adj.tracer = t;
        adj.trdata_d = trc_data.p;
        adj.noise = noise;
        adj.trT_d = trc_T.p;
        adj.trstatus_d = trc_i.p + 2 * npt * nb;
        gradient_chunk(level, nb, k_d, adj, wrt_log, q.data(), nullptr, grad_d, nullptr, nullptr, nullptr,
                       stats_adj ? stats_adj + done : nullptr);
        PMC_HIP(hipMemcpyAsync(th.data(), trc_T.p, sizeof(double) * npt * nb, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(not_exited + done, t->nex.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
        if (host) PMC_HIP(hipMemcpyAsync(grad + done * np, stage_grad.p, sizeof(double) * np * nb, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < nb; ++b) {
            double s = 0.0;
            for (size_t i = 0; i < npt; ++i) {
                const double dd = th[(size_t)b * npt + i] - data[i];
                s += dd * dd;
                if (T) T[(size_t)(done + b) * npt + i] = th[(size_t)b * npt + i];
            }
            if (loglik) loglik[done + b] = (-1. / (noise * 2)) * s;
        }
        done += nb;
    }
}

}  // namespace pmc

// First-order upwind transport of a passive solute on the Darcy flux (pmc_transport_*; numpy twin:
// parelagmc_amd/fe/transport.py).
//
// The scheme needs no geometry.  A row of the level's divergence matrix B lists the flux dofs of an element with their signs;
// the outward volume rate of element e through its l-th row entry is g_l = sign(B[e, f]) * (a_f * u_f) with one magnitude
// a_f per dof, so what leaves one element enters its neighbour bit for bit.  Per realization
//     out_e = sum_l max(g_l, 0),  in_e = sum_l max(-g_l, 0),  r_e = max(out_e, in_e),  rate = max_e r_e / V_e
//     nsteps = max(1, ceil((t_end * rate) / cfl)),  dt = t_end / nsteps,  w_e = dt / V_e,  d_e = 1 - w_e r_e
//     c_e' = d_e c_e + w_e sum_l max(-g_l, 0) cn_l
// (cn_l the neighbour's old concentration, c_in[f] on a boundary dof), every sum from 0.0 in ascending l.  The kernels follow
// the twin operation for operation; fused multiply-adds are switched off for this file so that the products round as numpy's.
//
// One thread per (element, realization) on the interleaved layout c[e * nb + b], one launch per time step, two concentration
// buffers: step s reads buffer s & 1 and writes the other, a column b with nsteps_b steps ends in buffer nsteps_b & 1 and its
// threads return at once in later launches.  Nothing is precomputed per (element, realization): a step re-reads the flux
// (each dof is shared by two elements and stays in the L2) and recomputes r_e, d_e, w_e and the inflow coefficients, which
// costs no memory and less traffic than streaming them.  The flux is read through (stride_face, stride_batch), so one
// kernel body serves the public sample-major input and the solver's interleaved solution with the same bits.
//
// Outlet dofs are boundary dofs, so each belongs to one element: the thread of that element keeps the dof's accumulator
// acc_j += dt m_j (no atomics) and, in the step n_r a report time r falls into, stores acc_j + tau_r m_j into a snapshot
// [r][j][b].  One launch after the last step sums every snapshot over j, and wgt_e c_e over e, in the order of the pmc_tracer
// reduction (thread t adds t, t + 256, ... ascending, a shuffle tree per wave, the wave sums ascending).
#include "handles.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace pmc {

namespace {

constexpr int kTransportThreads = 256;

__host__ __device__ inline int dof_id(int32_t enc) { return enc < 0 ? ~enc : enc; }

// what every kernel reads of the handle
struct TransportView {
    int n_elem, n_outlet, nreport, nnz;
    const int32_t* rec;      // width W > 0: per element enc[W], nbr[W]; general: enc[nnz], nbr[nnz]
    const int32_t* rowptr;   // general form only
    const double *a, *cin, *vol, *c0, *wgt;
};

// the row entries of element e in ascending order: f(enc, nbr).  enc is the dof f, or ~f where B[e, f] < 0; nbr is the other
// element of an interior dof, -1 on a boundary dof that is no outlet, -2 - j on outlet j.
template <int W, class F>
__device__ __forceinline__ void for_row(const TransportView& v, int e, F&& f) {
    if constexpr (W > 0) {
        int32_t enc[W], nbr[W];
        const int32_t* r = v.rec + (size_t)e * (2 * W);
#pragma unroll
        for (int l = 0; l < W; ++l) {
            enc[l] = r[l];
            nbr[l] = r[W + l];
        }
#pragma unroll
        for (int l = 0; l < W; ++l) f(enc[l], nbr[l]);
    } else {
        const int end = v.rowptr[e + 1];
        for (int p = v.rowptr[e]; p < end; ++p) f(v.rec[p], v.rec[(size_t)v.nnz + p]);
    }
}

__device__ __forceinline__ double outward(const TransportView& v, const double* __restrict__ ub, int64_t stride_face, int32_t enc) {
    const int f = dof_id(enc);
    const double g = v.a[f] * ub[(int64_t)f * stride_face];
    return enc < 0 ? -g : g;
}

// q[e * nb + b] = r_e / V_e (+inf where a rate of the row or the quotient is not finite) and c[e * nb + b] = c0[e]
template <int W>
__global__ __launch_bounds__(kTransportThreads) void transport_rates_kernel(TransportView v, int nb, const double* __restrict__ u,
                                                                            int64_t stride_face, int64_t stride_batch,
                                                                            double* __restrict__ c, double* __restrict__ q) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned e = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (e >= (unsigned)v.n_elem) return;
    const double* ub = u + (int64_t)b * stride_batch;
    double out = 0.0, in = 0.0;
    bool bad = false;
    for_row<W>(v, (int)e, [&](int32_t enc, int32_t) {
        const double g = outward(v, ub, stride_face, enc);
        bad = bad || !isfinite(g);
        out += fmax(g, 0.0);
        in += fmax(-g, 0.0);
    });
    const double r = fmax(out, in);
    const double qe = r / v.vol[e];
    q[(size_t)gid] = (bad || !isfinite(qe)) ? INFINITY : qe;
    c[(size_t)gid] = v.c0[e];
}

// rate[b] = max_e q[e * nb + b]: no entry is a NaN, so the maximum does not depend on the order
__global__ __launch_bounds__(kTransportThreads) void transport_rate_max_kernel(int n_elem, int nb, const double* __restrict__ q,
                                                                               double* __restrict__ rate) {
    __shared__ double wmax[kTransportThreads / 64];
    const int b = blockIdx.x;
    double m = 0.0;
    for (int e = threadIdx.x; e < n_elem; e += kTransportThreads) m = fmax(m, q[(size_t)e * nb + b]);
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTransportThreads / 64; ++w) m = fmax(m, wmax[w]);
        rate[b] = m;
    }
}

// step s of every column that has one: buf holds the two concentration buffers (n_elem * nb each)
template <int W>
__global__ __launch_bounds__(kTransportThreads) void transport_step_kernel(TransportView v, int nb, int s, const double* __restrict__ u,
                                                                           int64_t stride_face, int64_t stride_batch,
                                                                           const double* __restrict__ dtcol,
                                                                           const int32_t* __restrict__ ncol, double* buf,
                                                                           double* __restrict__ acc, double* __restrict__ snap) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned e = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (e >= (unsigned)v.n_elem) return;
    const int nsteps = ncol[b];
    if (s >= nsteps) return;
    const size_t len = (size_t)v.n_elem * nb;
    const double* src = buf + (s & 1) * len;
    double* dst = buf + ((s + 1) & 1) * len;
    const double* ub = u + (int64_t)b * stride_batch;
    const double dt = dtcol[b];
    const double w = dt / v.vol[e];
    const double ce = src[gid];
    double out = 0.0, in = 0.0, sacc = 0.0;
    for_row<W>(v, (int)e, [&](int32_t enc, int32_t nbr) {
        const double g = outward(v, ub, stride_face, enc);
        const double go = fmax(g, 0.0), gi = fmax(-g, 0.0);
        out += go;
        in += gi;
        const double cn = nbr >= 0 ? src[(size_t)nbr * nb + b] : v.cin[dof_id(enc)];
        sacc += gi * cn;
        if (nbr <= -2) {
            // an outlet dof of this element: its accumulator and the report times that fall into this step
            const int j = -2 - nbr;
            const size_t jb = (size_t)j * nb + b;
            const double m = go * ce;
            const double a0 = s ? acc[jb] : 0.0;
            const int64_t R = v.nreport, N = nsteps;
            int64_t r = ((int64_t)s * R + N - 1) / N;
            if (r < 1) r = 1;
            for (; r <= R; ++r) {
                const int64_t at = (r * N) / R, nr = at < N - 1 ? at : N - 1;
                if (nr != s) break;
                const double tau = ((double)(r * N - nr * R) / (double)R) * dt;
                snap[((size_t)(r - 1) * v.n_outlet + j) * nb + b] = a0 + tau * m;
            }
            acc[jb] = a0 + dt * m;
        }
    });
    const double r = fmax(out, in);
    const double d = 1.0 - w * r;
    dst[gid] = d * ce + w * sacc;
}

__device__ __forceinline__ double block_sum(double acc, double* wsum) {
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = wsum[0];
    for (int w = 1; w < kTransportThreads / 64; ++w) s += wsum[w];
    return s;
}

// blockIdx.x < nreport: curve[b][x] = sum_j snap[x][j][b] (0 for a column that took no step); blockIdx.x == nreport:
// stored[b] = sum_e wgt_e c_e in the column's final buffer.  q (may be NULL) receives the QoI of `kind`.
__global__ __launch_bounds__(kTransportThreads) void transport_finish_kernel(TransportView v, int nb, const int32_t* __restrict__ ncol,
                                                                             const double* __restrict__ buf,
                                                                             const double* __restrict__ snap, double* __restrict__ curve,
                                                                             double* __restrict__ stored, int kind, double* __restrict__ q) {
    __shared__ double wsum[kTransportThreads / 64];
    const int x = blockIdx.x, b = blockIdx.y;
    const int nsteps = ncol[b];
    double acc = 0.0;
    if (x < v.nreport) {
        if (nsteps > 0)
            for (int j = threadIdx.x; j < v.n_outlet; j += kTransportThreads) acc += snap[((size_t)x * v.n_outlet + j) * nb + b];
    } else {
        const double* c = buf + (size_t)(nsteps & 1) * v.n_elem * nb;
        for (int e = threadIdx.x; e < v.n_elem; e += kTransportThreads) acc += v.wgt[e] * c[(size_t)e * nb + b];
    }
    const double s = block_sum(acc, wsum);
    if (threadIdx.x != 0) return;
    if (x < v.nreport) {
        curve[(size_t)b * v.nreport + x] = s;
        if (q && kind == PMC_TRANSPORT_MASS_OUT && x == v.nreport - 1) q[b] = s;
    } else {
        stored[b] = s;
        if (q && kind == PMC_TRANSPORT_STORED) q[b] = s;
    }
}

// c_out[b][e] = the column's final buffer
__global__ __launch_bounds__(kTransportThreads) void transport_copy_out_kernel(int n_elem, int nb, const int32_t* __restrict__ ncol,
                                                                               const double* __restrict__ buf, double* __restrict__ c_out) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned b = gid / (unsigned)n_elem, e = gid % (unsigned)n_elem;
    if (b >= (unsigned)nb) return;
    c_out[gid] = buf[(size_t)(ncol[b] & 1) * n_elem * nb + (size_t)e * nb + b];
}

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kTransportThreads - 1) / kTransportThreads); }

}  // namespace

Transport::Transport(Ctx& c, const pmc_transport_mesh& m, const pmc_transport_params& p)
    : ctx(c), n_elem(m.n_elem), n_face(m.n_face), nreport(p.nreport), t_end(p.t_end), cfl(p.cfl) {
    PMC_REQUIRE(n_elem >= 1 && n_face >= 1, "pmc_transport_create: empty mesh");
    PMC_REQUIRE(m.rowptr && m.col && m.val && m.pore_volume, "pmc_transport_create: NULL array");
    PMC_REQUIRE(p.t_end > 0.0 && std::isfinite(p.t_end), "pmc_transport_create: t_end must be positive");
    PMC_REQUIRE(p.cfl > 0.0 && p.cfl <= 1.0, "pmc_transport_create: cfl outside (0, 1]");
    PMC_REQUIRE(p.nreport >= 1 && p.nreport <= 4096, "pmc_transport_create: nreport outside [1, 4096]");
    PMC_REQUIRE(p.max_steps >= 0 && p.max_steps <= (1 << 24), "pmc_transport_create: max_steps outside [0, 2^24]");
    max_steps = p.max_steps ? p.max_steps : 65536;
    PMC_REQUIRE(m.rowptr[0] == 0, "pmc_transport_create: bad rowptr");
    for (int e = 0; e < n_elem; ++e) PMC_REQUIRE(m.rowptr[e + 1] >= m.rowptr[e], "pmc_transport_create: bad rowptr");
    const int nnz = m.rowptr[n_elem];
    // every column of B: one entry (boundary) or two in different elements, of opposite sign and equal magnitude
    std::vector<int32_t> first(n_face, -1), second(n_face, -1);   // positions of a column's entries, ascending element
    for (int e = 0; e < n_elem; ++e) {
        PMC_REQUIRE(std::isfinite(m.pore_volume[e]) && m.pore_volume[e] > 0.0, "pmc_transport_create: pore volumes must be positive and finite");
        PMC_REQUIRE(!m.c0 || std::isfinite(m.c0[e]), "pmc_transport_create: c0 must be finite");
        PMC_REQUIRE(!m.weight || std::isfinite(m.weight[e]), "pmc_transport_create: weight must be finite");
        for (int q = m.rowptr[e]; q < m.rowptr[e + 1]; ++q) {
            const int32_t f = m.col[q];
            PMC_REQUIRE(f >= 0 && f < n_face, "pmc_transport_create: column index out of range");
            PMC_REQUIRE(std::isfinite(m.val[q]) && m.val[q] != 0.0, "pmc_transport_create: B holds a zero or non-finite entry");
            PMC_REQUIRE(second[f] < 0, "pmc_transport_create: a column of B must have one or two entries");
            (first[f] < 0 ? first[f] : second[f]) = q;
        }
    }
    std::vector<int32_t> row_of(nnz);
    for (int e = 0; e < n_elem; ++e)
        for (int q = m.rowptr[e]; q < m.rowptr[e + 1]; ++q) row_of[q] = e;
    std::vector<double> a_h(n_face), cin_h(n_face, 1.0);
    std::vector<int32_t> outlet_of(n_face, -1);
    n_outlet = 0;
    for (int f = 0; f < n_face; ++f) {
        PMC_REQUIRE(first[f] >= 0, "pmc_transport_create: a column of B must have one or two entries");
        const double va = m.val[first[f]];
        a_h[f] = std::fabs(va);
        if (second[f] >= 0) {
            const double vb = m.val[second[f]];
            PMC_REQUIRE(row_of[first[f]] != row_of[second[f]] && !(va * vb > 0.0) &&
                            std::fabs(va + vb) <= 1e-12 * std::max(std::fabs(va), std::fabs(vb)),
                        "pmc_transport_create: the two entries of a column of B must lie in two elements, with opposite signs and equal magnitudes");
            PMC_REQUIRE(!m.outlet || !m.outlet[f], "pmc_transport_create: an outlet flag on an interior dof");
        } else if (!m.outlet || m.outlet[f]) {
            outlet_of[f] = n_outlet++;
        }
        if (m.c_in) {
            PMC_REQUIRE(std::isfinite(m.c_in[f]), "pmc_transport_create: c_in must be finite");
            cin_h[f] = m.c_in[f];
        }
    }
    // rows: a register form for rows of exactly 3, 4 or 6 entries, the general form otherwise
    int wmin = nnz, wmax = 0;
    for (int e = 0; e < n_elem; ++e) {
        wmin = std::min(wmin, m.rowptr[e + 1] - m.rowptr[e]);
        wmax = std::max(wmax, m.rowptr[e + 1] - m.rowptr[e]);
    }
    width = (wmin == wmax && (wmax == 3 || wmax == 4 || wmax == 6)) ? wmax : 0;
    std::vector<int32_t> rec_h(2 * (size_t)nnz);
    for (int e = 0; e < n_elem; ++e)
        for (int q = m.rowptr[e]; q < m.rowptr[e + 1]; ++q) {
            const int32_t f = m.col[q];
            const int32_t other = second[f] < 0 ? (outlet_of[f] >= 0 ? -2 - outlet_of[f] : -1) : row_of[first[f] == q ? second[f] : first[f]];
            const int l = q - m.rowptr[e];
            const size_t at_enc = width ? (size_t)e * 2 * width + l : (size_t)q;
            const size_t at_nbr = width ? (size_t)e * 2 * width + width + l : (size_t)nnz + q;
            rec_h[at_enc] = m.val[q] > 0.0 ? f : ~f;
            rec_h[at_nbr] = other;
        }
    nnz_ = nnz;
    std::vector<double> c0_h(n_elem, 0.0);
    if (m.c0) std::copy(m.c0, m.c0 + n_elem, c0_h.begin());
    const double* wsrc = m.weight ? m.weight : m.pore_volume;
    ctx.activate();
    hipStream_t st = ctx.stream;
    rec.upload(rec_h, st);
    rowptr.upload(m.rowptr, (size_t)n_elem + 1, st);
    a.upload(a_h, st);
    cin.upload(cin_h, st);
    vol.upload(m.pore_volume, n_elem, st);
    c0.upload(c0_h, st);
    wgt.upload(wsrc, n_elem, st);
    PMC_HIP(hipStreamSynchronize(st));
}

// the whole computation for nb columns on stream st; the results stay in cbuf / curve_d / stored_d and the h_* vectors
void Transport::compute(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch, double* curve_d,
                        double* stored_d, int kind, double* q_d) {
    PMC_REQUIRE((int64_t)n_elem * nb < (int64_t(1) << 31), "pmc_transport: n_elem x nbatch of one launch must stay below 2^31");
    const size_t len = (size_t)n_elem * nb;
    cbuf.ensure(2 * len);
    acc.ensure((size_t)std::max(n_outlet, 1) * nb);
    snap.ensure((size_t)nreport * std::max(n_outlet, 1) * nb);
    col_rate.ensure(nb);
    col_dt.ensure(nb);
    col_steps.ensure(nb);
    const TransportView v{n_elem, n_outlet, nreport, nnz_, rec.p, rowptr.p, a.p, cin.p, vol.p, c0.p, wgt.p};
    const unsigned grid = blocks_for(len);
    auto by_width = [&](auto&& launch) {
        switch (width) {
            case 3: launch(std::integral_constant<int, 3>{}); break;
            case 4: launch(std::integral_constant<int, 4>{}); break;
            case 6: launch(std::integral_constant<int, 6>{}); break;
            default: launch(std::integral_constant<int, 0>{}); break;
        }
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    };
    // c = c0 into buffer 0, r_e / V_e into buffer 1 (which step 0 overwrites), their maximum per column
    by_width([&](auto W) {
        transport_rates_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(v, nb, u_d, stride_face, stride_batch, cbuf.p,
                                                                                       cbuf.p + len);
    });
    transport_rate_max_kernel<<<(unsigned)nb, kTransportThreads, 0, st>>>(n_elem, nb, cbuf.p + len, col_rate.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    h_rate.resize(nb);
    h_dt.resize(nb);
    h_treached.resize(nb);
    h_steps.resize(nb);
    h_status.resize(nb);
    PMC_HIP(hipMemcpyAsync(h_rate.data(), col_rate.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    int longest = 0;
    for (int b = 0; b < nb; ++b) {
        const double rate = h_rate[b];
        if (!std::isfinite(rate)) {
            h_status[b] = PMC_TRANSPORT_BAD_FLUX;
            h_steps[b] = 0;
            h_dt[b] = 0.0;
            h_treached[b] = 0.0;
            continue;
        }
        const double x = (t_end * rate) / cfl;
        const double cx = std::ceil(x);
        if (cx > (double)max_steps) {
            h_status[b] = PMC_TRANSPORT_STEP_LIMIT;
            h_steps[b] = max_steps;
            h_dt[b] = cfl / rate;
            h_treached[b] = (double)max_steps * h_dt[b];
        } else {
            h_status[b] = PMC_TRANSPORT_OK;
            h_steps[b] = cx < 1.0 ? 1 : (int32_t)cx;
            h_dt[b] = t_end / (double)h_steps[b];
            h_treached[b] = t_end;
        }
        longest = std::max(longest, h_steps[b]);
    }
    col_dt.upload(h_dt, st);
    col_steps.upload(h_steps, st);
    for (int s = 0; s < longest; ++s)
        by_width([&](auto W) {
            transport_step_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(v, nb, s, u_d, stride_face, stride_batch, col_dt.p,
                                                                                          col_steps.p, cbuf.p, acc.p, snap.p);
        });
    transport_finish_kernel<<<dim3((unsigned)nreport + 1, (unsigned)nb), kTransportThreads, 0, st>>>(v, nb, col_steps.p, cbuf.p, snap.p,
                                                                                                      curve_d, stored_d, kind, q_d);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

void Transport::run(int nbatch, const double* u, int64_t ld, double* c_out, double* curve, double* stored, double* rate,
                    double* t_reached, int32_t* nsteps, int32_t* status, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_transport_run: nbatch must be at least 1");
    PMC_REQUIRE(u && curve && stored && rate && t_reached && nsteps && status, "pmc_transport_run: NULL array");
    PMC_REQUIRE(ld >= n_face, "pmc_transport_run: ld is smaller than the number of flux dofs");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_transport_run: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const bool host = memspace == PMC_MEM_HOST;
    // pieces of at most 2^24 flux values / concentrations
    const int per = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t(1) << 24) / std::max(n_face, n_elem)));
    if (host) {
        stage_u.ensure((size_t)per * n_face);
        out_curve.ensure((size_t)per * nreport);
        out_stored.ensure(per);
        if (c_out) out_c.ensure((size_t)per * n_elem);
    }
    const hipMemcpyKind scal = host ? hipMemcpyHostToHost : hipMemcpyHostToDevice;
    for (int b0 = 0; b0 < nbatch; b0 += per) {
        const int n = std::min(per, nbatch - b0);
        const double* u_d = u + (size_t)b0 * ld;
        int64_t stride_batch = ld;
        if (host) {
            PMC_HIP(hipMemcpy2DAsync(stage_u.p, sizeof(double) * n_face, u_d, sizeof(double) * ld, sizeof(double) * n_face, n,
                                     hipMemcpyHostToDevice, st));
            u_d = stage_u.p;
            stride_batch = n_face;
        }
        double* curve_d = host ? out_curve.p : curve + (size_t)b0 * nreport;
        double* stored_d = host ? out_stored.p : stored + b0;
        compute(st, n, u_d, 1, stride_batch, curve_d, stored_d, 0, nullptr);
        if (c_out) {
            double* c_d = host ? out_c.p : c_out + (size_t)b0 * n_elem;
            transport_copy_out_kernel<<<blocks_for((size_t)n * n_elem), kTransportThreads, 0, st>>>(n_elem, n, col_steps.p, cbuf.p, c_d);
            PMC_HIP(hipGetLastError());
            count_kernel_launches(1);
            if (host) PMC_HIP(hipMemcpyAsync(c_out + (size_t)b0 * n_elem, c_d, sizeof(double) * n * n_elem, hipMemcpyDeviceToHost, st));
        }
        if (host) {
            PMC_HIP(hipMemcpyAsync(curve + (size_t)b0 * nreport, curve_d, sizeof(double) * n * nreport, hipMemcpyDeviceToHost, st));
            PMC_HIP(hipMemcpyAsync(stored + b0, stored_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        }
        PMC_HIP(hipMemcpyAsync(rate + b0, h_rate.data(), sizeof(double) * n, scal, st));
        PMC_HIP(hipMemcpyAsync(t_reached + b0, h_treached.data(), sizeof(double) * n, scal, st));
        PMC_HIP(hipMemcpyAsync(nsteps + b0, h_steps.data(), sizeof(int32_t) * n, scal, st));
        PMC_HIP(hipMemcpyAsync(status + b0, h_status.data(), sizeof(int32_t) * n, scal, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

void Transport::reduce(int nbatch, const double* curve, const double* stored, int kind, double* Q, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_transport_reduce: nbatch must be at least 1");
    PMC_REQUIRE(curve && stored && Q, "pmc_transport_reduce: NULL array");
    PMC_REQUIRE(kind == PMC_TRANSPORT_MASS_OUT || kind == PMC_TRANSPORT_STORED, "pmc_transport_reduce: kind must be PMC_TRANSPORT_MASS_OUT or _STORED");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_transport_reduce: bad memspace");
    const bool out = kind == PMC_TRANSPORT_MASS_OUT;
    const double* src = out ? curve + (nreport - 1) : stored;
    const size_t pitch = sizeof(double) * (out ? nreport : 1);
    if (memspace == PMC_MEM_HOST) {
        for (int b = 0; b < nbatch; ++b) Q[b] = src[(size_t)b * (out ? nreport : 1)];
        return;
    }
    ctx.activate();
    PMC_HIP(hipMemcpy2DAsync(Q, sizeof(double), src, pitch, sizeof(double), nbatch, hipMemcpyDeviceToHost, ctx.stream));
    PMC_HIP(hipStreamSynchronize(ctx.stream));
}

// the hook of Darcy::solve_chunk*: the transport on the interleaved solution sol[row * nb + col] (its first n_face rows are
// the flux block), the QoI of `kind` into q_d[0..nb) on the caller's stream.  Reads the nb rates on the host in between: the
// solve that calls it has synchronised the stream already.
void Transport::qoi_interleaved(hipStream_t st, int nb, const double* sol, int kind, double* q_d) {
    out_curve.ensure((size_t)nb * nreport);
    out_stored.ensure(nb);
    compute(st, nb, sol, nb, 1, out_curve.p, out_stored.p, kind, q_d);
}

}  // namespace pmc

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
#include <cstdint>
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

// the arithmetic of step s for element e of column b: c^{s+1}_e from the state src.  kOutlet: also the accumulators of the
// element's outlet dofs and the report times that fall into this step.  The forward kernel, the checkpointed forward pass of
// the adjoint and its recomputation all go through here, so a recomputed state has the forward bits.
template <int W, bool kOutlet>
__device__ __forceinline__ double step_value(const TransportView& v, int nb, int s, int nsteps, unsigned gid, unsigned e, unsigned b,
                                             const double* ub, int64_t stride_face, double dt, const double* __restrict__ src,
                                             double* __restrict__ acc, double* __restrict__ snap) {
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
        if (kOutlet && nbr <= -2) {
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
    return d * ce + w * sacc;
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
    dst[gid] = step_value<W, true>(v, nb, s, nsteps, gid, e, b, u + (int64_t)b * stride_batch, stride_face, dtcol[b], src, acc, snap);
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
// stored[b] = sum_e wgt_e c_e in the column's final buffer, buf + (nsteps & 1) * half (half 0: one buffer of final states).
// q (may be NULL) receives the QoI of `kind`.
__global__ __launch_bounds__(kTransportThreads) void transport_finish_kernel(TransportView v, int nb, const int32_t* __restrict__ ncol,
                                                                             const double* __restrict__ buf, size_t half,
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
        const double* c = buf + (size_t)(nsteps & 1) * half;
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

// ---- the discrete adjoint (pmc_transport_run_adjoint) ----------------------------------------------
// J = <curve_bar, curve> + stored_bar stored + <c_bar, c^N> per column, differentiated in u with three decisions of the forward
// pass held fixed: the step count, the sign of every g and the branch sigma_e = (out_e >= in_e) of r_e.  The forward pass
// keeps every K-th state; the backward sweep recomputes one segment of K states at a time with step_value and walks it
// backwards, one launch per step:
//     lam^n_e = d_e lam^{n+1}_e + sum_l go_l y_l,   y_l = w_nbr lam^{n+1}_nbr | beta^n on an outlet dof | 0
// while the element's thread accumulates P_e = sum_n c^n_e lam^{n+1}_e, X_f = sum_n cn^n_f lam^{n+1}_e for the dofs f through
// which it takes inflow (a dof is the inflow of at most one element: X is kept per dof, no atomics) and
// O_j = sum_n beta^n c^n_e for its outlet dofs.  The sweep stores w_e lam_e beside lam_e so that a neighbour reads the
// product instead of dividing.  One thread per (dof, column) then assembles u_bar.

// step s from src to dst; cfin (may be NULL) receives the state after a column's last step
template <int W, bool kOutlet>
__global__ __launch_bounds__(kTransportThreads) void transport_step_to_kernel(TransportView v, int nb, int s, const double* __restrict__ u,
                                                                              int64_t stride_face, int64_t stride_batch,
                                                                              const double* __restrict__ dtcol,
                                                                              const int32_t* __restrict__ ncol,
                                                                              const double* __restrict__ src, double* __restrict__ dst,
                                                                              double* __restrict__ acc, double* __restrict__ snap,
                                                                              double* __restrict__ cfin) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned e = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (e >= (unsigned)v.n_elem) return;
    const int nsteps = ncol[b];
    if (s >= nsteps) return;
    const double c1 = step_value<W, kOutlet>(v, nb, s, nsteps, gid, e, b, u + (int64_t)b * stride_batch, stride_face, dtcol[b], src, acc, snap);
    dst[gid] = c1;
    if (cfin && s == nsteps - 1) cfin[gid] = c1;
}

// beta[n * nb + b] = dt sum_{r: n_r > n} curve_bar[b][r] + sum_{r: n_r == n} tau_r curve_bar[b][r], r ascending in both sums
__global__ __launch_bounds__(kTransportThreads) void transport_beta_kernel(int nb, int nreport, int longest, const int32_t* __restrict__ ncol,
                                                                           const double* __restrict__ dtcol,
                                                                           const double* __restrict__ curve_bar, double* __restrict__ beta) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned n = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (n >= (unsigned)longest) return;
    const int64_t R = nreport, N = ncol[b];
    if (!curve_bar || (int64_t)n >= N) {
        beta[gid] = 0.0;
        return;
    }
    const double dt = dtcol[b];
    const double* cb = curve_bar + (size_t)b * nreport;
    double s1 = 0.0;
    for (int64_t r = 1; r <= R; ++r) {
        const int64_t at = (r * N) / R, nr = at < N - 1 ? at : N - 1;
        if (nr > (int64_t)n) s1 += cb[r - 1];
    }
    double be = dt * s1;
    for (int64_t r = 1; r <= R; ++r) {
        const int64_t at = (r * N) / R, nr = at < N - 1 ? at : N - 1;
        if (nr == (int64_t)n) be += (((double)(r * N - nr * R) / (double)R) * dt) * cb[r - 1];
    }
    beta[gid] = be;
}

// lam^N_e = stored_bar wgt_e + c_bar_e and w_e lam^N_e into both buffers of the pair: a column's first sweep step n = N - 1
// reads the buffer (n + 1) & 1, whatever its N.  stored_bar (nb) and c_bar (nb x n_elem) may be NULL: zero.
__global__ __launch_bounds__(kTransportThreads) void transport_adjoint_init_kernel(TransportView v, int nb, const double* __restrict__ dtcol,
                                                                                   const double* __restrict__ stored_bar,
                                                                                   const double* __restrict__ c_bar, double* __restrict__ lam,
                                                                                   double* __restrict__ wlam) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned e = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (e >= (unsigned)v.n_elem) return;
    const size_t len = (size_t)v.n_elem * nb;
    const double sb = stored_bar ? stored_bar[b] : 0.0;
    const double cb = c_bar ? c_bar[(size_t)b * v.n_elem + e] : 0.0;
    const double l = sb * v.wgt[e] + cb;
    const double wl = (dtcol[b] / v.vol[e]) * l;
    lam[gid] = l;
    lam[len + gid] = l;
    wlam[gid] = wl;
    wlam[len + gid] = wl;
}

// sweep step n of every column that has one: c holds c^n, (lam1, wlam1) the pair of step n + 1, (lam0, wlam0) receives step n
template <int W>
__global__ __launch_bounds__(kTransportThreads) void transport_adjoint_step_kernel(
    TransportView v, int nb, int n, const double* __restrict__ u, int64_t stride_face, int64_t stride_batch,
    const double* __restrict__ dtcol, const int32_t* __restrict__ ncol, const double* __restrict__ beta, const double* __restrict__ c,
    const double* __restrict__ lam1, const double* __restrict__ wlam1, double* __restrict__ lam0, double* __restrict__ wlam0,
    double* __restrict__ P, double* __restrict__ X, double* __restrict__ O, uint8_t* __restrict__ sig) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned e = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (e >= (unsigned)v.n_elem) return;
    if (n >= ncol[b]) return;
    const double* ub = u + (int64_t)b * stride_batch;
    const double w = dtcol[b] / v.vol[e];
    const double ce = c[gid], l1 = lam1[gid], bn = beta[(size_t)n * nb + b];
    double out = 0.0, in = 0.0, sacc = 0.0;
    for_row<W>(v, (int)e, [&](int32_t enc, int32_t nbr) {
        const double g = outward(v, ub, stride_face, enc);
        const double go = fmax(g, 0.0), gi = fmax(-g, 0.0);
        out += go;
        in += gi;
        double y = 0.0;
        if (nbr >= 0) {
            y = wlam1[(size_t)nbr * nb + b];
        } else if (nbr <= -2) {
            const size_t jb = (size_t)(-2 - nbr) * nb + b;
            y = bn;
            O[jb] += bn * ce;
        }
        sacc += go * y;
        if (g < 0.0) {
            const int f = dof_id(enc);
            const double cn = nbr >= 0 ? c[(size_t)nbr * nb + b] : v.cin[f];
            X[(size_t)f * nb + b] += cn * l1;
        }
    });
    const double r = fmax(out, in);
    const double d = 1.0 - w * r;
    const double l0 = d * l1 + sacc;
    lam0[gid] = l0;
    wlam0[gid] = w * l0;
    P[gid] += ce * l1;
    if (n == 0) sig[gid] = out >= in ? 1 : 0;
}

// u_bar of dof f, column b, written to ubar[f * stride_face_out + b * stride_batch_out]; side: per dof the element of its
// first entry and of its second (INT32_MIN: none), ~e where B[e, f] < 0, and its outlet index or -1.  Zero for a column
// that was not differentiated (ncol 0).
__global__ __launch_bounds__(kTransportThreads) void transport_adjoint_assemble_kernel(
    TransportView v, int n_face, const int32_t* __restrict__ side, int nb, const double* __restrict__ u, int64_t stride_face,
    int64_t stride_batch, const double* __restrict__ dtcol, const int32_t* __restrict__ ncol, const double* __restrict__ P,
    const double* __restrict__ X, const double* __restrict__ O, const uint8_t* __restrict__ sig, double* __restrict__ ubar,
    int64_t stride_face_out, int64_t stride_batch_out) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned f = gid / (unsigned)nb, b = gid % (unsigned)nb;
    if (f >= (unsigned)n_face) return;
    double* dst = ubar + (int64_t)f * stride_face_out + (int64_t)b * stride_batch_out;
    if (ncol[b] == 0) {
        *dst = 0.0;
        return;
    }
    const double af = v.a[f];
    const double gf = af * u[(int64_t)b * stride_batch + (int64_t)f * stride_face];
    const double dt = dtcol[b];
    const int j = side[3 * (size_t)f + 2];
    double sum = 0.0;
    for (int k = 0; k < 2; ++k) {
        const int32_t enc = side[3 * (size_t)f + k];
        if (enc == INT32_MIN) break;
        const bool neg = enc < 0;
        const size_t eb = (size_t)(neg ? ~enc : enc) * nb + b;
        const double g = neg ? -gf : gf;
        const double w = dt / v.vol[neg ? ~enc : enc];
        const double t1 = w * P[eb];
        const bool sg = sig[eb] != 0;
        double G = 0.0;
        if (g > 0.0 && sg) G = -t1;
        else if (g < 0.0 && !sg) G = t1;
        if (g < 0.0) G = G - w * X[gid];
        if (j >= 0 && g > 0.0) G = G + O[(size_t)j * nb + b];
        sum += neg ? -G : G;
    }
    *dst = af * sum;
}

// c0_bar[b][e] = lam^0, zero for a column that was not differentiated
__global__ __launch_bounds__(kTransportThreads) void transport_adjoint_c0_kernel(int n_elem, int nb, const int32_t* __restrict__ ncol,
                                                                                 const double* __restrict__ lam, double* __restrict__ c0_bar) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    const unsigned b = gid / (unsigned)n_elem, e = gid % (unsigned)n_elem;
    if (b >= (unsigned)nb) return;
    c0_bar[gid] = ncol[b] ? lam[(size_t)e * nb + b] : 0.0;
}

// curve_bar[b][r] = -(curve[b][r] - data[r]) / noise: the seed of loglik = -|curve - data|^2 / (2 noise)
__global__ __launch_bounds__(kTransportThreads) void transport_loglik_seed_kernel(int nb, int nreport, const double* __restrict__ curve,
                                                                                  const double* __restrict__ data, double noise,
                                                                                  double* __restrict__ curve_bar) {
    const unsigned gid = blockIdx.x * kTransportThreads + threadIdx.x;
    if (gid >= (unsigned)nb * (unsigned)nreport) return;
    curve_bar[gid] = -(curve[gid] - data[gid % (unsigned)nreport]) / noise;
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
    // per dof for the adjoint's assembly: its elements in ascending order (~e where B[e, f] < 0) and its outlet index
    std::vector<int32_t> side_h(3 * (size_t)n_face);
    for (int f = 0; f < n_face; ++f) {
        const auto enc_of = [&](int32_t q) { return m.val[q] > 0.0 ? row_of[q] : ~row_of[q]; };
        side_h[3 * (size_t)f] = enc_of(first[f]);
        side_h[3 * (size_t)f + 1] = second[f] >= 0 ? enc_of(second[f]) : INT32_MIN;
        side_h[3 * (size_t)f + 2] = outlet_of[f];
    }
    std::vector<double> c0_h(n_elem, 0.0);
    if (m.c0) std::copy(m.c0, m.c0 + n_elem, c0_h.begin());
    const double* wsrc = m.weight ? m.weight : m.pore_volume;
    ctx.activate();
    hipStream_t st = ctx.stream;
    rec.upload(rec_h, st);
    side.upload(side_h, st);
    rowptr.upload(m.rowptr, (size_t)n_elem + 1, st);
    a.upload(a_h, st);
    cin.upload(cin_h, st);
    vol.upload(m.pore_volume, n_elem, st);
    c0.upload(c0_h, st);
    wgt.upload(wsrc, n_elem, st);
    PMC_HIP(hipStreamSynchronize(st));
}

// one launch of a kernel templated on the row form: launch(std::integral_constant<int, W>) with W = 3 | 4 | 6 for the register
// forms, 0 for the general form
template <class F>
void Transport::by_width(F&& launch) const {
    switch (width) {
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        default: launch(std::integral_constant<int, 0>{}); break;
    }
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

// rate[b] = max_e q[e * nb + b] and from it, on the host, the step count, step size and status of every column (h_*), uploaded
// into col_dt / col_steps.  Returns the largest step count.
int Transport::plan_columns(hipStream_t st, int nb, const double* q_d) {
    transport_rate_max_kernel<<<(unsigned)nb, kTransportThreads, 0, st>>>(n_elem, nb, q_d, col_rate.p);
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
    return longest;
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
    // c = c0 into buffer 0, r_e / V_e into buffer 1 (which step 0 overwrites), their maximum per column
    by_width([&](auto W) {
        transport_rates_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(v, nb, u_d, stride_face, stride_batch, cbuf.p,
                                                                                       cbuf.p + len);
    });
    const int longest = plan_columns(st, nb, cbuf.p + len);
    for (int s = 0; s < longest; ++s)
        by_width([&](auto W) {
            transport_step_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(v, nb, s, u_d, stride_face, stride_batch, col_dt.p,
                                                                                          col_steps.p, cbuf.p, acc.p, snap.p);
        });
    transport_finish_kernel<<<dim3((unsigned)nreport + 1, (unsigned)nb), kTransportThreads, 0, st>>>(v, nb, col_steps.p, cbuf.p, len, snap.p,
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

void Transport::set_adjoint_segment(int K) {
    PMC_REQUIRE(K >= 0, "pmc_transport_set_adjoint_segment: K must not be negative");
    adj_segment = K;
}

// plan, then the forward pass: state s of the pass lives in checkpoint s / K where K divides s (and the sweep will want it),
// else in a pair of buffers by parity; every column's final state is copied to adj_fin by the thread that forms it
void Transport::adjoint_forward(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch, double* curve_d,
                                double* stored_d) {
    PMC_REQUIRE((int64_t)std::max(n_elem, n_face) * nb < (int64_t(1) << 31),
                "pmc_transport: n_elem x nbatch and n_face x nbatch of one launch must stay below 2^31");
    const size_t len = (size_t)n_elem * nb;
    adj_tmp.ensure(2 * len);
    adj_fin.ensure(len);
    acc.ensure((size_t)std::max(n_outlet, 1) * nb);
    snap.ensure((size_t)nreport * std::max(n_outlet, 1) * nb);
    col_rate.ensure(nb);
    col_dt.ensure(nb);
    col_steps.ensure(nb);
    const TransportView v{n_elem, n_outlet, nreport, nnz_, rec.p, rowptr.p, a.p, cin.p, vol.p, c0.p, wgt.p};
    const unsigned grid = blocks_for(len);
    // c^0 into the final states (a column without a step ends there), r_e / V_e into the pair
    by_width([&](auto W) {
        transport_rates_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(v, nb, u_d, stride_face, stride_batch, adj_fin.p,
                                                                                       adj_tmp.p);
    });
    adj_longest_fwd = plan_columns(st, nb, adj_tmp.p);
    // only columns whose status is OK are differentiated: the others take no part in the recomputation and the sweep
    h_steps_adj.resize(nb);
    adj_longest = 0;
    for (int b = 0; b < nb; ++b) {
        h_steps_adj[b] = h_status[b] == PMC_TRANSPORT_OK ? h_steps[b] : 0;
        adj_longest = std::max(adj_longest, h_steps_adj[b]);
    }
    col_steps_adj.upload(h_steps_adj, st);
    adj_K = adj_segment ? adj_segment : (int)std::ceil(std::sqrt((double)adj_longest));
    adj_K = std::max(1, std::min(adj_K, std::max(adj_longest, 1)));
    while ((int64_t)adj_K * adj_K < adj_longest && !adj_segment) ++adj_K;
    adj_nck = std::max(1, (adj_longest + adj_K - 1) / adj_K);
    adj_ck.ensure((size_t)adj_nck * len);
    PMC_HIP(hipMemcpyAsync(adj_ck.p, adj_fin.p, sizeof(double) * len, hipMemcpyDeviceToDevice, st));
    auto loc = [&](int s) {
        return (s % adj_K == 0 && s / adj_K < adj_nck) ? adj_ck.p + (size_t)(s / adj_K) * len : adj_tmp.p + (size_t)(s & 1) * len;
    };
    for (int s = 0; s < adj_longest_fwd; ++s)
        by_width([&](auto W) {
            transport_step_to_kernel<decltype(W)::value, true><<<grid, kTransportThreads, 0, st>>>(
                v, nb, s, u_d, stride_face, stride_batch, col_dt.p, col_steps.p, loc(s), loc(s + 1), acc.p, snap.p, adj_fin.p);
        });
    transport_finish_kernel<<<dim3((unsigned)nreport + 1, (unsigned)nb), kTransportThreads, 0, st>>>(v, nb, col_steps.p, adj_fin.p, 0, snap.p,
                                                                                                      curve_d, stored_d, 0, nullptr);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

void Transport::adjoint_backward(hipStream_t st, int nb, const double* u_d, int64_t stride_face, int64_t stride_batch,
                                 const double* curve_bar_d, const double* stored_bar_d, const double* c_bar_d, double* ubar_d,
                                 int64_t stride_face_out, int64_t stride_batch_out, double* c0_bar_d) {
    const size_t len = (size_t)n_elem * nb, flen = (size_t)n_face * nb, olen = (size_t)std::max(n_outlet, 1) * nb;
    const int K = adj_K, N = adj_longest;
    adj_seg.ensure((size_t)std::max(K - 1, 1) * len);
    adj_lam.ensure(2 * len);
    adj_wlam.ensure(2 * len);
    adj_beta.ensure((size_t)std::max(N, 1) * nb);
    adj_P.ensure(len);
    adj_X.ensure(flen);
    adj_O.ensure(olen);
    adj_sig.ensure(len);
    const TransportView v{n_elem, n_outlet, nreport, nnz_, rec.p, rowptr.p, a.p, cin.p, vol.p, c0.p, wgt.p};
    const unsigned grid = blocks_for(len);
    PMC_HIP(hipMemsetAsync(adj_P.p, 0, sizeof(double) * len, st));
    PMC_HIP(hipMemsetAsync(adj_X.p, 0, sizeof(double) * flen, st));
    PMC_HIP(hipMemsetAsync(adj_O.p, 0, sizeof(double) * olen, st));
    PMC_HIP(hipMemsetAsync(adj_sig.p, 0, len, st));
    if (N > 0) {
        transport_beta_kernel<<<blocks_for((size_t)N * nb), kTransportThreads, 0, st>>>(nb, nreport, N, col_steps_adj.p, col_dt.p, curve_bar_d,
                                                                                        adj_beta.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
    transport_adjoint_init_kernel<<<grid, kTransportThreads, 0, st>>>(v, nb, col_dt.p, stored_bar_d, c_bar_d, adj_lam.p, adj_wlam.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    for (int i = adj_nck - 1; i >= 0 && N > 0; --i) {
        const int n0 = i * K, n1 = std::min(n0 + K, N);
        auto state = [&](int n) { return n == n0 ? adj_ck.p + (size_t)i * len : adj_seg.p + (size_t)(n - n0 - 1) * len; };
        // the states n0 + 1 .. n1 - 1 of the segment, with the forward bits
        for (int n = n0; n + 1 < n1; ++n)
            by_width([&](auto W) {
                transport_step_to_kernel<decltype(W)::value, false><<<grid, kTransportThreads, 0, st>>>(
                    v, nb, n, u_d, stride_face, stride_batch, col_dt.p, col_steps_adj.p, state(n), state(n + 1), nullptr, nullptr, nullptr);
            });
        for (int n = n1 - 1; n >= n0; --n) {
            const size_t from = (size_t)((n + 1) & 1) * len, to = (size_t)(n & 1) * len;
            by_width([&](auto W) {
                transport_adjoint_step_kernel<decltype(W)::value><<<grid, kTransportThreads, 0, st>>>(
                    v, nb, n, u_d, stride_face, stride_batch, col_dt.p, col_steps_adj.p, adj_beta.p, state(n), adj_lam.p + from,
                    adj_wlam.p + from, adj_lam.p + to, adj_wlam.p + to, adj_P.p, adj_X.p, adj_O.p, adj_sig.p);
            });
        }
    }
    transport_adjoint_assemble_kernel<<<blocks_for(flen), kTransportThreads, 0, st>>>(
        v, n_face, side.p, nb, u_d, stride_face, stride_batch, col_dt.p, col_steps_adj.p, adj_P.p, adj_X.p, adj_O.p, adj_sig.p, ubar_d,
        stride_face_out, stride_batch_out);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    if (c0_bar_d) {
        transport_adjoint_c0_kernel<<<grid, kTransportThreads, 0, st>>>(n_elem, nb, col_steps_adj.p, adj_lam.p, c0_bar_d);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
}

const double* Transport::loglik_seed(hipStream_t st, int nb, const double* curve_d, const double* data_d, double noise) {
    seed_cb.ensure((size_t)nb * nreport);
    transport_loglik_seed_kernel<<<blocks_for((size_t)nb * nreport), kTransportThreads, 0, st>>>(nb, nreport, curve_d, data_d, noise,
                                                                                                 seed_cb.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    return seed_cb.p;
}

void Transport::run_adjoint(int nbatch, const double* u, int64_t ld, const double* curve_bar, const double* stored_bar,
                            const double* c_bar, double* u_bar, int64_t ld_bar, double* c0_bar, double* curve, double* stored,
                            int32_t* nsteps, int32_t* status, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_transport_run_adjoint: nbatch must be at least 1");
    PMC_REQUIRE(u && u_bar && status, "pmc_transport_run_adjoint: NULL array");
    PMC_REQUIRE(curve_bar || stored_bar || c_bar, "pmc_transport_run_adjoint: at least one of curve_bar, stored_bar and c_bar must be given");
    PMC_REQUIRE(ld >= n_face && ld_bar >= n_face, "pmc_transport_run_adjoint: ld or ld_bar is smaller than the number of flux dofs");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_transport_run_adjoint: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const bool host = memspace == PMC_MEM_HOST;
    const int per = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t(1) << 24) / std::max(n_face, n_elem)));
    out_curve.ensure((size_t)per * nreport);
    out_stored.ensure(per);
    if (host) {
        stage_u.ensure((size_t)per * n_face);
        stage_ubar.ensure((size_t)per * n_face);
        if (curve_bar) stage_cb.ensure((size_t)per * nreport);
        if (stored_bar) stage_sb.ensure(per);
        if (c_bar) stage_eb.ensure((size_t)per * n_elem);
        if (c0_bar) stage_c0bar.ensure((size_t)per * n_elem);
    }
    const hipMemcpyKind scal = host ? hipMemcpyHostToHost : hipMemcpyHostToDevice;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (int b0 = 0; b0 < nbatch; b0 += per) {
        const int n = std::min(per, nbatch - b0);
        const double* u_d = u + (size_t)b0 * ld;
        const double* cb_d = curve_bar ? curve_bar + (size_t)b0 * nreport : nullptr;
        const double* sb_d = stored_bar ? stored_bar + b0 : nullptr;
        const double* eb_d = c_bar ? c_bar + (size_t)b0 * n_elem : nullptr;
        double* ubar_d = u_bar + (size_t)b0 * ld_bar;
        double* c0bar_d = c0_bar ? c0_bar + (size_t)b0 * n_elem : nullptr;
        int64_t stride_batch = ld, stride_out = ld_bar;
        if (host) {
            PMC_HIP(hipMemcpy2DAsync(stage_u.p, sizeof(double) * n_face, u_d, sizeof(double) * ld, sizeof(double) * n_face, n,
                                     hipMemcpyHostToDevice, st));
            u_d = stage_u.p;
            stride_batch = n_face;
            if (cb_d) {
                PMC_HIP(hipMemcpyAsync(stage_cb.p, cb_d, sizeof(double) * n * nreport, hipMemcpyHostToDevice, st));
                cb_d = stage_cb.p;
            }
            if (sb_d) {
                PMC_HIP(hipMemcpyAsync(stage_sb.p, sb_d, sizeof(double) * n, hipMemcpyHostToDevice, st));
                sb_d = stage_sb.p;
            }
            if (eb_d) {
                PMC_HIP(hipMemcpyAsync(stage_eb.p, eb_d, sizeof(double) * n * n_elem, hipMemcpyHostToDevice, st));
                eb_d = stage_eb.p;
            }
            ubar_d = stage_ubar.p;
            stride_out = n_face;
            if (c0bar_d) c0bar_d = stage_c0bar.p;
        }
        adjoint_forward(st, n, u_d, 1, stride_batch, out_curve.p, out_stored.p);
        adjoint_backward(st, n, u_d, 1, stride_batch, cb_d, sb_d, eb_d, ubar_d, 1, stride_out, c0bar_d);
        if (host) {
            PMC_HIP(hipMemcpy2DAsync(u_bar + (size_t)b0 * ld_bar, sizeof(double) * ld_bar, stage_ubar.p, sizeof(double) * n_face,
                                     sizeof(double) * n_face, n, hipMemcpyDeviceToHost, st));
            if (c0_bar) PMC_HIP(hipMemcpyAsync(c0_bar + (size_t)b0 * n_elem, stage_c0bar.p, sizeof(double) * n * n_elem, hipMemcpyDeviceToHost, st));
        }
        if (curve) PMC_HIP(hipMemcpyAsync(curve + (size_t)b0 * nreport, out_curve.p, sizeof(double) * n * nreport, back, st));
        if (stored) PMC_HIP(hipMemcpyAsync(stored + b0, out_stored.p, sizeof(double) * n, back, st));
        if (nsteps) PMC_HIP(hipMemcpyAsync(nsteps + b0, h_steps.data(), sizeof(int32_t) * n, scal, st));
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

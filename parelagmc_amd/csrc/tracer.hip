// Particle travel times on the RT0 Darcy flux (pmc_tracer_*; numpy twin: parelagmc_amd/fe/tracer.py).
//
// One thread walks one particle of one realization through the mesh.  Inside an element every coordinate c (a box axis, a
// barycentric coordinate of a tetrahedron) obeys c' = v(c) with v affine in c, so the time to a candidate exit plane is
//     dt = (d / v) L(rho),   rho = (v_exit - v) / v,   L(rho) = log1p(rho) / rho                      (Pollock's method)
// and the other coordinates advance by c += v_c dt E(g_c dt), E(z) = expm1(z) / z.  The kernel follows the twin operation
// for operation (fused multiply-adds are switched off for this file so that the products round as numpy's do).
//
// Nothing is shared between threads: no LDS, no atomics, no scratch in the walk.  The flux is read through two strides, so
// the same kernel body serves the public sample-major layout (lanes along particles, blockIdx.y = realization) and the
// solver's interleaved solution sol[row * nb + col] (lanes along realizations: a wave starts in one element and its face
// gathers are contiguous).  A particle's results therefore have the same bits in both.  The walk is a for loop over a step
// counter bounded by max_steps; lanes that have finished idle under the exec mask, a wave costs its longest path.
//
// The per-realization QoI (tracer_reduce_kernel) is one workgroup per realization: thread t adds the particles t, t + 256, ...
// in ascending order, the 256 partial sums go through a fixed shuffle tree per wave and the four wave sums are added in
// ascending order - the tree of the pmc_ncg kernels.
#include "handles.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>

#pragma clang fp contract(off)

namespace pmc {

namespace {

constexpr int kTracerThreads = 256;
constexpr double kSeries = 0x1p-20;   // |argument| below which L and E switch to their series

// per-element records; a face id carries the sign of the element's outward normal against the face's global normal:
// f when they agree, ~f when they are opposite
struct alignas(16) BoxRec {
    int32_t face[6], nbr[6];   // local order z-, y-, x+, y+, x-, z+; nbr -1 on the boundary
    double phi;
    double lo[3], hi[3];
    double pad;
};
struct alignas(16) TetRec {
    int32_t face[4], nbr[4];   // local face i is opposite vertex i
    double phi, vol;
    double row[4][4];          // lambda_i(x) = row[i][0..2] . x + row[i][3]
    double edge[3][3];         // V_j - V_3, j = 0, 1, 2
    double v3[3];              // vertex 3: the position is formed relative to it (see walk)
};
static_assert(sizeof(BoxRec) == 112 && sizeof(TetRec) == 272, "record layout");

__host__ __device__ inline int face_id(int32_t enc) { return enc < 0 ? ~enc : enc; }

__device__ __forceinline__ double tracer_L(double rho) {
    return fabs(rho) < kSeries ? (1.0 - rho / 2.0) + rho * rho / 3.0 : log1p(rho) / rho;
}
__device__ __forceinline__ double tracer_E(double z) {
    return fabs(z) < kSeries ? (1.0 + z / 2.0) + z * z / 6.0 : expm1(z) / z;
}
__device__ __forceinline__ double clampd(double c, double lo, double hi) { return fmin(fmax(c, lo), hi); }

// outward flux through a local face of the realization whose fluxes start at ub
__device__ __forceinline__ double face_flux(const double* __restrict__ ub, int64_t stride_face, int32_t enc) {
    const double v = ub[(int64_t)face_id(enc) * stride_face];
    return enc < 0 ? -v : v;
}

struct Pick {             // the earliest exit candidate so far (ties keep the earlier candidate)
    double dt;
    int which;            // box: axis; tet: local face; -1: none
    int32_t face, nbr;
    double bound;         // box: the plane's coordinate
};
__device__ __forceinline__ void pick(Pick& p, bool cand, double dt, int which, int32_t face, int32_t nbr, double bound) {
    if (cand && dt < p.dt) {
        p.dt = dt;
        p.which = which;
        p.face = face;
        p.nbr = nbr;
        p.bound = bound;
    }
}

// one axis of a box: velocity v at the particle, its gradient g, and the exit candidate of the axis
template <int A, int LO, int HI>
__device__ __forceinline__ void box_axis(const BoxRec& r, const double* __restrict__ ub, int64_t stride_face, double vol,
                                         double x, double& v, double& g, Pick& p) {
    const double lo = r.lo[A], hi = r.hi[A], h = hi - lo;
    const double area = vol / h;
    const double vlo = -face_flux(ub, stride_face, r.face[LO]) / area;
    const double vhi = face_flux(ub, stride_face, r.face[HI]) / area;
    g = (vhi - vlo) / h;
    v = vlo + g * (x - lo);
    const bool up = v > 0.0 && vhi > 0.0;
    const bool cand = up || (v < 0.0 && vlo < 0.0);
    const double d = up ? hi - x : lo - x;
    const double vex = up ? vhi : vlo;
    const double dt = (d / v) * tracer_L((vex - v) / v);
    pick(p, cand, dt, A, up ? r.face[HI] : r.face[LO], up ? r.nbr[HI] : r.nbr[LO], up ? hi : lo);
}

template <int A>
__device__ __forceinline__ double box_advance(const BoxRec& r, const Pick& p, double x, double v, double g) {
    const double c = clampd(x + (v * p.dt) * tracer_E(g * p.dt), r.lo[A], r.hi[A]);
    return p.which == A ? p.bound : c;
}

struct Path {
    double T, x, y, z;
    int32_t exit_face, status, nsteps;
};

// What a walk leaves behind for the adjoint sweep.  The plain walk keeps nothing: its policy is empty
// and the kernel of pmc_tracer_run compiles to the code it had before the policy existed.
struct NoHist {
    __device__ __forceinline__ void box_step(int, int, const BoxRec&, const Path&, const Pick&) {}
    __device__ __forceinline__ void tet_step(int, int, double, double, double, double, const Pick&) {}
    __device__ __forceinline__ void tet_enter(const TetRec&, int) {}
};

template <class Hist>
__device__ __forceinline__ void walk(const BoxRec* __restrict__ recs, const double* __restrict__ ub, int64_t stride_face,
                                     int max_steps, int e, Path& o, Hist& hist) {
    {
        const BoxRec& r = recs[e];
        o.x = clampd(o.x, r.lo[0], r.hi[0]);
        o.y = clampd(o.y, r.lo[1], r.hi[1]);
        o.z = clampd(o.z, r.lo[2], r.hi[2]);
    }
    for (int s = 0; s < max_steps; ++s) {
        const BoxRec& r = recs[e];
        const double vol = ((r.hi[0] - r.lo[0]) * (r.hi[1] - r.lo[1])) * (r.hi[2] - r.lo[2]);
        Pick p{INFINITY, -1, -1, -1, 0.0};
        double vx, gx, vy, gy, vz, gz;
        box_axis<0, 4, 2>(r, ub, stride_face, vol, o.x, vx, gx, p);
        box_axis<1, 1, 3>(r, ub, stride_face, vol, o.y, vy, gy, p);
        box_axis<2, 0, 5>(r, ub, stride_face, vol, o.z, vz, gz, p);
        if (p.which < 0) {
            o.status = PMC_TRACER_STAGNANT;
            break;
        }
        hist.box_step(s, e, r, o, p);
        o.T += r.phi * p.dt;
        o.nsteps += 1;
        o.x = box_advance<0>(r, p, o.x, vx, gx);
        o.y = box_advance<1>(r, p, o.y, vy, gy);
        o.z = box_advance<2>(r, p, o.z, vz, gz);
        if (p.nbr < 0) {
            o.status = PMC_TRACER_EXITED;
            o.exit_face = face_id(p.face);
            break;
        }
        e = p.nbr;
    }
}

template <int I>
__device__ __forceinline__ double tet_lambda(const TetRec& r, double x, double y, double z) {
    return clampd(((r.row[I][0] * x + r.row[I][1] * y) + r.row[I][2] * z) + r.row[I][3], 0.0, 1.0);
}
template <int I>
__device__ __forceinline__ void tet_face(const TetRec& r, double F, double w, double v, double lam, Pick& p) {
    const bool cand = F > 0.0 && v < 0.0;
    const double dt = (-lam / v) * tracer_L((-w - v) / v);
    pick(p, cand, dt, I, r.face[I], r.nbr[I], 0.0);
}
template <int I>
__device__ __forceinline__ double tet_advance(const Pick& p, double lam, double v, double eb) {
    const double c = clampd(lam + (v * p.dt) * eb, 0.0, 1.0);
    return p.which == I ? 0.0 : c;
}

template <class Hist>
__device__ __forceinline__ void walk(const TetRec* __restrict__ recs, const double* __restrict__ ub, int64_t stride_face,
                                     int max_steps, int e, Path& o, Hist& hist) {
    double l0, l1, l2, l3;
    {
        const TetRec& r = recs[e];
        l0 = tet_lambda<0>(r, o.x, o.y, o.z);
        l1 = tet_lambda<1>(r, o.x, o.y, o.z);
        l2 = tet_lambda<2>(r, o.x, o.y, o.z);
        l3 = tet_lambda<3>(r, o.x, o.y, o.z);
    }
    for (int s = 0; s < max_steps; ++s) {
        const TetRec& r = recs[e];
        const double F0 = face_flux(ub, stride_face, r.face[0]), F1 = face_flux(ub, stride_face, r.face[1]);
        const double F2 = face_flux(ub, stride_face, r.face[2]), F3 = face_flux(ub, stride_face, r.face[3]);
        const double c3 = 3.0 * r.vol;
        const double b = (((F0 + F1) + F2) + F3) / c3;
        const double w0 = F0 / c3, w1 = F1 / c3, w2 = F2 / c3, w3 = F3 / c3;
        const double v0 = b * l0 - w0, v1 = b * l1 - w1, v2 = b * l2 - w2, v3 = b * l3 - w3;
        Pick p{INFINITY, -1, -1, -1, 0.0};
        tet_face<0>(r, F0, w0, v0, l0, p);
        tet_face<1>(r, F1, w1, v1, l1, p);
        tet_face<2>(r, F2, w2, v2, l2, p);
        tet_face<3>(r, F3, w3, v3, l3, p);
        if (p.which < 0) {
            o.status = PMC_TRACER_STAGNANT;
            break;
        }
        hist.tet_step(s, e, l0, l1, l2, l3, p);
        o.T += r.phi * p.dt;
        o.nsteps += 1;
        const double eb = tracer_E(b * p.dt);
        l0 = tet_advance<0>(p, l0, v0, eb);
        l1 = tet_advance<1>(p, l1, v1, eb);
        l2 = tet_advance<2>(p, l2, v2, eb);
        l3 = tet_advance<3>(p, l3, v3, eb);
        // the position relative to vertex 3: a coordinate that was set to zero or clamped (sum lambda != 1 by eta) moves it
        // by eta x an edge.  Formed as sum lambda_j V_j it would move by eta x |V_j|, an error that grows by |V| / h per
        // element and throws the particle out of the mesh within a dozen steps.
        o.x = r.v3[0] + ((l0 * r.edge[0][0] + l1 * r.edge[1][0]) + l2 * r.edge[2][0]);
        o.y = r.v3[1] + ((l0 * r.edge[0][1] + l1 * r.edge[1][1]) + l2 * r.edge[2][1]);
        o.z = r.v3[2] + ((l0 * r.edge[0][2] + l1 * r.edge[1][2]) + l2 * r.edge[2][2]);
        if (p.nbr < 0) {
            o.status = PMC_TRACER_EXITED;
            o.exit_face = face_id(p.face);
            break;
        }
        e = p.nbr;
        const TetRec& q = recs[e];
        const int f = face_id(p.face);
        hist.tet_enter(q, f);
        // barycentric coordinates in the neighbour; the entry face's is zero exactly
        l0 = face_id(q.face[0]) == f ? 0.0 : tet_lambda<0>(q, o.x, o.y, o.z);
        l1 = face_id(q.face[1]) == f ? 0.0 : tet_lambda<1>(q, o.x, o.y, o.z);
        l2 = face_id(q.face[2]) == f ? 0.0 : tet_lambda<2>(q, o.x, o.y, o.z);
        l3 = face_id(q.face[3]) == f ? 0.0 : tet_lambda<3>(q, o.x, o.y, o.z);
    }
}

// by_batch == 0: thread = particle blockIdx.x * 256 + threadIdx.x of realization batch0 + blockIdx.y;
// by_batch != 0: consecutive threads are consecutive realizations of one particle
template <class Rec>
__global__ __launch_bounds__(kTracerThreads) void tracer_walk_kernel(
    const Rec* __restrict__ recs, int npart, int nb, int by_batch, const double* __restrict__ x0,
    const int32_t* __restrict__ e0, const int32_t* __restrict__ orig, int max_steps, const double* __restrict__ u,
    int64_t stride_face, int64_t stride_batch, double* __restrict__ T, int32_t* __restrict__ exit_face,
    int32_t* __restrict__ status, int32_t* __restrict__ nsteps, double* __restrict__ x_exit) {
    const int64_t gid = (int64_t)blockIdx.x * kTracerThreads + threadIdx.x;
    const int64_t part = by_batch ? gid / nb : gid;
    const int b = by_batch ? (int)(gid % nb) : (int)blockIdx.y;
    if (part >= npart) return;
    const int p = (int)part;
    Path o{0.0, x0[3 * p], x0[3 * p + 1], x0[3 * p + 2], -1, PMC_TRACER_MAX_STEPS, 0};
    NoHist none;
    walk(recs, u + (int64_t)b * stride_batch, stride_face, max_steps, e0[p], o, none);
    const int64_t at = (int64_t)b * npart + orig[p];
    T[at] = o.T;
    exit_face[at] = o.exit_face;
    status[at] = o.status;
    nsteps[at] = o.nsteps;
    if (x_exit) {
        x_exit[3 * at] = o.x;
        x_exit[3 * at + 1] = o.y;
        x_exit[3 * at + 2] = o.z;
    }
}

__global__ __launch_bounds__(kTracerThreads) void tracer_reduce_kernel(int npart, const double* __restrict__ T,
                                                                       const int32_t* __restrict__ status, int kind,
                                                                       double* __restrict__ Q, int32_t* __restrict__ not_exited) {
    __shared__ double wsum[kTracerThreads / 64], wmin[kTracerThreads / 64];
    __shared__ int wcnt[kTracerThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * npart;
    double acc = 0.0, mn = INFINITY;
    int cnt = 0;
    for (int i = threadIdx.x; i < npart; i += kTracerThreads) {
        const double t = T[base + i];
        acc += t;
        mn = fmin(mn, t);
        cnt += status[base + i] != PMC_TRACER_EXITED;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        mn = fmin(mn, __shfl_xor(mn, off, 64));
        cnt += __shfl_xor(cnt, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = acc;
        wmin[threadIdx.x >> 6] = mn;
        wcnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0], m = wmin[0];
        int c = wcnt[0];
        for (int w = 1; w < kTracerThreads / 64; ++w) {
            s += wsum[w];
            m = fmin(m, wmin[w]);
            c += wcnt[w];
        }
        Q[blockIdx.x] = kind == PMC_TRACER_MEAN ? s / (double)npart : m;
        not_exited[blockIdx.x] = c;
    }
}

// ---- the adjoint (pmc_tracer_run_adjoint; twin: trace_adjoint) ------------------------------------
// Three kernels on records of their own.  A second forward walk keeps, per (step, thread), the element, the entry
// coordinates and the chosen exit; the sweep, one thread per (particle, column), goes through its steps last to first,
// carrying the adjoints of the time and of the position, and leaves the adjoint of the element's outward fluxes in the
// record; the assembly, one thread per (face, column), adds them in the fixed order of the contract.  Every array of the
// records is indexed s * N + tid (N threads of the launch), so a wave reads and writes contiguous runs.
//
// The visits of one (element, column) are found through a linked list: the sweep threads push their record index with an
// integer exchange on the list's head.  The order of the links is arbitrary and never reaches a sum: the assembly picks
// the visits in ascending (particle in the caller's order, step), kAsmKeys of them per traversal of the list.
constexpr double kDSeries = 0x1p-3;   // |argument| below which L' and E' are summed as series
constexpr int kLpTerms = 19, kEpTerms = 11;
constexpr int kAsmKeys = 32;

constexpr double factorial(int n) { return n <= 1 ? 1.0 : (double)n * factorial(n - 1); }

// The series' coefficients, highest power last: L'(rho) = sum_k (-1)^k k rho^(k - 1) / (k + 1), E'(z) = sum_k k z^(k - 1) /
// (k + 1)!.  Tables in constant memory and rolled Horner loops: unrolled, the 30 constants are hoisted out of the step loop
// into scalar registers and the sweep spills them.
struct SeriesTables {
    double lp[kLpTerms], ep[kEpTerms];
};
constexpr SeriesTables make_series() {
    SeriesTables t{};
    for (int k = 1; k <= kLpTerms; ++k) t.lp[k - 1] = (double)((k & 1) ? -k : k) / (double)(k + 1);
    for (int k = 1; k <= kEpTerms; ++k) t.ep[k - 1] = (double)k / factorial(k + 1);
    return t;
}
__constant__ SeriesTables kSeriesTab = make_series();

__device__ __forceinline__ double tracer_Lp_series(double rho) {
    double acc = kSeriesTab.lp[kLpTerms - 1];
#pragma unroll 1
    for (int k = kLpTerms - 2; k >= 0; --k) acc = kSeriesTab.lp[k] + rho * acc;
    return acc;
}
__device__ __forceinline__ double tracer_Ep_series(double z) {
    double acc = kSeriesTab.ep[kEpTerms - 1];
#pragma unroll 1
    for (int k = kEpTerms - 2; k >= 0; --k) acc = kSeriesTab.ep[k] + z * acc;
    return acc;
}

struct HistView {
    int64_t N, SN;        // threads of the launch; S * N
    int S;                // steps a record holds: the largest step count of the launch
    int32_t* elem;
    int32_t* code;        // box: axis | up << 2; tet: local exit face | (1 + local entry face, 0 at the start) << 2
    double* c;            // entry coordinates, c[k * SN + s * N + tid]: x, y, z of a box, lambda_0..3 of a tetrahedron
};

struct KeepHist {
    HistView h;
    int64_t tid;
    int entry;
    __device__ __forceinline__ void box_step(int s, int e, const BoxRec& r, const Path& o, const Pick& p) {
        if (s >= h.S) return;
        const int64_t i = (int64_t)s * h.N + tid;
        const double hi = p.which == 0 ? r.hi[0] : p.which == 1 ? r.hi[1] : r.hi[2];
        h.elem[i] = e;
        h.code[i] = p.which | (p.bound == hi ? 4 : 0);
        h.c[i] = o.x;
        h.c[h.SN + i] = o.y;
        h.c[2 * h.SN + i] = o.z;
    }
    __device__ __forceinline__ void tet_step(int s, int e, double l0, double l1, double l2, double l3, const Pick& p) {
        if (s >= h.S) return;
        const int64_t i = (int64_t)s * h.N + tid;
        h.elem[i] = e;
        h.code[i] = p.which | (entry << 2);
        h.c[i] = l0;
        h.c[h.SN + i] = l1;
        h.c[2 * h.SN + i] = l2;
        h.c[3 * h.SN + i] = l3;
    }
    __device__ __forceinline__ void tet_enter(const TetRec& q, int f) {
        entry = face_id(q.face[0]) == f ? 1 : face_id(q.face[1]) == f ? 2 : face_id(q.face[2]) == f ? 3 : 4;
    }
};

// thread -> (particle in sorted order, column of the launch, record slot), the mapping of tracer_walk_kernel
__device__ __forceinline__ bool adjoint_thread(int npart, int nb, int by_batch, int& p, int& b, int64_t& tid) {
    const int64_t gid = (int64_t)blockIdx.x * kTracerThreads + threadIdx.x;
    const int64_t part = by_batch ? gid / nb : gid;
    b = by_batch ? (int)(gid % nb) : (int)blockIdx.y;
    if (part >= npart) return false;
    p = (int)part;
    tid = by_batch ? gid : (int64_t)b * npart + part;
    return true;
}

template <class Rec>
__global__ __launch_bounds__(kTracerThreads) void tracer_history_kernel(
    const Rec* __restrict__ recs, int npart, int nb, int by_batch, const double* __restrict__ x0,
    const int32_t* __restrict__ e0, int max_steps, const double* __restrict__ u, int64_t stride_face, int64_t stride_batch,
    HistView h) {
    int p, b;
    int64_t tid;
    if (!adjoint_thread(npart, nb, by_batch, p, b, tid)) return;
    Path o{0.0, x0[3 * p], x0[3 * p + 1], x0[3 * p + 2], -1, PMC_TRACER_MAX_STEPS, 0};
    KeepHist keep{h, tid, 0};
    walk(recs, u + (int64_t)b * stride_batch, stride_face, max_steps, e0[p], o, keep);
}

struct BoxAxis {
    double lo, h, area, vlo, vhi, g, v, x;
};
template <int A, int LO, int HI>
__device__ __forceinline__ BoxAxis box_axis_values(const BoxRec& r, const double* __restrict__ ub, int64_t stride_face,
                                                   double vol, double x) {
    BoxAxis a;
    a.lo = r.lo[A];
    a.h = r.hi[A] - a.lo;
    a.area = vol / a.h;
    a.vlo = -face_flux(ub, stride_face, r.face[LO]) / a.area;
    a.vhi = face_flux(ub, stride_face, r.face[HI]) / a.area;
    a.g = (a.vhi - a.vlo) / a.h;
    a.v = a.vlo + a.g * (x - a.lo);
    a.x = x;
    return a;
}
// E(z) and E'(z) = (e^z - E) / z from one expm1; L(rho) and L'(rho) = (1 / (1 + rho) - L) / rho from one log1p
__device__ __forceinline__ void tracer_E_both(double z, double& E, double& Ep) {
    const double az = fabs(z);
    const double em = expm1(z);
    E = az < kSeries ? (1.0 + z / 2.0) + z * z / 6.0 : em / z;
    Ep = az < kDSeries ? tracer_Ep_series(z) : ((em + 1.0) - em / z) / z;
}
__device__ __forceinline__ void tracer_L_both(double rho, double& L, double& Lp) {
    const double ar = fabs(rho);
    const double lg = log1p(rho);
    L = ar < kSeries ? (1.0 - rho / 2.0) + rho * rho / 3.0 : lg / rho;
    Lp = ar < kDSeries ? tracer_Lp_series(rho) : (1.0 / (1.0 + rho) - lg / rho) / rho;
}

// a coordinate that is not the exit's: c = x + (v dt) E(g dt)
__device__ __forceinline__ void box_axis_back(double g, double v, double cb, double dt, double& dtb, double& vb, double& gb) {
    const double z = g * dt;
    double E, Ep;
    tracer_E_both(z, E, Ep);
    const double mb = cb * E;
    const double zb = (cb * (v * dt)) * Ep;
    vb = mb * dt;
    gb = zb * dt;
    dtb = dtb + mb * v;
    dtb = dtb + zb * g;
}
__device__ __forceinline__ void box_axis_flux(const BoxAxis& a, bool is_exit, bool up, double vexb, double vb, double gb,
                                              double& xin, double& fb_lo, double& fb_hi) {
    const double gba = gb + vb * (a.x - a.lo);
    xin = xin + vb * a.g;
    double vlob = vb - gba / a.h;
    double vhib = gba / a.h;
    if (is_exit) {
        if (up) vhib = vhib + vexb;
        else vlob = vlob + vexb;
    }
    fb_lo = -vlob / a.area;
    fb_hi = vhib / a.area;
}

// One step backwards (twin: _step_adjoint): xb0..2 holds the adjoint of the position after the step and receives that of
// the position at its entry; the adjoints of the outward fluxes go to fb[l * SN]
__device__ __forceinline__ void sweep_step(const BoxRec& r, const double* __restrict__ ub, int64_t stride_face,
                                           const double* __restrict__ c, int64_t SN, int code, double Tbar, double& xb0,
                                           double& xb1, double& xb2, double* __restrict__ fb) {
    const double vol = ((r.hi[0] - r.lo[0]) * (r.hi[1] - r.lo[1])) * (r.hi[2] - r.lo[2]);
    const BoxAxis a0 = box_axis_values<0, 4, 2>(r, ub, stride_face, vol, c[0]);
    const BoxAxis a1 = box_axis_values<1, 1, 3>(r, ub, stride_face, vol, c[SN]);
    const BoxAxis a2 = box_axis_values<2, 0, 5>(r, ub, stride_face, vol, c[2 * SN]);
    const int A = code & 3;
    const bool up = (code & 4) != 0;
#define PMC_SEL(m) (A == 0 ? a0.m : A == 1 ? a1.m : a2.m)
    const double vA = PMC_SEL(v), xA = PMC_SEL(x), loA = PMC_SEL(lo);
    const double vex = up ? PMC_SEL(vhi) : PMC_SEL(vlo);
#undef PMC_SEL
    const double hiA = A == 0 ? r.hi[0] : A == 1 ? r.hi[1] : r.hi[2];
    const double dist = up ? hiA - xA : loA - xA;
    const double q = dist / vA;
    const double rho = (vex - vA) / vA;
    double Lr, Lpr;
    tracer_L_both(rho, Lr, Lpr);
    const double dt = q * Lr;
    double dtb = r.phi * Tbar;
    // the two coordinates that are not the exit's, in ascending order
    const bool pf = A == 0, qf = A == 2;             // the first is axis 1 instead of 0; the second is axis 1 instead of 2
    double vbp, gbp, vbq, gbq;
    box_axis_back(pf ? a1.g : a0.g, pf ? a1.v : a0.v, pf ? xb1 : xb0, dt, dtb, vbp, gbp);
    box_axis_back(qf ? a1.g : a2.g, qf ? a1.v : a2.v, qf ? xb1 : xb2, dt, dtb, vbq, gbq);
    const double qb = dtb * Lr;
    const double rb = (dtb * q) * Lpr;
    const double vexb = rb / vA;
    const double vbA = -(qb * q) / vA - (rb * (1.0 + rho)) / vA;
    const double xinA = -(qb / vA);
    double xin0 = A == 0 ? xinA : xb0, xin1 = A == 1 ? xinA : xb1, xin2 = A == 2 ? xinA : xb2;
    const double vb0 = A == 0 ? vbA : vbp, vb1 = A == 1 ? vbA : A == 0 ? vbp : vbq, vb2 = A == 2 ? vbA : vbq;
    const double gb0 = A == 0 ? 0.0 : gbp, gb1 = A == 1 ? 0.0 : A == 0 ? gbp : gbq, gb2 = A == 2 ? 0.0 : gbq;
    double f0, f1, f2, f3, f4, f5;
    box_axis_flux(a0, A == 0, up, vexb, vb0, gb0, xin0, f4, f2);
    box_axis_flux(a1, A == 1, up, vexb, vb1, gb1, xin1, f1, f3);
    box_axis_flux(a2, A == 2, up, vexb, vb2, gb2, xin2, f0, f5);
    fb[0] = f0;
    fb[SN] = f1;
    fb[2 * SN] = f2;
    fb[3 * SN] = f3;
    fb[4 * SN] = f4;
    fb[5 * SN] = f5;
    xb0 = xin0;
    xb1 = xin1;
    xb2 = xin2;
}

__device__ __forceinline__ void sweep_step(const TetRec& r, const double* __restrict__ ub, int64_t stride_face,
                                           const double* __restrict__ c, int64_t SN, int code, double Tbar, double& xb0,
                                           double& xb1, double& xb2, double* __restrict__ fb) {
    const int A = code & 3, entry = (code >> 2) - 1;
    double F[4], lam[4], w[4], v[4], lnb[4], lamb[4], vb[4], wb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        F[i] = face_flux(ub, stride_face, r.face[i]);
        lam[i] = c[i * SN];
    }
    const double c3 = 3.0 * r.vol;
    const double b = (((F[0] + F[1]) + F[2]) + F[3]) / c3;
    double lamA = 0.0, vA = 0.0, wA = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = F[i] / c3;
        v[i] = b * lam[i] - w[i];
        if (i == A) {
            lamA = lam[i];
            vA = v[i];
            wA = w[i];
        }
    }
    const double q = -lamA / vA;
    const double rho = (-wA - vA) / vA;
    double Lr, Lpr, eb, ebp;
    tracer_L_both(rho, Lr, Lpr);
    const double dt = q * Lr;
    const double z = b * dt;
    tracer_E_both(z, eb, ebp);
#pragma unroll
    for (int j = 0; j < 3; ++j) lnb[j] = (r.edge[j][0] * xb0 + r.edge[j][1] * xb1) + r.edge[j][2] * xb2;
    lnb[3] = 0.0;
    double dtb = r.phi * Tbar, ebb = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i == A) lnb[i] = 0.0;
        const double mb = lnb[i] * eb;
        ebb = ebb + lnb[i] * (v[i] * dt);
        lamb[i] = lnb[i];
        vb[i] = mb * dt;
        wb[i] = 0.0;
        dtb = dtb + mb * v[i];
    }
    const double zb = ebb * ebp;
    double bb = zb * dt;
    dtb = dtb + zb * b;
    const double qb = dtb * Lr;
    const double rb = (dtb * q) * Lpr;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i == A) {
            lamb[i] = lamb[i] - qb / vA;
            vb[i] = (vb[i] - (qb * q) / vA) - (rb * (1.0 + rho)) / vA;
            wb[i] = -(rb / vA);
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bb = bb + vb[i] * lam[i];
        lamb[i] = lamb[i] + vb[i] * b;
        wb[i] = wb[i] - vb[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        fb[i * SN] = (wb[i] + bb) / c3;
        if (i == entry) lamb[i] = 0.0;                 // the entry face's coordinate was set, not computed
    }
    xb0 = ((r.row[0][0] * lamb[0] + r.row[1][0] * lamb[1]) + r.row[2][0] * lamb[2]) + r.row[3][0] * lamb[3];
    xb1 = ((r.row[0][1] * lamb[0] + r.row[1][1] * lamb[1]) + r.row[2][1] * lamb[2]) + r.row[3][1] * lamb[3];
    xb2 = ((r.row[0][2] * lamb[0] + r.row[1][2] * lamb[1]) + r.row[2][2] * lamb[2]) + r.row[3][2] * lamb[3];
}

// link[i] = (the record pushed before i on the list of its (element, column), the particle's index in the caller's order)
template <class Rec>
__global__ __launch_bounds__(kTracerThreads) void tracer_sweep_kernel(
    const Rec* __restrict__ recs, int npart, int nb, int by_batch, const int32_t* __restrict__ orig,
    const double* __restrict__ u, int64_t stride_face, int64_t stride_batch, HistView h, const int32_t* __restrict__ status,
    const int32_t* __restrict__ nsteps, const double* __restrict__ T_bar, const double* __restrict__ xe_bar,
    double* __restrict__ fbar, int2* __restrict__ link, int32_t* __restrict__ head, double* __restrict__ x0_bar) {
    int p, b;
    int64_t tid;
    if (!adjoint_thread(npart, nb, by_batch, p, b, tid)) return;
    const int32_t op = orig[p];
    const int64_t at = (int64_t)b * npart + op;
    double xb0 = 0.0, xb1 = 0.0, xb2 = 0.0;
    if (status[at] == PMC_TRACER_EXITED) {
        const double Tb = T_bar ? T_bar[at] : 0.0;
        if (xe_bar) {
            xb0 = xe_bar[3 * at];
            xb1 = xe_bar[3 * at + 1];
            xb2 = xe_bar[3 * at + 2];
        }
        const double* ub = u + (int64_t)b * stride_batch;
        const int ns = min(nsteps[at], h.S);
        for (int s = ns - 1; s >= 0; --s) {
            const int64_t i = (int64_t)s * h.N + tid;
            const int e = h.elem[i];
            sweep_step(recs[e], ub, stride_face, h.c + i, h.SN, h.code[i], Tb, xb0, xb1, xb2, fbar + i);
            const int prev = atomicExch(&head[(int64_t)e * nb + b], (int)i);
            link[i] = make_int2(prev, op);
        }
    }
    if (x0_bar) {
        x0_bar[3 * at] = xb0;
        x0_bar[3 * at + 1] = xb1;
        x0_bar[3 * at + 2] = xb2;
    }
}

// u_bar of one (face, column): from 0.0, over the (at most two) elements of the face in the order of face_elem, within an
// element over its visits in ascending (particle in the caller's order, step).  side[2 f + k] = element << 4 | local face
// << 1 | (outward normal against the global one), -1 for no element.  A key is particle << 32 | record index: for one
// particle of one column the record index ascends with the step.
__global__ __launch_bounds__(kTracerThreads) void tracer_assemble_kernel(
    int n_face, int nb, int by_batch, const int32_t* __restrict__ side, const int32_t* __restrict__ head,
    const int2* __restrict__ link, const double* __restrict__ fbar, int64_t SN, double* __restrict__ u_bar,
    int64_t stride_face, int64_t stride_batch) {
    const int64_t gid = (int64_t)blockIdx.x * kTracerThreads + threadIdx.x;
    const int64_t f = by_batch ? gid / nb : gid;
    const int b = by_batch ? (int)(gid % nb) : (int)blockIdx.y;
    if (f >= n_face) return;
    constexpr int64_t kNone = INT64_MAX;
    double acc = 0.0;
    for (int k = 0; k < 2; ++k) {
        const int32_t enc = side[2 * f + k];
        if (enc < 0) continue;
        const int hd = head[(int64_t)(enc >> 4) * nb + b];
        if (hd < 0) continue;
        const double* fb = fbar + (int64_t)((enc >> 1) & 7) * SN;
        const bool neg = (enc & 1) != 0;
        int64_t last = -1;
        for (;;) {
            int64_t key[kAsmKeys];
#pragma unroll
            for (int j = 0; j < kAsmKeys; ++j) key[j] = kNone;
            for (int n = hd; n >= 0;) {
                const int2 l = link[n];
                int64_t cand = ((int64_t)l.y << 32) | (int64_t)n;
                n = l.x;
                if (cand <= last || cand >= key[kAsmKeys - 1]) continue;
#pragma unroll
                for (int j = 0; j < kAsmKeys; ++j)       // insert into the ascending keys
                    if (cand < key[j]) {
                        const int64_t t = key[j];
                        key[j] = cand;
                        cand = t;
                    }
            }
#pragma unroll
            for (int j = 0; j < kAsmKeys; ++j)
                if (key[j] != kNone) {
                    const double v = fb[key[j] & 0x7fffffff];
                    acc = acc + (neg ? -v : v);
                    last = key[j];
                }
            if (key[kAsmKeys - 1] == kNone) break;
        }
    }
    u_bar[f * stride_face + (int64_t)b * stride_batch] = acc;
}

// T_bar of the QoI of tracer_reduce_kernel: MEAN 1 / npart on the particles that exited; MIN 1 on the lowest-index particle
// attaining the minimum, if it exited.  One workgroup per column.
__global__ __launch_bounds__(kTracerThreads) void tracer_seed_kernel(int npart, const double* __restrict__ T,
                                                                     const int32_t* __restrict__ status, int kind,
                                                                     double* __restrict__ T_bar) {
    __shared__ double wmin[kTracerThreads / 64];
    __shared__ int widx[kTracerThreads / 64];
    __shared__ int arg;
    const int64_t base = (int64_t)blockIdx.x * npart;
    if (kind == PMC_TRACER_MIN) {
        double mn = INFINITY;
        int at = INT_MAX;
        for (int i = threadIdx.x; i < npart; i += kTracerThreads) {
            const double t = T[base + i];
            if (t < mn) {
                mn = t;
                at = i;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double om = __shfl_xor(mn, off, 64);
            const int oa = __shfl_xor(at, off, 64);
            if (om < mn || (om == mn && oa < at)) {
                mn = om;
                at = oa;
            }
        }
        if ((threadIdx.x & 63) == 0) {
            wmin[threadIdx.x >> 6] = mn;
            widx[threadIdx.x >> 6] = at;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kTracerThreads / 64; ++w)
                if (wmin[w] < mn || (wmin[w] == mn && widx[w] < at)) {
                    mn = wmin[w];
                    at = widx[w];
                }
            arg = at;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < npart; i += kTracerThreads) {
        const bool ok = status[base + i] == PMC_TRACER_EXITED;
        T_bar[base + i] = !ok ? 0.0 : kind == PMC_TRACER_MEAN ? 1.0 / (double)npart : i == arg ? 1.0 : 0.0;
    }
}

// T_bar = -(T - data) / noise (the seed of the travel-time log-likelihood); zero on a column that has a censored particle
__global__ void tracer_loglik_seed_kernel(int64_t total, int npart, const double* __restrict__ T, const double* __restrict__ data,
                                          const int32_t* __restrict__ not_exited, double noise, double* __restrict__ T_bar) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) T_bar[i] = not_exited[i / npart] > 0 ? 0.0 : -(T[i] - data[i % npart]) / noise;
}

// ---- host: setup ------------------------------------------------------------------------------------------------------
struct V3 {
    double x, y, z;
};
inline V3 sub(const double* a, const double* b) { return V3{a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
constexpr int kTetFace[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};   // vertices of local face i, outward normal
constexpr int kBoxLo[3] = {4, 1, 0}, kBoxHi[3] = {2, 3, 5};

}  // namespace

int Tracer::default_max_steps(int n_elem) {
    int c = 0;
    while ((int64_t)c * c * c < n_elem) ++c;
    return 64 + 32 * c;
}

Tracer::Tracer(Ctx& c, const pmc_tracer_mesh& m, int nparticles, const double* x0_in, const int32_t* elem0, int max_steps_in)
    : ctx(c), kind(m.kind), n_elem(m.n_elem), n_face(m.n_face), npart(nparticles) {
    PMC_REQUIRE(kind == PMC_TRACER_BOX || kind == PMC_TRACER_SIMPLEX, "pmc_tracer_create: kind must be PMC_TRACER_BOX or _SIMPLEX");
    PMC_REQUIRE(n_elem >= 1 && n_face >= 1, "pmc_tracer_create: empty mesh");
    PMC_REQUIRE(m.elem_face && m.elem_sign && m.face_elem && m.geom && x0_in && elem0, "pmc_tracer_create: NULL array");
    PMC_REQUIRE(nparticles >= 1, "pmc_tracer_create: nparticles must be at least 1");
    PMC_REQUIRE(max_steps_in >= 0 && max_steps_in <= (1 << 22), "pmc_tracer_create: max_steps outside [0, 2^22]");
    max_steps = max_steps_in ? max_steps_in : default_max_steps(n_elem);
    const int nfe = kind == PMC_TRACER_BOX ? 6 : 4;
    if (m.porosity)
        for (int e = 0; e < n_elem; ++e) PMC_REQUIRE(m.porosity[e] > 0.0, "pmc_tracer_create: porosity must be positive");
    // the two tables must describe the same adjacency: every local face names a face that lists the element, the two
    // elements of an interior face see it with opposite signs, and every element a face lists names it back
    std::vector<int32_t> nbr((size_t)n_elem * nfe);
    std::vector<int> refs(n_face, 0), ssum(n_face, 0);
    for (int f = 0; f < n_face; ++f) {
        const int32_t a = m.face_elem[2 * (size_t)f], b = m.face_elem[2 * (size_t)f + 1];
        PMC_REQUIRE(a >= 0 && a < n_elem && b >= -1 && b < n_elem && a != b, "pmc_tracer_create: face_elem out of range");
    }
    for (int e = 0; e < n_elem; ++e)
        for (int l = 0; l < nfe; ++l) {
            const int32_t f = m.elem_face[(size_t)e * nfe + l];
            const int sg = m.elem_sign[(size_t)e * nfe + l];
            PMC_REQUIRE(f >= 0 && f < n_face && (sg == 1 || sg == -1), "pmc_tracer_create: elem_face / elem_sign out of range");
            const int32_t a = m.face_elem[2 * (size_t)f], b = m.face_elem[2 * (size_t)f + 1];
            PMC_REQUIRE(a == e || b == e, "pmc_tracer_create: elem_face and face_elem disagree");
            nbr[(size_t)e * nfe + l] = a == e ? b : a;
            ++refs[f];
            ssum[f] += sg;
        }
    for (int f = 0; f < n_face; ++f) {
        const bool interior = m.face_elem[2 * (size_t)f + 1] >= 0;
        PMC_REQUIRE(refs[f] == (interior ? 2 : 1) && (!interior || ssum[f] == 0), "pmc_tracer_create: elem_face and face_elem disagree");
    }
    auto enc = [&](int e, int l) {
        const int32_t f = m.elem_face[(size_t)e * nfe + l];
        return m.elem_sign[(size_t)e * nfe + l] > 0 ? f : ~f;
    };
    std::vector<char> rec_h((size_t)n_elem * (kind == PMC_TRACER_BOX ? sizeof(BoxRec) : sizeof(TetRec)));
    if (kind == PMC_TRACER_BOX) {
        BoxRec* R = reinterpret_cast<BoxRec*>(rec_h.data());
        for (int e = 0; e < n_elem; ++e) {
            BoxRec& r = R[e];
            for (int l = 0; l < 6; ++l) {
                r.face[l] = enc(e, l);
                r.nbr[l] = nbr[(size_t)e * 6 + l];
            }
            r.phi = m.porosity ? m.porosity[e] : 1.0;
            r.pad = 0.0;
            for (int a = 0; a < 3; ++a) {
                r.lo[a] = m.geom[6 * (size_t)e + a];
                r.hi[a] = m.geom[6 * (size_t)e + 3 + a];
                PMC_REQUIRE(std::isfinite(r.lo[a]) && std::isfinite(r.hi[a]) && r.hi[a] > r.lo[a], "pmc_tracer_create: a box needs lo < hi");
            }
        }
        // axis-aligned conforming boxes: across local face l the neighbour meets this box with its opposite face, in the
        // same plane bit for bit and with the same cross-section
        for (int e = 0; e < n_elem; ++e)
            for (int a = 0; a < 3; ++a)
                for (int side = 0; side < 2; ++side) {
                    const int l = side ? kBoxHi[a] : kBoxLo[a], lo = side ? kBoxLo[a] : kBoxHi[a];
                    const int32_t q = R[e].nbr[l];
                    if (q < 0) continue;
                    bool ok = face_id(R[q].face[lo]) == face_id(R[e].face[l]) && (side ? R[e].hi[a] == R[q].lo[a] : R[e].lo[a] == R[q].hi[a]);
                    for (int o = 0; o < 3; ++o)
                        if (o != a) ok = ok && R[e].lo[o] == R[q].lo[o] && R[e].hi[o] == R[q].hi[o];
                    PMC_REQUIRE(ok, "pmc_tracer_create: the boxes are not axis-aligned and conforming in the local face order z-, y-, x+, y+, x-, z+");
                }
    } else {
        TetRec* R = reinterpret_cast<TetRec*>(rec_h.data());
        for (int e = 0; e < n_elem; ++e) {
            TetRec& r = R[e];
            const double* V = m.geom + 12 * (size_t)e;
            for (int l = 0; l < 4; ++l) {
                r.face[l] = enc(e, l);
                r.nbr[l] = nbr[(size_t)e * 4 + l];
                for (int d = 0; d < 3; ++d) {
                    PMC_REQUIRE(std::isfinite(V[3 * l + d]), "pmc_tracer_create: vertex coordinates must be finite");
                    if (l < 3) r.edge[l][d] = V[3 * l + d] - V[9 + d];
                    else r.v3[d] = V[9 + d];
                }
            }
            const double vol6 = dot3(cross(sub(V + 3, V), sub(V + 6, V)), sub(V + 9, V));
            PMC_REQUIRE(vol6 > 0.0, "pmc_tracer_create: a simplex of non-positive volume");
            r.phi = m.porosity ? m.porosity[e] : 1.0;
            r.vol = vol6 / 6.0;
            for (int i = 0; i < 4; ++i) {
                const double* A = V + 3 * kTetFace[i][0];
                const V3 n = cross(sub(V + 3 * kTetFace[i][1], A), sub(V + 3 * kTetFace[i][2], A));
                const V3 g{-n.x / vol6, -n.y / vol6, -n.z / vol6};
                r.row[i][0] = g.x;
                r.row[i][1] = g.y;
                r.row[i][2] = g.z;
                r.row[i][3] = -dot3(g, V3{A[0], A[1], A[2]});
            }
        }
    }
    // start points: inside their element up to 1e-12 of its extent
    for (int p = 0; p < npart; ++p) {
        const int32_t e = elem0[p];
        PMC_REQUIRE(e >= 0 && e < n_elem, "pmc_tracer_create: elem0 out of range");
        const double* x = x0_in + 3 * (size_t)p;
        PMC_REQUIRE(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]), "pmc_tracer_create: a start point is not finite");
        bool in = true;
        if (kind == PMC_TRACER_BOX) {
            const BoxRec& r = reinterpret_cast<const BoxRec*>(rec_h.data())[e];
            for (int a = 0; a < 3; ++a) {
                const double tol = 1e-12 * (r.hi[a] - r.lo[a]);
                in = in && x[a] >= r.lo[a] - tol && x[a] <= r.hi[a] + tol;
            }
        } else {
            const TetRec& r = reinterpret_cast<const TetRec*>(rec_h.data())[e];
            for (int i = 0; i < 4; ++i)
                in = in && ((r.row[i][0] * x[0] + r.row[i][1] * x[1]) + r.row[i][2] * x[2]) + r.row[i][3] >= -1e-12;
        }
        PMC_REQUIRE(in, "pmc_tracer_create: a start point lies outside its elem0");
    }
    // particles in the order of their start elements (stable); the outputs undo the sort
    std::vector<int32_t> order(npart);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return elem0[a] < elem0[b]; });
    std::vector<double> xs(3 * (size_t)npart);
    std::vector<int32_t> es(npart);
    for (int p = 0; p < npart; ++p) {
        es[p] = elem0[order[p]];
        for (int d = 0; d < 3; ++d) xs[3 * (size_t)p + d] = x0_in[3 * (size_t)order[p] + d];
    }
    // the adjoint's assembly: per face its (at most two) elements in the order of face_elem, with the local face and the sign
    std::vector<int32_t> side_h(2 * (size_t)n_face, -1);
    if (n_elem < (1 << 27))
        for (int f = 0; f < n_face; ++f)
            for (int k = 0; k < 2; ++k) {
                const int32_t e = m.face_elem[2 * (size_t)f + k];
                if (e < 0) continue;
                for (int l = 0; l < nfe; ++l)
                    if (m.elem_face[(size_t)e * nfe + l] == f)
                        side_h[2 * (size_t)f + k] = (e << 4) | (l << 1) | (m.elem_sign[(size_t)e * nfe + l] > 0 ? 0 : 1);
            }
    ctx.activate();
    hipStream_t st = ctx.stream;
    recs.upload(rec_h, st);
    x0.upload(xs, st);
    e0.upload(es, st);
    orig.upload(order, st);
    side.upload(side_h, st);
    PMC_HIP(hipStreamSynchronize(st));
}

void Tracer::launch_walk(hipStream_t st, int nb, bool by_batch, const double* u_d, int64_t stride_face, int64_t stride_batch,
                         double* T_d, int32_t* face_d, int32_t* status_d, int32_t* steps_d, double* x_d) {
    // blockIdx.y carries the realization of the sample-major layout: at most 32768 per launch
    const int per = by_batch ? nb : std::min(nb, 32768);
    if (per < nb) count_solve_path(PMC_COUNT_TRACER_SPLIT);
    for (int b0 = 0; b0 < nb; b0 += per) {
        const int n = std::min(per, nb - b0);
        const int64_t threads = by_batch ? (int64_t)npart * n : npart;
        const dim3 grid((unsigned)((threads + kTracerThreads - 1) / kTracerThreads), by_batch ? 1u : (unsigned)n);
        const int64_t o = (int64_t)b0 * npart;
        double* xo = x_d ? x_d + 3 * o : nullptr;
        if (kind == PMC_TRACER_BOX)
            tracer_walk_kernel<BoxRec><<<grid, kTracerThreads, 0, st>>>(
                reinterpret_cast<const BoxRec*>(recs.p), npart, n, by_batch ? 1 : 0, x0.p, e0.p, orig.p, max_steps,
                u_d + (int64_t)b0 * stride_batch, stride_face, stride_batch, T_d + o, face_d + o, status_d + o, steps_d + o, xo);
        else
            tracer_walk_kernel<TetRec><<<grid, kTracerThreads, 0, st>>>(
                reinterpret_cast<const TetRec*>(recs.p), npart, n, by_batch ? 1 : 0, x0.p, e0.p, orig.p, max_steps,
                u_d + (int64_t)b0 * stride_batch, stride_face, stride_batch, T_d + o, face_d + o, status_d + o, steps_d + o, xo);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
}

void Tracer::launch_reduce(hipStream_t st, int nb, const double* T_d, const int32_t* status_d, int qkind, double* q_d,
                           int32_t* nex_d) {
    tracer_reduce_kernel<<<(unsigned)nb, kTracerThreads, 0, st>>>(npart, T_d, status_d, qkind, q_d, nex_d);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
}

void Tracer::run(int nbatch, const double* u, int64_t ld, double* T, int32_t* exit_face, int32_t* status, int32_t* nsteps,
                 double* x_exit, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_tracer_run: nbatch must be at least 1");
    PMC_REQUIRE(u && T && exit_face && status && nsteps, "pmc_tracer_run: NULL array");
    PMC_REQUIRE(ld >= n_face, "pmc_tracer_run: ld is smaller than the number of faces");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_tracer_run: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    if (memspace == PMC_MEM_DEVICE) {
        launch_walk(st, nbatch, false, u, 1, ld, T, exit_face, status, nsteps, x_exit);
        PMC_HIP(hipStreamSynchronize(st));
        return;
    }
    // host memory: the flux rows are staged in pieces of at most 2^24 values
    const int per = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t(1) << 24) / n_face));
    const size_t cnt = (size_t)per * npart;
    if (per < nbatch) count_solve_path(PMC_COUNT_TRACER_SPLIT);
    stage_u.ensure((size_t)per * n_face);
    out_T.ensure(cnt);
    out_x.ensure(3 * cnt);
    out_i.ensure(3 * cnt);
    for (int b0 = 0; b0 < nbatch; b0 += per) {
        const int n = std::min(per, nbatch - b0);
        const size_t c = (size_t)n * npart, o = (size_t)b0 * npart;
        PMC_HIP(hipMemcpy2DAsync(stage_u.p, sizeof(double) * n_face, u + (size_t)b0 * ld, sizeof(double) * ld,
                                 sizeof(double) * n_face, n, hipMemcpyHostToDevice, st));
        launch_walk(st, n, false, stage_u.p, 1, n_face, out_T.p, out_i.p, out_i.p + cnt, out_i.p + 2 * cnt, x_exit ? out_x.p : nullptr);
        PMC_HIP(hipMemcpyAsync(T + o, out_T.p, sizeof(double) * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(exit_face + o, out_i.p, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(status + o, out_i.p + cnt, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(nsteps + o, out_i.p + 2 * cnt, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        if (x_exit) PMC_HIP(hipMemcpyAsync(x_exit + 3 * o, out_x.p, sizeof(double) * 3 * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

void Tracer::reduce(int nbatch, const double* T, const int32_t* status, int qkind, double* Q, int32_t* not_exited, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_tracer_reduce: nbatch must be at least 1");
    PMC_REQUIRE(T && status && Q, "pmc_tracer_reduce: NULL array");
    PMC_REQUIRE(qkind == PMC_TRACER_MEAN || qkind == PMC_TRACER_MIN, "pmc_tracer_reduce: kind must be PMC_TRACER_MEAN or _MIN");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_tracer_reduce: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t cnt = (size_t)nbatch * npart;
    const double* T_d = T;
    const int32_t* s_d = status;
    if (memspace == PMC_MEM_HOST) {
        red_T.ensure(cnt);
        red_s.ensure(cnt);
        PMC_HIP(hipMemcpyAsync(red_T.p, T, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        PMC_HIP(hipMemcpyAsync(red_s.p, status, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, st));
        T_d = red_T.p;
        s_d = red_s.p;
    }
    q.ensure(nbatch);
    nex.ensure(nbatch);
    launch_reduce(st, nbatch, T_d, s_d, qkind, q.p, nex.p);
    std::vector<int32_t> nx(nbatch);
    PMC_HIP(hipMemcpyAsync(Q, q.p, sizeof(double) * nbatch, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipMemcpyAsync(nx.data(), nex.p, sizeof(int32_t) * nbatch, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    if (not_exited) std::copy(nx.begin(), nx.end(), not_exited);
}

// the hook of Darcy::solve_chunk*: walk on the interleaved solution sol[row * nb + col] (its first n_face rows are the flux
// block) and reduce to q_d[0..nb) on the caller's stream
void Tracer::qoi_interleaved(hipStream_t st, int nb, const double* sol, int qkind, double* q_d) {
    const size_t cnt = (size_t)nb * npart;
    out_T.ensure(cnt);
    out_i.ensure(3 * cnt);
    nex.ensure(nb);
    launch_walk(st, nb, true, sol, nb, 1, out_T.p, out_i.p, out_i.p + cnt, out_i.p + 2 * cnt, nullptr);
    launch_reduce(st, nb, out_T.p, out_i.p + cnt, qkind, q_d, nex.p);
}

// ---- host: the adjoint --------------------------------------------------------------------------------------------------
void Tracer::set_adjoint_scratch(int64_t bytes) {
    PMC_REQUIRE(bytes >= 0, "pmc_tracer_set_adjoint_scratch: bytes must not be negative");
    adj_cap = bytes;
}

// One adjoint launch of nb columns on stream st: the plain walk (the forward outputs, pmc_tracer_run's), then per chunk of
// columns the walk with history, the sweep and the assembly.  A chunk is as many columns as keep the records of the largest
// step count under the cap (at least one).  Nothing a column receives depends on its chunk: a thread meets only its own
// records, and the assembly orders a list by (particle, step).  Synchronises st once, for the step counts.
void Tracer::adjoint_launch(hipStream_t st, int nb, bool by_batch, const double* u_d, int64_t stride_face, int64_t stride_batch,
                            const double* Tbar_d, const double* xbar_d, double* ubar_d, int64_t stride_face_out,
                            int64_t stride_batch_out, double* x0bar_d, double* T_d, int32_t* face_d, int32_t* status_d,
                            int32_t* steps_d, const double* data_d, double noise) {
    PMC_REQUIRE(n_elem < (1 << 27), "pmc_tracer_run_adjoint: more than 2^27 elements");
    launch_walk(st, nb, by_batch, u_d, stride_face, stride_batch, T_d, face_d, status_d, steps_d, nullptr);
    if (data_d) {
        // the seed of the log-likelihood, zero on a column with a particle that did not exit (nex: their count per column)
        q.ensure(nb);
        nex.ensure(nb);
        launch_reduce(st, nb, T_d, status_d, PMC_TRACER_MEAN, q.p, nex.p);
        Tbar_d = loglik_seed(st, nb, T_d, data_d, noise);
    }
    const size_t cnt = (size_t)nb * npart;
    h_steps.resize(cnt);
    PMC_HIP(hipMemcpyAsync(h_steps.data(), steps_d, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    const int S = std::max(1, *std::max_element(h_steps.begin(), h_steps.end()));
    const bool box = kind == PMC_TRACER_BOX;
    const int nc = box ? 3 : 4, nf = box ? 6 : 4;
    const size_t per_visit = 16 + 8 * (size_t)(nc + nf);          // element, code, link; coordinates and flux adjoints
    const size_t per_col = per_visit * (size_t)S * npart + sizeof(int32_t) * (size_t)n_elem;
    const size_t cap = adj_cap > 0 ? (size_t)adj_cap : (size_t)256 << 20;
    int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, cap / per_col));
    // record indices and the sample-major grid: 2^31 records and 32768 columns per chunk at the most
    while (per > 1 && (size_t)S * npart * per >= ((size_t)1 << 31)) per >>= 1;
    PMC_REQUIRE((size_t)S * npart * per < ((size_t)1 << 31), "pmc_tracer_run_adjoint: the records of one column pass 2^31");
    if (!by_batch) per = std::min(per, 32768);
    adj_chunks = (nb + per - 1) / per;
    const size_t SNmax = (size_t)S * npart * per;
    adj_elem.ensure(SNmax);
    adj_code.ensure(SNmax);
    adj_link.ensure(2 * SNmax);
    adj_c.ensure(nc * SNmax);
    adj_fbar.ensure(nf * SNmax);
    adj_head.ensure((size_t)n_elem * per);
    for (int b0 = 0; b0 < nb; b0 += per) {
        const int n = std::min(per, nb - b0);
        const int64_t N = (int64_t)npart * n, SN = N * S;
        const HistView h{N, SN, S, adj_elem.p, adj_code.p, adj_c.p};
        const int64_t o = (int64_t)b0 * npart;
        const double* ub = u_d + (int64_t)b0 * stride_batch;
        const dim3 grid((unsigned)(((by_batch ? N : (int64_t)npart) + kTracerThreads - 1) / kTracerThreads), by_batch ? 1u : (unsigned)n);
        const dim3 agrid((unsigned)(((by_batch ? (int64_t)n_face * n : (int64_t)n_face) + kTracerThreads - 1) / kTracerThreads),
                         by_batch ? 1u : (unsigned)n);
        PMC_HIP(hipMemsetAsync(adj_head.p, 0xff, sizeof(int32_t) * (size_t)n_elem * n, st));
        int2* link = reinterpret_cast<int2*>(adj_link.p);
        const double* tb = Tbar_d ? Tbar_d + o : nullptr;
        const double* xb = xbar_d ? xbar_d + 3 * o : nullptr;
        double* x0b = x0bar_d ? x0bar_d + 3 * o : nullptr;
        if (box) {
            const BoxRec* R = reinterpret_cast<const BoxRec*>(recs.p);
            tracer_history_kernel<BoxRec><<<grid, kTracerThreads, 0, st>>>(R, npart, n, by_batch ? 1 : 0, x0.p, e0.p, max_steps, ub,
                                                                           stride_face, stride_batch, h);
            tracer_sweep_kernel<BoxRec><<<grid, kTracerThreads, 0, st>>>(R, npart, n, by_batch ? 1 : 0, orig.p, ub, stride_face,
                                                                         stride_batch, h, status_d + o, steps_d + o, tb, xb,
                                                                         adj_fbar.p, link, adj_head.p, x0b);
        } else {
            const TetRec* R = reinterpret_cast<const TetRec*>(recs.p);
            tracer_history_kernel<TetRec><<<grid, kTracerThreads, 0, st>>>(R, npart, n, by_batch ? 1 : 0, x0.p, e0.p, max_steps, ub,
                                                                           stride_face, stride_batch, h);
            tracer_sweep_kernel<TetRec><<<grid, kTracerThreads, 0, st>>>(R, npart, n, by_batch ? 1 : 0, orig.p, ub, stride_face,
                                                                         stride_batch, h, status_d + o, steps_d + o, tb, xb,
                                                                         adj_fbar.p, link, adj_head.p, x0b);
        }
        tracer_assemble_kernel<<<agrid, kTracerThreads, 0, st>>>(n_face, n, by_batch ? 1 : 0, side.p, adj_head.p, link, adj_fbar.p, SN,
                                                                 ubar_d + (int64_t)b0 * stride_batch_out, stride_face_out,
                                                                 stride_batch_out);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(3);
    }
}

void Tracer::run_adjoint(int nbatch, const double* u, int64_t ld, const double* T_bar, const double* x_exit_bar, double* u_bar,
                         int64_t ld_bar, double* x0_bar, double* T, int32_t* exit_face, int32_t* status, int32_t* nsteps,
                         int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_tracer_run_adjoint: nbatch must be at least 1");
    PMC_REQUIRE(u && u_bar && status, "pmc_tracer_run_adjoint: NULL array");
    PMC_REQUIRE(T_bar || x_exit_bar, "pmc_tracer_run_adjoint: T_bar or x_exit_bar must be given");
    PMC_REQUIRE(ld >= n_face && ld_bar >= n_face, "pmc_tracer_run_adjoint: ld or ld_bar is smaller than the number of faces");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_tracer_run_adjoint: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const bool host = memspace == PMC_MEM_HOST;
    // pieces as in run: at most 2^24 staged flux values
    const int per = host ? (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t(1) << 24) / n_face)) : nbatch;
    const size_t cnt = (size_t)per * npart;
    adj_T.ensure(cnt);
    adj_i.ensure(3 * cnt);
    if (host) {
        adj_stage_u.ensure((size_t)per * n_face);
        adj_stage_ubar.ensure((size_t)per * n_face);
        if (T_bar) adj_stage_tb.ensure(cnt);
        if (x_exit_bar) adj_stage_xb.ensure(3 * cnt);
        if (x0_bar) adj_stage_x0b.ensure(3 * cnt);
    }
    for (int b0 = 0; b0 < nbatch; b0 += per) {
        const int n = std::min(per, nbatch - b0);
        const size_t c = (size_t)n * npart, o = (size_t)b0 * npart;
        // forward outputs the caller did not ask for go to scratch
        double* T_d = !host && T ? T + o : adj_T.p;
        int32_t* face_d = !host && exit_face ? exit_face + o : adj_i.p;
        int32_t* status_d = !host ? status + o : adj_i.p + cnt;
        int32_t* steps_d = !host && nsteps ? nsteps + o : adj_i.p + 2 * cnt;
        if (!host) {
            adjoint_launch(st, n, false, u + (size_t)b0 * ld, 1, ld, T_bar ? T_bar + o : nullptr, x_exit_bar ? x_exit_bar + 3 * o : nullptr,
                           u_bar + (size_t)b0 * ld_bar, 1, ld_bar, x0_bar ? x0_bar + 3 * o : nullptr, T_d, face_d, status_d, steps_d);
            PMC_HIP(hipStreamSynchronize(st));
            continue;
        }
        PMC_HIP(hipMemcpy2DAsync(adj_stage_u.p, sizeof(double) * n_face, u + (size_t)b0 * ld, sizeof(double) * ld,
                                 sizeof(double) * n_face, n, hipMemcpyHostToDevice, st));
        if (T_bar) PMC_HIP(hipMemcpyAsync(adj_stage_tb.p, T_bar + o, sizeof(double) * c, hipMemcpyHostToDevice, st));
        if (x_exit_bar) PMC_HIP(hipMemcpyAsync(adj_stage_xb.p, x_exit_bar + 3 * o, sizeof(double) * 3 * c, hipMemcpyHostToDevice, st));
        adjoint_launch(st, n, false, adj_stage_u.p, 1, n_face, T_bar ? adj_stage_tb.p : nullptr, x_exit_bar ? adj_stage_xb.p : nullptr,
                       adj_stage_ubar.p, 1, n_face, x0_bar ? adj_stage_x0b.p : nullptr, T_d, face_d, status_d, steps_d);
        PMC_HIP(hipMemcpy2DAsync(u_bar + (size_t)b0 * ld_bar, sizeof(double) * ld_bar, adj_stage_ubar.p, sizeof(double) * n_face,
                                 sizeof(double) * n_face, n, hipMemcpyDeviceToHost, st));
        if (x0_bar) PMC_HIP(hipMemcpyAsync(x0_bar + 3 * o, adj_stage_x0b.p, sizeof(double) * 3 * c, hipMemcpyDeviceToHost, st));
        if (T) PMC_HIP(hipMemcpyAsync(T + o, T_d, sizeof(double) * c, hipMemcpyDeviceToHost, st));
        if (exit_face) PMC_HIP(hipMemcpyAsync(exit_face + o, face_d, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipMemcpyAsync(status + o, status_d, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        if (nsteps) PMC_HIP(hipMemcpyAsync(nsteps + o, steps_d, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

void Tracer::reduce_seed(int nbatch, const double* T, const int32_t* status, int qkind, double* T_bar, int memspace) {
    PMC_REQUIRE(nbatch >= 1, "pmc_tracer_reduce_seed: nbatch must be at least 1");
    PMC_REQUIRE(T && status && T_bar, "pmc_tracer_reduce_seed: NULL array");
    PMC_REQUIRE(qkind == PMC_TRACER_MEAN || qkind == PMC_TRACER_MIN, "pmc_tracer_reduce_seed: kind must be PMC_TRACER_MEAN or _MIN");
    PMC_REQUIRE(memspace == PMC_MEM_HOST || memspace == PMC_MEM_DEVICE, "pmc_tracer_reduce_seed: bad memspace");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t cnt = (size_t)nbatch * npart;
    const bool host = memspace == PMC_MEM_HOST;
    if (host) {
        red_T.ensure(cnt);
        red_s.ensure(cnt);
        seed_tb.ensure(cnt);
        PMC_HIP(hipMemcpyAsync(red_T.p, T, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        PMC_HIP(hipMemcpyAsync(red_s.p, status, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, st));
    }
    tracer_seed_kernel<<<(unsigned)nbatch, kTracerThreads, 0, st>>>(npart, host ? red_T.p : T, host ? red_s.p : status, qkind,
                                                                    host ? seed_tb.p : T_bar);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    if (host) PMC_HIP(hipMemcpyAsync(T_bar, seed_tb.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
}

const double* Tracer::loglik_seed(hipStream_t st, int nb, const double* T_d, const double* data_d, double noise) {
    const int64_t total = (int64_t)nb * npart;
    seed_tb.ensure((size_t)total);
    tracer_loglik_seed_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(total, npart, T_d, data_d, nex.p, noise, seed_tb.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(1);
    return seed_tb.p;
}

}  // namespace pmc

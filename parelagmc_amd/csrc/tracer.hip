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

__device__ __forceinline__ void walk(const BoxRec* __restrict__ recs, const double* __restrict__ ub, int64_t stride_face,
                                     int max_steps, int e, Path& o) {
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

__device__ __forceinline__ void walk(const TetRec* __restrict__ recs, const double* __restrict__ ub, int64_t stride_face,
                                     int max_steps, int e, Path& o) {
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
    walk(recs, u + (int64_t)b * stride_batch, stride_face, max_steps, e0[p], o);
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
    ctx.activate();
    hipStream_t st = ctx.stream;
    recs.upload(rec_h, st);
    x0.upload(xs, st);
    e0.upload(es, st);
    orig.upload(order, st);
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

}  // namespace pmc

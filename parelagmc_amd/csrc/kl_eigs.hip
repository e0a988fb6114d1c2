// Matrix-free eigensolver behind the Matern KL sampler (the reference's MaternCovariance::SolveEigenvalue, whose scalable
// branch is a block eigensolver on the generalised problem A v = lambda W v, A = W C W, W = diag(P0 mass)).
//
// With y = W^1/2 v the problem is K y = lambda y, K = W^1/2 C W^1/2, K_ij = sqrt(w_i) c(|x_i - x_j|) sqrt(w_j),
// c(r) = exp(-r / corlen) (3D Matern with nu = 1/2), c = 1 where r / corlen < 1e-10, K_ii = w_i.  K is never stored.
//
//   kl_matern_apply_kernel   Y = K X for a block of b columns.  Blocks live on the device ROW-major, n x bp with bp = b
//                            rounded up to 16 and zero pad columns, so a 16-column tile of a row is one 128-byte segment.
//                            v_mfma_f64_16x16x4f64 with A = a 16 x 4 tile of K that the lanes evaluate themselves (lane l:
//                            row l & 15, column l >> 4: one sqrt and one exp per MFMA step), B = 4 rows of X out of LDS,
//                            D = 16 rows of Y.  The K entry is used for every column tile of the block (up to 8 per
//                            workgroup column group).  The x_j, sqrt(w_j) and X rows of a chunk of kJc columns of K go
//                            through a double-buffered LDS stage, the next chunk in registers while one is multiplied.
//   kl_gram_kernel           partial A^T B (bp x bp) per row range, MFMA; kl_sum_parts_kernel adds the partials in a fixed
//                            order, so the result is deterministic for a fixed grid.
//   kl_rotate_kernel         Z = X S, S bp x bp, MFMA.
//   kl_lincomb_kernel, kl_colscale_kernel, kl_colsumsq_kernel: the O(n b) vector work of the filter and the stop rule.
//
// Host side (plain C++): Chebyshev-filtered subspace iteration, Cholesky-QR twice, cyclic Jacobi on the b x b projected
// matrix.  No LAPACK.
#include "handles.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>

namespace pmc {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kApWaves = 8;     // waves per workgroup of the block product: 16 rows of Y each, 128 rows per workgroup
constexpr int kJc = 32;         // columns of K per LDS stage
constexpr int kMaxTiles = 8;    // column tiles of 16 per workgroup: wider blocks take several column groups
constexpr int kMaxBlock = 512;  // m + guard

// Operand maps of v_mfma_f64_16x16x4f64 (checked with exact integer data in tests/test_gpu_kl.py):
//   A (16 x 4): lane l holds A[l & 15][l >> 4];   B (4 x 16): lane l holds B[l >> 4][l & 15];
//   D (16 x 16): lane l, register r holds D[(l >> 4) + 4 r][l & 15].
//
// pts[j] = (x_j, y_j, z_j, sqrt(w_j)).  Workgroup (bx, by, bz): rows [128 bx, 128 bx + 128), chunks [by cps, (by + 1) cps) of
// the columns of K, column tiles [bz NT, bz NT + NT) of X.  by > 0 exists only on small n (too few row blocks to fill the
// chip): every by writes its own partial Y, kl_sum_parts_kernel adds them.
// MFMA == false is the measurement build of the kernel: every K entry is still evaluated, the MFMAs are dropped.
template <int NT, bool MFMA>
__global__ __launch_bounds__(64 * kApWaves) void kl_matern_apply_kernel(int n, int bp, int nchunks, int cps,
                                                                         const double4* __restrict__ pts,
                                                                         const double* __restrict__ w, double inv_corlen,
                                                                         const double* __restrict__ X,
                                                                         double* __restrict__ Y) {
    constexpr int kCols = 16 * NT;
    constexpr int kLd = kCols + ((NT & 1) ? 0 : 16);   // row stride = 16 mod 32 doubles: the 4 rows an MFMA step reads
                                                       // start 32 banks apart (ds_read_b64: 64 banks of 4 bytes)
    constexpr int kStage = kJc * kCols / (64 * kApWaves);
    __shared__ double xs[2][kJc][kLd];
    __shared__ double4 ps[2][kJc];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, lr = lane & 15;
    const int i = (blockIdx.x * kApWaves + wave) * 16 + lr;
    const int c0 = blockIdx.z * kCols;
    double xi = 0.0, yi = 0.0, zi = 0.0, swi = 0.0, wi = 0.0;
    if (i < n) {
        const double4 p = pts[i];
        xi = p.x, yi = p.y, zi = p.z, swi = p.w;
        wi = w[i];
    }
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double xr[kStage];
    double4 pr = make_double4(0.0, 0.0, 0.0, 0.0);
    // entry e = tid + s 512 of the [kJc rows][kCols columns] tile: consecutive threads read consecutive columns of one row
    auto load_chunk = [&](int c) {
        const int j0 = c * kJc;
#pragma unroll
        for (int s = 0; s < kStage; ++s) {
            const int e = tid + s * 64 * kApWaves;
            const int j = j0 + e / kCols, col = c0 + e % kCols;
            xr[s] = (j < n && col < bp) ? X[(size_t)j * bp + col] : 0.0;
        }
        if (tid < kJc) pr = (j0 + tid < n) ? pts[j0 + tid] : make_double4(0.0, 0.0, 0.0, 0.0);   // sqrt(w) = 0: K_ij = 0 past n
    };
    const int c_lo = blockIdx.y * cps, c_hi = min(nchunks, c_lo + cps);
    if (c_lo < c_hi) load_chunk(c_lo);
    for (int c = c_lo; c < c_hi; ++c) {
        const int buf = (c - c_lo) & 1;
#pragma unroll
        for (int s = 0; s < kStage; ++s) {
            const int e = tid + s * 64 * kApWaves;
            xs[buf][e / kCols][e % kCols] = xr[s];
        }
        if (tid < kJc) ps[buf][tid] = pr;
        // this buffer was last read two chunks ago; every wave has passed the barrier of the chunk in between since
        __syncthreads();
        if (c + 1 < c_hi) load_chunk(c + 1);   // in flight while this chunk is multiplied
#pragma unroll
        for (int kk = 0; kk < kJc / 4; ++kk) {
            const int jj = 4 * kk + kq;
            const double4 p = ps[buf][jj];
            const double dx = xi - p.x, dy = yi - p.y, dz = zi - p.z;
            const double kr = sqrt(dx * dx + dy * dy + dz * dz) * inv_corlen;
            double a = (kr < 1e-10 ? 1.0 : exp(-kr)) * (swi * p.w);
            if (c * kJc + jj == i) a = wi;
            if (MFMA) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xs[buf][jj][16 * t + lr], acc[t], 0, 0, 0);
            } else {
                acc[0][0] += a * xs[buf][jj][lr];
            }
        }
    }
    double* y = Y + (size_t)blockIdx.y * n * bp;
    const int row0 = (blockIdx.x * kApWaves + wave) * 16 + kq;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = c0 + 16 * t + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            if (row < n && col < bp) y[(size_t)row * bp + col] = acc[t][r];
        }
    }
}

// out[e] = sum_s parts[s len + e], s ascending
__global__ void kl_sum_parts_kernel(size_t len, int nparts, const double* __restrict__ parts, double* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (size_t)gridDim.x * blockDim.x) {
        double s = parts[e];
        for (int p = 1; p < nparts; ++p) s += parts[(size_t)p * len + e];
        out[e] = s;
    }
}

// parts[blockIdx.x][a][c] = sum over the rows of range blockIdx.x of A[i][a] B[i][c]; one wave per 16 x 16 tile
// (blockIdx.y = tile_a bt + tile_c).  MFMA operand A = a 4-row slab of A transposed, operand B = the same rows of B.
__global__ __launch_bounds__(64) void kl_gram_kernel(int n, int bp, int rows_per, const double* __restrict__ A,
                                                     const double* __restrict__ B, double* __restrict__ parts) {
    const int lane = threadIdx.x, kq = lane >> 4, lr = lane & 15;
    const int bt = bp / 16;
    const int a0 = (blockIdx.y / bt) * 16, b0 = (blockIdx.y % bt) * 16;
    const int i_lo = blockIdx.x * rows_per, i_hi = min(n, i_lo + rows_per);
    f64x4 acc0 = f64x4{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
    for (int i = i_lo; i < i_hi; i += 8) {
        const int r0 = i + kq, r1 = i + 4 + kq;
        const double a_0 = r0 < i_hi ? A[(size_t)r0 * bp + a0 + lr] : 0.0, b_0 = r0 < i_hi ? B[(size_t)r0 * bp + b0 + lr] : 0.0;
        const double a_1 = r1 < i_hi ? A[(size_t)r1 * bp + a0 + lr] : 0.0, b_1 = r1 < i_hi ? B[(size_t)r1 * bp + b0 + lr] : 0.0;
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_0, b_0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_1, b_1, acc1, 0, 0, 0);
    }
    double* out = parts + (size_t)blockIdx.x * bp * bp;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(size_t)(a0 + kq + 4 * r) * bp + b0 + lr] = acc0[r] + acc1[r];
}

// Z = X S: 16 rows per wave, 4 column tiles per workgroup column (blockIdx.y)
constexpr int kRotTiles = 4;
__global__ __launch_bounds__(256) void kl_rotate_kernel(int n, int bp, const double* __restrict__ X,
                                                        const double* __restrict__ S, double* __restrict__ Z) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, lr = lane & 15;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    const int t0 = blockIdx.y * kRotTiles, bt = bp / 16;
    const int i = i0 + lr;
    f64x4 acc[kRotTiles];
#pragma unroll
    for (int t = 0; t < kRotTiles; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < bp; a += 4) {
        const double xa = i < n ? X[(size_t)i * bp + a + kq] : 0.0;
#pragma unroll
        for (int t = 0; t < kRotTiles; ++t) {
            if (t0 + t < bt)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, S[(size_t)(a + kq) * bp + 16 * (t0 + t) + lr], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < kRotTiles; ++t) {
        if (t0 + t >= bt) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + kq + 4 * r;
            if (row < n) Z[(size_t)row * bp + 16 * (t0 + t) + lr] = acc[t][r];
        }
    }
}

// Z = alpha A + beta B + gamma C (B, C may be null; Z may be one of the inputs)
__global__ void kl_lincomb_kernel(size_t len, double alpha, const double* A, double beta, const double* B, double gamma,
                                  const double* C, double* Z) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (size_t)gridDim.x * blockDim.x) {
        double z = alpha * A[e];
        if (B) z = fma(beta, B[e], z);
        if (C) z = fma(gamma, C[e], z);
        Z[e] = z;
    }
}

// X[i][c] *= s[c]
__global__ void kl_colscale_kernel(size_t len, int bp, const double* __restrict__ s, double* __restrict__ X) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (size_t)gridDim.x * blockDim.x)
        X[e] *= s[e % bp];
}

// parts[blockIdx.x][c] = sum over the rows of range blockIdx.x of (A[i][c] - theta[c] B[i][c])^2 (B null: of A[i][c]^2)
__global__ void kl_colsumsq_kernel(int n, int bp, int rows_per, const double* __restrict__ A, const double* __restrict__ B,
                                   const double* __restrict__ theta, double* __restrict__ parts) {
    const int i_lo = blockIdx.x * rows_per, i_hi = min(n, i_lo + rows_per);
    for (int c = threadIdx.x; c < bp; c += blockDim.x) {
        const double th = B ? theta[c] : 0.0;
        double s = 0.0;
        for (int i = i_lo; i < i_hi; ++i) {
            double v = A[(size_t)i * bp + c];
            if (B) v = fma(-th, B[(size_t)i * bp + c], v);
            s = fma(v, v, s);
        }
        parts[(size_t)blockIdx.x * bp + c] = s;
    }
}

// row-major n x bp (zero pad columns) <- column-major n x b, and back (first b columns)
__global__ void kl_to_rows_kernel(int n, int b, int bp, const double* __restrict__ cm, double* __restrict__ rm) {
    const size_t len = (size_t)n * bp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / bp;
        const int c = (int)(e % bp);
        rm[e] = c < b ? cm[(size_t)c * n + i] : 0.0;
    }
}
__global__ void kl_to_cols_kernel(int n, int b, int bp, const double* __restrict__ rm, double* __restrict__ cm) {
    const size_t len = (size_t)n * b;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (size_t)gridDim.x * blockDim.x) {
        const size_t c = e / n, i = e % n;
        cm[e] = rm[i * bp + c];
    }
}

unsigned grid_for(size_t len) { return (unsigned)std::min<size_t>((len + 255) / 256, 4096); }

// ---- device side of one problem -----------------------------------------------------------------------------------------
struct MaternOp {
    hipStream_t st;
    int n, b, bp;
    double inv_corlen;
    DevBuf<double4> pts;
    DevBuf<double> w;
    DevBuf<double> parts;   // partial Y of the split products / partial Gram matrices
    DevBuf<double> small;   // bp x bp matrix, theta / scale vectors
    int jsplit, cps, nchunks, gram_ranges, gram_rows, norm_ranges, norm_rows;
    int64_t products = 0;

    MaternOp(hipStream_t st_, int n_, int b_, const double* xyz, const double* w_diag, double corlen)
        : st(st_), n(n_), b(b_), bp((b_ + 15) / 16 * 16), inv_corlen(1.0 / corlen) {
        std::vector<double4> h((size_t)n);
        for (int i = 0; i < n; ++i) h[(size_t)i] = make_double4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], std::sqrt(w_diag[i]));
        pts.upload(h.data(), h.size(), st);
        w.upload(w_diag, (size_t)n, st);
        PMC_HIP(hipStreamSynchronize(st));   // h leaves scope
        nchunks = (n + kJc - 1) / kJc;
        // too few row blocks to fill the chip (256 CUs): split the columns of K over up to 16 workgroup rows
        const int row_blocks = (n + 16 * kApWaves - 1) / (16 * kApWaves);
        jsplit = std::max(1, std::min({16, 256 / row_blocks, nchunks}));
        cps = (nchunks + jsplit - 1) / jsplit;
        jsplit = (nchunks + cps - 1) / cps;
        // row ranges of the reductions: fixed by (n, bp) alone, so the sums are reproducible
        gram_ranges = std::max(1, std::min({64, n / 256, (1 << 22) / (bp * bp)}));
        gram_rows = (n + gram_ranges - 1) / gram_ranges;
        norm_ranges = std::max(1, std::min(256, n / 64));
        norm_rows = (n + norm_ranges - 1) / norm_ranges;
        size_t np = std::max((size_t)gram_ranges * bp * bp, (size_t)norm_ranges * bp);
        if (jsplit > 1) np = std::max(np, (size_t)jsplit * n * bp);
        parts.alloc(np);
        small.alloc((size_t)bp * bp + 2 * (size_t)bp);
    }
    size_t len() const { return (size_t)n * bp; }

    template <bool MFMA>
    void apply_t(const double* X, double* Y) {
        const int bt = bp / 16;
        const int groups = (bt + kMaxTiles - 1) / kMaxTiles;
        const int nt = (bt + groups - 1) / groups;
        const dim3 grid((unsigned)((n + 16 * kApWaves - 1) / (16 * kApWaves)), (unsigned)jsplit, (unsigned)groups);
        double* out = jsplit > 1 ? parts.p : Y;
#define PMC_KL_APPLY(NT)                                                                                                   \
    case NT:                                                                                                               \
        kl_matern_apply_kernel<NT, MFMA><<<grid, 64 * kApWaves, 0, st>>>(n, bp, nchunks, cps, pts.p, w.p, inv_corlen, X, out); \
        break;
        switch (nt) {
            PMC_KL_APPLY(1)
            PMC_KL_APPLY(2)
            PMC_KL_APPLY(3)
            PMC_KL_APPLY(4)
            PMC_KL_APPLY(5)
            PMC_KL_APPLY(6)
            PMC_KL_APPLY(7)
            PMC_KL_APPLY(8)
            default: throw Error(PMC_ERR_INTERNAL, "kl_matern_apply: bad tile count");
        }
#undef PMC_KL_APPLY
        PMC_HIP(hipGetLastError());
        if (jsplit > 1) {
            kl_sum_parts_kernel<<<grid_for(len()), 256, 0, st>>>(len(), jsplit, parts.p, Y);
            PMC_HIP(hipGetLastError());
        }
        count_kernel_launches(jsplit > 1 ? 2 : 1);
        ++products;
    }
    void apply(const double* X, double* Y) {
#ifdef PMC_KL_EVAL_ONLY
        apply_t<false>(X, Y);   // measurement build: the evaluations of K without the MFMAs
#else
        apply_t<true>(X, Y);
#endif
    }

    // host G (b x b, row-major) = A^T B
    void gram(const double* A, const double* B, std::vector<double>& G) {
        const int bt = bp / 16;
        kl_gram_kernel<<<dim3((unsigned)gram_ranges, (unsigned)(bt * bt)), 64, 0, st>>>(n, bp, gram_rows, A, B, parts.p);
        PMC_HIP(hipGetLastError());
        kl_sum_parts_kernel<<<grid_for((size_t)bp * bp), 256, 0, st>>>((size_t)bp * bp, gram_ranges, parts.p, small.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(2);
        std::vector<double> h((size_t)bp * bp);
        PMC_HIP(hipMemcpyAsync(h.data(), small.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        G.resize((size_t)b * b);
        for (int r = 0; r < b; ++r)
            for (int c = 0; c < b; ++c) G[(size_t)r * b + c] = h[(size_t)r * bp + c];
    }
    // Z = X S, S host b x b row-major
    void rotate(const double* X, const std::vector<double>& S, double* Z) {
        std::vector<double> h((size_t)bp * bp, 0.0);
        for (int r = 0; r < b; ++r)
            for (int c = 0; c < b; ++c) h[(size_t)r * bp + c] = S[(size_t)r * b + c];
        PMC_HIP(hipMemcpyAsync(small.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
        PMC_HIP(hipStreamSynchronize(st));   // h leaves scope
        const int bt = bp / 16;
        kl_rotate_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)((bt + kRotTiles - 1) / kRotTiles)), 256, 0, st>>>(
            n, bp, X, small.p, Z);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
    void lincomb(double alpha, const double* A, double beta, const double* B, double gamma, const double* C, double* Z) {
        kl_lincomb_kernel<<<grid_for(len()), 256, 0, st>>>(len(), alpha, A, beta, B, gamma, C, Z);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
    // ss[c] = sum_i (A[i][c] - theta[c] B[i][c])^2, c < b (B null: column sums of squares of A)
    void colsumsq(const double* A, const double* B, const std::vector<double>* theta, std::vector<double>& ss) {
        double* th = small.p + (size_t)bp * bp;
        if (B) {
            std::vector<double> h((size_t)bp, 0.0);
            std::copy(theta->begin(), theta->begin() + b, h.begin());
            PMC_HIP(hipMemcpyAsync(th, h.data(), sizeof(double) * bp, hipMemcpyHostToDevice, st));
            PMC_HIP(hipStreamSynchronize(st));
        }
        kl_colsumsq_kernel<<<(unsigned)norm_ranges, 256, 0, st>>>(n, bp, norm_rows, A, B, th, parts.p);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
        std::vector<double> h((size_t)norm_ranges * bp);
        PMC_HIP(hipMemcpyAsync(h.data(), parts.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
        ss.assign((size_t)b, 0.0);
        for (int r = 0; r < norm_ranges; ++r)
            for (int c = 0; c < b; ++c) ss[(size_t)c] += h[(size_t)r * bp + c];
    }
    void colscale(const std::vector<double>& s, double* X) {
        double* sd = small.p + (size_t)bp * bp + bp;
        std::vector<double> h((size_t)bp, 0.0);
        std::copy(s.begin(), s.begin() + b, h.begin());
        PMC_HIP(hipMemcpyAsync(sd, h.data(), sizeof(double) * bp, hipMemcpyHostToDevice, st));
        PMC_HIP(hipStreamSynchronize(st));
        kl_colscale_kernel<<<grid_for(len()), 256, 0, st>>>(len(), bp, sd, X);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
    }
};

// ---- small dense problems on the host ---------------------------------------------------------------------------------
// G = L L^T in place (lower triangle); false on a pivot that is not positive
bool cholesky(std::vector<double>& G, int b) {
    for (int j = 0; j < b; ++j) {
        double d = G[(size_t)j * b + j];
        for (int k = 0; k < j; ++k) d -= G[(size_t)j * b + k] * G[(size_t)j * b + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        d = std::sqrt(d);
        G[(size_t)j * b + j] = d;
        for (int i = j + 1; i < b; ++i) {
            double s = G[(size_t)i * b + j];
            for (int k = 0; k < j; ++k) s -= G[(size_t)i * b + k] * G[(size_t)j * b + k];
            G[(size_t)i * b + j] = s / d;
        }
    }
    return true;
}
// S = L^-T (upper triangular), L the lower triangle of `L`
void inverse_transposed(const std::vector<double>& L, int b, std::vector<double>& S) {
    std::vector<double> M((size_t)b * b, 0.0);   // M = L^-1, lower triangular
    for (int c = 0; c < b; ++c) {
        M[(size_t)c * b + c] = 1.0 / L[(size_t)c * b + c];
        for (int r = c + 1; r < b; ++r) {
            double s = 0.0;
            for (int k = c; k < r; ++k) s += L[(size_t)r * b + k] * M[(size_t)k * b + c];
            M[(size_t)r * b + c] = -s / L[(size_t)r * b + r];
        }
    }
    S.assign((size_t)b * b, 0.0);
    for (int r = 0; r < b; ++r)
        for (int c = 0; c <= r; ++c) S[(size_t)c * b + r] = M[(size_t)r * b + c];
}
// Cyclic Jacobi on the symmetric H (b x b, destroyed): theta descending, column k of S (row-major) its eigenvector
void jacobi_eig(std::vector<double>& H, int b, std::vector<double>& theta, std::vector<double>& S) {
    std::vector<double> Vt((size_t)b * b, 0.0);   // row k = eigenvector k: rotations act on contiguous rows
    for (int k = 0; k < b; ++k) Vt[(size_t)k * b + k] = 1.0;
    for (int r = 0; r < b; ++r)
        for (int c = r + 1; c < b; ++c) H[(size_t)r * b + c] = H[(size_t)c * b + r] = 0.5 * (H[(size_t)r * b + c] + H[(size_t)c * b + r]);
    const double eps = 2.220446049250313e-16;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < b - 1; ++p) {
            for (int q = p + 1; q < b; ++q) {
                const double apq = H[(size_t)p * b + q];
                const double app = H[(size_t)p * b + p], aqq = H[(size_t)q * b + q];
                if (std::fabs(apq) <= 0.25 * eps * std::sqrt(std::fabs(app * aqq)) || apq == 0.0) continue;
                rotated = true;
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                double* hp = &H[(size_t)p * b];
                double* hq = &H[(size_t)q * b];
                for (int k = 0; k < b; ++k) {   // rows p, q of the symmetric matrix
                    const double a = hp[k], d = hq[k];
                    hp[k] = c * a - s * d;
                    hq[k] = s * a + c * d;
                }
                for (int k = 0; k < b; ++k) {   // mirror into columns p, q
                    H[(size_t)k * b + p] = hp[k];
                    H[(size_t)k * b + q] = hq[k];
                }
                hp[p] = app - t * apq;
                hq[q] = aqq + t * apq;
                hp[q] = hq[p] = 0.0;
                double* vp = &Vt[(size_t)p * b];
                double* vq = &Vt[(size_t)q * b];
                for (int k = 0; k < b; ++k) {
                    const double a = vp[k], d = vq[k];
                    vp[k] = c * a - s * d;
                    vq[k] = s * a + c * d;
                }
            }
        }
        if (!rotated) break;
    }
    std::vector<int> order((size_t)b);
    for (int k = 0; k < b; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return H[(size_t)x * b + x] > H[(size_t)y * b + y]; });
    theta.resize((size_t)b);
    S.assign((size_t)b * b, 0.0);
    for (int k = 0; k < b; ++k) {
        const int o = order[(size_t)k];
        theta[(size_t)k] = H[(size_t)o * b + o];
        for (int r = 0; r < b; ++r) S[(size_t)r * b + k] = Vt[(size_t)o * b + r];
    }
}

// X <- orthonormal basis of span(X): columns scaled to unit length, then Cholesky-QR until two passes have run without a
// shift (a shifted pass only improves the conditioning for the next one)
void orthonormalise(MaternOp& op, double*& X, double*& Z) {
    const int b = op.b;
    std::vector<double> ss, G, S;
    int clean = 0;
    for (int pass = 0; pass < 6 && clean < 2; ++pass) {
        op.colsumsq(X, nullptr, nullptr, ss);
        for (int c = 0; c < b; ++c) {
            if (!(ss[(size_t)c] > 0.0) || !std::isfinite(ss[(size_t)c]))
                throw Error(PMC_ERR_INTERNAL, "pmc_kl_matern_eigs: a column of the block vanished or overflowed");
            ss[(size_t)c] = 1.0 / std::sqrt(ss[(size_t)c]);
        }
        op.colscale(ss, X);
        op.gram(X, X, G);
        for (int r = 0; r < b; ++r)
            for (int c = r + 1; c < b; ++c) G[(size_t)r * b + c] = G[(size_t)c * b + r] = 0.5 * (G[(size_t)r * b + c] + G[(size_t)c * b + r]);
        std::vector<double> L = G;
        bool shifted = false;
        if (!cholesky(L, b)) {
            // shifted Cholesky-QR: unit columns, so ||G|| <= b
            shifted = true;
            double shift = 1e-13 * b;
            for (int tries = 0;; ++tries) {
                L = G;
                for (int k = 0; k < b; ++k) L[(size_t)k * b + k] += shift;
                if (cholesky(L, b)) break;
                if (tries == 8) throw Error(PMC_ERR_INTERNAL, "pmc_kl_matern_eigs: the block lost rank (Cholesky-QR failed)");
                shift *= 100.0;
            }
        }
        inverse_transposed(L, b, S);
        op.rotate(X, S, Z);
        std::swap(X, Z);
        if (!shifted) ++clean;
    }
    if (clean < 2) throw Error(PMC_ERR_INTERNAL, "pmc_kl_matern_eigs: the block could not be orthonormalised");
}

void check_problem(const char* who, const pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag,
                   double corlen) {
    const std::string f(who);
    PMC_REQUIRE(dim == 3, f + ": only dim == 3 runs on the device (the 2D Matern kernel needs the Bessel function K1; 2D "
                              "meshes are small enough for a dense host solve)");
    PMC_REQUIRE(std::isfinite(corlen) && corlen > 0.0, f + ": corlen must be positive and finite");
    PMC_REQUIRE(n >= 1, f + ": n must be at least 1");
    PMC_REQUIRE(c != nullptr && centroids != nullptr && w_diag != nullptr, f + ": NULL argument (ctx / centroids / w_diag)");
    for (int i = 0; i < n; ++i) PMC_REQUIRE(std::isfinite(w_diag[i]) && w_diag[i] > 0.0, f + ": w_diag must be positive and finite");
    for (size_t e = 0; e < (size_t)n * 3; ++e) PMC_REQUIRE(std::isfinite(centroids[e]), f + ": centroids must be finite");
}

constexpr uint32_t kStartStream = 0x4b4c4531u;   // Philox stream of the start block ("KLE1")

}  // namespace

void kl_matern_apply(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int ncols,
                     const double* X, double* Y) {
    check_problem("pmc_kl_matern_apply", c, dim, n, centroids, w_diag, corlen);
    PMC_REQUIRE(ncols >= 1 && ncols <= kMaxBlock, "pmc_kl_matern_apply: ncols must lie in [1, 512]");
    PMC_REQUIRE(X != nullptr && Y != nullptr, "pmc_kl_matern_apply: NULL argument (X / Y)");
    c->activate();
    hipStream_t st = c->stream;
    MaternOp op(st, n, ncols, centroids, w_diag, corlen);
    DevBuf<double> cm((size_t)n * ncols), xr(op.len()), yr(op.len());
    PMC_HIP(hipMemcpyAsync(cm.p, X, sizeof(double) * n * ncols, hipMemcpyHostToDevice, st));
    kl_to_rows_kernel<<<grid_for(op.len()), 256, 0, st>>>(n, ncols, op.bp, cm.p, xr.p);
    PMC_HIP(hipGetLastError());
    op.apply(xr.p, yr.p);
    kl_to_cols_kernel<<<grid_for((size_t)n * ncols), 256, 0, st>>>(n, ncols, op.bp, yr.p, cm.p);
    PMC_HIP(hipGetLastError());
    count_kernel_launches(2);
    PMC_HIP(hipMemcpyAsync(Y, cm.p, sizeof(double) * n * ncols, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
}

void kl_matern_eigs(pmc_ctx* c, int dim, int n, const double* centroids, const double* w_diag, double corlen, int nmodes,
                    const pmc_kl_eigs_opts* opts, double* evals, double* evect0, pmc_kl_eigs_info* info) {
    const auto t_start = std::chrono::steady_clock::now();
    pmc_kl_eigs_opts o;
    pmc_kl_eigs_opts_default(&o);
    if (opts) o = *opts;
    PMC_REQUIRE(dim == 3, "pmc_kl_matern_eigs: only dim == 3 runs on the device (the 2D Matern kernel needs the Bessel function "
                          "K1; 2D meshes are small enough for a dense host solve)");
    PMC_REQUIRE(std::isfinite(corlen) && corlen > 0.0, "pmc_kl_matern_eigs: corlen must be positive and finite");
    PMC_REQUIRE(nmodes >= 1 && n >= 1, "pmc_kl_matern_eigs: nmodes and n must be at least 1");
    PMC_REQUIRE(o.guard >= 0 && o.degree >= 1 && o.max_iter >= 1 && std::isfinite(o.tol) && o.tol >= 0.0,
                "pmc_kl_matern_eigs: options out of range (guard >= 0, degree >= 1, max_iter >= 1, tol >= 0)");
    const int m = std::min(nmodes, n);   // MaternCovariance: the number of modes is capped by the number of elements
    PMC_REQUIRE((int64_t)m + o.guard <= kMaxBlock, "pmc_kl_matern_eigs: m + guard exceeds 512 (the projected problem is solved "
                                                   "by Jacobi rotations on the host)");
    PMC_REQUIRE(evals != nullptr && evect0 != nullptr, "pmc_kl_matern_eigs: NULL argument (evals / evect0)");
    check_problem("pmc_kl_matern_eigs", c, dim, n, centroids, w_diag, corlen);
    const int b = std::min(m + o.guard, n);
    c->activate();
    hipStream_t st = c->stream;
    MaternOp op(st, n, b, centroids, w_diag, corlen);
    const size_t len = op.len();
    DevBuf<double> buf0(len), buf1(len), buf2(len), buf3(len);
    double *X = buf0.p, *Y = buf1.p, *Z = buf2.p, *T = buf3.p;
    {
        // start block: n b standard normals of the project's Philox generator (seed from the options, stream kStartStream),
        // entry (i, c) = realization c, entry i
        DevBuf<double> cm((size_t)n * b);
        k::normal_fill(st, n, b, o.seed, 0, kStartStream, 0.0, 1.0, cm.p);
        kl_to_rows_kernel<<<grid_for(len), 256, 0, st>>>(n, b, op.bp, cm.p, X);
        PMC_HIP(hipGetLastError());
        count_kernel_launches(1);
        PMC_HIP(hipStreamSynchronize(st));
    }
    std::vector<double> H, S, theta, ss;
    auto ritz = [&] {   // X orthonormal: Y = K X, then rotate both to the Ritz basis
        op.apply(X, Y);
        op.gram(X, Y, H);
        jacobi_eig(H, b, theta, S);
        op.rotate(X, S, Z);
        op.rotate(Y, S, T);
        std::swap(X, Z);
        std::swap(Y, T);
    };
    auto residual = [&]() -> double {   // max over the wanted columns of ||K y_k - theta_k y_k|| / theta_1
        op.colsumsq(Y, X, &theta, ss);
        double r = 0.0;
        for (int k = 0; k < m; ++k) r = std::max(r, std::sqrt(ss[(size_t)k]));
        return r / theta[0];
    };
    orthonormalise(op, X, Z);
    ritz();
    double res = residual();
    int it = 0;
    bool converged = res <= o.tol;
    while (!converged && it < o.max_iter) {
        ++it;
        // Chebyshev filter of degree d on [0, theta_b], scaled to 1 at theta_1 (three-term form: no power of K is formed)
        // Without a guard column (b == m < n) theta_b is a wanted value: at the edge of the damped interval it would be
        // scaled by exactly 1 while the unwanted values inside reach 1 at the extrema of the polynomial, and column m would
        // never separate.  The interval ends at 0.9 theta_b then: theta_m lies outside, where the polynomial grows
        // monotonically, so it gains on every smaller eigenvalue whatever the true gap is.
        const double top = (b == m && b < n) ? 0.9 * theta[(size_t)b - 1] : theta[(size_t)b - 1];
        const double lo = std::max(top, 1e-14 * theta[0]);
        const double e = 0.5 * lo, cc = 0.5 * lo;
        double sigma = e / (theta[0] - cc);
        const double tau = 2.0 / sigma;
        // Y1 = (K X - c X) sigma / e, K X = Y is known
        op.lincomb(sigma / e, Y, -cc * sigma / e, X, 0.0, nullptr, Z);
        double *P0 = X, *P1 = Z, *F0 = Y, *F1 = T;   // previous, current, two free blocks
        for (int d = 2; d <= o.degree; ++d) {
            const double sigma2 = 1.0 / (tau - sigma);
            op.apply(P1, F0);
            op.lincomb(2.0 * sigma2 / e, F0, -2.0 * sigma2 * cc / e, P1, -sigma * sigma2, P0, F0);
            double* old = P0;
            P0 = P1;
            P1 = F0;
            F0 = old;
            sigma = sigma2;
        }
        X = P1, Y = P0, Z = F0, T = F1;
        orthonormalise(op, X, Z);
        ritz();
        res = residual();
        converged = res <= o.tol;
    }
    // y -> v = W^-1/2 y, ascending eigenvalues, largest-magnitude entry of a column (first on ties) positive
    std::vector<double> h(len);
    PMC_HIP(hipMemcpyAsync(h.data(), X, sizeof(double) * len, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < m; ++k) {
        const int src = m - 1 - k;
        evals[k] = theta[(size_t)src];
        double* v = evect0 + (size_t)k * n;
        double big = -1.0, sign = 1.0;
        for (int i = 0; i < n; ++i) {
            v[i] = h[(size_t)i * op.bp + src] / std::sqrt(w_diag[i]);
            if (std::fabs(v[i]) > big) {
                big = std::fabs(v[i]);
                sign = v[i] < 0.0 ? -1.0 : 1.0;
            }
        }
        if (sign < 0.0)
            for (int i = 0; i < n; ++i) v[i] = -v[i];
    }
    if (info) {
        info->iterations = it;
        info->block_products = (int32_t)op.products;
        info->converged = converged ? 1 : 0;
        info->max_residual_rel = res;
        info->gap_rel = b > m ? (theta[(size_t)m - 1] - theta[(size_t)m]) / theta[0] : 0.0;
        info->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
}

}  // namespace pmc

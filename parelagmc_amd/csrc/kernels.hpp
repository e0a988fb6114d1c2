// Launchers of the CDNA4 (gfx950) kernels of the ParELAGMC hot path (the units k_*.hip, over kdev.hpp: device-side helpers,
// sell_rows.hpp: the SELL-64 gather loops, and klaunch.hpp: host-side launch helpers; this header is the one interface the
// rest of the library sees).  A banner names the unit that defines the declarations below it.  A kernel template and every
// launcher that instantiates it live in the same unit: each unit carries its own device code object, and an instantiation
// reachable from two units would be compiled and shipped twice.
//
// Kernel <-> reference operation:
//   sell_spmm / sell_residual / sell_cheb_step : K5 block saddle-point SpMV, K7 smoother on M,
//        K8 V-cycle smoothing/residual/transfer, K3/K4 restriction/prolongation, K11 projection
//   minres_* / lincomb3 / dot                  : K6 MINRES vector operations
//   normal_fill                                : K1 NormalDistributionSampler
//   interleave / deinterleave                  : K2 white-noise RHS scaling, K9 exp, K10 gather (fused with the layout change)
//   darcy_*                                    : K12-K15 per-sample M(k), BC elimination, Schur refresh, QoI
//
// All vectors are "interleaved" batches:
// row i, column (realization) k of a batch of nb lives at v[i*nb + k], nb in {1,2,4,8,16,32} or - as 2, 4, 8 column groups
// of 32 handled by one launch (gridDim.y) - 64, 128, 256.
#pragma once
#include "common.hpp"

namespace pmc {

// The PRECONDITIONED Krylov vectors z = B^-1 v of the MINRES solves, in the storage pmc_solver_opts.precond_storage asks
// for: fp32 (default) or fp64.  They are the method's search directions: whatever is stored IS the direction, every inner
// product and recurrence uses the stored values, so rounding them to fp32 perturbs the preconditioner by 6e-8 relative and
// nothing else (iteration counts and converged fields unchanged to 1e-12, true residuals at full size:
// tests/test_gpu_round4.py); each z is written once and read three times per iteration.  Lanczos vectors, operator products,
// w, x and every scalar are fp64 whatever the option says.  The launchers below take the vector with its storage type at
// run time and pick the kernel instantiation (the fp64 ones are the kernels every other caller uses anyway).
struct zvec {
    void* p = nullptr;
    bool f32 = true;
    zvec() = default;
    zvec(void* p_, bool f32_) : p(p_), f32(f32_) {}
    size_t elem_bytes() const { return f32 ? 4 : 8; }
    zvec operator+(size_t elems) const { return zvec(static_cast<char*>(p) + elems * elem_bytes(), f32); }
    explicit operator bool() const { return p != nullptr; }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};
// The same pair (pointer, storage) also names the vectors that live only inside one application of a V-cycle: the right-hand
// side a level receives and the coarse correction it returns (fp32 between the levels of the fp32-intermediate path of a
// shared-value hierarchy, fp64 everywhere else).  zconst wraps a read-only operand.
inline zvec zconst(const double* p) { return zvec(const_cast<double*>(p), false); }
inline zvec zconst(const float* p) { return zvec(const_cast<float*>(p), true); }
// device buffer behind a zvec: `count` entries in either storage
struct ZBuf {
    DevBuf<float> b;
    void ensure(size_t count, bool f32) { b.ensure(f32 ? count : 2 * count); }
    zvec v(bool f32) const { return zvec(b.p, f32); }
};

// Device view of a SELL-64 matrix.  vals == shared values (nslots) or, when bv, per-realization
// values (nslots*NB, interleaved like vectors).
struct SellView {
    int nrows = 0, nslices = 0;
    const int* slice_off = nullptr;
    const int* cols = nullptr;
    const double* vals = nullptr;
    bool bv = false;
    const int* sched = nullptr;   // optional slice processing order
    int tag = 0;                  // 1 = block saddle-point operator (own kernel instantiation / profile row)
    int ncols_hint = 0;           // number of columns (rows of x): kernels with 32-bit gather offsets check it
    bool diag_last = false;       // see Sell::diag_last
    bool f32 = false;             // bv only: vals points at fp32 values (per-realization values of a PRECONDITIONER matrix)
    // > 0: the matrix was built from csr_split_rows(A, split_log2) - nrows counts the pieces; the k::vc_* launchers then
    // start their row-split instantiations (launches of at most 8 realizations), which add the pieces of a row
    int split_log2 = 0;
};
inline SellView view(const Sell& S) {
    return {S.nrows, S.nslices, S.slice_off.p, S.cols.p, S.vals.p, false, S.sched.p, 0, S.ncols, S.diag_last};
}
inline SellView view_split(const Sell& S, int sl) {
    SellView v = view(S);
    v.split_log2 = sl;
    return v;
}
inline SellView view_bv(const Sell& S, const double* vals) {
    return {S.nrows, S.nslices, S.slice_off.p, S.cols.p, vals, true, S.sched.p, 0, S.ncols};
}
inline SellView view_bv32(const Sell& S, const float* vals) {
    SellView v = view_bv(S, reinterpret_cast<const double*>(vals));
    v.f32 = true;
    return v;
}

// Element-grouped SELL view of a per-realization mass matrix M(k) = sum_e c(k_e) M_e: every row stores its entries in
// two groups of `gw` slice columns, one per element the row's dof belongs to; the values of a group are the SHARED
// element-matrix entries w, and the realization enters only through the two per-row coefficients coef[e12[row]][k].
// A row product is  c1 * sum_g1 w x  +  c2 * sum_g2 w x : the matrix costs 12 B per stored entry for the whole batch
// instead of 8 B per entry per realization.
struct EgView {
    int nrows = 0, nslices = 0, gw = 0;
    const int* cols = nullptr;     // [nslices][2 gw][64]
    const double* w = nullptr;     // same layout
    const int* e12 = nullptr;      // [nrows][2] coefficient rows (n_elem = constant-one row for eliminated dofs)
};

// ---- k_sell.hip
// capacity (in blocks of nb doubles) of a partial-sum buffer for (fused) dots over nrows rows of a batch of nb columns:
// allocate dot_capacity(nrows, nb) * nb doubles
int dot_capacity(int nrows, int nb);
// ---- k_krylov.hip
// kernels this process has launched through the library so far (all handles, all threads): launch-rate diagnostics
uint64_t kernel_launch_count();
void count_kernel_launches(int n);
// ---- solver.hip
// one more solve on `path`, or one more event of enum pmc_solve_path (the launchers count the size-gated forms they take)
void count_solve_path(int path);

namespace k {

// The w / x updates of up to kWxWindow consecutive MINRES iterations are applied in ONE pass over the vectors
// (minres_wx_deferred): nothing reads w or x before the solve ends, and every update needs only its own iteration's
// coefficients and preconditioned vector.  A pass over c iterations costs c streams of the preconditioned vectors plus
// the w0 / w1 / x it carries from the pass before to the pass after - so the window is as long as memory allows
// (minres_solve picks it per solve, 8 ... kWxWindow): a solve that fits into one window reads every preconditioned vector
// once and writes x once, nothing else (the first pass starts from literal zeros instead of loading w0 / w1 / x, the last
// pass does not store w0 / w1).  With fp32-stored u, 20 iterations: 4 x 21 + 8 = 92 bytes per entry and solve; with the
// window of 8 of round 5 it was 228 plus 24 of fills.
// A pass walks its window in trips: the preconditioned vectors of a trip's iterations are requested together, w0 / w1 / x
// stay in registers across the trips.  A thread owns several entries in the same columns (one load of an iteration's
// coefficients serves all of them), so a trip is as many iterations as about 64 registers of u hold - four at four values
// per thread and four entries - and at most kWxDefer (WxShape in k_krylov.hip).
#ifndef PMC_WX_DEFER_N
#define PMC_WX_DEFER_N 8
#endif
static constexpr int kWxDefer = PMC_WX_DEFER_N;
static constexpr int kWxWindow = 32;
struct WxDeferred {
    const void* u[kWxWindow];   // preconditioned vectors of the pending iterations (rows of the maintained block), oldest first
    int slot[kWxWindow];         // coefficient set (MinresState::cW ring) of each
    int cnt;
    bool f32;                    // storage of the u vectors
    bool first;                  // nothing applied yet in this solve: w0 = w1 = 0, not loaded
    bool x_zero;                 // ... and the initial guess is zero: x not loaded either
    bool last;                   // nothing follows in this solve: w0 / w1 not stored
};

// Device-resident MINRES scalars, one entry per batch column.
struct MinresState {
    double beta[kMaxBatch], beta_old[kMaxBatch], eta[kMaxBatch], eta0[kMaxBatch];
    double gamma0[kMaxBatch], gamma1[kMaxBatch], sigma0[kMaxBatch], sigma1[kMaxBatch];
    double goal[kMaxBatch], alpha[kMaxBatch], delta[kMaxBatch], rho2[kMaxBatch], rho3[kMaxBatch];
    double cV[3][kMaxBatch];  // v_new = cV0*q + cV1*v1 + cV2*v0
    int active[kMaxBatch], iters[kMaxBatch], flag[kMaxBatch];
    int n_active, it, ring;
    // w_new = cW0*u1 + cW1*w0 + cW2*w1 ; x += cW3*w_new.  Iteration i (0-based) writes set i % ring: ring == 1 when the
    // update follows its iteration at once, the solve's window when updates are deferred.  LAST member: the host reads
    // only what precedes it (kMinresHeadBytes) at the end of a solve.
    double cW[kWxWindow][4][kMaxBatch];
};
static constexpr size_t kMinresHeadBytes = offsetof(MinresState, cW);

// ---- k_sell.hip (the vc_* launchers too: their kernels share sell_row_range specialisations with sell_spmm_kernel, and
// vc_restrict32 starts sell_spmm_kernel itself - see the head of k_sell.hip)
// y = A x (accumulate=false) or y += A x.  If dot_partial != nullptr (accumulate must be false) also
// writes per-block partial sums of <dot_with, A x>; returns the number of partial blocks written.
int spmm(hipStream_t st, int nb, const SellView& A, const double* x, double* y, bool accumulate,
          double* dot_partial, const double* dot_with);
// the same product from a vector in zvec storage (shared values, no accumulation): the operator products of the solver loop
int spmm_z(hipStream_t st, int nb, const SellView& A, zvec x, double* y, double* dot_partial, zvec dot_with);
// A MINRES iteration that never stores q = A u runs the operator twice (shared values, fp32-stored u, the operator tagged
// 1): spmm_z_dot leaves only the partials of <u, A u> - the very partials of spmm_z(.., dot_with = x) - and, once the scalar
// step has turned them into the Lanczos coefficients, spmm_z_update recomputes the row sums (the same bits) and writes
// v = c0 (A u) + c1 v1 + c2 v over v (the vector before last) together with its fp32 copy y32: what lincomb3 computes from
// a stored q.  v_zero: v is zero and not read (first iteration).  c0, c1, c2: per-column coefficients on the device.
struct LanczosUpdate {
    const double* __restrict__ c0 = nullptr;
    const double* __restrict__ c1 = nullptr;
    const double* __restrict__ c2 = nullptr;
    const double* __restrict__ v1 = nullptr;
    float* __restrict__ y32 = nullptr;
};
int spmm_z_dot(hipStream_t st, int nb, const SellView& A, zvec x, double* dot_partial);
void spmm_z_update(hipStream_t st, int nb, const SellView& A, zvec x, const LanczosUpdate& lz, double* v, bool v_zero);
// out = r - A x and coarse[i] = sum of out over the rows 8 i .. 8 i + 7 (restriction with the transpose of an
// "8 consecutive children, unit weights" prolongator); A.nrows must be a multiple of 8
void residual_restrict8(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, double* out,
                        double* coarse);
// out = r - A x
void residual(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, double* out);
// the same values sample-major, out[k * A.nrows + i] = post(r - A x)[i][k], post = exp if do_exp: what deinterleave (identity
// rows, no scaling) makes of residual's result, without the interleaved vector in between (shared values)
void residual_samples(hipStream_t st, int nb, const SellView& A, const double* r, const double* x, bool do_exp, double* out);
// y = A x and y32 = its fp32 copy from one launch (shared values, untagged matrix): spmm followed by copy_r32, without the
// pass that reads y again
void spmm_store32(hipStream_t st, int nb, const SellView& A, const double* x, double* y, float* y32);
// Chebyshev / Jacobi step:  d = a*d + b*dinv.*(r - A xin);  xout = xin + d   (xin != xout).
// dot_partial != nullptr: also per-block partials of <r, xout>; returns the number of blocks written.
int cheb_step(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
              const double* xin, double* d, double* xout, double a, double b, double* dot_partial = nullptr);
// the LAST step of a polynomial whose result is a preconditioned Krylov vector: as cheb_step, the iterate goes to zvec
// storage (rounded before the fused dot), d is left as it was
int cheb_step_z(hipStream_t st, int nb, const SellView& A, const double* dinv, bool dinv_bv, const double* r,
                const double* xin, double* d, zvec zout, double a, double b, double* dot_partial = nullptr);
// one-pass degree-2 polynomial from a zero guess: xout = dinv.*(c0 r - c1 As r), As = A D^-1 (shared values)
int poly2(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, double* xout,
          double c0, double c1, double* dot_partial = nullptr, const double* xadd = nullptr,
          const double* dot_with = nullptr, const int* padd_idx = nullptr, const double* padd_x = nullptr);
// ... into zvec storage (the value stored is the one the fused <r, xout> uses)
int poly2_z(hipStream_t st, int nb, const SellView& As, const double* dinv, bool dinv_bv, const double* r, zvec xout,
            double c0, double c1, double* dot_partial = nullptr, const double* xadd = nullptr,
            const double* dot_with = nullptr, const int* padd_idx = nullptr, const double* padd_x = nullptr);
// V-cycle level with fp32 intermediates (shared values; see vc_poly2_kernel): pre-smoothing from zero into an fp32 iterate,
// residual + restriction from it (fp32 residual), res -= (S P) xc, and the post-smoothing x + xc[parent] + p2(res) -> result
// with the fused <r, result>.  The level's right-hand side r (fp64 Lanczos vector, its fp32 copy written by k::lincomb3, or the
// coarse right-hand side the level above wrote), the coarse right-hand side it writes and the coarse correction xc it
// gathers come in either storage (zvec): fp32 ones are widened on load and rounded once on store, all arithmetic is fp64.
void vc_presmooth32(hipStream_t st, int nb, const SellView& As, const double* dinv, zvec r, float* xout, double c0, double c1);
// restriction over groups of 8 consecutive rows fused into the residual
void vc_residual_restrict8_32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse);
void vc_residual32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out);   // no restriction
// residual + restriction of an aggregation level renumbered by agg_pack_rows (segments per slice: seg_ptr / seg_cid / seg_pos)
void vc_residual_restrict_agg32(hipStream_t st, int nb, const SellView& A, zvec r, const float* x, float* out, zvec coarse,
                                const int* seg_ptr, const int* seg_cid, const int* seg_pos);
// coarse = Pt res: the separate restriction of a level without a fused one
void vc_restrict32(hipStream_t st, int nb, const SellView& Pt, const float* res, zvec coarse);
void vc_residual_coarse32(hipStream_t st, int nb, const SellView& SP, float* res, zvec xc);
// r is the operand of the fused dot only (top level of a cycle: fp64)
int vc_postsmooth32_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                      zvec xout, double c0, double c1, const double* r, const int* parent, zvec xc, double* dot_partial);
// ... and for a level with per-realization fp32 values and diagonals (Darcy; no S P: the coarse correction is added to the
// fp32 iterate, then residual and post-smoothing): the fine residual of the restriction is never stored
void vc_presmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const double* r, float* xout, double c0,
                       double c1);
void vc_restrict8_32_bv(hipStream_t st, int nb, const SellView& A, const double* r, const float* x, double* coarse);
void vc_prolong8_32(hipStream_t st, int nb, int n, float* x, const double* xc);
void vc_residual32_bv(hipStream_t st, int nb, const SellView& A, const double* r, const float* x, float* out);
int vc_postsmooth32_bv(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                       double* xout, double c0, double c1, const double* r, double* dot_partial);
int vc_postsmooth32_bv_z(hipStream_t st, int nb, const SellView& As, const double* dinv, const float* res, const float* x,
                         zvec xout, double c0, double c1, const double* r, double* dot_partial);
// y = A1 x1 + A2 x2 (A1 per-realization values, A2 shared values, same rows); optional fused dot
int pair_spmm_z(hipStream_t st, int nb, const SellView& A1, zvec x1, const SellView& A2, zvec x2, double* y,
                double* dot_partial, zvec dot_with);
// ---- k_darcy.hip
// out[slot][k] = vals[slot][k] * colscale[cols[slot]][k]
void scale_cols_bv(hipStream_t st, int nb, int64_t nslots, const int* cols, const double* vals, const double* colscale,
                   double* out);
// the fp32 copies the preconditioner kernels read: out_scaled = (float)(vals * colscale[cols]), out_vals = (float)vals
void scale_cols_bv32(hipStream_t st, int nb, int64_t nslots, const int* cols, const double* vals, const double* colscale,
                     float* out_scaled, float* out_vals);
// ---- k_krylov.hip
// MINRES w/x update on an index list of rows (w0, w1, x compact [nsel][nb]; u full)
void minres_wx_idx(hipStream_t st, int nb, int nsel, const int* rows, const double* c0, zvec u, const double* c1,
                   double* w0, const double* c2, const double* w1, const double* c3, double* x);
// first step from a zero guess: d = b*dinv.*r; x = d
int cheb_first(hipStream_t st, int nb, int n, const double* dinv, bool dinv_bv, const double* r, double* d,
               double* x, double b, double* dot_partial = nullptr);
// both return the number of partial blocks written
int wdot(hipStream_t st, int nb, int n, const double* w, const double* x, double* partial);
int dot_z(hipStream_t st, int nb, int n, const double* a, zvec b, double* partial);
// out = in rounded to zvec storage; dot_partial != nullptr: partials of <r, out>.  Returns the partial-block count.
int convert_z(hipStream_t st, int nb, int n, const double* in, zvec out, const double* r, double* dot_partial);
// out = in and out32 = in rounded to fp32, one pass (copy + convert_z of the same vector)
void copy_r32(hipStream_t st, int nb, int n, const double* in, double* out, float* out32);
void reduce_final(hipStream_t st, int nb, int nblocks, const double* partial, double* out);
void lincomb3(hipStream_t st, int nb, int n, const double* c0, const double* a, const double* c1, const double* b,
              const double* c2, double* y, float* y32 = nullptr);
void minres_wx(hipStream_t st, int nb, int n, const double* c0, zvec u, const double* c1, double* w0,
               const double* c2, const double* w1, const double* c3, double* x);
void fill(hipStream_t st, size_t n, double* x, double v);
void copy(hipStream_t st, size_t n, const double* src, double* dst);
void scale(hipStream_t st, size_t n, const double* in, double a, double* out);   // out = a in

// per-block partial sums of one dot product, in up to two segments (n blocks of nb doubles each): kernels that run side
// by side on two streams write a segment each
struct DotParts {
    const double* p1 = nullptr;
    int n1 = 0;
    const double* p2 = nullptr;
    int n2 = 0;
    int total() const { return n1 + n2; }
};
void minres_init(hipStream_t st, int nb, MinresState* s, const DotParts& d, double rel_tol, double abs_tol, int ring = 1);
// the pending w / x updates of B.cnt iterations on n rows: for j < cnt  w = cW0 u_j + cW1 w0 + cW2 w1; x += cW3 w;
// (w0, w1) <- (w1, w).  w0 is the OLDER direction on entry and on return (no role swap by the caller).  B.first: w0 / w1
// (with B.x_zero also x) hold nothing yet and count as zeros; B.last: w0 / w1 are left as they are.
void minres_wx_deferred(hipStream_t st, int nb, int n, const MinresState* s, const WxDeferred& B, double* w0, double* w1,
                        double* x);
void minres_scal1(hipStream_t st, int nb, MinresState* s, const DotParts& d);
void minres_scal2(hipStream_t st, int nb, MinresState* s, const DotParts& d);
// scal2 of this iteration followed by scal1 of the next one (d1 = partials of the next operator product) in one launch
// stage (scal_stage_doubles() doubles, may be null): scratch of the multi-block first reduction stage for long lists
void minres_scal21(hipStream_t st, int nb, MinresState* s, const DotParts& d2, const DotParts& d1, double* stage = nullptr);
size_t scal_stage_doubles();

// ---- k_fields.hip
// realization b of the batch = generator realization first_id + b * id_stride
void normal_fill(hipStream_t st, int n, int nbatch, uint64_t seed, uint64_t first_id, uint32_t stream, double mean,
                 double sigma, double* out, uint64_t id_stride = 1);
// out[i*nb+k] = scale * in[k*n+i] * (w ? w[i] : 1)
void interleave(hipStream_t st, int nb, int n, const double* in, const double* w, double scale, double* out,
                const int* src = nullptr);
// out[i*nb+k] = scale * v[k*n+i] * (s ? s[k*n+i] : 1) * (rowscale ? rowscale[i] : 1)   (seed of Eval's adjoint)
void seed_interleave(hipStream_t st, int nb, int n, const double* v, const double* s, const double* rowscale, double scale,
                     double* out);
// out[k*m+i] = post(rowscale[i] * in[(idx?idx[i]:i)*nb + k])
void deinterleave(hipStream_t st, int nb, int m, const double* in, const int* idx, const double* rowscale, bool do_exp,
                  double* out);
void broadcast(hipStream_t st, int nb, int n, const double* a, double* out);

// ---- k_darcy.hip
void darcy_coef(hipStream_t st, int nb, int n, const double* kfield, bool k_divides, double* coef);
void darcy_assemble(hipStream_t st, int nb, const SellView& Mp, const int* slot_src, const int* c_ptr, const int* c_elem,
                    const double* c_val, const double* coef, const unsigned char* ess, const double* ess_data,
                    const double* rhs0, double* mvals, double* diag, double* l1inv, double* rhs_bc);
// y = M(k) x1 + A2 x2 over the same rows with M(k) element-grouped (the u-rows [M(k) | B^T] of the Darcy operator);
// dot_partial != nullptr: partials of <dot_with, y>.  Returns the partial-block count.
int eg_pair_spmm(hipStream_t st, int nb, const EgView& M, const double* coef, const double* x1, const SellView& A2,
                 const double* x2, double* y, double* dot_partial, const double* dot_with);
int eg_pair_spmm_z(hipStream_t st, int nb, const EgView& M, const double* coef, zvec x1, const SellView& A2,
                   zvec x2, double* y, double* dot_partial, zvec dot_with);
// one-pass degree-2 Chebyshev polynomial of D^-1 M(k) from a zero guess (see sell_poly2_kernel) on the element-grouped
// matrix: xout = dinv (c0 r - c1 M(k) (dinv r)); dot_partial != nullptr: partials of <r, xout>
int eg_poly2(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, double* xout,
             double c0, double c1, double* dot_partial);
int eg_poly2_z(hipStream_t st, int nb, const EgView& M, const double* coef, const double* dinv, const double* r, zvec xout,
               double c0, double c1, double* dot_partial);

// per-realization Gershgorin scaling of dinv (batched values): afterwards spec(diag(dinv) S) lies in (0, 1] for every
// realization; gwork = kMaxBatch doubles of scratch
void gersh_scale_bv(hipStream_t st, int nb, const SellView& S, double* dinv, double* gwork);
void refresh(hipStream_t st, int nb, int64_t nslots, const int* ptr, const int* idx, const double* w, const double* src,
             bool recip, double* out);
// back-substitution of the hybridized Darcy system (DarcyHybrid; interleaved [row][nb] vectors)
void darcy_backsub_u(hipStream_t st, int nb, int n_u, const int* owner, const double* kappa, const double* U0, const double* ug,
                     const double* t, double* out);
void darcy_backsub_p(hipStream_t st, int nb, int n_p, const double* kappa, const double* P0, const double* zg, const double* t,
                     double* out);
void diag_inv(hipStream_t st, int nb, int n, const int* diag_slot, const double* vals, double* dinv);

// Per-element mass sensitivity (darcy_gradient.hip): out[b n_elem + e] = f(k[b n_elem + e]) sum_a lam[faces_e(a)][b]
// (sum_a' M_e[a][a'] x[faces_e(a')][b]), f = -c'(k) (+1/k^2 with k_divides, -1 otherwise; times k with wrt_log).  faces / me:
// element-major in slices of 64 elements, column-major inside a slice ([slice][a][64], [slice][a nfe + a'][64]); x, lam
// interleaved [row][nb]; kfield and out sample-major.  One fixed summation order per element (a outer, a' inner), no atomics:
// column b of the result does not depend on nb.
struct ElemMassView {
    int n_elem = 0, nslices = 0, nfe = 0;
    const int* faces = nullptr;
    const double* me = nullptr;
};
void darcy_mass_sensitivity(hipStream_t st, int nb, const ElemMassView& E, const double* kfield, const double* x,
                            const double* lam, bool k_divides, bool wrt_log, double* out);

// Tangent right-hand side (darcy_hessian.hip), the transpose of the above in (dk, lam):
// out[f][b] = sum_s ndc[elem_s(f)][b] (sum_a' w_s(f)[a'] x[cols_s(f)(a')][b]) on the rows f < n_rows, exactly 0 where ess[f];
// ndc = f(k) dk with the f above (= -dc).  Face-major in slices of 64 faces, column-major inside a slice: elem [slice][s][64]
// (-1: no such side; its cols are valid rows, its w zero), cols / w [slice][s nfe + a'][64].  x and out interleaved [row][nb],
// kfield and dk sample-major.  Sides in ascending element id, a' ascending, no atomics: column b does not depend on nb.
struct FaceMassView {
    int n_rows = 0, n_elem = 0, nslices = 0, nfe = 0, nside = 0;
    const int* elem = nullptr;
    const int* cols = nullptr;
    const double* w = nullptr;
};
void darcy_mass_tangent(hipStream_t st, int nb, const FaceMassView& F, const double* kfield, const double* dk, const double* x,
                        const unsigned char* ess, bool k_divides, bool wrt_log, double* out);

}  // namespace k
}  // namespace pmc

// ---- small-level V-cycle tail: every level from some level on fits one workgroup's LDS ---------------
namespace pmc {
struct TailLevelDev {
    int n, nslices;
    int nslots;                 // total SELL slots of the level (column stride of transposed per-realization values)
    const int* slice_off;
    const int* cols;
    const double* vals;         // shared [nslots], per-realization [nslots][nb] (bv 1) or transposed [nb][nslots] (bv 2)
    const double* vals_scaled;  // S D^-1 on the same pattern, may be null
    const double* dinv;         // [n], [n][nb] (bv 1) or [nb][n] (bv 2)
    int p_nslices, pt_nslices;  // transfers to / from the next coarser level (unused on the last tail level)
    const int *p_off, *p_cols, *pt_off, *pt_cols;
    const double *p_vals, *pt_vals;
    double lmax;
    int last_degree;            // > 0: this level ends the recursion with a Chebyshev solve of that degree
    double last_ratio;
    int lds_off;                // offset (in doubles) of this level's [r | x | d] block
    // last tail level only, may be null: the dense inverse of its (shared-value, symmetric) operator, n x n - the recursion
    // then ends with x = A^-1 r in one pass instead of a many-step Chebyshev solve whose every step re-reads the matrix behind
    // two barriers (a 64-row level with 30 entries per row: ~40 of the tail's 146 us per cycle, all of it latency)
    const double* ainv;
};
static constexpr size_t kTailLdsDoubles = (160 * 1024 - 1024) / 8;
struct TailParams {
    int nlev, bv, smooth_degree;
    double smooth_ratio;
    TailLevelDev lev[8];
};
// Everything the persistent small-level solver of the sampler needs (device pointers; by value in the kernel arguments)
struct MiniSamplerParams {
    int n_u, n_s;
    const int *a_off, *a_cols;      // block operator A (SELL-64, shared values)
    const double* a_vals;
    const int *m_off, *m_cols;      // M with column-scaled values M D^-1 and the l1 inverse: one-pass degree-2 polynomial
    const double *m_scaled, *m_dinv;
    double mc0, mc1;
    const TailParams* tail;         // V-cycle of the Schur block from this level on, all in LDS
    int max_iter;
    double rel_tol, abs_tol;
    int x_row0, x_nrows;            // maintained rows of the solution
    size_t scratch_per_col;         // doubles of scratch per realization: 5 n + 3 x_nrows
};
// ---- k_tail.hip
namespace k {
// Whole preconditioned MINRES solves of nb realizations, one workgroup each (see mini_sampler_kernel).  b, x: interleaved
// [row][nb] vectors as in minres_solve; stats: nb device entries.
void mini_sampler_solve(hipStream_t st, int nb, const MiniSamplerParams& P, size_t lds_doubles, const double* b, double* x,
                        bool zero_guess, double* scratch, pmc_stats* stats);
// One workgroup per batch column runs the whole V-cycle over the tail levels in LDS.  r, xout: interleaved
// vectors of the first tail level.  dot_partial != nullptr: writes <r, xout> per column as ONE partial block.
// out32 / in32: xout / r point at fp32 storage
int mg_tail(hipStream_t st, int nb, const TailParams* dev_params, size_t lds_doubles, const double* r, double* xout,
            double* dot_partial, bool out32 = false, bool in32 = false);
inline int mg_tail_z(hipStream_t st, int nb, const TailParams* dev_params, size_t lds_doubles, const double* r, zvec xout,
                     double* dot_partial) {
    return mg_tail(st, nb, dev_params, lds_doubles, r, xout.as<double>(), dot_partial, xout.f32);
}
// x = ainv r, ainv dense n x n row-major (symmetric), r / x interleaved [row][nb] in the same storage, nb <= 8 (see
// dense_apply_kernel)
void dense_apply(hipStream_t st, int nb, int n, const double* ainv, zvec r, zvec x);
// out[k][i] = in[i][k]: per-realization values of a small level re-laid column-major for the tail kernel, whose
// workgroup k then streams only its own realization's values
void transpose_bv(hipStream_t st, int nb, size_t count, const double* in, double* out);
void transpose_bv32(hipStream_t st, int nb, size_t count, const float* in, double* out);   // fp32 source
}  // namespace k
}  // namespace pmc

// SPDE Matérn sampler on the device: PDESampler / EmbeddedPDESampler / L2ProjectionPDESampler
// ::Sample and ::Eval (reference: src/PDESampler.cpp:336-535, src/EmbeddedPDESampler.cpp:438-563,
// src/L2ProjectionPDESampler.cpp:621-757).
#include <atomic>
#include <algorithm>
#include <cmath>

#include <cstdlib>
#include <cstring>

#include "handles.hpp"

namespace pmc {

// PMC_DIAG_LAST=0 builds the block operator in plain CSR order (A/B switch for the diagonal-last fused dot)
static bool diag_last_on() {
    static const bool v = [] {
        const char* e = lab_env("PMC_DIAG_LAST");
        return !e || atoi(e) != 0;
    }();
    return v;
}


// S = diag_add + B diag(dM)^-1 B^T as host CSR (setup).  B has its essential columns removed.
HostCsr schur_host(const HostCsr& B, const HostCsr& Bt, const std::vector<double>& dM, const double* diag_add) {
    HostCsr S;
    S.nrows = S.ncols = B.nrows;
    S.rowptr.assign(B.nrows + 1, 0);
    std::vector<int> marker(B.nrows, -1);
    std::vector<std::pair<int, double>> row;
    for (int e = 0; e < B.nrows; ++e) {
        row.clear();
        auto add = [&](int c, double v) {
            if (marker[c] < 0) { marker[c] = (int)row.size(); row.emplace_back(c, v); }
            else row[marker[c]].second += v;
        };
        add(e, diag_add ? diag_add[e] : 0.0);
        for (int p = B.rowptr[e]; p < B.rowptr[e + 1]; ++p) {
            const int f = B.colind[p];
            const double w = B.vals[p] / dM[f];
            for (int q = Bt.rowptr[f]; q < Bt.rowptr[f + 1]; ++q) add(Bt.colind[q], w * Bt.vals[q]);
        }
        std::sort(row.begin(), row.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (auto& cv : row) { S.colind.push_back(cv.first); S.vals.push_back(cv.second); marker[cv.first] = -1; }
        S.rowptr[e + 1] = (int)S.colind.size();
    }
    return S;
}

// device V-cycle levels of an algebraic hierarchy (setup)
struct AggSegments {   // agg_pack_rows' tables of the finest level (empty: the restriction stays a product with P^T)
    std::vector<int> ptr, cid, pos;
};
// inv = S^-1 (dense, row-major, exactly symmetric) of a small SPD operator by Cholesky; false when S is not numerically SPD
bool spd_dense_inverse(const HostCsr& S, std::vector<double>& inv) {
    const int n = S.nrows;
    std::vector<double> a((size_t)n * n, 0.0);
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int p = S.rowptr[i]; p < S.rowptr[i + 1]; ++p) a[(size_t)i * n + S.colind[p]] = S.vals[p];
    for (int j = 0; j < n; ++j) {   // a = L L^T (lower, in place)
        double dj = a[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) dj -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
        if (!(dj > 0.0) || !std::isfinite(dj)) return false;
        const double l = std::sqrt(dj);
        a[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double v = a[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) v -= a[(size_t)i * n + k] * a[(size_t)j * n + k];
            a[(size_t)i * n + j] = v / l;
        }
    }
    std::vector<double> y(n);
    for (int c = 0; c < n; ++c) {          // column c of the inverse: L y = e_c, L^T x = y
        for (int i = 0; i < c; ++i) y[i] = 0.0;
        for (int i = c; i < n; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) v -= a[(size_t)i * n + k] * y[k];
            y[i] = v / a[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = y[i];
            for (int k = i + 1; k < n; ++k) v -= a[(size_t)k * n + i] * inv[(size_t)k * n + c];
            inv[(size_t)i * n + c] = v / a[(size_t)i * n + i];
        }
    }
    for (int i = 0; i < n; ++i)             // exactly symmetric (the kernels read it either way round)
        for (int j = 0; j < i; ++j) {
            const double v = 0.5 * (inv[(size_t)i * n + j] + inv[(size_t)j * n + i]);
            inv[(size_t)i * n + j] = inv[(size_t)j * n + i] = v;
        }
    return true;
}

static std::unique_ptr<Multigrid> build_chain(const std::vector<AmgLevelHost>& lv, const pmc_solver_opts& o, hipStream_t st,
                                              double ratio_scale = 1.0, bool f32_any_injection = false,
                                              const std::vector<AggSegments>* segs = nullptr) {
    std::unique_ptr<Multigrid> mg(new Multigrid());
    mg->smooth_degree = o.mg_smooth_degree;
    mg->smooth_ratio = ratio_scale * o.mg_smooth_ratio;
    mg->coarse_degree = o.mg_coarse_degree;
    mg->coarse_ratio = o.mg_coarse_ratio;
    mg->f32_intermediates = o.precond_storage != PMC_STORAGE_FP64;
    mg->f32_any_injection = f32_any_injection;
    mg->L.resize(lv.size());
    for (size_t l = 0; l < lv.size(); ++l) {
        MgLevel& m = mg->L[l];
        const HostCsr& S = lv[l].S;
        m.n = S.nrows;
        m.bv = false;
        sell_build(m.S, S, true, true, st);
        std::vector<double> dS = csr_diag(S);
        double lo = 0.0;
        m.lmax = gershgorin_scaled(S, dS, &lo) * 1.0001;
        if (lo > 0.0 && (m.lmax / lo <= 3.5 || (m.n <= 4096 && m.lmax / lo <= 40.0))) {
            m.is_last = true;
            m.last_ratio = m.lmax / (lo * 0.999);
            const double sk = std::sqrt(m.last_ratio);
            const double sig = (sk - 1.0) / (sk + 1.0);
            m.last_degree = std::min(16, std::max(2, (int)std::ceil(std::log(2.0 / 0.02) / std::log(1.0 / sig))));
        }
        for (double& v : dS) v = 1.0 / v;
        m.dinv.upload(dS, st);
        m.vals_scaled.upload(sell_scaled_values(m.S, S, dS), st);
        PMC_HIP(hipStreamSynchronize(st));
        m.S.h_src.clear(); m.S.h_src.shrink_to_fit();
        m.S.h_cols.clear(); m.S.h_cols.shrink_to_fit();
        if (m.is_last) { mg->L.resize(l + 1); break; }
        if (l + 1 < lv.size()) {
            const HostCsr& P = lv[l].P;
            m.P_host = P;
            sell_build(m.P, P, true, false, st);
            sell_build(m.Pt, csr_transpose(P), true, false, st);
            // indicator prolongator (plain aggregation): the coarse correction is folded into the post-smoothing
            bool injection = true;
            std::vector<int> parent(P.nrows, 0);
            for (int i = 0; i < P.nrows && injection; ++i) {
                injection = (P.rowptr[i + 1] - P.rowptr[i] == 1) && P.vals[P.rowptr[i]] == 1.0;
                if (injection) parent[i] = P.colind[P.rowptr[i]];
            }
            if (injection) {
                sell_build(m.SP, csr_spgemm(S, P), true, false, st);
                m.parent.upload(parent, st);
                m.has_sp = true;
                if (segs && l < segs->size() && !(*segs)[l].ptr.empty()) {
                    m.seg_ptr.upload((*segs)[l].ptr, st);
                    m.seg_cid.upload((*segs)[l].cid, st);
                    m.seg_pos.upload((*segs)[l].pos, st);
                    m.p_agg = true;
                }
                PMC_HIP(hipStreamSynchronize(st));
            }
        }
    }
    // The coarsest level of such a hierarchy is tiny and comparatively dense (64 rows with ~30 entries each at 400 k multipliers):
    // its many-step Chebyshev solve was ~40 us of pure latency per cycle inside the LDS tail.  Up to 192 rows it is solved
    // exactly with a dense inverse computed here once (host, Cholesky on the SPD level operator).
    if (f32_any_injection && !mg->L.empty()) {
        const char* e = lab_env("PMC_TAIL_AINV");
        const int n = lv[mg->L.size() - 1].S.nrows;
        std::vector<double> inv;
        if (n >= 2 && n <= 192 && !(e && atoi(e) == 0) && spd_dense_inverse(lv[mg->L.size() - 1].S, inv)) {
            mg->L.back().ainv.upload(inv, st);
            PMC_HIP(hipStreamSynchronize(st));
        }
        // Launches of at most 8 realizations (one per call under the reference's serial manager) leave the cycle even earlier:
        // the first inner level of at most 768 rows is solved exactly by a multi-workgroup dense product (Multigrid::cycle)
        mg->dense_nb = 8;
        if (const char* d = lab_env("PMC_DENSE_NB")) mg->dense_nb = atoi(d);
        const char* spl = lab_env("PMC_ROW_SPLIT");
        for (size_t l = 1; mg->dense_nb > 0 && l < mg->L.size(); ++l) {
            const int m = lv[l].S.nrows;
            if (m > 768) {
                // ... and the inner levels above it run row-split: their rows carry 17-40 entries, one wavefront walks a slice of
                // 64 of them as ONE chain of dependent gathers (a 5 k-row level: 80 wavefronts, 9-12 us per kernel whatever the
                // width).  Pieces of about 5 entries; levels of up to 65 536 rows (the split copy is extra memory and setup).
                MgLevel& ml = mg->L[l];
                if (m > 65536 || !ml.has_sp || ml.p_agg || ml.p_oct || (spl && atoi(spl) == 0)) continue;
                auto pieces = [](const HostCsr& A) {
                    const double avg = (double)A.rowptr[A.nrows] / std::max(1, A.nrows);
                    int sl = 0;
                    while (sl < 4 && avg / (1 << sl) > 6.0) ++sl;
                    return sl;
                };
                std::vector<double> dS = csr_diag(lv[l].S);
                for (double& v : dS) v = 1.0 / v;
                ml.split_log2 = pieces(lv[l].S);
                if (ml.split_log2 > 0) {
                    const HostCsr Ssp = csr_split_rows(lv[l].S, ml.split_log2);
                    sell_build(ml.S_split, Ssp, true, true, st);
                    ml.scaled_split.upload(sell_scaled_values(ml.S_split, Ssp, dS), st);
                    PMC_HIP(hipStreamSynchronize(st));
                    ml.S_split.h_src.clear(); ml.S_split.h_src.shrink_to_fit();
                    ml.S_split.h_cols.clear(); ml.S_split.h_cols.shrink_to_fit();
                    const HostCsr SPh = csr_spgemm(lv[l].S, lv[l].P);
                    ml.sp_split_log2 = pieces(SPh);
                    if (ml.sp_split_log2 > 0) {
                        sell_build(ml.SP_split, csr_split_rows(SPh, ml.sp_split_log2), true, false, st);
                        PMC_HIP(hipStreamSynchronize(st));
                    }
                }
                continue;
            }
            if (m > 192 && spd_dense_inverse(lv[l].S, inv)) {
                mg->L[l].dense_inv.upload(inv, st);
                PMC_HIP(hipStreamSynchronize(st));
            }
            break;
        }
    }
    mg->build_tails(st);
    return mg;
}

std::unique_ptr<Multigrid> build_sa_chain(const HostCsr& K, const std::vector<double>& w, const pmc_solver_opts& o,
                                          hipStream_t st) {
    return build_chain(sa_hierarchy(K, w, /*passes=*/2, /*theta=*/0.25, /*min_size=*/256, /*max_levels=*/14), o, st);
}

static std::vector<double> l1_inverse(const HostCsr& M) {
    std::vector<double> d(M.nrows);
    for (int i = 0; i < M.nrows; ++i) {
        double s = 0.0;
        for (int p = M.rowptr[i]; p < M.rowptr[i + 1]; ++p) s += std::fabs(M.vals[p]);
        PMC_REQUIRE(s > 0.0, "mass matrix has an empty row");
        d[i] = 1.0 / s;
    }
    return d;
}

Sampler::Sampler(Ctx& c, int nlevels_, int n_mc_, const pmc_sampler_level* in, double alpha_, double g_, bool logn,
                 const pmc_solver_opts& o)
    : ctx(c), nlevels(nlevels_), n_mc(n_mc_), alpha(alpha_), g(g_), lognormal(logn), opts(o) {
    PMC_REQUIRE(nlevels >= 1 && n_mc >= 1 && n_mc <= nlevels, "sampler: need 1 <= n_mc_levels <= nlevels");
    PMC_REQUIRE(in != nullptr, "sampler: levels is NULL");
    PMC_REQUIRE(alpha > 0.0, "sampler: alpha must be positive");
    ctx.activate();
    hipStream_t st = ctx.stream;
    lv.resize(nlevels);
    mg.L.resize(nlevels);
    mg.smooth_degree = o.mg_smooth_degree;
    mg.smooth_ratio = o.mg_smooth_ratio;
    mg.coarse_degree = o.mg_coarse_degree;
    mg.coarse_ratio = o.mg_coarse_ratio;
    mg.f32_intermediates = o.precond_storage != PMC_STORAGE_FP64;
    for (int l = 0; l < nlevels; ++l) {
        const pmc_sampler_level& L = in[l];
        SamplerLevel& d = lv[l];
        PMC_REQUIRE(L.n_u > 0 && L.n_s > 0, "sampler level: empty block");
        d.n_u = L.n_u;
        d.n_s = L.n_s;
        HostCsr M = csr_from_c(L.M, true, "sampler M");
        HostCsr B = csr_from_c(L.B, true, "sampler B");
        PMC_REQUIRE(M.nrows == L.n_u && M.ncols == L.n_u, "sampler M: wrong shape");
        PMC_REQUIRE(B.nrows == L.n_s && B.ncols == L.n_u, "sampler B: wrong shape");
        PMC_REQUIRE(L.w_diag != nullptr, "sampler w_diag is NULL");
        csr_sort_rows(M);
        csr_sort_rows(B);
        HostCsr Bt = csr_transpose(B);
        std::vector<double> maw(L.n_s), wsq(L.n_s), aw(L.n_s);
        for (int i = 0; i < L.n_s; ++i) {
            PMC_REQUIRE(L.w_diag[i] > 0.0, "sampler w_diag must be positive");
            maw[i] = -alpha * L.w_diag[i];
            aw[i] = alpha * L.w_diag[i];
            wsq[i] = std::sqrt(L.w_diag[i]);
        }
        if (l == 0) w0_host.assign(L.w_diag, L.w_diag + L.n_s);
        HostCsr A = csr_block2x2(M, Bt, B, maw.data());
        d.nnz = A.nnz();
        sell_build(d.A, A, true, false, st, diag_last_on());
        sell_schedule_two_blocks(d.A, L.n_u, st, &A);
        sell_build(d.M, M, true, true, st);
        std::vector<double> dM = csr_diag(M);
        for (double v : dM) PMC_REQUIRE(v > 0.0, "sampler M must have a positive diagonal");
        {
            std::vector<double> l1 = l1_inverse(M);
            d.ratio_M = o.cheb_ratio_M > 1.0 ? o.cheb_ratio_M : mass_block_ratio(M, l1);
            d.dinvM.upload(l1, st);
            d.M_scaled.upload(sell_scaled_values(d.M, M, l1), st);
            PMC_HIP(hipStreamSynchronize(st));
            d.M.h_src.clear(); d.M.h_src.shrink_to_fit();
            d.M.h_cols.clear(); d.M.h_cols.shrink_to_fit();
        }
        d.w_sqrt.upload(wsq, st);
        // Schur complement level
        std::vector<double> dMs(dM);
        for (double& v : dMs) v /= o.schur_scale;
        HostCsr S = schur_host(B, Bt, dMs, aw.data());
        if (l < n_mc && o.mg_coarsening != 0) {
            // internal algebraic hierarchy for this Monte Carlo level (always when asked for, on stretched cells in auto mode)
            HostCsr K = schur_host(B, Bt, dMs, nullptr);
            if (l == 0) anisotropy = csr_anisotropy(K);
            if (o.mg_coarsening == 1 || anisotropy > 10.0) {
                if ((int)amg.size() < n_mc) amg.resize(n_mc);
                amg[l] = build_sa_chain(K, aw, o, st);
            }
        }
        MgLevel& m = mg.L[l];
        m.n = L.n_s;
        m.bv = false;
        sell_build(m.S, S, true, true, st);
        std::vector<double> dS = csr_diag(S);
        double lo = 0.0;
        m.lmax = gershgorin_scaled(S, dS, &lo) * 1.0001;
        // reaction-dominated level (alpha |e| dominates the flux coupling): spec(D^-1 S) lies in the narrow
        // Gershgorin interval [lo, lmax]; a short Chebyshev polynomial on exactly that interval is an
        // (almost) exact solve, so the V-cycle stops here.
        // A small level (launch-latency bound below a few thousand rows) with a moderately narrow interval
        // is also solved in place by a longer polynomial instead of descending further.
        if (lo > 0.0 && (m.lmax / lo <= 3.5 || (L.n_s <= 4096 && m.lmax / lo <= 40.0))) {
            m.is_last = true;
            m.last_ratio = m.lmax / (lo * 0.999);
            const double sk = std::sqrt(m.last_ratio);
            const double sig = (sk - 1.0) / (sk + 1.0);
            m.last_degree = std::min(16, std::max(2, (int)std::ceil(std::log(2.0 / 0.02) / std::log(1.0 / sig))));
        }
        for (double& v : dS) v = 1.0 / v;
        m.dinv.upload(dS, st);
        m.vals_scaled.upload(sell_scaled_values(m.S, S, dS), st);
        PMC_HIP(hipStreamSynchronize(st));
        m.S.h_src.clear(); m.S.h_src.shrink_to_fit();
        m.S.h_cols.clear(); m.S.h_cols.shrink_to_fit();
        if (l + 1 < nlevels) {
            HostCsr P = csr_from_c(L.P, true, "sampler P");
            PMC_REQUIRE(P.nrows == L.n_s && P.ncols == in[l + 1].n_s, "sampler P: wrong shape");
            HostCsr Pt = csr_transpose(P);
            d.P_host = P;
            sell_build(m.P, P, true, false, st);
            sell_build(m.Pt, Pt, true, false, st);
            m.p_oct = csr_is_oct_injection(P);
            // injection-type prolongator (P0 on nested meshes): coarse correction folded into the post-smoothing
            bool injection = true;
            std::vector<int> parent(P.nrows, 0);
            for (int i = 0; i < P.nrows && injection; ++i) {
                injection = (P.rowptr[i + 1] - P.rowptr[i] == 1) && P.vals[P.rowptr[i]] == 1.0;
                if (injection) parent[i] = P.colind[P.rowptr[i]];
            }
            if (injection) {
                sell_build(m.SP, csr_spgemm(S, P), true, false, st);
                m.parent.upload(parent, st);
                m.has_sp = true;
            }
        }
        PMC_HIP(hipStreamSynchronize(st));
    }
    mg.build_tails(st);
    if (getenv("PMC_VERBOSE")) {
        for (int l = 0; l < nlevels; ++l) {
            const MgLevel& m = mg.L[l];
            fprintf(stderr, "[pmc] sampler level %d: n_u %d n_s %d ratio_M %.2f | S: lmax %.3f last %d (degree %d, ratio %.1f) "
                            "tail %s (%zu doubles) injection %d\n",
                    l, lv[l].n_u, lv[l].n_s, lv[l].ratio_M, m.lmax, (int)m.is_last, m.last_degree, m.last_ratio,
                    (l < (int)mg.tail.size() && mg.tail[l].p) ? "yes" : "no", l < (int)mg.tail_lds.size() ? mg.tail_lds[l] : 0,
                    (int)m.has_sp);
        }
    }
}

// Hybridized sampler (pmc_sampler_create_hybrid): the multiplier system H lambda = G f of every level, an aggregation
// multigrid on H as its preconditioner, and the element-local back-substitution s = z f - G^T lambda.
Sampler::Sampler(Ctx& c, int nlevels_, const pmc_hybrid_level* in, double alpha_, double g_, bool logn, const pmc_solver_opts& o)
    : ctx(c), nlevels(nlevels_), n_mc(nlevels_), alpha(alpha_), g(g_), lognormal(logn), opts(o), hybrid(true) {
    PMC_REQUIRE(nlevels >= 1, "hybrid sampler: need at least one level");
    PMC_REQUIRE(in != nullptr, "hybrid sampler: levels is NULL");
    PMC_REQUIRE(alpha > 0.0, "sampler: alpha must be positive");
    ctx.activate();
    hipStream_t st = ctx.stream;
    lv.resize(nlevels);
    mg.L.resize(nlevels);     // only the transfers between Monte Carlo levels live here
    amg.resize(nlevels);
    for (int l = 0; l < nlevels; ++l) {
        const pmc_hybrid_level& L = in[l];
        SamplerLevel& d = lv[l];
        PMC_REQUIRE(L.n_lambda > 0 && L.n_s > 0, "hybrid sampler level: empty block");
        PMC_REQUIRE(L.z_diag != nullptr && L.w_diag != nullptr, "hybrid sampler level: z_diag / w_diag is NULL");
        d.n_u = L.n_lambda;
        d.n_s = L.n_s;
        HostCsr H = csr_from_c(L.H, true, "hybrid H");
        HostCsr G = csr_from_c(L.G, true, "hybrid G");
        PMC_REQUIRE(H.nrows == L.n_lambda && H.ncols == L.n_lambda, "hybrid H: wrong shape");
        PMC_REQUIRE(G.nrows == L.n_lambda && G.ncols == L.n_s, "hybrid G: wrong shape");
        csr_sort_rows(H);
        csr_sort_rows(G);
        for (double v : csr_diag(H)) PMC_REQUIRE(v > 0.0, "hybrid H must have a positive diagonal");
        std::vector<double> zw(L.n_s);
        for (int i = 0; i < L.n_s; ++i) {
            PMC_REQUIRE(L.w_diag[i] > 0.0, "sampler w_diag must be positive");
            PMC_REQUIRE(L.z_diag[i] != 0.0, "hybrid z_diag must not vanish");
            zw[i] = L.z_diag[i] * std::sqrt(L.w_diag[i]);
        }
        if (l == 0) w0_host.assign(L.w_diag, L.w_diag + L.n_s);
        d.zw_sqrt.upload(zw, st);
        {
            std::vector<double> wsq(L.n_s);
            for (int i = 0; i < L.n_s; ++i) wsq[i] = std::sqrt(L.w_diag[i]);
            d.w_sqrt.upload(wsq, st);
        }
        d.nnz = H.nnz();
        // aggregates of ~9 rows per level (three matching passes + singletons joined): 19 -> 21 iterations at 400 k multipliers
        // against aggregates of ~4.4, but two kernel-launched levels above the LDS tail instead of four (measured, LAB_NOTES 9.11)
        int passes0 = 3, passes1 = 3;
        if (const char* e = lab_env("PMC_HYB_PASSES0")) passes0 = atoi(e);
        if (const char* e = lab_env("PMC_HYB_PASSES1")) passes1 = atoi(e);
        std::vector<AmgLevelHost> hier = agg_hierarchy(H, passes0, passes1, /*theta=*/0.25, /*min_size=*/256, /*max_levels=*/14);
        // The multipliers are internal unknowns: renumber them so that every aggregate of the finest level is a run of
        // consecutive rows inside one SELL slice - the restriction of the V-cycle's finest level is then taken by the residual
        // kernel itself (k::vc_residual_restrict_agg32).  H, G and the level's prolongator move to the new numbering; vectors
        // that cross the boundary in multiplier numbering (pmc_sampler_mult / _apply_operator / _apply_preconditioner) are
        // renumbered on the way in and out (lam_new2old / lam_old2new).
        // Levels below the finest are numbered by the library anyway: they are packed the same way (their restriction fused as
        // well), which renumbers the coarse ids the level above refers to.
        std::vector<AggSegments> segs(hier.size());
        // (product: the finest level only.  Packing the levels below as well re-pads their SELL slices - the LDS tail, which
        // holds them, went from 144 to 155 us per cycle - and the first coarse level's aggregates did not pack; LAB_NOTES 10.2)
        int pack_levels = (hier.size() >= 2 && o.precond_storage != PMC_STORAGE_FP64) ? 1 : 0;
        if (const char* e = lab_env("PMC_AGG_PACK")) pack_levels = std::min((int)hier.size() - 1, atoi(e));
        for (int pl = 0; pl < pack_levels; ++pl) {
            AggSegments sg;
            std::vector<int> new2old = agg_pack_rows(hier[(size_t)pl].P, sg.ptr, sg.cid, sg.pos);
            if (new2old.empty()) continue;
            std::vector<int> old2new(new2old.size());
            for (size_t i = 0; i < new2old.size(); ++i) old2new[(size_t)new2old[i]] = (int)i;
            hier[(size_t)pl].P = csr_permute(hier[(size_t)pl].P, new2old, true, false);
            if (pl == 0) {
                H = csr_permute(H, new2old, true, true);
                G = csr_permute(G, new2old, true, false);
                hier[0].S = H;
                d.lam_new2old.upload(new2old, st);
                d.lam_n2o_host = new2old;
                d.lam_old2new.upload(old2new, st);
            } else {
                hier[(size_t)pl].S = csr_permute(hier[(size_t)pl].S, new2old, true, true);
                // the level above names these rows as its coarse ids: prolongator columns and segment targets follow
                hier[(size_t)pl - 1].P = csr_permute(hier[(size_t)pl - 1].P, new2old, false, true);
                for (int& c : segs[(size_t)pl - 1].cid) c = old2new[(size_t)c];
            }
            segs[(size_t)pl] = std::move(sg);
        }
        sell_build(d.A, H, true, false, st, diag_last_on());
        sell_build(d.Gl, csr_transpose(G), true, false, st);
        for (int i = 0; i < G.nrows; ++i)
            for (int p = G.rowptr[i]; p < G.rowptr[i + 1]; ++p) G.vals[p] /= L.z_diag[G.colind[p]];
        sell_build(d.Gz, G, true, false, st);
        PMC_HIP(hipStreamSynchronize(st));
        // the aggregation hierarchy of H smooths on [lmax / (2 r), lmax], r = mg_smooth_ratio - twice the interval ratio of the
        // Schur-complement hierarchies (measured at 400 k multipliers, 4 lanes x 32: r = 8 2 630, 12 ... 30 2 900, 50 2 650
        // samples/s; 21 -> 20 iterations)
        amg[l] = build_chain(hier, o, st, /*ratio_scale=*/2.0, /*f32_any_injection=*/true, &segs);
        amg[l]->tail_later_nb = 8;
        if (const char* e = lab_env("PMC_TAIL_LATER_NB")) amg[l]->tail_later_nb = atoi(e);
        mg.L[l].n = L.n_s;
        if (l + 1 < nlevels) {
            HostCsr P = csr_from_c(L.P, true, "sampler P");
            PMC_REQUIRE(P.nrows == L.n_s && P.ncols == in[l + 1].n_s, "sampler P: wrong shape");
            d.P_host = P;
            sell_build(mg.L[l].P, P, true, false, st);
            HostCsr Pt = csr_transpose(P);
            sell_build(mg.L[l].Pt, Pt, true, false, st);
            // the last restriction of a finer xi lands on z f of the coarser level: rows scaled by that level's z
            for (int i = 0; i < Pt.nrows; ++i)
                for (int p = Pt.rowptr[i]; p < Pt.rowptr[i + 1]; ++p) Pt.vals[p] *= in[l + 1].z_diag[i];
            sell_build(lv[l + 1].Ptz, Pt, true, false, st);
        }
        PMC_HIP(hipStreamSynchronize(st));
        if (getenv("PMC_VERBOSE")) {
            const Multigrid& h = *amg[l];
            fprintf(stderr, "[pmc] hybrid sampler level %d: n_lambda %d n_s %d nnz(H) %lld | V-cycle levels", l, d.n_u, d.n_s,
                    (long long)d.nnz);
            for (size_t q = 0; q < h.L.size(); ++q)
                fprintf(stderr, " %d%s%s", h.L[q].n, h.L[q].has_sp ? "i" : "", (q < h.tail.size() && h.tail[q].p) ? "t" : "");
            fprintf(stderr, "\n");
            for (size_t q = 0; q < h.L.size(); ++q)
                fprintf(stderr, "[pmc]   V-cycle level %zu: S %lld entries in %lld slots, S P %lld in %lld, lmax %.3f\n", q,
                        (long long)h.L[q].S.nnz, (long long)h.L[q].S.nslots, (long long)h.L[q].SP.nnz, (long long)h.L[q].SP.nslots,
                        h.L[q].lmax);
        }
    }
}

void Sampler::set_projection(int level, int kind, const pmc_csr* Gt, const int32_t* idx, const double* inv_w,
                             int orig_size) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "set_projection: level out of range");
    PMC_REQUIRE(cond == nullptr, "set_projection: a conditioner is attached (pmc_sampler_set_conditioner); detach it first");
    SamplerLevel& d = lv[level];
    ctx.activate();
    hipStream_t st = ctx.stream;
    d.has_adj = false;   // the adjoint's transposed output map is rebuilt at the next pmc_sampler_eval_adjoint
    if (kind == PMC_PROJ_NONE) {
        d.proj = PMC_PROJ_NONE;
        d.out_size = d.n_s;
    } else if (kind == PMC_PROJ_GATHER) {
        PMC_REQUIRE(idx != nullptr && orig_size > 0 && orig_size <= d.n_s, "set_projection: bad gather arguments");
        for (int i = 0; i < orig_size; ++i) PMC_REQUIRE(idx[i] >= 0 && idx[i] < d.n_s, "set_projection: gather index out of range");
        d.gather.upload(idx, orig_size, st);
        d.proj = kind;
        d.out_size = orig_size;
    } else if (kind == PMC_PROJ_L2) {
        PMC_REQUIRE(Gt != nullptr && inv_w != nullptr, "set_projection: Gt / inv_w is NULL");
        HostCsr G = csr_from_c(*Gt, true, "Gt");
        PMC_REQUIRE(G.ncols == d.n_s && G.nrows == orig_size && orig_size > 0, "set_projection: Gt has the wrong shape");
        sell_build(d.Gt, G, true, false, st);
        d.inv_w.upload(inv_w, orig_size, st);
        d.proj = kind;
        d.out_size = orig_size;
    } else {
        throw Error(PMC_ERR_INVALID, "set_projection: unknown kind");
    }
    PMC_HIP(hipStreamSynchronize(st));
}

void Sampler::ensure(int level, int nb) {
    size_t nmax = 0, smax = 0;
    for (int l = 0; l <= level; ++l) {
        nmax = std::max(nmax, (size_t)lv[l].n_u + lv[l].n_s);   // hybrid: multipliers in rhs / sol, z f and the field behind
        smax = std::max(smax, (size_t)lv[l].n_s);
    }
    for (int l = level; l < nlevels; ++l) smax = std::max(smax, (size_t)lv[l].n_s);
    // L2-projected samplers return fields on the ORIGINAL mesh, which may have more elements than the enlarged one
    for (int l = 0; l < n_mc; ++l) smax = std::max(smax, (size_t)lv[l].out_size);
    rhs.ensure(nmax * nb);
    sol.ensure(nmax * nb);
    tA.ensure(smax * nb);
    tB.ensure(smax * nb);
    if (!hybrid) {   // scratch of the M-block polynomial
        cx.ensure((size_t)lv[level].n_u * nb);
        cd.ensure((size_t)lv[level].n_u * nb);
    }
    stage_in.ensure(smax * nb);
    stage_out.ensure(smax * nb);
    stage_emb.ensure(smax * nb);
}

void Sampler::sample(int level, uint64_t first_id, int nbatch, double* xi, int memspace) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "Sample: level out of range");
    PMC_REQUIRE(nbatch >= 1 && xi != nullptr, "Sample: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const int n = lv[level].n_s;
    if (memspace == PMC_MEM_DEVICE) {
        k::normal_fill(st, n, nbatch, ctx.seed, ctx.stream_id(first_id), (uint32_t)level, 0.0, 1.0, xi, (uint64_t)ctx.nparts);
    } else {
        DevBuf<double> tmp((size_t)n * nbatch);
        k::normal_fill(st, n, nbatch, ctx.seed, ctx.stream_id(first_id), (uint32_t)level, 0.0, 1.0, tmp.p, (uint64_t)ctx.nparts);
        PMC_HIP(hipMemcpyAsync(xi, tmp.p, sizeof(double) * n * nbatch, hipMemcpyDeviceToHost, st));
        PMC_HIP(hipStreamSynchronize(st));
    }
}

static std::atomic<uint64_t> g_fused_field_evals{0};
uint64_t fused_field_eval_count() { return g_fused_field_evals.load(std::memory_order_relaxed); }

// Interleaved vectors from level `from` to level `to` through the transfer operators of the caller's hierarchy: restriction
// with P^T down the levels (from < to; `last`, when given, takes the place of the last P^T) or prolongation with P up them
// (from > to).  The products ping-pong between tA and tB; the last one goes to `dst`, or stays in scratch when dst is NULL.
// Returns where the result is: src itself when from == to.
const double* Sampler::level_walk(int nb, int from, int to, const double* src, double* dst, const Sell* last) {
    hipStream_t st = ctx.stream;
    const int step = from < to ? 1 : -1;
    const double* cur = src;
    for (int l = from; l != to; l += step) {
        const bool final_step = l + step == to;
        const Sell& T = step < 0 ? mg.L[l - 1].P : (final_step && last) ? *last : mg.L[l].Pt;
        double* out = (final_step && dst) ? dst : (cur == tA.p ? tB.p : tA.p);
        k::spmm(st, nb, view(T), cur, out, false, nullptr, nullptr);
        cur = out;
    }
    return cur;
}

// The right-hand side of the multiplier system of `level`, Gz fz, as the kernel that writes it: the product is handed to the
// solve, which has it write the first Lanczos vector and its fp32 copy where it can (RhsFn); nothing reads the multiplier
// rows of rhs after the solve, only fz behind them
RhsFn Sampler::multiplier_rhs(int level, const double* fz) {
    const SellView Gzv = view(lv[level].Gz);
    RhsFn make_rhs;
    make_rhs.store = rhs.p;
    make_rhs.write = [Gzv, fz](const Lanes& L, int nb_, double* y, float* y32) {
        if (y32) k::spmm_store32(L.main, nb_, Gzv, fz, y, y32);
        else k::spmm(L.main, nb_, Gzv, fz, y, false, nullptr, nullptr);
    };
    return make_rhs;
}

void Sampler::eval_chunk(int level, int xi_level, int nb, const double* xi_d, double* s_d, const double* init_d,
                         int init_level, bool use_init, double* emb_d, pmc_stats* stats) {
    hipStream_t st = ctx.stream;
    SamplerLevel& d = lv[level];
    const int n_u = d.n_u, n_s = d.n_s;
    ensure(level, nb);
    if (stats) ctx.phase_mark(0);
    // rhs / sol hold [u- resp. lambda-sized vector | s-sized vector]: n_u + n_s rows each.
    // saddle-point: rhs_s = -g W^{1/2} xi on xi_level, restricted with Ps^T (PDESampler.cpp:423-438); rhs_u = 0 (:441-442).
    // hybridized: rhs_s = fz = z f with f the same vector, the last restriction (or the scale, without one) landing on z f
    // directly; rhs = G f = Gz fz; lambda = H^-1 rhs; s = fz - G^T lambda
    if (!hybrid) k::fill(st, (size_t)n_u * nb, rhs.p, 0.0);
    double* rhs_s = rhs.p + (size_t)n_u * nb;
    const double* scale = (hybrid && xi_level == level) ? d.zw_sqrt.p : lv[xi_level].w_sqrt.p;
    double* xi_il = xi_level == level ? rhs_s : tA.p;
    k::interleave(st, nb, lv[xi_level].n_s, xi_d, scale, -g, xi_il);
    level_walk(nb, xi_level, level, xi_il, rhs_s, hybrid ? &d.Ptz : nullptr);
    if (hybrid) {
        const double* fz = rhs_s;
        const RhsFn make_rhs = multiplier_rhs(level, fz);
        if (stats) ctx.phase_mark(1);
        solve_system(level, nb, true, 0, n_u, stats, &make_rhs);
        const SellView Glv = view(d.Gl);
        // the field as the caller gets it, from the back-substitution itself: identity output map, and neither an embedded
        // copy nor a conditioner that would want the interleaved field
        if (d.proj == PMC_PROJ_NONE && !cond && !emb_d && !Glv.bv) {
            k::residual_samples(st, nb, Glv, fz, sol.p, lognormal, s_d);
            g_fused_field_evals.fetch_add(1, std::memory_order_relaxed);
            return;
        }
        double* field = sol.p + (size_t)n_u * nb;
        k::residual(st, nb, Glv, fz, sol.p, field);
    } else {
        if (use_init) {   // initial guess (:498-515)
            double* sol_s = sol.p + (size_t)n_u * nb;
            k::fill(st, (size_t)n_u * nb, sol.p, 0.0);
            double* init_il = init_level == level ? sol_s : tA.p;
            k::interleave(st, nb, lv[init_level].n_s, init_d, nullptr, 1.0, init_il);
            level_walk(nb, init_level, level, init_il, sol_s);
        }
        if (stats) ctx.phase_mark(1);
        // only the s-block of the solution is ever read (PDESampler.cpp:526): maintain only those rows
        solve_system(level, nb, !use_init, n_u, n_s, stats);
    }
    // outputs (:526-533 and the embedded variants' maps)
    const double* sol_s = sol.p + (size_t)n_u * nb;
    if (d.proj == PMC_PROJ_NONE) {
        // with a conditioner the Gaussian field lands in s_d and is updated in place, exp() fused into that kernel's store
        k::deinterleave(st, nb, n_s, sol_s, nullptr, nullptr, lognormal && !cond, s_d);
        if (cond) cond->apply_device(level, nb, s_d, nullptr, s_d, lognormal, cond_tangent_width > 0, cond_tangent_width);
    } else if (d.proj == PMC_PROJ_GATHER) {
        k::deinterleave(st, nb, d.out_size, sol_s, d.gather.p, nullptr, lognormal, s_d);
    } else {
        k::spmm(st, nb, view(d.Gt), sol_s, tA.p, false, nullptr, nullptr);
        k::deinterleave(st, nb, d.out_size, tA.p, nullptr, d.inv_w.p, lognormal, s_d);
    }
    if (emb_d) k::deinterleave(st, nb, n_s, sol_s, nullptr, nullptr, false, emb_d);
}

// invA[level]->Mult(rhs, sol) (PDESampler.cpp:397,521): preconditioned MINRES on the interleaved member vectors rhs -> sol
// for nb realizations; rows [x_row0, x_row0 + x_nrows) of the solution are maintained.  The caller has marked phase 1.
void Sampler::solve_system(int level, int nb, bool zero_guess, int x_row0, int x_nrows, pmc_stats* stats, const RhsFn* rhs_fn,
                           uint64_t key_salt) {
    hipStream_t st = ctx.stream;
    SamplerLevel& d = lv[level];
    const int n_u = d.n_u, n_s = d.n_s, n = (int)system_rows(level);
    Multigrid* mgp = &cycle_mg(level);
    const int mg_l0 = cycle_hierarchy(level).first;
    // small level whose whole Schur V-cycle fits the LDS tail: one persistent workgroup per realization runs the entire
    // MINRES solve (k::mini_sampler_solve) instead of ~7 kernel launches per iteration
    static const int mini_env = [] {      // tuning override of opts.mini_max_rows
        const char* e = lab_env("PMC_MINI_MAX_ROWS");
        return e ? atoi(e) : -1;
    }();
    const int mini_max_rows = mini_env >= 0 ? mini_env : opts.mini_max_rows;
    const int degM = degree_M(level);
    const bool mini = !hybrid && n <= mini_max_rows && degM == 2 && opts.use_graph == 0 &&
                      mg_l0 < (int)mgp->tail.size() && mgp->tail[mg_l0].p != nullptr;
    if (mini) {
        MiniSamplerParams mp{};
        mp.n_u = n_u;
        mp.n_s = n_s;
        mp.a_off = d.A.slice_off.p; mp.a_cols = d.A.cols.p; mp.a_vals = d.A.vals.p;
        mp.m_off = d.M.slice_off.p; mp.m_cols = d.M.cols.p; mp.m_scaled = d.M_scaled.p; mp.m_dinv = d.dinvM.p;
        cheb2_coefficients(1.0, d.ratio_M, &mp.mc0, &mp.mc1);
        mp.tail = mgp->tail[mg_l0].p;
        mp.max_iter = opts.max_iter;
        mp.rel_tol = opts.rel_tol;
        mp.abs_tol = opts.abs_tol;
        mp.x_row0 = x_row0;
        mp.x_nrows = x_nrows;
        mp.scratch_per_col = (size_t)5 * n + (size_t)3 * x_nrows;
        mini_scratch.ensure(mp.scratch_per_col * nb);
        mini_stats.ensure(kMaxBatch);
        k::mini_sampler_solve(st, nb, mp, mgp->tail_lds[mg_l0], rhs.p, sol.p, zero_guess, mini_scratch.p, mini_stats.p);
        count_solve_path(PMC_PATH_MINI);
        if (stats) {
            ctx.phase_mark(2);
            PMC_HIP(hipMemcpyAsync(ctx.h_scal, mini_stats.p, sizeof(pmc_stats) * nb, hipMemcpyDeviceToHost, st));
            PMC_HIP(hipStreamSynchronize(st));
            std::memcpy(stats, ctx.h_scal, sizeof(pmc_stats) * nb);
            ctx.phase_report(stats, nb);
        }
    } else {
    LinOp A;
    A.n = n;
    A.n0 = hybrid ? 0 : n_u;
    SellView Av = view(d.A);
    Av.tag = 1;
    A.apply = [Av](const Lanes& L, int nb_, const double* x, double* y, double* partial, double*) {
        return k::DotParts{partial, k::spmm(L.main, nb_, Av, x, y, false, partial, x)};
    };
    A.apply_z = [Av](const Lanes& L, int nb_, zvec x, double* y, double* partial, double*) {
        return k::DotParts{partial, k::spmm_z(L.main, nb_, Av, x, y, partial, x)};
    };
    if (hybrid && !Av.bv) {   // the multiplier solve may run the operator twice per iteration and never store q (minres_solve)
        A.apply_z_dot = [Av](const Lanes& L, int nb_, zvec x, double* partial, double*) {
            return k::DotParts{partial, k::spmm_z_dot(L.main, nb_, Av, x, partial)};
        };
        A.apply_z_update = [Av](const Lanes& L, int nb_, zvec x, const k::LanczosUpdate& lz, double* v, bool v_zero) {
            k::spmm_z_update(L.main, nb_, Av, x, lz, v, v_zero);
        };
    }
    PrecFn prec = preconditioner(level, nb);
    // hybridized solver: the Lanczos update also writes the fp32 copy the cycle's first two kernels read (LAB_NOTES 10.9)
    work.want_r32 = hybrid && opts.precond_storage != PMC_STORAGE_FP64 && mgp->top_reads_r32(mg_l0, nb);
    if (const char* e = lab_env("PMC_R32")) work.want_r32 = work.want_r32 && atoi(e) != 0;
    work.r32_valid = false;
    mgp->smooth_timer = (hybrid && work.op_timer.on && opts.use_graph == 0) ? &vc_timer : nullptr;
    vc_timer.on = mgp->smooth_timer != nullptr;
    GraphHint hint;
    hint.key = hash_mix(hash_mix(hash_mix(0x5a, (uint64_t)level + 1), (uint64_t)nb), (uint64_t)x_row0);
    if (key_salt) hint.key = hash_mix(hint.key, key_salt);
    hint.sig = hash_ptr(hash_ptr(hash_ptr(mgp->signature(mg_l0), cx.p), cd.p), cx2.p);
    MinresResult res = minres_solve(ctx, nb, A, prec, rhs.p, sol.p, zero_guess, opts, work, x_row0, x_nrows, nullptr, hint, rhs_fn);
    if (vc_timer.on) vc_timer.harvest();   // minres_solve has synchronised the stream
    if (stats) {
        ctx.phase_mark(2);
        for (int kcol = 0; kcol < nb; ++kcol) stats[kcol] = res.col[kcol];
        ctx.phase_report(stats, nb);
    }
    }
}

// z = B^-1 r of `level`: the block-diagonal preconditioner of the MINRES solve (M-block polynomial | V-cycle on the Schur block)
PrecFn Sampler::preconditioner(int level, int nb) {
    SamplerLevel& d = lv[level];
    const int n_u = d.n_u;
    Multigrid* mgp = &cycle_mg(level);
    const int mg_l0 = cycle_hierarchy(level).first;
    if (hybrid) {   // SPD multiplier system: the V-cycle alone
        (void)nb;
        return [=](const Lanes& L, int nb_, const double* r, zvec z, double* dot_partial, double*) {
            // inside the MINRES loop the Lanczos update has left an fp32 copy of r (MinresWork::r32): the cycle's first two
            // kernels on the finest level read that
            mgp->r32_top = work.r32_valid ? work.r32.p : nullptr;
            work.r32_valid = false;
            const int nblk = mgp->vcycle_z(L.main, nb_, mg_l0, r, z, dot_partial);
            return k::DotParts{dot_partial, nblk, nullptr, 0};
        };
    }
    const SellView Mv = view(d.M);
    const double* dinvM = d.dinvM.p;
    ChebParams cpM{degree_M(level), 1.0, d.ratio_M, d.M_scaled.p};
    if (!cheb_fused(cpM, true)) cx2.ensure((size_t)n_u * nb);   // higher degrees iterate in fp64 scratch (cheb_apply_z)
    double* cxp = cx.p;
    double* cx2p = cx2.p;
    double* cdp = cd.p;
    return [=](const Lanes& L, int nb_, const double* r, zvec z, double* dot_partial, double* dot_partial2) {
        // The two diagonal blocks are independent.  The V-cycle of the S-block runs on the main stream; once its
        // bandwidth-bound finest-level kernels are enqueued, the one-pass polynomial of the M-block starts on the second
        // stream and fills the chip while the V-cycle's coarse levels (short kernels, a few workgroups each) run.
        int nblk_u = 0;
        auto m_block = [&]() {
            L.fork();
            nblk_u = cheb_apply_z(L.side(), nb_, Mv, dinvM, false, cpM, r, z, cxp, cx2p, cdp, dot_partial2);
        };
        const int nblk_s = mgp->vcycle_z(L.main, nb_, mg_l0, r + (size_t)n_u * nb_, z + (size_t)n_u * nb_, dot_partial, m_block);
        L.join();
        return k::DotParts{dot_partial, nblk_s, dot_partial2, nblk_u};   // <r, z> = s-block partials + u-block partials
    };
}

// post-smoothing of the finest V-cycle level: shared matrix (scaled values + column indices), 1 / diagonal and parent index
// per row; per realization res (fp32), the pre-smoothed iterate (fp32) and r (fp64, for the fused <r, z>) read, z written,
// and the coarse correction (in the storage level 1 returns it in: Multigrid::inner_f32) gathered once per coarse row
double Sampler::smoother_bytes(int level, int nb) const {
    if (!hybrid || level < 0 || level >= n_mc || !amg[level] || amg[level]->L.size() < 2) return 0.0;
    const MgLevel& m = amg[level]->L[0];
    const double zb = opts.precond_storage == PMC_STORAGE_FP64 ? 8.0 : 4.0;
    const double cb = amg[level]->inner_f32(1, 0, nb) ? 4.0 : 8.0;
    return 12.0 * (double)m.S.nnz + 12.0 * m.n + (double)nb * ((4.0 + 4.0 + 8.0 + zb) * m.n + cb * amg[level]->L[1].n);
}

void Sampler::apply_preconditioner(int level, int nbatch, const double* r_in, double* z_out, int memspace) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "apply_preconditioner: level out of range");
    PMC_REQUIRE(valid_batch(nbatch) && nbatch <= batch_width((size_t)lv[level].n_u + lv[level].n_s, false, ctx.device) && r_in != nullptr && z_out != nullptr,
                "apply_preconditioner: nbatch must be a launch width of the level");
    ctx.activate();
    hipStream_t st = ctx.stream;
    SamplerLevel& d = lv[level];
    const size_t n = system_rows(level);
    const int nb = nbatch;
    ensure(level, nb);
    DevBuf<double> stage, zi(n * nb), part((size_t)2 * dot_capacity((int)n, nb) * nb);
    const double* r_d = r_in;
    if (memspace == PMC_MEM_HOST) {
        stage.alloc(n * nb);
        PMC_HIP(hipMemcpyAsync(stage.p, r_in, sizeof(double) * n * nb, hipMemcpyHostToDevice, st));
        r_d = stage.p;
    }
    // hybrid handles: multiplier vectors cross the boundary in the caller's numbering (see lam_new2old)
    k::interleave(st, nb, (int)n, r_d, nullptr, 1.0, rhs.p, hybrid ? d.lam_new2old.p : nullptr);
    PrecFn prec = preconditioner(level, nb);
    // the result is taken in fp64: with PMC_STORAGE_FP32 the solver additionally rounds it to fp32 (6e-8 relative)
    prec(ctx.lanes(false), nb, rhs.p, zvec(zi.p, false), part.p, part.p + (size_t)dot_capacity((int)n, nb) * nb);
    double* out_d = memspace == PMC_MEM_HOST ? stage.p : z_out;
    k::deinterleave(st, nb, (int)n, zi.p, hybrid ? d.lam_old2new.p : nullptr, nullptr, false, out_d);
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipMemcpyAsync(z_out, stage.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
}

void Sampler::mult(int level, int nbatch, const double* rhs_in, double* sol_io, bool use_guess, int memspace, pmc_stats* stats) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "Mult: level out of range");
    PMC_REQUIRE(nbatch >= 1 && rhs_in != nullptr && sol_io != nullptr, "Mult: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    const size_t n = system_rows(level);
    const int width = batch_width((size_t)lv[level].n_u + lv[level].n_s, false, ctx.device);
    ensure(level, first_chunk(width, nbatch));
    // sol_io is read only with a guess and always written: an In (absent without a guess) and an Out on one staging buffer
    DevBuf<double> stage_r, stage_x;
    enum { RHS, GUESS, SOL, STATS };
    for_chunks(ctx, width, nbatch, memspace, true,
               {ChunkArg::in(rhs_in, n, stage_r), ChunkArg::in(use_guess ? sol_io : nullptr, n, stage_x), ChunkArg::out(sol_io, n, stage_x),
                ChunkArg::stats(stats)},
               [&](const Chunk& c) {
                   if (stats) ctx.phase_mark(0);
                   // hybrid handles: multiplier vectors cross the boundary in the caller's numbering (see lam_new2old)
                   const int* n2o = hybrid ? lv[level].lam_new2old.p : nullptr;
                   k::interleave(st, c.nb, (int)n, c.at<double>(RHS), nullptr, 1.0, rhs.p, n2o);
                   if (use_guess) k::interleave(st, c.nb, (int)n, c.at<double>(GUESS), nullptr, 1.0, sol.p, n2o);
                   if (stats) ctx.phase_mark(1);
                   solve_system(level, c.nb, !use_guess, 0, (int)n, c.at<pmc_stats>(STATS));
                   k::deinterleave(st, c.nb, (int)n, sol.p, hybrid ? lv[level].lam_old2new.p : nullptr, nullptr, false, c.at<double>(SOL));
               });
}

void Sampler::apply_operator(int level, int nb, const double* x, double* y, int memspace, int repeat, double* avg_ms,
                             double* bytes) {
    PMC_REQUIRE(level >= 0 && level < nlevels, "apply_operator: level out of range");
    PMC_REQUIRE(valid_batch(nb) && x != nullptr && y != nullptr && repeat >= 1, "apply_operator: bad arguments");
    ctx.activate();
    hipStream_t st = ctx.stream;
    SamplerLevel& d = lv[level];
    const size_t n = system_rows(level);
    DevBuf<double> xi(n * nb), yi(n * nb), stage;
    const double* xd = x;
    double* yd = y;
    if (memspace == PMC_MEM_HOST) {
        stage.alloc(n * nb);
        PMC_HIP(hipMemcpyAsync(stage.p, x, sizeof(double) * n * nb, hipMemcpyHostToDevice, st));
        xd = stage.p;
        yd = stage.p;
    }
    k::interleave(st, nb, (int)n, xd, nullptr, 1.0, xi.p, hybrid ? d.lam_new2old.p : nullptr);
    SellView Av = view(d.A);
    Av.tag = 2;   // own kernel instantiation: the profile row of these launches holds nothing else
    k::spmm(st, nb, Av, xi.p, yi.p, false, nullptr, nullptr);   // untimed first touch
    // laboratory probes (lab builds only): PMC_PROBE_FLUSH_MB = bytes overwritten between launches (evicts the operator
    // from L2 / Infinity Cache, i.e. the state in which MINRES finds it), PMC_PROBE_DOT = time the fused <x, Ax> variant
    const char* e_flush = lab_env("PMC_PROBE_FLUSH_MB");
    const char* e_dot = lab_env("PMC_PROBE_DOT");
    const size_t flush_bytes = e_flush ? (size_t)atol(e_flush) << 20 : 0;
    DevBuf<double> flush, part;
    if (flush_bytes) flush.alloc(flush_bytes / sizeof(double));
    if (e_dot && atoi(e_dot)) part.alloc((size_t)dot_capacity((int)n, nb) * nb);
    double total_ms = 0.0;
    if (!flush_bytes) {
        PMC_HIP(hipEventRecord(ctx.ev0, st));
        for (int r = 0; r < repeat; ++r) k::spmm(st, nb, Av, xi.p, yi.p, false, part.p, part.p ? xi.p : nullptr);
        PMC_HIP(hipEventRecord(ctx.ev1, st));
    } else {
        for (int r = 0; r < repeat; ++r) {
            PMC_HIP(hipMemsetAsync(flush.p, r & 0xff, flush_bytes, st));
            PMC_HIP(hipEventRecord(ctx.ev0, st));
            k::spmm(st, nb, Av, xi.p, yi.p, false, part.p, part.p ? xi.p : nullptr);
            PMC_HIP(hipEventRecord(ctx.ev1, st));
            PMC_HIP(hipStreamSynchronize(st));
            float ms1 = 0.f;
            PMC_HIP(hipEventElapsedTime(&ms1, ctx.ev0, ctx.ev1));
            total_ms += ms1;
        }
    }
    k::deinterleave(st, nb, (int)n, yi.p, hybrid ? d.lam_old2new.p : nullptr, nullptr, false, yd);
    if (memspace == PMC_MEM_HOST) PMC_HIP(hipMemcpyAsync(y, stage.p, sizeof(double) * n * nb, hipMemcpyDeviceToHost, st));
    PMC_HIP(hipStreamSynchronize(st));
    if (avg_ms) {
        if (!flush_bytes) {
            float ms = 0.f;
            PMC_HIP(hipEventElapsedTime(&ms, ctx.ev0, ctx.ev1));
            total_ms = ms;
        }
        *avg_ms = total_ms / repeat;
    }
    if (bytes) *bytes = 12.0 * d.A.nnz + 4.0 * d.A.nrows + (double)nb * 8.0 * ((double)d.A.nrows + d.A.ncols);
}

void Sampler::eval(int level, int xi_level, int nbatch, const double* xi, double* s_out, const double* init_s,
                   int init_level, bool use_init, double* emb_out, int memspace, pmc_stats* stats) {
    PMC_REQUIRE(level >= 0 && level < n_mc, "Eval: level out of range");
    PMC_REQUIRE(xi_level >= 0 && xi_level <= level, "Eval: xi_level must satisfy 0 <= xi_level <= level");
    PMC_REQUIRE(nbatch >= 1 && xi != nullptr && s_out != nullptr, "Eval: bad arguments");
    if (kl) {   // the 5-argument Eval of KLSampler ignores u and use_init (KLSampler.hpp:69-77)
        eval_kl(level, xi_level, nbatch, xi, s_out, emb_out, memspace, stats);
        return;
    }
    if (use_init) {
        PMC_REQUIRE(init_s != nullptr, "Eval: use_init without init_s");
        PMC_REQUIRE(init_level >= level && init_level < nlevels, "Eval: init_level must be coarser than or equal to level");
    }
    ctx.activate();
    hipStream_t st = ctx.stream;
    const int n_xi = lv[xi_level].n_s, n_out = lv[level].out_size, n_s = lv[level].n_s;
    const int n_init = use_init ? lv[init_level].n_s : 0;
    const int width = launch_width(level);
    const int widest = first_chunk(width, nbatch);
    // embed_s_out may alias init_s (the managers pass one buffer for both).  With several launches and a coarser
    // init_level a launch's embed rows (n_s each) would overwrite init rows (n_init < n_s each) of later launches before
    // they are read: keep a private copy of init_s for the whole call then.  (Device memory only; host memory: DESIGN.md,
    // "How a batched call becomes launches".)
    DevBuf<double> init_copy;
    if (use_init && memspace == PMC_MEM_DEVICE && emb_out == init_s && n_init != n_s && widest < nbatch) {
        init_copy.alloc((size_t)n_init * nbatch);
        PMC_HIP(hipMemcpyAsync(init_copy.p, init_s, sizeof(double) * n_init * nbatch, hipMemcpyDeviceToDevice, st));
        init_s = init_copy.p;
    }
    ensure(level, widest);   // the staging buffers are among what it sizes: no launch may grow them behind an upload
    // init_s and embed_s_out share stage_emb: a launch has consumed the guess before it writes the embedded field
    enum { XI, INIT, S, EMB, STATS };
    for_chunks(ctx, width, nbatch, memspace, memspace == PMC_MEM_HOST,
               {ChunkArg::in(xi, (size_t)n_xi, stage_in), ChunkArg::in(use_init ? init_s : nullptr, (size_t)n_init, stage_emb),
                ChunkArg::out(s_out, (size_t)n_out, stage_out), ChunkArg::out(emb_out, (size_t)n_s, stage_emb), ChunkArg::stats(stats)},
               [&](const Chunk& c) {
                   eval_chunk(level, xi_level, c.nb, c.at<double>(XI), c.at<double>(S), c.at<double>(INIT), init_level, use_init,
                              c.at<double>(EMB), c.at<pmc_stats>(STATS));
               });
    if (init_copy.p) PMC_HIP(hipStreamSynchronize(st));   // the private copy is released on return
}

// M-block degree of `level`: as asked for, or by the measured Chebyshev interval of the level - meshes with badly shaped
// cells (cube_tet_embed: lambda_max / lambda_min = 22 against 8 on uniform tetrahedra) pay for degree 4 (69.6 -> 55.9
// iterations, 20.0 -> 19.5 ms per batch at 314 k DoF), well shaped ones do not
int Sampler::degree_M(int level) const {
    return opts.cheb_degree_M > 0 ? opts.cheb_degree_M : (lv[level].ratio_M > 16.0 ? 4 : 2);
}

// the hierarchy the solves of `level` cycle on: the level's internal one from its level 0, or the caller's from `level`
CycleHierarchy Sampler::cycle_hierarchy(int level) const {
    const bool own = level < (int)amg.size() && amg[level];
    return CycleHierarchy{own ? *amg[level] : mg, own ? 0 : level, own};
}

// sizes and kernel-selection flags of one level of that cycle (pmc_sampler_vcycle_info; layout in include/pmc.h)
void Sampler::vcycle_info(int level, int vlevel, int* nvlevels, int64_t* info) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, "pmc_sampler_vcycle_info: level out of range");
    const CycleHierarchy h = cycle_hierarchy(level);
    const Multigrid& g = h.g;
    const int first = h.first;
    *nvlevels = (int)g.L.size() - first;
    PMC_REQUIRE(vlevel >= 0 && vlevel < *nvlevels, "pmc_sampler_vcycle_info: vlevel out of range");
    const MgLevel& m = g.L[(size_t)(first + vlevel)];
    // bit 0 is a statement about the tail DESCRIPTORS, not about a launch: one exists on this level or on one above it.  (The
    // in_tail of cycle_role is per launch width, and false below an is_last level outside the tail, which ends the cycle.)
    bool in_tail = false;
    for (int l = first; l <= first + vlevel; ++l) in_tail = in_tail || (l < (int)g.tail.size() && g.tail[l].p != nullptr);
    info[0] = m.n;
    info[1] = m.S.nnz;
    info[2] = m.S.nslots;
    info[3] = m.has_sp ? m.SP.nnz : 0;
    info[4] = m.has_sp ? m.SP.nslots : 0;
    info[5] = (in_tail ? 1 : 0) | (m.dense_inv.p ? 2 : 0) | ((int64_t)m.split_log2 << 4);
    info[6] = (m.p_agg || m.p_oct) ? 1 : 0;
}

// setup values of the V-cycle of `level` (pmc_sampler_vcycle_level; layout in include/pmc.h).  Reads setup only.
void Sampler::vcycle_level(int level, int vlevel, int* nvlevels, double* info) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, "pmc_sampler_vcycle_level: level out of range");
    const CycleHierarchy h = cycle_hierarchy(level);
    const Multigrid& g = h.g;
    const int first = h.first;
    const bool own = h.own;
    *nvlevels = (int)g.L.size() - first;
    PMC_REQUIRE(vlevel >= 0 && vlevel < *nvlevels, "pmc_sampler_vcycle_level: vlevel out of range");
    const MgLevel& m = g.L[(size_t)(first + vlevel)];
    bool tail_wide = false, tail_narrow = false;
    const int role_wide = g.cycle_role(first, kMaxBatch + 1, first + vlevel, &tail_wide);
    const int role_narrow = g.cycle_role(first, std::max(1, g.dense_nb), first + vlevel, &tail_narrow);
    const SamplerLevel& d = lv[level];
    info[0] = m.n;
    info[1] = m.lmax;
    info[2] = role_wide;
    info[3] = g.smooth_degree;
    info[4] = g.smooth_ratio;
    info[5] = m.is_last ? m.last_degree : g.coarse_degree;
    info[6] = m.is_last ? m.last_ratio : g.coarse_ratio;
    info[7] = own ? 1.0 : 0.0;   // internal hierarchies are plain Galerkin products; the caller's levels are rediscretized
    info[8] = hybrid ? 0.0 : d.ratio_M;
    info[9] = hybrid ? 0.0 : degree_M(level);
    info[10] = hybrid ? 2.0 : own ? 1.0 : 0.0;
    info[11] = g.dense_nb;
    info[12] = role_narrow;
    info[13] = tail_wide ? 1.0 : 0.0;
    info[14] = tail_narrow ? 1.0 : 0.0;
}

// P from vlevel + 1 to vlevel of the V-cycle of `level` (pmc_sampler_vcycle_prolongator): vlevel 0 of a hybridized handle in
// the caller's multiplier numbering (the agg_pack_rows renumbering undone into `scratch`)
const HostCsr& Sampler::vcycle_prolongator(int level, int vlevel, HostCsr& scratch) const {
    PMC_REQUIRE(level >= 0 && level < n_mc, "pmc_sampler_vcycle_prolongator: level out of range");
    const CycleHierarchy h = cycle_hierarchy(level);
    const Multigrid& g = h.g;
    const int first = h.first;
    const bool own = h.own;
    PMC_REQUIRE(vlevel >= 0 && first + vlevel + 1 < (int)g.L.size(), "pmc_sampler_vcycle_prolongator: vlevel out of range");
    const HostCsr& P = own ? g.L[(size_t)vlevel].P_host : lv[(size_t)(first + vlevel)].P_host;
    PMC_REQUIRE(P.nrows == g.L[(size_t)(first + vlevel)].n, "pmc_sampler_vcycle_prolongator: no prolongator kept");
    const std::vector<int>& n2o = lv[level].lam_n2o_host;
    if (!(hybrid && vlevel == 0 && !n2o.empty())) return P;
    std::vector<int> old2new(n2o.size());
    for (size_t i = 0; i < n2o.size(); ++i) old2new[(size_t)n2o[i]] = (int)i;
    scratch = csr_permute(P, old2new, true, false);   // row i of the result: the library's row old2new[i]
    return scratch;
}

}  // namespace pmc

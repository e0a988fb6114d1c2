// PDESamplerTest's result table from C++: DeviceKLSampler of parelagmc_amd/host/mfem_adapter.hpp (compiled against
// tests/c/mfem_shim.hpp) for ComputeL2Error / ComputeMaxError on mfem::Vector, and the parelagmc.hpp mirror over the same
// handle for the statistics (FieldStatistics) and the batched error calls on host and device vectors, which must agree with
// the adapter's.  Usage: as field_stats_smoke.c; prints the same table and a final line "field_stats_adapter_smoke OK".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "mfem_shim.hpp"

#include "../../parelagmc_amd/host/mfem_adapter.hpp"
#include "../../parelagmc_amd/host/parelagmc.hpp"

extern "C" {
#include "kl_io.h"
}

using namespace parelagmc;

int main(int argc, char** argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: field_stats_adapter_smoke problem.bin seed chi_index nsamples exact_expectation exact_variance\n");
        return 2;
    }
    kl_file k = kl_load(argv[1]);
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    const int chi_index = std::atoi(argv[3]);
    const int64_t nsamples = std::strtoll(argv[4], nullptr, 10);
    const double exact_e = std::atof(argv[5]), exact_v = std::atof(argv[6]);
    const int n0 = k.lv[0].n_s;
    mfem::Vector evals(k.evals, k.nmodes);
    std::vector<mfem::Vector> w;
    std::vector<mfem::SparseMatrix> P;
    w.reserve((size_t)k.nlevels);
    P.reserve((size_t)k.nlevels);
    std::vector<mfem_adapter::KLLevelOps> ops((size_t)k.nlevels);
    for (int l = 0; l < k.nlevels; ++l) {
        w.emplace_back(k.lv[l].w, k.lv[l].n_s);
        ops[(size_t)l].w_diag = &w.back();
        if (k.lv[l].has_p) {
            P.emplace_back(k.lv[l].P.nrows, k.lv[l].P.ncols, k.lv[l].P.rp, k.lv[l].P.ci, k.lv[l].P.v);
            ops[(size_t)l].P = &P.back();
        }
    }
    try {
        mfem_adapter::DeviceKLSampler smp(0, evals, k.evect0, n0, ops, k.lognormal != 0, seed);
        KLSampler mirror(smp.context(), smp.handle());
        std::vector<double> chi((size_t)n0, 0.0);
        chi[(size_t)chi_index] = 1.0;
        for (int l = 0; l < k.nlevels; ++l) {
            const int n = smp.SampleSize(l);
            Vector chi_v(smp.context(), PMC_MEM_HOST);
            chi_v.SetSize(n);
            for (int i = 0; i < n; ++i) chi_v.GetData()[i] = chi[(size_t)i];
            FieldStatistics fs(mirror, l, &chi_v);
            fs.Run(0, nsamples);
            mfem::Vector e(n), m2(n), cc(n);
            const int64_t N = fs.Read(e.GetData(), m2.GetData(), cc.GetData());
            const double exp_err = smp.ComputeL2Error(l, e, exact_e);
            const double var_err = smp.ComputeL2Error(l, m2, exact_v);
            const double max_err = smp.ComputeMaxError(l, e, exact_e);
            int ichi = 0;
            for (int i = 1; i < n; ++i)
                if (chi[(size_t)i] > chi[(size_t)ichi]) ichi = i;
            std::printf("level %d: N %lld exp_l2 %.17g var_l2 %.17g exp_max %.17g chi_cov %.17g\n", l, (long long)N, exp_err,
                        var_err, max_err, cc(ichi));
            if (N != nsamples) return 1;
            // the mirror's batched calls on host and device vectors: [e; m2] at once
            Vector two(smp.context(), PMC_MEM_HOST), two_d(smp.context(), PMC_MEM_DEVICE);
            two.SetSize(n, 2);
            two_d.SetSize(n, 2);
            for (int i = 0; i < n; ++i) {
                two.GetData()[i] = e(i);
                two.GetData()[n + i] = m2(i);
            }
            if (pmc_memcpy_h2d(smp.context(), two_d.GetData(), two.GetData(), sizeof(double) * 2 * n) != PMC_OK) return 1;
            for (const Vector* v : {&two, &two_d}) {
                double err[2], mx[2];
                mirror.ComputeL2Error(l, *v, exact_e, err);
                mirror.ComputeMaxError(l, *v, exact_e, mx);
                if (err[0] != exp_err || mx[0] != max_err) { std::fprintf(stderr, "mirror / adapter mismatch\n"); return 1; }
            }
            // a vector of the wrong length is refused before it reaches the device
            bool refused = false;
            try {
                smp.ComputeL2Error(l, mfem::Vector(n + 1), exact_e);
            } catch (const std::runtime_error&) {
                refused = true;
            }
            Vector short_v(smp.context(), PMC_MEM_HOST);
            short_v.SetSize(n - 1);
            try {
                (void)mirror.ComputeMaxError(l, short_v, exact_e);
                refused = false;
            } catch (const std::invalid_argument&) {
            }
            if (!refused) { std::fprintf(stderr, "a coefficient vector of the wrong length was accepted\n"); return 1; }
            // chi on the next level: P_l^T chi (PDESamplerTest.cpp:186-192)
            if (l + 1 < k.nlevels) {
                std::vector<double> nxt((size_t)k.lv[l + 1].n_s, 0.0);
                const kl_csr& Pl = k.lv[l].P;
                for (int r = 0; r < Pl.nrows; ++r)
                    for (int p = Pl.rp[r]; p < Pl.rp[r + 1]; ++p) nxt[(size_t)Pl.ci[p]] += Pl.v[p] * chi[(size_t)r];
                chi.swap(nxt);
            }
        }
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    std::printf("field_stats_adapter_smoke OK\n");
    return 0;
}

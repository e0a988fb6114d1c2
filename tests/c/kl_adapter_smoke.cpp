// KL sampler from C++: DeviceKLSampler of parelagmc_amd/host/mfem_adapter.hpp (compiled against tests/c/mfem_shim.hpp)
// driven the way the reference's managers drive an MLSampler - one realization per call - and the KLSampler mirror of
// parelagmc.hpp over the same handle.  Usage: kl_adapter_smoke problem.bin      final line "kl_adapter_smoke OK".
#include <cmath>
#include <cstdio>
#include <vector>

#include "mfem_shim.hpp"

#include "../../parelagmc_amd/host/mfem_adapter.hpp"
#include "../../parelagmc_amd/host/parelagmc.hpp"

extern "C" {
#include "kl_io.h"
}

using namespace parelagmc;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: kl_adapter_smoke problem.bin\n"); return 2; }
    kl_file k = kl_load(argv[1]);
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
        mfem_adapter::DeviceKLSampler smp(0, evals, k.evect0, n0, ops, k.lognormal != 0, 7);
        mfem::Vector xi, s, u;
        smp.Sample(0, xi);
        if (xi.Size() != n0) { std::fprintf(stderr, "Sample size\n"); return 1; }
        for (int l = 0; l < k.nlevels; ++l) {
            const int ns = k.lv[l].n_s;
            if (smp.SampleSize(l) != ns || smp.GetNNZ(l) != 0) { std::fprintf(stderr, "sizes on level %d\n", l); return 1; }
            double err = 0.0, ref = 0.0;
            for (int b = 0; b < k.nbatch; ++b) {
                mfem::Vector x(k.xi + (size_t)b * n0, n0);
                smp.Eval(l, x, s);
                // u (the previous call's field, on this or a finer level) and use_init are ignored on input; u returns the
                // Gaussian field
                smp.Eval(l, x, s, u, u.Size() > 0);
                if (s.Size() != ns || u.Size() != ns) { std::fprintf(stderr, "Eval sizes\n"); return 1; }
                for (int i = 0; i < ns; ++i) {
                    const double e = k.s_expect[l][(size_t)b * ns + i];
                    err = std::fmax(err, std::fabs(s(i) - e));
                    ref = std::fmax(ref, std::fabs(e));
                    const double g = k.lognormal ? std::exp(u(i)) : u(i);
                    err = std::fmax(err, std::fabs(g - s(i)) / std::fmax(1.0, std::fabs(s(i))) * ref);
                }
            }
            std::printf("level %d: max |s - s_expect| / max |s_expect| = %.3e, iterations %d\n", l, err / ref, smp.GetNumIters());
            if (!(err <= 1e-12 * ref) || smp.GetNumIters() != 0) return 1;
        }
        // the mirror class of parelagmc.hpp over the same handle
        KLSampler mirror(smp.context(), smp.handle());
        for (int l = 0; l < k.nlevels; ++l)
            if (mirror.SampleSize(l) != k.lv[l].n_s || mirror.GetNNZ(l) != 0) { std::fprintf(stderr, "mirror sizes\n"); return 1; }
        if (k.nlevels > 1) {
            const pmc_csr Pt = mirror.GetTrueP(0);
            if (Pt.nrows != n0 || Pt.ncols != k.lv[1].n_s) { std::fprintf(stderr, "mirror GetTrueP\n"); return 1; }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("kl_adapter_smoke OK\n");
    return 0;
}

// ParticleTracer::RunAdjoint of parelagmc.hpp from C++ (tests/test_gpu_tracer_adjoint.py builds and runs it): a channel of two
// unit boxes along x with an accelerating flux, u_bar of J = T of one particle against a central difference in the interior
// flux.  The particle moves along x only, so J is the sum of two closed-form crossing times.  The Darcy mirrors are referenced
// so that they must link.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../parelagmc_amd/host/parelagmc.hpp"

using namespace parelagmc;

static double T_of(ParticleTracer& t, pmc_ctx* ctx, const double* u11, double* ubar11, double* x0bar3) {
    Vector u(ctx, PMC_MEM_HOST), ub(ctx, PMC_MEM_HOST);
    u.SetSize(11, 1);
    for (int i = 0; i < 11; ++i) u.GetData()[i] = u11[i];
    double Tb = 1.0, T = 0.0, x0b[3];
    int32_t face = -1, status = -1, nsteps = 0;
    t.RunAdjoint(u, &Tb, nullptr, ub, x0b, &T, &face, &status, &nsteps);
    if (status != PMC_TRACER_EXITED || nsteps != 2 || face != 8) {
        std::printf("unexpected path: status %d, %d steps, exit face %d\n", status, nsteps, face);
        return NAN;
    }
    if (ubar11)
        for (int i = 0; i < 11; ++i) ubar11[i] = ub.GetData()[i];
    if (x0bar3)
        for (int i = 0; i < 3; ++i) x0bar3[i] = x0b[i];
    return T;
}

int main() {
    auto grad = &DarcySolver::SolveFwd_TracerGradient;
    auto loglik = &DarcySolver::ComputeGradTravelTimeLogLikelihood;
    auto seed = &ParticleTracer::ReduceSeed;
    if (!grad || !loglik || !seed) return 2;
    pmc_ctx* ctx = nullptr;
    if (pmc_ctx_create(0, &ctx) != PMC_OK) {
        std::printf("no context: %s\n", pmc_last_error());
        return 1;
    }
    int rc = 1;
    {
        // local faces z-, y-, x+, y+, x-, z+; face 2 is shared: x+ of box 0, x- of box 1
        const int32_t elem_face[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 10};
        const int8_t elem_sign[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, 1};
        const int32_t face_elem[22] = {0, -1, 0, -1, 0, 1, 0, -1, 0, -1, 0, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1};
        const double geom[12] = {0, 0, 0, 1, 1, 1, 1, 0, 0, 2, 1, 1};
        pmc_tracer_mesh mesh{PMC_TRACER_BOX, 2, 11, elem_face, elem_sign, face_elem, geom, nullptr};
        const double x0[3] = {0.25, 0.5, 0.5};
        const int32_t e0 = 0;
        ParticleTracer t(ctx, mesh, 1, x0, &e0);
        t.SetAdjointScratch(1);            // one column per chunk: no result depends on it
        double u[11] = {0, 0, 1.2, 0, -1.0, 0, 0, 0, 1.5, 0, 0}, ubar[11], x0bar[3];
        const double T0 = T_of(t, ctx, u, ubar, x0bar), h = 1e-6;
        u[2] = 1.2 + h;
        const double Tp = T_of(t, ctx, u, nullptr, nullptr);
        u[2] = 1.2 - h;
        const double Tm = T_of(t, ctx, u, nullptr, nullptr);
        const double fd = (Tp - Tm) / (2 * h);
        // box 0: v = 1 + 0.2 x, T_0 = ln(1.2 / 1.05) / 0.2; box 1: v = 1.2 + 0.3 (x - 1), T_1 = ln(1.5 / 1.2) / 0.3
        const double exact = std::log(1.2 / 1.05) / 0.2 + std::log(1.5 / 1.2) / 0.3;
        std::printf("T %.15g (exact %.15g)  u_bar[2] %.15g  central difference %.15g  x0_bar[0] %.15g\n", T0, exact, ubar[2], fd,
                    x0bar[0]);
        // dT / dx0 = -1 / v(x0) = -1 / 1.05
        if (std::isfinite(T0) && std::fabs(T0 - exact) <= 1e-14 * exact && std::fabs(ubar[2]) > 1e-3 &&
            std::fabs(fd - ubar[2]) <= 1e-7 * std::fabs(fd) && std::fabs(x0bar[0] + 1.0 / 1.05) <= 1e-13 && x0bar[1] == 0.0 &&
            x0bar[2] == 0.0)
            rc = 0;
    }
    pmc_ctx_destroy(ctx);
    if (rc == 0) std::printf("tracer adjoint smoke ok\n");
    return rc;
}

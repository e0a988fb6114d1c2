"""Setup side of the ratio managers' posterior field estimates (no GPU): the new declarations compile from C and C++, the
symbols are exported by both libraries and bound in Python, and a callbacks manager refuses the feature."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DEVICE = ["pmc_level_fields_accumulate_weighted"]
MANAGER = ["pmc_ratio_enable_field_stats", "pmc_ratio_field_stats"]


def _exported(lib):
    return subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout


def test_new_symbols_are_exported_and_bound():
    from parelagmc_amd import capi, host_api
    exp = _exported(capi.LIB_PATH)
    for nm in DEVICE:
        assert f" T {nm}\n" in exp, nm
        assert nm in capi.SYMBOLS, nm
    assert hasattr(capi.LevelFields, "accumulate_weighted")
    host = _exported(host_api.HOST_LIB_PATH)
    for nm in MANAGER:
        assert f" T {nm}\n" in host, nm
        assert nm in host_api.HOST_SYMBOLS, nm
    for nm in ("parelagmc::ML_BayesRatio_Manager::EnableFieldStatistics(parelagmc::Vector const&)",
               "parelagmc::ML_BayesRatio_Manager::FieldStatistics(parelagmc::Vector*, parelagmc::Vector*, "
               "parelagmc::Vector*, double*, double*)"):
        assert nm in host, nm
    assert hasattr(host_api.RatioManager, "enable_field_stats") and hasattr(host_api.RatioManager, "field_stats")


C_SRC = """#include <pmc.h>
#include <pmc_host.h>
int f(pmc_level_fields* lf, pmc_ratio* m) {
    double x = 0.0, w = 1.0;
    return pmc_level_fields_accumulate_weighted(lf, 1, &x, &w, &x, &w, PMC_MEM_HOST)
        + pmc_level_fields_accumulate_weighted(lf, 1, &x, &w, NULL, NULL, PMC_MEM_DEVICE)
        + pmc_ratio_enable_field_stats(m, &x, PMC_MEM_HOST)
        + pmc_ratio_field_stats(m, &x, NULL, NULL, &x, NULL, PMC_MEM_DEVICE);
}
"""


def test_headers_compile_as_c11_with_werror(tmp_path):
    src = tmp_path / "h.c"
    src.write_text(C_SRC)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mirror_compiles_as_cpp17(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text(C_SRC + """#include "parelagmc.hpp"
void g(parelagmc::ML_BayesRatio_Manager& m, parelagmc::Vector& w0, parelagmc::Vector& mean) {
    std::vector<double> l2(2), iv(2);
    m.EnableFieldStatistics(w0);
    if (m.FieldStatisticsEnabled()) m.FieldStatistics(&mean, nullptr, nullptr, l2.data(), iv.data());
}
struct P : parelagmc::BayesRatioProblem {
    void SamplePrior(int, parelagmc::Vector&, uint64_t, int) override {}
    void EvalPrior(int, const parelagmc::Vector&, parelagmc::Vector&) override {}
    void ComputeLikelihoodAndR(int, parelagmc::Vector&, double*, double*, double*) override {}
    int GetGlobalNumberOfDofs(int) const override { return 1; }
};
int h(const P& p) { return p.DarcyHandle() == nullptr ? p.PriorFieldSize(0) : 0; }
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "parelagmc_amd", "host"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _callbacks_manager(nlevels=2):
    from parelagmc_amd import host_api
    cb = dict(sample=lambda lvl, first, nb: np.zeros((nb, 2)),
              eval=lambda lvl, xl, xi, init, init_level: (np.ones((xi.shape[0], 2)), np.zeros((xi.shape[0], 2))),
              solve=lambda lvl, k: (np.ones(k.shape[0]), np.ones(k.shape[0])),
              xi_size=[2] * nlevels, sample_size=[2] * nlevels, ndofs=[4, 2][:nlevels])
    like = lambda lvl, k: (np.full(k.shape[0], 0.5), np.full(k.shape[0], 0.25), np.ones(k.shape[0]))   # noqa: E731
    return host_api.RatioManager(nlevels, callbacks=cb, likelihood=like, wall_time=False, batch=4)


def test_callbacks_manager_refuses_field_stats():
    """the callbacks manager's fields never reach the device: refused with PMC_ERR_INVALID, the manager still runs"""
    from parelagmc_amd import capi
    mgr = _callbacks_manager()
    with pytest.raises(capi.PmcError) as e:
        mgr.enable_field_stats(np.ones(2))
    assert e.value.code == -1 and "device-handle managers only" in str(e.value)
    with pytest.raises(capi.PmcError) as e:
        mgr.field_stats()
    assert e.value.code == -1 and "not enabled" in str(e.value)
    r = mgr.InitRun([3, 3])
    assert r["nsamples"].tolist() == [3, 3] and r["Z_estimate"] == pytest.approx(0.5)
    mgr.close()

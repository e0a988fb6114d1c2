"""Setup side of the field statistics (no GPU): chi_center_of_mass, the level-by-level restriction of chi, the exported
symbols and the C header."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _brute_force_chi(mesh, vol):
    """plain-Python restatement of chi_center_of_mass: serial sums, first strict minimum"""
    ne, dim = mesh.ne, mesh.dim
    xe = [[sum(float(mesh.verts[v][d]) for v in mesh.elems[e]) / len(mesh.elems[e]) for d in range(dim)] for e in range(ne)]
    volume = 0.0
    for e in range(ne):
        volume += float(vol[e])
    cm = []
    for d in range(dim):
        acc = 0.0
        for e in range(ne):
            acc += float(vol[e]) * xe[e][d]
        cm.append(acc / volume)
    best, arg = 1e10, -1
    for e in range(ne):
        dist = 0.0
        for d in range(dim):
            dist += (cm[d] - xe[e][d]) ** 2
        dist = dist ** 0.5
        if dist < best:
            best, arg = dist, e
    return arg


@pytest.mark.parametrize("n,sizes,etype,origin", [
    ([4, 4, 4], [2, 2, 2], "hex", None),             # PDESamplerTest's mesh: 8 elements tie at the centre
    ([3, 2, 5], [1.0, 2.0, 3.0], "hex", [0.3, -0.1, 0.7]),
    ([5, 3], [2.0, 1.0], "quad", None),
    ([2, 1], [2.0, 1.0], "quad", None),             # two elements exactly as near: the first one wins
])
def test_chi_center_of_mass_matches_a_brute_force_search(n, sizes, etype, origin):
    from parelagmc_amd.fe import box_mesh, build_spaces, chi_center_of_mass
    m = box_mesh(n, sizes, etype, origin=origin)
    sp_ = build_spaces(m)
    chi = chi_center_of_mass(sp_)
    assert chi.shape == (sp_.n_s,) and chi.sum() == 1.0 and set(np.unique(chi)) == {0.0, 1.0}
    assert int(np.argmax(chi)) == _brute_force_chi(m, sp_.vol)


@pytest.mark.parametrize("refine", [1, 2])
def test_chi_center_of_mass_on_refined_tet_boxes(refine):
    from parelagmc_amd.fe import build_hierarchy, chi_center_of_mass, kuhn_cube_tet
    h = build_hierarchy(kuhn_cube_tet(2.0), refine)
    sp_ = h.spaces[0]
    chi = chi_center_of_mass(sp_)
    assert chi.sum() == 1.0 and int(np.argmax(chi)) == _brute_force_chi(sp_.mesh, sp_.vol)


def test_chi_center_of_mass_keeps_the_first_of_tied_elements():
    from parelagmc_amd.fe import box_mesh, build_spaces, chi_center_of_mass
    m = box_mesh([4, 4, 4], [2, 2, 2], "hex")
    sp_ = build_spaces(m)
    xe = m.verts[m.elems].mean(axis=1)
    d = np.sqrt(((xe - 1.0) ** 2).sum(axis=1))
    tied = np.nonzero(d == d.min())[0]
    assert len(tied) == 8                               # the centre (1, 1, 1) is a vertex of 8 elements, exactly
    assert int(np.argmax(chi_center_of_mass(sp_))) == tied[0]
    m2 = box_mesh([2, 1], [2.0, 1.0], "quad")
    assert int(np.argmax(chi_center_of_mass(build_spaces(m2)))) == 0


def test_restrict_chi_is_the_product_with_the_transposed_prolongators(hex_hierarchy):
    from parelagmc_amd.fe import chi_center_of_mass, restrict_chi
    chi0 = chi_center_of_mass(hex_hierarchy.spaces[0])
    out = restrict_chi(chi0, hex_hierarchy.P)
    assert len(out) == hex_hierarchy.nlevels
    ref = chi0
    for lvl, P in enumerate(hex_hierarchy.P):
        Pd = P.toarray()
        ref = Pd.T @ ref
        assert out[lvl + 1].shape == (hex_hierarchy.spaces[lvl + 1].n_s,)
        assert np.array_equal(out[lvl + 1], ref)
    assert all(c.sum() == 1.0 for c in out)          # an indicator stays one under P0 injection transposes


def _exported(lib):
    out = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return out


def test_new_symbols_are_exported():
    from parelagmc_amd import capi, host_api
    names = ["pmc_field_stats_create", "pmc_field_stats_destroy", "pmc_field_stats_reset", "pmc_field_stats_accumulate",
             "pmc_field_stats_run", "pmc_field_stats_read", "pmc_field_stats_read_sums", "pmc_field_stats_chi_dot",
             "pmc_sampler_l2_error", "pmc_sampler_max_error", "pmc_sampler_set_output_hierarchy"]
    exp = _exported(capi.LIB_PATH)
    for nm in names:
        assert f" T {nm}\n" in exp, nm
        assert nm in capi.SYMBOLS
    host = _exported(host_api.HOST_LIB_PATH)
    for nm in ("parelagmc::PDESampler::ComputeL2Error(int, parelagmc::Vector const&, double) const",
               "parelagmc::PDESampler::ComputeMaxError(int, parelagmc::Vector const&, double) const",
               "parelagmc::FieldStatistics::Run(unsigned long, long)",
               "parelagmc::FieldStatistics::Read(double*, double*, double*) const"):
        assert nm in host, nm


def test_header_compiles_as_c11_with_werror(tmp_path):
    src = tmp_path / "h.c"
    src.write_text("#include <pmc.h>\n"
                   "int f(pmc_sampler* s, pmc_field_stats* fs) {\n"
                   "    double e = 0.0; int64_t n = 0;\n"
                   "    return pmc_field_stats_read(fs, &e, NULL, NULL, &n, PMC_MEM_HOST) + pmc_field_stats_run(fs, 0, 1)\n"
                   "        + pmc_sampler_l2_error(s, 0, 1, &e, 0.0, &e, PMC_MEM_HOST)"
                   " + pmc_sampler_set_output_hierarchy(s, 1, NULL, &e);\n}\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

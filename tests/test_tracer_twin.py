"""The numpy twin of the particle tracer (parelagmc_amd/fe/tracer.py) against exact paths, uniform flow and an ODE integrator,
the decision-margin cap of the shared cases, and the new C symbols (no GPU needed)."""
import os
import re
import subprocess

import numpy as np
import pytest

import tracer_cases as tc
from conftest import ROOT
from parelagmc_amd import capi
from parelagmc_amd.fe import tracer as tr

NEW_SYMBOLS = ("pmc_tracer_create", "pmc_tracer_destroy", "pmc_tracer_num_particles", "pmc_tracer_run", "pmc_tracer_reduce",
               "pmc_darcy_set_tracer")


def test_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmc.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in exported, s
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    assert "#define PMC_ABI_VERSION 3 " in open(os.path.join(ROOT, "include", "pmc.h")).read()
    assert lib.pmc_abi_version() == 3
    # the host mirror
    hpp = open(os.path.join(ROOT, "parelagmc_amd", "host", "parelagmc.hpp")).read()
    assert "class ParticleTracer" in hpp and "void SetTracer(" in hpp
    assert hasattr(capi, "Tracer") and hasattr(capi.DarcySolver, "SetTracer")


@pytest.mark.parametrize("path", tc.exact_paths(), ids=lambda p: p.name)
def test_exact_paths(path):
    for dtype in (np.float64, np.longdouble):
        r = tr.trace(path.mesh, path.u, path.x0, np.zeros(1, np.int32), dtype=dtype)
        assert r["status"][0] == tr.EXITED and r["exit_face"][0] == path.face and r["nsteps"][0] == 1
        assert abs(r["T"][0] - path.T) <= path.rtol * path.T
        assert np.abs(r["x_exit"][0] - path.x_exit).max() <= path.rtol
        assert np.isinf(r["margin"][0]) == (path.name.startswith("box"))


def test_series_and_closed_form_agree_at_the_switch():
    """L and E: the series and the closed form agree far below an ulp at |argument| = 2^-20, so the switch is no decision"""
    z = np.longdouble(2.0) ** -20
    for s in (z, -z):
        assert abs(((1 - s / 2) + s * s / 3) - np.log1p(s) / s) < 1e-19 * 4
        assert abs(((1 + s / 2) + s * s / 6) - np.expm1(s) / s) < 1e-19 * 4
    for x in (2.0 ** -20, np.nextafter(2.0 ** -20, 0), -2.0 ** -20, 0.0, 1e-300):
        assert abs(float(tr._L(np.float64(x))) - (1 - x / 2)) < 1e-12
        assert abs(float(tr._E(np.float64(x))) - (1 + x / 2)) < 1e-12


@pytest.mark.parametrize("name", ["hex0", "stretch", "tet2"])
def test_uniform_permeability(name):
    """k == 1: plug flow, every particle takes phi (L_z - 1e-3) area / |Q_total|"""
    from oracle.darcy_oracle import DarcyOracle
    c = tc.case(name)
    Q, _, sol = DarcyOracle(tc.problem(c.kind)).solve_fwd(c.level, np.ones(c.space.n_s), True)
    phi = 0.3
    mesh = tr.tracer_mesh(c.space, porosity=phi)
    r = tr.trace(mesh, sol[:c.space.n_u], c.x0, c.elem0)
    expect = phi * (c.extent[2] - 1e-3) * c.extent[0] * c.extent[1] / abs(Q)
    assert (r["status"] == tr.EXITED).all()
    assert np.abs(r["T"] / expect - 1).max() <= 1e-12
    assert (r["x_exit"][:, 2] == 0.0).all() if mesh.kind == tr.BOX else np.abs(r["x_exit"][:, 2]).max() < 1e-14
    assert np.abs(r["x_exit"][:, :2] - c.x0[:, :2]).max() < 1e-12
    assert (c.space.faces.face_bdr_attr[r["exit_face"]] == 1).all()


# Largest relative difference measured against solve_ivp (DOP853, rtol 1e-10, atol 1e-12, fields 0 and 2, particles 0-2):
# boxes 2.5e-8 (hex0), tetrahedra 2.4e-7 (tet2) - the integrator's error across the velocity-gradient jumps at the element
# faces.  The bound is the issue's: 40 x the 2.3e-7 its box prototype measured; the tetrahedra needed no widening.
ODE_RTOL = 1e-5


@pytest.mark.parametrize("name", tc.ISSUE_NAMES)
def test_against_ode_integrator(name):
    from scipy.integrate import solve_ivp
    c, u, r = tc.case(name), tc.oracle_flux(name), tc.oracle_paths(name)
    worst = 0.0
    for fld in (0, 2):
        for p in (0, 1, 2):
            def outflow(t, y):
                return y[2]
            outflow.terminal, outflow.direction = True, -1
            T = r["T"][fld, p]
            s = solve_ivp(lambda t, y: tr.velocity(c.mesh, u[fld], y), (0.0, 10 * T), c.x0[p], method="DOP853", rtol=1e-10,
                          atol=1e-12, events=outflow)
            assert len(s.t_events[0]) == 1 and r["status"][fld, p] == tr.EXITED
            worst = max(worst, abs(s.t_events[0][0] - T) / T)
            assert np.abs(s.y_events[0][0][:2] - r["x_exit"][fld, p, :2]).max() <= 1e-4 * c.extent.max()
    print(f"{name}: max relative difference to solve_ivp {worst:.3g}")
    assert worst <= ODE_RTOL


@pytest.mark.parametrize("name", tc.NAMES)
def test_margin_cap_and_paths(name):
    c, r = tc.case(name), tc.oracle_paths(name)
    keep = tc.kept(r["margin"])                        # asserts the 2 % cap
    assert keep.shape == (4, len(c.x0))
    assert (r["status"] == tr.EXITED).all()            # the flow leaves through the bottom ...
    attr = c.space.faces.face_bdr_attr[r["exit_face"]]
    if name == "tet3":                                 # ... or, in a start cell whose discrete flux points out, through the top
        assert np.isin(attr, (1, 6)).all() and (attr == 1).mean() > 0.95 and (r["nsteps"][attr == 6] == 1).all()
    else:
        assert (attr == 1).all()
    assert r["nsteps"].max() < tr.default_max_steps(c.mesh.n_elem)
    assert (r["T"] > 0).all()


def test_recorded_tolerances():
    """TOL_K and TOL_E of tracer_cases.py are what their method measures: not below it, and not more than 4 x above"""
    rounding = max(tc.rounding_deviation(n) for n in tc.NAMES)
    change = max(tc.perturbation_change(n) for n in tc.NAMES)
    print(f"float64 vs long double twin {rounding:.3g}; T under a 1e-8 flux perturbation {change:.3g}")
    assert tc.ROUNDING_RAW / 4 <= rounding <= tc.ROUNDING_RAW
    assert tc.PERTURBATION_RAW / 4 <= change <= tc.PERTURBATION_RAW


def test_statuses():
    c, u = tc.case("hex1"), tc.oracle_flux("hex1")[0]
    full = tc.oracle_paths("hex1")
    one = tr.trace(c.mesh, u, c.x0, c.elem0, max_steps=1)
    assert (one["status"] == tr.MAX_STEPS).all() and (one["nsteps"] == 1).all() and (one["exit_face"] == -1).all()
    assert (one["T"] > 0).all() and (one["T"] < full["T"][0]).all()
    still = tr.trace(c.mesh, np.zeros_like(u), c.x0, c.elem0)
    assert (still["status"] == tr.STAGNANT).all() and (still["T"] == 0).all() and (still["nsteps"] == 0).all()
    assert (still["x_exit"] == c.x0).all()
    q, nex = tr.reduce(still["T"], still["status"])
    assert q[0] == 0.0 and nex[0] == len(c.x0)
    # reversed flow: the start cells flow out through the inflow face, one step
    back = tr.trace(c.mesh, -u, c.x0, c.elem0)
    assert (back["status"] == tr.EXITED).all() and (back["nsteps"] == 1).all()
    assert (c.space.faces.face_bdr_attr[back["exit_face"]] == 6).all()
    assert (back["x_exit"][:, 2] == c.extent[2]).all()


def test_locate_is_geometric():
    """the elements of a refined level are not numbered x-fastest: locate must not assume they are"""
    c = tc.case("hex0")
    lo, hi = c.mesh.geom[:, :3], c.mesh.geom[:, 3:]
    assert ((lo[c.elem0] <= c.x0) & (c.x0 <= hi[c.elem0])).all()
    n, h = 8, c.extent / 8
    ijk = np.floor(c.x0 / h).astype(int)
    xfast = (ijk[:, 2] * n + ijk[:, 1]) * n + ijk[:, 0]
    assert (xfast != c.elem0).any()
    t = tc.case("tet2")
    rows, _ = tr.simplex_rows(t.mesh.geom)
    lam = np.einsum("pik,pk->pi", rows[t.elem0][:, :, :3], t.x0) + rows[t.elem0][:, :, 3]
    assert lam.min() >= -1e-12
    with pytest.raises(ValueError):
        tr.locate(c.mesh, [[0.5, 0.5, 2.5]])


def test_tracer_mesh_refuses_2d():
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    with pytest.raises(ValueError):
        tr.tracer_mesh(build_hierarchy(box_mesh([2, 2], [1, 1], "quad"), 0).spaces[0])
    assert tr.default_max_steps(512) == 64 + 32 * 8 and tr.default_max_steps(513) == 64 + 32 * 9

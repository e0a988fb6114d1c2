"""The numpy twin of the solute transport (parelagmc_amd/fe/transport.py): plug flow against the binomial distribution, bounds,
mass balance, the structures it refuses, the special columns, the recorded tolerances, and the new C symbols (no GPU
needed)."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import derivative_family_cases as dfc
import tracer_cases as trc
import transport_cases as tc
from conftest import ROOT
from parelagmc_amd import capi
from parelagmc_amd.fe import transport as tw

NEW_SYMBOLS = ("pmc_transport_create", "pmc_transport_destroy", "pmc_transport_size", "pmc_transport_run", "pmc_transport_reduce",
               "pmc_darcy_set_transport")
ULP = 2.0 ** -52


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in exported, s
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    assert "#define PMC_ABI_VERSION 3 " in header
    assert lib.pmc_abi_version() == 3
    for name in ("pmc_transport_mesh", "pmc_transport_params"):
        assert re.search(r"typedef struct %s\b" % name, text) and hasattr(capi, name), name
    hpp = open(os.path.join(ROOT, "parelagmc_amd", "host", "parelagmc.hpp")).read()
    assert "class SoluteTransport" in hpp and "void SetTransport(" in hpp
    assert hasattr(capi.DarcySolver, "SetTransport")
    t = capi.Transport
    assert (t.OK, t.STEP_LIMIT, t.BAD_FLUX, t.MASS_OUT, t.STORED) == (tw.OK, tw.STEP_LIMIT, tw.BAD_FLUX, tw.MASS_OUT, tw.STORED)
    assert hasattr(t, "Run") and hasattr(t, "Reduce")


@pytest.mark.parametrize("name", ["hex0", "stretch"])
def test_plug_flow(name):
    """k == 1: uniform flow from the top face down.  A cell in layer j from the inflow face has c = P(Binomial(n, nu) >= j + 1)
    after n steps, nu = dt v / (phi h_z); with one report per step the curve is what entered minus what is in place."""
    from oracle.darcy_oracle import DarcyOracle
    from scipy.stats import binom
    c, geo = tc.case(name), trc.case(name)
    u = DarcyOracle(tc.problem(c.kind)).solve_fwd(c.level, np.ones(c.mesh.n_elem), True)[2][:c.mesh.n_face]
    ext = geo.extent
    lo, hi = geo.mesh.geom[:, 2], geo.mesh.geom[:, 5]
    hz = hi[0] - lo[0]
    layer = np.rint((ext[2] - hi) / hz).astype(int)
    rate_in = float(tw.inflow_mass_rate(c.mesh, u)[0])
    v = rate_in / (ext[0] * ext[1])
    t_end = 0.6 * c.mesh.pore_volume.sum() / rate_in
    n = int(tw.plan(c.mesh, u, t_end, tc.CFL)["nsteps"][0])
    r = tw.advance(c.mesh, u, t_end, tc.CFL, nreport=n)
    assert r["status"][0] == tw.OK and r["nsteps"][0] == n
    nu = float(r["dt"][0]) * v / (tc.POROSITY * hz)
    expect = binom.sf(layer, n, nu)                      # P(X >= layer + 1)
    err = np.abs(r["c"][0] - expect).max()
    print(f"{name}: {n} steps, nu {nu:.4f}, largest |c - binomial| {err:.3g}")
    assert err <= 1e-11
    area_vol = np.bincount(layer, weights=c.mesh.pore_volume)                  # pore volume per layer
    steps = np.arange(1, n + 1)
    in_place = np.array([(area_vol * binom.sf(np.arange(len(area_vol)), m, nu)).sum() for m in steps])
    curve = rate_in * steps * float(r["dt"][0]) - in_place
    assert np.abs(r["curve"][0] - curve).max() <= 1e-11 * rate_in * t_end
    assert abs(r["stored"][0] - in_place[-1]) <= 1e-11 * rate_in * t_end


@pytest.mark.parametrize("name", tc.NAMES)
@pytest.mark.parametrize("nreport", [tc.NREPORT, 1])
def test_bounds_and_mass_balance(name, nreport):
    c, r = tc.case(name), tc.twin(name, nreport)
    assert r["c"].shape == (5, c.mesh.n_elem) and r["curve"].shape == (5, nreport)
    assert (r["c"] >= 0).all() and (r["c"] <= 1 + 4 * ULP).all()
    assert (np.diff(r["curve"], axis=1) >= 0).all() and (r["curve"] >= 0).all()
    assert (r["status"] == tw.OK).all() and (r["t_reached"] == c.t_end).all()
    # every boundary dof is an outlet: what entered = what left + what is in place (c0 = 0)
    inj = tc.injected(c.mesh, c.u, r["t_reached"])
    bal = np.abs(inj - r["curve"][:, -1] - r["stored"])[:4] / inj[:4]
    print(f"{name} nreport {nreport}: steps {r['nsteps']}, margins {np.array2string(r['margin'], precision=3)}, "
          f"mass balance {bal.max():.3g}")
    assert bal.max() <= 1e-12
    # the last report is the same whatever nreport is; stored is the pore volumes' dot product with c
    assert np.array_equal(r["curve"][:, -1], tc.twin(name, tc.NREPORT)["curve"][:, -1])
    assert np.abs(r["stored"] - r["c"] @ c.mesh.pore_volume).max() <= 1e-13 * c.mesh.pore_volume.sum()
    assert tc.kept(r["margin"]).sum() >= 4 and tc.kept(r["margin"], tc.MARGIN_E).sum() >= 4
    # the zero-flux column: one step in which nothing moves
    assert r["rate"][4] == 0 and r["nsteps"][4] == 1 and (r["c"][4] == 0).all() and (r["curve"][4] == 0).all()
    if name in ("quad1", "agg2_2"):
        assert r["nsteps"][:4].max() < tc.NREPORT                  # several reports fall into one step


def test_reports_interpolate_within_a_step():
    """report r of nreport lies at r t_end / nreport: the curve of 16 reports, read at every fourth, is the curve of 4, and
    inside one step it is linear"""
    for name in ("hex1", "agg2_2"):
        c = tc.case(name)
        fine = tc.twin(name, 16)
        coarse = tw.advance(c.mesh, c.u, c.t_end, tc.CFL, 4)
        assert np.abs(fine["curve"][:, 3::4] - coarse["curve"]).max() <= 1e-14 * c.mesh.pore_volume.sum()
    n_r, num = tw.report_steps(3, 16)
    assert list(n_r) == [0] * 5 + [1] * 5 + [2] * 6 and num[-1] == 16 and num[4] == 15 and num[5] == 2
    n_r, num = tw.report_steps(7, 1)
    assert list(n_r) == [6] and list(num) == [1]


def test_structures_that_are_refused():
    vol2 = tc.volumes("agg2", 2)
    smoothed = dfc.problem("agg2s").levels[2]
    assert np.bincount(smoothed.B.tocsr().indices).max() > 2
    with pytest.raises(ValueError):
        tw.transport_mesh(smoothed, vol2)
    from parelagmc_amd.fe.agglomerate import build_agglomerated_darcy_problem
    nonunit = build_agglomerated_darcy_problem(dfc.tet_spaces(2), dfc.NLEVELS_AGG, *dfc.BC_3D, ps_weights="nonunit")
    with pytest.raises(ValueError):
        tw.transport_mesh(nonunit.levels[1], tc.volumes("agg2", 1))
    tw.transport_mesh(dfc.problem("agg2").levels[2], vol2)           # the unsmoothed unit-weight level passes


def test_refusals():
    c = tc.case("quad0")
    tw.validate(c.mesh)
    for label, m in tc.bad_meshes(c.mesh):
        with pytest.raises(ValueError):
            tw.validate(m)
            pytest.fail(label)
    good = dict(t_end=c.t_end, cfl=tc.CFL, nreport=4, max_steps=0)
    for bad in tc.BAD_PARAMS:
        with pytest.raises(ValueError):
            tw.advance(c.mesh, c.u, **dict(good, **bad))
    tw.advance(c.mesh, c.u[:1], **dict(good, cfl=1.0, nreport=4096, max_steps=2 ** 24))
    with pytest.raises(ValueError):
        tw.reduce(np.zeros((1, 4)), np.zeros(1), kind=2)
    with pytest.raises(ValueError):
        tw.transport_mesh(c.dlevel, tc.volumes(c.kind, c.level), porosity=0.0)
    m = tw.transport_mesh(c.dlevel, tc.volumes(c.kind, c.level), tc.POROSITY, outlet=tw.validate(c.mesh).boundary, c_in=np.ones(c.mesh.n_face),
                          c0=np.zeros(c.mesh.n_elem), weight=c.mesh.pore_volume)
    r, ref = tw.advance(m, c.u, c.t_end, tc.CFL, 4), tw.advance(c.mesh, c.u, c.t_end, tc.CFL, 4)
    assert all(np.array_equal(r[k], ref[k]) for k in r)              # the defaults, spelled out


def test_special_columns():
    c, full = tc.case("hex1"), tc.twin("hex1")
    # STEP_LIMIT: max_steps steps of dt = cfl / rate
    r = tw.advance(c.mesh, c.u, c.t_end, tc.CFL, 4, max_steps=10)
    long = full["nsteps"] > 10
    assert long[:4].all() and not long[4]
    assert (r["status"][long] == tw.STEP_LIMIT).all() and (r["nsteps"][long] == 10).all() and r["status"][4] == tw.OK
    assert np.array_equal(r["dt"][long], tc.CFL / r["rate"][long]) and np.array_equal(r["t_reached"][long], 10 * r["dt"][long])
    assert (r["t_reached"][long] < c.t_end).all() and np.array_equal(r["rate"], full["rate"])
    inj = tc.injected(c.mesh, c.u, r["t_reached"])
    assert (np.abs(inj - r["curve"][:, -1] - r["stored"])[long] <= 1e-12 * inj[long]).all()
    p = tw.plan(c.mesh, c.u, c.t_end, tc.CFL, max_steps=10)
    assert all(np.array_equal(p[k], r[k]) for k in p)
    # BAD_FLUX: no step, c = c0, a zero curve - beside columns that keep their bits
    u = c.u.copy()
    u[1, 7] = np.nan
    u[2, 9] = np.inf
    c0 = np.linspace(0.0, 0.5, c.mesh.n_elem)
    m = dataclasses.replace(c.mesh, c0=c0)
    r, ref = tw.advance(m, u, c.t_end, tc.CFL, 4), tw.advance(m, c.u, c.t_end, tc.CFL, 4)
    for b in (1, 2):
        assert r["status"][b] == tw.BAD_FLUX and r["nsteps"][b] == 0 and np.isinf(r["rate"][b]) and r["t_reached"][b] == 0
        assert np.array_equal(r["c"][b], c0) and (r["curve"][b] == 0).all()
        assert abs(r["stored"][b] - c0 @ c.mesh.pore_volume) <= 1e-14
    for b in (0, 3, 4):
        assert all(np.array_equal(r[k][b], ref[k][b]) for k in r)
    # zero flux: one step in which nothing moves, whatever c0 is
    assert r["nsteps"][4] == 1 and r["status"][4] == tw.OK and np.array_equal(r["c"][4], c0) and r["margin"][4] == 1.0
    assert np.array_equal(tw.reduce(r["curve"], r["stored"], tw.MASS_OUT), r["curve"][:, -1])
    assert np.array_equal(tw.reduce(r["curve"], r["stored"], tw.STORED), r["stored"])


def test_tree_sum_is_the_device_order():
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 256, 257, 1000):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        assert abs(tw.tree_sum(v) - np.sum(v.astype(np.longdouble))) <= 4 * ULP * np.abs(v).sum()
    v = np.zeros(512)
    v[[0, 256]] = 1.0, 2.0 ** -53          # thread 0 adds both first: the small term is lost there
    assert tw.tree_sum(v) == 1.0
    v = np.zeros(512)
    v[[0, 1]] = 1.0, 2.0 ** -53
    assert tw.tree_sum(v) == 1.0


def test_recorded_tolerances():
    """TOL_K and TOL_E of transport_cases.py are what their method measures: not below it, and not more than 4 x above"""
    rounding = max(tc.rounding_deviation(n) for n in tc.NAMES)
    change = max(tc.perturbation_change(n) for n in tc.NAMES)
    print(f"float64 vs long double twin {rounding:.3g}; results under a 1e-8 flux perturbation {change:.3g}")
    assert tc.ROUNDING_RAW / 4 <= rounding <= tc.ROUNDING_RAW
    assert tc.PERTURBATION_RAW / 4 <= change <= tc.PERTURBATION_RAW
    assert tc.TOL_K == 16 * tc.ROUNDING_RAW and tc.TOL_E == 10 * tc.PERTURBATION_RAW

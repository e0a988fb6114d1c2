"""Upwind solute transport on the device (pmc_transport_*, pmc_darcy_set_transport; csrc/transport.hip) against the numpy twin
(parelagmc_amd/fe/transport.py): values on every element family, bitwise reproducibility, the SolveFwd hook, the direct-solve
oracle end to end, the managers' plumbing and the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import derivative_family_cases as dfc
import tracer_cases as trc
import transport_cases as tc
from parelagmc_amd.fe import transport as tw

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
TIGHT_AGG = dict(TIGHT, max_iter=600)          # the iteration limit of tests/test_gpu_agglomerated.py
# kernel against twin on the same flux: 16 x the largest deviation of the float64 twin from the long-double twin on the shared
# cases (4.2e-15, transport_cases.rounding_deviation; test_transport_twin.py re-measures it)
TOL_K = tc.TOL_K
# device solve + transport against the twin on the oracle's direct-solve flux: 10 x the twin's largest change under a 1e-8
# relative perturbation of that flux (7.7e-8, transport_cases.perturbation_change)
TOL_E = tc.TOL_E
KEYS = ("c", "curve", "stored", "rate", "t_reached", "nsteps", "status")
# (case, hybridized handle): the hooked solves
HOOKED = [("hex0", False), ("quad0", False), ("hex0", True), ("agg3_1", False)]

_transports = {}
_solvers = {}
_hooked = {}


def transport_for(gpu_ctx, name, nreport=tc.NREPORT):
    from parelagmc_amd import capi
    if (name, nreport) not in _transports:
        c = tc.case(name)
        _transports[name, nreport] = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, nreport)
    return _transports[name, nreport]


def solver(gpu_ctx, kind, hybrid=False):
    from parelagmc_amd import capi
    if (kind, hybrid) not in _solvers:
        opts = capi.solver_opts(**(TIGHT_AGG if kind.startswith("agg") else TIGHT))
        _solvers[kind, hybrid] = capi.DarcySolver(gpu_ctx, tc.problem(kind), opts, hybrid=hybrid)
    return _solvers[kind, hybrid]


def on_host(r):
    """the dict of Transport.Run as numpy arrays in the shapes of a host-memory call"""
    if isinstance(r["curve"], np.ndarray):
        return r
    nb = r["stored"].n
    return {k: v.download().reshape(nb, -1) if k in ("c", "curve") else v.download() for k, v in r.items()}


def same(a, b, rows_a, rows_b, keys=KEYS):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in keys)


def against_twin(c, got, ref, cols, keep, tol, what):
    """nsteps and status equal on the kept columns, c / curve / stored within tol (transport_cases.deviation)"""
    sub = {k: np.asarray(v)[cols] for k, v in ref.items()}
    keep = keep[cols]
    assert np.array_equal(got["nsteps"][keep], sub["nsteps"][keep]) and np.array_equal(got["status"][keep], sub["status"][keep]), what
    d = tc.deviation(c.mesh, c.u[cols], got, sub, keep)
    print(f"{what}: largest deviation {d:.3g} (tolerance {tol:.3g})")
    assert d <= tol, (what, d)


@pytest.mark.parametrize("name", tc.NAMES)
def test_run_matches_twin(gpu_ctx, name):
    c = tc.case(name)
    for nreport in (tc.NREPORT, 1):
        t, ref = transport_for(gpu_ctx, name, nreport), tc.twin(name, nreport)
        assert (t.n_elem, t.n_face, t.nreport) == (c.mesh.n_elem, c.mesh.n_face, nreport)
        assert t.n_outlet == int(tw.validate(c.mesh).boundary.sum())
        keep = tc.kept(ref["margin"])
        for cols in ([3], [1, 4, 3], [0, 1, 2, 3, 4]):
            u = np.ascontiguousarray(c.u[cols])
            host = t.Run(u)
            dev = on_host(t.Run(gpu_ctx.array(u), nbatch=len(cols)))
            assert same(host, dev, slice(None), slice(None))
            assert np.array_equal(host["rate"], ref["rate"][cols])                       # to the bit
            assert np.array_equal(host["t_reached"][keep[cols]], ref["t_reached"][cols][keep[cols]])
            against_twin(c, host, ref, cols, keep, TOL_K, f"{name} nreport {nreport} columns {cols}")
            lean = t.Run(u, want_c=False)                                                # c_out == NULL
            assert "c" not in lean and same(host, lean, slice(None), slice(None), KEYS[1:])
            assert np.array_equal(t.Reduce(host["curve"], host["stored"], t.MASS_OUT), host["curve"][:, -1])
            assert np.array_equal(t.Reduce(host["curve"], host["stored"], t.STORED), host["stored"])


@pytest.mark.parametrize("name", ["hex1", "quad0", "agg3_1"])
def test_bitwise(gpu_ctx, name):
    c, t = tc.case(name), transport_for(gpu_ctx, name)
    full = t.Run(c.u)
    assert set(full["nsteps"][:4] % 2) == {0, 1}                     # final results in both buffers, beside the one-step column
    assert same(full, t.Run(c.u), slice(None), slice(None))                                # two identical calls
    for b in range(5):
        assert same(full, t.Run(c.u[b:b + 1]), [b], [0]), b                                # nb = 1
    assert same(full, t.Run(c.u[[4, 2, 0]]), [4, 2, 0], [0, 1, 2])                         # nb = 3, other neighbours
    many = np.stack([c.u[i % 5] for i in range(67)])                                        # more than one wave of columns
    wide = t.Run(many)
    assert same(wide, full, slice(None), [i % 5 for i in range(67)])
    dev = t.Run(gpu_ctx.array(c.u), nbatch=5)                                              # device memory
    assert same(full, on_host(dev), slice(None), slice(None))
    strided = np.zeros((5, c.mesh.n_face + 7))                                             # a row stride above n_face
    strided[:, :c.mesh.n_face] = c.u
    assert same(full, t.Run(strided), slice(None), slice(None))
    for kind in (t.MASS_OUT, t.STORED):
        assert np.array_equal(t.Reduce(full["curve"], full["stored"], kind), t.Reduce(dev["curve"], dev["stored"], kind))


def test_special_columns(gpu_ctx):
    from parelagmc_amd import capi
    c = tc.case("hex1")
    short = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4, max_steps=10)
    r, ref = short.Run(c.u), tw.advance(c.mesh, c.u, c.t_end, tc.CFL, 4, max_steps=10)
    assert (r["status"][:4] == short.STEP_LIMIT).all() and (r["nsteps"][:4] == 10).all() and r["status"][4] == short.OK
    for key in ("rate", "t_reached", "nsteps", "status"):
        assert np.array_equal(r[key], ref[key]), key
    against_twin(c, r, ref, [0, 1, 2, 3, 4], np.ones(5, bool), TOL_K, "STEP_LIMIT")
    short.close()
    u = c.u.copy()
    u[1, 7], u[2, 9] = np.nan, np.inf
    c0 = np.linspace(0.0, 0.5, c.mesh.n_elem)
    m = dataclasses.replace(c.mesh, c0=c0)
    t = capi.Transport(gpu_ctx, m, c.t_end, tc.CFL, 4)
    r, clean, ref = t.Run(u), t.Run(c.u), tw.advance(m, u, c.t_end, tc.CFL, 4)
    for b in (1, 2):
        assert r["status"][b] == t.BAD_FLUX and r["nsteps"][b] == 0 and np.isinf(r["rate"][b]) and r["t_reached"][b] == 0
        assert np.array_equal(r["c"][b], c0) and (r["curve"][b] == 0).all() and abs(r["stored"][b] - ref["stored"][b]) <= 1e-14
    assert same(r, clean, [0, 3, 4], [0, 3, 4])                     # the good columns keep their bits beside the bad ones
    assert r["nsteps"][4] == 1 and np.array_equal(r["c"][4], c0)    # zero flux: one step in which nothing moves
    against_twin(dataclasses.replace(c, mesh=m), clean, tw.advance(m, c.u, c.t_end, tc.CFL, 4), [0, 1, 2, 3, 4], np.ones(5, bool),
                 TOL_K, "c0 != 0")
    t.close()
    # an outlet mask, inflow concentrations and weights of the caller's
    s = tw.validate(c.mesh)
    rng = np.random.default_rng(11)
    outlet = s.boundary & (rng.random(c.mesh.n_face) < 0.5)
    m = dataclasses.replace(c.mesh, outlet=outlet.astype(np.uint8), c_in=rng.uniform(0.2, 1.0, c.mesh.n_face),
                            weight=rng.uniform(0.0, 1.0, c.mesh.n_elem))
    t = capi.Transport(gpu_ctx, m, c.t_end, tc.CFL, 7)
    assert t.n_outlet == int(outlet.sum())
    r, ref = t.Run(c.u), tw.advance(m, c.u, c.t_end, tc.CFL, 7)
    against_twin(dataclasses.replace(c, mesh=m), r, ref, [0, 1, 2, 3, 4], tc.kept(ref["margin"]), TOL_K, "outlet mask")
    t.close()


def observations(c):
    import scipy.sparse as sp
    if c.kind == "hex":
        n_p = c.mesh.n_elem
        return sp.csr_matrix((np.ones(4), ([0, 0, 1, 1], [3, 4, n_p - 2, n_p - 1])), shape=(2, n_p))
    return dfc.observations(c.kind, c.level)


def hooked(gpu_ctx, name, hybrid):
    """the hooked solves of a case's four fields on one handle: Q of SolveFwd (with and without the solution) and of
    SolveFwd_RtnPressure for both kinds, ComputeG and the log-likelihood gradient with and without the attachment, and
    pmc_transport_run on the solution"""
    if (name, hybrid) not in _hooked:
        c = tc.case(name)
        ds, t = solver(gpu_ctx, c.kind, hybrid), transport_for(gpu_ctx, name)
        ds.SetObservations(c.level, observations(c))
        data = np.full(2, 0.1)

        def others():
            G, _, Qg = ds.ComputeG(c.level, c.k)
            ll, Gl, grad = ds.loglik_gradient(c.level, c.k, data, 0.01)
            return dict(G=G, Qg=Qg, ll=ll, Gl=Gl, grad=grad)

        out = dict(plain=ds.SolveFwd(c.level, c.k)[0], others_plain=others())
        for kind, tag in ((t.MASS_OUT, "out"), (t.STORED, "stored")):
            ds.SetTransport(c.level, t, kind)
            Q, _, sol = ds.SolveFwd(c.level, c.k, want_solution=True)
            out[tag] = dict(Q=Q, sol=sol, Q_nosol=ds.SolveFwd(c.level, c.k)[0], Qp=ds.SolveFwd_RtnPressure(c.level, c.k)[2])
        out["others_hooked"] = others()
        ds.SetTransport(c.level, None)
        out["detached"] = ds.SolveFwd(c.level, c.k)[0]
        out["run"] = t.Run(out["out"]["sol"])
        _hooked[name, hybrid] = out
    return _hooked[name, hybrid]


@pytest.mark.parametrize("name,hybrid", HOOKED)
def test_hooked_solves(gpu_ctx, name, hybrid):
    c, h, t = tc.case(name), hooked(gpu_ctx, name, hybrid), transport_for(gpu_ctx, name)
    run = h["run"]
    assert np.array_equal(h["out"]["sol"], h["stored"]["sol"])
    for tag, kind in (("out", t.MASS_OUT), ("stored", t.STORED)):
        q = t.Reduce(run["curve"], run["stored"], kind)
        for key in ("Q", "Q_nosol", "Qp"):
            assert np.array_equal(h[tag][key], q), (tag, key)                   # bit for bit
    assert (h["out"]["Q"] > 0).all() and (h["stored"]["Q"] > 0).all()
    assert not np.array_equal(h["out"]["Q"], h["plain"])
    for key, v in h["others_plain"].items():
        assert np.array_equal(v, h["others_hooked"][key]), key                   # ComputeG and the gradient keep <obs, x>
    assert np.array_equal(h["detached"], h["plain"])                             # detaching restores every bit


@pytest.mark.parametrize("name,hybrid", HOOKED)
def test_end_to_end_against_the_oracle(gpu_ctx, name, hybrid):
    c, h, ref = tc.case(name), hooked(gpu_ctx, name, hybrid), tc.twin(name)
    keep = tc.kept(ref["margin"], tc.MARGIN_E)
    flux = np.abs(h["out"]["sol"][:, :c.mesh.n_face] - c.u[:4]).max() / np.abs(c.u[:4]).max()
    print(f"{name} hybrid={hybrid}: flux differs from the oracle's by {flux:.3g} of its largest entry")
    against_twin(c, h["run"], ref, [0, 1, 2, 3], keep, TOL_E, f"{name} hybrid={hybrid}")


@pytest.mark.parametrize("nlanes", [1, 2])
def test_manager_sees_the_transport(nlanes):
    """MLMC_Manager::InitRun with a transport on both levels against a Python loop over Sample / Eval / hooked SolveFwd with the
    same realization ids: plumbing only (the values are checked above)"""
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_sampler_problem
    h, dp = trc.hierarchy("hex"), trc.problem("hex")
    sp = build_sampler_problem(h, corlen=0.1, lognormal=True)
    cases = [tc.case("hex0"), tc.case("hex1")]
    t_end = cases[0].t_end                                       # the same physical time on both levels
    ctxs = [capi.Context(0, seed=20261020) for _ in range(nlanes + 1)]
    sm = [capi.PDESampler(cx, sp, capi.solver_opts(**TIGHT)) for cx in ctxs]
    dr = [capi.DarcySolver(cx, dp, capi.solver_opts(**TIGHT)) for cx in ctxs]
    handles = [[capi.Transport(cx, cs.mesh, t_end, tc.CFL, 4) for cs in cases] for cx in ctxs]      # each lane holds its own
    for d, ts in zip(dr, handles):
        for lvl in (0, 1):
            d.SetTransport(lvl, ts[lvl], capi.Transport.MASS_OUT)
    mgr = host_api.MLMCManager(2, sampler=sm[0], solver=dr[0], wall_time=False, batch=4)
    for i in range(1, nlanes):
        mgr.add_lane(sm[i], dr[i])
    ns = [5, 9]
    r = mgr.InitRun(ns)
    s, d = sm[-1], dr[-1]                                        # the loop runs on handles of its own
    q1 = d.SolveFwd(1, s.Eval(1, s.Sample(1, 0, ns[1])))[0]
    xi = s.Sample(0, 0, ns[0])
    qf = d.SolveFwd(0, s.Eval(0, xi))[0]
    qc = d.SolveFwd(1, s.Eval(1, xi, xi_level=0))[0]
    eQ, eY = np.array([qf.mean(), q1.mean()]), np.array([(qf - qc).mean(), q1.mean()])
    assert list(r["nsamples"]) == ns
    assert np.abs(r["eQ"] / eQ - 1).max() <= 1e-12 and np.abs(r["eY"] - eY).max() <= 1e-12 * np.abs(eQ).max()
    pore = cases[0].mesh.pore_volume.sum()
    assert 0.05 * pore < eQ.min() and eQ.max() < 10 * pore      # a solute mass, not the boundary flux
    mgr.close()
    for cx in ctxs:
        cx.close()


def test_refusals(gpu_ctx):
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    c = tc.case("quad0")
    good = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4)
    ref = good.Run(c.u)

    def refused(fn, what=None):
        with pytest.raises(capi.PmcError) as e:
            fn()
        assert e.value.code == -1 and len(str(e.value)) > len("libpmc error -1: "), what
        assert same(good.Run(c.u), ref, slice(None), slice(None)), what      # the handle stays usable, with the same results

    params = dict(t_end=c.t_end, cfl=tc.CFL, nreport=4, max_steps=0)
    for label, m in tc.bad_meshes(c.mesh):
        refused(lambda: capi.Transport(gpu_ctx, m, **params), label)
    for bad in tc.BAD_PARAMS:
        refused(lambda: capi.Transport(gpu_ctx, c.mesh, **dict(params, **bad)), bad)
    # NULL arguments through the raw entry
    keep = capi._Keep()
    mesh = capi.pmc_transport_mesh(c.mesh.n_elem, c.mesh.n_face, keep.i32(c.mesh.rowptr), keep.i32(c.mesh.col), keep.f64(c.mesh.val),
                                   keep.f64(c.mesh.pore_volume), None, None, None, None)
    prm = capi.pmc_transport_params(c.t_end, tc.CFL, 4, 0)
    h = C.c_void_p()
    assert lib.pmc_transport_create(gpu_ctx.h, C.byref(mesh), C.byref(prm), C.byref(h)) == 0 and h.value
    lib.pmc_transport_destroy(h)
    h = C.c_void_p()
    assert lib.pmc_transport_create(None, C.byref(mesh), C.byref(prm), C.byref(h)) == -1 and not h.value
    assert lib.pmc_transport_create(gpu_ctx.h, None, C.byref(prm), C.byref(h)) == -1 and not h.value
    assert lib.pmc_transport_create(gpu_ctx.h, C.byref(mesh), None, C.byref(h)) == -1 and not h.value
    assert lib.pmc_transport_create(gpu_ctx.h, C.byref(mesh), C.byref(prm), None) == -1
    for name in ("rowptr", "col", "val", "pore_volume"):
        broken = capi.pmc_transport_mesh.from_buffer_copy(mesh)
        setattr(broken, name, None)
        assert lib.pmc_transport_create(gpu_ctx.h, C.byref(broken), C.byref(prm), C.byref(h)) == -1 and not h.value, name
    assert lib.pmc_transport_size(None, None, None, None, None) == -1
    # run / reduce: a refused call writes nothing
    u = np.ascontiguousarray(c.u[:1])
    f = {k: np.full(n, -7.0) for k, n in (("c", c.mesh.n_elem), ("curve", 4), ("stored", 1), ("rate", 1), ("t", 1))}
    i2 = [np.full(1, -7, np.int32) for _ in range(2)]

    def run(nb=1, pu=u.ctypes.data, ld=u.shape[1], curve=f["curve"].ctypes.data, ms=0):
        return lib.pmc_transport_run(good.h, nb, pu, ld, f["c"].ctypes.data, curve, f["stored"].ctypes.data, f["rate"].ctypes.data,
                                     f["t"].ctypes.data, i2[0].ctypes.data, i2[1].ctypes.data, ms)

    assert run(nb=0) == -1 and run(pu=None) == -1 and run(ld=u.shape[1] - 1) == -1 and run(curve=None) == -1 and run(ms=7) == -1
    assert lib.pmc_transport_run(None, 1, u.ctypes.data, u.shape[1], None, f["curve"].ctypes.data, f["stored"].ctypes.data,
                                 f["rate"].ctypes.data, f["t"].ctypes.data, i2[0].ctypes.data, i2[1].ctypes.data, 0) == -1
    assert all((a == -7).all() for a in list(f.values()) + i2)
    assert run() == 0 and np.array_equal(f["curve"], ref["curve"][0]) and np.array_equal(f["c"], ref["c"][0])
    refused(lambda: good.Reduce(ref["curve"], ref["stored"], kind=2))
    refused(lambda: good.Reduce(ref["curve"][:0], ref["stored"][:0]))
    Q = np.zeros(1)
    assert lib.pmc_transport_reduce(good.h, 1, ref["curve"].ctypes.data, ref["stored"].ctypes.data, 0, capi._ptr(Q, C.c_double), 7) == -1
    assert lib.pmc_transport_reduce(good.h, 1, None, ref["stored"].ctypes.data, 0, capi._ptr(Q, C.c_double), 0) == -1
    # set_transport: what set_tracer refuses, and a level holds a tracer or a transport, not both
    ds = solver(gpu_ctx, "quad")
    Q0 = ds.SolveFwd(0, c.k[:1])[0]
    refused(lambda: ds.SetTransport(2, good))
    refused(lambda: ds.SetTransport(-1, good))
    refused(lambda: ds.SetTransport(1, good))                                     # the level-0 mesh on level 1
    refused(lambda: ds.SetTransport(0, good, kind=5))
    assert lib.pmc_darcy_set_transport(None, 0, good.h, 0) == -1
    assert np.array_equal(ds.SolveFwd(0, c.k[:1])[0], Q0)                         # nothing was attached
    hx, hc = trc.case("hex1"), tc.case("hex1")
    dh = solver(gpu_ctx, "hex")
    tracer = capi.Tracer(gpu_ctx, hx.mesh, hx.x0, hx.elem0)
    tr_h = transport_for(gpu_ctx, "hex1")
    Qplain = dh.SolveFwd(1, hc.k[:1])[0]
    dh.SetTracer(1, tracer)
    Qtracer = dh.SolveFwd(1, hc.k[:1])[0]
    with pytest.raises(capi.PmcError):
        dh.SetTransport(1, tr_h)
    assert np.array_equal(dh.SolveFwd(1, hc.k[:1])[0], Qtracer)                   # the tracer is still the level's QoI
    dh.SetTracer(1, None)
    dh.SetTransport(1, tr_h)
    Qtransport = dh.SolveFwd(1, hc.k[:1])[0]
    with pytest.raises(capi.PmcError):
        dh.SetTracer(1, tracer)
    assert np.array_equal(dh.SolveFwd(1, hc.k[:1])[0], Qtransport)
    dh.SetTransport(1, None)
    assert np.array_equal(dh.SolveFwd(1, hc.k[:1])[0], Qplain)
    assert len({float(Qplain[0]), float(Qtracer[0]), float(Qtransport[0])}) == 3
    tracer.close()
    good.close()

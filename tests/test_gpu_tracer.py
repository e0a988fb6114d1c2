"""Particle travel times on the device (pmc_tracer_*, pmc_darcy_set_tracer; csrc/tracer.hip) against the numpy twin
(parelagmc_amd/fe/tracer.py) and the direct-solve oracle: values, bitwise reproducibility, statuses, the SolveFwd hook, the
managers' plumbing and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tracer_cases as tc
from parelagmc_amd.fe import tracer as tr

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
# kernel against twin on the same flux: 16 x the largest deviation of the float64 twin from the long-double twin on the
# shared cases (7.1e-14, measured on the CPU by tracer_cases.rounding_deviation; test_tracer_twin.py re-measures it)
TOL_K = tc.TOL_K
# device solve + walk against the twin on the oracle's direct-solve flux: 10 x the twin's largest relative change of T under a
# 1e-8 relative perturbation of that flux (5.5e-6, tracer_cases.perturbation_change)
TOL_E = tc.TOL_E
KEYS = ("T", "exit_face", "status", "nsteps", "x_exit")

_solvers = {}
_solved = {}


def solver(gpu_ctx, kind, hybrid=False):
    from parelagmc_amd import capi
    if (kind, hybrid) not in _solvers:
        _solvers[kind, hybrid] = capi.DarcySolver(gpu_ctx, tc.problem(kind), capi.solver_opts(**TIGHT), hybrid=hybrid)
    return _solvers[kind, hybrid]


def tracer_for(gpu_ctx, name, **kw):
    from parelagmc_amd import capi
    c = tc.case(name)
    return capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0, **kw)


def solved(gpu_ctx, name, hybrid=False):
    """one hooked SolveFwd of the case's four fields: Q (MEAN), the solution, and pmc_tracer_run on that solution"""
    if (name, hybrid) not in _solved:
        c = tc.case(name)
        ds = solver(gpu_ctx, c.kind, hybrid)
        t = tracer_for(gpu_ctx, name)
        ds.SetTracer(c.level, t, t.MEAN)
        Q, _, sol = ds.SolveFwd(c.level, c.k, want_solution=True)
        Q_nosol, _ = ds.SolveFwd(c.level, c.k)
        ds.SetTracer(c.level, t, t.MIN)
        Qmin, _ = ds.SolveFwd(c.level, c.k)
        ds.SetTracer(c.level, None)
        _solved[name, hybrid] = dict(Q=Q, Q_nosol=Q_nosol, Qmin=Qmin, sol=sol, run=t.Run(sol), tracer=t)
    return _solved[name, hybrid]


def compare_paths(got, ref, keep, tol, extent, what):
    """status, exit face and step count equal, T within tol (relative) and x_exit within tol of the domain's extent"""
    for key in ("status", "exit_face", "nsteps"):
        assert (got[key] == ref[key])[keep].all(), (what, key)
    dT = (np.abs(got["T"] - ref["T"]) / ref["T"])[keep].max()
    dx = (np.abs(got["x_exit"] - ref["x_exit"]).max(axis=2) / extent)[keep].max()
    print(f"{what}: max relative difference T {dT:.3g}, x_exit {dx:.3g} (tolerance {tol:.3g})")
    assert dT <= tol and dx <= tol, (what, dT, dx)


@pytest.mark.parametrize("name", tc.NAMES)
def test_kernel_matches_twin_on_the_library_flux(gpu_ctx, name):
    c, s = tc.case(name), solved(gpu_ctx, name)
    twin = tr.trace(c.mesh, s["sol"][:, :c.space.n_u], c.x0, c.elem0)
    compare_paths(s["run"], twin, tc.kept(twin["margin"]), TOL_K, c.extent.max(), name)


@pytest.mark.parametrize("name,hybrid", [(n, False) for n in tc.NAMES] + [("hex0", True), ("tet2", True)])
def test_end_to_end_against_the_oracle(gpu_ctx, name, hybrid):
    c, s, ref = tc.case(name), solved(gpu_ctx, name, hybrid), tc.oracle_paths(name)
    keep = tc.kept(ref["margin"])
    compare_paths(s["run"], ref, keep, TOL_E, c.extent.max(), f"{name} hybrid={hybrid}")
    # the hooked Q is the reduction of those paths, bit for bit, with and without sol_out, for MEAN and MIN
    t = s["tracer"]
    q, nex = t.Reduce(s["run"]["T"], s["run"]["status"], t.MEAN)
    qmin, _ = t.Reduce(s["run"]["T"], s["run"]["status"], t.MIN)
    assert (q == s["Q"]).all() and (q == s["Q_nosol"]).all() and (qmin == s["Qmin"]).all()
    assert (nex == 0).all() and (qmin == s["run"]["T"].min(axis=1)).all()
    assert np.abs(q / s["run"]["T"].mean(axis=1) - 1).max() < 1e-14


@pytest.mark.parametrize("path", tc.exact_paths(), ids=lambda p: p.name)
def test_exact_paths_on_the_device(gpu_ctx, path):
    from parelagmc_amd import capi
    t = capi.Tracer(gpu_ctx, path.mesh, path.x0, np.zeros(1, np.int32))
    r = t.Run(path.u[None, :])
    assert r["status"][0, 0] == t.EXITED and r["exit_face"][0, 0] == path.face and r["nsteps"][0, 0] == 1
    print(f"{path.name}: T relative error {abs(r['T'][0, 0] - path.T) / path.T:.3g} (tolerance {path.rtol:.3g})")
    assert abs(r["T"][0, 0] - path.T) <= path.rtol * path.T
    assert np.abs(r["x_exit"][0, 0] - path.x_exit).max() <= path.rtol
    t.close()


def same(a, b, rows_a, rows_b):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in KEYS)


@pytest.mark.parametrize("name", ["hex0", "tet2"])
def test_bitwise(gpu_ctx, name):
    c, s = tc.case(name), solved(gpu_ctx, name)
    t = s["tracer"]
    n_u = c.space.n_u
    u = np.stack([s["sol"][i % 4, :n_u] * (1.0 + 0.01 * (i // 4)) for i in range(67)])
    full = t.Run(u)
    assert same(full, t.Run(u), slice(None), slice(None))                                  # two identical calls
    for j in (0, 2, 66):
        assert same(full, t.Run(u[j:j + 1]), [j], [0])                                     # nb = 1
    assert same(full, t.Run(u[[5, 66, 1]]), [5, 66, 1], [0, 1, 2])                         # nb = 3, other neighbours
    dev = t.Run(gpu_ctx.array(u), nbatch=67)                                               # device memory
    assert same(full, {k: v.download().reshape(full[k].shape) for k, v in dev.items()}, slice(None), slice(None))
    wide = np.zeros((67, n_u + 5))                                                          # a row stride above n_face
    wide[:, :n_u] = u
    assert same(full, t.Run(wide), slice(None), slice(None))
    # sample-major against the interleaved path inside the solve is test_end_to_end_against_the_oracle's Q == Reduce(Run)
    q_host, _ = t.Reduce(full["T"], full["status"], t.MEAN)
    q_dev, _ = t.Reduce(dev["T"], dev["status"], t.MEAN)
    q_one, _ = t.Reduce(full["T"][66:], full["status"][66:], t.MEAN)
    assert (q_host == q_dev).all() and q_one[0] == q_host[66]


def test_statuses(gpu_ctx):
    from parelagmc_amd import capi
    for name in ("hex1", "tet1"):
        c, u = tc.case(name), tc.oracle_flux(name)
        one = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0, max_steps=1)
        r, twin = one.Run(u), tr.trace(c.mesh, u, c.x0, c.elem0, max_steps=1)
        assert (r["status"] == one.MAX_STEPS).all() and (r["nsteps"] == 1).all() and (r["exit_face"] == -1).all()
        assert np.abs(r["T"] / twin["T"] - 1).max() <= TOL_K
        q, nex = one.Reduce(r["T"], r["status"])
        assert (nex == len(c.x0)).all()
        one.close()
        t = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0)
        still = t.Run(np.zeros_like(u[:1]))
        assert (still["status"] == t.STAGNANT).all() and (still["T"] == 0).all() and (still["nsteps"] == 0).all()
        q, nex = t.Reduce(still["T"], still["status"], t.MEAN)
        assert q[0] == 0.0 and nex[0] == len(c.x0) == t.nparticles
        back = t.Run(-u[:1])                      # the start cells flow out through the inflow face
        assert (back["status"] == t.EXITED).all() and (c.space.faces.face_bdr_attr[back["exit_face"]] == 6).all()
        twin = tr.trace(c.mesh, -u[:1], c.x0, c.elem0)
        assert np.array_equal(back["nsteps"], twin["nsteps"])
        if c.mesh.kind == tr.BOX:                 # a tetrahedron under the inflow face may touch it with a vertex only
            assert (back["nsteps"] == 1).all()
        t.close()


def test_hook_leaves_everything_else_alone(gpu_ctx):
    import scipy.sparse as sp
    c = tc.case("hex0")
    ds, t = solver(gpu_ctx, c.kind), solved(gpu_ctx, "hex0")["tracer"]
    k = c.k[:3]
    n_p = c.space.n_s
    ds.SetObservations(c.level, sp.csr_matrix((np.ones(4), ([0, 0, 1, 1], [3, 4, n_p - 2, n_p - 1])), shape=(2, n_p)))

    def everything():
        Q, _ = ds.SolveFwd(c.level, k)
        Qs, _, sol = ds.SolveFwd(c.level, k, want_solution=True)
        P, _, Qp = ds.SolveFwd_RtnPressure(c.level, k)
        G, _, Qg = ds.ComputeG(c.level, k)
        Qd, _, grad = ds.solve_gradient(c.level, k)
        return dict(Q=Q, Qs=Qs, sol=sol, P=P, Qp=Qp, G=G, Qg=Qg, Qd=Qd, grad=grad)

    before = everything()
    ds.SetTracer(c.level, t, t.MEAN)
    hooked = everything()
    ds.SetTracer(c.level, None)
    after = everything()
    for key in before:
        assert np.array_equal(before[key], after[key]), key                    # detaching restores every bit
    for key in ("sol", "P", "G", "Qg", "Qd", "grad"):
        assert np.array_equal(before[key], hooked[key]), key                   # ComputeG and the gradient keep <obs, x>
    assert np.array_equal(hooked["Q"], hooked["Qs"]) and np.array_equal(hooked["Q"], hooked["Qp"])
    assert np.abs(hooked["Q"] / solved(gpu_ctx, "hex0")["Q"][:3] - 1).max() < 1e-6   # the travel time, whatever the batch
    assert not np.array_equal(hooked["Q"], before["Q"])


@pytest.mark.parametrize("nlanes", [1, 2])
def test_manager_sees_the_travel_time(nlanes):
    """MLMC_Manager::InitRun with tracers on both levels against a Python loop over Sample / Eval / hooked SolveFwd with the
    same realization ids: plumbing only (the values are checked above)"""
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_sampler_problem
    h, dp = tc.hierarchy("hex"), tc.problem("hex")
    sp = build_sampler_problem(h, corlen=0.1, lognormal=True)
    cases = [tc.case("hex0"), tc.case("hex1")]
    x0 = cases[1].x0                                             # the same physical starts on both levels
    ctxs = [capi.Context(0, seed=20261019) for _ in range(nlanes + 1)]
    sm = [capi.PDESampler(cx, sp, capi.solver_opts(**TIGHT)) for cx in ctxs]
    dr = [capi.DarcySolver(cx, dp, capi.solver_opts(**TIGHT)) for cx in ctxs]
    tracers = [[capi.Tracer(cx, cs.mesh, x0) for cs in cases] for cx in ctxs]      # each lane holds its own
    for d, ts in zip(dr, tracers):
        for lvl in (0, 1):
            d.SetTracer(lvl, ts[lvl], capi.Tracer.MEAN)
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
    assert eQ.min() > 0.5                                        # travel times, not the boundary flux
    mgr.close()
    for cx in ctxs:
        cx.close()


def test_refusals(gpu_ctx):
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    c, tet = tc.case("hex1"), tc.case("tet1")
    good = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0)
    u = tc.oracle_flux("hex1")
    ref = good.Run(u)

    def refused(fn):
        with pytest.raises(capi.PmcError) as e:
            fn()
        assert e.value.code == -1
        now = good.Run(u)                                        # the handle stays usable, with the same results
        assert all(np.array_equal(now[k], ref[k]) for k in KEYS)

    import copy
    import dataclasses

    def create(mesh=c.mesh, x0=c.x0, elem0=c.elem0, **kw):
        capi.Tracer(gpu_ctx, mesh, x0, elem0, **kw)

    def changed(mesh, **kw):
        return dataclasses.replace(mesh, **{k: copy.deepcopy(v) for k, v in kw.items()})

    refused(lambda: create(changed(c.mesh, kind=2)))
    refused(lambda: create(max_steps=-1))
    refused(lambda: create(max_steps=2 ** 22 + 1))
    phi = np.ones(c.mesh.n_elem)
    phi[7] = 0.0
    refused(lambda: create(changed(c.mesh, porosity=phi)))
    fe = c.mesh.face_elem.copy()
    fe[c.mesh.elem_face[5, 0]] = fe[c.mesh.elem_face[20, 5]]
    refused(lambda: create(changed(c.mesh, face_elem=fe)))                       # elem_face / face_elem disagree
    sg = c.mesh.elem_sign.copy()
    assert c.mesh.face_elem[c.mesh.elem_face[1, 2], 1] >= 0                     # an interior face
    sg[1, 2] = -sg[1, 2]
    refused(lambda: create(changed(c.mesh, elem_sign=sg)))
    geom = c.mesh.geom.copy()
    geom[9, 3] += 0.01                                                            # no longer conforming boxes
    refused(lambda: create(changed(c.mesh, geom=geom)))
    geom = c.mesh.geom.copy()
    geom[9, 5] = geom[9, 2]                                                       # lo == hi
    refused(lambda: create(changed(c.mesh, geom=geom)))
    ef = c.mesh.elem_face[:, [5, 1, 2, 3, 4, 0]].copy()                           # local faces in another order
    refused(lambda: create(changed(c.mesh, elem_face=ef, elem_sign=c.mesh.elem_sign[:, [5, 1, 2, 3, 4, 0]].copy())))
    verts = tet.mesh.geom.copy()
    verts[4, [0, 1]] = verts[4, [1, 0]]                                           # negative volume
    refused(lambda: create(changed(tet.mesh, geom=verts), tet.x0, tet.elem0))
    far = c.x0.copy()
    far[3, 0] += 0.75                                                             # outside its elem0
    refused(lambda: create(x0=far))
    bad = c.elem0.copy()
    bad[0] = c.mesh.n_elem
    refused(lambda: create(elem0=bad))
    # NULL arrays and nparticles < 1 through the raw entry
    m = capi.pmc_tracer_mesh(c.mesh.kind, c.mesh.n_elem, c.mesh.n_face, capi._ptr(c.mesh.elem_face, C.c_int32), None,
                             capi._ptr(c.mesh.face_elem, C.c_int32), capi._ptr(c.mesh.geom, C.c_double), None)
    h = C.c_void_p()
    x0, e0 = np.ascontiguousarray(c.x0), np.ascontiguousarray(c.elem0, np.int32)
    assert lib.pmc_tracer_create(gpu_ctx.h, C.byref(m), len(e0), capi._ptr(x0, C.c_double), capi._ptr(e0, C.c_int32), 0,
                                 C.byref(h)) == -1 and not h.value
    m.elem_sign = c.mesh.elem_sign.ctypes.data_as(C.POINTER(C.c_int8))
    assert lib.pmc_tracer_create(gpu_ctx.h, C.byref(m), 0, capi._ptr(x0, C.c_double), capi._ptr(e0, C.c_int32), 0,
                                 C.byref(h)) == -1 and not h.value
    assert lib.pmc_tracer_create(gpu_ctx.h, C.byref(m), len(e0), None, capi._ptr(e0, C.c_int32), 0, C.byref(h)) == -1
    # run / reduce
    T = np.full((1, good.nparticles), -7.0)
    i3 = [np.full((1, good.nparticles), -7, np.int32) for _ in range(3)]
    u1 = np.ascontiguousarray(u[:1])
    args = lambda nb, pu, ld, pT: (good.h, nb, pu, ld, pT, i3[0].ctypes.data, i3[1].ctypes.data, i3[2].ctypes.data, None, 0)
    assert lib.pmc_tracer_run(*args(0, u1.ctypes.data, u1.shape[1], T.ctypes.data)) == -1
    assert lib.pmc_tracer_run(*args(1, None, u1.shape[1], T.ctypes.data)) == -1
    assert lib.pmc_tracer_run(*args(1, u1.ctypes.data, u1.shape[1], None)) == -1
    assert lib.pmc_tracer_run(*args(1, u1.ctypes.data, u1.shape[1] - 1, T.ctypes.data)) == -1
    assert (T == -7.0).all() and all((a == -7).all() for a in i3)                # a refused call writes nothing
    refused(lambda: good.Reduce(ref["T"], ref["status"], kind=2))
    refused(lambda: good.Reduce(ref["T"][:0], ref["status"][:0]))
    # set_tracer
    ds = solver(gpu_ctx, "hex")
    Q0, _ = ds.SolveFwd(1, c.k[:1])
    refused(lambda: ds.SetTracer(2, good))
    refused(lambda: ds.SetTracer(-1, good))
    refused(lambda: ds.SetTracer(0, good))                                        # the level-1 mesh on level 0
    refused(lambda: ds.SetTracer(1, good, kind=5))
    assert np.array_equal(ds.SolveFwd(1, c.k[:1])[0], Q0)                         # nothing was attached
    assert lib.pmc_tracer_num_particles(good.h) == good.nparticles and lib.pmc_tracer_num_particles(None) == -1
    good.close()


def test_tracer_of_another_device_is_refused(gpu_ctx):
    from parelagmc_amd import capi
    c = tc.case("hex1")
    try:
        other = capi.Context(1)
    except capi.PmcError:
        pytest.skip("one GPU")
    t = capi.Tracer(other, c.mesh, c.x0, c.elem0)
    with pytest.raises(capi.PmcError):
        solver(gpu_ctx, "hex").SetTracer(1, t)
    other.close()

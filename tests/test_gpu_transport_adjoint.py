"""The adjoint of the solute transport on the device (pmc_transport_run_adjoint, pmc_darcy_transport_gradient,
pmc_darcy_transport_loglik_gradient; csrc/transport.hip) against the numpy twin
(fe.transport.advance_adjoint) and the twin chain to a gradient in k: values on every element family and seed combination,
bitwise independence of width, split, memory space, strides and segment length, the columns that are not differentiated,
the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import transport_adjoint_cases as ta
import transport_cases as tc
from conftest import ROOT
from parelagmc_amd.fe import transport as tw

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
TIGHT_AGG = dict(TIGHT, max_iter=600)
FWD = ("curve", "stored", "nsteps", "status")
ADJ = ("u_bar", "c0_bar") + FWD

_transports = {}
_solvers = {}


def transport_for(gpu_ctx, name, nreport=ta.NREPORT):
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


def on_host(r, nb):
    """the dict of Transport.run_adjoint as numpy arrays in the shapes of a host-memory call"""
    if isinstance(r["stored"], np.ndarray):
        return r
    return {k: v.download().reshape(nb, -1) if k in ("u_bar", "c0_bar", "curve") else v.download() for k, v in r.items()}


def same(a, b, rows_a, rows_b, keys=ADJ, nf=None):
    cut = lambda k, x: x[:, :nf] if (k == "u_bar" and nf) else x
    return all(np.array_equal(cut(k, a[k])[rows_a], cut(k, b[k])[rows_b]) for k in keys)


@pytest.mark.parametrize("name", ta.NAMES)
def test_kernel_matches_twin(gpu_ctx, name):
    c, t = tc.case(name), transport_for(gpu_ctx, name)
    before = t.Run(c.u)
    worst = 0.0
    for combo in ta.COMBOS:
        ref = ta.twin(name, combo)
        got = t.run_adjoint(c.u, **ta.seeds(name, combo))
        assert same(got, before, slice(None), slice(None), FWD), combo                  # the forward outputs, bit for bit
        assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["nsteps"], ref["nsteps"])
        worst = max(worst, ta.adjoint_deviation(got, ref))
    print(f"{name}: largest deviation of u_bar / c0_bar from the twin {worst:.3g} (tolerance {ta.TOL_KA:.3g})")
    assert worst <= ta.TOL_KA
    after = t.Run(c.u)
    assert all(np.array_equal(before[k], after[k]) for k in before)                     # pmc_transport_run keeps its bits


@pytest.mark.parametrize("name", ["hex1", "quad1", "agg3_1"])
def test_bit_independence(gpu_ctx, name):
    c, t = tc.case(name), transport_for(gpu_ctx, name)
    nf, ne = c.mesh.n_face, c.mesh.n_elem
    sd = ta.seeds(name, ta.SEED_NAMES)
    full = t.run_adjoint(c.u, **sd)
    assert np.abs(full["u_bar"][1]).max() > 0
    assert same(full, t.run_adjoint(c.u, **sd), slice(None), slice(None))                # a repeated call
    one = t.run_adjoint(c.u[1:2], **{k: v[1:2] for k, v in sd.items()})                 # nbatch = 1
    assert same(full, one, [1], [0])
    idx = [i % 5 for i in range(67)]                                                     # more than one wave of columns
    wide = t.run_adjoint(c.u[idx], **{k: v[idx] for k, v in sd.items()})
    assert same(wide, full, slice(None), idx)
    dev = t.run_adjoint(gpu_ctx.array(c.u), **{k: gpu_ctx.array(v) for k, v in sd.items()}, nbatch=5)
    assert same(full, on_host(dev, 5), slice(None), slice(None))                         # device memory
    ld = nf + ne                                                                         # the strides of a full solution
    strided = np.zeros((5, ld))
    strided[:, :nf] = c.u
    wide_out = t.run_adjoint(strided, **sd, ld_bar=ld)
    assert same(full, wide_out, slice(None), slice(None), nf=nf) and (wide_out["u_bar"][:, nf:] == 0).all()
    dev = t.run_adjoint(gpu_ctx.array(strided), **{k: gpu_ctx.array(v) for k, v in sd.items()}, nbatch=5, ld=ld, ld_bar=ld)
    assert same(full, on_host(dev, 5), slice(None), slice(None), nf=nf)
    try:
        for K in (1, 2, int(full["nsteps"].max()), 3 * int(full["nsteps"].max())):
            t.set_adjoint_segment(K)
            assert same(full, t.run_adjoint(c.u, **sd), slice(None), slice(None)), K
            assert same(full, t.run_adjoint(c.u[1:2], **{k: v[1:2] for k, v in sd.items()}), [1], [0]), K
    finally:
        t.set_adjoint_segment(0)
    assert same(full, t.run_adjoint(c.u, **sd), slice(None), slice(None))


def test_columns_that_are_not_differentiated(gpu_ctx):
    from parelagmc_amd import capi
    c = tc.case("hex1")
    sd = {k: v[:, :4] if k == "curve_bar" else v for k, v in ta.seeds("hex1", ta.SEED_NAMES).items()}
    t = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4)
    clean = t.run_adjoint(c.u, **sd)
    u = c.u.copy()
    u[1, 7] = np.nan
    r, fwd = t.run_adjoint(u, **sd), t.Run(u)
    assert r["status"][1] == t.BAD_FLUX and r["nsteps"][1] == 0
    assert (r["u_bar"][1] == 0).all() and (r["c0_bar"][1] == 0).all()
    assert same(r, fwd, slice(None), slice(None), FWD)
    assert same(r, clean, [0, 2, 3, 4], [0, 2, 3, 4])                   # the other columns keep their bits
    ref = tw.advance_adjoint(c.mesh, u, c.t_end, tc.CFL, 4, **sd)
    assert np.array_equal(ref["status"], r["status"]) and ta.adjoint_deviation(r, ref) <= ta.TOL_KA
    t.close()
    # columns 0 .. 3 would need 13 to 29 steps: with max_steps 20 two of them stop at the limit
    short = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4, max_steps=20)
    r, fwd = short.run_adjoint(c.u, **sd), short.Run(c.u)
    lim = r["status"] == short.STEP_LIMIT
    assert lim.sum() == 2 and (r["status"][~lim] == short.OK).all()
    assert (r["u_bar"][lim] == 0).all() and (r["c0_bar"][lim] == 0).all() and (r["nsteps"][lim] == 20).all()
    assert same(r, fwd, slice(None), slice(None), FWD)
    ok = np.flatnonzero(~lim)
    assert same(r, clean, ok, ok)
    ref = tw.advance_adjoint(c.mesh, c.u, c.t_end, tc.CFL, 4, **sd, max_steps=20)
    assert np.array_equal(ref["status"], r["status"]) and ta.adjoint_deviation(r, ref) <= ta.TOL_KA
    # the same through the Darcy entries, the columns at the limit beside the others in one launch of four: a zero gradient and
    # the status for the former, the bits of a handle without the limit for the latter
    ds, free = solver(gpu_ctx, "hex"), capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4)
    sd2 = {k: v[:4] for k, v in sd.items() if k != "c_bar"}
    data = np.linspace(0.1, 1.0, 4) * c.mesh.pore_volume.sum()
    g, g_free = ds.TransportGradient(c.level, short, c.k, **sd2, want_solution=True), ds.TransportGradient(c.level, free, c.k, **sd2)
    lim4 = g["status"] == short.STEP_LIMIT
    assert lim4.sum() == 2 and np.array_equal(lim4, lim[:4]) and (g_free["status"] == free.OK).all()
    assert (g["grad"][lim4] == 0).all() and (g["adj"][lim4] == 0).all() and (np.abs(g_free["grad"]).max(axis=1) > 0).all()
    assert np.array_equal(g["grad"][~lim4], g_free["grad"][~lim4])
    run = short.Run(g["sol"])
    assert all(np.array_equal(g[key], run[key]) for key in ("curve", "stored", "status"))
    ll, curve, status, grad = ds.TransportLoglikGradient(c.level, short, c.k, data, 0.5)
    ll_free, _, _, grad_free = ds.TransportLoglikGradient(c.level, free, c.k, data, 0.5)
    assert np.array_equal(status, g["status"]) and np.array_equal(curve, g["curve"])
    assert (grad[lim4] == 0).all() and np.array_equal(grad[~lim4], grad_free[~lim4]) and np.array_equal(ll[~lim4], ll_free[~lim4])
    want = -((curve - data) ** 2).sum(axis=1) / (2 * 0.5)
    assert np.abs(ll - want).max() <= 1e-12 * np.abs(want).max()
    free.close()
    short.close()


def test_refusals(gpu_ctx):
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    c = tc.case("quad0")
    nf, ne = c.mesh.n_face, c.mesh.n_elem
    t = capi.Transport(gpu_ctx, c.mesh, c.t_end, tc.CFL, 4)
    sd = {k: v[:, :4] if k == "curve_bar" else v for k, v in ta.seeds("quad0", ta.SEED_NAMES).items()}
    ref = t.run_adjoint(c.u, **sd)
    u = np.ascontiguousarray(c.u[:1])
    cb, sb, eb = (np.ascontiguousarray(sd[k][:1]) for k in ta.SEED_NAMES)
    f = {k: np.full(n, -7.0) for k, n in (("u_bar", nf), ("c0_bar", ne), ("curve", 4), ("stored", 1))}
    i2 = [np.full(1, -7, np.int32) for _ in range(2)]
    p = lambda a: None if a is None else a.ctypes.data

    def run(h=t.h, nb=1, pu=p(u), ld=u.shape[1], seeds=(cb, sb, eb), ubar=f["u_bar"], ld_bar=nf, status=i2[1], ms=0):
        return lib.pmc_transport_run_adjoint(h, nb, pu, ld, *[p(a) for a in seeds], p(ubar), ld_bar, p(f["c0_bar"]), p(f["curve"]),
                                             p(f["stored"]), p(i2[0]), p(status), ms)

    for what, kw in (("no seed", dict(seeds=(None, None, None))), ("u", dict(pu=None)), ("u_bar", dict(ubar=None)),
                     ("status", dict(status=None)), ("ld", dict(ld=nf - 1)), ("ld_bar", dict(ld_bar=nf - 1)), ("nbatch", dict(nb=0)),
                     ("memspace", dict(ms=7)), ("handle", dict(h=None))):
        assert run(**kw) == -1, what
        assert all((a == -7).all() for a in list(f.values()) + i2), what              # nothing was written
        assert len(lib.pmc_last_error()) > 0
    assert lib.pmc_transport_set_adjoint_segment(t.h, -1) == -1 and lib.pmc_transport_set_adjoint_segment(None, 1) == -1
    assert run() == 0 and np.array_equal(f["u_bar"], ref["u_bar"][0]) and np.array_equal(f["c0_bar"], ref["c0_bar"][0])
    assert same(t.run_adjoint(c.u, **sd), ref, slice(None), slice(None))              # the handle stays usable
    # the Darcy entries
    ds = solver(gpu_ctx, "quad")
    k = np.ascontiguousarray(c.k[:1])
    good = ds.TransportGradient(0, t, k, curve_bar=cb, stored_bar=sb)
    g, st, ll = np.full(ne, -7.0), np.full(1, -7, np.int32), np.full(1, -7.0)
    data = np.full(4, 0.1)

    def grad(d=ds.h, level=0, h=t.h, nb=1, pk=p(k), seeds=(cb, sb), status=st, pg=p(g), ms=0):
        return lib.pmc_darcy_transport_gradient(d, level, h, nb, pk, p(seeds[0]), p(seeds[1]), 0, None, None,
                                                capi._ptr(status, C.c_int32) if status is not None else None, pg, None, None, ms, None,
                                                None)

    def loglik(d=ds.h, level=0, h=t.h, nb=1, pk=p(k), pd=capi._ptr(data, C.c_double), noise=0.01, pg=p(g), ms=0):
        return lib.pmc_darcy_transport_loglik_gradient(d, level, h, nb, pk, pd, noise, 0, capi._ptr(ll, C.c_double), None,
                                                       capi._ptr(st, C.c_int32), pg, ms, None)

    other = transport_for(gpu_ctx, "hex1")                                             # of other sizes than the level
    for what, kw in (("darcy", dict(d=None)), ("level", dict(level=7)), ("level", dict(level=-1)), ("transport", dict(h=None)),
                     ("sizes", dict(h=other.h)), ("sizes", dict(level=1)), ("nbatch", dict(nb=0)), ("k", dict(pk=None)),
                     ("grad", dict(pg=None)), ("memspace", dict(ms=7))):
        assert grad(**kw) == -1, what
        assert loglik(**kw) == -1, what
    assert grad(seeds=(None, None)) == -1 and grad(status=None) == -1
    assert loglik(noise=0.0) == -1 and loglik(noise=-1.0) == -1 and loglik(pd=None) == -1
    assert (g == -7).all() and (st == -7).all() and (ll == -7).all()
    again = ds.TransportGradient(0, t, k, curve_bar=cb, stored_bar=sb)
    assert all(np.array_equal(good[key], again[key]) for key in good)
    assert grad() == 0 and np.array_equal(g, good["grad"][0]) and st[0] == 0
    t.close()


def device_gradients(gpu_ctx, name, hybrid):
    """the Darcy entry on the case's four fields: gradients in k and in log k, and pmc_transport_run on its solution"""
    c = tc.case(name)
    ds, t = solver(gpu_ctx, c.kind, hybrid), transport_for(gpu_ctx, name)
    sd = ta.seeds(name, ("curve_bar", "stored_bar"), slice(0, 4))
    out = {wrt_log: ds.TransportGradient(c.level, t, c.k, **sd, wrt_log=wrt_log, want_solution=True) for wrt_log in (False, True)}
    out["run"] = t.Run(out[False]["sol"])
    return out


@pytest.mark.parametrize("name,hybrid", ta.GRAD_CASES)
def test_darcy_transport_gradient(gpu_ctx, name, hybrid):
    c, t, ref = tc.case(name), transport_for(gpu_ctx, name), tc.twin(name)
    got = device_gradients(gpu_ctx, name, hybrid)
    keep = tc.kept(ref["margin"], tc.MARGIN_E)[:4]
    run = got["run"]
    for wrt_log in (False, True):
        r = got[wrt_log]
        assert (r["status"] == t.OK).all()
        assert np.array_equal(r["curve"], run["curve"]) and np.array_equal(r["stored"], run["stored"])       # the hook's bits
        assert np.array_equal(r["sol"], got[False]["sol"])
        fwd = dict(c=run["c"], curve=r["curve"], stored=r["stored"])
        sub = {k: np.asarray(v)[:4] for k, v in ref.items()}
        assert np.array_equal(run["nsteps"][keep], sub["nsteps"][keep])
        d = tc.deviation(c.mesh, c.u[:4], fwd, sub, keep)
        assert d <= tc.TOL_E, d
        worst = 0.0
        for b in np.flatnonzero(keep):
            g = ta.chain_gradient(name, b, ("curve_bar", "stored_bar"), wrt_log)[0]
            worst = max(worst, float(np.abs(r["grad"][b] - g).max() / np.abs(g).max()))
        print(f"{name} hybrid={hybrid} wrt_log={wrt_log}: gradient differs from the twin chain by {worst:.3g} of its largest entry, "
              f"curve / stored by {d:.3g} (tolerances {ta.TOL_G:.3g}, {tc.TOL_E:.3g})")
        assert worst <= ta.TOL_G


def test_split_and_width_independence(gpu_ctx):
    """nbatch 1, 3 and 5: a call is cut into launches of 4 + 1, 2 + 1 and 1 columns.  The transport's adjoint has the same
    bits at every width (test_bit_independence), the Darcy solves in front of and behind it have not - their paths depend
    on the launch width, for pmc_darcy_solve_gradient as well: on this case x of one column differs by 5.6e-16 and lam by
    1.3e-15 between a launch of 1 and a launch of 4.  So:
    - the column that every one of the three calls puts into a launch of one comes out bit for bit, as does every column
      when the same launches are issued by two calls instead of one;
    - at every width the entry is bit for bit the composition of the public pieces at that width - pmc_transport_run_adjoint
      on sol_out, then pmc_darcy_solve_gradient with adj_rhs = [u_bar; 0] - so whatever changes with the width is what
      pmc_darcy_solve_gradient changes: a width dependence of the transport's side would break this;
    - the columns that change their launch width stay within 16 x WIDTH_RAW (transport_adjoint_cases.py)."""
    from parelagmc_amd import capi
    import tracer_cases as trc
    name = "hex1"
    c, ds, t = tc.case(name), solver(gpu_ctx, "hex"), transport_for(gpu_ctx, name)
    idx = [0, 1, 2, 3, 1]
    k = np.ascontiguousarray(c.k[idx])
    sd = ta.seeds(name, ("curve_bar", "stored_bar"), idx)
    full = ds.TransportGradient(c.level, t, k, **sd, want_solution=True)                  # nbatch 5: launches of 4 + 1
    keys = ("grad", "curve", "stored", "status", "sol", "adj")
    part = lambda rows: ds.TransportGradient(c.level, t, k[rows], **{a: v[rows] for a, v in sd.items()}, want_solution=True)
    one, three = part([4]), part([2, 3, 4])                                               # nbatch 1; nbatch 3: launches of 2 + 1
    for key in keys:
        assert np.array_equal(one[key][0], full[key][4]) and np.array_equal(three[key][2], full[key][4]), key
    head = part([0, 1, 2, 3])                                                             # the launches of nbatch 5 in two calls
    assert all(np.array_equal(head[key], full[key][:4]) for key in keys)
    assert all(np.array_equal(part(idx)[key], full[key]) for key in keys)                 # a repeated call
    n = full["sol"].shape[1]
    for rows, r in (([4], one), ([2, 3, 4], three), ([0, 1, 2, 3], head), (idx, full)):
        ub = t.run_adjoint(r["sol"], **{a: v[rows] for a, v in sd.items()}, ld_bar=n, want_c0_bar=False)["u_bar"]
        _, _, g, x, lam = ds.solve_gradient(c.level, k[rows], ub, want_solution=True)
        assert np.array_equal(g, r["grad"]) and np.array_equal(x, r["sol"]) and np.array_equal(lam, r["adj"]), rows
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    moved = max(rel(three["grad"][0], full["grad"][2]), rel(three["grad"][1], full["grad"][3]), rel(part([1])["grad"][0], full["grad"][1]),
                rel(full["grad"][4], full["grad"][1]))                                    # widths 2 / 4, 1 / 4, and the same k at 1 / 4
    print(f"grad of a column at launch widths 1, 2 and 4: differs by {moved:.3g} of its largest entry "
          f"(tolerance {16 * ta.WIDTH_RAW:.3g})")
    assert moved <= 16 * ta.WIDTH_RAW
    Q, _, grad_q, sol, _ = ds.solve_gradient(c.level, k, want_solution=True)
    assert np.array_equal(sol, full["sol"])
    dev = ds.TransportGradient(c.level, t, gpu_ctx.array(k), **{a: gpu_ctx.array(v) for a, v in sd.items()}, nbatch=5,
                               grad_out=gpu_ctx.array(np.zeros_like(k)))
    assert np.array_equal(dev["grad"].download().reshape(k.shape), full["grad"])          # device memory
    assert np.array_equal(dev["curve"].download().reshape(5, -1), full["curve"])
    # a transport, then a tracer attached to the level: the new entries return the same bits, the old gradient keeps <obs, x>
    hx = trc.case(name)
    tracer = capi.Tracer(gpu_ctx, hx.mesh, hx.x0, hx.elem0)
    data = np.linspace(0.1, 1.0, ta.NREPORT) * c.mesh.pore_volume.sum()
    ll0 = ds.TransportLoglikGradient(c.level, t, k, data, 0.5)
    for attach, detach in ((lambda: ds.SetTransport(c.level, t, t.STORED), lambda: ds.SetTransport(c.level, None)),
                           (lambda: ds.SetTracer(c.level, tracer), lambda: ds.SetTracer(c.level, None))):
        attach()
        try:
            hooked = ds.TransportGradient(c.level, t, k, **sd, want_solution=True)
            assert all(np.array_equal(hooked[key], full[key]) for key in keys)
            assert all(np.array_equal(a, b) for a, b in zip(ds.TransportLoglikGradient(c.level, t, k, data, 0.5), ll0))
            Qh, _, gh = ds.solve_gradient(c.level, k)
            assert np.array_equal(Qh, Q) and np.array_equal(gh, grad_q)
        finally:
            detach()
    tracer.close()


@pytest.mark.parametrize("name,hybrid", [("hex1", False), ("quad0", False), ("hex1", True)])
def test_loglik_gradient(gpu_ctx, name, hybrid):
    c, ds, t = tc.case(name), solver(gpu_ctx, tc.case(name).kind, hybrid), transport_for(gpu_ctx, name)
    rng = np.random.default_rng(5)
    noise = 0.3
    data = tc.twin(name)["curve"][0] * (1 + 0.1 * rng.standard_normal(ta.NREPORT))
    for wrt_log in (False, True):
        ll, curve, status, grad = ds.TransportLoglikGradient(c.level, t, c.k, data, noise, wrt_log=wrt_log)
        assert (status == t.OK).all()
        want = -((curve - data) ** 2).sum(axis=1) / (2 * noise)
        assert np.abs(ll - want).max() <= 1e-12 * np.abs(want).max()
        gen = ds.TransportGradient(c.level, t, c.k, curve_bar=-(curve - data) / noise, wrt_log=wrt_log)
        assert np.array_equal(gen["curve"], curve)
        d = float((np.abs(grad - gen["grad"]).max(axis=1) / np.abs(gen["grad"]).max(axis=1)).max())
        print(f"{name} hybrid={hybrid} wrt_log={wrt_log}: log-likelihood gradient differs from the general entry by {d:.3g}")
        assert d <= ta.TOL_KA


def test_mirror_classes_compile_and_run(gpu_ctx, tmp_path):
    """SoluteTransport::RunAdjoint, DarcySolver::SolveFwd_TransportGradient and ::ComputeGradTransportLogLikelihood of
    parelagmc.hpp from a C++ caller: the adjoint identity of a tiny two-element channel against a finite difference"""
    src = os.path.join(ROOT, "tests", "c", "transport_adjoint_smoke.cpp")
    exe = str(tmp_path / "transport_adjoint_smoke")
    lib = os.path.join(ROOT, "parelagmc_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-L" + lib,
                    "-lpmc_host", "-lpmc", "-pthread", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "transport adjoint smoke ok" in out.stdout

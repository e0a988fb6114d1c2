"""The adjoint of the particle tracer on the device (pmc_tracer_run_adjoint, pmc_tracer_reduce_seed, pmc_darcy_tracer_gradient,
pmc_darcy_tracer_loglik_gradient; csrc/tracer.hip) against the numpy twin (fe.tracer.trace_adjoint):
values, bitwise reproducibility, censored particles, the refusals, the Darcy entries and the C++ mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tracer_adjoint_cases as ta
import tracer_cases as tc
from conftest import ROOT
from parelagmc_amd.fe import tracer as tr

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
KEYS = ("u_bar", "x0_bar") + ta.FWD_KEYS

_solvers = {}
_tracers = {}


def solver(gpu_ctx, kind, hybrid=False):
    from parelagmc_amd import capi
    if (kind, hybrid) not in _solvers:
        _solvers[kind, hybrid] = capi.DarcySolver(gpu_ctx, tc.problem(kind), capi.solver_opts(**TIGHT), hybrid=hybrid)
    return _solvers[kind, hybrid]


def tracer_for(gpu_ctx, name):
    from parelagmc_amd import capi
    if name not in _tracers:
        c = ta.case(name)
        _tracers[name] = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0)
    return _tracers[name]


def same(a, b, rows_a=slice(None), rows_b=slice(None), keys=KEYS):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in keys)


@pytest.mark.parametrize("name", ta.NAMES)
def test_kernel_matches_twin(gpu_ctx, name):
    """Measured on the MI355X: on the three tetrahedral cases the kernels return the twin's bits; on the box cases they do
    not (hex0 2.6e-14, hex1 4.2e-15, stretch 5.4e-16, crowded 1.4e-15 of the column's largest entry; tolerance 1.76e-12)."""
    c, t, u = ta.case(name), tracer_for(gpu_ctx, name), ta.flux(name)
    run = t.Run(u)
    for combo in ta.COMBOS:
        ref, got = ta.twin(name, combo), t.run_adjoint(u, **ta.seeds(name, combo))
        for key in ("status", "exit_face", "nsteps"):
            assert np.array_equal(got[key], ref[key]), (combo, key)
            assert np.array_equal(got[key], run[key]), (combo, key)
        assert np.array_equal(got["T"], run["T"])                       # the forward outputs are pmc_tracer_run's
        d = ta.adjoint_deviation(got, ref)
        bits = np.array_equal(got["u_bar"], ref["u_bar"]) and np.array_equal(got["x0_bar"], ref["x0_bar"])
        print(f"{name} {'+'.join(combo)}: kernel differs from the twin by {d:.3g} (tolerance {ta.TOL_KT:.3g}); same bits: {bits}")
        assert d <= ta.TOL_KT, (combo, d)
    if name == ta.CROWDED:                                              # one list holds hundreds of visits
        assert (run["nsteps"] >= 1).all() and len(c.x0) == 300


@pytest.mark.parametrize("name", ["hex0", "tet2", ta.CROWDED])
def test_bit_independence(gpu_ctx, name):
    c, t, u4 = ta.case(name), tracer_for(gpu_ctx, name), ta.flux(name)
    n_u, npart = c.mesh.n_face, len(c.x0)
    u = np.stack([u4[i % 4] * (1.0 + 0.01 * (i // 4)) for i in range(67)])
    rng = np.random.Generator(np.random.PCG64(3))
    sd = dict(T_bar=rng.standard_normal((67, npart)), x_exit_bar=rng.standard_normal((67, npart, 3)))
    sub = lambda rows: {k: np.ascontiguousarray(v[rows]) for k, v in sd.items()}
    before = t.Run(u)
    full = t.run_adjoint(u, **sd)
    assert t.adjoint_chunks() == 1
    assert same(full, t.run_adjoint(u, **sd))                                              # a repeated call
    for j in (0, 2, 66):
        assert same(full, t.run_adjoint(u[j:j + 1], **sub([j])), [j], [0])                 # nbatch 1
    rows = [5, 66, 1, 30, 2]
    assert same(full, t.run_adjoint(u[rows], **sub(rows)), rows, slice(None))              # nbatch 5, other neighbours
    dev = t.run_adjoint(gpu_ctx.array(u), **{k: gpu_ctx.array(v) for k, v in sd.items()}, nbatch=67)     # device memory
    assert same(full, {k: dev[k].download().reshape(full[k].shape) for k in KEYS})
    n = n_u + c.mesh.n_elem                                                                 # a full solution row
    wide = np.zeros((67, n))
    wide[:, :n_u] = u
    w = t.run_adjoint(wide, **sd, ld_bar=n)
    assert np.array_equal(w["u_bar"][:, :n_u], full["u_bar"]) and (w["u_bar"][:, n_u:] == 0).all()
    assert same(full, w, keys=KEYS[1:])
    # a forced small cap on the records: 67 columns in chunks of a few columns, then of one
    per_col = (16 + 8 * (9 if c.mesh.kind == tr.BOX else 8)) * int(full["nsteps"].max()) * npart + 4 * c.mesh.n_elem
    for cols in (5, 1):
        t.set_adjoint_scratch(cols * per_col)
        assert same(full, t.run_adjoint(u, **sd))
        assert t.adjoint_chunks() == -(-67 // cols)
    t.set_adjoint_scratch(1)                                                                # below one column: one column
    assert same(full, t.run_adjoint(u[:3], **sub(slice(0, 3))), slice(0, 3), slice(None)) and t.adjoint_chunks() == 3
    t.set_adjoint_scratch(0)
    after = t.Run(u)
    assert all(np.array_equal(before[k], after[k]) for k in before)                        # pmc_tracer_run is undisturbed
    assert all(np.array_equal(before[k], full[k]) for k in ta.FWD_KEYS)


def test_censored_particles(gpu_ctx):
    """a max_steps that censors some particles: they contribute nothing, their x0_bar is zero, and the others' results are
    those of a call whose censored seeds are zero"""
    from parelagmc_amd import capi
    for name in ("hex1", "tet1"):
        c, u = ta.case(name), ta.flux(name)
        free = ta.twin(name)
        cut = int(np.median(free["nsteps"]))
        t = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0, max_steps=cut)
        sd = ta.seeds(name, ta.BOTH)
        got = t.run_adjoint(u, **sd)
        ref = tr.trace_adjoint(c.mesh, u, c.x0, c.elem0, **sd, max_steps=cut)
        cens = got["status"] != t.EXITED
        assert cens.any() and (~cens).any() and np.array_equal(got["status"], ref["status"])
        assert (got["status"][cens] == t.MAX_STEPS).all() and (got["nsteps"][cens] == cut).all()
        assert (got["x0_bar"][cens] == 0).all()
        assert ta.adjoint_deviation(got, ref) <= ta.TOL_KT
        zeroed = t.run_adjoint(u, T_bar=sd["T_bar"] * ~cens, x_exit_bar=sd["x_exit_bar"] * ~cens[:, :, None])
        assert same(got, zeroed)
        t.close()
    # nothing exits: u_bar and x0_bar are zero
    t = tracer_for(gpu_ctx, "hex1")
    still = t.run_adjoint(np.zeros_like(ta.flux("hex1")[:2]), **ta.seeds("hex1", ta.BOTH, slice(0, 2)))
    assert (still["status"] == t.STAGNANT).all() and (still["u_bar"] == 0).all() and (still["x0_bar"] == 0).all()


def test_reduce_seed(gpu_ctx):
    t, u = tracer_for(gpu_ctx, "hex1"), ta.flux("hex1")
    run = t.Run(u)
    T, status = run["T"].copy(), run["status"].copy()
    status[1, 3] = t.MAX_STEPS
    T[2, 7] = T[2, 11] = T[2].min() / 2                                  # a tie: the lower index takes the seed
    status[3, int(T[3].argmin())] = t.STAGNANT                           # the minimum did not exit
    for kind in (t.MEAN, t.MIN):
        got, ref = t.reduce_seed(T, status, kind), tr.reduce_seed(T, status, kind)
        assert np.array_equal(got, ref), kind
        dev = t.Run(gpu_ctx.array(u), nbatch=4, want_x=False)
        assert np.array_equal(t.reduce_seed(dev["T"], dev["status"], kind).download().reshape(4, -1),
                              tr.reduce_seed(run["T"], run["status"], kind))
    mn = t.reduce_seed(T, status, t.MIN)
    assert mn[2, 7] == 1 and mn[2, 11] == 0 and mn[2].sum() == 1 and mn[3].sum() == 0 and mn[0].sum() == 1


def test_refusals(gpu_ctx):
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    c, t = ta.case("hex1"), tracer_for(gpu_ctx, "hex1")
    nf, npart = c.mesh.n_face, len(c.x0)
    sd = ta.seeds("hex1", ta.BOTH)
    ref = t.run_adjoint(ta.flux("hex1"), **sd)
    u = np.ascontiguousarray(ta.flux("hex1")[:1])
    tb, xb = (np.ascontiguousarray(sd[k][:1]) for k in ta.BOTH)
    f = {k: np.full(n, -7.0) for k, n in (("u_bar", nf), ("x0_bar", 3 * npart), ("T", npart))}
    i3 = [np.full(npart, -7, np.int32) for _ in range(3)]
    p = lambda a: None if a is None else a.ctypes.data

    def run(h=t.h, nb=1, pu=p(u), ld=u.shape[1], seeds=(tb, xb), ubar=f["u_bar"], ld_bar=nf, status=i3[1], ms=0):
        return lib.pmc_tracer_run_adjoint(h, nb, pu, ld, p(seeds[0]), p(seeds[1]), p(ubar), ld_bar, p(f["x0_bar"]), p(f["T"]),
                                          p(i3[0]), p(status), p(i3[2]), ms)

    for what, kw in (("no seed", dict(seeds=(None, None))), ("u", dict(pu=None)), ("u_bar", dict(ubar=None)),
                     ("status", dict(status=None)), ("ld", dict(ld=nf - 1)), ("ld_bar", dict(ld_bar=nf - 1)), ("nbatch", dict(nb=0)),
                     ("memspace", dict(ms=7)), ("handle", dict(h=None))):
        assert run(**kw) == -1, what
        assert all((a == -7).all() for a in list(f.values()) + i3), what              # nothing was written
        assert len(lib.pmc_last_error()) > 0
    assert lib.pmc_tracer_set_adjoint_scratch(t.h, -1) == -1 and lib.pmc_tracer_set_adjoint_scratch(None, 1) == -1
    assert lib.pmc_tracer_adjoint_chunks(None) == -1
    seed = np.full(npart, -7.0)
    T1, s1 = np.ascontiguousarray(ref["T"][:1]), np.ascontiguousarray(ref["status"][:1])
    for args in ((None, 1, p(T1), p(s1), 0, p(seed), 0), (t.h, 0, p(T1), p(s1), 0, p(seed), 0), (t.h, 1, None, p(s1), 0, p(seed), 0),
                 (t.h, 1, p(T1), None, 0, p(seed), 0), (t.h, 1, p(T1), p(s1), 2, p(seed), 0), (t.h, 1, p(T1), p(s1), 0, None, 0),
                 (t.h, 1, p(T1), p(s1), 0, p(seed), 7)):
        assert lib.pmc_tracer_reduce_seed(*args) == -1, args
    assert (seed == -7).all()
    assert run() == 0 and np.array_equal(f["u_bar"], ref["u_bar"][0]) and np.array_equal(f["x0_bar"].reshape(-1, 3), ref["x0_bar"][0])
    assert same(t.run_adjoint(ta.flux("hex1"), **sd), ref)                            # the handle stays usable
    # the Darcy entries
    ds = solver(gpu_ctx, "hex")
    k = np.ascontiguousarray(c.k[:1])
    good = ds.tracer_gradient(c.level, t, k, tb)
    ne = c.mesh.n_elem
    g, st, ll, nex = np.full(ne, -7.0), np.full(npart, -7, np.int32), np.full(1, -7.0), np.full(1, -7, np.int32)
    data = np.full(npart, 0.5)

    def grad(d=ds.h, level=c.level, h=t.h, nb=1, pk=p(k), ptb=p(tb), status=st, pg=p(g), ms=0):
        return lib.pmc_darcy_tracer_gradient(d, level, h, nb, pk, ptb, 0, None, p(status), pg, None, None, ms, None, None)

    def loglik(d=ds.h, level=c.level, h=t.h, nb=1, pk=p(k), pd=capi._ptr(data, C.c_double), noise=0.01, pg=p(g), ms=0, pn=nex):
        return lib.pmc_darcy_tracer_loglik_gradient(d, level, h, nb, pk, pd, noise, 0, capi._ptr(ll, C.c_double), None,
                                                    None if pn is None else capi._ptr(pn, C.c_int32), pg, ms, None)

    other = tracer_for(gpu_ctx, "hex0")                                                # of other sizes than the level
    for what, kw in (("darcy", dict(d=None)), ("level", dict(level=7)), ("level", dict(level=-1)), ("tracer", dict(h=None)),
                     ("sizes", dict(h=other.h)), ("sizes", dict(level=0)), ("nbatch", dict(nb=0)), ("k", dict(pk=None)),
                     ("grad", dict(pg=None)), ("memspace", dict(ms=7))):
        assert grad(**kw) == -1, what
        assert loglik(**kw) == -1, what
    assert grad(ptb=None) == -1 and grad(status=None) == -1
    assert loglik(noise=0.0) == -1 and loglik(noise=-1.0) == -1 and loglik(pd=None) == -1 and loglik(pn=None) == -1
    assert (g == -7).all() and (st == -7).all() and (ll == -7).all() and (nex == -7).all()
    again = ds.tracer_gradient(c.level, t, k, tb)
    assert all(np.array_equal(good[key], again[key]) for key in good)
    assert grad() == 0 and np.array_equal(g, good["grad"][0]) and (st == 0).all()


def test_tracer_of_another_device_is_refused(gpu_ctx):
    from parelagmc_amd import capi
    c = ta.case("hex1")
    try:
        other = capi.Context(1)
    except capi.PmcError:
        pytest.skip("one GPU")
    t = capi.Tracer(other, c.mesh, c.x0, c.elem0)
    with pytest.raises(capi.PmcError):
        solver(gpu_ctx, "hex").tracer_gradient(c.level, t, c.k[:1], ta.seeds("hex1", ("T_bar",), [0])["T_bar"])
    other.close()


@pytest.mark.parametrize("name,hybrid", [("hex1", False), ("tet1", False), ("hex1", True), ("tet1", True)])
def test_darcy_tracer_gradient(gpu_ctx, name, hybrid):
    c, t, ds = ta.case(name), tracer_for(gpu_ctx, name), solver(gpu_ctx, ta.case(name).kind, hybrid)
    Tb = ta.seeds(name, ("T_bar",))["T_bar"]
    for wrt_log in (False, True):
        r = ds.tracer_gradient(c.level, t, c.k, Tb, wrt_log=wrt_log, want_solution=True)
        run = t.Run(r["sol"])
        assert np.array_equal(r["T"], run["T"]) and np.array_equal(r["status"], run["status"])       # the hook's bits
        assert (r["status"] == t.EXITED).all()
        _, _, _, sol, _ = ds.solve_gradient(c.level, c.k, want_solution=True)
        assert np.array_equal(sol, r["sol"])
        worst = 0.0
        for b in range(4):
            g, ref = ta.chain_gradient(name, b, Tb[b], wrt_log)
            assert ta.same_path({k: v[0] for k, v in ref.items() if k in ta.FWD_KEYS},
                                {k: run[k][b] for k in ta.FWD_KEYS}).mean() >= 1 - ta.MARGIN_CAP
            worst = max(worst, float(np.abs(r["grad"][b] - g).max() / np.abs(g).max()))
        print(f"{name} hybrid={hybrid} wrt_log={wrt_log}: gradient differs from the twin chain by {worst:.3g} of its largest "
              f"entry (tolerance {ta.TOL_G:.3g})")
        assert worst <= ta.TOL_G


def test_split_and_width_independence(gpu_ctx):
    """nbatch 1, 3, 4 and 5: a call is cut into launches of 1, 2 + 1, 4 and 4 + 1 columns.  At every width the entry is bit for
    bit the composition of the public pieces at that width - pmc_tracer_run_adjoint on sol_out, then pmc_darcy_solve_gradient
    with adj_rhs = [u_bar; 0] - so whatever changes with the width is what pmc_darcy_solve_gradient changes."""
    from parelagmc_amd import capi
    import transport_cases as trc
    name = "hex1"
    c, ds, t = ta.case(name), solver(gpu_ctx, "hex"), tracer_for(gpu_ctx, name)
    idx = [0, 1, 2, 3, 1]
    k = np.ascontiguousarray(c.k[idx])
    Tb = ta.seeds(name, ("T_bar",), idx)["T_bar"]
    full = ds.tracer_gradient(c.level, t, k, Tb, want_solution=True)                       # nbatch 5: launches of 4 + 1
    keys = ("grad", "T", "status", "sol", "adj")
    part = lambda rows: ds.tracer_gradient(c.level, t, k[rows], Tb[rows], want_solution=True)
    one, three = part([4]), part([2, 3, 4])                                               # nbatch 1; nbatch 3: launches of 2 + 1
    for key in keys:
        assert np.array_equal(one[key][0], full[key][4]) and np.array_equal(three[key][2], full[key][4]), key
    head = part([0, 1, 2, 3])                                                             # the launches of nbatch 5 in two calls
    assert all(np.array_equal(head[key], full[key][:4]) for key in keys)
    assert all(np.array_equal(part(idx)[key], full[key]) for key in keys)                 # a repeated call
    n = full["sol"].shape[1]
    for rows, r in (([4], one), ([2, 3, 4], three), ([0, 1, 2, 3], head), (idx, full)):
        ub = t.run_adjoint(r["sol"], T_bar=Tb[rows], ld_bar=n, want_x0_bar=False)["u_bar"]
        _, _, g, x, lam = ds.solve_gradient(c.level, k[rows], ub, want_solution=True)
        assert np.array_equal(g, r["grad"]) and np.array_equal(x, r["sol"]) and np.array_equal(lam, r["adj"]), rows
    Q, _, grad_q, sol, _ = ds.solve_gradient(c.level, k, want_solution=True)
    assert np.array_equal(sol, full["sol"])
    dev = ds.tracer_gradient(c.level, t, gpu_ctx.array(k), gpu_ctx.array(Tb), nbatch=5, grad_out=gpu_ctx.array(np.zeros_like(k)))
    assert np.array_equal(dev["grad"].download().reshape(k.shape), full["grad"])          # device memory
    assert np.array_equal(dev["T"].download().reshape(5, -1), full["T"])
    assert np.array_equal(dev["status"].download().reshape(5, -1), full["status"])
    # a tracer, then a transport attached to the level: the new entries return the same bits, the old gradient keeps <obs, x>
    tm = trc.case(name)
    transport = capi.Transport(gpu_ctx, tm.mesh, tm.t_end, trc.CFL, 4)
    data = full["T"][0] * 1.1
    ll0 = ds.tracer_loglik_gradient(c.level, t, k, data, 0.5)
    for attach, detach in ((lambda: ds.SetTracer(c.level, t, t.MIN), lambda: ds.SetTracer(c.level, None)),
                           (lambda: ds.SetTransport(c.level, transport, transport.STORED), lambda: ds.SetTransport(c.level, None))):
        attach()
        try:
            hooked = ds.tracer_gradient(c.level, t, k, Tb, want_solution=True)
            assert all(np.array_equal(hooked[key], full[key]) for key in keys)
            assert all(np.array_equal(a, b) for a, b in zip(ds.tracer_loglik_gradient(c.level, t, k, data, 0.5), ll0))
            Qh, _, gh = ds.solve_gradient(c.level, k)
            assert np.array_equal(Qh, Q) and np.array_equal(gh, grad_q)
        finally:
            detach()
    transport.close()


@pytest.mark.parametrize("name,hybrid", [("hex1", False), ("tet1", True)])
def test_loglik_gradient(gpu_ctx, name, hybrid):
    from parelagmc_amd import capi
    c, ds, t = ta.case(name), solver(gpu_ctx, ta.case(name).kind, hybrid), tracer_for(gpu_ctx, name)
    rng = np.random.default_rng(5)
    noise = 0.3
    data = ta.twin(name)["T"][0] * (1 + 0.1 * rng.standard_normal(len(c.x0)))
    for wrt_log in (False, True):
        ll, T, nex, grad = ds.tracer_loglik_gradient(c.level, t, c.k, data, noise, wrt_log=wrt_log)
        assert (nex == 0).all()
        want = -((T - data) ** 2).sum(axis=1) / (2 * noise)
        assert np.abs(ll - want).max() <= 1e-12 * np.abs(want).max()
        gen = ds.tracer_gradient(c.level, t, c.k, -(T - data) / noise, wrt_log=wrt_log)
        assert np.array_equal(gen["T"], T)
        d = float((np.abs(grad - gen["grad"]).max(axis=1) / np.abs(gen["grad"]).max(axis=1)).max())
        print(f"{name} hybrid={hybrid} wrt_log={wrt_log}: log-likelihood gradient differs from the general entry by {d:.3g}")
        assert d <= ta.TOL_KT
    # a column with a censored particle: a zero gradient and its count
    free = ta.twin(name)
    short = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0, max_steps=int(free["nsteps"].max()) - 1)
    ll, T, nex, grad = ds.tracer_loglik_gradient(c.level, short, c.k, data, noise)
    run = short.Run(ds.SolveFwd(c.level, c.k, want_solution=True)[2])
    assert np.array_equal(nex, (run["status"] != short.EXITED).sum(axis=1)) and (nex > 0).any() and (nex == 0).any()
    assert (grad[nex > 0] == 0).all() and (np.abs(grad[nex == 0]).max(axis=1) > 0).all()
    short.close()


def test_mirror_classes_compile_and_run(gpu_ctx, tmp_path):
    """ParticleTracer::RunAdjoint, DarcySolver::SolveFwd_TracerGradient and ::ComputeGradTravelTimeLogLikelihood of
    parelagmc.hpp from a C++ caller: RunAdjoint on a two-box channel against a central difference"""
    src = os.path.join(ROOT, "tests", "c", "tracer_adjoint_smoke.cpp")
    exe = str(tmp_path / "tracer_adjoint_smoke")
    lib = os.path.join(ROOT, "parelagmc_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, src, "-L" + lib,
                    "-lpmc_host", "-lpmc", "-pthread", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tracer adjoint smoke ok" in out.stdout

"""The batched derivative entries of the Darcy handle (pmc_darcy_solve_gradient, _loglik_gradient, _transport_gradient,
_transport_loglik_gradient, _tracer_gradient, _tracer_loglik_gradient, _gn_hessvec, _mass_sensitivity, _mass_tangent) cut
a call into launches and stage host operands the same way (Darcy::for_chunks, csrc/darcy.hip).  Five columns make
launches of 4 + 1.  For every output of every entry: host and device memory return the same bits, the call returns the bits
of the two calls on its launches, and a repeated call returns the same bits.  No tolerance anywhere."""
import numpy as np
import pytest

import darcy_gradient_cases as dg
import tracer_adjoint_cases as ta
import tracer_cases as tc
import transport_cases as trc

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
NAME = "hex1"
IDX = [0, 1, 2, 3, 1]
NOISE = 0.5


class Rig:
    """one solver on the level of hex1 with two observation functionals, the case's tracer, a transport on the same mesh, and
    five columns of every operand"""

    def __init__(self, ctx):
        from parelagmc_amd import capi
        c, tm = ta.case(NAME), trc.case(NAME)
        self.ctx, self.level = ctx, c.level
        self.ds = capi.DarcySolver(ctx, tc.problem(c.kind), capi.solver_opts(**TIGHT))
        self.ds.SetObservations(c.level, dg.two_cell_observations(tc.hierarchy(c.kind), c.level))
        self.tracer = capi.Tracer(ctx, c.mesh, c.x0, c.elem0)
        self.transport = capi.Transport(ctx, tm.mesh, tm.t_end, trc.CFL, 4)
        L = tc.problem(c.kind).levels[c.level]
        self.n, self.n_p = L.n_u + L.n_p, L.n_p
        rng = np.random.Generator(np.random.PCG64(20261101))
        self.k = np.ascontiguousarray(c.k[IDX])
        self.cols = dict(
            k=self.k, T_bar=ta.seeds(NAME, ("T_bar",), IDX)["T_bar"], adj_rhs=rng.standard_normal((5, self.n)),
            x=rng.standard_normal((5, self.n)), lam=rng.standard_normal((5, self.n)), dk=rng.standard_normal((5, self.n_p)),
            curve_bar=rng.standard_normal((5, self.transport.nreport)), stored_bar=rng.standard_normal(5))
        self.data = dict(obs=rng.standard_normal(2), curve=rng.uniform(0.1, 1.0, self.transport.nreport),
                         T=rng.uniform(0.5, 2.0, len(c.x0)))

    def close(self):
        for h in (self.transport, self.tracer, self.ds):
            h.close()


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    r = Rig(gpu_ctx)
    yield r
    r.close()


def _host(a, nb):
    """an output as a (nb, -1) numpy array, wherever the entry left it"""
    return (a if isinstance(a, np.ndarray) else a.download()).reshape(nb, -1)


# Every entry: (rig, rows, device) -> dict of its outputs.  `put` hands an operand's rows over in the call's memory space,
# `out` makes an output buffer there.
def _io(rig, rows, device):
    nb = len(range(*rows.indices(5)))
    put = lambda name: rig.ctx.array(rig.cols[name][rows]) if device else np.ascontiguousarray(rig.cols[name][rows])
    out = lambda width: rig.ctx.empty(nb * width) if device else np.empty((nb, width))
    return nb, put, out


def solve_gradient(rig, rows, device, adj_rhs=False):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.solve_gradient(rig.level, put("k"), put("adj_rhs") if adj_rhs else None, nbatch=nb, grad_out=out(rig.n_p),
                              sol_out=out(rig.n), adj_out=out(rig.n))
    return dict(zip(("Q", "C", "grad", "sol", "adj"), r))


def solve_gradient_rhs(rig, rows, device):
    return solve_gradient(rig, rows, device, adj_rhs=True)


def loglik_gradient(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.loglik_gradient(rig.level, put("k"), rig.data["obs"], NOISE, nbatch=nb, grad_out=out(rig.n_p))
    return dict(zip(("loglik", "G", "grad"), r))


def transport_gradient(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.TransportGradient(rig.level, rig.transport, put("k"), put("curve_bar"), put("stored_bar"), nbatch=nb,
                                 grad_out=out(rig.n_p), want_solution=True)
    assert set(r) == {"grad", "curve", "stored", "status", "sol", "adj"}
    return r


def transport_loglik_gradient(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.TransportLoglikGradient(rig.level, rig.transport, put("k"), rig.data["curve"], NOISE, nbatch=nb,
                                       grad_out=out(rig.n_p))
    return dict(zip(("loglik", "curve", "status", "grad"), r))


def tracer_gradient(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.tracer_gradient(rig.level, rig.tracer, put("k"), put("T_bar"), nbatch=nb, grad_out=out(rig.n_p),
                               want_solution=True)
    assert set(r) == {"grad", "T", "status", "sol", "adj"}
    return r


def tracer_loglik_gradient(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    r = rig.ds.tracer_loglik_gradient(rig.level, rig.tracer, put("k"), rig.data["T"], NOISE, nbatch=nb, grad_out=out(rig.n_p))
    return dict(zip(("loglik", "T", "not_exited", "grad"), r))


def gn_hessvec(rig, rows, device):
    """with x_out, and again with that x as x_in"""
    nb, put, out = _io(rig, rows, device)
    hv, dG, x = rig.ds.gn_hessvec(rig.level, put("k"), put("dk"), NOISE, nbatch=nb, hv_out=out(rig.n_p), x_out=out(rig.n))
    hv2, dG2 = rig.ds.gn_hessvec(rig.level, put("k"), put("dk"), NOISE, x_in=x, nbatch=nb, hv_out=out(rig.n_p))
    return dict(hv=hv, dG=dG, x=x, hv_given_x=hv2, dG_given_x=dG2)


def mass_sensitivity(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    return dict(grad=rig.ds.mass_sensitivity(rig.level, put("k"), put("x"), put("lam"), nbatch=nb, grad_out=out(rig.n_p)))


def mass_tangent(rig, rows, device):
    nb, put, out = _io(rig, rows, device)
    return dict(t=rig.ds.mass_tangent(rig.level, put("k"), put("x"), put("dk"), nbatch=nb, t_out=out(rig.n)))


ENTRIES = [solve_gradient, solve_gradient_rhs, loglik_gradient, transport_gradient, transport_loglik_gradient, tracer_gradient,
           tracer_loglik_gradient, gn_hessvec, mass_sensitivity, mass_tangent]


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_entry_splits(rig, entry):
    run = lambda rows, device=False: {key: _host(a, len(range(*rows.indices(5)))) for key, a in entry(rig, rows, device).items()}
    whole = slice(0, 5)
    full = run(whole)
    assert all(a.shape[0] == 5 and a.size > 0 for a in full.values())
    dev, again, head, tail = run(whole, True), run(whole), run(slice(0, 4)), run(slice(4, 5))
    for key, a in full.items():
        assert dev[key].dtype == a.dtype and np.array_equal(dev[key], a), f"{key}: host and device memory differ"
        assert np.array_equal(head[key], a[:4]) and np.array_equal(tail[key], a[4:]), f"{key}: 5 differs from 4 and 1"
        assert np.array_equal(again[key], a), f"{key}: a repeated call differs"
    for key in ("grad", "hv", "t"):
        assert key not in full or (np.abs(full[key]).max(axis=1) > 0).all(), f"{key}: a column of zeros"


def test_solve_gradient_past_the_widest_launch(rig):
    """BatchWidth + 3 columns: launches of bw, 2 and 1.  The first and last columns of every launch against the three calls on
    the same columns."""
    bw = rig.ds.BatchWidth(rig.level)
    k = np.ascontiguousarray(rig.k[np.arange(bw + 3) % 4])
    call = lambda kk: rig.ds.solve_gradient(rig.level, kk, want_solution=True)
    full = call(k)
    parts = [call(k[:bw]), call(k[bw:bw + 2]), call(k[bw + 2:])]
    for name, a, pieces in zip(("Q", "C", "grad", "sol", "adj"), full, zip(*parts)):
        assert a.shape[0] == bw + 3
        joined = np.concatenate(pieces)
        for col in (0, 1, bw - 1, bw, bw + 1, bw + 2):
            assert np.array_equal(a[col], joined[col]), f"{name}: column {col}"

"""The batched entries of the sampler handle (pmc_sampler_eval, _eval_adjoint, _eval_tangent, _mult) and the forward solve of
the Darcy handle (pmc_darcy_solve_fwd, _solve_fwd_pressure) cut a call into launches and stage host operands through the
shared driver (csrc/chunks.hpp).  Five columns make launches of 4 + 1.  For every output of every entry, the per-column
iteration counts and convergence flags included: host and device memory return the same bits, the call returns the bits of
the two calls on its launches, a repeated call returns the same bits, and no column is all zeros.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import sampler_adjoint_cases as cases
import tracer_adjoint_cases as ta
import tracer_cases as tc

pytestmark = pytest.mark.gpu

TIGHT = dict(rel_tol=1e-12, abs_tol=1e-12, max_iter=400)
NAME = "hex1"
IDX = [0, 1, 2, 3, 1]


class Rig:
    """saddle-point, hybridized and lognormal handles on hex84 (n_s = 512 / 64), a gather handle on the ragged mesh, the Darcy
    solvers (plain and hybridized) on the level of hex1, and five columns of every operand"""

    def __init__(self, ctx):
        from parelagmc_amd import capi
        from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
        self.ctx = ctx
        h, o = cases.hierarchy("hex84"), capi.solver_opts(**TIGHT)
        self.smp = dict(
            saddle=capi.PDESampler(ctx, build_sampler_problem(h, corlen=cases.CORLEN), o),
            hybrid=capi.PDESampler(ctx, build_hybrid_sampler_problem(h, corlen=cases.CORLEN), o),
            lognormal=capi.PDESampler(ctx, build_sampler_problem(h, corlen=cases.CORLEN, lognormal=True), o),
            gather=capi.PDESampler(ctx, cases.gather_problem("ragged")[0], o, projection="gather"))
        c = ta.case(NAME)
        self.level = c.level
        self.ds = dict(plain=capi.DarcySolver(ctx, tc.problem(c.kind), o),
                       hybrid=capi.DarcySolver(ctx, tc.problem(c.kind), o, hybrid=True))
        self.k = np.ascontiguousarray(c.k[IDX])
        rng = np.random.Generator(np.random.PCG64(20261121))
        self.cols = {}
        for name, s in self.smp.items():
            L = s.problem.levels[0]
            n_sys = L.n_lambda if s.hybrid else L.n_u + L.n_s
            xi = rng.standard_normal((5, s.xi_size(0)))
            self.cols[name] = dict(xi=xi, dxi=rng.standard_normal((5, s.xi_size(0))), v=rng.standard_normal((5, s.SampleSize(0))),
                                   rhs=rng.standard_normal((5, n_sys)), guess=rng.standard_normal((5, n_sys)),
                                   s=s.Eval(0, xi, xi_level=0), coarse=s.Eval(1, xi, xi_level=0, want_embed=True)[1])

    def close(self):
        for h in list(self.smp.values()) + list(self.ds.values()):
            h.close()


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    r = Rig(gpu_ctx)
    yield r
    r.close()


def _host(a, nb):
    """an output as a (nb, -1) numpy array, wherever the entry left it"""
    return (a if isinstance(a, np.ndarray) else a.download()).reshape(nb, -1)


def _stats(st):
    return np.array([t[:2] for t in st], dtype=np.int64)


# Every entry: (rig, handle name, rows, device) -> dict of its outputs.  `put` hands an operand's rows over in the call's
# memory space, `out` makes an output buffer there.
def _io(rig, name, rows, device):
    nb = len(range(*rows.indices(5)))
    put = lambda key: rig.ctx.array(rig.cols[name][key][rows]) if device else np.ascontiguousarray(rig.cols[name][key][rows])
    out = lambda width: rig.ctx.empty(nb * width) if device else np.empty((nb, width))
    return rig.smp[name], nb, put, out


def eval_same_level(rig, name, rows, device):
    s, nb, put, out = _io(rig, name, rows, device)
    f, emb, st = s.Eval(0, put("xi"), xi_level=0, s_out=out(s.SampleSize(0)), embed_out=out(s.xi_size(0)), return_stats=True)
    return dict(s=f, emb=emb, stats=_stats(st))


def eval_finer_xi(rig, name, rows, device):
    s, nb, put, out = _io(rig, name, rows, device)
    f, st = s.Eval(1, put("xi"), xi_level=0, s_out=out(s.SampleSize(1)), return_stats=True)
    return dict(s=f, stats=_stats(st))


def eval_warm_start(rig, name, rows, device, alias=False):
    """Eval(0) from the coarse field of level 1 with the embedded output; alias: embed_out is the init_s buffer (device
    memory: the rows of init_s at the front of a buffer of nb embedded rows)"""
    s, nb, put, out = _io(rig, name, rows, device or alias)
    n0, n1 = s.xi_size(0), s.xi_size(1)
    if alias:
        emb = rig.ctx.array(np.concatenate([rig.cols[name]["coarse"][rows].ravel(), np.zeros(nb * (n0 - n1))]))
        init = emb
    else:
        emb, init = out(n0), put("coarse")
    f, emb, st = s.Eval(0, put("xi"), xi_level=0, init_s=init, init_level=1, use_init=True, s_out=out(s.SampleSize(0)),
                        embed_out=emb, return_stats=True)
    return dict(s=f, emb=emb, stats=_stats(st))


def eval_warm_start_aliased(rig, name, rows, device):
    return eval_warm_start(rig, name, rows, device, alias=True)


def eval_adjoint(rig, name, rows, device, with_s=False, xi_level=0):
    s, nb, put, out = _io(rig, name, rows, device)
    g, st = s.EvalAdjoint(0, put("v"), s_out=put("s") if with_s else None, xi_level=xi_level, grad_out=out(s.xi_size(xi_level)),
                          nbatch=nb, return_stats=True)
    return dict(grad=g, stats=_stats(st))


def eval_adjoint_s_out(rig, name, rows, device):
    return eval_adjoint(rig, name, rows, device, with_s=True)


def eval_tangent(rig, name, rows, device, with_s=False):
    s, nb, put, out = _io(rig, name, rows, device)
    d, st = s.EvalTangent(0, put("dxi"), s_out=put("s") if with_s else None, xi_level=0, ds_out=out(s.SampleSize(0)), nbatch=nb,
                          return_stats=True)
    return dict(ds=d, stats=_stats(st))


def eval_tangent_s_out(rig, name, rows, device):
    return eval_tangent(rig, name, rows, device, with_s=True)


def solve(rig, name, rows, device, guess=False):
    s, nb, put, out = _io(rig, name, rows, device)
    x, st = s.Solve(0, put("rhs"), guess=put("guess") if guess else None, return_stats=True)
    return dict(x=x, stats=_stats(st))


def solve_with_guess(rig, name, rows, device):
    return solve(rig, name, rows, device, guess=True)


def _solve_fwd(rig, name, k, device, sol):
    """sol: None, "full" or "pressure" (pmc_darcy_solve_fwd_pressure, called directly: the Python layer has it for host memory
    only)"""
    from parelagmc_amd import capi
    ds, nb = rig.ds[name], k.shape[0]
    kk = rig.ctx.array(k) if device else np.ascontiguousarray(k)
    if sol != "pressure":
        width = ds.GetGlobalNumberOfDofs(rig.level)
        so = None if sol is None else (rig.ctx.empty(nb * width) if device else np.empty((nb, width)))
        r = ds.SolveFwd(rig.level, kk, nbatch=nb, sol_out=so, return_stats=True)
        return dict(zip(("Q", "C", "sol", "stats") if sol else ("Q", "C", "stats"), r[:-1] + (_stats(r[-1]),)))
    n_p = ds.problem.levels[rig.level].n_p
    P = rig.ctx.empty(nb * n_p) if device else np.empty((nb, n_p))
    Q, Cc, st = np.empty(nb), np.empty(nb), (capi.pmc_stats * nb)()
    dbl = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pk, ms = capi._addr(kk)
    rc = rig.ctx.lib.pmc_darcy_solve_fwd_pressure(ds.h, rig.level, nb, pk, capi._addr(P)[0], dbl(Cc), dbl(Q), 1, ms, st)
    assert rc == 0, rig.ctx.lib.pmc_last_error().decode()
    return dict(Q=Q, C=Cc, sol=P, stats=_stats([(t.iterations, t.converged) for t in st]))


def solve_fwd(rig, name, rows, device):
    return _solve_fwd(rig, name, rig.k[rows], device, None)


def solve_fwd_solution(rig, name, rows, device):
    return _solve_fwd(rig, name, rig.k[rows], device, "full")


def solve_fwd_pressure(rig, name, rows, device):
    return _solve_fwd(rig, name, rig.k[rows], device, "pressure")


SAMPLERS = ("saddle", "hybrid", "lognormal", "gather")
CASES = ([(e, n) for e in (eval_same_level, eval_finer_xi, eval_adjoint, eval_tangent) for n in SAMPLERS] +
         [(e, n) for e in (eval_warm_start, eval_warm_start_aliased) for n in ("saddle", "lognormal", "gather")] +
         [(e, "lognormal") for e in (eval_adjoint_s_out, eval_tangent_s_out)] +
         [(e, n) for e in (solve, solve_with_guess) for n in ("saddle", "hybrid")] +
         [(e, n) for e in (solve_fwd, solve_fwd_solution, solve_fwd_pressure) for n in ("plain", "hybrid")])


@pytest.mark.parametrize("entry,name", CASES, ids=lambda a: a if isinstance(a, str) else a.__name__)
def test_entry_splits(rig, entry, name):
    run = lambda rows, device=False: {key: _host(a, len(range(*rows.indices(5)))) for key, a in entry(rig, name, rows, device).items()}
    whole = slice(0, 5)
    full = run(whole)
    assert all(a.shape[0] == 5 and a.size > 0 for a in full.values())
    dev, again, head, tail = run(whole, True), run(whole), run(slice(0, 4)), run(slice(4, 5))
    for key, a in full.items():
        assert dev[key].dtype == a.dtype and np.array_equal(dev[key], a), f"{key}: host and device memory differ"
        assert np.array_equal(head[key], a[:4]) and np.array_equal(tail[key], a[4:]), f"{key}: 5 differs from 4 and 1"
        assert np.array_equal(again[key], a), f"{key}: a repeated call differs"
        assert (np.abs(a).max(axis=1) > 0).all(), f"{key}: a column of zeros"
    if entry is eval_warm_start_aliased:   # (device memory in every run above) the bits of the call on two buffers
        apart = {key: _host(a, 5) for key, a in eval_warm_start(rig, name, whole, False).items()}
        assert all(np.array_equal(apart[key], a) for key, a in full.items()), "the aliased call differs from the call on two buffers"


def _columns_equal(full, parts, bw):
    for key, a in full.items():
        assert a.shape[0] == bw + 3
        joined = np.concatenate([p[key] for p in parts])
        for col in (0, bw - 1, bw, bw + 1, bw + 2):
            assert np.array_equal(a[col], joined[col]), f"{key}: column {col}"


@pytest.mark.parametrize("name", ("saddle", "hybrid"))
def test_eval_past_the_widest_launch(rig, name):
    """BatchWidth + 3 columns in host memory: launches of bw, 2 and 1.  The first and last columns of every launch against the
    three calls on the same columns."""
    s = rig.smp[name]
    bw = s.BatchWidth(0)
    xi = np.ascontiguousarray(rig.cols[name]["xi"][np.arange(bw + 3) % 5])

    def call(x):
        f, emb, st = s.Eval(0, x, xi_level=0, want_embed=True, return_stats=True)
        return dict(s=f, emb=emb, stats=_stats(st))
    _columns_equal(call(xi), [call(xi[:bw]), call(xi[bw:bw + 2]), call(xi[bw + 2:])], bw)


@pytest.mark.parametrize("name", ("plain", "hybrid"))
def test_solve_fwd_past_the_widest_launch(rig, name):
    """the same for SolveFwd with the full solution"""
    bw = rig.ds[name].BatchWidth(rig.level)
    k = np.ascontiguousarray(rig.k[np.arange(bw + 3) % 4])
    call = lambda kk: {key: _host(a, kk.shape[0]) for key, a in _solve_fwd(rig, name, kk, False, "full").items()}
    _columns_equal(call(k), [call(k[:bw]), call(k[bw:bw + 2]), call(k[bw + 2:])], bw)

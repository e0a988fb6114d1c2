"""The batched CG kernels behind Newton-CG (pmc_ncg_*: csrc/newton_cg.hip) without any PDE: the
operator is H = I + U U^T applied by numpy on the host, per column; a reference runs the same CG in longdouble.

Bounds.  A dot product over n entries is summed as: 16 entries per thread, an 8-level tree over the workgroup's 256 threads
(6 shuffle levels and the 4 wave sums), then the chunk sums in ascending order - a summation depth of
DEPTH(n) = min(n, 16) + 9 + (chunks - 1), so its first-order bound is DEPTH(n) u sum |a_i b_i|, u = 2^-53.  The vectors
inherit the scalars' errors step by step, amplified by the conditioning of H (about 130 at every n: problem()); the tests
measure
    ratio = |v - v_ref|_2 / ((step + 1) DEPTH(n) u |scale|),   scale = |d_ref| for d, |g| for r and p (they start at g and
                                                                shrink by cancellation), <g, g> for <r, r>,
print its maximum and assert 10 x the value measured on an MI355X: MEASURED_RATIO, recorded below.  The kernels are
deterministic, so the measured values are the same on every MI355X.
axpy_cols is one fma per entry (bound 2 u (|x| + |t d|) per entry, asserted as it stands) and dot_cols one dot (asserted
against DEPTH(n) u sum |a_i b_i| as it stands, no factor).  Bitwise statements are asserted bitwise."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 4096
NS = [1, 6, 63, 64, 65, 240, CHUNK - 1, CHUNK, CHUNK + 1, 40000]
NBS = [67, 1, 3, 4, 5, 64]
NBMAX = 67
STEPS = 4
U53 = 2.0 ** -53
MEASURED_RATIO = 18.3       # n = 65; between 4.7 (n = 40 000) and 18.3 over the sizes with more than one entry, 0.26 at n = 1
TOL_RATIO = 10 * MEASURED_RATIO
LD = np.longdouble


def depth(n):
    return min(n, 16) + 9 + ((n + CHUNK - 1) // CHUNK - 1)


def column_kind(b):
    """what column b is, whatever batch it sits in: 'masked', 'npc' (the operator returns -p), 'loose' (eta 0.3: ends
    early) or 'tight' (eta 1e-3)"""
    if b % 7 == 3:
        return "masked"
    if b % 11 == 6:
        return "npc"
    return "loose" if b % 5 == 1 else "tight"


def etas(cols):
    return np.array([0.3 if column_kind(b) == "loose" else 1e-3 for b in cols])


@functools.lru_cache(maxsize=None)
def problem(n):
    rng = np.random.default_rng(1000 + n)
    rank = min(8, n)
    # columns of norm about 2^(j/2): the eigenvalues of H = I + U U^T are about 1 + 2^j, j < 8, at every n, so that the
    # conditioning (about 130), and with it the measured ratio, does not grow with n
    U = rng.standard_normal((n, rank)) / np.sqrt(n) * np.sqrt(2.0 ** np.arange(rank))
    g = rng.standard_normal((NBMAX, n))
    junk = rng.standard_normal((3, NBMAX, n))       # what d, r, p hold before pmc_ncg_begin
    return U, g, junk


def apply_H(n, p, cols, dtype=np.float64):
    """H p per column (numpy, on the host), -p on the 'npc' columns; one matrix-vector product per column, so that a column's
    product does not depend on the batch it is computed in (a matrix-matrix product's rounding does)"""
    U = problem(n)[0].astype(dtype)
    p = p.astype(dtype)
    hp = np.stack([pb + U @ (U.T @ pb) for pb in p])
    for i, b in enumerate(cols):
        if column_kind(b) == "npc":
            hp[i] = -p[i]
    return hp


@functools.lru_cache(maxsize=None)
def reference(n):
    """the CG of all NBMAX columns in longdouble with the kernels' decisions: per step (d, r, p, rr, count, done, npc), and
    the smallest relative margin of a tolerance decision"""
    U, g, junk = problem(n)
    cols = list(range(NBMAX))
    g = g.astype(LD)
    d, r, p = (junk[i].astype(LD) for i in range(3))
    active = np.array([column_kind(b) != "masked" for b in cols])
    eta = etas(cols).astype(LD)
    rr = np.zeros(NBMAX, LD)
    tol2 = np.zeros(NBMAX, LD)
    count, npc = np.zeros(NBMAX, np.int32), np.zeros(NBMAX, np.int32)
    done = ~active
    for b in cols:
        if active[b]:
            d[b], r[b], p[b] = 0, g[b], g[b]
            rr[b] = g[b] @ g[b]
            tol2[b] = eta[b] * eta[b] * rr[b]
        else:
            p[b] = 0
    snaps, margin = [], np.inf
    for _ in range(STEPS):
        hp = apply_H(n, p, cols, LD)
        for b in cols:
            if done[b]:
                continue
            php = p[b] @ hp[b]
            count[b] += 1
            if not php > 0:
                if count[b] == 1:
                    d[b] = p[b]
                npc[b], done[b] = 1, True
                p[b] = 0
                continue
            alpha = rr[b] / php
            d[b] = d[b] + alpha * p[b]
            r[b] = r[b] - alpha * hp[b]
            new = r[b] @ r[b]
            margin = min(margin, float(abs(new - tol2[b]) / tol2[b]))
            if not new > tol2[b]:
                done[b] = True
                p[b] = 0
            else:
                p[b] = r[b] + (new / rr[b]) * p[b]
            rr[b] = new
        snaps.append((d.copy(), r.copy(), p.copy(), rr.copy(), count.copy(), done.copy(), npc.copy()))
    return snaps, margin


def run_device(ctx, ncg, n, cols, device_memory):
    """begin + STEPS steps of the columns `cols` (ids into the 67 of problem(n)); returns the snapshots (d, r, p, rr, count,
    done, npc) after every step, as float64 / int arrays downloaded from the workspace"""
    U, g, junk = problem(n)
    nb = len(cols)
    lib, h = ctx.lib, ctx.h
    for ptr, a in zip((ncg.direction_ptr(), ncg.residual_ptr(), ncg.search_direction_ptr()), junk):
        a = np.ascontiguousarray(a[cols])
        assert lib.pmc_memcpy_h2d(h, ptr, a.ctypes.data, a.nbytes) == 0
    put = (lambda a: ctx.array(a)) if device_memory else (lambda a: np.ascontiguousarray(a))
    gb = put(g[cols])
    ncg.begin(nb, gb, etas(cols), [0 if column_kind(b) == "masked" else 1 for b in cols])
    snaps = []
    for _ in range(STEPS):
        hp = put(apply_H(n, ncg.search_direction(nb), cols))
        ncg.step(nb, hp)
        rr, count, done, npc = ncg.status(nb)
        snaps.append((ncg.direction(nb), ncg.residual(nb), ncg.search_direction(nb), rr, count, done, npc))
        if device_memory:
            hp.free()
    if device_memory:
        gb.free()
    return snaps


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64) if np.asarray(a).dtype == np.float64 else a,
                          np.asarray(b).view(np.uint64) if np.asarray(b).dtype == np.float64 else b)


@pytest.mark.parametrize("device_memory", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", NS)
def test_cg_steps(gpu_ctx, n, device_memory):
    from parelagmc_amd import capi
    ref, margin = reference(n)
    assert margin > 1e-6, f"the test's own data decide a tolerance test by {margin:.1e}: choose another seed"
    U, g, junk = problem(n)
    ncg = capi.NewtonCG(gpu_ctx, n, NBMAX)
    base = None
    worst = 0.0
    for nb in NBS:
        cols = list(range(nb))
        snaps = run_device(gpu_ctx, ncg, n, cols, device_memory)
        if base is None:
            base = snaps
            again = run_device(gpu_ctx, ncg, n, cols, device_memory)
            assert all(same_bits(x, y) for s, t in zip(snaps, again) for x, y in zip(s, t)), "two identical runs differ"
        for step, (s, b67, rf) in enumerate(zip(snaps, base, ref)):
            for q in range(7):
                assert same_bits(s[q], np.asarray(b67[q])[:nb]), f"n {n} nb {nb} step {step}: item {q} depends on the batch"
            scale = (step + 1) * depth(n) * U53
            for b in cols:
                if column_kind(b) == "masked":
                    continue
                # r and p start at g and shrink by cancellation: their errors are measured against |g|, <r, r> against <g, g>
                ng = float(np.linalg.norm(g[b]))
                for q, nv in ((0, float(np.linalg.norm(rf[0][b]))), (1, ng), (2, ng)):
                    worst = max(worst, float(np.linalg.norm(s[q][b].astype(LD) - rf[q][b])) / (scale * nv))
                worst = max(worst, float(abs(LD(s[3][b]) - rf[3][b])) / (scale * ng * ng))
            assert np.array_equal(s[4], rf[4][:nb]) and np.array_equal(s[5] != 0, rf[5][:nb]) and np.array_equal(s[6], rf[6][:nb])
        # masked columns: d and r untouched, p zero; finished columns: nothing written after the step that ended them
        for b in cols:
            if column_kind(b) == "masked":
                for s in snaps:
                    assert same_bits(s[0][b], junk[0][b]) and same_bits(s[1][b], junk[1][b]) and not s[2][b].any()
            if column_kind(b) == "npc":
                assert snaps[0][6][b] == 1 and same_bits(snaps[0][0][b], g[b])      # d = g at the first step
            for step in range(1, STEPS):
                if snaps[step - 1][5][b]:
                    assert all(same_bits(snaps[step][q][b], snaps[step - 1][q][b]) for q in range(3))
                    assert not snaps[step][2][b].any()
    # beside other neighbours, in another order
    cols = [9, 2, 66, 5, 1] if n != 40000 else [9, 2, 5]
    snaps = run_device(gpu_ctx, ncg, n, cols, device_memory)
    for s, b67 in zip(snaps, base):
        for q in range(7):
            assert same_bits(s[q], np.asarray(b67[q])[cols]), f"n {n}: item {q} depends on the neighbours"
    ncg.close()
    print(f"n {n} {'device' if device_memory else 'host'}: worst ratio to the summation bound {worst:.3f} "
          f"(smallest decision margin {margin:.1e})")
    assert worst <= TOL_RATIO


@pytest.mark.parametrize("device_memory", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", NS)
def test_axpy_and_dot_cols(gpu_ctx, n, device_memory):
    from parelagmc_amd import capi
    rng = np.random.default_rng(2000 + n)
    x, d, o = (rng.standard_normal((NBMAX, n)) for _ in range(3))
    t = rng.standard_normal(NBMAX)
    t[[b for b in range(NBMAX) if b % 4 == 2]] = 0.0
    ncg = capi.NewtonCG(gpu_ctx, n, NBMAX)
    put = (lambda a: gpu_ctx.array(a)) if device_memory else (lambda a: np.array(a, order="C"))
    get = (lambda a, nb: a.download().reshape(nb, n)) if device_memory else (lambda a, nb: a)
    base = {}
    worst_dot = 0.0
    for nb in NBS:
        xa, da, oa = put(x[:nb]), put(d[:nb]), put(o[:nb])
        out = get(ncg.axpy_cols(nb, t[:nb], xa, da, oa), nb).copy()
        cp = put(o[:nb])
        copy = get(ncg.axpy_cols(nb, t[:nb], xa, None, cp), nb).copy()
        dots = ncg.dot_cols(nb, xa, da)
        xin = put(x[:nb])
        inplace = get(ncg.axpy_cols(nb, t[:nb], xin, da, xin), nb).copy()
        assert same_bits(ncg.dot_cols(nb, xa, da), dots)
        for b in range(nb):
            if t[b] == 0.0:
                assert same_bits(out[b], o[b]) and same_bits(copy[b], o[b]) and same_bits(inplace[b], x[b])
            else:
                refv = x[b].astype(LD) + LD(t[b]) * d[b].astype(LD)
                assert np.all(np.abs(out[b].astype(LD) - refv) <= 2 * U53 * (np.abs(x[b]) + np.abs(t[b] * d[b])))
                assert same_bits(copy[b], x[b]) and same_bits(inplace[b], out[b])
            refd = x[b].astype(LD) @ d[b].astype(LD)
            bound = depth(n) * U53 * float(np.abs(x[b]) @ np.abs(d[b]))
            worst_dot = max(worst_dot, float(abs(LD(dots[b]) - refd)) / bound)
        if not base:
            base = dict(out=out, dots=dots)
        assert same_bits(out, base["out"][:nb]) and same_bits(dots, base["dots"][:nb])
        if device_memory:
            for a in (xa, da, oa, cp, xin):
                a.free()
    # other neighbours
    cols = [9, 3, 66, 5]
    xa, da, oa = put(x[cols]), put(d[cols]), put(o[cols])
    tt = t[cols].copy()
    out = get(ncg.axpy_cols(4, tt, xa, da, oa), 4)
    assert same_bits(out, base["out"][cols]) and same_bits(ncg.dot_cols(4, xa, da), base["dots"][cols])
    # the workspace's own direction as an operand, in either memory space
    assert gpu_ctx.lib.pmc_memcpy_h2d(gpu_ctx.h, ncg.direction_ptr(), np.ascontiguousarray(d[cols]).ctypes.data, 4 * n * 8) == 0
    ob = put(o[cols])
    ms = capi.PMC_MEM_DEVICE if device_memory else capi.PMC_MEM_HOST
    import ctypes as C
    assert gpu_ctx.lib.pmc_ncg_axpy_cols(ncg.h, 4, tt.ctypes.data_as(C.POINTER(C.c_double)), capi._addr(xa)[0],
                                         ncg.direction_ptr(), capi._addr(ob)[0], ms) == 0
    assert same_bits(get(ob, 4), base["out"][cols])
    ncg.close()
    print(f"n {n}: dot_cols at most {worst_dot:.3f} of its summation bound")
    assert worst_dot <= 1.0


def test_ncg_refusals(gpu_ctx):
    import ctypes as C
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    h = C.c_void_p()
    for n, nb in ((0, 1), (1, 0), (-3, 4)):
        assert lib.pmc_ncg_create(gpu_ctx.h, n, nb, C.byref(h)) == -1
    assert lib.pmc_ncg_create(None, 4, 4, C.byref(h)) == -1
    ncg = capi.NewtonCG(gpu_ctx, 6, 4)
    g = np.ones((4, 6))
    H = capi.PMC_MEM_HOST
    dp = C.POINTER(C.c_double)
    eta = np.full(4, 0.5)
    pe, pg = eta.ctypes.data_as(dp), g.ctypes.data
    assert lib.pmc_ncg_begin(ncg.h, 5, pg, pe, None, H) == -1
    assert lib.pmc_ncg_begin(ncg.h, 0, pg, pe, None, H) == -1
    assert lib.pmc_ncg_begin(ncg.h, 4, None, pe, None, H) == -1
    assert lib.pmc_ncg_begin(ncg.h, 4, pg, None, None, H) == -1
    assert lib.pmc_ncg_begin(ncg.h, 4, pg, pe, None, 7) == -1
    assert lib.pmc_ncg_begin(ncg.h, 4, pg, (-eta).ctypes.data_as(dp), None, H) == -1
    assert lib.pmc_ncg_begin(None, 4, pg, pe, None, H) == -1
    assert lib.pmc_ncg_begin(ncg.h, 3, pg, pe, None, H) == 0
    assert lib.pmc_ncg_step(ncg.h, 4, pg, H) == -1 and "begin" in lib.pmc_last_error().decode()
    assert lib.pmc_ncg_step(ncg.h, 3, None, H) == -1
    assert lib.pmc_ncg_step(ncg.h, 3, pg, H) == 0
    out = np.empty(4)
    assert lib.pmc_ncg_dot_cols(ncg.h, 4, pg, pg, None, H) == -1 and lib.pmc_ncg_dot_cols(ncg.h, 4, None, pg, out.ctypes.data_as(dp), H) == -1
    assert lib.pmc_ncg_axpy_cols(ncg.h, 4, None, pg, pg, pg, H) == -1 and lib.pmc_ncg_axpy_cols(ncg.h, 4, pe, pg, pg, None, H) == -1
    assert lib.pmc_ncg_status(ncg.h, 5, None, None, None, None) == -1
    assert lib.pmc_ncg_direction(None) is None
    ncg.close()

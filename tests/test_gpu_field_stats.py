"""On-device field statistics and L2 / max errors (pmc_field_stats_*, pmc_sampler_l2_error / _max_error) on every kind of
sampler handle: exactness against math.fsum, bit-identical results for every split of the samples, the errors against
numpy through the handle's own prolongators, the statistics of PDESamplerTest's problem, and the refused calls.
Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KINDS = ["saddle", "hybrid", "gather", "l2", "kl_gauss", "kl_logn"]
NS = 10


def _embedded_hierarchy():
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    m = box_mesh([6, 6, 6], [3.0, 3.0, 3.0], "hex", origin=[-0.5, -0.5, -0.5])     # Build3DHexEnlargedMesh
    cen = m.verts[m.elems].mean(1)
    m.elem_attr[:] = np.where(np.all((cen > 0) & (cen < 2), axis=1), 1, 2)
    return build_hierarchy(m, 2)


_HE = []


def _make(ctx, kind, hier):
    """(sampler, output hierarchy (P list, w0) or None for the handle's own)"""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import (build_hybrid_sampler_problem, build_kl_sampler_problem, build_sampler_problem,
                                  l2_projection_hierarchy)
    if kind == "saddle":
        return capi.PDESampler(ctx, build_sampler_problem(hier, corlen=0.1)), None
    if kind == "hybrid":
        return capi.PDESampler(ctx, build_hybrid_sampler_problem(hier, corlen=0.1)), None
    if kind.startswith("kl"):
        return capi.KLSampler(ctx, build_kl_sampler_problem(hier, "analytic", corlen=0.1, lognormal=kind == "kl_logn")), None
    if not _HE:
        _HE.append(_embedded_hierarchy())
    he = _HE[0]
    if kind == "gather":
        sp_ = build_sampler_problem(he, corlen=0.1, embedded=True)
        idx = sp_.orig_index
        P = [he.P[l][idx[l]][:, idx[l + 1]].tocsr() for l in range(len(idx) - 1)]
        return capi.PDESampler(ctx, sp_, projection="gather"), (P, he.spaces[0].vol[idx[0]])
    smp = capi.PDESampler(ctx, build_sampler_problem(he, corlen=0.1), projection="l2",
                          l2_ops=l2_projection_hierarchy(hier, he))
    return smp, (list(hier.P), hier.spaces[0].vol)


def _chi(smp, hier, kind, level):
    """the drivers' indicator on `level` (a fixed element of the output numbering for the projected kinds)"""
    from parelagmc_amd.fe import chi_center_of_mass, restrict_chi
    if kind in ("gather", "l2"):
        chi = np.zeros(smp.SampleSize(level))
        chi[smp.SampleSize(level) // 3] = 1.0
        return chi
    return restrict_chi(chi_center_of_mass(hier.spaces[0]), hier.P)[level]


def _tiles(smp, level, N):
    """Eval output of ids 0 .. N-1 on the launch grid run() uses (launches of BatchWidth on multiples of it)"""
    W = smp.BatchWidth(level)
    s = [smp.Eval(level, smp.Sample(level, first_id=t * W, nbatch=W), xi_level=level) for t in range((N + W - 1) // W)]
    return np.concatenate(s)[:N]


@pytest.mark.parametrize("kind", KINDS)
def test_accumulators_are_compensated_sums(gpu_ctx, hex_hierarchy, kind):
    from parelagmc_amd import capi
    smp, _ = _make(gpu_ctx, kind, hex_hierarchy)
    level = 1
    s = smp.Eval(level, smp.Sample(level, first_id=100, nbatch=70), xi_level=level)
    chi = _chi(smp, hex_hierarchy, kind, level)
    fs = capi.FieldStatistics(smp, level, chi)
    fs.accumulate(s[:33]).accumulate(s[33:])
    acc, N = fs.read_sums()
    assert N == 70 and acc.shape == (6, s.shape[1])
    d = fs.chi_dot(s)
    assert np.allclose(d, s @ chi, rtol=1e-13, atol=1e-13 * np.abs(s).sum(axis=1).max())
    for k, terms in enumerate((s, s * s, d[:, None] * s)):       # the products rounded as the kernel rounds them
        got = acc[2 * k] + acc[2 * k + 1]
        for i in range(s.shape[1]):
            col = terms[:, i].tolist()
            ex = math.fsum(col)
            bound = 2 * EPS * abs(ex) + N * EPS * EPS * math.fsum(abs(x) for x in col)
            assert abs(got[i] - ex) <= bound, (kind, k, i, got[i], ex)
    e, m2, cc, n = fs.read()
    assert n == N
    for k, r in enumerate((e, m2, cc)):
        assert np.array_equal(r, (acc[2 * k] + acc[2 * k + 1]) * (1.0 / N))
    fs.close()
    smp.close()


@pytest.mark.parametrize("kind", KINDS)
def test_statistics_do_not_depend_on_the_split(gpu_ctx, hex_hierarchy, kind):
    from parelagmc_amd import capi
    smp, _ = _make(gpu_ctx, kind, hex_hierarchy)
    level = 1
    W = smp.BatchWidth(level)
    N = 2 * W + 5
    chi = _chi(smp, hex_hierarchy, kind, level)
    ref = capi.FieldStatistics(smp, level, chi).run(0, N).read_sums()[0]
    fs = capi.FieldStatistics(smp, level, chi)
    first = 0
    for n in (1, 3, W, N - W - 4):                   # ... the last chunk ragged
        fs.run(first, n)
        first += n
    got, cnt = fs.read_sums()
    assert cnt == N and np.array_equal(got, ref), kind
    # the same realizations held by the caller, fed in arbitrary splits
    s = _tiles(smp, level, N)
    fs.reset()
    for a, b in ((0, 5), (5, 6), (6, 23), (23, N)):
        fs.accumulate(s[a:b])
    assert np.array_equal(fs.read_sums()[0], ref), kind
    # a column's <chi, s> alone == inside a launch of 256
    S = np.concatenate([s, s[: 256 - len(s) % 256]])[:256] if len(s) < 256 else s[:256]
    assert S.shape[0] == 256
    d_all = fs.chi_dot(S)
    for c in (0, 7, 131, 255):
        assert np.array_equal(fs.chi_dot(S[c:c + 1]), d_all[c:c + 1])
    fs.close()
    smp.close()


@pytest.mark.parametrize("kind", KINDS)
def test_l2_and_max_errors_match_numpy(gpu_ctx, hex_hierarchy, kind, seeded_rng):
    from parelagmc_amd import capi
    smp, outh = _make(gpu_ctx, kind, hex_hierarchy)
    exact = 0.3
    levels = range(smp.nlevels)
    if outh is not None:
        for lvl in levels:   # the output lives on the original mesh: refused until its hierarchy is handed over
            c = np.zeros(smp.SampleSize(lvl))
            for fn in (smp.ComputeL2Error, smp.ComputeMaxError):
                with pytest.raises(capi.PmcError) as e:
                    fn(lvl, c, exact)
                assert e.value.code == -1
        smp.SetOutputHierarchy(*outh)
    for lvl in levels:
        n = smp.SampleSize(lvl)
        coeff = np.concatenate([seeded_rng.standard_normal((4, n)),
                                smp.Eval(lvl, smp.Sample(lvl, first_id=7, nbatch=3), xi_level=lvl)])
        x = coeff.T
        for l in range(lvl - 1, -1, -1):
            x = (outh[0][l] if outh else smp.GetTrueP(l)) @ x
        w0 = outh[1] if outh else hex_hierarchy.spaces[0].vol
        ref = ((x - exact) ** 2 * w0[:, None]).sum(axis=0)
        got = smp.ComputeL2Error(lvl, coeff, exact)
        assert np.allclose(got, ref, rtol=1e-12, atol=0), (kind, lvl)
        assert smp.ComputeL2Error(lvl, coeff[2], exact) == got[2]
        mx = np.maximum(coeff.max(axis=1) - exact, exact - coeff.min(axis=1))
        assert np.array_equal(smp.ComputeMaxError(lvl, coeff, exact), mx), (kind, lvl)
        dev = gpu_ctx.array(coeff)      # device-resident fields
        assert np.array_equal(smp.ComputeL2Error(lvl, dev, exact), got)
        dev.free()
    smp.close()


def test_statistics_of_pdesamplertest(gpu_ctx, hex_hierarchy):
    """PDESamplerTest's problem (4^3 hex on [0,2]^3 refined twice, corlen 0.1), N = 4096 realizations of level 1 through
    FieldStatistics.run, against the oracle's exact moments var_i = sum_j G_ij^2 of the linear map xi -> s."""
    from oracle.sampler_oracle import SamplerOracle
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem, chi_center_of_mass, restrict_chi
    sp = build_sampler_problem(hex_hierarchy, corlen=0.1)
    so = SamplerOracle(sp)
    n = sp.levels[1].n_s
    G = np.stack([so.eval(1, 1, e)[0] for e in np.eye(n)], axis=1)
    var = (G ** 2).sum(axis=1)
    smp = capi.PDESampler(gpu_ctx, sp)
    chi = restrict_chi(chi_center_of_mass(hex_hierarchy.spaces[0]), hex_hierarchy.P)[1]
    N = 4096
    fs = capi.FieldStatistics(smp, 1, chi).run(0, N)
    mean, m2, cc, cnt = fs.read()
    assert cnt == N
    z = mean / np.sqrt(var / N)
    assert np.abs(z).max() < 5.0 and abs(z.mean()) < 0.5
    ratio = m2 / var                       # the second moment about zero: E[s^2] = var
    assert np.abs(ratio - 1.0).max() < 0.15 and abs(ratio.mean() - 1.0) < 0.02
    cov = G @ (G.T @ chi)                  # E[<chi, s> s] = G G^T chi
    assert np.abs(cc - cov).max() < 6.0 * np.sqrt(np.max(var) * (chi @ (G @ G.T) @ chi) / N) + 1e-12
    # the L2 errors of the table against the exact moments
    e1 = smp.ComputeL2Error(1, mean, 0.0)
    assert e1 == pytest.approx(float(((mean) ** 2) @ hex_hierarchy.spaces[1].vol), rel=1e-12)
    fs.close()
    smp.close()


def _typical(golden, draws, what, nsig=3.3):
    m, s = float(np.mean(draws)), float(np.std(draws))
    print(f"[pin] {what}: reference {golden} | here {m:.4f} +- {s:.4f} | z = {(golden - m) / s:+.2f}")
    assert abs(golden - m) <= nsig * s, f"{what}: reference {golden} vs {m:.4f} +- {s:.4f} here"


def test_pdesamplertest_golden_column_through_field_statistics(gpu_ctx, hex_hierarchy):
    """|| E_10[s] ||_L2 on three levels (the goldens 1.2593 / 0.93103 / 0.63853 of PDESamplerTest) as FieldStatistics +
    ComputeL2Error compute them: the reference's draw must be a typical one."""
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_sampler_problem
    smp = capi.PDESampler(gpu_ctx, build_sampler_problem(hex_hierarchy, corlen=0.1))
    reps = 300
    for lvl, gold in enumerate((1.2593, 9.3103e-01, 6.3853e-01)):
        s = smp.Eval(lvl, smp.Sample(lvl, first_id=10_000 * (lvl + 1), nbatch=reps * NS))
        fs = capi.FieldStatistics(smp, lvl)
        E = []
        for r in range(reps):
            fs.reset().accumulate(s[r * NS:(r + 1) * NS])
            E.append(fs.read()[0])
        t = np.sqrt(smp.ComputeL2Error(lvl, np.array(E), 0.0))
        _typical(gold, t, f"PDESamplerTest level {lvl} (field statistics)")
        fs.close()
    smp.close()


def test_invalid_calls_are_refused(gpu_ctx, hex_hierarchy):
    from parelagmc_amd import capi
    lib = gpu_ctx.lib
    smp, _ = _make(gpu_ctx, "saddle", hex_hierarchy)
    n = smp.SampleSize(1)
    buf = np.zeros(4 * n)
    p = buf.ctypes.data
    h = C.c_void_p()
    assert lib.pmc_field_stats_create(smp.h, smp.nlevels, None, 0, C.byref(h)) == -1      # level out of range
    assert lib.pmc_field_stats_create(smp.h, -1, None, 0, C.byref(h)) == -1
    assert lib.pmc_field_stats_create(None, 1, None, 0, C.byref(h)) == -1                 # NULL handle
    assert lib.pmc_field_stats_create(smp.h, 1, None, 0, None) == -1
    fs = capi.FieldStatistics(smp, 1)                     # without chi
    cnt = C.c_int64(0)
    assert lib.pmc_field_stats_read(fs.h, p, None, None, C.byref(cnt), 0) == -1           # N = 0
    assert lib.pmc_field_stats_accumulate(fs.h, 0, p, 0) == -1                            # nbatch < 1
    assert lib.pmc_field_stats_accumulate(fs.h, 1, None, 0) == -1                         # NULL buffer
    assert lib.pmc_field_stats_accumulate(None, 1, p, 0) == -1
    assert lib.pmc_field_stats_run(fs.h, 0, 0) == -1                                      # nsamples < 1
    assert lib.pmc_field_stats_run(fs.h, 0, -3) == -1
    assert lib.pmc_field_stats_run(None, 0, 1) == -1
    assert lib.pmc_field_stats_reset(None) == -1
    fs.accumulate(buf[:n].reshape(1, n))
    assert lib.pmc_field_stats_read(fs.h, None, None, p, C.byref(cnt), 0) == -1           # chi_cov without chi
    assert lib.pmc_field_stats_read(None, p, None, None, C.byref(cnt), 0) == -1
    assert lib.pmc_field_stats_chi_dot(fs.h, 1, p, p, 0) == -1
    assert lib.pmc_field_stats_read(fs.h, p, p, None, C.byref(cnt), 0) == 0 and cnt.value == 1
    err = np.zeros(2)
    for fn in (lib.pmc_sampler_l2_error, lib.pmc_sampler_max_error):
        assert fn(smp.h, smp.nlevels, 1, p, 0.0, err.ctypes.data, 0) == -1                # level out of range
        assert fn(smp.h, -1, 1, p, 0.0, err.ctypes.data, 0) == -1
        assert fn(smp.h, 1, 0, p, 0.0, err.ctypes.data, 0) == -1                          # nbatch < 1
        assert fn(smp.h, 1, 1, None, 0.0, err.ctypes.data, 0) == -1                       # NULL buffers
        assert fn(smp.h, 1, 1, p, 0.0, None, 0) == -1
        assert fn(None, 1, 1, p, 0.0, err.ctypes.data, 0) == -1
    w = np.ones(smp.SampleSize(0))
    assert lib.pmc_sampler_set_output_hierarchy(smp.h, 0, None, w.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert lib.pmc_sampler_set_output_hierarchy(smp.h, 2, None, w.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert lib.pmc_sampler_set_output_hierarchy(None, 1, None, w.ctypes.data_as(C.POINTER(C.c_double))) == -1
    with pytest.raises(capi.PmcError):                    # a prolongator of the wrong shape
        smp.SetOutputHierarchy([hex_hierarchy.P[1]], w)
    fs.close()
    smp.close()


def _write_problem(path, prob):
    """tests/c/kl_io.h layout with no realizations (nbatch 0)"""
    import scipy.sparse as sps
    with open(path, "wb") as f:
        np.array([0x4b4c3031, len(prob.levels), prob.nmodes, 1 if prob.lognormal else 0, 0], np.int32).tofile(f)
        for L in prob.levels:
            np.array([L.n_s], np.int32).tofile(f)
            L.w_diag.astype(np.float64).tofile(f)
            np.array([0 if L.P is None else 1], np.int32).tofile(f)
            if L.P is not None:
                P = sps.csr_matrix(L.P)
                np.array([P.shape[0], P.shape[1], P.nnz], np.int32).tofile(f)
                P.indptr.astype(np.int32).tofile(f)
                P.indices.astype(np.int32).tofile(f)
                P.data.astype(np.float64).tofile(f)
        prob.evals.astype(np.float64).tofile(f)
        np.asfortranarray(prob.evect0).ravel(order="F").astype(np.float64).tofile(f)


def test_c_and_cpp_callers_print_the_python_table(hex_hierarchy, tmp_path):
    """tests/c/field_stats_smoke.c (plain C ABI) and tests/c/field_stats_adapter_smoke.cpp (MFEM adapter + parelagmc.hpp
    mirror, host and device vectors) print PDESamplerTest's table for a KL sampler; it must equal the Python path's."""
    import os
    import subprocess
    from conftest import ROOT
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_kl_sampler_problem, chi_center_of_mass, restrict_chi
    r = subprocess.run(["make", "-C", ROOT, "test-field-stats"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    prob = build_kl_sampler_problem(hex_hierarchy, "analytic", corlen=0.1)
    path = str(tmp_path / "kl.bin")
    _write_problem(path, prob)
    seed, N, exact_e, exact_v = 11, 300, 0.0, 1.0
    chi0 = chi_center_of_mass(hex_hierarchy.spaces[0])
    ichi = int(np.argmax(chi0))
    ctx = capi.Context(0, seed=seed)
    smp = capi.KLSampler(ctx, prob)
    chis = restrict_chi(chi0, hex_hierarchy.P)
    want = []
    for lvl in range(smp.nlevels):
        fs = capi.FieldStatistics(smp, lvl, chis[lvl]).run(0, N)
        e, m2, cc, cnt = fs.read()
        want.append((lvl, cnt, smp.ComputeL2Error(lvl, e, exact_e), smp.ComputeL2Error(lvl, m2, exact_v),
                     smp.ComputeMaxError(lvl, e, exact_e), cc[int(np.argmax(chis[lvl]))]))
        fs.close()
    smp.close()
    ctx.close()
    for exe in ("field_stats_smoke", "field_stats_adapter_smoke"):
        r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", exe), path, str(seed), str(ichi), str(N), repr(exact_e),
                            repr(exact_v)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith(f"{exe} OK"), r.stdout + r.stderr
        rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("level ")]
        got = [(int(t[1].rstrip(":")), int(t[3]), float(t[5]), float(t[7]), float(t[9]), float(t[11])) for t in rows]
        print(exe, got)
        assert got == want, (exe, got, want)


def test_stats_refuse_a_level_whose_sample_size_changed(gpu_ctx, hex_hierarchy):
    """the accumulators are sized at create: after pmc_sampler_set_projection changes sample_size(level) they refuse"""
    from parelagmc_amd import capi
    smp, _ = _make(gpu_ctx, "gather", hex_hierarchy)
    fs = capi.FieldStatistics(smp, 1)
    fs.run(0, 3)
    n_s = smp.xi_size(1)
    assert n_s != smp.SampleSize(1)
    assert gpu_ctx.lib.pmc_sampler_set_projection(smp.h, 1, capi.PMC_PROJ_NONE, None, None, None, 0) == 0
    assert smp.SampleSize(1) == n_s
    for call in (lambda: fs.run(0, 3), lambda: fs.accumulate(np.zeros((1, n_s))), lambda: fs.read()):
        with pytest.raises(capi.PmcError) as e:
            call()
        assert e.value.code == -1
    fs.close()
    smp.close()

"""Field statistics timing (pmc_field_stats_*, csrc/field_stats.hip) on BASELINE config 2: PDESampler on cube_tet refined
5 x, level 0 (n_s = 196 608), hybridized solver (bench.py's headline solver), launches of 64 realizations.

(a) one pmc_field_stats_accumulate of 64 device-resident realizations with chi (the <chi, s_c> pass + the compensated
    accumulate): device milliseconds (HIP events around `--reps` calls) and the algorithmic bandwidth,
    bytes = 8 n nb (s, dot pass) + 8 n (chi) + 8 n nb (s, accumulate) + 2 x 6 x 8 n (accumulators read + written);
(b) pmc_field_stats_run(0, N) against a bare device Sample + Eval loop of the same N in launches of 64 (wall clock after a
    synchronisation, alternating, best of `--trials`);
(c) the host path the tests used before: Sample + Eval into device memory, download, numpy sums of s, s^2, <chi, s> s.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refine", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--launches", type=int, default=16, help="launches of (b) and (c)")
    ap.add_argument("--trials", type=int, default=3)
    a = ap.parse_args()
    from bench import build_hybrid_problem
    from parelagmc_amd import capi
    from parelagmc_amd.fe import chi_center_of_mass, mesh_from_json, build_hierarchy
    prob = build_hybrid_problem(a.refine)
    ctx = capi.Context(0, seed=1)
    smp = capi.PDESampler(ctx, prob)
    lib = ctx.lib
    W = smp.BatchWidth(0)
    n, n_xi = smp.SampleSize(0), smp.xi_size(0)
    h = build_hierarchy(mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json")), a.refine)
    chi = chi_center_of_mass(h.spaces[0])
    assert chi.size == n
    res = {"workload": f"PDESampler (hybridized) cube_tet r={a.refine}, level 0, n_s={n}, launch width {W}",
           "hbm_tbs_assumed": HBM_TBS}
    # (a)
    xi, s = ctx.empty(W * n_xi), ctx.empty(W * n)
    smp.Sample(0, first_id=0, nbatch=W, out=xi)
    smp.Eval(0, xi, xi_level=0, s_out=s)
    fs = capi.FieldStatistics(smp, 0, chi)
    for _ in range(3):
        fs.accumulate(s, nbatch=W)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.reps):
        fs.accumulate(s, nbatch=W)
    ms = ctx.timer_stop() / a.reps
    byts = 8.0 * n * W + 8.0 * n + 8.0 * n * W + 2 * 6 * 8.0 * n
    res["accumulate"] = {"nb": W, "ms": ms, "bytes": byts, "tbs": byts / (ms * 1e-3) / 1e12,
                         "frac_of_hbm": byts / (ms * 1e-3) / 1e12 / HBM_TBS}
    # (b)
    N = a.launches * W

    def bare():
        for t in range(a.launches):
            smp.Sample(0, first_id=t * W, nbatch=W, out=xi)
            smp.Eval(0, xi, xi_level=0, s_out=s)
        ctx.synchronize()

    def run():
        fs.reset()
        fs.run(0, N)
        ctx.synchronize()

    bare()
    run()
    tb, tr = [], []
    for _ in range(a.trials):
        t0 = time.perf_counter()
        bare()
        tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        run()
        tr.append(time.perf_counter() - t0)
    res["run"] = {"nsamples": N, "bare_sample_eval_s": min(tb), "run_s": min(tr), "overhead": min(tr) / min(tb) - 1.0,
                  "bare_trials_s": tb, "run_trials_s": tr}
    # (c)
    acc = [np.zeros(n), np.zeros(n), np.zeros(n)]
    t0 = time.perf_counter()
    thost = 0.0
    for t in range(a.launches):
        smp.Sample(0, first_id=t * W, nbatch=W, out=xi)
        smp.Eval(0, xi, xi_level=0, s_out=s)
        ctx.synchronize()
        t1 = time.perf_counter()
        x = s.download().reshape(W, n)
        acc[0] += x.sum(axis=0)
        acc[1] += (x * x).sum(axis=0)
        acc[2] += (x @ chi) @ x
        thost += time.perf_counter() - t1
    res["host_path"] = {"nsamples": N, "total_s": time.perf_counter() - t0, "download_and_numpy_s": thost,
                        "per_launch_ms": thost / a.launches * 1e3}
    e, m2, cc, cnt = fs.read()
    res["host_vs_device_max_rel"] = float(max(np.abs(e - acc[0] / N).max() / np.abs(acc[0] / N).max(),
                                              np.abs(m2 - acc[1] / N).max() / np.abs(acc[1] / N).max()))
    fs.close()
    xi.free()
    s.free()
    smp.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

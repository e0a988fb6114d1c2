"""Posterior field statistics timing (pmc_ratio_enable_field_stats, csrc/level_fields.hip) on BASELINE config 3: the ratio
manager with the SPDE sampler and the Darcy solver on cube_hex 64^3 / 32^3 / 16^3, two observation functionals from
oracle.bayes_oracle, batch 256, InitRun [64, 256, 1024].

(a) one pmc_level_fields_accumulate_weighted of `--nb` device-resident fields of level 0 (n_p = 262 144) with their level-1
    partners and host weights: device milliseconds (HIP events around `--reps` calls) and the algorithmic bandwidth,
    bytes = 8 n nb (fine columns) + 8 n_c nb (coarse columns, each entry counted once) + 4 n (parent map)
            + 2 x 6 x 8 n (the six accumulators read and written);
(b) InitRun with fixed counts on two managers over the same handles, the feature off and on, alternating, best of
    `--trials`: wall seconds, realizations/s and the overhead.  The ratio managers have no Reset entry, so every trial
    adds realizations after the previous ones (the same counts, later ids, for both managers).
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
IC_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=16, help="realizations per accumulate in (a): level 0's launch width")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261003)
    a = ap.parse_args()
    from oracle.bayes_oracle import observation_functionals
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy, build_sampler_problem
    h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 4)       # bench.build_config3's hierarchy
    sp = build_sampler_problem(h, corlen=0.1, lognormal=True, n_mc_levels=3)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=3)
    ctx = capi.Context(0, seed=a.seed)
    smp, ds = capi.PDESampler(ctx, sp), capi.DarcySolver(ctx, dp)
    lib = ctx.lib
    n, nc = dp.levels[0].n_p, dp.levels[1].n_p
    res = {"workload": "config 3: cube_hex 64^3/32^3/16^3, ratio manager, 2 observations, batch 256, "
                       "InitRun [64, 256, 1024]", "hbm_tbs_assumed": HBM_TBS}
    # (a)
    f = capi.LevelFields(ctx, ds, 0, True)
    rng = np.random.default_rng(1)
    pf, pc = ctx.empty(a.nb * n), ctx.empty(a.nb * nc)
    pf.upload(rng.standard_normal(a.nb * n))
    pc.upload(rng.standard_normal(a.nb * nc))
    wf, wc = rng.random(a.nb), rng.random(a.nb)

    def acc():
        rc = lib.pmc_level_fields_accumulate_weighted(f.h, a.nb, pf.ptr, wf.ctypes.data, pc.ptr, wc.ctypes.data,
                                                      capi.PMC_MEM_DEVICE)
        assert rc == 0, lib.pmc_last_error()
    for _ in range(3):
        acc()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.reps):
        acc()
    ms = ctx.timer_stop() / a.reps
    byts = 8.0 * n * a.nb + 8.0 * nc * a.nb + 4.0 * n + 2 * 6 * 8.0 * n
    ws = 8.0 * n * a.nb + 8.0 * nc * a.nb + 4.0 * n + 6 * 8.0 * n
    res["accumulate_weighted"] = {"n": n, "n_coarse": nc, "nb": a.nb, "ms": ms, "bytes": byts,
                                  "tbs": byts / (ms * 1e-3) / 1e12, "frac_of_hbm": byts / (ms * 1e-3) / 1e12 / HBM_TBS,
                                  "working_set_bytes": ws, "fits_infinity_cache": ws < IC_BYTES}
    f.close()
    pf.free()
    pc.free()
    # (b)
    Gobs = observation_functionals(h, np.array([[0.5, 0.5, 0.5], [1.4, 1.2, 0.6]]), eps=0.3)
    for lvl in range(3):
        ds.SetObservations(lvl, Gobs[lvl])
    # synthetic data: G of one prior draw on level 0 (ids far from the managers' ranges)
    G_obs = ds.ComputeG(0, smp.Eval(0, smp.Sample(0, first_id=1 << 40, nbatch=1), xi_level=0))[0][0]
    ns = [64, 256, 1024]
    mgrs = {}
    for on in (False, True):
        m = host_api.RatioManager(3, sampler=smp, solver=ds, G_obs=G_obs, noise=0.05, wall_time=False, batch=256)
        if on:
            m.enable_field_stats(sp.levels[0].w_diag)       # the level-0 P0 mass
        m.InitRun(ns)                                  # warm-up: allocations at the widths of the timed rounds
        mgrs[on] = m
    t = {False: [], True: []}
    sums = {}
    for _ in range(a.trials):
        for on in (False, True):
            t0 = time.perf_counter()
            r = mgrs[on].InitRun(ns)
            t[on].append(time.perf_counter() - t0)
            sums[on] = r["sums"]
    tot = float(sum(ns))
    res["init_run"] = {"nsamples": ns, "off_s": min(t[False]), "on_s": min(t[True]),
                       "off_realizations_per_s": tot / min(t[False]), "on_realizations_per_s": tot / min(t[True]),
                       "overhead": min(t[True]) / min(t[False]) - 1.0, "off_trials_s": t[False], "on_trials_s": t[True],
                       "sums_equal": bool(np.array_equal(sums[True], sums[False]))}
    pm = mgrs[True].field_stats()
    res["maps"] = {"Z_estimate": r["Z_estimate"], "l2_mean_corr": pm["l2_mean_corr"].tolist(),
                   "int_var_corr": pm["int_var_corr"].tolist()}
    for m in mgrs.values():
        m.close()
    ds.close()
    smp.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

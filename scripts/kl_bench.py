"""KL sampler launch timing (pmc_sampler_create_kl, csrc/kl.hip) on the example_parameters.xml workload: hex 32^3 on [0,2]^3
(32 768 elements), AnalyticExponentialCovariance 10 x 10 x 10 = 1000 modes, corlen 0.1, 2 Monte Carlo levels.

Per launch width NB in (1, 64, 256): device milliseconds per Eval on level 0 (HIP events around `--reps` back-to-back
launches, device buffers, no stats), the algorithmic bytes 8 n m + 8 n NB + 8 m NB and flops 2 n m NB computed from the
shapes, and the achieved rates.  The fp64 MFMA rate the roofline uses is measured by scripts/lab/f64_mfma_rate.hip
(compiled here with hipcc).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def f64_rate():
    src = os.path.join(ROOT, "scripts", "lab", "f64_mfma_rate.hip")
    exe = os.path.join(ROOT, "build", "f64_mfma_rate")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-o", exe, src], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    return float(out[out.index("f64_mfma_tflops") + 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--widths", default="1,64,256")
    ap.add_argument("--no-rate", action="store_true", help="skip the f64 MFMA micro-benchmark")
    a = ap.parse_args()
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_kl_sampler_problem
    h = build_hierarchy(box_mesh([8, 8, 8], [2, 2, 2], "hex"), 2)
    prob = build_kl_sampler_problem(h, "analytic", nmodes=[10, 10, 10], domain_lengths=[2, 2, 2], corlen=0.1)
    n, m = prob.levels[0].n_s, prob.nmodes
    rate = None if a.no_rate else f64_rate()
    ctx = capi.Context(0, seed=1)
    smp = capi.KLSampler(ctx, prob)
    lib = ctx.lib
    res = {"workload": f"KLSampler analytic hex 32^3 n={n} m={m}, {prob.n_mc_levels} MC levels, level 0",
           "f64_mfma_tflops_measured": rate, "hbm_tbs_assumed": HBM_TBS, "launches": []}
    for nb in [int(x) for x in a.widths.split(",")]:
        xi = ctx.empty(nb * n)
        s = ctx.empty(nb * n)
        smp.Sample(0, first_id=0, nbatch=nb, out=xi)

        def launch():
            capi._check(lib.pmc_sampler_eval(smp.h, 0, 0, nb, xi.ptr, s.ptr, None, -1, 0, None, capi.PMC_MEM_DEVICE, None))
        for _ in range(3):
            launch()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(a.reps):
            launch()
        ms = ctx.timer_stop() / a.reps
        byts = 8.0 * n * m + 8.0 * n * nb + 8.0 * m * nb
        flops = 2.0 * n * m * nb
        t_mem = byts / (HBM_TBS * 1e12) * 1e3
        t_f64 = flops / (rate * 1e12) * 1e3 if rate else None
        bound = max(t_mem, t_f64) if t_f64 else t_mem
        res["launches"].append({"nb": nb, "ms": ms, "bytes": byts, "flops": flops, "tbs": byts / (ms * 1e-3) / 1e12,
                                "tflops": flops / (ms * 1e-3) / 1e12, "roofline_ms": bound, "ms_over_roofline": ms / bound,
                                "frac_of_hbm": (byts / (ms * 1e-3) / 1e12) / HBM_TBS})
        xi.free()
        s.free()
    smp.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

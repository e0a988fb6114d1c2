#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 17 (the adjoint of the samplers' Eval):

  * SPDE samplers at the size of BASELINE config 2 (cube_tet refined --refine times, one Monte Carlo level, default solver
    options): milliseconds per realization of EvalAdjoint beside Eval of the same handle on one launch width in device
    memory, for the saddle-point and the hybridized solver - host clock around calls that end in a stream synchronise,
    alternated, best of --reps - and the iteration counts of both solves;
  * KL handles on the scripts/kl_bench.py workload (hex 32^3, n = 32 768, m = 1000): device milliseconds per launch of the
    adjoint (kl_adjoint_mfma_kernel / kl_adjoint_gemv_kernel + the reduction of the partials) beside the forward launch
    (kl_mfma_kernel / kl_gemv_kernel) at nb = 1, 64, 256 - HIP events around --launches back-to-back launches, alternated,
    best of --reps - with the algorithmic bytes 8 n m + 8 n nb + 8 m nb (+ the partials written and read once).
Prints one JSON line per measurement and writes them to --out (default profiles/sampler_adjoint_bench.json).  Nothing is
asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pde(kind, refine, reps, small):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import (box_mesh, build_hierarchy, build_hybrid_sampler_problem, build_sampler_problem,
                                  mesh_from_json)
    if small:
        h = build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1)
    else:
        h = build_hierarchy(mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json")), refine)
    if kind == "hybrid":
        prob = build_hybrid_sampler_problem(h, corlen=0.1, n_mc_levels=1, builder=capi.library_hybrid_builder)
    else:
        prob = build_sampler_problem(h, corlen=0.1, n_mc_levels=1)
    ctx = capi.Context(0, seed=5)
    smp = capi.PDESampler(ctx, prob)
    nb = smp.BatchWidth(0)
    n = smp.xi_size(0)
    xi, s, g = ctx.empty(nb * n), ctx.empty(nb * n), ctx.empty(nb * n)
    smp.Sample(0, first_id=0, nbatch=nb, out=xi)
    v = ctx.array(np.random.default_rng(7).standard_normal((nb, n)))

    def fwd():
        return smp.Eval(0, xi, xi_level=0, s_out=s, return_stats=True)[-1]

    def adj():
        return smp.EvalAdjoint(0, v, grad_out=g, nbatch=nb, return_stats=True)[-1]

    fwd()
    adj()                                        # warm-up: code objects, buffers, the level's adjoint data
    best = {"fwd": float("inf"), "adj": float("inf")}
    st = {}
    for _ in range(reps):
        for what, fn in (("fwd", fwd), ("adj", adj)):
            ctx.synchronize()
            t0 = time.perf_counter()
            st[what] = fn()
            ctx.synchronize()
            best[what] = min(best[what], (time.perf_counter() - t0) * 1e3)
    rec = dict(what="pde", solver=kind, n_s=n, n_u=prob.levels[0].n_lambda if kind == "hybrid" else prob.levels[0].n_u, nb=nb,
               eval_ms_per_realization=best["fwd"] / nb, eval_adjoint_ms_per_realization=best["adj"] / nb,
               ratio=best["adj"] / best["fwd"], iterations_fwd=max(t[0] for t in st["fwd"]),
               iterations_adj=max(t[0] for t in st["adj"]))
    for a in (xi, s, g, v):
        a.free()
    smp.close()
    ctx.close()
    return rec


def kl(widths, reps, launches, small):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_kl_sampler_problem
    if small:
        h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 1)
        prob = build_kl_sampler_problem(h, "analytic", nmodes=[3, 3, 3], domain_lengths=[2, 2, 2], corlen=0.1)
    else:
        h = build_hierarchy(box_mesh([8, 8, 8], [2, 2, 2], "hex"), 2)
        prob = build_kl_sampler_problem(h, "analytic", nmodes=[10, 10, 10], domain_lengths=[2, 2, 2], corlen=0.1)
    n, m = prob.levels[0].n_s, prob.nmodes
    ctx = capi.Context(0, seed=1)
    smp = capi.KLSampler(ctx, prob)
    lib = ctx.lib
    chunk_rows = max(1024, -(-(-(-n // 32)) // 32) * 32)       # adjoint_chunk_rows of csrc/kl_adjoint.hip
    nchunks = -(-n // chunk_rows)
    recs = []
    for nb in widths:
        xi, s, g = ctx.empty(nb * n), ctx.empty(nb * n), ctx.empty(nb * n)
        smp.Sample(0, first_id=0, nbatch=nb, out=xi)

        def fwd():
            capi._check(lib.pmc_sampler_eval(smp.h, 0, 0, nb, xi.ptr, s.ptr, None, -1, 0, None, capi.PMC_MEM_DEVICE, None))

        def adj():
            capi._check(lib.pmc_sampler_eval_adjoint(smp.h, 0, 0, nb, s.ptr, None, g.ptr, capi.PMC_MEM_DEVICE, None))

        for fn in (fwd, adj, fwd, adj):
            fn()
        best = {"fwd": float("inf"), "adj": float("inf")}
        for _ in range(reps):
            for what, fn in (("fwd", fwd), ("adj", adj)):
                ctx.synchronize()
                ctx.timer_start()
                for _ in range(launches):
                    fn()
                best[what] = min(best[what], ctx.timer_stop() / launches)
        byts = 8.0 * n * m + 8.0 * n * nb + 8.0 * m * nb
        part = 2 * 8.0 * nchunks * min(nb, 256) * m * -(-nb // 256)
        recs.append(dict(what="kl", n=n, m=m, nb=nb, chunks=nchunks, forward_ms=best["fwd"], adjoint_ms=best["adj"],
                         ratio=best["adj"] / best["fwd"], bytes=byts, partial_bytes=part,
                         forward_tbs=byts / (best["fwd"] * 1e-3) / 1e12, adjoint_tbs=(byts + part) / (best["adj"] * 1e-3) / 1e12,
                         adjoint_tflops=2.0 * n * m * nb / (best["adj"] * 1e-3) / 1e12))
        for a in (xi, s, g):
            a.free()
    smp.close()
    ctx.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--refine", type=int, default=5, help="uniform refinements of cube_tet (5: BASELINE config 2)")
    ap.add_argument("--widths", default="1,64,256")
    ap.add_argument("--parts", default="kl,saddle,hybrid")
    ap.add_argument("--small", action="store_true", help="tiny meshes instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_adjoint_bench.json"))
    args = ap.parse_args()
    recs = []
    for part in args.parts.split(","):
        new = kl([int(x) for x in args.widths.split(",")], args.reps, args.launches, args.small) if part == "kl" else \
            [pde(part, args.refine, args.reps, args.small)]
        for r in new:
            print(json.dumps(r), flush=True)
        recs += new
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

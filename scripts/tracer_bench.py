#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 20 (particle travel times on the Darcy flux), on the finest level of hex 64^3 and of
cube_tet refined five times, default solver options, lognormal draws k = exp(N(0, 1)), 1024 particles released 1e-3 under the
inflow face, nb = 16 and 64 realizations:

  * pmc_tracer_run on the flux block of the solutions of those draws in device memory (the sample-major layout: lanes along
    particles): HIP events on the context's stream around the call, best of --reps; elements crossed per second;
  * the walk on the solver's interleaved solution (lanes along realizations) runs inside the hooked SolveFwd only; it is
    reported as the difference of the hooked solve to the unhooked solve that maintains the full solution (sol_out given),
    both on the same draws: host clock around calls that end in a stream synchronise, alternated, best of --reps.  The
    unhooked solve without sol_out (compact solution rows, what the managers ran before) is timed beside them.
Prints one JSON line per mesh and batch; --out also writes them to a JSON file.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hierarchy(name, small):
    """(hierarchy, axis of the flow, obs / inflow attributes set on that axis)"""
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if small:
        return build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1), 2
    if name == "hex64":
        return build_hierarchy(box_mesh([16, 16, 16], [1, 1, 1], "hex"), 2), 2
    m = mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json"))
    cen = m.verts[m.bdr].mean(axis=1)
    lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
    m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1, np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
    return build_hierarchy(m, 5), 0


def measure(name, nbs, nparticles, reps, small):
    import ctypes as C
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_darcy_problem
    from parelagmc_amd.fe import tracer as tr
    h, axis = hierarchy(name, small)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    L, space = dp.levels[0], h.spaces[0]
    rng = np.random.default_rng(7)
    lo, hi = space.mesh.verts.min(axis=0), space.mesh.verts.max(axis=0)
    x0 = lo + rng.uniform(0.05, 0.95, (nparticles, 3)) * (hi - lo)
    x0[:, axis] = hi[axis] - 1e-3
    mesh = tr.tracer_mesh(space)
    t0 = time.perf_counter()
    elem0 = tr.locate(mesh, x0)
    locate_s = time.perf_counter() - t0
    ctx = capi.Context(0, seed=5)
    ds = capi.DarcySolver(ctx, dp)
    tracer = capi.Tracer(ctx, mesh, x0, elem0)
    n = L.n_u + L.n_p
    recs = []
    for nb in nbs:
        k = ctx.array(np.exp(rng.standard_normal((nb, L.n_p))))
        sol = ctx.empty(nb * n)
        ds.SolveFwd(0, k, nbatch=nb, sol_out=sol)
        out = tracer.Run(sol, nbatch=nb, ld=n)                      # warm-up; the outputs are reused below
        run_ms = float("inf")
        for _ in range(reps):
            ctx.timer_start()
            capi._check(ctx.lib.pmc_tracer_run(tracer.h, nb, sol.ptr, n, out["T"].ptr, out["exit_face"].ptr, out["status"].ptr,
                                               out["nsteps"].ptr, out["x_exit"].ptr, capi.PMC_MEM_DEVICE))
            run_ms = min(run_ms, ctx.timer_stop())
        steps = out["nsteps"].download()
        status = out["status"].download()
        T = out["T"].download()

        def plain():
            return ds.SolveFwd(0, k, nbatch=nb)

        def full():
            return ds.SolveFwd(0, k, nbatch=nb, sol_out=sol)

        def hooked():
            ds.SetTracer(0, tracer, tracer.MEAN)
            try:
                return ds.SolveFwd(0, k, nbatch=nb)
            finally:
                ds.SetTracer(0, None)

        best = {}
        for fn in (plain, full, hooked):
            fn()
        for _ in range(reps):
            for fn in (plain, full, hooked):
                ctx.synchronize()
                t0 = time.perf_counter()
                q = fn()[0]
                best[fn.__name__] = min(best.get(fn.__name__, float("inf")), (time.perf_counter() - t0) * 1e3)
        recs.append(dict(mesh="hex8(small)" if small else name, n_p=L.n_p, n_u=L.n_u, nb=nb, particles=nparticles,
                         locate_s=locate_s, not_exited=int((status != 0).sum()), steps_min=int(steps.min()),
                         steps_mean=float(steps.mean()), steps_max=int(steps.max()), T_mean=float(T.mean()),
                         tracer_run_sample_major_ms=run_ms, steps_per_second=float(steps.sum()) / (run_ms * 1e-3),
                         solve_fwd_compact_ms=best["plain"], solve_fwd_full_solution_ms=best["full"],
                         solve_fwd_hooked_ms=best["hooked"], hooked_minus_full_ms=best["hooked"] - best["full"],
                         hooked_over_compact=best["hooked"] / best["plain"], Q_hooked_mean=float(np.mean(q))))
        print(json.dumps(recs[-1]), flush=True)
        for a in [k, sol] + list(out.values()):
            a.free()
    tracer.close()
    ds.close()
    ctx.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--meshes", default="hex64,tet5")
    ap.add_argument("--nb", default="16,64")
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--small", action="store_true", help="an 8^3 mesh instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out")
    args = ap.parse_args()
    recs = []
    for name in args.meshes.split(","):
        recs += measure(name, [int(b) for b in args.nb.split(",")], args.particles, args.reps, args.small)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

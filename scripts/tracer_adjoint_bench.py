#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 25 (the adjoint of the particle tracer), on the shapes of section 20's table: the
finest level of hex 64^3 and of cube_tet refined five times, default solver options, k = exp(N(0, 1)), 1024 particles released
1e-3 under the inflow face, nb = 16 and 64 realizations, device memory:

  * pmc_tracer_run against pmc_tracer_run_adjoint (seed T_bar = 1 / nparticles) on the flux block of the solutions of those
    draws: HIP events on the context's stream around the call, best of --reps.  The adjoint call holds a plain walk, a
    copy of the step counts to the host, a walk with history, the sweep and the assembly;
  * pmc_darcy_tracer_gradient against pmc_darcy_solve_gradient given the adjoint right-hand side [u_bar; 0] of the same
    draws: host clock around calls that end in a stream synchronise, alternated, best of --reps.  The difference is the
    tracer's share of the entry (on the interleaved layout);
  * one crowded case per mesh: the same number of particles released in one element (that of the first start point), so the
    lists of the first elements of the paths hold a visit of every particle.
Prints one JSON line per mesh and batch; --out also writes them to a JSON file.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tracer_bench import hierarchy  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        ctx.timer_start()
        fn()
        best = min(best, ctx.timer_stop())
    return best


def measure(name, nbs, nparticles, reps, small):
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
    elem0 = tr.locate(mesh, x0)
    # the crowded starts: every particle in the element of the first one
    e = int(elem0[0])
    if mesh.kind == tr.BOX:
        xc = mesh.geom[e, :3] + rng.uniform(0.05, 0.95, (nparticles, 3)) * (mesh.geom[e, 3:] - mesh.geom[e, :3])
    else:
        lam = rng.dirichlet(np.ones(4), nparticles) * 0.8 + 0.05
        xc = lam @ mesh.geom[e]
    ctx = capi.Context(0, seed=5)
    ds = capi.DarcySolver(ctx, dp)
    tracers = dict(spread=capi.Tracer(ctx, mesh, x0, elem0), crowded=capi.Tracer(ctx, mesh, xc, np.full(nparticles, e, np.int32)))
    n = L.n_u + L.n_p
    recs = []
    for nb in nbs:
        k = ctx.array(np.exp(rng.standard_normal((nb, L.n_p))))
        sol, grad = ctx.empty(nb * n), ctx.empty(nb * L.n_p)
        ds.SolveFwd(0, k, nbatch=nb, sol_out=sol)
        Tb = ctx.array(np.full((nb, nparticles), 1.0 / nparticles))
        for layout, t in tracers.items():
            out = t.Run(sol, nbatch=nb, ld=n, want_x=False)
            adj = t.run_adjoint(sol, T_bar=Tb, nbatch=nb, ld=n, ld_bar=n)
            ubar = adj["u_bar"]                                     # [u_bar; untouched p rows]: the p rows must be zero
            rhs = np.zeros((nb, n))
            rhs[:, :L.n_u] = ubar.download().reshape(nb, n)[:, :L.n_u]
            ubar.upload(rhs)
            addr = lambda a: a.ptr
            run_ms = timed(ctx, lambda: capi._check(ctx.lib.pmc_tracer_run(
                t.h, nb, sol.ptr, n, addr(out["T"]), addr(out["exit_face"]), addr(out["status"]), addr(out["nsteps"]), None,
                capi.PMC_MEM_DEVICE)), reps)
            scratch = ctx.empty(nb * n)
            adj_ms = timed(ctx, lambda: capi._check(ctx.lib.pmc_tracer_run_adjoint(
                t.h, nb, sol.ptr, n, Tb.ptr, None, scratch.ptr, n, addr(adj["x0_bar"]), addr(adj["T"]), addr(adj["exit_face"]),
                addr(adj["status"]), addr(adj["nsteps"]), capi.PMC_MEM_DEVICE)), reps)
            chunks = t.adjoint_chunks()
            steps, status = out["nsteps"].download(), out["status"].download()

            def entry():
                return ds.tracer_gradient(0, t, k, Tb, nbatch=nb, grad_out=grad)

            def pieces():
                return ds.solve_gradient(0, k, ubar, nbatch=nb, grad_out=grad)

            best = {}
            for fn in (entry, pieces):
                fn()
            for _ in range(reps):
                for fn in (entry, pieces):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    best[fn.__name__] = min(best.get(fn.__name__, float("inf")), (time.perf_counter() - t0) * 1e3)
            recs.append(dict(mesh="hex8(small)" if small else name, starts=layout, n_p=L.n_p, n_u=L.n_u, nb=nb,
                             particles=nparticles, not_exited=int((status != 0).sum()), steps_mean=float(steps.mean()),
                             steps_max=int(steps.max()), tracer_run_ms=run_ms, tracer_run_adjoint_ms=adj_ms,
                             adjoint_over_run=adj_ms / run_ms, adjoint_chunks=chunks,
                             visits_per_second=float(steps.sum()) / (adj_ms * 1e-3), darcy_tracer_gradient_ms=best["entry"],
                             darcy_solve_gradient_given_rhs_ms=best["pieces"], entry_minus_pieces_ms=best["entry"] - best["pieces"]))
            print(json.dumps(recs[-1]), flush=True)
            for a in list(out.values()) + list(adj.values()) + [scratch]:
                a.free()
        for a in (k, sol, grad, Tb):
            a.free()
    for t in tracers.values():
        t.close()
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

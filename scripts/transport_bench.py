#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 21 (upwind solute transport on the Darcy flux), on the finest level of hex 64^3 and of
cube_tet refined five times, default solver options, lognormal draws k = exp(N(0, 1)), nb = 16 and 64 realizations, porosity
0.3, cfl 0.9, 16 report times, t_end = one pore volume at the median throughput of the draws:

  * pmc_transport_run on the flux block of the solutions of those draws in device memory (the sample-major layout): HIP events
    on the context's stream around the call after a warm-up, best of --reps; steps per column (min / median / max); the time
    per step launch (the call runs as many step launches as its longest column has steps); the bytes of the step launches
    computed from the shapes - per active (column, step) the concentrations read and written (16 B per element) and the flux
    (8 B per dof), per launch the row records (8 B per row entry) and the pore volumes (8 B per element); gathers of the
    neighbours' concentrations are re-reads of those lines and not counted - and the rate they were moved at beside the
    5.6 TB/s the flat vector kernels of the library reach;
  * the hooked SolveFwd (the transport on the solver's interleaved solution) against the unhooked one with and without the full
    solution, on the same draws: host clock around calls that end in a stream synchronise, alternated, best of --reps.
Prints one JSON line per mesh and batch; --out also writes them to a JSON file.  Nothing is asserted; what a run did not
measure is recorded under "not_measured"."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLAT_VECTOR_BYTES_PER_S = 5.6e12
NOT_MEASURED = ["hardware counters of the step kernel (HBM bytes, L2 hit rate of the neighbour gathers)",
                "the general (ragged-row) form at benchmark size: both meshes take a register form (6 and 4 entries per row)",
                "host-memory callers (staging copies included)"]


def hierarchy(name, small):
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if small:
        return build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1)
    if name == "hex64":
        return build_hierarchy(box_mesh([16, 16, 16], [1, 1, 1], "hex"), 2)
    m = mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json"))
    cen = m.verts[m.bdr].mean(axis=1)
    lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
    m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1, np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
    return build_hierarchy(m, 5)


def measure(name, nbs, reps, small):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_darcy_problem
    from parelagmc_amd.fe import transport as tw
    h = hierarchy(name, small)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    L, space = dp.levels[0], h.spaces[0]
    mesh = tw.transport_mesh(L, space.vol, 0.3)
    width = int(np.diff(mesh.rowptr).max())
    rng = np.random.default_rng(7)
    ctx = capi.Context(0, seed=5)
    ds = capi.DarcySolver(ctx, dp)
    n = L.n_u + L.n_p
    recs = []
    for nb in nbs:
        k = ctx.array(np.exp(rng.standard_normal((nb, L.n_p))))
        sol = ctx.empty(nb * n)
        ds.SolveFwd(0, k, nbatch=nb, sol_out=sol)
        flux = sol.download().reshape(nb, n)[:8, :L.n_u]
        t_end = float(mesh.pore_volume.sum() / np.median(tw.inflow_mass_rate(mesh, flux)))
        tp = capi.Transport(ctx, mesh, t_end, 0.9, 16)
        out = tp.Run(sol, nbatch=nb, ld=n)                           # warm-up; the outputs are reused below
        run_ms = float("inf")
        for _ in range(reps):
            ctx.timer_start()
            capi._check(ctx.lib.pmc_transport_run(tp.h, nb, sol.ptr, n, out["c"].ptr, out["curve"].ptr, out["stored"].ptr,
                                                  out["rate"].ptr, out["t_reached"].ptr, out["nsteps"].ptr, out["status"].ptr,
                                                  capi.PMC_MEM_DEVICE))
            run_ms = min(run_ms, ctx.timer_stop())
        steps = out["nsteps"].download()
        status = out["status"].download()
        curve = out["curve"].download().reshape(nb, 16)
        launches = int(steps.max())
        step_bytes = float(steps.sum()) * (16.0 * L.n_p + 8.0 * L.n_u) + launches * (8.0 * len(mesh.col) + 8.0 * L.n_p)

        def plain():
            return ds.SolveFwd(0, k, nbatch=nb)

        def full():
            return ds.SolveFwd(0, k, nbatch=nb, sol_out=sol)

        def hooked():
            ds.SetTransport(0, tp, tp.MASS_OUT)
            try:
                return ds.SolveFwd(0, k, nbatch=nb)
            finally:
                ds.SetTransport(0, None)

        best = {}
        for fn in (plain, full, hooked):
            fn()
        for _ in range(reps):
            for fn in (plain, full, hooked):
                ctx.synchronize()
                t0 = time.perf_counter()
                q = fn()[0]
                best[fn.__name__] = min(best.get(fn.__name__, float("inf")), (time.perf_counter() - t0) * 1e3)
        recs.append(dict(mesh="hex8(small)" if small else name, n_p=L.n_p, n_u=L.n_u, row_entries=width, nb=nb, t_end=t_end,
                         n_outlet=tp.n_outlet, status_not_ok=int((status != 0).sum()), steps_min=int(steps.min()),
                         steps_median=float(np.median(steps)), steps_max=launches, transport_run_ms=run_ms,
                         ms_per_step_launch=run_ms / launches, step_bytes_total=step_bytes,
                         step_bytes_per_launch_all_columns=nb * (16.0 * L.n_p + 8.0 * L.n_u) + 8.0 * len(mesh.col) + 8.0 * L.n_p,
                         achieved_bytes_per_s=step_bytes / (run_ms * 1e-3), flat_vector_bytes_per_s=FLAT_VECTOR_BYTES_PER_S,
                         mass_out_over_pore_volume_mean=float(curve[:, -1].mean() / mesh.pore_volume.sum()),
                         solve_fwd_compact_ms=best["plain"], solve_fwd_full_solution_ms=best["full"],
                         solve_fwd_hooked_ms=best["hooked"], hooked_minus_full_ms=best["hooked"] - best["full"],
                         hooked_over_compact=best["hooked"] / best["plain"], Q_hooked_mean=float(np.mean(q)),
                         not_measured=NOT_MEASURED))
        print(json.dumps(recs[-1]), flush=True)
        tp.close()
        for a in [k, sol] + list(out.values()):
            a.free()
    ds.close()
    ctx.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--meshes", default="hex64,tet5")
    ap.add_argument("--nb", default="16,64")
    ap.add_argument("--small", action="store_true", help="an 8^3 mesh instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out")
    args = ap.parse_args()
    recs = []
    for name in args.meshes.split(","):
        recs += measure(name, [int(b) for b in args.nb.split(",")], args.reps, args.small)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 23 (the adjoint of the solute transport), at the four shapes of section 21's table: the
finest level of hex 64^3 and of cube_tet refined five times, default solver options, lognormal draws k = exp(N(0, 1)), nb = 16
and 64 realizations, porosity 0.3, cfl 0.9, 16 report times, t_end = one pore volume at the median throughput of the draws:

  * pmc_transport_run_adjoint (seeds on the curve and on stored) against pmc_transport_run on the flux block of the solutions
    of those draws in device memory (the sample-major layout): HIP events on the context's stream around the call after a
    warm-up, best of --reps.  An adjoint call issues N step launches of the checkpointed forward pass, N - N / K of the
    recomputation and N of the sweep (N: the longest column's steps, K: the segment, which the script sets with
    pmc_transport_set_adjoint_segment to ceil(sqrt(N)), the library's default); the time of a sweep launch is not measured
    but estimated as (adjoint - 2 x forward) / N, taking the forward pass and the recomputation at the price of
    pmc_transport_run;
  * the scratch the adjoint holds beyond the forward call's, from the shapes: (N / K + K - 1) states of checkpoints and segment,
    2 of the forward pair, 1 of final states, 4 of (lam, w lam), 1 of P, in units of n_elem nb doubles, X per dof, beta per step;
  * bytes from the shapes, per active (column, step): forward pass and recomputation 16 B per element and 8 B per dof each (the
    model of section 21); the sweep 48 B per element (c, lam read; P read and written; lam, w lam written) and 24 B per dof (the
    flux; X read and written by the one element that takes inflow through the dof) - 80 B per element and 40 B per dof in
    all, five times the forward call; gathers of the neighbours' c and w lam are re-reads and not counted;
  * pmc_darcy_transport_gradient against pmc_darcy_solve_gradient with a given adj_rhs on the same draws: host clock around
    calls that end in a stream synchronise, alternated, best of --reps.
Prints one JSON line per mesh and batch; --out also writes them to a JSON file.  Nothing is asserted; what a run did not
measure is recorded under "not_measured"."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
FLAT_VECTOR_BYTES_PER_S = 5.6e12
NOT_MEASURED = ["the sweep launch on its own (estimated from the call's time, see the script's docstring)",
                "hardware counters of the sweep kernel (HBM bytes, L2 hit rate of the gathers and of the X read-modify-writes)",
                "the general (ragged-row) form at benchmark size", "host-memory callers (staging copies included)"]


def measure(name, nbs, reps, small):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import build_darcy_problem
    from parelagmc_amd.fe import transport as tw
    from transport_bench import hierarchy
    h = hierarchy(name, small)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    L, space = dp.levels[0], h.spaces[0]
    mesh = tw.transport_mesh(L, space.vol, 0.3)
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
        cb, sb = ctx.array(rng.standard_normal((nb, 16))), ctx.array(rng.standard_normal(nb))
        fwd = tp.Run(sol, nbatch=nb, ld=n, want_c=False)
        # the segment is set here (to the library's own default rule) and not left to the library, so that the segment, the
        # checkpoint count, the scratch and the launch count reported below are those of the measured call
        N = int(fwd["nsteps"].download().max())
        K = max(1, math.ceil(math.sqrt(N)))
        tp.set_adjoint_segment(K)
        adj = tp.run_adjoint(sol, curve_bar=cb, stored_bar=sb, nbatch=nb, ld=n, ld_bar=n, want_c0_bar=False)   # warm-up
        fwd_ms = adj_ms = float("inf")
        for _ in range(reps):
            ctx.timer_start()
            capi._check(ctx.lib.pmc_transport_run(tp.h, nb, sol.ptr, n, None, fwd["curve"].ptr, fwd["stored"].ptr, fwd["rate"].ptr,
                                                  fwd["t_reached"].ptr, fwd["nsteps"].ptr, fwd["status"].ptr, capi.PMC_MEM_DEVICE))
            fwd_ms = min(fwd_ms, ctx.timer_stop())
            ctx.timer_start()
            capi._check(ctx.lib.pmc_transport_run_adjoint(tp.h, nb, sol.ptr, n, cb.ptr, sb.ptr, None, adj["u_bar"].ptr, n, None,
                                                          adj["curve"].ptr, adj["stored"].ptr, adj["nsteps"].ptr, adj["status"].ptr,
                                                          capi.PMC_MEM_DEVICE))
            adj_ms = min(adj_ms, ctx.timer_stop())
        steps, status = adj["nsteps"].download(), adj["status"].download()
        same_forward = bool(np.array_equal(adj["curve"].download(), fwd["curve"].download()))
        all_ok = bool(int(steps.max()) == N and not (status != 0).any())   # then N is also the length of the sweep
        nck = -(-N // K)                                              # states 0, K, 2 K, ... below N
        states = nck + (K - 1) + 2 + 1 + 4 + 1
        scratch = 8.0 * nb * (states * L.n_p + L.n_u) + 8.0 * nb * N
        active = float(steps.sum())
        fwd_bytes = active * (16.0 * L.n_p + 8.0 * L.n_u)
        adj_bytes = active * (80.0 * L.n_p + 40.0 * L.n_u)
        rhs = ctx.array(rng.standard_normal((nb, n)))
        grad = ctx.empty(nb * L.n_p)

        def given_rhs():
            return ds.solve_gradient(0, k, rhs, nbatch=nb, grad_out=grad)

        def transport_gradient():
            return ds.TransportGradient(0, tp, k, curve_bar=cb, stored_bar=sb, nbatch=nb, grad_out=grad)

        best = {}
        for fn in (given_rhs, transport_gradient):
            fn()
        for _ in range(reps):
            for fn in (given_rhs, transport_gradient):
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                best[fn.__name__] = min(best.get(fn.__name__, float("inf")), (time.perf_counter() - t0) * 1e3)
        recs.append(dict(mesh="hex8(small)" if small else name, n_p=L.n_p, n_u=L.n_u, nb=nb, t_end=t_end,
                         status_not_ok=int((status != 0).sum()), steps_min=int(steps.min()), steps_median=float(np.median(steps)),
                         steps_max=N, every_column_differentiated=all_ok, segment=K, checkpoints=nck, forward_outputs_equal=same_forward,
                         transport_run_ms=fwd_ms, run_adjoint_ms=adj_ms, adjoint_over_forward=adj_ms / fwd_ms,
                         step_launches_of_an_adjoint_call=3 * N - nck, ms_per_launch_forward=fwd_ms / N,
                         ms_per_launch_adjoint_mean=adj_ms / (3 * N - nck), ms_per_sweep_launch_estimated=(adj_ms - 2 * fwd_ms) / N,
                         adjoint_scratch_bytes=scratch, forward_bytes=fwd_bytes, adjoint_bytes=adj_bytes,
                         bytes_ratio_model=adj_bytes / fwd_bytes, forward_bytes_per_s=fwd_bytes / (fwd_ms * 1e-3),
                         adjoint_bytes_per_s=adj_bytes / (adj_ms * 1e-3), flat_vector_bytes_per_s=FLAT_VECTOR_BYTES_PER_S,
                         solve_gradient_given_rhs_ms=best["given_rhs"], transport_gradient_ms=best["transport_gradient"],
                         transport_gradient_minus_given_rhs_ms=best["transport_gradient"] - best["given_rhs"],
                         not_measured=NOT_MEASURED))
        print(json.dumps(recs[-1]), flush=True)
        tp.close()
        for a in [k, sol, cb, sb, rhs, grad] + list(fwd.values()) + list(adj.values()):
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

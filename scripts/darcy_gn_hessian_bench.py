#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 18 (Gauss-Newton Hessian-vector products of the Darcy log-likelihood), on the finest
level of hex 64^3 / 32^3 / 16^3 and of cube_tet refined five times, default solver options, one launch of 16 lognormal draws
k = exp(N(0, 1)) in device memory, two observation functionals, directions dk = N(0, 1):

  * milliseconds per realization of gn_hessvec with the forward solution given (tangent right-hand side + tangent solve +
    adjoint solve + gradient kernel) beside solve_gradient (forward solve + adjoint solve + gradient kernel) on the same
    draws: host clock around calls that end in a stream synchronise, alternated, best of --reps;
  * the tangent right-hand side kernel alone: HIP-event brackets around its launches inside those calls
    (pmc_darcy_set_operator_timing), its algorithmic bytes (pmc_darcy_mass_tangent_bytes) over the bracket time, beside the
    in-loop bracket of the Darcy operator's u-rows (eg_pair_spmm) of the same solves and beside the mass-sensitivity kernel.
Prints one JSON line per mesh and writes them to --out (profiles/darcy_gn_hessian_bench.json).  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOISE = 0.01


def hierarchy(name):
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if name == "hex64":
        return build_hierarchy(box_mesh([16, 16, 16], [1, 1, 1], "hex"), 2)
    m = mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json"))
    cen = m.verts[m.bdr].mean(axis=1)
    lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
    m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1, np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
    return build_hierarchy(m, 5)


def observations(h):
    """one cell, and a pair of cells weighted by their volumes"""
    vol = h.spaces[0].vol
    n = vol.size
    a, b, c = n // 3, (2 * n) // 3, (2 * n) // 3 + 1
    return sp.csr_matrix(([vol[a], vol[b], vol[c]], ([0, 1, 1], [a, b, c])), shape=(2, n))


def per_launch(ms, n, nbytes):
    return dict(us=1e3 * ms / max(n, 1), launches=n, bytes=nbytes, GBps=nbytes / (ms / max(n, 1)) * 1e-6 if ms > 0 else None)


def measure(name, reps, small, nb):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy
    h = build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1) if small else hierarchy(name)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    L = dp.levels[0]
    n = L.n_u + L.n_p
    ctx = capi.Context(0, seed=5)
    ds = capi.DarcySolver(ctx, dp)
    ds.SetObservations(0, observations(h))
    nb = min(ds.BatchWidth(0), nb)
    rng = np.random.default_rng(7)
    k = ctx.array(np.exp(rng.standard_normal((nb, L.n_p))))
    dk = ctx.array(rng.standard_normal((nb, L.n_p)))
    grad, hv, x = ctx.empty(nb * L.n_p), ctx.empty(nb * L.n_p), ctx.empty(nb * n)

    def gradient():
        return ds.solve_gradient(0, k, nbatch=nb, grad_out=grad, sol_out=x, return_stats=True)

    def hessvec():
        return ds.gn_hessvec(0, k, dk, NOISE, x_in=x, nbatch=nb, hv_out=hv, return_stats=True)

    out = {"grad": gradient(), "hess": hessvec()}      # warm-up: code objects, buffers, the level's data; x for hessvec
    best = {"grad": float("inf"), "hess": float("inf")}
    for _ in range(reps):
        for what, fn in (("grad", gradient), ("hess", hessvec)):
            ctx.synchronize()
            t0 = time.perf_counter()
            out[what] = fn()
            best[what] = min(best[what], (time.perf_counter() - t0) * 1e3)
    # kernel brackets, in a pass of their own (the timed operator launches leave the two-stream schedule)
    ds.set_operator_timing(True)
    ds.operator_time()
    ds.mass_sensitivity_time()
    ds.mass_tangent_time()
    for _ in range(reps):
        hessvec()
    op_ms, op_n, _ = ds.operator_time()
    ms_ms, ms_n, _ = ds.mass_sensitivity_time()
    mt_ms, mt_n, mt_gap = ds.mass_tangent_time()
    ds.set_operator_timing(False)
    rec = dict(mesh=name if not small else "hex8(small)", n_p=L.n_p, n_u=L.n_u, nb=nb,
               solve_gradient_ms_per_realization=best["grad"] / nb, gn_hessvec_ms_per_realization=best["hess"] / nb,
               ratio=best["hess"] / best["grad"],
               iterations_fwd=max(s[0] for s in out["grad"][-2]), iterations_grad_adj=max(s[0] for s in out["grad"][-1]),
               iterations_tangent=max(s[0] for s in out["hess"][-2]), iterations_hess_adj=max(s[0] for s in out["hess"][-1]),
               mass_tangent=per_launch(mt_ms, mt_n, ds.mass_tangent_bytes(0, nb)),
               mass_tangent_empty_bracket_us=1e3 * mt_gap / max(mt_n, 1),
               mass_sensitivity=per_launch(ms_ms, ms_n, ds.mass_sensitivity_bytes(0, nb)),
               operator=per_launch(op_ms, op_n, ds.operator_bytes(0, nb)))
    for a in (k, dk, grad, hv, x):
        a.free()
    ds.close()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nb", type=int, default=16)
    ap.add_argument("--meshes", default="hex64,tet5")
    ap.add_argument("--small", action="store_true", help="an 8^3 mesh instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "darcy_gn_hessian_bench.json"))
    args = ap.parse_args()
    recs = []
    for name in args.meshes.split(","):
        recs.append(measure(name, args.reps, args.small, args.nb))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

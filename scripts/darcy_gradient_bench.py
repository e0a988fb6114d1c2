#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 16 (adjoint gradients of the Darcy solve), on the finest level of hex 64^3 / 32^3 /
16^3 and of cube_tet refined five times, default solver options, one launch width of lognormal draws k = exp(N(0, 1)):

  * milliseconds per realization of solve_gradient (forward solve + adjoint solve + gradient kernel) beside solve_fwd on the
    same draws in device memory: host clock around calls that end in a stream synchronise, alternated, best of --reps;
  * the mass-sensitivity kernel alone: HIP-event brackets around its launches inside those calls
    (pmc_darcy_set_operator_timing), its algorithmic bytes (pmc_darcy_mass_sensitivity_bytes) over the bracket time, beside the
    in-loop bracket of the Darcy operator's u-rows (eg_pair_spmm) of the same solves.
Prints one JSON line per mesh; --out also writes them to a JSON file.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hierarchy(name):
    from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
    if name == "hex64":
        return build_hierarchy(box_mesh([16, 16, 16], [1, 1, 1], "hex"), 2)
    m = mesh_from_json(os.path.join(ROOT, "tests", "golden", "meshes", "cube_tet.json"))
    cen = m.verts[m.bdr].mean(axis=1)
    lo, hi = m.verts[:, 0].min(), m.verts[:, 0].max()
    m.bdr_attr = np.where(np.isclose(cen[:, 0], lo), 1, np.where(np.isclose(cen[:, 0], hi), 6, 2)).astype(m.bdr_attr.dtype)
    return build_hierarchy(m, 5)


def measure(name, reps, small):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy
    h = build_hierarchy(box_mesh([4, 4, 4], [1, 1, 1], "hex"), 1) if small else hierarchy(name)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    L = dp.levels[0]
    ctx = capi.Context(0, seed=5)
    ds = capi.DarcySolver(ctx, dp)
    nb = min(ds.BatchWidth(0), 32)
    rng = np.random.default_rng(7)
    k = ctx.array(np.exp(rng.standard_normal((nb, L.n_p))))
    grad = ctx.empty(nb * L.n_p)

    def fwd():
        return ds.SolveFwd(0, k, nbatch=nb, return_stats=True)

    def gradient():
        return ds.solve_gradient(0, k, nbatch=nb, grad_out=grad, return_stats=True)

    fwd()
    gradient()                                   # warm-up: code objects, buffers, the level's gradient data
    best = {"fwd": float("inf"), "grad": float("inf")}
    for _ in range(reps):
        for what, fn in (("fwd", fwd), ("grad", gradient)):
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            best[what] = min(best[what], (time.perf_counter() - t0) * 1e3)
    st_f, st_a = out[-2], out[-1]
    # kernel brackets, in a pass of their own (the timed operator launches leave the two-stream schedule)
    ds.set_operator_timing(True)
    ds.operator_time()
    ds.mass_sensitivity_time()
    for _ in range(reps):
        gradient()
    op_ms, op_n, op_gap = ds.operator_time()
    ms_ms, ms_n, ms_gap = ds.mass_sensitivity_time()
    ds.set_operator_timing(False)
    ms_bytes, op_bytes = ds.mass_sensitivity_bytes(0, nb), ds.operator_bytes(0, nb)
    rec = dict(mesh=name if not small else "hex8(small)", n_p=L.n_p, n_u=L.n_u, nb=nb,
               solve_fwd_ms_per_realization=best["fwd"] / nb, solve_gradient_ms_per_realization=best["grad"] / nb,
               ratio=best["grad"] / best["fwd"], iterations_fwd=max(s[0] for s in st_f), iterations_adj=max(s[0] for s in st_a),
               mass_sensitivity_us=1e3 * ms_ms / max(ms_n, 1), mass_sensitivity_launches=ms_n,
               mass_sensitivity_empty_bracket_us=1e3 * ms_gap / max(ms_n, 1), mass_sensitivity_bytes=ms_bytes,
               mass_sensitivity_GBps=ms_bytes / (ms_ms / max(ms_n, 1)) * 1e-6 if ms_ms > 0 else None,
               operator_us=1e3 * op_ms / max(op_n, 1), operator_launches=op_n, operator_bytes=op_bytes,
               operator_GBps=op_bytes / (op_ms / max(op_n, 1)) * 1e-6 if op_ms > 0 else None)
    for a in (k, grad):
        a.free()
    ds.close()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--meshes", default="hex64,tet5")
    ap.add_argument("--small", action="store_true", help="an 8^3 mesh instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out")
    args = ap.parse_args()
    recs = []
    for name in args.meshes.split(","):
        recs.append(measure(name, args.reps, args.small))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

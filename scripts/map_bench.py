#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 19 (batched MAP estimation by inexact Gauss-Newton-CG), on the finest level of hex 64^3
and of cube_tet refined five times, a lognormal SPDE prior, two observation functionals, default solver and MAP options, 16
starting points 0.5 * N(0, 1) in device memory:

  1. seconds of one pmc_bayes_map beside the same loop driven from Python through the existing entries
     (pmc_bayes_logpost_gradient, pmc_bayes_logpost_gn_hessvec) with the CG and line-search algebra in torch on the device -
     what a caller had before this entry: host clock around calls that end synchronised, alternated, best of --reps; the two
     must take the same integer trajectory for the comparison to mean anything, which is recorded;
  2. the three CG kernels of one pmc_ncg_step at n = 262 144, nb = 64: bytes moved (11 vector passes of 8 n nb bytes: <p, Hp>
     reads 2, the d / r update reads 4 and writes 2, the p update reads 2 and writes 1) over the time of a step - the time of
     (begin + step) pairs minus that of begins alone, each over --kreps calls between two synchronisations - beside
     add_inplace_kernel (pmc_sampler_logprior_hessvec, 3 passes) in the same process, and the step's share of one Hessian
     action of item 1.
Prints one JSON line per record and writes them to --out (profiles/map_bench.json).  Nothing is asserted."""
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


def observations(h):
    vol = h.spaces[0].vol
    n = vol.size
    a, b, c = n // 3, (2 * n) // 3, (2 * n) // 3 + 1
    return sp.csr_matrix(([vol[a], vol[b], vol[c]], ([0, 1, 1], [a, b, c])), shape=(2, n))


class Dev:
    """a torch tensor as the (ptr) object the host_api entries take for device memory"""

    def __init__(self, t):
        self.t, self.ptr = t, t.data_ptr()


def python_loop(smp, ds, xi, data, o):
    """pmc_bayes_map's loop over the two existing entries, vectors and algebra in torch on the device, decisions on host
    scalars: returns (outer iterations, Hessian actions) per column; xi (torch, nb x n) is overwritten"""
    import torch
    from parelagmc_amd import host_api
    nb, n = xi.shape
    n_p, nd = ds.problem.levels[0].n_p, ds.GetGlobalNumberOfDofs(0)
    g, gt, hp, trial = (torch.empty_like(xi) for _ in range(4))
    kst = torch.empty((nb, n_p), dtype=xi.dtype, device=xi.device)
    xst = torch.empty((nb, nd), dtype=xi.dtype, device=xi.device)

    # torch works on its own stream, the library on the context's: each side waits for the other around every call
    def grad(x, out):
        torch.cuda.synchronize()
        lp = host_api.bayes_logpost_gradient(smp, ds, 0, Dev(x), data, NOISE, nbatch=nb, grad_out=Dev(out))[0]
        smp.ctx.synchronize()
        return torch.from_numpy(lp)

    lp = grad(xi, g)
    gn = g.norm(dim=1).cpu()
    gn0 = gn.clone()
    running = torch.ones(nb, dtype=torch.bool)
    iters, nhess = torch.zeros(nb, dtype=torch.int64), torch.zeros(nb, dtype=torch.int64)
    for it in range(o.max_newton + 1):
        running &= ~(gn <= torch.maximum(o.grad_rtol * gn0, torch.tensor(o.grad_atol, dtype=gn.dtype)))
        if it == o.max_newton or not running.any():
            break
        run_d = running.to(xi.device)
        eta = torch.minimum(torch.tensor(o.eta_max, dtype=gn.dtype), torch.sqrt(gn / gn0)).to(xi.device)
        d = torch.zeros_like(xi)
        r = torch.where(run_d[:, None], g, torch.zeros_like(g))
        p = r.clone()
        rr = (r * r).sum(1)
        tol2 = eta * eta * rr
        live = run_d.clone()
        for j in range(o.max_cg):
            torch.cuda.synchronize()
            host_api.bayes_logpost_gn_hessvec(smp, ds, 0, Dev(xi), Dev(p), NOISE, state=(Dev(kst), Dev(xst), j > 0), nbatch=nb,
                                              hv_out=Dev(hp))
            smp.ctx.synchronize()
            nhess += live.cpu().to(torch.int64)
            php = (p * hp).sum(1)
            ok = live & (php > 0)
            alpha = torch.where(ok, rr / php, torch.zeros_like(rr))
            d += alpha[:, None] * p
            r -= alpha[:, None] * hp
            rr_new = torch.where(ok, (r * r).sum(1), rr)
            live = ok & (rr_new > tol2)
            p = torch.where(live[:, None], r + (rr_new / rr)[:, None] * p, torch.zeros_like(p))
            rr = rr_new
            if not live.any().item():
                break
        gd = (g * d).sum(1).cpu()
        t = running.to(gn.dtype)
        searching, accepted = running.clone(), torch.zeros(nb, dtype=torch.bool)
        for ls in range(o.max_backtracks + 1):
            torch.add(xi, t.to(xi.device)[:, None] * d, out=trial)
            lpt = grad(trial, gt)
            okk = searching & torch.isfinite(lpt) & (lpt >= lp + o.c1 * t * gd)
            accepted |= okk
            searching &= ~okk
            if ls == o.max_backtracks or not searching.any():
                break
            t = torch.where(searching, 0.5 * t, t)
        acc_d = accepted.to(xi.device)[:, None]
        xi.copy_(torch.where(acc_d, trial, xi))
        g.copy_(torch.where(acc_d, gt, g))
        lp = torch.where(accepted, lpt, lp)
        gn = torch.where(accepted, g.norm(dim=1).cpu(), gn)
        iters += accepted.to(torch.int64)
        running &= accepted
    return iters.tolist(), nhess.tolist()


def measure_map(name, reps, small, nb):
    import torch
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import build_darcy_problem, build_sampler_problem
    h = hierarchy(name, small)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)
    spb = build_sampler_problem(h, corlen=0.3, lognormal=True, n_mc_levels=1)
    ctx = capi.Context(0, seed=5)
    smp, ds = capi.PDESampler(ctx, spb), capi.DarcySolver(ctx, dp)
    ds.SetObservations(0, observations(h))
    n = spb.levels[0].n_s
    rng = np.random.default_rng(11)
    data = ds.ComputeG(0, smp.Eval(0, rng.standard_normal((1, n))))[0][0] + np.sqrt(NOISE) * rng.standard_normal(2)
    x0 = torch.from_numpy(0.5 * rng.standard_normal((nb, n))).cuda()
    o = host_api.map_opts()
    best = {"entry": float("inf"), "python": float("inf")}
    traj = {}
    for rep in range(reps + 1):                  # the first round warms up: code objects, buffers, the levels' data
        for what in ("entry", "python"):
            xi = x0.clone()
            torch.cuda.synchronize()
            ctx.synchronize()
            t0 = time.perf_counter()
            if what == "entry":
                _, res = host_api.bayes_map(smp, ds, 0, xi, data, NOISE, opts=o, nbatch=nb, history=False)
                traj[what] = (res["newton_iterations"].tolist(), res["hessian_actions"].tolist())
                status = res["status"].tolist()
            else:
                traj[what] = python_loop(smp, ds, xi, data, o)
            torch.cuda.synchronize()
            ctx.synchronize()
            if rep:
                best[what] = min(best[what], time.perf_counter() - t0)
    # one Hessian action with the state given, for the share of item 2
    v = torch.from_numpy(rng.standard_normal((nb, n))).cuda()
    hv = torch.empty_like(v)
    torch.cuda.synchronize()
    kst = torch.empty((nb, dp.levels[0].n_p), dtype=v.dtype, device=v.device)
    xst = torch.empty((nb, ds.GetGlobalNumberOfDofs(0)), dtype=v.dtype, device=v.device)
    act = float("inf")
    for rep in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        host_api.bayes_logpost_gn_hessvec(smp, ds, 0, Dev(x0), Dev(v), NOISE, state=(Dev(kst), Dev(xst), rep > 0), nbatch=nb,
                                          hv_out=Dev(hv))
        ctx.synchronize()
        if rep:
            act = min(act, time.perf_counter() - t0)
    rec = dict(what="map", mesh="hex8(small)" if small else name, n_xi=n, nb=nb, status=status,
               pmc_bayes_map_s=best["entry"], python_loop_s=best["python"], ratio=best["python"] / best["entry"],
               outer_iterations=traj["entry"][0], hessian_actions=traj["entry"][1],
               same_trajectory=traj["entry"] == traj["python"], hessian_action_ms=1e3 * act)
    ds.close()
    smp.close()
    ctx.close()
    return rec


def measure_kernels(n, nb, kreps, small):
    import torch
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_sampler_problem
    if small:
        n, nb = 4096, 8
    ctx = capi.Context(0, seed=5)
    smp = capi.PDESampler(ctx, build_sampler_problem(build_hierarchy(box_mesh([2, 2, 2], [1, 1, 1], "hex"), 0), corlen=0.3))
    ncg = capi.NewtonCG(ctx, n, nb)
    g = torch.randn((nb, n), dtype=torch.float64, device="cuda")
    hp = 2.0 * g + 0.1 * torch.randn_like(g)
    torch.cuda.synchronize()
    eta = np.zeros(nb)

    def timed(fn, reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) / reps

    def begin():
        ncg.begin(nb, g, eta)

    def begin_step():
        ncg.begin(nb, g, eta)
        ncg.step(nb, hp)

    def add_inplace():
        ctx.lib.pmc_sampler_logprior_hessvec(smp.h, n, nb, g.data_ptr(), hp.data_ptr(), capi.PMC_MEM_DEVICE)

    best = dict(begin=float("inf"), pair=float("inf"), add=float("inf"))
    for rep in range(4):
        for what, fn in (("begin", begin), ("pair", begin_step), ("add", add_inplace)):
            t = timed(fn, kreps)
            if rep:
                best[what] = min(best[what], t)
    vec = 8.0 * n * nb
    step_s = best["pair"] - best["begin"]
    rec = dict(what="kernels", n=n, nb=nb, step_us=1e6 * step_s, step_GBps=11 * vec / step_s * 1e-9,
               begin_us=1e6 * best["begin"], add_inplace_us=1e6 * best["add"], add_inplace_GBps=3 * vec / best["add"] * 1e-9)
    ncg.close()
    smp.close()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=50)
    ap.add_argument("--nb", type=int, default=16)
    ap.add_argument("--meshes", default="hex64,tet5")
    ap.add_argument("--small", action="store_true", help="an 8^3 mesh instead (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
    args = ap.parse_args()
    recs = [measure_kernels(262144, 64, args.kreps, args.small)]
    print(json.dumps(recs[-1]), flush=True)
    for name in args.meshes.split(","):
        recs.append(measure_map(name, args.reps, args.small, args.nb))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()

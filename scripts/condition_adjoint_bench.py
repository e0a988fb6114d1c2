#!/usr/bin/env python3
"""Measurements behind DESIGN.md section 22 (adjoint of the conditioning map), on hex 64^3 level 0 (n = 262 144), nobs = 64,
64 and 256 realizations per call.

  --kernels      launches the adjoint (pmc_conditioner_apply_adjoint on device arrays: cond_adjoint_mfma and
                 cond_adjoint_finish_kernel) beside its two yardsticks, which move the same matrix: the forward update
                 cond_update_mfma (pmc_conditioner_apply) and the KL adjoint's kl_adjoint_mfma_kernel on a KL handle of the
                 same n with m = nobs modes, `--reps` times each.  Run it under
                 `rocprofv3 --kernel-trace --stats -- python scripts/condition_adjoint_bench.py --kernels`, in a run of its
                 own, and read the kernel times from the profiler's statistics; the HIP-event times printed here are a
                 cross-check that includes launch gaps and each call's second, small kernel.
  --whole-path   a conditioned EvalAdjoint of one batch width (derivatives enabled) against the same hybridized handle
                 detached, alternated, best of three each; reports the overhead in percent.
Prints one JSON line per measurement; --out writes them to a JSON file."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOBS = 64


def adjoint_bytes(n, nobs_padded, nb, with_s=False):
    """algorithmic bytes of the adjoint: K once, v in (and s_out), w out; the O(nobs nb) terms left out"""
    return 8.0 * n * nobs_padded + (3 if with_s else 2) * 8.0 * n * nb


def update_bytes(n, nobs_padded, nobs, nb):
    """algorithmic bytes of the forward update kernel: K once, g in, s out, the coefficients"""
    return 8.0 * n * nobs_padded + 2 * 8.0 * n * nb + 8.0 * nobs * nb


def kl_adjoint_bytes(n, m, nb):
    """algorithmic bytes of kl_adjoint_mfma_kernel: Phi once, v in, the partials"""
    return 8.0 * n * m + 8.0 * n * nb + 8.0 * m * nb


def kernels(args, emit):
    from parelagmc_amd import capi
    from parelagmc_amd.fe.kl import KLLevel, KLProblem
    n = args.n
    rng = np.random.default_rng(1)
    phi, _ = np.linalg.qr(rng.standard_normal((n, NOBS)))
    phi *= np.sqrt(n)     # unit P0 mass norm with w = 1 / n
    prob = KLProblem([KLLevel(n, np.full(n, 1.0 / n), None)], 1, np.linspace(1.0, 0.1, NOBS), np.ascontiguousarray(phi), False,
                     "random", [phi])
    ctx = capi.Context(0, seed=3)
    smp = capi.KLSampler(ctx, prob)
    elems = np.sort(rng.choice(n, NOBS, replace=False))
    H0 = sp.csr_matrix((np.ones(NOBS), (np.arange(NOBS), elems)), shape=(NOBS, n))
    cond = capi.Conditioner(smp, H0, rng.standard_normal(NOBS), np.full(NOBS, 0.05))
    for nb in (64, 256):
        v = ctx.array(rng.standard_normal((nb, n)))
        w = ctx.empty(nb * n)
        g = ctx.array(rng.standard_normal((nb, n)))
        zeta = ctx.array(rng.standard_normal((nb, NOBS)))
        grad = ctx.empty(nb * n)
        res = {}
        for name, fn in (("kl_adjoint_mfma_kernel", lambda: smp.EvalAdjoint(0, v, xi_level=0, grad_out=grad, nbatch=nb)),
                         ("cond_update_mfma", lambda: cond.apply(0, g, zeta)),
                         ("cond_adjoint_mfma", lambda: cond.apply_adjoint(0, v, out=w))):
            for _ in range(2):
                fn()
            ctx.synchronize()
            best = float("inf")
            for _ in range(args.reps):
                ctx.timer_start()
                fn()
                best = min(best, ctx.timer_stop())
            res[name] = best
        ba, bu, bk = adjoint_bytes(n, NOBS, nb), update_bytes(n, NOBS, NOBS, nb), kl_adjoint_bytes(n, NOBS, nb)
        emit(dict(what="kernels_hip_events", n=n, nobs=NOBS, nb=nb, adjoint_call_ms=res["cond_adjoint_mfma"],
                  update_call_ms=res["cond_update_mfma"], kl_adjoint_call_ms=res["kl_adjoint_mfma_kernel"], adjoint_bytes=ba,
                  update_bytes=bu, kl_adjoint_bytes=bk, adjoint_GBps=ba / res["cond_adjoint_mfma"] * 1e-6,
                  update_GBps=bu / res["cond_update_mfma"] * 1e-6, kl_adjoint_GBps=bk / res["kl_adjoint_mfma_kernel"] * 1e-6,
                  adjoint_over_update=res["cond_adjoint_mfma"] / res["cond_update_mfma"],
                  adjoint_over_kl_adjoint=res["cond_adjoint_mfma"] / res["kl_adjoint_mfma_kernel"],
                  note="HIP events around the whole call: each call is two launches (reduction + finish, coefficients + "
                       "update, product + reduce)"))
        for a in (v, w, g, zeta, grad):
            a.free()
    cond.close()
    smp.close()
    ctx.close()


def whole_path(args, emit):
    from parelagmc_amd import capi
    from parelagmc_amd.fe import box_mesh, build_hierarchy, build_hybrid_sampler_problem
    e = round(args.n ** (1.0 / 3.0))
    h = build_hierarchy(box_mesh([e, e, e], [1, 1, 1], "hex"), 0)
    prob = build_hybrid_sampler_problem(h, corlen=0.1, lognormal=True)
    ctx = capi.Context(0, seed=3)
    smp = capi.PDESampler(ctx, prob)
    n = prob.levels[0].n_s
    rng = np.random.default_rng(2)
    elems = np.sort(rng.choice(n, NOBS, replace=False))
    H0 = sp.csr_matrix((np.ones(NOBS), (np.arange(NOBS), elems)), shape=(NOBS, n))
    cond = capi.Conditioner(smp, H0, rng.standard_normal(NOBS)).enable_derivatives()
    W = smp.BatchWidth(0)
    v = ctx.array(rng.standard_normal((W, n)))
    grad = ctx.empty(W * n)
    best = {False: float("inf"), True: float("inf")}
    smp.EvalAdjoint(0, v, xi_level=0, grad_out=grad, nbatch=W)
    for _ in range(3):
        for attached in (False, True):
            smp.SetConditioner(cond if attached else None)
            if attached and best[True] == float("inf"):
                smp.EvalAdjoint(0, v, xi_level=0, grad_out=grad, nbatch=W)      # the conditioner's buffers grow here
            ctx.timer_start()
            smp.EvalAdjoint(0, v, xi_level=0, grad_out=grad, nbatch=W)
            best[attached] = min(best[attached], ctx.timer_stop())
    emit(dict(what="whole_path", n=n, nobs=NOBS, nb=W, eval_adjoint_ms=best[False], conditioned_eval_adjoint_ms=best[True],
              overhead_percent=100.0 * (best[True] / best[False] - 1.0)))
    smp.SetConditioner(None)
    cond.close()
    smp.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--whole-path", action="store_true")
    ap.add_argument("--n", type=int, default=64 ** 3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    if args.kernels:
        kernels(args, emit)
    if args.whole_path:
        whole_path(args, emit)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Matrix-free Matern eigensolver (pmc_kl_matern_eigs / pmc_kl_matern_apply, csrc/kl_eigs.hip): what it costs on the project's
KL workload, hex 32^3 on [0,2]^3 (n = 32 768), corlen 0.1, m = 64, guard 16 (block of 80 columns).

  --mode all       (default) runs the three steps below as child processes and writes profiles/kl_matern_bench.json
  --mode solve     pmc_kl_matern_eigs at n = 32 768 (wall time, iterations, block products) and at n = 4096, m = 60 next to
                   the dense host matern_eigs; prints one JSON line
  --mode products  `--reps` block products of 80 columns at n = 32 768 and nothing else: the process that
                   `rocprofv3 --kernel-trace --stats` wraps (a run of its own, no counters alongside)

Kernel time per block product comes from the kernel-stats CSV of the traced run.  It is read against
    max(2 n^2 b / 49.2 TFLOP/s, time of the n^2 sqrt + exp evaluations on the VALU)
where 49.2 TFLOP/s is the fp64 MFMA rate DESIGN section 10 measured on this part.  The second term is measured: the same
trace of a laboratory build of the library that keeps the evaluations and drops the MFMAs
    make lab-lib LABEXTRA=-DPMC_KL_EVAL_ONLY
(parelagmc_amd/lib/libpmc_lab.so, selected with PMC_LIB; skipped, and reported as not measured, when that file is absent)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MFMA_TFLOPS = 49.2      # DESIGN section 10 (scripts/lab/f64_mfma_rate.hip on MI355X)
N_BIG, M_BIG, GUARD, CORLEN = 32, 64, 16, 0.1


def _points(nx):
    from parelagmc_amd.fe import box_mesh, build_hierarchy
    from parelagmc_amd.fe.mesh import element_centroids
    h = build_hierarchy(box_mesh([nx, nx, nx], [2, 2, 2], "hex"), 0)
    return h, np.ascontiguousarray(element_centroids(h.spaces[0].mesh)), np.ascontiguousarray(h.spaces[0].vol)


def products(reps):
    from parelagmc_amd import capi
    _, x, w = _points(N_BIG)
    ctx = capi.Context(0, seed=1)
    X = np.random.default_rng(0).standard_normal((w.size, M_BIG + GUARD))
    t0 = time.time()
    for _ in range(reps):
        capi.kl_matern_apply(ctx, x, w, CORLEN, X)
    ctx.close()
    print(json.dumps({"reps": reps, "host_seconds_per_call_with_transfers": (time.time() - t0) / reps}))


def solve():
    from parelagmc_amd import capi
    from parelagmc_amd.fe.kl import matern_eigs
    ctx = capi.Context(0, seed=1)
    res = {}
    _, x, w = _points(N_BIG)
    capi.kl_matern_eigs(ctx, x[:4096], w[:4096], CORLEN, 8)          # loads the code objects
    lam, _, info = capi.kl_matern_eigs(ctx, x, w, CORLEN, M_BIG, guard=GUARD)
    res["n32768_m64"] = dict(info, lambda_1=float(lam[-1]), lambda_m=float(lam[0]))
    h, x, w = _points(16)
    lam, _, info = capi.kl_matern_eigs(ctx, x, w, CORLEN, 60, guard=GUARD)
    t0 = time.time()
    lam_d, _ = matern_eigs(h, CORLEN, 60)
    res["n4096_m60"] = dict(info, host_dense_seconds=time.time() - t0, host_threads=os.cpu_count() if
                            "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]),
                            eigenvalue_error_rel=float(np.abs(lam - lam_d).max() / lam_d[-1]))
    ctx.close()
    print(json.dumps(res))


def _traced_products(outdir, reps, lib=None):
    """kernel-stats rows {kernel name: (calls, average ns)} of a traced --mode products run"""
    os.makedirs(outdir, exist_ok=True)
    env = dict(os.environ)
    if lib:
        env["PMC_LIB"] = lib
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "p", "--output-format", "csv", "--",
                    sys.executable, os.path.abspath(__file__), "--mode", "products", "--reps", str(reps)],
                   check=True, env=env, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
    with open(files[0]) as f:
        return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(f)}


def _apply_row(stats):
    rows = [(k, v) for k, v in stats.items() if "kl_matern_apply_kernel" in k]
    if len(rows) != 1:
        raise RuntimeError(f"expected one kl_matern_apply_kernel row, found {len(rows)}")
    return rows[0]


def run_all(a):
    out = {"workload": f"hex {N_BIG}^3 on [0,2]^3, n = {N_BIG ** 3}, corlen {CORLEN}, m = {M_BIG}, guard {GUARD}",
           "f64_mfma_tflops_reference": F64_MFMA_TFLOPS}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "solve"], check=True, capture_output=True,
                       text=True, timeout=900)
    out["solve"] = json.loads(r.stdout.strip().splitlines()[-1])
    n, b = N_BIG ** 3, M_BIG + GUARD
    flops = 2.0 * n * n * b
    name, (calls, avg_ns) = _apply_row(_traced_products(os.path.join(a.workdir, "kl_matern_trace"), a.reps))
    t_mfma = flops / (F64_MFMA_TFLOPS * 1e12)
    bp = {"kernel": name, "calls": calls, "columns": b, "ms": avg_ns * 1e-6, "flops": flops,
          "kernel_evaluations": float(n) * n, "tflops": flops / (avg_ns * 1e-9) / 1e12,
          "fraction_of_f64_mfma_rate": flops / (avg_ns * 1e-9) / 1e12 / F64_MFMA_TFLOPS, "bound_mfma_ms": t_mfma * 1e3}
    lab = os.path.join(ROOT, "parelagmc_amd", "lib", "libpmc_lab.so")
    if os.path.exists(lab):
        _, (_, eval_ns) = _apply_row(_traced_products(os.path.join(a.workdir, "kl_matern_trace_eval_only"), a.reps, lab))
        bp["bound_valu_evaluations_ms"] = eval_ns * 1e-6
        bp["bound_ms"] = max(t_mfma * 1e3, eval_ns * 1e-6)
        bp["ms_over_bound"] = bp["ms"] / bp["bound_ms"]
    else:
        bp["bound_valu_evaluations_ms"] = None       # not measured: no laboratory build of the library next to the product
    out["block_product"] = bp
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "solve", "products"])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--workdir", default=os.path.join(ROOT, "build", "kl_matern_bench"),
                    help="directory the traces are written to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_matern_bench.json"))
    a = ap.parse_args()
    if a.mode == "products":
        products(a.reps)
    elif a.mode == "solve":
        solve()
    else:
        run_all(a)


if __name__ == "__main__":
    main()

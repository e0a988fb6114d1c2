"""bench.py command line without a GPU: the rank launcher of `--gpus N` propagates a failing rank's exit code, and a launcher
environment that contradicts `--gpus` is refused before anything heavy happens.  --dump-outputs: the selection logic here, the
real run on the GPU (marked).  A plain run measures the headline alone, --full everything behind it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _run(args, env_extra=None, drop=()):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT") + tuple(drop):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=600)


def test_spawned_ranks_propagate_failure():
    """No GPU here: both ranks die in torch.cuda.set_device; the parent must return non-zero and print no JSON line
    (the reference's mpirun does the same for a failing rank)."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("needs a box without a GPU")
    r = _run(["--gpus", "2", "--refine", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-r6", "--no-mlmc"])
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "No HIP GPUs" in r.stderr or "no HIP device" in r.stderr or "RuntimeError" in r.stderr


def test_launcher_world_size_must_match_gpus():
    r = _run(["--gpus", "2"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def _canned_full_record():
    """a complete record as bench.py assembled it in round 4 (21.7 kB as ONE line: the driver kept only its tail)"""
    import json
    with open(os.path.join(ROOT, "profiles", "r04_bench_output.log")) as f:
        return json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])


REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def test_compact_line_fits_the_drivers_window_and_keeps_the_contract():
    import json
    sys.path.insert(0, ROOT)
    import bench
    full = _canned_full_record()
    assert len(json.dumps(full)) > 20000
    line = bench.compact_line(full)
    assert "\n" not in line and len(line) < bench.LINE_CAP <= 4096
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert d["value"] == float(f"{full['value']:.6g}") and d["metric"] == full["metric"]
    assert len(d["config"]["workload"]) <= 200 and len(d["roofline"]["kernel"]) <= 80
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "bytes_per_launch", "avg_kernel_ms", "operator_frac",
              "saddle_k5_frac", "solver_frac"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-3
    assert abs(d["roofline"]["saddle_k5_frac"] - full["extra"]["saddle_point_minres"]["roofline"]["frac"]) < 1e-3
    for k in ("value", "cores", "kind", "unit", "sample"):
        assert k in d["cpu_baseline"], k
    # extra: scalars and flat lists of scalars only
    for k, v in d["extra"].items():
        assert not isinstance(v, dict), k
        if isinstance(v, list):
            assert all(not isinstance(x, (dict, list)) for x in v), k
    assert d["extra"]["c3_value"] > 0 and len(d["extra"]["c4_values"]) == 3 and len(d["extra"]["c5_values"]) == 4


def test_compact_line_with_eight_ranks_and_a_farm_block_stays_below_the_cap():
    import json
    sys.path.insert(0, ROOT)
    import bench
    full = _canned_full_record()
    full["n_gpus"] = 8
    full["ranks"] = [dict(full["ranks"][0], rank=r, device=r, cpu_affinity={"pinned": True, "numa_node": r // 4, "ncpus": 48})
                     for r in range(8)]
    full.pop("cpu_baseline")
    full["extra"] = {"mlmc_farm": dict(full["extra"]["mlmc_config3"], allreduce_ms=0.3, allreduces_in_round=1,
                                       allreduce_ms_per_rank=[0.3] * 8, collective="rccl (pmc_allreduce_sum_f64 of the "
                                       "library's communicator)", ranks_in_rccl_communicator=8)}
    line = bench.compact_line(full)
    assert len(line) < bench.LINE_CAP
    d = json.loads(line)
    assert d["n_gpus"] == 8 and d["rank_seconds"]["max"] >= d["rank_seconds"]["min"]
    assert d["extra"]["farm_allreduces_in_round"] == 1 and "ranks" not in d


def test_compact_line_survives_failed_secondary_figures():
    import json
    sys.path.insert(0, ROOT)
    import bench
    full = _canned_full_record()
    full["extra"] = {k: {"error": "RuntimeError('x' * 5000)" + "y" * 5000, "wall_s": 1.0} for k in full["extra"]}
    full["cpu_baseline"] = {"error": "z" * 9000}
    d = json.loads(bench.compact_line(full))
    assert "mlmc_config3" in d["extra"]["errors"] and d["value"] > 0


def test_compact_line_of_the_round5_record_carries_the_event_overhead_fields():
    """the full record of this round's gate run (profiles/r05_gate_bench_full.json, written before bench.py computed the net
    figure itself): raw frac is kept as it is, the net-of-event-overhead figure is passed through when the record has it"""
    import json
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, "profiles", "r05_gate_bench_full.json")) as f:
        full = json.load(f)
    rf = full["roofline"]
    net = rf["bytes_per_launch"] / ((rf["avg_kernel_ms"] - rf["event_overhead_ms"]) * 1e-3) / 1e9 / bench.PEAK_GBS
    rf["frac_net_of_event_overhead"] = net
    line = bench.compact_line(full)
    assert len(line) < bench.LINE_CAP
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    r = d["roofline"]
    assert abs(r["frac"] - rf["frac"]) < 1e-3 and abs(r["frac_net_of_event_overhead"] - net) < 1e-3
    assert r["frac"] < r["frac_net_of_event_overhead"] < r["frac"] * 1.06      # a 4-5 us bracket on a ~147 us launch
    assert 0.003 < r["event_overhead_ms"] < 0.008
    assert d["cpu_baseline"]["solver"].startswith("PCG") and d["config"]["solver"] == "hybridization"


class _Buf:
    def __init__(self, a):
        self.a = a

    def download(self):
        return self.a.ravel().copy()


class _Farm:
    """the part of bench.SamplerFarm dump_outputs reads: ns lanes of (ctx, sampler, xi buffer, field buffer), nb x n each;
    entry (row, col) of a step holds 1000 * realization id + col (field: its negative)"""

    def __init__(self, ns, nb, n, step):
        self.ns, self.nb, self.n = ns, nb, n
        ids = step * ns * nb + np.arange(ns * nb)
        v = 1000.0 * ids[:, None] + np.arange(n)[None, :]
        self.lanes = [(None, None, _Buf(v[k * nb:(k + 1) * nb]), _Buf(-v[k * nb:(k + 1) * nb])) for k in range(ns)]


def _dumped(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("budget", [1 << 20, 6 << 10, 2 << 10])
def test_dump_outputs_fits_its_budget_and_keeps_rows_whole(tmp_path, budget):
    """--dump-outputs: float64 files only, within the byte budget, the same selection on every call; every dumped row is the
    realization realization_ids names (whole when one row fits, a fixed set of columns otherwise)"""
    sys.path.insert(0, ROOT)
    import bench
    ns, nb, n, step = 3, 4, 100, 7
    stats = [(20 + i, 1, 1.0, 1e-7) for i in range(ns * nb)]
    outs = []
    for k in range(2):
        d = str(tmp_path / f"d{k}")
        bench.dump_outputs(d, _Farm(ns, nb, n, step), step, stats, seed=11, budget=budget)
        outs.append(_dumped(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= budget
    a, b = outs
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype == np.float64 for v in a.values())
    ids, xi, s = a["realization_ids"], a["xi"], a["field"]
    cols = a.get("cell_ids", np.arange(n, dtype=np.float64))
    assert len(ids) >= 1 and len(set(ids)) == len(ids)
    assert set(ids) <= set(range(step * ns * nb, (step + 1) * ns * nb))
    assert np.array_equal(xi, 1000.0 * ids[:, None] + cols[None, :]) and np.array_equal(s, -xi)
    assert np.array_equal(a["stats"], np.asarray(stats, np.float64))
    if budget == 1 << 20:
        assert len(ids) == ns * nb and "cell_ids" not in a
    else:
        assert len(ids) < ns * nb
    assert ("cell_ids" in a) == (budget == 2 << 10)


def test_steps_below_one_are_refused():
    r = _run(["--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


def test_all_configs_without_full_is_refused():
    r = _run(["--all-configs"])
    assert r.returncode == 2 and "--full" in r.stderr


def _args(**kw):
    a = dict(full=False, no_extras=False, no_mlmc=False, no_r6=False, refine=5, only_config=None)
    a.update(kw)
    return argparse.Namespace(**a)


def test_only_a_full_run_sets_up_the_other_configurations():
    """a plain run starts no background setup worker and plans no extra.* figure, whatever --no-* options it is given"""
    sys.path.insert(0, ROOT)
    import bench
    for world in (1, 2):
        for kw in ({}, {"no_mlmc": True}, {"no_extras": True}, {"only_config": 4}):
            assert not bench.extras_planned(_args(**kw), world) and bench.setup_kinds(_args(**kw), world) == []
    assert bench.extras_planned(_args(full=True), 1) and not bench.extras_planned(_args(full=True), 2)
    assert bench.setup_kinds(_args(full=True), 1) == ["c3", "r6", "c4", "c5"]
    assert bench.setup_kinds(_args(full=True, refine=6, only_config=5), 1) == ["c3", "c5"]
    assert bench.setup_kinds(_args(full=True), 2) == ["c3"]
    assert bench.setup_kinds(_args(full=True, no_mlmc=True), 2) == []
    assert bench.setup_kinds(_args(full=True, no_extras=True), 1) == []
    assert bench.setup_kinds(_args(full=True, no_mlmc=True, no_r6=True), 1) == []


def test_compact_line_of_a_plain_run_is_the_headline_alone():
    """the record of a plain run has no roofline, cpu_baseline, extra or full record: the line carries none of them, not even
    as a block of nulls"""
    sys.path.insert(0, ROOT)
    import bench
    full = _canned_full_record()
    for k in ("roofline", "cpu_baseline", "extra", "full_record"):
        full.pop(k, None)
    d = json.loads(bench.compact_line(full))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert not {"roofline", "cpu_baseline", "extra", "full_record"} & d.keys()
    assert d["value"] == float(f"{full['value']:.6g}") and d["ms_per_step"] == float(f"{full['ms_per_step']:.6g}")


@pytest.mark.gpu
def test_dump_outputs_is_what_the_timed_path_computed(tmp_path):
    """bench.py --dump-outputs on a small headline: --steps timed steps (ms_per_step in the line), two runs with the same
    arguments dump the same arrays, and the dumped field is the sampler field of the dumped white noise (oracle direct solve)"""
    sys.path.insert(0, ROOT)
    import bench
    from oracle.sampler_oracle import SamplerOracle
    lines, dumps = [], []
    for k in range(2):
        d = str(tmp_path / f"run{k}")
        r = _run(["--refine", "3", "--streams", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-extras",
                  "--dump-outputs", d])
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(_dumped(d))
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    nb, ns = line["config"]["batch"], line["config"]["streams"]
    assert abs(line["value"] - nb * ns / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"]
    a, b = dumps
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    ids = a["realization_ids"]
    assert ids.min() >= (1 + 3 - 1) * ns * nb and ids.max() < (1 + 3) * ns * nb     # the last timed step's realizations
    assert a["stats"].shape == (ns * nb, 4) and np.all(a["stats"][:, 1] == 1)
    so = SamplerOracle(bench.build_problem(3))
    for j in (0, len(ids) - 1):
        ref = so.eval(0, 0, a["xi"][j])[0]
        assert np.linalg.norm(a["field"][j] - ref) / np.linalg.norm(ref) < 1e-5


@pytest.mark.gpu
def test_plain_run_times_what_a_full_run_times(tmp_path):
    """a plain run prints the headline alone (no roofline, cpu_baseline, extra or full record); --full adds the roofline
    block after the timed region, and both runs' last timed step dumps the same arrays"""
    lines, dumps = [], []
    for full in ([], ["--full", "--no-cpu-baseline", "--no-extras"]):
        d = str(tmp_path / f"run{len(full)}")
        r = _run(["--refine", "3", "--streams", "2", "--steps", "2", "--warmup", "1", "--dump-outputs", d] + full)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(_dumped(d))
    plain, full = lines
    assert not {"roofline", "cpu_baseline", "extra", "full_record"} & plain.keys()
    assert full["roofline"]["frac"] > 0 and full["full_record"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[k] == full[k], k
    a, b = dumps
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)

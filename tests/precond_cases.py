"""The handle registries the preconditioner tests (test_gpu_sampler_precond.py, test_gpu_precond.py) and the MINRES
trajectory tests (test_gpu_minres_trajectory.py) share: the sampler handles with what the fp64 oracles need from them, the
permeability fields of the Darcy batches, and the bound of a preconditioner column against its fp64 reference."""
import numpy as np

from conftest import golden_path

# relative L2 bound of a column of B^-1 r against the fp64 reference, per preconditioner storage
REF_TOL = {"fp64": 1e-12, "fp32": 1e-5}

# sampler handles of the preconditioner tests (MC level 0 of each; n_mc_levels = 1), see test_gpu_sampler_precond.py
HANDLES = {
    "hex32-saddle": dict(mesh=("hex", 3), kind="saddle", corlen=0.3, coarsening=0),
    "tet-saddle": dict(mesh=("tet", 2), kind="saddle", corlen=0.5, coarsening=0),
    "hex32-sa": dict(mesh=("hex", 3), kind="saddle", corlen=0.3, coarsening=1),
    "hex12-hybrid": dict(mesh=("hex3", 2), kind="hybrid", corlen=0.3, coarsening=0),
    "hex24-hybrid": dict(mesh=("hex3", 3), kind="hybrid", corlen=0.3, coarsening=0),
}
# ... and the two small saddle-point handles only the trajectory tests solve on: hex 4^3 refined twice (17 152 rows; corlen
# 0.5 needs about 40 iterations) and once (2 240 rows: inside mini_max_rows)
SOLVE_HANDLES = dict(HANDLES)
SOLVE_HANDLES.update({
    "hex16-saddle": dict(mesh=("hex", 2), kind="saddle", corlen=0.5, coarsening=0),
    "hex8-saddle": dict(mesh=("hex", 1), kind="saddle", corlen=0.1, coarsening=0),
})

# Solver options away from the defaults of pmc_solver_opts (test_gpu_precond_options.py): what each set reaches is said
# there.  The Darcy handles ignore schur_scale: darcy_options() leaves it out.
OPTION_SETS = {
    "deg1": dict(mg_smooth_degree=1, mg_coarse_degree=1, cheb_degree_M=1),
    "deg3": dict(mg_smooth_degree=3, mg_smooth_ratio=5.0, mg_coarse_degree=2, mg_coarse_ratio=30.0, cheb_degree_M=3,
                 cheb_ratio_M=6.0),
    "deg4": dict(mg_smooth_degree=4, mg_smooth_ratio=12.0, mg_coarse_degree=5, mg_coarse_ratio=50.0, cheb_degree_M=4,
                 schur_scale=0.7),
    "ratio": dict(mg_smooth_ratio=3.0, mg_coarse_degree=7, schur_scale=1.3),
}


def darcy_options(name):
    return {k: v for k, v in OPTION_SETS[name].items() if k != "schur_scale"}


# the M-block options of deg3: mini_sampler_kernel requires the degree-2 M-block, so the mini case solves without them
_DEG3_SCHUR = {k: v for k, v in OPTION_SETS["deg3"].items() if not k.endswith("_M")}

# sampler handles of test_gpu_precond_options.py beyond HANDLES: the smallest shapes that still leave the LDS tail - hex 5^3
# refined twice (20^3: Schur levels 8 000 / 1 000 / 125, three vectors each = 27 375 doubles against kTailLdsDoubles = 20 352)
# on the caller's hierarchy and on the internal smoothed aggregation - and hex 4^3 refined once with a correlation length at
# which no level is reaction-dominated (corlen 2: alpha = 1/4), so that the cycle ends on the LAST level with the polynomial of
# mg_coarse_degree / mg_coarse_ratio (at the other handles' corlen a level's own Gershgorin interval ends it: is_last)
OPTION_HANDLES = {
    "hex20-saddle": dict(mesh=("hex5", 2), kind="saddle", corlen=0.3, coarsening=0),
    "hex20-sa": dict(mesh=("hex5", 2), kind="saddle", corlen=0.3, coarsening=1, problem="hex20-saddle"),
    "hex8-long": dict(mesh=("hex", 1), kind="saddle", corlen=2.0, coarsening=0),
    # ... and 20^3 at corlen 0.03, where level 0 itself is reaction-dominated at every schur_scale of the sets (lmax / lo 2.1 to
    # 3.1 <= 3.5): the cycle is ONE polynomial, on a level too large for the tail - cycle_bottom on kernels
    "hex20-reaction": dict(mesh=("hex5", 2), kind="saddle", corlen=0.03, coarsening=0),
}
SOLVE_HANDLES.update(OPTION_HANDLES)
# ... and the two handles of the trajectory tests that solve under deg3: `opts` are part of the handle (every Handle of the
# name carries them, the one the reference preconditioner is exported from included).  The small one is hex8-long and not
# hex8-saddle: at corlen 0.1 level 0 of hex8-saddle is reaction-dominated, its cycle is ONE polynomial on the level's own
# interval and no smoothing option reaches it.
SOLVE_HANDLES.update({
    "hex8-long-deg3": dict(OPTION_HANDLES["hex8-long"], problem="hex8-long", opts=_DEG3_SCHUR),
    "hex16-saddle-deg3": dict(SOLVE_HANDLES["hex16-saddle"], problem="hex16-saddle", opts=OPTION_SETS["deg3"]),
})


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


_HIER = {}


def hierarchy(mesh):
    if mesh not in _HIER:
        from parelagmc_amd.fe import box_mesh, build_hierarchy, mesh_from_json
        kind, nref = mesh
        if kind == "tet":
            m = mesh_from_json(golden_path("meshes", "cube_tet.json"))
            _HIER[mesh] = build_hierarchy(m, nref)
        else:
            n = {"hex": 4, "hex3": 3, "hex5": 5}[kind]
            _HIER[mesh] = build_hierarchy(box_mesh([n, n, n], [2, 2, 2], "hex"), nref)
    return _HIER[mesh]


_PROBLEMS = {}


def sampler_problem(name):
    """the problem of a registered handle, built once: the handles of one name (both storages, every option set) share it.
    PDESampler only reads it - the arrays are copied to the device at create time - so sharing changes nothing a handle sees"""
    name = SOLVE_HANDLES[name].get("problem", name)
    if name not in _PROBLEMS:
        from parelagmc_amd.fe import build_hybrid_sampler_problem, build_sampler_problem
        cfg = SOLVE_HANDLES[name]
        build = build_hybrid_sampler_problem if cfg["kind"] == "hybrid" else build_sampler_problem
        _PROBLEMS[name] = build(hierarchy(cfg["mesh"]), corlen=cfg["corlen"], lognormal=True, n_mc_levels=1)
    return _PROBLEMS[name]


class Handle:
    """one sampler handle with what the tests read from it; **opts: solver options beyond the storage, mg_coarsening and
    the registered handle's own `opts`.
    problem: the handle is created on this problem instead of the registered one of `name` (then only a label) - another
    layout of it, say (test_gpu_input_layouts.py); mg_coarsening 0"""

    def __init__(self, ctx, name, storage, problem=None, **opts):
        from parelagmc_amd import capi
        if problem is None:
            cfg = SOLVE_HANDLES[name]
            self.prob = sampler_problem(name)
        else:
            cfg = dict(kind="hybrid" if hasattr(problem.levels[0], "n_lambda") else "saddle", coarsening=0)
            self.prob = problem
        self.hybrid = cfg["kind"] == "hybrid"
        st = capi.PMC_STORAGE_FP64 if storage == "fp64" else capi.PMC_STORAGE_FP32
        self.opts = capi.solver_opts(precond_storage=st, mg_coarsening=cfg["coarsening"], **{**cfg.get("opts", {}), **opts})
        self.smp = capi.PDESampler(ctx, self.prob, self.opts)
        self.setup = self.smp.vcycle_setup(0)
        self.info = self.smp.vcycle_levels(0)
        self.P = [self.smp.vcycle_prolongator(0, v) for v in range(len(self.setup) - 1)]
        L = self.prob.levels[0]
        self.n = L.n_lambda if self.hybrid else L.n_u + L.n_s
        self.top = self.smp.BatchWidth(0)
        self.dense_nb = int(self.setup[0]["dense_nb"])
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            from oracle.precond_oracle import SamplerPrecondOracle
            self._oracle = SamplerPrecondOracle(self.prob, 0, self.setup, self.P, self.opts.schur_scale)
        return self._oracle

    def narrow(self, nb):
        return nb <= self.dense_nb


def darcy_fields(rng, nb, n_p):
    """one permeability per column: log-normal with variances 0.25 .. 9, k == 1, and a 1e3-contrast two-valued field"""
    k = np.empty((nb, n_p))
    for j in range(nb):
        kind = j % 6
        if kind == 1:
            k[j] = 1.0
        elif kind == 4:
            k[j] = np.where(rng.random(n_p) < 0.3, 1e3, 1.0)
        else:
            k[j] = np.exp([0.5, 1.0, 3.0, 2.0, 0.0, 1.5][kind] * rng.standard_normal(n_p))
    return k


def darcy_hex_problem(hex_hierarchy):
    """the `hex` problem of test_gpu_precond.py: the octree hierarchy, flow from x = min to x = max"""
    from parelagmc_amd.fe import build_darcy_problem
    return build_darcy_problem(hex_hierarchy, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])


def darcy_hex24_problem():
    """hex 3^3 refined three times (24^3 = 13 824 pressure rows), one MC level, the flow of darcy_hex_problem: the smallest
    octree level above the 8 192 rows a per-realization LDS tail takes"""
    from parelagmc_amd.fe import build_darcy_problem
    return build_darcy_problem(hierarchy(("hex3", 3)), [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1],
                               n_mc_levels=1)


def darcy_flat24_problem():
    """the same 24^3 cells as ONE level: the cycle is the polynomial of mg_coarse_degree / mg_coarse_ratio alone, on a level
    above the tail's 8 192 rows (cycle_bottom on kernels)"""
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy
    h = build_hierarchy(box_mesh([24, 24, 24], [2, 2, 2], "hex"), 0)
    return build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], n_mc_levels=1)

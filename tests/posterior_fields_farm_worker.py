"""One rank of a two-process farm with posterior field estimates (started by tests/test_gpu_posterior_fields.py, both ranks
on device 0): ML_BayesRatio_Manager::SetFarm with a gloo SUM all-reduce, then the collective field_stats() read.
usage: posterior_fields_farm_worker.py <rank> <out.npz> <splitting>  (RANK / WORLD_SIZE / MASTER_* from the environment)"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out, splitting = sys.argv[2], bool(int(sys.argv[3]))
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle.bayes_oracle import observation_functionals
    from parelagmc_amd import capi, host_api
    from parelagmc_amd.fe import box_mesh, build_darcy_problem, build_hierarchy, build_sampler_problem
    h = build_hierarchy(box_mesh([4, 4, 4], [2, 2, 2], "hex"), 1)
    sp = build_sampler_problem(h, corlen=0.1, lognormal=True)
    dp = build_darcy_problem(h, [0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1])
    Gobs = observation_functionals(h, np.array([[0.5, 0.5, 0.5], [1.4, 1.2, 0.6]]), eps=0.3)
    ctx = capi.Context(0, seed=99)
    smp, ds = capi.PDESampler(ctx, sp), capi.DarcySolver(ctx, dp)
    for lvl in range(2):
        ds.SetObservations(lvl, Gobs[lvl])

    def reduce(buf):
        dist.all_reduce(torch.from_numpy(buf), op=dist.ReduceOp.SUM)     # shares memory with the C buffer

    mgr = host_api.RatioManager(2, sampler=smp, solver=ds, G_obs=np.array([0.6, 0.4]), noise=0.05, wall_time=False,
                                batch=4, splitting=splitting)
    mgr.set_farm(world, rank, reduce)
    mgr.enable_field_stats(h.spaces[0].vol)
    mgr.InitRun([10, 16])
    m = mgr.field_stats()
    np.savez(out, **m)
    mgr.close()
    ds.close()
    smp.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

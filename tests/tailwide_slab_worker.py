"""Worker for tests/test_gpu_tailwide.py (one process per rank, gloo, all ranks on the box's GPU): the same z-slab run with tailwide=1 and with tailwide=0 —
gathered u and p as raw bits after every step, pois.n, Δt, the launches of every step on every rank, and the counter: both tails of every step on every rank.
usage: tailwide_slab_worker.py NXxNYxNZ STEPS"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    import waterlily_jl_amd as w  # noqa: F401
    from waterlily_jl_amd import slab
    from waterlily_jl_amd._lib import check, lib
    L = lib()
    dims = tuple(int(v) for v in sys.argv[1].split("x"))
    steps = int(sys.argv[2])
    comm = slab.CallbackComm(dist)

    def run(tw):
        sim = slab.SlabSimulation(comm, dims, (0, 0, 0), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
        for k, v in (("resjac_min", 0), ("convt_min", 0), ("tailwide", tw)):
            check(L.wl_sim_set_option(sim._h, k.encode(), v))
        fields, launches = [], []
        for _ in range(steps):
            l0 = L.wl_launch_count()
            sim.mom_step_()
            launches.append(L.wl_launch_count() - l0)
            fields.append((sim.gather_field("u", dist), sim.gather_field("p", dist)))
        cnt = C.c_long()
        check(L.wl_sim_counter(sim._h, b"tailwide", C.byref(cnt)))
        out = (fields, launches, list(sim.pois_n), [np.float32(v).view(np.uint32) for v in sim.dt], int(cnt.value))
        dist.barrier()
        del sim
        return out

    f1, l1, n1, dt1, c1 = run(1)
    f0, l0, n0, dt0, c0 = run(0)
    print(f"rank {rank}: tailwide counter {c1} (off: {c0}), launches per step {l1} vs {l0}", flush=True)
    assert c1 == 2 * steps and c0 == 0, (c1, c0)
    assert l1 == l0, (l1, l0)
    assert n1 == n0 and dt1 == dt0, (n1, n0)
    if rank == 0:
        for s, ((u1, p1), (u0, p0)) in enumerate(zip(f1, f0)):
            for name, a, b in (("u", u1, u0), ("p", p1, p0)):
                x, y = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
                assert np.array_equal(x, y), (s, name, int((x != y).sum()))
    dist.barrier()
    comm.destroy()
    print(f"rank {rank}: tailwide slabs ok", flush=True)


if __name__ == "__main__":
    main()

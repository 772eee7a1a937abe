"""Worker for tests/test_gpu_bodyset.py::test_rotating_plate_across_a_slab_boundary (one process per rank, gloo, the box's one GPU):
a rotating plate measured on z-slabs through wl_sim_measure_bodyset against the single-domain composite."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gather(sim, name, ncomp, dist):
    """the global ghosted array from every rank's owned planes (+ the physical z-ghost planes)"""
    from waterlily_jl_amd._lib import check, lib
    g = sim.grid
    loc = np.empty((g.nx, g.ny, g.nz) + ((ncomp,) if ncomp else ()), dtype=np.float32, order="F")
    check(lib().wl_d2h(loc.ctypes.data_as(C.c_void_p), lib().wl_sim_field(sim._h, name.encode()), loc.nbytes, None))
    lo = g.k0 - (1 if g.gk + g.k0 == 1 else 0)
    hi = g.k1 + (1 if g.gk + g.k1 == g.gnz - 1 else 0)
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, (g.gk + lo, np.ascontiguousarray(loc[:, :, lo:hi])))
    full = np.zeros((g.nx, g.ny, g.gnz) + loc.shape[3:], dtype=np.float32, order="F")
    for z0, a in parts:
        full[:, :, z0:z0 + a.shape[2]] = a
    return full


def main():
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    import waterlily_jl_amd as w
    from waterlily_jl_amd import slab
    dims = tuple(int(v) for v in sys.argv[1].split("x"))
    steps = int(sys.argv[2])
    c = (dims[0] / 3.0, dims[1] / 2.0, dims[2] / 2.0)           # the plate's centre on the slab boundary of two ranks
    plate = lambda th: w.Body(("capsule", (0.0, 0.0, 0.0), 2.0, (1.0, 0.0, 0.0), 6.0),     # noqa: E731
                              w.RigidMap(c, (np.float32(0.3), 0.0, np.float32(th)), omega=(0.0, 0.0, 0.125)))
    comm = slab.CallbackComm(dist)
    sim = slab.SlabSimulation(comm, dims, (1.0, 0.0, 0.0), 8.0, U=1, nu=0.02, has_body=True)
    sim.measure_bodyset_(plate(1.0))
    ref = None
    if rank == 0:
        ref = w.FusedSimulation(dims, (1.0, 0.0, 0.0), 8.0, U=1, nu=0.02, has_body=True)
        ref.set_body(plate(1.0))
    fields = {k: gather(sim, k, n, dist) for k, n in (("sigma", 0), ("mu0", 3), ("mu1", 9), ("V", 3))}
    if rank == 0:
        for k, a in fields.items():
            b = ref.field(k)
            a = a.reshape(b.shape, order="F")
            if k == "sigma":
                a, b = a[1:-1, 1:-1, 1:-1], b[1:-1, 1:-1, 1:-1]       # σ's ghosts are not written by measure!
            assert np.array_equal(a, b), k
            print(f"{k}: equal", flush=True)
    for s in range(steps):
        sim.measure_bodyset_(plate(1.0 + 0.05 * s))
        sim.mom_step_()
        u = sim.gather_field("u", dist)
        if rank == 0:
            ref.measure_bodyset_(plate(1.0 + 0.05 * s))
            ref.mom_step_()
            du = np.abs(u - ref.field("u")).max()
            print(f"step {s}: max|du|={du:.3e} n_slab={sim.pois_n[-2:]} n_ref={ref.pois_n[-2:]}", flush=True)
            assert du < 5e-5, du
    fp = sim.force_bodyset(0, plate(1.0 + 0.05 * (steps - 1)))
    if rank == 0:
        rp = ref.pressure_force_body(plate(1.0 + 0.05 * (steps - 1)))
        assert np.abs(rp).max() > 0 and np.allclose(fp, rp, rtol=1e-3, atol=1e-3 * np.abs(rp).max()), (fp, rp)
    dist.barrier()
    del sim
    comm.destroy()
    print(f"rank {rank}: bodyset_slab ok", flush=True)


if __name__ == "__main__":
    main()

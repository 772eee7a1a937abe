"""The projection tails with four cells per thread and 16-byte accesses (option "tailwide", k_project_wide in csrc/wl_project.hip): the statements per cell are
those of the one- and two-cell kernels, so a handle with tailwide=1 against a handle with tailwide=0 on the same library must agree on u, u⁰, p on every cell
(ghosts, edges, corners) as raw bits, on pois.n and on the Δt history, with the same number of launches per call — over the shapes that put the row seam inside
and outside a quad, enough blocks for the slots of the encoded maximum to wrap, the speculation switched off piecewise, folded and deferred BC! with a nonzero U on
every axis, solves that are cut short (the gated tail returns early) and z-slabs.  The counter says which tails took the new form: both tails of every step
where the shape allows it, none where it does not (plane not a whole number of quads, a body)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
UBC = (0.3, -0.2, 0.1)
# interior sizes; with ghosts: 66×34×26 (the smallest the pair tails and the fused head take; 66 ≡ 2 mod 4: every other row seam lies inside a quad),
# 72×46×20 (72 ≡ 0 mod 4: no quad straddles a row; 46 rows are no whole number of 1024-float chunks), 256×128×42 (32 chunks per plane × 42 planes = 1344 blocks:
# the 1024 slots of the encoded maximum wrap)
SMALL, MOD0, MANY = (64, 32, 24), (70, 44, 18), (254, 126, 40)


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)
    da, db = [f32(v).view(np.uint32) for v in a.dt], [f32(v).view(np.uint32) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])


def random_u(oracle, dims, seed):
    rng = np.random.default_rng(seed)
    u = np.asfortranarray(rng.uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
    oracle.BC(u, UBC)
    return u


def make(w, dims, u0, **opts):
    """u0 = None: the wall-bounded TGV (U = 0); else a random field with U ≠ 0 on every axis (folded BC! and the U substituted on load are live)"""
    if u0 is None:
        sg = w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    else:
        sg = w.FusedSimulation(dims, UBC, dims[0], U=1, nu=0.02, u0=u0)
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def run_pair(w, on, off, calls, what, per_step=2):
    for q, k in enumerate(calls):
        res = []
        for s in (on, off):
            l0, c0 = w.lib().wl_launch_count(), s.counter("tailwide")
            if k == 0:
                s.mom_step_()
            else:
                s.mom_steps_(k)
            res.append((w.lib().wl_launch_count() - l0, s.counter("tailwide") - c0))
        (lon, con), (loff, coff) = res
        print(f"{what} call {q} k={k}: tailwide counter +{con} (off: +{coff}), launches {lon} vs {loff}")
        assert coff == 0, (what, q)
        assert con == per_step * max(k, 1), (what, q, k, con)
        assert lon == loff, (what, q, "launches", lon, loff)
        assert_same_state(on, off, (what, q, k))


MODES = {
    "default": {},
    "pdefer0": {"pdefer": 0},            # every tail stores p = x/Δt (the SP = 1 instances)
    "tailspec0": {"tailspec": 0},        # no tail is gated
    "headspec0": {"headspec": 0},
    "lazydt0": {"lazydt": 0},
    "bcdefer0": {"bcdefer": 0},          # u_in's boundary faces are read from memory
    "redo": {"resjac": 2},               # every head redone: the gated tail is withheld on every solve and launched after the read
    "store_f": {"store_f": 1},           # σ = flux_out is materialised
    "bcfold0": {"bcfold": 0},            # BC! as launches of its own: no folded stores
}


@pytest.mark.parametrize("dims", [SMALL, MOD0], ids=["66x34x26", "72x46x20"])
@pytest.mark.parametrize("mode", list(MODES))
def test_tailwide_is_bit_identical(w, oracle, mode, dims):
    u0 = random_u(oracle, dims, 211)
    on, off = make(w, dims, u0, tailwide=1, **MODES[mode]), make(w, dims, u0, tailwide=0, **MODES[mode])
    run_pair(w, on, off, (1, 2, 5, 0), mode)
    if mode == "redo":
        assert on.counter("tailspec") == 0 and on.counter("tailspec_armed") > 0
    if mode == "default":
        assert max(on.pois_n) >= 2, on.pois_n      # the random field needs several V-cycles on its first solves


@pytest.mark.parametrize("dims", [SMALL, MOD0, MANY], ids=["66x34x26", "72x46x20", "256x128x42"])
def test_tailwide_on_the_taylor_green_vortex(w, dims):
    """U = 0, the benchmark's flow; the large shape has more blocks than the encoded maximum has slots"""
    on, off = make(w, dims, None, tailwide=1), make(w, dims, None, tailwide=0)
    run_pair(w, on, off, (1, 2, 5) if dims != MANY else (1, 3), dims)


@pytest.mark.parametrize("itmx", [1, 2])
def test_tailwide_when_the_gated_tail_returns_early(w, oracle, itmx):
    """solver!'s cap below what the first solves of the random field need: the gated tail queued behind the last V-cycle finds the break test failed and returns
    at once (the maximum's slots keep −∞, nothing is stored), the host launches the tail again after its read"""
    u0 = random_u(oracle, SMALL, 71)
    on, off = make(w, SMALL, u0, tailwide=1, itmx=itmx), make(w, SMALL, u0, tailwide=0, itmx=itmx)
    run_pair(w, on, off, (0, 0, 2, 3), f"itmx={itmx}")
    armed, stood = on.counter("tailspec_armed"), on.counter("tailspec")
    print(f"itmx={itmx}: tailspec_armed {armed}, tailspec {stood}")
    assert armed - stood >= 1, (armed, stood)


def test_tailwide_stands_down(w, oracle):
    """a plane that is not a whole number of quads (66 × 35 floats), and a body (coefficients read from μ₀): the one- and two-cell kernels run, the counter stays 0"""
    dims = (64, 33, 24)
    u0 = random_u(oracle, dims, 223)
    on, off = make(w, dims, u0, tailwide=1), make(w, dims, u0, tailwide=0)
    run_pair(w, on, off, (2, 0), dims, per_step=0)

    N, R = 32, 4.0
    sims = []
    for tw in (1, 0):
        sg = w.FusedSimulation((N, N, N), (1, 0, 0), 2 * R, U=1, nu=2 * R / 3700, has_body=True)
        sg.set_option("tailwide", tw)
        sg.measure_sphere_((N / 2,) * 3, R, 1.0)
        for _ in range(3):
            sg.mom_step_()
        assert sg.counter("tailwide") == 0
        sims.append(sg)
    assert_same_state(sims[0], sims[1], "sphere")


@pytest.mark.parametrize("mode", ["default", "store_f", "pdefer0"])
def test_tailwide_when_the_maximum_slots_wrap_on_a_random_field(w, oracle, mode):
    """1344 blocks on 1024 slots of the encoded maximum, with U ≠ 0 (folded BC!, U substituted on load), σ materialised, p stored"""
    u0 = random_u(oracle, MANY, 227)
    on, off = make(w, MANY, u0, tailwide=1, **MODES[mode]), make(w, MANY, u0, tailwide=0, **MODES[mode])
    run_pair(w, on, off, (2, 0), f"many-{mode}")


@pytest.mark.parametrize("n,dims", [(2, "128x64x64"), (3, "192x48x96"), (4, "64x32x96")])
def test_tailwide_on_z_slabs_is_bit_identical(n, dims):
    """z-slabs call the same launchers with their own k0/k1/gk and nz ≠ gnz: P ranks on the box's GPU run the same steps with tailwide=1 and tailwide=0
    (tests/tailwide_slab_worker.py) — gathered u, p as raw bits, pois.n, Δt, launches per step, and the counter on every rank (2 per step)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + (os.getpid() % 400)), os.path.join(root, "tests", "tailwide_slab_worker.py"), dims, "3"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for q in range(n):
        assert f"rank {q}: tailwide slabs ok" in r.stdout

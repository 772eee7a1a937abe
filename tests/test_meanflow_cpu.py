"""The mean-flow observer without a GPU: the new entry points are declared alike in include/wlhip.h and _lib.py, packing UU's upper triangle loses nothing
in the restatement of tests/meanflow_ref.py, and the shapes and Δt histories of tests/test_gpu_meanflow.py hold what they were chosen for."""
import os
import re

import numpy as np
import pytest

import meanflow_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wl_sim_set_meanflow": 5, "wl_sim_meanflow_reset": 3, "wl_sim_meanflow_update": 2, "wl_sim_meanflow": 3, "wl_sim_meanflow_uu": 4, "wl_sim_meanflow_t": 3}
f32 = np.float32


def _decls():
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(wl_\w+)\s*\(([^;{]*?)\)\s*;", hdr)}


def test_abi_surface():
    from waterlily_jl_amd import _lib
    decl = _decls()
    for name, arity in NEW.items():
        assert decl.get(name) == arity, (name, decl.get(name))
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    bench = open(os.path.join(ROOT, "include", "wlhip_bench.h"), encoding="utf-8").read()
    for cnt in ("mean_updates", "mean_every"):
        assert f'"{cnt}"' in bench, cnt
    mk = open(os.path.join(ROOT, "waterlily.jl_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "wl_meanflow.hip" in mk


def test_python_surface_and_argument_validation():
    from waterlily_jl_amd import simulation as sm
    for name in ("set_meanflow", "reset_meanflow", "update_meanflow", "meanflow", "meanflow_uu", "load_meanflow_"):
        assert callable(getattr(sm.FusedSimulation, name)), name

    class H:      # set_meanflow validates before the library is reached
        D, _h = 3, None
    with pytest.raises(ValueError):
        sm.FusedSimulation.set_meanflow(H(), True, every=0)


@pytest.mark.parametrize("D", [2, 3])
def test_the_lower_triangle_is_the_upper_one_bit_for_bit(D):
    Ng = (7, 6, 5)[:D]
    rng = np.random.default_rng(D)
    m = mr.MeanRef(Ng, 0.0, True)
    t = f32(0)
    for k in range(20):
        u = rng.normal(size=Ng + (D,)).astype(f32) * f32(10.0 ** rng.integers(-3, 4))
        p = rng.normal(size=Ng).astype(f32)
        t = f32(t + f32(rng.uniform(0.01, 0.5)))
        m.update(p, u, t)
    for i in range(D):
        for j in range(i):
            assert np.array_equal(m.UU[..., i, j].view(np.uint32), m.UU[..., j, i].view(np.uint32)), (i, j)
    assert np.array_equal(mr.expand(mr.pack(m.UU), D).view(np.uint32), m.UU.view(np.uint32))
    tau = m.uu()
    assert np.array_equal(mr.expand(mr.pack(tau), D).view(np.uint32), tau.view(np.uint32))      # τ is symmetric in the same way


@pytest.mark.parametrize("D", [2, 3])
def test_packed_expanded_packed_is_the_identity(D):
    rng = np.random.default_rng(10 + D)
    packed = np.asfortranarray(rng.normal(size=(5, 4, 3)[:D] + (mr.npk(D),)).astype(f32))
    full = mr.expand(packed, D)
    assert full.shape[-2:] == (D, D)
    assert np.array_equal(mr.pack(full), packed)
    planes = sorted(mr.pk(i, j) for j in range(D) for i in range(j + 1))
    assert planes == list(range(mr.npk(D))) and mr.npk(D) == (3, 6)[D - 2]
    assert all(mr.pk(i, j) == mr.pk(j, i) for i in range(D) for j in range(D))
    assert [mr.pk(i, j) for j in range(2) for i in range(j + 1)] == [0, 1, 2]      # the 2-D planes are the first three of the 3-D ones


def test_gpu_shapes_reach_every_path_of_the_kernel():
    cs = [mr.cells(d) for d in mr.SHAPES]
    assert all(mr.levels(d) >= 3 for d in mr.SHAPES), "every shape can carry a handle"
    assert all(mr.levels(d) < 3 for d in mr.NO_HANDLE) and [mr.cells(d) for d in mr.NO_HANDLE] == [63, 2048, 693, 768]
    # three levels need an even side, so cs is even on every handle: of cs % 4 = 0, 1, 2, 3 only 0 and 2 exist there, and both are covered
    for dims in [(a, b) for a in range(3, 40) for b in range(3, 40)] + [(a, b, c) for a in range(3, 20) for b in range(3, 20) for c in range(3, 20)]:
        assert mr.levels(dims) < 3 or mr.cells(dims) % 2 == 0, dims
    assert {c % 4 for c in cs} == {0, 2}, cs
    per_group = mr.BLOCK * mr.CELLS_PER_THREAD
    assert any(c % 4 == 0 and c < per_group for c in cs), "a 16-byte case below one workgroup"
    assert any(c % 4 == 0 and c > per_group and c % per_group != 0 for c in cs), "a 16-byte case of several workgroups with a ragged last one"
    assert any(c % 4 == 0 and c % per_group == 0 for c in cs), "a 16-byte case of whole workgroups"
    assert any(c % 4 != 0 and c > mr.BLOCK for c in cs) and any(c % 4 != 0 and c < mr.BLOCK for c in cs), "one-cell cases above and below one workgroup"
    for D, shapes in ((2, mr.SHAPES_2D), (3, mr.SHAPES_3D)):
        res = {mr.cells(d) % 4 == 0 for d in shapes}
        assert all(len(d) == D for d in shapes) and res == {True, False}, (D, "both forms in this dimension")
    assert all(d in mr.SHAPES for d in [(6, 8), (8, 8, 8), (64, 32, 24)])


def test_the_weights_of_the_gpu_histories_lie_strictly_inside_0_1():
    assert len(mr.DT_HISTORY) == mr.N_UPDATES and all(d > 0 for d in mr.DT_HISTORY)
    assert len({float(d) for d in mr.DT_HISTORY}) == mr.N_UPDATES, "a varying Δt"
    ts = mr.times(mr.DT_HISTORY)
    m = mr.MeanRef((3, 3), 0.0, False)
    es = []
    for t in ts:
        es.append(m.weight(t)[1])
        m.t.append(f32(m.t[-1] + m.weight(t)[0]))
    assert es[0] == 1.0 and all(0.0 < e < 1.0 for e in es[1:]), es
    assert [float(v) for v in m.t[1:]] == [float(v) for v in ts]
    # an observer that updates every third step of the same history (the reference's user calling update! every three steps)
    m3 = mr.MeanRef((3, 3), 0.0, False)
    e3 = []
    for t in ts[2::3]:
        e3.append(m3.weight(t)[1])
        m3.t.append(f32(m3.t[-1] + m3.weight(t)[0]))
    assert e3[0] == 1.0 and all(0.0 < e < 1.0 for e in e3[1:]), e3

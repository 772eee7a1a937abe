"""The force band without a GPU: the geometry matrix of tests/forces_ref.py holds the classes it was chosen for, skipped tiles contribute exactly nothing
in the restatement, the forces the GPU comparisons will see are far above their tolerance, and the new entry points are declared alike in
include/wlhip.h and _lib.py and validate their arguments in Python."""
import os
import re

import numpy as np
import pytest

import forces_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wl_sim_set_force_record": 4, "wl_sim_read_forces": 5, "wl_sim_forces_bodyset": 5}
# the closed-form body the oracle develops a flow around, where the case's own body is not one it knows
STAND_IN = {"rotated_set": ("sphere", (30.2, 15.7, 11.6), 4.0)}


@pytest.mark.parametrize("name", list(fr.CASES))
def test_geometry_holds_its_class(name):
    c = fr.case(name)
    active, nt, nb, mask = fr.band(c["body"], c["Ng"])
    assert all(a <= b for a, b in zip(sorted(c["dims"], reverse=True), (64, 32, 24)))
    assert (len(active) > 0) == c["nonempty"], (name, len(active))
    assert (len(active) < nt) == c["skips"], (name, len(active), nt)
    assert (nb > 0) == c["nonempty"]
    assert list(active) == sorted(active)
    if name == "floor":          # every tile of the slab of tile rows the plane's band crosses
        tid, _ = fr.tile_index(c["Ng"])
        rows = np.unique((tid // -(-c["Ng"][0] // 64)) % -(-c["Ng"][1] // 4))
        hit_rows = np.unique((active // -(-c["Ng"][0] // 64)) % -(-c["Ng"][1] // 4))
        assert len(hit_rows) < len(rows) and len(active) == len(hit_rows) * (nt // len(rows))
    if name == "ragged_48x20x12":
        assert (c["Ng"][1] % 4, c["Ng"][2] % 4) != (0, 0) and c["Ng"][0] % 64 != 0
        ty, tz = active % 6, active // 6          # one tile in x, six rows of tiles, four planes of tiles
        assert ty.max() == 5 or tz.max() == 3, "the body reaches a ragged last tile"


def _oracle_fields(c, name, steps=3):
    from oracle import oracle as orc
    orc.build()
    body = STAND_IN[name] if name in STAND_IN else c["body"].shape
    so = orc.Simulation(c["dims"], c["uBC"], c["L"], U=1, nu=c["nu"], perdir=c["perdir"], body=body, T=np.float32)
    for _ in range(steps):
        so.step(remeasure=False)
    return so, so.p.copy(order="F"), so.u.copy(order="F")


@pytest.mark.parametrize("name", [n for n in fr.CASES if n != "outside"])
def test_skipped_tiles_add_nothing_and_the_force_is_far_above_the_tolerance(name):
    c = fr.case(name)
    so, p, u = _oracle_fields(c, name)
    _, _, nb, mask = fr.band(c["body"], c["Ng"])
    t = fr.terms(c["body"], p, u, c["nu"], c["x0"])
    assert np.all(t[:, ~mask] == 0.0), "a cell of a skipped tile contributes"
    full, banded = fr.sums(c["body"], p, u, c["nu"], c["x0"]), fr.sums(c["body"], p, u, c["nu"], c["x0"], mask=mask)
    assert np.array_equal(full, banded)
    tol = fr.tolerances(c["body"], p, u, c["nu"], c["x0"])
    D = len(c["dims"])
    pF = full[:D]
    if name not in STAND_IN:         # the oracle has this force: the restatement is the same sum
        ref = so.pressure_force()
        assert np.allclose(pF, ref, rtol=1e-4, atol=1e-6 * np.abs(ref).max()), (pF, ref)
        pF = ref
    print(f"[forces cpu] {name}: n_b {nb}, |pF| {np.linalg.norm(pF):.3e}, tol {tol[0]:.3e}")
    assert np.linalg.norm(pF) >= 100 * tol[0], (name, pF, tol)


def test_outside_body_has_no_band():
    c = fr.case("outside")
    active, nt, nb, mask = fr.band(c["body"], c["Ng"])
    assert len(active) == 0 and nb == 0 and not mask.any() and nt > 0


def _decls():
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(wl_\w+)\s*\(([^;{]*?)\)\s*;", hdr)}


def test_abi_surface():
    from waterlily_jl_amd import _lib
    decl = _decls()
    for name, arity in NEW.items():
        assert decl.get(name) == arity, (name, decl.get(name))
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    bench = open(os.path.join(ROOT, "include", "wlhip_bench.h"), encoding="utf-8").read()
    for cnt in ("force_records", "force_dropped", "force_tiles"):
        assert f'"{cnt}"' in bench, cnt


def test_python_argument_validation():
    from waterlily_jl_amd import simulation as sm
    from waterlily_jl_amd.bodies import Body
    leaf = sm._as_set(("sphere", (1.0, 2.0, 3.0), 2.0))
    assert isinstance(leaf, Body) and leaf.shape[0] == "sphere" and leaf.program(3).n == 1
    b = Body(("sphere", (1.0, 2.0), 2.0))
    assert sm._as_set(b) is b
    with pytest.raises(TypeError):
        sm._as_set(3.0)
    with pytest.raises(ValueError):
        sm._x0_checked((1.0, 2.0), 3)
    assert sm._x0_checked(None, 3) is None and list(sm._x0_checked((1.0, 2.0), 2)) == [1.0, 2.0, 0.0]
    rec = np.arange(24, dtype=np.float64).reshape(2, 12)
    pF, vF, pM, vM = sm._split_forces(rec, 2)
    assert pF.shape == (2, 2) and pM.shape == (2, 1) and vM[1, 0] == 21 and vF[0, 1] == 4
    pF, vF, pM, vM = sm._split_forces(rec, 3)
    assert pM.shape == (2, 3) and list(vM[0]) == [9, 10, 11]

    class H:      # set_force_record validates before the library is reached
        D, _h = 3, None
    with pytest.raises(ValueError):
        sm.FusedSimulation.set_force_record(H(), b, capacity=0)

"""Composite bodies without a GPU: RigidMap's rotation, the postfix encoding of set expressions, the ctypes/C/Julia layouts of
wl_rigid_map / wl_body_node / wl_bodyset, and the binding's new methods (reference: src/RigidMap.jl, src/Body.jl:91-107,
test/test_bodies.jl:54-107)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import waterlily_jl_amd as wl
from waterlily_jl_amd import bodies
from waterlily_jl_amd._lib import SIGNATURES, wl_body_node, wl_bodyset, wl_rigid_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "waterlily.jl_amd", "julia", "WaterLilyHIPExt.jl")
RTOL = float(np.sqrt(np.finfo(np.float32).eps))


def test_rotation_2d_matches_the_reference_formula():
    for th in (0.0, np.pi / 2, np.pi, 0.3, -1.2):
        R = bodies.rotation(th)
        assert R.dtype == np.float32 and R.shape == (2, 2)
        c, s = np.cos(np.float32(th)), np.sin(np.float32(th))
        assert np.array_equal(R, np.array([[c, s], [-s, c]], dtype=np.float32))
        assert np.allclose(R @ R.T, np.eye(2), atol=1e-6)
    assert np.allclose(bodies.rotation(np.pi / 2), [[0, 1], [-1, 0]], atol=1e-6)
    assert np.allclose(bodies.rotation(np.pi), [[-1, 0], [0, -1]], atol=1e-6)


def test_rotation_3d_euler_angles():
    assert np.allclose(bodies.rotation([np.pi, 0, 0]), np.diag([1, -1, -1]), atol=1e-6)    # 180° about x
    assert np.allclose(bodies.rotation([0, np.pi, 0]), np.diag([-1, 1, -1]), atol=1e-6)    # 180° about y
    assert np.allclose(bodies.rotation([0, 0, np.pi]), np.diag([-1, -1, 1]), atol=1e-6)    # 180° about z
    assert np.allclose(bodies.rotation([0, 0, np.pi / 2]), [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-6)
    for th in ([0.1, -0.4, 0.7], [1.0, 2.0, 3.0]):
        R = bodies.rotation(th)
        assert R.dtype == np.float32 and np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.isclose(np.linalg.det(R), 1, atol=1e-6)
        # RigidMap.jl:50-53 restated in float64
        t1, t2, t3 = th
        ref = [[np.cos(t3) * np.cos(t2), np.cos(t3) * np.sin(t2) * np.sin(t1) + np.sin(t3) * np.cos(t1), -np.cos(t3) * np.sin(t2) * np.cos(t1) + np.sin(t3) * np.sin(t1)],
               [-np.sin(t3) * np.cos(t2), -np.sin(t3) * np.sin(t2) * np.sin(t1) + np.cos(t3) * np.cos(t1), np.sin(t3) * np.sin(t2) * np.cos(t1) + np.cos(t3) * np.sin(t1)],
               [np.sin(t2), -np.cos(t2) * np.sin(t1), np.cos(t2) * np.cos(t1)]]
        assert np.allclose(R, ref, rtol=RTOL, atol=1e-6)


def _ops(prog):
    return [(prog.node[i].op, prog.node[i].kind) for i in range(prog.n)]


def test_set_expressions_encode_to_postfix():
    a, b, c = (bodies.Body(("sphere", (0, 0), r)) for r in (1, 2, 3))
    L, U, I, N = bodies.OP_LEAF, bodies.OP_UNION, bodies.OP_INTERSECT, bodies.OP_NEGATE
    assert _ops((a | b).program(2)) == [(L, 1), (L, 1), (U, 0)]
    assert _ops((a + b).program(2)) == [(L, 1), (L, 1), (U, 0)]
    assert _ops((a & b).program(2)) == [(L, 1), (L, 1), (I, 0)]
    assert _ops((-a).program(2)) == [(L, 1), (N, 0)]
    assert _ops((a - b).program(2)) == [(L, 1), (L, 1), (N, 0), (I, 0)]
    assert _ops(((a | b) & c).program(2)) == [(L, 1), (L, 1), (U, 0), (L, 1), (I, 0)]
    assert _ops((a | (b & c)).program(2)) == [(L, 1), (L, 1), (L, 1), (I, 0), (U, 0)]
    p = ((a | b) - c).program(2)
    assert [p.node[i].R for i in range(p.n) if p.node[i].op == L] == [1, 2, 3]
    cap = bodies.Body(("capsule", (1, 2), 2, (1, 0), 6)).program(2)
    assert cap.n == 1 and cap.node[0].kind == bodies.CAPSULE and cap.node[0].h == 6 and list(cap.node[0].m) == [1, 0, 0]
    cyl = bodies.Body(("cylinder", (1, 2, 3), 2, 2)).program(3)
    assert list(cyl.node[0].m) == [1, 1, 0] and cyl.node[0].mapped == 0


def test_setmap_reaches_every_leaf():
    """test/test_bodies.jl:89-93"""
    sdf = ("sphere", (0, 0), 1)
    body = bodies.Body(sdf, bodies.RigidMap((0, 0), 0)) + bodies.Body(sdf, bodies.RigidMap((1, 1), 0))
    body = bodies.setmap(body, theta=np.pi / 4, V=(1.0, 0))
    a, b = bodies.leaves(body)
    assert a.map.theta == b.map.theta == np.float32(np.pi / 4)
    assert np.allclose(a.map.V, [1, 0]) and np.allclose(b.map.V, [1, 0])
    assert np.array_equal(a.map.R, bodies.rotation(np.float32(np.pi / 4)))
    assert list(a.map.x0) == [0, 0] and list(b.map.x0) == [1, 1]
    p = body.program(2)
    for i in (0, 1):
        assert p.node[i].mapped == 1 and np.allclose(list(p.node[i].map.R)[:2], a.map.R[0]) and list(p.node[i].map.V)[:2] == [1, 0]
    with pytest.raises(ValueError):
        bodies.setmap(bodies.Body(sdf), theta=1.0)        # no map to set


def test_program_limits_raise():
    leaf = bodies.Body(("sphere", (0, 0), 1))
    b = leaf
    for _ in range(8):
        b = b | leaf
    with pytest.raises(ValueError, match="nodes"):
        b.program(2)                                        # 9 leaves + 8 unions = 17 nodes
    deep = leaf
    for _ in range(8):
        deep = leaf | deep                                  # right-deep: the stack grows with every leaf
    with pytest.raises(ValueError):
        deep.program(2)
    right = leaf
    for _ in range(7):
        right = leaf | right                                # 8 leaves + 7 unions = 15 nodes, stack 8: fits
    assert right.program(2).n == 15
    # (a stack deeper than 8 needs 9 leaves, i.e. more than 16 nodes in any well-formed program: the C validation of raw
    # programs covers it, tests/test_gpu_bodyset.py::test_malformed_programs_launch_nothing)


def _c_layout():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "wlhip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("wl_rigid_map %zu\nwl_body_node %zu\nwl_bodyset %zu\n", sizeof(wl_rigid_map), sizeof(wl_body_node), sizeof(wl_bodyset));
  F(wl_rigid_map, x0); F(wl_rigid_map, xp); F(wl_rigid_map, R); F(wl_rigid_map, V); F(wl_rigid_map, w);
  F(wl_body_node, op); F(wl_body_node, kind); F(wl_body_node, c); F(wl_body_node, R); F(wl_body_node, m); F(wl_body_node, h);
  F(wl_body_node, mapped); F(wl_body_node, map); F(wl_bodyset, n); F(wl_bodyset, node);
  printf("WL_BODYSET_MAX %d\nWL_BODYSET_STACK %d\n", WL_BODYSET_MAX, WL_BODYSET_STACK);
  return 0;
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return dict(line.rsplit(" ", 1) for line in out.strip().split("\n"))


def test_ctypes_layout_equals_the_c_layout():
    lay = _c_layout()
    assert int(lay["wl_rigid_map"]) == C.sizeof(wl_rigid_map)
    assert int(lay["wl_body_node"]) == C.sizeof(wl_body_node)
    assert int(lay["wl_bodyset"]) == C.sizeof(wl_bodyset)
    for T, name in ((wl_rigid_map, "wl_rigid_map"), (wl_body_node, "wl_body_node"), (wl_bodyset, "wl_bodyset")):
        for f, _ in T._fields_:
            assert int(lay[f"{name}.{f}"]) == getattr(T, f).offset, (name, f)
    assert int(lay["WL_BODYSET_MAX"]) == bodies.WL_BODYSET_MAX and int(lay["WL_BODYSET_STACK"]) == bodies.WL_BODYSET_STACK
    assert C.sizeof(wl_bodyset) < 4096 - 256            # passed by value as a kernel argument


def _header_struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            out += [re.sub(r"[\*\s]|\[\w+\]", "", n) for n in stmt.split(None, 1)[1].split(",")]
    return out


def test_julia_mirrors_match_the_header():
    src = open(JL, encoding="utf-8").read()
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    for jl, c in (("WlRigidMap", "wl_rigid_map"), ("WlBodyNode", "wl_body_node"), ("WlBodySet", "wl_bodyset")):
        m = re.search(r"struct %s; (.*?) end" % jl, src)
        assert m, jl
        fields = [f.split("::")[0].strip() for f in m.group(1).split(";") if f.strip()]
        assert fields == _header_struct_fields(hdr, c), (jl, fields)
    assert C.sizeof(wl_bodyset) == 4 + 16 * C.sizeof(wl_body_node)


def test_binding_defines_the_bodyset_methods():
    src = open(JL, encoding="utf-8").read()
    assert re.search(r"struct HipRigidBody\{[^}]*\} <: AbstractBody\n\s*shape::Union\{HipBody,HipCapsule\}\n\s*map::", src)
    for sig in ("function measure!(a::HFlow{D}, body::DeviceSet; ",
                "function WaterLily.pressure_force(p::HA, df::HA, body::DeviceSet, ",
                "function WaterLily.viscous_force(u::HA, ν, df::HA, body::DeviceSet, ",
                "function WaterLily.pressure_moment(x₀, p::HA, df, body::DeviceSet, ",
                "function WaterLily.viscous_moment(x₀, u::HA, ν, df, body::DeviceSet, "):
        assert sig in src, sig
    for sym in ("wl_measure_bodyset", "wl_pressure_force_bodyset", "wl_viscous_force_bodyset"):
        assert f"(:{sym}, libwlhip)" in src, sym


def test_bodyset_symbols_are_bound():
    for sym in ("wl_bodyset_measure_points", "wl_measure_bodyset", "wl_pressure_force_bodyset", "wl_viscous_force_bodyset",
                "wl_sim_measure_bodyset", "wl_sim_pressure_force_bodyset", "wl_sim_viscous_force_bodyset"):
        assert sym in SIGNATURES
    assert wl.Body is bodies.Body and wl.RigidMap is bodies.RigidMap and wl.setmap is bodies.setmap

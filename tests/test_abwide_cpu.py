"""The slot map of the pair smoother's exchange buffer W (csrc/wl_abwide.hpp): the one function kernel A, kernel B and this test share, compiled here as plain
C++.  A row of W holds one 512-byte segment per core column of kernel A (60 cells = 30 pairs in slots 0..29 of 32); every pair of a row must land in a slot of
its own, 16-byte aligned, inside the row pitch, never in a padding slot, and the segments must start on multiples of 512 bytes."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = """
#include "wl_abwide.hpp"
extern "C" unsigned t_pitch(int nx) { return wl::abw_pitch(nx); }
extern "C" unsigned t_slot(int i0) { return wl::abw_slot(i0); }
extern "C" int t_segments(int nx) { return wl::abw_segments(nx); }
"""


@pytest.fixture(scope="module")
def slotmap(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler (the one the oracle is built with)"
    d = tmp_path_factory.mktemp("abwide")
    (d / "slot.cpp").write_text(SRC)
    so = d / "libslot.so"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "waterlily.jl_amd", "csrc"), str(d / "slot.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    for f in (L.t_pitch, L.t_slot):
        f.restype = C.c_uint
    return L


@pytest.mark.parametrize("nx", [34, 62, 66, 122, 258, 514])
def test_every_pair_of_a_row_has_a_slot_of_its_own(slotmap, nx):
    pitch, nseg = slotmap.t_pitch(nx), slotmap.t_segments(nx)
    assert nseg == -(-(nx - 1) // 60) and pitch == 512 * nseg      # kernel A's tile columns (ptile<2,2>: 60 core cells), one segment each
    pairs = list(range(0, nx - 1, 2))                                # i0 even in [0, nx−2]
    slots = [slotmap.t_slot(i0) for i0 in pairs]
    assert len(set(slots)) == len(pairs)
    for i0, o in zip(pairs, slots):
        assert o % 16 == 0 and o + 16 <= pitch, (i0, o)
        seg, k = divmod(o, 512)
        assert seg == i0 // 60 and k // 16 == (i0 % 60) // 2, (i0, o)      # segment = the tile column whose core holds the pair; slot = the pair's place in that core
        assert k // 16 < 30, (i0, o)                                        # slots 30 and 31 are padding
    # the last segment holds what is left: a single pair at nx = 62
    assert sum(1 for o in slots if o // 512 == nseg - 1) == len(pairs) - 30 * (nseg - 1)
    if nx == 62:
        assert [o for o in slots if o // 512 == 1] == [512]

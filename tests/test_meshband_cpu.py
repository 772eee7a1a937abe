"""Band-limited mesh baking without a GPU (tests/meshband_ref.py): that the cases of tests/test_gpu_meshband.py hold what they are there for — the far-brick
counts pinned, every far brick of one sign and wholly beyond the band in the Float32 restatement, clipped samples inside searched bricks, far bricks on both
sides of the surface where a case promises them — that clip_ref is the full restatement inside the band, and that mesh_band sits a quarter cell above the
band rule of include/wlhip.h."""
import os

import numpy as np
import pytest

import meshband_ref as mb

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sides(name):
    band = mb.BAND[name]
    d = mb.full_ref(name)
    far = mb.far_bricks(name, band)
    out = inside = mixed = inband = 0
    for sl, f in zip(mb.bricks(name), far):
        if not f:
            continue
        blk = d[sl]
        inband += int((np.abs(blk) <= f32(band)).sum())
        if (blk > 0).all():
            out += 1
        elif (blk < 0).all():
            inside += 1
        else:
            mixed += 1
    return out, inside, mixed, inband


@pytest.mark.parametrize("name", mb.CASES)
def test_far_bricks_are_pinned_one_signed_and_beyond_the_band(name):
    out, inside, mixed, inband = _sides(name)
    assert mixed == 0 and inband == 0, (name, mixed, inband)
    if name in mb.FAR:
        assert (out, inside) == mb.FAR[name], (name, out, inside)
    else:                                                          # the small 2-D cases: bricks are 4×16, at most one lies beyond the band
        assert inside == 0 and out <= 1, (name, out, inside)
    if name in mb.INSIDE:
        assert out > 0 and inside > 0
    # the slack only ever removes bricks
    assert mb.far_bricks(name, mb.BAND[name], 2.0).sum() <= out + inside <= mb.far_bricks(name, mb.BAND[name], 0.0).sum()


@pytest.mark.parametrize("name", mb.CASES)
def test_searched_bricks_hold_clipped_samples_and_the_clip_is_the_full_field_inside_the_band(name):
    band = f32(mb.BAND[name])
    d, far = mb.full_ref(name), mb.far_bricks(name, mb.BAND[name], 0.0)
    clipped_in_searched = sum(int((np.abs(d[sl]) > band).sum()) for sl, f in zip(mb.bricks(name), far) if not f)
    assert clipped_in_searched > 0, name                         # the per-sample clip has work in every case
    c = mb.clip_ref(name, mb.BAND[name])
    inb = np.abs(d) <= band
    assert inb.any() and np.array_equal(c[inb].view(np.uint32), d[inb].view(np.uint32))
    assert np.array_equal(c[~inb].view(np.uint32), np.where(d[~inb] < 0, -band, band).astype(f32).view(np.uint32))


def test_the_velocity_mask_keeps_the_band_and_zeroes_the_rest():
    import meshvel_ref as mv
    name = "ico320"
    c = mb.case(name)
    Wv = mv.linear(c["V"])
    d, W = mb.clip_ref(name, mb.BAND[name], Wv)
    inb = np.abs(mb.full_ref(name)) <= f32(mb.BAND[name])
    assert not W[~inb].view(np.uint32).any() and np.abs(W[inb]).max() > 0.1
    assert np.array_equal(d.view(np.uint32), mb.clip_ref(name, mb.BAND[name]).view(np.uint32))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("spacing", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("offset", [0.0, 0.75, -1.5])
@pytest.mark.parametrize("eps", [1.0, 2.0])
def test_mesh_band_satisfies_the_rule_and_a_quarter_less_does_not(D, spacing, offset, eps):
    b = mb.mesh_band(eps, offset, spacing, D)
    need = 2.0 + eps + 1.0
    assert mb.band_rule(b, offset, need, spacing, D)
    assert mb.band_rule(b, offset, 2.0, spacing, D)              # the force calls ask less
    assert not mb.band_rule(b - 0.25 - 1e-5, offset, need, spacing, D)


def test_the_package_states_the_same_band():
    import waterlily_jl_amd.bodies as bodies
    for D in (2, 3):
        for sp in (0.5, 1.0, 2.0):
            assert bodies.mesh_band(1.5, -0.5, sp, D) == mb.mesh_band(1.5, -0.5, sp, D)
    assert bodies.mesh_band() == 2 + 1 + 1 + 3 ** 0.5 + 0.25


def test_the_header_declares_the_calls_with_hip_stream():
    h = open(os.path.join(ROOT, "include", "wlhip.h")).read()
    hb = open(os.path.join(ROOT, "include", "wlhip_bench.h")).read()
    assert "wl_sdf_lattice_from_mesh_band(" in h and "float band, unsigned flags, void* hip_stream);" in h
    assert "float wl_sdf_lattice_band(const wl_sdf_lattice* lattice);" in h
    assert "int wl_meshsdf_last_bricks(uint64_t* searched, uint64_t* skipped);" in hb
    assert "band − |R| > need + s·√D" in h and "BAKING" in h

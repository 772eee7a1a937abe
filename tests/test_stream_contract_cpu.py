"""Every entry point of include/wlhip.h that takes a `stream` has a stream-contract scenario in tests/test_gpu_streams.py: a leaf in its LEAF table, a
handle call in a `step("wl_...")` of a handle scenario — or stands in EXCLUDED with a reason.  Declaring a new entry point without a scenario fails here,
and so does removing a table row.  No GPU needed: the header and the test module are read, nothing is launched."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# only what cannot work on one GPU may stand here (include/wlhip.h: the RCCL communicator with more than one rank and its second communicator);
# neither takes a stream today, so nothing of the header is excluded
EXCLUDED = {
    "wl_comm_rccl_create": "more than one rank needs more than one GPU (RCCL refuses two ranks on one device)",
    "wl_comm_rccl_add_async": "collective over the ranks of wl_comm_rccl_create",
}
HANDLE_PREFIXES = ("wl_mg_", "wl_sim_")


def header_stream_functions():
    src = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = []
    for m in re.finditer(r"\b(?:int|float|double|size_t|wl_grid|float\s*\*|wl_mg\s*\*|const\s+char\s*\*)\s+(wl_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        if "typedef" in src[max(0, m.start() - 40):m.start()].splitlines()[-1]:
            continue
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def scenarios():
    import test_gpu_streams as t          # importing it launches nothing and needs no device
    src = open(os.path.join(ROOT, "tests", "test_gpu_streams.py"), encoding="utf-8").read()
    return set(t.LEAF_NAMES), set(re.findall(r"\bstep\(\s*\"(wl_\w+)\"", src))


def test_the_header_parses():
    fns = header_stream_functions()
    assert len(fns) == len(set(fns)) and len(fns) >= 80, len(fns)
    for must in ("wl_fill", "wl_cfl", "wl_mg_solve", "wl_sim_mom_steps", "wl_flow_stats", "wl_bodyset_measure_points", "wl_comm_halo_async", "wl_h2d"):
        assert must in fns, must
    assert "wl_mg_create" not in fns and "wl_sim_create" not in fns      # handle creation takes no stream (Conventions: default stream, returns finished)


def test_every_stream_entry_point_has_a_scenario():
    leaves, handle_calls = scenarios()
    missing = []
    for fn in header_stream_functions():
        if fn in EXCLUDED:
            continue
        if fn.startswith(HANDLE_PREFIXES):
            if fn not in handle_calls:
                missing.append(fn + " (no handle scenario calls it in a step)")
        elif fn not in leaves:
            missing.append(fn + " (no row in LEAF)")
    assert not missing, "entry points with a `stream` parameter and no stream scenario: " + ", ".join(missing)


def test_scenarios_name_real_entry_points_and_exclusions_stay_minimal():
    leaves, handle_calls = scenarios()
    fns = set(header_stream_functions())
    assert not (leaves | handle_calls) - fns, sorted((leaves | handle_calls) - fns)
    assert set(EXCLUDED) <= {"wl_comm_rccl_create", "wl_comm_rccl_add_async"}
    assert all(EXCLUDED.values())

"""Compile-time guard of the straight-line code at the two ends of a fused-loss wave (CPU test: hipcc cross-compiles
gfx950 without a GPU).  tests/test_isa_guard.py pins the scene loops; nothing there looks at what runs before the first
loop and after the last, which is where three serialisations were taken out (rendering_loss_body, svbrdf_device.h):

  * the launch's scalars are fetched together at wave entry: one `s_waitcnt lgkmcnt(0)` between wave entry and the first
    plane load of the by-value headline kernel (SVBRDF_K3_ENTRY_FETCH);
  * render 0's scene row is requested in front of the plane loads: no scalar load between the wait for the planes and
    the first geometry (SVBRDF_K3_EARLY_SCENE);
  * the wave sum uses lane swaps and DPP rotations: no ds_bpermute (SVBRDF_K3_DPP_SUM).

Each figure is compared with the same unit compiled in the same test run with the three switches off -- which is the
code from before the change -- and none of them may move a scene loop: same loops, same counts per trip.
"""
import os
import sys

import pytest

import unit_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs /opt/rocm/bin/hipcc (cross-compiles gfx950)")
HEADLINE = "k_rendering_loss_inlILb1ELb0ELb0"
SWITCHES_OFF = ["-DSVBRDF_K3_ENTRY_FETCH=0", "-DSVBRDF_K3_EARLY_SCENE=0", "-DSVBRDF_K3_DPP_SUM=0"]


def _compile_unit1(tmp, extra):
    return unit_build.compile_unit_asm(tmp, "svbrdf_k3_adjoint", "SCHED_ADJOINT", extra)


def _facts(text):
    """the straight-line facts of the by-value headline kernel, and its loops"""
    import isa_stats
    _, meta, whole, loops, ins, rng = isa_stats.analyse(text, HEADLINE)
    code = [(mn, ops) for _, _, mn, ops in ins]
    first_loop = min(a for a, _ in rng)
    planes = [i for i, (mn, _) in enumerate(code[:first_loop]) if mn and mn.startswith("buffer_load_dword")]
    assert len(planes) == 24, len(planes)
    entry_waits = sum(1 for mn, ops in code[:planes[0]] if mn == "s_waitcnt" and "lgkmcnt" in ops)
    # the wait that has every plane: the first `vmcnt(0)` behind the last plane load; the first geometry: the first v_rsq_f32
    landed = next(i for i in range(planes[-1], len(code)) if code[i][0] == "s_waitcnt" and "vmcnt(0)" in code[i][1])
    geometry = next(i for i in range(landed, len(code)) if code[i][0] and code[i][0].startswith("v_rsq_f32"))
    assert geometry < first_loop
    late_loads = sum(1 for mn, _ in code[landed:geometry] if mn and mn.startswith(("s_load", "s_buffer_load")))
    return {"entry_waits": entry_waits, "late_scalar_loads": late_loads,
            "bpermute": sum(1 for mn, _ in code if mn and mn.startswith("ds_bpermute")),
            "before_first_loop": first_loop, "after_last_loop": len(code) - 1 - max(b for _, b in rng),
            "vgprs": int(meta["NumVgprs"]), "scratch": int(meta["ScratchSize"]) + whole["scratch"], "loops": loops}


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa_ends")
    new, old = _facts(_compile_unit1(tmp, [])), _facts(_compile_unit1(tmp, SWITCHES_OFF))
    for k in ("entry_waits", "late_scalar_loads", "bpermute", "before_first_loop", "after_last_loop", "vgprs", "scratch"):
        print("%-20s switches off %4d   this build %4d" % (k, old[k], new[k]))
    return new, old


def test_scalars_are_awaited_once_before_the_first_plane_load(facts):
    new, old = facts
    # (switches off: S, the grid width, ws and the plane pointers cost one round trip each)
    assert new["entry_waits"] == 1 and new["entry_waits"] < old["entry_waits"], (new["entry_waits"], old["entry_waits"])


def test_no_scalar_load_between_the_planes_and_the_first_geometry(facts):
    new, old = facts
    # (switches off: render 0's scene row, and eps with 1/N, are fetched behind the plane wait)
    assert new["late_scalar_loads"] == 0 and new["late_scalar_loads"] < old["late_scalar_loads"], (new["late_scalar_loads"], old["late_scalar_loads"])


def test_wave_sum_leaves_the_lds_pipe(facts):
    new, old = facts
    # (switches off: the butterfly, one ds_bpermute_b32 per level)
    assert new["bpermute"] == 0 and new["bpermute"] < old["bpermute"]
    assert new["after_last_loop"] < old["after_last_loop"], (new["after_last_loop"], old["after_last_loop"])


def test_the_scene_loops_did_not_move(facts):
    """none of the three may be paid for inside a loop: the same two loops with the same instruction counts per trip,
    still 128 VGPRs at most and no scratch"""
    new, old = facts
    assert new["vgprs"] <= 128 and new["scratch"] == 0, new
    assert len(new["loops"]) == len(old["loops"]) == 2
    for a, b in zip(new["loops"], old["loops"]):
        for k in ("total", "valu", "trans", "salu", "smem", "vmem", "lds", "scratch", "waitcnt"):
            assert a[k] == b[k], (k, a, b)

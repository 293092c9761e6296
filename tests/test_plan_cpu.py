"""The rig plan's path and launch-shape rules (x_maps_amd/csrc/host/xm_plan.hpp: which kernels a frame or a group takes -- K0 / K0b /
none, the K1 variant, K2 tiled or pipelined, a captured group's redo on the device -- and the grid, block and dynamic LDS of every
launch) built alone with AddressSanitizer and UBSan.  tests/c_host/plan_host.cpp states, as literals worked out from the rules
as they stood before they had a header of their own: the paths and every launch shape of the benchmark's two rigs (C-1M in
projector view, the ESL-like owner-tile rig; their plans as xm_create builds them on an MI355X, profiles/plan_identity.md) for a
lone frame, groups of 2, 8 and 60, a captured group and the compact paths paused; and hand-built plans just below and at every
threshold of the rules.  Host code only: no GPU."""
import os
import subprocess

from test_k2_live_host_cpu import FLAGS, ROOT, _gxx_with_asan


def test_paths_and_launch_shapes_under_address_and_ub_sanitizers(tmp_path):
    gxx = _gxx_with_asan(tmp_path)
    exe = tmp_path / "plan_host"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok"

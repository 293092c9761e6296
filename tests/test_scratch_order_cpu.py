"""The ordering record of a handle's per-entry scratch (x_maps_amd/csrc/host/xm_scratch_order.hpp: the end-of-call event, the
stream of the call in flight, the dirty note of scratch that must be zero between calls) and the ingest rings' entry / tag arithmetic
(x_maps_amd/csrc/host/xm_ring_tag.hpp), built alone with AddressSanitizer and UBSan.  tests/c_host/scratch_order_host.cpp gives the
record an ops type that appends every call to a trace and compares the exact traces with what xm_process_time_surfaces,
xm_frames_to_time_surfaces, xm_frames_to_point_clouds and the two table setters did by hand before: first call, same stream again,
another stream, growth while in flight, a synchronous call, a table rewrite while in flight, a dirty note behind a failing call.
The ring's functions are held against literals: entry index, both tags, "tag names seq", a lapped entry, seq + 1 at 2^62 - 1.
Host code only: no GPU."""
import os
import subprocess

from test_k2_live_host_cpu import FLAGS, ROOT, _gxx_with_asan


def test_exact_call_traces_and_ring_tags_under_address_and_ub_sanitizers(tmp_path):
    gxx = _gxx_with_asan(tmp_path)
    exe = tmp_path / "scratch_order_host"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "scratch_order_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok"

"""A slot's ordering record (x_maps_amd/csrc/host/xm_slot_order.hpp: where the slot's last work ran, and the only code that
makes a stream or the host wait for it) built alone with AddressSanitizer and UBSan.  tests/c_host/slot_order_host.cpp gives it
an ops type that appends every call to a trace and compares the exact traces with what the call sites did by hand before:
group then frame on another / the same stream, eager work then a group, both records, the group-only variant, a capture, the
set form of a graph replay (one join per distinct dirty stream), the host wait, forget, a second identical call, a failing call.
Host code only: no GPU."""
import os
import subprocess

from test_k2_live_host_cpu import FLAGS, ROOT, _gxx_with_asan


def test_exact_call_traces_under_address_and_ub_sanitizers(tmp_path):
    gxx = _gxx_with_asan(tmp_path)
    exe = tmp_path / "slot_order_host"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "slot_order_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok"

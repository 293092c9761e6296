"""The agreement among a sharded handle's device threads (x_maps_amd/csrc/host/xm_agree.hpp: the host barrier in front of every
collective that hands all of them the first error, and that a thread leaving elsewhere poisons) built alone with ThreadSanitizer
and stressed by tests/c_host/agree_stress.cpp with 1, 2, 4 and 8 threads: all ranks fine, one code, two different codes in one
round, a rank that leaves while its peers wait, an arrival behind the poison, reset() and a clean round.  Host code only: no GPU."""
import os
import subprocess

from test_host_queue_cpu import FLAGS, ROOT, _gxx_with_tsan


def test_agreement_under_thread_sanitizer(tmp_path):
    gxx = _gxx_with_tsan(tmp_path)
    exe = tmp_path / "agree_stress"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "agree_stress.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)  # (a lost wake-up hangs)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok"

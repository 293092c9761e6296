"""The host threads' hand-over (x_maps_amd/csrc/host/xm_queue.hpp: the job queue of the launch workers and of the ingest's
copy, launch and out threads, the first-error latch) built alone with ThreadSanitizer and stressed by
tests/c_host/queue_stress.cpp: order, no lost job or wake-up, wait_done on work and on an error, one error with its own text
when two threads fail at once, and the out side's form of the queue -- a producer that runs some of the jobs itself and posts
them as done.  Host code only: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread"]


def _gxx_with_tsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx] + FLAGS + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ without -fsanitize=thread")
    return gxx


def test_job_queue_and_first_error_under_thread_sanitizer(tmp_path):
    gxx = _gxx_with_tsan(tmp_path)
    exe = tmp_path / "queue_stress"
    subprocess.run([gxx] + FLAGS + [os.path.join(ROOT, "tests", "c_host", "queue_stress.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)  # (a lost wake-up hangs)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok"

"""The in-place decision of the streaming queue (lightning_amd/csrc/host_ranges.h): a column queued with lamd_queue_*_batch_inplace crosses the
bus from the caller's memory only if ONE range registered with lamd_host_register holds all of it -- adjacent registrations, overlapping ones, a
pageable hole, an unregistered range and registrations from several threads, checked on the host (the GPU tests never queue a partly pinned
column: an asynchronous copy from such memory has hung the runtime)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_column_stays_in_place_only_inside_one_registered_range(tmp_path):
    exe = str(tmp_path / "host_ranges_test")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "lightning_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "host_ranges_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)

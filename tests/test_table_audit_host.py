"""lightning_amd/csrc/table_audit.h on the host under AddressSanitizer and UBSan (tests/c/table_audit_host.cpp, a stand-alone program with 4-bit
G-table windows): the table and every replacement image are heap blocks of exactly their size, and the audit of every range at every window boundary
and at both ends of the table reads nothing outside them.  lamd_debug_gtable_audit runs the same index arithmetic on the device; what the audit
decides is tested in tests/test_devmath_host.py (8- and 11-bit windows) and tests/test_gpu_tables.py (the shipped 24)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_audit_reads_stay_inside_the_table_and_the_image(tmp_path):
    exe = str(tmp_path / "table_audit_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DLAMD_GTABLE_WINDOW_BITS=4",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "table_audit_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr[-4000:])
    assert int(r.stdout.split()[1]) > 64 * 16 * 10

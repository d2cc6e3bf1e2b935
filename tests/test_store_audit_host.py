"""lightning_amd/csrc/store_audit.h on the host, under AddressSanitizer and UBSan: the CRC-32C the device computes (4- and 8-way slicing) against
the bitwise definition for every length 0..70 at every start alignment 0..7 and for a 65 535-byte buffer, the scid index, and the walk over
truncated, zero-filled and garbage-length files -- the file is untrusted input, every read must stay inside it (tests/c/store_audit_host.cpp,
a stand-alone program: the buffers it hands over are heap blocks of exactly the file's size)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crc_index_and_walk_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "store_audit_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "store_audit_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)

"""tests/kc_layout_host.cpp: the key-table stages through the interleaved scratch views against the flat layout, word for word, as a stand-alone
program under AddressSanitizer and UBSan (CPU only)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_interleaved_views_build_the_same_tables(tmp_path):
    exe = str(tmp_path / "kc_layout_host")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "kc_layout_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "32 cases, 0 mismatches" in r.stdout, r.stdout[-2000:]

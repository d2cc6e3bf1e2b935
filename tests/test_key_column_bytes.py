"""The size of a caller's key column (lightning_amd/csrc/key_column.h): key i lies at pub + i * pubstride and publen bytes of it are read, so a
column of n keys is (n - 1) * pubstride + publen bytes long -- the entry points that stage a key column (lamd_verify_ecdsa_batch,
lamd_pubkey_parse_batch, lamd_check_tx_sig_batch, lamd_check_tx_sig_tx_batch) used to copy n * pubstride bytes, past the end of a column that is
the last field of an array of structs.  Checked on the host, in a stand-alone program under AddressSanitizer and UBSan: the values, the
overflow report, and a copy of exactly that size out of a heap block that ends with the last key."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_key_column_ends_with_its_last_key(tmp_path):
    exe = str(tmp_path / "key_column_bytes_test")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "key_column_bytes_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)

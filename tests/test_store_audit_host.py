"""lightning_amd/csrc/store_audit.h on the host, under AddressSanitizer and UBSan: the CRC-32C the device computes (4- and 8-way slicing) against
the bitwise definition for every length 0..70 at every start alignment 0..7 and for a 65 535-byte buffer, the scid index, and the walk over
truncated, zero-filled and garbage-length files -- the file is untrusted input, every read must stay inside it (tests/c/store_audit_host.cpp,
a stand-alone program: the buffers it hands over are heap blocks of exactly the file's size); and the audit of the stores the reference ships
(test_reference_stores.py) with the signature verdicts handed in, whose offsets, signers and verdicts must equal test_store_audit.model's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_audit") / "store_audit_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_audit_host.cpp")])
    return path


def test_crc_index_and_walk_under_the_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def signers_and_signature_verdicts(orc, blob):
    """per record what the model looks a channel_update's signer up as (33 zero bytes: none, and for every other record) and what the oracle says
    of the record's signatures (0 for a record that has none)"""
    recs = sa.walk(blob)[0]
    first = {}
    for i, r in enumerate(recs):
        if not r[1] & sa.F_DELETED and sa._cann_scid(r[4]):
            first.setdefault(sa._cann_scid(r[4])[0], i)
    signer, sigv = [], []
    for i, (_, flags, _, _, m) in enumerate(recs):
        t = 0 if flags & sa.F_DELETED else int.from_bytes(m[:2], "big")
        who = bytes(33)
        if t == 258 and len(m) >= 112:
            a = first.get(int.from_bytes(m[98:106], "big"))
            if a is not None and a < i:
                o = sa._cann_scid(recs[a][4])[1] + 33 * (m[111] & 1)
                if len(recs[a][4]) >= o + 33:
                    who = recs[a][4][o:o + 33]
        signer.append(who)
        sigv.append(orc.sigcheck_channel_announcement(m) if t == 256 else orc.sigcheck_node_announcement(m) if t == 257 else
                    orc.sigcheck_channel_update(m, who if who != bytes(33) else sa.G33) if t == 258 else 0)
    return signer, sigv


@pytest.mark.parametrize("name", ["part1", "mainnet", "fixed", "canned"])
def test_host_audit_of_the_stores_the_reference_ships_equals_the_model(exe, tmp_path, orc, name):
    blob = rs.store(name)
    off, verdicts, s = sa.model(orc, blob)
    signer, sigv = signers_and_signature_verdicts(orc, blob)
    (tmp_path / "image").write_bytes(blob)
    (tmp_path / "sigv").write_bytes(np.array(sigv, dtype=np.int8).tobytes())
    r = subprocess.run([exe, str(tmp_path / "image"), str(tmp_path / "sigv"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda ext, dt: np.frombuffer((tmp_path / ("out." + ext)).read_bytes(), dtype=dt)
    assert [int(x) for x in arr("off", "<u8")] == off and [int(x) for x in arr("verdict", np.int8)] == verdicts
    ids = (tmp_path / "out.signer").read_bytes()
    assert [ids[33 * i:33 * i + 33] for i in range(len(off))] == signer and sum(1 for x in signer if x != bytes(33)) >= 2
    assert [int(x) for x in arr("walk", "<u8")] == [s["records"], s["live"], s["deleted"], s["end_offset"], 0] and s["end_reason"] == "eof"
    want = rs.COUNTS[name]
    assert (len(verdicts), {k: verdicts.count(k) for k in set(verdicts)}) == want[:2]

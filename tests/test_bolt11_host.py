"""lightning_amd/csrc/bolt11.h on the host, under AddressSanitizer and UBSan (tests/c/bolt11_host.cpp, a stand-alone program: the string and every
output column of a row are heap blocks of exactly their size): the per-string functions that k_bolt11_front and k_checkmessage_front run must
give the status so far, the hash, the signature bytes, the recovery id and the key that the sequential model (tests/text_sig_model.py) gives --
on every string the reference's tests hold (tests/golden/text_signatures.json), on every proper prefix of one of them, and on every synthesised
class.  The expectations the reference's own asserts pin, and the curve work behind the front end, are checked over the model here too, so that
the pinned table holds without a GPU; the device side of the same calls is tests/test_gpu_text_signatures.py."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_sig_model as M  # noqa: E402

ROOT = M.ROOT
KEY_310 = "03e7156ae33b0a208d0744199163177e909e80176e55d97a2f221ede0f934dd9ad"      # common/test/run-bolt11.c:310
HASH_KAT_B11 = "116fdb0f18352c886deb263f6466eb40e5e6518b80231a1f9df86088bfa48043"   # tests/golden/make_golden.py KAT-B11 (:465-467)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bolt11") / "bolt11_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path,
                           os.path.join(ROOT, "tests", "c", "bolt11_host.cpp")])
    return path


def _run(exe, d, mode, blob, width):
    d.mkdir()
    (d / "in").write_bytes(blob)
    r = subprocess.run([exe, mode, str(d / "in"), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-4000:])
    out = (d / "out").read_bytes()
    assert len(out) % width == 0
    return [out[k:k + width] for k in range(0, len(out), width)]


def host_bolt11(exe, d, strings):
    rows = _run(exe, d, "bolt11", struct.pack("<I", len(strings)) + b"".join(struct.pack("<I", len(s)) + s for s in strings), 132)
    assert len(rows) == len(strings)
    return [dict(status=struct.unpack("b", o[:1])[0], hash=o[1:33], sig=o[33:97], recid=o[97], key=o[98:131], have_n=bool(o[131])) for o in rows]


def host_messages(exe, d, pairs):
    blob = struct.pack("<I", len(pairs)) + b"".join(struct.pack("<I", len(m)) + m + struct.pack("<I", len(z)) + z for m, z in pairs)
    rows = _run(exe, d, "msg", blob, 98)
    assert len(rows) == len(pairs)
    return [dict(status=struct.unpack("b", o[:1])[0], hash=o[1:33], sig=o[33:97], recid=o[97]) for o in rows]


def ref_invoices():
    fx = M.fixture()
    return {r["line"]: r["str"].encode() for r in fx["invoices"] + fx["other_strings"]}


def test_front_end_equals_the_model_on_the_reference_strings_and_their_prefixes(exe, tmp_path):
    inv = ref_invoices()
    strings = list(inv.values()) + [inv[491][:k] for k in range(len(inv[491]))]
    got = host_bolt11(exe, tmp_path / "r", strings)
    for s, g in zip(strings, got):
        assert g == M.bolt11_front(s), s[:40]
    # row 7 of the pinned table: no proper prefix passes the front end
    assert all(g["status"] < 0 for g in got[len(inv):])
    # row 8: the signing data of KAT-B11
    by = dict(zip(strings, got))
    assert HASH_KAT_B11 in {g["hash"].hex() for g in got}
    # row 6: the upper-case string and its lower-case twin
    assert by[inv[520]]["status"] == 0 and by[inv[520]] == host_bolt11(exe, tmp_path / "l", [inv[520].lower()])[0]


def test_front_end_equals_the_model_on_every_synthesised_invoice(exe, tmp_path):
    rows = M.synth_invoices()
    got = host_bolt11(exe, tmp_path / "r", [s for _, s, _ in rows])
    for (name, s, _), g in zip(rows, got):
        assert g == M.bolt11_front(s), name
    # the front end alone already gives every status up to -5 that the rows expect (the `n` key's validity comes behind it)
    for (name, s, want), g in zip(rows, got):
        if want is not None and -5 <= want <= -1 and not name.startswith(("n/off-curve", "n/prefix04")):
            assert g["status"] == want, name


def test_front_end_equals_the_model_on_every_message_row(exe, tmp_path):
    fx = M.fixture()
    rows, _ = M.synth_messages()
    pairs = [(m, M._b(z)) for _, m, z, _ in rows] + [(t["message"].encode(), t["zbase"].encode()) for t in fx["checkmessage"]]
    got = host_messages(exe, tmp_path / "r", pairs)
    for (m, z), g in zip(pairs, got):
        assert g == M.checkmessage_front(m, z), (m[:20], z[:20])
    for (name, _, _, want), g in zip(rows, got):
        if want is not None and -3 <= want <= -1:
            assert g["status"] == want, name


def test_the_model_gives_what_the_reference_asserts():
    """the pinned table over the model itself (curve work by the C oracle and, again, by the big-integer one)"""
    fx = M.fixture()
    inv = ref_invoices()
    lines = [r["line"] for r in fx["invoices"]]
    for curve in ("orc", "pyref"):
        st, node, h, hn = M.bolt11_check([inv[ln] for ln in lines], curve)
        by = {ln: (int(s), bytes(k).hex()) for ln, s, k in zip(lines, st, node)}
        ok = [ln for ln in lines if by[ln][0] == 0]
        assert len(ok) == 26 and sum(by[ln][1] == KEY_310 for ln in ok) == 24                      # row 1
        assert by[495][0] == -1 and by[856][0] == -1 and by[870][0] == -1                          # rows 1, 2
        assert by[877][0] == -6 and by[884][0] == -3                                               # rows 3, 4
        assert by[689] == (0, KEY_310) and not hn[lines.index(689)]                                # row 5: wrong-length `n` fields, recovery
        assert not hn.any()
    assert M.bolt11_check([inv[863]])[0][0] == -1
    trip = fx["checkmessage"]
    st, node = M.checkmessage([t["message"] for t in trip], [t["zbase"] for t in trip], "pyref")
    assert list(st) == [0] * len(trip) and [bytes(k).hex() for k in node] == [t["pubkey"] for t in trip]     # row 9
    st2, node2 = M.checkmessage([t["message"] + "modified" for t in trip], [t["zbase"] for t in trip], "pyref")
    for t, s, k in zip(trip, st2, node2):                                                          # row 10
        assert s == -4 or (s == 0 and bytes(k).hex() != t["pubkey"])


def test_every_synthesised_row_has_the_status_its_construction_says():
    rows = M.synth_invoices()
    st = M.bolt11_check([s for _, s, _ in rows])[0]
    for (name, _, want), got in zip(rows, st):
        assert want is None or got == want, (name, want, got)
    assert {int(x) for x in st} == set(range(-7, 1))
    mrows, pub = M.synth_messages()
    mst, node = M.checkmessage([m for _, m, _, _ in mrows], [z for _, _, z, _ in mrows])
    for (name, _, _, want), got, k in zip(mrows, mst, node):
        assert want is None or got == want, (name, want, got)
        if name.startswith("len/"):
            assert bytes(k) == pub
    assert {int(x) for x in mst} == set(range(-4, 1))

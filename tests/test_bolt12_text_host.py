"""lightning_amd/csrc/bolt12_text.h on the host, under AddressSanitizer and UBSan (tests/c/bolt12_text_host.cpp, a stand-alone program: the string,
the decode scratch and every output column of a row are heap blocks of exactly their size): the per-string function that k_bolt12_text_front runs
must give the status so far, the kind, the key, the signature, the tagged hash and the two ids that the sequential model
(tests/bolt12_text_model.py) gives before key validity and the curve -- on every string of tests/golden/bolt12_strings.json (the reference-held
ones and the fuzz sample), on every proper prefix of one reference invoice, and on every synthesised class.  What is pinned about the
reference-held strings is checked over the model here too, so that it holds without a GPU; the device side of the same call is
tests/test_gpu_bolt12_text.py."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bolt12_text_model as M  # noqa: E402

ROOT = M.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bolt12") / "bolt12_text_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path,
                           os.path.join(ROOT, "tests", "c", "bolt12_text_host.cpp")])
    return path


def host_front(exe, d, strings):
    d.mkdir()
    (d / "in").write_bytes(struct.pack("<I", len(strings)) + b"".join(struct.pack("<I", len(s)) + s for s in strings))
    r = subprocess.run([exe, str(d / "in"), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-4000:])
    out = (d / "out").read_bytes()
    assert len(out) == 196 * len(strings)
    rows = [out[k:k + 196] for k in range(0, len(out), 196)]
    return [dict(status=struct.unpack("b", o[:1])[0], kind=o[1], have_key=bool(o[2]), key=o[3:36], sig=o[36:100], sighash=o[100:132], offer_id=o[132:164],
                 invreq_id=o[164:196]) for o in rows]


def _same(exe, d, strings, names=None):
    got = host_front(exe, d, strings)
    for k, (s, g) in enumerate(zip(strings, got)):
        assert g == M.bolt12_front(s), names[k] if names else s[:60]
    return got


def test_front_end_equals_the_model_on_every_fixture_string(exe, tmp_path):
    fx = M.fixture()
    strings = sorted({M._b(r["str"]) for r in fx["strings"]}) + [M._b(r["str"]) for r in fx["fuzz"]]
    got = _same(exe, tmp_path / "r", strings)
    assert {g["status"] for g in got} == set(range(-7, 1)) and {g["kind"] for g in got} == {0, 1, 2, 3}
    # an upper-cased reference string and its lower-case twin
    inv = next(M._b(r["str"]) for r in fx["strings"] if r["str"].startswith("lni1"))
    up, low = host_front(exe, tmp_path / "u", [inv.upper(), inv])
    assert up == low and up["status"] == 0


def test_front_end_equals_the_model_on_every_proper_prefix_of_a_reference_invoice(exe, tmp_path):
    inv = min((M._b(r["str"]) for r in M.fixture()["strings"] if r["str"].startswith("lni1")), key=len)
    got = _same(exe, tmp_path / "r", [inv[:k] for k in range(len(inv))])
    assert all(g["status"] < 0 for g in got)


def test_front_end_equals_the_model_on_every_synthesised_class(exe, tmp_path):
    rows = M.synth()
    got = _same(exe, tmp_path / "r", [s for _, s, _ in rows], [name for name, _, _ in rows])
    # the front end alone already gives every status down to -7 that the rows expect, but for the keys that are no curve points
    for (name, _, want), g in zip(rows, got):
        if want is not None and -7 <= want <= -1 and not name.startswith(("key/invreq-off", "key/invoice-off", "key/invreq-prefix", "key/invoice-prefix",
                                                                         "key/invreq-x=p", "key/invoice-x=p")):
            assert g["status"] == want, name
    got = _same(exe, tmp_path / "b", M.random_batch(300, 5))
    assert len({g["status"] for g in got}) >= 4


def test_the_model_gives_what_is_pinned_about_the_reference_strings():
    """the counts and the recorded ids, over the model itself (curve work by the C oracle and, again, by the big-integer one)"""
    fx = M.fixture()
    for curve in ("orc", "pyref"):
        p = M.pinned(fx, lambda strings: M.bolt12_check(strings, curve))
        assert (p["ok_invoices"], p["ok_invreqs"], p["ok_offers"]) == (7, 2, 7)
        assert p["no_key_invreqs"] == ["tests/test_pay.py"]
        assert p["offers_with_offer_id"] >= 3 and p["invoices_with_offer_id"] >= 3
        assert p["invreqs_with_invreq_id"] >= 2 and p["invoices_with_invreq_id"] >= 1
    assert sum("offer_id" in r for r in fx["strings"]) >= 6 and sum("invreq_id" in r for r in fx["strings"]) >= 2
    assert len(fx["fuzz"]) <= 24 * 4 * 9 and all(len(r["str"]) <= 1200 for r in fx["fuzz"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bolt12_strings.json")) < 200 * 1000


def test_every_synthesised_row_has_the_status_its_construction_says():
    rows = M.synth()
    st, kind = M.bolt12_check([s for _, s, _ in rows])[:2]
    for (name, _, want), got in zip(rows, st):
        assert want is None or got == want, (name, want, got)
    assert {int(x) for x in st} == set(range(-8, 1)) and {int(k) for k in kind} == {0, 1, 2, 3}
    # an id over two empty spans is SHA-256 of nothing
    by = {name: s for name, s, _ in rows}
    f = M.bolt12_front(by["span/invoice-nothing-inside"])
    assert f["status"] == 0 and f["offer_id"] == M.EMPTY_ID and f["invreq_id"] == M.EMPTY_ID
    f = M.bolt12_front(by["span/invoice-high-invreq-fields-only"])
    assert f["offer_id"] == M.EMPTY_ID and f["invreq_id"] != M.EMPTY_ID
    assert M.bolt12_front(b"lno1")["offer_id"] == M.EMPTY_ID

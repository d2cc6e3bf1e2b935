"""lightning_amd/csrc/store_digest.h on the host, under AddressSanitizer and UBSan (tests/c/store_digest_host.cpp, a stand-alone program: every buffer it
hands over is a heap block of exactly its size): the program's own checks of bigsize, limits, searches, split corners and parser rules; and the digest
of the golden stores, of the synthetic store (with and without verdicts), of its damaged copy and of hand-built stores, built stage by stage in file
order, in reverse and in a scrambled order of the records (the program compares the three itself), which must equal the sequential model of
channel_range_model -- as must the bytes of the replies to every query set, written at all four alignments of the output.  The device side of the same
calls, lamd_gossip_store_digest_build and lamd_channel_range_reply_batch, is test_channel_range's.  Last, the stores and vectors the reference ships
(test_reference_stores): the mainnet excerpt, the canned store, the two query vectors and the two update checksums."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_digest") / "store_digest_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_digest_host.cpp")])
    return path


def test_bigsize_limits_searches_split_and_parser_under_the_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def host_answers(exe, d, blob, verdict, queries, cap, chain=crm.CHAIN):
    """-> (digest entries, counters, status, [[reply bytes]]) as the host build of the header computes them"""
    d.mkdir()
    (d / "image").write_bytes(blob)
    if verdict is not None:
        (d / "verdicts").write_bytes(np.array(verdict, dtype=np.int8).tobytes())
    (d / "queries").write_bytes(struct.pack("<I", len(queries)) + b"".join(struct.pack("<I", len(q)) + q for q in queries))
    (d / "chain").write_bytes(chain)
    r = subprocess.run([exe, str(d / "image"), str(d / "verdicts") if verdict is not None else "-", str(d / "queries"), str(d / "chain"), str(cap), str(d / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    raw = (d / "out.digest").read_bytes()
    n = struct.unpack_from("<I", raw)[0]
    entries = []
    for j in range(n):
        scid, t0, t1, c0, c1, r0, r1, r2 = struct.unpack_from("<QIIIIIII", raw, 4 + 36 * j)
        entries.append((scid, (t0, t1), (c0, c1), (r0, r1, r2)))
    names = ("records", "channels", "entries", "channels_no_update", "updates_no_channel", "updates_in_front", "updates_short")
    counters = dict(zip(names, struct.unpack("<7Q", (d / "out.counters").read_bytes())))
    status = list(np.frombuffer((d / "out.status").read_bytes(), dtype=np.int8))
    first = np.frombuffer((d / "out.first").read_bytes(), dtype="<u8")
    off = np.frombuffer((d / "out.msgoff").read_bytes(), dtype="<u8")
    out = (d / "out.bytes").read_bytes()
    replies = [[out[int(off[j]):int(off[j + 1])] for j in range(int(first[q]), int(first[q + 1]))] for q in range(len(queries))]
    return entries, counters, status, replies


def check_against_model(exe, d, blob, verdict, queries, cap, chain=crm.CHAIN):
    want, wc = crm.sorted_digest(blob, verdict)
    entries, counters, status, replies = host_answers(exe, d, blob, verdict, queries, cap, chain)
    assert entries == want and counters == wc
    for k, q in enumerate(queries):
        ws, wr = crm.replies(want, chain, q, cap)
        assert (status[k], replies[k]) == (ws, wr), (k, q.hex(), status[k], ws, len(replies[k]), len(wr))
    return want


@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_host_digest_and_replies_of_the_golden_stores_equal_the_model(exe, tmp_path, name):
    blob = sa._golden(name)
    blocks = [e[0] >> 40 for e in crm.digest(blob)[0]]
    for k, cap in enumerate((0, 8, 24)):
        want = check_against_model(exe, tmp_path / str(k), blob, None, crm.query_kinds(blocks), cap)
        assert [e[0] for e in want] == sorted(e[0] for e in want) and len(want) == len(blocks)


def test_host_digest_of_the_synthetic_store_and_its_damaged_copy(exe, tmp_path, synthetic, damaged):
    img, (_, v, _) = synthetic
    blocks = [e[0] >> 40 for e in crm.digest(img)[0]]
    assert len(blocks) >= 12
    qs = crm.query_kinds(blocks)
    plain = check_against_model(exe, tmp_path / "plain", img, None, qs, 0)
    assert check_against_model(exe, tmp_path / "verdicts", img, list(v), qs, 16) == plain     # every live record of it is OK
    blob, (_, dv, _), _ = damaged
    good = check_against_model(exe, tmp_path / "damaged", blob, list(dv), qs, 0)
    loose = check_against_model(exe, tmp_path / "flags", blob, None, qs, 56)
    assert good != loose                                                                      # bad records are not served


def test_host_slot_cases_and_splits(exe, tmp_path):
    blob, names = crm.slot_store()
    want = check_against_model(exe, tmp_path / "slots", blob, None, crm.query_kinds([s >> 40 for s in names.values()]), 0)
    by = {e[0]: e for e in want}
    assert names["no_update"] not in by and by[names["replaced"]][1] == (8000, 0) and by[names["short"]][1] == (0, 51)
    for limit in (1, 2, 3, 7):
        pops = [p for p in (1, limit - 1, limit, limit + 1, 3 * limit + 1) if p]
        store = crm.population_store(pops)
        blocks = [100 + 3 * k for k in range(len(pops))]
        check_against_model(exe, tmp_path / ("split%d" % limit), store, None, crm.query_kinds(blocks), 8 * limit)
    for k, scids in enumerate(([], [crm.scid_of(7)], [crm.scid_of(9 - b, b) for b in range(5)])):
        check_against_model(exe, tmp_path / ("few%d" % k), crm.channel_store(scids, both=bool(k & 1)), None, crm.query_kinds([7]), 0)


def test_host_parser_cases(exe, tmp_path):
    """every status the parser gives, expected by hand and by the model: a 72-byte query cut at every length; bigsize forms; type order; unknown types;
    the option values"""
    long_q = crm.query(crm.CHAIN, 5, 9, 3, b"\x03\x02\xaa\xbb" + b"\x05\x15" + bytes(21))
    assert len(long_q) == 72
    cases = [(long_q[:k], 0 if k in (42, 45, 49) else -1) for k in range(72)] + [(long_q, 0)]
    Q = lambda tlvs: crm.query(crm.CHAIN, 5, 9, None, tlvs)
    cases += [(Q(b"\x01\x03\xfd\x00\x03"), -1), (Q(b"\xfd\x00\x01\x01\x03"), -1), (Q(b"\x01\xfd\x00\x01\x03"), -1), (Q(b"\x01\x01\xfc"), 0),   # non-minimal bigsize
              (Q(b"\x03\x00\x01\x01\x03"), -1), (Q(b"\x01\x01\x03\x01\x01\x03"), -1), (Q(b"\x01\x01\x03\x03\x00"), 0),                        # descending, twice
              (Q(b"\x02\x00"), -1), (Q(b"\x00\x00"), -1), (Q(b"\x01\x01\x03\xfd\x01\x00\x00"), -1),                                          # unknown even
              (Q(b"\x03\x00"), 0), (Q(b"\xfd\x01\x01\x01\x07"), 0), (Q(b"\x01\x01\x01\xff" + bytes([0, 0, 0, 1, 0, 0, 0, 1]) + b"\x00"), 0)]  # unknown odd
    cases += [(crm.query(crm.CHAIN, 5, 9, v), 0) for v in list(range(8)) + [0x100, 0xfd, 0x10003, 1 << 40]]
    cases += [(crm.query(crm.FOREIGN, 5, 9, 3), 1), (crm.query(crm.FOREIGN, 5, 9, None, b"\x02\x00"), -1)]
    blob = crm.channel_store([crm.scid_of(6), crm.scid_of(8, 1)], both=True)
    queries = [q for q, _ in cases]
    _, _, status, replies = host_answers(exe, tmp_path / "p", blob, None, queries, 0)
    assert status == [s for _, s in cases]
    want = crm.sorted_digest(blob)[0]
    for k, q in enumerate(queries):
        assert (status[k], replies[k]) == crm.replies(want, crm.CHAIN, q), (k, q.hex())
    # the option bits decide what a reply carries
    for v in list(range(8)) + [0x100, 0x10003]:
        d = crm.decode_reply(replies[queries.index(crm.query(crm.CHAIN, 5, 9, v))][0])
        assert (d["ts"] is not None, d["csum"] is not None) == (bool(v & 1), bool(v & 2)) and len(d["scids"]) == 2


@pytest.mark.parametrize("name,entries,bare", [("mainnet", 4, 84), ("canned", 2, 0)])
def test_host_digest_and_replies_of_the_stores_the_reference_ships(exe, tmp_path, orc, name, entries, bare):
    blob = rs.store(name)
    chain = rs.chain_of(blob)
    blocks = [e[0] >> 40 for e in crm.digest(blob)[0]]
    want = check_against_model(exe, tmp_path / "plain", blob, None, crm.query_kinds(blocks, chain), 0, chain)
    assert check_against_model(exe, tmp_path / "verdicts", blob, sa.model(orc, blob)[1], crm.mixed_queries(blocks, 65, chain), 8, chain) == want
    assert len(want) == entries and crm.digest(blob)[1]["channels_no_update"] == bare


def test_host_vector_queries_and_the_reference_checksums(exe, tmp_path):
    vec = rs.vectors()
    q1, q2 = vec["extended_queries"][:2]
    chain = bytes.fromhex(q1["msg"]["chainHash"])
    blocks = (34_999, 35_000, 35_099, 35_100, 99_999, 100_000, 101_499, 101_500)
    blob = crm.channel_store([crm.scid_of(b, 1, 0) for b in blocks], both=True)
    _, _, status, replies = host_answers(exe, tmp_path / "q", blob, None, [bytes.fromhex(q1["hex"]), bytes.fromhex(q2["hex"])], 0, chain)
    d1, d2 = crm.decode_reply(replies[0][0]), crm.decode_reply(replies[1][0])
    assert status == [0, 0] and [s >> 40 for s in d1["scids"]] == [100_000, 101_499] and [s >> 40 for s in d2["scids"]] == [35_000, 35_099]
    assert d1["ts"] is None and d1["csum"] is None and d2["ts"] is not None and d2["csum"] is not None
    ups = [bytes.fromhex(p["update"]) for p in vec["update_checksums"]]
    recs = []
    for k, m in enumerate(ups):
        recs += [crm.rec(crm.cann(int.from_bytes(m[98:106], "big"), k)), crm.rec(crm.AMOUNT), crm.rec(m, int.from_bytes(m[106:110], "big"))]
    want = check_against_model(exe, tmp_path / "c", sa.serialise(0x10, recs), None, [crm.query(crm.CHAIN, 0, 0xFFFFFFFF, 2)], 0)
    assert [e[2] for e in want] == [(p["checksum"], 0) for p in vec["update_checksums"]] == [(0x1112fa30, 0), (0xf32ce968, 0)]

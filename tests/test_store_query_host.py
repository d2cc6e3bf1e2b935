"""lightning_amd/csrc/store_query.h on the host, under AddressSanitizer and UBSan (tests/c/store_query_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the reference's fuzz corpus for query_short_channel_ids
(tests/golden/query_short_channel_ids_corpus.bin), one query cut at every length and every status case, on which the header and the sequential
model of scid_query_model must agree; and the directory and the answers against the model for the golden stores, the slot store, the hand-built
store and a store in three record orders, with and without verdicts -- the records and the occurrences visited in file order, in reverse and
in a scrambled order, the output written at all four alignments (the program compares those itself).  The device side of the same calls,
lamd_gossip_store_directory_build and lamd_short_channel_ids_reply_batch, is test_gpu_scid_query's.  One test pins the new
prototypes of include/lightning_amd.h to their ctypes bindings; the last ones run the query vector and the stores the reference ships
(test_reference_stores)."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_query") / "store_query_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_query_host.cpp")])
    return path


def host_run(exe, d, blob, queries, chain=crm.CHAIN, verdict=None):
    """-> dict of what the host build of the header computes; blob None: no image; chain None: every query against its own chain_hash"""
    d.mkdir()
    if blob is not None:
        (d / "image").write_bytes(blob)
    if verdict is not None:
        (d / "verdicts").write_bytes(np.array(verdict, dtype=np.int8).tobytes())
    (d / "queries").write_bytes(struct.pack("<I", len(queries)) + b"".join(struct.pack("<I", len(q)) + q for q in queries))
    (d / "chain").write_bytes(chain or b"")
    r = subprocess.run([exe, str(d / "image") if blob is not None else "-", str(d / "verdicts") if verdict is not None else "-", str(d / "queries"), str(d / "chain"),
                        str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda name, dt: np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)
    off, first, out = arr("msgoff", "<u8"), arr("first", "<u8"), (d / "out.bytes").read_bytes()
    spans = [range(int(first[q]), int(first[q + 1])) for q in range(len(queries))]
    ids = (d / "out.nodes").read_bytes()
    return dict(status=[int(x) for x in arr("status", np.int8)], per_query=[tuple(int(x) for x in r) for r in arr("perq", "<u4").reshape(-1, 4)],
                msgs=[[out[int(off[j]):int(off[j + 1])] for j in sp] for sp in spans], recs=[[int(arr("msgrec", "<u4")[j]) for j in sp] for sp in spans],
                nodes=[ids[k:k + 33] for k in range(0, len(ids), 33)], first=[int(x) for x in arr("nfirst", "<u4")], nann=[int(x) for x in arr("nann", "<u4")],
                bare_rec=[int(x) for x in arr("barerec", "<u4")], ranks=[int(x) for x in arr("ranks", "<u4")], counters=[int(x) for x in arr("counters", "<u8")])


def check_against_model(exe, d, blob, queries, verdict=None, chain=crm.CHAIN):
    got = host_run(exe, d, blob, queries, chain, verdict)
    m = sqm.directory(blob, verdict)
    assert (got["nodes"], got["first"], got["nann"], got["bare_rec"]) == (m["nodes"], m["first"], m["nann"], m["bare_rec"])
    assert got["ranks"] == [r for s in m["entries"] + m["bare"] for r in m["ranks"][s]]
    c = m["counters"]
    assert got["counters"] == [c["nodes"], c["nodes_announced"], c["nann_no_node"], c["nann_in_front"], c["nann_short"]]
    status, per_query, msgs, recs = sqm.answers(m, queries, chain)
    for name, a, b in zip(("status", "per_query", "msgs", "recs"), (got["status"], got["per_query"], got["msgs"], got["recs"]), (status, per_query, msgs, recs)):
        assert a == b, (name, a[:4], b[:4])
    return m, got


def corpus():
    raw = open(os.path.join(ROOT, "tests", "golden", "query_short_channel_ids_corpus.bin"), "rb").read()
    n, pos, out = struct.unpack_from("<I", raw)[0], 4, []
    for _ in range(n):
        ln = struct.unpack_from("<I", raw, pos)[0]
        out.append(raw[pos + 4:pos + 4 + ln])
        pos += 4 + ln
    assert pos == len(raw) and n == 552 and sum(len(m) - 2 for m in out) == 29612      # all of the reference's inputs, none left out
    return out


def test_the_fuzz_corpus_of_the_reference_parses_as_in_the_model(exe, tmp_path):
    msgs = corpus()
    assert all(m[:2] == b"\x01\x05" for m in msgs)
    # against its own chain every query gets past the chain check: the statuses behind it show
    got = host_run(exe, tmp_path / "own", None, msgs, None)
    want = [sqm.parse(m, m[2:34] if len(m) >= 34 else bytes(32))[0] for m in msgs]
    assert got["status"] == want and {-1, 0, 2, 3} <= set(want)
    assert got["per_query"] == [(len(sqm.parse(m, m[2:34])[1]), 0, 0, 0) if st == 0 else (0, 0, 0, 0) for m, st in zip(msgs, want)]
    assert got["msgs"] == [[struct.pack(">H", 262) + m[2:34] + b"\x01"] if st == 0 else [] for m, st in zip(msgs, want)]
    # against ours: whatever decodes is foreign and gets the end message with its own chain and 0
    got = host_run(exe, tmp_path / "ours", None, msgs, crm.CHAIN)
    assert got["status"] == [sqm.parse(m)[0] for m in msgs] and set(got["status"]) == {-1, 1, 2}
    assert got["msgs"] == [[struct.pack(">H", 262) + m[2:34] + b"\x00"] if st == 1 else [] for m, st in zip(msgs, got["status"])]


def test_a_query_cut_at_every_length_and_every_status_case(exe, tmp_path):
    blob, S, _ = sqm.hand_store()
    known = [S["two"], S["one"], S["bare"]]
    full = sqm.query(crm.CHAIN, known, [1, 0x11f, 6], tlvs=b"\x03\x01\xaa")
    assert len(full) == 36 + 25 + 2 + 6 + 3
    cuts = [full[:k] for k in range(len(full) + 1)]
    by_hand = [0 if k in (61, 69, 72) else -1 for k in range(len(full) + 1)]
    m, got = check_against_model(exe, tmp_path / "cuts", blob, cuts)
    assert got["status"] == by_hand
    cases = sqm.status_cases(known)
    assert {c[1] for c in cases} == {-1, 0, 1, 2, 3, 4}
    m, got = check_against_model(exe, tmp_path / "cases", blob, [c[0] for c in cases])
    assert got["status"] == [c[1] for c in cases]
    assert all(len(ms) == (1 if st == 1 else 0) for ms, st in zip(got["msgs"], got["status"]) if st != 0)      # a rejected query gets nothing, a foreign one the end alone


def test_the_hand_built_store(exe, tmp_path):
    blob, S, N = sqm.hand_store()
    m, got = check_against_model(exe, tmp_path / "hand", blob, sqm.flag_queries(sqm.directory(blob)))
    recs = m["recs"]
    ann = {nid: (recs[r][4] if r != sqm.NONE else None) for nid, r in zip(m["nodes"], m["nann"])}
    assert m["nodes"] == sorted(N[k] for k in ("a", "b", "c", "early", "never", "f5", "x", "y"))
    assert ann[N["a"]] == sqm.nann(N["a"], 800, fill=0x22) and ann[N["c"]] == sqm.nann(N["c"], 7, flen=3) and ann[N["f5"]] == sqm.nann(N["f5"], 4, fill=0x33)
    assert ann[N["early"]] is None and ann[N["never"]] is None and ann[N["b"]] is None and ann[N["x"]] is None and ann[N["y"]] is not None
    assert m["ranks"][S["cutid"]] == (sqm.NONE, sqm.NONE) and m["bare"] == [S["bare"]]
    c = m["counters"]
    assert (c["nann_no_node"], c["nann_in_front"], c["nann_short"]) == (2, 2, 3)


def stores():
    blob, _ = crm.slot_store()
    yield "slots", blob
    yield "hand", sqm.hand_store()[0]
    for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"):
        yield name, sa._golden(name)
    yield "empty", crm.channel_store([])


def mixed_queries(d, rng):
    chans = sorted(d["chan"])
    qs = sqm.flag_queries(d)[-4:] if chans else []
    for k in range(12):
        pick = [rng.choice(chans) ^ (1 << 62 if rng.random() < 0.2 else 0) for _ in range(rng.randrange(0, 9))] if chans else [5, 6][:k % 3]
        qs.append(sqm.query(crm.CHAIN, pick, None if k % 3 == 0 else [rng.randrange(0, 1 << (8 * (1 + k % 4))) for _ in pick]))
    return qs + [c[0] for c in sqm.status_cases((chans + [1, 2, 3])[:3])]


@pytest.mark.parametrize("name,blob", list(stores()), ids=[n for n, _ in stores()])
def test_host_directory_and_answers_equal_the_model(exe, tmp_path, name, blob):
    d = sqm.directory(blob)
    m, got = check_against_model(exe, tmp_path / "plain", blob, mixed_queries(d, random.Random(5)))
    if d["chan"]:
        assert {0, 1, 2, 3, 4, -1} == set(got["status"]) and sum(p[2] for p in got["per_query"]) and len(m["nodes"]) >= 2


def three_orders():
    """the same channels, updates and node_announcements with the channels in ascending, descending and shuffled order"""
    ids = [sqm.node_id(1000 + k, 2 + k % 2) for k in range(9)]
    chans = []
    for k in range(14):
        s = crm.scid_of(400 + k // 2, k % 2, 1)
        a, b = ids[k % 9], ids[(3 * k + 1) % 9]
        group = [crm.fast_rec(sqm.cann_ids(s, a, b, flen=k % 3)), crm.fast_rec(crm.AMOUNT)]
        if k % 4 != 3:
            group.append(crm.fast_rec(crm.cupd(s, k & 1, 50 + k)))
        if k % 4 == 0:
            group.append(crm.fast_rec(crm.cupd(s, 1 - (k & 1), 90 + k, 141)))
        group += [crm.fast_rec(sqm.nann(a, 10 + k, fill=k)), crm.fast_rec(sqm.nann(ids[(k + 5) % 9], 30 - k, flen=k % 2, fill=0x80 + k))]
        chans.append(group)
    rng = random.Random(3)
    shuffled = chans[:]
    rng.shuffle(shuffled)
    for name, order in (("ascending", chans), ("descending", chans[::-1]), ("shuffled", shuffled)):
        yield name, sa.serialise(0x10, [r for g in order for r in g])


@pytest.mark.parametrize("name,blob", list(three_orders()), ids=[n for n, _ in three_orders()])
def test_a_store_in_three_record_orders_with_and_without_verdicts(exe, tmp_path, name, blob):
    d = sqm.directory(blob)
    qs = mixed_queries(d, random.Random(7))
    check_against_model(exe, tmp_path / "plain", blob, qs)
    recs = sa.walk(blob)[0]
    verdict = [0] * len(recs)
    for i, r in enumerate(recs):                                  # some updates, node_announcements and announcements judged bad
        if i % 7 == 3 or (r[4][:2] == b"\x01\x00" and i % 5 == 0):
            verdict[i] = 3
    m, _ = check_against_model(exe, tmp_path / "verdicts", blob, qs, verdict)
    assert m["counters"] != d["counters"] or m["nann"] != d["nann"]


def test_new_prototypes_and_bindings_agree(tmp_path):
    """the prototypes this header section adds have the argument counts of their ctypes bindings, and the two summaries the layouts a C compiler gives them"""
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    names = ["lamd_gossip_store_directory_build", "lamd_store_directory_free", "lamd_store_directory_node_count", "lamd_store_directory_read_nodes",
             "lamd_store_directory_read_channels", "lamd_short_channel_ids_reply_batch"]
    for n in names:
        proto = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
        assert proto, n
        res, args = _ffi.SYMBOLS[n]
        assert len(proto.group(2).split(",")) == len(args), n
        assert {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t}[proto.group(1)] == res, n
        for text, ct in zip(proto.group(2).split(","), args):
            assert ("size_t" in text and "*" not in text) == (ct is ctypes.c_size_t), (n, text)
    pairs = [("lamd_store_directory_summary", _ffi.LamdStoreDirectorySummary), ("lamd_scid_reply_summary", _ffi.LamdScidReplySummary)]
    lines = []
    for cname, cls in pairs:
        lines.append('  printf("%%zu\\n", sizeof(%s));\n' % cname)
        lines += ['  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()]
    want = []
    for cname, cls in pairs:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f[0]).offset for f in cls._fields_]
    assert out == want, (out, want)


@pytest.mark.parametrize("name", ["mainnet", "canned"])
def test_host_directory_and_answers_for_the_stores_the_reference_ships(exe, tmp_path, orc, name):
    blob = rs.store(name)
    chain, v = rs.chain_of(blob), sa.model(orc, blob)[1]
    d = sqm.directory(blob, v)
    m, got = check_against_model(exe, tmp_path / "flags", blob, sqm.flag_queries(d, chain), v, chain)
    announced = [r for r in m["nann"] if r != sqm.NONE]
    assert (len(m["nodes"]), len(announced), len(m["chan"])) == ((126, 0, 88) if name == "mainnet" else (3, 3, 2))
    assert m["nodes"] == sorted(set(m["nodes"])) and set(got["status"]) == {0}
    sent = [x for ms in got["msgs"] for x in ms if x[:2] == b"\x01\x01"]
    assert bool(sent) == bool(announced) and set(sent) == {m["recs"][r][4] for r in announced}


def test_host_answer_to_the_vector_query(exe, tmp_path):
    q = rs.vectors()["extended_queries"][3]
    chain, known = bytes.fromhex(q["msg"]["chainHash"]), rs.scid("0x0x15465")
    blob = crm.channel_store([known], both=True)
    m, got = check_against_model(exe, tmp_path / "q", blob, [bytes.fromhex(q["hex"])], chain=chain)
    recs = sa.walk(blob)[0]
    assert got["status"] == [0] and got["per_query"] == [(3, 1, 3, 0)]
    assert got["msgs"] == [[recs[0][4], recs[2][4], recs[3][4], struct.pack(">H", 262) + chain + b"\x01"]]

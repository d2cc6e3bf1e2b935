"""lightning_amd/csrc/store_compare.h on the host, under AddressSanitizer and UBSan (tests/c/store_compare_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the program's own checks of the parser, the searches and the layout; the reference's fuzz
corpus for reply_channel_range (tests/golden/reply_channel_range_corpus.bin), one reply cut at every length and every status case, on which the
header and the sequential model of range_compare_model must agree; and classification, merge and the query_short_channel_ids bytes against the model
for hand-built stores and the golden ones -- the entries visited in file order, in reverse and in a scrambled order, the output written at all four
alignments (the program compares those itself).  The device side of the same call, lamd_channel_range_compare_batch, is test_gpu_range_compare's.
Last, the reply vector and the stores the reference ships (test_reference_stores)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import range_compare_model as rcm  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_compare") / "store_compare_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_compare_host.cpp")])
    return path


def test_parser_searches_and_layout_under_the_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def host_compare(exe, d, blob, msgs, chain=crm.CHAIN, want=None, max_unknown=0, max_stale=0, verdict=None):
    """-> (status, per_msg, unknown, stale, flags, [message bytes], bare) as the host build of the header computes them; blob None: an empty digest;
    chain None: every message against its own chain_hash"""
    d.mkdir()
    if blob is not None:
        (d / "image").write_bytes(blob)
    if verdict is not None:
        (d / "verdicts").write_bytes(np.array(verdict, dtype=np.int8).tobytes())
    (d / "msgs").write_bytes(struct.pack("<I", len(msgs)) + b"".join(struct.pack("<I", len(m)) + m for m in msgs))
    (d / "chain").write_bytes(chain or b"")
    if want is not None:
        (d / "want").write_bytes(b"".join(struct.pack("<II", *w) for w in want))
    r = subprocess.run([exe, str(d / "image") if blob is not None else "-", str(d / "verdicts") if verdict is not None else "-", str(d / "msgs"), str(d / "chain"),
                        str(d / "want") if want is not None else "-", str(max_unknown), str(max_stale), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda name, dt: np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)
    off, out = arr("msgoff", "<u8"), (d / "out.bytes").read_bytes()
    return ([int(x) for x in arr("status", np.int8)], [tuple(int(x) for x in r) for r in arr("permsg", "<u4").reshape(-1, 3)], [int(x) for x in arr("unknown", "<u8")],
            [int(x) for x in arr("stale", "<u8")], [int(x) for x in arr("flags", np.uint8)], [out[int(off[j]):int(off[j + 1])] for j in range(len(off) - 1)],
            [int(x) for x in arr("bare", "<u8")])


def check_against_model(exe, d, blob, msgs, want=None, max_unknown=0, max_stale=0, verdict=None, chain=crm.CHAIN):
    entries = crm.sorted_digest(blob, verdict)[0] if blob is not None else []
    bare = rcm.bare(blob, verdict) if blob is not None else []
    got = host_compare(exe, d, blob, msgs, chain, want, max_unknown, max_stale, verdict)
    model = rcm.compare(entries, bare, chain, msgs, want, max_unknown, max_stale)
    assert got[6] == bare
    for name, a, b in zip(("status", "per_msg", "unknown", "stale", "flags", "messages"), got, model):
        assert a == b, (name, a[:8], b[:8])
    return model


def corpus():
    raw = open(os.path.join(ROOT, "tests", "golden", "reply_channel_range_corpus.bin"), "rb").read()
    n, pos, out = struct.unpack_from("<I", raw)[0], 4, []
    for _ in range(n):
        ln = struct.unpack_from("<I", raw, pos)[0]
        out.append(raw[pos + 4:pos + 4 + ln])
        pos += 4 + ln
    assert pos == len(raw) and n == 683
    return out


def test_the_fuzz_corpus_of_the_reference_parses_as_in_the_model(exe, tmp_path):
    msgs = corpus()
    assert all(m[:2] == b"\x01\x08" for m in msgs)
    # against its own chain every message gets past the chain check: the statuses behind it show
    st = host_compare(exe, tmp_path / "own", None, msgs, None)[0]
    want = [rcm.parse(m, m[2:34] if len(m) >= 34 else bytes(32))[0] for m in msgs]
    assert st == want and {-1, 0, 2, 3, 5} <= set(st)
    # against ours: malformed or foreign, and nothing is looked up
    got = host_compare(exe, tmp_path / "ours", None, msgs, crm.CHAIN)
    assert got[0] == [rcm.parse(m)[0] for m in msgs] and set(got[0]) == {-1, 1} and got[2] == got[3] == got[5] == []
    # with a query outstanding that nothing overlaps
    st = host_compare(exe, tmp_path / "want", None, msgs, None, want=[(0xFFFFFFFF, 0xFFFFFFFF)] * len(msgs))[0]
    assert st == [rcm.parse(m, m[2:34] if len(m) >= 34 else bytes(32), (0xFFFFFFFF, 0xFFFFFFFF))[0] for m in msgs] and 4 in st and 0 not in st


def test_a_reply_cut_at_every_length_and_every_status_case(exe, tmp_path):
    s = [crm.scid_of(10 + k, k, 1) for k in range(3)]
    t = [(7, 8), (9, 10), (11, 12)]
    full = rcm.reply(crm.CHAIN, 5, 9, s, t, t)
    assert len(full) == 123
    cuts = [full[:k] for k in range(len(full) + 1)]
    by_hand = [0 if k in (70, 97, 123) else -1 for k in range(len(full) + 1)]
    got = check_against_model(exe, tmp_path / "cuts", None, cuts)
    assert got[0] == by_hand and got[1] == [(3, 3, 0) if x == 0 else (0, 0, 0) for x in by_hand] and got[2] == s
    cases = rcm.status_cases()
    assert {c[2] for c in cases} == {-1, 0, 1, 2, 3, 4, 5, 6}
    plain = [c for c in cases if c[1] is None]
    got = check_against_model(exe, tmp_path / "plain", None, [c[0] for c in plain])
    assert got[0] == [c[2] for c in plain]
    got = check_against_model(exe, tmp_path / "want", None, [c[0] for c in cases], want=[c[1] or (0, 0xFFFFFFFF) for c in cases])
    assert got[0] == [c[2] for c in cases]
    assert all(p == (0, 0, 0) for p, st in zip(got[1], got[0]) if st != 0) and len(got[2]) == 3      # rejected messages contribute nothing


def stores():
    blob, names = crm.slot_store()
    yield "slots", blob
    yield "channels", crm.channel_store([crm.scid_of(9 - b, b) for b in range(7)], both=True)
    yield "one_sided", crm.channel_store([crm.scid_of(700 + 3 * b, b % 5, b & 1) for b in range(40)])
    yield "population", crm.population_store([1, 2, 3, 8])
    yield "empty", crm.channel_store([])
    for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"):
        yield name, sa._golden(name)


@pytest.mark.parametrize("name,blob", list(stores()), ids=[n for n, _ in stores()])
def test_host_classification_merge_and_queries_equal_the_model(exe, tmp_path, name, blob):
    entries, bare = crm.sorted_digest(blob)[0], rcm.bare(blob)
    msgs = rcm.probe_replies(entries, bare) + [c[0] for c in rcm.status_cases()]
    status, per_msg, unknown, stale, flags, out = check_against_model(exe, tmp_path / "defaults", blob, msgs)
    if entries:
        assert {0, 1} <= set(status) and unknown and stale and {2, 4, 6} >= set(flags) and len(out) == 2
        assert sum(p[1] for p in per_msg) > len(unknown) and sum(p[2] for p in per_msg) >= len(stale)      # counted before merging
    if name == "slots":
        assert len(bare) == 1 and bare[0] in stale and flags[stale.index(bare[0])] == 2
    for k, (mu, ms) in enumerate(((1, 1), (2, 3), (3, 2), (7, 7))):
        check_against_model(exe, tmp_path / ("chunk%d" % k), blob, msgs, max_unknown=mu, max_stale=ms)


def test_host_digest_with_verdicts_and_want(exe, tmp_path):
    blob = crm.channel_store([crm.scid_of(50 + b, 1, b & 1) for b in range(12)], both=True)
    recs = sa.walk(blob)[0]
    verdict = [0] * len(recs)
    for i, r in enumerate(recs):                                                             # every update of three channels judged bad: they become bare
        if r[4][:2] == b"\x01\x02" and (int.from_bytes(r[4][98:106], "big") >> 40) in (51, 55, 59):
            verdict[i] = 3
    entries, bare = crm.sorted_digest(blob, verdict)[0], rcm.bare(blob, verdict)
    assert len(bare) == 3 and len(entries) == 9
    msgs = rcm.probe_replies(entries, bare, per=3)
    want = [(0, 0xFFFFFFFF) if k % 3 else (0, 5) for k in range(len(msgs))]                  # every third query ends at block 5: most replies miss it
    got = check_against_model(exe, tmp_path / "v", blob, msgs, want=want, verdict=verdict)
    assert {0, 1, 4} <= set(got[0])


@pytest.mark.parametrize("name", ["mainnet", "canned"])
def test_host_compare_over_the_stores_the_reference_ships(exe, tmp_path, orc, name):
    blob = rs.store(name)
    chain, v = rs.chain_of(blob), sa.model(orc, blob)[1]
    entries, bare = crm.sorted_digest(blob, v)[0], rcm.bare(blob, v)
    assert (len(entries), len(bare)) == ((4, 84) if name == "mainnet" else (2, 0))
    msgs = rcm.probe_replies(entries, bare, chain) + [c[0] for c in rcm.status_cases(chain)]
    m = check_against_model(exe, tmp_path / "probe", blob, msgs, verdict=v, chain=chain)
    assert {0, 1} <= set(m[0]) and m[2] and m[3] and (not bare or set(bare) & set(m[3]))
    check_against_model(exe, tmp_path / "chunks", blob, msgs, max_unknown=3, max_stale=2, chain=chain)


def test_host_compare_of_the_vector_reply(exe, tmp_path):
    rep = rs.vectors()["extended_queries"][2]
    chain, first, number, _, scids, ts, _ = rs.reply_fields(rep)
    msg, want = bytes.fromhex(rep["hex"]), [(122334, 123834)]
    m = check_against_model(exe, tmp_path / "empty", None, [msg], want=want, chain=chain)
    assert (m[0], m[2], m[3]) == ([0], scids, [])
    known, ours = rs.scid("0x7x30934"), (489645, 4786863)
    blob = sa.serialise(0x10, [crm.rec(crm.cann(known)), crm.rec(crm.AMOUNT), crm.rec(crm.cupd(known, 0, ours[0]), ours[0]), crm.rec(crm.cupd(known, 1, ours[1]), ours[1])])
    m = check_against_model(exe, tmp_path / "known", blob, [msg], want=want, chain=chain)
    assert ts[1] == (489645, 4786864) and (m[0], m[2], m[3], m[4]) == ([0], [scids[0], scids[2]], [known], [4])
    assert check_against_model(exe, tmp_path / "outside", blob, [msg], want=[(0, 100)], chain=chain)[0] == [4]

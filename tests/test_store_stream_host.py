"""lightning_amd/csrc/store_stream.h on the host, under AddressSanitizer and UBSan (tests/c/store_stream_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the stream index of a store image and the answers to gossip_timestamp_filter, on which
the header and the sequential model of timestamp_filter_model must agree -- for the golden stores, the synthetic store with and without the
verdicts of its damaged copy, and hand-built stores; the records, the peers and the lanes of every tile visited in file order, in reverse and
in a scrambled order, the output written at all four alignments (the program compares those itself).  The device side of the same calls,
lamd_gossip_store_stream_build and lamd_timestamp_filter_reply_batch, is test_gpu_timestamp_filter's.  One test pins the new
prototypes of include/lightning_amd.h to their ctypes bindings; the last one runs the stores the reference ships (test_reference_stores)."""
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
import timestamp_filter_model as tfm  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

ROOT = sa.ROOT
NOW = 1_700_000_000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_stream") / "store_stream_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_stream_host.cpp")])
    return path


def host_run(exe, d, blob, filters, now=NOW, cursors=None, budgets=None, verdict=None, offsets=None, chain=crm.CHAIN):
    """-> dict of what the host build of the header computes; budgets: None per peer = unlimited"""
    d.mkdir()
    (d / "image").write_bytes(blob)
    if offsets is not None:
        (d / "offsets").write_bytes(np.array(offsets, dtype="<u8").tobytes())
    if verdict is not None:
        (d / "verdicts").write_bytes(np.array(verdict, dtype=np.int8).tobytes())
    (d / "filters").write_bytes(struct.pack("<I", len(filters)) + b"".join(struct.pack("<I", len(f)) + f for f in filters))
    (d / "chain").write_bytes(chain)
    cur = [tfm.AS_FILTER] * len(filters) if cursors is None else cursors
    bud = [None] * len(filters) if budgets is None else budgets
    (d / "peers").write_bytes(struct.pack("<I", now) + b"".join(struct.pack("<Qq", c, 2 ** 63 - 1 if b is None else b) for c, b in zip(cur, bud)))
    r = subprocess.run([exe, str(d / "image"), str(d / "offsets") if offsets is not None else "-", str(d / "verdicts") if verdict is not None else "-",
                        str(d / "filters"), str(d / "chain"), str(d / "peers"), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda name, dt: np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)
    off, first, out, rec = arr("msgoff", "<u8"), arr("first", "<u8"), (d / "out.bytes").read_bytes(), arr("msgrec", "<u4")
    spans = [range(int(first[p]), int(first[p + 1])) for p in range(len(filters))]
    ints = lambda name, dt: [int(x) for x in arr(name, dt)]
    return dict(srec=ints("srec", "<u4"), sts=ints("sts", "<u4"), slen=ints("slen", "<u4"), spos=ints("spos", "<u4"), pmax=ints("pmax", "<u4"),
                counters=ints("counters", "<u8"), status=ints("status", np.int8), cursor=ints("cursor", "<u8"), done=ints("done", np.uint8),
                msgs=[[out[int(off[j]):int(off[j + 1])] for j in sp] for sp in spans], recs=[[int(rec[j]) for j in sp] for sp in spans])


def check_against_model(exe, d, blob, filters, now=NOW, cursors=None, budgets=None, verdict=None, recs=None, image=None, chain=crm.CHAIN):
    """image: the bytes handed over when they are not all of blob (a cut image); recs: what stands for rec_off"""
    img = blob if image is None else image
    got = host_run(exe, d, img, filters, now, cursors, budgets, verdict, None if recs is None else [r[0] for r in recs], chain)
    m = tfm.index(blob, verdict, recs, len(img))
    assert (got["srec"], got["sts"], got["slen"]) == ([e[0] for e in m["list"]], [e[1] for e in m["list"]], [len(e[2]) for e in m["list"]])
    assert got["spos"] == m["spos"] and got["counters"] == [m["counters"][k] for k in tfm.COUNTERS]
    run, pm = 0, []
    for ts in m["hts"]:
        run = max(run, ts)
        pm.append(run)
    assert got["pmax"] == pm
    want = tfm.answers(m, filters, chain, now, cursors, budgets)
    for name, a, b in zip(("status", "cursor", "done", "msgs", "recs"), (got[k] for k in ("status", "cursor", "done", "msgs", "recs")), want):
        assert a == b, (name, a[:4], b[:4])
    return m, want


def mixed_peers(m, rng, count=40):
    """filters, cursors and budgets over the index m: the corpus, then random windows around the store's timestamps"""
    filters = tfm.corpus()
    stamps = sorted({e[1] for e in m["list"]}) or [5]
    n = len(m["list"])
    for _ in range(count):
        a = rng.choice(stamps) + rng.randrange(-2, 3)
        filters.append(tfm.filt(crm.CHAIN, max(0, a), rng.choice([0, 1, 2, 50, 10 ** 6, 0xFFFFFFFF])))
    cursors = [tfm.AS_FILTER if k % 3 else rng.randrange(0, n + 1) for k in range(len(filters))]
    budgets = [rng.choice([None, -1, 0, 1, 137, 138, 139, 1000, 100000]) for _ in filters]
    return filters, cursors, budgets


@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_host_index_and_answers_for_the_stores_the_reference_wrote(exe, tmp_path, name):
    blob = sa._golden(name)
    m = tfm.index(blob)
    assert m["counters"]["streamable"] >= 3
    filters, cursors, budgets = mixed_peers(m, random.Random(1))
    _, want = check_against_model(exe, tmp_path / "plain", blob, filters, max(m["hts"]) + 100, cursors, budgets)
    assert set(want[0]) == {-1, 0, 1} and {0, 1} <= set(want[2]) and any(want[3])
    check_against_model(exe, tmp_path / "all", blob, tfm.corpus(), max(m["hts"]) + 100)


def test_host_index_of_the_synthetic_store_with_and_without_verdicts(exe, tmp_path, synthetic, damaged):
    img, (_, v, _) = synthetic
    m, _ = check_against_model(exe, tmp_path / "plain", img, *mixed_peers(tfm.index(img), random.Random(2))[:1])
    c = m["counters"]
    assert c["skipped_deleted"] and c["skipped_type"] and c["streamable"]
    check_against_model(exe, tmp_path / "ok", img, tfm.corpus(), verdict=list(v))
    blob, (_, dv, _), _ = damaged
    recs = sa.walk(blob)[0]
    filters, cursors, budgets = mixed_peers(tfm.index(blob, list(dv)), random.Random(3))
    md, _ = check_against_model(exe, tmp_path / "damaged", blob, filters, NOW, cursors, budgets, verdict=list(dv))
    assert md["counters"]["skipped_verdict"] >= 4 and len(recs) == len(dv)
    assert md["counters"]["streamable"] < tfm.index(blob)["counters"]["streamable"]


def flag_store():
    """deleted, dying, deleted + dying, non-public, one-byte and empty messages between streamable ones; timestamps 0 among them"""
    s = lambda k: crm.scid_of(700 + k, 0, 0)
    recs = [crm.fast_rec(crm.cann(s(0)), 0), crm.fast_rec(crm.AMOUNT, 0), crm.fast_rec(crm.cupd(s(0), 0, 100), 100),
            crm.fast_rec(crm.cupd(s(0), 1, 101), 101, sa.F_COMPLETED | sa.F_DELETED), crm.fast_rec(crm.cupd(s(0), 1, 102), 102, sa.F_COMPLETED | tfm.F_DYING),
            crm.fast_rec(crm.cupd(s(0), 1, 103), 103, sa.F_COMPLETED | sa.F_DELETED | tfm.F_DYING), crm.fast_rec(sqm.nann(sqm.node_id(1), 104), 104),
            crm.fast_rec(b"\x10\x0a" + bytes(12), 105), crm.fast_rec(b"\x01", 106, sa.F_COMPLETED | sa.F_DELETED), crm.fast_rec(b"", 107, sa.F_COMPLETED | sa.F_DELETED),
            crm.fast_rec(b"\x01\x03" + bytes(40), 108), crm.fast_rec(b"\x00\xff" + bytes(9), 109), crm.fast_rec(b"\x01\x02", 110), crm.fast_rec(crm.cupd(s(0), 1, 111), 0)]
    return sa.serialise(0x10, recs)


def test_every_skip_reason_and_the_filter_corpus(exe, tmp_path):
    blob = flag_store()
    m, want = check_against_model(exe, tmp_path / "corpus", blob, tfm.corpus(), 7300)
    c = m["counters"]
    assert (c["streamable"], c["skipped_deleted"], c["skipped_dying"], c["skipped_type"]) == (5, 4, 1, 4)
    by_hand = [-1] * 42 + [0] * 3 + [-1, -1, 1] + [0] * 14
    assert want[0] == by_hand
    parsed = [tfm.parse(f) for f in tfm.corpus()[48:]]
    assert parsed[:6] == [(0, 0, 0xFFFFFFFF, 0), (0, 0, 0, 0), (0, 0, 0xFFFFFFFE, 0), (0, 1, 0xFFFFFFFF, 2), (0, 1, 1, 2), (0, 1, 0xFFFFFFFF, 2)]
    assert parsed[6:9] == [(0, 0xFFFFFFFF, 0xFFFFFFFF, 1)] * 3 and parsed[9:12] == [(0, 0xFFFFFFFE, 0xFFFFFFFF, 2), (0, 0xFFFFFFFE, 0xFFFFFFFE, 2), (0, 0xFFFFFFFE, 0xFFFFFFFF, 2)]
    assert parsed[12:] == [(0, 0xFFFFFF00, 0xFFFFFFFF, 2), (0, 0xFFFFFF00, 0xFFFFFFFF, 2)]
    # timestamp 0 passes every filter; first_timestamp 0xFFFFFFFF sends nothing and is done at once
    only_zero = tfm.answer(m, tfm.filt(crm.CHAIN, 5000, 10), crm.CHAIN, 0, 0)
    assert only_zero[4] == [0, 13] and tfm.answer(m, tfm.filt(crm.CHAIN, 0xFFFFFFFF, 5), crm.CHAIN, 7300)[1:4] == (5, 1, [])
    # every budget around every message boundary, from every cursor
    lens = [len(e[2]) for e in m["list"]]
    cums = [sum(lens[:k]) for k in range(len(lens) + 1)]
    budgets = sorted({b + d for b in cums for d in (-1, 0, 1)})
    peers = [(tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF), c, b) for c in range(6) for b in budgets]
    check_against_model(exe, tmp_path / "budgets", blob, [p[0] for p in peers], 7300, [p[1] for p in peers], [p[2] for p in peers])


def recent_store():
    """header timestamps that are not monotone; the first one >= 5000 sits on a DELETED record, the first one >= 6000 on a channel_amount"""
    s = crm.scid_of(800, 0, 0)
    stamps = [3000, 1000, 4000, 2000, 5000, 100, 4500, 6000, 5500, 200, 7000, 6500]
    recs = []
    for k, ts in enumerate(stamps):
        flags, msg = sa.F_COMPLETED, crm.cupd(s, k & 1, ts, 130 + k)
        if ts == 5000:
            flags |= sa.F_DELETED
        if ts == 6000:
            msg = crm.AMOUNT
        recs.append(crm.fast_rec(msg, ts, flags))
    return sa.serialise(0x10, recs), stamps


def test_the_recent_position(exe, tmp_path):
    blob, stamps = recent_store()
    m = tfm.index(blob)
    assert len(m["list"]) == 10
    assert [tfm.recent(m, t) for t in (0, 3000, 3001, 4001, 5000, 5001, 6000, 6001, 7000, 7001, 0xFFFFFFFF)] == [0, 0, 2, 4, 4, 6, 6, 8, 8, 10, 10]
    f = tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF)
    nows = [7200 + t for t in (0, 3000, 3001, 4001, 5000, 5001, 6000, 6001, 7000, 7001)] + [7199, 0, 100, 7200 + 0xFFFFFFFF - 7200]
    for k, now in enumerate(nows):
        _, want = check_against_model(exe, tmp_path / ("now%d" % k), blob, [f, tfm.filt(crm.CHAIN, 4200, 2000)], now, budgets=[-1, None])
        assert want[1][0] == tfm.recent(m, (now - 7200) & 0xFFFFFFFF)
    assert tfm.answers(m, [f], crm.CHAIN, 7199, budgets=[-1])[1] == [10] and tfm.answers(m, [f], crm.CHAIN, 7200, budgets=[-1])[1] == [0]      # now < 7200 wraps: T is huge


def test_an_image_that_ends_early_and_offsets_that_point_outside(exe, tmp_path):
    blob = sa.serialise(0x10, [crm.fast_rec(crm.cupd(crm.scid_of(9, 0, 0), k & 1, 50 + k, 130 + k), 50 + k) for k in range(5)])
    recs = sa.walk(blob)[0]
    filters = [tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF), tfm.filt(crm.CHAIN, 52, 2)]
    for cut in (len(blob) - 1, len(blob) - 60, recs[4][0] + 12, recs[4][0] + 11, recs[4][0]):
        m, _ = check_against_model(exe, tmp_path / ("cut%d" % cut), blob, filters, recs=recs, image=blob[:cut])
        assert m["counters"]["skipped_frame"] == 1 and m["counters"]["streamable"] == 4
    wild = [(len(blob) + 5,) + recs[0][1:], recs[1], (2 ** 64 - 1,) + recs[2][1:], (len(blob) - 3,) + recs[3][1:], recs[4], (len(blob),) + recs[4][1:]]
    m, want = check_against_model(exe, tmp_path / "wild", blob, filters, 60 + 7200, recs=wild)
    assert m["counters"]["skipped_frame"] == 4 and want[4][0] == [1, 4] and m["hts"] == [0, 51, 0, 0, 54, 0]


def test_tile_edges(exe, tmp_path):
    """lists of 0, 1, 63, 64, 65, 128 and 129 entries; budgets that end on the last lane of a tile and on the first lane of the next"""
    for n in (0, 1, 63, 64, 65, 128, 129):
        recs = [crm.fast_rec(crm.cupd(crm.scid_of(20, 0, 0), k & 1, 1000 + k, 128 + (k * 7) % 23), 1000 + k) for k in range(n)]
        blob = sa.serialise(0x10, recs)
        lens = [len(r["msg"]) for r in recs]
        cum = lambda k: sum(lens[:k + 1])
        peers = [(tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF), tfm.AS_FILTER, b) for b in (-1, 0, None)]
        for e in (62, 63, 64, 127):
            if e < n:
                peers += [(tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF), tfm.AS_FILTER, cum(e) - d) for d in (0, 1)]
        peers += [(tfm.filt(crm.CHAIN, 1000 + e, 1), 0, None) for e in (0, 63, 64, 128) if e < n] + [(tfm.filt(crm.CHAIN, 5, 10), 0, None)]
        peers += [(tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF), c, 1000) for c in (0, 1, 63, 64, 65, n) if c <= n]
        check_against_model(exe, tmp_path / ("n%d" % n), blob, [p[0] for p in peers], 2000 + 7200, [p[1] for p in peers], [p[2] for p in peers])


def test_new_prototypes_and_bindings_agree(tmp_path):
    """the prototypes this header section adds have the argument counts of their ctypes bindings, and the two summaries the layouts a C compiler gives them"""
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    names = ["lamd_gossip_store_stream_build", "lamd_store_stream_free", "lamd_store_stream_count", "lamd_store_stream_read", "lamd_timestamp_filter_reply_batch"]
    for n in names:
        proto = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
        assert proto, n
        res, args = _ffi.SYMBOLS[n]
        assert len(proto.group(2).split(",")) == len(args), n
        assert {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t}[proto.group(1)] == res, n
        for text, ct in zip(proto.group(2).split(","), args):
            assert ("size_t" in text and "*" not in text) == (ct is ctypes.c_size_t), (n, text)
            assert ("uint32_t" in text and "*" not in text) == (ct is ctypes.c_uint32), (n, text)
    pairs = [("lamd_store_stream_summary", _ffi.LamdStoreStreamSummary), ("lamd_filter_reply_summary", _ffi.LamdFilterReplySummary)]
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


@pytest.mark.parametrize("name,streamable", [("mainnet", 92), ("canned", 9)])
def test_host_index_and_answers_for_the_stores_the_reference_ships(exe, tmp_path, orc, name, streamable):
    blob = rs.store(name)
    chain, v, now = rs.chain_of(blob), sa.model(orc, blob)[1], rs.newest(blob) + 100
    everything = tfm.filt(chain, 0, 0xFFFFFFFF)
    m, want = check_against_model(exe, tmp_path / "corpus", blob, tfm.corpus(chain) + [everything], now, verdict=v, chain=chain)
    assert m["counters"]["streamable"] == streamable == len(want[3][-1]) and set(want[0]) == {-1, 0, 1}
    # a budget of 1 000 bytes from every position: what a resumed peer is sent next
    n = len(m["list"])
    _, want = check_against_model(exe, tmp_path / "resumed", blob, [everything] * (n + 1), now, list(range(n + 1)), [1000] * (n + 1), chain=chain)
    assert want[2][-1] == 1 and want[2][0] == 0 and all(r == [e[0] for e in m["list"][c:c + len(r)]] for c, r in enumerate(want[4]))

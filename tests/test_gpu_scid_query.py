"""The directory of a store image and the answers to query_short_channel_ids on the device (lamd_gossip_store_directory_build,
lamd_short_channel_ids_reply_batch, include/lightning_amd.h) against the sequential model of scid_query_model.py: every status, count, record index
and output byte, with no tolerance.  The same code on the host, under the sanitizers, is test_store_query_host's."""
import ctypes
import os
import random
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
FAR = 1 << 62                                                                               # no store of these tests has a scid with this bit
END1 = struct.pack(">H", 262) + crm.CHAIN + b"\x01"


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def build(eng, blob, verdict=None, **kw):
    """-> (StoreDirectory, the model's directory), the readers and the summary compared"""
    m = sqm.directory(blob, verdict)
    with eng.gossip_store_digest(blob, verdict=verdict) as dg:
        dr = eng.gossip_store_directory(dg, blob, verdict=verdict, **kw)
    ids, first, nann = dr.nodes()
    assert [bytes(x) for x in ids] == m["nodes"] and [int(x) for x in first] == m["first"] and [int(x) for x in nann] == m["nann"]
    bare_rec, erank, brank = dr.channels()
    assert [int(x) for x in bare_rec] == m["bare_rec"]
    assert [tuple(int(x) for x in r) for r in erank] == [m["ranks"][s] for s in m["entries"]]
    assert [tuple(int(x) for x in r) for r in brank] == [m["ranks"][s] for s in m["bare"]]
    assert {k: dr.summary[k] for k in m["counters"]} == m["counters"] and len(dr) == len(m["nodes"])
    return dr, m


def answers_equal_model(eng, dr, m, queries, chain=crm.CHAIN):
    """-> the model's (status, per_query, messages, records), which the device must equal"""
    status, per_query, msgs, recs, s = eng.short_channel_ids_replies(dr, queries, chain, return_records=True, return_summary=True)
    model = sqm.answers(m, queries, chain)
    got = ([int(x) for x in status], [tuple(int(x) for x in r) for r in per_query], msgs, recs)
    for name, a, b in zip(("status", "per_query", "messages", "records"), got, model):
        assert a == b, (name, len(a), len(b), a[:4], b[:4])
    st, pq = model[0], model[1]
    assert s["by_status"] == [st.count(0)] + [st.count(k) for k in range(1, 5)] + [st.count(-1)]
    assert (s["scids"], s["known"], s["channel_messages"], s["node_messages"]) == tuple(sum(p[k] for p in pq) for k in range(4))
    assert (s["end_messages"], s["messages"], s["bytes"]) == (st.count(0) + st.count(1), sum(len(x) for x in model[2]), sum(len(y) for x in model[2] for y in x))
    return model


@pytest.fixture(scope="module")
def hand(eng):
    blob, S, N = sqm.hand_store()
    dr, m = build(eng, blob)
    yield dr, m, S, N
    dr.free()


def big_store(n=600):
    """n channels with both updates over 87 nodes, two thirds of them announced"""
    ids = [sqm.node_id(k, 2 + k % 2) for k in range(87)]
    recs = []
    for k in range(n):
        s = crm.scid_of(5000 + k // 2, k % 2, 1)
        recs += [crm.fast_rec(sqm.cann_ids(s, ids[k % 50], ids[50 + k % 37])), crm.fast_rec(crm.AMOUNT), crm.fast_rec(crm.cupd(s, 0, 1000 + 2 * k)),
                 crm.fast_rec(crm.cupd(s, 1, 1001 + 2 * k, 141))]
    recs += [crm.fast_rec(sqm.nann(ids[k], k, flen=k % 4, fill=k)) for k in range(87) if k % 3]
    return recs


@pytest.fixture(scope="module")
def six_hundred(eng):
    blob = sa.serialise(0x10, big_store())
    dr, m = build(eng, blob)
    yield dr, m
    dr.free()


# ------------------------------------------------------------------------------------------------ 1. the directory
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_directory_of_the_stores_the_reference_wrote(eng, name):
    dr, m = build(eng, sa._golden(name))
    assert len(m["nodes"]) >= 2
    answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, sorted(m["chan"])), sqm.query(crm.CHAIN, sorted(m["chan"])[::-1], [0x18] * len(m["chan"]))])
    dr.free()


def test_directory_of_the_slot_store_the_synthetic_store_and_its_damaged_copy(eng, synthetic, damaged):
    dr, m = build(eng, crm.slot_store()[0])
    assert len(m["bare"]) == 1
    dr.free()
    img, (_, v, _) = synthetic
    for verdict in (None, list(v)):
        dr, m = build(eng, img, verdict)
        answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, sorted(m["chan"])[:2000])])
        dr.free()
    blob, (_, dv, _), _ = damaged
    dr, m = build(eng, blob, list(dv))
    answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, sorted(m["chan"])[:2000])])
    dr.free()


# ------------------------------------------------------------------------------------------------ 2. the hand-built store, every flag
def test_the_hand_built_store_and_every_flag_value(eng, hand):
    dr, m, S, N = hand
    recs = m["recs"]
    ann = {nid: (recs[r][4] if r != sqm.NONE else None) for nid, r in zip(m["nodes"], m["nann"])}
    assert m["nodes"] == sorted(N[k] for k in ("a", "b", "c", "early", "never", "f5", "x", "y")) and m["bare"] == [S["bare"]]
    assert ann[N["a"]] == sqm.nann(N["a"], 800, fill=0x22) and ann[N["early"]] is None and ann[N["never"]] is None and ann[N["b"]] is None      # b's are cut short
    assert m["ranks"][S["cutid"]] == (sqm.NONE, sqm.NONE)
    c = dr.summary
    assert (c["nann_no_node"], c["nann_in_front"], c["nann_short"], c["nodes_announced"]) == (2, 2, 3, 4)
    model = answers_equal_model(eng, dr, m, sqm.flag_queries(m))
    # by hand: the channel with two updates, flag 0x1f: announcement, both updates, a's last announcement (b has none), the end
    q = sqm.query(crm.CHAIN, [S["two"]])
    st, pq, msgs, rec = sqm.answer(m, q)
    assert (st, pq) == (0, (1, 1, 3, 1)) and msgs == [sqm.cann_ids(S["two"], N["a"], N["b"]), crm.cupd(S["two"], 0, 10), crm.cupd(S["two"], 1, 11, 140),
                                                    sqm.nann(N["a"], 800, fill=0x22), END1]
    assert sqm.answer(m, sqm.query(crm.CHAIN, [S["bare"]]))[1] == (1, 1, 1, 1) and sqm.answer(m, sqm.query(crm.CHAIN, [S["cutid"]]))[1] == (1, 1, 2, 0)
    assert len(model[0]) == 32 * len(m["chan"]) + 4


# ------------------------------------------------------------------------------------------------ 3. flag forms
def test_flag_forms(eng, hand):
    dr, m, S, _ = hand
    wide = sqm.query(crm.CHAIN, [S["two"]], raw_flags=b"\xfd\x01\x1f")                          # the three-byte bigsize 0x011f: bits 0..4 are 0x1f
    loose = sqm.query(crm.CHAIN, [S["two"]], raw_flags=b"\xfd\x00\x1f")                         # 0x1f in three bytes: not minimal
    model = answers_equal_model(eng, dr, m, [wide, loose, sqm.query(crm.CHAIN, [S["two"]]), sqm.query(crm.CHAIN, [S["two"]], [1 << 63 | 5])])
    assert model[0] == [0, 2, 0, 0] and model[2][0] == model[2][2] and len(model[2][0]) == 5 and model[2][1] == [] and model[1][3] == (1, 1, 2, 0)


# ------------------------------------------------------------------------------------------------ 4. query cases
def test_duplicates_unknown_scids_and_the_querys_order(eng, hand):
    dr, m, S, N = hand
    two, one, bare = S["two"], S["one"], S["bare"]
    model = answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, [two, one, two]), sqm.query(crm.CHAIN, [two | FAR, 7, bare | FAR]),
                                             sqm.query(crm.CHAIN, sorted(S.values())[::-1]), sqm.query(crm.CHAIN, sorted(S.values())),
                                             sqm.query(crm.CHAIN, [7, two, 8, two | FAR, one], [1, 1, 1, 1, 2])])
    a_two = sqm.cann_ids(two, N["a"], N["b"])
    assert model[1][0] == (3, 3, 8, 1) and model[2][0].count(a_two) == 2 and model[2][0].count(sqm.nann(N["a"], 800, fill=0x22)) == 1      # channel messages twice, the node once
    assert model[1][1] == (3, 0, 0, 0) and model[2][1] == [END1]
    chan_part = lambda k: model[3][k][:model[1][k][2]]
    assert chan_part(2) != chan_part(3) and sorted(chan_part(2)) == sorted(chan_part(3))                                                  # the answer follows the query
    assert model[3][2][0] == m["chan"][max(S.values())][0]
    assert model[1][4] == (5, 2, 1, 0)                                                                                                       # bit 1 on a channel without update 0


# ------------------------------------------------------------------------------------------------ 5. ids that share long prefixes
def test_node_ids_that_differ_in_one_late_byte(eng):
    base = bytes([3]) + bytes(range(100, 132))
    ids = [base]
    for at in (8, 16, 24, 32, 7, 15, 23, 31):
        for delta in (1, 0x80):
            x = bytearray(base)
            x[at] = (x[at] + delta) & 0xff
            ids.append(bytes(x))
    ids += [bytes([0xff]) * 33, bytes(33), bytes([0xff]) * 32 + b"\xfe"]
    assert len(set(ids)) == len(ids)
    order = ids[:]
    random.Random(11).shuffle(order)
    recs, scids = [], []
    for k in range(len(order)):
        s = crm.scid_of(900 + k, 0, k & 1)
        scids.append(s)
        recs += [crm.fast_rec(sqm.cann_ids(s, order[k], order[(k + 7) % len(order)], flen=k % 3)), crm.fast_rec(crm.AMOUNT)]
    recs += [crm.fast_rec(crm.cann(crm.scid_of(990, 1, 1))[:320]), crm.fast_rec(crm.AMOUNT)]     # a channel that names no node, between them in the candidates
    recs += [crm.fast_rec(sqm.nann(x, k, fill=k)) for k, x in enumerate(order)]
    dr, m = build(eng, sa.serialise(0x10, recs))
    assert m["nodes"] == sorted(ids)
    model = answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, scids, [0x18] * len(scids)), sqm.query(crm.CHAIN, scids[::-1], [0x10] * len(scids))])
    got_ids = [x[72:105] for x in model[2][0][:-1]]
    assert got_ids == sorted(ids) and model[1][0] == (len(scids), len(scids), 0, len(ids))
    dr.free()


# ------------------------------------------------------------------------------------------------ 6. every status
def test_every_status(eng, hand):
    dr, m, S, _ = hand
    cases = sqm.status_cases([S["two"], S["one"], S["bare"]])
    model = answers_equal_model(eng, dr, m, [c[0] for c in cases])
    assert model[0] == [c[1] for c in cases] and set(model[0]) == {-1, 0, 1, 2, 3, 4}
    foreign = [k for k, st in enumerate(model[0]) if st == 1]
    assert len(foreign) >= 3 and all(model[2][k] == [struct.pack(">H", 262) + crm.FOREIGN + b"\x00"] for k in foreign)      # with and without bad scids


# ------------------------------------------------------------------------------------------------ 7. sizes
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 8191])
def test_queries_of_many_sizes(eng, six_hundred, count):
    dr, m = six_hundred
    chans = sorted(m["chan"])
    rng = random.Random(count)
    scids = [rng.choice(chans) ^ (FAR if rng.random() < 0.1 else 0) for _ in range(count)]
    model = answers_equal_model(eng, dr, m, [sqm.query(crm.CHAIN, scids), sqm.query(crm.CHAIN, scids, [rng.randrange(32) for _ in scids])])
    assert model[1][0][0] == count
    if count == 8191:                                                                            # (the most a be16 len holds)
        assert model[1][0][3] == 58 and model[1][0][1] < count                                   # every announced node, once


def test_a_batch_of_130_mixed_queries(eng, six_hundred):
    dr, m = six_hundred
    chans = sorted(m["chan"])
    rng = random.Random(130)
    cases = [c[0] for c in sqm.status_cases(chans[:3])]
    qs = []
    for k in range(130):
        if k % 5 == 4:
            qs.append(cases[(7 * (k // 5)) % len(cases)])                                      # 26 of the 31 cases, every status among them
        else:
            pick = [rng.choice(chans) ^ (FAR if rng.random() < 0.2 else 0) for _ in range([0, 1, 3, 64, 100, 7][k % 6])]
            qs.append(sqm.query(crm.CHAIN, pick, None if k % 3 == 0 else [rng.randrange(1 << 16) for _ in pick]))
    model = answers_equal_model(eng, dr, m, qs)
    assert set(model[0]) == {-1, 0, 1, 2, 3, 4} and (0, 0, 0, 0) in model[1]


# ------------------------------------------------------------------------------------------------ 8, 9. alignment, sizing
GUARD = 64


def raw_call(eng, dr, queries, pad=0, msg_cap=0, out_cap=0, host_out=True, d_out=None):
    """the C call itself, the queries behind `pad` bytes, every array pre-filled and followed by a guard region"""
    from lightning_amd import _ffi
    n = len(queries)
    qoff = np.zeros(n + 1, dtype=np.uint64)
    qoff[0] = pad
    qoff[1:] = pad + np.cumsum([len(q) for q in queries], dtype=np.uint64) if n else pad
    blob = np.frombuffer(b"\xA5" * pad + b"".join(queries) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(crm.CHAIN, dtype=np.uint8)
    status, per_query = np.full(n + GUARD, 99, dtype=np.int8), np.full(4 * n + GUARD, 0xABABABAB, dtype=np.uint32)
    first, msg_off = np.full(n + 1 + GUARD, 2 ** 64 - 1, dtype=np.uint64), np.full(msg_cap + 1 + GUARD, 2 ** 64 - 1, dtype=np.uint64)
    msg_rec, out = np.full(msg_cap + GUARD, 0xABABABAB, dtype=np.uint32), np.full(out_cap + GUARD, 0xEE, dtype=np.uint8)
    s = _ffi.LamdScidReplySummary()
    rc = eng._lib.lamd_short_channel_ids_reply_batch(eng._ctx, dr._h, chain.ctypes.data, n, blob.ctypes.data, qoff.ctypes.data, status.ctypes.data, per_query.ctypes.data,
                                                     first.ctypes.data, msg_cap, msg_off.ctypes.data, msg_rec.ctypes.data,
                                                     out.ctypes.data if host_out and d_out is None else None, None if d_out is None else d_out.data_ptr(), out_cap,
                                                     ctypes.byref(s))
    return rc, status, per_query, first, msg_off, msg_rec, out, s


def untouched(a, used=0):
    fill = {np.dtype(np.uint64): 2 ** 64 - 1, np.dtype(np.uint8): 0xEE, np.dtype(np.int8): 99, np.dtype(np.uint32): 0xABABABAB}[a.dtype]
    return bool((a[used:] == fill).all())


def test_queries_and_output_at_every_alignment_and_a_resident_image(eng, hand):
    import torch
    dr, m, S, _ = hand
    queries = sqm.flag_queries(m)[-4:] + [c[0] for c in sqm.status_cases([S["two"], S["one"], S["bare"]])]
    model = sqm.answers(m, queries)
    flat = b"".join(y for x in model[2] for y in x)
    M, nq = sum(len(x) for x in model[2]), len(queries)
    offs = list(np.cumsum([0] + [len(y) for x in model[2] for y in x]))
    for pad in range(4):
        rc, status, per_query, first, msg_off, msg_rec, out, s = raw_call(eng, dr, queries, pad, M, len(flat))
        assert rc == 0 and [int(x) for x in status[:nq]] == model[0] and [tuple(int(x) for x in per_query[4 * i:4 * i + 4]) for i in range(nq)] == model[1]
        assert out[:len(flat)].tobytes() == flat and [int(x) for x in msg_off[:M + 1]] == offs and [int(x) for x in msg_rec[:M]] == [y for x in model[3] for y in x]
        assert [int(x) for x in first[:nq + 1]] == list(np.cumsum([0] + [len(x) for x in model[2]]))
        assert untouched(status, nq) and untouched(per_query, 4 * nq) and untouched(first, nq + 1) and untouched(msg_off, M + 1) and untouched(msg_rec, M) and untouched(out, len(flat))
    eng._after_torch()
    for shift in (0, 1, 2, 3):                                                              # the output left on the device
        d = torch.full((len(flat) + shift + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert raw_call(eng, dr, queries, 3, M, len(flat), d_out=d[shift:])[0] == 0
        h = d.cpu().numpy()
        assert h[shift:shift + len(flat)].tobytes() == flat and set(h[:shift]) <= {0xEE} and set(h[shift + len(flat):]) == {0xEE}
        rc, *_, s = raw_call(eng, dr, queries, 3, M, len(flat) - 1, d_out=d[shift:])
        assert rc == -3 and s.bytes == len(flat)
        assert d.cpu().numpy()[shift:shift + len(flat)].tobytes() == flat                  # ... and left alone by the call that failed
    # the image resident, at an odd address, read in place: the same directory, the same answers
    blob = sqm.hand_store()[0]
    t = torch.zeros(len(blob) + 3, dtype=torch.uint8, device="cuda")
    t[3:] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with eng.gossip_store_digest(blob) as dg:
        res = eng.gossip_store_directory(dg, rec_off=sa_offsets(blob), d_store=t[3:], chain_hash=crm.CHAIN)
    got = eng.short_channel_ids_replies(res, queries, return_records=True)
    assert [bytes(x) for x in res.nodes()[0]] == m["nodes"] and got[2] == model[2] and got[3] == model[3]
    res.free()


def sa_offsets(blob):
    return np.array([r[0] for r in sa.walk(blob)[0]], dtype=np.uint64)


def test_caps_one_short_write_nothing_and_empty_inputs(eng, hand):
    from lightning_amd import Engine
    from lightning_amd.engine import LamdError
    dr, m, S, _ = hand
    queries = sqm.flag_queries(m)[-4:]
    model = sqm.answers(m, queries)
    M, total, nq = sum(len(x) for x in model[2]), sum(len(y) for x in model[2] for y in x), len(queries)
    for msg_cap, out_cap, host_out in ((M - 1, total, True), (M, total - 1, True), (0, 0, True), (0, 0, False)):
        rc, status, per_query, first, msg_off, msg_rec, out, s = raw_call(eng, dr, queries, 0, msg_cap, out_cap, host_out)
        assert rc == -3 and (s.messages, s.bytes, s.scids) == (M, total, sum(p[0] for p in model[1]))
        assert [int(x) for x in status[:nq]] == model[0] and [tuple(int(x) for x in per_query[4 * i:4 * i + 4]) for i in range(nq)] == model[1]
        assert [int(x) for x in first[:nq + 1]] == list(np.cumsum([0] + [len(x) for x in model[2]]))
        assert all(untouched(a) for a in (msg_off, msg_rec, out))
    rc, *_, msg_off, msg_rec, out, s = raw_call(eng, dr, queries, 0, M, 0, False)                 # no output asked for: the offsets alone
    assert rc == 0 and int(msg_off[M]) == total and [int(x) for x in msg_rec[:M]] == [y for x in model[3] for y in x] and untouched(out)
    rc, status, per_query, first, msg_off, *_, s = raw_call(eng, dr, [], 0, 1, 0)                  # nq == 0
    assert rc == 0 and int(first[0]) == 0 and int(msg_off[0]) == 0 and s.messages == 0
    assert answers_equal_model(eng, dr, m, []) == ([], [], [], [])
    # a directory of an empty digest: every scid is unknown, every accepted query gets its end message
    empty = sa.serialise(0x10, [])
    with eng.gossip_store_digest(empty) as dg:
        none = eng.gossip_store_directory(dg, empty)
    assert len(none) == 0 and none.summary["nodes"] == 0
    model = answers_equal_model(eng, none, sqm.directory(empty), queries + [sqm.query(crm.FOREIGN, [1])])
    assert model[2] == [[END1]] * nq + [[struct.pack(">H", 262) + crm.FOREIGN + b"\x00"]]
    none.free()
    only_amount = sa.serialise(0x10, [crm.fast_rec(crm.AMOUNT)])
    dr1, m1 = build(eng, only_amount)
    answers_equal_model(eng, dr1, m1, queries)
    dr1.free()
    # a digest of another n, and a directory of another context
    blob = sqm.hand_store()[0]
    with eng.gossip_store_digest(blob) as dg:
        off = sa_offsets(blob)
        with pytest.raises(LamdError):
            eng.gossip_store_directory(dg, blob, rec_off=off[:-1])
        with pytest.raises(LamdError):
            eng.gossip_store_directory(dg, only_amount)
    with Engine(0) as other, pytest.raises(LamdError):
        other.short_channel_ids_replies(dr, queries, crm.CHAIN)


# ------------------------------------------------------------------------------------------------ 10. round trip with the comparison
def test_round_trip_with_the_comparison(eng):
    import range_compare_model as rcm
    recs_a = big_store()
    chans = [recs_a[4 * k:4 * k + 4] for k in range(600)]
    recs_b, removed, stale = [], [], {}
    for k, (ann, amount, u0, u1) in enumerate(chans):
        s = crm.scid_of(5000 + k // 2, k % 2, 1)
        if k % 10 == 0:
            removed.append(s)
            continue
        ups = []
        for d, u in enumerate((u0, u1)):
            ts = int.from_bytes(u["msg"][106:110], "big")
            if (2 * k + d) % 7 == 0:                                                        # B's copy is one second older
                stale[s] = stale.get(s, 0) | (2 << d)
                u = crm.fast_rec(crm.cupd(s, d, ts - 1, len(u["msg"])))
            ups.append(u)
        recs_b += [ann, amount] + ups
    blob_a, blob_b = sa.serialise(0x10, recs_a), sa.serialise(0x10, recs_b)
    dra, ma = build(eng, blob_a)
    with eng.gossip_store_digest(blob_a) as da, eng.gossip_store_digest(blob_b) as db:
        st, replies = eng.channel_range_replies(da, crm.CHAIN, [crm.query(crm.CHAIN, 0, 0xFFFFFFFF, 1)], max_encoded_bytes=2000)
        assert int(st[0]) == 0 and len(replies[0]) > 3
        _, _, unknown, stale_scid, flags, queries = eng.channel_range_compare(db, crm.CHAIN, replies[0], max_unknown=25, max_stale=40)
    assert [int(x) for x in unknown] == removed and dict(zip((int(x) for x in stale_scid), (int(x) for x in flags))) == stale and len(queries) == 3 + 4
    model = answers_equal_model(eng, dra, ma, queries)
    assert set(model[0]) == {0} and all(x[-1] == END1 and x.count(END1) == 1 for x in model[2])
    walk = ma["recs"]
    anns = [walk[r][4] for q in model[3] for r in q[:-1] if walk[r][4][:2] == b"\x01\x00"]
    assert anns == [walk[ma["chan"][s][0]][4] for s in removed]                                 # exactly the removed channels' announcements
    stale_updates = [r for q in model[3][3:] for r in q[:-1]]
    assert stale_updates == [ma["chan"][s][1 + d] for s in sorted(stale) for d in (0, 1) if stale[s] & (2 << d)]      # exactly A's slot records for the flags
    assert all(p[3] == 0 for p in model[1][3:]) and all(p[3] > 0 for p in model[1][:3])
    dra.free()

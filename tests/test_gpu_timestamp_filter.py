"""The stream index of a store image and the answers to gossip_timestamp_filter on the device (lamd_gossip_store_stream_build,
lamd_timestamp_filter_reply_batch, include/lightning_amd.h) against the sequential model of timestamp_filter_model.py: every status, cursor, done
flag, record index and output byte, with no tolerance.  The same code on the host, under the sanitizers, is test_store_stream_host's."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_store_audit as sa  # noqa: E402
import timestamp_filter_model as tfm  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)
from test_store_stream_host import flag_store, mixed_peers, recent_store  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF)
NOW = 9200                                                                                  # recent: the first record stamped 2000 or later


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def offsets(recs):
    return np.array([r[0] for r in recs], dtype=np.uint64)


def build(eng, blob, verdict=None, recs=None, image=None):
    """-> (StoreStream, the model's index), read() and the summary compared.  recs: what stands for rec_off; image: the bytes handed over"""
    img = blob if image is None else image
    m = tfm.index(blob, verdict, recs, len(img))
    ss = eng.gossip_store_stream(img, rec_off=None if recs is None else offsets(recs), verdict=verdict)
    rec, ts, ln = ss.read()
    assert [int(x) for x in rec] == [e[0] for e in m["list"]] and [int(x) for x in ts] == [e[1] for e in m["list"]]
    assert [int(x) for x in ln] == [len(e[2]) for e in m["list"]] and len(ss) == len(m["list"])
    assert {k: ss.summary[k] for k in tfm.COUNTERS} == m["counters"]
    return ss, m


def answers_equal_model(eng, ss, m, filters, now=NOW, cursors=None, budgets=None, chain=crm.CHAIN):
    """-> the model's (status, cursor_out, done, messages, records), which the device must equal"""
    if cursors is not None:
        cursors = [tfm.AS_FILTER if c is None else c for c in cursors]
    status, cur, done, msgs, recs, s = eng.timestamp_filter_replies(ss, filters, chain, now, cursors, budgets, return_summary=True, return_records=True)
    model = tfm.answers(m, filters, chain, now, cursors, budgets)
    got = ([int(x) for x in status], [int(x) for x in cur], [int(x) for x in done], msgs, recs)
    for name, a, b in zip(("status", "cursor_out", "done", "messages", "records"), got, model):
        assert a == b, (name, len(a), len(b), a[:4], b[:4])
    st = model[0]
    assert s["by_status"] == [st.count(0), st.count(1), st.count(-1)] and s["finished"] == sum(model[2])
    assert (s["messages"], s["bytes"]) == (sum(len(x) for x in model[3]), sum(len(y) for x in model[3] for y in x))
    return model


def tile_store(n):
    """n channel_updates stamped 1000 + k, their lengths between 128 and 150"""
    return sa.serialise(0x10, [crm.fast_rec(crm.cupd(crm.scid_of(20, 0, 0), k & 1, 1000 + k, 128 + (k * 7) % 23), 1000 + k) for k in range(n)])


@pytest.fixture(scope="module")
def s129(eng):
    ss, m = build(eng, tile_store(129))
    yield ss, m
    ss.free()


# ------------------------------------------------------------------------------------------------ 1. the index
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_index_of_the_stores_the_reference_wrote(eng, name):
    blob = sa._golden(name)
    ss, m = build(eng, blob)
    assert m["counters"]["streamable"] >= 3 and m["counters"]["skipped_type"] >= 1
    filters, cursors, budgets = mixed_peers(m, random.Random(1))
    answers_equal_model(eng, ss, m, filters, max(m["hts"]) + 100, cursors, budgets)
    ss.free()


def test_index_of_the_synthetic_store_and_its_damaged_copy(eng, synthetic, damaged):
    img, (_, v, _) = synthetic
    for verdict in (None, list(v)):
        ss, m = build(eng, img, verdict)
        assert m["counters"]["skipped_deleted"] and m["counters"]["streamable"]
        answers_equal_model(eng, ss, m, tfm.corpus() + [ALL], max(m["hts"]) + 100)
        ss.free()
    blob, (_, dv, _), _ = damaged
    ss, m = build(eng, blob, list(dv))
    assert m["counters"]["skipped_verdict"] >= 4
    filters, cursors, budgets = mixed_peers(m, random.Random(3))
    answers_equal_model(eng, ss, m, filters, max(m["hts"]) + 100, cursors, budgets)
    ss.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129])
def test_lists_at_the_tile_edges(eng, n):
    ss, m = build(eng, tile_store(n))
    assert len(ss) == n
    filters = [ALL, ALL, ALL, tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF), tfm.filt(crm.CHAIN, 1000 + n - 1, 1), tfm.filt(crm.CHAIN, 0xFFFFFFFF, 0)]
    model = answers_equal_model(eng, ss, m, filters, NOW, budgets=[None, 0, -1, None, None, None])
    assert len(model[3][0]) == n and len(model[3][1]) == min(n, 1) and model[1][2] == 0 and model[1][5] == n
    ss.free()


def test_every_record_skipped_a_cut_image_and_a_wild_offset(eng):
    ss, m = build(eng, sa.serialise(0x10, [crm.fast_rec(crm.AMOUNT, 5), crm.fast_rec(crm.cupd(1, 0, 6), 6, sa.F_COMPLETED | sa.F_DELETED),
                                           crm.fast_rec(crm.cupd(1, 0, 7), 7, sa.F_COMPLETED | tfm.F_DYING)]))
    assert len(ss) == 0 and (ss.summary["skipped_type"], ss.summary["skipped_deleted"], ss.summary["skipped_dying"]) == (1, 1, 1)
    model = answers_equal_model(eng, ss, m, [ALL, tfm.filt(crm.CHAIN, 6, 1)], 7206)
    assert model[1:4] == ([0, 0], [1, 1], [[], []])
    ss.free()
    blob = flag_store()
    ss, m = build(eng, blob)
    assert len(ss) == 5
    answers_equal_model(eng, ss, m, tfm.corpus(), 7300)
    ss.free()
    blob = tile_store(5)
    recs = sa.walk(blob)[0]
    for cut in (len(blob) - 60, recs[4][0] + 12, recs[4][0] + 11):                           # in the middle of the last record's message, behind and inside its header
        ss, m = build(eng, blob, recs=recs, image=blob[:cut])
        assert (len(ss), ss.summary["skipped_frame"]) == (4, 1)
        answers_equal_model(eng, ss, m, [ALL, tfm.filt(crm.CHAIN, 1002, 2)])
        ss.free()
    wild = [(len(blob) + 5,) + recs[0][1:], recs[1], (2 ** 64 - 1,) + recs[2][1:], (len(blob) - 3,) + recs[3][1:], recs[4], (len(blob),) + recs[4][1:]]
    ss, m = build(eng, blob, recs=wild)
    assert ss.summary["skipped_frame"] == 4 and [int(x) for x in ss.read()[0]] == [1, 4]
    answers_equal_model(eng, ss, m, [ALL, tfm.filt(crm.CHAIN, 1004, 1), tfm.filt(crm.CHAIN, 1004, 1)], 1004 + 7200, cursors=[None, None, 0])
    ss.free()


def test_the_recent_position(eng):
    blob, stamps = recent_store()
    ss, m = build(eng, blob)
    f = tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF)
    nows = [7200 + t for t in (0, 3000, 3001, 4001, 5000, 5001, 6000, 6001, 7000, 7001, 0xFFFFFFFF - 7200)] + [7199, 0, 100]
    for now in nows:
        model = answers_equal_model(eng, ss, m, [f, f, tfm.filt(crm.CHAIN, 4200, 2000)], now, budgets=[-1, None, None])
        assert model[1][0] == tfm.recent(m, (now - 7200) & 0xFFFFFFFF)
    assert tfm.answers(m, [f], crm.CHAIN, 7200 + 5000, budgets=[-1])[1] == [4] and tfm.answers(m, [f], crm.CHAIN, 7199, budgets=[-1])[1] == [10]
    ss.free()


# ------------------------------------------------------------------------------------------------ 2. the walk
def test_budgets_on_both_sides_of_every_tile_edge(eng, s129):
    ss, m = s129
    lens = [len(e[2]) for e in m["list"]]
    cum = lambda k: sum(lens[:k + 1])
    budgets = [-1, 0, None] + [cum(e) - d for e in (62, 63, 64, 127) for d in (0, 1)]
    model = answers_equal_model(eng, ss, m, [ALL] * len(budgets), NOW, budgets=budgets)
    # the check comes before the message: a budget of exactly the bytes after entry e lets entry e + 1 through, one byte less does not
    assert [len(x) for x in model[3]] == [0, 1, 129, 64, 63, 65, 64, 66, 65, 129, 128]
    assert model[1] == [0, 1, 129, 64, 63, 65, 64, 66, 65, 129, 128] and model[2] == [0, 0, 1] + [0] * 8
    for start in (0, 63, 64, 65):                                                            # the same budgets from cursors around the edge
        answers_equal_model(eng, ss, m, [ALL] * len(budgets), NOW, [start] * len(budgets), [None if b is None else b - cum(start) + lens[start] for b in budgets])


def test_filters_that_pass_one_entry_or_none_and_every_cursor(eng, s129):
    ss, m = s129
    filters = [tfm.filt(crm.CHAIN, 1064, 1), tfm.filt(crm.CHAIN, 1128, 1), tfm.filt(crm.CHAIN, 5, 10), tfm.filt(crm.CHAIN, 2000, 10)]
    model = answers_equal_model(eng, ss, m, filters, NOW, cursors=[0, 0, 0, 0])
    assert model[4] == [[64], [128], [], []] and model[1] == [129] * 4 and model[2] == [1] * 4
    for c in (0, 63, 64, 65, 129):
        model = answers_equal_model(eng, ss, m, [ALL, ALL, tfm.filt(crm.CHAIN, 1064, 2)], NOW, [c] * 3, [None, 300, None])
        assert model[4][0] == list(range(c, 129))
    from lightning_amd.engine import LamdError
    with pytest.raises(LamdError):
        eng.timestamp_filter_replies(ss, [ALL, ALL], crm.CHAIN, NOW, cursors=[0, 130])
    model = answers_equal_model(eng, ss, m, [tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF)] * 3, 1100 + 7200, budgets=[None, 0, -1])      # as the filter says: recent
    assert model[4][0] == list(range(100, 129)) and model[1][2] == 100


def test_resumption_with_a_budget_of_1000_bytes(eng, s129):
    ss, m = s129
    for f in (ALL, tfm.filt(crm.CHAIN, 1010, 100), tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF)):
        whole = tfm.answer(m, f, crm.CHAIN, 1030 + 7200)
        cur, done, recs, msgs, calls = tfm.AS_FILTER, 0, [], [], 0
        while not done:
            st, c, d, ms, rs = eng.timestamp_filter_replies(ss, [f], crm.CHAIN, 1030 + 7200, [cur], [1000], return_records=True)
            assert tfm.answer(m, f, crm.CHAIN, 1030 + 7200, cur, 1000) == (int(st[0]), int(c[0]), int(d[0]), ms[0], rs[0])
            cur, done, recs, msgs, calls = int(c[0]), int(d[0]), recs + rs[0], msgs + ms[0], calls + 1
            assert calls < 40
        assert (recs, msgs) == (whole[4], whole[3]) and len(set(recs)) == len(recs) and calls >= 3


# ------------------------------------------------------------------------------------------------ 3. batches
def test_batches_of_0_1_and_65_peers_with_every_status_and_start_rule(eng, s129):
    ss, m = s129
    assert answers_equal_model(eng, ss, m, []) == ([], [], [], [], [])
    answers_equal_model(eng, ss, m, [tfm.filt(crm.CHAIN, 1100, 5)], 1120 + 7200)
    kinds = [ALL, ALL[:41], tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF), tfm.filt(crm.FOREIGN, 0, 0xFFFFFFFF), tfm.filt(crm.CHAIN, 1090, 20), tfm.filt(crm.CHAIN, 0xFFFFFFFF, 1),
             ALL, tfm.filt(crm.CHAIN, 0, 0xFFFFFFFF, typ=266), tfm.filt(crm.CHAIN, 5, 5)]
    filters = [kinds[k % len(kinds)] for k in range(65)]
    budgets = [[None, 500, 0, -1, 4000][k % 5] for k in range(65)]
    model = answers_equal_model(eng, ss, m, filters, 1080 + 7200, budgets=budgets)
    assert set(model[0]) == {-1, 0, 1} and {0, 1} <= set(model[2])
    empty = [k for k in range(1, 64) if not model[3][k] and model[3][k - 1] and model[3][k + 1]]
    assert empty                                                                             # peers without an answer between peers with one


# ------------------------------------------------------------------------------------------------ 4. sizes
GUARD = 64


def raw_call(eng, ss, filters, now=NOW, pad=0, msg_cap=0, out_cap=0, host_out=True, d_out=None, cursors=None, budgets=None):
    """the C call itself, the filters behind `pad` bytes, every array pre-filled and followed by a guard region"""
    from lightning_amd import _ffi
    n = len(filters)
    foff = np.zeros(n + 1, dtype=np.uint64)
    foff[0] = pad
    foff[1:] = pad + np.cumsum([len(f) for f in filters], dtype=np.uint64) if n else pad
    blob = np.frombuffer(b"\xA5" * pad + b"".join(filters) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(crm.CHAIN, dtype=np.uint8)
    cur = None if cursors is None else np.array(list(cursors) + [0], dtype=np.uint64)
    bud = None if budgets is None else np.array(list(budgets) + [0], dtype=np.int64)
    status, cursor_out, done = np.full(n + GUARD, 99, dtype=np.int8), np.full(n + GUARD, 2 ** 64 - 1, dtype=np.uint64), np.full(n + GUARD, 0xEE, dtype=np.uint8)
    first, msg_off = np.full(n + 1 + GUARD, 2 ** 64 - 1, dtype=np.uint64), np.full(msg_cap + 1 + GUARD, 2 ** 64 - 1, dtype=np.uint64)
    msg_rec, out = np.full(msg_cap + GUARD, 0xABABABAB, dtype=np.uint32), np.full(out_cap + GUARD, 0xEE, dtype=np.uint8)
    s = _ffi.LamdFilterReplySummary()
    rc = eng._lib.lamd_timestamp_filter_reply_batch(eng._ctx, ss._h, chain.ctypes.data, now, n, blob.ctypes.data, foff.ctypes.data, None if cur is None else cur.ctypes.data,
                                                    None if bud is None else bud.ctypes.data, status.ctypes.data, cursor_out.ctypes.data, done.ctypes.data,
                                                    first.ctypes.data, msg_cap, msg_off.ctypes.data, msg_rec.ctypes.data,
                                                    out.ctypes.data if host_out and d_out is None else None, None if d_out is None else d_out.data_ptr(), out_cap,
                                                    ctypes.byref(s))
    return rc, status, cursor_out, done, first, msg_off, msg_rec, out, s


def untouched(a, used=0):
    fill = {np.dtype(np.uint64): 2 ** 64 - 1, np.dtype(np.uint8): 0xEE, np.dtype(np.int8): 99, np.dtype(np.uint32): 0xABABABAB}[a.dtype]
    return bool((a[used:] == fill).all())


def test_sizes_caps_one_short_and_every_output_form(eng, s129):
    import torch
    ss, m = s129
    filters = [tfm.filt(crm.CHAIN, 1060, 9), ALL[:30], tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF), ALL]
    budgets = [2 ** 63 - 1, 0, 2 ** 63 - 1, 700]
    model = tfm.answers(m, filters, crm.CHAIN, 1120 + 7200, None, [None, 0, None, 700])
    flat = b"".join(y for x in model[3] for y in x)
    M, total, n = sum(len(x) for x in model[3]), len(flat), len(filters)
    offs = list(np.cumsum([0] + [len(y) for x in model[3] for y in x]))
    firsts = list(np.cumsum([0] + [len(x) for x in model[3]]))
    call = lambda **kw: raw_call(eng, ss, filters, 1120 + 7200, budgets=budgets, **kw)

    def sizes_ok(status, cursor_out, done, first, s):
        assert (s.messages, s.bytes, s.finished) == (M, total, sum(model[2])) and [int(x) for x in status[:n]] == model[0]
        assert [int(x) for x in cursor_out[:n]] == model[1] and [int(x) for x in done[:n]] == model[2] and [int(x) for x in first[:n + 1]] == firsts
        assert untouched(status, n) and untouched(cursor_out, n) and untouched(done, n) and untouched(first, n + 1)
    for msg_cap, out_cap, host_out in ((0, 0, True), (0, 0, False), (M - 1, total, True), (M, total - 1, True)):      # the sizes alone; a cap one short
        rc, status, cursor_out, done, first, msg_off, msg_rec, out, s = call(msg_cap=msg_cap, out_cap=out_cap, host_out=host_out)
        assert rc == -3
        sizes_ok(status, cursor_out, done, first, s)
        assert all(untouched(a) for a in (msg_off, msg_rec, out))                            # (out was poisoned with 0xEE)
    for pad in range(4):                                                                     # host out, the filters at every alignment
        rc, status, cursor_out, done, first, msg_off, msg_rec, out, s = call(pad=pad, msg_cap=M, out_cap=total)
        assert rc == 0
        sizes_ok(status, cursor_out, done, first, s)
        assert out[:total].tobytes() == flat and [int(x) for x in msg_off[:M + 1]] == offs and [int(x) for x in msg_rec[:M]] == [y for x in model[4] for y in x]
        assert untouched(msg_off, M + 1) and untouched(msg_rec, M) and untouched(out, total)
    rc, *_, msg_off, msg_rec, out, s = call(msg_cap=M, host_out=False)                            # neither output: the offsets alone
    assert rc == 0 and int(msg_off[M]) == total and [int(x) for x in msg_rec[:M]] == [y for x in model[4] for y in x] and untouched(out)
    eng._after_torch()
    for shift in (0, 1, 2, 3):                                                               # the output left on the device
        d = torch.full((total + shift + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert call(msg_cap=M, out_cap=total, d_out=d[shift:])[0] == 0
        h = d.cpu().numpy()
        assert h[shift:shift + total].tobytes() == flat and set(h[:shift]) <= {0xEE} and set(h[shift + total:]) == {0xEE}
        d.fill_(0xEE)
        torch.cuda.synchronize()
        rc, *_, s = call(msg_cap=M, out_cap=total - 1, d_out=d[shift:])
        assert rc == -3 and s.bytes == total and set(d.cpu().numpy()) == {0xEE}
    rc, status, cursor_out, done, first, msg_off, *_, s = raw_call(eng, ss, [], msg_cap=1)          # np == 0
    assert rc == 0 and int(first[0]) == 0 and int(msg_off[0]) == 0 and s.messages == 0
    from lightning_amd import Engine
    from lightning_amd.engine import LamdError
    with Engine(0) as other, pytest.raises(LamdError):                                         # an index of another context
        other.timestamp_filter_replies(ss, filters, crm.CHAIN, NOW)


# ------------------------------------------------------------------------------------------------ 5. lifetime
def test_an_index_of_a_repairs_resident_output_and_of_an_owned_copy(eng):
    import torch
    blob = sa._golden("gossip_store_mesh_3x3.bin")                                           # (a repair keeps only records whose signatures hold)
    d_big = torch.full((len(blob) + 46,), 0xCD, dtype=torch.uint8, device="cuda")
    got = eng.gossip_store_repair(blob, bytes(range(32)), d_out=d_big, host_out=False)
    torch.cuda.synchronize()
    out_len = got[6]["out_len"]
    repaired = d_big.cpu().numpy().tobytes()[:out_len]
    recs = sa.walk(repaired)[0]
    m = tfm.index(repaired)
    image = d_big[:out_len]
    ss = eng.gossip_store_stream(rec_off=offsets(recs), d_store=image)
    del image, d_big                                                                         # the index keeps the tensor alive
    assert len(ss) == len(m["list"]) >= 3 and [int(x) for x in ss.read()[0]] == [e[0] for e in m["list"]]
    mid = sorted(m["hts"])[len(m["hts"]) // 2]
    answers_equal_model(eng, ss, m, [ALL, tfm.filt(crm.CHAIN, 1, 0xFFFFFFFF), tfm.filt(crm.CHAIN, mid, 30)], mid + 7200, budgets=[None, 500, None])
    ss.free()
    copy = bytearray(tile_store(70))
    ss = eng.gossip_store_stream(bytes(copy))
    m = tfm.index(bytes(copy))
    for k in range(len(copy)):                                                               # the host image is the index' own copy: the caller's may go
        copy[k] = 0
    del copy
    answers_equal_model(eng, ss, m, [ALL, tfm.filt(crm.CHAIN, 1030, 5)])
    ss.free()


# ------------------------------------------------------------------------------------------------ 6. a larger store
def big_store(n=600):
    """n channels with both updates over 87 nodes, two thirds of them announced: 2 400 records and the node_announcements; every 50th
    update deleted, every 70th dying, header timestamps that jump back every 97 records"""
    ids = [sqm.node_id(k, 2 + k % 2) for k in range(87)]
    recs = []
    for k in range(n):
        s = crm.scid_of(5000 + k // 2, k % 2, 1)
        stamp = lambda j: 1000 + 2 * k + j - (900 if k % 97 == 0 else 0)
        f0 = sa.F_COMPLETED | (sa.F_DELETED if k % 50 == 7 else 0)
        f1 = sa.F_COMPLETED | (tfm.F_DYING if k % 70 == 9 else 0)
        recs += [crm.fast_rec(sqm.cann_ids(s, ids[k % 50], ids[50 + k % 37]), 0), crm.fast_rec(crm.AMOUNT, 0), crm.fast_rec(crm.cupd(s, 0, stamp(0)), stamp(0), f0),
                 crm.fast_rec(crm.cupd(s, 1, stamp(1), 141), stamp(1), f1)]
    recs += [crm.fast_rec(sqm.nann(ids[k], 2300 + k, flen=k % 4, fill=k), 2300 + k) for k in range(87) if k % 3]
    return recs


def test_a_larger_store_and_65_random_peers(eng):
    blob = sa.serialise(0x10, big_store())
    ss, m = build(eng, blob)
    n = len(m["list"])
    assert n > 1700 and ss.summary["skipped_deleted"] == 12 and ss.summary["skipped_dying"] == 9 and ss.summary["skipped_type"] == 600
    rng = random.Random(65)
    filters, cursors, budgets = [], [], []
    for k in range(65):
        first = rng.choice([0, 1, 0xFFFFFFFF, rng.randrange(900, 2500), rng.randrange(900, 2500)])
        filters.append(tfm.filt(crm.FOREIGN if k % 16 == 5 else crm.CHAIN, first, rng.choice([0, 1, 10, 300, 5000, 0xFFFFFFFF]))[:42 - (k % 13 == 4)])
        cursors.append(None if k % 2 else rng.randrange(0, n + 1))
        budgets.append(rng.choice([None, -1, 0, 1000, 20000, 10 ** 6]))
    model = answers_equal_model(eng, ss, m, filters, 2000 + 7200, cursors, budgets)
    assert set(model[0]) == {-1, 0, 1} and sum(len(x) for x in model[3]) > 5000
    ss.free()

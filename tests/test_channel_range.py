"""The channel digest of a gossip_store image on the device and the query_channel_range answers from it (lamd_gossip_store_digest_build,
lamd_channel_range_reply_batch, include/lightning_amd.h) against the sequential model of channel_range_model.py: the digest entry for entry and
counter for counter, the replies byte for byte, and for every answered query the properties BOLT #7 asks of a series of replies.  The stores are
the two the reference's gossipd wrote, the synthetic store of test_store_audit and its damaged copy, and hand-built ones (no valid signatures: the
digest reads none).  The same code on the host, under the sanitizers, is test_store_digest_host's."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
COUNTERS = ("records", "channels", "entries", "channels_no_update", "updates_no_channel", "updates_in_front", "updates_short")


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def entries_of(dg):
    scid, ts, csum, rec = dg.read()
    return [(int(scid[j]), (int(ts[j][0]), int(ts[j][1])), (int(csum[j][0]), int(csum[j][1])), tuple(int(x) for x in rec[j])) for j in range(len(scid))]


def digest_equals_model(eng, blob, verdict=None):
    """builds the digest, compares it and its counters with the model -> (StoreDigest, the model's sorted entries)"""
    want, wc = crm.sorted_digest(blob, verdict)
    dg = eng.gossip_store_digest(blob, verdict=verdict)
    got = entries_of(dg)
    bad = [(j, a, b) for j, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad and len(got) == len(want) == len(dg), (len(got), len(want), bad[:5])
    assert {k: dg.summary[k] for k in COUNTERS} == wc
    return dg, want


def replies_have_the_properties(want, q, status, replies, ours=crm.CHAIN):
    """what BOLT #7 and the split's contract ask of the replies to one query"""
    p = crm.parse_query(q)
    if p is None:
        assert status == -1 and replies == []
        return
    chain, first, number, option = p
    if chain != ours:
        assert status == 1 and replies == [crm.encode(chain, first, number, [], 0, 0)[:43] + b"\x00\x00"]
        return
    assert status == 0 and len(replies) >= 1
    number = crm.fix_number(first, number)
    sel = crm.gather_range(want, first, number)
    ds = [crm.decode_reply(r) for r in replies]
    assert all(len(r) <= 65535 for r in replies) and all(d["chain"] == ours for d in ds)
    assert [s for d in ds for s in d["scids"]] == [e[0] for e in sel]                       # the replies concatenate to the sorted selection
    assert sum(d["blocks"] for d in ds) == number and ds[0]["first"] == first               # their blocks sum to the (fixed-up) request
    assert all(a["first"] + a["blocks"] == b["first"] for a, b in zip(ds, ds[1:]))          # first_blocknums chain
    assert [d["final"] for d in ds] == [0] * (len(ds) - 1) + [1]                            # exactly the last one is complete
    for d in ds:
        assert (d["ts"] is not None, d["csum"] is not None) == (bool(option & 1), bool(option & 2))
    if option & 1:
        assert [t for d in ds for t in d["ts"]] == [e[1] for e in sel]
    if option & 2:
        assert [c for d in ds for c in d["csum"]] == [e[2] for e in sel]


def answers_equal_model(eng, dg, want, queries, cap=0, chain=crm.CHAIN):
    status, replies = eng.channel_range_replies(dg, chain, queries, max_encoded_bytes=cap)
    assert len(status) == len(replies) == len(queries)
    memo = {}
    for k, q in enumerate(queries):
        if q not in memo:
            memo[q] = crm.replies(want, chain, q, cap)
            replies_have_the_properties(want, q, int(status[k]), replies[k], chain)
        assert (int(status[k]), replies[k]) == memo[q], (k, q.hex(), int(status[k]), memo[q][0], len(replies[k]), len(memo[q][1]))
    return status, replies


# ------------------------------------------------------------------------------------------------ the digest
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_digest_of_the_stores_the_reference_wrote(eng, name):
    blob = sa._golden(name)
    dg, want = digest_equals_model(eng, blob)
    with dg:
        assert len(want) == (1 if "simple" in name else 12) and dg.summary["channels_no_update"] == 0
        answers_equal_model(eng, dg, want, crm.query_kinds([e[0] >> 40 for e in want]))


def test_digest_of_the_synthetic_store_with_and_without_verdicts(eng, synthetic, damaged):
    img, (_, v, _) = synthetic
    dg, plain = digest_equals_model(eng, img)
    dg.close()
    dg, judged = digest_equals_model(eng, img, list(v))
    dg.close()
    assert judged == plain and len(plain) >= 12
    blob, (_, dv, _), _ = damaged
    dg, good = digest_equals_model(eng, blob, list(dv))
    with dg:
        answers_equal_model(eng, dg, good, crm.query_kinds([e[0] >> 40 for e in good]))
    dg, loose = digest_equals_model(eng, blob)
    dg.close()
    served = {r for e in good for r in e[3] if r != crm.NONE}
    assert all(dv[r] == 0 for r in served) and good != loose                                # bad records are not served


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 5000])
def test_digest_of_hand_built_stores_in_three_orders(eng, n):
    asc = [crm.scid_of(1000 + k // 3, k % 3, k & 1) for k in range(n)]
    shuffled = list(asc)
    random.Random(n).shuffle(shuffled)
    first = None
    for scids in (asc, asc[::-1], shuffled):
        dg, want = digest_equals_model(eng, crm.big_store(scids))
        dg.close()
        assert [e[0] for e in want] == asc
        key = [e[:1] for e in want]
        first = first or key
        assert key == first


def test_slot_cases(eng):
    blob, names = crm.slot_store()
    dg, want = digest_equals_model(eng, blob)
    with dg:
        by = {e[0]: e for e in want}
        recs = sa.walk(blob)[0]
        assert names["no_update"] not in by and dg.summary["channels_no_update"] == 1
        assert by[names["dir0"]][1] == (11, 0) and by[names["dir0"]][2][1] == 0 and by[names["dir0"]][3][2] == crm.NONE
        assert by[names["dir1"]][1] == (0, 12) and by[names["dir1"]][2][0] == 0 and by[names["dir1"]][3][1] == crm.NONE
        assert by[names["both"]][1] == (14, 13) and 0 not in by[names["both"]][2]
        assert by[names["replaced"]][1] == (8000, 0)                                        # the later record wins, lower timestamp or not
        assert by[names["deleted_behind"]][1] == (0, 20)
        assert by[names["in_front"]][1] == (0, 31) and dg.summary["updates_in_front"] == 1 and dg.summary["updates_no_channel"] == 1
        assert by[names["short"]][1] == (0, 51) and dg.summary["updates_short"] == 1 and len(recs[by[names["short"]][3][2]][4]) == 112
        a, u0, u1 = by[names["twice"]][3]
        assert by[names["twice"]][1] == (60, 61) and a < u0 < u1 and recs[a][4][:2] == b"\x01\x00" and dg.summary["channels"] == len(names)
        seen = set()
        for length in range(112, 151):
            for al in range(4):
                e = by[names["crc_%d_%d" % (length, al)]]
                u = e[3][1] if e[3][1] != crm.NONE else e[3][2]
                assert len(recs[u][4]) == length and recs[u][0] % 4 == al
                seen.add((length, recs[u][0] % 4))
        assert len(seen) == 39 * 4
        answers_equal_model(eng, dg, want, crm.query_kinds([s >> 40 for s in names.values()]))


def test_resident_image_at_odd_addresses_and_the_return_codes(eng):
    import torch
    from lightning_amd import _ffi
    from lightning_amd.engine import LamdError, gossip_store_frame
    blob, _ = crm.slot_store()
    want = crm.sorted_digest(blob)[0]
    off = gossip_store_frame(blob)[0]
    for shift in (0, 1, 2, 3):
        d = torch.zeros(len(blob) + shift, dtype=torch.uint8, device="cuda")
        d[shift:] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        with eng.gossip_store_digest(None, rec_off=off, d_store=d[shift:]) as dg:
            assert entries_of(dg) == want
    # offsets that point anywhere: nothing is read outside the image, records that are none do not count
    wild = np.array(list(off[:40]) + [len(blob) - 5, len(blob), len(blob) + 1, 2 ** 63, 2 ** 64 - 1, 3], dtype=np.uint64)
    with eng.gossip_store_digest(blob, rec_off=wild) as dg:
        got = entries_of(dg)
        assert len(got) <= 40 and dg.summary["records"] == len(wild)
    lib, ctx = eng._lib, eng._ctx
    h, s = ctypes.c_void_p(), _ffi.LamdStoreDigestSummary()
    assert lib.lamd_gossip_store_digest_build(ctx, None, 0, None, 0, None, None, ctypes.byref(h), ctypes.byref(s)) == -3
    buf = np.frombuffer(blob, dtype=np.uint8)
    assert lib.lamd_gossip_store_digest_build(ctx, buf.ctypes.data, len(blob), None, 5, None, None, ctypes.byref(h), ctypes.byref(s)) == -3
    with eng.gossip_store_digest(blob) as dg:
        one = np.zeros(1, dtype=np.uint64)
        assert lib.lamd_store_digest_read(dg._h, len(dg) - 1, one.ctypes.data, None, None, None) == -3
        with pytest.raises(LamdError):
            eng._chk(lib.lamd_channel_range_reply_batch(ctx, dg._h, None, 0, None, None, 0, None, None, 0, None, None, None, 0, None))


# ------------------------------------------------------------------------------------------------ the replies
@pytest.fixture(scope="module")
def mesh(eng):
    blob = sa._golden("gossip_store_mesh_3x3.bin")
    want = crm.sorted_digest(blob)[0]
    with eng.gossip_store_digest(blob) as dg:
        yield dg, want


@pytest.mark.parametrize("count", [1, 64, 65, 300])
def test_batches_of_mixed_queries(eng, mesh, count):
    dg, want = mesh
    queries = crm.mixed_queries([e[0] >> 40 for e in want], count)
    status, replies = answers_equal_model(eng, dg, want, queries)
    if count >= 64:
        assert {-1, 0, 1} == set(int(x) for x in status)
        # the good queries' replies do not depend on what stands between them
        good = [q for q in queries if crm.parse_query(q) is not None]
        s2, r2 = eng.channel_range_replies(dg, crm.CHAIN, good)
        assert [r for r, s in zip(replies, status) if s != -1] == r2 and -1 not in set(int(x) for x in s2)


@pytest.mark.parametrize("limit", [1, 2, 3, 7])
def test_splits_at_small_limits(eng, limit):
    pops = [p for p in (1, limit - 1, limit, limit + 1, 3 * limit + 1) if p]
    blocks = [100 + 3 * k for k in range(len(pops))]
    dg, want = digest_equals_model(eng, crm.population_store(pops))
    with dg:
        assert len(want) == sum(pops)
        queries = crm.mixed_queries(blocks, 70)
        status, replies = answers_equal_model(eng, dg, want, queries, cap=8 * limit)
        assert crm.limit(0, 8 * limit) == limit
        whole = replies[queries.index(crm.query(crm.CHAIN, 0, 0xFFFFFFFF))]                 # no options: `limit` entries per reply at the most
        sizes = [len(crm.decode_reply(r)["scids"]) for r in whole]
        assert max(sizes) == limit and sum(sizes) == sum(pops) and len(whole) >= len(pops)
        answers_equal_model(eng, dg, want, queries[:9], cap=24 * limit)                    # the same limit for queries with both options


def test_one_reply_is_full_at_8186_entries(eng):
    scids = [crm.scid_of(200000 + k, 1, 0) for k in range(8187)]
    dg, want = digest_equals_model(eng, crm.big_store(scids[::-1]))
    with dg:
        q = crm.query(crm.CHAIN, 0, 0xFFFFFFFF)
        status, replies = answers_equal_model(eng, dg, want, [q, crm.query(crm.CHAIN, 0, 0xFFFFFFFF, 3)])
        assert [len(crm.decode_reply(r)["scids"]) for r in replies[0]] == [8186, 1]
        assert [len(crm.decode_reply(r)["scids"]) for r in replies[1]] == [2728, 2728, 2728, 3]
        assert len(replies[0][0]) == 46 + 8 * 8186 <= 65535


def test_caps_one_short_and_guard_regions(eng, mesh):
    import torch
    from lightning_amd import _ffi
    dg, want = mesh
    queries = crm.mixed_queries([e[0] >> 40 for e in want], 20)
    status, replies = eng.channel_range_replies(dg, crm.CHAIN, queries, max_encoded_bytes=16)
    flat = [r for rs in replies for r in rs]
    n_msgs, total = len(flat), sum(len(r) for r in flat)
    assert n_msgs > len(queries)
    lib, ctx = eng._lib, eng._ctx
    nq = len(queries)
    qoff = np.zeros(nq + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    blob = np.frombuffer(b"".join(queries) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(crm.CHAIN, dtype=np.uint8)
    GUARD = 64

    def call(msg_cap, out_cap, d_out=None):
        st, first = np.full(nq, 99, dtype=np.int8), np.full(nq + 1, 2 ** 64 - 1, dtype=np.uint64)
        msg_off, out = np.full(n_msgs + 1 + GUARD, 2 ** 64 - 1, dtype=np.uint64), np.full(total + GUARD, 0xEE, dtype=np.uint8)
        s = _ffi.LamdRangeReplySummary()
        rc = lib.lamd_channel_range_reply_batch(ctx, dg._h, chain.ctypes.data, nq, blob.ctypes.data, qoff.ctypes.data, 16, st.ctypes.data, first.ctypes.data, msg_cap,
                                                msg_off.ctypes.data, None if d_out is not None else out.ctypes.data, None if d_out is None else d_out.data_ptr(),
                                                out_cap, ctypes.byref(s))
        return rc, st, first, msg_off, out, s
    rc, st, first, msg_off, out, s = call(n_msgs, total)
    assert rc == 0 and (s.messages, s.bytes) == (n_msgs, total) and list(st) == list(status)
    assert out[:total].tobytes() == b"".join(flat) and set(out[total:]) == {0xEE} and set(int(x) for x in msg_off[n_msgs + 1:]) == {2 ** 64 - 1}
    assert int(msg_off[0]) == 0 and int(msg_off[n_msgs]) == total and int(first[nq]) == n_msgs
    for msg_cap, out_cap in ((n_msgs - 1, total), (n_msgs, total - 1), (0, 0)):
        rc, st, first, msg_off, out, s = call(msg_cap, out_cap)
        assert rc == -3 and (s.messages, s.bytes) == (n_msgs, total) and list(st) == list(status) and int(first[nq]) == n_msgs
        assert set(out) == {0xEE} and set(int(x) for x in msg_off) == {2 ** 64 - 1}        # nothing is written
    eng._after_torch()
    for shift in (0, 1, 2, 3):                                                              # the output left on the device, at every alignment
        d = torch.full((total + shift + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, _, _, _, _, s = call(n_msgs, total, d_out=d[shift:])
        assert rc == 0
        h = d.cpu().numpy()
        assert h[shift:shift + total].tobytes() == b"".join(flat) and set(h[:shift]) <= {0xEE} and set(h[shift + total:]) == {0xEE}
        rc, _, _, _, _, s = call(n_msgs, total - 1, d_out=d[shift:])
        assert rc == -3 and s.bytes == total


def test_digest_of_a_repaired_store_left_on_the_device(eng, damaged):
    import torch
    blob = damaged[0]
    d_out = torch.zeros(len(blob) + 46, dtype=torch.uint8, device="cuda")
    out, _, _, new_off, reason, _, rs = eng.gossip_store_repair_latest(blob, bytes(range(32)), d_out=d_out)
    kept = [int(o) for o, r in zip(new_off, reason) if r == 0]
    rec_off = np.array([1] + kept, dtype=np.uint64)                                         # the uuid record, then the kept ones
    assert list(rec_off) == [r[0] for r in sa.walk(out)[0]] and rs["out_len"] == len(out)
    want, wc = crm.sorted_digest(out)
    with eng.gossip_store_digest(None, rec_off=rec_off, d_store=d_out[:len(out)]) as dg:
        assert entries_of(dg) == want and {k: dg.summary[k] for k in COUNTERS} == wc and len(want) >= 8
        assert wc["updates_no_channel"] == wc["updates_in_front"] == wc["updates_short"] == 0
        answers_equal_model(eng, dg, want, crm.query_kinds([e[0] >> 40 for e in want]))

"""The store pipeline on the device -- audit, repair, latest-wins repair, digest, query_channel_range, reply_channel_range comparison,
query_short_channel_ids, gossip_timestamp_filter, channel_update receive -- on inputs nobody here authored: the mainnet excerpt, the canned
regtest store and the BOLT #7 vectors the reference ships (tests/golden/make_reference_stores.py; what they hold and what the reference's own
tests assert of them: test_reference_stores.py, which ties the sequential models to the same facts on the CPU).  Every comparison is exact:
with the models through the helpers of the feature's own GPU test, and with the reference's literals read from tests/golden/bolt7_vectors.json."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import range_compare_model as rcm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_channel_range as tcr  # noqa: E402
import test_gpu_range_compare as trc  # noqa: E402
import test_gpu_scid_query as tsq  # noqa: E402
import test_gpu_timestamp_filter as ttf  # noqa: E402
import test_gpu_update_receive as tur  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402
import test_store_latest as sl  # noqa: E402
import test_store_repair as sr  # noqa: E402
import timestamp_filter_model as tfm  # noqa: E402
import update_receive_model as urm  # noqa: E402

pytestmark = pytest.mark.gpu
H = bytes.fromhex
IMAGES = ("part1", "mainnet", "canned")


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def ref(orc):
    """name -> (image, the audit model's (offsets, verdicts, summary)), each computed once"""
    return {name: (rs.store(name), sa.model(orc, rs.store(name))) for name in IMAGES + ("fixed",)}


@pytest.fixture(scope="module")
def vec():
    return rs.vectors()


def checksum_store(vec):
    """two channels, 103x1x0 and 109x1x0, and the two updates of the reference's checksum test as their records: both are direction 0 of their
    channel; the first, of 130 bytes, is the one update in the suite without htlc_maximum_msat"""
    ups = [H(p["update"]) for p in vec["update_checksums"]]
    scids = [rs.scid("103x1x0"), rs.scid("109x1x0")]
    assert [int.from_bytes(m[98:106], "big") for m in ups] == scids and [m[111] & 1 for m in ups] == [0, 0] and [len(m) for m in ups] == [130, 138]
    recs = []
    for k, (s, m) in enumerate(zip(scids, ups)):
        recs += [crm.rec(crm.cann(s, k)), crm.rec(crm.AMOUNT), crm.rec(m, int.from_bytes(m[106:110], "big"))]
    return sa.serialise(0x10, recs), scids


# ------------------------------------------------------------------------------------------------ 1. the audit
@pytest.mark.parametrize("name", IMAGES + ("fixed",))
def test_audit_from_host_memory_and_from_a_resident_copy(eng, ref, name):
    import torch
    blob, want = ref[name]
    n, counts, sigs = rs.COUNTS[name]                                                                          # fixed: the tombstone's CRC corrected
    got = eng.gossip_store_audit(blob)
    sa._same(got, want)
    v = [int(x) for x in got[1]]
    assert (len(v), {k: v.count(k) for k in set(v)}, got[2]["signatures"]) == (n, counts, sigs)                # the counts, independently of the model
    assert got[2]["clean"] == (0 if name == "mainnet" else 1) and got[2]["bad_signature"] == [0, 0, 0, 0]
    for shift in (0, 3):                                                                                       # resident, at an odd device address too
        d = torch.zeros(len(blob) + shift, dtype=torch.uint8, device="cuda")
        d[shift:] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        sa._same(eng.gossip_store_audit(blob, d_store=d[shift:]), want)


def test_the_tombstone_alone_fails_and_its_correction_cleans_the_store(eng, ref):
    blob, _ = ref["mainnet"]
    off, v, s = eng.gossip_store_audit(blob)
    bad = [i for i, x in enumerate(v) if int(x) not in (sa.OK, sa.DELETED)]
    assert bad == [len(v) - 1] and int(off[-1]) == rs.TOMBSTONE_OFF and int(v[-1]) == sa.BAD_CHECKSUM and s["bad_checksum"] == 1
    assert blob[rs.TOMBSTONE_OFF + 12:rs.TOMBSTONE_OFF + 14] == struct.pack(">H", 4103)
    fixed, want = ref["fixed"]
    got = eng.gossip_store_audit(fixed)
    sa._same(got, want)
    assert got[2]["clean"] == 1 and got[2]["signatures"] == 356 and got[2]["ok"] == 180 and got[2]["skipped_deleted"] == 6


# ------------------------------------------------------------------------------------------------ 2. repair and latest-wins repair
@pytest.mark.parametrize("name", IMAGES)
def test_repair_equals_the_model_audits_clean_and_repairs_to_itself(eng, ref, name):
    blob, (_, v, _) = ref[name]
    want = sr.repair_model(blob, v, sr.UUID)
    got = eng.gossip_store_repair(blob, sr.UUID)
    sr._same(got, blob, v, want)
    if name != "mainnet":                                                                    # clean: what compactd's first phase writes
        assert got[0] == sr.compactd_first_phase(blob, sr.UUID) and set(want[0]) == {sr.KEPT, sr.R_DELETED}
    else:
        # the tombstone for its checksum; and the announcement in front of it, the one live announcement with no channel_amount behind it
        recs = sa.walk(blob)[0]
        assert [(i, x) for i, x in enumerate(want[0]) if x not in (sr.KEPT, sr.R_DELETED)] == [(184, sr.R_DEPENDENCY), (185, sr.R_VERDICT)]
        assert recs[184][4][:2] == b"\x01\x00" and recs[185][4][:2] == b"\x10\x07"
    kept = want[0].count(sr.KEPT)
    _, _, s = eng.gossip_store_audit(got[0])
    assert s["clean"] == 1 and s["records"] == kept + 1 == s["ok"]
    again = eng.gossip_store_repair(got[0], sr.UUID)
    assert again[0] == got[0] and again[6]["kept"] == kept and again[6]["dropped_bookkeeping"] == 1


def test_repair_drops_the_corrected_tombstone_as_store_bookkeeping(eng, ref):
    blob, (_, v, _) = ref["fixed"]
    want = sr.repair_model(blob, v, sr.UUID)
    got = eng.gossip_store_repair(blob, sr.UUID)
    sr._same(got, blob, v, want)
    assert int(got[4][-1]) == sr.R_BOOKKEEPING and got[6]["dropped_bookkeeping"] == 1 and got[6]["dropped_verdict"] == 0
    # The output is the one of the image as shipped: valid or not, the tombstone's own record is dropped and nothing is dropped because of it.
    # The channel it names, 686386x1093x1, is written out again with its amount record -- common/gossmap.c and pyln, which apply a valid tombstone,
    # would have dropped it from this input: the deliberate difference that test_a_valid_tombstone_is_not_applied_... below pins.  (The
    # R_DEPENDENCY in front of the tombstone is the announcement of another channel, which has the tombstone where its amount record should be.)
    assert got[0] == eng.gossip_store_repair(ref["mainnet"][0], sr.UUID)[0]
    assert [int(x) for x in got[4][rs.TOMBSTONED_ANN:]] == [sr.KEPT, sr.KEPT, sr.R_DEPENDENCY, sr.R_BOOKKEEPING] and want[0].count(sr.KEPT) == rs.KEPT["fixed"]
    assert rs.scid("686386x1093x1") in trc.bare_equals_model(eng, got[0])


@pytest.mark.parametrize("name", IMAGES)
def test_latest_wins_repair_at_the_stores_own_clock(eng, ref, name):
    """now = the newest header timestamp + 1, the reference's intervals.  At the default prune_interval of 1 209 600 s the model drops NO record
    as stale -- the updates of each image lie within 29 hours of its newest record -- so every live update survives and no wider interval is needed;
    nothing is superseded either (gossipd had deleted what it replaced), so the output is the plain repair's"""
    blob, (_, v, _) = ref[name]
    pol = dict(now=rs.newest(blob) + 1, future_slack=sl.SLACK, prune_interval=sl.PRUNE)
    want = sl.latest_model(blob, v, sl.UUID, **pol)
    got = eng.gossip_store_repair_latest(blob, sl.UUID, **pol)
    sl._same(got, blob, v, want)
    live_updates = [i for i, deleted, _ in rs.updates_in(blob) if not deleted]
    assert live_updates and all(want[0][i] == sl.KEPT for i in live_updates)
    assert not {sl.R_STALE, sl.R_SUPERSEDED, sl.R_TIMESTAMP} & set(want[0]) and want[2] == sr.repair_model(blob, v, sr.UUID)[2]
    stamps = [int.from_bytes(m[106:110], "big") for _, deleted, m in rs.updates_in(blob) if not deleted]
    assert pol["now"] - min(stamps) < 29 * 3600 < sl.PRUNE
    sl._closure(eng, got[0], pol, want[0].count(sl.KEPT))


# ------------------------------------------------------------------------------------------------ 3. the digest and the bare list
@pytest.mark.parametrize("name,entries,bare", [("mainnet", 4, 84), ("canned", 2, 0)])
def test_digest_and_bare_list(eng, ref, vec, name, entries, bare):
    blob, (_, v, _) = ref[name]
    for verdict in (None, v):
        dg, want = tcr.digest_equals_model(eng, blob, verdict)
        dg.close()
        assert len(want) == entries and len(trc.bare_equals_model(eng, blob, verdict)) == bare
    if name == "canned":
        lit = vec["canned"]
        e = {x[0]: x for x in want}[rs.scid(lit["scid"])]
        assert e[1] == tuple(d["timestamp"] for d in lit["directions"]) == (1700115313, 1700115313)


def test_a_valid_tombstone_is_not_applied_where_the_references_loaders_would_apply_it(eng, ref):
    """the deliberate difference test_reference_stores pins for the models, on the device: with the tombstone's CRC corrected common/gossmap.c
    and pyln would drop 686386x1093x1 and the node that has no other channel (87 channels, 125 nodes); flags alone decide here, so digest, bare
    list and directory keep both (88 channels of which 84 bare, 126 nodes), and a query for the channel is answered with its announcement"""
    blob, (_, v, _) = ref["fixed"]
    gone, lonely = rs.tombstone_divergence(blob, v)
    for verdict in (None, v):
        dg, want = tcr.digest_equals_model(eng, blob, verdict)
        with dg:
            assert dg.summary["channels"] == 88 and dg.summary["channels_no_update"] == 84
        bare = trc.bare_equals_model(eng, blob, verdict)
        assert len(want) == 4 and len(bare) == 84 and gone in bare and gone not in [e[0] for e in want]
    dr, m = tsq.build(eng, blob, v)
    ids = [bytes(x) for x in dr.nodes()[0]]
    assert len(ids) == 126 and lonely in ids and gone in m["chan"]
    model = tsq.answers_equal_model(eng, dr, m, [sqm.query(rs.MAINNET, [gone], [0x1f])], chain=rs.MAINNET)
    dr.free()
    ann = sa.walk(blob)[0][rs.TOMBSTONED_ANN][4]
    assert model[0] == [0] and model[2] == [[ann, struct.pack(">H", 262) + rs.MAINNET + b"\x01"]] and sa._cann_scid(ann)[0] == gone


def test_digest_checksums_are_the_references(eng, vec):
    blob, scids = checksum_store(vec)
    dg, want = tcr.digest_equals_model(eng, blob)
    with dg:
        got = tcr.entries_of(dg)
    sums = [p["checksum"] for p in vec["update_checksums"]]
    assert sums == [0x1112fa30, 0xf32ce968]
    assert [(e[0], e[2]) for e in got] == [(scids[0], (sums[0], 0)), (scids[1], (sums[1], 0))]
    assert [e[1] for e in got] == [(0x5d50f933, 0), (0x5d50f935, 0)]


# ------------------------------------------------------------------------------------------------ 4. query_channel_range
BLOCKS = (34_999, 35_000, 35_099, 35_100, 99_999, 100_000, 101_499, 101_500)


def test_the_vector_queries_select_their_blocks(eng, vec):
    q1, q2 = vec["extended_queries"][:2]
    chain = H(q1["msg"]["chainHash"])
    blob = crm.channel_store([crm.scid_of(b, 1, 0) for b in BLOCKS], both=True)
    dg, want = tcr.digest_equals_model(eng, blob)
    with dg:
        queries = [H(q1["hex"]), H(q2["hex"])]
        status, replies = tcr.answers_equal_model(eng, dg, want, queries, chain=chain)
        assert [int(x) for x in status] == [0, 0] and [len(r) for r in replies] == [1, 1]
        for q, r in zip((q1, q2), replies):
            first, number = q["msg"]["firstBlockNum"], q["msg"]["numberOfBlocks"]
            inside = [crm.scid_of(b, 1, 0) for b in BLOCKS if first <= b < first + number]               # from the JSON's numbers
            d = crm.decode_reply(r[0])
            assert (d["chain"], d["first"], d["blocks"], d["final"], d["scids"]) == (chain, first, number, 1, inside)
            assert (d["ts"] is not None, d["csum"] is not None) == (bool(q["msg"]["extensions"]),) * 2
        assert [s >> 40 for s in crm.decode_reply(replies[0][0])["scids"]] == [100_000, 101_499] and not vec["extended_queries"][0]["msg"]["extensions"]
        assert [s >> 40 for s in crm.decode_reply(replies[1][0])["scids"]] == [35_000, 35_099] and vec["extended_queries"][1]["msg"]["extensions"]
        by = {e[0]: e for e in want}
        d = crm.decode_reply(replies[1][0])
        assert d["ts"] == [by[s][1] for s in d["scids"]] and d["csum"] == [by[s][2] for s in d["scids"]]
        status, replies = tcr.answers_equal_model(eng, dg, want, queries)                              # under another chain they are foreign
        assert [int(x) for x in status] == [1, 1]


def test_the_checksum_tlv_carries_the_reference_checksums(eng, vec):
    blob, scids = checksum_store(vec)
    dg, want = tcr.digest_equals_model(eng, blob)
    with dg:
        status, replies = tcr.answers_equal_model(eng, dg, want, [crm.query(crm.CHAIN, 0, 0xFFFFFFFF, 2)])
    d = crm.decode_reply(replies[0][0])
    assert int(status[0]) == 0 and d["scids"] == scids and d["ts"] is None
    assert d["csum"] == [(p["checksum"], 0) for p in vec["update_checksums"]]


def test_mixed_queries_over_the_mainnet_digest(eng, ref):
    blob, _ = ref["mainnet"]
    dg, want = tcr.digest_equals_model(eng, blob)
    with dg:
        status, _ = tcr.answers_equal_model(eng, dg, want, crm.mixed_queries([e[0] >> 40 for e in want], 65, rs.MAINNET), chain=rs.MAINNET)
    assert {-1, 0, 1} == set(int(x) for x in status)


# ------------------------------------------------------------------------------------------------ 5. reply_channel_range comparison
def test_the_vector_reply_against_an_empty_digest_and_against_one_known_channel(eng, vec):
    rep = vec["extended_queries"][2]
    chain, first, number, _, scids, ts, _ = rs.reply_fields(rep)
    msg, want = H(rep["hex"]), [(122334, 123834)]
    assert scids == sorted(scids) and (first, first + number) == want[0]
    empty = crm.channel_store([])
    with eng.gossip_store_digest(empty) as dg:
        m = trc.compare_equals_model(eng, dg, [], [], [msg], want=want, chain=chain)
        assert (m[0], m[1], m[2], m[3]) == ([0], [(3, 3, 0)], scids, [])
    known = rs.scid("0x7x30934")
    ours = (489645, 4786863)
    blob = sa.serialise(0x10, [crm.rec(crm.cann(known)), crm.rec(crm.AMOUNT), crm.rec(crm.cupd(known, 0, ours[0]), ours[0]), crm.rec(crm.cupd(known, 1, ours[1]), ours[1])])
    entries = crm.sorted_digest(blob)[0]
    assert [(e[0], e[1]) for e in entries] == [(known, ours)]
    theirs = ts[scids.index(known)]
    flags = (2 if theirs[0] > ours[0] else 0) | (4 if theirs[1] > ours[1] else 0)                     # want_update(): theirs is newer than ours
    with eng.gossip_store_digest(blob) as dg:
        m = trc.compare_equals_model(eng, dg, entries, [], [msg], want=want, chain=chain)
        assert flags == 4 and (m[0], m[1], m[2], m[3], m[4]) == ([0], [(3, 2, 1)], [s for s in scids if s != known], [known], [4])
        outside = rcm.parse(msg, chain, (0, 100))[0]
        m = trc.compare_equals_model(eng, dg, entries, [], [msg], want=[(0, 100)], chain=chain)
        assert outside == 4 and m[0] == [4] and m[2] == m[3] == []


def test_probe_replies_over_the_mainnet_digest_and_its_bare_channels(eng, ref):
    blob, _ = ref["mainnet"]
    entries, bare = crm.sorted_digest(blob)[0], rcm.bare(blob)
    assert (len(entries), len(bare)) == (4, 84)
    with eng.gossip_store_digest(blob) as dg:
        m = trc.compare_equals_model(eng, dg, entries, bare, rcm.probe_replies(entries, bare, rs.MAINNET), chain=rs.MAINNET)
    assert set(bare) & set(m[3]) and not set(bare) & set(m[2]) and {2, 4} <= set(m[4])                # a bare channel is known, and stale for any timestamp


# ------------------------------------------------------------------------------------------------ 6. query_short_channel_ids
def test_the_vector_query_against_a_directory_that_knows_one_of_its_channels(eng, vec):
    q = vec["extended_queries"][3]
    chain, known = H(q["msg"]["chainHash"]), rs.scid("0x0x15465")
    assert [rs.scid(s) for s in q["msg"]["shortChannelIds"]["array"]].count(known) == 1
    blob = crm.channel_store([known], both=True)
    dr, m = tsq.build(eng, blob)
    model = tsq.answers_equal_model(eng, dr, m, [H(q["hex"])], chain=chain)
    dr.free()
    recs = sa.walk(blob)[0]
    assert model[0] == [0] and model[1] == [(3, 1, 3, 0)]
    assert model[2] == [[recs[0][4], recs[2][4], recs[3][4], struct.pack(">H", 262) + chain + b"\x01"]]


def test_the_mainnet_directory_and_every_flag_on_every_channel(eng, ref):
    blob, (_, v, _) = ref["mainnet"]
    chain = rs.chain_of(blob)
    assert chain == rs.MAINNET
    dr, m = tsq.build(eng, blob, v)
    ids, _, nann = dr.nodes()
    assert len(ids) == 126 and [bytes(x) for x in ids] == sorted({bytes(x) for x in ids}) and all(int(x) == sqm.NONE for x in nann)
    queries = sqm.flag_queries(m, chain)
    assert len(queries) == 32 * 88 + 4
    model = tsq.answers_equal_model(eng, dr, m, queries, chain=chain)
    dr.free()
    recs = m["recs"]
    for k, s in enumerate(sorted(m["chan"])):
        for f in range(32):
            msgs = model[2][32 * k + f]
            assert not any(x[:2] == b"\x01\x01" for x in msgs) and msgs[-1] == struct.pack(">H", 262) + chain + b"\x01"
            if f & 1:
                assert msgs[0] == recs[m["chan"][s][0]][4] and sa._cann_scid(msgs[0])[0] == s             # the stored announcement, byte for byte
            assert len(msgs) == 1 + sum(1 for b in range(3) if f >> b & 1 and m["chan"][s][b] != sqm.NONE)


def test_the_canned_directory_returns_its_node_announcements_once_each_in_memcmp_order(eng, ref, vec):
    blob, (_, v, _) = ref["canned"]
    chain = rs.chain_of(blob)
    dr, m = tsq.build(eng, blob, v)
    chans = sorted(m["chan"])
    model = tsq.answers_equal_model(eng, dr, m, [sqm.query(chain, chans + chans[::-1], [0x18] * 4), sqm.query(chain, chans)], chain=chain)
    dr.free()
    nanns = [x for x in model[2][0] if x[:2] == b"\x01\x01"]
    ids = [x[72 + int.from_bytes(x[66:68], "big"):][:33] for x in nanns]
    assert len(model[2][0]) == 4 and len(nanns) == 3 and ids == sorted(set(ids)) == m["nodes"] and all(H(x) in ids for x in vec["canned"]["node_ids"])
    assert [x for x in model[2][1] if x[:2] == b"\x01\x01"] == nanns and model[1][1] == (2, 2, 6, 3)


# ------------------------------------------------------------------------------------------------ 7. gossip_timestamp_filter
def test_the_mainnet_stream_index_the_filter_corpus_and_a_resumed_budget(eng, ref):
    blob, _ = ref["mainnet"]
    ss, m = ttf.build(eng, blob)
    assert m["counters"]["streamable"] == 92 == len(ss) and m["counters"]["skipped_deleted"] == 6 and m["counters"]["skipped_type"] == 88
    now = rs.newest(blob) + 100
    everything = tfm.filt(rs.MAINNET, 0, 0xFFFFFFFF)
    model = ttf.answers_equal_model(eng, ss, m, tfm.corpus(rs.MAINNET) + [everything], now, chain=rs.MAINNET)
    assert set(model[0]) == {-1, 0, 1} and len(model[3][-1]) == 92
    cur, done, recs, msgs, calls = tfm.AS_FILTER, 0, [], [], 0
    while not done:                                                                          # 1 000 bytes a call, resumed until done
        st, c, d, ms, rc = eng.timestamp_filter_replies(ss, [everything], rs.MAINNET, now, [cur], [1000], return_records=True)
        assert tfm.answer(m, everything, rs.MAINNET, now, cur, 1000) == (int(st[0]), int(c[0]), int(d[0]), ms[0], rc[0])
        cur, done, recs, msgs, calls = int(c[0]), int(d[0]), recs + rc[0], msgs + ms[0], calls + 1
        assert calls < 60
    ss.free()
    walked = sa.walk(blob)[0]
    assert recs == [e[0] for e in m["list"]] == sorted(recs) and len(recs) == 92 and msgs == [walked[i][4] for i in recs] and calls >= 20


# ------------------------------------------------------------------------------------------------ 8. channel_update receive
@pytest.fixture(scope="module")
def batch(ref):
    """the 8 channel_updates found in part 1 + part 2, the deleted ones included, in file order: real signatures of foreign implementations"""
    ups = rs.updates_in(ref["mainnet"][0])
    assert len(ups) == 8 and sum(1 for u in ups if u[1]) == 4 and all(len(u[2]) == 138 and u[2][66:98] == rs.MAINNET for u in ups)
    return ups


def test_receiving_the_stores_own_updates(eng, orc, ref, batch):
    blob, _ = ref["mainnet"]
    msgs = [m for _, _, m in batch]
    now = rs.newest(blob) + 1
    with tur.Resident(eng, blob, chain=rs.MAINNET) as res:
        want, _, s = tur.equals_model(orc, res, msgs, chain=rs.MAINNET, now=now)
        assert s["signature_rows"] == 8 and urm.BAD_SIGNATURE not in want["status"]
        assert all(want["status"][k] == urm.DUPLICATE for k, (_, deleted, _) in enumerate(batch) if not deleted)
        flipped = [m[:40] + bytes([m[40] ^ 1]) + m[41:] for m in msgs]                       # one bit of each signature's s
        bad, plan, _ = tur.equals_model(orc, res, flipped, chain=rs.MAINNET, now=now)
        assert urm.ACCEPTED not in bad["status"] and set(bad["status"]) == {urm.BAD_SIGNATURE} and not plan["records"]


def test_receiving_them_against_part_1_alone_closes_the_loop(eng, orc, ref, batch):
    from lightning_amd.engine import apply_update_plan, gossip_store_frame
    blob, _ = ref["part1"]
    msgs = [m for _, _, m in batch]
    now = rs.newest(ref["mainnet"][0]) + 1
    part1_scids = {sa._cann_scid(r[4])[0] for r in sa.walk(blob)[0] if not r[1] & sa.F_DELETED and sa._cann_scid(r[4])}
    with tur.Resident(eng, blob, chain=rs.MAINNET) as res:
        want, plan, _ = tur.equals_model(orc, res, msgs, chain=rs.MAINNET, now=now)
        later = [k for k, m in enumerate(msgs) if int.from_bytes(m[98:106], "big") not in part1_scids]
        assert later and all(want["status"][k] == urm.UNKNOWN for k in later) and want["status"].count(urm.UNKNOWN) == len(later)
        assert want["status"].count(urm.ACCEPTED) == rs.PART1_RECEIVE["accepted"] and len(later) == rs.PART1_RECEIVE["unknown"] and plan["records"]
        # one bit of each signature's s flipped, here where the unflipped batch has updates ACCEPTED: exactly those, and the other signed ones
        # unless decided in front of the signature batch, now fail it; nothing is accepted and nothing planned
        flipped = [m[:40] + bytes([m[40] ^ 1]) + m[41:] for m in msgs]
        bad, bad_plan, bs = tur.equals_model(orc, res, flipped, chain=rs.MAINNET, now=now)
        assert urm.ACCEPTED not in bad["status"] and not bad_plan["records"] and bs["signature_rows"] == rs.PART1_RECEIVE["signed"]
        assert all(b == urm.BAD_SIGNATURE for a, b in zip(want["status"], bad["status"]) if a == urm.ACCEPTED)
        assert [b for k, b in enumerate(bad["status"]) if k in later] == [urm.UNKNOWN] * len(later)
        image, rec_off = apply_update_plan(blob, gossip_store_frame(blob)[0], plan)
    assert image == urm.apply(blob, res.v, want)
    off, verdict, s = eng.gossip_store_audit(image)[:3]
    assert s["clean"] == 1 and [int(x) for x in off] == [int(x) for x in rec_off] and s["records"] == 94 + want["status"].count(urm.ACCEPTED)
    with tur.Resident(eng, image, list(verdict), chain=rs.MAINNET) as res2:
        again, plan2, _ = tur.equals_model(orc, res2, msgs, chain=rs.MAINNET, now=now)
        assert all(b in (urm.STALE, urm.DUPLICATE) for a, b in zip(want["status"], again["status"]) if a == urm.ACCEPTED) and not plan2["records"]
        assert [b for a, b in zip(want["status"], again["status"]) if a != urm.ACCEPTED] == [a for a in want["status"] if a != urm.ACCEPTED]

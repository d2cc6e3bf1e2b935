"""The sequential models of the store pipeline (test_store_audit.model, channel_range_model, range_compare_model, scid_query_model) against facts
nobody here authored: the stores and wire vectors the reference ships with expectations of its own authors, copied as data by
tests/golden/make_reference_stores.py --
  - a mainnet excerpt of August 2021 in two parts (part 2 is a tail appended to part 1): 186 records of foreign implementations, six of them
    deleted, seven with the obsolete flag bit 0x4000, 84 of 88 live channels without an update, no node_announcement, and a delete_chan tombstone
    whose header CRC is wrong (pyln's reader, which the file was made for, checks none);
  - the canned regtest store of common/test/run-gossmap_canned.c with what that test asserts a loader finds in it;
  - the two channel_updates of connectd/test/run-crc32_of_update.c with their BOLT #7 checksums;
  - the BOLT #7 extended-query vectors of gossipd/test/run-extended-info.c as field values and exact hex.
An error the models share with the device code cannot show where both are compared with each other; it shows here.  The same inputs on the
device: test_gpu_reference_stores.py; on the host builds under the sanitizers: the test_store_*_host.py files."""
import json
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import range_compare_model as rcm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_store_audit as sa  # noqa: E402

H = bytes.fromhex
F_OBSOLETE = 0x4000                                       # "push" in the stores of 2021; no reader of today looks at it
MAINNET = H("6fe28c0ab6f1b372c1a6a246ae63f74f931e8365e15a089c68d6190000000000")
TOMBSTONE_OFF, TOMBSTONE_CRC = 42653, 0x6f153b3e           # the last record of part 2 and the CRC-32C (seed 0) its message has
TOMBSTONED_ANN = 182                                      # the record of the announcement it names (183: its amount; 184: another channel's announcement)
# record counts by verdict, and the signatures checked: part 1, part 1 + part 2, the same with the tombstone's CRC corrected, the canned store
COUNTS = {"part1": (94, {sa.OK: 92, sa.DELETED: 2}, 182), "mainnet": (186, {sa.OK: 179, sa.DELETED: 6, sa.BAD_CHECKSUM: 1}, 356),
          "fixed": (186, {sa.OK: 180, sa.DELETED: 6}, 356), "canned": (13, {sa.OK: 11, sa.DELETED: 2}, 15)}
# The figures below are no literals of the reference: they follow from the counts above by this project's rules and were first seen in runs of the
# models.  What a repair keeps: every record not flagged DELETED; of part 1 + part 2 also not the tombstone (its checksum, or with that corrected
# store bookkeeping) nor the announcement in front of it, of 687509x1304x0, the one live announcement with no channel_amount record behind it
# (not the channel the tombstone names: that one, two records earlier, is kept): 186 - 6 - 2.
KEPT = {"part1": 92, "mainnet": 178, "fixed": 178, "canned": 11}
# The 8 channel_updates of part 1 + part 2 received against part 1 alone: 3 name channels only part 2 announces (UNKNOWN, no signer looked up),
# the other 5 go to the signature batch, and 3 of those are newer than what part 1 holds for their slot (ACCEPTED).
PART1_RECEIVE = dict(signed=5, unknown=3, accepted=3)


def vectors():
    with open(os.path.join(sa.ROOT, "tests", "golden", "bolt7_vectors.json")) as f:
        return json.load(f)


def scid(text):
    """'686200x1137x0' -> the 64-bit short_channel_id"""
    b, t, o = (int(x) for x in text.split("x"))
    return crm.scid_of(b, t, o)


def crc_bitwise(seed, data):
    """CRC-32C from its definition, bit by bit: shares nothing with the tables of test_store_audit.crc32c"""
    c = seed ^ 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def store(name):
    """'part1', 'mainnet' (part 1 + part 2), 'fixed' (mainnet with the tombstone's CRC corrected), 'canned' -> the image"""
    if name == "canned":
        return sa._golden("gossip_store_canned.bin")
    blob = sa._golden("gossip_store_mainnet_part1.bin")
    if name == "part1":
        return blob
    blob += sa._golden("gossip_store_mainnet_part2.bin")
    if name == "fixed":
        flags, ln, _, ts = struct.unpack(">HHII", blob[TOMBSTONE_OFF:TOMBSTONE_OFF + 12])
        assert TOMBSTONE_OFF + 12 + ln == len(blob)
        blob = blob[:TOMBSTONE_OFF + 4] + struct.pack(">I", crc_bitwise(ts, blob[TOMBSTONE_OFF + 12:])) + blob[TOMBSTONE_OFF + 8:]
    else:
        assert name == "mainnet"
    return blob


def chain_of(blob):
    """the chain_hash the first live channel_announcement of an image names"""
    m = next(r[4] for r in sa.walk(blob)[0] if not r[1] & sa.F_DELETED and r[4][:2] == b"\x01\x00")
    o = 260 + int.from_bytes(m[258:260], "big")
    return m[o:o + 32]


def newest(blob):
    """the newest header timestamp of an image"""
    return max(r[3] for r in sa.walk(blob)[0])


def updates_in(blob):
    """every channel_update of an image in file order, the deleted ones included -> [(record index, deleted, message)]"""
    return [(i, bool(r[1] & sa.F_DELETED), r[4]) for i, r in enumerate(sa.walk(blob)[0]) if r[4][:2] == b"\x01\x02"]


def query_fields(v):
    """a vector's field values -> (chain, first, number, option or None)"""
    m = v["msg"]
    assert m["extensions"] in ([], ["WANT_TIMESTAMPS | WANT_CHECKSUMS"])
    return H(m["chainHash"]), m["firstBlockNum"], m["numberOfBlocks"], 3 if m["extensions"] else None


def reply_fields(v):
    """-> (chain, first, number, complete, [scid], [(ts1, ts2)], [(csum1, csum2)])"""
    m = v["msg"]
    assert m["shortChannelIds"]["encoding"] == m["timestamps"]["encoding"] == "UNCOMPRESSED"
    return (H(m["chainHash"]), m["firstBlockNum"], m["numberOfBlocks"], m["complete"], [scid(s) for s in m["shortChannelIds"]["array"]],
            [(t["timestamp1"], t["timestamp2"]) for t in m["timestamps"]["timestamps"]], [(c["checksum1"], c["checksum2"]) for c in m["checksums"]["checksums"]])


def decode_update(m):
    """the fields of a channel_update with htlc_maximum_msat, by the offsets of BOLT #7"""
    ts, mflags, cflags, cltv, hmin, base, prop, hmax = struct.unpack(">IBBHQIIQ", m[106:138])
    return dict(timestamp=ts, message_flags=mflags, channel_flags=cflags, cltv_expiry_delta=cltv, htlc_minimum_msat=hmin, fee_base_msat=base,
                fee_proportional_millionths=prop, htlc_maximum_msat=hmax)


def signature_rows(orc, blob):
    """every signature a loader that trusts nothing checks in an image -> (hash32 [n, 32], sig64 [n, 64], key33 [n, 33]): four per live
    channel_announcement (node_1, node_2, bitcoin_1, bitcoin_2 over sha256d of the bytes behind the signatures), one per live channel_update
    (under the node id its announcement names for its direction), one per live node_announcement"""
    recs = sa.walk(blob)[0]
    ann, rows = {}, []
    for _, flags, _, _, m in recs:
        if flags & sa.F_DELETED:
            continue
        t = int.from_bytes(m[:2], "big")
        if t == 256:
            s, o = sa._cann_scid(m)
            ann.setdefault(s, m[o:o + 66])
            h = orc.sha256d(m[258:])
            rows += [(h, m[2 + 64 * k:66 + 64 * k], m[o + 33 * k:o + 33 * k + 33]) for k in range(4)]
        elif t == 258:
            ids = ann[int.from_bytes(m[98:106], "big")]
            rows.append((orc.sha256d(m[66:]), m[2:66], ids[33 * (m[111] & 1):][:33]))
        elif t == 257:
            o = 72 + int.from_bytes(m[66:68], "big")
            rows.append((orc.sha256d(m[66:]), m[2:66], m[o:o + 33]))
    col = lambda k, w: np.frombuffer(b"".join(r[k] for r in rows), dtype=np.uint8).reshape(len(rows), w).copy()
    return col(0, 32), col(1, 64), col(2, 33)


def amount_sat(recs, a):
    """the satoshis of the channel_amount record behind announcement record a"""
    m = recs[a + 1][4]
    assert m[:2] == b"\x10\x05" and len(m) == 10 and not recs[a + 1][1] & sa.F_DELETED
    return int.from_bytes(m[2:], "big")


# ------------------------------------------------------------------------------------------------ literals against the models
def test_the_fixtures_are_the_ones_the_generator_describes():
    v = vectors()
    assert (len(store("part1")), len(store("mainnet")), len(store("canned"))) == (21571, 42675, 2316)
    assert [x["msg"]["type"] for x in v["extended_queries"]] == ["QueryChannelRange", "QueryChannelRange", "ReplyChannelRange", "QueryShortChannelIds"]
    assert all("source" in x for x in v["extended_queries"] + v["update_checksums"] + [v["canned"], v["mainnet"]])
    assert chain_of(store("part1")) == chain_of(store("mainnet")) == MAINNET


def test_update_checksums_of_the_reference():
    pairs = vectors()["update_checksums"]
    assert [len(H(p["update"])) for p in pairs] == [130, 138] and [p["checksum"] for p in pairs] == [0x1112fa30, 0xf32ce968]
    for p in pairs:
        m = H(p["update"])
        assert crm.update_csum(m) == p["checksum"]
        assert crc_bitwise(0, m[66:106] + m[110:]) == p["checksum"]                             # the same from the definition: no table shared


def test_extended_query_vectors_build_and_parse():
    q1, q2, rep, ids = vectors()["extended_queries"]
    for q in (q1, q2):
        chain, first, number, option = query_fields(q)
        assert crm.query(chain, first, number, option).hex() == q["hex"]
        assert crm.parse_query(H(q["hex"])) == (chain, first, number, option or 0)
    chain, first, number, complete, scids, ts, csum = reply_fields(rep)
    assert rcm.reply(chain, first, number, scids, ts, csum, final=complete).hex() == rep["hex"]
    assert rcm.parse(H(rep["hex"]), chain, want=(122334, 123834)) == (0, scids, ts)
    d = crm.decode_reply(H(rep["hex"]))
    assert (d["chain"], d["first"], d["blocks"], d["final"], d["scids"], d["ts"], d["csum"]) == (chain, first, number, complete, scids, ts, csum)
    m = ids["msg"]
    assert m["extensions"] == [] and m["shortChannelIds"]["encoding"] == "UNCOMPRESSED"
    chain, scids = H(m["chainHash"]), [scid(s) for s in m["shortChannelIds"]["array"]]
    assert sqm.query(chain, scids).hex() == ids["hex"]
    assert sqm.parse(H(ids["hex"]), chain) == (0, scids, [0x1f] * 3)                          # no flags TLV: everything is asked for


# ------------------------------------------------------------------------------------------------ the canned store
def test_canned_store_holds_what_the_reference_asserts(orc):
    lit = vectors()["canned"]
    blob = store("canned")
    recs = sa.walk(blob)[0]
    _, v, s = sa.model(orc, blob)
    want = COUNTS["canned"]
    assert (len(v), {k: v.count(k) for k in set(v)}, s["signatures"], s["clean"]) == (want[0], want[1], want[2], 1)
    by = {e[0]: e for e in crm.sorted_digest(blob)[0]}
    e = by[scid(lit["scid"])]
    assert lit["scid"] == "110x1x0" and e[1] == (1700115313, 1700115313) == tuple(d["timestamp"] for d in lit["directions"])
    for d, want_fields in enumerate(lit["directions"]):
        got = decode_update(recs[e[3][1 + d]][4])
        assert got == want_fields and got["channel_flags"] == d
        assert (got["cltv_expiry_delta"], got["fee_base_msat"], got["fee_proportional_millionths"], got["htlc_maximum_msat"]) == (6, 20, 1000, 990_000_000)
    assert e[2] == tuple(crc_bitwise(0, recs[u][4][66:106] + recs[u][4][110:]) for u in e[3][1:])
    nodes = sqm.directory(blob)["nodes"]
    assert all(H(x) in nodes for x in lit["node_ids"]) and len(nodes) == 3
    assert amount_sat(recs, e[3][0]) == lit["capacity_sat"] == 1_000_000


# ------------------------------------------------------------------------------------------------ the mainnet store
def test_mainnet_verdicts_and_signatures(orc):
    for name in ("part1", "mainnet"):
        blob = store(name)
        n, counts, sigs = COUNTS[name]
        _, v, s = sa.model(orc, blob)
        assert (len(v), {k: v.count(k) for k in set(v)}, s["signatures"]) == (n, counts, sigs)
        assert s["bad_signature"] == [0, 0, 0, 0] and s["malformed"] == s["no_channel"] == s["redundant"] == 0 and s["end_reason"] == "eof"
        assert s["clean"] == (1 if name == "part1" else 0)
        # the same signatures under OpenSSL with libsecp256k1's rules, and under a real libsecp256k1 where the machine has one
        hs, sg, pk = signature_rows(orc, blob)
        assert len(hs) == sigs
        assert orc.ossl_ecdsa_verify_rules_batch(hs, sg, pk, 33).all()
        assert orc.ecdsa_verify_batch(hs, sg, pk, 33, 1).all()
        if orc.libsecp_available():
            assert orc.libsecp_ecdsa_verify_batch(hs, sg, pk, 33).all()


def test_the_one_bad_checksum_is_the_tombstone_and_its_correction_cleans_the_store(orc):
    lit = vectors()["mainnet"]
    blob = store("mainnet")
    off, v, _ = sa.model(orc, blob)
    bad = [i for i, x in enumerate(v) if x not in (sa.OK, sa.DELETED)]
    assert bad == [len(v) - 1] and off[bad[0]] == TOMBSTONE_OFF and v[bad[0]] == sa.BAD_CHECKSUM
    _, flags, crc, ts, m = sa.walk(blob)[0][bad[0]]
    assert (flags, ts, m) == (sa.F_COMPLETED, 0, struct.pack(">HQ", 4103, scid(lit["tombstoned_scid"]))) and lit["tombstoned_scid"] == "686386x1093x1"
    assert crc_bitwise(ts, m) == TOMBSTONE_CRC != crc
    _, fv, fs = sa.model(orc, store("fixed"))
    assert fs["clean"] == 1 and fs["signatures"] == 356 and fv == v[:-1] + [sa.OK]


def test_obsolete_flag_bit_changes_nothing(orc):
    blob = store("mainnet")
    recs = sa.walk(blob)[0]
    flagged = [i for i, r in enumerate(recs) if r[1] & F_OBSOLETE]
    _, v, _ = sa.model(orc, blob)
    assert len(flagged) == 7 and all(v[i] == sa.OK and not recs[i][1] & sa.F_DELETED for i in flagged)
    # ... nor does clearing it: the header's flags are not under the checksum
    cleared = bytearray(blob)
    for i in flagged:
        cleared[recs[i][0]] &= 0xBF
    assert sa.model(orc, bytes(cleared))[1] == v


def test_mainnet_channels_of_pylns_test(orc):
    lit = vectors()["mainnet"]
    blob = store("mainnet")
    recs = sa.walk(blob)[0]
    d = sqm.directory(blob, sa.model(orc, blob)[1])
    assert len(d["chan"]) == 88 and len(d["entries"]) == 4 and len(d["bare"]) == 84 and d["counters"]["nodes"] == 126 and d["counters"]["nodes_announced"] == 0
    assert amount_sat(recs, d["chan"][scid(lit["scid"])][0]) == lit["satoshis"] == 3_000_000
    # pyln's Gossmap checks no CRC and applies the delete_chan tombstone: its test expects 686386x1093x1 and the node that has no other channel
    # gone.  The C loader applies tombstones too (common/gossmap.c:900-901) but checks CRCs first (:870-888): it stops loading in front of this
    # one, so there the channel survives, as it does here, where the tombstone is BAD_CHECKSUM.  The announcement is not flagged DELETED in the file.
    gone = scid(lit["tombstoned_scid"])
    a = d["chan"][gone][0]
    assert gone in d["bare"] and not recs[a][1] & sa.F_DELETED and sa._cann_scid(recs[a][4])[0] == gone
    assert H(lit["node_pyln_drops"]) in d["nodes"] and H(lit["node_untouched"]) in d["nodes"]
    o = sa._cann_scid(recs[a][4])[1]
    assert {recs[a][4][o:o + 33], recs[a][4][o + 33:o + 66]} == {H(lit["node_pyln_drops"]), H(lit["node_untouched"])}


def tombstone_divergence(blob, verdicts):
    """what this project holds for part 1 + part 2 with the tombstone's CRC corrected, against what a loader that applies the tombstone holds ->
    (the tombstoned scid, the node that has no other channel).  Shared with the device's test of the same image."""
    lit = vectors()["mainnet"]
    gone, lonely = scid(lit["tombstoned_scid"]), H(lit["node_pyln_drops"])
    recs = sa.walk(blob)[0]
    assert set(verdicts) == {sa.OK, sa.DELETED} and verdicts[-1] == sa.OK and recs[-1][4] == struct.pack(">HQ", 4103, gone)
    ann = [i for i, r in enumerate(recs) if not r[1] & sa.F_DELETED and sa._cann_scid(r[4])]
    mine = [i for i in ann if sa._cann_scid(recs[i][4])[0] == gone]
    assert mine == [TOMBSTONED_ANN] and amount_sat(recs, TOMBSTONED_ANN) > 0                  # one live announcement with its amount record, in front
    ids = lambda m: {m[sa._cann_scid(m)[1]:][:33], m[sa._cann_scid(m)[1] + 33:][:33]}
    assert [i for i in ann if lonely in ids(recs[i][4])] == mine                              # the node's only channel
    assert all(sum(1 for i in ann if x in ids(recs[i][4])) > 1 for x in ids(recs[mine[0]][4]) - {lonely})
    return gone, lonely


def test_a_valid_tombstone_behind_unflagged_records_is_not_applied_unlike_the_reference(orc):
    """A DELIBERATE DIFFERENCE, pinned.  With the tombstone's CRC corrected, common/gossmap.c (:900-901, remove_channel_by_deletemsg) and pyln
    would remove 686386x1093x1 and, with it, node 029deaf9..., which has no other channel: 87 channels and 125 nodes.  This project decides live
    or dead by the DELETED flag alone and never applies a tombstone: 88 channels and 126 nodes, in digest, bare list and directory.  The rule is
    chosen because gossipd, the only writer of such a file, never writes a tombstone without flagging the announcement, its amount record and
    its updates DELETED in the same step (gossmap_manage.c:318-328), so on any store gossipd wrote both rules give the same result, and the flag
    is a per-record decision a device thread can take without a second pass over the file.  This image, of 2021 and corrected by hand, is
    not such a store; a caller that needs the loader's answer for one has to apply tombstones itself (include/lightning_amd.h says so)."""
    blob = store("fixed")
    v = sa.model(orc, blob)[1]
    gone, lonely = tombstone_divergence(blob, v)
    d = sqm.directory(blob, v)
    assert gone in d["chan"] and gone in d["bare"] and gone in rcm.bare(blob, v) and gone not in [e[0] for e in crm.sorted_digest(blob, v)[0]]
    assert lonely in d["nodes"]
    assert (len(d["chan"]), len(d["bare"]), len(d["nodes"])) == (88, 84, 126)                 # a loader applying the tombstone: 87, 83, 125
    shipped = sqm.directory(store("mainnet"), sa.model(orc, store("mainnet"))[1])
    assert all(d[k] == shipped[k] for k in ("chan", "entries", "bare", "nodes", "nann"))      # valid or not, the tombstone changes nothing
    # the repair writes the channel out again, announcement and amount, and drops only the tombstone's own record (and, for its own reason, the
    # announcement of ANOTHER channel in front of it): a loader reading the output finds the channel that gossmap.c would have dropped from the input
    import test_store_repair as sr
    reasons, _, out = sr.repair_model(blob, v, sr.UUID)
    assert reasons[TOMBSTONED_ANN:] == [sr.KEPT, sr.KEPT, sr.R_DEPENDENCY, sr.R_BOOKKEEPING] and reasons.count(sr.KEPT) == KEPT["fixed"]
    assert gone in sqm.directory(out)["bare"] and lonely in sqm.directory(out)["nodes"]

"""A sequential restatement of what lamd_gossip_store_directory_build and lamd_short_channel_ids_reply_batch (include/lightning_amd.h) compute, for
the tests of the device code (test_gpu_scid_query.py) and of its host build (test_store_query_host.py):
  - directory(): a gossmap-style pass over the records in file order: the record of every channel, the node ids its announcement names, the
    first announcement that names a node, the last node_announcement behind it (common/gossmap.c:650-668);
  - parse(): fromwire_query_short_channel_ids with fromwire_tlv's rules, decode_scid_query_flags, decode_short_ids and the checks of
    handle_query_short_channel_ids() (connectd/queries.c:260-368) in the reference's order -> one of the six statuses;
  - answer(): maybe_create_query_responses() (:112-255) run to its end for one query;
  - builders of announcements with chosen node ids, of node_announcements and of queries, next to channel_range_model.cann / cupd."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import range_compare_model as rcm  # noqa: E402
import test_store_audit as sa  # noqa: E402

NONE = 0xFFFFFFFF
END_OURS = lambda chain: struct.pack(">H", 262) + chain + b"\x01"


# ---- builders
def node_id(k, head=2):
    """a 33-byte id that looks like a compressed key"""
    return bytes([head]) + struct.pack(">Q", k) * 4


def cann_ids(scid, id1, id2, flen=0, length=None):
    """a channel_announcement with chosen node ids and feature length; length: cut (or padded) to that many bytes"""
    m = bytearray(b"\x55" * (430 + flen))
    m[0:2] = b"\x01\x00"
    m[258:260] = struct.pack(">H", flen)
    m[292 + flen:300 + flen] = struct.pack(">Q", scid)
    m[300 + flen:333 + flen] = id1
    m[333 + flen:366 + flen] = id2
    return bytes(m[:length]) if length is not None else bytes(m)


def nann(nid, ts=0, flen=0, length=None, fill=0x66):
    """a node_announcement: be16 257 | signature 64 | be16 flen | features | be32 timestamp | node_id 33 | rgb, alias, addresses"""
    m = bytearray(bytes([(fill + 3 * k) & 0xff for k in range(72 + flen + 33 + 37)]))
    m[0:2] = b"\x01\x01"
    m[66:68] = struct.pack(">H", flen)
    m[68 + flen:72 + flen] = struct.pack(">I", ts)
    m[72 + flen:105 + flen] = nid
    return bytes(m[:length]) if length is not None else bytes(m)


def query(chain, scids, flags=None, encoding=0, flag_encoding=0, tlvs=b"", raw_flags=None):
    """a raw query_short_channel_ids; flags: one int per scid written as a minimal bigsize (None: no TLV 1); raw_flags: the encoded flags as bytes"""
    enc = bytes([encoding]) + b"".join(struct.pack(">Q", s) for s in scids)
    q = struct.pack(">H", 261) + chain + struct.pack(">H", len(enc)) + enc
    if flags is not None or raw_flags is not None:
        v = bytes([flag_encoding]) + (raw_flags if raw_flags is not None else b"".join(crm.bigsize(f) for f in flags))
        q += b"\x01" + crm.bigsize(len(v)) + v
    return q + tlvs


# ---- the directory
def directory(blob, verdict=None, recs=None):
    """-> dict(chan: {scid: (ann, u0, u1)} (NONE where there is none), entries: [scid] ascending, bare: [scid] ascending, bare_rec: [record],
    nodes: [id] ascending, first: [record], nann: [record or NONE], ranks: {scid: (rank1, rank2)} (NONE: none), counters: dict)"""
    recs = sa.walk(blob)[0] if recs is None else recs
    entries = crm.sorted_digest(blob, verdict, recs)[0]
    bare = rcm.bare(blob, verdict, recs)
    counting = lambda i: not recs[i][1] & sa.F_DELETED and (verdict is None or verdict[i] == crm.OK)
    chan = {e[0]: tuple(e[3]) for e in entries}
    bare_rec = []
    for s in bare:
        a = min(i for i, r in enumerate(recs) if counting(i) and sa._cann_scid(r[4]) and sa._cann_scid(r[4])[0] == s)
        bare_rec.append(a)
        chan[s] = (a, NONE, NONE)
    ids_of, first = {}, {}
    for s, (a, _, _) in chan.items():
        m = recs[a][4]
        f = int.from_bytes(m[258:260], "big")
        if len(m) < 366 + f:
            ids_of[s] = None
            continue
        ids_of[s] = (m[300 + f:333 + f], m[333 + f:366 + f])
        for nid in ids_of[s]:
            first[nid] = min(first.get(nid, a), a)
    nodes = sorted(first)
    rank = {nid: r for r, nid in enumerate(nodes)}
    last = {}
    c = dict(nodes=len(nodes), nodes_announced=0, nann_no_node=0, nann_in_front=0, nann_short=0)
    for i, r in enumerate(recs):
        m = r[4]
        if not counting(i) or m[:2] != b"\x01\x01":
            continue
        f = int.from_bytes(m[66:68], "big") if len(m) >= 68 else 0
        if len(m) < 68 or len(m) < 105 + f:
            c["nann_short"] += 1
            continue
        nid = m[72 + f:105 + f]
        if nid not in first:
            c["nann_no_node"] += 1
        elif i <= first[nid]:
            c["nann_in_front"] += 1
        else:
            last[nid] = i                                  # last in file order wins
    c["nodes_announced"] = len(last)
    ranks = {s: (NONE, NONE) if ids_of[s] is None else tuple(rank[x] for x in ids_of[s]) for s in chan}
    return dict(chan=chan, entries=[e[0] for e in entries], bare=bare, bare_rec=bare_rec, nodes=nodes, first=[first[x] for x in nodes],
                nann=[last.get(x, NONE) for x in nodes], ranks=ranks, counters=c, recs=recs)


# ---- the parser
def parse(q, chain=crm.CHAIN):
    """-> (status, [scid], [flag byte])"""
    bad = (-1, [], [])
    if len(q) < 36 or q[:2] != struct.pack(">H", 261):
        return bad
    ln = int.from_bytes(q[34:36], "big")
    if 36 + ln > len(q):
        return bad
    enc = q[36:36 + ln]
    pos, prev, ftlv = 36 + ln, None, None
    while pos < len(q):
        r = crm.read_bigsize(q, pos)
        if r is None:
            return bad
        t, pos = r
        if prev is not None and t <= prev:
            return bad
        prev = t
        if t != 1 and t % 2 == 0:
            return bad
        r = crm.read_bigsize(q, pos)
        if r is None:
            return bad
        tl, pos = r
        if tl > len(q) - pos:
            return bad
        if t == 1:
            if tl == 0:                                     # no encoding_type byte
                return bad
            ftlv = q[pos:pos + tl]
        pos += tl
    flags = None
    if ftlv is not None:
        if ftlv[0] != 0:
            return 2, [], []
        flags, p = [], 1
        while p < len(ftlv):
            r = crm.read_bigsize(ftlv, p)
            if r is None:
                return 2, [], []
            flags.append(r[0] & 0x1f)
            p = r[1]
    if q[2:34] != chain:
        return 1, [], []
    if ln == 0 or enc[0] != 0 or (ln - 1) % 8:
        return 3, [], []
    scids = [int.from_bytes(enc[1 + 8 * k:9 + 8 * k], "big") for k in range((ln - 1) // 8)]
    if flags is None:
        flags = [0x1f] * len(scids)
    elif len(flags) != len(scids):
        return 4, [], []
    return 0, scids, flags


# ---- the answer
def answer(d, q, chain=crm.CHAIN):
    """-> (status, (scids, known, channel messages, node messages), [message bytes], [record index or NONE])"""
    st, scids, flags = parse(q, chain)
    if st == 1:
        return st, (0, 0, 0, 0), [struct.pack(">H", 262) + q[2:34] + b"\x00"], [NONE]
    if st != 0:
        return st, (0, 0, 0, 0), [], []
    recs, out, known, wanted = d["recs"], [], 0, set()
    for s, f in zip(scids, flags):
        if s not in d["chan"]:
            continue
        known += 1
        for k in range(3):
            if f >> k & 1 and d["chan"][s][k] != NONE:
                out.append(d["chan"][s][k])
        for k in range(2):
            if f >> (3 + k) & 1 and d["ranks"][s][k] != NONE:
                wanted.add(d["ranks"][s][k])
    n_chan = len(out)
    out += [d["nann"][r] for r in sorted(wanted) if d["nann"][r] != NONE]
    return 0, (len(scids), known, n_chan, len(out) - n_chan), [recs[i][4] for i in out] + [END_OURS(chain)], out + [NONE]


def answers(d, queries, chain=crm.CHAIN):
    """-> ([status], [per_query], [[message bytes]], [[record]]) for a batch"""
    res = [answer(d, q, chain) for q in queries]
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], [r[3] for r in res]


# ---- stores and query sets shared by the host-build test and the device test
def hand_store():
    """every case of the directory in one store -> (image, {name: scid}, {name: node id})"""
    N = {k: node_id(i + 1, 2 + (i & 1)) for i, k in enumerate(("a", "b", "c", "early", "never", "f5", "cut1", "cut2", "x", "y"))}
    S = {k: crm.scid_of(700 + 2 * i, 1, i & 1) for i, k in enumerate(("two", "one", "bare", "flen", "cutid", "late"))}
    R = crm.fast_rec
    recs = [R(nann(N["early"], 5)),                                                           # in front of its first channel: not announced
            R(nann(N["a"], 1)),                                                               # ... and so is this one of a
            R(cann_ids(S["two"], N["a"], N["b"])), R(crm.AMOUNT), R(crm.cupd(S["two"], 0, 10)), R(crm.cupd(S["two"], 1, 11, 140)),
            R(nann(N["a"], 900, fill=0x11)),
            R(cann_ids(S["one"], N["b"], N["early"])), R(crm.AMOUNT), R(crm.cupd(S["one"], 1, 12, 133)),
            R(cann_ids(S["bare"], N["c"], N["never"])), R(crm.AMOUNT),
            R(nann(N["a"], 800, fill=0x22)),                                                   # announced twice: the last wins, lower timestamp or not
            R(nann(N["c"], 7, flen=3)),
            R(nann(N["b"], 9, length=104)),                                                    # one byte short
            R(nann(N["b"], 9, flen=2, length=106)),                                            # ... with features
            R(nann(node_id(99), 9)),                                                           # no such node
            R(cann_ids(S["flen"], N["f5"], N["a"], flen=5)), R(crm.AMOUNT), R(crm.cupd(S["flen"], 0, 13)),
            R(nann(N["f5"], 3), flags=sa.F_COMPLETED | sa.F_DELETED), R(nann(N["f5"], 4, fill=0x33)),
            R(cann_ids(S["cutid"], N["cut1"], N["cut2"], length=333)), R(crm.AMOUNT), R(crm.cupd(S["cutid"], 0, 14)),   # cut before node_id_2
            R(nann(N["cut1"], 6)),                                                             # no announcement names cut1
            R(cann_ids(S["late"], N["x"], N["y"])), R(crm.AMOUNT), R(cann_ids(S["late"], N["a"], N["b"])), R(crm.AMOUNT),   # the first announcement is the channel
            R(crm.cupd(S["late"], 0, 15)), R(crm.cupd(S["late"], 1, 16)), R(nann(N["y"], 2)), R(b"\x01\x01" + bytes(40))]
    return sa.serialise(0x10, recs), S, N


def status_cases(known, chain=crm.CHAIN, foreign=crm.FOREIGN):
    """one query (at least) of every status, with its expected status by hand -> [(query, status)]; known: scids of the store"""
    s = list(known[:3])
    ids = b"".join(struct.pack(">Q", x) for x in s)
    ok = query(chain, s, [1, 2, 4])
    raw = lambda enc, tlvs=b"", ch=chain: struct.pack(">H", 261) + ch + struct.pack(">H", len(enc)) + enc + tlvs
    return [
        (ok, 0), (query(chain, s), 0), (query(chain, []), 0), (query(chain, [], []), 0), (query(chain, s, [0x11f, 1 << 40, 0xffffffffffffffff]), 0),
        (query(chain, s, [1, 2, 4], tlvs=b"\x03\x02\xaa\xbb"), 0),                             # an unknown odd type behind
        (ok[:35], -1), (b"\x01\x04" + ok[2:], -1), (ok[:50], -1), (b"", -1), (ok + b"\x04\x00", -1), (raw(b"\x00" + ids, b"\x01\x00"), -1),
        (raw(b"\x00" + ids, b"\x03\x00\x01\x01\x00"), -1), (raw(b"\x00" + ids, b"\xfd\x00\x01\x01\x00"), -1), (raw(b"\x00" + ids, b"\x01\x05\x00\x01"), -1),
        (query(chain, s, [1, 2, 4], flag_encoding=1), 2), (query(chain, s, raw_flags=b"\x01\xfd\x00\x05\x01"), 2),   # zlib; a flag not minimal
        (query(chain, s, raw_flags=b"\x01\x01\xfd\x01"), 2), (query(foreign, s, raw_flags=b"\xfe\x00"), 2),         # a flag past the end; ... even on a foreign chain
        (query(foreign, s, [1, 2, 4]), 1), (raw(b"\x01" + ids, ch=foreign), 1), (raw(b"", ch=foreign), 1), (query(foreign, s, [1]), 1),   # foreign, bad scids or not
        (raw(b""), 3), (raw(b"\x01" + ids), 3), (raw(b"\x00" + ids[:-1]), 3), (raw(b"\x00" + ids[:-1], b"\x01\x02\x00\x01"), 3),
        (query(chain, s, [1, 2]), 4), (query(chain, s, [1, 2, 4, 8]), 4), (query(chain, s, []), 4), (query(chain, [], [1]), 4),
    ]


def flag_queries(d, chain=crm.CHAIN):
    """every flag value on each channel, every channel without TLV, some unknown scids between them"""
    chans = sorted(d["chan"])
    out = [query(chain, [s], [f]) for s in chans for f in range(32)]
    out += [query(chain, chans), query(chain, chans[::-1], [0x1f] * len(chans)), query(chain, [s ^ 1 << 62 for s in chans]),
            query(chain, chans + chans[::-1] + [chans[0] ^ 1 << 62] + chans[:2], [(7 * k + 3) & 0xff for k in range(2 * len(chans) + 3)])]
    return out

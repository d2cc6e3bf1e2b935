"""A sequential restatement of what lamd_channel_range_compare_batch (include/lightning_amd.h) computes, for the tests of the device code
(test_gpu_range_compare.py) and of its host build (test_store_compare_host.py):
  - parse(): fromwire_reply_channel_range with fromwire_tlv's rules, then the checks of handle_reply_channel_range() and append_range_reply()
    (gossipd/queries.c:142-265) in the reference's order -> one of the seven statuses;
  - bare(): the channels of a store that have no update (channel_range_model.digest() counts them and drops them);
  - classify(): gossmap_find_chan + check_timestamps() / want_update() (gossipd/seeker.c:636-706) for one entry;
  - compare(): all of it for a batch, the two uintmaps as dicts, and the query_short_channel_ids messages (queries.c:46-139);
  - reply(): a builder of reply_channel_range bytes on top of channel_range_model.encode()."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402

MAX_UNKNOWN, MAX_STALE = 8000, 7000
UNKNOWN = "unknown"


def reply(chain, first, blocks, scids, ts=None, csum=None, final=1, tlvs=b""):
    """a raw reply_channel_range; ts / csum: one pair per scid or None (no TLV 1 / 3); tlvs: raw bytes appended"""
    entries = [(s, ts[k] if ts else (0, 0), csum[k] if csum else (0, 0)) for k, s in enumerate(scids)]
    return crm.encode(chain, first, blocks, entries, final, (1 if ts is not None else 0) | (2 if csum is not None else 0)) + tlvs


def parse(m, chain=crm.CHAIN, want=None):
    """-> (status, [scid], [(t1, t2)] or None).  want: (range_first_blocknum, range_end_blocknum) of the outstanding query, or None"""
    bad = (-1, [], None)
    if len(m) < 45 or m[:2] != struct.pack(">H", 264):
        return bad
    ln = int.from_bytes(m[43:45], "big")
    if 45 + ln > len(m):
        return bad
    enc = m[45:45 + ln]
    pos, prev, ts_tlv = 45 + ln, None, None
    while pos < len(m):
        r = crm.read_bigsize(m, pos)
        if r is None:
            return bad
        t, pos = r
        if prev is not None and t <= prev:
            return bad
        prev = t
        if t not in (1, 3) and t % 2 == 0:
            return bad
        r = crm.read_bigsize(m, pos)
        if r is None:
            return bad
        tl, pos = r
        if tl > len(m) - pos:
            return bad
        v = m[pos:pos + tl]
        if t == 1:
            if tl == 0:                                       # no encoding_type byte
                return bad
            ts_tlv = v
        if t == 3 and tl % 8:
            return bad
        pos += tl
    first, number = struct.unpack(">II", m[34:42])
    if m[2:34] != chain:
        return 1, [], None
    if first + number > 0xFFFFFFFF:
        return 2, [], None
    if ln == 0 or enc[0] != 0 or (ln - 1) % 8:
        return 3, [], None
    scids = [int.from_bytes(enc[1 + 8 * k:9 + 8 * k], "big") for k in range((ln - 1) // 8)]
    if want is not None and (first + number <= want[0] or first >= want[1]):
        return 4, [], None
    ts = None
    if ts_tlv is not None:
        if ts_tlv[0] != 0 or (len(ts_tlv) - 1) % 8:
            return 5, [], None
        ts = [struct.unpack(">II", ts_tlv[1 + 8 * k:9 + 8 * k]) for k in range((len(ts_tlv) - 1) // 8)]
        if len(ts) != len(scids):
            return 6, [], None
    return 0, scids, ts


def bare(blob, verdict=None, recs=None):
    """-> the scids of the channels without an update, ascending"""
    recs = sa.walk(blob)[0] if recs is None else recs
    chans = set()
    for i, r in enumerate(recs):
        if not r[1] & sa.F_DELETED and (verdict is None or verdict[i] == crm.OK) and sa._cann_scid(r[4]):
            chans.add(sa._cann_scid(r[4])[0])
    entries, c = crm.digest(blob, verdict, recs)
    out = sorted(chans - {e[0] for e in entries})
    assert len(out) == c["channels_no_update"] and len(chans) == c["channels"]
    return out


def classify(ours, bare_set, scid, ts):
    """ours: {scid: (ts0, ts1)} of the digest's entries -> UNKNOWN or the query_flags (0: nothing to do)"""
    if scid in ours:
        mine = ours[scid]
    elif scid in bare_set:
        mine = (0, 0)
    else:
        return UNKNOWN
    # want_update(): slot unset (0 in the digest) -> timestamp != 0; else timestamp > ours
    return (2 if ts[0] > mine[0] else 0) | (4 if ts[1] > mine[1] else 0)


def query_msgs(chain, scids, flags, per):
    out = []
    for a in range(0, len(scids), per):
        part = scids[a:a + per]
        m = struct.pack(">H", 261) + chain + struct.pack(">H", 1 + 8 * len(part)) + b"\x00" + b"".join(struct.pack(">Q", s) for s in part)
        if flags is not None:
            f = bytes(flags[a:a + per])
            m += b"\x01" + crm.bigsize(1 + len(f)) + b"\x00" + f
        out.append(m)
    return out


def compare(entries, bare_scids, chain, msgs, want=None, max_unknown=0, max_stale=0):
    """entries: the digest's (any order); -> (status [n], per_msg [(entries, unknown, stale)], unknown [scid], stale [scid], flags [int], [message bytes])"""
    ours, bare_set = {e[0]: e[1] for e in entries}, set(bare_scids)
    status, per_msg, unknown, stale = [], [], {}, {}
    for i, m in enumerate(msgs):
        st, scids, ts = parse(m, chain, None if want is None else want[i])
        status.append(st)
        nu = ns = 0
        for k, s in enumerate(scids):
            c = classify(ours, bare_set, s, ts[k] if ts is not None else (0, 0))
            if c == UNKNOWN:
                unknown[s] = True
                nu += 1
            elif c:
                stale[s] = stale.get(s, 0) | c
                ns += 1
        per_msg.append((len(scids), nu, ns))
    u, s = sorted(unknown), sorted(stale)
    f = [stale[x] for x in s]
    out = query_msgs(chain, u, None, max_unknown or MAX_UNKNOWN) + query_msgs(chain, s, f, max_stale or MAX_STALE)
    return status, per_msg, u, s, f, out


# ---- message sets shared by the host-build test and the device test
def status_cases(chain=crm.CHAIN, foreign=crm.FOREIGN):
    """one message (at least) of every status, with its expected status by hand -> [(message, want or None, status)]; the scids are unknown to every
    store of the tests, so a rejected message that contributed would show"""
    s = [crm.scid_of(0xABCDE0 + k, 7, 7) for k in range(3)]
    t = [(1, 2), (3, 4), (5, 6)]
    ok = reply(chain, 100, 50, s, t, t)
    enc = lambda e, tlvs=b"", first=100, number=50, ch=chain: struct.pack(">H", 264) + ch + struct.pack(">IIBH", first, number, 1, len(e)) + e + tlvs
    ids = b"".join(struct.pack(">Q", x) for x in s)
    tsb = b"".join(struct.pack(">II", *x) for x in t)
    return [
        (ok, None, 0), (ok, (0, 0xFFFFFFFF), 0), (reply(chain, 100, 50, []), None, 0), (reply(chain, 100, 50, [], []), None, 0),
        (ok[:44], None, -1), (b"\x01\x07" + ok[2:], None, -1), (ok[:60], None, -1), (b"", None, -1),
        (ok + b"\x04\x00", None, -1), (enc(b"\x00" + ids, b"\x03\x00\x01\x01\x00"), None, -1), (enc(b"\x00" + ids, b"\xfd\x00\x01\x01\x00"), None, -1),
        (enc(b"\x00" + ids, b"\x01\x00"), None, -1), (enc(b"\x00" + ids, b"\x03\x07" + bytes(7)), None, -1), (enc(b"\x00" + ids, b"\x01\x19\x00" + tsb[:20]), None, -1),
        (reply(foreign, 100, 50, s, t), None, 1), (enc(b"\x01" + ids, b"\x01\x19\x01" + tsb, ch=foreign), (0, 5), 1),      # foreign with a bad encoding: 1
        (reply(chain, 0xFFFFFFFF, 1, s), None, 2), (enc(b"\x00" + ids, b"\x01\x19\x01" + tsb, 0xFFFFFF00, 0x100), None, 2),  # overflow with bad timestamps: 2
        (enc(b""), None, 3), (enc(b"\x01" + ids), None, 3), (enc(b"\x00" + ids[:-1]), None, 3), (enc(b"\x01" + ids), (0, 5), 3),
        (ok, (150, 200), 4), (ok, (0, 100), 4), (ok, (149, 150), 0), (ok, (0, 101), 0), (enc(b"\x00" + ids, b"\x01\x19\x01" + tsb), (150, 200), 4),
        (enc(b"\x00" + ids, b"\x01\x19\x01" + tsb), None, 5), (enc(b"\x00" + ids, b"\x01\x18\x00" + tsb[:23]), None, 5),
        (enc(b"\x00" + ids, b"\x01\x11\x00" + tsb[:16]), None, 6), (enc(b"\x00" + ids[:8], b"\x01\x19\x00" + tsb), None, 6),
        (enc(b"\x00" + ids, b"\x01\x19\x00" + tsb + b"\x05\x02\xaa\xbb"), None, 0),                                       # an unknown odd type behind
    ]


def probe_replies(entries, bare_scids, chain=crm.CHAIN, per=5, foreign=crm.FOREIGN):
    """replies that touch every class over a digest: for every known scid in turn equal / newer in either / both / older timestamps, the bare ones with
    (0, 0) and (5, 0), an unknown scid beside each known one (some of them twice), the same again without TLV 1 and with checksums, and a foreign
    message of unknown scids in between -> [message]"""
    rows = []
    for k, e in enumerate(entries):
        a, b = e[1]
        rows.append((e[0], [(a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1), (max(a, 1) - 1, max(b, 1) - 1), (0, 0)][k % 6]))
        rows.append((e[0] ^ 0x8000 | 1 << 63, (k, k)))                                        # unknown (no store of the tests uses bit 63)
        if k % 4 == 0:
            rows.append((e[0] ^ 0x8000 | 1 << 63, (0, 0)))                                    # ... twice
        if k % 7 == 0:
            rows.append((e[0], (a, b + 2)))                                                   # the same known scid again: its flags OR
    for k, s in enumerate(bare_scids):
        rows += [(s, (0, 0)), (s, (5, 0))] if k % 2 == 0 else [(s, (0, 9))]
    msgs = []
    for a in range(0, len(rows), per):
        part = rows[a:a + per]
        scids, ts = [r[0] for r in part], [r[1] for r in part]
        kind = (a // per) % 4
        msgs.append(reply(chain, a, 10, scids, None if kind == 1 else ts, ts if kind == 2 else None, final=kind & 1))
        if kind == 3:
            msgs.append(reply(foreign, a, 10, [s ^ 0x4000 | 1 << 62 for s in scids], ts))
    return msgs

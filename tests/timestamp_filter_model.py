"""A sequential restatement of what lamd_gossip_store_stream_build and lamd_timestamp_filter_reply_batch (include/lightning_amd.h) compute, for
the tests: written from the text of handle_gossip_timestamp_filter_in and maybe_gossip_msg (connectd/multiplex.c), update_recent_timestamp
(connectd/connectd.c) and gossmap_stream_next / gossmap_iter_fast_forward (common/gossmap.c), record by record and message by message as
those loops read -- no tiles, no scans."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402

F_DYING = 0x0800
AS_FILTER = 2 ** 64 - 1
PUBLIC = (256, 257, 258)
COUNTERS = ("streamable", "skipped_deleted", "skipped_dying", "skipped_type", "skipped_verdict", "skipped_frame", "bytes")


def index(blob, verdict=None, recs=None, image_len=None):
    """-> dict(list: [(record index, header timestamp, message)] in file order, hts: [header timestamp of EVERY record, 0 without a header
    inside the image], counters).  recs: the walk's records, or any list of (off, flags, crc, ts, msg) that stands for rec_off: `blob` is then
    read at those offsets; image_len: the image ends there"""
    if recs is None:
        recs = sa.walk(blob)[0]
    end = len(blob) if image_len is None else image_len
    out, hts = [], []
    c = dict.fromkeys(COUNTERS, 0)
    for i, r in enumerate(recs):
        off = r[0]
        if off > end or end - off < 12:
            hts.append(0)
            c["skipped_frame"] += 1
            continue
        flags, ln, _, ts = struct.unpack(">HHII", blob[off:off + 12])
        hts.append(ts)
        if flags & sa.F_DELETED:
            c["skipped_deleted"] += 1
        elif verdict is not None and verdict[i] != crm.OK:
            c["skipped_verdict"] += 1
        elif flags & F_DYING:
            c["skipped_dying"] += 1
        elif end - off - 12 < ln or ln < 2:
            c["skipped_frame"] += 1
        elif int.from_bytes(blob[off + 12:off + 14], "big") not in PUBLIC:
            c["skipped_type"] += 1
        else:
            out.append((i, ts, bytes(blob[off + 12:off + 12 + ln])))
            c["streamable"] += 1
            c["bytes"] += ln
    # the number of streamable records in front of each record
    spos, k = [], 0
    for i in range(len(recs)):
        spos.append(k)
        if k < len(out) and out[k][0] == i:
            k += 1
    return dict(list=out, hts=hts, spos=spos + [len(out)], counters=c)


def filt(chain, first, rng, typ=265, tail=b""):
    """a raw gossip_timestamp_filter"""
    return struct.pack(">H", typ) + chain + struct.pack(">II", first, rng) + tail


def parse(f, chain=crm.CHAIN):
    """-> (status, min, max, rule): rule 0 from the start, 1 from the end, 2 from the recent position"""
    if len(f) < 42 or f[:2] != struct.pack(">H", 265):
        return (-1, 0, 0, 1)
    if f[2:34] != chain:
        return (1, 0, 0, 1)
    first, rng = struct.unpack(">II", f[34:42])
    lo, hi = first, (first + rng - 1) & 0xFFFFFFFF
    if hi < lo:
        hi = 0xFFFFFFFF
    return (0, lo, hi, 0 if first == 0 else 1 if first == 0xFFFFFFFF else 2)


def recent(idx, t):
    """gossmap_iter_fast_forward from the start: stop at the first record whose header timestamp is >= t; the position is that of the next
    message gossmap_stream_next would hand out from there"""
    for i, ts in enumerate(idx["hts"]):
        if ts >= t:
            return idx["spos"][i]
    return len(idx["list"])


def answer(idx, f, chain, now, cursor=AS_FILTER, budget=None):
    """-> (status, cursor_out, done, [message], [record index])"""
    st, lo, hi, rule = parse(f, chain)
    if st != 0:
        return st, cursor, 0, [], []
    lst = idx["list"]
    pos = cursor
    if cursor == AS_FILTER:
        pos = 0 if rule == 0 else len(lst) if rule == 1 else recent(idx, (now - 7200) & 0xFFFFFFFF)
    assert pos <= len(lst)
    sent, msgs, recs = 0, [], []
    while True:
        if budget is not None and sent > budget:                   # "Sent too much this second?": the iterator stays where it is
            return st, pos, 0, msgs, recs
        msg = None
        while pos < len(lst):                                      # gossmap_stream_next and the timestamp check behind it
            i, ts, m = lst[pos]
            pos += 1
            if ts and (ts < lo or ts > hi):
                continue
            msg = m
            break
        if msg is None:                                            # "No gossip left to send"
            return st, len(lst), 1, msgs, recs
        sent += len(msg)
        msgs.append(msg)
        recs.append(i)


def answers(idx, filters, chain=crm.CHAIN, now=0, cursors=None, budgets=None):
    """-> (status, cursor_out, done, messages per peer, records per peer)"""
    res = [answer(idx, f, chain, now, AS_FILTER if cursors is None else cursors[p], None if budgets is None else budgets[p]) for p, f in enumerate(filters)]
    return tuple([r[k] for r in res] for k in range(5))


def corpus(chain=crm.CHAIN):
    """the filter corpus of the tests -> [raw filter]"""
    full = filt(chain, 1000, 500, tail=b"\xaa\xbb")
    assert len(full) == 44
    out = [full[:k] for k in range(45)]
    out += [filt(chain, 0, 0xFFFFFFFF, typ=264), filt(chain, 0, 0xFFFFFFFF, typ=266), filt(crm.FOREIGN, 0, 0xFFFFFFFF)]
    out += [filt(chain, first, rng) for first in (0, 1, 0xFFFFFFFF, 0xFFFFFFFE) for rng in (0, 1, 0xFFFFFFFF)]
    out += [filt(chain, 0xFFFFFF00, 0x200), filt(chain, 0xFFFFFF00, 0x100)]      # one pair that wraps, one that ends exactly at UINT32_MAX
    return out

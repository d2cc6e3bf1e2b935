"""A sequential restatement of what lamd_channel_update_receive_batch (include/lightning_amd.h) computes, for the tests of the device code
(test_gpu_update_receive.py) and of its host build (test_store_receive_host.py).  It is written from the receive path of the reference,
gossmap_manage_channel_update() / process_channel_update() (gossipd/gossmap_manage.c:878-1120) and gossip_store_add / _del / _set_timestamp
(gossipd/gossip_store.c:49-78, 622-670): ONE message at a time, in arrival order, with a dict of slots.
  - view(): what the digest and the directory say about an image: the channels by scid (entries first, then the bare ones), the record and the
    signed timestamp of each direction, the two node ids, the announcement's DYING flag;
  - receive(): the statuses, flags, channel numbers and the plan;
  - apply(): the plan applied to the image, as the file stands after the reference has processed the batch."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_store_audit as sa  # noqa: E402

NONE = 0xFFFFFFFF
MALFORMED, ACCEPTED, WRONG_CHAIN, TIMESTAMP, HELD, PRIVATE, UNKNOWN, BAD_SIGNATURE, DONT_FORWARD, STALE, DUPLICATE = -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
SUPERSEDED, FIRST, DYING, PEER_UPDATE = 1, 2, 4, 8
F_DYING = 0x0800
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
U64 = (1 << 64) - 1
NO_KEY = bytes(33)                                      # what stands for the signer of a channel whose announcement is cut off before its ids


def view(blob, verdict=None):
    """-> dict(scids: [scid] (the channel numbers: entries ascending, then the bare ones ascending), chan: {scid: number},
    rec: [(ann, u0, u1)] (NONE: none), ts: [[ts0, ts1]] (the SIGNED timestamps of the slots' records), ids: [(id1, id2) or None], dying: [bool],
    recs: the walk's records)"""
    d = sqm.directory(blob, verdict)
    recs = d["recs"]
    entries = crm.sorted_digest(blob, verdict, recs)[0]
    scids = [e[0] for e in entries] + list(d["bare"])
    rec = [tuple(e[3]) for e in entries] + [(a, NONE, NONE) for a in d["bare_rec"]]
    ts = [list(e[1]) for e in entries] + [[0, 0] for _ in d["bare"]]
    ids, dying = [], []
    for a, _, _ in rec:
        m = recs[a][4]
        f = int.from_bytes(m[258:260], "big")
        ids.append((m[300 + f:333 + f], m[333 + f:366 + f]) if len(m) >= 366 + f else None)
        dying.append(bool(recs[a][1] & F_DYING))
    return dict(scids=scids, chan={s: k for k, s in enumerate(scids)}, rec=rec, ts=ts, ids=ids, dying=dying, recs=recs)


def signature_in_range(m):
    return int.from_bytes(m[2:34], "big") < N_ORDER and int.from_bytes(m[34:66], "big") < N_ORDER


def receive(v, msgs, chain, now, check, prune_interval=0, our_id=None, peers=None, held=()):
    """check(msg, id33) -> True when the signature verifies under id33.  peers: None, or one id or None per message.
    -> dict(status, flags, chan, signer (the id each checked message was checked under, None: not checked), add_msg, records (the bytes of each
    added record), del_rec (ascending), sets [(rec, ts, crc)], final {(chan, dir): ts in force} of the slots the batch touched)"""
    prune = prune_interval or 1209600
    n = len(msgs)
    status, flags, chan, signer = [None] * n, [0] * n, [NONE] * n, [None] * n
    in_force = {}                                        # (chan, dir) -> [ts or None, the image record or None, the accepted message or None]
    has_update = {}                                      # chan -> does either slot hold a record?
    held = set(held)
    dels, sets = [], []
    for i, m in enumerate(msgs):
        m = bytes(m)
        if len(m) < 138 or len(m) > 65535 or m[:2] != b"\x01\x02" or not signature_in_range(m):
            status[i] = MALFORMED
            continue
        if m[66:98] != chain:
            status[i] = WRONG_CHAIN
            continue
        scid, ts, mflags, cflags = int.from_bytes(m[98:106], "big"), int.from_bytes(m[106:110], "big"), m[110], m[111]
        if ts > ((now + 86400) & U64) or ts < ((now - prune) & U64):
            status[i] = TIMESTAMP
            continue
        if scid in held:
            status[i] = HELD
            continue
        c = v["chan"].get(scid)
        peer = None if peers is None else (peers[i] or NO_KEY)   # in a list of peers 33 zero bytes stand for "no source": they verify nothing
        if c is None:
            if peer is not None:
                signer[i] = bytes(peer)
                if check(m, signer[i]):
                    status[i], flags[i] = PRIVATE, PEER_UPDATE
                    continue
            status[i] = UNKNOWN
            continue
        chan[i] = c
        d = cflags & 1
        signer[i] = v["ids"][c][d] if v["ids"][c] is not None else NO_KEY
        if not check(m, signer[i]):
            status[i] = BAD_SIGNATURE
            continue
        if mflags & 2:
            status[i] = DONT_FORWARD
            continue
        if c not in has_update:
            has_update[c] = v["rec"][c][1] != NONE or v["rec"][c][2] != NONE
        slot = in_force.setdefault((c, d), [v["ts"][c][d], v["rec"][c][1 + d], None] if v["rec"][c][1 + d] != NONE else [None, None, None])
        if slot[0] is not None and ts <= slot[0]:
            status[i] = STALE if ts < slot[0] else DUPLICATE
            continue
        status[i] = ACCEPTED
        if slot[0] is None and not has_update[c]:
            flags[i] |= FIRST
            a = v["rec"][c][0]
            sets.append((a, ts, sa.crc32c(ts, v["recs"][a][4])))
        has_update[c] = True
        if v["dying"][c]:
            flags[i] |= DYING
        if slot[1] is not None:
            dels.append(slot[1])
        if slot[2] is not None:
            flags[slot[2]] |= SUPERSEDED
        if our_id is not None and v["ids"][c] is not None and v["ids"][c][1 - d] == bytes(our_id):
            flags[i] |= PEER_UPDATE
        slot[0], slot[1], slot[2] = ts, None, i
    add_msg = [i for i in range(n) if status[i] == ACCEPTED]
    records = []
    for i in add_msg:
        m, ts = bytes(msgs[i]), int.from_bytes(msgs[i][106:110], "big")
        hf = 0x2000 | (F_DYING if flags[i] & DYING else 0) | (0x8000 if flags[i] & SUPERSEDED else 0)
        records.append(struct.pack(">HHII", hf, len(m), sa.crc32c(ts, m), ts) + m)
    return dict(status=status, flags=flags, chan=chan, signer=signer, add_msg=add_msg, records=records, del_rec=sorted(dels), sets=sets,
                final={k: s[0] for k, s in in_force.items() if s[2] is not None})


def apply(blob, v, r):
    """the image after the batch: DELETED set on del_rec, the re-stamped announcement headers, the added records behind the old end"""
    out = bytearray(blob)
    for k in r["del_rec"]:
        out[v["recs"][k][0]] |= 0x80
    for a, ts, crc in r["sets"]:
        o = v["recs"][a][0]
        out[o + 4:o + 12] = struct.pack(">II", crc, ts)
    return bytes(out) + b"".join(r["records"])


# ---- builders shared by the host-build test and the device test: a signed store and a batch that meets every status and flag
T0 = 1_700_000_000 - 5000                                # the stores' timestamps lie around it; `now` of the tests is 1_700_000_000
NOW = 1_700_000_000


def checker(orc):
    """check(msg, id33) for receive(): the C oracle's sigcheck_channel_update, memoised (one batch is checked by several tests)"""
    memo = {}

    def check(m, id33):
        k = (bytes(m), bytes(id33))
        if k not in memo:
            memo[k] = orc.sigcheck_channel_update(k[0], k[1]) == 0
        return memo[k]
    return check


def hand_net(orc, seed=7):
    """a gossip_stream.Net of 9 nodes and 12 channels with DISTINCT scids; channels 0 .. 7 go into hand_store(), 8 .. 11 stay unknown"""
    import gossip_stream as gs
    net = gs.Net(orc, seed, n_nodes=9, n_chans=12)
    for c, ch in enumerate(net.chans):
        ch["scid"] = crm.scid_of(700_000 + 3 * c, 5 + c, c & 1)
    return net


def hand_store(net, chain):
    """-> the image: channel 0 with both updates, 1 with direction 0 alone, 2 and 3 bare (3's announcement DYING), 4 with both updates and a
    deleted older one, 5 bare, 6 with both, 7 bare.  The announcements are signed: the image passes the audit."""
    r = []
    for c in range(8):
        r += [crm.rec(net.cann(c, chain=chain), 0, sa.F_COMPLETED | (F_DYING if c == 3 else 0)), crm.rec(crm.AMOUNT)]
    for c, d, ts, flags in ((0, 0, T0, 0), (0, 1, T0 + 1, 0), (1, 0, T0 + 2, 0), (4, 0, T0 - 50, sa.F_DELETED), (4, 0, T0 + 3, 0), (4, 1, T0 + 4, 0), (6, 0, T0 + 5, 0),
                            (6, 1, T0 + 6, 0)):
        r.append(crm.rec(net.cupd(c, d, ts, chain=chain, extra=bytes(c)), ts, sa.F_COMPLETED | flags))
    return sa.serialise(0x10, r)


def hand_batch(net, chain, other_chain):
    """-> (msgs, peers, held, our_id): every status and every flag, odd lengths (so the offsets take every residue mod 4).  The peer of every
    message is node 1; our_id is a node of channel 6."""
    import gossip_stream as gs
    u = lambda c, d, ts, **kw: net.cupd(c, d, ts, chain=chain, **kw)
    peer_sk = net.node_sk[1]
    newer = u(0, 0, T0 + 10, extra=b"\x01")
    m = [newer, newer, u(0, 0, T0 - 5), u(0, 0, T0, extra=b"ab"), u(0, 0, T0 + 20, extra=b"abc"), u(0, 1, T0 + 30),
         gs.damage(net.rnd, u(0, 1, T0 + 40), "sig"), gs.damage(net.rnd, u(0, 1, T0 + 41), "r>=n"), u(0, 1, T0 + 42, mflags=3),
         net.cupd(0, 1, T0 + 43, chain=other_chain), u(0, 1, NOW + 86401), u(0, 1, NOW + 86400, extra=b"x"), u(0, 1, NOW - 1209601), u(1, 1, NOW - 1209600),
         u(5, 0, T0 + 50), u(9, 0, T0 + 51),                                      # held: a known and an unknown channel
         u(8, 0, T0 + 52, signer=peer_sk), u(8, 1, T0 + 53), u(10, 0, T0 + 54, signer=peer_sk, mflags=3),      # private, unknown, private
         u(2, 1, T0 + 60, extra=b"12345"), u(2, 0, T0 + 61), u(2, 1, T0 + 62), u(2, 1, T0 + 62, extra=b"z"),   # FIRST; not FIRST; supersedes; duplicate
         u(3, 0, T0 + 70), u(6, 0, T0 + 80), u(6, 1, T0 + 81), u(1, 1, T0 + 82),                               # DYING + FIRST; PEER_UPDATE one way or the other
         u(1, 0, T0 + 90)[:137], b"\x01\x01" + u(1, 0, T0 + 91)[2:], u(1, 0, T0 + 92) + b"\x00", b"", b"\x01",
         u(4, 0, T0 + 3 + 1, signer=net.node_sk[net.chans[4]["n"][1]]), u(4, 0, T0 + 3), u(4, 0, T0 - 50), u(4, 1, T0 + 100, extra=bytes(47)),
         u(7, 1, T0 + 110), u(7, 1, T0 + 105), u(7, 0, T0 + 111, mflags=0), u(0, 0, 0xFFFFFFFF), gs.damage(net.rnd, u(6, 0, T0 + 200), "tail")]
    m[29] = m[29][:-1] + b"\x07"                         # a trailing byte that was not signed: the signature fails
    held = [net.chans[5]["scid"], net.chans[9]["scid"]]
    return m, [net.node_id[1]] * len(m), held, net.node_id[net.chans[6]["n"][0]]

"""A sequential restatement of what lamd_node_announcement_receive_batch (include/lightning_amd.h) computes, for the tests of the device code
(test_gpu_node_receive.py) and of its host build (test_store_nodes_host.py).  It is written from the receive path of the reference,
gossmap_manage_node_announcement() / process_node_announcement() / all_node_channels_dying() (gossipd/gossmap_manage.c:288-298, 1122-1248),
fromwire_wireaddr_array (common/wireaddr.c:30-69, 858-889), fromwire_tlv (wire/tlvstream.c) and gossip_store_add / _del
(gossipd/gossip_store.c): ONE message at a time, in arrival order, with a dict node -> (timestamp, record).
  - view(): what the directory says about an image: the node ids ranked by memcmp, each node's announcement record in force and its HEADER
    timestamp, whether all of a node's channels are dying;
  - receive(): the statuses, flags, node ranks and the plan;
  - apply(): the plan applied to the image, as the file stands after the reference has processed the batch."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import scid_query_model as sqm  # noqa: E402
import test_store_audit as sa  # noqa: E402

NONE = 0xFFFFFFFF
MALFORMED, ACCEPTED, BAD_ADDRESSES, BAD_SIGNATURE, HELD, UNKNOWN, STALE, DUPLICATE = -1, 0, 1, 2, 3, 4, 5, 6
SUPERSEDED, DYING = 1, 4
F_DYING = 0x0800
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def view(blob, verdict=None):
    """-> dict(ids: [id33] ascending, rank: {id: rank}, nann: [record or NONE], ts: [header timestamp of that record or None], dying: [bool: every
    channel of the node carries DYING on its announcement record], scids: [scid] (entries, then bare), chan_rec: [announcement record],
    chan_rank: [(rank1, rank2)], entries: how many of the channels are digest entries, ent_rec: their (announcement, update 0, update 1), node_off: [image offset of the id inside the first announcement that names it], recs: the walk's records)"""
    d = sqm.directory(blob, verdict)
    recs = d["recs"]
    ids = list(d["nodes"])
    scids = list(d["entries"]) + list(d["bare"])
    alive = [False] * len(ids)
    for s in scids:
        if not recs[d["chan"][s][0]][1] & F_DYING:
            for r in d["ranks"][s]:
                if r != NONE:
                    alive[r] = True
    node_off = []
    for nid, a in zip(ids, d["first"]):
        m = recs[a][4]
        f = int.from_bytes(m[258:260], "big")
        node_off.append(recs[a][0] + 12 + (300 + f if m[300 + f:333 + f] == nid else 333 + f))
    return dict(ids=ids, rank={x: r for r, x in enumerate(ids)}, nann=list(d["nann"]), ts=[None if k == NONE else recs[k][3] for k in d["nann"]],
                dying=[not a for a in alive], scids=scids, chan_rec=[d["chan"][s][0] for s in scids], chan_rank=[d["ranks"][s] for s in scids],
                node_off=node_off, recs=recs, entries=len(d["entries"]), ent_rec=[tuple(d["chan"][s]) for s in d["entries"]])


def tlvs_ok(b):
    """node_ann_tlvs under fromwire_tlv's rules: strictly ascending types, lengths inside the message, an unknown even type fails, an unknown odd
    one is skipped; type 1 (option_will_fund): u16 u16 u16 u32 tu32 = 10 .. 14 bytes, the tu32 minimal"""
    pos, prev = 0, None
    while pos < len(b):
        t = crm.read_bigsize(b, pos)
        if t is None:
            return False
        typ, pos = t
        if prev is not None and typ <= prev:
            return False
        prev = typ
        if typ != 1 and typ % 2 == 0:
            return False
        t = crm.read_bigsize(b, pos)
        if t is None:
            return False
        ln, pos = t
        if ln > len(b) - pos:
            return False
        if typ == 1 and (ln < 10 or ln > 14 or (ln > 10 and b[pos + 10] == 0)):
            return False
        pos += ln
    return True


def addresses_ok(b):
    """fromwire_wireaddr_array: a descriptor cut off anywhere fails; an unknown type ends the walk; port 0 is skipped, no error"""
    pos = 0
    while pos < len(b):
        t = b[pos]
        pos += 1
        if t == 5:
            if pos >= len(b):
                return False
            alen = b[pos]
            pos += 1
        elif t in (1, 2, 3, 4):
            alen = {1: 4, 2: 16, 3: 10, 4: 35}[t]
        else:
            return True
        if len(b) - pos < alen + 2:
            return False
        pos += alen + 2
    return True


def parse(m):
    """fromwire_node_announcement -> (timestamp, node id, addresses) or None: malformed"""
    if len(m) < 142 or len(m) > 65535 or m[:2] != b"\x01\x01":
        return None
    if int.from_bytes(m[2:34], "big") >= N_ORDER or int.from_bytes(m[34:66], "big") >= N_ORDER:
        return None
    f = int.from_bytes(m[66:68], "big")
    k = 68 + f + 4                                        # node_id 33 | rgb 3 | alias 32 | addrlen 2 | addresses | tlvs
    if len(m) < k + 70:
        return None
    end = k + 70 + int.from_bytes(m[k + 68:k + 70], "big")
    if len(m) < end or not tlvs_ok(m[end:]):
        return None
    return int.from_bytes(m[k - 4:k], "big"), m[k:k + 33], m[k + 70:end]


def receive(v, msgs, check, pending=False):
    """check(msg) -> True when the signature verifies under the message's own node_id.
    -> dict(status, flags, node, checked (was the signature looked at?), add_msg, records (the bytes of each added record), del_rec (ascending),
    final {rank: (ts in force, the message that holds it)} of the nodes the batch touched)"""
    n = len(msgs)
    status, flags, node, checked = [None] * n, [0] * n, [NONE] * n, [False] * n
    in_force = {}                                        # rank -> [ts or None, the image record or None, the accepted message or None]
    dels = []
    for i, m in enumerate(msgs):
        m = bytes(m)
        p = parse(m)
        if p is None:
            status[i] = MALFORMED
            continue
        ts, nid, addrs = p
        if not addresses_ok(addrs):
            status[i] = BAD_ADDRESSES
            continue
        checked[i] = True
        if not check(m):
            status[i] = BAD_SIGNATURE
            continue
        r = v["rank"].get(nid)
        if r is None:
            status[i] = HELD if pending else UNKNOWN
            continue
        node[i] = r
        slot = in_force.setdefault(r, [v["ts"][r], v["nann"][r], None] if v["nann"][r] != NONE else [None, None, None])
        if slot[0] is not None and ts <= slot[0]:
            status[i] = STALE if ts < slot[0] else DUPLICATE
            continue
        status[i] = ACCEPTED
        if v["dying"][r]:
            flags[i] |= DYING
        if slot[1] is not None:
            dels.append(slot[1])
        if slot[2] is not None:
            flags[slot[2]] |= SUPERSEDED
        slot[0], slot[1], slot[2] = ts, None, i
    add_msg = [i for i in range(n) if status[i] == ACCEPTED]
    records = []
    for i in add_msg:
        m = bytes(msgs[i])
        ts = parse(m)[0]
        hf = 0x2000 | (F_DYING if flags[i] & DYING else 0) | (0x8000 if flags[i] & SUPERSEDED else 0)
        records.append(struct.pack(">HHII", hf, len(m), sa.crc32c(ts, m), ts) + m)
    return dict(status=status, flags=flags, node=node, checked=checked, add_msg=add_msg, records=records, del_rec=sorted(dels),
                final={r: (s[0], s[2]) for r, s in in_force.items() if s[2] is not None})


def apply(blob, v, r):
    """the image after the batch: DELETED set on del_rec, the added records behind the old end"""
    out = bytearray(blob)
    for k in r["del_rec"]:
        out[v["recs"][k][0]] |= 0x80
    return bytes(out) + b"".join(r["records"])


# ---- builders shared by the host-build test and the device test: a signed store and a batch that meets every status and flag
T0 = 1_700_000_000 - 5000


def checker(orc):
    """check(msg) for receive(): the C oracle's sigcheck_node_announcement, memoised (one batch is checked by several tests)"""
    memo = {}

    def check(m):
        k = bytes(m)
        if k not in memo:
            memo[k] = orc.sigcheck_node_announcement(k) == 0
        return memo[k]
    return check


def nann(net, sk, nid, ts, addrs=b"", tlvs=b"", features=b""):
    """a node_announcement for ANY 33 id bytes, signed with sk"""
    r = net.rnd
    body = len(features).to_bytes(2, "big") + features + ts.to_bytes(4, "big") + bytes(nid) + bytes(r.randrange(256) for _ in range(3))
    body += bytes(r.randrange(32, 127) for _ in range(32)) + len(addrs).to_bytes(2, "big") + addrs + tlvs
    return b"\x01\x01" + net.sign(sk, body) + body


# who owns which channel of hand_store(): node 3 and node 4 have dying channels only, node 5 a dying one and a single live one, node 8 none
PAIRS = ((0, 1), (0, 2), (3, 4), (3, 5), (5, 6), (6, 7), (1, 2), (0, 7), (8, 0), (8, 1), (8, 2), (8, 3))
DYING_CHANNELS = (2, 3)
TWIN_SCID = crm.scid_of(699_000, 1, 0)


def hand_net(orc, seed=11):
    """a gossip_stream.Net of 9 nodes and 12 channels with DISTINCT scids and the owners of PAIRS; channels 0 .. 7 go into hand_store()"""
    import gossip_stream as gs
    net = gs.Net(orc, seed, n_nodes=9, n_chans=12)
    for c, ch in enumerate(net.chans):
        ch["scid"] = crm.scid_of(700_000 + 3 * c, 5 + c, c & 1)
        a, b = PAIRS[c]
        ch["n"] = (a, b) if net.node_id[a] < net.node_id[b] else (b, a)
    return net


def twin_of(nid):
    """the id that equals nid in its first 32 bytes and differs in the 33rd"""
    return nid[:32] + bytes([nid[32] ^ 1])


def hand_store(net, chain, twins=False):
    """-> the image: channels 0 .. 7 (2 and 3 DYING) and the announcements of node 0 (T0), node 1 (timestamp 0), node 2 (signed T0 + 5 under a
    header that says T0 + 9), node 3 (T0 + 1; all its channels are dying) and node 6 (a deleted one of T0 - 50, then T0 + 3); nodes 4, 5 and 7
    have none.  Everything is signed: the image passes the audit -- unless twins is set: then an unsigned channel_announcement in front names
    twin_of(node 0's id) and twin_of(node 7's id), so that the directory ranks each of the two next to an id it shares 32 bytes with."""
    r = []
    if twins:
        r += [crm.rec(sqm.cann_ids(TWIN_SCID, *sorted((twin_of(net.node_id[0]), twin_of(net.node_id[7]))))), crm.rec(crm.AMOUNT)]
    for c in range(8):
        r += [crm.rec(net.cann(c, chain=chain), 0, sa.F_COMPLETED | (F_DYING if c in DYING_CHANNELS else 0)), crm.rec(crm.AMOUNT)]
    for n, ts, hdr_ts, flags in ((0, T0, T0, 0), (1, 0, 0, 0), (2, T0 + 5, T0 + 9, 0), (3, T0 + 1, T0 + 1, F_DYING), (6, T0 - 50, T0 - 50, sa.F_DELETED),
                                 (6, T0 + 3, T0 + 3, 0)):
        r.append(crm.rec(net.nann(n, ts, addrs=bytes([1, 10, 0, 0, n, 0x26, 0x07])), hdr_ts, sa.F_COMPLETED | flags))
    return sa.serialise(0x10, r)


ADDR = {1: b"\x01" + bytes(range(4)) + b"\x26\x07", 2: b"\x02" + bytes(range(16)) + b"\x26\x07", 3: b"\x03" + bytes(range(10)) + b"\x26\x07",
        4: b"\x04" + bytes(range(35)) + b"\x26\x07", 5: b"\x05\x0bexample.com\x26\x07"}
LEASE = struct.pack(">HHHI", 1, 2, 3, 4)                 # lease_rates in front of its tu32


def hand_batch(net):
    """-> [(name, msg)]: every status and every flag, odd lengths (so the offsets take every residue mod 4); the names say what each one is"""
    import gossip_stream as gs
    sk, nid = net.node_sk, net.node_id
    mk = lambda n, ts, **kw: nann(net, sk[n], nid[n], ts, **kw)
    neg = lambda n: (N_ORDER - int.from_bytes(sk[n], "big")).to_bytes(32, "big")      # the key of the same x with the other parity
    flip = lambda x: bytes([x[0] ^ 1]) + x[1:]
    newer = mk(0, T0 + 10, addrs=ADDR[1])
    b = [("newer", newer), ("its copy", newer), ("stale", mk(0, T0 - 5)), ("equal to the record's", mk(0, T0, addrs=ADDR[2])),
         ("newer still", mk(0, T0 + 20, features=b"\x01\x02\x03")),
         ("length 142", mk(7, T0 + 1)), ("length 141", mk(7, T0 + 2)[:141]), ("flen 5", mk(7, T0 + 3, features=bytes(5)))]
    b += [("address type %d" % t, mk(7, T0 + 10 + t, addrs=ADDR[t])) for t in range(1, 6)]
    b += [("address type %d cut" % t, mk(7, T0 + 20 + t, addrs=ADDR[t][:-1])) for t in range(1, 6)]
    b += [("all address types", mk(7, T0 + 30, addrs=b"".join(ADDR[t] for t in range(1, 6)))), ("type 5 of length 0", mk(7, T0 + 31, addrs=b"\x05\x00\x26\x07")),
          ("type 5 cut behind its length", mk(7, T0 + 32, addrs=ADDR[1] + b"\x05\x03")), ("type 5 cut behind its type", mk(7, T0 + 33, addrs=b"\x05")),
          ("type 1 cut behind its type", mk(7, T0 + 33, addrs=ADDR[2] + b"\x01")), ("port 0", mk(7, T0 + 34, addrs=b"\x01" + bytes(4) + b"\x00\x00" + ADDR[1])),
          ("unknown type, then garbage", mk(7, T0 + 35, addrs=ADDR[1] + b"\x09\xff\x05")), ("port 0 cut", mk(7, T0 + 36, addrs=b"\x01" + bytes(4) + b"\x00"))]
    b += [("tlv 1 of 10", mk(5, T0 + 40, tlvs=b"\x01\x0a" + LEASE)), ("tlv 1 of 14", mk(5, T0 + 41, tlvs=b"\x01\x0e" + LEASE + b"\x01\x00\x00\x00")),
          ("tlv 1 of 9", mk(5, T0 + 42, tlvs=b"\x01\x09" + LEASE[:9])), ("tlv 1 of 11, not minimal", mk(5, T0 + 43, tlvs=b"\x01\x0b" + LEASE + b"\x00")),
          ("tlv 1 of 15", mk(5, T0 + 43, tlvs=b"\x01\x0f" + LEASE + b"\x01\x00\x00\x00\x00")), ("unknown odd tlv", mk(5, T0 + 44, tlvs=b"\x03\x02ab")),
          ("unknown even tlv", mk(5, T0 + 45, tlvs=b"\x02\x02ab")), ("descending tlvs", mk(5, T0 + 46, tlvs=b"\x03\x00\x01\x0a" + LEASE)),
          ("ascending tlvs", mk(5, T0 + 47, tlvs=b"\x01\x0a" + LEASE + b"\x03\x00", addrs=ADDR[3])), ("tlv length past the end", mk(5, T0 + 48, tlvs=b"\x03\x05ab")),
          ("tlv 1 of 11", mk(5, T0 + 39, tlvs=b"\x01\x0b" + LEASE + b"\x07"))]
    good = mk(4, T0 + 50)
    b += [("r = n", good[:2] + N_ORDER.to_bytes(32, "big") + good[34:]), ("s = n", good[:34] + N_ORDER.to_bytes(32, "big") + good[66:]),
          ("a signature bit", gs.damage(net.rnd, mk(4, T0 + 51), "sig")), ("a signed byte", gs.damage(net.rnd, mk(4, T0 + 52), "tail")),
          ("type 258", b"\x01\x02" + good[2:]), ("empty", b""), ("one byte", b"\x01"), ("addrlen past the end", mk(4, T0 + 53, addrs=ADDR[1])[:-1]),
          ("an unsigned trailing byte", mk(4, T0 + 54) + b"\x05\x00")]
    b += [("id with first byte 5", nann(net, sk[4], b"\x05" + nid[4][1:], T0 + 55)), ("the twin of node 0", nann(net, sk[0], twin_of(nid[0]), T0 + 56)),
          ("node 0 beside its twin", mk(0, T0 + 21, addrs=b"\x63")), ("node 7 beside its twin", mk(7, T0 + 37)),
          ("node 0's x, the other parity", nann(net, neg(0), flip(nid[0]), T0 + 57)), ("node 8, in no channel", mk(8, T0 + 58, addrs=ADDR[4]))]
    b += [("ts 0, record of ts 0", mk(1, 0)), ("ts 1, record of ts 0", mk(1, 1)), ("ts 2^32 - 1, a record", mk(1, 0xFFFFFFFF)), ("after 2^32 - 1", mk(1, T0)),
          ("ts 0, no record", mk(4, 0)), ("ts 0 again", mk(4, 0, addrs=ADDR[5])), ("ts 2^32 - 1, no record", mk(4, 0xFFFFFFFF, addrs=b"\x07")),
          ("between signed and header", mk(2, T0 + 7)), ("the header's", mk(2, T0 + 9)), ("past the header", mk(2, T0 + 10)),
          ("all channels dying, a record", mk(3, T0 + 60)), ("and again", mk(3, T0 + 61, addrs=bytes(3))), ("one live channel", mk(5, T0 + 62)),
          ("the deleted record's", mk(6, T0 - 50)), ("the live record's", mk(6, T0 + 3)), ("past the live record", mk(6, T0 + 4, features=b"\x80"))]
    return b

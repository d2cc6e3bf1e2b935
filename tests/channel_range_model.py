"""A sequential restatement of what lamd_gossip_store_digest_build and lamd_channel_range_reply_batch (include/lightning_amd.h) compute, for the
tests of the device code (test_channel_range.py) and of its host build (test_store_digest_host.py):
  - digest(): a gossmap-style pass over the records in file order (common/gossmap.c: add_channel, update_channel);
  - gather_range(): connectd/queries.c gather_range() in the reference's order (gossmap index order = file order of the announcements) or sorted;
  - limit(), split(), encode(): max_entries(), queue_channel_ranges(), towire_reply_channel_range();
  - parse_query(): fromwire_query_channel_range with fromwire_tlv's rules;
  - replies(): all of it for one raw query.
CRC-32C is test_store_audit's; test_channel_range_model.py pins it by the RFC 3720 check value and the header CRCs of the golden stores."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_store_audit as sa  # noqa: E402

NONE = 0xFFFFFFFF
OK = 0
CHAIN = bytes(range(32, 64))


def update_csum(m):
    """crc32_of_update: the update without its signature and its timestamp"""
    return sa.crc32c(sa.crc32c(0, m[66:106]), m[110:])


def digest(blob, verdict=None, recs=None):
    """-> (entries in the REFERENCE's order [(scid, (ts0, ts1), (csum0, csum1), (rec_ann, rec_u0, rec_u1))], counters dict).  recs: the walk's
    records, or any list of (off, flags, crc, ts, msg) that stands for rec_off"""
    recs = sa.walk(blob)[0] if recs is None else recs
    chans, order = {}, []                                 # scid -> [ann index, u0, u1]
    c = dict(records=len(recs), channels=0, entries=0, channels_no_update=0, updates_no_channel=0, updates_in_front=0, updates_short=0)
    counting = lambda i: not recs[i][1] & sa.F_DELETED and (verdict is None or verdict[i] == OK)
    # the index holds announcements of the WHOLE file: an update in front of its channel is told apart from one without any
    first = {}
    for i, r in enumerate(recs):
        if counting(i) and sa._cann_scid(r[4]):
            first.setdefault(sa._cann_scid(r[4])[0], i)
    for i, r in enumerate(recs):
        if not counting(i):
            continue
        m = r[4]
        k = sa._cann_scid(m)
        if k:
            if first[k[0]] == i:
                chans[k[0]] = [i, None, None]
                order.append(k[0])
        elif m[:2] == b"\x01\x02":
            if len(m) < 112:
                c["updates_short"] += 1
                continue
            scid = int.from_bytes(m[98:106], "big")
            if scid not in first:
                c["updates_no_channel"] += 1
            elif first[scid] >= i:
                c["updates_in_front"] += 1
            else:
                chans[scid][1 + (m[111] & 1)] = i          # last in file order wins
    out = []
    for scid in order:
        a, u0, u1 = chans[scid]
        c["channels"] += 1
        if u0 is None and u1 is None:
            c["channels_no_update"] += 1
            continue
        ups = [recs[u][4] if u is not None else None for u in (u0, u1)]
        out.append((scid, tuple(int.from_bytes(m[106:110], "big") if m else 0 for m in ups), tuple(update_csum(m) if m else 0 for m in ups),
                    (a, NONE if u0 is None else u0, NONE if u1 is None else u1)))
    c["entries"] = len(out)
    return out, c


def sorted_digest(blob, verdict=None, recs=None):
    e, c = digest(blob, verdict, recs)
    return sorted(e, key=lambda x: x[0]), c


def bigsize(v):
    if v < 0xfd:
        return bytes([v])
    if v <= 0xffff:
        return b"\xfd" + struct.pack(">H", v)
    if v <= 0xffffffff:
        return b"\xfe" + struct.pack(">I", v)
    return b"\xff" + struct.pack(">Q", v)


def read_bigsize(b, pos):
    """-> (value, new pos) or None: cut off, or not minimally encoded"""
    if pos >= len(b):
        return None
    t = b[pos]
    if t < 0xfd:
        return t, pos + 1
    w, low = {0xfd: (2, 0xfd), 0xfe: (4, 0x10000), 0xff: (8, 0x100000000)}[t]
    if len(b) - pos - 1 < w:
        return None
    v = int.from_bytes(b[pos + 1:pos + 1 + w], "big")
    return (v, pos + 1 + w) if v >= low else None


def query(chain, first, number, option=None, tlvs=b""):
    """a raw query_channel_range; option: the query_option value (None: no TLV 1); tlvs: raw bytes appended behind it"""
    q = struct.pack(">H", 263) + chain + struct.pack(">II", first, number)
    if option is not None:
        v = bigsize(option)
        q += b"\x01" + bigsize(len(v)) + v
    return q + tlvs


def parse_query(q):
    """-> (chain, first, number, option) or None (malformed)"""
    if len(q) < 42 or q[:2] != struct.pack(">H", 263):
        return None
    pos, prev, option = 42, None, 0
    while pos < len(q):
        r = read_bigsize(q, pos)
        if r is None:
            return None
        t, pos = r
        if prev is not None and t <= prev:
            return None
        prev = t
        if t != 1 and t % 2 == 0:
            return None
        r = read_bigsize(q, pos)
        if r is None:
            return None
        ln, pos = r
        if ln > len(q) - pos:
            return None
        if t == 1:
            r = read_bigsize(q[:pos + ln], pos)
            if r is None or r[1] != pos + ln:
                return None
            option = r[0]
        pos += ln
    return q[2:34], int.from_bytes(q[34:38], "big"), int.from_bytes(q[38:42], "big"), option


def limit(opts, max_encoded_bytes=0):
    """max_entries()"""
    nbytes, per_entry = 65535 - 2 - (32 + 4 + 4 + 1 + 2), 8
    max_num = nbytes // per_entry
    for bit in (1, 2):
        if opts & bit:
            nbytes -= 1 + len(bigsize(max_num * 8))
            per_entry += 8
    if max_encoded_bytes and nbytes > max_encoded_bytes:
        nbytes = max_encoded_bytes
    nbytes = max(nbytes, per_entry)
    return nbytes // per_entry


def fix_number(first, number):
    return 0xFFFFFFFF - first if first + number > 0xFFFFFFFF else number


def gather_range(entries, first, number):
    """the entries (in the order given) whose block lies in [first, first + number - 1]; number is the fixed-up one"""
    if number == 0:
        return []
    end = first + number - 1
    return [e for e in entries if first <= e[0] >> 40 <= end]


def split(sel, first, number, lim):
    """queue_channel_ranges() over ASCENDING entries -> [(first, blocks, entries, sync_complete)]"""
    out, off = [], 0
    blk = lambda k: sel[k][0] >> 40
    while True:
        rem = len(sel) - off
        if rem <= lim:
            n, blocks = rem, number
        else:
            n = lim
            while n > 0 and blk(off + n - 1) == blk(off + lim):
                n -= 1
            if n == 0:
                n = lim
            blocks = blk(off + n) - first
        out.append((first, blocks, sel[off:off + n], int(blocks == number)))
        first, number, off = first + blocks, number - blocks, off + n
        if number == 0:
            return out


def encode(chain, first, blocks, entries, final, opts):
    n = len(entries)
    m = struct.pack(">H", 264) + chain + struct.pack(">IIBH", first, blocks, final, 1 + 8 * n) + b"\x00" + b"".join(struct.pack(">Q", e[0]) for e in entries)
    if opts & 1:
        m += b"\x01" + bigsize(1 + 8 * n) + b"\x00" + b"".join(struct.pack(">II", *e[1]) for e in entries)
    if opts & 2:
        m += b"\x03" + bigsize(8 * n) + b"".join(struct.pack(">II", *e[2]) for e in entries)
    return m


def replies(sorted_entries, our_chain, q, max_encoded_bytes=0):
    """-> (status, [reply bytes]) for one raw query over the sorted digest"""
    p = parse_query(q)
    if p is None:
        return -1, []
    chain, first, number, option = p
    if chain != our_chain:
        return 1, [struct.pack(">H", 264) + chain + struct.pack(">IIBH", first, number, 0, 0)]
    opts = option & 3
    number = fix_number(first, number)
    sel = gather_range(sorted_entries, first, number)
    return 0, [encode(chain, f, b, e, s, opts) for f, b, e, s in split(sel, first, number, limit(opts, max_encoded_bytes))]


def decode_reply(m):
    """-> dict(chain, first, blocks, final, scids, ts (list of pairs or None), csum (list of pairs or None)); asserts the framing"""
    assert m[:2] == struct.pack(">H", 264)
    first, blocks, final, ln = struct.unpack(">IIBH", m[34:45])
    d = dict(chain=m[2:34], first=first, blocks=blocks, final=final, scids=[], ts=None, csum=None)
    if ln == 0:
        assert len(m) == 45
        return d
    assert m[45] == 0 and (ln - 1) % 8 == 0
    n = (ln - 1) // 8
    d["scids"] = [int.from_bytes(m[46 + 8 * k:54 + 8 * k], "big") for k in range(n)]
    pos = 45 + ln
    while pos < len(m):
        t, pos = read_bigsize(m, pos)
        l, pos = read_bigsize(m, pos)
        v = m[pos:pos + l]
        assert len(v) == l
        pos += l
        if t == 1:
            assert l == 1 + 8 * n and v[0] == 0
            d["ts"] = [struct.unpack(">II", v[1 + 8 * k:9 + 8 * k]) for k in range(n)]
        else:
            assert t == 3 and l == 8 * n
            d["csum"] = [struct.unpack(">II", v[8 * k:8 * k + 8]) for k in range(n)]
    return d


# ---- hand-built stores: no valid signatures, CRCs valid all the same (serialise computes them)
def cann(scid, tag=0):
    m = bytearray(b"\x55" * 430)
    m[0:2] = b"\x01\x00"
    m[258:260] = b"\x00\x00"
    m[292:300] = struct.pack(">Q", scid)
    m[300:333] = bytes([2]) + bytes([tag & 0xff]) * 32
    m[333:366] = bytes([3]) + bytes([(tag >> 8) & 0xff]) * 32
    return bytes(m)


def cupd(scid, direction, ts, length=138, fill=0x33):
    m = bytearray(bytes([(fill + 7 * k) & 0xff for k in range(length)]))
    m[0:2] = b"\x01\x02"
    if length >= 106:
        m[98:106] = struct.pack(">Q", scid)
    if length >= 110:
        m[106:110] = struct.pack(">I", ts)
    if length >= 112:
        m[111] = (m[111] & 0xfe) | direction
    return bytes(m)


AMOUNT = b"\x10\x05" + bytes(8)


def rec(msg, ts=0, flags=sa.F_COMPLETED):
    return dict(flags=flags, ts=ts, msg=msg, crc=None)


def channel_store(scids, both=False):
    """one channel per scid, in the order given: announcement, amount, an update of direction (k & 1) -- and of the other one with `both`"""
    recs = []
    for k, s in enumerate(scids):
        recs += [rec(cann(s, k)), rec(AMOUNT), rec(cupd(s, k & 1, 1000 + k, 130 + k % 9), 1000 + k)]
        if both:
            recs.append(rec(cupd(s, 1 - (k & 1), 2000 + k, 136), 2000 + k))
    return sa.serialise(0x10, recs)


def scid_of(block, tx=0, out=0):
    return (block << 40) | (tx << 16) | out


# ---- stores and query sets shared by the host-build test and the device test
def fast_rec(msg, ts=0, flags=sa.F_COMPLETED):
    """a record whose header CRC is not computed (the digest reads none unless verdicts are given)"""
    return dict(flags=flags, ts=ts, msg=msg, crc=0)


def big_store(scids):
    """channel_store without header CRCs: for the stores of thousands of channels"""
    recs = []
    for k, s in enumerate(scids):
        recs += [fast_rec(cann(s, k)), fast_rec(AMOUNT), fast_rec(cupd(s, k & 1, 1000 + k, 130 + k % 9), 1000 + k)]
    return sa.serialise(0x10, recs)


def population_store(pops, start=100, gap=3):
    """blocks start, start + gap, ... holding pops[k] channels each, written in DESCENDING scid order"""
    scids = [scid_of(start + gap * k, t, t & 1) for k, p in enumerate(pops) for t in range(p)]
    return big_store(scids[::-1])


def slot_store():
    """every slot case of the digest in one store -> (image, {name: scid})"""
    recs, names = [], {}
    state = {"next": 500}

    def chan(name):
        s = scid_of(state["next"], 1, 0)
        state["next"] += 2
        names[name] = s
        recs.extend([fast_rec(cann(s, len(names))), fast_rec(AMOUNT)])
        return s
    chan("no_update")
    s = chan("dir0")
    recs.append(fast_rec(cupd(s, 0, 11)))
    s = chan("dir1")
    recs.append(fast_rec(cupd(s, 1, 12)))
    s = chan("both")
    recs += [fast_rec(cupd(s, 1, 13)), fast_rec(cupd(s, 0, 14, 150))]
    s = chan("replaced")
    recs += [fast_rec(cupd(s, 0, 9000, 140, 0x11)), fast_rec(cupd(s, 0, 8000, 141, 0x22))]          # the later one wins, lower timestamp or not
    s = chan("deleted_behind")
    recs += [fast_rec(cupd(s, 1, 20, 138, 0x44)), fast_rec(cupd(s, 1, 21, 138, 0x45), flags=sa.F_COMPLETED | sa.F_DELETED)]
    s = scid_of(state["next"], 1, 0)
    names["in_front"] = s
    state["next"] += 2
    recs += [fast_rec(cupd(s, 0, 30)), fast_rec(cann(s, 77)), fast_rec(AMOUNT), fast_rec(cupd(s, 1, 31))]
    recs.append(fast_rec(cupd(scid_of(3, 3, 3), 0, 40)))                                           # no such channel
    s = chan("short")
    recs += [fast_rec(cupd(s, 0, 50, 111)), fast_rec(cupd(s, 1, 51, 112))]
    s = chan("twice")
    recs += [fast_rec(cupd(s, 0, 60)), fast_rec(cann(s, 99)), fast_rec(AMOUNT), fast_rec(cupd(s, 1, 61))]
    size = 1 + sum(12 + len(r["msg"]) for r in recs)
    k = 0
    for length in range(112, 151):                                                                 # the CRC heads and tails: every length at every alignment
        for al in range(4):
            s = chan("crc_%d_%d" % (length, al))
            size += 12 + 430 + 12 + 10
            f = 2 + (al - (size + 12 + 2)) % 4
            recs.append(fast_rec(b"\x10\x0b" + bytes(f - 2)))
            size += 12 + f
            assert size % 4 == al
            recs.append(fast_rec(cupd(s, k & 1, 70 + k, length, 0x50 + k)))
            size += 12 + length
            k += 1
    blob = sa.serialise(0x10, recs)
    assert len(blob) == size
    return blob, names


FOREIGN = bytes(range(64, 96))


def query_kinds(blocks, chain=CHAIN):
    """one query of every kind the replies are tested with, over a store whose channels lie in `blocks` (a non-empty list) -> [raw query]"""
    lo, hi = min(blocks), max(blocks)
    inner = sorted(set(blocks))
    gap = next(((a + 1, b - a - 1) for a, b in zip(inner, inner[1:]) if b - a > 1), (hi + 5, 2))
    span = hi - lo + 1
    ranges = [(0, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0, 0xFFFFFFFF),                   # the whole chain, all four option combinations
              (lo, 0), (lo, 0xFFFFFFFF), (lo + 1, 0xFFFFFFFF), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF),   # nothing asked; first + number overflows
              (0, lo), (hi + 1, 1000), (0x1000000, 5), gap,                                          # below, above, beyond 24 bits, between
              (lo, span), (lo + 1, span - 1), (max(lo, 1) - 1, span + 1), (lo, span - 1), (lo, span + 1), (lo, 1), (hi, 1), (hi, 2), (lo - 1 if lo else 0, 1)]
    out = [query(chain, f, n, None if k % 5 == 4 else k % 4) for k, (f, n) in enumerate(ranges)]
    out[0] = query(chain, 0, 0xFFFFFFFF)                                                             # no TLV at all
    out.append(query(FOREIGN, lo, span, 3))
    out.append(query(chain, lo, span, 7, b"\x03\x02\xaa\xbb"))                                       # other option bits, an unknown odd type
    out.append(query(chain, lo, span, 0x100))
    out += [query(chain, lo, span, 3, b"\x04\x00"), query(chain, lo, span)[:41], b"\x01\x08" + query(chain, lo, span)[2:], b"",
            query(chain, lo, span, None, b"\x01\x03\xfd\x00\x03"), query(chain, lo, span, 1, b"\x01\x01\x02")]   # malformed, each in its way
    return out


def mixed_queries(blocks, count, chain=CHAIN):
    """`count` queries, the kinds in turn, the malformed ones spread between the good ones"""
    kinds = query_kinds(blocks, chain)
    good, bad = kinds[:-6], kinds[-6:]
    seq = []
    for k in range(count):
        seq.append(bad[(k // 4) % len(bad)] if k % 4 == 3 else good[(k - k // 4) % len(good)])
    return seq

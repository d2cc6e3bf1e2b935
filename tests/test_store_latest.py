"""The latest-wins repair of a gossip_store FILE (lamd_gossip_store_repair_latest, include/lightning_amd.h): the repair, and of the records that
pass it only the one gossipd's receive path would hold -- against a SEQUENTIAL restatement of the rules written here (latest_model: the records
in file order through `prev_timestamp >= timestamp: ignore`, then the prune pass, then the keep pass; verdicts by test_store_audit.model, i.e.
signatures by the C oracle), which the device's order-free atomicMax form must equal in reasons, new offsets, output bytes and every counter.
Stores: the two the reference's gossipd wrote, the synthetic one of test_store_audit and its damaged copy (clock off: the plain repair, byte
for byte), and hand-built ones -- replays, bad records, header / future timestamps, stale channels, one hot slot over block and wave edges,
winners and losers in different blocks, seeded duplicates injected into the synthetic store.
CPU: the struct layouts, the model on the hand-built stores, the precondition of the equality with the plain repair.  GPU: the device."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gossip_stream as gs  # noqa: E402
import test_store_audit as sa  # noqa: E402
import test_store_repair as sr  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)
from test_store_repair import AMOUNT, UUID, _rec  # noqa: E402

ROOT = sa.ROOT
OK, F_DELETED = sa.OK, sa.F_DELETED
KEPT, R_DELETED, R_VERDICT, R_DEPENDENCY, R_BOOKKEEPING, R_SUPERSEDED, R_TIMESTAMP, R_STALE = range(8)
DROPPED = sr.DROPPED
SLACK, PRUNE = 86_400, 1_209_600          # the reference's: a day ahead of the clock, two weeks of silence
NOW = gs.NOW
COUNTERS = ("kept", "dropped_deleted", "dropped_verdict", "dropped_dependency", "dropped_bookkeeping", "dropped_superseded", "dropped_timestamp",
            "dropped_stale")
OFF = dict(now=0, future_slack=SLACK, prune_interval=PRUNE)


# ------------------------------------------------------------------------------------------------ the model
def signed_ts(m):
    """the signed timestamp of a channel_update / node_announcement long enough to hold what the keep rules read, else None"""
    if m[:2] == b"\x01\x02" and len(m) >= 112:
        return int.from_bytes(m[106:110], "big")
    if m[:2] == b"\x01\x01" and len(m) >= 68:
        o = 68 + int.from_bytes(m[66:68], "big")
        if len(m) >= o + 4 + 33:
            return int.from_bytes(m[o:o + 4], "big")
    return None


def latest_model(blob, verdicts, uuid, now=0, future_slack=SLACK, prune_interval=PRUNE):
    """the rules of lamd_gossip_store_repair_latest as gossipd would arrive at them: ONE walk over the records in file order that feeds each
    eligible update / node_announcement to `prev_timestamp >= timestamp: ignore`, the prune pass over the channels, the keep pass
    -> (reasons, new_off, output image)"""
    recs = sa.walk(blob)[0]
    n = len(recs)
    live = [not r[1] & F_DELETED for r in recs]
    typ = [int.from_bytes(r[4][:2], "big") if live[i] else 0 for i, r in enumerate(recs)]
    first = {}                                            # scid -> the indexed announcement
    for i, r in enumerate(recs):
        if live[i] and sa._cann_scid(r[4]):
            first.setdefault(sa._cann_scid(r[4])[0], i)

    def eligible(i):
        ts = signed_ts(recs[i][4])
        return typ[i] in (257, 258) and verdicts[i] == OK and ts is not None and recs[i][3] == ts and (now == 0 or ts <= now + future_slack)

    def nann_id(m):
        o = 68 + int.from_bytes(m[66:68], "big") + 4
        return m[o:o + 33]

    reason = [None] * n
    for i, r in enumerate(recs):                          # provisional announcements: the plain repair's
        if typ[i] != 256:
            continue
        if verdicts[i] != OK:
            reason[i] = R_VERDICT
        elif not (i + 1 < n and live[i + 1] and typ[i + 1] == 4101 and len(recs[i + 1][4]) == 10 and verdicts[i + 1] == OK):
            reason[i] = R_DEPENDENCY
        else:
            reason[i] = KEPT
    held, dying = {}, set()                               # (announcement, direction) -> (ts, record) gossipd holds; announcements with a dying record
    for i, r in enumerate(recs):                          # the receive path, in file order
        m = r[4]
        if typ[i] == 258 and eligible(i):
            a = first.get(int.from_bytes(m[98:106], "big"))
            if a is None or a >= i or reason[a] != KEPT:
                continue
            ts, prev = signed_ts(m), held.get((a, m[111] & 1))
            if prev is not None and prev[0] >= ts:
                continue                                  # gossmap_manage.c:934-945
            held[(a, m[111] & 1)] = (ts, i)
        elif typ[i] == 4106 and verdicts[i] == OK and len(m) == 14:
            a = first.get(int.from_bytes(m[2:10], "big"))
            if a is not None and a < i:
                dying.add(a)
    nodes = {}                                            # node id -> lowest index of a FINALLY kept announcement that names it
    for a, r in enumerate(recs):                          # prune_network
        if typ[a] != 256 or reason[a] != KEPT:
            continue
        if now and prune_interval and a not in dying and any((a, d) in held and held[(a, d)][0] + prune_interval < now for d in (0, 1)):
            reason[a] = R_STALE
            continue
        o = sa._cann_scid(r[4])[1]
        for k in (r[4][o:o + 33], r[4][o + 33:o + 66]):
            nodes.setdefault(k, a)
    nheld = {}
    for i, r in enumerate(recs):                          # node_announcements, in file order (gossmap_manage.c:1134-1143)
        if typ[i] == 257 and eligible(i) and nodes.get(nann_id(r[4]), n) < i:
            ts, prev = signed_ts(r[4]), nheld.get(nann_id(r[4]))
            if prev is None or prev[0] < ts:
                nheld[nann_id(r[4])] = (ts, i)
    kept_cann = lambda j: 0 <= j < n and typ[j] == 256 and reason[j] == KEPT
    for i, r in enumerate(recs):                          # the keep pass
        m, t = r[4], typ[i]
        if t == 256:
            continue
        if not live[i]:
            x = R_DELETED
        elif verdicts[i] == sa.NO_CHANNEL:
            x = R_DEPENDENCY
        elif verdicts[i] != OK:
            x = R_VERDICT
        elif t in (4103, 4105, 4107):
            x = R_BOOKKEEPING
        elif t == 4101:
            x = KEPT if kept_cann(i - 1) else R_DEPENDENCY
        elif t in (258, 4106):
            if t == 4106 and len(m) != 14:
                x = R_VERDICT
            else:
                a = first.get(int.from_bytes(m[98:106] if t == 258 else m[2:10], "big"))
                x = KEPT if a is not None and a < i and kept_cann(a) else R_DEPENDENCY
                if t == 258:
                    if not eligible(i):
                        x = R_TIMESTAMP
                    elif x == KEPT and held[(a, m[111] & 1)][1] != i:
                        x = R_SUPERSEDED
        elif t == 257:
            x = KEPT if nodes.get(nann_id(m), n) < i else R_DEPENDENCY
            if not eligible(i):
                x = R_TIMESTAMP
            elif x == KEPT and nheld[nann_id(m)][1] != i:
                x = R_SUPERSEDED
        else:
            x = R_VERDICT
        reason[i] = x
    out = bytearray([blob[0]]) + sr.uuid_record(uuid)
    new_off = []
    for i, r in enumerate(recs):
        new_off.append(len(out) if reason[i] == KEPT else DROPPED)
        if reason[i] == KEPT:
            out += blob[r[0]:r[0] + 12 + len(r[4])]
    return reason, new_off, bytes(out)


# ------------------------------------------------------------------------------------------------ the hand-built stores
def _net(orc, seed, pairs):
    """a Net whose channel c joins the nodes pairs[c] (node_id_1 < node_id_2, as the announcement requires)"""
    net = gs.Net(orc, seed, n_nodes=1 + max(max(p) for p in pairs), n_chans=len(pairs))
    for ch, (a, b) in zip(net.chans, pairs):
        ch["n"] = (a, b) if net.node_id[a] < net.node_id[b] else (b, a)
    assert len({ch["scid"] for ch in net.chans}) == len(pairs)
    return net


def _upd(net, c, d, ts, hdr=None):
    return _rec(net.cupd(c, d, ts), ts=ts if hdr is None else hdr)


def _nann(net, node, ts, hdr=None):
    return _rec(net.nann(node, ts), ts=ts if hdr is None else hdr)


def _chan(net, c):
    return _rec(net.cann(c), ts=5) + _rec(AMOUNT)


def _dying(net, c, ln=14):
    return _rec((b"\x10\x0a" + net.chans[c]["scid"].to_bytes(8, "big") + (800_100).to_bytes(4, "big") + bytes(ln))[:ln])


def replay_store(orc):
    """one channel; direction 0 updated at 100, 300, 200 (file order), direction 1 twice at 50; node A announced at 10, 30, 20, node B once"""
    net = _net(orc, 91, [(0, 1)])
    a, b = net.chans[0]["n"]
    blob = bytes([0x10]) + _chan(net, 0) + b"".join(_upd(net, 0, 0, ts) for ts in (100, 300, 200)) + _upd(net, 0, 1, 50) + _upd(net, 0, 1, 50)
    blob += b"".join(_nann(net, a, ts) for ts in (10, 30, 20)) + _nann(net, b, 7)
    return blob, [KEPT, KEPT, R_SUPERSEDED, KEPT, R_SUPERSEDED, KEPT, R_SUPERSEDED, R_SUPERSEDED, KEPT, R_SUPERSEDED, KEPT]


def bad_record_store(orc):
    """channel 0: an update at 100, then one at 200 with a flipped signature bit.  Channel 1: a valid update at 200 IN FRONT of its announcement, one
    at 100 behind.  Channel 2: an update at 50, a second (REDUNDANT) copy of the announcement with its amount record, an update at 100"""
    net = _net(orc, 92, [(0, 1), (1, 2), (2, 3)])
    blob = bytes([0x10]) + _chan(net, 0) + _upd(net, 0, 0, 100) + _rec(sa._flip_sig(net.cupd(0, 0, 200), 0, 3), ts=200)
    blob += _upd(net, 1, 0, 200) + _chan(net, 1) + _upd(net, 1, 0, 100)
    blob += _chan(net, 2) + _upd(net, 2, 0, 50) + _chan(net, 2) + _upd(net, 2, 0, 100)
    return blob, [KEPT, KEPT, KEPT, R_VERDICT, R_DEPENDENCY, KEPT, KEPT, KEPT, KEPT, KEPT, R_SUPERSEDED, R_VERDICT, R_DEPENDENCY, KEPT]


def timestamp_store(orc, now):
    """channel 0 (nodes 0, 1): direction 0 -- header 400 over signed 500 (CRC over the header as it stands), then 300; direction 1 -- now + SLACK, then
    now + SLACK + 1; node 0 -- header 400 over signed 500, then 300; node 1 -- now + SLACK, then now + SLACK + 1.  Channel 1 (nodes 2, 3): the
    announcement's signature is bad; an update and a node_announcement with mismatching headers, and one of each with matching ones.
    The reasons are those under (now, SLACK, no prune interval: the channel's direction 0 was last updated at 300)"""
    net = _net(orc, 93, [(0, 1), (2, 3)])
    a, b = net.chans[0]["n"]
    blob = bytes([0x10]) + _chan(net, 0) + _upd(net, 0, 0, 500, hdr=400) + _upd(net, 0, 0, 300) + _upd(net, 0, 1, now + SLACK) + _upd(net, 0, 1, now + SLACK + 1)
    blob += _nann(net, a, 500, hdr=400) + _nann(net, a, 300) + _nann(net, b, now + SLACK) + _nann(net, b, now + SLACK + 1)
    blob += _rec(sa._flip_sig(net.cann(1), 2, 1), ts=5) + _rec(AMOUNT) + _upd(net, 1, 0, 77, hdr=78) + _upd(net, 1, 0, 77) + _nann(net, 2, 9, hdr=8) + _nann(net, 3, 9)
    return blob, [KEPT, KEPT, R_TIMESTAMP, KEPT, KEPT, R_TIMESTAMP, R_TIMESTAMP, KEPT, KEPT, R_TIMESTAMP,
                  R_VERDICT, R_DEPENDENCY, R_TIMESTAMP, R_DEPENDENCY, R_TIMESTAMP, R_DEPENDENCY]


def stale_store(orc, now):
    """X (nodes 0, 1): both directions at now - PRUNE.  Y (nodes 1, 2): direction 0 at now - PRUNE - 1, direction 1 at now; its dying record lies IN
    FRONT of the announcement (a dying record behind it would keep the channel, as Z's does).  Z (nodes 3, 4): direction 0 long silent, and a
    14-byte dying record.  W (nodes 5, 6): no update at all.  Then a node_announcement of the nodes 0, 1, 2, 3, 5.
    -> the image, the reasons under (now, SLACK, PRUNE), the records of Y the clock alone drops"""
    net = _net(orc, 94, [(0, 1), (1, 2), (3, 4), (5, 6)])
    blob = bytes([0x10]) + _chan(net, 0) + _upd(net, 0, 0, now - PRUNE) + _upd(net, 0, 1, now - PRUNE)
    blob += _dying(net, 1) + _chan(net, 1) + _upd(net, 1, 0, now - PRUNE - 1) + _upd(net, 1, 1, now)
    blob += _chan(net, 2) + _upd(net, 2, 0, now - PRUNE - 100) + _dying(net, 2)
    blob += _chan(net, 3)
    blob += b"".join(_nann(net, k, now - 50) for k in (0, 1, 2, 3, 5))
    reasons = [KEPT] * 4 + [R_DEPENDENCY, R_STALE, R_DEPENDENCY, R_DEPENDENCY, R_DEPENDENCY] + [KEPT] * 4 + [KEPT] * 2 + [KEPT, KEPT, R_DEPENDENCY, KEPT, KEPT]
    return blob, reasons, (5, 6, 7, 8, 17)


_EDGE = {}


def edge_store(orc, k, order):
    """the announcement, the amount record, k updates of direction 0: timestamps strictly rising, strictly falling, or all equal -> (image, the record kept)"""
    net = _net(orc, 95, [(0, 1)])
    head = bytes([0x10]) + _chan(net, 0)
    key = (k, order == "equal")
    if key not in _EDGE:                                  # rising and falling are the same signed records in opposite order
        _EDGE[key] = [_upd(net, 0, 0, 1000 if order == "equal" else 1000 + j) for j in range(k)]
    ups = _EDGE[key]
    return head + b"".join(reversed(ups) if order == "falling" else ups), 2 + (k - 1 if order == "rising" else 0)


SPREAD_CHANS = 600


def spread_store(orc):
    """600 channels, then three rounds of one update per (channel, direction): the three updates of a slot lie 1 200 records apart, their timestamps
    in an order that changes from slot to slot -> (image, the round that wins per channel)"""
    r = random.Random(96)
    pairs = [tuple(r.sample(range(40), 2)) for _ in range(SPREAD_CHANS)]
    net = _net(orc, 96, pairs)
    orders = [(100, 200, 300), (100, 300, 200), (200, 100, 300), (200, 300, 100), (300, 100, 200), (300, 200, 100), (100, 100, 50), (70, 90, 90)]
    blob = bytes([0x10]) + b"".join(_chan(net, c) for c in range(SPREAD_CHANS))
    for rnd in range(3):
        blob += b"".join(_upd(net, c, d, orders[(c + d) % 8][rnd]) for c in range(SPREAD_CHANS) for d in (0, 1))
    return blob, orders


def injected_store(orc, img):
    """the synthetic store with, behind each live channel_update and node_announcement, 0-3 freshly signed variants whose timestamps lie 5 below, at and 5
    above the original's, at seeded random places later in the file (never between an announcement and its amount record)"""
    net = gs.make_script(orc, sa.SEED, n_ops=sa.N_OPS, lifecycle=True)[0]
    by_scid, by_id = {ch["scid"]: c for c, ch in enumerate(net.chans)}, {k: j for j, k in enumerate(net.node_id)}
    r = random.Random(97)
    recs = [[blob] for blob in (img[o:o + 12 + len(m)] for o, _, _, _, m in sa.walk(img)[0])]       # per original record: itself, then what goes in behind it
    n, added = len(recs), 0
    info = sa.walk(img)[0]
    ok_slot = [not (not info[j][1] & F_DELETED and info[j][4][:2] == b"\x01\x00") for j in range(n)]   # nothing directly behind a live announcement
    for i, (_, flags, _, _, m) in enumerate(info):
        if flags & F_DELETED or m[:2] not in (b"\x01\x01", b"\x01\x02"):
            continue
        ts = signed_ts(m)
        for _ in range(r.randrange(4)):
            t2 = ts + r.choice((-5, 0, 5))
            if m[:2] == b"\x01\x02":
                new = _rec(net.cupd(by_scid[int.from_bytes(m[98:106], "big")], m[111] & 1, t2, disabled=bool(r.randrange(2))), ts=t2)
            else:
                o = 68 + int.from_bytes(m[66:68], "big") + 4
                new = _rec(net.nann(by_id[m[o:o + 33]], t2), ts=t2)
            j = r.choice([x for x in range(i, n) if ok_slot[x]])
            recs[j].insert(r.randrange(1, len(recs[j]) + 1), new)
            added += 1
    return img[:1] + b"".join(b"".join(x) for x in recs), added


class Stores:
    """the hand-built stores and their oracle verdicts, each built once per module"""
    def __init__(self, orc):
        self.orc, self._c = orc, {}

    def get(self, name, *args):
        if (name, args) not in self._c:
            built = globals()[name](self.orc, *args)
            self._c[(name, args)] = (built, sa.model(self.orc, built[0])[1])
        return self._c[(name, args)]


@pytest.fixture(scope="module")
def stores(orc):
    return Stores(orc)


# ------------------------------------------------------------------------------------------------ CPU
def _entry_refuses_a_null_context():
    """the entry point is exported and bound (no device is needed to be told LAMD_ERR_ARG)"""
    from lightning_amd import _ffi
    assert _ffi.load().lamd_gossip_store_repair_latest(None, None, 0, None, None, None, 0, None, None, None, None, None, None, None, 0, None, None) == -3


@pytest.mark.parametrize("name", ["Policy", "Summary"])
def test_latest_struct_layouts_match_the_header(tmp_path, name):
    """lamd_store_latest_policy / lamd_store_latest_summary <-> _ffi: size and every offset as a C compiler lays the header's declaration out, the same field
    names in the same order; the entry point is bound"""
    import re
    import subprocess
    from lightning_amd import Engine, _ffi
    cls, cname = getattr(_ffi, "LamdStoreLatest" + name), "lamd_store_latest_" + name.lower()
    fields = [f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n  printf("%%zu\\n", sizeof(%s));\n' % cname
                   + "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, f).offset for f in fields]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct[^{;]*\{([^}]*)\} %s;" % cname, hdr, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[[^\]]*\])?\s*[,;]", body) == fields
    assert callable(Engine.gossip_store_repair_latest) and "lamd_gossip_store_repair_latest" in _ffi.SYMBOLS
    _entry_refuses_a_null_context()


def _gossmap_last_in_file(blob, scid, d):
    """common/gossmap.c update_channel(): whichever live update of (scid, direction) comes last in the file"""
    ups = [m for _, f, _, _, m in sa.walk(blob)[0] if not f & F_DELETED and m[:2] == b"\x01\x02" and int.from_bytes(m[98:106], "big") == scid and m[111] & 1 == d]
    return signed_ts(ups[-1])


def test_model_of_the_hand_built_stores(orc, stores):
    """the sequential model gives the hand-built stores exactly the reasons their builders list; the plain repair's model keeps what replay needs it to"""
    _entry_refuses_a_null_context()
    (blob, want), v = stores.get("replay_store")
    assert set(v) == {OK} and latest_model(blob, v, UUID, **OFF)[0] == want
    assert set(sr.repair_model(blob, v, UUID)[0]) == {KEPT}
    scid = sa._cann_scid(sa.walk(blob)[0][0][4])[0]
    assert _gossmap_last_in_file(blob, scid, 0) == 200
    (blob, want), v = stores.get("bad_record_store")
    assert latest_model(blob, v, UUID, **OFF)[0] == want
    assert [v[i] for i in (3, 4, 11)] == [1, sa.NO_CHANNEL, sa.REDUNDANT] and all(x == OK for i, x in enumerate(v) if i not in (3, 4, 11))
    (blob, want), v = stores.get("timestamp_store", NOW)
    assert latest_model(blob, v, UUID, now=NOW, future_slack=SLACK, prune_interval=0)[0] == want
    off = latest_model(blob, v, UUID, **OFF)[0]           # without a clock the later timestamp wins
    assert [off[i] for i in (4, 5, 8, 9)] == [R_SUPERSEDED, KEPT, R_SUPERSEDED, KEPT] and off[:4] == want[:4] and off[10:] == want[10:]
    (blob, want, ys), v = stores.get("stale_store", NOW)
    assert set(v) == {OK} and latest_model(blob, v, UUID, now=NOW, future_slack=SLACK, prune_interval=PRUNE)[0] == want
    for pol in (dict(now=NOW, future_slack=SLACK, prune_interval=0), dict(now=0, future_slack=SLACK, prune_interval=PRUNE)):
        got = latest_model(blob, v, UUID, **pol)[0]
        assert got == sr.repair_model(blob, v, UUID)[0] == [KEPT if i in ys else x for i, x in enumerate(want)]
    for k in (63, 257):
        for order in ("rising", "falling", "equal"):
            (blob, keep), v = stores.get("edge_store", k, order)
            got = latest_model(blob, v, UUID, **OFF)[0]
            assert got.count(KEPT) == 3 and got[keep] == KEPT and got.count(R_SUPERSEDED) == k - 1
    (blob, orders), v = stores.get("spread_store")
    got = latest_model(blob, v, UUID, **OFF)[0]
    assert set(v) == {OK} and got.count(KEPT) == 4 * SPREAD_CHANS and got.count(R_SUPERSEDED) == 4 * SPREAD_CHANS
    for c in (0, 7, 599):
        for d in (0, 1):
            o = orders[(c + d) % 8]
            win = o.index(max(o))
            assert [got[2 * SPREAD_CHANS * (1 + rnd) + 2 * c + d] == KEPT for rnd in range(3)] == [rnd == win for rnd in range(3)]


def test_model_without_a_clock_equals_the_plain_repair_on_the_four_stores(orc, synthetic, damaged):
    """none of the four holds a live 257 / 258 whose header timestamp differs from the signed one, or two live OK records of one slot: the new call with the clock
    off must give the plain repair's output"""
    _entry_refuses_a_null_context()
    blobs = [(sa._golden(name),) * 2 for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin")]
    for blob, v in [(b, sa.model(orc, b)[1]) for b, _ in blobs] + [(synthetic[0], synthetic[1][1]), (damaged[0], damaged[1][1])]:
        assert latest_model(blob, v, UUID, **OFF) == sr.repair_model(blob, v, UUID)


def test_injected_duplicates_give_the_model_something_to_drop(orc, synthetic, stores):
    _entry_refuses_a_null_context()
    (blob, added), v = stores.get("injected_store", synthetic[0])
    assert added >= 30 and len(v) == len(synthetic[1][1]) + added and set(v) <= {OK, sa.DELETED}
    got = latest_model(blob, v, UUID, **OFF)[0]
    assert got.count(R_SUPERSEDED) == added and got.count(KEPT) == latest_model(synthetic[0], synthetic[1][1], UUID, **OFF)[0].count(KEPT)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def _same(got, blob, want_verdicts, want):
    """the device's (out, rec_off, verdict, new_off, reason, summary, latest summary) against the model's (reasons, new_off, image)"""
    out, off, v, new_off, reason, s, r = got
    wreason, wnew, wout = want
    assert list(off) == [x[0] for x in sa.walk(blob)[0]] and list(v) == list(want_verdicts)
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(reason, wreason)) if a != b]
    assert not bad and len(reason) == len(wreason), bad[:10]
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(new_off, wnew)) if int(a) != b]
    assert not bad, bad[:10]
    assert r["out_len"] == len(wout) == len(out)
    if out != wout:
        k = next(i for i, (a, b) in enumerate(zip(out, wout)) if a != b)
        raise AssertionError("output differs from byte %d on: %s / %s" % (k, out[k:k + 16].hex(), wout[k:k + 16].hex()))
    assert [r[k] for k in COUNTERS] == [wreason.count(k) for k in range(8)]
    assert len(out) <= len(blob) + 46


def _closure(eng, out, pol, kept):
    """the output audits clean, the plain repair drops its uuid record alone, and the same call on it returns it"""
    _, v, s = eng.gossip_store_audit(out)
    assert s["clean"] == 1 and s["records"] == kept + 1 == s["ok"], s
    plain = eng.gossip_store_repair(out, UUID)
    assert plain[0] == out and plain[6]["kept"] == kept and plain[6]["dropped_bookkeeping"] == 1 and list(plain[4]).count(KEPT) == kept
    again = eng.gossip_store_repair_latest(out, UUID, **pol)
    assert again[0] == out and [again[6][k] for k in COUNTERS] == [kept, 0, 0, 0, 1, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_without_a_clock_the_reference_stores_repair_as_the_plain_repair_and_compactd(eng, name):
    blob = sa._golden(name)
    got, plain = eng.gossip_store_repair_latest(blob, UUID), eng.gossip_store_repair(blob, UUID)
    assert got[0] == plain[0] == sr.compactd_first_phase(blob, UUID)
    assert [list(got[k]) for k in (1, 2, 3, 4)] == [list(plain[k]) for k in (1, 2, 3, 4)]
    assert [got[6][k] for k in COUNTERS] == [len(got[1]), 0, 0, 0, 0, 0, 0, 0] and got[6]["out_len"] == len(blob) + 46


@pytest.mark.gpu
def test_without_a_clock_the_synthetic_and_the_damaged_store_repair_as_the_plain_repair(eng, orc, synthetic, damaged):
    for blob, v in ((synthetic[0], synthetic[1][1]), (damaged[0], damaged[1][1])):
        got, plain = eng.gossip_store_repair_latest(blob, UUID, now=0), eng.gossip_store_repair(blob, UUID)
        assert got[0] == plain[0]
        assert [list(got[k]) for k in (1, 2, 3, 4)] == [list(plain[k]) for k in (1, 2, 3, 4)]
        assert [got[6][k] for k in COUNTERS[:5] + ("out_len",)] == [plain[6][k] for k in COUNTERS[:5] + ("out_len",)]
        _same(got, blob, v, latest_model(blob, v, UUID, **OFF))


@pytest.mark.gpu
def test_replayed_updates_and_node_announcements(eng, stores):
    (blob, want), v = stores.get("replay_store")
    _, av, s = eng.gossip_store_audit(blob)
    assert s["clean"] == 1                                # the audit has nothing to say about this store
    plain = eng.gossip_store_repair(blob, UUID)
    assert list(plain[4]) == [KEPT] * len(want)           # ... the plain repair keeps every record
    scid = sa._cann_scid(sa.walk(blob)[0][0][4])[0]
    assert _gossmap_last_in_file(plain[0], scid, 0) == 200    # ... and gossmap routes on the replayed update
    got = eng.gossip_store_repair_latest(blob, UUID)
    assert list(got[4]) == want
    _same(got, blob, v, latest_model(blob, v, UUID, **OFF))
    assert _gossmap_last_in_file(got[0], scid, 0) == 300 and got[6]["dropped_superseded"] == 5
    _closure(eng, got[0], OFF, want.count(KEPT))


@pytest.mark.gpu
def test_a_record_that_is_not_ok_never_supersedes(eng, stores):
    (blob, want), v = stores.get("bad_record_store")
    got = eng.gossip_store_repair_latest(blob, UUID)
    assert list(got[4]) == want
    _same(got, blob, v, latest_model(blob, v, UUID, **OFF))
    _closure(eng, got[0], OFF, want.count(KEPT))


@pytest.mark.gpu
def test_header_and_future_timestamps(eng, stores):
    (blob, want), v = stores.get("timestamp_store", NOW)
    pol = dict(now=NOW, future_slack=SLACK, prune_interval=0)
    got = eng.gossip_store_repair_latest(blob, UUID, **pol)
    assert list(got[4]) == want and got[6]["dropped_timestamp"] == 6
    _same(got, blob, v, latest_model(blob, v, UUID, **pol))
    _closure(eng, got[0], pol, want.count(KEPT))
    for pol in (OFF, dict(now=NOW, future_slack=SLACK + 1, prune_interval=0), dict(now=NOW + 1, future_slack=SLACK, prune_interval=0),
                dict(now=NOW, future_slack=0, prune_interval=0), dict(now=2 ** 64 - 1, future_slack=2 ** 32 - 1, prune_interval=0)):
        _same(eng.gossip_store_repair_latest(blob, UUID, **pol), blob, v, latest_model(blob, v, UUID, **pol))


@pytest.mark.gpu
def test_stale_channels(eng, stores):
    (blob, want, ys), v = stores.get("stale_store", NOW)
    pol = dict(now=NOW, future_slack=SLACK, prune_interval=PRUNE)
    got = eng.gossip_store_repair_latest(blob, UUID, **pol)
    assert list(got[4]) == want and got[6]["dropped_stale"] == 1
    _same(got, blob, v, latest_model(blob, v, UUID, **pol))
    _closure(eng, got[0], pol, want.count(KEPT))
    for pol in (dict(now=NOW, future_slack=SLACK, prune_interval=0), OFF):      # no interval, no clock: Y stays
        got = eng.gossip_store_repair_latest(blob, UUID, **pol)
        assert list(got[4]) == [KEPT if i in ys else x for i, x in enumerate(want)]
        _same(got, blob, v, latest_model(blob, v, UUID, **pol))
    for pol in (dict(now=NOW - 1, future_slack=SLACK, prune_interval=PRUNE), dict(now=NOW + 1, future_slack=SLACK, prune_interval=PRUNE),
                dict(now=1000, future_slack=2 ** 32 - 1, prune_interval=PRUNE), dict(now=2 ** 33, future_slack=SLACK, prune_interval=2 ** 32 - 1)):
        _same(eng.gossip_store_repair_latest(blob, UUID, **pol), blob, v, latest_model(blob, v, UUID, **pol))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["rising", "falling", "equal"])
@pytest.mark.parametrize("k", [63, 64, 65, 254, 255, 256, 257, 4096])
def test_one_slot_over_wave_and_block_edges(eng, stores, k, order):
    """k updates of ONE (channel, direction): around a wave (64 lanes) and a block (256), and 4 096 -- every lane of 16 blocks on one address"""
    (blob, keep), v = stores.get("edge_store", k, order)
    got = eng.gossip_store_repair_latest(blob, UUID)
    reason = list(got[4])
    assert reason[:2] == [KEPT, KEPT] and reason[keep] == KEPT and reason.count(KEPT) == 3 and reason.count(R_SUPERSEDED) == k - 1
    _same(got, blob, v, latest_model(blob, v, UUID, **OFF))


@pytest.mark.gpu
def test_winners_and_losers_in_different_blocks(eng, stores):
    (blob, _), v = stores.get("spread_store")
    got = eng.gossip_store_repair_latest(blob, UUID)
    assert got[6]["kept"] == 4 * SPREAD_CHANS == got[6]["dropped_superseded"]
    _same(got, blob, v, latest_model(blob, v, UUID, **OFF))


@pytest.mark.gpu
def test_injected_duplicates_on_the_synthetic_store(eng, synthetic, stores):
    (blob, added), v = stores.get("injected_store", synthetic[0])
    for pol in (OFF, dict(now=NOW + 3600, future_slack=SLACK, prune_interval=PRUNE)):
        want = latest_model(blob, v, UUID, **pol)
        got = eng.gossip_store_repair_latest(blob, UUID, **pol)
        _same(got, blob, v, want)
        assert got[6]["dropped_superseded"] >= 1
        _closure(eng, got[0], pol, want[0].count(KEPT))


@pytest.mark.gpu
def test_resident_input_and_output_and_the_documented_return_codes(eng, stores):
    import torch
    from lightning_amd import _ffi
    (blob, wreason), v = stores.get("replay_store")
    want = latest_model(blob, v, UUID, **OFF)
    host = eng.gossip_store_repair_latest(blob, UUID)
    assert host[0] == want[2]
    for shift in (0, 1, 2, 3):                            # the image and the output at odd device addresses too; the output buffer exactly as long as needed
        d = torch.zeros(len(blob) + shift, dtype=torch.uint8, device="cuda")
        d[shift:] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((len(want[2]) + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        lo = (4 - shift) % 4
        exact = d_out[lo:lo + len(want[2])]
        got = eng.gossip_store_repair_latest(blob, UUID, d_store=d[shift:], d_out=exact, host_out=shift == 0)
        assert got[0] == (want[2] if shift == 0 else None)
        torch.cuda.synchronize()
        back = d_out.cpu().numpy().tobytes()
        assert back[lo:lo + len(want[2])] == want[2] and set(back[:lo] + back[lo + len(want[2]):]) <= {0xAB}
        assert [list(got[k]) for k in (1, 2, 3, 4)] == [list(host[k]) for k in (1, 2, 3, 4)] and got[6]["out_len"] == len(want[2])
    d_big = torch.full((len(blob) + 46,), 0xCD, dtype=torch.uint8, device="cuda")      # a roomy device buffer, no host copy
    got = eng.gossip_store_repair_latest(blob, UUID, d_out=d_big, host_out=False)
    torch.cuda.synchronize()
    assert d_big.cpu().numpy().tobytes()[:got[6]["out_len"]] == want[2]
    out, off, vv, new_off, reason, s, r = eng.gossip_store_repair_latest(b"\x0d", UUID, now=NOW)      # a store holding only its version byte
    assert out == b"\x0d" + sr.uuid_record(UUID) and len(off) == 0 and s["clean"] == 1 and r["kept"] == 0 and r["out_len"] == 47
    # the documented return codes
    lib, ctx = eng._lib, eng._ctx
    buf, uu = np.frombuffer(blob, dtype=np.uint8), np.frombuffer(UUID, dtype=np.uint8)
    n = len(v)
    o, vb, no, rs = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    cnt, st, rp, pol = ctypes.c_size_t(0), _ffi.LamdStoreSummary(), _ffi.LamdStoreLatestSummary(), _ffi.LamdStoreLatestPolicy(0, SLACK, PRUNE)
    small = np.full(len(want[2]), 0xEE, dtype=np.uint8)
    call = lambda cap, out, d_out, out_cap, p=ctypes.byref(pol): lib.lamd_gossip_store_repair_latest(
        ctx, buf.ctypes.data, len(blob), None, uu.ctypes.data, p, cap, o.ctypes.data, vb.ctypes.data, no.ctypes.data, rs.ctypes.data, ctypes.byref(cnt), out, d_out,
        out_cap, ctypes.byref(st), ctypes.byref(rp))
    assert call(3, small.ctypes.data, None, len(small)) == -3 and cnt.value == n                   # too few entries: the count needed
    assert call(n, small.ctypes.data, None, len(small) - 1) == -3 and rp.out_len == len(want[2])    # output too small: the size needed, the rest filled in
    assert list(rs) == want[0] and list(no) == want[1] and list(vb) == v and set(small) == {0xEE} and rp.dropped_superseded == 5
    d_small = torch.full((len(want[2]) + 4,), 0xAB, dtype=torch.uint8, device="cuda")
    assert call(n, None, d_small.data_ptr(), len(want[2]) - 5) == -3 and rp.out_len == len(want[2])
    torch.cuda.synchronize()
    assert set(d_small.cpu().numpy().tobytes()[len(want[2]) - 5:]) == {0xAB}                        # nothing written behind out_cap
    assert call(n, None, None, 0) == 0 and rp.out_len == len(want[2]) and rp.kept == want[0].count(KEPT)   # the maps and the counters only
    assert call(n, small.ctypes.data, None, len(small), None) == -3 and set(small) == {0xEE}       # no policy
    assert call(n, small.ctypes.data, None, len(small)) == 0 and small.tobytes() == want[2]
    v1 = np.frombuffer(b"\x20" + blob[1:], dtype=np.uint8)
    assert lib.lamd_gossip_store_repair_latest(ctx, v1.ctypes.data, len(blob), None, uu.ctypes.data, ctypes.byref(pol), n, o.ctypes.data, vb.ctypes.data, no.ctypes.data,
                                               rs.ctypes.data, ctypes.byref(cnt), None, None, 0, ctypes.byref(st), ctypes.byref(rp)) == -3 and cnt.value == 0

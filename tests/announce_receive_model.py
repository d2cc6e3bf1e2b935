"""A sequential restatement of what lamd_channel_announcement_receive_batch and lamd_channel_announcement_confirm_batch (include/lightning_amd.h)
compute, for the tests of the device code (test_gpu_announce_receive.py) and of its host build (test_store_announce_host.py).  It is written from
the reference's text: gossmap_manage_channel_announcement() and gossmap_manage_handle_get_txout_reply() (gossipd/gossmap_manage.c:620-874),
node_announcements_not_dying() (:603-618), fromwire_channel_announcement (wire/peer_wire.csv), is_scid_depth_announceable()
(bitcoin/short_channel_id.h:82-87), bitcoin_redeem_2of2() / scriptpubkey_p2wsh() (bitcoin/script.c:149-165) and gossip_store_add
(gossipd/gossip_store.c:49-78): ONE message or reply at a time, with dicts for known / pending / early / failures.
  - receive(): status, scid, script per message, the ask list, and how many messages took the signature batch / the key parse alone;
  - confirm(): status and pending index per reply, the new failures, the record pairs, the node_announcement headers that lose DYING;
  - apply(): the confirm plan applied to the image.
The script is hashlib's; the signature verdicts and the validity of a key come from the oracle."""
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import node_receive_model as nrm  # noqa: E402
import test_store_audit as sa  # noqa: E402

NONE = 0xFFFFFFFF
N_ORDER = nrm.N_ORDER
F_DYING = 0x0800
MALFORMED, PENDING, ID_ORDER, WRONG_CHAIN, TXOUT_FAILED, KNOWN, BAD_ORDER, IN_BATCH, EARLY = -1, 0, 1, 2, 3, 4, 9, 10, 11
ACCEPTED, NOT_PENDING, NO_OUTPUT, WRONG_SCRIPT, REDUNDANT = 0, 1, 2, 3, 4
U32 = 0xFFFFFFFF


def frame(m):
    """the framing of fromwire_channel_announcement and the range of its eight scalars -> dict or None: malformed"""
    m = bytes(m)
    if len(m) < 432 or len(m) > 65535 or m[:2] != b"\x01\x00":
        return None
    f = int.from_bytes(m[258:260], "big")
    k = 260 + f + 40                                       # node_id_1 | node_id_2 | bitcoin_key_1 | bitcoin_key_2
    if len(m) < k + 132:
        return None
    for s in range(8):
        if int.from_bytes(m[2 + 32 * s:34 + 32 * s], "big") >= N_ORDER:
            return None
    return dict(chain=m[k - 40:k - 8], scid=int.from_bytes(m[k - 8:k], "big"), ids=(m[k:k + 33], m[k + 33:k + 66]), keys=(m[k + 66:k + 99], m[k + 99:k + 132]))


def script_of(key1, key2):
    lo, hi = sorted((bytes(key1), bytes(key2)))             # pubkey_cmp: memcmp of the serialised keys
    return b"\x00\x20" + hashlib.sha256(b"\x52\x21" + lo + b"\x21" + hi + b"\x52\xae").digest()


def blocknum(scid):
    return scid >> 40


def announceable(scid, height):
    return ((blocknum(scid) + 6 - 1) & U32) <= height


def receive(known, msgs, chain, blockheight, check, key_ok, held=(), failed=()):
    """known: the scids of the image's channels; check(msg) -> 0 or the first bad signature 1 .. 4; key_ok(key33) -> does fromwire_pubkey take it?
    -> dict(status, scid, spk ([34 bytes]), ask_msg, ask_scid, sig_rows, key_rows, pending {scid: message}, early {scid: message})"""
    n = len(msgs)
    status, scids, spk = [None] * n, [0] * n, [bytes(34)] * n
    known, held, failed = set(known), set(held), set(failed)
    pending, early, asks = {}, {}, []
    sig_rows = key_rows = 0
    for i, m in enumerate(msgs):
        m = bytes(m)
        p = frame(m)
        if p is None:
            status[i] = MALFORMED
            continue
        # the device decides the filters in front of the key parse; a message a filter drops has its two bitcoin keys parsed alone
        filt = None
        if not p["ids"][0] < p["ids"][1]:
            filt = ID_ORDER
        elif p["chain"] != bytes(chain):
            filt = WRONG_CHAIN
        elif p["scid"] in failed:
            filt = TXOUT_FAILED
        elif p["scid"] in known or p["scid"] in held:
            filt = KNOWN
        if filt is not None:
            key_rows += 2
        else:
            sig_rows += 4
        if not (key_ok(p["keys"][0]) and key_ok(p["keys"][1])):
            status[i] = MALFORMED                          # fromwire_pubkey fails inside fromwire_channel_announcement: in front of everything
            continue
        scids[i] = p["scid"]
        if filt is not None:
            status[i] = filt
            continue
        if p["scid"] in pending or p["scid"] in early:     # map_get (:683-684) sees what an earlier message of the batch left
            status[i] = IN_BATCH
            continue
        bad = check(m)
        if bad:
            status[i] = 4 + bad
            continue
        if not announceable(p["scid"], blockheight):
            if blockheight != 0 and blocknum(p["scid"]) > ((blockheight + 12) & U32):
                status[i] = BAD_ORDER
                continue
            early[p["scid"]] = i
            status[i] = EARLY
        else:
            pending[p["scid"]] = i
            status[i] = PENDING
            asks.append(i)
        spk[i] = script_of(*p["keys"])
    return dict(status=status, scid=scids, spk=spk, ask_msg=asks, ask_scid=[scids[i] for i in asks], sig_rows=sig_rows, key_rows=key_rows,
                pending=pending, early=early)


def amount_msg(sat):
    return struct.pack(">HQ", 4101, sat)


def record(msg, ts=0):
    return struct.pack(">HHII", 0x2000, len(msg), sa.crc32c(ts, msg), ts) + bytes(msg)


def confirm(v, pending, replies):
    """v: node_receive_model.view() of the image as it is now; pending: [(msg, spk34)] strictly ascending by scid; replies: [(scid, sat, script)]
    -> dict(status, pend, fail_scid, add_reply, records ([the two records of an accepted reply as one bytes]), clr_rec (ascending))"""
    known = set(v["scids"])
    pmap = {}
    for k, (m, _) in enumerate(pending):
        s = frame(m)["scid"]
        assert not pmap or s > max(pmap)
        pmap[s] = k
    dying = {r for r, k in enumerate(v["nann"]) if k != NONE and v["recs"][k][1] & F_DYING}
    status, pend, fails, adds, records, clr = [], [], [], [], [], []
    for r, (scid, sat, script) in enumerate(replies):
        k = pmap.pop(scid, None)                            # map_del: gone whatever becomes of it
        pend.append(NONE if k is None else k)
        if k is None:
            status.append(NOT_PENDING)
            continue
        msg, spk = pending[k]
        if len(script) == 0:
            status.append(NO_OUTPUT)
            fails.append(scid)
            continue
        if bytes(script) != bytes(spk):
            status.append(WRONG_SCRIPT)
            fails.append(scid)
            continue
        if scid in known:
            status.append(REDUNDANT)
            continue
        status.append(ACCEPTED)
        adds.append(r)
        records.append(record(bytes(msg)) + record(amount_msg(sat)))
        known.add(scid)
        for nid in frame(msg)["ids"]:                       # node_announcements_not_dying()
            rank = v["rank"].get(nid)
            if rank is not None and rank in dying:
                dying.discard(rank)
                clr.append(v["nann"][rank])
    return dict(status=status, pend=pend, fail_scid=fails, add_reply=adds, records=records, clr_rec=sorted(clr))


def apply(blob, v, r):
    """the image after the replies: DYING cleared on clr_rec, the record pairs behind the old end"""
    out = bytearray(blob)
    for k in r["clr_rec"]:
        out[v["recs"][k][0]] &= 0xF7
    return bytes(out) + b"".join(r["records"])


# ---- builders shared by the host-build test and the device test
def checkers(orc):
    """(check, key_ok) for receive(): the C oracle's sigcheck_channel_announcement and pubkey_parse, memoised"""
    memo, keys = {}, {}

    def check(m):
        k = bytes(m)
        if k not in memo:
            memo[k] = orc.sigcheck_channel_announcement(k)
            assert memo[k] >= 0, "the model asks about well-formed messages only"
        return memo[k]

    def key_ok(k33):
        k = bytes(k33)
        if k not in keys:
            keys[k] = orc.pubkey_parse(k) is not None
        return keys[k]
    return check, key_ok


def cann(net, c, scid=None, features=b"", chain=None, ids=None, keys=None, trailing=b"", swap_keys=False):
    """a channel_announcement of net's channel c, signed by the channel's four keys whatever ids / keys the message names"""
    import gossip_stream as gs
    ch = net.chans[c]
    a, b = ch["n"]
    ids = [net.node_id[a], net.node_id[b]] if ids is None else list(ids)
    bk, bsk, nsk = list(ch["bkey"]), list(ch["bsk"]), [net.node_sk[a], net.node_sk[b]]
    if swap_keys:
        bk.reverse()
        bsk.reverse()
    if keys is not None:
        bk = list(keys)
    tail = len(features).to_bytes(2, "big") + features + (gs.CHAIN if chain is None else chain) + (ch["scid"] if scid is None else scid).to_bytes(8, "big")
    tail += ids[0] + ids[1] + bk[0] + bk[1] + trailing
    return b"\x01\x00" + b"".join(net.sign(k, tail) for k in nsk + bsk) + tail


def break_sig(m, which):
    """signature `which` (1 .. 4) of a channel_announcement no longer verifies: one bit of its s"""
    b = bytearray(m)
    b[2 + 64 * (which - 1) + 63] ^= 1
    return bytes(b)


def scid_at(block, tx=1, out=0):
    return (block << 40) | (tx << 16) | out


HEIGHT = 800_000
N_NODES, N_CHANS = 8, 24
IN_STORE, WITH_UPDATE, HELD_CHAN, FAILED_CHAN = range(5), range(3), 5, 6      # channels 0 .. 2 are digest entries, 3 and 4 bare channels
DYING_NODES, PLAIN_NODES = (0, 2), (1,)                   # nodes whose node_announcement record carries 0x0800 / lacks it; the others have none


def hand_net(orc, seed=21):
    """a gossip_stream.Net of 8 nodes and 24 channels with DISTINCT scids, all deep enough at HEIGHT; channel c joins node c % 8 and node
    (c % 8 + 1 + c // 8) % 8, so channels 7 (7, 0) and 8 (0, 2) share node 0 and channel 9 joins nodes 1 and 3"""
    import gossip_stream as gs
    net = gs.Net(orc, seed, n_nodes=N_NODES, n_chans=N_CHANS, height=HEIGHT)
    for c, ch in enumerate(net.chans):
        ch["scid"] = scid_at(HEIGHT - 100 - c, 1 + c, c & 1)
        a = c % N_NODES
        b = (a + 1 + c // N_NODES) % N_NODES
        ch["n"] = (a, b) if net.node_id[a] < net.node_id[b] else (b, a)
    return net


def hand_store(net):
    """-> the image: channels 0 .. 4 (0 .. 2 with an update each), the node_announcements of nodes 0 and 2 under a header with DYING and of node 1
    under a plain one.  Everything is signed: the image passes the audit."""
    import channel_range_model as crm
    import gossip_stream as gs
    r = []
    for c in IN_STORE:
        r += [crm.rec(net.cann(c)), crm.rec(crm.AMOUNT)]
    for c in WITH_UPDATE:
        r.append(crm.rec(net.cupd(c, c & 1, gs.NOW - 100 + c), gs.NOW - 100 + c))
    for n in DYING_NODES + PLAIN_NODES:
        r.append(crm.rec(net.nann(n, gs.NOW - 50 + n), gs.NOW - 50 + n, sa.F_COMPLETED | (F_DYING if n in DYING_NODES else 0)))
    return sa.serialise(0x10, r)


def hand_lists(net):
    """-> (held, failed): the scids the caller holds in its pending / too-early maps and in its txout failures"""
    return [net.chans[HELD_CHAN]["scid"], scid_at(1, 1, 1)], [scid_at(2, 2, 0), net.chans[FAILED_CHAN]["scid"]]


def hand_batch(net):
    """-> [(name, msg)]: every status; odd lengths, so the offsets take every residue mod 4; the names say what each one is"""
    import gossip_stream as gs
    H = HEIGHT
    mk = lambda c, **kw: cann(net, c, **kw)
    nb = N_ORDER.to_bytes(32, "big")
    ids = lambda c: [net.node_id[x] for x in net.chans[c]["n"]]
    bk = lambda c: net.chans[c]["bkey"]
    off_curve = b"\x02" + (5).to_bytes(32, "big")
    good, plain, f1, f3 = mk(10), mk(12), mk(13, features=b"\x80"), mk(11, features=b"\x01\x02\x03")
    b = [("good", good), ("its copy", good), ("432 bytes, flen 0", plain), ("431 bytes", plain[:431]), ("430 bytes", plain[:430]), ("429 bytes", plain[:429]),
         ("flen 1", f1), ("flen 1 cut to 432", f1[:432]), ("flen 3", f3), ("flen 3 cut to 429 + flen", f3[:432]), ("flen 3 cut to 430 + flen", f3[:433]),
         ("flen 3 cut to 431 + flen", f3[:434]), ("flen past the end", good[:258] + b"\xff\xff" + good[260:]), ("3 trailing bytes", mk(14, trailing=b"\x01\x02\x03")),
         ("type 257", b"\x01\x01" + good[2:]), ("empty", b""), ("one byte", b"\x01")]
    for k in range(4):
        b += [("r = n in signature %d" % (k + 1), good[:2 + 64 * k] + nb + good[34 + 64 * k:]), ("s = n in signature %d" % (k + 1), good[:34 + 64 * k] + nb + good[66 + 64 * k:])]
    b += [("bitcoin_key_2 starts 04", mk(15, keys=(bk(15)[0], b"\x04" + bk(15)[1][1:]))), ("bitcoin_key_2 off the curve", mk(15, keys=(bk(15)[0], off_curve))),
          ("bitcoin_key_1 off the curve", mk(15, keys=(off_curve, bk(15)[1]))),
          ("known scid, bitcoin_key_2 starts 04", mk(0, keys=(bk(0)[0], b"\x04" + bk(0)[1][1:]))), ("known scid, bitcoin_key_2 off the curve", mk(0, keys=(bk(0)[0], off_curve))),
          ("foreign chain, bitcoin_key_1 off the curve", mk(15, chain=gs.OTHER_CHAIN, keys=(off_curve, bk(15)[1]))),
          ("node_id_2 starts 05", mk(15, ids=(ids(15)[0], b"\x05" + ids(15)[1][1:]))), ("node_id_1 starts 01", mk(15, ids=(b"\x01" + ids(15)[0][1:], ids(15)[1]))),
          ("node_id_1 == node_id_2", mk(15, ids=(ids(15)[0], ids(15)[0]))), ("ids swapped", net.cann(15, swap_ids=True)), ("foreign chain", mk(15, chain=gs.OTHER_CHAIN)),
          ("scid failed before", mk(FAILED_CHAN)), ("scid held", mk(HELD_CHAN)), ("scid a digest entry", mk(1)), ("scid a bare channel", mk(3)),
          ("a digest entry on a foreign chain", mk(1, chain=gs.OTHER_CHAIN)), ("held and failed", mk(HELD_CHAN, scid=net.chans[FAILED_CHAN]["scid"]))]
    b += [("signature %d damaged" % k, break_sig(mk(15 + k), k)) for k in range(1, 5)]
    b += [("blocknum == blockheight - 5", mk(20, scid=scid_at(H - 5, 7))), ("blocknum == blockheight - 4", mk(20, scid=scid_at(H - 4, 7))),
          ("blocknum == blockheight + 12", mk(20, scid=scid_at(H + 12, 7))), ("blocknum == blockheight + 13", mk(20, scid=scid_at(H + 13, 7)))]
    x, y = mk(21), mk(22, scid=scid_at(H + 13, 9))
    b += [("triple: bad node_signature_2", break_sig(x, 2)), ("triple: good", x), ("triple: bad bitcoin_signature_1", break_sig(x, 3)),
          ("ahead triple: bad node_signature_2", break_sig(y, 2)), ("ahead triple: good", y), ("ahead triple: bad bitcoin_signature_1", break_sig(y, 3)),
          ("early, then its damaged copy", break_sig(mk(20, scid=scid_at(H - 4, 7)), 4)), ("a copy whose bitcoin_key_2 is off the curve", mk(21, keys=(bk(21)[0], off_curve))),
          ("keys in one order", mk(23)), ("keys in the other order", mk(23, scid=net.chans[23]["scid"] + 1, swap_keys=True))]
    return b


def check_hand_cases(batch, want, blockheight):
    """what the issue names, read off the model's result by name: the model is no rubber stamp"""
    st = {name: want["status"][i] for i, (name, _) in enumerate(batch)}
    spk = {name: want["spk"][i] for i, (name, _) in enumerate(batch)}
    ok = EARLY if blockheight == 0 else PENDING
    assert st["good"] == ok and st["its copy"] == IN_BATCH and st["432 bytes, flen 0"] == ok and st["431 bytes"] == st["430 bytes"] == st["429 bytes"] == MALFORMED
    assert st["flen 1"] == st["flen 3"] == st["3 trailing bytes"] == ok and st["flen 3 cut to 431 + flen"] == st["flen past the end"] == MALFORMED
    assert all(st["%s = n in signature %d" % (w, k)] == MALFORMED for w in "rs" for k in range(1, 5))
    assert st["bitcoin_key_2 starts 04"] == st["bitcoin_key_2 off the curve"] == st["known scid, bitcoin_key_2 starts 04"] == st["known scid, bitcoin_key_2 off the curve"] == MALFORMED
    assert st["foreign chain, bitcoin_key_1 off the curve"] == MALFORMED and st["node_id_2 starts 05"] == 6 and st["node_id_1 starts 01"] == 5
    assert st["node_id_1 == node_id_2"] == st["ids swapped"] == ID_ORDER and st["foreign chain"] == st["a digest entry on a foreign chain"] == WRONG_CHAIN
    assert st["scid failed before"] == st["held and failed"] == TXOUT_FAILED and st["scid held"] == st["scid a digest entry"] == st["scid a bare channel"] == KNOWN
    assert [st["signature %d damaged" % k] for k in range(1, 5)] == [5, 6, 7, 8]
    if blockheight:
        assert [st["blocknum == blockheight %s" % s] for s in ("- 5", "- 4", "+ 12", "+ 13")] == [PENDING, EARLY, EARLY, BAD_ORDER]
        assert [st["triple: " + s] for s in ("bad node_signature_2", "good", "bad bitcoin_signature_1")] == [6, PENDING, IN_BATCH]
        assert [st["ahead triple: " + s] for s in ("bad node_signature_2", "good", "bad bitcoin_signature_1")] == [6, BAD_ORDER, 7]
        assert st["early, then its damaged copy"] == IN_BATCH
    else:
        assert all(s in (MALFORMED, ID_ORDER, WRONG_CHAIN, TXOUT_FAILED, KNOWN, 5, 6, 7, 8, IN_BATCH, EARLY) for s in want["status"]) and not want["ask_msg"]
    assert st["a copy whose bitcoin_key_2 is off the curve"] == MALFORMED
    assert st["keys in one order"] == st["keys in the other order"] == ok and spk["keys in one order"] == spk["keys in the other order"] != bytes(34)

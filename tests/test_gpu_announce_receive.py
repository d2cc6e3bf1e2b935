"""Receiving channel_announcement batches against a store image on the device, both halves (lamd_channel_announcement_receive_batch and
lamd_channel_announcement_confirm_batch, include/lightning_amd.h) against the sequential model of announce_receive_model.py: every status, scid,
script byte, list entry and output byte, with no tolerance.  The signatures are real (gossip_stream.Net signs with the oracle's signer; the
mainnet excerpt carries its own); the device checks them itself.  The same code on the host, under the sanitizers and with the verdicts handed
in, is test_store_announce_host's."""
import ctypes
import os
import random
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import announce_receive_model as arm  # noqa: E402
import gossip_stream as gs  # noqa: E402
import node_receive_model as nrm  # noqa: E402
import test_store_audit as sa  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -3
H = arm.HEIGHT


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def hand(orc):
    net = arm.hand_net(orc)
    return net, arm.hand_store(net), arm.hand_batch(net)


class Resident:
    """the digest and the directory of an image, and the model's view of it"""

    def __init__(self, eng, blob, verdict=None):
        self.eng, self.blob, self.v = eng, blob, nrm.view(blob, verdict)
        self.dg = eng.gossip_store_digest(blob, verdict=verdict)
        self.dr = eng.gossip_store_directory(self.dg, blob, verdict=verdict, chain_hash=gs.CHAIN)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.dr.free()
        self.dg.close()


def receive_equals_model(orc, res, msgs, height, held=(), failed=()):
    """one device call against the model -> (the model's result, the summary)"""
    check, key_ok = arm.checkers(orc)
    want = arm.receive(res.v["scids"], msgs, gs.CHAIN, height, check, key_ok, held, failed)
    status, scid, spk, asks, s = res.eng.channel_announcement_receive(res.dg, msgs, gs.CHAIN, height, held=held, failed=failed, return_summary=True)
    got = dict(status=[int(x) for x in status], scid=[int(x) for x in scid], spk=[bytes(x) for x in spk], ask_msg=[int(x) for x in asks["msg"]],
               ask_scid=[int(x) for x in asks["scid"]])
    for k in got:
        assert got[k] == want[k], (k, len(got[k]), len(want[k]), [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6])
    st = want["status"]
    assert s["by_status"] == [st.count(k) for k in range(12)] + [st.count(-1)] and s["asks"] == len(want["ask_msg"])
    assert (s["signature_rows"], s["keyparse_rows"]) == (want["sig_rows"], want["key_rows"])
    return want, s


def confirm_equals_model(res, pending, replies, **kw):
    want = arm.confirm(res.v, pending, replies)
    status, pend, fails, plan, s = res.eng.channel_announcement_confirm(res.dg, res.dr, [m for m, _ in pending], np.array([list(k) for _, k in pending], dtype=np.uint8),
                                                                        replies, return_summary=True, **kw)
    got = dict(status=[int(x) for x in status], pend=[int(x) for x in pend], fail_scid=[int(x) for x in fails], add_reply=[int(x) for x in plan["add_reply"]],
               clr_rec=[int(x) for x in plan["clr_rec"]])
    for k in got:
        assert got[k] == want[k], (k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6])
    if plan["records"] is not None:
        assert plan["records"] == b"".join(want["records"])
    offs, at = [], 0
    for r, j in zip(want["records"], want["add_reply"]):
        offs += [at, at + 12 + len(pending[want["pend"][j]][0])]
        at += len(r)
    assert [int(x) for x in plan["add_off"]] == offs and all(plan[k].size == 0 for k in ("del_rec", "set_rec", "set_ts", "set_crc"))
    st = want["status"]
    assert s["by_status"] == [st.count(k) for k in range(5)] and (s["adds"], s["bytes"], s["failures"], s["clears"]) == (st.count(0), at, len(want["fail_scid"]), len(want["clr_rec"]))
    return want, plan


# ------------------------------------------------------------------------------------------------ A. the named cases
def test_every_status_against_the_model(eng, orc, hand):
    """lengths around 432 + flen, flen 0 / 1 / 3 / past the end, trailing bytes, r = n and s = n in every signature, bitcoin keys that do not parse in
    front of every filter, node ids that are no keys, the id order, the chain, failed / held / entry / bare scids, each signature damaged, the
    block heights on both sides of every comparison, copies in front of and behind the first good one; blockheight unknown: everything good is early"""
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    held, failed = arm.hand_lists(net)
    with Resident(eng, blob) as res:
        for height in (H, 0):
            want, _ = receive_equals_model(orc, res, msgs, height, held, failed)
            arm.check_hand_cases(batch, want, height)
        receive_equals_model(orc, res, [], H)
        receive_equals_model(orc, res, [b"", b"\x01\x00", bytes(500), b"\x01\x00" + bytes(430)], H)
        receive_equals_model(orc, res, msgs, 0xFFFFFFF8)                                         # blockheight + 12 wraps as the reference's does
    with Resident(eng, b"\x10") as none:                                                        # no channel at all
        want, _ = receive_equals_model(orc, none, msgs, H)
        assert 4 not in want["status"]


# ------------------------------------------------------------------------------------------------ B. shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_wave(eng, orc, hand, n):
    net, blob, batch = hand
    rnd = random.Random(n)
    held, failed = arm.hand_lists(net)
    with Resident(eng, blob) as res:
        receive_equals_model(orc, res, [rnd.choice(batch)[1] for _ in range(n)], H, held, failed)


def test_five_thousand_copies_and_a_batch_of_known_channels(eng, orc, hand):
    net, blob, batch = hand
    with Resident(eng, blob) as res:
        want, s = receive_equals_model(orc, res, [batch[0][1]] * 5000, H)
        assert want["status"] == [0] + [10] * 4999 and s["signature_rows"] == 20000
        rnd = random.Random(7)
        mixed = [rnd.choice(batch[:3] + batch[42:56])[1] for _ in range(5000)]                   # a few scids, good and damaged copies interleaved
        receive_equals_model(orc, res, mixed, H)
        known = [net.cann(c) for c in arm.IN_STORE] * 40
        want, s = receive_equals_model(orc, res, known, H)
        assert set(want["status"]) == {4} and s["signature_rows"] == 0 and s["keyparse_rows"] == 2 * len(known)


def raw_receive(eng, dg, msgs, height, ask_cap):
    from lightning_amd import _ffi
    n = len(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(gs.CHAIN, dtype=np.uint8)
    a = dict(status=np.full(n, 77, dtype=np.int8), scid=np.full(n, 77, dtype=np.uint64), spk=np.full(34 * n, 77, dtype=np.uint8), ask_msg=np.full(n, 77, dtype=np.uint32),
             ask_scid=np.full(n, 77, dtype=np.uint64))
    s = _ffi.LamdAnnounceReceiveSummary()
    p = lambda k: a[k].ctypes.data
    rc = eng._lib.lamd_channel_announcement_receive_batch(eng._ctx, dg._h, chain.ctypes.data, height, n, blob.ctypes.data, off.ctypes.data, 0, None, 0, None, p("status"),
                                                          p("scid"), p("spk"), ask_cap, p("ask_msg"), p("ask_scid"), ctypes.byref(s))
    return rc, a, s


def test_receive_caps(eng, orc, hand):
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    check, key_ok = arm.checkers(orc)
    with Resident(eng, blob) as res:
        want = arm.receive(res.v["scids"], msgs, gs.CHAIN, H, check, key_ok)
        asks = len(want["ask_msg"])
        assert asks > 2
        verdicts = lambda a: [int(x) for x in a["status"]] == want["status"] and [int(x) for x in a["scid"]] == want["scid"] and bytes(a["spk"]) == b"".join(want["spk"])
        for cap in (0, asks - 1):
            rc, a, s = raw_receive(eng, res.dg, msgs, H, cap)
            assert rc == ERR_ARG and s.asks == asks and verdicts(a) and (a["ask_msg"] == 77).all() and (a["ask_scid"] == 77).all(), cap
        rc, a, s = raw_receive(eng, res.dg, msgs, H, asks)
        assert rc == 0 and verdicts(a) and [int(x) for x in a["ask_msg"][:asks]] == want["ask_msg"] and (a["ask_msg"][asks:] == 77).all()
        assert [int(x) for x in a["ask_scid"][:asks]] == want["ask_scid"] and (a["ask_scid"][asks:] == 77).all()
        from lightning_amd import Engine
        with Engine(0) as other:
            rc, a, _ = raw_receive(other, res.dg, msgs, H, len(msgs))
            assert rc == ERR_ARG and (a["status"] == 77).all()


# ------------------------------------------------------------------------------------------------ C. confirm
def pending_of(net, orc, res, chans, height=H):
    """the pending list a receive of these channels' announcements leaves: [(msg, spk)] ascending by scid"""
    check, key_ok = arm.checkers(orc)
    msgs = [net.cann(c) for c in chans]
    want = arm.receive(res.v["scids"], msgs, gs.CHAIN, height, check, key_ok)
    assert want["status"] == [0] * len(msgs)
    return [(msgs[i], want["spk"][i]) for _, i in sorted(want["pending"].items())]


def test_every_reply_status_and_the_dying_bits(eng, orc, hand):
    """an unknown scid, an empty script, scripts of 33 / 34 / 35 bytes that differ in the last byte, a scid that meanwhile sits in the digest, the same
    scid twice (good then spent, spent then good), sat 0 and 2^64 - 1; node 0's dying announcement is named once although channels 7 and 8 share the
    node, node 2's once, node 1's (no bit) and node 3's (no record) never"""
    net, blob, _ = hand
    with Resident(eng, blob) as res:
        pending = pending_of(net, orc, res, [7, 8, 9, 10, 11, 12, 13, 14])
        known = (net.cann(1, features=b"\x05"), arm.script_of(*net.chans[1]["bkey"]))            # pending, and meanwhile in the digest
        pending = sorted(pending + [known], key=lambda p: arm.frame(p[0])["scid"])
        spk = {arm.frame(m)["scid"]: k for m, k in pending}
        sc = lambda c: net.chans[c]["scid"]
        replies = [(arm.scid_at(5, 5, 5), 1000, spk[sc(7)]), (sc(7), 0, spk[sc(7)]), (sc(8), 0xFFFFFFFFFFFFFFFF, spk[sc(8)]), (sc(9), 77, spk[sc(9)]),
                   (sc(10), 5, b""), (sc(11), 5, spk[sc(11)][:33]), (sc(12), 5, spk[sc(12)][:33] + bytes([spk[sc(12)][33] ^ 1])), (sc(13), 5, spk[sc(13)] + b"\x00"),
                   (sc(1), 5, spk[sc(1)]), (sc(14), 9, spk[sc(14)]), (sc(14), 9, b""), (sc(10), 5, spk[sc(10)]), (sc(7), 1, spk[sc(7)])]
        want, plan = confirm_equals_model(res, pending, replies)
        assert want["status"] == [1, 0, 0, 0, 2, 3, 3, 3, 4, 0, 1, 1, 1] and want["fail_scid"] == [sc(10), sc(11), sc(12), sc(13)]
        rank = lambda n: res.v["rank"][net.node_id[n]]
        assert want["clr_rec"] == sorted(res.v["nann"][rank(n)] for n in arm.DYING_NODES) and res.v["nann"][rank(1)] != nrm.NONE and res.v["nann"][rank(3)] == nrm.NONE
        confirm_equals_model(res, pending, [])
        confirm_equals_model(res, [], replies[:4])
        confirm_equals_model(res, pending, list(reversed(replies)))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pending_lists_around_a_wave(eng, orc, hand, n):
    net, blob, _ = hand
    rnd = random.Random(n)
    with Resident(eng, blob) as res:
        pending = []
        for k in range(n):                                                                       # confirm checks no signature: any scid will do
            m = arm.cann(net, k % arm.N_CHANS, scid=arm.scid_at(H - 2000 + k, k, 1), features=bytes(k % 5))
            pending.append((m, arm.script_of(*arm.frame(m)["keys"])))
        replies = []
        for m, k in pending:
            roll = rnd.random()
            replies.append((arm.frame(m)["scid"], rnd.randrange(1 << 40), k if roll < 0.7 else b"" if roll < 0.8 else k[:-1] + b"\x00"))
        rnd.shuffle(replies)
        replies += replies[:3] + [(1, 1, b"")]
        confirm_equals_model(res, pending, replies)


def raw_confirm(eng, res, pending, replies, add_cap, out_cap, fail_cap, clr_cap, host_out=True, d_ptr=None, order=None):
    from lightning_amd import _ffi
    msgs = [m for m, _ in pending]
    np_, nr = len(msgs), len(replies)
    off = np.zeros(np_ + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)
    pspk = np.frombuffer(b"".join(k for _, k in pending) + b"\x00", dtype=np.uint8)
    r_scid, r_sat = np.array([r[0] for r in replies] + [0], dtype=np.uint64), np.array([r[1] for r in replies] + [0], dtype=np.uint64)
    soff = np.zeros(nr + 1, dtype=np.uint64)
    soff[1:] = np.cumsum([len(r[2]) for r in replies], dtype=np.uint64)
    scripts = np.frombuffer(b"".join(r[2] for r in replies) + b"\x00", dtype=np.uint8)
    a = dict(status=np.full(nr, 77, dtype=np.int8), pend=np.full(nr, 77, dtype=np.uint32), add_reply=np.full(nr, 77, dtype=np.uint32), add_off=np.full(nr, 77, dtype=np.uint64),
             out=np.full(int(off[np_]) + 34 * nr, 77, dtype=np.uint8), fail=np.full(nr, 77, dtype=np.uint64), clr=np.full(2 * nr, 77, dtype=np.uint32))
    s = _ffi.LamdAnnounceConfirmSummary()
    p = lambda k: a[k].ctypes.data
    rc = eng._lib.lamd_channel_announcement_confirm_batch(eng._ctx, res.dg._h, res.dr._h, np_, blob.ctypes.data, off.ctypes.data, pspk.ctypes.data, nr, r_scid.ctypes.data,
                                                          r_sat.ctypes.data, scripts.ctypes.data, soff.ctypes.data, p("status"), p("pend"), add_cap, p("add_reply"), p("add_off"),
                                                          p("out") if host_out else None, d_ptr, out_cap, fail_cap, p("fail"), clr_cap, p("clr"), ctypes.byref(s))
    return rc, a, s


def test_confirm_caps_alignments_and_a_list_that_does_not_ascend(eng, orc, hand):
    import torch
    net, blob, _ = hand
    with Resident(eng, blob) as res:
        pending = pending_of(net, orc, res, [7, 8, 9, 10, 11])
        replies = [(arm.frame(m)["scid"], 1000 + k, spk if k != 3 else b"\x00") for k, (m, spk) in enumerate(pending)]
        want = arm.confirm(res.v, pending, replies)
        adds, total, fails, clrs = len(want["add_reply"]), sum(len(r) for r in want["records"]), len(want["fail_scid"]), len(want["clr_rec"])
        assert adds == 4 and fails == 1 and clrs == 2
        untouched = lambda a: all((a[k] == 77).all() for k in ("add_reply", "add_off", "out", "fail", "clr"))
        verdicts = lambda a: [int(x) for x in a["status"]] == want["status"] and [int(x) for x in a["pend"]] == want["pend"]
        sizes = lambda s: (s.adds, s.bytes, s.failures, s.clears) == (adds, total, fails, clrs)
        rc, a, s = raw_confirm(eng, res, pending, replies, 0, 0, 0, 0, host_out=False)           # the sizes alone
        assert rc == ERR_ARG and sizes(s) and untouched(a) and verdicts(a)
        for caps in ((adds - 1, total, fails, clrs), (adds, total - 1, fails, clrs), (adds, total, fails - 1, clrs), (adds, total, fails, clrs - 1)):
            rc, a, s = raw_confirm(eng, res, pending, replies, *caps)
            assert rc == ERR_ARG and sizes(s) and untouched(a) and verdicts(a), caps
        rc, a, s = raw_confirm(eng, res, pending, replies, adds, total, fails, clrs)             # exactly enough
        assert rc == 0 and bytes(a["out"][:total]) == b"".join(want["records"]) and (a["out"][total:] == 77).all() and verdicts(a)
        assert [int(x) for x in a["clr"][:clrs]] == want["clr_rec"] and (a["clr"][clrs:] == 77).all() and [int(x) for x in a["fail"][:fails]] == want["fail_scid"]
        rc, a, s = raw_confirm(eng, res, pending, replies, adds, 0, fails, clrs, host_out=False)  # the lists without the bytes
        assert rc == 0 and [int(x) for x in a["add_reply"][:adds]] == want["add_reply"] and (a["out"] == 77).all()
        for mis in range(4):                                                                     # the bytes on the device, at every alignment, nothing around them
            buf = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            torch.cuda.synchronize()
            rc, a, s = raw_confirm(eng, res, pending, replies, adds, total, fails, clrs, host_out=mis == 3, d_ptr=buf.data_ptr() + mis)
            got = buf.cpu().numpy()
            assert rc == 0 and bytes(got[mis:mis + total]) == b"".join(want["records"]) and (got[:mis] == 0xEE).all() and (got[mis + total:] == 0xEE).all()
            assert mis != 3 or bytes(a["out"][:total]) == b"".join(want["records"])
        for bad in ([pending[1], pending[0]] + pending[2:], [pending[0], pending[0]], pending[:1] + [(b"\x01\x00" + bytes(100), bytes(34))]):
            rc, a, _ = raw_confirm(eng, res, bad, replies, 9, 10 ** 5, 9, 9)
            assert rc == ERR_ARG and (a["status"] == 77).all() and untouched(a)


# ------------------------------------------------------------------------------------------------ the loop closes
def test_the_applied_plan_audits_clean_and_a_second_receive_knows_the_channels(eng, orc, hand):
    from lightning_amd.engine import apply_update_plan, gossip_store_frame
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    held, failed = arm.hand_lists(net)
    with Resident(eng, blob) as res:
        want, _ = receive_equals_model(orc, res, msgs, H, held, failed)
        pending = [(msgs[i], want["spk"][i]) for _, i in sorted(want["pending"].items())]
        replies = [(s, 1000 + k, want["spk"][i]) for k, (s, i) in enumerate(zip(want["ask_scid"], want["ask_msg"]))]
        cwant, plan = confirm_equals_model(res, pending, replies)
        assert cwant["status"] == [0] * len(replies) and len(replies) > 5
        image, rec_off = apply_update_plan(blob, gossip_store_frame(blob)[0], plan)
    assert image == arm.apply(blob, res.v, cwant)
    off, verdict, s = eng.gossip_store_audit(image)[:3]
    assert s["clean"] == 1 and [int(x) for x in off] == [int(x) for x in rec_off]                # 1. the applied plan audits clean
    with Resident(eng, image, list(verdict)) as res2:
        new = set(want["ask_scid"])
        assert new <= {int(x) for x in res2.dg.read_bare()} and not new & set(res.v["scids"])    # 2. the new channels are bare channels
        ids = set(res2.v["ids"])
        assert all(nid in ids for m, _ in pending for nid in arm.frame(m)["ids"])                # 3. the directory ranks their nodes
        id33 = res2.dr.nodes()[0]
        assert [bytes(x) for x in id33] == res2.v["ids"]
        again, _ = receive_equals_model(orc, res2, msgs, H, held, failed)                        # 4. what was pending is known now
        assert all(b == 4 for a, b in zip(want["status"], again["status"]) if a == 0) and 0 not in again["status"]
        assert [b for a, b in zip(want["status"], again["status"]) if a in (-1, 1, 2, 3, 4)] == [a for a in want["status"] if a in (-1, 1, 2, 3, 4)]
        for r in cwant["clr_rec"]:
            assert not res2.v["recs"][r][1] & arm.F_DYING and res.v["recs"][r][1] & arm.F_DYING


# ------------------------------------------------------------------------------------------------ the pinned input nobody here authored
def test_the_mainnet_excerpt_is_received_and_confirmed_into_its_own_records(eng, orc):
    """the channel_announcements of the reference's mainnet excerpt (four real signatures each) against an empty image at a blockheight beyond them:
    all pending; confirmed with the model's scripts and the store's own amounts, the appended pairs carry the message bytes of the store's own pairs"""
    blob = sa._golden("gossip_store_mainnet_part1.bin") + sa._golden("gossip_store_mainnet_part2.bin")
    recs, at = [], 1
    while at + 12 <= len(blob):
        ln = struct.unpack(">H", blob[at + 2:at + 4])[0]
        recs.append(blob[at + 12:at + 12 + ln])
        at += 12 + ln
    pairs = [(recs[k], recs[k + 1]) for k in range(len(recs) - 1) if recs[k][:2] == b"\x01\x00" and recs[k + 1][:2] == b"\x10\x05"]
    assert len(pairs) == 88
    msgs = [m for m, _ in pairs]
    height = max(arm.blocknum(arm.frame(m)["scid"]) for m in msgs) + 6
    with Resident(eng, b"\x10") as res:
        want, s = receive_equals_model(orc, res, msgs, height)
        assert want["status"] == [0] * 88 and s["signature_rows"] == 4 * 88
        order = sorted(range(88), key=lambda i: want["scid"][i])
        pending = [(msgs[i], want["spk"][i]) for i in order]
        replies = [(want["scid"][i], int.from_bytes(pairs[i][1][2:10], "big"), want["spk"][i]) for i in range(88)]
        cwant, plan = confirm_equals_model(res, pending, replies)
        assert cwant["status"] == [0] * 88
        out, at = plan["records"], 0
        for m, amount in pairs:
            for part in (m, amount):
                flags, ln, crc, ts = struct.unpack(">HHII", out[at:at + 12])
                assert (flags, ln, ts) == (0x2000, len(part), 0) and out[at + 12:at + 12 + ln] == part and crc == sa.crc32c(0, part)
                at += 12 + ln
        assert at == len(out)

"""lightning_amd/csrc/store_announce.h on the host, under AddressSanitizer and UBSan (tests/c/store_announce_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the reception of channel_announcement batches against a store image and of
lightningd's txout replies, on which the header and the sequential model of announce_receive_model must agree exactly -- status, scid, every
script byte, which list a message is put on, every list entry and every output byte -- for a hand-built batch that meets every status, its
orders of arrival, copies of one announcement, and hand-built replies; the messages, rows, sorted positions and replies visited in arrival
order, in reverse and in a scrambled order, the output written at all four alignments (the program compares those itself).  The signature and
key-parse verdicts are an input computed by the oracle: the stages on both sides of the two batches are what is under test here; the device
side, batches included, is test_gpu_announce_receive's.  Two further tests: the confirm plan applied to the image of a live GossipIngest equals
the image that ingest holds after the same announcements and txout replies; and the new prototypes of include/lightning_amd.h agree with their
ctypes bindings."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import announce_receive_model as arm  # noqa: E402
import gossip_stream as gs  # noqa: E402
import node_receive_model as nrm  # noqa: E402
import test_store_audit as sa  # noqa: E402

ROOT = sa.ROOT
H = arm.HEIGHT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_announce") / "store_announce_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_announce_host.cpp")])
    return path


@pytest.fixture(scope="module")
def hand(orc):
    net = arm.hand_net(orc)
    return net, arm.hand_store(net), arm.hand_batch(net)


def _run(exe, args, d):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    return lambda name, dt: [int(x) for x in np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)]


def host_receive(exe, d, v, msgs, height, held, failed, verdicts):
    """-> dict of what the host build of the header computes.  verdicts: (signature verdict, key 1 parses, key 2 parses) per message"""
    d.mkdir()
    count = v["entries"]
    (d / "digest").write_bytes(struct.pack("<II", count, len(v["scids"]) - count) + np.array(v["scids"], dtype="<u8").tobytes())
    batch = struct.pack("<IIII", height, len(msgs), len(held), len(failed)) + gs.CHAIN + np.array(sorted(held), dtype="<u8").tobytes()
    batch += np.array(sorted(failed), dtype="<u8").tobytes() + b"".join(struct.pack("<I", len(m)) + bytes(m) for m in msgs)
    (d / "batch").write_bytes(batch)
    (d / "verdicts").write_bytes(b"".join(struct.pack("<bBB", *x) for x in verdicts))
    arr = _run(exe, ["receive", d / "digest", d / "batch", d / "verdicts", d / "out"], d)
    spk = (d / "out.spk").read_bytes()
    counts = arr("counts", "<u4")
    return dict(status=arr("status", np.int8), scid=arr("scid", "<u8"), spk=[spk[34 * i:34 * i + 34] for i in range(len(msgs))], ask_msg=arr("askmsg", "<u4"),
                ask_scid=arr("askscid", "<u8"), list=arr("list", np.uint8), sig_rows=4 * counts[0], key_rows=2 * counts[1])


def receive_against_model(exe, d, orc, v, msgs, height, held=(), failed=()):
    check, key_ok = arm.checkers(orc)
    want = arm.receive(v["scids"], msgs, gs.CHAIN, height, check, key_ok, held, failed)
    verdicts = []
    for m in msgs:
        p = arm.frame(m)
        # what the two batches say about a message; about one the header must not ask, a verdict that would show
        verdicts.append((3, 0, 0) if p is None else (orc.sigcheck_channel_announcement(bytes(m)), int(key_ok(p["keys"][0])), int(key_ok(p["keys"][1]))))
    got = host_receive(exe, d, v, msgs, height, held, failed, verdicts)
    for k in ("status", "scid", "spk", "ask_msg", "ask_scid", "sig_rows", "key_rows"):
        assert got[k] == want[k], (k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6] if isinstance(got[k], list) else (got[k], want[k]))
    assert all((ls == 0) == (arm.frame(m) is None) for ls, m in zip(got["list"], msgs))
    return want


def host_confirm(exe, d, blob, v, pending, replies):
    d.mkdir()
    (d / "image").write_bytes(blob)
    count = v["entries"]
    view = struct.pack("<IIII", len(v["recs"]), count, len(v["scids"]) - count, len(v["ids"])) + np.array([r[0] for r in v["recs"]], dtype="<u8").tobytes()
    view += np.array(v["scids"], dtype="<u8").tobytes() + np.array(v["node_off"], dtype="<u8").tobytes()
    view += np.array([0 if k == nrm.NONE else k + 1 for k in v["nann"]], dtype="<u4").tobytes()
    (d / "view").write_bytes(view)
    (d / "pending").write_bytes(struct.pack("<I", len(pending)) + b"".join(struct.pack("<I", len(m)) + bytes(m) + bytes(k) for m, k in pending))
    (d / "replies").write_bytes(struct.pack("<I", len(replies)) + b"".join(struct.pack("<QQI", s, sat, len(sc)) + bytes(sc) for s, sat, sc in replies))
    arr = _run(exe, ["confirm", d / "image", d / "view", d / "pending", d / "replies", d / "out"], d)
    return dict(status=arr("status", np.int8), pend=arr("pend", "<u4"), fail_scid=arr("fail", "<u8"), add_reply=arr("addreply", "<u4"), add_off=arr("addoff", "<u8"),
                clr_rec=arr("clr", "<u4"), bytes=(d / "out.bytes").read_bytes())


def confirm_against_model(exe, d, blob, v, pending, replies):
    want = arm.confirm(v, pending, replies)
    got = host_confirm(exe, d, blob, v, pending, replies)
    for k in ("status", "pend", "fail_scid", "add_reply", "clr_rec"):
        assert got[k] == want[k], (k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6])
    assert got["bytes"] == b"".join(want["records"])
    offs, at = [], 0
    for r in want["records"]:
        offs.append(at)
        at += len(r)
    assert got["add_off"] == offs
    return want, got


# ------------------------------------------------------------------------------------------------ the first half
def test_every_status_by_hand(exe, tmp_path, orc, hand):
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    assert len({len(m) % 4 for m in msgs}) == 4
    v = nrm.view(blob)
    held, failed = arm.hand_lists(net)
    for height in (H, 0):
        want = receive_against_model(exe, tmp_path / ("hand%d" % height), orc, v, msgs, height, held, failed)
        arm.check_hand_cases(batch, want, height)
    assert sorted(set(want["status"])) == [-1, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11]
    receive_against_model(exe, tmp_path / "wrap", orc, v, msgs, 0xFFFFFFF8)                        # blockheight + 12 wraps as the reference's does
    receive_against_model(exe, tmp_path / "low", orc, v, msgs, 3)                                 # everything is far ahead: bad gossip order
    receive_against_model(exe, tmp_path / "none", orc, v, [], H)
    receive_against_model(exe, tmp_path / "junk", orc, v, [b"", b"\x01\x00", bytes(500), b"\x01\x00" + bytes(430)], H)
    empty = receive_against_model(exe, tmp_path / "empty", orc, nrm.view(b"\x10"), msgs, H)      # an image without a channel
    assert 4 not in empty["status"]
    # the oracle calls malformed what the model calls malformed, for everything long enough to be framed
    check, key_ok = arm.checkers(orc)
    for m in msgs:
        p = arm.frame(m)
        if len(m) >= 260 and m[:2] == b"\x01\x00":
            assert (orc.sigcheck_channel_announcement(m) == -1) == (p is None or not (key_ok(p["keys"][0]) and key_ok(p["keys"][1]))), m.hex()


def test_orders_of_arrival_and_many_copies(exe, tmp_path, orc, hand):
    """the same messages reversed and shuffled and doubled: other winners, the same agreement; 600 copies of one announcement: one pending, the rest
    already pending -- whichever copy comes first"""
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    v = nrm.view(blob)
    held, failed = arm.hand_lists(net)
    seen = set()
    for k, order in enumerate((list(range(len(msgs)))[::-1], random.Random(4).sample(range(len(msgs)), len(msgs)), random.Random(5).sample(range(len(msgs)), len(msgs)))):
        want = receive_against_model(exe, tmp_path / ("o%d" % k), orc, v, [msgs[i] for i in order] * 2, H, held, failed)
        assert want["status"][len(msgs):].count(0) == 0                                          # the second copy of anything is at best already pending
        seen.add(tuple(want["status"]))
    assert len(seen) == 3
    good = msgs[0]
    want = receive_against_model(exe, tmp_path / "copies", orc, v, [good] * 600, H)
    assert want["status"] == [0] + [10] * 599
    rnd = random.Random(8)
    bad1, bad4 = arm.break_sig(good, 1), arm.break_sig(good, 4)
    want = receive_against_model(exe, tmp_path / "mixed", orc, v, [bad4, bad1, bad4] + [rnd.choice([good, bad1, bad4]) for _ in range(600)], H)
    assert want["status"][:3] == [8, 5, 8] and want["status"].count(0) == 1 and set(want["status"]) == {0, 5, 8, 10}
    known = [net.cann(c) for c in arm.IN_STORE] * 8
    want = receive_against_model(exe, tmp_path / "known", orc, v, known, H)
    assert set(want["status"]) == {4} and want["sig_rows"] == 0


# ------------------------------------------------------------------------------------------------ the second half
def pending_of(net, orc, v, chans):
    check, key_ok = arm.checkers(orc)
    msgs = [net.cann(c) for c in chans]
    want = arm.receive(v["scids"], msgs, gs.CHAIN, H, check, key_ok)
    assert want["status"] == [0] * len(msgs)
    return [(msgs[i], want["spk"][i]) for _, i in sorted(want["pending"].items())]


def test_every_reply_status_and_the_dying_bits(exe, tmp_path, orc, hand):
    net, blob, _ = hand
    v = nrm.view(blob)
    pending = pending_of(net, orc, v, [7, 8, 9, 10, 11, 12, 13, 14])
    known = (net.cann(1, features=b"\x05"), arm.script_of(*net.chans[1]["bkey"]))                # pending, and meanwhile in the digest
    bare = (net.cann(3, features=b"\x05\x06"), arm.script_of(*net.chans[3]["bkey"]))             # ... and meanwhile a bare channel
    pending = sorted(pending + [known, bare], key=lambda p: arm.frame(p[0])["scid"])
    spk = {arm.frame(m)["scid"]: k for m, k in pending}
    sc = lambda c: net.chans[c]["scid"]
    replies = [(arm.scid_at(5, 5, 5), 1000, spk[sc(7)]), (sc(7), 0, spk[sc(7)]), (sc(8), 0xFFFFFFFFFFFFFFFF, spk[sc(8)]), (sc(9), 77, spk[sc(9)]),
               (sc(10), 5, b""), (sc(11), 5, spk[sc(11)][:33]), (sc(12), 5, spk[sc(12)][:33] + bytes([spk[sc(12)][33] ^ 1])), (sc(13), 5, spk[sc(13)] + b"\x00"),
               (sc(1), 5, spk[sc(1)]), (sc(3), 5, spk[sc(3)]), (sc(14), 9, spk[sc(14)]), (sc(14), 9, b""), (sc(10), 5, spk[sc(10)]), (sc(7), 1, spk[sc(7)])]
    want, _ = confirm_against_model(exe, tmp_path / "replies", blob, v, pending, replies)
    assert want["status"] == [1, 0, 0, 0, 2, 3, 3, 3, 4, 4, 0, 1, 1, 1] and want["fail_scid"] == [sc(10), sc(11), sc(12), sc(13)]
    rank = lambda n: v["rank"][net.node_id[n]]
    assert want["clr_rec"] == sorted(v["nann"][rank(n)] for n in arm.DYING_NODES) and v["nann"][rank(1)] != nrm.NONE and v["nann"][rank(3)] == nrm.NONE
    back, _ = confirm_against_model(exe, tmp_path / "reversed", blob, v, pending, list(reversed(replies)))
    assert back["status"][:4] == [0, 0, 2, 1]                                                    # now sat 1 wins channel 7, channel 10 is good and channel 14 is spent
    confirm_against_model(exe, tmp_path / "noreply", blob, v, pending, [])
    confirm_against_model(exe, tmp_path / "nopending", blob, v, [], replies[:4])
    confirm_against_model(exe, tmp_path / "empty", b"\x10", nrm.view(b"\x10"), pending, replies)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pending_lists_around_a_wave(exe, tmp_path, orc, hand, n):
    net, blob, _ = hand
    v = nrm.view(blob)
    rnd = random.Random(n)
    pending = []
    for k in range(n):
        m = arm.cann(net, k % arm.N_CHANS, scid=arm.scid_at(H - 2000 + k, k, 1), features=bytes(k % 5))
        pending.append((m, arm.script_of(*arm.frame(m)["keys"])))
    replies = []
    for m, k in pending:
        roll = rnd.random()
        replies.append((arm.frame(m)["scid"], rnd.randrange(1 << 40), k if roll < 0.7 else b"" if roll < 0.8 else k[:-1] + b"\x00"))
    rnd.shuffle(replies)
    replies += replies[:3] + [(1, 1, b"")]
    confirm_against_model(exe, tmp_path / "c", blob, v, pending, replies)


# ------------------------------------------------------------------------------------------------ the loop closes on the CPU
def test_the_plan_applied_equals_the_ingests_own_store(exe, tmp_path, orc, hand):
    """a GossipIngest on the CPU back end gets a batch of announcements only; its GET_TXOUT events are the header's ask list; they are answered with
    txout_reply_batch; its store_image() afterwards is its image before with the header's confirm plan applied, byte for byte -- and with the
    model's.  The store has no dying node: the host ingest never clears DYING on a node's announcement when a new channel appears."""
    from lightning_amd.gossipd import GossipIngest
    net = hand[0]
    old, ops = gs.make_script(orc, 21, n_ops=300)
    with GossipIngest(None, gs.CHAIN, old.our_id, old.height + 200, gs.NOW, backend=sa.oracle_backend(orc)) as ing:
        gs.drive(old, ops, ing, 21)
        ing.new_block(H + 400)
        ing.process()
        before = ing.store_image()
        v = nrm.view(before)
        assert len(v["scids"]) >= 5 and not any(r[1] & arm.F_DYING for r in v["recs"]) and not set(v["scids"]) & {ch["scid"] for ch in net.chans}
        good = [net.cann(c) for c in range(arm.N_CHANS)]
        batch = good + good[:5] + [arm.break_sig(good[7], 2), net.cann(3, swap_ids=True), net.cann(4, chain=gs.OTHER_CHAIN), good[9][:400]]
        batch += [old.cann(c) for c in range(len(old.chans)) if old.chans[c]["scid"] in v["scids"]][:4]
        random.Random(3).shuffle(batch)
        seen = len(ing.events)
        for m in batch:
            ing.push(old.peers[1], m)
        ing.process()
        asked = [e[1] for e in ing.events[seen:] if e[0] == "GET_TXOUT"]
        want = receive_against_model(exe, tmp_path / "rx", orc, v, batch, H + 400)
        assert want["ask_scid"] == asked and len(asked) == arm.N_CHANS and {-1, 1, 2, 4, 6, 10} <= set(want["status"])
        pending = [(batch[i], want["spk"][i]) for _, i in sorted(want["pending"].items())]
        rnd = random.Random(5)
        order = rnd.sample(range(len(asked)), len(asked))
        replies = [(asked[k], 10_000 + k, b"" if j == 2 else bytes(34) if j == 5 else want["spk"][want["ask_msg"][k]]) for j, k in enumerate(order)]
        replies += [replies[0], (arm.scid_at(9, 9, 9), 5, replies[0][2])]
        soff = np.zeros(len(replies) + 1, dtype=np.uint64)
        soff[1:] = np.cumsum([len(r[2]) for r in replies], dtype=np.uint64)
        ing.txout_reply_batch(np.array([r[0] for r in replies], dtype=np.uint64), np.array([r[1] for r in replies], dtype=np.uint64),
                              np.frombuffer(b"".join(r[2] for r in replies) + b"\x00", dtype=np.uint8), soff)
        after = ing.store_image()
    cwant, got = confirm_against_model(exe, tmp_path / "cf", before, v, pending, replies)
    assert cwant["status"].count(0) == arm.N_CHANS - 2 and cwant["status"].count(1) == 2 and not got["clr_rec"]
    assert after == before + got["bytes"] and after == arm.apply(before, v, cwant)


def test_apply_update_plan_clears_the_dying_bits(hand):
    """apply_update_plan() honours an optional clr_rec and behaves as before without the key"""
    from lightning_amd.engine import apply_update_plan, gossip_store_frame
    net, blob, _ = hand
    v = nrm.view(blob)
    off = gossip_store_frame(blob)[0]
    none = np.zeros(0, dtype=np.uint32)
    plan = dict(add_msg=none, add_off=np.zeros(0, dtype=np.uint64), records=b"", del_rec=none, set_rec=none, set_ts=none, set_crc=none)
    assert apply_update_plan(blob, off, plan)[0] == blob
    dying = [k for k in v["nann"] if k != nrm.NONE and v["recs"][k][1] & arm.F_DYING]
    assert len(dying) == 2
    image, _ = apply_update_plan(blob, off, dict(plan, clr_rec=np.array(dying, dtype=np.uint32)))
    assert image == arm.apply(blob, v, dict(clr_rec=dying, records=[])) != blob


def test_new_prototypes_and_bindings_agree(tmp_path):
    """the prototypes this header section adds have the argument counts of their ctypes bindings, and the summaries the layout a C compiler gives them"""
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    lines = []
    want = []
    for n, count, cname, cls in (("lamd_channel_announcement_receive_batch", 18, "lamd_announce_receive_summary", _ffi.LamdAnnounceReceiveSummary),
                                 ("lamd_channel_announcement_confirm_batch", 25, "lamd_announce_confirm_summary", _ffi.LamdAnnounceConfirmSummary)):
        proto = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
        assert proto, n
        res, args = _ffi.SYMBOLS[n]
        assert len(proto.group(2).split(",")) == len(args) == count and res is ctypes.c_int and proto.group(1) == "int"
        for text, ct in zip(proto.group(2).split(","), args):
            assert (("size_t" in text or "uint64_t" in text) and "*" not in text) == (ct in (ctypes.c_size_t, ctypes.c_uint64)), text   # (one type on LP64)
            assert ("uint32_t" in text and "*" not in text) == (ct is ctypes.c_uint32), text
        lines += ['  printf("%%zu\\n", sizeof(%s));\n' % cname] + ['  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_]
        want += [ctypes.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
        assert hasattr(_ffi.load(), n)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()] == want

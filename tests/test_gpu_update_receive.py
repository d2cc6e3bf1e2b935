"""Receiving channel_update batches against a store image on the device (lamd_channel_update_receive_batch, include/lightning_amd.h) against the
sequential model of update_receive_model.py: every status, flag, channel number, list entry and output byte, with no tolerance.  The signatures
of the batches are real (gossip_stream.Net signs with the oracle's signer); the device checks them itself.  The same code on the host, under
the sanitizers and with the signature verdicts handed in, is test_store_receive_host's."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import gossip_stream as gs  # noqa: E402
import test_store_audit as sa  # noqa: E402
import update_receive_model as urm  # noqa: E402
from test_store_audit import synthetic  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = -3


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def hand(orc):
    net = urm.hand_net(orc)
    return net, urm.hand_store(net, crm.CHAIN), urm.hand_batch(net, crm.CHAIN, gs.OTHER_CHAIN)


class Resident:
    """the digest and the directory of an image, and the model's view of it"""

    def __init__(self, eng, blob, verdict=None, chain=crm.CHAIN):
        self.eng, self.blob, self.v = eng, blob, urm.view(blob, verdict)
        self.dg = eng.gossip_store_digest(blob, verdict=verdict)
        self.dr = eng.gossip_store_directory(self.dg, blob, verdict=verdict, chain_hash=chain)

    def close(self):
        self.dr.free()
        self.dg.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def equals_model(orc, res, msgs, chain=crm.CHAIN, now=urm.NOW, **kw):
    """one device call against the model -> (the model's result, the plan, the summary)"""
    want = urm.receive(res.v, msgs, chain, now, urm.checker(orc), kw.get("prune_interval", 0), kw.get("our_id"),
                       [kw["peers"]] * len(msgs) if isinstance(kw.get("peers"), bytes) else kw.get("peers"), kw.get("held", ()))
    status, flags, chan, plan, s = res.eng.channel_update_receive(res.dg, res.dr, msgs, chain, now, return_summary=True, **kw)
    got = dict(status=[int(x) for x in status], flags=[int(x) for x in flags], chan=[int(x) for x in chan], add_msg=[int(x) for x in plan["add_msg"]],
               del_rec=[int(x) for x in plan["del_rec"]], sets=list(zip(*([int(x) for x in plan[k]] for k in ("set_rec", "set_ts", "set_crc")))))
    for k in got:
        assert got[k] == want[k], (k, len(got[k]), len(want[k]), got[k][:6], want[k][:6])
    assert plan["records"] == b"".join(want["records"])
    offs, at = [], 0
    for r in want["records"]:
        offs.append(at)
        at += len(r)
    assert [int(x) for x in plan["add_off"]] == offs
    st = want["status"]
    assert s["by_status"] == [st.count(k) for k in range(10)] + [st.count(-1)]
    assert (s["accepted"], s["adds"], s["bytes"], s["deletions"], s["retimestamps"]) == (st.count(0), st.count(0), at, len(want["del_rec"]), len(want["sets"]))
    assert s["superseded"] == sum(1 for f in want["flags"] if f & 1) and s["signature_rows"] == sum(1 for x in want["signer"] if x is not None)
    return want, plan, s


# ------------------------------------------------------------------------------------------------ 1. the hand-built cases
def test_every_status_and_flag(eng, orc, hand):
    """a flipped signature bit, r >= n, DONT_FORWARD, equal timestamps, a peer-signed unknown channel, a held scid, and the rest of the table"""
    net, blob, (msgs, peers, held, ours) = hand
    with Resident(eng, blob) as res:
        want, _, _ = equals_model(orc, res, msgs, our_id=ours, peers=peers, held=held)
        assert sorted(set(want["status"])) == list(range(-1, 10)) and all(any(f & bit for f in want["flags"]) for bit in (1, 2, 4, 8))
        plain, _, _ = equals_model(orc, res, msgs)
        assert [plain["status"][i] for i in (14, 16, 18)] == [0, 5, 5]
        equals_model(orc, res, msgs, peers=net.node_id[1], our_id=ours)                          # one peer for all: stride 0
        mixed, _, _ = equals_model(orc, res, msgs, peers=[None if i % 3 == 0 else net.node_id[1] for i in range(len(msgs))])
        assert (mixed["status"][16], mixed["status"][18]) == (4, 5)
        early, _, _ = equals_model(orc, res, msgs, now=1000, prune_interval=2000)
        assert set(early["status"]) == {-1, 1, 2}
        equals_model(orc, res, [])
        equals_model(orc, res, [b"", b"\x01\x02", bytes(200)])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_wave(eng, orc, hand, n):
    net, blob, (msgs, peers, held, ours) = hand
    rnd = random.Random(n)
    batch = [rnd.choice(msgs) for _ in range(n)]
    with Resident(eng, blob) as res:
        equals_model(orc, res, batch, our_id=ours, peers=[peers[0]] * n, held=held)


def test_the_synthetic_store(eng, orc, synthetic):
    img, (_, ver, _) = synthetic
    net = gs.Net(orc, sa.SEED)                                                                  # the network that signed it (make_script's)
    rnd = random.Random(12)
    for verdict in (None, list(ver)):
        with Resident(eng, img, verdict) as res:
            batch = []
            for c in range(len(net.chans)):
                for d in (0, 1):
                    k = res.v["chan"].get(net.chans[c]["scid"])
                    base = res.v["ts"][k][d] if k is not None and res.v["rec"][k][1 + d] != urm.NONE else gs.NOW
                    batch += [net.cupd(c, d, base + x) for x in (-1, 0, 1, 1, 3)]
            rnd.shuffle(batch)
            want, _, _ = equals_model(orc, res, batch, chain=gs.CHAIN, now=gs.NOW + 500, our_id=net.our_id, peers=net.peers[1])
            assert {0, 8, 9} <= set(want["status"]) and want["del_rec"] and any(f & 1 for f in want["flags"])


# ------------------------------------------------------------------------------------------------ 2. many messages
def test_five_thousand_messages_on_one_slot_and_spread_over_all(eng, orc, hand):
    """some 40 to 50 distinct signed updates repeated in shuffled order: the sort and the scan cross their block boundaries, whether the whole batch is
    aimed at ONE slot or spread over every channel"""
    net, blob, _ = hand
    rnd = random.Random(5000)
    one = [net.cupd(0, 0, urm.T0 - 5 + k, chain=crm.CHAIN, extra=bytes(k % 7)) for k in range(40)]
    spread = [net.cupd(c, d, urm.T0 - 1 + k, chain=crm.CHAIN, extra=bytes((c + k) % 5)) for c in range(9) for d in (0, 1) for k in (0, 7, 12)]
    with Resident(eng, blob) as res:
        for ups in (one, spread):
            batch = [rnd.choice(ups) for _ in range(5000)]
            want, _, s = equals_model(orc, res, batch, peers=net.node_id[1])
            assert s["signature_rows"] == 5000 and want["status"].count(0) >= 2 and want["status"].count(8) + want["status"].count(9) > 4000
        assert set(want["chan"]) == set(range(8)) | {urm.NONE}


# ------------------------------------------------------------------------------------------------ 3. the raw call: sizes, caps, alignments, mismatches
def raw(eng, res, msgs, add_cap, out_cap, edit_cap, host_out=True, d_ptr=None, dg=None):
    lib, n = eng._lib, len(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(crm.CHAIN, dtype=np.uint8)
    a = dict(status=np.full(n, 77, dtype=np.int8), flags=np.full(n, 77, dtype=np.uint8), chan=np.full(n, 77, dtype=np.uint32), add_msg=np.full(n, 77, dtype=np.uint32),
             add_off=np.full(n, 77, dtype=np.uint64), out=np.full(int(off[n]) + 12 * n, 77, dtype=np.uint8), del_rec=np.full(n, 77, dtype=np.uint32),
             set_rec=np.full(n, 77, dtype=np.uint32), set_ts=np.full(n, 77, dtype=np.uint32), set_crc=np.full(n, 77, dtype=np.uint32))
    from lightning_amd import _ffi
    s = _ffi.LamdUpdateReceiveSummary()
    p = lambda k: a[k].ctypes.data
    rc = lib.lamd_channel_update_receive_batch(eng._ctx, (dg or res.dg)._h, res.dr._h, chain.ctypes.data, urm.NOW, 0, None, n, blob.ctypes.data, off.ctypes.data, None, 0, 0, None,
                                               p("status"), p("flags"), p("chan"), add_cap, p("add_msg"), p("add_off"), p("out") if host_out else None, d_ptr, out_cap,
                                               edit_cap, p("del_rec"), p("set_rec"), p("set_ts"), p("set_crc"), ctypes.byref(s))
    return rc, a, s


def test_sizes_alone_caps_one_short_and_output_alignments(eng, orc, hand):
    import torch
    net, blob, (msgs, _, _, _) = hand
    with Resident(eng, blob) as res:
        want = urm.receive(res.v, msgs, crm.CHAIN, urm.NOW, urm.checker(orc))
        adds, total, dels, sets = len(want["add_msg"]), sum(len(r) for r in want["records"]), len(want["del_rec"]), len(want["sets"])
        assert adds > sets > 0 and dels > sets                                                  # so that each list can be the one that does not fit
        untouched = lambda a: all((a[k] == 77).all() for k in ("add_msg", "add_off", "out", "del_rec", "set_rec", "set_ts", "set_crc"))
        rc, a, s = raw(eng, res, msgs, 0, 0, 0, host_out=False)                                  # the sizes alone
        assert rc == ERR_ARG and (s.adds, s.bytes, s.deletions, s.retimestamps) == (adds, total, dels, sets) and untouched(a)
        assert [int(x) for x in a["status"]] == want["status"] and [int(x) for x in a["flags"]] == want["flags"] and [int(x) for x in a["chan"]] == want["chan"]
        for caps in ((adds - 1, total, dels), (adds, total - 1, dels), (adds, total, dels - 1)):
            rc, a, s = raw(eng, res, msgs, *caps)
            assert rc == ERR_ARG and s.adds == adds and untouched(a) and [int(x) for x in a["status"]] == want["status"], caps
        only_sets = [m for i, m in enumerate(msgs) if want["flags"][i] & 2]                     # re-stamps and no deletion: the other edit list one short
        rc, a, s = raw(eng, res, only_sets, len(only_sets), 10 ** 6, len(only_sets) - 1)
        assert rc == ERR_ARG and (s.retimestamps, s.deletions) == (len(only_sets), 0) and untouched(a)
        rc, a, s = raw(eng, res, msgs, adds, total, dels)                                        # exactly enough
        assert rc == 0 and bytes(a["out"][:total]) == b"".join(want["records"]) and (a["out"][total:] == 77).all()
        assert [int(x) for x in a["del_rec"][:dels]] == want["del_rec"] and (a["del_rec"][dels:] == 77).all() and (a["add_msg"][adds:] == 77).all()
        rc, a, s = raw(eng, res, msgs, adds, 0, dels, host_out=False)                            # the lists without the bytes
        assert rc == 0 and [int(x) for x in a["add_msg"][:adds]] == want["add_msg"] and (a["out"] == 77).all()
        for mis in range(4):                                                                     # the bytes on the device, at every alignment, nothing around them
            buf = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            torch.cuda.synchronize()
            rc, a, s = raw(eng, res, msgs, adds, total, dels, host_out=mis == 3, d_ptr=buf.data_ptr() + mis)
            got = buf.cpu().numpy()
            assert rc == 0 and bytes(got[mis:mis + total]) == b"".join(want["records"]) and (got[:mis] == 0xEE).all() and (got[mis + total:] == 0xEE).all()
            assert mis != 3 or bytes(a["out"][:total]) == b"".join(want["records"])


def test_a_digest_of_another_image_is_refused(eng, orc, hand):
    net, blob, (msgs, _, _, _) = hand
    other = sa.serialise(0x10, sa.parse(blob)[:-3])
    with Resident(eng, blob) as res, Resident(eng, other) as res2:
        rc, a, _ = raw(eng, res, msgs, len(msgs), 10 ** 6, len(msgs), dg=res2.dg)
        assert rc == ERR_ARG and (a["status"] == 77).all()
        assert raw(eng, res, msgs, len(msgs), 10 ** 6, len(msgs))[0] == 0


# ------------------------------------------------------------------------------------------------ 4. the loop closes
def test_the_applied_plan_audits_clean_and_a_second_receive_finds_nothing_new(eng, orc, hand):
    from lightning_amd.engine import apply_update_plan, gossip_store_frame
    net, blob, (msgs, peers, held, ours) = hand
    with Resident(eng, blob) as res:
        want, plan, _ = equals_model(orc, res, msgs, our_id=ours, peers=peers, held=held)
        image, rec_off = apply_update_plan(blob, gossip_store_frame(blob)[0], plan)
    assert image == urm.apply(blob, res.v, want)
    off, verdict, s = eng.gossip_store_audit(image)[:3]
    assert s["clean"] == 1 and [int(x) for x in off] == [int(x) for x in rec_off] and s["skipped_deleted"] == len(want["del_rec"]) + 1 + sum(1 for f in want["flags"] if f & 1)
    with Resident(eng, image, list(verdict)) as res2:
        renumbered = {c: res2.v["chan"][res.v["scids"][c]] for c, _ in want["final"]}         # bare channels that got an update are entries now
        assert {(c, d): res2.v["ts"][renumbered[c]][d] for (c, d) in want["final"]} == want["final"]
        scid, ts, _, _ = res2.dg.read()
        by_scid = {int(s_): [int(x) for x in t] for s_, t in zip(scid, ts)}
        for (c, d), t in want["final"].items():
            assert by_scid[res.v["scids"][c]][d] == t
        again, plan2, _ = equals_model(orc, res2, msgs, our_id=ours, peers=peers, held=held)
        assert all(b in (8, 9) for a, b in zip(want["status"], again["status"]) if a == 0) and not plan2["records"]
        assert [b for a, b in zip(want["status"], again["status"]) if a != 0 and a < 8] == [a for a in want["status"] if a != 0 and a < 8]

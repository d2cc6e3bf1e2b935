"""Receiving node_announcement batches against a store image on the device (lamd_node_announcement_receive_batch, include/lightning_amd.h) against
the sequential model of node_receive_model.py: every status, flag, node rank, list entry and output byte, with no tolerance.  The signatures of
the batches are real (gossip_stream.Net signs with the oracle's signer); the device checks them itself.  The same code on the host, under the
sanitizers and with the signature verdicts handed in, is test_store_nodes_host's."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import node_receive_model as nrm  # noqa: E402
from test_store_nodes_host import check_hand_cases  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -3


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def hand(orc):
    net = nrm.hand_net(orc)
    return net, nrm.hand_store(net, crm.CHAIN, twins=True), nrm.hand_store(net, crm.CHAIN), nrm.hand_batch(net)


class Resident:
    """the directory of an image (and the digest it is built from), and the model's view of it"""

    def __init__(self, eng, blob, verdict=None):
        self.eng, self.blob, self.v = eng, blob, nrm.view(blob, verdict)
        self.dg = eng.gossip_store_digest(blob, verdict=verdict)
        self.dr = eng.gossip_store_directory(self.dg, blob, verdict=verdict, chain_hash=crm.CHAIN)

    def close(self):
        self.dr.free()
        self.dg.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def equals_model(orc, res, msgs, pending=False):
    """one device call against the model -> (the model's result, the plan, the summary)"""
    want = nrm.receive(res.v, msgs, nrm.checker(orc), pending)
    status, flags, node, plan, s = res.eng.node_announcement_receive(res.dr, msgs, pending=pending, return_summary=True)
    got = dict(status=[int(x) for x in status], flags=[int(x) for x in flags], node=[int(x) for x in node], add_msg=[int(x) for x in plan["add_msg"]],
               del_rec=[int(x) for x in plan["del_rec"]])
    for k in got:
        assert got[k] == want[k], (k, len(got[k]), len(want[k]), [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6])
    assert plan["records"] == b"".join(want["records"]) and all(plan[k].size == 0 and plan[k].dtype == np.uint32 for k in ("set_rec", "set_ts", "set_crc"))
    offs, at = [], 0
    for r in want["records"]:
        offs.append(at)
        at += len(r)
    assert [int(x) for x in plan["add_off"]] == offs
    st = want["status"]
    assert s["by_status"] == [st.count(k) for k in range(7)] + [st.count(-1)]
    assert (s["accepted"], s["adds"], s["bytes"], s["deletions"]) == (st.count(0), st.count(0), at, len(want["del_rec"]))
    assert s["superseded"] == sum(1 for f in want["flags"] if f & 1) and s["signature_rows"] == sum(want["checked"])
    return want, plan, s


# ------------------------------------------------------------------------------------------------ 1. the hand-built cases
def test_every_status_and_flag(eng, orc, hand):
    """lengths 141 and 142, flen 0 and 5, every address type whole and cut, the TLV tail's rules, r = n and s = n, an id that is no key, ids that share
    32 bytes, the other parity, timestamps 0 and 2^32 - 1 with and without a record, dying and live nodes, nothing pending and something pending"""
    net, blob, _, batch = hand
    msgs = [m for _, m in batch]
    with Resident(eng, blob) as res:
        for pending in (False, True):
            want, _, _ = equals_model(orc, res, msgs, pending)
            check_hand_cases(net, res.v, batch, want, pending)
        equals_model(orc, res, [])
        equals_model(orc, res, [b"", b"\x01\x01", bytes(200), b"\x01\x01" + bytes(140)])
    with Resident(eng, b"\x10") as none:                                                        # no channel, no node
        want, _, _ = equals_model(orc, none, msgs[:8], True)
        assert set(want["status"]) == {-1, 3}


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_wave(eng, orc, hand, n):
    net, blob, _, batch = hand
    rnd = random.Random(n)
    with Resident(eng, blob) as res:
        equals_model(orc, res, [rnd.choice(batch)[1] for _ in range(n)], bool(n & 1))


# ------------------------------------------------------------------------------------------------ 2. many messages
def test_five_thousand_messages_on_one_node_and_spread_over_all(eng, orc, hand):
    """some 40 to 50 distinct signed announcements repeated in shuffled order: the sort and the scan cross their block boundaries, whether the whole batch
    is aimed at ONE node or spread over every node"""
    net, blob, _, _ = hand
    rnd = random.Random(5000)
    one = [net.nann(0, nrm.T0 - 5 + k, addrs=bytes(k % 7)) for k in range(40)]
    spread = [net.nann(n, nrm.T0 - 1 + k, addrs=bytes((n + k) % 5)) for n in range(9) for k in (0, 2, 7, 8, 12)]
    with Resident(eng, blob) as res:
        for anns in (one, spread):
            batch = [rnd.choice(anns) for _ in range(5000)]
            want, _, s = equals_model(orc, res, batch)
            assert s["signature_rows"] == 5000 and want["status"].count(0) >= 2 and want["status"].count(5) + want["status"].count(6) > 4000
        assert set(want["node"]) == {res.v["rank"][net.node_id[n]] for n in range(8)} | {nrm.NONE}


# ------------------------------------------------------------------------------------------------ 3. the raw call: sizes, caps, alignments, mismatches
def raw(eng, dr, msgs, add_cap, out_cap, edit_cap, host_out=True, d_ptr=None):
    lib, n = eng._lib, len(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)
    a = dict(status=np.full(n, 77, dtype=np.int8), flags=np.full(n, 77, dtype=np.uint8), node=np.full(n, 77, dtype=np.uint32), add_msg=np.full(n, 77, dtype=np.uint32),
             add_off=np.full(n, 77, dtype=np.uint64), out=np.full(int(off[n]) + 12 * n, 77, dtype=np.uint8), del_rec=np.full(n, 77, dtype=np.uint32))
    from lightning_amd import _ffi
    s = _ffi.LamdNodeReceiveSummary()
    p = lambda k: a[k].ctypes.data
    rc = lib.lamd_node_announcement_receive_batch(eng._ctx, dr._h, n, blob.ctypes.data, off.ctypes.data, 0, p("status"), p("flags"), p("node"), add_cap, p("add_msg"),
                                                  p("add_off"), p("out") if host_out else None, d_ptr, out_cap, edit_cap, p("del_rec"), ctypes.byref(s))
    return rc, a, s


def test_sizes_alone_caps_one_short_and_output_alignments(eng, orc, hand):
    import torch
    net, blob, _, batch = hand
    msgs = [m for _, m in batch]
    with Resident(eng, blob) as res:
        want = nrm.receive(res.v, msgs, nrm.checker(orc))
        adds, total, dels = len(want["add_msg"]), sum(len(r) for r in want["records"]), len(want["del_rec"])
        assert adds > dels > 0
        untouched = lambda a: all((a[k] == 77).all() for k in ("add_msg", "add_off", "out", "del_rec"))
        verdicts = lambda a: all([int(x) for x in a[k]] == want[k] for k in ("status", "flags", "node"))
        rc, a, s = raw(eng, res.dr, msgs, 0, 0, 0, host_out=False)                               # the sizes alone
        assert rc == ERR_ARG and (s.adds, s.bytes, s.deletions) == (adds, total, dels) and untouched(a) and verdicts(a)
        for caps in ((adds - 1, total, dels), (adds, total - 1, dels), (adds, total, dels - 1)):
            rc, a, s = raw(eng, res.dr, msgs, *caps)
            assert rc == ERR_ARG and (s.adds, s.bytes, s.deletions) == (adds, total, dels) and untouched(a) and verdicts(a), caps
        rc, a, s = raw(eng, res.dr, msgs, adds, total, dels)                                     # exactly enough
        assert rc == 0 and bytes(a["out"][:total]) == b"".join(want["records"]) and (a["out"][total:] == 77).all()
        assert [int(x) for x in a["del_rec"][:dels]] == want["del_rec"] and (a["del_rec"][dels:] == 77).all() and (a["add_msg"][adds:] == 77).all()
        rc, a, s = raw(eng, res.dr, msgs, adds, 0, dels, host_out=False)                         # the lists without the bytes
        assert rc == 0 and [int(x) for x in a["add_msg"][:adds]] == want["add_msg"] and (a["out"] == 77).all()
        for mis in range(4):                                                                     # the bytes on the device, at every alignment, nothing around them
            buf = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            torch.cuda.synchronize()
            rc, a, s = raw(eng, res.dr, msgs, adds, total, dels, host_out=mis == 3, d_ptr=buf.data_ptr() + mis)
            got = buf.cpu().numpy()
            assert rc == 0 and bytes(got[mis:mis + total]) == b"".join(want["records"]) and (got[:mis] == 0xEE).all() and (got[mis + total:] == 0xEE).all()
            assert mis != 3 or bytes(a["out"][:total]) == b"".join(want["records"])


def test_a_directory_of_another_context_is_refused(eng, orc, hand):
    from lightning_amd import Engine
    net, blob, _, batch = hand
    msgs = [m for _, m in batch]
    with Resident(eng, blob) as res, Engine(0) as other:
        rc, a, _ = raw(other, res.dr, msgs, len(msgs), 10 ** 6, len(msgs))
        assert rc == ERR_ARG and (a["status"] == 77).all() and (a["out"] == 77).all()
        assert raw(eng, res.dr, msgs, len(msgs), 10 ** 6, len(msgs))[0] == 0


# ------------------------------------------------------------------------------------------------ 4. the loop closes
def test_the_applied_plan_audits_clean_and_a_second_receive_finds_nothing_new(eng, orc, hand):
    from lightning_amd.engine import apply_update_plan, gossip_store_frame
    net, _, blob, batch = hand                                                                   # the store without the unsigned twins: it audits clean
    msgs = [m for _, m in batch]
    with Resident(eng, blob) as res:
        want, plan, _ = equals_model(orc, res, msgs)
        image, rec_off = apply_update_plan(blob, gossip_store_frame(blob)[0], plan)
        n_before = len(res.v["recs"])
    assert image == nrm.apply(blob, res.v, want) and want["final"]
    off, verdict, s = eng.gossip_store_audit(image)[:3]
    assert s["clean"] == 1 and [int(x) for x in off] == [int(x) for x in rec_off] and s["skipped_deleted"] == len(want["del_rec"]) + 1 + sum(1 for f in want["flags"] if f & 1)
    with Resident(eng, image, list(verdict)) as res2:
        assert res2.v["ids"] == res.v["ids"]
        _, _, nann_rec = res2.dr.nodes()
        for r in range(len(res.v["ids"])):                                                       # each node's record in force is the model's final one
            final = want["final"].get(r)
            expect = res.v["nann"][r] if final is None else n_before + want["add_msg"].index(final[1])
            assert int(nann_rec[r]) == res2.v["nann"][r] == expect
            if final is not None:
                assert res2.v["ts"][r] == final[0] and res2.v["recs"][expect][4] == msgs[final[1]]
        again, plan2, _ = equals_model(orc, res2, msgs)
        assert all(b in (5, 6) for a, b in zip(want["status"], again["status"]) if a == 0) and not plan2["records"] and not len(plan2["del_rec"])
        assert [b for a, b in zip(want["status"], again["status"]) if a not in (0, 5, 6)] == [a for a in want["status"] if a not in (0, 5, 6)]

"""Parity tests proper: the HIP path (through the C ABI) against the golden vectors and the CPU
oracle on the same inputs.  Bit-exact accept/reject is the bar.  Needs an MI355X: -m gpu."""
import os
import random

import numpy as np
import pytest
import torch

import pyref
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu
H = bytes.fromhex
N = pyref.N


def _cores():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per) + 0.5)))
    except Exception:
        pass
    return n


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _rows(rows, w):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), w)


def test_native_library_is_what_runs(eng):
    inf = eng.info()
    assert inf["arch"].startswith("gfx950") and inf["gtable_bytes"] in (11 * (64 << 24), 11 * (72 << 24))   # 11 windows of 2^24 entries (8-word / 9-limb coordinates)
    import ctypes
    from lightning_amd import _build
    assert ctypes.CDLL(_build.LIB)  # the in-tree .so is loaded


def test_golden_ecdsa(eng, kat):
    for publen in (33, 65):
        vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 2 * publen]
        got = eng.verify_ecdsa(_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64),
                               _rows([H(v["pub"]) for v in vs], publen))
        bad = [v["name"] for v, g in zip(vs, got) if bool(g) != v["expect"]]
        assert not bad, bad[:10]


def test_golden_schnorr(eng, kat):
    vs = kat["schnorr"]
    got = eng.verify_schnorr(_rows([H(v["msg"]) for v in vs], 32), _rows([H(v["pk"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64))
    bad = [v["name"] for v, g in zip(vs, got) if bool(g) != v["expect"]]
    assert not bad, bad[:10]


def test_golden_gossip(eng, kat):
    vs = kat["gossip"]
    got = eng.sigcheck_gossip([H(v["msg"]) for v in vs], [H(v["node_id"]) if "node_id" in v else None for v in vs])
    bad = [(v["name"], int(g), v["expect"]) for v, g in zip(vs, got) if int(g) != v["expect"]]
    assert not bad, bad[:10]
    # the two verdicts the reference's own unit test asserts (run-check_channel_announcement.c:84-85,107-108)
    by = {v["name"]: int(g) for v, g in zip(vs, got)}
    assert by["KAT-G/orig"] == 1 and by["KAT-G/features-stripped"] == 2


def test_golden_pubkey_parse(eng, kat):
    for ln in (33, 65):
        vs = [v for v in kat["pubkey"] if len(v["pub"]) == 2 * ln]
        out, ok = eng.pubkey_parse(_rows([H(v["pub"]) for v in vs], ln))
        for v, o, k in zip(vs, out, ok):
            assert bool(k) == (v["expect"] is not None), v["pub"]
            if k:
                assert o.tobytes() == H(v["expect"])


def test_single_item_veneers(eng, kat):
    v = next(x for x in kat["ecdsa"] if x["name"] == "KAT-B11")
    assert eng.check_signed_hash_nodeid(H(v["hash"]), H(v["sig"]), H(v["pub"])) is True
    assert eng.check_signed_hash(H(v["hash"]), H(v["sig"]), H(v["pub"])) is True
    v = next(x for x in kat["ecdsa"] if x["name"] == "KAT-O/fee=165749")
    assert eng.check_signed_hash(H(v["hash"]), H(v["sig"]), H(v["pub"])) is False
    s = next(x for x in kat["schnorr"] if x["name"] == "BIP340/1")
    # check_schnorr_sig takes the full (compressed) key and drops the parity byte (bitcoin/signature.c:417-423)
    assert eng.check_schnorr_sig(H(s["msg"]), b"\x02" + H(s["pk"]), H(s["sig"])) is True
    assert eng.check_schnorr_sig(H(s["msg"]), b"\x03" + H(s["pk"]), H(s["sig"])) is True
    s = next(x for x in kat["schnorr"] if x["name"] == "BIP340/6")
    assert eng.check_schnorr_sig(H(s["msg"]), b"\x02" + H(s["pk"]), H(s["sig"])) is False


def _random_ecdsa(orc, rnd, n, publen):
    hs, sg, pk = [], [], []
    for i in range(n):
        d = rnd.randrange(1, N).to_bytes(32, "big")
        h = rnd.randbytes(32)
        s = orc.ecdsa_sign(h, d, rnd.randrange(1, N).to_bytes(32, "big"))
        p = orc.pubkey_create(d)
        if publen == 33:
            p = bytes([2 + (p[64] & 1)]) + p[1:33]
        c = rnd.randrange(10)
        if c == 0:
            h = bytes([h[0] ^ 1]) + h[1:]
        elif c == 1:
            j = rnd.randrange(64)
            s = s[:j] + bytes([s[j] ^ (1 << rnd.randrange(8))]) + s[j + 1:]
        elif c == 2:
            s = s[:32] + (N - int.from_bytes(s[32:], "big")).to_bytes(32, "big")
        elif c == 3:
            j = 1 + rnd.randrange(publen - 1)
            p = p[:j] + bytes([p[j] ^ (1 << rnd.randrange(8))]) + p[j + 1:]
        hs.append(h); sg.append(s); pk.append(p)
    return _rows(hs, 32), _rows(sg, 64), _rows(pk, publen)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1000, 5000])
def test_random_ecdsa_vs_oracle_ragged_sizes(eng, orc, n):
    rnd = random.Random(1000 + n)
    for publen in (33, 65):
        hs, sg, pk = _random_ecdsa(orc, rnd, n, publen)
        got = eng.verify_ecdsa(hs, sg, pk)
        exp = orc.ecdsa_verify_batch(hs, sg, pk, publen, 4).astype(bool)
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
        assert n < 50 or (exp.sum() > n // 2 and (~exp).sum() > 0)


def _random_schnorr(orc, rnd, n):
    """n BIP-340 rows, about three in eight damaged -> (msg [n,32], x-only key [n,32], sig [n,64], the oracle's verdicts)"""
    ms, ks, sg = [], [], []
    for i in range(n):
        d = rnd.randrange(1, N).to_bytes(32, "big")
        m = rnd.randbytes(32)
        s = orc.schnorr_sign(m, d, rnd.randbytes(32))
        k = orc.pubkey_create(d)[1:33]
        c = rnd.randrange(8)
        if c == 0:
            m = bytes([m[5] ^ 4]) + m[1:]
        elif c == 1:
            j = rnd.randrange(64)
            s = s[:j] + bytes([s[j] ^ (1 << rnd.randrange(8))]) + s[j + 1:]
        elif c == 2:
            j = rnd.randrange(32)
            k = k[:j] + bytes([k[j] ^ (1 << rnd.randrange(8))]) + k[j + 1:]
        ms.append(m); ks.append(k); sg.append(s)
    ms, ks, sg = _rows(ms, 32), _rows(ks, 32), _rows(sg, 64)
    return ms, ks, sg, orc.schnorr_verify_batch(ms, ks, sg, 4).astype(bool)


@pytest.mark.parametrize("n", [1, 64, 65, 700, 3000])
def test_random_schnorr_vs_oracle(eng, orc, n):
    ms, ks, sg, exp = _random_schnorr(orc, random.Random(2000 + n), n)
    got = eng.verify_schnorr(ms, ks, sg)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]


def test_empty_batch(eng):
    z = np.zeros((0, 32), np.uint8)
    assert eng.verify_ecdsa(z, np.zeros((0, 64), np.uint8), np.zeros((0, 33), np.uint8)).shape == (0,)
    assert eng.verify_schnorr(z, z, np.zeros((0, 64), np.uint8)).shape == (0,)


def test_streaming_queue_mixed_kinds_in_ticket_order(eng, orc, kat):
    rnd = random.Random(77)
    items = []
    es = [v for v in kat["ecdsa"]]
    ss = [v for v in kat["schnorr"]]
    for i in range(600):
        if rnd.random() < 0.3:
            v = rnd.choice(ss)
            items.append(("s", v))
        else:
            items.append(("e", rnd.choice(es)))
    tickets = []
    for kind, v in items:
        if kind == "e":
            tickets.append(eng.queue_ecdsa(H(v["hash"]), H(v["sig"]), H(v["pub"])))
        else:
            tickets.append(eng.queue_schnorr(H(v["msg"]), H(v["pk"]), H(v["sig"])))
    assert tickets == list(range(len(items)))      # a ticket is the position in the flush's verdict vector
    eng.flush()
    got = eng.wait()
    assert [bool(g) for g in got] == [v["expect"] for _, v in items]
    # second round re-uses the rings
    t = eng.queue_ecdsa(H(es[0]["hash"]), H(es[0]["sig"]), H(es[0]["pub"]))
    eng.flush()
    got = eng.wait()
    assert len(got) == 1 and bool(got[0]) == es[0]["expect"] and t == 0      # tickets restart with every flush


def test_device_generator_round_trip_and_oracle_sample(eng, orc):
    """sign on the GPU -> every row verifies on the GPU; a sample is re-verified by the CPU oracle;
    corrupted rows are rejected (size-independent properties used at full scale by bench.py)"""
    import torch
    from lightning_amd import workload
    for publen in (65, 33):
        w = workload.make_ecdsa(eng, 20000, nkeys=257, publen=publen)
        eng.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
        eng.synchronize()
        got = strict_bool(w.d_ok.cpu().numpy())
        assert np.array_equal(got, w.expect), (publen, np.nonzero(got != w.expect)[0][:10], w.classes[got != w.expect][:10])
        assert (~w.expect).sum() == 2000
        sl = slice(0, 1500)
        exp = orc.ecdsa_verify_batch(np.ascontiguousarray(w.cols[0][sl]), np.ascontiguousarray(w.cols[1][sl]),
                                     np.ascontiguousarray(w.cols[2][sl]), publen, 4).astype(bool)
        assert np.array_equal(got[sl], exp)
    w = workload.make_schnorr(eng, 20000, nkeys=300)
    eng.verify_schnorr_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.synchronize()
    got = strict_bool(w.d_ok.cpu().numpy())
    assert np.array_equal(got, w.expect), (np.nonzero(got != w.expect)[0][:10], w.classes[got != w.expect][:10])
    sl = slice(0, 1500)
    exp = orc.schnorr_verify_batch(np.ascontiguousarray(w.cols[0][sl]), np.ascontiguousarray(w.cols[1][sl]),
                                   np.ascontiguousarray(w.cols[2][sl]), 4).astype(bool)
    assert np.array_equal(got[sl], exp)


def test_repeated_keys_and_identical_rows(eng, kat):
    """483 HTLC signatures of one commitment share a key (channeld/channeld.c:2215-2232): same-key batches"""
    v = next(x for x in kat["ecdsa"] if x["name"] == "KAT-O/fee=165750")
    n = 484
    hs = _rows([H(v["hash"])] * n, 32).copy()
    sg = _rows([H(v["sig"])] * n, 64)
    pk = _rows([H(v["pub"])] * n, 33)
    hs[1::2, 7] ^= 1
    got = eng.verify_ecdsa(hs, sg, pk)
    assert got[0::2].all() and not got[1::2].any()


def test_cfg4_gossip_replay_small_vs_oracle_and_construction(eng, orc):
    """BASELINE configs[3] at a size the oracle finishes in seconds: device-built channel_announcements (4 signatures)
    + channel_updates, 1 % corrupted; per-message verdict = first bad signature"""
    from lightning_amd import workload
    w = workload.make_gossip(eng, 600, 2400, n_nodes=50, corrupt_frac=0.05)
    eng.sigcheck_gossip_device(w.n, w.d_msgs, w.d_off, w.d_ids, w.d_rowbase, w.rows, w.d_verdict)
    eng.synchronize()
    got = w.d_verdict.cpu().numpy()
    assert np.array_equal(got, w.expect), np.nonzero(got != w.expect)[0][:10]
    assert (w.expect != 0).sum() == 150 and set(np.unique(w.expect[:600])) == {0, 1, 2, 3, 4}
    # host-buffer API on the same bytes, and the CPU oracle on every message
    msgs = [w.msgs[int(w.off[i]):int(w.off[i + 1])].tobytes() for i in range(w.n)]
    ids = [w.ids[i].tobytes() if i >= w.n_cann else None for i in range(w.n)]
    assert np.array_equal(eng.sigcheck_gossip(msgs, ids), w.expect)
    for i in list(range(0, 600, 7)) + list(range(600, 3000, 13)):
        exp = orc.sigcheck_channel_announcement(msgs[i]) if i < 600 else orc.sigcheck_channel_update(msgs[i], ids[i])
        assert exp == w.expect[i], i
    # reference framing: 432-byte announcement, 138-byte update with a 72-byte signed region (wire/peer_wire.csv:344-381)
    assert len(msgs[0]) == 432 and len(msgs[-1]) == 138 and msgs[0][:2] == b"\x01\x00" and msgs[-1][:2] == b"\x01\x02"


def test_gossip_spans_any_selection_in_any_order_equals_the_range_call(eng):
    """lamd_sigcheck_gossip_spans_device (round 6): message i = msgs[start[i] : start[i] + len[i]] -- a PERMUTED selection of both message kinds,
    with gaps, as one call; every verdict equals the range call's (= construction) for the message it was taken from.  Also the two ranges a rank
    of a job cut per message kind holds (sharding.segment_bounds), as bench.py issues them."""
    import torch
    from lightning_amd import sharding, workload
    w = workload.make_gossip(eng, 700, 2100, n_nodes=40, corrupt_frac=0.08)
    rng = np.random.default_rng(0x5A)
    sel = rng.permutation(w.n)[:1900]                                   # any order, announcements and updates mixed, two thirds of the job
    d_sel = torch.from_numpy(sel).to("cuda:0")
    start = w.d_off[:-1][d_sel].contiguous()
    ln = (w.d_off[1:] - w.d_off[:-1])[d_sel].contiguous()
    ids = w.d_ids[d_sel].contiguous()
    rpm = (w.d_rowbase[1:] - w.d_rowbase[:-1])[d_sel]
    rowbase = torch.cat([torch.zeros(1, dtype=rpm.dtype, device=rpm.device), torch.cumsum(rpm, 0)]).contiguous()
    d_v = torch.full((len(sel),), 9, dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()
    eng.sigcheck_gossip_spans_device(len(sel), w.d_msgs, start, ln, ids, rowbase, int(rowbase[-1].item()), d_v)
    eng.synchronize()
    got = d_v.cpu().numpy()
    assert np.array_equal(got, w.expect[sel]), np.nonzero(got != w.expect[sel])[0][:10]
    assert set(np.unique(got)) >= {0, 1, 2, 3, 4}
    # a length that stops short of the message is that message's problem only (malformed -> -1), its neighbours keep their verdicts
    ln2 = ln.clone()
    ln2[5] = 40
    d_v.fill_(9)
    eng.sigcheck_gossip_spans_device(len(sel), w.d_msgs, start, ln2, ids, rowbase, int(rowbase[-1].item()), d_v)
    eng.synchronize()
    got2 = d_v.cpu().numpy()
    assert got2[5] == -1 and np.array_equal(np.delete(got2, 5), np.delete(w.expect[sel], 5))
    # an empty selection is no work; missing arrays are the caller's error (raw ABI)
    L, c = eng._lib, eng._ctx
    assert L.lamd_sigcheck_gossip_spans_device(c, 0, None, None, None, None, None, 0, None) == 0
    assert L.lamd_sigcheck_gossip_spans_device(c, 3, w.d_msgs.data_ptr(), start.data_ptr(), None, ids.data_ptr(), rowbase.data_ptr(), 3, d_v.data_ptr()) == -3
    assert L.lamd_sigcheck_gossip_spans_device(c, 3, w.d_msgs.data_ptr(), start.data_ptr(), ln.data_ptr(), ids.data_ptr(), rowbase.data_ptr(), 0, d_v.data_ptr()) == -3
    # the two ranges of rank 1 of 4 of the job cut per kind, as ONE call
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    gw = sharding.gossip_weights(w.msgs, w.off)
    sb = sharding.segment_bounds([0, w.n_cann, w.n], 4, gw)
    mine = [(int(sb[s, 1]), int(sb[s, 2])) for s in range(2)]
    sp = bench.gossip_spans(w, mine, "cuda:0")
    torch.cuda.synchronize()
    eng.sigcheck_gossip_spans_device(sp[0], w.d_msgs, sp[1], sp[2], sp[3], sp[4], sp[5], sp[6])
    eng.synchronize()
    assert np.array_equal(sp[6].cpu().numpy(), np.concatenate([w.expect[lo:hi] for lo, hi in mine]))
    assert mine[0][1] <= w.n_cann <= mine[1][0]


def test_cfg4_full_size_properties(eng, orc):
    """500 k channel_announcements + 2 M channel_updates = 4 M verifies on one GPU: every untouched message verifies,
    every corrupted one reports exactly the corrupted signature; an oracle sample agrees"""
    from lightning_amd import workload
    w = workload.make_gossip(eng, 500_000, 2_000_000, n_nodes=15000, corrupt_frac=0.01)
    assert w.rows == 4_000_000 and w.msgs.nbytes - 64 == 500_000 * 432 + 2_000_000 * 138
    eng.sigcheck_gossip_device(w.n, w.d_msgs, w.d_off, w.d_ids, w.d_rowbase, w.rows, w.d_verdict)
    eng.synchronize()
    got = w.d_verdict.cpu().numpy()
    assert np.array_equal(got, w.expect), (np.nonzero(got != w.expect)[0][:10])
    assert (got != 0).sum() == 25_000
    # EVERY message against the C oracle (not a sample): the workload is signed on the GPU with the engine's own arithmetic, so
    # "equals construction" alone would let a shared arithmetic error through
    exp = orc.sigcheck_gossip_batch(w.msgs, w.off, w.ids, _cores())
    assert np.array_equal(got, exp), (np.nonzero(got != exp)[0][:10])


def test_cfg5_commit_storm_streaming_batches(eng, orc):
    """BASELINE configs[4] shape: per channel 1 commitment signature + 483 HTLC signatures under one shared key,
    every 4th channel BIP-340, streamed as 484-row batches through the queue API; verdicts in ticket order"""
    from lightning_amd import workload
    st = workload.make_commit_storm(eng, 12, corrupt_frac=0.01)
    per = st["per"]
    assert per == 484 and list(st["kinds"]) == [0, 0, 0, 1] * 3
    we, ws = st["ecdsa"], st["schnorr"]
    # HTLC rows of a channel share the key, the commitment row has its own (channeld/channeld.c:2171,2224-2225)
    pk = we.cols[2].reshape(-1, per, 33)
    assert (pk[:, 1:, :] == pk[:, 1:2, :]).all() and not (pk[:, 0, :] == pk[:, 1, :]).all(axis=1).any()
    ie = isx = 0
    for c, kind in enumerate(st["kinds"]):
        if kind == 0:
            sl = slice(ie * per, (ie + 1) * per)
            for i in range(sl.start, sl.stop):
                eng.queue_ecdsa(we.cols[0][i].tobytes(), we.cols[1][i].tobytes(), we.cols[2][i].tobytes())
            eng.flush()
            got = eng.wait()
            assert np.array_equal(got, we.expect[sl]), c
            exp = orc.ecdsa_verify_batch(np.ascontiguousarray(we.cols[0][sl]), np.ascontiguousarray(we.cols[1][sl]),
                                         np.ascontiguousarray(we.cols[2][sl]), 33, 4).astype(bool)
            assert np.array_equal(got, exp)
            ie += 1
        else:
            sl = slice(isx * per, (isx + 1) * per)
            for i in range(sl.start, sl.stop):
                eng.queue_schnorr(ws.cols[0][i].tobytes(), ws.cols[1][i].tobytes(), ws.cols[2][i].tobytes())
            eng.flush()
            got = eng.wait()
            assert np.array_equal(got, ws.expect[sl]), c
            exp = orc.schnorr_verify_batch(np.ascontiguousarray(ws.cols[0][sl]), np.ascontiguousarray(ws.cols[1][sl]),
                                           np.ascontiguousarray(ws.cols[2][sl]), 4).astype(bool)
            assert np.array_equal(got, exp)
            isx += 1
    assert (~we.expect).sum() + (~ws.expect).sum() > 0


def test_cfg5_full_size_properties(eng, orc):
    """10 000 channels x 484 = 4.84 M verifies in super-batches: sign->verify round trip, corrupted rows rejected, and EVERY
    row against the C oracle"""
    from lightning_amd import workload
    st = workload.make_commit_storm(eng, 10_000)
    we, ws = st["ecdsa"], st["schnorr"]
    assert we.n + ws.n == 4_840_000
    eng.verify_ecdsa_device(we.dev[0], we.dev[1], we.dev[2], we.d_ok)
    eng.verify_schnorr_device(ws.dev[0], ws.dev[1], ws.dev[2], ws.d_ok)
    eng.synchronize()
    assert np.array_equal(strict_bool(we.d_ok.cpu().numpy()), we.expect)
    assert np.array_equal(strict_bool(ws.d_ok.cpu().numpy()), ws.expect)
    assert (~we.expect).sum() + (~ws.expect).sum() == int(we.n * 0.001) + int(ws.n * 0.001)
    ce = orc.ecdsa_verify_batch(we.cols[0], we.cols[1], we.cols[2], we.cols[2].shape[1], _cores()).astype(bool)
    cs = orc.schnorr_verify_batch(ws.cols[0], ws.cols[1], ws.cols[2], _cores()).astype(bool)
    assert np.array_equal(ce, we.expect) and np.array_equal(cs, ws.expect)


@pytest.fixture(scope="module", params=[7, 10])
def eng_keyed(request):
    """engine forced onto the keyed path (per-key comb tables) whenever a key repeats at all; both comb shapes"""
    import os
    from lightning_amd import Engine
    T = request.param
    os.environ["LAMD_KEYED"] = "1"
    os.environ["LAMD_KEYED_TEETH"] = str(T)
    try:
        e = Engine(0)
    finally:
        del os.environ["LAMD_KEYED"], os.environ["LAMD_KEYED_TEETH"]
    e.teeth = T
    yield e
    e.close()


def test_keyed_path_goldens_and_oracle(eng_keyed, orc, kat):
    e = eng_keyed
    for publen in (33, 65):
        vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 2 * publen]
        got = e.verify_ecdsa(_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64), _rows([H(v["pub"]) for v in vs], publen))
        bad = [v["name"] for v, g in zip(vs, got) if bool(g) != v["expect"]]
        assert not bad, bad[:10]
        inf = e.info()
        assert inf["last_keyed"] == e.teeth and 0 < inf["last_unique_keys"] < len(vs)
    vs = kat["schnorr"]
    got = e.verify_schnorr(_rows([H(v["msg"]) for v in vs], 32), _rows([H(v["pk"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64))
    bad = [v["name"] for v, g in zip(vs, got) if bool(g) != v["expect"]]
    assert not bad, bad[:10]
    assert e.info()["last_keyed"]
    vs = kat["gossip"]
    got = e.sigcheck_gossip([H(v["msg"]) for v in vs], [H(v["node_id"]) if "node_id" in v else None for v in vs])
    assert [int(g) for g in got] == [v["expect"] for v in vs]
    # random rows (distinct keys mixed with repeats) against the oracle, ragged sizes
    rnd = random.Random(99)
    for n in (3, 64, 65, 1000):
        hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
        hs, sg, pk = hs.copy(), sg.copy(), pk.copy()
        h = n // 2
        pk[h:2 * h] = pk[:h]                    # second half re-uses the first half's keys ...
        hs[h:2 * h:2] = hs[:h:2]                # ... every other row an exact duplicate (same verdict),
        sg[h:2 * h:2] = sg[:h:2]                # the others a foreign signature under that key (reject)
        got = e.verify_ecdsa(hs, sg, pk)
        exp = orc.ecdsa_verify_batch(hs, sg, pk, 33, 4).astype(bool)
        assert np.array_equal(got, exp), n


def test_keyed_path_auto_selection_and_parity(eng, orc):
    """auto mode: a big batch with few distinct keys takes the table path, a batch of distinct keys does not; both agree
    with the verdicts known by construction and with the oracle on a sample"""
    from lightning_amd import workload
    eng.cache_clear()                       # the counts below are those of keys met for the first time
    w = workload.make_ecdsa(eng, 30000, nkeys=100, publen=33)
    eng.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.synchronize()
    inf = eng.info()
    assert inf["last_keyed"] == 10 and 100 <= inf["last_unique_keys"] < 600  # >= 48 signatures per key: the 10-tooth comb
    assert inf["last_cache_hits"] == 0 and 90 <= inf["last_new_tables"] <= 110
    got = strict_bool(w.d_ok.cpu().numpy())
    assert np.array_equal(got, w.expect), (np.nonzero(got != w.expect)[0][:10], w.classes[got != w.expect][:10])
    sl = slice(0, 1200)
    exp = orc.ecdsa_verify_batch(np.ascontiguousarray(w.cols[0][sl]), np.ascontiguousarray(w.cols[1][sl]), np.ascontiguousarray(w.cols[2][sl]), 33, 4)
    assert np.array_equal(got[sl], exp.astype(bool))
    w = workload.make_schnorr(eng, 30000, nkeys=2000)
    eng.verify_schnorr_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.synchronize()
    assert eng.info()["last_keyed"] == 7                                       # ~13 signatures per key: the 7-tooth comb
    got = strict_bool(w.d_ok.cpu().numpy())
    assert np.array_equal(got, w.expect), (np.nonzero(got != w.expect)[0][:10], w.classes[got != w.expect][:10])
    w = workload.make_ecdsa(eng, 30000, nkeys=1 << 40, publen=65)          # all keys distinct
    eng.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.synchronize()
    inf = eng.info()
    assert not inf["last_keyed"] and inf["last_unique_keys"] > 29000
    assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect)


def test_chunk_splitting_small_chunks(orc, kat):
    """batches larger than one launch chunk are cut; forced here with 1000-row chunks"""
    import os
    from lightning_amd import Engine, workload
    os.environ["LAMD_CHUNK_ROWS"] = "1000"
    try:
        e = Engine(0)
    finally:
        del os.environ["LAMD_CHUNK_ROWS"]
    try:
        w = workload.make_ecdsa(e, 5300, nkeys=40, publen=33)
        e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
        e.synchronize()
        assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect)
        assert np.array_equal(e.verify_ecdsa(w.cols[0], w.cols[1], w.cols[2]), w.expect)
        ws = workload.make_schnorr(e, 3100, nkeys=1 << 40)
        assert np.array_equal(e.verify_schnorr(ws.cols[0], ws.cols[1], ws.cols[2]), ws.expect)
        g = workload.make_gossip(e, 700, 900, n_nodes=30, corrupt_frac=0.05)     # 3700 rows -> 4 chunks
        msgs = [g.msgs[int(g.off[i]):int(g.off[i + 1])].tobytes() for i in range(g.n)]
        ids = [g.ids[i].tobytes() if i >= g.n_cann else None for i in range(g.n)]
        assert np.array_equal(e.sigcheck_gossip(msgs, ids), g.expect)
        # the device-pointer entry cuts the same way (a message's four rows may straddle two chunks and two lanes)
        g.d_verdict.fill_(77)
        torch.cuda.synchronize()
        e.sigcheck_gossip_device(g.n, g.d_msgs, g.d_off, g.d_ids, g.d_rowbase, g.rows, g.d_verdict)
        e.synchronize()
        assert np.array_equal(g.d_verdict.cpu().numpy(), g.expect)
    finally:
        e.close()


def test_streaming_poll_and_error_states(eng, kat):
    import time
    from lightning_amd import LamdError
    v = kat["ecdsa"][0]
    with pytest.raises(LamdError):
        eng.wait()                      # nothing flushed
    for _ in range(300):
        eng.queue_ecdsa(H(v["hash"]), H(v["sig"]), H(v["pub"]))
    eng.flush()
    eng.queue_ecdsa(H(v["hash"]), H(v["sig"]), H(v["pub"]))         # queueing goes on while a flush is in flight ...
    eng.flush()
    sets = eng.info()["queue_sets"]
    for _ in range(sets - 2):
        eng.flush()                                                 # ... an empty flush is an outstanding flush too: one per staging set in all
    with pytest.raises(LamdError):
        eng.queue_ecdsa(H(v["hash"]), H(v["sig"]), H(v["pub"]))     # every staging set is in flight
    with pytest.raises(LamdError):
        eng.flush()
    got, t0 = None, time.time()
    while got is None and time.time() - t0 < 10:
        got = eng.poll()
    assert got is not None and len(got) == 300 and all(bool(x) == v["expect"] for x in got)
    assert list(eng.wait()) == [v["expect"]]                        # oldest first: the 1-row flush, then the empty ones
    assert [len(eng.wait()) for _ in range(sets - 2)] == [0] * (sets - 2)
    with pytest.raises(LamdError):
        eng.poll()                                                  # nothing outstanding any more
    with pytest.raises(ValueError):
        eng.verify_ecdsa(np.zeros((2, 32), np.uint8), np.zeros((2, 64), np.uint8), np.zeros((2, 40), np.uint8))   # 40-byte keys
    import ctypes
    ok = (ctypes.c_uint8 * 2)()
    rc = eng._lib.lamd_verify_ecdsa_batch(eng._ctx, 2, bytes(64), bytes(128), bytes(80), 40, 40, ok)               # and through the raw ABI
    assert rc == -3


def test_check_tx_sig_batch_fee_grind_kat(eng, kat):
    """onchaind/test/run-grind_feerate.c:119-154 through the device: 1000 candidate fees for one HTLC signature/key --
    check_tx_sig must accept exactly fee = 165 750 sat; plus the sighash-type gate of bitcoin/signature.c:206-211"""
    import pyref
    ko = next(v for v in kat["der"] if v["name"] == "KAT-O")
    sig = H(ko["expect_sig"])
    key = H("038ffd2621647812011960152bfb79c5a2787dfe6c4f37e2222547de054432eb7f")
    tx = H("0200000001e1ebca08cf1c301ac563580a1126d5c8fcb0e5e2043230b852c726553caf1e1d0000000000000000000160ae0a0000000000"
           "22002082e03c5a9cb79c82cd5a0572dc175290bc044609aabe9cc852d61927436041796d000000")
    txid, vout, seq, spk, lock = tx[5:37], 0, 0, tx[56:90], 109
    ws = H("76a914a8c40c334351dbe8e5908544f1c98fbcfb8719fc8763ac6721038ffd2621647812011960152bfb79c5a2787dfe6c4f37e2222547de05"
           "4432eb7f7c820120876475527c2103cf8e2f193a6aed60db80af75f3c8d59c2de735b299b7c7083527be9bd23b77a852ae67a914b8bcd51e"
           "fa35be1e50ae2d5f72f4500acb005c9c88ac6868")
    fees = list(range(165750 - 600, 165750 + 400))       # the reference grinds 1000 feerates
    pres = [pyref.bip143_sighash(2, [(txid, vout, seq)], [(700000 - f, spk)], lock, 0, ws, 700000, 1)[1] for f in fees]
    assert all(len(p) == 290 for p in pres)
    n = len(fees)
    got = eng.check_tx_sig_batch(pres, [1] * n, [1] * n, _rows([sig] * n, 64), _rows([key] * n, 33))
    assert got.sum() == 1 and fees[int(np.argmax(got))] == 165750
    # the gate: same good preimage under other sighash types / without witness script
    good = pres[600]
    types = [1, 0x83, 0x83, 2, 3, 0x81, 0, 1]
    wit = [1, 1, 0, 1, 1, 1, 1, 0]
    got = eng.check_tx_sig_batch([good] * 8, types, wit, _rows([sig] * 8, 64), _rows([key] * 8, 33))
    # SIGHASH_ALL passes the gate with or without a witness script, SINGLE|ANYONECANPAY only with one (here the caller
    # handed the same preimage bytes, so that row verifies too); every other type is rejected before any hashing
    assert [bool(x) for x in got] == [True, True, False, False, False, False, False, True]


def test_lanes_back_to_back_calls_without_host_sync(eng, orc):
    """successive device-pointer calls alternate between the engine's two lanes and overlap on the GPU; every call's
    verdict vector must still be complete and right after ONE synchronize, for ECDSA, BIP-340 and gossip interleaved"""
    from lightning_amd import workload
    ws = []
    for r in range(3):
        ws.append(("e", workload.make_ecdsa(eng, 40000 + 777 * r, seed=900 + r, nkeys=300 * (r + 1), publen=33 if r % 2 else 65)))
        ws.append(("s", workload.make_schnorr(eng, 30000 + 555 * r, seed=950 + r, nkeys=1 << 40 if r == 1 else 500)))
    g = workload.make_gossip(eng, 3000, 5000, n_nodes=200, corrupt_frac=0.03)
    eng.synchronize()
    for rep in range(3):
        for kind, w in ws:
            w.d_ok.zero_()
        torch.cuda.synchronize()
        for kind, w in ws:
            (eng.verify_ecdsa_device if kind == "e" else eng.verify_schnorr_device)(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
        g.d_verdict.fill_(99)
        torch.cuda.synchronize()
        eng.sigcheck_gossip_device(g.n, g.d_msgs, g.d_off, g.d_ids, g.d_rowbase, g.rows, g.d_verdict)
        eng.synchronize()
        gv = g.d_verdict
        for kind, w in ws:
            assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect), (rep, kind, w.n)
        assert np.array_equal(gv.cpu().numpy(), g.expect)
    inf = [eng.info(k) for k in range(eng.info()["lanes"])]
    assert len(inf) == 6 and {i["last_mode"] for i in inf} <= {0, 1}   # (LAMD_LANES default)
    # a caller's stream can wait for the results on the device instead of blocking the host
    kind, w = ws[0]
    w.d_ok.zero_()
    torch.cuda.synchronize()
    eng.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.stream_wait_results(torch.cuda.current_stream().cuda_stream)
    got = w.d_ok.clone()                       # on torch's stream: ordered after the verification by the event
    torch.cuda.synchronize()
    assert np.array_equal(strict_bool(got.cpu().numpy()), w.expect)
    eng.synchronize()


def test_two_phase_join_and_event_ordering(eng):
    """lamd_results_mark / lamd_stream_wait_mark: a consumer stream joins exactly the work that was marked, after later calls were
    submitted; lamd_wait_event: a verdict buffer is rewritten only after the consumer's copy of it.  The pattern of bench.py's
    collective path, checked against verdicts known by construction"""
    from lightning_amd import LamdError, workload
    wa = workload.make_ecdsa(eng, 50000, seed=4401, nkeys=700, publen=65)
    wb = workload.make_schnorr(eng, 45000, seed=4402, nkeys=600)
    eng.synchronize()
    consumer = torch.cuda.Stream()
    with pytest.raises(LamdError):
        eng.stream_wait_mark(13, consumer.cuda_stream)       # never marked
    with pytest.raises(LamdError):
        eng.results_mark(16)                                 # slots are 0..15
    copies, last_ev = [], [None, None]
    for rep in range(4):
        for slot, (w, call) in enumerate(((wa, eng.verify_ecdsa_device), (wb, eng.verify_schnorr_device))):
            if last_ev[slot] is not None:
                eng.wait_event(last_ev[slot].cuda_event)     # the consumer's copy of this buffer (previous round) comes first
            if rep == 2:                                     # poison through torch's stream: after the consumer's copy, before the call
                torch.cuda.current_stream().wait_event(last_ev[slot])
                w.d_ok.fill_(5)
                eng.wait_stream(torch.cuda.current_stream().cuda_stream)
            call(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
            eng.results_mark(slot)
        for slot, w in enumerate((wa, wb)):                  # joined late: both calls of the round are already queued
            eng.stream_wait_mark(slot, consumer.cuda_stream)
            with torch.cuda.stream(consumer):
                copies.append((w, w.d_ok.clone()))
                ev = torch.cuda.Event()
                ev.record()
            last_ev[slot] = ev
    consumer.synchronize()
    eng.synchronize()
    for w, got in copies:
        assert np.array_equal(strict_bool(got.cpu().numpy()), w.expect), w.kind


def test_single_lane_mode_matches(orc):
    import os
    from lightning_amd import Engine, LamdError, workload
    os.environ["LAMD_LANES"] = "1"
    try:
        e = Engine(0)
    finally:
        del os.environ["LAMD_LANES"]
    try:
        w = workload.make_ecdsa(e, 50000, seed=31, nkeys=700, publen=33)
        s = workload.make_schnorr(e, 20000, seed=32, nkeys=100)
        e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
        e.verify_schnorr_device(s.dev[0], s.dev[1], s.dev[2], s.d_ok)
        e.synchronize()
        assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect)
        assert np.array_equal(strict_bool(s.d_ok.cpu().numpy()), s.expect)
        assert e.info()["lanes"] == 1 and e.info(0) == e.info()
        with pytest.raises(LamdError):
            e.info(1)
    finally:
        e.close()


@pytest.mark.parametrize("env", [{"LAMD_FUSED_FRONT": "0"}, {"LAMD_MERGE_SIDE": "0"}, {"LAMD_ECMULT_CHAIN": "1"}, {"LAMD_ECMULT_CHAIN": "2", "LAMD_ECMULT_TAIL": "50000"}, {"LAMD_COPY_STREAM": "0"},
                                 {"LAMD_FUSED_FRONT": "0", "LAMD_CACHE": "0"}, {"LAMD_CACHE": "0"}, {"LAMD_GROUP": "0"}, {"LAMD_PAIRS": "1"},
                                 {"LAMD_PAIRS": "1", "LAMD_GROUP": "0", "LAMD_CACHE": "0"},
                                 # round 5: the flush's copies -- three with three events (round 4), one event, two copy streams, a full set as one copy or not
                                 {"LAMD_COPY_EVENTS": "3", "LAMD_COPY_ONE": "0"}, {"LAMD_COPY_EVENTS": "1", "LAMD_COPY_ONE": "0"}, {"LAMD_COPY_EVENTS": "2"},
                                 {"LAMD_COPY_STREAMS": "2"}, {"LAMD_COPY_EVENTS": "1", "LAMD_COPY_ONE": "1", "LAMD_COPY_STREAMS": "3"},
                                 # ... and calls cut into chunks that alternate between a lane and its peer (lamd_set_chunk_rows does the same at run time)
                                 {"LAMD_CHUNK_ROWS": "20000"},
                                 # round 6: the cold rows listed by k_partition again (after the table kernels), no wave priorities, every priority, the ladder on its own stream beside the early list
                                 {"LAMD_EARLY_COLD": "0"}, {"LAMD_PRIO": "0"}, {"LAMD_PRIO": "31"}, {"LAMD_EARLY_COLD": "0", "LAMD_PRIO": "0", "LAMD_CACHE": "0"}, {"LAMD_MERGE_SIDE": "0", "LAMD_CACHE": "0"}])
def test_scheduling_variants_give_the_same_verdicts(orc, env):
    """the round-2 front end (19 launches), the ladder on a stream of its own, chained ecmult launches, flush copies on the lane's prep
    stream, row lists in arrival order instead of grouped by key, the pairs-first ecmult kernel (k_ecmult_keyed_pairs: both comb shapes
    occur below): every scheduling variant the engine still carries must produce the verdicts of the default one -- against the C oracle on a
    sample and by construction on every row; calls back to back over all lanes, the streaming queue with more flushes in flight than lanes"""
    import os
    from lightning_amd import Engine, workload
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        w = workload.make_ecdsa(e, 120000, seed=41, nkeys=3000, publen=33)
        s = workload.make_schnorr(e, 90000, seed=42, nkeys=900)
        x = workload.make_ecdsa(e, 70000, seed=43, nkeys=1 << 40, publen=65, group=1)      # every row its own key: all on the ladder
        for rep in range(3):
            for wl in (w, s, x):
                wl.d_ok.fill_(9)
            torch.cuda.synchronize()
            e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
            e.verify_schnorr_device(s.dev[0], s.dev[1], s.dev[2], s.d_ok)
            e.verify_ecdsa_device(x.dev[0], x.dev[1], x.dev[2], x.d_ok)
            e.synchronize()
            for wl in (w, s, x):
                assert np.array_equal(strict_bool(wl.d_ok.cpu().numpy()), wl.expect), (env, rep, wl.kind)
        # lamd_set_chunk_rows at run time: the same calls cut in two / in many, then whole again
        for rows in (60000, 4096, 0):
            e.set_chunk_rows(rows)
            for wl in (w, x):
                wl.d_ok.fill_(9)
            torch.cuda.synchronize()
            e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
            e.results_mark_last(5)                       # one event on the call's own lane: a consumer that waits for it sees this call's verdicts
            e.stream_wait_mark(5, torch.cuda.current_stream().cuda_stream)
            got_w = w.d_ok.clone()                       # (on torch's stream, behind the mark)
            e.verify_ecdsa_device(x.dev[0], x.dev[1], x.dev[2], x.d_ok)
            e.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(strict_bool(got_w.cpu().numpy()), w.expect), (env, rows)
            assert np.array_equal(strict_bool(x.d_ok.cpu().numpy()), x.expect), (env, rows)
        sample = slice(0, 3000)
        assert np.array_equal(orc.ecdsa_verify_batch(*[np.ascontiguousarray(c[sample]) for c in w.cols], 33, 4).astype(bool), w.expect[sample])
        assert np.array_equal(orc.schnorr_verify_batch(*[np.ascontiguousarray(c[sample]) for c in s.cols], 4).astype(bool), s.expect[sample])
        # streaming: six flushes outstanding on four lanes
        pend = []
        for rep in range(8):
            wl = (w, s)[rep & 1]
            if wl is w:
                e.queue_ecdsa_batch(*wl.cols)
            else:
                e.queue_schnorr_batch(*wl.cols)
            e.flush()
            pend.append(wl)
            if len(pend) == 6:
                assert np.array_equal(e.wait(cap=pend[0].n).astype(bool), pend.pop(0).expect), env
        while pend:
            assert np.array_equal(e.wait(cap=pend[0].n).astype(bool), pend.pop(0).expect), env
    finally:
        e.close()


def test_engines_of_one_process_share_the_g_table(kat):
    """the 11 GiB static table of G exists once per device and process (reference-counted by lamd_init / lamd_shutdown): a second engine does
    not build another, closing the first leaves it to the second, and after the last one is gone the next engine builds it again"""
    import time
    from lightning_amd import Engine
    vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 66][:64]
    rows = (_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64), _rows([H(v["pub"]) for v in vs], 33))
    want = [v["expect"] for v in vs]
    e1 = Engine(0)
    t0 = time.perf_counter()
    e2 = Engine(0)
    t_second = time.perf_counter() - t0
    assert [bool(g) for g in e1.verify_ecdsa(*rows)] == want
    e1.close()
    assert [bool(g) for g in e2.verify_ecdsa(*rows)] == want          # the table outlives the engine that built it
    big = [np.concatenate([r] * 200) for r in rows]                     # the general path reads it too
    assert [bool(g) for g in e2.verify_ecdsa(*big)] == want * 200
    e2.close()
    with Engine(0) as e3:                                               # built afresh
        assert [bool(g) for g in e3.verify_ecdsa(*rows)] == want
    assert t_second < 5.0


def test_device_self_diagnostics(eng, kat):
    """the diagnostic entry points (every arithmetic stage evaluated on the device and, with the same inline functions, on
    the host) must report no difference -- they are how a code-generation problem is localised on a new toolchain"""
    v = next(x for x in kat["ecdsa"] if x["name"] == "KAT-B11")
    rc, rep = eng.selftest(H(v["hash"]), H(v["sig"]), H(v["pub"]))
    assert rc == 0, rep
    assert "host verdict lane0=1 device=1" in rep
    rc, rep = eng.inv_debug()
    assert rc == 0, rep
    for use_mul in (0, 1):
        rc, rep = eng.chain_debug(use_mul)
        assert rc == 0, rep


def test_one_call_larger_than_a_chunk_full_size(eng):
    """5 M rows in ONE call: two launch chunks (2^22 + the rest) on alternating lanes, 300 k distinct keys"""
    from lightning_amd import workload
    w = workload.make_ecdsa(eng, 5_000_000, seed=4242, nkeys=300_000, publen=33)
    eng.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
    eng.synchronize()
    got = strict_bool(w.d_ok.cpu().numpy())
    assert np.array_equal(got, w.expect), np.nonzero(got != w.expect)[0][:10]
    assert 0 < (~w.expect).sum() < w.n


def _kat_o(kat):
    ko = next(v for v in kat["der"] if v["name"] == "KAT-O")
    sig = H(ko["expect_sig"])
    key = H("038ffd2621647812011960152bfb79c5a2787dfe6c4f37e2222547de054432eb7f")
    tx = H("0200000001e1ebca08cf1c301ac563580a1126d5c8fcb0e5e2043230b852c726553caf1e1d0000000000000000000160ae0a0000000000"
           "22002082e03c5a9cb79c82cd5a0572dc175290bc044609aabe9cc852d61927436041796d000000")
    txid, vout, seq, spk, lock = tx[5:37], 0, 0, tx[56:90], 109
    ws = H("76a914a8c40c334351dbe8e5908544f1c98fbcfb8719fc8763ac6721038ffd2621647812011960152bfb79c5a2787dfe6c4f37e2222547de05"
           "4432eb7f7c820120876475527c2103cf8e2f193a6aed60db80af75f3c8d59c2de735b299b7c7083527be9bd23b77a852ae67a914b8bcd51e"
           "fa35be1e50ae2d5f72f4500acb005c9c88ac6868")
    amount_in_tx = int.from_bytes(tx[47:55], "little")
    pre = pyref.bip143_sighash(2, [(txid, vout, seq)], [(amount_in_tx, spk)], lock, 0, ws, 700000, 1)[1]
    outputs = amount_in_tx.to_bytes(8, "little") + bytes([len(spk)]) + spk
    return sig, key, pre, outputs


def test_grind_htlc_tx_fee_reference_kat(eng, kat, orc):
    """onchaind/test/run-grind_feerate.c:119-154 as the reference runs it: weight 663, feerates 249 001..250 000, input
    700 000 sat -> fee 165 750 (feerate 250 000); the device grind must stop where the reference's ascending loop stops"""
    sig, key, pre, outputs = _kat_o(kat)
    assert len(pre) == 290 and len(outputs) == 43
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, sig, 1, True, key) == (250000, 165750)
    ver = lambda h, s, k: orc.ecdsa_verify(h, s, k)
    assert pyref.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, sig, 1, True, key, verify=ver) == (250000, 165750)
    # wider and shifted ranges: always the LOWEST feerate giving fee 165 750 (250 000 * 663 / 1000 = 165 750 exactly)
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 0, 400000, sig, 1, True, key) == (250000, 165750)
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 250000, 250000, sig, 1, True, key) == (250000, 165750)
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 250001, 250001, sig, 1, True, key) == (250001, 165750)  # same fee, first in range
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 250002, 300000, sig, 1, True, key) is None
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 0, 249998, sig, 1, True, key) is None
    # the preimage's own hashOutputs bytes are irrelevant (every candidate replaces them)
    junk = pre[:-40] + bytes(32) + pre[-8:]
    assert eng.grind_htlc_tx_fee(junk, outputs, 700000, 663, 249001, 250000, sig, 1, True, key) == (250000, 165750)
    # gate, wrong key / signature, fee above the input
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, sig, 0x83, False, key) is None
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, sig, 2, True, key) is None
    other = H("02" + "79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798")
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, sig, 1, True, other) is None
    bad = sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
    assert eng.grind_htlc_tx_fee(pre, outputs, 700000, 663, 249001, 250000, bad, 1, True, key) is None
    assert eng.grind_htlc_tx_fee(pre, outputs, 165749, 663, 0, 400000, sig, 1, True, key) is None       # input too small for that fee


def test_reference_held_transactions_bolt3_htlc_and_second_grind_kat(eng, kat):
    """check_tx_sig from transaction templates on the signed BOLT #3 HTLC transactions the reference's channeld test holds (both signatures of
    each; rejected with the spent amount off by one) -- through the one-launch path (20 rows) and, repeated past 4096 rows, through the batch
    path with the BIP143 hash on the device; the second fee-grind known answer (run-grind_feerate-bug.c: only the cltv-586034 candidate fits)"""
    rows = kat["txsig"]
    txs = [dict(version=v["version"], locktime=v["locktime"], inputs=[(H(t), vout, seq) for t, vout, seq in v["inputs"]],
                outputs=[(a, H(spk)) for a, spk in v["outputs"]], input_num=v["input_num"], amount=v["amount"], script=H(v["script"]),
                sighash_type=v["sighash_type"], has_witness=v["has_witness"]) for v in rows]
    sigs, pubs, exp = _rows([H(v["sig"]) for v in rows], 64), _rows([H(v["pub"]) for v in rows], 33), [v["expect"] for v in rows]
    assert [bool(g) for g in eng.check_tx_sig_tx_batch(txs, sigs, pubs)] == exp
    reps = 4100 // len(rows) + 1
    got = eng.check_tx_sig_tx_batch(txs * reps, np.tile(sigs, (reps, 1)), np.tile(pubs, (reps, 1)))
    assert [bool(g) for g in got] == exp * reps
    for v in kat["grind"]:
        got = eng.grind_htlc_tx_fee(H(v["preimage"]), H(v["outputs"]), v["input_sat"], v["weight"], v["min_feerate"], v["max_feerate"], H(v["sig"]),
                                    v["sighash_type"], True, H(v["pub"]))
        assert (list(got) if got else None) == v["expect"], v["name"]


def test_grind_htlc_tx_fee_random_vs_oracle(eng, orc):
    """seeded synthetic HTLC transactions signed at a hidden feerate: the device grind and the restated reference loop
    (pyref.grind_htlc_tx_fee over the C oracle's ECDSA) must return the same (feerate, fee) -- or both nothing"""
    rnd = random.Random(2024)
    ver = lambda h, s, k: orc.ecdsa_verify(h, s, k)
    for case in range(12):
        sk = rnd.randrange(1, pyref.N).to_bytes(32, "big")
        pub = pyref.ser33(pyref.pubkey_create(int.from_bytes(sk, "big")))
        script = bytes(rnd.randrange(256) for _ in range(rnd.choice((1, 25, 133, 140, 200))))
        spk = bytes([0, 32]) + bytes(rnd.randrange(256) for _ in range(32))
        input_sat = rnd.randrange(50_000, 5_000_000)
        weight = rnd.choice((663, 703, 666, 706, 1000, 1))
        lo = rnd.randrange(0, 30_000)
        hi = lo + rnd.randrange(0, 3000)
        hidden = rnd.randrange(max(0, lo - 50), hi + 50) if case % 4 else hi + 1000       # sometimes outside the range
        fee = hidden * weight // 1000
        amount = max(0, input_sat - fee)
        txid = bytes(rnd.randrange(256) for _ in range(32))
        stype = 0x83 if case % 3 == 0 else 1
        sighash, pre = pyref.bip143_sighash(2, [(txid, rnd.randrange(4), rnd.randrange(2))], [(amount, spk)], rnd.randrange(1 << 31), 0, script, input_sat, stype)
        sig = orc.ecdsa_sign(sighash, sk, bytes(rnd.randrange(256) for _ in range(32)))
        outputs = amount.to_bytes(8, "little") + bytes([len(spk)]) + spk
        start = pre[:-40] + bytes(rnd.randrange(256) for _ in range(32)) + pre[-8:]
        exp = pyref.grind_htlc_tx_fee(start, outputs, input_sat, weight, lo, hi, sig, stype, True, pub, verify=ver)
        got = eng.grind_htlc_tx_fee(start, outputs, input_sat, weight, lo, hi, sig, stype, True, pub)
        assert got == exp, (case, got, exp)
        if lo <= hidden <= hi and fee <= input_sat:
            assert got is not None and got[1] == fee


def test_recover_goldens_and_random(eng, kat, orc):
    """lamd_ecdsa_recover_batch: the reference's BOLT11 invoices recover the pinned node id; edge classes; seeded random rows vs pyref"""
    rows = kat["recover"]
    keys, ok = eng.ecdsa_recover(_rows([H(v["hash"]) for v in rows], 32), _rows([H(v["sig"]) for v in rows], 64), [v["recid"] & 0xFF for v in rows])
    for v, k, o in zip(rows, keys, ok):
        assert (k.tobytes().hex() if o else None) == v["expect"], v["name"]
        assert o or not k.any()
    rnd = random.Random(31337)
    for n in (1, 63, 64, 700):
        hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
        rid = np.array([rnd.randrange(4) if i % 7 == 0 else rnd.randrange(2) for i in range(n)], dtype=np.uint8)
        sg = sg.copy()
        for i in range(0, n, 5):
            sg[i, rnd.randrange(64)] ^= 1 << rnd.randrange(8)          # damaged signatures still recover SOME key, or fail
        keys, ok = eng.ecdsa_recover(hs, sg, rid)
        for i in range(n):
            e = pyref.ecdsa_recover(hs[i].tobytes(), sg[i].tobytes(), int(rid[i]))
            assert (keys[i].tobytes() if ok[i] else None) == (pyref.ser33(e) if e else None), (n, i)
    assert eng.ecdsa_recover(np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), np.zeros(0, np.uint8))[1].shape == (0,)
    # a few thousand rows against the OpenSSL-arithmetic restatement (independent of pyref and of the device code)
    n = 4000
    hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
    sg = sg.copy()
    sg[::9, 40] ^= 0x04
    rid = np.array([rnd.randrange(2) for _ in range(n)], dtype=np.uint8)
    keys, ok = eng.ecdsa_recover(hs, sg, rid)
    hit = 0
    for i in range(n):
        e = orc.ossl_ecdsa_recover(hs[i].tobytes(), sg[i].tobytes(), int(rid[i]))
        assert (keys[i].tobytes() if ok[i] else None) == e, i
        hit += e == pk[i].tobytes()
    assert 0.3 * n < hit < 0.7 * n                    # the signer's key comes back for about half of the random recovery ids
    # and 60 000 rows against the C oracle's batch driver
    n = 60000
    hs, sg, pk = _random_ecdsa(orc, rnd, 2000, 33)
    hs, sg = np.tile(hs, (30, 1)), np.tile(sg, (30, 1))
    tw = np.frombuffer(bytes(rnd.randrange(256) for _ in range(n)), dtype=np.uint8)
    hs = hs.copy(); hs[:, 7] ^= tw                    # 60 000 distinct hashes under 2 000 signatures: all recover SOME key
    rid = (tw & 3).astype(np.uint8) % 2
    keys, ok = eng.ecdsa_recover(hs, sg, rid)
    ck, cok = orc.ecdsa_recover_batch(np.ascontiguousarray(hs), np.ascontiguousarray(sg), rid, 8)
    assert np.array_equal(ok, cok.astype(bool)) and np.array_equal(keys, ck) and ok.sum() > 0.4 * n


def test_recover_then_verify_round_trip_full_size(eng):
    """1 M generated signatures: for the untouched rows exactly one of the recovery ids 0/1 returns the signer's key, and EVERY
    key that recovery returns (damaged rows included) verifies the row's signature when fed back through the verification path"""
    from lightning_amd import workload
    w = workload.make_ecdsa(eng, 1_000_000, seed=777, nkeys=50_000, publen=33)
    n = w.n
    dev = w.d_ok.device
    keys = [torch.zeros((n, 33), dtype=torch.uint8, device=dev) for _ in range(2)]
    oks = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    rids = [torch.full((n,), rid, dtype=torch.uint8, device=dev) for rid in (0, 1)]
    torch.cuda.synchronize()                 # inputs made on torch's stream must be complete (and stay alive) for the engine's lanes
    for rid in (0, 1):
        eng.ecdsa_recover_device(w.dev[0], w.dev[1], rids[rid], keys[rid], oks[rid])
    eng.synchronize()
    signer = w.dev[2]
    match = [(keys[r] == signer).all(dim=1) & (oks[r] == 1) for r in (0, 1)]
    good = torch.from_numpy(w.expect).to(dev)
    assert bool(((match[0] ^ match[1]) | ~good).all())                  # valid rows: exactly one recovery id gives the signer
    assert int((match[0] | match[1])[good].sum()) == int(good.sum())
    for r in (0, 1):
        v = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.verify_ecdsa_device(w.dev[0], w.dev[1], keys[r], v)      # rows whose recovery failed carry a zero key: rejected
        eng.synchronize()
        rec_ok = oks[r] == 1
        # a recovered key satisfies the ECDSA equation by construction; verification adds only the low-S rule
        s_hi = w.dev[1][:, 32] >= 0x80
        assert bool(((v == 1) | ~rec_ok | s_hi).all())
        assert not bool((v[~rec_ok] == 1).any())


def test_streaming_pipelined_flushes(eng, orc):
    """a sidecar's inner loop: keep two flushes in flight while the next batch is being queued; verdicts come back per flush,
    oldest first, in ticket order, and equal the oracle's"""
    rnd = random.Random(555)
    batches = []
    for b in range(7):
        n = rnd.choice((1, 37, 484, 484, 1500))
        hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
        sg = sg.copy()
        sg[::3, 5] ^= 0x10
        batches.append((hs, sg, pk, orc.ecdsa_verify_batch(hs, sg, pk, 33, 4).astype(bool)))
    outstanding, results = [], []
    for hs, sg, pk, exp in batches:
        for i in range(hs.shape[0]):
            eng.queue_ecdsa(hs[i].tobytes(), sg[i].tobytes(), pk[i].tobytes())
        eng.flush()
        outstanding.append(exp)
        if len(outstanding) == 3:                       # up to three in flight while the next one is being filled
            results.append((eng.wait(), outstanding.pop(0)))
    while outstanding:
        results.append((eng.wait(), outstanding.pop(0)))
    assert len(results) == len(batches)
    for got, exp in results:
        assert np.array_equal(np.asarray(got, dtype=bool), exp)


def test_streaming_zero_copy_reserve_mixed_with_copies(eng, orc):
    """lamd_queue_reserve(): the producer writes its rows straight into the pinned staging set; mixed with the copying forms inside
    one flush (tickets keep counting across them), three kinds, several flushes in flight -- verdicts equal the oracle's"""
    rnd = random.Random(777)
    outstanding = []
    for b in range(6):
        n1, n2, n3 = rnd.choice((1, 64, 700)), rnd.choice((3, 484)), rnd.choice((5, 129))
        hs, sg, pk = _random_ecdsa(orc, rnd, n1 + n2, 33)
        sg = sg.copy(); sg[::4, 9] ^= 0x01
        e33 = orc.ecdsa_verify_batch(hs, sg, pk, 33, 4).astype(bool)
        hs65, sg65, pk65 = _random_ecdsa(orc, rnd, n3, 65)
        hs65 = hs65.copy(); hs65[::3, 0] ^= 0x80
        e65 = orc.ecdsa_verify_batch(hs65, sg65, pk65, 65, 4).astype(bool)
        t0, a, s_, k = eng.queue_reserve(n1, 33)                 # rows 0..n1 of the 33-byte-key queue, in place
        a[:], s_[:], k[:] = hs[:n1], sg[:n1], pk[:n1]
        t1 = eng.queue_ecdsa_batch(hs[n1:], sg[n1:], pk[n1:])   # the copying form continues the same queue
        t2, a, s_, k = eng.queue_reserve(n3, 65)
        a[:], s_[:], k[:] = hs65, sg65, pk65
        assert (t0, t1, t2) == (0, n1, n1 + n2)
        eng.flush()
        outstanding.append(np.concatenate([e33, e65]))
        if len(outstanding) == 3:
            assert np.array_equal(eng.wait(), outstanding.pop(0))
    while outstanding:
        assert np.array_equal(eng.wait(), outstanding.pop(0))
    with pytest.raises(Exception):
        eng.queue_reserve(4, 40)                                 # not a key length


def _page_block(x):
    """a copy of x in anonymous pages of its own (page-aligned, whole pages): what a host registers"""
    import mmap
    m = mmap.mmap(-1, max(mmap.PAGESIZE, (x.nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE))
    a = np.frombuffer(m, dtype=np.uint8, count=x.nbytes).reshape(x.shape)
    a[:] = x
    return a


def test_streaming_rows_queued_in_place(eng, orc):
    """lamd_queue_*_batch_inplace(): rows that stay in the caller's memory (registered or not) and cross the bus from there, mixed inside one flush
    with copied rows before, between and after them (tickets keep counting), three kinds, small batches (copied: the latency kernel's) and large
    ones, several flushes in flight -- verdicts equal the oracle's"""
    rnd = random.Random(4242)
    outstanding, keep = [], []
    for b in range(5):
        n_copy, n_in1, n_mid, n_in2 = rnd.choice((1, 300)), rnd.choice((4097, 9000)), rnd.choice((0, 77)), rnd.choice((5000, 4100))
        n = n_copy + n_in1 + n_mid + n_in2
        hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
        sg = sg.copy(); sg[::5, 40] ^= 0x04
        e33 = orc.ecdsa_verify_batch(hs, sg, pk, 33, 4).astype(bool)
        ns = rnd.choice((4500, 6000))
        ms, xs, ss, es = _random_schnorr(orc, rnd, ns)
        n65 = rnd.choice((10, 4200))
        hs65, sg65, pk65 = _random_ecdsa(orc, rnd, n65, 65)
        e65 = orc.ecdsa_verify_batch(hs65, sg65, pk65, 65, 4).astype(bool)
        o1, o2, o3 = n_copy, n_copy + n_in1, n_copy + n_in1 + n_mid
        # even batches: p1 and the BIP-340 rows live in blocks of whole pages of their own, registered (they stay in place); everything else -- p2, the
        # 65-byte-key rows, all of the odd batches -- is plain pageable memory (views of larger arrays): the engine copies such rows
        own = (lambda x: _page_block(x)) if b % 2 == 0 else np.ascontiguousarray
        part = lambda lo, hi, f: [f(x[lo:hi]) for x in (hs, sg, pk)]
        p1, p2 = part(o1, o2, own), part(o3, n, np.ascontiguousarray)
        sch = [own(x) for x in (ms, xs, ss)]
        p65 = [np.ascontiguousarray(x) for x in (hs65, sg65, pk65)]
        keep.append((p1, p2, sch, p65))                              # alive and unchanged until collected
        if b % 2 == 0:
            assert all(eng.host_register(x) for x in p1 + sch), "hipHostRegister refused whole pages of host memory"
        t0 = eng.queue_ecdsa_batch(hs[:o1], sg[:o1], pk[:o1])
        t1 = eng.queue_ecdsa_batch_inplace(*p1)
        if n_mid:
            eng.queue_ecdsa_batch(hs[o2:o3], sg[o2:o3], pk[o2:o3])
        t2 = eng.queue_ecdsa_batch_inplace(*p2)
        t3 = eng.queue_schnorr_batch_inplace(*sch)
        t4 = eng.queue_ecdsa_batch_inplace(*p65) if b % 2 else eng.queue_ecdsa_batch(*p65)
        assert (t0, t1, t2, t3, t4) == (0, o1, o3, n, n + ns)
        eng.flush()
        outstanding.append((np.concatenate([e33, es, e65]), b))
        if len(outstanding) == 3:
            exp, bb = outstanding.pop(0)
            assert np.array_equal(eng.wait(), exp), bb
            if bb % 2 == 0:
                assert all(eng.host_unregister(x) for x in keep[bb][0] + keep[bb][2])
    while outstanding:
        exp, bb = outstanding.pop(0)
        assert np.array_equal(eng.wait(), exp), bb
        if bb % 2 == 0:
            assert all(eng.host_unregister(x) for x in keep[bb][0] + keep[bb][2])
    with pytest.raises(ValueError):
        eng.queue_ecdsa_batch_inplace(hs[:, :31], sg, pk)


def _registered_block(eng, x, regs):
    """x copied into pages of its own, registered (lamd_host_register) -- recorded in regs for host_unregister"""
    a = _page_block(x)
    assert eng.host_register(a), "hipHostRegister refused whole pages of host memory"
    regs.append(a)
    return a


def test_streaming_in_place_rows_across_chunk_boundaries(eng, orc):
    """the in-place branch of lamd_flush with more rows in a kind than one chunk (set_chunk_rows 4 096 instead of 2^22): in-place runs
    that begin and end inside chunks and straddle one to three chunk boundaries, copied runs before, between and after them, three kinds, three
    flushes in flight -- verdicts equal the oracle's row for row, and lamd_info.last_flush_inplace_rows shows that the in-place rows crossed the bus
    from the caller's registered pages (not copied into the staging set)"""
    rnd = random.Random(6161)
    P33, P65, PS = 16000, 9600, 7600
    hs, sg, pk = _random_ecdsa(orc, rnd, P33, 33)
    e33 = orc.ecdsa_verify_batch(hs, sg, pk, 33, 8).astype(bool)
    hs65, sg65, pk65 = _random_ecdsa(orc, rnd, P65, 65)
    e65 = orc.ecdsa_verify_batch(hs65, sg65, pk65, 65, 8).astype(bool)
    ms, xs, ss, es = _random_schnorr(orc, rnd, PS)
    assert (~e33).sum() > P33 // 10 and (~es).sum() > PS // 10

    def pool(cols, exp, shift, n):        # n rows of a pool, starting at `shift` (wrapping): -> (columns, verdicts)
        idx = (np.arange(n) + shift) % len(exp)
        return [np.ascontiguousarray(c[idx]) for c in cols], exp[idx]

    eng.set_chunk_rows(4096)
    outstanding, regs_of = [], []
    try:
        for f in range(5):
            regs, exp, inplace = [], [], 0
            # ECDSA-33: copied | in place (straddles 2-3 chunk boundaries) | copied | in place (1-2) | copied
            lay33 = [(300 + 17 * f, False), (9000 + 613 * f, True), (77, False), (5000 - 211 * f, True), (123 + f, False)]
            # ECDSA-65: copied | in place (1-2 boundaries) | copied;  BIP-340: copied | in place (1-2) | copied
            lay65 = [(50 + 31 * f, False), (8500 - 397 * f, True), (20, False)]
            lays = [(6 * f + 1, False), (6000 + 401 * f, True), (5, False)]
            ticket = 0
            for kind, lay, cols, vexp in (("e33", lay33, (hs, sg, pk), e33), ("sch", lays, (ms, xs, ss), es), ("e65", lay65, (hs65, sg65, pk65), e65)):
                at = 1000 * f
                for n, inp in lay:
                    c, v = pool(cols, vexp, at, n)
                    at += n
                    if inp:
                        c = [_registered_block(eng, x, regs) for x in c]
                        inplace += n
                    if kind == "sch":
                        t = (eng.queue_schnorr_batch_inplace if inp else eng.queue_schnorr_batch)(*c)
                    else:
                        t = (eng.queue_ecdsa_batch_inplace if inp else eng.queue_ecdsa_batch)(*c)
                    assert t == ticket, (f, kind, t, ticket)
                    ticket += n
                    exp.append(v)
            eng.flush()
            moved = eng.info()["last_flush_inplace_rows"]
            assert moved == inplace, (f, moved, inplace)
            outstanding.append((np.concatenate(exp), f, regs))
            if len(outstanding) == 3:
                e, ff, rr = outstanding.pop(0)
                got = eng.wait()
                assert np.array_equal(got, e), (ff, np.nonzero(got != e)[0][:10])
                assert all(eng.host_unregister(x) for x in rr)
        while outstanding:
            e, ff, rr = outstanding.pop(0)
            got = eng.wait()
            assert np.array_equal(got, e), (ff, np.nonzero(got != e)[0][:10])
            assert all(eng.host_unregister(x) for x in rr)
    finally:
        eng.set_chunk_rows(0)


def test_in_place_column_over_two_registrations_is_copied(eng, orc):
    """a column that lies in two ADJACENT registered blocks -- pinned end to end, but by no single registration -- is copied into the staging set
    (lamd_info.last_flush_inplace_rows 0) and verifies like any other; the same rows in one registered block each stay in place"""
    import mmap
    rnd = random.Random(7171)
    n = 5000
    hs, sg, pk = _random_ecdsa(orc, rnd, n, 33)
    exp = orc.ecdsa_verify_batch(hs, sg, pk, 33, 8).astype(bool)
    pg = mmap.PAGESIZE
    half = (32 * n // 2 + pg - 1) // pg * pg                          # each block holds about half of the hash column
    m = mmap.mmap(-1, 2 * half)
    whole = np.frombuffer(m, dtype=np.uint8)
    lo, hi = whole[:half], whole[half:]
    regs = []
    assert eng.host_register(lo) and eng.host_register(hi), "hipHostRegister refused whole pages of host memory"
    try:
        start = half - 32 * (n // 2)                                    # the column's seam between the blocks falls after row n // 2
        col = whole[start:start + 32 * n].reshape(n, 32)
        col[:] = hs
        s2, k2 = _registered_block(eng, sg, regs), _registered_block(eng, pk, regs)
        assert eng.queue_ecdsa_batch_inplace(col, s2, k2) == 0
        eng.flush()
        assert eng.info()["last_flush_inplace_rows"] == 0
        got = eng.wait()
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
        h1 = _registered_block(eng, hs, regs)
        assert eng.queue_ecdsa_batch_inplace(h1, s2, k2) == 0
        eng.flush()
        assert eng.info()["last_flush_inplace_rows"] == n
        got = eng.wait()
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    finally:
        assert all(eng.host_unregister(x) for x in regs + [lo, hi])


def test_key_table_cache_warm_cold_and_bounded(orc):
    """the key-table cache: a second call over the same keys builds no table and verifies every row from cached combs (same
    verdicts); keys that do not parse are cached as such; a cache too small for the traffic empties itself and carries on;
    LAMD_CACHE=0 (tables live for one call) gives the same verdicts"""
    import os
    from lightning_amd import Engine, workload
    with Engine(0) as e:
        w = workload.make_ecdsa(e, 60000, seed=5151, nkeys=4000, publen=33)          # 15 rows per key: 7-tooth combs
        s = workload.make_schnorr(e, 40000, seed=5252, nkeys=300)                    # 133 rows per key: 10-tooth combs
        for rep in range(3):
            w.d_ok.fill_(9); s.d_ok.fill_(9)
            torch.cuda.synchronize()
            e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
            e.synchronize()
            ie = e.info()
            e.verify_schnorr_device(s.dev[0], s.dev[1], s.dev[2], s.d_ok)
            e.synchronize()
            isch = e.info()
            assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect), rep
            assert np.array_equal(strict_bool(s.d_ok.cpu().numpy()), s.expect), rep
            if rep == 0:
                assert ie["last_cache_hits"] == 0 and ie["last_new_tables"] > 3500 and ie["last_keyed"] == 7
                assert isch["last_new_tables"] >= 290 and isch["last_keyed"] == 10
                cold_rows = ie["last_cold_rows"]
            elif rep == 2:   # by now the host has seen the publishing calls complete: every table comes from the cache
                assert ie["last_new_tables"] == 0 and ie["last_cache_hits"] >= 60000 - cold_rows - 100 and ie["last_keyed"] == 7
                assert isch["last_new_tables"] == 0 and isch["last_cache_hits"] > 39000 and isch["last_keyed"] == 10
        assert e.info()["cache_enabled"] and e.info()["cache_resets"] == 0
        # a small batch under a cached key rides the cached comb (a commitment's 483 HTLC signatures on a known key)
        k = s.cols[1][0]
        sel = np.nonzero((s.cols[1] == k).all(axis=1))[0][:100]
        got = e.verify_schnorr(s.cols[0][sel], s.cols[1][sel], s.cols[2][sel])
        assert np.array_equal(got, s.expect[sel]) and e.info()["last_cache_hits"] == len(sel)
        # oracle pin on a sample of the cached-path verdicts
        exp = orc.ecdsa_verify_batch(w.cols[0][:1500], w.cols[1][:1500], w.cols[2][:1500], 33, 4).astype(bool)
        assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()[:1500]), exp)
        e.cache_clear()
        e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
        e.synchronize()
        assert e.info()["last_cache_hits"] == 0 and e.info()["cache_resets"] == 1
    os.environ["LAMD_CACHE_KEYS"] = "600"
    os.environ["LAMD_CACHE_KEYS10"] = "40"
    try:
        with Engine(0) as e:
            for rep in range(6):   # 4000 + 300 keys per round through a cache of 640: fills, falls back to the ladder, empties itself
                w = workload.make_ecdsa(e, 30000, seed=6000 + rep, nkeys=2000, publen=65)
                s = workload.make_schnorr(e, 20000, seed=6100 + rep, nkeys=150)
                e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
                e.verify_schnorr_device(s.dev[0], s.dev[1], s.dev[2], s.d_ok)
                e.synchronize()
                assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect), rep
                assert np.array_equal(strict_bool(s.d_ok.cpu().numpy()), s.expect), rep
            assert e.info()["cache_resets"] >= 1 and e.info()["cache_capacity"] == 640
    finally:
        del os.environ["LAMD_CACHE_KEYS"], os.environ["LAMD_CACHE_KEYS10"]
    os.environ["LAMD_CACHE"] = "0"
    try:
        with Engine(0) as e:
            w = workload.make_ecdsa(e, 50000, seed=5151, nkeys=3000, publen=33)
            for rep in range(2):
                e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
                e.synchronize()
                assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect)
                assert not e.info()["cache_enabled"] and e.info()["last_cache_hits"] == 0 and e.info()["last_new_tables"] > 2500
    finally:
        del os.environ["LAMD_CACHE"]


def test_keyed_fast_path_degenerate_rows_take_the_complete_formulas(eng_keyed, kat):
    """golden rows built so that an addition inside the comb meets +-its operand, or the result is the point at infinity
    (u1*G = -u2*Q), leave Z = 0 in the bare-formula kernel: they must be re-decided by the complete formulas, not guessed"""
    e = eng_keyed
    for publen, tags in ((65, ("u1G==u2Q", "R=inf")), (33, ("Q=G", "Q=lamG"))):
        vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 2 * publen and any(t in v["name"] for t in tags)]
        assert len(vs) >= 6
        # the same rows ONCE: <= 64 rows from host memory take the fused latency path (k_small_verify: complete formulas throughout)
        one = e.verify_ecdsa(_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64), _rows([H(v["pub"]) for v in vs], publen))
        assert [bool(g) for g in one] == [v["expect"] for v in vs]
        reps = 16                                   # each key several times, more than 64 rows: forced onto per-key tables (LAMD_KEYED=1)
        hs = _rows([H(v["hash"]) for v in vs] * reps, 32)
        sg = _rows([H(v["sig"]) for v in vs] * reps, 64)
        pk = _rows([H(v["pub"]) for v in vs] * reps, publen)
        got = e.verify_ecdsa(hs, sg, pk)
        assert [bool(g) for g in got] == [v["expect"] for v in vs] * reps
        if publen == 65:
            # u1*G + u2*Q = infinity, or the last addition is a doubling: Z = 0 in the bare formulas
            inf = e.info()
            assert inf["last_hot_rows"] > 0 and inf["last_suspect_rows"] >= 4 * reps, inf


@pytest.mark.parametrize("teeth", [7, 10])
def test_pairs_first_kernel_goldens_and_degenerate_rows(kat, teeth):
    """k_ecmult_keyed_pairs (LAMD_PAIRS=1: affine pair sums sharing one inversion per lane and batch of rows -- an experiment knob, kept
    parity-green): every ECDSA golden (reference KATs, every edge class, special keys) and every BIP-340 golden, each row repeated so
    that its key gets a comb table of the forced shape and a lane's batch holds several rows; the rows whose sums degenerate
    (u1*G = +-u2*Q, R = infinity, Q = G, Q = lambda*G) must come back from the complete formulas"""
    import os
    from lightning_amd import Engine
    env = {"LAMD_PAIRS": "1", "LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(teeth), "LAMD_CACHE": "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        suspects = 0
        for publen in (33, 65):
            vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 2 * publen]
            reps = (40000 + len(vs) - 1) // len(vs)
            got = e.verify_ecdsa(_rows([H(v["hash"]) for v in vs] * reps, 32), _rows([H(v["sig"]) for v in vs] * reps, 64), _rows([H(v["pub"]) for v in vs] * reps, publen))
            bad = sorted({v["name"] for v, g in zip(vs * reps, got) if bool(g) != v["expect"]})
            assert not bad, (publen, bad[:10])
            inf = e.info()
            assert inf["last_keyed"] == teeth and inf["last_hot_rows"] > 0.3 * len(got), inf   # (many goldens are decided before the ecmult: bad scalars, keys that do not parse)
            suspects += inf["last_suspect_rows"]
        assert suspects > 0
        vs = kat["schnorr"]
        reps = (40000 + len(vs) - 1) // len(vs)
        got = e.verify_schnorr(_rows([H(v["msg"]) for v in vs] * reps, 32), _rows([H(v["pk"]) for v in vs] * reps, 32), _rows([H(v["sig"]) for v in vs] * reps, 64))
        bad = sorted({v["name"] for v, g in zip(vs * reps, got) if bool(g) != v["expect"]})
        assert not bad, bad[:10]
    finally:
        e.close()


def test_check_tx_sig_from_transaction_templates_vs_spec_model(eng, orc):
    """check_tx_sig with the BIP143 hash built on the device (lamd_check_tx_sig_tx_batch): random transaction templates signed
    with the oracle's signer over pyref's sighash; a third of the rows damaged (amount, script byte, output, sequence, wrong
    input, sighash type outside the gate); verdicts against pyref sighash + oracle verify"""
    rnd = random.Random(1430)
    txs, sigs, pubs, exp = [], [], [], []
    keys = [(bytes(rnd.randrange(1, 256) for _ in range(32))) for _ in range(12)]
    pubs33 = [pyref.ser33(pyref.pubkey_create(int.from_bytes(d, "big"))) for d in keys]
    for it in range(3000):
        n_in, n_out = rnd.choice([1, 1, 2, 4]), rnd.choice([1, 1, 2, 3])
        inputs = [(bytes(rnd.randrange(256) for _ in range(32)), rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(n_in)]
        outputs = [(rnd.randrange(1 << 40), bytes(rnd.randrange(256) for _ in range(rnd.choice([22, 34, 34, 43])))) for _ in range(n_out)]
        script = bytes(rnd.randrange(256) for _ in range(rnd.choice([25, 71, 133, 133, 260])))
        t = dict(version=2, locktime=rnd.randrange(1 << 32), inputs=inputs, outputs=outputs, input_num=rnd.randrange(n_in),
                 amount=rnd.randrange(1 << 44), script=script, sighash_type=rnd.choice([1, 1, 1, 0x83]), has_witness=True)
        k = rnd.randrange(len(keys))
        h = pyref.bip143_sighash(2, inputs, outputs, t["locktime"], t["input_num"], script, t["amount"], t["sighash_type"])[0]
        sig = orc.ecdsa_sign(h, keys[k], bytes(rnd.randrange(1, 256) for _ in range(32)))
        dmg = rnd.randrange(18)
        if dmg == 0:
            t["amount"] ^= 1
        elif dmg == 1:
            t["script"] = script[:-1] + bytes([script[-1] ^ 4])
        elif dmg == 2:
            t["outputs"] = [(outputs[0][0] + 1, outputs[0][1])] + outputs[1:]
        elif dmg == 3:
            t["inputs"] = [(inputs[0][0], inputs[0][1], inputs[0][2] ^ 1)] + inputs[1:]
        elif dmg == 4 and n_in > 1:
            t["input_num"] = (t["input_num"] + 1) % n_in
        elif dmg == 5:
            t["sighash_type"] = rnd.choice([2, 3, 0x81, 0x82, 0])          # outside the gate: rejected whatever the signature
        elif dmg == 6:
            t["has_witness"] = False                                       # SINGLE|ANYONECANPAY needs a witness script; ALL does not
        h2 = pyref.bip143_sighash(2, t["inputs"], t["outputs"], t["locktime"], t["input_num"], t["script"], t["amount"], t["sighash_type"])[0]
        gate = t["sighash_type"] == 1 or (t["sighash_type"] == 0x83 and t["has_witness"])
        txs.append(t); sigs.append(sig); pubs.append(pubs33[k])
        exp.append(bool(gate and orc.ecdsa_verify(h2, sig, pubs33[k])))
    got = eng.check_tx_sig_tx_batch(txs, _rows(sigs, 64), _rows(pubs, 33))
    assert [bool(g) for g in got] == exp
    assert 1500 < sum(exp) < 2900


@pytest.mark.gpu
def test_ladder_whole_waves_of_degenerate_rows(eng, orc):
    """The per-signature ladder's hot form (bare additions, one Z == 0 test) hands a lane to the complete ladder when the test fires.  The goldens hold
    a handful of such rows; here whole waves of them, every row under its own never-seen key: z = -r*d (u1*G + u2*Q is the point at infinity:
    reject), z = r*d with s = 2*r*d/k (u1*G == u2*Q, the last addition is a doubling: accept), and honest rows between them.  Verdicts by
    construction, by the C oracle, and from the device -- through the batch path (ladder kernel) and, 64 rows at a time, the latency path"""
    rnd = random.Random(4242)
    N_ = pyref.N
    hs, sigs, pubs, exp = [], [], [], []
    for i in range(3 * 4096):
        d = rnd.randrange(1, N_)
        pub = orc.pubkey_create(d.to_bytes(32, "big"))
        kind = i % 3
        if kind == 0:      # R = infinity
            r, s_ = rnd.randrange(1, N_), rnd.randrange(1, N_ // 2)
            z, ok = (-r * d) % N_, False
        elif kind == 1:    # u1*G == u2*Q
            kk = rnd.randrange(1, N_)
            r = int.from_bytes(orc.pubkey_create(kk.to_bytes(32, "big"))[1:33], "big") % N_
            s_ = 2 * r * d * pow(kk, -1, N_) % N_
            if s_ > N_ // 2:
                s_ = N_ - s_
            z, ok = r * d % N_, True
        else:
            z = rnd.randrange(1 << 256)
            sg = orc.ecdsa_sign(z.to_bytes(32, "big"), d.to_bytes(32, "big"), rnd.randrange(1, N_).to_bytes(32, "big"))
            r, s_, ok = int.from_bytes(sg[:32], "big"), int.from_bytes(sg[32:], "big"), True
            z %= 1 << 256
        hs.append((z % (1 << 256)).to_bytes(32, "big")); sigs.append(r.to_bytes(32, "big") + s_.to_bytes(32, "big")); pubs.append(pub); exp.append(ok)
    h, sg, pk = _rows(hs, 32), _rows(sigs, 64), _rows(pubs, 65)
    want = np.array(exp)
    assert (np.asarray(orc.ecdsa_verify_batch(h, sg, pk, 65, 8)).astype(bool) == want).all()        # the construction is what the oracle sees
    got = np.asarray(eng.verify_ecdsa(h, sg, pk)).astype(bool)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    for o in range(0, 640, 64):                                                                      # the latency path's ladder (complete formulas)
        assert (np.asarray(eng.verify_ecdsa(h[o:o + 64], sg[o:o + 64], pk[o:o + 64])).astype(bool) == want[o:o + 64]).all()


@pytest.mark.gpu
def test_check_tx_sig_templates_at_the_stream_boundaries(eng, orc):
    """The device's BIP143 form lays each of a row's four SHA-256 streams out in a per-lane buffer of 960 bytes (k_txsig_tx_hash): every script
    length 0 .. 140 (each padding case of the preimage), the CompactSize steps (252 / 253 / 254), input and output lists up to and across the
    limits behind which txsig_pack hashes the row on the host (25 inputs, 900 bytes of outputs, a 700-byte script), no outputs at all,
    SIGHASH_SINGLE|ANYONECANPAY on an input with and without its output.  Every row carries a VALID signature over pyref's sighash, so a
    single wrong byte in any stream shows; every seventh row is damaged after signing."""
    rnd = random.Random(5150)
    rb = lambda k: bytes(rnd.randrange(256) for _ in range(k))
    keys = [bytes(rnd.randrange(1, 256) for _ in range(32)) for _ in range(5)]
    pubs33 = [pyref.ser33(pyref.pubkey_create(int.from_bytes(d, "big"))) for d in keys]
    shapes = [(1, 1, sl) for sl in range(0, 141)]
    shapes += [(1, 1, sl) for sl in (251, 252, 253, 254, 255, 256, 300, 511, 698, 699, 700, 701, 702, 786, 787, 900, 1500)]
    shapes += [(ni, 1, 133) for ni in (2, 3, 7, 24, 25, 26, 27, 30, 60)]
    shapes += [(1, no, 133) for no in (0, 2, 5, 19, 20, 21, 22, 23, 40)]        # 43 bytes each: 20 = 860, 21 = 903 bytes
    shapes += [(rnd.randrange(1, 27), rnd.randrange(0, 23), rnd.randrange(0, 720)) for _ in range(120)]
    txs, sigs, pubs, exp = [], [], [], []
    for it, (n_in, n_out, sl) in enumerate(shapes * 2):
        ty = 1 if it < len(shapes) else 0x83
        inputs = [(rb(32), rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(n_in)]
        outputs = [(rnd.randrange(1 << 40), rb(34)) for _ in range(n_out)]
        t = dict(version=2, locktime=rnd.randrange(1 << 32), inputs=inputs, outputs=outputs, input_num=rnd.randrange(n_in), amount=rnd.randrange(1 << 44),
                 script=rb(sl), sighash_type=ty, has_witness=True)
        k = it % len(keys)
        h = pyref.bip143_sighash(2, inputs, outputs, t["locktime"], t["input_num"], t["script"], t["amount"], ty)[0]
        sig = orc.ecdsa_sign(h, keys[k], bytes(rnd.randrange(1, 256) for _ in range(32)))
        if it % 7 == 3:
            what = rnd.randrange(4)
            if what == 0 and sl:
                j = rnd.randrange(sl)
                t["script"] = t["script"][:j] + bytes([t["script"][j] ^ 0x10]) + t["script"][j + 1:]
            elif what == 1 and n_out:
                j = rnd.randrange(n_out)
                t["outputs"] = outputs[:j] + [(outputs[j][0] ^ 1, outputs[j][1])] + outputs[j + 1:]
            elif what == 2:
                j = rnd.randrange(n_in)
                t["inputs"] = inputs[:j] + [(inputs[j][0], inputs[j][1] ^ 1, inputs[j][2])] + inputs[j + 1:]
            else:
                t["locktime"] ^= 1 << rnd.randrange(32)
        h2 = pyref.bip143_sighash(2, t["inputs"], t["outputs"], t["locktime"], t["input_num"], t["script"], t["amount"], ty)[0]
        txs.append(t); sigs.append(sig); pubs.append(pubs33[k])
        exp.append(bool(orc.ecdsa_verify(h2, sig, pubs33[k])))
    assert 17 < len(txs) <= 4096                       # the two-launch path (txsig_small_device)
    got = eng.check_tx_sig_tx_batch(txs, _rows(sigs, 64), _rows(pubs, 33))
    bad = [(i, shapes[i % len(shapes)], txs[i]["sighash_type"]) for i in range(len(txs)) if bool(got[i]) != exp[i]]
    assert not bad, bad[:10]
    assert sum(exp) > 0.8 * len(exp)
    # the same rows through the batch machinery (more than 4096 rows in one call)
    reps = 4096 // len(txs) + 1
    got = eng.check_tx_sig_tx_batch(txs * reps, np.tile(_rows(sigs, 64), (reps, 1)), np.tile(_rows(pubs, 33), (reps, 1)))
    assert [bool(g) for g in got] == exp * reps


@pytest.mark.gpu
def test_bolt12_reference_held_strings_on_device(eng, kat):
    """The lni1 / lnr1 literals of the reference tree (tests/test_misc.py:5254, tests/test_pay.py:7183, tests/test_xpay.py:788,
    doc/schemas -- signed by the reference's libsecp256k1; kat.json "bolt12"): lamd_bolt12_check_signature_batch must accept every
    one, reject their one-bit twins and the fuzz corpus' damaged streams; the sighash the device derives is the recorded one; and
    the derived (sighash, x-only key, signature) triples agree through lamd_verify_schnorr_batch"""
    rows = kat["bolt12"]
    assert sum(1 for v in rows if v["expect"]) >= 9
    for mn in (b"invoice", b"invoice_request"):
        grp = [v for v in rows if v["messagename"].encode() == mn]
        assert grp
        streams = [H(v["stream"]) for v in grp]
        got = eng.bolt12_check_signature_batch(streams, mn, b"signature", _rows([H(v["key"]) for v in grp], 33), _rows([H(v["sig"]) for v in grp], 64))
        bad = [v["name"] for v, g in zip(grp, got) if bool(g) != v["expect"]]
        assert not bad, bad
        mk, sh, ok = eng.bolt12_merkle_batch(streams, mn, b"signature")
        for i, v in enumerate(grp):
            fields = pyref.tlv_stream_parse(streams[i])
            m = pyref.bolt12_merkle(fields) if fields is not None else None
            assert bool(ok[i]) == (m is not None), v["name"]
            if m is not None:
                assert bytes(mk[i]) == m and bytes(sh[i]) == pyref.bolt12_sighash(mn, b"signature", m), v["name"]
                if v["sighash"] is not None and "flip-field" not in v["name"]:
                    assert bytes(sh[i]).hex() == v["sighash"]
    tri = [v for v in kat["schnorr"] if v["name"].startswith("bolt12/")]
    assert sum(1 for v in tri if v["expect"]) >= 9
    got = eng.verify_schnorr(_rows([H(v["msg"]) for v in tri], 32), _rows([H(v["pk"]) for v in tri], 32), _rows([H(v["sig"]) for v in tri], 64))
    assert [bool(g) for g in got] == [v["expect"] for v in tri]


@pytest.mark.gpu
def test_bolt12_signatures_device_front_end_vs_spec_model(eng):
    """BOLT #12 (rest of N4): merkle_tlv + sighash_from_merkle + check_schnorr_sig on the device (lamd_bolt12_check_signature_batch)
    -- the specification's n1 roots, the invoice_request of common/test/run-bolt12_merkle.c:332-361 (Alice 0x41.., Bob 0x42.. signs),
    and 1 500 random streams signed with the model's BIP-340 signer, a third damaged (value byte, type, signature, key, tag,
    a signature field's content -- which must NOT matter --, a stream that breaks the TLV rules)"""
    def tlv(t, v):
        return pyref.bigsize(t) + pyref.bigsize(len(v)) + v
    n1 = [(1, (1000).to_bytes(2, "big")), (2, ((1 << 40) | (2 << 16) | 3).to_bytes(8, "big")),
          (3, H("0266e4598d1d3c415f572a8488830b60f7e744ed9235eb0b1ba93283b315c03518") + (1).to_bytes(8, "big") + (2).to_bytes(8, "big"))]
    streams = [b"".join(tlv(t, v) for t, v in n1[:k]) for k in (1, 2, 3)]
    mk, sh, ok = eng.bolt12_merkle_batch(streams, b"invoice_request", b"signature")
    assert ok.all() and [bytes(r).hex() for r in mk] == ["b013756c8fee86503a0b4abdab4cddeb1af5d344ca6fc2fa8b6c08938caa6f93",
                                                         "c3774abbf4815aa54ccaa026bff6581f01f3be5fe814c620a252534f434bc0d1",
                                                         "ab2e79b1283b0b31e0b035258de23782df6b89a38cfa7237bde69aed1a658c5d"]
    assert all(bytes(sh[i]) == pyref.bolt12_sighash(b"invoice_request", b"signature", bytes(mk[i])) for i in range(3))
    # the reference test's invoice_request
    alice, bob = pyref.pubkey_create(int.from_bytes(b"A" * 32, "big")), pyref.pubkey_create(int.from_bytes(b"B" * 32, "big"))
    fields = [(0, bytes(8)), (6, b"USD"), (8, b"\x64"), (10, b"A Mathematical Treatise"), (22, pyref.ser33(alice)), (88, pyref.ser33(bob))]
    root = pyref.bolt12_merkle(fields)
    sig = pyref.schnorr_sign(pyref.bolt12_sighash(b"invoice_request", b"signature", root), int.from_bytes(b"B" * 32, "big"))
    st = b"".join(tlv(t, v) for t, v in fields) + tlv(240, sig)
    assert len(pyref.tlv_stream_parse(st)) == 7                     # as the reference asserts (:363)
    got = eng.bolt12_check_signature_batch([st, st, st], b"invoice_request", b"signature", _rows([pyref.ser33(bob), pyref.ser33(alice), pyref.ser33(bob)], 33),
                                           _rows([sig, sig, sig[:63] + bytes([sig[63] ^ 1])], 64))
    assert list(got) == [True, False, False]
    assert not eng.bolt12_check_signature_batch([st], b"invoice", b"signature", _rows([pyref.ser33(bob)], 33), _rows([sig], 64))[0]   # the tag is signed too
    rnd = random.Random(1240)
    keys = [rnd.randrange(1, pyref.N) for _ in range(9)]
    pubs = [pyref.ser33(pyref.pubkey_create(d)) for d in keys]
    streams, ks, sigs, exp = [], [], [], []
    for it in range(1500):
        nf = rnd.choice([1, 2, 3, 5, 6, 7, 8, 12, 17, 40])
        types = sorted(rnd.sample(list(range(0, 240)) + list(range(1001, 1060)) + [0x10000, 1 << 33], nf))
        fields = [(t, bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 1, 8, 33, 100, 253, 300])))) for t in types]
        k = rnd.randrange(len(keys))
        sig = pyref.schnorr_sign(pyref.bolt12_sighash(b"invoice", b"signature", pyref.bolt12_merkle(fields)), keys[k], bytes(rnd.randrange(256) for _ in range(32)))
        sigfield = (240, sig)
        key = pubs[k]
        dmg = rnd.randrange(21)
        if dmg == 0 and fields[0][1]:
            fields[0] = (fields[0][0], bytes([fields[0][1][0] ^ 1]) + fields[0][1][1:])
        elif dmg == 1:
            fields[-1] = (fields[-1][0] + 2, fields[-1][1])
        elif dmg == 2:
            sig = sig[:40] + bytes([sig[40] ^ 0x20]) + sig[41:]
        elif dmg == 3:
            key = pubs[(k + 1) % len(pubs)]
        elif dmg == 4:
            sigfield = (240, bytes(64))                       # the signature FIELD is no leaf: its content does not matter
        elif dmg == 5:
            key = bytes([key[0] ^ 1]) + key[1:]               # the parity byte is dropped: still valid
        allf = sorted(fields + [sigfield])
        st = b"".join(tlv(t, v) for t, v in allf)
        if dmg == 6:
            st = st[:-1]                                      # truncated: fromwire_tlv fails
        elif dmg == 7 and len(fields) > 1:
            st = tlv(*fields[1]) + tlv(*fields[0])            # not ascending
        streams.append(st); ks.append(key); sigs.append(sig)
        exp.append(pyref.bolt12_check_signature(st, b"invoice", b"signature", key, sig))
    got = eng.bolt12_check_signature_batch(streams, b"invoice", b"signature", _rows(ks, 33), _rows(sigs, 64))
    assert [bool(g) for g in got] == exp
    assert 1000 < sum(exp) < 1450


@pytest.mark.gpu
def test_single_calls_learn_a_recurring_key(orc):
    """one check_signed_hash()-sized call at a time (the fused launch k_small_verify): a key the cache does not know is verified by
    the ladder the first time, gets its comb table built and published the second time it shows up, and is a cache hit from the
    third call on; verdicts equal the oracle's throughout, for valid and damaged rows, ECDSA and BIP-340"""
    from lightning_amd import Engine, workload
    with Engine(0) as e:
        w = workload.make_ecdsa(e, 64, seed=9091, nkeys=1, publen=33, invalid_frac=0.25)     # ONE key, 64 signatures
        s = workload.make_schnorr(e, 64, seed=9092, nkeys=1, invalid_frac=0.25)
        for wl, fn, ref in ((w, e.verify_ecdsa, lambda c: orc.ecdsa_verify_batch(c[0], c[1], c[2], 33, 1)), (s, e.verify_schnorr, lambda c: orc.schnorr_verify_batch(c[0], c[1], c[2], 1))):
            seen = []
            for call in range(6):
                cols = [np.ascontiguousarray(c[call:call + 1]) for c in wl.cols]
                got = fn(*cols)
                assert bool(got[0]) == bool(wl.expect[call]) == bool(ref(cols)[0]), call
                inf = e.info()
                seen.append((inf["last_cache_hits"], inf["last_cold_rows"], inf["last_new_tables"]))
            assert seen[0] == (0, 1, 0), seen            # first sight: the ladder
            assert seen[1][2] == 1, seen                 # second sight: the table is built and published
            assert all(x == (1, 0, 0) for x in seen[2:]), seen   # afterwards: a cache hit in the fused launch
        # a batch of unknown keys next to a learnt one: verdicts stay exact while the fingerprints accumulate
        f = workload.make_ecdsa(e, 40, seed=9093, nkeys=1 << 40, publen=65, group=1, invalid_frac=0.2)
        for rep in range(3):
            got = e.verify_ecdsa(*f.cols)
            assert np.array_equal(got, f.expect) and np.array_equal(got, orc.ecdsa_verify_batch(f.cols[0], f.cols[1], f.cols[2], 65, 1).astype(bool)), rep


@pytest.mark.gpu
def test_one_launch_path_block_boundaries_and_mixed_shapes(orc):
    """calls of 1 .. 4096 rows are ONE launch (k_small_verify as a grid of 64-row blocks), 4097 rows take the general path: sizes around the
    block and path boundaries, every wave holding rows under 7-tooth keys, 10-tooth keys, keys without a table, keys that do not parse and
    damaged signatures side by side (the run-time comb body for mixed waves); ECDSA (33- and 65-byte keys) and BIP-340; every verdict
    against the C oracle"""
    from lightning_amd import Engine, workload
    with Engine(0) as e:
        for publen in (33, 65):
            a = workload.make_ecdsa(e, 30000, seed=5101 + publen, nkeys=2000, publen=publen)          # 15 rows per key: 7-tooth combs
            b = workload.make_ecdsa(e, 30000, seed=5102 + publen, nkeys=100, publen=publen)           # 300 rows per key: 10-tooth combs
            c = workload.make_ecdsa(e, 20000, seed=5103 + publen, nkeys=1 << 40, publen=publen, group=1)  # every row its own key (never met twice here): ladder
            for w in (a, b):
                for _ in range(2):                                                                    # second call: the host has seen the tables published
                    e.verify_ecdsa_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
                    e.synchronize()
                assert np.array_equal(strict_bool(w.d_ok.cpu().numpy()), w.expect)
            rng = np.random.default_rng(77 + publen)
            o = 0
            for n in (1, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 4097):
                src = rng.integers(0, 3, n)
                src[rng.integers(0, n)] = 2 if n < 4000 else 0                 # (at most a handful of ladder rows in the big calls: they are 0.9 ms each wave)
                if n >= 4000:
                    src[src == 2] = rng.integers(0, 2, int((src == 2).sum()))
                    src[:3] = 2
                idx = [rng.integers(0, 30000, n), rng.integers(0, 30000, n), (o + np.arange(n)) % 20000]
                o += n
                cols = [np.ascontiguousarray(np.where((src == 0)[:, None], a.cols[k][idx[0]], np.where((src == 1)[:, None], b.cols[k][idx[1]], c.cols[k][idx[2]]))) for k in range(3)]
                exp = np.where(src == 0, a.expect[idx[0]], np.where(src == 1, b.expect[idx[1]], c.expect[idx[2]]))
                got = e.verify_ecdsa(*cols)
                assert np.array_equal(got, exp), (publen, n)
                assert np.array_equal(got, orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], publen, 4).astype(bool)), (publen, n)
        s7 = workload.make_schnorr(e, 30000, seed=5201, nkeys=2000)
        s10 = workload.make_schnorr(e, 30000, seed=5202, nkeys=100)
        for w in (s7, s10):
            for _ in range(2):
                e.verify_schnorr_device(w.dev[0], w.dev[1], w.dev[2], w.d_ok)
                e.synchronize()
        rng = np.random.default_rng(99)
        for n in (1, 64, 65, 500, 4096):
            src = rng.integers(0, 2, n)
            idx = rng.integers(0, 30000, n)
            cols = [np.ascontiguousarray(np.where((src == 0)[:, None], s7.cols[k][idx], s10.cols[k][idx])) for k in range(3)]
            exp = np.where(src == 0, s7.expect[idx], s10.expect[idx])
            got = e.verify_schnorr(*cols)
            assert np.array_equal(got, exp), n
            assert np.array_equal(got, orc.schnorr_verify_batch(cols[0], cols[1], cols[2], 4).astype(bool)), n


@pytest.mark.gpu
def test_small_batches_with_a_cache_take_the_lookup_path(kat, orc):
    """small batches on an engine with the key-table cache: ONE kernel probes the cache and runs the cached comb or, on a miss, the
    ladder (k_ecmult_small).  Hits, misses, unparsable keys and damaged signatures in one batch; a commitment-shaped batch under a
    NEW key is verified by the ladder first, makes the next call build and publish the table, and hits from the third call on;
    degenerate rows under a cached key fall back to the complete formulas inside the kernel; BIP-340 the same way."""
    from lightning_amd import Engine, workload
    with Engine(0) as e:
        assert e.info()["cache_enabled"]
        big = workload.make_ecdsa(e, 40000, seed=777, nkeys=600, publen=33)           # 66 rows per key: cached combs
        e.verify_ecdsa_device(big.dev[0], big.dev[1], big.dev[2], big.d_ok)
        e.synchronize()
        assert np.array_equal(strict_bool(big.d_ok.cpu().numpy()), big.expect) and e.info()["last_new_tables"] > 500
        e.verify_ecdsa_device(big.dev[0], big.dev[1], big.dev[2], big.d_ok)           # the host has now seen the publishing call complete
        e.synchronize()
        fresh = workload.make_ecdsa(e, 4000, seed=778, nkeys=1 << 40, publen=33, group=1)      # keys the cache has never seen, every row its own
        o = 0
        for n in (1, 7, 32, 65, 484, 3000):
            sel, fsel = np.arange(n), np.arange(o, o + n)     # fresh keys never recur here (a recurring one would be learnt: test_single_calls_learn_a_recurring_key)
            o += n
            hs = np.concatenate([big.cols[0][sel], fresh.cols[0][fsel]]); sg = np.concatenate([big.cols[1][sel], fresh.cols[1][fsel]])
            pk = np.concatenate([big.cols[2][sel], fresh.cols[2][fsel]])
            exp = np.concatenate([big.expect[sel], fresh.expect[fsel]])
            got = e.verify_ecdsa(hs, sg, pk)
            assert np.array_equal(got, exp), n
            assert np.array_equal(got, orc.ecdsa_verify_batch(hs, sg, pk, 33, 2).astype(bool))
            inf = e.info()
            assert inf["last_cache_hits"] >= int(0.9 * n) and inf["last_new_tables"] == 0 and inf["last_cold_rows"] >= int(0.9 * n), (n, inf)
        # a commitment under a new htlc key: ladder, then the table-building path, then cache hits
        st = workload.make_commit_storm(e, 4, seed=4242)["ecdsa"]
        hh, ss, pp = [np.ascontiguousarray(x[484:968]) for x in st.cols]
        seen = []
        for call in range(4):
            got = e.verify_ecdsa(hh, ss, pp)
            assert np.array_equal(got, st.expect[484:968]), call
            inf = e.info()
            seen.append((inf["last_cache_hits"], inf["last_new_tables"]))
        assert seen[0] == (0, 0) and seen[1][1] == 2 and seen[2][0] == 484 and seen[3][0] == 484, seen      # the htlc key AND the funding key get tables
        # degenerate rows (Z = 0 in the bare formulas) under cached keys
        vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 130 and any(t in v["name"] for t in ("u1G==u2Q", "R=inf"))]
        assert len(vs) >= 6
        reps = 9000 // len(vs) + 1
        hs, sg, pk = _rows([H(v["hash"]) for v in vs] * reps, 32), _rows([H(v["sig"]) for v in vs] * reps, 64), _rows([H(v["pub"]) for v in vs] * reps, 65)
        assert [bool(g) for g in e.verify_ecdsa(hs, sg, pk)] == [v["expect"] for v in vs] * reps      # big: tables built and published
        e.verify_ecdsa(hs, sg, pk)
        got = e.verify_ecdsa(hs[:len(vs)], sg[:len(vs)], pk[:len(vs)])
        assert [bool(g) for g in got] == [v["expect"] for v in vs] and e.info()["last_cache_hits"] == len(vs)
        # BIP-340
        sb = workload.make_schnorr(e, 30000, seed=779, nkeys=200)
        e.verify_schnorr_device(sb.dev[0], sb.dev[1], sb.dev[2], sb.d_ok); e.synchronize()
        e.verify_schnorr_device(sb.dev[0], sb.dev[1], sb.dev[2], sb.d_ok); e.synchronize()
        sf = workload.make_schnorr(e, 500, seed=780, nkeys=1 << 40)
        for n in (1, 100, 500):
            ms = np.concatenate([sb.cols[0][:n], sf.cols[0][:n]]); ks = np.concatenate([sb.cols[1][:n], sf.cols[1][:n]]); ss2 = np.concatenate([sb.cols[2][:n], sf.cols[2][:n]])
            got = e.verify_schnorr(ms, ks, ss2)
            assert np.array_equal(got, np.concatenate([sb.expect[:n], sf.expect[:n]])), n
            assert np.array_equal(got, orc.schnorr_verify_batch(ms, ks, ss2, 2).astype(bool))
            assert e.info()["last_cache_hits"] >= int(0.9 * n)

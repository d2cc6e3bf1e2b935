"""Peers' reply_channel_range messages compared with the digest on the device (lamd_channel_range_compare_batch, lamd_store_digest_read_bare,
include/lightning_amd.h) against the sequential model of range_compare_model.py: every status, count, list and output byte, with no tolerance.  The
same code on the host, under the sanitizers, is test_store_compare_host's."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import range_compare_model as rcm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu
FAR = 1 << 63                                                                               # no store of these tests has a scid with this bit


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def compare_equals_model(eng, dg, entries, bare, msgs, want=None, mu=0, ms=0, chain=crm.CHAIN):
    """-> the model's (status, per_msg, unknown, stale, flags, messages), which the device must equal"""
    status, per_msg, unknown, stale, flags, out, s = eng.channel_range_compare(dg, chain, msgs, want=want, max_unknown=mu, max_stale=ms, return_summary=True)
    model = rcm.compare(entries, bare, chain, msgs, want, mu, ms)
    got = ([int(x) for x in status], [tuple(int(x) for x in r) for r in per_msg], [int(x) for x in unknown], [int(x) for x in stale], [int(x) for x in flags], out)
    for name, a, b in zip(("status", "per_msg", "unknown", "stale", "flags", "messages"), got, model):
        assert a == b, (name, len(a), len(b), a[:6], b[:6])
    st, pm = model[0], model[1]
    assert s["by_status"] == [st.count(0)] + [st.count(k) for k in range(1, 7)] + [st.count(-1)]
    assert (s["entries"], s["entries_unknown"], s["entries_stale"]) == tuple(sum(p[k] for p in pm) for k in range(3))
    n_u = -(-len(model[2]) // (mu or rcm.MAX_UNKNOWN))
    assert (s["unknown"], s["stale"], s["unknown_messages"], s["messages"], s["bytes"]) == (len(model[2]), len(model[3]), n_u, len(out), sum(len(m) for m in out))
    assert all(len(m) <= 65535 for m in out)
    return model


@pytest.fixture(scope="module")
def slots(eng):
    blob, names = crm.slot_store()
    entries, bare = crm.sorted_digest(blob)[0], rcm.bare(blob)
    with eng.gossip_store_digest(blob) as dg:
        yield dg, entries, bare, names


@pytest.fixture(scope="module")
def six_hundred(eng):
    """600 channels with an update in either direction"""
    blob = crm.channel_store([crm.scid_of(3000 + k // 2, k % 2, 1) for k in range(600)], both=True)
    entries = crm.sorted_digest(blob)[0]
    with eng.gossip_store_digest(blob) as dg:
        yield dg, entries


# ------------------------------------------------------------------------------------------------ 1. the bare list
def bare_equals_model(eng, blob, verdict=None):
    want = rcm.bare(blob, verdict)
    with eng.gossip_store_digest(blob, verdict=verdict) as dg:
        got = [int(x) for x in dg.read_bare()]
        assert got == want and got == sorted(got) and len(got) == dg.summary["channels_no_update"]
    return want


@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_bare_list_of_the_stores_the_reference_wrote(eng, name):
    assert bare_equals_model(eng, sa._golden(name)) == []


def test_bare_list_of_the_synthetic_store_its_damaged_copy_and_the_slot_store(eng, synthetic, damaged):
    img, (_, v, _) = synthetic
    assert bare_equals_model(eng, img) == bare_equals_model(eng, img, list(v))
    blob, (_, dv, _), _ = damaged
    strict, loose = bare_equals_model(eng, blob, list(dv)), bare_equals_model(eng, blob)
    assert set(loose) <= set(strict) | {e[0] for e in crm.digest(blob)[0]}
    sblob, names = crm.slot_store()
    assert bare_equals_model(eng, sblob) == [names["no_update"]]
    # several bare channels, written in descending order, between channels with updates
    recs = []
    for k in range(300):
        s = crm.scid_of(9000 - k, k % 3, 0)
        recs += [crm.fast_rec(crm.cann(s, k)), crm.fast_rec(crm.AMOUNT)] + ([crm.fast_rec(crm.cupd(s, k & 1, 5 + k))] if k % 3 else [])
    assert len(bare_equals_model(eng, sa.serialise(0x10, recs))) == 100


# ------------------------------------------------------------------------------------------------ 2. every branch
def one(eng, slots, scid, ts):
    dg, entries, bare, _ = slots
    return compare_equals_model(eng, dg, entries, bare, [rcm.reply(crm.CHAIN, 0, 1000, [scid], None if ts is None else [ts])])


def test_every_branch_of_the_classification(eng, slots):
    names = slots[3]
    by = {e[0]: e[1] for e in slots[1]}
    both, dir0 = names["both"], names["dir0"]
    assert by[both] == (14, 13) and by[dir0] == (11, 0)
    for scid, ts, unknown, stale, flags in ((both | FAR, (1, 1), [both | FAR], [], []),                  # unknown
                                            (both, (14, 13), [], [], []),                                  # known, equal
                                            (both, (15, 13), [], [both], [2]), (both, (14, 14), [], [both], [4]), (both, (15, 14), [], [both], [6]),
                                            (both, (13, 12), [], [], []), (both, (0, 0), [], [], []),      # the peer is older, or has none
                                            (dir0, (11, 0), [], [], []), (dir0, (11, 1), [], [dir0], [4]),  # our slot is unset: any timestamp of theirs is news
                                            (both, (0xFFFFFFFF, 0), [], [both], [2])):
        m = one(eng, slots, scid, ts)
        assert (m[2], m[3], m[4]) == (unknown, stale, flags), (hex(scid), ts)
        assert m[1] == [(1, len(unknown), len(stale))]


def test_a_channel_without_an_update_is_known(eng, slots):
    """fails where the comparison looks at the digest's entries alone: the bare list is what gossmap_find_chan finds beyond them"""
    s = slots[3]["no_update"]
    assert s in slots[2] and s not in {e[0] for e in slots[1]}
    m = one(eng, slots, s, (0, 0))
    assert (m[2], m[3], m[4]) == ([], [], []) and m[5] == []
    m = one(eng, slots, s, (5, 0))
    assert (m[2], m[3], m[4]) == ([], [s], [2])
    m = one(eng, slots, s, None)
    assert (m[2], m[3], m[4]) == ([], [], [])


def test_without_timestamps_nothing_known_is_stale(eng, slots):
    dg, entries, bare, names = slots
    known = [e[0] for e in entries] + bare
    msgs = [rcm.reply(crm.CHAIN, 0, 1000, sorted(known + [s | FAR for s in known[:50]]), None, None if k else [(9, 9)] * (len(known) + 50)) for k in range(2)]
    m = compare_equals_model(eng, dg, entries, bare, msgs)
    assert m[0] == [0, 0] and m[3] == [] and m[2] == sorted(s | FAR for s in known[:50]) and m[1] == [(len(known) + 50, 50, 0)] * 2
    everything = rcm.probe_replies(entries, bare)
    m = compare_equals_model(eng, dg, entries, bare, everything)
    assert set(m[4]) == {2, 4, 6} and names["no_update"] in m[3]


# ------------------------------------------------------------------------------------------------ 3. every status
def test_every_status_with_and_without_an_outstanding_query(eng, slots):
    dg, entries, bare, _ = slots
    cases = rcm.status_cases()
    plain = [c for c in cases if c[1] is None]
    m = compare_equals_model(eng, dg, entries, bare, [c[0] for c in plain])
    assert m[0] == [c[2] for c in plain]
    m = compare_equals_model(eng, dg, entries, bare, [c[0] for c in cases], want=[c[1] or (0, 0xFFFFFFFF) for c in cases])
    assert m[0] == [c[2] for c in cases] and set(m[0]) == {-1, 0, 1, 2, 3, 4, 5, 6}
    assert all(p == (0, 0, 0) for p, st in zip(m[1], m[0]) if st != 0) and len(m[2]) == 3      # the rejected ones' scids are all unknown, and are not listed
    rejected = [c[0] for c in cases if c[2] != 0]
    m = compare_equals_model(eng, dg, entries, bare, rejected, want=[c[1] or (0, 0xFFFFFFFF) for c in cases if c[2] != 0])
    assert 0 not in m[0] and m[2] == m[3] == m[5] == []


# ------------------------------------------------------------------------------------------------ 4. merging
def test_flags_are_ored_and_duplicates_are_listed_once(eng, slots):
    dg, entries, bare, names = slots
    both, u = names["both"], names["dir1"] | FAR
    R = lambda scids, ts: rcm.reply(crm.CHAIN, 0, 1000, scids, ts)
    msgs = [R([both, u], [(15, 13), (1, 1)]), R([u], [(0, 0)]), R([both, u], [(14, 14), (7, 7)]), R([u, both], [(3, 3), (14, 13)]), R([both], [(1, 1)])]
    for order in (msgs, msgs[::-1], msgs[2:] + msgs[:2]):
        m = compare_equals_model(eng, dg, entries, bare, order)
        assert (m[2], m[3], m[4]) == ([u], [both], [6])
        assert sorted(m[1]) == sorted([(2, 1, 1), (1, 1, 0), (2, 1, 1), (2, 1, 0), (1, 0, 0)])     # counted before merging
    assert len(m[5]) == 2 and len(m[5][0]) == 45 and len(m[5][1]) == 45 + 3 + 1


# ------------------------------------------------------------------------------------------------ 5. wave and block edges
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_block_edges(eng, six_hundred, total):
    dg, entries = six_hundred
    rows = []
    for e in range(total):
        w, lane = e // 64, e % 64
        kind = {0: "u", 1: "s", 2: "n", 3: "usn"[lane % 3], 4: "u" if lane == 17 else "s" if lane == 40 else "n", 5: "n" if lane == 63 else "u"}[w % 6]
        scid, (a, b) = entries[(7 * e) % 150][:2]                                    # beyond 150 entries scids repeat
        rows.append({"u": (scid | FAR, (e, e)), "s": (scid, (a + 1 + e % 2, b + e % 3)), "n": (scid, (a, b))}[kind])
    sizes, msgs, at = [1, 7, 64, 0, 100, 3, 129], [], 0
    while at < total:
        part = rows[at:at + sizes[len(msgs) % len(sizes)]]
        at += len(part)
        msgs.append(rcm.reply(crm.CHAIN, 0, 1 << 24, [r[0] for r in part], [r[1] for r in part]))
    m = compare_equals_model(eng, dg, entries, [], msgs)
    assert sum(p[0] for p in m[1]) == total and set(m[0]) == {0}
    if total >= 257:
        assert m[2] and m[3] and sum(p[2] for p in m[1]) > len(m[3])


# ------------------------------------------------------------------------------------------------ 6. chunking
def lists_of(entries, n_unknown, n_stale):
    """replies that leave exactly n_unknown unknown and n_stale stale scids"""
    scids = [e[0] | FAR for e in entries[:n_unknown]] + [e[0] for e in entries[:n_stale]]
    ts = [(0, 0)] * n_unknown + [(e[1][0] + 1 + k % 2, e[1][1] + k % 3) for k, e in enumerate(entries[:n_stale])]
    return [rcm.reply(crm.CHAIN, 0, 1 << 24, scids[a:a + 4000], ts[a:a + 4000]) for a in range(0, len(scids), 4000)]


@pytest.mark.parametrize("limit", [1, 2, 3, 7])
def test_chunks_at_small_limits(eng, six_hundred, limit):
    dg, entries = six_hundred
    sizes = [0, 1, limit - 1, limit, limit + 1, 3 * limit + 1]
    for k, n_u in enumerate(sizes):
        n_s = sizes[(k + 2) % len(sizes)]
        m = compare_equals_model(eng, dg, entries, [], lists_of(entries, n_u, n_s), mu=limit, ms=limit)
        assert (len(m[2]), len(m[3]), len(m[5])) == (n_u, n_s, -(-n_u // limit) - (-n_s // limit))
    m = compare_equals_model(eng, dg, entries, [], lists_of(entries, 3 * limit + 1, limit + 1), mu=limit, ms=7)       # the two limits are separate
    assert len(m[5]) == 4 + (2 if limit == 7 else 1)


@pytest.mark.parametrize("k", [251, 252, 253])
def test_the_flags_tlv_length_grows_to_three_bytes(eng, six_hundred, k):
    dg, entries = six_hundred
    m = compare_equals_model(eng, dg, entries, [], lists_of(entries, 0, k + 1), ms=k)
    assert [len(x) for x in m[5]] == [37 + 8 * k + 1 + (1 if k < 252 else 3) + 1 + k, 37 + 8 + 3 + 1]


def test_the_default_limits_and_their_bound(eng):
    from lightning_amd.engine import LamdError
    scids = [crm.scid_of(200000 + k, 1, 0) for k in range(7001)]
    blob = crm.big_store(scids[::-1])
    entries = crm.sorted_digest(blob)[0]
    with eng.gossip_store_digest(blob) as dg:
        msgs = lists_of(entries, 7001, 7001) + [rcm.reply(crm.CHAIN, 0, 1 << 24, [crm.scid_of(5, k, 5) for k in range(1000)])]
        m = compare_equals_model(eng, dg, entries, [], msgs)
        assert (len(m[2]), len(m[3])) == (8001, 7001)
        assert [len(x) for x in m[5]] == [37 + 8 * 8000, 45, 37 + 8 * 7000 + 5 + 7000, 37 + 8 + 3 + 1]
        for mu, ms in ((8001, 0), (0, 7001), (0xFFFFFFFF, 1)):
            with pytest.raises(LamdError):
                eng.channel_range_compare(dg, crm.CHAIN, msgs[:1], max_unknown=mu, max_stale=ms)
        compare_equals_model(eng, dg, entries, [], msgs, mu=8000, ms=7000)


# ------------------------------------------------------------------------------------------------ 7, 9. alignment, sizing
GUARD = 64


def raw_call(eng, dg, msgs, pad=0, scid_cap=0, msg_cap=0, out_cap=0, host_out=True, d_out=None, want=None, mu=0, ms=0):
    """the C call itself, the messages behind `pad` bytes, every array pre-filled and followed by a guard region"""
    from lightning_amd import _ffi
    n = len(msgs)
    moff = np.zeros(n + 1, dtype=np.uint64)
    moff[0] = pad
    moff[1:] = pad + np.cumsum([len(m) for m in msgs], dtype=np.uint64) if n else pad
    blob = np.frombuffer(b"\xA5" * pad + b"".join(msgs) + b"\x00", dtype=np.uint8)
    chain = np.frombuffer(crm.CHAIN, dtype=np.uint8)
    status, per_msg = np.full(n + GUARD, 99, dtype=np.int8), np.full(3 * n + GUARD, 0xABABABAB, dtype=np.uint32)
    unknown, stale = np.full(scid_cap + GUARD, 2 ** 64 - 1, dtype=np.uint64), np.full(scid_cap + GUARD, 2 ** 64 - 1, dtype=np.uint64)
    flags, msg_off = np.full(scid_cap + GUARD, 0xEE, dtype=np.uint8), np.full(msg_cap + GUARD, 2 ** 64 - 1, dtype=np.uint64)
    out = np.full(out_cap + GUARD, 0xEE, dtype=np.uint8)
    s = _ffi.LamdRangeCompareSummary()
    rc = eng._lib.lamd_channel_range_compare_batch(eng._ctx, dg._h, chain.ctypes.data, n, blob.ctypes.data, moff.ctypes.data, None, None, mu, ms, status.ctypes.data,
                                                   per_msg.ctypes.data, scid_cap, unknown.ctypes.data, stale.ctypes.data, flags.ctypes.data, msg_cap,
                                                   msg_off.ctypes.data, out.ctypes.data if host_out and d_out is None else None,
                                                   None if d_out is None else d_out.data_ptr(), out_cap, ctypes.byref(s))
    return rc, status, per_msg, unknown, stale, flags, msg_off, out, s


def untouched(a, used=0):
    fill = {np.dtype(np.uint64): 2 ** 64 - 1, np.dtype(np.uint8): 0xEE, np.dtype(np.int8): 99, np.dtype(np.uint32): 0xABABABAB}[a.dtype]
    return bool((a[used:] == fill).all())


def test_messages_and_output_at_every_alignment(eng, slots):
    import torch
    dg, entries, bare, _ = slots
    msgs = rcm.probe_replies(entries, bare, per=3)[:40] + [c[0] for c in rcm.status_cases() if c[1] is None]
    model = rcm.compare(entries, bare, crm.CHAIN, msgs, None, 5, 3)
    U, S, M, flat = len(model[2]), len(model[3]), len(model[5]), b"".join(model[5])
    assert U > 5 and S > 3
    for pad in range(8):                                                                    # the scid arrays start at every residue mod 8
        rc, status, per_msg, unknown, stale, flags, msg_off, out, s = raw_call(eng, dg, msgs, pad, max(U, S), M + 1, len(flat), mu=5, ms=3)
        assert rc == 0 and [int(x) for x in status[:len(msgs)]] == model[0] and [tuple(int(x) for x in per_msg[3 * i:3 * i + 3]) for i in range(len(msgs))] == model[1]
        assert [int(x) for x in unknown[:U]] == model[2] and [int(x) for x in stale[:S]] == model[3] and [int(x) for x in flags[:S]] == model[4]
        assert out[:len(flat)].tobytes() == flat and [int(x) for x in msg_off[:M + 1]] == list(np.cumsum([0] + [len(x) for x in model[5]]))
        assert untouched(status, len(msgs)) and untouched(per_msg, 3 * len(msgs)) and untouched(unknown, U) and untouched(stale, S) and untouched(flags, S)
        assert untouched(msg_off, M + 1) and untouched(out, len(flat))
    eng._after_torch()
    for shift in (0, 1, 2, 3):                                                              # the output left on the device
        d = torch.full((len(flat) + shift + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = raw_call(eng, dg, msgs, 3, max(U, S), M, len(flat), d_out=d[shift:], mu=5, ms=3)[0]
        assert rc == 0
        h = d.cpu().numpy()
        assert h[shift:shift + len(flat)].tobytes() == flat and set(h[:shift]) <= {0xEE} and set(h[shift + len(flat):]) == {0xEE}
        rc, *_, s = raw_call(eng, dg, msgs, 3, max(U, S), M, len(flat) - 1, d_out=d[shift:], mu=5, ms=3)
        assert rc == -3 and s.bytes == len(flat)
        assert d.cpu().numpy()[shift:shift + len(flat)].tobytes() == flat                  # ... and left alone by the call that failed


def test_caps_one_short_write_nothing(eng, slots):
    dg, entries, bare, _ = slots
    msgs = rcm.probe_replies(entries, bare, per=4)
    model = rcm.compare(entries, bare, crm.CHAIN, msgs, None, 6, 4)
    U, S, M, total = len(model[2]), len(model[3]), len(model[5]), sum(len(x) for x in model[5])
    cap = max(U, S)
    assert U != S
    for scid_cap, msg_cap, out_cap, host_out in ((cap - 1, M, total, True), (cap, M - 1, total, True), (cap, M, total - 1, True), (0, 0, 0, True), (0, 0, 0, False),
                                                 (min(U, S), M, total, True)):                 # scid_cap must hold EACH list
        rc, status, per_msg, unknown, stale, flags, msg_off, out, s = raw_call(eng, dg, msgs, 0, scid_cap, msg_cap, out_cap, host_out, mu=6, ms=4)
        assert rc == -3 and (s.unknown, s.stale, s.messages, s.bytes, s.unknown_messages) == (U, S, M, total, -(-U // 6))
        assert [int(x) for x in status[:len(msgs)]] == model[0] and [tuple(int(x) for x in per_msg[3 * i:3 * i + 3]) for i in range(len(msgs))] == model[1]
        assert all(untouched(a) for a in (unknown, stale, flags, msg_off, out))
    rc, _, _, unknown, stale, flags, msg_off, out, s = raw_call(eng, dg, msgs, 0, cap, M, 0, False, mu=6, ms=4)    # no output asked for: the lists alone
    assert rc == 0 and [int(x) for x in unknown[:U]] == model[2] and [int(x) for x in flags[:S]] == model[4] and int(msg_off[M]) == total and untouched(out)


def test_empty_batches_and_empty_digests(eng, slots):
    dg, entries, bare, _ = slots
    m = compare_equals_model(eng, dg, entries, bare, [])
    assert m == ([], [], [], [], [], [])
    rc, *_, msg_off, out, s = raw_call(eng, dg, [], 0, 0, 1, 0)
    assert rc == 0 and int(msg_off[0]) == 0 and s.messages == 0
    compare_equals_model(eng, dg, entries, bare, [rcm.reply(crm.CHAIN, 0, 5, []), b"", rcm.reply(crm.FOREIGN, 0, 5, [1, 2])])      # messages, but no entry
    probes = rcm.probe_replies(entries, bare)
    everything = sorted({s for m in probes for s in rcm.parse(m)[1]})
    with eng.gossip_store_digest(crm.big_store([])) as none:                                 # records, but no channel: everything is unknown
        assert len(none) == 0 and none.summary["records"] == 0
        m = compare_equals_model(eng, none, [], [], probes)
        assert m[2] == everything and m[3] == []
    with eng.gossip_store_digest(sa.serialise(0x10, [crm.fast_rec(crm.AMOUNT)])) as none:
        assert len(none) == 0 and none.summary["records"] == 1 and len(none.read_bare()) == 0
        assert compare_equals_model(eng, none, [], [], probes)[2] == everything
    only_bare = sa.serialise(0x10, [crm.fast_rec(crm.cann(crm.scid_of(77, 1, 1), 1)), crm.fast_rec(crm.AMOUNT)])
    with eng.gossip_store_digest(only_bare) as b:                                            # no entry at all, one bare channel
        s = crm.scid_of(77, 1, 1)
        m = compare_equals_model(eng, b, [], [s], [rcm.reply(crm.CHAIN, 0, 100, [s, s + 1], [(0, 3), (0, 3)])])
        assert (m[2], m[3], m[4]) == ([s + 1], [s], [4])
    # digests of other contexts are refused
    from lightning_amd import Engine
    from lightning_amd.engine import LamdError
    with Engine(0) as other, pytest.raises(LamdError):
        other.channel_range_compare(dg, crm.CHAIN, probes[:1])


# ------------------------------------------------------------------------------------------------ 8. round trip with the responder
def test_round_trip_with_the_responder(eng):
    rng = random.Random(8)
    chans_a, chans_b, expect_unknown, expect_stale = [], [], set(), {}
    for k in range(400):
        s = crm.scid_of(1000 + k // 3, k % 3, 0)
        kind = k % 8                                                    # 0: only in A, 1: only in B, 2: B newer in direction 0, 3: in direction 1, 4: A newer, 5: bare in A, else equal
        ta = tb = (100 + k, 200 + k)
        if kind == 2:
            tb = (ta[0] + 5, ta[1])
        if kind == 3:
            tb = (ta[0], ta[1] + 1)
        if kind == 4:
            ta = (ta[0] + 9, ta[1] + 9)
        for chans, ts, there, is_bare in ((chans_a, ta, kind != 1, kind == 5), (chans_b, tb, kind != 0, False)):
            if there:
                ups = [] if is_bare else [crm.fast_rec(crm.cupd(s, 0, ts[0])), crm.fast_rec(crm.cupd(s, 1, ts[1], 140))]
                chans.append([crm.fast_rec(crm.cann(s, k)), crm.fast_rec(crm.AMOUNT)] + ups)
        if kind == 1:
            expect_unknown.add(s)
        if kind in (2, 3, 5):
            expect_stale[s] = {2: 2, 3: 4, 5: 6}[kind]
    rng.shuffle(chans_b)                                                                     # B holds its channels in another order
    blob_a, blob_b = (sa.serialise(0x10, [r for c in chans for r in c]) for chans in (chans_a, chans_b))
    ea, ba, eb = crm.sorted_digest(blob_a)[0], rcm.bare(blob_a), crm.sorted_digest(blob_b)[0]
    assert len(ba) == 50 and expect_unknown == {e[0] for e in eb} - {e[0] for e in ea} - set(ba)  # the set arithmetic of the two model digests
    ours = {e[0]: e[1] for e in ea}
    ours.update({s: (0, 0) for s in ba})
    assert expect_stale == {e[0]: f for e in eb if e[0] in ours for f in [(2 if e[1][0] > ours[e[0]][0] else 0) | (4 if e[1][1] > ours[e[0]][1] else 0)] if f}
    with eng.gossip_store_digest(blob_a) as da, eng.gossip_store_digest(blob_b) as db:
        for option in (1, 3, 0):
            q = crm.query(crm.CHAIN, 0, 0xFFFFFFFF, option)
            st, replies = eng.channel_range_replies(db, crm.CHAIN, [q], max_encoded_bytes=800)      # several replies
            assert int(st[0]) == 0 and len(replies[0]) > 3
            m = compare_equals_model(eng, da, ea, ba, replies[0], want=[(0, 0xFFFFFFFF)] * len(replies[0]))
            assert set(m[0]) == {0} and m[2] == sorted(expect_unknown)
            assert dict(zip(m[3], m[4])) == (expect_stale if option & 1 else {})             # without timestamps no scid is stale
            st, own = eng.channel_range_replies(da, crm.CHAIN, [q], max_encoded_bytes=800)
            m = compare_equals_model(eng, da, ea, ba, own[0])
            assert m[2] == m[3] == m[5] == [] and sum(p[0] for p in m[1]) == len(ea)          # our own replies: nothing at all

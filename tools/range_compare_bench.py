"""Measures lamd_channel_range_compare_batch on one MI355X (not part of bench.py): stage times from HIP events (lamd_set_timing) and the wall
clock of the whole call, medians of warmed rounds.  Two workloads; in each a peer that holds the FULL store answers one whole-chain
query_channel_range with timestamps (lamd_channel_range_reply_batch), and its replies are compared with the digest of the same store with
every tenth channel removed and every seventh update made one second older:
  - the hand-built 5000-channel store of tests/channel_range_model.py;
  - the synthetic store of tools/channel_range_bench.py (--cann channel_announcements with their amount records, then --cupd channel_updates).
The digest is resident; the replies are host bytes, copied to the device by the call, and the lists and the query_short_channel_ids bytes come
back to the host.  One JSON line.

    python tools/range_compare_bench.py [--cann 150000 --cupd 450000 --runs 11]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--cann", type=int, default=150_000)
ap.add_argument("--cupd", type=int, default=450_000)
ap.add_argument("--runs", type=int, default=11)
args = ap.parse_args()
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from lightning_amd import Engine  # noqa: E402
from lightning_amd.workload import CANN_LEN, CUPD_LEN, make_gossip  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 3), median=round(xs[len(xs) // 2], 3), max=round(xs[-1], 3))


def records(msgs):
    """[n, len] messages -> [n, 12 + len] store records (COMPLETED, crc and timestamp 0)"""
    n, ln = msgs.shape
    out = np.zeros((n, 12 + ln), dtype=np.uint8)
    out[:, 0] = 0x20
    out[:, 2], out[:, 3] = ln >> 8, ln & 0xFF
    out[:, 12:] = msgs
    return out


def measure(eng, peer_image, our_image, chain):
    with eng.gossip_store_digest(peer_image) as theirs:
        status, replies = eng.channel_range_replies(theirs, chain, [crm.query(chain, 0, 0xFFFFFFFF, 1)])
        peer = {k: x for k, x in theirs.summary.items() if k != "stage_ms"}
    assert int(status[0]) == 0
    msgs = replies[0]
    stages, wall, info = [], [], {}
    with eng.gossip_store_digest(our_image) as ours:
        for run in range(3 + args.runs):                  # three warm-up rounds
            t0 = time.perf_counter()
            st, per_msg, unknown, stale, flags, out, s = eng.channel_range_compare(ours, chain, msgs, return_summary=True)
            t1 = time.perf_counter()
            if run >= 3:
                stages.append(s["stage_ms"])
                wall.append((t1 - t0) * 1e3)
        assert set(int(x) for x in st) == {0}
        info = dict(peer_digest=peer, our_digest={k: x for k, x in ours.summary.items() if k != "stage_ms"}, replies=len(msgs),
                    reply_bytes=sum(len(m) for m in msgs), **{k: x for k, x in s.items() if k != "stage_ms"})
    info["compare_stage_ms"] = {n: spread([x[j] for x in stages]) for j, n in enumerate(("classify", "merge", "plan", "encode"))}
    info["compare_stages_sum_ms"] = spread([sum(x) for x in stages])
    info["compare_call_ms"] = spread(wall)                # the wrapper's two calls: sizes first, then lists and bytes
    return info


def hand_built(thin):
    scids = [crm.scid_of(1000 + k // 3, k % 3, k & 1) for k in range(5000)][::-1]
    recs = []
    for k, s in enumerate(scids):
        if thin and k % 10 == 0:
            continue
        ts = 1000 + k - (1 if thin and k % 7 == 0 else 0)
        recs += [crm.fast_rec(crm.cann(s, k)), crm.fast_rec(crm.AMOUNT), crm.fast_rec(crm.cupd(s, k & 1, ts, 130 + k % 9), ts)]
    return sa.serialise(0x10, recs)


def synthetic(cann, cupd, thin):
    amount = np.zeros((len(cann), 10), dtype=np.uint8)
    amount[:, 0], amount[:, 1], amount[:, 7] = 0x10, 0x05, 1
    pairs = np.concatenate([records(cann), records(amount)], axis=1)
    if thin:
        pairs = pairs[np.arange(len(cann)) % 10 != 0]     # (the removed channels' updates stay: updates without a channel)
        cupd = cupd.copy()
        ts = (cupd[::7, 106:110].astype(np.uint32) << np.array([24, 16, 8, 0], dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
        ts = np.where(ts > 0, ts - 1, 0).astype(np.uint32)
        cupd[::7, 106:110] = np.stack([(ts >> sh) & 0xFF for sh in (24, 16, 8, 0)], axis=1).astype(np.uint8)
    return np.concatenate([np.array([0x10], dtype=np.uint8), pairs.reshape(-1), records(cupd).reshape(-1)])


with Engine(0) as eng:
    eng.set_timing(True)
    out = dict(runs=args.runs)
    out["hand_built_5000"] = measure(eng, hand_built(False), hand_built(True), crm.CHAIN)
    w = make_gossip(eng, args.cann, args.cupd)
    cann = w.msgs[:args.cann * CANN_LEN].reshape(args.cann, CANN_LEN)
    cupd = w.msgs[args.cann * CANN_LEN:args.cann * CANN_LEN + args.cupd * CUPD_LEN].reshape(args.cupd, CUPD_LEN)
    chain = bytes(cann[0, 260:292])                       # (no features: the chain_hash follows the feature length)
    out["synthetic"] = measure(eng, synthetic(cann, cupd, False), synthetic(cann, cupd, True), chain)
    print(json.dumps(out))

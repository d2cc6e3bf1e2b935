"""Measures lamd_gossip_store_directory_build and lamd_short_channel_ids_reply_batch on one MI355X (not part of bench.py): stage times from HIP
events (lamd_set_timing) and the wall clock of the whole call from Python, medians of warmed rounds, the image resident on the device.  Two stores:
  - the hand-built 5000-channel store of tools/range_compare_bench.py;
  - its synthetic store (--cann channel_announcements with their amount records, then --cupd channel_updates).
Per store: the digest build and the directory build; the replies to the query_short_channel_ids messages the comparison of DESIGN.md 3.17
writes for it (the same store with every tenth channel removed and every seventh update one second older, compared with the full store's
replies); and the replies to 64 queries of 8000 scids without TLV.  --digest-only: the digest build of the synthetic store alone (the
figure that must not move between commits).  One JSON line.

    python tools/scid_query_bench.py [--cann 150000 --cupd 450000 --runs 11] [--digest-only]
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
ap.add_argument("--digest-only", action="store_true")
args = ap.parse_args()
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from lightning_amd import Engine  # noqa: E402
from lightning_amd.engine import gossip_store_frame  # noqa: E402
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


def hand_built(thin):
    scids = [crm.scid_of(1000 + k // 3, k % 3, k & 1) for k in range(5000)][::-1]
    recs = []
    for k, s in enumerate(scids):
        if thin and k % 10 == 0:
            continue
        ts = 1000 + k - (1 if thin and k % 7 == 0 else 0)
        recs += [crm.fast_rec(crm.cann(s, k)), crm.fast_rec(crm.AMOUNT), crm.fast_rec(crm.cupd(s, k & 1, ts, 130 + k % 9), ts)]
    return np.frombuffer(sa.serialise(0x10, recs), dtype=np.uint8)


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


def timed(fn):
    """3 warm-up rounds, then --runs: -> ([stage_ms lists], [wall ms], the last result)"""
    stages, wall, res = [], [], None
    for run in range(3 + args.runs):
        t0 = time.perf_counter()
        res, ms = fn()
        t1 = time.perf_counter()
        if run >= 3:
            stages.append(ms)
            wall.append((t1 - t0) * 1e3)
    return stages, wall, res


def digest_build(eng, image, off, d_img):
    def one():
        with eng.gossip_store_digest(rec_off=off, d_store=d_img) as dg:
            return dict(dg.summary), dg.summary["stage_ms"]
    stages, wall, s = timed(one)
    return dict(records=s["records"], entries=s["entries"], stage_ms={n: spread([x[j] for x in stages]) for j, n in enumerate(("index", "slots", "channels", "sort", "entries"))},
                stages_sum_ms=spread([sum(x) for x in stages]), call_ms=spread(wall))


def replies(eng, dr, chain, queries):
    def one():
        st, pq, msgs, s = eng.short_channel_ids_replies(dr, queries, chain, return_summary=True)
        return s, s["stage_ms"]
    stages, wall, s = timed(one)
    enc = spread([x[3] for x in stages])
    return dict(queries=len(queries), query_bytes=sum(len(q) for q in queries), **{k: x for k, x in s.items() if k != "stage_ms"},
                stage_ms={n: spread([x[j] for x in stages]) for j, n in enumerate(("lookup", "nodes", "plan", "encode"))}, stages_sum_ms=spread([sum(x) for x in stages]),
                encode_gb_per_s=round(s["bytes"] / (enc["median"] * 1e6), 1) if enc["median"] else None,
                call_ms=spread(wall))                     # the wrapper's two calls: sizes first, then offsets and bytes


def measure(eng, full, thin, chain):
    off = gossip_store_frame(full)[0]
    d_img = torch.from_numpy(full.copy()).cuda()
    torch.cuda.synchronize()
    info = dict(image_bytes=int(full.size), digest_build=digest_build(eng, full, off, d_img))
    with eng.gossip_store_digest(rec_off=off, d_store=d_img) as dg:
        def one():
            dr = eng.gossip_store_directory(dg, rec_off=off, d_store=d_img)
            s = dict(dr.summary)
            dr.free()
            return s, s["stage_ms"]
        stages, wall, s = timed(one)
        info["directory_build"] = dict(**{k: x for k, x in s.items() if k != "stage_ms"},
                                       stage_ms={n: spread([x[j] for x in stages]) for j, n in enumerate(("bare", "candidates", "sort", "rank", "node_announcements"))},
                                       stages_sum_ms=spread([sum(x) for x in stages]), call_ms=spread(wall))
        status, range_replies = eng.channel_range_replies(dg, chain, [crm.query(chain, 0, 0xFFFFFFFF, 1)])
        scids = [int(x) for x in dg.read()[0]]
        with eng.gossip_store_directory(dg, rec_off=off, d_store=d_img) as dr, eng.gossip_store_digest(thin) as ours:
            queries = eng.channel_range_compare(ours, chain, range_replies[0])[5]
            info["replies_to_the_comparisons_queries"] = replies(eng, dr, chain, queries)
            pick = [scids[(7919 * k) % len(scids)] for k in range(64 * 8000)]
            head = b"\x01\x05" + chain + (1 + 8 * 8000).to_bytes(2, "big") + b"\x00"
            big = [head + np.array(pick[8000 * q:8000 * q + 8000], dtype=">u8").tobytes() for q in range(64)]
            info["replies_to_64_queries_of_8000"] = replies(eng, dr, chain, big)
    return info


with Engine(0) as eng:
    eng.set_timing(True)
    out = dict(runs=args.runs)
    if not args.digest_only:
        out["hand_built_5000"] = measure(eng, hand_built(False), hand_built(True), crm.CHAIN)
    w = make_gossip(eng, args.cann, args.cupd)
    cann = w.msgs[:args.cann * CANN_LEN].reshape(args.cann, CANN_LEN)
    cupd = w.msgs[args.cann * CANN_LEN:args.cann * CANN_LEN + args.cupd * CUPD_LEN].reshape(args.cupd, CUPD_LEN)
    chain = bytes(cann[0, 260:292])                       # (no features: the chain_hash follows the feature length)
    full = synthetic(cann, cupd, False)
    if args.digest_only:
        d_img = torch.from_numpy(full.copy()).cuda()
        torch.cuda.synchronize()
        out["synthetic_digest_build"] = digest_build(eng, full, gossip_store_frame(full)[0], d_img)
    else:
        out["synthetic"] = measure(eng, full, synthetic(cann, cupd, True), chain)
    print(json.dumps(out))

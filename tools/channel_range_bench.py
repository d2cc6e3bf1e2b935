"""Measures lamd_gossip_store_digest_build and lamd_channel_range_reply_batch on one MI355X (not part of bench.py): stage times from HIP
events (lamd_set_timing) and the wall clock of the whole calls, medians of warmed runs, on two stores:
  - the hand-built 5000-channel store of tests/channel_range_model.py (15 000 records, one update per channel);
  - the synthetic store of tools/store_audit_bench.py: the device-generated cfg4 traffic (lightning_amd/workload.py make_gossip), --cann
    channel_announcements each followed by its channel_amount record, then --cupd channel_updates.  The header CRCs are left 0: the digest
    reads none without verdicts.
The batch is 64 queries for the whole chain with both options.  Images resident, replies copied to the host.  One JSON line.

    python tools/channel_range_bench.py [--cann 150000 --cupd 450000 --runs 11]
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
ap.add_argument("--queries", type=int, default=64)
args = ap.parse_args()
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import channel_range_model as crm  # noqa: E402
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


def measure(eng, image, chain):
    off = gossip_store_frame(image)[0]
    d_image = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy() if isinstance(image, bytes) else image).cuda()
    torch.cuda.synchronize()
    queries = [crm.query(chain, 0, 0xFFFFFFFF, 3)] * args.queries
    build, build_wall, reply, reply_wall = [], [], [], []
    info = {}
    for run in range(3 + args.runs):                      # three warm-up rounds
        t0 = time.perf_counter()
        dg = eng.gossip_store_digest(None, rec_off=off, d_store=d_image)
        t1 = time.perf_counter()
        status, replies, s = eng.channel_range_replies(dg, chain, queries, return_summary=True)
        t2 = time.perf_counter()
        if run >= 3:
            build.append(dg.summary["stage_ms"])
            build_wall.append((t1 - t0) * 1e3)
            reply.append(s["stage_ms"])
            reply_wall.append((t2 - t1) * 1e3)
        info = dict(records=int(len(off)), image_bytes=int(d_image.numel()), digest={k: x for k, x in dg.summary.items() if k != "stage_ms"},
                    replies=s["messages"], reply_bytes=s["bytes"], entries_per_query=sum(len(crm.decode_reply(r)["scids"]) for r in replies[0]))
        assert set(int(x) for x in status) == {0} and info["entries_per_query"] == len(dg)
        dg.close()
    info["digest_stage_ms"] = {n: spread([st[j] for st in build]) for j, n in enumerate(("index", "slots", "channels", "sort", "entries"))}
    info["digest_stages_sum_ms"] = spread([sum(st) for st in build])
    info["digest_call_ms"] = spread(build_wall)
    info["reply_stage_ms"] = {n: spread([st[j] for st in reply]) for j, n in enumerate(("plan", "encode"))}
    info["reply_call_ms"] = spread(reply_wall)             # the wrapper's two calls: sizes first, then the bytes
    return info


with Engine(0) as eng:
    eng.set_timing(True)
    out = dict(runs=args.runs, queries=args.queries)
    out["hand_built_5000"] = measure(eng, crm.big_store([crm.scid_of(1000 + k // 3, k % 3, k & 1) for k in range(5000)][::-1]), crm.CHAIN)
    w = make_gossip(eng, args.cann, args.cupd)
    cann = w.msgs[:args.cann * CANN_LEN].reshape(args.cann, CANN_LEN)
    cupd = w.msgs[args.cann * CANN_LEN:args.cann * CANN_LEN + args.cupd * CUPD_LEN].reshape(args.cupd, CUPD_LEN)
    amount = np.zeros((args.cann, 10), dtype=np.uint8)
    amount[:, 0], amount[:, 1], amount[:, 7] = 0x10, 0x05, 1
    pairs = np.concatenate([records(cann), records(amount)], axis=1)
    image = np.concatenate([np.array([0x10], dtype=np.uint8), pairs.reshape(-1), records(cupd).reshape(-1)])
    chain = bytes(cann[0, 260:292])                       # (no features: the chain_hash follows the feature length)
    out["synthetic"] = measure(eng, image, chain)
    print(json.dumps(out))

"""Measures lamd_gossip_store_stream_build and lamd_timestamp_filter_reply_batch on one MI355X (not part of bench.py): stage times from HIP
events (lamd_set_timing) and the wall clock of the whole call from Python, medians of warmed rounds, the image resident on the device.  The
store: --groups times (channel_announcement, channel_amount, two channel_updates), header timestamps rising by one per group.  The peers:
--peers filters in turn "everything" (first_timestamp 0), "recent" and a window of --window seconds in the middle of the store, each with
--budget bytes, the window peers from cursor 0 (they read the whole list), the output left on the device.  One JSON line.

    python tools/timestamp_filter_bench.py [--groups 250000 --peers 64 --budget 1000000 --window 1000 --runs 11]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=250_000)
ap.add_argument("--peers", type=int, default=64)
ap.add_argument("--budget", type=int, default=1_000_000)
ap.add_argument("--window", type=int, default=1000)
ap.add_argument("--runs", type=int, default=11)
args = ap.parse_args()
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import channel_range_model as crm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from lightning_amd import Engine, _ffi  # noqa: E402

T0 = 1_000_000


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 3), median=round(xs[len(xs) // 2], 3), max=round(xs[-1], 3))


def store(groups):
    """-> (image uint8, rec_off uint64): one group's bytes tiled, the header timestamp of every record set to T0 + its group"""
    s = crm.scid_of(700, 1, 1)
    one = sa.serialise(0x10, [crm.fast_rec(crm.cann(s)), crm.fast_rec(crm.AMOUNT), crm.fast_rec(crm.cupd(s, 0, 5)), crm.fast_rec(crm.cupd(s, 1, 6, 141))])[1:]
    offs = np.array([r[0] - 1 for r in sa.walk(b"\x10" + one)[0]], dtype=np.uint64)
    body = np.tile(np.frombuffer(one, dtype=np.uint8), (groups, 1))
    ts = (T0 + np.arange(groups, dtype=np.uint32)).astype(">u4").view(np.uint8).reshape(groups, 4)
    for o in offs:
        body[:, int(o) + 8:int(o) + 12] = ts
    img = np.concatenate([np.array([0x10], dtype=np.uint8), body.reshape(-1)])
    rec_off = (1 + np.arange(groups, dtype=np.uint64)[:, None] * np.uint64(len(one)) + offs[None, :]).reshape(-1)
    return img, rec_off


def main():
    img, rec_off = store(args.groups)
    mid = T0 + args.groups // 2
    kinds = [(0, 0xFFFFFFFF), (1, 0xFFFFFFFF), (mid, args.window)]
    filters = [struct.pack(">H", 265) + crm.CHAIN + struct.pack(">II", *kinds[p % 3]) for p in range(args.peers)]
    now = T0 + args.groups - 100 + 7200                                                       # recent: the last 100 groups
    res = dict(records=int(rec_off.size), image_bytes=int(img.size), peers=args.peers, budget=args.budget, window=args.window)
    with Engine(0) as eng:
        eng.set_timing(True)
        d_img = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        builds, walls = [], []
        for _ in range(args.runs):
            t = time.perf_counter()
            ss = eng.gossip_store_stream(rec_off=rec_off, d_store=d_img)
            walls.append(1e3 * (time.perf_counter() - t))
            builds.append(ss.summary["stage_ms"])
            if _ < args.runs - 1:
                ss.free()
        res["streamable"] = len(ss)
        res["build_ms"] = dict(zip(("flags", "scans", "compact"), (spread([b[k] for b in builds[1:]]) for k in range(3))), call=spread(walls[1:]))
        n = len(filters)
        foff = np.zeros(n + 1, dtype=np.uint64)
        foff[1:] = np.cumsum([len(f) for f in filters], dtype=np.uint64)
        blob, chain = np.frombuffer(b"".join(filters) + b"\x00", dtype=np.uint8), np.frombuffer(crm.CHAIN, dtype=np.uint8)
        bud = np.full(n + 1, args.budget, dtype=np.int64)
        cin = np.array([0 if p % 3 == 2 else 2 ** 64 - 1 for p in range(n)] + [0], dtype=np.uint64)      # the window peers walk the whole list
        status, cur, done, first = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        s = _ffi.LamdFilterReplySummary()
        head = (eng._ctx, ss._h, chain.ctypes.data, now, n, blob.ctypes.data, foff.ctypes.data, cin.ctypes.data, bud.ctypes.data, status.ctypes.data, cur.ctypes.data,
                done.ctypes.data, first.ctypes.data)
        rc = eng._lib.lamd_timestamp_filter_reply_batch(*head, 0, None, None, None, None, 0, ctypes.byref(s))
        assert rc in (0, -3), rc
        msg_off, d_out = np.zeros(s.messages + 1, dtype=np.uint64), torch.zeros(max(1, s.bytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stages, walls = [], []
        for _ in range(args.runs):
            t = time.perf_counter()
            eng._chk(eng._lib.lamd_timestamp_filter_reply_batch(*head, s.messages, msg_off.ctypes.data, None, None, d_out.data_ptr(), s.bytes, ctypes.byref(s)))
            walls.append(1e3 * (time.perf_counter() - t))
            stages.append(list(s.stage_ms))
        res.update(messages=int(s.messages), bytes=int(s.bytes), finished=int(s.finished))
        res["reply_ms"] = dict(zip(("count", "scan", "write", "encode"), (spread([x[k] for x in stages[1:]]) for k in range(4))), call=spread(walls[1:]))
        ss.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Receiving one drained queue of channel_announcements and lightningd's txout replies two ways, on one MI355X, in one process:
  host path    lamd_gossipd_process() and lamd_gossipd_txout_reply_batch() with the engine as back end (csrc/gossip_ingest.cpp: framing, the scid
               look-up and the ordered replay on the host around one signature batch, then one reply at a time);
  device path  lamd_channel_announcement_receive_batch() against the digest of the SAME store image, then
               lamd_channel_announcement_confirm_batch() against its digest and directory.
The store is what a GossipIngest holds after the first half of n_anns synthetic channel_announcements (lightning_amd/workload.make_gossip) and
their txout replies; the batch is ALL n_anns announcements, so half of them are already known; every announcement that is asked about gets the
right script back.  The store has no node_announcement, so no DYING bit is cleared (the ingest never clears one).  The confirm plan,
applied to the image, must equal the image the ingest holds after the same batch and replies.  Prints one JSON line.
usage: bench_announce_receive.py [n_anns=100000] [reps=3]"""
import hashlib
import json
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
from lightning_amd import Engine, workload  # noqa: E402
from lightning_amd.engine import apply_update_plan, gossip_store_frame  # noqa: E402
from lightning_amd.gossipd import GossipIngest  # noqa: E402

NA = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
NODES = 15000
NOW, PRUNE, HEIGHT = 1 << 32, 0xFFFFFFFF, 700_000

eng = Engine(0)
g = workload.make_gossip(eng, NA, 0, n_nodes=NODES, corrupt_frac=0.0, device="cuda:0")
chain = bytes(g.msgs[260:292])
n = g.n_cann
half = n // 2
blob, off = g.msgs[:int(g.off[n]) + 1], g.off[:n + 1].copy()
scid_of, spk = [], []
for i in range(n):
    m = g.msgs[int(g.off[i]):int(g.off[i + 1])]
    scid_of.append(int.from_bytes(bytes(m[292:300]), "big"))
    k1, k2 = sorted([bytes(m[366:399]), bytes(m[399:432])])
    spk.append(b"\x00\x20" + hashlib.sha256(b"\x52\x21" + k1 + b"\x21" + k2 + b"\x52\xae").digest())
peer = bytes(g.msgs[300:333])


def replies_for(idx):
    return (np.array([scid_of[i] for i in idx], dtype=np.uint64), np.full(len(idx), 1_000_000, dtype=np.uint64),
            np.frombuffer(b"".join(spk[i] for i in idx) + b"\x00", dtype=np.uint8), np.arange(len(idx) + 1, dtype=np.uint64) * 34)


first, second = replies_for(range(half)), replies_for(range(half, n))
host_ms, before, after = [], None, None
for rep in range(REPS):
    with GossipIngest(eng, chain, peer, HEIGHT, NOW, prune_interval=PRUNE, collect_events=False) as ing:
        ing.push_batch(peer, blob[:int(off[half]) + 1], off[:half + 1].copy())
        ing.process()
        ing.txout_reply_batch(*first)
        if rep == 0:
            before = ing.store_image()
        t0 = time.perf_counter()
        ing.push_batch(peer, blob, off)
        t1 = time.perf_counter()
        ing.process()
        t2 = time.perf_counter()
        ing.txout_reply_batch(*second)
        t3 = time.perf_counter()
        host_ms.append(dict(push=(t1 - t0) * 1e3, process=(t2 - t1) * 1e3, replies=(t3 - t2) * 1e3))
        if rep == 0:
            after, channels = ing.store_image(), ing.stats()["channels"]

rec_off = gossip_store_frame(before)[0]
t0 = time.perf_counter()
dg = eng.gossip_store_digest(before, rec_off=rec_off)
dr = eng.gossip_store_directory(dg, before, rec_off=rec_off, chain_hash=chain)
index_ms = (time.perf_counter() - t0) * 1e3
eng.set_timing(True)
rx_ms, cf_ms, rx_stage, cf_stage, rs, cs, plan = [], [], [], [], None, None, None
for rep in range(REPS):
    t0 = time.perf_counter()
    status, scid, script, asks, rs = eng.channel_announcement_receive(dg, (blob, off), chain, HEIGHT, return_summary=True)
    rx_ms.append((time.perf_counter() - t0) * 1e3)
    rx_stage.append(rs["stage_ms"])
    # the caller's pending map: the asked messages ascending by scid, with their scripts
    order = asks["msg"][np.argsort(asks["scid"], kind="stable")]
    p_off = np.zeros(order.size + 1, dtype=np.uint64)
    p_off[1:] = np.cumsum((off[order + 1] - off[order]).astype(np.uint64))
    p_blob = np.concatenate([blob[int(off[i]):int(off[i + 1])] for i in order] + [np.zeros(1, dtype=np.uint8)])
    replies = replies_for([int(i) for i in asks["msg"]])
    t0 = time.perf_counter()
    cstatus, pend, fails, plan, cs = eng.channel_announcement_confirm(dg, dr, (p_blob, p_off), script[order], replies, return_summary=True)
    cf_ms.append((time.perf_counter() - t0) * 1e3)
    cf_stage.append(cs["stage_ms"])
eng.set_timing(False)
same = apply_update_plan(before, rec_off, plan)[0] == after
dr.free()
dg.close()
eng.close()
b1, b2 = int(np.argmin(rx_ms)), int(np.argmin(cf_ms))
print(json.dumps(dict(channels=int(channels), announcements=n, known=half, image_bytes=len(before), host_push_ms=min(h["push"] for h in host_ms),
                      host_process_ms=min(h["process"] for h in host_ms), host_replies_ms=min(h["replies"] for h in host_ms), host_all=host_ms, index_build_ms=index_ms,
                      receive_call_ms=rx_ms[b1], receive_all=rx_ms, receive_stage_ms=rx_stage[b1], receive_stages=["classify", "signatures and keys", "resolve", "scripts"],
                      confirm_call_ms=cf_ms[b2], confirm_all=cf_ms, confirm_stage_ms=cf_stage[b2], confirm_stages=["classify", "plan", "encode"],
                      receive_by_status=rs["by_status"], asks=rs["asks"], signature_rows=rs["signature_rows"], keyparse_rows=rs["keyparse_rows"],
                      confirm_by_status=cs["by_status"], added_bytes=cs["bytes"], applied_plan_equals_ingest_image=bool(same))))
sys.exit(0 if same else 1)

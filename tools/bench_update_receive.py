#!/usr/bin/env python3
"""Receiving one drained queue of channel_updates two ways, on one MI355X, in one process:
  host path    lamd_gossipd_process() with the engine as its back end (csrc/gossip_ingest.cpp: framing, hash maps, signer look-up and the ordered
               replay on the host around one signature batch);
  device path  lamd_channel_update_receive_batch() against the digest and the directory of the SAME store image.
The store is the one a GossipIngest holds after n_channels synthetic channel_announcements and their txout replies; the batch is n_updates
synthetic channel_updates of those channels (lightning_amd/workload.make_gossip: timestamps uniform in 32 bits, 1 % with a damaged body).  The
plan of the device path, applied to the image, must equal the image the ingest holds after the same batch.  Prints one JSON line.
usage: bench_update_receive.py [n_channels=100000] [n_updates=500000] [reps=3]"""
import hashlib
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
from lightning_amd import Engine, workload  # noqa: E402
from lightning_amd.engine import apply_update_plan, gossip_store_frame  # noqa: E402
from lightning_amd.gossipd import GossipIngest  # noqa: E402

NA = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
NU = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NOW, PRUNE = 1 << 32, 0xFFFFFFFF                       # every 32-bit timestamp but 0 is reasonable

eng = Engine(0)
g = workload.make_gossip(eng, NA, NU, n_nodes=15000, corrupt_frac=0.01, device="cuda:0")
chain = bytes(g.msgs[260:292])
peer = bytes(g.ids[g.n_cann])
cann_blob, cann_off = g.msgs[:int(g.off[g.n_cann]) + 1], g.off[:g.n_cann + 1].copy()
cupd_blob = np.ascontiguousarray(g.msgs[int(g.off[g.n_cann]):])
cupd_off = (g.off[g.n_cann:] - g.off[g.n_cann]).copy()
spk = []
for i in range(g.n_cann):
    m = g.msgs[int(g.off[i]):int(g.off[i + 1])]
    k1, k2 = sorted([bytes(m[366:399]), bytes(m[399:432])])
    spk.append(b"\x00\x20" + hashlib.sha256(b"\x52\x21" + k1 + b"\x21" + k2 + b"\x52\xae").digest())
spk_blob = np.frombuffer(b"".join(spk) + b"\x00", dtype=np.uint8)
spk_off = np.arange(g.n_cann + 1, dtype=np.uint64) * 34
scids, sats = np.arange(g.n_cann, dtype=np.uint64), np.full(g.n_cann, 1_000_000, dtype=np.uint64)

host_ms, before, after = [], None, None
for rep in range(REPS):
    with GossipIngest(eng, chain, peer, 700_000, NOW, prune_interval=PRUNE, collect_events=False) as ing:
        ing.push_batch(peer, cann_blob, cann_off)
        ing.process()
        ing.txout_reply_batch(scids, sats, spk_blob, spk_off)
        if rep == 0:
            before = ing.store_image()
        t0 = time.perf_counter()
        ing.push_batch(peer, cupd_blob, cupd_off)
        t1 = time.perf_counter()
        ing.process()
        t2 = time.perf_counter()
        host_ms.append(dict(push=(t1 - t0) * 1e3, process=(t2 - t1) * 1e3))
        if rep == 0:
            after, channels = ing.store_image(), ing.stats()["channels"]

rec_off = gossip_store_frame(before)[0]
t0 = time.perf_counter()
dg = eng.gossip_store_digest(before, rec_off=rec_off)
dr = eng.gossip_store_directory(dg, before, rec_off=rec_off, chain_hash=chain)
index_ms = (time.perf_counter() - t0) * 1e3
eng.set_timing(True)
dev_ms, stage_ms, s, plan, status = [], [], None, None, None
for rep in range(REPS):
    t0 = time.perf_counter()
    status, flags, chan, plan, s = eng.channel_update_receive(dg, dr, (cupd_blob, cupd_off), chain, NOW, PRUNE, our_id=peer, peers=peer, return_summary=True)
    dev_ms.append((time.perf_counter() - t0) * 1e3)
    stage_ms.append(s["stage_ms"])
eng.set_timing(False)
same = apply_update_plan(before, rec_off, plan)[0] == after
dr.free()
dg.close()
eng.close()
best = int(np.argmin(dev_ms))
print(json.dumps(dict(channels=int(channels), updates=NU, image_bytes=len(before), host_push_ms=min(h["push"] for h in host_ms),
                      host_process_ms=min(h["process"] for h in host_ms), host_all=host_ms, index_build_ms=index_ms, device_call_ms=dev_ms[best], device_all=dev_ms,
                      stage_ms=stage_ms[best], stages=["classify", "signatures", "resolve", "plan", "encode"], by_status=s["by_status"], accepted=s["accepted"],
                      superseded=s["superseded"], deletions=s["deletions"], retimestamps=s["retimestamps"], signature_rows=s["signature_rows"],
                      added_bytes=s["bytes"], applied_plan_equals_ingest_image=bool(same))))
sys.exit(0 if same else 1)

#!/usr/bin/env python3
"""Receiving one drained queue of node_announcements two ways, on one MI355X, in one process:
  host path    lamd_gossipd_process() with the engine as its back end (csrc/gossip_ingest.cpp: framing, the address walk, the node look-up and
               the ordered replay on the host around one signature batch);
  device path  lamd_node_announcement_receive_batch() against the directory of the SAME store image.
The store is the one bench_update_receive.py uses: what a GossipIngest holds after n_channels synthetic channel_announcements and their txout
replies (no dying channel: the ingest never marks a received node_announcement DYING).  The batch is n_anns synthetic
node_announcements of the store's nodes: the node keys of lightning_amd/workload.make_gossip derived again on the host, timestamps uniform in
32 bits, one to three address descriptors, 1 % with a damaged body; signed by the oracle's signer.  The plan of the device path, applied to the
image, must equal the image the ingest holds after the same batch.  Prints one JSON line.
usage: bench_node_receive.py [n_channels=100000] [n_anns=100000] [reps=3]"""
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
from oracle import orc  # noqa: E402

NA = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
NN = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NODES = 15000
NOW, PRUNE = 1 << 32, 0xFFFFFFFF
M64 = (1 << 64) - 1
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def node_key(seed, idx):
    """the secret key of node idx as csrc/lamd_testgen.hip draws it: rand_scalar(seed, idx, 1)"""
    v = sum(splitmix64(seed ^ splitmix64(idx * 4 + j + (1 << 56))) << (64 * j) for j in range(4))
    return ((v - N_ORDER if v >= N_ORDER else v) or 1).to_bytes(32, "big")


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


eng = Engine(0)
g = workload.make_gossip(eng, NA, 0, n_nodes=NODES, corrupt_frac=0.0, device="cuda:0")
chain = bytes(g.msgs[260:292])
cann_blob, cann_off = g.msgs[:int(g.off[g.n_cann]) + 1], g.off[:g.n_cann + 1].copy()
spk = []
in_store = set()
for i in range(g.n_cann):
    m = g.msgs[int(g.off[i]):int(g.off[i + 1])]
    in_store.update((bytes(m[300:333]), bytes(m[333:366])))
    k1, k2 = sorted([bytes(m[366:399]), bytes(m[399:432])])
    spk.append(b"\x00\x20" + hashlib.sha256(b"\x52\x21" + k1 + b"\x21" + k2 + b"\x52\xae").digest())
spk_blob = np.frombuffer(b"".join(spk) + b"\x00", dtype=np.uint8)
spk_off = np.arange(g.n_cann + 1, dtype=np.uint64) * 34
scids, sats = np.arange(g.n_cann, dtype=np.uint64), np.full(g.n_cann, 1_000_000, dtype=np.uint64)

# the batch: the keys of the first nodes (one that owns no channel is an unknown node), each announcement signed once
rng = np.random.Generator(np.random.PCG64(workload.SEED_CFG4 ^ 0x21))
t0 = time.perf_counter()
keys = []
for idx in range(min(NODES, max(64, NN // 8))):
    sk = node_key(workload.SEED_CFG4, idx)
    pub = orc.pubkey_create(sk)
    keys.append((sk, bytes([2 + (pub[64] & 1)]) + pub[1:33]))
known = sum(1 for _, nid in keys if nid in in_store)
ADDRS = (b"\x01\x7f\x00\x00\x01\x26\x07", b"\x02" + bytes(range(16)) + b"\x26\x07", b"\x04" + bytes(range(35)) + b"\x26\x07", b"\x05\x0bexample.org\x26\x07")
anns = []
for k in range(NN):
    sk, nid = keys[int(rng.integers(0, len(keys)))]
    addrs = b"".join(ADDRS[int(x)] for x in rng.integers(0, len(ADDRS), int(rng.integers(1, 4))))
    body = b"\x00\x00" + int(rng.integers(1, 1 << 32)).to_bytes(4, "big") + nid + rng.bytes(3) + rng.bytes(32) + len(addrs).to_bytes(2, "big") + addrs
    m = bytearray(b"\x01\x01" + orc.ecdsa_sign(sha256d(body), sk, rng.bytes(32)) + body)
    if rng.random() < 0.01:
        m[66 + 6 + int(rng.integers(0, 60))] ^= 1 << int(rng.integers(0, 8))
    anns.append(bytes(m))
sign_s = time.perf_counter() - t0
nann_off = np.zeros(NN + 1, dtype=np.uint64)
nann_off[1:] = np.cumsum([len(m) for m in anns], dtype=np.uint64)
nann_blob = np.frombuffer(b"".join(anns) + b"\x00", dtype=np.uint8)
peer = keys[0][1]

host_ms, before, after = [], None, None
for rep in range(REPS):
    with GossipIngest(eng, chain, peer, 700_000, NOW, prune_interval=PRUNE, collect_events=False) as ing:
        ing.push_batch(peer, cann_blob, cann_off)
        ing.process()
        ing.txout_reply_batch(scids, sats, spk_blob, spk_off)
        if rep == 0:
            before = ing.store_image()
        t0 = time.perf_counter()
        ing.push_batch(peer, nann_blob, nann_off)
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
dev_ms, stage_ms, s, plan = [], [], None, None
for rep in range(REPS):
    t0 = time.perf_counter()
    status, flags, node, plan, s = eng.node_announcement_receive(dr, (nann_blob, nann_off), return_summary=True)
    dev_ms.append((time.perf_counter() - t0) * 1e3)
    stage_ms.append(s["stage_ms"])
eng.set_timing(False)
same = apply_update_plan(before, rec_off, plan)[0] == after
nodes = len(dr)
dr.free()
dg.close()
eng.close()
best = int(np.argmin(dev_ms))
print(json.dumps(dict(channels=int(channels), nodes=nodes, announcements=NN, signers=len(keys), signers_in_store=known, signing_s=sign_s, image_bytes=len(before),
                      host_push_ms=min(h["push"] for h in host_ms), host_process_ms=min(h["process"] for h in host_ms), host_all=host_ms, index_build_ms=index_ms,
                      device_call_ms=dev_ms[best], device_all=dev_ms, stage_ms=stage_ms[best], stages=["classify", "signatures", "resolve", "plan", "encode"],
                      by_status=s["by_status"], accepted=s["accepted"], superseded=s["superseded"], deletions=s["deletions"], signature_rows=s["signature_rows"],
                      added_bytes=s["bytes"], applied_plan_equals_ingest_image=bool(same))))
sys.exit(0 if same else 1)

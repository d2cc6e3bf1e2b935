"""Measures lamd_gossip_store_audit on one MI355X (not part of bench.py): a synthetic gossip_store built on the device-generated cfg4
traffic (lightning_amd/workload.py make_gossip: channel_announcements + their channel_amount records + channel_updates), framed on the
host with valid CRCs; the time of every stage from HIP events (checksums, index, signers, signatures, verdicts) and of the whole call,
against lamd_sigcheck_gossip_spans_device over the same messages with host-supplied signers.  The slicing variant of k_store_crc is
chosen per process: run once with --ways 4 and once with --ways 8.

    python tools/store_audit_bench.py --ways 8 [--cann 150000 --cupd 450000 --runs 10]

--repair adds lamd_gossip_store_repair over the same image (resident in, output left resident): the keep, scan and pack stages from HIP
events, a plain device-to-device copy of out_len bytes timed the same way (the yardstick of k_store_pack), and the whole call next to the audit's.

--latest measures lamd_gossip_store_repair_latest instead, on that store with replays mixed in (seeded): the header timestamp of every update
is its signed one, and behind each update come 0-3 extra signed copies of its (channel, direction) -- a verbatim copy (equal timestamp) and
further updates of the same slot from a second stretch of the generator's stream (lower or higher timestamps), as far as the stream holds
any -- all updates then shuffled behind the announcements.  It reports the three stage_ms of the new call next to the plain repair's on the
same store in the same process, and the run-to-run spread of the signature stage they are to be read against.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--ways", type=int, default=4, choices=(4, 8))
ap.add_argument("--cann", type=int, default=150_000)
ap.add_argument("--cupd", type=int, default=450_000)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--repair", action="store_true")
ap.add_argument("--latest", action="store_true")
ap.add_argument("--seed", type=int, default=20)
args = ap.parse_args()
os.environ["LAMD_STORE_CRC_WAYS"] = str(args.ways)     # read once, at the first audit of the process
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lightning_amd import Engine  # noqa: E402
from lightning_amd.workload import CANN_LEN, CUPD_LEN, make_gossip  # noqa: E402


def crc32c_rows(seed, rows):
    """crc32c(seed[i], rows[i]) for equally long rows, one table step per byte column"""
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0x82F63B78), t >> 1)
    c = ~seed.astype(np.uint32)
    for k in range(rows.shape[1]):
        c = t[(c ^ rows[:, k]) & 0xFF] ^ (c >> 8)
    return ~c


def records(msgs, ts):
    """[n, len] messages -> [n, 12 + len] store records (COMPLETED, crc32c seeded with the timestamp)"""
    n, ln = msgs.shape
    out = np.zeros((n, 12 + ln), dtype=np.uint8)
    out[:, 0] = 0x20
    out[:, 2], out[:, 3] = ln >> 8, ln & 0xFF
    crc = crc32c_rows(ts, msgs)
    for k in range(4):
        out[:, 4 + k] = (crc >> (24 - 8 * k)) & 0xFF
        out[:, 8 + k] = (ts >> (24 - 8 * k)) & 0xFF
    out[:, 12:] = msgs
    return out


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 3), median=round(xs[len(xs) // 2], 3), max=round(xs[-1], 3))


def latest_bench(eng):
    """the store with replays, then the plain and the latest-wins repair over it: one JSON line"""
    rng = np.random.Generator(np.random.PCG64(args.seed))
    w = make_gossip(eng, args.cann, 2 * args.cupd)        # update u depends on (seed, u) alone: the first cupd are the plain store's
    cann = w.msgs[:args.cann * CANN_LEN].reshape(args.cann, CANN_LEN)
    cupd = w.msgs[args.cann * CANN_LEN:args.cann * CANN_LEN + 2 * args.cupd * CUPD_LEN].reshape(2 * args.cupd, CUPD_LEN)
    slot = (cupd[:, 98:106].astype(np.uint64) << (8 * np.arange(7, -1, -1, dtype=np.uint64))).sum(axis=1) * 2 + (cupd[:, 111] & 1)
    pool = {}                                             # slot -> the second stretch's updates of it
    for u in range(args.cupd, 2 * args.cupd):
        pool.setdefault(int(slot[u]), []).append(u)
    rows, extra = list(range(args.cupd)), rng.integers(0, 4, args.cupd)
    hist = [0, 0, 0, 0]
    for u in range(args.cupd):
        more = ([u] + [pool[int(slot[u])].pop() for _ in range(min(int(extra[u]) - 1, len(pool.get(int(slot[u]), ()))))]) if extra[u] else []
        hist[len(more)] += 1
        rows += more
    rows = np.array(rows)[rng.permutation(len(rows))]
    ups = cupd[rows]
    ts_u = (ups[:, 106:110].astype(np.uint32) << (8 * np.arange(3, -1, -1, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    amount = np.zeros((args.cann, 10), dtype=np.uint8)
    amount[:, 0], amount[:, 1], amount[:, 7] = 0x10, 0x05, 1
    pairs = np.concatenate([records(cann, np.arange(args.cann, dtype=np.uint32) + 1_600_000_000), records(amount, np.zeros(args.cann, dtype=np.uint32))], axis=1)
    image = np.concatenate([np.array([0x10], dtype=np.uint8), pairs.reshape(-1), records(ups, ts_u).reshape(-1)])
    d_image = torch.from_numpy(image).cuda()
    d_out = torch.zeros(image.size + 46, dtype=torch.uint8, device="cuda")
    uuid = bytes(range(32))
    torch.cuda.synchronize()
    calls = dict(plain=lambda: eng.gossip_store_repair(image, uuid, d_store=d_image, d_out=d_out, host_out=False),
                 latest=lambda: eng.gossip_store_repair_latest(image, uuid, now=0, d_store=d_image, d_out=d_out, host_out=False))
    first = {k: f() for k, f in calls.items()}            # warm-up, and what the two calls say about the store
    lat = first["latest"][6]
    assert np.array_equal(first["plain"][2], first["latest"][2]), "the two repairs' verdicts differ"
    fixed = d_out[:lat["out_len"]].cpu().numpy()          # (the latest call ran last)
    _, _, s2 = eng.gossip_store_audit(fixed, d_store=d_out[:lat["out_len"]])
    assert s2["clean"] == 1 and s2["records"] == lat["kept"] + 1, (s2, lat)
    eng.set_timing(True)
    stages, sig, wall = {k: [] for k in calls}, [], {k: [] for k in calls}
    for _ in range(args.runs):
        for k, f in calls.items():                        # alternating: both see the same box in the same state
            t0 = time.perf_counter()
            out = f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            stages[k].append(out[6]["stage_ms"])
            sig.append(out[5]["stage_ms"][3])
    eng.set_timing(False)
    keep = {k: spread([st[0] for st in stages[k]]) for k in calls}
    print(json.dumps(dict(
        latest=True, seed=args.seed, records=int(first["plain"][5]["records"]), updates=int(len(rows)), extra_copies_per_update=hist, image_bytes=int(image.size),
        runs=args.runs, plain={k: first["plain"][6][k] for k in ("kept", "dropped_verdict", "dropped_dependency", "out_len")},
        latest_summary={k: x for k, x in lat.items() if k != "stage_ms"},
        stage_ms={k: {n: spread([st[j] for st in stages[k]]) for j, n in enumerate(("keep", "scan", "pack"))} for k in calls},
        call_timed_ms={k: spread(wall[k]) for k in calls}, signature_stage_ms=spread(sig), signature_stage_spread_ms=round(max(sig) - min(sig), 3),
        keep_latest_minus_plain_ms=round(keep["latest"]["median"] - keep["plain"]["median"], 3))))


if args.latest:
    with Engine(0) as eng:
        latest_bench(eng)
    sys.exit(0)

with Engine(0) as eng:
    w = make_gossip(eng, args.cann, args.cupd)
    cann = w.msgs[:args.cann * CANN_LEN].reshape(args.cann, CANN_LEN)
    cupd = w.msgs[args.cann * CANN_LEN:args.cann * CANN_LEN + args.cupd * CUPD_LEN].reshape(args.cupd, CUPD_LEN)
    amount = np.zeros((args.cann, 10), dtype=np.uint8)
    amount[:, 0], amount[:, 1], amount[:, 7] = 0x10, 0x05, 1
    ts_a, ts_u = np.arange(args.cann, dtype=np.uint32) + 1_600_000_000, np.arange(args.cupd, dtype=np.uint32) + 1_650_000_000
    pairs = np.concatenate([records(cann, ts_a), records(amount, np.zeros(args.cann, dtype=np.uint32))], axis=1)
    image = np.concatenate([np.array([0x10], dtype=np.uint8), pairs.reshape(-1), records(cupd, ts_u).reshape(-1)])
    d_image = torch.from_numpy(image).cuda()
    # the same messages as a spans call with host-supplied signers: the baseline
    a_rec, u_rec = 12 + CANN_LEN + 22, 12 + CUPD_LEN
    start = np.concatenate([1 + 12 + a_rec * np.arange(args.cann, dtype=np.int64), 1 + a_rec * args.cann + 12 + u_rec * np.arange(args.cupd, dtype=np.int64)])
    length = np.concatenate([np.full(args.cann, CANN_LEN, dtype=np.int64), np.full(args.cupd, CUPD_LEN, dtype=np.int64)])
    d_start, d_len = torch.from_numpy(start).cuda(), torch.from_numpy(length).cuda()
    torch.cuda.synchronize()

    def spans():
        t0 = time.perf_counter()
        eng.sigcheck_gossip_spans_device(w.n, d_image, d_start, d_len, w.d_ids, w.d_rowbase, w.rows, w.d_verdict)
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def audit(resident):
        t0 = time.perf_counter()
        out = eng.gossip_store_audit(image, d_store=d_image if resident else None)
        return (time.perf_counter() - t0) * 1e3, out

    spans()
    assert np.array_equal(w.d_verdict.cpu().numpy(), w.expect), "baseline verdicts differ from the generator's"
    _, (off, verdict, s) = audit(True)
    v = verdict.astype(np.int64)
    assert s["records"] == 2 * args.cann + args.cupd and s["end_reason"] == "eof" and s["signatures"] == w.rows
    assert np.array_equal(v[0:2 * args.cann:2], w.expect[:args.cann]) and not v[1:2 * args.cann:2].any() and np.array_equal(v[2 * args.cann:], w.expect[args.cann:]), \
        "audit verdicts differ from the generator's"
    base = [spans() for _ in range(args.runs)]
    eng.set_timing(True)
    res, stages = [], []
    for _ in range(args.runs):
        ms, (_, _, s) = audit(True)
        res.append(ms)
        stages.append(s["stage_ms"])
    eng.set_timing(False)
    res_untimed = [audit(True)[0] for _ in range(args.runs)]
    host = [audit(False)[0] for _ in range(3)]
    names = ("crc", "index", "signers", "signatures", "verdict")
    repair = {}
    if args.repair:
        uuid = bytes(range(32))
        d_out = torch.zeros(image.size + 46, dtype=torch.uint8, device="cuda")

        def rep(host_out):
            t0 = time.perf_counter()
            out = eng.gossip_store_repair(image, uuid, d_store=d_image, d_out=d_out, host_out=host_out)
            return (time.perf_counter() - t0) * 1e3, out

        _, (_, _, rv, new_off, reason, _, r) = rep(False)
        assert np.array_equal(rv, verdict), "repair verdicts differ from the audit's"
        out_len = r["out_len"]
        # closure: the output audits clean and holds the kept records behind its uuid record
        fixed = d_out[:out_len].cpu().numpy()
        _, _, s2 = eng.gossip_store_audit(fixed, d_store=d_out[:out_len])
        assert s2["clean"] == 1 and s2["records"] == r["kept"] + 1, (s2, r)
        eng.set_timing(True)
        timed, rstages = [], []
        for _ in range(args.runs):
            ms, out = rep(False)
            timed.append(ms)
            rstages.append(out[6]["stage_ms"])
        eng.set_timing(False)
        untimed = [rep(False)[0] for _ in range(args.runs)]
        with_host = [rep(True)[0] for _ in range(3)]
        d_copy, copies = torch.empty(out_len, dtype=torch.uint8, device="cuda"), []
        for _ in range(args.runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_copy.copy_(d_out[:out_len])
            e1.record()
            e1.synchronize()
            copies.append(e0.elapsed_time(e1))
        pack_med, copy_med = spread([st[2] for st in rstages])["median"], spread(copies[1:])["median"]
        repair = dict(repair=dict(
            out_len=out_len, kept=r["kept"], dropped=[r[k] for k in ("dropped_deleted", "dropped_verdict", "dropped_dependency", "dropped_bookkeeping")],
            repair_resident_call_ms=spread(untimed), repair_resident_call_timed_ms=spread(timed), repair_resident_host_out_call_ms=spread(with_host),
            stage_ms={n: spread([st[k] for st in rstages]) for k, n in enumerate(("keep", "scan", "pack"))},
            d2d_copy_ms=spread(copies[1:]), pack_over_copy=round(pack_med / copy_med, 2), new_stages_ms=spread([sum(st) for st in rstages])))
    print(json.dumps(dict(repair,
        crc_ways=args.ways, records=s["records"], signatures=s["signatures"], image_bytes=int(image.size), runs=args.runs,
        spans_call_ms=spread(base), audit_resident_call_ms=spread(res_untimed), audit_resident_call_timed_ms=spread(res), audit_host_image_call_ms=spread(host),
        stage_ms={n: spread([st[k] for st in stages]) for k, n in enumerate(names)},
        new_stages_ms=spread([st[0] + st[1] + st[2] + st[4] for st in stages]),
        signature_stage_spread_ms=round(max(st[3] for st in stages) - min(st[3] for st in stages), 3))))

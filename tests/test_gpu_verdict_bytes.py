"""Verdict bytes are exactly 0 or 1, and BIP-340 stage 2 rejects on every device path.  The kernels of one call hand rows to each other through
the verdict byte (2: x(R) = r, parity still to be decided by k_schnorr_final / k_schnorr_final_fin, or a recovered point still to be compressed
by k_recover_final; 3: the bare formulas met Z = 0, k_ecmult_keyed_careful decides), and every caller treats a non-zero byte as an accept.  So
the rows here are those that only the LAST kernel of each route can refuse (bip340_stage2.py: x(R) = r with y(R) odd; R = infinity under a key
with a table), planted along the chains of rows one thread of the parity stage owns and mixed 50/50 with their accepted twins; every output
tensor is pre-filled with 9 and read through strict_bool; every comparison is exact.  test_bip340_stage2_host.py is the CPU side (the generator
against the C oracle and pyref, the same columns through the host build of the device code).  Needs an MI355X: -m gpu."""
import os
import time

import numpy as np
import pytest
import torch

import bip340_stage2 as st2
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu
H = bytes.fromhex


def _engine(env):
    from lightning_amd import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _rows(items, w):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), w).copy()


def _upload(cols):
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]
    torch.cuda.synchronize()
    return dev


def _fresh_ok(n):
    return torch.full((n,), 9, dtype=torch.uint8, device="cuda")           # a row the call never wrote fails the strict read


def _schnorr_device(e, dev):
    d_ok = _fresh_ok(dev[0].shape[0])
    torch.cuda.synchronize()
    e.verify_schnorr_device(dev[0], dev[1], dev[2], d_ok)
    e.synchronize()
    return d_ok.cpu().numpy()


def _exact(raw, exp, classes, what):
    """the raw bytes lie in {0, 1} and are the construction's"""
    got = strict_bool(raw)
    bad = np.flatnonzero(got != exp)
    cls = (lambda i: classes.get(i, "base")) if isinstance(classes, dict) else (lambda i: classes[i])
    assert not bad.size, ("%d rows differ" % bad.size, [(int(i), cls(int(i)), "accepted" if got[i] else "rejected") for i in bad[:8]], what)


@pytest.fixture(scope="module")
def pool_rows(orc):
    """4 500 rows tiled from the pool (built once): all 8 keys, every class; the C oracle agrees with the construction"""
    rows, m, k, s, exp = st2.tiled(4500, seed=3)
    assert np.array_equal(strict_bool(orc.schnorr_verify_batch(m, k, s, 4)), exp)
    classes = [r.cls for r in rows]
    assert all(classes.count(c) >= 400 for c in st2.CLASSES)
    return dict(rows=rows, cols=[m, k, s], exp=exp, classes=classes, dev=_upload([m, k, s]))


# ---- chains longer than one, both parity kernels
@pytest.mark.parametrize("env", [{}, {"LAMD_KEYED": "0"}], ids=["default-final_fin", "keyed0-final"])
def test_planted_chains_of_three_and_four_rows(orc, env):
    """n = 3 * 256 * CUs + 17: the smallest n at which every thread of the parity stage owns more than one row and some own one more than others.
    The base column is the workload generator's; every pattern of bip340_stage2.patterns() lies along a chain of 3 and along a chain of 4 rows,
    and 16 384 contiguous rows are odd_R / even_R by the seed.  Default engine: tables for the pool's 8 keys and most of the generator's,
    k_schnorr_final_fin over `fin`, which the ladder's rows (keys met too rarely for a table) share with the hot rows; LAMD_KEYED=0: the ladder,
    k_schnorr_final over the slots.  Both parity kernels are grid-stride loops, so the stride is the grid's size: 256 * CUs here."""
    from lightning_amd import workload
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * 256 * cu + 17
    stride = st2.final_stride(n, cu)
    assert stride == 256 * cu
    e = _engine(env)
    try:
        w = workload.make_schnorr(e, n, seed=0x340 + len(env), nkeys=n // 15, invalid_frac=0.01)
        cols, exp = w.cols, w.expect.copy()
        planted = st2.plant(cols, exp, stride, (3, 4), seed=7, block=1024)
        for length in (3, 4):
            assert [name for _, name in planted["chains"][length]] == [name for name, _ in st2.patterns(length)], planted["chains"]
            assert all(len(range(p, n, stride)) == length for p, _ in planted["chains"][length])
        assert planted["block"] == (1024, 16384)
        at = np.array(sorted(planted["classes"]))
        assert np.array_equal(strict_bool(orc.schnorr_verify_batch(*[np.ascontiguousarray(c[at]) for c in cols], 4)), exp[at])
        raw = _schnorr_device(e, _upload(cols))
        inf = e.info()
        _exact(raw, exp, planted["classes"], (env, inf))
        if env:
            assert inf["last_keyed"] == 0 and inf["last_hot_rows"] == 0 and inf["last_new_tables"] == 0, inf
        else:
            assert inf["last_keyed"] in (7, 10) and inf["last_hot_rows"] > n // 2 and inf["last_cold_rows"] > 0, inf
    finally:
        e.close()


# ---- the hot form, both comb shapes
@pytest.fixture(scope="module", params=[7, 10])
def eng_keyed(request):
    """engine forced onto per-key comb tables of one shape whenever a key has two rows"""
    e = _engine({"LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(request.param)})
    e.teeth = request.param
    yield e
    e.close()


def test_hot_form_decides_every_class(eng_keyed, pool_rows):
    """k_ecmult_keyed over the 8 keys' tables: schnorr_stage1 on the hot form's result parks Y * ZZZ and ZZ for stage 2; the R_inf rows leave Z = 0
    and go through marker 3 to the careful kernel.  Then again over warm tables."""
    e, p = eng_keyed, pool_rows
    e.cache_clear()
    n_inf = p["classes"].count("R_inf")
    for call in ("build", "repeat"):
        raw = _schnorr_device(e, p["dev"])
        inf = e.info()
        _exact(raw, p["exp"], p["classes"], (e.teeth, call, inf))
        assert inf["last_keyed"] == e.teeth and inf["last_hot_rows"] > 0 and inf["last_suspect_rows"] >= n_inf, (call, inf)
        if call == "build":
            assert inf["last_new_tables"] == st2.NKEYS and inf["last_hot_rows"] == len(p["exp"]), inf
        else:
            assert inf["last_cache_hits"] > 0 and inf["last_new_tables"] == 0, inf


@pytest.mark.parametrize("teeth", [7, 10])
def test_pairs_first_kernel_decides_every_class(pool_rows, teeth):
    p = pool_rows
    e = _engine({"LAMD_PAIRS": "1", "LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(teeth), "LAMD_CACHE": "0"})
    try:
        raw = _schnorr_device(e, p["dev"])
        inf = e.info()
        _exact(raw, p["exp"], p["classes"], (teeth, inf))
        assert inf["last_keyed"] == teeth and inf["last_hot_rows"] == len(p["exp"]) and inf["last_suspect_rows"] >= p["classes"].count("R_inf"), inf
    finally:
        e.close()


# ---- the one-launch path and the small cached path (host entry: strict through Engine's own reader)
def test_small_calls_from_host_memory(pool_rows):
    """k_small_verify / schnorr_accept_one on never-seen keys, then k_small_lookup with learnt keys, cached combs and the cold ladder: every size
    twice in a row"""
    from lightning_amd import Engine
    p = pool_rows
    first_odd = p["classes"].index("odd_R")
    with Engine(0) as e:
        for size in (1, 63, 64, 65, 700):
            sl = slice(first_odd, first_odd + size)
            assert "odd_R" in p["classes"][sl] and (size == 1 or {"even_R", "odd_R"} <= set(p["classes"][sl]))
            for call in (0, 1):
                got = e.verify_schnorr(*[c[sl] for c in p["cols"]])
                assert got.dtype == bool
                bad = np.flatnonzero(got != p["exp"][sl])
                assert not bad.size, (size, call, [(int(i), p["classes"][first_odd + int(i)]) for i in bad[:8]], e.info())


def _lane_rows(e):
    """per lane: (last_mode, last_keyed, rows on the lists of the lane's last keyed chunk)"""
    infs = [e.info(k) for k in range(e.info()["lanes"])]
    return [(i["last_mode"], i["last_keyed"], i["last_hot_rows"] + i["last_cold_rows"]) for i in infs]


# ---- the chunk split and the peer lane
def test_chunks_and_every_lane(pool_rows):
    """LAMD_CHUNK_ROWS=1000 (lamd_set_chunk_rows clamps to 4 096 rows and more, so it cannot cut 4 500 rows; the variable is not clamped): the
    call is cut into chunks of 1000, 1000, 1000, 1000 and 500 rows that alternate between the call's lane and its peer, each with its own tail
    launch -- seen in the lanes' own counters: the call's lane ended on 500 rows, its peer on 1000, no other lane ran.  LAMD_KEYED=1 so that every
    chunk, small as it is, takes the table-driven path and counts its rows.  Then the same call on every lane back to back, no host
    synchronisation between them, a verdict tensor each"""
    p = pool_rows
    n = len(p["exp"])
    assert n == 4500
    e = _engine({"LAMD_CHUNK_ROWS": "1000", "LAMD_KEYED": "1"})
    try:
        lanes = e.info()["lanes"]
        assert lanes >= 2
        raw = _schnorr_device(e, p["dev"])
        per_lane = _lane_rows(e)
        _exact(raw, p["exp"], p["classes"], ("chunks of 1000", per_lane))
        assert sorted(r for _, _, r in per_lane if r) == [500, 1000] and all(m == 1 and k in (7, 10) for m, k, r in per_lane if r), per_lane
        assert e.info()["last_hot_rows"] + e.info()["last_cold_rows"] == 500, e.info()          # the call's own lane ran the last chunk
        calls = max(6, lanes)
        outs = [_fresh_ok(n) for _ in range(calls)]
        torch.cuda.synchronize()
        for d_ok in outs:
            e.verify_schnorr_device(p["dev"][0], p["dev"][1], p["dev"][2], d_ok)
        e.synchronize()
        for k, d_ok in enumerate(outs):
            _exact(d_ok.cpu().numpy(), p["exp"], p["classes"], ("back to back", k))
        per_lane = _lane_rows(e)
        assert all(r in (500, 1000) for _, _, r in per_lane), per_lane                           # every lane has run chunks by now
    finally:
        e.close()


# ---- the streaming queue
@pytest.mark.parametrize("n_ecdsa,reps", [(20, 0), (300, 2)], ids=["small-flush", "general-path"])
def test_mixed_streaming_submission(kat, pool_rows, n_ecdsa, reps):
    """one submission holding ECDSA rows and BIP-340 rows of every class; the verdicts come through poll().  Each kind is flushed on its own: 20 + 30
    rows are two small flushes (one launch of k_small_verify each); 9 000 BIP-340 rows (the column twice: more than the 4 096 of a small flush and
    than the 8 192 below which a batch is only looked up in the cache) take the copies and the table-driven general path with k_schnorr_final_fin
    as its tail -- seen in the counters of the lane that ran it"""
    from lightning_amd import Engine
    p = pool_rows
    vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 66]
    vs = (vs * (n_ecdsa // len(vs) + 1))[:n_ecdsa]
    cols = [np.ascontiguousarray(np.tile(c, (reps, 1))) if reps else c[:30] for c in p["cols"]]
    classes = p["classes"] * reps if reps else p["classes"][:30]
    n_schnorr = len(classes)
    want = np.array([v["expect"] for v in vs] + (np.tile(p["exp"], reps) if reps else p["exp"][:30]).tolist(), dtype=bool)
    assert {"odd_R", "even_R", "R_inf"} <= set(classes) and 0 < want[:n_ecdsa].sum() < n_ecdsa and n_schnorr == (9000 if reps else 30)
    with Engine(0) as e:
        for call in range(2):
            assert e.queue_ecdsa_batch(_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64), _rows([H(v["pub"]) for v in vs], 33)) == 0
            assert e.queue_schnorr_batch(*cols) == n_ecdsa
            e.flush()
            deadline = time.monotonic() + 120
            got = e.poll(cap=len(want))
            while got is None and time.monotonic() < deadline:
                got = e.poll(cap=len(want))
            assert got is not None and got.dtype == bool and got.shape == want.shape
            bad = np.flatnonzero(got != want)
            assert not bad.size, (call, [(int(i), "ecdsa" if i < n_ecdsa else classes[int(i) - n_ecdsa]) for i in bad[:8]])
            e.synchronize()
            per_lane = _lane_rows(e)
            if reps:
                assert any(m == 1 and k in (7, 10) and r == n_schnorr for m, k, r in per_lane), (call, per_lane)


# ---- ECDSA through marker 3, recovery through marker 2
def test_ecdsa_suspect_rows_leave_no_marker(eng_keyed, kat):
    """the goldens whose comb sums degenerate (u1*G = +-u2*Q, R = infinity, Q = G, Q = lambda*G), each 16 times, through the device entry"""
    e = eng_keyed
    for publen, tags in ((65, ("u1G==u2Q", "R=inf")), (33, ("Q=G", "Q=lamG"))):
        vs = [v for v in kat["ecdsa"] if len(v["pub"]) == 2 * publen and any(t in v["name"] for t in tags)] * 16
        assert len(vs) >= 6 * 16
        dev = _upload([_rows([H(v[k]) for v in vs], w) for k, w in (("hash", 32), ("sig", 64), ("pub", publen))])
        d_ok = _fresh_ok(len(vs))
        torch.cuda.synchronize()
        e.verify_ecdsa_device(dev[0], dev[1], dev[2], d_ok)
        e.synchronize()
        inf = e.info()
        _exact(d_ok.cpu().numpy(), np.array([v["expect"] for v in vs], dtype=bool), [v["name"] for v in vs], (e.teeth, publen, inf))
        assert inf["last_keyed"] == e.teeth and inf["last_hot_rows"] > 0, (publen, inf)          # through the comb kernel
        if publen == 65:                                                                         # (no 33-byte row here is known to meet Z = 0)
            assert inf["last_suspect_rows"] > 0, inf


def test_recovery_leaves_no_marker(kat):
    from lightning_amd import Engine
    vs = kat["recover"]
    assert any(v["expect"] is None for v in vs) and any(v["expect"] is not None for v in vs)
    dev = _upload([_rows([H(v["hash"]) for v in vs], 32), _rows([H(v["sig"]) for v in vs], 64), np.array([v["recid"] for v in vs], dtype=np.uint8)])
    d_pub, d_ok = torch.full((len(vs), 33), 9, dtype=torch.uint8, device="cuda"), _fresh_ok(len(vs))
    torch.cuda.synchronize()
    with Engine(0) as e:
        e.ecdsa_recover_device(dev[0], dev[1], dev[2], d_pub, d_ok)
        e.synchronize()
        ok, keys = d_ok.cpu().numpy(), d_pub.cpu().numpy()
    _exact(ok, np.array([v["expect"] is not None for v in vs], dtype=bool), [v["name"] for v in vs], "recover")
    for v, o, k in zip(vs, ok, keys):
        assert (k.tobytes().hex() if o else None) == v["expect"], v["name"]

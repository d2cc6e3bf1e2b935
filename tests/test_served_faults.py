"""Fail-closed streaming through lamd_served: the stub engine (tests/c/stub_engine.c) is made to fail where the real engine can -- a queue call that
finds every staging set in flight or the set full (LAMD_ERR_STATE), a flush that fails after part of its set was sent, a collection that reports
another number of verdicts than were queued -- and every test asserts one rule: a row is reported 1 only if the engine verified it in the flush
that carried it; otherwise the call returns < 0 or the row reads 0.

The stub's verdict is a known function of the input bytes, so each test first streams a flush whose rows all read 1 from a client block, then
from the SAME block a flush whose rows all read 0 and whose way through the engine is made to fail: a verdict left over from the earlier flush
shows up as a 1.  Every case runs with the flush rows queued in place from the clients' registered blocks and copied (the runtime refuses to
pin: STUB_REFUSE_REGISTER=1)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_served as T

ROOT = T.ROOT
SIZES = (37, 23, 11)          # one flush = three runs: ECDSA 33-byte keys, BIP-340, ECDSA 65-byte keys
STALE_STATE, FLUSH_FAILS, MISCOUNT = 0x5E, 0xF1, 0xC7     # the stub's poison markers (second byte after 0xEE)
MODES = ["in_place", "copied"]


def _ecdsa(rng, n, kl, want, poison=None):
    """n ECDSA rows whose stub verdict is `want`; poison: the marker the stub reads in the first row's hash"""
    h, s, k = T._rows(rng, n, 32), T._rows(rng, n, 64), T._rows(rng, n, kl)
    if poison is not None:
        h[0, 0], h[0, 1] = 0xEE, poison
    k[:, -1] = (k[:, -1] & 0xFE) | ((h[:, 0] ^ s[:, 63] ^ want) & 1)
    assert np.all(T._stub_ecdsa(h, s, k) == want)
    return h, s, k


def _schnorr(rng, n, want, poison=None):
    m, x, s = T._rows(rng, n, 32), T._rows(rng, n, 32), T._rows(rng, n, 64)
    if poison is not None:
        m[0, 0], m[0, 1] = 0xEE, poison
    s[:, 3] = (s[:, 3] & 0xFE) | ((m[:, 1] ^ x[:, 2] ^ want) & 1)
    assert np.all(T._stub_schnorr(m, x, s) == want)
    return m, x, s


def _queue(L, ctx, rng, want, poison_run=None, marker=None, sizes=SIZES):
    """one open set of three runs whose rows all read `want` (a scalar) or the given per-run pattern; the first row of run `poison_run` carries
    `marker` -> the verdicts the stub gives, in ticket order"""
    wants = [np.full(n, want, np.uint8) if np.isscalar(want) else want[i] for i, n in enumerate(sizes)]
    p = [marker if poison_run == i else None for i in range(3)]
    h, s, k = _ecdsa(rng, sizes[0], 33, wants[0], p[0])
    assert L.lamd_queue_ecdsa_batch(ctx, sizes[0], h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0
    m, x, sg = _schnorr(rng, sizes[1], wants[1], p[1])
    assert L.lamd_queue_schnorr_batch(ctx, sizes[1], m.ctypes.data, x.ctypes.data, sg.ctypes.data) == sizes[0]
    h, s, k = _ecdsa(rng, sizes[2], 65, wants[2], p[2])
    assert L.lamd_queue_ecdsa_batch(ctx, sizes[2], h.ctypes.data, s.ctypes.data, k.ctypes.data, 65, 65) == sizes[0] + sizes[1]
    return np.concatenate(wants)


def _wait(L, ctx, n):
    """lamd_wait into a buffer that starts out all 9: -> (rc, the whole buffer, the count reported)"""
    ok, got = np.full(n, 9, np.uint8), ctypes.c_size_t(0)
    rc = L.lamd_wait(ctx, ok.ctypes.data, n, ctypes.byref(got))
    return rc, ok, got.value


def _fail_closed(rc, ok, cnt, exp):
    """the rule: an error leaves every verdict 0; a success reports exactly the flush's rows, and no row reads 1 that the engine did not verify"""
    if rc < 0:
        assert not ok.any(), "an error left verdicts the caller could read as 1: %s" % np.flatnonzero(ok)[:16]
    else:
        assert rc == 1 and cnt == len(exp), (rc, cnt, len(exp))
        assert not np.any(ok.astype(bool) & ~exp.astype(bool)), "rows read 1 that were never verified: %s" % np.flatnonzero(ok.astype(bool) & ~exp.astype(bool))[:16]
        assert np.array_equal(ok, exp)


def _server(stub, name, mode, monkeypatch, sets=None, extra=()):
    so, d = stub
    if mode == "copied":
        monkeypatch.setenv("STUB_REFUSE_REGISTER", "1")
    else:
        monkeypatch.delenv("STUB_REFUSE_REGISTER", raising=False)
    if sets:
        monkeypatch.setenv("STUB_QUEUE_SETS", str(sets))
    return T._start(os.path.join(d, "%s_%s.sock" % (name, mode)), so, list(extra))


def _stats(L, ctx):
    st = T.Stats()
    assert L.lamd_client_server_stats(ctx, ctypes.byref(st)) == 0
    return st


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("faults") / "libstub_engine.so")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "c", "stub_engine.c")])
    d = T._short_dir()
    yield so, d
    import shutil
    shutil.rmtree(d, ignore_errors=True)


def _ones_then_failing(L, ctx, rng, poison_run, marker):
    """a flush of all-1 rows (collected, checked), then from the same block a flush of all-0 rows whose run `poison_run` carries `marker`
    -> (rc, verdict buffer, count) of the second"""
    exp = _queue(L, ctx, rng, 1)
    assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
    rc, ok, cnt = _wait(L, ctx, len(exp))
    assert rc == 1 and cnt == len(exp) and ok.all(), (rc, cnt, L.lamd_last_error(ctx))
    exp = _queue(L, ctx, rng, 0, poison_run, marker)
    assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
    rc, ok, cnt = _wait(L, ctx, len(exp))
    _fail_closed(rc, ok, cnt, exp)
    return rc, ok, cnt


def _next_flush_is_exact(L, ctx, rng):
    """after a failure: a flush of mixed verdicts gets exactly its own verdicts and count"""
    want = [rng.integers(0, 2, n).astype(np.uint8) for n in SIZES]
    exp = _queue(L, ctx, rng, want)
    assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
    rc, ok, cnt = _wait(L, ctx, len(exp))
    assert rc == 1 and cnt == len(exp) and np.array_equal(ok, exp), (rc, cnt, L.lamd_last_error(ctx))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("run", [0, 1, 2], ids=["first_run", "middle_run", "last_run"])
def test_a_queue_call_that_fails_with_err_state_fails_the_flush(stub, mode, run, monkeypatch):
    """LAMD_ERR_STATE from a queue call was also the server's marker for "not failed while queued" -- the part was answered
    OK with only the rows queued before the failure copied, and the client read the rest of its verdicts from the block's previous flush"""
    p = _server(stub, "st%d" % run, mode, monkeypatch)
    try:
        L = T._client()
        rc0, ctx = T._connect(L, p.args[2])
        assert rc0 == 0, L.lamd_last_error(ctx)
        rng = np.random.default_rng(500 + run)
        rc, ok, cnt = _ones_then_failing(L, ctx, rng, run, STALE_STATE)
        assert rc == -5 and b"staging set full" in L.lamd_last_error(ctx), (rc, L.lamd_last_error(ctx))
        _next_flush_is_exact(L, ctx, rng)
        st = _stats(L, ctx)
        assert (st.flush_rows_in_place == 0) if mode == "copied" else (st.flush_rows_in_place > 0)
        L.lamd_shutdown(ctx)
    finally:
        T._stop(p)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("run", [0, 1, 2], ids=["first_run", "middle_run", "last_run"])
def test_a_flush_that_fails_part_way_answers_its_parts_with_the_error_and_carries_nothing_over(stub, mode, run, monkeypatch):
    """lamd_flush fails after part of the set was sent: the engine drops the open set (include/lightning_amd.h), the parts get the error, and the
    next flushes -- of the same client, from the same block rewritten, and of another client -- get exactly their own rows and count (stale rows
    carried into the next engine flush would change the count; in-place rows read after their client was answered would change the verdicts)"""
    p = _server(stub, "ff%d" % run, mode, monkeypatch)
    try:
        L = T._client()
        rc0, ctx = T._connect(L, p.args[2])
        rc1, ctx2 = T._connect(L, p.args[2])
        assert rc0 == 0 and rc1 == 0
        rng = np.random.default_rng(600 + run)
        rc, ok, cnt = _ones_then_failing(L, ctx, rng, run, FLUSH_FAILS)
        assert rc < 0 and b"flush failed part-way" in L.lamd_last_error(ctx), (rc, L.lamd_last_error(ctx))
        _next_flush_is_exact(L, ctx, rng)
        _next_flush_is_exact(L, ctx2, rng)
        # both clients with a flush each outstanding, one of them failing: whether or not the server merged them, the innocent one is exact
        exp_bad = _queue(L, ctx, rng, 0, run, FLUSH_FAILS)
        want = [rng.integers(0, 2, n).astype(np.uint8) for n in SIZES]
        exp_good = _queue(L, ctx2, rng, want)
        assert L.lamd_flush(ctx) == 0 and L.lamd_flush(ctx2) == 0
        _fail_closed(*_wait(L, ctx, len(exp_bad)), exp_bad)
        rc, ok, cnt = _wait(L, ctx2, len(exp_good))
        _fail_closed(rc, ok, cnt, exp_good)
        _next_flush_is_exact(L, ctx2, rng)
        _next_flush_is_exact(L, ctx, rng)
        L.lamd_shutdown(ctx)
        L.lamd_shutdown(ctx2)
    finally:
        T._stop(p)


@pytest.mark.parametrize("mode", MODES)
def test_a_flush_whose_verdict_count_does_not_match_fails_every_part(stub, mode, monkeypatch):
    """lamd_wait / lamd_poll report one verdict fewer than the engine flush carried: every client flush of it gets an error and reads no 1"""
    p = _server(stub, "mc", mode, monkeypatch)
    try:
        L = T._client()
        rc0, ctx = T._connect(L, p.args[2])
        assert rc0 == 0
        rng = np.random.default_rng(700)
        for run in range(3):
            rc, ok, cnt = _ones_then_failing(L, ctx, rng, run, MISCOUNT)
            assert rc == -5 and b"another number of verdicts" in L.lamd_last_error(ctx), (rc, L.lamd_last_error(ctx))
            _next_flush_is_exact(L, ctx, rng)
        L.lamd_shutdown(ctx)
    finally:
        T._stop(p)


SETS_CLIENT_SCRIPT = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_served as T, test_served_faults as F
L = T._client()
rc, ctx = T._connect(L, sys.argv[2])
assert rc == 0, L.lamd_last_error(ctx)
rng = np.random.default_rng(int(sys.argv[3]))
errors, stale, wrong, pend = 0, 0, 0, []
def collect():
    global errors, stale, wrong
    exp = pend.pop(0)
    rc, ok, cnt = F._wait(L, ctx, len(exp))
    if rc < 0:
        errors += 1
        print("error", rc, L.lamd_last_error(ctx))
        return
    stale += int(np.sum(ok.astype(bool) & ~exp.astype(bool)))
    wrong += int(cnt != len(exp) or not np.array_equal(ok, exp))
for it in range(int(sys.argv[4])):
    # alternately every row 1 and every row 0: a verdict left over from a block's previous flush reads 1 where 0 is due
    sizes = (int(rng.integers(1, 300)), int(rng.integers(1, 50)), int(rng.integers(1, 20)))
    pend.append(F._queue(L, ctx, rng, (it + 1) & 1, sizes=sizes))
    assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
    if len(pend) == 6:
        collect()
while pend:
    collect()
L.lamd_shutdown(ctx)
print("errors", errors, "stale", stale, "wrong", wrong)
"""


@pytest.mark.parametrize("mode", MODES)
def test_eight_clients_streaming_into_an_engine_with_three_staging_sets(stub, mode, monkeypatch):
    """an engine with fewer staging sets than the server's flushes in flight (STUB_QUEUE_SETS=3 against eight): the server sizes itself from
    lamd_get_info (queue_sets - 1 flushes in flight), so no queue call finds every set in flight -- no error, no stale verdict.  (--max-flush-rows
    64: every client flush becomes an engine flush of its own, so a round of the engine thread puts many of them in flight)"""
    p = _server(stub, "qs", mode, monkeypatch, sets=3, extra=["--max-flush-rows", "64"])
    try:
        procs = [subprocess.Popen([sys.executable, "-c", SETS_CLIENT_SCRIPT, ROOT, p.args[2], str(800 + i), "40"], stdout=subprocess.PIPE, text=True) for i in range(8)]
        outs = [q.communicate(timeout=180)[0] for q in procs]
        assert all(q.returncode == 0 for q in procs) and all(o.strip().endswith("errors 0 stale 0 wrong 0") for o in outs), outs
        L = T._client()
        rc, ctx = T._connect(L, p.args[2])
        assert rc == 0
        st = _stats(L, ctx)
        L.lamd_shutdown(ctx)
        assert st.flushes == 8 * 40 and st.flush_rows_in_place == (st.flush_rows if mode == "in_place" else 0)
    finally:
        T._stop(p)


def test_a_server_refuses_an_engine_with_one_staging_set(stub, monkeypatch):
    """rows are queued while a flush is in flight: an engine with a single staging set cannot stream under the server"""
    so, d = stub
    monkeypatch.setenv("STUB_QUEUE_SETS", "1")
    from lightning_amd import _build
    r = subprocess.run([_build.build_served()[0], "--socket", os.path.join(d, "one.sock"), "--engine", so], capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and "staging set" in r.stderr, (r.returncode, r.stderr)

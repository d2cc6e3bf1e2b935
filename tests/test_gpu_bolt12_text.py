"""Engine.bolt12_check (lamd_bolt12_check_text_batch) on the device against the sequential model (tests/bolt12_text_model.py): the strings the
reference holds and the fuzz sample (tests/golden/bolt12_strings.json) with what is pinned about them, every synthesised class, seeded random
mixed batches and their shuffles, a call that crosses the chunk loop, the empty batch and the argument checks.  Needs an MI355X: -m gpu."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bolt12_text_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


@pytest.fixture(scope="module")
def pool():
    return M.bases()


def _same(got, want, names=None):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = [i for i in range(len(w)) if not np.array_equal(g[i], w[i])]
            raise AssertionError(("column %d differs at rows" % k, bad[:10], [names[i] for i in bad[:10]] if names else None,
                                  [(g[i].tolist(), w[i].tolist()) for i in bad[:3]] if k < 2 else None))


def _columns_are_zero_where_the_header_says(got):
    st, kind, signer, sighash, offer_id, invreq_id = got
    own = (kind == 2) | (kind == 3)
    assert not kind[(st <= -1) & (st >= -3)].any() and kind[st < -3].all() and kind[st == 0].all()
    assert not signer[~((st == 0) & own)].any() and signer[(st == 0) & own].any(axis=1).all()
    assert not sighash[~(((st == 0) | (st == -8)) & own)].any() and sighash[((st == 0) | (st == -8)) & own].any(axis=1).all()
    assert not offer_id[st != 0].any() and offer_id[st == 0].any(axis=1).all()
    assert not invreq_id[~((st == 0) & own)].any() and invreq_id[(st == 0) & own].any(axis=1).all()


def test_fixture_strings_give_the_model_and_what_is_pinned(eng, fx):
    strings = sorted({r["str"] for r in fx["strings"]}) + [r["str"] for r in fx["fuzz"]]
    got = eng.bolt12_check(strings)
    _same(got, M.bolt12_check(strings))
    _columns_are_zero_where_the_header_says(got)
    p = M.pinned(fx, eng.bolt12_check)
    assert (p["ok_invoices"], p["ok_invreqs"], p["ok_offers"]) == (7, 2, 7)
    assert p["no_key_invreqs"] == ["tests/test_pay.py"]
    assert p["offers_with_offer_id"] >= 3 and p["invoices_with_offer_id"] >= 3
    assert p["invreqs_with_invreq_id"] >= 2 and p["invoices_with_invreq_id"] >= 1
    # an upper-cased reference string gives the same row as its lower-case twin
    for prefix in ("lno1", "lnr1", "lni1"):
        s = next(r["str"] for r in fx["strings"] if r["str"].startswith(prefix))
        a = eng.bolt12_check([s.upper(), s])
        assert a[0].tolist() == [0, 0] and all(np.array_equal(c[0], c[1]) for c in a)


def test_no_proper_prefix_of_a_reference_invoice_is_accepted(eng, fx):
    s = min((r["str"] for r in fx["strings"] if r["str"].startswith("lni1")), key=len)
    pre = [s[:k] for k in range(len(s))]
    got = eng.bolt12_check(pre)
    assert (got[0] != 0).all() and not got[2].any()
    _same(got, M.bolt12_check(pre))
    assert eng.bolt12_check([s])[0][0] == 0


def test_every_synthesised_class(eng):
    rows = M.synth()
    names, strings = [r[0] for r in rows], [r[1] for r in rows]
    got = eng.bolt12_check(strings)
    for name, want, g in zip(names, [r[2] for r in rows], got[0]):
        assert want is None or g == want, (name, want, int(g))
    _same(got, M.bolt12_check(strings), names)
    _columns_are_zero_where_the_header_says(got)
    assert {int(x) for x in got[0]} == set(range(-8, 1)) and {int(k) for k in got[1]} == {0, 1, 2, 3}
    by = {name: k for k, name in enumerate(names)}
    empty = np.frombuffer(M.EMPTY_ID, np.uint8)
    k = by["span/invoice-nothing-inside"]
    assert got[0][k] == 0 and np.array_equal(got[4][k], empty) and np.array_equal(got[5][k], empty)
    assert got[0][by["long/above-4096"]] == 0 and len(strings[by["long/above-4096"]]) > 4096


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_random_mixed_batches_and_their_shuffles(eng, pool, n):
    strings = M.random_batch(n, 2000 + n, pool)
    got = eng.bolt12_check(strings)
    _same(got, M.bolt12_check(strings))
    if n >= 63:
        assert set(got[1].tolist()) >= {1, 2, 3} and (got[0] == 0).sum() > n // 2 and (got[0] != 0).sum() >= n // 20
        assert len({len(s) for s in strings}) > 10
    # the same batch in another order: the permuted result (a row writing over a neighbour's scratch would show)
    perm = list(range(n))
    random.Random(n).shuffle(perm)
    again = eng.bolt12_check([strings[k] for k in perm])
    _same(again, [c[perm] for c in got])


def test_a_call_that_crosses_the_chunk_loop(eng, pool):
    """lamd_set_chunk_rows clamps at 4096: 4096 + 300 rows cross it once"""
    base = M.random_batch(314, 78, pool)
    strings = (base * 14)[:4396]
    want = M.bolt12_check(base)
    eng.set_chunk_rows(4096)
    try:
        got = eng.bolt12_check(strings)
    finally:
        eng.set_chunk_rows(0)
    _same(got, [np.concatenate([w] * 14)[:4396] for w in want])


def test_empty_batch_and_argument_checks(eng):
    got = eng.bolt12_check([])
    assert [c.shape for c in got] == [(0,), (0,), (0, 33), (0, 32), (0, 32), (0, 32)]
    lib, ctx = eng._lib, eng._ctx
    s = np.frombuffer(M.encode("lno", M.stream_of([(10, b"coffee")])), dtype=np.uint8)
    off = np.array([0, len(s)], dtype=np.uint64)
    status, kind, signer = np.zeros(1, np.int8), np.zeros(1, np.uint8), np.zeros(33, np.uint8)
    ARG = -3
    assert lib.lamd_bolt12_check_text_batch(ctx, 0, None, None, None, None, None, None, None, None) == 0
    good = [s.ctypes.data, off.ctypes.data, status.ctypes.data, kind.ctypes.data, signer.ctypes.data]
    assert lib.lamd_bolt12_check_text_batch(None, 1, *good, None, None, None) == ARG
    for k in range(5):
        a = list(good)
        a[k] = None
        assert lib.lamd_bolt12_check_text_batch(ctx, 1, *a, None, None, None) == ARG
    two = np.array([5, 9, 3], dtype=np.uint64)
    st2, kd2, sg2 = np.zeros(2, np.int8), np.zeros(2, np.uint8), np.zeros(66, np.uint8)
    assert lib.lamd_bolt12_check_text_batch(ctx, 2, s.ctypes.data, two.ctypes.data, st2.ctypes.data, kd2.ctypes.data, sg2.ctypes.data, None, None, None) == ARG
    # sighash32, offer_id32 and invreq_id32 may be NULL, each on its own
    want = M.bolt12_check([s.tobytes()])
    for k in range(3):
        cols = [np.zeros(32, np.uint8) for _ in range(3)]
        ptrs = [c.ctypes.data for c in cols]
        ptrs[k] = None
        status[0], kind[0] = 99, 99
        assert lib.lamd_bolt12_check_text_batch(ctx, 1, *good, *ptrs) == 0
        assert status[0] == want[0][0] == 0 and kind[0] == want[1][0] == 1
        for j in range(3):
            assert j == k or np.array_equal(cols[j], want[3 + j][0])


def test_timing_covers_the_new_launches(eng, fx):
    inv = sorted({r["str"] for r in fx["strings"] if r["str"].startswith("lni1")})
    strings = (inv * 64)[:64]
    eng.set_timing(True)
    try:
        st = eng.bolt12_check(strings)[0]
        t = eng.info()["last_text_ms"]
    finally:
        eng.set_timing(False)
    print("front end %.3f ms, key parse + curve work + merge %.3f ms at 64 strings" % (t[0], t[1]))
    assert t[0] > 0 and t[1] > 0 and (st == 0).all()

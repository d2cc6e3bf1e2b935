"""Engine.bolt11_check / Engine.checkmessage (lamd_bolt11_check_batch, lamd_checkmessage_batch) on the device against the sequential model
(tests/text_sig_model.py): the strings the reference's tests hold with what its asserts pin about them (tests/golden/text_signatures.json; the
line numbers are common/test/run-bolt11.c's and tests/test_misc.py's), every synthesised class, seeded random mixed batches, a call that crosses
the chunk loop, the empty batch and the argument checks.  Needs an MI355X: -m gpu."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_sig_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
KEY_310 = "03e7156ae33b0a208d0744199163177e909e80176e55d97a2f221ede0f934dd9ad"      # common/test/run-bolt11.c:310
HASH_KAT_B11 = "116fdb0f18352c886deb263f6466eb40e5e6518b80231a1f9df86088bfa48043"   # KAT-B11 (:465-467)


@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def _same(got, want, names=None):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = [i for i in range(len(w)) if not np.array_equal(g[i], w[i])]
            raise AssertionError(("column %d differs at rows" % k, bad[:10], [names[i] for i in bad[:10]] if names else None,
                                  [(g[i].tolist(), w[i].tolist()) for i in bad[:3]] if k == 0 else None))


def test_reference_invoices_give_what_the_reference_asserts(eng, fx):
    lines = [r["line"] for r in fx["invoices"]] + [fx["other_strings"][0]["line"]]
    strings = [r["str"] for r in fx["invoices"]] + [fx["other_strings"][0]["str"]]
    st, node, h, hn = eng.bolt11_check(strings)
    by = {ln: (int(s), bytes(k).hex(), bytes(x).hex()) for ln, s, k, x in zip(lines, st, node, h)}
    ok = [ln for ln in lines if by[ln][0] == 0]
    assert len(ok) == 26 and sum(by[ln][1] == KEY_310 for ln in ok) == 24 and all(by[ln][1] != "00" * 33 for ln in ok)   # row 1
    assert [by[ln][0] for ln in (495, 856, 863, 870)] == [-1] * 4                                  # rows 1, 2: "Bad bech32 string"
    assert by[877][0] == -6                                                                        # row 3: "signature recovery failed"
    assert by[884][0] == -3                                                                        # row 4: too short
    assert by[689][:2] == (0, KEY_310) and not hn.any()                                            # row 5: wrong-length `n` fields: recovery
    assert HASH_KAT_B11 in {by[ln][2] for ln in ok}                                                # row 8
    for ln in lines:
        if by[ln][0] != 0:
            assert by[ln][1] == "00" * 33
        if -3 <= by[ln][0] <= -1:
            assert by[ln][2] == "00" * 32
    _same((st, node, h, hn), M.bolt11_check(strings))
    # row 6: the upper-case string decodes like its lower-case twin
    up = next(r["str"] for r in fx["invoices"] if r["line"] == 520)
    a = eng.bolt11_check([up, up.lower()])
    assert a[0].tolist() == [0, 0] and np.array_equal(a[1][0], a[1][1]) and np.array_equal(a[2][0], a[2][1]) and bytes(a[1][0]).hex() == KEY_310


def test_no_proper_prefix_of_an_invoice_is_accepted(eng, fx):
    s = next(r["str"] for r in fx["invoices"] if r["line"] == 491)                                 # row 7 (the loop at :498)
    pre = [s[:k] for k in range(len(s))]
    st, node, h, hn = eng.bolt11_check(pre)
    assert (st != 0).all() and not node.any()
    _same((st, node, h, hn), M.bolt11_check(pre))
    assert eng.bolt11_check([s])[0][0] == 0


def test_every_synthesised_invoice_class(eng):
    rows = M.synth_invoices()
    names, strings = [r[0] for r in rows], [r[1] for r in rows]
    got = eng.bolt11_check(strings)
    for name, want, g in zip(names, [r[2] for r in rows], got[0]):
        assert want is None or g == want, (name, want, int(g))
    _same(got, M.bolt11_check(strings), names)
    assert {int(x) for x in got[0]} == set(range(-7, 1))
    assert got[3].sum() >= 10 and (got[0][got[3]] == 0).sum() >= 5


def test_checkmessage_triples_and_every_synthesised_class(eng, fx):
    trip = fx["checkmessage"]
    st, node = eng.checkmessage([t["message"] for t in trip], [t["zbase"] for t in trip])
    assert st.tolist() == [0] * len(trip) and [bytes(k).hex() for k in node] == [t["pubkey"] for t in trip]           # row 9
    st, node = eng.checkmessage([t["message"] + "modified" for t in trip], [t["zbase"] for t in trip])
    for t, s, k in zip(trip, st, node):                                                                                # row 10
        assert s == -4 or (s == 0 and bytes(k).hex() != t["pubkey"])
    _same((st, node), M.checkmessage([t["message"] + "modified" for t in trip], [t["zbase"] for t in trip]))
    rows, pub = M.synth_messages()
    names, msgs, zbs = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    got = eng.checkmessage(msgs, zbs)
    for name, want, g, k in zip(names, [r[3] for r in rows], got[0], got[1]):
        assert want is None or g == want, (name, want, int(g))
        if name.startswith("len/"):
            assert bytes(k) == pub
    _same(got, M.checkmessage(msgs, zbs), names)
    assert {int(x) for x in got[0]} == set(range(-4, 1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_random_mixed_batches(eng, n):
    strings = M.random_invoices(n, 1000 + n)
    got = eng.bolt11_check(strings)
    _same(got, M.bolt11_check(strings))
    if n >= 63:
        assert 0.25 * n < got[3].sum() < 0.75 * n and (got[0] == 0).sum() > n // 2 and (got[0] != 0).sum() >= n // 20


def test_a_call_that_crosses_the_chunk_loop(eng):
    """lamd_set_chunk_rows clamps at 4096: 4096 + 300 rows cross it once"""
    base = M.random_invoices(314, 77)
    strings = (base * 14)[:4396]
    S = M.Signer(5)
    sec, pub = S.key()
    msgs = [b"message %d" % i for i in range(150)]
    zbs = [M.signed_message(S, m, sec, pub) for m in msgs]
    zbs[7] = zbs[8]
    msgs, zbs = (msgs * 30)[:4396], (zbs * 30)[:4396]
    want = M.bolt11_check(base)
    mwant = M.checkmessage(msgs[:150], zbs[:150])
    eng.set_chunk_rows(4096)
    try:
        got = eng.bolt11_check(strings)
        mgot = eng.checkmessage(msgs, zbs)
    finally:
        eng.set_chunk_rows(0)
    _same(got, [np.concatenate([w] * 14)[:4396] for w in want])
    _same(mgot, [np.concatenate([w] * 30)[:4396] for w in mwant])
    assert (mgot[0] == 0).sum() >= 4396 - 60 and all(bytes(k) == pub for k, s in zip(mgot[1][:7], mgot[0][:7]) if s == 0)


def test_empty_batch_and_argument_checks(eng):
    st, node, h, hn = eng.bolt11_check([])
    assert st.shape == (0,) and node.shape == (0, 33) and h.shape == (0, 32) and hn.shape == (0,)
    st, node = eng.checkmessage([], [])
    assert st.shape == (0,) and node.shape == (0, 33)
    lib, ctx = eng._lib, eng._ctx
    s = np.frombuffer(b"lnbc1qqqqqqqq", dtype=np.uint8)
    off = np.array([0, len(s)], dtype=np.uint64)
    status, node = np.zeros(1, np.int8), np.zeros(33, np.uint8)
    ARG = -3
    assert lib.lamd_bolt11_check_batch(ctx, 0, None, None, None, None, None, None) == 0
    assert lib.lamd_checkmessage_batch(ctx, 0, None, None, None, None, None, None) == 0
    assert lib.lamd_bolt11_check_batch(None, 1, s.ctypes.data, off.ctypes.data, status.ctypes.data, node.ctypes.data, None, None) == ARG
    for k in range(4):
        a = [s.ctypes.data, off.ctypes.data, status.ctypes.data, node.ctypes.data]
        a[k] = None
        assert lib.lamd_bolt11_check_batch(ctx, 1, *a, None, None) == ARG
    for k in range(6):
        a = [s.ctypes.data, off.ctypes.data, s.ctypes.data, off.ctypes.data, status.ctypes.data, node.ctypes.data]
        a[k] = None
        assert lib.lamd_checkmessage_batch(ctx, 1, *a) == ARG
    # hash32 and have_n may be NULL
    assert lib.lamd_bolt11_check_batch(ctx, 1, s.ctypes.data, off.ctypes.data, status.ctypes.data, node.ctypes.data, None, None) == 0 and status[0] == -1


def test_timing_covers_the_new_launches(eng):
    strings = M.random_invoices(64, 3)
    eng.set_timing(True)
    try:
        eng.bolt11_check(strings)
        t = eng.info()["last_text_ms"]
    finally:
        eng.set_timing(False)
    print("front end %.3f ms, key parse + curve work + merge %.3f ms at 64 invoices" % (t[0], t[1]))
    assert t[0] > 0 and t[1] > 0

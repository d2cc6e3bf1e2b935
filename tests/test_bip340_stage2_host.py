"""CPU side of the verdict-byte contract (include/lightning_amd.h: every verdict byte the library writes is 0 or 1) and of the BIP-340 rows that
only stage 2 can decide (bip340_stage2.py): the two strict readers; the generator against the C oracle and pyref; and the host build of the
device code (devmath_host.cpp: schnorr_stage1 per row, then schnorr_final_thread per thread) over planted columns, raw bytes compared exactly
with the construction.  test_gpu_verdict_bytes.py is the device side."""
import ctypes

import numpy as np
import pytest

import bip340_stage2 as st2
import pyref
from test_devmath_host import dm  # noqa: F401  (the fixture that builds and loads libdevmath_host.so)
from verdict_bytes import strict_bool


# ---- the strict readers
@pytest.mark.parametrize("byte", [2, 3, 9])
def test_strict_readers_refuse_markers_and_unwritten_rows(byte):
    from lightning_amd.engine import LamdError, _verdicts
    raw = np.array([1, 0, 1, 1, byte, 0, byte], dtype=np.uint8)
    with pytest.raises(AssertionError, match=r"\(4, %d\)" % byte):
        strict_bool(raw)
    with pytest.raises(LamdError, match="verdict byte %d at row 4 " % byte):
        _verdicts(raw)
    with pytest.raises(LamdError, match="at row 0 "):
        _verdicts(raw[4:5])


def test_strict_readers_pass_zero_and_one():
    from lightning_amd.engine import _verdicts
    raw = np.array([1, 0, 0, 1, 1], dtype=np.uint8)
    for read in (strict_bool, _verdicts):
        got = read(raw)
        assert got.dtype == bool and got.tolist() == [True, False, False, True, True]
        assert read(np.zeros(0, dtype=np.uint8)).shape == (0,)
    assert strict_bool(np.array([[1, 0], [0, 1]], dtype=np.uint8)).shape == (2, 2)


# ---- the generator
def test_pool_classes_are_what_the_oracles_say(orc):
    rows = st2.pool()
    assert len(rows) <= 256 and len({r.pk for r in rows}) == st2.NKEYS
    cls = st2.by_class(rows)
    assert all(len(cls[c]) >= 32 for c in st2.CLASSES)
    assert {r.tag for r in cls["R_inf"]} == {"r=curve_x", "r=no_sqrt", "r=zero", "r=one"}
    m, k, s, exp = st2.columns(rows)
    assert np.array_equal(strict_bool(orc.schnorr_verify_batch(m, k, s, 4)), exp)
    assert [pyref.schnorr_verify(r.msg, r.pk, r.sig) for r in rows] == exp.tolist()
    for i, r in enumerate(rows):
        if r.cls in ("odd_R", "even_R"):
            t = rows[r.twin]
            assert t.twin == i and {r.cls, t.cls} == {"odd_R", "even_R"} and (t.pk, t.msg, t.sig[:32]) == (r.pk, r.msg, r.sig[:32]) and t.sig != r.sig
    # what makes the classes what they are: R = s*G - e*P itself
    for r in cls["odd_R"][:6] + cls["even_R"][:6] + cls["R_inf"][:8] + cls["flip"][:6]:
        e = st2._challenge(r.sig[:32], r.pk, r.msg)
        R = pyref.padd(pyref.pmul(int.from_bytes(r.sig[32:], "big"), pyref.G), pyref.pmul(pyref.N - e, pyref.lift_x(int.from_bytes(r.pk, "big"))))
        rx = int.from_bytes(r.sig[:32], "big")
        if r.cls == "R_inf":
            assert R is None
        elif r.cls == "flip":
            assert R is not None and R[0] != rx
        else:
            assert R[0] == rx and (R[1] & 1) == (r.cls == "odd_R")


def test_patterns_cover_the_listed_orders():
    O, E, I, F = "odd_R", "even_R", "R_inf", "flip"
    p3 = dict(st2.patterns(3))
    assert list(p3.values()) == [[O, O, O], [O, E, E], [E, O, E], [E, E, O], [O, F, O], [F, O, F], [F, F, O], [O, F, F], [E, I, E], [I, O, I]]
    p4 = dict(st2.patterns(4))
    assert set(p4) >= set(p3) - {"odd_middle1"} and all(len(v) == 4 for v in p4.values())
    assert p4["flip_odd_flip"] == [E, F, O, F] and p4["odd_flip_odd"] == [O, F, O, E] and p4["inf_odd_inf"] == [E, I, O, I]
    assert [n for n, _ in st2.patterns(1)] == ["all_odd"] and [v for _, v in st2.patterns(2)] == [[O, O], [O, E], [E, O]]
    assert st2.final_stride(196625, 256) == 65536 and st2.final_stride(1 << 20, 256) == 65536 and st2.final_stride(5000, 256) == 5120
    assert st2.final_stride(1 << 21, 256) == 1 << 17


# ---- the host build of the device code
def _device_code(dm, cols, threads):
    n = len(cols[0])
    out = ctypes.create_string_buffer(bytes([9]) * n, n)
    dm.dm_schnorr_verify_batch2(ctypes.c_size_t(n), cols[0].tobytes(), cols[1].tobytes(), cols[2].tobytes(), out, ctypes.c_size_t(threads))
    return np.frombuffer(out.raw, dtype=np.uint8)


def _check(raw, exp, planted, what):
    """the raw bytes are the construction's, exactly: first the markers, then the verdicts"""
    loose = raw != 0                                        # what a caller's `if (!ok[i])` sees
    bad = np.flatnonzero(loose != exp)
    differ = ("%d rows differ" % bad.size, [(int(i), planted[int(i)], "accepted" if loose[i] else "rejected") for i in bad[:8]])
    assert set(np.unique(raw).tolist()) <= {0, 1}, (what, "bytes equal to", sorted(set(np.unique(raw).tolist()) - {0, 1}),
                                                   "at rows", np.flatnonzero(raw > 1)[:8].tolist(), "read as non-zero = accept:", differ)
    assert not bad.size and np.array_equal(strict_bool(raw), exp), (what, differ)


N_HOST = 600


@pytest.fixture(scope="module")
def base():
    return st2.tiled(N_HOST, seed=11)


@pytest.mark.parametrize("threads,lengths", [(400, (1, 2)), (190, (3, 4)), (38, (15, 16)), (N_HOST, (1,)), (N_HOST + 37, (1,)), (4 * N_HOST, (1,))])
def test_planted_chains_through_the_host_build(dm, orc, base, threads, lengths):
    """600 pool rows, every pattern planted along chains of the lengths this `threads` gives (1 and 2; 3 and 4; 15 and 16), and threads >= n, where
    some threads own nothing"""
    rows, m, k, s, exp = base
    cols, exp = [m.copy(), k.copy(), s.copy()], exp.copy()
    planted = st2.plant(cols, exp, threads, lengths, seed=threads)
    classes = {**{i: r.cls for i, r in enumerate(rows)}, **planted["classes"]}
    for length in lengths:
        want = [n for n, _ in st2.patterns(length)]
        if length == 15:                                    # 8 chains of 15 rows beside the 30 of 16
            want = want[:8]
        assert [n for _, n in planted["chains"][length]] == want, (length, planted["chains"][length])
        for p, _ in planted["chains"][length]:
            assert len(range(p, N_HOST, threads)) == length
    assert np.array_equal(strict_bool(orc.schnorr_verify_batch(*cols, 4)), exp)
    _check(_device_code(dm, cols, threads), exp, classes, ("threads", threads))


@pytest.mark.parametrize("threads", [16, 150, N_HOST, 1000])
def test_fifty_fifty_block_through_the_host_build(dm, orc, base, threads):
    """a contiguous block of 256 rows, odd_R or even_R by the seed, inside the 600: chains of 37 and 38 rows, of 4, of 1"""
    rows, m, k, s, exp = base
    cols, exp = [m.copy(), k.copy(), s.copy()], exp.copy()
    planted = st2.plant(cols, exp, threads, (), seed=5, block=200, block_rows=256)
    classes = {**{i: r.cls for i, r in enumerate(rows)}, **planted["classes"]}
    blk = [planted["classes"][i] for i in range(200, 456)]
    assert planted["block"] == (200, 256) and 96 <= blk.count("odd_R") <= 160 and set(blk) == {"odd_R", "even_R"}
    if threads <= 16:
        assert all(len({blk[j] for j in range(t, 256, threads)}) == 2 for t in range(threads))      # both classes in every chain
    assert np.array_equal(strict_bool(orc.schnorr_verify_batch(*cols, 4)), exp)
    _check(_device_code(dm, cols, threads), exp, classes, ("block, threads", threads))

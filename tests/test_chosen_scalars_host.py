"""The accepting rows at chosen u1, u2 (chosen_scalars.py) checked on the CPU, so that a failure of test_gpu_chosen_scalars.py can be told from a wrong
generator or from wrong shared arithmetic: every row and every near-miss twin against the construction, the C oracle and the OpenSSL restatement
(pyref on a structured subset), the caps on what the low-S rule makes unreachable, and -- with 8-bit windows, the host harness's G table -- the rows
through the device arithmetic compiled for the host: the verification pipeline, the comb, the pairs-first form, the task split, recovery."""
import ctypes
import random

import numpy as np
import pytest

import chosen_scalars as cs
import pyref
from test_devmath_host import dm  # noqa: F401  (the host build of the device headers, a session fixture)

N = pyref.N
BITS = 24                            # the shipped G table walk (verify_core.h GTABLE_WINDOW_BITS)


def _verify_opinions(orc, rows, publen):
    hs, sg, pk = cs.columns(rows, publen)
    return orc.ecdsa_verify_batch(hs, sg, pk, publen, 4).astype(bool), orc.ossl_ecdsa_verify_rules_batch(hs, sg, pk, publen, 4).astype(bool)


def test_the_lists_are_what_their_names_say():
    for bits in (24, 8, 11):
        pats = cs.u1_patterns(bits)
        cs.check_u1_patterns(bits, pats)
        assert cs.u1_patterns(bits) == pats                                  # seeded
    assert cs.windows(24) == 11 and cs.task_groups(24) == ([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]], [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10]])
    assert len(cs.u1_patterns(24)) == 4 * 11 + 11 + 6 + 15 + 2 + 7
    u2s = cs.u2_list()
    assert set(u2s) >= {v for v in cs.U2_COMB + cs.U2_LADDER if v} and len(set(u2s)) == len(u2s) and 0 not in u2s
    assert len(u2s) == len({v for v in cs.U2_COMB + cs.U2_LADDER if v}) + cs.N_RANDOM_U2
    for u, w0 in ((0, 0), (1, 0), (N - 1, 10), (N - 1, 0), ((1 << 240) - 1, 3), (1 << 255, 10), (0xFFFF << 240, 10)):
        v, w = cs.near_miss_u1(u, 24, w0)
        assert 0 <= v < N and abs(v - u) == 1 << (24 * w)
        assert [a != b for a, b in zip(cs.digits(u, 24), cs.digits(v, 24))].count(True) == 1
        assert abs(cs.digit(u, 24, w) - cs.digit(v, 24, w)) == 1


@pytest.mark.parametrize("name", ["own", "fixed"])
def test_verification_rows_three_opinions(orc, name):
    """every accepting row accepts and every twin rejects for the C oracle and for OpenSSL's arithmetic (33- and 65-byte keys); the pair a row hits,
    recomputed from (z, r, s), is the pair it was asked for; pyref agrees on the structured rows"""
    rows = cs.row_sets(orc, BITS)[name]
    exp = np.array([r.expect for r in rows], dtype=bool)
    assert len(rows) > 800 and exp[0::2].all() and not exp[1::2].any()
    for publen in (33, 65):
        c, o = _verify_opinions(orc, rows, publen)
        assert np.array_equal(c, exp), [rows[i].tag for i in np.nonzero(c != exp)[0][:10]]
        assert np.array_equal(o, exp), [rows[i].tag for i in np.nonzero(o != exp)[0][:10]]
    for r, t in zip(rows[0::2], rows[1::2]):
        assert r.exact(), r.tag
        assert int.from_bytes(r.sig[32:], "big") <= N // 2 and t.sig == r.sig and t.key == r.key and t.u2 == r.u2
        d = [a != b for a, b in zip(cs.digits(r.u1, BITS), cs.digits(t.u1, BITS))]
        assert d.count(True) == 1 and abs(r.u1 - t.u1) == 1 << (BITS * d.index(True)), r.tag
    structured = [i for i, r in enumerate(rows) if r.tag.startswith("u1:") or r.tag.startswith("x:")][::3]   # (rows AND twins)
    assert len(structured) > 200
    for i in structured[:150]:
        r = rows[i]
        assert pyref.ecdsa_verify(r.hash, r.sig, r.key) == r.expect, r.tag
        if r.expect:                                                         # the point itself: R = u1*G + u2*Q has x = r
            Q = (int.from_bytes(r.key[1:33], "big"), int.from_bytes(r.key[33:], "big"))
            R = pyref.padd(pyref.pmul(r.u1, pyref.G), pyref.pmul(r.u2, Q))
            assert R[0] % N == int.from_bytes(r.sig[:32], "big"), r.tag


@pytest.mark.parametrize("name", ["recover", "recover_shared"])
def test_recovery_rows_three_opinions(orc, name):
    """every recovery row returns the key of the construction, every twin another key, for the C oracle and OpenSSL's arithmetic; pyref on the
    structured rows.  recover_shared: 32 rows (64 with twins) per r."""
    rows = cs.row_sets(orc, BITS)[name]
    hs, sg, rid = cs.columns(rows)
    keys, ok = orc.ecdsa_recover_batch(hs, sg, rid, 4)
    nr = len({r.sig[:32] for r in rows})
    assert nr == len(rows) // 2 if name == "recover" else nr == (len(rows) // 2 + 31) // 32
    for i, r in enumerate(rows):
        got = keys[i].tobytes() if ok[i] else None
        assert got == orc.ossl_ecdsa_recover(r.hash, r.sig, r.recid), r.tag
        if i % 2 == 0:
            assert r.exact() and got == r.expect, r.tag
        else:
            assert got != rows[i - 1].expect and r.sig == rows[i - 1].sig and r.u2 == rows[i - 1].u2, r.tag
    for i in [i for i, r in enumerate(rows) if r.tag.startswith("u1:") or r.tag.startswith("x:")][::9]:
        r = rows[i]
        e = pyref.ecdsa_recover(r.hash, r.sig, r.recid)
        assert (pyref.ser33(e) if e else None) == (keys[i].tobytes() if ok[i] else None), r.tag


def test_caps_unreachable_share_and_every_pattern_reached(orc):
    """the low-S rule makes a both-sides-structured pair unreachable under a fixed pool of 8 keys about once in 256: at the committed seed at most one
    pair in 64 of the WHOLE cross product, every reachable one accepted by both oracles -- and on every path's row set every u1 window pattern is hit
    exactly by an accepting row"""
    pairs = cs.cross_product(BITS)
    rows, unreachable = cs.verify_rows_fixed_keys(orc, random.Random(cs.SEED), pairs, cs.key_pool())
    assert len(rows) + len(unreachable) == len(pairs) == len(cs.u1_patterns(BITS)) * len(cs.u2_list())
    assert 64 * len(unreachable) <= len(pairs), (len(unreachable), len(pairs))
    assert all(r.exact() for r in rows)
    c, o = _verify_opinions(orc, rows, 33)
    assert c.all() and o.all()
    sets = cs.row_sets(orc, BITS)
    sample = sum(1 for t, _, _ in cs.pair_lists(BITS)[2])
    assert 64 * len(sets["unreachable"]) <= sample
    names = {n for n, _ in cs.u1_patterns(BITS)}
    for path in ("own", "fixed", "recover", "recover_shared"):
        assert cs.reached_patterns(sets[path], BITS) == names, (path, sorted(names - cs.reached_patterns(sets[path], BITS)))
        u2hit = {r.u2 for r in sets[path][0::2] if r.exact()}
        assert u2hit >= set(cs.u2_list()), path


def _push(fn, rows, publen, *args):
    hs, sg, pk = cs.columns(rows, publen)
    out = ctypes.create_string_buffer(len(rows))
    fn(*args, hs.tobytes(), sg.tobytes(), pk.tobytes(), publen, out)
    return np.frombuffer(out.raw, dtype=np.uint8)


def test_rows_through_the_host_build_of_the_device_code(dm, orc):  # noqa: F811
    """the same constructions aimed at the host harness's 8-bit windows (32 of them: 16 pairs, task groups of 8, ladder halves of 16), through the
    verification pipeline (ecmult_lane: the entry test_pipeline_random_vs_oracle uses), the comb (ecmult_lane_keyed_fast, 7 and 10 teeth), the
    pairs-first form (batches of 1 and 6 rows) and the task split of the latency path (comb 7 / 10 and the ladder halves, the four-wave merge);
    recovery through dm_recover_batch.  Verdicts are the construction's, which the C oracle confirms; a verdict byte that is neither 0 nor 1
    (the harness's "forms disagree" markers) fails too."""
    bits = dm.dm_gtable_window_bits()
    assert bits == 8
    sets = cs.row_sets(orc, bits, per=1)
    names = {n for n, _ in cs.u1_patterns(bits)}
    dm.dm_verify_pairs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    for path in ("own", "fixed"):
        rows = sets[path]
        exp = np.array([r.expect for r in rows], dtype=np.uint8)
        assert cs.reached_patterns(rows, bits) == names and exp[0::2].all() and not exp[1::2].any()
        hs, sg, pk = cs.columns(rows, 33)
        assert np.array_equal(orc.ecdsa_verify_batch(hs, sg, pk, 33, 4), exp)

        def check(got, what):
            assert np.array_equal(got, exp), (path, what, [(rows[i].tag, int(got[i])) for i in np.nonzero(got != exp)[0][:10]])

        publen, threads = (33, 5) if path == "own" else (65, 1)
        out = ctypes.create_string_buffer(len(rows))
        c = cs.columns(rows, publen)
        dm.dm_ecdsa_verify_batch(ctypes.c_size_t(len(rows)), c[0].tobytes(), c[1].tobytes(), c[2].tobytes(), publen, publen, out, ctypes.c_size_t(threads))
        check(np.frombuffer(out.raw, dtype=np.uint8), "pipeline")
        if path == "own":                                                    # rows under keys of their own: the ladder halves of the task split
            check(_push(dm.dm_verify_split, rows, 33, 0, 0, ctypes.c_size_t(len(rows))), "split 0")
            continue
        # the table shapes (the harness builds a table per row: 512 entries for 10 teeth, so that shape takes the rows that aim at the comb --
        # every u2, half of the cross product -- and leaves the u1-only rows, whose G walk is the same code, to the 7-tooth runs)
        keep = [i for i in range(0, len(rows), 2) if rows[i].tag.startswith("u2:") or (rows[i].tag.startswith("x:") and i % 4 == 0)]
        sub = np.array(sorted(keep + [i + 1 for i in keep]))
        assert {r.u2 for r in (rows[i] for i in keep)} >= set(cs.u2_list()) and len(keep) > 150
        full_rows, full_exp = rows, exp
        for T in (7, 10):
            if T == 10:
                rows, exp = [full_rows[i] for i in sub], full_exp[sub]
            check(_push(dm.dm_verify_keyed, rows, 33, 0, T, ctypes.c_size_t(len(rows))), ("comb", T))
            for batch in ((1, 6) if T == 7 else (6,)):
                check(_push(dm.dm_verify_pairs, rows, 65 if batch == 1 else 33, 0, T, len(rows), batch), ("pairs", T, batch))
            check(_push(dm.dm_verify_split, rows, 33, 0, T, ctypes.c_size_t(len(rows))), ("split", T))
    for path, threads in (("recover", 1), ("recover_shared", 7)):
        rows = sets[path]
        assert cs.reached_patterns(rows, bits) == names
        hs, sg, rid = cs.columns(rows)
        ck, cok = orc.ecdsa_recover_batch(hs, sg, rid, 4)
        for threads in (threads,):
            pub, ok = ctypes.create_string_buffer(33 * len(rows)), ctypes.create_string_buffer(len(rows))
            dm.dm_recover_batch(ctypes.c_size_t(len(rows)), hs.tobytes(), sg.tobytes(), rid.tobytes(), pub, ok, ctypes.c_size_t(threads))
            for i, r in enumerate(rows):
                got = pub.raw[33 * i:33 * i + 33] if ok.raw[i] else None
                assert got == (ck[i].tobytes() if cok[i] else None), (path, r.tag)
                assert got == r.expect if i % 2 == 0 else got != rows[i - 1].expect, (path, r.tag)

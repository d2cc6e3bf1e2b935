"""The table-driven ecmult's comb column on the device (k_ecmult_keyed<false>: the column's two table points summed first, that pair added to the
accumulator): verdicts against the C oracle for both comb shapes, at the wave boundaries, in the wave that holds both shapes, and for scalars
chosen to stress the recoding and to end at infinity.  Needs an MI355X: -m gpu."""
import os
import random

import numpy as np
import pytest
import torch

import chosen_scalars as cs
import pyref
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu
N = pyref.N
KEYS = (0x1F2E3D4C5B6A79881726354453627180AABBCCDDEEFF00112233445566778899, 0x6C1F00D5A3E2B4C7918D7E6F5A4B3C2D1E0F99887766554433221100FFEEDDCC)


def _rows(rows, w):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), w)


def _engine(env):
    from lightning_amd import Engine
    os.environ.update(env)
    try:
        return Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module", params=[7, 10])
def eng_keyed(request):
    """engine forced onto per-key comb tables of one shape whenever a key has two rows"""
    e = _engine({"LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(request.param)})
    e.teeth = request.param
    yield e
    e.close()


def _on_device(e, mode, cols):
    """the device-buffer entry points: the general path whatever the batch size (host buffers of <= 64 rows take the one-launch latency path)"""
    dev = [torch.from_numpy(np.array(c)).cuda() for c in cols]
    d_ok = torch.zeros(len(cols[0]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    (e.verify_ecdsa_device if mode == "ecdsa" else e.verify_schnorr_device)(dev[0], dev[1], dev[2], d_ok)
    e.synchronize()
    return strict_bool(d_ok.cpu().numpy())


def _ecdsa65(orc, rnd, keys):
    """one row per entry of keys (secret keys), 65-byte public keys, about one in ten with a damaged hash"""
    hs, sg, pk = [], [], []
    for i, d in enumerate(keys):
        h = rnd.randbytes(32)
        sg.append(orc.ecdsa_sign(h, d.to_bytes(32, "big"), rnd.randrange(1, N).to_bytes(32, "big")))
        pk.append(orc.pubkey_create(d.to_bytes(32, "big")))
        hs.append(bytes([h[0] ^ 0x10]) + h[1:] if i % 10 == 1 else h)
    return _rows(hs, 32), _rows(sg, 64), _rows(pk, 65)


def _bip340(orc, rnd, keys):
    ms, ks, sg = [], [], []
    for i, d in enumerate(keys):
        m = rnd.randbytes(32)
        sg.append(orc.schnorr_sign(m, d.to_bytes(32, "big"), rnd.randbytes(32)))
        ks.append(orc.pubkey_create(d.to_bytes(32, "big"))[1:33])
        ms.append(bytes([m[0] ^ 0x10]) + m[1:] if i % 10 == 1 else m)
    return _rows(ms, 32), _rows(ks, 32), _rows(sg, 64)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_two_keys_at_the_wave_boundaries(eng_keyed, orc, n):
    """n rows over two keys (alternating), ECDSA-65 and BIP-340, 7 and 10 teeth: a partial wave, the wave boundary, a few grid strides.  Two
    rows alternating are one row per key -- no table -- so n = 2 also runs with both rows under one key."""
    e = eng_keyed
    rnd = random.Random(7000 + 16 * e.teeth + n)
    layouts = [[KEYS[i % 2] for i in range(n)]] + ([[KEYS[0]] * n] if n == 2 else [])
    for keys in layouts:
        tabled = all(keys.count(k) >= 2 for k in set(keys))
        cols = _ecdsa65(orc, rnd, keys)
        exp = orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], 65, 2).astype(bool)
        assert 0 < exp.sum() < n
        e.cache_clear()
        got = _on_device(e, "ecdsa", cols)
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
        inf = e.info()
        assert (inf["last_keyed"], inf["last_hot_rows"]) == ((e.teeth, n) if tabled else (0, 0)), inf
        assert np.array_equal(e.verify_ecdsa(*cols), exp)
        cols = _bip340(orc, rnd, keys)
        exp = orc.schnorr_verify_batch(cols[0], cols[1], cols[2], 2).astype(bool)
        assert 0 < exp.sum() < n
        e.cache_clear()
        got = _on_device(e, "schnorr", cols)
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
        inf = e.info()
        assert (inf["last_keyed"], inf["last_hot_rows"]) == ((e.teeth, n) if tabled else (0, 0)), inf
        assert np.array_equal(e.verify_schnorr(*cols), exp)


def test_one_wave_holding_both_comb_shapes_and_cold_rows(orc):
    """the default thresholds: a key with 48 rows gets the 10-tooth comb, a key with 6 rows the 7-tooth comb, three keys met once get none --
    57 rows, one batch, so ONE wave of the ecmult kernel straddles list7 | list10 and runs both bodies, with the ladder's rows beside it"""
    rnd = random.Random(4806)
    keys = [KEYS[0]] * 48 + [KEYS[1]] * 6 + [rnd.randrange(1, N) for _ in range(3)]
    rnd.shuffle(keys)
    e = _engine({"LAMD_KEYED_MIN_ROWS": "1"})      # (a batch this small would otherwise be looked up in the cache only)
    try:
        for mode, cols in (("ecdsa", _ecdsa65(orc, rnd, keys)), ("schnorr", _bip340(orc, rnd, keys))):
            if mode == "ecdsa":
                exp = orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], 65, 2).astype(bool)
            else:
                exp = orc.schnorr_verify_batch(cols[0], cols[1], cols[2], 2).astype(bool)
            assert 45 <= exp.sum() < 57
            e.cache_clear()
            got = _on_device(e, mode, cols)
            assert np.array_equal(got, exp), (mode, np.nonzero(got != exp)[0][:10])
            inf = e.info()
            assert (inf["last_keyed"], inf["last_hot_rows"], inf["last_cold_rows"], inf["last_new_tables"]) == (10, 54, 3, 2), inf
    finally:
        e.close()


def test_chosen_scalars_through_the_comb(eng_keyed, orc):
    """ECDSA rows with s = 1, r = u2, hash = u1 verify u1*G + u2*Q for exactly those scalars: u2 from the list that stresses the recoding
    (+-lambda, lambda +- 1, 2^127, 2^128 +- 1, n - 1, ..), u1 tiny, random, and the values that make the result infinity or G (rows that meet
    Z = 0, reported SUSPECT and decided by the complete formulas).  Every verdict is the oracle's."""
    e = eng_keyed
    d = KEYS[1]
    rng = random.Random(77)
    u2s = cs.U2_COMB + [rng.randrange(1, N) for _ in range(12)]                                                # (u2 = 0 is r = 0: not a signature)
    pub = orc.pubkey_create(d.to_bytes(32, "big"))
    hs, sg, ninf = [], [], 0
    for u2 in u2s:
        for u1 in (1, rng.randrange(1, N), (-u2 * d) % N, (-u2 * d + 1) % N):                                 # (u1 = 0 is skipped with the list's u2 = 0)
            ninf += u1 == (-u2 * d) % N
            hs.append(u1.to_bytes(32, "big"))
            sg.append(u2.to_bytes(32, "big") + (1).to_bytes(32, "big"))
    cols = (_rows(hs, 32), _rows(sg, 64), _rows([pub] * len(hs), 65))
    exp = orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], 65, 2).astype(bool)
    for u2, got in zip(u2s, exp.reshape(len(u2s), -1)):
        assert not got[2]                                   # the row whose sum is infinity is no signature
    e.cache_clear()
    got = _on_device(e, "ecdsa", cols)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    inf = e.info()
    assert inf["last_keyed"] == e.teeth and inf["last_hot_rows"] == len(hs) and inf["last_suspect_rows"] >= ninf == len(u2s), inf
    assert np.array_equal(e.verify_ecdsa(*cols), exp)       # > 64 rows from host memory: the same path


def test_chosen_scalars_through_the_comb_accepting(eng_keyed, orc):
    """the same u2 list on rows that ACCEPT iff the comb computes exactly u1*G + u2*Q (chosen_scalars.py: r = x(R), s = r/u2, hash = u1*s under the two
    keys above; u1 random, redrawn until s is low, and u1 = 0, 1 where one of the keys gives a low s), each with its near-miss twin (one digit of
    the G walk off by one: rejects), next to the rows whose sum is infinity: a comb that computes a wrong point at u2 = lambda + 1 fails here, where
    the test above -- every expected verdict False -- would not notice.  The suspect counter and the infinity rows are checked as above."""
    e = eng_keyed
    rng = random.Random(78)
    u2s = cs.U2_COMB + [rng.randrange(1, N) for _ in range(12)]
    pairs = [("u2:%d" % j, None, u2) for j, u2 in enumerate(u2s)] + [("u1=%d:%d" % (u1, j), u1, u2) for u1 in (0, 1) for j, u2 in enumerate(u2s)]
    acc, unreachable = cs.verify_rows_fixed_keys(orc, rng, pairs, list(KEYS))
    assert sum(r.tag.startswith("u2:") for r in acc) == len(u2s) and all(r.exact() for r in acc)      # every u2 of the list is hit exactly
    assert len(acc) + len(unreachable) == len(pairs) and len(unreachable) < len(u2s)                  # (two keys: a pair is out of reach once in four)
    rows = cs.with_twins(acc, 24)
    pub = orc.pubkey_create(KEYS[1].to_bytes(32, "big"))
    for u2 in u2s:                                           # s = 1, r = u2, hash = u1 = -u2*d: the sum is infinity
        rows.append(cs.Row("verify", ((-u2 * KEYS[1]) % N).to_bytes(32, "big"), u2.to_bytes(32, "big") + (1).to_bytes(32, "big"), pub, (None, u2), "inf", expect=False))
    cols = cs.columns(rows, 65)
    exp = orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], 65, 2).astype(bool)
    assert np.array_equal(exp, np.array([r.expect for r in rows], dtype=bool)) and 0 < exp.sum() == len(acc)
    e.cache_clear()
    got = _on_device(e, "ecdsa", cols)
    assert np.array_equal(got, exp), [(rows[i].tag, hex(rows[i].u1), hex(rows[i].u2)) for i in np.nonzero(got != exp)[0][:10]]
    inf = e.info()
    assert inf["last_keyed"] == e.teeth and inf["last_hot_rows"] == len(rows) and inf["last_suspect_rows"] >= len(u2s), inf
    assert np.array_equal(e.verify_ecdsa(*cols), exp)       # > 64 rows from host memory: the same path

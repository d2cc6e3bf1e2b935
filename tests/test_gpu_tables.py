"""Every entry of the tables the device builds for itself, against ground truth.

The static G table (11 windows x 2^24 entries, 11 GiB): lamd_debug_gtable_audit judges every entry on the device from field multiplications alone
(lightning_amd/csrc/table_audit.h -- no group-law code, no inversion, nothing k_gtable_build ran); negative controls show that it flags exactly what is
wrong; a sample read back to the host is compared with the C oracle and pyref, which trust nothing of the device.  The per-key comb tables (7 and 10
teeth, both builders): every entry of every table a batch built, read back and compared with the oracle."""
import os
import random

import numpy as np
import pytest

import pyref

import gtable_cases as gc
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu

P, N = pyref.P, pyref.N
BITS, NWIN = 24, 11
ENTRIES = NWIN << BITS
LAST = (1 << BITS) - 1
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72


class _Engines:
    """the module's engines: one plain Engine(0) and the keyed ones, made on demand"""

    def __init__(self):
        self.plain, self.keyed = None, {}

    def eng(self):
        if self.plain is None:
            from lightning_amd import Engine
            self.plain = Engine(0)
        return self.plain

    def eng_keyed(self, T, tree):
        """as the eng_keyed fixture of tests/test_gpu_parity.py, plus the choice of the table builder"""
        self.eng()
        if (T, tree) not in self.keyed:
            from lightning_amd import Engine
            env = {"LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(T), "LAMD_KC_TREE": str(tree)}
            os.environ.update(env)
            try:
                self.keyed[(T, tree)] = Engine(0)
            finally:
                for k in env:
                    del os.environ[k]
        return self.keyed[(T, tree)]

    def close_all(self):
        for e in list(self.keyed.values()) + ([self.plain] if self.plain is not None else []):
            e.close()
        self.plain, self.keyed = None, {}


@pytest.fixture(scope="module")
def engines():
    es = _Engines()
    yield es
    es.close_all()


@pytest.fixture
def eng(engines):
    return engines.eng()


def _read_entries(e, first, count):
    """entries [first, first + count) of the engine's G table as uint32 [count, 16]"""
    return e.debug_read(e.READ_GTABLE, first * 64, count * 64).view(np.uint32).reshape(count, 16).copy()


def _upload(img):
    import torch
    return torch.from_numpy(np.array(img, dtype=np.uint32).view(np.int32)).cuda()


def _reasons(res, first, count):
    """the audit's report as a reason mask per entry of the range (complete when it fits the report list)"""
    assert res["bad"] == len(res["listed"]), res["bad"]
    r = np.zeros(count, dtype=np.uint32)
    for idx, reason in res["listed"]:
        assert first <= idx < first + count and reason
        r[idx - first] = reason
    if res["bad"]:
        assert (res["first_bad"], res["first_reason"]) == res["listed"][0]
    return r


def _oracle_entry(orc, w, d):
    pt = orc.pubkey_create(((d << (BITS * w)) % N).to_bytes(32, "big"))
    return int.from_bytes(pt[1:33], "big"), int.from_bytes(pt[33:], "big")


# ------------------------------------------------------------------------------------------------ the G table

def test_whole_g_table_audits_clean(eng):
    """all 11 * 2^24 entries of the table this process's engines verify with"""
    assert eng.GTABLE_ENTRIES == ENTRIES and eng.info()["gtable_bytes"] == ENTRIES * 64
    res = eng.gtable_audit(0, ENTRIES)
    assert res["bad"] == 0, res


def test_audit_is_faster_than_the_build_and_clean_after_a_rebuild():
    """Per entry the audit is about a dozen field multiplications and three 64-byte reads, the build 24 doublings, 24 additions and an inversion: the
    audit of the whole table must take less time than the creation of the engine that built it, in the same process.  That process is a fresh one
    (tests/gtable_child.py): in this one an engine of an earlier module may keep the table alive, and Engine(0) then builds nothing.  There, with
    every engine closed the table is freed (tests/test_gpu_parity.py test_engines_of_one_process_share_the_g_table) and the next engine builds it again:
    one full window and the slices at the window boundaries of the rebuilt table audit clean."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gtable_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    times = "engine creation %.3f s, full G-table audit %.3f s, creation after closing every engine %.3f s (11 GiB allocated by the two creations: %s, %s)" % (
        out["t_create"], out["t_audit"], out["t_create_again"], out["table_allocated_by_create"], out["table_allocated_again"])
    print(times)
    assert out["full"]["bad"] == 0, out["full"]
    assert out["t_audit"] < out["t_create"], times
    assert out["window7"]["bad"] == 0 and all(s["bad"] == 0 for s in out["slices"]) and len(out["slices"]) == NWIN + 1, out


def test_g_table_slices_at_the_edges(eng):
    from lightning_amd.engine import LamdError
    for count in (1, 2, 3, 255, 256, 257):
        assert eng.gtable_audit(0, count)["bad"] == 0, count
    for w in range(1, NWIN):
        assert eng.gtable_audit((w << BITS) - 3, 7)["bad"] == 0, w          # 2^24 w - 3 .. 2^24 w + 3
    assert eng.gtable_audit(ENTRIES - 3, 3)["bad"] == 0
    for first in (0, 12345, ENTRIES):
        assert eng.gtable_audit(first, 0) == dict(bad=0, first_bad=None, first_reason=0, listed=[])
    for first, count in ((ENTRIES - 3, 4), (ENTRIES, 1), (ENTRIES + 1, 0), (0, ENTRIES + 1), (1 << 63, 1 << 63)):
        with pytest.raises(LamdError, match="bad argument"):
            eng.gtable_audit(first, count)
    with pytest.raises(LamdError, match="bad argument"):                    # the read-back is bounded in the same way
        eng.debug_read(eng.READ_GTABLE, ENTRIES * 64 - 32, 64)
    assert not eng.debug_read(eng.READ_GTABLE, 3 << (BITS + 6), 64).any()   # digit 0 of window 3


SLICE_FIRST, SLICE_COUNT = (3 << BITS) + (1 << 23) - 2048, 4096


@pytest.fixture(scope="module")
def slice3(engines):
    img = _read_entries(engines.eng(), SLICE_FIRST, SLICE_COUNT)
    img.setflags(write=False)
    return img


def test_negative_control_uncorrupted_copy_is_clean(eng, slice3):
    assert eng.gtable_audit(SLICE_FIRST, SLICE_COUNT, _upload(slice3))["bad"] == 0


@pytest.mark.parametrize("cls", gc.GENERIC, ids=lambda f: f.__name__)
def test_negative_control_on_the_device(eng, slice3, cls):
    """4 096 entries of window 3 (digits 2^23 - 2048 ..) read back, corrupted on the host as in the CPU tests, uploaded as a replacement image: the
    first, a middle, the last and the two positions at a wave's edge; the bad set is exactly what the relations predict"""
    src = lambda idx: _read_entries(eng, idx, 1)[0]
    for k in (0, 63, 64, 2048, SLICE_COUNT - 1):
        img = slice3.copy()
        i = SLICE_FIRST + k
        corrupted, must, must_not = cls(img, SLICE_FIRST, i, src)
        res = eng.gtable_audit(SLICE_FIRST, SLICE_COUNT, _upload(img))
        gc.check(_reasons(res, SLICE_FIRST, SLICE_COUNT), SLICE_FIRST, SLICE_COUNT, corrupted, BITS, NWIN, i, must, must_not, cls.__name__)


def test_negative_control_base_and_digit0_entries(eng):
    """a wrong entry 1 fails through the rest of its window (here: of the slice); entry 1 of window 0 := 2G is caught by the anchor alone; a
    non-zero digit-0 entry is reported by itself"""
    for w in (0, 3):
        first, count = w << BITS, 4096
        true = _read_entries(eng, first, count)
        img = true.copy()
        if w == 0:
            img[1] = gc.entry(*pyref.pmul(2, pyref.G))
        else:
            img[1] = true[5]                                              # another point of the table
        res = eng.gtable_audit(first, count, _upload(img))
        assert res["bad"] == count - 1 and res["first_bad"] == first + 1 and len(res["listed"]) == 64
        assert res["first_reason"] == (gc.ANCHOR if w == 0 else res["first_reason"] & (gc.X | gc.Y))
        assert all(first < idx < first + count and r for idx, r in res["listed"])
        img = true.copy()
        corrupted, must, must_not = gc.nonzero_digit0(img, first, first, None)
        res = eng.gtable_audit(first, count, _upload(img))
        gc.check(_reasons(res, first, count), first, count, corrupted, BITS, NWIN, first, must, must_not, "nonzero_digit0")
        # entry 1 of the next window reads this window's entry 1 as B' -- from the engine's own table
        assert eng.gtable_audit(((w + 1) << BITS) | 1, 1)["bad"] == 0


def test_replacement_image_is_confined_to_its_range(eng):
    """the LAST entry of window 5 corrupted in a replacement slice that ends there: the slice's audit flags it; entry 1 of window 6, whose rule reads
    that entry, audited on its own reads the engine's table and is clean"""
    count = 256
    first = (6 << BITS) - count
    img = _read_entries(eng, first, count)
    i = first + count - 1
    corrupted, must, must_not = gc.flip_y_bit(img, first, i, None)
    res = eng.gtable_audit(first, count, _upload(img))
    assert res["bad"] == 1 and res["listed"] == [(i, res["first_reason"])] and res["first_reason"] & gc.OFF_CURVE
    assert eng.gtable_audit((6 << BITS) | 1, 1)["bad"] == 0
    # ... while a range that holds both sees the damage behind entry 1 of window 6
    img = _read_entries(eng, first, count + 2)
    gc.flip_y_bit(img, first, i, None)
    res = eng.gtable_audit(first, count + 2, _upload(img))
    assert [idx for idx, _ in res["listed"]] == [i, (6 << BITS) | 1]


def _sample_digits(w):
    rnd = random.Random(0x6A7 + w)
    edge = [1, 2, 3, LAST - 1, LAST, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 0x555555, 0xAAAAAA] + [1 << k for k in range(BITS)]
    return edge, [rnd.randrange(1, 1 << BITS) for _ in range(1000)]


@pytest.mark.parametrize("w", range(NWIN))
def test_g_table_sample_against_the_oracle_and_pyref(eng, orc, w):
    """the one check that does not trust the device's field arithmetic: entries read back and compared with d * 2^(24 w) * G from the C oracle
    (edge digits, every power of two, 1 000 seeded random digits) and, for 20 of them, from pyref; entry 0 is zero"""
    edge, rand = _sample_digits(w)
    assert not _read_entries(eng, w << BITS, 1).any()
    for d in edge + rand:
        assert gc.xy(_read_entries(eng, (w << BITS) | d, 1)[0]) == _oracle_entry(orc, w, d), (w, d)
    for d in edge[:10] + rand[:10]:
        assert gc.xy(_read_entries(eng, (w << BITS) | d, 1)[0]) == pyref.pmul((d << (BITS * w)) % N, pyref.G), (w, d)


# ------------------------------------------------------------------------------------------------ key tables, every entry

def _secrets(K):
    rnd = random.Random(4242 + K)
    return ([1, 2, N - 1, LAM % N] + [rnd.randrange(1, N) for _ in range(K)])[:K]


def _off_curve_key():
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    return b"\x02" + x.to_bytes(32, "big")


def _ser(pt65, publen):
    return pt65 if publen == 65 else bytes([2 + (pt65[64] & 1)]) + pt65[1:33]


def _key_words(key):
    kw = np.frombuffer(key.ljust(68, b"\0"), dtype="<u4").copy()
    kw[16] |= len(key) << 8
    return kw


def _batch(orc, keys, secrets, seed):
    """every key signs two valid rows (a key without a secret: two rows that cannot verify); the second rows follow all the first ones"""
    rnd = random.Random(seed)
    hs, sg, pk = [], [], []
    for _ in range(2):
        for key, d in zip(keys, secrets):
            h = bytes(rnd.randrange(256) for _ in range(32))
            hs.append(h)
            sg.append(orc.ecdsa_sign(h, (d or 7).to_bytes(32, "big"), bytes(rnd.randrange(256) for _ in range(32))))
            pk.append(key)
    w = len(keys[0])
    return (np.frombuffer(b"".join(hs), dtype=np.uint8).reshape(-1, 32), np.frombuffer(b"".join(sg), dtype=np.uint8).reshape(-1, 64),
            np.frombuffer(b"".join(pk), dtype=np.uint8).reshape(-1, w))


def _check_table(orc, T, tab, d):
    """every entry m = 0 .. NE of one key's table and its Z block: canonical words, beta * x in the middle, and x / Zc^2, y / Zc^3 = k_m * d * G"""
    D = {7: 19, 10: 13}[T]
    ne = 1 << (T - 1)
    assert len(tab) == ((ne + 1) * 24 + 16) * 4
    zc = int.from_bytes(tab[(ne + 1) * 96:(ne + 1) * 96 + 32], "little")
    assert 0 < zc < P
    zi = pow(zc, P - 2, P)
    zi2, zi3 = zi * zi % P, zi * zi * zi % P
    for m in range(ne + 1):
        x, bx, y = (int.from_bytes(tab[96 * m + 32 * c:96 * m + 32 * c + 32], "little") for c in range(3))
        assert x < P and bx < P and y < P, m
        assert bx == BETA * x % P, m
        k = 1 if m == ne else (1 << ((T - 1) * D)) + sum((1 if (m >> i) & 1 else -1) << (i * D) for i in range(T - 1))
        pt = orc.pubkey_create((k * d % N).to_bytes(32, "big"))
        assert (x * zi2 % P, y * zi3 % P) == (int.from_bytes(pt[1:33], "big"), int.from_bytes(pt[33:], "big")), (hex(d), m)
    return ne + 1


@pytest.mark.parametrize("K", [1, 3, 4, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("tree", [0, 1], ids=["chains", "tree"])
@pytest.mark.parametrize("T", [7, 10])
def test_every_entry_of_every_key_table(engines, orc, T, tree, K):
    """K keys with known secrets (1, 2, n - 1, lambda, random ones) as 33-byte encodings plus one key that is not on the curve, then the first five of
    them again as 65-byte encodings (other cache entries, other tables): the oracle's verdicts come back, every key is in the cache with a table of
    the forced shape, and EVERY entry of every table is the multiple of the key it stands for.  K crosses the builders' key -> thread edges (4 or 32
    chain threads per key, up to 4 keys per tree lane, waves of 64)."""
    import torch
    e = engines.eng_keyed(T, tree)
    assert e.info()["cache_enabled"]
    e.cache_clear()
    secrets = _secrets(K)
    pts = [orc.pubkey_create(d.to_bytes(32, "big")) for d in secrets]
    calls = [([_ser(p, 33) for p in pts] + [_off_curve_key()], secrets + [None]), ([_ser(p, 65) for p in pts[:5]], secrets[:5])]
    for keys, ds in calls:
        hs, sg, pk = _batch(orc, keys, ds, 77 * K + len(keys[0]))
        # device columns: a host-buffer call of <= 64 rows takes the one-launch latency path, which builds no table
        d_h, d_s, d_p = (torch.from_numpy(a.copy()).cuda() for a in (hs, sg, pk))
        d_ok = torch.zeros(len(hs), dtype=torch.uint8, device="cuda")
        e.verify_ecdsa_device(d_h, d_s, d_p, d_ok)
        e.synchronize()
        got = strict_bool(d_ok.cpu().numpy())
        exp = orc.ecdsa_verify_batch(hs, sg, pk, pk.shape[1], 4).astype(bool)
        assert np.array_equal(got, exp)
        assert list(exp) == [d is not None for d in ds] * 2                 # valid rows under every real key, none under the other
        assert e.info()["last_keyed"] == T
    n_ent = K + 1 + min(K, 5)                   # entry ids are handed out from 0 after cache_clear(): one per distinct encoding, no more
    ents = e.debug_read(e.READ_CACHE_ENTS, 0, n_ent * 80).view(np.uint32).reshape(n_ent, 20)
    by_key = {ents[j, :17].tobytes(): ents[j] for j in range(n_ent)}
    assert len(by_key) == n_ent
    which, stride = (e.READ_POOL7, (65 * 24 + 16) * 4) if T == 7 else (e.READ_POOL10, (513 * 24 + 16) * 4)
    slots, compared = set(), 0
    for keys, ds in calls:
        for key, d in zip(keys, ds):
            ent = by_key[_key_words(key).tobytes()]
            meta, seq, slot = int(ent[17]), int(ent[18]), int(ent[19])
            assert seq != 0
            if d is None:
                assert meta & 0xFF == 0          # the key that does not parse is entered as such: an entry without a table, its rows rejected
                continue
            assert meta & 0xFF == T and slot not in slots
            slots.add(slot)
            compared += _check_table(orc, T, e.debug_read(which, slot * stride, stride).tobytes(), d)
    assert compared == (K + min(K, 5)) * ((1 << (T - 1)) + 1)

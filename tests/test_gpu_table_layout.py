"""The two key-table kernels of the fused front end (k_keys_bases_both, k_kc_finish_both): resident grids -- a fixed number of blocks walks groups of
64 keys / 256 (key, chain) threads up to the extents in the call's plan --, their intermediate words interleaved over the wave / the block and reused
by every group a block walks (verify_core.h kc_lanes), every table entry written once, the cache entry written without a local copy.

Engines with the key-table cache off (every call builds its tables) and one lane, so that the tables of the last call can be read back: ECDSA-65 and
BIP-340 calls over 1 .. 1 000 distinct keys with 6 rows each (7-tooth combs), three keys with 48 rows (10-tooth combs), a key that does not parse in
the middle of a wave of good ones.  Every entry of every table is checked as tests/test_gpu_tables.py checks it (x / Zc^2, y / Zc^3 against the C
oracle's multiple of the key); the verdicts are the ones known by construction.  A table is a function of its key alone, so a key audited once is the
reference for every later build of it: the calls with LAMD_TABLE_GRID = 1 and 2 -- every block loops and ends on a partial group -- must reproduce
the audited tables bit for bit.  Needs an MI355X: -m gpu."""
import os
import random

import numpy as np
import pytest
import torch

import chosen_scalars as cs
import pyref
from test_gpu_tables import _check_table, _key_words
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu

P, N = pyref.P, pyref.N
KMAX, ROWS7, ROWS10 = 1000, 6, 48
STRIDE = {7: (65 * 24 + 16) * 4, 10: (513 * 24 + 16) * 4}


def _rows(rows, w):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), w)


@pytest.fixture(scope="module")
def engines():
    """engines by LAMD_TABLE_GRID (None: the default grid), made on demand: cache off, one lane, no minimum batch size for the table path"""
    from lightning_amd import Engine
    made = {}

    def get(grid=None):
        if grid not in made:
            env = {"LAMD_CACHE": "0", "LAMD_LANES": "1", "LAMD_KEYED_MIN_ROWS": "1"}
            if grid is not None:
                env["LAMD_TABLE_GRID"] = str(grid)
            os.environ.update(env)
            try:
                made[grid] = Engine(0)
            finally:
                for k in env:
                    del os.environ[k]
            assert not made[grid].info()["cache_enabled"]
        return made[grid]
    yield get
    for e in made.values():
        e.close()


class _Material:
    """KMAX secrets whose public keys have an even y -- the 65-byte key and the x-only key then stand for the SAME point, hence the same table -- and, per
    key, 48 signed rows of each kind made on demand (about one row in ten with a damaged hash: it must be rejected)"""

    def __init__(self, orc):
        self.orc = orc
        rnd = random.Random(0x7AB1E)
        self.secrets, self.pub65 = [], []
        for d in [1, 2, N - 1] + [rnd.randrange(1, N) for _ in range(2 * KMAX + 64)]:
            pt = orc.pubkey_create(d.to_bytes(32, "big"))
            if pt[64] & 1 == 0 and len(self.secrets) < KMAX:
                self.secrets.append(d)
                self.pub65.append(pt)
        assert len(self.secrets) == KMAX
        self.rows = {}
        self.audited = {}     # (T, secret) -> the table's bytes, every entry checked against the oracle

    def row(self, mode, i, j):
        """row j of key i: (hash / message, signature, expected verdict)"""
        if (mode, i, j) not in self.rows:
            rnd = random.Random((i * 64 + j) * 2 + (mode == "ecdsa"))
            d, h = self.secrets[i].to_bytes(32, "big"), rnd.randbytes(32)
            sig = self.orc.ecdsa_sign(h, d, rnd.randrange(1, N).to_bytes(32, "big")) if mode == "ecdsa" else self.orc.schnorr_sign(h, d, rnd.randbytes(32))
            bad = rnd.randrange(10) == 0
            self.rows[(mode, i, j)] = (bytes([h[0] ^ 0x10]) + h[1:] if bad else h, sig, not bad)
        return self.rows[(mode, i, j)]

    def key(self, mode, i):
        return self.pub65[i] if mode == "ecdsa" else self.pub65[i][1:33]


@pytest.fixture(scope="module")
def material(orc):
    return _Material(orc)


def _bad_key(mode):
    """a key that does not parse: (x, y) off the curve / an x without a point"""
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    return b"\x04" + x.to_bytes(32, "big") + (1).to_bytes(32, "big") if mode == "ecdsa" else x.to_bytes(32, "big")


def _call(e, mat, mode, plan):
    """plan: [(key index or None for the key that does not parse, rows)] -- the rows of the keys interleaved (row j of every key, then row j + 1),
    one call on device buffers; -> (verdicts, expected verdicts)"""
    hs, sg, pk, exp = [], [], [], []
    for j in range(max(r for _, r in plan)):
        for i, r in plan:
            if j >= r:
                continue
            h, s, ok = mat.row(mode, 0 if i is None else i, j)
            hs.append(h); sg.append(s); exp.append(ok and i is not None)
            pk.append(_bad_key(mode) if i is None else mat.key(mode, i))
    cols = (_rows(hs, 32), _rows(sg, 64), _rows(pk, len(pk[0])))
    if mode == "schnorr":
        cols = (cols[0], cols[2], cols[1])
    dev = [torch.from_numpy(np.array(c)).cuda() for c in cols]
    d_ok = torch.zeros(len(hs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    (e.verify_ecdsa_device if mode == "ecdsa" else e.verify_schnorr_device)(dev[0], dev[1], dev[2], d_ok)
    e.synchronize()
    return strict_bool(d_ok.cpu().numpy()), np.array(exp, dtype=bool)


def _check_tables(e, mat, mode, plan):
    """every key of the call has a cache entry; every entry of its table is right (audited against the oracle the first time the key's table of that
    shape is seen, compared bit for bit with the audited table afterwards); no two keys share a slot.  -> tables checked"""
    tabled = [(i, r) for i, r in plan if r >= ROWS7]
    ents = e.debug_read(e.READ_CACHE_ENTS, 0, len(tabled) * 80).view(np.uint32).reshape(len(tabled), 20)
    by_key = {ents[j, :17].tobytes(): ents[j] for j in range(len(tabled))}
    assert len(by_key) == len(tabled)
    # (slots are handed out from 0 in every call of an engine without a cache, one per new key of the shape, the key that does not parse included)
    count = {T: sum(1 for i, r in tabled if (r >= ROWS10) == (T == 10)) for T in (7, 10)}
    pools = {T: e.debug_read(which, 0, STRIDE[T] * count[T]) for T, which in ((7, e.READ_POOL7), (10, e.READ_POOL10)) if count[T]}
    slots, checked = set(), 0
    for i, r in tabled:
        ent = by_key[_key_words(_bad_key(mode) if i is None else mat.key(mode, i)).tobytes()]
        meta, seq, slot = int(ent[17]), int(ent[18]), int(ent[19])
        assert seq != 0
        if i is None:
            assert meta & 0xFF == 0
            continue
        T = 10 if r >= ROWS10 else 7
        assert meta & 0xFF == T and (T, slot) not in slots
        slots.add((T, slot))
        tab = pools[T][slot * STRIDE[T]:(slot + 1) * STRIDE[T]].tobytes()
        d = mat.secrets[i]
        if (T, d) not in mat.audited:
            _check_table(mat.orc, T, tab, d)
            mat.audited[(T, d)] = tab
        used = STRIDE[T] - 32                       # entries and Zc; the 8 words behind Zc are padding that nothing writes
        assert tab[:used] == mat.audited[(T, d)][:used], (mode, i, T)
        checked += 1
    return checked


def _run(e, mat, mode, plan):
    got, exp = _call(e, mat, mode, plan)
    assert 0 < exp.sum() < len(exp) or len(exp) < 20
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    good = sum(1 for i, r in plan if i is not None and r >= ROWS7)
    inf = e.info()
    new_keys = sum(1 for i, r in plan if r >= ROWS7)          # (the key that does not parse is counted: it is entered as such)
    assert inf["last_new_tables"] == new_keys and inf["last_hot_rows"] == sum(r for i, r in plan if i is not None and r >= ROWS7), inf
    assert _check_tables(e, mat, mode, plan) == good


@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, KMAX])
@pytest.mark.parametrize("mode", ["ecdsa", "schnorr"])
def test_seven_tooth_tables_of_k_keys(engines, material, mode, K):
    """K keys x 6 rows: a partial wave of keys, the wave and block edges of both kernels (64 keys per bases group, 64 keys x 4 chains per finish group),
    more groups than one"""
    _run(engines(), material, mode, [(i, ROWS7) for i in range(K)])


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("K", [257, KMAX])
@pytest.mark.parametrize("mode", ["ecdsa", "schnorr"])
def test_every_loop_runs_more_than_once(engines, material, mode, K, grid):
    """1 and 2 blocks: 257 keys are 5 bases groups (the last with one key) and 5 finish groups (the last with four threads), 1 000 keys 16 and 16
    (40 keys, 160 threads in the last) -- every wave and every block iterates and ends on a partial group"""
    _run(engines(grid), material, mode, [(i, ROWS7) for i in range(K)])


@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("mode", ["ecdsa", "schnorr"])
def test_both_shapes_in_one_call(engines, material, mode, grid):
    """three keys with 48 rows (10-tooth tables: 32 chains per key, 96 threads of one finish group) among 70 keys with 6 rows and two met once: the
    7-tooth groups come first, then the 10-tooth group, in both kernels"""
    plan = [(i, ROWS7) for i in range(30)] + [(900, ROWS10)] + [(i, ROWS7) for i in range(30, 70)] + [(901, ROWS10), (902, ROWS10), (950, 1), (951, 1)]
    _run(engines(grid), material, mode, plan)


@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("mode", ["ecdsa", "schnorr"])
def test_a_key_that_does_not_parse_inside_a_live_wave(engines, material, mode, grid):
    """key 40 of 81 is off the curve / has no point: its lane of the bases wave and its four lanes of the finish block do nothing while their
    neighbours work; it is entered as a key without a table and its rows are rejected"""
    plan = [(i, ROWS7) for i in range(40)] + [(None, ROWS7)] + [(i, ROWS7) for i in range(40, 80)]
    _run(engines(grid), material, mode, plan)


@pytest.mark.parametrize("grid", [None, 1])
def test_suspect_rows_take_the_careful_pass(engines, orc, grid):
    """accepting rows at chosen u1, u2 (chosen_scalars.py), their near-miss twins and rows whose sum is infinity, under two keys: the bare formulas
    report the infinity rows as suspects and the careful launch -- a small fixed grid that walks the row lists -- decides them"""
    keys = (0x1F2E3D4C5B6A79881726354453627180AABBCCDDEEFF00112233445566778899, 0x6C1F00D5A3E2B4C7918D7E6F5A4B3C2D1E0F99887766554433221100FFEEDDCC)
    rng = random.Random(78)
    u2s = cs.U2_COMB + [rng.randrange(1, N) for _ in range(12)]
    acc, _ = cs.verify_rows_fixed_keys(orc, rng, [("u2:%d" % j, None, u2) for j, u2 in enumerate(u2s)], list(keys))
    assert len(acc) == len(u2s) and all(r.exact() for r in acc)
    rows = cs.with_twins(acc, 24)
    pub = orc.pubkey_create(keys[1].to_bytes(32, "big"))
    for u2 in u2s:                                           # s = 1, r = u2, hash = u1 = -u2*d: the sum is infinity
        rows.append(cs.Row("verify", ((-u2 * keys[1]) % N).to_bytes(32, "big"), u2.to_bytes(32, "big") + (1).to_bytes(32, "big"), pub, (None, u2), "inf", expect=False))
    cols = cs.columns(rows, 65)
    exp = np.array([r.expect for r in rows], dtype=bool)
    assert np.array_equal(orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], 65, 2).astype(bool), exp) and exp.sum() == len(acc)
    e = engines(grid)
    dev = [torch.from_numpy(np.array(c)).cuda() for c in cols]
    d_ok = torch.zeros(len(rows), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.verify_ecdsa_device(dev[0], dev[1], dev[2], d_ok)
    e.synchronize()
    got = strict_bool(d_ok.cpu().numpy())
    assert np.array_equal(got, exp), [(rows[i].tag, hex(rows[i].u1), hex(rows[i].u2)) for i in np.nonzero(got != exp)[0][:10]]
    inf = e.info()
    assert inf["last_keyed"] in (7, 10) and inf["last_hot_rows"] == len(rows) and inf["last_suspect_rows"] >= len(u2s), inf

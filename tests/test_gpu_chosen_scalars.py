"""Accepting rows at chosen u1, u2 on every device ecmult path.  chosen_scalars.py builds ECDSA rows that verify iff the device computes exactly
R = u1*G + u2*Q for a u1 aimed at the 24-bit G table walk (one window non-zero, one window zero, one task wave's windows only, a pair of the
pairs-first kernel with an entry missing, the ends of the range) and a u2 aimed at the GLV split and the recodings (+-lambda^i, tiny / even / zero
halves, halves that cancel), each with a near-miss twin -- the same (r, s), one window digit of u1 off by one -- that must reject; recovery rows
return the point itself.  Expected verdicts and keys are the C oracle's, which must agree with the construction; test_chosen_scalars_host.py is the
CPU side (OpenSSL, pyref, the host build of the device code) that tells a device fault from a wrong generator.

The path a call took is asserted from Engine.info() wherever info() exposes it.  It does not expose:
  - which kernel ran a recovery call (there is one: the ladder kernel in MODE_RECOVER, rows sharing an r included -- recovery builds no tables);
  - the ladder of a LAMD_KEYED=0 engine (info() reports a call without lists: only the absence of tables is asserted);
  - that LAMD_PAIRS=1 took effect (the lists and counters are those of the plain comb kernel), and how many rows a lane's batch held;
  - which comb body (one shape, or the run-time shape of a wave holding 7- and 10-tooth keys) a wave of the one-launch path ran.
Needs an MI355X: -m gpu."""
import os

import numpy as np
import pytest
import torch

import chosen_scalars as cs
import pyref
from verdict_bytes import strict_bool

pytestmark = pytest.mark.gpu
BITS = 24                            # verify_core.h GTABLE_WINDOW_BITS as shipped


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


def _on_device(e, cols):
    """the device-buffer entry: the general path whatever the batch size"""
    dev = [torch.from_numpy(np.array(c)).cuda() for c in cols]
    d_ok = torch.zeros(len(cols[0]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.verify_ecdsa_device(dev[0], dev[1], dev[2], d_ok)
    e.synchronize()
    return strict_bool(d_ok.cpu().numpy())


def _cols_exp(orc, rows, publen):
    """the rows' columns and the C oracle's verdicts, which are the construction's: every row accepts, every twin rejects"""
    cols = cs.columns(rows, publen)
    exp = orc.ecdsa_verify_batch(cols[0], cols[1], cols[2], publen, 4).astype(bool)
    assert np.array_equal(exp, np.array([r.expect for r in rows], dtype=bool)) and 0 < exp.sum() < len(rows)
    return cols, exp


def _same(got, exp, rows, what):
    bad = np.nonzero(np.asarray(got) != exp)[0]
    assert not len(bad), (what, len(bad), [(rows[i].tag, hex(rows[i].u1), hex(rows[i].u2)) for i in bad[:6]])


@pytest.fixture(scope="module")
def sets(orc):
    s = cs.row_sets(orc, BITS)
    names = {n for n, _ in cs.u1_patterns(BITS)}
    for path in ("own", "fixed", "recover", "recover_shared"):
        assert cs.reached_patterns(s[path], BITS) == names and len(s[path]) > 800
    return s


@pytest.mark.parametrize("env", [{}, {"LAMD_KEYED": "0"}], ids=["default", "keyed0"])
def test_ladder_kernel_rows_under_keys_of_their_own(orc, sets, env):
    """the general path's per-signature ladder (ecmult_lane_fast: signed odd digits, the top digit the accumulator, the branching G walk): every row
    its own key through the device-buffer entry, on a default engine (a key is met twice at most: no table) and on one that never builds tables.
    The twins follow the rows as a block: a twin next to its row would be a run of rows under one unknown key, which a default engine answers by
    building tables in its next small call."""
    rows = sets["own"][0::2] + sets["own"][1::2]
    e = _engine(env)
    try:
        for publen in (33, 65):
            cols, exp = _cols_exp(orc, rows, publen)
            _same(_on_device(e, cols), exp, rows, (env, publen))
            inf = e.info()
            assert inf["last_keyed"] == 0 and inf["last_hot_rows"] == 0 and inf["last_new_tables"] == 0, inf
            if not env:
                assert inf["last_cold_rows"] == len(rows) and inf["last_cache_hits"] == 0, inf
    finally:
        e.close()


@pytest.fixture(scope="module", params=[7, 10])
def eng_keyed(request):
    """engine forced onto per-key comb tables of one shape whenever a key has two rows"""
    e = _engine({"LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(request.param)})
    e.teeth = request.param
    yield e
    e.close()


def test_comb_kernel_rows_under_the_key_pool(eng_keyed, orc, sets):
    """k_ecmult_keyed<false>, 7 and 10 teeth: every u1 window pattern x a random u2, a random u1 x every u2, and the cross-product sample, all under
    8 keys -- every row on a comb list"""
    e = eng_keyed
    rows = sets["fixed"]
    assert not sets["unreachable"] or 64 * len(sets["unreachable"]) <= len(rows) // 2
    for publen in (65, 33):
        cols, exp = _cols_exp(orc, rows, publen)
        e.cache_clear()
        _same(_on_device(e, cols), exp, rows, (e.teeth, publen))
        inf = e.info()
        assert inf["last_keyed"] == e.teeth and inf["last_hot_rows"] == len(rows) and inf["last_new_tables"] == cs.KEY_POOL_SIZE, inf
        _same(e.verify_ecdsa(*cols), exp, rows, (e.teeth, publen, "host buffers"))      # > 64 rows from host memory: the same path
        assert e.info()["last_keyed"] == e.teeth and e.info()["last_hot_rows"] == len(rows)


@pytest.mark.parametrize("teeth", [7, 10])
def test_pairs_first_kernel_rows_under_the_key_pool(orc, sets, teeth):
    """k_ecmult_keyed_pairs (LAMD_PAIRS=1): the same rows once (every lane one row: batches of one) and tiled until every lane of the persistent
    grid owns two or three rows, so that rows whose G pairs are not formed (a zero digit) share an inversion with rows whose pairs are"""
    rows = sets["fixed"]
    cols, exp = _cols_exp(orc, rows, 65)
    e = _engine({"LAMD_PAIRS": "1", "LAMD_KEYED": "1", "LAMD_KEYED_TEETH": str(teeth), "LAMD_CACHE": "0"})
    try:
        _same(_on_device(e, cols), exp, rows, (teeth, "once"))
        inf = e.info()
        assert inf["last_keyed"] == teeth and inf["last_hot_rows"] == len(rows), inf
        lanes = inf["compute_units"] * 3 * 4 * 64                               # the persistent grid (ecmult_stage)
        reps = (2 * lanes + lanes // 2) // len(rows) + 1
        tiled = [np.ascontiguousarray(np.tile(c, (reps, 1))) for c in cols]
        got = e.verify_ecdsa(*tiled)
        inf = e.info()
        assert inf["last_keyed"] == teeth and inf["last_hot_rows"] == reps * len(rows) > 2 * lanes, inf
        _same(got, np.tile(exp, reps), rows * reps, (teeth, "tiled", reps))
    finally:
        e.close()


def _chunks(rows, size):
    return [rows[o:o + size] for o in range(0, len(rows), size)]


def test_one_launch_path_never_seen_keys(orc, sets):
    """k_small_verify, keys without a table: the two ladder halves on two task waves, u1*G spread over four (three windows each, the last wave two:
    the single-group patterns leave three of them at infinity), the three-level merge.  The u1 patterns in calls of 64 rows or fewer (a row and its
    twin, which share the key, in the same call; no key comes back in a later call, which would send it to the table-building path), every other
    row in ONE call of more than 64 rows."""
    from lightning_amd import Engine
    rows = sets["own"]
    first = [i for i in range(0, len(rows), 2) if rows[i].tag.startswith("u1:")]
    small = [rows[j] for i in first for j in (i, i + 1)]
    rest = [rows[j] for i in range(0, len(rows), 2) if i not in set(first) for j in (i, i + 1)]
    assert {r.tag[3:] for r in small[0::2]} == {n for n, _ in cs.u1_patterns(BITS)} and 64 < len(rest) <= 4096
    with Engine(0) as e:
        assert e.info()["cache_enabled"]
        calls = _chunks(small, 64) + [rest]
        assert len(calls[-2]) < 64                                              # (a partial wave among them)
        for k, part in enumerate(calls):
            cols, exp = _cols_exp(orc, part, 33 if k % 2 else 65)
            _same(e.verify_ecdsa(*cols), exp, part, ("call", k, len(part)))
            inf = e.info()
            assert (inf["last_cold_rows"], inf["last_cache_hits"], inf["last_keyed"], inf["last_new_tables"]) == (len(part), 0, 0, 0), (k, inf)


def test_one_launch_path_cached_keys(orc, sets):
    """k_small_verify over cached comb tables: four keys of the pool primed with 10-tooth tables and four with 7-tooth tables through the device
    entry (twice: the host has then seen the publishing call complete), then host-buffer calls of 64 rows or fewer -- one shape alone, and both in
    one wave (the run-time comb body) -- and one call of all rows.  The four comb parts on four task waves, u1*G over the other four."""
    rows = sets["fixed"]
    pool = [cs.ser65(cs.mul_g(orc, d)) for d in cs.key_pool()]
    ten, seven = set(pool[:4]), set(pool[4:])
    count = {k: 0 for k in pool}
    prime = []
    for i in range(0, len(rows), 2):                                            # every row of the first four keys, 10 rows (and twins) of the others
        count[rows[i].key] += 1
        if rows[i].key in ten or count[rows[i].key] <= 10:
            prime += [rows[i], rows[i + 1]]
    assert all(count[k] >= 48 for k in ten) and all(count[k] >= 10 for k in seven)     # the default thresholds: 48 rows per key -> 10 teeth, 6 -> 7 teeth
    e = _engine({"LAMD_KEYED_MIN_ROWS": "1"})                                   # (a batch this small would otherwise be looked up in the cache only)
    try:
        assert e.info()["cache_enabled"]
        cols, exp = _cols_exp(orc, prime, 65)
        _same(_on_device(e, cols), exp, prime, "priming call")
        inf = e.info()
        assert (inf["last_keyed"], inf["last_hot_rows"], inf["last_new_tables"], inf["last_cold_rows"]) == (10, len(prime), 8, 0), inf
        _same(_on_device(e, cols), exp, prime, "second call")
        inf = e.info()
        assert (inf["last_cache_hits"], inf["last_new_tables"]) == (len(prime), 0), inf
        pats = [j for i in range(0, len(rows), 2) if rows[i].tag.startswith("u1:") for j in (i, i + 1)]
        calls = [("10 teeth", [rows[j] for j in pats if rows[j].key in ten][:64], 10), ("7 teeth", [rows[j] for j in pats if rows[j].key in seven][:64], 7)]
        calls += [("patterns %d" % k, [rows[j] for j in part], 10) for k, part in enumerate(_chunks(pats, 64))]
        calls += [("one shape each, whole set", [r for r in rows if r.key in ten], 10), ("all rows", rows, 10)]
        seen = set()
        for what, part, keyed in calls:
            cols, exp = _cols_exp(orc, part, 65)
            _same(e.verify_ecdsa(*cols), exp, part, what)
            inf = e.info()
            assert (inf["last_cache_hits"], inf["last_hot_rows"], inf["last_cold_rows"], inf["last_keyed"], inf["last_new_tables"]) == (len(part), len(part), 0, keyed, 0), (what, inf)
            seen |= {r.tag[3:] for r in part if r.tag.startswith("u1:") and r.expect}
        assert seen == {n for n, _ in cs.u1_patterns(BITS)}
        assert 64 < len(calls[-2][1]) <= 4096 and 64 < len(rows) <= 4096 and all(len(c[1]) <= 64 for c in calls[:-2])
    finally:
        e.close()


@pytest.mark.parametrize("name", ["recover", "recover_shared"])
def test_recovery_returns_the_exact_point(orc, sets, name):
    """lamd_ecdsa_recover_batch: Q = u1*G + u2*R with u1 = -z/r, u2 = s/r at the chosen pairs, rows with distinct r and 64 rows (32 and their twins)
    per r: the 33 bytes against the construction, the C oracle and (structured rows) pyref; every twin returns another key"""
    from lightning_amd import Engine
    rows = sets[name]
    hs, sg, rid = cs.columns(rows)
    ck, cok = orc.ecdsa_recover_batch(hs, sg, rid, 4)
    with Engine(0) as e:
        keys, ok = e.ecdsa_recover(hs, sg, rid)
        assert np.array_equal(ok, cok.astype(bool)) and np.array_equal(keys, ck), [rows[i].tag for i in np.nonzero((keys != ck).any(axis=1) | (ok != cok.astype(bool)))[0][:6]]
        for i, r in enumerate(rows):
            got = keys[i].tobytes() if ok[i] else None
            if i % 2 == 0:
                assert ok[i] and got == r.expect and r.exact(), r.tag
            else:
                assert got != rows[i - 1].expect, r.tag
        for i in [i for i, r in enumerate(rows) if r.tag.startswith("u1:") or r.tag.startswith("x:")][::17]:
            p = pyref.ecdsa_recover(rows[i].hash, rows[i].sig, rows[i].recid)
            assert (pyref.ser33(p) if p else None) == (keys[i].tobytes() if ok[i] else None), rows[i].tag
        small = [j for i in range(0, len(rows), 2) if rows[i].tag.startswith("u1:") for j in (i, i + 1)][:64]     # and a call of one wave
        keys, ok = e.ecdsa_recover(hs[small], sg[small], rid[small])
        assert np.array_equal(ok, cok[small].astype(bool)) and np.array_equal(keys, ck[small])

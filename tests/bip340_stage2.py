"""BIP-340 rows that only the second stage of the device's acceptance test can decide, and a way to plant them along the chains of rows one
thread of that stage owns.

The device splits BIP-340 acceptance (verify_core.h): stage 1, in the ecmult kernel, tests R != infinity and x(R) == r and marks the survivors
PENDING (verdict byte 2); stage 2 (schnorr_final_thread) gives thread t the rows t, t + T, t + 2T, ..., inverts all their pending Z with one
inversion and tests the parity of y(R).  A row that stage 2 must REJECT -- x(R) == r with y(R) odd -- is the only kind that shows a stage 2
that was skipped, ran short or mixed up its chain, and neither the workload generator nor the oracle's edge generator has one.

Classes (d negated first if y(P) is odd, as BIP-340 signing does):
  odd_R   reject   k with y(kG) odd, NOT negated: r = x(kG), e = H(r || x(P) || m), s = k + e*d.  The verifier reaches exactly R = kG.
  even_R  accept   the same (d, m, r) with k negated: the twin of an odd_R row, a correct signature.
  R_inf   reject   any r < p, s = e*d: s*G - e*P is the point at infinity.  r is the x of a curve point, an x with no square root, 0 and 1.
  flip    reject   an even_R row with one bit of s flipped: another R, rejected by stage 1 -- the non-pending neighbour in a chain.

Pure Python over oracle/pyref.py, seeded; one pmul per odd/even pair and one per key.  pool() is cached: tests copy its rows."""
import collections
import functools
import random

import numpy as np

import pyref

P, N, G = pyref.P, pyref.N, pyref.G
CLASSES = ("odd_R", "even_R", "R_inf", "flip")
EXPECT = {"odd_R": False, "even_R": True, "R_inf": False, "flip": False}
NKEYS = 8
Row = collections.namedtuple("Row", "cls msg pk sig expect key twin tag")       # twin: the pool index of the odd_R / even_R partner (or None)


def _challenge(r32, px32, msg32):
    return int.from_bytes(pyref.tagged_hash("BIP0340/challenge", r32 + px32 + msg32), "big") % N


def _b(v):
    return v.to_bytes(32, "big")


@functools.lru_cache(maxsize=None)
def pool(seed=340, pairs=80, infs=40, flips=40):
    """-> tuple of Row, at most 256: `pairs` odd_R rows each followed by its even_R twin, then R_inf and flip rows, over NKEYS keys"""
    assert 2 * pairs + infs + flips <= 256 and infs >= 8
    rnd = random.Random(seed)
    keys = []
    for _ in range(NKEYS):
        d = rnd.randrange(1, N)
        Q = pyref.pmul(d, G)
        keys.append((N - d if Q[1] & 1 else d, _b(Q[0])))
    rows, rxs = [], []
    for i in range(pairs):
        kid = i % NKEYS
        d, px = keys[kid]
        msg = rnd.randbytes(32)
        k = rnd.randrange(1, N)
        R = pyref.pmul(k, G)
        k_odd = k if R[1] & 1 else N - k                    # y((N - k) G) = p - y(kG): exactly one of the two is odd
        r32 = _b(R[0])
        e = _challenge(r32, px, msg)
        rxs.append(R[0])
        rows.append(Row("odd_R", msg, px, r32 + _b((k_odd + e * d) % N), False, kid, len(rows) + 1, "pair%d" % i))
        rows.append(Row("even_R", msg, px, r32 + _b((N - k_odd + e * d) % N), True, kid, len(rows) - 1, "pair%d" % i))
    nosqrt = []
    x = rnd.randrange(2, P)
    while len(nosqrt) < infs:
        if pyref.lift_x(x) is None:
            nosqrt.append(x)
        x += 1
    for i in range(infs):
        kid = i % NKEYS
        d, px = keys[kid]
        msg = rnd.randbytes(32)
        kind = ("curve_x", "no_sqrt", "zero", "one")[i % 4] if i < 16 else ("curve_x", "no_sqrt")[i % 2]
        r = {"curve_x": rxs[i % len(rxs)], "no_sqrt": nosqrt[i], "zero": 0, "one": 1}[kind]
        e = _challenge(_b(r), px, msg)
        s = e * d % N
        assert s
        rows.append(Row("R_inf", msg, px, _b(r) + _b(s), False, kid, None, "r=" + kind))
    evens = [r for r in rows if r.cls == "even_R"]
    for i in range(flips):
        src = evens[rnd.randrange(len(evens))]
        bit = rnd.randrange(256)
        s = int.from_bytes(src.sig[32:], "big") ^ (1 << bit)
        if s >= N:                                          # (would be rejected by the scalar check, before any stage: keep it a stage-1 reject)
            s = int.from_bytes(src.sig[32:], "big") ^ 1
        rows.append(Row("flip", src.msg, src.pk, src.sig[:32] + _b(s), False, src.key, None, "bit%d" % bit))
    assert all(r.expect == EXPECT[r.cls] for r in rows)
    return tuple(rows)


def by_class(rows=None):
    rows = pool() if rows is None else rows
    return {c: [r for r in rows if r.cls == c] for c in CLASSES}


def columns(rows):
    """-> (msg uint8 [n,32], pk uint8 [n,32], sig uint8 [n,64], expect bool [n])"""
    col = lambda k, w: np.frombuffer(b"".join(getattr(r, k) for r in rows), dtype=np.uint8).reshape(len(rows), w).copy()
    return col("msg", 32), col("pk", 32), col("sig", 64), np.array([r.expect for r in rows], dtype=bool)


def tiled(n, seed=1):
    """n pool rows in a seeded order (every pool row before any comes again) -> (rows, columns...)"""
    rnd = random.Random(seed)
    rows = []
    while len(rows) < n:
        part = list(pool())
        rnd.shuffle(part)
        rows += part
    rows = rows[:n]
    return (rows,) + columns(rows)


def final_stride(n, compute_units):
    """the engine's final_threads() restated, and the stride its grid gives schnorr_final_thread: threads in blocks of 256"""
    t = (n + 15) // 16
    m = 256 * compute_units
    t = t if t >= m else min(n, m)
    return (t + 255) // 256 * 256


def patterns(length):
    """the class patterns planted along one chain of `length` rows, in the chain's order; positions a pattern does not name hold even_R rows
    (pending, accepted): every row odd_R; odd_R only first / only in the middle / only last; then the three-row patterns, alternately at the
    chain's start and at its end"""
    O, E, I, F = "odd_R", "even_R", "R_inf", "flip"
    out = [("all_odd", [O] * length)]
    if length >= 2:
        where = sorted({0, length // 2, (length - 1) // 2, length - 1} if length >= 3 else {0, 1})
        for j in where:
            name = "odd_first" if j == 0 else "odd_last" if j == length - 1 else "odd_middle%d" % j
            out.append((name, [O if i == j else E for i in range(length)]))
    if length >= 3:
        triples = [("odd_flip_odd", (O, F, O)), ("flip_odd_flip", (F, O, F)), ("flip_flip_odd", (F, F, O)), ("odd_flip_flip", (O, F, F)),
                   ("even_inf_even", (E, I, E)), ("inf_odd_inf", (I, O, I))]
        for k, (name, tri) in enumerate(triples):
            at = 0 if k % 2 == 0 else length - 3
            out.append((name, [tri[i - at] if at <= i < at + 3 else E for i in range(length)]))
    return out


def plant(cols, expect, stride, lengths, seed=2, block=None, block_rows=16384):
    """overwrites rows of the column (cols = [msg, pk, sig] numpy arrays, expect bool; all changed in place) with pool rows:
      - for every chain length in `lengths`, every pattern of patterns(length) along a chain of its own: rows p, p + stride, p + 2 * stride, ...
        for the lowest free p whose chain has that length;
      - block (a first row) given: block_rows contiguous rows from there, each odd_R or even_R with probability 1/2 from the seed -- whatever
        the row-to-thread mapping is, chains through the block mix both classes.
    -> dict(chains={length: [(p, pattern name), ...]}, classes={row: class}, block=(first, rows) or None)"""
    n = len(expect)
    rnd = random.Random(seed)
    cls = by_class()
    taken = {}

    def put(i, row):
        assert i not in taken and 0 <= i < n
        cols[0][i] = np.frombuffer(row.msg, dtype=np.uint8)
        cols[1][i] = np.frombuffer(row.pk, dtype=np.uint8)
        cols[2][i] = np.frombuffer(row.sig, dtype=np.uint8)
        expect[i] = row.expect
        taken[i] = row.cls
    blk = range(0)
    if block is not None:
        blk = range(block, block + block_rows)
        assert blk.stop <= n
    chains = {}
    used = set()
    for length in lengths:
        chains[length] = []
        for name, pat in patterns(length):
            p = next((p for p in range(min(stride, n)) if p not in used and len(range(p, n, stride)) == length
                      and not any(i in blk for i in range(p, n, stride))), None)
            if p is None:
                continue
            used.add(p)
            pair = cls["odd_R"][rnd.randrange(len(cls["odd_R"]))]           # an odd_R row's even_R neighbours include its own twin
            for j, c in enumerate(pat):
                row = pool()[pair.twin] if c == "even_R" and j % 2 else pair if c == "odd_R" and j == 0 else cls[c][rnd.randrange(len(cls[c]))]
                put(p + j * stride, row)
            chains[length].append((p, name))
    for i in blk:
        put(i, cls["odd_R" if rnd.random() < 0.5 else "even_R"][rnd.randrange(len(cls["odd_R"]))])
    return dict(chains=chains, classes=taken, block=(blk.start, len(blk)) if len(blk) else None)

"""Signature rows whose verdict depends on the exact point R = u1*G + u2*Q at CHOSEN u1, u2 (a plain helper module, shared by
test_chosen_scalars_host.py, test_gpu_chosen_scalars.py and the tests the scalar lists were collected from).

An ECDSA row (z, r, s) under Q verifies iff x(z/s * G + r/s * Q) = r (mod n).  Pick u1, u2, form R = u1*G + u2*Q, set r = x(R) mod n, s = r/u2,
z = u1*s: then z/s = u1, r/s = u2 and the row ACCEPTS iff the verifier computes exactly that point.  The low-S rule costs one degree of freedom
(negating s gives the pair (-u1, -u2)), so every construction keeps redrawing whatever it is free to redraw -- the nonce, the random side of the
pair, the key out of a pool -- until s is low, and reports the pairs it could not reach.  Key recovery returns Q = -z/r * G + s/r * R: with R = k*G,
r = x(R), s = u2*r, z = -u1*r every pair is reachable and the 33 output bytes are the point itself.

Every row carries the EFFECTIVE pair, recomputed from (z, r, s), and a near-miss twin: the same (r, s) with one window digit of u1 off by one,
which must reject (recovery: must return another key).

The u1 list is aimed at the G table walk (windows of `bits` bits: 24 as shipped, 8 in the host harness), the u2 list at the GLV split and the
signed-digit recodings."""
import random

import pyref

N = pyref.N
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
SEED = 20240611                      # the committed seed: test_chosen_scalars_host.py asserts the caps at it
KEY_POOL_SIZE = 8

# ---- u2: the recoding lists (test_gpu_pair_column.py, test_devmath_host.py import them back)
# the comb's list: +-lambda^i (one GLV half exactly +-1), lambda +- 1, tiny / even / zero halves, halves that cancel, n - 1, (n + 1)/2
U2_COMB = [1, 2, 3, 4, N - 1, N - 2, LAM, N - LAM, LAM + 1, LAM - 1, 2 * LAM % N, (LAM + 2) % N, LAM * LAM % N, (N - LAM * LAM) % N,
           1 << 127, (1 << 128) - 1, 1 << 128, (1 << 128) + 1, ((1 << 127) * LAM + 2) % N, (N + 1) // 2]
# the ladder's list: every small u2 (the top digit of the signed odd recoding initialises the accumulator), multiples of lambda that fill a digit
U2_LADDER = list(range(0, 40)) + [N - 1, N - 2, N - 3, LAM, N - LAM, LAM + 1, LAM - 1, 2 * LAM % N, (LAM + 2) % N, 3 * LAM % N, (15 * LAM) % N, (16 * LAM + 1) % N,
                                  LAM * LAM % N, (N - LAM * LAM) % N, 1 << 127, (1 << 128) - 1, 1 << 128, (1 << 128) + 1, ((1 << 127) * LAM + 2) % N, (N + 1) // 2,
                                  (1 << 129) - 1, ((1 << 128) - 1) * LAM % N, (0x88888888888888888888888888888888 * (LAM + 1)) % N]
N_RANDOM_U2 = 12


def u2_list(seed=SEED):
    """the union of the recoding lists (u2 = 0 is r = 0 or s = 0: not a signature) and a dozen seeded random scalars; the random ones come last"""
    out = []
    for v in U2_COMB + U2_LADDER:
        if v and v not in out:
            out.append(v)
    rng = random.Random(seed * 1000 + 2)
    return out + [rng.randrange(1, N) for _ in range(N_RANDOM_U2)]


# ---- u1: the window patterns
def windows(bits):
    return (256 + bits - 1) // bits


def digit(u, bits, w):
    return (u >> (bits * w)) & ((1 << bits) - 1)


def digits(u, bits):
    return [digit(u, bits, w) for w in range(windows(bits))]


def task_groups(bits):
    """the windows k_small_verify's four G waves take for a row with a comb table, and the two halves a ladder row's split uses (small_g_windows)"""
    W = windows(bits)
    q, h = (W + 3) // 4, (W + 1) // 2
    comb = [list(range(t * q, min((t + 1) * q, W))) for t in range(4)]
    return [g for g in comb if g], [list(range(0, h)), list(range(h, W))]


def u1_patterns(bits, seed=SEED):
    """[(name, u1)]: every pattern of zero / non-zero windows at which a G table walk branches, and the scalars at the ends of the range"""
    W = windows(bits)
    rng = random.Random(seed * 1000 + 1)
    full = (1 << bits) - 1
    top_max = (N - 1) >> (bits * (W - 1))          # the last window is narrower (16 bits of 24; 8 of 8) and capped so that u1 < n

    def nz(w):                                     # a non-zero digit for window w that keeps u1 < n whatever the lower windows hold
        return rng.randrange(1, full + 1) if w < W - 1 else rng.randrange(1, top_max)

    def build(nonzero):
        return sum(nz(w) << (bits * w) for w in sorted(nonzero))

    out = []
    for w in range(W):
        cap = full if w < W - 1 else top_max
        topbits = bits if w < W - 1 else top_max.bit_length()
        for kind, d in (("1", 1), ("msb", 1 << (topbits - 1)), ("ones", cap), ("rnd", rng.randrange(2, cap))):
            out.append(("one:%d:%s" % (w, kind), min(d, cap) << (bits * w)))
    for w in range(W):
        out.append(("allbut:%d" % w, build(set(range(W)) - {w})))
    comb, ladder = task_groups(bits)
    for g in comb:
        out.append(("combsplit:%d-%d" % (g[0], g[-1]), build(g)))
    for g in ladder:
        out.append(("laddersplit:%d-%d" % (g[0], g[-1]), build(g)))
    for p in range(W // 2):                        # the pairs-first kernel: pair (2p, 2p + 1) with one or both entries missing
        for kind, zero in (("first0", {2 * p}), ("second0", {2 * p + 1}), ("both0", {2 * p, 2 * p + 1})):
            out.append(("pair:%d:%s" % (p, kind), build(set(range(W)) - zero)))
    if W & 1:                                      # ... and the lone last window
        out.append(("last:zero", build(range(W - 1))))
        out.append(("last:nonzero", build(range(W))))
    out += [("0", 0), ("1", 1), ("n-1", N - 1), ("n-2", N - 2), ("(n+1)/2", (N + 1) // 2), ("2^255", 1 << 255), ("2^240-1", (1 << 240) - 1)]
    assert all(0 <= u < N for _, u in out)
    return out


def check_u1_patterns(bits, pats):
    """the list is what its names say (the tests call this: a generator that drifts must not pass silently)"""
    W = windows(bits)
    byname = dict(pats)
    assert len(byname) == len(pats)
    for name, u in pats:
        nzw = {w for w, d in enumerate(digits(u, bits)) if d}
        f = name.split(":")
        if f[0] == "one":
            assert nzw == {int(f[1])}, name
        elif f[0] == "allbut":
            assert nzw == set(range(W)) - {int(f[1])}, name
        elif f[0] in ("combsplit", "laddersplit"):
            lo, hi = (int(x) for x in f[1].split("-"))
            assert nzw == set(range(lo, hi + 1)), name
        elif f[0] == "pair":
            p = int(f[1])
            assert nzw == set(range(W)) - {"first0": {2 * p}, "second0": {2 * p + 1}, "both0": {2 * p, 2 * p + 1}}[f[2]], name
        elif name == "last:zero":
            assert nzw == set(range(W - 1))
        elif name == "last:nonzero":
            assert nzw == set(range(W))
    comb, ladder = task_groups(bits)
    assert sum(n.startswith("combsplit") for n in byname) == len(comb) and sum(n.startswith("laddersplit") for n in byname) == 2
    assert sum(n.startswith("one:") for n in byname) == 4 * W and sum(n.startswith("pair:") for n in byname) == 3 * (W // 2)


def near_miss_u1(u1, bits, w0):
    """u1 with ONE window digit off by one (no carry into another window), starting the search at window w0 -> (u1', w)"""
    W = windows(bits)
    for off in range(W):
        w = (w0 + off) % W
        step = 1 << (bits * w)
        top = ((1 << 256) - 1) >> (bits * w) if w == W - 1 else (1 << bits) - 1
        d = (u1 >> (bits * w)) & top
        if d < top and u1 + step < N:
            return u1 + step, w
        if d > 0:
            return u1 - step, w
    raise AssertionError("no window of %x can move" % u1)


# ---- rows
def _b(v):
    return v.to_bytes(32, "big")


def _inv(a):
    return pow(a, -1, N)


def mul_g(orc, k):
    """k*G, 1 <= k < n, by the C oracle (pyref.pmul takes milliseconds)"""
    pub = orc.pubkey_create(_b(k))
    return int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")


def ser65(pt):
    return b"\x04" + _b(pt[0]) + _b(pt[1])


def ser33(pt):
    return bytes([2 + (pt[1] & 1)]) + _b(pt[0])


class Row:
    """one verification (hash, sig, pub65) or recovery (hash, sig, recid -> key33) row, the pair it was asked to hit (`want`, None = a random side),
    the pair it does hit (`u1`, `u2`, recomputed from the row's bytes) and its expected outcome by construction (`expect`: verdict / key bytes)"""

    def __init__(self, kind, h, sig, key, want, tag, recid=None, expect=True):
        self.kind, self.hash, self.sig, self.key, self.want, self.tag, self.recid, self.expect = kind, h, sig, key, want, tag, recid, expect
        self.u1, self.u2 = effective(kind, h, sig)

    def exact(self):
        return all(w is None or w == g for w, g in zip(self.want, (self.u1, self.u2)))


def effective(kind, h, sig):
    """(u1, u2) as the verifier derives them: z/s, r/s -- or -z/r, s/r for recovery"""
    z, r, s = int.from_bytes(h, "big") % N, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if kind == "verify":
        si = _inv(s)
        return z * si % N, r * si % N
    ri = _inv(r)
    return (-z) * ri % N, s * ri % N


def _verify_row(orc, u1, u2, d, k, want, tag):
    """the row for nonce point k*G = u1*G + u2*(d*G), or None when it is no low-S signature"""
    if k == 0 or d == 0 or u2 == 0:
        return None
    r = mul_g(orc, k)[0] % N
    if r == 0:
        return None
    s = r * _inv(u2) % N
    if s == 0 or s > N // 2:
        return None
    return Row("verify", _b(u1 * s % N), _b(r) + _b(s), ser65(mul_g(orc, d)), want, tag)


def verify_row_own_key(orc, rng, u1, u2, tag=""):
    """a row under a key of its own that hits (u1, u2) exactly: draw the nonce k until s = x(k*G)/u2 is low; the key's secret is (k - u1)/u2"""
    while True:
        k = rng.randrange(1, N)
        row = _verify_row(orc, u1, u2, (k - u1) * _inv(u2) % N, k, (u1, u2), tag)
        if row is not None:
            return row


def key_pool(seed=SEED, size=KEY_POOL_SIZE):
    rng = random.Random(seed * 1000 + 3)
    return [rng.randrange(1, N) for _ in range(size)]


def verify_rows_fixed_keys(orc, rng, pairs, keys):
    """pairs: [(tag, u1, u2)], None for a random side -> (rows, unreachable).  A random side is redrawn until s is low (the structured side is exact);
    a pair with both sides given is tried under each key of the pool (s is low under about half of them): the pairs no key reaches come back
    in `unreachable`, never dropped silently."""
    rows, unreachable = [], []
    for i, (tag, u1, u2) in enumerate(pairs):
        row = None
        if u1 is None or u2 is None:
            d = keys[i % len(keys)]
            while row is None:
                a = rng.randrange(N) if u1 is None else u1
                b = rng.randrange(1, N) if u2 is None else u2
                row = _verify_row(orc, a, b, d, (a + b * d) % N, (u1, u2), tag)
        else:
            for j in range(len(keys)):
                d = keys[(i + j) % len(keys)]
                row = _verify_row(orc, u1, u2, d, (u1 + u2 * d) % N, (u1, u2), tag)
                if row is not None:
                    break
        if row is None:
            unreachable.append((tag, u1, u2))
        else:
            rows.append(row)
    return rows, unreachable


def recover_row(orc, u1, u2, k, tag=""):
    """the recovery row with R = k*G that returns Q = u1*G + u2*R: r = x(R), s = u2*r, z = -u1*r, recid = parity of y(R)"""
    R = mul_g(orc, k)
    q = (u1 + u2 * k) % N
    assert R[0] < N and u2 and q, "pick another k"
    r = R[0]
    return Row("recover", _b(-u1 * r % N), _b(r) + _b(u2 * r % N), None, (u1, u2), tag, recid=R[1] & 1, expect=ser33(mul_g(orc, q)))


def twin(row, bits, w0):
    """the near-miss twin: the row's (r, s) and key with z' = (u1 +- 2^(bits*w)) * s (recovery: -(u1 +- ..) * r) -- one digit of the G walk off by one"""
    v, w = near_miss_u1(row.u1, bits, w0)
    r, s = int.from_bytes(row.sig[:32], "big"), int.from_bytes(row.sig[32:], "big")
    z = v * s % N if row.kind == "verify" else -v * r % N
    t = Row(row.kind, _b(z), row.sig, row.key, (v, row.u2), row.tag + "~w%d" % w, recid=row.recid, expect=False if row.kind == "verify" else None)
    assert (t.u1, t.u2) == (v, row.u2)
    return t


def with_twins(rows, bits):
    """rows and twins interleaved (row 2i, its twin 2i + 1): the twin's window walks through all of them"""
    out = []
    for i, r in enumerate(rows):
        out += [r, twin(r, bits, i % windows(bits))]
    return out


# ---- the row sets every test takes its rows from
def pair_lists(bits, seed=SEED, per=4):
    """the three lists of (tag, u1, u2) the issue names: every u1 pattern x a random u2, a random u1 x every u2, and a sample of the cross product
    (`per` u2 values for every u1 pattern, walking through the u2 list so that every u2 is met)"""
    pats, u2s = u1_patterns(bits, seed), u2_list(seed)
    a = [("u1:" + n, u, None) for n, u in pats]
    b = [("u2:%d" % j, None, v) for j, v in enumerate(u2s)]
    c = [("x:%s:%d" % (n, (i * per + j) % len(u2s)), u, u2s[(i * per + j) % len(u2s)]) for i, (n, u) in enumerate(pats) for j in range(per)]
    assert len(pats) * per >= len(u2s)
    return a, b, c


def cross_product(bits, seed=SEED):
    pats, u2s = u1_patterns(bits, seed), u2_list(seed)
    return [("x:%s:%d" % (n, j), u, v) for n, u in pats for j, v in enumerate(u2s)]


_SETS = {}


def row_sets(orc, bits, seed=SEED, per=4):
    """{"own": rows under keys of their own (the ladder), "fixed": rows under the key pool (table paths), "unreachable": the pairs of the cross-product
    sample no key of the pool reaches, "recover": recovery rows with distinct r, "recover_shared": the same pairs with 32 rows per r}, each list with
    its twins interleaved.  Built once per (bits, seed, per) and shared: treat as read-only."""
    key = (bits, seed, per)
    if key not in _SETS:
        a, b, c = pair_lists(bits, seed, per)
        rng = random.Random(seed * 1000 + 4)
        fill = lambda p: [(t, rng.randrange(N) if u1 is None else u1, rng.randrange(1, N) if u2 is None else u2) for t, u1, u2 in p]
        own = [verify_row_own_key(orc, rng, u1, u2, t) for t, u1, u2 in fill(a + b + c)]
        fixed, unreachable = verify_rows_fixed_keys(orc, rng, a + b + c, key_pool(seed))
        rec_pairs = fill(a + b + c)
        rec = [recover_row(orc, u1, u2, rng.randrange(1, N), t) for t, u1, u2 in rec_pairs]
        ks = [rng.randrange(1, N) for _ in range((len(rec_pairs) + 31) // 32)]
        shared = [recover_row(orc, u1, u2, ks[i // 32], t) for i, (t, u1, u2) in enumerate(rec_pairs)]
        _SETS[key] = {"own": with_twins(own, bits), "fixed": with_twins(fixed, bits), "unreachable": unreachable,
                      "recover": with_twins(rec, bits), "recover_shared": with_twins(shared, bits)}
    return _SETS[key]


def reached_patterns(rows, bits, seed=SEED):
    """names of the u1 patterns some accepting row of `rows` hits exactly"""
    byval = {}
    for n, u in u1_patterns(bits, seed):
        byval.setdefault(u, []).append(n)
    return {n for r in rows if r.expect not in (False, None) and r.exact() for n in byval.get(r.u1, [])}


def columns(rows, publen=65):
    """numpy uint8 columns (hash [n,32], sig [n,64], key [n,publen] or recid [n])"""
    import numpy as np
    col = lambda items, w: np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), w).copy()
    hs, sg = col([r.hash for r in rows], 32), col([r.sig for r in rows], 64)
    if rows[0].kind == "recover":
        return hs, sg, np.array([r.recid for r in rows], dtype=np.uint8)
    keys = [r.key if publen == 65 else bytes([2 + (r.key[64] & 1)]) + r.key[1:33] for r in rows]
    return hs, sg, col(keys, publen)

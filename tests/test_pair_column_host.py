"""The comb column's group law on the host (tests/c/pair_column_host.cpp: lightning_amd/csrc/group.h with magnitude assertions on): the column's two
table points are summed first (ge_add_ge_fast, affine + affine -> Jacobian with Z^2, Z^3) and that pair is added to the accumulator
(gej_add_pair_fast), where two successive mixed additions (gej_add_ge_fast) stood before.  CPU only."""
import ctypes
import os
import random
import subprocess

import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = pyref.P
LIM29, LIM24 = (1 << 29) + (1 << 21), (1 << 24) + (1 << 13)     # fe.h: the limb bounds of a magnitude-1 value
M29 = (1 << 29) - 1


@pytest.fixture(scope="module")
def pc():
    so = os.path.join(HERE, "libpair_column_host.so")
    src = os.path.join(HERE, "c", "pair_column_host.cpp")
    deps = [src] + [os.path.join(ROOT, "lightning_amd", "csrc", f) for f in ("lamd_common.h", "fe.h", "group.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
    return ctypes.CDLL(so)


def limbs(v):
    """canonical limbs of v in [0, 2^256)"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l)) % P


def arr(*ls):
    flat = [x for l in ls for x in l]
    return (ctypes.c_uint32 * len(flat))(*flat)


def rand_point(rnd):
    while True:
        pt = pyref.lift_x(rnd.randrange(P))
        if pt is not None:
            return pt if rnd.random() < 0.5 else pyref.pneg(pt)


def jacobian(rnd, pt, zmag):
    """pt with a random Z as the accumulator's 27 limbs; zmag 2: Z's limbs doubled, as gej_double leaves them (Z3 = 2*Y*Z)"""
    z = rnd.randrange(1, P)
    zl = limbs(z) if zmag == 1 else [2 * x for x in limbs(z * pow(2, -1, P) % P)]
    return limbs(pt[0] * z * z % P) + limbs(pt[1] * pow(z, 3, P) % P) + zl


def affine(acc):
    z = val(acc[18:27])
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (val(acc[0:9]) * zi * zi % P, val(acc[9:18]) * pow(zi, 3, P) % P)


def pair_of(pc, p1, neg1, p2, neg2):
    out = (ctypes.c_uint32 * 45)()
    pc.pc_pair(arr(limbs(p1[0]), limbs(p1[1])), neg1, arr(limbs(p2[0]), limbs(p2[1])), neg2, out)
    return list(out)


def add_pair(pc, acc, zmag, pair):
    out = (ctypes.c_uint32 * 27)()
    m = pc.pc_add_pair(arr(acc), zmag, arr(pair), out)
    return list(out), m


def add_two(pc, acc, zmag, p1, neg1, p2, neg2):
    out = (ctypes.c_uint32 * 27)()
    m = pc.pc_add_two(arr(acc), zmag, arr(limbs(p1[0]), limbs(p1[1])), neg1, arr(limbs(p2[0]), limbs(p2[1])), neg2, out)
    return list(out), m


def double(pc, acc, zmag):
    out = (ctypes.c_uint32 * 27)()
    m = pc.pc_double(arr(acc), zmag, out)
    return list(out), m


def signed(pt, neg):
    return pyref.pneg(pt) if neg else pt


def test_pair_sum_then_pair_addition_equals_two_mixed_additions(pc):
    rnd = random.Random(0x9a17)
    for it in range(320):
        a, p1, p2 = rand_point(rnd), rand_point(rnd), rand_point(rnd)
        neg1, neg2 = (it >> 0) & 1, (it >> 1) & 1          # every combination of the lazy negation
        zmag = 1 + ((it >> 2) & 1)
        acc = jacobian(rnd, a, zmag)
        pair = pair_of(pc, p1, neg1, p2, neg2)
        want_pair = pyref.padd(signed(p1, neg1), signed(p2, neg2))
        assert affine(pair[:27]) == want_pair                                  # the first column: the pair IS the accumulator
        assert val(pair[27:36]) == pow(val(pair[18:27]), 2, P) and val(pair[36:45]) == pow(val(pair[18:27]), 3, P)
        new, _ = add_pair(pc, acc, zmag, pair)
        old, _ = add_two(pc, acc, zmag, p1, neg1, p2, neg2)
        assert affine(new) == affine(old) == pyref.padd(a, want_pair), it
        # and a column further: doubling, then the next pair
        q1, q2 = rand_point(rnd), rand_point(rnd)
        d, dm = double(pc, new, 1)
        new2, _ = add_pair(pc, d, dm, pair_of(pc, q1, neg2, q2, neg1))
        old2, _ = add_two(pc, d, dm, q1, neg2, q2, neg1)
        dbl = pyref.padd(affine(new), affine(new))
        assert affine(new2) == affine(old2) == pyref.padd(dbl, pyref.padd(signed(q1, neg2), signed(q2, neg1))), it


def _bound_fe(rnd, mag=1):
    """limbs at or near the bounds of a magnitude-`mag` value (not canonical: the formulas are identities in the field)"""
    mode = rnd.random()
    if mode < 0.4:
        return [mag * LIM29] * 8 + [mag * LIM24]
    if mode < 0.5:
        return [0] * 9
    if mode < 0.7:
        return [mag * LIM29 - rnd.randrange(4) for _ in range(8)] + [mag * LIM24 - rnd.randrange(4)]
    return [rnd.randrange(mag * LIM29 + 1) for _ in range(8)] + [rnd.randrange(mag * LIM24 + 1)]


def test_formulas_at_the_magnitude_bounds(pc):
    """every input limb at the largest value a caller can hand over -- table entries as raw limbs (magnitude 1, y magnitude 2 after the lazy
    negation), the accumulator's x, y of magnitude 1 and z of magnitude 2 after a doubling: the host build's assertions watch every
    intermediate magnitude and column sum, and the results equal the formulas evaluated on integers"""
    rnd = random.Random(0xb0d5)
    for it in range(300):
        x1, y1, x2, y2 = (_bound_fe(rnd) for _ in range(4))
        neg1, neg2 = it & 1, (it >> 1) & 1
        out = (ctypes.c_uint32 * 45)()
        pc.pc_pair(arr(x1, y1), neg1, arr(x2, y2), neg2, out)
        pair = list(out)
        vx1, vx2 = val(x1), val(x2)
        vy1, vy2 = (-val(y1) if neg1 else val(y1)) % P, (-val(y2) if neg2 else val(y2)) % P
        h, r = (vx2 - vx1) % P, (vy2 - vy1) % P
        x3 = (r * r - h ** 3 - 2 * vx1 * h * h) % P
        y3 = (r * (vx1 * h * h - x3) - vy1 * h ** 3) % P
        assert [val(pair[9 * i:9 * i + 9]) for i in range(5)] == [x3, y3, h, h * h % P, h ** 3 % P], it
        zmag = 1 + ((it >> 2) & 1)
        acc = _bound_fe(rnd) + _bound_fe(rnd) + _bound_fe(rnd, zmag)
        b = [_bound_fe(rnd) for _ in range(5)] if it % 3 else [pair[9 * i:9 * i + 9] for i in range(5)]
        got, m = add_pair(pc, acc, zmag, [x for l in b for x in l])
        assert m <= 2
        X1, Y1, Z1 = val(acc[0:9]), val(acc[9:18]), val(acc[18:27])
        X2, Y2, Z2, ZZ2, ZZZ2 = (val(l) for l in b)
        u1, s1 = X1 * ZZ2 % P, Y1 * ZZZ2 % P
        h, r = (X2 * Z1 * Z1 - u1) % P, (Y2 * Z1 ** 3 - s1) % P
        x3 = (r * r - h ** 3 - 2 * u1 * h * h) % P
        y3 = (r * (u1 * h * h - x3) - s1 * h ** 3) % P
        assert [val(got[0:9]), val(got[9:18]), val(got[18:27])] == [x3, y3, Z1 * Z2 * h % P], it


def test_degenerate_columns_leave_a_zero_z_that_stays(pc):
    """E1 = +-E2 inside a column and an accumulator equal to +- the pair are not excluded by an argument about honest scalars but caught: each
    leaves Z = 0, the zero survives the next column (doubling + pair addition) and is what the one test at the end (ZZ of the XYZZ form) sees"""
    rnd = random.Random(0xdea1)
    for it in range(24):
        a, p1, p2, q1, q2 = (rand_point(rnd) for _ in range(5))
        zmag = 1 + (it & 1)
        n1, n2 = (it >> 1) & 1, (it >> 2) & 1
        good = pair_of(pc, p1, n1, p2, n2)
        s = pyref.padd(signed(p1, n1), signed(p2, n2))
        zero_states = []
        for same_sign in (True, False):                      # E1 = E2 and E1 = -E2
            bad = pair_of(pc, p1, n1, p1, n1 if same_sign else 1 - n1)
            assert val(bad[18:27]) == 0 and val(bad[27:36]) == 0 and val(bad[36:45]) == 0
            zero_states.append((bad[:27], 1))                # the first column: that pair is the accumulator
            zero_states.append(add_pair(pc, jacobian(rnd, a, zmag), zmag, bad))
        for sign in (0, 1):                                  # accumulator = +pair and = -pair
            zero_states.append(add_pair(pc, jacobian(rnd, signed(s, sign), zmag), zmag, good))
        for st, m in zero_states:
            assert val(st[18:27]) == 0 and affine(st) is None
            assert pc.pc_zz_is_zero(arr(st), m) == 1
            d, dm = double(pc, st, m)
            nxt, nm = add_pair(pc, d, dm, pair_of(pc, q1, n2, q2, n1))
            assert val(nxt[18:27]) == 0
            assert pc.pc_zz_is_zero(arr(nxt), nm) == 1
        ok, m = add_pair(pc, jacobian(rnd, a, zmag), zmag, good)
        assert pc.pc_zz_is_zero(arr(ok), m) == 0 and affine(ok) == pyref.padd(a, s)

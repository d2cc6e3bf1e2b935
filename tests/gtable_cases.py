"""Corruptions of a G-table image and the bad set the audit's relations predict for them (lightning_amd/csrc/table_audit.h).  Shared by the host
tests (tests/test_devmath_host.py: 8-bit and 11-bit windows) and the device tests (tests/test_gpu_tables.py: 24-bit windows).

An image is a numpy uint32 array [count, 16] holding the entries [first, first + count) of a table: x | y, eight little-endian words each.  `src(idx)`
returns the TRUE entry at any flat index (window << bits | digit) as 16 words."""
import numpy as np

import pyref

P = pyref.P
ZERO, NONCANON, OFF_CURVE, ANCHOR, X, Y, DEGENERATE = 1, 2, 4, 8, 16, 32, 64


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def entry(x, y):
    return np.array(words(x) + words(y), dtype=np.uint32)


def xy(e):
    return (sum(int(e[i]) << (32 * i) for i in range(8)), sum(int(e[8 + i]) << (32 * i) for i in range(8)))


def small_x_point():
    """a curve point whose x is so small that x + p still fits 256 bits"""
    x = 1
    while True:
        y = pow(x ** 3 + 7, (P + 1) // 4, P)
        if y * y % P == (x ** 3 + 7) % P:
            assert x + P < 1 << 256
            return x, y
        x += 1


def small_y_point():
    """... and one with such a y (p = 7 mod 9: a cubic residue a has the cube root a^((p + 2) / 9))"""
    assert P % 9 == 7
    y = 1
    while True:
        a = (y * y - 7) % P
        x = pow(a, (P + 2) // 9, P)
        if pow(x, 3, P) == a:
            assert y + P < 1 << 256
            return x, y
        y += 1


def affected(corrupted, bits, nwin):
    """every flat index whose rule reads a corrupted entry: the entry itself; its successor (entry 1 of the next window for the last digit); for a
    window's entry 1 the whole window and entry 1 of the next"""
    last = (1 << bits) - 1
    out = set()
    for c in corrupted:
        w, d = c >> bits, c & last
        out.add(c)
        if d == 0:
            continue
        if d == 1:
            out.update(range(c + 1, c + last))
        elif d != last:
            out.add(c + 1)
        if d in (1, last) and w + 1 < nwin:
            out.add(((w + 1) << bits) | 1)
    return out


# Each class: f(img, first, i, src) corrupts the image around flat index i (first <= i < first + len(img)) in place and returns
# (the set of flat indices it changed, bits the reason mask of entry i must have, bits it must not have).
def flip_x_bit(img, first, i, src):
    img[i - first, 2] ^= 1 << 13
    return {i}, OFF_CURVE, ZERO | NONCANON


def flip_y_bit(img, first, i, src):
    img[i - first, 8] ^= 1 << 5
    return {i}, OFF_CURVE, ZERO | NONCANON


def negate_y(img, first, i, src):
    x, y = xy(img[i - first])
    img[i - first] = entry(x, P - y)
    return {i}, 0, ZERO | NONCANON | OFF_CURVE | X | DEGENERATE      # the x relations cannot tell y from -y: the y relation (or the anchor) must


def swap_neighbours(img, first, i, src):
    j = i + 1 if i + 1 < first + len(img) else i - 1
    img[[i - first, j - first]] = img[[j - first, i - first]]
    return {i, j}, 0, ZERO | NONCANON | OFF_CURVE | ANCHOR


def replace_by_d_plus_2(img, first, i, src):
    img[i - first] = src(i + 2)
    return {i}, 0, ZERO | NONCANON | OFF_CURVE


def noncanonical_x(img, first, i, src):
    x, y = small_x_point()
    img[i - first] = entry(x + P, y)
    return {i}, NONCANON, ZERO | OFF_CURVE


def noncanonical_y(img, first, i, src):
    x, y = small_y_point()
    img[i - first] = entry(x, y + P)
    return {i}, NONCANON, ZERO | OFF_CURVE


def canonical_small_x(img, first, i, src):
    """the control of noncanonical_x: the same foreign point stored canonically is wrong for the relations only"""
    x, y = small_x_point()
    img[i - first] = entry(x, y)
    return {i}, 0, ZERO | NONCANON | OFF_CURVE


def off_curve_plausible(img, first, i, src):
    img[i - first, 8:] = src(i + 1)[8:]          # x of this multiple, y of the next: two words that both occur in the table
    return {i}, OFF_CURVE, ZERO | NONCANON


def all_zero(img, first, i, src):
    img[i - first] = 0
    return {i}, OFF_CURVE, ZERO | NONCANON


# for entries with digit >= 2 and two more digits of the same window above them
GENERIC = [flip_x_bit, flip_y_bit, negate_y, swap_neighbours, replace_by_d_plus_2, noncanonical_x, noncanonical_y, canonical_small_x,
           off_curve_plausible, all_zero]


def nonzero_digit0(img, first, i, src):
    img[i - first, 15] = 1
    return {i}, ZERO, NONCANON | OFF_CURVE | ANCHOR | X | Y | DEGENERATE


def check(reasons, first, img_len, corrupted, bits, nwin, i, must, must_not, what):
    """reasons: uint32 [img_len], the audit's masks of [first, first + img_len).  The bad set is exactly the predicted one; entry i's mask is sensible"""
    got = {first + int(k) for k in np.nonzero(reasons)[0]}
    want = {j for j in affected(corrupted, bits, nwin) if first <= j < first + img_len}
    assert got == want, (what, i, sorted(got ^ want)[:10])
    r = int(reasons[i - first])
    assert r and (r & must) == must and not (r & must_not), (what, i, r)

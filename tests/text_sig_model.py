"""Sequential model of lamd_bolt11_check_batch and lamd_checkmessage_batch (include/lightning_amd.h), written the way the reference does the
work -- decode the whole string into a list, then walk it -- and NOT the way lightning_amd/csrc/bolt11.h streams it.  The curve work goes
through the oracles: oracle/orc.py (C) for batches, oracle/pyref.py (big integers) on request.  Also here: a bech32 invoice encoder and the
synthesised rows that tests/test_bolt11_host.py and tests/test_gpu_text_signatures.py share."""
import hashlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc  # noqa: E402
import pyref as R  # noqa: E402

CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
ZCHARS = "ybndrfg8ejkmcpqxot1uwisza345h769"
N = R.N
B11_OK, B11_BAD_BECH32, B11_BAD_PREFIX, B11_MALFORMED, B11_BAD_RECID, B11_SIG_RANGE, B11_NO_KEY, B11_BAD_SIGNATURE = 0, -1, -2, -3, -4, -5, -6, -7
MSG_OK, MSG_BAD_ZBASE, MSG_BAD_LENGTH, MSG_BAD_SIG, MSG_NO_KEY = 0, -1, -2, -3, -4
SIGNED_PREFIX = b"Lightning Signed Message:"
GEN = (0x3b6a57b2, 0x26508e6d, 0x1ea119fa, 0x3d4233dd, 0x2a1462b3)
BECH32M = 0x2bc830a3


def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "text_signatures.json")))


def _b(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def polymod(values):
    chk = 1
    for v in values:
        top = chk >> 25
        chk = ((chk & 0x1FFFFFF) << 5) ^ v
        for i in range(5):
            if (top >> i) & 1:
                chk ^= GEN[i]
    return chk


def bech32_decode(s):
    """bech32_decode() (common/bech32.c:94-155) without its length cap: (lower-cased hrp, data values without the checksum), or None"""
    s = _b(s)
    if len(s) < 8:
        return None
    sep = s.rfind(b"1")
    if sep < 1 or len(s) - sep - 1 < 6:          # no separator / empty hrp / no room for the checksum
        return None
    hrp, data = s[:sep], s[sep + 1:]
    if any(c < 33 or c > 126 for c in hrp):
        return None
    vals = []
    for c in data:
        if c & 0x80:
            return None
        k = CHARSET.find(chr(c).lower())
        if k < 0:
            return None
        vals.append(k)
    both = hrp + data
    if any(0x61 <= c <= 0x7a for c in both) and any(0x41 <= c <= 0x5a for c in both):
        return None
    low = hrp.lower()
    if polymod([c >> 5 for c in low] + [0] + [c & 31 for c in low] + vals) != 1:
        return None
    return low, vals[:-6]


def pack5(vals, pad):
    """5 -> 8 bits: (bytes, leftover bits as an integer, their count); pad = the last byte is filled with zero bits"""
    acc = bits = 0
    out = bytearray()
    for v in vals:
        acc = ((acc << 5) | v) & 0xFFFF
        bits += 5
        if bits >= 8:
            bits -= 8
            out.append((acc >> bits) & 0xFF)
    left = acc & ((1 << bits) - 1)
    if pad and bits:
        out.append((left << (8 - bits)) & 0xFF)
    return bytes(out), left, bits


def to5(b, pad=True):
    acc = bits = 0
    out = []
    for c in b:
        acc = ((acc << 8) | c) & 0xFFFF
        bits += 8
        while bits >= 5:
            bits -= 5
            out.append((acc >> bits) & 31)
    if bits:
        assert pad
        out.append((acc << (5 - bits)) & 31)
    return out


def bolt11_front(s):
    """what can be said before any curve arithmetic: dict(status in 0, -1 .. -5; hash, sig, recid, key, have_n)"""
    r = dict(status=0, hash=bytes(32), sig=bytes(64), recid=0, key=bytes(33), have_n=False)
    dec = bech32_decode(s)
    if dec is None:
        return dict(r, status=B11_BAD_BECH32)
    hrp, data = dec
    if not hrp.startswith(b"ln"):
        return dict(r, status=B11_BAD_PREFIX)
    bad = dict(r, status=B11_MALFORMED)
    left = len(data)            # data_len of bolt11_decode_nosig
    pos = 0
    if left < 7:                # the 35-bit timestamp
        return bad
    pos, left = 7, left - 7
    key = None
    while left > 104:
        tag, flen = data[pos], (data[pos + 1] << 5) | data[pos + 2]
        pos, left = pos + 3, left - 3
        if flen > left:
            return bad
        body = data[pos:pos + flen]
        pos, left = pos + flen, left - flen
        if tag == 19 and flen == 53 and key is None:    # decode_n: pull_expected_length(53), no padding allowed
            kb, extra, _ = pack5(body, False)
            key = kb
            if extra:
                return bad
    if left != 104:             # "can't read signature": pull_bits(520)
        return bad
    sig65, _, nbits = pack5(data[pos:], False)
    assert len(sig65) == 65 and nbits == 0
    h = hashlib.sha256(hrp + pack5(data[:pos], True)[0]).digest()
    r = dict(r, hash=h, sig=sig65[:64], recid=sig65[64], key=key or bytes(33), have_n=key is not None)
    if sig65[64] > 3:
        return dict(r, status=B11_BAD_RECID)
    if int.from_bytes(sig65[:32], "big") >= N or int.from_bytes(sig65[32:64], "big") >= N:
        return dict(r, status=B11_SIG_RANGE)
    return r


def _verify(h, sig, key, curve):
    if curve == "pyref":
        return bool(R.ecdsa_verify(h, sig, key))
    return bool(orc.ecdsa_verify(h, sig, key))


def _recover(h, sig, recid, curve):
    if curve == "pyref":
        pt = R.ecdsa_recover(h, sig, recid)
        return None if pt is None else R.ser33(pt)
    return orc.ecdsa_recover(h, sig, recid)


def _key_valid(key, curve):
    return (R.pubkey_parse(key) if curve == "pyref" else orc.pubkey_parse(key)) is not None


def bolt11_check(strings, curve="orc"):
    """-> (status int8 [n], node_id uint8 [n,33], hash uint8 [n,32], have_n bool [n]), row by row"""
    n = len(strings)
    status, node, hashes, have_n = np.zeros(n, np.int8), np.zeros((n, 33), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, bool)
    for i, s in enumerate(strings):
        f = bolt11_front(s)
        st = f["status"]
        if st in (0, B11_BAD_RECID, B11_SIG_RANGE) and f["have_n"] and not _key_valid(f["key"], curve):
            f = dict(f, status=B11_MALFORMED, hash=bytes(32), have_n=False)    # decode_n fails inside the walk
            st = B11_MALFORMED
        key = None
        if st == 0:
            if f["have_n"]:
                if _verify(f["hash"], f["sig"], f["key"], curve):
                    key = f["key"]
                else:
                    st = B11_BAD_SIGNATURE
            else:
                key = _recover(f["hash"], f["sig"], f["recid"], curve)
                if key is None:
                    st = B11_NO_KEY
        status[i] = st
        if key is not None:
            node[i] = np.frombuffer(key, np.uint8)
        hashes[i] = np.frombuffer(f["hash"], np.uint8)
        have_n[i] = f["have_n"]
    return status, node, hashes, have_n


def from_zbase32(zb):
    """from_zbase32() (lightningd/signmessage.c:36-55): the bytes, or None"""
    vals = []
    for c in _b(zb):
        k = ZCHARS.find(chr(c)) if c < 128 else -1
        if k < 0:
            return None
        vals.append(k)
    out, left, bits = pack5(vals, False)
    if bits:                    # len != tal_bytelen: 5 * count is no multiple of 8
        return None
    return out


def checkmessage_front(msg, zb):
    r = dict(status=0, hash=bytes(32), sig=bytes(64), recid=0)
    raw = from_zbase32(zb)
    if raw is None:
        return dict(r, status=MSG_BAD_ZBASE)
    if len(raw) != 65:
        return dict(r, status=MSG_BAD_LENGTH)
    r = dict(r, sig=raw[1:], recid=(raw[0] - 31) & 0xFF)
    if not 0 <= raw[0] - 31 <= 3:
        return dict(r, status=MSG_BAD_SIG)
    if int.from_bytes(raw[1:33], "big") >= N or int.from_bytes(raw[33:], "big") >= N:
        return dict(r, status=MSG_BAD_SIG)
    return dict(r, hash=hashlib.sha256(hashlib.sha256(SIGNED_PREFIX + _b(msg)).digest()).digest())


def checkmessage(messages, zbases, curve="orc"):
    n = len(messages)
    status, node = np.zeros(n, np.int8), np.zeros((n, 33), np.uint8)
    for i, (m, z) in enumerate(zip(messages, zbases)):
        f = checkmessage_front(m.encode("utf-8") if isinstance(m, str) else m, z)
        st = f["status"]
        if st == 0:
            key = _recover(f["hash"], f["sig"], f["recid"], curve)
            if key is None:
                st = MSG_NO_KEY
            else:
                node[i] = np.frombuffer(key, np.uint8)
        status[i] = st
    return status, node


# ------------------------------------------------------------------------------------------------------------ encoders and signers
def bech32_encode(hrp, vals, const=1):
    """any hrp bytes, any 5-bit values; const = what the final polymod shall be (1: bech32)"""
    hrp = _b(hrp)
    low = hrp.lower()
    pre = [c >> 5 for c in low] + [0] + [c & 31 for c in low] + list(vals)
    pm = polymod(pre + [0] * 6) ^ const
    chk = [(pm >> (5 * (5 - i))) & 31 for i in range(6)]
    return hrp + b"1" + bytes(ord(CHARSET[v]) for v in list(vals) + chk)


def field(tag, vals):
    vals = list(vals)
    assert 0 <= tag < 32 and len(vals) < 1024
    return [tag, len(vals) >> 5, len(vals) & 31] + vals


def n_field(key33, last_bit=0, tag=19):
    v = to5(key33)          # 264 bits -> 53 values, the last one padded with one zero bit
    assert len(v) == 53
    v[52] |= last_bit
    return field(tag, v)


def body_values(timestamp, fields):
    out = [(timestamp >> (5 * (6 - i))) & 31 for i in range(7)]
    for f in fields:
        out += f
    return out


class Signer:
    """deterministic keys and nonces; signs through the C oracle"""

    def __init__(self, seed):
        self.rnd = random.Random(seed)

    def scalar(self):
        return self.rnd.randrange(1, N).to_bytes(32, "big")

    def key(self):
        sec = self.scalar()
        pub = orc.pubkey_create(sec)
        x, y = pub[-64:-32], pub[-32:]
        return sec, bytes([2 + (y[-1] & 1)]) + x

    def sign(self, h, sec, pub33):
        """-> (sig64 low-S, recid)"""
        sig = orc.ecdsa_sign(h, sec, self.scalar())
        for recid in range(4):
            if orc.ecdsa_recover(h, sig, recid) == pub33:
                return sig, recid
        raise AssertionError("no recovery id")


def invoice_hash(hrp, body):
    return hashlib.sha256(_b(hrp).lower() + pack5(body, True)[0]).digest()


def assemble(hrp, body, sig64, recid, const=1):
    return bech32_encode(hrp, list(body) + to5(bytes(sig64) + bytes([recid]), False), const)


def high_s(sig64):
    return sig64[:32] + (N - int.from_bytes(sig64[32:], "big")).to_bytes(32, "big")


def zbase_encode(raw):
    return "".join(ZCHARS[v] for v in to5(raw))


def signed_message(signer, msg, sec, pub):
    h = hashlib.sha256(hashlib.sha256(SIGNED_PREFIX + msg).digest()).digest()
    sig, recid = signer.sign(h, sec, pub)
    return zbase_encode(bytes([31 + recid]) + sig)


P_FIELD = field(1, to5(bytes(range(32))))     # a payment hash, so the rows look like invoices


def synth_invoices(seed=11):
    """[(name, string, expected status or None = whatever the model says)] -- the synthesised classes: `n` fields, bech32 faults, framing, SHA-256 padding edges"""
    S = Signer(seed)
    rows = []
    sec, pub = S.key()
    sec2, pub2 = S.key()
    hrp = b"lnbc2500u"
    ts = 1496314658
    plain = body_values(ts, [P_FIELD])
    withn = body_values(ts, [P_FIELD, n_field(pub)])

    def signed(name, body, expect, key=(sec, pub), h=hrp, mut=None, const=1):
        hh = invoice_hash(h, body)
        sig, recid = S.sign(hh, key[0], key[1])
        if mut:
            sig, recid = mut(sig, recid)
        rows.append((name, assemble(h, body, sig, recid, const), expect))

    # -- `n` fields
    signed("n/good", withn, 0)
    signed("plain/good", plain, 0)
    signed("n/high-s", withn, B11_BAD_SIGNATURE, mut=lambda s, r: (high_s(s), r ^ 1))
    signed("plain/high-s", plain, 0, mut=lambda s, r: (high_s(s), r ^ 1))
    for k in (1, 2, 3):
        signed("n/wrong-recid-%d" % k, withn, 0, mut=lambda s, r, k=k: (s, r ^ k))
    signed("n/recid4", withn, B11_BAD_RECID, mut=lambda s, r: (s, 4))
    signed("plain/recid4", plain, B11_BAD_RECID, mut=lambda s, r: (s, 4))
    signed("plain/recid255", plain, B11_BAD_RECID, mut=lambda s, r: (s, 255))
    nb = N.to_bytes(32, "big")
    signed("n/r=n", withn, B11_SIG_RANGE, mut=lambda s, r: (nb + s[32:], r))
    signed("plain/r=n", plain, B11_SIG_RANGE, mut=lambda s, r: (nb + s[32:], r))
    signed("plain/s=n", plain, B11_SIG_RANGE, mut=lambda s, r: (s[:32] + nb, r))
    signed("plain/s=2^256-1", plain, B11_SIG_RANGE, mut=lambda s, r: (s[:32] + b"\xff" * 32, r))
    signed("n/r=n-1", withn, B11_BAD_SIGNATURE, mut=lambda s, r: ((N - 1).to_bytes(32, "big") + s[32:], r))
    signed("n/r=0", withn, B11_BAD_SIGNATURE, mut=lambda s, r: (bytes(32) + s[32:], r))
    signed("n/s=0", withn, B11_BAD_SIGNATURE, mut=lambda s, r: (s[:32] + bytes(32), r))
    signed("plain/r=0", plain, B11_NO_KEY, mut=lambda s, r: (bytes(32) + s[32:], r))
    signed("plain/s=0", plain, B11_NO_KEY, mut=lambda s, r: (s[:32] + bytes(32), r))
    signed("n/wrong-signer", withn, B11_BAD_SIGNATURE, key=(sec2, pub2))
    signed("n/trailing-bit", body_values(ts, [P_FIELD, n_field(pub, last_bit=1)]), B11_MALFORMED)
    x = int.from_bytes(pub[1:], "big")
    while R.lift_x(x) is not None:
        x += 1
    signed("n/off-curve", body_values(ts, [P_FIELD, n_field(b"\x02" + x.to_bytes(32, "big"))]), B11_MALFORMED)
    signed("n/prefix04", body_values(ts, [P_FIELD, n_field(b"\x04" + pub[1:])]), B11_MALFORMED)
    signed("n/off-curve+recid4", body_values(ts, [P_FIELD, n_field(b"\x02" + x.to_bytes(32, "big"))]), B11_MALFORMED, mut=lambda s, r: (s, 4))
    two = body_values(ts, [n_field(pub), P_FIELD, n_field(pub2)])
    signed("n/two/first-signs", two, 0)
    signed("n/two/second-signs", two, B11_BAD_SIGNATURE, key=(sec2, pub2))
    signed("n/two/second-invalid", body_values(ts, [n_field(pub), n_field(b"\x04" + pub[1:])]), 0)
    for ln in (52, 54):
        wrong = field(19, to5(pub)[:52] if ln == 52 else to5(pub) + [0])
        b = body_values(ts, [wrong, P_FIELD, n_field(pub2)])
        signed("n/wrong-length-%d/second-signs" % ln, b, 0, key=(sec2, pub2))
        signed("n/wrong-length-%d/first-signs" % ln, b, B11_BAD_SIGNATURE)
        signed("n/wrong-length-%d/alone" % ln, body_values(ts, [wrong, P_FIELD]), 0)      # no key: recovery
    # -- bech32 faults
    good = assemble(hrp, withn, *S.sign(invoice_hash(hrp, withn), sec, pub))
    assert bolt11_front(good)["status"] == 0
    at = len(hrp) + 1 + 30
    rows.append(("bech32/flipped-char", good[:at] + (b"q" if good[at:at + 1] != b"q" else b"p") + good[at + 1:], B11_BAD_BECH32))
    signed("bech32/bech32m", withn, B11_BAD_BECH32, const=BECH32M)
    rows.append(("bech32/bit7", good[:at] + bytes([good[at] | 0x80]) + good[at + 1:], B11_BAD_BECH32))
    rows.append(("bech32/bit7-hrp", bytes([good[0] | 0x80]) + good[1:], B11_BAD_BECH32))
    rows.append(("bech32/one-in-data", good[:at] + b"1" + good[at + 1:], B11_BAD_BECH32))
    rows.append(("bech32/b-in-data", good[:at] + b"b" + good[at + 1:], B11_BAD_BECH32))
    rows.append(("bech32/space-in-hrp", b"ln c" + good[4:], B11_BAD_BECH32))
    rows.append(("bech32/mixed-case", good[:at] + good[at:].upper(), B11_BAD_BECH32))
    rows.append(("bech32/upper", good.upper(), 0))
    rows.append(("bech32/no-separator", good.replace(b"1", b"q"), B11_BAD_BECH32))
    rows.append(("bech32/empty-hrp", bech32_encode(b"", withn), B11_BAD_BECH32))
    rows.append(("bech32/short", b"ln1qqqq", B11_BAD_BECH32))
    rows.append(("bech32/empty", b"", B11_BAD_BECH32))
    signed("prefix/xn", withn, B11_BAD_PREFIX, h=b"xnbc2500u")
    signed("prefix/l", withn, B11_BAD_PREFIX, h=b"l")
    signed("prefix/l2n", withn, B11_BAD_PREFIX, h=b"l2n")
    signed("prefix/ln-alone", withn, 0, h=b"ln")
    # -- framing
    eat = body_values(ts, [P_FIELD]) + [3, 0, 5]            # a field whose five values are the first of the signature
    signed("framing/length-eats-signature", eat, B11_MALFORMED)
    signed("framing/length-past-end", body_values(ts, [P_FIELD]) + [3, 31, 31], B11_MALFORMED)
    signed("framing/header-in-signature-1", body_values(ts, [P_FIELD]) + [3], B11_MALFORMED)
    signed("framing/header-in-signature-2", body_values(ts, [P_FIELD]) + [3, 0], B11_MALFORMED)
    signed("framing/empty-field-last", body_values(ts, [P_FIELD]) + [3, 0, 0], 0)
    for m in (0, 6, 7, 110, 111):
        vals = [S.rnd.randrange(32) for _ in range(m)]
        rows.append(("framing/%d-values" % m, bech32_encode(hrp, vals), B11_MALFORMED if m < 111 else None))
    signed("framing/no-fields", body_values(ts, []), 0)
    # -- SHA-256 padding edges: hashed length L = len(hrp) + ceil(5 m / 8) for every L in 53..66 and 117..130, every m mod 8
    seen_l, seen_mod = set(), set()
    for hl, h in ((4, b"lnbc"), (5, b"lntb1")):
        for L in list(range(53, 67)) + list(range(117, 131)):
            for m in range(10, 220):
                if hl + (5 * m + 7) // 8 == L:
                    b = body_values(ts, [field(2, [S.rnd.randrange(32) for _ in range(m - 10)])])
                    assert len(b) == m
                    signed("sha/L=%d/m=%d" % (L, m), b, 0, h=h)
                    seen_l.add(L)
                    seen_mod.add(m % 8)
    assert seen_l == set(range(53, 67)) | set(range(117, 131)) and seen_mod == set(range(8))
    long_body = body_values(ts, [field(2 + (k % 5), [S.rnd.randrange(32) for _ in range(1023)]) for k in range(20)])
    signed("sha/long", long_body, 0)
    signed("sha/long+n", long_body + n_field(pub), 0)
    assert len(rows[-2][1]) > 20000
    return rows


def synth_messages(seed=12):
    """[(name, message bytes, zbase, expected status or None)]"""
    S = Signer(seed)
    sec, pub = S.key()
    rows = []
    for ln in (0, 30, 31, 38, 39, 40, 94, 95, 1000):
        msg = bytes(S.rnd.randrange(256) for _ in range(ln))
        rows.append(("len/%d" % ln, msg, signed_message(S, msg, sec, pub), 0))
    msg = b"a message"
    zb = signed_message(S, msg, sec, pub)
    raw = from_zbase32(zb)
    for ln in (0, 8, 96, 103, 104, 105, 112):
        z = (zb + "yyyyyyyy")[:ln]
        rows.append(("zbase/%d-chars" % ln, msg, z, MSG_OK if ln == 104 else MSG_BAD_LENGTH if ln % 8 == 0 else MSG_BAD_ZBASE))
    rows.append(("zbase/upper", msg, zb[:20] + zb[20].upper() + zb[21:], MSG_BAD_ZBASE if zb[20].isalpha() else None))
    rows.append(("zbase/upper-all", msg, zb.upper(), MSG_BAD_ZBASE))
    rows.append(("zbase/l", msg, zb[:50] + "l" + zb[51:], MSG_BAD_ZBASE))
    rows.append(("zbase/bit7", msg, zb.encode()[:50] + bytes([zb.encode()[50] | 0x80]) + zb.encode()[51:], MSG_BAD_ZBASE))
    rows.append(("zbase/bad-char-and-bad-length", msg, zb[:50] + "!", MSG_BAD_ZBASE))
    for b0 in (0, 30, 35, 255):
        rows.append(("sig/byte0=%d" % b0, msg, zbase_encode(bytes([b0]) + raw[1:]), MSG_BAD_SIG))
    for b0 in (31, 32, 33, 34):
        rows.append(("sig/byte0=%d" % b0, msg, zbase_encode(bytes([b0]) + raw[1:]), None))
    nb = N.to_bytes(32, "big")
    rows.append(("sig/r=n", msg, zbase_encode(raw[:1] + nb + raw[33:]), MSG_BAD_SIG))
    rows.append(("sig/s=n", msg, zbase_encode(raw[:33] + nb), MSG_BAD_SIG))
    rows.append(("sig/r=0", msg, zbase_encode(raw[:1] + bytes(32) + raw[33:]), MSG_NO_KEY))
    rows.append(("sig/s=0", msg, zbase_encode(raw[:33] + bytes(32)), MSG_NO_KEY))
    rows.append(("sig/high-s", msg, zbase_encode(raw[:1] + high_s(raw[1:])), 0))
    rows.append(("other-message", msg + b"modified", zb, None))
    return rows, pub


def random_invoices(n, seed):
    """a mixed batch: about half the rows carry `n`; every fifth row is damaged in one random character or one signature byte"""
    S = Signer(seed)
    keys = [S.key() for _ in range(4)]
    out = []
    for i in range(n):
        sec, pub = keys[S.rnd.randrange(4)]
        fields = [P_FIELD, field(13, [S.rnd.randrange(32) for _ in range(S.rnd.randrange(40))])]
        if S.rnd.randrange(2):
            fields.insert(S.rnd.randrange(3), n_field(pub))
        hrp = S.rnd.choice([b"lnbc", b"lntb20m", b"lnbcrt1u", b"LNBC5P"])
        body = body_values(S.rnd.randrange(1 << 35), fields)
        sig, recid = S.sign(invoice_hash(hrp, body), sec, pub)
        damage = S.rnd.randrange(2) if i % 5 == 4 else -1     # every fifth row: one signature byte or one character
        if damage == 0:
            k = S.rnd.randrange(64)
            sig = sig[:k] + bytes([sig[k] ^ (1 << S.rnd.randrange(8))]) + sig[k + 1:]
        s = assemble(hrp, body, sig, recid)
        if hrp.isupper():
            s = s.upper()
        if damage == 1:
            k = S.rnd.randrange(len(s))
            s = s[:k] + bytes([S.rnd.choice(b"qpzry9x8gf2tvdw0s3jn54khce6mua7l1bQ")]) + s[k + 1:]
        out.append(s)
    return out

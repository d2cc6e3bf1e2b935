"""Sequential model of lamd_bolt12_check_text_batch (include/lightning_amd.h), written the way the reference does the work -- collapse the string
into a new one, decode it into a list of values, pull the bytes, parse the fields into a list, then ask questions of that list -- and NOT the way
lightning_amd/csrc/bolt12_text.h streams it.  TLV parsing, merkle root, tagged hash, key parsing and BIP-340 come from oracle/pyref.py; batches
verify through the C oracle (oracle/orc.py).  Also here: the encoder, the signer (pyref.schnorr_sign: no signing code in the product) and the
synthesised rows that tests/test_bolt12_text_host.py and tests/test_gpu_bolt12_text.py share."""
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
OK, UNFINISHED, BAD_BECH32, BAD_PREFIX, MALFORMED, OUT_OF_RANGE, NO_KEY, NO_SIGNATURE, BAD_SIGNATURE = 0, -1, -2, -3, -4, -5, -6, -7, -8
KIND_NONE, KIND_OFFER, KIND_INVREQ, KIND_INVOICE = 0, 1, 2, 3
KINDS = {b"lno": KIND_OFFER, b"lnr": KIND_INVREQ, b"lni": KIND_INVOICE}
HRP = {v: k for k, v in KINDS.items()}
KEY_TYPE = {KIND_INVREQ: 88, KIND_INVOICE: 176}
MESSAGENAME = {KIND_INVREQ: b"invoice_request", KIND_INVOICE: b"invoice"}
SPACES = b" \t\n\v\f\r"          # ccan's cisspace
EMPTY_ID = hashlib.sha256(b"").digest()


def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bolt12_strings.json")))


def _b(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def collapse(s):
    """b12_string_to_data's first loop (common/bolt12.c:125-142): the collapsed string, or None = 'unfinished string'"""
    out = bytearray()
    have_plus = False
    for i, c in enumerate(s):
        if i != 0 and i + 1 != len(s) and not have_plus and c == 0x2b:
            have_plus = True
            continue
        if have_plus and c in SPACES:
            continue
        have_plus = False
        out.append(c)
    return None if have_plus else bytes(out)


def from_bech32_charset(b):
    """common/bech32_util.c:74-120 -> (lower-cased hrp, bytes) or None"""
    sep = b.find(b"1")
    if sep < 0:
        return None
    hrp = b[:sep].split(b"\0")[0]                # tal_strndup: a C string
    upper = any(0x41 <= c <= 0x5a for c in hrp)
    lower = any(0x61 <= c <= 0x7a for c in hrp)
    vals = []
    for c in b[sep + 1:]:
        if 0x41 <= c <= 0x5a:
            upper = True
            c += 32
        elif 0x61 <= c <= 0x7a:
            lower = True
        if c >= 128:
            return None
        k = CHARSET.find(chr(c))
        if k < 0:
            return None
        vals.append(k)
    if upper and lower:
        return None
    bits = "".join(format(v, "05b") for v in vals)
    pad = len(bits) % 8
    if pad >= 5:
        return None
    whole = len(bits) - pad
    if "1" in bits[whole:]:
        return None
    return hrp.lower(), bytes(int(bits[k:k + 8], 2) for k in range(0, whole, 8))


def ser(t, v):
    return R.bigsize(t) + R.bigsize(len(v)) + bytes(v)


def tlv_span(stream, minfield, maxfield):
    """common/bolt12.c:670-695 on a stream that parses, pointers as offsets and NULL as None -> the span's bytes.  Where the reference would
    compute NULL - start (start set, end never), the span is empty."""
    cursor = 0
    start = end = None
    while cursor < len(stream):
        before = cursor
        t, cursor = R.bigsize_read(stream, cursor)
        ln, cursor = R.bigsize_read(stream, cursor)
        if t >= minfield and start is None:
            start = before
        if t > maxfield:
            break
        cursor += ln
        end = cursor
    if start is None:
        start = end
    if start is None or end is None:
        return b""
    assert end >= start
    return stream[start:end]


def calc_offer(stream):
    return hashlib.sha256(tlv_span(stream, 1, 79) + tlv_span(stream, 1000000000, 1999999999)).digest()


def calc_invreq(stream):
    return hashlib.sha256(tlv_span(stream, 0, 159) + tlv_span(stream, 1000000000, 2999999999)).digest()


def _inside(t, ranges):
    return any(lo <= t <= hi for lo, hi in ranges)


def bolt12_front(s):
    """everything before key validity and the curve: dict(status in 0, -1 .. -7; kind, key, have_key, sig, sighash, offer_id, invreq_id)"""
    r = dict(status=0, kind=KIND_NONE, key=bytes(33), have_key=False, sig=bytes(64), sighash=bytes(32), offer_id=bytes(32), invreq_id=bytes(32))
    flat = collapse(_b(s))
    if flat is None:
        return dict(r, status=UNFINISHED)
    dec = from_bech32_charset(flat)
    if dec is None:
        return dict(r, status=BAD_BECH32)
    hrp, data = dec
    if hrp not in KINDS:
        return dict(r, status=BAD_PREFIX)
    kind = KINDS[hrp]
    r = dict(r, kind=kind)
    fields = R.tlv_stream_parse(data)
    if fields is None:
        return dict(r, status=MALFORMED)
    by = dict(fields)
    key = sig = None
    if kind != KIND_OFFER:
        key, sig = by.get(KEY_TYPE[kind]), by.get(240)
        if (key is not None and len(key) != 33) or (sig is not None and len(sig) != 64):
            return dict(r, status=MALFORMED)
    if key is not None:
        r = dict(r, key=bytes(key), have_key=True)
    if kind == KIND_OFFER and any(not _inside(t, ((1, 79), (1000000000, 1999999999))) for t, _ in fields):
        return dict(r, status=OUT_OF_RANGE)
    if kind == KIND_INVREQ and any(not 240 <= t <= 1000 and not _inside(t, ((0, 159), (1000000000, 2999999999))) for t, _ in fields):
        return dict(r, status=OUT_OF_RANGE)
    if kind != KIND_OFFER:
        if key is None:
            return dict(r, status=NO_KEY)
        if sig is None:
            return dict(r, status=NO_SIGNATURE)
    r = dict(r, offer_id=calc_offer(data))
    if kind == KIND_OFFER:
        return r
    return dict(r, invreq_id=calc_invreq(data), sig=bytes(sig), sighash=R.bolt12_sighash(MESSAGENAME[kind], b"signature", R.bolt12_merkle(fields)))


def bolt12_check(strings, curve="orc"):
    """-> (status int8 [n], kind uint8 [n], signer uint8 [n,33], sighash, offer_id, invreq_id uint8 [n,32]), row by row"""
    n = len(strings)
    status, kind, signer = np.zeros(n, np.int8), np.zeros(n, np.uint8), np.zeros((n, 33), np.uint8)
    sighash, offer_id, invreq_id = (np.zeros((n, 32), np.uint8) for _ in range(3))
    for i, s in enumerate(strings):
        f = bolt12_front(s)
        st = f["status"]
        if f["have_key"] and st in (OK, OUT_OF_RANGE, NO_SIGNATURE):
            valid = (R.pubkey_parse(f["key"]) if curve == "pyref" else orc.pubkey_parse(f["key"])) is not None
            if not valid:                       # fromwire_pubkey fails inside fromwire_tlv
                f = dict(f, status=MALFORMED, sighash=bytes(32))
                st = MALFORMED
        if st == OK and f["kind"] != KIND_OFFER:
            verify = R.schnorr_verify if curve == "pyref" else orc.schnorr_verify
            if not verify(f["sighash"], f["key"][1:], f["sig"]):
                st = BAD_SIGNATURE
        status[i], kind[i] = st, f["kind"]
        sighash[i] = np.frombuffer(f["sighash"], np.uint8)
        if st == OK:
            offer_id[i] = np.frombuffer(f["offer_id"], np.uint8)
            invreq_id[i] = np.frombuffer(f["invreq_id"], np.uint8)
            if f["kind"] != KIND_OFFER:
                signer[i] = np.frombuffer(f["key"], np.uint8)
    return status, kind, signer, sighash, offer_id, invreq_id


def pinned(fx, check):
    """the counts the tests pin over the fixture's reference-held strings; check = bolt12_check or the engine's call of the same shape"""
    rows = fx["strings"]
    uniq = sorted({r["str"] for r in rows})
    st, kind, _, _, offer_id, invreq_id = check(uniq)
    by = {s: (int(a), int(k), bytes(o).hex(), bytes(i).hex()) for s, a, k, o, i in zip(uniq, st, kind, offer_id, invreq_id)}
    count = lambda k: sum(1 for s in uniq if by[s][:2] == (0, k))
    # an id the reference itself wrote down: the model's id of an accepted string is among the recorded ones
    known = {key: {r["hex"] for r in fx["recorded"] if r["key"] == key} for key in ("offer_id", "invreq_id")}
    with_offer_id = {k: {s for s in uniq if by[s][:2] == (0, k) and by[s][2] in known["offer_id"]} for k in (1, 2, 3)}
    with_invreq_id = {k: {s for s in uniq if by[s][:2] == (0, k) and by[s][3] in known["invreq_id"]} for k in (1, 2, 3)}
    for r in rows:                      # ids stated next to the string itself
        if by[r["str"]][0] == 0:
            assert r.get("offer_id", by[r["str"]][2]) == by[r["str"]][2], r
            assert r.get("invreq_id", by[r["str"]][3]) == by[r["str"]][3], r
    return dict(ok_invoices=count(3), ok_invreqs=count(2), ok_offers=count(1),
                no_key_invreqs=sorted(r["file"] for r in rows if by[r["str"]][:2] == (NO_KEY, 2)),
                offers_with_offer_id=len(with_offer_id[1]), invoices_with_offer_id=len(with_offer_id[3]),
                invreqs_with_invreq_id=len(with_invreq_id[2]), invoices_with_invreq_id=len(with_invreq_id[3]))


# ------------------------------------------------------------------------------------------------------------ encoder, signer, synthesised rows
def to5(b):
    bits = "".join(format(c, "08b") for c in b)
    bits += "0" * (-len(bits) % 5)
    return [int(bits[k:k + 5], 2) for k in range(0, len(bits), 5)]


def encode_vals(hrp, vals):
    return _b(hrp) + b"1" + bytes(ord(CHARSET[v]) for v in vals)


def encode(hrp, stream):
    """to_bech32_charset (common/bech32_util.c:133-148)"""
    return encode_vals(hrp, to5(stream))


def stream_of(fields):
    return b"".join(ser(t, v) for t, v in fields)


class Signer:
    """deterministic keys; BIP-340 signatures from oracle/pyref.py"""

    def __init__(self, seed):
        self.rnd = random.Random(seed)

    def key(self, parity=None):
        while True:
            d = self.rnd.randrange(1, R.N)
            pub = R.ser33(R.pubkey_create(d))
            if parity is None or pub[0] == parity:
                return d, pub

    def blob(self, n):
        return bytes(self.rnd.randrange(256) for _ in range(n))

    def sign(self, kind, fields, d):
        """the fields with field 240 put in its place"""
        fields = sorted([(t, bytes(v)) for t, v in fields if t != 240])
        h = R.bolt12_sighash(MESSAGENAME[kind], b"signature", R.bolt12_merkle(fields))
        return sorted(fields + [(240, R.schnorr_sign(h, d))])


def synth(seed=12):
    """[(name, string, expected status or None = whatever the model says)]: every class the GPU test lists.  A few dozen streams are signed; the
    other rows are mutations of them."""
    S = Signer(seed)
    rows = []
    d, pub = S.key(2)
    d3, pub3 = S.key(3)
    d2, pub2 = S.key()
    meta = (0, S.blob(16))
    invreq_f = S.sign(KIND_INVREQ, [meta, (10, b"coffee"), (22, pub2), (82, b"\x01"), (88, pub)], d)
    invoice_f = S.sign(KIND_INVOICE, [meta, (10, b"coffee"), (22, pub2), (88, pub3), (164, S.blob(4)), (168, S.blob(32)), (170, b"\x64"), (176, pub)], d)
    offer_f = [(10, b"coffee"), (22, pub2)]
    invreq, invoice, offer = encode("lnr", stream_of(invreq_f)), encode("lni", stream_of(invoice_f)), encode("lno", stream_of(offer_f))
    add = lambda name, s, want: rows.append((name, _b(s), want))
    add("good/offer", offer, OK)
    add("good/invreq", invreq, OK)
    add("good/invoice", invoice, OK)
    add("good/invoice-upper", invoice.upper(), OK)
    # -- the `+` forms of common/test/run-bolt12-format-string-test.c:188-215, over the signed invoice: four accepted, five refused
    cut = lambda *ws: [invoice[sum(ws[:k]):sum(ws[:k + 1])] for k in range(len(ws))] + [invoice[sum(ws):]]
    a, b, c = invoice[:40], invoice[40:90], invoice[90:]
    add("plus/after-first-char", invoice[:1] + b"+" + invoice[1:], OK)
    add("plus/several", b"+".join(cut(15, 31, 18, 70)), OK)
    p = cut(15, 31, 18, 70)
    add("plus/whitespace", p[0] + b"+ " + p[1] + b"+  " + p[2] + b"+\n" + p[3] + b"+\r\n " + p[4], OK)
    add("plus/at-end", invoice + b"+", BAD_BECH32)            # the last byte is never a join: a data character outside the alphabet
    add("plus/whitespace-at-end", invoice + b"+ ", UNFINISHED)
    add("plus/at-start", b"+" + invoice, BAD_PREFIX)          # the first byte is never a join: the hrp is "+lni"
    add("plus/whitespace-at-start", b"+ " + invoice, BAD_PREFIX)
    add("plus/double", invoice[:2] + b"++" + invoice[2:], BAD_PREFIX)      # the second one stays: the hrp is "ln+i"
    add("plus/double-in-data", a + b"++" + b + c, BAD_BECH32)
    add("plus/double-spaced", a + b"+ +" + b + c, BAD_BECH32)
    add("plus/whitespace-before", a + b" +" + b + c, BAD_BECH32)
    for ch in SPACES:
        add("space/%d-behind-plus" % ch, a + b"+" + bytes([ch]) + b + c, OK)
        add("space/%d-alone" % ch, a + bytes([ch]) + b + c, BAD_BECH32)
    add("space/nbsp-behind-plus", a + b"+\xa0" + b + c, BAD_BECH32)
    add("plus/unfinished-inner", a + b"+", BAD_BECH32)        # the last byte is never a join
    add("plus/unfinished", a + b"+\n", UNFINISHED)
    add("plus/unfinished-before-fault", b"lnx1b" + b"+ ", UNFINISHED)
    add("plus/in-hrp", b"l+ni" + invoice[3:], OK)
    add("plus/before-separator", b"lni+\n" + invoice[3:], OK)
    # -- separator, hrp, case, alphabet
    add("bech32/no-separator", invoice.replace(b"1", b"q"), BAD_BECH32)
    add("bech32/empty-hrp", invoice[3:], BAD_PREFIX)
    add("bech32/empty", b"", BAD_BECH32)
    add("bech32/separator-alone", b"1", BAD_PREFIX)
    add("bech32/second-one-in-data", a + b"1" + b + c, BAD_BECH32)
    add("prefix/lnx", b"lnx" + invoice[3:], BAD_PREFIX)
    add("prefix/ln", b"ln" + invoice[3:], BAD_PREFIX)
    add("prefix/lnii", b"lnii" + invoice[3:], BAD_PREFIX)
    add("prefix/nul-ends-hrp", b"lni\0zz" + invoice[3:], OK)
    add("prefix/nul-hides-case", b"lni\0ZZ" + invoice[3:], OK)
    add("case/mixed-hrp", b"lNi" + invoice[3:], BAD_BECH32)
    add("case/upper-hrp-lower-data", b"LNI" + invoice[3:], BAD_BECH32)
    add("case/mixed-data", a + b.upper() + c, BAD_BECH32)
    add("case/upper-digits-only", encode_vals("LNO", [0, 15, 0, 15, 0, 15, 0, 0]), None)
    add("bech32/byte-128", a + b"\x80" + b[1:] + c, BAD_BECH32)
    add("bech32/byte-255", a + b"\xff" + b[1:] + c, BAD_BECH32)
    add("bech32/b-in-data", a + b"b" + b[1:] + c, BAD_BECH32)
    add("bech32/byte-128-in-hrp", b"ln\xe9" + invoice[3:], BAD_PREFIX)
    # -- value counts and padding bits
    for count in (1, 3, 6, 9, 11, 14):
        add("pad/count-%d" % count, encode_vals("lno", [0] * count), BAD_BECH32)
    for count in (2, 4, 5, 7, 8):
        add("pad/count-%d-zero" % count, encode_vals("lno", [0] * count), None)
        add("pad/count-%d-last-bit" % count, encode_vals("lno", [0] * (count - 1) + [1]), None if count == 8 else BAD_BECH32)
    add("pad/count-2-high-spare-bit", encode_vals("lno", [0, 2]), BAD_BECH32)
    add("pad/empty-data-offer", b"lno1", OK)
    add("pad/empty-data-invreq", b"lnr1", NO_KEY)
    add("pad/empty-data-invoice", b"lni1", NO_KEY)
    # -- TLV rules
    raw = lambda hrp, stream, want, name: add(name, encode(hrp, stream), want)
    raw("lno", b"\xfd\x00\x0a\x01x", MALFORMED, "tlv/non-minimal-type")
    raw("lno", b"\x0a\xfd\x00\x01x", MALFORMED, "tlv/non-minimal-length")
    raw("lno", b"\xfe\x00\x00\xff\xff\x00", MALFORMED, "tlv/non-minimal-type-5")
    raw("lno", b"\xff\x00\x00\x00\x00\xff\xff\xff\xff\x00", MALFORMED, "tlv/non-minimal-type-9")
    raw("lno", b"\x0a\x01x\xfd\x01", MALFORMED, "tlv/truncated-type")
    raw("lno", b"\x0a\x01x\x0b", MALFORMED, "tlv/missing-length")
    raw("lno", b"\x0a\x01x\x0b\xfd\x01", MALFORMED, "tlv/truncated-length")
    raw("lno", b"\x0a\x01x\x0b\x02y", MALFORMED, "tlv/truncated-value")
    raw("lno", b"\x0a\xff\xff\xff\xff\xff\xff\xff\xff\xff", MALFORMED, "tlv/huge-length")
    raw("lno", b"\x0a\x01x\x0a\x01y", MALFORMED, "tlv/equal-types")
    raw("lno", b"\x0b\x01x\x0a\x01y", MALFORMED, "tlv/decreasing-types")
    raw("lno", stream_of([(10, b"x"), (1000000000, b"y"), (1999999999, b"")]), OK, "tlv/5-byte-types")
    raw("lno", stream_of([(10, b"x" * 300)]), OK, "tlv/3-byte-length")
    raw("lno", stream_of([(1 << 32, b"x")]), OUT_OF_RANGE, "tlv/9-byte-type")
    raw("lnr", stream_of([(88, pub), (240, bytes(64))]) + b"\x00", MALFORMED, "tlv/malformed-behind-key")
    # -- key and signature fields
    swap = lambda fields, t, v: [(ft, v if ft == t else fv) for ft, fv in fields]
    for kind, hrp, fields in ((KIND_INVREQ, "lnr", invreq_f), (KIND_INVOICE, "lni", invoice_f)):
        kt = KEY_TYPE[kind]
        tag = "invreq" if kind == KIND_INVREQ else "invoice"
        raw(hrp, stream_of(swap(fields, kt, pub[:32])), MALFORMED, "key/%s-32-bytes" % tag)
        raw(hrp, stream_of(swap(fields, kt, pub + b"\0")), MALFORMED, "key/%s-34-bytes" % tag)
        raw(hrp, stream_of(swap(fields, kt, b"\x04" + pub[1:])), MALFORMED, "key/%s-prefix-04" % tag)
        x = int.from_bytes(pub[1:], "big")
        while R.lift_x(x) is not None:
            x += 1
        off_curve = b"\x02" + x.to_bytes(32, "big")
        raw(hrp, stream_of(swap(fields, kt, off_curve)), MALFORMED, "key/%s-off-curve" % tag)
        raw(hrp, stream_of(swap(fields, kt, b"\x02" + R.P.to_bytes(32, "big"))), MALFORMED, "key/%s-x=p" % tag)
        raw(hrp, stream_of([f for f in swap(fields, kt, off_curve) if f[0] != 240]), MALFORMED, "key/%s-off-curve-no-signature" % tag)
        sig = dict(fields)[240]
        raw(hrp, stream_of(swap(fields, 240, sig[:63])), MALFORMED, "sig/%s-63-bytes" % tag)
        raw(hrp, stream_of(swap(fields, 240, sig + b"\0")), MALFORMED, "sig/%s-65-bytes" % tag)
        raw(hrp, stream_of([f for f in fields if f[0] != kt]), NO_KEY, "missing/%s-key" % tag)
        raw(hrp, stream_of([f for f in fields if f[0] != 240]), NO_SIGNATURE, "missing/%s-signature" % tag)
        raw(hrp, stream_of([f for f in fields if f[0] not in (kt, 240)]), NO_KEY, "missing/%s-both" % tag)
        flip = lambda v, k=5: v[:k] + bytes([v[k] ^ 4]) + v[k + 1:]
        raw(hrp, stream_of(swap(fields, 240, flip(sig))), BAD_SIGNATURE, "flip/%s-r" % tag)
        raw(hrp, stream_of(swap(fields, 240, flip(sig, 40))), BAD_SIGNATURE, "flip/%s-s" % tag)
        raw(hrp, stream_of(swap(fields, 10, b"coffef")), BAD_SIGNATURE, "flip/%s-field" % tag)
        raw(hrp, stream_of(swap(fields, kt, pub2)), BAD_SIGNATURE, "flip/%s-other-key" % tag)
        xk = int.from_bytes(pub[1:], "big")
        bit = next(k for k in range(256) if R.lift_x(xk ^ (1 << k)) is not None)      # one bit away, and a curve point again
        raw(hrp, stream_of(swap(fields, kt, pub[:1] + (xk ^ (1 << bit)).to_bytes(32, "big"))), BAD_SIGNATURE, "flip/%s-key-bit" % tag)
        raw(hrp, stream_of(swap(fields, kt, bytes([pub[0] ^ 1]) + pub[1:])), BAD_SIGNATURE, "flip/%s-parity-byte" % tag)     # the same x-only key, another leaf
        raw(hrp, stream_of(swap(fields, 240, R.P.to_bytes(32, "big") + sig[32:])), BAD_SIGNATURE, "range/%s-r=p" % tag)
        raw(hrp, stream_of(swap(fields, 240, b"\xff" * 32 + sig[32:])), BAD_SIGNATURE, "range/%s-r=2^256-1" % tag)
        raw(hrp, stream_of(swap(fields, 240, sig[:32] + R.N.to_bytes(32, "big"))), BAD_SIGNATURE, "range/%s-s=n" % tag)
        raw(hrp, stream_of(swap(fields, 240, bytes(64))), BAD_SIGNATURE, "range/%s-zero-signature" % tag)
        raw(hrp, stream_of(sorted(fields + [(241, b"second")])), OK, "sig/%s-241-beside-240" % tag)
        raw(hrp, stream_of(sorted(fields + [(1000, b"")])), OK, "sig/%s-1000-beside-240" % tag)
    # -- signatures over the invoice's own sighash that only the last steps of the BIP-340 test refuse (bip340_stage2.py): R = s*G - e*P has x(R) = r
    #    and an ODD y (the nonce is not negated); R is the point at infinity (s = e*d).  d is the key with even y (pub starts 02)
    body = sorted(f for f in invoice_f if f[0] != 240)
    h = R.bolt12_sighash(MESSAGENAME[KIND_INVOICE], b"signature", R.bolt12_merkle(body))
    k = int.from_bytes(R.sha256(b"odd_R" + h), "big") % R.N
    Rk = R.pmul(k, R.G)
    k = k if Rk[1] & 1 else R.N - k
    rx = Rk[0].to_bytes(32, "big")
    e = int.from_bytes(R.tagged_hash("BIP0340/challenge", rx + pub[1:] + h), "big") % R.N
    raw("lni", stream_of(sorted(body + [(240, rx + ((k + e * d) % R.N).to_bytes(32, "big"))])), BAD_SIGNATURE, "stage2/invoice-odd-R")
    raw("lni", stream_of(sorted(body + [(240, rx + ((R.N - k + e * d) % R.N).to_bytes(32, "big"))])), OK, "stage2/invoice-even-R-twin")
    raw("lni", stream_of(sorted(body + [(240, rx + (e * d % R.N).to_bytes(32, "big"))])), BAD_SIGNATURE, "stage2/invoice-R-inf")
    raw("lnr", stream_of(invoice_f), OUT_OF_RANGE, "kind/invoice-data-under-lnr")
    raw("lni", stream_of(invreq_f), NO_KEY, "kind/invreq-data-under-lni")
    raw("lno", stream_of(invreq_f), OUT_OF_RANGE, "kind/invreq-data-under-lno")
    raw("lnr", stream_of(offer_f), NO_KEY, "kind/offer-data-under-lnr")
    f03 = S.sign(KIND_INVOICE, [meta, (88, pub), (176, pub3)], d3)
    raw("lni", stream_of(f03), OK, "key/03-verifies")
    raw("lnr", stream_of(S.sign(KIND_INVREQ, [meta, (88, pub3)], d3)), OK, "key/03-verifies-invreq")
    # -- range boundaries
    for t, want in ((159, OK), (160, OUT_OF_RANGE), (161, OUT_OF_RANGE), (239, OUT_OF_RANGE), (241, OK), (1000, OK), (1001, OUT_OF_RANGE),
                    (999999999, OUT_OF_RANGE), (1000000000, OK), (2999999999, OK), (3000000000, OUT_OF_RANGE), (3000000001, OUT_OF_RANGE)):
        f = S.sign(KIND_INVREQ, [meta, (88, pub), (t, b"edge")], d)
        raw("lnr", stream_of(f), want, "range/invreq-%d" % t)
    raw("lnr", stream_of([f for f in S.sign(KIND_INVREQ, [meta, (88, pub), (160, b"edge")], d) if f[0] != 240]), OUT_OF_RANGE, "range/invreq-160-unsigned")
    for t, want in ((0, OUT_OF_RANGE), (1, OK), (79, OK), (80, OUT_OF_RANGE), (81, OUT_OF_RANGE), (240, OUT_OF_RANGE), (999999999, OUT_OF_RANGE),
                    (1000000000, OK), (1999999999, OK), (2000000000, OUT_OF_RANGE), (2000000001, OUT_OF_RANGE)):
        raw("lno", stream_of(sorted([(10, b"coffee"), (t, b"edge")])), want, "range/offer-%d" % t)
    raw("lni", stream_of(S.sign(KIND_INVOICE, [meta, (160, b"x"), (176, pub), (3000000001, b"edge"), (1 << 40, b"far")], d)), OK, "range/invoice-any")
    # the spans of the ids: nothing inside (SHA-256 of nothing), one side only, the null-pointer case (first field above the upper bound)
    raw("lni", stream_of(S.sign(KIND_INVOICE, [(176, pub)], d)), OK, "span/invoice-no-offer-fields")
    raw("lni", stream_of(S.sign(KIND_INVOICE, [(176, pub), (1000000005, b"x")], d)), OK, "span/invoice-high-offer-fields-only")
    raw("lni", stream_of(S.sign(KIND_INVOICE, [(176, pub), (2000000005, b"x")], d)), OK, "span/invoice-high-invreq-fields-only")
    raw("lni", stream_of(S.sign(KIND_INVOICE, [(176, pub), (3000000005, b"x")], d)), OK, "span/invoice-nothing-inside")
    # -- leaf counts
    for leaves in (1, 2, 3, 4, 5, 8, 9, 17):
        f = S.sign(KIND_INVOICE, [(176, pub)] + [(2 * k, S.blob(k % 7)) for k in range(leaves - 1)], d)
        raw("lni", stream_of(f), OK, "leaves/%d" % leaves)
    big = S.sign(KIND_INVOICE, [meta, (10, S.blob(3000)), (176, pub)], d)
    raw("lni", stream_of(big), OK, "long/above-4096")
    assert len(rows[-1][1]) > 4096
    s = rows[-1][1]
    add("long/above-4096-joined", b"+\n ".join(s[k:k + 700] for k in range(0, len(s), 700)), OK)
    return rows


def bases(seed=21, count=24):
    """signed invoice requests and invoices and plain offers of unequal lengths, as strings"""
    S = Signer(seed)
    keys = [S.key() for _ in range(3)]
    out = []
    for i in range(count):
        d, pub = keys[i % 3]
        kind = (KIND_OFFER, KIND_INVREQ, KIND_INVOICE)[i % 3]
        fields = [(0, S.blob(8 + i)), (10, S.blob(S.rnd.randrange(1, 60))), (22, keys[(i + 1) % 3][1])]
        if S.rnd.randrange(2):
            fields.append((1000000000 + i, S.blob(S.rnd.randrange(200))))
        if kind == KIND_OFFER:
            fields = fields[1:]
        else:
            fields.append((88, pub if kind == KIND_INVREQ else keys[(i + 2) % 3][1]))
            if kind == KIND_INVOICE:
                fields += [(164, S.blob(4)), (168, S.blob(32)), (176, pub)]
            fields = S.sign(kind, fields, d)
        out.append(encode(HRP[kind], stream_of(sorted(fields))))
    return out


def random_batch(n, seed, pool=None):
    """a mixed batch drawn from the signed bases: two rows in five are damaged in one character, upper-cased, joined or cut short"""
    pool = pool or bases()
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        s = rnd.choice(pool)
        how = rnd.randrange(10)
        if how == 0:
            k = rnd.randrange(len(s))
            s = s[:k] + bytes([rnd.choice(b"qpzry9x8gf2tvdw0s3jn54khce6mua7l1bQ+ ")]) + s[k + 1:]
        elif how == 1:
            s = s.upper()
        elif how == 2:
            k = rnd.randrange(1, len(s) - 1)
            s = s[:k] + b"+" + rnd.choice([b"", b" ", b"\n  "]) + s[k:]
        elif how == 3:
            s = s[:rnd.randrange(len(s))]
        out.append(s)
    return out

"""How the kernels read the caller's bytes (include/lightning_amd.h): key columns with a stride larger than the key, byte columns that start at
addresses which are not 4-byte aligned, and the double SHA-256 of the device at its padding edges (the 0x80 byte, the length words, the extra block).
The arithmetic is tested elsewhere; here every row set is small and fixed and only its LAYOUT varies -- stride, filling of the gaps, shift of the
buffers, length and start of the hashed strings.  Expected verdicts come from the C oracle and hashlib on the same bytes (recovered keys from
pyref, parsed keys and BOLT #12 verdicts from tests/golden/kat.json), never from the engine; the engine's own packed / aligned call of the same rows
must agree as well.
CPU: the builders and what they promise (classes, residues, alignments, the oracle agreeing with the construction).  GPU: the comparisons."""
import functools
import hashlib
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gossip_stream as gs  # noqa: E402
import pyref  # noqa: E402
from verdict_bytes import strict_bool  # noqa: E402

H = bytes.fromhex
N, P = pyref.N, pyref.P
STRIDES = {33: (34, 36, 64, 97), 65: (66, 68, 128)}
FILLS = ("random", "key", "ff")
SHIFTS = ((1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 2, 3, 1))     # (hash / message, signature, key, outputs); the last one is the mixed case
LEAD = 61        # the key column handed over is the tail of a larger array and starts this far into it
FILL = 0xEE      # what surrounds a shifted output buffer


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def _orc():
    import orc
    orc.lib()
    return orc


def _rows(rows, w):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), w).copy()


def _flip(b, pos, mask):
    return b[:pos] + bytes([b[pos] ^ mask]) + b[pos + 1:]


# ------------------------------------------------------------------------------------------------ builders (CPU)
def _bad_keys(orc, rnd, publen):
    """16 keys that do not parse: off the curve, a prefix the length does not allow, a coordinate >= p"""
    def valid():
        p65 = orc.pubkey_create(rnd.randrange(1, N).to_bytes(32, "big"))
        return p65[1:33], p65[33:65]
    out = []
    if publen == 32:
        while len(out) < 10:                                        # x without a point
            x = rnd.randrange(1, P).to_bytes(32, "big")
            if orc.pubkey_parse(b"\x02" + x) is None:
                out.append(x)
        out += [(P + k).to_bytes(32, "big") for k in range(6)]      # x >= p
    elif publen == 33:
        while len(out) < 6:
            x = rnd.randrange(1, P).to_bytes(32, "big")
            if orc.pubkey_parse(b"\x02" + x) is None:
                out.append(bytes([2 + (len(out) & 1)]) + x)
        out += [bytes([pre]) + valid()[0] for pre in (0x00, 0x01, 0x04, 0x05, 0xFF)]
        out += [bytes([2 + (k & 1)]) + (P + k).to_bytes(32, "big") for k in range(5)]
    else:
        for k in range(5):
            x, y = valid()
            out.append(b"\x04" + x + _flip(y, 31 - k, 1 << k))       # not on the curve
        for pre in (0x00, 0x02, 0x03, 0x05):
            x, y = valid()
            out.append(bytes([pre]) + x + y)
        for k in range(3):                                          # hybrid with the wrong parity byte
            x, y = valid()
            out.append(bytes([7 - (y[31] & 1)]) + x + y)
        for k in range(2):
            out.append(b"\x04" + (P + k).to_bytes(32, "big") + valid()[1])
            out.append(b"\x04" + valid()[0] + (P + k + 1).to_bytes(32, "big"))
    assert len(out) == 16 and all(len(k) == publen for k in out)
    return out


@functools.lru_cache(maxsize=None)
def signed_rows(publen):
    """320 rows under keys of `publen` bytes (33 / 65: ECDSA, 32: BIP-340), in four segments of 64 rows under ONE key, 12 rows under distinct valid
    keys and 4 rows under keys that do not parse; every fourth row damaged after signing (hash bit, s bit, another row's signature).
    -> (hash / msg [n,32], sig [n,64], key [n,publen], cls [n] 0 hot / 1 distinct / 2 bad key, damaged bool [n], the oracle's verdicts uint8 [n])"""
    orc = _orc()
    rnd = random.Random(0xA110 + publen)

    def key():
        d = rnd.randrange(1, N).to_bytes(32, "big")
        p65 = orc.pubkey_create(d)
        return d, (p65 if publen == 65 else (bytes([2 + (p65[64] & 1)]) + p65[1:33] if publen == 33 else p65[1:33]))

    def sign(d):
        m = rnd.randbytes(32)
        if publen == 32:
            return m, orc.schnorr_sign(m, d, rnd.randbytes(32))
        return m, orc.ecdsa_sign(m, d, rnd.randrange(1, N).to_bytes(32, "big"))
    bad = _bad_keys(orc, rnd, publen)
    hs, sg, pk, cls = [], [], [], []
    for seg in range(4):
        hot = key()
        for kind, cnt in ((0, 64), (1, 12), (2, 4)):
            for j in range(cnt):
                d, p = hot if kind == 0 else key()
                if kind == 2:
                    d, p = hot[0], bad[4 * seg + j]        # a good signature of another key: only the key decides
                m, s = sign(d)
                hs.append(m); sg.append(s); pk.append(p); cls.append(kind)
    damaged = np.zeros(len(hs), dtype=bool)
    for i in range(1, len(hs), 4):
        damaged[i] = True
        k = (i // 4) % 3
        if k == 0:
            hs[i] = _flip(hs[i], i % 32, 1 << (i % 8))
        elif k == 1:
            sg[i] = _flip(sg[i], 32 + i % 32, 1 << (i % 8))
        else:
            sg[i] = sg[i - 1]
    hs, sg, pk = _rows(hs, 32), _rows(sg, 64), _rows(pk, publen)
    exp = orc.schnorr_verify_batch(hs, pk, sg, 4) if publen == 32 else orc.ecdsa_verify_batch(hs, sg, pk, publen, 4)
    return hs, sg, pk, np.array(cls), damaged, exp


def _other_key(keys, valid, i):
    """a row of `valid` whose key is not row i's"""
    for t in range(len(valid)):
        j = valid[(7 * i + 3 + t) % len(valid)]
        if not np.array_equal(keys[j], keys[i]):
            return keys[j]
    raise AssertionError("one key only")


def strided_column(keys, stride, fill, valid=None):
    """the keys at `stride` in a buffer of exactly (n - 1) * stride + keylen bytes -- the tail of a larger array, so that it ends where the array ends.
    The gaps hold: "random" bytes (different from row to row, also between rows of one key), "key" the leading bytes of another row's valid key
    (valid: the rows whose keys parse; default all), "ff"."""
    n, L = keys.shape
    valid = np.arange(n) if valid is None else valid
    nbytes = (n - 1) * stride + L
    rng = np.random.default_rng(1000 * stride + L)
    big = rng.integers(0, 256, size=LEAD + nbytes, dtype=np.uint8) if fill == "random" else np.full(LEAD + nbytes, 0xFF, dtype=np.uint8)
    col = big[LEAD:]
    pad = stride - L
    for i in range(n):
        col[i * stride:i * stride + L] = keys[i]
        if i == n - 1:
            break
        gap = col[i * stride + L:(i + 1) * stride]
        if fill == "random":
            gap[0] = (37 * i + 11) & 0xFF                             # neighbours never agree in the first byte behind the key
        elif fill == "key":
            gap[:] = np.resize(_other_key(keys, valid, i), pad)
    assert col.size == nbytes and col.base is big and col.ctypes.data + nbytes == big.ctypes.data + big.size
    return col


@functools.lru_cache(maxsize=None)
def preimage_set():
    """check_tx_sig rows whose preimages take every length 0..200 and a few long ones, laid back to back; signed over hashlib's double SHA-256 under
    one of 5 keys; every fifth row has a preimage byte flipped after signing (first, last, next to a 64-byte boundary); a few sighash types outside
    the gate.  -> (preimages, types uint8 [n], has_witness uint8 [n], sig [n,64], key33 [n,33], construction bool [n], expected bool [n])"""
    orc = _orc()
    rnd = random.Random(0x7E1)
    lens = list(range(201)) + [255, 256, 257, 1000, 4095, 4096, 4097]
    keys = []
    for _ in range(5):
        d = rnd.randrange(1, N).to_bytes(32, "big")
        keys.append((d, gs.Net.compress(orc.pubkey_create(d))))
    pre, types, wit, sg, pk, cons, exp = [], [], [], [], [], [], []
    for i, ln in enumerate(lens):
        m = rnd.randbytes(ln)
        d, p = keys[i % 5]
        s = orc.ecdsa_sign(sha256d(m), d, rnd.randrange(1, N).to_bytes(32, "big"))
        t, w, good = 1, i & 1, True
        if i % 5 == 3:
            cands = [q for q in (0, ln - 1, 63, 64, 127, 128, 191, 192, ln - 64) if 0 <= q < ln]
            m = _flip(m, cands[(i // 5) % len(cands)], 1 << (i % 8))
            good = False
        if i % 23 == 7:
            t, good = (2, 3, 0x81, 0x82, 0)[(i // 23) % 5], False        # outside the gate: refused whatever the signature
        elif i % 29 == 11:
            t, w = 0x83, 1                                                # SINGLE|ANYONECANPAY with a witness script passes the gate
        elif i % 31 == 13:
            t, w, good = 0x83, 0, False                                   # ... and without one does not
        gate = t == 1 or (t == 0x83 and w == 1)
        pre.append(m); types.append(t); wit.append(w); sg.append(s); pk.append(p); cons.append(good)
        exp.append(bool(gate and orc.ecdsa_verify(sha256d(m), s, p)))
    return pre, np.array(types, dtype=np.uint8), np.array(wit, dtype=np.uint8), _rows(sg, 64), _rows(pk, 33), np.array(cons), np.array(exp)


@functools.lru_cache(maxsize=None)
def gossip_set():
    """gossip_stream.padding_edge_messages, a fifth of them damaged (a signature bit, or a byte of the signed tail next to a 64-byte block boundary
    or at its end), back to back.  -> dict(msgs, ids (per message or None), tails (signed-tail lengths), damaged, blob, off, idarr [n,33], rowbase,
    expect int8 [n]: the oracle's verdict per message)"""
    orc = _orc()
    net = gs.Net(orc, 0x6055)
    rnd = random.Random(0x51DE)
    msgs, ids, tails, damaged = [], [], [], []
    for i, (m, nid, tl) in enumerate(gs.padding_edge_messages(net)):
        dmg = i % 5 == 2
        if dmg and (i // 5) % 2 == 0:
            m = gs.damage(rnd, m, "sig")
        elif dmg:
            so = len(m) - tl
            if m[:2] == b"\x01\x00":       # channel_announcement: stay inside features | chain_hash | short_channel_id (the keys behind them decide other verdicts)
                end = 2 + int.from_bytes(m[so:so + 2], "big") + 40
                cands = [q for q in (63, 64, 127, 128) if 2 <= q < end] or [end - 35]
            else:                          # node_announcement: not the two length fields (0, 1 and 74, 75) nor the node id; channel_update: any byte
                cands = [q for q in (63, 64, 127, 128, 191, 192, tl - 1) if q < tl and not (m[:2] == b"\x01\x01" and q in (74, 75))]
            m = _flip(m, so + cands[(i // 10) % len(cands)], 0x10)
        msgs.append(m); ids.append(nid); tails.append(tl); damaged.append(dmg)
    exp = [orc.sigcheck_channel_announcement(m) if m[:2] == b"\x01\x00" else orc.sigcheck_node_announcement(m) if m[:2] == b"\x01\x01"
           else orc.sigcheck_channel_update(m, nid) for m, nid in zip(msgs, ids)]
    n = len(msgs)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    rowbase = np.zeros(n + 1, dtype=np.uint64)
    rowbase[1:] = np.cumsum([4 if m[:2] == b"\x01\x00" else 1 for m in msgs])
    idarr = np.zeros((n, 33), dtype=np.uint8)
    for i, k in enumerate(ids):
        if k is not None:
            idarr[i] = np.frombuffer(k, dtype=np.uint8)
    return dict(msgs=msgs, ids=ids, tails=np.array(tails), damaged=np.array(damaged), blob=np.frombuffer(b"".join(msgs), dtype=np.uint8).copy(), off=off,
                idarr=idarr, rowbase=rowbase, expect=np.array(exp, dtype=np.int8))


@functools.lru_cache(maxsize=None)
def template_set():
    """40 check_tx_sig rows as transaction templates (lamd_check_tx_sig_tx_batch) under 4 keys, every fourth damaged after signing
    -> (txs, sig [n,64], key33 [n,33], expected bool [n]: the gate and the oracle on pyref's BIP143 hash)"""
    orc = _orc()
    rnd = random.Random(0x7A7)
    keys = []
    for _ in range(4):
        d = rnd.randrange(1, N).to_bytes(32, "big")
        keys.append((d, gs.Net.compress(orc.pubkey_create(d))))
    txs, sg, pk, exp = [], [], [], []
    for i in range(40):
        n_in, n_out = (1, 1, 2, 4)[i % 4], (1, 2, 3)[i % 3]
        inputs = [(rnd.randbytes(32), rnd.randrange(1 << 32), rnd.randrange(1 << 32)) for _ in range(n_in)]
        outputs = [(rnd.randrange(1 << 40), rnd.randbytes((22, 34, 43)[(i + j) % 3])) for j in range(n_out)]
        t = dict(version=2, locktime=rnd.randrange(1 << 32), inputs=inputs, outputs=outputs, input_num=i % n_in, amount=rnd.randrange(1 << 44),
                 script=rnd.randbytes((25, 71, 133, 260)[i % 4]), sighash_type=0x83 if i % 7 == 3 else 1, has_witness=True)
        d, p = keys[(i // 3) % 4]                         # neighbouring rows share their key
        s = orc.ecdsa_sign(pyref.bip143_sighash(2, inputs, outputs, t["locktime"], t["input_num"], t["script"], t["amount"], t["sighash_type"])[0], d,
                           rnd.randrange(1, N).to_bytes(32, "big"))
        if i % 4 == 2:
            k = (i // 4) % 3
            if k == 0:
                t["amount"] ^= 1
            elif k == 1:
                t["script"] = _flip(t["script"], len(t["script"]) - 1, 4)
            else:
                t["sighash_type"] = 2
        h = pyref.bip143_sighash(2, t["inputs"], t["outputs"], t["locktime"], t["input_num"], t["script"], t["amount"], t["sighash_type"])[0]
        gate = t["sighash_type"] == 1 or (t["sighash_type"] == 0x83 and t["has_witness"])
        txs.append(t); sg.append(s); pk.append(p); exp.append(bool(gate and orc.ecdsa_verify(h, s, p)))
    return txs, _rows(sg, 64), _rows(pk, 33), np.array(exp)


# ------------------------------------------------------------------------------------------------ what the builders promise (CPU)
@pytest.mark.parametrize("publen", [33, 65, 32])
def test_signed_rows_hold_every_class_and_the_oracle_agrees_with_the_construction(publen):
    hs, sg, pk, cls, damaged, exp = signed_rows(publen)
    n = len(exp)
    assert n == 320 and [(cls == k).sum() for k in range(3)] == [256, 48, 16] and damaged.sum() == 80
    assert np.array_equal(exp.astype(bool), (cls != 2) & ~damaged)
    assert exp.sum() >= n // 2 and (exp == 0).sum() >= n // 10
    keys = [pk[i].tobytes() for i in range(n)]
    assert len(set(k for k, c in zip(keys, cls) if c == 0)) == 4 and len(set(k for k, c in zip(keys, cls) if c == 1)) == 48
    assert len(set(k for k, c in zip(keys, cls) if c == 2)) == 16
    orc = _orc()
    for k, c in zip(keys, cls):       # a bad key is bad by itself, whatever is signed under it
        parsed = orc.pubkey_parse(b"\x02" + k if publen == 32 else k)
        assert (parsed is None) == (c == 2)
    assert any(keys[i] == keys[i - 1] for i in range(1, n)) and any(keys[i] != keys[i - 1] for i in range(1, n))


@pytest.mark.parametrize("publen,stride", [(L, s) for L in (33, 65) for s in STRIDES[L]] + [(32, 33), (32, 40)])
def test_a_strided_column_is_the_tail_of_its_array_and_differs_from_the_packed_one(publen, stride):
    keys, valid = signed_rows(publen)[2], np.nonzero(signed_rows(publen)[3] != 2)[0]
    n = keys.shape[0]
    for fill in FILLS:
        col = strided_column(keys, stride, fill, valid)
        assert col.size == (n - 1) * stride + publen
        assert all(np.array_equal(col[i * stride:i * stride + publen], keys[i]) for i in range(n))
        # read with the wrong pitch (keylen for stride) the column gives other keys from row 1 on, and the gaps are not all alike
        assert not np.array_equal(col[publen:2 * publen], keys[1])
        gaps = [col[i * stride + publen:(i + 1) * stride].tobytes() for i in range(n - 1)]
        if fill == "random":
            assert all(gaps[i][0] != gaps[i + 1][0] for i in range(n - 2))
        elif fill == "key":
            for i, g in enumerate(gaps):      # the start of a key that parses and is not this row's
                assert any(np.resize(keys[j], stride - publen).tobytes() == g and not np.array_equal(keys[j], keys[i]) for j in valid)
        else:
            assert set(b"".join(gaps)) == {0xFF}


def _residues_covered(lengths):
    cnt = np.bincount(np.asarray(lengths) % 64, minlength=64)
    return cnt.min() >= 2 and all(cnt[r] >= 1 for r in (55, 56, 63, 0))


def test_preimages_cover_every_padding_residue_and_alignment():
    pre, types, wit, sg, pk, cons, exp = preimage_set()
    lens = [len(m) for m in pre]
    assert _residues_covered(lens) and {0, 55, 56, 63, 64, 119, 120, 127, 128, 4095, 4096, 4097} <= set(lens)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert set(starts % 4) == {0, 1, 2, 3}
    assert np.array_equal(cons, exp)                       # the oracle on hashlib's hash agrees with the construction
    assert exp.sum() >= len(exp) // 2 and (~exp).sum() >= len(exp) // 10
    assert set(types) >= {1, 0x83, 2, 0x81} and len(set(pk[i].tobytes() for i in range(len(pre)))) == 5


def test_gossip_tails_cover_every_padding_residue_and_alignment():
    g = gossip_set()
    n = len(g["msgs"])
    kinds = [m[:2] for m in g["msgs"]]
    assert kinds.count(b"\x01\x01") == 131 and kinds.count(b"\x01\x00") == 67 and kinds.count(b"\x01\x02") == 12
    for kind in (b"\x01\x01", b"\x01\x00"):               # each builder by itself, and the updates at the four edges
        own = g["tails"][[k == kind for k in kinds]]
        assert (np.bincount(own % 64, minlength=64).min() >= 2 if kind == b"\x01\x01" else len(set(own % 64)) == 64)
        assert {55, 56, 63, 0} <= set(own % 64)
    assert {55, 56, 63, 0} <= set(g["tails"][[k == b"\x01\x02" for k in kinds]] % 64)
    assert _residues_covered(g["tails"])
    assert set(g["off"][:-1] % 4) == {0, 1, 2, 3}
    assert all(len(m) - t == (258 if m[:2] == b"\x01\x00" else 66) for m, t in zip(g["msgs"], g["tails"]))
    # the oracle agrees with the construction: untouched messages verify, damaged ones do not
    assert np.array_equal(g["expect"] == 0, ~g["damaged"])
    assert (g["expect"] == 0).sum() >= n // 2 and (g["expect"] != 0).sum() >= n // 10
    assert g["damaged"][[k == b"\x01\x00" for k in kinds]].any() and g["damaged"][[k == b"\x01\x02" for k in kinds]].any()


def test_templates_hold_passing_and_failing_rows():
    txs, sg, pk, exp = template_set()
    assert len(txs) == 40 and exp.sum() == 30 and any(pk[i].tobytes() == pk[i - 1].tobytes() for i in range(1, 40))


# ------------------------------------------------------------------------------------------------ engines and calls (GPU)
def _engine(**env):
    """an engine created under `env`; the environment is set around Engine(0) only"""
    from lightning_amd import Engine
    os.environ.update(env)
    try:
        return Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module", params=[7, 10])
def eng_keyed(request):
    """the keyed path whenever a key repeats at all, both comb shapes; keyed_mode > 0 also keeps host calls of more than 64 rows off the latency path"""
    e = _engine(LAMD_KEYED="1", LAMD_KEYED_TEETH=str(request.param))
    e.teeth = request.param
    yield e
    e.close()


@pytest.fixture
def eng_unfused():
    """the unfused front end, for the one test that uses it: closed when that test ends, so that it never lives beside a keyed engine"""
    e = _engine(LAMD_KEYED="1", LAMD_FUSED_FRONT="0")
    yield e
    e.close()


def _err(e):
    return e._lib.lamd_last_error(e._ctx)


def host_ecdsa(e, hs, sg, col, publen, stride):
    n = hs.shape[0]
    ok = np.full(n, 9, dtype=np.uint8)
    rc = e._lib.lamd_verify_ecdsa_batch(e._ctx, n, hs.ctypes.data, sg.ctypes.data, col.ctypes.data, publen, stride, ok.ctypes.data)
    assert rc == 0, (rc, _err(e))
    return ok


def _dev(a, shift=0):
    """the bytes of `a` in device memory, `shift` bytes into an allocation filled with FILL -> (allocation, view of the bytes)"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    d = torch.full((flat.size + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    assert d.data_ptr() % 8 == 0
    v = d[shift:shift + flat.size]
    v.copy_(torch.from_numpy(flat))
    return d, v


def _dev_out(nbytes, shift=0):
    import torch
    d = torch.full((nbytes + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    assert d.data_ptr() % 8 == 0
    return d, d[shift:shift + nbytes]


def _out(d, v, shift):
    """the bytes written into view v of allocation d; the bytes around it must still hold FILL"""
    h = d.cpu().numpy()
    n = v.numel()
    assert (h[:shift] == FILL).all() and (h[shift + n:] == FILL).all()
    return h[shift:shift + n].copy()


def dev_ecdsa(e, hs, sg, key_bytes, publen, stride, shifts=(0, 0, 0, 0)):
    """lamd_verify_ecdsa_batch_device; key_bytes: the key column as it lies (packed or strided)"""
    import torch
    n = hs.shape[0]
    (_, dh), (_, ds), (_, dk) = _dev(hs, shifts[0]), _dev(sg, shifts[1]), _dev(key_bytes, shifts[2])
    do, vo = _dev_out(n, shifts[3])
    torch.cuda.synchronize()
    rc = e._lib.lamd_verify_ecdsa_batch_device(e._ctx, n, dh.data_ptr(), ds.data_ptr(), dk.data_ptr(), publen, stride, vo.data_ptr())
    assert rc == 0, (rc, _err(e))
    e.synchronize()
    return _out(do, vo, shifts[3])


def dev_schnorr(e, ms, sg, ks, shifts=(0, 0, 0, 0)):
    import torch
    n = ms.shape[0]
    (_, dm), (_, ds), (_, dk) = _dev(ms, shifts[0]), _dev(sg, shifts[1]), _dev(ks, shifts[2])
    do, vo = _dev_out(n, shifts[3])
    torch.cuda.synchronize()
    rc = e._lib.lamd_verify_schnorr_batch_device(e._ctx, n, dm.data_ptr(), dk.data_ptr(), ds.data_ptr(), vo.data_ptr())
    assert rc == 0, (rc, _err(e))
    e.synchronize()
    return _out(do, vo, shifts[3])


def _counters(e):
    inf = e.info()
    return {k: inf[k] for k in ("last_unique_keys", "last_new_tables", "last_cache_hits")}


# ------------------------------------------------------------------------------------------------ A. strided keys
def _strided_vs_packed(e, publen, stride, device_too):
    hs, sg, pk, cls, damaged, exp = signed_rows(publen)
    packed = host_ecdsa(e, hs, sg, pk, publen, publen)
    assert np.array_equal(packed, exp), np.nonzero(packed != exp)[0][:10]
    valid = np.nonzero(cls != 2)[0]
    for fill in FILLS:
        col = strided_column(pk, stride, fill, valid)
        got = host_ecdsa(e, hs, sg, col, publen, stride)
        assert np.array_equal(got, exp), (fill, np.nonzero(got != exp)[0][:10])
        if device_too:
            got = dev_ecdsa(e, hs, sg, col, publen, stride)
            assert np.array_equal(got, exp), (fill, "device", np.nonzero(got != exp)[0][:10])
    return hs, sg, pk, exp


@pytest.mark.gpu
def test_strided_keys_unfused_front_end(eng_unfused):
    """the 19-launch front end (k_dedupe_insert, k_keys, k_cache_publish) reads keys at the stride"""
    for publen, stride in ((33, 36), (65, 66)):
        _strided_vs_packed(eng_unfused, publen, stride, device_too=False)
        assert eng_unfused.info()["last_keyed"]


@pytest.mark.gpu
@pytest.mark.parametrize("publen,stride", [(L, s) for L in (33, 65) for s in STRIDES[L]])
def test_strided_keys_latency_path(eng, publen, stride):
    """the default engine, host API, <= 4096 rows: run_small's repack, fingerprints and neighbour compare -- and, from a key's second sight on, the
    learning call down the general path"""
    _strided_vs_packed(eng, publen, stride, device_too=True)


@pytest.mark.gpu
@pytest.mark.parametrize("publen,stride", [(L, s) for L in (33, 65) for s in STRIDES[L]])
def test_strided_keys_general_path_and_its_counters(eng_keyed, publen, stride):
    """keyed engines: tables for the four hot keys, the ladder for the distinct ones, k_keys_cold's reject for the bad ones; host and device API.  A kernel
    that hashed or compared `stride` bytes of a key would count other unique keys, build other tables and miss the cache: the packed call of the same
    rows is the reference for the counters"""
    e = eng_keyed
    hs, sg, pk, exp = _strided_vs_packed(e, publen, stride, device_too=True)
    assert e.info()["last_keyed"] == e.teeth
    for fill in FILLS:
        col = strided_column(pk, stride, fill, np.nonzero(signed_rows(publen)[3] != 2)[0])
        seq = {}
        for name, keys, pitch in (("packed", pk, publen), ("strided", col, stride)):
            e.cache_clear()
            first = host_ecdsa(e, hs, sg, keys, publen, pitch)
            c1 = _counters(e)
            second = host_ecdsa(e, hs, sg, keys, publen, pitch)
            c2 = _counters(e)
            assert np.array_equal(first, exp) and np.array_equal(second, exp), (fill, name)
            seq[name] = (c1, c2)
        (p1, p2), (s1, s2) = seq["packed"], seq["strided"]
        assert s1["last_unique_keys"] == p1["last_unique_keys"] > 0 and s1["last_new_tables"] == p1["last_new_tables"] > 0, (fill, p1, s1)
        assert s1["last_cache_hits"] == p1["last_cache_hits"] == 0, (fill, p1, s1)
        assert s2["last_cache_hits"] == p2["last_cache_hits"] > 0 and s2["last_new_tables"] == p2["last_new_tables"], (fill, p2, s2)


def _tx_sig_strided(e):
    pre, types, wit, sg, pk, cons, exp = preimage_set()
    assert np.array_equal(e.check_tx_sig_batch(pre, types, wit, sg, pk), exp)
    for fill in ("random", "key"):
        got = e.check_tx_sig_batch(pre, types, wit, sg, strided_column(pk, 36, fill), key_layout=(33, 36))
        assert np.array_equal(got, exp), (fill, np.nonzero(got != exp)[0][:10])


@pytest.mark.gpu
def test_strided_keys_check_tx_sig_batch(eng):
    _tx_sig_strided(eng)          # hashed on the host, the rows through the latency path


@pytest.mark.gpu
def test_strided_keys_check_tx_sig_batch_general_path(eng_keyed):
    _tx_sig_strided(eng_keyed)    # k_txsig_hash, then the batch machinery


def _tx_templates_strided(e, rows):
    txs, sg, pk, exp = template_set()
    txs, sg, pk, exp = txs[:rows], sg[:rows], pk[:rows], exp[:rows]
    assert np.array_equal(e.check_tx_sig_tx_batch(txs, sg, pk), exp)
    for fill in ("random", "key"):
        got = e.check_tx_sig_tx_batch(txs, sg, strided_column(pk, 64, fill), key_layout=(33, 64))
        assert np.array_equal(got, exp), (rows, fill, np.nonzero(got != exp)[0][:10])


@pytest.mark.gpu
def test_strided_keys_check_tx_sig_tx_batch(eng):
    _tx_templates_strided(eng, 12)     # <= 16 rows: BIP143 on the host, one launch
    _tx_templates_strided(eng, 40)     # 17..4096 rows: k_txsig_tx_hash in front of the latency kernel


@pytest.mark.gpu
def test_strided_keys_check_tx_sig_tx_batch_general_path(eng_keyed):
    _tx_templates_strided(eng_keyed, 40)


@pytest.mark.gpu
def test_strided_keys_streaming_queue(eng):
    """lamd_queue_ecdsa_batch packs a strided column into the staging set row by row"""
    for publen, stride in ((33, 64), (65, 68)):
        hs, sg, pk, cls, damaged, exp = signed_rows(publen)
        col = strided_column(pk, stride, "key")
        first = eng._lib.lamd_queue_ecdsa_batch(eng._ctx, len(exp), hs.ctypes.data, sg.ctypes.data, col.ctypes.data, publen, stride)
        assert first == 0, (first, _err(eng))
        eng.flush()
        got = eng.wait()
        assert np.array_equal(got, exp.astype(bool)), np.nonzero(got != exp.astype(bool))[0][:10]


@pytest.mark.gpu
def test_strided_keys_bolt12(eng, eng_keyed, kat):
    """keystride 48: the reference-held invoices and invoice_requests with their damaged twins (kat.json "bolt12")"""
    for e in (eng, eng_keyed):
        for mn in (b"invoice", b"invoice_request"):
            grp = [v for v in kat["bolt12"] if v["messagename"].encode() == mn]
            exp = [v["expect"] for v in grp]
            assert any(exp) and not all(exp)
            streams, sg, pk = [H(v["stream"]) for v in grp], _rows([H(v["sig"]) for v in grp], 64), _rows([H(v["key"]) for v in grp], 33)
            assert [bool(g) for g in e.bolt12_check_signature_batch(streams, mn, b"signature", pk, sg)] == exp
            for fill in ("random", "ff"):
                got = e.bolt12_check_signature_batch(streams, mn, b"signature", strided_column(pk, 48, fill), sg, keystride=48)
                assert [bool(g) for g in got] == exp, (mn, fill)


def _parse(e, col, n, publen, stride):
    out, ok = np.full((n, 64), FILL, dtype=np.uint8), np.full(n, 9, dtype=np.uint8)
    rc = e._lib.lamd_pubkey_parse_batch(e._ctx, n, col.ctypes.data, publen, stride, out.ctypes.data, ok.ctypes.data)
    assert rc == 0, (rc, _err(e))
    return out, ok


@pytest.mark.gpu
def test_strided_keys_pubkey_parse(eng, kat, orc):
    for publen, stride in ((33, 36), (65, 68)):
        vs = [v for v in kat["pubkey"] if len(v["pub"]) == 2 * publen]
        assert any(v["expect"] is None for v in vs) and any(v["expect"] is not None for v in vs)
        pk = _rows([H(v["pub"]) for v in vs], publen)
        for fill in ("random", "ff"):
            out, ok = _parse(eng, strided_column(pk, stride, fill), len(vs), publen, stride)
            for v, o, k in zip(vs, out, ok):
                assert k == (v["expect"] is not None), v["pub"]
                assert not k or o.tobytes() == H(v["expect"]), v["pub"]
    xs = signed_rows(32)[2]                                   # x-only keys, lifted to even y: the oracle parses 02 || x
    want = [orc.pubkey_parse(b"\x02" + xs[i].tobytes()) for i in range(len(xs))]
    for stride in (32, 33, 40):
        for fill in FILLS if stride > 32 else ("ff",):
            out, ok = _parse(eng, strided_column(xs, stride, fill, np.nonzero(signed_rows(32)[3] != 2)[0]) if stride > 32 else xs, len(xs), 32, stride)
            assert strict_bool(ok).tolist() == [w is not None for w in want], (stride, fill)
            assert all(o.tobytes() == w for o, w in zip(out, want) if w is not None), (stride, fill)


@pytest.mark.gpu
def test_a_stride_shorter_than_the_key_is_refused_everywhere(eng, kat):
    from lightning_amd.engine import LamdError
    L, c = eng._lib, eng._ctx
    for publen in (33, 65):
        hs, sg, pk, cls, damaged, exp = signed_rows(publen)
        n, ok = 8, np.full(8, 9, dtype=np.uint8)
        bad = publen - 1
        assert L.lamd_verify_ecdsa_batch(c, n, hs.ctypes.data, sg.ctypes.data, pk.ctypes.data, publen, bad, ok.ctypes.data) == -3
        (_, dh), (_, ds), (_, dk), (do, vo) = _dev(hs[:n]), _dev(sg[:n]), _dev(pk[:n]), _dev_out(n)
        assert L.lamd_verify_ecdsa_batch_device(c, n, dh.data_ptr(), ds.data_ptr(), dk.data_ptr(), publen, bad, vo.data_ptr()) == -3
        assert L.lamd_pubkey_parse_batch(c, n, pk.ctypes.data, publen, bad, None, ok.ctypes.data) == -3
        assert L.lamd_queue_ecdsa_batch(c, n, hs.ctypes.data, sg.ctypes.data, pk.ctypes.data, publen, bad) == -3
        assert (ok == 9).all() and (_out(do, vo, 0) == FILL).all()
    assert L.lamd_pubkey_parse_batch(c, 4, signed_rows(32)[2].ctypes.data, 32, 31, None, ok.ctypes.data) == -3
    flat33 = np.ascontiguousarray(signed_rows(33)[2]).reshape(-1)
    pre, types, wit, sg, pk, cons, exp = preimage_set()
    with pytest.raises(LamdError, match="bad argument"):
        eng.check_tx_sig_batch(pre[:8], types[:8], wit[:8], sg[:8], flat33, key_layout=(33, 32))
    txs, sg, pk, exp = template_set()
    with pytest.raises(LamdError, match="bad argument"):
        eng.check_tx_sig_tx_batch(txs[:8], sg[:8], flat33, key_layout=(33, 32))
    grp = [v for v in kat["bolt12"] if v["messagename"] == "invoice"][:4]
    with pytest.raises(LamdError, match="bad argument"):
        eng.bolt12_check_signature_batch([H(v["stream"]) for v in grp], b"invoice", b"signature", flat33, _rows([H(v["sig"]) for v in grp], 64), keystride=32)
    hs, sg, pk, cls, damaged, exp = signed_rows(33)          # nothing was queued by the refused calls: the next ticket is 0
    assert L.lamd_queue_ecdsa_batch(c, 8, hs.ctypes.data, sg.ctypes.data, pk.ctypes.data, 33, 33) == 0
    eng.flush()
    assert np.array_equal(eng.wait(), exp[:8].astype(bool))


# ------------------------------------------------------------------------------------------------ B. unaligned device buffers
def _unaligned_verify(e):
    for publen in (33, 65):
        hs, sg, pk, cls, damaged, exp = signed_rows(publen)
        aligned = dev_ecdsa(e, hs, sg, pk, publen, publen)
        assert np.array_equal(aligned, exp)
        for sh in SHIFTS:
            got = dev_ecdsa(e, hs, sg, pk, publen, publen, sh)
            assert np.array_equal(got, exp), (publen, sh, np.nonzero(got != exp)[0][:10])
    ms, sg, ks, cls, damaged, exp = signed_rows(32)
    assert np.array_equal(dev_schnorr(e, ms, sg, ks), exp)
    for sh in SHIFTS:
        got = dev_schnorr(e, ms, sg, ks, sh)
        assert np.array_equal(got, exp), (sh, np.nonzero(got != exp)[0][:10])


@pytest.mark.gpu
def test_unaligned_device_columns_verify(eng):
    _unaligned_verify(eng)


@pytest.mark.gpu
def test_unaligned_device_columns_verify_keyed(eng_keyed):
    _unaligned_verify(eng_keyed)


@functools.lru_cache(maxsize=None)
def recover_rows():
    """kat.json "recover" -> (hash [n,32], sig [n,64], recid uint8 [n], keys [n,33] (zero where there is none), ok uint8 [n]) by pyref.ecdsa_recover"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "kat.json")) as f:
        rows = json.load(f)["recover"]
    hs, sg = _rows([H(v["hash"]) for v in rows], 32), _rows([H(v["sig"]) for v in rows], 64)
    rid = np.array([v["recid"] & 0xFF for v in rows], dtype=np.uint8)
    keys, ok = np.zeros((len(rows), 33), dtype=np.uint8), np.zeros(len(rows), dtype=np.uint8)
    for i, v in enumerate(rows):
        q = pyref.ecdsa_recover(hs[i].tobytes(), sg[i].tobytes(), int(rid[i]))
        assert (pyref.ser33(q).hex() if q else None) == v["expect"], v["name"]
        if q:
            keys[i], ok[i] = np.frombuffer(pyref.ser33(q), dtype=np.uint8), 1
    return hs, sg, rid, keys, ok


def test_recover_rows_hold_keys_and_failures():
    hs, sg, rid, keys, ok = recover_rows()
    assert ok.sum() >= len(ok) // 2 and (ok == 0).sum() >= 4 and set(rid) >= {0, 1, 2, 3}


def _unaligned_recover(e):
    import torch
    hs, sg, rid, keys, ok = recover_rows()
    n = len(ok)
    for sh in ((0, 0, 0, 0),) + SHIFTS:
        (_, dh), (_, ds), (_, dr) = _dev(hs, sh[0]), _dev(sg, sh[1]), _dev(rid, sh[2])
        (dk, vk), (do, vo) = _dev_out(33 * n, sh[2]), _dev_out(n, sh[3])
        torch.cuda.synchronize()
        rc = e._lib.lamd_ecdsa_recover_batch_device(e._ctx, n, dh.data_ptr(), ds.data_ptr(), dr.data_ptr(), vk.data_ptr(), vo.data_ptr())
        assert rc == 0, (rc, _err(e))
        e.synchronize()
        assert np.array_equal(_out(do, vo, sh[3]), ok), sh
        assert np.array_equal(_out(dk, vk, sh[2]).reshape(n, 33), keys), sh


@pytest.mark.gpu
def test_unaligned_device_columns_recover(eng):
    _unaligned_recover(eng)


@pytest.mark.gpu
def test_unaligned_device_columns_recover_keyed(eng_keyed):
    _unaligned_recover(eng_keyed)


def _gossip_device(e, shift, spans):
    """the messages of gossip_set through lamd_sigcheck_gossip_batch_device, or -- in reverse order -- through the spans call; blob, node ids and verdicts
    `shift` bytes into their allocations (the uint64 arrays stay aligned, as the header asks)"""
    import torch
    g = gossip_set()
    n = len(g["msgs"])
    order = np.arange(n)[::-1].copy() if spans else np.arange(n)
    (_, db), (_, di) = _dev(g["blob"], shift), _dev(g["idarr"][order], shift)
    dv, vv = _dev_out(n, shift)
    rows_per = (g["rowbase"][1:] - g["rowbase"][:-1])[order]
    rowbase = np.concatenate([[0], np.cumsum(rows_per)]).astype(np.uint64)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
    d_rb = i64(rowbase)
    torch.cuda.synchronize()
    if spans:
        d_start, d_len = i64(g["off"][:-1][order]), i64((g["off"][1:] - g["off"][:-1])[order])
        rc = e._lib.lamd_sigcheck_gossip_spans_device(e._ctx, n, db.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), di.data_ptr(), d_rb.data_ptr(),
                                                      int(rowbase[-1]), vv.data_ptr())
    else:
        d_off = i64(g["off"])
        rc = e._lib.lamd_sigcheck_gossip_batch_device(e._ctx, n, db.data_ptr(), d_off.data_ptr(), di.data_ptr(), d_rb.data_ptr(), int(rowbase[-1]), vv.data_ptr())
    assert rc == 0, (rc, _err(e))
    e.synchronize()
    got = _out(dv, vv, shift).view(np.int8)
    want = g["expect"][order]
    assert np.array_equal(got, want), (shift, spans, np.nonzero(got != want)[0][:10])


@pytest.mark.gpu
def test_unaligned_device_gossip(eng):
    for shift in (1, 2, 3):
        _gossip_device(eng, shift, spans=False)
        _gossip_device(eng, shift, spans=True)


@pytest.mark.gpu
def test_unaligned_device_gossip_keyed(eng_keyed):
    for shift in (1, 2, 3):
        _gossip_device(eng_keyed, shift, spans=False)
        _gossip_device(eng_keyed, shift, spans=True)


# ------------------------------------------------------------------------------------------------ C. device double SHA-256 at the padding edges
@pytest.mark.gpu
def test_device_sha256d_of_preimages_at_every_padding_edge(eng_keyed):
    """k_txsig_hash (the keyed engines keep a 208-row call off the host-hashing latency path): every length 0..200 and the long ones, every start alignment"""
    pre, types, wit, sg, pk, cons, exp = preimage_set()
    got = eng_keyed.check_tx_sig_batch(pre, types, wit, sg, pk)
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), [(int(i), len(pre[i]), int(types[i])) for i in bad[:10]]
    assert eng_keyed.info()["last_keyed"] == eng_keyed.teeth


@pytest.mark.gpu
def test_host_sha256d_of_preimages_on_the_latency_path(eng):
    pre, types, wit, sg, pk, cons, exp = preimage_set()
    assert np.array_equal(eng.check_tx_sig_batch(pre, types, wit, sg, pk), exp)


def _gossip_all_forms(e):
    g = gossip_set()
    _gossip_device(e, 0, spans=False)
    _gossip_device(e, 0, spans=True)
    got = e.sigcheck_gossip(g["msgs"], g["ids"])
    bad = np.nonzero(got != g["expect"])[0]
    assert not len(bad), [(int(i), int(g["tails"][i]), int(got[i]), int(g["expect"][i])) for i in bad[:10]]


@pytest.mark.gpu
def test_device_sha256d_of_gossip_tails_at_every_padding_edge(eng):
    _gossip_all_forms(eng)


@pytest.mark.gpu
def test_device_sha256d_of_gossip_tails_at_every_padding_edge_keyed(eng_keyed):
    """... and the host call of a keyed engine, which hashes in k_gossip_expand as well"""
    _gossip_all_forms(eng_keyed)

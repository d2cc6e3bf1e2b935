"""The audit of a gossip_store FILE (lamd_gossip_store_frame / lamd_gossip_store_audit, include/lightning_amd.h): the walk over the records
as common/gossmap.c map_catchup() does it, the CRC-32C of every live record, the look-up of every channel_update's signer in the store
itself, all signatures, and the record-level verdicts -- against a Python model of the same rules written here (signatures by the C
oracle), on the two stores the reference's own gossipd wrote (tests/golden/gossip_store_*.bin) and on a synthetic store with deleted
records, tombstones, dying records and every kind of damage the verdict table names.
CPU: the walk, the model's preconditions.  GPU: the device verdicts, record for record."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gossip_stream as gs  # noqa: E402

OK, MALFORMED, BAD_CHECKSUM, NO_CHANNEL, UNKNOWN_TYPE, REDUNDANT, DELETED = 0, -1, -2, -3, -4, -5, 8
KNOWN = (256, 257, 258, 4101, 4103, 4105, 4106, 4107)
F_DELETED, F_COMPLETED = 0x8000, 0x2000
G33 = bytes.fromhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798")   # any valid key: stands in where no signer exists

_T = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _T.append(_c)


def crc32c(seed, data):
    """ccan/crc32c's crc32c(seed, data, len), byte at a time over the table the bitwise definition gives"""
    c = seed ^ 0xFFFFFFFF
    for b in data:
        c = _T[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def walk(blob):
    """map_catchup's walk as the header of lamd_gossip_store_audit states it -> (records [(off, flags, crc, ts, msg)], end_reason, end_offset)"""
    assert len(blob) >= 1 and not blob[0] & 0xE0
    recs, off, why = [], 1, "eof"
    while True:
        if len(blob) - off < 12:
            if off != len(blob):
                why = "partial_header"
            break
        flags, ln, crc, ts = struct.unpack(">HHII", blob[off:off + 12])
        if not flags & F_COMPLETED:
            why = "incomplete"
            break
        if off + 12 + ln > len(blob):
            why = "truncated"
            break
        msg = blob[off + 12:off + 12 + ln]
        if not flags & F_DELETED:
            if ln < 2:
                why = "short"
                break
            if msg[:2] == b"\x01\x00" and len(blob) - (off + 12 + ln) < 12 + 2 + 8:
                why = "no_amount"
                break
        recs.append((off, flags, crc, ts, bytes(msg)))
        off += 12 + ln
        if not flags & F_DELETED and msg[:2] == b"\x10\x09":
            why = "store_ended"
            break
    return recs, why, off


def _cann_scid(m):
    """(scid, offset of node_id_1) of a channel_announcement long enough to hold its scid, else None"""
    if len(m) < 260 or m[:2] != b"\x01\x00":
        return None
    so = 260 + int.from_bytes(m[258:260], "big") + 32
    if len(m) < so + 8:
        return None
    return int.from_bytes(m[so:so + 8], "big"), so + 8


def model(orc, blob):
    """the audit, record by record, by the verdict table of include/lightning_amd.h -> (offsets, verdicts, summary)"""
    recs, why, end = walk(blob)
    first = {}                                            # scid -> lowest index of a LIVE channel_announcement
    for i, (_, flags, _, _, m) in enumerate(recs):
        if not flags & F_DELETED and _cann_scid(m):
            first.setdefault(_cann_scid(m)[0], i)
    out, sigs = [], 0
    for i, (_, flags, crc, ts, m) in enumerate(recs):
        if flags & F_DELETED:
            out.append(DELETED)
            continue
        t = int.from_bytes(m[:2], "big")
        sigs += 4 if t == 256 else (1 if t in (257, 258) else 0)
        if crc32c(ts, m) != crc:
            out.append(BAD_CHECKSUM)
        elif t not in KNOWN:
            out.append(UNKNOWN_TYPE)
        elif t == 256:
            sv = orc.sigcheck_channel_announcement(m)
            out.append(MALFORMED if sv == -1 else (REDUNDANT if first[_cann_scid(m)[0]] != i else sv))
        elif t == 257:
            out.append(orc.sigcheck_node_announcement(m))
        elif t == 258:
            signer = None
            if len(m) >= 112:
                a = first.get(int.from_bytes(m[98:106], "big"))
                if a is not None and a < i:
                    am = recs[a][4]
                    o = _cann_scid(am)[1] + 33 * (m[111] & 1)
                    if len(am) >= o + 33:
                        signer = am[o:o + 33]
            sv = orc.sigcheck_channel_update(m, signer or G33)
            out.append(MALFORMED if sv == -1 else (NO_CHANNEL if signer is None else sv))
        else:
            out.append(OK)
    s = dict(version=blob[0], records=len(recs), live=sum(1 for r in recs if not r[1] & F_DELETED), deleted=sum(1 for r in recs if r[1] & F_DELETED),
             end_offset=end, end_reason=why, signatures=sigs, ok=out.count(OK), skipped_deleted=out.count(DELETED), bad_checksum=out.count(BAD_CHECKSUM),
             unknown_type=out.count(UNKNOWN_TYPE), malformed=out.count(MALFORMED), redundant=out.count(REDUNDANT), no_channel=out.count(NO_CHANNEL),
             bad_signature=[out.count(k) for k in (1, 2, 3, 4)])
    s["clean"] = int(why == "eof" and s["ok"] + s["skipped_deleted"] == len(recs))
    return [r[0] for r in recs], out, s


def serialise(version, recs):
    """recs: dicts {flags, ts, msg, crc (None: computed)} -> the file"""
    out = bytearray([version])
    for r in recs:
        crc = crc32c(r["ts"], r["msg"]) if r.get("crc") is None else r["crc"]
        out += struct.pack(">HHII", r["flags"], len(r["msg"]), crc, r["ts"]) + r["msg"]
    return bytes(out)


def parse(blob):
    return [dict(flags=f, ts=ts, msg=m, crc=crc) for _, f, crc, ts, m in walk(blob)[0]]


def _golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name), "rb").read()


def oracle_backend(orc):
    def sig(blob, off, ids):
        n = len(off) - 1
        return list(orc.sigcheck_gossip_batch(np.frombuffer(blob + b"\x00", dtype=np.uint8), np.array(off, dtype=np.uint64),
                                              np.frombuffer(ids + b"\x00", dtype=np.uint8)[:33 * n].reshape(n, 33), 1))

    def key(keys):
        return [1 if orc.pubkey_parse(keys[33 * i:33 * i + 33]) is not None else 0 for i in range(len(keys) // 33)]
    return sig, key


SEED, N_OPS = 33, 450


@pytest.fixture(scope="module")
def synthetic(orc):
    """the store a gossipd life cycle leaves behind (deleted records, tombstones, dying flags): (image, model of the image).  The script is driven up to
    its first prune_network: that prune (16 days later) removes every channel, and an audit needs live ones."""
    from lightning_amd.gossipd import GossipIngest
    net, ops = gs.make_script(orc, SEED, n_ops=N_OPS, lifecycle=True)
    ops = ops[:next(i for i, op in enumerate(ops) if op[0] == "time")]
    with GossipIngest(None, gs.CHAIN, net.our_id, net.height, gs.NOW, backend=oracle_backend(orc)) as ing:
        gs.drive(net, ops, ing, SEED)
        img = ing.store_image()
    return img, model(orc, img)


def _flip_sig(m, k, bit):
    b = bytearray(m)
    b[2 + 64 * k + 40] ^= 1 << bit     # a low byte of s: stays in range
    return bytes(b)


@pytest.fixture(scope="module")
def damaged(orc, synthetic):
    """a copy of the synthetic store with at least two records damaged per class -> (image, model, {class: the verdict the class must show})"""
    img, (_, verdicts, _) = synthetic
    recs = parse(img)
    assert len(recs) == len(verdicts)
    typ = [int.from_bytes(r["msg"][:2], "big") if not r["flags"] & F_DELETED else 0 for r in recs]
    # channels with a live announcement and at least one live update behind it, each used for ONE class of damage
    chans = []
    for i, r in enumerate(recs):
        if typ[i] == 256:
            scid = _cann_scid(r["msg"])[0]
            ups = [j for j in range(i + 1, len(recs)) if typ[j] == 258 and int.from_bytes(recs[j]["msg"][98:106], "big") == scid]
            if ups:
                chans.append((i, ups))
    assert len(chans) >= 12, len(chans)
    take = iter(chans)
    mark = {}                                             # id(record) -> class name
    def fresh(r, **kw):
        r.update(kw, crc=None)
    for _ in range(2):                                    # a flipped body bit, checksum left alone
        a, ups = next(take)
        m = bytearray(recs[ups[0]]["msg"]); m[120] ^= 4
        recs[ups[0]]["msg"] = bytes(m); mark[id(recs[ups[0]])] = "body"
        m = bytearray(recs[a + 1]["msg"]); m[5] ^= 1     # the channel_amount record
        assert typ[a + 1] == 4101
        recs[a + 1]["msg"] = bytes(m); mark[id(recs[a + 1])] = "body"
    for k in (1, 3):                                      # a flipped signature bit, checksum recomputed
        a, ups = next(take)
        fresh(recs[a], msg=_flip_sig(recs[a]["msg"], k, k)); mark[id(recs[a])] = "sig"
        fresh(recs[ups[0]], msg=_flip_sig(recs[ups[0]]["msg"], 0, k)); mark[id(recs[ups[0]])] = "sig"
    nanns = [i for i, t in enumerate(typ) if t == 257]
    assert len(nanns) >= 4
    fresh(recs[nanns[0]], msg=_flip_sig(recs[nanns[0]]["msg"], 0, 5)); mark[id(recs[nanns[0]])] = "sig"
    for _ in range(2):                                    # the direction bit
        a, ups = next(take)
        m = bytearray(recs[ups[-1]]["msg"]); m[111] ^= 1
        fresh(recs[ups[-1]], msg=bytes(m)); mark[id(recs[ups[-1]])] = "direction"
    for _ in range(2):                                    # the announcement deleted: its live updates have no channel
        a, ups = next(take)
        recs[a]["flags"] |= F_DELETED
        for j in ups:
            mark[id(recs[j])] = "orphan"
    moved = []
    for _ in range(2):                                    # an update in front of its announcement
        a, ups = next(take)
        mark[id(recs[ups[0]])] = "moved"
        moved.append((recs[a], recs[ups[0]]))
    for i, t in zip(nanns[1:3], (4102, 4104)):            # the obsolete private types
        fresh(recs[i], msg=t.to_bytes(2, "big") + recs[i]["msg"][2:]); mark[id(recs[i])] = "unknown"
    for cut in (100, 120):                                # a truncated update, checksum valid
        a, ups = next(take)
        fresh(recs[ups[0]], msg=recs[ups[0]]["msg"][:cut]); mark[id(recs[ups[0]])] = "truncated"
    for ann, upd in moved:
        recs.remove(upd)
        recs.insert(next(i for i, r in enumerate(recs) if r is ann), upd)
    orig = parse(img)
    for a, _ in chans[:2]:                                # a second copy of a live announcement and its amount record, at the end
        copy = dict(orig[a], crc=None)
        recs += [copy, dict(orig[a + 1], crc=None)]
        mark[id(copy)] = "copy"
    n_complete = len(recs)
    recs.append(dict(flags=0, ts=7, msg=orig[nanns[3]]["msg"], crc=None))             # a record still being written
    blob = serialise(img[0], recs)
    classes = [mark.get(id(r)) for r in recs[:n_complete]]
    return blob, model(orc, blob), classes


# ------------------------------------------------------------------------------------------------ CPU
def test_summary_struct_layout_matches_the_header(tmp_path):
    """lamd_store_summary <-> _ffi.LamdStoreSummary: size and every offset as a C compiler lays the header's declaration out, and the same field names
    in the same order"""
    import re
    import subprocess
    from lightning_amd import _ffi
    fields = [f[0] for f in _ffi.LamdStoreSummary._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lamd_store_summary));\n'
                   + "".join('  printf("%%zu\\n", offsetof(lamd_store_summary, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_ffi.LamdStoreSummary)
    assert out[1:] == [getattr(_ffi.LamdStoreSummary, f).offset for f in fields]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct[^{;]*\{([^}]*)\} lamd_store_summary;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[[^\]]*\])?\s*[,;]", body) == fields


@pytest.mark.parametrize("name,count", [("gossip_store_simple.bin", 6), ("gossip_store_mesh_3x3.bin", 57)])
def test_frame_of_the_stores_the_reference_wrote(name, count):
    from lightning_amd.engine import gossip_store_frame
    blob = _golden(name)
    off, s = gossip_store_frame(blob)
    assert len(off) == count == s["records"] == s["live"] and s["deleted"] == 0 and s["version"] == 15
    assert s["end_offset"] == len(blob) and s["end_reason"] == "eof"
    assert list(off) == [r[0] for r in walk(blob)[0]]
    assert s["clean"] == 0 and s["ok"] == 0 and s["signatures"] == 0          # the walk alone judges nothing


def test_frame_stop_conditions_on_hand_built_tails():
    from lightning_amd import _ffi
    from lightning_amd.engine import LamdError, gossip_store_frame
    base = _golden("gossip_store_simple.bin")
    recs = parse(base)
    cann = next(r for r in recs if r["msg"][:2] == b"\x01\x00")
    uuid = dict(flags=F_COMPLETED, ts=0, msg=b"\x10\x0b" + bytes(32), crc=None)
    rec = lambda r: serialise(0, [r])[1:]
    tails = {
        "eof": rec(uuid),
        "partial_header": rec(uuid) + b"\x20\x00\x00",
        "incomplete": rec(dict(uuid, flags=0)) + rec(uuid),
        "truncated": rec(uuid)[:-1],
        "short": rec(dict(uuid, msg=b"\x01")),
        "store_ended": rec(dict(uuid, msg=b"\x10\x09" + bytes(8))) + rec(uuid),
        "no_amount": rec(dict(cann, crc=None)) + rec(uuid)[:21],
        "zero_fill": bytes(100),
    }
    u = len(rec(uuid))
    # records counted, and where the walk stops (bytes behind the base file)
    expect = {"eof": (7, u), "partial_header": (7, u), "incomplete": (6, 0), "truncated": (6, 0), "short": (6, 0), "store_ended": (7, 22), "no_amount": (6, 0),
              "zero_fill": (6, 0)}
    for why, tail in tails.items():
        blob = base + tail
        off, s = gossip_store_frame(blob)
        want, wwhy, wend = walk(blob)
        assert (list(off), s["end_reason"], s["end_offset"]) == ([r[0] for r in want], wwhy, wend), why
        assert s["end_reason"] == {"zero_fill": "incomplete"}.get(why, why)
        assert (s["records"], s["end_offset"] - len(base)) == expect[why], why
    # a deleted record is skipped whatever it holds
    off, s = gossip_store_frame(base + rec(dict(uuid, flags=F_COMPLETED | F_DELETED, msg=b"")))
    assert s["records"] == 7 and s["deleted"] == 1 and s["end_reason"] == "eof"
    # the version byte alone; a major version that is not 0; arrays too small
    assert gossip_store_frame(b"\x10")[1]["records"] == 0 and gossip_store_frame(b"\x10")[1]["end_reason"] == "eof"
    for bad in (b"\x2f" + base[1:], b""):
        with pytest.raises(LamdError):
            gossip_store_frame(bad)
    lib = _ffi.load()
    buf, off2 = np.frombuffer(base, dtype=np.uint8), np.zeros(2, dtype=np.uint64)
    n, st = ctypes.c_size_t(0), _ffi.LamdStoreSummary()
    assert lib.lamd_gossip_store_frame(buf.ctypes.data, len(base), 2, off2.ctypes.data, ctypes.byref(n), ctypes.byref(st)) == -3 and n.value == 6
    assert list(off2) == [r[0] for r in walk(base)[0]][:2]


def test_model_finds_the_reference_stores_good(orc):
    """what the GPU test relies on: the CPU oracle says every record of both files has a good checksum and good signatures, every update follows its announcement"""
    for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"):
        _, v, s = model(orc, _golden(name))
        assert set(v) == {OK} and s["clean"] == 1 and s["signatures"] > 0


def test_model_of_the_synthetic_store_and_of_its_damaged_copy(orc, synthetic, damaged):
    """the precondition of the GPU comparison: the undamaged image is judged OK / SKIPPED_DELETED only (and holds deleted records, tombstones and dying
    flags); every class of damage shows the verdict the table gives it, on the damaged records and on no other"""
    img, (_, v, s) = synthetic
    assert set(v) == {OK, DELETED} and s["clean"] == 1 and 100 <= s["records"] <= 600, s
    recs = parse(img)
    assert s["deleted"] >= 5 and any(r["msg"][:2] == b"\x10\x07" for r in recs) and any(r["flags"] & 0x0800 for r in recs)
    blob, (_, dv, ds), classes = damaged
    want = {"body": (BAD_CHECKSUM,), "sig": (1, 2, 3, 4), "direction": (1,), "orphan": (NO_CHANNEL,), "moved": (NO_CHANNEL,), "copy": (REDUNDANT,),
            "unknown": (UNKNOWN_TYPE,), "truncated": (MALFORMED,), None: (OK, DELETED)}
    for i, (c, x) in enumerate(zip(classes, dv)):
        assert x in want[c], (i, c, x)
    for c in want:
        assert classes.count(c) >= 2, c
    assert sorted(x for c, x in zip(classes, dv) if c == "sig") == [1, 1, 1, 2, 4]
    assert ds["end_reason"] == "incomplete" and ds["clean"] == 0 and ds["records"] == len(classes) and ds["end_offset"] < len(blob)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def _same(got, want):
    off, v, s = got
    woff, wv, ws = want
    assert list(off) == woff
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(v, wv)) if a != b]
    assert not bad and len(v) == len(wv), bad[:10]
    for k, x in ws.items():
        assert s[k] == x, (k, s[k], x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_audit_of_the_stores_the_reference_wrote(eng, name):
    blob = _golden(name)
    off, v, s = eng.gossip_store_audit(blob)
    recs = walk(blob)[0]
    kinds = [int.from_bytes(r[4][:2], "big") for r in recs]
    assert list(off) == [r[0] for r in recs]
    assert list(v) == [0] * len(recs), list(v)
    assert s["clean"] == 1 and s["ok"] == len(recs) and s["end_reason"] == "eof" and s["end_offset"] == len(blob)
    assert s["signatures"] == 4 * kinds.count(256) + kinds.count(258) + kinds.count(257) > 0


@pytest.mark.gpu
def test_audit_of_the_synthetic_store_equals_the_model_record_for_record(eng, synthetic, damaged):
    img, want = synthetic
    assert set(want[1]) == {OK, DELETED}
    _same(eng.gossip_store_audit(img), want)
    blob, dwant, _ = damaged
    _same(eng.gossip_store_audit(blob), dwant)


def _crc_edge_image():
    """records of type 4107 whose MESSAGE starts at every alignment 0..7 with every length 2..70 (a filler record in front sets the alignment),
    and two of 65 535 bytes; every other record carries a wrong checksum"""
    rnd = np.random.RandomState(5)
    out, want = bytearray([0x10]), []

    def add(ln, good):
        m = b"\x10\x0b" + rnd.bytes(ln - 2)
        ts = int(rnd.randint(0, 1 << 31))
        crc = crc32c(ts, m) ^ (0 if good else 1 << int(rnd.randint(0, 32)))
        out.extend(struct.pack(">HHII", F_COMPLETED, ln, crc, ts) + m)
        want.append(OK if crc == crc32c(ts, m) else BAD_CHECKSUM)
    k = 0
    for ln in range(2, 71):
        for al in range(8):
            add(2 + (al - (len(out) + 26)) % 8, True)     # the filler: 12 + filler + 12 more bytes to the next message
            assert (len(out) + 12) % 8 == al
            add(ln, k % 2 == 0)
            k += 1
    add(65535, True)
    add(65535, False)
    return bytes(out), want


@pytest.mark.gpu
def test_crc_edges_on_the_device(eng):
    blob, want = _crc_edge_image()
    assert want.count(BAD_CHECKSUM) >= 276 and want.count(OK) >= 2 * 276
    off, v, s = eng.gossip_store_audit(blob)
    assert s["end_reason"] == "eof" and len(v) == len(want)
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(v, want)) if a != b]
    assert not bad, bad[:10]
    assert s["bad_checksum"] == want.count(BAD_CHECKSUM) and s["clean"] == 0 and s["signatures"] == 0


@pytest.mark.gpu
def test_resident_image_and_the_documented_return_codes(eng, damaged):
    import torch
    from lightning_amd import _ffi
    blob, dwant, _ = damaged
    host = eng.gossip_store_audit(blob)
    for shift in (0, 3):                                  # the image at an odd device address too
        d = torch.zeros(len(blob) + shift, dtype=torch.uint8, device="cuda")
        d[shift:] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        got = eng.gossip_store_audit(blob, d_store=d[shift:])
        assert list(got[0]) == list(host[0]) and list(got[1]) == list(host[1]) == dwant[1]
        assert {k: x for k, x in got[2].items() if k != "stage_ms"} == {k: x for k, x in host[2].items() if k != "stage_ms"}
    off, v, s = eng.gossip_store_audit(b"\x10")           # a store holding only its version byte
    assert len(off) == 0 and len(v) == 0 and s["clean"] == 1 and s["records"] == 0 and s["end_reason"] == "eof"
    lib, ctx = eng._lib, eng._ctx
    buf = np.frombuffer(blob, dtype=np.uint8)
    o2, v2 = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.int8)
    n, st = ctypes.c_size_t(0), _ffi.LamdStoreSummary()
    assert lib.lamd_gossip_store_audit(ctx, buf.ctypes.data, len(blob), None, 3, o2.ctypes.data, v2.ctypes.data, ctypes.byref(n), ctypes.byref(st)) == -3
    assert n.value == len(dwant[1])
    v1 = np.frombuffer(b"\x20" + blob[1:], dtype=np.uint8)
    assert lib.lamd_gossip_store_audit(ctx, v1.ctypes.data, len(blob), None, 3, o2.ctypes.data, v2.ctypes.data, ctypes.byref(n), ctypes.byref(st)) == -3
    assert n.value == 0

"""The repair of a gossip_store FILE (lamd_gossip_store_repair, include/lightning_amd.h): the audit, the keep rules, the exclusive scan of the
kept sizes and the copy, all on the device -- against a Python model of the keep rules written here (verdicts by test_store_audit.model,
i.e. signatures by the C oracle), on the two stores the reference's own gossipd wrote (where the result must equal what the first phase of
gossipd/compactd.c writes: restated below), on the synthetic store of test_store_audit and its damaged copy, and on hand-built stores that
walk the scan's tile edges and the copy's alignment and length edges.
CPU: the model's preconditions, the summary's layout.  GPU: the device output, byte for byte."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gossip_stream as gs  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

ROOT = sa.ROOT
OK, NO_CHANNEL, F_DELETED, F_COMPLETED = sa.OK, sa.NO_CHANNEL, sa.F_DELETED, sa.F_COMPLETED
KEPT, R_DELETED, R_VERDICT, R_DEPENDENCY, R_BOOKKEEPING = 0, 1, 2, 3, 4
DROPPED = 2 ** 64 - 1
UUID = bytes(range(100, 132))
SCAN_TILE = 256          # STORE_SCAN_TILE of lightning_amd/csrc/store_repair.h: the records one block of the scan kernels takes
PACK_STAGE = 2048        # STORE_PACK_STAGE: the window of records a block of the copy stages; a longer one is searched in global memory


def uuid_record(uuid):
    msg = b"\x10\x0b" + uuid
    return struct.pack(">HHII", F_COMPLETED, len(msg), sa.crc32c(0, msg), 0) + msg


def repair_model(blob, verdicts, uuid):
    """the keep rules of include/lightning_amd.h, record by record -> (reasons, new_off, output image)"""
    recs = sa.walk(blob)[0]
    n = len(recs)
    live = [not r[1] & F_DELETED for r in recs]
    typ = [int.from_bytes(r[4][:2], "big") if live[i] else 0 for i, r in enumerate(recs)]
    first = {}                                            # scid -> lowest index of a LIVE channel_announcement
    for i, r in enumerate(recs):
        if live[i] and sa._cann_scid(r[4]):
            first.setdefault(sa._cann_scid(r[4])[0], i)
    reason = [None] * n
    nodes = {}                                            # node id -> lowest index of a KEPT channel_announcement that names it
    for i, r in enumerate(recs):
        if typ[i] != 256:
            continue
        if verdicts[i] != OK:
            reason[i] = R_VERDICT
        elif not (i + 1 < n and live[i + 1] and typ[i + 1] == 4101 and len(recs[i + 1][4]) == 10 and verdicts[i + 1] == OK):
            reason[i] = R_DEPENDENCY
        else:
            reason[i] = KEPT
            o = sa._cann_scid(r[4])[1]
            for k in (r[4][o:o + 33], r[4][o + 33:o + 66]):
                nodes.setdefault(k, i)
    kept_cann = lambda j: j is not None and 0 <= j < n and typ[j] == 256 and reason[j] == KEPT
    for i, r in enumerate(recs):
        m, t = r[4], typ[i]
        if t == 256:
            continue
        if not live[i]:
            reason[i] = R_DELETED
        elif verdicts[i] == NO_CHANNEL:
            reason[i] = R_DEPENDENCY
        elif verdicts[i] != OK:
            reason[i] = R_VERDICT
        elif t in (4103, 4105, 4107):
            reason[i] = R_BOOKKEEPING
        elif t == 4101:
            reason[i] = KEPT if kept_cann(i - 1) else R_DEPENDENCY
        elif t in (258, 4106):
            if t == 4106 and len(m) != 14:
                reason[i] = R_VERDICT
            else:
                a = first.get(int.from_bytes(m[98:106] if t == 258 else m[2:10], "big"))
                reason[i] = KEPT if a is not None and a < i and kept_cann(a) else R_DEPENDENCY
        elif t == 257:
            o = 68 + int.from_bytes(m[66:68], "big") + 4
            reason[i] = KEPT if nodes.get(m[o:o + 33], n) < i else R_DEPENDENCY
        else:
            reason[i] = R_VERDICT
    out = bytearray([blob[0]]) + uuid_record(uuid)
    new_off = []
    for i, r in enumerate(recs):
        new_off.append(len(out) if reason[i] == KEPT else DROPPED)
        if reason[i] == KEPT:
            out += blob[r[0]:r[0] + 12 + len(r[4])]
    return reason, new_off, bytes(out)


def compactd_first_phase(blob, uuid):
    """what gossipd/compactd.c writes before it catches up with the daemon: the version byte, a fresh uuid record, then every record that is
    not flagged deleted and is neither a uuid (4107) nor a delete_chan (4103) record, whatever it holds"""
    out = bytearray([blob[0]]) + uuid_record(uuid)
    for off, flags, _, _, m in sa.walk(blob)[0]:
        if not flags & F_DELETED and int.from_bytes(m[:2], "big") not in (4107, 4103):
            out += blob[off:off + 12 + len(m)]
    return bytes(out)


def _rec(msg, flags=F_COMPLETED, ts=0):
    return struct.pack(">HHII", flags, len(msg), sa.crc32c(ts, msg), ts) + msg


AMOUNT = b"\x10\x05" + (1_000_000).to_bytes(8, "big")


def scan_edge_store(orc, k):
    """one signed announcement + its amount record, k chan_dying records of its scid (all kept, 26 bytes each), and between them stray 4101
    records and records of an unknown type with seeded random lengths 2..300 (all dropped): behind every one of the first 600 dying records,
    then behind every 61st, so that the kept records start at every source alignment"""
    net = gs.Net(orc, 77, n_nodes=2, n_chans=1)
    rnd = np.random.RandomState(1000 + k % 997)
    out = bytearray([0x10]) + _rec(net.cann(0), ts=5) + _rec(AMOUNT)
    dying = b"\x10\x0a" + net.chans[0]["scid"].to_bytes(8, "big")
    for j in range(k):
        out += _rec(dying + (800_000 + j).to_bytes(4, "big"))
        if j < 600 or j % 61 == 0:
            body = rnd.bytes(int(rnd.randint(0, 299)))
            out += _rec((b"\x10\x05" if rnd.randint(2) else b"\x10\x06") + body, ts=int(rnd.randint(1 << 31)))
    return bytes(out)


def length_edge_store(orc):
    """a signed announcement + amount, then 41 node_announcements of its two nodes whose address tails give lengths of every residue mod 4
    at start offsets of every residue mod 4, one of more than 4 096 bytes and one of 65 535, the most a record's 16-bit length holds"""
    net = gs.Net(orc, 78, n_nodes=2, n_chans=1)
    out = bytearray([0x10]) + _rec(net.cann(0), ts=6) + _rec(AMOUNT)
    base = len(net.nann(0, 1))                            # 142 bytes with empty addresses
    tails = [(j * 7) % 23 for j in range(38)] + [4200 - base, 65535 - base, 3]
    for j, t in enumerate(tails):
        m = net.nann(j % 2, 1000 + j, addrs=bytes([j & 0xFF]) * t)        # (the tail as addresses: their length field reaches as far as the record's)
        assert len(m) == base + t
        out += _rec(m, ts=1000 + j)
    return bytes(out), tails


# ------------------------------------------------------------------------------------------------ CPU
def test_repair_summary_struct_layout_matches_the_header(tmp_path):
    """lamd_store_repair_summary <-> _ffi.LamdStoreRepairSummary: size and every offset as a C compiler lays the header's declaration out, and the same
    field names in the same order"""
    import re
    import subprocess
    from lightning_amd import _ffi
    fields = [f[0] for f in _ffi.LamdStoreRepairSummary._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lamd_store_repair_summary));\n'
                   + "".join('  printf("%%zu\\n", offsetof(lamd_store_repair_summary, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_ffi.LamdStoreRepairSummary)
    assert out[1:] == [getattr(_ffi.LamdStoreRepairSummary, f).offset for f in fields]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct[^{;]*\{([^}]*)\} lamd_store_repair_summary;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[[^\]]*\])?\s*[,;]", body) == fields
    from lightning_amd import Engine
    assert callable(Engine.gossip_store_repair)


def test_model_keeps_what_compactd_keeps_of_the_reference_stores(orc):
    """what the GPU test relies on: on the stores the reference wrote every record passes and every dependency is in front of its dependant, so the
    model's output is compactd's"""
    for name in ("gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"):
        blob = sa._golden(name)
        reason, new_off, out = repair_model(blob, sa.model(orc, blob)[1], UUID)
        assert out == compactd_first_phase(blob, UUID)
        assert set(reason) == {KEPT} and len(out) == len(blob) + 46          # (these files carry no uuid record: the output is as long as one can get)


def test_model_of_the_hand_built_stores(orc):
    """the hand-built stores hold what their builders promise: every dying record and every node_announcement kept, every stray dropped, every
    alignment and length residue present"""
    blob = scan_edge_store(orc, SCAN_TILE + 1)
    _, v, s = sa.model(orc, blob)
    reason, new_off, out = repair_model(blob, v, UUID)
    recs = sa.walk(blob)[0]
    dying = [i for i, r in enumerate(recs) if r[4][:2] == b"\x10\x0a"]
    assert len(dying) == SCAN_TILE + 1 and all(reason[i] == KEPT for i in dying) and reason[:2] == [KEPT, KEPT]
    assert reason.count(KEPT) == len(dying) + 2 and reason.count(R_VERDICT) > 50 and reason.count(R_DEPENDENCY) > 50
    assert {recs[i][0] % 4 for i in dying} == {0, 1, 2, 3} and {new_off[i] % 4 for i in dying} >= {1, 3}
    blob, tails = length_edge_store(orc)
    _, v, s = sa.model(orc, blob)
    assert s["clean"] == 1 and s["records"] == 2 + len(tails)
    reason, new_off, out = repair_model(blob, v, UUID)
    assert reason == [KEPT] * (2 + len(tails)) and out == blob[:1] + uuid_record(UUID) + blob[1:]
    recs = sa.walk(blob)[0][2:]
    assert {len(r[4]) % 4 for r in recs} == {0, 1, 2, 3} and {r[0] % 4 for r in recs} == {0, 1, 2, 3}
    assert max(len(r[4]) for r in recs) == 65535 and sum(1 for r in recs if 4096 < len(r[4]) < 65535) == 1


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from lightning_amd import Engine
    with Engine(0) as e:
        yield e


def _same(got, blob, want_verdicts, want):
    """the device's (out, rec_off, verdict, new_off, reason, summary, repair summary) against the model's (reasons, new_off, image)"""
    out, off, v, new_off, reason, s, r = got
    wreason, wnew, wout = want
    assert list(off) == [x[0] for x in sa.walk(blob)[0]] and list(v) == list(want_verdicts)
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(reason, wreason)) if a != b]
    assert not bad and len(reason) == len(wreason), bad[:10]
    bad = [(i, int(a), b) for i, (a, b) in enumerate(zip(new_off, wnew)) if int(a) != b]
    assert not bad, bad[:10]
    assert r["out_len"] == len(wout) == len(out)
    if out != wout:
        k = next(i for i, (a, b) in enumerate(zip(out, wout)) if a != b)
        raise AssertionError("output differs from byte %d on: %s / %s" % (k, out[k:k + 16].hex(), wout[k:k + 16].hex()))
    assert [r[k] for k in ("kept", "dropped_deleted", "dropped_verdict", "dropped_dependency", "dropped_bookkeeping")] == [wreason.count(k) for k in range(5)]
    assert len(out) <= len(blob) + 46


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_repair_of_the_stores_the_reference_wrote_equals_compactd(eng, name):
    blob = sa._golden(name)
    out, off, v, new_off, reason, s, r = eng.gossip_store_repair(blob, UUID)
    assert out == compactd_first_phase(blob, UUID)
    assert s["clean"] == 1 and list(v) == [0] * len(off) and r["kept"] == len(off) and r["out_len"] == len(blob) + 46
    for o, no in zip(off, new_off):                       # every new_off points at an identical record
        ln = 12 + int.from_bytes(blob[int(o) + 2:int(o) + 4], "big")
        assert int(no) != DROPPED and out[int(no):int(no) + ln] == blob[int(o):int(o) + ln]


@pytest.mark.gpu
def test_repair_of_the_damaged_store_equals_the_model(eng, orc, synthetic, damaged):
    blob, (_, dv, _), classes = damaged
    want = repair_model(blob, dv, UUID)
    got = eng.gossip_store_repair(blob, UUID)
    _same(got, blob, dv, want)
    reason = list(got[4])
    recs = sa.walk(blob)[0]
    expect = {"body": R_VERDICT, "sig": R_VERDICT, "direction": R_VERDICT, "orphan": R_DEPENDENCY, "moved": R_DEPENDENCY, "copy": R_VERDICT,
              "unknown": R_VERDICT, "truncated": R_VERDICT}
    for i, c in enumerate(classes):
        if c is not None:
            assert reason[i] == expect[c], (i, c, reason[i])
    # a damaged amount record takes its announcement with it, and the announcement that channel's updates
    hit = 0
    for i, c in enumerate(classes):
        if c == "body" and recs[i][4][:2] == b"\x10\x05":
            scid = sa._cann_scid(recs[i - 1][4])[0]
            assert reason[i - 1] == R_DEPENDENCY
            ups = [j for j, r in enumerate(recs) if r[4][:2] == b"\x01\x02" and not r[1] & F_DELETED and int.from_bytes(r[4][98:106], "big") == scid
                   and classes[j] is None]
            assert ups and all(reason[j] == R_DEPENDENCY for j in ups)
            hit += 1
    assert hit == 2
    # so does an announcement with a bad signature; an announcement's second copy does not
    for i, c in enumerate(classes):
        if c in ("sig", "copy") and recs[i][4][:2] == b"\x01\x00":
            assert reason[i + 1] == R_DEPENDENCY
    assert set(reason) == {KEPT, R_DELETED, R_VERDICT, R_DEPENDENCY, R_BOOKKEEPING}
    img, (_, sv, _) = synthetic
    _same(eng.gossip_store_repair(img, UUID), img, sv, repair_model(img, sv, UUID))


@pytest.mark.gpu
def test_repaired_stores_audit_clean_and_repair_to_themselves(eng, synthetic, damaged):
    for blob in (synthetic[0], damaged[0]):
        out, _, _, _, _, _, r = eng.gossip_store_repair(blob, UUID)
        _, v, s = eng.gossip_store_audit(out)
        assert s["clean"] == 1 and s["records"] == r["kept"] + 1 == s["ok"], (s, r)
        again = eng.gossip_store_repair(out, UUID)
        assert again[0] == out and again[6]["kept"] == r["kept"] and again[6]["dropped_bookkeeping"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE * SCAN_TILE + 1])
def test_scan_tiles_and_source_alignments(eng, orc, k):
    """k kept dying records between dropped strays: record counts below, at and above one tile of the scan (SCAN_TILE = 256 records per block), and
    above tile * tile, where the tile sums themselves no longer fit one tile"""
    blob = scan_edge_store(orc, k)
    _, v, _ = sa.model(orc, blob)
    want = repair_model(blob, v, UUID)
    assert want[0].count(KEPT) == k + 2
    _same(eng.gossip_store_repair(blob, UUID), blob, v, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_scan_with_record_counts_at_the_tile_edge(eng, orc, n):
    """the scan runs over n + 1 sizes (the last one closes it): stores of n records around the tile, every second dying record a deleted one"""
    net = gs.Net(orc, 77, n_nodes=2, n_chans=1)
    dying = b"\x10\x0a" + net.chans[0]["scid"].to_bytes(8, "big")
    blob = bytes([0x10]) + _rec(net.cann(0), ts=5) + _rec(AMOUNT)
    blob += b"".join(_rec(dying + j.to_bytes(4, "big"), flags=F_COMPLETED | (F_DELETED if j % 2 else 0x0800)) for j in range(n - 2))
    _, v, s = sa.model(orc, blob)
    assert s["records"] == n
    want = repair_model(blob, v, UUID)
    assert want[0].count(KEPT) == 2 + (n - 1) // 2 and want[0].count(R_DELETED) == (n - 2) // 2
    _same(eng.gossip_store_repair(blob, UUID), blob, v, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [PACK_STAGE - 1, PACK_STAGE, PACK_STAGE + 1, 3 * PACK_STAGE])
def test_long_runs_of_dropped_records(eng, orc, n):
    """n records whose kept ones fit one block of the copy -- announcement, amount, a dying record, n - 4 deleted ones, a dying record: the window that
    block searches holds all n records, below, at and above what it stages (PACK_STAGE = 2048 records)"""
    net = gs.Net(orc, 77, n_nodes=2, n_chans=1)
    dying = b"\x10\x0a" + net.chans[0]["scid"].to_bytes(8, "big")
    blob = bytes([0x10]) + _rec(net.cann(0), ts=5) + _rec(AMOUNT) + _rec(dying + bytes(4))
    blob += b"".join(_rec(dying + j.to_bytes(4, "big"), flags=F_COMPLETED | F_DELETED) for j in range(n - 4)) + _rec(dying + b"\xff\xff\xff\xff", ts=9)
    _, v, s = sa.model(orc, blob)
    assert s["records"] == n
    want = repair_model(blob, v, UUID)
    assert want[0].count(KEPT) == 4 and want[0].count(R_DELETED) == n - 4 and want[0][-1] == KEPT and len(want[2]) < 4 * 2048
    _same(eng.gossip_store_repair(blob, UUID), blob, v, want)


@pytest.mark.gpu
def test_record_lengths_and_start_offsets(eng, orc):
    blob, tails = length_edge_store(orc)
    _, v, _ = sa.model(orc, blob)
    want = repair_model(blob, v, UUID)
    assert want[0] == [KEPT] * (2 + len(tails))
    _same(eng.gossip_store_repair(blob, UUID), blob, v, want)


@pytest.mark.gpu
def test_resident_input_and_output_and_the_documented_return_codes(eng, damaged):
    import torch
    from lightning_amd import _ffi
    blob, (_, dv, _), _ = damaged
    want = repair_model(blob, dv, UUID)
    host = eng.gossip_store_repair(blob, UUID)
    assert host[0] == want[2]
    for shift in (0, 1, 2, 3):                            # the image and the output at odd device addresses too; the output buffer exactly as long as needed
        d = torch.zeros(len(blob) + shift, dtype=torch.uint8, device="cuda")
        d[shift:] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((len(want[2]) + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        exact = d_out[(4 - shift) % 4:(4 - shift) % 4 + len(want[2])]
        got = eng.gossip_store_repair(blob, UUID, d_store=d[shift:], d_out=exact, host_out=shift == 0)
        assert got[0] == (want[2] if shift == 0 else None)
        torch.cuda.synchronize()
        back = d_out.cpu().numpy().tobytes()
        lo = (4 - shift) % 4
        assert back[lo:lo + len(want[2])] == want[2] and set(back[:lo] + back[lo + len(want[2]):]) <= {0xAB}
        assert [list(got[k]) for k in (1, 2, 3, 4)] == [list(host[k]) for k in (1, 2, 3, 4)] and got[6]["out_len"] == len(want[2])
    # a roomy device buffer, no host copy
    d_big = torch.full((len(blob) + 46,), 0xCD, dtype=torch.uint8, device="cuda")
    got = eng.gossip_store_repair(blob, UUID, d_out=d_big, host_out=False)
    torch.cuda.synchronize()
    assert d_big.cpu().numpy().tobytes()[:got[6]["out_len"]] == want[2]
    # a store holding only its version byte: version + uuid record
    out, off, v, new_off, reason, s, r = eng.gossip_store_repair(b"\x0d", UUID)
    assert out == b"\x0d" + uuid_record(UUID) and len(out) == 47 and len(off) == 0 and s["clean"] == 1 and r["kept"] == 0 and r["out_len"] == 47
    d47 = torch.zeros(47, dtype=torch.uint8, device="cuda")
    eng.gossip_store_repair(b"\x0d", UUID, d_out=d47, host_out=False)
    assert d47.cpu().numpy().tobytes() == out
    # the documented return codes
    lib, ctx = eng._lib, eng._ctx
    buf, uu = np.frombuffer(blob, dtype=np.uint8), np.frombuffer(UUID, dtype=np.uint8)
    n = len(dv)
    o, vv, no, rs = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    cnt, st, rp = ctypes.c_size_t(0), _ffi.LamdStoreSummary(), _ffi.LamdStoreRepairSummary()
    small = np.full(len(want[2]), 0xEE, dtype=np.uint8)
    call = lambda cap, out, d_out, out_cap: lib.lamd_gossip_store_repair(ctx, buf.ctypes.data, len(blob), None, uu.ctypes.data, cap, o.ctypes.data, vv.ctypes.data,
                                                                         no.ctypes.data, rs.ctypes.data, ctypes.byref(cnt), out, d_out, out_cap, ctypes.byref(st), ctypes.byref(rp))
    assert call(3, small.ctypes.data, None, len(small)) == -3 and cnt.value == n                   # too few entries: the count needed
    assert call(n, small.ctypes.data, None, len(small) - 1) == -3 and rp.out_len == len(want[2])    # output too small: the size needed, the rest filled in
    assert list(rs) == want[0] and list(no) == want[1] and list(vv) == dv and set(small) == {0xEE}
    d_small = torch.full((len(want[2]) + 4,), 0xAB, dtype=torch.uint8, device="cuda")
    assert call(n, None, d_small.data_ptr(), len(want[2]) - 5) == -3 and rp.out_len == len(want[2])
    torch.cuda.synchronize()
    assert set(d_small.cpu().numpy().tobytes()[len(want[2]) - 5:]) == {0xAB}                        # nothing written behind out_cap
    assert call(n, None, None, 0) == 0 and rp.out_len == len(want[2]) and rp.kept == want[0].count(KEPT)   # the maps and the counters only
    assert call(n, small.ctypes.data, None, len(small)) == 0 and small.tobytes() == want[2]
    v1 = np.frombuffer(b"\x20" + blob[1:], dtype=np.uint8)
    assert lib.lamd_gossip_store_repair(ctx, v1.ctypes.data, len(blob), None, uu.ctypes.data, n, o.ctypes.data, vv.ctypes.data, no.ctypes.data, rs.ctypes.data,
                                        ctypes.byref(cnt), None, None, 0, ctypes.byref(st), ctypes.byref(rp)) == -3 and cnt.value == 0

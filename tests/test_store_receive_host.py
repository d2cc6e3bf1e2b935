"""lightning_amd/csrc/store_receive.h on the host, under AddressSanitizer and UBSan (tests/c/store_receive_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the reception of channel_update batches against a store image, on which the header
and the sequential model of update_receive_model must agree exactly -- status, flags, channel numbers, signers, every list and every output byte
-- for the golden stores, the synthetic store with and without the verdicts of its damaged copy, and a hand-built batch that meets every status
and flag; the messages, rows and sorted positions visited in arrival order, in reverse and in a scrambled order, the output written at all four
alignments (the program compares those itself).  The signature verdicts are an input computed by the oracle: the stages on both sides of the
signature batch are what is under test here; the device side, signature batch included, is test_gpu_update_receive's.  Two further tests: the
plan applied to the image of a live GossipIngest equals the image that ingest holds after it has processed the same batch; and the new
prototype of include/lightning_amd.h agrees with its ctypes binding.  Last, the updates of the stores the reference ships (test_reference_stores),
foreign signatures and all, received against those stores."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_range_model as crm  # noqa: E402
import gossip_stream as gs  # noqa: E402
import test_reference_stores as rs  # noqa: E402
import test_store_audit as sa  # noqa: E402
import update_receive_model as urm  # noqa: E402
from test_store_audit import damaged, synthetic  # noqa: E402,F401  (fixtures)

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_receive") / "store_receive_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_receive_host.cpp")])
    return path


def host_run(exe, d, blob, v, msgs, chain, now, sigv, prune=0, our_id=None, peers=None, held=()):
    """-> dict of what the host build of the header computes.  sigv: one verdict per message"""
    d.mkdir()
    (d / "image").write_bytes(blob)
    count = sum(1 for r in v["rec"] if r[1] != urm.NONE or r[2] != urm.NONE)
    nbare = len(v["rec"]) - count
    view = struct.pack("<III", len(v["recs"]), count, nbare) + np.array([r[0] for r in v["recs"]], dtype="<u8").tobytes()
    view += np.array(v["scids"], dtype="<u8").tobytes() + np.array([x for r in v["rec"][:count] for x in r], dtype="<u4").tobytes()
    view += np.array([r[0] for r in v["rec"][count:]], dtype="<u4").tobytes() + np.array([x for t in v["ts"][:count] for x in t], dtype="<u4").tobytes()
    (d / "view").write_bytes(view)
    hs = sorted(set(held))
    batch = chain + struct.pack("<QII", now, prune or 1209600, our_id is not None) + (bytes(33) if our_id is None else bytes(our_id))
    batch += struct.pack("<II", peers is not None, len(hs)) + np.array(hs, dtype="<u8").tobytes() + struct.pack("<I", len(msgs))
    for i, m in enumerate(msgs):
        batch += struct.pack("<I", len(m)) + bytes(m)
        if peers is not None:
            batch += bytes(33) if peers[i] is None else bytes(peers[i])
    (d / "batch").write_bytes(batch)
    (d / "sigv").write_bytes(np.array(sigv, dtype=np.int8).tobytes())
    r = subprocess.run([exe, str(d / "image"), str(d / "view"), str(d / "batch"), str(d / "sigv"), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda name, dt: [int(x) for x in np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)]
    signer = (d / "out.signer").read_bytes()
    return dict(status=arr("status", np.int8), flags=arr("flags", np.uint8), chan=arr("chan", "<u4"), add_msg=arr("addmsg", "<u4"), add_off=arr("addoff", "<u8"),
                del_rec=arr("del", "<u4"), sets=list(zip(arr("setrec", "<u4"), arr("setts", "<u4"), arr("setcrc", "<u4"))), bytes=(d / "out.bytes").read_bytes(),
                rows=arr("rows", "<u4")[0], signer=[signer[34 * i + 1:34 * i + 34] if signer[34 * i] else None for i in range(len(msgs))])


def check_against_model(exe, d, orc, blob, msgs, chain, now, verdict=None, **kw):
    v = urm.view(blob, verdict)
    want = urm.receive(v, msgs, chain, now, urm.checker(orc), kw.get("prune", 0), kw.get("our_id"), kw.get("peers"), kw.get("held", ()))
    # the verdict of the signature batch for each message under the signer the model names (1 where the model checks none: whatever the header
    # asks about such a message must fail)
    sigv = [1 if s is None else (0 if urm.checker(orc)(m, s) else 1) for m, s in zip(msgs, want["signer"])]
    got = host_run(exe, d, blob, v, msgs, chain, now, sigv, **kw)
    for k in ("status", "flags", "chan", "signer", "add_msg", "del_rec", "sets"):
        assert got[k] == want[k], (k, got[k][:6], want[k][:6])
    assert got["bytes"] == b"".join(want["records"]) and got["rows"] == sum(1 for s in want["signer"] if s is not None)
    offs, at = [], 0
    for r in want["records"]:
        offs.append(at)
        at += len(r)
    assert got["add_off"] == offs
    return v, want


@pytest.fixture(scope="module")
def hand(orc):
    net = urm.hand_net(orc)
    return net, urm.hand_store(net, crm.CHAIN), urm.hand_batch(net, crm.CHAIN, gs.OTHER_CHAIN)


def test_every_status_and_flag_by_hand(exe, tmp_path, orc, hand):
    net, blob, (msgs, peers, held, ours) = hand
    v, want = check_against_model(exe, tmp_path / "hand", orc, blob, msgs, crm.CHAIN, urm.NOW, our_id=ours, peers=peers, held=held)
    assert sorted(set(want["status"])) == list(range(-1, 10))
    assert all(any(f & bit for f in want["flags"]) for bit in (1, 2, 4, 8)) and {3, 6} <= set(want["flags"])
    # by hand: the newer update, its copy, a stale one, a newer one still: accepted and superseded, duplicate, stale, accepted
    assert want["status"][:5] == [0, 9, 8, 8, 0] and want["flags"][:5] == [1, 0, 0, 0, 0] and want["chan"][0] == 0
    assert want["status"][10:14] == [2, 0, 2, 0]                                                 # both edges of the window, and one past each
    assert (want["status"][16], want["flags"][16], want["status"][17], want["status"][18]) == (4, 8, 5, 4)
    assert [want["flags"][i] for i in (19, 20, 21, 23)] == [3, 0, 0, 6] and want["status"][22] == 9
    assert want["del_rec"] == [16, 17, 21, 22, 23] and len(want["sets"]) == 3 and [s[0] for s in want["sets"]] == [4, 6, 14]
    assert urm.apply(blob, v, want)[:len(blob)] != blob and sa.model(orc, urm.apply(blob, v, want))[2]["clean"] == 1
    # no peers: the private ones are unknown; no held list and no our_id
    _, bare = check_against_model(exe, tmp_path / "plain", orc, blob, msgs, crm.CHAIN, urm.NOW)
    assert [bare["status"][i] for i in (14, 15, 16, 17, 18)] == [0, 5, 5, 5, 5] and not any(f & 8 for f in bare["flags"])
    # per-message peers, some without a source; now below the prune interval: now - prune wraps and everything is too old
    mixed = [None if i % 3 == 0 else net.node_id[1] for i in range(len(msgs))]
    _, mx = check_against_model(exe, tmp_path / "mixed", orc, blob, msgs, crm.CHAIN, urm.NOW, peers=mixed)
    assert (mx["status"][16], mx["status"][18]) == (4, 5)
    _, early = check_against_model(exe, tmp_path / "early", orc, blob, msgs, crm.CHAIN, 1000, prune=2000)
    assert set(early["status"]) == {-1, 1, 2}
    _, short = check_against_model(exe, tmp_path / "prune", orc, blob, msgs, crm.CHAIN, urm.NOW, prune=4990, peers=peers)
    assert short["status"].count(2) > want["status"].count(2)


def test_orders_of_arrival(exe, tmp_path, orc, hand):
    """the same messages reversed and shuffled: other winners, the same agreement"""
    net, blob, (msgs, peers, held, ours) = hand
    seen = set()
    for k, order in enumerate((list(range(len(msgs)))[::-1], random.Random(4).sample(range(len(msgs)), len(msgs)), random.Random(5).sample(range(len(msgs)), len(msgs)))):
        _, want = check_against_model(exe, tmp_path / ("o%d" % k), orc, blob, [msgs[i] for i in order] * 2, crm.CHAIN, urm.NOW, our_id=ours, peers=peers * 2, held=held)
        assert want["status"][len(msgs):].count(0) == 0                                          # the second copy of anything is at best a duplicate
        seen.add(tuple(want["status"]))
    assert len(seen) == 3


def test_one_slot_and_empty_batches(exe, tmp_path, orc, hand):
    net, blob, _ = hand
    ups = [net.cupd(0, 0, urm.T0 + 1 + k, chain=crm.CHAIN, extra=bytes(k % 5)) for k in range(12)]
    rnd = random.Random(9)
    batch = [rnd.choice(ups) for _ in range(300)]
    _, want = check_against_model(exe, tmp_path / "slot", orc, blob, batch, crm.CHAIN, urm.NOW)
    assert set(want["status"]) == {0, 8, 9} and want["del_rec"] == [16] and want["flags"].count(1) == want["status"].count(0) - 1
    check_against_model(exe, tmp_path / "none", orc, blob, [], crm.CHAIN, urm.NOW)
    check_against_model(exe, tmp_path / "one", orc, blob, [ups[3]], crm.CHAIN, urm.NOW)
    check_against_model(exe, tmp_path / "junk", orc, blob, [b"", b"\x01\x02", bytes(200)], crm.CHAIN, urm.NOW)


def updates_for(v, rnd, count):
    """unsigned updates over the channels of a view (the stores of these tests were not signed by keys we hold): every one fails its signature,
    or is decided in front of it"""
    out = []
    for _ in range(count):
        c = rnd.randrange(len(v["scids"]))
        d = rnd.randrange(2)
        ts = (v["ts"][c][d] or urm.T0) + rnd.randrange(-2, 3)
        out.append(crm.cupd(v["scids"][c] if rnd.random() < 0.9 else v["scids"][c] ^ 1 << 60, d, ts, 138 + rnd.randrange(4)))
    return out


@pytest.mark.parametrize("name", ["gossip_store_simple.bin", "gossip_store_mesh_3x3.bin"])
def test_the_stores_the_reference_wrote(exe, tmp_path, orc, name):
    """the golden stores' own updates received again (duplicates of the records in force: status 9 under the real signers), older and newer copies
    of them with broken signatures, and updates of unknown channels"""
    blob = sa._golden(name)
    v = urm.view(blob)
    ups = [r[4] for r in v["recs"] if not r[1] & sa.F_DELETED and r[4][:2] == b"\x01\x02"]
    assert ups and v["scids"]
    chain = ups[0][66:98]
    now = max(int.from_bytes(m[106:110], "big") for m in ups) + 100
    rnd = random.Random(11)
    batch = list(ups) + updates_for(v, rnd, 40)
    batch = [m[:66] + chain + m[98:] if m[66:98] != chain else m for m in batch]
    rnd.shuffle(batch)
    _, want = check_against_model(exe, tmp_path / "g", orc, blob, batch, chain, now, peers=[bytes([2]) + bytes(range(32))] * len(batch))
    assert want["status"].count(9) >= 1 and 6 in want["status"] and want["status"].count(0) == 0


def test_the_synthetic_store_with_and_without_verdicts(exe, tmp_path, orc, synthetic, damaged):
    img, (_, ver, _) = synthetic
    net = gs.Net(orc, sa.SEED)                                                                # the network that signed it (make_script's)
    rnd = random.Random(12)
    for tag, blob, verdict in (("plain", img, None), ("ok", img, list(ver)), ("damaged", damaged[0], list(damaged[1][1]))):
        v = urm.view(blob, verdict)
        batch = []
        for c in range(len(net.chans)):
            for d in (0, 1):
                k = v["chan"].get(net.chans[c]["scid"])
                base = v["ts"][k][d] if k is not None and v["rec"][k][1 + d] != urm.NONE else gs.NOW
                batch += [net.cupd(c, d, base + x) for x in (-1, 0, 1, 1, 3)]
        rnd.shuffle(batch)
        _, want = check_against_model(exe, tmp_path / tag, orc, blob, batch, gs.CHAIN, gs.NOW + 500, our_id=net.our_id, peers=[net.peers[1]] * len(batch))
        assert {0, 8, 9} <= set(want["status"]) and want["del_rec"] and any(f & 1 for f in want["flags"])
        if tag == "plain":
            assert 5 in want["status"] and any(f & 8 for f in want["flags"])


def test_the_plan_applied_equals_the_ingests_own_store(exe, tmp_path, orc):
    """closing the loop on the CPU: a GossipIngest (oracle backend, no pending state) whose store_image() is received against; the same batch
    pushed through the ingest; its image afterwards is the old image with the HEADER's plan applied (the bytes and lists the host build of
    store_receive.h wrote), byte for byte -- and so with the model's"""
    from lightning_amd.gossipd import GossipIngest
    net, ops = gs.make_script(orc, 21, n_ops=300)
    with GossipIngest(None, gs.CHAIN, net.our_id, net.height + 200, gs.NOW, backend=sa.oracle_backend(orc)) as ing:
        gs.drive(net, ops, ing, 21)
        ing.new_block(net.height + 400)
        ing.process()
        before = ing.store_image()
        v = urm.view(before)
        assert len(v["scids"]) >= 5
        known = [c for c in range(len(net.chans)) if net.chans[c]["scid"] in v["chan"]]
        unknown = [c for c in range(len(net.chans)) if net.chans[c]["scid"] not in v["chan"]]
        batch = []
        for c in known[:8] + unknown[:2]:
            for d in (0, 1):
                k = v["chan"].get(net.chans[c]["scid"])
                base = v["ts"][k][d] if k is not None and v["rec"][k][1 + d] != urm.NONE else gs.NOW
                batch += [net.cupd(c, d, base + x) for x in (0, 2, 1, 5)]
        random.Random(3).shuffle(batch)
        for m in batch:
            ing.push(net.peers[1], m)
        ing.process()
        after = ing.store_image()
    peers = [net.peers[1]] * len(batch)
    want = urm.receive(v, batch, gs.CHAIN, gs.NOW, urm.checker(orc), our_id=net.our_id, peers=peers)
    sigv = [1 if s is None else (0 if urm.checker(orc)(m, s) else 1) for m, s in zip(batch, want["signer"])]
    got = host_run(exe, tmp_path / "ingest", before, v, batch, gs.CHAIN, gs.NOW, sigv, our_id=net.our_id, peers=peers)
    assert got["status"].count(0) >= 8 and {5, 8, 9} <= set(got["status"])
    applied = bytearray(before)                                                              # the header's plan, applied as a caller would
    for k in got["del_rec"]:
        applied[v["recs"][k][0]] |= 0x80
    for a, ts, crc in got["sets"]:
        applied[v["recs"][a][0] + 4:v["recs"][a][0] + 12] = struct.pack(">II", crc, ts)
    assert after == bytes(applied) + got["bytes"]
    assert after == urm.apply(before, v, want) and got["status"] == want["status"]


def test_new_prototype_and_binding_agree(tmp_path):
    """the prototype this header section adds has the argument count of its ctypes binding, and the summary the layout a C compiler gives it"""
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    n = "lamd_channel_update_receive_batch"
    proto = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
    assert proto, n
    res, args = _ffi.SYMBOLS[n]
    assert len(proto.group(2).split(",")) == len(args) == 29 and res is ctypes.c_int and proto.group(1) == "int"
    for text, ct in zip(proto.group(2).split(","), args):
        assert (("size_t" in text or "uint64_t" in text) and "*" not in text) == (ct in (ctypes.c_size_t, ctypes.c_uint64)), text   # (one type on LP64)
        assert ("uint32_t" in text and "*" not in text) == (ct is ctypes.c_uint32), text
    cls = _ffi.LamdUpdateReceiveSummary
    assert [f[0] for f in cls._fields_][-2:] == ["stage_ms", "signature_rows"]
    lines = ['  printf("%zu\\n", sizeof(lamd_update_receive_summary));\n'] + ['  printf("%%zu\\n", offsetof(lamd_update_receive_summary, %s));\n' % f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()]
    assert out == [ctypes.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert hasattr(_ffi.load(), n)


@pytest.mark.parametrize("name", ["mainnet", "part1", "canned"])
def test_the_stores_the_reference_ships_receive_their_own_updates(exe, tmp_path, orc, name):
    """every channel_update found in the image (for part 1: in part 1 + part 2), the deleted ones included, in file order, then the same with one bit
    of each signature flipped"""
    blob = rs.store(name)
    ups = rs.updates_in(rs.store("mainnet") if name == "part1" else blob)
    msgs, chain = [m for _, _, m in ups], rs.chain_of(blob)
    now = max(r[3] for r in sa.walk(rs.store("mainnet") if name == "part1" else blob)[0]) + 1
    v, want = check_against_model(exe, tmp_path / "own", orc, blob, msgs, chain, now, verdict=sa.model(orc, blob)[1])
    assert 6 not in want["status"] and sum(1 for s in want["signer"] if s is not None) == (rs.PART1_RECEIVE["signed"] if name == "part1" else len(msgs))
    if name != "part1":
        assert all(want["status"][k] == urm.DUPLICATE for k, u in enumerate(ups) if not u[1])
    else:
        assert want["status"].count(urm.UNKNOWN) == rs.PART1_RECEIVE["unknown"] and want["status"].count(urm.ACCEPTED) == rs.PART1_RECEIVE["accepted"]
        assert sa.model(orc, urm.apply(blob, v, want))[2]["clean"] == 1
    flipped = [m[:40] + bytes([m[40] ^ 1]) + m[41:] for m in msgs]
    _, bad = check_against_model(exe, tmp_path / "flipped", orc, blob, flipped, chain, now)
    assert urm.ACCEPTED not in bad["status"] and urm.BAD_SIGNATURE in bad["status"]
    if name == "part1":                                                                          # what was accepted now fails its signature
        assert all(b == urm.BAD_SIGNATURE for a, b in zip(want["status"], bad["status"]) if a == urm.ACCEPTED)
        assert sum(1 for s in bad["signer"] if s is not None) == rs.PART1_RECEIVE["signed"] and bad["status"].count(urm.UNKNOWN) == rs.PART1_RECEIVE["unknown"]

"""lightning_amd/csrc/store_nodes.h on the host, under AddressSanitizer and UBSan (tests/c/store_nodes_host.cpp, a stand-alone program: every
buffer it hands over is a heap block of exactly its size): the reception of node_announcement batches against a store image, on which the
header and the sequential model of node_receive_model must agree exactly -- status, flags, node ranks, which signatures are looked at, every
list and every output byte -- for a hand-built batch that meets every status and flag, its orders of arrival, batches aimed at one node, the
synthetic store with and without verdicts, and the literals of the reference's own test; the channels, messages, rows and sorted positions
visited in arrival order, in reverse and in a scrambled order, the output written at all four alignments (the program compares those itself).
The signature verdicts are an input computed by the oracle: the stages on both sides of the signature batch are what is under test here; the
device side, signature batch included, is test_gpu_node_receive's.  Two further tests: the plan applied to the image of a live GossipIngest
equals the image that ingest holds after it has processed the same batch; and the new prototype of include/lightning_amd.h agrees with its
ctypes binding."""
import ctypes
import json
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
import node_receive_model as nrm  # noqa: E402
import test_store_audit as sa  # noqa: E402
from test_store_audit import synthetic  # noqa: E402,F401  (fixture)

ROOT = sa.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("store_nodes") / "store_nodes_host")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lightning_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "c", "store_nodes_host.cpp")])
    return path


def host_run(exe, d, blob, v, msgs, sigv, pending=False):
    """-> dict of what the host build of the header computes.  sigv: one verdict per message"""
    d.mkdir()
    (d / "image").write_bytes(blob)
    count = v["entries"]
    nbare = len(v["scids"]) - count
    u4 = lambda x: np.array(x, dtype="<u4").tobytes()
    view = struct.pack("<IIII", len(v["recs"]), count, nbare, len(v["ids"])) + np.array([r[0] for r in v["recs"]], dtype="<u8").tobytes()
    view += u4([x for e in v["ent_rec"] for x in e]) + u4(v["chan_rec"][count:]) + u4([x for r in v["chan_rank"] for x in r])
    view += np.array(v["node_off"], dtype="<u8").tobytes() + u4([0 if k == nrm.NONE else k + 1 for k in v["nann"]])
    (d / "view").write_bytes(view)
    batch = struct.pack("<II", int(pending), len(msgs)) + b"".join(struct.pack("<I", len(m)) + bytes(m) for m in msgs)
    (d / "batch").write_bytes(batch)
    (d / "sigv").write_bytes(np.array(sigv, dtype=np.int8).tobytes())
    r = subprocess.run([exe, str(d / "image"), str(d / "view"), str(d / "batch"), str(d / "sigv"), str(d / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    arr = lambda name, dt: [int(x) for x in np.frombuffer((d / ("out." + name)).read_bytes(), dtype=dt)]
    return dict(status=arr("status", np.int8), flags=arr("flags", np.uint8), node=arr("node", "<u4"), checked=[bool(x) for x in arr("checked", np.uint8)],
                add_msg=arr("addmsg", "<u4"), add_off=arr("addoff", "<u8"), del_rec=arr("del", "<u4"), bytes=(d / "out.bytes").read_bytes(), rows=arr("rows", "<u4")[0])


def check_against_model(exe, d, orc, blob, msgs, verdict=None, pending=False):
    v = nrm.view(blob, verdict)
    check = nrm.checker(orc)
    want = nrm.receive(v, msgs, check, pending)
    # the verdict of the signature batch for each message (1 where the model looks at none: whatever the header asks about such a message must fail)
    sigv = [(0 if check(m) else 1) if c else 1 for m, c in zip(msgs, want["checked"])]
    got = host_run(exe, d, blob, v, msgs, sigv, pending)
    for k in ("status", "flags", "node", "checked", "add_msg", "del_rec"):
        assert got[k] == want[k], (k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6])
    assert got["bytes"] == b"".join(want["records"]) and got["rows"] == sum(want["checked"])
    offs, at = [], 0
    for r in want["records"]:
        offs.append(at)
        at += len(r)
    assert got["add_off"] == offs
    return v, want


@pytest.fixture(scope="module")
def hand(orc):
    net = nrm.hand_net(orc)
    return net, nrm.hand_store(net, crm.CHAIN, twins=True), nrm.hand_batch(net)


def by_name(batch, want, key="status"):
    out = {}
    for (name, _), x in zip(batch, want[key]):
        out.setdefault(name, x)
    return out


def check_hand_cases(net, v, batch, want, pending):
    """what the issue's named cases come to, by hand (shared with the device test)"""
    st, fl, nd = by_name(batch, want), by_name(batch, want, "flags"), by_name(batch, want, "node")
    assert sorted(set(want["status"])) == [-1, 0, 1, 2] + [3 if pending else 4] + [5, 6]
    assert (st["newer"], st["its copy"], st["stale"], st["equal to the record's"], fl["newer"]) == (0, 6, 5, 5, 1)
    assert (st["length 142"], st["length 141"], st["flen 5"]) == (0, -1, 0) and len(dict(batch)["length 142"]) == 142
    for t in range(1, 6):
        assert (st["address type %d" % t], st["address type %d cut" % t]) == (0, 1)
    assert (st["all address types"], st["type 5 of length 0"], st["type 5 cut behind its length"], st["type 5 cut behind its type"]) == (0, 0, 1, 1)
    assert (st["type 1 cut behind its type"], st["port 0"], st["unknown type, then garbage"], st["port 0 cut"]) == (1, 0, 0, 1)
    assert (st["tlv 1 of 10"], st["tlv 1 of 14"], st["tlv 1 of 9"], st["tlv 1 of 11, not minimal"], st["tlv 1 of 15"]) == (0, 0, -1, -1, -1)
    assert (st["unknown odd tlv"], st["unknown even tlv"], st["descending tlvs"], st["ascending tlvs"], st["tlv length past the end"]) == (0, -1, -1, 0, -1)
    assert st["tlv 1 of 11"] == 5                                                                # well-formed, and older than what was accepted
    assert (st["r = n"], st["s = n"], st["a signature bit"], st["a signed byte"], st["type 258"], st["empty"], st["addrlen past the end"]) == (-1, -1, 2, 2, -1, -1, -1)
    assert (st["an unsigned trailing byte"], st["id with first byte 5"], st["the twin of node 0"]) == (2, 2, 2)
    unknown = 3 if pending else 4
    assert (st["node 0's x, the other parity"], st["node 8, in no channel"]) == (unknown, unknown)
    rank = v["rank"]
    assert (nd["node 0 beside its twin"], nd["node 7 beside its twin"]) == (rank[net.node_id[0]], rank[net.node_id[7]])
    assert abs(rank[nrm.twin_of(net.node_id[0])] - rank[net.node_id[0]]) == 1 and nd["the twin of node 0"] == nrm.NONE
    assert all((n == nrm.NONE) == (s not in (0, 5, 6)) for n, s in zip(want["node"], want["status"]))
    assert (st["ts 0, record of ts 0"], st["ts 1, record of ts 0"], st["ts 2^32 - 1, a record"], st["after 2^32 - 1"]) == (6, 0, 0, 5)
    assert (st["ts 0, no record"], st["ts 0 again"], st["ts 2^32 - 1, no record"], fl["ts 0, no record"]) == (0, 6, 0, 1 | 4)
    assert (st["between signed and header"], st["the header's"], st["past the header"]) == (5, 6, 0)
    assert (fl["all channels dying, a record"], fl["and again"], fl["one live channel"], st["one live channel"]) == (1 | 4, 4, 0, 0)
    assert (st["the deleted record's"], st["the live record's"], st["past the live record"]) == (5, 6, 0)
    # the records of nodes 0, 1, 2, 3 and 6 are deleted once each, and nothing else
    assert want["del_rec"] == sorted(v["nann"][rank[net.node_id[k]]] for k in (0, 1, 2, 3, 6))


def test_every_status_and_flag_by_hand(exe, tmp_path, orc, hand):
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    assert len({len(m) % 4 for m in msgs}) == 4
    for pending in (False, True):
        v, want = check_against_model(exe, tmp_path / ("hand%d" % pending), orc, blob, msgs, pending=pending)
        check_hand_cases(net, v, batch, want, pending)
    # the same batch against the store without the twins: it passes the audit, and so does what the plan makes of it
    clean = nrm.hand_store(net, crm.CHAIN)
    v, want = check_against_model(exe, tmp_path / "clean", orc, clean, msgs)
    assert sa.model(orc, clean)[2]["clean"] == 1 and nrm.apply(clean, v, want)[:len(clean)] != clean and sa.model(orc, nrm.apply(clean, v, want))[2]["clean"] == 1
    # the oracle calls malformed what the model's parser calls malformed, for everything long enough to be looked at
    assert all((orc.sigcheck_node_announcement(m) == -1) == (nrm.parse(m) is None) for m in msgs if len(m) >= 142)


def test_orders_of_arrival(exe, tmp_path, orc, hand):
    """the same messages reversed and shuffled: other winners, the same agreement"""
    net, blob, batch = hand
    msgs = [m for _, m in batch]
    seen = set()
    for k, order in enumerate((list(range(len(msgs)))[::-1], random.Random(4).sample(range(len(msgs)), len(msgs)), random.Random(5).sample(range(len(msgs)), len(msgs)))):
        _, want = check_against_model(exe, tmp_path / ("o%d" % k), orc, blob, [msgs[i] for i in order] * 2, pending=bool(k & 1))
        assert want["status"][len(msgs):].count(0) == 0                                          # the second copy of anything is at best a duplicate
        seen.add(tuple(want["status"]))
    assert len(seen) == 3


def test_one_node_and_empty_batches(exe, tmp_path, orc, hand):
    net, blob, _ = hand
    anns = [net.nann(0, nrm.T0 - 3 + k, addrs=bytes(k % 5)) for k in range(12)]
    rnd = random.Random(9)
    batch = [rnd.choice(anns) for _ in range(300)]
    v, want = check_against_model(exe, tmp_path / "node", orc, blob, batch)
    assert set(want["status"]) == {0, 5, 6} and want["del_rec"] == [v["nann"][v["rank"][net.node_id[0]]]] and want["flags"].count(1) == want["status"].count(0) - 1
    check_against_model(exe, tmp_path / "none", orc, blob, [])
    check_against_model(exe, tmp_path / "one", orc, blob, [anns[3]])
    check_against_model(exe, tmp_path / "junk", orc, blob, [b"", b"\x01\x01", bytes(200), b"\x01\x01" + bytes(140)])
    # an image without a channel: every node is unknown
    _, empty = check_against_model(exe, tmp_path / "empty", orc, b"\x10", anns[:3], pending=True)
    assert empty["status"] == [3, 3, 3]


def test_the_synthetic_store_with_and_without_verdicts(exe, tmp_path, orc, synthetic):
    """the store a gossipd life cycle leaves behind -- deleted records, dying channels --, its nodes' announcements around their timestamps in force"""
    img, (_, ver, _) = synthetic
    net = gs.Net(orc, sa.SEED)                                                                # the network that signed it (make_script's)
    rnd = random.Random(12)
    for tag, verdict in (("plain", None), ("ok", list(ver))):
        v = nrm.view(img, verdict)
        batch = []
        for n in range(len(net.node_id)):
            r = v["rank"].get(net.node_id[n])
            base = v["ts"][r] if r is not None and v["ts"][r] is not None else gs.NOW
            batch += [net.nann(n, base + x, addrs=bytes(x + 1)) for x in (-1, 0, 1, 1, 3)]
        rnd.shuffle(batch)
        _, want = check_against_model(exe, tmp_path / tag, orc, img, batch, verdict=verdict)
        assert {0, 5, 6} <= set(want["status"]) and want["del_rec"] and any(f & 1 for f in want["flags"])


def test_the_plan_applied_equals_the_ingests_own_store(exe, tmp_path, orc):
    """closing the loop on the CPU: a GossipIngest (oracle backend, no pending state) whose store_image() is received against; the same batch
    pushed through the ingest; its image afterwards is the old image with the HEADER's plan applied (the bytes and lists the host build of
    store_nodes.h wrote), byte for byte -- and so with the model's.  The store has no dying channel: the ingest never marks a freshly received
    node_announcement DYING, the reference and this call do."""
    from lightning_amd.gossipd import GossipIngest
    net, ops = gs.make_script(orc, 21, n_ops=300)
    with GossipIngest(None, gs.CHAIN, net.our_id, net.height + 200, gs.NOW, backend=sa.oracle_backend(orc)) as ing:
        gs.drive(net, ops, ing, 21)
        ing.new_block(net.height + 400)
        ing.process()
        before = ing.store_image()
        v = nrm.view(before)
        assert len(v["ids"]) >= 5 and not any(v["dying"]) and not any(r[1] & nrm.F_DYING for r in v["recs"])
        known = [n for n in range(len(net.node_id)) if net.node_id[n] in v["rank"]]
        batch = []
        for n in known:
            r = v["rank"][net.node_id[n]]
            base = v["ts"][r] if v["ts"][r] is not None else gs.NOW
            batch += [net.nann(n, base + x, addrs=bytes(x)) for x in (0, 2, 1, 5)]
        stranger = bytes(range(1, 33))
        batch += [nrm.nann(net, stranger, net.compress(orc.pubkey_create(stranger)), gs.NOW), gs.damage(net.rnd, net.nann(known[0], gs.NOW + 50), "sig")]
        random.Random(3).shuffle(batch)
        for m in batch:
            ing.push(net.peers[1], m)
        ing.process()
        after = ing.store_image()
    check = nrm.checker(orc)
    want = nrm.receive(v, batch, check)
    got = host_run(exe, tmp_path / "ingest", before, v, batch, [(0 if check(m) else 1) if c else 1 for m, c in zip(batch, want["checked"])])
    assert got["status"].count(0) >= 8 and {2, 4, 5, 6} <= set(got["status"]) and any(x is not None for x in v["ts"]) and any(x is None for x in v["ts"])
    applied = bytearray(before)                                                              # the header's plan, applied as a caller would
    for k in got["del_rec"]:
        applied[v["recs"][k][0]] |= 0x80
    assert after == bytes(applied) + got["bytes"]
    assert after == nrm.apply(before, v, want) and got["status"] == want["status"]


def test_the_literals_of_the_reference(exe, tmp_path, orc):
    """the node_announcements of lightningd/test/run-check_node_announcement.c against an empty directory: the statuses the fixture recorded"""
    with open(os.path.join(ROOT, "tests", "golden", "node_announcements.json")) as f:
        items = json.load(f)["announcements"]
    assert len(items) == 3 and sum(i["zero_signature"] for i in items) == 1 and sum(i["tlv_bytes"] > 0 for i in items) == 1
    msgs = [bytes.fromhex(i["hex"]) for i in items]
    _, want = check_against_model(exe, tmp_path / "lit", orc, b"\x10", msgs)
    assert want["status"] == [i["status"] for i in items] == [4, 2, 4]
    assert [orc.sigcheck_node_announcement(m) for m in msgs] == [i["oracle_sigcheck"] for i in items]
    _, held = check_against_model(exe, tmp_path / "held", orc, b"\x10", msgs, pending=True)
    assert held["status"] == [3, 2, 3]


def test_new_prototype_and_binding_agree(tmp_path):
    """the prototype this header section adds has the argument count of its ctypes binding, and the summary the layout a C compiler gives it"""
    from lightning_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lightning_amd.h")).read(), flags=re.S)
    n = "lamd_node_announcement_receive_batch"
    proto = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
    assert proto, n
    res, args = _ffi.SYMBOLS[n]
    assert len(proto.group(2).split(",")) == len(args) == 18 and res is ctypes.c_int and proto.group(1) == "int"
    for text, ct in zip(proto.group(2).split(","), args):
        assert (("size_t" in text or "uint64_t" in text) and "*" not in text) == (ct in (ctypes.c_size_t, ctypes.c_uint64)), text   # (one type on LP64)
        assert (re.search(r"\bint\b", text) is not None and "*" not in text) == (ct is ctypes.c_int), text
    cls = _ffi.LamdNodeReceiveSummary
    assert [f[0] for f in cls._fields_] == ["by_status", "accepted", "superseded", "adds", "bytes", "deletions", "signature_rows", "stage_ms"]
    lines = ['  printf("%zu\\n", sizeof(lamd_node_receive_summary));\n'] + ['  printf("%%zu\\n", offsetof(lamd_node_receive_summary, %s));\n' % f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lightning_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()]
    assert out == [ctypes.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert hasattr(_ffi.load(), n)

"""The shared-service front (include/lightning_amd_served.h): lamd_served owns the engine, client processes use it through
liblightning_amd_client.so -- same C prototypes as the engine library.
CPU part: the server bound to a stub engine (tests/c/stub_engine.c: verdicts are a fixed function of the input bytes) -- framing of every
operation, requests of several client PROCESSES merged into one engine call and scattered back, error propagation, fail-closed without a server.
GPU part (-m gpu): the real engine behind the server, 8 client processes issuing BASELINE configs[4] commitments; verdicts equal the in-process
engine's and the oracle's."""
import ctypes
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 484


class Stats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("requests", "engine_calls", "merged_requests", "merged_rows", "largest_merge_requests", "clients_now", "clients_total",
                                               "flushes", "flush_rows", "engine_flushes", "largest_engine_flush_requests", "devices")] + [("rows_by_device", ctypes.c_uint64 * 8)] + \
               [("flush_rows_in_place", ctypes.c_uint64), ("pinned_blocks_now", ctypes.c_uint64)]


class TxTemplate(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint32), ("locktime", ctypes.c_uint32), ("inputs40", ctypes.c_void_p), ("n_inputs", ctypes.c_uint32),
                ("input_num", ctypes.c_uint32), ("amount_sat", ctypes.c_uint64), ("outputs", ctypes.c_void_p), ("outputs_len", ctypes.c_uint64),
                ("n_outputs", ctypes.c_uint32), ("script", ctypes.c_void_p), ("script_len", ctypes.c_uint64)]


def _client():
    from lightning_amd import _build
    L = ctypes.CDLL(_build.build_served()[1])
    L.lamd_last_error.restype = ctypes.c_char_p
    L.lamd_last_error.argtypes = [ctypes.c_void_p]
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.lamd_init.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    L.lamd_shutdown.argtypes = [vp]
    L.lamd_verify_ecdsa_batch.argtypes = [vp, sz, vp, vp, vp, sz, sz, vp]
    L.lamd_verify_schnorr_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    L.lamd_pubkey_parse_batch.argtypes = [vp, sz, vp, sz, sz, vp, vp]
    L.lamd_sigcheck_gossip_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    L.lamd_check_signed_hash.argtypes = [vp, vp, vp, vp, sz]
    L.lamd_check_schnorr_sig.argtypes = [vp, vp, vp, vp]
    L.lamd_ecdsa_recover_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.lamd_check_commitment_signed.argtypes = [vp, vp, vp, vp, ctypes.c_uint8, sz, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    L.lamd_grind_htlc_tx_fee.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint8, ctypes.c_int, vp,
                                         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
    L.lamd_client_server_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.lamd_queue_ecdsa.argtypes = [vp, vp, vp, vp, sz]
    L.lamd_queue_schnorr.argtypes = [vp, vp, vp, vp]
    L.lamd_queue_ecdsa_batch.argtypes = [vp, sz, vp, vp, vp, sz, sz]
    L.lamd_queue_schnorr_batch.argtypes = [vp, sz, vp, vp, vp]
    L.lamd_queue_reserve.argtypes = [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.lamd_flush.argtypes = [vp]
    L.lamd_poll.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.lamd_wait.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    return L


def _start(sock, engine=None, extra=()):
    from lightning_amd import _build
    exe = _build.build_served()[0]
    cmd = [exe, "--socket", sock] + (["--engine", engine] if engine else []) + list(extra) + os.environ.get("LAMD_SERVED_TEST_ARGS", "").split()
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    line = p.stdout.readline()
    if "ready" not in line:
        p.kill()
        raise RuntimeError("lamd_served did not start: %r %r" % (line, p.stderr.read()))
    p.ready_line = line
    return p


def _stop(p):
    p.terminate()
    try:
        out = p.communicate(timeout=20)[0]
    except subprocess.TimeoutExpired:
        p.kill()
        out = ""
    return out


def _short_dir():
    """a fresh private directory for unix sockets: a socket path must fit sun_path (108 bytes), and pytest's own temporary directories can lie
    deeper than that"""
    for base in (tempfile.gettempdir(), "/tmp"):
        if len(base) <= 48 and os.access(base, os.W_OK | os.X_OK):
            return tempfile.mkdtemp(prefix="lamd-", dir=base)
    raise RuntimeError("no temporary directory with a path short enough for a unix socket")


@pytest.fixture
def sockdir():
    d = _short_dir()
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """(the stub engine library, a short directory for the sockets of the stub-backed tests)"""
    so = str(tmp_path_factory.mktemp("served") / "libstub_engine.so")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "c", "stub_engine.c")])
    d = _short_dir()
    yield so, d
    shutil.rmtree(d, ignore_errors=True)


def _connect(L, sock):
    os.environ["LAMD_SERVED_SOCKET"] = sock
    ctx = ctypes.c_void_p()
    rc = L.lamd_init(ctypes.byref(ctx), 0)
    return rc, ctx


def _rows(rng, n, w):
    return np.ascontiguousarray(rng.integers(0, 256, (n, w), dtype=np.uint8))


def _commitment_from_dicts(L, ctx, commit_tx, fund33, commit_sig, commit_type, htlc_txs, hkey33, htlc_sigs, htlc_types):
    """lamd_check_commitment_signed through the client library on templates given as the dicts of tests/test_gpu_commitment.py -> (rc, first_bad, ok rows)"""
    def varint(v):
        return bytes([v]) if v < 0xfd else (b"\xfd" + v.to_bytes(2, "little") if v <= 0xffff else b"\xfe" + v.to_bytes(4, "little"))
    keep = []

    def tmpl(t):
        ins = b"".join(bytes(i[0]) + int(i[1]).to_bytes(4, "little") + int(i[2]).to_bytes(4, "little") for i in t["inputs"])
        outs = b"".join(int(a).to_bytes(8, "little") + varint(len(spk)) + bytes(spk) for a, spk in t["outputs"])
        bufs = [ctypes.create_string_buffer(x, len(x) + 1) for x in (ins, outs, bytes(t["script"]))]
        keep.extend(bufs)
        return TxTemplate(t["version"], t["locktime"], ctypes.addressof(bufs[0]), len(t["inputs"]), t.get("input_num", 0), t["amount"], ctypes.addressof(bufs[1]), len(outs),
                          len(t["outputs"]), ctypes.addressof(bufs[2]), len(t["script"]))
    n = len(htlc_txs)
    arr = (TxTemplate * (n + 1))(*([tmpl(commit_tx)] + [tmpl(t) for t in htlc_txs]))
    sigs = np.frombuffer(b"".join(htlc_sigs) + b"\x00", dtype=np.uint8).copy()
    types = np.array(list(htlc_types) + [0], dtype=np.uint8)
    fb = ctypes.c_int64(7)
    okr = np.zeros(n + 1, np.uint8)
    rc = L.lamd_check_commitment_signed(ctx, ctypes.addressof(arr), bytes(fund33), bytes(commit_sig), commit_type, n, ctypes.addressof(arr) + ctypes.sizeof(TxTemplate), bytes(hkey33),
                                        sigs.ctypes.data, types.ctypes.data, ctypes.byref(fb), okr.ctypes.data)
    return rc, fb.value, [bool(x) for x in okr]


def _stub_commitment(rng, n_htlc):
    """a random commitment (templates, keys, signatures) and the verdict rows tests/c/stub_engine.c gives them; -> (call(L, ctx) -> (rc, first_bad, ok_rows), expect)"""
    bufs, tm, expect = [], (TxTemplate * (n_htlc + 1))(), []
    sigs, types = _rows(rng, n_htlc + 1, 64), rng.choice([1, 0x83], n_htlc + 1).astype(np.uint8)
    fund, hkey = _rows(rng, 1, 33), _rows(rng, 1, 33)
    for i in range(n_htlc + 1):
        ins, outs, sc = _rows(rng, 1, 40), _rows(rng, 1, int(rng.integers(9, 60))), _rows(rng, 1, int(rng.integers(1, 140)))
        bufs += [ins, outs, sc]
        tm[i] = TxTemplate(int(rng.integers(1, 3)), int(rng.integers(0, 1 << 30)), ins.ctypes.data, 1, 0, int(rng.integers(1, 1 << 40)), outs.ctypes.data, outs.shape[1], 1,
                           sc.ctypes.data, sc.shape[1])
        key = fund if i == 0 else hkey
        expect.append(int((tm[i].version ^ tm[i].amount_sat ^ int(types[i]) ^ int(sigs[i, 0]) ^ int(key[0, 1]) ^ int(ins[0, 0]) ^ int(outs[0, -1]) ^ int(sc[0, 0])) & 1))

    def call(L, ctx):
        fb = ctypes.c_int64(7)
        okr = np.zeros(n_htlc + 1, np.uint8)
        rc = L.lamd_check_commitment_signed(ctx, ctypes.addressof(tm), fund.ctypes.data, sigs[0].ctypes.data, int(types[0]), n_htlc, ctypes.addressof(tm) + ctypes.sizeof(TxTemplate),
                                            hkey.ctypes.data, sigs[1:].ctypes.data if n_htlc else None, types[1:].ctypes.data if n_htlc else None, ctypes.byref(fb), okr.ctypes.data)
        return rc, fb.value, list(okr)
    call.keep = (bufs, tm, sigs, types, fund, hkey)
    return call, expect


def test_every_operation_round_trips_through_the_server(stub):
    so, d = stub
    sock = os.path.join(d, "a.sock")
    p = _start(sock, so)
    L = _client()
    try:
        rc, ctx = _connect(L, sock)
        assert rc == 0, L.lamd_last_error(ctx)
        rng = np.random.default_rng(1)
        for n, kl in ((1, 33), (484, 33), (5000, 65), (70000, 65)):      # the last one outgrows the first shared block: the client re-attaches a bigger one
            h, s, k = _rows(rng, n, 32), _rows(rng, n, 64), _rows(rng, n, kl)
            ok = np.full(n, 9, np.uint8)
            assert L.lamd_verify_ecdsa_batch(ctx, n, h.ctypes.data, s.ctypes.data, k.ctypes.data, kl, kl, ok.ctypes.data) == 0, L.lamd_last_error(ctx)
            assert np.array_equal(ok, (h[:, 0] ^ s[:, 63] ^ k[:, kl - 1]) & 1)
        # a strided key array is packed by the client
        h, s, k = _rows(rng, 50, 32), _rows(rng, 50, 64), _rows(rng, 50, 80)
        ok = np.zeros(50, np.uint8)
        assert L.lamd_verify_ecdsa_batch(ctx, 50, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 80, ok.ctypes.data) == 0
        assert np.array_equal(ok, (h[:, 0] ^ s[:, 63] ^ k[:, 32]) & 1)
        m, x, sg = _rows(rng, 300, 32), _rows(rng, 300, 32), _rows(rng, 300, 64)
        ok = np.zeros(300, np.uint8)
        assert L.lamd_verify_schnorr_batch(ctx, 300, m.ctypes.data, x.ctypes.data, sg.ctypes.data, ok.ctypes.data) == 0
        assert np.array_equal(ok, (m[:, 1] ^ x[:, 2] ^ sg[:, 3]) & 1)
        # single-item veneers: 1 / 0, the BIP-340 one drops the parity byte of the 33-byte key
        assert L.lamd_check_signed_hash(ctx, h[0].ctypes.data, s[0].ctypes.data, k[0].ctypes.data, 33) == int((h[0, 0] ^ s[0, 63] ^ k[0, 32]) & 1)
        k33 = _rows(rng, 1, 33)
        assert L.lamd_check_schnorr_sig(ctx, m[0].ctypes.data, k33.ctypes.data, sg[0].ctypes.data) == int((m[0, 1] ^ k33[0, 3] ^ sg[0, 3]) & 1)
        # key parse: two output sections
        pk = _rows(rng, 40, 33)
        pk[:, 0] = rng.integers(1, 6, 40)
        xy, ok = np.zeros((40, 64), np.uint8), np.zeros(40, np.uint8)
        assert L.lamd_pubkey_parse_batch(ctx, 40, pk.ctypes.data, 33, 33, xy.ctypes.data, ok.ctypes.data) == 0
        assert np.array_equal(ok, np.isin(pk[:, 0], (2, 3, 4)).astype(np.uint8)) and np.array_equal(xy[:, :32], pk[:, 1:33])
        assert L.lamd_pubkey_parse_batch(ctx, 40, pk.ctypes.data, 33, 33, None, ok.ctypes.data) == 0
        # gossip: blob + offsets (made relative by the client) + node ids
        lens = rng.integers(3, 500, 60)
        blob = _rows(rng, int(lens.sum()) + 7, 1).reshape(-1)
        off = (np.concatenate([[0], np.cumsum(lens)]) + 7).astype(np.uint64)
        ids = _rows(rng, 60, 33)
        v = np.zeros(60, np.int8)
        assert L.lamd_sigcheck_gossip_batch(ctx, 60, blob.ctypes.data, off.ctypes.data, ids.ctypes.data, v.ctypes.data) == 0
        assert np.array_equal(v, ((blob[off[:-1].astype(np.int64) + 2] & 3) + (ids[:, 0] & 1)).astype(np.int8))
        # recovery
        rid = rng.integers(0, 4, 30).astype(np.uint8)
        pub, ok = np.zeros((30, 33), np.uint8), np.zeros(30, np.uint8)
        hh, ss = _rows(rng, 30, 32), _rows(rng, 30, 64)
        assert L.lamd_ecdsa_recover_batch(ctx, 30, hh.ctypes.data, ss.ctypes.data, rid.ctypes.data, pub.ctypes.data, ok.ctypes.data) == 0
        assert np.array_equal(pub[:, 1:], hh ^ ss[:, :32]) and np.array_equal(pub[:, 0], 2 + (rid & 1)) and ok.all()
        # one commitment_signed: templates flattened by the client, rebuilt by the server
        for n_htlc in (483, 0, 7):
            call, expect = _stub_commitment(rng, n_htlc)
            rc, fb, okr = call(L, ctx)
            assert rc == 0, L.lamd_last_error(ctx)
            assert okr == expect and fb == (expect.index(0) if 0 in expect else -1)
        sigs, fund = call.keep[2], call.keep[4]
        # grind: scalars in the header, the answer in the reply's rc
        pre, outs = _rows(rng, 1, 290), _rows(rng, 1, 43)
        rate, fee = ctypes.c_uint32(0), ctypes.c_uint64(0)
        assert L.lamd_grind_htlc_tx_fee(ctx, pre.ctypes.data, 290, outs.ctypes.data, 43, 700000, 663, 100, 250000, sigs[0].ctypes.data, 1, 1, fund.ctypes.data,
                                        ctypes.byref(rate), ctypes.byref(fee)) == 1
        assert rate.value == 100 + (290 + 43) % (250000 - 100 + 1) and fee.value == rate.value * 663 // 1000 + 700000 % 7
        assert L.lamd_grind_htlc_tx_fee(ctx, pre.ctypes.data, 290, outs.ctypes.data, 43, 700000, 663, 100, 250000, sigs[0].ctypes.data, 1, 0, fund.ctypes.data,
                                        ctypes.byref(rate), ctypes.byref(fee)) == 0
        # an engine error travels back with its text; the connection stays usable
        h = _rows(rng, 4, 32)
        h[0, :2] = 0xEE
        ok = np.zeros(4, np.uint8)
        assert L.lamd_verify_ecdsa_batch(ctx, 4, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 80, ok.ctypes.data) == -2
        assert b"poisoned" in L.lamd_last_error(ctx)
        st = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st)) == 0 and st.clients_now == 1 and st.requests >= 15
        L.lamd_shutdown(ctx)
    finally:
        _stop(p)


CLIENT_SCRIPT = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_served as T
L = T._client()
rc, ctx = T._connect(L, sys.argv[2])
assert rc == 0, L.lamd_last_error(ctx)
rng = np.random.default_rng(int(sys.argv[3]))
bad = 0
for it in range(int(sys.argv[4])):
    n = T.PER
    h, s, k = T._rows(rng, n, 32), T._rows(rng, n, 64), T._rows(rng, n, 33)
    ok = np.full(n, 9, np.uint8)
    assert L.lamd_verify_ecdsa_batch(ctx, n, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33, ok.ctypes.data) == 0
    bad += int((ok != ((h[:, 0] ^ s[:, 63] ^ k[:, 32]) & 1)).sum())
    if it % 2 == 0:   # a commitment_signed validation: merged with the other clients' into one check_tx_sig batch on the server
        call, expect = T._stub_commitment(rng, int(rng.integers(0, 40)))
        rc, fb, okr = call(L, ctx)
        assert rc == 0, L.lamd_last_error(ctx)
        bad += int(okr != expect) + int(fb != (expect.index(0) if 0 in expect else -1))
    if it % 5 == 0:
        m, x, sg = T._rows(rng, 64, 32), T._rows(rng, 64, 32), T._rows(rng, 64, 64)
        ok = np.zeros(64, np.uint8)
        assert L.lamd_verify_schnorr_batch(ctx, 64, m.ctypes.data, x.ctypes.data, sg.ctypes.data, ok.ctypes.data) == 0
        bad += int((ok != ((m[:, 1] ^ x[:, 2] ^ sg[:, 3]) & 1)).sum())
L.lamd_shutdown(ctx)
print("bad", bad)
"""


def test_requests_of_eight_client_processes_are_merged_and_scattered_back(stub):
    so, d = stub
    sock = os.path.join(d, "b.sock")
    p = _start(sock, so, ["--linger-us", "300"])
    try:
        procs = [subprocess.Popen([sys.executable, "-c", CLIENT_SCRIPT, ROOT, sock, str(100 + i), "40"], stdout=subprocess.PIPE, text=True) for i in range(8)]
        outs = [q.communicate(timeout=120)[0] for q in procs]
        assert all(q.returncode == 0 for q in procs) and all(o.strip().endswith("bad 0") for o in outs), outs
        L = _client()
        rc, ctx = _connect(L, sock)
        assert rc == 0
        st = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st)) == 0
        L.lamd_shutdown(ctx)
        # 8 x (40 + 20 + 8) requests; with eight clients waiting at once most of them travelled in merged calls
        assert st.clients_total == 9 and st.requests >= 8 * 68
        assert st.merged_requests >= 100 and st.largest_merge_requests >= 3 and st.engine_calls < st.requests
    finally:
        out = _stop(p)
    assert "requests" in out


def _stub_ecdsa(h, s, k):
    return (h[:, 0] ^ s[:, 63] ^ k[:, -1]) & 1


def _stub_schnorr(m, x, s):
    return (m[:, 1] ^ x[:, 2] ^ s[:, 3]) & 1


def _queue_mixed(L, ctx, rng, sizes=(40, 17, 9)):
    """one open set of mixed kinds (ECDSA-33 batch, BIP-340 batch, ECDSA-65 batch, one single ECDSA-33 triple) -> expected verdicts in ticket order"""
    n33, ns, n65 = sizes
    exp, keep = [], []
    h, s, k = _rows(rng, n33, 32), _rows(rng, n33, 64), _rows(rng, n33, 33)
    assert L.lamd_queue_ecdsa_batch(ctx, n33, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0
    exp.append(_stub_ecdsa(h, s, k))
    m, x, sg = _rows(rng, ns, 32), _rows(rng, ns, 32), _rows(rng, ns, 64)
    assert L.lamd_queue_schnorr_batch(ctx, ns, m.ctypes.data, x.ctypes.data, sg.ctypes.data) == n33
    exp.append(_stub_schnorr(m, x, sg))
    h2, s2, k2 = _rows(rng, n65, 32), _rows(rng, n65, 64), _rows(rng, n65, 80)          # 65-byte keys at a stride of 80
    assert L.lamd_queue_ecdsa_batch(ctx, n65, h2.ctypes.data, s2.ctypes.data, k2.ctypes.data, 65, 80) == n33 + ns
    exp.append(_stub_ecdsa(h2, s2, k2[:, :65]))
    h3, s3, k3 = _rows(rng, 1, 32), _rows(rng, 1, 64), _rows(rng, 1, 33)
    assert L.lamd_queue_ecdsa(ctx, h3.ctypes.data, s3.ctypes.data, k3.ctypes.data, 33) == n33 + ns + n65
    exp.append(_stub_ecdsa(h3, s3, k3))
    return np.concatenate(exp)


def _collect(L, ctx, cap, block=True):
    ok, n = np.full(cap, 9, np.uint8), ctypes.c_size_t(0)
    if block:
        rc = L.lamd_wait(ctx, ok.ctypes.data, cap, ctypes.byref(n))
    else:
        for _ in range(20000):
            rc = L.lamd_poll(ctx, ok.ctypes.data, cap, ctypes.byref(n))
            if rc != 0:
                break
            time.sleep(0.0005)
    return rc, ok[:n.value]


def test_streaming_flushes_keep_their_order_and_their_rows(stub):
    """round 6: lamd_queue_* / lamd_flush / lamd_poll / lamd_wait over the service, three (stub) devices behind it"""
    so, d = stub
    sock = os.path.join(d, "s.sock")
    p = _start(sock, so, ["--devices", "0,1,2"])
    # every device's engine thread lives on the NUMA node its device hangs on, where the engine library knows it (the stub: node 0 for devices 0 and 1,
    # unknown for device 2); --no-numa leaves the threads alone
    assert "device 0 on NUMA node 0, device 1 on NUMA node 0" in p.ready_line and "device 2 on NUMA" not in p.ready_line, p.ready_line
    q = _start(sock + ".nn", so, ["--devices", "0,1", "--no-numa"])
    assert "NUMA" not in q.ready_line
    _stop(q)
    try:
        L = _client()
        rc, ctx = _connect(L, sock)
        assert rc == 0, L.lamd_last_error(ctx)
        rng = np.random.default_rng(77)
        ok1 = np.zeros(8, np.uint8)
        n = ctypes.c_size_t(0)
        assert L.lamd_wait(ctx, ok1.ctypes.data, 8, ctypes.byref(n)) == -5 and b"no flush" in L.lamd_last_error(ctx)      # nothing outstanding
        assert L.lamd_flush(ctx) == 0                                                                                        # an empty set is no flush
        # eight flushes outstanding, the ninth is refused until one is collected; every flush comes back in submission order with ITS rows
        exps = []
        for f in range(8):
            exps.append(_queue_mixed(L, ctx, rng, (40 + f, 17, 9)))
            assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
        extra = _queue_mixed(L, ctx, rng)
        assert L.lamd_flush(ctx) == -5 and b"outstanding" in L.lamd_last_error(ctx)
        # a synchronous call between a flush and its collection gets ITS answer
        h, s, k = _rows(rng, 30, 32), _rows(rng, 30, 64), _rows(rng, 30, 33)
        oks = np.full(30, 9, np.uint8)
        assert L.lamd_verify_ecdsa_batch(ctx, 30, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33, oks.ctypes.data) == 0 and np.array_equal(oks, _stub_ecdsa(h, s, k))
        for f in range(8):
            rc, got = _collect(L, ctx, 4096, block=(f % 2 == 0))
            assert rc == 1 and np.array_equal(got, exps[f]), (f, rc, L.lamd_last_error(ctx))
            if f == 0:
                assert L.lamd_flush(ctx) == 0          # the ninth set, queued above, goes out now that a block is free
        rc, got = _collect(L, ctx, 4096)
        assert rc == 1 and np.array_equal(got, extra)
        # too small a verdict buffer is the caller's error, and the flush stays collectable
        exp = _queue_mixed(L, ctx, rng)
        assert L.lamd_flush(ctx) == 0
        assert _collect(L, ctx, 3)[0] == -3
        rc, got = _collect(L, ctx, 4096)
        assert rc == 1 and np.array_equal(got, exp)
        # the producer form: rows written in place
        ph, ps, pk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        assert L.lamd_queue_reserve(ctx, 25, 33, ctypes.byref(ph), ctypes.byref(ps), ctypes.byref(pk)) == 0
        h, s, k = _rows(rng, 25, 32), _rows(rng, 25, 64), _rows(rng, 25, 33)
        ctypes.memmove(ph, h.ctypes.data, h.nbytes); ctypes.memmove(ps, s.ctypes.data, s.nbytes); ctypes.memmove(pk, k.ctypes.data, k.nbytes)
        assert L.lamd_flush(ctx) == 0
        rc, got = _collect(L, ctx, 64)
        assert rc == 1 and np.array_equal(got, _stub_ecdsa(h, s, k))
        # an engine error inside a flush is that flush's: the next one is fine
        h, s, k = _rows(rng, 5, 32), _rows(rng, 5, 64), _rows(rng, 5, 33)
        h[0, 0] = h[0, 1] = 0xEE
        assert L.lamd_queue_ecdsa_batch(ctx, 5, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0 and L.lamd_flush(ctx) == 0
        exp = _queue_mixed(L, ctx, rng)
        assert L.lamd_flush(ctx) == 0
        assert _collect(L, ctx, 64)[0] == -2 and b"poisoned" in L.lamd_last_error(ctx)
        rc, got = _collect(L, ctx, 4096)
        assert rc == 1 and np.array_equal(got, exp)
        # a block grows with the flush it has to carry (3 MB of rows in one set)
        big = 20000
        h, s, k = _rows(rng, big, 32), _rows(rng, big, 64), _rows(rng, big, 33)
        assert L.lamd_queue_ecdsa_batch(ctx, big, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0 and L.lamd_flush(ctx) == 0
        rc, got = _collect(L, ctx, big)
        assert rc == 1 and np.array_equal(got, _stub_ecdsa(h, s, k))
        # key affinity: flushes that begin with the SAME key meet the same device; other keys spread over the devices
        st0 = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st0)) == 0 and st0.devices == 3
        key = _rows(rng, 1, 33)
        for f in range(12):
            h, s = _rows(rng, 10, 32), _rows(rng, 10, 64)
            k = np.repeat(key, 10, axis=0)
            assert L.lamd_queue_ecdsa_batch(ctx, 10, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0 and L.lamd_flush(ctx) == 0
            rc, got = _collect(L, ctx, 16)
            assert rc == 1 and np.array_equal(got, _stub_ecdsa(h, s, k))
        st1 = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st1)) == 0
        grew = [st1.rows_by_device[i] - st0.rows_by_device[i] for i in range(3)]
        assert sorted(grew) == [0, 0, 120], grew
        for f in range(30):
            h, s, k = _rows(rng, 4, 32), _rows(rng, 4, 64), _rows(rng, 4, 33)
            assert L.lamd_queue_ecdsa_batch(ctx, 4, h.ctypes.data, s.ctypes.data, k.ctypes.data, 33, 33) == 0 and L.lamd_flush(ctx) == 0
            assert _collect(L, ctx, 16)[0] == 1
        st2 = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st2)) == 0
        assert sum(1 for i in range(3) if st2.rows_by_device[i] > st1.rows_by_device[i]) >= 2
        assert st2.flushes == 8 + 1 + 1 + 1 + 2 + 1 + 12 + 30 and st2.engine_flushes <= st2.flushes and st2.flush_rows >= big
        # every flush block was pinned when it was attached and its rows were queued in place (the stub computes their verdicts from the block when the
        # flush is collected, and refuses in-place rows outside registered memory); the poisoned flush's rows never got that far
        assert st2.pinned_blocks_now >= 1 and 0 < st2.flush_rows - st2.flush_rows_in_place <= 64
        L.lamd_shutdown(ctx)
    finally:
        out = _stop(p)
    assert "engine flushes" in out


STREAM_CLIENT_SCRIPT = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_served as T
L = T._client()
rc, ctx = T._connect(L, sys.argv[2])
assert rc == 0, L.lamd_last_error(ctx)
rng = np.random.default_rng(int(sys.argv[3]))
bad, pend = 0, []
for it in range(int(sys.argv[4])):
    pend.append(T._queue_mixed(L, ctx, rng, (int(rng.integers(1, 300)), int(rng.integers(1, 50)), int(rng.integers(1, 20)))))
    assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
    if len(pend) == 6:
        rc, got = T._collect(L, ctx, 4096, block=bool(it & 1))
        bad += int(rc != 1 or not np.array_equal(got, pend.pop(0)))
while pend:
    rc, got = T._collect(L, ctx, 4096)
    bad += int(rc != 1 or not np.array_equal(got, pend.pop(0)))
L.lamd_shutdown(ctx)
print("bad", bad)
"""


@pytest.mark.parametrize("mode", ["in_place", "copy_flushes", "runtime_refuses_to_pin"])
def test_streams_of_eight_client_processes_share_the_engine_flushes(stub, mode, monkeypatch):
    """... with the flush rows queued in place from the clients' pinned blocks (the default), copied (--copy-flushes), and copied because the runtime
    refuses to pin a block (the fallback): the same verdicts"""
    so, d = stub
    sock = os.path.join(d, "t_%s.sock" % mode)
    if mode == "runtime_refuses_to_pin":
        monkeypatch.setenv("STUB_REFUSE_REGISTER", "1")
    p = _start(sock, so, ["--devices", "0,1"] + (["--copy-flushes"] if mode == "copy_flushes" else []))
    try:
        procs = [subprocess.Popen([sys.executable, "-c", STREAM_CLIENT_SCRIPT, ROOT, sock, str(300 + i), "60"], stdout=subprocess.PIPE, text=True) for i in range(8)]
        outs = [q.communicate(timeout=180)[0] for q in procs]
        assert all(q.returncode == 0 for q in procs) and all(o.strip().endswith("bad 0") for o in outs), outs
        L = _client()
        rc, ctx = _connect(L, sock)
        assert rc == 0
        st = Stats()
        for _ in range(100):      # the server lets go of a client's blocks when it sees the connection close: a moment after the process has gone
            assert L.lamd_client_server_stats(ctx, ctypes.byref(st)) == 0
            if st.pinned_blocks_now == 0 and st.clients_now == 1:
                break
            time.sleep(0.05)
        L.lamd_shutdown(ctx)
        assert st.flushes == 8 * 60 and st.engine_flushes <= st.flushes and st.rows_by_device[0] > 0 and st.rows_by_device[1] > 0
        assert st.rows_by_device[0] + st.rows_by_device[1] == st.flush_rows
        assert st.flush_rows_in_place == (st.flush_rows if mode == "in_place" else 0) and st.pinned_blocks_now == 0     # the clients are gone: nothing stays pinned
    finally:
        _stop(p)


def test_without_a_server_everything_fails_closed(stub, sockdir):
    L = _client()
    rc, ctx = _connect(L, os.path.join(sockdir, "nobody.sock"))
    assert rc == -1 and b"no lamd_served" in L.lamd_last_error(ctx)
    L.lamd_shutdown(ctx)
    # ... and so does the mirror built on the client library: check_signed_hash() is false, sigcheck_* returns an "engine error" string
    from lightning_amd import _build
    shim = ctypes.CDLL(_build.build_served()[2])
    shim.lamd_shim_setup.restype = ctypes.c_bool
    shim.check_signed_hash.restype = ctypes.c_bool
    shim.lamd_shim_last_error.restype = ctypes.c_char_p
    assert shim.lamd_shim_setup() is False and b"no lamd_served" in shim.lamd_shim_last_error()
    buf = ctypes.create_string_buffer(64)
    assert shim.check_signed_hash(buf, buf, buf) is False
    # a server whose engine has no device does not come up at all (there is no CPU verification to serve)
    so, d = stub
    from lightning_amd import _build as b2
    r = subprocess.run([b2.build_served()[0], "--socket", os.path.join(d, "c.sock"), "--engine", so, "--device", "99"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and "lamd_init" in r.stderr


def test_the_client_trusts_only_a_server_of_its_own_user_and_there_is_no_default_under_tmp(stub, sockdir):
    """whoever binds a world-writable path first would answer every check with "good".  No default path outside LAMD_SERVED_SOCKET /
    XDG_RUNTIME_DIR; the client checks SO_PEERCRED and the socket file's owner; the server binds 0600 from the start, does not replace a path it does
    not own, and a raw PUBKEY_PARSE with a bad key length fails instead of answering rc 0 with stale bytes."""
    so, d = stub
    from lightning_amd import _build
    served = _build.build_served()[0]
    L = _client()
    # no socket path at all: neither side invents one
    env = {k: v for k, v in os.environ.items() if k not in ("LAMD_SERVED_SOCKET", "XDG_RUNTIME_DIR")}
    r = subprocess.run([served, "--engine", so], capture_output=True, text=True, timeout=30, env=env)
    assert r.returncode == 2 and "LAMD_SERVED_SOCKET" in r.stderr
    code = ("import ctypes,sys; L=ctypes.CDLL(sys.argv[1]); L.lamd_last_error.restype=ctypes.c_char_p; c=ctypes.c_void_p(); "
            "rc=L.lamd_init(ctypes.byref(c),0); print(rc, L.lamd_last_error(c).decode())")
    r = subprocess.run([sys.executable, "-c", code, _build.build_served()[1]], capture_output=True, text=True, timeout=30, env=env)
    assert r.stdout.startswith("-1 ") and "LAMD_SERVED_SOCKET" in r.stdout
    # XDG_RUNTIME_DIR is the default's home
    sock = os.path.join(sockdir, "lamd_served.sock")
    env2 = dict(env, XDG_RUNTIME_DIR=sockdir)
    p = subprocess.Popen([served, "--engine", so], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env2)
    try:
        assert "ready on " + sock in p.stdout.readline()
        assert (os.stat(sock).st_mode & 0o777) == 0o600
        r = subprocess.run([sys.executable, "-c", code, _build.build_served()[1]], capture_output=True, text=True, timeout=30, env=env2)
        assert r.stdout.startswith("0 "), r.stdout + r.stderr
        # a client that expects its server under another uid refuses this one before sending a row
        r = subprocess.run([sys.executable, "-c", code, _build.build_served()[1]], capture_output=True, text=True, timeout=30,
                           env=dict(env2, LAMD_SERVED_UID=str(os.geteuid() + 1)))
        assert r.stdout.startswith("-1 ") and "refusing to trust" in r.stdout
        # PUBKEY_PARSE with a key length the engine does not know: an error, not rc 0 over stale output bytes (raw request, as a foreign client would send it)
        rc, ctx = _connect(L, sock)
        assert rc == 0
        ok = np.full(4, 1, np.uint8)
        xy = np.zeros((4, 64), np.uint8)
        keys = np.zeros((4, 40), np.uint8)
        assert L.lamd_pubkey_parse_batch(ctx, 4, keys.ctypes.data, 40, 40, xy.ctypes.data, ok.ctypes.data) == -3          # the client refuses it itself ...
        import socket as pysock, struct
        raw = pysock.socket(pysock.AF_UNIX, pysock.SOCK_STREAM)
        raw.connect(sock)
        fd = os.memfd_create("blk")
        os.ftruncate(fd, 1 << 16)
        hdr = lambda op, n, scalar0, lens: struct.pack("<IIQ6Q I 4x 20Q".replace(" ", ""), 0x4C414D44, op, n, scalar0, 0, 0, 0, 0, 0, len(lens), *(list(lens) + [0] * (20 - len(lens))))
        pysock.send_fds(raw, [hdr(1, 0, 1 << 16, [])], [fd])
        rep = raw.recv(4096)
        assert struct.unpack_from("<Ii", rep)[1] == 0
        raw.sendall(hdr(4, 4, 40, [160]))               # ... and the server answers a raw one with LAMD_ERR_ARG
        rep = raw.recv(4096)
        assert struct.unpack_from("<Ii", rep) == (0x4C414D44, -3) and b"publen" in rep
        raw.close()
        os.close(fd)
        L.lamd_shutdown(ctx)
    finally:
        _stop(p)
    # a path that exists and is not a socket of this user is not replaced
    victim = pathlib.Path(sockdir) / "notasocket"
    victim.write_text("x")
    r = subprocess.run([served, "--engine", so, "--socket", str(victim)], capture_output=True, text=True, timeout=30, env=env)
    assert r.returncode == 1 and "not replacing" in r.stderr and victim.read_text() == "x"


GPU_CLIENT_SCRIPT = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_served as T
L = T._client()
rc, ctx = T._connect(L, sys.argv[2])
assert rc == 0, L.lamd_last_error(ctx)
d = np.load(sys.argv[3])
h, s, k, e = d["h"], d["s"], d["k"], d["e"]
bad = 0
sys.path.insert(0, os.path.join(sys.argv[1], "oracle"))
import json, test_gpu_commitment as C
kat = json.load(open(os.path.join(sys.argv[1], "tests", "golden", "kat.json")))
ctx_tx, fund, csig, htxs, hkey, hsigs, _, _ = C._bolt3(kat)
for rep in range(int(sys.argv[4])):
    # the BOLT #3 commitment the reference holds signed, all good and with HTLC (rep % 5) damaged: merged with the other clients' on the server
    for sigs, want in ((hsigs, -1), (hsigs[:rep % 5] + [C._flip(hsigs[rep % 5])] + hsigs[rep % 5 + 1:], 1 + rep % 5)):
        rc, fb, okr = T._commitment_from_dicts(L, ctx, ctx_tx, fund, csig, 1, htxs, hkey, sigs, [1] * 5)
        assert rc == 0, L.lamd_last_error(ctx)
        bad += int(fb != want) + int(okr != [i != want for i in range(6)])
    for a in range(0, len(h), T.PER):
        z = min(len(h), a + T.PER)
        ok = np.full(z - a, 9, np.uint8)
        assert L.lamd_verify_ecdsa_batch(ctx, z - a, h[a:z].ctypes.data, s[a:z].ctypes.data, k[a:z].ctypes.data, 33, 33, ok.ctypes.data) == 0, L.lamd_last_error(ctx)
        bad += int((ok != e[a:z]).sum())
L.lamd_shutdown(ctx)
print("bad", bad)
"""


@pytest.mark.gpu
def test_eight_client_processes_share_one_engine(orc, kat, tmp_path, sockdir):
    """the real engine behind lamd_served: 8 client processes, each validating its own channels' commitments (1 + 483 signatures per request, the htlc key
    recurring) -- every verdict equals the oracle's, the server merged concurrent requests into shared launches, and the mirror over the client
    library (liblightning_amd_cln_client.so) gives the reference's answers"""
    sock = os.path.join(sockdir, "gpu.sock")
    p = _start(sock)
    try:
        files = []
        for i in range(8):
            n = PER * 6
            h, s, k, c, e = orc.gen_ecdsa_edge_batch(0x5E12 + i, n, 33, 4)
            # commitments: the 483 HTLC rows of a request under ONE key (rows re-signed is not possible here, so the expected verdict follows the oracle)
            f = str(tmp_path / ("rows%d.npz" % i))
            np.savez(f, h=h, s=s, k=k, e=e.astype(np.uint8))
            files.append(f)
        procs = [subprocess.Popen([sys.executable, "-c", GPU_CLIENT_SCRIPT, ROOT, sock, files[i], "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(8)]
        outs = [q.communicate(timeout=300) for q in procs]
        assert all(q.returncode == 0 for q in procs), [o[1][-400:] for o in outs]
        assert all(o[0].strip().endswith("bad 0") for o in outs), [o[0] for o in outs]
        L = _client()
        rc, ctx = _connect(L, sock)
        assert rc == 0
        st = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(st)) == 0
        assert st.requests >= 8 * 18 and st.merged_requests > 0 and st.engine_calls < st.requests
        # goldens through the client: ECDSA, BIP-340, a reference-signed gossip message
        H = bytes.fromhex
        for v in [v for v in kat["ecdsa"] if len(v["pub"]) == 66][:40]:
            assert L.lamd_check_signed_hash(ctx, H(v["hash"]), H(v["sig"]), H(v["pub"]), 33) == int(v["expect"]), v["name"]
        for v in kat["schnorr"][:15]:
            ok = np.zeros(1, np.uint8)
            assert L.lamd_verify_schnorr_batch(ctx, 1, H(v["msg"]), H(v["pk"]), H(v["sig"]), ok.ctypes.data) == 0
            assert bool(ok[0]) == v["expect"], v["name"]
        L.lamd_shutdown(ctx)
        # the mirror over the client library: the reference's unit-test expectation (gossipd/test/run-check_channel_announcement.c:84-85)
        from lightning_amd import _build
        from test_cln_shim import _cann_args, _cann_call
        shim = ctypes.CDLL(_build.build_served()[2])
        for nme in ("lamd_shim_setup", "pubkey_from_der", "fromwire_secp256k1_ecdsa_signature"):
            getattr(shim, nme).restype = ctypes.c_bool
        shim.sigcheck_channel_announcement_len.restype = ctypes.c_char_p
        shim.sigcheck_channel_announcement_len.argtypes = [ctypes.c_void_p] * 10 + [ctypes.c_size_t]
        shim.lamd_shim_last_error.restype = ctypes.c_char_p
        assert shim.lamd_shim_setup(), shim.lamd_shim_last_error()
        m = H(next(v for v in kat["gossip"] if v["name"] == "KAT-G/orig")["msg"])
        sigs, ids, keys = _cann_args(shim, m)
        err = _cann_call(shim, sigs, ids, keys, m)
        assert err is not None and err.startswith(b"Bad node_signature_1 3044022011effc9ed10f")
        good = H(next(v for v in kat["gossip"] if v["kind"] == "channel_announcement" and v["expect"] == 0)["msg"])
        sigs, ids, keys = _cann_args(shim, good)
        assert _cann_call(shim, sigs, ids, keys, good) is None
    finally:
        _stop(p)


GPU_STREAM_CLIENT_SCRIPT = r"""
import ctypes, os, sys, time, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_served as T
L = T._client()
rc, ctx = T._connect(L, sys.argv[2])
assert rc == 0, L.lamd_last_error(ctx)
d = np.load(sys.argv[3])
per_flush, depth, go = int(sys.argv[4]) * T.PER, int(sys.argv[5]), sys.argv[6]
kinds = [(d["eh"], d["es"], d["ek"], d["ee"], 33), (d["sm"], d["sk"], d["ss"], d["se"], 32)]
jobs = []
for ki, (a, b, c, e, kl) in enumerate(kinds):
    for o in range(0, len(a), per_flush):
        jobs.append((o / max(1, len(a)), ki, o, min(len(a), o + per_flush)))
jobs.sort()
def run():
    bad, pend, rows = 0, [], 0
    ok, n = np.zeros(per_flush, np.uint8), ctypes.c_size_t(0)
    def collect():
        nonlocal bad
        e = pend.pop(0)
        rc = L.lamd_wait(ctx, ok.ctypes.data, per_flush, ctypes.byref(n))
        bad += int(rc != 1 or n.value != len(e) or not np.array_equal(ok[:n.value], e))
    for _, ki, o, z in jobs:
        a, b, c, e, kl = kinds[ki]
        if kl == 33:
            assert L.lamd_queue_ecdsa_batch(ctx, z - o, a[o:z].ctypes.data, b[o:z].ctypes.data, c[o:z].ctypes.data, 33, 33) == 0, L.lamd_last_error(ctx)
        else:
            assert L.lamd_queue_schnorr_batch(ctx, z - o, a[o:z].ctypes.data, b[o:z].ctypes.data, c[o:z].ctypes.data) == 0, L.lamd_last_error(ctx)
        assert L.lamd_flush(ctx) == 0, L.lamd_last_error(ctx)
        pend.append(e[o:z])
        rows += z - o
        if len(pend) == depth:
            collect()
    while pend:
        collect()
    return bad, rows
bad0, _ = run()                      # first pass: blocks attached, staging sets and lane workspaces allocated
open(go + ".ready%s" % sys.argv[7], "w").close()
while not os.path.exists(go):
    time.sleep(0.0005)
t0 = time.time()
bad, rows = run()
t1 = time.time()
L.lamd_shutdown(ctx)
print("bad %d rows %d t0 %.6f t1 %.6f" % (bad0 + bad, rows, t0, t1))
"""


@pytest.mark.gpu
def test_eight_client_processes_stream_their_commitments_through_the_service(tmp_path, sockdir):
    """VERDICT r05 "next" 8: BASELINE configs[4] as channelds see it -- 8 client processes, each STREAMING its channels' commitments (flushes kept in
    flight: lamd_queue_*_batch / lamd_flush / lamd_wait of the client library) through ONE lamd_served.  Every verdict equals construction (= the
    in-process engine's, checked on the same rows), and the rate of the whole job is compared with the same job streamed by one in-process
    producer (the ratio lands in gpurun_out/served_stream.json: median 0.84 with the flush rows queued in place from the clients' pinned blocks and the engine threads on their GPU's NUMA node (0.74 with
    --no-numa, 0.63 with --copy-flushes), profiles/r06_served_stream.txt; asserted >= 0.4 -- the box's host cores decide the rest)."""
    import json
    import torch
    from lightning_amd import Engine, workload
    NCH, CPF, DEPTH, W = 4000, 64, 6, 8
    eng = Engine(0)
    try:
        st = workload.make_commit_storm(eng, NCH, device="cuda:0")
        per = st["per"]
        assert per == PER
        # in-process: the same flushes (64 commitments each), the two kinds interleaved, DEPTH in flight
        def inproc(inplace=False):
            jobs = []
            for kind in ("ecdsa", "schnorr"):
                wl = st[kind]
                for o in range(0, wl.n, CPF * per):
                    jobs.append((o / wl.n, kind, o, min(wl.n, o + CPF * per)))
            jobs.sort()
            pend, bad = [], 0
            t0 = time.time()
            for _, kind, o, z in jobs:
                wl = st[kind]
                if inplace:
                    (eng.queue_ecdsa_batch_inplace if kind == "ecdsa" else eng.queue_schnorr_batch_inplace)(wl.cols[0][o:z], wl.cols[1][o:z], wl.cols[2][o:z])
                else:
                    (eng.queue_ecdsa_batch if kind == "ecdsa" else eng.queue_schnorr_batch)(wl.cols[0][o:z], wl.cols[1][o:z], wl.cols[2][o:z])
                eng.flush()
                pend.append(wl.expect[o:z])
                if len(pend) == DEPTH:
                    bad += int((eng.wait() != pend.pop(0)).sum())
            while pend:
                bad += int((eng.wait() != pend.pop(0)).sum())
            return time.time() - t0, bad
        inproc()
        t_in, bad_in = min(inproc() for _ in range(3))
        assert bad_in == 0
        # the same producer with its rows queued IN PLACE (the columns pinned once: lamd_host_register): no host copy at all
        cols = [c for kind in ("ecdsa", "schnorr") for c in st[kind].cols]
        pinned = all(eng.host_register(c) for c in cols)
        inproc(True)
        t_in_place, bad_in_place = min(inproc(True) for _ in range(3))
        assert bad_in_place == 0
        if pinned:
            assert all(eng.host_unregister(c) for c in cols)
        nv = st["ecdsa"].n + st["schnorr"].n
    finally:
        eng.close()
    torch.cuda.synchronize()
    sock = os.path.join(sockdir, "stream.sock")
    p = _start(sock)
    try:
        files, go = [], str(tmp_path / "go")
        for i in range(W):   # client i takes every W-th block of whole commitments of both kinds
            sl = lambda wl: np.concatenate([np.arange(c * per, (c + 1) * per) for c in range(i, wl.n // per, W)])
            ie, is_ = sl(st["ecdsa"]), sl(st["schnorr"])
            f = str(tmp_path / ("shard%d.npz" % i))
            np.savez(f, eh=st["ecdsa"].cols[0][ie], es=st["ecdsa"].cols[1][ie], ek=st["ecdsa"].cols[2][ie], ee=st["ecdsa"].expect[ie].astype(np.uint8),
                     sm=st["schnorr"].cols[0][is_], sk=st["schnorr"].cols[1][is_], ss=st["schnorr"].cols[2][is_], se=st["schnorr"].expect[is_].astype(np.uint8))
            files.append(f)
        procs = [subprocess.Popen([sys.executable, "-c", GPU_STREAM_CLIENT_SCRIPT, ROOT, sock, files[i], str(CPF), str(DEPTH), go, str(i)], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True) for i in range(W)]
        t_wait = time.time()
        while not all(os.path.exists(go + ".ready%d" % i) for i in range(W)):
            assert time.time() - t_wait < 240 and all(q.poll() is None for q in procs), [q.communicate()[1][-400:] for q in procs if q.poll() is not None]
            time.sleep(0.01)
        open(go, "w").close()
        outs = [q.communicate(timeout=300) for q in procs]
        assert all(q.returncode == 0 for q in procs), [o[1][-400:] for o in outs]
        vals = [dict(zip(o[0].split()[0::2], o[0].split()[1::2])) for o in outs]
        assert all(int(v["bad"]) == 0 for v in vals), vals
        assert sum(int(v["rows"]) for v in vals) == nv
        t_served = max(float(v["t1"]) for v in vals) - min(float(v["t0"]) for v in vals)
        L = _client()
        rc, ctx = _connect(L, sock)
        assert rc == 0
        stt = Stats()
        assert L.lamd_client_server_stats(ctx, ctypes.byref(stt)) == 0
        L.lamd_shutdown(ctx)
        rec = {"verifies": nv, "clients": W, "commitments_per_flush": CPF, "flushes_in_flight_per_client": DEPTH, "in_process_s": t_in, "served_s": t_served, "in_process_in_place_s": t_in_place, "in_process_columns_pinned": bool(pinned),
               "in_process_verifies_per_s": nv / t_in, "served_verifies_per_s": nv / t_served, "served_over_in_process": t_in / t_served,
               "client_flushes": int(stt.flushes), "engine_flushes": int(stt.engine_flushes), "largest_engine_flush_requests": int(stt.largest_engine_flush_requests),
               "flush_rows": int(stt.flush_rows), "flush_rows_in_place": int(stt.flush_rows_in_place), "server_args": os.environ.get("LAMD_SERVED_TEST_ARGS", "")}
        print("served streaming:", rec)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        json.dump(rec, open(os.path.join(ROOT, "gpurun_out", "served_stream.json"), "w"), indent=1)
        assert stt.flushes >= 2 * (nv // (CPF * per)) and stt.engine_flushes <= stt.flushes
        assert t_in / t_served >= 0.4, rec
    finally:
        _stop(p)

"""Python front end over the C ABI (include/lightning_amd.h).  Device memory and streams come
from PyTorch-ROCm when the *_device methods are used; the numpy methods go through the
library's own staging.  Nothing here computes: every verdict comes from the HIP kernels."""
import ctypes

import numpy as np

from . import _ffi

ERRORS = {0: "OK", -1: "no usable gfx950 device", -2: "HIP error", -3: "bad argument", -4: "out of memory", -5: "bad state"}


class LamdError(RuntimeError):
    pass


def _verdicts(ok):
    """the verdict column of a finished call -> bool.  Every byte the library writes is 0 or 1 (include/lightning_amd.h); the kernels' own
    markers (2: BIP-340 parity or recovery still pending, 3: suspect, for the careful kernel) never leave a lane's workspace, and any
    non-zero byte would read as an accept -- so anything else is an error, not a verdict."""
    if ok.size and ok.max() > 1:
        bad = np.flatnonzero(ok > 1)
        raise LamdError("verdict byte %d at row %d is neither 0 nor 1 (%d such rows of %d)" % (int(ok[bad[0]]), int(bad[0]), bad.size, ok.size))
    return ok.astype(bool)


def _u8(a, shape_tail):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(-1, shape_tail)
    if a.shape[1] != shape_tail:
        raise ValueError("expected rows of %d bytes, got %r" % (shape_tail, a.shape))
    return a


def _key_column(pub, layout):
    """the key column of a call -> (array to keep alive, key length, stride).  layout None: pub is [n, keylen], packed (stride = keylen).
    layout (keylen, stride): pub is a flat uint8 buffer with key i at i * stride, handed to the library where it lies -- it need hold no
    more than (n - 1) * stride + keylen bytes"""
    if layout is None:
        pub = np.ascontiguousarray(pub, dtype=np.uint8)
        return pub, pub.shape[1], pub.shape[1]
    if pub.dtype != np.uint8 or pub.ndim != 1 or not pub.flags.c_contiguous:
        raise ValueError("a strided key column is a flat C-contiguous uint8 buffer")
    return pub, int(layout[0]), int(layout[1])


STORE_END_REASONS = ("eof", "partial_header", "incomplete", "truncated", "short", "store_ended", "no_amount")   # LAMD_STORE_END_*


def _store_summary(s):
    d = {k: int(getattr(s, k)) for k in ("version", "clean", "records", "live", "deleted", "end_offset", "ok", "skipped_deleted", "bad_checksum", "unknown_type",
                                         "malformed", "redundant", "no_channel", "signatures")}
    d.update(end_reason=STORE_END_REASONS[s.end_reason], bad_signature=[int(x) for x in s.bad_signature], stage_ms=list(s.stage_ms))
    return d


def _repair_summary(r):
    d = {k: int(getattr(r, k)) for k in ("kept", "dropped_deleted", "dropped_verdict", "dropped_dependency", "dropped_bookkeeping", "out_len")}
    d["stage_ms"] = list(r.stage_ms)
    return d


def _latest_summary(r):
    d = {k: int(getattr(r, k)) for k in ("kept", "dropped_deleted", "dropped_verdict", "dropped_dependency", "dropped_bookkeeping", "dropped_superseded",
                                         "dropped_timestamp", "dropped_stale", "out_len")}
    d["stage_ms"] = list(r.stage_ms)
    return d


def _store_blob(blob):
    a = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, dtype=np.uint8)
    return a, a.size, (a if a.size else np.zeros(1, dtype=np.uint8))


def gossip_store_frame(blob):
    """lamd_gossip_store_frame: the walk over a gossip_store image (bytes or numpy uint8), on the host, no context.
    -> (rec_off uint64 [records], summary dict)"""
    lib = _ffi.load()
    _, n_bytes, buf = _store_blob(blob)
    n, s = ctypes.c_size_t(0), _ffi.LamdStoreSummary()
    rc = lib.lamd_gossip_store_frame(buf.ctypes.data, n_bytes, 0, None, ctypes.byref(n), ctypes.byref(s))
    if rc < 0 and n.value == 0:
        raise LamdError("lamd_gossip_store_frame: %s" % ERRORS.get(rc, rc))
    off = np.zeros(max(1, n.value), dtype=np.uint64)
    rc = lib.lamd_gossip_store_frame(buf.ctypes.data, n_bytes, n.value, off.ctypes.data, ctypes.byref(n), ctypes.byref(s))
    if rc < 0:
        raise LamdError("lamd_gossip_store_frame: %s" % ERRORS.get(rc, rc))
    return off[:n.value], _store_summary(s)


def apply_update_plan(blob, rec_off, plan):
    """the plan of Engine.channel_update_receive applied to the image it was made for, in numpy: the DELETED bit of every del_rec set, the
    headers of the set_rec announcements re-stamped (timestamp and crc), the DYING bit of every clr_rec header cleared where the plan has that
    key (Engine.channel_announcement_confirm's), the added records appended behind the old end.
    -> (image bytes, rec_off uint64 extended by the added records): audit it, or build digest, directory and stream index again"""
    img, n_bytes, _ = _store_blob(blob)
    if plan["records"] is None:
        raise ValueError("the plan holds no record bytes (host_out=False)")
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    out = np.concatenate([img[:n_bytes], np.frombuffer(plan["records"], dtype=np.uint8)])
    out[off[np.asarray(plan["del_rec"], dtype=np.int64)].astype(np.int64)] |= 0x80
    at = off[np.asarray(plan["set_rec"], dtype=np.int64)].astype(np.int64)
    for k, word in ((4, plan["set_crc"]), (8, plan["set_ts"])):
        be = np.asarray(word, dtype=">u4").view(np.uint8).reshape(-1, 4)
        for x in range(4):
            out[at + k + x] = be[:, x]
    if "clr_rec" in plan:
        out[off[np.asarray(plan["clr_rec"], dtype=np.int64)].astype(np.int64)] &= 0xF7
    return out.tobytes(), np.concatenate([off, np.uint64(n_bytes) + np.asarray(plan["add_off"], dtype=np.uint64)])


class StoreDigest:
    """lamd_store_digest: the channel digest Engine.gossip_store_digest built, resident on the device.  close() it before its Engine."""

    def __init__(self, engine, handle, summary):
        self._eng, self._h = engine, handle
        self.summary = {k: (list(getattr(summary, k)) if k == "stage_ms" else int(getattr(summary, k))) for k, _ in summary._fields_}

    def __len__(self):
        return int(self._eng._lib.lamd_store_digest_count(self._h)) if self._h else 0

    def read(self):
        """-> (scid uint64 [count], ts uint32 [count, 2], csum uint32 [count, 2], rec uint32 [count, 3] (0xFFFFFFFF: none))"""
        n = len(self)
        scid, ts, csum, rec = (np.zeros(max(1, n), dtype=np.uint64), np.zeros((max(1, n), 2), dtype=np.uint32), np.zeros((max(1, n), 2), dtype=np.uint32),
                               np.zeros((max(1, n), 3), dtype=np.uint32))
        self._eng._chk(self._eng._lib.lamd_store_digest_read(self._h, n, scid.ctypes.data, ts.ctypes.data, csum.ctypes.data, rec.ctypes.data))
        return scid[:n], ts[:n], csum[:n], rec[:n]

    def read_bare(self):
        """-> scid uint64 [summary["channels_no_update"]]: the channels without an update, ascending"""
        n = int(self._eng._lib.lamd_store_digest_bare_count(self._h)) if self._h else 0
        scid = np.zeros(max(1, n), dtype=np.uint64)
        self._eng._chk(self._eng._lib.lamd_store_digest_read_bare(self._h, n, scid.ctypes.data))
        return scid[:n]

    def close(self):
        if self._h:
            self._eng._lib.lamd_store_digest_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class StoreDirectory:
    """lamd_store_directory: the directory Engine.gossip_store_directory built, resident on the device.  It refers to the image: a resident
    d_store must stay alive until free().  free() it before its Engine."""

    def __init__(self, engine, handle, summary, entries, bare, keep, chain_hash=None):
        self._eng, self._h, self._entries, self._bare, self._keep = engine, handle, entries, bare, keep
        self.chain_hash = None if chain_hash is None else bytes(chain_hash)
        self.summary = {k: (list(getattr(summary, k)) if k == "stage_ms" else int(getattr(summary, k))) for k, _ in summary._fields_}

    def __len__(self):
        return int(self._eng._lib.lamd_store_directory_node_count(self._h)) if self._h else 0

    def nodes(self):
        """-> (id uint8 [nodes, 33], first uint32 [nodes], nann_rec uint32 [nodes] (0xFFFFFFFF: not announced)), in rank order"""
        n = len(self)
        ids, first, nann = np.zeros((max(1, n), 33), dtype=np.uint8), np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32)
        self._eng._chk(self._eng._lib.lamd_store_directory_read_nodes(self._h, n, ids.ctypes.data, first.ctypes.data, nann.ctypes.data))
        return ids[:n], first[:n], nann[:n]

    def channels(self):
        """-> (bare_rec uint32 [bare], entry_rank uint32 [entries, 2], bare_rank uint32 [bare, 2] (0xFFFFFFFF: no node))"""
        e, b = self._entries, self._bare
        bare_rec, erank, brank = np.zeros(max(1, b), dtype=np.uint32), np.zeros((max(1, e), 2), dtype=np.uint32), np.zeros((max(1, b), 2), dtype=np.uint32)
        self._eng._chk(self._eng._lib.lamd_store_directory_read_channels(self._h, e, b, bare_rec.ctypes.data, erank.ctypes.data, brank.ctypes.data))
        return bare_rec[:b], erank[:e], brank[:b]

    def free(self):
        if self._h:
            self._eng._lib.lamd_store_directory_free(self._h)
            self._h = self._keep = None

    close = free

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class StoreStream:
    """lamd_store_stream: the stream index Engine.gossip_store_stream built, resident on the device: the records gossmap_stream_next would hand
    out, in file order.  It refers to the image: a resident d_store must stay alive until free().  free() it before its Engine."""

    def __init__(self, engine, handle, summary, keep):
        self._eng, self._h, self._keep = engine, handle, keep
        self.summary = {k: (list(getattr(summary, k)) if k == "stage_ms" else int(getattr(summary, k))) for k, _ in summary._fields_}

    def __len__(self):
        return int(self._eng._lib.lamd_store_stream_count(self._h)) if self._h else 0

    def read(self):
        """-> (rec uint32 [count] (the record index), ts uint32 [count] (its header timestamp), len uint32 [count] (its message length)), in file order"""
        n = len(self)
        rec, ts, ln = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32)
        self._eng._chk(self._eng._lib.lamd_store_stream_read(self._h, n, rec.ctypes.data, ts.ctypes.data, ln.ctypes.data))
        return rec[:n], ts[:n], ln[:n]

    def free(self):
        if self._h:
            self._eng._lib.lamd_store_stream_free(self._h)
            self._h = self._keep = None

    close = free

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class Engine:
    """One context = one GPU, one stream.  Mirrors lamd_init()/lamd_shutdown()."""

    def __init__(self, device=0):
        self._lib = _ffi.load()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.lamd_init(ctypes.byref(self._ctx), device)
        if rc != 0:
            msg = self._lib.lamd_last_error(self._ctx).decode() if self._ctx else ""
            if self._ctx:
                self._lib.lamd_shutdown(self._ctx)
                self._ctx = ctypes.c_void_p()
            raise LamdError("lamd_init failed: %s %s" % (ERRORS.get(rc, rc), msg))
        self.device = device

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.lamd_shutdown(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise LamdError("%s: %s" % (ERRORS.get(rc, rc), self._lib.lamd_last_error(self._ctx).decode()))
        return rc

    # ---- host-buffer batches (numpy uint8 in, numpy bool out)
    def verify_ecdsa(self, hash32, sig64, pub):
        pub = np.ascontiguousarray(pub, dtype=np.uint8)
        if pub.ndim != 2 or pub.shape[1] not in (33, 65):
            raise ValueError("pub must be [n,33] or [n,65]")
        hash32, sig64 = _u8(hash32, 32), _u8(sig64, 64)
        n = hash32.shape[0]
        if not (sig64.shape[0] == n == pub.shape[0]):
            raise ValueError("row counts differ")
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_verify_ecdsa_batch(self._ctx, n, hash32.ctypes.data, sig64.ctypes.data, pub.ctypes.data,
                                                    pub.shape[1], pub.shape[1], ok.ctypes.data))
        return _verdicts(ok)

    def verify_schnorr(self, msg32, xonly32, sig64):
        msg32, xonly32, sig64 = _u8(msg32, 32), _u8(xonly32, 32), _u8(sig64, 64)
        n = msg32.shape[0]
        if not (xonly32.shape[0] == n == sig64.shape[0]):
            raise ValueError("row counts differ")
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_verify_schnorr_batch(self._ctx, n, msg32.ctypes.data, xonly32.ctypes.data, sig64.ctypes.data,
                                                      ok.ctypes.data))
        return _verdicts(ok)

    def check_tx_sig_batch(self, preimages, sighash_types, has_witness, sig64, pub, key_layout=None):
        """preimages: list of bytes (BIP143 preimages); returns bool verdicts (gate + SHA256d + verify, all on the device).
        key_layout (publen, pubstride): pub is a flat strided key column (_key_column)"""
        n = len(preimages)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in preimages], dtype=np.uint64)
        blob = np.frombuffer(b"".join(preimages) + b"\x00", dtype=np.uint8)
        types = np.ascontiguousarray(sighash_types, dtype=np.uint8)
        wit = np.ascontiguousarray(has_witness, dtype=np.uint8)
        sig64 = _u8(sig64, 64)
        pub, publen, pubstride = _key_column(pub, key_layout)
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_check_tx_sig_batch(self._ctx, n, blob.ctypes.data, off.ctypes.data, types.ctypes.data, wit.ctypes.data,
                                                    sig64.ctypes.data, pub.ctypes.data, publen, pubstride, ok.ctypes.data))
        return _verdicts(ok)

    def check_tx_sig_tx_batch(self, txs, sig64, pub, key_layout=None):
        """txs: list of dicts {version, locktime, inputs: [(txid32, vout, sequence)], outputs: [(amount, spk)], input_num, amount, script,
        sighash_type, has_witness}; the BIP143 sighash is computed on the device (lamd_check_tx_sig_tx_batch).  Returns bool verdicts.
        key_layout (publen, pubstride): pub is a flat strided key column (_key_column)"""
        n = len(txs)
        u32 = lambda k: np.array([t[k] for t in txs], dtype=np.uint32)
        inputs = b"".join(b"".join(bytes(i[0]) + int(i[1]).to_bytes(4, "little") + int(i[2]).to_bytes(4, "little") for i in t["inputs"]) for t in txs)

        def varint(v):
            return bytes([v]) if v < 0xfd else (b"\xfd" + v.to_bytes(2, "little") if v <= 0xffff else b"\xfe" + v.to_bytes(4, "little"))
        outs = [b"".join(int(a).to_bytes(8, "little") + varint(len(spk)) + bytes(spk) for a, spk in t["outputs"]) for t in txs]
        scripts = [bytes(t["script"]) for t in txs]
        off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        in_off, out_off, sc_off = off([len(t["inputs"]) for t in txs]), off([len(o) for o in outs]), off([len(x) for x in scripts])
        blob = lambda b: np.frombuffer(b + b"\x00", dtype=np.uint8)
        ib, ob, sb = blob(inputs), blob(b"".join(outs)), blob(b"".join(scripts))
        ver, lock, inum, nout = u32("version"), u32("locktime"), u32("input_num"), np.array([len(t["outputs"]) for t in txs], dtype=np.uint32)
        amt = np.array([t["amount"] for t in txs], dtype=np.uint64)
        types = np.array([t["sighash_type"] for t in txs], dtype=np.uint8)
        wit = np.array([1 if t["has_witness"] else 0 for t in txs], dtype=np.uint8)
        sig64 = _u8(sig64, 64)
        pub, publen, pubstride = _key_column(pub, key_layout)
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_check_tx_sig_tx_batch(self._ctx, n, ver.ctypes.data, lock.ctypes.data, ib.ctypes.data, in_off.ctypes.data, inum.ctypes.data,
                                                       amt.ctypes.data, ob.ctypes.data, out_off.ctypes.data, nout.ctypes.data, sb.ctypes.data,
                                                       sc_off.ctypes.data, types.ctypes.data, wit.ctypes.data, sig64.ctypes.data, pub.ctypes.data,
                                                       publen, pubstride, ok.ctypes.data))
        return _verdicts(ok)

    def commitment_call(self, commit_tx, remote_funding33, commit_sig64, commit_sighash_type, htlc_txs, remote_htlckey33, htlc_sigs64, htlc_sighash_types):
        """the arguments of check_commitment_signed() marshalled ONCE; returns a function that makes the C call and nothing else -> (first_bad, ok_rows).
        (bench.py times this: flattening 484 templates in Python costs more than the call.)"""
        def varint(v):
            return bytes([v]) if v < 0xfd else (b"\xfd" + v.to_bytes(2, "little") if v <= 0xffff else b"\xfe" + v.to_bytes(4, "little"))
        keep = []

        def tmpl(t):
            ins = b"".join(bytes(i[0]) + int(i[1]).to_bytes(4, "little") + int(i[2]).to_bytes(4, "little") for i in t["inputs"])
            outs = b"".join(int(a).to_bytes(8, "little") + varint(len(spk)) + bytes(spk) for a, spk in t["outputs"])
            bufs = [ctypes.create_string_buffer(x, len(x) + 1) for x in (ins, outs, bytes(t["script"]))]
            keep.extend(bufs)
            return _ffi.LamdTxTemplate(t["version"], t["locktime"], ctypes.addressof(bufs[0]), len(t["inputs"]), t.get("input_num", 0), t["amount"],
                                       ctypes.addressof(bufs[1]), len(outs), len(t["outputs"]), ctypes.addressof(bufs[2]), len(t["script"]))
        ct = tmpl(commit_tx)
        n = len(htlc_txs)
        arr = (_ffi.LamdTxTemplate * max(1, n))(*[tmpl(t) for t in htlc_txs])
        sigs = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in htlc_sigs64) + b"\x00", dtype=np.uint8))
        types = np.array(list(htlc_sighash_types) + [0], dtype=np.uint8)
        first_bad = ctypes.c_int64(0)
        ok = np.zeros(1 + n, dtype=np.uint8)
        fk, hk, cs = bytes(remote_funding33), bytes(remote_htlckey33), bytes(commit_sig64)
        keep += [ct, arr, sigs, types, fk, hk, cs]

        def call():
            self._chk(self._lib.lamd_check_commitment_signed(self._ctx, ctypes.addressof(ct), fk, cs, commit_sighash_type, n, ctypes.addressof(arr), hk,
                                                             sigs.ctypes.data, types.ctypes.data, ctypes.byref(first_bad), ok.ctypes.data))
            return int(first_bad.value), _verdicts(ok)
        call.keep = keep
        return call

    def check_commitment_signed(self, commit_tx, remote_funding33, commit_sig64, commit_sighash_type, htlc_txs, remote_htlckey33, htlc_sigs64,
                                htlc_sighash_types):
        """ONE commitment_signed (channeld/channeld.c:2171-2232) through lamd_check_commitment_signed.  commit_tx / htlc_txs[i]: dicts {version,
        locktime, inputs: [(txid32, vout, sequence)], outputs: [(amount, spk)], input_num, amount, script}.  Returns (first_bad, ok_rows):
        first_bad = -1 all good, 0 the commitment signature, 1 + i htlc_sigs[i] -- the first failure in the reference's order."""
        return self.commitment_call(commit_tx, remote_funding33, commit_sig64, commit_sighash_type, htlc_txs, remote_htlckey33, htlc_sigs64,
                                    htlc_sighash_types)()

    @staticmethod
    def _streams(streams):
        off = np.concatenate([[0], np.cumsum([len(x) for x in streams])]).astype(np.uint64)
        return np.frombuffer(b"".join(bytes(x) for x in streams) + b"\x00", dtype=np.uint8), off

    def bolt12_check_signature_batch(self, streams, messagename, fieldname, key33, sig64, keystride=None):
        """streams: list of serialised TLV streams; key33 uint8 [n,33]; sig64 uint8 [n,64] -> bool verdicts (lamd_bolt12_check_signature_batch).
        keystride: key33 is a flat strided key column (_key_column)"""
        blob, off = self._streams(streams)
        sig64 = _u8(sig64, 64)
        key33, _, stride = _key_column(_u8(key33, 33) if keystride is None else key33, None if keystride is None else (33, keystride))
        ok = np.zeros(len(streams), dtype=np.uint8)
        self._chk(self._lib.lamd_bolt12_check_signature_batch(self._ctx, len(streams), blob.ctypes.data, off.ctypes.data, messagename, fieldname,
                                                              key33.ctypes.data, stride, sig64.ctypes.data, ok.ctypes.data))
        return _verdicts(ok)

    def bolt12_merkle_batch(self, streams, messagename, fieldname):
        """-> (merkle roots uint8 [n,32], signature hashes uint8 [n,32], ok bool [n])"""
        blob, off = self._streams(streams)
        n = len(streams)
        mk, sh, ok = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_bolt12_merkle_batch(self._ctx, n, blob.ctypes.data, off.ctypes.data, messagename, fieldname, mk.ctypes.data,
                                                     sh.ctypes.data, ok.ctypes.data))
        return mk, sh, _verdicts(ok)

    def ecdsa_recover(self, hash32, sig64, recid):
        """numpy uint8 [n,32], [n,64], [n] -> (keys uint8 [n,33], ok bool [n]); secp256k1_ecdsa_recover semantics"""
        hash32, sig64 = _u8(hash32, 32), _u8(sig64, 64)
        recid = np.ascontiguousarray(recid, dtype=np.uint8)
        n = hash32.shape[0]
        keys = np.zeros((n, 33), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n:
            self._chk(self._lib.lamd_ecdsa_recover_batch(self._ctx, n, hash32.ctypes.data, sig64.ctypes.data, recid.ctypes.data,
                                                         keys.ctypes.data, ok.ctypes.data))
        return keys, _verdicts(ok)

    def bolt11_check(self, strings):
        """strings: BOLT #11 invoices as bolt11_decode() takes them (str or bytes, no "lightning:" prefix) -> (status int8 [n] (LAMD_B11_*),
        node_id uint8 [n,33], hash uint8 [n,32], have_n bool [n]): decoding, hashing, recovery or verification under the `n` key on the device
        (lamd_bolt11_check_batch)"""
        blob, off = self._streams([x.encode("latin-1") if isinstance(x, str) else x for x in strings])
        n = len(strings)
        status, node, h, hn = np.zeros(n, dtype=np.int8), np.zeros((n, 33), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_bolt11_check_batch(self._ctx, n, blob.ctypes.data, off.ctypes.data, status.ctypes.data, node.ctypes.data, h.ctypes.data,
                                                    hn.ctypes.data))
        return status, node, h, _verdicts(hn)

    def checkmessage(self, messages, zbases):
        """messages, zbases: the message and the zbase32 signature string of each checkmessage call (str or bytes) -> (status int8 [n] (LAMD_MSG_*),
        node_id uint8 [n,33]: the recovered key) (lamd_checkmessage_batch)"""
        enc = lambda xs: [x.encode("utf-8") if isinstance(x, str) else x for x in xs]
        if len(messages) != len(zbases):
            raise ValueError("one signature string per message")
        mblob, moff = self._streams(enc(messages))
        zblob, zoff = self._streams(enc(zbases))
        n = len(messages)
        status, node = np.zeros(n, dtype=np.int8), np.zeros((n, 33), dtype=np.uint8)
        self._chk(self._lib.lamd_checkmessage_batch(self._ctx, n, mblob.ctypes.data, moff.ctypes.data, zblob.ctypes.data, zoff.ctypes.data, status.ctypes.data,
                                                    node.ctypes.data))
        return status, node

    def bolt12_check(self, strings):
        """strings: BOLT #12 offers, invoice requests and invoices as offer_decode() / invrequest_decode() / invoice_decode() take them (str or
        bytes; the kinds may be mixed) -> (status int8 [n] (LAMD_B12_*), kind uint8 [n] (LAMD_B12_KIND_*), signer uint8 [n,33], sighash uint8
        [n,32], offer_id uint8 [n,32], invreq_id uint8 [n,32]): join collapse, bech32 decoding, the TLV walk, the ids, the merkle root and the
        BIP-340 verification under the string's own key on the device (lamd_bolt12_check_text_batch)"""
        blob, off = self._streams([x.encode("latin-1") if isinstance(x, str) else x for x in strings])
        n = len(strings)
        status, kind, signer = np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.uint8), np.zeros((n, 33), dtype=np.uint8)
        sighash, offer_id, invreq_id = (np.zeros((n, 32), dtype=np.uint8) for _ in range(3))
        self._chk(self._lib.lamd_bolt12_check_text_batch(self._ctx, n, blob.ctypes.data, off.ctypes.data, status.ctypes.data, kind.ctypes.data,
                                                         signer.ctypes.data, sighash.ctypes.data, offer_id.ctypes.data, invreq_id.ctypes.data))
        return status, kind, signer, sighash, offer_id, invreq_id

    def _after_torch(self):
        """order the next submission after what torch's current stream holds (the tensors handed to the *_device methods are
        usually produced there); a device-side event, no host synchronisation.  The caller still has to keep the tensors alive
        until the results are complete."""
        if not getattr(self, "auto_order", True):
            return
        try:
            import torch
            self._chk(self._lib.lamd_wait_stream(self._ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        except ImportError:
            pass

    def ecdsa_recover_device(self, d_hash32, d_sig64, d_recid, d_pub33, d_ok):
        self._after_torch()
        self._chk(self._lib.lamd_ecdsa_recover_batch_device(self._ctx, d_hash32.shape[0], d_hash32.data_ptr(), d_sig64.data_ptr(),
                                                            d_recid.data_ptr(), d_pub33.data_ptr(), d_ok.data_ptr()))

    def grind_htlc_tx_fee(self, preimage, outputs, input_sat, weight, min_feerate, max_feerate, sig64, sighash_type, has_witness, pub33):
        """grind_htlc_tx_fee (onchaind/onchaind.c:388-438) on the device: (feerate, fee) of the lowest matching feerate, or None"""
        rate, fee = ctypes.c_uint32(0), ctypes.c_uint64(0)
        pre, outs, sig, key = bytes(preimage), bytes(outputs), bytes(sig64), bytes(pub33)
        rc = self._chk(self._lib.lamd_grind_htlc_tx_fee(self._ctx, pre, len(pre), outs, len(outs), int(input_sat), int(weight), int(min_feerate),
                                                         int(max_feerate), sig, int(sighash_type), int(bool(has_witness)), key,
                                                         ctypes.byref(rate), ctypes.byref(fee)))
        return (rate.value, fee.value) if rc == 1 else None

    def pubkey_parse(self, pub):
        pub = np.ascontiguousarray(pub, dtype=np.uint8)
        n, ln = pub.shape
        out = np.zeros((n, 64), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._lib.lamd_pubkey_parse_batch(self._ctx, n, pub.ctypes.data, ln, ln, out.ctypes.data, ok.ctypes.data))
        return out, _verdicts(ok)

    def sigcheck_gossip(self, msgs, node_ids=None):
        """msgs: list of bytes (raw wire messages).  node_ids: list of 33-byte ids (or None entries), needed for
        channel_update.  Returns int8 verdicts (see lamd_sigcheck_gossip_batch)."""
        n = len(msgs)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(msgs) + b"\x00", dtype=np.uint8)
        ids_ptr = None
        if node_ids is not None:
            ids = np.zeros((n, 33), dtype=np.uint8)
            for i, k in enumerate(node_ids):
                if k is not None:
                    ids[i] = np.frombuffer(k, dtype=np.uint8)
            ids_ptr = ids.ctypes.data
        verdict = np.zeros(n, dtype=np.int8)
        self._chk(self._lib.lamd_sigcheck_gossip_batch(self._ctx, n, blob.ctypes.data, off.ctypes.data, ids_ptr, verdict.ctypes.data))
        return verdict

    def gossip_store_audit(self, blob, d_store=None):
        """lamd_gossip_store_audit over a gossip_store image (bytes or numpy uint8): checksums and every signature, on the device.
        d_store: the same image resident in a torch uint8 CUDA tensor (it is then not copied).
        -> (rec_off uint64 [records], verdict int8 [records], summary dict)"""
        _, n_bytes, buf = _store_blob(blob)
        cnt, s = ctypes.c_size_t(0), _ffi.LamdStoreSummary()
        self._lib.lamd_gossip_store_frame(buf.ctypes.data, n_bytes, 0, None, ctypes.byref(cnt), ctypes.byref(s))   # the count; the audit reports every error itself
        n = cnt.value
        off, verdict = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.int8)
        d_ptr = None
        if d_store is not None:
            if d_store.numel() != n_bytes:
                raise ValueError("the resident image and the host image differ in size")
            self._after_torch()
            d_ptr = d_store.data_ptr()
        self._chk(self._lib.lamd_gossip_store_audit(self._ctx, buf.ctypes.data, n_bytes, d_ptr, n, off.ctypes.data, verdict.ctypes.data, ctypes.byref(cnt),
                                                    ctypes.byref(s)))
        return off[:cnt.value], verdict[:cnt.value], _store_summary(s)

    def gossip_store_repair(self, blob, uuid, d_store=None, d_out=None, host_out=True):
        """lamd_gossip_store_repair over a gossip_store image (bytes or numpy uint8): the audit, then the store that holds the records which passed and
        whose dependencies passed, behind a fresh uuid record (uuid: 32 bytes).  d_store: the image resident in a torch uint8 CUDA tensor.
        d_out: a torch uint8 CUDA tensor the output is left in (len(blob) + 46 bytes always suffice); host_out=False: no copy to the host.
        -> (out bytes or None, rec_off uint64 [records], verdict int8 [records], new_off uint64 [records] (2**64 - 1: dropped), reason uint8 [records],
            audit summary dict, repair summary dict)"""
        return self._store_repair(None, blob, uuid, d_store, d_out, host_out)

    def gossip_store_repair_latest(self, blob, uuid, now=0, future_slack=86400, prune_interval=1209600, d_store=None, d_out=None, host_out=True):
        """lamd_gossip_store_repair_latest: gossip_store_repair, and of the node_announcements and channel_updates that pass it only the latest per node
        and per (channel, direction); records whose header timestamp is not the signed one or lies more than future_slack seconds ahead of `now`
        are dropped, and so are channels a direction of which has been silent for more than prune_interval seconds.  now=0: no clock (both rules
        that need one are off).  Arguments and result as gossip_store_repair; reasons 5 superseded, 6 timestamp, 7 stale; the last dict is
        lamd_store_latest_summary."""
        return self._store_repair(_ffi.LamdStoreLatestPolicy(int(now), int(future_slack), int(prune_interval)), blob, uuid, d_store, d_out, host_out)

    def _store_repair(self, policy, blob, uuid, d_store, d_out, host_out):
        _, n_bytes, buf = _store_blob(blob)
        uuid = np.frombuffer(bytes(uuid), dtype=np.uint8)
        if uuid.size != 32:
            raise ValueError("the uuid has 32 bytes")
        cnt, s = ctypes.c_size_t(0), _ffi.LamdStoreSummary()
        r = _ffi.LamdStoreRepairSummary() if policy is None else _ffi.LamdStoreLatestSummary()
        self._lib.lamd_gossip_store_frame(buf.ctypes.data, n_bytes, 0, None, ctypes.byref(cnt), ctypes.byref(s))   # the count; the repair reports every error itself
        n = cnt.value
        off, verdict = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.int8)
        new_off, reason = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint8)
        d_ptr = d_out_ptr = None
        if d_store is not None:
            if d_store.numel() != n_bytes:
                raise ValueError("the resident image and the host image differ in size")
            d_ptr = d_store.data_ptr()
        out_cap = n_bytes + 46
        if d_out is not None:
            d_out_ptr, out_cap = d_out.data_ptr(), d_out.numel()
        if d_store is not None or d_out is not None:
            self._after_torch()
        out = np.zeros(out_cap, dtype=np.uint8) if host_out else None
        head = (self._ctx, buf.ctypes.data, n_bytes, d_ptr, uuid.ctypes.data)
        tail = (n, off.ctypes.data, verdict.ctypes.data, new_off.ctypes.data, reason.ctypes.data, ctypes.byref(cnt), out.ctypes.data if host_out else None, d_out_ptr,
                out_cap, ctypes.byref(s), ctypes.byref(r))
        if policy is None:
            self._chk(self._lib.lamd_gossip_store_repair(*head, *tail))
        else:
            self._chk(self._lib.lamd_gossip_store_repair_latest(*head, ctypes.byref(policy), *tail))
        k = cnt.value
        return (out[:r.out_len].tobytes() if host_out else None, off[:k], verdict[:k], new_off[:k], reason[:k], _store_summary(s),
                _repair_summary(r) if policy is None else _latest_summary(r))

    def gossip_store_digest(self, blob=None, rec_off=None, verdict=None, d_store=None):
        """lamd_gossip_store_digest_build: the channel digest of a gossip_store image, resident on the device: one entry per channel with an
        update (scid, both timestamps, both update checksums, the record indices), sorted by scid.  blob: the image (bytes or numpy uint8),
        and / or d_store: the image in a torch uint8 CUDA tensor (read in place); rec_off: the records' offsets (default: the walk over
        blob); verdict: optional int8 per record, the audit's -- records that are not OK do not count.  -> StoreDigest"""
        if blob is None and d_store is None:
            raise ValueError("an image on the host or on the device is needed")
        buf_ptr, n_bytes = None, 0
        if blob is not None:
            _, n_bytes, buf = _store_blob(blob)
            buf_ptr = buf.ctypes.data
            if rec_off is None:
                rec_off = gossip_store_frame(blob)[0]
        if rec_off is None:
            raise ValueError("a resident image needs rec_off")
        d_ptr = None
        if d_store is not None:
            if blob is not None and d_store.numel() != n_bytes:
                raise ValueError("the resident image and the host image differ in size")
            n_bytes = d_store.numel()
            self._after_torch()
            d_ptr = d_store.data_ptr()
        off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        v = None
        if verdict is not None:
            v = np.ascontiguousarray(verdict, dtype=np.int8)
            if v.size != off.size:
                raise ValueError("one verdict per record")
        h, s = ctypes.c_void_p(), _ffi.LamdStoreDigestSummary()
        self._chk(self._lib.lamd_gossip_store_digest_build(self._ctx, buf_ptr, n_bytes, d_ptr, off.size, off.ctypes.data if off.size else None,
                                                           v.ctypes.data if v is not None and v.size else None, ctypes.byref(h), ctypes.byref(s)))
        return StoreDigest(self, h, s)

    def channel_range_replies(self, digest, chain_hash, queries, max_encoded_bytes=0, return_summary=False):
        """lamd_channel_range_reply_batch: the reply_channel_range messages to a batch of raw query_channel_range messages, from a
        StoreDigest.  chain_hash: the 32 bytes of the chain this node serves; max_encoded_bytes: the reference's dev_max_encoding_bytes
        (0: none).  -> (status int8 [queries] (0 answered, -1 malformed: no reply, 1 foreign chain: one empty reply), [[bytes, ...], ...])"""
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(q) for q in queries) + b"\x00", dtype=np.uint8)
        status, first = np.zeros(max(1, nq), dtype=np.int8), np.zeros(nq + 1, dtype=np.uint64)
        s = _ffi.LamdRangeReplySummary()
        head = (self._ctx, digest._h, chain.ctypes.data, nq, blob.ctypes.data, qoff.ctypes.data, int(max_encoded_bytes), status.ctypes.data, first.ctypes.data)
        rc = self._lib.lamd_channel_range_reply_batch(*head, 0, None, None, None, 0, ctypes.byref(s))          # the sizes
        if rc < 0 and not (rc == -3 and s.messages):
            self._chk(rc)
        msg_off, out = np.zeros(s.messages + 1, dtype=np.uint64), np.zeros(max(1, s.bytes), dtype=np.uint8)
        self._chk(self._lib.lamd_channel_range_reply_batch(*head, s.messages, msg_off.ctypes.data, out.ctypes.data, None, s.bytes, ctypes.byref(s)))
        raw = out.tobytes()
        replies = [[raw[int(msg_off[j]):int(msg_off[j + 1])] for j in range(int(first[q]), int(first[q + 1]))] for q in range(nq)]
        if return_summary:
            return status[:nq], replies, {k: (list(getattr(s, k)) if k == "stage_ms" else int(getattr(s, k))) for k, _ in s._fields_}
        return status[:nq], replies

    def channel_range_compare(self, digest, chain_hash, msgs, want=None, max_unknown=0, max_stale=0, return_summary=False):
        """lamd_channel_range_compare_batch: peers' raw reply_channel_range messages compared with a StoreDigest, as the seeker does.
        chain_hash: the 32 bytes of our chain; want: optional [(range_first_blocknum, range_end_blocknum)] per message, the outstanding
        queries; max_unknown / max_stale: scids per query_short_channel_ids message (0: 8000 / 7000).
        -> (status int8 [msgs] (0 accepted, -1 malformed, 1..6: see the header), per_msg uint32 [msgs, 3] (entries, unknown, stale, before
        merging), unknown uint64 (ascending, each once), stale uint64 (ascending, each once), flags uint8 (the query_flags of each stale
        scid), [bytes, ...]: the query_short_channel_ids messages, those for the unknown list first)"""
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        n = len(msgs)
        if want is not None and len(want) != n:
            raise ValueError("one (first, end) per message")
        moff = np.zeros(n + 1, dtype=np.uint64)
        moff[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\x00", dtype=np.uint8)
        wf = we = None
        if want is not None:
            w = np.ascontiguousarray(np.array(want, dtype=np.uint32).reshape(n, 2))
            wf, we = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
            wf, we = (wf if n else np.zeros(1, dtype=np.uint32)), (we if n else np.zeros(1, dtype=np.uint32))
        status, per_msg = np.zeros(max(1, n), dtype=np.int8), np.zeros((max(1, n), 3), dtype=np.uint32)
        s = _ffi.LamdRangeCompareSummary()
        head = (self._ctx, digest._h, chain.ctypes.data, n, blob.ctypes.data, moff.ctypes.data, None if wf is None else wf.ctypes.data,
                None if we is None else we.ctypes.data, int(max_unknown), int(max_stale), status.ctypes.data, per_msg.ctypes.data)
        rc = self._lib.lamd_channel_range_compare_batch(*head, 0, None, None, None, 0, None, None, None, 0, ctypes.byref(s))          # the sizes
        if rc < 0 and not (rc == -3 and s.messages):
            self._chk(rc)
        cap = max(1, s.unknown, s.stale)
        unknown, stale, flags = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint8)
        msg_off, out = np.zeros(s.messages + 1, dtype=np.uint64), np.zeros(max(1, s.bytes), dtype=np.uint8)
        self._chk(self._lib.lamd_channel_range_compare_batch(*head, cap, unknown.ctypes.data, stale.ctypes.data, flags.ctypes.data, s.messages + 1,
                                                             msg_off.ctypes.data, out.ctypes.data, None, max(1, s.bytes), ctypes.byref(s)))
        raw = out.tobytes()
        messages = [raw[int(msg_off[j]):int(msg_off[j + 1])] for j in range(int(s.messages))]
        res = (status[:n], per_msg[:n], unknown[:s.unknown], stale[:s.stale], flags[:s.stale], messages)
        if return_summary:
            return res + ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    def gossip_store_directory(self, digest, blob=None, rec_off=None, verdict=None, d_store=None, chain_hash=None):
        """lamd_gossip_store_directory_build: the directory of a gossip_store image, from the (image, rec_off, verdict) its StoreDigest was built
        from and that digest: the records of every channel, the distinct node ids ranked by their 33 bytes, the node_announcement of each.  blob: the
        image (copied to the device and owned by the directory), or d_store: the image in a torch uint8 CUDA tensor, read in place (the directory
        keeps a reference to the tensor).  chain_hash: optional, the chain short_channel_ids_replies answers for by default.  -> StoreDirectory"""
        if chain_hash is not None and len(bytes(chain_hash)) != 32:
            raise ValueError("the chain_hash has 32 bytes")
        if blob is None and d_store is None:
            raise ValueError("an image on the host or on the device is needed")
        buf_ptr, n_bytes = None, 0
        if blob is not None:
            _, n_bytes, buf = _store_blob(blob)
            buf_ptr = buf.ctypes.data
            if rec_off is None:
                rec_off = gossip_store_frame(blob)[0]
        if rec_off is None:
            raise ValueError("a resident image needs rec_off")
        d_ptr = None
        if d_store is not None:
            if blob is not None and d_store.numel() != n_bytes:
                raise ValueError("the resident image and the host image differ in size")
            n_bytes = d_store.numel()
            self._after_torch()
            d_ptr = d_store.data_ptr()
        off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        v = None
        if verdict is not None:
            v = np.ascontiguousarray(verdict, dtype=np.int8)
            if v.size != off.size:
                raise ValueError("one verdict per record")
        h, s = ctypes.c_void_p(), _ffi.LamdStoreDirectorySummary()
        self._chk(self._lib.lamd_gossip_store_directory_build(self._ctx, buf_ptr, n_bytes, d_ptr, off.size, off.ctypes.data if off.size else None,
                                                              v.ctypes.data if v is not None and v.size else None, digest._h, ctypes.byref(h), ctypes.byref(s)))
        return StoreDirectory(self, h, s, len(digest), int(self._lib.lamd_store_digest_bare_count(digest._h)), d_store, chain_hash)

    def short_channel_ids_replies(self, directory, queries, chain_hash=None, return_summary=False, return_records=False):
        """lamd_short_channel_ids_reply_batch: the answers to a batch of raw query_short_channel_ids messages, from a StoreDirectory: per query
        the stored channel_announcements and channel_updates its flags ask for, in the query's order, the node_announcements asked for, each
        once, in the order of the node ids, and reply_short_channel_ids_end.  chain_hash: the 32 bytes of the chain this node serves
        (default: the one given to gossip_store_directory).
        -> (status int8 [queries] (0 answered, -1 malformed, 1 foreign chain: the end message alone, 2 bad flags, 3 bad scids, 4 flag count),
        per_query uint32 [queries, 4] (scids, known, channel messages, node messages), [[bytes, ...], ...]); return_records: and per message the
        record index it was copied from (0xFFFFFFFF: an end message)"""
        if chain_hash is None:
            chain_hash = directory.chain_hash
        if chain_hash is None:
            raise ValueError("a chain_hash is needed: here or at gossip_store_directory")
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(q) for q in queries) + b"\x00", dtype=np.uint8)
        status, per_query, first = np.zeros(max(1, nq), dtype=np.int8), np.zeros((max(1, nq), 4), dtype=np.uint32), np.zeros(nq + 1, dtype=np.uint64)
        s = _ffi.LamdScidReplySummary()
        head = (self._ctx, directory._h, chain.ctypes.data, nq, blob.ctypes.data, qoff.ctypes.data, status.ctypes.data, per_query.ctypes.data, first.ctypes.data)
        rc = self._lib.lamd_short_channel_ids_reply_batch(*head, 0, None, None, None, None, 0, ctypes.byref(s))          # the sizes
        if rc < 0 and not (rc == -3 and s.messages):
            self._chk(rc)
        msg_off, msg_rec, out = np.zeros(s.messages + 1, dtype=np.uint64), np.zeros(max(1, s.messages), dtype=np.uint32), np.zeros(max(1, s.bytes), dtype=np.uint8)
        self._chk(self._lib.lamd_short_channel_ids_reply_batch(*head, s.messages, msg_off.ctypes.data, msg_rec.ctypes.data, out.ctypes.data, None, s.bytes,
                                                               ctypes.byref(s)))
        raw = out.tobytes()
        spans = [range(int(first[q]), int(first[q + 1])) for q in range(nq)]
        res = (status[:nq], per_query[:nq], [[raw[int(msg_off[j]):int(msg_off[j + 1])] for j in sp] for sp in spans])
        if return_records:
            res += ([[int(msg_rec[j]) for j in sp] for sp in spans],)
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    def gossip_store_stream(self, blob=None, rec_off=None, verdict=None, d_store=None):
        """lamd_gossip_store_stream_build: the stream index of a gossip_store image: the records a peer's gossip_timestamp_filter can be answered
        with (DELETED and DYING clear, verdict OK where verdicts are given, type 256, 257 or 258, inside the image), in file order, with their
        header timestamps and lengths, and the prefix maximum of all header timestamps for the "recent" position.  blob: the image (copied to the
        device and owned by the index), or d_store: the image in a torch uint8 CUDA tensor, read in place (the index keeps a reference to the
        tensor).  A snapshot: build it again after a repair.  -> StoreStream"""
        if blob is None and d_store is None:
            raise ValueError("an image on the host or on the device is needed")
        buf_ptr, n_bytes = None, 0
        if blob is not None:
            _, n_bytes, buf = _store_blob(blob)
            buf_ptr = buf.ctypes.data
            if rec_off is None:
                rec_off = gossip_store_frame(blob)[0]
        if rec_off is None:
            raise ValueError("a resident image needs rec_off")
        d_ptr = None
        if d_store is not None:
            if blob is not None and d_store.numel() != n_bytes:
                raise ValueError("the resident image and the host image differ in size")
            n_bytes = d_store.numel()
            self._after_torch()
            d_ptr = d_store.data_ptr()
        off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        v = None
        if verdict is not None:
            v = np.ascontiguousarray(verdict, dtype=np.int8)
            if v.size != off.size:
                raise ValueError("one verdict per record")
        h, s = ctypes.c_void_p(), _ffi.LamdStoreStreamSummary()
        self._chk(self._lib.lamd_gossip_store_stream_build(self._ctx, buf_ptr, n_bytes, d_ptr, off.size, off.ctypes.data if off.size else None,
                                                           v.ctypes.data if v is not None and v.size else None, ctypes.byref(h), ctypes.byref(s)))
        return StoreStream(self, h, s, d_store)

    def timestamp_filter_replies(self, stream, filters, chain_hash, now, cursors=None, budgets=None, return_summary=False, return_records=False):
        """lamd_timestamp_filter_reply_batch: what a batch of peers that sent raw gossip_timestamp_filter messages are streamed from a StoreStream.
        chain_hash: the 32 bytes of the chain this node serves; now: the clock in seconds (the "recent" position is the first record stamped
        now - 7200 or later); cursors: per peer a position in the list to resume at, or None / 2**64 - 1: where the filter says (the start for
        first_timestamp 0, the end for 0xFFFFFFFF, else the recent position); budgets: per peer the bytes it may be sent in this call (a message
        is sent while the bytes so far are <= budget; < 0: nothing), None: unlimited.
        -> (status int8 [peers] (0 streamed, -1 malformed, 1 foreign chain), cursor_out uint64 [peers], done uint8 [peers] (1: the list ended),
        [[bytes, ...], ...]); return_records: and per message the record index it was copied from"""
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        n = len(filters)
        foff = np.zeros(n + 1, dtype=np.uint64)
        foff[1:] = np.cumsum([len(f) for f in filters], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(f) for f in filters) + b"\x00", dtype=np.uint8)
        cur = bud = None
        if cursors is not None:
            if len(cursors) != n:
                raise ValueError("one cursor per peer")
            cur = np.array([2 ** 64 - 1 if c is None else int(c) for c in cursors] + [0], dtype=np.uint64)
        if budgets is not None:
            if len(budgets) != n:
                raise ValueError("one budget per peer")
            bud = np.array([2 ** 63 - 1 if b is None else int(b) for b in budgets] + [0], dtype=np.int64)
        status, cursor_out, done, first = (np.zeros(max(1, n), dtype=np.int8), np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint8),
                                           np.zeros(n + 1, dtype=np.uint64))
        s = _ffi.LamdFilterReplySummary()
        head = (self._ctx, stream._h, chain.ctypes.data, int(now) & 0xFFFFFFFF, n, blob.ctypes.data, foff.ctypes.data, None if cur is None else cur.ctypes.data,
                None if bud is None else bud.ctypes.data, status.ctypes.data, cursor_out.ctypes.data, done.ctypes.data, first.ctypes.data)
        rc = self._lib.lamd_timestamp_filter_reply_batch(*head, 0, None, None, None, None, 0, ctypes.byref(s))          # the sizes
        if rc < 0 and not (rc == -3 and s.messages):
            self._chk(rc)
        msg_off, msg_rec, out = np.zeros(s.messages + 1, dtype=np.uint64), np.zeros(max(1, s.messages), dtype=np.uint32), np.zeros(max(1, s.bytes), dtype=np.uint8)
        self._chk(self._lib.lamd_timestamp_filter_reply_batch(*head, s.messages, msg_off.ctypes.data, msg_rec.ctypes.data, out.ctypes.data, None, s.bytes,
                                                              ctypes.byref(s)))
        raw = out.tobytes()
        spans = [range(int(first[p]), int(first[p + 1])) for p in range(n)]
        res = (status[:n], cursor_out[:n], done[:n], [[raw[int(msg_off[j]):int(msg_off[j + 1])] for j in sp] for sp in spans])
        if return_records:
            res += ([[int(msg_rec[j]) for j in sp] for sp in spans],)
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    def channel_update_receive(self, digest, directory, msgs, chain_hash=None, now=0, prune_interval=0, our_id=None, peers=None, held=(),
                               d_out=None, host_out=True, return_summary=False):
        """lamd_channel_update_receive_batch: a drained queue of raw channel_update messages received against the image a StoreDigest and a
        StoreDirectory were built from (both by this Engine): look-ups, signers, ONE signature batch, "newer wins, first among equals" in arrival
        order.  msgs: a list of messages, or (blob uint8, off uint64 [n + 1]): message i = blob[off[i]:off[i + 1]].  chain_hash: the 32 bytes of our chain (default: the one given to gossip_store_directory); now: the clock in seconds;
        prune_interval: 0 = 1209600; our_id: our 33-byte node id or None; peers: None, one 33-byte id for all messages, or one per message (None
        there: no source); held: the scids of the caller's pending and too-early announcements; d_out: a torch uint8 CUDA tensor the added
        records are written to (at its data pointer, any alignment) instead of, or with host_out besides, the host.
        -> (status int8 [msgs] (0 accepted, -1 malformed, 1 wrong chain, 2 timestamp, 3 held, 4 private, 5 unknown channel, 6 bad signature,
        7 DONT_FORWARD, 8 stale, 9 duplicate), flags uint8 [msgs] (1 SUPERSEDED, 2 FIRST, 4 DYING, 8 PEER_UPDATE), chan uint32 [msgs]
        (0xFFFFFFFF: none), plan): plan = dict(add_msg uint32 [adds], add_off uint64 [adds], records bytes or None (without host_out), del_rec
        uint32 ascending, set_rec / set_ts / set_crc uint32 [re-stamps]) -- apply_update_plan() applies it to the image"""
        if chain_hash is None:
            chain_hash = directory.chain_hash
        if chain_hash is None:
            raise ValueError("a chain_hash is needed: here or at gossip_store_directory")
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        if isinstance(msgs, tuple):                       # (blob uint8, off uint64 [n + 1]): a drained queue in one buffer
            blob, off = np.ascontiguousarray(msgs[0], dtype=np.uint8), np.ascontiguousarray(msgs[1], dtype=np.uint64)
            n = off.size - 1
            if n < 0 or (n and int(off[n]) > blob.size):
                raise ValueError("the offsets do not fit the blob")
        else:
            n = len(msgs)
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\x00", dtype=np.uint8)
        ours = None
        if our_id is not None:
            ours = np.frombuffer(bytes(our_id), dtype=np.uint8)
            if ours.size != 33:
                raise ValueError("a node id has 33 bytes")
        pid, stride = None, 0
        if peers is not None and n:
            if isinstance(peers, (bytes, bytearray)):
                pid = np.frombuffer(bytes(peers), dtype=np.uint8)
            else:
                if len(peers) != n:
                    raise ValueError("one peer per message")
                pid, stride = np.frombuffer(b"".join(bytes(33) if p is None else bytes(p) for p in peers), dtype=np.uint8), 33
            if pid.size != (33 if stride == 0 else 33 * n):
                raise ValueError("a node id has 33 bytes")
        hs = np.array(sorted(set(int(s) for s in held)) + [0], dtype=np.uint64)
        status, flags, chan = np.zeros(max(1, n), dtype=np.int8), np.zeros(max(1, n), dtype=np.uint8), np.zeros(max(1, n), dtype=np.uint32)
        # no plan is longer than the batch: one call, no sizing pass (it would run the signature batch twice)
        cap, nbytes = max(1, n), max(1, int(off[n] - off[0]) + 12 * n)
        add_msg, add_off = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64)
        del_rec, set_rec, set_ts, set_crc = (np.zeros(cap, dtype=np.uint32) for _ in range(4))
        out = np.zeros(nbytes, dtype=np.uint8) if host_out else None
        d_ptr = None
        if d_out is not None:
            if d_out.numel() < nbytes:
                raise ValueError("d_out must hold the messages and 12 bytes each")
            self._after_torch()
            d_ptr = d_out.data_ptr()
        s = _ffi.LamdUpdateReceiveSummary()
        self._chk(self._lib.lamd_channel_update_receive_batch(
            self._ctx, digest._h, directory._h, chain.ctypes.data, int(now), int(prune_interval), None if ours is None else ours.ctypes.data, n,
            blob.ctypes.data, off.ctypes.data, None if pid is None else pid.ctypes.data, stride, hs.size - 1, hs.ctypes.data if hs.size > 1 else None,
            status.ctypes.data, flags.ctypes.data, chan.ctypes.data, cap, add_msg.ctypes.data, add_off.ctypes.data,
            None if out is None else out.ctypes.data, d_ptr, nbytes, cap, del_rec.ctypes.data, set_rec.ctypes.data, set_ts.ctypes.data, set_crc.ctypes.data,
            ctypes.byref(s)))
        plan = dict(add_msg=add_msg[:s.adds], add_off=add_off[:s.adds], records=None if out is None else out[:s.bytes].tobytes(), del_rec=del_rec[:s.deletions],
                    set_rec=set_rec[:s.retimestamps], set_ts=set_ts[:s.retimestamps], set_crc=set_crc[:s.retimestamps])
        res = (status[:n], flags[:n], chan[:n], plan)
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    def node_announcement_receive(self, directory, msgs, pending=False, d_out=None, host_out=True, return_summary=False):
        """lamd_node_announcement_receive_batch: a drained queue of raw node_announcement messages received against the image a StoreDirectory
        was built from (by this Engine): framing, TLV tail and address descriptors, ONE signature batch under each message's own node_id, "newer
        wins" in arrival order.  msgs: a list of messages, or (blob uint8, off uint64 [n + 1]): message i = blob[off[i]:off[i + 1]].  pending: the
        caller's pending or too-early channel_announcement maps are not empty (an unknown node's message is held, not refused); d_out: a torch
        uint8 CUDA tensor the added records are written to (at its data pointer, any alignment) instead of, or with host_out besides, the host.
        -> (status int8 [msgs] (0 accepted, -1 malformed, 1 malformed addresses, 2 bad signature, 3 held, 4 unknown node, 5 stale, 6 duplicate),
        flags uint8 [msgs] (1 SUPERSEDED, 4 DYING), node uint32 [msgs] (the rank in the directory, 0xFFFFFFFF: none), plan): plan = dict(add_msg
        uint32 [adds], add_off uint64 [adds], records bytes or None (without host_out), del_rec uint32 ascending, set_rec / set_ts / set_crc: empty
        uint32 arrays -- nothing is re-stamped) -- apply_update_plan() applies it to the image"""
        if isinstance(msgs, tuple):                       # (blob uint8, off uint64 [n + 1]): a drained queue in one buffer
            blob, off = np.ascontiguousarray(msgs[0], dtype=np.uint8), np.ascontiguousarray(msgs[1], dtype=np.uint64)
            n = off.size - 1
            if n < 0 or (n and int(off[n]) > blob.size):
                raise ValueError("the offsets do not fit the blob")
        else:
            n = len(msgs)
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\x00", dtype=np.uint8)
        status, flags, node = np.zeros(max(1, n), dtype=np.int8), np.zeros(max(1, n), dtype=np.uint8), np.zeros(max(1, n), dtype=np.uint32)
        # no plan is longer than the batch: one call, no sizing pass (it would run the signature batch twice)
        cap, nbytes = max(1, n), max(1, int(off[n] - off[0]) + 12 * n)
        add_msg, add_off, del_rec = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        out = np.zeros(nbytes, dtype=np.uint8) if host_out else None
        d_ptr = None
        if d_out is not None:
            if d_out.numel() < nbytes:
                raise ValueError("d_out must hold the messages and 12 bytes each")
            self._after_torch()
            d_ptr = d_out.data_ptr()
        s = _ffi.LamdNodeReceiveSummary()
        self._chk(self._lib.lamd_node_announcement_receive_batch(
            self._ctx, directory._h, n, blob.ctypes.data, off.ctypes.data, int(bool(pending)), status.ctypes.data, flags.ctypes.data, node.ctypes.data,
            cap, add_msg.ctypes.data, add_off.ctypes.data, None if out is None else out.ctypes.data, d_ptr, nbytes, cap, del_rec.ctypes.data, ctypes.byref(s)))
        none = np.zeros(0, dtype=np.uint32)
        plan = dict(add_msg=add_msg[:s.adds], add_off=add_off[:s.adds], records=None if out is None else out[:s.bytes].tobytes(), del_rec=del_rec[:s.deletions],
                    set_rec=none, set_ts=none.copy(), set_crc=none.copy())
        res = (status[:n], flags[:n], node[:n], plan)
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    @staticmethod
    def _msg_blob(msgs):
        """a list of messages, or (blob uint8, off uint64 [n + 1]) -> (blob, off, n)"""
        if isinstance(msgs, tuple):
            blob, off = np.ascontiguousarray(msgs[0], dtype=np.uint8), np.ascontiguousarray(msgs[1], dtype=np.uint64)
            n = off.size - 1
            if n < 0 or (n and int(off[n]) > blob.size):
                raise ValueError("the offsets do not fit the blob")
            return blob, off, n
        n = len(msgs)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        return np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\x00", dtype=np.uint8), off, n

    def channel_announcement_receive(self, digest, msgs, chain_hash, blockheight, held=(), failed=(), return_summary=False):
        """lamd_channel_announcement_receive_batch: a drained queue of raw channel_announcement messages received against the digest of a store
        image (built by this Engine): framing, the filters, ONE signature batch with four rows per message that passed them, the bitcoin keys alone
        of the others, "already pending from this batch" in arrival order, the funding scripts.  msgs: a list of messages, or (blob uint8, off
        uint64 [n + 1]).  blockheight 0: unknown.  held: the scids of the caller's pending and too-early maps, failed: of its txout failures.
        -> (status int8 [msgs] (0 pending: ask lightningd, -1 malformed, 1 node ids not ordered, 2 foreign chain, 3 txout failed before, 4 known,
        5 .. 8 the first bad signature, 9 bad gossip order, 10 already pending from this batch, 11 early), scid uint64 [msgs] (0: malformed),
        spk uint8 [msgs, 34] (the expected scriptpubkey for the statuses 0 and 11, zeros otherwise), asks = dict(msg uint32 [asks], scid uint64
        [asks]): the get_txout requests in arrival order)"""
        chain = np.frombuffer(bytes(chain_hash), dtype=np.uint8)
        if chain.size != 32:
            raise ValueError("the chain_hash has 32 bytes")
        blob, off, n = self._msg_blob(msgs)
        hs = np.array(sorted(set(int(s) for s in held)) + [0], dtype=np.uint64)
        fs = np.array(sorted(set(int(s) for s in failed)) + [0], dtype=np.uint64)
        cap = max(1, n)
        status, scid, spk = np.zeros(cap, dtype=np.int8), np.zeros(cap, dtype=np.uint64), np.zeros((cap, 34), dtype=np.uint8)
        ask_msg, ask_scid = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64)
        s = _ffi.LamdAnnounceReceiveSummary()
        self._chk(self._lib.lamd_channel_announcement_receive_batch(
            self._ctx, digest._h, chain.ctypes.data, int(blockheight), n, blob.ctypes.data, off.ctypes.data, hs.size - 1, hs.ctypes.data, fs.size - 1,
            fs.ctypes.data, status.ctypes.data, scid.ctypes.data, spk.ctypes.data, cap, ask_msg.ctypes.data, ask_scid.ctypes.data, ctypes.byref(s)))
        res = (status[:n], scid[:n], spk[:n], dict(msg=ask_msg[:s.asks], scid=ask_scid[:s.asks]))
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    def channel_announcement_confirm(self, digest, directory, pending_msgs, pending_spk, replies, d_out=None, host_out=True, return_summary=False):
        """lamd_channel_announcement_confirm_batch: lightningd's txout replies against the caller's pending announcements and the digest and
        directory of the image as it is now.  pending_msgs: the raw announcements STRICTLY ASCENDING by scid (a list, or (blob, off)); pending_spk:
        their scripts from channel_announcement_receive, uint8 [pending, 34]; replies: a list of (scid, sat, script bytes) in arrival order, or the four
        arrays GossipIngest.txout_reply_batch takes (scid, sat, scripts, script_off).
        -> (status int8 [replies] (0 accepted, 1 nothing pending, 2 no unspent output, 3 another script, 4 redundant), pend uint32 [replies] (the
        pending message consumed, 0xFFFFFFFF: none), fail_scid uint64 (the statuses 2 and 3: the caller's new txout failures), plan): plan =
        dict(add_reply uint32 [adds], add_off uint64 [2 adds] (the offset of EVERY record: the announcement and the channel_amount of each accepted
        reply), records bytes or None (without host_out), clr_rec uint32 ascending (node_announcement headers whose DYING bit is cleared),
        del_rec / set_rec / set_ts / set_crc: empty) -- apply_update_plan() applies it to the image"""
        blob, off, np_ = self._msg_blob(pending_msgs)
        pspk = np.ascontiguousarray(pending_spk, dtype=np.uint8).reshape(-1)
        if pspk.size != 34 * np_:
            raise ValueError("one 34-byte script per pending announcement")
        pspk = np.concatenate([pspk, np.zeros(1, dtype=np.uint8)])
        if isinstance(replies, tuple):                    # (scid uint64 [nr], sat uint64 [nr], scripts uint8, script_off uint64 [nr + 1]): as txout_reply_batch takes them
            r_scid, r_sat = (np.concatenate([np.asarray(a, dtype=np.uint64), np.zeros(1, dtype=np.uint64)]) for a in replies[:2])
            scripts, soff = np.ascontiguousarray(replies[2], dtype=np.uint8), np.ascontiguousarray(replies[3], dtype=np.uint64)
            nr = soff.size - 1
            if nr < 0 or r_scid.size != nr + 1 or r_sat.size != nr + 1 or (nr and int(soff[nr]) > scripts.size):
                raise ValueError("the replies' arrays do not fit each other")
            scripts = np.concatenate([scripts, np.zeros(1, dtype=np.uint8)])
        else:
            nr = len(replies)
            r_scid = np.array([int(r[0]) for r in replies] + [0], dtype=np.uint64)
            r_sat = np.array([int(r[1]) for r in replies] + [0], dtype=np.uint64)
            soff = np.zeros(nr + 1, dtype=np.uint64)
            soff[1:] = np.cumsum([len(r[2]) for r in replies], dtype=np.uint64)
            scripts = np.frombuffer(b"".join(bytes(r[2]) for r in replies) + b"\x00", dtype=np.uint8)
        # a pending message is appended once at most: its bytes, two headers and the amount (d_out must hold this much)
        cap, nbytes = max(1, nr), max(1, int(off[np_] - off[0]) + 34 * min(nr, np_))
        status, pend = np.zeros(cap, dtype=np.int8), np.zeros(cap, dtype=np.uint32)
        add_reply, add_off, fail_scid, clr_rec = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(2 * cap, dtype=np.uint32)
        out = np.zeros(nbytes, dtype=np.uint8) if host_out else None
        d_ptr = None
        if d_out is not None:
            if d_out.numel() < nbytes:
                raise ValueError("d_out must hold the pending messages and 34 bytes per reply")
            self._after_torch()
            d_ptr = d_out.data_ptr()
        s = _ffi.LamdAnnounceConfirmSummary()
        self._chk(self._lib.lamd_channel_announcement_confirm_batch(
            self._ctx, digest._h, directory._h, np_, blob.ctypes.data, off.ctypes.data, pspk.ctypes.data, nr, r_scid.ctypes.data, r_sat.ctypes.data,
            scripts.ctypes.data, soff.ctypes.data, status.ctypes.data, pend.ctypes.data, cap, add_reply.ctypes.data, add_off.ctypes.data,
            None if out is None else out.ctypes.data, d_ptr, nbytes, cap, fail_scid.ctypes.data, 2 * cap, clr_rec.ctypes.data, ctypes.byref(s)))
        none = np.zeros(0, dtype=np.uint32)
        first = add_off[:s.adds]
        took = pend[add_reply[:s.adds]].astype(np.int64)
        lens = (off[took + 1] - off[took]).astype(np.uint64)
        both = np.stack([first, first + np.uint64(12) + lens], axis=1).reshape(-1) if s.adds else np.zeros(0, dtype=np.uint64)
        plan = dict(add_reply=add_reply[:s.adds], add_off=both, records=None if out is None else out[:s.bytes].tobytes(), clr_rec=clr_rec[:s.clears],
                    del_rec=none, set_rec=none.copy(), set_ts=none.copy(), set_crc=none.copy())
        res = (status[:nr], pend[:nr], fail_scid[:s.failures], plan)
        if return_summary:
            res += ({k: (list(getattr(s, k)) if k in ("stage_ms", "by_status") else int(getattr(s, k))) for k, _ in s._fields_},)
        return res

    # ---- single-item veneers (reference semantics)
    def check_signed_hash(self, hash32, sig64, pubkey):
        return bool(self._chk(self._lib.lamd_check_signed_hash(self._ctx, bytes(hash32), bytes(sig64), bytes(pubkey), len(pubkey))))

    def check_signed_hash_nodeid(self, hash32, sig64, node_id33):
        return bool(self._chk(self._lib.lamd_check_signed_hash_nodeid(self._ctx, bytes(hash32), bytes(sig64), bytes(node_id33))))

    def check_schnorr_sig(self, hash32, pubkey33, sig64):
        return bool(self._chk(self._lib.lamd_check_schnorr_sig(self._ctx, bytes(hash32), bytes(pubkey33), bytes(sig64))))

    # ---- streaming
    def queue_ecdsa(self, hash32, sig64, pubkey):
        return self._chk(self._lib.lamd_queue_ecdsa(self._ctx, bytes(hash32), bytes(sig64), bytes(pubkey), len(pubkey)))

    def queue_schnorr(self, msg32, xonly32, sig64):
        return self._chk(self._lib.lamd_queue_schnorr(self._ctx, bytes(msg32), bytes(xonly32), bytes(sig64)))

    def queue_ecdsa_batch(self, hash32, sig64, pub):
        """numpy uint8 [n,32], [n,64], [n,33|65]: first ticket"""
        hash32, sig64 = _u8(hash32, 32), _u8(sig64, 64)
        pub = np.ascontiguousarray(pub, dtype=np.uint8)
        return self._chk(self._lib.lamd_queue_ecdsa_batch(self._ctx, hash32.shape[0], hash32.ctypes.data, sig64.ctypes.data, pub.ctypes.data,
                                                          pub.shape[1], pub.shape[1]))

    def queue_schnorr_batch(self, msg32, xonly32, sig64):
        msg32, xonly32, sig64 = _u8(msg32, 32), _u8(xonly32, 32), _u8(sig64, 64)
        return self._chk(self._lib.lamd_queue_schnorr_batch(self._ctx, msg32.shape[0], msg32.ctypes.data, xonly32.ctypes.data, sig64.ctypes.data))

    def queue_reserve(self, n, keylen):
        """zero-copy producer form: (first ticket, hash/msg [n,32], sig [n,64], key [n,keylen]) -- numpy views of the pinned staging
        set, to be filled before flush() and not kept beyond the next queue_* / flush call"""
        ptr = [ctypes.c_void_p() for _ in range(3)]
        first = self._chk(self._lib.lamd_queue_reserve(self._ctx, int(n), int(keylen), *[ctypes.byref(p) for p in ptr]))
        views = [np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(int(n), w)) for p, w in zip(ptr, (32, 64, int(keylen)))]
        return (first, *views)

    def queue_ecdsa_batch_inplace(self, hash32, sig64, pub):
        """the rows are NOT copied: C-contiguous numpy uint8 [n,32], [n,64], [n,33|65] that the caller keeps alive and unchanged until the flush
        carrying them has been collected (wait / poll); pin them with host_register() for DMA.  First ticket."""
        for a, w in ((hash32, 32), (sig64, 64)):
            if a.dtype != np.uint8 or not a.flags.c_contiguous or a.ndim != 2 or a.shape[1] != w:
                raise ValueError("in-place rows must be C-contiguous uint8 [n,%d]" % w)
        if pub.dtype != np.uint8 or not pub.flags.c_contiguous or pub.ndim != 2 or pub.shape[0] != hash32.shape[0] or sig64.shape[0] != hash32.shape[0]:
            raise ValueError("in-place keys must be C-contiguous uint8 [n,33|65]")
        return self._chk(self._lib.lamd_queue_ecdsa_batch_inplace(self._ctx, hash32.shape[0], hash32.ctypes.data, sig64.ctypes.data, pub.ctypes.data, pub.shape[1]))

    def queue_schnorr_batch_inplace(self, msg32, xonly32, sig64):
        for a, w in ((msg32, 32), (xonly32, 32), (sig64, 64)):
            if a.dtype != np.uint8 or not a.flags.c_contiguous or a.ndim != 2 or a.shape[1] != w or a.shape[0] != msg32.shape[0]:
                raise ValueError("in-place rows must be C-contiguous uint8 [n,%d]" % w)
        return self._chk(self._lib.lamd_queue_schnorr_batch_inplace(self._ctx, msg32.shape[0], msg32.ctypes.data, xonly32.ctypes.data, sig64.ctypes.data))

    def host_register(self, arr):
        """pins a numpy array's memory for every device (rows queued in place leave it by DMA); False when the runtime refuses the range"""
        return self._lib.lamd_host_register(self._ctx, arr.ctypes.data, arr.nbytes) == 0

    def host_unregister(self, arr):
        return self._lib.lamd_host_unregister(self._ctx, arr.ctypes.data) == 0

    def flush(self):
        self._chk(self._lib.lamd_flush(self._ctx))

    def wait(self, cap=1 << 20):
        ok = np.zeros(cap, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        self._chk(self._lib.lamd_wait(self._ctx, ok.ctypes.data, cap, ctypes.byref(n)))
        return _verdicts(ok[:n.value])

    def poll(self, cap=1 << 20):
        ok = np.zeros(cap, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        rc = self._chk(self._lib.lamd_poll(self._ctx, ok.ctypes.data, cap, ctypes.byref(n)))
        return _verdicts(ok[:n.value]) if rc == 1 else None

    # ---- device-resident API (torch uint8 CUDA tensors; asynchronous on self.stream_ptr)
    def verify_ecdsa_device(self, d_hash, d_sig, d_pub, d_ok):
        n, publen = d_pub.shape
        self._after_torch()
        self._chk(self._lib.lamd_verify_ecdsa_batch_device(self._ctx, n, d_hash.data_ptr(), d_sig.data_ptr(), d_pub.data_ptr(),
                                                           publen, publen, d_ok.data_ptr()))

    def verify_schnorr_device(self, d_msg, d_xonly, d_sig, d_ok):
        n = d_msg.shape[0]
        self._after_torch()
        self._chk(self._lib.lamd_verify_schnorr_batch_device(self._ctx, n, d_msg.data_ptr(), d_xonly.data_ptr(), d_sig.data_ptr(),
                                                             d_ok.data_ptr()))

    def gen_ecdsa_device(self, seed, nkeys, d_hash, d_sig, d_pub, group=0):
        n, publen = d_pub.shape
        self._after_torch()   # the output tensors may still be being filled on torch's stream (torch.zeros)
        self._chk(_ffi.load_testgen().lamd_gen_ecdsa_device(self._ctx, n, seed, nkeys, group, publen, d_hash.data_ptr(), d_sig.data_ptr(), d_pub.data_ptr()))

    def gen_schnorr_device(self, seed, nkeys, d_msg, d_xonly, d_sig, group=0):
        n = d_msg.shape[0]
        self._after_torch()
        self._chk(_ffi.load_testgen().lamd_gen_schnorr_device(self._ctx, n, seed, nkeys, group, d_msg.data_ptr(), d_xonly.data_ptr(), d_sig.data_ptr()))

    def gen_gossip_device(self, seed, n_cann, n_cupd, n_nodes, d_msgs, d_ids):
        self._after_torch()
        self._chk(_ffi.load_testgen().lamd_gen_gossip_device(self._ctx, n_cann, n_cupd, seed, n_nodes, d_msgs.data_ptr(), d_ids.data_ptr()))

    def sigcheck_gossip_device(self, n, d_msgs, d_off, d_ids, d_rowbase, rows, d_verdict):
        self._after_torch()
        self._chk(self._lib.lamd_sigcheck_gossip_batch_device(self._ctx, n, d_msgs.data_ptr(), d_off.data_ptr(),
                                                              d_ids.data_ptr() if d_ids is not None else None, d_rowbase.data_ptr(), rows,
                                                              d_verdict.data_ptr()))

    def sigcheck_gossip_spans_device(self, n, d_msgs, d_start, d_len, d_ids, d_rowbase, rows, d_verdict):
        """lamd_sigcheck_gossip_spans_device: message i = d_msgs[d_start[i] : d_start[i] + d_len[i]]; ids / rowbase / verdicts index the selection"""
        self._after_torch()
        self._chk(self._lib.lamd_sigcheck_gossip_spans_device(self._ctx, n, d_msgs.data_ptr(), d_start.data_ptr(), d_len.data_ptr(),
                                                              d_ids.data_ptr() if d_ids is not None else None, d_rowbase.data_ptr(), rows,
                                                              d_verdict.data_ptr()))

    def selftest(self, hash32, sig64, pub33):
        buf = ctypes.create_string_buffer(4096)
        rc = self._chk(self._lib.lamd_selftest(self._ctx, bytes(hash32), bytes(sig64), bytes(pub33), buf, 4096))
        return rc, buf.value.decode()

    def chain_debug(self, use_mul):
        buf = ctypes.create_string_buffer(8192)
        rc = self._chk(self._lib.lamd_chain_debug(self._ctx, int(use_mul), buf, 8192))
        return rc, buf.value.decode()

    def inv_debug(self):
        buf = ctypes.create_string_buffer(8192)
        rc = self._chk(self._lib.lamd_inv_debug(self._ctx, buf, 8192))
        return rc, buf.value.decode()

    def fuzz_field(self, lanes=16384, iters=64, seed=1):
        """(mismatching lanes, field operations executed on the device, report)"""
        buf = ctypes.create_string_buffer(4096)
        ops = ctypes.c_uint64(0)
        rc = self._chk(self._lib.lamd_fuzz_field(self._ctx, lanes, iters, seed, ctypes.byref(ops), buf, 4096))
        return rc, ops.value, buf.value.decode()

    # lamd_debug_read's buffers that tests name
    READ_POOL7, READ_GTABLE, READ_POOL10, READ_CACHE_ENTS = 8, 9, 10, 11
    GTABLE_ENTRIES, GTABLE_ENTRY_BYTES = 11 << 24, 64

    def debug_read(self, which, offset, nbytes):
        """lamd_debug_read: nbytes at offset of internal buffer `which` (include/lightning_amd_debug.h) as numpy uint8"""
        out = np.zeros(max(1, nbytes), dtype=np.uint8)
        self._chk(self._lib.lamd_debug_read(self._ctx, int(which), offset, nbytes, out.ctypes.data))
        return out[:nbytes]

    def gtable_audit(self, first, count, image=None):
        """lamd_debug_gtable_audit over the entries [first, first + count) of the static G table; image: a torch uint8 / int32 device tensor of
        exactly count * 64 bytes that replaces the range.  -> dict(bad, first_bad, first_reason, listed=[(index, reason), ...] (at most 64))"""
        ptr = None
        if image is not None:
            if image.numel() * image.element_size() != count * self.GTABLE_ENTRY_BYTES or not image.is_contiguous():
                raise ValueError("image must hold exactly count entries of 64 bytes")
            import torch
            torch.cuda.current_stream().synchronize()      # a diagnostic: the image is complete before the audit reads it
            ptr = image.data_ptr()
        r = _ffi.LamdGtableAuditResult()
        self._chk(self._lib.lamd_debug_gtable_audit(self._ctx, first, count, ptr, ctypes.byref(r)))
        return dict(bad=int(r.bad), first_bad=int(r.first_bad) if r.bad else None, first_reason=int(r.first_reason),
                    listed=sorted((int(r.list_index[i]), int(r.list_reason[i])) for i in range(r.n_list)))

    def synchronize(self):
        self._chk(self._lib.lamd_synchronize(self._ctx))

    @property
    def stream_ptr(self):
        return self._lib.lamd_stream(self._ctx)

    def set_timing(self, on=True):
        self._chk(self._lib.lamd_set_timing(self._ctx, int(on)))

    def set_ecmult_chain(self, on):
        """large table-driven ecmult launches one after the other (True) or overlapping (False, default): lamd_set_ecmult_chain"""
        self._chk(self._lib.lamd_set_ecmult_chain(self._ctx, int(on)))

    def stream_wait_results(self, stream_ptr):
        """make a caller's HIP stream wait (on the device) for every verification submitted so far"""
        self._chk(self._lib.lamd_stream_wait_results(self._ctx, ctypes.c_void_p(stream_ptr)))

    def wait_event(self, event_ptr):
        """verification submitted from now on waits (on the device) for a hipEvent_t the caller recorded"""
        self._chk(self._lib.lamd_wait_event(self._ctx, ctypes.c_void_p(event_ptr)))

    def results_mark(self, slot):
        """remember "everything submitted so far" in slot 0..3 (no waiting); see stream_wait_mark"""
        self._chk(self._lib.lamd_results_mark(self._ctx, int(slot)))

    def results_mark_last(self, slot):
        """lamd_results_mark_last: one event, on the lane of the call submitted last"""
        self._chk(self._lib.lamd_results_mark_last(self._ctx, slot))

    def stream_wait_mark(self, slot, stream_ptr):
        """make a caller's HIP stream wait (on the device) for the work remembered by results_mark(slot)"""
        self._chk(self._lib.lamd_stream_wait_mark(self._ctx, int(slot), ctypes.c_void_p(stream_ptr)))

    def wait_stream(self, stream_ptr):
        """verification submitted from now on waits (on the device) for what the caller's stream holds now"""
        self._chk(self._lib.lamd_wait_stream(self._ctx, ctypes.c_void_p(stream_ptr)))

    def info(self, lane=None):
        inf = _ffi.LamdInfo()
        if lane is None:
            self._chk(self._lib.lamd_get_info(self._ctx, ctypes.byref(inf)))
        else:
            self._chk(self._lib.lamd_get_lane_info(self._ctx, int(lane), ctypes.byref(inf)))
        return dict(device=inf.device, compute_units=inf.compute_units, arch=inf.arch.decode(), gtable_bytes=inf.gtable_bytes,
                    last_kernel_ms=list(inf.last_kernel_ms), last_unique_keys=inf.last_unique_keys, last_hot_rows=inf.last_hot_rows, last_keyed=int(inf.last_keyed), last_mode=int(inf.last_mode), lanes=int(inf.lanes),
                    last_cache_hits=inf.last_cache_hits, last_cold_rows=inf.last_cold_rows, last_new_tables=inf.last_new_tables,
                    last_suspect_rows=inf.last_suspect_rows, cache_enabled=bool(inf.cache_enabled), cache_entries=inf.cache_entries,
                    cache_capacity=inf.cache_capacity, cache_resets=inf.cache_resets,
                    keyed_ecmult_ms_sum=list(inf.keyed_ecmult_ms_sum), keyed_ecmult_launches=list(inf.keyed_ecmult_launches), hw_queues_env=int(inf.hw_queues_env), queue_sets=int(inf.queue_sets),
                    last_flush_inplace_rows=int(inf.last_flush_inplace_rows), last_text_ms=list(inf.last_text_ms))

    def set_chunk_rows(self, rows):
        """lamd_set_chunk_rows: rows per launch sequence of the calls that follow (0 = default 2^22)"""
        self._chk(self._lib.lamd_set_chunk_rows(self._ctx, rows))

    def mul32_peak(self, waves_per_simd=3, min_ms=4.0, launches=5):
        """lamd_debug_mul32_peak: sustained v_mad_u64_u32 rate of the chip (lane-ops/s), average launch ms, s_memtime / s_memrealtime ratio"""
        r, ms, ck = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._chk(self._lib.lamd_debug_mul32_peak(self._ctx, waves_per_simd, min_ms, launches, ctypes.byref(r), ctypes.byref(ms), ctypes.byref(ck)))
        return r.value, ms.value, ck.value

    def cache_clear(self):
        """empty the key-table cache (cold-path measurements)"""
        self._chk(self._lib.lamd_cache_clear(self._ctx))

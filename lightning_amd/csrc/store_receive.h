// Receiving channel_update batches against a store image: the per-message, per-row and per-output-word logic of
// lamd_channel_update_receive_batch (include/lightning_amd.h), as inline functions that compile for gfx950 and, unchanged, for the host
// (tests/c/store_receive_host.cpp runs them under the sanitizers).
//   - the classification of a raw message in the order of gossmap_manage_channel_update() (gossipd/gossmap_manage.c:1010-1120): framing and
//     the signature's range (wire/fromwire.c:196-198), chain, timestamp_reasonable() (:997-1008), the held scids, gossmap_find_chan as two
//     bisections in the digest's entries and in the bare list, the signer -- node_id_1 / node_id_2 of the channel's announcement in the image,
//     or the source peer's id for an unknown channel (:1101-1110);
//   - what the signature's verdict makes of it (process_channel_update(), :900-932), and the sort key of a candidate: 2 * channel + direction;
//   - "newer wins, first among equals" (:935-951) over the candidates sorted by slot, arrival order kept inside a slot: the running
//     maximum of (slot << 33) | (ts + 1) tells each row the timestamp in force in front of it;
//   - the plan: one store record per accepted message (gossip_store.c:49-78), the records the slots held before, the announcements
//     whose header is re-stamped (:655-670);
//   - the encoder of the added records, one aligned 32-bit word of the OUTPUT at a time.
// Every read of the image stays inside [store, store + store_len), every read of the batch inside its messages.
#pragma once
#include "store_stream.h"

namespace lamd {

enum {
  STORE_RX_MALFORMED = -1, STORE_RX_ACCEPTED = 0, STORE_RX_WRONG_CHAIN = 1, STORE_RX_TIMESTAMP = 2, STORE_RX_HELD = 3, STORE_RX_PRIVATE = 4,
  STORE_RX_UNKNOWN = 5, STORE_RX_BAD_SIGNATURE = 6, STORE_RX_DONT_FORWARD = 7, STORE_RX_STALE = 8, STORE_RX_DUPLICATE = 9,
  STORE_RX_PENDING = 100   // between the stages: the message has a signature row (or, behind it, is a candidate)
};
constexpr u32 STORE_RX_SUPERSEDED = 1, STORE_RX_FIRST = 2, STORE_RX_DYING = 4, STORE_RX_PEER_UPDATE = 8;
constexpr u32 STORE_RX_MIN = 138, STORE_RX_MAX = 65535;   // every fixed field of a channel_update; the longest wire message
constexpr u64 STORE_RX_PAD = ~(u64)0;                      // the sort key of a message that is no candidate
constexpr u64 STORE_RX_TS_MASK = ((u64)1 << 33) - 1;       // ts + 1 of a scan item; 0 there: no timestamp
constexpr u64 STORE_RX_MAX_CHANNELS = (u64)1 << 30;        // so that (slot << 33) | (ts + 1) stays below the pads' all-ones
enum { STORE_RX_SIGNER_NONE = 0, STORE_RX_SIGNER_IMAGE = 1, STORE_RX_SIGNER_PEER = 2, STORE_RX_SIGNER_NO_KEY = 3 };

// the digest and the directory as the receive path reads them: channel c < count is entry c, channel count + j is bare channel j
struct store_rx_view {
  const u8 *store; size_t store_len; const u64 *rec_off; u32 n_rec;
  const u64 *scid; u32 count, nbare;        // the entries' scids, then the bare ones: each part ascending
  const u32 *ent_rec, *bare_rec, *ts;       // 3 records per entry (announcement, update 0, update 1); one per bare channel; 2 signed timestamps per entry
};
struct store_rx_params { u64 now; u32 prune, have_our; u8 chain[32], our_id[33]; };
// the batch: message i = msgs[off[i], off[i + 1]); peers: the id of message i's source at peers + i * peer_stride, nullptr: none has one
struct store_rx_batch { const u8 *msgs; const u64 *off; u32 n; const u8 *peers; u64 peer_stride; const u64 *held; u32 n_held; };
struct store_rx_msg { int32_t status; u32 chan, ts, signer; u64 idoff; u32 dir, dont_forward; };

// the group order n, most significant word first
LAMD_HD u32 store_rx_n_word(u32 k) {
  return k < 3 ? 0xFFFFFFFFu : k == 3 ? 0xFFFFFFFEu : k == 4 ? 0xBAAEDCE6u : k == 5 ? 0xAF48A03Bu : k == 6 ? 0xBFD25E8Cu : 0xD0364141u;
}
LAMD_HD bool store_rx_ge_n(const u8 *p) {   // the 32 big-endian bytes at p, at any alignment, are >= n
  for (u32 k = 0; k < 8; k++) {
    const u32 w = store_be32(p + 4 * k), nw = store_rx_n_word(k);
    if (w != nw) return w > nw;
  }
  return true;
}
// the announcement record of channel c, STORE_NONE: none
LAMD_HD u32 store_rx_ann(const store_rx_view &v, u32 c) {
  if (c < v.count) return v.ent_rec[3 * (size_t)c];
  return c - v.count < v.nbare ? v.bare_rec[c - v.count] : STORE_NONE;
}
// the record slot (c, d) holds in the image, STORE_NONE: none; and its signed timestamp
LAMD_HD u32 store_rx_slot_rec(const store_rx_view &v, u32 c, u32 d) { return c < v.count ? v.ent_rec[3 * (size_t)c + 1 + d] : STORE_NONE; }

// ---- stage 1, every message: statuses -1 .. 3 and 5 (an unknown channel without a peer) are final, everything else is PENDING and gets a
// signature row
LAMD_HD store_rx_msg store_rx_classify(const store_rx_view &v, const store_rx_params &p, const store_rx_batch &b, u32 i) {
  store_rx_msg r;
  r.status = STORE_RX_MALFORMED;
  r.chan = STORE_NONE;
  r.ts = r.dir = r.dont_forward = 0;
  r.signer = STORE_RX_SIGNER_NONE;
  r.idoff = 0;
  const u64 len = b.off[i + 1] - b.off[i];
  const u8 *m = b.msgs + b.off[i];
  if (len < STORE_RX_MIN || len > STORE_RX_MAX || store_be16(m) != STORE_T_CUPD || store_rx_ge_n(m + 2) || store_rx_ge_n(m + 34)) return r;
  u32 diff = 0;
  for (u32 k = 0; k < 32; k++) diff |= (u32)(m[66 + k] ^ p.chain[k]);
  if (diff) { r.status = STORE_RX_WRONG_CHAIN; return r; }
  r.ts = store_be32(m + 106);
  if ((u64)r.ts > p.now + 86400 || (u64)r.ts < p.now - p.prune) { r.status = STORE_RX_TIMESTAMP; return r; }   // u64 as the reference: now < prune wraps
  const u64 scid = store_be64(m + 98);
  if (b.n_held && store_cmp_find(b.held, b.n_held, scid) != STORE_NONE) { r.status = STORE_RX_HELD; return r; }
  r.dont_forward = (m[110] >> 1) & 1;
  r.dir = m[111] & 1;
  u32 c = store_cmp_find(v.scid, v.count, scid);
  if (c == STORE_NONE) {
    const u32 j = store_cmp_find(v.scid + v.count, v.nbare, scid);
    if (j != STORE_NONE) c = v.count + j;
  }
  if (c == STORE_NONE) {
    r.status = b.peers ? STORE_RX_PENDING : STORE_RX_UNKNOWN;
    r.signer = b.peers ? STORE_RX_SIGNER_PEER : STORE_RX_SIGNER_NONE;
    return r;
  }
  r.chan = c;
  r.status = STORE_RX_PENDING;
  const u32 a = store_rx_ann(v, c);
  r.signer = a < v.n_rec && store_dir_cann_ids(v.store, v.store_len, v.rec_off[a], &r.idoff) ? STORE_RX_SIGNER_IMAGE : STORE_RX_SIGNER_NO_KEY;
  return r;
}
// the row of a PENDING message: its span in the batch, its signer (zeros: a channel whose announcement is cut off in front of its ids --
// no valid key, the signature fails), the message it belongs to
LAMD_HD void store_rx_row(const store_rx_view &v, const store_rx_batch &b, const store_rx_msg &r, u32 i, u32 row, u64 *start, u64 *len, u8 *ids33,
                          u32 *row_msg) {
  start[row] = b.off[i];
  len[row] = b.off[i + 1] - b.off[i];
  row_msg[row] = i;
  const u8 *id = r.signer == STORE_RX_SIGNER_IMAGE ? v.store + r.idoff + 33 * r.dir : r.signer == STORE_RX_SIGNER_PEER ? b.peers + b.peer_stride * i : nullptr;
  for (u32 k = 0; k < 33; k++) ids33[33 * (size_t)row + k] = id ? id[k] : 0;
}

// ---- stage 2, every message, behind the signature batch (sigv: 0 = the signature verifies): statuses 4 .. 7 are final; a candidate stays
// PENDING and returns its slot, everything else STORE_RX_PAD
LAMD_HD u64 store_rx_settle(int8_t *status, u8 *flags, const u32 *chan, const u8 *aux, const u32 *row_of, const int8_t *sigv, u32 i) {
  if (status[i] != STORE_RX_PENDING) return STORE_RX_PAD;
  const bool ok = sigv[row_of[i]] == 0;
  if (chan[i] == STORE_NONE) {
    status[i] = ok ? STORE_RX_PRIVATE : STORE_RX_UNKNOWN;
    if (ok) flags[i] = (u8)STORE_RX_PEER_UPDATE;
    return STORE_RX_PAD;
  }
  if (!ok) { status[i] = STORE_RX_BAD_SIGNATURE; return STORE_RX_PAD; }
  if (aux[i] & 2) { status[i] = STORE_RX_DONT_FORWARD; return STORE_RX_PAD; }
  return 2 * (u64)chan[i] + (aux[i] & 1);
}
// the scan item of sorted position p: the pads behind the candidates carry the largest value, so the maximum stays monotone
LAMD_HD u64 store_rx_item(const u64 *key, const u32 *val, const u32 *ts, u32 p) {
  return key[p] == STORE_RX_PAD ? STORE_RX_PAD : (key[p] << 33) | ((u64)ts[val[p]] + 1);
}

// ---- stage 3, every sorted position.  key / val: the stable sort by slot (arrival order inside a slot), run: the inclusive maximum of the
// items.  The row in front tells a row its slot's maximum so far, or that it heads its slot; the image's record seeds the slot.
struct store_rx_sorted { const u64 *key; const u32 *val; const u64 *run; u32 n; };
// what stage 3 leaves per MESSAGE (all preset to 0 but del_key: all ones): count and size for the scans of the adds, the FIRST mark for the
// scan of the re-stamps, the record the message's slot held before
struct store_rx_marks { u32 *acnt, *abytes, *scnt, *del_key; };
// Returns whether the row deletes a record of the image.
LAMD_HD bool store_rx_resolve(const store_rx_view &v, const store_rx_params &pr, const store_rx_batch &b, const store_rx_sorted &s, const u32 *ts, u32 p,
                              int8_t *status, u8 *flags, const store_rx_marks &k) {
  const u64 key = s.key[p];
  if (key == STORE_RX_PAD) return false;
  const u32 i = s.val[p], c = (u32)(key >> 1), d = (u32)(key & 1);
  const u64 mine = (u64)ts[i] + 1, before = p ? s.run[p - 1] : 0;
  const u64 so_far = p && (before >> 33) == key ? before & STORE_RX_TS_MASK : 0;   // 0: the row heads its slot
  const u32 held = store_rx_slot_rec(v, c, d);
  const u64 seed = held != STORE_NONE ? (u64)v.ts[2 * (size_t)c + d] + 1 : 0;
  const u64 in_force = so_far > seed ? so_far : seed;
  if (mine <= in_force) {
    status[i] = (int8_t)(mine == in_force ? STORE_RX_DUPLICATE : STORE_RX_STALE);
    return false;
  }
  status[i] = STORE_RX_ACCEPTED;
  u32 f = 0;
  // the slot's last row carries its final maximum: a larger one than mine was accepted behind me
  const u32 end = store_sq_lower(s.key + p, s.n - p, key + 1) + p;
  if ((s.run[end - 1] & STORE_RX_TS_MASK) > mine) f |= STORE_RX_SUPERSEDED;
  // the first accepted row of a slot deletes what the slot held
  const bool deletes = held != STORE_NONE && so_far <= seed;
  if (deletes) k.del_key[i] = held;
  const u32 a = store_rx_ann(v, c);
  u64 idoff = 0;
  const bool ids = a < v.n_rec && store_dir_cann_ids(v.store, v.store_len, v.rec_off[a], &idoff);
  if (a < v.n_rec && v.rec_off[a] <= v.store_len && v.store_len - v.rec_off[a] >= STORE_HDR &&
      (store_read_hdr(v.store + v.rec_off[a]).flags & STORE_FLAG_DYING))
    f |= STORE_RX_DYING;
  if (ids && pr.have_our) {
    u32 diff = 0;
    for (u32 x = 0; x < 33; x++) diff |= (u32)(v.store[idoff + 33 * (1 - d) + x] ^ pr.our_id[x]);
    if (!diff) f |= STORE_RX_PEER_UPDATE;
  }
  // FIRST: both slots of the channel are empty in the image, the row heads its slot, and the other slot's head arrived later (or there is none)
  if (so_far == 0 && held == STORE_NONE && store_rx_slot_rec(v, c, 1 - d) == STORE_NONE) {
    const u32 q = store_sq_lower(s.key, s.n, key ^ 1);
    if (!(q < s.n && s.key[q] == (key ^ 1) && s.val[q] < i)) {
      f |= STORE_RX_FIRST;
      k.scnt[i] = 1;
    }
  }
  flags[i] = (u8)f;
  k.acnt[i] = 1;
  k.abytes[i] = (u32)(STORE_HDR + (b.off[i + 1] - b.off[i]));
  return deletes;
}

// ---- stage 4, every message: the plan.  apos / abyte / spos: the exclusive scans of the marks
struct store_rx_plan_out { u64 add_cap, edit_cap; u32 *add_msg; u64 *add_off; u32 *set_rec, *set_ts, *set_crc; };
template <int WAYS>
LAMD_HD void store_rx_plan(const u32 *T, const store_rx_view &v, const int8_t *status, const u8 *flags, const u32 *chan, const u32 *ts, const u64 *apos,
                           const u64 *abyte, const u64 *spos, const store_rx_plan_out &o, u32 i) {
  if (status[i] != STORE_RX_ACCEPTED) return;
  if (apos[i] < o.add_cap) {
    o.add_msg[apos[i]] = i;
    o.add_off[apos[i]] = abyte[i];
  }
  if (!(flags[i] & STORE_RX_FIRST) || spos[i] >= o.edit_cap) return;
  const u32 a = store_rx_ann(v, chan[i]);
  u32 len = 0;
  const u8 *m = a < v.n_rec ? store_live_msg(v.store, v.store_len, v.rec_off[a], &len) : nullptr;
  o.set_rec[spos[i]] = a;
  o.set_ts[spos[i]] = ts[i];
  o.set_crc[spos[i]] = m ? store_crc32c<WAYS>(T, ts[i], m, len) : 0;
}

// ---- the encoder.  Record j = a 12-byte header (be16 flags, be16 len, be32 crc32c seeded with the timestamp, be32 timestamp:
// gossip_store.c:64-68, COMPLETED set, DYING as the channel, DELETED when a later message of the batch took its slot) and message add_msg[j].
template <int WAYS>
LAMD_HD void store_rx_header(const u32 *T, const store_rx_batch &b, const u8 *flags, const u32 *ts, u32 i, u8 *hdr12) {
  const u32 len = (u32)(b.off[i + 1] - b.off[i]), crc = store_crc32c<WAYS>(T, ts[i], b.msgs + b.off[i], len);
  const u32 hf = STORE_FLAG_COMPLETED | (flags[i] & STORE_RX_DYING ? STORE_FLAG_DYING : 0) | (flags[i] & STORE_RX_SUPERSEDED ? STORE_FLAG_DELETED : 0);
  hdr12[0] = (u8)(hf >> 8);
  hdr12[1] = (u8)hf;
  hdr12[2] = (u8)(len >> 8);
  hdr12[3] = (u8)len;
  for (u32 k = 0; k < 4; k++) {
    hdr12[4 + k] = store_range_be(crc, 4, k);
    hdr12[8 + k] = store_range_be(ts[i], 4, k);
  }
}
struct store_rx_out { const u64 *add_off; const u32 *add_msg; u32 adds; const u8 *hdr; const u8 *msgs; const u64 *off; };
// Word k of the output, as store_sq_word: the bytes B0 = 4k - mis .. B0 + 3 with mis = out & 3; total = the adds' bytes
LAMD_HD void store_rx_word(const store_rx_out &o, u8 *out, u64 total, u32 mis, u64 k) {
  if (4 * k + 4 <= mis) return;
  const u64 B0 = 4 * k < mis ? 0 : 4 * k - mis;
  if (B0 >= total) return;
  u32 j = store_range_locate(o.add_off, o.adds, B0), w = 0;
  const bool whole = 4 * k >= mis && B0 + 4 <= total;
  for (u32 x = 0; x < 4; x++) {
    if (4 * k + x < mis) continue;
    const u64 B = 4 * k + x - mis;
    if (B >= total) break;
    while (j + 1 < o.adds && o.add_off[j + 1] <= B) j++;   // a record has 150 bytes at least: one step
    const u64 at = B - o.add_off[j];
    const u8 byte = at < STORE_HDR ? o.hdr[STORE_HDR * (size_t)j + at] : o.msgs[o.off[o.add_msg[j]] + at - STORE_HDR];
    if (whole) w |= (u32)byte << (8 * x); else out[B] = byte;
  }
  if (whole) *(u32 *)__builtin_assume_aligned(out + B0, 4) = w;
}

}  // namespace lamd

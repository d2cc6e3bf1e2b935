// Receiving channel_announcement batches against a store image, in the reference's two halves: the per-message, per-position and per-reply logic
// of lamd_channel_announcement_receive_batch and lamd_channel_announcement_confirm_batch (include/lightning_amd.h), as inline functions that
// compile for gfx950 and, unchanged, for the host (tests/c/store_announce_host.cpp runs them under the sanitizers).
//   - the classification of a raw message in the order of gossmap_manage_channel_announcement() (gossipd/gossmap_manage.c:620-753): framing
//     and the range of the eight signature scalars (fromwire_channel_announcement), node_id_1 < node_id_2, the chain, the caller's txout
//     failures, "already known" as four bisections (failures, held scids, the digest's entries, the bare channels).  What a filter drops goes
//     on the key-parse list (its two bitcoin keys alone decide between its filter's status and malformed), everything else on the signature list;
//   - what the two verdicts make of it, and the item of the scan: the arrival index of a message with four good signatures whose scid is
//     not "bad gossip order", all ones otherwise;
//   - "already pending from this batch" over the messages sorted by scid, arrival order kept inside a scid: the running minimum of the items
//     of a scid tells each position the earliest good copy at or in front of it -- no walk of a scid's messages;
//   - scriptpubkey_p2wsh(bitcoin_redeem_2of2()) (bitcoin/script.c:149-165), two compressions of sha256.h;
//   - the replies of gossmap_manage_handle_get_txout_reply() (:757-874): the pending announcement by bisection, the first reply of a scid by a
//     minimum per pending slot, the script comparison, "redundant", the two records of an accepted reply and node_announcements_not_dying()
//     (:603-618).  The records are encoded by store_receive.h's store_rx_header / store_rx_word.
// Every read of the image stays inside [store, store + store_len), every read of a batch inside its messages.
#pragma once
#include "store_receive.h"
#include "store_query.h"
#include "verify_core.h"
#include "sha256.h"

namespace lamd {

enum {
  STORE_CA_MALFORMED = -1, STORE_CA_PENDING = 0, STORE_CA_ID_ORDER = 1, STORE_CA_WRONG_CHAIN = 2, STORE_CA_TXOUT_FAILED = 3, STORE_CA_KNOWN = 4,
  STORE_CA_BAD_SIGNATURE = 4,   // + k, the first failing signature 1 .. 4
  STORE_CA_BAD_ORDER = 9, STORE_CA_IN_BATCH = 10, STORE_CA_EARLY = 11,
  STORE_CA_CANDIDATE = 100      // + k between the stages: a message of the signature list whose keys parse; k: its signature verdict 0 .. 4
};
enum { STORE_CA_LIST_NONE = 0, STORE_CA_LIST_SIGNATURES = 1, STORE_CA_LIST_KEYS = 2 };
constexpr u32 STORE_CA_MIN = 432, STORE_CA_MAX = 65535;   // every fixed field of a channel_announcement without features; the longest wire message
constexpr u32 STORE_CA_SCRIPT = 71, STORE_CA_SPK = 34, STORE_CA_AMOUNT = 10;

// the digest as the receive path reads it: the entries' scids and the bare channels', each ascending
struct store_ca_view { const u64 *scid; u32 count; const u64 *bare; u32 nbare; };
// the batch: message i = msgs[off[i], off[i + 1]); held: the caller's pending and too-early maps together, failed: its txout failures, both ascending
struct store_ca_batch { const u8 *msgs; const u64 *off; u32 n; const u64 *held; u32 n_held; const u64 *failed; u32 n_failed; u32 blockheight; u8 chain[32]; };
struct store_ca_msg { int32_t status; u32 list; u64 scid; u32 keyoff; };

// short_channel_id_blocknum(); "bad gossip order" and is_scid_depth_announceable() in the reference's unsigned 32-bit arithmetic
LAMD_HD u32 store_ca_blocknum(u64 scid) { return (u32)(scid >> 40); }
// (bad order is asked of a scid that is not announceable only: near 2^32 blockheight + 12 wraps, and the reference never gets there)
LAMD_HD bool store_ca_early(u64 scid, u32 blockheight) { return !((u32)(store_ca_blocknum(scid) + 5) <= blockheight); }
LAMD_HD bool store_ca_bad_order(u64 scid, u32 blockheight) {
  return store_ca_early(scid, blockheight) && blockheight != 0 && store_ca_blocknum(scid) > (u32)(blockheight + 12);
}

// ---- stage 1, every message: the framing half of -1 is final (no list); statuses 1 .. 4 are the filter's and go on the key-parse list; what
// passes every filter goes on the signature list with status PENDING
LAMD_HD store_ca_msg store_ca_classify(const store_ca_view &v, const store_ca_batch &b, u32 i) {
  store_ca_msg r;
  r.status = STORE_CA_MALFORMED;
  r.list = STORE_CA_LIST_NONE;
  r.scid = 0;
  r.keyoff = 0;
  const u64 len = b.off[i + 1] - b.off[i];
  const u8 *m = b.msgs + b.off[i];
  if (len < STORE_CA_MIN || len > STORE_CA_MAX || store_be16(m) != STORE_T_CANN) return r;
  const gossip_frame f = gossip_parse_frame(m, (size_t)len);
  if (f.bad) return r;
  for (u32 k = 0; k < 8; k++)
    if (store_rx_ge_n(m + 2 + 32 * k)) return r;
  // keyoff: node_id_1 33 | node_id_2 33 | bitcoin_key_1 33 | bitcoin_key_2 33 (inside the message: the frame is good); in front of it the scid, the chain
  r.keyoff = (u32)f.keyoff;
  r.scid = store_be64(m + f.keyoff - 8);
  r.list = STORE_CA_LIST_KEYS;
  if (store_dir_idcmp(m + f.keyoff, m + f.keyoff + 33) >= 0) { r.status = STORE_CA_ID_ORDER; return r; }
  u32 diff = 0;
  for (u32 k = 0; k < 32; k++) diff |= (u32)(m[f.keyoff - 40 + k] ^ b.chain[k]);
  if (diff) { r.status = STORE_CA_WRONG_CHAIN; return r; }
  if (b.n_failed && store_cmp_find(b.failed, b.n_failed, r.scid) != STORE_NONE) { r.status = STORE_CA_TXOUT_FAILED; return r; }
  if (store_cmp_find(v.scid, v.count, r.scid) != STORE_NONE || store_cmp_find(v.bare, v.nbare, r.scid) != STORE_NONE ||
      (b.n_held && store_cmp_find(b.held, b.n_held, r.scid) != STORE_NONE)) {
    r.status = STORE_CA_KNOWN;
    return r;
  }
  r.status = STORE_CA_PENDING;
  r.list = STORE_CA_LIST_SIGNATURES;
  return r;
}
// row `row` of the signature list: the message's span (four signature rows of the batch); of the key-parse list: its two bitcoin keys
LAMD_HD void store_ca_sig_row(const store_ca_batch &b, u32 i, u32 row, u64 *start, u64 *len) {
  start[row] = b.off[i];
  len[row] = b.off[i + 1] - b.off[i];
}
LAMD_HD void store_ca_key_row(const store_ca_batch &b, u32 i, u32 keyoff, u32 row, u8 *keys33) {
  const u8 *k = b.msgs + b.off[i] + keyoff + 66;
  for (u32 x = 0; x < 66; x++) keys33[66 * (size_t)row + x] = k[x];
}

// ---- stage 2, every message, behind the two batches.  sigv: the verdict of the signature batch per row of the signature list (-1: a bitcoin
// key does not parse, 0: four good signatures, k: the first failing one); keyok: the validity bytes of the key-parse list, two per row.
// Malformed becomes final (scid 0); a message of the signature list becomes CANDIDATE + k.  Returns the item of the scan.
LAMD_HD u32 store_ca_settle(int8_t *status, u64 *scid, const u8 *list, const u32 *row_of, const int8_t *sigv, const u8 *keyok, u32 blockheight, u32 i) {
  if (list[i] == STORE_CA_LIST_KEYS) {
    if (!(keyok[2 * (size_t)row_of[i]] && keyok[2 * (size_t)row_of[i] + 1])) { status[i] = STORE_CA_MALFORMED; scid[i] = 0; }
    return STORE_NONE;
  }
  if (list[i] != STORE_CA_LIST_SIGNATURES) return STORE_NONE;
  const int v = sigv[row_of[i]];
  if (v < 0 || v > 4) { status[i] = STORE_CA_MALFORMED; scid[i] = 0; return STORE_NONE; }
  status[i] = (int8_t)(STORE_CA_CANDIDATE + v);
  return v == 0 && !store_ca_bad_order(scid[i], blockheight) ? i : STORE_NONE;
}

// ---- stage 3, every sorted position.  val: the stable sort of ALL messages by scid (arrival order inside a scid); first: the inclusive minimum
// of the items inside each run of equal scids.  A candidate behind the earliest good copy of its scid is "already pending"; the earliest good
// copy itself is early or pending; with no good copy at or in front of it a candidate keeps its own verdict -- a bad signature, or four good
// ones under a scid that is bad gossip order.  acnt (all 0): 1 where the status is PENDING, for the scan of the ask list.
LAMD_HD void store_ca_resolve(const u32 *val, const u32 *first, const u64 *scid, u32 blockheight, u32 p, int8_t *status, u32 *acnt) {
  const u32 i = val[p];
  if (status[i] < STORE_CA_CANDIDATE) return;
  const int v = status[i] - STORE_CA_CANDIDATE;
  int s;
  if (first[p] < i) s = STORE_CA_IN_BATCH;
  else if (v) s = STORE_CA_BAD_SIGNATURE + v;
  else if (store_ca_bad_order(scid[i], blockheight)) s = STORE_CA_BAD_ORDER;
  else s = store_ca_early(scid[i], blockheight) ? STORE_CA_EARLY : STORE_CA_PENDING;
  status[i] = (int8_t)s;
  if (s == STORE_CA_PENDING) acnt[i] = 1;
}

// ---- stage 4, every message: the script of a pending or early message, its place in the ask list (apos: the exclusive scan of acnt).
// byte x of the 72 bytes that are hashed behind each other: OP_2, push 33, the lesser key, push 33, the greater key, OP_2, OP_CHECKMULTISIG, 0x80
LAMD_HD u8 store_ca_script_byte(const u8 *lo, const u8 *hi, u32 x) {
  if (x < 2) return x ? 0x21 : 0x52;
  if (x < 35) return lo[x - 2];
  if (x == 35) return 0x21;
  if (x < 69) return hi[x - 36];
  return x == 69 ? 0x52 : x == 70 ? 0xae : 0x80;
}
LAMD_HD void store_ca_spk(const u8 *key1, const u8 *key2, u8 *spk34) {
  const bool swap = store_dir_idcmp(key1, key2) > 0;   // pubkey_cmp: memcmp of the 33 serialised bytes
  const u8 *lo = swap ? key2 : key1, *hi = swap ? key1 : key2;
  u32 st[8] = LAMD_SHA256_IV, w[16];
#pragma unroll
  for (u32 j = 0; j < 16; j++)
    w[j] = ((u32)store_ca_script_byte(lo, hi, 4 * j) << 24) | ((u32)store_ca_script_byte(lo, hi, 4 * j + 1) << 16) |
           ((u32)store_ca_script_byte(lo, hi, 4 * j + 2) << 8) | store_ca_script_byte(lo, hi, 4 * j + 3);
  sha256_compress(st, w);
  w[0] = ((u32)store_ca_script_byte(lo, hi, 64) << 24) | ((u32)store_ca_script_byte(lo, hi, 65) << 16) | ((u32)store_ca_script_byte(lo, hi, 66) << 8) |
         store_ca_script_byte(lo, hi, 67);
  w[1] = ((u32)store_ca_script_byte(lo, hi, 68) << 24) | ((u32)store_ca_script_byte(lo, hi, 69) << 16) | ((u32)store_ca_script_byte(lo, hi, 70) << 8) |
         store_ca_script_byte(lo, hi, 71);
#pragma unroll
  for (u32 j = 2; j < 15; j++) w[j] = 0;
  w[15] = 8 * STORE_CA_SCRIPT;
  sha256_compress(st, w);
  spk34[0] = 0x00;
  spk34[1] = 0x20;
#pragma unroll
  for (u32 j = 0; j < 8; j++)
    for (u32 x = 0; x < 4; x++) spk34[2 + 4 * j + x] = (u8)(st[j] >> (24 - 8 * x));
}
LAMD_HD void store_ca_finish(const store_ca_batch &b, const int8_t *status, const u64 *scid, const u32 *keyoff, const u64 *apos, u64 ask_cap, u8 *spk34,
                             u32 *ask_msg, u64 *ask_scid, u32 i) {
  u8 *o = spk34 + STORE_CA_SPK * (size_t)i;
  if (status[i] != STORE_CA_PENDING && status[i] != STORE_CA_EARLY) {
    for (u32 x = 0; x < STORE_CA_SPK; x++) o[x] = 0;
    return;
  }
  const u8 *k = b.msgs + b.off[i] + keyoff[i] + 66;
  store_ca_spk(k, k + 33, o);
  if (status[i] == STORE_CA_PENDING && apos[i] < ask_cap) {
    ask_msg[apos[i]] = i;
    ask_scid[apos[i]] = scid[i];
  }
}

// ======== the second half: lightningd's replies
enum { STORE_CF_ACCEPTED = 0, STORE_CF_NOT_PENDING = 1, STORE_CF_NO_OUTPUT = 2, STORE_CF_WRONG_SCRIPT = 3, STORE_CF_REDUNDANT = 4 };
// the digest and the directory of the image as it is now
struct store_cf_view {
  const u64 *scid; u32 count; const u64 *bare; u32 nbare;
  const u8 *store; size_t store_len; const u64 *rec_off; u32 n_rec; const u64 *node_off; const u32 *node_nann; u32 nodes;   // node_nann: index + 1, 0: none
};
// the pending announcements (message p = pmsgs[poff[p], poff[p + 1]), at least STORE_CA_MIN bytes and well framed, pscid strictly ascending, their
// scripts) and the replies (script r = scripts[soff[r], soff[r + 1]))
struct store_cf_batch {
  const u8 *pmsgs; const u64 *poff, *pscid; const u8 *pspk; u32 np;
  const u64 *r_scid, *r_sat; const u8 *scripts; const u64 *soff; u32 nr;
};
// ---- stage 1, every reply: its pending announcement; the first reply of a pending slot (first: all ones) is the smallest index
LAMD_HD void store_cf_match(const store_cf_batch &b, u32 r, u32 *pend, u32 *first) {
  const u32 p = store_cmp_find(b.pscid, b.np, b.r_scid[r]);
  pend[r] = p;
  if (p != STORE_NONE) store_dir_min(&first[p], r);
}
// the record of node id33's announcement when its header carries DYING, STORE_NONE otherwise
LAMD_HD u32 store_cf_dying_nann(const store_cf_view &v, const u8 *id33) {
  const u32 rank = store_dir_find_node(v.store, v.node_off, v.nodes, id33);
  if (rank == STORE_NONE || v.node_nann[rank] == 0) return STORE_NONE;
  const u32 rec = v.node_nann[rank] - 1;
  if (!(rec < v.n_rec && v.rec_off[rec] <= v.store_len && v.store_len - v.rec_off[rec] >= STORE_HDR)) return STORE_NONE;
  return store_read_hdr(v.store + v.rec_off[rec]).flags & STORE_FLAG_DYING ? rec : STORE_NONE;
}
// ---- stage 2, every reply: the status; a reply behind the first of its scid finds nothing pending (pend: STORE_NONE).  What it leaves (all
// preset to 0 but clr_key: all ones): count and size of the accepted replies' record pairs, the count of the txout failures, and per node id
// of an accepted announcement the dying node_announcement record
struct store_cf_marks { u32 *acnt, *abytes, *fcnt, *clr_key; };
LAMD_HD int store_cf_classify(const store_cf_view &v, const store_cf_batch &b, u32 r, u32 *pend, const u32 *first, const store_cf_marks &k) {
  const u32 p = pend[r];
  if (p == STORE_NONE || first[p] != r) { pend[r] = STORE_NONE; return STORE_CF_NOT_PENDING; }
  const u64 slen = b.soff[r + 1] - b.soff[r];
  if (slen == 0) { k.fcnt[r] = 1; return STORE_CF_NO_OUTPUT; }
  u32 diff = slen != STORE_CA_SPK;
  for (u32 x = 0; !diff && x < STORE_CA_SPK; x++) diff |= (u32)(b.scripts[b.soff[r] + x] ^ b.pspk[STORE_CA_SPK * (size_t)p + x]);
  if (diff) { k.fcnt[r] = 1; return STORE_CF_WRONG_SCRIPT; }
  const u64 scid = b.r_scid[r];
  if (store_cmp_find(v.scid, v.count, scid) != STORE_NONE || store_cmp_find(v.bare, v.nbare, scid) != STORE_NONE) return STORE_CF_REDUNDANT;
  const u8 *m = b.pmsgs + b.poff[p];
  const u32 mlen = (u32)(b.poff[p + 1] - b.poff[p]), keyoff = 300 + store_be16(m + 258);
  k.acnt[r] = 1;
  k.abytes[r] = (u32)(2 * STORE_HDR + mlen + STORE_CA_AMOUNT);
  for (u32 x = 0; x < 2; x++) k.clr_key[2 * (size_t)r + x] = store_cf_dying_nann(v, m + keyoff + 33 * x);
  return STORE_CF_ACCEPTED;
}
// ---- stage 3, every sorted position of the clr keys: does it open a run of equal records (the pads, all ones, open none)?
LAMD_HD u32 store_cf_clr_head(const u32 *sorted, u32 p) { return sorted[p] != STORE_NONE && (p == 0 || sorted[p - 1] != sorted[p]); }
// ---- stage 4, every reply: the plan.  apos / abyte / fpos: the exclusive scans of the marks.  An accepted reply j = apos[r] makes the records
// 2j (its announcement: message pend[r] of the pending blob) and 2j + 1 (its amount: message np + j, ten bytes written here behind the blob),
// as store_rx_header / store_rx_word read them: rec_msg / rec_off per RECORD, off2 the offsets of np + accepted messages.
struct store_cf_plan_out {
  u64 add_cap, fail_cap; u32 *add_reply; u64 *add_off, *fail_scid;
  u32 *rec_msg; u64 *rec_off, *off2; u8 *amounts; u64 amounts_at;   // amounts = pmsgs + amounts_at: behind the pending messages
};
LAMD_HD void store_cf_plan(const store_cf_batch &b, const int8_t *status, const u32 *pend, const u64 *apos, const u64 *abyte, const u64 *fpos,
                           const store_cf_plan_out &o, u32 r) {
  if ((status[r] == STORE_CF_NO_OUTPUT || status[r] == STORE_CF_WRONG_SCRIPT) && fpos[r] < o.fail_cap) o.fail_scid[fpos[r]] = b.r_scid[r];
  if (status[r] != STORE_CF_ACCEPTED) return;
  const u64 j = apos[r];
  const u32 p = pend[r], mlen = (u32)(b.poff[p + 1] - b.poff[p]);
  if (j < o.add_cap) {
    o.add_reply[j] = r;
    o.add_off[j] = abyte[r];
  }
  o.rec_msg[2 * j] = p;
  o.rec_msg[2 * j + 1] = b.np + (u32)j;
  o.rec_off[2 * j] = abyte[r];
  o.rec_off[2 * j + 1] = abyte[r] + STORE_HDR + mlen;
  o.off2[b.np + j + 1] = o.amounts_at + STORE_CA_AMOUNT * (j + 1);   // (off2[0 .. np] are the pending offsets)
  u8 *a = o.amounts + STORE_CA_AMOUNT * j;
  a[0] = (u8)(STORE_T_AMOUNT >> 8);
  a[1] = (u8)STORE_T_AMOUNT;
  for (u32 x = 0; x < 8; x++) a[2 + x] = store_range_be(b.r_sat[r], 8, x);
}

}  // namespace lamd

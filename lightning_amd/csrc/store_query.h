// The directory of a store image and the answers to query_short_channel_ids from it: the per-record, per-occurrence and per-output-word logic
// of lamd_gossip_store_directory_build / lamd_short_channel_ids_reply_batch (include/lightning_amd.h), as inline functions that compile for
// gfx950 and, unchanged, for the host (tests/c/store_query_host.cpp runs them under the sanitizers).
//   - the record of a channel without an update (the digest keeps the records of its entries only): a bisection in the bare list and a
//     32-bit atomicMin, lowest index wins;
//   - the node ids an announcement names, the 8-byte chunks of an id for the LSD sort, the comparison of two ids as memcmp does it;
//   - the node_announcement of a node: a bisection in the ranked ids and a 32-bit atomicMax of index + 1, highest index wins;
//   - the parser of a query (fromwire_query_short_channel_ids, fromwire_tlv's rules, decode_scid_query_flags, decode_short_ids) and the
//     checks of handle_query_short_channel_ids() (connectd/queries.c:260-368) in the reference's order;
//   - one scid occurrence: gossmap_find_chan as two binary searches, the records its flag asks for and the ranks it remembers;
//   - the encoder, one aligned 32-bit word of the OUTPUT at a time, from byte loads: store records sit at any alignment.
// Every read of the image stays inside [store, store + store_len) whatever rec_off holds.
#pragma once
#include "store_compare.h"

namespace lamd {

// ---- the directory
LAMD_HD void store_dir_min(u32 *slot, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(slot, v);
#else
  if (v < *slot) *slot = v;
#endif
}
// every record: a counting channel_announcement whose scid is bare channel j goes to bare_rec[j] (all STORE_NONE), lowest index wins
LAMD_HD void store_dir_bare_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *bare, u32 nbare,
                                u32 *bare_rec) {
  u32 len, idoff;
  u64 scid;
  const u8 *m = store_digest_msg(store, store_len, rec_off, verdict, i, &len);
  if (!m || !store_cann_scid(m, len, &scid, &idoff)) return;
  const u32 j = store_cmp_find(bare, nbare, scid);
  if (j != STORE_NONE) store_dir_min(&bare_rec[j], i);
}
// the ids the announcement at record offset `off` names: with feature length f (the be16 at 258) node_id_1 sits at message offset 300 + f,
// node_id_2 at 333 + f; an announcement shorter than 366 + f names none.  *idoff: the image offset of node_id_1.
LAMD_HD bool store_dir_cann_ids(const u8 *store, size_t store_len, u64 off, u64 *idoff) {
  u32 len;
  const u8 *m = store_live_msg(store, store_len, off, &len);
  if (!m || len < 260 || store_be16(m) != STORE_T_CANN) return false;
  const u32 f = store_be16(m + 258);
  if (len < 366 + f) return false;
  *idoff = off + STORE_HDR + 300 + f;
  return true;
}
constexpr u64 STORE_DIR_NO_ID = ~(u64)0;   // a candidate that names no id (its announcement is cut off)
constexpr u32 STORE_DIR_PASSES = 6;        // the LSD sort: byte 32, bytes 24..31, 16..23, 8..15, 0..7, then "names no id" (1 bit)
// the key of pass p for the candidate whose id sits at image offset idoff
LAMD_HD u64 store_dir_pass_key(const u8 *store, u64 idoff, u32 p) {
  if (p == 5) return idoff == STORE_DIR_NO_ID;
  if (idoff == STORE_DIR_NO_ID) return 0;
  return p == 0 ? (u64)store[idoff + 32] : store_be64(store + idoff + 8 * (4 - p));
}
LAMD_HD int store_dir_idcmp(const u8 *a, const u8 *b) {   // memcmp over 33 bytes
  for (int i = 0; i < 33; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
// does candidate j of the sorted list (perm: sorted position -> candidate; the first `valid` name an id) open a run of equal ids?
LAMD_HD bool store_dir_head(const u8 *store, const u64 *cand_off, const u32 *perm, u32 valid, u32 j) {
  if (j >= valid) return false;
  return j == 0 || store_dir_idcmp(store + cand_off[perm[j]], store + cand_off[perm[j - 1]]) != 0;
}
// the rank of id33 among the nodes (node_off: image offsets of their ids, ascending by the ids), STORE_NONE: no such node
LAMD_HD u32 store_dir_find_node(const u8 *store, const u64 *node_off, u32 nodes, const u8 *id33) {
  u32 lo = 0, hi = nodes;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (store_dir_idcmp(store + node_off[mid], id33) < 0) lo = mid + 1; else hi = mid;
  }
  return lo < nodes && store_dir_idcmp(store + node_off[lo], id33) == 0 ? lo : STORE_NONE;
}
// every record: a counting node_announcement of >= 105 + f bytes (f: the be16 at 66, the id sits at 72 + f) behind the first announcement
// that names its node goes to node_nann[rank] (all 0) as index + 1, highest index wins.  Returns what became of the record:
enum { STORE_DIR_NANN_NONE = 0, STORE_DIR_NANN_PUT = 1, STORE_DIR_NANN_NO_NODE = 2, STORE_DIR_NANN_IN_FRONT = 3, STORE_DIR_NANN_SHORT = 4 };
LAMD_HD u32 store_dir_nann_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *node_off,
                               const u32 *node_first, u32 nodes, u32 *node_nann) {
  u32 len;
  const u8 *m = store_digest_msg(store, store_len, rec_off, verdict, i, &len);
  if (!m || len < 2 || store_be16(m) != STORE_T_NANN) return STORE_DIR_NANN_NONE;
  if (len < 68) return STORE_DIR_NANN_SHORT;
  const u32 f = store_be16(m + 66);
  if (len < 105 + f) return STORE_DIR_NANN_SHORT;
  const u32 r = store_dir_find_node(store, node_off, nodes, m + 72 + f);
  if (r == STORE_NONE) return STORE_DIR_NANN_NO_NODE;
  if (i <= node_first[r]) return STORE_DIR_NANN_IN_FRONT;
  store_digest_slot_put(&node_nann[r], i + 1);
  return STORE_DIR_NANN_PUT;
}

// ---- query_short_channel_ids.  be16 261 | chain_hash 32 | be16 len | encoded_short_ids len | tlv stream; TLV 1 = encoding_type (a byte),
// encoded_query_flags (a run of bigsizes).
enum { STORE_SQ_ANSWERED = 0, STORE_SQ_FOREIGN = 1, STORE_SQ_BAD_FLAGS = 2, STORE_SQ_BAD_SCIDS = 3, STORE_SQ_FLAG_COUNT = 4, STORE_SQ_MALFORMED = -1 };
constexpr u32 STORE_SQ_HEAD = 36;        // the query in front of encoded_short_ids
constexpr u32 STORE_SQ_END_BYTES = 35;   // reply_short_channel_ids_end: be16 262 | chain_hash 32 | full_information 1
constexpr u32 STORE_SQ_ALL = 0x1f;       // the flag of every scid of a query without TLV 1
struct store_sq_query {
  int32_t status;       // STORE_SQ_*
  u32 n;                // scids; 0 unless answered
  u64 scid_at;          // offset of the first be64 scid in the batch's bytes
  u32 flags_at, flags_len;   // the run of bigsizes inside the query (flags_at 0: no TLV 1)
};
// base: the offset of q in the batch
LAMD_HD store_sq_query store_sq_parse(const u8 *q, size_t len, u64 base, const u8 *our_chain32) {
  store_sq_query r;
  r.status = STORE_SQ_MALFORMED;
  r.n = 0;
  r.scid_at = 0;
  r.flags_at = r.flags_len = 0;
  if (len < STORE_SQ_HEAD || store_be16(q) != 261) return r;
  const u32 l = store_be16(q + 34);
  if (l > len - STORE_SQ_HEAD) return r;
  size_t pos = STORE_SQ_HEAD + l, f_pos = 0;
  u64 prev = 0, f_len = 0;
  bool first = true, have_flags = false;
  while (pos < len) {
    u64 type, tl;
    if (!store_bigsize(q, len, &pos, &type)) return r;
    if (!first && type <= prev) return r;
    first = false;
    prev = type;
    if (type != 1 && !(type & 1)) return r;
    if (!store_bigsize(q, len, &pos, &tl) || tl > len - pos) return r;
    if (type == 1) {
      if (tl == 0) return r;   // no encoding_type byte to read
      have_flags = true;
      f_pos = pos;
      f_len = tl;
    }
    pos += (size_t)tl;
  }
  u32 n_flags = 0;
  if (have_flags) {
    r.status = STORE_SQ_BAD_FLAGS;
    if (q[f_pos] != 0) return r;
    const size_t end = f_pos + (size_t)f_len;
    for (size_t p = f_pos + 1; p < end; n_flags++) {
      u64 v;
      if (!store_bigsize(q, end, &p, &v)) return r;
    }
  }
  u32 same = 0;
  for (int b = 0; b < 32; b++) same |= (u32)(q[2 + b] ^ our_chain32[b]);
  if (same) { r.status = STORE_SQ_FOREIGN; return r; }
  if (l == 0 || q[STORE_SQ_HEAD] != 0 || (l - 1) % 8 != 0) { r.status = STORE_SQ_BAD_SCIDS; return r; }
  if (have_flags && n_flags != (l - 1) / 8) { r.status = STORE_SQ_FLAG_COUNT; return r; }
  r.status = STORE_SQ_ANSWERED;
  r.n = (l - 1) / 8;
  r.scid_at = base + STORE_SQ_HEAD + 1;
  if (have_flags) {
    r.flags_at = (u32)f_pos + 1;
    r.flags_len = (u32)f_len - 1;
  }
  return r;
}
// the flags of an answered query, one byte per scid: bits 0..4 of each bigsize, STORE_SQ_ALL without TLV 1
LAMD_HD void store_sq_flags(const u8 *q, const store_sq_query &p, u8 *out) {
  size_t pos = p.flags_at;
  const size_t end = (size_t)p.flags_at + p.flags_len;
  for (u32 k = 0; k < p.n; k++) {
    u64 v = STORE_SQ_ALL;
    if (p.flags_at) (void)store_bigsize(q, end, &pos, &v);
    out[k] = (u8)(v & STORE_SQ_ALL);
  }
}

// ---- one scid occurrence.  The directory as the responder reads it: the channels are the digest's entries (ent_rec: announcement, update
// 0, update 1; STORE_NONE where there is none) and behind them the bare ones; chan_rank: the ranks of a channel's two nodes.
struct store_sq_dir {
  const u8 *store; size_t store_len; const u64 *rec_off; u32 n;
  const u64 *scid; const u32 *ent_rec; u32 count;
  const u64 *bare; const u32 *bare_rec; u32 nbare;
  const u32 *chan_rank; const u32 *node_nann; u32 nodes;
};
// the length of record r's message if r is a live record inside the image, else 0 (such a record is never sent)
LAMD_HD u32 store_sq_msg_len(const store_sq_dir &d, u32 r) {
  if (r >= d.n) return 0;
  u32 len;
  return store_live_msg(d.store, d.store_len, d.rec_off[r], &len) ? len : 0;
}
// rec3: the records to send (announcement, update 0, update 1), STORE_NONE where the flag does not ask or there is none; *bytes: their
// sizes' sum; rank2: the ranks remembered for bits 3 and 4, STORE_NONE where none.  Returns whether the scid is a channel.
LAMD_HD bool store_sq_lookup(const store_sq_dir &d, u64 scid, u32 flag, u32 *rec3, u32 *bytes, u32 *rank2) {
  rec3[0] = rec3[1] = rec3[2] = rank2[0] = rank2[1] = STORE_NONE;
  *bytes = 0;
  u32 have[3] = {STORE_NONE, STORE_NONE, STORE_NONE}, c = store_cmp_find(d.scid, d.count, scid);
  if (c != STORE_NONE) {
    for (u32 k = 0; k < 3; k++) have[k] = d.ent_rec[3 * (size_t)c + k];
  } else {
    const u32 j = store_cmp_find(d.bare, d.nbare, scid);
    if (j == STORE_NONE) return false;
    c = d.count + j;
    have[0] = d.bare_rec[j];
  }
  for (u32 k = 0; k < 3; k++) {
    const u32 len = (flag >> k) & 1 ? store_sq_msg_len(d, have[k]) : 0;
    if (len) {
      rec3[k] = have[k];
      *bytes += len;
    }
  }
  for (u32 k = 0; k < 2; k++)
    if ((flag >> (3 + k)) & 1) rank2[k] = d.chan_rank[2 * (size_t)c + k];
  return true;
}
// the first element of key[0, n) (ascending) that is >= v
LAMD_HD u32 store_sq_lower(const u64 *key, u32 n, u64 v) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (key[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- the encoder.  Message j is a copy of record msg_rec[j]'s message, or with STORE_NONE the end message of its query (found by
// bisection in reply_first): be16 262, the QUERY's chain_hash (ours when it was answered), full_information = answered.
struct store_sq_out {
  const u64 *msg_off; const u32 *msg_rec; u32 n_msgs;
  const u64 *reply_first; u32 nq;
  const u8 *queries; const u64 *qoff; const int8_t *status;
};
LAMD_HD u8 store_sq_msg_byte(const store_sq_dir &d, const store_sq_out &o, u32 j, u32 x) {
  const u32 r = o.msg_rec[j];
  if (r != STORE_NONE) return d.store[d.rec_off[r] + STORE_HDR + x];
  if (x < 2) return store_range_be(262, 2, x);
  const u32 q = store_range_locate(o.reply_first, o.nq, j);
  if (x < 34) return o.queries[o.qoff[q] + x];
  return o.status[q] == STORE_SQ_ANSWERED;
}
// Word k of the output, as store_range_word: the bytes B0 = 4k - mis .. B0 + 3 with mis = out & 3; total = msg_off[n_msgs]
LAMD_HD void store_sq_word(const store_sq_dir &d, const store_sq_out &o, u8 *out, u64 total, u32 mis, u64 k) {
  if (4 * k + 4 <= mis) return;
  const u64 B0 = 4 * k < mis ? 0 : 4 * k - mis;
  if (B0 >= total) return;
  u32 j = store_range_locate(o.msg_off, o.n_msgs, B0), w = 0;
  const bool whole = 4 * k >= mis && B0 + 4 <= total;
  for (u32 b = 0; b < 4; b++) {
    if (4 * k + b < mis) continue;
    const u64 B = 4 * k + b - mis;
    if (B >= total) break;
    while (j + 1 < o.n_msgs && o.msg_off[j + 1] <= B) j++;
    const u8 v = store_sq_msg_byte(d, o, j, (u32)(B - o.msg_off[j]));
    if (whole) w |= (u32)v << (8 * b); else out[B] = v;
  }
  if (whole) *(u32 *)__builtin_assume_aligned(out + B0, 4) = w;
}

}  // namespace lamd

// gossip_store digest and query_channel_range answers: the per-record, per-entry, per-query and per-output-word logic of
// lamd_gossip_store_digest_build / lamd_channel_range_reply_batch (include/lightning_amd.h), as inline functions that compile for gfx950
// and, unchanged, for the host (tests/c/store_digest_host.cpp runs them under the sanitizers).
//   - which records count (DELETED flag clear, verdict OK where verdicts are given) and the scid index over the counting announcements;
//   - one slot per (channel, direction): record index + 1 of the LAST counting channel_update behind the announcement, written with a
//     32-bit atomicMax, so that the highest index wins whatever the order in which the lanes arrive (update_channel(), common/gossmap.c);
//   - the entry of a channel: both timestamps, both checksums (crc32_of_update, connectd/queries.c:429-470), the three record indices;
//   - the query parser (fromwire_query_channel_range and fromwire_tlv's rules), max_entries() (:519-561);
//   - the plan of a query: two binary searches in the sorted digest, then queue_channel_ranges() (:641-711) with an explicit bound;
//   - the encoder of reply_channel_range, one aligned 32-bit word of the OUTPUT at a time.
// Every read of the image stays inside [store, store + store_len): the image on the device need not be the file the host walked.
#pragma once
#include "store_latest.h"

namespace lamd {

// ---- what counts.  verdict may be nullptr: flags alone decide.
LAMD_HD const u8 *store_digest_msg(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, u32 *len) {
  if (verdict && verdict[i] != LAMD_STORE_OK) return nullptr;
  return store_live_msg(store, store_len, rec_off[i], len);
}
// stage 1, every record: a counting channel_announcement that holds its scid goes into the scid index (store_audit.h: lowest index wins)
LAMD_HD void store_digest_index_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, u64 *keys, u32 *vals,
                                    u32 bits) {
  u32 len, idoff;
  u64 scid;
  const u8 *m = store_digest_msg(store, store_len, rec_off, verdict, i, &len);
  if (m && store_cann_scid(m, len, &scid, &idoff)) store_index_insert(keys, vals, bits, scid, i);
}
// stage 2, every record.  slot: 2 * n words, all 0; slot[2 * a + d] ends as 1 + the HIGHEST index of a counting channel_update of >= 112
// bytes behind its indexed announcement a with channel_flags & 1 == d.  Returns what became of the record:
enum { STORE_DIGEST_UPD_NONE = 0, STORE_DIGEST_UPD_PUT = 1, STORE_DIGEST_UPD_NO_CHANNEL = 2, STORE_DIGEST_UPD_IN_FRONT = 3, STORE_DIGEST_UPD_SHORT = 4 };
LAMD_HD void store_digest_slot_put(u32 *slot, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(slot, v);
#else
  if (v > *slot) *slot = v;
#endif
}
LAMD_HD u32 store_digest_slot_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *keys,
                                  const u32 *vals, u32 bits, u32 *slot) {
  u32 len;
  const u8 *m = store_digest_msg(store, store_len, rec_off, verdict, i, &len);
  if (!m || len < 2 || store_be16(m) != STORE_T_CUPD) return STORE_DIGEST_UPD_NONE;
  if (len < 112) return STORE_DIGEST_UPD_SHORT;   // deliberate: gossmap would read the scid and the flags past its end
  const u32 a = store_index_find(keys, vals, bits, store_be64(m + 98));
  if (a == STORE_NONE) return STORE_DIGEST_UPD_NO_CHANNEL;
  if (a >= i) return STORE_DIGEST_UPD_IN_FRONT;
  store_digest_slot_put(&slot[2 * (size_t)a + (m[111] & 1)], i + 1);
  return STORE_DIGEST_UPD_PUT;
}
// stage 3, every record: is record i a channel (the indexed announcement of its scid)?  0 no, 1 with an update (an entry), 2 without
LAMD_HD u32 store_digest_chan_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *keys,
                                  const u32 *vals, u32 bits, const u32 *slot, u64 *scid) {
  u32 len, idoff;
  const u8 *m = store_digest_msg(store, store_len, rec_off, verdict, i, &len);
  if (!m || !store_cann_scid(m, len, scid, &idoff) || store_index_find(keys, vals, bits, *scid) != i) return 0;
  return (slot[2 * (size_t)i] | slot[2 * (size_t)i + 1]) ? 1 : 2;
}
// crc32_of_update: the update without its signature and its timestamp -- bytes [66, 106) and [110, len).  store_crc32c takes any pointer
// (bytes until it is 4-aligned, then aligned 32-bit loads), so the two parts may start anywhere in an image that starts anywhere.
template <int WAYS> LAMD_HD u32 store_digest_csum(const u32 *T, const u8 *m, u32 len) {
  return store_crc32c<WAYS>(T, store_crc32c<WAYS>(T, 0, m + 66, 40), m + 110, len - 110);
}
// stage 5, every entry: announcement a's timestamps, checksums and record indices.  ts2 / csum2: 2 words, rec3: 3 words.
template <int WAYS> LAMD_HD void store_digest_entry_one(const u32 *T, const u8 *store, size_t store_len, const u64 *rec_off, u32 a, const u32 *slot,
                                                        u32 *ts2, u32 *csum2, u32 *rec3) {
  rec3[0] = a;
  for (u32 d = 0; d < 2; d++) {
    const u32 s = slot[2 * (size_t)a + d];
    u32 len = 0;
    const u8 *m = s ? store_live_msg(store, store_len, rec_off[s - 1], &len) : nullptr;
    if (m && len >= 112) {
      ts2[d] = store_be32(m + 106);
      csum2[d] = store_digest_csum<WAYS>(T, m, len);
      rec3[1 + d] = s - 1;
    } else {
      ts2[d] = 0;
      csum2[d] = 0;
      rec3[1 + d] = STORE_NONE;
    }
  }
}

// ---- query_channel_range.  be16 263 | chain_hash 32 | be32 first_blocknum | be32 number_of_blocks | tlv stream; TLV 1 = query_option.
enum { STORE_RANGE_ANSWERED = 0, STORE_RANGE_FOREIGN = 1, STORE_RANGE_MALFORMED = -1 };
enum { STORE_RANGE_TIMESTAMPS = 1, STORE_RANGE_CHECKSUMS = 2 };
constexpr u32 STORE_RANGE_QUERY_MIN = 42;   // the query without TLVs
constexpr u32 STORE_RANGE_HEAD = 45;        // reply: type 2 | chain_hash 32 | first 4 | blocks 4 | sync_complete 1 | len 2
struct store_range_query {
  int32_t kind;                // STORE_RANGE_*
  u32 first, number;           // as received (FOREIGN echoes them); store_range_fix() gives what is answered
  u32 opts, limit;             // query_option & 3; entries per reply
  u8 chain[32];                // the query's own chain_hash
};
struct store_range_msg { u32 first, blocks, off, n, final, opts, query; };   // off: index of the first entry in the digest
struct store_range_total { u32 msgs; u64 bytes; };

// BigSize (BOLT #1), minimal encodings only.  false: cut off or not minimal.
LAMD_HD bool store_bigsize(const u8 *p, size_t len, size_t *pos, u64 *v) {
  if (*pos >= len) return false;
  const u8 b = p[(*pos)++];
  if (b < 0xfd) { *v = b; return true; }
  const u32 w = b == 0xfd ? 2 : b == 0xfe ? 4 : 8;
  if (len - *pos < w) return false;
  u64 x = 0;
  for (u32 k = 0; k < w; k++) x = (x << 8) | p[(*pos)++];
  *v = x;
  return x >= (w == 2 ? (u64)0xfd : w == 4 ? (u64)0x10000 : (u64)0x100000000ull);
}
LAMD_HD u32 store_bigsize_len(u64 v) { return v < 0xfd ? 1 : v <= 0xffff ? 3 : v <= 0xffffffffull ? 5 : 9; }
// max_entries(): how many entries one reply holds.  cap = dev_max_encoding_bytes, 0: none.
LAMD_HD u32 store_range_limit(u32 opts, u32 cap) {
  u32 bytes = 65535 - 2 - 43, per_entry = 8;
  const u32 overhead = 1 + store_bigsize_len((u64)(bytes / per_entry) * 8);
  if (opts & STORE_RANGE_TIMESTAMPS) { bytes -= overhead; per_entry += 8; }
  if (opts & STORE_RANGE_CHECKSUMS) { bytes -= overhead; per_entry += 8; }
  if (cap && bytes > cap) bytes = cap;
  if (bytes < per_entry) bytes = per_entry;
  return bytes / per_entry;
}
// The parse, by fromwire_tlv's rules: types strictly ascending, type and length minimal, an unknown even type fails, an unknown odd one
// is skipped, the known one must use its length exactly.  our_chain32: the chain this node serves.
LAMD_HD store_range_query store_range_parse(const u8 *q, size_t len, const u8 *our_chain32, u32 max_encoded_bytes) {
  store_range_query r;
  r.kind = STORE_RANGE_MALFORMED;
  r.first = r.number = r.opts = r.limit = 0;
  for (int b = 0; b < 32; b++) r.chain[b] = 0;
  if (len < STORE_RANGE_QUERY_MIN || store_be16(q) != 263) return r;
  u64 option = 0, prev = 0;
  bool first = true;
  size_t pos = STORE_RANGE_QUERY_MIN;
  while (pos < len) {
    u64 type, l;
    if (!store_bigsize(q, len, &pos, &type)) return r;
    if (!first && type <= prev) return r;
    first = false;
    prev = type;
    if (type != 1 && !(type & 1)) return r;
    if (!store_bigsize(q, len, &pos, &l) || l > len - pos) return r;
    if (type == 1) {
      size_t vpos = pos;
      if (!store_bigsize(q, pos + (size_t)l, &vpos, &option) || vpos != pos + (size_t)l) return r;
    }
    pos += (size_t)l;
  }
  u32 same = 0;
  for (int b = 0; b < 32; b++) { r.chain[b] = q[2 + b]; same |= (u32)(q[2 + b] ^ our_chain32[b]); }
  r.first = store_be32(q + 34);
  r.number = store_be32(q + 38);
  r.opts = (u32)option & 3;
  r.limit = store_range_limit(r.opts, max_encoded_bytes);
  r.kind = same ? STORE_RANGE_FOREIGN : STORE_RANGE_ANSWERED;
  return r;
}
// first_blocknum + number_of_blocks overflows: number = UINT32_MAX - first (:746-748)
LAMD_HD u32 store_range_fix(u32 first, u32 number) { return (u32)(first + number) < first ? 0xFFFFFFFFu - first : number; }

LAMD_HD u32 store_range_block(u64 scid) { return (u32)(scid >> 40); }
// the first entry of scid[0, count) (ascending) whose block is >= block (strict: > block): count if there is none
LAMD_HD u32 store_range_bound(const u64 *scid, u32 count, u32 block, bool strict) {
  u32 lo = 0, hi = count;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2, b = store_range_block(scid[mid]);
    if (strict ? b <= block : b < block) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the size of a reply with n entries
LAMD_HD u32 store_range_msg_bytes(const store_range_query &q, u32 n) {
  if (q.kind == STORE_RANGE_FOREIGN) return STORE_RANGE_HEAD;
  u32 b = STORE_RANGE_HEAD + 1 + 8 * n;
  if (q.opts & STORE_RANGE_TIMESTAMPS) b += 1 + store_bigsize_len(1 + 8 * (u64)n) + 1 + 8 * n;
  if (q.opts & STORE_RANGE_CHECKSUMS) b += 1 + store_bigsize_len(8 * (u64)n) + 8 * n;
  return b;
}
// The plan of one query over the digest's sorted scids: queue_channel_ranges().  Message k of the query goes to out[k] while k < out_cap
// (out may be nullptr with out_cap 0: count only); `query` is stored in each message.  The loop runs count + 1 times at the most: every
// reply but the last takes at least one entry.  Returns the number of messages and the sum of their sizes.
LAMD_HD store_range_total store_range_plan(const store_range_query &q, u32 query, const u64 *scid, u32 digest_count, store_range_msg *out, u32 out_cap) {
  store_range_total t{0, 0};
  if (q.kind == STORE_RANGE_MALFORMED) return t;
  if (q.kind == STORE_RANGE_FOREIGN) {
    if (out_cap) out[0] = store_range_msg{q.first, q.number, 0, 0, 0, 0, query};
    t.msgs = 1;
    t.bytes = STORE_RANGE_HEAD;
    return t;
  }
  u32 first = q.first, number = store_range_fix(q.first, q.number), lo = 0, count = 0;
  if (number) {
    lo = store_range_bound(scid, digest_count, first, false);
    count = store_range_bound(scid, digest_count, first + number - 1, true) - lo;
  }
  const u64 *s = scid + lo;
  const u32 limit = q.limit ? q.limit : 1;
  u32 off = 0;
  for (u32 it = 0; it <= count; it++) {
    const u32 rem = count - off;
    u32 n, blocks;
    if (rem <= limit) {
      n = rem;
      blocks = number;
    } else {
      // "while n > 0 and block(s[off + n - 1]) == block(s[off + limit]): n--" from n = limit: the scids ascend, so the entries of that
      // block are the tail of [off, off + limit) and n ends at the first of them -- found by bisection, not by a walk of `limit` loads
      n = store_range_bound(s + off, limit, store_range_block(s[off + limit]), false);
      if (n == 0) n = limit;   // one block holds more than a reply: the boundary is broken (the reference reads s[off - 1] here)
      blocks = store_range_block(s[off + n]) - first;
    }
    if (t.msgs < out_cap) out[t.msgs] = store_range_msg{first, blocks, lo + off, n, blocks == number, q.opts, query};
    t.msgs++;
    t.bytes += store_range_msg_bytes(q, n);
    first += blocks;
    number -= blocks;
    off += n;
    if (number == 0) break;
  }
  return t;
}

// ---- the encoder.  The digest as the encoder reads it:
struct store_digest_view { const u64 *scid; const u32 *ts, *csum; };   // ts / csum: 2 words per entry
LAMD_HD u8 store_range_be(u64 v, u32 width, u32 k) { return (u8)(v >> (8 * (width - 1 - k))); }   // byte k of v written big-endian in `width` bytes
// a bigsize of 1 or 3 bytes (the lengths here stay below 65536)
LAMD_HD u8 store_range_bigsize_byte(u32 v, u32 k) { return v < 0xfd ? (u8)v : k == 0 ? (u8)0xfd : store_range_be(v, 2, k - 1); }
// byte x of message m (x < its size)
LAMD_HD u8 store_range_msg_byte(const store_range_msg &m, const store_range_query &q, const store_digest_view &d, u32 x) {
  if (x < 2) return store_range_be(264, 2, x);
  if (x < 34) return q.chain[x - 2];
  if (x < 38) return store_range_be(m.first, 4, x - 34);
  if (x < 42) return store_range_be(m.blocks, 4, x - 38);
  if (x < 43) return (u8)m.final;
  if (q.kind == STORE_RANGE_FOREIGN) return 0;   // len 0, nothing behind it
  if (x < 45) return store_range_be(1 + 8 * m.n, 2, x - 43);
  if (x < 46) return 0;   // encoding: uncompressed
  x -= 46;
  if (x < 8 * m.n) return store_range_be(d.scid[m.off + x / 8], 8, x & 7);
  x -= 8 * m.n;
  if (m.opts & STORE_RANGE_TIMESTAMPS) {
    const u32 l = 1 + 8 * m.n, ll = store_bigsize_len(l);
    if (x < 1) return 1;
    if (x < 1 + ll) return store_range_bigsize_byte(l, x - 1);
    if (x < 2 + ll) return 0;   // encoding: uncompressed
    x -= 2 + ll;
    if (x < 8 * m.n) return store_range_be(d.ts[2 * (size_t)(m.off + x / 8) + ((x >> 2) & 1)], 4, x & 3);
    x -= 8 * m.n;
  }
  const u32 l = 8 * m.n, ll = store_bigsize_len(l);
  if (x < 1) return 3;
  if (x < 1 + ll) return store_range_bigsize_byte(l, x - 1);
  x -= 1 + ll;
  return store_range_be(d.csum[2 * (size_t)(m.off + x / 8) + ((x >> 2) & 1)], 4, x & 3);
}
// the message that holds output byte B (B < msg_off[n_msgs]): the last j with msg_off[j] <= B
LAMD_HD u32 store_range_locate(const u64 *msg_off, u32 n_msgs, u64 B) {
  u32 lo = 0, hi = n_msgs - 1;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo + 1) / 2;
    if (msg_off[mid] <= B) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// Word k of the output: the bytes B0 = 4k - mis .. B0 + 3 with mis = out & 3, so that out + B0 is 4-aligned; total = msg_off[n_msgs].  A word
// that lies inside [0, total) is ONE aligned store, put together in registers; the words at the two ends go byte by byte.
LAMD_HD void store_range_word(const store_range_msg *msgs, const u64 *msg_off, u32 n_msgs, const store_range_query *queries, const store_digest_view &d,
                              u8 *out, u64 total, u32 mis, u64 k) {
  if (4 * k + 4 <= mis) return;
  const u64 B0 = 4 * k < mis ? 0 : 4 * k - mis;
  if (B0 >= total) return;
  u32 j = store_range_locate(msg_off, n_msgs, B0), w = 0;
  const bool whole = 4 * k >= mis && B0 + 4 <= total;
  for (u32 b = 0; b < 4; b++) {
    if (4 * k + b < mis) continue;
    const u64 B = 4 * k + b - mis;
    if (B >= total) break;
    while (j + 1 < n_msgs && msg_off[j + 1] <= B) j++;   // a reply has 45 bytes at least: one step
    const u8 v = store_range_msg_byte(msgs[j], queries[msgs[j].query], d, (u32)(B - msg_off[j]));
    if (whole) w |= (u32)v << (8 * b); else out[B] = v;
  }
  if (whole) *(u32 *)__builtin_assume_aligned(out + B0, 4) = w;
}

}  // namespace lamd

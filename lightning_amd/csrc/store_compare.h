// The seeker's comparison of peers' reply_channel_range messages with the digest: the per-message, per-entry and per-output-word logic of
// lamd_channel_range_compare_batch (include/lightning_amd.h), as inline functions that compile for gfx950 and, unchanged, for the host
// (tests/c/store_compare_host.cpp runs them under the sanitizers).
//   - the parser of a reply (fromwire_reply_channel_range and fromwire_tlv's rules) and the checks of handle_reply_channel_range() and
//     append_range_reply() (gossipd/queries.c:142-265) in the reference's order: the first that fails is the message's status;
//   - the class of one entry: gossmap_find_chan as two binary searches (the digest's entries, then its channels without an update),
//     want_update() / check_timestamps() (gossipd/seeker.c:636-689) as two comparisons;
//   - the head of a run in a sorted list, for the merge;
//   - the layout of the query_short_channel_ids messages (gossipd/queries.c:46-139) in closed form, and their encoder, one aligned 32-bit
//     word of the OUTPUT at a time.
// The parser reads [m, m + len) only; an entry is read where the parser of the same bytes has found it.
#pragma once
#include "store_digest.h"

namespace lamd {

// ---- reply_channel_range.  be16 264 | chain_hash 32 | be32 first_blocknum | be32 number_of_blocks | u8 sync_complete | be16 len |
// encoded_short_ids len | tlv stream; TLV 1 = timestamps_tlv (encoding_type, encoded_timestamps), TLV 3 = checksums_tlv.
enum { STORE_CMP_ACCEPTED = 0, STORE_CMP_FOREIGN = 1, STORE_CMP_OVERFLOW = 2, STORE_CMP_BAD_SCIDS = 3, STORE_CMP_NO_OVERLAP = 4, STORE_CMP_BAD_TIMESTAMPS = 5,
       STORE_CMP_TIMESTAMP_COUNT = 6, STORE_CMP_MALFORMED = -1 };
constexpr u64 STORE_CMP_NO_TS = ~(u64)0;
struct store_cmp_msg {
  int32_t status;   // STORE_CMP_*
  u32 n;            // entries; 0 unless accepted
  u64 scid_at;      // offset of the first be64 scid in the batch's bytes
  u64 ts_at;        // ... of the first pair of be32 timestamps; STORE_CMP_NO_TS: the reply has no TLV 1, every pair is (0, 0)
};
// base: the offset of m in the batch (scid_at and ts_at count from the batch's first byte).  want: the peer's outstanding query,
// range_first_blocknum and the exclusive range_end_blocknum; without it the overlap check is the caller's.
LAMD_HD store_cmp_msg store_cmp_parse(const u8 *m, size_t len, u64 base, const u8 *our_chain32, bool have_want, u32 want_first, u32 want_end) {
  store_cmp_msg r;
  r.status = STORE_CMP_MALFORMED;
  r.n = 0;
  r.scid_at = 0;
  r.ts_at = STORE_CMP_NO_TS;
  if (len < STORE_RANGE_HEAD || store_be16(m) != 264) return r;
  const u32 l = store_be16(m + 43);
  if (l > len - STORE_RANGE_HEAD) return r;
  size_t pos = STORE_RANGE_HEAD + l, ts_pos = 0;
  u64 prev = 0, ts_len = 0;
  bool first = true, have_ts = false;
  while (pos < len) {
    u64 type, tl;
    if (!store_bigsize(m, len, &pos, &type)) return r;
    if (!first && type <= prev) return r;
    first = false;
    prev = type;
    if (type != 1 && type != 3 && !(type & 1)) return r;
    if (!store_bigsize(m, len, &pos, &tl) || tl > len - pos) return r;
    if (type == 1) {
      if (tl == 0) return r;   // no encoding_type byte to read
      have_ts = true;
      ts_pos = pos;
      ts_len = tl;
    }
    if (type == 3 && (tl & 7)) return r;   // an array of 8-byte channel_update_checksums
    pos += (size_t)tl;
  }
  u32 same = 0;
  for (int b = 0; b < 32; b++) same |= (u32)(m[2 + b] ^ our_chain32[b]);
  const u32 first_block = store_be32(m + 34), number = store_be32(m + 38);
  if (same) { r.status = STORE_CMP_FOREIGN; return r; }
  if ((u32)(first_block + number) < first_block) { r.status = STORE_CMP_OVERFLOW; return r; }
  if (l == 0 || m[STORE_RANGE_HEAD] != 0 || (l - 1) % 8 != 0) { r.status = STORE_CMP_BAD_SCIDS; return r; }
  if (have_want && (first_block + number <= want_first || first_block >= want_end)) { r.status = STORE_CMP_NO_OVERLAP; return r; }
  if (have_ts) {
    if (m[ts_pos] != 0 || (ts_len - 1) % 8 != 0) { r.status = STORE_CMP_BAD_TIMESTAMPS; return r; }
    if ((ts_len - 1) / 8 != (l - 1) / 8) { r.status = STORE_CMP_TIMESTAMP_COUNT; return r; }
    r.ts_at = base + ts_pos + 1;
  }
  r.status = STORE_CMP_ACCEPTED;
  r.n = (l - 1) / 8;
  r.scid_at = base + STORE_RANGE_HEAD + 1;
  return r;
}

// ---- the class of an entry.  The digest as the comparison reads it: the entries (ts: 2 words each) and the channels without an update,
// both ascending by scid.
struct store_cmp_digest { const u64 *scid; const u32 *ts; u32 count; const u64 *bare; u32 nbare; };
enum { STORE_CMP_NOTHING = 0, STORE_CMP_UNKNOWN = 1 };   // 2, 4, 6: stale, the value is the query_flags (SCID_QF_UPDATE1 | SCID_QF_UPDATE2)
LAMD_HD u32 store_cmp_find(const u64 *a, u32 n, u64 key) {   // the index of key in a[0, n) (ascending), STORE_NONE: not there
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < n && a[lo] == key ? lo : STORE_NONE;
}
// entry k of accepted message m.  An unset slot of ours is 0 in the digest, so `theirs > ours` is want_update()'s `timestamp != 0` there.
LAMD_HD u32 store_cmp_entry(const u8 *msgs, const store_cmp_msg &m, u32 k, const store_cmp_digest &d, u64 *scid) {
  *scid = store_be64(msgs + m.scid_at + 8 * (u64)k);
  u32 theirs[2] = {0, 0}, ours[2] = {0, 0};
  if (m.ts_at != STORE_CMP_NO_TS) {
    theirs[0] = store_be32(msgs + m.ts_at + 8 * (u64)k);
    theirs[1] = store_be32(msgs + m.ts_at + 8 * (u64)k + 4);
  }
  const u32 j = store_cmp_find(d.scid, d.count, *scid);
  if (j != STORE_NONE) {
    ours[0] = d.ts[2 * (size_t)j];
    ours[1] = d.ts[2 * (size_t)j + 1];
  } else if (store_cmp_find(d.bare, d.nbare, *scid) == STORE_NONE) {
    return STORE_CMP_UNKNOWN;
  }
  return (theirs[0] > ours[0] ? 2u : 0u) | (theirs[1] > ours[1] ? 4u : 0u);
}
// ---- the merge: does element j of a sorted list open a run of equal scids?
LAMD_HD bool store_cmp_head(const u64 *key, u32 j) { return j == 0 || key[j] != key[j - 1]; }

// ---- query_short_channel_ids.  be16 261 | chain_hash 32 | be16 1 + 8k | 0x00 | k be64 scids, and for the stale list behind it
// 0x01 | bigsize 1 + k | 0x00 | k flag bytes (every flag is below 0xfd: one byte of bigsize each).  The messages of the unknown list
// come first, max_unknown scids each except the last, then those of the stale list, max_stale each.
constexpr u32 STORE_CMP_MAX_UNKNOWN = 8000, STORE_CMP_MAX_STALE = 7000;   // gossipd/seeker.c:297, :382
constexpr u32 STORE_CMP_QUERY_HEAD = 37;
struct store_cmp_layout {
  u32 unknown, stale;           // the merged lists' lengths
  u32 max_unknown, max_stale;   // >= 1
  u8 chain[32];
};
LAMD_HD u32 store_cmp_msgs_of(u32 count, u32 per) { return (u32)(((u64)count + per - 1) / per); }
LAMD_HD u32 store_cmp_query_bytes(u32 k, bool stale) {
  return STORE_CMP_QUERY_HEAD + 8 * k + (stale ? 1 + store_bigsize_len(1 + (u64)k) + 1 + k : 0);
}
// the size of the first j messages of one list (j <= its messages)
LAMD_HD u64 store_cmp_list_bytes(u32 count, u32 per, u64 j, bool stale) {
  const u64 full = (j < store_cmp_msgs_of(count, per) || count % per == 0) ? j : j - 1;   // ... of them with `per` entries
  return full * store_cmp_query_bytes(per, stale) + (full < j ? store_cmp_query_bytes(count % per, stale) : 0);
}
LAMD_HD u64 store_cmp_messages(const store_cmp_layout &y) {
  return (u64)store_cmp_msgs_of(y.unknown, y.max_unknown) + store_cmp_msgs_of(y.stale, y.max_stale);
}
// where message j starts in the output; j = store_cmp_messages(): the total
LAMD_HD u64 store_cmp_msg_off(const store_cmp_layout &y, u64 j) {
  const u64 mu = store_cmp_msgs_of(y.unknown, y.max_unknown);
  if (j <= mu) return store_cmp_list_bytes(y.unknown, y.max_unknown, j, false);
  return store_cmp_list_bytes(y.unknown, y.max_unknown, mu, false) + store_cmp_list_bytes(y.stale, y.max_stale, j - mu, true);
}
// byte x of message j (x < its size); flags: one word per stale scid
LAMD_HD u8 store_cmp_msg_byte(const store_cmp_layout &y, const u64 *unknown, const u64 *stale, const u32 *flags, u32 j, u32 x) {
  const u32 mu = store_cmp_msgs_of(y.unknown, y.max_unknown);
  const bool st = j >= mu;
  const u32 per = st ? y.max_stale : y.max_unknown, count = st ? y.stale : y.unknown;
  const u64 base = (u64)(st ? j - mu : j) * per;
  const u32 k = count - base < per ? (u32)(count - base) : per;
  if (x < 2) return store_range_be(261, 2, x);
  if (x < 34) return y.chain[x - 2];
  if (x < 36) return store_range_be(1 + 8 * k, 2, x - 34);
  if (x < 37) return 0;   // encoding: uncompressed
  const u32 s = x - STORE_CMP_QUERY_HEAD;   // behind the head: the scids
  if (s < 8 * k) return store_range_be((st ? stale : unknown)[base + s / 8], 8, s & 7);
  const u32 t = s - 8 * k, ll = store_bigsize_len(1 + (u64)k);   // behind them: the flags' TLV
  if (t < 1) return 1;
  if (t < 1 + ll) return store_range_bigsize_byte(1 + k, t - 1);
  if (t < 2 + ll) return 0;   // encoding: uncompressed
  return (u8)flags[base + t - 2 - ll];
}
// Word k of the output, as store_range_word: the bytes B0 = 4k - mis .. B0 + 3 with mis = out & 3; total = msg_off[n_msgs]
LAMD_HD void store_cmp_word(const store_cmp_layout &y, const u64 *msg_off, u32 n_msgs, const u64 *unknown, const u64 *stale, const u32 *flags, u8 *out,
                            u64 total, u32 mis, u64 k) {
  if (4 * k + 4 <= mis) return;
  const u64 B0 = 4 * k < mis ? 0 : 4 * k - mis;
  if (B0 >= total) return;
  u32 j = store_range_locate(msg_off, n_msgs, B0), w = 0;
  const bool whole = 4 * k >= mis && B0 + 4 <= total;
  for (u32 b = 0; b < 4; b++) {
    if (4 * k + b < mis) continue;
    const u64 B = 4 * k + b - mis;
    if (B >= total) break;
    while (j + 1 < n_msgs && msg_off[j + 1] <= B) j++;   // a query has 45 bytes at least: one step
    const u8 v = store_cmp_msg_byte(y, unknown, stale, flags, j, (u32)(B - msg_off[j]));
    if (whole) w |= (u32)v << (8 * b); else out[B] = v;
  }
  if (whole) *(u32 *)__builtin_assume_aligned(out + B0, 4) = w;
}

}  // namespace lamd

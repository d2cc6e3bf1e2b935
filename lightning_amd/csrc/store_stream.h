// Streaming a store image to peers that sent gossip_timestamp_filter: the per-record, per-peer and per-tile logic of
// lamd_gossip_store_stream_build / lamd_timestamp_filter_reply_batch (include/lightning_amd.h), as inline functions that compile for gfx950
// and, unchanged, for the host (tests/c/store_stream_host.cpp runs them under the sanitizers).
//   - what gossmap_stream_next (common/gossmap.c:1873-1981) hands out: a record with DELETED and DYING clear whose type is 256, 257 or 258,
//     and, as the digest has it, one that counts (verdict OK where verdicts are given) and lies inside the image;
//   - the recent position (update_recent_timestamp, connectd/connectd.c:2287-2300; gossmap_iter_fast_forward, gossmap.c:1984-2004) as a
//     bisection in the prefix maximum of ALL records' header timestamps;
//   - the parser of a filter (handle_gossip_timestamp_filter_in, connectd/multiplex.c:844-902).  be16 265 | chain_hash 32 | be32
//     first_timestamp | be32 timestamp_range, 42 bytes; bytes behind them are ignored: the generated fromwire_ of a message ends with
//     `return cursor != NULL;` (tools/gen/impl_template:410) and does not look at what is left;
//   - one tile of 64 entries of the walk maybe_gossip_msg (multiplex.c:622-701) does one record per wakeup: which lanes pass the filter,
//     which of them are taken under the byte budget, where the walk stops.
// The encoder is store_query.h's store_sq_word, unchanged: every message here is the copy of a record.
// Every read of the image stays inside [store, store + store_len) whatever rec_off holds.
#pragma once
#include "store_query.h"

namespace lamd {

constexpr u32 STORE_FLAG_DYING = 0x0800;

// ---- the stream index.  What record i is to a stream; the first reason in this order decides.
enum {
  STORE_STREAM_OK = 0,        // streamable
  STORE_STREAM_FRAME = 1,     // its header, or its whole message, is not inside the image, or the message has no type
  STORE_STREAM_DELETED = 2,
  STORE_STREAM_VERDICT = 3,   // verdicts are given and verdict[i] != LAMD_STORE_OK
  STORE_STREAM_DYING = 4,
  STORE_STREAM_TYPE = 5,      // not 256, 257 or 258
  STORE_STREAM_CLASSES = 6
};
// *hts: the header timestamp as the fast-forward reads it (0: no header inside the image), whatever the class; *ts, *len: the header
// timestamp and the message length of a streamable record
LAMD_HD u32 store_stream_class(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, u32 *hts, u32 *ts, u32 *len) {
  *hts = *ts = *len = 0;
  const u64 off = rec_off[i];
  if (off > store_len || store_len - off < STORE_HDR) return STORE_STREAM_FRAME;
  const store_hdr h = store_read_hdr(store + off);
  *hts = h.ts;
  if (h.flags & STORE_FLAG_DELETED) return STORE_STREAM_DELETED;
  if (verdict && verdict[i] != LAMD_STORE_OK) return STORE_STREAM_VERDICT;
  if (h.flags & STORE_FLAG_DYING) return STORE_STREAM_DYING;
  if (store_len - off - STORE_HDR < h.len || h.len < 2) return STORE_STREAM_FRAME;
  const u32 t = store_be16(store + off + STORE_HDR);
  if (t != STORE_T_CANN && t != STORE_T_NANN && t != STORE_T_CUPD) return STORE_STREAM_TYPE;
  *ts = h.ts;
  *len = h.len;
  return STORE_STREAM_OK;
}
// recent(T): pmax[n] is the inclusive prefix maximum of the n records' header timestamps, so it is monotone and its first element >= T is
// the first record whose timestamp is >= T; spos[n + 1] counts the streamable records in front of each record, spos[n] is all of them
LAMD_HD u32 store_stream_recent(const u32 *pmax, const u32 *spos, u32 n, u32 T) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (pmax[mid] < T) lo = mid + 1; else hi = mid;
  }
  return spos[lo];
}

// ---- gossip_timestamp_filter
enum { STORE_TF_STREAMED = 0, STORE_TF_FOREIGN = 1, STORE_TF_MALFORMED = -1 };
enum { STORE_TF_FROM_START = 0, STORE_TF_FROM_END = 1, STORE_TF_FROM_RECENT = 2 };
constexpr u32 STORE_TF_BYTES = 42;
constexpr u32 STORE_TF_RECENT_SECONDS = 7200;
constexpr u64 STORE_TF_AS_FILTER = ~(u64)0;   // the cursor "as the filter says"
struct store_tf_filter {
  int32_t status;   // STORE_TF_*
  u32 min, max;     // a record with header timestamp ts != 0 is sent if min <= ts <= max
  u32 rule;         // STORE_TF_FROM_*: where the stream starts
};
LAMD_HD store_tf_filter store_tf_parse(const u8 *f, size_t len, const u8 *our_chain32) {
  store_tf_filter r;
  r.status = STORE_TF_MALFORMED;
  r.min = r.max = 0;
  r.rule = STORE_TF_FROM_END;
  if (len < STORE_TF_BYTES || store_be16(f) != 265) return r;
  u32 same = 0;
  for (int b = 0; b < 32; b++) same |= (u32)(f[2 + b] ^ our_chain32[b]);
  if (same) { r.status = STORE_TF_FOREIGN; return r; }
  const u32 first = store_be32(f + 34), range = store_be32(f + 38);
  r.status = STORE_TF_STREAMED;
  r.min = first;
  r.max = first + range - 1;   // in 32 bits, as the reference computes it
  if (r.max < r.min) r.max = 0xFFFFFFFFu;
  r.rule = first == 0 ? STORE_TF_FROM_START : first == 0xFFFFFFFFu ? STORE_TF_FROM_END : STORE_TF_FROM_RECENT;
  return r;
}
// one peer of a batch as the walk reads it
struct store_tf_peer {
  int32_t status;
  u32 min, max, rule;
  u64 cursor;       // a position in the streamable list, or STORE_TF_AS_FILTER
  int64_t budget;   // bytes; < 0: nothing is taken
};
// the index as the walk reads it
struct store_tf_index {
  const u32 *srec, *sts, *slen, *spos, *pmax;
  u32 n, n_stream;
};
// where the walk of peer p starts; now: the clock, in seconds
LAMD_HD u64 store_tf_start(const store_tf_index &x, const store_tf_peer &p, u32 now) {
  if (p.cursor != STORE_TF_AS_FILTER) return p.cursor;
  if (p.rule == STORE_TF_FROM_START) return 0;
  if (p.rule == STORE_TF_FROM_END) return x.n_stream;
  return store_stream_recent(x.pmax, x.spos, x.n, now - STORE_TF_RECENT_SECONDS);   // in 32 bits: now < 7200 wraps, as in the reference
}
LAMD_HD bool store_tf_pass(u32 ts, u32 min, u32 max) { return ts == 0 || (min <= ts && ts <= max); }
// A tile: 64 consecutive entries.  carry: the bytes taken in front of the tile; incl: the sum of the PASSING entries' lengths up to and
// including this lane.  A message is sent while the bytes sent so far are <= budget, the check comes before the message: the lane whose
// message makes the total exceed the budget is still taken, and is the last one.
LAMD_HD bool store_tf_stops(bool pass, u64 carry, u32 incl, int64_t budget) { return pass && (int64_t)(carry + incl) > budget; }
// the lanes taken: the passing ones up to and including the first stopping one
LAMD_HD u64 store_tf_taken(u64 pass_mask, u64 stop_mask) {
  if (!stop_mask) return pass_mask;
  const u64 first = stop_mask & (~stop_mask + 1);
  return pass_mask & (first | (first - 1));
}
LAMD_HD u32 store_tf_first_lane(u64 mask) {   // mask != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return (u32)__ffsll((long long)mask) - 1;
#else
  u32 l = 0;
  while (!((mask >> l) & 1)) l++;
  return l;
#endif
}

}  // namespace lamd

// gossip_store repair: the per-record and per-output-word logic of lamd_gossip_store_repair (include/lightning_amd.h), as inline functions
// that compile for gfx950 and, unchanged, for the host (tests/c/store_repair_host.cpp runs them under the sanitizers).
//   - the keep rules: which records of an audited store go into the rewritten one, and why the others do not (a reason byte per record);
//   - the node table over the node ids of the kept channel_announcements (open addressing, keys compared as the 33 bytes in the image,
//     lowest record index wins: the discipline of the scid index in store_audit.h);
//   - the head of the rewritten store (version byte + a fresh uuid record);
//   - the copy, one aligned 32-bit word of the OUTPUT at a time: the record an output byte belongs to is found by binary search in the
//     exclusive scan of the kept sizes, the word is put together from two aligned words of the source.
// Every read stays inside [store, store + store_len): the image on the device need not be the file the host walked.
#pragma once
#include "store_audit.h"

namespace lamd {

enum { STORE_DROP_KEPT = 0, STORE_DROP_DELETED = 1, STORE_DROP_VERDICT = 2, STORE_DROP_DEPENDENCY = 3, STORE_DROP_BOOKKEEPING = 4 };
constexpr u32 STORE_UUID_MSG = 34;                                 // be16 4107 | 32 bytes
constexpr u32 STORE_REPAIR_HEAD = 1 + STORE_HDR + STORE_UUID_MSG;  // version byte + the uuid record: 47 bytes in front of the first kept record
constexpr u32 STORE_SCAN_TILE = 256;                               // records per block of the scan kernels (one per lane)
constexpr u64 STORE_NODE_EMPTY = ~(u64)0;                          // empty slot of the node table

LAMD_HD u32 store_be16(const u8 *p) { return ((u32)p[0] << 8) | p[1]; }
// the record at `off` is a live channel_announcement: these are k_store_keep_chan's records, every other one is k_store_keep_rest's
LAMD_HD bool store_is_live_cann(const u8 *store, size_t store_len, u64 off) {
  u32 len;
  const u8 *m = store_live_msg(store, store_len, off, &len);
  return m && len >= 2 && store_be16(m) == STORE_T_CANN;
}

// ---- the node table: keys[1 << bits] (all STORE_NODE_EMPTY) hold the image offset of a 33-byte node id, vals[1 << bits] (all STORE_NONE)
// end as the LOWEST record index among the kept announcements that name that node: deterministic whatever the order of insertion.  The
// table has room for twice the ids of all live announcements; a probe sequence is nevertheless cut off after one round (an id that finds
// no slot is not in the table: its node_announcements are dropped, never kept by mistake).
LAMD_HD u32 store_node_home(const u8 *id33, u32 bits) {
  u64 h = 0x9E3779B97F4A7C15ull;
  for (int o = 0; o < 33; o += 8) {
    u64 w = 0;
    for (int b = 0; b < 8 && o + b < 33; b++) w |= (u64)id33[o + b] << (8 * b);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  return (u32)((h * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}
LAMD_HD bool store_node_eq(const u8 *a, const u8 *b) {
  u32 d = 0;
  for (int i = 0; i < 33; i++) d |= (u32)(a[i] ^ b[i]);
  return d == 0;
}
// idoff: offset in the image of a node id of kept announcement `rec` (idoff + 33 <= store_len)
LAMD_HD void store_node_insert(const u8 *store, u64 *keys, u32 *vals, u32 bits, u64 idoff, u32 rec) {
  const u32 cap = (u32)1 << bits;
  u32 s = store_node_home(store + idoff, bits);
  for (u32 probes = 0; probes < cap; probes++, s = (s + 1) & (cap - 1)) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u64 old = atomicCAS((unsigned long long *)&keys[s], (unsigned long long)STORE_NODE_EMPTY, (unsigned long long)idoff);
#else
    const u64 old = keys[s];
    if (old == STORE_NODE_EMPTY) keys[s] = idoff;
#endif
    if (old == STORE_NODE_EMPTY || old == idoff || store_node_eq(store + old, store + idoff)) {
#if defined(__HIP_DEVICE_COMPILE__)
      atomicMin(&vals[s], rec);
#else
      if (rec < vals[s]) vals[s] = rec;
#endif
      return;
    }
  }
}
LAMD_HD u32 store_node_find(const u8 *store, const u64 *keys, const u32 *vals, u32 bits, const u8 *id33) {
  const u32 cap = (u32)1 << bits;
  u32 s = store_node_home(id33, bits);
  for (u32 probes = 0; probes < cap; probes++, s = (s + 1) & (cap - 1)) {
    const u64 k = keys[s];
    if (k == STORE_NODE_EMPTY) return STORE_NONE;
    if (store_node_eq(store + k, id33)) return vals[s];
  }
  return STORE_NONE;
}

// ---- the keep rules (the table in lightning_amd.h).  Both functions return the record's STORE_DROP_* reason and set *size to the bytes the
// record takes in the output: 12 + len when kept, else 0.
// A live channel_announcement (store_is_live_cann).  *idoff: image offset of node_id_1 (node_id_2 follows), set when kept.
LAMD_HD u32 store_keep_cann(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 n, u32 i, u32 *size, u64 *idoff) {
  *size = 0;
  if (verdict[i] != LAMD_STORE_OK) return STORE_DROP_VERDICT;
  u32 len, alen, io;
  u64 scid;
  const u8 *m = store_live_msg(store, store_len, rec_off[i], &len);
  if (!m || !store_cann_scid(m, len, &scid, &io) || len < io + 66) return STORE_DROP_VERDICT;   // (an OK verdict says it is neither)
  // the channel_amount record behind it: gossmap reads the amount from there without looking at what it is (gossmap.c:488-492)
  if (i + 1 >= n || verdict[i + 1] != LAMD_STORE_OK) return STORE_DROP_DEPENDENCY;
  const u8 *am = store_live_msg(store, store_len, rec_off[i + 1], &alen);
  if (!am || alen != 10 || store_be16(am) != STORE_T_AMOUNT) return STORE_DROP_DEPENDENCY;
  *size = (u32)STORE_HDR + len;
  *idoff = rec_off[i] + STORE_HDR + io;
  return STORE_DROP_KEPT;
}
// record j is a kept channel_announcement: reason[j] is read only where k_store_keep_chan wrote it
LAMD_HD bool store_kept_cann(const u8 *store, size_t store_len, const u64 *rec_off, const u8 *reason, u32 n, u32 j) {
  return j < n && store_is_live_cann(store, store_len, rec_off[j]) && reason[j] == STORE_DROP_KEPT;
}
// Every record that is NOT a live channel_announcement.  reason[] holds the announcements' reasons, (nkeys, nvals, nbits) their node ids.
LAMD_HD u32 store_keep_other(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 n, u32 i, const u64 *keys,
                             const u32 *vals, u32 bits, const u64 *nkeys, const u32 *nvals, u32 nbits, const u8 *reason, u32 *size) {
  *size = 0;
  const u64 off = rec_off[i];
  if (off <= store_len && store_len - off >= STORE_HDR && (store_read_hdr(store + off).flags & STORE_FLAG_DELETED)) return STORE_DROP_DELETED;
  u32 len;
  const u8 *m = store_live_msg(store, store_len, off, &len);
  if (m && verdict[i] == LAMD_STORE_NO_CHANNEL) return STORE_DROP_DEPENDENCY;   // the audit has already missed the announcement
  if (!m || len < 2 || verdict[i] != LAMD_STORE_OK) return STORE_DROP_VERDICT;
  switch (store_be16(m)) {
    case STORE_T_AMOUNT:
      if (i == 0 || !store_kept_cann(store, store_len, rec_off, reason, n, i - 1)) return STORE_DROP_DEPENDENCY;
      break;
    case STORE_T_CUPD:
    case STORE_T_DYING: {
      const bool upd = store_be16(m) == STORE_T_CUPD;
      if (upd ? len < 112 : len != 14) return STORE_DROP_VERDICT;   // chan_dying: be16 type | scid 8 | be32 deadline
      const u32 a = store_index_find(keys, vals, bits, store_be64(m + (upd ? 98 : 2)));
      if (a >= i || !store_kept_cann(store, store_len, rec_off, reason, n, a)) return STORE_DROP_DEPENDENCY;   // (STORE_NONE is the largest index)
      break;
    }
    case STORE_T_NANN: {   // be16 type | signature 64 | be16 flen | features | be32 timestamp | node_id 33
      if (len < 68) return STORE_DROP_VERDICT;
      const u32 io = 68 + store_be16(m + 66) + 4;
      if (len < io + 33) return STORE_DROP_VERDICT;
      if (store_node_find(store, nkeys, nvals, nbits, m + io) >= i) return STORE_DROP_DEPENDENCY;
      break;
    }
    case STORE_T_DELETE_CHAN:
    case STORE_T_UUID:
    case STORE_T_ENDED:
      return STORE_DROP_BOOKKEEPING;
    default:
      return STORE_DROP_VERDICT;   // (an OK verdict says the type is known, and a live 256 never comes here)
  }
  *size = (u32)STORE_HDR + len;
  return STORE_DROP_KEPT;
}

// ---- the head of the output: the input's version byte, then the uuid record (flags COMPLETED, timestamp 0, crc32c seeded with 0)
struct store_head { u8 b[STORE_REPAIR_HEAD + 1]; };
LAMD_HD store_head store_make_head(u8 version, const u8 *uuid32) {
  store_head h;
  u32 T[4 * 256];
  store_crc_build_tables(T, 4);
  u8 *msg = h.b + 1 + STORE_HDR;
  msg[0] = STORE_T_UUID >> 8;
  msg[1] = STORE_T_UUID & 0xff;
  for (int i = 0; i < 32; i++) msg[2 + i] = uuid32[i];
  const u32 crc = store_crc32c<4>(T, 0, msg, STORE_UUID_MSG);
  h.b[0] = version;
  h.b[1] = STORE_FLAG_COMPLETED >> 8;
  h.b[2] = 0;
  h.b[3] = 0;
  h.b[4] = STORE_UUID_MSG;
  for (int i = 0; i < 4; i++) { h.b[5 + i] = (u8)(crc >> (24 - 8 * i)); h.b[9 + i] = 0; }
  h.b[STORE_REPAIR_HEAD] = 0;
  return h;
}

// ---- the copy.  pos[0..n] = exclusive scan of the sizes (pos[n] = their sum): payload byte x of the output (output byte STORE_REPAIR_HEAD +
// x) belongs to the LAST record r with pos[r] <= x -- dropped records have size 0 and share their pos with the kept one behind them.
// The copy reads pos[] and rec_off[] through a view: the arrays themselves, or the window [lo, lo + STORE_PACK_STAGE] of them a block has
// staged in LDS (pos relative to pos[lo], 32 bits: the records of one block's words span far less) -- the search is a chain of dependent
// loads, and in LDS a link of it costs a fraction of what it costs in global memory.
constexpr u32 STORE_PACK_STAGE = 2048;
struct store_pack_global { const u64 *rec_off, *pos; };
struct store_pack_staged { const u64 *rec_off; const u32 *rel; u32 lo; u64 base; };   // rec_off[j - lo], base + rel[j - lo]
LAMD_HD u64 store_pack_pos(const store_pack_global &v, u32 j) { return v.pos[j]; }
LAMD_HD u64 store_pack_pos(const store_pack_staged &v, u32 j) { return v.base + v.rel[j - v.lo]; }
LAMD_HD u64 store_pack_off(const store_pack_global &v, u32 j) { return v.rec_off[j]; }
LAMD_HD u64 store_pack_off(const store_pack_staged &v, u32 j) { return v.rec_off[j - v.lo]; }
// store_pack_locate: the record of payload byte x, searched in [lo, hi]; requires pos[lo] <= x
template <class V> LAMD_HD u32 store_pack_locate(const V &v, u32 lo, u32 hi, u64 x) {
  while (lo < hi) {
    const u32 mid = lo + (hi - lo + 1) / 2;
    if (store_pack_pos(v, mid) <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// c = 1..4 bytes of the image from offset s (s + c <= store_len), little-endian in the result: two aligned 32-bit loads shifted together
// where both lie inside the image, byte loads at its two ends
LAMD_HD u32 store_pack_gather(const u8 *store, size_t store_len, u64 s, u32 c) {
  const uintptr_t p = (uintptr_t)(store + s), a = p & ~(uintptr_t)3;
  u32 v = 0;
  if (a >= (uintptr_t)store && a + 8 <= (uintptr_t)store + store_len) {
    const u32 sh = 8 * (u32)(p & 3), w0 = store_load32((const u8 *)a), w1 = store_load32((const u8 *)a + 4);
    v = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
  } else {
    for (u32 b = 0; b < c; b++) v |= (u32)store[s + b] << (8 * b);
  }
  return c < 4 ? v & (((u32)1 << (8 * c)) - 1) : v;
}
// c = 1..4 payload bytes from x (x + c <= pos[n]); a kept record has 12 bytes at least, so they lie in two records at most
template <class V> LAMD_HD u32 store_pack_bytes(const u8 *store, size_t store_len, const V &v, u32 lo, u32 hi, u64 x, u32 c) {
  const u32 r = store_pack_locate(v, lo, hi, x);
  const u64 avail = store_pack_pos(v, r + 1) - x;
  const u32 c0 = avail < c ? (u32)avail : c;
  u32 w = store_pack_gather(store, store_len, store_pack_off(v, r) + (x - store_pack_pos(v, r)), c0);
  if (c0 < c) {
    const u32 r2 = store_pack_locate(v, r + 1, hi, x + c0);
    w |= store_pack_gather(store, store_len, store_pack_off(v, r2) + (x + c0 - store_pack_pos(v, r2)), c - c0) << (8 * c0);
  }
  return w;
}
// Word k of the output: the bytes B0 = 4k - mis .. B0 + 3, where mis = out & 3, so that out + B0 is 4-aligned.  lim = the bytes to write
// (min(capacity, STORE_REPAIR_HEAD + pos[n])).  A word that lies in the payload and inside lim is ONE aligned store; the words that
// touch the head, byte 0 or lim go byte by byte.  [lo, hi]: records that hold every payload byte of this word (0 and n - 1 will do).
template <class V> LAMD_HD void store_pack_word(const u8 *store, size_t store_len, const V &v, u32 lo, u32 hi, const store_head &head, u8 *out, u64 lim,
                                                u32 mis, u64 k) {
  const u64 B1 = 4 * k + 4 - mis;   // one past the word's last byte
  if (B1 >= STORE_REPAIR_HEAD + 4 && B1 <= lim) {
    *(u32 *)__builtin_assume_aligned(out + (B1 - 4), 4) = store_pack_bytes(store, store_len, v, lo, hi, B1 - 4 - STORE_REPAIR_HEAD, 4);
    return;
  }
  for (u32 b = 0; b < 4; b++) {
    if (4 * k + b < mis) continue;
    const u64 B = 4 * k + b - mis;
    if (B >= lim) break;
    out[B] = B < STORE_REPAIR_HEAD ? head.b[B] : (u8)store_pack_bytes(store, store_len, v, lo, hi, B - STORE_REPAIR_HEAD, 1);
  }
}

}  // namespace lamd

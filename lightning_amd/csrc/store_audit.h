// gossip_store audit: the per-record logic of lamd_gossip_store_frame / lamd_gossip_store_audit (include/lightning_amd.h), as inline
// functions that compile for gfx950 and, unchanged, for the host (tests/c/store_audit_host.cpp runs them under the sanitizers).
//   - the CRC-32C of a record as ccan/crc32c computes it (Castagnoli, reflected polynomial 0x82F63B78, seed = the header's timestamp:
//     gossip_store.c:67), table driven with 4- or 8-way slicing;
//   - the classification of a record before any signature is looked at (deleted / checksum / type);
//   - the scid index over the live channel_announcements (open addressing, lowest record index wins) and the signer look-up of a
//     channel_update (gossmap_manage.c:920-922 does it with the gossmap);
//   - the merge of all of it into the record's verdict;
//   - the sequential walk over the file's headers, as common/gossmap.c map_catchup() (:815-937) does it.
#pragma once
#include "lamd_common.h"
#include "../../include/lightning_amd.h"

namespace lamd {

// struct gossip_hdr (common/gossip_store.h:44-49): be16 flags | be16 len | be32 crc | be32 timestamp, then len bytes of message
constexpr size_t STORE_HDR = 12;
constexpr u32 STORE_FLAG_DELETED = 0x8000, STORE_FLAG_COMPLETED = 0x2000;
enum {
  STORE_T_CANN = 256, STORE_T_NANN = 257, STORE_T_CUPD = 258,
  STORE_T_AMOUNT = 4101, STORE_T_DELETE_CHAN = 4103, STORE_T_ENDED = 4105, STORE_T_DYING = 4106, STORE_T_UUID = 4107
};
constexpr u32 STORE_NONE = 0xFFFFFFFFu;             // "no record" / "no selection row"
constexpr u64 STORE_EMPTY_KEY = ~(u64)0;            // empty slot of the scid index; the scid of that value lives in the extra slot `cap`
enum { STORE_AUX_REDUNDANT = 1, STORE_AUX_NO_CHANNEL = 2 };

struct store_hdr { u32 flags, len, crc, ts; };
LAMD_HD store_hdr store_read_hdr(const u8 *h) {
  store_hdr r;
  r.flags = ((u32)h[0] << 8) | h[1];
  r.len = ((u32)h[2] << 8) | h[3];
  r.crc = ((u32)h[4] << 24) | ((u32)h[5] << 16) | ((u32)h[6] << 8) | h[7];
  r.ts = ((u32)h[8] << 24) | ((u32)h[9] << 16) | ((u32)h[10] << 8) | h[11];
  return r;
}
LAMD_HD bool store_known_type(u32 t) {
  return t == STORE_T_CANN || t == STORE_T_NANN || t == STORE_T_CUPD || t == STORE_T_AMOUNT || t == STORE_T_DELETE_CHAN || t == STORE_T_ENDED ||
         t == STORE_T_DYING || t == STORE_T_UUID;
}

// ---- CRC-32C.  Table k, entry i = the CRC state after byte i followed by k zero bytes: T[0] from the bitwise definition, T[k][i] =
// (T[k-1][i] >> 8) ^ T[0][T[k-1][i] & 0xff] -- every further table reads T[0] only, so a block builds all of them behind ONE barrier.
LAMD_HD u32 store_crc_t0(u32 i) {
  u32 c = i;
  for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
  return c;
}
LAMD_HD void store_crc_build_tables(u32 *T, int ways) {
  for (u32 i = 0; i < 256; i++) T[i] = store_crc_t0(i);
  for (int k = 1; k < ways; k++)
    for (u32 i = 0; i < 256; i++) T[256 * k + i] = (T[256 * (k - 1) + i] >> 8) ^ T[T[256 * (k - 1) + i] & 0xff];
}
LAMD_HD u32 store_load32(const u8 *p) { return *(const u32 *)__builtin_assume_aligned(p, 4); }  // little-endian hosts and gfx950 alike
// crc32c(seed, p, len) with WAYS x 256 tables at T (LDS on the device).  A record starts at any byte offset: bytes one by one until the
// pointer is 4-aligned, then 32-bit loads (one per step with 4 ways, two with 8), then the tail bytes.
template <int WAYS> LAMD_HD u32 store_crc32c(const u32 *T, u32 seed, const u8 *p, size_t len) {
  static_assert(WAYS == 4 || WAYS == 8, "slicing by 4 or by 8");
  u32 c = ~seed;
  while (len && ((uintptr_t)p & 3)) { c = T[(c ^ *p++) & 0xff] ^ (c >> 8); len--; }
  if (WAYS == 4) {
    for (; len >= 4; p += 4, len -= 4) {
      const u32 a = store_load32(p) ^ c;
      c = T[768 + (a & 0xff)] ^ T[512 + ((a >> 8) & 0xff)] ^ T[256 + ((a >> 16) & 0xff)] ^ T[a >> 24];
    }
  } else {
    for (; len >= 8; p += 8, len -= 8) {
      const u32 a = store_load32(p) ^ c, b = store_load32(p + 4);
      c = T[1792 + (a & 0xff)] ^ T[1536 + ((a >> 8) & 0xff)] ^ T[1280 + ((a >> 16) & 0xff)] ^ T[1024 + (a >> 24)] ^
          T[768 + (b & 0xff)] ^ T[512 + ((b >> 8) & 0xff)] ^ T[256 + ((b >> 16) & 0xff)] ^ T[b >> 24];
    }
  }
  for (; len; len--) c = T[(c ^ *p++) & 0xff] ^ (c >> 8);
  return ~c;
}

// ---- what a record is before any signature is looked at: SKIPPED_DELETED, BAD_CHECKSUM, UNKNOWN_TYPE or 0 (goes on).  `off` is the offset
// of the record's gossip_hdr; a record that does not lie inside the image cannot be checksummed and is reported as BAD_CHECKSUM (the host
// walk never hands one over: this guards an image on the device that is not the file the host walked).
template <int WAYS> LAMD_HD int store_precheck_one(const u32 *T, const u8 *store, size_t store_len, u64 off) {
  if (off > store_len || store_len - off < STORE_HDR) return LAMD_STORE_BAD_CHECKSUM;
  const store_hdr h = store_read_hdr(store + off);
  if (h.flags & STORE_FLAG_DELETED) return LAMD_STORE_SKIPPED_DELETED;
  if (store_len - off - STORE_HDR < h.len) return LAMD_STORE_BAD_CHECKSUM;
  const u8 *m = store + off + STORE_HDR;
  if (store_crc32c<WAYS>(T, h.ts, m, h.len) != h.crc) return LAMD_STORE_BAD_CHECKSUM;
  if (h.len < 2 || !store_known_type(((u32)m[0] << 8) | m[1])) return LAMD_STORE_UNKNOWN_TYPE;
  return LAMD_STORE_OK;
}

// a LIVE record's message, or nullptr (deleted, or outside the image)
LAMD_HD const u8 *store_live_msg(const u8 *store, size_t store_len, u64 off, u32 *len) {
  if (off > store_len || store_len - off < STORE_HDR) return nullptr;
  const store_hdr h = store_read_hdr(store + off);
  if ((h.flags & STORE_FLAG_DELETED) || store_len - off - STORE_HDR < h.len) return nullptr;
  *len = h.len;
  return store + off + STORE_HDR;
}
LAMD_HD u64 store_be64(const u8 *p) {
  u64 v = 0;
  for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
  return v;
}
// channel_announcement: 4 signatures | u16 flen | features | chain_hash 32 | scid 8 | node_id_1 33 | node_id_2 33 | ... (add_channel,
// common/gossmap.c:451-476).  false = not a channel_announcement long enough to hold its scid.
LAMD_HD bool store_cann_scid(const u8 *m, u32 len, u64 *scid, u32 *idoff) {
  if (len < 260 || (((u32)m[0] << 8) | m[1]) != STORE_T_CANN) return false;
  const u32 so = 260 + (((u32)m[258] << 8) | m[259]) + 32;
  if (len < so + 8) return false;
  *scid = store_be64(m + so);
  *idoff = so + 8;
  return true;
}

// ---- the scid index: keys[cap + 1] (all STORE_EMPTY_KEY), vals[cap + 1] (all STORE_NONE), cap = 2^bits >= 2 x the live announcements.
// vals[s] ends as the LOWEST record index among the live announcements of keys[s]: deterministic whatever the order of insertion.
LAMD_HD u32 store_index_home(u64 scid, u32 bits) { return (u32)((scid * 0x9E3779B97F4A7C15ull) >> (64 - bits)); }
LAMD_HD void store_index_insert(u64 *keys, u32 *vals, u32 bits, u64 scid, u32 rec) {
  const u32 cap = (u32)1 << bits;
  u32 s = cap;  // the scid that looks like an empty slot has a slot of its own
  if (scid != STORE_EMPTY_KEY) {
    for (s = store_index_home(scid, bits);; s = (s + 1) & (cap - 1)) {
#if defined(__HIP_DEVICE_COMPILE__)
      const u64 old = atomicCAS((unsigned long long *)&keys[s], (unsigned long long)STORE_EMPTY_KEY, (unsigned long long)scid);
#else
      const u64 old = keys[s];
      if (old == STORE_EMPTY_KEY) keys[s] = scid;
#endif
      if (old == STORE_EMPTY_KEY || old == scid) break;
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(&vals[s], rec);
#else
  if (rec < vals[s]) vals[s] = rec;
#endif
}
LAMD_HD u32 store_index_find(const u64 *keys, const u32 *vals, u32 bits, u64 scid) {
  const u32 cap = (u32)1 << bits;
  if (scid == STORE_EMPTY_KEY) return vals[cap];
  for (u32 s = store_index_home(scid, bits);; s = (s + 1) & (cap - 1)) {
    const u64 k = keys[s];
    if (k == scid) return vals[s];
    if (k == STORE_EMPTY_KEY) return STORE_NONE;
  }
}
// record `rec` is a live channel_announcement that holds an scid: into the index
LAMD_HD void store_index_one(const u8 *store, size_t store_len, u64 off, u32 rec, u64 *keys, u32 *vals, u32 bits) {
  u32 len, idoff;
  u64 scid;
  const u8 *m = store_live_msg(store, store_len, off, &len);
  if (m && store_cann_scid(m, len, &scid, &idoff)) store_index_insert(keys, vals, bits, scid, rec);
}
// What the index says about record `rec` (returns STORE_AUX_* bits):
//   channel_announcement -- REDUNDANT when a live announcement of its scid has a lower record index;
//   channel_update of >= 112 bytes (scid at 98, channel_flags at 111) -- its signer: node_id_1 / node_id_2 by channel_flags & 1 of the live
//   announcement of its scid with a LOWER record index, copied to id33; NO_CHANNEL (id33 zeroed) when there is none, or when that
//   announcement is cut off before the node id.  Every other record: id33 zeroed (gossip_expand_one calls a shorter update malformed).
LAMD_HD u32 store_signer_one(const u8 *store, size_t store_len, const u64 *rec_off, u32 rec, const u64 *keys, const u32 *vals, u32 bits,
                             u8 *id33) {
  u32 len, aux = 0;
  const u8 *m = store_live_msg(store, store_len, rec_off[rec], &len), *id = nullptr;
  if (m && len >= 2) {
    const u32 type = ((u32)m[0] << 8) | m[1];
    u64 scid;
    u32 idoff;
    if (type == STORE_T_CANN && store_cann_scid(m, len, &scid, &idoff)) {
      if (store_index_find(keys, vals, bits, scid) != rec) aux = STORE_AUX_REDUNDANT;
    } else if (type == STORE_T_CUPD && len >= 112) {
      const u32 a = store_index_find(keys, vals, bits, store_be64(m + 98));
      aux = STORE_AUX_NO_CHANNEL;
      if (a < rec) {   // (STORE_NONE is the largest index)
        u32 alen, aoff;
        u64 ascid;
        const u8 *am = store_live_msg(store, store_len, rec_off[a], &alen);
        if (am && store_cann_scid(am, alen, &ascid, &aoff)) {
          aoff += 33 * (m[111] & 1);
          if (alen >= aoff + 33) { id = am + aoff; aux = 0; }
        }
      }
    }
  }
  if (id33)
    for (int b = 0; b < 33; b++) id33[b] = id ? id[b] : 0;
  return aux;
}
// the record's verdict, first match in the order of the table in lightning_amd.h: `pre` from store_precheck_one; a record with signature
// rows (has_sig) brings lamd_sigcheck_gossip_batch's verdict `sig` (-1, 0, 1..4) and the STORE_AUX_* bits
LAMD_HD int store_merge_one(int pre, bool has_sig, int sig, u32 aux) {
  if (pre != LAMD_STORE_OK || !has_sig) return pre;
  if (sig == -1) return LAMD_STORE_MALFORMED;
  if (aux & STORE_AUX_REDUNDANT) return LAMD_STORE_REDUNDANT;
  if (aux & STORE_AUX_NO_CHANNEL) return LAMD_STORE_NO_CHANNEL;
  return sig;
}

// ---- the walk (host): headers only, every read inside [0, len).  visit(index, off, hdr, type) is called for every record; type is 0 for a
// deleted record (its message is not looked at).  Returns false for a file that is no version-0 gossip_store (major version != 0).
template <class F> static inline bool store_walk(const u8 *store, size_t len, lamd_store_summary *s, F visit) {
  *s = lamd_store_summary();
  if (len < 1) return false;
  s->version = store[0];
  if (store[0] & 0xE0) return false;   // GOSSIP_STORE_MAJOR_VERSION_MASK (common/gossip_store.h)
  size_t off = 1;
  s->end_reason = LAMD_STORE_END_EOF;
  for (;;) {
    if (len - off < STORE_HDR) {
      if (off != len) s->end_reason = LAMD_STORE_END_PARTIAL_HEADER;
      break;
    }
    const store_hdr h = store_read_hdr(store + off);
    if (!(h.flags & STORE_FLAG_COMPLETED)) { s->end_reason = LAMD_STORE_END_INCOMPLETE; break; }
    if (len - off - STORE_HDR < h.len) { s->end_reason = LAMD_STORE_END_TRUNCATED; break; }
    const size_t next = off + STORE_HDR + h.len;
    u32 type = 0;
    if (!(h.flags & STORE_FLAG_DELETED)) {
      if (h.len < 2) { s->end_reason = LAMD_STORE_END_SHORT; break; }
      type = ((u32)store[off + STORE_HDR] << 8) | store[off + STORE_HDR + 1];
      // gossipd writes the channel_amount record right behind the announcement: until it is there the announcement is not read (gossmap.c:488-492)
      if (type == STORE_T_CANN && len - next < STORE_HDR + 2 + 8) { s->end_reason = LAMD_STORE_END_NO_AMOUNT; break; }
      s->live++;
    } else {
      s->deleted++;
    }
    visit((size_t)s->records, (u64)off, h, type);
    s->records++;
    off = next;
    if (type == STORE_T_ENDED) { s->end_reason = LAMD_STORE_END_STORE_ENDED; break; }
  }
  s->end_offset = off;
  return true;
}

}  // namespace lamd

// gossip_store latest-wins repair: the per-record logic of lamd_gossip_store_repair_latest (include/lightning_amd.h), as inline functions
// that compile for gfx950 and, unchanged, for the host (tests/c/store_latest_host.cpp runs them under the sanitizers).  On top of the keep
// rules of store_repair.h:
//   - the SIGNED timestamp of a node_announcement / channel_update, and whether the record is eligible (the header's timestamp equals it,
//     and it does not lie further ahead of the caller's clock than the policy allows);
//   - one winner per (channel, direction) and per node: a 64-bit key (timestamp << 32 | ~record index) per slot, written with atomicMax, so
//     that the highest timestamp wins and, among equal ones, the lowest record index -- whatever the order in which the lanes arrive.  That
//     is what gossipd's `prev_timestamp >= timestamp: ignore` (gossmap_manage.c:934-945, :1134-1143) leaves of records taken in file order;
//   - the prune rule (prune_network, gossmap_manage.c:409-471) for the announcements, read from those slots;
//   - the reasons 5..7 that follow from it.
// The stages, one function per record each: store_latest_upd_one (slots of the updates, dying marks), store_latest_cann_one (final
// announcements), store_latest_node_one (slots of the node_announcements), store_latest_other_one (every other record).  A stage reads
// what the stage before it wrote with atomics, so on the device each one is a launch of its own.
// Every read stays inside [store, store + store_len): the image on the device need not be the file the host walked.
#pragma once
#include "store_repair.h"

namespace lamd {

enum { STORE_DROP_SUPERSEDED = 5, STORE_DROP_TIMESTAMP = 6, STORE_DROP_STALE = 7 };

LAMD_HD u32 store_be32(const u8 *p) { return ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | p[3]; }

// ---- the slots.  0 = empty; a record's key is never 0 (its index is below STORE_NONE, so the low word is at least 1).
LAMD_HD u64 store_latest_key(u32 ts, u32 rec) { return ((u64)ts << 32) | (u32)~rec; }
LAMD_HD u32 store_latest_ts(u64 key) { return (u32)(key >> 32); }
LAMD_HD void store_latest_put(u64 *slot, u64 key) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax((unsigned long long *)slot, (unsigned long long)key);
#else
  if (key > *slot) *slot = key;
#endif
}

// ---- timestamps.  m / len: a live record's message.  true for a channel_update of >= 112 bytes (timestamp at 106, channel_flags at 111)
// and for a node_announcement that holds its node id (be16 type | signature 64 | be16 flen | features | be32 timestamp | node_id 33):
// the lengths store_keep_other asks for.  *idoff: offset of the node id in the message (257) / of the scid (258).
LAMD_HD bool store_signed_ts(const u8 *m, u32 len, u32 *type, u32 *ts, u32 *idoff) {
  if (len < 2) return false;
  *type = store_be16(m);
  if (*type == STORE_T_CUPD) {
    if (len < 112) return false;
    *ts = store_be32(m + 106);
    *idoff = 98;
    return true;
  }
  if (*type != STORE_T_NANN || len < 68) return false;
  const u32 to = 68 + store_be16(m + 66);
  if (len < to + 4 + 33) return false;
  *ts = store_be32(m + to);
  *idoff = to + 4;
  return true;
}
// the header's timestamp is the signed one, and the signed one is at most future_slack seconds ahead of the clock (64 bits, no wrap)
LAMD_HD bool store_ts_eligible(u32 hdr_ts, u32 ts, const lamd_store_latest_policy &pol) {
  if (hdr_ts != ts) return false;
  return pol.now == 0 || pol.now >= ts || (u64)ts - pol.now <= pol.future_slack;
}
// a slot's winner is older than the prune interval: timestamp < now - interval, written without the subtraction (now may be the smaller)
LAMD_HD bool store_ts_stale(u64 key, const lamd_store_latest_policy &pol) {
  return key != 0 && pol.now != 0 && pol.prune_interval != 0 && (u64)store_latest_ts(key) + pol.prune_interval < pol.now;
}
// the message of record i if it is a live, verdict-OK node_announcement / channel_update (else nullptr), with store_signed_ts's results and
// whether it is eligible
LAMD_HD const u8 *store_latest_msg(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i,
                                   const lamd_store_latest_policy &pol, u32 *type, u32 *ts, u32 *idoff, bool *eligible) {
  if (verdict[i] != LAMD_STORE_OK) return nullptr;
  u32 len;
  const u8 *m = store_live_msg(store, store_len, rec_off[i], &len);
  if (!m || !store_signed_ts(m, len, type, ts, idoff)) return nullptr;
  *eligible = store_ts_eligible(store_read_hdr(store + rec_off[i]).ts, *ts, pol);
  return m;
}

// the slot of a node id in the node table (STORE_NONE: not there): store_node_find, returning where instead of what
LAMD_HD u32 store_node_slot(const u8 *store, const u64 *keys, u32 bits, const u8 *id33) {
  const u32 cap = (u32)1 << bits;
  u32 s = store_node_home(id33, bits);
  for (u32 probes = 0; probes < cap; probes++, s = (s + 1) & (cap - 1)) {
    const u64 k = keys[s];
    if (k == STORE_NODE_EMPTY) return STORE_NONE;
    if (store_node_eq(store + k, id33)) return s;
  }
  return STORE_NONE;
}

// ---- stage 1, every record: an eligible channel_update behind its indexed announcement `a` goes into latest[2 * a + direction]
// (latest: 2 * n slots, all 0); a live, OK, 14-byte chan_dying record behind its indexed announcement sets dying[a] (n bytes, all 0).
// Whether `a` is kept is not asked: the slots of a dropped announcement are never read.
LAMD_HD void store_latest_upd_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *keys,
                                  const u32 *vals, u32 bits, const lamd_store_latest_policy &pol, u64 *latest, u8 *dying) {
  u32 type, ts, idoff, len;
  bool eligible;
  const u8 *m = store_latest_msg(store, store_len, rec_off, verdict, i, pol, &type, &ts, &idoff, &eligible);
  if (m) {
    if (type != STORE_T_CUPD || !eligible) return;
    const u32 a = store_index_find(keys, vals, bits, store_be64(m + 98));
    if (a < i) store_latest_put(&latest[2 * (size_t)a + (m[111] & 1)], store_latest_key(ts, i));   // (STORE_NONE is the largest index)
    return;
  }
  if (verdict[i] != LAMD_STORE_OK) return;
  m = store_live_msg(store, store_len, rec_off[i], &len);
  if (!m || len != 14 || store_be16(m) != STORE_T_DYING) return;
  const u32 a = store_index_find(keys, vals, bits, store_be64(m + 2));
  if (a < i) dying[a] = 1;
}

// ---- stage 2, a live channel_announcement (store_is_live_cann): store_keep_cann's reason, or STALE when it would be kept, no dying
// record names it, and the winner of one of its directions is older than the prune interval (a direction without update counts as fresh:
// get_timestamp() gives UINT32_MAX for it, gossmap_manage.c:383-396).  *size, *idoff as store_keep_cann.
LAMD_HD u32 store_latest_cann_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 n, u32 i,
                                  const lamd_store_latest_policy &pol, const u64 *latest, const u8 *dying, u32 *size, u64 *idoff) {
  const u32 r = store_keep_cann(store, store_len, rec_off, verdict, n, i, size, idoff);
  if (r != STORE_DROP_KEPT || dying[i]) return r;
  if (!store_ts_stale(latest[2 * (size_t)i], pol) && !store_ts_stale(latest[2 * (size_t)i + 1], pol)) return r;
  *size = 0;
  return STORE_DROP_STALE;
}

// ---- stage 3, every record: an eligible node_announcement whose node is in the table of the FINAL announcements with a lower record
// index goes into nlatest[its slot] (nlatest: parallel to nvals, all 0)
LAMD_HD void store_latest_node_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 i, const u64 *nkeys,
                                   const u32 *nvals, u32 nbits, const lamd_store_latest_policy &pol, u64 *nlatest) {
  u32 type, ts, idoff;
  bool eligible;
  const u8 *m = store_latest_msg(store, store_len, rec_off, verdict, i, pol, &type, &ts, &idoff, &eligible);
  if (!m || type != STORE_T_NANN || !eligible) return;
  const u32 s = store_node_slot(store, nkeys, nbits, m + idoff);
  if (s != STORE_NONE && nvals[s] < i) store_latest_put(&nlatest[s], store_latest_key(ts, i));
}

// ---- stage 4, every record that is not a live channel_announcement: store_keep_other against the final announcements and their node
// table; then, for a verdict-OK node_announcement / channel_update only: TIMESTAMP when it is not eligible (kept dependencies or not),
// SUPERSEDED when it is eligible, its dependencies are kept and its key is not the one in its slot.
LAMD_HD u32 store_latest_other_one(const u8 *store, size_t store_len, const u64 *rec_off, const int8_t *verdict, u32 n, u32 i, const u64 *keys,
                                   const u32 *vals, u32 bits, const u64 *nkeys, const u32 *nvals, u32 nbits, const u8 *reason,
                                   const lamd_store_latest_policy &pol, const u64 *latest, const u64 *nlatest, u32 *size) {
  const u32 r = store_keep_other(store, store_len, rec_off, verdict, n, i, keys, vals, bits, nkeys, nvals, nbits, reason, size);
  if (r != STORE_DROP_KEPT && r != STORE_DROP_DEPENDENCY) return r;
  u32 type, ts, idoff;
  bool eligible;
  const u8 *m = store_latest_msg(store, store_len, rec_off, verdict, i, pol, &type, &ts, &idoff, &eligible);
  if (!m) return r;
  if (!eligible) { *size = 0; return STORE_DROP_TIMESTAMP; }
  if (r != STORE_DROP_KEPT) return r;
  u64 winner;   // (kept: the look-ups below found the announcement / the node a moment ago)
  if (type == STORE_T_CUPD) {
    winner = latest[2 * (size_t)store_index_find(keys, vals, bits, store_be64(m + 98)) + (m[111] & 1)];
  } else {
    const u32 s = store_node_slot(store, nkeys, nbits, m + idoff);
    winner = s != STORE_NONE ? nlatest[s] : 0;
  }
  if (winner == store_latest_key(ts, i)) return r;
  *size = 0;
  return STORE_DROP_SUPERSEDED;
}

}  // namespace lamd

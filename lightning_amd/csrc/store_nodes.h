// Receiving node_announcement batches against a store image: the per-channel, per-message and per-row logic of
// lamd_node_announcement_receive_batch (include/lightning_amd.h), as inline functions that compile for gfx950 and, unchanged, for the host
// (tests/c/store_nodes_host.cpp runs them under the sanitizers).
//   - which nodes have a channel that is not dying (all_node_channels_dying(), gossipd/gossmap_manage.c:288-298): one channel at a time, a
//     plain store of 1 to both of its nodes' marks;
//   - the classification of a raw message in the order of gossmap_manage_node_announcement() (:1163-1248): framing, the TLV tail and the
//     signature's range (fromwire_node_announcement), the walk of the address descriptors (fromwire_wireaddr_array, common/wireaddr.c:30-69,
//     858-889), gossmap_find_node as a 33-byte bisection in the directory's ranked ids; the signer is the message's own node_id;
//   - what the signature's verdict makes of it, and the sort key of a candidate: its node's rank;
//   - "newer wins" (process_node_announcement(), :1122-1161) over the candidates sorted by rank, arrival order kept inside a rank: the running
//     maximum of (rank << 33) | (ts + 1) tells each row the timestamp in force in front of it; the HEADER timestamp of the node's record in the
//     image seeds it (gossip_store_get_timestamp);
//   - the plan: one store record per accepted message, the records the nodes held before.  The records are encoded by store_receive.h's
//     store_rx_header / store_rx_word, which the flags' bit values are shared with.
// Every read of the image stays inside [store, store + store_len), every read of the batch inside its messages.
#pragma once
#include "store_receive.h"
#include "verify_core.h"

namespace lamd {

enum {
  STORE_NR_MALFORMED = -1, STORE_NR_ACCEPTED = 0, STORE_NR_BAD_ADDRESSES = 1, STORE_NR_BAD_SIGNATURE = 2, STORE_NR_HELD = 3, STORE_NR_UNKNOWN = 4,
  STORE_NR_STALE = 5, STORE_NR_DUPLICATE = 6,
  STORE_NR_PENDING = 100   // between the stages: the message has a signature row (or, behind it, is a candidate)
};
constexpr u32 STORE_NR_MIN = 142, STORE_NR_MAX = 65535;   // every fixed field of a node_announcement without features; the longest wire message
constexpr u64 STORE_NR_MAX_NODES = (u64)1 << 30;          // so that (rank << 33) | (ts + 1) stays below the pads' all-ones

// the directory as the receive path reads it: channel c < count is entry c, channel count + j is bare channel j; node_nann: index + 1 of the
// node's announcement in force, 0: none
struct store_nr_view {
  const u8 *store; size_t store_len; const u64 *rec_off; u32 n_rec;
  const u32 *ent_rec, *bare_rec, *chan_rank; u32 count, nbare;   // 3 records per entry (the announcement first); one per bare channel; 2 ranks per channel
  const u64 *node_off; const u32 *node_nann; u32 nodes;          // the image offsets of the ids, ascending by the ids
};
// the batch: message i = msgs[off[i], off[i + 1]); pending: the caller's pending or too-early channel_announcement maps are not empty
struct store_nr_batch { const u8 *msgs; const u64 *off; u32 n, pending; };
struct store_nr_msg { int32_t status; u32 node, ts; };

// ---- stage 0, every channel: a channel whose announcement record lacks DYING marks both of its nodes alive (alive: one byte per node, all 0)
LAMD_HD void store_nr_alive(const store_nr_view &v, u32 c, u8 *alive) {
  const u32 a = c < v.count ? v.ent_rec[3 * (size_t)c] : v.bare_rec[c - v.count];
  if (a < v.n_rec && v.rec_off[a] <= v.store_len && v.store_len - v.rec_off[a] >= STORE_HDR &&
      (store_read_hdr(v.store + v.rec_off[a]).flags & STORE_FLAG_DYING))
    return;
  for (u32 k = 0; k < 2; k++) {
    const u32 r = v.chan_rank[2 * (size_t)c + k];
    if (r < v.nodes) alive[r] = 1;
  }
}

// the address descriptors of a node_announcement (fromwire_wireaddr_array): type 1 -> 4 bytes, 2 -> 16, 3 -> 10, 4 -> 35, 5 -> a length byte and
// that many, each followed by a 2-byte port (0: ignored, no error); a descriptor cut off anywhere fails, an unknown type ends the walk
LAMD_HD bool store_nr_addrs_ok(const u8 *p, u32 len) {
  u32 pos = 0;
  while (pos < len) {
    const u32 t = p[pos++];
    u32 alen;
    if (t == 1) alen = 4;
    else if (t == 2) alen = 16;
    else if (t == 3) alen = 10;
    else if (t == 4) alen = 35;
    else if (t == 5) {
      if (pos >= len) return false;
      alen = p[pos++];
    } else return true;
    if (len - pos < alen + 2) return false;
    pos += alen + 2;
  }
  return true;
}

// ---- stage 1, every message: statuses -1 and 1 are final, everything else is PENDING and gets a signature row -- an unknown node too: the
// reference checks the signature before it looks the node up
LAMD_HD store_nr_msg store_nr_classify(const store_nr_view &v, const store_nr_batch &b, u32 i) {
  store_nr_msg r;
  r.status = STORE_NR_MALFORMED;
  r.node = STORE_NONE;
  r.ts = 0;
  const u64 len = b.off[i + 1] - b.off[i];
  const u8 *m = b.msgs + b.off[i];
  if (len < STORE_NR_MIN || len > STORE_NR_MAX || store_be16(m) != STORE_T_NANN) return r;
  const gossip_frame f = gossip_parse_frame(m, (size_t)len);
  if (f.bad || store_rx_ge_n(m + 2) || store_rx_ge_n(m + 34)) return r;
  // keyoff: node_id 33 | rgb_color 3 | alias 32 | addrlen u16 | addresses (inside the message: the frame is good)
  if (!store_nr_addrs_ok(m + f.keyoff + 70, store_be16(m + f.keyoff + 68))) { r.status = STORE_NR_BAD_ADDRESSES; return r; }
  r.ts = store_be32(m + f.keyoff - 4);
  r.node = store_dir_find_node(v.store, v.node_off, v.nodes, m + f.keyoff);
  r.status = STORE_NR_PENDING;
  return r;
}
// the row of a PENDING message: its span in the batch and the message it belongs to (the signer is the message's own id)
LAMD_HD void store_nr_row(const store_nr_batch &b, u32 i, u32 row, u64 *start, u64 *len, u32 *row_msg) {
  start[row] = b.off[i];
  len[row] = b.off[i + 1] - b.off[i];
  row_msg[row] = i;
}

// ---- stage 2, every message, behind the signature batch (sigv: 0 = the signature verifies): statuses 2 .. 4 are final and name no node; a
// candidate stays PENDING and returns its node's rank, everything else STORE_RX_PAD
LAMD_HD u64 store_nr_settle(int8_t *status, u32 *node, const u32 *row_of, const int8_t *sigv, u32 pending, u32 i) {
  if (status[i] != STORE_NR_PENDING) return STORE_RX_PAD;
  if (sigv[row_of[i]] != 0) {
    status[i] = STORE_NR_BAD_SIGNATURE;
    node[i] = STORE_NONE;
    return STORE_RX_PAD;
  }
  if (node[i] == STORE_NONE) {
    status[i] = (int8_t)(pending ? STORE_NR_HELD : STORE_NR_UNKNOWN);
    return STORE_RX_PAD;
  }
  return node[i];
}
// (the scan item of a sorted position is store_rx_item's)

// ---- stage 3, every sorted position.  s: the stable sort by rank (arrival order inside a rank) and the inclusive maximum of the items.  The
// row in front tells a row its node's maximum so far, or that it heads its node; the header of the image's record seeds the node.
// what stage 3 leaves per MESSAGE (all preset to 0 but del_key: all ones): count and size for the scans of the adds, the record the node held
struct store_nr_marks { u32 *acnt, *abytes, *del_key; };
// Returns whether the row deletes a record of the image.
LAMD_HD bool store_nr_resolve(const store_nr_view &v, const store_nr_batch &b, const store_rx_sorted &s, const u32 *ts, const u8 *alive, u32 p,
                              int8_t *status, u8 *flags, const store_nr_marks &k) {
  const u64 key = s.key[p];
  if (key == STORE_RX_PAD) return false;
  const u32 i = s.val[p], r = (u32)key;
  const u64 mine = (u64)ts[i] + 1, before = p ? s.run[p - 1] : 0;
  const u64 so_far = p && (before >> 33) == key ? before & STORE_RX_TS_MASK : 0;   // 0: the row heads its node
  u32 held = r < v.nodes ? v.node_nann[r] - 1 : STORE_NONE;                          // index + 1, 0: none
  if (!(held < v.n_rec && v.rec_off[held] <= v.store_len && v.store_len - v.rec_off[held] >= STORE_HDR)) held = STORE_NONE;
  const u64 seed = held != STORE_NONE ? (u64)store_read_hdr(v.store + v.rec_off[held]).ts + 1 : 0;
  const u64 in_force = so_far > seed ? so_far : seed;
  if (mine <= in_force) {
    status[i] = (int8_t)(mine == in_force ? STORE_NR_DUPLICATE : STORE_NR_STALE);
    return false;
  }
  status[i] = STORE_NR_ACCEPTED;
  u32 f = 0;
  // the node's last row carries its final maximum: a larger one than mine was accepted behind me
  const u32 end = store_sq_lower(s.key + p, s.n - p, key + 1) + p;
  if ((s.run[end - 1] & STORE_RX_TS_MASK) > mine) f |= STORE_RX_SUPERSEDED;
  if (!(r < v.nodes && alive[r])) f |= STORE_RX_DYING;
  flags[i] = (u8)f;
  k.acnt[i] = 1;
  k.abytes[i] = (u32)(STORE_HDR + (b.off[i + 1] - b.off[i]));
  // the first accepted row of a node deletes what the node held
  const bool deletes = held != STORE_NONE && so_far <= seed;
  if (deletes) k.del_key[i] = held;
  return deletes;
}

// ---- stage 4, every message: where its record goes.  apos / abyte: the exclusive scans of the marks
LAMD_HD void store_nr_plan(const int8_t *status, const u64 *apos, const u64 *abyte, u64 add_cap, u32 *add_msg, u64 *add_off, u32 i) {
  if (status[i] != STORE_NR_ACCEPTED || apos[i] >= add_cap) return;
  add_msg[apos[i]] = i;
  add_off[apos[i]] = abyte[i];
}

}  // namespace lamd

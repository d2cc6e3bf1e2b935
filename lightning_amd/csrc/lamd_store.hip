// liblightning_amd.so, the gossip_store calls: audit, repair, latest-wins repair, digest, channel-range replies, the comparison of peers' replies,
// the directory of an image and the answers to query_short_channel_ids, the stream index of an image and the answers to gossip_timestamp_filter,
// the reception of channel_update, node_announcement and channel_announcement batches against an image
#include "engine_internal.h"
#include "store_audit.h"
#include "store_repair.h"
#include "store_latest.h"
#include "store_digest.h"
#include "store_compare.h"
#include "store_query.h"
#include "store_stream.h"
#include "store_receive.h"
#include "store_nodes.h"
#include "store_announce.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_scan_by_key.hpp>
#include <memory>

// ---- gossip_store audit (lamd_gossip_store_audit; per-record logic in store_audit.h).  One lane per record throughout.
// The slicing tables of the CRC-32C in LDS, built by a block of 256 threads: thread t computes entry t of table 0 from the bitwise definition,
// every further table reads table 0 only.  Ends behind a barrier: every thread may read T.
template <int WAYS>
__device__ __forceinline__ void block_crc_tables(u32 *T) {
  const u32 t = threadIdx.x;
  u32 v = store_crc_t0(t);
  T[t] = v;
  __syncthreads();
  for (int k = 1; k < WAYS; k++) {
    v = (v >> 8) ^ T[v & 0xff];
    T[256 * k + t] = v;
  }
  __syncthreads();
}
// k_store_crc: the block builds the slicing tables in LDS (block_crc_tables), then each lane checksums its record -- bytes until the pointer
// is 4-aligned, 32-bit loads, tail bytes -- and classifies it.  A lane's cost is its record's length: gossip records are 130-450 bytes, the
// 65 535-byte maximum is correct, not fast.
template <int WAYS>
__global__ void __launch_bounds__(256) k_store_crc(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                   int8_t *__restrict__ pre) {
  __shared__ u32 T[WAYS * 256];
  block_crc_tables<WAYS>(T);
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) pre[i] = (int8_t)store_precheck_one<WAYS>(T, store, store_len, rec_off[i]);
}
// keys / vals: (1 << bits) + 1 slots, preset to all-ones bytes (STORE_EMPTY_KEY / STORE_NONE)
__global__ void __launch_bounds__(256) k_store_index(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                     u64 *keys, u32 *vals, u32 bits) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_index_one(store, store_len, rec_off[i], i, keys, vals, bits);
}
// sel[i] = the record's row in the signature selection (STORE_NONE: it has none): a channel_update's signer goes to ids33 + 33 * sel[i]
__global__ void __launch_bounds__(256) k_store_signers(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                       const u32 *__restrict__ sel, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                       u32 bits, u8 *__restrict__ ids33, u8 *__restrict__ aux) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u32 j = sel[i];
  aux[i] = (u8)store_signer_one(store, store_len, rec_off, i, keys, vals, bits, j != STORE_NONE ? ids33 + 33 * (size_t)j : nullptr);
}
__global__ void __launch_bounds__(256) k_store_verdict(u32 n, const int8_t *__restrict__ pre, const u32 *__restrict__ sel,
                                                       const int8_t *__restrict__ sigv, const u8 *__restrict__ aux, int8_t *__restrict__ verdict) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u32 j = sel[i];
  verdict[i] = (int8_t)store_merge_one(pre[i], j != STORE_NONE, j != STORE_NONE ? sigv[j] : 0, aux[i]);
}

// ---- gossip_store repair (lamd_gossip_store_repair; per-record and per-word logic in store_repair.h), behind k_store_verdict on the same stream.
// k_store_keep_chan: the live channel_announcements -- reason and size, and the two node ids of each kept one into the node table
// (nkeys / nvals: 1 << nbits slots, preset to all-ones bytes).  k_store_keep_rest: every other record (it reads the announcements' reasons,
// so it is a launch of its own); lane n writes the closing size 0, so that the scan ends with the sum.
__global__ void __launch_bounds__(256) k_store_keep_chan(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                         const int8_t *__restrict__ verdict, u64 *nkeys, u32 *nvals, u32 nbits, u8 *__restrict__ reason,
                                                         u32 *__restrict__ size) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !store_is_live_cann(store, store_len, rec_off[i])) return;
  u32 sz;
  u64 idoff = 0;
  const u32 r = store_keep_cann(store, store_len, rec_off, verdict, n, i, &sz, &idoff);
  reason[i] = (u8)r;
  size[i] = sz;
  if (r == STORE_DROP_KEPT) {
    store_node_insert(store, nkeys, nvals, nbits, idoff, i);
    store_node_insert(store, nkeys, nvals, nbits, idoff + 33, i);
  }
}
__global__ void __launch_bounds__(256) k_store_keep_rest(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                         const int8_t *__restrict__ verdict, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                         u32 bits, const u64 *__restrict__ nkeys, const u32 *__restrict__ nvals, u32 nbits, u8 *reason,
                                                         u32 *__restrict__ size) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) { size[n] = 0; return; }
  if (store_is_live_cann(store, store_len, rec_off[i])) return;
  u32 sz;
  reason[i] = (u8)store_keep_other(store, store_len, rec_off, verdict, n, i, keys, vals, bits, nkeys, nvals, nbits, reason, &sz);
  size[i] = sz;
}
// ---- the keep stages of the latest-wins repair (lamd_gossip_store_repair_latest; per-record logic in store_latest.h) in place of the two
// kernels above.  Each reads what the one before it wrote with atomics (update slots and dying marks -> announcements and node table ->
// node slots -> the rest), so each is a launch of its own: no workgroup waits for another.  latest: 2 * n slots, nlatest: 1 << nbits slots,
// dying: n bytes, all preset to 0; nkeys / nvals as above.  Lane n of k_store_latest_rest writes the closing size 0.
__global__ void __launch_bounds__(256) k_store_latest_upd(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                          const int8_t *__restrict__ verdict, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                          u32 bits, lamd_store_latest_policy pol, u64 *latest, u8 *dying) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_latest_upd_one(store, store_len, rec_off, verdict, i, keys, vals, bits, pol, latest, dying);
}
__global__ void __launch_bounds__(256) k_store_latest_chan(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                           const int8_t *__restrict__ verdict, lamd_store_latest_policy pol,
                                                           const u64 *__restrict__ latest, const u8 *__restrict__ dying, u64 *nkeys, u32 *nvals,
                                                           u32 nbits, u8 *__restrict__ reason, u32 *__restrict__ size) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !store_is_live_cann(store, store_len, rec_off[i])) return;
  u32 sz;
  u64 idoff = 0;
  const u32 r = store_latest_cann_one(store, store_len, rec_off, verdict, n, i, pol, latest, dying, &sz, &idoff);
  reason[i] = (u8)r;
  size[i] = sz;
  if (r == STORE_DROP_KEPT) {
    store_node_insert(store, nkeys, nvals, nbits, idoff, i);
    store_node_insert(store, nkeys, nvals, nbits, idoff + 33, i);
  }
}
__global__ void __launch_bounds__(256) k_store_latest_node(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                           const int8_t *__restrict__ verdict, const u64 *__restrict__ nkeys,
                                                           const u32 *__restrict__ nvals, u32 nbits, lamd_store_latest_policy pol, u64 *nlatest) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_latest_node_one(store, store_len, rec_off, verdict, i, nkeys, nvals, nbits, pol, nlatest);
}
__global__ void __launch_bounds__(256) k_store_latest_rest(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                           const int8_t *__restrict__ verdict, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                           u32 bits, const u64 *__restrict__ nkeys, const u32 *__restrict__ nvals, u32 nbits,
                                                           lamd_store_latest_policy pol, const u64 *__restrict__ latest,
                                                           const u64 *__restrict__ nlatest, u8 *reason, u32 *__restrict__ size) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) { size[n] = 0; return; }
  if (store_is_live_cann(store, store_len, rec_off[i])) return;
  u32 sz;
  reason[i] = (u8)store_latest_other_one(store, store_len, rec_off, verdict, n, i, keys, vals, bits, nkeys, nvals, nbits, reason, pol, latest, nlatest, &sz);
  size[i] = sz;
}
// The exclusive scan of the sizes, 64-bit, in tiles of STORE_SCAN_TILE = one block: k_store_scan_reduce leaves one sum per tile, the sums are
// scanned the same way (level by level until one tile holds them), k_store_scan_apply scans inside each tile and adds the tile's base.
// Separate launches, no workgroup waits for another.  With new_off (the record level) it also writes the records' offsets in the output.
template <class In>
__global__ void __launch_bounds__(256) k_store_scan_reduce(u64 n, const In *__restrict__ in, u64 *__restrict__ sums) {
  __shared__ u64 w[4];
  const u32 t = threadIdx.x;
  const u64 i = (u64)blockIdx.x * STORE_SCAN_TILE + t;
  u64 v = i < n ? (u64)in[i] : 0;
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  if ((t & 63) == 0) w[t >> 6] = v;
  __syncthreads();
  if (t == 0) sums[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}
template <class In>
__global__ void __launch_bounds__(256) k_store_scan_apply(u64 n, const In *in, const u64 *__restrict__ base, u64 *out, u64 n_rec,
                                                          const u8 *__restrict__ reason, u64 *__restrict__ new_off) {
  __shared__ u64 s[STORE_SCAN_TILE];
  const u32 t = threadIdx.x;
  const u64 i = (u64)blockIdx.x * STORE_SCAN_TILE + t;
  const u64 v = i < n ? (u64)in[i] : 0;
  s[t] = v;
  __syncthreads();
  for (u32 d = 1; d < STORE_SCAN_TILE; d <<= 1) {
    const u64 a = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  if (i >= n) return;
  const u64 x = s[t] - v + (base ? base[blockIdx.x] : 0);
  out[i] = x;
  if (new_off && i < n_rec) new_off[i] = reason[i] == STORE_DROP_KEPT ? STORE_REPAIR_HEAD + x : ~(u64)0;
}
// k_store_pack: one aligned 32-bit word of the OUTPUT per lane and step, 256 consecutive words per block and step: the stores of a wave
// are 256 contiguous bytes whatever the records' lengths and alignments, and a lane's time does not depend on any record's length.  A
// block owns STORE_PACK_WORDS consecutive words; lanes 0 and 1 find the records of its first and last payload byte in the whole scan, the
// block stages that window of the scan and of the record offsets in LDS and every lane searches there (a window of more than
// STORE_PACK_STAGE records -- a long run of dropped ones inside the block's bytes -- is searched in global memory instead).  The grid is
// sized by the upper bound len + 46: blocks behind the output's end leave at once.
constexpr u32 STORE_PACK_WORDS = 2048;
__global__ void __launch_bounds__(256) k_store_pack(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                    const u64 *__restrict__ pos, store_head head, u8 *__restrict__ out, u64 out_cap) {
  __shared__ u32 range[2];
  __shared__ u32 rel[STORE_PACK_STAGE + 1];
  __shared__ u64 roff[STORE_PACK_STAGE];
  const u32 t = threadIdx.x, mis = (u32)((uintptr_t)out & 3);
  const u64 total = STORE_REPAIR_HEAD + pos[n], lim = out_cap < total ? out_cap : total;
  const u64 k0 = (u64)blockIdx.x * STORE_PACK_WORDS, k1 = k0 + STORE_PACK_WORDS;
  if (4 * k0 >= lim + mis) return;
  if (t < 2) {
    const u64 bf = 4 * k0 > mis ? 4 * k0 - mis : 0, bl = 4 * k1 - mis < lim ? 4 * k1 - mis : lim;   // the block's bytes: [bf, bl)
    u32 r = 0;
    if (bl > STORE_REPAIR_HEAD)
      r = store_pack_locate(store_pack_global{rec_off, pos}, 0, n - 1, t ? bl - STORE_REPAIR_HEAD - 1 : (bf > STORE_REPAIR_HEAD ? bf - STORE_REPAIR_HEAD : 0));
    range[t] = r;
  }
  __syncthreads();
  const u32 lo = range[0], hi = range[1];
  if (hi - lo < STORE_PACK_STAGE) {
    const u64 base = pos[lo];
    for (u32 j = t; j <= hi - lo + 1; j += 256) rel[j] = (u32)(pos[lo + j] - base);
    for (u32 j = t; j <= hi - lo; j += 256) roff[j] = rec_off[lo + j];
    __syncthreads();
    const store_pack_staged v{roff, rel, lo, base};
    for (u64 k = k0 + t; k < k1; k += 256) store_pack_word(store, store_len, v, lo, hi, head, out, lim, mis, k);
  } else {
    const store_pack_global v{rec_off, pos};
    for (u64 k = k0 + t; k < k1; k += 256) store_pack_word(store, store_len, v, lo, hi, head, out, lim, mis, k);
  }
}

// ---- gossip_store digest (lamd_gossip_store_digest_build; per-record and per-entry logic in store_digest.h).  One lane per record; each
// stage reads what the one before wrote with atomics, so each is a launch of its own.  cnt: DIGEST_CNT_* counters, all 0; a wave adds
// its count with one atomic.  keys / vals: (1 << bits) + 1 slots preset to all-ones bytes; slot: 2 * n words preset to 0.
enum { DIGEST_CNT_ENTRIES = 0, DIGEST_CNT_CHANNELS = 1, DIGEST_CNT_NO_UPDATE = 2, DIGEST_CNT_NO_CHANNEL = 3, DIGEST_CNT_IN_FRONT = 4, DIGEST_CNT_SHORT = 5, DIGEST_CNTS = 8 };
__device__ __forceinline__ void wave_count(u32 *counter, bool pred) {
  const u64 mask = __ballot(pred);
  if ((threadIdx.x & 63u) == 0 && mask) atomicAdd(counter, (u32)__popcll(mask));
}
__global__ void __launch_bounds__(256) k_digest_index(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                      const int8_t *__restrict__ verdict, u64 *keys, u32 *vals, u32 bits) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_digest_index_one(store, store_len, rec_off, verdict, i, keys, vals, bits);
}
__global__ void __launch_bounds__(256) k_digest_slots(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                      const int8_t *__restrict__ verdict, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                      u32 bits, u32 *slot, u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  const u32 r = i < n ? store_digest_slot_one(store, store_len, rec_off, verdict, i, keys, vals, bits, slot) : (u32)STORE_DIGEST_UPD_NONE;
  wave_count(&cnt[DIGEST_CNT_NO_CHANNEL], r == STORE_DIGEST_UPD_NO_CHANNEL);
  wave_count(&cnt[DIGEST_CNT_IN_FRONT], r == STORE_DIGEST_UPD_IN_FRONT);
  wave_count(&cnt[DIGEST_CNT_SHORT], r == STORE_DIGEST_UPD_SHORT);
}
// the channels with an update, compacted in any order as (scid, announcement index) pairs: pair_key / pair_val hold n pairs preset to
// all-ones bytes, so that behind the cnt[DIGEST_CNT_ENTRIES] real pairs the largest key stands -- a stable sort of all n pairs leaves the
// real ones in front, the scid of that value included.  The channels without an update: their scids alone, compacted the same way into bare_key
// (n keys preset to all-ones bytes; cnt[DIGEST_CNT_NO_UPDATE] is their allocator and so their count).
__global__ void __launch_bounds__(256) k_digest_chan(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                     const int8_t *__restrict__ verdict, const u64 *__restrict__ keys, const u32 *__restrict__ vals,
                                                     u32 bits, const u32 *__restrict__ slot, u64 *__restrict__ pair_key, u32 *__restrict__ pair_val, u64 *__restrict__ bare_key,
                                                     u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  u64 scid = 0;
  const u32 c = i < n ? store_digest_chan_one(store, store_len, rec_off, verdict, i, keys, vals, bits, slot, &scid) : 0u;
  const u32 e = wave_alloc(&cnt[DIGEST_CNT_ENTRIES], c == 1, 0, nullptr);
  if (c == 1 && e < n) {
    pair_key[e] = scid;
    pair_val[e] = i;
  }
  const u32 b = wave_alloc(&cnt[DIGEST_CNT_NO_UPDATE], c == 2, 0, nullptr);
  if (c == 2 && b < n) bare_key[b] = scid;
  wave_count(&cnt[DIGEST_CNT_CHANNELS], c != 0);
}
// entry j of the sorted digest, j < cnt[DIGEST_CNT_ENTRIES] (the grid covers n): ann[j] = its announcement.  The CRC tables as in k_store_crc.
__global__ void __launch_bounds__(256) k_digest_entries(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                        const u32 *__restrict__ slot, const u32 *__restrict__ ann, const u32 *__restrict__ cnt,
                                                        u32 *__restrict__ ts, u32 *__restrict__ csum, u32 *__restrict__ rec) {
  __shared__ u32 T[4 * 256];
  block_crc_tables<4>(T);
  const u32 j = blockIdx.x * 256 + threadIdx.x, count = cnt[DIGEST_CNT_ENTRIES] < n ? cnt[DIGEST_CNT_ENTRIES] : n;
  if (j >= count) return;
  const u32 a = ann[j];
  if (a >= n) return;   // (never: the first `count` pairs are real)
  store_digest_entry_one<4>(T, store, store_len, rec_off, a, slot, ts + 2 * (size_t)j, csum + 2 * (size_t)j, rec + 3 * (size_t)j);
}

// ---- query_channel_range answers (lamd_channel_range_reply_batch; per-query and per-word logic in store_digest.h).
// k_range_count: one lane per query runs the searches and the split and leaves the number of its replies and of their bytes.
__global__ void __launch_bounds__(256) k_range_count(u32 nq, const store_range_query *__restrict__ queries, const u64 *__restrict__ scid, u32 count,
                                                     u32 *__restrict__ n_msgs, u64 *__restrict__ n_bytes) {
  const u32 q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const store_range_total t = store_range_plan(queries[q], q, scid, count, nullptr, 0);
  n_msgs[q] = t.msgs;
  n_bytes[q] = t.bytes;
}
// k_range_scan: ONE block; the exclusive scans of both arrays, tile by tile with a carry: msg_first[nq + 1], byte_first[nq + 1]
__global__ void __launch_bounds__(256) k_range_scan(u32 nq, const u32 *__restrict__ n_msgs, const u64 *__restrict__ n_bytes, u64 *__restrict__ msg_first,
                                                    u64 *__restrict__ byte_first) {
  __shared__ u64 sm[256], sb[256];
  const u32 t = threadIdx.x;
  u64 cm = 0, cb = 0;
  for (u32 base = 0; base <= nq; base += 256) {
    const u32 q = base + t;
    const u64 vm = q < nq ? (u64)n_msgs[q] : 0, vb = q < nq ? n_bytes[q] : 0;
    sm[t] = vm;
    sb[t] = vb;
    __syncthreads();
    for (u32 d = 1; d < 256; d <<= 1) {
      const u64 am = t >= d ? sm[t - d] : 0, ab = t >= d ? sb[t - d] : 0;
      __syncthreads();
      sm[t] += am;
      sb[t] += ab;
      __syncthreads();
    }
    if (q <= nq) {
      msg_first[q] = cm + sm[t] - vm;
      byte_first[q] = cb + sb[t] - vb;
    }
    cm += sm[255];
    cb += sb[255];
    __syncthreads();
  }
}
// k_range_plan: the split again, now writing: the replies of query q are msgs[msg_first[q] ..], as far as they lie below msg_cap, and
// msg_off[j] their offsets in the output; the last query's lane closes msg_off with the total
__global__ void __launch_bounds__(256) k_range_plan(u32 nq, const store_range_query *__restrict__ queries, const u64 *__restrict__ scid, u32 count,
                                                    const u64 *__restrict__ msg_first, const u64 *__restrict__ byte_first, u64 msg_cap,
                                                    store_range_msg *__restrict__ msgs, u64 *__restrict__ msg_off) {
  const u32 q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const u64 j0 = msg_first[q];
  if (q == nq - 1 && msg_first[nq] <= msg_cap) msg_off[msg_first[nq]] = byte_first[nq];
  if (j0 >= msg_cap) return;
  const u64 room = msg_cap - j0;
  const store_range_query qu = queries[q];
  const store_range_total t = store_range_plan(qu, q, scid, count, msgs + j0, room < 0xFFFFFFFFull ? (u32)room : 0xFFFFFFFFu);
  u64 off = byte_first[q];
  for (u32 k = 0; k < t.msgs && k < room; k++) {
    msg_off[j0 + k] = off;
    off += store_range_msg_bytes(qu, msgs[j0 + k].n);
  }
}
// k_range_encode: one aligned 32-bit word of the output per lane
__global__ void __launch_bounds__(256) k_range_encode(u64 words, const store_range_msg *__restrict__ msgs, const u64 *__restrict__ msg_off, u32 n_msgs,
                                                      const store_range_query *__restrict__ queries, store_digest_view d, u8 *__restrict__ out, u64 total) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k < words) store_range_word(msgs, msg_off, n_msgs, queries, d, out, total, (u32)((uintptr_t)out & 3), k);
}

// ---- gossip_store audit
static void store_count_verdicts(const int8_t *v, size_t n, lamd_store_summary *s) {
  for (size_t i = 0; i < n; i++) {
    switch (v[i]) {
      case LAMD_STORE_OK: s->ok++; break;
      case LAMD_STORE_SKIPPED_DELETED: s->skipped_deleted++; break;
      case LAMD_STORE_BAD_CHECKSUM: s->bad_checksum++; break;
      case LAMD_STORE_UNKNOWN_TYPE: s->unknown_type++; break;
      case LAMD_STORE_MALFORMED: s->malformed++; break;
      case LAMD_STORE_REDUNDANT: s->redundant++; break;
      case LAMD_STORE_NO_CHANNEL: s->no_channel++; break;
      default:
        if (v[i] >= 1 && v[i] <= 4) s->bad_signature[v[i] - 1]++;
    }
  }
  s->clean = s->end_reason == LAMD_STORE_END_EOF && s->ok + s->skipped_deleted == n;
}
extern "C" int lamd_gossip_store_frame(const uint8_t *store, size_t len, size_t cap, uint64_t *rec_off, size_t *n_records,
                                       lamd_store_summary *summary) {
  if (!store || !n_records || !summary || (cap && !rec_off)) return LAMD_ERR_ARG;
  *n_records = 0;
  if (!store_walk(store, len, summary, [&](size_t i, u64 off, const store_hdr &, u32) {
        if (i < cap) rec_off[i] = off;
      }))
    return LAMD_ERR_ARG;
  *n_records = (size_t)summary->records;
  return summary->records > cap ? LAMD_ERR_ARG : LAMD_OK;
}
// Everything between the host walk and the final copy is queued on one lane's stream: image (unless resident) and the walk's arrays up,
// four kernels and the signature batch, the verdict bytes down.  store_job: what the queued stages leave on the device for the caller --
// lamd_gossip_store_audit copies the verdicts down, lamd_gossip_store_repair queues its own stages behind them first.
struct store_job {
  lamd_ctx *L = nullptr;      // the lane; nullptr: nothing is queued (no record, or an error before the first copy)
  size_t n = 0, n_cann = 0;   // records; live channel_announcements
  const u8 *img = nullptr;    // the image on the device
  const u64 *d_recoff = nullptr;
  const u64 *d_keys = nullptr;
  const u32 *d_vals = nullptr;
  u32 bits = 0;               // the scid index
  const int8_t *d_verdict = nullptr;
  std::vector<u64> pack;      // the queued copy reads it: lives until the stream has been synchronised
};
static int store_audit_queue(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t cap, uint64_t *rec_off, size_t *n_records,
                             lamd_store_summary *summary, store_job *job) {
  *n_records = 0;
  // the walk: record offsets, and the selection of the signature batch -- the live 256 / 257 / 258 records (4 rows / 1 / 1)
  std::vector<u64> start, mlen, rowbase;
  std::vector<u32> sel;
  size_t n_cann = 0;
  u64 rows = 0;
  if (!store_walk(store, len, summary, [&](size_t i, u64 off, const store_hdr &h, u32 type) {
        if (i < cap) rec_off[i] = off;
        const bool sig = type == STORE_T_CANN || type == STORE_T_NANN || type == STORE_T_CUPD;
        sel.push_back(sig ? (u32)start.size() : STORE_NONE);
        if (!sig) return;
        start.push_back(off + STORE_HDR);
        mlen.push_back(h.len);
        rowbase.push_back(rows);
        rows += type == STORE_T_CANN ? 4 : 1;
        n_cann += type == STORE_T_CANN;
      })) {
    ctx->err = "not a gossip_store of major version 0";
    return LAMD_ERR_ARG;
  }
  const size_t n = (size_t)summary->records, nsel = start.size();
  *n_records = n;
  if (n > cap) { ctx->err = "gossip_store audit: rec_off / verdict too small"; return LAMD_ERR_ARG; }
  if (n >= (size_t)STORE_NONE || rows >= (u64)STORE_NONE) { ctx->err = "gossip_store audit: too many records"; return LAMD_ERR_ARG; }
  summary->signatures = rows;
  if (n == 0) return LAMD_OK;
  rowbase.push_back(rows);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  lamd_ctx *L;
  int rc = pick_lane(ctx, &L);
  if (rc != LAMD_OK) return rc;
  u32 bits = 1;
  while (((size_t)1 << bits) < 2 * n_cann) bits++;
  const size_t slots = ((size_t)1 << bits) + 1;
  // host arrays, one copy: rec_off u64[n] | start u64[nsel] | len u64[nsel] | rowbase u64[nsel + 1] | sel u32[n]
  std::vector<u64> &pack = job->pack;   // queued copies read it: every error return behind this line drains the stream (drain_fail)
  pack.assign(n + 3 * nsel + 1 + (n + 1) / 2, 0);
  for (size_t i = 0; i < n; i++) pack[i] = rec_off[i];
  if (nsel) {
    memcpy(&pack[n], start.data(), 8 * nsel);
    memcpy(&pack[n + nsel], mlen.data(), 8 * nsel);
  }
  memcpy(&pack[n + 2 * nsel], rowbase.data(), 8 * (nsel + 1));
  memcpy(&pack[n + 3 * nsel + 1], sel.data(), 4 * n);
  if ((rc = ensure(L, &L->store.host, pack.size() * 8)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if ((rc = ensure(L, &L->store.ids, nsel * 33 + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if ((rc = ensure(L, &L->store.tab, slots * 12)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if ((rc = ensure(L, &L->store.out, 3 * n + nsel + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (!d_store && (rc = ensure(L, &L->store.img, len + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  const bool timed = ctx->timing;
  if (timed) STCHK(L->store.t_audit.create());
  hipStream_t st = L->stream;
  const u64 *d_pack = L->store.host.as<const u64>();
  const u64 *d_recoff = d_pack, *d_start = d_pack + n, *d_len = d_start + nsel, *d_rowbase = d_len + nsel;
  const u32 *d_sel = (const u32 *)(d_rowbase + nsel + 1);
  u64 *d_keys = L->store.tab.as<u64>();
  u32 *d_vals = (u32 *)(d_keys + slots);
  int8_t *d_pre = L->store.out.as<int8_t>(), *d_verdict = d_pre + n, *d_sigv = d_verdict + n;
  u8 *d_aux = (u8 *)(d_sigv + nsel);
  const u8 *img = (const u8 *)d_store;
  if (!d_store) {
    STCHK(hipMemcpyAsync(L->store.img.p, store, len, hipMemcpyHostToDevice, st));
    img = L->store.img.as<const u8>();
  }
  STCHK(hipMemcpyAsync(L->store.host.p, pack.data(), pack.size() * 8, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(L->store.tab.p, 0xFF, slots * 12, st));
  // slicing by 8 measured faster (0.24 ms against 0.42 ms on 750 000 records, profiles/store_audit.txt): LAMD_STORE_CRC_WAYS=8 selects it.  The
  // default stays the variant the GPU tests have run with until they have run with the other one.
  static const int crc_ways = [] { const char *e = getenv("LAMD_STORE_CRC_WAYS"); return e && atoi(e) == 8 ? 8 : 4; }();
  const dim3 grid(blocks_for(n)), block(256);
  if (timed) STCHK(L->store.t_audit.record(0, st));
  if (crc_ways == 8) hipLaunchKernelGGL(k_store_crc<8>, grid, block, 0, st, (u32)n, img, len, d_recoff, d_pre);
  else hipLaunchKernelGGL(k_store_crc<4>, grid, block, 0, st, (u32)n, img, len, d_recoff, d_pre);
  if (timed) STCHK(L->store.t_audit.record(1, st));
  hipLaunchKernelGGL(k_store_index, grid, block, 0, st, (u32)n, img, len, d_recoff, d_keys, d_vals, bits);
  if (timed) STCHK(L->store.t_audit.record(2, st));
  hipLaunchKernelGGL(k_store_signers, grid, block, 0, st, (u32)n, img, len, d_recoff, d_sel, (const u64 *)d_keys, (const u32 *)d_vals, bits,
                     L->store.ids.as<u8>(), d_aux);
  STCHK(hipGetLastError());
  if (timed) STCHK(L->store.t_audit.record(3, st));
  if (nsel && (rc = gossip_device(L, nsel, img, d_start, L->store.ids.as<const u8>(), d_rowbase, (size_t)rows, d_sigv, d_len)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (timed) STCHK(L->store.t_audit.record(4, st));
  hipLaunchKernelGGL(k_store_verdict, grid, block, 0, st, (u32)n, (const int8_t *)d_pre, d_sel, (const int8_t *)d_sigv, (const u8 *)d_aux, d_verdict);
  STCHK(hipGetLastError());
  if (timed) STCHK(L->store.t_audit.record(5, st));
  job->L = L;
  job->n = n;
  job->n_cann = n_cann;
  job->img = img;
  job->d_recoff = d_recoff;
  job->d_keys = d_keys;
  job->d_vals = d_vals;
  job->bits = bits;
  job->d_verdict = d_verdict;
  return LAMD_OK;
}
// behind the synchronisation that ends a timed audit: the stage times
static int store_audit_times(lamd_ctx *ctx, lamd_ctx *L, lamd_store_summary *summary) {
  HIPCHK(ctx, L->store.t_audit.read(5, summary->stage_ms));
  return LAMD_OK;
}
extern "C" int lamd_gossip_store_audit(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t cap, uint64_t *rec_off,
                                       int8_t *verdict, size_t *n_records, lamd_store_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!store || !n_records || !summary || (cap && (!rec_off || !verdict))) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  store_job job;
  int rc = store_audit_queue(ctx, store, len, d_store, cap, rec_off, n_records, summary, &job);
  if (rc != LAMD_OK) return rc;
  lamd_ctx *L = job.L;
  if (!L) { store_count_verdicts(verdict, 0, summary); return LAMD_OK; }
  STCHK(hipMemcpyAsync(verdict, job.d_verdict, job.n, hipMemcpyDeviceToHost, L->stream));
  STCHK(hipStreamSynchronize(L->stream));
  if (ctx->timing && (rc = store_audit_times(ctx, L, summary)) != LAMD_OK) return rc;
  store_count_verdicts(verdict, job.n, summary);
  return LAMD_OK;
}

// ---- gossip_store repair: the audit's stages, then keep flags, scan and copy on the same stream.  ONE wait more than the audit: the
// verdicts, reasons, offsets and the output's length come down first (the length decides how much of the image follows).
// lamd_gossip_store_repair and lamd_gossip_store_repair_latest differ in their keep stages alone: what lies in front of them
// (store_rep_plan, store_repair_empty) and behind them (store_repair_finish) is one piece of code.
struct store_rep_plan {
  std::vector<size_t> cnt;   // the scan's levels: cnt[0] = n + 1 sizes (the last one 0), cnt[k + 1] = the tiles of level k, until one tile holds a level
  size_t n_sums = 0, nslots = 0, upper = 0;   // all tiles' sums; slots of the node table; no output is longer than `upper`
  u32 nbits = 1;
  store_rep_plan() = default;
  store_rep_plan(size_t n, size_t n_cann, size_t len) : cnt{n + 1} {
    while (cnt.back() > STORE_SCAN_TILE) cnt.push_back((cnt.back() + STORE_SCAN_TILE - 1) / STORE_SCAN_TILE);
    for (size_t k = 1; k < cnt.size(); k++) n_sums += cnt[k];
    while (((size_t)1 << nbits) < 4 * n_cann) nbits++;
    nslots = (size_t)1 << nbits;
    upper = len + STORE_REPAIR_HEAD - 1;
  }
};
struct store_rep_dev {   // where the keep stages left their results, and where the output goes
  u64 *pos, *newoff, *sums;
  u32 *size;
  u8 *reason, *img_out;
  size_t dev_cap;
};
// a store without any record: the version byte and the uuid record
static int store_repair_empty(lamd_ctx *ctx, const store_head &head, int8_t *verdict, lamd_store_summary *summary, uint8_t *out, void *d_out, size_t out_cap,
                              uint64_t *out_len) {
  store_count_verdicts(verdict, 0, summary);
  *out_len = STORE_REPAIR_HEAD;
  if ((out || d_out) && out_cap < STORE_REPAIR_HEAD) { ctx->err = "gossip_store repair: output buffer too small"; return LAMD_ERR_ARG; }
  if (out) memcpy(out, head.b, STORE_REPAIR_HEAD);
  if (d_out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpy(d_out, head.b, STORE_REPAIR_HEAD, hipMemcpyHostToDevice));
  }
  return LAMD_OK;
}
// Behind the keep stages (slot 0 of t_rep was recorded in front of them): the scan, the copy, the two waits.  counts[r] = records with reason r;
// stage_ms: keep, scan, copy.  *out_len and the counts are set before the output's size is checked against out_cap.
static int store_repair_finish(lamd_ctx *ctx, const store_job &job, size_t len, const store_rep_plan &plan, const store_rep_dev &d, const store_head &head,
                               int8_t *verdict, uint64_t *new_off, uint8_t *reason, uint8_t *out, bool want_out, size_t out_cap,
                               lamd_store_summary *summary, uint64_t counts[8], uint64_t *out_len, double stage_ms[3]) {
  lamd_ctx *L = job.L;
  const size_t n = job.n;
  const std::vector<size_t> &cnt = plan.cnt;
  const bool timed = ctx->timing;
  hipStream_t st = L->stream;
  int rc;
  STCHK(hipGetLastError());
  if (timed) STCHK(L->store.t_rep.record(1, st));
  {
    std::vector<u64 *> lvl{d.pos};   // level k >= 1 lives in d.sums and is scanned in place
    for (size_t k = 1, o = 0; k < cnt.size(); o += cnt[k], k++) lvl.push_back(d.sums + o);
    const size_t top = cnt.size() - 1;
    for (size_t k = 0; k < top; k++) {
      if (k == 0) hipLaunchKernelGGL(k_store_scan_reduce<u32>, dim3((unsigned)cnt[1]), dim3(256), 0, st, (u64)cnt[0], (const u32 *)d.size, lvl[1]);
      else hipLaunchKernelGGL(k_store_scan_reduce<u64>, dim3((unsigned)cnt[k + 1]), dim3(256), 0, st, (u64)cnt[k], (const u64 *)lvl[k], lvl[k + 1]);
    }
    for (size_t k = top + 1; k-- > 0;) {
      const u64 *base = k == top ? nullptr : lvl[k + 1];
      const dim3 grid((unsigned)((cnt[k] + STORE_SCAN_TILE - 1) / STORE_SCAN_TILE));
      if (k == 0) hipLaunchKernelGGL(k_store_scan_apply<u32>, grid, dim3(256), 0, st, (u64)cnt[0], (const u32 *)d.size, base, d.pos, (u64)n, (const u8 *)d.reason, d.newoff);
      else hipLaunchKernelGGL(k_store_scan_apply<u64>, grid, dim3(256), 0, st, (u64)cnt[k], (const u64 *)lvl[k], base, lvl[k], (u64)0, (const u8 *)nullptr, (u64 *)nullptr);
    }
  }
  STCHK(hipGetLastError());
  if (timed) STCHK(L->store.t_rep.record(2, st));
  if (want_out && d.dev_cap) {
    const size_t words = (3 + (plan.upper < d.dev_cap ? plan.upper : d.dev_cap)) / 4 + 1;
    hipLaunchKernelGGL(k_store_pack, dim3((unsigned)((words + STORE_PACK_WORDS - 1) / STORE_PACK_WORDS)), dim3(256), 0, st, (u32)n, job.img, len, job.d_recoff,
                       (const u64 *)d.pos, head, d.img_out, (u64)d.dev_cap);
    STCHK(hipGetLastError());
  }
  if (timed) STCHK(L->store.t_rep.record(3, st));
  u64 payload = 0;
  STCHK(hipMemcpyAsync(verdict, job.d_verdict, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(reason, d.reason, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(new_off, d.newoff, 8 * n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&payload, d.pos + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  if (timed) {
    if ((rc = store_audit_times(ctx, L, summary)) != LAMD_OK) return rc;
    STCHK(L->store.t_rep.read(3, stage_ms));
  }
  store_count_verdicts(verdict, n, summary);
  for (size_t i = 0; i < n; i++) counts[reason[i] & 7]++;
  *out_len = STORE_REPAIR_HEAD + payload;
  if (want_out && *out_len > out_cap) { ctx->err = "gossip_store repair: output buffer too small"; return LAMD_ERR_ARG; }
  if (out) {
    STCHK(hipMemcpyAsync(out, d.img_out, *out_len, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));
  }
  return LAMD_OK;
}
// What both repairs do in front of their keep stages: the arguments they share, the audit's queue, the head, the scan's plan, the workspace of
// ws_bytes(n, n_sums, nslots) bytes, the output image and the events.  f->job.L == nullptr behind LAMD_OK: a store without records, the call is complete.
struct store_rep_frame {
  store_job job;   // (a queued copy reads its vector: the frame lives until the call returns)
  store_head head;
  store_rep_plan plan;
  bool want_out = false;
  u8 *img_out = nullptr;   // where the output goes on the device, dev_cap bytes of room
  size_t dev_cap = 0;
};
template <class Summary>   // the reasons both repairs know
static void store_repair_counts(Summary *s, const uint64_t counts[8]) {
  s->kept = counts[STORE_DROP_KEPT];
  s->dropped_deleted = counts[STORE_DROP_DELETED];
  s->dropped_verdict = counts[STORE_DROP_VERDICT];
  s->dropped_dependency = counts[STORE_DROP_DEPENDENCY];
  s->dropped_bookkeeping = counts[STORE_DROP_BOOKKEEPING];
}
static bool store_repair_args_ok(const uint8_t *store, const uint8_t *uuid32, size_t cap, const uint64_t *rec_off, const int8_t *verdict, const uint64_t *new_off,
                                 const uint8_t *reason, const size_t *n_records, const lamd_store_summary *summary) {
  return store && uuid32 && n_records && summary && !(cap && (!rec_off || !verdict || !new_off || !reason));
}
static int store_repair_begin(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, const uint8_t *uuid32, size_t cap, uint64_t *rec_off,
                              int8_t *verdict, size_t *n_records, uint8_t *out, void *d_out, size_t out_cap, lamd_store_summary *summary, uint64_t *out_len,
                              size_t (*ws_bytes)(size_t n, size_t n_sums, size_t nslots), store_rep_frame *f) {
  int rc = store_audit_queue(ctx, store, len, d_store, cap, rec_off, n_records, summary, &f->job);
  if (rc != LAMD_OK) return rc;
  f->head = store_make_head(store[0], uuid32);
  f->want_out = out || d_out;
  lamd_ctx *L = f->job.L;
  if (!L) return store_repair_empty(ctx, f->head, verdict, summary, out, d_out, out_cap, out_len);
  f->plan = store_rep_plan(f->job.n, f->job.n_cann, len);
  if ((rc = ensure(L, &L->store.rep, ws_bytes(f->job.n, f->plan.n_sums, f->plan.nslots))) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (f->want_out && !d_out && (rc = ensure(L, &L->store.pack, f->plan.upper + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  f->img_out = d_out ? (u8 *)d_out : L->store.pack.as<u8>();
  f->dev_cap = d_out ? out_cap : f->plan.upper;
  if (ctx->timing) STCHK(L->store.t_rep.create());
  return LAMD_OK;
}
extern "C" int lamd_gossip_store_repair(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, const uint8_t *uuid32, size_t cap,
                                        uint64_t *rec_off, int8_t *verdict, uint64_t *new_off, uint8_t *reason, size_t *n_records, uint8_t *out,
                                        void *d_out, size_t out_cap, lamd_store_summary *summary, lamd_store_repair_summary *repair) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!repair || !store_repair_args_ok(store, uuid32, cap, rec_off, verdict, new_off, reason, n_records, summary)) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *repair = lamd_store_repair_summary();
  store_rep_frame f;
  // pos u64[n + 1] | new_off u64[n] | sums u64[n_sums] | nkeys u64[nslots] | nvals u32[nslots] | size u32[n + 1] | reason u8[n]
  int rc = store_repair_begin(ctx, store, len, d_store, uuid32, cap, rec_off, verdict, n_records, out, d_out, out_cap, summary, &repair->out_len,
                              [](size_t n, size_t n_sums, size_t nslots) { return 8 * (2 * n + 1 + n_sums + nslots) + 4 * (nslots + n + 1) + n + 16; }, &f);
  lamd_ctx *L = f.job.L;
  if (rc != LAMD_OK || !L) return rc;
  const store_job &job = f.job;
  const store_rep_plan &plan = f.plan;
  const size_t n = job.n, n_sums = plan.n_sums, nslots = plan.nslots;
  const bool timed = ctx->timing;
  hipStream_t st = L->stream;
  u64 *d_pos = L->store.rep.as<u64>(), *d_newoff = d_pos + n + 1, *d_sums = d_newoff + n, *d_nkeys = d_sums + n_sums;
  u32 *d_nvals = (u32 *)(d_nkeys + nslots), *d_size = d_nvals + nslots;
  u8 *d_reason = (u8 *)(d_size + n + 1);
  const store_rep_dev dev{d_pos, d_newoff, d_sums, d_size, d_reason, f.img_out, f.dev_cap};
  STCHK(hipMemsetAsync(d_nkeys, 0xFF, nslots * 12, st));
  if (timed) STCHK(L->store.t_rep.record(0, st));
  hipLaunchKernelGGL(k_store_keep_chan, dim3(blocks_for(n)), dim3(256), 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, d_nkeys, d_nvals, plan.nbits,
                     d_reason, d_size);
  hipLaunchKernelGGL(k_store_keep_rest, dim3(blocks_for(n + 1)), dim3(256), 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, job.d_keys, job.d_vals,
                     job.bits, (const u64 *)d_nkeys, (const u32 *)d_nvals, plan.nbits, d_reason, d_size);
  uint64_t counts[8] = {};
  rc = store_repair_finish(ctx, job, len, plan, dev, f.head, verdict, new_off, reason, out, f.want_out, out_cap, summary, counts, &repair->out_len, repair->stage_ms);
  store_repair_counts(repair, counts);
  return rc;
}

// ---- latest-wins repair: the same call with four keep stages (store_latest.h) in place of two
extern "C" int lamd_gossip_store_repair_latest(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, const uint8_t *uuid32,
                                               const lamd_store_latest_policy *policy, size_t cap, uint64_t *rec_off, int8_t *verdict, uint64_t *new_off,
                                               uint8_t *reason, size_t *n_records, uint8_t *out, void *d_out, size_t out_cap,
                                               lamd_store_summary *summary, lamd_store_latest_summary *latest) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!policy || !latest || !store_repair_args_ok(store, uuid32, cap, rec_off, verdict, new_off, reason, n_records, summary)) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *latest = lamd_store_latest_summary();
  const lamd_store_latest_policy pol = *policy;
  store_rep_frame f;
  // pos u64[n + 1] | new_off u64[n] | sums u64[n_sums] | latest u64[2 n] | nlatest u64[nslots] | nkeys u64[nslots] | nvals u32[nslots] | size u32[n + 1] |
  // reason u8[n] | dying u8[n]
  int rc = store_repair_begin(ctx, store, len, d_store, uuid32, cap, rec_off, verdict, n_records, out, d_out, out_cap, summary, &latest->out_len,
                              [](size_t n, size_t n_sums, size_t nslots) { return 8 * (4 * n + 1 + n_sums + 2 * nslots) + 4 * (nslots + n + 1) + 2 * n + 16; }, &f);
  lamd_ctx *L = f.job.L;
  if (rc != LAMD_OK || !L) return rc;
  const store_job &job = f.job;
  const store_rep_plan &plan = f.plan;
  const size_t n = job.n, n_sums = plan.n_sums, nslots = plan.nslots;
  const bool timed = ctx->timing;
  hipStream_t st = L->stream;
  u64 *d_pos = L->store.rep.as<u64>(), *d_newoff = d_pos + n + 1, *d_sums = d_newoff + n, *d_latest = d_sums + n_sums, *d_nlatest = d_latest + 2 * n,
      *d_nkeys = d_nlatest + nslots;
  u32 *d_nvals = (u32 *)(d_nkeys + nslots), *d_size = d_nvals + nslots;
  u8 *d_reason = (u8 *)(d_size + n + 1), *d_dying = d_reason + n;
  const store_rep_dev dev{d_pos, d_newoff, d_sums, d_size, d_reason, f.img_out, f.dev_cap};
  if (timed) STCHK(L->store.t_rep.record(0, st));
  STCHK(hipMemsetAsync(d_latest, 0, 8 * (2 * n + nslots), st));
  STCHK(hipMemsetAsync(d_nkeys, 0xFF, nslots * 12, st));
  STCHK(hipMemsetAsync(d_dying, 0, n, st));
  const dim3 grid(blocks_for(n)), block(256);
  hipLaunchKernelGGL(k_store_latest_upd, grid, block, 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, job.d_keys, job.d_vals, job.bits, pol, d_latest,
                     d_dying);
  hipLaunchKernelGGL(k_store_latest_chan, grid, block, 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, pol, (const u64 *)d_latest, (const u8 *)d_dying,
                     d_nkeys, d_nvals, plan.nbits, d_reason, d_size);
  hipLaunchKernelGGL(k_store_latest_node, grid, block, 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, (const u64 *)d_nkeys, (const u32 *)d_nvals,
                     plan.nbits, pol, d_nlatest);
  hipLaunchKernelGGL(k_store_latest_rest, dim3(blocks_for(n + 1)), block, 0, st, (u32)n, job.img, len, job.d_recoff, job.d_verdict, job.d_keys, job.d_vals,
                     job.bits, (const u64 *)d_nkeys, (const u32 *)d_nvals, plan.nbits, pol, (const u64 *)d_latest, (const u64 *)d_nlatest, d_reason, d_size);
  uint64_t counts[8] = {};
  rc = store_repair_finish(ctx, job, len, plan, dev, f.head, verdict, new_off, reason, out, f.want_out, out_cap, summary, counts, &latest->out_len, latest->stage_ms);
  store_repair_counts(latest, counts);
  latest->dropped_superseded = counts[STORE_DROP_SUPERSEDED];
  latest->dropped_timestamp = counts[STORE_DROP_TIMESTAMP];
  latest->dropped_stale = counts[STORE_DROP_STALE];
  return rc;
}

// ---- the channel digest of a store image, and query_channel_range answered from it.  Both calls run on the context's own stream.
struct lamd_store_digest {
  lamd_ctx *ctx = nullptr;
  void *mem = nullptr;        // scid u64[cap] | bare u64[cap] | ts u32[2 cap] | csum u32[2 cap] | rec u32[3 cap]
  u64 *scid = nullptr, *bare = nullptr;   // bare: the scids of the channels without an update, ascending
  u32 *ts = nullptr, *csum = nullptr, *rec = nullptr;
  size_t cap = 0, count = 0, nbare = 0;   // cap = the records of the store: the sorts run over that many pairs / keys
};
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
extern "C" void lamd_store_digest_free(lamd_store_digest *d) {
  if (!d) return;
  if (d->mem) {
    (void)hipSetDevice(d->ctx->device);
    (void)hipFree(d->mem);
  }
  delete d;
}
extern "C" size_t lamd_store_digest_count(const lamd_store_digest *d) { return d ? d->count : 0; }
extern "C" int lamd_store_digest_read(const lamd_store_digest *d, size_t cap, uint64_t *scid, uint32_t *ts, uint32_t *csum, uint32_t *rec) {
  if (!d) return LAMD_ERR_ARG;
  lamd_ctx *ctx = d->ctx;
  if (cap < d->count) { ctx->err = "gossip_store digest: arrays too small"; return LAMD_ERR_ARG; }
  if (d->count == 0) return LAMD_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (scid) HIPCHK(ctx, hipMemcpy(scid, d->scid, 8 * d->count, hipMemcpyDeviceToHost));
  if (ts) HIPCHK(ctx, hipMemcpy(ts, d->ts, 8 * d->count, hipMemcpyDeviceToHost));
  if (csum) HIPCHK(ctx, hipMemcpy(csum, d->csum, 8 * d->count, hipMemcpyDeviceToHost));
  if (rec) HIPCHK(ctx, hipMemcpy(rec, d->rec, 12 * d->count, hipMemcpyDeviceToHost));
  return LAMD_OK;
}
extern "C" size_t lamd_store_digest_bare_count(const lamd_store_digest *d) { return d ? d->nbare : 0; }
extern "C" int lamd_store_digest_read_bare(const lamd_store_digest *d, size_t cap, uint64_t *scid) {
  if (!d) return LAMD_ERR_ARG;
  lamd_ctx *ctx = d->ctx;
  if (cap < d->nbare || (d->nbare && !scid)) { ctx->err = "gossip_store digest: array too small"; return LAMD_ERR_ARG; }
  if (d->nbare == 0) return LAMD_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(scid, d->bare, 8 * d->nbare, hipMemcpyDeviceToHost));
  return LAMD_OK;
}
extern "C" int lamd_gossip_store_digest_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
                                              const int8_t *verdict, lamd_store_digest **digest, lamd_store_digest_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (digest) *digest = nullptr;
  if ((!store && !d_store) || !digest || !summary || (n && !rec_off)) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  if (n >= (size_t)STORE_NONE / 2) { ctx->err = "gossip_store digest: too many records"; return LAMD_ERR_ARG; }
  *summary = lamd_store_digest_summary();
  summary->records = n;
  // an error return drains the stream (drain_fail: queued copies read the caller's arrays), then the digest frees itself
  std::unique_ptr<lamd_store_digest, void (*)(lamd_store_digest *)> D(new (std::nothrow) lamd_store_digest(), lamd_store_digest_free);
  if (!D) return LAMD_ERR_NOMEM;
  D->ctx = ctx;
  D->cap = n;
  if (n == 0) { *digest = D.release(); return LAMD_OK; }
  lamd_ctx *L = ctx;
  hipStream_t st = ctx->stream;
  hipError_t e0 = hipSetDevice(ctx->device);
  if (e0 == hipSuccess) e0 = hipMalloc(&D->mem, 44 * n);
  if (e0 != hipSuccess) {
    ctx->err = std::string("gossip_store digest: ") + hipGetErrorString(e0);
    return drain_fail(ctx, L, e0 == hipErrorOutOfMemory ? LAMD_ERR_NOMEM : LAMD_ERR_HIP);
  }
  D->scid = (u64 *)D->mem;
  D->bare = D->scid + n;
  D->ts = (u32 *)(D->bare + n);
  D->csum = D->ts + 2 * n;
  D->rec = D->csum + 2 * n;
  u32 bits = 1;
  while (((size_t)1 << bits) < 2 * n) bits++;
  const size_t slots = ((size_t)1 << bits) + 1;
  size_t sort_bytes = 0, sort_bare_bytes = 0;
  STCHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 64, st));
  STCHK(rocprim::radix_sort_keys(nullptr, sort_bare_bytes, (const u64 *)nullptr, (u64 *)nullptr, n, 0, 64, st));
  if (sort_bare_bytes > sort_bytes) sort_bytes = sort_bare_bytes;   // the two sorts follow each other in one workspace
  // rec_off u64[n] | pair_key u64[n] | bare_key u64[n] | keys u64[slots] | vals u32[slots] | slot u32[2 n] | pair_val u32[n] | ann u32[n] | cnt u32[DIGEST_CNTS] |
  // verdict i8[n] | (256-aligned) the sorts' workspace
  const size_t o_sort = align_up(8 * (3 * n + slots) + 4 * (slots + 4 * n + DIGEST_CNTS) + n, 256);
  int rc;
  if ((rc = ensure(ctx, &ctx->store.dig, o_sort + sort_bytes + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (!d_store && (rc = ensure(ctx, &ctx->store.img, len + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  u64 *d_recoff = ctx->store.dig.as<u64>(), *d_pkey = d_recoff + n, *d_bkey = d_pkey + n, *d_keys = d_bkey + n;
  u32 *d_vals = (u32 *)(d_keys + slots), *d_slot = d_vals + slots, *d_pval = d_slot + 2 * n, *d_ann = d_pval + n, *d_cnt = d_ann + n;
  int8_t *d_verdict = verdict ? (int8_t *)(d_cnt + DIGEST_CNTS) : nullptr;
  void *d_sort = ctx->store.dig.as<u8>() + o_sort;
  const u8 *img = (const u8 *)d_store;
  if (!d_store) {
    STCHK(hipMemcpyAsync(ctx->store.img.p, store, len, hipMemcpyHostToDevice, st));
    img = ctx->store.img.as<const u8>();
  }
  STCHK(hipMemcpyAsync(d_recoff, rec_off, 8 * n, hipMemcpyHostToDevice, st));
  if (verdict) STCHK(hipMemcpyAsync(d_verdict, verdict, n, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(d_pkey, 0xFF, 8 * (2 * n + slots) + 4 * slots, st));   // pair_key, bare_key, keys, vals
  STCHK(hipMemsetAsync(d_slot, 0, 8 * n, st));
  STCHK(hipMemsetAsync(d_pval, 0xFF, 4 * n, st));
  STCHK(hipMemsetAsync(d_cnt, 0, 4 * DIGEST_CNTS, st));
  const dim3 grid(blocks_for(n)), block(256);
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  hipLaunchKernelGGL(k_digest_index, grid, block, 0, st, (u32)n, img, len, (const u64 *)d_recoff, (const int8_t *)d_verdict, d_keys, d_vals, bits);
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  hipLaunchKernelGGL(k_digest_slots, grid, block, 0, st, (u32)n, img, len, (const u64 *)d_recoff, (const int8_t *)d_verdict, (const u64 *)d_keys, (const u32 *)d_vals,
                     bits, d_slot, d_cnt);
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  hipLaunchKernelGGL(k_digest_chan, grid, block, 0, st, (u32)n, img, len, (const u64 *)d_recoff, (const int8_t *)d_verdict, (const u64 *)d_keys, (const u32 *)d_vals,
                     bits, (const u32 *)d_slot, d_pkey, d_pval, d_bkey, d_cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  STCHK(rocprim::radix_sort_pairs(d_sort, sort_bytes, (const u64 *)d_pkey, D->scid, (const u32 *)d_pval, d_ann, n, 0, 64, st));
  STCHK(rocprim::radix_sort_keys(d_sort, sort_bytes, (const u64 *)d_bkey, D->bare, n, 0, 64, st));
  if (timed) STCHK(ctx->store.t_dig.record(4, st));
  hipLaunchKernelGGL(k_digest_entries, grid, block, 0, st, (u32)n, img, len, (const u64 *)d_recoff, (const u32 *)d_slot, (const u32 *)d_ann, (const u32 *)d_cnt, D->ts,
                     D->csum, D->rec);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(5, st));
  u32 cnt[DIGEST_CNTS] = {};
  STCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  if (timed) STCHK(ctx->store.t_dig.read(5, summary->stage_ms));
  D->count = cnt[DIGEST_CNT_ENTRIES];
  D->nbare = cnt[DIGEST_CNT_NO_UPDATE];
  summary->entries = cnt[DIGEST_CNT_ENTRIES];
  summary->channels = cnt[DIGEST_CNT_CHANNELS];
  summary->channels_no_update = cnt[DIGEST_CNT_NO_UPDATE];
  summary->updates_no_channel = cnt[DIGEST_CNT_NO_CHANNEL];
  summary->updates_in_front = cnt[DIGEST_CNT_IN_FRONT];
  summary->updates_short = cnt[DIGEST_CNT_SHORT];
  *digest = D.release();
  return LAMD_OK;
}

extern "C" int lamd_channel_range_reply_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, size_t nq, const uint8_t *queries,
                                              const uint64_t *qoff, uint32_t max_encoded_bytes, int8_t *status, uint64_t *reply_first, size_t msg_cap,
                                              uint64_t *msg_off, uint8_t *out, void *d_out, size_t out_cap, lamd_range_reply_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!digest || digest->ctx != ctx || !chain_hash32 || !summary || !reply_first || (nq && (!queries || !qoff || !status)) || (msg_cap && !msg_off) ||
      nq >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_range_reply_summary();
  reply_first[0] = 0;
  if (nq == 0) {
    if (msg_cap) msg_off[0] = 0;
    return LAMD_OK;
  }
  std::vector<store_range_query> qs(nq);
  for (size_t q = 0; q < nq; q++) {
    if (qoff[q + 1] < qoff[q]) { ctx->err = "channel_range replies: decreasing query offsets"; return LAMD_ERR_ARG; }
    qs[q] = store_range_parse(queries + qoff[q], (size_t)(qoff[q + 1] - qoff[q]), chain_hash32, max_encoded_bytes);
    status[q] = (int8_t)qs[q].kind;
    (qs[q].kind == STORE_RANGE_ANSWERED ? summary->answered : qs[q].kind == STORE_RANGE_FOREIGN ? summary->foreign : summary->malformed)++;
  }
  lamd_ctx *L = ctx;   // queued copies read this frame's vectors: STCHK drains the stream
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const u32 count = (u32)digest->count;
  // no query has more than count + 1 replies: the device arrays need not follow a generous msg_cap
  const u64 most = (u64)nq * ((u64)count + 1), cap_dev = msg_cap < most ? msg_cap : most;
  // msg_first u64[nq + 1] | byte_first u64[nq + 1] | n_bytes u64[nq] | msg_off u64[cap_dev + 1] | queries[nq] | msgs[cap_dev] | n_msgs u32[nq]
  int rc;
  if ((rc = ensure(ctx, &ctx->store.rng, 8 * (3 * nq + 2 + cap_dev + 1) + sizeof(store_range_query) * nq + sizeof(store_range_msg) * cap_dev + 4 * nq + 16)) != LAMD_OK)
    return rc;
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  u64 *d_mfirst = ctx->store.rng.as<u64>(), *d_bfirst = d_mfirst + nq + 1, *d_nbytes = d_bfirst + nq + 1, *d_msgoff = d_nbytes + nq;
  store_range_query *d_qs = (store_range_query *)(d_msgoff + cap_dev + 1);
  store_range_msg *d_msgs = (store_range_msg *)(d_qs + nq);
  u32 *d_nmsgs = (u32 *)(d_msgs + cap_dev);
  std::vector<u64> h_first(2 * (nq + 1)), h_msgoff(cap_dev + 1);
  const dim3 grid(blocks_for(nq)), block(256);
  STCHK(hipMemcpyAsync(d_qs, qs.data(), sizeof(store_range_query) * nq, hipMemcpyHostToDevice, st));
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  hipLaunchKernelGGL(k_range_count, grid, block, 0, st, (u32)nq, (const store_range_query *)d_qs, (const u64 *)digest->scid, count, d_nmsgs, d_nbytes);
  hipLaunchKernelGGL(k_range_scan, dim3(1), block, 0, st, (u32)nq, (const u32 *)d_nmsgs, (const u64 *)d_nbytes, d_mfirst, d_bfirst);
  hipLaunchKernelGGL(k_range_plan, grid, block, 0, st, (u32)nq, (const store_range_query *)d_qs, (const u64 *)digest->scid, count, (const u64 *)d_mfirst,
                     (const u64 *)d_bfirst, (u64)cap_dev, d_msgs, d_msgoff);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  STCHK(hipMemcpyAsync(h_first.data(), d_mfirst, 16 * (nq + 1), hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(h_msgoff.data(), d_msgoff, 8 * (cap_dev + 1), hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  const u64 n_msgs = h_first[nq], total = h_first[2 * nq + 1];
  summary->messages = n_msgs;
  summary->bytes = total;
  memcpy(reply_first, h_first.data(), 8 * (nq + 1));
  if (n_msgs > msg_cap) { ctx->err = "channel_range replies: msg_off too small"; return LAMD_ERR_ARG; }
  const bool want_out = out || d_out;
  if (want_out && total > out_cap) { ctx->err = "channel_range replies: output buffer too small"; return LAMD_ERR_ARG; }
  if (msg_off) memcpy(msg_off, h_msgoff.data(), 8 * (n_msgs + 1));
  if (!want_out || n_msgs == 0) return LAMD_OK;
  if (!d_out && (rc = ensure(ctx, &ctx->store.rng_out, total + 16)) != LAMD_OK) return rc;
  u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.rng_out.as<u8>();
  const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
  hipLaunchKernelGGL(k_range_encode, dim3((unsigned)((words + 255) / 256)), block, 0, st, words, (const store_range_msg *)d_msgs, (const u64 *)d_msgoff, (u32)n_msgs,
                     (const store_range_query *)d_qs, store_digest_view{digest->scid, digest->ts, digest->csum}, d_bytes, total);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  if (timed) STCHK(ctx->store.t_dig.read(2, summary->stage_ms));
  return LAMD_OK;
}


// ---- peers' reply_channel_range compared with the digest (lamd_channel_range_compare_batch; per-message, per-entry and per-word logic in
// store_compare.h).  cnt: CMP_CNT_* words, all 0; the two lists' allocators take one atomic per wave.
enum { CMP_CNT_UNKNOWN = 0, CMP_CNT_STALE = 1, CMP_CNT_UNKNOWN_MERGED = 2, CMP_CNT_STALE_MERGED = 3, CMP_CNTS = 4 };
// k_cmp_classify: one lane per entry of the accepted messages; ent_first[n_msgs + 1]: the prefix sums of their entry counts.  cls[e] = the class;
// the unknown scids and the stale (scid, flags) pairs are compacted in any order (E slots each, the keys preset to all-ones bytes as in k_digest_chan).
__global__ void __launch_bounds__(256) k_cmp_classify(u32 E, const u8 *__restrict__ bytes, const store_cmp_msg *__restrict__ pm, const u64 *__restrict__ ent_first,
                                                      u32 n_msgs, store_cmp_digest d, u8 *__restrict__ cls, u64 *__restrict__ unk_key,
                                                      u64 *__restrict__ stale_key, u32 *__restrict__ stale_val, u32 *cnt) {
  const u32 e = blockIdx.x * 256 + threadIdx.x;
  u64 scid = 0;
  u32 c = STORE_CMP_NOTHING;
  if (e < E) {
    const u32 i = store_range_locate(ent_first, n_msgs, e);
    c = store_cmp_entry(bytes, pm[i], (u32)(e - ent_first[i]), d, &scid);
    cls[e] = (u8)c;
  }
  const u32 pu = wave_alloc(&cnt[CMP_CNT_UNKNOWN], c == STORE_CMP_UNKNOWN, 0, nullptr), ps = wave_alloc(&cnt[CMP_CNT_STALE], c > STORE_CMP_UNKNOWN, 0, nullptr);
  if (c == STORE_CMP_UNKNOWN && pu < E) unk_key[pu] = scid;
  if (c > STORE_CMP_UNKNOWN && ps < E) {
    stale_key[ps] = scid;
    stale_val[ps] = c;
  }
}
// k_cmp_per_msg: one WAVE per message sums the classes of its entries: per_msg[3 i ..] = entries, unknown, stale.  No atomics.
__global__ void __launch_bounds__(256) k_cmp_per_msg(u32 n_msgs, const u64 *__restrict__ ent_first, const u8 *__restrict__ cls, u32 *__restrict__ per_msg) {
  const u32 i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (i >= n_msgs) return;   // (the whole wave)
  const u64 a = ent_first[i], b = ent_first[i + 1];
  u32 u = 0, s = 0;
  for (u64 e = a + lane; e < b; e += 64) {
    const u32 c = cls[e];
    u += c == STORE_CMP_UNKNOWN;
    s += c > STORE_CMP_UNKNOWN;
  }
  for (int o = 32; o; o >>= 1) {
    u += __shfl_down(u, o);
    s += __shfl_down(s, o);
  }
  if (lane == 0) {
    per_msg[3 * (size_t)i] = (u32)(b - a);
    per_msg[3 * (size_t)i + 1] = u;
    per_msg[3 * (size_t)i + 2] = s;
  }
}
// The merge of one sorted list of *count real elements (the pads behind them are not looked at): k_cmp_heads marks where a run of equal
// scids opens, rocPRIM's inclusive scan numbers the runs, k_cmp_merge writes run r's scid to out_key[r] and ORs its elements' flags into
// out_val[r] (preset to 0; nullptr for the unknown list) -- OR does not care in which order the lanes arrive.
__global__ void __launch_bounds__(256) k_cmp_heads(u32 E, const u64 *__restrict__ key, const u32 *__restrict__ count, u32 *__restrict__ head) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= E) return;
  const u32 c = *count < E ? *count : E;
  head[j] = j < c && store_cmp_head(key, j);
}
__global__ void __launch_bounds__(256) k_cmp_merge(u32 E, const u64 *__restrict__ key, const u32 *__restrict__ val, const u32 *__restrict__ count,
                                                   const u32 *__restrict__ pos, u64 *__restrict__ out_key, u32 *out_val) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  const u32 c = *count < E ? *count : E;
  if (j >= c) return;
  const u32 r = pos[j] - 1;
  if (store_cmp_head(key, j)) out_key[r] = key[j];
  if (out_val) atomicOr(&out_val[r], val[j]);
}
// k_cmp_plan: the merged lists' lengths into cnt, and the offset of every message and of the end (msg_off[0 .. messages]; the grid covers max_msgs + 1)
__global__ void __launch_bounds__(256) k_cmp_plan(u32 E, u32 max_msgs, u32 max_unknown, u32 max_stale, const u32 *__restrict__ pos_unknown,
                                                  const u32 *__restrict__ pos_stale, u32 *cnt, u64 *__restrict__ msg_off) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  const u32 cu = cnt[CMP_CNT_UNKNOWN] < E ? cnt[CMP_CNT_UNKNOWN] : E, cs = cnt[CMP_CNT_STALE] < E ? cnt[CMP_CNT_STALE] : E;
  store_cmp_layout y;
  y.unknown = cu ? pos_unknown[cu - 1] : 0;
  y.stale = cs ? pos_stale[cs - 1] : 0;
  y.max_unknown = max_unknown;
  y.max_stale = max_stale;
  if (j == 0) {
    cnt[CMP_CNT_UNKNOWN_MERGED] = y.unknown;
    cnt[CMP_CNT_STALE_MERGED] = y.stale;
  }
  if (j <= max_msgs && j <= store_cmp_messages(y)) msg_off[j] = store_cmp_msg_off(y, j);
}
// k_cmp_encode: one aligned 32-bit word of the output per lane
__global__ void __launch_bounds__(256) k_cmp_encode(u64 words, store_cmp_layout y, const u64 *__restrict__ msg_off, u32 n_msgs, const u64 *__restrict__ unknown,
                                                    const u64 *__restrict__ stale, const u32 *__restrict__ flags, u8 *__restrict__ out, u64 total) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k < words) store_cmp_word(y, msg_off, n_msgs, unknown, stale, flags, out, total, (u32)((uintptr_t)out & 3), k);
}

extern "C" int lamd_channel_range_compare_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, size_t n, const uint8_t *msgs,
                                                const uint64_t *moff, const uint32_t *want_first, const uint32_t *want_end, uint32_t max_unknown,
                                                uint32_t max_stale, int8_t *status, uint32_t *per_msg, size_t scid_cap, uint64_t *unknown_scid,
                                                uint64_t *stale_scid, uint8_t *stale_flags, size_t msg_cap, uint64_t *msg_off, uint8_t *out, void *d_out,
                                                size_t out_cap, lamd_range_compare_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!digest || digest->ctx != ctx || !chain_hash32 || !summary || (n && (!msgs || !moff || !status || !per_msg)) || !want_first != !want_end ||
      (scid_cap && (!unknown_scid || !stale_scid || !stale_flags)) || (msg_cap && !msg_off) || n >= (size_t)STORE_NONE ||
      max_unknown > STORE_CMP_MAX_UNKNOWN || max_stale > STORE_CMP_MAX_STALE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_range_compare_summary();
  store_cmp_layout y;
  y.unknown = y.stale = 0;
  y.max_unknown = max_unknown ? max_unknown : STORE_CMP_MAX_UNKNOWN;
  y.max_stale = max_stale ? max_stale : STORE_CMP_MAX_STALE;
  memcpy(y.chain, chain_hash32, 32);
  // the framing, on the host: status, and where the entries of the accepted messages lie
  std::vector<store_cmp_msg> pm(n);
  std::vector<u64> first(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    if (moff[i + 1] < moff[i]) { ctx->err = "channel_range comparison: decreasing message offsets"; return LAMD_ERR_ARG; }
    pm[i] = store_cmp_parse(msgs + moff[i], (size_t)(moff[i + 1] - moff[i]), moff[i], chain_hash32, want_first != nullptr, want_first ? want_first[i] : 0,
                            want_end ? want_end[i] : 0);
    status[i] = (int8_t)pm[i].status;
    summary->by_status[pm[i].status < 0 ? 7 : pm[i].status]++;
    first[i + 1] = first[i] + pm[i].n;
    per_msg[3 * i] = per_msg[3 * i + 1] = per_msg[3 * i + 2] = 0;
  }
  const u64 total_entries = first[n];
  if (total_entries >= (u64)STORE_NONE) { ctx->err = "channel_range comparison: too many entries"; return LAMD_ERR_ARG; }
  summary->entries = total_entries;
  if (total_entries == 0) {   // nothing to look up: no list, no message
    if (msg_cap) msg_off[0] = 0;
    return LAMD_OK;
  }
  const u32 E = (u32)total_entries;
  const size_t n_bytes = (size_t)moff[n];
  const u64 max_msgs = (u64)store_cmp_msgs_of(E, y.max_unknown) + store_cmp_msgs_of(E, y.max_stale);
  lamd_ctx *L = ctx;   // queued copies read this frame's vectors: STCHK drains the stream
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, (size_t)E, 0, 64, st));
  STCHK(rocprim::radix_sort_keys(nullptr, need, (const u64 *)nullptr, (u64 *)nullptr, (size_t)E, 0, 64, st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::inclusive_scan(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, (size_t)E, rocprim::plus<u32>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  // ent_first u64[n + 1] | unk_key, stale_key, unk_sorted, stale_sorted, unk_out, stale_out u64[E] each | msg_off u64[max_msgs + 1] | pm[n] |
  // stale_val, stale_val_sorted, head, pos_unk, pos_stale, flags_out u32[E] each | per_msg u32[3 n] | cnt u32[CMP_CNTS] | cls u8[E] | the messages |
  // (256-aligned) the workspace of the sorts and the scans
  const size_t o_tmp = align_up(8 * (n + 1 + 6 * (size_t)E + max_msgs + 1) + sizeof(store_cmp_msg) * n + 4 * (6 * (size_t)E + 3 * n + CMP_CNTS) + E + n_bytes, 256);
  int rc;
  if ((rc = ensure(ctx, &ctx->store.cmp, o_tmp + tmp_bytes + 16)) != LAMD_OK) return rc;
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  u64 *d_first = ctx->store.cmp.as<u64>(), *d_ukey = d_first + n + 1, *d_skey = d_ukey + E, *d_usort = d_skey + E, *d_ssort = d_usort + E, *d_uout = d_ssort + E,
      *d_sout = d_uout + E, *d_msgoff = d_sout + E;
  store_cmp_msg *d_pm = (store_cmp_msg *)(d_msgoff + max_msgs + 1);
  u32 *d_sval = (u32 *)(d_pm + n), *d_svsort = d_sval + E, *d_head = d_svsort + E, *d_upos = d_head + E, *d_spos = d_upos + E, *d_flags = d_spos + E,
      *d_permsg = d_flags + E, *d_cnt = d_permsg + 3 * n;
  u8 *d_cls = (u8 *)(d_cnt + CMP_CNTS), *d_msgs = d_cls + E;
  void *d_tmp = ctx->store.cmp.as<u8>() + o_tmp;
  u32 cnt[CMP_CNTS] = {};
  std::vector<u32> h_flags;
  STCHK(hipMemcpyAsync(d_first, first.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(d_pm, pm.data(), sizeof(store_cmp_msg) * n, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(d_msgs, msgs, n_bytes, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(d_ukey, 0xFF, 16 * (size_t)E, st));   // unk_key, stale_key
  STCHK(hipMemsetAsync(d_sval, 0, 4 * (size_t)E, st));
  STCHK(hipMemsetAsync(d_flags, 0, 4 * (size_t)E, st));
  STCHK(hipMemsetAsync(d_cnt, 0, 4 * CMP_CNTS, st));
  const dim3 grid(blocks_for(E)), block(256);
  const store_cmp_digest dg{digest->scid, digest->ts, (u32)digest->count, digest->bare, (u32)digest->nbare};
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  hipLaunchKernelGGL(k_cmp_classify, grid, block, 0, st, E, (const u8 *)d_msgs, (const store_cmp_msg *)d_pm, (const u64 *)d_first, (u32)n, dg, d_cls, d_ukey, d_skey,
                     d_sval, d_cnt);
  hipLaunchKernelGGL(k_cmp_per_msg, dim3((unsigned)((n + 3) / 4)), block, 0, st, (u32)n, (const u64 *)d_first, (const u8 *)d_cls, d_permsg);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  // stable sorts of all E slots: the pads (largest key) stay behind the real elements, whatever scids the peers sent
  STCHK(rocprim::radix_sort_keys(d_tmp, tmp_bytes, (const u64 *)d_ukey, d_usort, (size_t)E, 0, 64, st));
  STCHK(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, (const u64 *)d_skey, d_ssort, (const u32 *)d_sval, d_svsort, (size_t)E, 0, 64, st));
  hipLaunchKernelGGL(k_cmp_heads, grid, block, 0, st, E, (const u64 *)d_usort, (const u32 *)(d_cnt + CMP_CNT_UNKNOWN), d_head);
  STCHK(rocprim::inclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_head, d_upos, (size_t)E, rocprim::plus<u32>(), st));
  hipLaunchKernelGGL(k_cmp_merge, grid, block, 0, st, E, (const u64 *)d_usort, (const u32 *)nullptr, (const u32 *)(d_cnt + CMP_CNT_UNKNOWN), (const u32 *)d_upos, d_uout,
                     (u32 *)nullptr);
  hipLaunchKernelGGL(k_cmp_heads, grid, block, 0, st, E, (const u64 *)d_ssort, (const u32 *)(d_cnt + CMP_CNT_STALE), d_head);
  STCHK(rocprim::inclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_head, d_spos, (size_t)E, rocprim::plus<u32>(), st));
  hipLaunchKernelGGL(k_cmp_merge, grid, block, 0, st, E, (const u64 *)d_ssort, (const u32 *)d_svsort, (const u32 *)(d_cnt + CMP_CNT_STALE), (const u32 *)d_spos, d_sout,
                     d_flags);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  hipLaunchKernelGGL(k_cmp_plan, dim3(blocks_for((size_t)max_msgs + 1)), block, 0, st, E, (u32)max_msgs, y.max_unknown, y.max_stale, (const u32 *)d_upos,
                     (const u32 *)d_spos, d_cnt, d_msgoff);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  STCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(per_msg, d_permsg, 12 * n, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: counts and sizes
  if (timed) STCHK(ctx->store.t_dig.read(3, summary->stage_ms));
  y.unknown = cnt[CMP_CNT_UNKNOWN_MERGED];
  y.stale = cnt[CMP_CNT_STALE_MERGED];
  const u64 n_msgs = store_cmp_messages(y), total = store_cmp_msg_off(y, n_msgs);
  summary->entries_unknown = cnt[CMP_CNT_UNKNOWN];
  summary->entries_stale = cnt[CMP_CNT_STALE];
  summary->unknown = y.unknown;
  summary->stale = y.stale;
  summary->unknown_messages = store_cmp_msgs_of(y.unknown, y.max_unknown);
  summary->messages = n_msgs;
  summary->bytes = total;
  const bool want_out = out || d_out;
  if (y.unknown > scid_cap || y.stale > scid_cap) { ctx->err = "channel_range comparison: scid arrays too small"; return LAMD_ERR_ARG; }
  if (n_msgs > msg_cap) { ctx->err = "channel_range comparison: msg_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "channel_range comparison: output buffer too small"; return LAMD_ERR_ARG; }
  if (msg_off)
    for (u64 j = 0; j <= n_msgs; j++) msg_off[j] = store_cmp_msg_off(y, j);   // the closed form k_cmp_plan has left on the device
  if (n_msgs == 0) return LAMD_OK;
  if (y.unknown) STCHK(hipMemcpyAsync(unknown_scid, d_uout, 8 * (size_t)y.unknown, hipMemcpyDeviceToHost, st));
  if (y.stale) {
    h_flags.resize(y.stale);
    STCHK(hipMemcpyAsync(stale_scid, d_sout, 8 * (size_t)y.stale, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(h_flags.data(), d_flags, 4 * (size_t)y.stale, hipMemcpyDeviceToHost, st));
  }
  if (want_out) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.cmp_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.cmp_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    hipLaunchKernelGGL(k_cmp_encode, dim3((unsigned)((words + 255) / 256)), block, 0, st, words, y, (const u64 *)d_msgoff, (u32)n_msgs, (const u64 *)d_uout,
                       (const u64 *)d_sout, (const u32 *)d_flags, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_dig.record(4, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the lists and the bytes
  if (timed && want_out) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_dig.ev[3], ctx->store.t_dig.ev[4]));
    summary->stage_ms[3] = ms;
  }
  for (u32 j = 0; j < y.stale; j++) stale_flags[j] = (uint8_t)h_flags[j];
  return LAMD_OK;
}

// ---- the directory of a store image (lamd_gossip_store_directory_build; per-record logic in store_query.h).  cnt: DIR_CNT_* words, all 0.
enum { DIR_CNT_VALID = 0, DIR_CNT_NODES = 1, DIR_CNT_ANNOUNCED = 2, DIR_CNT_NO_NODE = 3, DIR_CNT_IN_FRONT = 4, DIR_CNT_SHORT = 5, DIR_CNTS = 8 };
// bare_rec: one word per bare channel, preset to all-ones bytes
__global__ void __launch_bounds__(256) k_dir_bare(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                  const int8_t *__restrict__ verdict, const u64 *__restrict__ bare, u32 nbare, u32 *bare_rec) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_dir_bare_one(store, store_len, rec_off, verdict, i, bare, nbare, bare_rec);
}
// one lane per channel c (the entries, then the bare ones): candidates 2 c and 2 c + 1 are its two node ids, or name none
__global__ void __launch_bounds__(256) k_dir_cand(u32 channels, u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                  const u32 *__restrict__ ent_rec, u32 count, const u32 *__restrict__ bare_rec, u64 *__restrict__ cand_off,
                                                  u32 *__restrict__ cand_rec, u32 *__restrict__ perm, u32 *cnt) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (c < channels) {
    const u32 a = c < count ? ent_rec[3 * (size_t)c] : bare_rec[c - count];
    u64 idoff = 0;
    ok = a < n && store_dir_cann_ids(store, store_len, rec_off[a], &idoff);
    for (u32 k = 0; k < 2; k++) {
      cand_off[2 * (size_t)c + k] = ok ? idoff + 33 * k : STORE_DIR_NO_ID;
      cand_rec[2 * (size_t)c + k] = a;
      perm[2 * (size_t)c + k] = 2 * c + k;
    }
  }
  const u64 mask = __ballot(ok);
  if ((threadIdx.x & 63u) == 0 && mask) atomicAdd(&cnt[DIR_CNT_VALID], 2 * (u32)__popcll(mask));
}
__global__ void __launch_bounds__(256) k_dir_keys(u32 m, const u8 *__restrict__ store, const u64 *__restrict__ cand_off, const u32 *__restrict__ perm, u32 pass,
                                                  u64 *__restrict__ key) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j < m) key[j] = store_dir_pass_key(store, cand_off[perm[j]], pass);
}
__global__ void __launch_bounds__(256) k_dir_heads(u32 m, const u8 *__restrict__ store, const u64 *__restrict__ cand_off, const u32 *__restrict__ perm,
                                                   const u32 *__restrict__ cnt, u32 *__restrict__ head) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  head[j] = store_dir_head(store, cand_off, perm, cnt[DIR_CNT_VALID] < m ? cnt[DIR_CNT_VALID] : m, j);
}
// chan_rank: preset to all-ones bytes, node_first too; the lane of the last candidate with an id leaves the number of nodes
__global__ void __launch_bounds__(256) k_dir_merge(u32 m, const u64 *__restrict__ cand_off, const u32 *__restrict__ cand_rec, const u32 *__restrict__ perm,
                                                   const u32 *__restrict__ head, const u32 *__restrict__ pos, u32 *__restrict__ chan_rank,
                                                   u64 *__restrict__ node_off, u32 *node_first, u32 *cnt) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  const u32 valid = cnt[DIR_CNT_VALID] < m ? cnt[DIR_CNT_VALID] : m;
  if (j >= valid) return;
  const u32 r = pos[j] - 1, c = perm[j];
  chan_rank[c] = r;
  if (head[j]) node_off[r] = cand_off[c];
  atomicMin(&node_first[r], cand_rec[c]);
  if (j == valid - 1) cnt[DIR_CNT_NODES] = pos[j];
}
// node_nann: one word per node, preset to 0
__global__ void __launch_bounds__(256) k_dir_nann(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                  const int8_t *__restrict__ verdict, const u64 *__restrict__ node_off, const u32 *__restrict__ node_first,
                                                  u32 *node_nann, u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  const u32 r = i < n ? store_dir_nann_one(store, store_len, rec_off, verdict, i, node_off, node_first, cnt[DIR_CNT_NODES], node_nann) : (u32)STORE_DIR_NANN_NONE;
  wave_count(&cnt[DIR_CNT_NO_NODE], r == STORE_DIR_NANN_NO_NODE);
  wave_count(&cnt[DIR_CNT_IN_FRONT], r == STORE_DIR_NANN_IN_FRONT);
  wave_count(&cnt[DIR_CNT_SHORT], r == STORE_DIR_NANN_SHORT);
}
__global__ void __launch_bounds__(256) k_dir_announced(u32 m, const u32 *__restrict__ node_nann, u32 *cnt) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  wave_count(&cnt[DIR_CNT_ANNOUNCED], j < m && j < cnt[DIR_CNT_NODES] && node_nann[j] != 0);
}
// the nodes' ids, gathered for lamd_store_directory_read_nodes: one lane per byte
__global__ void __launch_bounds__(256) k_dir_ids(u32 nodes, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ node_off, u8 *__restrict__ ids) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= 33 * (size_t)nodes) return;
  const u64 at = node_off[j / 33] + j % 33;
  ids[j] = at < store_len ? store[at] : 0;
}

struct lamd_store_directory {
  lamd_ctx *ctx = nullptr;
  void *mem = nullptr;          // rec_off u64[n] | scid u64[channels] | node_off u64[2 channels] | ent_rec u32[3 count] | bare_rec u32[nbare] |
                                // chan_rank, node_first, node_nann u32[2 channels] each | the image, unless it is the caller's
  const u8 *img = nullptr;      // the image on the device: inside mem, or the caller's d_store
  size_t img_len = 0, n = 0, count = 0, nbare = 0, nodes = 0;
  u64 *rec_off = nullptr, *scid = nullptr, *node_off = nullptr;   // scid: the entries' scids, then the bare ones
  u32 *ent_rec = nullptr, *bare_rec = nullptr, *chan_rank = nullptr, *node_first = nullptr, *node_nann = nullptr;
  store_sq_dir view() const {
    return store_sq_dir{img, img_len, rec_off, (u32)n, scid, ent_rec, (u32)count, scid + count, bare_rec, (u32)nbare, chan_rank, node_nann, (u32)nodes};
  }
};
extern "C" void lamd_store_directory_free(lamd_store_directory *d) {
  if (!d) return;
  if (d->mem) {
    (void)hipSetDevice(d->ctx->device);
    (void)hipFree(d->mem);
  }
  delete d;
}
extern "C" size_t lamd_store_directory_node_count(const lamd_store_directory *d) { return d ? d->nodes : 0; }
extern "C" int lamd_store_directory_read_nodes(const lamd_store_directory *d, size_t cap, uint8_t *id33, uint32_t *first, uint32_t *nann_rec) {
  if (!d) return LAMD_ERR_ARG;
  lamd_ctx *ctx = d->ctx;
  if (cap < d->nodes) { ctx->err = "gossip_store directory: arrays too small"; return LAMD_ERR_ARG; }
  if (d->nodes == 0) return LAMD_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (id33) {
    void *ids = nullptr;
    HIPCHK(ctx, hipMalloc(&ids, 33 * d->nodes));
    hipLaunchKernelGGL(k_dir_ids, dim3(blocks_for(33 * d->nodes)), dim3(256), 0, ctx->stream, (u32)d->nodes, d->img, d->img_len, (const u64 *)d->node_off, (u8 *)ids);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(id33, ids, 33 * d->nodes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    else (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ids);
    HIPCHK(ctx, e);
  }
  if (first) HIPCHK(ctx, hipMemcpy(first, d->node_first, 4 * d->nodes, hipMemcpyDeviceToHost));
  if (nann_rec) {
    HIPCHK(ctx, hipMemcpy(nann_rec, d->node_nann, 4 * d->nodes, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < d->nodes; r++) nann_rec[r] -= 1;   // index + 1, 0: none -> index, UINT32_MAX: none
  }
  return LAMD_OK;
}
extern "C" int lamd_store_directory_read_channels(const lamd_store_directory *d, size_t cap_entries, size_t cap_bare, uint32_t *bare_rec, uint32_t *entry_rank,
                                                  uint32_t *bare_rank) {
  if (!d) return LAMD_ERR_ARG;
  lamd_ctx *ctx = d->ctx;
  if (cap_entries < d->count || cap_bare < d->nbare) { ctx->err = "gossip_store directory: arrays too small"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (bare_rec && d->nbare) HIPCHK(ctx, hipMemcpy(bare_rec, d->bare_rec, 4 * d->nbare, hipMemcpyDeviceToHost));
  if (entry_rank && d->count) HIPCHK(ctx, hipMemcpy(entry_rank, d->chan_rank, 8 * d->count, hipMemcpyDeviceToHost));
  if (bare_rank && d->nbare) HIPCHK(ctx, hipMemcpy(bare_rank, d->chan_rank + 2 * d->count, 8 * d->nbare, hipMemcpyDeviceToHost));
  return LAMD_OK;
}
extern "C" int lamd_gossip_store_directory_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
                                                 const int8_t *verdict, const lamd_store_digest *digest, lamd_store_directory **directory,
                                                 lamd_store_directory_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (directory) *directory = nullptr;
  if ((!store && !d_store) || !digest || digest->ctx != ctx || !directory || !summary || (n && !rec_off) || n != digest->cap) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_store_directory_summary();
  std::unique_ptr<lamd_store_directory, void (*)(lamd_store_directory *)> D(new (std::nothrow) lamd_store_directory(), lamd_store_directory_free);
  if (!D) return LAMD_ERR_NOMEM;
  D->ctx = ctx;
  D->n = n;
  D->count = digest->count;
  D->nbare = digest->nbare;
  D->img_len = len;
  if (n == 0) { *directory = D.release(); return LAMD_OK; }
  const size_t count = D->count, nbare = D->nbare, channels = count + nbare, m = 2 * channels;   // channels <= n < 2^31
  lamd_ctx *L = ctx;   // queued copies read the caller's arrays: an error return drains the stream (drain_fail), then the directory frees itself
  hipStream_t st = ctx->stream;
  const size_t o_img = 8 * (n + channels + m) + 4 * (3 * count + nbare + 3 * m);
  hipError_t e0 = hipSetDevice(ctx->device);
  if (e0 == hipSuccess) e0 = hipMalloc(&D->mem, o_img + (d_store ? 0 : len) + 16);
  if (e0 != hipSuccess) {
    ctx->err = std::string("gossip_store directory: ") + hipGetErrorString(e0);
    return drain_fail(ctx, L, e0 == hipErrorOutOfMemory ? LAMD_ERR_NOMEM : LAMD_ERR_HIP);
  }
  D->rec_off = (u64 *)D->mem;
  D->scid = D->rec_off + n;
  D->node_off = D->scid + channels;
  D->ent_rec = (u32 *)(D->node_off + m);
  D->bare_rec = D->ent_rec + 3 * count;
  D->chan_rank = D->bare_rec + nbare;
  D->node_first = D->chan_rank + m;
  D->node_nann = D->node_first + m;
  D->img = d_store ? (const u8 *)d_store : (const u8 *)D->mem + o_img;
  size_t tmp_bytes = 0, need = 0;
  if (m) {
    STCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, m, 0, 64, st));
    STCHK(rocprim::inclusive_scan(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, m, rocprim::plus<u32>(), st));
    if (need > tmp_bytes) tmp_bytes = need;
  }
  // cand_off, key_in, key_out u64[m] each | cand_rec, perm_a, perm_b, head, pos u32[m] each | cnt u32[DIR_CNTS] | verdict i8[n] | (256-aligned) the sorts' workspace
  const size_t o_tmp = align_up(24 * m + 20 * m + 4 * DIR_CNTS + n, 256);
  int rc;
  if ((rc = ensure(ctx, &ctx->store.dir, o_tmp + tmp_bytes + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  u64 *d_coff = ctx->store.dir.as<u64>(), *d_kin = d_coff + m, *d_kout = d_kin + m;
  u32 *d_crec = (u32 *)(d_kout + m), *d_perm = d_crec + m, *d_perm2 = d_perm + m, *d_head = d_perm2 + m, *d_pos = d_head + m, *d_cnt = d_pos + m;
  int8_t *d_verdict = verdict ? (int8_t *)(d_cnt + DIR_CNTS) : nullptr;
  void *d_tmp = ctx->store.dir.as<u8>() + o_tmp;
  const u8 *img = D->img;
  if (!d_store) STCHK(hipMemcpyAsync((void *)img, store, len, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(D->rec_off, rec_off, 8 * n, hipMemcpyHostToDevice, st));
  if (verdict) STCHK(hipMemcpyAsync(d_verdict, verdict, n, hipMemcpyHostToDevice, st));
  if (count) {
    STCHK(hipMemcpyAsync(D->scid, digest->scid, 8 * count, hipMemcpyDeviceToDevice, st));
    STCHK(hipMemcpyAsync(D->ent_rec, digest->rec, 12 * count, hipMemcpyDeviceToDevice, st));
  }
  if (nbare) STCHK(hipMemcpyAsync(D->scid + count, digest->bare, 8 * nbare, hipMemcpyDeviceToDevice, st));
  if (m) {
    STCHK(hipMemsetAsync(D->bare_rec, 0xFF, 4 * (nbare + 2 * m), st));   // bare_rec, chan_rank, node_first
    STCHK(hipMemsetAsync(D->node_nann, 0, 4 * m, st));
  }
  STCHK(hipMemsetAsync(d_cnt, 0, 4 * DIR_CNTS, st));
  const dim3 grid(blocks_for(n)), gm(blocks_for(m)), block(256);
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  if (nbare)
    hipLaunchKernelGGL(k_dir_bare, grid, block, 0, st, (u32)n, img, len, (const u64 *)D->rec_off, (const int8_t *)d_verdict, (const u64 *)(D->scid + count), (u32)nbare,
                       D->bare_rec);
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  if (m) {
    hipLaunchKernelGGL(k_dir_cand, dim3(blocks_for(channels)), block, 0, st, (u32)channels, (u32)n, img, len, (const u64 *)D->rec_off, (const u32 *)D->ent_rec, (u32)count,
                       (const u32 *)D->bare_rec, d_coff, d_crec, d_perm, d_cnt);
    STCHK(hipGetLastError());
  }
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  if (m) {
    // stable, least significant chunk first; the one-bit pass last: the candidates without an id end behind all others, whatever ids there are
    for (u32 pass = 0; pass < STORE_DIR_PASSES; pass++) {
      hipLaunchKernelGGL(k_dir_keys, gm, block, 0, st, (u32)m, img, (const u64 *)d_coff, (const u32 *)d_perm, pass, d_kin);
      STCHK(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, (const u64 *)d_kin, d_kout, (const u32 *)d_perm, d_perm2, m, 0, pass == 0 ? 8 : pass == 5 ? 1 : 64, st));
      std::swap(d_perm, d_perm2);
    }
  }
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  if (m) {
    hipLaunchKernelGGL(k_dir_heads, gm, block, 0, st, (u32)m, img, (const u64 *)d_coff, (const u32 *)d_perm, (const u32 *)d_cnt, d_head);
    STCHK(rocprim::inclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_head, d_pos, m, rocprim::plus<u32>(), st));
    hipLaunchKernelGGL(k_dir_merge, gm, block, 0, st, (u32)m, (const u64 *)d_coff, (const u32 *)d_crec, (const u32 *)d_perm, (const u32 *)d_head, (const u32 *)d_pos,
                       D->chan_rank, D->node_off, D->node_first, d_cnt);
    STCHK(hipGetLastError());
  }
  if (timed) STCHK(ctx->store.t_dig.record(4, st));
  if (m) {
    hipLaunchKernelGGL(k_dir_nann, grid, block, 0, st, (u32)n, img, len, (const u64 *)D->rec_off, (const int8_t *)d_verdict, (const u64 *)D->node_off,
                       (const u32 *)D->node_first, D->node_nann, d_cnt);
    hipLaunchKernelGGL(k_dir_announced, gm, block, 0, st, (u32)m, (const u32 *)D->node_nann, d_cnt);
    STCHK(hipGetLastError());
  }
  if (timed) STCHK(ctx->store.t_dig.record(5, st));
  u32 cnt[DIR_CNTS] = {};
  STCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  if (timed) STCHK(ctx->store.t_dig.read(5, summary->stage_ms));
  D->nodes = cnt[DIR_CNT_NODES];
  summary->nodes = cnt[DIR_CNT_NODES];
  summary->nodes_announced = cnt[DIR_CNT_ANNOUNCED];
  summary->nann_no_node = cnt[DIR_CNT_NO_NODE];
  summary->nann_in_front = cnt[DIR_CNT_IN_FRONT];
  summary->nann_short = cnt[DIR_CNT_SHORT];
  *directory = D.release();
  return LAMD_OK;
}

// ---- query_short_channel_ids answers (lamd_short_channel_ids_reply_batch; per-occurrence and per-word logic in store_query.h).  The items of a
// batch with S occurrences: item e < S is occurrence e, item S + j is slot j of the sorted distinct (query, rank) keys (2 S slots), item 3 S closes
// the scans.  cnt: SQ_CNT_* words, all 0.
enum { SQ_CNT_KEYS = 0, SQ_CNT_NODES = 1, SQ_CNTS = 4 };
// k_sq_lookup: one lane per occurrence; occ_first[nq + 1]: the prefix sums of the answered queries' scid counts; scid_at[q]: where query q's scids
// start in `bytes`; nkey: 2 S keys preset to all-ones bytes, the real ones compacted in any order
__global__ void __launch_bounds__(256) k_sq_lookup(u32 S, const u8 *__restrict__ bytes, const u64 *__restrict__ scid_at, const u64 *__restrict__ occ_first, u32 nq,
                                                   const u8 *__restrict__ flags, store_sq_dir d, u32 *__restrict__ occ_rec, u32 *__restrict__ icnt,
                                                   u32 *__restrict__ ibytes, u8 *__restrict__ known, u64 *__restrict__ nkey, u32 *cnt) {
  const u32 e = blockIdx.x * 256 + threadIdx.x;
  u32 rank2[2] = {STORE_NONE, STORE_NONE}, q = 0;
  if (e < S) {
    q = store_range_locate(occ_first, nq, e);
    u32 rec3[3], b;
    known[e] = store_sq_lookup(d, store_be64(bytes + scid_at[q] + 8 * (u64)(e - occ_first[q])), flags[e], rec3, &b, rank2);
    for (u32 k = 0; k < 3; k++) occ_rec[3 * (size_t)e + k] = rec3[k];
    icnt[e] = (rec3[0] != STORE_NONE) + (rec3[1] != STORE_NONE) + (rec3[2] != STORE_NONE);
    ibytes[e] = b;
  }
  for (u32 k = 0; k < 2; k++) {
    const bool pred = rank2[k] != STORE_NONE;
    const u32 p = wave_alloc(&cnt[SQ_CNT_KEYS], pred, 0, nullptr);
    if (pred && p < 2 * S) nkey[p] = ((u64)q << 32) | rank2[k];
  }
}
// k_sq_nodes: one lane per slot of the distinct keys (uniq; npos: the scan that numbered them) and one for the closing item: the node's announcement
__global__ void __launch_bounds__(256) k_sq_nodes(u32 S, const u64 *__restrict__ uniq, const u32 *__restrict__ npos, u32 *cnt, store_sq_dir d,
                                                  u32 *__restrict__ node_rec, u32 *__restrict__ icnt, u32 *__restrict__ ibytes) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j > 2 * S) return;
  const u32 ck = cnt[SQ_CNT_KEYS] < 2 * S ? cnt[SQ_CNT_KEYS] : 2 * S, U = ck ? npos[ck - 1] : 0;
  if (j == 0) cnt[SQ_CNT_NODES] = U;
  u32 rec = STORE_NONE, len = 0;
  if (j < U) {
    const u32 rank = (u32)uniq[j], nn = rank < d.nodes ? d.node_nann[rank] : 0;
    len = nn ? store_sq_msg_len(d, nn - 1) : 0;
    if (len) rec = nn - 1;
  }
  if (j < 2 * S) node_rec[j] = rec;
  icnt[S + j] = rec != STORE_NONE;
  ibytes[S + j] = len;
}
// k_sq_per_query: one WAVE per query sums its known occurrences; lane 0 reads the rest off the scans: per_query[4 q ..] = scids, known, channel
// messages, node messages; n_msgs / n_bytes: all its replies; qlo[q]: its first slot among the distinct keys
__global__ void __launch_bounds__(256) k_sq_per_query(u32 nq, u32 S, const int8_t *__restrict__ status, const u64 *__restrict__ occ_first,
                                                      const u8 *__restrict__ known, const u64 *__restrict__ uniq, const u32 *__restrict__ cnt,
                                                      const u64 *__restrict__ mscan, const u64 *__restrict__ bscan, u32 *__restrict__ per_query,
                                                      u32 *__restrict__ n_msgs, u64 *__restrict__ n_bytes, u32 *__restrict__ qlo) {
  const u32 q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= nq) return;   // (the whole wave)
  const u64 a = occ_first[q], b = occ_first[q + 1];
  u32 kn = 0;
  for (u64 e = a + lane; e < b; e += 64) kn += known[e];
  for (int o = 32; o; o >>= 1) kn += __shfl_down(kn, o);
  if (lane) return;
  u32 pq[4] = {0, 0, 0, 0}, msgs = 0, lo = 0;
  u64 bytes = 0;
  if (status[q] == STORE_SQ_ANSWERED) {
    const u32 U = cnt[SQ_CNT_NODES], hi = store_sq_lower(uniq, U, ((u64)q + 1) << 32);
    lo = store_sq_lower(uniq, U, (u64)q << 32);
    pq[0] = (u32)(b - a);
    pq[1] = kn;
    pq[2] = (u32)(mscan[b] - mscan[a]);
    pq[3] = (u32)(mscan[S + hi] - mscan[S + lo]);
    msgs = pq[2] + pq[3] + 1;
    bytes = (bscan[b] - bscan[a]) + (bscan[S + hi] - bscan[S + lo]) + STORE_SQ_END_BYTES;
  } else if (status[q] == STORE_SQ_FOREIGN) {
    msgs = 1;
    bytes = STORE_SQ_END_BYTES;
  }
  for (u32 k = 0; k < 4; k++) per_query[4 * (size_t)q + k] = pq[k];
  n_msgs[q] = msgs;
  n_bytes[q] = bytes;
  qlo[q] = lo;
}
// k_sq_plan: one lane per item and per query: where each message starts and which record it copies (STORE_NONE: an end message)
__global__ void __launch_bounds__(256) k_sq_plan(u32 S, u32 nq, const int8_t *__restrict__ status, const u64 *__restrict__ occ_first,
                                                 const u32 *__restrict__ occ_rec, const u32 *__restrict__ node_rec, const u64 *__restrict__ uniq,
                                                 const u32 *__restrict__ cnt, const u32 *__restrict__ qlo, const u64 *__restrict__ mscan,
                                                 const u64 *__restrict__ bscan, const u64 *__restrict__ msg_first, const u64 *__restrict__ byte_first,
                                                 store_sq_dir d, u64 *__restrict__ msg_off, u32 *__restrict__ msg_rec) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < S) {
    const u32 q = store_range_locate(occ_first, nq, i);
    const u64 a = occ_first[q];
    u64 mi = msg_first[q] + (mscan[i] - mscan[a]), bo = byte_first[q] + (bscan[i] - bscan[a]);
    for (u32 k = 0; k < 3; k++) {
      const u32 r = occ_rec[3 * i + k];
      if (r == STORE_NONE) continue;
      msg_off[mi] = bo;
      msg_rec[mi++] = r;
      bo += store_sq_msg_len(d, r);
    }
  } else if (i < 3 * (u64)S) {
    const u64 j = i - S;
    if (j >= cnt[SQ_CNT_NODES] || node_rec[j] == STORE_NONE) return;
    const u32 q = (u32)(uniq[j] >> 32);
    const u64 a = occ_first[q], b = occ_first[q + 1], lo = qlo[q];
    const u64 mi = msg_first[q] + (mscan[b] - mscan[a]) + (mscan[S + j] - mscan[S + lo]);
    msg_off[mi] = byte_first[q] + (bscan[b] - bscan[a]) + (bscan[S + j] - bscan[S + lo]);
    msg_rec[mi] = node_rec[j];
  } else if (i < 3 * (u64)S + nq) {
    const u32 q = (u32)(i - 3 * (u64)S);
    if (status[q] == STORE_SQ_ANSWERED || status[q] == STORE_SQ_FOREIGN) {
      msg_off[msg_first[q + 1] - 1] = byte_first[q + 1] - STORE_SQ_END_BYTES;
      msg_rec[msg_first[q + 1] - 1] = STORE_NONE;
    }
    if (q == nq - 1) msg_off[msg_first[nq]] = byte_first[nq];
  }
}
// k_sq_encode: one aligned 32-bit word of the output per lane
__global__ void __launch_bounds__(256) k_sq_encode(u64 words, store_sq_dir d, store_sq_out o, u8 *__restrict__ out, u64 total) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k < words) store_sq_word(d, o, out, total, (u32)((uintptr_t)out & 3), k);
}

extern "C" int lamd_short_channel_ids_reply_batch(lamd_ctx *ctx, const lamd_store_directory *directory, const uint8_t *chain_hash32, size_t nq,
                                                  const uint8_t *queries, const uint64_t *qoff, int8_t *status, uint32_t *per_query, uint64_t *reply_first,
                                                  size_t msg_cap, uint64_t *msg_off, uint32_t *msg_rec, uint8_t *out, void *d_out, size_t out_cap,
                                                  lamd_scid_reply_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!directory || directory->ctx != ctx || !chain_hash32 || !summary || !reply_first || (nq && (!queries || !qoff || !status || !per_query)) ||
      (msg_cap && !msg_off) || nq >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_scid_reply_summary();
  reply_first[0] = 0;
  if (nq == 0) {
    if (msg_cap) msg_off[0] = 0;
    return LAMD_OK;
  }
  // the framing, on the host: status, where the scids of the answered queries lie, and their flags, one byte each
  const u64 q0 = qoff[0];
  std::vector<u64> first(nq + 1, 0), q_at(nq), scid_at(nq, 0);
  std::vector<store_sq_query> pq(nq);
  for (size_t q = 0; q < nq; q++) {
    if (qoff[q + 1] < qoff[q]) { ctx->err = "short_channel_ids replies: decreasing query offsets"; return LAMD_ERR_ARG; }
    pq[q] = store_sq_parse(queries + qoff[q], (size_t)(qoff[q + 1] - qoff[q]), qoff[q] - q0, chain_hash32);
    status[q] = (int8_t)pq[q].status;
    summary->by_status[pq[q].status < 0 ? 5 : pq[q].status]++;
    summary->end_messages += pq[q].status == STORE_SQ_ANSWERED || pq[q].status == STORE_SQ_FOREIGN;
    first[q + 1] = first[q] + pq[q].n;
    q_at[q] = qoff[q] - q0;
    scid_at[q] = pq[q].scid_at;
  }
  if (first[nq] >= (u64)STORE_NONE) { ctx->err = "short_channel_ids replies: too many scids"; return LAMD_ERR_ARG; }
  const size_t S = (size_t)first[nq], K = 2 * S, I1 = 3 * S + 1, MM = 5 * S + nq + 1, n_bytes = (size_t)(qoff[nq] - q0);
  summary->scids = S;
  std::vector<u8> flags(S + 1);
  for (size_t q = 0; q < nq; q++)
    if (pq[q].n) store_sq_flags(queries + qoff[q], pq[q], flags.data() + first[q]);
  lamd_ctx *L = ctx;   // queued copies read this frame's vectors: STCHK drains the stream
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  if (S) {
    STCHK(rocprim::radix_sort_keys(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, K, 0, 64, st));
    STCHK(rocprim::inclusive_scan(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, K, rocprim::plus<u32>(), st));
    if (need > tmp_bytes) tmp_bytes = need;
  }
  STCHK(rocprim::exclusive_scan(nullptr, need, (const u32 *)nullptr, (u64 *)nullptr, (u64)0, I1, rocprim::plus<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  // occ_first u64[nq + 1] | q_at, scid_at u64[nq] each | nkey, nsort, uniq u64[K] each | mscan, bscan u64[I1] each | msg_first, byte_first u64[nq + 1] each |
  // n_bytes u64[nq] | msg_off u64[MM] | occ_rec u32[3 S] | node_rec, head, npos u32[K] each | icnt, ibytes u32[I1] each | n_msgs, qlo u32[nq] each |
  // per_query u32[4 nq] | msg_rec u32[MM] | cnt u32[SQ_CNTS] | known, flags u8[S] each | status i8[nq] | the queries | (256-aligned) the sort's and the scans' workspace
  const size_t o_tmp = align_up(8 * (6 * nq + 3 + 3 * K + 2 * I1 + MM) + 4 * (3 * S + 3 * K + 2 * I1 + 6 * nq + MM + SQ_CNTS) + 2 * S + nq + n_bytes, 256);
  int rc;
  if ((rc = ensure(ctx, &ctx->store.sq, o_tmp + tmp_bytes + 16)) != LAMD_OK) return rc;
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  u64 *d_first = ctx->store.sq.as<u64>(), *d_qat = d_first + nq + 1, *d_scidat = d_qat + nq, *d_nkey = d_scidat + nq, *d_nsort = d_nkey + K, *d_uniq = d_nsort + K,
      *d_mscan = d_uniq + K, *d_bscan = d_mscan + I1, *d_mfirst = d_bscan + I1, *d_bfirst = d_mfirst + nq + 1, *d_nbytes = d_bfirst + nq + 1, *d_msgoff = d_nbytes + nq;
  u32 *d_occrec = (u32 *)(d_msgoff + MM), *d_noderec = d_occrec + 3 * S, *d_head = d_noderec + K, *d_npos = d_head + K, *d_icnt = d_npos + K, *d_ibytes = d_icnt + I1,
      *d_nmsgs = d_ibytes + I1, *d_qlo = d_nmsgs + nq, *d_perq = d_qlo + nq, *d_msgrec = d_perq + 4 * nq, *d_cnt = d_msgrec + MM;
  u8 *d_known = (u8 *)(d_cnt + SQ_CNTS), *d_flags = d_known + S, *d_queries = d_flags + S + nq;
  int8_t *d_status = (int8_t *)(d_flags + S);
  void *d_tmp = ctx->store.sq.as<u8>() + o_tmp;
  std::vector<u64> h_first(2 * (nq + 1));
  STCHK(hipMemcpyAsync(d_first, first.data(), 8 * (nq + 1), hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(d_qat, q_at.data(), 8 * nq, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(d_scidat, scid_at.data(), 8 * nq, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(d_status, status, nq, hipMemcpyHostToDevice, st));
  if (n_bytes) STCHK(hipMemcpyAsync(d_queries, queries + q0, n_bytes, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(d_cnt, 0, 4 * SQ_CNTS, st));
  const store_sq_dir dv = directory->view();
  const dim3 block(256);
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  if (S) {
    STCHK(hipMemcpyAsync(d_flags, flags.data(), S, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(d_nkey, 0xFF, 8 * K, st));
    hipLaunchKernelGGL(k_sq_lookup, dim3(blocks_for(S)), block, 0, st, (u32)S, (const u8 *)d_queries, (const u64 *)d_scidat, (const u64 *)d_first, (u32)nq,
                       (const u8 *)d_flags, dv, d_occrec, d_icnt, d_ibytes, d_known, d_nkey, d_cnt);
    STCHK(hipGetLastError());
  }
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  if (S) {
    // a stable sort of all 2 S slots: the pads (largest key) stay behind the real keys
    STCHK(rocprim::radix_sort_keys(d_tmp, tmp_bytes, (const u64 *)d_nkey, d_nsort, K, 0, 64, st));
    hipLaunchKernelGGL(k_cmp_heads, dim3(blocks_for(K)), block, 0, st, (u32)K, (const u64 *)d_nsort, (const u32 *)(d_cnt + SQ_CNT_KEYS), d_head);
    STCHK(rocprim::inclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_head, d_npos, K, rocprim::plus<u32>(), st));
    hipLaunchKernelGGL(k_cmp_merge, dim3(blocks_for(K)), block, 0, st, (u32)K, (const u64 *)d_nsort, (const u32 *)nullptr, (const u32 *)(d_cnt + SQ_CNT_KEYS),
                       (const u32 *)d_npos, d_uniq, (u32 *)nullptr);
  }
  hipLaunchKernelGGL(k_sq_nodes, dim3(blocks_for(K + 1)), block, 0, st, (u32)S, (const u64 *)d_uniq, (const u32 *)d_npos, d_cnt, dv, d_noderec, d_icnt, d_ibytes);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  STCHK(rocprim::exclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_icnt, d_mscan, (u64)0, I1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_ibytes, d_bscan, (u64)0, I1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_sq_per_query, dim3((unsigned)((nq + 3) / 4)), block, 0, st, (u32)nq, (u32)S, (const int8_t *)d_status, (const u64 *)d_first, (const u8 *)d_known,
                     (const u64 *)d_uniq, (const u32 *)d_cnt, (const u64 *)d_mscan, (const u64 *)d_bscan, d_perq, d_nmsgs, d_nbytes, d_qlo);
  hipLaunchKernelGGL(k_range_scan, dim3(1), block, 0, st, (u32)nq, (const u32 *)d_nmsgs, (const u64 *)d_nbytes, d_mfirst, d_bfirst);
  hipLaunchKernelGGL(k_sq_plan, dim3(blocks_for(3 * S + nq)), block, 0, st, (u32)S, (u32)nq, (const int8_t *)d_status, (const u64 *)d_first, (const u32 *)d_occrec,
                     (const u32 *)d_noderec, (const u64 *)d_uniq, (const u32 *)d_cnt, (const u32 *)d_qlo, (const u64 *)d_mscan, (const u64 *)d_bscan,
                     (const u64 *)d_mfirst, (const u64 *)d_bfirst, dv, d_msgoff, d_msgrec);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  STCHK(hipMemcpyAsync(h_first.data(), d_mfirst, 16 * (nq + 1), hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(per_query, d_perq, 16 * nq, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: sizes and offsets
  if (timed) STCHK(ctx->store.t_dig.read(3, summary->stage_ms));
  const u64 n_msgs = h_first[nq], total = h_first[2 * nq + 1];
  memcpy(reply_first, h_first.data(), 8 * (nq + 1));
  for (size_t q = 0; q < nq; q++) {
    summary->known += per_query[4 * q + 1];
    summary->channel_messages += per_query[4 * q + 2];
    summary->node_messages += per_query[4 * q + 3];
  }
  summary->messages = n_msgs;
  summary->bytes = total;
  const bool want_out = out || d_out;
  if (n_msgs > msg_cap) { ctx->err = "short_channel_ids replies: msg_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "short_channel_ids replies: output buffer too small"; return LAMD_ERR_ARG; }
  if (msg_off) STCHK(hipMemcpyAsync(msg_off, d_msgoff, 8 * (n_msgs + 1), hipMemcpyDeviceToHost, st));
  if (msg_rec && n_msgs) STCHK(hipMemcpyAsync(msg_rec, d_msgrec, 4 * n_msgs, hipMemcpyDeviceToHost, st));
  if (want_out && n_msgs) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.sq_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.sq_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    const store_sq_out ov{d_msgoff, d_msgrec, (u32)n_msgs, d_mfirst, (u32)nq, d_queries, d_qat, d_status};
    hipLaunchKernelGGL(k_sq_encode, dim3((unsigned)((words + 255) / 256)), block, 0, st, words, dv, ov, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_dig.record(4, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the offsets and the bytes
  if (timed && want_out && n_msgs) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_dig.ev[3], ctx->store.t_dig.ev[4]));
    summary->stage_ms[3] = ms;
  }
  return LAMD_OK;
}

// ---- the stream index of a store image (lamd_gossip_store_stream_build; per-record logic in store_stream.h).  cnt: one word per
// STORE_STREAM_* class, all 0; bytes: the streamable messages' lengths, 0.
// k_ts_flag: one lane per record and one that closes the flags: flag[n + 1], the header timestamp of every record, timestamp and length of the streamable ones
__global__ void __launch_bounds__(256) k_ts_flag(u32 n, const u8 *__restrict__ store, size_t store_len, const u64 *__restrict__ rec_off,
                                                 const int8_t *__restrict__ verdict, u32 *__restrict__ flag, u32 *__restrict__ hts, u32 *__restrict__ tts,
                                                 u32 *__restrict__ tlen, u32 *cnt, unsigned long long *bytes) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  u32 cls = STORE_STREAM_CLASSES, h = 0, ts = 0, len = 0;
  if (i < n) {
    cls = store_stream_class(store, store_len, rec_off, verdict, i, &h, &ts, &len);
    flag[i] = cls == STORE_STREAM_OK;
    hts[i] = h;
    tts[i] = ts;
    tlen[i] = len;
  } else if (i == n) {
    flag[n] = 0;
  }
  for (u32 c = 0; c < STORE_STREAM_CLASSES; c++) wave_count(&cnt[c], cls == c);
  u32 w = len;   // 64 lengths of 16 bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
  if ((threadIdx.x & 63u) == 0 && w) atomicAdd(bytes, (unsigned long long)w);
}
// k_ts_compact: one lane per record; spos: the exclusive scan of the flags
__global__ void __launch_bounds__(256) k_ts_compact(u32 n, const u32 *__restrict__ flag, const u32 *__restrict__ spos, const u32 *__restrict__ tts,
                                                    const u32 *__restrict__ tlen, u32 *__restrict__ srec, u32 *__restrict__ sts, u32 *__restrict__ slen) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const u32 k = spos[i];   // < n: at most i streamable records lie in front of record i
  srec[k] = i;
  sts[k] = tts[i];
  slen[k] = tlen[i];
}

struct lamd_store_stream {
  lamd_ctx *ctx = nullptr;
  void *mem = nullptr;          // rec_off u64[n] | spos u32[n + 1] | pmax, srec, sts, slen u32[n] each | the image, unless it is the caller's
  const u8 *img = nullptr;      // the image on the device: inside mem, or the caller's d_store
  size_t img_len = 0, n = 0, count = 0;
  u64 *rec_off = nullptr;
  u32 *spos = nullptr, *pmax = nullptr, *srec = nullptr, *sts = nullptr, *slen = nullptr;
  store_tf_index view() const { return store_tf_index{srec, sts, slen, spos, pmax, (u32)n, (u32)count}; }
};
extern "C" void lamd_store_stream_free(lamd_store_stream *s) {
  if (!s) return;
  if (s->mem) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipFree(s->mem);
  }
  delete s;
}
extern "C" size_t lamd_store_stream_count(const lamd_store_stream *s) { return s ? s->count : 0; }
extern "C" int lamd_store_stream_read(const lamd_store_stream *s, size_t cap, uint32_t *rec, uint32_t *ts, uint32_t *len) {
  if (!s) return LAMD_ERR_ARG;
  lamd_ctx *ctx = s->ctx;
  if (cap < s->count) { ctx->err = "gossip_store stream: arrays too small"; return LAMD_ERR_ARG; }
  if (s->count == 0) return LAMD_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (rec) HIPCHK(ctx, hipMemcpy(rec, s->srec, 4 * s->count, hipMemcpyDeviceToHost));
  if (ts) HIPCHK(ctx, hipMemcpy(ts, s->sts, 4 * s->count, hipMemcpyDeviceToHost));
  if (len) HIPCHK(ctx, hipMemcpy(len, s->slen, 4 * s->count, hipMemcpyDeviceToHost));
  return LAMD_OK;
}
extern "C" int lamd_gossip_store_stream_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
                                              const int8_t *verdict, lamd_store_stream **stream, lamd_store_stream_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (stream) *stream = nullptr;
  if ((!store && !d_store) || !stream || !summary || (n && !rec_off) || n >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_store_stream_summary();
  std::unique_ptr<lamd_store_stream, void (*)(lamd_store_stream *)> S(new (std::nothrow) lamd_store_stream(), lamd_store_stream_free);
  if (!S) return LAMD_ERR_NOMEM;
  S->ctx = ctx;
  S->n = n;
  S->img_len = len;
  lamd_ctx *L = ctx;   // queued copies read the caller's arrays: an error return drains the stream (drain_fail), then the index frees itself
  hipStream_t st = ctx->stream;
  const size_t o_img = 8 * n + 4 * (5 * n + 2);
  hipError_t e0 = hipSetDevice(ctx->device);
  if (e0 == hipSuccess) e0 = hipMalloc(&S->mem, o_img + (d_store ? 0 : len) + 16);
  if (e0 != hipSuccess) {
    ctx->err = std::string("gossip_store stream: ") + hipGetErrorString(e0);
    return drain_fail(ctx, L, e0 == hipErrorOutOfMemory ? LAMD_ERR_NOMEM : LAMD_ERR_HIP);
  }
  S->rec_off = (u64 *)S->mem;
  S->spos = (u32 *)(S->rec_off + n);
  S->pmax = S->spos + n + 1;
  S->srec = S->pmax + n;
  S->sts = S->srec + n;
  S->slen = S->sts + n;
  S->img = d_store ? (const u8 *)d_store : (const u8 *)S->mem + o_img;
  if (n == 0) {   // an empty list: spos[0] = 0 is all a walk reads
    STCHK(hipMemsetAsync(S->spos, 0, 4, st));
    STCHK(hipStreamSynchronize(st));
    *stream = S.release();
    return LAMD_OK;
  }
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::exclusive_scan(nullptr, tmp_bytes, (const u32 *)nullptr, (u32 *)nullptr, (u32)0, n + 1, rocprim::plus<u32>(), st));
  STCHK(rocprim::inclusive_scan(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, n, rocprim::maximum<u32>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  // bytes u64 | cnt u32[8] | flag u32[n + 1] | hts, tts, tlen u32[n] each | verdict i8[n] | (256-aligned) the scans' workspace
  const size_t o_tmp = align_up(8 + 32 + 4 * (4 * n + 1) + n, 256);
  int rc;
  if ((rc = ensure(ctx, &ctx->store.ts, o_tmp + tmp_bytes + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  unsigned long long *d_bytes = ctx->store.ts.as<unsigned long long>();
  u32 *d_cnt = (u32 *)(d_bytes + 1), *d_flag = d_cnt + 8, *d_hts = d_flag + n + 1, *d_tts = d_hts + n, *d_tlen = d_tts + n;
  int8_t *d_verdict = verdict ? (int8_t *)(d_tlen + n) : nullptr;
  void *d_tmp = ctx->store.ts.as<u8>() + o_tmp;
  const u8 *img = S->img;
  if (!d_store) STCHK(hipMemcpyAsync((void *)img, store, len, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(S->rec_off, rec_off, 8 * n, hipMemcpyHostToDevice, st));
  if (verdict) STCHK(hipMemcpyAsync(d_verdict, verdict, n, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(d_bytes, 0, 8 + 32, st));
  const dim3 block(256);
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  hipLaunchKernelGGL(k_ts_flag, dim3(blocks_for(n + 1)), block, 0, st, (u32)n, img, len, (const u64 *)S->rec_off, (const int8_t *)d_verdict, d_flag, d_hts, d_tts, d_tlen,
                     d_cnt, d_bytes);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  STCHK(rocprim::exclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_flag, S->spos, (u32)0, n + 1, rocprim::plus<u32>(), st));
  STCHK(rocprim::inclusive_scan(d_tmp, tmp_bytes, (const u32 *)d_hts, S->pmax, n, rocprim::maximum<u32>(), st));
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  hipLaunchKernelGGL(k_ts_compact, dim3(blocks_for(n)), block, 0, st, (u32)n, (const u32 *)d_flag, (const u32 *)S->spos, (const u32 *)d_tts, (const u32 *)d_tlen, S->srec,
                     S->sts, S->slen);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  struct { unsigned long long bytes; u32 cnt[8]; } h = {};
  static_assert(sizeof h == 40, "bytes, then the counters");
  STCHK(hipMemcpyAsync(&h, d_bytes, sizeof h, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  if (timed) STCHK(ctx->store.t_dig.read(3, summary->stage_ms));
  S->count = h.cnt[STORE_STREAM_OK];
  summary->streamable = h.cnt[STORE_STREAM_OK];
  summary->skipped_deleted = h.cnt[STORE_STREAM_DELETED];
  summary->skipped_dying = h.cnt[STORE_STREAM_DYING];
  summary->skipped_type = h.cnt[STORE_STREAM_TYPE];
  summary->skipped_verdict = h.cnt[STORE_STREAM_VERDICT];
  summary->skipped_frame = h.cnt[STORE_STREAM_FRAME];
  summary->bytes = h.bytes;
  *stream = S.release();
  return LAMD_OK;
}

// ---- gossip_timestamp_filter answers (lamd_timestamp_filter_reply_batch; per-peer and per-tile logic in store_stream.h).
// k_tf_select: ONE WAVE per peer, in a workgroup of its own.  WRITE false: the counting pass leaves n_msgs, n_bytes, cursor_out, done.
// WRITE true: the same tiles again; the taken entries go to msg_rec / msg_off behind msg_first[p] / byte_first[p] (below n_total, which
// the counting pass found), the last peer's wave closes msg_off with the total.
template <bool WRITE>
__global__ void __launch_bounds__(64) k_tf_select(u32 np, const store_tf_peer *__restrict__ peers, u32 now, store_tf_index x, u32 *__restrict__ n_msgs,
                                                  u64 *__restrict__ n_bytes, u64 *__restrict__ cursor_out, u8 *__restrict__ done,
                                                  const u64 *__restrict__ msg_first, const u64 *__restrict__ byte_first, u64 n_total,
                                                  u64 *__restrict__ msg_off, u32 *__restrict__ msg_rec) {
  const u32 p = blockIdx.x, lane = threadIdx.x;
  if (p >= np) return;   // (the whole wave)
  const store_tf_peer pe = peers[p];
  if (WRITE && p == np - 1 && lane == 0) msg_off[n_total] = byte_first[np];
  u64 cur = pe.cursor, bytes = 0;
  u32 msgs = 0, fin = 0;
  if (pe.status == STORE_TF_STREAMED) {
    cur = store_tf_start(x, pe, now);
    if (cur > x.n_stream) cur = x.n_stream;   // (never: the host checked the cursors)
    if (pe.budget >= 0) {
      const u64 m0 = WRITE ? msg_first[p] : 0, b0 = WRITE ? byte_first[p] : 0;
      // cur, bytes, msgs and every branch below are uniform across the wave.  The loads of the next tile are issued in front of the work on
      // this one, and a tile nothing of which passes costs a ballot: a narrow filter walks a long list at the speed of its loads.
      u64 k = cur + lane;
      bool in = k < x.n_stream;
      u32 ts = in ? x.sts[k] : 0, len = in ? x.slen[k] : 0;
      for (;;) {
        if (cur >= x.n_stream) { cur = x.n_stream; fin = 1; break; }
        const u64 k_next = k + 64;
        const bool in_next = k_next < x.n_stream;
        const u32 ts_next = in_next ? x.sts[k_next] : 0, len_next = in_next ? x.slen[k_next] : 0;
        const bool pass = in && store_tf_pass(ts, pe.min, pe.max);
        const u64 pm = __ballot(pass);
        if (pm) {
          u32 incl = pass ? len : 0;   // 64 lengths of 16 bits
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const u32 t = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += t;
          }
          const u64 sm = __ballot(store_tf_stops(pass, bytes, incl, pe.budget)), take = store_tf_taken(pm, sm);
          if (WRITE && ((take >> lane) & 1)) {
            const u64 slot = m0 + msgs + (u32)__popcll(take & ((1ull << lane) - 1ull));
            if (slot < n_total) {
              msg_rec[slot] = x.srec[k];
              msg_off[slot] = b0 + bytes + incl - len;
            }
          }
          msgs += (u32)__popcll(take);
          const u32 last = sm ? store_tf_first_lane(sm) : 63u;
          bytes += (u32)__builtin_amdgcn_readfirstlane((int)__shfl(incl, (int)last, 64));
          if (sm) { cur += last + 1; break; }
        }
        cur += 64;
        k = k_next;
        in = in_next;
        ts = ts_next;
        len = len_next;
      }
    }
  }
  if (!WRITE && lane == 0) {
    n_msgs[p] = msgs;
    n_bytes[p] = bytes;
    cursor_out[p] = cur;
    done[p] = (u8)fin;
  }
}

extern "C" int lamd_timestamp_filter_reply_batch(lamd_ctx *ctx, const lamd_store_stream *stream, const uint8_t *chain_hash32, uint32_t now, size_t np,
                                                 const uint8_t *filters, const uint64_t *foff, const uint64_t *cursor_in, const int64_t *budget, int8_t *status,
                                                 uint64_t *cursor_out, uint8_t *done, uint64_t *reply_first, size_t msg_cap, uint64_t *msg_off,
                                                 uint32_t *msg_rec, uint8_t *out, void *d_out, size_t out_cap, lamd_filter_reply_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!stream || stream->ctx != ctx || !chain_hash32 || !summary || !reply_first || (np && (!filters || !foff || !status || !cursor_out || !done)) ||
      (msg_cap && !msg_off) || np >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_filter_reply_summary();
  reply_first[0] = 0;
  if (np == 0) {
    if (msg_cap) msg_off[0] = 0;
    return LAMD_OK;
  }
  // the framing, on the host: status, bounds and start rule of every peer
  std::vector<store_tf_peer> peers(np);
  for (size_t p = 0; p < np; p++) {
    if (foff[p + 1] < foff[p]) { ctx->err = "timestamp filter replies: decreasing filter offsets"; return LAMD_ERR_ARG; }
    const u64 c = cursor_in ? cursor_in[p] : STORE_TF_AS_FILTER;
    if (c != STORE_TF_AS_FILTER && c > stream->count) { ctx->err = "timestamp filter replies: a cursor behind the end of the list"; return LAMD_ERR_ARG; }
    const store_tf_filter f = store_tf_parse(filters + foff[p], (size_t)(foff[p + 1] - foff[p]), chain_hash32);
    peers[p] = store_tf_peer{f.status, f.min, f.max, f.rule, c, budget ? budget[p] : INT64_MAX};
  }
  for (size_t p = 0; p < np; p++) {
    status[p] = (int8_t)peers[p].status;
    summary->by_status[peers[p].status < 0 ? 2 : peers[p].status]++;
  }
  lamd_ctx *L = ctx;   // queued copies read this frame's vectors: STCHK drains the stream
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // peers store_tf_peer[np] | n_bytes u64[np] | msg_first, byte_first u64[np + 1] each | cursor_out u64[np] | n_msgs u32[np] | done u8[np]
  static_assert(sizeof(store_tf_peer) == 32, "the peers lie in front of 8-byte words");
  int rc;
  if ((rc = ensure(ctx, &ctx->store.ts, 32 * np + 8 * (4 * np + 2) + 4 * np + np + 16)) != LAMD_OK) return rc;
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_dig.create());
  store_tf_peer *d_peers = ctx->store.ts.as<store_tf_peer>();
  u64 *d_nbytes = (u64 *)(d_peers + np), *d_mfirst = d_nbytes + np, *d_bfirst = d_mfirst + np + 1, *d_cur = d_bfirst + np + 1;
  u32 *d_nmsgs = (u32 *)(d_cur + np);
  u8 *d_done = (u8 *)(d_nmsgs + np);
  std::vector<u64> h_first(2 * (np + 1));
  STCHK(hipMemcpyAsync(d_peers, peers.data(), 32 * np, hipMemcpyHostToDevice, st));
  const store_tf_index xv = stream->view();
  const dim3 wave(64), grid((unsigned)np);
  if (timed) STCHK(ctx->store.t_dig.record(0, st));
  hipLaunchKernelGGL(k_tf_select<false>, grid, wave, 0, st, (u32)np, (const store_tf_peer *)d_peers, now, xv, d_nmsgs, d_nbytes, d_cur, d_done, (const u64 *)nullptr,
                     (const u64 *)nullptr, (u64)0, (u64 *)nullptr, (u32 *)nullptr);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(1, st));
  hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(256), 0, st, (u32)np, (const u32 *)d_nmsgs, (const u64 *)d_nbytes, d_mfirst, d_bfirst);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(2, st));
  STCHK(hipMemcpyAsync(h_first.data(), d_mfirst, 16 * (np + 1), hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(cursor_out, d_cur, 8 * np, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(done, d_done, np, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: sizes, cursors and done flags
  if (timed) STCHK(ctx->store.t_dig.read(2, summary->stage_ms));
  const u64 n_msgs = h_first[np], total = h_first[2 * np + 1];
  memcpy(reply_first, h_first.data(), 8 * (np + 1));
  for (size_t p = 0; p < np; p++) summary->finished += done[p];
  summary->messages = n_msgs;
  summary->bytes = total;
  const bool want_out = out || d_out;
  if (n_msgs >= (u64)STORE_NONE) { ctx->err = "timestamp filter replies: too many messages for one call"; return LAMD_ERR_ARG; }
  if (n_msgs > msg_cap) { ctx->err = "timestamp filter replies: msg_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "timestamp filter replies: output buffer too small"; return LAMD_ERR_ARG; }
  if (!msg_off && !(want_out && n_msgs)) return LAMD_OK;
  // msg_off u64[n_msgs + 1] | msg_rec u32[n_msgs]
  if ((rc = ensure(ctx, &ctx->store.ts_msg, 12 * n_msgs + 8 + 16)) != LAMD_OK) return rc;
  u64 *d_msgoff = ctx->store.ts_msg.as<u64>();
  u32 *d_msgrec = (u32 *)(d_msgoff + n_msgs + 1);
  if (timed) STCHK(ctx->store.t_dig.record(3, st));
  hipLaunchKernelGGL(k_tf_select<true>, grid, wave, 0, st, (u32)np, (const store_tf_peer *)d_peers, now, xv, (u32 *)nullptr, (u64 *)nullptr, (u64 *)nullptr, (u8 *)nullptr,
                     (const u64 *)d_mfirst, (const u64 *)d_bfirst, n_msgs, d_msgoff, d_msgrec);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_dig.record(4, st));
  if (msg_off) STCHK(hipMemcpyAsync(msg_off, d_msgoff, 8 * (n_msgs + 1), hipMemcpyDeviceToHost, st));
  if (msg_rec && n_msgs) STCHK(hipMemcpyAsync(msg_rec, d_msgrec, 4 * n_msgs, hipMemcpyDeviceToHost, st));
  if (want_out && n_msgs) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.ts_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.ts_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    // every message is the copy of a record: the encoder of the short_channel_ids replies, with a directory that holds the image alone
    const store_sq_dir dv{stream->img, stream->img_len, stream->rec_off, (u32)stream->n, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0};
    const store_sq_out ov{d_msgoff, d_msgrec, (u32)n_msgs, d_mfirst, (u32)np, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_sq_encode, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, words, dv, ov, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_dig.record(5, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the offsets and the bytes
  if (timed) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_dig.ev[3], ctx->store.t_dig.ev[4]));
    summary->stage_ms[2] = ms;
    if (want_out && n_msgs) {
      STCHK(hipEventElapsedTime(&ms, ctx->store.t_dig.ev[4], ctx->store.t_dig.ev[5]));
      summary->stage_ms[3] = ms;
    }
  }
  return LAMD_OK;
}

// ---- channel_update reception (lamd_channel_update_receive_batch; per-message, per-row and per-word logic in store_receive.h).  One lane per
// message, per sorted position or per output word; each stage reads what the one before it wrote, so each is a launch of its own.
// cnt: RX_CNT_* words, all 0.
enum { RX_CNT_ROWS = 0, RX_CNT_DELS = 1, RX_CNTS = 4 };
// k_rx_classify: statuses -1 .. 3, the two bisections, the signer; the PENDING messages get consecutive signature rows with one atomic per
// wave (in any order: row_msg / row_of tie a row to its message).  rowbase: the identity, one row per span.  start / len: preset to 0 -- the
// rows behind the last real one are empty spans: nothing is read through them, their rows of the signature batch are all-zero and fail.
__global__ void __launch_bounds__(256) k_rx_classify(store_rx_view v, store_rx_params p, store_rx_batch b, int8_t *__restrict__ status, u32 *__restrict__ chan,
                                                     u32 *__restrict__ ts, u8 *__restrict__ aux, u32 *__restrict__ row_of, u64 *__restrict__ start,
                                                     u64 *__restrict__ len, u8 *__restrict__ ids33, u32 *__restrict__ row_msg, u64 *__restrict__ rowbase, u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  store_rx_msg r;
  r.status = STORE_RX_MALFORMED;
  if (i < b.n) {
    r = store_rx_classify(v, p, b, i);
    status[i] = (int8_t)r.status;
    chan[i] = r.chan;
    ts[i] = r.ts;
    aux[i] = (u8)(r.dir | (r.dont_forward << 1));
    rowbase[i] = i;
    if (i == b.n - 1) rowbase[b.n] = b.n;
  }
  const bool pending = i < b.n && r.status == STORE_RX_PENDING;
  const u32 row = wave_alloc(&cnt[RX_CNT_ROWS], pending);
  if (i < b.n) row_of[i] = pending ? row : STORE_NONE;
  if (pending && row < b.n) store_rx_row(v, b, r, i, row, start, len, ids33, row_msg);
}
__global__ void __launch_bounds__(256) k_rx_settle(u32 n, int8_t *__restrict__ status, u8 *__restrict__ flags, const u32 *__restrict__ chan,
                                                   const u8 *__restrict__ aux, const u32 *__restrict__ row_of, const int8_t *__restrict__ sigv,
                                                   u64 *__restrict__ key, u32 *__restrict__ val) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = store_rx_settle(status, flags, chan, aux, row_of, sigv, i);
  val[i] = i;
}
__global__ void __launch_bounds__(256) k_rx_items(u32 n, const u64 *__restrict__ key, const u32 *__restrict__ val, const u32 *__restrict__ ts,
                                                  u64 *__restrict__ item) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) item[p] = store_rx_item(key, val, ts, p);
}
__global__ void __launch_bounds__(256) k_rx_resolve(store_rx_view v, store_rx_params pr, store_rx_batch b, store_rx_sorted s, const u32 *__restrict__ ts,
                                                    int8_t *status, u8 *flags, store_rx_marks k, u32 *cnt) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  const bool deletes = p < s.n && store_rx_resolve(v, pr, b, s, ts, p, status, flags, k);
  wave_count(&cnt[RX_CNT_DELS], deletes);
}
// k_rx_plan: where each accepted message's record goes, and the re-stamped announcements with their checksums.  The CRC tables as in k_store_crc.
__global__ void __launch_bounds__(256) k_rx_plan(u32 n, store_rx_view v, const int8_t *__restrict__ status, const u8 *__restrict__ flags,
                                                 const u32 *__restrict__ chan, const u32 *__restrict__ ts, const u64 *__restrict__ apos,
                                                 const u64 *__restrict__ abyte, const u64 *__restrict__ spos, store_rx_plan_out o) {
  __shared__ u32 T[4 * 256];
  block_crc_tables<4>(T);
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_rx_plan<4>(T, v, status, flags, chan, ts, apos, abyte, spos, o, i);
}
// k_rx_encode: one lane per added record writes its 12-byte header; k_rx_copy: one aligned 32-bit word of the output per lane
__global__ void __launch_bounds__(256) k_rx_encode(u32 adds, store_rx_batch b, const u32 *__restrict__ add_msg, const u8 *__restrict__ flags,
                                                   const u32 *__restrict__ ts, u8 *__restrict__ hdr) {
  __shared__ u32 T[4 * 256];
  block_crc_tables<4>(T);
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j < adds) store_rx_header<4>(T, b, flags, ts, add_msg[j], hdr + STORE_HDR * (size_t)j);
}
__global__ void __launch_bounds__(256) k_rx_copy(u64 words, store_rx_out o, u8 *__restrict__ out, u64 total) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k < words) store_rx_word(o, out, total, (u32)((uintptr_t)out & 3), k);
}

// the workspace of one call, carved out of store.rx: with base == nullptr the same walk gives its size
struct rx_ws {
  u64 *off, *start, *len, *rowbase, *key, *skey, *item, *run, *apos, *abyte, *spos, *add_off, *held;
  u32 *chan, *ts, *row_of, *row_msg, *val, *sval, *acnt, *abytes, *scnt, *del_key, *del_sorted, *add_msg, *set_rec, *set_ts, *set_crc, *cnt;
  int8_t *status, *sigv;
  u8 *flags, *aux, *ids33, *hdr, *msgs, *peers, *tmp;
  size_t bytes;
  rx_ws(u8 *base, size_t n, size_t n_held, size_t msg_bytes, size_t peer_bytes, size_t tmp_bytes) {
    size_t at = 0;
    auto take = [&](auto **p, size_t count) {
      using T = std::remove_reference_t<decltype(**p)>;
      *p = base ? (T *)(base + at) : nullptr;
      at += sizeof(T) * count;
    };
    take(&off, n + 1); take(&start, n); take(&len, n); take(&rowbase, n + 1); take(&key, n); take(&skey, n); take(&item, n); take(&run, n);
    take(&apos, n + 1); take(&abyte, n + 1); take(&spos, n + 1); take(&add_off, n + 1); take(&held, n_held);
    take(&chan, n); take(&ts, n); take(&row_of, n); take(&row_msg, n); take(&val, n); take(&sval, n);
    take(&acnt, n + 1); take(&abytes, n + 1); take(&scnt, n + 1);   // (one memset clears the three)
    take(&del_key, n); take(&del_sorted, n); take(&add_msg, n); take(&set_rec, n); take(&set_ts, n); take(&set_crc, n); take(&cnt, RX_CNTS);
    take(&status, n); take(&sigv, n); take(&flags, n); take(&aux, n); take(&ids33, 33 * n); take(&hdr, STORE_HDR * n); take(&msgs, msg_bytes + 1);
    take(&peers, peer_bytes);
    at = align_up(at, 256);
    take(&tmp, tmp_bytes);
    bytes = at + 16;
  }
};

extern "C" int lamd_channel_update_receive_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const lamd_store_directory *directory,
                                                 const uint8_t *chain_hash32, uint64_t now, uint32_t prune_interval, const uint8_t *our_id33, size_t n,
                                                 const uint8_t *msgs, const uint64_t *off, const uint8_t *source_peers33, size_t peer_stride, size_t n_held,
                                                 const uint64_t *held_scid, int8_t *status, uint8_t *flags, uint32_t *chan, size_t add_cap, uint32_t *add_msg,
                                                 uint64_t *add_off, uint8_t *out, void *d_out, size_t out_cap, size_t edit_cap, uint32_t *del_rec,
                                                 uint32_t *set_rec, uint32_t *set_ts, uint32_t *set_crc, lamd_update_receive_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!digest || !directory || !chain_hash32 || !summary || (n && (!msgs || !off || !status || !flags || !chan)) || (add_cap && (!add_msg || !add_off)) ||
      (edit_cap && (!del_rec || !set_rec || !set_ts || !set_crc)) || (n_held && !held_scid) || (source_peers33 && peer_stride && peer_stride < 33) ||
      n >= (size_t)STORE_NONE / 2 || n_held >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  // the digest and the directory of ONE image, built by this context (as lamd_gossip_store_directory_build checks its digest)
  if (digest->ctx != ctx || directory->ctx != ctx || directory->n != digest->cap || directory->count != digest->count || directory->nbare != digest->nbare) {
    ctx->err = "channel_update receive: the digest and the directory do not belong to this context and to one image";
    return LAMD_ERR_ARG;
  }
  if ((u64)directory->count + directory->nbare >= STORE_RX_MAX_CHANNELS) { ctx->err = "channel_update receive: too many channels"; return LAMD_ERR_ARG; }
  *summary = lamd_update_receive_summary();
  if (n == 0) return LAMD_OK;
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) { ctx->err = "channel_update receive: decreasing message offsets"; return LAMD_ERR_ARG; }
  for (size_t k = 1; k < n_held; k++)
    if (held_scid[k] <= held_scid[k - 1]) { ctx->err = "channel_update receive: held_scid is not ascending"; return LAMD_ERR_ARG; }
  const size_t msg_bytes = (size_t)(off[n] - off[0]), peer_bytes = source_peers33 ? (n - 1) * peer_stride + 33 : 0;
  std::vector<u64> rel(n + 1);   // a queued copy reads it: STCHK drains the stream
  for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
  store_rx_params pr;
  pr.now = now;
  pr.prune = prune_interval ? prune_interval : 1209600;
  pr.have_our = our_id33 != nullptr;
  memcpy(pr.chain, chain_hash32, 32);
  memset(pr.our_id, 0, 33);
  if (our_id33) memcpy(pr.our_id, our_id33, 33);
  lamd_ctx *L = ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 32, st));
  STCHK(rocprim::radix_sort_keys(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 32, st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::inclusive_scan(nullptr, need, (const u64 *)nullptr, (u64 *)nullptr, n, rocprim::maximum<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::exclusive_scan(nullptr, need, (const u32 *)nullptr, (u64 *)nullptr, (u64)0, n + 1, rocprim::plus<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  int rc;
  if ((rc = ensure(ctx, &ctx->store.rx, rx_ws(nullptr, n, n_held, msg_bytes, peer_bytes, tmp_bytes).bytes)) != LAMD_OK) return rc;
  const rx_ws w(ctx->store.rx.as<u8>(), n, n_held, msg_bytes, peer_bytes, tmp_bytes);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_rx.create());
  STCHK(hipMemcpyAsync(w.off, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
  if (msg_bytes) STCHK(hipMemcpyAsync(w.msgs, msgs + off[0], msg_bytes, hipMemcpyHostToDevice, st));
  if (peer_bytes) STCHK(hipMemcpyAsync(w.peers, source_peers33, peer_bytes, hipMemcpyHostToDevice, st));
  if (n_held) STCHK(hipMemcpyAsync(w.held, held_scid, 8 * n_held, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(w.start, 0, 16 * n, st));                  // start, len
  STCHK(hipMemsetAsync(w.acnt, 0, 12 * (n + 1), st));             // acnt, abytes, scnt
  STCHK(hipMemsetAsync(w.del_key, 0xFF, 4 * n, st));
  STCHK(hipMemsetAsync(w.cnt, 0, 4 * RX_CNTS, st));
  STCHK(hipMemsetAsync(w.flags, 0, n, st));
  const store_rx_view v{directory->img, directory->img_len, directory->rec_off, (u32)directory->n, directory->scid, (u32)directory->count, (u32)directory->nbare,
                        directory->ent_rec, directory->bare_rec, digest->ts};
  const store_rx_batch b{w.msgs, w.off, (u32)n, peer_bytes ? w.peers : nullptr, (u64)peer_stride, w.held, (u32)n_held};
  const dim3 grid(blocks_for(n)), block(256);
  if (timed) STCHK(ctx->store.t_rx.record(0, st));
  hipLaunchKernelGGL(k_rx_classify, grid, block, 0, st, v, pr, b, w.status, w.chan, w.ts, w.aux, w.row_of, w.start, w.len, w.ids33, w.row_msg, w.rowbase, w.cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(1, st));
  // ONE signature batch over n spans: the real rows in front, empty spans behind them (the host does not wait for their number)
  if ((rc = gossip_device(ctx, n, w.msgs, w.start, w.ids33, w.rowbase, n, w.sigv, w.len)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (timed) STCHK(ctx->store.t_rx.record(2, st));
  hipLaunchKernelGGL(k_rx_settle, grid, block, 0, st, (u32)n, w.status, w.flags, (const u32 *)w.chan, (const u8 *)w.aux, (const u32 *)w.row_of,
                     (const int8_t *)w.sigv, w.key, w.val);
  // stable: arrival order inside a slot; the slots need 31 bits, the pads (all ones) end behind them
  STCHK(rocprim::radix_sort_pairs(w.tmp, tmp_bytes, (const u64 *)w.key, w.skey, (const u32 *)w.val, w.sval, n, 0, 32, st));
  hipLaunchKernelGGL(k_rx_items, grid, block, 0, st, (u32)n, (const u64 *)w.skey, (const u32 *)w.sval, (const u32 *)w.ts, w.item);
  STCHK(rocprim::inclusive_scan(w.tmp, tmp_bytes, (const u64 *)w.item, w.run, n, rocprim::maximum<u64>(), st));
  hipLaunchKernelGGL(k_rx_resolve, grid, block, 0, st, v, pr, b, store_rx_sorted{w.skey, w.sval, w.run, (u32)n}, (const u32 *)w.ts, w.status, w.flags,
                     store_rx_marks{w.acnt, w.abytes, w.scnt, w.del_key}, w.cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(3, st));
  STCHK(rocprim::radix_sort_keys(w.tmp, tmp_bytes, (const u32 *)w.del_key, w.del_sorted, n, 0, 32, st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.acnt, w.apos, (u64)0, n + 1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.abytes, w.abyte, (u64)0, n + 1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.scnt, w.spos, (u64)0, n + 1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_rx_plan, grid, block, 0, st, (u32)n, v, (const int8_t *)w.status, (const u8 *)w.flags, (const u32 *)w.chan, (const u32 *)w.ts,
                     (const u64 *)w.apos, (const u64 *)w.abyte, (const u64 *)w.spos, store_rx_plan_out{(u64)n, (u64)n, w.add_msg, w.add_off, w.set_rec, w.set_ts, w.set_crc});
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(4, st));
  u64 totals[3] = {0, 0, 0};
  u32 cnt[RX_CNTS] = {};
  STCHK(hipMemcpyAsync(status, w.status, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(flags, w.flags, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(chan, w.chan, 4 * n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[0], w.apos + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[1], w.abyte + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[2], w.spos + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(cnt, w.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: verdicts and sizes
  if (timed) STCHK(ctx->store.t_rx.read(4, summary->stage_ms));
  for (size_t i = 0; i < n; i++) {
    summary->by_status[status[i] < 0 ? 10 : status[i] <= 9 ? status[i] : 10]++;
    summary->superseded += (flags[i] & STORE_RX_SUPERSEDED) != 0;
  }
  const u64 adds = totals[0], total = totals[1], sets = totals[2], dels = cnt[RX_CNT_DELS];
  summary->accepted = summary->adds = adds;
  summary->bytes = total;
  summary->deletions = dels;
  summary->retimestamps = sets;
  summary->signature_rows = cnt[RX_CNT_ROWS];
  const bool want_out = out || d_out;
  if (adds > add_cap) { ctx->err = "channel_update receive: add_msg / add_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "channel_update receive: output buffer too small"; return LAMD_ERR_ARG; }
  if (dels > edit_cap || sets > edit_cap) { ctx->err = "channel_update receive: the edit lists are too small"; return LAMD_ERR_ARG; }
  if (adds) {
    STCHK(hipMemcpyAsync(add_msg, w.add_msg, 4 * adds, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(add_off, w.add_off, 8 * adds, hipMemcpyDeviceToHost, st));
  }
  if (dels) STCHK(hipMemcpyAsync(del_rec, w.del_sorted, 4 * dels, hipMemcpyDeviceToHost, st));
  if (sets) {
    STCHK(hipMemcpyAsync(set_rec, w.set_rec, 4 * sets, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(set_ts, w.set_ts, 4 * sets, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(set_crc, w.set_crc, 4 * sets, hipMemcpyDeviceToHost, st));
  }
  const bool encode = want_out && adds;
  if (encode) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.rx_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.rx_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    if (timed) STCHK(ctx->store.t_rx.record(5, st));
    hipLaunchKernelGGL(k_rx_encode, dim3(blocks_for(adds)), block, 0, st, (u32)adds, b, (const u32 *)w.add_msg, (const u8 *)w.flags, (const u32 *)w.ts, w.hdr);
    hipLaunchKernelGGL(k_rx_copy, dim3((unsigned)((words + 255) / 256)), block, 0, st, words,
                       store_rx_out{w.add_off, w.add_msg, (u32)adds, w.hdr, w.msgs, w.off}, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_rx.record(6, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the lists and the bytes
  if (timed && encode) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_rx.ev[5], ctx->store.t_rx.ev[6]));
    summary->stage_ms[4] = ms;
  }
  return LAMD_OK;
}

// ---- node_announcement reception (lamd_node_announcement_receive_batch; per-channel, per-message and per-row logic in store_nodes.h).  One
// lane per channel, per message, per sorted position or per output word; each stage reads what the one before it wrote, so each is a launch
// of its own.  The scan items, the record headers and the output words are k_rx_items', k_rx_encode's and k_rx_copy's.  cnt: RX_CNT_* words, all 0.
// k_nr_alive: alive, one byte per node, all 0: every channel that is not dying stores a 1 for both of its nodes
__global__ void __launch_bounds__(256) k_nr_alive(store_nr_view v, u8 *alive) {
  const u32 c = blockIdx.x * 256 + threadIdx.x;
  if (c < v.count + v.nbare) store_nr_alive(v, c, alive);
}
// k_nr_classify: statuses -1 and 1, the bisection in the ranked ids, the timestamp; the PENDING messages get consecutive signature rows with
// one atomic per wave, as k_rx_classify's.  start / len: preset to 0 -- the rows behind the last real one are empty spans.
__global__ void __launch_bounds__(256) k_nr_classify(store_nr_view v, store_nr_batch b, int8_t *__restrict__ status, u32 *__restrict__ node, u32 *__restrict__ ts,
                                                     u32 *__restrict__ row_of, u64 *__restrict__ start, u64 *__restrict__ len, u32 *__restrict__ row_msg,
                                                     u64 *__restrict__ rowbase, u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  store_nr_msg r;
  r.status = STORE_NR_MALFORMED;
  if (i < b.n) {
    r = store_nr_classify(v, b, i);
    status[i] = (int8_t)r.status;
    node[i] = r.node;
    ts[i] = r.ts;
    rowbase[i] = i;
    if (i == b.n - 1) rowbase[b.n] = b.n;
  }
  const bool pending = i < b.n && r.status == STORE_NR_PENDING;
  const u32 row = wave_alloc(&cnt[RX_CNT_ROWS], pending);
  if (i < b.n) row_of[i] = pending ? row : STORE_NONE;
  if (pending && row < b.n) store_nr_row(b, i, row, start, len, row_msg);
}
__global__ void __launch_bounds__(256) k_nr_settle(u32 n, u32 pending, int8_t *__restrict__ status, u32 *__restrict__ node, const u32 *__restrict__ row_of,
                                                   const int8_t *__restrict__ sigv, u64 *__restrict__ key, u32 *__restrict__ val) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  key[i] = store_nr_settle(status, node, row_of, sigv, pending, i);
  val[i] = i;
}
__global__ void __launch_bounds__(256) k_nr_resolve(store_nr_view v, store_nr_batch b, store_rx_sorted s, const u32 *__restrict__ ts,
                                                    const u8 *__restrict__ alive, int8_t *status, u8 *flags, store_nr_marks k, u32 *cnt) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  const bool deletes = p < s.n && store_nr_resolve(v, b, s, ts, alive, p, status, flags, k);
  wave_count(&cnt[RX_CNT_DELS], deletes);
}
__global__ void __launch_bounds__(256) k_nr_plan(u32 n, const int8_t *__restrict__ status, const u64 *__restrict__ apos, const u64 *__restrict__ abyte,
                                                 u64 add_cap, u32 *__restrict__ add_msg, u64 *__restrict__ add_off) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) store_nr_plan(status, apos, abyte, add_cap, add_msg, add_off, i);
}

// the workspace of one call, carved out of store.rx (the two receive calls of a context run one behind the other): with base == nullptr the
// same walk gives its size
struct nr_ws {
  u64 *off, *start, *len, *rowbase, *key, *skey, *item, *run, *apos, *abyte, *add_off;
  u32 *node, *ts, *row_of, *row_msg, *val, *sval, *acnt, *abytes, *del_key, *del_sorted, *add_msg, *cnt;
  int8_t *status, *sigv;
  u8 *flags, *alive, *hdr, *msgs, *tmp;
  size_t bytes;
  nr_ws(u8 *base, size_t n, size_t nodes, size_t msg_bytes, size_t tmp_bytes) {
    size_t at = 0;
    auto take = [&](auto **p, size_t count) {
      using T = std::remove_reference_t<decltype(**p)>;
      *p = base ? (T *)(base + at) : nullptr;
      at += sizeof(T) * count;
    };
    take(&off, n + 1); take(&start, n); take(&len, n); take(&rowbase, n + 1); take(&key, n); take(&skey, n); take(&item, n); take(&run, n);
    take(&apos, n + 1); take(&abyte, n + 1); take(&add_off, n + 1);
    take(&node, n); take(&ts, n); take(&row_of, n); take(&row_msg, n); take(&val, n); take(&sval, n);
    take(&acnt, n + 1); take(&abytes, n + 1);   // (one memset clears the two)
    take(&del_key, n); take(&del_sorted, n); take(&add_msg, n); take(&cnt, RX_CNTS);
    take(&status, n); take(&sigv, n); take(&flags, n); take(&alive, nodes + 1); take(&hdr, STORE_HDR * n); take(&msgs, msg_bytes + 1);
    at = align_up(at, 256);
    take(&tmp, tmp_bytes);
    bytes = at + 16;
  }
};

extern "C" int lamd_node_announcement_receive_batch(lamd_ctx *ctx, const lamd_store_directory *directory, size_t n, const uint8_t *msgs, const uint64_t *off,
                                                    int announcements_pending, int8_t *status, uint8_t *flags, uint32_t *node, size_t add_cap,
                                                    uint32_t *add_msg, uint64_t *add_off, uint8_t *out, void *d_out, size_t out_cap, size_t edit_cap,
                                                    uint32_t *del_rec, lamd_node_receive_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!directory || !summary || (n && (!msgs || !off || !status || !flags || !node)) || (add_cap && (!add_msg || !add_off)) || (edit_cap && !del_rec) ||
      n >= (size_t)STORE_NONE / 2) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  if (directory->ctx != ctx) { ctx->err = "node_announcement receive: the directory does not belong to this context"; return LAMD_ERR_ARG; }
  if ((u64)directory->nodes >= STORE_NR_MAX_NODES) { ctx->err = "node_announcement receive: too many nodes"; return LAMD_ERR_ARG; }
  *summary = lamd_node_receive_summary();
  if (n == 0) return LAMD_OK;
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) { ctx->err = "node_announcement receive: decreasing message offsets"; return LAMD_ERR_ARG; }
  const size_t msg_bytes = (size_t)(off[n] - off[0]), nodes = directory->nodes, channels = directory->count + directory->nbare;
  std::vector<u64> rel(n + 1);   // a queued copy reads it: STCHK drains the stream
  for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
  lamd_ctx *L = ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 32, st));
  STCHK(rocprim::radix_sort_keys(nullptr, need, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 32, st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::inclusive_scan(nullptr, need, (const u64 *)nullptr, (u64 *)nullptr, n, rocprim::maximum<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::exclusive_scan(nullptr, need, (const u32 *)nullptr, (u64 *)nullptr, (u64)0, n + 1, rocprim::plus<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  int rc;
  if ((rc = ensure(ctx, &ctx->store.rx, nr_ws(nullptr, n, nodes, msg_bytes, tmp_bytes).bytes)) != LAMD_OK) return rc;
  const nr_ws w(ctx->store.rx.as<u8>(), n, nodes, msg_bytes, tmp_bytes);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_rx.create());
  STCHK(hipMemcpyAsync(w.off, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
  if (msg_bytes) STCHK(hipMemcpyAsync(w.msgs, msgs + off[0], msg_bytes, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(w.start, 0, 16 * n, st));                  // start, len
  STCHK(hipMemsetAsync(w.acnt, 0, 8 * (n + 1), st));              // acnt, abytes
  STCHK(hipMemsetAsync(w.del_key, 0xFF, 4 * n, st));
  STCHK(hipMemsetAsync(w.cnt, 0, 4 * RX_CNTS, st));
  STCHK(hipMemsetAsync(w.flags, 0, n, st));
  STCHK(hipMemsetAsync(w.alive, 0, nodes + 1, st));
  const store_nr_view v{directory->img, directory->img_len, directory->rec_off, (u32)directory->n, directory->ent_rec, directory->bare_rec, directory->chan_rank,
                        (u32)directory->count, (u32)directory->nbare, directory->node_off, directory->node_nann, (u32)nodes};
  const store_nr_batch b{w.msgs, w.off, (u32)n, announcements_pending ? 1u : 0u};
  const store_rx_batch eb{w.msgs, w.off, (u32)n, nullptr, 0, nullptr, 0};   // the batch as the record encoder reads it
  const dim3 grid(blocks_for(n)), block(256);
  if (timed) STCHK(ctx->store.t_rx.record(0, st));
  if (channels) hipLaunchKernelGGL(k_nr_alive, dim3(blocks_for(channels)), block, 0, st, v, w.alive);
  hipLaunchKernelGGL(k_nr_classify, grid, block, 0, st, v, b, w.status, w.node, w.ts, w.row_of, w.start, w.len, w.row_msg, w.rowbase, w.cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(1, st));
  // ONE signature batch over n spans, each message under its own node_id: the real rows in front, empty spans behind them
  if ((rc = gossip_device(ctx, n, w.msgs, w.start, nullptr, w.rowbase, n, w.sigv, w.len)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (timed) STCHK(ctx->store.t_rx.record(2, st));
  hipLaunchKernelGGL(k_nr_settle, grid, block, 0, st, (u32)n, b.pending, w.status, w.node, (const u32 *)w.row_of, (const int8_t *)w.sigv, w.key, w.val);
  // stable: arrival order inside a node; the ranks need 30 bits, the pads (all ones) end behind them
  STCHK(rocprim::radix_sort_pairs(w.tmp, tmp_bytes, (const u64 *)w.key, w.skey, (const u32 *)w.val, w.sval, n, 0, 32, st));
  hipLaunchKernelGGL(k_rx_items, grid, block, 0, st, (u32)n, (const u64 *)w.skey, (const u32 *)w.sval, (const u32 *)w.ts, w.item);
  STCHK(rocprim::inclusive_scan(w.tmp, tmp_bytes, (const u64 *)w.item, w.run, n, rocprim::maximum<u64>(), st));
  hipLaunchKernelGGL(k_nr_resolve, grid, block, 0, st, v, b, store_rx_sorted{w.skey, w.sval, w.run, (u32)n}, (const u32 *)w.ts, (const u8 *)w.alive, w.status,
                     w.flags, store_nr_marks{w.acnt, w.abytes, w.del_key}, w.cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(3, st));
  STCHK(rocprim::radix_sort_keys(w.tmp, tmp_bytes, (const u32 *)w.del_key, w.del_sorted, n, 0, 32, st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.acnt, w.apos, (u64)0, n + 1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.abytes, w.abyte, (u64)0, n + 1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_nr_plan, grid, block, 0, st, (u32)n, (const int8_t *)w.status, (const u64 *)w.apos, (const u64 *)w.abyte, (u64)n, w.add_msg, w.add_off);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(4, st));
  u64 totals[2] = {0, 0};
  u32 cnt[RX_CNTS] = {};
  STCHK(hipMemcpyAsync(status, w.status, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(flags, w.flags, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(node, w.node, 4 * n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[0], w.apos + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[1], w.abyte + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(cnt, w.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: verdicts and sizes
  if (timed) STCHK(ctx->store.t_rx.read(4, summary->stage_ms));
  for (size_t i = 0; i < n; i++) {
    summary->by_status[status[i] < 0 || status[i] > 6 ? 7 : status[i]]++;
    summary->superseded += (flags[i] & STORE_RX_SUPERSEDED) != 0;
  }
  const u64 adds = totals[0], total = totals[1], dels = cnt[RX_CNT_DELS];
  summary->accepted = summary->adds = adds;
  summary->bytes = total;
  summary->deletions = dels;
  summary->signature_rows = cnt[RX_CNT_ROWS];
  const bool want_out = out || d_out;
  if (adds > add_cap) { ctx->err = "node_announcement receive: add_msg / add_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "node_announcement receive: output buffer too small"; return LAMD_ERR_ARG; }
  if (dels > edit_cap) { ctx->err = "node_announcement receive: del_rec too small"; return LAMD_ERR_ARG; }
  if (adds) {
    STCHK(hipMemcpyAsync(add_msg, w.add_msg, 4 * adds, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(add_off, w.add_off, 8 * adds, hipMemcpyDeviceToHost, st));
  }
  if (dels) STCHK(hipMemcpyAsync(del_rec, w.del_sorted, 4 * dels, hipMemcpyDeviceToHost, st));
  const bool encode = want_out && adds;
  if (encode) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.rx_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.rx_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    if (timed) STCHK(ctx->store.t_rx.record(5, st));
    hipLaunchKernelGGL(k_rx_encode, dim3(blocks_for(adds)), block, 0, st, (u32)adds, eb, (const u32 *)w.add_msg, (const u8 *)w.flags, (const u32 *)w.ts, w.hdr);
    hipLaunchKernelGGL(k_rx_copy, dim3((unsigned)((words + 255) / 256)), block, 0, st, words,
                       store_rx_out{w.add_off, w.add_msg, (u32)adds, w.hdr, w.msgs, w.off}, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_rx.record(6, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the lists and the bytes
  if (timed && encode) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_rx.ev[5], ctx->store.t_rx.ev[6]));
    summary->stage_ms[4] = ms;
  }
  return LAMD_OK;
}

// ---- channel_announcement reception, both halves (lamd_channel_announcement_receive_batch / _confirm_batch; per-message, per-position and
// per-reply logic in store_announce.h).  One lane per message, per sorted position, per reply or per output word; each stage reads what the one
// before it wrote, so each is a launch of its own.  The record headers and the output words are k_rx_encode's and k_rx_copy's.
enum { CA_CNT_SIGS = 0, CA_CNT_KEYS = 1, CA_CNTS = 4 };
// k_ca_classify: the framing half of -1 and statuses 1 .. 4; the rows of the TWO lists with one atomic per wave each: a message that passed the
// filters gets a span of the signature batch, a message a filter dropped gets its two bitcoin keys parsed.  rowbase: four rows per span.
__global__ void __launch_bounds__(256) k_ca_classify(store_ca_view v, store_ca_batch b, int8_t *__restrict__ status, u64 *__restrict__ scid, u32 *__restrict__ keyoff,
                                                     u8 *__restrict__ list, u32 *__restrict__ row_of, u64 *__restrict__ start, u64 *__restrict__ len,
                                                     u64 *__restrict__ rowbase, u8 *__restrict__ keys33, u32 *cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  store_ca_msg r;
  r.status = STORE_CA_MALFORMED;
  r.list = STORE_CA_LIST_NONE;
  r.keyoff = 0;
  if (i < b.n) {
    r = store_ca_classify(v, b, i);
    status[i] = (int8_t)r.status;
    scid[i] = r.scid;
    keyoff[i] = r.keyoff;
    list[i] = (u8)r.list;
    rowbase[i] = 4 * (u64)i;
    if (i == b.n - 1) rowbase[b.n] = 4 * (u64)b.n;
  }
  const bool sig = i < b.n && r.list == STORE_CA_LIST_SIGNATURES, key = i < b.n && r.list == STORE_CA_LIST_KEYS;
  const u32 srow = wave_alloc(&cnt[CA_CNT_SIGS], sig), krow = wave_alloc(&cnt[CA_CNT_KEYS], key);
  if (i < b.n) row_of[i] = sig ? srow : key ? krow : STORE_NONE;
  if (sig && srow < b.n) store_ca_sig_row(b, i, srow, start, len);
  if (key && krow < b.n) store_ca_key_row(b, i, r.keyoff, krow, keys33);
}
__global__ void __launch_bounds__(256) k_ca_settle(u32 n, u32 blockheight, int8_t *__restrict__ status, u64 *__restrict__ scid, const u8 *__restrict__ list,
                                                   const u32 *__restrict__ row_of, const int8_t *__restrict__ sigv, const u8 *__restrict__ keyok,
                                                   u64 *__restrict__ key, u32 *__restrict__ item, u32 *__restrict__ val) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 k = scid[i];   // (the sort key is the scid the message carries, malformed or not: only candidates are resolved)
  item[i] = store_ca_settle(status, scid, list, row_of, sigv, keyok, blockheight, i);
  key[i] = k;
  val[i] = i;
}
__global__ void __launch_bounds__(256) k_ca_items(u32 n, const u32 *__restrict__ sval, const u32 *__restrict__ item, u32 *__restrict__ sitem) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) sitem[p] = item[sval[p]];
}
__global__ void __launch_bounds__(256) k_ca_resolve(u32 n, u32 blockheight, const u32 *__restrict__ sval, const u32 *__restrict__ first,
                                                    const u64 *__restrict__ scid, int8_t *status, u32 *acnt) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) store_ca_resolve(sval, first, scid, blockheight, p, status, acnt);
}
// k_ca_script: scriptpubkey_p2wsh(bitcoin_redeem_2of2()) of the pending and early messages, two compressions per lane; the ask list
__global__ void __launch_bounds__(256) k_ca_script(store_ca_batch b, const int8_t *__restrict__ status, const u64 *__restrict__ scid,
                                                   const u32 *__restrict__ keyoff, const u64 *__restrict__ apos, u64 ask_cap, u8 *__restrict__ spk34,
                                                   u32 *__restrict__ ask_msg, u64 *__restrict__ ask_scid) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i < b.n) store_ca_finish(b, status, scid, keyoff, apos, ask_cap, spk34, ask_msg, ask_scid, i);
}

// the workspace of one call, carved out of store.rx (the receive calls of a context run one behind the other)
struct ca_ws {
  u64 *off, *start, *len, *rowbase, *scid, *key, *skey, *apos, *ask_scid, *held, *failed;
  u32 *keyoff, *row_of, *val, *sval, *item, *sitem, *first, *acnt, *ask_msg, *cnt, *qwords;
  int8_t *status, *sigv;
  u8 *list, *keys33, *keyok, *spk, *msgs, *tmp;
  size_t bytes;
  ca_ws(u8 *base, size_t n, size_t n_held, size_t n_failed, size_t msg_bytes, size_t tmp_bytes) {
    size_t at = 0;
    auto take = [&](auto **p, size_t count) {
      using T = std::remove_reference_t<decltype(**p)>;
      *p = base ? (T *)(base + at) : nullptr;
      at += sizeof(T) * count;
    };
    take(&off, n + 1); take(&start, n); take(&len, n); take(&rowbase, n + 1); take(&scid, n); take(&key, n); take(&skey, n); take(&apos, n + 1);
    take(&ask_scid, n); take(&held, n_held); take(&failed, n_failed);
    take(&qwords, 32 * n);   // 64 bytes per key, two keys per message
    take(&keyoff, n); take(&row_of, n); take(&val, n); take(&sval, n); take(&item, n); take(&sitem, n); take(&first, n); take(&acnt, n + 1);
    take(&ask_msg, n); take(&cnt, CA_CNTS);
    take(&status, n); take(&sigv, n); take(&list, n); take(&keys33, 66 * n); take(&keyok, 2 * n); take(&spk, STORE_CA_SPK * n); take(&msgs, msg_bytes + 1);
    at = align_up(at, 256);
    take(&tmp, tmp_bytes);
    bytes = at + 16;
  }
};

extern "C" int lamd_channel_announcement_receive_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, uint32_t blockheight,
                                                       size_t n, const uint8_t *msgs, const uint64_t *off, size_t n_held, const uint64_t *held_scid,
                                                       size_t n_failed, const uint64_t *failed_scid, int8_t *status, uint64_t *scid, uint8_t *spk34,
                                                       size_t ask_cap, uint32_t *ask_msg, uint64_t *ask_scid, lamd_announce_receive_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!digest || !chain_hash32 || !summary || (n && (!msgs || !off || !status || !scid || !spk34)) || (ask_cap && (!ask_msg || !ask_scid)) ||
      (n_held && !held_scid) || (n_failed && !failed_scid) || n >= (size_t)STORE_NONE / 4 || n_held >= (size_t)STORE_NONE || n_failed >= (size_t)STORE_NONE) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  if (digest->ctx != ctx) { ctx->err = "channel_announcement receive: the digest does not belong to this context"; return LAMD_ERR_ARG; }
  *summary = lamd_announce_receive_summary();
  if (n == 0) return LAMD_OK;
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) { ctx->err = "channel_announcement receive: decreasing message offsets"; return LAMD_ERR_ARG; }
  for (size_t k = 1; k < n_held; k++)
    if (held_scid[k] <= held_scid[k - 1]) { ctx->err = "channel_announcement receive: held_scid is not ascending"; return LAMD_ERR_ARG; }
  for (size_t k = 1; k < n_failed; k++)
    if (failed_scid[k] <= failed_scid[k - 1]) { ctx->err = "channel_announcement receive: failed_scid is not ascending"; return LAMD_ERR_ARG; }
  const size_t msg_bytes = (size_t)(off[n] - off[0]);
  std::vector<u64> rel(n + 1);   // a queued copy reads it: STCHK drains the stream
  for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
  lamd_ctx *L = ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, n, 0, 64, st));
  STCHK(rocprim::inclusive_scan_by_key(nullptr, need, (const u64 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, n, rocprim::minimum<u32>(),
                                       rocprim::equal_to<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  STCHK(rocprim::exclusive_scan(nullptr, need, (const u32 *)nullptr, (u64 *)nullptr, (u64)0, n + 1, rocprim::plus<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  int rc;
  if ((rc = ensure(ctx, &ctx->store.rx, ca_ws(nullptr, n, n_held, n_failed, msg_bytes, tmp_bytes).bytes)) != LAMD_OK) return rc;
  const ca_ws w(ctx->store.rx.as<u8>(), n, n_held, n_failed, msg_bytes, tmp_bytes);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_rx.create());
  STCHK(hipMemcpyAsync(w.off, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
  if (msg_bytes) STCHK(hipMemcpyAsync(w.msgs, msgs + off[0], msg_bytes, hipMemcpyHostToDevice, st));
  if (n_held) STCHK(hipMemcpyAsync(w.held, held_scid, 8 * n_held, hipMemcpyHostToDevice, st));
  if (n_failed) STCHK(hipMemcpyAsync(w.failed, failed_scid, 8 * n_failed, hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(w.acnt, 0, 4 * (n + 1), st));
  STCHK(hipMemsetAsync(w.cnt, 0, 4 * CA_CNTS, st));
  const store_ca_view v{digest->scid, (u32)digest->count, digest->bare, (u32)digest->nbare};
  store_ca_batch b{w.msgs, w.off, (u32)n, w.held, (u32)n_held, w.failed, (u32)n_failed, blockheight, {}};
  memcpy(b.chain, chain_hash32, 32);
  const dim3 grid(blocks_for(n)), block(256);
  if (timed) STCHK(ctx->store.t_rx.record(0, st));
  hipLaunchKernelGGL(k_ca_classify, grid, block, 0, st, v, b, w.status, w.scid, w.keyoff, w.list, w.row_of, w.start, w.len, w.rowbase, w.keys33, w.cnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(1, st));
  // the lengths of the two lists: eight bytes the host waits for, so that a batch of known channels costs no signature row at all (four
  // all-zero rows per message would be what the ecmult still walks)
  u32 cnt[CA_CNTS] = {};
  STCHK(hipMemcpyAsync(cnt, w.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));
  const size_t sigs = cnt[CA_CNT_SIGS], keys = cnt[CA_CNT_KEYS];
  if (sigs > n || keys > n || sigs + keys > n) { ctx->err = "channel_announcement receive: the lists are longer than the batch"; return LAMD_ERR_HIP; }
  // ONE signature batch over the spans of the signature list, four rows each, every signer taken from its message
  if (sigs && (rc = gossip_device(ctx, sigs, w.msgs, w.start, nullptr, w.rowbase, 4 * sigs, w.sigv, w.len)) != LAMD_OK) return drain_fail(ctx, L, rc);
  // the key-parse list: the validity bytes of its bitcoin keys (the kernel behind lamd_pubkey_parse_batch)
  if (keys && (rc = launch_key_validity(ctx, st, 2 * keys, w.keys33, w.qwords, w.keyok)) != LAMD_OK) return drain_fail(ctx, L, rc);
  if (timed) STCHK(ctx->store.t_rx.record(2, st));
  hipLaunchKernelGGL(k_ca_settle, grid, block, 0, st, (u32)n, blockheight, w.status, w.scid, (const u8 *)w.list, (const u32 *)w.row_of, (const int8_t *)w.sigv,
                     (const u8 *)w.keyok, w.key, w.item, w.val);
  // stable: arrival order inside a scid, all 64 bits of it
  STCHK(rocprim::radix_sort_pairs(w.tmp, tmp_bytes, (const u64 *)w.key, w.skey, (const u32 *)w.val, w.sval, n, 0, 64, st));
  hipLaunchKernelGGL(k_ca_items, grid, block, 0, st, (u32)n, (const u32 *)w.sval, (const u32 *)w.item, w.sitem);
  STCHK(rocprim::inclusive_scan_by_key(w.tmp, tmp_bytes, (const u64 *)w.skey, (const u32 *)w.sitem, w.first, n, rocprim::minimum<u32>(),
                                       rocprim::equal_to<u64>(), st));
  hipLaunchKernelGGL(k_ca_resolve, grid, block, 0, st, (u32)n, blockheight, (const u32 *)w.sval, (const u32 *)w.first, (const u64 *)w.scid, w.status, w.acnt);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(3, st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.acnt, w.apos, (u64)0, n + 1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_ca_script, grid, block, 0, st, b, (const int8_t *)w.status, (const u64 *)w.scid, (const u32 *)w.keyoff, (const u64 *)w.apos, (u64)n, w.spk,
                     w.ask_msg, w.ask_scid);
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(4, st));
  u64 asks = 0;
  STCHK(hipMemcpyAsync(status, w.status, n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(scid, w.scid, 8 * n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(spk34, w.spk, STORE_CA_SPK * n, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&asks, w.apos + n, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: verdicts and sizes
  if (timed) STCHK(ctx->store.t_rx.read(4, summary->stage_ms));
  for (size_t i = 0; i < n; i++) summary->by_status[status[i] < 0 || status[i] > 11 ? 12 : status[i]]++;
  summary->asks = asks;
  summary->signature_rows = 4 * sigs;
  summary->keyparse_rows = 2 * keys;
  if (asks > ask_cap) { ctx->err = "channel_announcement receive: ask_msg / ask_scid too small"; return LAMD_ERR_ARG; }
  if (asks) {
    STCHK(hipMemcpyAsync(ask_msg, w.ask_msg, 4 * asks, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(ask_scid, w.ask_scid, 8 * asks, hipMemcpyDeviceToHost, st));
    STCHK(hipStreamSynchronize(st));   // the second wait: the ask list
  }
  return LAMD_OK;
}

// ---- the replies.  k_ca_match: the pending announcement of every reply, the first reply of every pending slot (one 32-bit atomicMin)
__global__ void __launch_bounds__(256) k_ca_match(store_cf_batch b, u32 *__restrict__ pend, u32 *first) {
  const u32 r = blockIdx.x * 256 + threadIdx.x;
  if (r < b.nr) store_cf_match(b, r, pend, first);
}
__global__ void __launch_bounds__(256) k_ca_confirm(store_cf_view v, store_cf_batch b, int8_t *__restrict__ status, u32 *__restrict__ pend,
                                                    const u32 *__restrict__ first, store_cf_marks k) {
  const u32 r = blockIdx.x * 256 + threadIdx.x;
  if (r < b.nr) status[r] = (int8_t)store_cf_classify(v, b, r, pend, first, k);
}
__global__ void __launch_bounds__(256) k_ca_clr_heads(u32 m, const u32 *__restrict__ sorted, u32 *__restrict__ head) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  if (p < m) head[p] = store_cf_clr_head(sorted, p);
}
__global__ void __launch_bounds__(256) k_ca_clr_write(u32 m, const u32 *__restrict__ sorted, const u32 *__restrict__ head, const u64 *__restrict__ pos,
                                                      u32 *__restrict__ clr) {
  const u32 p = blockIdx.x * 256 + threadIdx.x;
  if (p < m && head[p]) clr[pos[p]] = sorted[p];
}
__global__ void __launch_bounds__(256) k_ca_plan(store_cf_batch b, const int8_t *__restrict__ status, const u32 *__restrict__ pend, const u64 *__restrict__ apos,
                                                 const u64 *__restrict__ abyte, const u64 *__restrict__ fpos, store_cf_plan_out o) {
  const u32 r = blockIdx.x * 256 + threadIdx.x;
  if (r < b.nr) store_cf_plan(b, status, pend, apos, abyte, fpos, o, r);
}

// the workspace of one confirm call, carved out of store.rx.  msgs: the pending messages, then ten bytes per reply for the amount messages
struct cf_ws {
  u64 *off2, *pscid, *r_scid, *r_sat, *soff, *apos, *abyte, *fpos, *cpos, *add_off, *fail_scid, *rec_off;
  u32 *pend, *first, *acnt, *abytes, *fcnt, *clr_key, *clr_sorted, *clr_head, *clr, *add_reply, *rec_msg, *zero;
  int8_t *status;
  u8 *pspk, *scripts, *hdr, *flags0, *msgs, *tmp;
  size_t bytes;
  cf_ws(u8 *base, size_t np, size_t nr, size_t msg_bytes, size_t script_bytes, size_t tmp_bytes) {
    size_t at = 0;
    auto take = [&](auto **p, size_t count) {
      using T = std::remove_reference_t<decltype(**p)>;
      *p = base ? (T *)(base + at) : nullptr;
      at += sizeof(T) * count;
    };
    take(&off2, np + nr + 1); take(&pscid, np); take(&r_scid, nr); take(&r_sat, nr); take(&soff, nr + 1); take(&apos, nr + 1); take(&abyte, nr + 1);
    take(&fpos, nr + 1); take(&cpos, 2 * nr + 1); take(&add_off, nr); take(&fail_scid, nr); take(&rec_off, 2 * nr + 1);
    take(&pend, nr); take(&first, np);
    take(&acnt, nr + 1); take(&abytes, nr + 1); take(&fcnt, nr + 1);   // (one memset clears the three)
    take(&clr_key, 2 * nr); take(&clr_sorted, 2 * nr); take(&clr_head, 2 * nr + 1); take(&clr, 2 * nr); take(&add_reply, nr); take(&rec_msg, 2 * nr);
    take(&zero, np + nr);    // the timestamps of the records: all 0
    take(&status, nr); take(&pspk, STORE_CA_SPK * np); take(&scripts, script_bytes + 1); take(&hdr, STORE_HDR * 2 * nr); take(&flags0, np + nr);
    take(&msgs, msg_bytes + STORE_CA_AMOUNT * nr + 1);
    at = align_up(at, 256);
    take(&tmp, tmp_bytes);
    bytes = at + 16;
  }
};

extern "C" int lamd_channel_announcement_confirm_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const lamd_store_directory *directory, size_t np,
                                                       const uint8_t *pend_msgs, const uint64_t *pend_off, const uint8_t *pend_spk34, size_t nr,
                                                       const uint64_t *r_scid, const uint64_t *r_sat, const uint8_t *r_scripts, const uint64_t *r_script_off,
                                                       int8_t *status, uint32_t *pend, size_t add_cap, uint32_t *add_reply, uint64_t *add_off, uint8_t *out,
                                                       void *d_out, size_t out_cap, size_t fail_cap, uint64_t *fail_scid, size_t clr_cap, uint32_t *clr_rec,
                                                       lamd_announce_confirm_summary *summary) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!digest || !directory || !summary || (np && (!pend_msgs || !pend_off || !pend_spk34)) || (nr && (!r_scid || !r_sat || !r_script_off || !status || !pend)) ||
      (add_cap && (!add_reply || !add_off)) || (fail_cap && !fail_scid) || (clr_cap && !clr_rec) || np >= (size_t)STORE_NONE / 4 || nr >= (size_t)STORE_NONE / 4) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  // the digest and the directory of ONE image, built by this context
  if (digest->ctx != ctx || directory->ctx != ctx || directory->n != digest->cap || directory->count != digest->count || directory->nbare != digest->nbare) {
    ctx->err = "channel_announcement confirm: the digest and the directory do not belong to this context and to one image";
    return LAMD_ERR_ARG;
  }
  *summary = lamd_announce_confirm_summary();
  // the pending announcements as the caller's map iterates them: well framed, strictly ascending by scid
  std::vector<u64> pscid(np), rel(np + nr + 1), srel(nr + 1);
  for (size_t p = 0; p < np; p++) {
    if (pend_off[p + 1] < pend_off[p]) { ctx->err = "channel_announcement confirm: decreasing message offsets"; return LAMD_ERR_ARG; }
    const u8 *m = pend_msgs + pend_off[p];
    const size_t len = (size_t)(pend_off[p + 1] - pend_off[p]);
    if (len < STORE_CA_MIN || len > STORE_CA_MAX || store_be16(m) != STORE_T_CANN) { ctx->err = "channel_announcement confirm: a pending message is no channel_announcement"; return LAMD_ERR_ARG; }
    const gossip_frame f = gossip_parse_frame(m, len);
    if (f.bad) { ctx->err = "channel_announcement confirm: a pending message is no channel_announcement"; return LAMD_ERR_ARG; }
    pscid[p] = store_be64(m + f.keyoff - 8);
    if (p && pscid[p] <= pscid[p - 1]) { ctx->err = "channel_announcement confirm: the pending announcements are not strictly ascending by scid"; return LAMD_ERR_ARG; }
  }
  if (nr == 0) return LAMD_OK;
  for (size_t r = 0; r < nr; r++)
    if (r_script_off[r + 1] < r_script_off[r]) { ctx->err = "channel_announcement confirm: decreasing script offsets"; return LAMD_ERR_ARG; }
  const size_t msg_bytes = np ? (size_t)(pend_off[np] - pend_off[0]) : 0, script_bytes = (size_t)(r_script_off[nr] - r_script_off[0]);
  if (script_bytes && !r_scripts) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  for (size_t p = 0; p <= np; p++) rel[p] = np ? pend_off[p] - pend_off[0] : 0;
  for (size_t j = 1; j <= nr; j++) rel[np + j] = 0;   // (k_ca_plan writes the offsets of the amount messages)
  for (size_t r = 0; r <= nr; r++) srel[r] = r_script_off[r] - r_script_off[0];
  lamd_ctx *L = ctx;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_bytes = 0, need = 0;
  STCHK(rocprim::radix_sort_keys(nullptr, tmp_bytes, (const u32 *)nullptr, (u32 *)nullptr, 2 * nr, 0, 32, st));
  STCHK(rocprim::exclusive_scan(nullptr, need, (const u32 *)nullptr, (u64 *)nullptr, (u64)0, 2 * nr + 1, rocprim::plus<u64>(), st));
  if (need > tmp_bytes) tmp_bytes = need;
  int rc;
  if ((rc = ensure(ctx, &ctx->store.rx, cf_ws(nullptr, np, nr, msg_bytes, script_bytes, tmp_bytes).bytes)) != LAMD_OK) return rc;
  const cf_ws w(ctx->store.rx.as<u8>(), np, nr, msg_bytes, script_bytes, tmp_bytes);
  const bool timed = ctx->timing;
  if (timed) STCHK(ctx->store.t_rx.create());
  STCHK(hipMemcpyAsync(w.off2, rel.data(), 8 * (np + nr + 1), hipMemcpyHostToDevice, st));
  if (np) {
    STCHK(hipMemcpyAsync(w.pscid, pscid.data(), 8 * np, hipMemcpyHostToDevice, st));
    STCHK(hipMemcpyAsync(w.pspk, pend_spk34, STORE_CA_SPK * np, hipMemcpyHostToDevice, st));
    STCHK(hipMemsetAsync(w.first, 0xFF, 4 * np, st));
  }
  if (msg_bytes) STCHK(hipMemcpyAsync(w.msgs, pend_msgs + pend_off[0], msg_bytes, hipMemcpyHostToDevice, st));
  if (script_bytes) STCHK(hipMemcpyAsync(w.scripts, r_scripts + r_script_off[0], script_bytes, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(w.r_scid, r_scid, 8 * nr, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(w.r_sat, r_sat, 8 * nr, hipMemcpyHostToDevice, st));
  STCHK(hipMemcpyAsync(w.soff, srel.data(), 8 * (nr + 1), hipMemcpyHostToDevice, st));
  STCHK(hipMemsetAsync(w.acnt, 0, 12 * (nr + 1), st));             // acnt, abytes, fcnt
  STCHK(hipMemsetAsync(w.clr_key, 0xFF, 8 * nr, st));
  STCHK(hipMemsetAsync(w.clr_head, 0, 4 * (2 * nr + 1), st));
  STCHK(hipMemsetAsync(w.zero, 0, 4 * (np + nr), st));
  STCHK(hipMemsetAsync(w.flags0, 0, np + nr, st));
  const store_cf_view v{digest->scid, (u32)digest->count, digest->bare, (u32)digest->nbare, directory->img, directory->img_len, directory->rec_off,
                        (u32)directory->n, directory->node_off, directory->node_nann, (u32)directory->nodes};
  const store_cf_batch b{w.msgs, w.off2, w.pscid, w.pspk, (u32)np, w.r_scid, w.r_sat, w.scripts, w.soff, (u32)nr};
  const dim3 grid(blocks_for(nr)), grid2(blocks_for(2 * nr)), block(256);
  if (timed) STCHK(ctx->store.t_rx.record(0, st));
  hipLaunchKernelGGL(k_ca_match, grid, block, 0, st, b, w.pend, w.first);
  hipLaunchKernelGGL(k_ca_confirm, grid, block, 0, st, v, b, w.status, w.pend, (const u32 *)w.first, store_cf_marks{w.acnt, w.abytes, w.fcnt, w.clr_key});
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(1, st));
  // node_announcements_not_dying(): the dying records of the accepted announcements' nodes, ascending, each once
  STCHK(rocprim::radix_sort_keys(w.tmp, tmp_bytes, (const u32 *)w.clr_key, w.clr_sorted, 2 * nr, 0, 32, st));
  hipLaunchKernelGGL(k_ca_clr_heads, grid2, block, 0, st, (u32)(2 * nr), (const u32 *)w.clr_sorted, w.clr_head);
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.clr_head, w.cpos, (u64)0, 2 * nr + 1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_ca_clr_write, grid2, block, 0, st, (u32)(2 * nr), (const u32 *)w.clr_sorted, (const u32 *)w.clr_head, (const u64 *)w.cpos, w.clr);
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.acnt, w.apos, (u64)0, nr + 1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.abytes, w.abyte, (u64)0, nr + 1, rocprim::plus<u64>(), st));
  STCHK(rocprim::exclusive_scan(w.tmp, tmp_bytes, (const u32 *)w.fcnt, w.fpos, (u64)0, nr + 1, rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(k_ca_plan, grid, block, 0, st, b, (const int8_t *)w.status, (const u32 *)w.pend, (const u64 *)w.apos, (const u64 *)w.abyte, (const u64 *)w.fpos,
                     store_cf_plan_out{(u64)nr, (u64)nr, w.add_reply, w.add_off, w.fail_scid, w.rec_msg, w.rec_off, w.off2, w.msgs + msg_bytes, (u64)msg_bytes});
  STCHK(hipGetLastError());
  if (timed) STCHK(ctx->store.t_rx.record(2, st));
  u64 totals[4] = {0, 0, 0, 0};
  STCHK(hipMemcpyAsync(status, w.status, nr, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(pend, w.pend, 4 * nr, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[0], w.apos + nr, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[1], w.abyte + nr, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[2], w.fpos + nr, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipMemcpyAsync(&totals[3], w.cpos + 2 * nr, 8, hipMemcpyDeviceToHost, st));
  STCHK(hipStreamSynchronize(st));   // the first wait: verdicts and sizes
  if (timed) STCHK(ctx->store.t_rx.read(2, summary->stage_ms));
  for (size_t r = 0; r < nr; r++) summary->by_status[status[r] < 0 || status[r] > 4 ? 1 : status[r]]++;
  const u64 adds = totals[0], total = totals[1], fails = totals[2], clrs = totals[3];
  summary->adds = adds;
  summary->bytes = total;
  summary->failures = fails;
  summary->clears = clrs;
  const bool want_out = out || d_out;
  if (adds > add_cap) { ctx->err = "channel_announcement confirm: add_reply / add_off too small"; return LAMD_ERR_ARG; }
  if (want_out && total > out_cap) { ctx->err = "channel_announcement confirm: output buffer too small"; return LAMD_ERR_ARG; }
  if (fails > fail_cap) { ctx->err = "channel_announcement confirm: fail_scid too small"; return LAMD_ERR_ARG; }
  if (clrs > clr_cap) { ctx->err = "channel_announcement confirm: clr_rec too small"; return LAMD_ERR_ARG; }
  if (adds) {
    STCHK(hipMemcpyAsync(add_reply, w.add_reply, 4 * adds, hipMemcpyDeviceToHost, st));
    STCHK(hipMemcpyAsync(add_off, w.add_off, 8 * adds, hipMemcpyDeviceToHost, st));
  }
  if (fails) STCHK(hipMemcpyAsync(fail_scid, w.fail_scid, 8 * fails, hipMemcpyDeviceToHost, st));
  if (clrs) STCHK(hipMemcpyAsync(clr_rec, w.clr, 4 * clrs, hipMemcpyDeviceToHost, st));
  const bool encode = want_out && adds;
  if (encode) {
    if (!d_out && (rc = ensure(ctx, &ctx->store.rx_out, total + 16)) != LAMD_OK) return drain_fail(ctx, L, rc);
    u8 *d_bytes = d_out ? (u8 *)d_out : ctx->store.rx_out.as<u8>();
    const u64 words = (total + ((uintptr_t)d_bytes & 3) + 3) / 4;
    const store_rx_batch eb{w.msgs, w.off2, (u32)(np + adds), nullptr, 0, nullptr, 0};   // the pending and the amount messages as the record encoder reads them
    if (timed) STCHK(ctx->store.t_rx.record(5, st));
    hipLaunchKernelGGL(k_rx_encode, dim3(blocks_for(2 * adds)), block, 0, st, (u32)(2 * adds), eb, (const u32 *)w.rec_msg, (const u8 *)w.flags0, (const u32 *)w.zero, w.hdr);
    hipLaunchKernelGGL(k_rx_copy, dim3((unsigned)((words + 255) / 256)), block, 0, st, words,
                       store_rx_out{w.rec_off, w.rec_msg, (u32)(2 * adds), w.hdr, w.msgs, w.off2}, d_bytes, total);
    STCHK(hipGetLastError());
    if (timed) STCHK(ctx->store.t_rx.record(6, st));
    if (out) STCHK(hipMemcpyAsync(out, d_bytes, total, hipMemcpyDeviceToHost, st));
  }
  STCHK(hipStreamSynchronize(st));   // the second wait: the lists and the bytes
  if (timed && encode) {
    float ms = 0;
    STCHK(hipEventElapsedTime(&ms, ctx->store.t_rx.ev[5], ctx->store.t_rx.ev[6]));
    summary->stage_ms[2] = ms;
  }
  return LAMD_OK;
}

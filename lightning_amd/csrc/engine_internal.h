// The engine's internals, as far as the other translation units of liblightning_amd.so may know them: the context, its workspaces and the
// handful of core functions (lamd_engine.hip) that the front ends (lamd_frontends.hip), the gossip_store calls (lamd_store.hip) and the debuggers
// (lamd_debug.hip) are built on.  No kernel is launched from a unit other than the one that defines it and no device symbol crosses a unit:
// the library builds without relocatable device code.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <random>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/lightning_amd.h"
#include "../../include/lightning_amd_debug.h"
#include "verify_core.h"

using namespace lamd;

constexpr int MAX_LANES = 8;
#ifndef LAMD_PRIO_DEFAULT
#define LAMD_PRIO_DEFAULT 13   // lamd_engine.hip, g_prio
#endif

// The one piece of device code in this header: kernels of the core (the list builders) and of lamd_store.hip (k_digest_chan) both call it.  It is
// force-inlined into each of them, so no device symbol crosses a unit.
// Wave-aggregated allocation from a global counter: ONE atomic per wavefront (an uncontended device atomic costs
// ~10 ns; a million lane-level atomics on one word serialise into >10 ms -- measured).  Every lane of the wave must call
// it; lanes with pred get consecutive indices.  `weight` (optional) is summed over the pred lanes into *wsum.
__device__ __forceinline__ u32 wave_alloc(u32 *counter, bool pred, u32 weight = 0, u32 *wsum = nullptr) {
  const u64 mask = __ballot(pred);
  const u32 lane = threadIdx.x & 63u;
  const u32 prefix = (u32)__popcll(mask & ((1ull << lane) - 1ull));
  if (wsum) {
    u32 w = pred ? weight : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if (lane == 0 && w) atomicAdd(wsum, w);
  }
  u32 base = 0;
  if (mask == 0) return 0;
  const int leader = __ffsll((long long)mask) - 1;
  if ((int)lane == leader) base = atomicAdd(counter, (u32)__popcll(mask));
  base = __shfl(base, leader, 64);
  return base + prefix;
}

static constexpr size_t CHUNK_DEFAULT = (size_t)1 << 22;  // signatures per launch sequence (4 GiB of table slots at most; allocated on demand)

// a device workspace: grown by ensure(), freed by its owner's destructor (release(): where the code frees early)
struct devbuf {
  void *p = nullptr;
  size_t cap = 0;
  devbuf() {}   // (user-provided: no aggregate, so nothing builds a second owner from a pointer and a size)
  devbuf(const devbuf &) = delete;
  devbuf &operator=(const devbuf &) = delete;
  ~devbuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

// The boundaries of a call's stages as events: made when a timed call first runs, slot k recorded between two stages, the intervals read behind the
// synchronisation that ends the call.
template <int N>
struct stage_timer {
  hipEvent_t ev[N] = {};
  hipError_t create() {
    hipError_t r = hipSuccess;
    for (auto &e : ev)
      if (!e && r == hipSuccess) r = hipEventCreate(&e);
    return r;
  }
  hipError_t record(int k, hipStream_t st) { return hipEventRecord(ev[k], st); }
  hipError_t read(int stages, double *ms) const {   // ms[k] = from slot k to slot k + 1
    hipError_t r = hipSuccess;
    for (int k = 0; k < stages && r == hipSuccess; k++) {
      float f = 0;
      r = hipEventElapsedTime(&f, ev[k], ev[k + 1]);
      if (r == hipSuccess) ms[k] = f;
    }
    return r;
  }
  void destroy() {
    for (auto &e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

enum { Q_ECDSA33 = 0, Q_ECDSA65 = 1, Q_SCHNORR = 2, Q_KINDS = 3 };
#ifndef LAMD_QUEUE_SETS
#define LAMD_QUEUE_SETS 9
#endif
constexpr int QUEUE_SETS = LAMD_QUEUE_SETS;  // staging sets of the streaming queue: one open + up to QUEUE_SETS - 1 flushes in flight

struct lamd_ctx {
  int device = 0;
  int gtable_device = -1;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop;
  u32 *gtable = nullptr;
  std::string err;
  // per-call workspaces (grown on demand, reused)
  devbuf recs, qwords, keyok, slots, vbuf;
  // keyed path: row -> cache entry, de-duplication of the rows the cache did not know, new keys per comb shape (hk[0]: 7 teeth,
  // hk[1]: 10 teeth -- representative row, cache entry, table slot; parsed key, validity, build scratch), row lists per shape + cold rows
  devbuf row_ent, kd_table, kd_rep, kd_uid, kd_uniq, kd_count, kd_newent, plan, kt_fin;
  struct shape_ws { devbuf row, ent, slot, qwords, keyok, scratch; } hk[2];
  devbuf kc_chains;               // the finish kernel's per-chain words: KC_CHAIN_CHUNKS 16-byte chunks per thread of its resident grid, interleaved over a block (verify_core.h kc_lanes)
  devbuf list7, list10, listcold, listcold_ok;
  // latency path (k_small_verify): pinned, device-mapped staging for up to SMALL_MAX rows, the verdict bytes and the completion word
  u8 *h_small = nullptr;
  // pinned: the flattened transaction templates of a lamd_check_commitment_signed / mid-size check_tx_sig call, copied to HBM from here (lamd_frontends.hip)
  struct tmpl_ws {
    u8 *h = nullptr;
    size_t cap = 0;
  } tmpl;
  devbuf small_done;          // block counter of k_small_verify grids (device memory)
  std::vector<u64> small_missed;   // fingerprints of keys the latency path verified without a table (MISS_SLOTS, 4-way set-associative)
  u32 prio_mask = LAMD_PRIO_DEFAULT; // LAMD_PRIO: which kernel classes raise their wave priority (g_prio)
  unsigned spin_us = 2000;         // LAMD_SPIN_US: longest busy-wait of a latency-path call before it blocks in the runtime
  std::vector<u64> learn_fps;      // the fingerprints that recurred in the call that set force_learn: only these keys get tables (learn_filter)
  devbuf learn_dev;
  bool force_learn = false;         // the next small call on this context builds tables for every key the cache misses
  u32 small_ticket = 0;
  bool small_kernel = true;   // LAMD_SMALL_KERNEL=0: such calls take the general path
  u32 *h_plan = nullptr;   // pinned read-back of the last call's plan + cache counters (statistics only: nothing waits for it)
  // Key-table cache.  The root context owns the shared one (LAMD_CACHE=1, default): entries + index + one table pool per
  // comb shape, filled by whichever lane meets a key often enough, looked up by every later call.  With LAMD_CACHE=0 every
  // lane uses its own private instance without an index, reset at the start of each call (tables live for one call).
  struct key_cache {
    bool shared = false;
    u32 cap_ent = 0, cap7 = 0, cap10 = 0, index_mask = 0;
    devbuf ents, index, pool7, pool10, counters;
  } cache_store;
  key_cache *cache = nullptr;       // what this context's calls use (lanes: the root's when shared)
  lamd_ctx *root = nullptr;         // lanes: the context that owns them
  int lane_id = 0;                  // 0 = the root context itself, 1.. = lanes
  u32 call_seq = 0;                 // root: sequence number of the last submitted keyed call
  u32 pub_seq[MAX_LANES + 1] = {};  // root: per lane (by lane_id), the sequence number of its last publishing call ...
  hipEvent_t ev_pub[MAX_LANES + 1] = {};   // ... and the event recorded after it
  u32 vis_seq[MAX_LANES + 1] = {};  // root: per lane, the newest publishing call the host has SEEN complete
  bool pub_pending[MAX_LANES + 1] = {};
  int cache_mode = 1;               // LAMD_CACHE
  size_t cache_keys = (size_t)1 << 20, cache_keys10 = (size_t)1 << 16;   // LAMD_CACHE_KEYS / LAMD_CACHE_KEYS10
  u32 cache_hwm[3] = {0, 0, 0};     // root: last counters read back (entries, 7-tooth slots, 10-tooth slots)
  u32 cache_resets = 0;
  size_t last_hits = 0, last_cold = 0, last_l7 = 0, last_l10 = 0;
  devbuf keyok_row;
  hipStream_t stream2 = nullptr;   // scalar prep runs here, concurrently with the key work on `stream`
  hipStream_t stream3 = nullptr;   // cold rows of a partitioned chunk
  hipEvent_t ev_fork = nullptr, ev_prep = nullptr, ev_cold = nullptr, ev_keys = nullptr, ev_sigs = nullptr;
  bool sigs_pending = false;  // lamd_flush sent the signature copy down another stream: the first kernel of the main stream that reads signatures waits for ev_sigs_wait
  hipEvent_t ev_sigs_wait = nullptr;   // the event that copy is followed by (the lane's own ev_sigs, or the staging set's)
  // root only: the H2D copies of the flushes, behind nothing but each other (lamd_flush).  Round 5 experiment: SEVERAL such streams, successive flushes taking
  // turns (LAMD_COPY_STREAMS, default 1: two and three measured SLOWER, 212 / 203 against 218 M/s -- profiles/r05_ab_variants.txt).  On ONE stream the three copies of a flush and the copies of the next flush follow each other with gaps of
  // 0.1-1 ms (rocprofv3 --memory-copy-trace of the cold streaming loop, profiles/r05_stream_timeline.txt): 3.0 ms of transfers took 3.5-3.9 ms, the
  // stream was busy 85-90 % of the time and set the loop's pace -- 4.25 ms per flush against the 4.05 ms the kernels need --, every call's front end
  // started the moment its keys landed and only one table-driven ecmult launch was ever in flight.  With two streams the next flush's copies run in
  // the gaps of the current one's.
  static constexpr int MAX_COPY_STREAMS = 4;
  hipStream_t copy_streams[MAX_COPY_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  int n_copy_streams = 1;
  bool copy_one = true;         // LAMD_COPY_ONE=0: a full staging set still goes down as three copies
  int copy_events = 0;          // LAMD_COPY_EVENTS: events a flush records between / behind its three copies (3: keys | signatures | hashes, 2: keys | rest, 1: all; 0: by load)
  unsigned copy_turn = 0;
  bool use_copy_stream = true;         // LAMD_COPY_STREAM=0: a flush's copies go down its lane's prep stream (the round-2 form)
  int keyed_mode = -1;           // -1 auto, 0 never, 1 whenever keys repeat at all (LAMD_KEYED)
  size_t keyed_min_rows = 8192;  // below this a batch is latency-bound: per-signature ladder
  bool early_cold = true;         // LAMD_EARLY_COLD=0: the cold rows' list is made by k_partition, after the table kernels (rounds 1-5)
  bool fused_front = true;        // LAMD_FUSED_FRONT=0: the front end of a keyed call as the 19 launches + 5 fills of round 2 (see k_call_init)
  bool kc_tree = false;           // LAMD_KC_TREE=1: key tables by the affine tree builder (k_kc_tree_both) instead of the Gray-code chains (k_kc_finish_both); read on the root context
  unsigned table_grid = 0;        // LAMD_TABLE_GRID: blocks of the resident grids of k_keys_bases_both / k_kc_finish_both (0: one per compute unit -- table_grid()); read on the root context
  bool small_fused = true;        // LAMD_SMALL_FUSED=0: small batches take the partitioning path even with a cache
  bool last_small_fused = false;  // the previous small batch of this lane ran k_ecmult_small (its plan holds P_DENSE)
  size_t last_small_n = 0;
  double keyed_min_uses = 6.0;   // average signatures per distinct key that pays for a (comb) table
  double keyed_dense_uses = 48.0;  // ... and for the 10-tooth comb (512 entries per key)
  int keyed_teeth = 0;             // 0 = choose by re-use, 7 or 10 = force that comb (LAMD_KEYED_TEETH)
  int last_mode = 0;
  size_t last_n = 0;
  bool last_keyed_call = false;
  devbuf in_a, in_b, in_c, out;       // staging for the host-buffer API
  devbuf g_msgs, g_off, g_ids, g_rowbase, g_hash, g_sig, g_pub, g_malformed, g_ok, g_verdict;
  // gossip_store calls (lamd_store.hip).  audit: image, the host walk's arrays, signers, scid index, per-record bytes; repair: reasons, sizes, offsets,
  // block sums, node table, and the output image; digest build: its tables and the sort's workspace; range replies: plan arrays, the messages;
  // range comparison: the peers' messages, classes, lists, the sorts' workspace, and the queries it writes; directory build: candidates, keys,
  // permutations, the sorts' workspace; short_channel_ids replies: the queries, per-occurrence and per-node arrays, offsets, and the messages.
  // channel_update, node_announcement and channel_announcement reception, the txout replies included (rx, rx_out, t_rx: one call at a time): the
  // batch, its per-message, per-row and per-slot arrays, the plan, and the added records.
  // t_audit / t_rep: the stage boundaries of an audit and of a repair's own stages; t_dig: those of a digest or directory build, a range reply, a
  // comparison, a short_channel_ids reply, a stream index build or a timestamp filter reply; t_rx: those of a reception call (channel_update, node_announcement, channel_announcement, txout replies)
  struct store_ws {
    devbuf img, host, ids, tab, out, rep, pack, dig, rng, rng_out, cmp, cmp_out, dir, sq, sq_out, ts, ts_msg, ts_out, rx, rx_out;
    stage_timer<6> t_audit;
    stage_timer<4> t_rep;
    stage_timer<6> t_dig;
    stage_timer<7> t_rx;
    void destroy_events() { t_audit.destroy(); t_rep.destroy(); t_dig.destroy(); t_rx.destroy(); }
  } store;
  // text front ends (lamd_frontends.hip: lamd_bolt11_check_batch, lamd_checkmessage_batch, lamd_bolt12_check_text_batch): the per-row columns; events in
  // front of the front-end kernel, behind it, behind the merge; what they measured last: front end, curve work + merge
  struct text_ws {
    devbuf cols;
    stage_timer<3> t;
    double ms[2] = {0, 0};
    void destroy_events() { t.destroy(); }
  } text;
  // timing
  bool timing = false;
  bool ev_recorded = false;
  int ecmult_waves = 3;
  bool pairs = false;              // LAMD_PAIRS=1 (experiment, parity-green, measured slower: DESIGN.md 4): the table-driven ecmult of a large call pairs first (k_ecmult_keyed_pairs)
                                   // instead of one mixed addition per table entry (k_ecmult_keyed<false>)
  bool group_rows = true;          // LAMD_GROUP=0: the row lists of a large call stay in arrival order (no k_group_*)
  devbuf g_cnt, g_base, g_rank, g_touched, g_list7, g_list10;   // k_group_*: histogram / range bases over the cache's entry ids, rank per listed row, touched entries, grouped lists
  devbuf pairs_ws;                 // parking slots of k_ecmult_keyed_pairs (PAIRS_SLOTS x 48 bytes per resident lane)
  size_t prep_batch = 16;  // signatures sharing one scalar inversion in the ECDSA prep (LAMD_PREP_BATCH)
  size_t prep_min_threads = 0;  // LAMD_PREP_MIN_THREADS: fewest prep threads of a large batch (0 = 256 per CU)
  u64 hash_seed = 0x243F6A8885A308D3ULL;
  size_t chunk = CHUNK_DEFAULT;  // LAMD_CHUNK_ROWS (tests force small chunks to exercise the splitting)
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double last_ms[4] = {0, 0, 0, 0};
  // the dominant kernel alone: an event pair right around every large table-driven ecmult launch while timing is on (the
  // start event sits AFTER the waits for the prep / cold streams, so the interval is the launch itself, as rocprofv3 sees it);
  // read and summed per mode (ECDSA / BIP-340) by lamd_synchronize(), reset by lamd_set_timing()
  static const int MARK_SLOTS = 16;
  hipEvent_t ev_mark[MARK_SLOTS][MAX_LANES + 1] = {};  // lamd_results_mark(): one event per lane stream (+ the context's own)
  bool mark_set[MARK_SLOTS] = {};
  int mark_only[MARK_SLOTS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};  // lamd_results_mark_last(): the one lane whose event the slot holds (-1: every lane's)
  static const int KEV = 64;
  hipEvent_t kev[KEV][2] = {};
  int kev_mode[KEV] = {};
  int kev_n = 0;
  double keyed_ms_sum[2] = {0, 0};
  size_t keyed_launches[2] = {0, 0};
  // streaming queues (pinned host staging): QUEUE_SETS sets, one being filled while up to QUEUE_SETS - 1 flushed ones are
  // in flight (each on the lane picked at its flush), collected oldest first
  struct queue {
    // ONE pinned block per (set, kind), laid out for `cap` rows: keys | signatures | hashes (the order a flush sends them); h_c / h_b / h_a point
    // into it.  A flush that fills the set exactly (n == cap: a producer that reserves its batch in one go) crosses the bus as ONE copy.
    u8 *h_blk = nullptr;
    u8 *h_a = nullptr, *h_b = nullptr, *h_c = nullptr, *h_ok = nullptr;  // hash/msg, sig, key (inside h_blk); verdicts (own block)
    size_t cap = 0, n = 0;
    static size_t key_bytes_padded(size_t cap, size_t keybytes) { return (cap * keybytes + 63) & ~(size_t)63; }
    static size_t blk_bytes(size_t cap, size_t keybytes) { return key_bytes_padded(cap, keybytes) + cap * 96; }
    struct span { size_t row0; u32 ticket0; size_t count; };
    std::vector<span> tickets;  // rows [row0, row0 + count) of this queue return as verdicts [ticket0, ...) of the staging set
    // rows that were queued IN PLACE (lamd_queue_*_batch_inplace): they have a row range in the set and in its device twin like any other, but
    // their bytes stay in the caller's (registered) memory and cross the bus from there -- no host copy at all.  Ordered by row0, disjoint.
    struct foreign_span { size_t row0, count; const u8 *a, *b, *c; };
    std::vector<foreign_span> foreign;
    devbuf d_blk, d_ok;   // the device twin of h_blk (same layout), the verdicts
    hipEvent_t ev_keys = nullptr, ev_sigs = nullptr, ev_all = nullptr;  // behind the three H2D copies of a flush on the copy stream
    bool small_flush = false;   // this flush ran as ONE k_small_verify launch over the staging rows themselves (h_ok + cap: the rows' shapes)
  };
  struct queue_set {
    queue q[Q_KINDS];
    hipEvent_t done = nullptr;
    size_t rows = 0;  // triples queued into this set so far = the next ticket
  } qs[QUEUE_SETS];
  int q_open = 0;                 // the set being filled, -1 when every set is in flight
  int q_fifo[QUEUE_SETS] = {0};   // flushed sets, oldest first
  int q_inflight = 0;
  size_t last_flush_inplace_rows = 0;   // rows the last successful lamd_flush sent from the callers' registered memory (lamd_info)
  // Lanes: the device-pointer entry points rotate over LAMD_LANES (default 6) complete sub-contexts (own streams and
  // workspaces, the G table shared), so that the latency-bound front end of one call (key de-duplication, the count
  // read-back, table building) runs under the VALU-bound ecmult kernels of the calls before it.  A lane's `peer` is the
  // next lane; the root context (the handle the caller holds) keeps its own stream for staging, queues, generators.
  lamd_ctx *lane[MAX_LANES] = {};
  int nlanes = 0;
  lamd_ctx *peer = nullptr;
  lamd_ctx *last_lane = nullptr;
  lamd_ctx *last_chunk_lane = nullptr;  // where the last chunk of this lane's last call ran (itself or its peer)
  bool is_lane = false;
  int next_lane = 0;
  hipEvent_t ev_lane = nullptr, ev_join = nullptr;
  // root: the large table-driven ecmult launches of successive calls run one after the other (LAMD_ECMULT_CHAIN, see ecmult_stage)
  hipEvent_t ev_ecm[MAX_LANES + 1] = {};
  int ecm_last = -1;
  int ecm_chain = 0;
  size_t ecm_chain_min = 65536;
  u32 ecm_tail = 131072;             // LAMD_ECMULT_TAIL: work items of the low-priority second part (LAMD_ECMULT_CHAIN=2)
  hipStream_t stream_lo = nullptr;   // lanes, LAMD_ECMULT_CHAIN=2: lowest-priority stream of that second part
  hipEvent_t ev_lo_go = nullptr, ev_lo_done = nullptr;
};

#define HIPCHK(ctx, call)                                                                           \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
      return LAMD_ERR_HIP;                                                                          \
    }                                                                                               \
  } while (0)

static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// the input of lamd_selftest and of the arithmetic debuggers: one st_in per lane
constexpr int ST_LANES = 64;
constexpr int ST_WORDS = 512;  // output words per lane
struct st_in { u32 a[8], b[8]; u8 hash[32], sig[64], pub33[33], pad[3]; };

// An error return of a call that has queued work on lane L (the context itself, or one of its lanes): queued copies may still read the vectors of the
// frame that is being left, so the stream drains first; the caller reads the error on the handle it holds.
static inline int drain_fail(lamd_ctx *ctx, lamd_ctx *L, int code) {
  (void)hipStreamSynchronize(L->stream);
  if (L != ctx) ctx->err = L->err;
  return code;
}
// HIPCHK for such a call: needs `ctx` and `L` in scope
#define STCHK(call) \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) { L->err = std::string(#call) + ": " + hipGetErrorString(e_); return drain_fail(ctx, L, LAMD_ERR_HIP); } } while (0)

// ---- the seam: what lamd_engine.hip defines for the other units.  Everything else of the core is static there.
// (Above: the types and constants they share with it, wave_alloc, and st_in, the one input format of lamd_selftest and the debuggers.)
int ensure(lamd_ctx *ctx, devbuf *b, size_t bytes);   // grows a workspace (drains the device before it frees the old one)
int pick_lane(lamd_ctx *root, lamd_ctx **out);        // the lane the next device-pointer call runs on, ordered behind the context's own stream
int cache_maybe_reset(lamd_ctx *root);
bool small_path(const lamd_ctx *ctx, size_t rows);    // does a call of `rows` rows from host memory take the one-launch path (run_small)?
int run_small(lamd_ctx *ctx, int mode, size_t n, const u8 *a, const u8 *sig, const u8 *key, int keylen, size_t keystride, u8 *ok,
              const u8 *d_a32 = nullptr, const u8 *d_gate = nullptr);
int run_device(lamd_ctx *ctx, int mode, size_t n, const u8 *d_a, const u8 *d_sig, const u8 *d_key, int keylen, size_t keystride, u8 *d_ok,
               u8 *keyok_out = nullptr);
int recover_device(lamd_ctx *ctx, size_t n, const u8 *d_hash, const u8 *d_sig, const u8 *d_recid, u8 *d_pub33, u8 *d_ok);
int gossip_device(lamd_ctx *ctx, size_t n, const u8 *d_msgs, const u64 *d_off, const u8 *d_ids, const u64 *d_rowbase, size_t rows, int8_t *d_verdict,
                  const u64 *d_len = nullptr);
// the validity byte of n 33-byte keys (k_keys on `stream`); qwords: 64 bytes of workspace per key
int launch_key_validity(lamd_ctx *ctx, hipStream_t stream, size_t n, const u8 *key33, u32 *qwords, u8 *keyok);

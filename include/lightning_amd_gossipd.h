/* lightning_amd_gossipd.h -- batched gossip ingest: the receive side of Core Lightning's gossipd
 * (gossipd/gossipd.c:172-286 handle_recv_gossip -> gossipd/gossmap_manage.c:620-753 channel_announcement,
 * :878-1120 channel_update, :1129-1248 node_announcement, :753-872 get_txout reply, :1255-1342 queued messages,
 * :1358-1390 new block) restructured around ONE device call per drained queue instead of one libsecp256k1 call per
 * signature.  C ABI, host code in liblightning_amd_cln.so (lightning_amd/csrc/gossip_ingest.cpp).
 *
 * How a batch runs (lamd_gossipd_process):
 *   1. every queued message (what connectd forwards, connectd/multiplex.c:829-842: source peer + raw wire message) is
 *      framed on the host, and the filters that need no curve arithmetic are evaluated against the state as it is
 *      BEFORE the batch: malformed framing / r,s >= n, unknown chain_hash, unreasonable timestamp, short_channel_id
 *      already known / pending / in the txout-failure set;
 *   2. everything whose outcome can depend on a signature is verified in one lamd_sigcheck_gossip_batch() call
 *      (identical (message, signer) pairs -- the same announcement relayed by several peers -- once); announcements
 *      that step 1 already knows it will drop only have their two bitcoin keys parsed (lamd_pubkey_parse_batch),
 *      because fromwire_channel_announcement rejects an invalid key as "Malformed" BEFORE any of those filters
 *      (bitcoin/pubkey.c:102-113);
 *   3. the messages are applied strictly in arrival order with the reference's own control flow, the precomputed
 *      verdicts standing in for the sigcheck_*() calls -- so every ordering dependency (a channel_update waits for its
 *      channel_announcement to be accepted and confirmed, :1060-1097; a duplicate announcement is dropped only if the
 *      earlier copy was accepted, :673-676) resolves exactly as it does one message at a time.
 * What is kept: the announce/update/node maps, the pending and too-early announcement maps with their queued
 * channel_updates and node_announcements, the txout-failure set, and an append-only store (records with timestamps,
 * deletions marked) together with the byte image of the gossip_store FILE those records make (common/gossip_store.h:15-59), pruning
 * (prune_network) and dying / spent channels (channel_spent, new_block).  What is not: compaction, the seeker, local (known_amount)
 * announcements, and the peers' queries (query_channel_range is answered from a store image by lamd_channel_range_reply_batch and the
 * seeker's comparison of peers' reply_channel_range with the store is lamd_channel_range_compare_batch, include/lightning_amd.h; the
 * query_short_channel_ids responder is lamd_short_channel_ids_reply_batch and a peer's gossip_timestamp_filter is answered by
 * lamd_timestamp_filter_reply_batch, both from the same image; the per-peer state of a stream -- gossip_rcvd_filter, the 60-second
 * timer, dev_suppress_gossip -- stays with the caller; the channel_update half of step 1 - 3 against such an image, look-ups and replay on
 * the device, is lamd_channel_update_receive_batch, the node_announcement half lamd_node_announcement_receive_batch, and the
 * channel_announcement half with its txout replies lamd_channel_announcement_receive_batch / lamd_channel_announcement_confirm_batch: with them
 * every gossip message can be received against an image; what stays with the caller there are the pending, too-early and txout-failure maps
 * themselves, new_block's promotion of early entries, reprocess_queued_msgs, the warnings' texts and the seeker) -- events tell the host daemon what the reference would have done (send a warning, ask lightningd for a txout,
 * append to / delete from / re-flag the store) and it does the I/O.
 *
 * Everything observable is reported through the event callback, in the order the reference would produce it; texts
 * (warnings, traces) are the reference's own format strings. */
#ifndef LIGHTNING_AMD_GOSSIPD_H
#define LIGHTNING_AMD_GOSSIPD_H
#include <stddef.h>
#include <stdint.h>

#include "lightning_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lamd_gossipd lamd_gossipd;

enum lamd_gossipd_event_kind {
	LAMD_GEV_WARNING = 1,        /* queue_peer_msg(towire_warningfmt(text)) to peer (gossipd.c:277-283, gossmap_manage.c:589-596) */
	LAMD_GEV_GET_TXOUT = 2,      /* towire_gossipd_get_txout(scid) to lightningd (gossmap_manage.c:749-750, :1385-1386) */
	LAMD_GEV_STORE_ADD = 3,      /* gossip_store_add(data, timestamp): record number `index`, wire type `type` */
	LAMD_GEV_STORE_DEL = 4,      /* gossip_store_del(record `index`) */
	LAMD_GEV_STORE_SET_TS = 5,   /* gossip_store_set_timestamp(record `index`, timestamp) (gossmap_manage.c:950-951) */
	LAMD_GEV_PEER_UPDATE = 6,    /* tell_lightningd_peer_update: scid, values[0..4] = fee_base, fee_ppm, cltv, htlc_min, htlc_max */
	LAMD_GEV_TRACE = 7,          /* status_peer_trace(peer, text): "Bad gossip order: ..." (gossmap_manage.c:576-579), the Received ... lines */
	LAMD_GEV_QUERY_CHANNEL = 8,  /* query_unknown_channel(peer, scid) (gossmap_manage.c:908) */
	LAMD_GEV_QUERY_NODE = 9,     /* query_unknown_node(peer, node id in data) (gossmap_manage.c:1232) */
	LAMD_GEV_GOOD_GOSSIP = 10,   /* peer_supplied_good_gossip(peer, 1) */
	LAMD_GEV_TXOUT_FAILED = 11,  /* txout_failures_add(scid) (gossmap_manage.c:868-869) */
	LAMD_GEV_STORE_FLAG = 12,    /* gossip_store_set_flag(record `index`, values[1] = GOSSIP_STORE_DYING_BIT) (gossmap_manage.c:367-372,1472-1495) */
	LAMD_GEV_STORE_WRITE = 13    /* only with config.emit_store_writes: pwrite(gossip_store, data, len, offset = values[0]) -- applying these in
	                              * order to a file reproduces lamd_gossipd_store_image() byte for byte */
};

typedef struct lamd_gossipd_event {
	int kind;
	int has_peer;
	uint8_t peer[33];
	uint64_t scid;
	uint64_t index;      /* store record number */
	uint32_t type;       /* wire type of a store record */
	uint32_t timestamp;
	uint64_t values[5];
	const char *text;    /* NUL-terminated, valid during the callback */
	const uint8_t *data; /* valid during the callback */
	size_t len;
} lamd_gossipd_event;

typedef void (*lamd_gossipd_event_fn)(void *user, const lamd_gossipd_event *ev);

typedef struct lamd_gossipd_config {
	uint8_t chain_hash[32];   /* chainparams->genesis_blockhash as it appears on the wire */
	uint8_t our_id[33];       /* daemon->id: updates for channels INTO this node are reported (gossmap_manage.c:973-983) */
	uint32_t blockheight;     /* daemon->current_blockheight (0 = unknown) */
	uint64_t now;             /* seconds since the epoch; 0 = read the clock at every lamd_gossipd_process() */
	uint32_t prune_interval;  /* GOSSIP_PRUNE_INTERVAL: 1209600 (0 = that default) */
	uint8_t store_version;    /* first byte of the gossip_store image: 0 = GOSSIP_STORE_VER (0 << 5 | 16, gossip_store.c:24); a minor version
	                           * below 16 writes no uuid record (the fixtures under contrib/pyln-client/tests/data are v15) */
	uint8_t emit_store_writes; /* 1 = report every write to the image as a LAMD_GEV_STORE_WRITE event */
	uint8_t store_uuid[32];   /* the uuid record's content (the reference draws it at random, gossip_store.c:186-197) */
} lamd_gossipd_config;

/* A verification back end with the signature of lamd_sigcheck_gossip_batch / lamd_pubkey_parse_batch.  The product uses
 * the engine (lamd_gossipd_new with a context); the hook exists so that the host logic can be tested on a machine
 * without a GPU against a sequential model -- the library itself contains no CPU verification.
 * node_ids33 is NULL when no message of the batch has an explicit signer (a batch without channel_update, as for
 * lamd_sigcheck_gossip_batch); a back end must not read it then. */
typedef int (*lamd_gossipd_sigcheck_fn)(void *user, size_t n, const uint8_t *msgs, const uint64_t *off, const uint8_t *node_ids33,
					int8_t *verdict);
typedef int (*lamd_gossipd_keyparse_fn)(void *user, size_t n, const uint8_t *pub33, uint8_t *ok);

/* ctx: the engine context verdicts come from (NULL only when lamd_gossipd_set_backend() is called before the first
 * lamd_gossipd_process()).  Returns NULL on allocation failure. */
lamd_gossipd *lamd_gossipd_new(lamd_ctx *ctx, const lamd_gossipd_config *cfg, lamd_gossipd_event_fn on_event, void *user);
void lamd_gossipd_free(lamd_gossipd *g);
void lamd_gossipd_set_backend(lamd_gossipd *g, lamd_gossipd_sigcheck_fn sigcheck, lamd_gossipd_keyparse_fn keyparse, void *user);

/* connectd -> gossipd: one raw peer message (type 256/257/258) from source_peer33 (may be NULL: generated locally).
 * Queues only; LAMD_ERR_STATE when more than 500 000 messages are waiting (connectd drops there, multiplex.c:829-833). */
int lamd_gossipd_push(lamd_gossipd *g, const uint8_t *source_peer33, const uint8_t *msg, size_t len);
/* n messages at once: message i is msgs + off[i] .. off[i+1] from source_peers33 + peer_stride*i (source_peers33 NULL: no peer;
 * peer_stride 0: one peer for all) */
int lamd_gossipd_push_batch(lamd_gossipd *g, size_t n, const uint8_t *source_peers33, size_t peer_stride, const uint8_t *msgs,
			    const uint64_t *off);
/* Drains the queue as ONE batch (see above).  Returns the number of messages applied, or a negative LAMD_ERR_*: after an
 * engine error nothing is lost -- the messages that were not applied are back at the head of the queue, in order, and no peer
 * has been sent a warning because of it.
 * NOT re-entrant: the event callback runs inside this call and must not call lamd_gossipd_process / _txout_reply[_batch] /
 * _new_block (they return LAMD_ERR_STATE); collect the LAMD_GEV_GET_TXOUT requests and answer them after it returns.
 * lamd_gossipd_push[_batch] from the callback is fine. */
long lamd_gossipd_process(lamd_gossipd *g);
/* lightningd's answer to LAMD_GEV_GET_TXOUT (gossmap_manage.c:753-872); script_len 0 = no unspent output.  Channel_updates
 * and node_announcements that were waiting are verified (one batch) and applied once nothing is pending any more. */
int lamd_gossipd_txout_reply(lamd_gossipd *g, uint64_t scid, uint64_t sat, const uint8_t *script, size_t script_len);
/* n replies in order (reply i's script: scripts + script_off[i] .. script_off[i+1]).  *applied (may be NULL) = how many
 * replies took effect; on an error return the caller resumes with reply *applied + 1 (reply *applied itself registered its
 * channel; the updates that waited for it stay queued until the next successful reply or process()). */
int lamd_gossipd_txout_reply_batch(lamd_gossipd *g, size_t n, const uint64_t *scids, const uint64_t *sats, const uint8_t *scripts,
				   const uint64_t *script_off, size_t *applied);
/* gossmap_manage_new_block (:1389-1437): too-early announcements that are now deep enough become pending; dying channels whose
 * deadline has come are removed (kill_spent_channel -> remove_channel, :296-387) */
int lamd_gossipd_new_block(lamd_gossipd *g, uint32_t blockheight);
/* gossmap_manage_channel_spent (:1439-1497): lightningd saw the funding output of `scid` spent at `blockheight`: the channel is
 * marked dying in the store (chan_dying record, DYING flag on its announcement, updates and -- if every channel of a node is dying
 * -- that node's announcement) and removed 72 blocks later by lamd_gossipd_new_block(). */
int lamd_gossipd_channel_spent(lamd_gossipd *g, uint32_t blockheight, uint64_t scid);
/* prune_network (:398-470): removes every channel one of whose directions has no channel_update newer than now - prune_interval
 * (delete_chan tombstone, records marked deleted, node_announcements deleted / moved behind a surviving channel_announcement).
 * The reference runs it from a timer every prune_interval / 4; here the host daemon owns the timer.  Returns the number of
 * channels pruned. */
long lamd_gossipd_prune(lamd_gossipd *g);
/* The gossip_store file as the reference's gossip_store.c would hold it after the same operations (common/gossip_store.h:15-59:
 * version byte, then struct gossip_hdr {flags, len, crc32c seeded with the timestamp, timestamp} + message per record; a v16
 * store starts with the uuid record).  Store events carry the record's offset in values[0] (the offset gossip_store_add()
 * returns: of the message, after its header).  Valid until the next call that changes the ingest. */
size_t lamd_gossipd_store_image(const lamd_gossipd *g, const uint8_t **data);
void lamd_gossipd_set_time(lamd_gossipd *g, uint64_t now);   /* called from an event callback: takes effect when lamd_gossipd_process() returns */

typedef struct lamd_gossipd_stats {
	uint64_t messages;          /* applied so far */
	uint64_t batches;           /* device calls for signatures */
	uint64_t verified_messages; /* messages sent to the device for signatures (after de-duplication) */
	uint64_t verified_sigs;     /* signatures those carried (4 per channel_announcement) */
	uint64_t keyparse_messages; /* announcements whose bitcoin keys only were parsed */
	uint64_t duplicates;        /* identical (message, signer) pairs verified once */
	uint64_t late_verifies;     /* sigcheck needed during the ordered replay that the plan had not foreseen (0 expected) */
	uint64_t channels, nodes, pending, early, queued_updates, queued_nodes, store_records;
	uint64_t run_updates;       /* channel_updates applied by all cores, as runs of plain updates of known channels (the others are replayed one by one) */
	uint64_t sub_batches;       /* planning stages run (a drained queue is cut into sub-batches: the next one is planned while one is applied) */
	uint64_t overlapped_stages; /* of those, planning stages that ran under an apply pass */
	uint64_t run_announcements; /* channel_announcements entered into the map of waiting announcements by all cores, as runs of plain announcements */
	uint64_t run_nodes;         /* node_announcements applied by all cores, as runs of plain announcements of known nodes (gossmap_manage.c:1162-1243) */
} lamd_gossipd_stats;
void lamd_gossipd_get_stats(const lamd_gossipd *g, lamd_gossipd_stats *out);
/* diagnostic: the ingest's open-addressing maps against std::unordered_map over `ops` random operations; 0 = every check passed */
long lamd_gossipd_selftest_maps(uint64_t seed, long ops);

#ifdef __cplusplus
}
#endif
#endif

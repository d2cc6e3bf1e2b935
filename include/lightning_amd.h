/* lightning_amd -- MI355X (gfx950) batched secp256k1 signature verification.
 *
 * C ABI of liblightning_amd.so: the drop-in boundary for Core Lightning's signature-check
 * hot path.  Every entry point names the reference interface it replaces (paths relative to
 * the Core Lightning tree, v26.06.6).  Plain pointers and sizes only; all byte formats are the
 * SERIALISED forms the reference handles at its own boundaries (the opaque in-memory
 * secp256k1_pubkey / secp256k1_ecdsa_signature layouts are implementation-defined and never
 * cross this ABI):
 *     hash / sighash / BIP-340 message : 32 raw bytes   (struct sha256_double, bitcoin/shadouble.h:9-11)
 *     ECDSA signature                  : 64-byte compact big-endian r||s (wire/fromwire.c:188-199)
 *     public key                       : 33-byte SEC1 compressed (struct node_id, common/node_id.h:11-13;
 *                                        pubkey_to_der, bitcoin/pubkey.c:26-34) or 65-byte uncompressed
 *     BIP-340 signature / x-only key   : 64 / 32 raw bytes (struct bip340sig, bitcoin/signature.h:145-147)
 *
 * Verdict convention: ok[i] = 1 iff the reference would have accepted, i.e.
 *     parse_ok(signature) && parse_ok(key) && verify_ok
 * so a host-side parse failure and a device-side reject are indistinguishable from the
 * reference's combined outcome.  Every byte the library writes into an `ok` buffer, on the host or on
 * the device, is exactly 0 or 1 once the call's work is complete (for the *_device entry points: once
 * the stream has reached the end of the call).  The kernels of one call hand rows to each other through
 * markers in that byte -- 2: x(R) = r or the recovered point found, parity / compression still to be
 * decided; 3: the bare formulas met Z = 0, the complete ones decide -- but those are internal and never
 * leave the lane's workspace.  Callers may therefore test `if (!ok[i])`; a byte above 1 is a bug in the
 * library, never an accept.  There is NO CPU fallback: without a working HIP device every
 * call returns LAMD_ERR_NO_DEVICE / LAMD_ERR_HIP and the caller must fail closed.
 *
 * Threading: a context owns one device, one stream and its staging buffers; calls on one
 * context must be serialised by the caller (the reference's daemons are single-threaded:
 * gossipd/gossipd.c:620-625, channeld/channeld.c:7063-7121).  Use one context per thread/GPU.
 */
#ifndef LIGHTNING_AMD_H
#define LIGHTNING_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lamd_ctx lamd_ctx;

enum {
	LAMD_OK = 0,
	LAMD_ERR_NO_DEVICE = -1, /* no usable HIP device (or wrong architecture) */
	LAMD_ERR_HIP = -2,       /* a HIP call failed; lamd_last_error() has the text */
	LAMD_ERR_ARG = -3,       /* bad argument (NULL, unsupported key length, ...) */
	LAMD_ERR_NOMEM = -4,
	LAMD_ERR_STATE = -5      /* streaming API misuse (poll before flush, queue full, ...) */
};

/* A context is NOT thread-safe -- including the single-item veneers and every host-buffer call of <= 4096 rows, which share one pinned block
 * and one completion word per context: one context per calling thread, or serialise the calls (lamd_multi_* below runs one context per device
 * behind its own lock).  A latency-path call busy-waits for its completion word for at most LAMD_SPIN_US microseconds (default 2000), then
 * blocks in the runtime.  Every entry point returns a
 * LAMD_ERR_* code (< 0) or a documented non-negative value; lamd_last_error() describes the last failure. */
/* ---- lifecycle.  Replaces the process-global secp256k1_ctx set up in common/setup.c:58
 * (secp256k1_ctx = wally_get_secp_context(), common/utils.c:16): the one-time work here is the
 * upload/build of the static table of G multiples in HBM.
 * Hardware queues: the context runs its calls on several HIP streams ("lanes", LAMD_LANES) that only overlap when each has a
 * hardware queue of its own.  ROCm reads GPU_MAX_HW_QUEUES (default 4) at the runtime's FIRST call.  PRECONDITION for full
 * throughput: the host process exports GPU_MAX_HW_QUEUES=16 (or setenv()s it) BEFORE its first HIP call -- the library does not
 * touch the process environment.  lamd_init() records what it found (lamd_info.hw_queues_env; 0 = unset, i.e. the runtime's 4:
 * the lanes then share queues and the pipelined loop runs ~7 % slower, nothing else changes).  Create the context BEFORE an RCCL communicator (ncclCommInitRank / torch.distributed
 * init_process_group): RCCL's own streams otherwise take hardware queues first and the lanes end up sharing one (measured:
 * -8 % on the 2 M-row step).  Correctness does not depend on either (tests run at 4, 16 and 32 queues). */
int lamd_init(lamd_ctx **ctx, int device);
void lamd_shutdown(lamd_ctx *ctx);
const char *lamd_last_error(const lamd_ctx *ctx);
const char *lamd_version(void);

/* ---- batch verification, host buffers in, host verdicts out (H2D + kernels + D2H, synchronous).
 * A call of <= 4096 rows is ONE kernel launch (k_small_verify, a grid of 64-row blocks): the rows travel through pinned device-mapped
 * memory, each verification is split over eight waves, the verdict bytes come back the same way (LAMD_SMALL_KERNEL=0 sends such calls
 * down the general path).  A key such calls bring for the second time gets its comb table built and cached, so recurring keys (a peer's
 * node id, a channel's htlc key) are cache hits from their third sight on.
 *
 * lamd_verify_ecdsa_batch: n independent check_signed_hash() calls (bitcoin/signature.c:174-192,
 * decl bitcoin/signature.h:85-87).  publen is 33 or 65 for every key of the batch; key i is at
 * pub + i*pubstride.  With publen 33 this is check_signed_hash_nodeid() (common/node_id.c:72-80).
 * 65-byte keys may be 0x04 or hybrid 0x06/0x07, as secp256k1_ec_pubkey_parse accepts them.
 *
 * Key columns (every pubstride / keystride of this header, host or device memory): only the publen bytes of each key are read, so the
 * buffer need hold (n-1)*pubstride + publen bytes -- the keys may be the last field of an array of structs; pubstride < publen is
 * LAMD_ERR_ARG.  Alignment: the byte columns (hashes, messages, signatures, keys, recids, sighash types, preimage / message / TLV blobs,
 * node ids, verdicts and key outputs) may start at ANY address, host or device; arrays of wider elements need their natural alignment --
 * the uint64 offset, start, length, rowbase and amount arrays 8 bytes, the uint32 arrays 4. */
int lamd_verify_ecdsa_batch(lamd_ctx *ctx, size_t n, const uint8_t *hash32, const uint8_t *sig64,
			    const uint8_t *pub, size_t publen, size_t pubstride, uint8_t *ok);

/* n independent check_schnorr_sig() calls (bitcoin/signature.c:408-430, decl signature.h:129-131):
 * BIP-340 verification of a 32-byte message under an x-only key. */
int lamd_verify_schnorr_batch(lamd_ctx *ctx, size_t n, const uint8_t *msg32, const uint8_t *xonly32,
			      const uint8_t *sig64, uint8_t *ok);

/* ---- the same with every buffer already resident in HBM (device pointers), asynchronous: the work is ordered after
 * whatever is already queued on the context's stream (lamd_stream()) and the verdicts are complete after
 * lamd_synchronize(), or, without blocking the host, for a stream passed to lamd_stream_wait_results().  Successive
 * calls rotate over LAMD_LANES internal lanes (default 6; own streams and workspaces) so that one call's key
 * de-duplication and table building run under the ecmult kernels of the calls before it; LAMD_LANES=1 turns that off
 * (strictly one stream).  d_ok is never read and is written once per call, with final verdicts (one device-to-device copy at the
 * end of the call): calls in flight at the same time may be handed the same verdict buffer.
 * This is what bench.py times. */
int lamd_verify_ecdsa_batch_device(lamd_ctx *ctx, size_t n, const void *d_hash32, const void *d_sig64,
				   const void *d_pub, size_t publen, size_t pubstride, void *d_ok);
int lamd_verify_schnorr_batch_device(lamd_ctx *ctx, size_t n, const void *d_msg32, const void *d_xonly32,
				     const void *d_sig64, void *d_ok);
void *lamd_stream(lamd_ctx *ctx); /* hipStream_t */
int lamd_synchronize(lamd_ctx *ctx);
/* `stream` (hipStream_t) waits, on the device, for every verification submitted so far */
int lamd_stream_wait_results(lamd_ctx *ctx, void *stream);
/* The same in two phases: lamd_results_mark() remembers "everything submitted so far" in slot 0..15 (events on the lanes' streams,
 * nothing waits); lamd_stream_wait_mark() later makes `stream` wait for exactly that work.  A consumer that joins late -- after
 * the next batch has been submitted -- keeps its stream's wait short: a wait that sits in a hardware queue for a whole batch
 * holds up every other stream that shares the queue (bench.py's collective path: the all-gather of step k is issued after the
 * calls of step k+1). */
int lamd_results_mark(lamd_ctx *ctx, int slot);
/* ... "the call submitted last" only: ONE event, on the lane that ran it -- what the consumer of that call's verdict buffer needs (bench.py's
 * per-call all-gathers); lamd_stream_wait_mark() then waits for that one event. */
int lamd_results_mark_last(lamd_ctx *ctx, int slot);
int lamd_stream_wait_mark(lamd_ctx *ctx, int slot, void *stream);
/* verification submitted from now on waits, on the device, for what `stream` holds at this moment */
int lamd_wait_stream(lamd_ctx *ctx, void *stream);
/* the same for one event (hipEvent_t) the caller recorded: verification submitted from now on waits, on the device, for it */
int lamd_wait_event(lamd_ctx *ctx, void *event);

/* ---- single-item veneers with the reference's exact boolean semantics (1 = true, 0 = false,
 * < 0 = engine error: treat as failure).  They run a batch of one through the one-launch path above (0.17-0.21 ms under a key
 * the cache knows, ~0.9 ms at a key's first sight on one MI355X); callers on the hot path should batch. */
int lamd_check_signed_hash(lamd_ctx *ctx, const uint8_t hash32[32], const uint8_t sig64[64],
			   const uint8_t *pubkey, size_t publen);          /* bitcoin/signature.h:85-87 */
int lamd_check_signed_hash_nodeid(lamd_ctx *ctx, const uint8_t hash32[32], const uint8_t sig64[64],
				  const uint8_t node_id33[33]);             /* common/node_id.h:80-82 */
int lamd_check_schnorr_sig(lamd_ctx *ctx, const uint8_t hash32[32], const uint8_t pubkey33[33],
			   const uint8_t bip340sig64[64]);                   /* bitcoin/signature.h:129-131 */

/* ---- n independent check_tx_sig() calls (bitcoin/signature.c:194-221, decl signature.h:120-124) on caller-built
 * BIP143 preimages: preimage i = preimages[off[i]..off[i+1]) is what wally_tx_get_btc_signature_hash() hashes for
 * (tx, input, script, amount, sighash_type) -- signature.c:145-148.  The device applies the sighash-type gate
 * (:206-211: SIGHASH_ALL, or SINGLE|ANYONECANPAY only with a witness script), double-SHA256s the preimage and
 * verifies.  This is also the shape of onchaind's fee grind (one signature/key against many candidate
 * transactions, onchaind/onchaind.c:389-438): pass the same sig/key n times. */
int lamd_check_tx_sig_batch(lamd_ctx *ctx, size_t n, const uint8_t *preimages, const uint64_t *off,
			    const uint8_t *sighash_type, const uint8_t *has_witness_script,
			    const uint8_t *sig64, const uint8_t *pub, size_t publen, size_t pubstride, uint8_t *ok);

/* ---- the same from TRANSACTION TEMPLATES: n independent check_tx_sig(tx, input_num, script, witness_script, key, sig) calls
 * (bitcoin/signature.c:194-221) with the BIP143 signature hash of bitcoin_tx_hash_for_sig() (:120-151, libwally's
 * wally_tx_get_btc_signature_hash with WALLY_TX_FLAG_USE_WITNESS) computed ON THE DEVICE: hashPrevouts / hashSequence /
 * hashOutputs, the preimage and its double SHA-256 are streamed piecewise, nothing is serialised on the host.
 * Row i describes one (transaction, input, signature):
 *   version[i], locktime[i]
 *   inputs40 + 40*in_off[i] .. in_off[i+1]   : the transaction's inputs, 40 bytes each: txid (32, as hashed) | vout u32 LE | nSequence u32 LE
 *   input_num[i]                              : which input the signature is for (>= the number of inputs: verdict 0; the reference asserts)
 *   amount_sat[i]                             : that input's amount (psbt_input_get_amount)
 *   outputs + out_off[i] .. out_off[i+1]      : the n_outputs[i] outputs in wire form (amount u64 LE | CompactSize | scriptPubKey), back to back
 *   scripts + script_off[i] .. script_off[i+1]: the script the reference would hash -- the witness script, or the redeemscript when there is none
 *   sighash_type[i], has_witness_script[i]    : the gate of :206-211 (SIGHASH_ALL, or SINGLE|ANYONECANPAY only with a witness script)
 * All offsets are uint64, arrays of n+1 entries.  The Elements branch (:136-143) is out of scope. */
int lamd_check_tx_sig_tx_batch(lamd_ctx *ctx, size_t n, const uint32_t *version, const uint32_t *locktime,
			       const uint8_t *inputs40, const uint64_t *in_off, const uint32_t *input_num, const uint64_t *amount_sat,
			       const uint8_t *outputs, const uint64_t *out_off, const uint32_t *n_outputs,
			       const uint8_t *scripts, const uint64_t *script_off,
			       const uint8_t *sighash_type, const uint8_t *has_witness_script,
			       const uint8_t *sig64, const uint8_t *pub, size_t publen, size_t pubstride, uint8_t *ok);

/* ---- ONE commitment_signed as ONE call: the loop of channeld/channeld.c:2171-2232 (handle_peer_commit_sig).  The reference checks
 *   check_tx_sig(txs[0], 0, NULL, funding_wscript, &remote_funding, &commit_sig)            (:2171)
 * and then, for i = 0 .. tal_count(htlc_sigs) - 1,
 *   check_tx_sig(txs[1+i], 0, NULL, wscript_i, &remote_htlckey, &htlc_sigs[i])              (:2224)
 * one signature per call, failing the peer at the first bad one.  Here the 1 + N rows are one batch -- the largest natural batch of the
 * product, <= 1 + 483 signatures, N of them under ONE key: the BIP143 hashes of all 1 + N inputs are computed on the device from the
 * templates (a row with a long output / input list -- the commitment transaction's one output per HTLC -- is hashed on the host while the
 * rows are packed: SHA-256 is sequential and one lane would need milliseconds for it), a commitment of <= 4096 rows is one small copy and two
 * launches (k_txsig_tx_hash, then k_small_verify taking hashes and sighash-type gate from device memory), larger ones take the batch machinery.
 *   *first_bad = -1: every signature verifies;  0: the commitment signature does not;  1 + i: htlc_sigs[i] is the first that does not
 * -- the reference's order, so the caller prints exactly the warning the reference would ("Bad commit_sig signature ..." with or without
 * "for htlc": include/cln_shim.h check_commit_sigs()).  ok_rows (optional, 1 + n_htlc bytes): every row's verdict.
 * A transaction template is what check_tx_sig() / bitcoin_tx_hash_for_sig() (bitcoin/signature.c:120-151,194-221) read of one (transaction, input):
 * the fields of lamd_check_tx_sig_tx_batch(), one struct per row; `script` is the witness script (funding_wscript; the HTLC output's wscript). */
typedef struct lamd_tx_template {
	uint32_t version, locktime;
	const uint8_t *inputs40;   /* n_inputs x (txid 32, as hashed | vout u32 LE | nSequence u32 LE) */
	uint32_t n_inputs;
	uint32_t input_num;        /* the input the signature is for (0 for commitment and HTLC transactions) */
	uint64_t amount_sat;       /* that input's amount */
	const uint8_t *outputs;    /* the outputs in wire form, back to back (amount u64 LE | CompactSize | scriptPubKey) */
	uint64_t outputs_len;
	uint32_t n_outputs;
	const uint8_t *script;     /* the witness script the signature commits to */
	uint64_t script_len;
} lamd_tx_template;
int lamd_check_commitment_signed(lamd_ctx *ctx, const lamd_tx_template *commit_tx, const uint8_t remote_funding33[33],
				 const uint8_t commit_sig64[64], uint8_t commit_sighash_type,
				 size_t n_htlc, const lamd_tx_template *htlc_txs, const uint8_t remote_htlckey33[33],
				 const uint8_t *htlc_sigs64, const uint8_t *htlc_sighash_types,
				 int64_t *first_bad, uint8_t *ok_rows);

/* ---- BOLT #12 signatures: n independent bolt12_check_signature(fields, messagename, fieldname, key, sig) calls
 * (common/bolt12.c:80-92): merkle_tlv() over the TLV stream minus its signature fields (types 240..1000) and
 * sighash_from_merkle() (common/bolt12_merkle.c:227-318: H("LnLeaf"), H("LnNonce"|first-tlv), H("LnBranch"), tag
 * "lightning"|messagename|fieldname, bitcoin/signature.c:389-405) run on the device in front of the BIP-340 verification of
 * check_schnorr_sig() (:408-430).  Row i: the serialised TLV stream tlvs + off[i] .. off[i+1] (off: n+1 entries) as it came off
 * the wire -- the reference hashes the re-serialised fields, which for a stream fromwire_tlv() accepts (minimal BigSize, ascending
 * types) are these bytes; a stream breaking those rules gets verdict 0 -- key33 + keystride*i the signer (33-byte compressed key:
 * the parity byte is dropped as :417-422 do), sig64 + 64*i the signature. */
int lamd_bolt12_check_signature_batch(lamd_ctx *ctx, size_t n, const uint8_t *tlvs, const uint64_t *off, const char *messagename,
				      const char *fieldname, const uint8_t *key33, size_t keystride, const uint8_t *sig64, uint8_t *ok);
/* the two hashes alone: merkle32 + 32*i = merkle_tlv(), sighash32 + 32*i = sighash_from_merkle() (either may be NULL), ok[i] = the
 * stream obeys the TLV rules and holds at least one non-signature field */
int lamd_bolt12_merkle_batch(lamd_ctx *ctx, size_t n, const uint8_t *tlvs, const uint64_t *off, const char *messagename,
			     const char *fieldname, uint8_t *merkle32, uint8_t *sighash32, uint8_t *ok);

/* n independent secp256k1_ecdsa_recoverable_signature_parse_compact() + secp256k1_ecdsa_recover() calls as made by
 * common/bolt11.c:1021-1046 (invoices without an `n` field) and lightningd/signmessage.c:193: sig64 = r||s, recid 0..3.
 * pub33[i] = the recovered key, compressed (what node_id_from_pubkey() stores), ok[i] = 1; where the library calls would
 * fail (r or s >= n or zero, recid > 3, recid & 2 with r >= p - n, no curve point with that x, infinity) ok[i] = 0 and the
 * key bytes are zero.  There is no low-S rule on this path, as in the reference. */
int lamd_ecdsa_recover_batch(lamd_ctx *ctx, size_t n, const uint8_t *hash32, const uint8_t *sig64, const uint8_t *recid,
			     uint8_t *pub33, uint8_t *ok);
int lamd_ecdsa_recover_batch_device(lamd_ctx *ctx, size_t n, const void *d_hash32, const void *d_sig64, const void *d_recid,
				    void *d_pub33, void *d_ok);

/* ---- the same two call sites FROM THEIR TEXT: the signature half of bolt11_decode() (common/bolt11.c:980-1062) and of checkmessage
 * (lightningd/signmessage.c:148-198) as one device call each over strings.  Decoding (bech32 / zbase32), the 5-bit to 8-bit repacking, the hashing,
 * the choice between recovery and verification under the invoice's `n` field and the curve work all run on the device, one lane per string; the
 * front-end kernel (k_bolt11_front / k_checkmessage_front), the key-parse kernel over the `n` keys, the verification batch (rows with `n`), the
 * recovery batch (rows without) and the merge are queued on one stream without the host waiting in between.
 *
 * lamd_bolt11_check_batch: string i = strs[off[i] .. off[i+1]) (off: n+1 entries), no terminator, exactly what bolt11_decode() would be handed: the
 * caller has stripped any "lightning:" prefix.  No length cap.  status[i] is the FIRST of these that applies, in the reference's order:
 *   -1 LAMD_B11_BAD_BECH32     bech32_decode() (common/bech32.c:94-155) refuses the string: shorter than 8; no separator (the LAST '1'), an empty
 *                              hrp, fewer than 6 data characters; an hrp byte outside 33..126; a data byte with bit 7 set or outside the alphabet
 *                              (both cases map); mixed case anywhere in the string; a final polymod other than 1 (bech32m is refused)
 *   -2 LAMD_B11_BAD_PREFIX     the lower-cased hrp does not start with "ln"
 *   -3 LAMD_B11_MALFORMED      framing or the `n` field.  D = the data values without the checksum: 7 of them are the 35-bit timestamp; while more
 *                              than 104 remain: 1 tag, a 2-value length, that many values -- a length greater than what remains (signature
 *                              included) is malformed; at the end exactly 104 must remain.  The first field with tag 19 (`n`) and length
 *                              exactly 53 is the payee key: malformed if its 265th bit is set or its 33 bytes are no valid compressed key
 *                              (pubkey_from_node_id).  A tag-19 field of another length, and every one behind the key, is skipped like any
 *                              other field (pull_expected_length / unknown_field)
 *   -4 LAMD_B11_BAD_RECID      byte 64 of the 65 signature bytes is above 3 (with an `n` field too)
 *   -5 LAMD_B11_SIG_RANGE      r or s >= n (secp256k1_ecdsa_recoverable_signature_parse_compact)
 *   -6 LAMD_B11_NO_KEY         no `n` field, and secp256k1_ecdsa_recover fails.  No low-S rule on this path
 *   -7 LAMD_B11_BAD_SIGNATURE  an `n` field, and secp256k1_ecdsa_verify under it fails: the low-S rule applies, the recovery id is ignored
 *    0 LAMD_B11_OK
 * node_id33 + 33*i = the recovered key or the `n` key; zero unless the status is OK.  hash32 + 32*i (may be NULL) = SHA-256(lower-cased hrp ||
 * the data values in front of the signature packed 5 -> 8 bits, the last byte padded with zero bits): the hash_u5 result; zero for statuses
 * -1 .. -3.  have_n[i] (may be NULL) = 1 iff an `n` key was found; zero for statuses -1 .. -3.
 * CONTRACT: fields other than `n` are walked and hashed, never interpreted -- chain name, amount, the required p / s / d|h fields, features,
 * utf-8 and route keys stay bolt11_decode_nosig()'s job (:748-975).  For a string bolt11_decode() accepts the status is OK and the key is its
 * receiver_id; for a string it rejects for one of the reasons above, with nothing unchecked failing earlier, the status is that reason. */
enum { LAMD_B11_OK = 0, LAMD_B11_BAD_BECH32 = -1, LAMD_B11_BAD_PREFIX = -2, LAMD_B11_MALFORMED = -3,
       LAMD_B11_BAD_RECID = -4, LAMD_B11_SIG_RANGE = -5, LAMD_B11_NO_KEY = -6, LAMD_B11_BAD_SIGNATURE = -7 };
int lamd_bolt11_check_batch(lamd_ctx *ctx, size_t n, const uint8_t *strs, const uint64_t *off,
			    int8_t *status, uint8_t *node_id33, uint8_t *hash32 /* may be NULL */, uint8_t *have_n /* may be NULL */);
/* lamd_checkmessage_batch: message i = msgs[moff[i] .. moff[i+1]) (any bytes, none included), its signature string zbase[zoff[i] .. zoff[i+1]).
 * status[i], the first that applies:
 *   -1 LAMD_MSG_BAD_ZBASE   a character outside "ybndrfg8ejkmcpqxot1uwisza345h769" (case-sensitive), or a character count that is no multiple
 *                           of 8: from_zbase32() returns NULL (:36-55)
 *   -2 LAMD_MSG_BAD_LENGTH  the string decodes to other than 65 bytes (:173)
 *   -3 LAMD_MSG_BAD_SIG     byte 0 - 31 is not in 0..3, or r or s >= n (:178-183).  The reference hands an out-of-range id to the library
 *                           unchecked (the library's argument check then calls its illegal-argument callback); here it is a bad signature
 *   -4 LAMD_MSG_NO_KEY      recovery fails over SHA256(SHA256("Lightning Signed Message:" || msg)) (:188-198)
 *    0 LAMD_MSG_OK          node_id33 + 33*i holds the key (zero otherwise): the caller compares it with the claimed key or looks it up in the graph
 * Both calls: n == 0 is LAMD_OK; a NULL input, status or node_id33 is LAMD_ERR_ARG; calls of more than the chunk size (lamd_set_chunk_rows) run their
 * curve work chunk by chunk; with lamd_set_timing(ctx, 1) lamd_info.last_text_ms holds the device time of the front end and of what follows it. */
enum { LAMD_MSG_OK = 0, LAMD_MSG_BAD_ZBASE = -1, LAMD_MSG_BAD_LENGTH = -2, LAMD_MSG_BAD_SIG = -3, LAMD_MSG_NO_KEY = -4 };
int lamd_checkmessage_batch(lamd_ctx *ctx, size_t n, const uint8_t *msgs, const uint64_t *moff,
			    const uint8_t *zbase, const uint64_t *zoff, int8_t *status, uint8_t *node_id33);
/* lamd_bolt12_check_text_batch: BOLT #12 offers, invoice requests and invoices FROM THEIR TEXT -- the stage in front of
 * lamd_bolt12_check_signature_batch, built like lamd_bolt11_check_batch: the front-end kernel (k_bolt12_text_front: the `+` joins, bech32 without
 * checksum, the TLV walk, the two ids, merkle_tlv() and sighash_from_merkle()), the key-parse kernel, the BIP-340 batch over all n rows and the
 * merge are queued on one stream without the host waiting in between.  String i = strs[off[i] .. off[i+1]) (off: n+1 entries), no terminator, no
 * length cap: exactly what offer_decode(), invrequest_decode() or invoice_decode() would be handed; a batch may mix the three kinds.
 * status[i] is the FIRST of these that applies, in the reference's order:
 *   -1 LAMD_B12_UNFINISHED     b12_string_to_data (common/bolt12.c:125-142): a '+' that is neither the first nor the last byte and does not directly
 *                              follow another joining '+' is dropped, and so are the bytes ccan's cisspace accepts (space, \t \n \v \f \r) behind
 *                              it; the string ends while still inside such a join
 *   -2 LAMD_B12_BAD_BECH32     from_bech32_charset + bech32_pull_bits (common/bech32_util.c:34-120) over the collapsed string: no '1' (the
 *                              separator is the FIRST '1'; an empty hrp passes here); a data byte >= 128 or outside the alphabet after case
 *                              folding; both an upper-case and a lower-case letter anywhere in hrp or data; 5*count mod 8 >= 5; a non-zero
 *                              padding bit.  The reference keeps the hrp as a C string: a NUL byte in it ends it, for the case test too
 *   -3 LAMD_B12_BAD_PREFIX     the lower-cased hrp is not "lno", "lnr" or "lni"
 *   -4 LAMD_B12_MALFORMED      the decoded bytes break fromwire_tlv's generic rules (wire/tlvstream.c:144-300: type and length minimal BigSize, the
 *                              length inside the stream, types strictly increasing); or, for an invoice request / an invoice, the kind's key field
 *                              (88 invreq_payer_id / 176 invoice_node_id) is present with a length other than 33 or its bytes are no valid
 *                              compressed key (fromwire_pubkey, bitcoin/pubkey.c:102-113), or field 240 is present with a length other than 64
 *   -5 LAMD_B12_OUT_OF_RANGE   any_field_outside_range (common/bolt12.c:211-213, :362-364).  Offer: any field outside 1..79 and
 *                              1000000000..1999999999.  Invoice request: any field other than types 240..1000 outside 0..159 and
 *                              1000000000..2999999999.  Invoices have no such rule
 *   -6 LAMD_B12_NO_KEY         an invoice request or invoice without its key field ("Missing invreq_payer_id" / "Missing node_id")
 *   -7 LAMD_B12_NO_SIGNATURE   an invoice request or invoice without field 240
 *   -8 LAMD_B12_BAD_SIGNATURE  bolt12_check_signature(fields, "invoice_request" | "invoice", "signature", key, sig) fails (common/bolt12.c:80-110,
 *                              plugins/offers_invreq_hook.c:1064-1077)
 *    0 LAMD_B12_OK             an offer that reached here carries no signature to check
 * kind[i] = LAMD_B12_KIND_*: set from the prefix test on, NONE for statuses -1 .. -3.  signer33 + 33*i = the key field's 33 bytes for OK rows of
 * kind invreq / invoice, zero otherwise.  sighash32 + 32*i (may be NULL) = sighash_from_merkle() for rows of kind invreq / invoice whose status is
 * OK or BAD_SIGNATURE, zero otherwise.  offer_id32 + 32*i (may be NULL) = calc_offer() for OK rows: SHA-256 over tlv_span(1, 79) ||
 * tlv_span(1000000000, 1999999999) of the decoded bytes; zero otherwise.  invreq_id32 + 32*i (may be NULL) = calc_invreq() for OK rows of kind
 * invreq / invoice: the spans are 0..159 and 1000000000..2999999999; zero otherwise.  tlv_span is the reference's (common/bolt12.c:670-695) with one
 * deviation: where it would subtract from a null pointer (the first field at or above the lower bound lies above the upper bound and no field
 * precedes it) the span is empty.  An id over two empty spans is SHA-256 of nothing (e3b0c442...).
 * CONTRACT: only the kind's key field and field 240 are interpreted.  The unknown-even-type rule (it needs each message's list of known types), the
 * inner encodings of all other known fields, features, chains, required fields, paths and expiry stay with the host's decoder.  For a string the
 * reference accepts the status is OK and the key is its signer; for a string it rejects for one of the reasons above, with nothing unchecked
 * failing earlier, the status is that reason.
 * n == 0 is LAMD_OK; a NULL strs, off, status, kind or signer33, and decreasing offsets, are LAMD_ERR_ARG; calls of more than the chunk size run
 * their curve work chunk by chunk; with lamd_set_timing(ctx, 1) lamd_info.last_text_ms covers this call's launches too. */
enum { LAMD_B12_OK = 0, LAMD_B12_UNFINISHED = -1, LAMD_B12_BAD_BECH32 = -2, LAMD_B12_BAD_PREFIX = -3, LAMD_B12_MALFORMED = -4,
       LAMD_B12_OUT_OF_RANGE = -5, LAMD_B12_NO_KEY = -6, LAMD_B12_NO_SIGNATURE = -7, LAMD_B12_BAD_SIGNATURE = -8 };
enum { LAMD_B12_KIND_NONE = 0, LAMD_B12_KIND_OFFER = 1, LAMD_B12_KIND_INVREQ = 2, LAMD_B12_KIND_INVOICE = 3 };
int lamd_bolt12_check_text_batch(lamd_ctx *ctx, size_t n, const uint8_t *strs, const uint64_t *off, int8_t *status, uint8_t *kind,
				 uint8_t *signer33, uint8_t *sighash32 /* may be NULL */, uint8_t *offer_id32 /* may be NULL */,
				 uint8_t *invreq_id32 /* may be NULL */);

/* grind_htlc_tx_fee() (onchaind/onchaind.c:388-438): find the feerate whose fee makes `sig64` (one remote HTLC signature,
 * one key) verify.  For feerate = min_feerate..max_feerate: fee = feerate * weight / 1000 (amount_tx_fee), equal consecutive
 * fees are tried once, fees above input_sat end the search; candidate = the transaction with output 0 paying
 * input_sat - fee.  The caller hands the BIP143 preimage of the transaction as it stands (any output-0 amount; the 32
 * bytes of hashOutputs sit 40 bytes before its end, bitcoin/signature.c:120-151) and the serialised outputs that
 * hashOutputs covers (amount of output 0 first).  All hashing and curve work runs on the device; (r/s)*Q is computed once
 * and each candidate costs two small double-SHA256 and the G-table additions.  Returns 1 = found (*feerate, *fee = the
 * lowest matching feerate and its fee, exactly the pair the reference's ascending loop stops at), 0 = none, < 0 error. */
int lamd_grind_htlc_tx_fee(lamd_ctx *ctx, const uint8_t *preimage, size_t preimage_len, const uint8_t *outputs,
			   size_t outputs_len, uint64_t input_sat, uint64_t weight, uint32_t min_feerate,
			   uint32_t max_feerate, const uint8_t sig64[64], uint8_t sighash_type, int has_witness_script,
			   const uint8_t pubkey33[33], uint32_t *feerate, uint64_t *fee);

/* ---- public-key parsing: n independent pubkey_from_der() / pubkey_from_node_id() calls
 * (bitcoin/pubkey.c:14-24, common/node_id.c:21-27 -> secp256k1_ec_pubkey_parse; publen 33 or 65),
 * or secp256k1_xonly_pubkey_parse with publen 32 (bitcoin/signature.c:422).  ok[i] = validity,
 * out64 + 64*i = affine X||Y big-endian (unspecified when invalid).  out64 may be NULL. */
int lamd_pubkey_parse_batch(lamd_ctx *ctx, size_t n, const uint8_t *pub, size_t publen, size_t pubstride,
			    uint8_t *out64, uint8_t *ok);

/* ---- gossip: gossipd/sigcheck.c on raw wire messages, batched.
 * msgs: the messages back to back; off[i]..off[i+1] delimits message i (off has n+1 entries).
 * kind is inferred from the 2-byte type (256 channel_announcement, 257 node_announcement,
 * 258 channel_update).  For channel_update the signer is not in the message (the reference looks
 * it up in the gossmap, gossipd/gossmap_manage.c:920-922): node_ids holds one 33-byte id per
 * message (ignored for the other kinds; may be NULL if the batch has no channel_update).
 * verdict[i]: 0 = OK (reference returns NULL); k > 0 = first bad signature, numbered as the
 * reference's messages name them -- channel_announcement: 1 "Bad node_signature_1",
 * 2 "Bad node_signature_2", 3 "Bad bitcoin_signature_1", 4 "Bad bitcoin_signature_2"
 * (gossipd/sigcheck.c:78-113); others: 1 "Bad signature for" (:35-41, :144-161);
 * -1 = malformed: what fromwire_* would have rejected before sigcheck runs (truncated message,
 * compact signature with r or s >= n, wire/fromwire.c:196-198; invalid bitcoin_key,
 * bitcoin/pubkey.c:102-113). */
int lamd_sigcheck_gossip_batch(lamd_ctx *ctx, size_t n, const uint8_t *msgs, const uint64_t *off,
			       const uint8_t *node_ids33, int8_t *verdict);

/* Device-resident variant (asynchronous on the context's stream).  d_off: uint64[n+1] byte offsets;
 * d_rowbase: uint64[n+1], d_rowbase[i] = number of signatures in messages 0..i-1 (4 per
 * channel_announcement, 1 otherwise), rows = d_rowbase[n]. */
int lamd_sigcheck_gossip_batch_device(lamd_ctx *ctx, size_t n, const void *d_msgs, const void *d_off,
				      const void *d_node_ids33, const void *d_rowbase, size_t rows,
				      void *d_verdict);
/* The spans form of the device-resident variant: message i = d_msgs[d_start[i], d_start[i] + d_len[i]) (uint64[n] each) -- any selection of a
 * resident message blob, in any order, as ONE call: what a rank of a replay cut per message kind verifies (its range of the channel_announcements
 * and its range of the channel_updates; lightning_amd/sharding.py segment_bounds).  d_node_ids33, d_rowbase, rows, d_verdict index the SELECTION. */
int lamd_sigcheck_gossip_spans_device(lamd_ctx *ctx, size_t n, const void *d_msgs, const void *d_start, const void *d_len,
				      const void *d_node_ids33, const void *d_rowbase, size_t rows, void *d_verdict);

/* ---- audit of a gossip_store FILE: every live record's checksum and every signature in it, before the daemon trusts the file.
 * The reference's start-up load (gossmap_load_initial -> map_catchup, common/gossmap.c:815-937) checks framing, flags and the CRC-32C of
 * each live record (csum_matches, :799-812) and never looks at a signature again (gossipd/gossmap_manage.c:508-539): a store copied from
 * another node, fetched as a snapshot, or damaged in a way that keeps the CRCs valid is loaded as it stands.  Here the checksums, the look-up
 * of every channel_update's signer in the store itself (the channel_announcement of its short_channel_id, node_id_1 / node_id_2 by the
 * direction bit: what gossmap_manage.c:920-922 asks the gossmap) and all signatures are one device call.
 *
 * The walk over the records is sequential, runs on the host and reads headers only (struct gossip_hdr, common/gossip_store.h:44-49, and
 * the 2-byte type).  It follows map_catchup: starts at offset 1 and stops -- lamd_store_summary.end_reason, end_offset -- when fewer than
 * 12 bytes are left, at a record without the COMPLETED flag, at one that reaches past the end of the file, at a live one shorter than 2
 * bytes, BEHIND a gossip_store_ended record (4105; the reference reopens the new file, here it is reported), and at a live
 * channel_announcement that is not followed by room for its channel_amount record (gossmap.c:488-492).  A file whose major version (top
 * three bits of byte 0) is not 0 is refused with LAMD_ERR_ARG.
 *
 * verdict[i] of record i, the first that applies:
 *    8  LAMD_STORE_SKIPPED_DELETED  DELETED flag set: nothing checked (gossmap.c:844-847)
 *   -2  LAMD_STORE_BAD_CHECKSUM     crc32c(timestamp, msg, len) != hdr.crc (:870-888, gossip_store.c:67)
 *   -4  LAMD_STORE_UNKNOWN_TYPE     not 256 / 257 / 258 / 4101 / 4103 / 4105 / 4106 / 4107 (:918-925; the obsolete 4102 / 4104 included)
 *   -1  LAMD_STORE_MALFORMED        what lamd_sigcheck_gossip_batch calls -1
 *   -5  LAMD_STORE_REDUNDANT        a live channel_announcement of this scid exists at a lower offset (gossmap.c:475-486)
 *   -3  LAMD_STORE_NO_CHANNEL       channel_update without a live channel_announcement of its scid at a lower offset (update_channel
 *                                   false, :898-899), or whose announcement is cut off before the node id
 *  1..4                             the first bad signature, numbered as lamd_sigcheck_gossip_batch numbers them
 *    0  LAMD_STORE_OK               checksum good; for the three gossip kinds every signature good
 * Verdicts of different records are independent except for the signer look-up: an update is judged against the node ids of its
 * announcement whatever that announcement's own verdict.  Live or dead is decided by the FLAGS ALONE: gossipd itself marks what a
 * delete_chan tombstone (4103) removes as DELETED (gossip_store.c:622-638), so tombstones are checksummed and counted, never applied.
 * THIS DIFFERS FROM THE REFERENCE'S LOADERS, which do apply one: common/gossmap.c removes the tombstone's channel
 * (:900-901, remove_channel_by_deletemsg :612-626) and so does pyln's Gossmap.  On a store gossipd wrote the result is the same, because
 * remove_channel writes the tombstone AND flags the announcement, its amount record and its updates DELETED (gossmap_manage.c:318-328).
 * On a store where a valid tombstone stands behind records that are not flagged, it is not: gossmap.c drops the channel (and a node that
 * has no other), this library keeps both in digest, bare list and directory.  The one natural case is among the reference's own
 * fixtures: the last record of contrib/pyln-client/tests/data/gossip_store-part2.xz (2021) is a tombstone for 686386x1093x1 whose
 * announcement is not flagged.  As shipped it also fails its CRC: pyln checks none and drops the channel; gossmap.c checks
 * (csum_matches, :870-888) and stops loading in front of it, so the channel survives there; here the record is LAMD_STORE_BAD_CHECKSUM and
 * the channel stays.  With the CRC corrected gossmap.c would drop the channel and this library still keeps it: tests/test_reference_stores.py
 * pins that difference, the repairs included: they drop the tombstone's own record and keep the channel it names.
 * Records 4101 / 4106 / 4107 get the checksum only; following store_ended into the new file, dying deadlines, the upgrade of old versions
 * and the legacy 0x4000 push bit of version 15 (ignored) are left to the reference's own load. */
enum {
	LAMD_STORE_OK = 0,
	LAMD_STORE_MALFORMED = -1,
	LAMD_STORE_BAD_CHECKSUM = -2,
	LAMD_STORE_NO_CHANNEL = -3,
	LAMD_STORE_UNKNOWN_TYPE = -4,
	LAMD_STORE_REDUNDANT = -5,
	LAMD_STORE_SKIPPED_DELETED = 8
};
enum {
	LAMD_STORE_END_EOF = 0,            /* the walk consumed the file to its last byte */
	LAMD_STORE_END_PARTIAL_HEADER = 1, /* 1..11 bytes left */
	LAMD_STORE_END_INCOMPLETE = 2,     /* a record without the COMPLETED flag */
	LAMD_STORE_END_TRUNCATED = 3,      /* a record reaches past the end of the file */
	LAMD_STORE_END_SHORT = 4,          /* a live record of fewer than 2 bytes */
	LAMD_STORE_END_STORE_ENDED = 5,    /* a gossip_store_ended record: counted, the walk stops behind it */
	LAMD_STORE_END_NO_AMOUNT = 6       /* a live channel_announcement without room for its channel_amount record: not counted */
};
typedef struct {
	int version;              /* byte 0 of the file */
	int end_reason;           /* LAMD_STORE_END_* */
	int clean;                /* 1 iff end_reason is LAMD_STORE_END_EOF and every verdict is OK or SKIPPED_DELETED (always 0 from lamd_gossip_store_frame) */
	uint64_t records, live, deleted;
	uint64_t end_offset;      /* where the walk stopped */
	/* one counter per verdict code, summed from the verdict array (all 0 from lamd_gossip_store_frame) */
	uint64_t ok, skipped_deleted, bad_checksum, unknown_type, malformed, redundant, no_channel;
	uint64_t bad_signature[4]; /* verdicts 1..4 */
	uint64_t signatures;      /* signature rows verified: 4 per live channel_announcement, 1 per live node_announcement / channel_update */
	double stage_ms[5];       /* with lamd_set_timing(ctx, 1): device time of checksums, index, signers, signatures, verdicts (HIP events); else 0 */
} lamd_store_summary;
/* host only, no context: the walk.  rec_off[i] = offset of record i's gossip_hdr (cap entries; may be NULL with cap == 0).  cap too small:
 * LAMD_ERR_ARG with *n_records = the count needed and the summary filled. */
int lamd_gossip_store_frame(const uint8_t *store, size_t len, size_t cap, uint64_t *rec_off, size_t *n_records, lamd_store_summary *summary);
/* the audit.  d_store == NULL: `store` is copied to the device; otherwise the image is already resident at d_store (len bytes) and `store`
 * (host) is read for the 12 bytes of header + 2 of type per record only.  rec_off / verdict: cap entries each (call lamd_gossip_store_frame
 * first to size them; cap too small: LAMD_ERR_ARG with *n_records = the count needed).  The device work is queued without any host
 * synchronisation between its stages -- CRC-32C of every live record (k_store_crc), scid index of the live announcements (k_store_index),
 * signers and redundancy (k_store_signers), ONE signature batch over the live 256 / 257 / 258 records (the spans form of
 * lamd_sigcheck_gossip_spans_device), the merge (k_store_verdict) -- and ends with one copy of the verdict bytes; the call returns when
 * they have arrived.  A store holding only its version byte is LAMD_OK with clean = 1. */
int lamd_gossip_store_audit(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t cap, uint64_t *rec_off,
			    int8_t *verdict, size_t *n_records, lamd_store_summary *summary);

/* ---- repair of a gossip_store FILE: the audit, and behind it, on the device, the store that holds what passed.
 * The reference's load stops at the first bad checksum (common/gossmap.c:870-888) and never checks a signature; its only rewriting tool,
 * gossipd/compactd.c, copies every record that is not flagged deleted (and is not a uuid or delete_chan record), whatever it holds.  Here
 * the rewritten store holds the records whose verdict is OK and whose dependencies are kept, in file order, behind a fresh uuid record.
 *
 * Record i is KEPT iff it is live (DELETED flag clear), verdict[i] == LAMD_STORE_OK, and, by its type ("indexed" = the lowest-index live
 * channel_announcement of that short_channel_id, as the audit's scid index returns it):
 *    256 channel_announcement  record i+1 exists, is live, is of type 4101 and length 10 and has verdict OK: gossmap reads the amount
 *                              from the record that follows without checking what it is (gossmap.c:488-492)
 *   4101 channel_amount        record i-1 is a kept 256
 *    258 channel_update        the indexed announcement of its scid has a lower record index and is kept
 *   4106 chan_dying            its length is 14, and the indexed announcement of its scid has a lower record index and is kept
 *    257 node_announcement     its node_id equals node_id_1 or node_id_2 of a kept channel_announcement with a lower record index
 *   4103 delete_chan, 4107 uuid, 4105 store_ended   never kept (compactd's first phase drops the first two; the walk stops behind the third)
 *   anything else              never kept
 * reason[i], why record i is not in the output:
 *   0  kept
 *   1  DELETED flag set
 *   2  the record itself: verdict[i] is neither OK nor NO_CHANNEL (or a chan_dying record is not 14 bytes long)
 *   3  a dependency: its announcement is dropped or missing (verdict NO_CHANNEL included), its amount record is missing or not OK, its
 *      node is in no kept announcement with a lower index
 *   4  store bookkeeping: 4103 / 4105 / 4107
 * for a live record the first of 2, 4, 3 that applies.
 *
 * The output: the input's version byte; one uuid record built from uuid32 (flags COMPLETED, timestamp 0, type 4107, crc32c seeded with 0:
 * 46 bytes); the kept records, headers verbatim (the DYING flag bit with them), in file order.  It is never longer than len + 46 bytes.
 * new_off[i] = offset of record i's gossip_hdr in the output, UINT64_MAX for a dropped record: the map gossmap_manage needs when it
 * swaps files. */
typedef struct {
	uint64_t kept;
	/* one counter per reason 1..4 */
	uint64_t dropped_deleted, dropped_verdict, dropped_dependency, dropped_bookkeeping;
	uint64_t out_len;         /* length of the rewritten store */
	double stage_ms[3];       /* with lamd_set_timing(ctx, 1): device time of keep flags, scan, copy (HIP events); else 0 */
} lamd_store_repair_summary;
/* store / len / d_store / cap / rec_off / verdict / n_records / summary: as lamd_gossip_store_audit, unchanged in meaning.  new_off / reason:
 * cap entries each.  The output goes to `out` (host) and / or stays on the device at d_out; out_cap is the size of each one given, both
 * may be NULL (the maps and the counters only).  A device buffer of len + 46 bytes always suffices.  Too few entries: LAMD_ERR_ARG with
 * *n_records = the count needed.  out_cap too small: LAMD_ERR_ARG with repair->out_len = the size needed and everything else filled in;
 * what d_out then holds is unspecified (nothing is written behind out_cap).
 * The device work is queued behind the audit's on the same stream: keep flags (k_store_keep_chan: announcements, and their node ids into
 * a table; k_store_keep_rest: everything else), the exclusive scan of the kept sizes (reduce, scan of the sums, apply: separate launches),
 * the copy (k_store_pack: one aligned 32-bit word of the output per lane).  The host waits twice: for verdicts, reasons, offsets and the
 * output's length, then -- with `out` -- for that many bytes of image.  A store holding only its version byte gives version + uuid record. */
int lamd_gossip_store_repair(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, const uint8_t *uuid32, size_t cap,
			     uint64_t *rec_off, int8_t *verdict, uint64_t *new_off, uint8_t *reason, size_t *n_records, uint8_t *out,
			     void *d_out, size_t out_cap, lamd_store_summary *summary, lamd_store_repair_summary *repair);

/* ---- latest-wins repair of a gossip_store FILE: the repair above, and of the records that pass it only the one gossipd would hold now.
 * The audit and the repair above answer "is every record intact, validly signed, and are its dependencies there?" and read no timestamp.
 * Nor does the reference's load: update_channel() and node_announcement() (common/gossmap.c:585-610, :650-668) take whichever live record
 * comes LAST in file order.  Timestamps are compared on the receive path alone -- `prev_timestamp >= timestamp` means ignore
 * (gossipd/gossmap_manage.c:934-945, :1134-1143), timestamp_reasonable() (:997-1008) -- and gossipd flags what it supersedes DELETED
 * (:964-966), so a store it wrote itself never shows the difference.  A copied, concatenated or edited store does: a validly signed old
 * channel_update placed behind the current one is what gossmap then routes on; a header timestamp (the one gossipd's filters read,
 * gossip_store_get_timestamp) may differ from the signed one under a recomputed CRC; a channel silent for more than two weeks stays until
 * prune_network() (:409-471) first runs.
 *
 * Signed timestamp ts(i): channel_update -- the be32 at message offset 106; node_announcement -- the be32 at 68 + flen.
 * ELIGIBLE: a live 257 / 258 with verdict OK whose header timestamp equals ts(i), and, with a clock (policy->now != 0), with
 *           ts(i) <= now + future_slack (64-bit).
 * WINNER of a set of records: the highest ts; among equal ts the LOWEST record index -- what `prev_timestamp >= timestamp: ignore` leaves
 *           of records that arrive in file order.
 * "Indexed announcement" as in the audit: the lowest-index live 256 of that scid, whatever its verdict.  In this order:
 *   1  provisional announcements: as the repair decides (verdict OK, the amount record behind it OK)
 *   2  per provisionally kept announcement a:  latest[a][d] = the winner among the eligible updates i > a whose indexed announcement is
 *      a and whose channel_flags & 1 is d;  dying[a] = a live, OK, 14-byte 4106 record i > a names its scid
 *   3  final announcements: a is STALE iff now != 0 and prune_interval != 0 and !dying[a] and, for some d, latest[a][d] exists with
 *      ts + prune_interval < now (64-bit).  A direction without any update counts as fresh (get_timestamp() gives UINT32_MAX,
 *      :383-396); ts == now - prune_interval keeps the channel (:440).  The node table holds the node ids of the FINALLY kept
 *      announcements, lowest record index per node
 *   4  nlatest[node] = the winner among the eligible 257 records i whose node_id is in that table with a table index < i
 *   5  every other record, below
 * reason[i], the first that applies:
 *   1  DELETED flag set
 *   2 / 4 / 3  exactly as the repair decides among them (a record with verdict NO_CHANNEL is 3), but against the FINAL announcements and
 *      their node table: the amount record, the updates and the dying records of a stale channel, and the node_announcement of a node whose
 *      channels are all stale, are 3
 *   7  STALE: an announcement the repair would keep, by step 3 (every other announcement keeps the repair's reason)
 *   6  TIMESTAMP: a 257 / 258 with verdict OK that is not eligible -- reported whether or not its dependencies are kept, in place of 3
 *   5  SUPERSEDED: an eligible 257 / 258 with kept dependencies that is not the winner of its slot
 *   0  kept
 * So: a record whose verdict is not OK never supersedes anything; an update in front of its announcement never supersedes one behind it;
 * with now == 0 neither the clock half of ELIGIBLE nor STALE applies; the output audits clean, the plain repair of it drops its uuid record
 * alone, and this call on it with the same policy and uuid returns it unchanged. */
typedef struct {
	uint64_t now;            /* UNIX seconds; 0 = no clock: the FUTURE and the STALE rule are off */
	uint32_t future_slack;   /* seconds a signed timestamp may lie ahead of now (the reference: 86 400) */
	uint32_t prune_interval; /* seconds; 0 = the STALE rule is off (the reference: 1 209 600, common/gossip_constants.h:85) */
} lamd_store_latest_policy;
typedef struct {
	uint64_t kept;
	uint64_t dropped_deleted, dropped_verdict, dropped_dependency, dropped_bookkeeping,   /* reasons 1..4, as the repair */
		 dropped_superseded, dropped_timestamp, dropped_stale;                         /* reasons 5..7 */
	uint64_t out_len;
	double stage_ms[3];      /* keep stages (all the new launches), scan, copy */
} lamd_store_latest_summary;
/* Every argument shared with lamd_gossip_store_repair keeps that call's meaning, return codes and sizes; the output has its format (version
 * byte, uuid record, the kept records verbatim in file order) and is never longer than len + 46 bytes.  policy == NULL: LAMD_ERR_ARG.
 * The device work is queued behind the audit's on the same stream, one lane per record, each stage a launch of its own because it reads
 * what the one before wrote with atomics: k_store_latest_upd (eligibility, the update slots -- one 64-bit key ts << 32 | ~index per
 * (announcement, direction), written with atomicMax -- and the dying marks), k_store_latest_chan (final announcements, node table),
 * k_store_latest_node (the node slots), k_store_latest_rest (every other record); then the repair's scan, copy and two host waits.
 * stage_ms (with lamd_set_timing): the four launches and the clearing of their tables; scan; copy. */
int lamd_gossip_store_repair_latest(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, const uint8_t *uuid32,
				    const lamd_store_latest_policy *policy, size_t cap, uint64_t *rec_off, int8_t *verdict, uint64_t *new_off,
				    uint8_t *reason, size_t *n_records, uint8_t *out, void *d_out, size_t out_cap,
				    lamd_store_summary *summary, lamd_store_latest_summary *latest);

/* ---- serving a trusted store: the channel digest of a gossip_store image on the device, and the replies to query_channel_range from it.
 * What connectd/queries.c does per query -- gather_range() (:564-634) walks every channel, re-reads both channel_updates of each channel in
 * range and checksums them, queue_channel_ranges() (:641-711) cuts the result into reply_channel_range messages -- split in two: the digest
 * is built once per store, a batch of queries is answered from it.
 *
 * THE DIGEST.  store / len / d_store: the image, as in the audit, but either may be NULL (host `store` is copied, a resident d_store is read
 * in place: e.g. the d_out a repair has left).  rec_off[n]: the records, from lamd_gossip_store_frame or, for a repair's output, the kept
 * new_off in order.  verdict[n]: optional, the audit's.  The device reads headers and types itself; every read stays inside the image
 * whatever rec_off holds.  The rules are gossmap's load (common/gossmap.c:451-509, :585-610); as in the audit, flags alone decide whether
 * a record is live and tombstones are not applied.
 *   COUNTS   record i counts iff its DELETED flag is clear and, with verdict, verdict[i] == LAMD_STORE_OK
 *   CHANNEL  the lowest-index counting 256 of its scid; later 256 records of that scid are ignored
 *   SLOT [a][d]  the HIGHEST-index counting 258 of >= 112 bytes whose scid (message offset 98) is that of channel a, with a < i, and
 *            whose channel_flags & 1 (offset 111) is d: last in file order wins whatever the timestamps (update_channel(), not the
 *            receive path).  A 258 shorter than 112 bytes is ignored -- deliberately: the reference would read past its end.
 *   ENTRY    one per channel with at least one slot set (the policy of queries.c:603-607): scid; ts[d] = the be32 at message offset 106 of
 *            the slot's record, or 0; csum[d] = crc32c(crc32c(0, m + 66, 40), m + 110, len - 110), or 0 (crc32_of_update, :429-470);
 *            rec[3] = the record indices of the announcement and of the two updates, UINT32_MAX where there is none
 * The entries are SORTED ASCENDING BY SCID.  That is the one deliberate difference from the reference, which since it dropped its uintmap
 * emits channels in gossmap index order (:593-596) although BOLT #7 requires ascending short_channel_ids and its own split at block
 * boundaries assumes them: tests/golden/gossip_store_mesh_3x3.bin, written by the reference, holds its channels out of order.
 *   BARE     the scids of the channels WITHOUT any slot set, ascending: gossmap_find_chan finds these too, so the comparison of peers'
 *            replies (below) must know them; the replies never list them.  Their number is channels_no_update.
 * Launches, one stream, no host wait between them: k_digest_index (scid index), k_digest_slots (a 32-bit atomicMax of index + 1 per
 * slot), k_digest_chan (channels, compaction of (scid, announcement) pairs and of the bare scids), rocPRIM's radix sorts of the pairs
 * and of the bare scids (both inside the stage "sort"), k_digest_entries (timestamps and checksums, written in sorted order).  The call
 * waits once, at its end, for the counters below.
 * The digest lives on the device until lamd_store_digest_free (before lamd_shutdown of its context); it does not refer to the image. */
typedef struct lamd_store_digest lamd_store_digest;
typedef struct {
	uint64_t records;             /* n */
	uint64_t channels;            /* channels seen */
	uint64_t entries;             /* ... of them with at least one update: the digest's count */
	uint64_t channels_no_update;  /* ... and without any: the bare list's count */
	uint64_t updates_no_channel, updates_in_front, updates_short;   /* counting 258 records ignored, by reason */
	double stage_ms[5];           /* with lamd_set_timing: index, slots, channels, sort, entries */
} lamd_store_digest_summary;
int lamd_gossip_store_digest_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
				   const int8_t *verdict, lamd_store_digest **digest, lamd_store_digest_summary *summary);
void lamd_store_digest_free(lamd_store_digest *digest);
size_t lamd_store_digest_count(const lamd_store_digest *digest);
/* copies the digest back: scid[cap], ts[2 * cap], csum[2 * cap], rec[3 * cap] (any may be NULL); cap < count: LAMD_ERR_ARG */
int lamd_store_digest_read(const lamd_store_digest *digest, size_t cap, uint64_t *scid, uint32_t *ts, uint32_t *csum, uint32_t *rec);
/* the channels without an update: their number, and their scids copied back, ascending; cap < count: LAMD_ERR_ARG */
size_t lamd_store_digest_bare_count(const lamd_store_digest *digest);
int lamd_store_digest_read_bare(const lamd_store_digest *digest, size_t cap, uint64_t *scid);

/* THE REPLIES.  Query q is the raw wire message queries + qoff[q] .. qoff[q + 1]: be16 263 | chain_hash 32 | be32 first_blocknum | be32
 * number_of_blocks | TLV stream; TLV 1 = query_option, a bigsize, bit 0 asks for timestamps, bit 1 for checksums, other bits are ignored.
 * The queries are parsed on the host by fromwire_tlv's rules (ascending types, minimal bigsize, an unknown even type fails, an unknown odd
 * one is skipped).  status[q]:
 *    0  answered
 *   -1  malformed: no reply (the reference sends "Bad query_channel_range w/tlvs ..."; the caller owns that text)
 *    1  foreign chain_hash: exactly one reply that echoes the query's chain_hash, first_blocknum and number_of_blocks as received, with
 *       sync_complete 0, len 0 and no TLVs (:735-744)
 * The replies of query q are the messages reply_first[q] .. reply_first[q + 1] - 1; message j is the bytes out + msg_off[j] .. msg_off[j + 1].
 * msg_cap or out_cap too small: LAMD_ERR_ARG with summary->messages / summary->bytes = what is needed, status and reply_first filled in
 * and nothing written to msg_off, out or d_out.  out and d_out both NULL: the sizes alone.
 * SELECTION  if first + number overflows, number = UINT32_MAX - first (:746-748); end = first + number - 1; the entries whose scid >> 40
 *            lies in [first, end], none when number == 0: two binary searches in the digest.
 * LIMIT      max_entries() (:519-561): bytes = 65535 - 2 - 43, per_entry = 8; each option asked for subtracts 1 + bigsize_len(8186 * 8) = 4
 *            and adds 8 to per_entry; bytes is capped by max_encoded_bytes when that is not 0 (dev_max_encoding_bytes) and raised to
 *            per_entry when it falls below; limit = bytes / per_entry: 8186, 4092, 4092, 2728 without a cap.
 * SPLIT      queue_channel_ranges() with its one out-of-bounds corner made definite.  s = the selected scids, off = 0; loop:
 *              rem = count - off; if rem <= limit: n = rem, blocks = number; else n = limit; while n > 0 and block(s[off + n - 1]) ==
 *              block(s[off + limit]): n--; if n == 0: n = limit (one block holds more than a message: the boundary is broken, as the
 *              reference chooses to, but its loop reads s[off - 1]); blocks = block(s[off + n]) - first.
 *              emit (first, blocks, entries off .. off + n, sync_complete = (blocks == number)); first += blocks, number -= blocks,
 *              off += n; while number != 0.
 *            A query with number == 0 or one that selects nothing gives one reply without entries, sync_complete 1.  The device loop is
 *            bounded by count + 1 iterations.
 * MESSAGE    (:372-426, wire/peer_wire.csv:400-412) be16 264 | chain_hash | be32 first | be32 blocks | u8 sync_complete | be16 1 + 8n | 0x00
 *            (uncompressed) | n be64 scids | with bit 0: 0x01, bigsize 1 + 8n, 0x00, n x (be32 ts[0], be32 ts[1]) | with bit 1: 0x03,
 *            bigsize 8n, n x (be32 csum[0], be32 csum[1]).  With n = 0 both TLVs are still there when asked for, type 1 with length 1 and
 *            type 3 with length 0: send_reply_channel_range() hands over a non-NULL, zero-length checksums_tlv (tal_dup_arr of 0
 *            elements, :410-413), the generated towire of a TLV record (tools/gen/impl_template:220-245) returns NULL only for a NULL
 *            field and an empty array otherwise, and towire_tlv() (wire/tlvstream.c:350-362) writes type and length of whatever is not NULL.
 * Device work: k_range_count (one lane per query: searches and split, counting), k_range_scan (messages and bytes per query to
 * offsets), k_range_plan (the split again, writing (first, blocks, off, n, final, flags) and the offset of every message), then
 * k_range_encode, one aligned 32-bit word of the output per lane, bytes swapped in registers.  The host waits once for sizes and
 * offsets and once for the bytes. */
typedef struct {
	uint64_t answered, malformed, foreign;   /* queries by status */
	uint64_t messages, bytes;                /* replies and their total size: what msg_cap and out_cap must hold */
	double stage_ms[2];                      /* with lamd_set_timing: plan (count, scan, plan), encode */
} lamd_range_reply_summary;
int lamd_channel_range_reply_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, size_t nq, const uint8_t *queries,
				   const uint64_t *qoff, uint32_t max_encoded_bytes, int8_t *status, uint64_t *reply_first, size_t msg_cap,
				   uint64_t *msg_off, uint8_t *out, void *d_out, size_t out_cap, lamd_range_reply_summary *summary);

/* THE COMPARISON: what the seeker does with a peer's reply_channel_range messages -- handle_reply_channel_range() (gossipd/queries.c:183-359)
 * feeding process_scid_probe() (gossipd/seeker.c:708-735) -- for a batch of raw messages from any number of peers, against the digest.
 * Message i is the bytes msgs + moff[i] .. moff[i + 1] (the call reads msgs[0, moff[n])): be16 264 | chain_hash 32 | be32 first_blocknum |
 * be32 number_of_blocks | u8 sync_complete | be16 len | encoded_short_ids | TLV stream (1: encoding_type + encoded_timestamps, 3: checksums).
 * STATUS, parsed on the host, the checks in the reference's order, the first failure decides:
 *   -1  not a reply_channel_range: shorter than 45 bytes, type not 264, len past the end, a TLV stream that breaks fromwire_tlv's rules
 *       (ascending types, minimal bigsize, unknown even type), TLV 1 of length 0, TLV 3 of a length that is no multiple of 8 (:197-203)
 *    1  chain_hash is not chain_hash32 (:205-209)
 *    2  first_blocknum + number_of_blocks overflows 32 bits (:218-222)
 *    3  encoded_short_ids does not decode: len 0, first byte not 0 (zlib is gone, common/decode_array.c:26-42), (len - 1) % 8 != 0 (:224-229)
 *    4  only with want_first[n] / want_end[n], the peer's outstanding query (range_first_blocknum, exclusive range_end_blocknum):
 *       first + number <= want_first or first >= want_end (:257-265)
 *    5  TLV 1: encoding_type not 0, or (length - 1) % 8 != 0 (:153-157, decode_array.c:84-113)
 *    6  the number of timestamp pairs is not the number of scids (:158-163)
 *    0  accepted; len == 1 is accepted with no entries.  TLV 3 is validated as above and otherwise ignored.
 *   "reply without query" (:211-215) and the sync_complete / block tally (:290-358) are per-peer protocol state: the caller's.
 * CLASS of every entry of every accepted message (scid; t1, t2 = its timestamps, (0, 0) without TLV 1 -- zero_ts, :150):
 *   scid is digest entry j:          flags = (t1 > ts[j][0] ? 2 : 0) | (t2 > ts[j][1] ? 4 : 0)   (SCID_QF_UPDATE1 / 2; an unset slot is 0 in
 *                                    the digest, so this is want_update()'s `timestamp != 0` there, seeker.c:642-650)
 *   else scid is in the bare list:   the same with both of our timestamps 0
 *   else:                            unknown
 *   flags == 0: nothing to do.  per_msg[3 * n]: entries, unknown entries, stale entries (flags != 0) of each message, BEFORE merging
 *   (what peer_supplied_query_response and set_preferred_peer need); a rejected message has 0, 0, 0.
 * MERGE  unknown_scid: the unknown scids ascending, each once (uintmap_add refuses duplicates, :700).  stale_scid / stale_flags: the
 *   stale scids ascending, each once, with the OR of the flags of all its entries (*stale |= query_flag, :688).  Neither depends on the
 *   order of the messages.  DELIBERATE DIFFERENCE: the reference stops adding unknown scids once it holds more than 10 000 (:696), in
 *   arrival order; this call returns all of them and reports the counts -- a bounded map is the caller's policy, and arrival order means
 *   nothing in a batch.
 * QUERIES  the query_short_channel_ids messages (queries.c:46-139, wire/peer_wire.csv:382-389) for the unknown list first, max_unknown
 *   scids each except the last (0: 8000, seeker.c:297), then for the stale list, max_stale each (0: 7000, :382); a value above its
 *   default is LAMD_ERR_ARG; an empty list gives no message.  unknown: be16 261 | chain_hash32 | be16 1 + 8k | 0x00 | k be64 scids
 *   (37 + 8k bytes); stale: the same, then 0x01 | bigsize 1 + k | 0x00 | k flag bytes.  Message j is out + msg_off[j] .. msg_off[j + 1],
 *   the first summary->unknown_messages of them are those of the unknown list.  The bytes go to out (host), d_out (device, any
 *   alignment), or neither.
 * SIZES  scid_cap must hold each list, msg_cap the messages, out_cap the bytes (when out or d_out is given).  One too small:
 *   LAMD_ERR_ARG with summary, status and per_msg filled in and nothing written to the lists, msg_off, out or d_out.  All caps 0: the
 *   sizes alone (LAMD_OK when there is nothing to hold).
 * Device work, on the context's stream: k_cmp_classify (one lane per entry: its message by bisection in the prefix sums, two binary
 * searches, compaction with one atomic per wave), k_cmp_per_msg (one wave per message, no atomics), rocPRIM's radix sorts, then per list
 * k_cmp_heads, an inclusive scan and k_cmp_merge; k_cmp_plan (message offsets); k_cmp_encode, one aligned 32-bit word of the output per
 * lane.  The host waits once for counts and sizes and once for the lists and the bytes.  Limits: n and the sum of the entries below
 * UINT32_MAX, moff non-decreasing, the digest built by this context. */
typedef struct {
	uint64_t by_status[8];   /* messages: [0] accepted, [1..6] statuses 1..6, [7] malformed */
	uint64_t entries, entries_unknown, entries_stale;   /* before merging */
	uint64_t unknown, stale; /* after merging: what scid_cap must hold (each list) */
	uint64_t unknown_messages, messages, bytes;   /* what msg_cap and out_cap must hold */
	double stage_ms[4];      /* with lamd_set_timing: classify, merge, plan, encode */
} lamd_range_compare_summary;
int lamd_channel_range_compare_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, size_t n, const uint8_t *msgs,
				     const uint64_t *moff, const uint32_t *want_first, const uint32_t *want_end, uint32_t max_unknown,
				     uint32_t max_stale, int8_t *status, uint32_t *per_msg, size_t scid_cap, uint64_t *unknown_scid,
				     uint64_t *stale_scid, uint8_t *stale_flags, size_t msg_cap, uint64_t *msg_off, uint8_t *out, void *d_out,
				     size_t out_cap, lamd_range_compare_summary *summary);

/* ---- answering query_short_channel_ids from a store image: what handle_query_short_channel_ids() (connectd/queries.c:260-368) and
 * maybe_create_query_responses() (:112-255) send for a peer's query, for a batch of raw queries, as copies of the stored messages.
 *
 * THE DIRECTORY is built from the same (image, rec_off, verdict) as a digest plus that digest; n differing from the digest's records is
 * LAMD_ERR_ARG.  Unlike the digest it REFERS TO THE IMAGE: a host `store` is copied to the device and owned by the directory, a resident
 * d_store is read in place and the caller keeps it alive until lamd_store_directory_free; rec_off is uploaded and kept; what it needs of
 * the digest is copied, the digest may be freed.  Every device read stays inside the image whatever rec_off holds.  "Counts" is the
 * digest's word: DELETED flag clear and, with verdict, verdict[i] == LAMD_STORE_OK.
 *   CHANNEL -> RECORDS  digest entry j: its rec[3] as is.  Bare channel j: the lowest-index counting 256 of that scid (one lane per
 *            record bisects the bare list, a 32-bit atomicMin).  The channels are numbered entries first, then the bare ones.
 *   NODES    the distinct 33-byte node ids named by the announcements of all channels: with feature length f (the be16 at message
 *            offset 258) node_id_1 sits at offset 300 + f and node_id_2 at 333 + f; an announcement shorter than 366 + f names no
 *            nodes.  first = the lowest announcement record index naming the node.
 *   RANK     the nodes ascending by memcmp of the 33 bytes; a node's rank is its position.  Node ids are attacker-chosen, so no
 *            shortened key decides: a stable LSD sort over the 2 x channels candidates, five rocPRIM radix_sort_pairs passes over 8-byte
 *            chunks gathered from the image (the first one the 33rd byte alone) and a one-bit pass that moves the candidates without an
 *            id behind the others; then heads of runs, an inclusive scan, and the merge.  Each channel keeps the ranks of its two
 *            nodes, or UINT32_MAX.
 *   NODE ANNOUNCEMENT of a node: the HIGHEST-index counting 257 of >= 105 + f bytes (f: the be16 at offset 66, the id sits at 72 + f)
 *            whose id is that node and whose index is greater than the node's first: the last one in the file wins whatever the
 *            timestamps, and one in front of the node's first channel does not count (common/gossmap.c:650-668).  A 32-bit atomicMax of
 *            index + 1; the 257 records find their node by bisection in the ranked ids.
 * The call runs on the context's stream and waits once, at its end, for the counters. */
typedef struct lamd_store_directory lamd_store_directory;
typedef struct {
	uint64_t nodes;             /* distinct node ids */
	uint64_t nodes_announced;   /* ... of them with a node_announcement */
	uint64_t nann_no_node, nann_in_front, nann_short;   /* counting 257 records ignored, by reason */
	double stage_ms[5];         /* with lamd_set_timing: bare records, candidates, sort, rank, node announcements */
} lamd_store_directory_summary;
int lamd_gossip_store_directory_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
				      const int8_t *verdict, const lamd_store_digest *digest, lamd_store_directory **directory,
				      lamd_store_directory_summary *summary);
void lamd_store_directory_free(lamd_store_directory *directory);
size_t lamd_store_directory_node_count(const lamd_store_directory *directory);
/* the nodes in rank order: id33[33 * cap], first[cap], nann_rec[cap] (UINT32_MAX: not announced); any may be NULL; cap < count: LAMD_ERR_ARG */
int lamd_store_directory_read_nodes(const lamd_store_directory *directory, size_t cap, uint8_t *id33, uint32_t *first, uint32_t *nann_rec);
/* the channels: bare_rec[cap_bare] (the announcement's record of each bare channel, in the bare list's order), entry_rank[2 * cap_entries],
 * bare_rank[2 * cap_bare] (the ranks of node_id_1 and node_id_2, UINT32_MAX: none); any may be NULL; a cap below its count: LAMD_ERR_ARG */
int lamd_store_directory_read_channels(const lamd_store_directory *directory, size_t cap_entries, size_t cap_bare, uint32_t *bare_rec,
				       uint32_t *entry_rank, uint32_t *bare_rank);

/* THE REPLIES.  Framing as lamd_channel_range_reply_batch: query q is queries + qoff[q] .. qoff[q + 1] (the call reads
 * queries[qoff[0], qoff[nq])), its replies are the messages reply_first[q] .. reply_first[q + 1] - 1, message j is out + msg_off[j] ..
 * msg_off[j + 1]; msg_rec[j] (optional) is the record index the message was copied from, UINT32_MAX for an end message.
 * STATUS, parsed on the host (the bigsize flags are sequential), the first failure decides:
 *   -1  not a query_short_channel_ids: shorter than 36 bytes, type not 261, len past the end, a TLV stream that breaks fromwire_tlv's rules
 *       (ascending types, minimal bigsize, unknown even type), TLV 1 of length 0
 *    2  TLV 1: encoding_type not 0, or a flag that is not a minimal bigsize or runs past the end (common/decode_array.c:45-82)
 *    1  foreign chain_hash: exactly one reply, be16 262 | THEIR chain_hash | 0x00.  DELIBERATE DIFFERENCE: the call stops there; the
 *       reference (:304-310) does not return and goes on to answer from our chain's store.
 *    3  encoded_short_ids does not decode: len 0, first byte not 0, (len - 1) % 8 != 0 (decode_array.c:7-43)
 *    4  the number of flags is not the number of scids
 *    0  answered
 *   "Bad concurrent query" (:320-323) is per-peer state, and so is the pacing of one scid per wakeup: the caller's.  This call returns
 *   the whole answer.  A flag may be any 64-bit bigsize, bits 0..4 are looked at; without TLV 1 every flag is 0x1f.
 * ANSWER of an accepted query, in this order:
 *   1. for each scid OCCURRENCE, in the query's order: the channel_announcement (bit 0), the channel_update of direction 0 (bit 1, if the
 *      slot is set), that of direction 1 (bit 2).  A duplicate scid is answered again, an unknown scid gives nothing.
 *   2. the node_announcements of the distinct nodes asked for with bits 3 (node_id_1) and 4 (node_id_2) over the whole query, in rank
 *      order, each once, for those that have one (uniquify_node_ids, :85-107).
 *   3. reply_short_channel_ids_end: be16 262 | chain_hash32 | 0x01, 35 bytes.
 *   A query with no scid (len == 1) gives the end message alone.  per_query[4 * nq]: scids, known scids, channel messages, node messages
 *   (0, 0, 0, 0 unless answered).
 * SIZES  msg_cap must hold the messages, out_cap the bytes (when out or d_out is given).  One too small: LAMD_ERR_ARG with summary, status,
 *   per_query and reply_first filled in and nothing written to msg_off, msg_rec, out or d_out.  All caps 0: the sizes alone.  The bytes
 *   go to out (host), d_out (device, any alignment), or neither.
 * Device work, on the context's stream: k_sq_lookup (one lane per occurrence: its query by bisection in the prefix sums, the be64 scid
 * byte by byte, two binary searches, its <= 3 records and their sizes -- the be16 len of the record header --, (query << 32 | rank) keys
 * compacted with one atomic per wave), rocPRIM's stable radix sort of all key slots (pads of all-ones), k_cmp_heads, an inclusive scan
 * and k_cmp_merge (each query's distinct nodes in rank order), k_sq_nodes (their announcements), two exclusive scans over occurrences
 * and nodes (messages, bytes), k_sq_per_query and k_range_scan (every query's first message and byte), k_sq_plan (msg_off, msg_rec),
 * k_sq_encode, one aligned 32-bit word of the output per lane, its four bytes built in registers from byte loads.  The host waits once
 * for sizes and offsets and once for the bytes.  Limits: nq and the sum of the scids below UINT32_MAX, qoff non-decreasing, the
 * directory built by this context. */
typedef struct {
	uint64_t by_status[6];   /* queries: [0] answered, [1..4] statuses 1..4, [5] malformed */
	uint64_t scids, known;   /* occurrences in the answered queries; ... of them channels of the store */
	uint64_t channel_messages, node_messages, end_messages;
	uint64_t messages, bytes;   /* what msg_cap and out_cap must hold */
	double stage_ms[4];      /* with lamd_set_timing: lookup, nodes (sort, merge, announcements), plan (scans, per query, offsets), encode */
} lamd_scid_reply_summary;
int lamd_short_channel_ids_reply_batch(lamd_ctx *ctx, const lamd_store_directory *directory, const uint8_t *chain_hash32, size_t nq,
				       const uint8_t *queries, const uint64_t *qoff, int8_t *status, uint32_t *per_query, uint64_t *reply_first,
				       size_t msg_cap, uint64_t *msg_off, uint32_t *msg_rec, uint8_t *out, void *d_out, size_t out_cap,
				       lamd_scid_reply_summary *summary);

/* ---- answering gossip_timestamp_filter from a store image: what handle_gossip_timestamp_filter_in() (connectd/multiplex.c:844-902) sets up
 * and what maybe_gossip_msg() (:622-701) then sends, one gossmap_stream_next() (common/gossmap.c:1873-1981) per wakeup, for a batch of peers
 * at once, as copies of the stored messages.
 *
 * THE STREAM INDEX is built from (image, rec_off, verdict) as a digest is and needs none.  Like the directory it REFERS TO THE IMAGE: a host
 * `store` is copied to the device and owned by the index, a resident d_store is read in place and the caller keeps it alive until
 * lamd_store_stream_free; rec_off is uploaded and kept.  Every device read stays inside the image whatever rec_off holds.  It is a snapshot:
 * rebuild it after a repair.
 *   STREAMABLE  record i, when the first of these that applies is none: its 12-byte header is not inside the image (skipped_frame); DELETED
 *            (0x8000) is set (skipped_deleted); verdict is given and verdict[i] != LAMD_STORE_OK (skipped_verdict); DYING (0x0800) is set
 *            (skipped_dying); its whole message is not inside the image or is shorter than 2 bytes (skipped_frame); its type is not 256,
 *            257 or 258 (skipped_type).
 *   THE LIST    the streamable records in file order, k = 0 .. count - 1: the record index, its HEADER timestamp, its message length; and
 *            for every record i the number of streamable records in front of it.
 *   RECENT(T)   the position in the list of the first streamable record at or behind the first record, of ANY type and whatever its
 *            flags, whose header timestamp is >= T; count if there is none.  (gossmap_iter_fast_forward, gossmap.c:1984-2004, reads raw
 *            headers only.  The reference moves one iterator forward once a minute; every record in front of it had a timestamp below
 *            an older, smaller bound, so a search from the start finds the same record.)  Kept as the inclusive prefix maximum of all
 *            records' header timestamps -- monotone, a record without a header inside the image adds 0 -- and found by bisection.
 * Device work, on the context's stream: k_ts_flag (one lane per record: class, timestamps, length; the counters with one atomic per wave),
 * rocPRIM's exclusive scan of the flags (n + 1 items) and inclusive max-scan of the timestamps, k_ts_compact (the list).  The call waits
 * once, at its end, for the counters. */
typedef struct lamd_store_stream lamd_store_stream;
typedef struct {
	uint64_t streamable;        /* the list's length */
	uint64_t skipped_deleted, skipped_dying, skipped_type, skipped_verdict, skipped_frame;   /* the other records, by reason */
	uint64_t bytes;             /* the streamable messages' lengths, summed */
	double stage_ms[3];         /* with lamd_set_timing: flags, scans, compaction */
} lamd_store_stream_summary;
int lamd_gossip_store_stream_build(lamd_ctx *ctx, const uint8_t *store, size_t len, const void *d_store, size_t n, const uint64_t *rec_off,
				   const int8_t *verdict, lamd_store_stream **stream, lamd_store_stream_summary *summary);
void lamd_store_stream_free(lamd_store_stream *stream);
size_t lamd_store_stream_count(const lamd_store_stream *stream);
/* the list: rec[cap], ts[cap], len[cap]; any may be NULL; cap < count: LAMD_ERR_ARG */
int lamd_store_stream_read(const lamd_store_stream *stream, size_t cap, uint32_t *rec, uint32_t *ts, uint32_t *len);

/* THE REPLIES.  Framing as lamd_short_channel_ids_reply_batch: the filter of peer p is filters + foff[p] .. foff[p + 1], its messages are
 * reply_first[p] .. reply_first[p + 1] - 1, message j is out + msg_off[j] .. msg_off[j + 1]; msg_rec[j] (optional) is the record index
 * the message was copied from.
 * STATUS per peer, parsed on the host:
 *   -1  not a gossip_timestamp_filter: shorter than 42 bytes, or type not 265.  Bytes behind the 42 are ignored (the generated fromwire_
 *       returns cursor != NULL, tools/gen/impl_template:410).  No messages.
 *    1  foreign chain_hash: no messages; the warning is the caller's.
 *    0  streamed: min = first_timestamp, max = first_timestamp + timestamp_range - 1 in 32 bits, UINT32_MAX if that is below min.
 *   A peer that is not streamed gets cursor_out = its cursor_in (UINT64_MAX with a NULL array) and done = 0: its stream is as it was.
 * CURSOR  a position in the list, 0 .. count.  cursor_in[p] == UINT64_MAX, or a NULL array: "as the filter says" -- 0 for first_timestamp
 *   0, count for 0xFFFFFFFF, else RECENT(now - 7200), the subtraction in 32 bits.  Any other value resumes there: the next wakeup of a
 *   throttled peer.  A value above count: LAMD_ERR_ARG.
 * THE WALK from the cursor, in list order: an entry PASSES if its header timestamp ts is 0 or min <= ts <= max.  A passing entry is taken
 *   while the bytes taken so far are <= budget[p] (the check comes before the message, so the last one may overshoot); as soon as they
 *   exceed it the walk stops, cursor_out = the last taken position + 1, done = 0.  When the list ends first: cursor_out = count, done = 1.
 *   budget < 0: nothing is taken, cursor_out = the resolved start, done = 0.  A NULL budget: unlimited.
 *   The per-peer state -- gossip_rcvd_filter, the 60-second timer, dev_suppress_gossip -- and the warnings' text are the caller's.
 * SIZES  as lamd_short_channel_ids_reply_batch: msg_cap must hold the messages, out_cap the bytes (when out or d_out is given).  One too
 *   small: LAMD_ERR_ARG with summary, status, cursor_out, done and reply_first filled in and nothing written to msg_off, msg_rec, out or
 *   d_out.  All caps 0: the sizes alone.  The bytes go to out (host), d_out (device, any alignment), or neither.
 * Device work, on the context's stream: k_tf_select, ONE WAVEFRONT per peer in a one-wave workgroup, walks the list from the cursor in
 * tiles of 64 entries -- coalesced loads of timestamps and lengths, the predicate as a ballot mask, a wave-wide inclusive scan of the
 * passing lengths with cross-lane shuffles, the 64-bit byte total carried across tiles, a stop test that is uniform across the wave, each
 * taken entry's slot from the popcount of the mask below its lane.  It runs twice: a counting pass (messages, bytes, cursor_out, done),
 * k_range_scan over the peers, then, behind the first wait, the writing pass over the same tiles (msg_rec, msg_off) and k_sq_encode,
 * one aligned 32-bit word of the output per lane.  The host waits once for the sizes and once for the bytes; no host round trip inside
 * the walk.  Limits: np and the messages of one call below UINT32_MAX, foff non-decreasing, the index built by this context. */
typedef struct {
	uint64_t by_status[3];   /* peers: [0] streamed, [1] foreign chain, [2] malformed */
	uint64_t messages, bytes;   /* what msg_cap and out_cap must hold */
	uint64_t finished;       /* peers with done = 1 */
	double stage_ms[4];      /* with lamd_set_timing: count, scan, write, encode */
} lamd_filter_reply_summary;
int lamd_timestamp_filter_reply_batch(lamd_ctx *ctx, const lamd_store_stream *stream, const uint8_t *chain_hash32, uint32_t now, size_t np,
				      const uint8_t *filters, const uint64_t *foff, const uint64_t *cursor_in, const int64_t *budget, int8_t *status,
				      uint64_t *cursor_out, uint8_t *done, uint64_t *reply_first, size_t msg_cap, uint64_t *msg_off,
				      uint32_t *msg_rec, uint8_t *out, void *d_out, size_t out_cap, lamd_filter_reply_summary *summary);

/* ---- receiving channel_update batches against a store image on the device: the receive path of gossmap_manage_channel_update() /
 * process_channel_update() (gossipd/gossmap_manage.c:878-1120) for a drained queue of raw messages.  The digest holds what that path asks
 * the gossmap -- every channel by scid and the timestamp in force per direction --, the directory the two node ids of every channel and the
 * image itself.  The call looks the channels up, finds the signers, runs ONE signature batch and applies "newer wins, first among equals"
 * in ARRIVAL ORDER; it returns a verdict per message and the exact bytes and edits gossip_store_add / _del / _set_timestamp
 * (gossipd/gossip_store.c:49-78, 622-670) would make.  It changes neither the image nor the digest nor the directory: apply the plan,
 * then build them again.  The digest and the directory must come from this context and from the same image (LAMD_ERR_ARG otherwise).
 * Message i is msgs + off[i] .. off[i + 1]; source_peers33 + i * peer_stride is the id of the peer it came from (peer_stride 0: one peer for
 * all; NULL: no message has a source; an id that is no valid key -- 33 zero bytes -- verifies nothing, so it stands for "no source").
 * STATUS per message: the first that applies, in the reference's order.
 *   -1  malformed: shorter than 138 bytes, longer than 65535, type not 258, or signature r or s >= n (wire/fromwire.c:196-198).  Bytes behind
 *       the 138 are legal and are signed.
 *    1  wrong chain (:1048-1051)
 *    2  unreasonable timestamp: ts > now + 86400 or ts < now - prune_interval, in unsigned 64-bit arithmetic (:997-1008; prune_interval 0:
 *       1209600)
 *    3  held: the scid is in held_scid (ascending), the caller's pending and too-early announcements (:1060-1097).  The caller queues it.
 *    4  private: the scid is neither a digest entry nor a bare channel, a source peer is given, and the signature verifies under the PEER's
 *       id (:1101-1110)
 *    5  unknown channel (:900-917).  The txout-failure set stays with the caller.
 *    6  bad signature under node_id_1 / node_id_2 of the channel, by channel_flags & 1 (:919-926).  An id that is no valid key, and an
 *       announcement cut off in front of its ids, fail here.
 *    7  DONT_FORWARD: message_flags & 2 (:929-932)
 *    8  stale: ts < the timestamp in force of its slot (channel, direction)       (:935-945)
 *    9  duplicate: ts == the timestamp in force
 *    0  accepted
 *   The timestamp in force of a slot starts as the digest's ts if the slot's record exists, else as "none" (anything that got this far is
 *   accepted), and then becomes the timestamp of each accepted message in turn.  DELIBERATE: the reference compares with the stored record's
 *   HEADER timestamp (gossip_store_get_timestamp), the digest holds the SIGNED one; they are equal in every store gossipd or
 *   lamd_gossip_store_repair_latest wrote.
 * FLAGS per message (0 unless stated):
 *   bit 0  SUPERSEDED   accepted, and a later message of the batch was accepted for the same slot: its record is added, then deleted
 *   bit 1  FIRST        accepted, and the first accepted message, in arrival order over BOTH directions, of a channel whose two slots were
 *                       both empty: it re-stamps the announcement (:946-951)
 *   bit 2  DYING        accepted, and the channel's announcement record carries 0x0800 (:957-962)
 *   bit 3  PEER_UPDATE  accepted and the node of the OTHER direction is our_id33 (:968-978); always set for status 4
 * chan[i]: the directory's channel number -- the digest's entries, then the bare channels --, UINT32_MAX where the channel is unknown or the
 *   status is below 4.
 * THE PLAN
 *   add_msg[j], add_off[j], j < adds: one store record per accepted message, in arrival order: message add_msg[j]'s record starts at byte
 *     add_off[j] of the output and is 12 bytes longer than the message: be16 flags = 0x2000 | 0x0800 if DYING | 0x8000 if SUPERSEDED, be16
 *     len, be32 crc32c seeded with ts, be32 ts, the message -- what the file holds behind its old end after the reference has processed the batch.
 *   del_rec[k], k < deletions: the image records those slots held before, ascending: set their DELETED bit.
 *   set_rec / set_ts / set_crc [k], k < retimestamps: for every FIRST, in arrival order: the announcement record, its new header timestamp
 *     and its recomputed crc.
 * SIZES  as lamd_short_channel_ids_reply_batch: add_cap must hold the adds, edit_cap the deletions and the re-stamps (each list by itself),
 *   out_cap the bytes (when out or d_out is given).  One too small: LAMD_ERR_ARG with summary, status, flags and chan filled in and nothing
 *   written to the plan's arrays, out or d_out.  All caps 0: the verdicts and the sizes alone.  The bytes go to out (host), d_out (device, any
 *   alignment), or neither.
 * Device work, on the context's stream: k_rx_classify (one lane per message: byte loads at any alignment, statuses -1 .. 3, two bisections,
 * the 33-byte signer gathered from the image through the directory, the row's span; rows compacted with one atomic per wave), ONE signature
 * batch over the spans (the audit's form; the spans behind the last row are empty), k_rx_settle, a stable rocPRIM radix sort of the
 * candidates by slot = 2 * chan + direction, an inclusive max-scan over (slot << 33) | (ts + 1) -- slots ascend, so the row in front tells a row
 * its slot's maximum so far, whatever the number of messages aimed at one slot --, k_rx_resolve (accepted iff ts + 1 > max(seed, that);
 * SUPERSEDED from the slot's last row, FIRST from the other slot's head, both by bisection), a sort of the deleted records, three exclusive
 * scans in arrival order, k_rx_plan, and behind the first wait k_rx_encode (headers, CRC-32C) and k_rx_copy (one aligned 32-bit word of the
 * output per lane).  The host waits once for the verdicts and sizes and once for the lists and bytes.  Limits: n below 2^31, fewer than 2^30
 * channels, off non-decreasing. */
typedef struct {
	uint64_t by_status[11];     /* messages: [0] .. [9] statuses 0 .. 9, [10] malformed */
	uint64_t accepted, superseded;
	uint64_t adds, bytes;       /* what add_cap and out_cap must hold */
	uint64_t deletions, retimestamps;   /* what edit_cap must hold, each */
	double stage_ms[5];         /* with lamd_set_timing: classify, signatures, resolve, plan, encode */
	uint64_t signature_rows;    /* the rows of the signature batch */
} lamd_update_receive_summary;
int lamd_channel_update_receive_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const lamd_store_directory *directory,
				      const uint8_t *chain_hash32, uint64_t now, uint32_t prune_interval, const uint8_t *our_id33, size_t n,
				      const uint8_t *msgs, const uint64_t *off, const uint8_t *source_peers33, size_t peer_stride, size_t n_held,
				      const uint64_t *held_scid, int8_t *status, uint8_t *flags, uint32_t *chan, size_t add_cap, uint32_t *add_msg,
				      uint64_t *add_off, uint8_t *out, void *d_out, size_t out_cap, size_t edit_cap, uint32_t *del_rec,
				      uint32_t *set_rec, uint32_t *set_ts, uint32_t *set_crc, lamd_update_receive_summary *summary);

/* ---- receiving node_announcement batches against a store image on the device: the receive path of gossmap_manage_node_announcement() /
 * process_node_announcement() (gossipd/gossmap_manage.c:1122-1248) for a drained queue of raw messages.  The directory holds what that path
 * asks the gossmap: the distinct node ids ranked by memcmp, each node's announcement record in force, the ranks of every channel's two
 * nodes, and the image itself.  The call parses the messages, runs ONE signature batch, each message under its own node_id, and applies
 * "newer wins" in ARRIVAL ORDER; it returns a verdict per message and the exact bytes and edits gossip_store_add / _del
 * (gossipd/gossip_store.c:49-78, 622-653) would make.  It changes neither the image nor the directory: apply the plan, then build them again.
 * The directory must come from this context (LAMD_ERR_ARG otherwise).  Message i is msgs + off[i] .. off[i + 1].  announcements_pending
 * (0 / 1): the caller's pending or too-early channel_announcement maps are not empty (:1225-1226).  There is no chain hash, no clock and no
 * source peer: the reference applies none of them to this message (timestamp_reasonable() is not called on this path, the peer is only scored).
 * STATUS per message: the first that applies, in the reference's order.
 *   -1  malformed (:1186-1199): shorter than 142 bytes (2 + 64 + 2 + flen + 4 + 33 + 3 + 32 + 2 with flen = 0), longer than 65535, type not
 *       257, flen or addrlen past the end, the bytes behind the addresses no valid node_ann_tlvs stream (fromwire_tlv's rules: strictly
 *       ascending types, lengths inside the message, an unknown even type fails, an unknown odd one is skipped; type 1, option_will_fund, has 10
 *       to 14 bytes and a minimal tu32), or signature r or s >= n (wire/fromwire.c:196-198)
 *    1  malformed wireaddrs (:1202-1215, common/wireaddr.c:30-69, 858-889): `addresses` is walked descriptor by descriptor -- type 1: 4
 *       bytes, 2: 16, 3: 10, 4: 35, 5: a length byte, then that many; each followed by a 2-byte port -- and a descriptor is cut off
 *       somewhere, behind its type byte or a type 5's length byte included.  An unknown type ends the walk successfully, whatever follows;
 *       port 0 is ignored, no error.
 *    2  bad signature under the message's own node_id (:1217-1220).  An id that is no valid key fails here.
 *    3  held: the node id is not in the directory and announcements_pending is set (:1225-1233).  The caller queues it.
 *    4  unknown node (:1235-1243)
 *    5  stale: ts < the timestamp in force of its node       (:1133-1140)
 *    6  duplicate: ts == the timestamp in force
 *    0  accepted
 *   The timestamp in force of a node starts as the HEADER timestamp of its announcement record in the image (gossip_store_get_timestamp; the
 *   directory's nann_rec) or, for a node without one, as "none" (anything that got this far is accepted), and then becomes the timestamp of
 *   each accepted message in turn.
 * FLAGS per message (0 unless stated; the bit values of lamd_channel_update_receive_batch):
 *   bit 0  SUPERSEDED   accepted, and a later message of the batch was accepted for the same node: its record is added, then deleted
 *   bit 2  DYING        accepted, and every channel of the node carries 0x0800 on its announcement record (all_node_channels_dying(),
 *                       :288-298, :1145-1149)
 * node[i]: the node's rank in the directory; UINT32_MAX for the statuses -1 and 1 .. 4.
 * THE PLAN
 *   add_msg[j], add_off[j], j < adds: one store record per accepted message, in arrival order, exactly as lamd_channel_update_receive_batch
 *     writes them: be16 flags = 0x2000 | 0x0800 if DYING | 0x8000 if SUPERSEDED, be16 len, be32 crc32c seeded with ts, be32 ts, the message.
 *   del_rec[k], k < deletions: the image records the nodes held before (each deleted by its node's first accepted message), ascending: set
 *     their DELETED bit.
 *   There are no re-stamps.
 * SIZES  as lamd_channel_update_receive_batch: add_cap must hold the adds, edit_cap the deletions, out_cap the bytes (when out or d_out is
 *   given).  One too small: LAMD_ERR_ARG with summary, status, flags and node filled in and nothing written to the plan's arrays, out or
 *   d_out.  All caps 0: the verdicts and the sizes alone.  The bytes go to out (host), d_out (device, any alignment), or neither.
 * Device work, on the context's stream: k_nr_alive (one lane per channel: a channel that is not dying stores a 1 for both of its nodes),
 * k_nr_classify (one lane per message: byte loads at any alignment, statuses -1 and 1, the 33-byte bisection, the row's span; rows compacted
 * with one atomic per wave -- an unknown node has a row too, the reference checks the signature first), ONE signature batch over the spans,
 * k_nr_settle (statuses 2 .. 4), a stable rocPRIM radix sort of the candidates by rank, an inclusive max-scan over (rank << 33) | (ts + 1) --
 * whatever the number of messages aimed at one node --, k_nr_resolve (seeded with the header timestamp read from the image; SUPERSEDED from
 * the node's last row by bisection, DYING from k_nr_alive), a sort of the deleted records, two exclusive scans in arrival order, k_nr_plan, and
 * behind the first wait the update call's k_rx_encode and k_rx_copy.  The host waits once for the verdicts and sizes and once for the lists
 * and bytes.  Limits: n below 2^31, fewer than 2^30 nodes, off non-decreasing. */
typedef struct {
	uint64_t by_status[8];      /* messages: [0] .. [6] statuses 0 .. 6, [7] malformed */
	uint64_t accepted, superseded;
	uint64_t adds, bytes;       /* what add_cap and out_cap must hold */
	uint64_t deletions;         /* what edit_cap must hold */
	uint64_t signature_rows;    /* the rows of the signature batch */
	double stage_ms[5];         /* with lamd_set_timing: classify, signatures, resolve, plan, encode */
} lamd_node_receive_summary;
int lamd_node_announcement_receive_batch(lamd_ctx *ctx, const lamd_store_directory *directory, size_t n, const uint8_t *msgs, const uint64_t *off,
					 int announcements_pending, int8_t *status, uint8_t *flags, uint32_t *node, size_t add_cap,
					 uint32_t *add_msg, uint64_t *add_off, uint8_t *out, void *d_out, size_t out_cap, size_t edit_cap,
					 uint32_t *del_rec, lamd_node_receive_summary *summary);

/* ---- receiving channel_announcement batches against a store image on the device, in the reference's two halves:
 * gossmap_manage_channel_announcement() (gossipd/gossmap_manage.c:620-753) for a drained queue of raw messages, and
 * gossmap_manage_handle_get_txout_reply() (:757-874) for a batch of lightningd's replies.  Between the two lies a map the caller owns: the
 * pending and too-early queues and the txout-failure set stay with the caller, who hands them in as sorted scids.  What is not here: those
 * maps themselves, new_block's promotion of early entries (the caller submits them again, they come back as asks), reprocess_queued_msgs, the
 * warnings' texts, the seeker's remove_unknown_scid, and local (known_amount) announcements.
 *
 * 1. lamd_channel_announcement_receive_batch: message i is msgs + off[i] .. off[i + 1].  Known channels are the digest's entries plus its bare
 * channels; the digest must come from this context (LAMD_ERR_ARG otherwise).  blockheight 0: unknown.  held_scid: the caller's pending and
 * too-early maps together, failed_scid: its txout failures; both strictly ascending (LAMD_ERR_ARG otherwise).  There is no directory, no clock
 * and no peer: the reference uses the source only for the warning, which stays with the caller.
 * STATUS per message: the first that applies, in the reference's order.
 *   -1  malformed (:644-649): shorter than 432 + flen bytes (2 + 4 * 64 + 2 + flen + 32 + 8 + 4 * 33), longer than 65535, type not 256, flen past
 *       the end, r or s of any of the four signatures >= n, or bitcoin_key_1 / bitcoin_key_2 no valid compressed point (fromwire_pubkey).  The
 *       node ids are NOT validated here (fromwire_node_id copies bytes): a bad id fails its signature.  Trailing bytes are legal, and signed.
 *    1  node_id_1 is not memcmp-less than node_id_2 (:659-663)
 *    2  foreign chain (:669-670)
 *    3  the scid is in failed_scid (:677-679)
 *    4  known: a digest entry, a bare channel, or in held_scid (:682-685)
 *    5 .. 8  bad node_signature_1, node_signature_2, bitcoin_signature_1, bitcoin_signature_2: the first that fails (sigcheck.c:78-113)
 *    9  bad gossip order: blockheight != 0 and blocknum(scid) > blockheight + 12 (:722-728)
 *   10  already pending from this batch: an EARLIER message of the batch with the same scid got status 0 or 11 (the map_get of :683-684 seeing
 *       what that message left).  It sits in front of the signature check: a later copy with damaged signatures gets 10, not 5 .. 8; a copy
 *       in front of the first good one gets its own 5 .. 8.
 *   11  early: blocknum + 5 > blockheight, blockheight 0 included (is_scid_depth_announceable).  The caller keeps it in its too-early map.
 *    0  pending: the caller keeps it and asks lightningd.
 * scid[i]: the message's short_channel_id; 0 for status -1.
 * spk34[34 i ..]: for the statuses 0 and 11 scriptpubkey_p2wsh(bitcoin_redeem_2of2()) -- 00 20 SHA256(52 21 <lesser key> 21 <greater key> 52 ae),
 *   the keys ordered by memcmp of their 33 bytes (bitcoin/script.c:149-165) --, 34 zero bytes otherwise.
 * THE ASK LIST  ask_msg[j], ask_scid[j], j < asks: the messages of status 0 in arrival order -- the get_txout requests.
 * SIZES  ask_cap must hold the asks.  Too small: LAMD_ERR_ARG with summary, status, scid and spk34 filled in and nothing written to the list.
 *   ask_cap 0: the verdicts and the size alone.
 * Device work, on the context's stream: k_ca_classify (one lane per message, byte loads at any alignment: framing, the eight scalars, statuses
 * 1 .. 4 by comparisons and four bisections; the rows compacted into TWO lists with one atomic per wave each), ONE signature batch over the spans
 * of the messages that passed the filters, four rows each (a bitcoin key that does not parse makes the message malformed), the key validity
 * kernel over the two bitcoin keys of the messages a filter dropped (the reference calls them malformed BEFORE its filters) -- a batch of known
 * channels costs no signature --, k_ca_settle, a stable rocPRIM radix sort by the 64-bit scid, an inclusive minimum scan by key over the
 * arrival indexes of the good copies, k_ca_resolve per sorted position (statuses 5 .. 11 and 0; no walk of a scid's messages), an exclusive
 * scan in arrival order, k_ca_script (two SHA-256 compressions per lane, the ask list).  The host waits for the two lists' lengths (eight
 * bytes), once for the verdicts and sizes and once for the ask list.  Limits: n below 2^30, off non-decreasing. */
typedef struct {
	uint64_t by_status[13];     /* messages: [0] .. [11] statuses 0 .. 11, [12] malformed */
	uint64_t asks;              /* what ask_cap must hold */
	uint64_t signature_rows;    /* the rows of the signature batch: 4 per message that passed the filters */
	uint64_t keyparse_rows;     /* the keys parsed alone: 2 per message a filter dropped */
	double stage_ms[4];         /* with lamd_set_timing: classify, signatures and keys, resolve, scripts */
} lamd_announce_receive_summary;
int lamd_channel_announcement_receive_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const uint8_t *chain_hash32, uint32_t blockheight,
					    size_t n, const uint8_t *msgs, const uint64_t *off, size_t n_held, const uint64_t *held_scid,
					    size_t n_failed, const uint64_t *failed_scid, int8_t *status, uint64_t *scid, uint8_t *spk34,
					    size_t ask_cap, uint32_t *ask_msg, uint64_t *ask_scid, lamd_announce_receive_summary *summary);

/* 2. lamd_channel_announcement_confirm_batch: digest and directory of the image as it is NOW (one image, this context).  The caller's pending
 * announcements: np raw messages, pending message p = pend_msgs + pend_off[p] .. pend_off[p + 1], well framed and STRICTLY ASCENDING by scid, as the
 * reference's uintmap iterates (anything else: LAMD_ERR_ARG), with their scripts from call 1 in pend_spk34.  nr replies in arrival order: r_scid,
 * r_sat, script r = r_scripts + r_script_off[r] .. r_script_off[r + 1].
 * STATUS per reply, in the reference's order.
 *    1  no pending announcement of that scid (:771-782) -- every reply behind the FIRST one of the same scid in the batch included: map_del
 *       consumed the entry whatever became of it
 *    2  empty script: no unspent output (:791-810)
 *    3  the script is not byte-equal to the pending one; a length other than 34 fails here (:812-819)
 *    4  redundant: the scid is a digest entry or a bare channel (:822-847).  Dropped, and NOT a txout failure.
 *    0  accepted
 * pend[r]: the index of the pending message the reply consumed, UINT32_MAX for status 1.
 * fail_scid[k], k < failures: the scids of the statuses 2 and 3 in reply order; the caller adds them to its failure set.
 * THE PLAN
 *   add_reply[j], add_off[j], j < adds: per accepted reply, in reply order, TWO records back to back, the first at add_off[j]: the announcement --
 *     be16 flags 0x2000, be16 len, be32 crc32c seeded with timestamp 0, be32 timestamp 0, the message -- and gossip_store_channel_amount --
 *     the same header over 10 bytes: be16 4101, be64 sat (:850-852, gossip_store.c:49-78).
 *   clr_rec[k], k < clears: node_announcements_not_dying() (:603-618) for both node ids of every accepted announcement: the node's announcement
 *     record in force (the directory's nann_rec) where its header carries 0x0800; ascending, each record once.  Clear 0x08 of byte 0 of those
 *     headers; the flag lies outside the CRC.
 *   There are no deletions and no re-stamps.
 * SIZES  add_cap must hold the adds, fail_cap the failures, clr_cap the clears, out_cap the bytes (when out or d_out is given).  One too small:
 *   LAMD_ERR_ARG with summary, status and pend filled in and nothing written to the lists, out or d_out.  All caps 0: the verdicts and sizes alone.
 *   The bytes go to out (host), d_out (device, any alignment), or neither.
 * Device work: k_ca_match (a bisection per reply, one 32-bit atomicMin of the reply index per pending slot), k_ca_confirm (the status; per
 * accepted node id a 33-byte bisection and the header of its record), a sort of the dying records and k_ca_clr_heads / k_ca_clr_write (unique),
 * exclusive scans in reply order, k_ca_plan, and behind the first wait the update call's k_rx_encode and k_rx_copy.  The host waits once for the
 * verdicts and sizes and once for the lists and bytes.  Limits: np and nr below 2^30. */
typedef struct {
	uint64_t by_status[5];      /* replies: statuses 0 .. 4 */
	uint64_t adds, bytes;       /* what add_cap and out_cap must hold */
	uint64_t failures;          /* what fail_cap must hold */
	uint64_t clears;            /* what clr_cap must hold */
	double stage_ms[3];         /* with lamd_set_timing: classify, plan, encode */
} lamd_announce_confirm_summary;
int lamd_channel_announcement_confirm_batch(lamd_ctx *ctx, const lamd_store_digest *digest, const lamd_store_directory *directory, size_t np,
					    const uint8_t *pend_msgs, const uint64_t *pend_off, const uint8_t *pend_spk34, size_t nr,
					    const uint64_t *r_scid, const uint64_t *r_sat, const uint8_t *r_scripts, const uint64_t *r_script_off,
					    int8_t *status, uint32_t *pend, size_t add_cap, uint32_t *add_reply, uint64_t *add_off, uint8_t *out,
					    void *d_out, size_t out_cap, size_t fail_cap, uint64_t *fail_scid, size_t clr_cap, uint32_t *clr_rec,
					    lamd_announce_confirm_summary *summary);

/* ---- streaming front end for callers that produce triples one at a time (channeld's
 * commitment_signed loop, channeld/channeld.c:2171,2215-2232; gossip ingest).  Triples are
 * appended to a pinned staging set; flush launches everything queued so far as one batch (asynchronous) and opens the
 * next set, so queueing continues while flushes are in flight: up to 9 flushes may be outstanding (LAMD_ERR_STATE beyond
 * that, until one is collected), successive flushes run on alternating lanes.  A flush's three host-to-device copies go down
 * a copy stream of their own in flush order, so with more flushes outstanding than lanes (4) the rows of the next flush are
 * already in HBM when its lane comes free.  A flush of <= 4096 rows (one commitment_signed) is ONE launch of the latency kernel over the
 * pinned staging rows themselves -- no copies at all; its verdicts arrive through lamd_poll / lamd_wait like any other flush's.  poll/wait return the verdicts of the
 * OLDEST outstanding flush, in submission (ticket) order. */
/* A ticket is the position of the triple's verdict in the vector its flush returns: tickets count 0, 1, 2, ... across
 * the kinds inside the open staging set and restart at 0 after every lamd_flush() (fewer than 2^30 triples per flush). */
int lamd_queue_ecdsa(lamd_ctx *ctx, const uint8_t hash32[32], const uint8_t sig64[64],
		     const uint8_t *pubkey, size_t publen); /* returns the ticket (>= 0) or an error */
int lamd_queue_schnorr(lamd_ctx *ctx, const uint8_t msg32[32], const uint8_t xonly32[32],
		       const uint8_t sig64[64]);
/* n triples at once (row strides 32, 64, pubstride): returns the first ticket, the others follow consecutively */
int lamd_queue_ecdsa_batch(lamd_ctx *ctx, size_t n, const uint8_t *hash32, const uint8_t *sig64, const uint8_t *pubkey,
			   size_t publen, size_t pubstride);
int lamd_queue_schnorr_batch(lamd_ctx *ctx, size_t n, const uint8_t *msg32, const uint8_t *xonly32, const uint8_t *sig64);
/* Zero-copy producer form: queues n triples (keylen 33 / 65: ECDSA with compressed / uncompressed keys; 32: BIP-340 with x-only keys) and
 * returns WHERE their rows live in the pinned staging set -- n rows of 32, 64 and keylen bytes, contiguous -- instead of copying them from
 * a caller-owned buffer.  The caller writes the rows before lamd_flush(); the pointers are valid until the next lamd_queue_* / lamd_flush call
 * on this context (a later push may move the set).  Returns the first ticket like the batch forms. */
int lamd_queue_reserve(lamd_ctx *ctx, size_t n, size_t keylen, uint8_t **hash32, uint8_t **sig64, uint8_t **key);
/* In-place form for a host that ALREADY holds the rows in pinned memory (lamd_served: its clients' shared blocks): the n triples (keys packed, publen
 * / 32 bytes each) get tickets like the batch forms, but their bytes are not copied -- they cross the bus from the caller's buffers when the set is
 * flushed.  The buffers must stay unchanged until the flush that carries the rows has been collected (lamd_poll / lamd_wait).  Batches of <= 4 096
 * rows (the latency kernel reads the staging rows themselves) are copied as by lamd_queue_*_batch, and so is every column that does not lie inside
 * ONE range registered with lamd_host_register(): a column spanning two registrations, one with a pageable hole, and memory pinned by other means
 * (hipHostMalloc, another library's registration) are copied.  lamd_host_register() pins a range for every device (hipHostRegister, portable):
 * register whole, page-aligned blocks, once, and keep them registered while rows of theirs are queued.
 * Both may be called from any thread while another drives the context.  (Replaces nothing in the reference: the producer side of SURVEY.md 8(f)'s
 * sidecar, channeld/channeld.c:7063-7121 being one process per channel.) */
int lamd_queue_ecdsa_batch_inplace(lamd_ctx *ctx, size_t n, const uint8_t *hash32, const uint8_t *sig64, const uint8_t *pubkey, size_t publen);
int lamd_queue_schnorr_batch_inplace(lamd_ctx *ctx, size_t n, const uint8_t *msg32, const uint8_t *xonly32, const uint8_t *sig64);
int lamd_host_register(lamd_ctx *ctx, void *p, size_t bytes);
int lamd_host_unregister(lamd_ctx *ctx, void *p);
/* The NUMA node device `device` hangs on (sysfs), -1 when unknown: run the producer threads and allocate the buffers that feed a device there. */
int lamd_device_numa_node(int device);
/* A failed flush (< 0) drops the rows queued since the previous flush: their tickets are void and no verdicts are reported for them; the
 * engine has stopped reading their buffers (in-place rows included) when it returns, and the next flush carries only rows queued after it. */
int lamd_flush(lamd_ctx *ctx);
/* 1 = finished (ok[0..*n) filled, tickets in submission order), 0 = still running, < 0 error */
int lamd_poll(lamd_ctx *ctx, uint8_t *ok, size_t cap, size_t *n);
int lamd_wait(lamd_ctx *ctx, uint8_t *ok, size_t cap, size_t *n);

/* ---- several MI355X behind one host process (the sidecar that serves a node's channeld / gossipd processes owns every GPU).
 * lamd_multi_init(): one engine context and one host thread per device (devices == NULL: 0 .. n_devices-1), then an RCCL communicator over them
 * (librccl.so is dlopen()ed here, never by a single-GPU process).  A call cuts its rows into n_devices contiguous ranges on GROUP boundaries
 * (lamd_shard_bounds: a channel_announcement's four signatures / a commitment's 1 + 483 rows stay on one device, so a per-key table is built
 * once), copies and verifies every range on its device (the ranges' host-to-device copies run side by side, piece k+1 of a range under the
 * kernels of piece k), all-gathers the verdict bytes ON THE DEVICES (ncclAllGather over xGMI, shards padded to the largest: every device
 * ends with the whole vector) and copies the vector to the host once, from the first device.  A gossip batch made of a few runs of one kind
 * (a replay: its channel_announcements, then its channel_updates) is cut RUN BY RUN -- device i takes range i of every run, in one engine call --
 * so that every device holds the same mix; the verdicts still come back in the caller's order.  Verdicts are exactly those of the
 * single-device calls (lamd_verify_ecdsa_batch, lamd_verify_schnorr_batch, lamd_sigcheck_gossip_batch); with n_devices == 1 the same path
 * runs on one GPU, collective included.  One call at a time per lamd_multi (internally locked); < 0 = LAMD_ERR_*, lamd_multi_last_error(). */
typedef struct lamd_multi lamd_multi;
int lamd_multi_init(lamd_multi **m, const int *devices, int n_devices);
void lamd_multi_shutdown(lamd_multi *m);
const char *lamd_multi_last_error(const lamd_multi *m);
int lamd_multi_devices(const lamd_multi *m);
lamd_ctx *lamd_multi_ctx(lamd_multi *m, int i);   /* device i's engine context (statistics, lamd_get_info); not for concurrent verification calls */
/* group_rows: rows that must stay together (1 = any row boundary; 484 = one commitment_signed; 4 = the rows of a channel_announcement) */
int lamd_multi_verify_ecdsa_batch(lamd_multi *m, size_t n, const uint8_t *hash32, const uint8_t *sig64, const uint8_t *pub, size_t publen,
				  size_t pubstride, size_t group_rows, uint8_t *ok);
int lamd_multi_verify_schnorr_batch(lamd_multi *m, size_t n, const uint8_t *msg32, const uint8_t *xonly32, const uint8_t *sig64, size_t group_rows,
				    uint8_t *ok);
/* raw wire messages as for lamd_sigcheck_gossip_batch: sharded by MESSAGE, balanced by signatures (4 per channel_announcement) */
int lamd_multi_sigcheck_gossip_batch(lamd_multi *m, size_t n, const uint8_t *msgs, const uint64_t *off, const uint8_t *node_ids33, int8_t *verdict);
/* The partition itself: n_groups groups of group_rows[g] rows each (NULL: one row each) into n_shards contiguous ranges of whole groups,
 * balanced by rows; bounds_groups[0..n_shards] (and, if not NULL, bounds_rows[0..n_shards]) receive the cut points.  Shards may be empty. */
int lamd_shard_bounds(size_t n_groups, const uint32_t *group_rows, int n_shards, size_t *bounds_groups, size_t *bounds_rows);

/* Synthetic signed test traffic (the signer kernels tests/ and bench.py use) is NOT in this library: see
 * include/lightning_amd_testgen.h -> liblightning_amd_testgen.so. */

/* Diagnostics (device self-test, arithmetic fuzzers, work-buffer peeks) live in lightning_amd_debug.h: they are exported by the
 * same library but are not part of the drop-in boundary. */

/* ---- introspection for benchmarks / tests */
typedef struct {
	int device;
	int compute_units;
	char arch[64];
	size_t gtable_bytes;
	double last_kernel_ms[4]; /* prep, keys (+ key tables), ecmult, BIP-340 parity stage of the last launch sequence when timing is on */
	/* counts of the last chunk that took the keyed path (read back asynchronously: exact after lamd_synchronize()) */
	size_t last_unique_keys;  /* distinct public keys among the rows the cache did not know */
	size_t last_hot_rows;     /* rows verified against per-key comb tables (the rest took the per-signature ladder) */
	int last_keyed;           /* 0: ladder only; else the largest comb used (7 or 10 teeth) */
	int last_mode;            /* 0: the last chunk was ECDSA, 1: BIP-340 */
	int lanes;                /* number of lanes (LAMD_LANES, default 6; 1 = strictly one stream) */
	size_t last_cache_hits;   /* rows whose key already had a table in the cache */
	size_t last_cold_rows;    /* rows that took the ladder */
	size_t last_new_tables;   /* comb tables built by that chunk */
	size_t last_suspect_rows; /* rows re-decided by the complete addition formulas (crafted scalars / result at infinity) */
	int cache_enabled;        /* LAMD_CACHE (default 1): comb tables persist across calls */
	size_t cache_entries, cache_capacity; /* keys with a cached table (as last read back) / LAMD_CACHE_KEYS + LAMD_CACHE_KEYS10 */
	size_t cache_resets;      /* how often the bounded cache was emptied because it filled up */
	/* the dominant kernel by itself: HIP events right around every large table-driven ecmult launch ([0] ECDSA, [1] BIP-340)
	 * of this lane since lamd_set_timing(ctx, 1); summed by lamd_synchronize() */
	double keyed_ecmult_ms_sum[2];
	size_t keyed_ecmult_launches[2];
	int hw_queues_env;        /* GPU_MAX_HW_QUEUES as lamd_init() found it (0 = unset: the runtime's default of 4; < 16 costs overlap between the lanes) */
	int queue_sets;           /* staging sets of the streaming queue = the most flushes that may be outstanding */
	size_t last_flush_inplace_rows; /* rows the last lamd_flush() sent to the device straight from the callers' registered memory (queued in place, not copied) */
	double last_text_ms[2];   /* with timing on: device time of the last lamd_bolt11_check_batch / lamd_checkmessage_batch / lamd_bolt12_check_text_batch --the front-end kernel; key parse, curve work and merge */
} lamd_info;
int lamd_get_info(lamd_ctx *ctx, lamd_info *info);
int lamd_get_lane_info(lamd_ctx *ctx, int lane, lamd_info *info); /* the last call that ran on lane 0 .. lanes-1 */
int lamd_set_timing(lamd_ctx *ctx, int enable); /* record HIP events around each kernel group; (re)starts the keyed_ecmult_* sums */
/* Empties the key-table cache (drains the device first).  The cache is bounded (LAMD_CACHE_KEYS 7-tooth tables, 2^20 by
 * default = 6.3 GB of HBM; LAMD_CACHE_KEYS10 10-tooth tables, 2^16 = 3.2 GB) and empties itself when it fills up;
 * benchmarks call this to measure the cold path. */
int lamd_cache_clear(lamd_ctx *ctx);
/* Scheduling of the large (>= 65 536 rows) table-driven ecmult launches of successive calls.  0 (default; LAMD_ECMULT_CHAIN): they overlap
 * whenever the lanes let them -- highest throughput (230 against 224 M verifies/s in the pipelined loop), each launch stretched by its
 * neighbour (6.9 ms against 3.1 ms by itself).  1: a launch waits for the one submitted before it -- the kernel saturates the VALU issue
 * port by itself, so what runs under it is only the other lanes' front end (3.9 ms in the loop). */
int lamd_set_ecmult_chain(lamd_ctx *ctx, int enable);
/* Rows per launch sequence ("chunk") of the device-pointer and streaming calls that follow: a call of more rows is cut into chunks that alternate
 * between the call's lane and its peer lane, so that chunk k+1's front end (key de-duplication, tables, row lists) runs under chunk k's ecmult
 * launch.  Default 2^22 (rows == 0 restores it; clamped to [4096, 2^22]).  A caller whose call is the only thing the device has to do -- one rank's
 * shard of a strong-scaling job -- gains by cutting it in two; a caller that keeps several calls in flight leaves it alone (the calls overlap). */
int lamd_set_chunk_rows(lamd_ctx *ctx, size_t rows);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTNING_AMD_H */

// liblightning_amd.so, the front ends: calls that turn transactions, TLV streams and text into the rows the core verifies
#include "engine_internal.h"
#include "key_column.h"
#include "bolt11.h"
#include "bolt12_text.h"

// ---- gossip: per message, double-SHA256 of the signed tail and expansion into (hash, sig, key) rows
// ---- check_tx_sig batches: double-SHA256 of caller-built BIP143 preimages (bitcoin/signature.c:120-151 hashes them
// through libwally) and the sighash-type gate of bitcoin/signature.c:206-211
// (txsig_hash_one / txsig_tx_hash_one / gossip_expand_one / gossip_reduce_one: verify_core.h -- shared by these kernels and by the host-side latency paths,
// and compiled for the host by tests/devmath_host.cpp)
__global__ void __launch_bounds__(256) k_txsig_hash(size_t n, const u8 *__restrict__ pre, const u64 *__restrict__ off,
                                                    const u8 *__restrict__ sighash_type, const u8 *__restrict__ has_witness,
                                                    u8 *__restrict__ hash32, u8 *__restrict__ gate) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  gate[i] = txsig_hash_one(pre + off[i], (size_t)(off[i + 1] - off[i]), sighash_type[i], has_witness[i] != 0, hash32 + 32 * i);
}
// ---- BIP143 on the device, one (transaction, input) per lane: what bip143_sighash() (verify_core.h: the host's form, byte-wise streaming) computes,
// laid out for a wavefront.  The streaming form compiled to 72 k instructions (every shs_update site carries its own unrolled compression: 580 KB of code for
// an instruction cache of 64 KB) with the block buffer in scratch because it is indexed by a run-time byte count: 226 us for the 483 HTLC rows of a
// commitment_signed, a third of it compressions.  Here each of the four streams of a row (hashPrevouts, hashSequence, hashOutputs, the preimage) is laid
// out as a padded message in a per-lane LDS buffer -- word j of lane t at w[j * TXH_LANES + t], so a wave's accesses fall into 64 different banks whatever
// position each lane is at -- and hashed by ONE loop with ONE compression site (the second hash of the double SHA-256 is that loop's last turn).  Bytes
// from global memory are fetched sixteen at a time so that their latencies overlap.  A row whose streams do not fit the buffer never gets here: txsig_pack
// hashes it on the host (TXSIG_DEV_MAX_*).
constexpr int TXH_LANES = 64;
constexpr u32 TXH_WORDS = 240;                      // per lane: 960 bytes = 15 blocks (61 440 bytes of LDS per work-group)
constexpr u32 TXH_MAX_STREAM = 4 * TXH_WORDS - 9;   // 0x80 and the 64-bit length must fit behind the message
__device__ __forceinline__ void txh_put(u32 *w, u32 pos, u32 byte) {  // message byte `pos`; words are big-endian, LDS is little-endian
  reinterpret_cast<u8 *>(w + (size_t)(pos >> 2) * TXH_LANES)[3 - (pos & 3)] = (u8)byte;
}
__device__ __forceinline__ u32 txh_copy(u32 *w, u32 pos, const u8 *__restrict__ p, u32 n) {
#pragma unroll 1
  for (u32 k = 0; k < n; k += 16) {
    u32 b[16];
#pragma unroll
    for (u32 j = 0; j < 16; j++) b[j] = p[k + j < n ? k + j : n - 1];  // sixteen loads in flight; the index is clamped, not predicated
#pragma unroll
    for (u32 j = 0; j < 16; j++)
      if (k + j < n) txh_put(w, pos + k + j, b[j]);
  }
  return pos + n;
}
__device__ __forceinline__ u32 txh_put_be32(u32 *w, u32 pos, u32 v) {
#pragma unroll
  for (int k = 0; k < 4; k++) txh_put(w, pos + k, v >> (24 - 8 * k));
  return pos + 4;
}
__device__ __forceinline__ u32 txh_put_le(u32 *w, u32 pos, u64 v, int bytes) {
  for (int k = 0; k < bytes; k++) txh_put(w, pos + k, (u32)(v >> (8 * k)));
  return pos + bytes;
}
// false: the template is inconsistent (bip143_sighash's cases) or a stream does not fit the buffer; h = SHA256d of the preimage as 8 big-endian words
__device__ __forceinline__ bool bip143_sighash_lane(u32 *w, const tx_view &t, u32 in_idx, const u8 *__restrict__ script, u32 script_len, u64 amount,
                                                    u32 sighash_type, u32 h[8]) {
  if (in_idx >= t.n_in) return false;
  if (t.outputs_len > TXH_MAX_STREAM || (u64)t.n_in * 36 > TXH_MAX_STREAM || (u64)script_len + 165 > TXH_MAX_STREAM) return false;
  const bool acp = (sighash_type & 0x80u) != 0;
  const u32 base = sighash_type & 0x1fu;
  const bool single = base == 3, none = base == 2;
  // the outputs must parse; SINGLE needs the boundaries of output [in_idx]
  size_t at = 0, one_off = 0, one_len = 0;
  for (u32 k = 0; k < t.n_out; k++) {
    if (t.outputs_len - at < 8) return false;
    u64 sl;
    const size_t l = tx_compact_size(t.outputs + at + 8, t.outputs_len - at - 8, &sl);
    if (!l || sl > t.outputs_len - at - 8 - l) return false;
    const size_t len = 8 + l + (size_t)sl;
    if (k == in_idx) { one_off = at; one_len = len; }
    at += len;
  }
  if (at != t.outputs_len) return false;
  u32 hp[8], hs[8], ho[8];
#pragma unroll
  for (int j = 0; j < 8; j++) hp[j] = hs[j] = ho[j] = h[j] = 0;
#pragma unroll 1
  for (int ph = 0; ph < 4; ph++) {
    u32 len = 0;
    bool run = true;
    if (ph == 0) {  // hashPrevouts
      run = !acp;
      if (run)
        for (u32 i = 0; i < t.n_in; i++) len = txh_copy(w, len, t.inputs + 40 * (size_t)i, 36);
    } else if (ph == 1) {  // hashSequence
      run = !acp && !single && !none;
      if (run)
        for (u32 i = 0; i < t.n_in; i++) len = txh_copy(w, len, t.inputs + 40 * (size_t)i + 36, 4);
    } else if (ph == 2) {  // hashOutputs
      if (single) {
        run = in_idx < t.n_out;
        if (run) len = txh_copy(w, 0, t.outputs + one_off, (u32)one_len);
      } else if (none) {
        run = false;
      } else {
        len = txh_copy(w, 0, t.outputs, (u32)t.outputs_len);
      }
    } else {  // nVersion | hashPrevouts | hashSequence | outpoint | varint script | amount | nSequence | hashOutputs | nLockTime | type
      len = txh_put_le(w, len, t.version, 4);
#pragma unroll
      for (int j = 0; j < 8; j++) len = txh_put_be32(w, len, hp[j]);
#pragma unroll
      for (int j = 0; j < 8; j++) len = txh_put_be32(w, len, hs[j]);
      len = txh_copy(w, len, t.inputs + 40 * (size_t)in_idx, 36);
      if (script_len < 0xfd) len = txh_put_le(w, len, script_len, 1);
      else if (script_len <= 0xffff) { len = txh_put_le(w, len, 0xfd, 1); len = txh_put_le(w, len, script_len, 2); }
      else { len = txh_put_le(w, len, 0xfe, 1); len = txh_put_le(w, len, script_len, 4); }
      len = txh_copy(w, len, script, script_len);
      len = txh_put_le(w, len, amount, 8);
      len = txh_copy(w, len, t.inputs + 40 * (size_t)in_idx + 36, 4);
#pragma unroll
      for (int j = 0; j < 8; j++) len = txh_put_be32(w, len, ho[j]);
      len = txh_put_le(w, len, t.locktime, 4);
      len = txh_put_le(w, len, sighash_type, 4);
    }
    if (!run) continue;
    // padding: 0x80, zeros to the last two words of a block, the bit length
    u32 pos = len;
    txh_put(w, pos++, 0x80u);
    while (pos & 3) txh_put(w, pos++, 0u);
    u32 wi = pos >> 2;
    for (; (wi & 15) != 14; wi++) w[(size_t)wi * TXH_LANES] = 0;
    w[(size_t)wi * TXH_LANES] = 0;
    w[(size_t)(wi + 1) * TXH_LANES] = len * 8;
    const u32 nb = (wi + 2) >> 4;
    u32 st[8] = LAMD_SHA256_IV;
#pragma unroll 1
    for (u32 b = 0; b <= nb; b++) {  // turn nb = the second hash, over the first one's digest
      u32 x[16];
      if (b < nb) {
#pragma unroll
        for (u32 j = 0; j < 16; j++) x[j] = w[(size_t)(16 * b + j) * TXH_LANES];
      } else {
        const u32 iv[8] = LAMD_SHA256_IV;
#pragma unroll
        for (int j = 0; j < 8; j++) { x[j] = st[j]; st[j] = iv[j]; }
        x[8] = 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; j++) x[j] = 0;
        x[15] = 256;
      }
      sha256_compress(st, x);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (ph == 0) hp[j] = st[j];
      else if (ph == 1) hs[j] = st[j];
      else if (ph == 2) ho[j] = st[j];
      else h[j] = st[j];
    }
  }
  return true;
}
// hash32 must be 4-byte aligned (it is a device allocation of the context)
__global__ void __launch_bounds__(TXH_LANES) k_txsig_tx_hash(size_t n, const u32 *__restrict__ version, const u32 *__restrict__ locktime,
                                                             const u8 *__restrict__ inputs40, const u64 *__restrict__ in_off,
                                                             const u32 *__restrict__ input_num, const u64 *__restrict__ amount,
                                                             const u8 *__restrict__ outputs, const u64 *__restrict__ out_off,
                                                             const u32 *__restrict__ n_outputs, const u8 *__restrict__ scripts,
                                                             const u64 *__restrict__ script_off, const u8 *__restrict__ sighash_type,
                                                             const u8 *__restrict__ has_witness, const u8 *__restrict__ host_done,
                                                             const u8 *__restrict__ host_hash, u8 *__restrict__ hash32, u8 *__restrict__ gate) {
  __shared__ u32 lds[TXH_WORDS * TXH_LANES];
  const size_t i = (size_t)blockIdx.x * TXH_LANES + threadIdx.x;
  if (i >= n) return;
  if (host_done[i]) {  // a row with a long input / output list or script: the host hashed it (txsig_pack) -- one lane would walk 20 KB of outputs for milliseconds
    for (int b = 0; b < 32; b++) hash32[32 * i + b] = host_hash[32 * i + b];
    gate[i] = host_done[i] == 1;
    return;
  }
  const u8 t = sighash_type[i];
  bool pass = t == 1 || (t == 0x83 && has_witness[i]);  // the gate of bitcoin/signature.c:206-211 (txsig_tx_hash_one)
  u32 h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (pass) {
    tx_view tv;
    tv.version = version[i];
    tv.locktime = locktime[i];
    tv.inputs = inputs40 + 40 * in_off[i];
    tv.n_in = (u32)(in_off[i + 1] - in_off[i]);
    tv.outputs = outputs + out_off[i];
    tv.outputs_len = (size_t)(out_off[i + 1] - out_off[i]);
    tv.n_out = n_outputs[i];
    const u64 sl = script_off[i + 1] - script_off[i];
    pass = sl <= TXH_MAX_STREAM && bip143_sighash_lane(lds + threadIdx.x, tv, input_num[i], scripts + script_off[i], (u32)sl, amount[i], t, h);
  }
  u32 *out = reinterpret_cast<u32 *>(hash32) + 8 * i;
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = pass ? __builtin_bswap32(h[j]) : 0u;
  gate[i] = pass;
}
// ---- BOLT #12: merkle root + tagged signature hash of one TLV stream per lane (bolt12.h); valid[i] = the stream obeys the TLV rules
__global__ void __launch_bounds__(64) k_bolt12_hash(size_t n, const u8 *__restrict__ tlvs, const u64 *__restrict__ off, bolt12_mids mids,
                                                    u8 *__restrict__ root32, u8 *__restrict__ msg32, u8 *__restrict__ valid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u8 root[32], msg[32];
  for (int b = 0; b < 32; b++) root[b] = msg[b] = 0;
  const bool ok = bolt12_merkle_root(tlvs + off[i], (size_t)(off[i + 1] - off[i]), mids, root);
  if (ok) bolt12_sighash(mids, root, msg);
  valid[i] = ok;
  for (int b = 0; b < 32; b++) { if (root32) root32[32 * i + b] = root[b]; msg32[32 * i + b] = msg[b]; }
}
__global__ void __launch_bounds__(256) k_apply_gate(size_t n, const u8 *__restrict__ gate, u8 *__restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !gate[i]) ok[i] = 0;
}

// ---- text front ends, one string per lane (bolt11.h): the columns the recovery and verification launches behind them take.  A row belongs to the
// recovery batch (no `n` key) or to the verification batch (`n` key) only with status 0 so far; for every other row the batch gets what its early
// reject removes -- recovery id 0xFF, a zero signature -- so both batches run over all n rows and nothing is compacted.  A row without an `n` key
// carries the generator as its key: the key-parse kernel and the verification batch see a valid point.
__device__ __constant__ static const u8 TEXT_DUMMY_KEY[33] = {0x02, 0x79, 0xBE, 0x66, 0x7E, 0xF9, 0xDC, 0xBB, 0xAC, 0x55, 0xA0, 0x62, 0x95, 0xCE, 0x87, 0x0B, 0x07,
                                                              0x02, 0x9B, 0xFC, 0xDB, 0x2D, 0xCE, 0x28, 0xD9, 0x59, 0xF2, 0x81, 0x5B, 0x16, 0xF8, 0x17, 0x98};
__global__ void __launch_bounds__(64) k_bolt11_front(size_t n, const u8 *__restrict__ strs, const u64 *__restrict__ off, int8_t *__restrict__ pre,
                                                     u8 *__restrict__ hash32, u8 *__restrict__ sig64, u8 *__restrict__ recid_rec, u8 *__restrict__ sig_ver,
                                                     u8 *__restrict__ key33, u8 *__restrict__ have_n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u8 recid, hn;
  const int st = bolt11_front_one(strs + off[i], (size_t)(off[i + 1] - off[i]), hash32 + 32 * i, sig64 + 64 * i, &recid, key33 + 33 * i, &hn);
  pre[i] = (int8_t)st;
  have_n[i] = hn;
  recid_rec[i] = st == LAMD_B11_OK && !hn ? recid : 0xFF;
  const bool ver = st == LAMD_B11_OK && hn;
  for (int b = 0; b < 64; b++) sig_ver[64 * i + b] = ver ? sig64[64 * i + b] : 0;
  if (!hn)
    for (int b = 0; b < 33; b++) key33[33 * i + b] = TEXT_DUMMY_KEY[b];
}
__global__ void __launch_bounds__(64) k_checkmessage_front(size_t n, const u8 *__restrict__ msgs, const u64 *__restrict__ moff, const u8 *__restrict__ zb,
                                                           const u64 *__restrict__ zoff, int8_t *__restrict__ pre, u8 *__restrict__ hash32,
                                                           u8 *__restrict__ sig64, u8 *__restrict__ recid_rec) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u8 recid;
  const int st = checkmessage_front_one(msgs + moff[i], (size_t)(moff[i + 1] - moff[i]), zb + zoff[i], (size_t)(zoff[i + 1] - zoff[i]), hash32 + 32 * i,
                                        sig64 + 64 * i, &recid);
  pre[i] = (int8_t)st;
  recid_rec[i] = st == LAMD_MSG_OK ? recid : 0xFF;
}
// status and key of a row from what the stages left.  have_n == nullptr (checkmessage): no row has a key of its own.  With one: an `n` key that is
// no point is MALFORMED, in front of what the signature bytes say (the reference parses the key while it walks the fields), and takes the
// row's hash with it.
__global__ void __launch_bounds__(256) k_text_merge(size_t n, const int8_t *__restrict__ pre, u8 *__restrict__ have_n, const u8 *__restrict__ keyok,
                                                    const u8 *__restrict__ ok_ver, const u8 *__restrict__ ok_rec, const u8 *__restrict__ pub_rec,
                                                    const u8 *__restrict__ key33, u8 *__restrict__ hash32, int no_key, int8_t *__restrict__ status,
                                                    u8 *__restrict__ node_id33) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool hn = have_n && have_n[i];
  int st = pre[i];
  if (hn && !keyok[i] && (st == LAMD_B11_OK || st == LAMD_B11_BAD_RECID || st == LAMD_B11_SIG_RANGE)) {
    st = LAMD_B11_MALFORMED;
    have_n[i] = 0;
    for (int b = 0; b < 32; b++) hash32[32 * i + b] = 0;
  }
  if (st == 0) {
    if (hn) st = ok_ver[i] == 1 ? 0 : LAMD_B11_BAD_SIGNATURE;
    else st = ok_rec[i] == 1 ? 0 : no_key;
  }
  status[i] = (int8_t)st;
  const u8 *src = hn ? key33 + 33 * i : pub_rec + 33 * i;
  for (int b = 0; b < 33; b++) node_id33[33 * i + b] = st == 0 ? src[b] : 0;
}

// ---- BOLT #12 from its text, one string per lane (bolt12_text.h).  Row i decodes into scratch[off[i] .. off[i+1]): a string never decodes to more bytes
// than it has, so the rows cannot overlap.  Only a row with status 0 so far and a key of its own (an invoice request, an invoice) belongs to the BIP-340
// batch; every other row gets what the batch's early reject removes -- a zero signature under the generator's x -- so the batch runs over all n rows.
// key33 keeps a present key whatever the status behind it (-5, -7, 0), for the key-parse kernel's validity byte; without one it holds the generator.
__global__ void __launch_bounds__(64) k_bolt12_text_front(size_t n, const u8 *__restrict__ strs, const u64 *__restrict__ off, u8 *__restrict__ scratch,
                                                          bolt12_text_mids mids, int8_t *__restrict__ pre, u8 *__restrict__ kind, u8 *__restrict__ have_key,
                                                          u8 *__restrict__ key33, u8 *__restrict__ xonly, u8 *__restrict__ sig64, u8 *__restrict__ hash32,
                                                          u8 *__restrict__ offer_id, u8 *__restrict__ invreq_id) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t len = (size_t)(off[i + 1] - off[i]);
  size_t dlen;
  u8 kd, hk;
  const int st = bolt12_text_front_one(strs + off[i], len, scratch + off[i], len, &dlen, mids, &kd, key33 + 33 * i, &hk, sig64 + 64 * i, hash32 + 32 * i,
                                       offer_id + 32 * i, invreq_id + 32 * i);
  pre[i] = (int8_t)st;
  kind[i] = kd;
  have_key[i] = hk;
  const bool ver = st == LAMD_B12_OK && kd != LAMD_B12_KIND_OFFER;
  for (int b = 0; b < 32; b++) xonly[32 * i + b] = ver ? key33[33 * i + 1 + b] : TEXT_DUMMY_KEY[1 + b];
  if (!hk)
    for (int b = 0; b < 33; b++) key33[33 * i + b] = TEXT_DUMMY_KEY[b];
}
// status, signer and ids of a row from what the stages left.  A present key that is no curve point is MALFORMED (fromwire_pubkey fails inside
// fromwire_tlv), ahead of what the ranges, field 240 and the signature say, and takes the row's hash with it.
__global__ void __launch_bounds__(256) k_bolt12_text_merge(size_t n, const int8_t *__restrict__ pre, const u8 *__restrict__ kind, const u8 *__restrict__ have_key,
                                                           const u8 *__restrict__ keyok, const u8 *__restrict__ ok_ver, const u8 *__restrict__ key33,
                                                           u8 *__restrict__ hash32, u8 *__restrict__ offer_id, u8 *__restrict__ invreq_id,
                                                           int8_t *__restrict__ status, u8 *__restrict__ signer33) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int st = pre[i];
  const bool own_key = kind[i] == LAMD_B12_KIND_INVREQ || kind[i] == LAMD_B12_KIND_INVOICE;
  if (have_key[i] && !keyok[i] && (st == LAMD_B12_OK || st == LAMD_B12_OUT_OF_RANGE || st == LAMD_B12_NO_SIGNATURE)) {
    st = LAMD_B12_MALFORMED;
    for (int b = 0; b < 32; b++) hash32[32 * i + b] = 0;
  }
  if (st == LAMD_B12_OK && own_key) st = ok_ver[i] == 1 ? LAMD_B12_OK : LAMD_B12_BAD_SIGNATURE;
  status[i] = (int8_t)st;
  if (st != LAMD_B12_OK)
    for (int b = 0; b < 32; b++) offer_id[32 * i + b] = invreq_id[32 * i + b] = 0;
  for (int b = 0; b < 33; b++) signer33[33 * i + b] = st == LAMD_B12_OK && own_key ? key33[33 * i + b] : 0;
}

// ---- fee grind (verify_core.h "fee grind"): one thread prepares, one thread per candidate feerate
__global__ void __launch_bounds__(64) k_grind_setup(const u8 *__restrict__ sig64, const u8 *__restrict__ pub33,
                                                    const u8 *__restrict__ pre, u32 lead_blocks, u32 *__restrict__ slot,
                                                    const u32 *__restrict__ gtable, grind_setup *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  grind_setup g;
  grind_prepare(&g, sig64, pub33, pre, lead_blocks, slot, gtable);
  *out = g;
}
// candidate c = feerate min_rate + c; *best = the smallest matching c (0xFFFFFFFF: none)
__global__ void __launch_bounds__(256) k_grind(u32 ncand, u32 min_rate, u64 weight, u64 input_sat, const u8 *__restrict__ tail,
                                               u32 tail_len, u32 lead_bytes, const u8 *__restrict__ outputs, u32 outputs_len,
                                               const grind_setup *__restrict__ setup, const u32 *__restrict__ gtable,
                                               u32 *__restrict__ best) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncand || !setup->valid) return;
  if (grind_candidate(c, min_rate, weight, input_sat, tail, tail_len, lead_bytes, outputs, outputs_len, *setup, gtable)) atomicMin(best, c);
}

// ---- what the calls with a gate share (a row whose gate byte is 0 is rejected whatever its signature says)
// the latency path under a gate the host made.  LAMD_OK: verdicts in ok[]; 1: a key the latency path met before without a table is back -- the caller takes
// the batch path, which learns it (force_learn is set); else an error
static int run_small_gated(lamd_ctx *ctx, int mode, size_t n, const u8 *hash32, const u8 *sig64, const u8 *key, int keylen, size_t keystride, const u8 *gate,
                           u8 *ok) {
  const int rc = run_small(ctx, mode, n, hash32, sig64, key, keylen, keystride, ok);
  if (rc == 1) ctx->force_learn = true;
  if (rc != LAMD_OK) return rc;
  for (size_t i = 0; i < n; i++)
    if (!gate[i]) ok[i] = 0;
  return LAMD_OK;
}
// the batch path under a gate the device made: hashes in in_a, signatures in in_b, keys in in_c, the gate in g_malformed; verdicts through `out`
static int run_device_gated(lamd_ctx *ctx, int mode, size_t n, int keylen, size_t keystride, u8 *ok) {
  const int rc = run_device(ctx, mode, n, ctx->in_a.as<const u8>(), ctx->in_b.as<const u8>(), ctx->in_c.as<const u8>(), keylen, keystride, ctx->out.as<u8>());
  ctx->force_learn = false;
  if (rc != LAMD_OK) return rc;
  hipLaunchKernelGGL(k_apply_gate, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, n, ctx->g_malformed.as<const u8>(), ctx->out.as<u8>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(ok, ctx->out.p, n, hipMemcpyDeviceToHost, ctx->stream));
  return lamd_synchronize(ctx);   // (what the caller uploaded from its frame has been read when this returns)
}

// ---- check_tx_sig batches
constexpr size_t TXSIG_HOST_HASH_ROWS = 16;  // check_tx_sig batches up to here hash on the host (one launch); above, on the device (two launches)
extern "C" int lamd_check_tx_sig_batch(lamd_ctx *ctx, size_t n, const uint8_t *preimages, const uint64_t *off, const uint8_t *sighash_type,
                                       const uint8_t *has_witness, const uint8_t *sig64, const uint8_t *pub, size_t publen, size_t pubstride,
                                       uint8_t *ok) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!preimages || !off || !sighash_type || !has_witness || !sig64 || !pub || !ok || (publen != 33 && publen != 65) || pubstride < publen) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  size_t keybytes;
  if (!lamd::key_column_bytes(n, publen, pubstride, &keybytes)) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  // a few rows (an unmodified channeld checks ONE signature per check_tx_sig() call, channeld.c:2171,2224): gate + double SHA-256 on the
  // host -- the kernel's own inline function -- and the rows through the one-launch latency path
  if (small_path(ctx, n) && ctx->keyed_mode <= 0) {
    if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
    std::vector<u8> hs(32 * n), gate(n);
    for (size_t i = 0; i < n; i++) gate[i] = txsig_hash_one(preimages + off[i], (size_t)(off[i + 1] - off[i]), sighash_type[i], has_witness[i] != 0, &hs[32 * i]);
    if ((rc = run_small_gated(ctx, MODE_ECDSA, n, hs.data(), sig64, pub, (int)publen, pubstride, gate.data(), ok)) != 1) return rc;
  }
  const size_t total = off[n] - off[0];
  std::vector<u64> rel(n + 1);
  for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
  if ((rc = ensure(ctx, &ctx->g_msgs, total + 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_off, (n + 1) * 8)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_ids, 2 * n)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_malformed, n)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_a, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_b, n * 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_c, keybytes)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->out, n)) != LAMD_OK) return rc;
  u8 *d_types = ctx->g_ids.as<u8>(), *d_wit = d_types + n;
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_msgs.p, preimages + off[0], total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_types, sighash_type, n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_wit, has_witness, n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_b.p, sig64, n * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_c.p, pub, keybytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_txsig_hash, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, n, ctx->g_msgs.as<const u8>(), ctx->g_off.as<const u64>(),
                     (const u8 *)d_types, (const u8 *)d_wit, ctx->in_a.as<u8>(), ctx->g_malformed.as<u8>());
  HIPCHK(ctx, hipGetLastError());
  return run_device_gated(ctx, MODE_ECDSA, n, (int)publen, pubstride, ok);
}

// ---- check_tx_sig from transaction templates: the templates of a call as ONE staging blob (fixed-width columns first, 16-byte aligned, then the
// three byte strings; offsets relative to the call's first row) and the hashing kernel over it
struct txsig_blob {
  std::vector<u8> st;
  size_t o_inoff, o_outoff, o_scoff, o_amt, o_ver, o_lock, o_inum, o_nout, o_type, o_wit, o_in, o_out, o_sc, o_hdone, o_hhash, total;
};
// A row whose transaction has long lists (a commitment transaction with its 485 outputs: 20 KB under hashOutputs) or a very long script is hashed on the HOST
// while the blob is packed: SHA-256 is sequential, one lane needed ~6.5 ms for the 20 KB (measured: the whole 484-row call took that long), a host core
// ~0.1 ms; and the device's per-lane message buffer (k_txsig_tx_hash) holds 951 bytes per stream.  host_done: 0 = the device hashes the row, 1 = hashed here
// and the gate passed, 2 = hashed here and the gate refused.
constexpr size_t TXSIG_DEV_MAX_OUT = 900, TXSIG_DEV_MAX_IN = 25, TXSIG_DEV_MAX_SCRIPT = 700;  // each stream of a device row stays below TXH_MAX_STREAM
static_assert(TXSIG_DEV_MAX_OUT <= TXH_MAX_STREAM && 36 * TXSIG_DEV_MAX_IN <= TXH_MAX_STREAM && TXSIG_DEV_MAX_SCRIPT + 165 <= TXH_MAX_STREAM, "device rows must fit the lane buffer");
static void txsig_pack(txsig_blob &B, size_t n, const uint32_t *version, const uint32_t *locktime, const uint8_t *inputs40, const uint64_t *in_off,
                       const uint32_t *input_num, const uint64_t *amount_sat, const uint8_t *outputs, const uint64_t *out_off, const uint32_t *n_outputs,
                       const uint8_t *scripts, const uint64_t *script_off, const uint8_t *sighash_type, const uint8_t *has_witness) {
  const size_t nin = (size_t)(in_off[n] - in_off[0]), nout_b = (size_t)(out_off[n] - out_off[0]), nsc = (size_t)(script_off[n] - script_off[0]);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
  B.o_inoff = take((n + 1) * 8); B.o_outoff = take((n + 1) * 8); B.o_scoff = take((n + 1) * 8); B.o_amt = take(n * 8); B.o_ver = take(n * 4);
  B.o_lock = take(n * 4); B.o_inum = take(n * 4); B.o_nout = take(n * 4); B.o_type = take(n); B.o_wit = take(n); B.o_in = take(nin * 40 + 16);
  B.o_out = take(nout_b + 16); B.o_sc = take(nsc + 16); B.o_hdone = take(n); B.o_hhash = take(32 * n); B.total = o;
  B.st.assign(B.total, 0);
  std::vector<u8> &st = B.st;
  auto rel = [&](size_t at, const uint64_t *src) { for (size_t i = 0; i <= n; i++) ((u64 *)&st[at])[i] = src[i] - src[0]; };
  rel(B.o_inoff, in_off); rel(B.o_outoff, out_off); rel(B.o_scoff, script_off);
  memcpy(&st[B.o_amt], amount_sat, n * 8); memcpy(&st[B.o_ver], version, n * 4); memcpy(&st[B.o_lock], locktime, n * 4);
  memcpy(&st[B.o_inum], input_num, n * 4); memcpy(&st[B.o_nout], n_outputs, n * 4); memcpy(&st[B.o_type], sighash_type, n); memcpy(&st[B.o_wit], has_witness, n);
  memcpy(&st[B.o_in], inputs40 + 40 * in_off[0], nin * 40); memcpy(&st[B.o_out], outputs + out_off[0], nout_b); memcpy(&st[B.o_sc], scripts + script_off[0], nsc);
  for (size_t i = 0; i < n; i++)
    if ((size_t)(out_off[i + 1] - out_off[i]) > TXSIG_DEV_MAX_OUT || (size_t)(in_off[i + 1] - in_off[i]) > TXSIG_DEV_MAX_IN ||
        (size_t)(script_off[i + 1] - script_off[i]) > TXSIG_DEV_MAX_SCRIPT) {
      const bool pass = txsig_tx_hash_one(i, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type,
                                          has_witness, &st[B.o_hhash + 32 * i]);
      st[B.o_hdone + i] = pass ? 1 : 2;
    }
}
// BIP143 hash + gate of every row of the blob at `d` (device memory, or pinned device-mapped host memory) -> d_hash32, d_gate
static int txsig_hash_launch(lamd_ctx *ctx, size_t n, const txsig_blob &B, const u8 *d, u8 *d_hash32, u8 *d_gate) {
  hipLaunchKernelGGL(k_txsig_tx_hash, dim3((unsigned)((n + TXH_LANES - 1) / TXH_LANES)), dim3(TXH_LANES), 0, ctx->stream, n, (const u32 *)(d + B.o_ver), (const u32 *)(d + B.o_lock), d + B.o_in,
                     (const u64 *)(d + B.o_inoff), (const u32 *)(d + B.o_inum), (const u64 *)(d + B.o_amt), d + B.o_out, (const u64 *)(d + B.o_outoff),
                     (const u32 *)(d + B.o_nout), d + B.o_sc, (const u64 *)(d + B.o_scoff), d + B.o_type, d + B.o_wit, d + B.o_hdone, d + B.o_hhash, d_hash32, d_gate);
  HIPCHK(ctx, hipGetLastError());
  return LAMD_OK;
}
// the general path: templates to the device, BIP143 hashes there, the batch machinery, the gate, verdicts back
static int txsig_tx_general(lamd_ctx *ctx, size_t n, const uint32_t *version, const uint32_t *locktime, const uint8_t *inputs40, const uint64_t *in_off,
                            const uint32_t *input_num, const uint64_t *amount_sat, const uint8_t *outputs, const uint64_t *out_off, const uint32_t *n_outputs,
                            const uint8_t *scripts, const uint64_t *script_off, const uint8_t *sighash_type, const uint8_t *has_witness, const uint8_t *sig64,
                            const uint8_t *pub, size_t publen, size_t pubstride, uint8_t *ok) {
  int rc;
  size_t keybytes;
  if (!lamd::key_column_bytes(n, publen, pubstride, &keybytes)) { ctx->err = "bad argument"; ctx->force_learn = false; return LAMD_ERR_ARG; }
  txsig_blob B;
  txsig_pack(B, n, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type, has_witness);
  if ((rc = ensure(ctx, &ctx->g_msgs, B.total)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_malformed, n)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_a, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_b, n * 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_c, keybytes)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->out, n)) != LAMD_OK) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_msgs.p, B.st.data(), B.total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_b.p, sig64, n * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_c.p, pub, keybytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = txsig_hash_launch(ctx, n, B, ctx->g_msgs.as<const u8>(), ctx->in_a.as<u8>(), ctx->g_malformed.as<u8>())) != LAMD_OK) return rc;
  return run_device_gated(ctx, MODE_ECDSA, n, (int)publen, pubstride, ok);  // (B.st is pageable: the runtime staged it before hipMemcpyAsync returned)
}

// <= SMALL_MAX rows with the BIP143 hashes made ON THE DEVICE: the templates go into a pinned block, ONE asynchronous copy takes them to HBM, k_txsig_tx_hash
// leaves hashes and gate in device memory, k_small_verify -- queued right behind it -- takes them from there.  One small copy, two launches.  (Hashing on
// the host, which the small callers do for a handful of rows, is ~12 SHA-256 compressions per row: 1.7 ms for a 484-row commitment, 14 ms for eight of them.)
// LAMD_OK: verdicts in ok[]; 1: a key the latency path met before without a table is back -- the caller takes the batch path (force_learn is set).
static int txsig_small_device(lamd_ctx *ctx, size_t n, const uint32_t *version, const uint32_t *locktime, const uint8_t *inputs40, const uint64_t *in_off,
                              const uint32_t *input_num, const uint64_t *amount_sat, const uint8_t *outputs, const uint64_t *out_off, const uint32_t *n_outputs,
                              const uint8_t *scripts, const uint64_t *script_off, const uint8_t *sighash_type, const uint8_t *has_witness, const uint8_t *sig64,
                              const uint8_t *pub, size_t publen, size_t pubstride, uint8_t *ok) {
  int rc;
  txsig_blob B;
  txsig_pack(B, n, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type, has_witness);
  if (ctx->tmpl.cap < B.total) {
    if (ctx->tmpl.h) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipHostFree(ctx->tmpl.h); ctx->tmpl.h = nullptr; ctx->tmpl.cap = 0; }
    const size_t want = B.total + B.total / 2 + 4096;
    HIPCHK(ctx, hipHostMalloc((void **)&ctx->tmpl.h, want, hipHostMallocMapped | hipHostMallocCoherent));
    ctx->tmpl.cap = want;
  }
  if ((rc = ensure(ctx, &ctx->in_a, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_malformed, n)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_msgs, B.total)) != LAMD_OK) return rc;
  memcpy(ctx->tmpl.h, B.st.data(), B.total);
  // one asynchronous copy of the block (pinned -> HBM, ~250 B per row), then the hashing kernel over HBM.  The first version of this path let the kernel
  // read the templates where they lay, through the device mapping of the pinned block: 484 lanes walking ~250 bytes each byte by byte over PCIe took 6.5 ms
  // (rocprofv3, tools/commit_trace_probe.py) -- reading host memory from a kernel is fine for one 161-byte row, not for a SHA-256 input stream.
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_msgs.p, ctx->tmpl.h, B.total, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = txsig_hash_launch(ctx, n, B, ctx->g_msgs.as<const u8>(), ctx->in_a.as<u8>(), ctx->g_malformed.as<u8>())) != LAMD_OK) return rc;
  rc = run_small(ctx, MODE_ECDSA, n, nullptr, sig64, pub, (int)publen, pubstride, ok, ctx->in_a.as<const u8>(), ctx->g_malformed.as<const u8>());
  if (rc == 1) ctx->force_learn = true;
  return rc;
}

extern "C" int lamd_check_tx_sig_tx_batch(lamd_ctx *ctx, size_t n, const uint32_t *version, const uint32_t *locktime, const uint8_t *inputs40,
                                          const uint64_t *in_off, const uint32_t *input_num, const uint64_t *amount_sat, const uint8_t *outputs,
                                          const uint64_t *out_off, const uint32_t *n_outputs, const uint8_t *scripts, const uint64_t *script_off,
                                          const uint8_t *sighash_type, const uint8_t *has_witness, const uint8_t *sig64, const uint8_t *pub,
                                          size_t publen, size_t pubstride, uint8_t *ok) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!version || !locktime || !inputs40 || !in_off || !input_num || !amount_sat || !outputs || !out_off || !n_outputs || !scripts || !script_off ||
      !sighash_type || !has_witness || !sig64 || !pub || !ok || (publen != 33 && publen != 65) || pubstride < publen) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
  if (small_path(ctx, n) && ctx->keyed_mode <= 0 && n <= TXSIG_HOST_HASH_ROWS) {
    // a handful of rows: BIP143 hash on the host (the kernels' own inline function), rows through the latency path in ONE launch
    std::vector<u8> hs(32 * n), gate(n);
    for (size_t i = 0; i < n; i++)
      gate[i] = txsig_tx_hash_one(i, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type,
                                  has_witness, &hs[32 * i]);
    if ((rc = run_small_gated(ctx, MODE_ECDSA, n, hs.data(), sig64, pub, (int)publen, pubstride, gate.data(), ok)) != 1) return rc;
  } else if (small_path(ctx, n) && ctx->keyed_mode <= 0) {  // up to 4 096 rows (several commitments at once: lamd_served's merged call): hashes on the device
    rc = txsig_small_device(ctx, n, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type, has_witness,
                            sig64, pub, publen, pubstride, ok);
    if (rc != 1) return rc;
  }
  return txsig_tx_general(ctx, n, version, locktime, inputs40, in_off, input_num, amount_sat, outputs, out_off, n_outputs, scripts, script_off, sighash_type,
                          has_witness, sig64, pub, publen, pubstride, ok);
}

// ---- one commitment_signed as ONE call (channeld/channeld.c:2171-2232): include/lightning_amd.h
extern "C" int lamd_check_commitment_signed(lamd_ctx *ctx, const lamd_tx_template *commit_tx, const uint8_t remote_funding33[33], const uint8_t commit_sig64[64],
                                            uint8_t commit_sighash_type, size_t n_htlc, const lamd_tx_template *htlc_txs, const uint8_t remote_htlckey33[33],
                                            const uint8_t *htlc_sigs64, const uint8_t *htlc_sighash_types, int64_t *first_bad, uint8_t *ok_rows) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!commit_tx || !remote_funding33 || !commit_sig64 || !first_bad || (n_htlc && (!htlc_txs || !remote_htlckey33 || !htlc_sigs64 || !htlc_sighash_types))) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  *first_bad = 0;  // fails closed: an error return never leaves "all good" behind
  const size_t n = 1 + n_htlc;
  // the 1 + N (transaction, input 0 .. , signature) rows in the reference's order: row 0 the commitment transaction under the funding key,
  // row 1 + i HTLC transaction i under the htlc key
  std::vector<uint32_t> version(n), locktime(n), input_num(n), n_outputs(n);
  std::vector<uint64_t> in_off(n + 1), out_off(n + 1), sc_off(n + 1), amount(n);
  std::vector<u8> type(n), wit(n, 1), sig(64 * n), pub(33 * n);
  size_t nin = 0, nout = 0, nsc = 0;
  for (size_t i = 0; i < n; i++) {
    const lamd_tx_template *t = i ? &htlc_txs[i - 1] : commit_tx;
    if ((t->n_inputs && !t->inputs40) || (t->outputs_len && !t->outputs) || (t->script_len && !t->script)) {
      ctx->err = "bad argument: transaction template with a null array";
      return LAMD_ERR_ARG;
    }
    in_off[i] = nin; out_off[i] = nout; sc_off[i] = nsc;
    nin += t->n_inputs; nout += t->outputs_len; nsc += t->script_len;
  }
  in_off[n] = nin; out_off[n] = nout; sc_off[n] = nsc;
  std::vector<u8> inputs(40 * nin + 1), outputs(nout + 1), scripts(nsc + 1);
  for (size_t i = 0; i < n; i++) {
    const lamd_tx_template *t = i ? &htlc_txs[i - 1] : commit_tx;
    version[i] = t->version; locktime[i] = t->locktime; input_num[i] = t->input_num; n_outputs[i] = t->n_outputs; amount[i] = t->amount_sat;
    if (t->n_inputs) memcpy(&inputs[40 * in_off[i]], t->inputs40, 40 * (size_t)t->n_inputs);
    if (t->outputs_len) memcpy(&outputs[out_off[i]], t->outputs, t->outputs_len);
    if (t->script_len) memcpy(&scripts[sc_off[i]], t->script, t->script_len);
    type[i] = i ? htlc_sighash_types[i - 1] : commit_sighash_type;
    memcpy(&sig[64 * i], i ? htlc_sigs64 + 64 * (i - 1) : commit_sig64, 64);
    memcpy(&pub[33 * i], i ? remote_htlckey33 : remote_funding33, 33);
  }
  std::vector<u8> okv(n, 0);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
  bool done = false;
  if (small_path(ctx, n) && ctx->keyed_mode <= 0) {
    rc = txsig_small_device(ctx, n, version.data(), locktime.data(), inputs.data(), in_off.data(), input_num.data(), amount.data(), outputs.data(), out_off.data(),
                            n_outputs.data(), scripts.data(), sc_off.data(), type.data(), wit.data(), sig.data(), pub.data(), 33, 33, okv.data());
    if (rc == LAMD_OK) done = true;
    else if (rc != 1) return rc;   // 1: a key the latency path met before without a table is back (the channel's htlc key): built and published below
  }
  if (!done) {
    rc = txsig_tx_general(ctx, n, version.data(), locktime.data(), inputs.data(), in_off.data(), input_num.data(), amount.data(), outputs.data(), out_off.data(),
                          n_outputs.data(), scripts.data(), sc_off.data(), type.data(), wit.data(), sig.data(), pub.data(), 33, 33, okv.data());
    if (rc != LAMD_OK) return rc;
  }
  int64_t bad = -1;
  for (size_t i = 0; i < n && bad < 0; i++)
    if (!okv[i]) bad = (int64_t)i;  // 0: the commitment signature (:2171), 1 + i: htlc_sigs[i] (:2224) -- the first in the reference's order
  *first_bad = bad;
  if (ok_rows) memcpy(ok_rows, okv.data(), n);
  return LAMD_OK;
}

// ---- BOLT #12 signatures: n independent bolt12_check_signature(fields, messagename, fieldname, key, sig) calls (common/bolt12.c:80-92)
// the three tag midstates of a BOLT #12 signature: "LnLeaf", "LnBranch", "lightning" || messagename || fieldname (bitcoin/signature.c:389-405)
static bolt12_mids bolt12_make_mids(const char *messagename, const char *fieldname) {
  bolt12_mids mids;
  const u8 leaf[6] = {'L', 'n', 'L', 'e', 'a', 'f'}, branch[8] = {'L', 'n', 'B', 'r', 'a', 'n', 'c', 'h'};
  bolt12_tag_midstate(leaf, 6, leaf, 0, mids.leaf);
  bolt12_tag_midstate(branch, 8, branch, 0, mids.branch);
  const std::string tag2 = std::string(messagename) + fieldname;
  bolt12_tag_midstate((const u8 *)"lightning", 9, (const u8 *)tag2.data(), tag2.size(), mids.sig);
  return mids;
}
static int bolt12_hash_device(lamd_ctx *ctx, size_t n, const uint8_t *tlvs, const uint64_t *off, const char *messagename, const char *fieldname,
                              u8 *d_root, u8 *d_msg, u8 *d_valid) {
  const size_t total = (size_t)(off[n] - off[0]);
  std::vector<u64> rel(n + 1);
  for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
  int rc;
  if ((rc = ensure(ctx, &ctx->g_msgs, total + 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_off, (n + 1) * 8)) != LAMD_OK) return rc;
  const bolt12_mids mids = bolt12_make_mids(messagename, fieldname);
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_msgs.p, tlvs + off[0], total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->g_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // rel lives on this frame
  hipLaunchKernelGGL(k_bolt12_hash, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, n, ctx->g_msgs.as<const u8>(), ctx->g_off.as<const u64>(), mids,
                     d_root, d_msg, d_valid);
  HIPCHK(ctx, hipGetLastError());
  return LAMD_OK;
}
extern "C" int lamd_bolt12_merkle_batch(lamd_ctx *ctx, size_t n, const uint8_t *tlvs, const uint64_t *off, const char *messagename,
                                        const char *fieldname, uint8_t *merkle32, uint8_t *sighash32, uint8_t *ok) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!tlvs || !off || !messagename || !fieldname || !ok) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, &ctx->in_a, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_b, n * 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_malformed, n)) != LAMD_OK) return rc;
  if ((rc = bolt12_hash_device(ctx, n, tlvs, off, messagename, fieldname, ctx->in_b.as<u8>(), ctx->in_a.as<u8>(), ctx->g_malformed.as<u8>())) != LAMD_OK) return rc;
  if (merkle32) HIPCHK(ctx, hipMemcpyAsync(merkle32, ctx->in_b.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (sighash32) HIPCHK(ctx, hipMemcpyAsync(sighash32, ctx->in_a.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ok, ctx->g_malformed.p, n, hipMemcpyDeviceToHost, ctx->stream));
  return lamd_synchronize(ctx);
}
extern "C" int lamd_bolt12_check_signature_batch(lamd_ctx *ctx, size_t n, const uint8_t *tlvs, const uint64_t *off, const char *messagename,
                                                 const char *fieldname, const uint8_t *key33, size_t keystride, const uint8_t *sig64, uint8_t *ok) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!tlvs || !off || !messagename || !fieldname || !key33 || keystride < 33 || !sig64 || !ok) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
  // check_schnorr_sig serialises the key compressed and drops the parity byte (bitcoin/signature.c:417-422)
  std::vector<u8> xonly(n * 32);
  for (size_t i = 0; i < n; i++) memcpy(&xonly[32 * i], key33 + keystride * i + 1, 32);
  // a few invoices / offers (one per bolt12_check_signature() call, common/bolt12.c:80-92): merkle root and tagged hash on the host --
  // the kernel's own inline functions (bolt12.h) -- and the rows through the one-launch latency path
  if (n <= 256 && small_path(ctx, n) && ctx->keyed_mode <= 0) {
    const bolt12_mids mids = bolt12_make_mids(messagename, fieldname);
    std::vector<u8> msg(32 * n, 0), valid(n);
    for (size_t i = 0; i < n; i++) {
      u8 root[32];
      valid[i] = bolt12_merkle_root(tlvs + off[i], (size_t)(off[i + 1] - off[i]), mids, root);
      if (valid[i]) bolt12_sighash(mids, root, &msg[32 * i]);
    }
    if ((rc = run_small_gated(ctx, MODE_SCHNORR, n, msg.data(), sig64, xonly.data(), 32, 32, valid.data(), ok)) != 1) return rc;
  }
  if ((rc = ensure(ctx, &ctx->in_a, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_b, n * 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->in_c, n * 32)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_malformed, n)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->out, n)) != LAMD_OK) return rc;
  if ((rc = bolt12_hash_device(ctx, n, tlvs, off, messagename, fieldname, nullptr, ctx->in_a.as<u8>(), ctx->g_malformed.as<u8>())) != LAMD_OK) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_b.p, sig64, n * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->in_c.p, xonly.data(), n * 32, hipMemcpyHostToDevice, ctx->stream));
  return run_device_gated(ctx, MODE_SCHNORR, n, 32, 32, ok);   // xonly lives on this frame
}

// ---- signatures from their text: BOLT #11 invoices and signed messages (bolt11.h).  The front-end kernel, the key-parse kernel, the verification
// batch, the recovery batch and the merge are queued on the context's stream without the host waiting in between; both batches run over all
// n rows (k_bolt11_front on how the rows that do not belong to a batch leave it at once).
struct text_cols {
  int8_t *pre, *status;
  u8 *hash, *sig, *sig_ver, *key, *recid_rec, *have_n, *keyok, *ok_ver, *ok_rec, *pub_rec, *node_id;
  u32 *qwords;
};
static size_t text_cols_bytes(size_t n) { return n * (64 + 32 + 64 + 64 + 33 + 33 + 33 + 7) + 64; }
static text_cols text_cols_at(u8 *p, size_t n) {
  text_cols c;
  c.qwords = (u32 *)p; p += 64 * n;     // what k_keys writes next to keyok (16-byte aligned: uint4 stores); never read
  c.hash = p; p += 32 * n;              // 4-byte aligned
  c.sig = p; p += 64 * n;
  c.sig_ver = p; p += 64 * n;
  c.key = p; p += 33 * n;
  c.pub_rec = p; p += 33 * n;
  c.node_id = p; p += 33 * n;
  c.pre = (int8_t *)p; p += n;
  c.status = (int8_t *)p; p += n;
  c.recid_rec = p; p += n;
  c.have_n = p; p += n;
  c.keyok = p; p += n;
  c.ok_ver = p; p += n;
  c.ok_rec = p;
  return c;
}
// ---- the skeleton the three text calls share, in stream order: text_begin (offset checks, workspaces, the strings and their offsets up, timing begun),
// the call's front-end kernel, text_front_done (the front end's time; the key-parse kernel where rows carry keys), the call's batches and its merge kernel,
// text_finish (the merge's time, the results down, the wait, the times read).  What a stage returns other than LAMD_OK the call hands to drain_fail: the
// queued copies read the call's frame.
struct text_in { const uint8_t *strs; const uint64_t *off; };   // n strings back to back, n + 1 offsets
struct text_frame {
  std::vector<u64> rel[2];   // the queued copies read them: they live until the stream has been synchronised
  const u8 *strs = nullptr;  // on the device: the strings of every input, one input behind the other
  const u64 *off[2] = {};    // n + 1 offsets into strs per input
  u8 *scratch = nullptr;     // as many bytes as the strings have, behind them (where asked for)
  u8 *cols = nullptr;        // the per-row columns
};
struct text_out { void *dst; const void *src; size_t bytes; };   // dst == nullptr: the caller did not ask for this result
// strings back to back on the device, offsets relative to the first; `rel` must outlive the copies
static int text_upload(lamd_ctx *ctx, size_t n, const uint8_t *strs, const uint64_t *off, devbuf *d_strs, size_t at, u64 *d_off, std::vector<u64> &rel) {
  const size_t total = (size_t)(off[n] - off[0]);
  rel.resize(n + 1);
  for (size_t i = 0; i <= n; i++) {
    if (off[i] < off[0] || (i && off[i] < off[i - 1])) { ctx->err = "offsets must not decrease"; return LAMD_ERR_ARG; }
    rel[i] = off[i] - off[0] + at;
  }
  if (total) HIPCHK(ctx, hipMemcpyAsync(d_strs->as<u8>() + at, strs + off[0], total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  return LAMD_OK;
}
static int text_begin(lamd_ctx *ctx, size_t n, int n_in, const text_in *in, bool scratch, size_t cols_bytes, text_frame *f) {
  size_t total = 0;
  for (int k = 0; k < n_in; k++) {
    if (in[k].off[n] < in[k].off[0]) { ctx->err = "offsets must not decrease"; return LAMD_ERR_ARG; }
    total += (size_t)(in[k].off[n] - in[k].off[0]);
  }
  int rc;
  if ((rc = ensure(ctx, &ctx->g_msgs, (scratch ? 2 : 1) * total + 64)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->g_off, n_in * (n + 1) * 8)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->text.cols, cols_bytes)) != LAMD_OK) return rc;
  f->strs = ctx->g_msgs.as<const u8>();
  f->scratch = ctx->g_msgs.as<u8>() + total;
  f->cols = ctx->text.cols.as<u8>();
  size_t at = 0;
  for (int k = 0; k < n_in; k++) {
    u64 *d_off = ctx->g_off.as<u64>() + k * (n + 1);
    f->off[k] = d_off;
    if ((rc = text_upload(ctx, n, in[k].strs, in[k].off, &ctx->g_msgs, at, d_off, f->rel[k])) != LAMD_OK) return rc;
    at += (size_t)(in[k].off[n] - in[k].off[0]);
  }
  if (!ctx->timing) return LAMD_OK;
  HIPCHK(ctx, ctx->text.t.create());
  HIPCHK(ctx, ctx->text.t.record(0, ctx->stream));
  return LAMD_OK;
}
// key33 != nullptr: the key-parse kernel for its validity byte alone (its affine words in qwords are not read again): the verification batch parses the keys
// it needs once more, but reports validity only for the rows its early reject lets through, and a bad key counts whatever the signature bytes are
static int text_front_done(lamd_ctx *ctx, size_t n, const u8 *key33, u32 *qwords, u8 *keyok) {
  if (hipGetLastError() != hipSuccess) { ctx->err = "text front end: launch failed"; return LAMD_ERR_HIP; }
  if (ctx->timing) HIPCHK(ctx, ctx->text.t.record(1, ctx->stream));
  return key33 ? launch_key_validity(ctx, ctx->stream, n, key33, qwords, keyok) : LAMD_OK;
}
static int text_finish(lamd_ctx *ctx, std::initializer_list<text_out> outs) {
  if (hipGetLastError() != hipSuccess) { ctx->err = "text merge: launch failed"; return LAMD_ERR_HIP; }
  if (ctx->timing) HIPCHK(ctx, ctx->text.t.record(2, ctx->stream));
  for (const text_out &o : outs)
    if (o.dst) HIPCHK(ctx, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
  const int rc = lamd_synchronize(ctx);
  if (rc != LAMD_OK || !ctx->timing) return rc;
  HIPCHK(ctx, ctx->text.t.read(2, ctx->text.ms));
  return LAMD_OK;
}
extern "C" int lamd_bolt11_check_batch(lamd_ctx *ctx, size_t n, const uint8_t *strs, const uint64_t *off, int8_t *status, uint8_t *node_id33,
                                       uint8_t *hash32, uint8_t *have_n) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!strs || !off || !status || !node_id33) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
  const text_in in{strs, off};
  text_frame f;
  if ((rc = text_begin(ctx, n, 1, &in, false, text_cols_bytes(n), &f)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  const text_cols c = text_cols_at(f.cols, n);
  hipLaunchKernelGGL(k_bolt11_front, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, n, f.strs, f.off[0], c.pre, c.hash, c.sig, c.recid_rec, c.sig_ver,
                     c.key, c.have_n);
  if ((rc = text_front_done(ctx, n, c.key, c.qwords, c.keyok)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  if ((rc = run_device(ctx, MODE_ECDSA, n, c.hash, c.sig_ver, c.key, 33, 33, c.ok_ver)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  if ((rc = recover_device(ctx, n, c.hash, c.sig, c.recid_rec, c.pub_rec, c.ok_rec)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  hipLaunchKernelGGL(k_text_merge, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, n, (const int8_t *)c.pre, c.have_n, (const u8 *)c.keyok, (const u8 *)c.ok_ver,
                     (const u8 *)c.ok_rec, (const u8 *)c.pub_rec, (const u8 *)c.key, c.hash, (int)LAMD_B11_NO_KEY, c.status, c.node_id);
  rc = text_finish(ctx, {{status, c.status, n}, {node_id33, c.node_id, n * 33}, {hash32, c.hash, n * 32}, {have_n, c.have_n, n}});
  return rc == LAMD_OK ? rc : drain_fail(ctx, ctx, rc);
}
extern "C" int lamd_checkmessage_batch(lamd_ctx *ctx, size_t n, const uint8_t *msgs, const uint64_t *moff, const uint8_t *zbase, const uint64_t *zoff,
                                       int8_t *status, uint8_t *node_id33) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!msgs || !moff || !zbase || !zoff || !status || !node_id33) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  const text_in in[2] = {{msgs, moff}, {zbase, zoff}};   // messages | signature strings
  text_frame f;
  if ((rc = text_begin(ctx, n, 2, in, false, text_cols_bytes(n), &f)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  const text_cols c = text_cols_at(f.cols, n);
  hipLaunchKernelGGL(k_checkmessage_front, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, n, f.strs, f.off[0], f.strs, f.off[1], c.pre, c.hash, c.sig,
                     c.recid_rec);
  if ((rc = text_front_done(ctx, n, nullptr, nullptr, nullptr)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  if ((rc = recover_device(ctx, n, c.hash, c.sig, c.recid_rec, c.pub_rec, c.ok_rec)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  hipLaunchKernelGGL(k_text_merge, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, n, (const int8_t *)c.pre, (u8 *)nullptr, (const u8 *)nullptr, (const u8 *)nullptr,
                     (const u8 *)c.ok_rec, (const u8 *)c.pub_rec, (const u8 *)nullptr, c.hash, (int)LAMD_MSG_NO_KEY, c.status, c.node_id);
  rc = text_finish(ctx, {{status, c.status, n}, {node_id33, c.node_id, n * 33}});
  return rc == LAMD_OK ? rc : drain_fail(ctx, ctx, rc);
}

// ---- BOLT #12 offers, invoice requests and invoices from their text (bolt12_text.h): the same skeleton with the BIP-340 batch in place of the ECDSA and
// recovery batches.  The decode scratch lies behind the strings in the same buffer.
struct b12_cols {
  int8_t *pre, *status;
  u8 *hash, *offer_id, *invreq_id, *sig, *xonly, *key, *signer, *kind, *have_key, *keyok, *ok_ver;
  u32 *qwords;
};
static size_t b12_cols_bytes(size_t n) { return n * (64 + 4 * 32 + 64 + 33 + 33 + 6) + 64; }
static b12_cols b12_cols_at(u8 *p, size_t n) {
  b12_cols c;
  c.qwords = (u32 *)p; p += 64 * n;     // what k_keys writes next to keyok (16-byte aligned: uint4 stores); never read
  c.hash = p; p += 32 * n;
  c.xonly = p; p += 32 * n;
  c.sig = p; p += 64 * n;
  c.offer_id = p; p += 32 * n;
  c.invreq_id = p; p += 32 * n;
  c.key = p; p += 33 * n;
  c.signer = p; p += 33 * n;
  c.pre = (int8_t *)p; p += n;
  c.status = (int8_t *)p; p += n;
  c.kind = p; p += n;
  c.have_key = p; p += n;
  c.keyok = p; p += n;
  c.ok_ver = p;
  return c;
}
extern "C" int lamd_bolt12_check_text_batch(lamd_ctx *ctx, size_t n, const uint8_t *strs, const uint64_t *off, int8_t *status, uint8_t *kind,
                                            uint8_t *signer33, uint8_t *sighash32, uint8_t *offer_id32, uint8_t *invreq_id32) {
  if (!ctx) return LAMD_ERR_ARG;
  if (n == 0) return LAMD_OK;
  if (!strs || !off || !status || !kind || !signer33) { ctx->err = "bad argument"; return LAMD_ERR_ARG; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = cache_maybe_reset(ctx)) != LAMD_OK) return rc;
  const text_in in{strs, off};
  text_frame f;
  if ((rc = text_begin(ctx, n, 1, &in, true, b12_cols_bytes(n), &f)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  const b12_cols c = b12_cols_at(f.cols, n);
  bolt12_text_mids mids;
  bolt12_text_make_mids(&mids);
  hipLaunchKernelGGL(k_bolt12_text_front, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, n, f.strs, f.off[0], f.scratch, mids, c.pre, c.kind, c.have_key,
                     c.key, c.xonly, c.sig, c.hash, c.offer_id, c.invreq_id);
  if ((rc = text_front_done(ctx, n, c.key, c.qwords, c.keyok)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  if ((rc = run_device(ctx, MODE_SCHNORR, n, c.hash, c.sig, c.xonly, 32, 32, c.ok_ver)) != LAMD_OK) return drain_fail(ctx, ctx, rc);
  hipLaunchKernelGGL(k_bolt12_text_merge, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, n, (const int8_t *)c.pre, (const u8 *)c.kind, (const u8 *)c.have_key,
                     (const u8 *)c.keyok, (const u8 *)c.ok_ver, (const u8 *)c.key, c.hash, c.offer_id, c.invreq_id, c.status, c.signer);
  rc = text_finish(ctx, {{status, c.status, n}, {kind, c.kind, n}, {signer33, c.signer, n * 33}, {sighash32, c.hash, n * 32}, {offer_id32, c.offer_id, n * 32},
                         {invreq_id32, c.invreq_id, n * 32}});
  return rc == LAMD_OK ? rc : drain_fail(ctx, ctx, rc);
}

// ---- fee grind: see k_grind.  Returns 1 (found; *feerate, *fee set), 0 (no candidate verifies) or an error < 0.
extern "C" int lamd_grind_htlc_tx_fee(lamd_ctx *ctx, const uint8_t *preimage, size_t preimage_len, const uint8_t *outputs,
                                      size_t outputs_len, uint64_t input_sat, uint64_t weight, uint32_t min_feerate,
                                      uint32_t max_feerate, const uint8_t sig64[64], uint8_t sighash_type, int has_witness_script,
                                      const uint8_t pubkey33[33], uint32_t *feerate, uint64_t *fee) {
  if (!ctx) return LAMD_ERR_ARG;
  if (!preimage || !outputs || !sig64 || !pubkey33 || !feerate || !fee || preimage_len < 40 + 4 || outputs_len < 9 ||
      outputs_len > (size_t)GRIND_MAX_OUTPUTS || weight == 0 || weight > ((uint64_t)1 << 31)) {
    ctx->err = "bad argument";
    return LAMD_ERR_ARG;
  }
  // the sighash-type gate of check_tx_sig (bitcoin/signature.c:206-211) is the same for every candidate
  if (!(sighash_type == 1 || (sighash_type == 0x83 && has_witness_script))) return 0;
  if (max_feerate < min_feerate) return 0;
  const size_t ncand = (size_t)max_feerate - min_feerate + 1;
  if (ncand > ((size_t)1 << 30)) {
    ctx->err = "feerate range too large";
    return LAMD_ERR_ARG;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t lead = ((preimage_len - 40) / 64) * 64, tail_len = preimage_len - lead;  // hashOutputs starts in the first tail block
  // staging: preimage | outputs | sig | key | setup | best
  const size_t o_out = (preimage_len + 15) & ~(size_t)15, o_sig = (o_out + outputs_len + 15) & ~(size_t)15, o_key = o_sig + 64,
               o_setup = o_key + 48, o_best = o_setup + ((sizeof(grind_setup) + 15) & ~(size_t)15), total = o_best + 16;
  int rc;
  if ((rc = ensure(ctx, &ctx->g_msgs, total)) != LAMD_OK) return rc;
  if ((rc = ensure(ctx, &ctx->slots, (size_t)SLOT_WORDS * 4)) != LAMD_OK) return rc;
  std::vector<u8> stage(total, 0);
  memcpy(&stage[0], preimage, preimage_len);
  memcpy(&stage[o_out], outputs, outputs_len);
  memcpy(&stage[o_sig], sig64, 64);
  memcpy(&stage[o_key], pubkey33, 33);
  memset(&stage[o_best], 0xFF, 4);
  u8 *d = ctx->g_msgs.as<u8>();
  HIPCHK(ctx, hipMemcpyAsync(d, stage.data(), total, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_grind_setup, dim3(1), dim3(64), 0, ctx->stream, d + o_sig, d + o_key, d, (u32)(lead / 64), ctx->slots.as<u32>(),
                     (const u32 *)ctx->gtable, (grind_setup *)(d + o_setup));
  hipLaunchKernelGGL(k_grind, dim3(blocks_for(ncand)), dim3(256), 0, ctx->stream, (u32)ncand, min_feerate, weight, input_sat, d + lead,
                     (u32)tail_len, (u32)lead, d + o_out, (u32)outputs_len, (const grind_setup *)(d + o_setup), (const u32 *)ctx->gtable,
                     (u32 *)(d + o_best));
  HIPCHK(ctx, hipGetLastError());
  u32 best = 0xFFFFFFFFu;
  HIPCHK(ctx, hipMemcpyAsync(&best, d + o_best, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (best == 0xFFFFFFFFu) return 0;
  *feerate = min_feerate + best;
  *fee = (uint64_t)*feerate * weight / 1000;
  return 1;
}


// Text front ends, one string per lane: what lies between an invoice / a signed-message string and the (hash32, sig64, recid) row that the
// recovery and verification machinery takes (include/lightning_amd.h: lamd_bolt11_check_batch, lamd_checkmessage_batch).  Inline functions
// that compile for gfx950 and, unchanged, for the host (tests/c/bolt11_host.cpp runs them under the sanitizers).
//
//   BOLT #11 (common/bolt11.c:748-1062, common/bech32.c:94-155, common/hash_u5.c): bech32 decoding of the whole string, the walk over the
//   tagged fields, SHA-256 over the lower-cased hrp and the 5-bit values in front of the signature, the 65 signature bytes and the `n` key.
//   checkmessage (lightningd/signmessage.c:36-55, :148-198): zbase32 decoding of the 65 signature bytes and
//   SHA256(SHA256("Lightning Signed Message:" || msg)).
//
// Both are STREAMING: no buffer whose size depends on the string.  Pass 1 of an invoice finds the separator (backwards from the end) and runs
// the checksum and the case test; pass 2 walks the fields and feeds the hash.  The hash takes its input through a bit accumulator (8 bits per
// hrp byte, 5 per data value, 32 per word of the padding) that emits big-endian words into a fixed 16-word block; the block is written with
// compile-time indices only (a select per word), so it stays in registers, and every function below has ONE site where a word enters the
// block -- one unrolled compression in its code, not one per caller (lamd_engine.hip, k_txsig_tx_hash, on what the other form costs).
#pragma once
#include "sha256.h"
#include "../../include/lightning_amd.h"

namespace lamd {

struct text_rev { int8_t v[256]; };
constexpr text_rev text_make_rev(const char *charset, bool fold_case) {
  text_rev t{};
  for (int i = 0; i < 256; i++) t.v[i] = -1;
  for (int i = 0; i < 32; i++) {
    const int c = (unsigned char)charset[i];
    t.v[c] = (int8_t)i;
    if (fold_case && c >= 'a' && c <= 'z') t.v[c - 32] = (int8_t)i;
  }
  return t;
}
// BIP-173's data alphabet (both cases map; bytes with bit 7 set do not) and the zbase32 alphabet (case-sensitive)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ static const text_rev B11_REV = text_make_rev("qpzry9x8gf2tvdw0s3jn54khce6mua7l", true);
__device__ __constant__ static const text_rev ZBASE_REV = text_make_rev("ybndrfg8ejkmcpqxot1uwisza345h769", false);
#else
static constexpr text_rev B11_REV = text_make_rev("qpzry9x8gf2tvdw0s3jn54khce6mua7l", true);
static constexpr text_rev ZBASE_REV = text_make_rev("ybndrfg8ejkmcpqxot1uwisza345h769", false);
#endif

LAMD_HD u32 bech32_polymod_step(u32 pre) {
  const u32 b = pre >> 25;
  return ((pre & 0x1FFFFFFu) << 5) ^ ((b & 1) ? 0x3b6a57b2u : 0) ^ ((b & 2) ? 0x26508e6du : 0) ^ ((b & 4) ? 0x1ea119fau : 0) ^ ((b & 8) ? 0x3d4233ddu : 0) ^
         ((b & 16) ? 0x2a1462b3u : 0);
}

// ---- SHA-256 fed `bits` (1..32) at a time
struct bit_sha {
  u32 st[8];
  u32 w[16];
  u32 nw;      // words in the block
  u32 nbits;   // bits waiting in acc (< 32)
  u64 acc;
  u64 total;   // message bits absorbed
};
LAMD_HD void bit_sha_init(bit_sha *s) {
  const u32 iv[8] = LAMD_SHA256_IV;
#pragma unroll
  for (int i = 0; i < 8; i++) s->st[i] = iv[i];
#pragma unroll
  for (int i = 0; i < 16; i++) s->w[i] = 0;
  s->nw = 0;
  s->nbits = 0;
  s->acc = 0;
  s->total = 0;
}
// the one site (per caller's loop) where a word enters the block
LAMD_HD void bit_sha_push(bit_sha *s, u32 v, u32 bits) {
  s->acc = (s->acc << bits) | v;
  s->nbits += bits;
  if (s->nbits >= 32) {
    s->nbits -= 32;
    const u32 word = (u32)(s->acc >> s->nbits);
#pragma unroll
    for (u32 j = 0; j < 16; j++) s->w[j] = s->nw == j ? word : s->w[j];
    if (++s->nw == 16) {
      sha256_compress(s->st, s->w);
      s->nw = 0;
    }
  }
}
// What follows the message, as a sequence of pushes: step 0 = 0x80, then zero bytes up to the last two words of a block, then the length.
// Returns false when the padding is complete (nothing was pushed).  The message must end on a byte boundary.
LAMD_HD bool bit_sha_pad_next(const bit_sha *s, u32 *step, u32 *v, u32 *bits) {
  if (*step == 0) { *v = 0x80; *bits = 8; *step = 1; return true; }
  if (*step == 1) {
    if (s->nbits != 0 || s->nw != 14) { *v = 0; *bits = 8; return true; }
    *v = (u32)(s->total >> 32); *bits = 32; *step = 2; return true;
  }
  if (*step == 2) { *v = (u32)s->total; *bits = 32; *step = 3; return true; }
  return false;
}
LAMD_HD void bit_sha_digest(const bit_sha *s, u8 out32[32]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out32[4 * i] = (u8)(s->st[i] >> 24); out32[4 * i + 1] = (u8)(s->st[i] >> 16);
    out32[4 * i + 2] = (u8)(s->st[i] >> 8); out32[4 * i + 3] = (u8)s->st[i];
  }
}

// r or s >= n (secp256k1_ecdsa_recoverable_signature_parse_compact's overflow test) on the 64 big-endian bytes
LAMD_HD bool text_bytes_ge_n(const u8 *b32) {
  const u8 nb[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
                     0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};
  int cmp = 0;
  for (int i = 0; i < 32; i++)
    if (cmp == 0) cmp = (int)b32[i] - (int)nb[i];
  return cmp >= 0;
}
LAMD_HD bool text_sig_out_of_range(const u8 *sig64) { return text_bytes_ge_n(sig64) || text_bytes_ge_n(sig64 + 32); }

// ---- BOLT #11.  Returns the status so far -- LAMD_B11_OK, _BAD_BECH32, _BAD_PREFIX, _MALFORMED, _BAD_RECID, _SIG_RANGE -- what can be said
// without curve arithmetic: whether the `n` key is a point (MALFORMED if not), recovery and verification come behind it.
//   hash32   the signed hash (hash_u5 over hrp and data in front of the signature); zero when the status is -1 .. -3
//   sig64    r || s, *recid byte 64 of the signature: zero when the status is -1 .. -3
//   key33    the 33 bytes of the first 53-value `n` field, *have_n = 1; without one, and when the status is -1 .. -3, zero and *have_n = 0
constexpr size_t B11_SIG_VALUES = 104;   // 520 bits
LAMD_HD int bolt11_front_one(const u8 *str, size_t len, u8 hash32[32], u8 sig64[64], u8 *recid, u8 key33[33], u8 *have_n) {
  for (int b = 0; b < 32; b++) hash32[b] = 0;
  for (int b = 0; b < 64; b++) sig64[b] = 0;
  for (int b = 0; b < 33; b++) key33[b] = 0;
  *recid = 0;
  *have_n = 0;
  // -- pass 1: bech32_decode().  The separator is the LAST '1'; the case test covers hrp and data
  if (len < 8) return LAMD_B11_BAD_BECH32;
  size_t ndata = 0;
  while (ndata < len && str[len - 1 - ndata] != '1') ndata++;
  if (1 + ndata >= len || ndata < 6) return LAMD_B11_BAD_BECH32;   // no separator, empty hrp, no room for the checksum
  const size_t hrp_len = len - 1 - ndata;
  u32 chk = 1;
  bool lower = false, upper = false;
  for (size_t i = 0; i < hrp_len; i++) {
    u32 ch = str[i];
    if (ch < 33 || ch > 126) return LAMD_B11_BAD_BECH32;
    if (ch >= 'a' && ch <= 'z') lower = true;
    else if (ch >= 'A' && ch <= 'Z') { upper = true; ch += 32; }
    chk = bech32_polymod_step(chk) ^ (ch >> 5);
  }
  chk = bech32_polymod_step(chk);
  for (size_t i = 0; i < hrp_len; i++) chk = bech32_polymod_step(chk) ^ (str[i] & 0x1fu);
  for (size_t i = hrp_len + 1; i < len; i++) {
    const u32 c = str[i];
    const int v = B11_REV.v[c];   // -1 for every byte with bit 7 set
    if (c >= 'a' && c <= 'z') lower = true;
    if (c >= 'A' && c <= 'Z') upper = true;
    if (v < 0) return LAMD_B11_BAD_BECH32;
    chk = bech32_polymod_step(chk) ^ (u32)v;
  }
  if (lower && upper) return LAMD_B11_BAD_BECH32;
  if (chk != 1) return LAMD_B11_BAD_BECH32;   // bech32m (0x2bc830a3) included
  // -- the prefix: the first two bytes of the hrp, lower-cased, are "ln"
  if (hrp_len < 2 || (str[0] | 0x20) != 'l' || (str[1] | 0x20) != 'n') return LAMD_B11_BAD_PREFIX;
  // -- pass 2.  m values without the checksum: 7 of timestamp, fields, 104 of signature.  Fewer than 111 cannot be framed (the timestamp
  // is cut, or the signature is)
  const size_t m = ndata - 6;
  if (m < 7 + B11_SIG_VALUES) return LAMD_B11_MALFORMED;
  const size_t hashed = m - B11_SIG_VALUES;
  const u8 *data = str + hrp_len + 1;
  bit_sha s;
  bit_sha_init(&s);
  // walk state: what the value at k is
  enum { W_TS, W_TAG, W_LEN_HI, W_LEN_LO, W_BODY };
  u32 what = W_TS, tag = 0, flen = 0;
  size_t left = 7;              // values left of the timestamp / the field's body
  bool in_key = false, found = false, malformed = false;
  u32 kacc = 0, kbits = 0, kbytes = 0;
  size_t pos = 0;               // hrp byte, then data value, being absorbed
  u32 pad_step = 0;
  // phases of the ONE push site: hrp bytes, data values, zero bits up to a byte boundary, the SHA-256 padding
  enum { P_HRP, P_DATA, P_ALIGN, P_PAD, P_DONE };
  u32 phase = P_HRP;
#pragma unroll 1
  while (phase != P_DONE) {
    u32 v = 0, bits = 0;
    bool message = true;   // counts towards the hashed length
    if (phase == P_HRP) {
      u32 ch = str[pos];
      if (ch >= 'A' && ch <= 'Z') ch += 32;
      v = ch;
      bits = 8;
      if (++pos == hrp_len) { phase = P_DATA; pos = 0; }
    } else if (phase == P_DATA) {
      v = (u32)B11_REV.v[data[pos]];
      bits = 5;
      if (what == W_TS) {
        if (--left == 0) what = W_TAG;
      } else if (what == W_TAG) {
        // a field starts here only if more than 104 values remain, and then its three header values are read whatever follows: they must
        // lie in front of the signature for exactly 104 values to remain at the end
        if (hashed - pos < 3) { malformed = true; break; }
        tag = v;
        what = W_LEN_HI;
      } else if (what == W_LEN_HI) {
        flen = v << 5;
        what = W_LEN_LO;
      } else if (what == W_LEN_LO) {
        flen |= v;
        if (flen > hashed - (pos + 1)) { malformed = true; break; }   // longer than what remains, or eating into the signature
        // the first `n` field of the right length is the key; any other is skipped like an unknown field
        in_key = tag == 19 && flen == 53 && !found;
        if (in_key) { found = true; kacc = 0; kbits = 0; kbytes = 0; }
        left = flen;
        what = flen ? W_BODY : W_TAG;
      } else {
        if (in_key) {
          kacc = (kacc << 5) | v;
          kbits += 5;
          if (kbits >= 8 && kbytes < 33) {
            kbits -= 8;
            key33[kbytes++] = (u8)(kacc >> kbits);
          }
        }
        if (--left == 0) {
          if (in_key && (kacc & 1)) { malformed = true; break; }   // 265 bits: the last one must be zero (pull_bits without padding)
          in_key = false;
          what = W_TAG;
        }
      }
      if (++pos == hashed) phase = (s.nbits + 5) & 7 ? P_ALIGN : P_PAD;
    } else if (phase == P_ALIGN) {
      bits = 8 - (s.nbits & 7);   // hash_u5_done: the last byte is padded with zero bits
      phase = P_PAD;
    } else {
      message = false;
      if (!bit_sha_pad_next(&s, &pad_step, &v, &bits)) { phase = P_DONE; break; }
    }
    s.total += message ? bits : 0;
    bit_sha_push(&s, v, bits);
  }
  // the walk ends between two fields (the timestamp's seven values and every header and body lie in front of the signature by the tests above)
  if (malformed || what != W_TAG) {
    for (int b = 0; b < 33; b++) key33[b] = 0;
    return LAMD_B11_MALFORMED;
  }
  // -- the signature: 104 values = 65 bytes
  {
    u32 acc = 0, nb = 0, out = 0;
    for (size_t k = hashed; k < m; k++) {
      acc = (acc << 5) | (u32)B11_REV.v[data[k]];
      nb += 5;
      if (nb >= 8) {
        nb -= 8;
        const u8 byte = (u8)(acc >> nb);
        if (out < 64) sig64[out] = byte;
        else *recid = byte;
        out++;
      }
    }
  }
  bit_sha_digest(&s, hash32);
  *have_n = found;
  if (*recid > 3) return LAMD_B11_BAD_RECID;
  if (text_sig_out_of_range(sig64)) return LAMD_B11_SIG_RANGE;
  return LAMD_B11_OK;
}

// ---- checkmessage.  Returns LAMD_MSG_OK, _BAD_ZBASE, _BAD_LENGTH or _BAD_SIG; recovery comes behind it.
//   hash32   SHA256d("Lightning Signed Message:" || msg) when the status is OK, else zero
//   sig64    bytes 1 .. 64 of the decoded signature, *recid = byte 0 - 31; zero unless the string decodes to 65 bytes
constexpr size_t ZBASE_SIG_CHARS = 104;   // 65 bytes
LAMD_HD int checkmessage_front_one(const u8 *msg, size_t mlen, const u8 *zb, size_t zlen, u8 hash32[32], u8 sig64[64], u8 *recid) {
  for (int b = 0; b < 32; b++) hash32[b] = 0;
  for (int b = 0; b < 64; b++) sig64[b] = 0;
  *recid = 0;
  // from_zbase32(): every character is looked up first, then the bits must come out even (a multiple of 8 characters)
  for (size_t i = 0; i < zlen; i++)
    if (ZBASE_REV.v[zb[i]] < 0) return LAMD_MSG_BAD_ZBASE;
  if (zlen % 8) return LAMD_MSG_BAD_ZBASE;
  if (zlen != ZBASE_SIG_CHARS) return LAMD_MSG_BAD_LENGTH;
  u32 byte0 = 0;
  {
    u32 acc = 0, nb = 0, out = 0;
    for (size_t k = 0; k < ZBASE_SIG_CHARS; k++) {
      acc = (acc << 5) | (u32)ZBASE_REV.v[zb[k]];
      nb += 5;
      if (nb >= 8) {
        nb -= 8;
        const u8 byte = (u8)(acc >> nb);
        if (out == 0) byte0 = byte;
        else sig64[out - 1] = byte;
        out++;
      }
    }
  }
  // The reference hands byte0 - 31 to the library unchecked (the library's ARG_CHECK then calls its illegal-argument callback); here an id
  // outside 0..3 is a bad signature
  *recid = (u8)(byte0 - 31);
  if (byte0 < 31 || byte0 > 34) return LAMD_MSG_BAD_SIG;
  if (text_sig_out_of_range(sig64)) return LAMD_MSG_BAD_SIG;
  const u8 prefix[25] = {'L', 'i', 'g', 'h', 't', 'n', 'i', 'n', 'g', ' ', 'S', 'i', 'g', 'n', 'e', 'd', ' ', 'M', 'e', 's', 's', 'a', 'g', 'e', ':'};
  bit_sha s;
  bit_sha_init(&s);
  // phases of the one push site: the prefix, the message, the padding, then the second hash: the digest's eight words and their padding
  enum { P_PREFIX, P_MSG, P_PAD, P_SECOND, P_DONE };
  u32 phase = P_PREFIX, pad_step = 0, second = 0;
  size_t pos = 0;
  u32 d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  while (phase != P_DONE) {
    u32 v = 0, bits = 8;
    if (phase == P_PREFIX) {
      v = prefix[pos];
      s.total += 8;
      if (++pos == 25) { phase = mlen ? P_MSG : P_PAD; pos = 0; }
    } else if (phase == P_MSG) {
      v = msg[pos];
      s.total += 8;
      if (++pos == mlen) phase = P_PAD;
    } else if (phase == P_PAD) {
      if (!bit_sha_pad_next(&s, &pad_step, &v, &bits)) {
        const u32 iv[8] = LAMD_SHA256_IV;
#pragma unroll
        for (int i = 0; i < 8; i++) { d[i] = s.st[i]; s.st[i] = iv[i]; }
        phase = P_SECOND;
        continue;
      }
    } else {
      bits = 32;
#pragma unroll
      for (u32 j = 0; j < 8; j++) v = second == j ? d[j] : v;
      if (second == 8) v = 0x80000000u;
      if (second == 15) v = 256;
      if (++second == 16) phase = P_DONE;
    }
    bit_sha_push(&s, v, bits);
  }
  bit_sha_digest(&s, hash32);
  return LAMD_MSG_OK;
}

}  // namespace lamd

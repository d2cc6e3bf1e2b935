// BOLT #12 text front end, one string per lane: what lies between an offer / invoice-request / invoice STRING ("lno1...", "lnr1...", "lni1...")
// and the (sighash32, sig64, x-only key) row that the BIP-340 verification takes (include/lightning_amd.h: lamd_bolt12_check_text_batch).  One
// inline function that compiles for gfx950 and, unchanged, for the host (tests/c/bolt12_text_host.cpp runs it under the sanitizers).  Include
// behind verify_core.h (streaming SHA-256, wire_bigsize, bolt12.h) and bolt11.h (text_make_rev / B11_REV).
//
//   b12_string_to_data (common/bolt12.c:112-156): the `+` joins are collapsed and the characters behind the FIRST '1' repacked 5 -> 8 bits
//   (from_bech32_charset + bech32_pull_bits, common/bech32_util.c:34-120; no checksum) in ONE pass over the string, into a span the caller
//   gives: a string of len bytes never decodes to more than 5*len/8 bytes.  Everything behind that reads the DECODED bytes, bounded by their
//   count: the TLV walk (fromwire_tlv's generic rules, wire/tlvstream.c:144-300) that finds the key field, field 240 and the fields outside the
//   kind's ranges, the two ids (calc_offer / calc_invreq, common/bolt12.c:697-756) and merkle_tlv + sighash_from_merkle (bolt12.h).
#pragma once

namespace lamd {

struct bolt12_text_mids {
  u32 leaf[8], branch[8];                 // "LnLeaf", "LnBranch"
  u32 sig_invreq[8], sig_invoice[8];      // "lightning" || "invoice_request" | "invoice" || "signature": a lane picks one by its kind
};
// what the host computes once per call
inline void bolt12_text_make_mids(bolt12_text_mids *m) {
  const u8 leaf[6] = {'L', 'n', 'L', 'e', 'a', 'f'}, branch[8] = {'L', 'n', 'B', 'r', 'a', 'n', 'c', 'h'};
  bolt12_tag_midstate(leaf, 6, leaf, 0, m->leaf);
  bolt12_tag_midstate(branch, 8, branch, 0, m->branch);
  bolt12_tag_midstate((const u8 *)"lightning", 9, (const u8 *)"invoice_requestsignature", 24, m->sig_invreq);
  bolt12_tag_midstate((const u8 *)"lightning", 9, (const u8 *)"invoicesignature", 16, m->sig_invoice);
}

LAMD_HD bool b12_in(u64 t, u64 lo, u64 hi) { return t >= lo && t <= hi; }

// SHA-256 over tlv_span(lo1, hi1) || tlv_span(lo2, hi2) (common/bolt12.c:670-695) of a stream that obeys the TLV rules: types ascend, so each
// span is the run of fields whose type lies inside its bounds, and hi1 < lo2 puts the first run in front of the second.  A span without a
// field is empty (also where the reference would subtract from a null pointer); two empty spans give SHA-256 of nothing.
LAMD_HD void b12_span_hash(const u8 *tlv, size_t dlen, u64 lo1, u64 hi1, u64 lo2, u64 hi2, u8 out32[32]) {
  sha_stream s;
  shs_init(&s);
  size_t pos = 0;
  while (pos < dlen) {
    const size_t start = pos;
    u64 type = 0, length = 0;
    size_t l = wire_bigsize(tlv + pos, dlen - pos, &type);
    if (!l) break;
    pos += l;
    l = wire_bigsize(tlv + pos, dlen - pos, &length);
    if (!l) break;
    pos += l;
    if (length > dlen - pos) break;
    pos += (size_t)length;
    if (b12_in(type, lo1, hi1) || b12_in(type, lo2, hi2)) shs_update(&s, tlv + start, pos - start);
  }
  shs_final(&s, out32);
}

// Returns the status so far -- LAMD_B12_OK, _UNFINISHED, _BAD_BECH32, _BAD_PREFIX, _MALFORMED, _OUT_OF_RANGE, _NO_KEY, _NO_SIGNATURE -- what can
// be said without curve arithmetic: whether the key is a point (MALFORMED if not, ahead of -5 .. -7) and the verification come behind it.
//   out, cap     the decode span; *dlen = the decoded bytes in it (0 for statuses -1 and -2).  cap >= 5*len/8 always suffices
//   *kind        LAMD_B12_KIND_*; NONE for statuses -1 .. -3
//   key33        the kind's key field (88 / 176), *have_key = 1, where the field is present with 33 bytes and the status is not -1 .. -4; else zero
//   sig64        field 240, sighash32 = sighash_from_merkle(): status OK and kind invreq / invoice; else zero
//   offer_id32   status OK; invreq_id32: status OK and kind invreq / invoice; else zero
LAMD_HD int bolt12_text_front_one(const u8 *str, size_t len, u8 *out, size_t cap, size_t *dlen, const bolt12_text_mids &mids, u8 *kind, u8 key33[33],
                                  u8 *have_key, u8 sig64[64], u8 sighash32[32], u8 offer_id32[32], u8 invreq_id32[32]) {
  for (int b = 0; b < 33; b++) key33[b] = 0;
  for (int b = 0; b < 64; b++) sig64[b] = 0;
  for (int b = 0; b < 32; b++) sighash32[b] = offer_id32[b] = invreq_id32[b] = 0;
  *kind = LAMD_B12_KIND_NONE;
  *have_key = 0;
  *dlen = 0;
  // -- one pass: collapse the joins, split at the first '1', repack.  A fault is remembered, not returned: "unfinished" is known only at the end
  bool have_plus = false, sep = false, bad = false, lower = false, upper = false, hrp_cut = false;
  u32 hrp_n = 0;          // hrp bytes in front of its first NUL byte (the reference keeps the hrp as a C string)
  u8 h[3] = {0, 0, 0};    // the first three of them, lower-cased
  u32 acc = 0, nb = 0;
  size_t n_out = 0;
#pragma unroll 1
  for (size_t i = 0; i < len; i++) {
    const u32 c = str[i];
    if (i != 0 && i + 1 != len && !have_plus && c == '+') { have_plus = true; continue; }
    if (have_plus && (c == ' ' || (c >= 9 && c <= 13))) continue;   // ccan's cisspace: space, \t \n \v \f \r
    have_plus = false;
    if (!sep) {
      if (c == '1') { sep = true; continue; }
      if (c == 0) hrp_cut = true;
      if (hrp_cut) continue;
      u32 lc = c;
      if (c >= 'A' && c <= 'Z') { upper = true; lc = c + 32; }
      else if (c >= 'a' && c <= 'z') lower = true;
      if (hrp_n < 3) h[hrp_n] = (u8)lc;
      hrp_n++;
      continue;
    }
    const int v = B11_REV.v[c];   // both cases map; -1 for every byte with bit 7 set
    if (c >= 'A' && c <= 'Z') upper = true;
    if (c >= 'a' && c <= 'z') lower = true;
    if (v < 0) bad = true;
    if (bad) continue;
    acc = ((acc << 5) | (u32)v) & 0xFFFu;
    nb += 5;
    if (nb >= 8) {
      nb -= 8;
      if (n_out < cap) out[n_out] = (u8)(acc >> nb);
      else bad = true;   // cannot happen with cap >= 5*len/8
      n_out++;
    }
  }
  if (have_plus) return LAMD_B12_UNFINISHED;
  // nb = 5*count mod 8: five or more spare bits are a superfluous character, and the spare bits must be zero
  if (!sep || bad || (lower && upper) || nb >= 5 || (acc & ((1u << nb) - 1u))) return LAMD_B12_BAD_BECH32;
  if (hrp_n != 3 || h[0] != 'l' || h[1] != 'n' || (h[2] != 'o' && h[2] != 'r' && h[2] != 'i')) return LAMD_B12_BAD_PREFIX;
  const u32 k = h[2] == 'o' ? LAMD_B12_KIND_OFFER : h[2] == 'r' ? LAMD_B12_KIND_INVREQ : LAMD_B12_KIND_INVOICE;
  *kind = (u8)k;
  *dlen = n_out;
  // -- the TLV walk over out[0 .. n_out)
  const u64 key_type = k == LAMD_B12_KIND_INVREQ ? 88 : 176;
  bool oor = false, found_key = false, found_sig = false;
  size_t key_at = 0, sig_at = 0;
  {
    bool first = true;
    u64 prev = 0;
    size_t pos = 0;
#pragma unroll 1
    while (pos < n_out) {
      u64 type = 0, length = 0;
      size_t l = wire_bigsize(out + pos, n_out - pos, &type);
      if (!l) return LAMD_B12_MALFORMED;
      pos += l;
      if (!first && type <= prev) return LAMD_B12_MALFORMED;
      first = false;
      prev = type;
      l = wire_bigsize(out + pos, n_out - pos, &length);
      if (!l) return LAMD_B12_MALFORMED;
      pos += l;
      if (length > n_out - pos) return LAMD_B12_MALFORMED;
      if (k == LAMD_B12_KIND_OFFER) {
        if (!b12_in(type, 1, 79) && !b12_in(type, 1000000000ull, 1999999999ull)) oor = true;
      } else {
        if (type == key_type) {
          if (length != 33) return LAMD_B12_MALFORMED;
          found_key = true;
          key_at = pos;
        }
        if (type == 240) {
          if (length != 64) return LAMD_B12_MALFORMED;
          found_sig = true;
          sig_at = pos;
        }
        if (k == LAMD_B12_KIND_INVREQ && !b12_in(type, 240, 1000) && !b12_in(type, 0, 159) && !b12_in(type, 1000000000ull, 2999999999ull)) oor = true;
      }
      pos += (size_t)length;
    }
  }
  if (found_key) {
    for (int b = 0; b < 33; b++) key33[b] = out[key_at + b];
    *have_key = 1;
  }
  if (oor) return LAMD_B12_OUT_OF_RANGE;
  if (k != LAMD_B12_KIND_OFFER) {
    if (!found_key) return LAMD_B12_NO_KEY;
    if (!found_sig) return LAMD_B12_NO_SIGNATURE;
  }
  b12_span_hash(out, n_out, 1, 79, 1000000000ull, 1999999999ull, offer_id32);
  if (k == LAMD_B12_KIND_OFFER) return LAMD_B12_OK;
  b12_span_hash(out, n_out, 0, 159, 1000000000ull, 2999999999ull, invreq_id32);
  for (int b = 0; b < 64; b++) sig64[b] = out[sig_at + b];
  bolt12_mids m;
  for (int j = 0; j < 8; j++) {
    m.leaf[j] = mids.leaf[j];
    m.branch[j] = mids.branch[j];
    m.sig[j] = k == LAMD_B12_KIND_INVREQ ? mids.sig_invreq[j] : mids.sig_invoice[j];
  }
  u8 root[32];
  // the stream obeys the TLV rules and the key field is a leaf, so a root exists
  if (!bolt12_merkle_root(out, n_out, m, root)) return LAMD_B12_MALFORMED;
  bolt12_sighash(m, root, sighash32);
  return LAMD_B12_OK;
}

}  // namespace lamd

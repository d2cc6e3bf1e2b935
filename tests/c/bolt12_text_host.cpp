// Host build of lightning_amd/csrc/bolt12_text.h under AddressSanitizer / UBSan (tests/test_bolt12_text_host.py): the per-string function the kernel
// k_bolt12_text_front runs, over a file of strings.
//   bolt12_text_host IN OUT   IN: u32 count, then per row u32 length + the string (lengths little-endian).  OUT, per row: status so far (int8) |
//                             kind | have_key | key33 | sig64 | sighash32 | offer_id32 | invreq_id32  (196 bytes)
// Every buffer handed to the function is a heap block of EXACTLY its size -- the string, the decode scratch of 5*len/8 bytes, and each output
// column of the row -- so a read or write one byte outside is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "verify_core.h"
#include "bolt11.h"
#include "bolt12_text.h"

using namespace lamd;

static std::vector<u8> read_file(const char *path) {
  std::vector<u8> v;
  FILE *f = fopen(path, "rb");
  if (!f) { printf("cannot read %s\n", path); exit(2); }
  u8 buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
static u32 u32le(const std::vector<u8> &v, size_t *at) {
  if (v.size() - *at < 4) { printf("input cut off\n"); exit(2); }
  u32 x;
  memcpy(&x, &v[*at], 4);
  *at += 4;
  return x;
}

int main(int argc, char **argv) {
  if (argc != 3) { printf("usage: bolt12_text_host IN OUT\n"); return 2; }
  const std::vector<u8> in = read_file(argv[1]);
  size_t at = 0;
  const u32 n = u32le(in, &at);
  bolt12_text_mids mids;
  bolt12_text_make_mids(&mids);
  std::vector<u8> out;
  for (u32 i = 0; i < n; i++) {
    const u32 len = u32le(in, &at);
    if (in.size() - at < len) { printf("input cut off\n"); return 2; }
    u8 *s = (u8 *)malloc(len);
    if (len) memcpy(s, &in[at], len);
    at += len;
    const size_t cap = (size_t)5 * len / 8;
    u8 *scratch = (u8 *)malloc(cap);
    u8 *kind = (u8 *)malloc(1), *have_key = (u8 *)malloc(1), *key = (u8 *)malloc(33), *sig = (u8 *)malloc(64), *sighash = (u8 *)malloc(32),
       *offer_id = (u8 *)malloc(32), *invreq_id = (u8 *)malloc(32);
    size_t dlen = 0;
    const int st = bolt12_text_front_one(s, len, scratch, cap, &dlen, mids, kind, key, have_key, sig, sighash, offer_id, invreq_id);
    if (dlen > cap) { printf("row %u: %zu decoded bytes in a span of %zu\n", i, dlen, cap); return 1; }
    out.push_back((u8)(int8_t)st);
    out.push_back(*kind);
    out.push_back(*have_key);
    out.insert(out.end(), key, key + 33);
    out.insert(out.end(), sig, sig + 64);
    out.insert(out.end(), sighash, sighash + 32);
    out.insert(out.end(), offer_id, offer_id + 32);
    out.insert(out.end(), invreq_id, invreq_id + 32);
    free(s); free(scratch); free(kind); free(have_key); free(key); free(sig); free(sighash); free(offer_id); free(invreq_id);
  }
  FILE *f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("cannot write %s\n", argv[2]); return 2; }
  fclose(f);
  printf("ok\n");
  return 0;
}

// Host build of lightning_amd/csrc/bolt11.h under AddressSanitizer / UBSan (tests/test_bolt11_host.py): the per-string functions the kernels
// k_bolt11_front and k_checkmessage_front run, over a file of strings.
//   bolt11_host bolt11 IN OUT   IN: u32 count, then per row u32 length + the string.  OUT, per row: status so far (int8) | hash32 | sig64 |
//                               recid | key33 | have_n  (132 bytes)
//   bolt11_host msg IN OUT      IN: u32 count, then per row u32 length + message, u32 length + zbase string.  OUT, per row: status so far
//                               (int8) | hash32 | sig64 | recid  (98 bytes)
// (lengths little-endian).  Every buffer handed to the functions is a heap block of EXACTLY its size -- the string, and each output column of
// the row -- so a read or write one byte outside is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bolt11.h"

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
struct reader {
  const std::vector<u8> &v;
  size_t at = 0;
  u32 u32le() {
    if (v.size() - at < 4) { printf("input cut off\n"); exit(2); }
    u32 x;
    memcpy(&x, &v[at], 4);
    at += 4;
    return x;
  }
  // an exact-size heap copy of the next `len` bytes
  u8 *block(size_t len) {
    if (v.size() - at < len) { printf("input cut off\n"); exit(2); }
    u8 *p = (u8 *)malloc(len ? len : 1);
    if (len) memcpy(p, &v[at], len);
    else { free(p); p = (u8 *)malloc(0); }
    at += len;
    return p;
  }
};

int main(int argc, char **argv) {
  if (argc != 4 || (strcmp(argv[1], "bolt11") && strcmp(argv[1], "msg"))) { printf("usage: bolt11_host bolt11|msg IN OUT\n"); return 2; }
  const bool msg_mode = !strcmp(argv[1], "msg");
  const std::vector<u8> in = read_file(argv[2]);
  reader r{in};
  const u32 n = r.u32le();
  std::vector<u8> out;
  for (u32 i = 0; i < n; i++) {
    u8 *hash = (u8 *)malloc(32), *sig = (u8 *)malloc(64), *recid = (u8 *)malloc(1), *key = (u8 *)malloc(33), *have_n = (u8 *)malloc(1);
    int st;
    if (msg_mode) {
      const u32 mlen = r.u32le();
      u8 *m = r.block(mlen);
      const u32 zlen = r.u32le();
      u8 *z = r.block(zlen);
      st = checkmessage_front_one(m, mlen, z, zlen, hash, sig, recid);
      free(m);
      free(z);
    } else {
      const u32 len = r.u32le();
      u8 *s = r.block(len);
      st = bolt11_front_one(s, len, hash, sig, recid, key, have_n);
      free(s);
    }
    out.push_back((u8)(int8_t)st);
    out.insert(out.end(), hash, hash + 32);
    out.insert(out.end(), sig, sig + 64);
    out.push_back(*recid);
    if (!msg_mode) {
      out.insert(out.end(), key, key + 33);
      out.push_back(*have_n);
    }
    free(hash); free(sig); free(recid); free(key); free(have_n);
  }
  FILE *f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("cannot write %s\n", argv[3]); return 2; }
  fclose(f);
  printf("ok\n");
  return 0;
}

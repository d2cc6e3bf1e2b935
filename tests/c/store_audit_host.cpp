// Host build of lightning_amd/csrc/store_audit.h under AddressSanitizer / UBSan (tests/test_store_audit_host.py):
//  - store_crc32c<4> / <8> against the bitwise definition of CRC-32C for every length 0..70 at every start alignment 0..7, and for one
//    65 535-byte buffer;
//  - the scid index: lowest record wins, the key that looks like an empty slot, colliding keys;
//  - store_walk on truncated, zero-filled and garbage-length files.  Every buffer handed to the walk is a heap block of EXACTLY len bytes,
//    so a read past the end is an ASan report.
// With three arguments, IMAGE SIGV OUT, it runs none of those: it audits the store file IMAGE with the signature verdicts handed in and writes
// offsets, verdicts, signers and the walk's summary to OUT.* for the test to compare with the sequential model (audit_file below).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "store_audit.h"

using namespace lamd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static u32 crc_bitwise(u32 seed, const u8 *p, size_t len) {
  u32 c = ~seed;
  for (size_t i = 0; i < len; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
  }
  return ~c;
}
static u64 rnd_state = 0x1234567ull;
static u32 rnd() {
  rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
  return (u32)(rnd_state >> 33);
}

static void put_hdr(std::vector<u8> &f, u32 flags, u32 len, u32 crc, u32 ts) {
  const u32 w[3] = {(flags << 16) | len, crc, ts};
  for (u32 x : w)
    for (int s = 24; s >= 0; s -= 8) f.push_back((u8)(x >> s));
}
static void put_rec(std::vector<u8> &f, u32 flags, u32 ts, const std::vector<u8> &msg) {
  put_hdr(f, flags, (u32)msg.size(), crc_bitwise(ts, msg.data(), msg.size()), ts);
  f.insert(f.end(), msg.begin(), msg.end());
}
struct walked { lamd_store_summary s; std::vector<u64> off; bool ok; };
// the walk over an exact-size heap copy of f[0, len)
static walked walk(const std::vector<u8> &f, size_t len) {
  u8 *buf = (u8 *)malloc(len ? len : 1);
  if (len) memcpy(buf, f.data(), len);
  walked w;
  w.ok = store_walk(buf, len, &w.s, [&](size_t i, u64 off, const store_hdr &h, u32 type) {
    CHECK(i == w.off.size());
    CHECK(off + STORE_HDR + h.len <= len);
    CHECK(!(h.flags & STORE_FLAG_DELETED) || type == 0);
    w.off.push_back(off);
  });
  free(buf);
  return w;
}

static std::vector<u8> read_file(const char *path) {
  std::vector<u8> out;
  FILE *f = fopen(path, "rb");
  if (!f) { printf("cannot read %s\n", path); exit(2); }
  u8 tmp[4096];
  for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) out.insert(out.end(), tmp, tmp + k);
  fclose(f);
  return out;
}
static void write_file(const std::string &path, const void *p, size_t len) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, len, f) != len) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

// IMAGE SIGV OUT: the audit of a store file with the signature verdicts handed in (SIGV: one int8 per record, what the signature batch says
// of it; read for live records of type 256 / 257 / 258 only).  The walk, both CRC widths, the scid index filled in file order and in reverse,
// the signer look-up and the merge -> OUT.off (u64 per record), OUT.verdict (int8), OUT.signer (33 bytes per record), OUT.walk (5 x u64:
// records, live, deleted, end_offset, end_reason).
static int audit_file(const char *image, const char *sigv_path, const std::string &base, const u32 *T4, const u32 *T8) {
  const std::vector<u8> file = read_file(image), sigv = read_file(sigv_path);
  const size_t len = file.size();
  u8 *buf = (u8 *)malloc(len ? len : 1);   // exactly the file: a read past it is an ASan report
  if (len) memcpy(buf, file.data(), len);
  lamd_store_summary s;
  std::vector<u64> off;
  std::vector<u32> type;
  if (!store_walk(buf, len, &s, [&](size_t, u64 o, const store_hdr &, u32 t) { off.push_back(o); type.push_back(t); })) { printf("not a store\n"); return 1; }
  const size_t n = off.size();
  CHECK(sigv.size() == n && s.records == n);
  u32 bits = 1;
  while (((size_t)1 << bits) < 2 * n + 2) bits++;
  const size_t cap = (size_t)1 << bits;
  std::vector<u64> keys(cap + 1, STORE_EMPTY_KEY), rkeys(cap + 1, STORE_EMPTY_KEY);
  std::vector<u32> vals(cap + 1, STORE_NONE), rvals(cap + 1, STORE_NONE);
  for (size_t i = 0; i < n; i++) {
    store_index_one(buf, len, off[i], (u32)i, keys.data(), vals.data(), bits);
    store_index_one(buf, len, off[n - 1 - i], (u32)(n - 1 - i), rkeys.data(), rvals.data(), bits);
  }
  std::vector<int8_t> verdict(n);
  std::vector<u8> signer(33 * n + 1);
  for (size_t i = 0; i < n; i++) {
    const int pre = store_precheck_one<4>(T4, buf, len, off[i]);
    CHECK(pre == store_precheck_one<8>(T8, buf, len, off[i]));
    u8 rid[33];
    const u32 aux = store_signer_one(buf, len, off.data(), (u32)i, keys.data(), vals.data(), bits, &signer[33 * i]);
    CHECK(aux == store_signer_one(buf, len, off.data(), (u32)i, rkeys.data(), rvals.data(), bits, rid) && !memcmp(rid, &signer[33 * i], 33));
    const bool has_sig = type[i] == STORE_T_CANN || type[i] == STORE_T_NANN || type[i] == STORE_T_CUPD;
    verdict[i] = (int8_t)store_merge_one(pre, has_sig, (int8_t)sigv[i], aux);
  }
  free(buf);
  const u64 w[5] = {s.records, s.live, s.deleted, s.end_offset, (u64)s.end_reason};
  write_file(base + ".off", off.data(), 8 * n);
  write_file(base + ".verdict", verdict.data(), n);
  write_file(base + ".signer", signer.data(), 33 * n);
  write_file(base + ".walk", w, sizeof w);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

int main(int argc, char **argv) {
  static u32 T4[4 * 256], T8[8 * 256];
  store_crc_build_tables(T4, 4);
  store_crc_build_tables(T8, 8);
  if (argc == 4) return audit_file(argv[1], argv[2], argv[3], T4, T8);
  CHECK(T4[1] == 0xF26B8303u);                                                  // the first entry of every published CRC-32C table
  {
    const u8 *digits = (const u8 *)"123456789";
    CHECK(crc_bitwise(0, digits, 9) == 0xE3069283u);                             // the check value of CRC-32C
    CHECK(store_crc32c<4>(T4, 0, digits, 9) == 0xE3069283u && store_crc32c<8>(T8, 0, digits, 9) == 0xE3069283u);
  }
  // every length 0..70 at every alignment 0..7: exact-size heap blocks, so the 32-bit loads may not run over the end
  for (size_t len = 0; len <= 70; len++)
    for (size_t al = 0; al < 8; al++) {
      u8 *exact = (u8 *)malloc(al + len ? al + len : 1);   // (malloc aligns to 16: `al` is the start alignment)
      for (size_t i = 0; i < al + len; i++) exact[i] = (u8)rnd();
      const u32 seed = rnd(), want = crc_bitwise(seed, exact + al, len);
      CHECK(store_crc32c<4>(T4, seed, exact + al, len) == want);
      CHECK(store_crc32c<8>(T8, seed, exact + al, len) == want);
      free(exact);
    }
  {
    std::vector<u8> big(65535 + 3);
    for (auto &b : big) b = (u8)rnd();
    for (size_t al = 0; al < 3; al += 2) {
      const u32 want = crc_bitwise(0xDEADBEEFu, big.data() + al, 65535);
      CHECK(store_crc32c<4>(T4, 0xDEADBEEFu, big.data() + al, 65535) == want);
      CHECK(store_crc32c<8>(T8, 0xDEADBEEFu, big.data() + al, 65535) == want);
    }
  }
  // the scid index
  {
    const u32 bits = 3, cap = 8;
    std::vector<u64> keys(cap + 1, STORE_EMPTY_KEY);
    std::vector<u32> vals(cap + 1, STORE_NONE);
    store_index_insert(keys.data(), vals.data(), bits, 42, 9);
    store_index_insert(keys.data(), vals.data(), bits, 42, 5);
    store_index_insert(keys.data(), vals.data(), bits, 42, 7);
    store_index_insert(keys.data(), vals.data(), bits, STORE_EMPTY_KEY, 11);
    store_index_insert(keys.data(), vals.data(), bits, 0, 3);
    for (u64 k = 100; k < 102; k++) store_index_insert(keys.data(), vals.data(), bits, k << 40, (u32)k);
    CHECK(store_index_find(keys.data(), vals.data(), bits, 42) == 5);
    CHECK(store_index_find(keys.data(), vals.data(), bits, STORE_EMPTY_KEY) == 11);
    CHECK(store_index_find(keys.data(), vals.data(), bits, 0) == 3);
    CHECK(store_index_find(keys.data(), vals.data(), bits, (u64)101 << 40) == 101);
    CHECK(store_index_find(keys.data(), vals.data(), bits, 43) == STORE_NONE);
  }
  // ---- the walk
  std::vector<u8> uuid(34, 7), amount(10, 0), cann(430, 1), cupd(138, 2);
  uuid[0] = 0x10; uuid[1] = 0x0B;       // 4107
  amount[0] = 0x10; amount[1] = 0x05;   // 4101
  cann[0] = 1; cann[1] = 0;             // 256
  cupd[0] = 1; cupd[1] = 2;             // 258
  std::vector<u8> f = {0x10};
  put_rec(f, 0x2000, 0, uuid);
  put_rec(f, 0x2000, 5, cann);
  put_rec(f, 0x2000, 0, amount);
  put_rec(f, 0xA000, 6, cupd);          // deleted
  put_rec(f, 0x2800, 7, cupd);          // dying flag
  {
    walked w = walk(f, f.size());
    CHECK(w.ok && w.s.records == 5 && w.s.live == 4 && w.s.deleted == 1 && w.s.end_reason == LAMD_STORE_END_EOF && w.s.end_offset == f.size() && w.s.version == 16);
    CHECK(w.off.size() == 5 && w.off[0] == 1 && w.off[1] == 1 + 12 + 34);
  }
  // every prefix of the file: the walk stays inside it and ends on a record boundary
  for (size_t len = 0; len <= f.size(); len++) {
    walked w = walk(f, len);
    CHECK(w.ok == (len >= 1));
    if (!w.ok) continue;
    CHECK(w.s.end_offset <= len && w.s.records == w.off.size());
    CHECK((w.s.end_reason == LAMD_STORE_END_EOF) == (w.s.end_offset == len));
  }
  {   // the announcement is not read before its amount record has room
    const size_t cut = 1 + 12 + 34 + 12 + 430 + 21;
    walked w = walk(f, cut);
    CHECK(w.s.records == 1 && w.s.end_reason == LAMD_STORE_END_NO_AMOUNT && w.s.end_offset == 1 + 12 + 34);
    w = walk(f, cut + 1);
    CHECK(w.s.records == 3 && w.s.end_reason == LAMD_STORE_END_EOF);
  }
  {   // zero fill behind good records: no COMPLETED flag
    std::vector<u8> z = f;
    z.resize(z.size() + 100, 0);
    walked w = walk(z, z.size());
    CHECK(w.s.records == 5 && w.s.end_reason == LAMD_STORE_END_INCOMPLETE && w.s.end_offset == f.size());
    std::vector<u8> allz(64, 0);
    w = walk(allz, 64);
    CHECK(w.ok && w.s.records == 0 && w.s.end_reason == LAMD_STORE_END_INCOMPLETE && w.s.end_offset == 1);
  }
  {   // a length that points past the end, live and deleted; a live record of one byte; store_ended; major version 1
    std::vector<u8> g = f;
    put_hdr(g, 0x2000, 0xFFFF, 0, 0);
    g.resize(g.size() + 40, 3);
    walked w = walk(g, g.size());
    CHECK(w.s.records == 5 && w.s.end_reason == LAMD_STORE_END_TRUNCATED && w.s.end_offset == f.size());
    g[f.size()] = 0xA0;
    w = walk(g, g.size());
    CHECK(w.s.records == 5 && w.s.end_reason == LAMD_STORE_END_TRUNCATED);
    std::vector<u8> h = f;
    put_hdr(h, 0x2000, 1, 0, 0);
    h.push_back(9);
    w = walk(h, h.size());
    CHECK(w.s.records == 5 && w.s.end_reason == LAMD_STORE_END_SHORT && w.s.end_offset == f.size());
    h[f.size()] = 0xA0;                  // deleted: skipped whatever its length
    w = walk(h, h.size());
    CHECK(w.s.records == 6 && w.s.deleted == 2 && w.s.end_reason == LAMD_STORE_END_EOF);
    std::vector<u8> e = f, ended(10, 0);
    ended[0] = 0x10; ended[1] = 0x09;    // 4105
    put_rec(e, 0x2000, 0, ended);
    put_rec(e, 0x2000, 0, uuid);
    w = walk(e, e.size());
    CHECK(w.s.records == 6 && w.s.end_reason == LAMD_STORE_END_STORE_ENDED && w.s.end_offset == f.size() + 22);
    std::vector<u8> v = f;
    v[0] = 0x2F;
    CHECK(!walk(v, v.size()).ok);
    v[0] = 0x0F;
    CHECK(walk(v, v.size()).ok);
  }
  // garbage: random bytes with the COMPLETED bit forced on now and then, random lengths
  for (int round = 0; round < 2000; round++) {
    const size_t len = 1 + rnd() % 300;
    std::vector<u8> g(len);
    for (auto &b : g) b = (u8)rnd();
    g[0] &= 0x1F;
    for (size_t p = 1; p + 4 <= len; p += 1 + rnd() % 40) { g[p] |= 0x20; g[p + 2] = 0; g[p + 3] = (u8)(rnd() % 60); }
    walked w = walk(g, len);
    CHECK(w.ok && w.s.end_offset <= len && w.s.live + w.s.deleted == w.s.records);
  }
  // the device-side readers on an image that is not the one the walk saw: offsets and lengths are checked against the image's size
  {
    u8 *buf = (u8 *)malloc(f.size());
    memcpy(buf, f.data(), f.size());
    CHECK(store_precheck_one<4>(T4, buf, f.size(), 1) == LAMD_STORE_OK);
    CHECK(store_precheck_one<8>(T8, buf, f.size(), 1 + 12 + 34) == LAMD_STORE_OK);
    CHECK(store_precheck_one<4>(T4, buf, f.size(), f.size() - 5) == LAMD_STORE_BAD_CHECKSUM);
    CHECK(store_precheck_one<4>(T4, buf, f.size() - 1, f.size() - 150) == LAMD_STORE_BAD_CHECKSUM);
    CHECK(store_precheck_one<4>(T4, buf, f.size(), f.size() + 100) == LAMD_STORE_BAD_CHECKSUM);
    buf[1 + 12 + 20] ^= 1;
    CHECK(store_precheck_one<4>(T4, buf, f.size(), 1) == LAMD_STORE_BAD_CHECKSUM);
    u32 len;
    CHECK(store_live_msg(buf, f.size(), f.size() - 5, &len) == nullptr);
    free(buf);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

// Host build of lightning_amd/csrc/store_repair.h under AddressSanitizer / UBSan (tests/test_store_repair_host.py).
// Without arguments, the program's own checks:
//  - the node table: lowest record wins, equal ids at different image offsets share a slot, a full table drops instead of looping;
//  - store_pack_gather at every source alignment, 1..4 bytes, at both ends of an exact-size heap block;
//  - the whole repair of a hand-built store into exact-size output blocks at every output alignment 0..3 and with a short capacity, the copy
//    through the whole arrays and through staged windows of 1, 7 and 2048 output words.
// With arguments IMAGE VERDICTS UUID OUT: the repair of the image file with the verdict bytes of VERDICTS (one per record of the walk) and
// the 32-byte uuid file, on the host with the functions the kernels run; OUT.reason, OUT.new_off (u64 little-endian) and OUT.image are
// written for the caller to compare with its model.  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "store_repair.h"

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
static u64 rnd_state = 0x7654321ull;
static u32 rnd() {
  rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
  return (u32)(rnd_state >> 33);
}
static void put_rec(std::vector<u8> &f, u32 flags, u32 ts, const std::vector<u8> &msg) {
  const u32 w[3] = {(flags << 16) | (u32)msg.size(), crc_bitwise(ts, msg.data(), msg.size()), ts};
  for (u32 x : w)
    for (int s = 24; s >= 0; s -= 8) f.push_back((u8)(x >> s));
  f.insert(f.end(), msg.begin(), msg.end());
}

struct repaired {
  std::vector<u64> rec_off, new_off;
  std::vector<u8> reason, image;   // image: what was written, at most `cap` bytes
  u64 out_len = 0;
};
// The repair as lamd_gossip_store_repair runs it, stage by stage, on exact-size heap copies; the output block starts `mis` bytes behind a
// 4-aligned address and has `cap` bytes.
static repaired repair(const std::vector<u8> &file, const std::vector<int8_t> &verdict, const u8 *uuid32, u32 mis, u64 cap) {
  repaired R;
  const size_t len = file.size();
  u8 *store = (u8 *)malloc(len);
  memcpy(store, file.data(), len);
  lamd_store_summary s;
  size_t n_cann = 0;
  CHECK(store_walk(store, len, &s, [&](size_t, u64 off, const store_hdr &, u32 type) { R.rec_off.push_back(off); n_cann += type == STORE_T_CANN; }));
  const u32 n = (u32)R.rec_off.size();
  if (verdict.size() != n) { printf("%zu verdicts for %u records\n", verdict.size(), n); exit(2); }
  u32 bits = 1, nbits = 1;
  while (((size_t)1 << bits) < 2 * n_cann) bits++;
  while (((size_t)1 << nbits) < 4 * n_cann) nbits++;
  std::vector<u64> keys(((size_t)1 << bits) + 1, STORE_EMPTY_KEY), nkeys((size_t)1 << nbits, STORE_NODE_EMPTY), pos(n + 1);
  std::vector<u32> vals(((size_t)1 << bits) + 1, STORE_NONE), nvals((size_t)1 << nbits, STORE_NONE), size(n + 1, 0);
  R.reason.assign(n, 0xEE);
  const u64 *off = R.rec_off.data();
  for (u32 i = 0; i < n; i++) store_index_one(store, len, off[i], i, keys.data(), vals.data(), bits);
  for (u32 i = 0; i < n; i++) {   // k_store_keep_chan
    if (!store_is_live_cann(store, len, off[i])) continue;
    u64 idoff = 0;
    R.reason[i] = (u8)store_keep_cann(store, len, off, verdict.data(), n, i, &size[i], &idoff);
    if (R.reason[i] == STORE_DROP_KEPT) {
      store_node_insert(store, nkeys.data(), nvals.data(), nbits, idoff, i);
      store_node_insert(store, nkeys.data(), nvals.data(), nbits, idoff + 33, i);
    }
  }
  for (u32 i = n; i-- > 0;)   // k_store_keep_rest, in the order least like the file's: no record's rule may lean on a neighbour's turn
    if (!store_is_live_cann(store, len, off[i]))
      R.reason[i] = (u8)store_keep_other(store, len, off, verdict.data(), n, i, keys.data(), vals.data(), bits, nkeys.data(), nvals.data(), nbits,
                                         R.reason.data(), &size[i]);
  u64 sum = 0;
  for (u32 i = 0; i <= n; i++) { pos[i] = sum; sum += size[i]; }
  R.new_off.resize(n);
  for (u32 i = 0; i < n; i++) R.new_off[i] = R.reason[i] == STORE_DROP_KEPT ? STORE_REPAIR_HEAD + pos[i] : ~(u64)0;
  R.out_len = STORE_REPAIR_HEAD + sum;
  const store_head head = store_make_head(store[0], uuid32);
  const u64 lim = cap < R.out_len ? cap : R.out_len;
  u8 *block = (u8 *)malloc((size_t)(mis + lim) ? (size_t)(mis + lim) : 1);   // (malloc aligns to 16)
  u8 *out = block + mis;
  const store_pack_global whole{off, pos.data()};
  for (u64 k = 0; 4 * k < mis + lim; k++) store_pack_word(store, len, whole, 0, n ? n - 1 : 0, head, out, lim, mis, k);
  R.image.assign(out, out + lim);
  // ... and through staged windows, as a block of k_store_pack takes them: `words` words each, the window found by two searches in the whole scan
  for (u64 words : {(u64)1, (u64)7, (u64)2048}) {
    memset(block, 0xEE, (size_t)(mis + lim));
    for (u64 k0 = 0; 4 * k0 < mis + lim; k0 += words) {
      const u64 k1 = k0 + words, bf = 4 * k0 > mis ? 4 * k0 - mis : 0, bl = 4 * k1 - mis < lim ? 4 * k1 - mis : lim;
      u32 lo = 0, hi = 0;
      if (bl > STORE_REPAIR_HEAD) {
        lo = store_pack_locate(whole, 0, n - 1, bf > STORE_REPAIR_HEAD ? bf - STORE_REPAIR_HEAD : 0);
        hi = store_pack_locate(whole, 0, n - 1, bl - STORE_REPAIR_HEAD - 1);
      }
      std::vector<u32> rel(hi - lo + 2);   // exact sizes: a read outside the window is an ASan report
      std::vector<u64> roff(hi - lo + 1);
      for (u32 j = 0; j < rel.size() && lo + j <= n; j++) rel[j] = (u32)(pos[lo + j] - pos[lo]);
      for (u32 j = 0; j < roff.size() && lo + j < n; j++) roff[j] = off[lo + j];
      const store_pack_staged window{roff.data(), rel.data(), lo, pos[lo]};
      for (u64 k = k0; k < k1 && 4 * k < mis + lim; k++) store_pack_word(store, len, window, lo, hi, head, out, lim, mis, k);
    }
    CHECK(lim == 0 || memcmp(out, R.image.data(), (size_t)lim) == 0);
  }
  free(block);
  free(store);
  return R;
}

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
static void write_file(const std::string &path, const void *p, size_t len) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, len, f) != len) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

// a channel_announcement of 430 bytes: no features, scid, the two node ids filled with `a` and `b`
static std::vector<u8> make_cann(u64 scid, u8 a, u8 b) {
  std::vector<u8> m(430, 0x55);
  m[0] = 1; m[1] = 0; m[258] = 0; m[259] = 0;
  for (int i = 0; i < 8; i++) m[292 + i] = (u8)(scid >> (56 - 8 * i));
  memset(&m[300], a, 33);
  memset(&m[333], b, 33);
  return m;
}
static std::vector<u8> make_nann(u8 id, size_t tail) {
  std::vector<u8> m(2 + 64 + 2 + 4 + 33 + tail, 0x44);
  m[0] = 1; m[1] = 1; m[66] = 0; m[67] = 0;
  memset(&m[72], id, 33);
  return m;
}
static std::vector<u8> make_scid_msg(u32 type, size_t len, size_t at, u64 scid) {
  std::vector<u8> m(len, 0x33);
  m[0] = (u8)(type >> 8); m[1] = (u8)type;
  for (int i = 0; i < 8; i++) m[at + i] = (u8)(scid >> (56 - 8 * i));
  return m;
}

int main(int argc, char **argv) {
  if (argc == 5) {
    const std::vector<u8> file = read_file(argv[1]), vb = read_file(argv[2]), uuid = read_file(argv[3]);
    if (uuid.size() != 32) { printf("the uuid file has %zu bytes\n", uuid.size()); return 2; }
    const std::vector<int8_t> verdict(vb.begin(), vb.end());
    const repaired R = repair(file, verdict, uuid.data(), 0, ~(u64)0);
    const repaired S = repair(file, verdict, uuid.data(), 3, ~(u64)0);
    CHECK(S.image == R.image && R.image.size() == R.out_len);
    const std::string base = argv[4];
    write_file(base + ".reason", R.reason.data(), R.reason.size());
    write_file(base + ".new_off", R.new_off.data(), 8 * R.new_off.size());
    write_file(base + ".image", R.image.data(), R.image.size());
    if (failures) return 1;
    printf("ok\n");
    return 0;
  }
  // ---- the node table
  {
    std::vector<u8> img(33 * 6);
    const u8 fill[6] = {0, 1, 2, 3, 1, 0};   // ids 4 and 5 equal ids 1 and 0, at other offsets
    for (int k = 0; k < 6; k++) memset(&img[33 * k], fill[k], 33);
    const u32 bits = 3;
    std::vector<u64> keys(8, STORE_NODE_EMPTY);
    std::vector<u32> vals(8, STORE_NONE);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 1, 9);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 4, 5);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 1, 7);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 0, 12);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 5, 11);
    store_node_insert(img.data(), keys.data(), vals.data(), bits, 33 * 2, 3);
    CHECK(store_node_find(img.data(), keys.data(), vals.data(), bits, &img[33 * 1]) == 5);
    CHECK(store_node_find(img.data(), keys.data(), vals.data(), bits, &img[33 * 4]) == 5);
    CHECK(store_node_find(img.data(), keys.data(), vals.data(), bits, &img[33 * 0]) == 11);
    CHECK(store_node_find(img.data(), keys.data(), vals.data(), bits, &img[33 * 2]) == 3);
    CHECK(store_node_find(img.data(), keys.data(), vals.data(), bits, &img[33 * 3]) == STORE_NONE);
    int used = 0;
    for (u64 k : keys) used += k != STORE_NODE_EMPTY;
    CHECK(used == 3);
    // a table with no free slot: the insert gives up, the look-up ends
    std::vector<u8> many(33 * 5);
    for (size_t i = 0; i < many.size(); i++) many[i] = (u8)rnd();
    std::vector<u64> k2(4, STORE_NODE_EMPTY);
    std::vector<u32> v2(4, STORE_NONE);
    for (u32 k = 0; k < 5; k++) store_node_insert(many.data(), k2.data(), v2.data(), 2, 33 * k, k);
    for (u32 k = 0; k < 4; k++) CHECK(store_node_find(many.data(), k2.data(), v2.data(), 2, &many[33 * k]) == k);
    CHECK(store_node_find(many.data(), k2.data(), v2.data(), 2, &many[33 * 4]) == STORE_NONE);
  }
  // ---- the gather: every offset of a block of exactly 23 bytes at every base alignment, 1..4 bytes
  for (size_t al = 0; al < 4; al++) {
    const size_t len = 23;
    u8 *block = (u8 *)malloc(al + len), *p = block + al;
    for (size_t i = 0; i < al + len; i++) block[i] = (u8)rnd();
    for (size_t s = 0; s < len; s++)
      for (u32 c = 1; c <= 4 && s + c <= len; c++) {
        u32 want = 0;
        for (u32 b = 0; b < c; b++) want |= (u32)p[s + b] << (8 * b);
        CHECK(store_pack_gather(p, len, s, c) == want);
      }
    free(block);
  }
  // ---- the uuid record
  u8 uuid[32];
  for (auto &b : uuid) b = (u8)rnd();
  {
    const store_head h = store_make_head(0x0D, uuid);
    CHECK(h.b[0] == 0x0D && h.b[1] == 0x20 && h.b[2] == 0 && h.b[3] == 0 && h.b[4] == 34 && h.b[13] == 0x10 && h.b[14] == 0x0B);
    CHECK(memcmp(&h.b[15], uuid, 32) == 0 && h.b[9] == 0 && h.b[10] == 0 && h.b[11] == 0 && h.b[12] == 0);
    const u32 crc = crc_bitwise(0, &h.b[13], 34);
    CHECK(h.b[5] == (u8)(crc >> 24) && h.b[6] == (u8)(crc >> 16) && h.b[7] == (u8)(crc >> 8) && h.b[8] == (u8)crc);
  }
  // ---- a hand-built store, every rule once; the expected reason stands next to each record
  std::vector<u8> f = {0x10};
  std::vector<int8_t> v;
  std::vector<u8> want;
  std::vector<u8> amount(10, 0);
  amount[0] = 0x10; amount[1] = 0x05;
  auto add = [&](u32 flags, const std::vector<u8> &m, int verdict, u8 reason) { put_rec(f, flags, rnd(), m); v.push_back((int8_t)verdict); want.push_back(reason); };
  std::vector<u8> olduuid(34, 9);
  olduuid[0] = 0x10; olduuid[1] = 0x0B;
  add(0x2000, olduuid, 0, 4);                                  // 0  the old uuid record
  add(0x2000, make_nann(0xA1, 5), 0, 3);                       // 1  a node_announcement in front of its channel
  add(0x2000, make_cann(100, 0xA1, 0xA2), 0, 0);               // 2  kept
  add(0x2000, amount, 0, 0);                                   // 3
  add(0x2000, make_scid_msg(258, 138, 98, 100), 0, 0);         // 4  its update
  add(0x2800, make_scid_msg(258, 137, 98, 100), 0, 0);         // 5  ... with the DYING flag, and an odd length
  add(0x2000, make_nann(0xA2, 0), 0, 0);                       // 6  node_id_2 of record 2
  add(0x2000, make_nann(0xA3, 1), 0, 3);                       // 7  a node of no channel
  add(0x2000, make_scid_msg(4106, 14, 2, 100), 0, 0);          // 8  chan_dying
  add(0x2000, make_scid_msg(4106, 15, 2, 100), 0, 2);          // 9  ... of the wrong length
  add(0x2000, make_scid_msg(4106, 14, 2, 101), 0, 3);          // 10 ... of an unknown channel
  add(0xA000, make_scid_msg(258, 138, 98, 100), 8, 1);         // 11 deleted
  add(0x2000, make_cann(200, 0xB1, 0xB2), 0, 3);               // 12 its amount record has a bad checksum
  add(0x2000, amount, -2, 2);                                  // 13
  add(0x2000, make_scid_msg(258, 138, 98, 200), 0, 3);         // 14 an update of channel 200
  add(0x2000, make_nann(0xB1, 2), 0, 3);                       // 15 a node of channel 200 only
  add(0x2000, make_cann(300, 0xA1, 0xC2), 2, 2);               // 16 a bad signature
  add(0x2000, amount, 0, 3);                                   // 17
  add(0x2000, make_nann(0xC2, 3), 0, 3);                       // 18
  add(0x2000, make_scid_msg(4103, 10, 2, 100), 0, 4);          // 19 a tombstone
  add(0x2000, amount, 0, 3);                                   // 20 a stray amount record
  add(0x2000, make_cann(400, 0xD1, 0xD2), 0, 3);               // 21 followed by something else
  add(0x2000, make_scid_msg(258, 138, 98, 400), -3, 3);        // 22 the audit found no channel: a dependency
  add(0x2000, make_cann(100, 0xE1, 0xE2), -5, 2);              // 23 a second announcement of channel 100
  add(0x2000, amount, 0, 3);                                   // 24
  add(0x2000, make_nann(0xE1, 4), 0, 3);                       // 25
  add(0x2000, make_scid_msg(258, 138, 98, 100), 1, 2);         // 26 a bad signature
  add(0x2000, make_cann(500, 0xA3, 0xA1), 0, 0);               // 27 kept: node A3 is known from here on
  add(0x2000, amount, 0, 0);                                   // 28
  add(0x2000, make_nann(0xA3, 301), 0, 0);                     // 29
  add(0x2000, make_cann(600, 0xF1, 0xF2), 0, 3);               // 30 the last record: no amount record behind it can be kept
  add(0x2000, amount, 8, 1);                                   // 31 (deleted; its flags say live: the verdict alone decides nothing)
  f[f.size() - 22] |= 0x80;                                    // ... so set the flag too
  {
    const repaired R = repair(f, v, uuid, 0, ~(u64)0);
    CHECK(R.reason == want);
    const store_head h = store_make_head(0x10, uuid);
    std::vector<u8> img(h.b, h.b + STORE_REPAIR_HEAD);
    for (size_t i = 0; i < want.size(); i++) {
      const u64 end = i + 1 < want.size() ? R.rec_off[i + 1] : f.size();
      CHECK(R.new_off[i] == (want[i] ? ~(u64)0 : (u64)img.size()));
      if (!want[i]) img.insert(img.end(), f.begin() + R.rec_off[i], f.begin() + end);
    }
    CHECK(R.out_len == img.size() && R.image == img);
    CHECK(img.size() <= f.size() + 46);
    for (u32 mis = 0; mis < 4; mis++)
      for (u64 cap : {(u64)0, (u64)1, (u64)46, (u64)47, (u64)48, (u64)49, (u64)50, (u64)51, (u64)img.size() - 1, (u64)img.size(), (u64)img.size() + 5}) {
        const repaired S = repair(f, v, uuid, mis, cap);
        const size_t w = cap < img.size() ? (size_t)cap : img.size();
        CHECK(S.out_len == img.size() && S.image.size() == w && (w == 0 || memcmp(S.image.data(), img.data(), w) == 0));
      }
    // nothing kept; no record at all
    std::vector<int8_t> bad(v.size(), -2);
    const repaired N = repair(f, bad, uuid, 1, ~(u64)0);
    CHECK(N.out_len == STORE_REPAIR_HEAD && N.image.size() == STORE_REPAIR_HEAD && memcmp(N.image.data(), img.data(), STORE_REPAIR_HEAD) == 0);
    const repaired E = repair(std::vector<u8>{0x10}, std::vector<int8_t>(), uuid, 2, ~(u64)0);
    CHECK(E.out_len == STORE_REPAIR_HEAD && E.image == N.image && E.reason.empty());
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

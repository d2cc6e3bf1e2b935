// Host build of lightning_amd/csrc/store_latest.h under AddressSanitizer / UBSan (tests/test_store_latest_host.py).
// Without arguments, the program's own checks:
//  - the slot keys: higher timestamp wins, among equal ones the lower record index, whatever the order of arrival; the empty slot; the
//    timestamps 0 and 0xFFFFFFFF; the highest record index there is;
//  - the 64-bit comparisons of the future and the stale rule: at now < prune_interval, around 2^32, at the largest clock;
//  - the signed timestamp of both message kinds at their shortest lengths;
//  - a node table without a free slot: the slot look-up ends;
//  - the whole latest-wins repair of a hand-built store, every new reason once, stage by stage on exact-size heap blocks, stage 1, 3 and 4
//    in file order, in reverse and in a scrambled order: the result may not depend on the order in which the lanes arrive.
// With arguments IMAGE VERDICTS UUID POLICY OUT: the repair of the image file with the verdict bytes of VERDICTS (one per record of the
// walk), the 32-byte uuid file and the 16-byte policy file (u64 now | u32 future_slack | u32 prune_interval, little-endian), on the host
// with the functions the kernels run; OUT.reason, OUT.new_off (u64 little-endian) and OUT.image are written for the caller to compare
// with its model.  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "store_latest.h"

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
static void put_rec(std::vector<u8> &f, u32 flags, u32 ts, const std::vector<u8> &msg) {
  const u32 w[3] = {(flags << 16) | (u32)msg.size(), crc_bitwise(ts, msg.data(), msg.size()), ts};
  for (u32 x : w)
    for (int s = 24; s >= 0; s -= 8) f.push_back((u8)(x >> s));
  f.insert(f.end(), msg.begin(), msg.end());
}

struct repaired {
  std::vector<u64> rec_off, new_off;
  std::vector<u8> reason, image;
  u64 out_len = 0;
};
// the order in which a stage visits the records: 0 file order, 1 reverse, 2 scrambled
static std::vector<u32> visit_order(u32 n, int how) {
  std::vector<u32> o(n);
  for (u32 i = 0; i < n; i++) o[i] = how == 1 ? n - 1 - i : i;
  if (how == 2)
    for (u32 i = n; i > 1; i--) { const u32 j = rnd() % i, t = o[i - 1]; o[i - 1] = o[j]; o[j] = t; }
  return o;
}
// The repair as lamd_gossip_store_repair_latest runs it, stage by stage, on exact-size heap copies.
static repaired repair(const std::vector<u8> &file, const std::vector<int8_t> &verdict, const u8 *uuid32, const lamd_store_latest_policy &pol, int how) {
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
  std::vector<u64> keys(((size_t)1 << bits) + 1, STORE_EMPTY_KEY), nkeys((size_t)1 << nbits, STORE_NODE_EMPTY), pos(n + 1), latest(2 * (size_t)n, 0),
      nlatest((size_t)1 << nbits, 0);
  std::vector<u32> vals(((size_t)1 << bits) + 1, STORE_NONE), nvals((size_t)1 << nbits, STORE_NONE), size(n + 1, 0);
  std::vector<u8> dying(n, 0);
  R.reason.assign(n, 0xEE);
  const u64 *off = R.rec_off.data();
  const int8_t *v = verdict.data();
  for (u32 i = 0; i < n; i++) store_index_one(store, len, off[i], i, keys.data(), vals.data(), bits);
  for (u32 i : visit_order(n, how))   // k_store_latest_upd
    store_latest_upd_one(store, len, off, v, i, keys.data(), vals.data(), bits, pol, latest.data(), dying.data());
  for (u32 i : visit_order(n, how)) {   // k_store_latest_chan
    if (!store_is_live_cann(store, len, off[i])) continue;
    u64 idoff = 0;
    R.reason[i] = (u8)store_latest_cann_one(store, len, off, v, n, i, pol, latest.data(), dying.data(), &size[i], &idoff);
    if (R.reason[i] == STORE_DROP_KEPT) {
      store_node_insert(store, nkeys.data(), nvals.data(), nbits, idoff, i);
      store_node_insert(store, nkeys.data(), nvals.data(), nbits, idoff + 33, i);
    }
  }
  for (u32 i : visit_order(n, how))   // k_store_latest_node
    store_latest_node_one(store, len, off, v, i, nkeys.data(), nvals.data(), nbits, pol, nlatest.data());
  for (u32 i : visit_order(n, how))   // k_store_latest_rest
    if (!store_is_live_cann(store, len, off[i]))
      R.reason[i] = (u8)store_latest_other_one(store, len, off, v, n, i, keys.data(), vals.data(), bits, nkeys.data(), nvals.data(), nbits, R.reason.data(), pol,
                                               latest.data(), nlatest.data(), &size[i]);
  u64 sum = 0;
  for (u32 i = 0; i <= n; i++) { pos[i] = sum; sum += size[i]; }
  R.new_off.resize(n);
  for (u32 i = 0; i < n; i++) R.new_off[i] = R.reason[i] == STORE_DROP_KEPT ? STORE_REPAIR_HEAD + pos[i] : ~(u64)0;
  R.out_len = STORE_REPAIR_HEAD + sum;
  const store_head head = store_make_head(store[0], uuid32);
  u8 *out = (u8 *)malloc((size_t)R.out_len);
  const store_pack_global whole{off, pos.data()};
  for (u64 k = 0; 4 * k < R.out_len; k++) store_pack_word(store, len, whole, 0, n ? n - 1 : 0, head, out, R.out_len, 0, k);
  R.image.assign(out, out + R.out_len);
  free(out);
  free(store);
  return R;
}
// ... in all three orders, which must agree
static repaired repair_any_order(const std::vector<u8> &file, const std::vector<int8_t> &verdict, const u8 *uuid32, const lamd_store_latest_policy &pol) {
  const repaired R = repair(file, verdict, uuid32, pol, 0);
  for (int how : {1, 2, 2}) {
    const repaired S = repair(file, verdict, uuid32, pol, how);
    CHECK(S.reason == R.reason && S.new_off == R.new_off && S.image == R.image && S.out_len == R.out_len);
  }
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
static void put_be32(u8 *p, u32 x) { for (int i = 0; i < 4; i++) p[i] = (u8)(x >> (24 - 8 * i)); }
static std::vector<u8> make_nann(u8 id, u32 ts, size_t tail) {
  std::vector<u8> m(2 + 64 + 2 + 4 + 33 + tail, 0x44);
  m[0] = 1; m[1] = 1; m[66] = 0; m[67] = 0;
  put_be32(&m[68], ts);
  memset(&m[72], id, 33);
  return m;
}
static std::vector<u8> make_cupd(u64 scid, u32 dir, u32 ts, size_t len = 138) {
  std::vector<u8> m(len, 0x33);
  m[0] = 1; m[1] = 2;
  for (int i = 0; i < 8; i++) m[98 + i] = (u8)(scid >> (56 - 8 * i));
  put_be32(&m[106], ts);
  m[111] = (u8)dir;
  return m;
}
static std::vector<u8> make_dying(u64 scid, size_t len = 14) {
  std::vector<u8> m(len, 0x22);
  m[0] = 0x10; m[1] = 0x0A;
  for (int i = 0; i < 8; i++) m[2 + i] = (u8)(scid >> (56 - 8 * i));
  return m;
}

int main(int argc, char **argv) {
  if (argc == 6) {
    const std::vector<u8> file = read_file(argv[1]), vb = read_file(argv[2]), uuid = read_file(argv[3]), pb = read_file(argv[4]);
    if (uuid.size() != 32 || pb.size() != 16) { printf("the uuid file has %zu bytes, the policy file %zu\n", uuid.size(), pb.size()); return 2; }
    lamd_store_latest_policy pol;
    memcpy(&pol.now, &pb[0], 8);
    memcpy(&pol.future_slack, &pb[8], 4);
    memcpy(&pol.prune_interval, &pb[12], 4);
    const repaired R = repair_any_order(file, std::vector<int8_t>(vb.begin(), vb.end()), uuid.data(), pol);
    CHECK(R.image.size() == R.out_len);
    const std::string base = argv[5];
    write_file(base + ".reason", R.reason.data(), R.reason.size());
    write_file(base + ".new_off", R.new_off.data(), 8 * R.new_off.size());
    write_file(base + ".image", R.image.data(), R.image.size());
    if (failures) return 1;
    printf("ok\n");
    return 0;
  }
  // ---- the keys
  {
    CHECK(store_latest_key(0, 0) == 0xFFFFFFFFull && store_latest_key(0, STORE_NONE - 1) == 1);   // never the empty slot's 0
    CHECK(store_latest_key(0xFFFFFFFFu, 0) == ~(u64)0 && store_latest_ts(store_latest_key(0xFFFFFFFFu, 7)) == 0xFFFFFFFFu);
    CHECK(store_latest_key(5, 9) > store_latest_key(4, 0) && store_latest_key(5, 3) > store_latest_key(5, 4) && store_latest_key(1, STORE_NONE - 1) > store_latest_key(0, 0));
    struct { u32 ts, rec; } in[6] = {{7, 10}, {9, 30}, {9, 20}, {0, 1}, {9, 25}, {8, 2}};
    for (int how = 0; how < 12; how++) {
      u64 *slot = (u64 *)malloc(8);
      *slot = 0;
      for (u32 k : visit_order(6, how < 2 ? how : 2)) store_latest_put(slot, store_latest_key(in[k].ts, in[k].rec));
      CHECK(*slot == store_latest_key(9, 20));
      free(slot);
    }
    u64 one = 0;
    store_latest_put(&one, store_latest_key(0, 5));      // timestamp 0 takes the empty slot
    CHECK(one == store_latest_key(0, 5));
    store_latest_put(&one, store_latest_key(0, 6));
    CHECK(one == store_latest_key(0, 5));
    store_latest_put(&one, store_latest_key(0xFFFFFFFFu, 6));
    store_latest_put(&one, store_latest_key(0xFFFFFFFFu, 8));
    CHECK(one == store_latest_key(0xFFFFFFFFu, 6));
  }
  // ---- the two clock rules, in 64 bits
  {
    const lamd_store_latest_policy off{0, 0, 1209600}, small{1000, 86400, 1209600}, big{((u64)1 << 32) + 10, 20, 100}, top{~(u64)0, 0xFFFFFFFFu, 0xFFFFFFFFu},
        edge{0xFFFFFFF0ull, 0x20, 0xFFFFFFFFu};
    CHECK(store_ts_eligible(5, 5, off) && !store_ts_eligible(4, 5, off) && store_ts_eligible(0xFFFFFFFFu, 0xFFFFFFFFu, off));
    CHECK(store_ts_eligible(87400, 87400, small) && !store_ts_eligible(87401, 87401, small) && store_ts_eligible(0, 0, small));
    CHECK(store_ts_eligible(0xFFFFFFFFu, 0xFFFFFFFFu, big) && store_ts_eligible(0xFFFFFFFFu, 0xFFFFFFFFu, top));
    CHECK(store_ts_eligible(0xFFFFFFFFu, 0xFFFFFFFFu, edge));                          // now + slack = 2^32 + 0x10: no 32-bit wrap
    const lamd_store_latest_policy edge2{0xFFFFFFF0ull, 0x0E, 0};
    CHECK(!store_ts_eligible(0xFFFFFFFFu, 0xFFFFFFFFu, edge2) && store_ts_eligible(0xFFFFFFFEu, 0xFFFFFFFEu, edge2));
    // stale: ts + interval < now.  now < interval: nothing is stale (no wrap below 0)
    CHECK(!store_ts_stale(store_latest_key(0, 3), small) && !store_ts_stale(0, big) && !store_ts_stale(store_latest_key(0, 3), off));
    CHECK(store_ts_stale(store_latest_key(0xFFFFFFFFu - 100, 3), big));               // 2^32 - 1 < 2^32 + 10
    CHECK(!store_ts_stale(store_latest_key(0xFFFFFFFFu - 89, 3), big) && store_ts_stale(store_latest_key(0xFFFFFFFFu - 90, 3), big));   // the boundary: ts == now - interval stays
    CHECK(store_ts_stale(store_latest_key(0xFFFFFFFFu, 3), top) && !store_ts_stale(store_latest_key(0xFFFFFFFFu, 3), lamd_store_latest_policy{0x1FFFFFFFEull, 0, 0xFFFFFFFFu}));
    CHECK(!store_ts_stale(store_latest_key(1, 3), lamd_store_latest_policy{5000, 0, 0}));   // no interval
  }
  // ---- the signed timestamp at the shortest lengths, on exact-size blocks
  {
    u32 type, ts, idoff;
    for (size_t len : {(size_t)111, (size_t)112}) {
      std::vector<u8> m = make_cupd(1, 1, 0xA1B2C3D4u, 112);
      m.resize(len);
      u8 *p = (u8 *)malloc(len);
      memcpy(p, m.data(), len);
      CHECK(store_signed_ts(p, (u32)len, &type, &ts, &idoff) == (len == 112));
      if (len == 112) CHECK(type == STORE_T_CUPD && ts == 0xA1B2C3D4u && idoff == 98);
      free(p);
    }
    for (size_t cut : {(size_t)0, (size_t)1, (size_t)40}) {
      std::vector<u8> m = make_nann(0x77, 0x01020304u, 0);
      m.resize(m.size() - cut);
      u8 *p = (u8 *)malloc(m.size());
      memcpy(p, m.data(), m.size());
      CHECK(store_signed_ts(p, (u32)m.size(), &type, &ts, &idoff) == (cut == 0));
      if (cut == 0) CHECK(type == STORE_T_NANN && ts == 0x01020304u && idoff == 72 && p[idoff] == 0x77);
      free(p);
    }
    const u8 other[2] = {0x10, 0x05};
    CHECK(!store_signed_ts(other, 2, &type, &ts, &idoff) && !store_signed_ts(other, 1, &type, &ts, &idoff));
  }
  // ---- a node table with no free slot: the slot look-up finds what is there and ends for what is not
  {
    std::vector<u8> many(33 * 5);
    for (size_t i = 0; i < many.size(); i++) many[i] = (u8)rnd();
    std::vector<u64> k2(4, STORE_NODE_EMPTY);
    std::vector<u32> v2(4, STORE_NONE);
    for (u32 k = 0; k < 5; k++) store_node_insert(many.data(), k2.data(), v2.data(), 2, 33 * k, k);
    bool seen[4] = {};
    for (u32 k = 0; k < 4; k++) {
      const u32 s = store_node_slot(many.data(), k2.data(), 2, &many[33 * k]);
      CHECK(s < 4 && !seen[s] && v2[s] == k && store_node_find(many.data(), k2.data(), v2.data(), 2, &many[33 * k]) == k);
      if (s < 4) seen[s] = true;
    }
    CHECK(store_node_slot(many.data(), k2.data(), 2, &many[33 * 4]) == STORE_NONE);
  }
  // ---- a hand-built store, every new rule once; the expected reason stands next to each record.  N = the clock, P = the prune interval
  u8 uuid[32];
  for (auto &b : uuid) b = (u8)rnd();
  const u32 N = 1700000000u, P = 1209600u, S = 86400u;
  const lamd_store_latest_policy pol{N, S, P};
  std::vector<u8> f = {0x10};
  std::vector<int8_t> v;
  std::vector<u8> want;
  std::vector<u8> amount(10, 0);
  amount[0] = 0x10; amount[1] = 0x05;
  auto add = [&](u32 hdr_ts, const std::vector<u8> &m, int verdict, u8 reason) { put_rec(f, 0x2000, hdr_ts, m); v.push_back((int8_t)verdict); want.push_back(reason); };
  add(N - 9, make_cupd(100, 0, N - 9), -3, 3);                 // 0  in front of its announcement: never supersedes record 3
  add(0, make_cann(100, 0xA1, 0xA2), 0, 0);                    // 1  channel 100, fresh
  add(0, amount, 0, 0);                                        // 2
  add(N - 10, make_cupd(100, 0, N - 10), 0, 5);                // 3  superseded by 5
  add(N - 20, make_cupd(100, 1, N - 20), 0, 5);                // 4  the other direction, its own slot: superseded by 9
  add(N - 5, make_cupd(100, 0, N - 5), 0, 0);                  // 5  the winner
  add(N - 5, make_cupd(100, 0, N - 5), 0, 5);                  // 6  the same timestamp later in the file
  add(N - 1, make_cupd(100, 0, N - 1), 1, 2);                  // 7  a bad signature never wins
  add(N - 7, make_cupd(100, 0, N - 2), 0, 6);                  // 8  header timestamp differs from the signed one
  add(N + S, make_cupd(100, 1, N + S), 0, 0);                  // 9  as far ahead as allowed: wins direction 1 ...
  add(N + S + 1, make_cupd(100, 1, N + S + 1), 0, 6);          // 10 one second further
  add(N - 30, make_nann(0xA1, N - 30, 3), 0, 5);               // 11 node A1: superseded by 13
  add(N - 30, make_nann(0xA2, N - 30, 0), 0, 0);               // 12 node A2: its only one
  add(N - 3, make_nann(0xA1, N - 3, 1), 0, 0);                 // 13
  add(N - 4, make_nann(0xA1, N - 3, 2), 0, 6);                 // 14 header differs
  add(N - 2, make_nann(0xA1, N - 2, 2), 4, 2);                 // 15 a bad signature never wins
  add(0, make_cann(200, 0xA2, 0xB2), 0, 7);                    // 16 channel 200: direction 1 silent for P + 1 seconds
  add(0, amount, 0, 3);                                        // 17
  add(N, make_cupd(200, 0, N), 0, 3);                          // 18
  add(N - P - 1, make_cupd(200, 1, N - P - 1), 0, 3);          // 19
  add(N - 8, make_cupd(200, 1, N - 9), 0, 6);                  // 20 ... a fresher one that is not eligible does not save it, and reports 6
  add(N, make_nann(0xB2, N, 0), 0, 3);                         // 21 a node of channel 200 only
  add(N, make_nann(0xB2, N - 1, 0), 0, 6);                     // 22 ... 6 comes before 3
  add(0, make_dying(200, 15), 0, 2);                           // 23 a dying record of the wrong length keeps nothing
  add(0, make_cann(300, 0xC1, 0xC2), 0, 0);                    // 24 channel 300: at the boundary, kept
  add(0, amount, 0, 0);                                        // 25
  add(N - P, make_cupd(300, 0, N - P), 0, 0);                  // 26
  add(0, make_cann(400, 0xD1, 0xD2), 0, 0);                    // 27 channel 400: long silent, but dying
  add(0, amount, 0, 0);                                        // 28
  add(5, make_cupd(400, 1, 5), 0, 0);                          // 29
  add(0, make_dying(400), 0, 0);                               // 30
  add(0, make_cann(500, 0xE1, 0xE2), 0, 0);                    // 31 channel 500: no update at all
  add(0, amount, 0, 0);                                        // 32
  add(0, make_dying(600), 0, 3);                               // 33 in front of its announcement: marks nothing
  add(0, make_cann(600, 0xF1, 0xC1), 0, 7);                    // 34 channel 600: stale
  add(0, amount, 0, 3);                                        // 35
  add(7, make_cupd(600, 0, 7), 0, 3);                          // 36
  add(N, make_nann(0xC1, N, 0), 0, 0);                         // 37 node C1 is in channel 300 too
  add(N, make_nann(0xF1, N, 0), 0, 3);                         // 38
  {
    const repaired R = repair_any_order(f, v, uuid, pol);
    CHECK(R.reason == want);
    for (size_t i = 0; i < want.size(); i++)
      if (i < R.reason.size() && R.reason[i] != want[i]) printf("record %zu: reason %u, expected %u\n", i, R.reason[i], want[i]);
    const store_head h = store_make_head(0x10, uuid);
    std::vector<u8> img(h.b, h.b + STORE_REPAIR_HEAD);
    for (size_t i = 0; i < want.size(); i++) {
      const u64 end = i + 1 < want.size() ? R.rec_off[i + 1] : f.size();
      CHECK(R.new_off[i] == (want[i] ? ~(u64)0 : (u64)img.size()));
      if (!want[i]) img.insert(img.end(), f.begin() + R.rec_off[i], f.begin() + end);
    }
    CHECK(R.out_len == img.size() && R.image == img && img.size() <= f.size() + 46);
    // without a clock: no 7, no future rule -- channel 200 and 600 stay, record 10 wins direction 1 of channel 100
    const repaired Q = repair_any_order(f, v, uuid, lamd_store_latest_policy{0, S, P});
    CHECK(Q.reason[16] == 0 && Q.reason[34] == 0 && Q.reason[10] == 0 && Q.reason[9] == 5 && Q.reason[19] == 0 && Q.reason[20] == 6 && Q.reason[21] == 0 && Q.reason[22] == 6);
    // a clock, no interval: the future rule alone
    const repaired T = repair_any_order(f, v, uuid, lamd_store_latest_policy{N, S, 0});
    CHECK(T.reason[16] == 0 && T.reason[34] == 0 && T.reason[10] == 6 && T.reason[9] == 0);
    // the output repairs to itself (its uuid record is the one record dropped)
    size_t kept = 0;
    for (u8 r : want) kept += r == 0;
    const std::vector<int8_t> ok(kept + 1, 0);
    const repaired A = repair_any_order(R.image, ok, uuid, pol);
    CHECK(A.image == R.image && A.reason[0] == 4);
    for (size_t i = 1; i < A.reason.size(); i++) CHECK(A.reason[i] == 0);
    // no record at all
    const repaired E = repair_any_order(std::vector<u8>{0x10}, std::vector<int8_t>(), uuid, pol);
    CHECK(E.out_len == STORE_REPAIR_HEAD && E.reason.empty());
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

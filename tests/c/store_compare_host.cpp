// Host build of lightning_amd/csrc/store_compare.h under AddressSanitizer / UBSan (tests/test_store_compare_host.py).
// Without arguments, the program's own checks: the parser's statuses and their precedence, a reply cut at every length, the searches at the
// lists' ends, the closed form of the message offsets against a running sum, the bigsize of the flags' TLV where it grows.
// With arguments IMAGE VERDICTS MSGS CHAIN WANT MAX_UNKNOWN MAX_STALE OUT: the digest of the image file with its bare list (IMAGE "-": an
// empty digest; VERDICTS: one byte per record, or "-"), built with the functions the kernels run; then lamd_channel_range_compare_batch's
// stages over the messages of MSGS (u32 count, then u32 length + bytes per message, little-endian) for the 32-byte chain hash in CHAIN (an
// EMPTY file: every message is parsed against its own chain_hash bytes) and the outstanding queries of WANT (per message u32 first, u32
// end; "-": none): the entries classified in file order, in reverse and in a scrambled order -- the three must agree --, merged, and the
// queries written with the output at all four alignments -- which must agree too.  OUT.status, OUT.permsg (3 x u32 per message),
// OUT.unknown, OUT.stale (u64), OUT.flags (u8), OUT.msgoff (u64), OUT.bytes and OUT.bare (u64) are written for the caller to compare with
// its model.  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_compare.h"

using namespace lamd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static u64 rnd_state = 0x2345678ull;
static u32 rnd() {
  rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
  return (u32)(rnd_state >> 33);
}
template <class T> static T *block(size_t n, int fill) {
  T *p = (T *)malloc(n ? n * sizeof(T) : 1);
  memset(p, fill, n * sizeof(T));
  return p;
}
template <class T> static T *block_of(const std::vector<T> &v) {
  T *p = block<T>(v.size(), 0);
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
static std::vector<u32> visit_order(u32 n, int how) {
  std::vector<u32> o(n);
  for (u32 i = 0; i < n; i++) o[i] = how == 1 ? n - 1 - i : i;
  if (how == 2)
    for (u32 i = n; i > 1; i--) { const u32 j = rnd() % i, t = o[i - 1]; o[i - 1] = o[j]; o[j] = t; }
  return o;
}

struct digest {
  std::vector<u64> scid, bare;
  std::vector<u32> ts;
  bool operator==(const digest &o) const { return scid == o.scid && bare == o.bare && ts == o.ts; }
};
// lamd_gossip_store_digest_build's stages (store_digest.h), each over the records in the order `how`; the bare list as k_digest_chan compacts it
static digest build(const std::vector<u8> &file, const std::vector<int8_t> *verdict, int how) {
  digest D;
  const size_t len = file.size();
  u8 *store = block_of(file);
  lamd_store_summary s;
  std::vector<u64> offs;
  CHECK(store_walk(store, len, &s, [&](size_t, u64 off, const store_hdr &, u32) { offs.push_back(off); }));
  const u32 n = (u32)offs.size();
  if (verdict && verdict->size() != n) { printf("%zu verdicts for %u records\n", verdict->size(), n); exit(2); }
  u64 *off = block_of(offs);
  int8_t *v = verdict ? block_of(*verdict) : nullptr;
  u32 bits = 1;
  while (((size_t)1 << bits) < 2 * (size_t)n) bits++;
  const size_t slots = ((size_t)1 << bits) + 1;
  u64 *keys = block<u64>(slots, 0xFF);
  u32 *vals = block<u32>(slots, 0xFF), *slot = block<u32>(2 * (size_t)n, 0);
  u32 T[4 * 256];
  store_crc_build_tables(T, 4);
  for (u32 i : visit_order(n, how)) store_digest_index_one(store, len, off, v, i, keys, vals, bits);
  for (u32 i : visit_order(n, how)) store_digest_slot_one(store, len, off, v, i, keys, vals, bits, slot);
  std::vector<std::pair<u64, u32>> pairs;
  for (u32 i : visit_order(n, how)) {
    u64 scid = 0;
    const u32 c = store_digest_chan_one(store, len, off, v, i, keys, vals, bits, slot, &scid);
    if (c == 1) pairs.push_back({scid, i});
    if (c == 2) D.bare.push_back(scid);
  }
  std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<u64, u32> &a, const std::pair<u64, u32> &b) { return a.first < b.first; });
  std::sort(D.bare.begin(), D.bare.end());
  for (auto &p : pairs) {
    u32 ts[2], csum[2], rec[3];
    store_digest_entry_one<4>(T, store, len, off, p.second, slot, ts, csum, rec);
    D.scid.push_back(p.first);
    D.ts.push_back(ts[0]);
    D.ts.push_back(ts[1]);
  }
  for (void *p : {(void *)store, (void *)off, (void *)v, (void *)keys, (void *)vals, (void *)slot}) free(p);
  return D;
}

struct result {
  std::vector<int8_t> status;
  std::vector<u32> per_msg;
  std::vector<u64> unknown, stale, msg_off;
  std::vector<u8> flags, bytes;
};
struct lists {
  std::vector<u8> cls;
  std::vector<u64> unknown, stale;
  std::vector<u32> flags;
  bool operator==(const lists &o) const { return cls == o.cls && unknown == o.unknown && stale == o.stale && flags == o.flags; }
};
// k_cmp_classify over the entries in the order `how`, then the merge: sort, heads, run numbers, OR
static lists classify(const u8 *batch, const store_cmp_msg *pm, const u64 *first, u32 n, const store_cmp_digest &d, int how) {
  lists R;
  const u32 E = (u32)first[n];
  R.cls.assign(E, 0xEE);
  std::vector<u64> ukey;
  std::vector<std::pair<u64, u32>> spair;
  for (u32 e : visit_order(E, how)) {
    const u32 i = store_range_locate(first, n, e);
    CHECK(first[i] <= e && e < first[i + 1]);
    u64 scid = 0;
    const u32 c = store_cmp_entry(batch, pm[i], (u32)(e - first[i]), d, &scid);
    R.cls[e] = (u8)c;
    if (c == STORE_CMP_UNKNOWN) ukey.push_back(scid);
    if (c > STORE_CMP_UNKNOWN) spair.push_back({scid, c});
  }
  std::sort(ukey.begin(), ukey.end());
  std::stable_sort(spair.begin(), spair.end(), [](const std::pair<u64, u32> &a, const std::pair<u64, u32> &b) { return a.first < b.first; });
  u64 *uk = block_of(ukey), *sk = block<u64>(spair.size(), 0);
  for (size_t j = 0; j < spair.size(); j++) sk[j] = spair[j].first;
  for (u32 j = 0; j < ukey.size(); j++)
    if (store_cmp_head(uk, j)) R.unknown.push_back(uk[j]);
  for (u32 j = 0; j < spair.size(); j++) {
    if (store_cmp_head(sk, j)) { R.stale.push_back(sk[j]); R.flags.push_back(0); }
    R.flags.back() |= spair[j].second;
  }
  free(uk);
  free(sk);
  return R;
}
static result compare(const digest &D, const u8 *chain32, const std::vector<std::vector<u8>> &msgs, const std::vector<u32> *want, u32 max_unknown, u32 max_stale) {
  result A;
  const u32 n = (u32)msgs.size();
  std::vector<u8> all;
  std::vector<store_cmp_msg> pmv(n);
  std::vector<u64> firstv(n + 1, 0);
  for (u32 i = 0; i < n; i++) {
    u8 *raw = block_of(msgs[i]);
    u8 own[32] = {};
    if (!chain32 && msgs[i].size() >= 34) memcpy(own, &msgs[i][2], 32);
    pmv[i] = store_cmp_parse(raw, msgs[i].size(), all.size(), chain32 ? chain32 : own, want != nullptr, want ? (*want)[2 * i] : 0, want ? (*want)[2 * i + 1] : 0);
    free(raw);
    CHECK((pmv[i].status == STORE_CMP_ACCEPTED) || pmv[i].n == 0);
    A.status.push_back((int8_t)pmv[i].status);
    firstv[i + 1] = firstv[i] + pmv[i].n;
    all.insert(all.end(), msgs[i].begin(), msgs[i].end());
  }
  u8 *batch = block_of(all);
  store_cmp_msg *pm = block_of(pmv);
  u64 *first = block_of(firstv), *scid = block_of(D.scid), *bare = block_of(D.bare);
  u32 *ts = block_of(D.ts);
  const store_cmp_digest d{scid, ts, (u32)D.scid.size(), bare, (u32)D.bare.size()};
  const lists R = classify(batch, pm, first, n, d, 0);
  for (int how : {1, 2, 2}) CHECK(classify(batch, pm, first, n, d, how) == R);
  for (u32 i = 0; i < n; i++) {   // k_cmp_per_msg
    u32 u = 0, s = 0;
    for (u64 e = first[i]; e < first[i + 1]; e++) { u += R.cls[e] == STORE_CMP_UNKNOWN; s += R.cls[e] > STORE_CMP_UNKNOWN; }
    A.per_msg.insert(A.per_msg.end(), {(u32)(first[i + 1] - first[i]), u, s});
  }
  A.unknown = R.unknown;
  A.stale = R.stale;
  for (u32 f : R.flags) { CHECK(f == 2 || f == 4 || f == 6); A.flags.push_back((u8)f); }
  store_cmp_layout y;
  y.unknown = (u32)R.unknown.size();
  y.stale = (u32)R.stale.size();
  y.max_unknown = max_unknown ? max_unknown : STORE_CMP_MAX_UNKNOWN;
  y.max_stale = max_stale ? max_stale : STORE_CMP_MAX_STALE;
  if (chain32) memcpy(y.chain, chain32, 32); else memset(y.chain, 0, 32);
  const u32 n_msgs = (u32)store_cmp_messages(y);
  u64 *msg_off = block<u64>((size_t)n_msgs + 1, 0);   // k_cmp_plan
  for (u32 j = 0; j <= n_msgs; j++) msg_off[j] = store_cmp_msg_off(y, j);
  A.msg_off.assign(msg_off, msg_off + n_msgs + 1);
  const u64 total = msg_off[n_msgs];
  u64 *lu = block_of(R.unknown), *ls = block_of(R.stale);
  u32 *lf = block_of(R.flags);
  for (u32 mis = 0; mis < 4 && n_msgs; mis++) {   // k_cmp_encode, the output at every alignment
    u8 *raw = block<u8>((size_t)total + 4, 0xEE), *out = raw + mis;
    for (u64 k = 0; 4 * k < total + mis; k++) store_cmp_word(y, msg_off, n_msgs, lu, ls, lf, out, total, mis, k);
    for (u32 b = 0; b < mis; b++) CHECK(raw[b] == 0xEE);
    for (u32 b = mis; b < 4; b++) CHECK(out[total + b - mis] == 0xEE);
    if (mis == 0) A.bytes.assign(out, out + total);
    else CHECK(!memcmp(out, A.bytes.data(), (size_t)total));
    free(raw);
  }
  for (void *p : {(void *)batch, (void *)pm, (void *)first, (void *)scid, (void *)bare, (void *)ts, (void *)msg_off, (void *)lu, (void *)ls, (void *)lf}) free(p);
  return A;
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
  if (!f || (len && fwrite(p, 1, len, f) != len)) { printf("cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}
static void be(std::vector<u8> &m, u64 v, int width) {
  for (int s = 8 * (width - 1); s >= 0; s -= 8) m.push_back((u8)(v >> s));
}
// a reply with the given encoded_short_ids and TLV bytes
static std::vector<u8> make_reply(const u8 *chain32, u32 first, u32 number, const std::vector<u8> &encoded, const std::vector<u8> &tlvs) {
  std::vector<u8> m = {1, 8};
  m.insert(m.end(), chain32, chain32 + 32);
  be(m, first, 4);
  be(m, number, 4);
  m.push_back(1);
  be(m, encoded.size(), 2);
  m.insert(m.end(), encoded.begin(), encoded.end());
  m.insert(m.end(), tlvs.begin(), tlvs.end());
  return m;
}
static std::vector<u8> scids_of(u32 n, u8 encoding = 0) {
  std::vector<u8> e = {encoding};
  for (u32 k = 0; k < n; k++) be(e, ((u64)(100 + k) << 40) | k, 8);
  return e;
}
static std::vector<u8> ts_tlv(u32 n, u8 encoding = 0, u32 extra = 0) {
  std::vector<u8> t = {1, (u8)(1 + 8 * n + extra), encoding};
  for (u32 k = 0; k < 8 * n + extra; k++) t.push_back((u8)k);
  return t;
}
static std::vector<u8> cat(std::vector<u8> a, const std::vector<u8> &b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

int main(int argc, char **argv) {
  if (argc == 9) {
    const bool with_image = strcmp(argv[1], "-") != 0, with_verdict = strcmp(argv[2], "-") != 0, with_want = strcmp(argv[5], "-") != 0;
    const std::vector<u8> mb = read_file(argv[3]), chain = read_file(argv[4]);
    std::vector<int8_t> verdict;
    if (with_verdict) { const std::vector<u8> vb = read_file(argv[2]); verdict.assign(vb.begin(), vb.end()); }
    if ((chain.size() != 32 && !chain.empty()) || mb.size() < 4) { printf("the chain file has %zu bytes, the message file %zu\n", chain.size(), mb.size()); return 2; }
    digest D;
    if (with_image) {
      const std::vector<u8> file = read_file(argv[1]);
      D = build(file, with_verdict ? &verdict : nullptr, 0);
      for (int how : {1, 2}) CHECK(build(file, with_verdict ? &verdict : nullptr, how) == D);
    }
    std::vector<std::vector<u8>> msgs;
    u32 n, pos = 4;
    memcpy(&n, mb.data(), 4);
    for (u32 i = 0; i < n; i++) {
      u32 l;
      if (mb.size() - pos < 4) { printf("the message file is cut off\n"); return 2; }
      memcpy(&l, &mb[pos], 4);
      pos += 4;
      if (mb.size() - pos < l) { printf("the message file is cut off\n"); return 2; }
      msgs.emplace_back(mb.begin() + pos, mb.begin() + pos + l);
      pos += l;
    }
    std::vector<u32> want;
    if (with_want) {
      const std::vector<u8> wb = read_file(argv[5]);
      if (wb.size() != 8 * (size_t)n) { printf("the want file has %zu bytes for %u messages\n", wb.size(), n); return 2; }
      want.resize(2 * (size_t)n);
      if (n) memcpy(want.data(), wb.data(), wb.size());
    }
    const result A = compare(D, chain.empty() ? nullptr : chain.data(), msgs, with_want ? &want : nullptr, (u32)strtoul(argv[6], nullptr, 10),
                             (u32)strtoul(argv[7], nullptr, 10));
    const std::string base = argv[8];
    write_file(base + ".status", A.status.data(), A.status.size());
    write_file(base + ".permsg", A.per_msg.data(), 4 * A.per_msg.size());
    write_file(base + ".unknown", A.unknown.data(), 8 * A.unknown.size());
    write_file(base + ".stale", A.stale.data(), 8 * A.stale.size());
    write_file(base + ".flags", A.flags.data(), A.flags.size());
    write_file(base + ".msgoff", A.msg_off.data(), 8 * A.msg_off.size());
    write_file(base + ".bytes", A.bytes.data(), A.bytes.size());
    write_file(base + ".bare", D.bare.data(), 8 * D.bare.size());
    if (failures) return 1;
    printf("ok\n");
    return 0;
  }
  u8 chain[32], other[32];
  for (int i = 0; i < 32; i++) { chain[i] = (u8)(i + 1); other[i] = (u8)(i + 1); }
  other[0] ^= 0x80;
  auto parse = [&](const std::vector<u8> &m, bool have_want = false, u32 wf = 0, u32 we = 0) {
    u8 *p = block_of(m);
    const store_cmp_msg r = store_cmp_parse(p, m.size(), 1000, chain, have_want, wf, we);
    free(p);
    CHECK(r.status == STORE_CMP_ACCEPTED || (r.n == 0 && r.ts_at == STORE_CMP_NO_TS));
    return r;
  };
  // ---- the parser: every status, then the order of precedence
  {
    store_cmp_msg r = parse(make_reply(chain, 7, 9, scids_of(3), {}));
    CHECK(r.status == 0 && r.n == 3 && r.scid_at == 1046 && r.ts_at == STORE_CMP_NO_TS);
    r = parse(make_reply(chain, 7, 9, scids_of(3), cat(ts_tlv(3), {3, 24, 1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8})));
    CHECK(r.status == 0 && r.n == 3 && r.ts_at == 1000 + 45 + 25 + 3);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(0), {})).status == 0 && parse(make_reply(chain, 7, 9, scids_of(0), {})).n == 0);   // the encoding byte alone
    CHECK(parse(make_reply(chain, 7, 9, scids_of(0), ts_tlv(0))).status == 0);
    std::vector<u8> m = make_reply(chain, 7, 9, scids_of(1), {});
    m[1] = 7;
    CHECK(parse(m).status == -1);                                                                  // a query, not a reply
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {1, 0})).status == -1);                        // TLV 1 without its encoding byte
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {3, 7, 0, 0, 0, 0, 0, 0, 0})).status == -1);   // TLV 3 of 7 bytes
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {3, 0})).status == 0 && parse(make_reply(chain, 7, 9, scids_of(1), {3, 8, 0, 0, 0, 0, 0, 0, 0, 0})).status == 0);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {2, 0})).status == -1 && parse(make_reply(chain, 7, 9, scids_of(1), {0, 0})).status == -1);   // unknown even
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {5, 1, 0xAA})).status == 0);                   // unknown odd
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), cat({3, 0}, ts_tlv(1)))).status == -1);        // descending
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), cat(ts_tlv(1), ts_tlv(1)))).status == -1);     // twice
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {0xfd, 0, 1, 1, 0})).status == -1);            // type not minimal
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {1, 0xfd, 0, 9, 0, 1, 2, 3, 4, 5, 6, 7, 8})).status == -1);   // length not minimal
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), {1, 9, 0, 1, 2, 3})).status == -1);            // value cut off
    m = make_reply(chain, 7, 9, scids_of(1), {});
    m[44] = 10;                                                                                     // len runs past the end
    CHECK(parse(m).status == -1);
    CHECK(parse(make_reply(other, 7, 9, scids_of(1), {})).status == 1);
    CHECK(parse(make_reply(chain, 0xFFFFFFFFu, 1, scids_of(1), {})).status == 2 && parse(make_reply(chain, 0xFFFFFFFEu, 1, scids_of(1), {})).status == 0);
    CHECK(parse(make_reply(chain, 7, 9, {}, {})).status == 3 && parse(make_reply(chain, 7, 9, scids_of(1, 1), {})).status == 3);
    m = scids_of(2);
    m.pop_back();
    CHECK(parse(make_reply(chain, 7, 9, m, {})).status == 3);
    const std::vector<u8> ok = make_reply(chain, 100, 50, scids_of(1), {});                         // blocks [100, 150)
    CHECK(parse(ok, true, 150, 200).status == 4 && parse(ok, true, 149, 200).status == 0 && parse(ok, true, 0, 100).status == 4 && parse(ok, true, 0, 101).status == 0);
    CHECK(parse(ok, true, 100, 150).status == 0 && parse(ok, true, 0, 0xFFFFFFFFu).status == 0 && parse(ok, true, 120, 120).status == 0 &&
          parse(ok, true, 150, 150).status == 4 && parse(ok, true, 100, 100).status == 4);   // the formula of :257-258, an empty query included
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), ts_tlv(1, 1))).status == 5 && parse(make_reply(chain, 7, 9, scids_of(1), ts_tlv(1, 0, 3))).status == 5);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(2), ts_tlv(1))).status == 6 && parse(make_reply(chain, 7, 9, scids_of(1), ts_tlv(2))).status == 6 &&
          parse(make_reply(chain, 7, 9, scids_of(1), ts_tlv(0))).status == 6);
    // precedence: malformed < foreign < overflow < scids < overlap < timestamps < count
    CHECK(parse(make_reply(other, 0xFFFFFFFFu, 1, scids_of(1, 1), {2, 0})).status == -1);
    CHECK(parse(make_reply(other, 0xFFFFFFFFu, 1, scids_of(1, 1), ts_tlv(1, 1)), true, 0, 1).status == 1);
    CHECK(parse(make_reply(chain, 0xFFFFFFFFu, 1, scids_of(1, 1), ts_tlv(1, 1)), true, 0, 1).status == 2);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1, 1), ts_tlv(1, 1)), true, 0, 1).status == 3);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(1), ts_tlv(1, 1)), true, 0, 1).status == 4);
    CHECK(parse(make_reply(chain, 7, 9, scids_of(2), ts_tlv(1, 1)), true, 0, 8).status == 5);
    // a 3-entry reply with both TLVs (70 + 27 + 26 bytes) cut at every length: whole at 70, 97 and 123
    std::vector<u8> csum = {3, 24};
    for (int k = 0; k < 24; k++) csum.push_back((u8)(0xC0 + k));
    const std::vector<u8> full = make_reply(chain, 7, 9, scids_of(3), cat(ts_tlv(3), csum));
    CHECK(full.size() == 123);
    for (size_t l = 0; l <= full.size(); l++) {
      r = parse(std::vector<u8>(full.begin(), full.begin() + l));
      CHECK(r.status == (l == 70 || l == 97 || l == 123 ? 0 : -1));
      if (r.status == 0) CHECK(r.n == 3 && (r.ts_at == STORE_CMP_NO_TS) == (l == 70));
    }
  }
  // ---- the searches
  {
    const std::vector<u64> v = {5, 9, 9000, ~(u64)0 - 1, ~(u64)0};
    u64 *a = block_of(v);
    for (u32 k = 0; k < v.size(); k++) CHECK(store_cmp_find(a, (u32)v.size(), v[k]) == k);
    for (u64 x : {(u64)0, (u64)4, (u64)6, (u64)8999, ~(u64)0 - 2}) CHECK(store_cmp_find(a, (u32)v.size(), x) == STORE_NONE);
    CHECK(store_cmp_find(a, 4, ~(u64)0) == STORE_NONE && store_cmp_find(nullptr, 0, 5) == STORE_NONE && store_cmp_find(a, 1, 5) == 0 && store_cmp_find(a, 1, 9) == STORE_NONE);
    free(a);
  }
  // ---- the layout: the closed form against a running sum; the flags' TLV length grows from 1 to 3 bytes at k = 252
  CHECK(store_cmp_query_bytes(1, false) == 45 && store_cmp_query_bytes(8000, false) == 64037 && store_cmp_query_bytes(7000, true) == 63042);
  CHECK(store_cmp_query_bytes(251, true) == 37 + 8 * 251 + 3 + 251 && store_cmp_query_bytes(252, true) == 37 + 8 * 252 + 5 + 252);
  for (u32 mu : {1u, 2u, 3u, 7u, 252u, 8000u})
    for (u32 ms : {1u, 3u, 251u, 252u, 253u, 7000u})
      for (u32 U : {0u, 1u, mu - 1, mu, mu + 1, 3 * mu + 1})
        for (u32 S : {0u, 1u, ms - 1, ms, ms + 1, 3 * ms + 1}) {
          store_cmp_layout y;
          y.unknown = U; y.stale = S; y.max_unknown = mu; y.max_stale = ms;
          memcpy(y.chain, chain, 32);
          const u64 M = store_cmp_messages(y);
          CHECK(M == (U + mu - 1) / mu + (S + ms - 1) / ms);
          u64 sum = 0;
          for (u64 j = 0; j < M; j++) {
            CHECK(store_cmp_msg_off(y, j) == sum);
            const bool st = j >= (U + mu - 1) / mu;
            const u64 jj = st ? j - (U + mu - 1) / mu : j, per = st ? ms : mu, cnt = st ? S : U;
            const u32 k = (u32)std::min<u64>(per, cnt - jj * per);
            CHECK(k >= 1);
            sum += store_cmp_query_bytes(k, st);
            CHECK(store_cmp_query_bytes(k, st) <= 65535);
          }
          CHECK(store_cmp_msg_off(y, M) == sum);
        }
  // ---- classification and merge by hand: a digest of two entries and one bare channel
  {
    digest D;
    D.scid = {10, 20};
    D.ts = {100, 0, 50, 60};
    D.bare = {15};
    auto scids_ts = [&](std::vector<std::pair<u64, std::pair<u32, u32>>> es, bool with_ts) {
      std::vector<u8> enc = {0}, t = {1, (u8)(1 + 8 * es.size()), 0};
      for (auto &e : es) { be(enc, e.first, 8); be(t, e.second.first, 4); be(t, e.second.second, 4); }
      return make_reply(chain, 0, 100, enc, with_ts ? t : std::vector<u8>{});
    };
    std::vector<std::vector<u8>> msgs = {
        scids_ts({{10, {100, 0}}, {20, {50, 60}}, {15, {0, 0}}, {30, {0, 0}}}, true),   // equal, equal, bare with nothing, unknown
        scids_ts({{10, {101, 0}}, {20, {49, 61}}, {15, {5, 0}}, {30, {9, 9}}}, true),   // flag 2, flag 4, bare flag 2, unknown again
        scids_ts({{10, {0, 1}}, {20, {51, 0}}, {15, {0, 7}}}, true),                     // flag 4 (slot unset, theirs != 0), flag 2, flag 4
        scids_ts({{10, {999, 999}}, {40, {1, 1}}}, false),                               // no TLV 1: known is never stale; unknown stays unknown
        make_reply(other, 0, 100, scids_of(5), {})};                                     // rejected: contributes nothing
    const result A = compare(D, chain, msgs, nullptr, 0, 0);
    CHECK(A.status == (std::vector<int8_t>{0, 0, 0, 0, 1}));
    CHECK(A.per_msg == (std::vector<u32>{4, 1, 0, 4, 1, 3, 3, 0, 3, 2, 1, 0, 0, 0, 0}));
    CHECK(A.unknown == (std::vector<u64>{30, 40}) && A.stale == (std::vector<u64>{10, 15, 20}) && A.flags == (std::vector<u8>{6, 6, 6}));
    CHECK(A.msg_off == (std::vector<u64>{0, 37 + 16, 37 + 16 + 37 + 24 + 3 + 3}));
    const u8 *q = &A.bytes[53];
    CHECK(store_be16(q) == 261 && !memcmp(q + 2, chain, 32) && store_be16(q + 34) == 25 && q[36] == 0 && store_be64(q + 37) == 10 && store_be64(q + 53) == 20 &&
          q[61] == 1 && q[62] == 4 && q[63] == 0 && q[64] == 6 && q[66] == 6);
    const result B = compare(D, chain, msgs, nullptr, 1, 2);
    CHECK(B.msg_off.size() == 5 && B.unknown == A.unknown && B.flags == A.flags && B.msg_off[4] == 2 * 45 + (37 + 16 + 3 + 2) + (37 + 8 + 3 + 1));
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

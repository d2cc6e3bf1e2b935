// Host build of lightning_amd/csrc/store_digest.h under AddressSanitizer / UBSan (tests/test_store_digest_host.py).
// Without arguments, the program's own checks: bigsize, the four uncapped limits and capped ones, the binary searches at the digest's ends,
// the split's corners (a block larger than a reply, the iteration bound) and the parser's rules.
// With arguments IMAGE VERDICTS QUERIES CHAIN MAX_ENCODED_BYTES OUT: the digest of the image file (VERDICTS: one byte per record of the walk,
// or "-" for none), built stage by stage with the functions the kernels run, in file order, in reverse and in a scrambled order of the
// records -- the three must agree; then the replies to the queries of QUERIES (u32 count, then u32 length + bytes per query, little-endian)
// for the 32-byte chain hash in CHAIN, written with the output at all four alignments -- which must agree too.  OUT.digest (u32 count, then
// per entry u64 scid | u32 ts[2] | u32 csum[2] | u32 rec[3]), OUT.counters (7 x u64: the summary's), OUT.status, OUT.first (u64), OUT.msgoff
// (u64) and OUT.bytes are written for the caller to compare with its model.  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_digest.h"

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
static std::vector<u32> visit_order(u32 n, int how) {
  std::vector<u32> o(n);
  for (u32 i = 0; i < n; i++) o[i] = how == 1 ? n - 1 - i : i;
  if (how == 2)
    for (u32 i = n; i > 1; i--) { const u32 j = rnd() % i, t = o[i - 1]; o[i - 1] = o[j]; o[j] = t; }
  return o;
}

struct digest {
  std::vector<u64> scid;
  std::vector<u32> ts, csum, rec;
  u64 counters[7] = {};   // records, channels, entries, channels_no_update, updates_no_channel, updates_in_front, updates_short
  bool operator==(const digest &o) const {
    return scid == o.scid && ts == o.ts && csum == o.csum && rec == o.rec && !memcmp(counters, o.counters, sizeof counters);
  }
};
// lamd_gossip_store_digest_build's stages, each over the records in the order `how`
static digest build(const std::vector<u8> &file, const std::vector<int8_t> *verdict, int how) {
  digest D;
  const size_t len = file.size();
  u8 *store = block<u8>(len, 0);
  memcpy(store, file.data(), len);
  lamd_store_summary s;
  std::vector<u64> offs;
  CHECK(store_walk(store, len, &s, [&](size_t, u64 off, const store_hdr &, u32) { offs.push_back(off); }));
  const u32 n = (u32)offs.size();
  if (verdict && verdict->size() != n) { printf("%zu verdicts for %u records\n", verdict->size(), n); exit(2); }
  u64 *off = block<u64>(n, 0);
  int8_t *v = verdict ? block<int8_t>(n, 0) : nullptr;
  for (u32 i = 0; i < n; i++) { off[i] = offs[i]; if (v) v[i] = (*verdict)[i]; }
  u32 bits = 1;
  while (((size_t)1 << bits) < 2 * (size_t)n) bits++;
  const size_t slots = ((size_t)1 << bits) + 1;
  u64 *keys = block<u64>(slots, 0xFF), *pkey = block<u64>(n, 0xFF), *skey = block<u64>(n, 0);
  u32 *vals = block<u32>(slots, 0xFF), *slot = block<u32>(2 * (size_t)n, 0), *pval = block<u32>(n, 0xFF), *ann = block<u32>(n, 0);
  u32 T[4 * 256];
  store_crc_build_tables(T, 4);
  for (u32 i : visit_order(n, how)) store_digest_index_one(store, len, off, v, i, keys, vals, bits);
  for (u32 i : visit_order(n, how)) {
    const u32 r = store_digest_slot_one(store, len, off, v, i, keys, vals, bits, slot);
    D.counters[4] += r == STORE_DIGEST_UPD_NO_CHANNEL;
    D.counters[5] += r == STORE_DIGEST_UPD_IN_FRONT;
    D.counters[6] += r == STORE_DIGEST_UPD_SHORT;
  }
  u32 count = 0;
  for (u32 i : visit_order(n, how)) {
    u64 scid = 0;
    const u32 c = store_digest_chan_one(store, len, off, v, i, keys, vals, bits, slot, &scid);
    if (c == 1) { pkey[count] = scid; pval[count] = i; count++; }
    D.counters[1] += c != 0;
    D.counters[3] += c == 2;
  }
  D.counters[0] = n;
  D.counters[2] = count;
  // the sort of all n pairs, stable: the pads (largest key) stay behind the real pairs
  std::vector<u32> perm(n);
  for (u32 i = 0; i < n; i++) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](u32 a, u32 b) { return pkey[a] < pkey[b]; });
  for (u32 i = 0; i < n; i++) { skey[i] = pkey[perm[i]]; ann[i] = pval[perm[i]]; }
  u32 *ts = block<u32>(2 * (size_t)count, 0), *csum = block<u32>(2 * (size_t)count, 0), *rec = block<u32>(3 * (size_t)count, 0);
  for (u32 j : visit_order(count, how)) {
    CHECK(ann[j] < n);
    store_digest_entry_one<4>(T, store, len, off, ann[j], slot, ts + 2 * (size_t)j, csum + 2 * (size_t)j, rec + 3 * (size_t)j);
  }
  D.scid.assign(skey, skey + count);
  D.ts.assign(ts, ts + 2 * (size_t)count);
  D.csum.assign(csum, csum + 2 * (size_t)count);
  D.rec.assign(rec, rec + 3 * (size_t)count);
  for (void *p : {(void *)store, (void *)off, (void *)v, (void *)keys, (void *)pkey, (void *)skey, (void *)vals, (void *)slot, (void *)pval, (void *)ann, (void *)ts,
                  (void *)csum, (void *)rec})
    free(p);
  return D;
}
static digest build_any_order(const std::vector<u8> &file, const std::vector<int8_t> *verdict) {
  const digest D = build(file, verdict, 0);
  for (int how : {1, 2, 2}) CHECK(build(file, verdict, how) == D);
  return D;
}

struct answers {
  std::vector<int8_t> status;
  std::vector<u64> first, msg_off;
  std::vector<u8> bytes;
};
// lamd_channel_range_reply_batch's stages over exact-size copies of the digest
static answers reply(const digest &D, const u8 *chain32, const std::vector<std::vector<u8>> &queries, u32 max_encoded_bytes) {
  answers A;
  const u32 nq = (u32)queries.size(), count = (u32)D.scid.size();
  u64 *scid = block<u64>(count, 0);
  u32 *ts = block<u32>(2 * (size_t)count, 0), *csum = block<u32>(2 * (size_t)count, 0);
  if (count) {
    memcpy(scid, D.scid.data(), 8 * (size_t)count);
    memcpy(ts, D.ts.data(), 8 * (size_t)count);
    memcpy(csum, D.csum.data(), 8 * (size_t)count);
  }
  store_range_query *qs = block<store_range_query>(nq, 0);
  for (u32 q = 0; q < nq; q++) {
    u8 *raw = block<u8>(queries[q].size(), 0);
    if (!queries[q].empty()) memcpy(raw, queries[q].data(), queries[q].size());
    qs[q] = store_range_parse(raw, queries[q].size(), chain32, max_encoded_bytes);
    free(raw);
    A.status.push_back((int8_t)qs[q].kind);
  }
  u64 n_msgs = 0, total = 0;
  A.first.assign(nq + 1, 0);
  std::vector<u64> bfirst(nq + 1, 0);
  for (u32 q = 0; q < nq; q++) {   // k_range_count, k_range_scan
    const store_range_total t = store_range_plan(qs[q], q, scid, count, nullptr, 0);
    A.first[q] = n_msgs;
    bfirst[q] = total;
    n_msgs += t.msgs;
    total += t.bytes;
  }
  A.first[nq] = n_msgs;
  store_range_msg *msgs = block<store_range_msg>((size_t)n_msgs, 0);
  u64 *msg_off = block<u64>((size_t)n_msgs + 1, 0);
  for (u32 q = 0; q < nq; q++) {   // k_range_plan
    const u64 j0 = A.first[q];
    const store_range_total t = store_range_plan(qs[q], q, scid, count, msgs + j0, (u32)(n_msgs - j0));
    CHECK(t.msgs == A.first[q + 1] - j0);
    u64 o = bfirst[q];
    for (u32 k = 0; k < t.msgs; k++) { msg_off[j0 + k] = o; o += store_range_msg_bytes(qs[q], msgs[j0 + k].n); }
    CHECK(o == bfirst[q] + t.bytes);
    // a cap one short: the same replies, nothing behind the cap
    if (t.msgs > 1) {
      store_range_msg *few = block<store_range_msg>(t.msgs - 1, 0);
      CHECK(store_range_plan(qs[q], q, scid, count, few, t.msgs - 1).msgs == t.msgs && !memcmp(few, msgs + j0, sizeof(store_range_msg) * (t.msgs - 1)));
      free(few);
    }
  }
  msg_off[n_msgs] = total;
  A.msg_off.assign(msg_off, msg_off + n_msgs + 1);
  const store_digest_view view{scid, ts, csum};
  for (u32 mis = 0; mis < 4 && n_msgs; mis++) {   // k_range_encode, the output at every alignment
    u8 *raw = block<u8>((size_t)total + 4, 0xEE), *out = raw + mis;
    for (u64 k = 0; 4 * k < total + mis; k++) store_range_word(msgs, msg_off, (u32)n_msgs, qs, view, out, total, mis, k);
    for (u32 b = 0; b < mis; b++) CHECK(raw[b] == 0xEE);
    for (u32 b = mis; b < 4; b++) CHECK(out[total + b - mis] == 0xEE);
    if (mis == 0) A.bytes.assign(out, out + total);
    else CHECK(!memcmp(out, A.bytes.data(), (size_t)total));
    free(raw);
  }
  for (void *p : {(void *)scid, (void *)ts, (void *)csum, (void *)qs, (void *)msgs, (void *)msg_off}) free(p);
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
static std::vector<u8> make_query(const u8 *chain32, u32 first, u32 number, const std::vector<u8> &tlvs) {
  std::vector<u8> q = {1, 7};
  q.insert(q.end(), chain32, chain32 + 32);
  for (u32 x : {first, number})
    for (int s = 24; s >= 0; s -= 8) q.push_back((u8)(x >> s));
  q.insert(q.end(), tlvs.begin(), tlvs.end());
  return q;
}

int main(int argc, char **argv) {
  if (argc == 7) {
    const std::vector<u8> file = read_file(argv[1]), qb = read_file(argv[3]), chain = read_file(argv[4]);
    std::vector<int8_t> verdict;
    const bool with_verdict = strcmp(argv[2], "-") != 0;
    if (with_verdict) { const std::vector<u8> vb = read_file(argv[2]); verdict.assign(vb.begin(), vb.end()); }
    if (chain.size() != 32 || qb.size() < 4) { printf("the chain file has %zu bytes, the query file %zu\n", chain.size(), qb.size()); return 2; }
    const digest D = build_any_order(file, with_verdict ? &verdict : nullptr);
    std::vector<std::vector<u8>> queries;
    u32 nq, pos = 4;
    memcpy(&nq, qb.data(), 4);
    for (u32 q = 0; q < nq; q++) {
      u32 l;
      if (qb.size() - pos < 4) { printf("the query file is cut off\n"); return 2; }
      memcpy(&l, &qb[pos], 4);
      pos += 4;
      if (qb.size() - pos < l) { printf("the query file is cut off\n"); return 2; }
      queries.emplace_back(qb.begin() + pos, qb.begin() + pos + l);
      pos += l;
    }
    const answers A = reply(D, chain.data(), queries, (u32)strtoul(argv[5], nullptr, 10));
    const std::string base = argv[6];
    std::vector<u8> dg(4 + 36 * D.scid.size());
    const u32 count = (u32)D.scid.size();
    memcpy(&dg[0], &count, 4);
    for (u32 j = 0; j < count; j++) {
      u8 *e = &dg[4 + 36 * (size_t)j];
      memcpy(e, &D.scid[j], 8);
      memcpy(e + 8, &D.ts[2 * (size_t)j], 8);
      memcpy(e + 16, &D.csum[2 * (size_t)j], 8);
      memcpy(e + 24, &D.rec[3 * (size_t)j], 12);
    }
    write_file(base + ".digest", dg.data(), dg.size());
    write_file(base + ".counters", D.counters, sizeof D.counters);
    write_file(base + ".status", A.status.data(), A.status.size());
    write_file(base + ".first", A.first.data(), 8 * A.first.size());
    write_file(base + ".msgoff", A.msg_off.data(), 8 * A.msg_off.size());
    write_file(base + ".bytes", A.bytes.data(), A.bytes.size());
    if (failures) return 1;
    printf("ok\n");
    return 0;
  }
  // ---- bigsize: every width at its smallest and largest value, the non-minimal forms, the cut-off ones
  {
    struct { std::vector<u8> b; bool ok; u64 v; } cases[] = {
        {{0x00}, true, 0}, {{0xfc}, true, 0xfc}, {{0xfd, 0x00, 0xfd}, true, 0xfd}, {{0xfd, 0xff, 0xff}, true, 0xffff}, {{0xfd, 0x00, 0xfc}, false, 0},
        {{0xfe, 0x00, 0x01, 0x00, 0x00}, true, 0x10000}, {{0xfe, 0x00, 0x00, 0xff, 0xff}, false, 0}, {{0xff, 0, 0, 0, 1, 0, 0, 0, 0}, true, 0x100000000ull},
        {{0xff, 0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff}, false, 0}, {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, true, ~(u64)0}, {{0xfd, 0x01}, false, 0},
        {{0xfe, 1, 2, 3}, false, 0}, {{0xff, 1, 2, 3, 4, 5, 6, 7}, false, 0}, {{}, false, 0}};
    for (auto &c : cases) {
      u8 *p = block<u8>(c.b.size(), 0);
      if (!c.b.empty()) memcpy(p, c.b.data(), c.b.size());
      size_t pos = 0;
      u64 v = 0;
      const bool ok = store_bigsize(p, c.b.size(), &pos, &v);
      CHECK(ok == c.ok);
      if (ok) CHECK(v == c.v && pos == c.b.size() && store_bigsize_len(v) == c.b.size());
      free(p);
    }
  }
  // ---- max_entries()
  CHECK(store_range_limit(0, 0) == 8186 && store_range_limit(1, 0) == 4092 && store_range_limit(2, 0) == 4092 && store_range_limit(3, 0) == 2728);
  CHECK(store_range_limit(0, 8) == 1 && store_range_limit(0, 7) == 1 && store_range_limit(0, 1) == 1 && store_range_limit(3, 23) == 1 && store_range_limit(3, 24) == 1);
  CHECK(store_range_limit(0, 16) == 2 && store_range_limit(0, 23) == 2 && store_range_limit(3, 72) == 3 && store_range_limit(1, 112) == 7 && store_range_limit(0, 1u << 30) == 8186);
  CHECK(store_range_fix(5, 0xFFFFFFFBu) == 0xFFFFFFFAu && store_range_fix(5, 0xFFFFFFFAu) == 0xFFFFFFFAu && store_range_fix(0, 0xFFFFFFFFu) == 0xFFFFFFFFu &&
        store_range_fix(0xFFFFFFFFu, 1) == 0 && store_range_fix(0xFFFFFFFFu, 0) == 0);
  u8 chain[32], other[32];
  for (int i = 0; i < 32; i++) { chain[i] = (u8)(i + 1); other[i] = (u8)(i + 1); }
  other[31] ^= 1;
  // ---- the parser
  {
    auto parse = [&](const std::vector<u8> &q) {
      u8 *p = block<u8>(q.size(), 0);
      if (!q.empty()) memcpy(p, q.data(), q.size());
      const store_range_query r = store_range_parse(p, q.size(), chain, 0);
      free(p);
      return r;
    };
    store_range_query r = parse(make_query(chain, 7, 9, {}));
    CHECK(r.kind == STORE_RANGE_ANSWERED && r.first == 7 && r.number == 9 && r.opts == 0 && r.limit == 8186);
    for (u32 o = 0; o < 8; o++) {
      r = parse(make_query(chain, 7, 9, {1, 1, (u8)o}));
      CHECK(r.kind == STORE_RANGE_ANSWERED && r.opts == (o & 3) && r.limit == store_range_limit(o & 3, 0));
    }
    CHECK(parse(make_query(chain, 7, 9, {1, 3, 0xfd, 0x01, 0x00})).kind == STORE_RANGE_ANSWERED && parse(make_query(chain, 7, 9, {1, 3, 0xfd, 0x01, 0x03})).opts == 3);
    CHECK(parse(make_query(chain, 7, 9, {1, 3, 0xfd, 0x00, 0x03})).kind == STORE_RANGE_MALFORMED);   // value not minimal
    CHECK(parse(make_query(chain, 7, 9, {1, 2, 0x03, 0x00})).kind == STORE_RANGE_MALFORMED);         // length longer than the value
    CHECK(parse(make_query(chain, 7, 9, {1, 0})).kind == STORE_RANGE_MALFORMED);
    CHECK(parse(make_query(chain, 7, 9, {0xfd, 0x00, 0x01, 1, 3})).kind == STORE_RANGE_MALFORMED);   // type not minimal
    CHECK(parse(make_query(chain, 7, 9, {1, 0xfd, 0x00, 0x01, 3})).kind == STORE_RANGE_MALFORMED);   // length not minimal
    CHECK(parse(make_query(chain, 7, 9, {3, 0, 1, 1, 3})).kind == STORE_RANGE_MALFORMED);            // descending
    CHECK(parse(make_query(chain, 7, 9, {1, 1, 3, 1, 1, 3})).kind == STORE_RANGE_MALFORMED);         // twice
    CHECK(parse(make_query(chain, 7, 9, {2, 0})).kind == STORE_RANGE_MALFORMED && parse(make_query(chain, 7, 9, {0, 0})).kind == STORE_RANGE_MALFORMED);
    r = parse(make_query(chain, 7, 9, {1, 1, 2, 3, 2, 0xAA, 0xBB, 0xfd, 0x01, 0x01, 0}));          // unknown odd types are skipped
    CHECK(r.kind == STORE_RANGE_ANSWERED && r.opts == 2);
    CHECK(parse(make_query(chain, 7, 9, {3, 2, 0xAA})).kind == STORE_RANGE_MALFORMED);               // value cut off
    r = parse(make_query(other, 7, 9, {1, 1, 3}));
    CHECK(r.kind == STORE_RANGE_FOREIGN && r.first == 7 && r.number == 9 && !memcmp(r.chain, other, 32));
    CHECK(parse(make_query(other, 7, 9, {2, 0})).kind == STORE_RANGE_MALFORMED);                     // malformed comes first
    std::vector<u8> q = make_query(chain, 7, 9, {});
    q[1] = 8;
    CHECK(parse(q).kind == STORE_RANGE_MALFORMED);
    q = make_query(chain, 7, 9, {1, 1, 3});
    for (size_t l = 0; l < q.size(); l++) CHECK(parse(std::vector<u8>(q.begin(), q.begin() + l)).kind == (l == 42 ? STORE_RANGE_ANSWERED : STORE_RANGE_MALFORMED));
  }
  // ---- searches and split on a digest built by hand: blocks 10 (1 entry), 20 (3), 21 (1), 0xFFFFFF (2)
  {
    digest D;
    for (u64 s : {((u64)10 << 40) | 5, ((u64)20 << 40) | 1, ((u64)20 << 40) | 2, ((u64)20 << 40) | 3, ((u64)21 << 40), ((u64)0xFFFFFF << 40), ~(u64)0}) {
      D.scid.push_back(s);
      for (int d = 0; d < 2; d++) { D.ts.push_back((u32)(s >> 40) + d); D.csum.push_back(rnd()); }
    }
    const u32 n = (u32)D.scid.size();
    u64 *s = block<u64>(n, 0);
    memcpy(s, D.scid.data(), 8 * (size_t)n);
    CHECK(store_range_bound(s, n, 0, false) == 0 && store_range_bound(s, n, 10, false) == 0 && store_range_bound(s, n, 10, true) == 1 && store_range_bound(s, n, 11, false) == 1);
    CHECK(store_range_bound(s, n, 20, false) == 1 && store_range_bound(s, n, 20, true) == 4 && store_range_bound(s, n, 0xFFFFFF, false) == 5 &&
          store_range_bound(s, n, 0xFFFFFF, true) == 7 && store_range_bound(s, n, 0x1000000, false) == 7 && store_range_bound(s, n, 0xFFFFFFFFu, true) == 7);
    CHECK(store_range_bound(nullptr, 0, 5, false) == 0 && store_range_bound(nullptr, 0, 5, true) == 0);
    free(s);
    auto plan = [&](u32 first, u32 number, u32 cap, std::vector<store_range_msg> *m) {
      std::vector<std::vector<u8>> qs = {make_query(chain, first, number, {})};
      const answers A = reply(D, chain, qs, cap);
      m->clear();
      for (size_t j = 0; j + 1 < A.msg_off.size(); j++) {
        const u8 *b = &A.bytes[A.msg_off[j]];
        m->push_back(store_range_msg{store_be32(b + 34), store_be32(b + 38), 0, (store_be16(b + 43) - 1) / 8, b[42], 0, 0});
      }
      return A;
    };
    std::vector<store_range_msg> m;
    plan(0, 0xFFFFFFFFu, 0, &m);
    CHECK(m.size() == 1 && m[0].n == 7 && m[0].blocks == 0xFFFFFFFFu && m[0].final == 1);
    plan(0, 0, 0, &m);
    CHECK(m.size() == 1 && m[0].n == 0 && m[0].blocks == 0 && m[0].final == 1);
    plan(11, 9, 0, &m);   // between the blocks
    CHECK(m.size() == 1 && m[0].n == 0 && m[0].first == 11 && m[0].blocks == 9 && m[0].final == 1);
    plan(0, 100, 16, &m);   // limit 2: 10 | 20 20 (the block is broken: 0 blocks) | 20 21 (the rest fits)
    CHECK(m.size() == 3 && m[0].n == 1 && m[0].first == 0 && m[0].blocks == 20 && m[1].n == 2 && m[1].first == 20 && m[1].blocks == 0 && m[2].n == 2 &&
          m[2].first == 20 && m[2].blocks == 80 && m[2].final == 1 && !m[0].final && !m[1].final);
    plan(20, 0xFFFFFFF0u, 8, &m);   // limit 1, first + number overflows: 6 replies of one entry, blocks 20 and 0xFFFFFF broken
    CHECK(m.size() == 6 && m[5].final == 1 && m[5].first + m[5].blocks == 0xFFFFFFFFu);
    u64 sum = 0;
    for (auto &x : m) sum += x.blocks;
    CHECK(sum == 0xFFFFFFFFu - 20);
    std::vector<std::vector<u8>> qs = {make_query(other, 3, 4, {1, 1, 3}), make_query(chain, 3, 4, {2, 0}), make_query(chain, 10, 11, {1, 1, 3})};
    const answers A = reply(D, chain, qs, 0);
    CHECK(A.first == (std::vector<u64>{0, 1, 1, 2}) && A.msg_off[1] == 45 && A.status == (std::vector<int8_t>{1, -1, 0}));
    CHECK(A.bytes[42] == 0 && A.bytes[43] == 0 && A.bytes[44] == 0 && !memcmp(&A.bytes[2], other, 32) && store_be32(&A.bytes[34]) == 3 && store_be32(&A.bytes[38]) == 4);
    CHECK(A.msg_off[2] - 45 == 46 + 8 * 4 + 3 + 8 * 4 + 2 + 8 * 4);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

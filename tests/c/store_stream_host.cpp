// Host build of lightning_amd/csrc/store_stream.h under AddressSanitizer / UBSan (tests/test_store_stream_host.py).
// Arguments IMAGE OFFSETS VERDICTS FILTERS CHAIN PEERS OUT: the stream index of the image file (OFFSETS: one u64 per record, or "-": the
// offsets of the header walk; VERDICTS: one byte per record, or "-"), built with the functions the kernels run, the records visited in file
// order, in reverse and in a scrambled order -- the three must agree; then lamd_timestamp_filter_reply_batch's stages over the filters of
// FILTERS (u32 count, then u32 length + bytes per filter, little-endian) for the 32-byte chain hash in CHAIN and the peers of PEERS (u32 now,
// then per peer u64 cursor_in, i64 budget), the peers and the lanes of every tile visited in the three orders -- which must agree --, and the
// output written at all four alignments -- which must agree too.  OUT.srec, OUT.sts, OUT.slen, OUT.spos, OUT.pmax (u32), OUT.counters (7 x
// u64: streamable, deleted, dying, type, verdict, frame, bytes), OUT.status, OUT.cursor (u64), OUT.done (u8), OUT.first, OUT.msgoff (u64),
// OUT.msgrec (u32) and OUT.bytes are written for the caller to compare with its model.  Every buffer handed over is a heap block of
// EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "store_stream.h"

using namespace lamd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static u64 rnd_state = 0x3456789ull;
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

struct stream_index {
  std::vector<u64> off;
  std::vector<u32> srec, sts, slen, spos, pmax;
  u64 counters[7] = {0, 0, 0, 0, 0, 0, 0};
  bool operator==(const stream_index &o) const {
    return srec == o.srec && sts == o.sts && slen == o.slen && spos == o.spos && pmax == o.pmax && !memcmp(counters, o.counters, sizeof counters);
  }
};
// lamd_gossip_store_stream_build's stages, the records visited in the order `how`
static stream_index build(const u8 *store, size_t len, const std::vector<u64> &offs, const std::vector<int8_t> *verdict, int how) {
  stream_index X;
  X.off = offs;
  const u32 n = (u32)offs.size();
  u64 *off = block_of(offs);
  int8_t *v = verdict ? block_of(*verdict) : nullptr;
  u32 *flag = block<u32>((size_t)n + 1, 0xEE), *hts = block<u32>(n, 0xEE), *tts = block<u32>(n, 0xEE), *tlen = block<u32>(n, 0xEE);
  u64 cls_count[STORE_STREAM_CLASSES] = {0, 0, 0, 0, 0, 0};
  // k_ts_flag
  for (u32 i : visit_order(n + 1, how)) {
    if (i == n) { flag[n] = 0; continue; }
    const u32 cls = store_stream_class(store, len, off, v, i, &hts[i], &tts[i], &tlen[i]);
    flag[i] = cls == STORE_STREAM_OK;
    cls_count[cls]++;
    X.counters[6] += tlen[i];
  }
  X.counters[0] = cls_count[STORE_STREAM_OK];
  X.counters[1] = cls_count[STORE_STREAM_DELETED];
  X.counters[2] = cls_count[STORE_STREAM_DYING];
  X.counters[3] = cls_count[STORE_STREAM_TYPE];
  X.counters[4] = cls_count[STORE_STREAM_VERDICT];
  X.counters[5] = cls_count[STORE_STREAM_FRAME];
  // the scans
  u32 *spos = block<u32>((size_t)n + 1, 0xEE), *pmax = block<u32>(n, 0xEE);
  for (u32 i = 0, run = 0, mx = 0; i <= n; i++) {
    spos[i] = run;
    run += flag[i];
    if (i < n) pmax[i] = mx = hts[i] > mx ? hts[i] : mx;
  }
  // k_ts_compact
  const u32 count = spos[n];
  u32 *srec = block<u32>(count, 0xEE), *sts = block<u32>(count, 0xEE), *slen = block<u32>(count, 0xEE);
  for (u32 i : visit_order(n, how)) {
    if (!flag[i]) continue;
    srec[spos[i]] = i;
    sts[spos[i]] = tts[i];
    slen[spos[i]] = tlen[i];
  }
  X.srec.assign(srec, srec + count);
  X.sts.assign(sts, sts + count);
  X.slen.assign(slen, slen + count);
  X.spos.assign(spos, spos + n + 1);
  X.pmax.assign(pmax, pmax + n);
  for (void *p : {(void *)off, (void *)v, (void *)flag, (void *)hts, (void *)tts, (void *)tlen, (void *)spos, (void *)pmax, (void *)srec, (void *)sts, (void *)slen}) free(p);
  return X;
}

struct result {
  std::vector<int8_t> status;
  std::vector<u64> cursor, first, msg_off;
  std::vector<u8> done, bytes;
  std::vector<u32> msg_rec;
  bool operator==(const result &o) const {
    return status == o.status && cursor == o.cursor && first == o.first && msg_off == o.msg_off && done == o.done && bytes == o.bytes && msg_rec == o.msg_rec;
  }
};
struct peer_out { u32 msgs; u64 bytes, cursor; u8 done; };
// k_tf_select for one peer: the tiles in order, the lanes of a tile in the order `how`.  msg_off / msg_rec nullptr: the counting pass.
static peer_out select_one(const store_tf_index &x, const store_tf_peer &pe, u32 now, int how, u64 m0, u64 b0, u64 n_total, u64 *msg_off, u32 *msg_rec) {
  peer_out r{0, 0, pe.cursor, 0};
  if (pe.status != STORE_TF_STREAMED) return r;
  u64 cur = store_tf_start(x, pe, now), bytes = 0;
  CHECK(cur <= x.n_stream);
  u32 msgs = 0;
  u8 fin = 0;
  if (pe.budget >= 0) {
    for (;;) {
      if (cur >= x.n_stream) { cur = x.n_stream; fin = 1; break; }
      bool pass[64];
      u32 len[64], incl[64];
      for (u32 lane : visit_order(64, how)) {
        const u64 k = cur + lane;
        const bool in = k < x.n_stream;
        len[lane] = in ? x.slen[k] : 0;
        pass[lane] = in && store_tf_pass(x.sts[k], pe.min, pe.max);
      }
      u64 pm = 0, sm = 0;
      for (u32 lane = 0, run = 0; lane < 64; lane++) incl[lane] = run += pass[lane] ? len[lane] : 0;   // (the wave's scan)
      for (u32 lane : visit_order(64, how)) {
        pm |= (u64)pass[lane] << lane;
        sm |= (u64)store_tf_stops(pass[lane], bytes, incl[lane], pe.budget) << lane;
      }
      const u64 take = store_tf_taken(pm, sm);
      if (msg_off)
        for (u32 lane : visit_order(64, how)) {
          if (!((take >> lane) & 1)) continue;
          const u64 slot = m0 + msgs + (u32)__builtin_popcountll(take & ((1ull << lane) - 1ull));
          CHECK(slot < n_total);
          msg_rec[slot] = x.srec[cur + lane];
          msg_off[slot] = b0 + bytes + incl[lane] - len[lane];
        }
      msgs += (u32)__builtin_popcountll(take);
      const u32 last = sm ? store_tf_first_lane(sm) : 63u;
      bytes += incl[last];
      if (sm) { cur += last + 1; break; }
      cur += 64;
    }
  }
  return peer_out{msgs, bytes, cur, fin};
}
// the stages of lamd_timestamp_filter_reply_batch, the peers visited in the order `how`
static result reply(const stream_index &X, const u8 *store, size_t len, const u8 *chain32, const std::vector<std::vector<u8>> &filters, u32 now,
                    const std::vector<u64> &cursors, const std::vector<int64_t> &budgets, int how) {
  result A;
  const u32 np = (u32)filters.size();
  std::vector<store_tf_peer> peersv(np);
  A.status.resize(np);
  for (u32 p = 0; p < np; p++) {
    u8 *one = block_of(filters[p]);   // a block of its own: the parser reads [f, f + len) only
    const store_tf_filter f = store_tf_parse(one, filters[p].size(), chain32);
    free(one);
    peersv[p] = store_tf_peer{f.status, f.min, f.max, f.rule, cursors[p], budgets[p]};
    A.status[p] = (int8_t)f.status;
  }
  u64 *off = block_of(X.off);
  u32 *srec = block_of(X.srec), *sts = block_of(X.sts), *slen = block_of(X.slen), *spos = block_of(X.spos), *pmax = block_of(X.pmax);
  store_tf_peer *peers = block_of(peersv);
  const store_tf_index x{srec, sts, slen, spos, pmax, (u32)X.pmax.size(), (u32)X.srec.size()};
  // the counting pass, k_range_scan
  std::vector<peer_out> po(np);
  for (u32 p : visit_order(np, how)) po[p] = select_one(x, peers[p], now, how, 0, 0, 0, nullptr, nullptr);
  u64 *msg_first = block<u64>((size_t)np + 1, 0), *byte_first = block<u64>((size_t)np + 1, 0);
  for (u32 p = 0; p < np; p++) {
    msg_first[p + 1] = msg_first[p] + po[p].msgs;
    byte_first[p + 1] = byte_first[p] + po[p].bytes;
    A.cursor.push_back(po[p].cursor);
    A.done.push_back(po[p].done);
  }
  // the writing pass
  const u32 n_msgs = (u32)msg_first[np];
  const u64 total = byte_first[np];
  u64 *msg_off = block<u64>((size_t)n_msgs + 1, 0xEE);
  u32 *msg_rec = block<u32>(n_msgs, 0xEE);
  for (u32 p : visit_order(np, how)) {
    const peer_out again = select_one(x, peers[p], now, how, msg_first[p], byte_first[p], n_msgs, msg_off, msg_rec);
    CHECK(again.msgs == po[p].msgs && again.bytes == po[p].bytes && again.cursor == po[p].cursor && again.done == po[p].done);
  }
  msg_off[n_msgs] = total;
  for (u32 j = 0; j < n_msgs; j++) CHECK(msg_off[j] < msg_off[j + 1]);
  // k_sq_encode at the four alignments, with a directory that holds the image alone
  const store_sq_dir d{store, len, off, (u32)X.off.size(), nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0};
  const store_sq_out o{msg_off, msg_rec, n_msgs, msg_first, np, nullptr, nullptr, nullptr};
  for (u32 mis = 0; mis < 4 && n_msgs; mis++) {
    u8 *raw = block<u8>((size_t)total + 8, 0xEE), *out = raw + ((4 - ((uintptr_t)raw & 3)) & 3) + mis;
    const u64 words = (total + mis + 3) / 4;
    for (u64 k : visit_order((u32)words, how)) store_sq_word(d, o, out, total, mis, k);
    for (u8 *p = raw; p < out; p++) CHECK(*p == 0xEE);
    for (u8 *p = out + total; p < raw + total + 8; p++) CHECK(*p == 0xEE);
    if (mis == 0) A.bytes.assign(out, out + total);
    else CHECK(!memcmp(A.bytes.data(), out, total));
    free(raw);
  }
  A.first.assign(msg_first, msg_first + np + 1);
  A.msg_off.assign(msg_off, msg_off + n_msgs + 1);
  A.msg_rec.assign(msg_rec, msg_rec + n_msgs);
  for (void *p : {(void *)off, (void *)srec, (void *)sts, (void *)slen, (void *)spos, (void *)pmax, (void *)peers, (void *)msg_first, (void *)byte_first, (void *)msg_off,
                  (void *)msg_rec})
    free(p);
  return A;
}

static std::vector<u8> slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  std::vector<u8> v;
  u8 buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
template <class T> static void dump(const std::string &path, const T *p, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, sizeof(T), n, f) != n)) { perror(path.c_str()); exit(2); }
  fclose(f);
}

int main(int argc, char **argv) {
  if (argc != 8) { printf("usage: %s IMAGE OFFSETS|- VERDICTS|- FILTERS CHAIN PEERS OUT\n", argv[0]); return 2; }
  const std::vector<u8> file = slurp(argv[1]);
  u8 *store = block_of(file);
  std::vector<u64> offs;
  if (strcmp(argv[2], "-") != 0) {
    const std::vector<u8> raw = slurp(argv[2]);
    offs.resize(raw.size() / 8);
    if (!offs.empty()) memcpy(offs.data(), raw.data(), 8 * offs.size());
  } else {
    lamd_store_summary s;
    CHECK(store_walk(store, file.size(), &s, [&](size_t, u64 off, const store_hdr &, u32) { offs.push_back(off); }));
  }
  std::vector<int8_t> verdict;
  const bool have_verdict = strcmp(argv[3], "-") != 0;
  if (have_verdict) {
    const std::vector<u8> raw = slurp(argv[3]);
    verdict.assign(raw.begin(), raw.end());
    if (verdict.size() != offs.size()) { printf("%zu verdicts for %zu records\n", verdict.size(), offs.size()); return 2; }
  }
  const stream_index X = build(store, file.size(), offs, have_verdict ? &verdict : nullptr, 0);
  for (int how = 1; how < 3; how++) CHECK(build(store, file.size(), offs, have_verdict ? &verdict : nullptr, how) == X);
  for (size_t i = 1; i < X.pmax.size(); i++) CHECK(X.pmax[i - 1] <= X.pmax[i]);
  const std::vector<u8> raw = slurp(argv[4]), chain = slurp(argv[5]), praw = slurp(argv[6]);
  if (chain.size() != 32) { printf("the chain hash has 32 bytes\n"); return 2; }
  std::vector<std::vector<u8>> filters;
  size_t pos = 4;
  u32 count = 0;
  if (raw.size() >= 4) memcpy(&count, raw.data(), 4);
  for (u32 k = 0; k < count; k++) {
    u32 l = 0;
    if (raw.size() - pos < 4) { printf("bad filter file\n"); return 2; }
    memcpy(&l, raw.data() + pos, 4);
    pos += 4;
    if (raw.size() - pos < l) { printf("bad filter file\n"); return 2; }
    filters.emplace_back(raw.begin() + pos, raw.begin() + pos + l);
    pos += l;
  }
  if (praw.size() != 4 + 16 * (size_t)count) { printf("bad peer file\n"); return 2; }
  u32 now = 0;
  memcpy(&now, praw.data(), 4);
  std::vector<u64> cursors(count);
  std::vector<int64_t> budgets(count);
  for (u32 k = 0; k < count; k++) {
    memcpy(&cursors[k], praw.data() + 4 + 16 * (size_t)k, 8);
    memcpy(&budgets[k], praw.data() + 12 + 16 * (size_t)k, 8);
  }
  u8 *chain32 = block_of(chain);
  const result A = reply(X, store, file.size(), chain32, filters, now, cursors, budgets, 0);
  for (int how = 1; how < 3; how++) CHECK(reply(X, store, file.size(), chain32, filters, now, cursors, budgets, how) == A);
  const std::string out = argv[7];
  dump(out + ".srec", X.srec.data(), X.srec.size());
  dump(out + ".sts", X.sts.data(), X.sts.size());
  dump(out + ".slen", X.slen.data(), X.slen.size());
  dump(out + ".spos", X.spos.data(), X.spos.size());
  dump(out + ".pmax", X.pmax.data(), X.pmax.size());
  dump(out + ".counters", X.counters, 7);
  dump(out + ".status", A.status.data(), A.status.size());
  dump(out + ".cursor", A.cursor.data(), A.cursor.size());
  dump(out + ".done", A.done.data(), A.done.size());
  dump(out + ".first", A.first.data(), A.first.size());
  dump(out + ".msgoff", A.msg_off.data(), A.msg_off.size());
  dump(out + ".msgrec", A.msg_rec.data(), A.msg_rec.size());
  dump(out + ".bytes", A.bytes.data(), A.bytes.size());
  free(store);
  free(chain32);
  if (failures) printf("%d checks failed\n", failures);
  else printf("ok\n");
  return failures ? 1 : 0;
}

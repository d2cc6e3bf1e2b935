// Host build of lightning_amd/csrc/store_query.h under AddressSanitizer / UBSan (tests/test_store_query_host.py).
// Arguments IMAGE VERDICTS QUERIES CHAIN OUT: the digest of the image file (IMAGE "-": no image, an empty directory; VERDICTS: one byte per
// record, or "-") and its directory, built with the functions the kernels run, the records visited in file order, in reverse and in a scrambled
// order -- the three must agree; then lamd_short_channel_ids_reply_batch's stages over the queries of QUERIES (u32 count, then u32 length +
// bytes per query, little-endian) for the 32-byte chain hash in CHAIN (an EMPTY file: every query is parsed against its own chain_hash
// bytes), the occurrences visited in the three orders -- which must agree --, and the output written at all four alignments -- which must agree
// too.  OUT.nodes (33 bytes each), OUT.nfirst, OUT.nann, OUT.barerec, OUT.ranks (u32), OUT.counters (5 x u64: nodes, announced, no node, in
// front, short), OUT.status, OUT.perq (4 x u32 per query), OUT.first, OUT.msgoff (u64), OUT.msgrec (u32) and OUT.bytes are written for the
// caller to compare with its model.  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_query.h"

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

// the directory with everything it refers to: plain vectors for the comparison of the three orders, heap blocks for the responder
struct directory {
  std::vector<u64> off, scid, bare, node_off;
  std::vector<u32> ent_rec, bare_rec, chan_rank, node_first, node_nann;
  u64 counters[5] = {0, 0, 0, 0, 0};
  bool operator==(const directory &o) const {
    return scid == o.scid && bare == o.bare && node_off == o.node_off && ent_rec == o.ent_rec && bare_rec == o.bare_rec && chan_rank == o.chan_rank &&
           node_first == o.node_first && node_nann == o.node_nann && !memcmp(counters, o.counters, sizeof counters);
  }
};
// lamd_gossip_store_digest_build's stages (store_digest.h), then lamd_gossip_store_directory_build's, each over the records in the order `how`
static directory build(const u8 *store, size_t len, const std::vector<u64> &offs, const std::vector<int8_t> *verdict, int how) {
  directory D;
  D.off = offs;
  const u32 n = (u32)offs.size();
  if (n == 0) return D;
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
    D.ent_rec.insert(D.ent_rec.end(), rec, rec + 3);
  }
  // k_dir_bare
  const u32 count = (u32)D.scid.size(), nbare = (u32)D.bare.size(), channels = count + nbare, m = 2 * channels;
  u64 *bare = block_of(D.bare);
  u32 *bare_rec = block<u32>(nbare, 0xFF);
  for (u32 i : visit_order(n, how)) store_dir_bare_one(store, len, off, v, i, bare, nbare, bare_rec);
  D.bare_rec.assign(bare_rec, bare_rec + nbare);
  // k_dir_cand
  u64 *cand_off = block<u64>(m, 0);
  u32 *cand_rec = block<u32>(m, 0), *perm = block<u32>(m, 0), *perm2 = block<u32>(m, 0);
  u32 valid = 0;
  for (u32 c : visit_order(channels, how)) {
    const u32 a = c < count ? D.ent_rec[3 * (size_t)c] : bare_rec[c - count];
    u64 idoff = 0;
    const bool ok = a < n && store_dir_cann_ids(store, len, off[a], &idoff);
    for (u32 k = 0; k < 2; k++) {
      cand_off[2 * c + k] = ok ? idoff + 33 * k : STORE_DIR_NO_ID;
      cand_rec[2 * c + k] = a;
      perm[2 * c + k] = 2 * c + k;
    }
    valid += ok ? 2 : 0;
  }
  // the LSD sort: a stable counting of each pass' keys (std::stable_sort stands for rocPRIM's radix sort)
  for (u32 pass = 0; pass < STORE_DIR_PASSES; pass++) {
    std::vector<std::pair<u64, u32>> kv(m);
    for (u32 j = 0; j < m; j++) kv[j] = {store_dir_pass_key(store, cand_off[perm[j]], pass), perm[j]};
    std::stable_sort(kv.begin(), kv.end(), [](const std::pair<u64, u32> &a, const std::pair<u64, u32> &b) { return a.first < b.first; });
    for (u32 j = 0; j < m; j++) perm2[j] = kv[j].second;
    std::swap(perm, perm2);
  }
  // k_dir_heads, the scan, k_dir_merge
  u32 *head = block<u32>(m, 0), *pos = block<u32>(m, 0), *chan_rank = block<u32>(m, 0xFF), *node_first = block<u32>(m, 0xFF), *node_nann = block<u32>(m, 0);
  u64 *node_off = block<u64>(m, 0);
  for (u32 j : visit_order(m, how)) head[j] = store_dir_head(store, cand_off, perm, valid, j);
  for (u32 j = 0, run = 0; j < m; j++) pos[j] = run += head[j];
  const u32 nodes = valid ? pos[valid - 1] : 0;
  for (u32 j : visit_order(valid, how)) {
    const u32 r = pos[j] - 1, c = perm[j];
    chan_rank[c] = r;
    if (head[j]) node_off[r] = cand_off[c];
    store_dir_min(&node_first[r], cand_rec[c]);
  }
  for (u32 r = 1; r < nodes; r++) CHECK(store_dir_idcmp(store + node_off[r - 1], store + node_off[r]) < 0);
  // k_dir_nann
  for (u32 i : visit_order(n, how)) {
    const u32 r = store_dir_nann_one(store, len, off, v, i, node_off, node_first, nodes, node_nann);
    if (r >= STORE_DIR_NANN_NO_NODE) D.counters[r]++;
  }
  D.counters[0] = nodes;
  for (u32 r = 0; r < nodes; r++) D.counters[1] += node_nann[r] != 0;
  D.node_off.assign(node_off, node_off + nodes);
  D.chan_rank.assign(chan_rank, chan_rank + m);
  D.node_first.assign(node_first, node_first + nodes);
  D.node_nann.assign(node_nann, node_nann + nodes);
  for (void *p : {(void *)off, (void *)v, (void *)keys, (void *)vals, (void *)slot, (void *)bare, (void *)bare_rec, (void *)cand_off, (void *)cand_rec, (void *)perm,
                  (void *)perm2, (void *)head, (void *)pos, (void *)chan_rank, (void *)node_first, (void *)node_nann, (void *)node_off})
    free(p);
  return D;
}

struct result {
  std::vector<int8_t> status;
  std::vector<u32> per_query, msg_rec;
  std::vector<u64> first, msg_off;
  std::vector<u8> bytes;
  bool operator==(const result &o) const {
    return status == o.status && per_query == o.per_query && msg_rec == o.msg_rec && first == o.first && msg_off == o.msg_off && bytes == o.bytes;
  }
};
// the stages of lamd_short_channel_ids_reply_batch, the occurrences visited in the order `how`
static result reply(const directory &D, const u8 *store, size_t len, const u8 *chain32, const std::vector<std::vector<u8>> &queries, int how) {
  result A;
  const u32 nq = (u32)queries.size();
  std::vector<u64> qoffv(nq + 1, 0), firstv(nq + 1, 0), scidatv(nq, 0);
  std::vector<u8> batchv;
  for (u32 q = 0; q < nq; q++) {
    batchv.insert(batchv.end(), queries[q].begin(), queries[q].end());
    qoffv[q + 1] = batchv.size();
  }
  u8 *batch = block_of(batchv);
  std::vector<store_sq_query> pq(nq);
  A.status.resize(nq);
  for (u32 q = 0; q < nq; q++) {
    u8 *one = block_of(queries[q]);   // a block of its own: the parser reads [q, q + len) only
    static const u8 zero32[32] = {0};
    pq[q] = store_sq_parse(one, queries[q].size(), qoffv[q], chain32 ? chain32 : queries[q].size() >= 34 ? one + 2 : zero32);
    free(one);
    A.status[q] = (int8_t)pq[q].status;
    firstv[q + 1] = firstv[q] + pq[q].n;
    scidatv[q] = pq[q].scid_at;
  }
  const u32 S = (u32)firstv[nq], K = 2 * S, I1 = 3 * S + 1;
  u8 *flags = block<u8>(S, 0xEE);
  for (u32 q = 0; q < nq; q++)
    if (pq[q].n) store_sq_flags(batch + qoffv[q], pq[q], flags + firstv[q]);
  u64 *off = block_of(D.off), *scid = block_of(D.scid), *bare = block_of(D.bare), *first = block_of(firstv), *qoff = block_of(qoffv);
  u32 *ent_rec = block_of(D.ent_rec), *bare_rec = block_of(D.bare_rec), *chan_rank = block_of(D.chan_rank), *node_nann = block_of(D.node_nann);
  int8_t *status = block_of(A.status);
  const store_sq_dir d{store, len, off, (u32)D.off.size(), scid, ent_rec, (u32)D.scid.size(), bare, bare_rec, (u32)D.bare.size(), chan_rank, node_nann, (u32)D.node_nann.size()};
  // k_sq_lookup
  u32 *occ_rec = block<u32>(3 * (size_t)S, 0xEE), *icnt = block<u32>(I1, 0xEE), *ibytes = block<u32>(I1, 0xEE), *node_rec = block<u32>(K, 0xEE);
  u8 *known = block<u8>(S, 0xEE);
  std::vector<u64> nkey;
  for (u32 e : visit_order(S, how)) {
    const u32 q = store_range_locate(first, nq, e);
    CHECK(first[q] <= e && e < first[q + 1]);
    u32 rank2[2], b;
    known[e] = store_sq_lookup(d, store_be64(batch + scidatv[q] + 8 * (u64)(e - first[q])), flags[e], occ_rec + 3 * (size_t)e, &b, rank2);
    icnt[e] = 0;
    for (u32 k = 0; k < 3; k++) icnt[e] += occ_rec[3 * (size_t)e + k] != STORE_NONE;
    ibytes[e] = b;
    for (u32 k = 0; k < 2; k++)
      if (rank2[k] != STORE_NONE) nkey.push_back(((u64)q << 32) | rank2[k]);
  }
  // the sort, heads, merge; k_sq_nodes
  std::sort(nkey.begin(), nkey.end());
  u64 *nk = block_of(nkey), *uniq = block<u64>(K, 0xEE);
  u32 U = 0;
  for (u32 j = 0; j < nkey.size(); j++)
    if (store_cmp_head(nk, j)) uniq[U++] = nk[j];
  for (u32 j = 0; j <= K; j++) {
    u32 rec = STORE_NONE, l = 0;
    if (j < U) {
      const u32 rank = (u32)uniq[j], nn = rank < d.nodes ? d.node_nann[rank] : 0;
      l = nn ? store_sq_msg_len(d, nn - 1) : 0;
      if (l) rec = nn - 1;
    }
    if (j < K) node_rec[j] = rec;
    icnt[S + j] = rec != STORE_NONE;
    ibytes[S + j] = l;
  }
  // the scans, k_sq_per_query, k_range_scan
  u64 *mscan = block<u64>(I1, 0), *bscan = block<u64>(I1, 0), *msg_first = block<u64>(nq + 1, 0), *byte_first = block<u64>(nq + 1, 0);
  for (u32 i = 0; i + 1 < I1; i++) { mscan[i + 1] = mscan[i] + icnt[i]; bscan[i + 1] = bscan[i] + ibytes[i]; }
  std::vector<u32> qlo(nq, 0);
  A.per_query.assign(4 * (size_t)nq, 0);
  for (u32 q = 0; q < nq; q++) {
    const u64 a = first[q], b = first[q + 1];
    u64 msgs = 0, bytes = 0;
    if (status[q] == STORE_SQ_ANSWERED) {
      const u32 hi = store_sq_lower(uniq, U, ((u64)q + 1) << 32), lo = store_sq_lower(uniq, U, (u64)q << 32);
      qlo[q] = lo;
      u32 *p = &A.per_query[4 * (size_t)q];
      p[0] = (u32)(b - a);
      for (u64 e = a; e < b; e++) p[1] += known[e];
      p[2] = (u32)(mscan[b] - mscan[a]);
      p[3] = (u32)(mscan[S + hi] - mscan[S + lo]);
      msgs = p[2] + p[3] + 1;
      bytes = (bscan[b] - bscan[a]) + (bscan[S + hi] - bscan[S + lo]) + STORE_SQ_END_BYTES;
    } else if (status[q] == STORE_SQ_FOREIGN) {
      msgs = 1;
      bytes = STORE_SQ_END_BYTES;
    }
    msg_first[q + 1] = msg_first[q] + msgs;
    byte_first[q + 1] = byte_first[q] + bytes;
  }
  // k_sq_plan
  const u32 n_msgs = (u32)msg_first[nq];
  const u64 total = byte_first[nq];
  u64 *msg_off = block<u64>((size_t)n_msgs + 1, 0xEE);
  u32 *msg_rec = block<u32>(n_msgs, 0xEE);
  for (u32 i : visit_order(S, how)) {
    const u32 q = store_range_locate(first, nq, i);
    const u64 a = first[q];
    u64 mi = msg_first[q] + (mscan[i] - mscan[a]), bo = byte_first[q] + (bscan[i] - bscan[a]);
    for (u32 k = 0; k < 3; k++) {
      const u32 r = occ_rec[3 * (size_t)i + k];
      if (r == STORE_NONE) continue;
      msg_off[mi] = bo;
      msg_rec[mi++] = r;
      bo += store_sq_msg_len(d, r);
    }
  }
  for (u32 j : visit_order(U, how)) {
    if (node_rec[j] == STORE_NONE) continue;
    const u32 q = (u32)(uniq[j] >> 32);
    const u64 a = first[q], b = first[q + 1], lo = qlo[q];
    const u64 mi = msg_first[q] + (mscan[b] - mscan[a]) + (mscan[S + j] - mscan[S + lo]);
    msg_off[mi] = byte_first[q] + (bscan[b] - bscan[a]) + (bscan[S + j] - bscan[S + lo]);
    msg_rec[mi] = node_rec[j];
  }
  for (u32 q = 0; q < nq; q++)
    if (status[q] == STORE_SQ_ANSWERED || status[q] == STORE_SQ_FOREIGN) {
      msg_off[msg_first[q + 1] - 1] = byte_first[q + 1] - STORE_SQ_END_BYTES;
      msg_rec[msg_first[q + 1] - 1] = STORE_NONE;
    }
  msg_off[n_msgs] = total;
  for (u32 j = 0; j < n_msgs; j++) CHECK(msg_off[j] < msg_off[j + 1]);
  // k_sq_encode at the four alignments
  const store_sq_out o{msg_off, msg_rec, n_msgs, msg_first, nq, batch, qoff, status};
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
  A.first.assign(msg_first, msg_first + nq + 1);
  A.msg_off.assign(msg_off, msg_off + n_msgs + 1);
  A.msg_rec.assign(msg_rec, msg_rec + n_msgs);
  for (void *p : {(void *)batch, (void *)flags, (void *)off, (void *)scid, (void *)bare, (void *)first, (void *)qoff, (void *)ent_rec, (void *)bare_rec, (void *)chan_rank,
                  (void *)node_nann, (void *)status, (void *)occ_rec, (void *)icnt, (void *)ibytes, (void *)node_rec, (void *)known, (void *)nk, (void *)uniq, (void *)mscan,
                  (void *)bscan, (void *)msg_first, (void *)byte_first, (void *)msg_off, (void *)msg_rec})
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
  if (argc != 6) { printf("usage: %s IMAGE|- VERDICTS|- QUERIES CHAIN OUT\n", argv[0]); return 2; }
  const bool have_image = strcmp(argv[1], "-") != 0;
  const std::vector<u8> file = have_image ? slurp(argv[1]) : std::vector<u8>();
  u8 *store = block_of(file);
  std::vector<u64> offs;
  if (have_image) {
    lamd_store_summary s;
    CHECK(store_walk(store, file.size(), &s, [&](size_t, u64 off, const store_hdr &, u32) { offs.push_back(off); }));
  }
  std::vector<int8_t> verdict;
  const bool have_verdict = strcmp(argv[2], "-") != 0;
  if (have_verdict) {
    const std::vector<u8> raw = slurp(argv[2]);
    verdict.assign(raw.begin(), raw.end());
    if (verdict.size() != offs.size()) { printf("%zu verdicts for %zu records\n", verdict.size(), offs.size()); return 2; }
  }
  const directory D = build(store, file.size(), offs, have_verdict ? &verdict : nullptr, 0);
  for (int how = 1; how < 3; how++) CHECK(build(store, file.size(), offs, have_verdict ? &verdict : nullptr, how) == D);
  const std::vector<u8> raw = slurp(argv[3]), chain = slurp(argv[4]);
  if (!chain.empty() && chain.size() != 32) { printf("the chain hash has 32 bytes\n"); return 2; }
  std::vector<std::vector<u8>> queries;
  size_t pos = 4;
  u32 count = 0;
  if (raw.size() >= 4) memcpy(&count, raw.data(), 4);
  for (u32 k = 0; k < count; k++) {
    u32 l = 0;
    if (raw.size() - pos < 4) { printf("bad query file\n"); return 2; }
    memcpy(&l, raw.data() + pos, 4);
    pos += 4;
    if (raw.size() - pos < l) { printf("bad query file\n"); return 2; }
    queries.emplace_back(raw.begin() + pos, raw.begin() + pos + l);
    pos += l;
  }
  u8 *chain32 = chain.empty() ? nullptr : block_of(chain);
  const result A = reply(D, store, file.size(), chain32, queries, 0);
  for (int how = 1; how < 3; how++) CHECK(reply(D, store, file.size(), chain32, queries, how) == A);
  const std::string out = argv[5];
  std::vector<u8> ids;
  for (u64 o : D.node_off) ids.insert(ids.end(), store + o, store + o + 33);
  std::vector<u32> nann(D.node_nann);
  for (u32 &x : nann) x -= 1;
  dump(out + ".nodes", ids.data(), ids.size());
  dump(out + ".nfirst", D.node_first.data(), D.node_first.size());
  dump(out + ".nann", nann.data(), nann.size());
  dump(out + ".barerec", D.bare_rec.data(), D.bare_rec.size());
  dump(out + ".ranks", D.chan_rank.data(), D.chan_rank.size());
  dump(out + ".counters", D.counters, 5);
  dump(out + ".status", A.status.data(), A.status.size());
  dump(out + ".perq", A.per_query.data(), A.per_query.size());
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

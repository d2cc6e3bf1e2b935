// Host build of lightning_amd/csrc/store_nodes.h under AddressSanitizer / UBSan (tests/test_store_nodes_host.py).
// Arguments IMAGE VIEW BATCH SIGV OUT.  IMAGE: the store image.  VIEW (little-endian): u32 n_rec, count, nbare, nodes; u64 rec_off[n_rec];
// u32 ent_rec[3 count]; u32 bare_rec[nbare]; u32 chan_rank[2 (count + nbare)]; u64 node_off[nodes]; u32 node_nann[nodes] (index + 1, 0: none) --
// what the directory holds.  BATCH: u32 pending, u32 n, then per message u32 length and the bytes.  SIGV: one int8 per MESSAGE, the verdict of
// the signature batch for that message under its own node_id (the stages on both sides of the signature batch are what is under test; which
// messages this program asks about is written to OUT.checked for the caller to compare).  lamd_node_announcement_receive_batch's stages run
// with the functions the kernels run, the channels, the messages, the rows and the sorted positions visited in arrival order, in reverse and
// in a scrambled order -- the three must agree --, and the output is written at all four alignments -- which must agree too.  OUT.status (i8),
// OUT.flags (u8), OUT.node (u32), OUT.checked (u8), OUT.addmsg (u32), OUT.addoff (u64), OUT.del (u32), OUT.bytes, OUT.rows (u32: the signature
// rows).  Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_nodes.h"

using namespace lamd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static u64 rnd_state = 0x5678912ull;
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
template <class T> static void write_file(const std::string &path, const std::vector<T> &v) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) { printf("cannot write %s\n", path.c_str()); exit(2); }
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
  fclose(f);
}
struct reader {
  const std::vector<u8> &b;
  size_t at = 0;
  template <class T> T get() {
    T v;
    if (at + sizeof(T) > b.size()) { printf("input file too short\n"); exit(2); }
    memcpy(&v, b.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  template <class T> std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    for (size_t k = 0; k < n; k++) v[k] = get<T>();
    return v;
  }
};

struct result {
  std::vector<int8_t> status;
  std::vector<u8> flags, checked, bytes;
  std::vector<u32> node, add_msg, del;
  std::vector<u64> add_off;
  u32 rows = 0;
  bool operator==(const result &o) const {
    return status == o.status && flags == o.flags && checked == o.checked && bytes == o.bytes && node == o.node && add_msg == o.add_msg && del == o.del &&
           add_off == o.add_off && rows == o.rows;
  }
};

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: IMAGE VIEW BATCH SIGV OUT\n"); return 2; }
  const std::vector<u8> image = read_file(argv[1]), view_b = read_file(argv[2]), batch_b = read_file(argv[3]), sigv_b = read_file(argv[4]);
  reader vr{view_b};
  const u32 n_rec = vr.get<u32>(), count = vr.get<u32>(), nbare = vr.get<u32>(), nodes = vr.get<u32>();
  u64 *rec_off = block_of(vr.take<u64>(n_rec));
  u32 *ent_rec = block_of(vr.take<u32>(3 * (size_t)count)), *bare_rec = block_of(vr.take<u32>(nbare)), *chan_rank = block_of(vr.take<u32>(2 * ((size_t)count + nbare)));
  u64 *node_off = block_of(vr.take<u64>(nodes));
  u32 *node_nann = block_of(vr.take<u32>(nodes));
  u8 *store = block_of(image);
  const store_nr_view v{store, image.size(), rec_off, n_rec, ent_rec, bare_rec, chan_rank, count, nbare, node_off, node_nann, nodes};
  reader br{batch_b};
  const u32 pending = br.get<u32>(), n = br.get<u32>();
  std::vector<u8> msgs_v;
  std::vector<u64> off_v{0};
  for (u32 i = 0; i < n; i++) {
    const u32 len = br.get<u32>();
    const std::vector<u8> m = br.take<u8>(len);
    msgs_v.insert(msgs_v.end(), m.begin(), m.end());
    off_v.push_back(msgs_v.size());
  }
  CHECK(sigv_b.size() == n);
  u8 *msgs = block_of(msgs_v);
  u64 *off = block_of(off_v);
  const store_nr_batch b{msgs, off, n, pending};
  const store_rx_batch eb{msgs, off, n, nullptr, 0, nullptr, 0};
  u32 T[4 * 256];
  store_crc_build_tables(T, 4);

  std::vector<result> runs;
  for (int how = 0; how < 3; how++) {
    result R;
    // k_nr_alive
    u8 *alive = block<u8>(nodes, 0);
    for (u32 c : visit_order(count + nbare, how)) store_nr_alive(v, c, alive);
    int8_t *status = block<int8_t>(n, 0xEE), *sigv = block<int8_t>(n, 0xEE);
    u8 *flags = block<u8>(n, 0);
    u32 *node = block<u32>(n, 0xEE), *ts = block<u32>(n, 0xEE), *row_of = block<u32>(n, 0xEE), *row_msg = block<u32>(n, 0xEE);
    u64 *start = block<u64>(n, 0), *len = block<u64>(n, 0);
    // k_nr_classify: rows in the order the messages are visited
    u32 rows = 0;
    for (u32 i : visit_order(n, how)) {
      const store_nr_msg r = store_nr_classify(v, b, i);
      status[i] = (int8_t)r.status;
      node[i] = r.node;
      ts[i] = r.ts;
      row_of[i] = STORE_NONE;
      if (r.status != STORE_NR_PENDING) continue;
      row_of[i] = rows;
      store_nr_row(b, i, rows++, start, len, row_msg);
    }
    R.rows = rows;
    R.checked.assign(n, 0);
    for (u32 r = 0; r < rows; r++) {   // the signature batch: the caller's verdict for the row's message
      const u32 i = row_msg[r];
      CHECK(start[r] == off[i] && len[r] == off[i + 1] - off[i] && row_of[i] == r);
      sigv[r] = (int8_t)sigv_b[i];
      R.checked[i] = 1;
    }
    // k_nr_settle, the stable sort, k_rx_items, the max-scan
    u64 *key = block<u64>(n, 0xEE), *skey = block<u64>(n, 0xEE), *item = block<u64>(n, 0xEE), *run = block<u64>(n, 0xEE);
    u32 *sval = block<u32>(n, 0xEE);
    for (u32 i : visit_order(n, how)) key[i] = store_nr_settle(status, node, row_of, sigv, pending, i);
    std::vector<u32> perm(n);
    for (u32 i = 0; i < n; i++) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](u32 x, u32 y) { return (u32)key[x] < (u32)key[y]; });   // the device sorts bits 0 .. 31
    for (u32 p = 0; p < n; p++) { skey[p] = key[perm[p]]; sval[p] = perm[p]; }
    for (u32 p : visit_order(n, how)) item[p] = store_rx_item(skey, sval, ts, p);
    for (u32 p = 0; p < n; p++) run[p] = p && run[p - 1] > item[p] ? run[p - 1] : item[p];
    // k_nr_resolve
    u32 *acnt = block<u32>((size_t)n + 1, 0), *abytes = block<u32>((size_t)n + 1, 0), *del_key = block<u32>(n, 0xFF);
    u32 dels = 0;
    const store_rx_sorted s{skey, sval, run, n};
    for (u32 p : visit_order(n, how)) dels += store_nr_resolve(v, b, s, ts, alive, p, status, flags, store_nr_marks{acnt, abytes, del_key});
    // the sort of the deleted records, the scans, k_nr_plan
    std::vector<u32> dsort(del_key, del_key + n);
    std::sort(dsort.begin(), dsort.end());
    u64 *apos = block<u64>((size_t)n + 1, 0xEE), *abyte = block<u64>((size_t)n + 1, 0xEE);
    u64 ra = 0, rb = 0;
    for (u32 i = 0; i <= n; i++) {
      apos[i] = ra; abyte[i] = rb;
      ra += acnt[i]; rb += abytes[i];
    }
    const u64 adds = apos[n], total = abyte[n];
    for (u32 k = 0; k < n; k++) CHECK((k < dels) == (dsort[k] != STORE_NONE));
    u32 *add_msg = block<u32>(adds, 0xEE);
    u64 *add_off = block<u64>(adds, 0xEE);
    for (u32 i : visit_order(n, how)) store_nr_plan(status, apos, abyte, adds, add_msg, add_off, i);
    // k_rx_encode, k_rx_copy at four alignments
    u8 *hdr = block<u8>(STORE_HDR * adds, 0xEE);
    for (u32 j : visit_order((u32)adds, how)) store_rx_header<4>(T, eb, flags, ts, add_msg[j], hdr + STORE_HDR * (size_t)j);
    const store_rx_out o{add_off, add_msg, (u32)adds, hdr, msgs, off};
    for (u32 mis = 0; mis < 4; mis++) {
      u8 *raw = (u8 *)aligned_alloc(4, (total + mis + 3) / 4 * 4 + 4);
      u8 *out = raw + mis;   // the words the encoder stores lie inside [out, out + total)
      memset(raw, 0xEE, (total + mis + 3) / 4 * 4 + 4);
      const u64 words = (total + mis + 3) / 4;
      if (adds)
        for (u32 k : visit_order((u32)words, how)) store_rx_word(o, out, total, mis, k);
      const std::vector<u8> got(out, out + total);
      if (mis == 0) R.bytes = got; else CHECK(got == R.bytes);
      for (u32 x = 0; x < mis; x++) CHECK(raw[x] == 0xEE);
      for (u64 x = total + mis; x < (total + mis + 3) / 4 * 4 + 4; x++) CHECK(raw[x] == 0xEE);
      free(raw);
    }
    R.status.assign(status, status + n);
    R.flags.assign(flags, flags + n);
    R.node.assign(node, node + n);
    R.add_msg.assign(add_msg, add_msg + adds);
    R.add_off.assign(add_off, add_off + adds);
    R.del.assign(dsort.begin(), dsort.begin() + dels);
    for (void *p : {(void *)alive, (void *)status, (void *)sigv, (void *)flags, (void *)node, (void *)ts, (void *)row_of, (void *)row_msg, (void *)start, (void *)len,
                    (void *)key, (void *)skey, (void *)item, (void *)run, (void *)sval, (void *)acnt, (void *)abytes, (void *)del_key, (void *)apos, (void *)abyte,
                    (void *)add_msg, (void *)add_off, (void *)hdr})
      free(p);
    runs.push_back(R);
  }
  CHECK(runs[0] == runs[1]);
  CHECK(runs[0] == runs[2]);
  const result &R = runs[0];
  const std::string out = argv[5];
  write_file(out + ".status", R.status);
  write_file(out + ".flags", R.flags);
  write_file(out + ".node", R.node);
  write_file(out + ".checked", R.checked);
  write_file(out + ".addmsg", R.add_msg);
  write_file(out + ".addoff", R.add_off);
  write_file(out + ".del", R.del);
  write_file(out + ".bytes", R.bytes);
  write_file(out + ".rows", std::vector<u32>{R.rows});
  for (void *p : {(void *)rec_off, (void *)ent_rec, (void *)bare_rec, (void *)chan_rank, (void *)node_off, (void *)node_nann, (void *)store, (void *)msgs, (void *)off}) free(p);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

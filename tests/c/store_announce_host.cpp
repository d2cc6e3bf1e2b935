// Host build of lightning_amd/csrc/store_announce.h under AddressSanitizer / UBSan (tests/test_store_announce_host.py).
//   receive DIGEST BATCH VERDICTS OUT
//     DIGEST (little-endian): u32 count, nbare; u64 scid[count]; u64 bare[nbare].  BATCH: u32 blockheight, n, n_held, n_failed; u8 chain[32];
//     u64 held[n_held]; u64 failed[n_failed]; then per message u32 length and the bytes.  VERDICTS: three bytes per MESSAGE -- the verdict the
//     signature batch would give it (int8: -1, 0, 1 .. 4) and the validity of its bitcoin_key_1 / bitcoin_key_2 (the stages on both sides of the
//     two batches are what is under test; which list a message is put on is written to OUT.list for the caller to compare).
//     OUT.status (i8), OUT.scid (u64), OUT.spk (34 bytes each), OUT.askmsg (u32), OUT.askscid (u64), OUT.list (u8), OUT.counts (u32 x 2).
//   confirm IMAGE VIEW PENDING REPLIES OUT
//     VIEW: u32 n_rec, count, nbare, nodes; u64 rec_off[n_rec]; u64 scid[count]; u64 bare[nbare]; u64 node_off[nodes]; u32 node_nann[nodes]
//     (index + 1, 0: none).  PENDING: u32 np, then per message u32 length, the bytes, 34 script bytes.  REPLIES: u32 nr, then per reply u64 scid,
//     u64 sat, u32 script length, the script.  OUT.status (i8), OUT.pend (u32), OUT.fail (u64), OUT.addreply (u32), OUT.addoff (u64), OUT.clr (u32),
//     OUT.bytes.
// The stages run with the functions the kernels run, the messages, rows, sorted positions, replies and output words visited in arrival order, in
// reverse and in a scrambled order -- the three must agree --, and the output is written at all four alignments -- which must agree too.
// Every buffer handed over is a heap block of EXACTLY its size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "store_announce.h"

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
static void free_all(std::initializer_list<void *> l) {
  for (void *p : l) free(p);
}

struct rx_result {
  std::vector<int8_t> status;
  std::vector<u64> scid, ask_scid;
  std::vector<u8> spk, list;
  std::vector<u32> ask_msg, counts;
  bool operator==(const rx_result &o) const {
    return status == o.status && scid == o.scid && ask_scid == o.ask_scid && spk == o.spk && list == o.list && ask_msg == o.ask_msg && counts == o.counts;
  }
};

static int receive(char **argv) {
  const std::vector<u8> dig_b = read_file(argv[2]), batch_b = read_file(argv[3]), ver_b = read_file(argv[4]);
  reader dr{dig_b};
  const u32 count = dr.get<u32>(), nbare = dr.get<u32>();
  u64 *dscid = block_of(dr.take<u64>(count)), *bare = block_of(dr.take<u64>(nbare));
  const store_ca_view v{dscid, count, bare, nbare};
  reader br{batch_b};
  const u32 blockheight = br.get<u32>(), n = br.get<u32>(), n_held = br.get<u32>(), n_failed = br.get<u32>();
  const std::vector<u8> chain = br.take<u8>(32);
  u64 *held = block_of(br.take<u64>(n_held)), *failed = block_of(br.take<u64>(n_failed));
  std::vector<u8> msgs_v;
  std::vector<u64> off_v{0};
  for (u32 i = 0; i < n; i++) {
    const u32 len = br.get<u32>();
    const std::vector<u8> m = br.take<u8>(len);
    msgs_v.insert(msgs_v.end(), m.begin(), m.end());
    off_v.push_back(msgs_v.size());
  }
  CHECK(ver_b.size() == 3 * (size_t)n);
  u8 *msgs = block_of(msgs_v);
  u64 *off = block_of(off_v);
  store_ca_batch b{msgs, off, n, held, n_held, failed, n_failed, blockheight, {}};
  memcpy(b.chain, chain.data(), 32);

  std::vector<rx_result> runs;
  for (int how = 0; how < 3; how++) {
    rx_result R;
    int8_t *status = block<int8_t>(n, 0xEE), *sigv = block<int8_t>(n, 0xEE);
    u64 *scid = block<u64>(n, 0xEE), *start = block<u64>(n, 0xEE), *len = block<u64>(n, 0xEE), *key = block<u64>(n, 0xEE), *skey = block<u64>(n, 0xEE);
    u32 *keyoff = block<u32>(n, 0xEE), *row_of = block<u32>(n, 0xEE), *item = block<u32>(n, 0xEE), *sval = block<u32>(n, 0xEE), *sitem = block<u32>(n, 0xEE),
        *first = block<u32>(n, 0xEE), *acnt = block<u32>((size_t)n + 1, 0);
    u8 *list = block<u8>(n, 0xEE), *keys33 = block<u8>(66 * (size_t)n, 0xEE), *keyok = block<u8>(2 * (size_t)n, 0xEE);
    // k_ca_classify: the rows of the two lists in the order the messages are visited
    u32 sigs = 0, keys = 0;
    std::vector<u32> sig_msg, key_msg;
    for (u32 i : visit_order(n, how)) {
      const store_ca_msg r = store_ca_classify(v, b, i);
      status[i] = (int8_t)r.status;
      scid[i] = r.scid;
      keyoff[i] = r.keyoff;
      list[i] = (u8)r.list;
      row_of[i] = STORE_NONE;
      if (r.list == STORE_CA_LIST_SIGNATURES) {
        row_of[i] = sigs;
        store_ca_sig_row(b, i, sigs++, start, len);
        sig_msg.push_back(i);
      } else if (r.list == STORE_CA_LIST_KEYS) {
        row_of[i] = keys;
        store_ca_key_row(b, i, r.keyoff, keys++, keys33);
        key_msg.push_back(i);
      }
    }
    // the two batches: the caller's verdicts for the row's message
    for (u32 r = 0; r < sigs; r++) {
      const u32 i = sig_msg[r];
      CHECK(start[r] == off[i] && len[r] == off[i + 1] - off[i]);
      sigv[r] = (int8_t)ver_b[3 * (size_t)i];
    }
    for (u32 r = 0; r < keys; r++) {
      const u32 i = key_msg[r];
      CHECK(memcmp(keys33 + 66 * (size_t)r, msgs + off[i] + keyoff[i] + 66, 66) == 0);
      keyok[2 * (size_t)r] = ver_b[3 * (size_t)i + 1];
      keyok[2 * (size_t)r + 1] = ver_b[3 * (size_t)i + 2];
    }
    // k_ca_settle, the stable sort by the 64-bit scid, k_ca_items, the minimum scan by key
    for (u32 i : visit_order(n, how)) {
      const u64 k = scid[i];
      item[i] = store_ca_settle(status, scid, list, row_of, sigv, keyok, blockheight, i);
      key[i] = k;
    }
    std::vector<u32> perm(n);
    for (u32 i = 0; i < n; i++) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](u32 x, u32 y) { return key[x] < key[y]; });
    for (u32 p = 0; p < n; p++) { skey[p] = key[perm[p]]; sval[p] = perm[p]; }
    for (u32 p : visit_order(n, how)) sitem[p] = item[sval[p]];
    for (u32 p = 0; p < n; p++) first[p] = p && skey[p - 1] == skey[p] && first[p - 1] < sitem[p] ? first[p - 1] : sitem[p];
    // k_ca_resolve, the scan, k_ca_script
    for (u32 p : visit_order(n, how)) store_ca_resolve(sval, first, scid, blockheight, p, status, acnt);
    u64 *apos = block<u64>((size_t)n + 1, 0xEE);
    u64 run = 0;
    for (u32 i = 0; i <= n; i++) { apos[i] = run; run += acnt[i]; }
    const u64 asks = apos[n];
    u8 *spk = block<u8>(STORE_CA_SPK * (size_t)n, 0xEE);
    u32 *ask_msg = block<u32>(asks, 0xEE);
    u64 *ask_scid = block<u64>(asks, 0xEE);
    for (u32 i : visit_order(n, how)) store_ca_finish(b, status, scid, keyoff, apos, asks, spk, ask_msg, ask_scid, i);
    R.status.assign(status, status + n);
    R.scid.assign(scid, scid + n);
    R.spk.assign(spk, spk + STORE_CA_SPK * (size_t)n);
    R.list.assign(list, list + n);
    R.ask_msg.assign(ask_msg, ask_msg + asks);
    R.ask_scid.assign(ask_scid, ask_scid + asks);
    R.counts = {sigs, keys};
    free_all({status, sigv, scid, start, len, key, skey, keyoff, row_of, item, sval, sitem, first, acnt, list, keys33, keyok, apos, spk, ask_msg, ask_scid});
    runs.push_back(R);
  }
  CHECK(runs[0] == runs[1]);
  CHECK(runs[0] == runs[2]);
  const rx_result &R = runs[0];
  const std::string out = argv[5];
  write_file(out + ".status", R.status);
  write_file(out + ".scid", R.scid);
  write_file(out + ".spk", R.spk);
  write_file(out + ".list", R.list);
  write_file(out + ".askmsg", R.ask_msg);
  write_file(out + ".askscid", R.ask_scid);
  write_file(out + ".counts", R.counts);
  free_all({dscid, bare, held, failed, msgs, off});
  return 0;
}

struct cf_result {
  std::vector<int8_t> status;
  std::vector<u32> pend, add_reply, clr;
  std::vector<u64> fail, add_off;
  std::vector<u8> bytes;
  bool operator==(const cf_result &o) const {
    return status == o.status && pend == o.pend && add_reply == o.add_reply && clr == o.clr && fail == o.fail && add_off == o.add_off && bytes == o.bytes;
  }
};

static int confirm(char **argv) {
  const std::vector<u8> image = read_file(argv[2]), view_b = read_file(argv[3]), pend_b = read_file(argv[4]), rep_b = read_file(argv[5]);
  reader vr{view_b};
  const u32 n_rec = vr.get<u32>(), count = vr.get<u32>(), nbare = vr.get<u32>(), nodes = vr.get<u32>();
  u64 *rec_off = block_of(vr.take<u64>(n_rec)), *dscid = block_of(vr.take<u64>(count)), *bare = block_of(vr.take<u64>(nbare)), *node_off = block_of(vr.take<u64>(nodes));
  u32 *node_nann = block_of(vr.take<u32>(nodes));
  u8 *store = block_of(image);
  const store_cf_view v{dscid, count, bare, nbare, store, image.size(), rec_off, n_rec, node_off, node_nann, nodes};
  reader pr{pend_b};
  const u32 np = pr.get<u32>();
  std::vector<u8> msgs_v, spk_v;
  std::vector<u64> off_v{0}, pscid_v;
  for (u32 p = 0; p < np; p++) {
    const u32 len = pr.get<u32>();
    const std::vector<u8> m = pr.take<u8>(len), k = pr.take<u8>(STORE_CA_SPK);
    const gossip_frame f = gossip_parse_frame(m.data(), m.size());
    CHECK(len >= STORE_CA_MIN && !f.bad);
    pscid_v.push_back(store_be64(m.data() + f.keyoff - 8));
    CHECK(p == 0 || pscid_v[p] > pscid_v[p - 1]);
    msgs_v.insert(msgs_v.end(), m.begin(), m.end());
    spk_v.insert(spk_v.end(), k.begin(), k.end());
    off_v.push_back(msgs_v.size());
  }
  if (failures) return 1;
  reader rr{rep_b};
  const u32 nr = rr.get<u32>();
  std::vector<u64> rscid_v, rsat_v, soff_v{0};
  std::vector<u8> scripts_v;
  for (u32 r = 0; r < nr; r++) {
    rscid_v.push_back(rr.get<u64>());
    rsat_v.push_back(rr.get<u64>());
    const u32 len = rr.get<u32>();
    const std::vector<u8> s = rr.take<u8>(len);
    scripts_v.insert(scripts_v.end(), s.begin(), s.end());
    soff_v.push_back(scripts_v.size());
  }
  const u64 msg_bytes = msgs_v.size();
  u64 *pscid = block_of(pscid_v), *rscid = block_of(rscid_v), *rsat = block_of(rsat_v), *soff = block_of(soff_v);
  u8 *pspk = block_of(spk_v), *scripts = block_of(scripts_v);
  u32 T[4 * 256];
  store_crc_build_tables(T, 4);

  std::vector<cf_result> runs;
  for (int how = 0; how < 3; how++) {
    cf_result R;
    // the pending messages, then room for ten bytes per reply; the offsets of np + nr messages
    u8 *msgs = block<u8>(msg_bytes + STORE_CA_AMOUNT * (size_t)nr, 0xEE);
    if (msg_bytes) memcpy(msgs, msgs_v.data(), msg_bytes);
    u64 *off2 = block<u64>((size_t)np + nr + 1, 0);
    for (u32 p = 0; p <= np; p++) off2[p] = off_v[p];
    const store_cf_batch b{msgs, off2, pscid, pspk, np, rscid, rsat, scripts, soff, nr};
    int8_t *status = block<int8_t>(nr, 0xEE);
    u32 *pend = block<u32>(nr, 0xEE), *first = block<u32>(np, 0xFF), *acnt = block<u32>((size_t)nr + 1, 0), *abytes = block<u32>((size_t)nr + 1, 0),
        *fcnt = block<u32>((size_t)nr + 1, 0), *clr_key = block<u32>(2 * (size_t)nr, 0xFF);
    for (u32 r : visit_order(nr, how)) store_cf_match(b, r, pend, first);
    for (u32 r : visit_order(nr, how)) status[r] = (int8_t)store_cf_classify(v, b, r, pend, first, store_cf_marks{acnt, abytes, fcnt, clr_key});
    // the sort of the dying records, the heads, the scans
    std::vector<u32> csort(clr_key, clr_key + 2 * (size_t)nr);
    std::sort(csort.begin(), csort.end());
    u32 *sorted = block_of(csort);
    for (u32 p : visit_order(2 * nr, how))
      if (store_cf_clr_head(sorted, p)) R.clr.push_back(sorted[p]);
    std::sort(R.clr.begin(), R.clr.end());   // (the device scatters by the scan of the heads: ascending)
    u64 *apos = block<u64>((size_t)nr + 1, 0xEE), *abyte = block<u64>((size_t)nr + 1, 0xEE), *fpos = block<u64>((size_t)nr + 1, 0xEE);
    u64 ra = 0, rb = 0, rf = 0;
    for (u32 r = 0; r <= nr; r++) {
      apos[r] = ra; abyte[r] = rb; fpos[r] = rf;
      ra += acnt[r]; rb += abytes[r]; rf += fcnt[r];
    }
    const u64 adds = apos[nr], total = abyte[nr], fails = fpos[nr];
    u32 *add_reply = block<u32>(adds, 0xEE), *rec_msg = block<u32>(2 * adds, 0xEE);
    u64 *add_off = block<u64>(adds, 0xEE), *fail = block<u64>(fails, 0xEE), *rec_off2 = block<u64>(2 * adds, 0xEE);
    const store_cf_plan_out o{adds, fails, add_reply, add_off, fail, rec_msg, rec_off2, off2, msgs + msg_bytes, msg_bytes};
    for (u32 r : visit_order(nr, how)) store_cf_plan(b, status, pend, apos, abyte, fpos, o, r);
    // k_rx_encode, k_rx_copy at four alignments
    u8 *hdr = block<u8>(STORE_HDR * 2 * adds, 0xEE), *flags0 = block<u8>((size_t)np + nr, 0);
    u32 *zero = block<u32>((size_t)np + nr, 0);
    const store_rx_batch eb{msgs, off2, (u32)(np + adds), nullptr, 0, nullptr, 0};
    for (u32 j : visit_order((u32)(2 * adds), how)) store_rx_header<4>(T, eb, flags0, zero, rec_msg[j], hdr + STORE_HDR * (size_t)j);
    const store_rx_out ro{rec_off2, rec_msg, (u32)(2 * adds), hdr, msgs, off2};
    for (u32 mis = 0; mis < 4; mis++) {
      u8 *raw = (u8 *)aligned_alloc(4, (total + mis + 3) / 4 * 4 + 4);
      u8 *out = raw + mis;   // the words the encoder stores lie inside [out, out + total)
      memset(raw, 0xEE, (total + mis + 3) / 4 * 4 + 4);
      const u64 words = (total + mis + 3) / 4;
      if (adds)
        for (u32 k : visit_order((u32)words, how)) store_rx_word(ro, out, total, mis, k);
      const std::vector<u8> got(out, out + total);
      if (mis == 0) R.bytes = got; else CHECK(got == R.bytes);
      for (u32 x = 0; x < mis; x++) CHECK(raw[x] == 0xEE);
      for (u64 x = total + mis; x < (total + mis + 3) / 4 * 4 + 4; x++) CHECK(raw[x] == 0xEE);
      free(raw);
    }
    R.status.assign(status, status + nr);
    R.pend.assign(pend, pend + nr);
    R.add_reply.assign(add_reply, add_reply + adds);
    R.add_off.assign(add_off, add_off + adds);
    R.fail.assign(fail, fail + fails);
    free_all({msgs, off2, status, pend, first, acnt, abytes, fcnt, clr_key, sorted, apos, abyte, fpos, add_reply, rec_msg, add_off, fail, rec_off2, hdr, flags0, zero});
    runs.push_back(R);
  }
  CHECK(runs[0] == runs[1]);
  CHECK(runs[0] == runs[2]);
  const cf_result &R = runs[0];
  const std::string out = argv[6];
  write_file(out + ".status", R.status);
  write_file(out + ".pend", R.pend);
  write_file(out + ".fail", R.fail);
  write_file(out + ".addreply", R.add_reply);
  write_file(out + ".addoff", R.add_off);
  write_file(out + ".clr", R.clr);
  write_file(out + ".bytes", R.bytes);
  free_all({rec_off, dscid, bare, node_off, node_nann, store, pscid, rscid, rsat, soff, pspk, scripts});
  return 0;
}

int main(int argc, char **argv) {
  int rc = 2;
  if (argc == 6 && !strcmp(argv[1], "receive")) rc = receive(argv);
  else if (argc == 7 && !strcmp(argv[1], "confirm")) rc = confirm(argv);
  else printf("usage: receive DIGEST BATCH VERDICTS OUT | confirm IMAGE VIEW PENDING REPLIES OUT\n");
  if (rc) return rc;
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

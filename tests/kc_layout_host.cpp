// The key-table builder through the interleaved views (verify_core.h kc_lanes) against the same stages on a key's flat scratch area
// (keytable_build): for 7 and 10 teeth, 1 / 3 / 64 / 65 keys and groups of 1 / 4 / 64 / 256 keys, every word of every table and of its Zc must be
// the same.  A stand-alone program (built with -fsanitize=address,undefined by tests/test_kc_layout_host.py): the interleaved areas are sized
// exactly, with guard chunks on both sides that must come back untouched.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../lightning_amd/csrc/verify_core.h"

using namespace lamd;

static const int GUARD = 8;
static const u32 PATTERN = 0xA5C3F00Du;

struct guarded {
  std::vector<kc_chunk> mem;
  explicit guarded(size_t chunks) : mem(chunks + 2 * GUARD) {
    for (auto &c : mem)
      for (u32 &w : c.w) w = PATTERN;
  }
  u32 *words() { return mem[GUARD].w; }
  bool intact() const {
    for (int i = 0; i < GUARD; i++)
      for (int j = 0; j < 4; j++)
        if (mem[i].w[j] != PATTERN || mem[mem.size() - 1 - i].w[j] != PATTERN) return false;
    return true;
  }
};

// the k-th point of the test: the first x >= 1000 k + 2 with a point on the curve, even or odd y in turn
static ge test_point(int k) {
  for (u32 x = 1000u * (u32)k + 2u;; x++) {
    u8 key[33] = {};
    key[0] = (u8)(2 + (k & 1));
    key[29] = (u8)(x >> 24); key[30] = (u8)(x >> 16); key[31] = (u8)(x >> 8); key[32] = (u8)x;
    u32 qx[8], qy[8];
    if (parse_pubkey(key, 33, qx, qy)) return ge_from_words(qx, qy);
  }
}

template <int T>
static int run(int nkeys, int stride) {
  constexpr int NS = kc_nsub(T);
  // reference, made once per key: the stages on a flat scratch area
  static std::vector<ge> qs;
  static std::vector<std::vector<u32>> ref;
  for (int k = (int)qs.size(); k < nkeys; k++) {
    qs.push_back(test_point(k));
    ref.emplace_back(kc_stride(T), 0u);
    std::vector<u32> scratch(kc_scratch_words(T));
    keytable_build<T>(ref[k].data(), scratch.data(), qs[k]);
  }
  // groups of `stride` keys: their key words interleaved over the group's keys, their chain words over its stride * NS chains; stage by stage over
  // all keys, as the kernels run them
  const size_t groups = ((size_t)nkeys + stride - 1) / stride, cstride = (size_t)stride * NS;
  guarded keys(groups * stride * kc_key_chunks(T)), chains(groups * cstride * KC_CHAIN_CHUNKS);
  std::vector<std::vector<u32>> tab(nkeys, std::vector<u32>(kc_stride(T), 0u));
  const auto key_view = [&](int k) { return kc_lanes{keys.words() + (size_t)(k / stride) * stride * 4 * kc_key_chunks(T), (size_t)stride, (size_t)(k % stride)}; };
  const auto chain_view = [&](int k, int sub) {
    return kc_lanes{chains.words() + (size_t)(k / stride) * cstride * 4 * KC_CHAIN_CHUNKS, cstride, (size_t)(k % stride) * NS + sub};
  };
  for (int k = 0; k < nkeys; k++) kc_bases_at<T>(key_view(k), qs[k]);
  for (int k = 0; k < nkeys; k++)
    for (int s = 0; s < NS; s++) kc_chain_fwd_at<T>(tab[k].data(), key_view(k), chain_view(k, s), s);
  for (int k = 0; k < nkeys; k++) kc_prefix_at<T>(tab[k].data(), key_view(k), chain_view(k, 0), qs[k]);
  for (int k = 0; k < nkeys; k++)
    for (int s = 0; s < NS; s++) kc_chain_bwd_at<T>(tab[k].data(), chain_view(k, s), s);
  int bad = 0;
  for (int k = 0; k < nkeys; k++)
    for (int w = 0; w < kc_stride(T); w++)
      if (tab[k][w] != ref[k][w]) {
        if (!bad) printf("T=%d keys=%d stride=%d: key %d word %d is %08x, expected %08x\n", T, nkeys, stride, k, w, tab[k][w], ref[k][w]);
        bad++;
      }
  if (!keys.intact() || !chains.intact()) {
    printf("T=%d keys=%d stride=%d: guard words overwritten\n", T, nkeys, stride);
    bad++;
  }
  // (an all-zero Zc would make every comparison above vacuous)
  bool zc = false;
  for (int w = 0; w < TW; w++) zc |= ref[0][kc_words(T) + w] != 0;
  if (!zc) bad++;
  return bad;
}

int main() {
  int bad = 0, cases = 0;
  for (int nkeys : {1, 3, 64, 65})
    for (int stride : {1, 4, 64, 256}) {
      bad += run<7>(nkeys, stride);
      bad += run<10>(nkeys, stride);
      cases += 2;
    }
  printf("kc_layout_host: %d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}

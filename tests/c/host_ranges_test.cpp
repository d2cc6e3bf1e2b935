// lightning_amd/csrc/host_ranges.h on the host (tests/test_host_ranges.py): the decision whether a column queued "in place" may cross the bus from
// the caller's memory -- only if ONE registered range holds all of it.  Prints "ok" and exits 0, or names the first check that failed.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "host_ranges.h"

static std::atomic<int> failures{0};
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

int main() {
  static unsigned char mem[1 << 20];
  unsigned char *const B = mem;
  lamd::host_ranges r;

  // nothing registered: nothing stays in place
  CHECK(!r.covers(B, 1));
  CHECK(!r.covers(nullptr, 16));

  // one range: inside, both edges, one byte past either edge, empty and wrapping queries
  r.add(B + 4096, 8192);
  CHECK(r.covers(B + 4096, 8192));
  CHECK(r.covers(B + 4096, 1));
  CHECK(r.covers(B + 4096 + 8191, 1));
  CHECK(r.covers(B + 5000, 100));
  CHECK(!r.covers(B + 4095, 2));
  CHECK(!r.covers(B + 4096, 8193));
  CHECK(!r.covers(B + 4096 + 8192, 1));
  CHECK(!r.covers(B + 4096, 0));
  CHECK(!r.covers((const void *)(~(uintptr_t)0 - 4), 64));

  // two ADJACENT ranges: each covers its own part, a column across the seam is in neither
  r.add(B + 4096 + 8192, 4096);
  CHECK(r.covers(B + 4096 + 8192, 4096));
  CHECK(r.covers(B + 4096, 8192));
  CHECK(!r.covers(B + 4096 + 8000, 400));
  CHECK(!r.covers(B + 4096, 8192 + 4096));

  // a HOLE: two ranges with unregistered pages between them -- a column over the hole is copied, so is one that only touches it
  r.add(B + 65536, 4096);
  r.add(B + 65536 + 3 * 4096, 4096);
  CHECK(!r.covers(B + 65536, 4 * 4096));
  CHECK(!r.covers(B + 65536 + 4000, 200));
  CHECK(r.covers(B + 65536 + 3 * 4096, 4096));

  // OVERLAPPING ranges: a column inside either one is covered (also one that begins in the later range and ends inside the earlier, larger one);
  // a column that needs both is not
  r.add(B + 131072, 16384);
  r.add(B + 131072 + 8192, 16384);
  CHECK(r.covers(B + 131072 + 100, 16000));
  CHECK(r.covers(B + 131072 + 8192 + 100, 16000));
  CHECK(r.covers(B + 131072 + 9000, 1000));
  CHECK(!r.covers(B + 131072, 16384 + 8192));

  // an unregistered range stops covering at once; unregistering what was never registered says so and changes nothing
  CHECK(r.remove(B + 4096));
  CHECK(!r.covers(B + 4096, 1));
  CHECK(r.covers(B + 4096 + 8192, 4096));
  CHECK(!r.remove(B + 4096));
  CHECK(!r.remove(B + 4097));
  CHECK(r.size() == 5);

  // several threads registering and unregistering blocks of their own while others ask: every thread's own block is covered between its add and
  // its remove, and after all of them have gone only the ranges registered above are left
  std::vector<std::thread> th;
  for (int t = 0; t < 8; t++)
    th.emplace_back([&, t] {
      unsigned char *const own = B + 262144 + t * 65536;
      for (int i = 0; i < 2000; i++) {
        const size_t len = 4096 * (1 + (i + t) % 8);
        r.add(own, len);
        if (!r.covers(own, len) || !r.covers(own + len - 1, 1) || r.covers(own, len + 1)) failures++;
        if (!r.covers(B + 4096 + 8192, 4096)) failures++;
        if (!r.remove(own) || r.covers(own, 1)) failures++;
      }
    });
  for (auto &x : th) x.join();
  CHECK(r.size() == 5);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures.load());
    return 1;
  }
  printf("ok\n");
  return 0;
}

// lightning_amd/csrc/key_column.h on the host (tests/test_key_column_bytes.py, built with -fsanitize=address,undefined): the number of bytes of a
// caller's key column that may be read -- (n - 1) * stride + keylen, not n * stride -- its overflow report, and a copy of that size out of a heap
// block that is exactly as long as the contract makes readable (one byte more and the sanitizer stops the program).  Prints "ok" and exits 0, or
// names the first check that failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "key_column.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

static bool kcb(size_t n, size_t keylen, size_t stride, size_t *out) { return lamd::key_column_bytes(n, keylen, stride, out); }

int main() {
  size_t b = 99;
  // no rows: nothing is read, whatever the stride
  CHECK(kcb(0, 33, 33, &b) && b == 0);
  b = 99;
  CHECK(kcb(0, 65, 0, &b) && b == 0);
  b = 99;
  CHECK(kcb(0, 33, SIZE_MAX, &b) && b == 0);
  // one row: the key alone
  CHECK(kcb(1, 33, 33, &b) && b == 33);
  CHECK(kcb(1, 33, 4096, &b) && b == 33);
  CHECK(kcb(1, 65, SIZE_MAX, &b) && b == 65);
  // packed columns: n * keylen
  CHECK(kcb(320, 33, 33, &b) && b == 320 * 33);
  CHECK(kcb(320, 65, 65, &b) && b == 320 * 65);
  CHECK(kcb(7, 32, 32, &b) && b == 7 * 32);
  // strided columns end with the last key
  CHECK(kcb(2, 33, 34, &b) && b == 34 + 33);
  CHECK(kcb(320, 33, 97, &b) && b == 319 * 97 + 33);
  CHECK(kcb(320, 65, 128, &b) && b == 319 * 128 + 65);
  CHECK(kcb(5, 32, 40, &b) && b == 4 * 40 + 32);
  CHECK(kcb(4096, 33, 48, &b) && b == 4095 * 48 + 33);
  // a stride shorter than the key is the caller's error
  b = 99;
  CHECK(!kcb(2, 33, 32, &b) && b == 0);
  CHECK(!kcb(1, 65, 64, &b) && b == 0);
  // overflow of size_t: in the product, and in the sum behind it
  b = 99;
  CHECK(!kcb(3, 33, SIZE_MAX / 2 + 1, &b) && b == 0);
  CHECK(!kcb(SIZE_MAX, 33, 33, &b) && b == 0);
  CHECK(!kcb(SIZE_MAX / 64 + 2, 65, 64 + 1, &b) && b == 0);
  CHECK(kcb(2, 33, SIZE_MAX - 33, &b) && b == SIZE_MAX);       // the largest column that fits
  CHECK(!kcb(2, 33, SIZE_MAX - 32, &b) && b == 0);             // one byte more does not
  CHECK(kcb(3, 1, (SIZE_MAX - 1) / 2, &b) && b == 2 * ((SIZE_MAX - 1) / 2) + 1);
  CHECK(!kcb(3, 2, (SIZE_MAX - 1) / 2, &b) && b == 0);

  // the copy every entry point makes: the keys are the LAST field of an array of structs on the heap, so the column handed over ends with the
  // block; copying key_column_bytes() bytes stays inside it (n * stride would not: the sanitizer reports a heap-buffer-overflow)
  const size_t cases[][3] = {{320, 33, 34}, {320, 33, 97}, {64, 65, 66}, {64, 65, 128}, {9, 32, 33}, {1, 33, 97}};
  for (const auto &c : cases) {
    const size_t n = c[0], keylen = c[1], stride = c[2], lead = stride - keylen;   // struct = `lead` bytes of other fields, then the key
    unsigned char *block = (unsigned char *)malloc(n * stride);
    CHECK(block != nullptr);
    if (!block) break;
    for (size_t i = 0; i < n * stride; i++) block[i] = (unsigned char)(i * 131 + 7);
    const unsigned char *column = block + lead;
    size_t bytes = 0;
    CHECK(kcb(n, keylen, stride, &bytes));
    CHECK(column + bytes == block + n * stride);
    std::vector<unsigned char> staged(bytes);
    memcpy(staged.data(), column, bytes);
    for (size_t i = 0; i < n; i++) CHECK(memcmp(&staged[i * stride], block + i * stride + lead, keylen) == 0);
    free(block);
  }

  if (failures) return 1;
  printf("ok\n");
  return 0;
}

// lightning_amd/csrc/table_audit.h on the host under AddressSanitizer and UBSan: a stand-alone program.  The table and every replacement image are
// heap blocks of exactly their size, so an audit that read one entry before or behind the table, or outside a replacement image's range, aborts here
// -- the same index arithmetic runs in k_gtable_audit on the device, where such a read would go unnoticed or fault.
// Built with -DLAMD_GTABLE_WINDOW_BITS=4 (64 windows of 16 entries: every rule, every window boundary, cheap to build).
// Prints "ok <entries audited>" and exits 0, or names what went wrong and exits 1.
#define LAMD_CHECK_MAG 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "table_audit.h"
using namespace lamd;

// one copy of the audit's code in the program (every call below would inline another)
__attribute__((noinline)) static u32 audit(const gt_view &v, size_t idx) { return gtable_audit_entry(v, idx); }

static int fail(const char *what, size_t a, size_t b) {
  printf("FAIL %s %zu %zu\n", what, a, b);
  return 1;
}

int main() {
  const size_t per = (size_t)1 << GTABLE_WINDOW_BITS;
  u32 *table = (u32 *)malloc(GTABLE_BYTES);   // exactly the table: no slack for an out-of-range read to land in
  if (!table) return fail("malloc", 0, 0);
  memset(table, 0, GTABLE_BYTES);
  const u32 gx[8] = LAMD_GX, gy[8] = LAMD_GY;
  u32 base[16];
  memcpy(base, gx, 32);
  memcpy(base + 8, gy, 32);
  for (int w = 0; w < GTABLE_WINDOWS; w++) {
    for (u32 d = 1; d < per; d++) gtable_compute_entry(table + ((size_t)w * per + d) * GT_ENTRY_WORDS, base, d);
    gej b = gej_from_ge(ge_from_words(base, base + 8));
    for (int i = 0; i < GTABLE_WINDOW_BITS; i++) b = gej_double(b);
    const fe zi = fe_inv(fe_norm_weak(b.z)), zi2 = fe_sqr(zi);
    fe_to_words(base, fe_normalize(fe_mul(b.x, zi2)));
    fe_to_words(base + 8, fe_normalize(fe_mul(b.y, fe_mul(zi2, zi))));
  }
  size_t audited = 0;
  // the whole table, read in place
  {
    const gt_view v = {table, nullptr, 0, GTABLE_ENTRIES};
    for (size_t i = 0; i < GTABLE_ENTRIES; i++, audited++)
      if (audit(v, i)) return fail("clean table flagged", i, audit(v, i));
  }
  // every range [first, first + count) with count = 1 .. 3 windows' worth at every first near a window boundary and at both ends of the table, the
  // range read from an image of exactly count entries (a copy: still clean), the rest from the table
  for (size_t first = 0; first < GTABLE_ENTRIES; first++) {
    const size_t d = first & (per - 1);
    if (!(d <= 3 || d >= per - 3)) continue;
    for (size_t count : {(size_t)1, (size_t)2, (size_t)3, per - 1, per, per + 1, 3 * per}) {
      if (count > GTABLE_ENTRIES - first) continue;
      u32 *image = (u32 *)malloc(count * GT_ENTRY_WORDS * sizeof(u32));
      if (!image) return fail("malloc", first, count);
      memcpy(image, table + first * GT_ENTRY_WORDS, count * GT_ENTRY_WORDS * sizeof(u32));
      const gt_view v = {table, image, first, count};
      for (size_t k = 0; k < count; k++, audited++)
        if (audit(v, first + k)) { free(image); return fail("clean image flagged", first, count); }
      // a wrong last entry is seen inside the range, and by nobody who reads the table behind it
      image[(count - 1) * GT_ENTRY_WORDS + GT_ENTRY_WORDS - 1] ^= 4u;
      const bool digit0 = ((first + count - 1) & (per - 1)) == 0;
      const u32 r = audit(v, first + count - 1);
      if (!r || (digit0 ? r != (u32)GTA_ZERO : !(r & GTA_OFF_CURVE))) { free(image); return fail("wrong last entry not flagged", first, count); }
      const gt_view plain = {table, nullptr, 0, 0};
      for (size_t j = first + count; j < GTABLE_ENTRIES && j <= first + count + 1; j++)
        if (audit(plain, j)) { free(image); return fail("table read through the image", first, count); }
      free(image);
    }
  }
  free(table);
  printf("ok %zu\n", audited);
  return 0;
}

// Audit of the static G table (verify_core.h "Static table of G"): judges ONE entry of a table image from field operations only.
// Diagnostic -- no verdict path includes a call of it.  It shares nothing with the builder (k_gtable_build / gtable_compute_entry: gej_double,
// gej_add_ge, fe_inv_var) but the field primitives fe_mul / fe_sqr / add / neg / normalise, which lamd_fuzz_field checks against the host:
// no gej_*, no inversion.
//
// Window w, digit d holds d * 2^(BITS*w) * G.  Write B = T[w][1].  With the anchor T[0][1] = G the rules below prove every entry by induction:
//   d = 0           all words zero
//   d >= 1          both coordinates canonical (the stored words, not a reduced value, read as an integer below p); y^2 = x^3 + 7
//   d = 1, w = 0    the entry is LAMD_GX / LAMD_GY
//   d = 1, w > 0    chord rule with P1 = T[w-1][2^BITS - 1], the base B' = T[w-1][1], P3 = this entry     ((2^BITS - 1) B' + B' = 2^BITS B')
//   d = 2           tangent rule from B:   M = 3 x_B^2, D = 2 y_B (D = 0 is itself a failure):
//                       x3 D^2 = M^2 - 2 x_B D^2          (y3 + y_B) D = M (x_B - x3)
//   d >= 3          chord rule with P1 = T[w][d-1]:   H = x1 - x_B, R = y1 - y_B (H = 0 is itself a failure):
//                       x3 H^2 = R^2 - (x1 + x_B) H^2     (y3 + y1) H = R (x1 - x3)
// Entry i is judged by the step i-1 -> i, so ONE wrong entry is reported at itself and at its successor; a wrong base entry at every entry of
// its window and at entry 1 of the next.
#ifndef LAMD_TABLE_AUDIT_H
#define LAMD_TABLE_AUDIT_H
#include "verify_core.h"

namespace lamd {

// reason bits (include/lightning_amd_debug.h LAMD_GTA_*)
enum {
  GTA_ZERO = 1,        // the d = 0 entry is not all zero
  GTA_NONCANON = 2,    // a coordinate's stored words are not the canonical representative
  GTA_OFF_CURVE = 4,   // y^2 != x^3 + 7
  GTA_ANCHOR = 8,      // T[0][1] != G
  GTA_X = 16,          // the x relation of the chord / tangent rule fails
  GTA_Y = 32,          // the y relation fails
  GTA_DEGENERATE = 64  // H = 0 (chord) or D = 0 (tangent): the operands cannot be the points the rule needs
};

// A table image in which the entries [first, first + count) may come from a replacement image of exactly that range (image != nullptr)
struct gt_view {
  const u32 *table;
  const u32 *image;
  size_t first, count;
};
LAMD_HD const u32 *gt_entry(const gt_view &v, size_t i) {
  return (v.image && i - v.first < v.count) ? v.image + (i - v.first) * GT_ENTRY_WORDS : v.table + i * GT_ENTRY_WORDS;  // i < first wraps: not below count
}

LAMD_HD bool gt_coord_canonical(const u32 *c) {
  if (!LAMD_TABLE_LIMBS) return !words_ge_p(c);
  bool ok = c[8] <= FE_M24;
  for (int i = 0; i < 8; i++) ok &= c[i] <= FE_M29;
  if (!ok) return false;
  const fe n = fe_normalize(slot_load_raw(c));
  for (int i = 0; i < 9; i++) ok &= n.n[i] == c[i];
  return ok;
}

// P3 = P1 + B by the chord through P1 and B, without a division
LAMD_HD u32 gt_chord(const u32 *p1, const u32 *b, const fe &x3, const fe &y3) {
  const fe x1 = slot_load_fe(p1), y1 = slot_load_fe(p1 + TW), xb = slot_load_fe(b), yb = slot_load_fe(b + TW);
  const fe h = fe_norm_weak(fe_sub(x1, xb, 1)), r = fe_norm_weak(fe_sub(y1, yb, 1));
  if (fe_is_zero(h)) return GTA_DEGENERATE;
  const fe h2 = fe_sqr(h);
  u32 bad = 0;
  const fe rx = fe_add(fe_sqr(r), fe_neg(fe_mul(fe_add(x1, xb), h2), 1));
  if (!fe_equal(rx, fe_mul(x3, h2), 1)) bad |= GTA_X;
  const fe ry = fe_mul(r, fe_norm_weak(fe_sub(x1, x3, 1)));
  if (!fe_equal(fe_mul(fe_add(y3, y1), h), ry, 1)) bad |= GTA_Y;
  return bad;
}
// P3 = 2 B by the tangent at B
LAMD_HD u32 gt_tangent(const u32 *b, const fe &x3, const fe &y3) {
  const fe xb = slot_load_fe(b), yb = slot_load_fe(b + TW);
  const fe m = fe_norm_weak(fe_mul_int(fe_sqr(xb), 3)), d = fe_mul_int(yb, 2);
  if (fe_is_zero(d)) return GTA_DEGENERATE;
  const fe d2 = fe_sqr(d);
  u32 bad = 0;
  const fe rx = fe_add(fe_sqr(m), fe_neg(fe_mul(fe_mul_int(xb, 2), d2), 1));
  if (!fe_equal(rx, fe_mul(x3, d2), 1)) bad |= GTA_X;
  const fe ry = fe_mul(m, fe_norm_weak(fe_sub(xb, x3, 1)));
  if (!fe_equal(fe_mul(fe_add(y3, yb), d), ry, 1)) bad |= GTA_Y;
  return bad;
}

// reason mask of entry idx (flat index: window << BITS | digit) of the image v; 0 = good
LAMD_HD u32 gtable_audit_entry(const gt_view &v, size_t idx) {
  constexpr size_t DMASK = ((size_t)1 << GTABLE_WINDOW_BITS) - 1;
  const size_t w = idx >> GTABLE_WINDOW_BITS, d = idx & DMASK;
  const u32 *e = gt_entry(v, idx);
  if (d == 0) {
    u32 any = 0;
    for (int i = 0; i < GT_ENTRY_WORDS; i++) any |= e[i];
    return any ? (u32)GTA_ZERO : 0u;
  }
  u32 bad = 0;
  if (!gt_coord_canonical(e) || !gt_coord_canonical(e + TW)) bad |= GTA_NONCANON;
  const fe x3 = slot_load_fe(e), y3 = slot_load_fe(e + TW);
  if (!fe_equal(fe_sqr(y3), fe_add(fe_mul(fe_sqr(x3), x3), fe_set_int(7)), 2)) bad |= GTA_OFF_CURVE;
  if (d == 1) {
    if (w == 0) {
      const u32 gx[8] = LAMD_GX, gy[8] = LAMD_GY;
      if (!fe_equal(x3, fe_from_words(gx), 1) || !fe_equal(y3, fe_from_words(gy), 1)) bad |= GTA_ANCHOR;
    } else {
      bad |= gt_chord(gt_entry(v, idx - 2), gt_entry(v, idx - DMASK - 1), x3, y3);  // T[w-1][2^BITS - 1] and T[w-1][1]
    }
  } else if (d == 2) {
    bad |= gt_tangent(gt_entry(v, idx - 1), x3, y3);
  } else {
    bad |= gt_chord(gt_entry(v, idx - 1), gt_entry(v, idx - d + 1), x3, y3);
  }
  return bad;
}

}  // namespace lamd
#endif

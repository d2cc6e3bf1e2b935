// CPU build of the comb column's group law (lightning_amd/csrc/group.h compiled for the host with magnitude checking on): the affine + affine
// pair sum (ge_add_ge_fast) and the accumulator + pair addition (gej_add_pair_fast) next to what they replace, two successive
// gej_add_ge_fast.  Test infrastructure only (tests/test_pair_column_host.py).  Field elements cross the boundary as their 9 raw limbs, so the
// test chooses the limbs (up to the magnitude bounds) and reads results without a normalisation in between.
#define LAMD_CHECK_MAG 1
#include "../../lightning_amd/csrc/group.h"
using namespace lamd;

static fe in_fe(const u32 *l, int mag) { fe a; for (int i = 0; i < 9; i++) a.n[i] = l[i]; a.mag = mag; fe_verify(a); return a; }
static void out_fe(u32 *l, const fe &a) { for (int i = 0; i < 9; i++) l[i] = a.n[i]; }
// acc: x | y | z (27 limbs), x and y magnitude 1, z magnitude zmag
static gej in_gej(const u32 *l, int zmag) { gej a; a.x = in_fe(l, 1); a.y = in_fe(l + 9, 1); a.z = in_fe(l + 18, zmag); a.inf = false; return a; }
static int out_gej(u32 *l, const gej &a) { out_fe(l, a.x); out_fe(l + 9, a.y); out_fe(l + 18, a.z); LAMD_ASSERT(a.x.mag <= 1 && a.y.mag <= 1 && a.z.mag <= 2); return a.z.mag; }
// a table entry as the column meets it: x | y (18 limbs, magnitude 1), then the lazy negation (y magnitude 2)
static ge in_ge(const u32 *l, int neg) { ge p; p.x = in_fe(l, 1); p.y = in_fe(l + 9, 1); return ge_neg_if_lazy(p, neg != 0); }

extern "C" {
// pair: x | y | z | zz | zzz (45 limbs)
void pc_pair(const u32 *p1, int neg1, const u32 *p2, int neg2, u32 *pair) {
  const gejzz r = ge_add_ge_fast(in_ge(p1, neg1), in_ge(p2, neg2));
  LAMD_ASSERT(r.x.mag <= 1 && r.y.mag <= 1 && r.z.mag <= 1 && r.zz.mag <= 1 && r.zzz.mag <= 1);
  out_fe(pair, r.x); out_fe(pair + 9, r.y); out_fe(pair + 18, r.z); out_fe(pair + 27, r.zz); out_fe(pair + 36, r.zzz);
}
// out = acc + pair; returns the magnitude of out's z
int pc_add_pair(const u32 *acc, int zmag, const u32 *pair, u32 *out) {
  gejzz b;
  b.x = in_fe(pair, 1); b.y = in_fe(pair + 9, 1); b.z = in_fe(pair + 18, 1); b.zz = in_fe(pair + 27, 1); b.zzz = in_fe(pair + 36, 1);
  return out_gej(out, gej_add_pair_fast(in_gej(acc, zmag), b));
}
// out = (acc + p1) + p2, the two mixed additions of the column before
int pc_add_two(const u32 *acc, int zmag, const u32 *p1, int neg1, const u32 *p2, int neg2, u32 *out) {
  return out_gej(out, gej_add_ge_fast(gej_add_ge_fast(in_gej(acc, zmag), in_ge(p1, neg1)), in_ge(p2, neg2)));
}
int pc_double(const u32 *acc, int zmag, u32 *out) { return out_gej(out, gej_double(in_gej(acc, zmag))); }
// what the caller's one test at the end of the G run sees: ZZ of the XYZZ form == 0 ?
int pc_zz_is_zero(const u32 *acc, int zmag) { return fe_is_zero(gexz_from_gej(in_gej(acc, zmag)).zz); }
}

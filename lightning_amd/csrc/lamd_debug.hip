// liblightning_amd.so, the debuggers of include/lightning_amd_debug.h (lamd_selftest and the G-table audit stay with the core they check)
#include "engine_internal.h"
#include "fuzz.h"

// What the three arithmetic debuggers share: ST_LANES seeded random inputs (b as well where asked), ONE launch of one ST_LANES-lane block on the context's
// stream, its `words` output words.  The device buffers free themselves on every return.
template <class Launch>
static int debug_run(lamd_ctx *ctx, u64 s, bool with_b, size_t words, std::vector<st_in> &in, std::vector<u32> &got, Launch launch) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  in.assign(ST_LANES, st_in());
  for (int i = 0; i < ST_LANES; i++)
    for (int j = 0; j < 8; j++) {
      in[i].a[j] = (u32)splitmix64(s++);
      if (with_b) in[i].b[j] = (u32)splitmix64(s++);
    }
  devbuf d_in, d_out;
  int rc;
  if ((rc = ensure(ctx, &d_in, sizeof(st_in) * ST_LANES)) != LAMD_OK || (rc = ensure(ctx, &d_out, words * 4)) != LAMD_OK) return rc;
  HIPCHK(ctx, hipMemcpy(d_in.p, in.data(), sizeof(st_in) * ST_LANES, hipMemcpyHostToDevice));
  launch(d_in.as<const st_in>(), d_out.as<u32>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  got.resize(words);
  HIPCHK(ctx, hipMemcpy(got.data(), d_out.p, words * 4, hipMemcpyDeviceToHost));
  return LAMD_OK;
}

// ---- op-level chain debugger: device runs a dependent chain of fe_sqr / fe_mul and records raw limbs in and out of
// every step; the host re-executes each step on the device's own inputs and reports the first disagreement.
constexpr int CH_ITERS = 300;
__global__ void __launch_bounds__(64) k_chain_debug(const st_in *in, u32 *out, int use_mul) {
  const int lane = threadIdx.x;
  fe a = fe_from_words(in[lane].a);
  const fe b = fe_from_words(in[lane].b);
  u32 *o = out + (size_t)lane * CH_ITERS * 18;
#pragma unroll 1
  for (int it = 0; it < CH_ITERS; it++) {
    for (int i = 0; i < 9; i++) o[it * 18 + i] = a.n[i];
    const fe r = use_mul ? fe_mul(a, b) : fe_sqr(a);
    for (int i = 0; i < 9; i++) o[it * 18 + 9 + i] = r.n[i];
    a = r;
  }
}
extern "C" int lamd_chain_debug(lamd_ctx *ctx, int use_mul, char *report, size_t cap) {
  if (!ctx) return LAMD_ERR_ARG;
  std::vector<st_in> in;
  std::vector<u32> got;
  const int rc = debug_run(ctx, 0x7654321, true, (size_t)ST_LANES * CH_ITERS * 18, in, got, [&](const st_in *d_in, u32 *d_out) {
    hipLaunchKernelGGL(k_chain_debug, dim3(1), dim3(ST_LANES), 0, ctx->stream, d_in, d_out, use_mul);
  });
  if (rc != LAMD_OK) return rc;
  int nbad = 0;
  std::string rep;
  char buf[512];
  for (int lane = 0; lane < ST_LANES; lane++) {
    const fe b = fe_from_words(in[lane].b);
    for (int it = 0; it < CH_ITERS; it++) {
      const u32 *o = &got[((size_t)lane * CH_ITERS + it) * 18];
      fe a;
      for (int i = 0; i < 9; i++) a.n[i] = o[i];
      const fe r = use_mul ? fe_mul(a, b) : fe_sqr(a);
      bool bad = false;
      for (int i = 0; i < 9; i++) bad |= r.n[i] != o[9 + i];
      if (bad) {
        if (nbad < 3) {
          snprintf(buf, sizeof buf, "lane %d it %d in=[%x %x %x %x %x %x %x %x %x] dev=[%x %x %x %x %x %x %x %x %x] host=[%x %x %x %x %x %x %x %x %x]; ",
                   lane, it, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11], o[12], o[13], o[14], o[15], o[16], o[17],
                   r.n[0], r.n[1], r.n[2], r.n[3], r.n[4], r.n[5], r.n[6], r.n[7], r.n[8]);
          rep += buf;
          if (use_mul) { snprintf(buf, sizeof buf, "b=[%x %x %x %x %x %x %x %x %x]; ", b.n[0], b.n[1], b.n[2], b.n[3], b.n[4], b.n[5], b.n[6], b.n[7], b.n[8]); rep += buf; }
        }
        nbad++;
      }
    }
  }
  if (report && cap) { strncpy(report, rep.c_str(), cap - 1); report[cap - 1] = 0; }
  return nbad;
}

// ---- inversion-chain debugger: every intermediate of the addition chain, device vs host
constexpr int INV_ITEMS = 24;
LAMD_HD void inv_debug_lane(const u32 aw[8], u32 *o) {
  const fe a = fe_from_words(aw);
  fe items[INV_ITEMS];
  int k = 0;
  const int ns[8] = {1, 2, 3, 5, 11, 22, 44, 88};
  for (int j = 0; j < 8; j++) items[k++] = fe_sqr_n(a, ns[j]);  // 0..7
  const fe x2 = fe_mul(fe_sqr(a), a);
  const fe x3 = fe_mul(fe_sqr(x2), a);
  const fe x6 = fe_mul(fe_sqr_n(x3, 3), x3);
  const fe x9 = fe_mul(fe_sqr_n(x6, 3), x3);
  const fe x11 = fe_mul(fe_sqr_n(x9, 2), x2);
  const fe x22 = fe_mul(fe_sqr_n(x11, 11), x11);
  const fe x44 = fe_mul(fe_sqr_n(x22, 22), x22);
  const fe x88 = fe_mul(fe_sqr_n(x44, 44), x44);
  const fe x176 = fe_mul(fe_sqr_n(x88, 88), x88);
  const fe x220 = fe_mul(fe_sqr_n(x176, 44), x44);
  const fe x223 = fe_mul(fe_sqr_n(x220, 3), x3);
  items[k++] = x2; items[k++] = x3; items[k++] = x6; items[k++] = x9; items[k++] = x11; items[k++] = x22;   // 8..13
  items[k++] = x44; items[k++] = x88; items[k++] = x176; items[k++] = x220; items[k++] = x223;              // 14..18
  const fe_chain ch = fe_pow_chain(a);
  items[k++] = ch.x2; items[k++] = ch.x22; items[k++] = ch.x223;                                             // 19..21
  items[k++] = fe_inv(a);                                                                                     // 22
  items[k++] = fe_sqrt_candidate(a);                                                                          // 23
  for (int j = 0; j < INV_ITEMS; j++) {
    u32 w[8];
    fe_to_words(w, fe_normalize(items[j]));
    for (int i = 0; i < 8; i++) o[j * 8 + i] = w[i];
  }
}
__global__ void __launch_bounds__(64) k_inv_debug(const st_in *in, u32 *out) {
  inv_debug_lane(in[threadIdx.x].a, out + threadIdx.x * INV_ITEMS * 8);
}
extern "C" int lamd_inv_debug(lamd_ctx *ctx, char *report, size_t cap) {
  if (!ctx) return LAMD_ERR_ARG;
  std::vector<st_in> in;
  std::vector<u32> got, exp(INV_ITEMS * 8);
  const int rc = debug_run(ctx, 0xABCDEF, false, (size_t)ST_LANES * INV_ITEMS * 8, in, got, [&](const st_in *d_in, u32 *d_out) {
    hipLaunchKernelGGL(k_inv_debug, dim3(1), dim3(ST_LANES), 0, ctx->stream, d_in, d_out);
  });
  if (rc != LAMD_OK) return rc;
  int mask = 0;
  std::string rep;
  for (int lane = 0; lane < ST_LANES; lane++) {
    inv_debug_lane(in[lane].a, exp.data());
    for (int j = 0; j < INV_ITEMS; j++)
      if (memcmp(&exp[j * 8], &got[((size_t)lane * INV_ITEMS + j) * 8], 32)) {
        if (!(mask & (1 << j))) {
          rep += "item " + std::to_string(j) + " first bad at lane " + std::to_string(lane) + "; ";
          if (rep.size() < 1500) {
            char buf[400];
            const u32 *g = &got[((size_t)lane * INV_ITEMS + j) * 8], *e = &exp[j * 8], *aw = in[lane].a;
            snprintf(buf, sizeof buf, "a=%08x%08x%08x%08x%08x%08x%08x%08x dev=%08x%08x%08x%08x%08x%08x%08x%08x host=%08x%08x%08x%08x%08x%08x%08x%08x; ",
                     aw[7], aw[6], aw[5], aw[4], aw[3], aw[2], aw[1], aw[0], g[7], g[6], g[5], g[4], g[3], g[2], g[1], g[0], e[7], e[6], e[5], e[4], e[3], e[2], e[1], e[0]);
            rep += buf;
          }
        }
        mask |= 1 << j;
      }
  }
  if (report && cap) { strncpy(report, rep.c_str(), cap - 1); report[cap - 1] = 0; }
  return mask;
}

// ---- x2 debugger: fe_mul(fe_sqr(a), a) in several code shapes, raw limbs out
__global__ void __launch_bounds__(64) k_x2_debug(const st_in *in, u32 *out) {
  const int lane = threadIdx.x;
  u32 *o = out + lane * 64;
  const fe a = fe_from_words(in[lane].a);
  {  // A: fused, raw result
    const fe r = fe_mul(fe_sqr(a), a);
    for (int i = 0; i < 9; i++) o[i] = r.n[i];
  }
  {  // B: intermediate forced through an opaque register barrier
    fe s2 = fe_sqr(a);
#if defined(__HIP_DEVICE_COMPILE__)
    for (int i = 0; i < 9; i++) asm volatile("" : "+v"(s2.n[i]));
#endif
    const fe r = fe_mul(s2, a);
    for (int i = 0; i < 9; i++) o[9 + i] = s2.n[i];
    for (int i = 0; i < 9; i++) o[18 + i] = r.n[i];
  }
  {  // C: fused then normalized
    const fe r = fe_normalize(fe_mul(fe_sqr(a), a));
    for (int i = 0; i < 9; i++) o[27 + i] = r.n[i];
  }
  {  // D: a*a via fe_mul, then *a
    const fe r = fe_mul(fe_mul(a, a), a);
    for (int i = 0; i < 9; i++) o[36 + i] = r.n[i];
  }
}
extern "C" int lamd_x2_debug(lamd_ctx *ctx, char *report, size_t cap) {
  if (!ctx) return LAMD_ERR_ARG;
  std::vector<st_in> in;
  std::vector<u32> got;
  const int rc = debug_run(ctx, 0xABCDEF, false, (size_t)ST_LANES * 64, in, got, [&](const st_in *d_in, u32 *d_out) {
    hipLaunchKernelGGL(k_x2_debug, dim3(1), dim3(ST_LANES), 0, ctx->stream, d_in, d_out);
  });
  if (rc != LAMD_OK) return rc;
  std::string rep;
  int mask = 0;
  char buf[600];
  for (int lane = 0; lane < ST_LANES; lane++) {
    const fe a = fe_from_words(in[lane].a);
    const fe s2 = fe_sqr(a);
    const fe r = fe_mul(s2, a);
    const fe rn = fe_normalize(r);
    const fe rd = fe_mul(fe_mul(a, a), a);
    const u32 *o = &got[lane * 64];
    const fe *exps[5] = {&r, &s2, &r, &rn, &rd};
    const char *names[5] = {"A_fused_raw", "B_sqr_raw", "B_mul_raw", "C_fused_norm", "D_mulmul"};
    for (int t = 0; t < 5; t++) {
      bool bad = false;
      for (int i = 0; i < 9; i++) bad |= exps[t]->n[i] != o[t * 9 + i];
      if (bad) {
        if (!(mask & (1 << t))) {
          const u32 *g = o + t * 9;
          const u32 *e = exps[t]->n;
          snprintf(buf, sizeof buf, "%s lane %d dev=[%x %x %x %x %x %x %x %x %x] host=[%x %x %x %x %x %x %x %x %x]; ", names[t], lane, g[0], g[1], g[2], g[3], g[4],
                   g[5], g[6], g[7], g[8], e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8]);
          rep += buf;
        }
        mask |= 1 << t;
      }
    }
  }
  if (report && cap) { strncpy(report, rep.c_str(), cap - 1); report[cap - 1] = 0; }
  return mask;
}

// ---- randomised arithmetic fuzz (fuzz.h): the same inline function on the device and in this TU's host pass
__global__ void __launch_bounds__(256) k_fuzz_field(size_t lanes, int iters, u64 seed, u64 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < lanes) out[i] = fuzz_lane(seed, i, iters);
}
extern "C" int lamd_fuzz_field(lamd_ctx *ctx, size_t lanes, int iters, uint64_t seed, uint64_t *ops, char *report, size_t cap) {
  if (!ctx || lanes == 0 || lanes > ((size_t)1 << 24) || iters < 1 || iters > 100000) return LAMD_ERR_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  u64 *d_out = nullptr;
  HIPCHK(ctx, hipMalloc(&d_out, lanes * 8));
  hipLaunchKernelGGL(k_fuzz_field, dim3(blocks_for(lanes)), dim3(256), 0, ctx->stream, lanes, iters, (u64)seed, d_out);
  HIPCHK(ctx, hipGetLastError());
  std::vector<u64> got(lanes);
  HIPCHK(ctx, hipMemcpyAsync(got.data(), d_out, lanes * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  (void)hipFree(d_out);
  int nbad = 0;
  std::string rep;
  for (size_t i = 0; i < lanes; i++) {
    const u64 exp = fuzz_lane(seed, i, iters);
    if (exp != got[i]) {
      if (nbad < 4) rep += "lane " + std::to_string(i) + " device " + std::to_string(got[i]) + " host " + std::to_string(exp) + "; ";
      nbad++;
    }
  }
  if (ops) *ops = (uint64_t)lanes * ((uint64_t)iters * FZ_OPS_PER_ITER + FZ_OPS_TAIL);
  if (report && cap) { strncpy(report, rep.c_str(), cap - 1); report[cap - 1] = 0; }
  return nbad;
}

// ---- diagnostic peek into the engine's device work buffers (tests / debugging only)
// ---- the roofline's denominator, measured in the process that reports it (include/lightning_amd_debug.h lamd_debug_mul32_peak): a dependency-free
// stream of v_mad_u64_u32 -- eight independent 64-bit accumulators per lane, the carry-out in an SGPR pair as the multiplier's columns have it --
// on every SIMD of the chip at a given occupancy, long enough (>= min_ms per launch) for the clock governor to settle where the ecmult kernel's
// launches (3-4 ms) run.  s_memtime / s_memrealtime deltas of one wave give the counter ratio next to it.
#define LAMD_MAD8 "v_mad_u64_u32 %0, s[20:21], %8, %9, %0\n\tv_mad_u64_u32 %1, s[20:21], %8, %9, %1\n\tv_mad_u64_u32 %2, s[20:21], %8, %9, %2\n\t" \
                  "v_mad_u64_u32 %3, s[20:21], %8, %9, %3\n\tv_mad_u64_u32 %4, s[20:21], %8, %9, %4\n\tv_mad_u64_u32 %5, s[20:21], %8, %9, %5\n\t" \
                  "v_mad_u64_u32 %6, s[20:21], %8, %9, %6\n\tv_mad_u64_u32 %7, s[20:21], %8, %9, %7\n\t"
__global__ void __launch_bounds__(256) k_mul32_peak(u32 *__restrict__ out, u32 iters, u64 *__restrict__ clocks) {
  const u32 x = threadIdx.x * 2654435761u + 12345u + blockIdx.x, y = x ^ 0x9E3779B9u;
  u64 a0 = x, a1 = y, a2 = x + 1, a3 = y + 1, a4 = x + 2, a5 = y + 2, a6 = x + 3, a7 = y + 3;
  const u64 c0 = __builtin_readcyclecounter(), r0 = wall_clock64();
  for (u32 it = 0; it < iters; it++) {
#pragma unroll
    for (int r = 0; r < 16; r++)
      asm volatile(LAMD_MAD8 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(x), "v"(y) : "s20", "s21");
  }
  const u64 c1 = __builtin_readcyclecounter(), r1 = wall_clock64();
  out[blockIdx.x * blockDim.x + threadIdx.x] = (u32)(a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7);
  if (blockIdx.x == 0 && threadIdx.x == 0) { clocks[0] = c1 - c0; clocks[1] = r1 - r0; }
}
extern "C" int lamd_debug_mul32_peak(lamd_ctx *ctx, int waves_per_simd, double min_ms, int launches, double *lane_ops_per_s, double *avg_launch_ms,
                                     double *memtime_per_realtime) {
  if (!ctx || waves_per_simd < 1 || waves_per_simd > 8 || launches < 1 || !lane_ops_per_s) return LAMD_ERR_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const unsigned blocks = (unsigned)ctx->prop.multiProcessorCount * (unsigned)waves_per_simd;  // 256 threads = one wave per SIMD of a CU
  u32 *d_out = nullptr;
  u64 *d_clk = nullptr;
  HIPCHK(ctx, hipMalloc((void **)&d_out, (size_t)blocks * 256 * 4));
  if (hipMalloc((void **)&d_clk, 16) != hipSuccess) { (void)hipFree(d_out); ctx->err = "hipMalloc failed"; return LAMD_ERR_NOMEM; }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = LAMD_OK;
  auto run = [&](u32 iters, float *ms) -> bool {
    if (hipEventRecord(e0, ctx->stream) != hipSuccess) return false;
    hipLaunchKernelGGL(k_mul32_peak, dim3(blocks), dim3(256), 0, ctx->stream, d_out, iters, d_clk);
    return hipEventRecord(e1, ctx->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
  };
  float ms = 0;
  u32 iters = 2000;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || !run(200, &ms) || !run(iters, &ms)) rc = LAMD_ERR_HIP;
  if (rc == LAMD_OK) {
    if (min_ms <= 0) iters = 150;  // the sub-millisecond launch of the round-1 micro-benchmark, for comparison
    else if (ms > 0) iters = (u32)((double)iters * min_ms / ms * 1.05) + 1;
    double sum = 0, ratio = 0;
    for (int l = 0; l < launches && rc == LAMD_OK; l++) {
      if (!run(iters, &ms)) { rc = LAMD_ERR_HIP; break; }
      sum += ms;
      u64 clk[2] = {0, 0};
      if (hipMemcpy(clk, d_clk, 16, hipMemcpyDeviceToHost) == hipSuccess && clk[1]) ratio += (double)clk[0] / (double)clk[1];
    }
    if (rc == LAMD_OK) {
      const double avg = sum / launches;
      *lane_ops_per_s = (double)blocks * 256.0 * (double)iters * 128.0 / (avg * 1e-3);
      if (avg_launch_ms) *avg_launch_ms = avg;
      if (memtime_per_realtime) *memtime_per_realtime = ratio / launches;
    }
  }
  if (rc != LAMD_OK) ctx->err = "lamd_debug_mul32_peak: HIP error";
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(d_out);
  (void)hipFree(d_clk);
  return rc;
}
extern "C" const void *lamd_debug_gtable(lamd_ctx *ctx) { return ctx ? (const void *)ctx->gtable : nullptr; }
extern "C" int lamd_debug_read(lamd_ctx *ctx, int which, size_t offset, size_t nbytes, void *out) {
  if (!ctx || !out) return LAMD_ERR_ARG;
  const lamd_ctx::key_cache &kc = ctx->cache_store;
  struct span { const void *p; size_t cap; };
  const auto of = [](const devbuf &b) { return span{b.p, b.cap}; };   // (the G table is no devbuf of the context: the device's engines share it)
  const span bufs[] = {of(ctx->recs), of(ctx->keyok), of(ctx->kd_rep), of(ctx->kd_uid), of(ctx->row_ent), of(ctx->kd_uniq), of(ctx->hk[0].keyok), of(ctx->hk[0].qwords),
                       of(kc.pool7), span{ctx->gtable, ctx->gtable ? GTABLE_BYTES : 0}, of(kc.pool10), of(kc.ents)};
  if (which < 0 || which >= (int)(sizeof(bufs) / sizeof(bufs[0])) || !bufs[which].p || offset > bufs[which].cap || nbytes > bufs[which].cap - offset) {
    ctx->err = "debug_read: no such buffer / out of range";
    return LAMD_ERR_ARG;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(out, (const u8 *)bufs[which].p + offset, nbytes, hipMemcpyDeviceToHost));
  return LAMD_OK;
}

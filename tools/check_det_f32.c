/* check_det_f32.c — the accuracy of the reproducible f32 math over ALL 2^32 float32 inputs, on the host twins.
 *
 *   gcc -O2 -std=c11 -ffp-contract=off -pthread -o check_det_f32 tools/check_det_f32.c \
 *       oracle/gymrl_oracle.c oracle/lunar_oracle.c oracle/offpolicy_oracle.c -lm
 *
 * Links oracle/gymrl_oracle.c's orc_expf / orc_logf / orc_tanhf / orc_tanhf_sel / orc_sincosf (the bits of det_expf / det_logf /
 * det_tanhf / det_tanhf_sel / det_sincosf: tests/test_det_math_gpu.py) and restates nothing.  Reference: libm in double.  Per
 * function: the maximum error in ulps of the correctly rounded float32 result and the input where it occurs, over
 *   exp     -87.33654f < x <= 88.72283f (outside, the result is the documented flush to +0 / +inf)
 *   log     finite x > 0, denormals included
 *   tanh    every x that is not NaN
 *   sincos  |x| < 8000, with the maximum absolute error as well (near a zero of sin or cos the reduction's absolute error
 *           is many ulps of a tiny result)
 * and whether orc_tanhf (branchy) and orc_tanhf_sel (select) carry the same bits for every input, NaN = NaN.
 * At most 16 threads, each over a contiguous slice of the bit patterns. */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

float orc_expf(float x);
float orc_logf(float x);
float orc_tanhf(float x);
float orc_tanhf_sel(float x);
void orc_sincosf(float x, float* s, float* c);

enum { F_EXP, F_LOG, F_TANH, F_SIN, F_COS, F_COUNT };
static const char* kName[F_COUNT] = {"exp", "log", "tanh", "sin", "cos"};

typedef struct {
  uint64_t lo, hi;
  double max_ulp[F_COUNT], max_abs[F_COUNT];
  uint32_t at_ulp[F_COUNT], at_abs[F_COUNT];
  uint64_t tanh_forms_differ;
  uint32_t tanh_first_diff;
} slice_t;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* |y - d| in ulps of (float)d, the correctly rounded result */
static void score(slice_t* s, int f, uint32_t u, float y, double d) {
  const float rf = (float)d;
  double abs_err, ulps;
  if (isinf(rf) || isinf(y)) {
    abs_err = (rf == y) ? 0.0 : INFINITY;
    ulps = abs_err;
  } else {
    const float a = fabsf(rf);
    const double ulp = (double)nextafterf(a, INFINITY) - (double)a;
    abs_err = fabs((double)y - d);
    ulps = abs_err / ulp;
  }
  if (ulps > s->max_ulp[f]) { s->max_ulp[f] = ulps; s->at_ulp[f] = u; }
  if (abs_err > s->max_abs[f]) { s->max_abs[f] = abs_err; s->at_abs[f] = u; }
}

static void* run(void* arg) {
  slice_t* s = (slice_t*)arg;
  for (uint64_t v = s->lo; v < s->hi; ++v) {
    const uint32_t u = (uint32_t)v;
    const float x = as_float(u);
    const float tb = orc_tanhf(x), ts = orc_tanhf_sel(x);
    if (as_bits(tb) != as_bits(ts) && !(tb != tb && ts != ts)) {
      if (!s->tanh_forms_differ) s->tanh_first_diff = u;
      s->tanh_forms_differ++;
    }
    if (x != x) continue;
    score(s, F_TANH, u, tb, tanh((double)x));
    if (x > -87.33654f && x <= 88.72283f) score(s, F_EXP, u, orc_expf(x), exp((double)x));
    if (x > 0.0f && !isinf(x)) score(s, F_LOG, u, orc_logf(x), log((double)x));
    if (fabsf(x) < 8000.0f) {
      float sn, cs;
      orc_sincosf(x, &sn, &cs);
      score(s, F_SIN, u, sn, sin((double)x));
      score(s, F_COS, u, cs, cos((double)x));
    }
  }
  return NULL;
}

int main(void) {
  long nt = sysconf(_SC_NPROCESSORS_ONLN);
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;
  pthread_t th[16];
  slice_t sl[16];
  memset(sl, 0, sizeof sl);
  const uint64_t total = 1ull << 32;
  for (long t = 0; t < nt; ++t) {
    sl[t].lo = total * (uint64_t)t / (uint64_t)nt;
    sl[t].hi = total * (uint64_t)(t + 1) / (uint64_t)nt;
    pthread_create(&th[t], NULL, run, &sl[t]);
  }
  for (long t = 0; t < nt; ++t) pthread_join(th[t], NULL);
  slice_t m = sl[0];
  for (long t = 1; t < nt; ++t) {
    for (int f = 0; f < F_COUNT; ++f) {
      if (sl[t].max_ulp[f] > m.max_ulp[f]) { m.max_ulp[f] = sl[t].max_ulp[f]; m.at_ulp[f] = sl[t].at_ulp[f]; }
      if (sl[t].max_abs[f] > m.max_abs[f]) { m.max_abs[f] = sl[t].max_abs[f]; m.at_abs[f] = sl[t].at_abs[f]; }
    }
    if (sl[t].tanh_forms_differ && !m.tanh_forms_differ) m.tanh_first_diff = sl[t].tanh_first_diff;
    m.tanh_forms_differ += sl[t].tanh_forms_differ;
  }
  for (int f = 0; f < F_COUNT; ++f)
    printf("%-5s max %.4f ulp at x = 0x%08x (%.9g)   max abs %.4g at x = 0x%08x (%.9g)\n", kName[f], m.max_ulp[f], m.at_ulp[f],
           (double)as_float(m.at_ulp[f]), m.max_abs[f], m.at_abs[f], (double)as_float(m.at_abs[f]));
  if (m.tanh_forms_differ)
    printf("tanh  branchy and select forms DIFFER on %llu inputs, first x = 0x%08x\n", (unsigned long long)m.tanh_forms_differ,
           m.tanh_first_diff);
  else
    printf("tanh  branchy and select forms carry the same bits on all 2^32 inputs (NaN = NaN)\n");
  return m.tanh_forms_differ ? 1 : 0;
}

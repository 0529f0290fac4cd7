// offpolicy_step.hip — a whole SAC vector step (sac_pendulum.py:269-310) in five launches.
//
// Round 3's step was ~60 launches of 4-14 us each (profiles/r03_sac_kernel_stats.csv: 0.325 ms per vector step, the acting
// forward at 0.03 of the f32-MFMA peak): every Linear of a 128-row batch is ~1 us of MFMA work behind a dispatch, a first
// load from L2 and a drain.  Nothing in a forward or input-gradient pass mixes batch rows, so here ONE workgroup of 16
// waves carries a 16-row slab of the batch through a whole chain of layers — activations in LDS, weights read from L2
// in nn.Linear's own layout, a workgroup barrier between layers — and only what reduces over the batch (weight
// gradients, loss sums) sits behind a kernel boundary:
//
//   sac_act_kernel   N/16 workgroups: Actor forward, reparameterised draw, Pendulum step, replay row         (acting)
//   sac_p1_kernel    B/16 workgroups: draw + gather, target chain, Q(s, a), loss gradient, critic dX chain    (rows)
//   sac_dw_kernel    one wave per 16 x 16 weight tile: dW tile, Adam on it, soft target update; loss sums    (tiles)
//   sac_p3_kernel    B/16 workgroups: actor forward + draw, Q(s, a) of the new critic, chain back to the actor (rows)
//   sac_dw_kernel    actor tiles + Adam; loss sums; the float64 temperature step                               (tiles)
//
// Every tile is computed by the device functions of lin_device.hpp — the MFMA sequence of gymrl_lin_fwd / _bwd_input /
// _bwd_weight — and every scalar expression is the one of the stand-alone kernels it replaces (offpolicy.hip sac_*,
// optim.hip adam_one / soft update, replay.hip, env_classic_device.hpp), so parameters, Adam moments, target network,
// temperature and replay ring after a step equal the layer-by-layer path's bit for bit (tests/test_fused_step_gpu.py).
//
// TD3 / DDPG (td3_pendulum.py:171-228, ddpg_pendulum.py:150-194) run on the same stages, further down: td3_act_kernel, td3_r1_kernel,
// td3_dw_kernel (sac_dw_body behind a delayed-step word), td3_r3_kernel — one workgroup per slab and phase, no hand-off at all.
#include "env_classic_device.hpp"
#include "lin_device.hpp"

namespace {

using namespace gymrl;
using lin::act_bwd;
using lin::act_fwd;

constexpr int kWaves = 16, kThreads = 64 * kWaves;
constexpr int kMaxBatch = 8192;      // (ops.FUSED_MAX_BATCH) rows of an update: 512 slabs
constexpr int kDwMaxSlices = 32;     // lin_device.hpp bwd_weight_slices(B <= 8192, ...) <= cdiv(B, 256)

// Probe build only (make prof): 100 MHz wall-clock stamps at the stage boundaries of workgroup 0 (tools/probe_sac_stages.py)
#ifdef GYMRL_PROF_BUILD
__device__ long long g_step_prof[4][32];
#define STEP_MARK(k, i) do { if (threadIdx.x == 0 && bx == 0) g_step_prof[k][i] = (long long)wall_clock64(); } while (0)
#else
#define STEP_MARK(k, i) do {} while (0)
#endif
constexpr int kMaxD = 8, kMaxA = 4;
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;   // math.log(math.sqrt(2*math.pi))
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- hand-off between the row phases and the tile phases (caller-owned workspace) -------------------------------------
struct SacWs {
  float *s, *a;                       // [B][D], [B][A]: the gathered batch
  float *H1[2], *Z1[2], *H2[2], *Z2[2], *dq[2];      // critic net i: activations and dL/dz per layer
  float *aH1, *aZ1, *aH2, *aZ2, *dmean, *dls;        // actor
  double* terms;                      // [B][3]: per-row critic term, actor term, temperature term
  double* terms2;                     // [B]: the second Q network's critic term (its workgroup's share of terms[.][0])
  float *xtq[2], *xmisc;              // P1: the two target networks' Q(s', a') columns [16 S] and {reward, done, logp'} [16 S][4], from the
                                      // target-chain workgroups to the critic-chain workgroups (each forms y itself)
  unsigned int* sync;                 // [16]: gymrl_sac_step's phase counters (0 acting, 1 P1, 2 P2, 3 P3 done; 6 next ticket, 7 finished workgroups);
                                      // the large-batch row kernels' tickets (slab_grid: 8 / 9 P1's, 10 / 11 P3's) — all zero between launches
  unsigned int* flag;                 // [8][ceil(B / 16)]: hand-off flags (1 = waiting to be consumed; zero before the first launch, left zero):
                                      //   P1: 0 / 1 target network 1 -> critic workgroup 1 / 2, 5 / 6 target network 2 -> critic workgroup 1 / 2;
                                      //   P3: 2 / 3 Q1 / Q2, 4 the second network's dZ1 slab
  float *xa, *xq[2], *xpart;          // P3's exchanges: action [16 S][kMaxA], the two Q columns [16 S], network 1's half of the d action chain [16 S][kMaxA]
  float* dw_parts;                    // B > 512: the weight-gradient tiles' slice partials (DwArgs)
  float *xmean, *xls, *xeps, *xlp;    // the actor step's sample (mean, log_std, eps [16 S][kMaxA], logp [16 S]): P1's critic-chain workgroup
                                      // computes it while it waits for y, P3 starts from it
  __host__ __device__ static size_t carve(SacWs* w, void* base, int B, int D, int A, int H) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? reinterpret_cast<float*>(static_cast<char*>(base) + off) : nullptr; off += ((n * 4 + 255) & ~(size_t)255); return p; };
    float* s = take((size_t)B * D); float* a = take((size_t)B * A);
    float* h[16];
    for (int i = 0; i < 12; ++i) h[i] = take((size_t)B * H);
    float* dq0 = take(B); float* dq1 = take(B); float* dm = take((size_t)B * A); float* dl = take((size_t)B * A);
    double* terms = reinterpret_cast<double*>(take((size_t)B * 6));
    const size_t S16 = (size_t)(B + 15) / 16 * 16;
    double* terms2 = reinterpret_cast<double*>(take((size_t)B * 2));
    float* tq0 = take(S16); float* tq1 = take(S16); float* xmi = take(S16 * 4);
    unsigned int* fl = reinterpret_cast<unsigned int*>(take(8 * S16 / 16));
    unsigned int* sy = reinterpret_cast<unsigned int*>(take(16));
    float* xa = take(S16 * 4); float* xq0 = take(S16); float* xq1 = take(S16); float* xpart = take(S16 * 4);
    float* xm = take(S16 * 4); float* xl = take(S16 * 4); float* xe = take(S16 * 4); float* xp = take(S16);
    // weight-gradient tiles beyond 512 rows: at most 16 slices of 320 floats per tile, tiles of the larger (critic) group
    const size_t dw_tiles = B > 512 ? 2 * ((size_t)((H + 15) / 16) * ((D + A + 15) / 16) + (size_t)((H + 15) / 16) * ((H + 15) / 16) + (size_t)((H + 15) / 16)) : 0;
    float* dwp = take(dw_tiles * kDwMaxSlices * 320);
    if (w) {
      w->dw_parts = dwp;
      w->terms2 = terms2; w->xtq[0] = tq0; w->xtq[1] = tq1; w->xmisc = xmi; w->flag = fl; w->sync = sy; w->xa = xa; w->xq[0] = xq0; w->xq[1] = xq1; w->xpart = xpart;
      w->xmean = xm; w->xls = xl; w->xeps = xe; w->xlp = xp;
      w->s = s; w->a = a;
      w->H1[0] = h[0]; w->H1[1] = h[1]; w->Z1[0] = h[2]; w->Z1[1] = h[3]; w->H2[0] = h[4]; w->H2[1] = h[5]; w->Z2[0] = h[6]; w->Z2[1] = h[7];
      w->aH1 = h[8]; w->aZ1 = h[9]; w->aH2 = h[10]; w->aZ2 = h[11];
      w->dq[0] = dq0; w->dq[1] = dq1; w->dmean = dm; w->dls = dl; w->terms = terms;
    }
    return off;
  }
};

// ---- a stage = up to four independent layers over the slab; their tiles are dealt round-robin to the 16 waves -----------
// (independent layers share a stage — Q(s, a)'s forward rides along with the target chain's — because a stage costs a
// workgroup barrier and one L2 round trip for the weights whatever it computes)
struct FwdItem {
  int X, ldx, X2, ldx2, K, K1, N;          // input slab(s) in LDS (float offsets; X2 < 0: none), reduction, outputs
  const float* W; const float* b;
  int Ys, ldy; float* Yg; int ldyg;        // output slab in LDS, optional copy in global memory
  int act; float lo, hi;
  const float* Wimg;                       // forward image of W (square layers, lin_device.hpp) or nullptr: read W in place
};
__device__ __forceinline__ FwdItem fwd_item(int X, int ldx, int X2, int ldx2, int K, int K1, int N, const float* W, const float* b, int Ys,
                                            int ldy, float* Yg, int ldyg, int act, float lo = 0.0f, float hi = 0.0f, const float* Wimg = nullptr) {
  return FwdItem{X, ldx, X2, ldx2, K, K1, N, W, b, Ys, ldy, Yg, ldyg, act, lo, hi, Wimg};
}

template <int NI>
__device__ __forceinline__ void fwd_stage(float* lds, const FwdItem (&it)[NI], int row0, int nrows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  int g0 = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const FwdItem& I = it[i];
    const int ntiles = (I.N + 15) >> 4;
    for (int t = (wave - g0) & (kWaves - 1); t < ntiles; t += kWaves) {
      const int nb = t * 16;
      const f32x4 acc = I.Wimg ? lin::tile_fwd_img(lds + I.X, I.ldx, I.K >> 4, I.Wimg, t, lane)
                               : lin::tile_fwd(lds + I.X, I.ldx, I.X2 >= 0 ? lds + I.X2 : nullptr, I.ldx2, I.K, I.K1, I.W, I.N, nb, lane);
      const int n = nb + r;
      if (n < I.N) {
        const float bv = I.b ? I.b[n] : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 4 * q + g;
          const float y = act_fwd(acc[g] + bv, I.act, I.lo, I.hi);
          lds[I.Ys + row * I.ldy + n] = y;
          if (I.Yg && row < nrows) I.Yg[(size_t)(row0 + row) * I.ldyg + n] = y;
        }
      }
    }
    g0 += ntiles;
  }
}

// dX = dZ . W (+ dZb . Wb: ONE accumulator running on over a second layer — the gradient of an input two layers share);
// then dL/dz of the layer below = dX * act'(its saved output Hs).
struct BwdItem {
  int dZ, ldz, N; const float* W; int K;   // dZ slab in LDS, its width, the layer's weight [N][K]
  int dZb; const float* Wb;                // optional second (dZ, W) pair of the same shape (dZb < 0: none)
  int Hs, ldh, act_below;                  // saved output of the layer below in LDS (Hs < 0: no activation)
  int Out, ldo; float* Outg; int ldog;     // dL/dz of the layer below: LDS slab (Out < 0: none) and / or global
  const float* Wimg;                       // input-gradient image of W (square layers) or nullptr
};

template <int NI>
__device__ __forceinline__ void bwd_stage(float* lds, const BwdItem (&it)[NI], int row0, int nrows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  int g0 = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const BwdItem& I = it[i];
    const int ktiles = (I.K + 15) >> 4;
    for (int t = (wave - g0) & (kWaves - 1); t < ktiles; t += kWaves) {
      const int kb = t * 16;
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if (I.Wimg) acc = lin::tile_bwd_input_img(acc, lds + I.dZ, I.ldz, I.N >> 4, I.Wimg, t, lane);
      else acc = lin::tile_bwd_input(acc, lds + I.dZ, I.ldz, I.N, I.W, I.K, kb, lane);
      if (I.dZb >= 0) acc = lin::tile_bwd_input(acc, lds + I.dZb, I.ldz, I.N, I.Wb, I.K, kb, lane);
      const int kc = kb + r;
      if (kc < I.K) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 4 * q + g;
          float v = acc[g];
          if (I.Hs >= 0) v = v * act_bwd(lds[I.Hs + row * I.ldh + kc], I.act_below, 0.0f, 0.0f);
          if (I.Out >= 0) lds[I.Out + row * I.ldo + kc] = v;
          if (I.Outg && row < nrows) I.Outg[(size_t)(row0 + row) * I.ldog + kc] = v;
        }
      }
    }
    g0 += ktiles;
  }
}

// N(0,1) draw of the fused path when the caller passes no explicit draws: NoisyNet's Box-Muller on its own stream ids
__device__ __forceinline__ float fused_normal(uint64_t seed, uint64_t counter, uint32_t stream, uint32_t i) {
  return box_muller(seed, counter, stream, i);
}

// Actor.sample's tail for one row (offpolicy.hip sac_sample_fwd_kernel, the same expressions)
__device__ __forceinline__ void sample_row(const float* mean, const float* log_std, const float* eps, int A, float bound, float* action,
                                           float& logp) {
  float lp = 0.0f;
  for (int j = 0; j < A; ++j) {
    const float mu = mean[j], std = det_expf(log_std[j]);
    const float x = mu + std * eps[j];
    const float t = det_tanhf(x);
    action[j] = t * bound;
    const float var = std * std, log_scale = det_logf(std);
    float l = -((x - mu) * (x - mu)) / (2.0f * var) - log_scale - kLogSqrt2Pi;
    l -= det_logf(bound * (1.0f - t * t) + 1e-6f);
    lp += l;
  }
  logp = lp;
}

// The eight weight images of gymrl_sac_update_args.images (f32[8][H*H]); all null when the caller passed none or H % 16 != 0
struct Images {
  const float *af, *c1f, *c2f, *t1f, *t2f, *ab, *c1b, *c2b;
  __host__ __device__ Images(const float* base, int H) {
    const bool on = base && (H & 15) == 0;
    const size_t n = (size_t)H * H;
    af = on ? base : nullptr; c1f = on ? base + n : nullptr; c2f = on ? base + 2 * n : nullptr; t1f = on ? base + 3 * n : nullptr;
    t2f = on ? base + 4 * n : nullptr; ab = on ? base + 5 * n : nullptr; c1b = on ? base + 6 * n : nullptr; c2b = on ? base + 7 * n : nullptr;
  }
};

struct Lds {                          // float offsets of the small per-row slabs, then the [16][ld] activation slabs
  int S, S2, A, A2, Mean, Ls, Eps, Q0, Q1, Cq0, Cq1, Dq0, Dq1, Misc, big;
  __device__ Lds() {
    int o = 0;
    S = o; o += 16 * kMaxD; S2 = o; o += 16 * kMaxD; A = o; o += 16 * kMaxA; A2 = o; o += 16 * kMaxA;
    Mean = o; o += 16 * kMaxA; Ls = o; o += 16 * kMaxA; Eps = o; o += 16 * kMaxA;
    Q0 = o; o += 16 * 4; Q1 = o; o += 16 * 4; Cq0 = o; o += 16 * 4; Cq1 = o; o += 16 * 4; Dq0 = o; o += 16 * 4; Dq1 = o; o += 16 * 4; Misc = o; o += 16 * 4;
    big = o;
  }
};
constexpr int kSmallFloats = 16 * (2 * kMaxD + 5 * kMaxA + 7 * 4);

// The NARROW layers' parameters (fc1: [H][D (+ A)], the heads [A][H], fc3 [1][H], their biases) are copied into LDS slabs the
// role does not use, at the start of the kernel and under the gather's own memory round trips: a narrow stage is one dependent
// chain of <= 64 MFMAs (1 us) behind an L2 — right after a launch, HBM — round trip for its weights (1.5-2 us), and a step has a
// dozen of them on its critical path.  Same values, same order: only where the operand is read from changes.
struct Stager {
  float* lds; int at;
  int n = 0, total = 0;
  static constexpr int kMaxSeg = 12;
  const float* src[kMaxSeg]; int dst[kMaxSeg], cnt[kMaxSeg];
  __device__ __forceinline__ const float* put(const float* s, int count) {      // reserve; run() copies
    src[n] = s; dst[n] = at; cnt[n] = count; ++n;
    total += count;
    at += (count + 3) & ~3;                              // 16-byte rows for the f32x4 operand reads
    return lds + dst[n - 1];
  }
  // every segment in ONE pass over the concatenation, four elements per thread in flight (as separate loops the segments'
  // round trips followed one another: +2 us in front of the gather).  issue() requests the first pass's elements, commit()
  // writes them to LDS (and runs any further pass): what lies between the two — P1's index draw — overlaps the round trip.
  float v[4]; int d[4];
  __device__ __forceinline__ void fetch(int e0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int off = e0 + j * kThreads;
      const bool live = off < total;
      const float* p = src[0]; int base = dst[0]; bool found = false;
#pragma unroll
      for (int i = 0; i < kMaxSeg; ++i) {
        if (i < n && !found) {
          if (off < cnt[i]) { p = src[i] + off; base = dst[i] + off; found = true; }
          else off -= cnt[i];
        }
      }
      v[j] = live ? *p : 0.0f;
      d[j] = live ? base : -1;
    }
  }
  __device__ __forceinline__ void store() const {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (d[j] >= 0) lds[d[j]] = v[j];
  }
  __device__ __forceinline__ void issue() { fetch(threadIdx.x); }
  __device__ __forceinline__ void commit() {
    store();
    for (int e0 = threadIdx.x + 4 * kThreads; e0 < total; e0 += 4 * kThreads) { fetch(e0); store(); }
  }
  __device__ __forceinline__ void run() { issue(); commit(); }
};

// ======================================================================================================== P1 =====
// hand-off between the paired workgroups of a slab: the producer's data stores, a workgroup barrier, then ONE release store of
// the flag; the consumer's thread 0 spins on it (agent scope), a workgroup barrier, the data is read with agent-scope loads,
// and the consumer — the flag's only reader — clears it for the next launch
__device__ __forceinline__ void flag_post(unsigned int* f) { __hip_atomic_store(f, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
// (polling with relaxed loads and ONE acquire fence at the end: an acquire per poll invalidates the compute unit's L1 and the
// XCD's L2 lines each time round, under the workgroups that are streaming weights through them)
// Every spin in this file is BOUNDED: kSpinLimit polls (each a sleep + an L2 round trip, ~0.3-1 us: seconds in all, against
// hand-offs that take microseconds) and then a trap — the launch fails with a hardware exception and every later HIP call
// reports it, instead of a training run that hangs silently if a producer should ever not be running (see slab_grid below for
// why it always is).
constexpr unsigned int kSpinLimit = 1u << 23;
__device__ __forceinline__ void flag_wait(unsigned int* f) {
  unsigned int polls = 0;
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1u) {
    __builtin_amdgcn_s_sleep(2);
    if (++polls > kSpinLimit) __builtin_trap();
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
__device__ __forceinline__ void flag_clear(unsigned int* f) { __hip_atomic_store(f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float xload(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xstore(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// phase counters of the one-launch step (gymrl_sac_step): a workgroup that has finished a phase adds one with a release, after
// every wave has waited for its own global stores and a workgroup barrier; a workgroup of a later phase spins until the
// count is complete (acquire: what it then reads with plain loads is what the producers wrote), thread 0 for everybody
__device__ __forceinline__ void phase_done(unsigned int* c) {
  // __syncthreads() alone waits for LDS traffic only (s_waitcnt lgkmcnt(0); s_barrier): every wave first waits until its OWN
  // global stores have reached the L2 (vmcnt(0)), then the barrier, then thread 0's release writes the L2 back and publishes
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void phase_wait(const unsigned int* c, unsigned int n) {
  if (c) {
    if (threadIdx.x == 0) {
      unsigned int polls = 0;
      while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) {
        __builtin_amdgcn_s_sleep(8);
        if (++polls > kSpinLimit) __builtin_trap();
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
  }
}

// Four workgroups per 16-row slab (blockIdx.y): ONE compute unit's f32 MFMA rate is what a slab's stage costs, so every
// chain that does not depend on another runs on a compute unit of its own —
//   0 / 1  the target chain of target network 1 / 2: actor(s'), a' and logp' (both compute them: nothing is waited for), then
//          THEIR network's Q(s', a') (:233-236), posted with a release flag per consumer;
//   2 / 3  the critic chain of Q network 1 / 2: Q(s, a) (:239), then — both target columns taken — y (:237), the loss gradient
//          and the input-gradient chain of its network (:240-241).  Workgroup 2 also runs the ACTOR step's forward (:248) in
//          the time it would otherwise wait.
// All workgroups of every slab are resident (4 * B / 16 <= 64 of 256 CUs) and the producers wait for nobody: no deadlock.
// Every flag has one writer and one reader, who clears it.  Same layers, same order per element as the per-layer path.
// ring_ready / ring_n (the one-launch step): the acting workgroups of the same launch that must have written their replay rows
// before this workgroup gathers (its index draw does not wait for them)
template <int HC>
__device__ __forceinline__ void sac_p1_body(const gymrl_sac_update_args& a, const SacWs& ws, float* lds, const int bx, const int role, const int S,
                                            const unsigned int* ring_ready, unsigned int ring_n) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld, H1a = X1 + 16 * ld, H1b = H1a + 16 * ld, H2a = H1b + 16 * ld, H2b = H2a + 16 * ld;
  const int T2a = H2b + 16 * ld, T2b = T2a + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool target_chain = role < 2;
  const int n = role & 1;                                // which of the twin networks this workgroup carries
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  unsigned int* const f_t[2] = {ws.flag + (size_t)n * S + bx, ws.flag + (size_t)(5 + n) * S + bx};   // target net 1 / 2 -> critic workgroup n
#define P1_MARK_T(i) do { if (role == 0) STEP_MARK(3, i); } while (0)
#define P1_MARK_C(i) do { if (role == 2) STEP_MARK(0, i); } while (0)
  // ---- 0: index draw + ring gather (one thread per row; rows beyond the batch are zero); each workgroup takes what its chain reads ----
  P1_MARK_T(0); P1_MARK_C(0);
  // the narrow layers' parameters into slabs this role leaves free (Stager): target chain X0 / X1 / T2a busy, critic chain
  // H1a / H2a / X0 (+ T2a / T2b in the workgroup that also runs the actor step's forward)
  const float *aw0 = nullptr, *ab0 = nullptr, *aw2 = nullptr, *aw3 = nullptr, *ab2 = nullptr, *ab3 = nullptr;   // actor fc1, heads
  const float *qw0, *qb0, *qw2, *qb2;                                                                            // this role's Q network: fc1, fc3
  Stager sg{lds, target_chain ? H1a : X1};
  {
    const gymrl_sac_critic_params& net = target_chain ? a.target : a.critic;
    qw0 = sg.put(net.w[3 * n], H * (D + A)); qb0 = sg.put(net.b[3 * n], H);
    qw2 = sg.put(net.w[3 * n + 2], H); qb2 = sg.put(net.b[3 * n + 2], 1);
    if (target_chain || n == 0) {
      sg.at = H1b;
      aw0 = sg.put(a.actor.w[0], H * D); ab0 = sg.put(a.actor.b[0], H);
      sg.at = H2b;
      aw2 = sg.put(a.actor.w[2], A * H); aw3 = sg.put(a.actor.w[3], A * H);
      ab2 = sg.put(a.actor.b[2], A); ab3 = sg.put(a.actor.b[3], A);
    }
    sg.issue();
  }
  int64_t row = 0;
  if (t < nrows) {
    const int b = row0 + t;
    if (a.idx) row = a.idx[b];
    else {
      uint64_t counter = a.idx_counter; uint32_t size = (uint32_t)a.idx_size;
      if (a.idx_dev) { const uint64_t* d = static_cast<const uint64_t*>(a.idx_dev); counter = d[0]; size = (uint32_t)(int64_t)d[1]; }
      int bits = 2;
      while (((int64_t)1 << bits) < (int64_t)size) ++bits;
      row = keyed_permute((uint32_t)b, size, bits / 2, bits - bits / 2, a.idx_seed ^ 0x5265706C61794944ull, counter);
    }
  }
  sg.commit();
  phase_wait(ring_ready, ring_n);
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    if (target_chain) {
      for (int k = 0; k < kMaxD; ++k) lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      for (int j = 0; j < kMaxA; ++j) {
        float e = 0.0f;
        if (ok && j < A) e = a.eps_next ? a.eps_next[(size_t)b * A + j] : fused_normal(a.noise_seed, ncounter, 3u, (uint32_t)(b * A + j));
        lds[L.Eps + t * kMaxA + j] = e;
      }
      lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
      lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;          // dones become float32 (dqn_cartpole.py:155)
    } else {
      for (int k = 0; k < kMaxD; ++k) {
        const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
        lds[L.S + t * kMaxD + k] = sv;
        if (n == 0 && ok && k < D) ws.s[(size_t)b * D + k] = sv;
      }
      for (int j = 0; j < kMaxA; ++j) {
        const float av = (ok && j < A) ? __uint_as_float(a.r_action[row * A + j]) : 0.0f;
        lds[L.A + t * kMaxA + j] = av;
        if (n == 0 && ok && j < A) ws.a[(size_t)b * A + j] = av;
      }
    }
  }
  __syncthreads();
  if (target_chain) {
    P1_MARK_T(1);
    // ---- the actor on s' (:233) ----
    {
      const FwdItem st[1] = {fwd_item(L.S2, kD, -1, 0, D, D, H, aw0, ab0, X0, ld, nullptr, 0, R)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(2);
    {
      const FwdItem st[1] = {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.af)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(3);
    {
      const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, A, aw2, ab2, L.Mean, kA, nullptr, 0, NA),
                             fwd_item(X1, ld, -1, 0, H, H, A, aw3, ab3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
      fwd_stage<2>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(4);
    if (t < 16) {                         // a', logp' (:234)
      float lp;
      sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, lds + L.A2 + t * kMaxA, lp);
      lds[L.Misc + t * 4 + 2] = lp;
    }
    __syncthreads();
    P1_MARK_T(5);
    // ---- target Q(s', a') of this workgroup's network (:235-236) ----
    {
      const FwdItem st[1] = {fwd_item(L.S2, kD, L.A2, kA, D + A, D, H, qw0, qb0, X0, ld, nullptr, 0, R)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(6);
    {
      const FwdItem st[1] = {fwd_item(X0, ld, -1, 0, H, H, H, a.target.w[3 * n + 1], a.target.b[3 * n + 1], T2a, ld, nullptr, 0, R, 0.0f, 0.0f, n ? im.t2f : im.t1f)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(7);
    {
      const FwdItem st[1] = {fwd_item(T2a, ld, -1, 0, H, H, 1, qw2, qb2, L.Q0, 4, nullptr, 0, NA)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    P1_MARK_T(8);
    if (t < 16) {                         // (16 slots per slab: the columns are padded to whole slabs)
      xstore(ws.xtq[n] + row0 + t, lds[L.Q0 + t * 4]);
      if (n == 0) {
        for (int k = 0; k < 3; ++k) xstore(ws.xmisc + (size_t)(row0 + t) * 4 + k, lds[L.Misc + t * 4 + k]);
      }
    }
    __syncthreads();
    if (t == 0) { flag_post(ws.flag + (size_t)(n ? 5 : 0) * S + bx); flag_post(ws.flag + (size_t)(n ? 6 : 1) * S + bx); }
    P1_MARK_T(9);
    return;
  }
  P1_MARK_C(1);
  // ---- Q(s, a) of this workgroup's network (:239) ----
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, L.A, kA, D + A, D, H, qw0, qb0, H1a, ld, ws.H1[n], H, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  P1_MARK_C(2);
  {
    const FwdItem st[1] = {fwd_item(H1a, ld, -1, 0, H, H, H, a.critic.w[3 * n + 1], a.critic.b[3 * n + 1], H2a, ld, ws.H2[n], H, R, 0.0f, 0.0f, n ? im.c2f : im.c1f)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  P1_MARK_C(3);
  {
    const FwdItem st[1] = {fwd_item(H2a, ld, -1, 0, H, H, 1, qw2, qb2, L.Cq0, 4, nullptr, 0, NA)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  P1_MARK_C(4);
  // ---- while the target chains are still on their way: a, logp = Actor.sample(s) of the ACTOR step (:248).  It reads the
  // actor's parameters only, which nothing touches before P4 — so it is the work of P3 that does not have to wait for the
  // critic's update (P2), done here in the first critic workgroup's idle time; P3 starts from what is saved. ----
  if (n == 0) {
    const int AH1 = T2a, AH2 = T2b;                    // (P3's slab positions)
    if (t < 16) {
      const int b = row0 + t;
      const bool ok = t < nrows;
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      for (int j = 0; j < kMaxA; ++j) {
        float e = 0.0f;
        if (ok && j < A) e = a.eps_cur ? a.eps_cur[(size_t)b * A + j] : fused_normal(a.noise_seed, ncounter, 4u, (uint32_t)(b * A + j));
        lds[L.Eps + t * kMaxA + j] = e;
      }
    }
    {
      const FwdItem st[1] = {fwd_item(L.S, kD, -1, 0, D, D, H, aw0, ab0, AH1, ld, ws.aH1, H, R)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    {
      const FwdItem st[1] = {fwd_item(AH1, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], AH2, ld, ws.aH2, H, R, 0.0f, 0.0f, im.af)};
      fwd_stage<1>(lds, st, row0, nrows);
    }
    __syncthreads();
    {
      const FwdItem st[2] = {fwd_item(AH2, ld, -1, 0, H, H, A, aw2, ab2, L.Mean, kA, nullptr, 0, NA),
                             fwd_item(AH2, ld, -1, 0, H, H, A, aw3, ab3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
      fwd_stage<2>(lds, st, row0, nrows);
    }
    __syncthreads();
    if (t < 16) {
      float lp;
      sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, lds + L.A2 + t * kMaxA, lp);
      const size_t o = (size_t)(row0 + t) * kMaxA;
      for (int j = 0; j < kMaxA; ++j) {
        ws.xa[o + j] = lds[L.A2 + t * kMaxA + j]; ws.xmean[o + j] = lds[L.Mean + t * kMaxA + j];
        ws.xls[o + j] = lds[L.Ls + t * kMaxA + j]; ws.xeps[o + j] = lds[L.Eps + t * kMaxA + j];
      }
      ws.xlp[row0 + t] = lp;
    }
  }
  // ---- both target columns ----
  if (t == 0) { flag_wait(f_t[0]); flag_wait(f_t[1]); }
  __syncthreads();
  P1_MARK_C(5);
  if (t < 16) {
    // y (:237; offpolicy.hip sac_target_kernel), then the critic loss gradient (:240-241; sac_critic_kernel)
    const float alpha = (float)exp(a.log_alpha[0]);
    const float* mi = ws.xmisc + (size_t)(row0 + t) * 4;
    const float tq = fminf(xload(ws.xtq[0] + row0 + t), xload(ws.xtq[1] + row0 + t)) - alpha * xload(mi + 2);
    const float y = xload(mi + 0) + a.gamma * (1.0f - xload(mi + 1)) * tq;
    const float invB = 1.0f / (float)a.B;
    const float e = lds[L.Cq0 + t * 4] - y;
    const float d = 2.0f * e * invB;
    for (int k = 0; k < 4; ++k) lds[L.Dq0 + t * 4 + k] = k == 0 ? d : 0.0f;
    if (t < nrows) {
      ws.dq[n][row0 + t] = d;
      if (n == 0) ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)(e * e);       // the row's critic term = this + terms2 (P2 adds them)
      else ws.terms2[row0 + t] = (double)(e * e);
    }
  }
  __syncthreads();
  if (t == 0) { flag_clear(f_t[0]); flag_clear(f_t[1]); }                        // consumed: ready for the next launch
  P1_MARK_C(6);
  // ---- input-gradient chain of this Q network (what q.backward() computes before the weight gradients) ----
  {
    const BwdItem st[1] = {BwdItem{L.Dq0, 4, 1, qw2, H, -1, nullptr, H2a, ld, R, X0, ld, ws.Z2[n], H, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  P1_MARK_C(7);
  {
    const BwdItem st[1] = {BwdItem{X0, ld, H, a.critic.w[3 * n + 1], H, -1, nullptr, H1a, ld, R, -1, 0, ws.Z1[n], H, n ? im.c2b : im.c1b}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  P1_MARK_C(8);
#undef P1_MARK_T
#undef P1_MARK_C
}

// Grid shapes of the row kernels, and why a waiting workgroup's producer is always running.
//   B <= 256 (the reference's batch sizes): dim3(slabs, R), y = role — at most 64 workgroups of one per compute unit, every one
//   of them resident at once on the chip's 256 compute units whatever the dispatch order (the launch refuses a device with
//   fewer compute units than workgroups — slab_launch_grid takes the ticketed form there), so nobody can wait for a workgroup that is not running.
//   Larger batches (SURVEY 8(d)'s B = 4096 / 8192 lines: up to 4 x 512 workgroups on 256 compute units): a 1-D grid of
//   slabs * R blocks whose place in the launch is NOT blockIdx (HIP promises no dispatch order, and consecutive blocks go
//   round-robin to the eight XCDs) but a TICKET taken at entry (one relaxed fetch-add per workgroup): logical place v = the
//   v-th workgroup to START.  The started workgroups are therefore always the logical prefix [0, k), whatever the dispatcher
//   did.  Place v is slab v / R, slot v % R, and `order` maps slots to roles producers-first, so (a) a one-way waiter
//   (P1's critic chains, Rainbow's policy(s) pass) has a higher ticket than its producers — they started before it and wait
//   for nobody —, and (b) of two workgroups that exchange both ways (P3) only the LAST started one, place k - 1, can ever
//   wait for a partner that has not started: every other started workgroup has its whole slab running, finishes, and frees a
//   compute unit for place k.  No assumption about residency or dispatch order is left.  The last workgroup to finish zeroes
//   the two counters for the next launch (tk[0] next ticket, tk[1] finished).
struct SlabGrid { int slab, role, slabs; unsigned int* tk; };
template <int R>
__device__ __forceinline__ SlabGrid slab_grid(unsigned int* tk, const int (&order)[R]) {
  if (gridDim.y > 1) return SlabGrid{(int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, nullptr};   // all resident: y IS the role (the longest chain first)
#ifdef GYMRL_PROBE_NO_TICKETS          // A/B probe only (tools/probes): the place is blockIdx, as before round 6
  const int v0 = (int)blockIdx.x;
  return SlabGrid{v0 / R, order[v0 % R], (int)gridDim.x / R, nullptr};
#endif
  __shared__ unsigned int place;
  if (threadIdx.x == 0) place = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const int v = (int)__builtin_amdgcn_readfirstlane(place);
  return SlabGrid{v / R, order[v % R], (int)gridDim.x / R, tk};
}
__device__ __forceinline__ void slab_grid_done(const SlabGrid& g) {
  if (g.tk && threadIdx.x == 0 &&
      __hip_atomic_fetch_add(g.tk + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
    // everybody has started (they all finished): nobody takes a ticket any more; the kernel boundary publishes the stores
    __hip_atomic_store(g.tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g.tk + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
inline int device_cus() {                      // compute units of the current device (asked once per device)
  static int cus[64];
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!cus[dev] && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus[dev] = v;
  return cus[dev];
}
// the y = role form only while every workgroup has a compute unit of its own (B <= 256 on this chip: at
// most 64 of 256; a partitioned or masked device with fewer compute units takes the ticketed form instead)
__host__ inline dim3 slab_launch_grid(int slabs, int R) { return (slabs * 16 <= 256 && slabs * R <= device_cus()) ? dim3(slabs, R) : dim3(slabs * R); }

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_p1_kernel(const gymrl_sac_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[4] = {0, 1, 2, 3};                 // the two target chains wait for nobody; the critic chains wait for them
  const SlabGrid g = slab_grid<4>(ws.sync + 8, order);
  sac_p1_body<HC>(a, ws, lds, g.slab, g.role, g.slabs, nullptr, 0u);
  slab_grid_done(g);
}

// ======================================================================================================== P3 =====
// Two workgroups per slab here as well (blockIdx.y), both starting from the sample P1 saved: workgroup 0 carries Q2 and the
// way back through the actor, workgroup 1 (the helper) only Q1 — forward, backward to its first layer's dZ.  They exchange
// the two Q columns (both ways: the min's tie rule needs both) and the helper's half of d action (1 -> 0): d action is ONE
// accumulator chain over both networks in the per-layer path (Q1's terms, then Q2's), so the helper runs Q1's half and
// workgroup 0 goes on from its 16 x A partial sums.
// rows_ready / critic_ready (the one-launch step): P1's and P2's phase counters — the saved sample and slabs are P1's, the
// critic's parameters P2's; what does not need the updated critic is loaded before the second wait
template <int HC>
__device__ __forceinline__ void sac_p3_body(const gymrl_sac_update_args& a, const SacWs& ws, float* lds, const int bx, const int by, const int S,
                                            const unsigned int* rows_ready, unsigned int rows_n, const unsigned int* critic_ready, unsigned int critic_n) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld, H1a = X1 + 16 * ld, H1b = H1a + 16 * ld, H2a = H1b + 16 * ld, H2b = H2a + 16 * ld;
  const int AH1 = H2b + 16 * ld, AH2 = AH1 + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool helper = by == 1;                           // the workgroup that carries Q1 only; workgroup 0: the actor and Q2
  unsigned int* f_q[2] = {ws.flag + 2 * S + bx, ws.flag + 3 * S + bx};
  unsigned int* f_dz = ws.flag + 4 * S + bx;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  if (!helper) STEP_MARK(1, 0);
  phase_wait(rows_ready, rows_n);
  // the batch's states and the actor step's sample (a, logp, mean, log_std, eps: P1 computed them); workgroup 0 also takes the
  // actor's two activation slabs back for the way home
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (ok && k < D) ? ws.s[(size_t)b * D + k] : 0.0f;
    const size_t o = (size_t)(row0 + t) * kMaxA;
    for (int j = 0; j < kMaxA; ++j) {
      lds[L.A + t * kMaxA + j] = ws.xa[o + j];
      if (!helper) { lds[L.Mean + t * kMaxA + j] = ws.xmean[o + j]; lds[L.Ls + t * kMaxA + j] = ws.xls[o + j]; lds[L.Eps + t * kMaxA + j] = ws.xeps[o + j]; }
    }
    if (!helper) lds[L.Misc + t * 4 + 2] = ws.xlp[row0 + t];
  }
  if (!helper) {
    for (int e = t; e < 16 * H; e += kThreads) {
      const int rr = e / H, c = e % H;
      const bool ok = rr < nrows;
      lds[AH1 + rr * ld + c] = ok ? ws.aH1[(size_t)(row0 + rr) * H + c] : 0.0f;
      lds[AH2 + rr * ld + c] = ok ? ws.aH2[(size_t)(row0 + rr) * H + c] : 0.0f;
    }
  }
  phase_wait(critic_ready, critic_n);
  // the narrow layers' parameters into a slab this workgroup leaves free (Stager): its Q network's fc1 and fc3 — forward, and
  // fc1 again as the d action chain's operand — and, for the way home, the actor's heads
  const int n = helper ? 0 : 1;
  const int H1n = n ? H1b : H1a, H2n = n ? H2b : H2a, Xn = n ? X1 : X0, Qn = n ? L.Q1 : L.Q0, Dqn = n ? L.Dq1 : L.Dq0;
  Stager sg{lds, n ? H1a : H1b};
  const float* qw0 = sg.put(a.critic.w[3 * n], H * (D + A)); const float* qb0 = sg.put(a.critic.b[3 * n], H);
  const float* qw2 = sg.put(a.critic.w[3 * n + 2], H); const float* qb2 = sg.put(a.critic.b[3 * n + 2], 1);
  const float *aw2 = nullptr, *aw3 = nullptr;
  if (!helper) { sg.at = H2a; aw2 = sg.put(a.actor.w[2], A * H); aw3 = sg.put(a.actor.w[3], A * H); }
  sg.run();
  __syncthreads();
  if (!helper) STEP_MARK(1, 1);
  // ---- Q(s, a) of the critic P2 has just updated (:249-250): this workgroup's network ----
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, L.A, kA, D + A, D, H, qw0, qb0, H1n, ld, nullptr, 0, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (!helper) STEP_MARK(1, 2);
  {
    const FwdItem st[1] = {fwd_item(H1n, ld, -1, 0, H, H, H, a.critic.w[3 * n + 1], a.critic.b[3 * n + 1], H2n, ld, nullptr, 0, R, 0.0f, 0.0f, n ? im.c2f : im.c1f)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (!helper) STEP_MARK(1, 3);
  {
    const FwdItem st[1] = {fwd_item(H2n, ld, -1, 0, H, H, 1, qw2, qb2, Qn, 4, nullptr, 0, NA)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (!helper) STEP_MARK(1, 4);
  // the two Q columns meet: each workgroup posts its own, takes the other's
  if (t < 16) xstore(ws.xq[n] + row0 + t, lds[Qn + t * 4]);
  __syncthreads();
  if (t == 0) { flag_post(f_q[n]); flag_wait(f_q[1 - n]); }
  __syncthreads();
  float dlogp = 0.0f;
  if (t < 16) {                         // offpolicy.hip sac_actor_kernel
    const float other = xload(ws.xq[1 - n] + row0 + t);
    const float own = lds[Qn + t * 4];
    const float qa = n ? other : own, qc = n ? own : other;            // Q1, Q2
    const float invB = 1.0f / (float)a.B;
    const float w1 = qa < qc ? 1.0f : (qa == qc ? 0.5f : 0.0f);          // torch.min tie rule
    const float dn = n ? -(1.0f - w1) * invB : -w1 * invB;
    for (int k = 0; k < 4; ++k) lds[Dqn + t * 4 + k] = k == 0 ? dn : 0.0f;
    if (!helper) {
      const float alpha = (float)exp(a.log_alpha[0]);
      const float lp = lds[L.Misc + t * 4 + 2];
      dlogp = alpha * invB;
      if (t < nrows) {
        ws.terms[(size_t)(row0 + t) * 3 + 1] = (double)(alpha * lp - fminf(qa, qc));
        ws.terms[(size_t)(row0 + t) * 3 + 2] = (double)(lp + a.target_entropy);
      }
    }
  }
  __syncthreads();
  if (t == 0) flag_clear(f_q[1 - n]);
  if (!helper) STEP_MARK(1, 5);
  // ---- back through this workgroup's Q network to its first layer (the parameters are frozen here: no weight gradients) ----
  {
    const BwdItem st[1] = {BwdItem{Dqn, 4, 1, qw2, H, -1, nullptr, H2n, ld, R, Xn, ld, nullptr, 0, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (!helper) STEP_MARK(1, 6);
  {
    const BwdItem st[1] = {BwdItem{Xn, ld, H, a.critic.w[3 * n + 1], H, -1, nullptr, H1n, ld, R, H2n, ld, nullptr, 0, n ? im.c2b : im.c1b}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  // d action = the action columns of (dZ1_Q1 . W1_Q1 + dZ1_Q2 . W1_Q2): ONE accumulator over both networks (the layers share their
  // input), network 1's terms first.  The helper runs its half of the chain and hands the 16 x A partial sums over (wave 0's own
  // stores, published by its lane 0's release); workgroup 0 goes on from them with network 2's terms — the same MFMA sequence
  // per element as the one-workgroup chain, and 16 x A floats cross instead of a 16 x H slab.
  {
    const int lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    const bool mine = r >= D && r < D + A;
    if (helper) {
      if (wave == 0) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        acc = lin::tile_bwd_input(acc, lds + H2n, ld, H, qw0, D + A, 0, lane);
        if (mine) {
#pragma unroll
          for (int g = 0; g < 4; ++g) xstore(ws.xpart + (size_t)(row0 + 4 * q + g) * kMaxA + (r - D), acc[g]);
        }
        if (lane == 0) flag_post(f_dz);
      }
      return;
    }
    STEP_MARK(1, 7);
    if (wave == 0) {
      if (lane == 0) flag_wait(f_dz);
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if (mine) {
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = xload(ws.xpart + (size_t)(row0 + 4 * q + g) * kMaxA + (r - D));
      }
      acc = lin::tile_bwd_input(acc, lds + H2n, ld, H, qw0, D + A, 0, lane);
      if (mine) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[L.A2 + (4 * q + g) * kMaxA + (r - D)] = acc[g];
      }
      if (lane == 0) flag_clear(f_dz);
    }
  }
  __syncthreads();
  STEP_MARK(1, 8);
  if (t < 16) {                         // offpolicy.hip sac_sample_bwd_kernel, then the heads' dL/dz (log_std through its clamp)
    for (int j = 0; j < kMaxA; ++j) {
      float dm = 0.0f, dl = 0.0f;
      if (j < A) {
        const float mu = lds[L.Mean + t * kMaxA + j], ls = lds[L.Ls + t * kMaxA + j], e = lds[L.Eps + t * kMaxA + j];
        const float std = det_expf(ls);
        const float x = mu + std * e;
        const float th = det_tanhf(x);
        const float omt = 1.0f - th * th;
        const float ga = lds[L.A2 + t * kMaxA + j], gl = dlogp;
        const float dx = ga * a.bound * omt + gl * (2.0f * th * a.bound * omt / (a.bound * omt + 1e-6f));
        dm = dx;
        dl = (dx * (std * e) - gl) * act_bwd(ls, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max);
        if (t < nrows) { ws.dmean[(size_t)(row0 + t) * A + j] = dm; ws.dls[(size_t)(row0 + t) * A + j] = dl; }
      }
      lds[L.Dq0 + t * 4 + j] = dm; lds[L.Dq1 + t * 4 + j] = dl;
    }
  }
  __syncthreads();
  STEP_MARK(1, 9);
  // ---- back through the actor: heads (one summed input gradient), fc2 ----
  {
    const BwdItem st[1] = {BwdItem{L.Dq0, 4, A, aw2, H, L.Dq1, aw3, AH2, ld, R, X0, ld, ws.aZ2, H, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  STEP_MARK(1, 10);
  {
    const BwdItem st[1] = {BwdItem{X0, ld, H, a.actor.w[1], H, -1, nullptr, AH1, ld, R, -1, 0, ws.aZ1, H, im.ab}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  STEP_MARK(1, 11);
}

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_p3_kernel(const gymrl_sac_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[2] = {0, 1};                       // they exchange both ways: case (b) of slab_grid's comment
  const SlabGrid g = slab_grid<2>(ws.sync + 10, order);
  sac_p3_body<HC>(a, ws, lds, g.slab, g.role, g.slabs, nullptr, 0u, nullptr, 0u);
  slab_grid_done(g);
}

// ================================================================================================= P2 / P4 =====
struct DwSeg {
  const float* dZ; const float* X; const float* X2;
  float* W; float* b; float* Wt; float* bt;       // parameters and (critic) their target twins
  float* img_f; float* img_b; float* img_tf;      // weight images to keep in step (square layers; nullptr: none)
  int ldz, ldx, ldx2, N, K, K1, wave0;            // wave0: first global wave of this segment
  int slices, tile0;                              // waves per tile (lin_device.hpp bwd_weight_slices: 1 up to 512 rows) and the segment's first tile
};
struct DwArgs {
  DwSeg seg[6];
  int nseg, total_waves, B;
  float* parts; int phase, total_tiles;           // B > 512: [tile][slice][64 lanes][5] slice partials; phase 1 = this launch writes them (one wave per
                                                  // tile and slice), phase 2 = it adds them and takes the tiles' optimiser steps (one wave per tile); 0: up to 512 rows, one launch
  float* p; float* m; float* v;                   // flat parameter buffer and its Adam moments
  float adam[4]; const float* adam_dev;
  float omb1, beta2, omb2, eps;
  float tau, omt;
  int store_grads;                                // != 0: seg.W / seg.b are gradient DESTINATIONS (overwritten), no optimiser step
  // store_grads: segment 0 is Rainbow's stacked noisy head and its gradient is split here (lin.hip noisy_split_kernel)
  int split_heads, split_A;
  float* dw_mu[2]; float* dw_sigma[2]; float* db_mu[2]; float* db_sigma[2]; const float* w_eps[2]; const float* b_eps[2];
  // loss sums + temperature (the launch's last workgroup)
  const double* terms; int term0, nterms; double* sums;
  const double* terms_b;                          // SAC's critic term is the sum of its two workgroups' shares (nullptr: terms alone)
  int alpha_step;
  double* log_alpha; double* alpha_m; double* alpha_v; double lr_alpha, abeta1, abeta2, aeps; double alpha_bias[2];
  const double* alpha_bias_dev; double* alpha_loss;
};

// One wave per 16 x 16 tile of a weight gradient + its Adam step; the last block of the group sums the loss terms (its first
// 256 threads: the stand-alone kernels' order) and steps the temperature.  block / nblocks: this block's place in the group.
// polyak: whether the segments' target twins (Wt / bt / img_tf) are written at all — TD3's critic tiles skip them on the
// steps between two delayed ones (td3_dw_kernel); every other caller leaves it true
__device__ __forceinline__ void sac_dw_body(const DwArgs& a, const int block, const int nblocks, double (*sm)[4], const bool polyak = true) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  if (block == nblocks - 1) {
    if (a.phase == 1) return;
    // ---- the loss sums in the stand-alone kernels' order (offpolicy.hip: one row per thread, block_partials per 256 rows — a
    // single block adds its partial to the zeroed destination itself, more blocks go through finalize_kernel's second level) ----
    __shared__ double part[3][kMaxBatch / 256];
    __shared__ double fin[3];
    const int nb = (a.B + 255) / 256;
    for (int j = 0; j < nb; ++j) {
      double v[3] = {0.0, 0.0, 0.0};
      if (threadIdx.x < 256) {
        const int b = 256 * j + (int)threadIdx.x;
        if (b < a.B)
          for (int k = 0; k < a.nterms; ++k)
            v[k] += (a.terms_b && a.term0 + k == 0) ? a.terms[(size_t)b * 3] + a.terms_b[b] : a.terms[(size_t)b * 3 + a.term0 + k];
        for (int k = 0; k < a.nterms; ++k) {
          const double s = wave_sum(v[k]);
          if (lane == 0) sm[k][wave] = s;
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < a.nterms) {
        double s = 0.0;
        for (int w = 0; w < 4; ++w) s += sm[threadIdx.x][w];
        part[threadIdx.x][j] = s;
      }
      __syncthreads();
    }
    if (nb > 1) {                           // finalize_kernel: thread i takes partial i (nb <= 256), the same two-level sum again
      double v[3] = {0.0, 0.0, 0.0};
      if (threadIdx.x < 256) {
        if ((int)threadIdx.x < nb)
          for (int k = 0; k < a.nterms; ++k) v[k] += part[k][threadIdx.x];
        for (int k = 0; k < a.nterms; ++k) {
          const double s = wave_sum(v[k]);
          if (lane == 0) sm[k][wave] = s;
        }
      }
      __syncthreads();
    }
    if ((int)threadIdx.x < a.nterms) {
      double s;
      if (nb > 1) { s = 0.0; for (int w = 0; w < 4; ++w) s += sm[threadIdx.x][w]; }
      else s = part[threadIdx.x][0];
      fin[threadIdx.x] = s;
      a.sums[a.term0 + threadIdx.x] = 0.0 + s;
    }
    if (!a.alpha_step) return;
    __syncthreads();
    if (threadIdx.x == 0) {               // offpolicy.hip sac_alpha_step_kernel
      double bc1 = a.alpha_bias[0], bc2_sqrt = sqrt(a.alpha_bias[1]);
      if (a.alpha_bias_dev) { bc1 = a.alpha_bias_dev[0]; bc2_sqrt = sqrt(a.alpha_bias_dev[1]); }
      const double mean_term = (0.0 + fin[1]) / (double)a.B;
      if (a.alpha_loss) a.alpha_loss[0] = -(a.log_alpha[0] * mean_term);
      const double g = -mean_term;
      a.alpha_m[0] = a.alpha_m[0] + (g - a.alpha_m[0]) * (1.0 - a.abeta1);
      a.alpha_v[0] = a.alpha_v[0] * a.abeta2 + (1.0 - a.abeta2) * g * g;
      const double denom = sqrt(a.alpha_v[0]) / bc2_sqrt + a.aeps;
      a.log_alpha[0] = a.log_alpha[0] - (a.lr_alpha / bc1) * (a.alpha_m[0] / denom);
    }
    return;
  }
  const int gw = block * (int)(blockDim.x >> 6) + wave;
  if (gw >= (a.phase == 2 ? a.total_tiles : a.total_waves)) return;
  int si = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k) if (k < a.nseg && gw >= (a.phase == 2 ? a.seg[k].tile0 : a.seg[k].wave0)) si = k;
  const DwSeg& s = a.seg[si];
  const int S = a.phase == 0 ? 1 : s.slices;
  const int rel = gw - (a.phase == 2 ? s.tile0 : s.wave0);
  const int local = a.phase == 1 ? rel / S : rel, slice = a.phase == 1 ? rel - local * S : 0, ktiles = (s.K + 15) >> 4;
  const int nt = local / ktiles, cg = local - nt * ktiles, kb = cg * 16;
  const int kc = kb + r;
  // More than 512 rows: the tile's reduction is cut into lin.hip's slices (bwd_weight_slices).  Phase 1: ONE WAVE PER SLICE
  // leaves its partial in the workspace (a lone wave walking 4096 rows was 118 us per launch); phase 2, the next launch: one
  // wave per tile adds them in lin_slice_reduce_kernel's order and goes on with the tile's optimiser step.  (A single launch
  // with a counter per tile — the last wave to arrive reduces — was built first and measured 2.4 x SLOWER: every agent-scope
  // release / acquire writes back and invalidates an XCD's L2, and 13 000 waves did one each.)
  f32x4 sl_acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float sl_col = 0.0f;
  if (a.phase == 1) {
    const int rps = lin::bwd_weight_rows_per_slice(a.B, S), b0 = slice * rps, rows = a.B - b0 < rps ? a.B - b0 : rps;
    f32x4 part = {0.0f, 0.0f, 0.0f, 0.0f};
    float pc = 0.0f;
    if (rows > 0)
      part = lin::tile_bwd_weight(s.dZ + (size_t)b0 * s.ldz, s.ldz, s.N, nt, s.X + (size_t)b0 * s.ldx, s.ldx,
                                  s.X2 ? s.X2 + (size_t)b0 * s.ldx2 : nullptr, s.ldx2, s.K, s.K1, kb, rows, lane, pc);
    float* mine = a.parts + ((size_t)(s.tile0 + local) * kDwMaxSlices + slice) * 320;   // (segments differ in S: a fixed pitch per tile)
    *reinterpret_cast<f32x4*>(mine + 4 * lane) = part;
    mine[256 + lane] = pc;
    return;
  }
  if (a.phase == 2) {
    const int each = (S + 7) / 8;
    for (int g = 0; g < 8; ++g) {
      f32x4 gs = {0.0f, 0.0f, 0.0f, 0.0f};
      float gc = 0.0f;
      for (int k = g * each; k < (g + 1) * each && k < S; ++k) {
        const float* src = a.parts + ((size_t)(s.tile0 + local) * kDwMaxSlices + k) * 320;
        gs += *reinterpret_cast<const f32x4*>(src + 4 * lane);
        gc += src[256 + lane];
      }
      if (g == 0) { sl_acc = gs; sl_col = gc; }
      else { sl_acc += gs; sl_col += gc; }
    }
  }
  // the optimiser's state of this tile (parameter, both moments, the target twin) is requested BEFORE the gradient's own
  // loads and MFMA chain: behind them it was a second memory round trip per tile
  lin::AdamScalars ad;
  ad.step_size = a.adam_dev ? a.adam_dev[0] : a.adam[0];
  ad.bc2_sqrt = a.adam_dev ? a.adam_dev[2] : a.adam[2];
  ad.omb1 = a.omb1; ad.beta2 = a.beta2; ad.omb2 = a.omb2; ad.eps = a.eps;
  float Pv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Mv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Vv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!a.store_grads && kc < s.K) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int no = nt * 16 + 4 * q + g;
      if (no >= s.N) continue;
      const size_t o = (size_t)no * s.K + kc;
      const size_t po = (size_t)(s.W - a.p) + o;
      Pv[g] = s.W[o]; Mv[g] = a.m[po]; Vv[g] = a.v[po];
      if (s.Wt && polyak) Tv[g] = s.Wt[o];
    }
  }
  float colsum = sl_col;
  const f32x4 acc = a.phase == 2 ? sl_acc : lin::tile_bwd_weight(s.dZ, s.ldz, s.N, nt, s.X, s.ldx, s.X2, s.ldx2, s.K, s.K1, kb, a.B, lane, colsum);
  if (a.store_grads && a.split_heads && si == 0) {
    // d mu = dW, d sigma = dW * eps, per NoisyLinear layer: rows 0 .. A-1 the advantage stream, row A the value stream
    if (kc < s.K) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int no = nt * 16 + 4 * q + g;
        if (no >= s.N) continue;
        const int l = no < a.split_A ? 0 : 1, n = no - (l ? a.split_A : 0);
        const size_t o = (size_t)n * s.K + kc;
        a.dw_mu[l][o] = acc[g];
        a.dw_sigma[l][o] = acc[g] * a.w_eps[l][o];
      }
    }
    const int nn = nt * 16 + r;
    if (cg == 0 && q == 0 && nn < s.N) {
      const int l = nn < a.split_A ? 0 : 1, n = nn - (l ? a.split_A : 0);
      a.db_mu[l][n] = colsum;
      a.db_sigma[l][n] = colsum * a.b_eps[l][n];
    }
    return;
  }
  if (a.store_grads) {                            // Rainbow: clip_grad_norm_ needs every gradient before Adam may run
    if (kc < s.K) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int no = nt * 16 + 4 * q + g;
        if (no < s.N) s.W[(size_t)no * s.K + kc] = acc[g];
      }
    }
    const int nn = nt * 16 + r;
    if (cg == 0 && q == 0 && nn < s.N && s.b) s.b[nn] = colsum;
    return;
  }
  if (kc < s.K) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int no = nt * 16 + 4 * q + g;
      if (no >= s.N) continue;
      const size_t o = (size_t)no * s.K + kc;
      const size_t po = (size_t)(s.W - a.p) + o;
      float P = Pv[g], M = Mv[g], V = Vv[g];
      lin::adam_elem(P, acc[g], M, V, ad);
      s.W[o] = P; a.m[po] = M; a.v[po] = V;
      float T = 0.0f;
      if (s.Wt && polyak) { T = a.tau * P + a.omt * Tv[g]; s.Wt[o] = T; }
      const int steps = s.K >> 4;
      if (s.img_f) s.img_f[lin::img_fwd_index(no, kc, steps)] = P;
      if (s.img_b) s.img_b[lin::img_bwd_index(no, kc, steps)] = P;
      if (s.img_tf && polyak) s.img_tf[lin::img_fwd_index(no, kc, steps)] = T;
    }
  }
  const int n = nt * 16 + r;
  if (cg == 0 && q == 0 && n < s.N && s.b) {
    const size_t po = (size_t)(s.b - a.p) + n;
    float P = s.b[n], M = a.m[po], V = a.v[po];
    lin::adam_elem(P, colsum, M, V, ad);
    s.b[n] = P; a.m[po] = M; a.v[po] = V;
    if (s.bt && polyak) s.bt[n] = a.tau * P + a.omt * s.bt[n];
  }
}

__global__ __launch_bounds__(256) void sac_dw_kernel(const DwArgs a) {
  __shared__ double sm[3][4];
  sac_dw_body(a, blockIdx.x, gridDim.x, sm);
}
// one launch up to 512 rows; beyond: the slice partials, then their ordered sums + the tiles' epilogues + the loss sums
static void launch_dw(DwArgs d, hipStream_t stream) {
  hipLaunchKernelGGL(sac_dw_kernel, dim3((d.total_waves + 3) / 4 + 1), dim3(256), 0, stream, d);
  if (d.phase == 1) {
    d.phase = 2;
    hipLaunchKernelGGL(sac_dw_kernel, dim3((d.total_tiles + 3) / 4 + 1), dim3(256), 0, stream, d);
  }
}

// ==================================================================================================== acting =====
template <int HC>
__device__ __forceinline__ void sac_act_body(const gymrl_sac_act_args& a, float* lds, const int bx) {
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);      // HC: the hidden width this instance is built for (0: any)
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  STEP_MARK(2, 0);
  Stager sg{lds, X1 + 16 * ld};                          // (slabs 2, 3)
  const float* w0 = sg.put(a.actor.w[0], H * D); const float* b0 = sg.put(a.actor.b[0], H);
  const float* w2 = sg.put(a.actor.w[2], A * H); const float* w3 = sg.put(a.actor.w[3], A * H);
  const float* b2 = sg.put(a.actor.b[2], A); const float* b3 = sg.put(a.actor.b[3], A);
  sg.run();
  if (t < 16) {
    const int i = row0 + t;
    const bool ok = t < nrows;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (ok && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
    const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
    for (int j = 0; j < kMaxA; ++j) {
      float e = 0.0f;
      if (ok && j < A) e = a.eps ? a.eps[(size_t)i * A + j] : fused_normal(a.noise_seed, ncounter, 2u, (uint32_t)(i * A + j));
      lds[L.Eps + t * kMaxA + j] = e;
    }
  }
  __syncthreads();
  STEP_MARK(2, 1);
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const Images im(a.images, H);
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, -1, 0, D, D, H, w0, b0, X0, ld, nullptr, 0, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  STEP_MARK(2, 2);
  {
    const FwdItem st[1] = {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.af)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  STEP_MARK(2, 3);
  {
    const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, A, w2, b2, L.Mean, kA, nullptr, 0, GYMRL_ACT_NONE),
                           fwd_item(X1, ld, -1, 0, H, H, A, w3, b3, L.Ls, kA, nullptr, 0, GYMRL_ACT_CLAMP, a.log_std_min, a.log_std_max)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  STEP_MARK(2, 4);
  // one lane per env: draw, Pendulum step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    const bool ok = t < nrows;
    ClassicStep<3> r;
    r.done = false; r.ret = 0.0; r.len = 0;
    if (ok) {
      const int i = row0 + t;
      float act[kMaxA], lp;
      sample_row(lds + L.Mean + t * kMaxA, lds + L.Ls + t * kMaxA, lds + L.Eps + t * kMaxA, A, a.bound, act, lp);
      const PendulumState st(a.env_state, a.N);
      pendulum_step_one(st, i, a.env_seed, a.env_id0, act[0], r);
      const int64_t cursor = a.cursor_dev ? a.cursor_dev[0] : a.cursor;
      const int64_t row = (cursor + i) % a.cap;
      for (int k = 0; k < D; ++k) {
        a.r_state[row * D + k] = lds[L.S + t * kMaxD + k];
        a.r_next[row * D + k] = r.o_term[k];              // the TERMINAL observation is what the buffer keeps (:283)
        a.obs_out[(size_t)i * D + k] = r.o_next[k];
      }
      for (int j = 0; j < A; ++j) {
        a.r_action[row * A + j] = __float_as_uint(act[j]);
        if (a.action_out) a.action_out[(size_t)i * A + j] = act[j];
      }
      a.r_reward[row] = r.reward;
      a.r_flag[row] = r.done;                             // done = terminated or truncated
      if (a.rew_out) a.rew_out[i] = r.reward;
      if (a.done_out) a.done_out[i] = r.done;
      if (r.done && a.ep_ret_out) a.ep_ret_out[i] = (float)r.ret;
    }
    accumulate_ep_stats(a.ep_stats, r.done && ok, r.ret, r.len);
  }
  STEP_MARK(2, 5);
}

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_act_kernel(const gymrl_sac_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  sac_act_body<HC>(a, lds, blockIdx.x);
}

// ======================================================================================== the step as ONE launch =====
// gymrl_sac_step: acting + env step + replay rows, then the whole update, in one grid.  Block ranges are the five phases in
// order (acting | P1: 4 per slab | P2: critic tiles | P3: 2 per slab | P4: actor tiles); a phase that needs an earlier one
// complete spins on that phase's counter (phase_wait) — a launch boundary's 3-4 us become ~1 us, and what a phase can do
// before it needs its predecessor (P1's index draw: 6 Philox-keyed Feistel rounds; P3's loads of the saved sample and the
// actor's slabs) is hidden behind it.  No deadlock: the acting blocks wait for nobody, every wait is on an earlier range, and
// the blocks that can wait (at most 4 + 2 per slab + the tile blocks: < 150 at B = 256) are fewer than the 256 compute units,
// so whatever order the dispatcher takes, the blocks a waiter needs get a unit.  The last block to finish (a ticket) clears
// the counters: the workspace is as zero after the launch as before it.
struct SacStepArgs {
  gymrl_sac_act_args act; gymrl_sac_update_args upd; SacWs ws; DwArgs c, p;
  int n_act, slabs, c_blocks, p_blocks;
};
static_assert(sizeof(SacStepArgs) <= 4096, "kernel arguments");

template <int HC>
__global__ __launch_bounds__(kThreads) void sac_step_kernel(const SacStepArgs by_value) {
  // read in place from the kernel-argument segment (the struct is the first argument): as a by-value object the dynamic
  // indices into its pointer tables made hipcc copy all of it into every lane's scratch (3.5 KB per lane)
  const SacStepArgs& s = *(const SacStepArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double sm[3][4];
  unsigned int* const sync = s.ws.sync;
  const int S = s.slabs;
  // the block's place in the launch is the order in which it STARTED (a ticket), not blockIdx: every phase_wait / flag_wait
  // below waits for places lower than its own or — P1's / P3's pairs — for a place at most 3 S (48) higher, whose
  // workgroups start as the earlier ones finish (slab_grid's argument: the started places are always a prefix)
  __shared__ unsigned int place;
  if (threadIdx.x == 0) place = __hip_atomic_fetch_add(sync + 6, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  int b = (int)__builtin_amdgcn_readfirstlane(place);
  if (b < s.n_act) {
    sac_act_body<HC>(s.act, lds, b);
    phase_done(sync + 0);
  } else if ((b -= s.n_act) < 4 * S) {
    const int role = b / S;
    sac_p1_body<HC>(s.upd, s.ws, lds, b - role * S, role, S, sync + 0, (unsigned)s.n_act);
    if (role >= 2) phase_done(sync + 1);
  } else if ((b -= 4 * S) < s.c_blocks) {
    [[maybe_unused]] const int bx = b;                 // (probe build: stamps of the group's first block)
    STEP_MARK(2, 16);
    phase_wait(sync + 1, 2u * S);
    STEP_MARK(2, 17);
    sac_dw_body(s.c, b, s.c_blocks, sm);
    phase_done(sync + 2);
    STEP_MARK(2, 18);
  } else if ((b -= s.c_blocks) < 2 * S) {
    const int by = b / S;
    sac_p3_body<HC>(s.upd, s.ws, lds, b - by * S, by, S, sync + 1, 2u * S, sync + 2, (unsigned)s.c_blocks);
    if (by == 0) phase_done(sync + 3);
  } else {
    b -= 2 * S;
    [[maybe_unused]] const int bx = b;
    STEP_MARK(2, 19);
    phase_wait(sync + 3, (unsigned)S);
    STEP_MARK(2, 20);
    sac_dw_body(s.p, b, s.p_blocks, sm);
    STEP_MARK(2, 21);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(sync + 7, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      for (int k = 0; k < 4; ++k) __hip_atomic_store(sync + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(sync + 6, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(sync + 7, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ============================================================================================== Rainbow =====
struct RbWs {
  float *s, *h1, *h2, *dS, *dZ2, *dZ1;      // [B][D], [B][H], [B][H], [B][A+1], [B][H], [B][H]
  double* terms;                             // [B][3] (column 0: w * td^2)
  float* xz;                                 // [2][16 S][4]: head outputs of policy(s') and target(s') on their way to the policy(s) workgroup
  unsigned int* flag;                        // [2][S]: their hand-off flags (zero before the first launch, left zero)
  unsigned int* tk;                          // [2]: slab_grid's next ticket / finished count of the large-batch row kernel (zero between launches)
  float* dw_parts;                           // B > 512: the weight-gradient tiles' slice partials (DwArgs)
  __host__ __device__ static size_t carve(RbWs* w, void* base, int B, int D, int A, int H) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? reinterpret_cast<float*>(static_cast<char*>(base) + off) : nullptr; off += ((n * 4 + 255) & ~(size_t)255); return p; };
    float* s_ = take((size_t)B * D); float* h1 = take((size_t)B * H); float* h2 = take((size_t)B * H); float* dS = take((size_t)B * (A + 1));
    float* z2 = take((size_t)B * H); float* z1 = take((size_t)B * H);
    double* terms = reinterpret_cast<double*>(take((size_t)B * 6));
    const size_t S16 = (size_t)(B + 15) / 16 * 16;
    float* xz = take(2 * S16 * 4);
    unsigned int* fl = reinterpret_cast<unsigned int*>(take(2 * S16 / 16));
    unsigned int* tk = reinterpret_cast<unsigned int*>(take(2));
    const size_t dw_tiles = B > 512 ? (size_t)((A + 1 + 15) / 16) * ((H + 15) / 16) + (size_t)((H + 15) / 16) * ((H + 15) / 16) + (size_t)((H + 15) / 16) * ((D + 15) / 16) : 0;
    float* dwp = take(dw_tiles * kDwMaxSlices * 320);
    if (w) { w->s = s_; w->h1 = h1; w->h2 = h2; w->dS = dS; w->dZ2 = z2; w->dZ1 = z1; w->terms = terms; w->xz = xz; w->flag = fl;
             w->tk = tk; w->dw_parts = dwp; }
    return off;
  }
};

// The dueling combination of one row (lin.hip lin_fwd_kernel's GYMRL_ACT_DUELING epilogue): z[0 .. A-1] = advantage stream,
// z[A] = value stream -> q[k] = value + (z[k] - mean(advantage)); returns the greedy action (first index of the maximum).
// The epilogue sums the advantages with a 16-lane butterfly over zero-padded lanes: ((z0 + z1) + (z2 + 0)) for A <= 3.
__device__ __forceinline__ int dueling_row(const float* z, int A, float* q) {
  const float z0 = z[0], z1 = A > 1 ? z[1] : 0.0f, z2 = A > 2 ? z[2] : 0.0f;
  const float sum = (z0 + z1) + (z2 + 0.0f);
  const float v = z[A];
  int bi = 0;
  float best = 0.0f;
  for (int k = 0; k < A; ++k) {
    const float qv = v + (z[k] - sum / (float)A);
    q[k] = qv;
    if (k == 0 || qv > best) { best = qv; bi = k; }
  }
  return bi;
}

constexpr int kRbMaxA = 3;

// Three workgroups per 16-row slab (blockIdx.y): policy(s) — the pass the gradient flows through —, policy(s') and target(s')
// are independent chains until the double-DQN target meets the TD error (:320-334), and a slab's stage costs what ONE compute
// unit's f32 MFMA rate makes of its items (three 256 x 256 layers per stage on one CU before).  Workgroups 1 and 2 publish
// their head outputs ([16][4]) with release flags; workgroup 0, whose own forward takes as long, consumes them, clears the
// flags and runs the loss and the way back.  The producers wait for nobody and come first in the launch (slab_grid: y / slot
// 0, 1 -> passes 1, 2; the waiting pass 0 last), so the pass that waits always finds its producers started.
template <int HC>                       // HC: the hidden width this instance is built for (0: any), as the SAC kernels'
__device__ __forceinline__ void rainbow_rows_body(const gymrl_rainbow_update_args& a, const RbWs& ws, float* lds, const SlabGrid& sg_) {
  const Lds L;
  const int D = a.D, A = a.A, A1 = a.A + 1, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int H1 = L.big, H2 = H1 + 16 * ld, X0 = H2 + 16 * ld;
  // head outputs of the three passes: [16][4] slabs in the small area (Q0, Q1, Cq0), dS in Dq0
  const int Za = L.Q0, Zb = L.Q1, Zc = L.Cq0, DS = L.Dq0;
  const int bx = sg_.slab;
  const int row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int pass = sg_.role;            // 0: policy(s) [second draw], 1: policy(s') [first draw], 2: target(s') [means]
  const int S = sg_.slabs;
  if (t < 16) {                         // gather (replay.hip replay_gather_kernel): what this workgroup's pass reads
    const int b = row0 + t;
    const bool ok = t < nrows;
    const int64_t row = ok ? a.idx[b] : 0;
    const float* src = pass == 0 ? a.r_state : a.r_next;
    for (int k = 0; k < kMaxD; ++k) {
      const float sv = (ok && k < D) ? src[row * D + k] : 0.0f;
      lds[L.S + t * kMaxD + k] = sv;
      if (pass == 0 && ok && k < D) ws.s[(size_t)b * D + k] = sv;
    }
    if (pass == 0) {
      lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
      lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;
      lds[L.Misc + t * 4 + 2] = ok ? __int_as_float((int)a.r_action[row]) : 0.0f;
      lds[L.Misc + t * 4 + 3] = (ok && a.is_weight) ? a.is_weight[b] : 1.0f;
    }
  }
  __syncthreads();
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD;
  const size_t hw = (size_t)A1 * H;
  const bool tgt = pass == 2;
  const int hslot = pass == 0 ? 2 : (pass == 1 ? 0 : 1);            // the stacked heads: first draw | target means | second draw
  const int Zme = pass == 0 ? Zc : (pass == 1 ? Za : Zb);
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, -1, 0, D, D, H, tgt ? a.t_fc1_w : a.p_fc1_w, tgt ? a.t_fc1_b : a.p_fc1_b, H1, ld, pass == 0 ? ws.h1 : nullptr, H, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(H1, ld, -1, 0, H, H, H, tgt ? a.t_fc2_w : a.p_fc2_w, tgt ? a.t_fc2_b : a.p_fc2_b, H2, ld, pass == 0 ? ws.h2 : nullptr, H, R,
                                    0.0f, 0.0f, tgt ? a.t_fc2_img_f : a.p_fc2_img_f)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(H2, ld, -1, 0, H, H, A1, a.head_w + hslot * hw, a.head_b + hslot * A1, Zme, 4, nullptr, 0, NA)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (pass != 0) {                      // the head outputs go to workgroup 0
    float* xz = ws.xz + ((size_t)(pass - 1) * S * 16 + row0) * 4;
    if (t < 64) xstore(xz + t, lds[Zme + t]);
    __syncthreads();
    if (t == 0) flag_post(ws.flag + (pass - 1) * S + bx);
    return;
  }
  if (t == 0) { flag_wait(ws.flag + bx); flag_wait(ws.flag + S + bx); }
  __syncthreads();
  if (t < 64) {
    lds[Za + t] = xload(ws.xz + ((size_t)row0) * 4 + t);
    lds[Zb + t] = xload(ws.xz + ((size_t)S * 16 + row0) * 4 + t);
  }
  __syncthreads();
  if (t == 0) { flag_clear(ws.flag + bx); flag_clear(ws.flag + S + bx); }
  if (t < 16) {
    // dueling heads, the double-DQN target and the IS-weighted loss gradient (offpolicy.hip dqn_td_kernel), dueling backward (lin.hip)
    float q_no[kRbMaxA], q_nt[kRbMaxA], q[kRbMaxA];
    const int astar = dueling_row(lds + Za + t * 4, A, q_no);
    dueling_row(lds + Zb + t * 4, A, q_nt);
    dueling_row(lds + Zc + t * 4, A, q);
    const float invB = 1.0f / (float)a.B;
    const float nq = q_nt[astar];
    const float y = lds[L.Misc + t * 4 + 0] + a.gamma_n * nq * (1.0f - lds[L.Misc + t * 4 + 1]);
    const int act = __float_as_int(lds[L.Misc + t * 4 + 2]);
    const float td = q[act] - y;
    const float wb = lds[L.Misc + t * 4 + 3];
    float dq[kRbMaxA], sum = 0.0f;
    for (int k = 0; k < A; ++k) { dq[k] = (k == act) ? (2.0f * td) * wb * invB : 0.0f; sum += dq[k]; }
    const float m = sum / (float)A;
    for (int k = 0; k < 4; ++k) {
      const float v = k < A ? dq[k] - m : (k == A ? sum : 0.0f);
      lds[DS + t * 4 + k] = v;
      if (t < nrows && k < A1) ws.dS[(size_t)(row0 + t) * A1 + k] = v;
    }
    if (t < nrows) {
      a.td_out[row0 + t] = td;
      ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)((td * td) * wb);
    }
  }
  __syncthreads();
  // loss.backward() of this pass: head -> fc2 (the input gradients; the weight gradients are the tile launch's)
  {
    const BwdItem st[1] = {BwdItem{DS, 4, A1, a.head_w + 2 * hw, H, -1, nullptr, H2, ld, R, X0, ld, ws.dZ2, H, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[1] = {BwdItem{X0, ld, H, a.p_fc2_w, H, -1, nullptr, H1, ld, R, -1, 0, ws.dZ1, H, a.p_fc2_img_b}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
}

template <int HC>
__global__ __launch_bounds__(kThreads) void rainbow_rows_kernel(const gymrl_rainbow_update_args a, const RbWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int order[3] = {1, 2, 0};                    // policy(s') and target(s') first: pass 0 waits for them
  const SlabGrid g = slab_grid<3>(ws.tk, order);
  rainbow_rows_body<HC>(a, ws, lds, g);
  slab_grid_done(g);
}

// Greedy acting on the noisy Q + CartPole + the n-step window: one lane per env after the network.  NS slabs of 16 envs per
// workgroup: at N = 8192 the 16-row form is 512 workgroups = two rounds over the 256 compute units, each streaming every
// weight again (45 us per launch); 32 rows per workgroup stream them once for two MFMA chains.
template <int NS>
__device__ __forceinline__ void act_layer(float* lds, int X, int ldx, int K, const float* W, const float* b, int N, int Ys, int ldy, int act,
                                          const float* Wimg = nullptr) {       // Wimg: forward image of a square W (K == N, % 16)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += kWaves) {
    const int nb = t * 16;
    f32x4 acc[2];
    if (Wimg) {
      if (NS == 2) lin::tile_fwd_img_x2_t<0>(lds + X, lds + X + 16 * ldx, ldx, K >> 4, Wimg, t, lane, acc[0], acc[1]);
      else acc[0] = lin::tile_fwd_img(lds + X, ldx, K >> 4, Wimg, t, lane);
    } else if (NS == 2) lin::tile_fwd_x2(lds + X, lds + X + 16 * ldx, ldx, K, W, N, nb, lane, acc[0], acc[1]);
    else acc[0] = lin::tile_fwd(lds + X, ldx, nullptr, 0, K, K, W, N, nb, lane);
    const int n = nb + r;
    if (n < N) {
      const float bv = b ? b[n] : 0.0f;
#pragma unroll
      for (int sl = 0; sl < NS; ++sl)
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[Ys + (16 * sl + 4 * q + g) * ldy + n] = act_fwd(acc[sl][g] + bv, act, 0.0f, 0.0f);
    }
  }
}

template <int NS, int HC>
__global__ __launch_bounds__(kThreads) void rainbow_act_kernel(const gymrl_rainbow_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kRows = 16 * NS;
  const int D = a.D, A = a.A, A1 = a.A + 1, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int S = 0, Q = S + kRows * kMaxD, X0 = Q + kRows * 4, X1 = X0 + kRows * ld;
  const int row0 = blockIdx.x * kRows, nrows = min(kRows, a.N - row0);
  const int t = threadIdx.x;
  if (t < kRows) {
    const int i = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[S + t * kMaxD + k] = (t < nrows && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
  act_layer<NS>(lds, S, kMaxD, D, a.fc1_w, a.fc1_b, H, X0, ld, GYMRL_ACT_RELU);
  __syncthreads();
  act_layer<NS>(lds, X0, ld, H, a.fc2_w, a.fc2_b, H, X1, ld, GYMRL_ACT_RELU, a.fc2_img);
  __syncthreads();
  act_layer<NS>(lds, X1, ld, H, a.head_w, a.head_b, A1, Q, 4, GYMRL_ACT_NONE);
  __syncthreads();
  if (t < 64) {
    const bool ok = t < nrows;
    ClassicStep<4> r;
    r.done = false; r.ret = 0.0; r.len = 0;
    if (ok) {
      const int e = row0 + t;
      float q[kRbMaxA];
      const int act = dueling_row(lds + Q + t * 4, A, q);
      const CartPoleState st(a.env_state, a.N);
      cartpole_step_one(st, e, a.env_seed, a.env_id0, act, r);
      for (int k = 0; k < D; ++k) a.obs_out[(size_t)e * D + k] = r.o_next[k];
      if (a.action_out) a.action_out[e] = act;
      if (a.rew_out) a.rew_out[e] = r.reward;
      if (a.done_out) a.done_out[e] = r.done;
      if (r.done && a.ep_ret_out) a.ep_ret_out[e] = (float)r.ret;
      // ---- replay.hip nstep_push_kernel for env e (deque.append :186-187, _get_n_step_transition :207-218) ----
      const int N = a.N, n_steps = a.n_steps;
      int64_t pushes = a.pushes, cursor = a.cursor;
      if (a.push_dev) { pushes = a.push_dev[0]; cursor = a.push_dev[1]; }
      const int slot = (int)(pushes % n_steps);
      const bool emit = pushes + 1 >= n_steps;
      const size_t so = (size_t)slot * N + e;
      for (int k = 0; k < D; ++k) {
        a.w_state[so * D + k] = lds[S + t * kMaxD + k];
        a.w_next[so * D + k] = r.o_term[k];
      }
      a.w_action[so] = act; a.w_reward[so] = r.reward;
      // :376 terminal = done and step != max_steps_per_episode - 1, by the step INDEX inside the episode
      const uint8_t term_now = (uint8_t)((r.done && r.len != a.max_episode_steps) ? 1 : 0);
      a.w_terminal[so] = term_now;
      a.w_done[so] = r.done;
      if (emit) {
        const int oldest = (slot + 1) % n_steps;
        int src = slot;
        double Rr = 0.0;
        for (int i = n_steps - 1; i >= 0; --i) {
          const int sidx = (oldest + i) % n_steps;
          const size_t o = (size_t)sidx * N + e;
          // this push's own slot comes from the registers that have just been stored (same lane)
          const bool dn = sidx == slot ? r.done : (a.w_done[o] != 0);
          const float rw = sidx == slot ? r.reward : a.w_reward[o];
          const double d = dn ? 1.0 : 0.0;
          Rr = (double)rw + a.gamma * (1.0 - d) * Rr;
          if (dn) src = sidx;
        }
        const int64_t row = (cursor + e) % a.cap;
        const size_t oo = (size_t)oldest * N + e, ss = (size_t)src * N + e;
        for (int k = 0; k < D; ++k) {
          a.r_state[row * D + k] = oldest == slot ? lds[S + t * kMaxD + k] : a.w_state[oo * D + k];
          a.r_next[row * D + k] = src == slot ? r.o_term[k] : a.w_next[ss * D + k];
        }
        a.r_action[row] = (uint32_t)(oldest == slot ? act : a.w_action[oo]);
        a.r_reward[row] = (float)Rr;
        a.r_flag[row] = src == slot ? term_now : a.w_terminal[ss];
      }
    }
    accumulate_ep_stats(a.ep_stats, r.done && ok, r.ret, r.len);
  }
}

inline bool rb_shape_ok(int B, int D, int A, int H) {
  return B > 0 && B <= kMaxBatch && D > 0 && D <= kMaxD && A > 0 && A <= kRbMaxA && H >= 4 && H <= 256 && (H & 3) == 0;
}

// All eight images from the parameters as they are (after load_state_dict / a checkpoint / a hard target copy)
__global__ __launch_bounds__(256) void sac_pack_kernel(const gymrl_sac_update_args a) {
  const int H = a.H, steps = H >> 4;
  const size_t hh = (size_t)H * H;
  const float* src[8] = {a.actor.w[1], a.critic.w[1], a.critic.w[4], a.target.w[1], a.target.w[4], a.actor.w[1], a.critic.w[1], a.critic.w[4]};
  const int which = blockIdx.y;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < hh; o += (size_t)gridDim.x * 256) {
    const int n = (int)(o / H), k = (int)(o % H);
    const float v = src[which][o];
    a.images[which * hh + (which < 5 ? lin::img_fwd_index(n, k, steps) : lin::img_bwd_index(n, k, steps))] = v;
  }
}

inline bool sac_shape_ok(int B, int D, int A, int H) {
  return B > 0 && B <= kMaxBatch && D > 0 && D <= kMaxD && A > 0 && A <= kMaxA && H >= 4 && H <= 256 && (H & 3) == 0;
}
inline size_t lds_bytes(int H, int slabs) { return sizeof(float) * (size_t)(kSmallFloats + slabs * 16 * lin::slab_ld(H)); }

// ========================================================================================== TD3 / DDPG =====
// td3_pendulum.py:171-228 and ddpg_pendulum.py:150-194 on the stages above.  SAC's step with a deterministic tanh actor,
// clipped Gaussian noise (offpolicy.hip noisy_action_kernel's two expressions) in place of the reparameterised sample, no
// temperature, one critic or two, and an actor phase that runs on the delayed steps only.  ONE workgroup carries a slab
// through a whole row phase: the chains that SAC deals to four workgroups ride along as items of the same stages (up to
// three H x H layers per stage on one compute unit), so nothing in these kernels waits for another workgroup — no flag, no
// counter — and a step that is not delayed can drop its actor phases by a return that is uniform over the grid.
constexpr int kTd3MaxBatch = 256;      // (ops.TD3_FUSED_MAX_BATCH) one grid of at most 16 slabs per row phase
struct Td3Images {                     // gymrl_td3_update_args.images, f32[9][H*H]; all null without images or H % 16 != 0
  const float *af, *cf[2], *tf[2], *atf, *ab, *cb[2];
  __host__ __device__ Td3Images(const float* base, int H) {
    const bool on = base && (H & 15) == 0;
    const size_t n = (size_t)H * H;
    auto at = [&](int k) { return on ? base + k * n : nullptr; };
    af = at(0); cf[0] = at(1); cf[1] = at(2); tf[0] = at(3); tf[1] = at(4); atf = at(5); ab = at(6); cb[0] = at(7); cb[1] = at(8);
  }
};
__device__ __forceinline__ int td3_delayed(const gymrl_td3_update_args& a) { return a.delayed_dev ? a.delayed_dev[0] : a.delayed; }

// ---- R1: draw + gather, actor_target(s'), smoothing noise, target critic(s), y, critic(s) on (s, a), loss gradient, dX chain ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_r1_kernel(const gymrl_td3_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld, C1a = X1 + 16 * ld, C1b = C1a + 16 * ld, C2a = C1b + 16 * ld, C2b = C2a + 16 * ld;
  const int T0 = C2b + 16 * ld, T1 = T0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const bool twin = a.n_critics == 2;
  const int Hn = twin ? H : 0, On = twin ? 1 : 0;      // the second network's items: no tiles when there is one critic
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Td3Images im(a.images, H);
  const gymrl_sac_critic_params &c = a.critic, &ct = a.critic_target;
  // ---- index draw + ring gather: one thread per row, rows beyond the batch are zero ----
  if (t < 16) {
    const int b = row0 + t;
    const bool ok = t < nrows;
    int64_t row = 0;
    if (ok) {
      if (a.idx) row = a.idx[b];
      else {
        uint64_t counter = a.idx_counter; uint32_t size = (uint32_t)a.idx_size;
        if (a.idx_dev) { const uint64_t* d = static_cast<const uint64_t*>(a.idx_dev); counter = d[0]; size = (uint32_t)(int64_t)d[1]; }
        int bits = 2;
        while (((int64_t)1 << bits) < (int64_t)size) ++bits;
        row = keyed_permute((uint32_t)b, size, bits / 2, bits - bits / 2, a.idx_seed ^ 0x5265706C61794944ull, counter);
      }
    }
    for (int k = 0; k < kMaxD; ++k) {
      const float sv = (ok && k < D) ? a.r_state[row * D + k] : 0.0f;
      lds[L.S + t * kMaxD + k] = sv;
      lds[L.S2 + t * kMaxD + k] = (ok && k < D) ? a.r_next[row * D + k] : 0.0f;
      if (ok && k < D) ws.s[(size_t)b * D + k] = sv;
    }
    for (int j = 0; j < kMaxA; ++j) {
      const float av = (ok && j < A) ? __uint_as_float(a.r_action[row * A + j]) : 0.0f;
      lds[L.A + t * kMaxA + j] = av;
      if (ok && j < A) ws.a[(size_t)b * A + j] = av;
    }
    lds[L.Misc + t * 4 + 0] = ok ? a.r_reward[row] : 0.0f;
    lds[L.Misc + t * 4 + 1] = ok ? (float)a.r_flag[row] : 0.0f;            // dones become float32
  }
  __syncthreads();
  // ---- actor_target(s') next to critic(s, a): three independent chains, layer by layer ----
  {
    const FwdItem st[3] = {fwd_item(L.S2, kD, -1, 0, D, D, H, a.actor_target.w[0], a.actor_target.b[0], X0, ld, nullptr, 0, R),
                           fwd_item(L.S, kD, L.A, kA, D + A, D, H, c.w[0], c.b[0], C1a, ld, ws.H1[0], H, R),
                           fwd_item(L.S, kD, L.A, kA, D + A, D, Hn, c.w[3], c.b[3], C1b, ld, ws.H1[1], H, R)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X0, ld, -1, 0, H, H, H, a.actor_target.w[1], a.actor_target.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.atf),
                           fwd_item(C1a, ld, -1, 0, H, H, H, c.w[1], c.b[1], C2a, ld, ws.H2[0], H, R, 0.0f, 0.0f, im.cf[0]),
                           fwd_item(C1b, ld, -1, 0, H, H, Hn, c.w[4], c.b[4], C2b, ld, ws.H2[1], H, R, 0.0f, 0.0f, im.cf[1])};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[3] = {fwd_item(X1, ld, -1, 0, H, H, A, a.actor_target.w[2], a.actor_target.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH),
                           fwd_item(C2a, ld, -1, 0, H, H, 1, c.w[2], c.b[2], L.Cq0, 4, nullptr, 0, NA),
                           fwd_item(C2b, ld, -1, 0, H, H, On, c.w[5], c.b[5], L.Cq1, 4, nullptr, 0, NA)};
    fwd_stage<3>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // a' (:191-196): offpolicy.hip noisy_action_kernel, mode 1
    const int b = row0 + t;
    const bool smooth = twin && a.policy_noise != 0.0;
    const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
    for (int j = 0; j < kMaxA; ++j) {
      float v = 0.0f;
      if (t < nrows && j < A) {
        const float mu = lds[L.Mean + t * kMaxA + j] * a.bound;
        v = mu;
        if (smooth) {
          const int i = b * A + j;
          const double e = a.eps ? a.eps[i] : (double)box_muller(a.noise_seed, ncounter, 2u, (uint32_t)i);
          float nz = (float)e * (float)a.policy_noise;
          nz = fminf(fmaxf(nz, -a.noise_clip), a.noise_clip);
          v = fminf(fmaxf(mu + nz, -a.bound), a.bound);
        }
      }
      lds[L.A2 + t * kMaxA + j] = v;
    }
  }
  __syncthreads();
  // ---- the target critic(s) on (s', a') (:197) ----
  {
    const FwdItem st[2] = {fwd_item(L.S2, kD, L.A2, kA, D + A, D, H, ct.w[0], ct.b[0], X0, ld, nullptr, 0, R),
                           fwd_item(L.S2, kD, L.A2, kA, D + A, D, Hn, ct.w[3], ct.b[3], T0, ld, nullptr, 0, R)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(X0, ld, -1, 0, H, H, H, ct.w[1], ct.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[0]),
                           fwd_item(T0, ld, -1, 0, H, H, Hn, ct.w[4], ct.b[4], T1, ld, nullptr, 0, R, 0.0f, 0.0f, im.tf[1])};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[2] = {fwd_item(X1, ld, -1, 0, H, H, 1, ct.w[2], ct.b[2], L.Q0, 4, nullptr, 0, NA),
                           fwd_item(T1, ld, -1, 0, H, H, On, ct.w[5], ct.b[5], L.Q1, 4, nullptr, 0, NA)};
    fwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {
    // y (:198-199; offpolicy.hip sac_target_kernel with log_alpha = 0 and a zero log-prob: alpha = 1, DDPG passes Q' twice), then
    // the loss gradient (:203-204; sac_critic_kernel / mse_kernel)
    const float alpha = (float)exp(0.0);
    const float q0 = lds[L.Q0 + t * 4], q1 = twin ? lds[L.Q1 + t * 4] : q0;
    const float tq = fminf(q0, q1) - alpha * 0.0f;
    const float y = lds[L.Misc + t * 4 + 0] + a.gamma * (1.0f - lds[L.Misc + t * 4 + 1]) * tq;
    const float invB = 1.0f / (float)a.B;
    for (int n = 0; n < a.n_critics; ++n) {
      const float e = lds[(n ? L.Cq1 : L.Cq0) + t * 4] - y;
      const float d = 2.0f * e * invB;
      for (int k = 0; k < 4; ++k) lds[(n ? L.Dq1 : L.Dq0) + t * 4 + k] = k == 0 ? d : 0.0f;
      if (t < nrows) {
        ws.dq[n][row0 + t] = d;
        if (n == 0) ws.terms[(size_t)(row0 + t) * 3 + 0] = (double)(e * e);
        else ws.terms2[row0 + t] = (double)(e * e);
      }
    }
  }
  __syncthreads();
  // ---- the critics' input-gradient chain (what backward() computes before the weight gradients) ----
  {
    const BwdItem st[2] = {BwdItem{L.Dq0, 4, 1, c.w[2], H, -1, nullptr, C2a, ld, R, X0, ld, ws.Z2[0], H, nullptr},
                           BwdItem{L.Dq1, 4, 1, c.w[5], Hn, -1, nullptr, C2b, ld, R, T0, ld, ws.Z2[1], H, nullptr}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[2] = {BwdItem{X0, ld, H, c.w[1], H, -1, nullptr, C1a, ld, R, -1, 0, ws.Z1[0], H, im.cb[0]},
                           BwdItem{T0, ld, H, c.w[4], Hn, -1, nullptr, C1b, ld, R, -1, 0, ws.Z1[1], H, im.cb[1]}};
    bwd_stage<2>(lds, st, row0, nrows);
  }
}

// ---- R3 (delayed steps): actor(s), Q1(s, actor(s)) of the updated critic, -mean's gradient back to the actor's first layer ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_r3_kernel(const gymrl_td3_update_args a, const SacWs ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (!td3_delayed(a)) return;            // one word, the same for every workgroup of the grid
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, AH1 = X0 + 16 * ld, AH2 = AH1 + 16 * ld, H1 = AH2 + 16 * ld, H2 = H1 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.B - row0);
  const int t = threadIdx.x;
  const int R = GYMRL_ACT_RELU, NA = GYMRL_ACT_NONE, kD = kMaxD, kA = kMaxA;
  const Td3Images im(a.images, H);
  const gymrl_sac_critic_params& c = a.critic;
  if (t < 16) {
    const int b = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? ws.s[(size_t)b * D + k] : 0.0f;
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, -1, 0, D, D, H, a.actor.w[0], a.actor.b[0], AH1, ld, ws.aH1, H, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(AH1, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], AH2, ld, ws.aH2, H, R, 0.0f, 0.0f, im.af)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(AH2, ld, -1, 0, H, H, A, a.actor.w[2], a.actor.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16)
    for (int j = 0; j < kMaxA; ++j) lds[L.A + t * kMaxA + j] = (t < nrows && j < A) ? lds[L.Mean + t * kMaxA + j] * a.bound : 0.0f;
  __syncthreads();
  // ---- critic.q1(s, actor(s)) (:213): the parameters T2 has just written ----
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, L.A, kA, D + A, D, H, c.w[0], c.b[0], H1, ld, nullptr, 0, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(H1, ld, -1, 0, H, H, H, c.w[1], c.b[1], H2, ld, nullptr, 0, R, 0.0f, 0.0f, im.cf[0])};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(H2, ld, -1, 0, H, H, 1, c.w[2], c.b[2], L.Q0, 4, nullptr, 0, NA)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  if (t < 16) {                           // offpolicy.hip neg_mean_kernel
    const float g = -1.0f / (float)a.B;
    for (int k = 0; k < 4; ++k) lds[L.Dq0 + t * 4 + k] = k == 0 ? g : 0.0f;
    if (t < nrows) ws.terms[(size_t)(row0 + t) * 3 + 1] = (double)lds[L.Q0 + t * 4];
  }
  __syncthreads();
  // ---- back through the frozen critic to the action ----
  {
    const BwdItem st[1] = {BwdItem{L.Dq0, 4, 1, c.w[2], H, -1, nullptr, H2, ld, R, X0, ld, nullptr, 0, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[1] = {BwdItem{X0, ld, H, c.w[1], H, -1, nullptr, H1, ld, R, H2, ld, nullptr, 0, im.cb[0]}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const int lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    if (wave == 0) {                      // d action = the action columns of dZ1 . W1
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = lin::tile_bwd_input(acc, lds + H2, ld, H, c.w[0], D + A, 0, lane);
      if (r >= D && r < D + A) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lds[L.A2 + (4 * q + g) * kMaxA + (r - D)] = acc[g];
      }
    }
  }
  __syncthreads();
  if (t < 16) {                           // through `* action_bound` and fc3's tanh (its dL/dz, from the saved output)
    for (int j = 0; j < 4; ++j) {
      float dz = 0.0f;
      if (j < A) {
        const float dy = lds[L.A2 + t * kMaxA + j] * a.bound;
        dz = dy * act_bwd(lds[L.Mean + t * kMaxA + j], GYMRL_ACT_TANH, 0.0f, 0.0f);
        if (t < nrows) ws.dmean[(size_t)(row0 + t) * A + j] = dz;
      }
      lds[L.Dq1 + t * 4 + j] = dz;
    }
  }
  __syncthreads();
  {
    const BwdItem st[1] = {BwdItem{L.Dq1, 4, A, a.actor.w[2], H, -1, nullptr, AH2, ld, R, X0, ld, ws.aZ2, H, nullptr}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const BwdItem st[1] = {BwdItem{X0, ld, H, a.actor.w[1], H, -1, nullptr, AH1, ld, R, -1, 0, ws.aZ1, H, im.ab}};
    bwd_stage<1>(lds, st, row0, nrows);
  }
}

// T2 (gate = 0: every step; the target twins move on delayed steps only) and T4 (gate = 1: delayed steps only)
__global__ __launch_bounds__(256) void td3_dw_kernel(const DwArgs a, const int32_t* delayed_dev, const int delayed_host, const int gate) {
  __shared__ double sm[3][4];
  const int delayed = delayed_dev ? delayed_dev[0] : delayed_host;
  if (gate && !delayed) return;
  sac_dw_body(a, blockIdx.x, gridDim.x, sm, delayed != 0);
}

// ---- acting: actor forward, exploration noise (noisy_action_kernel mode 0), Pendulum step, replay row ----
template <int HC>
__global__ __launch_bounds__(kThreads) void td3_act_kernel(const gymrl_td3_act_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L;
  const int D = a.D, A = a.A, H = HC ? HC : a.H, ld = lin::slab_ld(H);
  const int X0 = L.big, X1 = X0 + 16 * ld;
  const int bx = blockIdx.x, row0 = bx * 16, nrows = min(16, a.N - row0);
  const int t = threadIdx.x;
  if (t < 16) {
    const int i = row0 + t;
    for (int k = 0; k < kMaxD; ++k) lds[L.S + t * kMaxD + k] = (t < nrows && k < D) ? a.obs[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
  const int R = GYMRL_ACT_RELU, kD = kMaxD, kA = kMaxA;
  const float* af = (a.images && (H & 15) == 0) ? a.images : nullptr;
  {
    const FwdItem st[1] = {fwd_item(L.S, kD, -1, 0, D, D, H, a.actor.w[0], a.actor.b[0], X0, ld, nullptr, 0, R)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(X0, ld, -1, 0, H, H, H, a.actor.w[1], a.actor.b[1], X1, ld, nullptr, 0, R, 0.0f, 0.0f, af)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  {
    const FwdItem st[1] = {fwd_item(X1, ld, -1, 0, H, H, A, a.actor.w[2], a.actor.b[2], L.Mean, kA, nullptr, 0, GYMRL_ACT_TANH)};
    fwd_stage<1>(lds, st, row0, nrows);
  }
  __syncthreads();
  // one lane per env: noise, Pendulum step with auto-reset, replay row (the first wave: 16 lanes busy)
  if (t < 64) {
    const bool ok = t < nrows;
    ClassicStep<3> r;
    r.done = false; r.ret = 0.0; r.len = 0;
    if (ok) {
      const int i = row0 + t;
      const uint64_t ncounter = a.noise_counter_dev ? a.noise_counter_dev[0] : a.noise_counter;
      float act[kMaxA];
      for (int j = 0; j < A; ++j) {
        const int e_i = i * A + j;
        const float mu = lds[L.Mean + t * kMaxA + j] * a.bound;
        const double e = a.eps ? a.eps[e_i] : (double)box_muller(a.noise_seed, ncounter, 2u, (uint32_t)e_i);
        double v = (double)mu + e * a.noise_std;
        v = v < -(double)a.bound ? -(double)a.bound : (v > (double)a.bound ? (double)a.bound : v);
        act[j] = (float)v;
      }
      const PendulumState st(a.env_state, a.N);
      pendulum_step_one(st, i, a.env_seed, a.env_id0, act[0], r);
      const int64_t cursor = a.cursor_dev ? a.cursor_dev[0] : a.cursor;
      const int64_t row = (cursor + i) % a.cap;
      for (int k = 0; k < D; ++k) {
        a.r_state[row * D + k] = lds[L.S + t * kMaxD + k];
        a.r_next[row * D + k] = r.o_term[k];              // the TERMINAL observation is what the buffer keeps
        a.obs_out[(size_t)i * D + k] = r.o_next[k];
      }
      for (int j = 0; j < A; ++j) {
        a.r_action[row * A + j] = __float_as_uint(act[j]);
        if (a.action_out) a.action_out[(size_t)i * A + j] = act[j];
      }
      a.r_reward[row] = r.reward;
      a.r_flag[row] = r.done;                             // done = terminated or truncated
      if (a.rew_out) a.rew_out[i] = r.reward;
      if (a.done_out) a.done_out[i] = r.done;
      if (r.done && a.ep_ret_out) a.ep_ret_out[i] = (float)r.ret;
    }
    accumulate_ep_stats(a.ep_stats, r.done && ok, r.ret, r.len);
  }
}

// All nine images from the parameters as they are (after load_state_dict, soft_update(), a layer-by-layer update)
__global__ __launch_bounds__(256) void td3_pack_kernel(const gymrl_td3_update_args a) {
  const int H = a.H, steps = H >> 4;
  const size_t hh = (size_t)H * H;
  const float* src[9] = {a.actor.w[1], a.critic.w[1], a.critic.w[4], a.critic_target.w[1], a.critic_target.w[4], a.actor_target.w[1],
                         a.actor.w[1], a.critic.w[1], a.critic.w[4]};
  const int which = blockIdx.y;
  if (!src[which]) return;                 // DDPG: no second Q network
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < hh; o += (size_t)gridDim.x * 256) {
    const int n = (int)(o / H), k = (int)(o % H);
    a.images[which * hh + (which < 6 ? lin::img_fwd_index(n, k, steps) : lin::img_bwd_index(n, k, steps))] = src[which][o];
  }
}

inline bool td3_shape_ok(int B, int D, int A, int H) {
  return B > 0 && B <= kTd3MaxBatch && D > 0 && D <= kMaxD && A > 0 && A <= kMaxA && H >= 4 && H <= 256 && (H & 3) == 0;
}

}  // namespace

extern "C" {

size_t gymrl_sac_update_workspace_bytes(int B, int D, int A, int H) {
  if (B <= 0 || D <= 0 || A <= 0 || H <= 0) return 0;
  return SacWs::carve(nullptr, nullptr, B, D, A, H) + 256;
}

#ifdef GYMRL_PROF_BUILD
int gymrl_step_prof_read(long long* out_host) {      // probe build only: [4][32] stamps of the last launches (workgroup 0)
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_step_prof), sizeof(long long) * 128) == hipSuccess ? 0 : -1;
}
#endif

size_t gymrl_sac_args_bytes(int which) { return which == 0 ? sizeof(gymrl_sac_act_args) : which == 1 ? sizeof(gymrl_sac_update_args) : 0; }

static bool sac_act_args_ok(const gymrl_sac_act_args& a) {
  if (a.N <= 0 || !sac_shape_ok(1, a.D, a.A, a.H) || a.env_kind != GYMRL_ENV_PENDULUM || a.D != 3 || a.A != 1) return false;
  if (!a.env_state || !a.obs || !a.obs_out || !a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || a.cap < a.N) return false;
  for (int k = 0; k < 4; ++k) if (!a.actor.w[k] || !a.actor.b[k]) return false;
  return true;
}

int gymrl_sac_act_step(const gymrl_sac_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_act_args& a = *args;
  if (!sac_act_args_ok(a)) return -22;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)sac_act_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 4)) != hipSuccess ||
        hipFuncSetAttribute((const void*)sac_act_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 4)) != hipSuccess)
      return -1000 - (int)hipGetLastError();
    attr_set = true;
  }
  hipLaunchKernelGGL(a.H == 256 ? sac_act_kernel<256> : sac_act_kernel<0>, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 4), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

size_t gymrl_rainbow_update_workspace_bytes(int B, int D, int A, int H) {
  if (B <= 0 || D <= 0 || A <= 0 || H <= 0) return 0;
  return RbWs::carve(nullptr, nullptr, B, D, A, H) + 256;
}
size_t gymrl_rainbow_args_bytes(int which) { return which == 0 ? sizeof(gymrl_rainbow_act_args) : which == 1 ? sizeof(gymrl_rainbow_update_args) : 0; }

int gymrl_rainbow_act_step(const gymrl_rainbow_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_rainbow_act_args& a = *args;
  if (a.N <= 0 || !rb_shape_ok(1, a.D, a.A, a.H) || a.env_kind != GYMRL_ENV_CARTPOLE || a.D != 4 || a.A != 2) return -22;
  if (!a.env_state || !a.obs || !a.obs_out || !a.fc1_w || !a.fc1_b || !a.fc2_w || !a.fc2_b || !a.head_w || !a.head_b) return -22;
  if (!a.w_state || !a.w_action || !a.w_reward || !a.w_next || !a.w_terminal || !a.w_done || a.n_steps <= 0 || a.pushes < 0 ||
      !a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || a.cap < a.N || a.cursor < 0)
    return -22;
  if (a.fc2_img && (a.H & 15) != 0) return -22;
  auto act_lds = [](int H, int ns) { return sizeof(float) * (size_t)(16 * ns * (kMaxD + 4 + 2 * lin::slab_ld(H))); };
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)rainbow_act_kernel<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)act_lds(256, 1)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rainbow_act_kernel<2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)act_lds(256, 2)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rainbow_act_kernel<1, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)act_lds(256, 1)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rainbow_act_kernel<2, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)act_lds(256, 2)) != hipSuccess)
      return -1000 - (int)hipGetLastError();
    attr_set = true;
  }
  using ActK = void (*)(const gymrl_rainbow_act_args);
  const ActK k1 = rainbow_act_kernel<1, 0>, k2 = rainbow_act_kernel<2, 0>, k1w = rainbow_act_kernel<1, 256>, k2w = rainbow_act_kernel<2, 256>;
  const bool wide = a.H == 256;      // the instances built for the reference's hidden width
  // more envs than one round of 16-row workgroups over the 256 compute units: 32 rows per workgroup (weights streamed once)
  if (a.N > 16 * 256 && (a.D & 3) == 0 && (a.H & 3) == 0)
    hipLaunchKernelGGL(wide ? k2w : k2, dim3((a.N + 31) / 32), dim3(kThreads), act_lds(a.H, 2), (hipStream_t)stream_, a);
  else
    hipLaunchKernelGGL(wide ? k1w : k1, dim3((a.N + 15) / 16), dim3(kThreads), act_lds(a.H, 1), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_rainbow_update(const gymrl_rainbow_update_args* args, int phase, void* stream_) {
  if (!args || phase < 0 || phase > 2) return -22;
  const gymrl_rainbow_update_args& a = *args;
  if (!rb_shape_ok(a.B, a.D, a.A, a.H)) return -22;
  if (!a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || !a.idx || !a.p_fc1_w || !a.p_fc1_b || !a.p_fc2_w || !a.p_fc2_b ||
      !a.t_fc1_w || !a.t_fc1_b || !a.t_fc2_w || !a.t_fc2_b || !a.head_w || !a.head_b || !a.td_out || !a.loss_sum || !a.d_fc1_w || !a.d_fc1_b ||
      !a.d_fc2_w || !a.d_fc2_b || (!a.split_heads && (!a.d_head_w || !a.d_head_b)) || !a.workspace)
    return -22;
  if ((a.p_fc2_img_f || a.p_fc2_img_b || a.t_fc2_img_f) && (a.H & 15) != 0) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)rainbow_rows_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 7)) != hipSuccess ||
        hipFuncSetAttribute((const void*)rainbow_rows_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 7)) != hipSuccess)
      return -1000 - (int)hipGetLastError();
    attr_set = true;
  }
  RbWs ws;
  void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(a.workspace) + 255) & ~(uintptr_t)255);
  RbWs::carve(&ws, base, a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A1 = a.A + 1, H = a.H;
  if (phase != 2) hipLaunchKernelGGL(H == 256 ? rainbow_rows_kernel<256> : rainbow_rows_kernel<0>, slab_launch_grid((B + 15) / 16, 3), dim3(kThreads), lds_bytes(H, 7), stream, a, ws);
  if (phase == 1) { GYMRL_CHECK_LAUNCH(); return 0; }
  DwArgs d{};
  int w0 = 0, ns = 0, t0 = 0;
  auto seg = [&](const float* dZ, int ldz, int N, const float* X, int ldx, int K, float* gW, float* gb) {
    DwSeg& s = d.seg[ns++];
    s.dZ = dZ; s.X = X; s.X2 = nullptr; s.W = gW; s.b = gb; s.Wt = nullptr; s.bt = nullptr;
    s.img_f = nullptr; s.img_b = nullptr; s.img_tf = nullptr;
    s.ldz = ldz; s.ldx = ldx; s.ldx2 = 0; s.N = N; s.K = K; s.K1 = K; s.wave0 = w0;
    const int tl = ((N + 15) / 16) * ((K + 15) / 16);
    s.slices = lin::bwd_weight_slices(B, N, K); s.tile0 = t0;
    w0 += tl * s.slices; t0 += tl;
  };
  seg(ws.dS, A1, A1, ws.h2, H, H, a.d_head_w, a.d_head_b);       // the stacked noisy heads (gymrl_noisy_split takes it from here)
  seg(ws.dZ2, H, H, ws.h1, H, H, a.d_fc2_w, a.d_fc2_b);
  seg(ws.dZ1, H, H, ws.s, D, D, a.d_fc1_w, a.d_fc1_b);
  d.nseg = ns; d.total_waves = w0; d.total_tiles = t0; d.B = B; d.store_grads = 1; d.parts = ws.dw_parts; d.phase = B > 512 ? 1 : 0;
  d.split_heads = a.split_heads ? 1 : 0; d.split_A = a.A;
  for (int l = 0; l < 2; ++l) {
    d.dw_mu[l] = a.dw_mu[l]; d.dw_sigma[l] = a.dw_sigma[l]; d.db_mu[l] = a.db_mu[l]; d.db_sigma[l] = a.db_sigma[l];
    d.w_eps[l] = a.w_eps[l]; d.b_eps[l] = a.b_eps[l];
    if (a.split_heads && (!a.dw_mu[l] || !a.dw_sigma[l] || !a.db_mu[l] || !a.db_sigma[l] || !a.w_eps[l] || !a.b_eps[l])) return -22;
  }
  d.terms = ws.terms; d.term0 = 0; d.nterms = 1; d.sums = a.loss_sum; d.alpha_step = 0;
  launch_dw(d, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_sac_pack_images(const gymrl_sac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_update_args& a = *args;
  if (!a.images || a.H <= 0 || (a.H & 15) != 0 || a.H > 256) return -22;
  if (!a.actor.w[1] || !a.critic.w[1] || !a.critic.w[4] || !a.target.w[1] || !a.target.w[4]) return -22;
  hipLaunchKernelGGL(sac_pack_kernel, dim3((a.H * a.H + 255) / 256, 8), dim3(256), 0, (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static bool sac_update_args_ok(const gymrl_sac_update_args& a) {
  if (!sac_shape_ok(a.B, a.D, a.A, a.H)) return false;
  if (!a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || !a.workspace || !a.sums || !a.log_alpha || !a.alpha_m || !a.alpha_v ||
      !a.actor_p || !a.actor_m || !a.actor_v || !a.critic_p || !a.critic_m || !a.critic_v || (!a.idx && a.idx_size < a.B))
    return false;
  for (int k = 0; k < 4; ++k) if (!a.actor.w[k] || !a.actor.b[k]) return false;
  for (int k = 0; k < 6; ++k) if (!a.critic.w[k] || !a.critic.b[k] || !a.target.w[k] || !a.target.b[k]) return false;
  return true;
}

static int sac_set_lds_attr() {
  static bool attr_set = false;
  if (!attr_set) {
    const void* fns[6] = {(const void*)sac_p1_kernel<0>, (const void*)sac_p1_kernel<256>, (const void*)sac_p3_kernel<0>, (const void*)sac_p3_kernel<256>,
                          (const void*)sac_step_kernel<0>, (const void*)sac_step_kernel<256>};
    for (const void* f : fns)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 8)) != hipSuccess) return -1000 - (int)hipGetLastError();
    attr_set = true;
  }
  return 0;
}

// The tile lists of P2 (critic: c) and P4 (actor + temperature: p)
static void sac_build_dw(const gymrl_sac_update_args& a, const SacWs& ws, DwArgs& c, DwArgs& p) {
  const int B = a.B, D = a.D, A = a.A, H = a.H;
  auto tiles = [](int N, int K) { return ((N + 15) / 16) * ((K + 15) / 16); };
  int w0 = 0, ns = 0, t0 = 0;
  const bool use_img = a.images && (a.H & 15) == 0;
  const size_t hh = (size_t)a.H * a.H;
  auto img = [&](int k) { return use_img ? a.images + k * hh : nullptr; };
  auto seg = [&](DwArgs& d, const float* dZ, int ldz, int N, const float* X, int ldx, const float* X2, int ldx2, int K, int K1, float* W, float* b,
                 float* Wt, float* bt, float* img_f = nullptr, float* img_b = nullptr, float* img_tf = nullptr) {
    DwSeg& s = d.seg[ns++];
    s.dZ = dZ; s.X = X; s.X2 = X2; s.W = W; s.b = b; s.Wt = Wt; s.bt = bt;
    s.img_f = img_f; s.img_b = img_b; s.img_tf = img_tf;
    s.ldz = ldz; s.ldx = ldx; s.ldx2 = ldx2; s.N = N; s.K = K; s.K1 = K1; s.wave0 = w0;
    s.slices = lin::bwd_weight_slices(B, N, K); s.tile0 = t0;
    w0 += tiles(N, K) * s.slices; t0 += tiles(N, K);
  };
  // critic: launch order of the layer-by-layer backward is irrelevant here (tiles are independent); fc1/fc4, fc2/fc5, fc3/fc6
  c = DwArgs{};
  for (int i = 0; i < 2; ++i) {
    seg(c, ws.Z1[i], H, H, ws.s, D, ws.a, A, D + A, D, a.critic.w[3 * i], a.critic.b[3 * i], a.target.w[3 * i], a.target.b[3 * i]);
    seg(c, ws.Z2[i], H, H, ws.H1[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 1], a.critic.b[3 * i + 1], a.target.w[3 * i + 1], a.target.b[3 * i + 1],
        img(1 + i), img(6 + i), img(3 + i));
    seg(c, ws.dq[i], 1, 1, ws.H2[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 2], a.critic.b[3 * i + 2], a.target.w[3 * i + 2], a.target.b[3 * i + 2]);
  }
  c.nseg = ns; c.total_waves = w0; c.total_tiles = t0; c.B = B; c.parts = ws.dw_parts; c.phase = B > 512 ? 1 : 0;
  c.p = a.critic_p; c.m = a.critic_m; c.v = a.critic_v;
  for (int k = 0; k < 4; ++k) c.adam[k] = a.adam_critic[k];
  c.adam_dev = a.adam_critic_dev;
  c.omb1 = (float)(1.0 - a.beta1); c.beta2 = (float)a.beta2; c.omb2 = (float)(1.0 - a.beta2); c.eps = (float)a.eps_adam;
  c.tau = (float)a.tau; c.omt = (float)(1.0 - a.tau);
  c.terms = ws.terms; c.terms_b = ws.terms2; c.term0 = 0; c.nterms = 1; c.sums = a.sums; c.alpha_step = 0;

  p = DwArgs{};
  w0 = 0; ns = 0; t0 = 0;
  seg(p, ws.aZ1, H, H, ws.s, D, nullptr, 0, D, D, a.actor.w[0], a.actor.b[0], nullptr, nullptr);
  seg(p, ws.aZ2, H, H, ws.aH1, H, nullptr, 0, H, H, a.actor.w[1], a.actor.b[1], nullptr, nullptr, img(0), img(5), nullptr);
  seg(p, ws.dmean, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[2], a.actor.b[2], nullptr, nullptr);
  seg(p, ws.dls, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[3], a.actor.b[3], nullptr, nullptr);
  p.nseg = ns; p.total_waves = w0; p.total_tiles = t0; p.B = B; p.parts = ws.dw_parts; p.phase = B > 512 ? 1 : 0;
  p.p = a.actor_p; p.m = a.actor_m; p.v = a.actor_v;
  for (int k = 0; k < 4; ++k) p.adam[k] = a.adam_actor[k];
  p.adam_dev = a.adam_actor_dev;
  p.omb1 = c.omb1; p.beta2 = c.beta2; p.omb2 = c.omb2; p.eps = c.eps;
  p.tau = 0.0f; p.omt = 0.0f;
  p.terms = ws.terms; p.term0 = 1; p.nterms = 2; p.sums = a.sums; p.alpha_step = 1;
  p.log_alpha = a.log_alpha; p.alpha_m = a.alpha_m; p.alpha_v = a.alpha_v; p.lr_alpha = a.lr_alpha;
  p.abeta1 = 0.9; p.abeta2 = 0.999; p.aeps = 1e-8;
  p.alpha_bias[0] = a.alpha_bias[0]; p.alpha_bias[1] = a.alpha_bias[1]; p.alpha_bias_dev = a.alpha_bias_dev; p.alpha_loss = a.alpha_loss;
}

int gymrl_sac_update(const gymrl_sac_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_sac_update_args& a = *args;
  if (!sac_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = sac_set_lds_attr()) return rc;
  SacWs ws;
  void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(a.workspace) + 255) & ~(uintptr_t)255);
  SacWs::carve(&ws, base, a.B, a.D, a.A, a.H);
  const int H = a.H, slabs = (a.B + 15) / 16;
  DwArgs c, p;
  sac_build_dw(a, ws, c, p);
  // (the instances built for the reference's hidden width 256 know every reduction length at compile time)
  hipLaunchKernelGGL(H == 256 ? sac_p1_kernel<256> : sac_p1_kernel<0>, slab_launch_grid(slabs, 4), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);   // y / role: the two target chains, the two critic chains
  launch_dw(c, stream);
  hipLaunchKernelGGL(H == 256 ? sac_p3_kernel<256> : sac_p3_kernel<0>, slab_launch_grid(slabs, 2), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);   // y / role: the actor + Q2, then Q1
  launch_dw(p, stream);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_sac_step(const gymrl_sac_act_args* act_args, const gymrl_sac_update_args* upd_args, void* stream_) {
  if (!act_args || !upd_args) return -22;
  const gymrl_sac_act_args& a = *act_args;
  const gymrl_sac_update_args& u = *upd_args;
  if (!sac_act_args_ok(a) || !sac_update_args_ok(u) || a.H != u.H || u.B > 256) return -22;   // one grid: every waiting block must be resident
  if (const int rc = sac_set_lds_attr()) return rc;
  SacStepArgs s;
  s.act = a; s.upd = u;
  void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(u.workspace) + 255) & ~(uintptr_t)255);
  SacWs::carve(&s.ws, base, u.B, u.D, u.A, u.H);
  sac_build_dw(u, s.ws, s.c, s.p);
  s.n_act = (a.N + 15) / 16; s.slabs = (u.B + 15) / 16;
  s.c_blocks = (s.c.total_waves + kWaves - 1) / kWaves + 1; s.p_blocks = (s.p.total_waves + kWaves - 1) / kWaves + 1;
  const int blocks = s.n_act + 6 * s.slabs + s.c_blocks + s.p_blocks;
  hipLaunchKernelGGL(u.H == 256 ? sac_step_kernel<256> : sac_step_kernel<0>, dim3(blocks), dim3(kThreads), lds_bytes(u.H, 8), (hipStream_t)stream_, s);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------- TD3 / DDPG ----
size_t gymrl_td3_update_workspace_bytes(int B, int D, int A, int H) {      // SAC's hand-off layout: the same slabs per network
  if (B <= 0 || D <= 0 || A <= 0 || H <= 0) return 0;
  return SacWs::carve(nullptr, nullptr, B, D, A, H) + 256;
}
size_t gymrl_td3_args_bytes(int which) { return which == 0 ? sizeof(gymrl_td3_act_args) : which == 1 ? sizeof(gymrl_td3_update_args) : 0; }

static int td3_set_lds_attr() {
  static bool attr_set = false;
  if (!attr_set) {
    const void* fns[6] = {(const void*)td3_r1_kernel<0>, (const void*)td3_r1_kernel<256>, (const void*)td3_r3_kernel<0>, (const void*)td3_r3_kernel<256>,
                          (const void*)td3_act_kernel<0>, (const void*)td3_act_kernel<256>};
    for (const void* f : fns)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 8)) != hipSuccess) return -1000 - (int)hipGetLastError();
    attr_set = true;
  }
  return 0;
}

int gymrl_td3_act_step(const gymrl_td3_act_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_act_args& a = *args;
  if (a.N <= 0 || !td3_shape_ok(1, a.D, a.A, a.H) || a.env_kind != GYMRL_ENV_PENDULUM || a.D != 3 || a.A != 1) return -22;
  if (!a.env_state || !a.obs || !a.obs_out || !a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || a.cap < a.N || a.cursor < 0) return -22;
  for (int k = 0; k < 3; ++k) if (!a.actor.w[k] || !a.actor.b[k]) return -22;
  if (const int rc = td3_set_lds_attr()) return rc;
  hipLaunchKernelGGL(a.H == 256 ? td3_act_kernel<256> : td3_act_kernel<0>, dim3((a.N + 15) / 16), dim3(kThreads), lds_bytes(a.H, 2), (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

static bool td3_update_args_ok(const gymrl_td3_update_args& a) {
  if (!td3_shape_ok(a.B, a.D, a.A, a.H) || (a.n_critics != 1 && a.n_critics != 2)) return false;
  if (!a.r_state || !a.r_action || !a.r_reward || !a.r_next || !a.r_flag || !a.workspace || !a.sums || !a.actor_p || !a.actor_m || !a.actor_v ||
      !a.critic_p || !a.critic_m || !a.critic_v || (!a.idx && !a.idx_dev && a.idx_size < a.B))
    return false;
  for (int k = 0; k < 3; ++k) if (!a.actor.w[k] || !a.actor.b[k] || !a.actor_target.w[k] || !a.actor_target.b[k]) return false;
  for (int k = 0; k < 3 * a.n_critics; ++k) if (!a.critic.w[k] || !a.critic.b[k] || !a.critic_target.w[k] || !a.critic_target.b[k]) return false;
  return true;
}

int gymrl_td3_pack_images(const gymrl_td3_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_update_args& a = *args;
  if (!a.images || a.H <= 0 || (a.H & 15) != 0 || a.H > 256 || (a.n_critics != 1 && a.n_critics != 2)) return -22;
  if (!a.actor.w[1] || !a.actor_target.w[1] || !a.critic.w[1] || !a.critic_target.w[1] || (a.n_critics == 2 && (!a.critic.w[4] || !a.critic_target.w[4]))) return -22;
  hipLaunchKernelGGL(td3_pack_kernel, dim3((a.H * a.H + 255) / 256, 9), dim3(256), 0, (hipStream_t)stream_, a);
  GYMRL_CHECK_LAUNCH();
  return 0;
}

int gymrl_td3_update(const gymrl_td3_update_args* args, void* stream_) {
  if (!args) return -22;
  const gymrl_td3_update_args& a = *args;
  if (!td3_update_args_ok(a)) return -22;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = td3_set_lds_attr()) return rc;
  SacWs ws;
  void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(a.workspace) + 255) & ~(uintptr_t)255);
  SacWs::carve(&ws, base, a.B, a.D, a.A, a.H);
  const int B = a.B, D = a.D, A = a.A, H = a.H, slabs = (B + 15) / 16;
  // the tile lists of T2 (critic: c) and T4 (actor: p), as sac_build_dw's
  auto tiles = [](int N, int K) { return ((N + 15) / 16) * ((K + 15) / 16); };
  const bool use_img = a.images && (H & 15) == 0;
  const size_t hh = (size_t)H * H;
  auto img = [&](int k) { return use_img ? a.images + k * hh : nullptr; };
  int w0 = 0, ns = 0;
  auto seg = [&](DwArgs& d, const float* dZ, int ldz, int N, const float* X, int ldx, const float* X2, int ldx2, int K, int K1, float* W, float* b,
                 float* Wt, float* bt, float* img_f = nullptr, float* img_b = nullptr, float* img_tf = nullptr) {
    DwSeg& s = d.seg[ns++];
    s.dZ = dZ; s.X = X; s.X2 = X2; s.W = W; s.b = b; s.Wt = Wt; s.bt = bt;
    s.img_f = img_f; s.img_b = img_b; s.img_tf = img_tf;
    s.ldz = ldz; s.ldx = ldx; s.ldx2 = ldx2; s.N = N; s.K = K; s.K1 = K1; s.wave0 = w0;
    s.slices = 1; s.tile0 = w0;
    w0 += tiles(N, K);
  };
  auto finish = [&](DwArgs& d, float* p, float* m, float* v, const float (&adam)[4], const float* adam_dev, int term0, const double* terms_b) {
    d.nseg = ns; d.total_waves = w0; d.total_tiles = w0; d.B = B; d.parts = nullptr; d.phase = 0;
    d.p = p; d.m = m; d.v = v;
    for (int k = 0; k < 4; ++k) d.adam[k] = adam[k];
    d.adam_dev = adam_dev;
    d.omb1 = (float)(1.0 - a.beta1); d.beta2 = (float)a.beta2; d.omb2 = (float)(1.0 - a.beta2); d.eps = (float)a.eps_adam;
    d.tau = (float)a.tau; d.omt = (float)(1.0 - a.tau);
    d.terms = ws.terms; d.terms_b = terms_b; d.term0 = term0; d.nterms = 1; d.sums = a.sums; d.alpha_step = 0;
  };
  DwArgs c{}, p{};
  for (int i = 0; i < a.n_critics; ++i) {
    seg(c, ws.Z1[i], H, H, ws.s, D, ws.a, A, D + A, D, a.critic.w[3 * i], a.critic.b[3 * i], a.critic_target.w[3 * i], a.critic_target.b[3 * i]);
    seg(c, ws.Z2[i], H, H, ws.H1[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 1], a.critic.b[3 * i + 1], a.critic_target.w[3 * i + 1], a.critic_target.b[3 * i + 1],
        img(1 + i), img(7 + i), img(3 + i));
    seg(c, ws.dq[i], 1, 1, ws.H2[i], H, nullptr, 0, H, H, a.critic.w[3 * i + 2], a.critic.b[3 * i + 2], a.critic_target.w[3 * i + 2], a.critic_target.b[3 * i + 2]);
  }
  finish(c, a.critic_p, a.critic_m, a.critic_v, a.adam_critic, a.adam_critic_dev, 0, a.n_critics == 2 ? ws.terms2 : nullptr);
  w0 = 0; ns = 0;
  seg(p, ws.aZ1, H, H, ws.s, D, nullptr, 0, D, D, a.actor.w[0], a.actor.b[0], a.actor_target.w[0], a.actor_target.b[0]);
  seg(p, ws.aZ2, H, H, ws.aH1, H, nullptr, 0, H, H, a.actor.w[1], a.actor.b[1], a.actor_target.w[1], a.actor_target.b[1], img(0), img(6), img(5));
  seg(p, ws.dmean, A, A, ws.aH2, H, nullptr, 0, H, H, a.actor.w[2], a.actor.b[2], a.actor_target.w[2], a.actor_target.b[2]);
  finish(p, a.actor_p, a.actor_m, a.actor_v, a.adam_actor, a.adam_actor_dev, 1, nullptr);
  const bool wide = H == 256;            // the instances built for the reference's hidden width
  hipLaunchKernelGGL(wide ? td3_r1_kernel<256> : td3_r1_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 8), stream, a, ws);
  hipLaunchKernelGGL(td3_dw_kernel, dim3((c.total_waves + 3) / 4 + 1), dim3(256), 0, stream, c, a.delayed_dev, a.delayed, 0);
  if (a.delayed_dev || a.delayed) {      // (a host-side zero: the actor phases are not even launched)
    hipLaunchKernelGGL(wide ? td3_r3_kernel<256> : td3_r3_kernel<0>, dim3(slabs), dim3(kThreads), lds_bytes(H, 5), stream, a, ws);
    hipLaunchKernelGGL(td3_dw_kernel, dim3((p.total_waves + 3) / 4 + 1), dim3(256), 0, stream, p, a.delayed_dev, a.delayed, 1);
  }
  GYMRL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// slab_step_device.hpp — what the row-slab step kernels of every off-policy algorithm share.
//
// offpolicy_step.hip (SAC), rainbow_step.hip (Rainbow), td3_step.hip (TD3 / DDPG), dsac_step.hip (discrete SAC) and dqn_step.hip (DQN) carry a 16-row slab of the batch through
// a chain of layers in ONE workgroup of 16 waves (offpolicy_step.hip's header has the argument).  Here: the stages (fwd_stage /
// bwd_stage over FwdItem / BwdItem), the LDS layout (Lds), the narrow layers' staging (Stager), the hand-off flags,
// the grid shapes and their deadlock argument (slab_grid), SAC's and TD3's hand-off workspace (SacWs), the
// weight-gradient tile kernel (DwArgs / sac_dw_body / sac_dw_kernel) with its host-side list builder (DwBuilder), and the
// blocks that the algorithms had each carried a copy of: the replay index draw, the Pendulum / CartPole
// acting tails, the weight-image slots and their packing, the entry points' argument checks and the small host helpers.  Everything is __forceinline__ device code or inline host code inside an anonymous
// namespace: every translation unit that includes this header has its own file-local kernels and the library exports none of it.
#pragma once
#include <initializer_list>
#include "env_classic_device.hpp"
#include "lin_device.hpp"

namespace gymrl {
namespace slab {
namespace {

using lin::act_bwd;
using lin::act_fwd;

constexpr int kWaves = 16, kThreads = 64 * kWaves;
constexpr int kMaxBatch = 8192;      // (ops.FUSED_MAX_BATCH) rows of an update: 512 slabs
constexpr int kDwMaxSlices = 32;     // lin_device.hpp bwd_weight_slices(B <= 8192, ...) <= cdiv(B, 256)
constexpr int kMaxD = 8, kMaxA = 4;

// 256-byte aligned float arrays handed out one after another from `base` (nullptr: only the sizes are added up)
struct carve_taker {
  void* base; size_t off = 0;
  __host__ __device__ float* operator()(size_t n) {
    float* p = base ? reinterpret_cast<float*>(static_cast<char*>(base) + off) : nullptr;
    off += ((n * 4 + 255) & ~(size_t)255);
    return p;
  }
};
inline void* align256(void* p) { return reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }
// a gymrl_*_update_workspace_bytes: the carved size + the slack align256 may use up
template <class Ws>
inline size_t workspace_bytes(int B, int D, int A, int H) {
  if (B <= 0 || D <= 0 || A <= 0 || H <= 0) return 0;
  return Ws::carve(nullptr, nullptr, B, D, A, H) + 256;
}

// ---- what an entry point refuses with -22 before anything touches HIP: where the algorithms' checks differ, the call site says so ----
inline bool slab_shape_ok(int B, int max_batch, int D, int A, int H) {
  return B > 0 && B <= max_batch && D > 0 && D <= kMaxD && A > 0 && A <= kMaxA && H >= 4 && H <= 256 && (H & 3) == 0;
}
inline bool all_set(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if (!p) return false;
  return true;
}
// the first `layers` layers of a gymrl_*_params struct (all of them by default; DDPG's single critic fills three of six)
template <class Net>
inline bool net_ok(const Net& n, int layers = (int)(sizeof(Net::w) / sizeof(void*))) {
  for (int k = 0; k < layers; ++k) if (!n.w[k] || !n.b[k]) return false;
  return true;
}
template <class Args>
inline bool ring_ok(const Args& a) { return all_set({a.r_state, a.r_action, a.r_reward, a.r_next, a.r_flag}); }
// the fixed (D, A) of the env kinds an act kernel steps (ClassicDims of env_classic_device.hpp); {0, 0}, which no argument block
// passes, for every other kind
struct ActDims { int D, A; };
template <int KIND>
constexpr ActDims act_dims_of() { return ActDims{ClassicDims<KIND>::kObs, ClassicDims<KIND>::kActions}; }
inline ActDims act_env_dims(int env_kind) {
  switch (env_kind) {
    case GYMRL_ENV_CARTPOLE: return act_dims_of<GYMRL_ENV_CARTPOLE>();
    case GYMRL_ENV_PENDULUM: return act_dims_of<GYMRL_ENV_PENDULUM>();
    case GYMRL_ENV_MOUNTAINCAR: return act_dims_of<GYMRL_ENV_MOUNTAINCAR>();
    case GYMRL_ENV_ACROBOT: return act_dims_of<GYMRL_ENV_ACROBOT>();
    default: return ActDims{0, 0};
  }
}
// an act step's env, I/O and ring: the env kind the entry point steps, with that kind's D and A; refuse_neg_cursor: SAC's act step
// has never looked at the cursor
template <class Args>
inline bool act_args_ok(const Args& a, int env_kind, bool refuse_neg_cursor) {
  const ActDims dims = act_env_dims(env_kind);
  return a.N > 0 && slab_shape_ok(1, 1, a.D, a.A, a.H) && a.env_kind == env_kind && a.D == dims.D && a.A == dims.A &&
         all_set({a.env_state, a.obs, a.obs_out}) && ring_ok(a) && a.cap >= a.N && !(refuse_neg_cursor && a.cursor < 0);
}
// the kinds gymrl_dqn_act_step_classic / gymrl_dsac_act_step_classic have an instance for (ops.FUSED_ACT_KINDS)
inline bool classic_act_kind_ok(int env_kind) {
  return env_kind == GYMRL_ENV_CARTPOLE || env_kind == GYMRL_ENV_MOUNTAINCAR || env_kind == GYMRL_ENV_ACROBOT;
}
// an update's replay rows: the caller's list, (where idx_dev_counts) the device's draw record, or a keyed draw over idx_size >= B rows
template <class Args>
inline bool draw_ok(const Args& a, bool idx_dev_counts) { return a.idx || (idx_dev_counts && a.idx_dev) || a.idx_size >= a.B; }
// a pack call's images buffer and width
template <class Args>
inline bool pack_args_ok(const Args& a) { return a.images && a.H > 0 && (a.H & 15) == 0 && a.H <= 256; }
// the k-th H x H weight image of an update's or an act step's `images`; all null without a buffer or when H % 16 != 0
struct ImageSlots {
  const float* base; bool on; size_t n;
  __host__ __device__ ImageSlots(const float* images, int H) : base(images), on(images && (H & 15) == 0), n((size_t)H * H) {}
  __host__ __device__ const float* operator()(int k) const { return on ? base + k * n : nullptr; }
};

// ---- hand-off between the row phases and the tile phases (caller-owned workspace) -------------------------------------
struct SacWs {
  float *s, *a;                       // [B][D], [B][A]: the gathered batch
  float *H1[2], *Z1[2], *H2[2], *Z2[2], *dq[2];      // critic net i: activations and dL/dz per layer
  float *aH1, *aZ1, *aH2, *aZ2, *dmean, *dls;        // actor
  double* terms;                      // [B][3]: per-row critic term, actor term, temperature term
  double* terms2;                     // [B]: the second Q network's critic term (its workgroup's share of terms[.][0])
  float *xtq[2], *xmisc;              // P1: the two target networks' Q(s', a') columns [16 S] and {reward, done, logp'} [16 S][4], from the
                                      // target-chain workgroups to the critic-chain workgroups (each forms y itself)
  unsigned int* sync;                 // [16]: the large-batch row kernels' tickets (slab_grid: 0 / 1 P1's, 2 / 3 P3's), zero between launches;
                                      // the other twelve words are unused and keep the workspace's layout
  unsigned int* flag;                 // [8][ceil(B / 16)]: hand-off flags (1 = waiting to be consumed; zero before the first launch, left zero):
                                      //   P1: 0 / 1 target network 1 -> critic workgroup 1 / 2, 5 / 6 target network 2 -> critic workgroup 1 / 2;
                                      //   P3: 2 / 3 Q1 / Q2, 4 the second network's dZ1 slab
  float *xa, *xq[2], *xpart;          // P3's exchanges: action [16 S][kMaxA], the two Q columns [16 S], network 1's half of the d action chain [16 S][kMaxA]
  float* dw_parts;                    // B > 512: the weight-gradient tiles' slice partials (DwArgs)
  float *xmean, *xls, *xeps, *xlp;    // the actor step's sample (mean, log_std, eps [16 S][kMaxA], logp [16 S]): P1's critic-chain workgroup
                                      // computes it while it waits for y, P3 starts from it
  __host__ __device__ static size_t carve(SacWs* w, void* base, int B, int D, int A, int H) {
    carve_taker take{base};
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
    return take.off;
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

// a stage of ONE item and the workgroup barrier behind it: fwd_one(lds, {fwd_item(...)}, row0, nrows).  (The item arrives as the
// one-element list the stage itself takes: copied out of a `const FwdItem&` the same kernels came out 2-4 VGPRs apart.)
__device__ __forceinline__ void fwd_one(float* lds, const FwdItem (&item)[1], int row0, int nrows) {
  fwd_stage<1>(lds, item, row0, nrows);
  __syncthreads();
}
__device__ __forceinline__ void bwd_one(float* lds, const BwdItem (&item)[1], int row0, int nrows) {
  bwd_stage<1>(lds, item, row0, nrows);
  __syncthreads();
}

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
inline size_t lds_bytes(int H, int slabs) { return sizeof(float) * (size_t)(kSmallFloats + slabs * 16 * lin::slab_ld(H)); }

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

// hand-off between the paired workgroups of a slab: the producer's data stores, a workgroup barrier, then ONE release store of
// the flag; the consumer's thread 0 spins on it (agent scope), a workgroup barrier, the data is read with agent-scope loads,
// and the consumer — the flag's only reader — clears it for the next launch
__device__ __forceinline__ void flag_post(unsigned int* f) { __hip_atomic_store(f, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
// (polling with relaxed loads and ONE acquire fence at the end: an acquire per poll invalidates the compute unit's L1 and the
// XCD's L2 lines each time round, under the workgroups that are streaming weights through them)
// Every spin of these kernels is BOUNDED: kSpinLimit polls (each a sleep + an L2 round trip, ~0.3-1 us: seconds in all, against
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

// ================================================================================================= weight-gradient tiles =====
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
  float clamp_abs;                                // > 0: every gradient element is clamped to +-clamp_abs before Adam's moments (optim.hip adam_one; DQN's +-1); 0: off
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
  // alpha_step == 2: discrete SAC's float32 temperature (offpolicy.hip dsac_alpha_kernel) — its scalar and moments, the target
  // entropy and the step count the bias corrections are formed from when alpha_bias_dev is null; lr_alpha / abeta1 / abeta2 /
  // aeps hold that kernel's float32 arguments
  float* log_alpha_f; float* alpha_m_f; float* alpha_v_f; float target_entropy_f; int64_t alpha_t;
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
    if (a.alpha_step == 2) {              // offpolicy.hip dsac_alpha_kernel on fin[1] = the entropy sum (float32 arithmetic)
      if (threadIdx.x == 0) {
        const float lr = (float)a.lr_alpha, b1 = (float)a.abeta1, b2 = (float)a.abeta2, eps = (float)a.aeps;
        const float alpha = det_expf(a.log_alpha_f[0]);
        const float mean_gap = (float)((0.0 + fin[1]) / (double)a.B) - a.target_entropy_f;
        if (a.alpha_loss) a.alpha_loss[0] = (double)(alpha * mean_gap);
        const float g = alpha * mean_gap;
        const float mm = b1 * a.alpha_m_f[0] + (1.0f - b1) * g;
        const float vv = b2 * a.alpha_v_f[0] + (1.0f - b2) * g * g;
        a.alpha_m_f[0] = mm; a.alpha_v_f[0] = vv;
        const double bc1 = a.alpha_bias_dev ? a.alpha_bias_dev[0] : 1.0 - pow((double)b1, (double)a.alpha_t);
        const double bc2 = a.alpha_bias_dev ? a.alpha_bias_dev[1] : 1.0 - pow((double)b2, (double)a.alpha_t);
        const float step_size = (float)((double)lr / bc1);
        const float denom = (float)(sqrt((double)vv) / sqrt(bc2)) + eps;
        a.log_alpha_f[0] = a.log_alpha_f[0] - step_size * (mm / denom);
      }
      return;
    }
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
      lin::adam_elem(P, acc[g], M, V, ad, a.clamp_abs);
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
    lin::adam_elem(P, colsum, M, V, ad, a.clamp_abs);
    s.b[n] = P; a.m[po] = M; a.v[po] = V;
    if (s.bt && polyak) s.bt[n] = a.tau * P + a.omt * s.bt[n];
  }
}

__global__ __launch_bounds__(256) void sac_dw_kernel(const DwArgs a) {
  __shared__ double sm[3][4];
  sac_dw_body(a, blockIdx.x, gridDim.x, sm);
}
// one launch up to 512 rows; beyond: the slice partials, then their ordered sums + the tiles' epilogues + the loss sums
inline void launch_dw(DwArgs d, hipStream_t stream) {
  hipLaunchKernelGGL(sac_dw_kernel, dim3((d.total_waves + 3) / 4 + 1), dim3(256), 0, stream, d);
  if (d.phase == 1) {
    d.phase = 2;
    hipLaunchKernelGGL(sac_dw_kernel, dim3((d.total_tiles + 3) / 4 + 1), dim3(256), 0, stream, d);
  }
}

// The replay row of batch element b: the caller's index list or, without one, the keyed permutation of [0, size) under the
// update's seed and counter (host words, or the device words idx_dev points to).  Args: an update's argument struct.
template <class Args>
__device__ __forceinline__ int64_t replay_draw_row(const Args& a, int b) {
  if (a.idx) return a.idx[b];
  uint64_t counter = a.idx_counter; uint32_t size = (uint32_t)a.idx_size;
  if (a.idx_dev) { const uint64_t* d = static_cast<const uint64_t*>(a.idx_dev); counter = d[0]; size = (uint32_t)(int64_t)d[1]; }
  int bits = 2;
  while (((int64_t)1 << bits) < (int64_t)size) ++bits;
  return keyed_permute((uint32_t)b, size, bits / 2, bits - bits / 2, a.idx_seed ^ 0x5265706C61794944ull, counter);
}

// The acting kernels' tail for lane t < 64 of the first wave, one lane per env: Pendulum step with auto-reset under act[]
// (read only where t < nrows), the replay row at (cursor + i) % cap, the outputs, the episode statistics (every lane of the
// wave takes part in their sum).  lds + L.S: the observations the network has just read.  Args: an acting argument struct.
template <class Args>
__device__ __forceinline__ void pendulum_act_tail(const Args& a, const float* lds, const Lds& L, int t, int row0, int nrows, const float (&act)[kMaxA]) {
  const bool ok = t < nrows;
  const int D = a.D, A = a.A;
  ClassicStep<3> r;
  r.done = false; r.ret = 0.0; r.len = 0;
  if (ok) {
    const int i = row0 + t;
    const PendulumState st(a.env_state, a.N);
    pendulum_step_one(st, i, a.env_seed, a.env_id0, act[0], r);
    const int64_t cursor = a.cursor_dev ? a.cursor_dev[0] : a.cursor;
    const int64_t row = (cursor + i) % a.cap;
    for (int k = 0; k < D; ++k) {
      a.r_state[row * D + k] = lds[L.S + t * kMaxD + k];
      a.r_next[row * D + k] = r.o_term[k];              // the TERMINAL observation is what the buffer keeps (sac_pendulum.py:283)
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

// The same tail for a classic-control env under a discrete action, KIND = CartPole-v1, MountainCar-v0 or Acrobot-v1 (ClassicEnv of
// env_classic_device.hpp: the stepper's own arithmetic and auto-reset): the ring row {state, uint32 action word, reward, TERMINAL
// observation, done} at (cursor + i) % cap, the outputs env.step(..., done_out, term_obs_out, ep_ret_out) + memory.push write.  The
// row loops run over the kind's own width (ClassicDims::kObs) and unroll per env — but for CartPole, whose instance keeps the run-time
// a.D (== 4: act_args_ok) it has always looped over, so that the kernels a CartPole run launches stay instruction for instruction
// what they were (DESIGN 4ad has what the constant width would change there).  (Rainbow's tail pushes into an n-step window between
// the step and the ring row and keeps its own copy.)
template <int KIND, class Args>
__device__ __forceinline__ void classic_act_tail(const Args& a, const float* lds, const Lds& L, int t, int row0, int nrows, int act) {
  using Env = ClassicEnv<KIND>;
  const int D = KIND == GYMRL_ENV_CARTPOLE ? a.D : (int)Env::kObs;
  const bool ok = t < nrows;
  ClassicStep<Env::kObs> r;
  r.done = false; r.ret = 0.0; r.len = 0;
  if (ok) {
    const int i = row0 + t;
    const typename Env::State st(a.env_state, a.N);
    Env::step(st, i, a.env_seed, a.env_id0, act, r);
    const int64_t cursor = a.cursor_dev ? a.cursor_dev[0] : a.cursor;
    const int64_t row = (cursor + i) % a.cap;
    for (int k = 0; k < D; ++k) {
      a.r_state[row * D + k] = lds[L.S + t * kMaxD + k];
      a.r_next[row * D + k] = r.o_term[k];
      a.obs_out[(size_t)i * D + k] = r.o_next[k];
    }
    a.r_action[row] = (uint32_t)act;
    a.r_reward[row] = r.reward;
    a.r_flag[row] = r.done;
    if (a.action_out) a.action_out[i] = act;
    if (a.rew_out) a.rew_out[i] = r.reward;
    if (a.done_out) a.done_out[i] = r.done;
    if (r.done && a.ep_ret_out) a.ep_ret_out[i] = (float)r.ret;
  }
  accumulate_ep_stats(a.ep_stats, r.done && ok, r.ret, r.len);
}
// its CartPole instance, under the name the two-action kernels (ddqn_step.hip's dueling act, noisy_dqn_step.hip) call
template <class Args>
__device__ __forceinline__ void cartpole_act_tail(const Args& a, const float* lds, const Lds& L, int t, int row0, int nrows, int act) {
  classic_act_tail<GYMRL_ENV_CARTPOLE>(a, lds, L, t, row0, nrows, act);
}

// All weight images (f32[n][H*H]) from the parameters as they are (after load_state_dict / a checkpoint / a hard target copy /
// a layer-by-layer update): grid.y = image, the first n_fwd of them forward images, the rest input-gradient images
// (lin_device.hpp); a null source (DDPG: no second Q network) leaves its image alone
struct PackTable { const float* src[9]; int n_fwd; };
__global__ __launch_bounds__(256) void pack_images_kernel(const PackTable tb, float* images, const int H) {
  const int steps = H >> 4;
  const size_t hh = (size_t)H * H;
  const int which = blockIdx.y;
  if (!tb.src[which]) return;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < hh; o += (size_t)gridDim.x * 256) {
    const int n = (int)(o / H), k = (int)(o % H);
    images[which * hh + (which < tb.n_fwd ? lin::img_fwd_index(n, k, steps) : lin::img_bwd_index(n, k, steps))] = tb.src[which][o];
  }
}

// The tile list of one sac_dw_kernel launch, segment by segment: seg() appends a layer's weight gradient (wave0 / tile0 run on
// over the segments, slices by lin_device.hpp's cut of the batch; the images arrive as the kernels' read-only slots and are
// written here), finish() closes the list, optimiser() sets Adam's fields, close() is both + the target twins' tau and the
// loss terms.  What else a launch needs (the temperature step, Rainbow's split heads) the caller sets on `d` itself.
struct DwBuilder {
  DwArgs& d; int B;
  int w0 = 0, ns = 0, t0 = 0;
  void seg(const float* dZ, int ldz, int N, const float* X, int ldx, const float* X2, int ldx2, int K, int K1, float* W, float* b,
           float* Wt = nullptr, float* bt = nullptr, const float* img_f = nullptr, const float* img_b = nullptr, const float* img_tf = nullptr) {
    DwSeg& s = d.seg[ns++];
    s.dZ = dZ; s.X = X; s.X2 = X2; s.W = W; s.b = b; s.Wt = Wt; s.bt = bt;
    s.img_f = const_cast<float*>(img_f); s.img_b = const_cast<float*>(img_b); s.img_tf = const_cast<float*>(img_tf);
    s.ldz = ldz; s.ldx = ldx; s.ldx2 = ldx2; s.N = N; s.K = K; s.K1 = K1; s.wave0 = w0;
    const int tl = ((N + 15) / 16) * ((K + 15) / 16);
    s.slices = lin::bwd_weight_slices(B, N, K); s.tile0 = t0;
    w0 += tl * s.slices; t0 += tl;
  }
  void finish(float* parts) { d.nseg = ns; d.total_waves = w0; d.total_tiles = t0; d.B = B; d.parts = parts; d.phase = B > 512 ? 1 : 0; }
  void optimiser(float* p, float* m, float* v, const float (&adam)[4], const float* adam_dev, double beta1, double beta2, double eps) {
    d.p = p; d.m = m; d.v = v;
    for (int k = 0; k < 4; ++k) d.adam[k] = adam[k];
    d.adam_dev = adam_dev;
    d.omb1 = (float)(1.0 - beta1); d.beta2 = (float)beta2; d.omb2 = (float)(1.0 - beta2); d.eps = (float)eps;
  }
  // Args: an update's argument struct (beta1, beta2, eps_adam); terms [term0, term0 + nterms) of `terms` (+ terms_b on term 0) -> sums
  template <class Args>
  void close(const Args& a, float* parts, float* p, float* m, float* v, const float (&adam)[4], const float* adam_dev, float tau, float omt,
             const double* terms, const double* terms_b, int term0, int nterms, double* sums) {
    finish(parts);
    optimiser(p, m, v, adam, adam_dev, a.beta1, a.beta2, a.eps_adam);
    d.tau = tau; d.omt = omt;
    d.terms = terms; d.terms_b = terms_b; d.term0 = term0; d.nterms = nterms; d.sums = sums; d.alpha_step = 0;
  }
};

}  // namespace
}  // namespace slab
}  // namespace gymrl

// actor_impl.h -- the actor kernel (include/beacon_actor.h: bcn_actor_act, bcn_actor_values), templated on the real type and
// instantiated by actor.hip (float32, the hot path) and actor_f64.hip (float64).  The networks -- tile, staging, layers, the head's
// log-density terms -- are policy_net.h; here: the two MLPs on the tile, then one lane per replica draws and writes.
// With cfg.agents = A > 1 a "replica" below is a ROW, agent b % A of replica b / A: only the mask is indexed per replica (b / A),
// and the host passes replica_offset A as the index of row 0.
#pragma once
#include "../env1d.h"                     // bcn_philox4x32: the project's one Philox definition
#include "policy_net.h"

template <typename real>
struct ActorArgs {
  const real* params;
  const real* obs;                  // [n_rows][obs_dim]
  long long n_rows;
  int obs_dim, n_hidden, hidden[BCN_ACTOR_MAX_LAYERS], activation, kind, act_dim;
  int hmax_pad;                     // rows of one activation buffer: the widest hidden layer
  int wcols;                        // columns of the weight slab: the widest layer output, rounded up to 4, + 4
  real low, high;
  ActorNet pi, vf;
  unsigned log_std;                 // element offset
  int values_only;                  // bcn_actor_values: the value network alone, into value_out
  // state
  uint32_t* counters;
  void* actions;                    // real [B][act_dim] or int32 [B]
  real *raw, *logp, *value, *dist;
  const uint8_t* mask;              // [n_rows / agents]: one byte per replica
  uint32_t seed_lo, seed_hi;
  long long replica_offset;         // the global index of row 0: the first replica's times agents
  int deterministic;
  const int32_t* cursor;
  int T;
  real *logp_seq, *value_seq, *raw_seq;
  int agents;                       // rows per replica, >= 1 (last: the fields above keep their offsets)
};

// ln u1 and 2 u2 of the Box-Muller pair from the four Philox words (beacon_actor.h).
// float32: k + 0.5 with k = w0 >> 8 is exact only below 2^23; above, u1 = 1 - (2^24 - k - 0.5) 2^-24 with an exact bracket, and
// log1p keeps the bits that forming u1 itself would round away (u1 -> 1 is where the radius is small).
__device__ __forceinline__ void actor_bm_uniforms(const uint32_t (&w)[4], float& ln_u1, float& two_u2) {
  const uint32_t k = w[0] >> 8;
  if (k < (1u << 23)) ln_u1 = logf(((float)k + 0.5f) * (1.0f / 16777216.0f));
  else ln_u1 = log1pf(-(((float)((1u << 24) - k) - 0.5f) * (1.0f / 16777216.0f)));
  two_u2 = (float)(w[1] >> 8) * (1.0f / 8388608.0f);
}
__device__ __forceinline__ void actor_bm_uniforms(const uint32_t (&w)[4], double& ln_u1, double& two_u2) {
  const unsigned long long r1 = ((unsigned long long)w[0] << 21) ^ (unsigned long long)(w[1] >> 11);
  const unsigned long long r2 = ((unsigned long long)w[2] << 21) ^ (unsigned long long)(w[3] >> 11);
  ln_u1 = log(((double)r1 + 0.5) * (1.0 / 9007199254740992.0));
  two_u2 = (double)r2 * (1.0 / 4503599627370496.0);
}
__device__ __forceinline__ float actor_single_uniform(const uint32_t (&w)[4], float) { return (float)(w[0] >> 8) * (1.0f / 16777216.0f); }
__device__ __forceinline__ double actor_single_uniform(const uint32_t (&w)[4], double) {
  return (double)(((unsigned long long)w[0] << 21) ^ (unsigned long long)(w[1] >> 11)) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ void actor_sincospi(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void actor_sincospi(double x, double* s, double* c) { sincospi(x, s, c); }

template <typename real>
__global__ __launch_bounds__(ACTOR_NT) void actor_kernel(const ActorArgs<real> A) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char actor_lds[];
  real* hA = reinterpret_cast<real*>(actor_lds);      // two activation buffers [hmax_pad][TBP], used in turn
  real* hB = hA + (size_t)A.hmax_pad * TBP;
  real* xs = hB + (size_t)A.hmax_pad * TBP;           // [KS][TBP]
  real* ws = xs + (size_t)KS * TBP;                   // [KS][wcols]
  real* pi = ws + (size_t)KS * A.wcols;               // [BCN_ACTOR_MAX_ACT][TBP]
  real* vf = pi + (size_t)BCN_ACTOR_MAX_ACT * TBP;    // [1][TBP]
  const long long row0 = (long long)blockIdx.x * TB;

  const auto out_of = [=](int l) { return (l & 1) ? hB : hA; };
  if (!A.values_only) policy_mlp<real, false>(A, A.pi, A.act_dim, row0, nullptr, out_of, xs, ws, pi);
  policy_mlp<real, false>(A, A.vf, 1, row0, nullptr, out_of, xs, ws, vf);
  __syncthreads();

  // one lane per replica from here on: it alone owns the replica's output rows and its counter
  const int r = threadIdx.x;
  const long long b = row0 + r;
  if (r >= TB || b >= A.n_rows) return;
  const real value = vf[r];
  if (A.values_only) { A.value[b] = value; return; }
  // the mask is per replica: with agents the row's byte is b / agents (b < 2^31, cfg.batch is an int32: one 32-bit division per row)
  if (A.mask && A.mask[A.agents > 1 ? (long long)((uint32_t)b / (uint32_t)A.agents) : b] == 0) return;

  const int n = A.act_dim;
  real head[BCN_ACTOR_MAX_ACT], rawv[BCN_ACTOR_MAX_ACT];
#pragma unroll
  for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) head[i] = i < n ? pi[i * TBP + r] : real(0);
  const uint32_t ctr = A.counters[b];
  const uint32_t gb = (uint32_t)(unsigned long long)(A.replica_offset + b);
  real logp = real(0);
  const real* log_std = A.params + A.log_std;

  if (A.kind == BCN_ACTOR_GAUSSIAN) {
    real* act_out = static_cast<real*>(A.actions);
#pragma unroll
    for (int j = 0; j < BCN_ACTOR_MAX_ACT / 2; j++) {
      if (2 * j >= n) break;
      real z0 = real(0), z1 = real(0);
      if (!A.deterministic) {
        uint32_t w[4];
        bcn_philox4x32(gb, ctr, (uint32_t)j, 2u, A.seed_lo, A.seed_hi, w);
        real ln_u1, two_u2, s, c;
        actor_bm_uniforms(w, ln_u1, two_u2);
        const real radius = sqrt(real(-2) * ln_u1);
        actor_sincospi(two_u2, &s, &c);
        z0 = radius * c;
        z1 = radius * s;
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int i = 2 * j + h;
        if (i >= n) break;
        const real z = h ? z1 : z0, ls = log_std[i];
        const real rw = A.deterministic ? head[i] : head[i] + actor_exp(ls) * z;
        rawv[i] = rw;
        logp += policy_gauss_logp<real>(z, ls);
        act_out[b * n + i] = rw < A.low ? A.low : (rw > A.high ? A.high : rw);
        A.raw[b * n + i] = rw;
        A.dist[b * n + i] = head[i];
      }
    }
  } else {
    POLICY_LOG_SUM_EXP(head, n)
    real d[BCN_ACTOR_MAX_ACT];
#pragma unroll
    for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) d[i] = i < n ? (head[i] - mx) - lse : real(0);
    int a = n - 1;
    if (A.deterministic) {
      a = 0;
      real best = d[0];
#pragma unroll
      for (int i = 1; i < BCN_ACTOR_MAX_ACT; i++)
        if (i < n && d[i] > best) { best = d[i]; a = i; }
    } else {
      uint32_t w[4];
      bcn_philox4x32(gb, ctr, 0u, 2u, A.seed_lo, A.seed_hi, w);
      const real u = actor_single_uniform(w, real(0));
      real cum = real(0);
      bool found = false;
#pragma unroll
      for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) {
        if (i < n - 1 && !found) {
          cum += actor_exp(d[i]);
          if (u < cum) { a = i; found = true; }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) {
      if (i < n) {
        rawv[i] = head[i];
        A.raw[b * n + i] = head[i];
        A.dist[b * n + i] = d[i];
        if (i == a) logp = d[i];
      }
    }
    static_cast<int32_t*>(A.actions)[b] = a;
  }
  A.logp[b] = logp;
  A.value[b] = value;
  if (!A.deterministic) A.counters[b] = ctr + 1u;
  if (A.cursor) {
    const int t = A.cursor[0];
    if (t >= 0 && t < A.T) {
      const long long s = (long long)t * A.n_rows + b;
      A.logp_seq[s] = logp;
      A.value_seq[s] = value;
#pragma unroll
      for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)
        if (i < n) A.raw_seq[s * n + i] = rawv[i];
    }
  }
}

// bytes of dynamic LDS of one workgroup
template <typename real>
inline size_t actor_lds_bytes(int hmax_pad, int wcols) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  return sizeof(real) * ((size_t)2 * hmax_pad * TBP + (size_t)KS * TBP + (size_t)KS * wcols + (size_t)(BCN_ACTOR_MAX_ACT + 1) * TBP);
}

// defined by actor.hip (float) and actor_f64.hip (double): the launch, hipError_t as int
template <typename real> int actor_launch(const ActorArgs<real>& a, void* stream);

#define ACTOR_DEFINE_LAUNCH(real)                                                                                      \
  template <> int actor_launch<real>(const ActorArgs<real>& a, void* stream) {                                         \
    constexpr int TB = ActorGeom<real>::TB;                                                                            \
    const size_t lds = actor_lds_bytes<real>(a.hmax_pad, a.wcols);                                                     \
    static size_t lds_allowed[64] = {0};                                                                               \
    const hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(&actor_kernel<real>), lds, lds_allowed);       \
    if (e != hipSuccess) return (int)e;                                                                                \
    const unsigned nblk = (unsigned)((a.n_rows + TB - 1) / TB);                                                        \
    hipLaunchKernelGGL(actor_kernel<real>, dim3(nblk), dim3(ACTOR_NT), lds, static_cast<hipStream_t>(stream), a);      \
    return (int)hipGetLastError();                                                                                     \
  }

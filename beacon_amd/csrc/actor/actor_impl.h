// actor_impl.h -- the actor kernel (include/beacon_actor.h: bcn_actor_act, bcn_actor_values), templated on the real type and
// instantiated by actor.hip (float32, the hot path) and actor_f64.hip (float64).
//
// A workgroup of 256 lanes owns a tile of TB replicas (64 in float32, 32 in float64) and runs the two MLPs on it one after the
// other, layer by layer.  Activations live in LDS k-major, h[k][replica] with TBP = TB + 4 columns, so that the four consecutive
// replicas of a lane are one 16-byte read (float32) and the outputs of a layer are written as such rows.  A layer's weights are
// staged per K-slab of KS rows, transposed to w[k][out]: the largest matrix, 128 x 512 float32, is 256 KB and never fits the 160 KB
// LDS as a whole, a slab of it is 33 KB.  The first layer's input is staged the same way from the observation rows in HBM.
//
// Each lane keeps a register tile of (4 NPASS) replicas x 4 outputs: lane = og * nrg + rg with nog = the power of two >=
// ceil(out / 4) output groups and nrg = 256 / nog replica groups (NPASS = 2 when nog = 32, i.e. out > 64: the tile's replicas in
// two halves).  Per k a lane reads one 16-byte weight chunk (shared by the nrg lanes of its output group: a broadcast) and one
// replica chunk per pass (consecutive lanes read consecutive chunks: conflict-free), 2 reads for 16 fma.  Plain fma, not the
// float32 MFMA: the matrix rate equals the vector rate on gfx950 and both are exact fma chains, so MFMA would only save LDS reads --
// and its 32x32 / 16x16 output blocks would leave 3/4 of the lanes' work on padding at the widths an RL policy has (a head of 1 ..
// 16 outputs, obs_dim 6) while the k-ordered chain per output that the header promises (and bcn_actor_values repeats bit for bit)
// falls out of the plain form for every shape.
//
// Rows of a partial tile are staged as zeros and never stored; columns of a partial slab are not looped over: nothing is read
// past a row or past the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../env1d.h"                     // bcn_philox4x32: the project's one Philox definition
#include "../../../include/beacon_actor.h"

#define ACTOR_NT 256

template <typename real> struct ActorGeom;
template <> struct ActorGeom<float> { static constexpr int TB = 64, KS = 64; };
template <> struct ActorGeom<double> { static constexpr int TB = 32, KS = 32; };

// four consecutive reals of an LDS row, 16-byte aligned: one ds_read_b128 (float32) or two (float64)
template <typename real> struct alignas(16) ActorV4 { real v[4]; };

struct ActorNet {
  // element offsets into the parameter buffer: layers 0 .. n_hidden - 1 and the head (index n_hidden)
  unsigned w[BCN_ACTOR_MAX_LAYERS + 1], b[BCN_ACTOR_MAX_LAYERS + 1];
};

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
  const uint8_t* mask;
  uint32_t seed_lo, seed_hi;
  long long replica_offset;
  int deterministic;
  const int32_t* cursor;
  int T;
  real *logp_seq, *value_seq, *raw_seq;
};

__device__ __forceinline__ float actor_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double actor_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float actor_exp(float x) { return expf(x); }
__device__ __forceinline__ double actor_exp(double x) { return exp(x); }
__device__ __forceinline__ float actor_log(float x) { return logf(x); }
__device__ __forceinline__ double actor_log(double x) { return log(x); }
__device__ __forceinline__ float actor_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double actor_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

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

// Stage ks columns (from k0 on) of the first `rows` rows of the row-major matrix src[.][K] into LDS transposed, dst[k * ld + row], and
// zeros for the rows from `valid` up to `rows`.  The global loads of ACTOR_STAGE_U elements per lane are issued before the first LDS
// store, so one round trip to memory covers all of them (issued one by one, the round trips of a slab added up to most of a launch).
#define ACTOR_STAGE_U 8
template <typename real>
__device__ __forceinline__ void actor_stage(const real* __restrict__ src, int K, int k0, int ks, int rows, int valid, real* dst, int ld) {
  const int total = rows * ks;
  for (int e0 = threadIdx.x; e0 < total; e0 += ACTOR_NT * ACTOR_STAGE_U) {
    real v[ACTOR_STAGE_U];
    int at[ACTOR_STAGE_U];
#pragma unroll
    for (int u = 0; u < ACTOR_STAGE_U; u++) {
      const int e = e0 + u * ACTOR_NT;
      const int r = e / ks, k = e - r * ks;
      at[u] = e < total ? k * ld + r : -1;
      v[u] = (e < total && r < valid) ? src[(size_t)r * K + k0 + k] : real(0);
    }
#pragma unroll
    for (int u = 0; u < ACTOR_STAGE_U; u++)
      if (at[u] >= 0) dst[at[u]] = v[u];
  }
}

// One layer on the workgroup's tile: out[o][r] = f(b[o] + sum_k W[o][k] in[k][r]) for o < OUT, r < TB.
//   xin   the input k-major in LDS (row stride TBP), or nullptr: the rows of `obs` from `row0` on (staged per slab into xs)
//   out   LDS, row stride TBP (must not alias xin)
//   f     0 tanh, 1 relu, 2 identity
template <typename real>
__device__ __forceinline__ void actor_layer(const real* __restrict__ W, const real* __restrict__ bias, int K, int OUT, int f, const real* xin,
                                            const real* __restrict__ obs, long long row0, long long n_rows, real* xs, real* ws, int wcols,
                                            real* out) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  constexpr int NPASS = 2;
  const int lane = threadIdx.x;
  const int out4 = (OUT + 3) & ~3;
  int nog = 1;
  while (nog * 4 < out4) nog <<= 1;                 // <= 32: OUT <= 128
  const int nrg = ACTOR_NT / nog;
  const int og = lane / nrg, rg = lane - og * nrg;
  const int o0 = og * 4;
  const bool has_out = o0 < out4;

  real acc[NPASS][4][4];                            // [pass][replica][output]
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const real bj = (has_out && o0 + j < OUT) ? bias[o0 + j] : real(0);
#pragma unroll
    for (int p = 0; p < NPASS; p++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[p][i][j] = bj;
  }
  const int r_a = rg * 4, r_b = (nrg + rg) * 4;     // first replica of pass 0 / pass 1
  const bool act_a = has_out && r_a < TB, act_b = has_out && r_b < TB;

  for (int k0 = 0; k0 < K; k0 += KS) {
    const int ks = min(KS, K - k0);
    __syncthreads();                                // the previous slab's (or layer's) readers of ws / xs are done
    // weights: W[o][k0 + k] -> ws[k][o], o < out4 (zeros behind OUT); consecutive lanes read consecutive k of one row
    actor_stage<real>(W, K, k0, ks, out4, OUT, ws, wcols);
    // observations: obs[row0 + r][k0 + k] -> xs[k][r]; rows behind the batch: zeros
    if (xin == nullptr) actor_stage<real>(obs + (size_t)row0 * K, K, k0, ks, TB, (int)min((long long)TB, n_rows - row0), xs, TBP);
    __syncthreads();
    const real* x = xin ? xin + (size_t)k0 * TBP : xs;
    if (act_a) {
#pragma unroll 4
      for (int k = 0; k < ks; k++) {               // four steps' LDS reads are in flight before the first fma needs one
        const ActorV4<real> wq = *reinterpret_cast<const ActorV4<real>*>(ws + k * wcols + o0);
        const ActorV4<real> xq = *reinterpret_cast<const ActorV4<real>*>(x + k * TBP + r_a);
        const real* wv = wq.v;
        const real* xa = xq.v;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[0][i][j] = actor_fma(wv[j], xa[i], acc[0][i][j]);
        if (act_b) {
          const ActorV4<real> xr = *reinterpret_cast<const ActorV4<real>*>(x + k * TBP + r_b);
          const real* xb = xr.v;
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[1][i][j] = actor_fma(wv[j], xb[i], acc[1][i][j]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NPASS; p++) {
    const int r0 = p ? r_b : r_a;
    if (!(p ? act_b : act_a)) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (o0 + j >= OUT) continue;
      ActorV4<real> q;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        real v = acc[p][i][j];
        if (f == 0) v = actor_tanh(v);
        else if (f == 1) v = v > real(0) ? v : real(0);
        q.v[i] = v;
      }
      *reinterpret_cast<ActorV4<real>*>(out + (o0 + j) * TBP + r0) = q;
    }
  }
}

// One MLP on the tile; the head's outputs land in `head` (LDS, [n_head][TBP]).
template <typename real>
__device__ __forceinline__ void actor_mlp(const ActorArgs<real>& A, const ActorNet& net, int n_head, long long row0, real* hA, real* hB, real* xs,
                                          real* ws, real* head) {
  const real* in = nullptr;
  int K = A.obs_dim;
  for (int l = 0; l < A.n_hidden; l++) {
    real* o = (l & 1) ? hB : hA;
    actor_layer<real>(A.params + net.w[l], A.params + net.b[l], K, A.hidden[l], A.activation, in, A.obs, row0, A.n_rows, xs, ws, A.wcols, o);
    in = o;
    K = A.hidden[l];
  }
  actor_layer<real>(A.params + net.w[A.n_hidden], A.params + net.b[A.n_hidden], K, n_head, 2, in, A.obs, row0, A.n_rows, xs, ws, A.wcols, head);
}

template <typename real>
__global__ __launch_bounds__(ACTOR_NT) void actor_kernel(const ActorArgs<real> A) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char actor_lds[];
  real* hA = reinterpret_cast<real*>(actor_lds);
  real* hB = hA + (size_t)A.hmax_pad * TBP;
  real* xs = hB + (size_t)A.hmax_pad * TBP;           // [KS][TBP]
  real* ws = xs + (size_t)KS * TBP;                   // [KS][wcols]
  real* pi = ws + (size_t)KS * A.wcols;               // [BCN_ACTOR_MAX_ACT][TBP]
  real* vf = pi + (size_t)BCN_ACTOR_MAX_ACT * TBP;    // [1][TBP]
  const long long row0 = (long long)blockIdx.x * TB;

  if (!A.values_only) actor_mlp<real>(A, A.pi, A.act_dim, row0, hA, hB, xs, ws, pi);
  actor_mlp<real>(A, A.vf, 1, row0, hA, hB, xs, ws, vf);
  __syncthreads();

  // one lane per replica from here on: it alone owns the replica's output rows and its counter
  const int r = threadIdx.x;
  const long long b = row0 + r;
  if (r >= TB || b >= A.n_rows) return;
  const real value = vf[r];
  if (A.values_only) { A.value[b] = value; return; }
  if (A.mask && A.mask[b] == 0) return;

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
        logp += (real(-0.5) * z * z - ls) - real(0.91893853320467274178);
        act_out[b * n + i] = rw < A.low ? A.low : (rw > A.high ? A.high : rw);
        A.raw[b * n + i] = rw;
        A.dist[b * n + i] = head[i];
      }
    }
  } else {
    real mx = head[0];
#pragma unroll
    for (int i = 1; i < BCN_ACTOR_MAX_ACT; i++)
      if (i < n && head[i] > mx) mx = head[i];
    real se = real(0);
#pragma unroll
    for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)
      if (i < n) se += actor_exp(head[i] - mx);
    const real lse = actor_log(se);
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
    int dev = 0;                                                                                                       \
    hipError_t e = hipGetDevice(&dev);                                                                                 \
    if (e != hipSuccess) return (int)e;                                                                                \
    if (lds > 48 * 1024 && (dev < 0 || dev >= 64 || lds_allowed[dev] < lds)) {                                         \
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&actor_kernel<real>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                              160 * 1024);                                                                             \
      if (e != hipSuccess) return (int)e;                                                                              \
      if (dev >= 0 && dev < 64) lds_allowed[dev] = 160 * 1024;                                                         \
    }                                                                                                                  \
    const unsigned nblk = (unsigned)((a.n_rows + TB - 1) / TB);                                                        \
    hipLaunchKernelGGL(actor_kernel<real>, dim3(nblk), dim3(ACTOR_NT), lds, static_cast<hipStream_t>(stream), a);      \
    return (int)hipGetLastError();                                                                                     \
  }

// es_impl.h -- the kernels of libbeacon_es.so (include/beacon_es.h), templated on the real type and instantiated by es.hip (float32)
// and es_f64.hip (float64).
//
// The Box-Muller pair (td3_normal_pair), the tree (td3_tree) and the finish and Adam kernels are ../td3/td3_impl.h's templates,
// instantiated in this unit (that file and ../actor/policy_net.h are included, not changed; nothing of another library is linked).
// policy_layer shares ONE weight slab across a tile of rows; here every member has its own weights, so the population's network is a
// tile kernel of its own:
//   es_act_kernel      the MLP of replica b with row b / R of the population (or the one shared row), and the action
//   es_begin_kernel    the antithetic perturbation and the reset of the fitness bookkeeping
//   es_observe_kernel  the fitness bookkeeping behind a step
//   es_fit_kernel, es_rank_kernel, es_partial_kernel, es_reduce_kernel, es_tick_kernel    the update in front of finish and Adam
//
// es_act_kernel.  A workgroup of 256 lanes owns a tile of at most TR = BCN_ES_TILE_ROWS consecutive rows of the batch: the rows of G
// consecutive members (G R <= TR), or TR rows of one member whose rows it walks tile after tile.  Activations live in LDS row-major,
// h[row][HP], in two buffers used in turn.  Per layer and per slab of KS reduction steps the slab of every member of the tile is
// copied as it lies in HBM -- consecutive lanes load consecutive 16-byte chunks of one matrix row -- into ws[(member, output)][LDK]
// with LDK = KS + 4.  A lane owns (row, output) pairs, pair = lane, lane + 256, ...; for a pair it walks k in steps of four: one
// 16-byte read of its weight row and one of its input row per four fma.
// LDS banks: the 16 lanes that one ds_read_b128 group serves hold 16 consecutive outputs of one row, their weight rows lie LDK = KS + 4
// reals apart, and KS is a multiple of 8: in float32 (KS + 4) / 4 is odd, so the 16 rows start in 16 different 16-byte slots of the
// 256-byte bank row -- conflict-free; the input read is one address for the group, a broadcast.  (Stored transposed as policy_layer
// stores it, the weight read would be conflict-free too, but the staging writes of one matrix row would all land on a few banks.)
// The running sum of a pair is kept in the output buffer between slabs (the pair's own word: no other lane touches it).
// LDS: sizeof(real) (2 TR HP + TR LDK + G nmax LDK) bytes; at 3 x 128, G = 1: 76 288 in float32, 111 616 in float64, of 163 840.
// No atomics, no inter-workgroup communication inside a launch.
#pragma once
#include "../td3/td3_impl.h"              // actor_impl.h, policy_net.h and env1d.h (bcn_philox4x32) come with it
#include "../../../include/beacon_es.h"

#define ES_NT TD3_NT
#define ES_TR BCN_ES_TILE_ROWS
#define ES_MAX_PSEGS (2 * (BCN_ACTOR_MAX_LAYERS + 1))
static_assert(BCN_ES_MAX_ACT == BCN_ACTOR_MAX_ACT, "the head's width is the actor's");
static_assert(BCN_ES_N_STATS <= ES_NT, "one lane per statistic");

template <typename real> struct EsGeom;
template <> struct EsGeom<float> { static constexpr int KS = 64; };
template <> struct EsGeom<double> { static constexpr int KS = 32; };

// the parameter layout: element offsets and counts of the segments w0, b0, w1, b1, ...
struct EsLayout {
  int n_segs;
  unsigned off[ES_MAX_PSEGS], cnt[ES_MAX_PSEGS];
  unsigned E;
};

__device__ __forceinline__ bool es_is_gap(const EsLayout& L, unsigned e) {
  bool in = false;
  for (int s = 0; s < L.n_segs; s++) in = in || (e >= L.off[s] && e - L.off[s] < L.cnt[s]);
  return !in;
}

// ---- acting ---------------------------------------------------------------------------------------------------------------------------
template <typename real>
struct EsActArgs {
  const real* weights;        // [M][E], or one row (shared)
  const real* obs;            // [B][obs_dim]
  const uint8_t* mask;
  real* actions;              // Box
  int32_t* actions_i;         // Discrete
  long long B, R;             // the batch; rows per member (shared: B, one member)
  int M;                      // members (shared: 1)
  int G;                      // members per workgroup (1 where R > TR)
  long long tiles;            // R > TR: tiles per member, ceil(R / TR); else 0
  int split;                  // R > TR: workgroups per member
  int obs_dim, n_out, n_hidden, hidden[BCN_ACTOR_MAX_LAYERS], activation, kind;
  int HP, nmax;
  real center, half;
  EsLayout lay;
};

// the slab [N][q0 .. q0 + ks) of the row-major matrix W[N][K] into dst[o * LDK + k]; four loads per lane in flight before the first store
template <typename real>
__device__ __forceinline__ void es_stage_w(const real* __restrict__ W, int N, int K, int q0, int ks, real* dst) {
  constexpr int LDK = EsGeom<real>::KS + 4, U = 4;
  if ((K & 3) == 0) {                                 // every chunk of four lies in one matrix row, 16-byte aligned (float64: 32)
    const int kc = ks >> 2, total = N * kc;
    for (int c0 = threadIdx.x; c0 < total; c0 += ES_NT * U) {
      ActorV4<real> v[U];
      int at[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int c = c0 + u * ES_NT;
        at[u] = -1;
        if (c < total) {
          const int o = c / kc, k = (c - o * kc) << 2;
          at[u] = o * LDK + k;
          v[u] = *reinterpret_cast<const ActorV4<real>*>(W + (size_t)o * K + q0 + k);
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (at[u] >= 0) *reinterpret_cast<ActorV4<real>*>(dst + at[u]) = v[u];
    }
  } else {
    const int total = N * ks;
    for (int c0 = threadIdx.x; c0 < total; c0 += ES_NT * U) {
      real v[U];
      int at[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int c = c0 + u * ES_NT;
        at[u] = -1;
        if (c < total) {
          const int o = c / ks, k = c - o * ks;
          at[u] = o * LDK + k;
          v[u] = W[(size_t)o * K + q0 + k];
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (at[u] >= 0) dst[at[u]] = v[u];
    }
  }
}

template <typename real>
__global__ __launch_bounds__(ES_NT) void es_act_kernel(const EsActArgs<real> A) {
  constexpr int TR = ES_TR, KS = EsGeom<real>::KS, LDK = KS + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char es_lds[];
  real* hA = reinterpret_cast<real*>(es_lds);         // [TR][HP]
  real* hB = hA + (size_t)TR * A.HP;                  // [TR][HP]
  real* xs = hB + (size_t)TR * A.HP;                  // [TR][LDK]
  real* ws = xs + (size_t)TR * LDK;                   // [G nmax][LDK]
  const int HP = A.HP, tid = threadIdx.x;

  // this workgroup's member(s) and tiles
  long long tile = 0, tile_end = 1, tile_step = 1;
  int p0, nm;
  if (A.tiles > 0) {                                  // one member, its tiles tile, tile + split, ...
    p0 = (int)(blockIdx.x / (unsigned)A.split);
    nm = 1;
    tile = blockIdx.x - (unsigned)p0 * (unsigned)A.split;
    tile_end = A.tiles;
    tile_step = A.split;
  } else {
    p0 = (int)blockIdx.x * A.G;
    nm = min(A.G, A.M - p0);
  }
  for (; tile < tile_end; tile += tile_step) {
    long long b0;
    int rows, rpm;                                    // rows of the tile; rows per member in it
    if (A.tiles > 0) {
      b0 = (long long)p0 * A.R + tile * TR;
      rows = (int)min((long long)TR, A.R - tile * TR);
      rpm = TR;                                       // r / rpm = 0: the one member
    } else {
      b0 = (long long)p0 * A.R;
      rows = nm * (int)A.R;
      rpm = (int)A.R;
    }
    const real* in = nullptr;
    int K = A.obs_dim;
    for (int l = 0; l <= A.n_hidden; l++) {
      const int N = l < A.n_hidden ? A.hidden[l] : A.n_out;
      const int f = l < A.n_hidden ? A.activation : 2;
      real* out = (l & 1) ? hB : hA;
      const unsigned w_off = A.lay.off[2 * l], b_off = A.lay.off[2 * l + 1];
      for (int q0 = 0; q0 < K; q0 += KS) {
        const int ks = min(KS, K - q0);
        __syncthreads();                              // the previous slab's (layer's, tile's) readers of ws / xs are done, its writers too
        for (int mi = 0; mi < nm; mi++)
          es_stage_w<real>(A.weights + (size_t)(p0 + mi) * A.lay.E + w_off, N, K, q0, ks, ws + (size_t)mi * N * LDK);
        if (l == 0) {
          const int total = rows * ks;
          for (int e = tid; e < total; e += ES_NT) {
            const int r = e / ks, k = e - r * ks;
            xs[r * LDK + k] = A.obs[(size_t)(b0 + r) * K + q0 + k];
          }
        }
        __syncthreads();
        const real* x = l == 0 ? xs : in + q0;
        const int xld = l == 0 ? LDK : HP;
        const bool last = q0 + ks >= K;
        const int pairs = rows * N;
        for (int idx = tid; idx < pairs; idx += ES_NT) {
          const int r = idx / N, o = idx - r * N;
          const int mi = r / rpm;
          real acc = q0 == 0 ? A.weights[(size_t)(p0 + mi) * A.lay.E + b_off + o] : out[r * HP + o];
          const real* wrow = ws + ((size_t)mi * N + o) * LDK;
          const real* xrow = x + (size_t)r * xld;
          int k = 0;
#pragma unroll 4
          for (; k + 4 <= ks; k += 4) {
            const ActorV4<real> wq = *reinterpret_cast<const ActorV4<real>*>(wrow + k);
            const ActorV4<real> xq = *reinterpret_cast<const ActorV4<real>*>(xrow + k);
#pragma unroll
            for (int i = 0; i < 4; i++) acc = actor_fma(wq.v[i], xq.v[i], acc);
          }
          for (; k < ks; k++) acc = actor_fma(wrow[k], xrow[k], acc);
          if (last) {
            if (f == 0) acc = actor_tanh(acc);
            else if (f == 1) acc = acc > real(0) ? acc : real(0);
          }
          out[r * HP + o] = acc;
        }
      }
      in = out;
      K = N;
    }
    __syncthreads();                                  // the head's outputs are complete
    if (tid < rows) {
      const long long b = b0 + tid;
      if (!(A.mask && A.mask[b] == 0)) {
        const real* head = in + (size_t)tid * HP;
        const int n = A.n_out;
        if (A.kind == BCN_ES_BOX) {
          real* o = A.actions + b * n;
          for (int i = 0; i < n; i++) {
            const real mu = A.center + A.half * actor_tanh(head[i]);
            o[i] = mu;
          }
        } else {
          real best = -INFINITY;
          int arg = 0;
          for (int j = 0; j < n; j++) {
            const real q = head[j];
            if (q > best) { best = q; arg = j; }
          }
          A.actions_i[b] = arg;
        }
      }
    }
  }
}

// ---- begin ------------------------------------------------------------------------------------------------------------------------------
template <typename real>
struct EsBeginArgs {
  const real* theta;
  real* pop;
  const int32_t* gen;
  double* fit;
  int32_t* len;
  uint8_t* alive;
  long long B;
  int M;
  real sigma;
  uint32_t k0, k1;
  EsLayout lay;
};

// one lane per (pair j, element pair h): the four words pop[2j][2h], pop[2j][2h + 1], pop[2j + 1][2h], pop[2j + 1][2h + 1]; the lanes
// i < B also reset replica i's bookkeeping
template <typename real>
__global__ __launch_bounds__(ES_NT) void es_begin_kernel(const EsBeginArgs<real> A) {
  const long long i = (long long)blockIdx.x * ES_NT + threadIdx.x;
  if (i < A.B) {
    A.fit[i] = 0.0;
    A.len[i] = 0;
    A.alive[i] = 1;
  }
  const unsigned E = A.lay.E, half = E >> 1;          // E is even: the buffer is a multiple of 16 bytes
  const long long j = i / half;
  const unsigned h = (unsigned)(i - j * half);
  if (j >= A.M / 2) return;
  real z[2] = {real(0), real(0)};
  if (A.sigma != real(0)) td3_normal_pair<real>((uint32_t)j, (uint32_t)A.gen[0], h, 11u, A.k0, A.k1, z[0], z[1]);
  real* even = A.pop + (size_t)(2 * j) * E;
  real* odd = even + E;
  for (int c = 0; c < 2; c++) {
    const unsigned e = 2 * h + c;
    const real t = A.theta[e];
    const bool gap = A.sigma == real(0) || es_is_gap(A.lay, e);
    even[e] = gap ? t : actor_fma(A.sigma, z[c], t);
    odd[e] = gap ? t : actor_fma(-A.sigma, z[c], t);
  }
}

// ---- observe ----------------------------------------------------------------------------------------------------------------------------
template <typename real>
__global__ __launch_bounds__(ES_NT) void es_observe_kernel(long long B, double* fit, int32_t* len, uint8_t* alive, const real* rwd,
                                                           const uint8_t* done, const uint8_t* trunc) {
  const long long b = (long long)blockIdx.x * ES_NT + threadIdx.x;
  if (b >= B || alive[b] == 0) return;
  fit[b] += (double)rwd[b];
  len[b] += 1;
  if ((done[b] | trunc[b]) != 0) alive[b] = 0;
}

// ---- update -----------------------------------------------------------------------------------------------------------------------------
// the largest of the 256 lanes' values by the tree 128, 64, ... 1 (the shape of td3_tree)
__device__ __forceinline__ double es_tree_max(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int d = ES_NT / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] = sh[t + d] > sh[t] ? sh[t + d] : sh[t];
    __syncthreads();
  }
  return sh[0];
}

template <typename real>      // (a template only so that each unit instantiates its own)
__global__ __launch_bounds__(ES_NT) void es_fit_kernel(int M, long long R, const double* fit, double* member_fit) {
  const int p = blockIdx.x * ES_NT + threadIdx.x;
  if (p >= M) return;
  double s = 0.0;
  for (long long r = 0; r < R; r++) s += fit[(long long)p * R + r];
  const double F = s / (double)R;
  member_fit[p] = F != F ? -INFINITY : F;
}

// u_p from the counting rank; workgroup 0: the statistics over the members with F_p > -inf
template <typename real>
__global__ __launch_bounds__(ES_NT) void es_rank_kernel(int M, const double* member_fit, double* util, double* stats) {
  __shared__ double sh[ES_NT];
  __shared__ double Fq[ES_NT];
  const int t = threadIdx.x;
  const int p = blockIdx.x * ES_NT + t;
  const double Fp = p < M ? member_fit[p] : 0.0;
  int rank = 0;
  for (int q0 = 0; q0 < M; q0 += ES_NT) {
    __syncthreads();
    if (q0 + t < M) Fq[t] = member_fit[q0 + t];
    __syncthreads();
    const int nq = min(ES_NT, M - q0);
    for (int q = 0; q < nq; q++) {
      const double F = Fq[q];
      rank += (F < Fp || (F == Fp && q0 + q < p)) ? 1 : 0;
    }
  }
  if (p < M) util[p] = (double)rank / (double)(M - 1) - 0.5;
  if (blockIdx.x != 0) return;
  double s = 0.0, cnt = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int q = t; q < M; q += ES_NT) {
    const double F = member_fit[q];
    if (F > -INFINITY) {
      s += F; cnt += 1.0;
      mn = F < mn ? F : mn;
      mx = F > mx ? F : mx;
    }
  }
  const double n = td3_tree(cnt, sh);
  const double sum = td3_tree(s, sh);
  const double mean = n > 0.0 ? sum / n : 0.0;
  double d2 = 0.0;
  for (int q = t; q < M; q += ES_NT) {
    const double F = member_fit[q];
    if (F > -INFINITY) d2 += (F - mean) * (F - mean);
  }
  const double var = td3_tree(d2, sh);
  const double fmin = -es_tree_max(-mn, sh);
  const double fmax = es_tree_max(mx, sh);
  double first = -(double)M;                          // the lowest index of the maximum, as the largest negated index
  for (int q = t; q < M; q += ES_NT)
    if (member_fit[q] > -INFINITY && member_fit[q] == fmax && -(double)q > first) first = -(double)q;
  const double best = -es_tree_max(first, sh);
  if (t == 0) {
    const bool any = n > 0.0;
    stats[BCN_ES_STAT_FIT_MEAN] = mean;
    stats[BCN_ES_STAT_FIT_STD] = any ? sqrt(var / n) : 0.0;
    stats[BCN_ES_STAT_FIT_MIN] = any ? fmin : 0.0;
    stats[BCN_ES_STAT_FIT_MAX] = any ? fmax : 0.0;
    stats[BCN_ES_STAT_BEST_MEMBER] = any ? best : 0.0;
    stats[BCN_ES_STAT_NAN_MEMBERS] = (double)M - n;
    stats[BCN_ES_STAT_SPARE] = 0.0;
  }
}

template <typename real>
struct EsGradArgs {
  real* theta;
  const int32_t* gen;
  const double* util;
  double* partial;            // [chunks][E]
  real* grad;
  double* norm2;
  int M, chunks;
  double denom;               // M sigma
  real weight_decay;
  uint32_t k0, k1;
  EsLayout lay;
};

// blockIdx.y = the chunk; one lane per element pair h: both components of the pair of (j, gen[0], h, 11) for the chunk's pairs j
template <typename real>
__global__ __launch_bounds__(ES_NT) void es_partial_kernel(const EsGradArgs<real> A) {
  const unsigned E = A.lay.E, half = E >> 1;
  const unsigned h = blockIdx.x * ES_NT + threadIdx.x;
  if (h >= half) return;
  const int c = blockIdx.y;
  const int j0 = c * BCN_ES_PAIR_CHUNK, j1 = min(A.M / 2, j0 + BCN_ES_PAIR_CHUNK);
  const uint32_t gen = (uint32_t)A.gen[0];
  double s0 = 0.0, s1 = 0.0;
  for (int j = j0; j < j1; j++) {
    real z0, z1;
    td3_normal_pair<real>((uint32_t)j, gen, h, 11u, A.k0, A.k1, z0, z1);
    const double du = A.util[2 * j] - A.util[2 * j + 1];
    s0 += du * (double)z0;
    s1 += du * (double)z1;
  }
  A.partial[(size_t)c * E + 2 * h] = s0;
  A.partial[(size_t)c * E + 2 * h + 1] = s1;
}

template <typename real>
__global__ __launch_bounds__(ES_NT) void es_reduce_kernel(const EsGradArgs<real> A) {
  __shared__ double sh[ES_NT];
  const unsigned E = A.lay.E;
  const unsigned e = blockIdx.x * ES_NT + threadIdx.x;
  double sq = 0.0;
  if (e < E) {
    real gr = real(0);
    if (!es_is_gap(A.lay, e)) {
      double s = 0.0;
      for (int c = 0; c < A.chunks; c++) s += A.partial[(size_t)c * E + e];
      const real g = (real)(s / A.denom);
      gr = -(g) + A.weight_decay * A.theta[e];
    }
    A.grad[e] = gr;
    sq = (double)gr * (double)gr;
  }
  const double q = td3_tree(sq, sh);
  if (threadIdx.x == 0) A.norm2[blockIdx.x] = q;
}

template <typename real>
__global__ void es_tick_kernel(int32_t* gen) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    gen[0] = (int32_t)((uint32_t)gen[0] + 1u);
    gen[1] = gen[1] + 1;
  }
}

// ---- the launches: defined by es.hip (float) and es_f64.hip (double); hipError_t as int -------------------------------------------------
template <typename real>
inline size_t es_lds_bytes(int HP, int nmax, int G) {
  constexpr int LDK = EsGeom<real>::KS + 4;
  return sizeof(real) * ((size_t)2 * ES_TR * HP + (size_t)ES_TR * LDK + (size_t)G * nmax * LDK);
}

template <typename real>
struct EsUpdateArgs {
  int M;
  long long R;
  const double* fit;
  double *member_fit, *util, *stats;
  EsGradArgs<real> g;
  Td3AdamArgs<real> adam;
};

template <typename real> int es_launch_act(const EsActArgs<real>& a, int grid, void* stream);
template <typename real> int es_launch_begin(const EsBeginArgs<real>& a, void* stream);
template <typename real> int es_launch_observe(long long B, double* fit, int32_t* len, uint8_t* alive, const real* rwd, const uint8_t* done,
                                               const uint8_t* trunc, void* stream);
template <typename real> int es_launch_update(const EsUpdateArgs<real>& a, void* stream);

#define ES_CHECK_LAUNCH()                          \
  {                                                \
    const hipError_t e_ = hipGetLastError();       \
    if (e_ != hipSuccess) return (int)e_;          \
  }

#define ES_DEFINE_LAUNCH(real)                                                                                           \
  template <> int es_launch_act<real>(const EsActArgs<real>& a, int grid, void* stream) {                               \
    static size_t lds_allowed[64] = {0};                                                                                \
    const size_t lds = es_lds_bytes<real>(a.HP, a.nmax, a.G);                                                           \
    const hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(es_act_kernel<real>), lds, lds_allowed);        \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(es_act_kernel<real>, dim3(grid), dim3(ES_NT), lds, static_cast<hipStream_t>(stream), a);         \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int es_launch_begin<real>(const EsBeginArgs<real>& a, void* stream) {                                     \
    const long long pairs = (long long)(a.M / 2) * (a.lay.E >> 1);                                                      \
    const long long n = pairs > a.B ? pairs : a.B;                                                                      \
    hipLaunchKernelGGL(es_begin_kernel<real>, dim3((unsigned)((n + ES_NT - 1) / ES_NT)), dim3(ES_NT), 0,                \
                       static_cast<hipStream_t>(stream), a);                                                            \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int es_launch_observe<real>(long long B, double* fit, int32_t* len, uint8_t* alive, const real* rwd,      \
                                          const uint8_t* done, const uint8_t* trunc, void* stream) {                    \
    hipLaunchKernelGGL(es_observe_kernel<real>, dim3((unsigned)((B + ES_NT - 1) / ES_NT)), dim3(ES_NT), 0,              \
                       static_cast<hipStream_t>(stream), B, fit, len, alive, rwd, done, trunc);                         \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int es_launch_update<real>(const EsUpdateArgs<real>& a, void* stream) {                                   \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    const int mb = (a.M + ES_NT - 1) / ES_NT;                                                                           \
    const unsigned E = a.g.lay.E;                                                                                       \
    const int eb = (int)((E + ES_NT - 1) / ES_NT), hb = (int)(((E >> 1) + ES_NT - 1) / ES_NT);                          \
    hipLaunchKernelGGL(es_fit_kernel<real>, dim3(mb), dim3(ES_NT), 0, s, a.M, a.R, a.fit, a.member_fit);                \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(es_rank_kernel<real>, dim3(mb), dim3(ES_NT), 0, s, a.M, (const double*)a.member_fit, a.util,    \
                       a.stats);                                                                                        \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(es_partial_kernel<real>, dim3(hb, a.g.chunks), dim3(ES_NT), 0, s, a.g);                          \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(es_reduce_kernel<real>, dim3(eb), dim3(ES_NT), 0, s, a.g);                                       \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(td3_finish_kernel<real>, dim3(1), dim3(ES_NT), 0, s, (const double*)a.g.norm2, eb,               \
                       a.stats + BCN_ES_STAT_GRAD_NORM);                                                                \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(td3_adam_kernel<real>, dim3(eb), dim3(ES_NT), 0, s, a.adam);                                     \
    ES_CHECK_LAUNCH()                                                                                                   \
    hipLaunchKernelGGL(es_tick_kernel<real>, dim3(1), dim3(64), 0, s, a.adam.step);                                     \
    return (int)hipGetLastError();                                                                                      \
  }

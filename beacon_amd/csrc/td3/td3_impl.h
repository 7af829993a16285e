// td3_impl.h -- the kernels of libbeacon_td3.so (include/beacon_td3.h), templated on the real type and instantiated by td3.hip
// (float32) and td3_f64.hip (float64).
//
// Every network runs on the actor's tile with the actor's layer: the geometry, the staging, policy_layer in its forward and its
// transposed form and the walk policy_mlp are ../actor/policy_net.h, compiled into this library too and not changed by it; the
// Box-Muller and single-uniform forms are ../actor/actor_impl.h's.  What policy_net.h lacks is here:
//   td3_dw        dW[o][k] = sum_r D[o][r] X[k][r] over the tile's rows into the workgroup's slab (the form of the learner's)
//   td3_backward  the backward pass of one MLP from the gradient at its head
//   dQ/da         the gradient at the ACTION columns of a critic's first layer's input (td3_actor_kernel)
// A critic's input row [obs | a] is not one matrix in HBM, and the tile's [D][TBP] copy of it (139 KB at D = 512) does not fit LDS
// beside the activations: the launch in front (td3_next_kernel, td3_mu_kernel) writes the rows to the work buffer, and the critic
// stages them from there like observations.  Likewise mu's and Q_1's activations do not fit together: td3_actor_kernel keeps Q_1's,
// runs it backward down to dQ/da (16 registers per row), then runs mu forward AGAIN with its activations kept, then backward.
// LDS of the tile kernels: n_hidden activation buffers [hmax][TBP], xs [KS][TBP], ws [KS][wcols], head [16][TBP], the rows' sources
// int32 [TB] -- the learner's sum: 160 256 bytes in float32, 158 336 in float64 at the limits (3 x 128), of 163 840.
// No atomics, no inter-workgroup communication inside a launch.
#pragma once
#include "../actor/actor_impl.h"          // policy_net.h and env1d.h (bcn_philox4x32) come with it
#include "../../../include/beacon_td3.h"

#define TD3_NT ACTOR_NT

template <typename real>
struct Td3Args {
  const real* params;
  const real* target;
  int obs_dim, act_dim, D, n_hidden, hidden[BCN_ACTOR_MAX_LAYERS], activation, n_critics, hmax_pad, wcols;
  ActorNet mu, q[2];
  real low, high, center, half;
  // bcn_td3_act
  const real* obs;
  long long n_rows;
  const uint8_t* mask;
  uint32_t* counters;
  real* actions;
  int mode;
  real sigma;
  uint32_t seed_lo, seed_hi;
  long long replica_offset;
  // the replay memory
  const real *m_obs, *m_act, *m_rwd, *m_next;
  const uint8_t *m_boot, *m_live;
  long long capacity;
  // the minibatch
  const int32_t* idx;
  long long m, tiles;
  real gamma, sigma_t, c_noise;
  const int32_t* step;
  real *rw, *xa, *xb;
  real* slabs;
  size_t slab_elems;
  double* wg_stats;
};

// what policy_mlp reads of a kernel's argument block: one network's input rows and parameter buffer
template <typename real>
struct Td3View {
  const real* params;
  const real* obs;
  long long n_rows;
  int obs_dim, n_hidden, hidden[BCN_ACTOR_MAX_LAYERS], activation, wcols;
};

template <typename real>
__device__ __forceinline__ Td3View<real> td3_view(const Td3Args<real>& A, const real* params, const real* rows, long long n_rows, int in_dim) {
  Td3View<real> V;
  V.params = params; V.obs = rows; V.n_rows = n_rows; V.obs_dim = in_dim; V.n_hidden = A.n_hidden;
  for (int l = 0; l < BCN_ACTOR_MAX_LAYERS; l++) V.hidden[l] = A.hidden[l];
  V.activation = A.activation; V.wcols = A.wcols;
  return V;
}

template <typename real>
struct Td3Lds {
  real *hbuf, *xs, *ws, *head;
  int* rowsrc;
  size_t hstride;
};

template <typename real>
__device__ __forceinline__ Td3Lds<real> td3_carve(unsigned char* lds, int n_hidden, int hmax_pad, int wcols) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  Td3Lds<real> L;
  L.hbuf = reinterpret_cast<real*>(lds);
  L.hstride = (size_t)hmax_pad * TBP;
  L.xs = L.hbuf + (size_t)n_hidden * L.hstride;         // [KS][TBP]
  L.ws = L.xs + (size_t)KS * TBP;                        // [KS][wcols]
  L.head = L.ws + (size_t)KS * wcols;                    // [BCN_ACTOR_MAX_ACT][TBP]
  L.rowsrc = reinterpret_cast<int*>(L.head + (size_t)BCN_ACTOR_MAX_ACT * TBP);      // [TB]
  return L;
}

template <typename real>
inline size_t td3_lds_bytes(int n_hidden, int hmax_pad, int wcols) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  return sizeof(real) * ((size_t)n_hidden * hmax_pad * TBP + (size_t)KS * TBP + (size_t)KS * wcols + (size_t)BCN_ACTOR_MAX_ACT * TBP) + sizeof(int) * TB;
}

// the standard normal pair of the header from the four words at one counter
template <typename real>
__device__ __forceinline__ void td3_normal_pair(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, real& z0, real& z1) {
  uint32_t w[4];
  bcn_philox4x32(c0, c1, c2, c3, k0, k1, w);
  real ln_u1, two_u2, s, c;
  actor_bm_uniforms(w, ln_u1, two_u2);
  const real radius = sqrt(real(-2) * ln_u1);
  actor_sincospi(two_u2, &s, &c);
  z0 = radius * c;
  z1 = radius * s;
}

template <typename real>
__device__ __forceinline__ real td3_clamp(real x, real lo, real hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the sources of the tile's rows: idx[row] where it names a live row of the memory, else -1 (staged as zeros)
template <typename real>
__device__ __forceinline__ void td3_rowsrc(const Td3Args<real>& A, long long row0, int* rowsrc) {
  constexpr int TB = ActorGeom<real>::TB;
  const int r = threadIdx.x;
  if (r < TB) {
    int src = -1;
    if (row0 + r < A.m) {
      const long long s = A.idx[row0 + r];
      if (s >= 0 && s < A.capacity && A.m_live[s] != 0) src = (int)s;
    }
    rowsrc[r] = src;
  }
}

// ---- acting ----------------------------------------------------------------------------------------------------------------------
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_act_kernel(const Td3Args<real> A) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char td3_lds[];
  const Td3Lds<real> L = td3_carve<real>(td3_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  if (A.mode != BCN_TD3_UNIFORM) {
    const Td3View<real> V = td3_view(A, A.params, A.obs, A.n_rows, A.obs_dim);
    policy_mlp<real, false>(V, A.mu, A.act_dim, row0, nullptr, out_of, L.xs, L.ws, L.head);
  }
  __syncthreads();
  const int r = threadIdx.x;
  const long long b = row0 + r;
  if (r >= TB || b >= A.n_rows) return;
  if (A.mask && A.mask[b] == 0) return;
  const int n = A.act_dim;
  const uint32_t ctr = A.counters[b];
  const uint32_t gb = (uint32_t)(unsigned long long)(A.replica_offset + b);
  real* out = A.actions + b * n;
  if (A.mode == BCN_TD3_UNIFORM) {
    for (int j = 0; j < n; j++) {
      uint32_t w[4];
      bcn_philox4x32(gb, ctr, (uint32_t)j, 4u, A.seed_lo, A.seed_hi, w);
      out[j] = A.low + (A.high - A.low) * actor_single_uniform(w, real(0));
    }
  } else {
    const real hs = A.half * A.sigma;
    for (int j = 0; 2 * j < n; j++) {
      real z0 = real(0), z1 = real(0);
      if (A.mode == BCN_TD3_NOISY) td3_normal_pair<real>(gb, ctr, (uint32_t)j, 4u, A.seed_lo, A.seed_hi, z0, z1);
      for (int h = 0; h < 2 && 2 * j + h < n; h++) {
        const int i = 2 * j + h;
        const real mu = A.center + A.half * actor_tanh(L.head[i * TBP + r]);
        out[i] = A.mode == BCN_TD3_NOISY ? td3_clamp<real>(mu + hs * (h ? z1 : z0), A.low, A.high) : mu;
      }
    }
  }
  if (A.mode != BCN_TD3_DETERMINISTIC) A.counters[b] = ctr + 1u;
}

// ---- the replay memory -----------------------------------------------------------------------------------------------------------
template <typename real>
struct ReplayArgs {
  int32_t* head;
  real *obs, *act, *rwd, *next;
  uint8_t *boot, *live;
  long long C;
  int T, B, od, ad;
  const real *r_obs, *r_act, *r_rwd, *r_final;
  const uint8_t *r_done, *r_trunc, *r_valid;
  const int32_t* cursor;
};

__device__ __forceinline__ long long replay_steps(const int32_t* cursor, int T) {
  const int c = cursor[0];
  return c < 0 ? 0 : (c > T ? T : c);
}

// one lane per (transition, column k < max(od, ad)): the copy; nothing here writes head
template <typename real>
__global__ __launch_bounds__(TD3_NT) void replay_append_kernel(const ReplayArgs<real> A) {
  const int wc = A.od > A.ad ? A.od : A.ad;
  const long long e = (long long)blockIdx.x * TD3_NT + threadIdx.x;
  const long long tb = e / wc;
  const int k = (int)(e - tb * wc);
  if (tb >= (long long)A.T * A.B) return;
  if (tb / A.B >= replay_steps(A.cursor, A.T)) return;
  long long h0 = A.head[0] % A.C;
  if (h0 < 0) h0 += A.C;
  const long long slot = (h0 + tb) % A.C;
  const bool fin = (A.r_done[tb] | A.r_trunc[tb]) != 0;
  if (k < A.od) {
    A.obs[slot * A.od + k] = A.r_obs[tb * A.od + k];
    A.next[slot * A.od + k] = fin ? A.r_final[tb * A.od + k] : A.r_obs[(tb + A.B) * A.od + k];
  }
  if (k < A.ad) A.act[slot * A.ad + k] = A.r_act[tb * A.ad + k];
  if (k == 0) {
    A.rwd[slot] = A.r_rwd[tb];
    A.boot[slot] = (!fin || A.r_trunc[tb] != 0) ? 1 : 0;
    A.live[slot] = A.r_valid[tb] != 0 ? 1 : 0;
  }
}

template <typename real>
__global__ void replay_advance_kernel(int32_t* head, const int32_t* cursor, int T, int B, long long C) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const long long add = replay_steps(cursor, T) * B;       // <= C
    long long h0 = head[0] % C;
    if (h0 < 0) h0 += C;
    head[0] = (int32_t)((h0 + add) % C);
    const long long st = (long long)head[1] + add;
    head[1] = (int32_t)(st > C ? C : st);
    head[2] = (int32_t)((uint32_t)head[2] + (uint32_t)add);
  }
}

template <typename real>      // (templates only so that each unit instantiates its own)
__global__ __launch_bounds__(TD3_NT) void replay_sample_kernel(long long m, uint32_t k0, uint32_t k1, const int32_t* head, int32_t* idx) {
  const long long i = (long long)blockIdx.x * TD3_NT + threadIdx.x;
  if (i >= m) return;
  const uint32_t stored = head[1] > 1 ? (uint32_t)head[1] : 1u;
  uint32_t w[4];
  bcn_philox4x32((uint32_t)i, (uint32_t)head[3], 0u, 5u, k0, k1, w);
  idx[i] = (int32_t)(((unsigned long long)w[0] * (unsigned long long)stored) >> 32);
}

template <typename real>
__global__ void replay_sample_tick_kernel(int32_t* head) {
  if (threadIdx.x == 0 && blockIdx.x == 0) head[3] = (int32_t)((uint32_t)head[3] + 1u);
}

// ---- the slabs ---------------------------------------------------------------------------------------------------------------------
// dW[o][k0 + k] (+)= sum_r D[o][r] X[k][r] for o < OUT, k < ks, r ascending over the tile; with k0 = 0 also db[o] (+)= sum_r D[o][r].
// D, X: LDS, row stride TBP, complete (the caller synchronised).  gW: the workgroup's slab at the matrix [OUT][K], gB at the bias.
// `first`: the workgroup's first tile stores, the later ones add.  Lane = og * nkg + kg owns the outputs 4 og .. 4 og + 3 and, per
// chunk of 4 nkg columns, the columns 4 kg .. 4 kg + 3.
template <typename real>
__device__ __forceinline__ void td3_dw(const real* D, int OUT, const real* X, int ks, real* __restrict__ gW, real* __restrict__ gB, int K, int k0,
                                       bool first) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const int lane = threadIdx.x;
  const int out4 = (OUT + 3) & ~3;
  int nog = 1;
  while (nog * 4 < out4) nog <<= 1;
  const int nkg = TD3_NT / nog;
  const int og = lane / nkg, kg = lane - og * nkg;
  const int o0 = og * 4;
  if (o0 < OUT) {
    for (int kb = kg * 4; kb < ks; kb += nkg * 4) {
      real acc[4][4];                               // [output][column]
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[j][i] = real(0);
#pragma unroll 2
      for (int r = 0; r < TB; r += 4) {
        ActorV4<real> d[4], x[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (o0 + j < OUT) d[j] = *reinterpret_cast<const ActorV4<real>*>(D + (o0 + j) * TBP + r);
          else d[j] = ActorV4<real>{{real(0), real(0), real(0), real(0)}};
          if (kb + j < ks) x[j] = *reinterpret_cast<const ActorV4<real>*>(X + (kb + j) * TBP + r);
          else x[j] = ActorV4<real>{{real(0), real(0), real(0), real(0)}};
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) acc[j][i] = actor_fma(d[j].v[c], x[i].v[c], acc[j][i]);
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (o0 + j < OUT && kb + i < ks) {
            real* at = gW + (size_t)(o0 + j) * K + k0 + kb + i;
            *at = first ? acc[j][i] : *at + acc[j][i];
          }
    }
  }
  if (k0 == 0 && lane < OUT) {
    real s = real(0);
    for (int r = 0; r < TB; r++) s += D[lane * TBP + r];
    gB[lane] = first ? s : gB[lane] + s;
  }
}

// Backward pass of one MLP: `head` holds the gradient at the head's outputs, the activation buffers the forward pass's outputs.
// The first layer's input is staged again from V.obs: GATHER = false the rows from row0 on (up to V.n_rows), true the rows of rowsrc.
template <typename real, bool GATHER>
__device__ __forceinline__ void td3_backward(const Td3View<real>& V, const ActorNet& net, int n_head, long long row0, const int* rowsrc,
                                             const Td3Lds<real>& L, real* slab, bool first) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  for (int l = V.n_hidden; l >= 0; l--) {
    const real* D = l == V.n_hidden ? L.head : L.hbuf + l * L.hstride;
    const int OUT = l == V.n_hidden ? n_head : V.hidden[l];
    __syncthreads();                                // D is complete
    if (l > 0) {
      const int K = V.hidden[l - 1];
      real* X = L.hbuf + (l - 1) * L.hstride;
      td3_dw<real>(D, OUT, X, K, slab + net.w[l], slab + net.b[l], K, 0, first);
      // the gradient at this layer's input, in place over X (policy_layer synchronises before it writes anything; the transposed
      // form is instantiated as the learner instantiates it: no bias, xin given, so neither gather nor rows are touched)
      policy_layer<real, true, true>(V.params + net.w[l], nullptr, OUT, K, V.activation, D, V.obs, 0, 0, rowsrc, L.xs, L.ws, V.wcols, X);
    } else {
      const int K = V.obs_dim;
      for (int k0 = 0; k0 < K; k0 += KS) {
        const int ks = min(KS, K - k0);
        if (k0) __syncthreads();                    // the previous slab's readers of xs are done
        if constexpr (GATHER) actor_stage<real, true>(V.obs, K, k0, ks, TB, 0, rowsrc, L.xs, TBP);
        else actor_stage<real, false>(V.obs + (size_t)row0 * K, K, k0, ks, TB, (int)min((long long)TB, V.n_rows - row0), nullptr, L.xs, TBP);
        __syncthreads();
        td3_dw<real>(D, OUT, L.xs, ks, slab + net.w[0], slab + net.b[0], K, k0, first);
      }
    }
  }
}

// the workgroup's sums of `n` per-row terms staged in xs rows 0 .. n - 1, added in float64 for r ascending by lane s < n
template <typename real>
__device__ __forceinline__ void td3_tile_stats(const real* xs, int n, double& st) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const int r = threadIdx.x;
  if (r < n)
    for (int q = 0; q < TB; q++) st += (double)xs[r * TBP + q];
}

// ---- the critic step -----------------------------------------------------------------------------------------------------------
// launch 1: a' per row, and the minibatch's rows [s | a], [s' | a'], (rwd, boot, w) into the work buffer.  One workgroup per tile.
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_next_kernel(const Td3Args<real> A) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char td3_lds[];
  const Td3Lds<real> L = td3_carve<real>(td3_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  td3_rowsrc(A, row0, L.rowsrc);
  const Td3View<real> V = td3_view(A, A.target, A.m_next, 0, A.obs_dim);
  policy_mlp<real, true>(V, A.mu, A.act_dim, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
  __syncthreads();
  const int r = threadIdx.x, n = A.act_dim, od = A.obs_dim, D = A.D;
  const long long row = row0 + r;
  if (r < TB && row < A.m) {
    const int src = L.rowsrc[r];
    const uint32_t ctr = (uint32_t)A.step[2];
    for (int j = 0; 2 * j < n; j++) {
      real z0, z1;
      td3_normal_pair<real>((uint32_t)row, ctr, (uint32_t)j, 6u, A.seed_lo, A.seed_hi, z0, z1);
      for (int h = 0; h < 2 && 2 * j + h < n; h++) {
        const int i = 2 * j + h;
        real an = real(0), a = real(0);
        if (src >= 0) {
          const real mu = A.center + A.half * actor_tanh(L.head[i * TBP + r]);
          const real eps = td3_clamp<real>(A.sigma_t * (h ? z1 : z0), -A.c_noise, A.c_noise);
          an = td3_clamp<real>(mu + A.half * eps, A.low, A.high);
          a = A.m_act[(size_t)src * n + i];
        }
        A.xb[(size_t)row * D + od + i] = an;
        A.xa[(size_t)row * D + od + i] = a;
      }
    }
    A.rw[row] = src >= 0 ? A.m_rwd[src] : real(0);
    A.rw[A.m + row] = src >= 0 && A.m_boot[src] != 0 ? real(1) : real(0);
    A.rw[2 * A.m + row] = src >= 0 ? real(1) : real(0);
  }
  for (int e = threadIdx.x; e < TB * od; e += TD3_NT) {
    const int q = e / od, k = e - q * od;
    if (row0 + q >= A.m) break;
    const int src = L.rowsrc[q];
    A.xa[(size_t)(row0 + q) * D + k] = src >= 0 ? A.m_obs[(size_t)src * od + k] : real(0);
    A.xb[(size_t)(row0 + q) * D + k] = src >= 0 ? A.m_next[(size_t)src * od + k] : real(0);
  }
}

// launch 2: y, the critics' losses and their gradients into the workgroup's slab
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_critic_kernel(const Td3Args<real> A) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char td3_lds[];
  const Td3Lds<real> L = td3_carve<real>(td3_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x;
  double st = 0.0;                                    // lane s < 5: the workgroup's sum of term s
  bool first = true;
  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB, row = row0 + r;
    const bool own = r < TB && row < A.m;
    __syncthreads();                                  // the previous tile's readers of xs are done
    const real w = own ? A.rw[2 * A.m + row] : real(0);
    // ---- y ----
    real qmin = real(0);
    const Td3View<real> Vt = td3_view(A, A.target, A.xb, A.m, A.D);
    for (int i = 0; i < A.n_critics; i++) {
      policy_mlp<real, false>(Vt, A.q[i], 1, row0, nullptr, out_of, L.xs, L.ws, L.head);
      __syncthreads();
      if (r < TB) {
        const real q = L.head[r];
        qmin = i == 0 ? q : (q < qmin ? q : qmin);
      }
    }
    const real y = own ? A.rw[row] + (A.gamma * A.rw[A.m + row]) * qmin : real(0);
    // ---- the critics ----
    real t_loss = real(0), t_q[2] = {real(0), real(0)};
    const Td3View<real> V = td3_view(A, A.params, A.xa, A.m, A.D);
    for (int i = 0; i < A.n_critics; i++) {
      policy_mlp<real, false>(V, A.q[i], 1, row0, nullptr, out_of, L.xs, L.ws, L.head);
      __syncthreads();
      if (r < TB) {
        const real q = L.head[r], err = q - y;
        t_loss += w * (err * err);
        t_q[i] = w * q;
        L.head[r] = w * (real(2) * err);
      }
      td3_backward<real, false>(V, A.q[i], 1, row0, nullptr, L, slab, first);
    }
    __syncthreads();
    if (r < TB) {
      L.xs[0 * TBP + r] = t_loss; L.xs[1 * TBP + r] = t_q[0]; L.xs[2 * TBP + r] = t_q[1];
      L.xs[3 * TBP + r] = w * y; L.xs[4 * TBP + r] = w;
    }
    __syncthreads();
    td3_tile_stats<real>(L.xs, 5, st);
  }
  if (r < BCN_TD3_N_STATS) {
    // slots: 0 loss, 1 q1, 2 q2, 3 y, 5 w
    const int slot = r < 4 ? r : (r == 4 ? 5 : (r == 5 ? 4 : r));
    A.wg_stats[(size_t)blockIdx.x * BCN_TD3_N_STATS + slot] = r < 5 ? st : 0.0;
  }
}

// ---- the policy step -----------------------------------------------------------------------------------------------------------
// launch 1: the rows [s | mu(s)] into xb.  One workgroup per tile.
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_mu_kernel(const Td3Args<real> A) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char td3_lds[];
  const Td3Lds<real> L = td3_carve<real>(td3_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  td3_rowsrc(A, row0, L.rowsrc);
  const Td3View<real> V = td3_view(A, A.params, A.m_obs, 0, A.obs_dim);
  policy_mlp<real, true>(V, A.mu, A.act_dim, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
  __syncthreads();
  const int n = A.act_dim, od = A.obs_dim, D = A.D;
  for (int e = threadIdx.x; e < TB * D; e += TD3_NT) {
    const int q = e / D, k = e - q * D;
    if (row0 + q >= A.m) break;
    const int src = L.rowsrc[q];
    real v = real(0);
    if (src >= 0) v = k < od ? A.m_obs[(size_t)src * od + k] : A.center + A.half * actor_tanh(L.head[(k - od) * TBP + q]);
    A.xb[(size_t)(row0 + q) * D + k] = v;
  }
  (void)n;
}

// launch 2: -sum w Q_1(s, mu(s)) and its gradient down Q_1's action columns and down mu into the workgroup's slab
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_actor_kernel(const Td3Args<real> A) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char td3_lds[];
  const Td3Lds<real> L = td3_carve<real>(td3_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x, n = A.act_dim, od = A.obs_dim, D = A.D;
  double st = 0.0;                                    // lane 4: the sum of -w Q_1, lane 5: of w
  bool first = true;
  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB, row = row0 + r;
    const bool own = r < TB && row < A.m;
    __syncthreads();                                  // the previous tile's readers of xs and rowsrc are done
    td3_rowsrc(A, row0, L.rowsrc);
    const real w = own ? A.rw[2 * A.m + row] : real(0);
    // ---- Q_1 forward, its activations kept; backward to the first layer's pre-activation, no dW ----
    const Td3View<real> Vq = td3_view(A, A.params, A.xb, A.m, D);
    policy_mlp<real, false>(Vq, A.q[0], 1, row0, nullptr, out_of, L.xs, L.ws, L.head);
    __syncthreads();
    real t_pl = real(0);
    if (r < TB) {
      t_pl = -(w * L.head[r]);
      L.head[r] = -w;
    }
    for (int l = A.n_hidden; l >= 1; l--) {
      const real* Dg = l == A.n_hidden ? L.head : hbuf + l * hstride;
      const int OUT = l == A.n_hidden ? 1 : A.hidden[l];
      __syncthreads();                                // Dg is complete
      policy_layer<real, true, true>(A.params + A.q[0].w[l], nullptr, OUT, A.hidden[l - 1], A.activation, Dg, A.xb, 0, 0, L.rowsrc, L.xs,
                                     L.ws, A.wcols, hbuf + (l - 1) * hstride);
    }
    __syncthreads();                                  // g0 = hbuf[0] is complete
    // ---- dQ/da_j[r] = sum_q W0[q][od + j] g0[q][r], q ascending: into xs, then 16 registers of the row's lane ----
    {
      const real* W0 = A.params + A.q[0].w[0];
      const int d1 = A.hidden[0];
      for (int e = r; e < n * TB; e += TD3_NT) {
        const int j = e / TB, q = e - j * TB;
        real acc = real(0);
        for (int o = 0; o < d1; o++) acc = actor_fma(W0[(size_t)o * D + od + j], hbuf[o * TBP + q], acc);
        L.xs[j * TBP + q] = acc;
      }
    }
    __syncthreads();
    real da[BCN_ACTOR_MAX_ACT];
#pragma unroll
    for (int j = 0; j < BCN_ACTOR_MAX_ACT; j++) da[j] = (r < TB && j < n) ? L.xs[j * TBP + r] : real(0);
    // ---- mu forward again, its activations kept; backward ----
    const Td3View<real> Vm = td3_view(A, A.params, A.m_obs, 0, od);
    policy_mlp<real, true>(Vm, A.mu, n, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
    __syncthreads();
    if (r < TB) {
#pragma unroll
      for (int j = 0; j < BCN_ACTOR_MAX_ACT; j++)
        if (j < n) {
          const real t = actor_tanh(L.head[j * TBP + r]);
          L.head[j * TBP + r] = da[j] * (A.half * (real(1) - t * t));
        }
    }
    td3_backward<real, true>(Vm, A.mu, n, 0, L.rowsrc, L, slab, first);
    __syncthreads();
    if (r < TB) {
#pragma unroll
      for (int s = 0; s < 4; s++) L.xs[s * TBP + r] = real(0);
      L.xs[4 * TBP + r] = t_pl;
      L.xs[5 * TBP + r] = w;
    }
    __syncthreads();
    td3_tile_stats<real>(L.xs, 6, st);
  }
  // slots: 4 the policy loss, 5 w
  if (r < BCN_TD3_N_STATS) A.wg_stats[(size_t)blockIdx.x * BCN_TD3_N_STATS + r] = r == 4 || r == 5 ? st : 0.0;
}

// ---- reduce, norm, Adam, Polyak ------------------------------------------------------------------------------------------------
template <typename real>
struct Td3ReduceArgs {
  const real* slabs;
  size_t slab_elems;
  int used;                         // slabs written: the backward launch's workgroups
  const double* wg_stats;
  real* grad;
  int e0, e1;                       // the element range of the optimiser's segments
  double* norm2;                    // [blocks]
  double* stats;
  int which;
};

// the 256 lanes' values by the tree 128, 64, ... 1; the sum is in sh[0] behind the last barrier
__device__ __forceinline__ double td3_tree(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int d = TD3_NT / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  return sh[0];
}

// grad[p] = (sum_g slab_g[p]) / W for g ascending, p = e0 + block * 256 + lane; the block's part of the squared norm; block 0: the statistics
template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_reduce_kernel(const Td3ReduceArgs<real> A) {
  __shared__ double tot[BCN_TD3_N_STATS];
  __shared__ double sh[TD3_NT];
  const int t = threadIdx.x;
  if (t < BCN_TD3_N_STATS) {
    double s = 0.0;
    for (int g = 0; g < A.used; g++) s += A.wg_stats[(size_t)g * BCN_TD3_N_STATS + t];
    tot[t] = s;
  }
  __syncthreads();
  const double W = tot[BCN_TD3_STAT_W] > 1.0 ? tot[BCN_TD3_STAT_W] : 1.0;
  const int p = A.e0 + blockIdx.x * TD3_NT + t;
  double sq = 0.0;
  if (p < A.e1) {
    double s = 0.0;
    for (int g = 0; g < A.used; g++) s += (double)A.slabs[(size_t)g * A.slab_elems + p];
    const real gr = (real)(s / W);
    A.grad[p] = gr;
    sq = (double)gr * (double)gr;
  }
  const double q = td3_tree(sq, sh);
  if (t == 0) {
    A.norm2[blockIdx.x] = q;
    if (blockIdx.x == 0) {
      if (A.which == BCN_TD3_OPT_CRITIC) {
        A.stats[BCN_TD3_STAT_CRITIC_LOSS] = tot[0] / W;
        A.stats[BCN_TD3_STAT_Q1] = tot[1] / W;
        A.stats[BCN_TD3_STAT_Q2] = tot[2] / W;
        A.stats[BCN_TD3_STAT_TARGET] = tot[3] / W;
      } else {
        A.stats[BCN_TD3_STAT_POLICY_LOSS] = tot[4] / W;
      }
      A.stats[BCN_TD3_STAT_W] = W;
    }
  }
}

template <typename real>      // (a template only so that each unit instantiates its own)
__global__ __launch_bounds__(TD3_NT) void td3_finish_kernel(const double* norm2, int n_blocks, double* out) {
  __shared__ double sh[TD3_NT];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n_blocks; i += TD3_NT) s += norm2[i];
  const double q = td3_tree(s, sh);
  if (t == 0) out[0] = sqrt(q);
}

template <typename real>
struct Td3AdamArgs {
  real* params;
  const real* grad;
  real *m, *v;
  int32_t* step;
  const double* norm;
  int e0, e1, which;
  double lr, beta1, beta2, eps, max_grad_norm;
};

template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_adam_kernel(const Td3AdamArgs<real> A) {
  const int p = A.e0 + blockIdx.x * TD3_NT + threadIdx.x;
  if (p >= A.e1) return;
  double scale = 1.0;
  if (A.max_grad_norm > 0.0) {
    scale = A.max_grad_norm / (A.norm[0] + 1e-6);
    scale = scale < 1.0 ? scale : 1.0;
  }
  const double t = (double)(A.step[A.which] + 1);
  const real step_size = (real)(A.lr / (1.0 - pow(A.beta1, t)));
  const real bc2_sqrt = (real)sqrt(1.0 - pow(A.beta2, t));
  const real g = A.grad[p] * (real)scale;
  real m = A.m[p], v = A.v[p];
  m = m + (real)(1.0 - A.beta1) * (g - m);
  v = (real)A.beta2 * v + (real)(1.0 - A.beta2) * (g * g);
  A.m[p] = m;
  A.v[p] = v;
  const real denom = actor_sqrt(v) / bc2_sqrt + (real)A.eps;
  A.params[p] = A.params[p] - step_size * (m / denom);
}

template <typename real>
__global__ void td3_tick_kernel(int32_t* step, int which) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    step[which] = step[which] + 1;
    if (which == BCN_TD3_OPT_CRITIC) step[2] = (int32_t)((uint32_t)step[2] + 1u);
  }
}

template <typename real>
__global__ __launch_bounds__(TD3_NT) void td3_polyak_kernel(const real* __restrict__ params, real* __restrict__ target, int n, real tau) {
  const int p = blockIdx.x * TD3_NT + threadIdx.x;
  if (p < n) {
    const real t = target[p];
    target[p] = t + tau * (params[p] - t);
  }
}

// ---- the launches: defined by td3.hip (float) and td3_f64.hip (double); hipError_t as int ------------------------------------------
enum { TD3_K_ACT = 0, TD3_K_NEXT = 1, TD3_K_CRITIC = 2, TD3_K_MU = 3, TD3_K_ACTOR = 4 };
template <typename real> int td3_launch_tile(int kernel, const Td3Args<real>& a, int grid, void* stream);
template <typename real> int td3_launch_reduce(const Td3ReduceArgs<real>& r, int blocks, double* norm_out, void* stream);
template <typename real> int td3_launch_adam(const Td3AdamArgs<real>& a, void* stream);
template <typename real> int td3_launch_polyak(const real* params, real* target, int n, real tau, void* stream);
template <typename real> int td3_launch_append(const ReplayArgs<real>& a, void* stream);

#define TD3_DEFINE_LAUNCH(real)                                                                                          \
  template <> int td3_launch_tile<real>(int kernel, const Td3Args<real>& a, int grid, void* stream) {                   \
    typedef void (*kern_t)(const Td3Args<real>);                                                                        \
    static const kern_t table[5] = {td3_act_kernel<real>, td3_next_kernel<real>, td3_critic_kernel<real>,               \
                                    td3_mu_kernel<real>, td3_actor_kernel<real>};                                       \
    static size_t lds_allowed[5][64] = {{0}};                                                                           \
    const size_t lds = td3_lds_bytes<real>(a.n_hidden, a.hmax_pad, a.wcols);                                            \
    const hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(table[kernel]), lds, lds_allowed[kernel]);      \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(table[kernel], dim3(grid), dim3(TD3_NT), lds, static_cast<hipStream_t>(stream), a);              \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int td3_launch_reduce<real>(const Td3ReduceArgs<real>& r, int blocks, double* norm_out, void* stream) {   \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(td3_reduce_kernel<real>, dim3(blocks), dim3(TD3_NT), 0, s, r);                                   \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(td3_finish_kernel<real>, dim3(1), dim3(TD3_NT), 0, s, (const double*)r.norm2, blocks, norm_out); \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int td3_launch_adam<real>(const Td3AdamArgs<real>& a, void* stream) {                                     \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(td3_adam_kernel<real>, dim3((a.e1 - a.e0 + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0, s, a);        \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(td3_tick_kernel<real>, dim3(1), dim3(64), 0, s, a.step, a.which);                                \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int td3_launch_polyak<real>(const real* params, real* target, int n, real tau, void* stream) {            \
    hipLaunchKernelGGL(td3_polyak_kernel<real>, dim3((n + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0,                       \
                       static_cast<hipStream_t>(stream), params, target, n, tau);                                       \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int td3_launch_append<real>(const ReplayArgs<real>& a, void* stream) {                                    \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    const long long wc = a.od > a.ad ? a.od : a.ad;                                                                     \
    const long long total = (long long)a.T * a.B * wc;                                                                  \
    hipLaunchKernelGGL(replay_append_kernel<real>, dim3((unsigned)((total + TD3_NT - 1) / TD3_NT)), dim3(TD3_NT), 0, s, a); \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(replay_advance_kernel<real>, dim3(1), dim3(64), 0, s, a.head, a.cursor, a.T, a.B, a.C);                \
    return (int)hipGetLastError();                                                                                      \
  }

// sac_impl.h -- the kernels of libbeacon_sac.so (include/beacon_sac.h), templated on the real type and instantiated by sac.hip
// (float32) and sac_f64.hip (float64).
//
// Every network runs on the actor's tile with the actor's layer (../actor/policy_net.h); the slabs, the backward pass of one MLP, the
// tile's sums, the tree and the Adam, Polyak and finish kernels are ../td3/td3_impl.h's templates, instantiated in this unit (that
// file is included, not changed; nothing of libbeacon_td3.so is linked).  What both lack is here:
//   sac_component  one action component of the squashed Gaussian: the draw, its action and its log-density term (the header's lp_j)
//   the 2 act_dim-row head, the per-row min of two critics' action gradients, the temperature's gradient
//
// Where the head lives.  The policy's head is ONE matrix [2 act_dim][h_last], up to 32 rows; the tile's head buffer has 16.  The
// head layer's input is an activation buffer in LDS, never staged rows, so policy_layer does not touch the staging buffer xs
// ([KS][TBP], KS = 64 / 32 rows) while it runs: the head's 2 act_dim <= 32 outputs are written INTO xs, mean rows 0 .. n - 1, raw
// log-std rows n .. 2n - 1, by one policy_layer call; the gradient at the head overwrites them in place and td3_backward reads its
// top layer's D from there (a Td3Lds whose `head` is xs).  By the time td3_backward stages the first layer's input into xs again, D is
// an activation buffer.  The 16-row head buffer keeps the critics' one-row heads.
// LDS of the tile kernels, the sum of td3_impl.h with wcols = pad4(max(hmax, 2 act_dim)) + 4:
//   n_hidden [hmax][TBP] + xs [KS][TBP] + ws [KS][wcols] + head [16][TBP] reals + rowsrc int32 [TB]
//   float32 (TB 64, KS 64, TBP 68) at 3 x 128, act_dim 16:  4 (26 112 + 4 352 + 8 448 + 1 088) + 256 = 160 256 bytes
//   float64 (TB 32, KS 32, TBP 36) at 3 x 128, act_dim 16:  8 (13 824 + 1 152 + 4 224 +   576) + 128 = 158 336 bytes
// of 163 840 (SAC_LDS_LIMIT): the 32-row head costs nothing beside TD3's sum, because 2 act_dim <= KS in both dtypes (asserted below).
// sac_cfg_ok (sac.hip) refuses a cfg whose sum exceeds the limit before any launch.
// No atomics, no inter-workgroup communication inside a launch.
#pragma once
#include "../td3/td3_impl.h"              // actor_impl.h, policy_net.h and env1d.h (bcn_philox4x32) come with it
#include "../../../include/beacon_sac.h"

#define SAC_LDS_LIMIT (160 * 1024)
static_assert(2 * BCN_ACTOR_MAX_ACT <= ActorGeom<float>::KS && 2 * BCN_ACTOR_MAX_ACT <= ActorGeom<double>::KS, "the head's rows live in xs");
static_assert(BCN_SAC_N_STATS <= TD3_NT, "one lane per statistic");

template <typename real>
struct SacArgs {
  Td3Args<real> t;            // the networks, the rows, the memory's segments, the work buffer: the fields of TD3's block (mu = pi)
  unsigned la;                // the element of log_alpha in the parameter buffer
  real ln_half;               // ln h, formed in float64 and rounded once
};

__device__ __forceinline__ float sac_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double sac_log1p(double x) { return log1p(x); }

template <typename real>
struct SacDraw {
  real a, lp, t, sdz;
  bool pass;                  // the clamp passes gradient: -20 <= raw <= 2
};

// one component: mean m, raw log-std, standard normal z (the header's formulas, in its order)
template <typename real>
__device__ __forceinline__ SacDraw<real> sac_component(real m, real raw, real z, real center, real half, real ln_half) {
  SacDraw<real> d;
  d.pass = raw >= real(-20) && raw <= real(2);
  const real ls = td3_clamp<real>(raw, real(-20), real(2));
  const real sd = actor_exp(ls);
  d.sdz = sd * z;
  const real u = m + d.sdz;
  d.t = actor_tanh(u);
  d.a = center + half * d.t;
  const real x = real(-2) * u;
  const real sp = (x > real(0) ? x : real(0)) + sac_log1p(actor_exp(-actor_abs(x)));      // softplus(-2u)
  const real gauss = ((real(-0.5) * z * z - ls) - real(0.91893853320467274178)) - ln_half;
  d.lp = gauss - real(2) * ((real(0.69314718055994530942) - u) - sp);
  return d;
}

template <typename real>
__device__ __forceinline__ Td3Lds<real> sac_head_in_xs(const Td3Lds<real>& L) {
  Td3Lds<real> H = L;
  H.head = L.xs;
  return H;
}

// ---- acting ----------------------------------------------------------------------------------------------------------------------
template <typename real>
__global__ __launch_bounds__(TD3_NT) void sac_act_kernel(const SacArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char sac_lds[];
  const Td3Lds<real> L = td3_carve<real>(sac_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  const int n = A.act_dim;
  if (A.mode != BCN_SAC_UNIFORM) {
    const Td3View<real> V = td3_view(A, A.params, A.obs, A.n_rows, A.obs_dim);
    policy_mlp<real, false>(V, A.mu, 2 * n, row0, nullptr, out_of, L.xs, L.ws, L.xs);
  }
  __syncthreads();
  const int r = threadIdx.x;
  const long long b = row0 + r;
  if (r >= TB || b >= A.n_rows) return;
  if (A.mask && A.mask[b] == 0) return;
  const uint32_t ctr = A.counters[b];
  const uint32_t gb = (uint32_t)(unsigned long long)(A.replica_offset + b);
  real* out = A.actions + b * n;
  if (A.mode == BCN_SAC_UNIFORM) {
    for (int j = 0; j < n; j++) {
      uint32_t w[4];
      bcn_philox4x32(gb, ctr, (uint32_t)j, 7u, A.seed_lo, A.seed_hi, w);
      out[j] = A.low + (A.high - A.low) * actor_single_uniform(w, real(0));
    }
  } else if (A.mode == BCN_SAC_DETERMINISTIC) {
    for (int j = 0; j < n; j++) out[j] = A.center + A.half * actor_tanh(L.xs[j * TBP + r]);
  } else {
    for (int j = 0; 2 * j < n; j++) {
      real z0, z1;
      td3_normal_pair<real>(gb, ctr, (uint32_t)j, 7u, A.seed_lo, A.seed_hi, z0, z1);
      for (int h = 0; h < 2 && 2 * j + h < n; h++) {
        const int i = 2 * j + h;
        out[i] = sac_component<real>(L.xs[i * TBP + r], L.xs[(n + i) * TBP + r], h ? z1 : z0, A.center, A.half, S.ln_half).a;
      }
    }
  }
  if (A.mode != BCN_SAC_DETERMINISTIC) A.counters[b] = ctr + 1u;
}

// ---- launch 1 of both steps: a draw of the CURRENT policy per row, and the rows into the work buffer ---------------------------------
// NEXT = true   (critic step)  pi on s', stream 8 at step[3]: the rows [s' | a'] into xb, [s | a] into xa, (rwd, boot, w, log pi') into rw
// NEXT = false  (policy step)  pi on s,  stream 9 at step[4]: the rows [s | a~] into xb
// One workgroup per tile.
template <typename real, bool NEXT>
__global__ __launch_bounds__(TD3_NT) void sac_draw_kernel(const SacArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char sac_lds[];
  const Td3Lds<real> L = td3_carve<real>(sac_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  const int r = threadIdx.x, n = A.act_dim, od = A.obs_dim, D = A.D;
  td3_rowsrc(A, row0, L.rowsrc);
  const real* rows = NEXT ? A.m_next : A.m_obs;
  const Td3View<real> V = td3_view(A, A.params, rows, 0, od);
  policy_mlp<real, true>(V, A.mu, 2 * n, 0, L.rowsrc, out_of, L.xs, L.ws, L.xs);
  __syncthreads();
  const long long row = row0 + r;
  if (r < TB && row < A.m) {
    const int src = L.rowsrc[r];
    const uint32_t ctr = (uint32_t)A.step[NEXT ? 3 : 4];
    real lp = real(0);
    for (int j = 0; 2 * j < n; j++) {
      real z0, z1;
      td3_normal_pair<real>((uint32_t)row, ctr, (uint32_t)j, NEXT ? 8u : 9u, A.seed_lo, A.seed_hi, z0, z1);
      for (int h = 0; h < 2 && 2 * j + h < n; h++) {
        const int i = 2 * j + h;
        real an = real(0);
        if (src >= 0) {
          const SacDraw<real> d = sac_component<real>(L.xs[i * TBP + r], L.xs[(n + i) * TBP + r], h ? z1 : z0, A.center, A.half, S.ln_half);
          an = d.a;
          lp += d.lp;
        }
        A.xb[(size_t)row * D + od + i] = an;
        if constexpr (NEXT) A.xa[(size_t)row * D + od + i] = src >= 0 ? A.m_act[(size_t)src * n + i] : real(0);
      }
    }
    if constexpr (NEXT) {
      A.rw[row] = src >= 0 ? A.m_rwd[src] : real(0);
      A.rw[A.m + row] = src >= 0 && A.m_boot[src] != 0 ? real(1) : real(0);
      A.rw[2 * A.m + row] = src >= 0 ? real(1) : real(0);
      A.rw[3 * A.m + row] = lp;
    }
  }
  for (int e = threadIdx.x; e < TB * od; e += TD3_NT) {
    const int q = e / od, k = e - q * od;
    if (row0 + q >= A.m) break;
    const int src = L.rowsrc[q];
    A.xb[(size_t)(row0 + q) * D + k] = src >= 0 ? rows[(size_t)src * od + k] : real(0);
    if constexpr (NEXT) A.xa[(size_t)(row0 + q) * D + k] = src >= 0 ? A.m_obs[(size_t)src * od + k] : real(0);
  }
}

// ---- the critic step, launch 2: y, the critics' losses and their gradients into the workgroup's slab -----------------------------------
template <typename real>
__global__ __launch_bounds__(TD3_NT) void sac_critic_kernel(const SacArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char sac_lds[];
  const Td3Lds<real> L = td3_carve<real>(sac_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x;
  const real alpha = actor_exp(A.params[S.la]);
  double st = 0.0;                                    // lane s < 6: the workgroup's sum of term s
  bool first = true;
  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB, row = row0 + r;
    const bool own = r < TB && row < A.m;
    __syncthreads();                                  // the previous tile's readers of xs are done
    const real w = own ? A.rw[2 * A.m + row] : real(0);
    const real lpn = own ? A.rw[3 * A.m + row] : real(0);
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
    const real y = own ? A.rw[row] + (A.gamma * A.rw[A.m + row]) * (qmin - alpha * lpn) : real(0);
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
      L.xs[3 * TBP + r] = w * y; L.xs[4 * TBP + r] = w; L.xs[5 * TBP + r] = w * lpn;
    }
    __syncthreads();
    td3_tile_stats<real>(L.xs, 6, st);
  }
  if (r < BCN_SAC_N_STATS) {
    // lane s < 6 holds term s: loss, q1, q2, y to their slots, w to W, w log pi' to next_logp; the other lanes zero the other slots
    const int slot[BCN_SAC_N_STATS] = {0, 1, 2, 3, BCN_SAC_STAT_W, BCN_SAC_STAT_NEXT_LOGP, 4, 6, 7, 8, 10, 11};
    A.wg_stats[(size_t)blockIdx.x * BCN_SAC_N_STATS + slot[r]] = r < 6 ? st : 0.0;
  }
}

// ---- the policy step, launch 2 -------------------------------------------------------------------------------------------------------
// sum w (alpha log pi - Q_min) and its gradient: down each critic to its action columns (no dW), the smaller Q's kept in 16 registers
// of the row's lane, then down pi from both halves of the head into the workgroup's slab
template <typename real>
__global__ __launch_bounds__(TD3_NT) void sac_actor_kernel(const SacArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char sac_lds[];
  const Td3Lds<real> L = td3_carve<real>(sac_lds, A.n_hidden, A.hmax_pad, A.wcols);
  const Td3Lds<real> H = sac_head_in_xs(L);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x, n = A.act_dim, od = A.obs_dim, D = A.D;
  const real alpha = actor_exp(A.params[S.la]);
  const uint32_t ctr = (uint32_t)A.step[4];
  double st = 0.0;                                    // lane 0: the sum of w (alpha log pi - Q_min), lane 1: of w, lane 2: of w log pi
  bool first = true;
  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB, row = row0 + r;
    const bool own = r < TB && row < A.m;
    __syncthreads();                                  // the previous tile's readers of xs and rowsrc are done
    td3_rowsrc(A, row0, L.rowsrc);
    const real w = own ? A.rw[2 * A.m + row] : real(0);
    // ---- each critic forward, its activations kept; backward to the first layer's pre-activation, no dW; -w dQ/da ----
    real da[BCN_ACTOR_MAX_ACT];
#pragma unroll
    for (int j = 0; j < BCN_ACTOR_MAX_ACT; j++) da[j] = real(0);
    real qsel = real(0);
    const Td3View<real> Vq = td3_view(A, A.params, A.xb, A.m, D);
    for (int i = 0; i < A.n_critics; i++) {
      policy_mlp<real, false>(Vq, A.q[i], 1, row0, nullptr, out_of, L.xs, L.ws, L.head);
      __syncthreads();
      real qv = real(0);
      if (r < TB) {
        qv = L.head[r];
        L.head[r] = -w;
      }
      for (int l = A.n_hidden; l >= 1; l--) {
        const real* Dg = l == A.n_hidden ? L.head : hbuf + l * hstride;
        const int OUT = l == A.n_hidden ? 1 : A.hidden[l];
        __syncthreads();                              // Dg is complete
        policy_layer<real, true, true>(A.params + A.q[i].w[l], nullptr, OUT, A.hidden[l - 1], A.activation, Dg, A.xb, 0, 0, L.rowsrc, L.xs,
                                       L.ws, A.wcols, hbuf + (l - 1) * hstride);
      }
      __syncthreads();                                // g0 = hbuf[0] is complete
      {
        const real* W0 = A.params + A.q[i].w[0];
        const int d1 = A.hidden[0];
        for (int e = r; e < n * TB; e += TD3_NT) {
          const int j = e / TB, q = e - j * TB;
          real acc = real(0);
          for (int o = 0; o < d1; o++) acc = actor_fma(W0[(size_t)o * D + od + j], hbuf[o * TBP + q], acc);
          L.xs[j * TBP + q] = acc;
        }
      }
      __syncthreads();
      const bool take = i == 0 || qv < qsel;          // Q_2 only where it is strictly smaller
      if (take) qsel = qv;
#pragma unroll
      for (int j = 0; j < BCN_ACTOR_MAX_ACT; j++)
        if (r < TB && j < n && take) da[j] = L.xs[j * TBP + r];
    }
    // ---- pi forward again, its activations kept, the head in xs; the gradient at the head in place; backward ----
    const Td3View<real> Vm = td3_view(A, A.params, A.m_obs, 0, od);
    policy_mlp<real, true>(Vm, A.mu, 2 * n, 0, L.rowsrc, out_of, L.xs, L.ws, L.xs);
    __syncthreads();
    real t_pl = real(0), t_lp = real(0);
    if (r < TB) {
      const real wa = w * alpha;
      real lp = real(0);
      for (int j = 0; 2 * j < n; j++) {
        real z0, z1;
        td3_normal_pair<real>((uint32_t)row, ctr, (uint32_t)j, 9u, A.seed_lo, A.seed_hi, z0, z1);
        for (int h = 0; h < 2 && 2 * j + h < n; h++) {
          const int i = 2 * j + h;
          const SacDraw<real> d = sac_component<real>(L.xs[i * TBP + r], L.xs[(n + i) * TBP + r], h ? z1 : z0, A.center, A.half, S.ln_half);
          real dai = real(0);
#pragma unroll
          for (int k = 0; k < BCN_ACTOR_MAX_ACT; k++)
            if (k == i) dai = da[k];
          const real gu = dai * (A.half * (real(1) - d.t * d.t)) + wa * (real(2) * d.t);
          L.xs[i * TBP + r] = gu;
          L.xs[(n + i) * TBP + r] = d.pass ? gu * d.sdz - wa : real(0);
          lp += d.lp;
        }
      }
      t_pl = w * (alpha * lp - qsel);
      t_lp = w * lp;
    }
    td3_backward<real, true>(Vm, A.mu, 2 * n, 0, L.rowsrc, H, slab, first);
    __syncthreads();
    if (r < TB) {
      L.xs[0 * TBP + r] = t_pl;
      L.xs[1 * TBP + r] = w;
      L.xs[2 * TBP + r] = t_lp;
    }
    __syncthreads();
    td3_tile_stats<real>(L.xs, 3, st);
  }
  if (r < BCN_SAC_N_STATS) {
    const int slot[BCN_SAC_N_STATS] = {BCN_SAC_STAT_POLICY_LOSS, BCN_SAC_STAT_W, BCN_SAC_STAT_LOGP, 0, 1, 2, 3, 6, 7, 9, 10, 11};
    A.wg_stats[(size_t)blockIdx.x * BCN_SAC_N_STATS + slot[r]] = r < 3 ? st : 0.0;
  }
}

// ---- reduce --------------------------------------------------------------------------------------------------------------------------
template <typename real>
struct SacReduceArgs {
  Td3ReduceArgs<real> r;            // which: BCN_SAC_OPT_CRITIC or BCN_SAC_OPT_POLICY
  const real* params;
  int la;
  double target_entropy;
};

// grad[p] = (sum_g slab_g[p]) / W for g ascending, p = e0 + block * 256 + lane; the block's part of the squared norm; block 0: the
// statistics, and behind the policy step the temperature's gradient into grad[la]
template <typename real>
__global__ __launch_bounds__(TD3_NT) void sac_reduce_kernel(const SacReduceArgs<real> S) {
  const Td3ReduceArgs<real>& A = S.r;
  __shared__ double tot[BCN_SAC_N_STATS];
  __shared__ double sh[TD3_NT];
  const int t = threadIdx.x;
  if (t < BCN_SAC_N_STATS) {
    double s = 0.0;
    for (int g = 0; g < A.used; g++) s += A.wg_stats[(size_t)g * BCN_SAC_N_STATS + t];
    tot[t] = s;
  }
  __syncthreads();
  const double W = tot[BCN_SAC_STAT_W] > 1.0 ? tot[BCN_SAC_STAT_W] : 1.0;
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
      if (A.which == BCN_SAC_OPT_CRITIC) {
        A.stats[BCN_SAC_STAT_CRITIC_LOSS] = tot[BCN_SAC_STAT_CRITIC_LOSS] / W;
        A.stats[BCN_SAC_STAT_Q1] = tot[BCN_SAC_STAT_Q1] / W;
        A.stats[BCN_SAC_STAT_Q2] = tot[BCN_SAC_STAT_Q2] / W;
        A.stats[BCN_SAC_STAT_TARGET] = tot[BCN_SAC_STAT_TARGET] / W;
        A.stats[BCN_SAC_STAT_NEXT_LOGP] = tot[BCN_SAC_STAT_NEXT_LOGP] / W;
      } else {
        const double ag = -((tot[BCN_SAC_STAT_LOGP] + S.target_entropy * tot[BCN_SAC_STAT_W]) / W);
        A.stats[BCN_SAC_STAT_POLICY_LOSS] = tot[BCN_SAC_STAT_POLICY_LOSS] / W;
        A.stats[BCN_SAC_STAT_LOGP] = tot[BCN_SAC_STAT_LOGP] / W;
        A.stats[BCN_SAC_STAT_ALPHA_GRAD] = ag;
        A.grad[S.la] = (real)ag;
      }
      A.stats[BCN_SAC_STAT_ALPHA] = (double)actor_exp(S.params[S.la]);
      A.stats[BCN_SAC_STAT_W] = W;
    }
  }
}

template <typename real>
__global__ void sac_tick_kernel(int32_t* step, int which) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    step[which] = step[which] + 1;
    if (which == BCN_SAC_OPT_CRITIC) step[3] = (int32_t)((uint32_t)step[3] + 1u);
    if (which == BCN_SAC_OPT_POLICY) step[4] = (int32_t)((uint32_t)step[4] + 1u);
  }
}

// ---- the launches: defined by sac.hip (float) and sac_f64.hip (double); hipError_t as int ----------------------------------------------
enum { SAC_K_ACT = 0, SAC_K_NEXT = 1, SAC_K_CRITIC = 2, SAC_K_PI = 3, SAC_K_ACTOR = 4 };
template <typename real> int sac_launch_tile(int kernel, const SacArgs<real>& a, int grid, void* stream);
template <typename real> int sac_launch_reduce(const SacReduceArgs<real>& r, int blocks, double* norm_out, void* stream);
template <typename real> int sac_launch_adam(const Td3AdamArgs<real>& a, void* stream);
template <typename real> int sac_launch_polyak(const real* params, real* target, int n, real tau, void* stream);

#define SAC_DEFINE_LAUNCH(real)                                                                                          \
  template <> int sac_launch_tile<real>(int kernel, const SacArgs<real>& a, int grid, void* stream) {                   \
    typedef void (*kern_t)(const SacArgs<real>);                                                                        \
    static const kern_t table[5] = {sac_act_kernel<real>, sac_draw_kernel<real, true>, sac_critic_kernel<real>,         \
                                    sac_draw_kernel<real, false>, sac_actor_kernel<real>};                              \
    static size_t lds_allowed[5][64] = {{0}};                                                                           \
    const size_t lds = td3_lds_bytes<real>(a.t.n_hidden, a.t.hmax_pad, a.t.wcols);                                      \
    const hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(table[kernel]), lds, lds_allowed[kernel]);      \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(table[kernel], dim3(grid), dim3(TD3_NT), lds, static_cast<hipStream_t>(stream), a);              \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int sac_launch_reduce<real>(const SacReduceArgs<real>& r, int blocks, double* norm_out, void* stream) {   \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(sac_reduce_kernel<real>, dim3(blocks), dim3(TD3_NT), 0, s, r);                                   \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(td3_finish_kernel<real>, dim3(1), dim3(TD3_NT), 0, s, (const double*)r.r.norm2, blocks, norm_out); \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int sac_launch_adam<real>(const Td3AdamArgs<real>& a, void* stream) {                                     \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(td3_adam_kernel<real>, dim3((a.e1 - a.e0 + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0, s, a);        \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(sac_tick_kernel<real>, dim3(1), dim3(64), 0, s, a.step, a.which);                                \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int sac_launch_polyak<real>(const real* params, real* target, int n, real tau, void* stream) {            \
    hipLaunchKernelGGL(td3_polyak_kernel<real>, dim3((n + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0,                       \
                       static_cast<hipStream_t>(stream), params, target, n, tau);                                       \
    return (int)hipGetLastError();                                                                                      \
  }

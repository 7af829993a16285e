// dqn_impl.h -- the kernels of libbeacon_dqn.so (include/beacon_dqn.h), templated on the real type and instantiated by dqn.hip
// (float32) and dqn_f64.hip (float64).
//
// The network runs on the actor's tile with the actor's layer (../actor/policy_net.h); the carve of the LDS, the rows' sources, the
// slabs, the backward pass of one MLP, the tile's sums, the tree and the finish, Adam and ring-advance kernels are
// ../td3/td3_impl.h's templates, instantiated in this unit (that file is included, not changed; nothing of libbeacon_td3.so is
// linked).  What both lack is here:
//   dqn_values      Q_j of one row from the head's outputs in LDS (plain and dueling) and the first-maximum argmax
//   dqn_q_kernel    the whole gradient of one minibatch in ONE launch
//   dqn_act_kernel  the epsilon-greedy act launch with int32 actions; the same kernel writes the Q values for bcn_dqn_q
//   dqn_append_kernel  the ring's copy launch for int32 rollout actions (ReplayArgs::r_act is const real*)
//
// Why one launch where TD3 takes two.  A critic's input is [obs | a], no row of the memory, so TD3 writes the rows to the work buffer
// in a launch of its own.  Here the network's input IS a row of the memory: all three forward passes gather it through rowsrc, the
// per-row scalars (j*, y, w, rwd, boot) live in registers of the lanes r < TB, and the activation buffers are used by each forward
// pass in turn -- only the last one's are kept for the backward pass.
// LDS of the tile kernels, the sum of td3_impl.h with wcols = pad4(max(hmax, R)) + 4, R = n_actions + dueling <= 16:
//   n_hidden [hmax][TBP] + xs [KS][TBP] + ws [KS][wcols] + head [16][TBP] reals + rowsrc int32 [TB]
//   float32 (TB 64, KS 64, TBP 68) at 3 x 128:  4 (26 112 + 4 352 + 8 448 + 1 088) + 256 = 160 256 bytes
//   float64 (TB 32, KS 32, TBP 36) at 3 x 128:  8 (13 824 + 1 152 + 4 224 +   576) + 128 = 158 336 bytes
// of 163 840 (DQN_LDS_LIMIT).  dqn_cfg_ok (dqn.hip) refuses a cfg whose sum exceeds the limit before any launch.
// No atomics, no inter-workgroup communication inside a launch.
#pragma once
#include "../td3/td3_impl.h"              // actor_impl.h, policy_net.h and env1d.h (bcn_philox4x32) come with it
#include "../../../include/beacon_dqn.h"

#define DQN_LDS_LIMIT (160 * 1024)
static_assert(BCN_DQN_MAX_ACTIONS == BCN_ACTOR_MAX_ACT, "the head's rows live in the tile's head buffer");
static_assert(BCN_DQN_N_STATS <= TD3_NT, "one lane per statistic");

template <typename real>
struct DqnArgs {
  Td3Args<real> t;            // the network (mu = q), the rows, the memory's segments, the slabs: the fields of TD3's block; act_dim = n_actions
  int n_head;                 // n_actions + dueling
  int dueling, double_q;
  real inv_n;                 // 1 / n_actions, formed once
  real huber;                 // kappa, or <= 0
  real eps;
  const real* eps_dev;        // wins where it is not NULL
  int32_t* actions_i;         // bcn_dqn_act
  real* q_out;                // bcn_dqn_q: [n_rows][n_actions]; NULL in bcn_dqn_act
};

// Q_j of row r from the head's outputs ([n_head][TBP] in LDS)
template <typename real>
struct DqnRow {
  real v, mean;               // dueling: V and (sum_k A_k) / n
  bool dueling;
};

template <typename real>
__device__ __forceinline__ DqnRow<real> dqn_row(const real* head, int r, int n, bool dueling) {
  constexpr int TBP = ActorGeom<real>::TB + 4;
  DqnRow<real> R;
  R.dueling = dueling; R.v = real(0); R.mean = real(0);
  if (dueling) {
    real s = real(0);
    for (int k = 0; k < n; k++) s += head[k * TBP + r];
    R.mean = s / real(n);
    R.v = head[n * TBP + r];
  }
  return R;
}

template <typename real>
__device__ __forceinline__ real dqn_value(const DqnRow<real>& R, const real* head, int r, int j) {
  constexpr int TBP = ActorGeom<real>::TB + 4;
  const real h = head[j * TBP + r];
  return R.dueling ? (R.v + h) - R.mean : h;
}

// the first maximum: replaced only on strict >, so a NaN never wins
template <typename real>
__device__ __forceinline__ int dqn_argmax(const DqnRow<real>& R, const real* head, int r, int n) {
  real best = -INFINITY;
  int arg = 0;
  for (int j = 0; j < n; j++) {
    const real q = dqn_value(R, head, r, j);
    if (q > best) { best = q; arg = j; }
  }
  return arg;
}

// ---- acting, and the Q values of given rows -----------------------------------------------------------------------------------------
template <typename real>
__global__ __launch_bounds__(TD3_NT) void dqn_act_kernel(const DqnArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char dqn_lds[];
  const Td3Lds<real> L = td3_carve<real>(dqn_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  const long long row0 = (long long)blockIdx.x * TB;
  const int n = A.act_dim;
  if (A.mode != BCN_DQN_UNIFORM) {
    const Td3View<real> V = td3_view(A, A.params, A.obs, A.n_rows, A.obs_dim);
    policy_mlp<real, false>(V, A.mu, S.n_head, row0, nullptr, out_of, L.xs, L.ws, L.head);
  }
  __syncthreads();
  const int r = threadIdx.x;
  const long long b = row0 + r;
  if (r >= TB || b >= A.n_rows) return;
  if (S.q_out) {
    const DqnRow<real> R = dqn_row<real>(L.head, r, n, S.dueling != 0);
    for (int j = 0; j < n; j++) S.q_out[b * n + j] = dqn_value(R, L.head, r, j);
    return;
  }
  if (A.mask && A.mask[b] == 0) return;
  const uint32_t ctr = A.counters[b];
  int a = 0;
  if (A.mode != BCN_DQN_UNIFORM) a = dqn_argmax(dqn_row<real>(L.head, r, n, S.dueling != 0), L.head, r, n);
  if (A.mode != BCN_DQN_GREEDY) {
    const uint32_t gb = (uint32_t)(unsigned long long)(A.replica_offset + b);
    uint32_t w[4];
    bcn_philox4x32(gb, ctr, 0u, 10u, A.seed_lo, A.seed_hi, w);
    const int rnd = (int)(((unsigned long long)w[3] * (unsigned long long)n) >> 32);
    if (A.mode == BCN_DQN_UNIFORM) a = rnd;
    else {
      const real eps = S.eps_dev ? S.eps_dev[0] : S.eps;
      if (actor_single_uniform(w, real(0)) < eps) a = rnd;
    }
    A.counters[b] = ctr + 1u;
  }
  S.actions_i[b] = a;
}

// ---- the ring's copy launch for int32 actions ---------------------------------------------------------------------------------------
template <typename real>
struct DqnReplayArgs {
  ReplayArgs<real> r;         // ad = 1; r_act unused (NULL)
  const int32_t* r_act_i;     // int32 [T][B]
};

// one lane per (transition, observation column): replay_append_kernel of td3_impl.h with the action converted, (real)a
template <typename real>
__global__ __launch_bounds__(TD3_NT) void dqn_append_kernel(const DqnReplayArgs<real> S) {
  const ReplayArgs<real>& A = S.r;
  const int wc = A.od;
  const long long e = (long long)blockIdx.x * TD3_NT + threadIdx.x;
  const long long tb = e / wc;
  const int k = (int)(e - tb * wc);
  if (tb >= (long long)A.T * A.B) return;
  if (tb / A.B >= replay_steps(A.cursor, A.T)) return;
  long long h0 = A.head[0] % A.C;
  if (h0 < 0) h0 += A.C;
  const long long slot = (h0 + tb) % A.C;
  const bool fin = (A.r_done[tb] | A.r_trunc[tb]) != 0;
  A.obs[slot * A.od + k] = A.r_obs[tb * A.od + k];
  A.next[slot * A.od + k] = fin ? A.r_final[tb * A.od + k] : A.r_obs[(tb + A.B) * A.od + k];
  if (k == 0) {
    A.act[slot] = (real)S.r_act_i[tb];
    A.rwd[slot] = A.r_rwd[tb];
    A.boot[slot] = (!fin || A.r_trunc[tb] != 0) ? 1 : 0;
    A.live[slot] = A.r_valid[tb] != 0 ? 1 : 0;
  }
}

// ---- the gradient of one minibatch ---------------------------------------------------------------------------------------------------
template <typename real>
__global__ __launch_bounds__(TD3_NT) void dqn_q_kernel(const DqnArgs<real> S) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const Td3Args<real>& A = S.t;
  extern __shared__ __attribute__((aligned(16))) unsigned char dqn_lds[];
  const Td3Lds<real> L = td3_carve<real>(dqn_lds, A.n_hidden, A.hmax_pad, A.wcols);
  real* hbuf = L.hbuf;
  const size_t hstride = L.hstride;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x, n = A.act_dim;
  const bool dueling = S.dueling != 0;
  double st = 0.0;                                    // lane s < 6: the workgroup's sum of term s
  bool first = true;
  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB;
    __syncthreads();                                  // the previous tile's readers of xs and rowsrc are done
    td3_rowsrc(A, row0, L.rowsrc);
    // the row's own lane: the stored action; a row whose action is no index of the head is dead
    int a = 0;
    real rwd = real(0), gb = real(0), w = real(0);
    if (r < TB) {
      int src = L.rowsrc[r];
      if (src >= 0) {
        const real af = A.m_act[src];
        if (af >= real(0) && af < real(n) && (real)(int)af == af) a = (int)af;
        else L.rowsrc[r] = src = -1;
      }
      if (src >= 0) {
        rwd = A.m_rwd[src];
        gb = A.m_boot[src] != 0 ? A.gamma : real(0);
        w = real(1);
      }
    }
    const Td3View<real> Vn = td3_view(A, A.params, A.m_next, 0, A.obs_dim);
    const Td3View<real> Vt = td3_view(A, A.target, A.m_next, 0, A.obs_dim);
    const Td3View<real> V = td3_view(A, A.params, A.m_obs, 0, A.obs_dim);
    // ---- j* of the online network on s' (double) ----
    int jstar = -1;
    if (S.double_q) {
      policy_mlp<real, true>(Vn, A.mu, S.n_head, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
      __syncthreads();
      if (r < TB) jstar = dqn_argmax(dqn_row<real>(L.head, r, n, dueling), L.head, r, n);
    }
    // ---- y from the target network on s' ----
    policy_mlp<real, true>(Vt, A.mu, S.n_head, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
    __syncthreads();
    real y = real(0);
    if (r < TB && w != real(0)) {
      const DqnRow<real> R = dqn_row<real>(L.head, r, n, dueling);
      const int j = jstar >= 0 ? jstar : dqn_argmax(R, L.head, r, n);
      y = rwd + gb * dqn_value(R, L.head, r, j);
    }
    // ---- the online network on s, its activations kept; loss, statistics, the gradient at the head ----
    policy_mlp<real, true>(V, A.mu, S.n_head, 0, L.rowsrc, out_of, L.xs, L.ws, L.head);
    __syncthreads();
    real t_loss = real(0), t_q = real(0), t_abs = real(0), t_max = real(0);
    if (r < TB) {
      const DqnRow<real> R = dqn_row<real>(L.head, r, n, dueling);
      const real qa = dqn_value(R, L.head, r, a);
      const real qmax = dqn_value(R, L.head, r, dqn_argmax(R, L.head, r, n));
      const real delta = qa - y, ad = actor_abs(delta);
      real g = delta, loss = real(0.5) * (delta * delta);
      if (S.huber > real(0) && ad > S.huber) {
        g = delta < real(0) ? -S.huber : S.huber;
        loss = S.huber * (ad - real(0.5) * S.huber);
      }
      g = w * g;
      t_loss = w * loss; t_q = w * qa; t_abs = w * ad; t_max = w * qmax;
      for (int j = 0; j < n; j++) {
        const real ind = j == a ? real(1) : real(0);
        L.head[j * TBP + r] = dueling ? g * (ind - S.inv_n) : g * ind;
      }
      if (dueling) L.head[n * TBP + r] = g;
    }
    td3_backward<real, true>(V, A.mu, S.n_head, 0, L.rowsrc, L, slab, first);
    __syncthreads();
    if (r < TB) {
      L.xs[0 * TBP + r] = t_loss; L.xs[1 * TBP + r] = t_q; L.xs[2 * TBP + r] = w * y;
      L.xs[3 * TBP + r] = t_abs; L.xs[4 * TBP + r] = w; L.xs[5 * TBP + r] = t_max;
    }
    __syncthreads();
    td3_tile_stats<real>(L.xs, 6, st);
  }
  if (r < BCN_DQN_N_STATS) {
    // lane s < 6 holds term s: loss, q, y, |delta|, w to their slots, max_j Q_j to q_max_mean; the other lanes zero the other slots
    const int slot[BCN_DQN_N_STATS] = {0, 1, 2, 3, BCN_DQN_STAT_W, BCN_DQN_STAT_Q_MAX_MEAN, BCN_DQN_STAT_GRAD_NORM, BCN_DQN_STAT_SPARE};
    A.wg_stats[(size_t)blockIdx.x * BCN_DQN_N_STATS + slot[r]] = r < 6 ? st : 0.0;
  }
}

// ---- reduce --------------------------------------------------------------------------------------------------------------------------
// grad[p] = (sum_g slab_g[p]) / W for g ascending, p = e0 + block * 256 + lane; the block's part of the squared norm; block 0: the
// statistics (td3_reduce_kernel with this library's eight words)
template <typename real>
__global__ __launch_bounds__(TD3_NT) void dqn_reduce_kernel(const Td3ReduceArgs<real> A) {
  __shared__ double tot[BCN_DQN_N_STATS];
  __shared__ double sh[TD3_NT];
  const int t = threadIdx.x;
  if (t < BCN_DQN_N_STATS) {
    double s = 0.0;
    for (int g = 0; g < A.used; g++) s += A.wg_stats[(size_t)g * BCN_DQN_N_STATS + t];
    tot[t] = s;
  }
  __syncthreads();
  const double W = tot[BCN_DQN_STAT_W] > 1.0 ? tot[BCN_DQN_STAT_W] : 1.0;
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
      A.stats[BCN_DQN_STAT_LOSS] = tot[BCN_DQN_STAT_LOSS] / W;
      A.stats[BCN_DQN_STAT_Q_MEAN] = tot[BCN_DQN_STAT_Q_MEAN] / W;
      A.stats[BCN_DQN_STAT_TARGET_MEAN] = tot[BCN_DQN_STAT_TARGET_MEAN] / W;
      A.stats[BCN_DQN_STAT_TD_ABS_MEAN] = tot[BCN_DQN_STAT_TD_ABS_MEAN] / W;
      A.stats[BCN_DQN_STAT_Q_MAX_MEAN] = tot[BCN_DQN_STAT_Q_MAX_MEAN] / W;
      A.stats[BCN_DQN_STAT_W] = W;
      A.stats[BCN_DQN_STAT_SPARE] = 0.0;
    }
  }
}

// target[p] += tau (params[p] - target[p]); tau = 1 is the hard copy, exactly (t + (p - t) rounds twice and need not give p back)
template <typename real>
__global__ __launch_bounds__(TD3_NT) void dqn_polyak_kernel(const real* __restrict__ params, real* __restrict__ target, int n, real tau) {
  const int p = blockIdx.x * TD3_NT + threadIdx.x;
  if (p < n) {
    const real t = target[p], v = params[p];
    target[p] = tau == real(1) ? v : t + tau * (v - t);
  }
}

template <typename real>
__global__ void dqn_tick_kernel(int32_t* step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step[0] = step[0] + 1;
}

// ---- the launches: defined by dqn.hip (float) and dqn_f64.hip (double); hipError_t as int ----------------------------------------------
enum { DQN_K_ACT = 0, DQN_K_Q = 1 };
template <typename real> int dqn_launch_tile(int kernel, const DqnArgs<real>& a, int grid, void* stream);
template <typename real> int dqn_launch_reduce(const Td3ReduceArgs<real>& r, int blocks, double* norm_out, void* stream);
template <typename real> int dqn_launch_adam(const Td3AdamArgs<real>& a, void* stream);
template <typename real> int dqn_launch_polyak(const real* params, real* target, int n, real tau, void* stream);
template <typename real> int dqn_launch_append(const DqnReplayArgs<real>& a, void* stream);

#define DQN_DEFINE_LAUNCH(real)                                                                                          \
  template <> int dqn_launch_tile<real>(int kernel, const DqnArgs<real>& a, int grid, void* stream) {                   \
    typedef void (*kern_t)(const DqnArgs<real>);                                                                        \
    static const kern_t table[2] = {dqn_act_kernel<real>, dqn_q_kernel<real>};                                          \
    static size_t lds_allowed[2][64] = {{0}};                                                                           \
    const size_t lds = td3_lds_bytes<real>(a.t.n_hidden, a.t.hmax_pad, a.t.wcols);                                      \
    const hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(table[kernel]), lds, lds_allowed[kernel]);      \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(table[kernel], dim3(grid), dim3(TD3_NT), lds, static_cast<hipStream_t>(stream), a);              \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int dqn_launch_reduce<real>(const Td3ReduceArgs<real>& r, int blocks, double* norm_out, void* stream) {   \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(dqn_reduce_kernel<real>, dim3(blocks), dim3(TD3_NT), 0, s, r);                                   \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(td3_finish_kernel<real>, dim3(1), dim3(TD3_NT), 0, s, (const double*)r.norm2, blocks, norm_out); \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int dqn_launch_adam<real>(const Td3AdamArgs<real>& a, void* stream) {                                     \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    hipLaunchKernelGGL(td3_adam_kernel<real>, dim3((a.e1 - a.e0 + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0, s, a);        \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(dqn_tick_kernel<real>, dim3(1), dim3(64), 0, s, a.step);                                         \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int dqn_launch_polyak<real>(const real* params, real* target, int n, real tau, void* stream) {            \
    hipLaunchKernelGGL(dqn_polyak_kernel<real>, dim3((n + TD3_NT - 1) / TD3_NT), dim3(TD3_NT), 0,                       \
                       static_cast<hipStream_t>(stream), params, target, n, tau);                                       \
    return (int)hipGetLastError();                                                                                      \
  }                                                                                                                     \
  template <> int dqn_launch_append<real>(const DqnReplayArgs<real>& a, void* stream) {                                 \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                   \
    const long long total = (long long)a.r.T * a.r.B * a.r.od;                                                          \
    hipLaunchKernelGGL(dqn_append_kernel<real>, dim3((unsigned)((total + TD3_NT - 1) / TD3_NT)), dim3(TD3_NT), 0, s, a); \
    const hipError_t e = hipGetLastError();                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                 \
    hipLaunchKernelGGL(replay_advance_kernel<real>, dim3(1), dim3(64), 0, s, a.r.head, a.r.cursor, a.r.T, a.r.B, a.r.C); \
    return (int)hipGetLastError();                                                                                      \
  }

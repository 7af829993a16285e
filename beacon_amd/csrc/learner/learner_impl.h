// learner_impl.h -- the kernels of libbeacon_learner.so (include/beacon_learner.h: bcn_learner_grad, bcn_learner_step), templated on
// the real type and instantiated by learner.hip (float32) and learner_f64.hip (float64).
//
// The backward launch runs the actor's networks on the actor's tile: the geometry, the staging (with the learner's GATHERED rows: idx,
// zero rows for weight 0), the layer in its forward and its transposed form, the walk over an MLP and the head's log-density terms are
// ../actor/policy_net.h, compiled into both libraries.  What is the learner's own:
//   learner_dw      dW[o][k] = sum_r D[o][r] X[k][r] over the tile's rows: each lane owns 4 x 4 entries, reads four 16-byte chunks of
//                   each array per four rows (64 fma per 8 LDS reads) and adds its entries to the workgroup's slab in HBM
// LDS: n_hidden activation buffers [hmax][TBP] (every layer's output is kept: the backward pass overwrites them with the gradients,
// top down), xs [KS][TBP] (a slab of gathered observations; between layers: scratch for the sums over the tile's rows), ws
// [KS][wcols], head [16][TBP], the rows' sources int32 [TB].  At the limits (3 x 128 wide): 160 256 bytes in float32, 158 336 in
// float64, of 163 840.
//
// Plain fma for the same reasons as in the actor (policy_net.h); no atomics, no inter-workgroup communication inside a launch.
#pragma once
#include "../actor/actor_impl.h"          // policy_net.h comes with it
#include "../../../include/beacon_learner.h"

#define LEARNER_NT ACTOR_NT
#define LEARNER_MAX_PSEGS (4 * (BCN_ACTOR_MAX_LAYERS + 1) + 1)
#define LEARNER_RED_PARAMS 64        // parameters per block of the reduce launch
#define LEARNER_RED_SPLIT 4          // lanes per parameter: each adds a quarter of the slabs

template <typename real>
struct LearnerArgs {
  const real* params;
  const real* obs;                  // [n_rows][obs_dim]
  const void* act;                  // real [n_rows][act_dim] or int32 [n_rows]
  const real *logp_old, *adv, *ret;
  const void* weight;
  const int32_t* idx;
  const int32_t* cursor;
  long long n_rows, m, tiles;
  int weight_kind, rows_per_step;
  int obs_dim, n_hidden, hidden[BCN_ACTOR_MAX_LAYERS], activation, kind, act_dim;
  int hmax_pad, wcols;
  ActorNet pi, vf;
  unsigned log_std;
  real clip, vf_coef, ent_coef;
  real* slabs;                      // [grid][slab_elems]
  size_t slab_elems;
  double* wg_stats;                 // [grid][8]
  int rows_per_weight;              // consecutive rows that share one element of weight, >= 1 (last: the fields above keep their offsets)
};

template <typename real>
struct LearnerReduceArgs {
  const real* slabs;
  size_t slab_elems;
  int used;                         // slabs written: the backward launch's workgroups
  const double* wg_stats;
  real* grad;
  int n_elems;                      // elements of the gradient buffer, gaps between segments included
  int n_segs;
  int seg_begin[LEARNER_MAX_PSEGS], seg_end[LEARNER_MAX_PSEGS];
  double* norm2;                    // [blocks]
  double* stats;
  double vf_coef, ent_coef;
};

template <typename real>
struct LearnerAdamArgs {
  real* params;
  const real* grad;
  real *m, *v;
  const int32_t* step;
  const double* stats;
  int n_elems;
  double lr, beta1, beta2, eps, max_grad_norm;
  double target_kl, lr_end, lr_steps;       // appended (bcn_learner_adam): all 0 is the update without a stop rule and without a schedule
};

// the KL stop rule of include/beacon_learner.h, the same for every Adam lane and for the tick: nothing writes these words during the
// Adam launch.  A NaN approx_kl does not stop (the comparison is false).  Only called with target_kl > 0.
__device__ __forceinline__ bool learner_kl_stop(const int32_t* step, const double* stats, double target_kl) {
  return step[2] != 0 || stats[BCN_LEARNER_STAT_KL] > 1.5 * target_kl;
}

// dW[o][k0 + k] (+)= sum_r D[o][r] X[k][r] for o < OUT, k < ks, r ascending over the tile; with k0 = 0 also db[o] (+)= sum_r D[o][r].
// D, X: LDS, row stride TBP, complete (the caller synchronised).  gW: the workgroup's slab at the matrix [OUT][K], gB at the bias.
// `first`: the workgroup's first tile stores, the later ones add.  Lane = og * nkg + kg owns the outputs 4 og .. 4 og + 3 and, per
// chunk of 4 nkg columns, the columns 4 kg .. 4 kg + 3: consecutive lanes touch consecutive addresses of a slab row.
template <typename real>
__device__ __forceinline__ void learner_dw(const real* D, int OUT, const real* X, int ks, real* __restrict__ gW, real* __restrict__ gB, int K,
                                           int k0, bool first) {
  constexpr int TB = ActorGeom<real>::TB, TBP = TB + 4;
  const int lane = threadIdx.x;
  const int out4 = (OUT + 3) & ~3;
  int nog = 1;
  while (nog * 4 < out4) nog <<= 1;
  const int nkg = LEARNER_NT / nog;
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
template <typename real>
__device__ __forceinline__ void learner_backward(const LearnerArgs<real>& A, const ActorNet& net, int n_head, const int* rowsrc, real* hbuf,
                                                 size_t hstride, real* xs, real* ws, real* head, real* slab, bool first) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  for (int l = A.n_hidden; l >= 0; l--) {
    const real* D = l == A.n_hidden ? head : hbuf + l * hstride;
    const int OUT = l == A.n_hidden ? n_head : A.hidden[l];
    __syncthreads();                                // D is complete
    if (l > 0) {
      const int K = A.hidden[l - 1];
      real* X = hbuf + (l - 1) * hstride;
      learner_dw<real>(D, OUT, X, K, slab + net.w[l], slab + net.b[l], K, 0, first);
      // the gradient at this layer's input, in place over X (policy_layer synchronises before it writes anything)
      policy_layer<real, true, true>(A.params + net.w[l], nullptr, OUT, K, A.activation, D, A.obs, 0, 0, rowsrc, xs, ws, A.wcols, X);
    } else {
      const int K = A.obs_dim;
      for (int k0 = 0; k0 < K; k0 += KS) {
        const int ks = min(KS, K - k0);
        if (k0) __syncthreads();                    // the previous slab's readers of xs are done
        actor_stage<real, true>(A.obs, K, k0, ks, TB, 0, rowsrc, xs, TBP);
        __syncthreads();
        learner_dw<real>(D, OUT, xs, ks, slab + net.w[0], slab + net.b[0], K, k0, first);
      }
    }
  }
}

template <typename real>
__global__ __launch_bounds__(LEARNER_NT) void learner_backward_kernel(const LearnerArgs<real> A) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char learner_lds[];
  real* hbuf = reinterpret_cast<real*>(learner_lds);
  const size_t hstride = (size_t)A.hmax_pad * TBP;
  const auto out_of = [=](int l) { return hbuf + l * hstride; };      // every layer's output is kept for the backward pass
  real* xs = hbuf + (size_t)A.n_hidden * hstride;     // [KS][TBP]
  real* ws = xs + (size_t)KS * TBP;                   // [KS][wcols]
  real* head = ws + (size_t)KS * A.wcols;             // [BCN_ACTOR_MAX_ACT][TBP]
  int* rowsrc = reinterpret_cast<int*>(head + (size_t)BCN_ACTOR_MAX_ACT * TBP);   // [TB]
  real* slab = A.slabs + (size_t)blockIdx.x * A.slab_elems;
  const int r = threadIdx.x;
  const int n = A.act_dim;
  const real* log_std = A.params + A.log_std;
  double st = 0.0;                                    // lane s < 6: the workgroup's sum of statistic s
  bool first = true;

  for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x, first = false) {
    const long long row0 = tile * TB;
    __syncthreads();                                  // the previous tile's readers of xs and rowsrc are done
    // ---- the rows' sources and weights: one lane per row -------------------------------------------------------------------
    real w = real(0);
    int src = -1, cls = 0;
    if (r < TB && row0 + r < A.m) {
      const long long s = A.idx ? (long long)A.idx[row0 + r] : row0 + r;
      long long lim = A.n_rows;
      if (A.cursor) {
        const long long c = A.cursor[0] > 0 ? A.cursor[0] : 0;
        lim = min(lim, c * (long long)A.rows_per_step);
      }
      if (s >= 0 && s < lim) {
        // the row's weight element: s itself, or s / rows_per_weight (s < n_rows < 2^31: one 32-bit division per row per tile)
        const long long ws = A.rows_per_weight > 1 ? (long long)((uint32_t)s / (uint32_t)A.rows_per_weight) : s;
        real wv = real(1);
        if (A.weight_kind == BCN_LEARNER_W_U8) wv = (real) static_cast<const uint8_t*>(A.weight)[ws];
        else if (A.weight_kind == BCN_LEARNER_W_REAL) wv = static_cast<const real*>(A.weight)[ws];
        bool ok = wv > real(0);
        if (ok && A.kind == BCN_ACTOR_CATEGORICAL) {
          cls = static_cast<const int32_t*>(A.act)[s];
          ok = cls >= 0 && cls < n;
        }
        if (ok) { w = wv; src = (int)s; }
      }
    }
    if (r < TB) rowsrc[r] = src;

    // ---- the policy network ----------------------------------------------------------------------------------------------
    policy_mlp<real, true>(A, A.pi, n, 0, rowsrc, out_of, xs, ws, head);
    __syncthreads();
    real t_pg = real(0), t_h = real(0), t_kl = real(0), t_cf = real(0), t_v = real(0);
    if (r < TB) {
      real hd[BCN_ACTOR_MAX_ACT], dl[BCN_ACTOR_MAX_ACT], gl[BCN_ACTOR_MAX_ACT];
#pragma unroll
      for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) {
        hd[i] = i < n ? head[i * TBP + r] : real(0);
        dl[i] = real(0);
        gl[i] = real(0);
      }
      if (src >= 0) {
        real logp = real(0), H = real(0);
        real z[BCN_ACTOR_MAX_ACT], e[BCN_ACTOR_MAX_ACT];      // Gaussian: z, exp(-log_std); categorical: d, p
        if (A.kind == BCN_ACTOR_GAUSSIAN) {
          const real* a = static_cast<const real*>(A.act) + (size_t)src * n;
#pragma unroll
          for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) {
            z[i] = e[i] = real(0);
            if (i < n) {
              const real ls = log_std[i];
              e[i] = actor_exp(-ls);
              z[i] = (a[i] - hd[i]) * e[i];
              logp += policy_gauss_logp<real>(z[i], ls);
              H += ls + real(1.41893853320467274178);
            }
          }
        } else {
          POLICY_LOG_SUM_EXP(hd, n)
#pragma unroll
          for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++) {
            z[i] = e[i] = real(0);
            if (i < n) {
              z[i] = (hd[i] - mx) - lse;
              e[i] = actor_exp(z[i]);
              H -= e[i] * z[i];
              if (i == cls) logp = z[i];
            }
          }
        }
        const real dlp = logp - A.logp_old[src];
        const real ratio = actor_exp(dlp), adv = A.adv[src];
        const real lo = real(1) - A.clip, hi = real(1) + A.clip;
        const real s1 = ratio * adv, s2 = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * adv;
        const bool unclipped = s1 <= s2;
        const real g = unclipped ? -s1 : real(0);              // d pg / d logp
        t_pg = w * -(unclipped ? s1 : s2);
        t_h = w * H;
        t_kl = w * ((ratio - real(1)) - dlp);
        t_cf = actor_abs(ratio - real(1)) > A.clip ? w : real(0);
        if (A.kind == BCN_ACTOR_GAUSSIAN) {
#pragma unroll
          for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)
            if (i < n) {
              dl[i] = w * (g * z[i] * e[i]);
              gl[i] = w * (g * (z[i] * z[i] - real(1)) - A.ent_coef);
            }
        } else {
#pragma unroll
          for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)
            if (i < n) dl[i] = w * (g * ((i == cls ? real(1) : real(0)) - e[i]) + A.ent_coef * (e[i] * (z[i] + H)));
        }
      }
#pragma unroll
      for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)
        if (i < n) {
          head[i * TBP + r] = dl[i];
          xs[i * TBP + r] = gl[i];
        }
    }
    __syncthreads();
    if (A.kind == BCN_ACTOR_GAUSSIAN && r < n) {               // d L / d log_std: the sum over the tile's rows
      real s = real(0);
      for (int q = 0; q < TB; q++) s += xs[r * TBP + q];
      real* at = slab + A.log_std + r;
      *at = first ? s : *at + s;
    }
    learner_backward<real>(A, A.pi, n, rowsrc, hbuf, hstride, xs, ws, head, slab, first);

    // ---- the value network -----------------------------------------------------------------------------------------------
    policy_mlp<real, true>(A, A.vf, 1, 0, rowsrc, out_of, xs, ws, head);
    __syncthreads();
    if (r < TB) {
      real d = real(0);
      if (src >= 0) {
        const real err = head[r] - A.ret[src];
        t_v = w * (err * err);
        d = w * (A.vf_coef * (real(2) * err));
      }
      head[r] = d;
    }
    learner_backward<real>(A, A.vf, 1, rowsrc, hbuf, hstride, xs, ws, head, slab, first);

    // ---- the statistics: per-row terms through xs, summed in float64 for r ascending -----------------------------------------
    __syncthreads();
    if (r < TB) {
      xs[0 * TBP + r] = t_pg; xs[1 * TBP + r] = t_v; xs[2 * TBP + r] = t_h;
      xs[3 * TBP + r] = t_kl; xs[4 * TBP + r] = t_cf; xs[5 * TBP + r] = w;
    }
    __syncthreads();
    if (r < 6)
      for (int q = 0; q < TB; q++) st += (double)xs[r * TBP + q];
  }
  if (r < BCN_LEARNER_N_STATS) A.wg_stats[(size_t)blockIdx.x * BCN_LEARNER_N_STATS + r] = r < 6 ? st : 0.0;
}

// grad[p] = (sum_g slab_g[p]) / W for g ascending; the block's part of the squared norm; block 0: stats[0 .. 6].
// Lane = part * 64 + j: parameter blockIdx * 64 + j, the slabs part * ceil(used / 4) ... of it.
template <typename real>
__global__ __launch_bounds__(LEARNER_NT) void learner_reduce_kernel(const LearnerReduceArgs<real> A) {
  __shared__ double tot[BCN_LEARNER_N_STATS];
  __shared__ double wg[BCN_LEARNER_N_STATS][BCN_LEARNER_MAX_GRID + 1];
  __shared__ double part[LEARNER_RED_SPLIT][LEARNER_RED_PARAMS];
  const int t = threadIdx.x;
  // the workgroups' partial statistics: one row per lane, every load in flight at once; then statistic s is summed by lane s for g ascending
  for (int g = t; g < A.used; g += LEARNER_NT) {
    double v[BCN_LEARNER_N_STATS];
#pragma unroll
    for (int k = 0; k < BCN_LEARNER_N_STATS; k++) v[k] = A.wg_stats[(size_t)g * BCN_LEARNER_N_STATS + k];
#pragma unroll
    for (int k = 0; k < BCN_LEARNER_N_STATS; k++) wg[k][g] = v[k];
  }
  __syncthreads();
  if (t < BCN_LEARNER_N_STATS) {
    double s = 0.0;
    for (int g = 0; g < A.used; g++) s += wg[t][g];
    tot[t] = s;
  }
  const int j = t % LEARNER_RED_PARAMS, sp = t / LEARNER_RED_PARAMS;
  const int p = blockIdx.x * LEARNER_RED_PARAMS + j;
  bool in_seg = false;
  if (p < A.n_elems)
    for (int s = 0; s < A.n_segs; s++) in_seg = in_seg || (p >= A.seg_begin[s] && p < A.seg_end[s]);
  const int per = (A.used + LEARNER_RED_SPLIT - 1) / LEARNER_RED_SPLIT;
  const int g0 = sp * per, g1 = min(A.used, g0 + per);
  double s = 0.0;
  if (in_seg) {
    for (int g = g0; g < g1; g += 8) {              // eight loads in flight, added in the order g ascending
      real v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = g + u < g1 ? A.slabs[(size_t)(g + u) * A.slab_elems + p] : real(0);
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (g + u < g1) s += (double)v[u];
    }
  }
  part[sp][j] = s;
  __syncthreads();
  const double W = tot[5] > 1.0 ? tot[5] : 1.0;
  if (sp == 0) {
    double sum = part[0][j];
#pragma unroll
    for (int q = 1; q < LEARNER_RED_SPLIT; q++) sum += part[q][j];
    const real g = (real)(sum / W);
    if (p < A.n_elems) A.grad[p] = in_seg ? g : real(0);
    part[0][j] = in_seg ? (double)g * (double)g : 0.0;
  }
  __syncthreads();
  if (t == 0) {
    double q = 0.0;
    for (int i = 0; i < LEARNER_RED_PARAMS; i++) q += part[0][i];
    A.norm2[blockIdx.x] = q;
    if (blockIdx.x == 0) {
      const double pg = tot[0] / W, vf = tot[1] / W, ent = tot[2] / W;
      A.stats[BCN_LEARNER_STAT_LOSS] = pg + A.vf_coef * vf - A.ent_coef * ent;
      A.stats[BCN_LEARNER_STAT_PG] = pg;
      A.stats[BCN_LEARNER_STAT_VF] = vf;
      A.stats[BCN_LEARNER_STAT_ENTROPY] = ent;
      A.stats[BCN_LEARNER_STAT_KL] = tot[3] / W;
      A.stats[BCN_LEARNER_STAT_CLIP_FRAC] = tot[4] / W;
      A.stats[BCN_LEARNER_STAT_W] = W;
    }
  }
}

// stats[7] = sqrt(sum of the reduce launch's partials): lane t adds the partials t, t + 256, ... ascending, then a fixed tree
template <typename real>      // (a template only so that each unit instantiates its own)
__global__ __launch_bounds__(LEARNER_NT) void learner_finish_kernel(const double* norm2, int n_blocks, double* stats) {
  __shared__ double sh[LEARNER_NT];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n_blocks; i += LEARNER_NT) s += norm2[i];
  sh[t] = s;
  __syncthreads();
  for (int d = LEARNER_NT / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  if (t == 0) stats[BCN_LEARNER_STAT_GRAD_NORM] = sqrt(sh[0]);
}

template <typename real>
__global__ __launch_bounds__(LEARNER_NT) void learner_adam_kernel(const LearnerAdamArgs<real> A) {
  const int p = blockIdx.x * LEARNER_NT + threadIdx.x;
  if (p >= A.n_elems) return;
  if (A.target_kl > 0.0 && learner_kl_stop(A.step, A.stats, A.target_kl)) return;      // params, m and v stay as they are
  const double norm = A.stats[BCN_LEARNER_STAT_GRAD_NORM];
  double scale = 1.0;
  if (A.max_grad_norm > 0.0) {
    scale = A.max_grad_norm / (norm + 1e-6);
    scale = scale < 1.0 ? scale : 1.0;
  }
  const double t = (double)(A.step[0] + 1);
  double lr = A.lr;
  if (A.lr_steps > 0.0) {                             // linear from lr to lr_end over lr_steps steps TAKEN, then lr_end
    const double done = (double)A.step[0];
    lr = A.lr + (A.lr_end - A.lr) * (done < A.lr_steps ? done : A.lr_steps) / A.lr_steps;
  }
  const real step_size = (real)(lr / (1.0 - pow(A.beta1, t)));
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

// the step is counted, or -- under the stop rule -- the flag is set and the skipped step counted; target_kl <= 0: step[1 .. 3] are
// neither read nor written
template <typename real>
__global__ void learner_tick_kernel(int32_t* step, const double* stats, double target_kl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (target_kl > 0.0 && learner_kl_stop(step, stats, target_kl)) {
      step[2] = 1;
      step[3] = step[3] + 1;
    } else {
      step[0] = step[0] + 1;
    }
  }
}

// bytes of dynamic LDS of one workgroup of the backward launch
template <typename real>
inline size_t learner_lds_bytes(int n_hidden, int hmax_pad, int wcols) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  return sizeof(real) * ((size_t)n_hidden * hmax_pad * TBP + (size_t)KS * TBP + (size_t)KS * wcols + (size_t)BCN_ACTOR_MAX_ACT * TBP) + sizeof(int) * TB;
}

// defined by learner.hip (float) and learner_f64.hip (double): the launches, hipError_t as int
template <typename real> int learner_launch_grad(const LearnerArgs<real>& a, const LearnerReduceArgs<real>& r, int grid, int red_blocks, void* stream);
template <typename real> int learner_launch_step(const LearnerAdamArgs<real>& a, int32_t* step, void* stream);

#define LEARNER_DEFINE_LAUNCH(real)                                                                                     \
  template <> int learner_launch_grad<real>(const LearnerArgs<real>& a, const LearnerReduceArgs<real>& r, int grid,    \
                                            int red_blocks, void* stream) {                                            \
    const size_t lds = learner_lds_bytes<real>(a.n_hidden, a.hmax_pad, a.wcols);                                        \
    static size_t lds_allowed[64] = {0};                                                                               \
    hipError_t e = policy_allow_lds(reinterpret_cast<const void*>(&learner_backward_kernel<real>), lds, lds_allowed);  \
    if (e != hipSuccess) return (int)e;                                                                                \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                  \
    hipLaunchKernelGGL(learner_backward_kernel<real>, dim3(grid), dim3(LEARNER_NT), lds, s, a);                        \
    e = hipGetLastError();                                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                \
    hipLaunchKernelGGL(learner_reduce_kernel<real>, dim3(red_blocks), dim3(LEARNER_NT), 0, s, r);                      \
    e = hipGetLastError();                                                                                             \
    if (e != hipSuccess) return (int)e;                                                                                \
    hipLaunchKernelGGL(learner_finish_kernel<real>, dim3(1), dim3(LEARNER_NT), 0, s, (const double*)r.norm2, red_blocks, r.stats); \
    return (int)hipGetLastError();                                                                                     \
  }                                                                                                                    \
  template <> int learner_launch_step<real>(const LearnerAdamArgs<real>& a, int32_t* step, void* stream) {             \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                  \
    hipLaunchKernelGGL(learner_adam_kernel<real>, dim3((a.n_elems + LEARNER_NT - 1) / LEARNER_NT), dim3(LEARNER_NT), 0, s, a); \
    const hipError_t e = hipGetLastError();                                                                            \
    if (e != hipSuccess) return (int)e;                                                                                \
    hipLaunchKernelGGL(learner_tick_kernel<real>, dim3(1), dim3(64), 0, s, step, a.stats, a.target_kl);                \
    return (int)hipGetLastError();                                                                                     \
  }

/* beacon_sac.h -- C ABI of libbeacon_sac.so: soft actor-critic on the device -- a tanh-squashed Gaussian policy with a state-dependent
 * log-std, one or two critics Q(s, a), their targets and a learned temperature (hand-written HIP for gfx950).
 *
 * The library is a unit of its own, like the actor's, the learner's, the epochs' and the TD3 library: it takes device pointers and
 * sizes only and adds nothing to the other five headers.  Its networks run on the actor's tile with the actor's layer
 * (csrc/actor/policy_net.h); the slabs, the backward pass of one MLP and the Adam, Polyak and finish kernels are the templates of
 * csrc/td3/td3_impl.h, instantiated in this library too; what both lack is csrc/sac/sac_impl.h.  The replay memory is NOT restated
 * here: it is libbeacon_td3.so's (bcn_replay_layout, bcn_replay_append, bcn_replay_sample of include/beacon_td3.h), and this library
 * receives its six row segments as separate device pointers plus the capacity.
 * Every launch: no host read, no allocation, no atomics, sums in a fixed order (float64 where include/beacon_td3.h uses float64),
 * separate launches as the only synchronisation between workgroups, capturable in a graph, bit-reproducible.
 *
 * Conventions: every function returns 0 (BCN_SAC_OK) or a BCN_SAC_ERR_* code (*_layout: the segment count, 0 on error; *_bytes: the
 * byte count, 0 on error); bcn_sac_last_error() gives text.  Pointers named *_dev are DEVICE pointers; "real" is float for dtype 0
 * and double for dtype 1.  Every argument is checked before a device is touched.
 *
 * ---- Networks ----------------------------------------------------------------------------------------------------------------
 * cfg: the fields of bcn_td3_cfg (SAC needs none more: target_entropy and the optimisers' rates are arguments of the launches);
 * 1 .. 3 hidden layers of 1 .. 128 units (the same widths for every network), activation tanh (0) or relu (1), act_dim n in 1 .. 16,
 * obs_dim >= 1 with D = obs_dim + act_dim <= 512, one scalar bound pair low < high STRICTLY (ln h appears below), n_critics 1 or 2.
 *   c = (high + low) / 2,  h = (high - low) / 2,  ln h: formed in float64 and rounded once to real
 *   policy pi     an MLP obs_dim -> 2n with a linear head: ONE matrix [2n][h_last]; rows 0 .. n - 1 are the mean, rows n .. 2n - 1
 *                 the raw log-std
 *   critics Q_i   MLPs D -> 1 on the row [obs | a], with a linear head
 * Every output of every layer is the fma chain  acc = bias;  acc = fma(W[o][k], x[k], acc)  for k ascending, then the activation.
 * One parameter buffer holds the segments  pi_w0, pi_b0, ... pi_w{L}, pi_b{L}, q1_w0, ... q1_b{L}, (q2_w0, ... q2_b{L}), log_alpha [1]
 * for L = n_hidden, each 16-byte aligned, matrices [out][in]; q*_w0 is [hidden[0]][D] with the observation columns first.  The
 * temperature is alpha = exp(log_alpha), read on the device.  A target buffer has the same layout; only its q segments are ever
 * read (there is no target policy); Polyak runs over the whole buffer.
 * LDS: the 2n <= 32 head rows of pi live in the tile's row staging buffer ([64][68] float32, [32][36] float64), which is dead while
 * the head layer runs (its input is an activation buffer); the sum per dtype is stated in csrc/sac/sac_impl.h -- 160 256 bytes in
 * float32 and 158 336 in float64 at act_dim 16, hidden 3 x 128, of BCN_SAC_LDS_LIMIT = 163 840.  bcn_sac_lds_bytes(cfg) returns the
 * sum; a cfg whose sum exceeded the limit would be refused by every function here before any launch.
 *
 * ---- The policy, per row -----------------------------------------------------------------------------------------------------------
 * With head[0 .. 2n) the head's outputs and z_j standard normal, for j ascending:
 *   m_j  = head[j];  ls_j = clamp(head[n + j], -20, 2);  sd_j = exp(ls_j)
 *   u_j  = m_j + sd_j z_j;  t_j = tanh(u_j);  a_j = c + h t_j
 *   lp_j = (((-z_j^2 / 2 - ls_j) - ln(2 pi) / 2) - ln h) - 2 ((ln 2 - u_j) - softplus(-2 u_j))
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   log pi = sum_j lp_j, j ascending from 0
 * ln(1 - t^2) = 2 (ln 2 - u - softplus(-2u)) exactly; it is never evaluated as log(1 - t * t), which is -inf once tanh rounds to 1
 * (|u| > 9 in float32, 19 in float64): log pi stays finite for any finite u.
 * Derivatives: d log pi / d u_j = 2 t_j (through the squashing term; z is the draw and carries none); d / d ls_j adds -1 directly and
 * sd_j z_j times the u term; the clamp passes gradient where -20 <= raw <= 2 (both ends included: torch.clamp's rule).
 *
 * ---- Random streams ----------------------------------------------------------------------------------------------------------
 * All draws are words of the project's one Philox4x32-10 definition under the key (low, high word of seed).  The last counter word
 * names the stream: 0 .. 6 are taken (include/beacon_td3.h lists them; 5 is replay sampling, bcn_replay_sample), and here
 *   7 acting                                   counter (replica_offset + b, counters[b], j, 7)
 *   8 the next action in the critic target     counter (i, step[3], j, 8),  i the row of the minibatch
 *   9 the policy step's draw                   counter (i, step[4], j, 9)
 * A standard normal pair (z_{2j}, z_{2j+1}) comes from the four words at pair index j by the actor's Box-Muller form, as in
 * include/beacon_td3.h.  The uniform mode's u in [0, 1) at index j = the action component is TD3's single uniform, on stream 7.
 *
 * ---- Acting: bcn_sac_act, ONE launch -------------------------------------------------------------------------------------------
 * One workgroup per tile of rows runs pi on obs_dev [batch][obs_dim] and writes actions_dev [batch][act_dim]:
 *   BCN_SAC_DETERMINISTIC  a = c + h tanh(m)
 *   BCN_SAC_SAMPLE         a as above with z from stream 7
 *   BCN_SAC_UNIFORM        a = low + (high - low) u  (pi is not evaluated)
 * `counters` (uint32 [batch], the first segment of the state buffer) tick once per stochastic launch (sample, uniform).  A replica
 * whose mask byte is 0 keeps its action row and its counter.
 *
 * ---- The update --------------------------------------------------------------------------------------------------------------
 * A minibatch is the m rows idx_dev names; w = live (0 or 1), W = max(sum w, 1).  A row with w = 0, or an index outside 0 .. C - 1,
 * is staged as zeros: its fields may hold anything, NaN included.
 * bcn_sac_critic_grad, FOUR launches:
 *   1. next:    per row  a' ~ pi_params(s') (the CURRENT policy) with z from stream 8, and log pi'; the rows [s' | a'] and [s | a] and
 *               (rwd, boot, w, log pi') go to the work buffer
 *   2. critic:  per row  y = rwd + (gamma boot) (min_i Q_i,target(s', a') - alpha log pi')  (no gradient through y, none into alpha);
 *               loss = sum_i sum_rows w (Q_i(s, a) - y)^2 / W;  the gradient of its numerator for the q segments into per-workgroup
 *               slabs: workgroup g of G = min(tiles, bcn_sac_grid) walks the tiles g, g + G, ... and adds tile after tile, rows
 *               ascending inside a tile.  The two critics run one after the other.
 *   3. reduce:  grad[p] = (sum_g slab_g[p]) / W for g ascending, in float64, rounded once; the statistics
 *   4. finish:  stats[critic_grad_norm] = sqrt(sum grad^2) over the q segments, in float64 in a fixed tree
 * bcn_sac_actor_grad, FOUR launches (it reads (w) of the LAST bcn_sac_critic_grad's minibatch: call it behind one, same idx):
 *   1. pi:      a~ ~ pi(s) per row with z from stream 9; the rows [s | a~] go to the work buffer
 *   2. actor:   loss = sum w (alpha log pi - Q_min) / W.  Q_1 forward with its activations kept; backward down to the ACTION columns of
 *               its first layer's input, dQ/da_j = sum_q W0[q][obs_dim + j] g0[q] for q ascending; with two critics the same for Q_2,
 *               and per row the gradient (and the value) of the smaller Q: Q_2's only where Q_2 < Q_1 strictly.  pi forward again with
 *               its activations kept (the same draw); the gradient at the head, per row times w,
 *                 g_u,j = -dQ/da_j h (1 - t_j^2) + alpha 2 t_j;   g_m,j = g_u,j;   g_ls,j = (g_u,j sd_j z_j - alpha) [clamp passes]
 *               then backward down pi from all 2n head rows into the slabs.  The critics get no gradient; alpha gets none from this loss.
 *   3. reduce:  as above over the pi segments; and the temperature's gradient  grad[log_alpha] = -(sum w log pi + target_entropy sum w)
 *               / W  -- the derivative of  -log_alpha sum w (log pi + target_entropy) / W  with log pi the VALUE of these draws -- in
 *               float64, rounded once; stats[policy_loss], stats[logp_mean], stats[alpha_grad]
 *   4. finish:  stats[policy_grad_norm] over the pi segments (the log_alpha element is no part of it)
 * bcn_sac_adam, TWO launches: Adam of include/beacon_learner.h, the arithmetic of bcn_td3_adam, over the q segments (which =
 * BCN_SAC_OPT_CRITIC), the pi segments (BCN_SAC_OPT_POLICY) or the log_alpha element (BCN_SAC_OPT_ALPHA), t = step[which] + 1; global-
 * norm clipping (max_grad_norm > 0) applies to CRITIC and POLICY only.  Then one lane ticks step[which], and with CRITIC also step[3],
 * with POLICY also step[4]: the counters of streams 8 and 9.
 * bcn_sac_polyak, ONE launch: target[p] += tau (params[p] - target[p]) over the whole buffer (tau rounded once to real).
 * One SAC minibatch is sample (2, libbeacon_td3.so) + critic_grad (4) + adam (2) + actor_grad (4) + adam POLICY (2) + adam ALPHA (2,
 * only when the temperature is learned) + polyak (1) = 17 launches, 15 with a fixed temperature.  Whether the alpha step runs is the
 * CALLER's control flow.
 *
 * stats (float64 [12], a segment of the state buffer): critic_loss, q1_mean, q2_mean, target_mean (the W-weighted means of Q_1(s, a),
 * Q_2(s, a) -- 0 with one critic -- and y), policy_loss, W, critic_grad_norm, policy_grad_norm (before clipping), logp_mean (of the
 * policy step's draws), next_logp_mean (of the critic step's), alpha (exp(log_alpha) as the last reduce launch read it), alpha_grad.
 */
#ifndef BEACON_SAC_H
#define BEACON_SAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_SAC_API __attribute__((visibility("default")))
#define BCN_SAC_API_VERSION 1

enum { BCN_SAC_OK = 0, BCN_SAC_ERR_ARG = 1, BCN_SAC_ERR_HIP = 2 };
/* element types of a segment */
enum { BCN_SAC_REAL = 0, BCN_SAC_I32 = 1, BCN_SAC_U32 = 2, BCN_SAC_F64 = 3, BCN_SAC_U8 = 4 };
enum { BCN_SAC_DETERMINISTIC = 0, BCN_SAC_SAMPLE = 1, BCN_SAC_UNIFORM = 2 };
enum { BCN_SAC_OPT_CRITIC = 0, BCN_SAC_OPT_POLICY = 1, BCN_SAC_OPT_ALPHA = 2 };
enum { BCN_SAC_STAT_CRITIC_LOSS = 0, BCN_SAC_STAT_Q1 = 1, BCN_SAC_STAT_Q2 = 2, BCN_SAC_STAT_TARGET = 3, BCN_SAC_STAT_POLICY_LOSS = 4,
       BCN_SAC_STAT_W = 5, BCN_SAC_STAT_CRITIC_NORM = 6, BCN_SAC_STAT_POLICY_NORM = 7, BCN_SAC_STAT_LOGP = 8, BCN_SAC_STAT_NEXT_LOGP = 9,
       BCN_SAC_STAT_ALPHA = 10, BCN_SAC_STAT_ALPHA_GRAD = 11, BCN_SAC_N_STATS = 12 };

#define BCN_SAC_MAX_IN 512        /* obs_dim + act_dim, at most */
#define BCN_SAC_MAX_GRID 128      /* workgroups of the backward launches, at most */
#define BCN_SAC_MAX_SEGS 32
#define BCN_SAC_LDS_LIMIT 163840  /* bytes of dynamic LDS a tile kernel may ask for */

typedef struct {
  int32_t batch;        /* replicas bcn_sac_act serves and the state buffer counts for */
  int32_t obs_dim, act_dim;
  int32_t dtype;        /* 0 float32, 1 float64 */
  int32_t n_hidden, hidden[3];
  int32_t activation;   /* 0 tanh, 1 relu */
  double low, high;     /* low < high */
  int32_t n_critics;    /* 1 or 2 */
} bcn_sac_cfg;

/* One named segment: row_elems elements of kind `elem` at `offset` bytes (the fields of bcn_td3_seg; planes is 0). */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;
  int32_t planes;
  int64_t row_elems;
} bcn_sac_seg;

typedef struct {
  const void* params_dev;     /* the parameter buffer */
  const void* target_dev;     /* the target buffer (critic_grad) */
  const void* obs_dev;        /* the replay memory's segments, `capacity` rows each: real [C][obs_dim] */
  const void* act_dev;        /* real [C][act_dim] */
  const void* rwd_dev;        /* real [C] */
  const void* next_obs_dev;   /* real [C][obs_dim] */
  const uint8_t* boot_dev;    /* uint8 [C] */
  const uint8_t* live_dev;    /* uint8 [C] */
  const int32_t* idx_dev;     /* int32 [m] */
  void* work_dev;             /* bcn_sac_work_bytes(cfg, m) bytes */
  void* state_dev;            /* bcn_sac_state_bytes(cfg) bytes */
  int64_t m;                  /* rows of the minibatch, 1 .. 2^31 - 1 */
  int64_t capacity;
  double gamma, target_entropy;
  uint64_t seed;
} bcn_sac_batch;

typedef struct { double lr, beta1, beta2, eps, max_grad_norm; } bcn_sac_adam_hyper;

/* params: the segments above.  state: counters uint32 [batch], step int32 [8] ([0] critic Adam steps, [1] policy Adam steps, [2] alpha
 * Adam steps, [3] the counter of stream 8, [4] of stream 9, the rest unused), stats float64 [12], adam_m and adam_v real [elements of
 * the parameter buffer].  work (for a minibatch of m rows; all but the last three segments do not depend on m, and it is scratch but
 * for `grad`): grad (the parameter layout), wg_stats, norm2, slabs, rw real [4][m], xa and xb real [m][D].  The slabs must be ZERO
 * before the first use (a new buffer of zeros): the gaps between segments are never written and are read by the reduce launch. */
BCN_SAC_API int bcn_sac_params_layout(const bcn_sac_cfg* cfg, bcn_sac_seg* segs, int max_segs);
BCN_SAC_API size_t bcn_sac_params_bytes(const bcn_sac_cfg* cfg);
BCN_SAC_API int bcn_sac_state_layout(const bcn_sac_cfg* cfg, bcn_sac_seg* segs, int max_segs);
BCN_SAC_API size_t bcn_sac_state_bytes(const bcn_sac_cfg* cfg);
BCN_SAC_API int bcn_sac_work_layout(const bcn_sac_cfg* cfg, int64_t m, bcn_sac_seg* segs, int max_segs);
BCN_SAC_API size_t bcn_sac_work_bytes(const bcn_sac_cfg* cfg, int64_t m);
/* the workgroups of the backward launches at most: min(BCN_SAC_MAX_GRID, max(8, 64 MiB / bytes of one slab)); 0 for a refused cfg */
BCN_SAC_API int bcn_sac_grid(const bcn_sac_cfg* cfg);
/* the dynamic LDS of a tile kernel for this cfg in bytes; 0 for a refused cfg */
BCN_SAC_API size_t bcn_sac_lds_bytes(const bcn_sac_cfg* cfg);

BCN_SAC_API int bcn_sac_act(const bcn_sac_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            void* actions_dev, int mode, uint64_t seed, int64_t replica_offset, void* stream);

BCN_SAC_API int bcn_sac_critic_grad(const bcn_sac_cfg* cfg, const bcn_sac_batch* batch, void* stream);
BCN_SAC_API int bcn_sac_actor_grad(const bcn_sac_cfg* cfg, const bcn_sac_batch* batch, void* stream);
BCN_SAC_API int bcn_sac_adam(const bcn_sac_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, int which,
                             const bcn_sac_adam_hyper* hyper, void* stream);
BCN_SAC_API int bcn_sac_polyak(const bcn_sac_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream);

BCN_SAC_API const char* bcn_sac_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

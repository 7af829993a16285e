/* beacon_td3.h -- C ABI of libbeacon_td3.so: an off-policy learner on the device -- a replay memory, a deterministic policy with
 * one or two critics Q(s, a), and the TD3 / DDPG update (hand-written HIP for gfx950).
 *
 * The library is a unit of its own, like the actor's, the learner's and the epochs': it takes device pointers and sizes only and
 * adds nothing to include/beacon_hip.h, beacon_actor.h, beacon_learner.h or beacon_epochs.h.  Its networks run on the actor's tile
 * with the actor's layer (csrc/actor/policy_net.h, compiled into this library too); what that file lacks is csrc/td3/td3_impl.h.
 * Every launch: no host read, no allocation, no atomics, sums in a fixed order, separate launches as the only synchronisation
 * between workgroups, capturable in a graph, bit-reproducible.
 *
 * Conventions: every function returns 0 (BCN_TD3_OK) or a BCN_TD3_ERR_* code (*_layout: the segment count, 0 on error; *_bytes: the
 * byte count, 0 on error); bcn_td3_last_error() gives text.  Pointers named *_dev are DEVICE pointers; "real" is float for dtype 0
 * and double for dtype 1.  Every argument is checked before a device is touched.
 *
 * ---- Networks ----------------------------------------------------------------------------------------------------------------
 * cfg: 1 .. 3 hidden layers of 1 .. 128 units (the same widths for every network), activation tanh (0) or relu (1), act_dim 1 .. 16,
 * obs_dim >= 1 with D = obs_dim + act_dim <= 512, one scalar bound pair low <= high, n_critics 1 or 2.
 *   policy mu     an MLP obs_dim -> act_dim with a linear head;  a = c + h tanh(head),  c = (high + low) / 2,  h = (high - low) / 2
 *                 (c and h are formed in float64 and rounded once to real)
 *   critics Q_i   MLPs D -> 1 on the row [obs | a], with a linear head
 * Every output of every layer is the fma chain  acc = bias;  acc = fma(W[o][k], x[k], acc)  for k ascending, then the activation:
 * the chain of include/beacon_actor.h.
 * One parameter buffer holds the segments  mu_w0, mu_b0, ... mu_w{L}, mu_b{L}, q1_w0, ... q1_b{L}, (q2_w0, ... q2_b{L})  for L =
 * n_hidden, each 16-byte aligned, matrices [out][in]; q*_w0 is [hidden[0]][D] with the observation columns first.  A target buffer
 * has the same layout.  Fresh buffers are the caller's to fill (zeros are valid parameters).
 *
 * ---- Random streams ----------------------------------------------------------------------------------------------------------
 * All draws are words of the project's one Philox4x32-10 definition under the key (low, high word of seed).  The last counter word
 * names the stream: 0 inlet noise, 1 random-start reset, 2 the actor, 3 the epochs' permutation, and here
 *   4 exploration       counter (replica_offset + b, counters[b], j, 4)
 *   5 replay sampling   counter (i, head[3], 0, 5)
 *   6 target smoothing  counter (i, step[2], j, 6),  i the row of the minibatch
 * A standard normal pair (z_{2j}, z_{2j+1}) comes from the four words at pair index j by the actor's Box-Muller form
 * (include/beacon_actor.h: u1, u2 per dtype; radius = sqrt(-2 ln u1); z_{2j} = radius cos(pi 2u2), z_{2j+1} = radius sin(pi 2u2)).
 * A single uniform u in [0, 1) at index j is bcn_set_noise's: (w0 >> 8) 2^-24 in float32, ((w0 << 21) ^ (w1 >> 11)) 2^-53 in float64.
 *
 * ---- Acting: bcn_td3_act, ONE launch -------------------------------------------------------------------------------------------
 * One workgroup per tile of rows runs mu on obs_dev [batch][obs_dim] and writes actions_dev [batch][act_dim]:
 *   BCN_TD3_DETERMINISTIC  a = mu(s)
 *   BCN_TD3_NOISY          a = clamp(mu(s) + (h sigma) z, low, high), z from stream 4 (h sigma: one product in real)
 *   BCN_TD3_UNIFORM        a = low + (high - low) u, u the single uniform of stream 4 at index j = the action component
 * `counters` (uint32 [batch], the first segment of the state buffer) tick once per stochastic launch (noisy, uniform).  A replica
 * whose mask byte is 0 keeps its action row and its counter.
 *
 * ---- Replay memory -----------------------------------------------------------------------------------------------------------
 * One packed buffer of C = capacity rows (bcn_replay_layout):
 *   head int32 [4]: [0] the write position, [1] the rows stored (<= C), [2] the rows ever appended (it wraps), [3] the samples drawn
 *   obs [C][obs_dim], act [C][act_dim], rwd [C], next_obs [C][obs_dim]: real;  boot uint8 [C], live uint8 [C]
 * bcn_replay_append moves the recorded steps of a rollout (pointers to its segments: obs [T + 1][B][obs_dim], act [T][B][act_dim],
 * rwd [T][B], done, trunc, valid uint8 [T][B], final_obs [T][B][obs_dim], cursor int32) into the ring.  With n = min(max(cursor[0],
 * 0), T) read on the device, transition (t, b), t < n, goes to slot (head[0] + t B + b) mod C:
 *   fin = done | trunc;  next_obs = fin ? final_obs[t][b] : obs[t + 1][b];  boot = (!fin || trunc) ? 1 : 0  (the bootstrap rule of
 *   bcn_rollout_gae);  live = valid[t][b] != 0;  obs, act, rwd copied as they are
 * TWO launches: the copy (every workgroup reads the old head, none writes it), then one lane advances head[0] = (head[0] + n B)
 * mod C, head[1] = min(head[1] + n B, C), head[2] += n B.  T B > C is an argument error.  No compaction: a row with live = 0
 * occupies a slot and weighs nothing.
 * bcn_replay_sample fills idx_dev int32 [m] with replacement: idx[i] = mulhi32(w0, stored) = (w0 stored) >> 32, w0 word 0 of
 * stream 5 at (i, head[3], 0, 5), stored = max(head[1], 1) read on the device; then head[3] += 1.  TWO launches.  A pure function of
 * (m, seed, stored, head[3]).
 *
 * ---- The update --------------------------------------------------------------------------------------------------------------
 * A minibatch is the m rows idx_dev names; w = live (0 or 1), W = max(sum w, 1).  A row with w = 0, or an index outside 0 .. C - 1,
 * is staged as zeros: its fields may hold anything, NaN included.
 * bcn_td3_critic_grad, FOUR launches:
 *   1. next:    per row  a' = clamp(mu_target(s') + h clamp(sigma_target z, -c_noise, c_noise), low, high), z from stream 6; the rows
 *               [s' | a'] and [s | a] and (rwd, boot, w) go to the work buffer
 *   2. critic:  per row  y = rwd + (gamma boot) min_i Q_i,target(s', a')  (no gradient through y);  loss = sum_i sum_rows w (Q_i(s, a) -
 *               y)^2 / W;  the gradient of its numerator for the q segments into per-workgroup slabs: workgroup g of G = min(tiles,
 *               bcn_td3_grid) walks the tiles g, g + G, ... and adds tile after tile, rows ascending inside a tile
 *   3. reduce:  grad[p] = (sum_g slab_g[p]) / W for g ascending, in float64, rounded once; the statistics
 *   4. finish:  stats[critic_grad_norm] = sqrt(sum grad^2) over the q segments, in float64 in a fixed tree
 * bcn_td3_actor_grad, FOUR launches (it reads (w) of the LAST bcn_td3_critic_grad's minibatch: call it behind one, same idx):
 *   1. mu:      a = mu(s) per row; the rows [s | a] go to the work buffer
 *   2. actor:   loss = -sum w Q_1(s, mu(s)) / W.  Q_1 forward with its activations kept; backward down to the ACTION columns of its
 *               first layer's input, dQ/da_j = sum_q W0[q][obs_dim + j] g0[q] for q ascending (g0: the gradient at the first
 *               layer's pre-activation); only that is kept.  mu forward again with its activations kept; the head's gradient is
 *               dQ/da_j h (1 - tanh^2(head_j)); backward down mu into the slabs.  The critic's parameters get no gradient.
 *   3. reduce, 4. finish: as above over the mu segments; stats[policy_loss], stats[policy_grad_norm]
 * bcn_td3_adam, TWO launches: Adam of include/beacon_learner.h (step_size = lr / (1 - beta1^t), m += (1 - beta1)(g - m), v = beta2 v +
 * (1 - beta2) g^2, p -= step_size m / (sqrt(v) / sqrt(1 - beta2^t) + eps), g scaled by min(1, max_grad_norm / (norm + 1e-6)) when
 * max_grad_norm > 0) over the q segments (which = BCN_TD3_OPT_CRITIC) or the mu segments (BCN_TD3_OPT_POLICY), t = step[which] + 1;
 * then one lane ticks step[which], and for the critic also step[2], the smoothing stream's counter.
 * bcn_td3_polyak, ONE launch: target[p] += tau (params[p] - target[p]) over the whole buffer (tau rounded once to real).
 * A TD3 update of one minibatch is sample (2) + critic_grad (4) + adam (2) = 8 launches, and on every policy_delay-th minibatch
 * actor_grad (4) + adam (2) + polyak (1) = 7 more.  Whether the policy step runs is the CALLER's control flow.
 *
 * stats (float64 [8], a segment of the state buffer): critic_loss, q1_mean, q2_mean, target_mean (the W-weighted means of Q_1(s, a),
 * Q_2(s, a) -- 0 with one critic -- and y), policy_loss, W, critic_grad_norm, policy_grad_norm (before clipping).
 */
#ifndef BEACON_TD3_H
#define BEACON_TD3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_TD3_API __attribute__((visibility("default")))
#define BCN_TD3_API_VERSION 1

enum { BCN_TD3_OK = 0, BCN_TD3_ERR_ARG = 1, BCN_TD3_ERR_HIP = 2 };
/* element types of a segment */
enum { BCN_TD3_REAL = 0, BCN_TD3_I32 = 1, BCN_TD3_U32 = 2, BCN_TD3_F64 = 3, BCN_TD3_U8 = 4 };
enum { BCN_TD3_DETERMINISTIC = 0, BCN_TD3_NOISY = 1, BCN_TD3_UNIFORM = 2 };
enum { BCN_TD3_OPT_CRITIC = 0, BCN_TD3_OPT_POLICY = 1 };
enum { BCN_TD3_STAT_CRITIC_LOSS = 0, BCN_TD3_STAT_Q1 = 1, BCN_TD3_STAT_Q2 = 2, BCN_TD3_STAT_TARGET = 3, BCN_TD3_STAT_POLICY_LOSS = 4,
       BCN_TD3_STAT_W = 5, BCN_TD3_STAT_CRITIC_NORM = 6, BCN_TD3_STAT_POLICY_NORM = 7, BCN_TD3_N_STATS = 8 };

#define BCN_TD3_MAX_IN 512        /* obs_dim + act_dim, at most */
#define BCN_TD3_MAX_GRID 128      /* workgroups of the backward launches, at most */
#define BCN_TD3_MAX_SEGS 32

typedef struct {
  int32_t batch;        /* replicas bcn_td3_act serves and the state buffer counts for */
  int32_t obs_dim, act_dim;
  int32_t dtype;        /* 0 float32, 1 float64 */
  int32_t n_hidden, hidden[3];
  int32_t activation;   /* 0 tanh, 1 relu */
  double low, high;
  int32_t n_critics;    /* 1 (DDPG) or 2 (TD3) */
} bcn_td3_cfg;

/* One named segment: row_elems elements of kind `elem` at `offset` bytes (the fields of bcn_actor_seg; planes is 0). */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;
  int32_t planes;
  int64_t row_elems;
} bcn_td3_seg;

typedef struct {
  const void* params_dev;     /* the parameter buffer */
  const void* target_dev;     /* the target buffer (critic_grad) */
  const void* mem_dev;        /* the replay buffer of `capacity` rows */
  const int32_t* idx_dev;     /* int32 [m] */
  void* work_dev;             /* bcn_td3_work_bytes(cfg, m) bytes */
  void* state_dev;            /* bcn_td3_state_bytes(cfg) bytes */
  int64_t m;                  /* rows of the minibatch, 1 .. 2^31 - 1 */
  int64_t capacity;
  double gamma, target_noise, noise_clip;
  uint64_t seed;
} bcn_td3_batch;

typedef struct { double lr, beta1, beta2, eps, max_grad_norm; } bcn_td3_adam_hyper;

/* params: the segments above.  state: counters uint32 [batch], step int32 [4] ([0] critic Adam steps, [1] policy Adam steps, [2] the
 * smoothing draws, [3] unused), stats float64 [8], adam_m and adam_v real [elements of the parameter buffer].  work (for a minibatch
 * of m rows; all but the last three segments do not depend on m, and it is scratch but for `grad`): grad (the parameter layout),
 * wg_stats, norm2, slabs, rw real [3][m], xa and xb real [m][D].  replay: above.  The slabs must be ZERO before the first use (a new
 * buffer of zeros): the gaps between segments are never written and are read by the reduce launch. */
BCN_TD3_API int bcn_td3_params_layout(const bcn_td3_cfg* cfg, bcn_td3_seg* segs, int max_segs);
BCN_TD3_API size_t bcn_td3_params_bytes(const bcn_td3_cfg* cfg);
BCN_TD3_API int bcn_td3_state_layout(const bcn_td3_cfg* cfg, bcn_td3_seg* segs, int max_segs);
BCN_TD3_API size_t bcn_td3_state_bytes(const bcn_td3_cfg* cfg);
BCN_TD3_API int bcn_td3_work_layout(const bcn_td3_cfg* cfg, int64_t m, bcn_td3_seg* segs, int max_segs);
BCN_TD3_API size_t bcn_td3_work_bytes(const bcn_td3_cfg* cfg, int64_t m);
BCN_TD3_API int bcn_replay_layout(const bcn_td3_cfg* cfg, int64_t capacity, bcn_td3_seg* segs, int max_segs);
BCN_TD3_API size_t bcn_replay_bytes(const bcn_td3_cfg* cfg, int64_t capacity);
/* the workgroups of the backward launches at most: min(BCN_TD3_MAX_GRID, max(8, 64 MiB / bytes of one slab)); 0 for a refused cfg */
BCN_TD3_API int bcn_td3_grid(const bcn_td3_cfg* cfg);

BCN_TD3_API int bcn_td3_act(const bcn_td3_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            void* actions_dev, int mode, double sigma, uint64_t seed, int64_t replica_offset, void* stream);

BCN_TD3_API int bcn_replay_append(const bcn_td3_cfg* cfg, int64_t capacity, void* mem_dev, int T, const void* obs_dev, const void* act_dev,
                                  const void* rwd_dev, const uint8_t* done_dev, const uint8_t* trunc_dev, const uint8_t* valid_dev,
                                  const void* final_obs_dev, const int32_t* cursor_dev, void* stream);
BCN_TD3_API int bcn_replay_sample(int64_t m, uint64_t seed, int32_t* head_dev, int32_t* idx_dev, void* stream);

BCN_TD3_API int bcn_td3_critic_grad(const bcn_td3_cfg* cfg, const bcn_td3_batch* batch, void* stream);
BCN_TD3_API int bcn_td3_actor_grad(const bcn_td3_cfg* cfg, const bcn_td3_batch* batch, void* stream);
BCN_TD3_API int bcn_td3_adam(const bcn_td3_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, int which,
                             const bcn_td3_adam_hyper* hyper, void* stream);
BCN_TD3_API int bcn_td3_polyak(const bcn_td3_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream);

BCN_TD3_API const char* bcn_td3_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

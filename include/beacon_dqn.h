/* beacon_dqn.h -- C ABI of libbeacon_dqn.so: a value-based learner for DISCRETE action spaces on the device -- a Q network with one
 * output per action, the max / argmax target (plain and double), dueling heads, the Huber loss, an epsilon-greedy act launch that
 * writes int32 actions, and the append that moves int32 rollout actions into the replay ring (hand-written HIP for gfx950).
 *
 * The library is a unit of its own, like the other six: it takes device pointers and sizes only and adds nothing to their headers.
 * Its network runs on the actor's tile with the actor's layer (csrc/actor/policy_net.h); the slabs, the backward pass of one MLP and
 * the finish, Adam and ring-advance kernels are the templates of csrc/td3/td3_impl.h, instantiated in this library too; what
 * both lack is csrc/dqn/dqn_impl.h.  The replay memory is NOT restated here: it is libbeacon_td3.so's (bcn_replay_layout and
 * bcn_replay_sample of include/beacon_td3.h, laid out with act_dim = 1), and this library receives its segments as separate device
 * pointers plus the capacity.  The ring's act segment [C][1] holds the action index as a real, exactly.
 * Every launch: no host read, no allocation, no atomics, sums in a fixed order (float64 where include/beacon_td3.h uses float64),
 * separate launches as the only synchronisation between workgroups, capturable in a graph, bit-reproducible.
 *
 * Conventions: every function returns 0 (BCN_DQN_OK) or a BCN_DQN_ERR_* code (*_layout: the segment count, 0 on error; *_bytes: the
 * byte count, 0 on error); bcn_dqn_last_error() gives text.  Pointers named *_dev are DEVICE pointers; "real" is float for dtype 0
 * and double for dtype 1.  Every argument is checked before a device is touched.
 *
 * ---- The network ---------------------------------------------------------------------------------------------------------------
 * cfg: 1 .. 3 hidden layers of 1 .. 128 units, activation tanh (0) or relu (1), obs_dim 1 .. 512, n = n_actions in 2 .. 16, dueling 0
 * or 1 with n + dueling <= 16: the head is ONE matrix of R = n + dueling rows and stays within the tile's 16-row head buffer.
 * Every output of every layer is the fma chain  acc = bias;  acc = fma(W[o][k], x[k], acc)  for k ascending, then the activation: the
 * chain of include/beacon_actor.h.  One parameter buffer holds the segments  q_w0, q_b0, ... q_w{L}, q_b{L}  for L = n_hidden, each
 * 16-byte aligned, matrices [out][in]; q_w{L} is [R][h_last].  A target buffer has the same layout.
 *   plain head     Q_j = head_j,  j < n
 *   dueling head   A_j = head_j for j < n, V = head_n (the LAST row);  Q_j = (V + A_j) - (sum_k A_k) / n, the sum taken for k
 *                  ascending from 0, the quotient formed once per row
 *   argmax         the FIRST maximum: best = -inf, arg = 0; for j ascending, Q_j replaces best only where Q_j > best strictly.  A NaN
 *                  never wins (no comparison with it is true).  max_j Q_j is Q_arg.
 * LDS of the tile kernels, the sum of csrc/td3/td3_impl.h with wcols = pad4(max(hmax, R)) + 4: 160 256 bytes in float32 and 158 336 in
 * float64 at 3 x 128, of BCN_DQN_LDS_LIMIT = 163 840.  bcn_dqn_lds_bytes(cfg) returns the sum; a cfg whose sum exceeded the limit
 * would be refused by every function here before any launch.
 *
 * ---- Random stream -------------------------------------------------------------------------------------------------------------
 * All draws are words of the project's one Philox4x32-10 definition under the key (low, high word of seed).  The last counter word
 * names the stream: 0 .. 9 are taken (include/beacon_td3.h and include/beacon_sac.h list them; 5 is replay sampling), and here
 *   10 acting    counter (replica_offset + b, counters[b], 0, 10), words w[0 .. 3]
 *   u   = the single uniform of include/beacon_td3.h from (w[0], w[1]):  (w0 >> 8) 2^-24 in float32, ((w0 << 21) ^ (w1 >> 11)) 2^-53 in
 *         float64; u in [0, 1)
 *   rnd = mulhi32(w[3], n) = (w3 n) >> 32, an action in 0 .. n - 1
 *
 * ---- Acting: bcn_dqn_act, ONE launch -------------------------------------------------------------------------------------------
 * One workgroup per tile of rows runs Q on obs_dev [batch][obs_dim] and writes actions_dev int32 [batch]:
 *   BCN_DQN_GREEDY   a = argmax_j Q_j
 *   BCN_DQN_EPSILON  a = rnd where u < eps, else argmax_j Q_j.  eps = 0 is greedy, eps = 1 is uniform.
 *   BCN_DQN_UNIFORM  a = rnd  (Q is not evaluated)
 * eps is `eps`, or, where eps_dev is not NULL, the one real eps_dev points to, read on the device: the pointer wins.
 * `counters` (uint32 [batch], the first segment of the state buffer) tick once per stochastic launch (epsilon, uniform).  A replica
 * whose mask byte is 0 keeps its action and its counter.
 * bcn_dqn_q, ONE launch: q_dev [n_rows][n] = Q of rows_dev [n_rows][obs_dim], the values the act launch takes its argmax of.
 *
 * ---- Append: bcn_dqn_append, TWO launches --------------------------------------------------------------------------------------
 * bcn_replay_append of include/beacon_td3.h for a rollout whose act segment is int32 [T][B]: the same slots, wrap, next_obs, boot and
 * live, the cursor read on the device, the copy launch and then one lane that advances head; the action is stored as (real)a.  The
 * ring is given by its segments: head int32 [4], obs [C][obs_dim], act [C][1], rwd [C], next_obs [C][obs_dim], boot, live uint8 [C].
 * T B > C is an argument error.
 *
 * ---- The update --------------------------------------------------------------------------------------------------------------
 * A minibatch is the m rows idx_dev names; w = live (0 or 1), W = max(sum w, 1).  A row with w = 0, an index outside 0 .. C - 1, or a
 * stored action that is no integer in 0 .. n - 1 is DEAD: it is staged as zeros and gets w = 0; its fields may hold anything, NaN
 * included.  It is never an out-of-range head index.
 * bcn_dqn_grad, THREE launches:
 *   1. q:       workgroup g of G = min(tiles, bcn_dqn_grid) walks the tiles g, g + G, ...; per tile, with a the stored action,
 *                 double_q:  j* = argmax_j Q_j(s'; params);  y = rwd + (gamma boot) Q_{j*}(s'; target)
 *                 else:      y = rwd + (gamma boot) max_j Q_j(s'; target)                   (no gradient through y)
 *                 delta = Q_a(s; params) - y
 *                 huber <= 0 (MSE):  row loss = delta^2 / 2;                                       g = w delta
 *                 kappa = huber > 0: row loss = |delta| <= kappa ? delta^2 / 2 : kappa (|delta| - kappa / 2);  g = w clamp(delta, -kappa, kappa)
 *                 loss = sum w (row loss) / W
 *               the gradient at the head: plain  g at row a, 0 elsewhere;  dueling  g ((j == a ? 1 : 0) - 1 / n) at A_j and g at V (1 / n
 *               formed once in real); then the backward pass of the network into the workgroup's slab, tile after tile, rows
 *               ascending inside a tile
 *   2. reduce:  grad[p] = (sum_g slab_g[p]) / W for g ascending, in float64, rounded once; the statistics
 *   3. finish:  stats[grad_norm] = sqrt(sum grad^2), in float64 in a fixed tree
 * bcn_dqn_adam, TWO launches: Adam of include/beacon_learner.h, the arithmetic of bcn_td3_adam, over all segments, t = step[0] + 1;
 * then one lane ticks step[0].
 * bcn_dqn_polyak, ONE launch: target[p] += tau (params[p] - target[p]) over the whole buffer (tau rounded once to real); tau = 1 is
 * the hard copy, target[p] = params[p] exactly (t + (p - t) rounds twice and need not give p back, so that case is a branch).
 * One DQN minibatch is sample (2, libbeacon_td3.so) + grad (3) + adam (2) + polyak (1) = 8 launches, 7 without the target step.
 * Whether the target step runs is the CALLER's control flow.
 *
 * stats (float64 [8], a segment of the state buffer): loss, q_mean (the W-weighted mean of Q_a(s)), target_mean (of y), td_abs_mean (of
 * |delta|), W, grad_norm (before clipping), q_max_mean (of max_j Q_j(s)), and one spare word (0).
 */
#ifndef BEACON_DQN_H
#define BEACON_DQN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_DQN_API __attribute__((visibility("default")))
#define BCN_DQN_API_VERSION 1

enum { BCN_DQN_OK = 0, BCN_DQN_ERR_ARG = 1, BCN_DQN_ERR_HIP = 2 };
/* element types of a segment */
enum { BCN_DQN_REAL = 0, BCN_DQN_I32 = 1, BCN_DQN_U32 = 2, BCN_DQN_F64 = 3, BCN_DQN_U8 = 4 };
enum { BCN_DQN_GREEDY = 0, BCN_DQN_EPSILON = 1, BCN_DQN_UNIFORM = 2 };
enum { BCN_DQN_STAT_LOSS = 0, BCN_DQN_STAT_Q_MEAN = 1, BCN_DQN_STAT_TARGET_MEAN = 2, BCN_DQN_STAT_TD_ABS_MEAN = 3, BCN_DQN_STAT_W = 4,
       BCN_DQN_STAT_GRAD_NORM = 5, BCN_DQN_STAT_Q_MAX_MEAN = 6, BCN_DQN_STAT_SPARE = 7, BCN_DQN_N_STATS = 8 };

#define BCN_DQN_MAX_OBS 512       /* obs_dim, at most */
#define BCN_DQN_MAX_ACTIONS 16    /* n_actions + dueling, at most */
#define BCN_DQN_MAX_GRID 128      /* workgroups of the backward launch, at most */
#define BCN_DQN_MAX_SEGS 16
#define BCN_DQN_LDS_LIMIT 163840  /* bytes of dynamic LDS a tile kernel may ask for */

typedef struct {
  int32_t batch;        /* replicas bcn_dqn_act serves and the state buffer counts for */
  int32_t obs_dim, n_actions;
  int32_t dtype;        /* 0 float32, 1 float64 */
  int32_t n_hidden, hidden[3];
  int32_t activation;   /* 0 tanh, 1 relu */
  int32_t dueling;      /* 0 or 1 */
} bcn_dqn_cfg;

/* One named segment: row_elems elements of kind `elem` at `offset` bytes (the fields of bcn_td3_seg; planes is 0). */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;
  int32_t planes;
  int64_t row_elems;
} bcn_dqn_seg;

typedef struct {
  const void* params_dev;     /* the parameter buffer */
  const void* target_dev;     /* the target buffer */
  const void* obs_dev;        /* the replay memory's segments, `capacity` rows each: real [C][obs_dim] */
  const void* act_dev;        /* real [C][1]: the action index */
  const void* rwd_dev;        /* real [C] */
  const void* next_obs_dev;   /* real [C][obs_dim] */
  const uint8_t* boot_dev;    /* uint8 [C] */
  const uint8_t* live_dev;    /* uint8 [C] */
  const int32_t* idx_dev;     /* int32 [m] */
  void* work_dev;             /* bcn_dqn_work_bytes(cfg) bytes */
  void* state_dev;            /* bcn_dqn_state_bytes(cfg) bytes */
  int64_t m;                  /* rows of the minibatch, 1 .. 2^31 - 1 */
  int64_t capacity;
  double gamma;
  double huber;               /* kappa > 0, or <= 0 for the squared loss */
  int32_t double_q;           /* 0 or 1 */
  int32_t reserved;           /* 0 */
} bcn_dqn_batch;

typedef struct { double lr, beta1, beta2, eps, max_grad_norm; } bcn_dqn_adam_hyper;

/* params: the segments above.  state: counters uint32 [batch], step int32 [4] ([0] Adam steps, the rest unused), stats float64 [8],
 * adam_m and adam_v real [elements of the parameter buffer].  work (no segment depends on m; scratch but for `grad`): grad (the
 * parameter layout), wg_stats, norm2, slabs.  The slabs must be ZERO before the first use (a new buffer of zeros): the gaps between
 * segments are never written and are read by the reduce launch. */
BCN_DQN_API int bcn_dqn_params_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs);
BCN_DQN_API size_t bcn_dqn_params_bytes(const bcn_dqn_cfg* cfg);
BCN_DQN_API int bcn_dqn_state_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs);
BCN_DQN_API size_t bcn_dqn_state_bytes(const bcn_dqn_cfg* cfg);
BCN_DQN_API int bcn_dqn_work_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs);
BCN_DQN_API size_t bcn_dqn_work_bytes(const bcn_dqn_cfg* cfg);
/* the workgroups of the backward launch at most: min(BCN_DQN_MAX_GRID, max(8, 64 MiB / bytes of one slab)); 0 for a refused cfg */
BCN_DQN_API int bcn_dqn_grid(const bcn_dqn_cfg* cfg);
/* the dynamic LDS of a tile kernel for this cfg in bytes; 0 for a refused cfg */
BCN_DQN_API size_t bcn_dqn_lds_bytes(const bcn_dqn_cfg* cfg);

BCN_DQN_API int bcn_dqn_act(const bcn_dqn_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            int32_t* actions_dev, int mode, double eps, const void* eps_dev, uint64_t seed, int64_t replica_offset,
                            void* stream);
BCN_DQN_API int bcn_dqn_q(const bcn_dqn_cfg* cfg, const void* params_dev, const void* rows_dev, int64_t n_rows, void* q_dev, void* stream);

BCN_DQN_API int bcn_dqn_append(const bcn_dqn_cfg* cfg, int64_t capacity, int32_t* head_dev, void* obs_dev, void* act_dev, void* rwd_dev,
                               void* next_obs_dev, uint8_t* boot_dev, uint8_t* live_dev, int T, const void* ro_obs_dev,
                               const int32_t* ro_act_dev, const void* ro_rwd_dev, const uint8_t* ro_done_dev, const uint8_t* ro_trunc_dev,
                               const uint8_t* ro_valid_dev, const void* ro_final_obs_dev, const int32_t* ro_cursor_dev, void* stream);

BCN_DQN_API int bcn_dqn_grad(const bcn_dqn_cfg* cfg, const bcn_dqn_batch* batch, void* stream);
BCN_DQN_API int bcn_dqn_adam(const bcn_dqn_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, const bcn_dqn_adam_hyper* hyper,
                             void* stream);
BCN_DQN_API int bcn_dqn_polyak(const bcn_dqn_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream);

BCN_DQN_API const char* bcn_dqn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

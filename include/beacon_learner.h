/* beacon_learner.h -- C ABI of libbeacon_learner.so: the PPO update of an on-device actor (hand-written HIP for gfx950).
 *
 * bcn_learner_grad computes the PPO clipped-surrogate loss of a minibatch and its gradient with respect to every parameter of
 * an actor (include/beacon_actor.h: the parameter buffer of bcn_actor_params_layout); bcn_learner_step applies Adam to that
 * parameter buffer in place.  Five launches per minibatch in all, no host read, no allocation, no atomics: every buffer is
 * bit-reproducible run to run and both calls can be captured in a graph.  The library is a unit of its own, like the actor's: it
 * takes device pointers and sizes only and adds nothing to include/beacon_hip.h or include/beacon_actor.h.
 *
 * Conventions: those of beacon_actor.h.  Every function returns 0 (BCN_LEARNER_OK) or a BCN_LEARNER_ERR_* code (the *_layout /
 * *_bytes functions: the segment count / the byte count, 0 on a bad argument); bcn_learner_last_error() gives text.  Pointers
 * named *_dev are DEVICE pointers; "real" is float for dtype 0 and double for dtype 1.  The cfg is the actor's, and the checks of
 * a cfg are the actor's; cfg->batch is not used.  Every argument is checked before a device is touched.
 *
 * ---- The loss -------------------------------------------------------------------------------------------------------------
 * A minibatch is m rows.  Row i has an observation row, the action taken (Gaussian kind: the UNCLIPPED sample, `raw` of the
 * actor; categorical kind: the int32 class), logp_old, adv, ret and a weight w_i >= 0 (no weight array: w_i = 1).  With
 * W = max(sum_i w_i, 1):
 *
 *   L = (1 / W) sum_i w_i [ pg_i + vf_coef v_i - ent_coef H_i ]
 *
 * Forward: the two MLPs of bcn_actor_act on the row, the same layer definition (every output the fma chain for k ascending;
 *   tanh or max(., 0) on the hidden layers, linear heads).
 * Gaussian:     z_k = (a_k - mean_k) exp(-log_std_k);  logp = sum_k (-1/2 z_k^2 - log_std_k - 1/2 ln 2 pi);
 *               H = sum_k (log_std_k + 1/2 ln 2 pi e)
 * Categorical:  d = the log-softmax of the logits as the actor forms it ((l_k - max l) - ln sum exp(l - max l));
 *               logp = d[a];  H = -sum_k exp(d_k) d_k
 * Surrogate:    ratio = exp(logp - logp_old);  pg = -min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv)
 * Value:        v = (value - ret)^2
 * Diagnostics:  approx_kl = (ratio - 1) - ln ratio (= (ratio - 1) - (logp - logp_old));  clip_frac = [ |ratio - 1| > clip ]
 *
 * ---- The gradient ---------------------------------------------------------------------------------------------------------
 * dL / d theta for every segment of bcn_actor_params_layout, log_std included, in a buffer of the same layout.  Per row, with
 * c = w (the division by W comes last):
 *   g = d pg / d logp = -ratio adv  where ratio adv <= clamp(ratio, 1 - clip, 1 + clip) adv (the unclipped branch is the minimum:
 *       inside the clip range both are the same number), else 0
 *   Gaussian:     d L / d mean_k = c g z_k exp(-log_std_k);   d L / d log_std_k = c (g (z_k^2 - 1) - ent_coef)
 *   Categorical:  d L / d l_k = c (g ([k = a] - p_k) + ent_coef p_k (d_k + H)),  p_k = exp(d_k)
 *   Value head:   d L / d value = c vf_coef 2 (value - ret)
 * and from the heads down by the chain rule: for a layer y = W x + b with the gradient D at y, dW[o][k] = sum_rows D[o] x[k],
 * db[o] = sum_rows D[o], and the gradient at x is (sum_o W[o][k] D[o]) f'(x) with f' = 1 - x^2 for tanh and [x > 0] for relu, x
 * being the layer's OUTPUT (relu: x > 0 exactly where its input is > 0; the derivative at an input <= 0 is 0, the framework's
 * convention).  Products and sums over the rows of a tile and over tiles are in the buffer's precision; the sum over workgroups
 * and the division by W are in float64, rounded once; the statistics and W are summed in float64.
 *
 * ---- Rows -----------------------------------------------------------------------------------------------------------------
 * Row i of the minibatch is row s = idx_dev[i] (int32; idx_dev = NULL: s = i) of EVERY per-row array: obs_dev [n_rows][obs_dim],
 * act_dev (real [n_rows][act_dim] or int32 [n_rows]), logp_old_dev, adv_dev, ret_dev (real [n_rows]) and weight_dev (uint8 or
 * real [n_rows] by weight_kind).  A row is INACTIVE -- weight 0 -- when its weight is 0 (or not > 0: a NaN weight), when s is
 * outside 0 .. n_rows - 1, when its categorical class is outside 0 .. act_dim - 1, or, with cursor_dev != NULL, when
 * s >= min(max(cursor_dev[0], 0) rows_per_step, n_rows): the rows of steps that a rollout has not recorded, decided on the
 * device.  Of an inactive row only idx and the weight (and the class) are read; its observation, adv, ret and logp_old may hold
 * anything, NaN included: it is staged as zeros and adds +0 to every sum.  Rows behind m stage as zeros too.  Nothing is read
 * past a row or past an array.
 * With rows_per_weight = R > 1 the weight of source row s is weight_dev[s / R] and weight_dev holds n_rows / R elements: the
 * per-agent rows of an actor with cfg.agents = R under the per-replica `valid` bytes of a rollout.  Every other array, idx_dev,
 * the cursor rule and rows_per_step count ROWS as before.  R = 0 or 1: nothing changes.
 *
 * ---- Launches -------------------------------------------------------------------------------------------------------------
 * bcn_learner_grad, three launches in stream order:
 *  1. backward: a FIXED grid of G = min(bcn_learner_grid(cfg), tiles) workgroups of 256 lanes; a tile is 64 rows (float32) or 32
 *     (float64); workgroup g walks the tiles g, g + G, g + 2 G, ... in that order.  Per tile and network: the forward pass
 *     with every layer's activations kept in LDS, the head's gradient, then layer by layer downwards dW and db -- added to
 *     the workgroup's own slab of the work buffer (a plain read-modify-write by the one lane that owns the entry; the first tile
 *     stores) -- and the gradient at the layer's input, in place over the activations.  No input gradient for the first layer,
 *     whose inputs are staged again per slab of 64 (32) columns.
 *  2. reduce: one lane per parameter adds the G slabs for g ascending, divides by W (the sum of the G partial weights for g
 *     ascending), writes grad_dev and a per-block partial of the squared norm; block 0 writes stats[0 .. 6].
 *  3. finish: one workgroup adds the partials in a fixed order and writes stats[7].
 * bcn_learner_step, two launches: Adam (one lane per parameter) and the tick of the step counter (one lane).
 * Separate launches in stream order are the only synchronisation between workgroups: no tickets, flags or waits.
 *
 * ---- Adam -----------------------------------------------------------------------------------------------------------------
 * torch.optim.Adam without weight decay and without amsgrad, on the gradient clipped to a global norm, in the buffer's precision:
 *   s = min(1, max_grad_norm / (stats[7] + 1e-6)) (1 for max_grad_norm <= 0);  g' = s g;  t = step + 1
 *   m = m + (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2
 *   theta = theta - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * The gradient buffer keeps the unclipped gradient.  The step counter lives in the optimiser buffer and advances ON THE DEVICE:
 * a captured step keeps counting at replay.  lr, the betas, eps and max_grad_norm are arguments of the launch: a captured graph
 * keeps the values it was recorded with.
 *
 * ---- The KL stop rule and the learning-rate schedule (fields appended to bcn_learner_adam) -----------------------------------
 * Both are decided ON THE DEVICE, from words the launches before left, so they keep working when a captured update is replayed.
 * The optimiser buffer's step segment, int32 [4], holds: [0] the Adam steps taken, [1] the permutations drawn (the epoch word of
 * bcn_epochs_permute, include/beacon_epochs.h), [2] the stop flag, [3] the steps the stop rule skipped.
 * target_kl > 0: with P = (step[2] != 0) || (stats[approx_kl] > 1.5 target_kl) -- evaluated by every Adam lane and by the tick from
 *   the same words, which nothing writes during the Adam launch --
 *     P true:   Adam touches neither params nor m nor v; the tick sets step[2] = 1 and step[3] += 1 and leaves step[0] alone
 *     P false:  the step above; step[0] += 1
 *   A NaN approx_kl does not stop (the comparison is false).  This is the target_kl rule of the common PPO implementations: the
 *   minibatch whose approx_kl exceeds 1.5 times the target is not applied, and neither is any later one of the update -- their
 *   bcn_learner_grad launches still run, there being no host decision, and move nothing.  bcn_epochs_begin clears the flag at the
 *   head of the next update.  target_kl <= 0: step[2] and step[3] are neither read nor written.
 * lr_steps > 0: the step uses lr_t = lr + (lr_end - lr) min(step[0], lr_steps) / lr_steps, in float64 from the device counter: a
 *   skipped step does not advance it, and behind lr_steps steps the rate is lr_end.  lr_steps <= 0: lr.
 */
#ifndef BEACON_LEARNER_H
#define BEACON_LEARNER_H

#include "beacon_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_LEARNER_API __attribute__((visibility("default")))
#define BCN_LEARNER_API_VERSION 1

enum { BCN_LEARNER_OK = 0, BCN_LEARNER_ERR_ARG = 1, BCN_LEARNER_ERR_HIP = 2 };
/* a fourth element type beside BCN_ACTOR_REAL / _I32 / _U32 */
enum { BCN_LEARNER_F64 = 3 };
enum { BCN_LEARNER_W_NONE = 0, BCN_LEARNER_W_U8 = 1, BCN_LEARNER_W_REAL = 2 };
/* the entries of the stats segment (float64) */
enum { BCN_LEARNER_STAT_LOSS = 0, BCN_LEARNER_STAT_PG = 1, BCN_LEARNER_STAT_VF = 2, BCN_LEARNER_STAT_ENTROPY = 3, BCN_LEARNER_STAT_KL = 4,
       BCN_LEARNER_STAT_CLIP_FRAC = 5, BCN_LEARNER_STAT_W = 6, BCN_LEARNER_STAT_GRAD_NORM = 7, BCN_LEARNER_N_STATS = 8 };

#define BCN_LEARNER_MAX_GRID 256   /* workgroups of the backward launch, at most */

typedef struct {
  const void* obs_dev;       /* real [n_rows][obs_dim] */
  const void* act_dev;       /* Gaussian: real [n_rows][act_dim], the unclipped samples; categorical: int32 [n_rows] */
  const void* logp_old_dev;  /* real [n_rows] */
  const void* adv_dev;       /* real [n_rows] */
  const void* ret_dev;       /* real [n_rows] */
  const void* weight_dev;    /* uint8 or real [n_rows / rows_per_weight] by weight_kind; ignored (may be NULL) for BCN_LEARNER_W_NONE */
  const int32_t* idx_dev;    /* int32 [m] row numbers, or NULL: rows 0 .. m - 1 (then m <= n_rows) */
  const int32_t* cursor_dev; /* int32, the `cursor` segment of a rollout buffer, or NULL */
  int64_t n_rows;            /* rows of every per-row array, >= 1 */
  int64_t m;                 /* rows of the minibatch, 1 .. 2^31 - 1 */
  int32_t weight_kind;       /* BCN_LEARNER_W_* */
  int32_t rows_per_step;     /* with cursor_dev: rows per recorded step (the rollout's batch; with agents: batch x agents), >= 1 */
  int32_t rows_per_weight;   /* APPENDED (a batch that ends at rows_per_step, zero-filled behind it, means what it meant): consecutive
                              * rows that share one weight, >= 0; 0 means 1.  It divides n_rows */
} bcn_learner_batch;

typedef struct {
  double clip;      /* >= 0 */
  double vf_coef;
  double ent_coef;
} bcn_learner_loss;

typedef struct {
  double lr, beta1, beta2, eps;   /* betas in [0, 1) */
  double max_grad_norm;           /* <= 0: no clipping */
  /* APPENDED (an adam that ends at max_grad_norm, zero-filled behind it, means what it meant): the stop rule and the schedule above.
   * All three finite.  With all three 0 nothing new is read or written and the step is the one of version 1, bit for bit. */
  double target_kl;               /* > 0: the KL stop rule; <= 0: none, step[2] and step[3] are neither read nor written */
  double lr_end, lr_steps;        /* lr_steps > 0: the learning rate goes linearly from lr to lr_end over lr_steps steps taken */
} bcn_learner_adam;

/* The gradient buffer: the segments of bcn_actor_params_layout, name for name and offset for offset. */
BCN_LEARNER_API int bcn_learner_grad_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs);
BCN_LEARNER_API size_t bcn_learner_grad_bytes(const bcn_actor_cfg* cfg);

/* The optimiser buffer, three segments (planes = 0):
 *   m, v   real [bcn_learner_grad_bytes / sizeof(real)]: the moments, element for element as the parameter buffer
 *   step   int32 [4]: [0] the Adam steps taken, [1] the permutations drawn, [2] the KL stop flag, [3] the steps it skipped (above)
 * A zeroed buffer is a fresh optimiser. */
BCN_LEARNER_API int bcn_learner_opt_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs);
BCN_LEARNER_API size_t bcn_learner_opt_bytes(const bcn_actor_cfg* cfg);

/* The work buffer, four segments (planes = 0); only `stats` is for the caller:
 *   stats    float64 [8]: loss, pg loss, value loss, entropy, approx_kl, clip_frac (each the weighted mean over the minibatch), W,
 *            and the gradient's 2-norm before clipping
 *   wg_stats float64 [grid][8]  the workgroups' partial sums
 *   norm2    float64 [blocks of the reduce launch]
 *   slabs    real [grid][bcn_learner_grad_bytes / sizeof(real)]
 * It needs no initialisation. */
BCN_LEARNER_API int bcn_learner_work_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs);
BCN_LEARNER_API size_t bcn_learner_work_bytes(const bcn_actor_cfg* cfg);

/* The fixed grid of the backward launch: min(256, max(8, 64 MiB / bcn_learner_grad_bytes)), a function of the cfg alone; 0 on a bad
 * cfg.  (A slab is a whole gradient; at the widest networks, 2 x 10^5 parameters, 256 of them would be 200 MB.) */
BCN_LEARNER_API int bcn_learner_grid(const bcn_actor_cfg* cfg);

/* Loss, statistics and gradient of one minibatch (above).  params_dev is read only. */
BCN_LEARNER_API int bcn_learner_grad(const bcn_actor_cfg* cfg, const void* params_dev, const bcn_learner_batch* batch,
                                     const bcn_learner_loss* loss, void* grad_dev, void* work_dev, void* stream);

/* One Adam step on params_dev in place from grad_dev and the norm in the work buffer's stats[7] (above). */
BCN_LEARNER_API int bcn_learner_step(const bcn_actor_cfg* cfg, void* params_dev, const void* grad_dev, void* opt_dev, const void* work_dev,
                                     const bcn_learner_adam* adam, void* stream);

BCN_LEARNER_API const char* bcn_learner_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

/* beacon_actor.h -- C ABI of libbeacon_actor.so: the on-device actor of a rollout (hand-written HIP for gfx950).
 *
 * ONE launch reads the observation rows a step left, evaluates a policy MLP and a value MLP, draws the action from the
 * project's Philox stream and writes action, log-probability and value -- under a rollout, also into the slot the rollout's
 * device cursor names.  The library is a unit of its own: it takes no bcn_env_t, only device pointers and sizes, and adds
 * nothing to include/beacon_hip.h.
 *
 * Conventions: every function returns 0 (BCN_ACTOR_OK) or a BCN_ACTOR_ERR_* code (the *_layout / *_bytes functions: the segment
 * count / the byte count, 0 on a bad argument); bcn_actor_last_error() gives text.  Pointers named *_dev are DEVICE pointers;
 * "real" is float for dtype 0 and double for dtype 1 (the values of BCN_F32 / BCN_F64 of beacon_hip.h); `stream` is a hipStream_t
 * passed as void*.  The layout functions touch no device and need none.
 */
#ifndef BEACON_ACTOR_H
#define BEACON_ACTOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_ACTOR_API __attribute__((visibility("default")))
#define BCN_ACTOR_API_VERSION 1

enum { BCN_ACTOR_OK = 0, BCN_ACTOR_ERR_ARG = 1, BCN_ACTOR_ERR_HIP = 2 };
enum { BCN_ACTOR_TANH = 0, BCN_ACTOR_RELU = 1 };
enum { BCN_ACTOR_GAUSSIAN = 0, BCN_ACTOR_CATEGORICAL = 1 };
/* element types of a segment (the numbers of BCN_SNAP_REAL / _I32 / _U32 of beacon_hip.h) */
enum { BCN_ACTOR_REAL = 0, BCN_ACTOR_I32 = 1, BCN_ACTOR_U32 = 2 };

#define BCN_ACTOR_MAX_OBS 512
#define BCN_ACTOR_MAX_HIDDEN 128
#define BCN_ACTOR_MAX_LAYERS 3
#define BCN_ACTOR_MAX_ACT 16
#define BCN_ACTOR_MAX_SEGS 20      /* no layout has more segments than this */

typedef struct {
  int32_t batch;        /* replicas B >= 1 */
  int32_t obs_dim;      /* 1 .. 512 */
  int32_t dtype;        /* 0 float32, 1 float64 */
  int32_t n_hidden;     /* 1 .. 3 hidden layers, the same widths in both networks */
  int32_t hidden[3];    /* each 1 .. 128 (entries behind n_hidden are ignored) */
  int32_t activation;   /* BCN_ACTOR_TANH / BCN_ACTOR_RELU */
  int32_t kind;         /* BCN_ACTOR_GAUSSIAN / BCN_ACTOR_CATEGORICAL */
  int32_t act_dim;      /* Gaussian: 1 .. 16 components; categorical: 2 .. 16 classes */
  double low, high;     /* the Box bound of a Gaussian action, low <= high (ignored by the categorical kind) */
  int32_t agents;       /* APPENDED (a cfg that ends at `high`, zero-filled behind it, means what it meant): rows per replica, >= 0;
                         * 0 means 1.  With agents = A > 1 the rows are the agents of B / A replicas, row b = agent b % A of
                         * replica b / A (shkadov's jets under one shared policy): `batch` stays the number of ROWS, a multiple of A */
} bcn_actor_cfg;

/* One named segment of a packed buffer: planes arrays of [rows][row_elems] elements of kind `elem` at `offset` bytes, one behind the
 * other; planes = 0: ONE array of row_elems elements that does not scale with the batch.  Every offset is a multiple of 16. */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;         /* BCN_ACTOR_REAL / _I32 / _U32 */
  int32_t planes;
  int64_t row_elems;
} bcn_actor_seg;

/* The parameter buffer: ONE device buffer of reals holds both networks.  With L = n_hidden, d_0 = obs_dim, d_l = hidden[l - 1] and
 * the head widths d_pi = act_dim, d_vf = 1, its segments are, in this order (planes = 0 for all):
 *   pi_w0 [d_1][d_0], pi_b0 [d_1], ... pi_w{L-1}, pi_b{L-1}, pi_w{L} [act_dim][d_L], pi_b{L} [act_dim]      the policy network
 *   vf_w0, vf_b0, ... vf_w{L} [1][d_L], vf_b{L} [1]                                                        the value network
 *   log_std [act_dim]                                                   Gaussian kind only (row_elems = 0 for the categorical kind)
 * Each matrix is [out][in] row-major (the framework's Linear.weight), followed by its bias.  4 (L + 1) + 1 segments.
 * Writes the first max_segs into segs (segs may be NULL) and returns their number; 0 and bcn_actor_last_error on a bad cfg. */
BCN_ACTOR_API int bcn_actor_params_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs);
BCN_ACTOR_API size_t bcn_actor_params_bytes(const bcn_actor_cfg* cfg);

/* The state buffer: the replicas' draw counters and the outputs of a launch, six segments (planes = 1, rows = batch):
 *   counters uint32 [B]          stochastic launches that wrote the replica since the buffer was zeroed
 *   actions  real [B][act_dim]   Gaussian: the clipped sample; categorical: int32 [B], the class -- what the env's step takes
 *   raw      real [B][act_dim]   Gaussian: the unclipped sample; categorical: the logits (the policy head's outputs)
 *   logp     real [B]
 *   value    real [B]
 *   dist     real [B][act_dim]   Gaussian: the mean (the policy head's outputs); categorical: the log-probabilities */
BCN_ACTOR_API int bcn_actor_state_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs);
BCN_ACTOR_API size_t bcn_actor_state_bytes(const bcn_actor_cfg* cfg);

/* The sequence buffer of a rollout of T >= 1 steps, three segments (planes = T, rows = batch):
 *   logp_seq real [T][B], value_seq real [T][B], raw_seq real [T][B][act_dim] */
BCN_ACTOR_API int bcn_actor_seq_layout(const bcn_actor_cfg* cfg, int T, bcn_actor_seg* segs, int max_segs);
BCN_ACTOR_API size_t bcn_actor_seq_bytes(const bcn_actor_cfg* cfg, int T);

/* ONE launch on `stream`: both networks on every row of obs_dev [B][obs_dim], the draw, the outputs into state_dev.
 *
 * The networks.  A hidden layer is h = act(W x + b), the heads are linear.  Every output is the fma chain
 *   y = b; y = fma(W[o][k], x[k], y) for k = 0, 1, ... in - 1
 * in the buffer's precision, one rounding per step; tanh / max(., 0) follow.  (A float64 dot product in another order differs
 * by the usual summation-order bound only.)
 *
 * The stream.  key = (low, high 32-bit word of `seed`); (w0, w1, w2, w3) = Philox4x32-10(counter = (replica_offset + b, the
 * replica's draw counter, j, 2), key).  Word 0 of the counter is (replica_offset + b) mod 2^32: the global index wraps, as the
 * 32-bit draw counter does.  Word 3 of the counter is 0 for the inlet noise of bcn_set_noise and 1 for the warm-up count
 * of bcn_shkadov_reset_random, so an actor may share its env's seed.
 *
 * Gaussian, deterministic = 0.  mean = the policy head.  For the pair j = 0, 1, ... of components (2j, 2j + 1):
 *   float32: u1 = ((w0 >> 8) + 0.5) 2^-24 in (0, 1), u2 = (w1 >> 8) 2^-24 in [0, 1)
 *   float64: with r1 = (w0 << 21) ^ (w1 >> 11) and r2 = (w2 << 21) ^ (w3 >> 11), the 53-bit forms of bcn_set_noise:
 *            u1 = (r1 + 0.5) 2^-53 (the sum rounded to nearest even: never 0, 1 for r1 = 2^53 - 1), u2 = r2 2^-53
 *   Box-Muller: radius = sqrt(-2 ln u1), angle = 2 pi u2, z_2j = radius cos(angle), z_2j+1 = radius sin(angle); for an odd act_dim
 *   the last pair's second half is not used.
 *   raw_i = mean_i + exp(log_std_i) z_i;  actions_i = min(max(raw_i, low), high);
 *   logp = sum_i (-1/2 z_i^2 - log_std_i - 1/2 ln 2 pi), summed for i ascending: the density of the UNCLIPPED sample.
 * Categorical, deterministic = 0.  raw = the logits l; dist_m = (l_m - max l) - ln sum_m exp(l_m - max l), the sum for m ascending.
 *   u = (w0 >> 8) 2^-24 (float32) or r1 2^-53 (float64) of the draw with j = 0: the single-uniform form of bcn_set_noise.
 *   The action is the smallest k with u < sum_{m <= k} exp(dist_m), summed for m ascending in the buffer's precision; the last class
 *   takes the remainder.  logp = dist[action].
 * deterministic != 0.  Gaussian: raw = mean, logp = the formula at z = 0.  Categorical: the first class that attains the maximum
 *   of dist, logp = its dist entry.  No draw is made and no counter ticks.
 *
 * The draw counter.  A stochastic launch advances the counter of every replica it writes by one.
 * mask_dev (uint8 [B], may be NULL): a replica whose byte is 0 keeps every output row and its counter.
 * Agents.  With cfg.agents = A > 1 every per-row rule above holds with "row" for "replica" (B = cfg.batch rows, each with its own
 *   draw, outputs and counter), except that
 *     mask_dev is uint8 [B / A], one byte per REPLICA: row b reads mask_dev[b / A], so a masked replica keeps all A rows;
 *     replica_offset stays the global index of the first REPLICA: word 0 of the counter is (replica_offset A + b) mod 2^32, the
 *     product taken in 64 bits -- what a batch of B rows with replica_offset A in place of replica_offset draws, and what the
 *     rows of this shard draw in the unsharded batch.
 *   A = 0 or 1: nothing changes.
 * The rollout slot.  With cursor_dev != NULL (int32, the `cursor` segment of a rollout buffer) the launch reads t = cursor_dev[0] ON
 *   THE DEVICE; if 0 <= t < T it also writes logp, value and raw of the replicas it writes into row t of seq_dev
 *   (bcn_actor_seq_layout(cfg, T)); otherwise it writes no slot.  The cursor is never written.  cursor_dev = NULL: seq_dev and T are
 *   not used.
 * No host read, no allocation, no atomics (one lane owns a replica's outputs and counter): the call can be captured in a graph. */
BCN_ACTOR_API int bcn_actor_act(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, void* state_dev,
                                const uint8_t* mask_dev, uint64_t seed, int64_t replica_offset, int deterministic,
                                const int32_t* cursor_dev, int T, void* seq_dev, void* stream);

/* The value network alone on n_rows >= 1 rows obs_dev [n_rows][obs_dim] -> out_dev real [n_rows] (cfg->batch is not used): the
 * last_value and final_values of a GAE.  The same arithmetic as in bcn_actor_act: out_dev[b] equals, bit for bit, the `value` that
 * launch writes for the same row. */
BCN_ACTOR_API int bcn_actor_values(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, int64_t n_rows,
                                   void* out_dev, void* stream);

BCN_ACTOR_API const char* bcn_actor_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

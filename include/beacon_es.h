/* beacon_es.h -- C ABI of libbeacon_es.so: an evolution-strategies learner on the device (Salimans et al. 2017: antithetic Gaussian
 * perturbations, centred ranks, Adam) -- a population of M policies, ONE PER MEMBER, run over a batch of B = M R replicas, the
 * perturbation, the fitness bookkeeping, the ranks, the gradient estimate and the optimiser step (hand-written HIP for gfx950).
 *
 * The library is a unit of its own, like the other seven: it takes device pointers and sizes only and adds nothing to their headers.
 * The Box-Muller pair, the finish, Adam and tree routines are the templates of csrc/td3/td3_impl.h (with csrc/actor/policy_net.h
 * behind it), instantiated in this library too; what both lack -- an MLP whose weights differ per row group -- is csrc/es/es_impl.h.
 * Every launch: no host read, no allocation, no atomics, no inline assembly, sums in the fixed order stated here, separate launches as
 * the only synchronisation between workgroups, capturable in a graph, bit-reproducible.
 *
 * Conventions: every function returns 0 (BCN_ES_OK) or a BCN_ES_ERR_* code (*_layout: the segment count, 0 on error; *_bytes and
 * bcn_es_group: the count, 0 on error); bcn_es_last_error() gives text.  Pointers named *_dev are DEVICE pointers; "real" is float for
 * dtype 0 and double for dtype 1.  Every argument is checked before a device is touched.
 *
 * ---- The model -----------------------------------------------------------------------------------------------------------------
 * cfg: batch B and members M; M even, 2 .. BCN_ES_MAX_MEMBERS; B = M R with R >= 1 replicas per member; replica b belongs to member
 * p = b / R.  obs_dim 1 .. 512.  kind 0 (BCN_ES_BOX): act_dim 1 .. 16 and one bound pair low <= high; kind 1 (BCN_ES_DISCRETE):
 * n_actions 2 .. 16.  1 .. 3 hidden layers of 1 .. 128 units, activation tanh (0) or relu (1).  `group`: 0, or the members one workgroup
 * of the act launch serves (below).
 * ONE deterministic policy MLP obs_dim -> n_out (act_dim, or n_actions) with a linear head.  Every output of every layer is the fma
 * chain  acc = bias;  acc = fma(W[o][k], x[k], acc)  for k ascending, then the activation: the chain of include/beacon_actor.h.
 *   Box       a_i = c + h tanh(head_i) with c = (real)((high + low) / 2), h = (real)((high - low) / 2): the deterministic action of
 *             include/beacon_td3.h, the same expression
 *   Discrete  the FIRST maximum of head_j: best = -inf, arg = 0; for j ascending, head_j replaces best only where head_j > best
 *             strictly (a NaN never wins): the rule of include/beacon_dqn.h; written as int32
 *
 * ---- Buffers ---------------------------------------------------------------------------------------------------------------------
 * theta   the segments pi_w0, pi_b0, ... pi_w{L}, pi_b{L} for L = n_hidden, each 16-byte aligned, matrices [out][in]: E reals INCLUDING
 *         the gaps between segments (bcn_es_params_bytes = E sizeof(real))
 * pop     real [M][E]: row p is member p's parameters in the layout of theta
 * state   gen int32 [4] ([0] the generation, [1] the Adam steps, two spare words); fit float64 [B]; len int32 [B]; alive uint8 [B];
 *         member_fit, util float64 [M] each; stats float64 [8]: fit_mean, fit_std, fit_min, fit_max, best_member, nan_members,
 *         grad_norm (before clipping), spare (0); adam_m, adam_v real [E]
 * work    grad real [E] (the parameter layout); norm2 float64 [ceil(E / 256)]; partial float64 [ceil(M / 2 / BCN_ES_PAIR_CHUNK)][E]
 *         (scratch)
 * A new state buffer is zeros.
 *
 * ---- Noise -----------------------------------------------------------------------------------------------------------------------
 * All draws are words of the project's one Philox4x32-10 definition under the key (low, high word of seed).  The last counter word
 * names the stream: 0 .. 10 are taken (include/beacon_td3.h, include/beacon_sac.h and include/beacon_dqn.h list them), and here
 *   11 perturbation   for pair j = p >> 1 and element e, eps_j[e] is component e & 1 of the Box-Muller pair of the words at counter
 *                     (j, gen[0], e >> 1, 11): the actor's Box-Muller form per dtype (include/beacon_actor.h)
 *
 * ---- bcn_es_begin, ONE launch ----------------------------------------------------------------------------------------------------
 * pop[p][e] = fma(s sigma, eps_j[e], theta[e]) with s = +1 for even p and -1 for odd p, sigma rounded once to real; a gap element is
 * written as theta's.  In the same launch fit = 0, len = 0, alive = 1 for every replica.  sigma = 0 is legal: pop[p] == theta bit
 * for bit.  gen[0] is read on the device.
 *
 * ---- bcn_es_act, ONE launch ------------------------------------------------------------------------------------------------------
 * Replica b runs the MLP on row b of obs_dev [B][obs_dim] with row b / R of weights_dev ([M][E]); with shared = 1 every replica uses
 * the ONE row weights_dev points to (theta itself, for evaluation).  It writes actions_dev: real [B][act_dim], or int32 [B].  A
 * replica whose mask byte is 0 keeps its action.
 * The tile kernel: a workgroup of 256 lanes serves G consecutive members whose G R rows fit a tile of BCN_ES_TILE_ROWS rows, or, where
 * R exceeds a tile, one member whose rows it walks tile after tile (the tiles of one member are dealt to at most as many workgroups
 * as keep the launch at about BCN_ES_WANT_GRID workgroups).  Per layer and per slab of KS reduction steps (64 in float32, 32 in
 * float64) the slab of each member's matrix goes from HBM to LDS with coalesced loads, 16 bytes per lane where the layer's input
 * width is a multiple of 4, and every row of the member in the tile takes it from there; activations stay in LDS.  A member whose rows
 * fit one tile (R <= BCN_ES_TILE_ROWS) is read from HBM exactly once per launch.  A member that spans several tiles is NOT: its slabs
 * are staged again for every tile, by up to `split` workgroups that may run on different XCDs; whether those reads are served by a
 * cache or by HBM is not guaranteed and was not measured.  One lane owns an (output, row) pair and runs its chain in k order, so the result for a replica depends neither on R nor
 * on the grouping.  Nothing is read past a row, a member or the batch.
 * G: cfg.group where it is not 0 (1 .. BCN_ES_MAX_GROUP; a group > 1 needs group R <= BCN_ES_TILE_ROWS), else the largest
 * G <= min(BCN_ES_MAX_GROUP, BCN_ES_TILE_ROWS / R, M / 512), at least 1, whose LDS fits; bcn_es_group(cfg) returns it.
 * Dynamic LDS, bcn_es_lds_bytes(cfg):  sizeof(real) (2 TR HP + TR (KS + 4) + G nmax (KS + 4))  with TR = BCN_ES_TILE_ROWS, nmax the
 * widest layer output (the head included) and HP = nmax rounded up to a multiple of 4.  A cfg whose sum exceeds BCN_ES_LDS_LIMIT is
 * refused by every function here before any launch.
 *
 * ---- bcn_es_observe, ONE launch (behind every env step) --------------------------------------------------------------------------
 * Where alive[b]:  fit[b] += (double)rwd[b];  len[b] += 1;  alive[b] = 0 if done[b] | trunc[b].  So fitness is the return of the
 * replica's FIRST episode of the generation; under auto-reset the later episodes weigh nothing.
 *
 * ---- bcn_es_update, SEVEN launches -----------------------------------------------------------------------------------------------
 *   1. fit:     F_p = (sum_{r < R} fit[p R + r]) / R for r ascending, in float64; a NaN F_p counts as -inf: member_fit[p]
 *   2. rank:    rank_p = #{q : F_q < F_p, or F_q == F_p and q < p};  u_p = rank_p / (M - 1) - 0.5 in float64: util[p].  The statistics,
 *               by workgroup 0, over the n members with F_p > -inf (a NaN member is none of them; all 0 where n = 0): lane t adds
 *               p = t, t + 256, ...
 *               ascending, the 256 lanes' values by the tree 128, 64 ... 1;  fit_mean = sum / n;  fit_std = sqrt(sum (F - mean)^2 / n);
 *               fit_min, fit_max;  best_member the lowest p with F_p = fit_max;  nan_members = M - n
 *   3. partial: for chunk c of BCN_ES_PAIR_CHUNK pairs:  partial[c][e] = sum_j (u_{2j} - u_{2j+1}) (double)eps_j[e] for j ascending
 *               inside the chunk, in float64, eps regenerated (never read back from pop)
 *   4. reduce:  g[e] = (real)((sum_c partial[c][e]) / (M sigma)) for c ascending, rounded once;
 *               grad[e] = -(g[e]) + weight_decay theta[e] (weight_decay rounded once to real); a gap element is 0
 *   5. finish:  stats[grad_norm] = sqrt(sum grad^2), in float64 in a fixed tree
 *   6. adam:    Adam of include/beacon_learner.h, the arithmetic of bcn_td3_adam, on theta over all E elements with max_grad_norm
 *               clipping on grad and t = gen[1] + 1; hyper.eps > 0 is required (in a gap grad = m = v = 0, and 0 / (0 + eps) must be 0)
 *   7. tick:    one lane: gen[0] += 1, gen[1] += 1
 * sigma <= 0 is an argument error here.
 */
#ifndef BEACON_ES_H
#define BEACON_ES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_ES_API __attribute__((visibility("default")))
#define BCN_ES_API_VERSION 1

enum { BCN_ES_OK = 0, BCN_ES_ERR_ARG = 1, BCN_ES_ERR_HIP = 2 };
/* element types of a segment */
enum { BCN_ES_REAL = 0, BCN_ES_I32 = 1, BCN_ES_U32 = 2, BCN_ES_F64 = 3, BCN_ES_U8 = 4 };
enum { BCN_ES_BOX = 0, BCN_ES_DISCRETE = 1 };
enum { BCN_ES_STAT_FIT_MEAN = 0, BCN_ES_STAT_FIT_STD = 1, BCN_ES_STAT_FIT_MIN = 2, BCN_ES_STAT_FIT_MAX = 3, BCN_ES_STAT_BEST_MEMBER = 4,
       BCN_ES_STAT_NAN_MEMBERS = 5, BCN_ES_STAT_GRAD_NORM = 6, BCN_ES_STAT_SPARE = 7, BCN_ES_N_STATS = 8 };

#define BCN_ES_MAX_MEMBERS 16384  /* members, at most */
#define BCN_ES_MAX_OBS 512        /* obs_dim, at most */
#define BCN_ES_MAX_ACT 16         /* act_dim and n_actions, at most */
#define BCN_ES_PAIR_CHUNK 64      /* pairs per partial sum of the gradient */
#define BCN_ES_TILE_ROWS 32       /* rows of a tile of the act launch */
#define BCN_ES_MAX_GROUP 8        /* members per workgroup of the act launch, at most */
#define BCN_ES_WANT_GRID 1024     /* workgroups the act launch aims at where members span tiles */
#define BCN_ES_MAX_SEGS 16
#define BCN_ES_LDS_LIMIT 163840   /* bytes of dynamic LDS the act launch may ask for */

typedef struct {
  int32_t batch;        /* B = members x replicas per member */
  int32_t members;      /* M, even */
  int32_t obs_dim;
  int32_t kind;         /* 0 Box, 1 Discrete */
  int32_t act_dim;      /* Box: 1 .. 16 (ignored for Discrete) */
  int32_t n_actions;    /* Discrete: 2 .. 16 (ignored for Box) */
  int32_t dtype;        /* 0 float32, 1 float64 */
  int32_t n_hidden, hidden[3];
  int32_t activation;   /* 0 tanh, 1 relu */
  int32_t group;        /* 0: the library chooses; else members per workgroup of the act launch */
  int32_t reserved;     /* 0 */
  double low, high;     /* Box: the one bound pair */
} bcn_es_cfg;

/* One named segment: row_elems elements of kind `elem` at `offset` bytes (the fields of bcn_td3_seg; planes is 0). */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;
  int32_t planes;
  int64_t row_elems;
} bcn_es_seg;

typedef struct { double sigma, lr, beta1, beta2, eps, max_grad_norm, weight_decay; } bcn_es_hyper;

BCN_ES_API int bcn_es_params_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs);
BCN_ES_API size_t bcn_es_params_bytes(const bcn_es_cfg* cfg);
BCN_ES_API int bcn_es_state_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs);
BCN_ES_API size_t bcn_es_state_bytes(const bcn_es_cfg* cfg);
BCN_ES_API int bcn_es_work_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs);
BCN_ES_API size_t bcn_es_work_bytes(const bcn_es_cfg* cfg);
/* the members one workgroup of the act launch serves; 0 for a refused cfg */
BCN_ES_API int bcn_es_group(const bcn_es_cfg* cfg);
/* the dynamic LDS of the act launch for this cfg in bytes; 0 for a refused cfg */
BCN_ES_API size_t bcn_es_lds_bytes(const bcn_es_cfg* cfg);

BCN_ES_API int bcn_es_begin(const bcn_es_cfg* cfg, const void* theta_dev, void* pop_dev, void* state_dev, double sigma, uint64_t seed,
                            void* stream);
BCN_ES_API int bcn_es_act(const bcn_es_cfg* cfg, const void* weights_dev, int shared, const void* obs_dev, const uint8_t* mask_dev,
                          void* actions_dev, void* stream);
BCN_ES_API int bcn_es_observe(const bcn_es_cfg* cfg, void* state_dev, const void* rwd_dev, const uint8_t* done_dev, const uint8_t* trunc_dev,
                              void* stream);
BCN_ES_API int bcn_es_update(const bcn_es_cfg* cfg, void* theta_dev, void* state_dev, void* work_dev, const bcn_es_hyper* hyper,
                             uint64_t seed, void* stream);

BCN_ES_API const char* bcn_es_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

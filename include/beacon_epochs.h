/* beacon_epochs.h -- C ABI of libbeacon_epochs.so: what a PPO update needs around its minibatches (hand-written HIP for gfx950).
 *
 * bcn_epochs_permute draws the shuffle of an epoch -- a permutation of the rows, a pure function of (n, seed, epoch) from the
 * project's one Philox definition -- and bcn_epochs_begin opens an update: it clears the learner's stop flag and standardises the
 * advantages with float64 sums in a fixed order.  With bcn_learner_grad / bcn_learner_step (include/beacon_learner.h) between them
 * a whole update is a chain of the library's own launches: no host read, no allocation, no atomics, bit-reproducible, capturable
 * as ONE graph.  The library is a unit of its own, like the actor's and the learner's: it takes device pointers and sizes only and
 * adds nothing to include/beacon_hip.h, beacon_actor.h or beacon_learner.h.
 *
 * Conventions: every function returns 0 (BCN_EPOCHS_OK) or a BCN_EPOCHS_ERR_* code (work_layout / work_bytes: the segment count /
 * the byte count); bcn_epochs_last_error() gives text.  Pointers named *_dev are DEVICE pointers; "real" is float for dtype 0 and
 * double for dtype 1.  Every argument is checked before a device is touched.
 *
 * ---- The permutation --------------------------------------------------------------------------------------------------------
 * idx_dev int32 [n] becomes a permutation of 0 .. n - 1, for 1 <= n <= 2^31 - 1: a Feistel network over the k bits that hold
 * n - 1, walked along its cycles until it lands below n.
 *   Geometry.  k = max(2, bit_length(n - 1)), hl = k / 2 (rounded down), hr = k - hl.
 *   The map.   Split x < 2^k into L = x >> hr (hl bits) and R = x & (2^hr - 1).  For the rounds r = 0 .. 5: an even r gives
 *              L ^= F(r, R) & (2^hl - 1), an odd r gives R ^= F(r, L) & (2^hr - 1), where F(r, h) is word 0 of Philox4x32-10 at
 *              the counter (h, epoch, r, 3) under the key (low, high word of seed).  Then f(x) = (L << hr) | R.
 *              The counter's last word 3 is this stream's own: 0 is the inlet noise, 1 the random-start reset, 2 the actor.
 *   The output. idx[i] is the first of f(i), f(f(i)), ... that is < n (cycle walking).
 *   Why it ends. Each round XORs one half by a function of the other, so f is a bijection of 0 .. 2^k - 1 whatever F is.  The walk
 *              from i < n stays on i's cycle, which holds an element < n -- i itself -- so it ends within 2^k applications, and
 *              distinct i end at distinct values.  The kernel's loop is a `for` bounded by 2^k, never a `while`.
 *              The domain 2^k is below 2 n for n >= 3, so a walk takes under two applications on average.
 * `epoch` is the uint32 the word epoch_dev[0] holds (the learner's step[1]: the permutations drawn so far).  Two launches in stream
 * order: the permutation (one lane per i), then the tick epoch_dev[0] += 1 -- so a captured update draws a new permutation at every
 * replay.  The definition is restated on the host in tests/epochs_ref.py.
 * Stated limit: six rounds on a few bits are no random permutation.  For n below about 16 the distribution over whole permutations
 * is visibly not uniform (n = 5 over 24 000 epochs: all 120 permutations occur, chi-square 6 694 at 119 degrees of freedom).  It is
 * a shuffle for minibatches of hundreds of rows and more, where what matters -- which minibatch a row falls into, and which rows
 * share one -- is uniform (tests/test_epochs_host.py).
 *
 * ---- The standardisation ----------------------------------------------------------------------------------------------------
 * Rows.  Row s of n_rows is ACTIVE by the learner's rules: weight_dev[s / rows_per_weight] > 0 (uint8 or real by weight_kind; no
 * weight array: every row; a NaN weight is not > 0) and, with cursor_dev != NULL, s < min(max(cursor_dev[0], 0) rows_per_step,
 * n_rows).  Of an inactive row only the weight is read: its adv may hold anything, NaN included, and is no part of any sum.
 * With c the number of active rows:
 *   mean = (sum adv) / max(c, 1);   var = (sum (adv - mean)^2) / max(c - 1, 1);   out = (adv - mean) / (sqrt(var) + 1e-8)
 * over the active rows, all in float64 (a float32 adv is exact in it), and out rounded ONCE to the buffer's precision; an inactive
 * row gets +0.  Two passes: the deviations are taken from the mean, never from a sum of squares.
 * Order.  A chunk is 1024 consecutive rows; the grid is G = min(BCN_EPOCHS_GRID, chunks) workgroups of 256 lanes; workgroup g
 * walks the chunks g, g + G, g + 2 G, ...; in a chunk lane t takes the rows t, t + 256, t + 512, t + 768 of it, in that order, and
 * adds them to its one float64 accumulator across all its chunks; the 256 accumulators are added by the tree 128, 64, ... 1 in
 * LDS; the G partials are added for g ascending.  Three launches in stream order, which are the only synchronisation between
 * workgroups (no tickets, flags, waits or atomics):
 *   1. sum:   the partials of (sum adv, c) into the work buffer; workgroup 0 clears the stop flag
 *   2. dev:   every workgroup forms mean from the G partials, then the partials of sum (adv - mean)^2; workgroup 0 writes moments[0, 2]
 *   3. write: every workgroup forms var from the G partials and writes its rows of adv_out; workgroup 0 writes moments[1, 3]
 * The result does not depend on how workgroups are scheduled.  adv_out_dev may not alias adv_dev.
 * Without `normalize`, bcn_epochs_begin is one launch of one lane that clears the stop flag.
 *
 * ---- The stop flag ----------------------------------------------------------------------------------------------------------
 * step_dev is the `step` segment of the learner's optimiser buffer, int32 [4]: [0] the Adam steps taken, [1] the permutations
 * drawn (epoch_dev of bcn_epochs_permute), [2] the KL stop flag, [3] the steps the stop rule skipped.  bcn_epochs_begin sets
 * step_dev[2] = 0 and touches no other word; step_dev = NULL: no flag is cleared (then `normalize` must be set).
 */
#ifndef BEACON_EPOCHS_H
#define BEACON_EPOCHS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_EPOCHS_API __attribute__((visibility("default")))
#define BCN_EPOCHS_API_VERSION 1

enum { BCN_EPOCHS_OK = 0, BCN_EPOCHS_ERR_ARG = 1, BCN_EPOCHS_ERR_HIP = 2 };
/* element types of a segment: the numbers of BCN_ACTOR_REAL and BCN_LEARNER_F64 */
enum { BCN_EPOCHS_REAL = 0, BCN_EPOCHS_F64 = 3 };
enum { BCN_EPOCHS_W_NONE = 0, BCN_EPOCHS_W_U8 = 1, BCN_EPOCHS_W_REAL = 2 };
/* the entries of the moments segment (float64) */
enum { BCN_EPOCHS_MOM_MEAN = 0, BCN_EPOCHS_MOM_VAR = 1, BCN_EPOCHS_MOM_COUNT = 2, BCN_EPOCHS_MOM_DENOM = 3, BCN_EPOCHS_N_MOMENTS = 4 };

#define BCN_EPOCHS_GRID 64        /* workgroups of the standardisation's launches, at most */
#define BCN_EPOCHS_CHUNK 1024     /* rows of a chunk */
#define BCN_EPOCHS_ROUNDS 6       /* Feistel rounds of the permutation */
#define BCN_EPOCHS_MAX_SEGS 4

/* One named segment of the work buffer: row_elems elements of kind `elem` at `offset` bytes (the fields of bcn_actor_seg). */
typedef struct {
  char name[16];
  uint64_t offset;
  int32_t elem;         /* BCN_EPOCHS_F64 */
  int32_t planes;       /* 0 */
  int64_t row_elems;
} bcn_epochs_seg;

typedef struct {
  const void* adv_dev;        /* real [n_rows]; ignored without normalize */
  void* adv_out_dev;          /* real [n_rows]; ignored without normalize */
  const void* weight_dev;     /* uint8 or real [n_rows / rows_per_weight] by weight_kind; ignored for BCN_EPOCHS_W_NONE */
  const int32_t* cursor_dev;  /* int32, the `cursor` segment of a rollout buffer, or NULL */
  int32_t* step_dev;          /* int32 [4], the `step` segment of the learner's optimiser buffer, or NULL */
  void* work_dev;             /* bcn_epochs_work_bytes() bytes; ignored without normalize */
  int64_t n_rows;             /* 1 .. 2^31 - 1 */
  int32_t dtype;              /* 0 float32, 1 float64 */
  int32_t normalize;          /* 0: clear the flag only */
  int32_t weight_kind;        /* BCN_EPOCHS_W_* */
  int32_t rows_per_step;      /* with cursor_dev: rows per recorded step, >= 1 */
  int32_t rows_per_weight;    /* consecutive rows that share one weight, >= 0; 0 means 1.  It divides n_rows */
} bcn_epochs_batch;

/* The work buffer of bcn_epochs_begin, three float64 segments (planes = 0); only `moments` is for the caller:
 *   moments  [4]: mean, var, the count of active rows, sqrt(var) + 1e-8 of the last standardisation
 *   part     [BCN_EPOCHS_GRID][2]: the workgroups' partial (sum adv, count)
 *   part2    [BCN_EPOCHS_GRID]: the workgroups' partial sum of squared deviations
 * The same for every n_rows and dtype.  It needs no initialisation. */
BCN_EPOCHS_API int bcn_epochs_work_layout(bcn_epochs_seg* segs, int max_segs);
BCN_EPOCHS_API size_t bcn_epochs_work_bytes(void);

/* idx_dev int32 [n] = the permutation of (n, seed, epoch_dev[0]) above; then epoch_dev[0] += 1.  Two launches. */
BCN_EPOCHS_API int bcn_epochs_permute(int64_t n, uint64_t seed, int32_t* epoch_dev, int32_t* idx_dev, void* stream);

/* The head of an update (above): the stop flag, and with batch->normalize the standardised advantages.  Three launches, or one. */
BCN_EPOCHS_API int bcn_epochs_begin(const bcn_epochs_batch* batch, void* stream);

BCN_EPOCHS_API const char* bcn_epochs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

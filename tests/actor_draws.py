"""Draws of the actor's stream built on purpose (not a test module): per replica, the draw counter whose Box-Muller radius is
extreme, found by scanning tests/actor_ref.py's restatement of the stream.  A few thousand ordinary draws never reach the tails of
Box-Muller -- a radius above 4 has probability e^-8, one below 1e-2 has 5e-5 -- so tests/test_actor_draws_host.py (the conditions, on
the CPU) and tests/test_gpu_actor_edges.py (the device) write these counters into the actor's state instead of waiting for them.

The parameters put every other corner of the stream into the same launch: both key words are non-zero, and replica_offset + b wraps
at 2^32 inside the batch (row 3 has the global index 0)."""
import functools

import numpy as np

import actor_ref as R

SEED = 0x1234567887654321
OFFSET = 2 ** 32 - 3
B = 128
N_SCAN = 2 ** 17
CHUNK = 2 ** 13                      # counters per vectorised Philox call: B x CHUNK uint64 temporaries of 8 MB each

# the categorical tail case: classes 0 and 3 are rarer than the exemption DELTA = 1e-5 of tests/test_gpu_actor.py is wide
TAIL_P = (2.0 ** -17, 0.5, 0.5 - 2.0 ** -16, 2.0 ** -17)
# a draw within eight steps of a float32 u of a reference boundary may fall either way: the float32 rounding of a three-term
# cumulative sum near 1 is a few 2^-24
DELTA_TAIL = 2.0 ** -21
CAP_TAIL = 0.06                      # at most this share of the draws may be exempt


@functools.lru_cache(maxsize=None)
def extreme_counters(seed=SEED, replica_offset=OFFSET, B=B, n_scan=N_SCAN):
    """int64 [B], read-only: per row b the counter c in [0, n_scan) whose pair j = 0 has the smallest (even b) or the largest (odd b)
    k = w0 >> 8 (the first such c on a tie).  u1 = (k + 0.5) 2^-24 in float32, and the float64 u1 takes its top 24 bits from the same
    k: the smallest k is the largest radius and the largest k the smallest radius in both precisions, and k 2^-24 is (the top of) the
    categorical kind's single uniform too."""
    rows = np.arange(B)[:, None]
    best = np.zeros(B, dtype=np.int64)
    best_k = np.where(np.arange(B) % 2 == 0, np.iinfo(np.int64).max, -1)
    even = np.arange(B) % 2 == 0
    for c0 in range(0, n_scan, CHUNK):
        ctr = np.arange(c0, min(c0 + CHUNK, n_scan))
        k = (R.words(seed, replica_offset, rows, ctr[None, :], 0)[0] >> R.U8).astype(np.int64)
        at = np.where(even, k.argmin(axis=1), k.argmax(axis=1))
        got = k[np.arange(B), at]
        better = np.where(even, got < best_k, got > best_k)         # strict: an earlier chunk keeps a tie
        best, best_k = np.where(better, ctr[at], best), np.where(better, got, best_k)
    best.setflags(write=False)
    return best


def pair0(counters, dtype, seed=SEED, replica_offset=OFFSET):
    """(u1, u2, radius) of the pair j = 0 of every row at its counter, float64 arithmetic on the uniforms of `dtype`"""
    u1, u2 = R.pair_uniforms(R.words(seed, replica_offset, np.arange(len(counters)), np.asarray(counters), 0), dtype)
    return u1, u2, np.sqrt(-2.0 * np.log(u1))


def f32_pair(w0, w1, complement):
    """(z0, z1) of the header's float32 pair formula in NumPy float32, every elementary function correctly rounded (evaluated in
    float64 on the float32 argument, rounded once).  complement = False forms u1 = (k + 0.5) 2^-24 in float32 and takes its log;
    True takes log1p(-(2^24 - k - 0.5) 2^-24) for k >= 2^23, where k + 0.5 is no float32 and u1 itself would lose the bits that
    set a small radius."""
    f32, f64 = np.float32, np.float64
    fn = lambda f, x: f(x.astype(f64)).astype(f32)
    k = (np.asarray(w0, dtype=np.uint64) >> R.U8).astype(np.int64)
    scale = f32(2.0 ** -24)
    ln_u1 = fn(np.log, (k.astype(f32) + f32(0.5)) * scale)
    if complement:
        comp = ((2 ** 24 - np.maximum(k, 2 ** 23)).astype(f32) - f32(0.5)) * scale         # (the rows of the other branch: any valid k)
        ln_u1 = np.where(k < 2 ** 23, ln_u1, fn(np.log1p, -comp))
    two_u2 = (np.asarray(w1, dtype=np.uint64) >> R.U8).astype(f32) * f32(2.0 ** -23)
    radius = np.sqrt(f32(-2.0) * ln_u1)
    assert ln_u1.dtype == f32 and two_u2.dtype == f32 and radius.dtype == f32
    c, s = fn(lambda x: np.cos(np.pi * x), two_u2), fn(lambda x: np.sin(np.pi * x), two_u2)
    return radius * c, radius * s


def tail_classes(dist, counters, dtype, seed=SEED, replica_offset=OFFSET):
    """(class, exempt, u) per row of the categorical rule on the float64 log-probabilities `dist` [B, n] at each row's counter;
    exempt: u lies within DELTA_TAIL of one of the reference's cumulative boundaries"""
    u = R.single_uniform(R.words(seed, replica_offset, np.arange(len(counters)), np.asarray(counters), 0), dtype)
    a, cum = R.categorical(dist, u)
    return a, (np.abs(u[:, None] - cum) <= DELTA_TAIL).any(axis=1), u

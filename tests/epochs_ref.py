"""The shuffle and the standardisation of libbeacon_epochs.so restated on the host (not a test module): NumPy only, written from
include/beacon_epochs.h, on noise_ref.philox4x32_10.  Nothing here reads the kernels' constants."""
import numpy as np

import noise_ref as P

ROUNDS = 6
STREAM = 3            # the counter's last word: 0 inlet noise, 1 random-start reset, 2 the actor, 3 this shuffle


def geometry(n):
    """(k, hl, hr): the domain's bits and the two halves' of the header"""
    k = max(2, int(n - 1).bit_length())
    hl = k // 2
    return k, hl, k - hl


def round_tables(n, seed, epoch):
    """F(r, h) of the header for every round r and every value h of the half it reads: a round function sees hr bits (r even) or
    hl bits (r odd), at most 2^16 values, so each is evaluated once and f becomes six look-ups"""
    _, hl, hr = geometry(n)
    k0, k1 = P._key(seed)
    return [P.philox4x32_10(np.arange(1 << (hr if r % 2 == 0 else hl), dtype=np.uint64), int(epoch) & 0xFFFFFFFF, r, STREAM, k0, k1)[0]
            for r in range(ROUNDS)]


def feistel(x, n, seed, epoch, tables=None):
    """f of the header on an array of values < 2^k"""
    k, hl, hr = geometry(n)
    F = tables if tables is not None else round_tables(n, seed, epoch)
    x = np.asarray(x, dtype=np.uint64)
    ml, mr = np.uint64((1 << hl) - 1), np.uint64((1 << hr) - 1)
    L, R = x >> np.uint64(hr), x & mr
    for r in range(ROUNDS):
        if r % 2 == 0:
            L = L ^ (F[r][R.astype(np.int64)] & ml)
        else:
            R = R ^ (F[r][L.astype(np.int64)] & mr)
    return (L << np.uint64(hr)) | R


def permutation(n, seed, epoch, walks=False):
    """idx int64 [n]: idx[i] is the first of f(i), f(f(i)), ... below n; with `walks` also the longest walk (applications of f).
    AssertionError if a walk has not ended within 2^k applications."""
    n = int(n)
    assert 1 <= n < 1 << 31
    k, _, _ = geometry(n)
    out = np.full(n, -1, dtype=np.int64)
    todo = np.arange(n, dtype=np.int64)               # the positions still walking
    x = todo.astype(np.uint64)
    longest = 0
    tables = round_tables(n, seed, epoch)
    while todo.size:
        longest += 1
        assert longest <= 1 << k, (n, seed, epoch)
        x = feistel(x, n, seed, epoch, tables)
        done = x < np.uint64(n)
        out[todo[done]] = x[done].astype(np.int64)
        todo, x = todo[~done], x[~done]
    return (out, longest) if walks else out


def active_rows(n_rows, weight=None, rows_per_weight=1, cursor=None, rows_per_step=1):
    """bool [n_rows]: the header's row rules"""
    s = np.arange(n_rows)
    on = np.ones(n_rows, dtype=bool)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            on &= np.asarray(weight)[s // max(int(rows_per_weight), 1)] > 0
    if cursor is not None:
        on &= s < min(max(int(cursor), 0) * int(rows_per_step), n_rows)
    return on


def standardise(adv, on):
    """(out float64 [n], mean, var, count): the header's two-pass arithmetic in float64, np.sum's order; inactive rows 0"""
    a = np.asarray(adv, dtype=np.float64)
    c = int(on.sum())
    mean = a[on].sum() / max(c, 1)
    var = ((a[on] - mean) ** 2).sum() / max(c - 1, 1)
    out = np.zeros(a.shape, dtype=np.float64)
    out[on] = (a[on] - mean) / (np.sqrt(var) + 1e-8)
    return out, mean, var, c

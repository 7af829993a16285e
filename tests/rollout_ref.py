"""The yardsticks of the rollout tests (not a test module): the GAE recurrence of bcn_rollout_gae (include/beacon_hip.h) restated in
float64 NumPy, an independent extended-precision formulation of the same quantity, the random inputs both are fed, and the
tolerance that goes with them."""
import numpy as np


def gae_inputs(rng, T, ncols, cols=1, p_fin=0.2, p_invalid=0.1, dtype=np.float64):
    """Random inputs of one rollout: rwd, values, final_values [T, ncols], last_value [ncols] (rounded to `dtype`, returned in
    float64: an exact upcast), done, trunc, valid uint8 [T, ncols / cols] -- roughly p_fin terminal steps, half of them time limits
    (done = trunc = 1, which bootstrap) and half blow-ups (done alone, terminal), and roughly p_invalid skipped steps."""
    B = ncols // cols
    r = lambda scale, *shape: (scale * rng.standard_normal(shape)).astype(dtype).astype(np.float64)
    fin = rng.random((T, B)) < p_fin
    limit = rng.random((T, B)) < 0.5
    done = fin.astype(np.uint8)
    trunc = (fin & limit).astype(np.uint8)
    valid = (rng.random((T, B)) >= p_invalid).astype(np.uint8)
    return dict(rwd=r(1.0, T, ncols), values=r(3.0, T, ncols), final_values=r(3.0, T, ncols), last_value=r(3.0, ncols), done=done,
                trunc=trunc, valid=valid)


def gae_ref(rwd, values, last_value, done, trunc, valid, final_values=None, gamma=0.99, lam=0.95, cols=1, n=None):
    """bcn_rollout_gae in float64, operation for operation: (adv, ret) [T, ncols]; rows t >= n are NaN (not written)."""
    T, ncols = rwd.shape
    n = T if n is None else min(int(n), T)
    rep = lambda f: np.repeat(np.asarray(f), cols, axis=-1)           # the flags of replica c // cols
    adv, ret = np.full((T, ncols), np.nan), np.full((T, ncols), np.nan)
    nv, gae = np.array(last_value, dtype=np.float64), np.zeros(ncols)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n - 1, -1, -1):
            d, tr, ok = rep(done[t]) != 0, rep(trunc[t]) != 0, rep(valid[t]) != 0
            fin = d | tr
            boot = np.where(tr, final_values[t], 0.0) if final_values is not None else np.zeros(ncols)
            delta = rwd[t] + gamma * np.where(fin, boot, nv) - values[t]
            g = delta + np.where(fin, 0.0, gamma * lam * gae)
            adv[t] = np.where(ok, g, 0.0)
            ret[t] = np.where(ok, g + values[t], values[t])
            gae = np.where(ok, g, gae)
            nv = np.where(ok, values[t], nv)
    return adv, ret


def gae_explicit(rwd, values, last_value, done, trunc, valid, final_values=None, gamma=0.99, lam=0.95, cols=1):
    """The same quantity without the recurrence, in numpy.longdouble: every column is cut into episodes at done | trunc, its skipped
    steps dropped, and every advantage is the explicit sum of (gamma lam)^k delta over the rest of its episode."""
    L = np.longdouble
    T, ncols = rwd.shape
    adv, ret = np.zeros((T, ncols), dtype=L), np.zeros((T, ncols), dtype=L)
    g, gl = L(gamma), L(gamma) * L(lam)
    for c in range(ncols):
        b = c // cols
        ret[:, c] = values[:, c]
        steps = [t for t in range(T) if valid[t, b]]
        episodes, cur = [], []
        for t in steps:
            cur.append(t)
            if done[t, b] or trunc[t, b]:
                episodes.append(cur)
                cur = []
        if cur:
            episodes.append(cur)
        for ep in episodes:
            last = ep[-1]
            delta = {}
            for i, t in enumerate(ep):
                if t != last:
                    nxt = L(values[ep[i + 1], c])
                elif done[t, b] or trunc[t, b]:
                    nxt = L(final_values[t, c]) if (final_values is not None and trunc[t, b]) else L(0)
                else:
                    nxt = L(last_value[c])
                delta[t] = L(rwd[t, c]) + g * nxt - L(values[t, c])
            for i, t in enumerate(ep):
                adv[t, c] = sum((gl ** k * delta[u] for k, u in enumerate(ep[i:])), L(0))
                ret[t, c] = adv[t, c] + L(values[t, c])
    return adv, ret


def gae_bound(T, adv, values, rwd):
    """8 T 2^-53 A per column, A = max |adv| + max |values| + max |rwd| of the column: five roundings per step, each of a quantity
    bounded by A, carried on with a factor <= 1.  [ncols]; NaN entries are left out of the maxima."""
    with np.errstate(invalid="ignore"):
        amax = lambda x: np.nan_to_num(np.nanmax(np.abs(np.asarray(x, dtype=np.float64)), axis=0), nan=0.0)
        return 8.0 * T * 2.0 ** -53 * (amax(adv) + amax(values) + amax(rwd))

"""The on-device actor restated on the host (not a test module): both MLPs, the Philox mapping, Box-Muller, the clip, both
log-probability formulas and the categorical rule of include/beacon_actor.h.  NumPy only, everything in float64, written from the
header: nothing here reads the kernel.  The Philox rounds are noise_ref's."""
import numpy as np

from noise_ref import _key, philox4x32_10

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)
U21, U11, U8 = np.uint64(21), np.uint64(11), np.uint64(8)


def mlp(x, layers, activation):
    """x [n, in] through [(W [out, in], b [out]), ...]: act(W x + b) for all but the last pair, which is linear.  float64."""
    h = np.asarray(x, dtype=np.float64)
    for l, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if l < len(layers) - 1:
            h = np.tanh(h) if activation == "tanh" else np.maximum(h, 0.0)
    return h


def words(seed, replica_offset, b, ctr, j):
    """(w0, w1, w2, w3) of counter (replica_offset + b, ctr, j, 2) under the key (low, high word of seed); the arguments broadcast."""
    k0, k1 = _key(seed)
    return philox4x32_10(np.asarray(b, dtype=np.int64) + int(replica_offset), ctr, j, 2, k0, k1)


def pair_uniforms(w, dtype):
    """(u1, u2) of a Box-Muller pair as float64 values: the float32 forms are exact in float64; the float64 u1 rounds (r1 + 0.5) to
    nearest even as the device's float64 sum does."""
    w0, w1, w2, w3 = w
    if np.dtype(dtype) == np.float32:
        return ((w0 >> U8).astype(np.float64) + 0.5) * 2.0 ** -24, (w1 >> U8).astype(np.float64) * 2.0 ** -24
    r1, r2 = (w0 << U21) ^ (w1 >> U11), (w2 << U21) ^ (w3 >> U11)
    return (r1.astype(np.float64) + 0.5) * 2.0 ** -53, r2.astype(np.float64) * 2.0 ** -53


def single_uniform(w, dtype):
    """the single-uniform form of bcn_set_noise: (w0 >> 8) 2^-24 or ((w0 << 21) ^ (w1 >> 11)) 2^-53"""
    w0, w1, _, _ = w
    if np.dtype(dtype) == np.float32:
        return (w0 >> U8).astype(np.float64) * 2.0 ** -24
    return ((w0 << U21) ^ (w1 >> U11)).astype(np.float64) * 2.0 ** -53


def normals(seed, replica_offset, b, ctr, act_dim, dtype):
    """z [len(b), act_dim]: component 2j = radius cos(angle), 2j + 1 = radius sin(angle) of the draw j; b, ctr: [n] arrays"""
    b, ctr = np.asarray(b), np.asarray(ctr)
    z = np.zeros((b.size, act_dim))
    for j in range((act_dim + 1) // 2):
        u1, u2 = pair_uniforms(words(seed, replica_offset, b, ctr, j), dtype)
        radius, angle = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        z[:, 2 * j] = radius * np.cos(angle)
        if 2 * j + 1 < act_dim:
            z[:, 2 * j + 1] = radius * np.sin(angle)
    return z


def gaussian(mean, log_std, z, low, high):
    """(actions, raw, logp) of the Gaussian kind; z = 0 is the deterministic mode"""
    log_std = np.asarray(log_std, dtype=np.float64)
    raw = mean + np.exp(log_std) * z
    logp = (-0.5 * z * z - log_std - HALF_LN_2PI).sum(axis=1)
    return np.minimum(np.maximum(raw, low), high), raw, logp


def log_softmax(logits):
    s = logits - logits.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


def categorical(dist, u):
    """The smallest k with u < sum_{m <= k} exp(dist_m), the last class taking the remainder: (actions [n], cum [n, classes - 1], the
    boundaries u was compared with)."""
    cum = np.cumsum(np.exp(dist[:, :-1]), axis=1)
    return (u[:, None] >= cum).sum(axis=1), cum


def first_argmax(dist):
    return np.argmax(dist, axis=1)           # numpy returns the first maximum


def act(obs, pi, vf, log_std, activation, kind, dtype, seed, replica_offset, counters, low=-1.0, high=1.0, deterministic=False):
    """One launch: dict of actions, raw, logp, value, dist, z / u (the draws) and the counters afterwards.  kind: "gaussian" /
    "categorical"; dtype: the DEVICE buffer's precision (it selects the uniforms' form; the arithmetic here is float64)."""
    obs = np.asarray(obs, dtype=np.float64)
    n = obs.shape[0]
    b = np.arange(n)
    counters = np.asarray(counters, dtype=np.int64)
    head = mlp(obs, pi, activation)
    out = {"value": mlp(obs, vf, activation)[:, 0], "counters": counters + (0 if deterministic else 1)}
    if kind == "gaussian":
        z = np.zeros_like(head) if deterministic else normals(seed, replica_offset, b, counters, head.shape[1], dtype)
        out["actions"], out["raw"], out["logp"] = gaussian(head, log_std, z, low, high)
        out["dist"], out["z"] = head, z
    else:
        dist = log_softmax(head)
        if deterministic:
            a, u, cum = first_argmax(dist), None, None
        else:
            u = single_uniform(words(seed, replica_offset, b, counters, 0), dtype)
            a, cum = categorical(dist, u)
        out.update(actions=a, raw=head, dist=dist, logp=dist[b, a], u=u, cum=cum)
    return out

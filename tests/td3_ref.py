"""include/beacon_td3.h restated on the host (not a test module), from the header alone: nothing here reads a kernel constant.

Networks, losses, gradients, Adam and Polyak: torch autograd on the CPU, float64 by default (Ref(dtype=torch.float32) is the same
arithmetic in float32 -- another summation order than the device's, the yardstick of the float32 tolerances).
The replay ring, the sampling indices and the three random streams: NumPy on tests/noise_ref.philox4x32_10."""
import numpy as np
import torch

from noise_ref import philox4x32_10

U8, U11, U21, S32 = np.uint64(8), np.uint64(11), np.uint64(21), np.uint64(32)
STREAM_EXPLORE, STREAM_SAMPLE, STREAM_SMOOTH = 4, 5, 6
STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "policy_loss", "W", "critic_grad_norm", "policy_grad_norm")


def _key(seed):
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return seed & 0xFFFFFFFF, seed >> 32


# ---- the streams -----------------------------------------------------------------------------
def pair_uniforms(w, dtype):
    """(u1, u2) of a Box-Muller pair as float64 values, the actor's forms per dtype"""
    w0, w1, w2, w3 = w
    if np.dtype(dtype) == np.float32:
        return ((w0 >> U8).astype(np.float64) + 0.5) * 2.0 ** -24, (w1 >> U8).astype(np.float64) * 2.0 ** -24
    r1, r2 = (w0 << U21) ^ (w1 >> U11), (w2 << U21) ^ (w3 >> U11)
    return (r1.astype(np.float64) + 0.5) * 2.0 ** -53, r2.astype(np.float64) * 2.0 ** -53


def single_uniform(w, dtype):
    w0, w1, _, _ = w
    if np.dtype(dtype) == np.float32:
        return (w0 >> U8).astype(np.float64) * 2.0 ** -24
    return ((w0 << U21) ^ (w1 >> U11)).astype(np.float64) * 2.0 ** -53


def normals(seed, c0, c1, n, stream, dtype):
    """z [len(c0), n] in float64: components 2j, 2j + 1 from the words at counter (c0, c1, j, stream)"""
    k0, k1 = _key(seed)
    c0 = np.asarray(c0, dtype=np.int64)
    c1 = np.broadcast_to(np.asarray(c1, dtype=np.int64), c0.shape)
    z = np.zeros((c0.size, n))
    for j in range((n + 1) // 2):
        u1, u2 = pair_uniforms(philox4x32_10(c0, c1, j, stream, k0, k1), dtype)
        radius, angle = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        z[:, 2 * j] = radius * np.cos(angle)
        if 2 * j + 1 < n:
            z[:, 2 * j + 1] = radius * np.sin(angle)
    return z


def explore_normals(seed, replica_offset, counters, n, dtype):
    """stream 4 at (replica_offset + b, counters[b], j, 4)"""
    b = np.arange(len(counters), dtype=np.int64) + int(replica_offset)
    return normals(seed, b, counters, n, STREAM_EXPLORE, dtype)


def explore_uniforms(seed, replica_offset, counters, n, dtype):
    """u [B, n] in [0, 1): the single uniform of stream 4 at index j = the action component"""
    k0, k1 = _key(seed)
    b = np.arange(len(counters), dtype=np.int64) + int(replica_offset)
    return np.stack([single_uniform(philox4x32_10(b, np.asarray(counters, dtype=np.int64), j, STREAM_EXPLORE, k0, k1), dtype) for j in range(n)], axis=1)


def smooth_normals(seed, m, ctr, n, dtype):
    """stream 6 at (i, ctr, j, 6), i the minibatch row"""
    return normals(seed, np.arange(m, dtype=np.int64), int(ctr), n, STREAM_SMOOTH, dtype)


def sample_idx(m, seed, stored, drawn):
    """idx [m]: mulhi32(w0, max(stored, 1)) with w0 word 0 of stream 5 at (i, drawn, 0, 5)"""
    k0, k1 = _key(seed)
    w0 = philox4x32_10(np.arange(m, dtype=np.int64), int(drawn) & 0xFFFFFFFF, 0, STREAM_SAMPLE, k0, k1)[0]
    return ((w0 * np.uint64(max(int(stored), 1))) >> S32).astype(np.int64)


# ---- the ring ------------------------------------------------------------------------------------
class Ring(object):
    """The replay memory of the header in NumPy: head [4], obs, act, rwd, next_obs, boot, live"""

    def __init__(self, capacity, obs_dim, act_dim, dtype=np.float64):
        C = self.C = int(capacity)
        self.head = np.zeros(4, dtype=np.int32)
        self.obs, self.next_obs = np.zeros((C, obs_dim), dtype), np.zeros((C, obs_dim), dtype)
        self.act, self.rwd = np.zeros((C, act_dim), dtype), np.zeros(C, dtype)
        self.boot, self.live = np.zeros(C, np.uint8), np.zeros(C, np.uint8)

    def append(self, obs, act, rwd, done, trunc, valid, final_obs, cursor):
        """obs [T + 1, B, od], act [T, B, ad], rwd, done, trunc, valid [T, B], final_obs [T, B, od], cursor: the steps recorded"""
        T, B = rwd.shape
        assert T * B <= self.C
        n = min(max(int(cursor), 0), T)
        h0 = int(self.head[0])
        for t in range(n):
            for b in range(B):
                s = (h0 + t * B + b) % self.C
                fin = bool(done[t, b]) or bool(trunc[t, b])
                self.obs[s], self.act[s], self.rwd[s] = obs[t, b], act[t, b], rwd[t, b]
                self.next_obs[s] = final_obs[t, b] if fin else obs[t + 1, b]
                self.boot[s] = 1 if (not fin or bool(trunc[t, b])) else 0
                self.live[s] = 1 if valid[t, b] else 0
        self.head[0] = (h0 + n * B) % self.C
        self.head[1] = min(int(self.head[1]) + n * B, self.C)
        self.head[2] = np.int32(np.uint32((int(np.uint32(self.head[2])) + n * B) & 0xFFFFFFFF))
        return self

    def sample(self, m, seed):
        idx = sample_idx(m, seed, int(self.head[1]), int(np.uint32(self.head[3])))
        self.head[3] = np.int32(np.uint32((int(np.uint32(self.head[3])) + 1) & 0xFFFFFFFF))
        return idx

    def gather(self, idx):
        """the minibatch as a dict of float64 arrays; w = live"""
        idx = np.asarray(idx)
        return {"s": self.obs[idx].astype(np.float64), "a": self.act[idx].astype(np.float64), "r": self.rwd[idx].astype(np.float64),
                "s2": self.next_obs[idx].astype(np.float64), "boot": self.boot[idx].astype(np.float64), "w": (self.live[idx] != 0).astype(np.float64)}


# ---- networks, losses, Adam ----------------------------------------------------------------------
def segment_names(n_hidden, n_critics):
    return ["%s_%s%d" % (net, k, l) for net in ("mu", "q1", "q2")[:1 + n_critics] for l in range(n_hidden + 1) for k in ("w", "b")]


class Ref(object):
    """weights, target: {segment name: array / tensor} (matrices [out, in]); both are copied"""

    def __init__(self, obs_dim, act_dim, hidden, activation, low, high, n_critics, weights, target=None, dtype=torch.float64):
        self.od, self.ad, self.hidden, self.activation, self.n_critics, self.dtype = obs_dim, act_dim, tuple(hidden), activation, n_critics, dtype
        self.low, self.high = float(low), float(high)
        self.c, self.h = (self.high + self.low) / 2.0, (self.high - self.low) / 2.0
        self.names = segment_names(len(self.hidden), n_critics)
        cp = lambda d: {k: torch.as_tensor(np.asarray(d[k]), dtype=torch.float64).to(dtype).clone() for k in self.names}
        self.W, self.Wt = cp(weights), cp(target if target is not None else weights)
        self.m = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.steps = [0, 0]
        self.min_pre = np.inf                 # relu: the smallest |pre-activation| of a live row seen since reset_margins()

    def names_of(self, which):
        return [k for k in self.names if k.startswith("mu") == (which == 1)]

    def mlp(self, W, net, x, live=None):
        for l in range(len(self.hidden)):
            x = x @ W["%s_w%d" % (net, l)].T + W["%s_b%d" % (net, l)]
            if self.activation == "relu":
                if live is not None and bool(live.any()):
                    self.min_pre = min(self.min_pre, float(x.detach()[live].abs().min()))
                x = torch.relu(x)
            else:
                x = torch.tanh(x)
        L = len(self.hidden)
        return x @ W["%s_w%d" % (net, L)].T + W["%s_b%d" % (net, L)]

    def mu(self, W, s, live=None):
        return self.c + self.h * torch.tanh(self.mlp(W, "mu", s, live))

    def q(self, W, i, s, a, live=None):
        return self.mlp(W, "q%d" % (i + 1), torch.cat([s, a], dim=1), live)[:, 0]

    def _batch(self, batch):
        w = torch.as_tensor(batch["w"], dtype=torch.float64)
        live = w > 0
        t = {}
        for k in ("s", "a", "r", "s2", "boot"):
            x = torch.as_tensor(batch[k], dtype=torch.float64)
            x = torch.where(live.view(-1, *([1] * (x.dim() - 1))), x, torch.zeros_like(x))      # a dead row is staged as zeros
            t[k] = x.to(self.dtype)
        return t, w.to(self.dtype), live

    def _leaves(self):
        return {k: v.clone().requires_grad_(True) for k, v in self.W.items()}

    def critic(self, batch, z, gamma, target_noise, noise_clip):
        """dict: loss, grads (q segments), stats, and the margins of the non-smooth points over the live rows: `twin` |Q'_1 - Q'_2|,
        `noise` the distance of sigma z from +-c_noise, `bound` of mu' + h eps from low / high; the arrays `noise_raw`, `a_raw` for
        a case that means to hit a clamp"""
        t, w, live = self._batch(batch)
        z = torch.as_tensor(z, dtype=torch.float64).to(self.dtype)
        with torch.no_grad():
            raw = target_noise * z
            eps = raw.clamp(-noise_clip, noise_clip)
            a_raw = self.mu(self.Wt, t["s2"], live) + self.h * eps
            a2 = a_raw.clamp(self.low, self.high)
            qt = [self.q(self.Wt, i, t["s2"], a2, live) for i in range(self.n_critics)]
            qmin = qt[0] if self.n_critics == 1 else torch.minimum(qt[0], qt[1])
            y = t["r"] + gamma * t["boot"] * qmin
        Wl = self._leaves()
        Wsum = torch.clamp(w.sum(), min=1.0)
        qs = [self.q(Wl, i, t["s"], t["a"], live) for i in range(self.n_critics)]
        loss = sum((w * (q - y) ** 2).sum() for q in qs) / Wsum
        names = self.names_of(0)
        grads = dict(zip(names, torch.autograd.grad(loss, [Wl[k] for k in names])))
        lv = live.numpy()
        f = lambda x: x.detach().to(torch.float64).numpy()
        margins = {"twin": float(np.abs(f(qt[0]) - f(qt[1]))[lv].min()) if self.n_critics == 2 and lv.any() else np.inf,
                   "noise": float(np.abs(np.abs(f(raw)) - noise_clip)[lv].min()) if lv.any() and target_noise > 0 else np.inf,
                   "bound": float(np.minimum(np.abs(f(a_raw) - self.low), np.abs(f(a_raw) - self.high))[lv].min()) if lv.any() else np.inf}
        loss_v = float(loss.detach())
        stats = {"critic_loss": loss_v, "q1_mean": float((w * qs[0].detach()).sum() / Wsum),
                 "q2_mean": float((w * qs[1].detach()).sum() / Wsum) if self.n_critics == 2 else 0.0, "target_mean": float((w * y).sum() / Wsum),
                 "W": float(Wsum), "critic_grad_norm": float(torch.sqrt(sum((g.to(torch.float64) ** 2).sum() for g in grads.values())))}
        return {"loss": loss_v, "grads": grads, "stats": stats, "margins": margins, "y": f(y), "noise_raw": f(raw), "a_raw": f(a_raw),
                "row_term_max": float(max(float(((q.detach() - y) ** 2)[live].abs().max()) if lv.any() else 0.0 for q in qs))}

    def policy(self, batch):
        """dict: loss = -sum w Q_1(s, mu(s)) / W, grads (mu segments), stats"""
        t, w, live = self._batch(batch)
        Wl = self._leaves()
        Wsum = torch.clamp(w.sum(), min=1.0)
        q = self.q(Wl, 0, t["s"], self.mu(Wl, t["s"], live), live)
        loss = -(w * q).sum() / Wsum
        names = self.names_of(1)
        grads = dict(zip(names, torch.autograd.grad(loss, [Wl[k] for k in names])))
        stats = {"policy_loss": float(loss.detach()), "W": float(Wsum),
                 "policy_grad_norm": float(torch.sqrt(sum((g.to(torch.float64) ** 2).sum() for g in grads.values())))}
        return {"loss": float(loss.detach()), "grads": grads, "stats": stats}

    def adam(self, which, grads, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0):
        """the formula of include/beacon_learner.h on the segments of optimiser `which` (0 critic, 1 policy)"""
        names = self.names_of(which)
        norm = float(torch.sqrt(sum((grads[k].to(torch.float64) ** 2).sum() for k in names)))
        scale = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 else 1.0
        self.steps[which] += 1
        t = self.steps[which]
        step_size, bc2 = lr / (1.0 - betas[0] ** t), np.sqrt(1.0 - betas[1] ** t)
        for k in names:
            g = grads[k] * scale
            self.m[k] = self.m[k] + (1.0 - betas[0]) * (g - self.m[k])
            self.v[k] = betas[1] * self.v[k] + (1.0 - betas[1]) * g * g
            self.W[k] = self.W[k] - step_size * (self.m[k] / (torch.sqrt(self.v[k]) / bc2 + eps))

    def polyak(self, tau):
        for k in self.names:
            self.Wt[k] = self.Wt[k] + tau * (self.W[k] - self.Wt[k])

    def act(self, obs, z, sigma):
        """(mu, noisy action) for rows obs and draws z"""
        with torch.no_grad():
            mu = self.mu(self.W, torch.as_tensor(obs, dtype=torch.float64).to(self.dtype))
            a = (mu + self.h * sigma * torch.as_tensor(z, dtype=torch.float64).to(self.dtype)).clamp(self.low, self.high)
        return mu.to(torch.float64).numpy(), a.to(torch.float64).numpy()


def random_weights(obs_dim, act_dim, hidden, n_critics, seed, scale=1.0):
    """{segment name: float64 array}: N(0, scale^2 / in) matrices and small biases"""
    rng = np.random.default_rng(seed)
    out = {}
    for net, first, head in (("mu", obs_dim, act_dim), ("q1", obs_dim + act_dim, 1), ("q2", obs_dim + act_dim, 1))[:1 + n_critics]:
        dims = [first] + list(hidden) + [head]
        for l in range(len(hidden) + 1):
            out["%s_w%d" % (net, l)] = rng.standard_normal((dims[l + 1], dims[l])) * scale / np.sqrt(dims[l])
            out["%s_b%d" % (net, l)] = rng.standard_normal(dims[l + 1]) * 0.1
    return out

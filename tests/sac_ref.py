"""include/beacon_sac.h restated on the host (not a test module), from the header alone: nothing here reads a kernel constant.

The policy, log pi, both losses and the temperature's: torch on the CPU, autograd gives the gradients; float64 by default
(Ref(dtype=torch.float32) is the same arithmetic in float32 -- another summation order than the device's, the yardstick of the
float32 tolerances).  Adam and Polyak as written in the header.  The three random streams (7 acting, 8 the critic step's next action,
9 the policy step's draw): NumPy on tests/noise_ref.philox4x32_10, through the pair and single-uniform forms of tests/td3_ref.py; the
replay ring and its sampling (stream 5) ARE td3_ref's, as the memory is libbeacon_td3.so's."""
import math

import numpy as np
import torch

from noise_ref import philox4x32_10
from td3_ref import Ring, _key, normals, sample_idx, single_uniform  # noqa: F401  (Ring and sample_idx: for the tests)

STREAM_ACT, STREAM_NEXT, STREAM_PI = 7, 8, 9
LS_MIN, LS_MAX = -20.0, 2.0
STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "policy_loss", "W", "critic_grad_norm", "policy_grad_norm", "logp_mean",
         "next_logp_mean", "alpha", "alpha_grad")


# ---- the streams -----------------------------------------------------------------------------
def act_normals(seed, replica_offset, counters, n, dtype):
    """stream 7 at (replica_offset + b, counters[b], j, 7)"""
    b = np.arange(len(counters), dtype=np.int64) + int(replica_offset)
    return normals(seed, b, counters, n, STREAM_ACT, dtype)


def act_uniforms(seed, replica_offset, counters, n, dtype):
    """u [B, n] in [0, 1): the single uniform of stream 7 at index j = the action component"""
    k0, k1 = _key(seed)
    b = np.arange(len(counters), dtype=np.int64) + int(replica_offset)
    return np.stack([single_uniform(philox4x32_10(b, np.asarray(counters, dtype=np.int64), j, STREAM_ACT, k0, k1), dtype) for j in range(n)], axis=1)


def next_normals(seed, m, ctr, n, dtype):
    """stream 8 at (i, ctr, j, 8), i the minibatch row, ctr = step[3]"""
    return normals(seed, np.arange(m, dtype=np.int64), int(ctr), n, STREAM_NEXT, dtype)


def pi_normals(seed, m, ctr, n, dtype):
    """stream 9 at (i, ctr, j, 9), ctr = step[4]"""
    return normals(seed, np.arange(m, dtype=np.int64), int(ctr), n, STREAM_PI, dtype)


# ---- the squashed Gaussian ---------------------------------------------------------------------
def softplus(x):
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def squash(head, z, c, h):
    """(a [m, n], log pi [m], u, raw log-std) from the head's outputs [m, 2n] and the draws z [m, n]: the header's formulas"""
    n = head.shape[1] // 2
    mean, raw = head[:, :n], head[:, n:]
    ls = raw.clamp(LS_MIN, LS_MAX)
    u = mean + torch.exp(ls) * z
    a = c + h * torch.tanh(u)
    lp = (((-0.5 * z * z - ls) - 0.5 * math.log(2.0 * math.pi)) - math.log(h)) - 2.0 * ((math.log(2.0) - u) - softplus(-2.0 * u))
    return a, lp.sum(dim=1), u, raw


# ---- networks, losses, Adam ----------------------------------------------------------------------
def segment_names(n_hidden, n_critics):
    return ["%s_%s%d" % (net, k, l) for net in ("pi", "q1", "q2")[:1 + n_critics] for l in range(n_hidden + 1) for k in ("w", "b")] + ["log_alpha"]


class Ref(object):
    """weights, target: {segment name: array / tensor} (matrices [out, in]; log_alpha [1]); both are copied"""

    def __init__(self, obs_dim, act_dim, hidden, activation, low, high, n_critics, weights, target=None, dtype=torch.float64):
        self.od, self.ad, self.hidden, self.activation, self.n_critics, self.dtype = obs_dim, act_dim, tuple(hidden), activation, n_critics, dtype
        self.low, self.high = float(low), float(high)
        self.c, self.h = (self.high + self.low) / 2.0, (self.high - self.low) / 2.0
        self.names = segment_names(len(self.hidden), n_critics)
        cp = lambda d: {k: torch.as_tensor(np.asarray(d[k]), dtype=torch.float64).reshape(np.asarray(d[k]).shape).to(dtype).clone() for k in self.names}
        self.W, self.Wt = cp(weights), cp(target if target is not None else weights)
        self.m = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.steps = [0, 0, 0]
        self.min_pre = np.inf                 # relu: the smallest |pre-activation| of a live row seen since construction

    def names_of(self, which):
        """the segments of optimiser `which`: 0 critic, 1 policy, 2 alpha"""
        if which == 2:
            return ["log_alpha"]
        return [k for k in self.names if k != "log_alpha" and k.startswith("pi") == (which == 1)]

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

    def pi(self, W, s, z, live=None):
        """(a, log pi, u, raw log-std) for rows s and draws z"""
        return squash(self.mlp(W, "pi", s, live), z, self.c, self.h)

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

    def _z(self, z):
        return torch.as_tensor(z, dtype=torch.float64).to(self.dtype)

    def _clamp_margin(self, raw, lv):
        raw = raw.detach().to(torch.float64).numpy()
        return float(np.minimum(np.abs(raw - LS_MIN), np.abs(raw - LS_MAX))[lv].min()) if lv.any() else np.inf

    def critic(self, batch, z, gamma):
        """dict: loss, grads (q segments), stats, and over the live rows the margins of the non-smooth points: `twin` |Q'_1 - Q'_2|,
        `clamp` the distance of the raw log-std of pi(s') from -20 and 2; the arrays `raw` and `u` of the next action's draw"""
        t, w, live = self._batch(batch)
        lv = live.numpy()
        with torch.no_grad():
            alpha = torch.exp(self.W["log_alpha"][0])
            a2, lp2, u2, raw2 = self.pi(self.W, t["s2"], self._z(z), live)          # the CURRENT policy
            qt = [self.q(self.Wt, i, t["s2"], a2, live) for i in range(self.n_critics)]
            qmin = qt[0] if self.n_critics == 1 else torch.minimum(qt[0], qt[1])
            y = t["r"] + gamma * t["boot"] * (qmin - alpha * lp2)
        Wl = self._leaves()
        Wsum = torch.clamp(w.sum(), min=1.0)
        qs = [self.q(Wl, i, t["s"], t["a"], live) for i in range(self.n_critics)]
        loss = sum((w * (q - y) ** 2).sum() for q in qs) / Wsum
        names = self.names_of(0)
        grads = dict(zip(names, torch.autograd.grad(loss, [Wl[k] for k in names])))
        f = lambda x: x.detach().to(torch.float64).numpy()
        margins = {"twin": float(np.abs(f(qt[0]) - f(qt[1]))[lv].min()) if self.n_critics == 2 and lv.any() else np.inf,
                   "clamp": self._clamp_margin(raw2, lv)}
        loss_v = float(loss.detach())
        stats = {"critic_loss": loss_v, "q1_mean": float((w * qs[0].detach()).sum() / Wsum),
                 "q2_mean": float((w * qs[1].detach()).sum() / Wsum) if self.n_critics == 2 else 0.0, "target_mean": float((w * y).sum() / Wsum),
                 "W": float(Wsum), "critic_grad_norm": float(torch.sqrt(sum((g.to(torch.float64) ** 2).sum() for g in grads.values()))),
                 "next_logp_mean": float((w * lp2).sum() / Wsum), "alpha": float(alpha)}
        terms = [((q.detach() - y) ** 2)[live] for q in qs] + [lp2[live].abs(), y[live].abs()]
        return {"loss": loss_v, "grads": grads, "stats": stats, "margins": margins, "y": f(y), "raw": f(raw2), "u": f(u2), "logp": f(lp2),
                "row_term_max": float(max(float(x.abs().max()) for x in terms)) if lv.any() else 0.0}

    def policy(self, batch, z, target_entropy):
        """dict: loss = sum w (alpha log pi - min_i Q_i(s, a~)) / W with alpha a constant, grads (pi segments, and log_alpha: the
        gradient of -log_alpha sum w (log pi + target_entropy) / W with log pi a constant), stats, margins (`twin` |Q_1 - Q_2| at a~,
        `clamp`), the arrays `raw`, `u`, `logp`"""
        t, w, live = self._batch(batch)
        lv = live.numpy()
        Wl = self._leaves()
        Wsum = torch.clamp(w.sum(), min=1.0)
        alpha = torch.exp(self.W["log_alpha"][0]).detach()
        a, lp, u, raw = self.pi(Wl, t["s"], self._z(z), live)
        qs = [self.q(Wl, i, t["s"], a, live) for i in range(self.n_critics)]
        qmin = qs[0] if self.n_critics == 1 else torch.where(qs[1] < qs[0], qs[1], qs[0])       # Q_2 only where strictly smaller
        loss = (w * (alpha * lp - qmin)).sum() / Wsum
        names = self.names_of(1)
        grads = dict(zip(names, torch.autograd.grad(loss, [Wl[k] for k in names])))
        la = Wl["log_alpha"]
        alpha_loss = -(la[0] * (w * (lp.detach() + target_entropy)).sum()) / Wsum
        grads["log_alpha"] = torch.autograd.grad(alpha_loss, [la])[0]
        f = lambda x: x.detach().to(torch.float64).numpy()
        margins = {"twin": float(np.abs(f(qs[0]) - f(qs[1]))[lv].min()) if self.n_critics == 2 and lv.any() else np.inf,
                   "clamp": self._clamp_margin(raw, lv)}
        pnorm = float(torch.sqrt(sum((grads[k].to(torch.float64) ** 2).sum() for k in names)))
        stats = {"policy_loss": float(loss.detach()), "W": float(Wsum), "policy_grad_norm": pnorm, "logp_mean": float((w * lp.detach()).sum() / Wsum),
                 "alpha": float(alpha), "alpha_grad": float(grads["log_alpha"][0])}
        terms = [lp.detach()[live].abs(), qmin.detach()[live].abs()]
        return {"loss": float(loss.detach()), "alpha_loss": float(alpha_loss.detach()), "grads": grads, "stats": stats, "margins": margins,
                "raw": f(raw), "u": f(u), "logp": f(lp), "row_term_max": float(max(float(x.max()) for x in terms)) if lv.any() else 0.0}

    def adam(self, which, grads, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0):
        """the formula of include/beacon_learner.h on the segments of optimiser `which` (0 critic, 1 policy, 2 alpha: never clipped)"""
        names = self.names_of(which)
        norm = float(torch.sqrt(sum((grads[k].to(torch.float64) ** 2).sum() for k in names)))
        scale = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 and which != 2 else 1.0
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

    def act(self, obs, z):
        """(deterministic action c + h tanh(mean), sampled action) for rows obs and draws z, as float64 arrays"""
        with torch.no_grad():
            s = torch.as_tensor(obs, dtype=torch.float64).to(self.dtype)
            head = self.mlp(self.W, "pi", s)
            det = self.c + self.h * torch.tanh(head[:, :self.ad])
            a = squash(head, self._z(z), self.c, self.h)[0]
        return det.to(torch.float64).numpy(), a.to(torch.float64).numpy()


def random_weights(obs_dim, act_dim, hidden, n_critics, seed, scale=1.0, alpha=0.7):
    """{segment name: float64 array}: N(0, scale^2 / in) matrices and small biases; log_alpha = ln(alpha)"""
    rng = np.random.default_rng(seed)
    out = {}
    for net, first, head in (("pi", obs_dim, 2 * act_dim), ("q1", obs_dim + act_dim, 1), ("q2", obs_dim + act_dim, 1))[:1 + n_critics]:
        dims = [first] + list(hidden) + [head]
        for l in range(len(hidden) + 1):
            out["%s_w%d" % (net, l)] = rng.standard_normal((dims[l + 1], dims[l])) * scale / np.sqrt(dims[l])
            out["%s_b%d" % (net, l)] = rng.standard_normal(dims[l + 1]) * 0.1
    out["log_alpha"] = np.array([np.log(alpha)])
    return out

"""include/beacon_dqn.h restated on the host (not a test module), from the header alone: nothing here reads a kernel constant.

The network with and without the dueling head, both targets, both losses, the gradient, Adam and Polyak: torch autograd on the CPU,
float64 by default (Ref(dtype=torch.float32) is the same arithmetic in float32 -- another summation order than the device's, the
yardstick of the float32 tolerances).  The first-maximum rule, stream 10 and the append of int32 actions: NumPy on
tests/noise_ref.philox4x32_10.  The ring and stream 5 are tests/td3_ref.py's."""
import numpy as np
import torch

from noise_ref import philox4x32_10
from td3_ref import Ring, _key, sample_idx, single_uniform  # noqa: F401  (Ring, sample_idx: re-exported for the tests)

S32 = np.uint64(32)
STREAM_ACT = 10
STATS = ("loss", "q_mean", "target_mean", "td_abs_mean", "W", "grad_norm", "q_max_mean", "spare")
GREEDY, EPSILON, UNIFORM = "greedy", "epsilon", "uniform"


# ---- the first maximum ----------------------------------------------------------------------------
def first_argmax(q):
    """arg [m] of q [m, n] by the header's rule: best = -inf, arg = 0; for j ascending q_j replaces best only where q_j > best
    strictly.  A NaN never wins; a row of NaN (or of -inf) gives 0."""
    q = np.asarray(q, dtype=np.float64)
    best, arg = np.full(q.shape[0], -np.inf), np.zeros(q.shape[0], dtype=np.int64)
    for j in range(q.shape[1]):
        with np.errstate(invalid="ignore"):
            take = q[:, j] > best
        best, arg = np.where(take, q[:, j], best), np.where(take, j, arg)
    return arg


def top_two_gap(q):
    """[m]: the distance between the largest and the second largest entry of every row of q [m, n]"""
    s = np.sort(np.asarray(q, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ---- stream 10 ---------------------------------------------------------------------------------
def act_draws(seed, replica_offset, counters, n, dtype):
    """(u [B] in [0, 1) as float64, rnd [B] in 0 .. n - 1) from the words at (replica_offset + b, counters[b], 0, 10)"""
    k0, k1 = _key(seed)
    b = (np.arange(len(counters), dtype=np.int64) + int(replica_offset)) & 0xFFFFFFFF
    w = philox4x32_10(b, np.asarray(counters, dtype=np.int64) & 0xFFFFFFFF, 0, STREAM_ACT, k0, k1)
    return single_uniform(w, dtype), ((w[3] * np.uint64(n)) >> S32).astype(np.int64)


def act(q, u, rnd, mode, eps=0.0):
    """actions [B] for Q values q [B, n] (ignored in the uniform mode) and the draws"""
    if mode == UNIFORM:
        return np.asarray(rnd).copy()
    g = first_argmax(q)
    return g if mode == GREEDY else np.where(np.asarray(u) < eps, rnd, g)


# ---- the append of int32 actions -----------------------------------------------------------------
def append_int(ring, obs, act_i, rwd, done, trunc, valid, final_obs, cursor):
    """bcn_dqn_append: td3_ref.Ring.append (a ring with act_dim = 1) with the int32 [T, B] actions converted, (real)a"""
    act_i = np.asarray(act_i)
    assert act_i.dtype == np.int32 and act_i.shape == rwd.shape
    return ring.append(obs, act_i.astype(ring.act.dtype)[:, :, None], rwd, done, trunc, valid, final_obs, cursor)


# ---- the network, the loss, Adam ----------------------------------------------------------------
def segment_names(n_hidden):
    return ["q_%s%d" % (k, l) for l in range(n_hidden + 1) for k in ("w", "b")]


class Ref(object):
    """weights, target: {segment name: array / tensor} (matrices [out, in]; the head [n + dueling, h_last]); both are copied"""

    def __init__(self, obs_dim, n_actions, hidden, activation, dueling, weights, target=None, dtype=torch.float64):
        self.od, self.n, self.hidden, self.activation, self.dueling, self.dtype = obs_dim, n_actions, tuple(hidden), activation, bool(dueling), dtype
        self.names = segment_names(len(self.hidden))
        cp = lambda d: {k: torch.as_tensor(np.asarray(d[k]), dtype=torch.float64).to(dtype).clone() for k in self.names}
        self.W, self.Wt = cp(weights), cp(target if target is not None else weights)
        self.m = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.W.items()}
        self.steps = 0
        self.min_pre = np.inf                 # relu: the smallest |pre-activation| of a live row seen since it was last reset

    def head(self, W, x, live=None):
        for l in range(len(self.hidden)):
            x = x @ W["q_w%d" % l].T + W["q_b%d" % l]
            if self.activation == "relu":
                if live is not None and bool(live.any()):
                    self.min_pre = min(self.min_pre, float(x.detach()[live].abs().min()))
                x = torch.relu(x)
            else:
                x = torch.tanh(x)
        L = len(self.hidden)
        return x @ W["q_w%d" % L].T + W["q_b%d" % L]

    def q(self, W, x, live=None):
        """Q [rows, n]: head_j, or (V + A_j) - (sum_k A_k) / n"""
        h = self.head(W, x, live)
        if not self.dueling:
            return h
        A, V = h[:, :self.n], h[:, self.n:self.n + 1]
        return (V + A) - A.sum(dim=1, keepdim=True) / self.n

    def q_values(self, obs, target=False):
        with torch.no_grad():
            return self.q(self.Wt if target else self.W, torch.as_tensor(obs, dtype=torch.float64).to(self.dtype)).to(torch.float64).numpy()

    def _batch(self, batch):
        a = np.asarray(batch["a"], dtype=np.float64).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok = (a >= 0) & (a < self.n) & (np.floor(a) == a)
        w = torch.as_tensor(np.asarray(batch["w"], dtype=np.float64) * ok, dtype=torch.float64)       # an action outside 0 .. n - 1: a dead row
        live = w > 0
        t = {}
        for k in ("s", "r", "s2", "boot"):
            x = torch.as_tensor(batch[k], dtype=torch.float64)
            x = torch.where(live.view(-1, *([1] * (x.dim() - 1))), x, torch.zeros_like(x))      # a dead row is staged as zeros
            t[k] = x.to(self.dtype)
        t["a"] = torch.as_tensor(np.where(live.numpy(), np.nan_to_num(a), 0.0).astype(np.int64))
        return t, w.to(self.dtype), live

    def _leaves(self):
        return {k: v.clone().requires_grad_(True) for k, v in self.W.items()}

    def loss(self, batch, gamma, double=True, huber=None):
        """dict: loss, grads, stats, y, delta, and over the live rows the margins of the non-smooth points: `gap_online` the top-two gap
        of Q(s'; params) (double only), `gap_target` of Q(s'; target) (plain only), `huber` ||delta| - kappa|, `gap_qmax` of Q(s;
        params) (a statistic only); per-row arrays of the gaps for a case that means to hit a tie"""
        t, w, live = self._batch(batch)
        lv = live.numpy()
        f = lambda x: x.detach().to(torch.float64).numpy()
        rows = torch.arange(len(w))
        with torch.no_grad():
            qt = self.q(self.Wt, t["s2"], live)
            if double:
                qo = self.q(self.W, t["s2"], live)
                jstar = torch.as_tensor(first_argmax(f(qo)))
                gaps = {"gap_online": top_two_gap(f(qo))}
            else:
                jstar = torch.as_tensor(first_argmax(f(qt)))
                gaps = {"gap_target": top_two_gap(f(qt))}
            y = t["r"] + (gamma * t["boot"]) * qt[rows, jstar]
            y = torch.where(live, y, torch.zeros_like(y))
        Wl = self._leaves()
        Wsum = torch.clamp(w.sum(), min=1.0)
        qs = self.q(Wl, t["s"], live)
        qa = qs[rows, t["a"]]
        delta = qa - y
        if huber is None:
            row = 0.5 * delta * delta
        else:
            ad = delta.abs()
            row = torch.where(ad <= huber, 0.5 * delta * delta, huber * (ad - 0.5 * huber))
        loss = (w * row).sum() / Wsum
        grads = dict(zip(self.names, torch.autograd.grad(loss, [Wl[k] for k in self.names])))
        qmax = f(qs)[np.arange(len(lv)), first_argmax(f(qs))]
        wn, Wn = f(w), float(Wsum)
        stats = {"loss": float(loss.detach()), "q_mean": float((wn * f(qa)).sum() / Wn), "target_mean": float((wn * f(y)).sum() / Wn),
                 "td_abs_mean": float((wn * np.abs(f(delta))).sum() / Wn), "W": Wn,
                 "grad_norm": float(torch.sqrt(sum((g.to(torch.float64) ** 2).sum() for g in grads.values()))),
                 "q_max_mean": float((wn * qmax).sum() / Wn), "spare": 0.0}
        mn = lambda x: float(x[lv].min()) if lv.any() else np.inf
        margins = {k: mn(v) for k, v in gaps.items()}
        margins["gap_qmax"] = mn(top_two_gap(f(qs)))
        margins["huber"] = mn(np.abs(np.abs(f(delta)) - huber)) if huber is not None else np.inf
        return {"loss": float(loss.detach()), "grads": grads, "stats": stats, "margins": margins, "gaps": dict(gaps, gap_qmax=top_two_gap(f(qs))),
                "y": f(y), "delta": f(delta), "live": lv, "jstar": jstar.numpy(),
                "row_term_max": float(f(row)[lv].max()) if lv.any() else 0.0}

    def adam(self, grads, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0):
        """the formula of include/beacon_learner.h over all segments"""
        norm = float(torch.sqrt(sum((grads[k].to(torch.float64) ** 2).sum() for k in self.names)))
        scale = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 else 1.0
        self.steps += 1
        t = self.steps
        step_size, bc2 = lr / (1.0 - betas[0] ** t), np.sqrt(1.0 - betas[1] ** t)
        for k in self.names:
            g = grads[k] * scale
            self.m[k] = self.m[k] + (1.0 - betas[0]) * (g - self.m[k])
            self.v[k] = betas[1] * self.v[k] + (1.0 - betas[1]) * g * g
            self.W[k] = self.W[k] - step_size * (self.m[k] / (torch.sqrt(self.v[k]) / bc2 + eps))

    def polyak(self, tau):
        for k in self.names:
            self.Wt[k] = self.W[k].clone() if tau == 1.0 else self.Wt[k] + tau * (self.W[k] - self.Wt[k])


def random_weights(obs_dim, n_actions, hidden, dueling, seed, scale=1.0):
    """{segment name: float64 array}: N(0, scale^2 / in) matrices and small biases"""
    rng = np.random.default_rng(seed)
    out = {}
    dims = [obs_dim] + list(hidden) + [n_actions + int(bool(dueling))]
    for l in range(len(hidden) + 1):
        out["q_w%d" % l] = rng.standard_normal((dims[l + 1], dims[l])) * scale / np.sqrt(dims[l])
        out["q_b%d" % l] = rng.standard_normal(dims[l + 1]) * 0.1
    return out

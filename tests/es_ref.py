"""include/beacon_es.h restated on the host (not a test module), from the header alone: nothing here reads a kernel constant.

NumPy.  A Layout names the DEVICE's dtype -- it decides the segments' offsets and gaps, the form of the uniforms, and what sigma, the
weight decay and the Box's centre and half width are rounded to -- and the dtype of the ARITHMETIC, float64 by default.
arith=np.float32 runs the same formulas in float32 (the normals are formed in float64 from the float32 uniforms and rounded once; the
sums of a layer are NumPy's, another order than the device's): the yardstick of the float32 tolerances.  The stream is tests/noise_ref.philox4x32_10 through td3_ref.normals."""
import numpy as np

import td3_ref
from dqn_ref import first_argmax, top_two_gap  # noqa: F401  (the first-maximum rule of include/beacon_dqn.h)

STREAM_PERTURB = 11
PAIR_CHUNK = 64
STATS = ("fit_mean", "fit_std", "fit_min", "fit_max", "best_member", "nan_members", "grad_norm", "spare")


class Layout(object):
    """the parameter layout: segments pi_w0, pi_b0, ..., each 16-byte aligned; E elements including the gaps"""

    def __init__(self, obs_dim, hidden, n_out, dtype=np.float64, arith=np.float64):
        self.obs_dim, self.hidden, self.n_out, self.dtype = int(obs_dim), tuple(int(h) for h in hidden), int(n_out), np.dtype(dtype)
        self.arith = np.dtype(arith)
        esz = self.dtype.itemsize
        dims = [self.obs_dim] + list(self.hidden) + [self.n_out]
        self.names, self.shapes, self.offsets = [], {}, {}
        off = 0
        for l in range(len(self.hidden) + 1):
            for name, shape in (("pi_w%d" % l, (dims[l + 1], dims[l])), ("pi_b%d" % l, (dims[l + 1],))):
                off = (off + 15) & ~15
                self.names.append(name)
                self.shapes[name], self.offsets[name] = shape, off // esz
                off += int(np.prod(shape)) * esz
        self.E = ((off + 15) & ~15) // esz
        self.used = np.zeros(self.E, dtype=bool)
        for name in self.names:
            self.used[self.offsets[name]:self.offsets[name] + int(np.prod(self.shapes[name]))] = True

    def pack(self, weights):
        """{name: array} -> the vector [E] as the device holds it (rounded to its dtype), in the arithmetic's dtype; gaps 0"""
        v = np.zeros(self.E, dtype=self.arith)
        for name in self.names:
            a = np.asarray(weights[name], dtype=self.dtype).astype(self.arith).reshape(-1)
            assert a.size == int(np.prod(self.shapes[name])), name
            v[self.offsets[name]:self.offsets[name] + a.size] = a
        return v

    def unpack(self, v):
        v = np.asarray(v)
        return {name: v[..., self.offsets[name]:self.offsets[name] + int(np.prod(self.shapes[name]))].reshape(v.shape[:-1] + self.shapes[name])
                for name in self.names}


def random_weights(obs_dim, hidden, n_out, seed, scale=1.0):
    """{segment name: float64 array}: N(0, scale^2 / in) matrices and small biases"""
    rng = np.random.default_rng(seed)
    dims = [obs_dim] + list(hidden) + [n_out]
    out = {}
    for l in range(len(hidden) + 1):
        out["pi_w%d" % l] = rng.standard_normal((dims[l + 1], dims[l])) * scale / np.sqrt(dims[l])
        out["pi_b%d" % l] = rng.standard_normal(dims[l + 1]) * 0.1
    return out


# ---- noise, begin ------------------------------------------------------------------------------------
def eps(seed, gen, members, E, dtype):
    """eps [M / 2, E] as float64: component e & 1 of the pair at counter (j, gen, e >> 1, 11)"""
    return td3_ref.normals(seed, np.arange(members // 2), int(gen) & 0xFFFFFFFF, E, STREAM_PERTURB, dtype)


def perturb(theta, sigma, seed, gen, members, lay):
    """pop [M, E]: fma(s sigma, eps_j[e], theta[e]) on the segments, theta on the gaps; sigma = 0: theta"""
    dt = lay.arith
    theta = np.asarray(theta, dtype=dt)
    pop = np.tile(theta, (members, 1))
    sg = dt.type(lay.dtype.type(sigma))
    if sg == 0:
        return pop
    z = eps(seed, gen, members, lay.E, lay.dtype).astype(dt)
    pop[0::2] = np.where(lay.used, theta + sg * z, theta)
    pop[1::2] = np.where(lay.used, theta - sg * z, theta)
    return pop


# ---- the network ---------------------------------------------------------------------------------------
def heads(rows, obs, lay, activation):
    """head [B, n_out]: rows [B, E] the parameter row of every replica, obs [B, obs_dim]; in the layout's arithmetic.
    With relu also returns the smallest |pre-activation|."""
    dt = lay.arith
    W = lay.unpack(np.asarray(rows, dtype=dt))
    x = np.asarray(obs, dtype=dt)
    min_pre = np.inf
    for l in range(len(lay.hidden) + 1):
        x = np.einsum("bok,bk->bo", W["pi_w%d" % l], x) + W["pi_b%d" % l]
        if l < len(lay.hidden):
            if activation == "relu":
                min_pre = min(min_pre, float(np.abs(x).min()))
                x = np.maximum(x, 0)
            else:
                x = np.tanh(x)
    return x.astype(dt), min_pre


def act(rows, obs, lay, activation, kind, low=-1.0, high=1.0):
    """Box (kind 0): a [B, act_dim] = c + h tanh(head); Discrete (kind 1): the first maximum, int64 [B]"""
    h, _ = heads(rows, obs, lay, activation)
    if kind == 0:
        dt, dev = lay.arith.type, lay.dtype.type
        return dt(dev((high + low) / 2.0)) + dt(dev((high - low) / 2.0)) * np.tanh(h)
    return first_argmax(h)


def member_rows(pop, replicas):
    """[M R, E]: replica b under row b // R"""
    return np.repeat(np.asarray(pop), replicas, axis=0)


# ---- observe -----------------------------------------------------------------------------------------
def observe(fit, length, alive, rwd, done, trunc):
    """in place: where alive, fit += rwd, len += 1, and done | trunc ends the replica"""
    a = alive != 0
    with np.errstate(invalid="ignore"):
        fit[a] += np.asarray(rwd, dtype=np.float64)[a]
    length[a] += 1
    alive[a & ((np.asarray(done) != 0) | (np.asarray(trunc) != 0))] = 0


# ---- ranks, gradient, Adam ---------------------------------------------------------------------------------
def ranks(fit, members):
    """(member_fit [M] with NaN as -inf, util [M], stats dict without grad_norm) of fit [M R]"""
    fit = np.asarray(fit, dtype=np.float64).reshape(members, -1)
    R = fit.shape[1]
    F = np.zeros(members)
    for r in range(R):
        with np.errstate(invalid="ignore"):
            F = F + fit[:, r]
    F = F / R
    F = np.where(np.isnan(F), -np.inf, F)
    idx = np.arange(members)
    rank = np.array([int(((F < F[p]) | ((F == F[p]) & (idx < p))).sum()) for p in range(members)])
    util = rank / (members - 1) - 0.5
    ok = F > -np.inf
    n = int(ok.sum())
    if n:
        mean = float(F[ok].sum() / n)
        st = {"fit_mean": mean, "fit_std": float(np.sqrt(((F[ok] - mean) ** 2).sum() / n)), "fit_min": float(F[ok].min()),
              "fit_max": float(F[ok].max()), "best_member": float(np.flatnonzero(ok & (F == F[ok].max()))[0])}
    else:
        st = {"fit_mean": 0.0, "fit_std": 0.0, "fit_min": 0.0, "fit_max": 0.0, "best_member": 0.0}
    st["nan_members"], st["spare"] = float(members - n), 0.0
    return F, util, st


def gradient(util, theta, sigma, weight_decay, seed, gen, lay):
    """grad [E] in the layout's arithmetic: g = (sum_j (u_2j - u_2j+1) eps_j) / (M sigma) in float64, chunks of PAIR_CHUNK pairs,
    rounded once; grad = -g + weight_decay theta; gaps 0"""
    dt = lay.arith
    M = len(util)
    z = eps(seed, gen, M, lay.E, lay.dtype).astype(dt).astype(np.float64)
    du = np.asarray(util[0::2]) - np.asarray(util[1::2])
    total = np.zeros(lay.E)
    for c0 in range(0, M // 2, PAIR_CHUNK):
        part = np.zeros(lay.E)
        for j in range(c0, min(M // 2, c0 + PAIR_CHUNK)):
            part = part + du[j] * z[j]
        total = total + part
    g = (total / (M * float(lay.dtype.type(sigma)))).astype(dt)
    grad = -g + dt.type(lay.dtype.type(weight_decay)) * np.asarray(theta, dtype=dt)
    return np.where(lay.used, grad, dt.type(0)).astype(dt)


class Ref(object):
    """theta, Adam moments, the generation and step counters: begin() -> pop, update(fit) -> the step"""

    def __init__(self, lay, activation, kind, members, theta, seed, sigma, lr, weight_decay=0.0, betas=(0.9, 0.999), eps_adam=1e-8,
                 max_grad_norm=0.0, low=-1.0, high=1.0):
        self.lay, self.activation, self.kind, self.M, self.seed = lay, activation, kind, int(members), int(seed)
        self.sigma, self.lr, self.wd, self.betas, self.eps_adam, self.max_grad_norm = sigma, lr, weight_decay, betas, eps_adam, max_grad_norm
        self.low, self.high = low, high
        self.theta = np.array(theta, dtype=lay.arith)
        self.m, self.v = np.zeros_like(self.theta), np.zeros_like(self.theta)
        self.gen, self.steps = 0, 0
        self.pop = None

    def begin(self):
        self.pop = perturb(self.theta, self.sigma, self.seed, self.gen, self.M, self.lay)
        return self.pop

    def act(self, obs, shared=False):
        B = len(obs)
        rows = np.tile(self.theta, (B, 1)) if shared else member_rows(self.pop, B // self.M)
        return act(rows, obs, self.lay, self.activation, self.kind, self.low, self.high)

    def adam(self, grad):
        dt = self.lay.arith.type
        norm = float(np.sqrt((grad.astype(np.float64) ** 2).sum()))
        scale = min(1.0, self.max_grad_norm / (norm + 1e-6)) if self.max_grad_norm > 0 else 1.0
        self.steps += 1
        t = self.steps
        step_size, bc2 = dt(self.lr / (1.0 - self.betas[0] ** t)), dt(np.sqrt(1.0 - self.betas[1] ** t))
        g = grad * dt(scale)
        self.m = self.m + dt(1.0 - self.betas[0]) * (g - self.m)
        self.v = dt(self.betas[1]) * self.v + dt(1.0 - self.betas[1]) * (g * g)
        self.theta = (self.theta - step_size * (self.m / (np.sqrt(self.v) / bc2 + dt(self.eps_adam)))).astype(self.lay.arith)
        return norm

    def update(self, fit):
        """one update from fit [M R]; returns (member_fit, util, grad, stats)"""
        F, util, st = ranks(fit, self.M)
        grad = gradient(util, self.theta, self.sigma, self.wd, self.seed, self.gen, self.lay)
        st["grad_norm"] = self.adam(grad)
        self.gen += 1
        return F, util, grad, st


# ---- the learning setup of tests/test_es_host.py and tests/test_gpu_es.py ---------------------------------
LEARN = dict(obs_dim=6, hidden=(8,), act_dim=2, low=-0.5, high=1.5, sigma=0.1, lr=0.05, members=64, seed=20260117,
             target=(0.3, 1.1))


def learning_setup(dtype=np.float64, arith=np.float64):
    """(lay, theta0 [E], obs [M, obs_dim], target [act_dim]): fixed uniform observation rows, one per member; the fitness of a replica
    is -|a - a*|^2"""
    L = LEARN
    lay = Layout(L["obs_dim"], L["hidden"], L["act_dim"], dtype, arith)
    theta0 = lay.pack(random_weights(L["obs_dim"], L["hidden"], L["act_dim"], 5))
    obs = np.random.default_rng(6).uniform(-1.0, 1.0, (L["members"], L["obs_dim"])).astype(dtype).astype(arith)
    return lay, theta0, obs, np.asarray(L["target"], dtype=np.float64)


def learning_fitness(actions, target):
    """[B] float64: -|a - a*|^2"""
    return -((np.asarray(actions, dtype=np.float64) - target) ** 2).sum(axis=1)


def learning_ref(dtype=np.float64, arith=np.float64):
    L = LEARN
    lay, theta0, obs, target = learning_setup(dtype, arith)
    return Ref(lay, "tanh", 0, L["members"], theta0, L["seed"], L["sigma"], L["lr"], low=L["low"], high=L["high"]), obs, target

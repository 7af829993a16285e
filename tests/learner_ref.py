"""The reference of the on-device learner (include/beacon_learner.h): torch autograd in float64 on the CPU.

The two networks are torch.nn.Sequential built from the weights as the device holds them (cast to float64); the loss is the header's
formula written with torch ops, its gradient comes from backward(), the optimiser is torch.optim.Adam behind clip_grad_norm_.
tests/test_learner_host.py pins this file against a central finite difference, so that the formula and the code agree.

Ref(..., dtype=torch.float32) runs the same modules and the same loss in float32 on the CPU: what honest float32 arithmetic in
another summation order gives, the yardstick of the device's float32 error (tests/test_gpu_learner.py: rel)."""
import math

import torch
import torch.nn as nn

STATS = ("loss", "pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac", "weight", "grad_norm")


class Ref(object):
    def __init__(self, weights, hidden, activation, kind, dtype=torch.float64):
        """weights: {segment name: array-like} -- pi_w0, pi_b0, ... vf_w{L}, vf_b{L}, log_std (Gaussian); kind: 0 Gaussian, 1 categorical;
        dtype: the precision everything is held and computed in"""
        self.kind, self.hidden, self.activation, self.dtype = kind, tuple(hidden), activation, dtype
        cast = self._cast
        self.named = []                                   # (segment name, Parameter) in the layout's order

        def net(prefix):
            mods = []
            for l in range(len(hidden) + 1):
                W = cast(weights["%s_w%d" % (prefix, l)]).cpu()
                lin = nn.Linear(W.shape[1], W.shape[0]).to(dtype)
                with torch.no_grad():
                    lin.weight.copy_(W)
                    lin.bias.copy_(cast(weights["%s_b%d" % (prefix, l)]).cpu().reshape(-1))
                self.named += [("%s_w%d" % (prefix, l), lin.weight), ("%s_b%d" % (prefix, l), lin.bias)]
                mods.append(lin)
                if l < len(hidden):
                    mods.append(nn.Tanh() if activation == "tanh" else nn.ReLU())
            return nn.Sequential(*mods)

        self.pi, self.vf = net("pi"), net("vf")
        self.log_std = None
        if kind == 0:
            self.log_std = nn.Parameter(cast(weights["log_std"]).cpu().reshape(-1).clone())
            self.named.append(("log_std", self.log_std))

    def _cast(self, x):
        return torch.as_tensor(x).to(self.dtype)

    def parameters(self):
        return [p for _, p in self.named]

    def preactivations(self, obs):
        """every hidden layer's input to its activation, both networks: a list of [m, width] tensors"""
        out = []
        with torch.no_grad():
            for seq in (self.pi, self.vf):
                x = self._cast(obs)
                for mod in seq:
                    x = mod(x)
                    if isinstance(mod, nn.Linear):
                        out.append(x.clone())
                out.pop()                                 # the head has no activation
        return out

    @staticmethod
    def _run(seq, x, trace):
        """seq(x); with a trace list, every Linear's (input, output) is appended and the output keeps its gradient"""
        if trace is None:
            return seq(x)
        for mod in seq:
            y = mod(x)
            if isinstance(mod, nn.Linear):
                y.retain_grad()
                trace.append((x.detach(), y))
            x = y
        return x

    def terms(self, obs, act, logp_old, adv, ret, w, clip, vf_coef, ent_coef, trace=None):
        """the loss and everything on the way to it; the rows are the minibatch's (already gathered), w [m] their weights (or None)"""
        obs = self._cast(obs)
        logp_old, adv, ret = (self._cast(x).reshape(-1) for x in (logp_old, adv, ret))
        m = obs.shape[0]
        w = torch.ones(m, dtype=self.dtype) if w is None else self._cast(w).reshape(-1)
        head = self._run(self.pi, obs, trace)
        value = self._run(self.vf, obs, trace)[:, 0]
        z = None
        if self.kind == 0:
            a = self._cast(act).reshape(m, -1)
            z = (a - head) * torch.exp(-self.log_std)
            logp = (-0.5 * z * z - self.log_std - 0.5 * math.log(2.0 * math.pi)).sum(1)
            H = (self.log_std + 0.5 * math.log(2.0 * math.pi * math.e)).sum().expand(m)
        else:
            d = torch.log_softmax(head, dim=1)
            logp = d.gather(1, torch.as_tensor(act).long().reshape(m, 1))[:, 0]
            H = -(torch.exp(d) * d).sum(1)
        ratio = torch.exp(logp - logp_old)
        pg = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
        v = (value - ret) ** 2
        W = torch.clamp(w.sum(), min=1.0)
        # a row of weight 0 may hold NaN: it is no part of any sum
        on = w > 0
        wsum = lambda x: (w[on] * x[on]).sum() / W
        loss = wsum(pg + vf_coef * v - ent_coef * H)
        kl = (ratio - 1.0) - torch.log(ratio)
        cf = ((ratio - 1.0).abs() > clip).to(self.dtype)
        return dict(loss=loss, pg_loss=wsum(pg), vf_loss=wsum(v), entropy=wsum(H), approx_kl=wsum(kl), clip_frac=wsum(cf), weight=W,
                    ratio=ratio.detach()[on], logp=logp.detach(), value=value.detach(), z=None if z is None else z.detach()[on])

    def row_term_max(self, obs, act, logp_old, adv, ret, w=None, clip=0.2, vf_coef=0.5, ent_coef=0.0):
        """max |per-row term| of the weight and bias gradients: a gradient entry is (sum over the rows of its per-row terms) / W, the
        term of dW[o][k] at row r is delta[r][o] x[r][k] (delta: the gradient of W x loss at the layer's output, x: its input), so the
        largest is max_r max_o |delta| max(1, max_k |x|) over the layers of both networks.  (log_std's terms, w (g (z^2 - 1) - ent_coef)
        with |g| <= ratio |adv|, are bounded by the quantities the caller asserts on beside this one.)"""
        for p in self.parameters():
            p.grad = None
        trace = []
        t = self.terms(obs, act, logp_old, adv, ret, w, clip, vf_coef, ent_coef, trace=trace)
        (t["loss"] * t["weight"]).backward()
        worst = 0.0
        for x, y in trace:
            d = y.grad.abs().max(dim=1).values
            worst = max(worst, float((d * x.abs().max(dim=1).values.clamp(min=1.0)).max()))
        for p in self.parameters():
            p.grad = None
        return worst

    def grad(self, obs, act, logp_old, adv, ret, w=None, clip=0.2, vf_coef=0.5, ent_coef=0.0):
        """({segment name: gradient}, {statistic: float}, terms): p.grad holds the gradient afterwards"""
        for p in self.parameters():
            p.grad = None
        t = self.terms(obs, act, logp_old, adv, ret, w, clip, vf_coef, ent_coef)
        t["loss"].backward()
        grads = {name: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for name, p in self.named}
        stats = {k: float(t[k].detach()) for k in STATS[:7]}
        stats["grad_norm"] = float(torch.sqrt(sum((g * g).sum() for g in grads.values())))
        return grads, stats, t

    def adam(self, lr, betas, eps, start_step=0):
        """torch.optim.Adam over the parameters; start_step > 0: as if that many steps had been taken and left zero moments (the state
        a learner has whose step counter was set by hand)"""
        opt = torch.optim.Adam(self.parameters(), lr=lr, betas=betas, eps=eps)
        if start_step:
            for p in self.parameters():
                opt.state[p] = {"step": torch.tensor(float(start_step)), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        return opt

    def clip_and_step(self, opt, max_grad_norm):
        """clip_grad_norm_ (max_grad_norm > 0) and one optimiser step on the gradients of the last grad(); returns the norm before"""
        norm = float(torch.sqrt(sum((p.grad * p.grad).sum() for p in self.parameters())))
        if max_grad_norm > 0:
            nn.utils.clip_grad_norm_(self.parameters(), max_grad_norm)
        opt.step()
        return norm

    def moments(self, opt):
        """({name: exp_avg}, {name: exp_avg_sq}, step)"""
        m = {name: opt.state[p]["exp_avg"].clone() for name, p in self.named}
        v = {name: opt.state[p]["exp_avg_sq"].clone() for name, p in self.named}
        return m, v, int(opt.state[self.named[0][1]]["step"])

#!/usr/bin/env python3
"""Cost per step of the running normalisation of observations and rewards (VecEnv.set_normalize, csrc/normalize.hip) next to
the same normalisation written with torch ops, measured in the same process:
  (a) step_autoreset with the normaliser on: the step kernel, the bookkeeping launch, the masked reset and the two normalising
      launches;
  (b) step_autoreset followed by the same normalisation as in-place torch ops on the same tensors (TorchNormalize below: what the
      VecNormalize wrapper of the RL libraries does, with the statistics in float64);
  (s) step_autoreset alone.
Each path eager and as an n-step graph.  Episode counters are staggered over the whole episode, so resets happen at the rate of a
long training run.  The paths alternate a/b/s/a/b/s ... in one process; a window is `--steps` steps between two host clock reads,
the second behind a device synchronise; every window is reported, with the median and the spread (max - min) of each path.
One JSON line per case, also appended to profiles/normalize_bench.jsonl.
usage: python scripts/bench_normalize.py [--rounds 5] [--steps 200] [--only lorenz] [--out profiles/normalize_bench.jsonl]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beacon_amd import vec as V

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200, help="steps per timed window (2D cases: a tenth of it)")
ap.add_argument("--graph-steps", type=int, default=20, help="steps per captured graph")
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_normalize.py measures on a GPU; there is no CPU fallback"


def rayleigh():
    p = os.path.join(ROOT, "tests", "golden", "rayleigh_128x64_init.npz")
    init = np.load(p)["fields"] if os.path.exists(p) else None
    return V.VecRayleigh(512, dev, "f32", init, L=2.56, H=1.28)


CASES = [
    ("burgers B=1024 f32", lambda: V.VecBurgers(1024, dev, "f32"), 1),
    ("shkadov B=1024 f32", lambda: V.VecShkadov(1024, dev, "f32"), 1),
    ("lorenz B=2^20 f32", lambda: V.VecLorenz(1 << 20, dev, "f32"), 1),
    ("rayleigh 128x64 B=512 f32", rayleigh, 10),
]


def action(env):
    if env.action_is_int:
        return torch.ones((env.batch,), dtype=torch.int32, device=dev)
    shape = (env.batch,) if env.n_actions == 1 and not isinstance(env, V.VecRayleigh) else (env.batch, env.n_actions)
    return torch.full(shape, 0.25, dtype=env.tdtype, device=dev)


class TorchNormalize(object):
    """bcn_normalize (include/beacon_hip.h), kind step, with an episode buffer, as torch ops: nothing allocated per call that the
    caching allocator does not hand back, no host read (the number of counted replicas stays a device scalar)."""

    def __init__(self, env, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_rwd=10.0):
        B, n = env.batch, env.obs_dim
        self.gamma, self.eps, self.clip_obs, self.clip_rwd = gamma, eps, clip_obs, clip_rwd
        f64 = dict(dtype=torch.float64, device=dev)
        self.obs_mean, self.obs_var, self.obs_count = torch.zeros(n, **f64), torch.ones(n, **f64), torch.zeros((), **f64)
        self.ret_mean, self.ret_var, self.ret_count = torch.zeros((), **f64), torch.ones((), **f64), torch.zeros((), **f64)
        self.ret = torch.zeros(B, **f64)
        self.norm_obs, self.norm_rwd, self.norm_final_obs = torch.zeros_like(env.obs), torch.zeros_like(env.rwd), torch.zeros_like(env.obs)

    @staticmethod
    def merge(mean, var, count, x, w, n):
        """x [B, ...] float64, w the 0 / 1 weights of the counted rows (broadcast over x), n their number (a device scalar)"""
        safe = n.clamp(min=1.0)
        mb = (x * w).sum(0) / safe
        m2 = (((x - mb) ** 2) * w).sum(0)
        d, tot = mb - mean, (count + n).clamp(min=1.0)
        mean += d * n / tot
        var.copy_((var * count + m2 + d * d * count * n / tot) / tot * (n > 0) + var * (n == 0))
        count += n

    def update(self, env, ep):
        ok = (env.status & 3) == 0
        w = ok.double()
        n = w.sum()
        x = torch.where(ok[:, None], env.obs, 0).double()          # a blown-up row never enters a mean
        self.merge(self.obs_mean, self.obs_var, self.obs_count, x, w[:, None], n)
        inv = torch.rsqrt(self.obs_var + self.eps)
        self.norm_obs.copy_(((env.obs.double() - self.obs_mean) * inv).clamp_(-self.clip_obs, self.clip_obs))
        self.ret.mul_(self.gamma).add_(env.rwd)
        self.merge(self.ret_mean, self.ret_var, self.ret_count, torch.where(ok, self.ret, 0), w, n)
        self.norm_rwd.copy_((env.rwd.double() * torch.rsqrt(self.ret_var + self.eps)).clamp_(-self.clip_rwd, self.clip_rwd))
        self.ret.masked_fill_((env.done | env.trunc).bool(), 0)
        fin = ((ep.final_obs.double() - self.obs_mean) * inv).clamp_(-self.clip_obs, self.clip_obs)
        torch.where(ep.finished.bool()[:, None], fin.to(self.norm_final_obs.dtype), self.norm_final_obs, out=self.norm_final_obs)


def replaced(env, tn, a):
    ep = env.step_autoreset(a)[4]
    tn.update(env, ep)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def summary(r, key, us):
    r[key + "_us"] = [round(x, 3) for x in us]
    r[key + "_median_us"] = float(np.median(us))
    r[key + "_spread_us"] = float(max(us) - min(us))


NAMES = {"a": "normalize", "b": "torch", "s": "autoreset"}
for name, make, div in CASES:
    if args.only and args.only not in name:
        continue
    n, ng = max(args.steps // div, 10), args.graph_steps
    envs = {k: make() for k in ("a", "b", "s")}
    for env in envs.values():
        env.reset()
        env.set_stp(np.arange(env.batch) % env.n_act)
    envs["a"].set_normalize()
    a = action(envs["b"])
    tn = TorchNormalize(envs["b"])
    eager = {"a": lambda: envs["a"].step_autoreset(a), "b": lambda: replaced(envs["b"], tn, a), "s": lambda: envs["s"].step_autoreset(a)}
    r = {"case": name, "steps_per_window": n, "graph_steps": ng, "rounds": args.rounds}
    for fn in eager.values():                    # warm-up: code objects, the buffers, the allocator
        for _ in range(10):
            fn()
    us = {k: [] for k in eager}
    for _ in range(args.rounds):
        for k in sorted(eager):
            us[k].append(window(eager[k], n))
    for k in sorted(us):
        summary(r, NAMES[k] + "_eager", us[k])
    an = a.unsqueeze(0).expand(ng, *a.shape).contiguous()
    graphs = {k: envs[k].capture(an, None, n_steps=ng, keep_steps=False, autoreset=True).graph for k in ("a", "s")}
    gb = torch.cuda.CUDAGraph()
    env, ep = envs["b"], envs["b"].episodes
    if getattr(env, "gen", None) is not None:
        gb.register_generator_state(env.gen)     # (as StepGraph does for an env that draws its own noise)
    torch.cuda.synchronize()
    with torch.cuda.graph(gb):
        for _ in range(ng):
            env._masked(None, lambda m: env._enqueue_step(a, None, m, ep))      # what capture(autoreset=True) records per step
            tn.update(env, ep)
    graphs["b"] = gb
    for g in graphs.values():
        g.replay()
    us = {k: [] for k in graphs}
    reps = max(n // ng, 2)
    for _ in range(args.rounds):
        for k in sorted(graphs):
            us[k].append(window(graphs[k].replay, reps) / ng)
    for k in sorted(us):
        summary(r, NAMES[k] + "_graph", us[k])
    nz = envs["a"].normalizer
    r["obs_count"] = float(nz.obs_count[0])
    r["obs_count_torch"] = float(tn.obs_count)
    # the two normalisers saw the same env: their statistics agree to rounding
    r["obs_mean_max_abs_diff"] = float((nz.obs_mean - tn.obs_mean).abs().max())
    r["obs_var_max_rel_diff"] = float(((nz.obs_var - tn.obs_var).abs() / tn.obs_var.abs().clamp(min=1e-300)).max())
    for mode in ("eager", "graph"):
        d = r["normalize_%s_median_us" % mode] - r["torch_%s_median_us" % mode]
        r["normalize_minus_torch_%s_us" % mode] = d
        r["normalize_faster_by_more_than_spread_%s" % mode] = bool(-d > r["torch_%s_spread_us" % mode])
        r["normalize_minus_autoreset_%s_us" % mode] = r["normalize_%s_median_us" % mode] - r["autoreset_%s_median_us" % mode]
    line = json.dumps(r)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    for env in envs.values():
        env.close()
    del envs, graphs, gb, tn, nz
    torch.cuda.empty_cache()

#!/usr/bin/env python3
"""Cost per step of VecEnv.step_autoreset (csrc/episode.hip) next to the sequence it replaces, measured in the same process:
  (a) step_autoreset: the step kernel, one bookkeeping launch, the masked reset;
  (b) step(); final = obs.clone(); reset_done(); and the torch ops a trainer needs for the same statistics (trainer_stats below);
  (s) the plain step() alone, for comparison with a tree that has no step_autoreset (only (b) and (s) are timed there).
Each path eager and as an n-step graph.  Episode counters are staggered over the whole episode, so resets happen at the rate of a
long training run.  The paths alternate a/b/s/a/b/s ... in one process; a window is `--steps` steps between two host clock reads,
the second behind a device synchronise; every window is reported, with the median and the spread (max - min) of each path.
One JSON line per case, also appended to profiles/episode_bench.jsonl.
usage: python scripts/bench_episode.py [--rounds 5] [--steps 200] [--only lorenz] [--out profiles/episode_bench.jsonl]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_episode.py measures on a GPU; there is no CPU fallback"


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


class TrainerStats(object):
    """the statistics of EpisodeStats kept by in-place torch ops, as a trainer without step_autoreset does"""

    def __init__(self, env):
        B = env.batch
        self.ret = torch.zeros(B, dtype=env.tdtype, device=dev)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.last_ret, self.last_len = self.ret.clone(), self.len.clone()
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.sum_ret = torch.zeros(B, dtype=torch.float64, device=dev)
        self.sum_len = torch.zeros(B, dtype=torch.int64, device=dev)
        self.final = torch.zeros_like(env.obs)

    def update(self, rwd, done, trunc):
        fin = (done | trunc).bool()
        self.ret += rwd
        self.len += 1
        torch.where(fin, self.ret, self.last_ret, out=self.last_ret)
        torch.where(fin, self.len, self.last_len, out=self.last_len)
        self.count += fin
        self.sum_ret += torch.where(fin, self.ret, 0).double()
        self.sum_len += torch.where(fin, self.len, 0)
        self.ret.masked_fill_(fin, 0)
        self.len.masked_fill_(fin, 0)


def replaced(env, st, a, clone=True):
    env.step(a)
    if clone:
        st.final = env.obs.clone()
    else:
        st.final.copy_(env.obs)           # inside a graph: a fixed address
    st.update(env.rwd, env.done, env.trunc)
    env.reset_done()


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


for name, make, div in CASES:
    if args.only and args.only not in name:
        continue
    has = hasattr(V.VecEnv, "step_autoreset")
    n, ng = max(args.steps // div, 10), args.graph_steps
    envs = {k: make() for k in (("a", "b", "s") if has else ("b", "s"))}
    for env in envs.values():
        env.reset()
        env.set_stp(np.arange(env.batch) % env.n_act)
    a = action(envs["b"])
    st = TrainerStats(envs["b"])
    eager = {"b": lambda: replaced(envs["b"], st, a), "s": lambda: envs["s"].step(a)}
    if has:
        eager["a"] = lambda: envs["a"].step_autoreset(a)
    r = {"case": name, "steps_per_window": n, "graph_steps": ng, "rounds": args.rounds}
    for fn in eager.values():                    # warm-up: code objects, the episodes buffer, the allocator
        for _ in range(10):
            fn()
    us = {k: [] for k in eager}
    for _ in range(args.rounds):
        for k in sorted(eager):
            us[k].append(window(eager[k], n))
    for k in sorted(us):
        summary(r, {"a": "autoreset_eager", "b": "replaced_eager", "s": "step_eager"}[k], us[k])
    # graphs of ng steps each (the plain step: the env's own capture)
    an = a.unsqueeze(0).expand(ng, *a.shape).contiguous()
    graphs = {"s": envs["s"].capture(an, None, n_steps=ng, keep_steps=False).graph}
    if has:
        graphs["a"] = envs["a"].capture(an, None, n_steps=ng, keep_steps=False, autoreset=True).graph
    gb = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(gb):
        for _ in range(ng):
            replaced(envs["b"], st, a, clone=False)
    graphs["b"] = gb
    for g in graphs.values():
        g.replay()
    us = {k: [] for k in graphs}
    reps = max(n // ng, 2)
    for _ in range(args.rounds):
        for k in sorted(graphs):
            us[k].append(window(graphs[k].replay, reps) / ng)
    for k in sorted(us):
        summary(r, {"a": "autoreset_graph", "b": "replaced_graph", "s": "step_graph"}[k], us[k])
    if has:
        r["episodes_tracked"] = envs["a"].episodes.totals()["episodes"]
        r["episodes_trainer"] = int(st.count.sum())
        for mode in ("eager", "graph"):
            d = r["autoreset_%s_median_us" % mode] - r["replaced_%s_median_us" % mode]
            r["autoreset_minus_replaced_%s_us" % mode] = d
            r["autoreset_not_slower_%s" % mode] = bool(d <= r["replaced_%s_spread_us" % mode])
    line = json.dumps(r)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    for env in envs.values():
        env.close()
    del envs, graphs, gb, st
    torch.cuda.empty_cache()

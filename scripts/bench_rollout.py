#!/usr/bin/env python3
"""Cost of the on-device rollout storage (VecEnv.rollout, csrc/rollout.hip) and of compute_gae, next to the same work written with
torch ops, measured in the same process.
Recording, per step:
  (s) step_autoreset alone;
  (a) step_autoreset with a rollout attached: the same launches plus the recording launch and the one lane that advances the cursor;
  (b) step_autoreset followed by torch copy_ of the same data into preallocated [T, ...] tensors (obs, act, rwd, status, done, trunc)
      plus a masked copy of final_obs (torch.where on episodes.finished).
Each path eager and as a T-step graph.  Episode counters are staggered over the whole episode, so resets happen at the rate of a long
training run.  The paths alternate a/b/s/a/b/s ... in one process; a window is one rollout of T steps between two host clock reads,
the second behind a device synchronise; every window is reported, with the median and the spread (max - min) of each path.
GAE, per call: Rollout.compute_gae against the same recurrence as a T-iteration torch loop (float64 accumulators, as the kernel), at
T = 128 for B = 512, 1024 and 2^20, on synthetic flags (20 % ends, half of them truncations).
One JSON line per case, also appended to profiles/rollout_bench.jsonl.
usage: python scripts/bench_rollout.py [--rounds 5] [--T 128] [--only lorenz] [--out profiles/rollout_bench.jsonl]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beacon_amd import vec as V

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--T", type=int, default=128, help="steps per rollout (2D case: a quarter of it)")
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_rollout.py measures on a GPU; there is no CPU fallback"


def rayleigh():
    p = os.path.join(ROOT, "tests", "golden", "rayleigh_128x64_init.npz")
    init = np.load(p)["fields"] if os.path.exists(p) else None
    return V.VecRayleigh(512, dev, "f32", init, L=2.56, H=1.28)


CASES = [
    ("burgers B=1024 f32", lambda: V.VecBurgers(1024, dev, "f32"), 1),
    ("shkadov B=1024 f32", lambda: V.VecShkadov(1024, dev, "f32"), 1),
    ("lorenz B=2^20 f32", lambda: V.VecLorenz(1 << 20, dev, "f32"), 1),
    ("rayleigh 128x64 B=512 f32", rayleigh, 4),
]


def action(env):
    if env.action_is_int:
        return torch.ones((env.batch,), dtype=torch.int32, device=dev)
    shape = (env.batch,) if env.n_actions == 1 and not isinstance(env, V.VecRayleigh) else (env.batch, env.n_actions)
    return torch.full(shape, 0.25, dtype=env.tdtype, device=dev)


class TorchRollout(object):
    """what Rollout holds, as preallocated tensors filled by copy_ (slot k from a host counter)"""

    def __init__(self, env, T, a):
        z = lambda t, n=T: torch.zeros((n,) + tuple(t.shape), dtype=t.dtype, device=dev)
        self.obs, self.act, self.rwd, self.status = z(env.obs, T + 1), z(a), z(env.rwd), z(env.status)
        self.done, self.trunc, self.final_obs = z(env.done), z(env.trunc), z(env.obs)

    def store(self, env, ep, a, k):
        self.obs[k + 1].copy_(env.obs)
        self.act[k].copy_(a)
        self.rwd[k].copy_(env.rwd)
        self.status[k].copy_(env.status)
        self.done[k].copy_(env.done)
        self.trunc[k].copy_(env.trunc)
        torch.where(ep.finished.bool()[:, None], ep.final_obs, self.final_obs[k], out=self.final_obs[k])


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def summary(r, key, us):
    r[key + "_us"] = [round(x, 3) for x in us]
    r[key + "_median_us"] = float(np.median(us))
    r[key + "_spread_us"] = float(max(us) - min(us))


def verdict(r, mode):
    a, b, s = (r["%s_%s_median_us" % (k, mode)] for k in ("rollout", "torch", "autoreset"))
    spread = max(r["%s_%s_spread_us" % (k, mode)] for k in ("rollout", "torch", "autoreset"))
    r["rollout_minus_autoreset_%s_us" % mode] = a - s
    r["torch_minus_autoreset_%s_us" % mode] = b - s
    r["rollout_cheaper_than_torch_by_more_than_spread_%s" % mode] = bool((b - s) - (a - s) > spread)
    r["rollout_inside_spread_%s" % mode] = bool(abs(a - s) <= spread)


NAMES = {"a": "rollout", "b": "torch", "s": "autoreset"}
for name, make, div in CASES:
    if args.only and args.only not in name:
        continue
    T = max(args.T // div, 8)
    envs = {k: make() for k in ("a", "b", "s")}
    for env in envs.values():
        env.reset()
        env.set_stp(np.arange(env.batch) % env.n_act)
    ro = envs["a"].rollout(T)
    a = action(envs["b"])
    tr = TorchRollout(envs["b"], T, a)

    def eager_a():
        ro.begin()
        for _ in range(T):
            envs["a"].step_autoreset(a)

    def eager_b():
        env = envs["b"]
        tr.obs[0].copy_(env.obs)
        for k in range(T):
            tr.store(env, env.step_autoreset(a)[4], a, k)

    def eager_s():
        for _ in range(T):
            envs["s"].step_autoreset(a)

    eager = {"a": eager_a, "b": eager_b, "s": eager_s}
    r = {"case": name, "T": T, "rounds": args.rounds, "unit": "us per step"}
    for fn in eager.values():                    # warm-up: code objects, the buffers, the allocator
        fn()
    us = {k: [] for k in eager}
    for _ in range(args.rounds):
        for k in sorted(eager):
            us[k].append(window(eager[k]) / T)
    for k in sorted(us):
        summary(r, NAMES[k] + "_eager", us[k])
    r["steps_recorded_eager"] = ro.check()[0]
    an = a.unsqueeze(0).expand(T, *a.shape).contiguous()
    ro.begin()
    graphs = {k: envs[k].capture(an, None, n_steps=T, keep_steps=False, autoreset=True).graph for k in ("a", "s")}
    gb = torch.cuda.CUDAGraph()
    env, ep = envs["b"], envs["b"].episodes
    if getattr(env, "gen", None) is not None:
        gb.register_generator_state(env.gen)     # (as StepGraph does for an env that draws its own noise)
    torch.cuda.synchronize()
    with torch.cuda.graph(gb):
        tr.obs[0].copy_(env.obs)
        for k in range(T):
            env._masked(None, lambda m: env._enqueue_step(a, None, m, ep))      # what capture(autoreset=True) records per step
            tr.store(env, ep, a, k)
    graphs["b"] = gb

    def replay(k):
        if k == "a":
            ro.begin()                           # part of every rollout
        graphs[k].replay()

    for k in graphs:
        replay(k)
    us = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k in sorted(graphs):
            us[k].append(window(lambda: replay(k)) / T)
    for k in sorted(us):
        summary(r, NAMES[k] + "_graph", us[k])
    r["steps_recorded_graph"] = ro.check()[0]
    for mode in ("eager", "graph"):
        verdict(r, mode)
    line = json.dumps(r)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    for env in envs.values():
        env.close()
    del envs, graphs, gb, tr, ro
    torch.cuda.empty_cache()


# ---- GAE -------------------------------------------------------------------------------------------------------------------------
def torch_gae(rwd, values, last_value, final_values, done, trunc, valid, gamma, lam, adv, ret):
    """the recurrence of bcn_rollout_gae as a T-iteration loop of elementwise ops on [B] tensors, float64 accumulators"""
    nv, gae = last_value.double(), torch.zeros_like(last_value, dtype=torch.float64)
    for t in range(rwd.shape[0] - 1, -1, -1):
        fin, ok, v = (done[t] | trunc[t]).bool(), valid[t].bool(), values[t].double()
        boot = torch.where(trunc[t].bool(), final_values[t].double(), 0.0)
        delta = rwd[t].double() + gamma * torch.where(fin, boot, nv) - v
        g = delta + torch.where(fin, 0.0, gamma * lam * gae)
        adv[t].copy_(torch.where(ok, g, 0.0))
        ret[t].copy_(torch.where(ok, g + v, v))
        gae = torch.where(ok, g, gae)
        nv = torch.where(ok, v, nv)


for B in (512, 1024, 1 << 20):
    name = "gae T=%d B=%d f32" % (args.T, B)
    if args.only and args.only not in name:
        continue
    T = args.T
    env = V.VecLorenz(B, dev, "f32")
    ro = env.rollout(T, final_obs=False)
    g = torch.Generator(device=dev).manual_seed(B)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    ro.rwd.copy_(rnd(T, B))
    fin = torch.rand((T, B), generator=g, device=dev) < 0.2
    ro.done.copy_(fin)
    ro.trunc.copy_(fin & (torch.rand((T, B), generator=g, device=dev) < 0.5))
    ro.valid.copy_(torch.rand((T, B), generator=g, device=dev) >= 0.1)
    ro.cursor[0] = T
    values, final, last = rnd(T, B), rnd(T, B), rnd(B)
    adv, ret = torch.zeros_like(values), torch.zeros_like(values)
    paths = {"kernel": lambda: ro.compute_gae(values, last, final, 0.99, 0.95),
             "torch": lambda: torch_gae(ro.rwd, values, last, final, ro.done, ro.trunc, ro.valid, 0.99, 0.95, adv, ret)}
    r = {"case": name, "T": T, "rounds": args.rounds, "unit": "us per call"}
    for fn in paths.values():
        fn()
    r["max_abs_diff_adv"] = float((ro.adv - adv).abs().max())
    r["max_abs_diff_ret"] = float((ro.ret - ret).abs().max())
    us = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k in sorted(paths):
            us[k].append(window(paths[k]))
    for k in sorted(us):
        summary(r, "gae_" + k, us[k])
    r["torch_over_kernel"] = r["gae_torch_median_us"] / r["gae_kernel_median_us"]
    line = json.dumps(r)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    env.close()
    del env, ro
    torch.cuda.empty_cache()

"""Time of one Actor.act() against the same two networks evaluated by the framework with its own sampling.

Three shapes (hidden (64, 64), tanh, float32, a clipped Gaussian): burgers B = 1024, sloshing B = 1024, rayleigh B = 512 (obs 384,
act_dim 10).  No solver runs: the observation rows are random tensors of the env's obs_dim.  Each shape is timed four ways -- the
actor eagerly and inside a replayed graph, the framework path eagerly and graph-captured -- in rounds that alternate the four
(A/B/A/B), device events around `--iters` calls each.

The two lorenz shapes of the plan (B = 2^20, categorical 3, float32 and float64) are not in the table: their framework baseline
(log_softmax, torch.multinomial) ended the process with a device-side assertion of torch.multinomial at B = 2^20 before a number
was taken, for a reason that was not found, so that baseline is not part of this script.

    python scripts/actor_time.py --out profiles/actor_time.jsonl"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import Actor, spaces, vec  # noqa: E402


class Shape(object):
    """what Actor reads of an env, without the solver"""
    _norm_on = False

    def __init__(self, batch, obs_dim, kind, n, dtype):
        self.batch, self.obs_dim, self.tdtype = batch, obs_dim, dtype
        self.device = torch.device("cuda", torch.cuda.current_device())
        assert kind == "gaussian"
        self.action_is_int = False
        self.action_space = spaces.box(-1.0, 1.0, (n,))
        self.obs = torch.rand((batch, obs_dim), dtype=dtype, device=self.device) * 2 - 1


def bare(cls):
    c = getattr(vec, cls)
    return c._derive(c.__new__(c))._make_spaces()


def shapes():
    bur, slo = bare("VecBurgers"), bare("VecSloshing")
    return [("burgers", 1024, bur.observation_space.shape[0], "gaussian", bur.action_space.shape[0], torch.float32),
            ("sloshing", 1024, slo.observation_space.shape[0], "gaussian", slo.action_space.shape[0], torch.float32),
            ("rayleigh", 512, 384, "gaussian", 10, torch.float32)]


def mlp(dims, dtype, device):
    nn = torch.nn
    layers = []
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(nn.Linear(i, o))
        if k < len(dims) - 2:
            layers.append(nn.Tanh())
    return nn.Sequential(*layers).to(device=device, dtype=dtype)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "actor_time.py needs the GPU"
    hidden = (64, 64)
    for name, B, obs_dim, kind, n, dtype in shapes():
        env = Shape(B, obs_dim, kind, n, dtype)
        actor = Actor(env, hidden=hidden, seed=1)
        pi, vf = mlp([obs_dim, 64, 64, n], dtype, env.device), mlp([obs_dim, 64, 64, 1], dtype, env.device)
        log_std = torch.full((n,), -0.5, dtype=dtype, device=env.device)
        actor.load_modules(pi, vf, log_std)
        half_ln_2pi = 0.5 * float(np.log(2.0 * np.pi))
        out = {}

        def framework():
            with torch.no_grad():
                head, out["value"] = pi(env.obs), vf(env.obs)[:, 0]
                z = torch.randn_like(head)
                raw = head + torch.exp(log_std) * z
                out["actions"], out["logp"] = raw.clamp(-1.0, 1.0), (-0.5 * z * z - log_std - half_ln_2pi).sum(dim=1)

        iters = args.iters
        fns = {"actor_eager": actor.act, "framework_eager": framework}
        for fn in fns.values():                       # warm-up: code objects, the allocator, the GEMM choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for key, fn in (("actor_graph", actor.act), ("framework_graph", framework)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            g.replay()
            fns[key] = g.replay
        torch.cuda.synchronize()
        us = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k in sorted(fns):                     # A / B / A / B: the four alternate inside every round
                us[k].append(window(fns[k], iters))
        r = {"shape": name, "batch": B, "obs_dim": obs_dim, "kind": kind, "act_dim": n, "dtype": "f64" if dtype == torch.float64 else "f32",
             "hidden": hidden, "rounds": args.rounds, "iters": iters, "unit": "us per act"}
        for k in sorted(us):
            r[k] = round(float(np.median(us[k])), 2)
            r[k + "_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
        r["actor_wins_eager"] = r["actor_eager"] < r["framework_eager"]
        r["actor_wins_graph"] = r["actor_graph"] < r["framework_graph"]
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del actor, pi, vf, fns, env
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Time of one Learner.grad() + Learner.step() against the same PPO minibatch update done by the framework: eager autograd over two
torch.nn.Sequential, clip_grad_norm_ and torch.optim.Adam on the same GPU -- what a user of Actor had before.

Two shapes (m = 16 384 rows, hidden (64, 64), tanh, float32, Gaussian): obs_dim 5, act_dim 1 -- one VecBurgers minibatch -- and obs_dim
384, act_dim 10.  No solver runs: the rows are random tensors.  Each shape is timed three ways -- the learner eagerly, the learner
inside a replayed graph, the framework path eagerly -- in rounds that alternate them (A/B/A/B), device events around `--iters` updates
each.  The launch counts are the device kernels one update enqueues, counted by torch.profiler in a pass of its own (null when the
profiler gives no device events).

    python scripts/learner_bench.py --out profiles/learner_bench.jsonl"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import Actor, Learner  # noqa: E402
from actor_time import Shape, mlp, window  # noqa: E402

SHAPES = [("burgers", 16384, 5, 1), ("rayleigh", 16384, 384, 10)]
HYPER = dict(lr=3e-4, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-8)


def kernels_per_call(fn):
    """device kernels one call enqueues, by torch.profiler; None if it reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "learner_bench.py needs the GPU"
    hidden, dtype = (64, 64), torch.float32
    for name, m, obs_dim, n in SHAPES:
        env = Shape(m, obs_dim, "gaussian", n, dtype)
        dev = env.device
        actor = Actor(env, hidden=hidden, seed=1)
        pi, vf = mlp([obs_dim, 64, 64, n], dtype, dev), mlp([obs_dim, 64, 64, 1], dtype, dev)
        log_std = torch.nn.Parameter(torch.full((n,), -0.5, dtype=dtype, device=dev))
        actor.load_modules(pi, vf, log_std.detach())
        learner = Learner(actor, **HYPER)
        g = torch.Generator(device=dev).manual_seed(3)
        obs = env.obs
        act = torch.randn((m, n), dtype=dtype, device=dev, generator=g) * 0.5
        adv, ret = torch.randn((m,), dtype=dtype, device=dev, generator=g), torch.randn((m,), dtype=dtype, device=dev, generator=g)
        with torch.no_grad():
            z = (act - pi(obs)) * torch.exp(-log_std)
            logp_old = (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi)).sum(1) + (torch.rand((m,), dtype=dtype, device=dev, generator=g) - 0.5)
        params = list(pi.parameters()) + list(vf.parameters()) + [log_std]
        opt = torch.optim.Adam(params, lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"])
        clip, half_ln_2pi = HYPER["clip_range"], 0.5 * math.log(2 * math.pi)

        def library():
            learner.grad(obs, act, logp_old, adv, ret)
            learner.step()

        def framework():
            head, value = pi(obs), vf(obs)[:, 0]
            z = (act - head) * torch.exp(-log_std)
            logp = (-0.5 * z * z - log_std - half_ln_2pi).sum(1)
            ratio = torch.exp(logp - logp_old)
            pg = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
            vl = ((value - ret) ** 2).mean()
            ent = (log_std + 0.5 + half_ln_2pi).sum()
            loss = pg + HYPER["vf_coef"] * vl - HYPER["ent_coef"] * ent
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, HYPER["max_grad_norm"])
            opt.step()

        fns = {"learner_eager": library, "framework_eager": framework}
        for fn in fns.values():                       # warm-up: code objects, the allocator, the GEMM choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        launches = {k: kernels_per_call(fn) for k, fn in fns.items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            library()
        graph.replay()
        fns["learner_graph"] = graph.replay
        torch.cuda.synchronize()
        us = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k in sorted(fns):                     # A / B / A / B: the three alternate inside every round
                us[k].append(window(fns[k], args.iters))
        r = {"shape": name, "m": m, "obs_dim": obs_dim, "act_dim": n, "dtype": "f32", "hidden": hidden, "rounds": args.rounds, "iters": args.iters,
             "unit": "us per grad + step", "learner_launches": 5, "profiled_kernels": launches}
        for k in sorted(us):
            r[k] = round(float(np.median(us[k])), 2)
            r[k + "_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
        r["learner_not_slower_eager"] = r["learner_eager"] <= r["framework_eager"]
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del learner, actor, pi, vf, opt, fns, env, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

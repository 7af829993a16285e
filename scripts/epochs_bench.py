"""Time of one whole PPO update three ways on the same GPU at the same commit: plan.run() -- the library's own shuffle
and standardisation around grad() + step() --, the replay of plan.capture()'s graph, and learner.update() -- torch.randperm and torch
arithmetic around the same grad() + step().

The workload is the burgers-sized case of scripts/learner_bench.py as a real rollout: VecBurgers, 1024 replicas x 16 steps = 16 384
rows, hidden (64, 64), tanh, float32, 10 epochs x 4 minibatches.  The method is learner_bench.py's: rounds that alternate the three
(A/B/C/A/B/C), device events around `--iters` updates each, the median over `--rounds` rounds.  lr = 0, so that every window updates
the same policy on the same rollout (Adam's arithmetic does not depend on the rate).  The launch counts are the device kernels one
update enqueues, counted by torch.profiler in a pass of its own (null when the profiler gives no device events).

    python scripts/epochs_bench.py --out profiles/epochs_bench.jsonl"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import beacon_amd  # noqa: E402
from beacon_amd import Actor, Learner  # noqa: E402
from actor_time import mlp, window  # noqa: E402
from learner_bench import kernels_per_call  # noqa: E402

HYPER = dict(lr=0.0, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "epochs_bench.py needs the GPU"
    B, T, hidden, epochs, nmb, dtype = 1024, 16, (64, 64), 10, 4, torch.float32
    env = beacon_amd.VecBurgers(B, dtype="f32", seed=5)
    actor = Actor(env, hidden=hidden, seed=1)
    n = actor.act_dim
    pi, vf = mlp([env.obs_dim, 64, 64, n], dtype, actor.device), mlp([env.obs_dim, 64, 64, 1], dtype, actor.device)
    actor.load_modules(pi, vf, torch.full((n,), -0.5, dtype=dtype))
    ro = env.rollout(T)
    actor.attach(ro)
    env.reset()
    ro.begin()
    for _ in range(T):
        env.step_autoreset(actor.act())
    adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs), actor.values(ro.final_obs.view(-1, env.obs_dim)).view(T, B))
    learner = Learner(actor, **HYPER)
    plan = learner.plan(ro, epochs=epochs, minibatches=nmb, seed=7)
    fns = {"plan_run": lambda: plan.run(adv, ret), "update": lambda: learner.update(ro, adv, ret, epochs=epochs, minibatches=nmb)}
    for fn in fns.values():                           # warm-up: code objects, the allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    launches = {k: kernels_per_call(fn) for k, fn in fns.items()}
    graph = plan.capture(adv, ret)
    graph.replay()
    fns["plan_graph"] = graph.replay
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k in sorted(fns):                         # the three alternate inside every round
            us[k].append(window(fns[k], args.iters))
    assert ro.check() == (T, False)
    r = {"shape": "burgers", "rows": T * B, "replicas": B, "steps": T, "obs_dim": env.obs_dim, "act_dim": n, "dtype": "f32", "hidden": hidden,
         "epochs": epochs, "minibatches": nmb, "rounds": args.rounds, "iters": args.iters, "unit": "us per update",
         "plan_launches_expected": 3 + epochs * (2 + nmb * 5), "profiled_kernels": launches}
    for k in sorted(us):
        r[k] = round(float(np.median(us[k])), 1)
        r[k + "_min_max"] = [round(min(us[k]), 1), round(max(us[k]), 1)]
    r["plan_run_not_slower"] = r["plan_run"] <= r["update"]
    r["plan_graph_not_slower"] = r["plan_graph"] <= r["update"]
    line = json.dumps(r)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()

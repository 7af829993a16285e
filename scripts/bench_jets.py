#!/usr/bin/env python3
"""Cost per step of the per-jet reward launch of shkadov (VecShkadov.set_jet_rewards, csrc/shkadov_jets.hip) at the shkadov
benchmark configuration (B = 1024, 10 jets, nx = 4096, float32), measured in one process:
  (off) step() with the feature off -- what a tree without the feature runs (there only this path is timed: run the script in
        both trees, alternating, to compare "off" with the parent's step());
  (on)  step() with set_jet_rewards(True): the step kernel and the per-jet launch with statistics;
  (ns)  the same with stats=False.
Each path eager and as an n-step graph, every env on its own copy of the same developed film and the same actions.  The paths
alternate off/on/ns/off/on/ns ... ; a window is `--steps` steps between two host clock reads, the second behind a device
synchronise; every window is reported, with the median and the spread (max - min) of each path.
One JSON line, also appended to --out.
usage: python scripts/bench_jets.py [--rounds 5] [--steps 200] [--graph-steps 20] [--warm 200] [--out profiles/jets_bench.jsonl]"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beacon_amd import vec as V

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
ap.add_argument("--graph-steps", type=int, default=20, help="steps per captured graph")
ap.add_argument("--warm", type=int, default=200, help="uncontrolled steps that develop the film before anything is timed")
ap.add_argument("--label", default="", help="recorded in the line (which tree this is)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jets_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_jets.py measures on a GPU; there is no CPU fallback"

B = 1024
has = hasattr(V.VecShkadov, "set_jet_rewards")
paths = ("off", "on", "ns") if has else ("off",)


def make(path):
    env = V.VecShkadov(B, dev, "f32", None, L0=699.2, n_jets=10)          # scripts/bench_envs.py: BASELINE configs[2]
    assert env.nx == 4096
    env.reset()
    env.warmup(args.warm, torch.zeros((B, 10), dtype=torch.float32, device=dev))
    if path != "off":
        env.set_jet_rewards(True, stats=path == "on")
    return env


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


envs = {p: make(p) for p in paths}
rng = np.random.default_rng(7)
a = torch.as_tensor(rng.uniform(-1, 1, (B, 10)), dtype=torch.float32, device=dev)
n, ng = args.steps, args.graph_steps
eager = {p: (lambda e=envs[p]: e.step(a)) for p in paths}
r = {"case": "shkadov B=1024 10 jets nx=4096 f32", "label": args.label, "has_jet_rewards": has, "steps_per_window": n,
     "graph_steps": ng, "rounds": args.rounds, "kernel": None}
for fn in eager.values():                        # warm-up: code objects, the allocator
    for _ in range(10):
        fn()
us = {p: [] for p in paths}
for _ in range(args.rounds):
    for p in paths:
        us[p].append(window(eager[p], n))
for p in paths:
    summary(r, "step_%s_eager" % p, us[p])
r["kernel"] = envs["off"].kernel_name
an = a.unsqueeze(0).expand(ng, *a.shape).contiguous()
graphs = {p: envs[p].capture(an, None, n_steps=ng, keep_steps=False).graph for p in paths}
for g in graphs.values():
    g.replay()
us = {p: [] for p in paths}
reps = max(n // ng, 2)
for _ in range(args.rounds):
    for p in paths:
        us[p].append(window(graphs[p].replay, reps) / ng)
for p in paths:
    summary(r, "step_%s_graph" % p, us[p])
if has:
    for mode in ("eager", "graph"):
        for p in ("on", "ns"):
            r["%s_minus_off_%s_us" % (p, mode)] = r["step_%s_%s_median_us" % (p, mode)] - r["step_off_%s_median_us" % mode]
    assert bool(torch.isfinite(envs["on"].rwd_jets).all())
    # the rows sum to the step's own reward (float32: (n_jets l_rwd + 3) 2^-24 relative)
    e = envs["on"]
    err = (e.rwd_jets.double().sum(1) - e.rwd.double()).abs() / e.rwd.double().abs()
    r["sum_over_jets_vs_rwd_max_rel"] = float(err.max())
line = json.dumps(r)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as fh:
    fh.write(line + "\n")
for env in envs.values():
    env.close()

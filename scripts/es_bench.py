"""Time of the evolution-strategies launches on the device against the same steps written in eager torch on the same GPU.

Two units of work, M = 512 members, R = 1, obs_dim 40, act_dim 10, hidden (64, 64), tanh, float32; no solver runs:
  act             the actions of the 512 replicas, each under its own member's network.  Library: ONE launch (agent.act()).  Framework:
                  three torch.baddbmm over per-member weight tensors [M, out, in] and the activations between them.
  begin + update  a generation's perturbation and its update from given fitness values.  Library: 1 + 7 launches.  Framework:
                  torch.randn perturbations [M / 2, E] kept for the update, argsort ranks, one matrix-vector product for the gradient
                  and torch.optim.Adam.
The arms alternate inside every round (A / B / A / B), device events around `--iters` units each; the medians over the rounds are
printed and appended to --out.  `act` is also given against the time in which pop, M E sizeof(real) bytes, streams from HBM once at
the rate a float4 copy reaches on this device (6.29 TB/s), and for the forced group sizes 1, 2, 4.

    python scripts/es_bench.py --out profiles/es_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import ES  # noqa: E402
from actor_time import Shape, mlp, window  # noqa: E402

MEMBERS, OBS_DIM, ACT_DIM, HIDDEN = 512, 40, 10, (64, 64)
HYPER = dict(sigma=0.05, lr=0.01)
HBM_COPY_RATE = 6.29e12           # bytes per second, a float4 copy on this device


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "es_bench.py needs the GPU"
    dtype = torch.float32
    env = Shape(MEMBERS, OBS_DIM, "gaussian", ACT_DIM, dtype)
    dev = env.device
    pi = mlp([OBS_DIM, 64, 64, ACT_DIM], dtype, dev)
    agents = {}
    for group in (0, 1, 2, 4):
        a = ES(env, hidden=HIDDEN, seed=1, group=group, **HYPER)
        a.load_modules(pi).begin()
        agents[group] = a
    agent = agents[0]
    M, E = agent.members, agent.n_elems
    fit = torch.randn(M, dtype=torch.float64, device=dev)

    def library_generation():
        agent.begin()
        agent.fit.copy_(fit)
        agent.update()

    # the framework path: per-member weight tensors, torch.randn noise, argsort ranks, torch.optim.Adam
    dims = [OBS_DIM, 64, 64, ACT_DIM]
    theta = torch.nn.Parameter(torch.cat([p.detach().reshape(-1) for p in pi.parameters()]))
    n = theta.numel()
    opt = torch.optim.Adam([theta], lr=HYPER["lr"])
    state = {"pop": theta.detach().repeat(M, 1)}

    def split(pop):
        out, at = [], 0
        for i, o in zip(dims[:-1], dims[1:]):
            W = pop[:, at:at + o * i].view(M, o, i)
            at += o * i
            b = pop[:, at:at + o].view(M, o, 1)
            at += o
            out.append((W, b))
        return out

    def framework_act():
        x = env.obs.unsqueeze(2)
        layers = split(state["pop"])
        for l, (W, b) in enumerate(layers):
            x = torch.baddbmm(b, W, x)
            if l < len(layers) - 1:
                x = torch.tanh(x)
        return torch.tanh(x.squeeze(2))

    def framework_generation():
        with torch.no_grad():
            eps = torch.randn((M // 2, n), dtype=dtype, device=dev)
            pop = torch.empty((M, n), dtype=dtype, device=dev)
            pop[0::2] = theta + HYPER["sigma"] * eps
            pop[1::2] = theta - HYPER["sigma"] * eps
            state["pop"] = pop
            rank = torch.argsort(torch.argsort(fit)).to(torch.float64)
            u = rank / (M - 1) - 0.5
            g = ((u[0::2] - u[1::2]).to(dtype) @ eps) / (M * HYPER["sigma"])
            theta.grad = -g
        opt.step()

    fns = {"act_library": agent.act, "act_framework": framework_act, "generation_library": library_generation, "generation_framework": framework_generation}
    for g_, a in agents.items():
        if g_:
            fns["act_library_group%d" % g_] = a.act
    for fn in fns.values():                       # warm-up: code objects, the allocator, the GEMM choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k in sorted(fns):                     # the arms alternate inside every round
            us[k].append(window(fns[k], args.iters))
    pop_bytes = M * E * 4
    r = {"members": M, "replicas": 1, "obs_dim": OBS_DIM, "act_dim": ACT_DIM, "hidden": HIDDEN, "dtype": "f32", "rounds": args.rounds, "iters": args.iters,
         "unit": "us per call", "E": E, "pop_bytes": pop_bytes, "group_chosen": agent.group, "lds_bytes": agent.lds_bytes,
         "generation_library_launches": 1 + 7 + 1, "pop_stream_us": round(pop_bytes / HBM_COPY_RATE * 1e6, 2), "pop_stream_rate_bytes_per_s": HBM_COPY_RATE,
         "pop_stream_rate_source": "quoted, not measured by this script: the float4-copy rate of BASELINE.md for this device"}
    for k in sorted(us):
        r[k] = round(float(np.median(us[k])), 2)
        r[k + "_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    r["act_library_over_pop_stream"] = round(r["act_library"] / r["pop_stream_us"], 2)
    line = json.dumps(r)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

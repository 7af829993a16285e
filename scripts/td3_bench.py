"""Time of a TD3 update on the device against the same update written in eager torch on the same GPU.

One unit of work is TWO minibatches at policy_delay 2: two critic steps (sample, target action with smoothing, y, both critics'
loss and gradient, Adam) and one policy step (the gradient through Q_1, Adam) with its Polyak step.  Hidden (64, 64), tanh, obs_dim
40, act_dim 10, float32, m = 256 and m = 4096 rows sampled from a memory of 65 536 random transitions; no solver runs.  The library
is timed as ONE captured graph (agent.plan(mem, 2, m).capture()) and eagerly; the framework path is torch.randint for the indices,
index_select for the rows, autograd over three torch.nn.Sequential, two torch.optim.Adam and torch._foreach ops for Polyak.  The arms
alternate inside every round (A / B / A / B), device events around `--iters` units each; the medians over the rounds are printed
and appended to --out.

    python scripts/td3_bench.py --out profiles/td3_bench.txt"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import TD3  # noqa: E402
from actor_time import Shape, mlp, window  # noqa: E402

OBS_DIM, ACT_DIM, HIDDEN, CAPACITY = 40, 10, (64, 64), 65536
HYPER = dict(lr=1e-3, gamma=0.99, tau=0.005, policy_delay=2, target_noise=0.2, noise_clip=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "td3_bench.py needs the GPU"
    dtype = torch.float32
    for m in (256, 4096):
        env = Shape(4, OBS_DIM, "gaussian", ACT_DIM, dtype)
        dev = env.device
        agent = TD3(env, hidden=HIDDEN, seed=1, **HYPER)
        D = OBS_DIM + ACT_DIM
        mu, q1, q2 = (mlp([i, 64, 64, o], dtype, dev) for i, o in ((OBS_DIM, ACT_DIM), (D, 1), (D, 1)))
        agent.load_modules(mu, q1, q2)
        mem = agent.replay(CAPACITY)
        g = torch.Generator(device=dev).manual_seed(3)
        mem.obs.copy_(torch.randn(mem.obs.shape, dtype=dtype, device=dev, generator=g))
        mem.next_obs.copy_(torch.randn(mem.obs.shape, dtype=dtype, device=dev, generator=g))
        mem.act.copy_(torch.rand(mem.act.shape, dtype=dtype, device=dev, generator=g) * 2 - 1)
        mem.rwd.copy_(torch.randn(mem.rwd.shape, dtype=dtype, device=dev, generator=g))
        mem.boot.fill_(1)
        mem.live.fill_(1)
        mem.head.copy_(torch.tensor([0, CAPACITY, CAPACITY, 0], dtype=torch.int32))
        plan = agent.plan(mem, 2, m)

        # the framework path: the same update on the same memory's tensors
        import copy
        tmu, tq1, tq2 = (copy.deepcopy(x) for x in (mu, q1, q2))
        nets, tnets = [mu, q1, q2], [tmu, tq1, tq2]
        qparams = list(q1.parameters()) + list(q2.parameters())
        opt_q = torch.optim.Adam(qparams, lr=HYPER["lr"])
        opt_mu = torch.optim.Adam(mu.parameters(), lr=HYPER["lr"])
        src = [p for n in nets for p in n.parameters()]
        dst = [p for n in tnets for p in n.parameters()]

        def framework():
            for k in range(2):
                idx = torch.randint(0, CAPACITY, (m,), device=dev)
                s, a, r, s2 = mem.obs.index_select(0, idx), mem.act.index_select(0, idx), mem.rwd.index_select(0, idx), mem.next_obs.index_select(0, idx)
                boot, w = mem.boot.index_select(0, idx).to(dtype), mem.live.index_select(0, idx).to(dtype)
                W = w.sum().clamp_(min=1.0)
                with torch.no_grad():
                    eps = (torch.randn((m, ACT_DIM), dtype=dtype, device=dev) * HYPER["target_noise"]).clamp_(-HYPER["noise_clip"], HYPER["noise_clip"])
                    a2 = (torch.tanh(tmu(s2)) + eps).clamp_(-1.0, 1.0)
                    x2 = torch.cat([s2, a2], 1)
                    y = r + HYPER["gamma"] * boot * torch.minimum(tq1(x2)[:, 0], tq2(x2)[:, 0])
                x = torch.cat([s, a], 1)
                loss = ((w * (q1(x)[:, 0] - y) ** 2).sum() + (w * (q2(x)[:, 0] - y) ** 2).sum()) / W
                opt_q.zero_grad(set_to_none=True)
                loss.backward()
                opt_q.step()
                if k == 1:
                    pl = -(w * q1(torch.cat([s, torch.tanh(mu(s))], 1))[:, 0]).sum() / W
                    opt_mu.zero_grad(set_to_none=True)
                    pl.backward()
                    opt_mu.step()
                    with torch.no_grad():
                        torch._foreach_lerp_(dst, src, HYPER["tau"])

        fns = {"library_eager": plan.run, "framework_eager": framework}
        for fn in fns.values():                       # warm-up: code objects, the allocator, the GEMM choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        graph = plan.capture()
        graph.replay()
        fns["library_graph"] = graph.replay
        torch.cuda.synchronize()
        us = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k in sorted(fns):                     # A / B / A / B: the arms alternate inside every round
                us[k].append(window(fns[k], args.iters))
        r = {"m": m, "obs_dim": OBS_DIM, "act_dim": ACT_DIM, "hidden": HIDDEN, "dtype": "f32", "rounds": args.rounds, "iters": args.iters,
             "unit": "us per 2 critic steps + 1 policy step + Polyak", "library_launches": 2 * 8 + 7}
        for k in sorted(us):
            r[k] = round(float(np.median(us[k])), 2)
            r[k + "_min_max"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del agent, mem, plan, graph, fns, env
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

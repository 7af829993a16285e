"""Time of a DQN update on the device against the same update written in eager torch on the same GPU.

One unit of work is ONE minibatch of 8 launches with double Q-learning: sample, the online argmax on s', y from the target network,
the Huber loss and its gradient, Adam, and the Polyak step.  Hidden (64, 64), tanh, mixing's obs_dim 192 and n = 4 actions, float32,
m = 256 and m = 4096 rows sampled from a memory of 65 536 random transitions; no solver runs.  The library is timed as ONE captured
graph (agent.plan(mem, 1, m).capture()) and eagerly; the framework path is torch.randint for the indices, index_select for the rows,
autograd over one torch.nn.Sequential plus a frozen copy, torch.optim.Adam and torch._foreach_lerp_ for Polyak.  The arms alternate
inside every round (A / B / A / B), device events around `--iters` units each; the medians over the rounds are printed and appended
to --out.

    python scripts/dqn_bench.py --out profiles/dqn_bench.txt"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import DQN  # noqa: E402
from actor_time import mlp, window  # noqa: E402

OBS_DIM, N_ACTIONS, HIDDEN, CAPACITY = 192, 4, (64, 64), 65536
HYPER = dict(lr=1e-3, gamma=0.99, tau=0.005, huber=1.0)


class Shape(object):
    """what DQN reads of an env, without the solver"""
    _norm_on = False
    action_is_int = True

    def __init__(self, batch, obs_dim, n, dtype):
        self.batch, self.obs_dim, self.tdtype = batch, obs_dim, dtype
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.action_space = types.SimpleNamespace(n=n)
        self.obs = torch.rand((batch, obs_dim), dtype=dtype, device=self.device) * 2 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dqn_bench.py needs the GPU"
    dtype = torch.float32
    for m in (256, 4096):
        env = Shape(4, OBS_DIM, N_ACTIONS, dtype)
        dev = env.device
        agent = DQN(env, hidden=HIDDEN, double=True, dueling=False, seed=1, **HYPER)
        q = mlp([OBS_DIM, 64, 64, N_ACTIONS], dtype, dev)
        agent.load_modules(q)
        mem = agent.replay(CAPACITY)
        g = torch.Generator(device=dev).manual_seed(3)
        mem.obs.copy_(torch.randn(mem.obs.shape, dtype=dtype, device=dev, generator=g))
        mem.next_obs.copy_(torch.randn(mem.obs.shape, dtype=dtype, device=dev, generator=g))
        mem.act.copy_(torch.randint(0, N_ACTIONS, mem.act.shape, device=dev, generator=g).to(dtype))
        mem.rwd.copy_(torch.randn(mem.rwd.shape, dtype=dtype, device=dev, generator=g))
        mem.boot.fill_(1)
        mem.live.fill_(1)
        mem.head.copy_(torch.tensor([0, CAPACITY, CAPACITY, 0], dtype=torch.int32))
        plan = agent.plan(mem, 1, m)

        # the framework path: the same update on the same memory's tensors
        tq = copy.deepcopy(q).requires_grad_(False)
        opt = torch.optim.Adam(q.parameters(), lr=HYPER["lr"])
        src, dst = list(q.parameters()), list(tq.parameters())
        huber = torch.nn.HuberLoss(reduction="none", delta=HYPER["huber"])

        def framework():
            idx = torch.randint(0, CAPACITY, (m,), device=dev)
            s, a, r, s2 = mem.obs.index_select(0, idx), mem.act.index_select(0, idx), mem.rwd.index_select(0, idx), mem.next_obs.index_select(0, idx)
            boot, w = mem.boot.index_select(0, idx).to(dtype), mem.live.index_select(0, idx).to(dtype)
            W = w.sum().clamp_(min=1.0)
            with torch.no_grad():
                jstar = q(s2).argmax(dim=1, keepdim=True)
                y = r + HYPER["gamma"] * boot * tq(s2).gather(1, jstar)[:, 0]
            qa = q(s).gather(1, a.to(torch.int64))[:, 0]
            loss = (w * huber(qa, y)).sum() / W
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
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
        r = {"m": m, "obs_dim": OBS_DIM, "n_actions": N_ACTIONS, "hidden": HIDDEN, "dtype": "f32", "double": True, "rounds": args.rounds,
             "iters": args.iters, "unit": "us per minibatch (sample, gradient, Adam, Polyak)", "library_launches": 8}
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

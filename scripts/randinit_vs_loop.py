"""Measurements for shkadov's random-start reset, in bench.py's shkadov setting (N = 4096, 10 jets, B = 1024,
float32, developed film):
  fused  the fused launch (set_random_init + reset_random_device) against the host loop (reset_random), both with the same explicit
         counts, one seeded draw on {0 .. 400}: both times, the numbers of launches, one action step for scale
  step   ms per action step of the step kernel, three runs of 50 steps (what bench.py --full reports as shkadov-v0 N=4096)
usage: python scripts/randinit_vs_loop.py {fused|step} TAG [OUT.jsonl]   -- prints one JSON line (and appends it to OUT.jsonl)"""
import json
import os
import sys
import time

import numpy as np
import torch

mode, tag = sys.argv[1], sys.argv[2]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beacon_amd import vec as V  # noqa: E402

dev = "cuda:0"
B = 1024
rng = np.random.default_rng(0)
env = V.VecShkadov(B, dev, "f32", None, L0=699.2, n_jets=10)
env.reset()
env.warmup(env.n_warmup_ref, torch.zeros((B, 10), dtype=env.tdtype, device=dev))
out = {"tag": tag, "mode": mode, "nx": env.nx, "kernel_shape": list(env.kernel_shape)}


def sync():
    torch.cuda.synchronize()


if mode == "step":
    a10 = torch.as_tensor(rng.uniform(-1, 1, (64, B, 10)), dtype=env.tdtype, device=dev)
    runs = []
    for r in range(3):
        for k in range(5):
            env.step(a10[k])
        sync()
        t0 = time.perf_counter()
        for k in range(50):
            env.step(a10[k % 64])
        sync()
        runs.append((time.perf_counter() - t0) / 50 * 1e3)
    out["ms_per_step"] = runs
else:
    # the developed film of replica 0 as the film every reset reloads
    st = env.get_state()[0, :2].double().cpu().numpy()
    env.close()
    env = V.VecShkadov(B, dev, "f32", st, L0=699.2, n_jets=10)
    counts = torch.as_tensor(np.random.default_rng(1).integers(0, 401, B), dtype=torch.int32, device=dev)
    out["counts_sum"] = int(counts.sum()); out["counts_max"] = int(counts.max())
    loop, fused = [], []
    for r in range(2):
        sync(); t0 = time.perf_counter()
        env.reset_random(400, counts)
        sync(); loop.append((time.perf_counter() - t0) * 1e3)
    s_loop = env.get_state().clone()
    env.set_random_init(400)
    for r in range(2):
        sync(); t0 = time.perf_counter()
        env.reset_random_device(counts)
        sync(); fused.append((time.perf_counter() - t0) * 1e3)
    s_fused = env.get_state()
    out["loop_ms"] = loop; out["fused_ms"] = fused
    out["loop_launches"] = 1 + int(counts.max()); out["fused_launches"] = 1
    # different noise counters (no tick in the loop): only a sanity figure
    out["max_abs_h_minus_1_loop"] = float((s_loop[:, 0] - 1).abs().max()); out["max_abs_h_minus_1_fused"] = float((s_fused[:, 0] - 1).abs().max())
    # one action step of the same batch, for scale
    a = torch.zeros((B, 10), dtype=env.tdtype, device=dev)
    env.set_random_init(None)
    for k in range(3):
        env.step(a)
    sync(); t0 = time.perf_counter()
    for k in range(20):
        env.step(a)
    sync(); out["step_ms"] = (time.perf_counter() - t0) / 20 * 1e3
print(json.dumps(out))
if len(sys.argv) > 3:
    with open(sys.argv[3], "a") as fh:
        fh.write(json.dumps(out) + "\n")

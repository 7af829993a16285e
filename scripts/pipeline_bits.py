#!/usr/bin/env python3
"""sha256 of every buffer the step pipeline writes, after one fixed sequence on five small envs in both dtypes: reset, 6
step_autoreset with every applicable feature on (normalisation everywhere; random-start reset and per-jet rewards on shkadov),
one masked step, a snapshot.  For comparing two commits that must compute the same bits (a host-side refactor): run it on both
on the same machine and diff the outputs.  Not a test: the hashes of float results change with every legitimate kernel change.
usage: python scripts/pipeline_bits.py > profiles/pipeline_bits.txt"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beacon_amd import vec as V                         # noqa: E402
from beacon_amd.envs import packaged_init               # noqa: E402

DEV = "cuda:0"
assert torch.cuda.is_available(), "pipeline_bits.py runs the kernels; there is no CPU fallback"
OVERLAP = dict(L0=30.0, jet_pos=30.0, jet_space=7.3, n_jets=4)
ENVS = [("lorenz", lambda dt: V.VecLorenz(257, DEV, dt)),
        ("burgers", lambda dt: V.VecBurgers(1, DEV, dt)),
        ("rayleigh", lambda dt: V.VecRayleigh(3, DEV, dt, init_fields=packaged_init("rayleigh"))),
        ("shkadov_one_jet", lambda dt: V.VecShkadov(3, DEV, dt, n_jets=1)),
        ("shkadov_overlap", lambda dt: V.VecShkadov(3, DEV, dt, init_fields=packaged_init("shkadov"), **OVERLAP))]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def actions(env, n, seed):
    g = torch.Generator().manual_seed(seed)
    if env.action_is_int:
        return torch.randint(0, 3, (n, env.batch), generator=g, dtype=torch.int32).to(DEV)
    shape = (n, env.batch) if env.n_actions == 1 and not isinstance(env, V.VecRayleigh) else (n, env.batch, env.n_actions)
    return (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0).to(device=DEV, dtype=env.tdtype)


for name, make in ENVS:
    for dt in ("f32", "f64"):
        env = make(dt)
        shk = isinstance(env, V.VecShkadov)
        if name == "rayleigh":
            env.set_ndt_act(5)
        if shk:
            env.set_random_init(3).set_jet_rewards()
        env.set_normalize()
        env.reset()
        env.set_stp(env.n_act - 1 - np.arange(env.batch) % 4)          # episodes end at steps 1 .. 4 of the 6
        a = actions(env, 7, 11)
        for k in range(6):
            env.step_autoreset(a[k])
        mask = torch.arange(env.batch, device=DEV) % 2 == 0
        env.step(a[6], mask=mask)
        snap = env.snapshot()
        torch.cuda.synchronize()
        bufs = [("out_buf", env.out_buf), ("snapshot", snap.buf), ("episodes", env.episodes.buf), ("normalizer", env.normalizer.buf)]
        if shk:
            bufs += [("jet_episodes", env.jet_episodes.buf), ("n_rand", env.n_rand)]
        print("%s %s episodes=%d kernel=%s" % (name, dt, int(env.episodes.count.sum()), env.kernel_name))
        for what, t in bufs:
            print("  %-12s %8d bytes  %s" % (what, t.numel() * t.element_size(), sha(t)))
        env.close()

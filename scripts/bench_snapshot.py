#!/usr/bin/env python3
"""Cost of VecEnv.snapshot / restore / fork (csrc/snapshot.hip) next to two yardsticks measured in the same process:
the FLOOR -- the snapshot's bytes moved once by the runtime's own device-to-device copy -- and the NEAREST EQUIVALENT of the
calls that existed before snapshots, set_state(get_state()) + set_stp(get_stp()) (fields and episode counter only, eight 2D
copies and two host synchronisations).  Device time from events around each call, warm-up, median.  One JSON line per case, also
appended to profiles/snapshot_bench.jsonl.  On a tree without snapshots only the equivalent is timed.
usage: python scripts/bench_snapshot.py [--reps 30] [--only rayleigh] [--out profiles/snapshot_bench.jsonl]"""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beacon_amd import vec as V

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"

CASES = [
    ("rayleigh 128x64 B=512 f32", lambda: V.VecRayleigh(512, dev, "f32", L=2.56, H=1.28)),
    ("rayleigh 128x64 B=512 f64", lambda: V.VecRayleigh(512, dev, "f64", L=2.56, H=1.28)),
    ("mixing 100x100 B=512 f32", lambda: V.VecMixing(512, dev, "f32")),
    ("shkadov N=4096 B=1024 f32", lambda: V.VecShkadov(1024, dev, "f32", None, L0=699.2, n_jets=10)),
    ("burgers N=512 B=1024 f32", lambda: V.VecBurgers(1024, dev, "f32", nx=512)),
    ("lorenz B=65536 f32", lambda: V.VecLorenz(65536, dev, "f32")),
    ("lorenz B=2^20 f32", lambda: V.VecLorenz(1 << 20, dev, "f32")),
]


def timed(fn):
    """median device microseconds of fn() over args.reps calls, each between two events"""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(us))


for name, make in CASES:
    if args.only and args.only not in name:
        continue
    env = make()
    env.reset()
    r = {"case": name}

    def equivalent():
        env.set_state(env.get_state())
        env.set_stp(env.get_stp())
    r["set_state_get_state_us"] = timed(equivalent)
    if hasattr(env, "snapshot"):
        snap = env.snapshot()
        nbytes = snap.buf.numel()
        src = torch.randint(0, env.batch, (env.batch,), device=dev, dtype=torch.int32)
        dst = torch.empty_like(snap.buf)
        r["bytes"] = nbytes
        r["floor_copy_us"] = timed(lambda: dst.copy_(snap.buf))
        r["snapshot_us"] = timed(lambda: env.snapshot(out=snap))
        r["restore_us"] = timed(lambda: env.restore(snap))
        r["restore_gather_us"] = timed(lambda: env.restore(snap, src=src))
        r["fork_us"] = timed(lambda: env.fork(src))
        r["restore_of_snapshot_us"] = timed(lambda: env.restore(env.snapshot(out=snap)))
        # snapshot bytes moved (each read once and written once) over time; fork and restore(snapshot()) move them twice
        for k, times in (("floor_copy", 1), ("snapshot", 1), ("restore", 1), ("restore_gather", 1), ("fork", 2), ("restore_of_snapshot", 2)):
            r[k + "_GBps"] = times * nbytes / r[k + "_us"] / 1e3
        r["snapshot_vs_floor"] = r["snapshot_us"] / r["floor_copy_us"]
        r["restore_vs_floor"] = r["restore_us"] / r["floor_copy_us"]
        r["restore_of_snapshot_vs_equivalent"] = r["restore_of_snapshot_us"] / r["set_state_get_state_us"]
    line = json.dumps(r)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    env.close()
    del env
    torch.cuda.empty_cache()

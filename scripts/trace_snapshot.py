#!/usr/bin/env python3
"""Known call counts for a kernel trace of the launch-bound cases: per env (burgers N = 512 B = 1024, lorenz B = 65536) 11
snapshot() and 10 restore() after one reset(), nothing else.  Under
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d <dir> -o run -- python3 scripts/trace_snapshot.py
the kernel stats must show 22 calls of snapshot_copy_k<false>, 20 of snapshot_copy_k<true> and no memory copies
(scripts/prof.sh <tag> scripts/trace_snapshot.py does the same with the counter passes on top).  DESIGN.md section 11."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from beacon_amd import vec as V

for env in (V.VecBurgers(1024, "cuda:0", "f32", nx=512), V.VecLorenz(65536, "cuda:0", "f32")):
    env.reset()
    snap = env.snapshot()
    for _ in range(10):
        env.snapshot(out=snap)
    for _ in range(10):
        env.restore(snap)
    torch.cuda.synchronize()
    env.close()
print("trace script done")

#!/usr/bin/env python
"""Cost of Renderer.draw() (csrc/render.hip) on the device, not part of bench.py: ms per draw by graph replay, and the write
bandwidth the frame bytes imply, for
    rayleigh 128x64, B = 512, scale 1 and scale 4;  mixing 100x100, B = 512, scale 4;  shkadov N = 4096, B = 1024, 512 x 128
and, in the same process and alternating with the kernel, a plain-torch restatement of the field panel (index arithmetic, lut[idx],
repeat_interleave: at least three launches and two temporaries for the same bytes), also replayed from a graph.

    python scripts/render_cost.py [--replays 200] [--rounds 5] [--out profiles/render_cost.txt]

Every line is printed and, with --out, written to that file.  Needs a GPU: without one it fails."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def graph_of(fn):
    """fn() once eagerly (code objects, allocator), then captured; returns (graph, what fn returned under capture)"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def ms_per_replay(g, replays):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        g.replay()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / replays


def torch_field(plane, lo, hi, lut, scale):
    """the field panel in plain torch: [B, ny + 2, nx + 2] -> uint8 [B, ny scale, nx scale, 3] (no strip, NaN not treated)"""
    v = plane[:, 1:-1, 1:-1].flip(1)
    idx = ((v - lo) / (hi - lo) * 256.0).clamp(0.0, 255.0).to(torch.int64)
    return lut[idx].repeat_interleave(scale, 1).repeat_interleave(scale, 2)


def seeded_fields(env, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    st = torch.rand((env.batch,) + env.state_shape(), generator=g, dtype=torch.float32) * (1.2 * (hi - lo)) + (lo - 0.1 * (hi - lo))
    env.set_state(st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_cost.py needs a ROCm GPU")
    from beacon_amd import vec as V
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# %s, torch %s; ms per call by graph replay, median (min - max) of %d rounds of %d replays" %
        (torch.cuda.get_device_name(0), torch.__version__, a.rounds, a.replays))
    L0 = next(x / 10.0 for x in range(7400, 7600) if V.VecShkadov._derive(V.VecShkadov.__new__(V.VecShkadov), L0=x / 10.0).nx == 4096)
    cases = [("rayleigh 128x64 B=512 scale 1", lambda: V.VecRayleigh(512, "cuda:0", "f32", L=2.56, H=1.28), dict(scale=1), (-0.5, 0.5)),
             ("rayleigh 128x64 B=512 scale 4", lambda: V.VecRayleigh(512, "cuda:0", "f32", L=2.56, H=1.28), dict(scale=4), (-0.5, 0.5)),
             ("mixing 100x100 B=512 scale 4", lambda: V.VecMixing(512, "cuda:0", "f32"), dict(scale=4), (0.0, 1.0)),
             ("shkadov N=4096 B=1024 512x128", lambda: V.VecShkadov(1024, "cuda:0", "f32", L0=L0), dict(width=512, height=128), None)]
    for name, make, kw, rng in cases:
        env = make()
        env.reset()
        if rng is not None:
            seeded_fields(env, rng[0], rng[1], 1)
        else:
            assert env.nx == 4096
            st = env.get_state()
            st[:, 0] = 1.0 + 0.4 * torch.sin(torch.linspace(0.0, 60.0, env.nx, device=st.device))[None, :] * torch.rand((env.batch, 1), device=st.device)
            env.set_state(st)
        # the field panels twice: as renderer() draws them by default, and without the strip -- the bytes the plain-torch panel writes
        rds = [("draw()", env.renderer(**kw))] + ([("draw(strip=0)", env.renderer(strip=0, **kw))] if rng is not None else [])
        graphs = [(what, rd, graph_of(rd.draw)[0]) for what, rd in rds]
        if rng is not None:
            plane, lut, bare = env.get_state()[:, 3].contiguous(), rds[1][1].lut, rds[1][1].frames
            g_t, out_t = graph_of(lambda: torch_field(plane, rng[0], rng[1], lut, kw["scale"]))
            graphs.append(("plain torch", None, g_t))
            say("%-30s bytes in which the kernel's panel and the plain-torch one differ: %d of %d" % (name, int((bare != out_t).sum()), bare.numel()))
        times = [[] for _ in graphs]
        for _ in range(a.rounds):                          # alternating: the arms share whatever else the machine does
            for k, (_, _, g) in enumerate(graphs):
                times[k].append(ms_per_replay(g, a.replays))
        med = [float(np.median(t)) for t in times]
        for (what, rd, _), t, m in zip(graphs, times, med):
            nbytes = out_t.numel() if rd is None else rd.frames.numel()
            say("%-30s %-13s %8.4f ms (%.4f - %.4f)  %6.1f MB per call  %5.2f TB/s written%s" %
                (name, what, m, min(t), max(t), nbytes / 1e6, nbytes / m / 1e9, "" if rd is not None else "  draw(strip=0) / torch = %.3f" % (med[1] / m)))
        env.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

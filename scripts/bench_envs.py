#!/usr/bin/env python3
"""Secondary benchmark lines (BASELINE.json configs 2, 3, 5 + sloshing, lorenz, vortex): env steps/s and effective GB/s
(SURVEY 8d algorithmic bytes / launch time) of the other solver kernels on one GPU, with the float64 C
oracle timed on a bounded sample next to each.  Not the headline metric (that is bench.py).
usage: python scripts/bench_envs.py [--steps K] [--no-cpu] [--only burgers,lorenz,...] [--params] [--variant 0]
--params gives every replica its own physical parameters (VecEnv.set_params: a full table; the 2D envs then run the generic kernel,
or with --opt params_kernel=1 their register-resident kernels that read the table: _VecNS2D.set_params_kernel);
"rayleigh" (the headline grid at B = 512) and "tall" run only when named in --only."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# Bytes per replica-step that an ODE kernel must move (esz = 4 / 8), with actions given:
#   lorenz: read x[3], t (4 reals), the int32 action and stp; write x[3], fx[3], t (7 reals), the action, stp, obs[6] and rwd
#           (7 reals), done, trunc (2 B) and status (4 B)              -> 18 esz + 22 B  (f64 166 B, f32 94 B)
#   vortex: read x[4], t, y (6 reals), the action[2] (2 reals) and stp; write x[4], fx[4], t, y, kmod, kphase, u[2] (14 reals),
#           stp, obs[8] and rwd (9 reals), done, trunc and status        -> 31 esz + 14 B  (f64 262 B, f32 138 B)
# with per-replica parameters set (VecEnv.set_params) a replica reads its columns of the table besides: lorenz 3 reals (sigma, rho,
# beta: f32 106 B, f64 190 B), vortex 2 (ire, weight: f32 146 B, f64 278 B)
ODE_BYTES = {"lorenz": (18, 22), "vortex": (31, 14)}
ODE_PARAM_REALS = {"lorenz": 3, "vortex": 2}


def ode_bytes_per_replica_step(name, esz, params=False):
    nr, ni = ODE_BYTES[name]
    return (nr + (ODE_PARAM_REALS[name] if params else 0)) * esz + ni


def spread_params(env):
    """a full table: every parameter of every replica within +-10 % of the constructor's value, a different factor per replica"""
    B = env.batch
    f = 1.0 + 0.1 * np.cos(np.arange(B) * 0.7)
    env.set_params(**{k: v * np.roll(f, 3 * i) for i, (k, v) in enumerate(env.params.items())})


def apply_opts(env, opts):
    """--opt name=value: bcn_set_option; params_kernel goes through set_params_kernel, which also attaches an on-demand grid's
    table-reading kernel"""
    for o in opts:
        name, value = o.split("=")[0], int(o.split("=")[1])
        if name == "params_kernel" and hasattr(env, "set_params_kernel"):
            env.set_params_kernel("fast" if value else "generic")
        else:
            env.set_option(name, value)


def main():
    sys.path.insert(0, ROOT)
    from beacon_amd import vec as V
    from beacon_amd.envs import packaged_init
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--ode-batch", type=int, action="append", default=[], help="lorenz / vortex batch sizes (default 1024, 65536, 2^20)")
    ap.add_argument("--params", action="store_true", help="every replica with its own physical parameters (VecEnv.set_params): a full table")
    ap.add_argument("--variant", type=int, default=-1, help="2D envs: bcn_set_variant (0 = the generic kernel)")
    ap.add_argument("--opt", action="append", default=[], help="name=value for bcn_set_option on every env (e.g. cells_per_thread=4)")
    args = ap.parse_args()
    dev = "cuda:0"


    def timed(env, step_fn, K, W):
        for k in range(W):
            step_fn(k)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
        t0 = time.perf_counter()
        for k in range(K):
            ev[k][0].record(); step_fn(W + k); ev[k][1].record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return wall, float(np.mean([a.elapsed_time(b) for a, b in ev]))


    def cpu_1d(make, step, seconds=8.0):
        from oracle import oracle as O
        e = make(O)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            step(e, n); n += 1
        return n / (time.perf_counter() - t0)


    out = []
    K, W = args.steps, args.warmup
    rng = np.random.default_rng(7)

    if not args.only or "burgers" in args.only:
        B = 1024
        env = V.VecBurgers(B, dev, "f32", nx=512)
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        a = torch.as_tensor(rng.uniform(-1, 1, (K + W, B)), dtype=torch.float32, device=dev)
        nz = torch.as_tensor(rng.uniform(-0.1, 0.1, (K + W, B)), dtype=torch.float32, device=dev)
        wall, ms = timed(env, lambda k: env.step(a[k], nz[k]), K, W)
        bytes_ = 12.0 * env.nx * env.ndt_act * B
        r = {"env": "burgers-v0 B=1024 N=512 (BASELINE configs[1])", "kernel": env.kernel_name, "env_steps_per_s": B * K / wall,
             "launch_ms": ms, "effective_GBps": bytes_ / (ms * 1e-3) / 1e9, "dtype": "f32", "params": bool(args.params)}
        if not args.no_cpu:
            r["cpu_oracle_env_steps_per_s_1core"] = cpu_1d(lambda O: (lambda e: (e.reset(), e)[1])(O.burgers(nx=512)),
                                                           lambda e, n: e.step([0.3], 0.05))
        out.append(r); env.close()

    if not args.only or "shkadov" in args.only:
        B = 1024
        env = V.VecShkadov(B, dev, "f32", None, L0=699.2, n_jets=10)
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        # from a developed film (shkadov/init.py: 4000 uncontrolled action steps under inlet noise), as bench.py's line
        env.warmup(env.n_warmup_ref, torch.zeros((B, 10), dtype=torch.float32, device=dev))
        a = torch.as_tensor(rng.uniform(-1, 1, (K + W, B, 10)), dtype=torch.float32, device=dev)
        nz = torch.as_tensor(rng.uniform(-5e-4, 5e-4, (K + W, B, 50)), dtype=torch.float32, device=dev)
        wall, ms = timed(env, lambda k: env.step(a[k], nz[k]), K, W)
        bytes_ = 32.0 * env.nx * env.ndt_act * B
        r = {"env": "shkadov-v0 B=1024 10 jets N=4096 (BASELINE configs[2])", "kernel": env.kernel_name,
             "env_steps_per_s": B * K / wall, "launch_ms": ms, "effective_GBps": bytes_ / (ms * 1e-3) / 1e9, "dtype": "f32", "params": bool(args.params)}
        if not args.no_cpu:
            def mk(O):
                e = O.shkadov(init=False, L0=699.2, n_jets=10); e.reset_fields(); return e
            r["cpu_oracle_env_steps_per_s_1core"] = cpu_1d(mk, lambda e, n: e.step([0.1] * 10, np.zeros(50)))
        out.append(r); env.close()

    if not args.only or "sloshing" in args.only:
        B = 1024
        env = V.VecSloshing(B, dev, "f32", packaged_init("sloshing"))
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        a = torch.as_tensor(rng.uniform(-1, 1, (K + W, B)), dtype=torch.float32, device=dev)
        wall, ms = timed(env, lambda k: env.step(a[k]), K, W)
        bytes_ = 32.0 * env.nx * env.ndt_act * B
        r = {"env": "sloshing-v0 B=1024 N=200", "kernel": env.kernel_name, "env_steps_per_s": B * K / wall,
             "launch_ms": ms, "effective_GBps": bytes_ / (ms * 1e-3) / 1e9, "dtype": "f32", "params": bool(args.params)}
        if not args.no_cpu:
            def mk(O):
                e = O.sloshing(init_fields=packaged_init("sloshing")); e.reset(); return e
            r["cpu_oracle_env_steps_per_s_1core"] = cpu_1d(mk, lambda e, n: e.step([0.2]))
        out.append(r); env.close()

    if not args.only or "mixing" in args.only:
        B = 512
        env = V.VecMixing(B, dev, "f32")
        if args.variant >= 0:
            env.set_variant(args.variant)
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        a = torch.as_tensor(rng.integers(0, 4, (K + W, B)), dtype=torch.int32, device=dev)
        Km, Wm = min(K, 4), 1
        wall, ms = timed(env, lambda k: env.step(a[k]), Km, Wm)
        sw = env.sweeps.cpu().numpy()
        bytes_ = env.nx * env.ny * 4.0 * (20.0 * sw.size + 3.0 * float(sw.sum()))
        r = {"env": "mixing-v0 B=512 100x100 (BASELINE configs[4]), first steps from rest", "kernel": env.kernel_name,
             "env_steps_per_s": B * Km / wall, "launch_ms": ms, "effective_GBps": bytes_ / (ms * 1e-3) / 1e9,
             "mean_sweeps_per_timestep": float(sw.mean()), "dtype": "f32", "params": bool(args.params)}
        out.append(r); env.close()

    if "rayleigh" in args.only:   # the headline grid (bench.py) at B = 512, first steps from the packaged start: the price of the generic kernel
        B = 512
        env = V.VecRayleigh(B, dev, "f32", None, L=2.56, H=1.28)
        if args.variant >= 0:
            env.set_variant(args.variant)
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        env.set_state(np.tile(np.ascontiguousarray(env.perturbed_conduction_state().transpose(0, 2, 1))[None], (B, 1, 1, 1)))
        a = torch.as_tensor(rng.uniform(-0.75, 0.75, (K + 1, B, env.n_sgts)), dtype=torch.float32, device=dev)
        Km, Wm = min(K, 2), 1
        wall, ms = timed(env, lambda k: env.step(a[k]), Km, Wm)
        sw = env.sweeps.cpu().numpy()
        r = {"env": "rayleigh-v0 128x64 B=512, first steps from the perturbed conduction state", "kernel": env.kernel_name,
             "env_steps_per_s": B * Km / wall, "launch_ms": ms, "mean_sweeps_per_timestep": float(sw.mean()), "dtype": "f32", "params": bool(args.params)}
        out.append(r); env.close()

    if "tall" in args.only:      # a grid above ny = 128 (ns2d_fast4_impl.h): mixing(L=1, H=2) = 100x200, one replica per CU
        B = 256
        env = V.VecMixing(B, dev, "f32", L=1.0, H=2.0)
        apply_opts(env, args.opt)
        if args.params:
            spread_params(env)
        env.reset()
        a = torch.as_tensor(rng.integers(0, 4, (K + 3, B)), dtype=torch.int32, device=dev)
        Km, Wm = min(K, 3), 3
        wall, ms = timed(env, lambda k: env.step(a[k]), Km, Wm)
        sw = env.sweeps.cpu().numpy()
        bytes_ = env.nx * env.ny * 4.0 * (20.0 * sw.size + 3.0 * float(sw.sum()))
        r = {"env": "mixing-v0 L=1 H=2 (100x200) B=256", "kernel": env.kernel_name,
             "env_steps_per_s": B * Km / wall, "launch_ms": ms, "effective_GBps": bytes_ / (ms * 1e-3) / 1e9,
             "mean_sweeps_per_timestep": float(sw.mean()), "dtype": "f32", "params": bool(args.params)}
        out.append(r); env.close()

    # the ODE envs (csrc/ode_env.h): one lane per replica, B from a trainer's 1 024 to 2^20; eager steps and a 100-step StepGraph.
    for name in ("lorenz", "vortex"):
        if args.only and name not in args.only:
            continue
        cls = V.VecLorenz if name == "lorenz" else V.VecVortex
        for B in (args.ode_batch or (1024, 65536, 1 << 20)):
            for dt in ("f32", "f64"):
                env = cls(B, dev, dt)
                apply_opts(env, args.opt)
                env.reset()
                gen = torch.Generator(device=dev)
                gen.manual_seed(7)
                if name == "lorenz":
                    a = torch.randint(0, 3, (100, B), generator=gen, device=dev, dtype=torch.int32)
                else:
                    a = (2 * torch.rand((100, B, 2), generator=gen, device=dev, dtype=torch.float64) - 1).to(env.tdtype)
                if args.params:
                    spread_params(env)
                bytes_ = ode_bytes_per_replica_step(name, 4 if dt == "f32" else 8, params=args.params) * B
                wall, ms = timed(env, lambda k: env.step(a[k % 100]), K, W)
                g = env.capture(a, n_steps=100, keep_steps=False)
                g.replay()
                torch.cuda.synchronize()
                reps = max(1, K // 20)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                gms = e0.elapsed_time(e1) / (100 * reps)
                r = {"env": "%s-v0 B=%d" % (name, B), "dtype": dt, "kernel": env.kernel_name, "bytes_per_replica_step": bytes_ / B,
                     "eager_env_steps_per_s": B * K / wall, "eager_us_per_step": ms * 1e3,
                     "eager_effective_GBps": bytes_ / (ms * 1e-3) / 1e9,
                     "graph_env_steps_per_s": B / (gms * 1e-3), "graph_us_per_step": gms * 1e3,
                     "graph_effective_GBps": bytes_ / (gms * 1e-3) / 1e9, "opts": args.opt, "params": bool(args.params)}
                out.append(r)
                del g
                env.close()

    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

"""Every 2D kernel family against the float64 oracle from ENERGETIC, asymmetric flow (tests/flow_states.py).

The other oracle comparisons of the on-demand kernels start from a fluid at rest, where a wrong neighbour in a convective term or
in a transport coefficient moves a float32 result by less than its tolerance (tests/golden/energetic_sensitivity.json
has the reference's own numbers).  Here every replica starts from velocities of 0.5 (rayleigh) or 1.0 (mixing) without symmetry.

Nothing here reads the reference tree."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import flow_states as FS
from test_gpu_parity import DEV, F64_TOL, _oracle_replica, dev2ref, f32tol, maxdiff

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from beacon_amd import vec as V


@pytest.mark.parametrize("idx", range(len(FS.CASES)), ids=[FS.case_id(c) for c in FS.CASES])
def test_kernels_vs_oracle_from_energetic_flow(idx):
    """flow_states.CASES -- the built-in grids (rayleigh 50x50, 128x64, mixing 100x100) and the smallest on-demand grid of every
    (rows per lane, dtype, env) family, plus one grid with dx != dy -- through the generic kernel, the register-resident kernel in a
    plain launch and under the ticket scheduler (2, 2, 2), against the float64 oracle.  The protocol of test_jit_kernels_vs_oracle,
    but B = 4 replicas with their OWN start state (flow_states.energetic_state, seeds 0..3, max(|u|, |v|) = 0.5 for rayleigh, 1.0 for mixing) and their own
    action, and one env step of 4 timesteps.  All four fields (ghosts included), obs, rwd and the sweep counts of every timestep:
    float64 1e-9 (p 5e-8) with counts within 1; float32 flow_states.F32_ENERGETIC[rows, kind] (10 x the measured error, capped by
    tests/test_flow_states_host.py from the reference's sensitivity to a slipped neighbour), the first two counts within max(3, 2 %)
    and the total within 2 %.  The register-resident kernel is the one choose() names (built-in grids: the library's own); plain and ticket launches are bit-identical
    in obs, rwd, counts and interior fields; no two replicas compute the same."""
    from beacon_amd import jit
    c = FS.CASES[idx]
    kind, L, H, kw, dt = c["kind"], c["L"], c["H"], c["kw"], c["dtype"]
    f64 = dt == "f64"
    B = FS.BATCH
    st0, acts = FS.case_inputs(c)
    dev0 = np.ascontiguousarray(np.swapaxes(st0, -1, -2))
    mk = (lambda: V.VecRayleigh(B, DEV, dt, None, L=L, H=H, **kw)) if kind == 0 else (lambda: V.VecMixing(B, DEV, dt, L=L, H=H, **kw))
    runs = {}
    for tag, variant, sched in (("generic", 0, None), ("plain", 1, (0, 0, 0)), ("ticket", 1, (2, 2, 2))):
        env = mk()
        try:
            nx, ny = env.nx, env.ny
            assert (nx, ny) == (c["nx"], c["ny"])
            assert ((nx, ny, f64, kind) in jit.BUILTIN_GRIDS) == c["builtin"]
            if variant and not c["builtin"]:
                p = getattr(env, "_plugin", None)
                assert p is not None and p.verified is True, "no verified plugin for %dx%d %s" % (nx, ny, dt)
            env.set_ndt_act(FS.NDT)
            assert env.set_variant(variant) == variant
            if sched is not None:
                env.set_sched(*sched)
            env.reset()
            env.set_state(dev0)
            obs, rwd, _, _, _ = env.step(acts)
            env.check_status()
            if variant:
                assert env.kernel_name == {1: "ns2d_fast", 2: "ns2d_fast2", 4: "ns2d_fast4"}[FS.rows(c)] + ("_sched" if sched[0] == 2 else "_step")
            else:
                assert env.kernel_name == "ns2d_generic_step"
            n = 3 * env.nx_obs_pts * env.ny_obs_pts
            runs[tag] = (dev2ref(env.get_state()), obs.double().cpu().numpy()[:, -n:], rwd.double().cpu().numpy(),
                         env.sweeps.cpu().numpy().astype(np.int64))
        finally:
            env.close()
    with ThreadPoolExecutor(max_workers=B) as ex:       # the ctypes calls of the oracle release the GIL
        ref = list(ex.map(lambda b: _oracle_replica(kind, L, H, kw, FS.NDT, st0[b], acts[b]), range(B)))
    S = "T" if kind == 0 else "C"
    names = list("uvp" + S) + ["obs", "rwd"]
    err = {tag: dict.fromkeys(names, 0.0) for tag in runs}
    dsw = {tag: 0 for tag in runs}
    for tag in runs:
        st, obs, rwd, sw = runs[tag]
        for b in range(B):
            rst, rob, rrw, ritp = ref[b]
            for i, F in enumerate("uvp" + S):
                err[tag][F] = max(err[tag][F], maxdiff(st[b][i], rst[i], tag=F))
            err[tag]["obs"] = max(err[tag]["obs"], maxdiff(obs[b], rob[-obs.shape[1]:], tag="obs"))
            err[tag]["rwd"] = max(err[tag]["rwd"], maxdiff(rwd[b], rrw, tag="rwd"))
            dsw[tag] = max(dsw[tag], int(np.abs(sw[b] - ritp).max()))
    fam = FS.family(c)
    for tag in ("generic", "plain", "ticket"):
        print("MEASURED %s family %s %s: %s | sweeps off by <= %d of %s"
              % (FS.case_id(c), fam, tag, " ".join("%s %.1e" % (F, err[tag][F]) for F in names), dsw[tag],
                 [int(ref[b][3].max()) for b in range(B)]))
    if f64:
        t = f32tol(F64_TOL, F64_TOL, 50 * F64_TOL, F64_TOL, F64_TOL, F64_TOL)
    else:
        t = FS.F32_ENERGETIC[fam]
    fails = []
    for tag in ("generic", "plain", "ticket"):
        st, obs, rwd, sw = runs[tag]
        for F in names:
            if not err[tag][F] <= t[F]:
                fails.append("%s %s: %.3e > %.1e" % (tag, F, err[tag][F], t[F]))
        for b in range(B):
            ritp = ref[b][3]
            if f64:
                good = np.all(np.abs(sw[b] - ritp) <= 1)
            else:
                good = (np.all(np.abs(sw[b][:2] - ritp[:2]) <= np.maximum(3, 0.02 * ritp[:2])) and
                        abs(int(sw[b].sum()) - int(ritp.sum())) <= 0.02 * ritp.sum())
            if not good:
                fails.append("%s replica %d sweeps %s vs oracle %s" % (tag, b, sw[b].tolist(), ritp.tolist()))
    assert not fails, fails
    pl, tk = runs["plain"], runs["ticket"]
    assert np.array_equal(pl[1], tk[1]) and np.array_equal(pl[2], tk[2]) and np.array_equal(pl[3], tk[3])
    assert np.array_equal(pl[0][:, :, 1:-1, 1:-1], tk[0][:, :, 1:-1, 1:-1])
    for a in range(B):              # distinct states per replica: a kernel that mixes replicas up, or steps one twice, shows here
        for b in range(a + 1, B):
            for i in range(4):
                assert not np.array_equal(pl[0][a, i, 1:-1, 1:-1], pl[0][b, i, 1:-1, 1:-1]), (a, b, i)
            assert not np.array_equal(pl[1][a], pl[1][b]) and pl[2][a] != pl[2][b], (a, b)

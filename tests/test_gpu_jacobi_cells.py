"""The float32 one-row-per-lane Jacobi cells stated in runs -- several cells per asm statement (csrc/bcn_jacobi_cells.h,
csrc/ns2d_fast_runs.hip) -- on the strip widths that take different run shapes, against the float64 oracle.

    128x64  built in   R = 16: interior runs 7 + 7 and 6 + 6 (full runs), the four edge and the four exchanged cells one statement each
    50x50   built in   R = 5:  a short run of 3 and a single-cell run
    53x50   on demand  R = 7 (odd), last strip 4 wide: one run of 5, a remainder run of 3; the last wave: a run of 2 and no second run
    150x50  built in   R = 15 (odd): a full run and a remainder run, 7 + 6; the second sweep's 11 inner cells as 5, the barrier, 6

Each case first asks what it runs on: the library says whether a built-in grid steps through the kernels with runs
(bcn_builtin_cell_runs; both units' kernels carry the same names), the plugin says it of itself (bcn_jit_cell_runs).

Per grid: 3 replicas from the energetic states of tests/flow_states.py (seeds 0..2), each with its own action, one env step of 4
timesteps, through the register-resident kernel in a plain launch and under the ticket scheduler, under the default evaluation plan
and under conv_plan 0 (every sweep evaluated: the single evaluated sweeps' and the pairs' cells instead of the plain double
sweeps').  Fields (ghosts included), obs and rwd within flow_states.F32_ENERGETIC[(1, 0)] -- the tolerance of
tests/test_gpu_energetic.py for this kernel family from these states --, and the sweep count of every timestep EQUAL under both plans.
The oracle runs once per grid.  Nothing here reads the reference tree."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import flow_states as FS
from test_gpu_parity import DEV, _oracle_replica, dev2ref, maxdiff

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from beacon_amd import vec as V

B = 3
# (case, strip width R, columns of the last strip)
GRIDS = [(FS._case(0, 128, 64, "f32", 1), 16, 16), (FS._case(0, 50, 50, "f32", 1), 5, 5), (FS._case(0, 53, 50, "f32"), 7, 4),
         (FS._case(0, 150, 50, "f32", 1), 15, 15)]
LAUNCHES = [("plain", (0, 0, 0)), ("ticket", (2, 2, 2))]


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(gi):
    c = GRIDS[gi][0]
    st0, acts = FS.case_inputs(c)
    st0, acts = st0[:B], acts[:B]
    with ThreadPoolExecutor(max_workers=B) as ex:       # the ctypes calls of the oracle release the GIL
        ref = list(ex.map(lambda b: _oracle_replica(0, c["L"], c["H"], c["kw"], FS.NDT, st0[b], acts[b]), range(B)))
    st0.setflags(write=False)
    return st0, acts, ref


def _strip_width(c):
    from beacon_amd import jit
    if c["builtin"]:
        row, = [b for b in jit.builtin_rows() if (b["nx"], b["ny"], b["f64"], b["kind"]) == (c["nx"], c["ny"], 0, 0)]
        return row["rows"], row["R"], c["nx"] - (-(-c["nx"] // row["R"]) - 1) * row["R"]
    m = jit.choose(c["nx"], c["ny"], False, 0)
    return m["rows"], m["R"], jit.geometry(1, c["nx"], c["ny"], m["R"], m["gf"], False)["rl"]


@pytest.mark.parametrize("launch", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
@pytest.mark.parametrize("gi", range(len(GRIDS)), ids=[FS.case_id(g[0]) for g in GRIDS])
def test_cell_runs_vs_oracle_and_sweep_counts_under_both_plans(gi, launch):
    c, R, RL = GRIDS[gi]
    tag, sched = LAUNCHES[launch]
    assert _strip_width(c) == (1, R, RL), "the mapping this case was chosen for"
    if c["builtin"]:
        from beacon_amd import _lib
        assert _lib.load().bcn_builtin_cell_runs(c["nx"], c["ny"]) == 1, "this grid does not step through the kernels with runs"
    st0, acts, ref = _inputs_and_oracle(gi)
    dev0 = np.ascontiguousarray(np.swapaxes(st0, -1, -2))
    runs = {}
    for plan in (None, 0):
        env = V.VecRayleigh(B, DEV, "f32", None, L=c["L"], H=c["H"], **c["kw"])
        try:
            assert (env.nx, env.ny) == (c["nx"], c["ny"])
            if not c["builtin"]:
                p = getattr(env, "_plugin", None)
                assert p is not None and p.verified is True, "no verified plugin for %dx%d" % (env.nx, env.ny)
                assert ctypes.CDLL(p.path).bcn_jit_cell_runs() == 1, "the plugin's kernels do not have the runs"
            env.set_ndt_act(FS.NDT)
            assert env.set_variant(1) == 1
            env.set_sched(*sched)
            if plan is not None:
                env.set_option("conv_plan", plan)
            env.reset()
            env.set_state(dev0)
            obs, rwd, _, _, _ = env.step(acts.copy())
            env.check_status()
            assert env.kernel_name == "ns2d_fast" + ("_sched" if sched[0] == 2 else "_step")
            n = 3 * env.nx_obs_pts * env.ny_obs_pts
            runs[plan] = (dev2ref(env.get_state()), obs.double().cpu().numpy()[:, -n:], rwd.double().cpu().numpy(),
                          env.sweeps.cpu().numpy().astype(np.int64))
        finally:
            env.close()
    t = FS.F32_ENERGETIC[(1, 0)]
    names = list("uvpT") + ["obs", "rwd"]
    fails = []
    for plan, (st, obs, rwd, sw) in runs.items():
        err = dict.fromkeys(names, 0.0)
        for b in range(B):
            rst, rob, rrw, _ = ref[b]
            for i, F in enumerate("uvpT"):
                err[F] = max(err[F], maxdiff(st[b][i], rst[i], tag=F))
            err["obs"] = max(err["obs"], maxdiff(obs[b], rob[-obs.shape[1]:], tag="obs"))
            err["rwd"] = max(err["rwd"], maxdiff(rwd[b], rrw, tag="rwd"))
        print("MEASURED %s %s conv_plan %s: %s | sweeps %s, oracle %s"
              % (FS.case_id(c), tag, "default" if plan is None else plan, " ".join("%s %.1e" % (F, err[F]) for F in names),
                 sw.tolist(), [ref[b][3].tolist() for b in range(B)]))
        fails += ["conv_plan %s %s: %.3e > %.1e" % (plan, F, err[F], t[F]) for F in names if not err[F] <= t[F]]
    assert not fails, fails
    # the default plan skips evaluations, never sweeps: it stops where the plan that evaluates every sweep stops
    assert runs[None][3].shape == (B, FS.NDT) and np.array_equal(runs[None][3], runs[0][3]), (runs[None][3].tolist(), runs[0][3].tolist())
    for a in range(B):              # distinct replicas
        for b in range(a + 1, B):
            assert not np.array_equal(runs[None][1][a], runs[None][1][b])

"""What the float64 reference says a slipped neighbour costs -- TEST INFRASTRUCTURE.

A register-resident kernel that maps one column or one row of cells to the wrong lane reads ONE wrong neighbour in that column or
row; its formulas are right.  This script plants such slips in copies of oracle/beacon_oracle.c -- one textual single-site
replacement at a time, each asserted to match exactly once, each confined to the column i == nx / 2 + 2 or the row j == ny / 2 + 2 --
builds every copy with the Makefile's flags and runs the original and the mutant through two protocols on the CPU:

  energetic   tests/test_gpu_energetic.py: replica b starts from flow_states.energetic_state(seed b), own action, 4 timesteps;
  quiet       tests/test_gpu_parity.py::test_jit_kernels_vs_oracle: jit._seeded_rayleigh_state / reset(), 12 timesteps.

Recorded per grid of flow_states.CASES, mutation and protocol: max |mutant - original| of u, v, p, T/C (ghosts included), obs and rwd
and the largest difference of a sweep count, each the largest over the 4 replicas (a test fails when one replica does).  Output:
tests/golden/energetic_sensitivity.json -- numbers and names only.  tests/test_flow_states_host.py recomputes two entries (a stale
file is a red test) and caps the float32 tolerances of the GPU test from this file.  Run from the repo root:
python oracle/make_sensitivity.py"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O                      # noqa: E402
import flow_states as FS                            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "energetic_sensitivity.json")
QUIET_NDT = 12
COL, ROW = "i == nx / 2 + 2", "j == ny / 2 + 2"

# name -> (what slips, text of oracle/beacon_oracle.c, its replacement).  Outside the one column / row a mutant computes the
# original's bits: the replaced expression is kept under the other arm of the conditional.
MUTATIONS = {
    "u_conv_diag_col": ("u-convection: v(i-1, j+1) read as v(i, j+1) in one column",
                        "double vN = 0.5 * (F(v, i, j + 1) + F(v, i - 1, j + 1));",
                        "double vN = 0.5 * (F(v, i, j + 1) + F(v, (%s) ? i : i - 1, j + 1));" % COL),
    "u_conv_diag_row": ("u-convection: v(i-1, j+1) read as v(i-1, j) in one row",
                        "double vN = 0.5 * (F(v, i, j + 1) + F(v, i - 1, j + 1));",
                        "double vN = 0.5 * (F(v, i, j + 1) + F(v, i - 1, (%s) ? j : j + 1));" % ROW),
    "v_conv_diag_row": ("v-convection: u(i+1, j-1) read as u(i+1, j) in one row",
                        "double uE = 0.5 * (F(u, i + 1, j) + F(u, i + 1, j - 1));",
                        "double uE = 0.5 * (F(u, i + 1, j) + F(u, i + 1, (%s) ? j : j - 1));" % ROW),
    "v_conv_diag_col": ("v-convection: u(i+1, j-1) read as u(i, j-1) in one column",
                        "double uE = 0.5 * (F(u, i + 1, j) + F(u, i + 1, j - 1));",
                        "double uE = 0.5 * (F(u, i + 1, j) + F(u, (%s) ? i : i + 1, j - 1));" % COL),
    "u_face_avg_col": ("u-equation: the east face average takes u(i, j) twice in one column",
                       "double uE = 0.5 * (F(u, i + 1, j) + F(u, i, j));",
                       "double uE = 0.5 * (F(u, (%s) ? i : i + 1, j) + F(u, i, j));" % COL),
    "v_face_avg_row": ("v-equation: the south face average takes v(i, j-2) for v(i, j-1) in one row",
                       "double vS = 0.5 * (F(v, i, j) + F(v, i, j - 1));",
                       "double vS = 0.5 * (F(v, i, j) + F(v, i, (%s) ? j - 2 : j - 1));" % ROW),
    "tr_face_ew_col": ("transport: the east face velocity u(i+1, j) read as u(i, j) in one column",
                       "double uE = F(u, i + 1, j), uW = F(u, i, j),",
                       "double uE = F(u, (%s) ? i : i + 1, j), uW = F(u, i, j)," % COL),
    "tr_face_ns_row": ("transport: the north face velocity v(i, j+1) read as v(i, j) in one row",
                       "vN = F(v, i, j + 1), vS = F(v, i, j);",
                       "vN = F(v, i, (%s) ? j : j + 1), vS = F(v, i, j);" % ROW),
    "tr_coef_west_col": ("transport: the velocity inside the implicit west coefficient (the factor of the new T(i-1, j)) is u(i-1, j) in one column",
                         "(uE * TE - uW * TW) / dx",
                         "(uE * TE - ((%s) ? 0.5 * (F(u, i - 1, j) * F(T, i - 1, j) + uW * F(T, i, j)) : uW * TW)) / dx" % COL),
    "tr_coef_south_row": ("transport: the velocity inside the implicit south coefficient (the factor of the new T(i, j-1)) is v(i, j-1) in one row",
                          "(vN * TN - vS * TS) / dy;",
                          "(vN * TN - ((%s) ? 0.5 * (F(v, i, j - 1) * F(T, i, j - 1) + vS * F(T, i, j)) : vS * TS)) / dy;" % ROW),
}
FIELDS = ("u", "v", "p", "S", "obs", "rwd", "sweeps")


def makefile_flags():
    """CC and CFLAGS as oracle/Makefile states them."""
    val = {}
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            for k in ("CC", "CFLAGS"):
                if line.startswith(k + " ?= "):
                    val[k] = line.split("?= ", 1)[1].split()
    return val["CC"], val["CFLAGS"]


def build_mutants(names, tmp):
    """{name: CDLL}, "original" included: each one a copy of this repository's beacon_oracle.c with one replacement."""
    cc, cflags = makefile_flags()
    with open(os.path.join(ROOT, "oracle", "beacon_oracle.c")) as fh:
        src = fh.read()
    libs = {}
    for name in ["original"] + list(names):
        text = src
        if name != "original":
            _, old, new = MUTATIONS[name]
            assert src.count(old) == 1, (name, src.count(old))
            text = src.replace(old, new)
        cfile, so = os.path.join(tmp, name + ".c"), os.path.join(tmp, name + ".so")
        with open(cfile, "w") as fh:
            fh.write(text)
        subprocess.check_call(cc + cflags + ["-shared", "-o", so, cfile, "-lm"])
        L = C.CDLL(so)
        L.orc_ns2d_rwd.restype = C.c_double
        libs[name] = L
    return libs


def run_replica(L, c, ndt, st0, a):
    """One replica of case `c` through the library L: (fields [4, nx+2, ny+2], newest obs, rwd, sweeps per timestep).  st0 None:
    the env's own reset state.  The same sequence as oracle.py's step(): condition the action, solve, obs, rwd."""
    kind = c["kind"]
    o = O.rayleigh(init=False, L=c["L"], H=c["H"], **c["kw"]) if kind == 0 else O.mixing(L=c["L"], H=c["H"], **c["kw"])
    o.cfg.ndt_act = ndt
    o.reset_fields()
    if st0 is not None:
        o.st[:4] = st0
    av = np.array(a, dtype=np.float64).reshape(-1) if kind == 0 else np.array([float(a)])
    if kind == 0:
        L.orc_rayleigh_condition_action(C.byref(o.cfg), O.dp(av))
    itp = np.zeros(ndt, dtype=np.int32)
    rc = L.orc_ns2d_solve(C.byref(o.cfg), O.dp(o.st.reshape(-1)), O.dp(av), itp.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, "the Jacobi solve ran into itmax"
    L.orc_ns2d_obs(C.byref(o.cfg), O.dp(o.u), O.dp(o.v), O.dp(o.S), O.dp(o.obs))
    n = 3 * o.cfg.nx_obs_pts * o.cfg.ny_obs_pts
    return o.st[:4].copy(), o.obs.reshape(-1)[-n:].copy(), float(L.orc_ns2d_rwd(C.byref(o.cfg), O.dp(o.S))), itp.astype(np.int64)


def protocol_inputs(c, protocol):
    """(ndt, states or None per replica, actions) of a protocol."""
    if protocol == "energetic":
        st, acts = FS.case_inputs(c)
        return FS.NDT, list(st), acts
    if c["kind"] == 0:
        from beacon_amd import jit
        env = types.SimpleNamespace(nx=c["nx"], ny=c["ny"], L=c["L"], batch=1)
        st0 = np.swapaxes(jit._seeded_rayleigh_state(env)[0], -1, -2)
        return QUIET_NDT, [st0] * FS.BATCH, np.random.default_rng(0).uniform(-1, 1, (FS.BATCH, c["kw"].get("n_sgts", 10)))
    return QUIET_NDT, [None] * FS.BATCH, np.arange(FS.BATCH)


def run_protocol(L, c, protocol):
    ndt, sts, acts = protocol_inputs(c, protocol)
    return [run_replica(L, c, ndt, sts[b], acts[b]) for b in range(FS.BATCH)]


def effect(ref, mut):
    """max over the replicas of max |mutant - original| per quantity."""
    e = dict.fromkeys(FIELDS, 0.0)
    for (rs, ro, rr, ri), (ms, mo, mr, mi) in zip(ref, mut):
        for k, F in enumerate("uvpS"):
            e[F] = max(e[F], float(np.abs(ms[k] - rs[k]).max()))
        e["obs"] = max(e["obs"], float(np.abs(mo - ro).max()))
        e["rwd"] = max(e["rwd"], abs(mr - rr))
        e["sweeps"] = max(e["sweeps"], float(np.abs(mi - ri).max()))
    return e


def sensitivity(cases, names):
    """{grid id: {mutation: {protocol: {quantity: effect}}}} for the given cases and mutation names."""
    tmp = tempfile.mkdtemp(prefix="sens_")
    try:
        libs = build_mutants(names, tmp)
        jobs = [(c, p, n) for c in cases for p in ("energetic", "quiet") for n in ["original"] + list(names)]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:       # the ctypes calls release the GIL
            res = dict(zip([(FS.grid_id(c), p, n) for c, p, n in jobs], ex.map(lambda t: run_protocol(libs[t[2]], t[0], t[1]), jobs)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {FS.grid_id(c): {n: {p: effect(res[FS.grid_id(c), p, "original"], res[FS.grid_id(c), p, n]) for p in ("energetic", "quiet")}
                            for n in names} for c in cases}


def main():
    data = {"protocols": {"energetic": "flow_states.energetic_state per replica, %d timesteps" % FS.NDT,
                          "quiet": "jit._seeded_rayleigh_state / reset(), %d timesteps" % QUIET_NDT},
            "mutations": {n: m[0] for n, m in MUTATIONS.items()},
            "effects": sensitivity(FS.grids(), list(MUTATIONS))}
    with open(OUT, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for g, muts in data["effects"].items():
        for n, e in muts.items():
            print("%-18s %-18s energetic u %.1e v %.1e S %.1e obs %.1e sweeps %3d | quiet u %.1e v %.1e S %.1e obs %.1e sweeps %3d"
                  % (g, n, *[e["energetic"][k] for k in ("u", "v", "S", "obs", "sweeps")], *[e["quiet"][k] for k in ("u", "v", "S", "obs", "sweeps")]))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

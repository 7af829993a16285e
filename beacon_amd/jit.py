"""Register-resident kernels for grids that are not built into libbeacon_hip.so.

The reference takes any domain size (rayleigh.py:20-27: nx = 50 L, ny = 50 H; mixing.py:20-28: nx = 100 L, ny = 100 H);
the register-resident kernels are templates over the grid (csrc/ns2d_fast_impl.h: one row per lane, ny <= 64;
csrc/ns2d_fast2_impl.h: two rows per lane, 64 < ny <= 128; csrc/ns2d_fast4_impl.h: 128 < ny <= 256, the Poisson solve
in registers with 2..4 rows per lane and the other phases from HBM/L2).  libbeacon_hip.so carries the metric grid and the
reference's defaults; for any other grid `plugin_for()` compiles csrc/jit/ns2d_jit.hip for that ONE grid with hipcc
(about 30 s, once: the shared object is cached in beacon_amd/_jit/, keyed by a hash of its sources and flags, and
travels with the tree like the library itself) and hands its launcher to the library through bcn_set_fast_plugin.
No hipcc, BEACON_JIT=0 or a grid the mapping cannot hold (ny > 256, LDS, registers) -> None: the env keeps the
generic kernel (still on the GPU; only slower).

First-use self-check.  A plugin is a NEW template instantiation compiled on the user's box, at the register limit of the
target (256 VGPRs plus spills), and round 4 met one such instantiation that computed wrong results under a neutral source
change (the 110x64 float64 two-body kernel).  So no plugin is attached on trust: the first env that wants it runs
`verify()` -- six timesteps of a seeded state through the plugin (plain launch and ticket scheduler) and through the generic
kernel, which is ordinary HIP without hand-scheduled code: float64 fields within 1e-9 with equal sweep counts (+-1), float32
within the on-demand grids' tolerance.  Agreement is remembered next to the shared object (`<plugin>.ok`, tagged with the device
and the HIP runtime, so another box checks again); a mismatch leaves `<plugin>.bad`, warns, and the env -- this one and every
later one -- keeps the generic kernel.

Per-replica parameters (VecEnv.set_params) on a plugin grid.  The kernels that read the parameter table are a second shared
object of the same grid, built with PRM_DEFS (-DBCN_JIT_PRM=1: csrc/ns2d_prm.h) -- the plain plugin keeps the code it has.  It is
built, checked and attached only when an env asks for it (_VecNS2D.set_params_kernel("fast")); its verify() is the same comparison
with a table of three distinct parameter sets on both envs (SELF_CHECK_PARAMS), so that the generic kernel reads the table and so
does the plugin; its `.ok` / `.bad` markers are its own."""
import ctypes as C
import fcntl
import os
import subprocess
import warnings

from . import build as _build

class JitWarning(UserWarning):
    """Every warning of this module: a plugin that could not be built / loaded / checked, or that failed its self-check.
    tests/conftest.py turns the category into an error, so a refused plugin is a red test, not a line in a log."""


JIT_DIR = os.path.join(_build.PKG, "_jit")
JIT_SRC = os.path.join(_build.CSRC, "jit", "ns2d_jit.hip")
_LOADED = {}


def _library():
    """libbeacon_hip.so with its two internal queries declared (csrc/ns2d_geom.h: no part of the ABI of include/beacon_hip.h)."""
    from . import _lib
    L = _lib.load()
    if L.bcn_jit_geometry.argtypes is None:
        L.bcn_jit_geometry.restype = C.c_int
        L.bcn_jit_geometry.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong)]
        L.bcn_jit_builtin.restype = C.c_int
        L.bcn_jit_builtin.argtypes = [C.c_int, C.POINTER(C.c_int)]
    return L


def geometry(rows, nx, ny, r, g, f64):
    """What csrc/ns2d_geom.h says about strips of `r` columns of an nx x ny grid in kernel family `rows` (1, 2, 4; g: gf, or rpl for
    the hybrid): None where the family cannot hold the mapping (its shape, or more LDS than a workgroup has), else dict(nw, rl,
    threads, lds, scratch) -- waves, columns of the last one, threads, LDS bytes of a launch, elements of global field scratch.  The
    library computes it, from the header its kernels are built from and with its compiled prefetch depths."""
    out = (C.c_longlong * 5)()
    if not _library().bcn_jit_geometry(rows, nx, ny, r, g, int(bool(f64)), out):
        return None
    return dict(zip(("nw", "rl", "threads", "lds", "scratch"), (int(v) for v in out)))


def builtin_rows():
    """The register-resident instantiations built into libbeacon_hip.so (csrc/ns2d_builtin.h), as the library enumerates them:
    [dict(f64, nx, ny, kind, rows, R, gf)]."""
    L, out, rows = _library(), (C.c_int * 7)(), []
    while L.bcn_jit_builtin(len(rows), out):
        rows.append(dict(zip(("f64", "nx", "ny", "kind", "rows", "R", "gf"), [bool(out[0])] + [int(v) for v in out[1:]])))
    return rows


def builtin_grids():
    """jit.BUILTIN_GRIDS: the grids of libbeacon_hip.so's own register-resident kernels as {(nx, ny, f64, kind)} -- no plugin is built
    for them.  Derived from builtin_rows() at its first use (importing this module loads no library)."""
    if "BUILTIN_GRIDS" not in globals():
        globals()["BUILTIN_GRIDS"] = frozenset((b["nx"], b["ny"], b["f64"], b["kind"]) for b in builtin_rows())
    return globals()["BUILTIN_GRIDS"]


def __getattr__(name):
    if name == "BUILTIN_GRIDS":
        return builtin_grids()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _choose4(nx, ny, f64):
    """ns2d_fast4_impl.h: only the Poisson solve lives in registers (rpl = ceil(ny / 64) rows per lane, strips of r columns); 16
    waves of 128 VGPRs where phi and the rhs of a strip fit them, else 8 waves of 256; the fields stay in HBM/L2."""
    if ny > 256:
        return None
    rpl = -(-ny // 64)
    for nwmax, words in ((16, 28), (8, 60)):
        if f64 and nwmax > 8:
            continue
        r = -(-nx // nwmax)
        if r * rpl * (2 if f64 else 1) > words:
            continue
        g = geometry(4, nx, ny, r, rpl, f64)
        if g is not None:
            return {"rows": 4, "R": r, "gf": 0, "nw": g["nw"], "rpl": rpl}
    return None


def choose(nx, ny, f64, kind):
    """Mapping of an nx x ny grid onto one workgroup: dict(rows, R, gf) or None.  Waves: 8 (two per SIMD, 256 VGPRs
    each) where the strips fit the register file, else 12 or 16; the last wave may take fewer columns (>= 3).
    Everything in registers / LDS where that fits (rows 1: ny <= 64, rayleigh; rows 2: ny <= 128), else the hybrid of
    ns2d_fast4_impl.h (rows 4: tall grids, wide grids, mixing below ny = 64).
    This is the policy -- which wave counts to try, in which order, up to which strip width, and what float64 is refused; whether
    a family can hold a candidate (strips, LDS) is geometry()'s answer: csrc/ns2d_geom.h, not restated here."""
    if nx < 6 or ny < 4:
        return None
    if ny <= 64 and kind == 0:      # ns2d_fast_impl.h (one row per lane) implements the rayleigh boundary conditions only
        for nw, rmax in ((8, 16 if f64 else 26), (12, 18), (16, 12), (10, 20), (6, 26), (5, 26), (4, 26), (3, 26), (2, 26)):
            if f64 and nw > 8:
                continue
            r = -(-nx // nw)
            if r > rmax:
                continue
            # float64: at most 16 columns per lane.  Strips of unequal width: round 4's two-body float64 kernel of 110x64 (strips of
            # 14 and 12 columns, two instantiations of the body in one kernel) computed ONE wrong word per timestep under a neutral
            # source change -- lane 0 of the column where the two bodies meet.  Since round 6 the float64 kernel with
            # T in the global scratch (gf = 2) has ONE body: the last strip is as wide as the others, its surplus columns dead
            # (ns2d_fast_impl.h: DEADC); the all-global variant (gf = 1) keeps equal strips only.  Every plugin, of whatever family,
            # is compared with the generic kernel before its first use (verify()).
            if f64 and r > 16:
                continue
            # float64 on fewer than 8 waves: refused.  The 6-wave one-body kernels with strips of 9 columns (50x64: 5 x 9 + 5
            # live; 51x60: 5 x 9 + 6) disagree with the generic kernel and the oracle by O(1) in T, the ticket scheduler worse
            # than the plain launch (tests/test_gpu_parity.py::test_jit_kernels_vs_oracle, its 50x64 case); the cause is not
            # found, so these grids take the hybrid (rows 4) instead.  6-wave strips of 10 and 11 columns measured exact.
            if f64 and nw != 8:
                continue
            for gf in ((2, 1) if f64 else (0,)):
                g = geometry(1, nx, ny, r, gf, f64)
                # (strips of r columns that make fewer waves than the candidate: another candidate's mapping)
                if g is None or g["nw"] != nw or (gf == 1 and g["rl"] != r):
                    continue
                return {"rows": 1, "R": r, "gf": gf, "nw": nw}
    elif 64 < ny <= 128:
        # float64: the fields live in a global scratch, the Poisson rhs in LDS (gf = 1); rayleigh and mixing alike
        for nw, rmax in (((8, 13), (7, 13), (6, 13), (5, 13), (4, 13)) if f64 else ((8, 16), (12, 10), (16, 7), (7, 16), (6, 20), (5, 24), (4, 26))):
            r = -(-nx // nw)
            if r > rmax:
                continue
            g = geometry(2, nx, ny, r, 1 if f64 else 0, f64)
            if g is not None and g["nw"] == nw:
                return {"rows": 2, "R": r, "gf": 1 if f64 else 0, "nw": nw}
    return _choose4(nx, ny, f64)


CHECKING = False      # inside verify(): the envs it builds attach the plugin without verifying it again


def _runtime_tag():
    import torch
    try:
        name = torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName
    except Exception:      # noqa: BLE001
        name = "?"
    return "%s hip %s" % (name, getattr(torch.version, "hip", None))


def _seeded_rayleigh_state(env):
    import numpy as np
    x, y = (np.arange(env.nx + 2) - 0.5) / env.nx, (np.arange(env.ny + 2) - 0.5) / env.ny
    st0 = np.zeros((4, env.nx + 2, env.ny + 2))
    st0[3] = (0.5 - y)[None, :] + 0.08 * np.sin(2 * np.pi * x * env.L)[:, None] * np.sin(np.pi * y)[None, :]
    return np.tile(np.ascontiguousarray(st0.transpose(0, 2, 1))[None], (env.batch, 1, 1, 1))


SELF_CHECK_F64 = dict(u=1e-9, v=1e-9, p=5e-8, S=1e-9)
# float32: 10 x the largest plugin-vs-generic difference over every float32 case of test_jit_kernels_vs_oracle (12 timesteps,
# 4 replicas; m: u 4.8e-7, v 5.4e-7, p 5.8e-5, T/C 7.7e-7).  Before: 2e-4 for u, v, T/C and 1e-2 for p.
SELF_CHECK_F32 = dict(u=4.8e-6, v=5.4e-6, p=5.8e-4, S=7.7e-6)


# extra -D flags of a plugin's table-reading twin, and the table its self-check runs with (one set per replica of the batch of 3)
PRM_DEFS = {"BCN_JIT_PRM": 1}
SELF_CHECK_PARAMS = {0: dict(ra=(8.0e3, 5.0e4, 2.0e5)), 1: dict(re=(100.0, 200.0, 400.0), pe=(1.0e4, 1.0e5, 2.0e3))}


def compare_with_generic(make_env, kind, f64, ndt=6, batch=3, stats=None, params=False):
    """(ok, report): `ndt` timesteps of a seeded state through the attached register-resident kernel -- plain launch and
    ticket scheduler (chunks of two timesteps on two persistent workgroups: hand-offs through HBM) -- against the generic
    kernel.  float64: fields within 1e-9 (p 5e-8), sweep counts within 1; float32: per field,
    SELF_CHECK_F32 (u 4.8e-6, v 5.4e-6, T/C 7.7e-6, p 5.8e-4: 10 x the largest plugin-vs-generic differences measured over every
    float32 case of tests/test_gpu_parity.py::test_jit_kernels_vs_oracle), counts within max(3, 2 %).  `stats`: a dict, filled
    with the per-field differences and the sweep counts of each run.  `params`: every env carries the per-replica table
    SELF_CHECK_PARAMS and the register-resident runs select the table-reading kernels (set_params_kernel("fast")): the check of a
    parameter plugin, which also requires that those kernels, not the generic one, took the steps."""
    import numpy as np
    import torch
    runs = {}
    for tag, variant, sched in (("generic", 0, None), ("plain", 1, (0, 0, 0)), ("ticket", 1, (2, 2, 2))):
        env = make_env(batch)
        try:
            env.set_ndt_act(ndt)
            got = env.set_variant(variant)
            if sched is not None:
                env.set_sched(*sched)
            if params:
                if variant == 1:
                    env.set_params_kernel("fast")
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")      # (ParamsWarning of an env left on the generic kernel: reported as a mismatch below)
                    env.set_params(**{k: np.resize(np.asarray(v), batch) for k, v in SELF_CHECK_PARAMS[kind].items()})
            env.reset()
            if kind == 0:
                env.set_state(_seeded_rayleigh_state(env))
                a = np.random.default_rng(3).uniform(-1, 1, (batch, env.n_sgts))
            else:
                a = np.array([0, 2, 3] * batch)[:batch]
            env.step(a)
            torch.cuda.synchronize(env.device)
            runs[tag] = (env.get_state().double().cpu().numpy(), env.sweeps.cpu().numpy().astype(np.int64),
                         env.status.cpu().numpy().copy(), env.kernel_name, got)
        finally:
            env.close()
    ref = runs["generic"]
    tol = SELF_CHECK_F64 if f64 else SELF_CHECK_F32
    rep, ok = [], True
    for tag in ("plain", "ticket"):
        st, sw, status, kname, got = runs[tag]
        d = np.abs(st - ref[0])
        d = np.where(np.isfinite(d), d, np.inf)
        dm = {F: float(d[:, i].max()) for i, F in enumerate("uvpS")}
        ds = int(np.abs(sw - ref[1]).max())
        if stats is not None:
            stats[tag] = dict(dm, sweeps=ds, sweeps_max=int(ref[1].max()))
        good = (got == 1 and (not params or kname.startswith("ns2d_fast")) and not status.any() and not ref[2].any() and all(dm[F] <= tol[F] for F in "uvpS") and
                ds <= (1 if f64 else max(3, int(0.02 * ref[1].max()))))
        ok = ok and good
        rep.append("%s (%s): u %.2e v %.2e p %.2e T/C %.2e sweeps %d of %d status %s%s"
                   % (tag, kname, dm["u"], dm["v"], dm["p"], dm["S"], ds, int(ref[1].max()), np.unique(status).tolist(),
                      "" if good else "  <-- MISMATCH"))
    return ok, "; ".join(rep)


def _read(path):
    try:
        with open(path) as fh:
            return fh.read()
    except OSError:
        return None


def _verdict_on_disk(p, tag):
    """True / False from the marker files beside the shared object, None where there is none for this device + runtime.  Both
    markers start with the runtime tag; one written on another device or HIP runtime is ignored (the plugin is checked again)."""
    bad = _read(p.path + ".bad")
    if bad is not None and bad.split("\n")[0].strip() == tag:
        return False, bad.strip()[:300]
    ok = _read(p.path + ".ok")
    if ok is not None and ok.split("\n")[0].strip() == tag:
        return True, ok
    return None, ""


def verify(p, make_env, kind, f64, params=False):
    """Sets p.verified (True / False) -- from the marker files next to the shared object, or by running compare_with_generic()
    (params: with a per-replica parameter table, for a plugin built with PRM_DEFS).
    One process per plugin runs the comparison: the N ranks of a fresh node queue on `<plugin>.vlock` and all but the first find
    the first one's verdict on disk when the lock comes to them."""
    global CHECKING
    tag = _runtime_tag()

    def settle(v, text):
        p.verified = v
        if not v:
            warnings.warn("beacon_amd.jit: %s failed its self-check earlier (%s); the generic kernel stays selected"
                          % (os.path.basename(p.path), text), JitWarning)

    v, text = _verdict_on_disk(p, tag)
    if v is not None:
        return settle(v, text)
    lock = None
    try:
        lock = open(p.path + ".vlock", "w")
        fcntl.flock(lock, fcntl.LOCK_EX)
    except OSError:
        lock = None                 # read-only package directory: every process checks for itself
    try:
        v, text = _verdict_on_disk(p, tag)       # written by another rank while this one waited
        if v is not None:
            return settle(v, text)
        CHECKING = True
        try:
            ok, rep = compare_with_generic(make_env, kind, f64, params=params)
        except Exception as e:      # noqa: BLE001 -- could not run (out of memory, ...): no verdict, no plugin for this env
            warnings.warn("beacon_amd.jit: the self-check of %s could not run (%s: %s); the generic kernel stays selected for this env"
                          % (os.path.basename(p.path), type(e).__name__, e), JitWarning)
            return
        finally:
            CHECKING = False
        p.verified, p.report = bool(ok), rep
        try:
            with open(p.path + (".ok" if ok else ".bad"), "w") as fh:
                fh.write("%s\n%s\n" % (tag, rep))
            try:
                os.remove(p.path + (".bad" if ok else ".ok"))     # the other verdict, from another device or runtime
            except FileNotFoundError:
                pass
            if lock is not None:
                os.remove(p.path + ".vlock")      # the verdict is on disk: a rank still queued on the lock finds it there
        except OSError:
            pass                    # read-only package directory: the verdict holds for this process
    finally:
        if lock is not None:
            fcntl.flock(lock, fcntl.LOCK_UN)
            lock.close()
    if not ok:
        warnings.warn("beacon_amd.jit: the register-resident kernel %s DISAGREES with the generic kernel on its self-check (%s); "
                      "it is not used: the generic kernel stays selected" % (os.path.basename(p.path), rep), JitWarning)


def selftest(device="cuda:0", verbose=False):
    """The register-resident kernels BUILT INTO libbeacon_hip.so through the comparison that guards a plugin's first use
    (compare_with_generic: six timesteps of a seeded state, plain launch and ticket scheduler, against the generic kernel).
    What to run after rebuilding the library with another ROCm / hipcc: these kernels sit at the register limit of the target
    and their code generation is the compiler's.  Returns {name: (ok, report)}."""
    from . import vec as V
    out = {}
    for name, kind, kw, dt in selftest_cases():
        if kind == 0:
            mk = lambda B, dt=dt, kw=kw: V.VecRayleigh(B, device, dt, None, **kw)
        else:
            mk = lambda B, dt=dt, kw=kw: V.VecMixing(B, device, dt, **kw)
        ok, rep = compare_with_generic(mk, kind, dt == "f64")
        out["%s %s" % (name, dt)] = (ok, rep)
        if verbose:
            print("%-24s %s  %s" % (name + " " + dt, "ok " if ok else "BAD", rep), flush=True)
    return out


def selftest_cases():
    """selftest()'s cases, one per row of builtin_rows(): (name, kind, domain lengths of the env's constructor, "f32" | "f64")."""
    return [("%s %dx%d" % (("rayleigh", "mixing")[b["kind"]], b["nx"], b["ny"]), b["kind"],
             dict(L=_extent(b["nx"], (50.0, 100.0)[b["kind"]]), H=_extent(b["ny"], (50.0, 100.0)[b["kind"]])), "f64" if b["f64"] else "f32")
            for b in builtin_rows()]


def _unit(defs):
    """The build.Unit of the plugin with these -D flags: one hipcc command, named by its hash instead of carrying a .sig."""
    def commands(cc, tmp, objdir):
        return [], _build.compile_cmd(JIT_SRC, tmp, _build.JIT_FLAGS, defs, mode=("-shared",), cc=cc)
    return _build.Unit(None, lambda: [JIT_SRC], lambda: (_build.ARCH, _build.FLAGS, _build.JIT_FLAGS, sorted(defs.items())), commands, sig=False)


def build_plugin(nx, ny, f64, kind, verbose=False, extra_defs=None):
    """Path of the shared object for this grid (compiling it if needed), or None.  extra_defs: more -D flags (part of the
    plugin's name hash), e.g. {"BCN_JIT_BREAK": 1} -- the deliberately wrong kernel of the self-check's own test."""
    m = choose(nx, ny, f64, kind)
    if m is None or os.environ.get("BEACON_JIT", "1") == "0":
        return None
    defs = {"BCN_JIT_ROWS": m["rows"], "BCN_JIT_REAL": "double" if f64 else "float", "BCN_JIT_NX": nx, "BCN_JIT_NY": ny,
            "BCN_JIT_R": m["R"], "BCN_JIT_KIND": kind, "BCN_JIT_GF": m["gf"]}
    if m["rows"] == 4:
        defs["BCN_JIT_RPL"] = m["rpl"]
    for d in os.environ.get("BEACON_JIT_DEFS", "").split():   # experiments: extra -D flags (scripts/tall_base.py)
        defs[d.partition("=")[0]] = d.partition("=")[2] or "1"
    defs.update(extra_defs or {})
    u = _unit(defs)
    u.lib = os.path.join(JIT_DIR, "ns2d_%dx%d_%s_k%d_r%d_%s.so" % (nx, ny, "f64" if f64 else "f32", kind, m["R"], u.signature()[:12]))
    if not u.stale():
        return u.lib
    if u.compiler() is None or _build.no_build():
        return None
    try:
        return u.build(verbose=verbose)               # (one lock per plugin: N ranks of one node asking for the same grid)
    except (OSError, subprocess.CalledProcessError) as e:
        # a read-only package directory, a full disk or a compiler error: the env keeps the generic kernel
        # (still on the GPU, only slower) instead of failing in its constructor
        warnings.warn("beacon_amd.jit: no register-resident kernel for %dx%d (%s); the generic kernel stays selected"
                      % (nx, ny, e), JitWarning)
        return None


class Plugin(object):
    def __init__(self, path):
        self.path = path
        self.lib = C.CDLL(path)                       # bcn_set_error resolves against libbeacon_hip.so (RTLD_GLOBAL)
        self.lib.bcn_jit_scratch_elems.restype = C.c_size_t
        self.lib.bcn_jit_lds_bytes.restype = C.c_size_t
        self.fn = C.cast(self.lib.bcn_jit_launch, C.c_void_p)
        # a plugin built with PRM_DEFS: the launcher of its table-reading kernels (bcn_set_fast_plugin_params)
        self.fn_prm = C.cast(self.lib.bcn_jit_launch_prm, C.c_void_p) if hasattr(self.lib, "bcn_jit_launch_prm") else None
        self.scratch = int(self.lib.bcn_jit_scratch_elems())
        self.lds = int(self.lib.bcn_jit_lds_bytes())
        self.verified = None          # True / False once verify() has compared it with the generic kernel
        self.report = ""


def plugin_for(nx, ny, f64, kind, extra_defs=None):
    """Loaded plugin (kept alive for the life of the process) for this grid, or None."""
    key = (nx, ny, bool(f64), kind, tuple(sorted((extra_defs or {}).items())))
    if key not in _LOADED:
        path = build_plugin(nx, ny, f64, kind, extra_defs=extra_defs)
        try:
            p = Plugin(path) if path else None
        except (OSError, AttributeError) as e:        # a truncated or foreign shared object in the cache
            warnings.warn("beacon_amd.jit: cannot load %s (%s); the generic kernel stays selected" % (path, e), JitWarning)
            p = None
        if p is not None and not os.environ.get("BEACON_JIT_DEFS"):     # (experiments may change the depth: the plugin's own figures rule)
            m = choose(nx, ny, f64, kind)
            g = geometry(m["rows"], nx, ny, m["R"], m["rpl"] if m["rows"] == 4 else m["gf"], f64)
            if g is None or (p.lds, p.scratch) != (g["lds"], g["scratch"]):
                warnings.warn("beacon_amd.jit: %s reports %d bytes of LDS and %d elements of field scratch, the library's geometry of its "
                              "mapping says %s; the generic kernel stays selected"
                              % (os.path.basename(p.path), p.lds, p.scratch, g and "%d and %d" % (g["lds"], g["scratch"])), JitWarning)
                p = None
        _LOADED[key] = p
    return _LOADED[key]


# grids of the -m gpu tests (tests/test_gpu_parity.py::test_jit_grids_*): built by __graft_entry__.build() so that
# they ship with the tree; any other grid compiles at its first use
TEST_GRIDS = [(75, 50, False, 0), (75, 50, True, 0), (53, 50, False, 0), (110, 64, False, 0), (110, 64, True, 0),
              (50, 70, False, 0), (60, 120, False, 0), (100, 110, False, 1), (150, 50, True, 0), (110, 65, False, 0),
              (100, 105, False, 1), (50, 70, True, 0), (50, 150, False, 0), (50, 150, True, 0), (64, 200, False, 0),
              (100, 200, False, 1), (50, 145, False, 0), (50, 149, True, 0), (100, 130, False, 1),
              (300, 50, False, 0), (200, 100, False, 1), (53, 150, False, 0), (106, 200, False, 1),
              # float64, two rows per lane, ODD ny, strips of unequal width (9 / 5, 10 / 7): the class of the wrong kernel of round 5
              (50, 75, True, 0), (57, 107, True, 0), (100, 105, True, 1), (50, 75, False, 0),
              # float64, one row per lane, ONE body with dead columns in the last strip (round 6): 7 x 7 + 3 live, 7 x 16 + 13 live
              (52, 50, True, 0), (125, 55, True, 0)]


def fuzz_grids(seed=5):
    """22 random domain sizes with a register-resident mapping, as (L, H, f64, kind): the reference takes any L, H
    (rayleigh.py:20-27, mixing.py:20-28).  Drawn until every kernel family has its quota -- (rows per lane, float64):
    one row 4 + 3, two rows 4 + 3, the hybrid 6 + 2.  Seeded, so that __graft_entry__.build() compiles exactly the plugins
    that tests/test_gpu_parity.py::test_jit_fuzzed_grids_agree_with_the_generic_kernel asks for."""
    import numpy as np
    rng = np.random.default_rng(seed)
    quota = {(1, False): 4, (1, True): 3, (2, False): 4, (2, True): 3, (4, False): 6, (4, True): 2}
    out = []
    while any(quota.values()):
        kind = int(rng.integers(0, 2))
        f64 = bool(rng.integers(0, 2))
        if kind == 0:        # (below L, H = 1 the reference divides by zero: nx_obs_pts = 4 int(L))
            L = round(float(rng.uniform(1.0, 4.5)), 2)
            H = round(float(rng.uniform(1.0, 1.3) if rng.integers(0, 2) else rng.uniform(1.0, 3.2)), 2)
            nx, ny = int(50 * L), int(50 * H)
        else:
            L, H = round(float(rng.uniform(1.0, 1.7)), 2), round(float(rng.uniform(1.0, 2.3)), 2)
            nx, ny = int(100 * L), int(100 * H)
        m = choose(nx, ny, f64, kind)
        if m is None or nx * ny > 30000 or not quota.get((m["rows"], f64)):
            continue
        quota[(m["rows"], f64)] -= 1
        out.append((L, H, f64, kind))
    return out


def _grid(L, H, kind):
    n = 50 if kind == 0 else 100
    return int(n * L), int(n * H)


def fuzz_cases(seed=6):
    """fuzz_grids() (default constructor arguments) plus 15 draws that cover what those 22 never met (the
    wrong 50x75 float64 kernel was the only float64 two-rows-per-lane grid with ODD ny anyone had built, and it ran with
    n_sgts = 5, ra = 5e4): per kernel family and precision -- (rows per lane, float64) -- an odd-ny quota (one row 2 + 2, two rows
    rayleigh 2 + 2 and mixing 2 + 1, the hybrid 1 + 1 each), every case with the reference's OTHER constructor arguments drawn as well: rayleigh n_sgts in 1..12
    and ra in [8e3, 2e5] (rayleigh.py:20-27), mixing re in [50, 400], pe in [1e3, 1e5], side in [0.3, 0.7], C0 in [0.5, 2]
    (mixing.py:20-34).  Returns (L, H, f64, kind, kwargs)."""
    import numpy as np
    out = [(L, H, f64, kind, {}) for L, H, f64, kind in fuzz_grids()]
    rng = np.random.default_rng(seed)
    quota = {(1, False, 0): 2, (1, True, 0): 2, (2, False, 0): 2, (2, True, 0): 2, (2, False, 1): 2, (2, True, 1): 1,
             (4, False, 0): 1, (4, True, 0): 1, (4, False, 1): 1, (4, True, 1): 1}
    while any(quota.values()):
        kind = int(rng.integers(0, 2))
        f64 = bool(rng.integers(0, 2))
        if kind == 0:
            L = round(float(rng.uniform(1.0, 4.5)), 2)
            H = round(float(rng.uniform(1.0, 1.3) if rng.integers(0, 2) else rng.uniform(1.0, 3.2)), 2)
            kw = dict(n_sgts=int(rng.integers(1, 13)), ra=float(round(10.0 ** rng.uniform(np.log10(8e3), np.log10(2e5)), -2)))
        else:
            L, H = round(float(rng.uniform(1.0, 1.7)), 2), round(float(rng.uniform(1.0, 2.3)), 2)
            kw = dict(re=float(round(rng.uniform(50, 400), 0)), pe=float(round(10.0 ** rng.uniform(3, 5), -1)),
                      side=round(float(rng.uniform(0.3, 0.7)), 2), C0=round(float(rng.uniform(0.5, 2.0)), 2))
        nx, ny = _grid(L, H, kind)
        m = choose(nx, ny, f64, kind)
        if m is None or ny % 2 == 0 or nx * ny > 30000 or not quota.get((m["rows"], f64, kind)):
            continue
        quota[(m["rows"], f64, kind)] -= 1
        out.append((L, H, f64, kind, kw))
    return out


# the grids where choose() switches family, and the narrowest last strips, as (nx, ny, f64, kind, with other constructor
# arguments).  The family a grid maps to is in the comment (rows per lane: 1 / 2 / 4 = hybrid; "3 live": last strip of 3 columns)
BOUNDARY_GRIDS = [
    # rayleigh: ny = 64 / 65, one row per lane <-> two rows (51x65: strips of 8, the last one 3 live)
    # (50x64 float64 took the 6-wave one-row kernel, which was wrong: choose() now maps it to the hybrid; 120x64: 8 x 15)
    (50, 64, False, 0, False), (50, 64, True, 0, True), (120, 64, True, 0, False), (51, 65, False, 0, True),
    (51, 65, True, 0, False),
    # ny = 128 / 129, two rows <-> hybrid (52x129 float64: hybrid, 3 live)
    (50, 128, False, 0, False), (50, 128, True, 0, True), (50, 129, False, 0, True), (52, 129, True, 0, False),
    # ny = 255 / 256: the hybrid with 4 rows per lane, the tallest grid admitted
    (50, 255, False, 0, False), (50, 256, False, 0, True),
    # the width limit of the one-row family: float32 nx 152 -> 153 at ny = 64 and 206 -> 207 at ny = 50 (153x64: hybrid, 3 live)
    (152, 64, False, 0, True), (153, 64, False, 0, False), (206, 50, False, 0, False), (207, 50, False, 0, True),
    # float64: nx 128 -> 129 (one row, 8 strips of 16 <-> hybrid)
    (128, 50, True, 0, False), (129, 50, True, 0, True), (129, 64, True, 0, False),
    # last strips of 3 live columns: one row per lane (52x50: 7 x 7 + 3) and the hybrid (213x50: 15 x 14 + 3)
    (52, 50, False, 0, True), (213, 50, False, 0, False),
    # mixing 100x128: hybrid in float32, two rows in float64; ny = 129 / 255 / 256 on the hybrid
    (100, 128, False, 1, True), (100, 128, True, 1, False), (100, 129, False, 1, False), (100, 255, False, 1, True),
    (100, 256, False, 1, False),
    # mixing float32 hybrid, 16 strips of 8 columns, the last one 3 live
    (123, 100, False, 1, True),
    # mixing float64 even ny: two rows only for nx 100..104 (104x110, 104x100), the hybrid for nx 105..120 (105x100, 120x128); odd ny:
    # two rows 102x101, hybrid 110x101 (each class at least twice with fuzz_cases())
    (104, 110, True, 1, True), (104, 100, True, 1, False), (105, 100, True, 1, False), (120, 128, True, 1, True),
    (102, 101, True, 1, False),
    (110, 101, True, 1, True),
]


def _extent(c, n):
    """A domain length whose grid is exactly c cells of 1 / n (int(n L) == c)."""
    return c / n if int(n * (c / n)) == c else (c + 0.5) / n


def oracle_cases(seed=7):
    """fuzz_cases() followed by BOUNDARY_GRIDS, as (L, H, f64, kind, kwargs): the list tests/test_gpu_parity.py::
    test_jit_kernels_vs_oracle runs through the plugin and the generic kernel against the float64 oracle.  The boundary grids
    marked for it draw the reference's other constructor arguments from the ranges of fuzz_cases() (seeded)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = list(fuzz_cases())
    for nx, ny, f64, kind, args in BOUNDARY_GRIDS:
        if (nx, ny, f64, kind) in builtin_grids():
            continue
        n = 50.0 if kind == 0 else 100.0
        kw = {}
        if args and kind == 0:
            kw = dict(n_sgts=int(rng.integers(1, 13)), ra=float(round(10.0 ** rng.uniform(np.log10(8e3), np.log10(2e5)), -2)))
        elif args:
            kw = dict(re=float(round(rng.uniform(50, 400), 0)), pe=float(round(10.0 ** rng.uniform(3, 5), -1)),
                      side=round(float(rng.uniform(0.3, 0.7)), 2), C0=round(float(rng.uniform(0.5, 2.0)), 2))
        out.append((_extent(nx, n), _extent(ny, n), f64, kind, kw))
    return out


def oracle_grid_keys():
    return [_grid(L, H, kind) + (f64, kind) for L, H, f64, kind, _ in oracle_cases()]


def fuzz_grid_keys():
    return [_grid(L, H, kind) + (f64, kind) for L, H, f64, kind, _ in fuzz_cases()]


# plugins built with extra -D flags: the deliberately wrong kernels of the self-check's own tests (dt x 1.5; float32 two rows
# per lane with dt x (1 + eps): a subtle error, under the old float32 bound of the self-check but over the per-field one)
BREAK2_GRID = (60, 80, False, 0)
BREAK2_DEFS = {"BCN_JIT_BREAK": 2, "BCN_JIT_BREAK_EPS": "3e-4"}
# the parameter plugins (PRM_DEFS) of the grids tests/test_gpu_params_fast.py uses: one per kernel family -- rows 1; rows 2 float64
# (global scratch); rows 2 mixing; rows 4 -- and the deliberately wrong one of the self-check's test
PRM_TEST_GRIDS = [(75, 50, False, 0), (50, 75, True, 0), (100, 110, False, 1), (50, 150, False, 0)]
PRM_BREAK_GRID = (75, 50, True, 0)
# The float32 one-row-per-lane strip widths whose Jacobi cells are stated in runs (csrc/bcn_jacobi_cells.h: jacobi_runs_fit), one
# on-demand rayleigh grid per width R and, among them, every last-strip width 8..11 -- a second body that takes the runs because R
# does -- and the 3-column last strip.  Each is built twice: the default plugin and its cell-by-cell twin (RUNS_TWIN_DEFS), which
# tests/test_gpu_jacobi_cells.py holds to each other bit for bit.  (nx, ny, f64, kind); R / last strip in the comments.  Kept out of
# TEST_GRIDS: the test_jit_grids_* tests need not run them.
RUNS_GRIDS = [(52, 50, False, 0),       # 7 / 3
              (56, 64, False, 0),       # 7 / 7, ny = 64
              (90, 50, False, 0),       # 12 / 6
              (104, 64, False, 0),      # 13 / 13, ny = 64
              (105, 50, False, 0),      # 14 / 7
              (113, 50, False, 0),      # 15 / 8
              (121, 50, False, 0),      # 16 / 9
              (129, 64, False, 0),      # 17 / 10, ny = 64
              (137, 50, False, 0),      # 18 / 11
              (152, 50, False, 0),      # 19 / 19
              (153, 50, False, 0),      # 20 / 13
              (168, 50, False, 0),      # 21 / 21
              (169, 50, False, 0),      # 22 / 15
              (184, 50, False, 0),      # 23 / 23
              (185, 50, False, 0),      # 24 / 17
              (195, 50, False, 0),      # 25 / 20
              (201, 50, False, 0)]      # 26 / 19
RUNS_TWIN_DEFS = {"BCN_JACOBI_RUNS": 0}
# the two ends of the band of widths that stay cell by cell (R - 4 in 4..7): R = 8 and R = 11, default plugins only
RUNS_EXCLUDED_GRIDS = [(60, 53, False, 0), (88, 50, False, 0)]
EXTRA_BUILDS = ([((75, 50, True, 0), {"BCN_JIT_BREAK": 1}), (BREAK2_GRID, BREAK2_DEFS)] + [(g, dict(PRM_DEFS)) for g in PRM_TEST_GRIDS] +
                [(PRM_BREAK_GRID, dict(PRM_DEFS, BCN_JIT_BREAK=1))] + [(g, dict(RUNS_TWIN_DEFS)) for g in RUNS_GRIDS])


def runs_default_grids():
    """RUNS_GRIDS and RUNS_EXCLUDED_GRIDS without those whose default plugin another list builds already."""
    other = set(TEST_GRIDS) | set(oracle_grid_keys())
    return [g for g in RUNS_GRIDS + RUNS_EXCLUDED_GRIDS if g not in other]


def _bounds_job(cell):
    from . import stoprule
    try:
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=2):
            stoprule.bounds(*cell)
    except ImportError:
        stoprule.bounds(*cell)


def prebuild(grids=None, verbose=False):
    """Compile the plugins of a list of (nx, ny, f64, kind) grids (used by __graft_entry__.build() for the grids the
    tests touch, so that they ship with the tree)."""
    from concurrent.futures import ThreadPoolExecutor
    todo = [(g, None) for g in (grids or (TEST_GRIDS + [k for k in oracle_grid_keys() if k not in TEST_GRIDS]))]
    if grids is None:
        todo += [(g, None) for g in runs_default_grids()] + EXTRA_BUILDS
    with ThreadPoolExecutor(max_workers=int(os.environ.get("BEACON_JIT_JOBS", "4"))) as ex:
        paths = list(ex.map(lambda t: build_plugin(t[0][0], t[0][1], t[0][2], t[0][3], verbose, t[1]), todo))
    # the slow-mode constants of the same grids (beacon_amd/stoprule.py; only the one-row-per-lane rayleigh kernels use them),
    # cached in JIT_DIR too: a test on the GPU box then reads them instead of spending a minute of dense algebra
    from . import stoprule
    cells = [(nx, ny, kind, 0.25) for (nx, ny, f64, kind), _ in todo]
    if grids is None:
        for L, H, f64, kind, _ in oracle_cases():
            nx, ny = _grid(L, H, kind)
            dx, dy = float(L / nx), float(H / ny)
            cells.append((nx, ny, kind, dy * dy / (2.0 * (dx * dx + dy * dy))))
    want = [c for c in sorted(set(cells)) if c[1] <= 128 and min(c[0], c[1]) >= 48 and not os.path.exists(stoprule._cache_file(*c))]
    if want:      # ~10 s of dense algebra per grid: a few grids at a time, two BLAS threads each
        from concurrent.futures import ProcessPoolExecutor
        with ProcessPoolExecutor(max_workers=int(os.environ.get("BEACON_JIT_JOBS", "4"))) as ex:
            list(ex.map(_bounds_job, want))
    if os.path.isdir(JIT_DIR):
        # drop the plugins of older source states of THESE grids (same name up to the hash); plugins that users compiled
        # on demand for other grids stay (a stale one is merely unused: build_plugin() compiles the current hash next to it)
        keep = {os.path.basename(p) for p in paths if p}
        stems = {k.rsplit("_", 1)[0] for k in keep}
        for f in os.listdir(JIT_DIR):
            if f.endswith(".so") and f not in keep and f.rsplit("_", 1)[0] in stems:
                os.remove(os.path.join(JIT_DIR, f))
                for mark in (".ok", ".bad"):
                    if os.path.exists(os.path.join(JIT_DIR, f + mark)):
                        os.remove(os.path.join(JIT_DIR, f + mark))
            elif f.endswith(".lock"):
                # a lock file another process holds (flock) must stay: unlinking it would let a third process lock a NEW
                # file of the same name and compile the same plugin beside the holder
                lp = os.path.join(JIT_DIR, f)
                try:
                    with open(lp, "r+") as lk:
                        fcntl.flock(lk, fcntl.LOCK_EX | fcntl.LOCK_NB)
                        try:
                            os.remove(lp)
                        finally:
                            fcntl.flock(lk, fcntl.LOCK_UN)
                except OSError:
                    pass
    return paths

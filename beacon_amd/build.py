"""The in-tree build of every library this package ships, stated once: libbeacon_hip.so (hand-written HIP for gfx950, hipcc),
libbeacon_actor.so, libbeacon_learner.so and libbeacon_epochs.so (actor.py, learner.py, epochs.py), libbeacon_torch.so (torch_ext.py, g++) and the per-grid kernel
plugins (jit.py).  Each is a `Unit`: its sources, its flags, its commands.  The machinery is Unit's:

  what a library depends on   closure(): the quoted #include lines of its sources, followed transitively
  whether it is current       CONTENT, not mtime (a snapshot or a fresh checkout may reset file times): the sidecar `<lib>.sig` holds
                              a hash of every file of deps(), the flags and the architecture, taken BEFORE the compiler runs
  how it is built             under the file lock `<lib>.lock` (N ranks of one node importing the package at once), objects in a
                              per-process directory under csrc/_obj, four compiles at a time, linked to a temporary name and
                              os.replace'd; the .sig written and renamed; nothing temporary left, on success or failure
  the argv of one file        compile_cmd(): the build, the plugins, scripts and tests that look at a unit's assembly
  BEACON_NO_BUILD=1           no_build()

The shared objects are git-ignored but travel to the GPU box with the snapshot of the tree."""
import ctypes as C
import fcntl
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
INC = os.path.join(os.path.dirname(PKG), "include")
LIB = os.path.join(PKG, "libbeacon_hip.so")
OBJ = os.path.join(PKG, "csrc", "_obj")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-fvisibility=hidden",
         "-fgpu-rdc" if False else "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-but-set-variable"]


# per-file flags.  ns2d_fast: the SLP vectoriser packs the Jacobi arithmetic into v_pk_* ops at the
# price of many register shuffles -- measured slower than the scalar stream on gfx950.
# ns2d_fast2 (256 VGPRs + ~100 spilled): without the scheduler's "unclustered high register pressure" re-scheduling stage the phases
# outside the Jacobi loop lose fewer cycles to spills than the loop gains -- measured twice, A/B/A/B on one box (round 6,
# scripts/variants.py): mixing 100x100 B=512 float32 29.83 -> 29.56 ms, float64 89.7 -> 88.2; the same flag on ns2d_fast: no gain.  Without the SDWA
# peephole on top: 29.92 -> 29.66 (1 301 -> 1 270 cycles per sweep).
# (nine other scheduler switches -- max-ilp / max-memory-clause / iterative-minreg strategies, AMDGPU trackers, no post-RA scheduler, no
# memop clustering, metric bias 0 / 100 -- gained nothing on any of the three kernels: profiles/r06_sched_flags_ab.log)
# ns2d_fast.hip (the float32 instantiations; the float64 ones are ns2d_fast_f64.hip, the same source): -O2 -- measured A/B/A/B on one
# box (round 6): the headline kernel 781 -> 772 cycles per sweep, 18.37 -> 18.18 ms over kstat's 8 steps; the float64 kernel loses
# 0.7 % with it and keeps -O3 (profiles/r06_sched_flags_ab.log)
FILE_FLAGS = {"ns2d_fast.hip": ["-fno-slp-vectorize", "-ffp-contract=on", "-O2"],
              # the float32 one-row built-ins with their Jacobi cells in runs: the flags of ns2d_fast.hip
              "ns2d_fast_runs.hip": ["-fno-slp-vectorize", "-ffp-contract=on", "-O2"],
              "ns2d_fast_f64.hip": ["-fno-slp-vectorize", "-ffp-contract=on"],
              "ns2d_fast2.hip": ["-fno-slp-vectorize", "-ffp-contract=on", "-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule",
                                 "-mllvm", "-amdgpu-sdwa-peephole=0"],
              # the same kernels reading the per-replica parameter table (csrc/ns2d_prm.h): each with the flags of its sibling
              "ns2d_fast_prm.hip": ["-fno-slp-vectorize", "-ffp-contract=on", "-O2"],
              "ns2d_fast_prm_f64.hip": ["-fno-slp-vectorize", "-ffp-contract=on"],
              "ns2d_fast2_prm.hip": ["-fno-slp-vectorize", "-ffp-contract=on", "-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule",
                                     "-mllvm", "-amdgpu-sdwa-peephole=0"],
              # float64 1D kernels: the reference's operation order without FMA contraction -> bit-identical fields
              "env1d_f64.hip": ["-ffp-contract=off"],
              # shkadov's random-start reset loops the float64 step body: the same flag, the same bits
              "shkadov_warm_f64.hip": ["-ffp-contract=off"],
              # float64 ODE envs (lorenz, vortex): the host ports' operation order without FMA contraction -> bit-identical episodes
              "ode_f64.hip": ["-ffp-contract=off"],
              # the GAE recurrence in the operation order its documentation states, one rounding per operation (the float64 NumPy
              # restatement in the tests is the same sequence)
              "rollout.hip": ["-ffp-contract=off"],
              # the frame kernels equal their NumPy restatement byte for byte: one rounding per operation, and the float division the
              # correctly rounded one whatever the toolchain's default becomes
              "render.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]}


# the on-demand kernels (beacon_amd/jit.py: csrc/jit/ns2d_jit.hip, any family, any precision): the flags their verification and
# timings were made with
JIT_FLAGS = ["-fno-slp-vectorize", "-ffp-contract=on"]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def no_build():
    """BEACON_NO_BUILD=1 (exported by the profiling scripts): never spawn a compiler from this process -- under rocprofv3 the
    children would inherit the profiler's preload (scripts/prof_bench.sh).  Read here only.  What follows from it is the caller's:
    Unit.load() raises (a stale binary is never dlopen'ed: its structs and signatures may disagree with this source tree),
    torch_ext.build_ext() and jit.build_plugin() return None."""
    return os.environ.get("BEACON_NO_BUILD") == "1"


def compile_cmd(src, out, file_flags=None, defs=None, extra=(), mode=("-c",), cc=None, tables=None):
    """The argv that compiles one file: FLAGS, the file's own flags, -D `defs`, `extra`, the include directory, `mode` ("-c" for the
    build; ("--cuda-device-only", "-S") for a look at the assembly; ("-shared",) for a plugin).  `file_flags`: the table basename ->
    flags the file is looked up in (default FILE_FLAGS), or the list itself.  `tables`: the build module of another checkout, whose
    FLAGS, FILE_FLAGS, INC and hipcc() are meant (scripts/params_fast_kernels.py compiles two checkouts side by side)."""
    b = tables or sys.modules[__name__]
    ff = b.FILE_FLAGS if file_flags is None else file_flags
    if isinstance(ff, dict):
        ff = ff.get(os.path.basename(src), [])
    return ([cc or b.hipcc()] + b.FLAGS + list(ff) + ["-D%s=%s" % kv for kv in sorted((defs or {}).items())] + list(extra) +
            ["-I", b.INC] + list(mode) + [src, "-o", out])


_INCLUDE = re.compile(rb"^[ \t]*#[ \t]*include\b[ \t]*(.*)$", re.M)


def quoted_includes(path, text):
    """The names of the `#include "..."` lines of `text`; `#include <...>` is the toolchain's and ignored; anything else after
    #include (a macro) is an error: the dependency rule could not follow it."""
    names = []
    for rest in _INCLUDE.findall(text):
        m = re.match(rb'"([^"]+)"|<[^>]+>', rest)
        if m is None:
            raise RuntimeError("%s: `#include %s` is neither \"...\" nor <...>: the build cannot tell what it depends on"
                               % (path, rest.decode(errors="replace").strip()))
        if m.group(1):
            names.append(m.group(1).decode())
    return names


def closure(sources):
    """{path: bytes} of `sources` and every file their quoted includes reach, each include looked for beside the includer, then in
    csrc/, then in include/ (whether or not a preprocessor condition guards it: at least what the compiler reads).  One that
    resolves nowhere is an error."""
    seen, todo = {}, [os.path.abspath(s) for s in sources]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        with open(f, "rb") as fh:
            seen[f] = fh.read()
        for name in quoted_includes(f, seen[f]):
            for d in (os.path.dirname(f), CSRC, INC):
                if os.path.isfile(os.path.join(d, name)):
                    todo.append(os.path.normpath(os.path.join(d, name)))
                    break
            else:
                raise RuntimeError("%s includes \"%s\", which is neither beside it nor in %s nor in %s" % (f, name, CSRC, INC))
    return seen


def sweep_objdirs(root=None):
    """Remove the per-process object directories of builders that are gone (a build that was killed leaves its p<pid> behind,
    and the directory ships with every snapshot of the tree): csrc/_obj/p<pid> and the units' csrc/_obj/<unit>/p<pid>."""
    root = root or OBJ
    if not os.path.isdir(root):
        return
    for d in os.listdir(root):
        if not (d.startswith("p") and d[1:].isdigit()):
            if os.path.isdir(os.path.join(root, d)):
                sweep_objdirs(os.path.join(root, d))
            continue
        pid = int(d[1:])
        if pid != os.getpid():
            try:
                os.kill(pid, 0)                        # still running: somebody else's build in progress
                continue
            except ProcessLookupError:
                pass
            except OSError:
                continue
        shutil.rmtree(os.path.join(root, d), ignore_errors=True)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


class Unit(object):
    """One in-tree library, described as data; deps(), signature(), stale(), build() and load() are stated here once.
    `lib`: the output; `sources`: () -> its source files; `key`: () -> whatever besides file contents belongs in the hash (flags
    without absolute paths, a version); `commands`: (cc, tmp, objdir) -> (compile argvs, run four at a time; the argv that
    writes `tmp`) -- a single-command build has no compile argvs and no `obj`; `compiler`: () -> path or None; `obj`: where the
    per-process object directory goes; `signatures`: symbol -> (restype, argtypes) for load(); `sig`: False for an output that
    carries the hash in its name (a plugin) and has no sidecar."""

    def __init__(self, lib, sources, key, commands, compiler=hipcc, obj=None, signatures=None, sig=True):
        self.lib, self.sources, self.key, self.commands, self.compiler = lib, sources, key, commands, compiler
        self.obj, self.signatures, self.sig, self._loaded = obj, signatures, sig, None

    def deps(self):
        return sorted(closure(self.sources()))

    def signature(self):
        """Hash of everything the library is built from: key(), and name and content of every file of deps().  Independent of
        where the tree lies."""
        h = hashlib.sha256()
        h.update(repr(self.key()).encode())
        for f, text in sorted(closure(self.sources()).items()):
            h.update(os.path.basename(f).encode())
            h.update(text)
        return h.hexdigest()

    def stale(self):
        if not self.sig:
            return not os.path.exists(self.lib)
        if not os.path.exists(self.lib) or not os.path.exists(self.lib + ".sig"):
            return True
        with open(self.lib + ".sig") as fh:
            return fh.read().strip() != self.signature()

    def build(self, force=False, verbose=False):
        """Build the library if it is stale (or `force`); returns its path.  The signature is taken before the compiler runs, so
        a source edited during the build leaves the library stale.  Whatever happens, no temporary file and no object directory
        stays behind, and the previous library and .sig stay whole until the new ones replace them."""
        if not force and not self.stale():
            sweep_objdirs()
            return self.lib
        cc = self.compiler()
        if cc is None:
            raise RuntimeError("no compiler found: cannot build %s" % os.path.basename(self.lib))
        os.makedirs(os.path.dirname(self.lib), exist_ok=True)
        tmp, sigtmp = "%s.tmp%d" % (self.lib, os.getpid()), "%s.sig.tmp%d" % (self.lib, os.getpid())
        objdir = os.path.join(self.obj, "p%d" % os.getpid()) if self.obj else None
        with open(self.lib + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)           # one builder at a time per output (N ranks of one node ask at once)
            try:
                if not force and not self.stale():     # another process built it while we waited
                    return self.lib
                sig = self.signature()
                if objdir:
                    os.makedirs(objdir, exist_ok=True)
                compiles, link = self.commands(cc, tmp, objdir)
                with ThreadPoolExecutor(max_workers=4) as ex:       # (never sized by the CPU count: a GPU box lends 16 of many)
                    list(ex.map(lambda cmd: _run(cmd, verbose), compiles))
                _run(link, verbose)
                os.replace(tmp, self.lib)
                if self.sig:
                    with open(sigtmp, "w") as fh:
                        fh.write(sig + "\n")
                    os.replace(sigtmp, self.lib + ".sig")
            finally:
                for f in (tmp, sigtmp):
                    if os.path.exists(f):
                        os.remove(f)
                if objdir:
                    shutil.rmtree(objdir, ignore_errors=True)
                sweep_objdirs()
                fcntl.flock(lock, fcntl.LOCK_UN)
        return self.lib

    def load(self, signatures=None, mode=C.DEFAULT_MODE, no_compiler=None):
        """dlopen the library (building it first when stale) and declare every symbol of the table; a missing library or symbol is
        an error.  `no_compiler`: the error text of a stale library that nothing here can build."""
        if self._loaded is None:
            if self.stale():
                if no_build():
                    raise RuntimeError("%s is missing or stale and BEACON_NO_BUILD=1: run "
                                       "`python -c 'import __graft_entry__ as g; g.build()'` first" % os.path.basename(self.lib))
                if no_compiler and self.compiler() is None:
                    raise RuntimeError(no_compiler)
                self.build()
            L = C.CDLL(self.lib, mode=mode)
            for name, (res, args) in (signatures or self.signatures).items():
                fn = getattr(L, name)                  # AttributeError if the library lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            self._loaded = L
        return self._loaded


def hip_library(lib, src_dir, file_flags, obj, signatures=None):
    """The Unit of a library of src_dir/*.hip: every file with FLAGS and its entry of `file_flags` (a table, or () -> table),
    linked by hipcc.  FLAGS and a callable's table are read when they are used, not here: scripts/kstat.py and its kin extend
    FLAGS, or rebind FILE_FLAGS, and then build."""
    table = file_flags if callable(file_flags) else (lambda: file_flags)

    def sources():
        return sorted(glob.glob(os.path.join(src_dir, "*.hip")))

    def commands(cc, tmp, objdir):
        objs = [os.path.join(objdir, os.path.basename(s)[:-4] + ".o") for s in sources()]
        return ([compile_cmd(s, o, table(), cc=cc) for s, o in zip(sources(), objs)],
                [cc, "-shared", "-fPIC", "--offload-arch=" + ARCH, "-o", tmp] + objs)

    return Unit(lib, sources, lambda: (ARCH, FLAGS, sorted(table().items())), commands, obj=obj, signatures=signatures)


# libbeacon_hip.so: every csrc/*.hip.  (include/beacon_actor.h and beacon_learner.h belong to libbeacon_actor.so and
# libbeacon_learner.so, units of their own -- beacon_amd/actor.py, beacon_amd/learner.py; no source of this library includes them)
MAIN = hip_library(LIB, CSRC, lambda: FILE_FLAGS, OBJ)
sources, _deps, signature, stale = MAIN.sources, MAIN.deps, MAIN.signature, MAIN.stale


def build_lib(force=False, verbose=False):
    """Compile every csrc/*.hip for gfx950 and link libbeacon_hip.so.  Returns its path."""
    return MAIN.build(force=force, verbose=verbose)


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))

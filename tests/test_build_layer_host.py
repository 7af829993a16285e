"""The in-tree build, stated once in beacon_amd/build.py: what a library depends on (the closure of its quoted includes), what moves its
signature, and the one build step (signature first, lock, private objects, atomic replace, nothing left behind) -- the step on a toy
library whose "compiler" is a Python script, so neither hipcc nor a GPU is involved."""
import builtins
import glob
import io
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the -D set of one on-demand grid (75x50 float32 rayleigh: one row per lane, strips of 10 columns), as jit.build_plugin states it
PLUGIN_DEFS = {"BCN_JIT_ROWS": 1, "BCN_JIT_REAL": "float", "BCN_JIT_NX": 75, "BCN_JIT_NY": 50, "BCN_JIT_R": 10, "BCN_JIT_KIND": 0, "BCN_JIT_GF": 0}
KINDS = ("main", "actor", "learner", "extension", "plugin")


def _unit(kind):
    from beacon_amd import actor, build, jit, learner, torch_ext
    return {"main": lambda: build.MAIN, "actor": lambda: actor._UNIT, "learner": lambda: learner._UNIT, "extension": lambda: torch_ext._UNIT,
            "plugin": lambda: jit._unit(PLUGIN_DEFS)}[kind]()


def _edited(monkeypatch, path):
    """From here on, whoever reads `path` as bytes gets its content plus one line; nothing on disk is touched."""
    real_open, path = builtins.open, os.path.abspath(path)

    def edited(f, mode="r", *a, **kw):
        if mode == "rb" and os.path.abspath(f) == path:
            with real_open(f, "rb") as fh:
                return io.BytesIO(fh.read() + b"\n// edited\n")
        return real_open(f, mode, *a, **kw)
    monkeypatch.setattr(builtins, "open", edited)


def _as_built(monkeypatch, tmp_path, u):
    """`u` as if it had just been built, somewhere else: a library and the sidecar its description asks for."""
    monkeypatch.setattr(u, "lib", str(tmp_path / "lib.so"))
    open(u.lib, "w").close()
    if u.sig:
        with open(u.lib + ".sig", "w") as fh:
            fh.write(u.signature() + "\n")
    assert not u.stale()


def _path(name):
    from beacon_amd import build
    hits = [p for p in (os.path.join(build.INC, name), os.path.join(build.CSRC, name)) if os.path.exists(p)]
    assert len(hits) == 1, name
    return hits[0]


# ---- the dependency rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_file_of_deps_moves_the_signature(kind, monkeypatch, tmp_path):
    u = _unit(kind)
    deps, before = u.deps(), u.signature()
    assert set(u.sources()) <= set(deps) and len(deps) > len(u.sources()) and all(os.path.isabs(f) for f in deps)
    _as_built(monkeypatch, tmp_path, u)
    for f in deps:
        with monkeypatch.context() as m:
            _edited(m, f)
            assert u.signature() != before, f
            if u.sig:
                assert u.stale(), f
            else:                                  # named by its hash: the edited source's library is another file
                assert u.signature()[:12] not in before
        assert u.signature() == before and not u.stale()


@pytest.mark.parametrize("kind,names", [("plugin", ("render.h", "beacon_actor.h")),
                                        ("main", ("beacon_actor.h", "beacon_learner.h", "ns2d_fast4_impl.h"))])
def test_a_file_outside_deps_does_not_move_the_signature(kind, names, monkeypatch):
    u = _unit(kind)
    before = u.signature()
    for name in names:
        assert _path(name) not in u.deps()
        with monkeypatch.context() as m:
            _edited(m, _path(name))
            with open(_path(name), "rb") as fh:
                assert fh.read().endswith(b"// edited\n")              # the edit is in force
            assert u.signature() == before, name


def test_the_c_header_moves_every_library_that_includes_it(monkeypatch):
    units = [_unit(k) for k in KINDS]
    before = [u.signature() for u in units]
    _edited(monkeypatch, _path("beacon_hip.h"))
    for kind, u, b in zip(KINDS, units, before):
        assert u.signature() != b, kind


def test_the_signature_does_not_depend_on_where_the_tree_lies():
    """What is hashed besides the files: no absolute path among it (the files go in by basename and content)."""
    for kind in KINDS:
        flat = repr(_unit(kind).key())
        assert ROOT not in flat and not re.search(r"'/\w", flat), (kind, flat)


def test_no_include_the_rule_cannot_classify():
    """Every #include under csrc/ and include/ is <...> or "...", and every quoted one resolves by the rule (beside the includer,
    csrc/, include/): the closure of ALL files stands."""
    from beacon_amd import build
    files = [os.path.join(d, f) for top in (build.CSRC, build.INC) for d, _, fs in os.walk(top) if "_obj" not in d for f in fs
             if f.endswith((".h", ".hip", ".inc", ".cpp"))]
    assert len(files) > 50
    n = 0
    for f in files:
        with open(f, "rb") as fh:
            text = fh.read()
        n += len(build.quoted_includes(f, text))
        assert len(re.findall(rb"^[ \t]*#[ \t]*include\b", text, flags=re.M)) == len(re.findall(rb"^[ \t]*#[ \t]*include[ \t]*[<\"]", text, flags=re.M)), f
    assert n > 80 and set(build.closure(files)) == {os.path.abspath(f) for f in files}


def test_the_rule_reads_include_lines(tmp_path):
    from beacon_amd import build
    text = b'#include <vector>\n  #  include "a.h"  // why\n// #include "commented.h"\n#if 0\n#include "guarded.h"\n#endif\nint x; /* #include "inline.h" */\n'
    assert build.quoted_includes("t", text) == ["a.h", "guarded.h"]
    with pytest.raises(RuntimeError, match="neither"):
        build.quoted_includes("t", b"#define H \"a.h\"\n#include H\n")
    # beside the includer first, then csrc/, then include/; one that is nowhere is an error
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "s.hip").write_bytes(b'#include "bcn_common.h"\n#include "../up.h"\n')
    (tmp_path / "sub" / "bcn_common.h").write_bytes(b"// a namesake beside the includer wins\n")
    (tmp_path / "up.h").write_bytes(b'#include "beacon_actor.h"\n')
    got = build.closure([str(tmp_path / "sub" / "s.hip")])
    assert set(got) == {str(tmp_path / "sub" / "s.hip"), str(tmp_path / "sub" / "bcn_common.h"), str(tmp_path / "up.h"),
                        os.path.join(build.INC, "beacon_actor.h")}
    (tmp_path / "up.h").write_bytes(b'#include "no_such_header.h"\n')
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        build.closure([str(tmp_path / "sub" / "s.hip")])


def test_the_closure_holds_what_the_preprocessor_reads(tmp_path):
    """hipcc -MM (host pass, the unit's own flags) of every source of every hipcc-built library and of the plugin source with one
    grid's -D set: each file it lists inside the repository is in that library's deps()."""
    from beacon_amd import build, jit
    if build.hipcc() is None:
        pytest.skip("no hipcc")
    jobs = []
    for kind in ("main", "actor", "learner", "plugin"):
        u = _unit(kind)
        for i, cmd in enumerate(u.commands(build.hipcc(), str(tmp_path / "unused"), str(tmp_path))[0] or [u.commands(build.hipcc(), "unused", None)[1]]):
            src = [a for a in cmd if a.endswith(".hip")]
            assert len(src) == 1
            cut = cmd[:cmd.index("-c") if "-c" in cmd else cmd.index("-shared")]        # compiler, flags, -D, -I: the unit's own
            jobs.append((kind, set(u.deps()), cut + ["--cuda-host-only", "-MM", src[0], "-o", str(tmp_path / ("%s%d.d" % (kind, i)))]))
    assert len(jobs) == len(build.sources()) + 5 and jit.JIT_SRC in jobs[-1][2]

    def listed(job):
        subprocess.run(job[2], check=True, capture_output=True)
        with open(job[2][-1]) as fh:
            return [os.path.normpath(p) for p in fh.read().replace("\\\n", " ").split()[1:]]
    with ThreadPoolExecutor(max_workers=4) as ex:
        for (kind, deps, cmd), files in zip(jobs, ex.map(listed, jobs)):
            inside = {f for f in files if f.startswith(ROOT + os.sep)}
            assert inside and inside <= deps, (kind, cmd[-3], sorted(inside - deps))


# ---- the build step, on a toy library --------------------------------------------------------------------------------------------
STUB = r'''
import os, sys, time
ctl, what, out, ins = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
flag = lambda name: os.path.exists(os.path.join(ctl, name))
with open(os.path.join(ctl, "log"), "a") as fh:
    fh.write(what + "\n")
data = b"".join(open(f, "rb").read() for f in ins)
if what == "cc" and flag("edit"):                      # the source changes while it "compiles"
    with open(ins[0], "ab") as fh:
        fh.write(b"// edited during the build\n")
if what == "ld" and flag("wait"):                      # hold the lock until the other builder stands in front of it
    open(os.path.join(ctl, "started"), "w").close()
    for _ in range(12000):
        if flag("go"):
            break
        time.sleep(0.005)
    else:
        sys.exit(3)
with open(out, "wb") as fh:
    fh.write(data)
sys.exit(1 if flag("fail_" + what) else 0)
'''


def toy_unit(root):
    """A library of two sources and a header under `root`, "compiled" by STUB (copy) and "linked" (concatenate)."""
    from beacon_amd import build
    root = str(root)
    stub = os.path.join(root, "stub.py")
    if not os.path.exists(stub):
        os.makedirs(os.path.join(root, "src"))
        for name, text in (("a.src", '#include "toy.h"\na\n'), ("b.src", "b\n"), ("toy.h", "h\n")):
            with open(os.path.join(root, "src", name), "w") as fh:
                fh.write(text)
        with open(stub, "w") as fh:
            fh.write(STUB)

    def sources():
        return sorted(glob.glob(os.path.join(root, "src", "*.src")))

    def commands(cc, tmp, objdir):
        objs = [os.path.join(objdir, os.path.basename(s) + ".o") for s in sources()]
        return [[cc, stub, root, "cc", o, s] for s, o in zip(sources(), objs)], [cc, stub, root, "ld", tmp] + objs
    return build.Unit(os.path.join(root, "out", "libtoy.so"), sources, lambda: ("toy",), commands, compiler=lambda: sys.executable,
                      obj=os.path.join(root, "_obj", "toy"))


def _log(root):
    with open(os.path.join(str(root), "log")) as fh:
        return fh.read().split()


def _leftovers(root):
    return [os.path.join(d, n) for d, ds, fs in os.walk(str(root)) for n in ds + fs if ".tmp" in n or re.fullmatch(r"p\d+", n)]


@pytest.fixture
def toy(tmp_path, monkeypatch):
    from beacon_amd import build
    monkeypatch.setattr(build, "OBJ", str(tmp_path / "_obj"))        # (the sweep's root: the toy's directory lies under it, as a unit's does)
    return toy_unit(tmp_path)


def test_a_build_records_the_signature_and_leaves_nothing_behind(toy, tmp_path):
    assert toy.stale() and [os.path.basename(f) for f in toy.deps()] == ["a.src", "b.src", "toy.h"]
    sig = toy.signature()
    assert toy.build() == toy.lib and not toy.stale()
    assert open(toy.lib).read() == '#include "toy.h"\na\nb\n' and open(toy.lib + ".sig").read() == sig + "\n"
    assert _log(tmp_path) == ["cc", "cc", "ld"] and not _leftovers(tmp_path)
    assert toy.build() == toy.lib and _log(tmp_path) == ["cc", "cc", "ld"]            # fresh: no compiler
    toy.build(force=True)
    assert _log(tmp_path) == ["cc", "cc", "ld"] * 2 and not _leftovers(tmp_path)


@pytest.mark.parametrize("stage", ["cc", "ld"])
def test_a_failed_build_leaves_the_previous_library_whole(stage, toy, tmp_path):
    toy.build()
    was = open(toy.lib, "rb").read(), open(toy.lib + ".sig", "rb").read()
    with open(toy.sources()[1], "a") as fh:
        fh.write("b2\n")
    (tmp_path / ("fail_" + stage)).touch()
    assert toy.stale()
    with pytest.raises(subprocess.CalledProcessError):
        toy.build()
    assert (open(toy.lib, "rb").read(), open(toy.lib + ".sig", "rb").read()) == was and toy.stale()
    assert _log(tmp_path)[3:] == (["cc", "cc"] if stage == "cc" else ["cc", "cc", "ld"])      # it did get that far
    assert not _leftovers(tmp_path)


def test_the_recorded_signature_is_the_one_from_before_the_compiler_ran(toy, tmp_path):
    before = toy.signature()
    (tmp_path / "edit").touch()
    toy.build()
    assert open(toy.sources()[0]).read().endswith("// edited during the build\n")
    assert open(toy.lib + ".sig").read().strip() == before != toy.signature()
    assert toy.stale()                                     # the edit is not in the library: it is built again


def test_two_builders_of_one_stale_library_build_it_once(toy, tmp_path, monkeypatch):
    """The other process links (and holds the lock) until this one stands in front of the lock, past its first staleness check; this
    one then finds the library fresh behind the lock and starts no compiler."""
    from beacon_amd import build
    (tmp_path / "wait").touch()
    code = "import sys; sys.path[:0] = [%r, %r]; import test_build_layer_host as t; t.toy_unit(%r).build()" % (ROOT, os.path.dirname(__file__), str(tmp_path))
    other = subprocess.Popen([sys.executable, "-c", code])
    try:
        for _ in range(12000):
            if (tmp_path / "started").exists() or other.poll() is not None:
                break
            time.sleep(0.005)
        assert (tmp_path / "started").exists() and other.poll() is None and toy.stale()
        real_flock, asked = build.fcntl.flock, []

        def flock(fh, op):
            if op == build.fcntl.LOCK_EX:
                asked.append(fh.name)
                (tmp_path / "go").touch()
            return real_flock(fh, op)
        monkeypatch.setattr(build.fcntl, "flock", flock)
        assert toy.build() == toy.lib
        assert asked == [toy.lib + ".lock"]
    finally:
        (tmp_path / "go").touch()
        assert other.wait() == 0
    assert _log(tmp_path) == ["cc", "cc", "ld"] and not toy.stale() and not _leftovers(tmp_path)


def test_the_object_directories_of_dead_builders_are_swept_for_every_library(toy, tmp_path):
    gone = subprocess.Popen([sys.executable, "-c", "pass"])
    gone.wait()
    dead, live = "p%d" % gone.pid, "p%d" % os.getppid()
    dirs = [tmp_path / "_obj" / dead, tmp_path / "_obj" / "toy" / dead, tmp_path / "_obj" / "actor" / dead, tmp_path / "_obj" / "learner" / live]
    for d in dirs:
        d.mkdir(parents=True)
        (d / "x.o").touch()
    toy.build()
    assert [d.exists() for d in dirs] == [False, False, False, True]
    dirs[1].mkdir()
    toy.build()                                            # fresh: nothing is compiled, the sweep still runs
    assert _log(tmp_path) == ["cc", "cc", "ld"] and not dirs[1].exists() and dirs[3].exists()


def test_no_build_has_its_four_outcomes(monkeypatch, tmp_path):
    """BEACON_NO_BUILD=1 with every library missing: _lib.load and a unit's load raise, build_ext and build_plugin return None, and
    nobody starts a compiler."""
    from beacon_amd import _lib, actor, build, jit, torch_ext

    def no_compiler(*a, **k):
        raise AssertionError("a compiler was started: %r" % (a,))
    monkeypatch.setattr(build.subprocess, "check_call", no_compiler)
    monkeypatch.setattr(_lib, "_LIB", None)
    for u in (build.MAIN, actor._UNIT, torch_ext._UNIT):
        monkeypatch.setattr(u, "lib", str(tmp_path / os.path.basename(u.lib)))
        monkeypatch.setattr(u, "_loaded", None)
    monkeypatch.setattr(jit, "JIT_DIR", str(tmp_path / "_jit"))
    monkeypatch.setattr(jit, "choose", lambda nx, ny, f64, kind: {"rows": 1, "R": 10, "gf": 0, "nw": 8})
    monkeypatch.setenv("BEACON_NO_BUILD", "1")
    with pytest.raises(RuntimeError, match=r"^libbeacon_hip\.so is missing or stale and BEACON_NO_BUILD=1: run `python -c 'import __graft_entry__ as g; g\.build\(\)'` first$"):
        _lib.load()
    with pytest.raises(RuntimeError, match=r"^libbeacon_actor\.so is missing or stale and BEACON_NO_BUILD=1: run `python -c 'import __graft_entry__ as g; g\.build\(\)'` first$"):
        actor.load()
    assert torch_ext.build_ext() is None and torch_ext.build_ext(force=True) is None
    assert jit.build_plugin(75, 50, False, 0) is None
    assert os.listdir(str(tmp_path)) == []
    # without the variable and without hipcc: the main library's other text
    monkeypatch.delenv("BEACON_NO_BUILD")
    monkeypatch.setattr(build.MAIN, "compiler", lambda: None)
    with pytest.raises(RuntimeError, match="missing or older than its sources and hipcc is not available to build it; beacon_amd has no CPU fallback"):
        _lib.load()


def test_a_plugin_that_cannot_be_built_is_a_warning_and_leaves_no_file(monkeypatch, tmp_path):
    """The plugins go through the same routine with their differences: a compiler error is a JitWarning and None, not an exception,
    the half-written temporary output is gone, and no .sig is written for a library named by its hash."""
    from beacon_amd import build, jit
    monkeypatch.setattr(jit, "JIT_DIR", str(tmp_path / "_jit"))
    monkeypatch.setattr(jit, "choose", lambda nx, ny, f64, kind: {"rows": 1, "R": 10, "gf": 0, "nw": 8})
    monkeypatch.setattr(build, "OBJ", str(tmp_path / "_obj"))
    cc = tmp_path / "cc"
    cc.write_text("#!%s\nimport os, sys\na = sys.argv\nopen(a[a.index('-o') + 1], 'w').write('half')\n"
                  "sys.exit(int(os.path.exists(%r)))\n" % (sys.executable, str(tmp_path / "fail")))
    cc.chmod(0o755)
    monkeypatch.setenv("HIPCC", str(cc))                   # build.hipcc() takes it
    (tmp_path / "fail").touch()
    with pytest.warns(jit.JitWarning, match="no register-resident kernel for 75x50"):
        assert jit.build_plugin(75, 50, False, 0) is None
    assert [f for f in os.listdir(str(tmp_path / "_jit")) if not f.endswith(".lock")] == []
    (tmp_path / "fail").unlink()
    path = jit.build_plugin(75, 50, False, 0)
    assert os.path.basename(path) == "ns2d_75x50_f32_k0_r10_%s.so" % jit._unit(PLUGIN_DEFS).signature()[:12]
    assert [f for f in os.listdir(str(tmp_path / "_jit")) if not f.endswith(".lock")] == [os.path.basename(path)]

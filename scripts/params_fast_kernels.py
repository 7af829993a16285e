#!/usr/bin/env python3
"""Per-kernel resource table of the register-resident 2D units, from hipcc's device assembly.

    python scripts/params_fast_kernels.py [--root CHECKOUT] [--out FILE.json] [--asm-dir DIR]

Compiles ns2d_fast.hip, ns2d_fast_f64.hip, ns2d_fast2.hip and one on-demand plugin grid per kernel family
(`hipcc --offload-arch=gfx950 --cuda-device-only -S`, the library's own flags) of the checkout at --root and
writes, keyed by unit and mangled kernel name: .vgpr_count, .sgpr_count, .private_segment_fixed_size, the LDS size
and the number of instruction lines.  Run on the commit BEFORE the per-replica parameter kernels it produced
tests/golden/params_fast_parent_kernels.json; tests/test_params_fast_host.py runs the same functions on the tree
under test and expects the same table: the plain units kept their code.  --asm-dir keeps the assembly files
(for a full diff of two checkouts).

    python scripts/params_fast_kernels.py --resources FILE.md

compiles the parameter units (ns2d_fast_prm.hip, ns2d_fast_prm_f64.hip, ns2d_fast2_prm.hip) and the parameter plugins of
PLUGIN_GRIDS as well and writes every table-reading kernel next to its plain sibling: VGPRs, SGPRs, scratch bytes, occupancy
(the figures of -Rpass-analysis=kernel-resource-usage, read from the assembly's metadata and its "; Occupancy:" comments), the
number of instruction lines, and the scalar loads of the unit (s_load_*: the table reads are among them).

    python scripts/params_fast_kernels.py --compare PARENT_ROOT [--jobs N] [--only TEXT] [--asm-dir DIR] [--out FILE.md]

compiles every object of compare_objects() -- the generic unit, the register-resident units and their parameter twins, the plugin
grids of COMPARE_GRIDS, the parameter plugins of jit.PRM_TEST_GRIDS and the four units of the actor and the learner (POLICY_UNITS;
--only actor/, --only learner/) -- for this tree (--root) and for the checkout at
PARENT_ROOT (a `git worktree` of the parent commit) and reports, per object and per kernel symbol, `identical` or the resource
rows that differ: whole-file identity first, else per-function bodies with their local labels renumbered.  What a refactoring of
the kernel sources that must not change the code is checked with.  --only: the objects whose name contains TEXT; with --asm-dir
the parent's files already there (DIR/parent) are reused.  Exit status 1 unless every kernel is identical."""
import argparse
import importlib.machinery
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
import zlib

UNITS = ("ns2d_fast.hip", "ns2d_fast_f64.hip", "ns2d_fast2.hip")
# one plugin grid per family (beacon_amd/jit.py: TEST_GRIDS): rows 1, rows 2, rows 4
PLUGIN_GRIDS = ((75, 50, False, 0), (100, 110, False, 1), (50, 150, False, 0))
# --compare: every unit that includes the 2D cell arithmetic, and plugin grids per family -- one row per lane (float32, float64,
# float64 with dead columns), two rows (mixing, float64 odd ny on the global scratch, float64 mixing), the hybrid
COMPARE_UNITS = ("ns2d_generic.hip",) + UNITS + ("ns2d_fast_prm.hip", "ns2d_fast_prm_f64.hip", "ns2d_fast2_prm.hip")
COMPARE_GRIDS = ((75, 50, False, 0), (75, 50, True, 0), (52, 50, True, 0), (100, 110, False, 1), (50, 75, True, 0),
                 (100, 105, True, 1), (50, 150, False, 0), (50, 150, True, 0), (100, 200, False, 1))
# --compare: the units that include the policy network (csrc/actor/policy_net.h)
POLICY_UNITS = ("actor/actor.hip", "actor/actor_f64.hip", "learner/learner.hip", "learner/learner_f64.hip")


def _load(root, name):
    """beacon_amd/<name>.py of the checkout at `root`, inside a stand-in package per checkout: a module's `from . import build` is
    that checkout's build.py, and the checkout's __init__.py does not run."""
    pkg = "_pfk_%08x" % zlib.crc32(os.path.abspath(root).encode())
    if pkg not in sys.modules:
        spec = importlib.machinery.ModuleSpec(pkg, None, is_package=True)
        spec.submodule_search_locations = [os.path.join(root, "beacon_amd")]
        sys.modules[pkg] = importlib.util.module_from_spec(spec)
    return importlib.import_module(pkg + "." + name)


def normalise(text):
    """The assembly without what depends on where and when it was compiled: the compilation-unit id."""
    return re.sub(r"__hip_cuid_\w+", "__hip_cuid_", text)


def kernel_table(text):
    """{kernel symbol: {vgpr, sgpr, scratch, lds, insts}} of a device assembly file"""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)

        def num(key):
            return int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.M | re.S).group(1)
        insts = len(re.findall(r"^\t[a-z]\w*(?:\s|$)", body, flags=re.M))
        out[name] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), scratch=num("private_segment_fixed_size"),
                         lds=num("group_segment_fixed_size"), insts=insts)
    return out


def occupancy(text):
    """{kernel symbol: waves per SIMD} from the "; Occupancy:" comment behind each kernel"""
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^; Occupancy: (\d+)", text, flags=re.M | re.S):
        out[m.group(1)] = int(m.group(2))
    return out


def scalar_loads(text, name):
    body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.M | re.S).group(1)
    return len(re.findall(r"^\ts_load_", body, flags=re.M)), len(re.findall(r"^\t(?:global|flat)_load_", body, flags=re.M))


def sibling(name):
    """What pairs a table-reading kernel with its plain sibling: the mangled name up to the argument list, and plain / ticketed"""
    return name.split("Ev8NS2DArgsIT_E")[0], "SchedCtl" in name


def resources(root, asm_dir):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if here not in sys.path:
        sys.path.insert(0, here)
    from beacon_amd import jit
    build = _load(root, "build")
    pairs = [(u, u.replace(".hip", "_prm.hip").replace("_f64_prm", "_prm_f64")) for u in UNITS]
    texts = []
    for plain, prm in pairs:
        texts.append((plain, unit_asm(build, plain, os.path.join(asm_dir, plain + ".s")), unit_asm(build, prm, os.path.join(asm_dir, prm + ".s"))))
    for g in PLUGIN_GRIDS:
        stem = os.path.join(asm_dir, plugin_key(g).replace(" ", "_"))
        texts.append((plugin_key(g), plugin_asm(build, plugin_defs(jit.choose, *g), stem + ".s"),
                      plugin_asm(build, plugin_defs(jit.choose, *g, extra={"BCN_JIT_PRM": 1}), stem + "_prm.s")))
    rows = []
    for unit, t0, t1 in texts:
        k0, k1, o0, o1 = kernel_table(t0), kernel_table(t1), occupancy(t0), occupancy(t1)
        by = {sibling(n): n for n in k0}
        for n1 in sorted(k1):
            n0 = by.get(sibling(n1))
            if n0 is None or "NS2DArgs" not in n1:
                continue
            short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", n1.split("Ev8NS2DArgs")[0])
            a, b = k0[n0], k1[n1]
            s0, s1 = scalar_loads(t0, n0), scalar_loads(t1, n1)
            rows.append("| %s | %s | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d |" % (
                unit, short, a["vgpr"], b["vgpr"], a["sgpr"], b["sgpr"], a["scratch"], b["scratch"], o0[n0], o1[n1],
                a["insts"], b["insts"], s0[0], s1[0], s0[1], s1[1]))
    head = ("| unit | kernel | VGPRs | SGPRs | scratch bytes | occupancy | instruction lines | s_load | global / flat loads |\n"
            "|---|---|---|---|---|---|---|---|---|\n")
    return head + "\n".join(rows) + "\n"


ASM = ("--cuda-device-only", "-S")


def _compile_cmd(build, src, out, file_flags=None, defs=None):
    """This tree's build.compile_cmd over the tables (FLAGS, FILE_FLAGS, include directory) of the checkout `build` is of, which
    may be from before it had the function."""
    from beacon_amd.build import compile_cmd
    return compile_cmd(src, out, file_flags, defs, mode=ASM, tables=build)


def unit_asm(build, unit, out_path, file_flags=None):
    """`file_flags`: the table of per-file flags when it is not build.FILE_FLAGS (the actor's, the learner's)"""
    subprocess.check_call(_compile_cmd(build, os.path.join(build.CSRC, unit), out_path, file_flags))
    return normalise(open(out_path).read())


def plugin_defs(jit_choose, nx, ny, f64, kind, extra=None):
    m = jit_choose(nx, ny, f64, kind)
    defs = {"BCN_JIT_ROWS": m["rows"], "BCN_JIT_REAL": "double" if f64 else "float", "BCN_JIT_NX": nx, "BCN_JIT_NY": ny,
            "BCN_JIT_R": m["R"], "BCN_JIT_KIND": kind, "BCN_JIT_GF": m["gf"]}
    if m["rows"] == 4:
        defs["BCN_JIT_RPL"] = m["rpl"]
    defs.update(extra or {})
    return defs


def plugin_asm(build, defs, out_path):
    subprocess.check_call(_compile_cmd(build, os.path.join(build.CSRC, "jit", "ns2d_jit.hip"), out_path, build.JIT_FLAGS, defs))
    return normalise(open(out_path).read())


def plugin_key(g):
    return "jit %dx%d %s k%d" % (g[0], g[1], "f64" if g[2] else "f32", g[3])


def table_of(root, asm_dir):
    """The table of the checkout at `root` (its sources, its build flags; the grid -> family mapping is this tree's jit.choose)."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if here not in sys.path:
        sys.path.insert(0, here)
    from beacon_amd import jit
    build = _load(root, "build")
    out = {}
    for unit in UNITS:
        out[unit] = kernel_table(unit_asm(build, unit, os.path.join(asm_dir, unit + ".s")))
    for g in PLUGIN_GRIDS:
        out[plugin_key(g)] = kernel_table(plugin_asm(build, plugin_defs(jit.choose, *g), os.path.join(asm_dir, plugin_key(g).replace(" ", "_") + ".s")))
    return out


def compare_objects(jit):
    """[(name, compile(build, out_path) -> normalised assembly)] of --compare"""
    objs = [(u, lambda b, o, u=u: unit_asm(b, u, o)) for u in COMPARE_UNITS]
    for grids, extra, tail in ((COMPARE_GRIDS, None, ""), (jit.PRM_TEST_GRIDS, {"BCN_JIT_PRM": 1}, " prm")):
        for g in grids:
            objs.append((plugin_key(g) + tail, lambda b, o, g=g, extra=extra: plugin_asm(b, plugin_defs(jit.choose, *g, extra=extra), o)))
    for u in POLICY_UNITS:                              # their flags: FILE_FLAGS of actor.py / learner.py of the checkout `b` is of
        objs.append((u, lambda b, o, u=u: unit_asm(b, u, o, _load(os.path.dirname(b.PKG), u.split("/")[0]).FILE_FLAGS)))
    return objs


def function_bodies(text):
    """{kernel symbol: its instructions, local labels renumbered in order of appearance}"""
    out = {}
    for name in kernel_table(text):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.M | re.S).group(1)
        seen = {}
        out[name] = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), body)
    return out


def compare(root, parent, asm_dir, jobs, only):
    """(markdown report, all identical) of this tree against the checkout at `parent`"""
    from concurrent.futures import ThreadPoolExecutor
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if here not in sys.path:
        sys.path.insert(0, here)
    from beacon_amd import jit
    objs = [o for o in compare_objects(jit) if only is None or only in o[0]]
    sides = {"parent": _load(parent, "build"), "this": _load(root, "build")}
    for side in sides:
        os.makedirs(os.path.join(asm_dir, side), exist_ok=True)

    def one(job):
        side, (name, fn) = job
        path = os.path.join(asm_dir, side, name.replace(" ", "_").replace("/", "_") + ".s")
        if side == "parent" and os.path.exists(path):
            return normalise(open(path).read())
        return fn(sides[side], path)
    jobs_ = [(side, o) for o in objs for side in ("parent", "this")]
    with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16))) as ex:
        texts = dict(zip(((s, o[0]) for s, o in jobs_), ex.map(one, jobs_)))
    lines = ["| object | kernel | code |", "|---|---|---|"]
    same = True
    for name, _ in objs:
        t0, t1 = texts[("parent", name)], texts[("this", name)]
        k0, k1 = kernel_table(t0), kernel_table(t1)
        b0, b1 = (None, None) if t0 == t1 else (function_bodies(t0), function_bodies(t1))
        lines.append("| %s | whole file, %d kernels | %s |" % (name, len(k1), "identical" if t0 == t1 else "differs"))
        for k in sorted(set(k0) | set(k1)):
            if k not in k0 or k not in k1:
                verdict = "only in the parent" if k in k0 else "only in this tree"
            elif t0 == t1 or b0[k] == b1[k]:
                verdict = "identical"
            else:
                verdict = "DIFFERS: " + ", ".join("%s %d -> %d" % (f, k0[k][f], k1[k][f]) for f in ("vgpr", "sgpr", "scratch", "lds", "insts"))
            same = same and verdict == "identical"
            lines.append("| %s | `%s` | %s |" % (name, k, verdict))
    lines.append("")
    lines.append("%d objects: %s" % (len(objs), "every kernel identical to the parent's" if same else "NOT all identical"))
    return "\n".join(lines) + "\n", same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--asm-dir", default=None)
    ap.add_argument("--resources", default=None, help="write the plain / parameter resource table (markdown rows) to this file")
    ap.add_argument("--compare", default=None, metavar="PARENT_ROOT", help="report, per kernel, whether this tree's code is the parent checkout's")
    ap.add_argument("--jobs", type=int, default=8, help="--compare: compiles at a time (at most 16)")
    ap.add_argument("--only", default=None, help="--compare: only the objects whose name contains this text")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm_dir = a.asm_dir or tmp
        os.makedirs(asm_dir, exist_ok=True)
        if a.compare:
            report, same = compare(os.path.abspath(a.root), os.path.abspath(a.compare), asm_dir, a.jobs, a.only)
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(report)
            sys.stdout.write(report)
            sys.exit(0 if same else 1)
        if a.resources:
            with open(a.resources, "w") as fh:
                fh.write(resources(os.path.abspath(a.root), asm_dir))
            return
        tab = table_of(os.path.abspath(a.root), asm_dir)
    text = json.dumps(tab, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()

"""DPP wait states, checked in the disassembly of what hipcc built (not a test module; tests/test_isa_hazards_host.py and
tests/test_gpu_parity.py use it).

gfx950 does not interlock a VALU write in front of a DPP read of the same VGPR, and hipcc's hazard recognizer does not look inside
`asm` strings: the hand-written DPP statements of csrc/bcn_dpp.h, ns2d_fast_impl.h and ns2d_fast2_impl.h carry their own pad, or rest
on where the compiler places the code around them.  This module reads the gfx950 code objects of a host shared object
(`llvm-objdump --offloading`, in a temporary directory) or of a device object, disassembles them (`llvm-objdump -t -d`), rebuilds the
control flow of every function from its s_branch / s_cbranch_* (target: the address behind the branch + 4 x simm16) and searches
BACKWARDS from every DPP instruction through all predecessors, loop back-edges included, until the window is used up.

Wait states as LLVM's GCNHazardRecognizer counts them: every instruction is 1, `s_nop N` is N + 1.  The "distance" of a writer is
the number of wait states BETWEEN it and the reader (0: adjacent).  The constants are those of LLVM's checkDPPHazards:

  R1  VALU write of a VGPR -> DPP instruction reading it AS ITS DPP SOURCE (src0): >= DPP_VGPR_WAIT_STATES (2) on every path.
  R2  VALU write of EXEC (v_cmpx*) -> any DPP instruction: >= DPP_EXEC_WAIT_STATES (5).

A VALU writer is every v_* instruction except v_nop, v_readlane / v_readfirstlane and the compares that write SGPRs / VCC only; a
register range v[a:b] writes each of its registers, v_swap both operands, and a DPP instruction is a writer like any other.  Loads
(ds_*, global_*, ...) are no VALU and no writer under R1.  A DPP instruction is one that carries a quad_perm / row_* / wave_* /
row_bcast control.

Where the search cannot see the writer:
  entry   a DPP read inside 2 wait states of the entry of a NON-kernel function (transport_chain_f32 is noinline): the caller's last
          write is unknown.  The entry of a kernel ends a path safely.
  return  the same behind a call (s_swappc_b64 / s_call_b64): the callee's last write is unknown.
Both are findings of their own kind and fail a scan like R1 / R2.

The strict reading.  LLVM applies the 2 states to EVERY VGPR operand of a DPP instruction (its `old` value -- the destination -- and
the accumulator of v_fmac included), not to src0 only.  R1 is restricted to src0 on purpose: the second v_add_f32_dpp of
bcn_dpp::add_above_below reads the first one's result as a plain operand at distance 0, and that path is bit-exact against the
float64 oracle in every test.  Sites that violate ONLY the stricter reading are COUNTED and reported ("strict"), and fail nothing:
whether the hardware needs the wait states for the non-DPP operands is unmeasured.

Nothing else is looked for: two rules, one instruction class.  Run time: a second or two per plugin, 23 s for the library (18 code
objects, 1.2 M lines of disassembly); scan_files() runs one child interpreter per file, at most 8 at a time, that imports neither
torch nor the package.

  python tests/isa_hazards.py [--json] [--objdump PATH] FILE...      # summary (exit status 1 where something was found)"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DPP_VGPR_WAIT_STATES = 2
DPP_EXEC_WAIT_STATES = 5
WINDOW = max(DPP_VGPR_WAIT_STATES, DPP_EXEC_WAIT_STATES)      # how far back a search goes; distances are reported below it

_FUNC = re.compile(r"^([0-9a-fA-F]{8,16}) <(.+)>:\s*$")
_INS = re.compile(r"^\s+([a-z][a-z0-9_]*)\s*(.*?)\s*//\s*([0-9a-fA-F]+):")
_KD = re.compile(r"\s(\S+)\.kd\s*$")
_VGPR = re.compile(r"(?<![A-Za-z0-9_])v(?:\[(\d+):(\d+)\]|(\d+))(?![A-Za-z0-9_\[])")
_DPP_CTRL = re.compile(r"\b(?:quad_perm:|row_(?:shl|shr|ror|bcast|newbcast|share|xmask):|row_(?:half_)?mirror\b|wave_(?:shl|shr|rol|ror):)")
_CBRANCH = re.compile(r"^s_cbranch_(?:scc0|scc1|vccz|vccnz|execz|execnz|cdbgsys|cdbguser|cdbgsys_or_user|cdbgsys_and_user)$")
_NO_VGPR_WRITE = re.compile(r"^v_(?:nop|readlane|readfirstlane|cmp_|cmpx_)")
_END = ("s_endpgm", "s_setpc_b64", "s_endpgm_saved")
_CALL = ("s_swappc_b64", "s_call_b64")


def objdump():
    """llvm-objdump of the ROCm installation whose hipcc builds the kernels (beacon_amd.build.hipcc()), or None."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from beacon_amd import build
    finally:
        sys.path.pop(0)
    cc = build.hipcc()
    if cc is None:
        return None
    for c in (cc, os.path.realpath(cc)):
        root = os.path.dirname(os.path.dirname(c))
        for sub in (("llvm", "bin"), ("lib", "llvm", "bin")):
            p = os.path.join(root, *(sub + ("llvm-objdump",)))
            if os.path.exists(p):
                return p
    return None


def _regs(text):
    out = set()
    for a, b, c in _VGPR.findall(text):
        out.update(range(int(a), int(b) + 1) if a else (int(c),))
    return out


class Ins(object):
    __slots__ = ("addr", "mnem", "text", "ws", "writes", "exec_write", "dpp", "src0", "reads", "flow", "target")

    def __init__(self, addr, mnem, operands):
        self.addr, self.mnem = addr, mnem
        self.text = ("%s %s" % (mnem, operands)).strip()
        ops = [o.strip() for o in operands.split(",")] if operands else []
        self.ws = 1
        if mnem == "s_nop":
            self.ws = int(ops[0], 0) + 1
        valu = mnem.startswith("v_")
        self.writes = frozenset()
        if valu and ops and not _NO_VGPR_WRITE.match(mnem):
            self.writes = frozenset(_regs(ops[0]) | (_regs(ops[1]) if mnem.startswith("v_swap") and len(ops) > 1 else set()))
        self.exec_write = mnem.startswith("v_cmpx")
        self.dpp = bool(valu and _DPP_CTRL.search(operands))
        self.src0, self.reads = frozenset(), frozenset()
        if self.dpp:
            rest = ops[1:]
            while rest and not _regs(rest[0]) and re.match(r"^(vcc|s\d+|s\[\d+:\d+\])$", rest[0]):
                rest = rest[1:]           # the carry-out of v_addc_co_u32_dpp and its kin
            self.src0 = frozenset(_regs(rest[0])) if rest else frozenset()
            self.reads = frozenset(_regs(operands))
        self.flow, self.target = None, None
        if mnem == "s_branch" or _CBRANCH.match(mnem):
            simm = int(ops[0], 0) & 0xFFFF
            self.flow = "branch" if mnem == "s_branch" else "cbranch"
            self.target = addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)
        elif mnem in _END:
            self.flow = "end"
        elif mnem in _CALL:
            self.flow = "call"


def parse(text):
    """objdump -t -d output -> [(function name, is_kernel, [Ins])].  A function is a kernel where the symbol table holds its
    kernel descriptor `<name>.kd`."""
    kernels, funcs, cur = set(), [], None
    for line in text.splitlines():
        if line.startswith("\t") or line.startswith(" "):
            if cur is not None:
                m = _INS.match(line)
                if m:
                    cur.append(Ins(int(m.group(3), 16), m.group(1), m.group(2)))
            continue
        m = _FUNC.match(line)
        if m:
            cur = []
            funcs.append((m.group(2), cur))
            continue
        m = _KD.search(line)
        if m:
            kernels.add(m.group(1))
    return [(name, name in kernels, ins) for name, ins in funcs if ins]


def check_function(name, is_kernel, ins):
    """-> dict(dpp, min, at2, strict, mnems, findings).  `min`: the smallest distance of a VALU writer of a DPP source below WINDOW
    (None: no DPP source is written that close); `at2`: DPP instructions whose nearest such writer sits at exactly 2."""
    index = {i.addr: k for k, i in enumerate(ins)}
    jumps = {}
    for k, i in enumerate(ins):
        if i.target is not None and i.target in index:
            jumps.setdefault(index[i.target], []).append(k)
    out = dict(dpp=0, min=None, at2=0, strict=0, mnems={}, findings=[])

    def finding(kind, reader, writer, d):
        out["findings"].append(dict(kind=kind, function=name, address="0x%x" % reader.addr, writer=writer, reader=reader.text, distance=d))

    for k, r in enumerate(ins):
        if not r.dpp:
            continue
        out["dpp"] += 1
        out["mnems"][r.mnem] = out["mnems"].get(r.mnem, 0) + 1
        nearest, r1, strict = None, False, False
        seen, todo = {}, [(k, 0)]
        while todo:
            pos, d = todo.pop()
            if seen.get(pos, WINDOW) <= d:
                continue
            seen[pos] = d
            if pos == 0 and not is_kernel and d < DPP_VGPR_WAIT_STATES:
                finding("entry", r, "(entry of a non-kernel function: the caller's last write is unknown)", d)
            preds = list(jumps.get(pos, ()))
            if pos > 0 and ins[pos - 1].flow not in ("branch", "end"):
                preds.append(pos - 1)
            for p in preds:
                w = ins[p]
                if w.flow == "call":
                    if d < DPP_VGPR_WAIT_STATES:
                        finding("return", r, w.text + "  (the callee's last write is unknown)", d)
                    continue
                if w.writes & r.src0:
                    nearest = d if nearest is None else min(nearest, d)
                    if d < DPP_VGPR_WAIT_STATES:
                        r1 = True
                        finding("R1", r, "0x%x  %s" % (w.addr, w.text), d)
                elif w.writes & r.reads and d < DPP_VGPR_WAIT_STATES:
                    strict = True
                if w.exec_write and d < DPP_EXEC_WAIT_STATES:
                    finding("R2", r, "0x%x  %s" % (w.addr, w.text), d)
                if d + w.ws < WINDOW:
                    todo.append((p, d + w.ws))
        if nearest is not None:
            out["min"] = nearest if out["min"] is None else min(out["min"], nearest)
            out["at2"] += nearest == DPP_VGPR_WAIT_STATES
        out["strict"] += strict and not r1
    return out


def check_text(text):
    """Disassembly text -> {function name: check_function()} for the functions that hold a DPP instruction."""
    res = {}
    for name, is_kernel, ins in parse(text):
        c = check_function(name, is_kernel, ins)
        if c["dpp"]:
            key, n = name, 1
            while key in res:           # the same (anonymous-namespace) name in another code object of the file
                n += 1
                key = "%s #%d" % (name, n)
            res[key] = c
    return res


def assemble(src):
    """A few lines of hand-written assembly -> text in objdump's layout, for the tests of the checker itself.  `.kernel NAME` /
    `.func NAME` open a function, `LABEL:` names the next instruction, a branch may name a label; every instruction takes 4 bytes."""
    lines, labels, addr = [], {}, 0x100
    for raw in src.strip().splitlines():
        s = raw.strip()
        if not s:
            continue
        if s.startswith(".kernel ") or s.startswith(".func "):
            addr = (addr + 0xFF) // 0x100 * 0x100
            lines.append((s.split()[0], s.split()[1], addr))
        elif s.endswith(":"):
            labels[s[:-1]] = addr
        else:
            lines.append(("ins", s, addr))
            addr += 4
    out = ["SYMBOL TABLE:"] + ["%016x g     O .rodata\t0000000000000040 %s.kd" % (a, n) for k, n, a in lines if k == ".kernel"]
    out += ["", "Disassembly of section .text:"]
    for kind, s, a in lines:
        if kind != "ins":
            out += ["", "%016x <%s>:" % (a, s)]
            continue
        mnem, _, ops = s.partition(" ")
        if (mnem == "s_branch" or _CBRANCH.match(mnem)) and ops.strip() in labels:
            ops = str(((labels[ops.strip()] - a - 4) // 4) & 0xFFFF)
        out.append("\t%-58s // %012X: 00000000" % ((mnem + " " + ops).strip(), a))
    return "\n".join(out) + "\n"


def _is_amdgpu_elf(path):
    with open(path, "rb") as fh:
        h = fh.read(20)
    return h[:4] == b"\x7fELF" and len(h) == 20 and h[18] | (h[19] << 8) == 224       # EM_AMDGPU


def scan_file(path, tool):
    """One host shared object (its gfx950 code objects) or one device object -> report dict."""
    rep = dict(file=os.path.basename(path), code_objects=0, functions={})
    with tempfile.TemporaryDirectory() as tmp:
        if _is_amdgpu_elf(path):
            objs = [path]
        else:
            name = os.path.basename(path)
            shutil.copyfile(path, os.path.join(tmp, name))      # the bundles are written next to the input: keep the tree clean
            subprocess.run([tool, "--offloading", name], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
            objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f != name and "amdgcn" in f and os.path.getsize(os.path.join(tmp, f)))
        for o in objs:
            text = subprocess.run([tool, "-t", "-d", o], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
            rep["code_objects"] += 1
            for fn, c in check_text(text).items():
                key, n = fn, 1
                while key in rep["functions"]:
                    n += 1
                    key = "%s #%d" % (fn, n)
                rep["functions"][key] = c
    return summarise(rep)


def summarise(rep):
    f = rep["functions"].values()
    mins = [c["min"] for c in f if c["min"] is not None]
    rep.update(dpp=sum(c["dpp"] for c in f), min=min(mins) if mins else None, at2=sum(c["at2"] for c in f),
               strict=sum(c["strict"] for c in f), findings=[x for c in f for x in c["findings"]], mnems={})
    for c in f:
        for m, n in c["mnems"].items():
            rep["mnems"][m] = rep["mnems"].get(m, 0) + n
    return rep


def scan_files(paths, tool=None, jobs=8):
    """[report] in the order of `paths`: one child interpreter per file (this file as a program), at most min(jobs, 8) at a time.
    The children import neither torch nor beacon_amd and open no GPU."""
    tool = tool or objdump()
    if tool is None:
        raise RuntimeError("llvm-objdump not found next to hipcc")

    def one(p):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--objdump", tool, p], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, universal_newlines=True)
        if r.returncode not in (0, 1):
            raise RuntimeError("scan of %s failed: %s" % (p, r.stderr[-2000:]))
        return json.loads(r.stdout)[0]

    with ThreadPoolExecutor(max_workers=max(1, min(jobs, 8))) as ex:
        return list(ex.map(one, paths))


def format_finding(file, x):
    return "%s: %s in %s at %s, distance %d: writer [%s] reader [%s]" % (file, x["kind"], x["function"], x["address"], x["distance"],
                                                                        x["writer"], x["reader"])


def format_summary(reports, functions=False):
    """Markdown table: per artifact the DPP count, the smallest distance, the count at exactly 2, the strict-reading count, findings."""
    rows = ["| artifact | code objects | DPP instructions | smallest distance | at exactly 2 | strict reading only | findings |",
            "|---|---|---|---|---|---|---|"]
    for r in reports:
        rows.append("| %s | %d | %d | %s | %d | %d | %d |" % (r["file"], r["code_objects"], r["dpp"], "-" if r["min"] is None else r["min"],
                                                              r["at2"], r["strict"], len(r["findings"])))
        if functions:
            for fn, c in sorted(r["functions"].items()):
                rows.append("| &nbsp;&nbsp;`%s` | | %d | %s | %d | %d | %d |" % (fn, c["dpp"], "-" if c["min"] is None else c["min"], c["at2"],
                                                                              c["strict"], len(c["findings"])))
    return "\n".join(rows)


def all_findings(reports):
    return [format_finding(r["file"], x) for r in reports for x in r["findings"]]


def main(argv):
    as_json, tool, files = False, None, []
    it = iter(argv)
    for a in it:
        if a == "--json":
            as_json = True
        elif a == "--objdump":
            tool = next(it)
        else:
            files.append(a)
    tool = tool or objdump()
    reps = [scan_file(f, tool) for f in files]
    if as_json:
        json.dump(reps, sys.stdout)
    else:
        print(format_summary(reps, functions=True))
        for line in all_findings(reps):
            print(line)
    return 1 if any(r["findings"] for r in reps) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

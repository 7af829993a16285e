"""The DPP wait-state scan (tests/isa_hazards.py) and what it guards, on the CPU: no test here needs a GPU or loads a kernel.

  1. the checker itself on hand-written disassembly snippets (no compiler involved);
  2. every hand-written instruction under beacon_amd/csrc is one somebody decided the hazard rules of (an allow-list);
  3. libbeacon_hip.so and every plugin in beacon_amd/_jit/: zero R1 / R2 violations, zero entry / return findings -- with proof
     that the scan saw the hand-written DPP sites;
  4. the pad of transport_chain_f32 (BCN_CHAIN_NOP) is tested, not trusted: the 75x50 float32 rayleigh unit compiled as it is
     (clean) and with the pad removed (flagged, inside transport_chain_f32 only).

Run time of the whole file, measured on 8 cores: 50 s (1 and 2: under 2 s; 3: 33 s -- the library's 18 code objects are 23 s of
one child process, the 105 plugins run beside it in 7 more; 4: 13 s, two 10 s compilations side by side)."""
import glob
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import isa_hazards as H
from conftest import ROOT

CSRC = os.path.join(ROOT, "beacon_amd", "csrc")
DPP = " wave_shr:1 row_mask:0xf bank_mask:0xf"


def _tool():
    tool = H.objdump()
    if tool is None:
        pytest.skip("no llvm-objdump next to hipcc (beacon_amd.build.hipcc()): nothing to disassemble with")
    return tool


# ---- 1. the checker on hand-written snippets ----------------------------------------------------------------------------------
# (name, assembly, expected findings as (kind, distance) in any order, expected strict-only count)
K = ".kernel k\n v_mov_b32 v9, 0\n s_nop 7\n"          # a kernel whose entry is far from everything
SNIPPETS = [
    ("distance 0 is flagged", K + "v_add_f32 v1, v2, v3\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 0)], 0),
    ("distance 1 is flagged", K + "v_add_f32 v1, v2, v3\n v_mov_b32 v7, 0\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 1)], 0),
    ("distance 2 passes", K + "v_add_f32 v1, v2, v3\n v_mov_b32 v7, 0\n v_mov_b32 v8, 0\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("s_nop 0 counts 1", K + "v_add_f32 v1, v2, v3\n s_nop 0\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 1)], 0),
    ("s_nop 1 counts 2", K + "v_add_f32 v1, v2, v3\n s_nop 1\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("an SALU instruction counts 1", K + "v_add_f32 v1, v2, v3\n s_add_i32 s0, s1, 2\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 1)], 0),
    ("two SALU instructions count 2", K + "v_add_f32 v1, v2, v3\n s_add_i32 s0, s1, 2\n s_mov_b32 s3, 0\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("the writer is a DPP instruction itself", K + "s_nop 1\n v_add_f32_dpp v1, v2, v3" + DPP + "\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 0)], 0),
    ("a 64-bit write overlaps the source (high half)", K + "v_pk_fma_f32 v[26:27], v[0:1], v[2:3], v[6:7]\n v_fmac_f32_dpp v4, v27, v5" + DPP, [("R1", 0)], 0),
    ("a 64-bit write next to the source", K + "v_pk_fma_f32 v[26:27], v[0:1], v[2:3], v[6:7]\n v_fmac_f32_dpp v4, v28, v5" + DPP, [], 0),
    ("v_swap writes both operands", K + "v_swap_b32 v1, v2\n v_add_f32_dpp v4, v2, v5" + DPP, [("R1", 0)], 0),
    ("ds_read is no VALU writer", K + "ds_read_b32 v1, v2\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("global_load is no VALU writer", K + "global_load_dword v1, v[2:3], off\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("v_readlane and a VCC compare write no VGPR", K + "v_readlane_b32 s1, v1, 3\n v_cmp_lt_f32_e32 vcc, v1, v2\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("a plain (src1) read at distance 0 passes, strict counts it", K + "v_add_f32 v5, v2, v3\n v_add_f32_dpp v4, v1, v5" + DPP, [], 1),
    ("the accumulator of v_fmac at distance 0: strict only", K + "v_add_f32 v4, v2, v3\n v_fmac_f32_dpp v4, v1, v5" + DPP, [], 1),
    ("bcn_dpp::add_above_below: the second add reads the first one's result as src1", K + "v_mov_b32 v2, 0\n s_nop 1\n"
     " v_add_f32_dpp v0, v2, v3 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
     " v_add_f32_dpp v1, v2, v0 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", [], 1),
    ("across a fall-through label", K + "s_cbranch_scc1 L\n v_mov_b32 v7, 0\n v_add_f32 v1, v2, v3\nL:\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 0)], 0),
    ("across a taken branch", K + "v_add_f32 v1, v2, v3\n s_cbranch_scc1 L\n v_mov_b32 v7, 0\n v_mov_b32 v8, 0\n s_nop 3\nL:\n v_add_f32_dpp v4, v1, v5" + DPP,
     [("R1", 1)], 0),
    ("across an unconditional branch", K + "v_add_f32 v1, v2, v3\n s_branch L\n s_endpgm\nL:\n v_add_f32_dpp v4, v1, v5" + DPP, [("R1", 1)], 0),
    ("nothing falls through an unconditional branch", K + "s_cbranch_scc1 L\n v_add_f32 v1, v2, v3\n s_branch E\nL:\n v_add_f32_dpp v4, v1, v5" + DPP + "\nE:\n s_endpgm",
     [], 0),
    ("around a loop back-edge: writer last in the body, reader first", K + "L:\n v_add_f32_dpp v4, v1, v5" + DPP + "\n s_nop 3\n v_add_f32 v1, v4, v3\n s_cbranch_scc1 L\n s_endpgm",
     [("R1", 1)], 0),
    ("around a loop back-edge with the pad behind the writer", K + "L:\n v_add_f32_dpp v4, v1, v5" + DPP + "\n s_nop 3\n v_add_f32 v1, v4, v3\n s_nop 0\n s_cbranch_scc1 L\n s_endpgm",
     [], 0),
    ("one of two predecessors only", K + "s_cbranch_scc1 A\n v_mov_b32 v1, 0\n s_nop 1\n s_branch J\nA:\n v_mov_b32 v1, 1\nJ:\n v_add_f32_dpp v4, v1, v5" + DPP,
     [("R1", 0)], 0),
    ("both predecessors padded", K + "s_cbranch_scc1 A\n v_mov_b32 v1, 0\n s_nop 1\n s_branch J\nA:\n v_mov_b32 v1, 1\n s_nop 1\nJ:\n v_add_f32_dpp v4, v1, v5" + DPP,
     [], 0),
    ("v_cmpx at 4 states is flagged", K + "v_cmpx_lt_f32_e32 vcc, v8, v9\n s_nop 3\n v_add_f32_dpp v4, v1, v5" + DPP, [("R2", 4)], 0),
    ("v_cmpx at 5 states passes", K + "v_cmpx_lt_f32_e32 vcc, v8, v9\n s_nop 4\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("an SALU write of EXEC is not R2's business", K + "s_and_saveexec_b64 s[0:1], vcc\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("inside 2 states of a non-kernel function's entry", ".func f\n s_waitcnt vmcnt(0)\n v_add_f32_dpp v4, v1, v5" + DPP + "\n s_setpc_b64 s[30:31]", [("entry", 1)], 0),
    ("2 states behind a non-kernel function's entry", ".func f\n s_waitcnt vmcnt(0)\n s_nop 0\n v_add_f32_dpp v4, v1, v5" + DPP + "\n s_setpc_b64 s[30:31]", [], 0),
    ("the entry of a kernel ends a path safely", ".kernel k\n v_add_f32_dpp v4, v1, v5" + DPP + "\n s_endpgm", [], 0),
    ("directly behind a call", K + "s_swappc_b64 s[30:31], s[4:5]\n v_add_f32_dpp v4, v1, v5" + DPP, [("return", 0)], 0),
    ("2 states behind a call", K + "s_swappc_b64 s[30:31], s[4:5]\n s_nop 1\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("a function does not see the one in front of it", ".kernel a\n s_nop 7\n v_add_f32 v1, v2, v3\n.kernel k\n v_add_f32_dpp v4, v1, v5" + DPP, [], 0),
    ("quad_perm and row_shr are DPP controls too", K + "v_mov_b32 v1, 0\n v_mov_b32_dpp v4, v1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n s_nop 1\n"
     " v_mov_b32 v2, 0\n v_add_f32_dpp v6, v2, v2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", [("R1", 0), ("R1", 0)], 0),
    ("the carry-out is not the DPP source", K + "v_mov_b32 v2, 0\n v_addc_co_u32_dpp v1, vcc, v2, v3, vcc" + DPP, [("R1", 0)], 0),
    ("SDWA and plain VALU read anything at distance 0", K + "v_add_f32 v1, v2, v3\n v_add_f32_sdwa v4, v1, v5 dst_sel:DWORD src0_sel:WORD_1 src1_sel:DWORD\n v_add_f32 v6, v4, v1", [], 0),
]


@pytest.mark.parametrize("case", SNIPPETS, ids=[c[0] for c in SNIPPETS])
def test_checker_on_hand_written_snippets(case):
    name, src, want, strict = case
    res = H.check_text(H.assemble(src))
    got = sorted((x["kind"], x["distance"]) for c in res.values() for x in c["findings"])
    assert got == sorted(want), (name, [c["findings"] for c in res.values()])
    assert sum(c["strict"] for c in res.values()) == strict, name
    for c in res.values():
        for x in c["findings"]:       # a finding names function, address, writer and reader
            assert x["function"] in ("k", "f") and x["address"].startswith("0x") and "dpp" in x["reader"] and x["writer"]


def test_checker_reports_counts_and_distances():
    """Per function: the number of DPP instructions, the smallest distance of a writer of a DPP source, how many sit at exactly 2."""
    src = (K + "v_mov_b32 v1, 0\n s_nop 1\n v_add_f32_dpp v4, v1, v5" + DPP +                 # 2
           "\n v_mov_b32 v2, 0\n s_nop 2\n v_add_f32_dpp v6, v2, v5" + DPP +                  # 3
           "\n v_mov_b32 v3, 0\n s_nop 0\n s_nop 0\n v_fmac_f32_dpp v7, v3, v5" + DPP +       # 2
           "\n s_nop 7\n v_add_f32_dpp v8, v3, v5" + DPP + "\n s_endpgm")                     # beyond the window
    res = H.check_text(H.assemble(src))
    assert list(res) == ["k"]
    c = res["k"]
    assert (c["dpp"], c["min"], c["at2"], c["strict"], c["findings"]) == (4, 2, 2, 0, [])
    assert c["mnems"] == {"v_add_f32_dpp": 3, "v_fmac_f32_dpp": 1}
    rep = H.summarise(dict(file="x", code_objects=1, functions=res))
    assert (rep["dpp"], rep["min"], rep["at2"], rep["strict"], rep["findings"]) == (4, 2, 2, 0, [])
    assert "| x | 1 | 4 | 2 | 2 | 0 | 0 |" in H.format_summary([rep])


def test_branch_targets_are_the_address_behind_the_branch_plus_4_simm16():
    """objdump prints simm16 unsigned (s_cbranch_execnz 65507 is 29 instructions BACK): the same arithmetic on real output."""
    text = ("0000000000009200 <f>:\n"
            "\tv_add_f32_dpp v4, v1, v5 wave_shr:1 row_mask:0xf bank_mask:0xf// 000000009200: 00000000 00000000\n"
            "\ts_nop 3                                                    // 000000009208: BF800003\n"
            "\tv_add_f32_e32 v1, v2, v3                                   // 00000000920C: 00000000\n"
            "\ts_cbranch_execnz 65531                                     // 000000009210: BF89FFFB <f+0x0>\n"
            "\ts_endpgm                                                   // 000000009214: BF810000\n")
    (name, is_kernel, ins), = H.parse(text)
    assert not is_kernel and ins[3].target == 0x9200 and ins[1].ws == 4 and ins[0].dpp and ins[0].src0 == {1} and ins[2].writes == {1}
    kinds = sorted((x["kind"], x["distance"]) for x in H.check_function(name, is_kernel, ins)["findings"])
    assert kinds == [("R1", 1), ("entry", 0)]


# ---- 2. no unknown hand-written instruction -------------------------------------------------------------------------------------
# what is allowed and nothing else: the pads, the waits, the DPP adds / fmac of bcn_dpp.h and the transport chains with the plain VALU
# of jacobi_cell_eq, and "" -- the empty statements that only fence the compiler
ALLOWED_ASM = {"", "s_nop", "s_waitcnt", "v_add_f32", "v_add_f32_dpp", "v_fma_f32", "v_fmac_f32_dpp"}
_STR = r'"(?:[^"\\\n]|\\.)*"'


def asm_mnemonics(extra_defines=None):
    """{mnemonic: [file:line, ...]} of every asm(...) / asm volatile(...) statement under beacon_amd/csrc; string macros such as
    BCN_CHAIN_NOP are resolved from their #define ("" for an empty statement)."""
    files = [os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs if f.endswith((".h", ".hip", ".inc", ".cpp")) and "_obj" not in d]
    text = {f: open(f).read().replace("\\\n", " \n") for f in files}
    macros = dict(extra_defines or {})
    for t in text.values():
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+((?:%s[ \t]*)+)$" % _STR, t, re.M):
            macros.setdefault(m.group(1), "".join(s[1:-1] for s in re.findall(_STR, m.group(2))))
    out = {}
    for f, t in sorted(text.items()):
        for m in re.finditer(r"\b(?:asm|__asm__|__asm)\b\s*(?:volatile\b|__volatile__\b)?\s*\(", t):
            pos, tmpl = m.end(), ""
            while True:
                tok = re.compile(r"\s*(%s|\w+)" % _STR).match(t, pos)
                if not tok:
                    break
                s = tok.group(1)
                assert s.startswith('"') or s in macros, "%s: asm template token %r is neither a string nor a known string macro" % (f, s)
                tmpl += s[1:-1] if s.startswith('"') else macros[s]
                pos = tok.end()
            where = "%s:%d" % (os.path.relpath(f, ROOT), t.count("\n", 0, m.start()) + 1)
            lines = [l.strip() for l in re.split(r"\\n|;", tmpl.replace("\\t", " ")) if l.strip()]
            for l in lines or [""]:
                out.setdefault(l.split()[0] if l else "", []).append(where)
    return out


def test_every_hand_written_instruction_is_on_the_allow_list():
    found = asm_mnemonics()
    unknown = {k: v for k, v in found.items() if k not in ALLOWED_ASM}
    assert not unknown, ("hand-written instructions nobody has decided the hazard rules of (tests/isa_hazards.py checks the two DPP rules "
                         "only): %s" % unknown)
    # the collector sees the statements this is about: both DPP forms, the pads, the fences -- and the macro resolved
    assert {"v_add_f32_dpp", "v_fmac_f32_dpp", "s_nop", ""} <= set(found)
    sites = lambda k, name: [w for w in found[k] if name in w]
    assert len(sites("v_add_f32_dpp", "bcn_dpp.h")) == 6 and len(sites("v_fmac_f32_dpp", "ns2d_fast_impl.h")) == 1
    assert len(sites("v_fmac_f32_dpp", "ns2d_fast2_impl.h")) == 2
    assert len(sites("s_nop", "ns2d_fast_impl.h")) == 1                      # BCN_CHAIN_NOP, from its #define
    assert not [w for w in asm_mnemonics({"BCN_CHAIN_NOP": ""}).get("s_nop", []) if "ns2d_fast_impl.h" in w]


# ---- 3. everything that is built -------------------------------------------------------------------------------------------------
def _report(reports):
    print()
    print(H.format_summary(reports))
    for line in H.all_findings(reports):
        print(line)


def test_nothing_that_is_built_holds_a_dpp_hazard(monkeypatch):
    """libbeacon_hip.so and every beacon_amd/_jit/*.so (after __graft_entry__.build(): every plugin the GPU tests load), read as
    files: nothing is loaded into this process."""
    from beacon_amd import build, jit
    tool = _tool()
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    lib = build.build_lib()
    plugins = sorted(glob.glob(os.path.join(jit.JIT_DIR, "*.so")))
    reports = H.scan_files([lib] + plugins, tool)
    _report(reports)
    assert not H.all_findings(reports)
    # not vacuous: the scan saw the hand-written sites
    libr = reports[0]
    assert libr["code_objects"] >= 6 and libr["dpp"] > 10000
    for m in ALLOWED_ASM:
        if m.endswith("_dpp"):
            assert libr["mnems"].get(m, 0) > 0, m
    chains = [c for fn, c in libr["functions"].items() if "transport_chain_f32" in fn]
    assert chains and all(c["mnems"].get("v_fmac_f32_dpp", 0) > 0 for c in chains)
    assert libr["min"] is not None and libr["min"] >= H.DPP_VGPR_WAIT_STATES and libr["at2"] > 0      # the margin is zero somewhere
    if os.path.isdir(jit.JIT_DIR):
        assert len(plugins) >= len(jit.TEST_GRIDS) + len(jit.EXTRA_BUILDS)
        by_name = {r["file"]: r for r in reports[1:]}
        monkeypatch.setenv("BEACON_NO_BUILD", "1")           # (names only: nothing is compiled here)
        rows4 = [g for g in jit.TEST_GRIDS if jit.choose(*g)["rows"] == 4][0]
        want = [(g, dict(jit.PRM_DEFS)) for g in jit.PRM_TEST_GRIDS] + [(rows4, None)]
        for g, defs in want:
            p = jit.build_plugin(g[0], g[1], g[2], g[3], extra_defs=defs)
            assert p is not None and os.path.basename(p) in by_name, (g, defs)
            assert by_name[os.path.basename(p)]["dpp"] > 0, (g, defs)
        assert all(r["dpp"] > 0 for r in reports[1:])


# ---- 4. the pad is tested, not trusted -----------------------------------------------------------------------------------------
def test_removing_the_chain_pad_is_flagged_in_transport_chain_f32(tmp_path):
    """csrc/jit/ns2d_jit.hip for the 75x50 float32 rayleigh grid, device only, with the -D set and the flags of jit.build_plugin:
    clean as it is; with -DBCN_CHAIN_NOP= (the pad of ns2d_fast_impl.h's chain step removed) the scan names transport_chain_f32."""
    from beacon_amd import build, jit
    tool, cc = _tool(), build.hipcc()
    nx, ny, f64, kind = 75, 50, False, 0
    m = jit.choose(nx, ny, f64, kind)
    assert (m["rows"], m["R"], m["gf"]) == (1, 10, 0)
    defs = {"BCN_JIT_ROWS": m["rows"], "BCN_JIT_REAL": "float", "BCN_JIT_NX": nx, "BCN_JIT_NY": ny, "BCN_JIT_R": m["R"],
            "BCN_JIT_KIND": kind, "BCN_JIT_GF": m["gf"]}

    def compile_and_scan(tag, extra):
        obj = str(tmp_path / (tag + ".co"))
        subprocess.check_call(build.compile_cmd(jit.JIT_SRC, obj, build.JIT_FLAGS, defs, extra,
                                                mode=("--offload-device-only", "--no-gpu-bundle-output", "-c")))
        return H.scan_file(obj, tool)

    with ThreadPoolExecutor(max_workers=2) as ex:
        clean, bare = ex.map(lambda a: compile_and_scan(*a), [("as_is", []), ("no_pad", ["-DBCN_CHAIN_NOP="])])
    _report([clean, bare])
    assert clean["dpp"] > 1000 and not clean["findings"], H.all_findings([clean])
    assert any("transport_chain_f32" in fn and c["mnems"].get("v_fmac_f32_dpp") for fn, c in clean["functions"].items())
    if not bare["findings"]:
        pytest.xfail("this compiler keeps >= 2 wait states in front of the chain's DPP step without the pad (smallest distance %s): "
                     "the red half of the pair no longer exists, the scan of the built tree is the only guard" % bare["min"])
    assert all(x["kind"] == "R1" and "transport_chain_f32" in x["function"] for x in bare["findings"]), H.all_findings([bare])
    assert all("v_fmac_f32_dpp" in x["reader"] for x in bare["findings"])

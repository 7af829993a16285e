"""The plain double-sweep loop of the headline kernel, read in the compiler's own assembly (no GPU, one compile).

csrc/ns2d_fast_runs.hip is compiled to assembly with beacon_amd.build's flags, device only, the way scripts/valu_model.py does;
ns2d_fast_sched<float,128,64,16,0,true,0> holds the plain double sweep -- 2 x (16 + 1) cells, no reduction -- as its innermost loops
with 68 DPP adds (hipcc emits two copies: the opening of a solve and the skips between evaluations).  Each cell is six hand-written
instructions (v_add_f32, s_nop 1, 2 x v_add_f32_dpp, 2 x v_fma_f32: bcn_dpp.h); csrc/bcn_jacobi_cells.h states the 34 cells of a
double sweep in EIGHT asm statements (7 + 7 interior, the 4 halo-dependent, the 4 exchanged, 6 + 6 interior), so what can be derived is:

  * 170 cell instructions (34 v_add_f32 + 68 v_add_f32_dpp + 68 v_fma_f32) and exactly 34 `s_nop 1`, one per cell;
  * at most 7 other s_nop: hipcc pads one wait state behind an asm statement that another one follows directly, and eight statements
    have seven places in between;
  * no v_mov_b32 from an SGPR: cx goes to the final v_fma_f32 of a cell as a scalar operand;
  * at most 170 + 7 vector instructions: the cells, the four selects on the wave-uniform wall conditions (xw1, xe1, yw, ye) and the
    three exchange addresses -- the wave-class copies of the loop and the addresses kept live were measured and left out, DESIGN.md 6 ("slot by slot");
  * nothing spilled inside the loop."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

KERNEL = "ns2d_fast_schedIfLi128ELi64ELi16ELi0ELb1ELi0EE"
CELLS = 2 * (16 + 1)


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    from beacon_amd import build as B
    cc = B.hipcc()
    if cc is None:
        pytest.skip("no hipcc: nothing to compile with")
    asm = str(tmp_path_factory.mktemp("jacobi_loop") / "ns2d_fast.s")
    subprocess.check_call(B.compile_cmd(os.path.join(B.CSRC, "ns2d_fast_runs.hip"), asm, mode=("--cuda-device-only", "-S")))
    with open(asm) as fh:
        s = fh.read()
    m = re.search(r'^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end' % KERNEL, s, re.S | re.M)
    assert m, "kernel %s not in the assembly" % KERNEL
    lines = [l.strip() for l in m.group(2).split("\n")]
    lines = [l for l in lines if l and not l.startswith(";") and not (l.startswith(".") and not l.startswith(".LBB"))]
    labels = {mm.group(1): i for i, l in enumerate(lines) for mm in [re.match(r'(\.LBB\d+_\d+):', l)] if mm}
    out = []
    for i, l in enumerate(lines):
        mm = re.match(r's_cbranch_\w+ (\.LBB\d+_\d+)|s_branch (\.LBB\d+_\d+)', l)
        t = mm and (mm.group(1) or mm.group(2))
        if t and t in labels and labels[t] < i:
            body = lines[labels[t] + 1:i + 1]
            if any(re.match(r's_cbranch|s_branch', b) for b in body[:-1]):
                continue                                   # not innermost
            if sum("_dpp" in b for b in body) == 2 * CELLS and sum(b.startswith("ds_") for b in body) <= 8:
                out.append((t, body))
    assert out, "no innermost loop with %d DPP adds and no reduction: the plain double sweep" % (2 * CELLS)
    return out


def _count(body, pattern):
    return sum(bool(re.match(pattern, b)) for b in body)


def test_the_plain_double_sweep_is_its_cells_and_little_else(loops):
    for label, body in loops:
        n = dict(add=_count(body, r'v_add_f32(_e32|_e64)? '), dpp=_count(body, r'v_add_f32_dpp '), fma=_count(body, r'v_fma_f32 '),
                 nop1=_count(body, r's_nop 1$'), nop=_count(body, r's_nop '), valu=_count(body, r'v_'),
                 mov_s=_count(body, r'v_mov_b32\w* v\d+, s\d+'),
                 spill=_count(body, r'(scratch_|buffer_(load|store)|v_readlane|v_writelane|v_accvgpr)'))
        print(label, len(body), "instructions", n)
        assert (n["add"], n["dpp"], n["fma"]) == (CELLS, 2 * CELLS, 2 * CELLS), (label, n)
        assert n["add"] + n["dpp"] + n["fma"] == 170
        assert n["nop1"] == CELLS, (label, n)                       # the in-cell wait state, one per cell
        assert n["nop"] - n["nop1"] <= 7, (label, n)                # eight statements
        assert n["mov_s"] == 0, (label, [b for b in body if re.match(r'v_mov_b32\w* v\d+, s\d+', b)])
        assert n["valu"] <= 170 + 7, (label, n, [b for b in body if b.startswith("v_") and not re.match(r'v_(add_f32|fma_f32)', b)])
        assert n["spill"] == 0, (label, n)


def test_the_halo_dependent_cells_stay_behind_the_interior_ones(loops):
    """The first LDS wait of a trip (the halos requested behind the previous barrier) sits behind the 14 interior cells of the first
    sweep, and the barrier behind the first run of the second sweep's inner columns: 14 + 4 + 4 + 6 = 28 cells in front of it."""
    for label, body in loops:
        cells_before = lambda k: sum(b.startswith("v_add_f32_dpp") for b in body[:k]) // 2
        waits = [k for k, b in enumerate(body) if b.startswith("s_waitcnt") and "lgkmcnt" in b]
        bars = [k for k, b in enumerate(body) if b.startswith("s_barrier")]
        assert waits and len(bars) == 1, (label, waits, bars)
        assert cells_before(waits[0]) == 14, (label, cells_before(waits[0]))
        assert cells_before(bars[0]) == 28, (label, cells_before(bars[0]))

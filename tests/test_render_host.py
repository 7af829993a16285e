"""CPU-side checks of the device frames (VecEnv.renderer, bcn_render; csrc/render.hip): the default colour table, the NumPy
restatement of the pixel rules (tests/render_ref.py) against matplotlib's own colour mapping and against examples worked by hand,
the entry points through the host layers, and the Python layer's argument errors -- none of which needs a GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import render_ref as R
from conftest import ROOT

DT = {"f32": np.float32, "f64": np.float64}


def test_default_table():
    from beacon_amd.render import colormap_lut
    lut = colormap_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (5, 48, 97) and tuple(lut[255]) == (103, 0, 31)
    assert np.array_equal(lut, colormap_lut())
    mpl = pytest.importorskip("matplotlib")
    ref = mpl.colormaps["RdBu_r"](np.arange(256), bytes=True)[:, :3]
    d = np.abs(lut.astype(int) - ref.astype(int))
    print("entries that differ from matplotlib's RdBu_r: %d of 768, by at most %d" % (int((d > 0).sum()), int(d.max())))
    assert d.max() <= 1


def _value_set(vmin, vmax, dtype):
    """2 000 000 seeded values reaching beyond the range on both sides, the 257 bin edges and both neighbours of each"""
    rng = np.random.default_rng(20240)
    span = vmax - vmin
    v = rng.uniform(vmin - 0.1 * span, vmax + 0.1 * span, 2_000_000).astype(dtype)
    edges = (vmin + np.arange(257) / 256.0 * span).astype(dtype)
    return np.concatenate([v, edges, np.nextafter(edges, dtype(-np.inf)), np.nextafter(edges, dtype(np.inf))])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("vmin,vmax", [(-0.5, 0.5), (0.0, 1.0)])
def test_colour_rule_equals_matplotlib(vmin, vmax, dtype):
    mpl = pytest.importorskip("matplotlib")
    from matplotlib.colors import Normalize
    cmap = mpl.colormaps["RdBu_r"]
    table = cmap(np.arange(256), bytes=True)[:, :3]
    v = _value_set(vmin, vmax, DT[dtype])
    assert v.size == 2_000_771 and v.dtype == DT[dtype]
    want = cmap(Normalize(vmin, vmax)(v), bytes=True)[:, :3]
    got = R.colorize(v, vmin, vmax, table, DT[dtype])
    bad = int((got != want).any(axis=1).sum())
    print("%s (%g, %g): %d mismatches of %d" % (dtype, vmin, vmax, bad, v.size))
    assert bad == 0


def test_field_panel_orientation_and_nan():
    lut = np.zeros((256, 3), np.uint8)
    lut[:, 0] = np.arange(256)
    nx, ny, s = 5, 3, 2
    plane = np.zeros((ny + 2, nx + 2), np.float32)
    plane[3, 2] = 1.0                 # cell i = 2, j = 3: the top row of a 3-row domain, second column
    plane[1, 5] = np.nan              # cell i = 5, j = 1: bottom row, last column
    plane[0, :] = 0.7                 # ghost cells never show
    img = R.field_panel(plane, s, 0.0, 1.0, lut, np.float32)
    assert img.shape == (ny * s, nx * s, 3)
    want = np.zeros((ny * s, nx * s), int)
    want[0:2, 2:4] = 255              # r // 2 = 0 -> j = 3; c // 2 = 1 -> i = 2
    assert np.array_equal(img[..., 0], want)
    img[..., 0] = 1                   # the NaN cell is black in every channel, whatever the table holds at index 0
    lut[:] = 9
    img = R.field_panel(plane, s, 0.0, 1.0, lut, np.float32)
    assert (img[4:6, 8:10] == 0).all() and (img[0:4] == 9).all() and (img[4:6, 0:8] == 9).all()


def test_colour_index_edges():
    for dt in (np.float32, np.float64):
        idx = R.color_index([-1.0, 0.0, 1.0 / 256, 0.5, 255.0 / 256, np.nextafter(dt(1), dt(0)), 1.0, 2.0, np.inf, -np.inf, np.nan], 0.0, 1.0, dt)
        assert idx.tolist() == [0, 0, 1, 128, 255, 255, 255, 255, 255, 0, -1]


def test_line_panel_joins_a_step_and_marks_non_finite_columns():
    # two samples, two columns, H = 8 over (0, 1): y = 0.95 -> row int(0.05 * 8) = 0; y = 0.05 -> row int(0.95 * 8) = 7
    img = R.line_panel([0.95, 0.05], 2, 8, 0.0, 1.0, 0.5, np.float64)
    assert (img[:, 0] == R.BLUE).all()                     # column 0 covers samples 0 .. 1: the step is joined over all rows
    col1 = img[:, 1]
    assert (col1[7] == R.BLUE).all() and (col1[4] == R.GREY).all()      # column 1: sample 1 alone; the reference level row(0.5) = 4
    assert (col1[[0, 1, 2, 3, 5, 6]] == R.WHITE).all()
    # clamping and the reference level under the curve
    img = R.line_panel([2.0, -1.0, 0.5, 0.5], 4, 4, 0.0, 1.0, 0.5, np.float32)
    assert (img[:, 0] == R.BLUE).all()                     # rows 0 (above the axis) .. 3 (below it)
    assert (img[2, 2] == R.BLUE).all() and (img[2, 3] == R.BLUE).all() and (img[0, 3] == R.WHITE).all()
    # a NaN or an infinity paints its columns red over the whole height: columns 0 and 1 both cover sample 1
    img = R.line_panel([0.5, np.nan, 0.5, 0.5, np.inf, 0.5, 0.5, 0.5], 8, 4, 0.0, 1.0, 0.5, np.float32)
    red = [(img[:, c] == R.RED).all() for c in range(8)]
    assert red == [True, True, False, True, True, False, False, False]
    # fewer columns than samples, not dividing them: column c covers (c n) // W .. min(((c + 1) n) // W, n - 1)
    y = np.linspace(0.0, 1.0, 7)
    img = R.line_panel(y, 3, 16, 0.0, 1.0, 2.0, np.float64)
    for c, (i0, i1) in enumerate([(0, 2), (2, 4), (4, 6)]):
        rows = [min(int((1.0 - y[i]) * 16), 15) for i in (i0, i1)]
        blue = np.where((img[:, c] == R.BLUE).all(axis=1))[0]
        assert blue.min() == min(rows) and blue.max() == max(rows) and len(blue) == max(rows) - min(rows) + 1


def test_control_strip_round_half_up():
    # strip 16: m = 8.  |c| m = 0.5 -> 1 row, 0.49 / 8 -> 0, 1.5 -> 2, 2.5 -> 3 (half UP, not to even), 8 -> 8
    cases = [(0.0625, 1), (0.06, 0), (0.1875, 2), (0.3125, 3), (1.0, 8), (3.0, 8), (0.0, 0)]
    for dt in (np.float32, np.float64):
        for c, n in cases:
            top, bot, col = R.bar_rows(c, 16, dt)
            assert (top, bot) == (8 - n, 8) and (col == R.RED or n == 0), (c, top, bot)
            top, bot, col = R.bar_rows(-c, 16, dt)
            assert (top, bot) == (8, 8 + n) and (col == R.NEG or c == 0), (c, top, bot)
        # the formula of the header is |c| m rounded half up, for every value whose product is exact
        for k in range(0, 129):
            c = k / 128.0
            assert R.bar_rows(c, 16, dt)[0] == 8 - int(Fraction(k, 128) * 8 + Fraction(1, 2))
        assert R.bar_rows(np.nan, 16, dt)[2] is None
    assert R.bar_rows(1.0, 17, np.float32)[:2] == (0, 8) and R.bar_rows(-1.0, 17, np.float32)[:2] == (8, 16)     # odd strip: m = 8
    # columns: control k of 3 in 10 columns owns [0, 3), [3, 6), [6, 10); the bar the middle half, [c0 + w // 4, c1 - w // 4)
    img = R.control_strip([1.0, -1.0, 0.5], 10, 4, np.float32)
    assert img.shape == (4, 10, 3)
    red0 = (img == R.RED).all(axis=2)
    blue = (img == R.NEG).all(axis=2)
    assert red0[:2, 0:3].all() and not red0[2:, 0:3].any()
    assert blue[2:, 3:6].all() and not blue[:2].any()
    assert red0[1, 7:9].all() and not red0[0, 6:10].any() and not red0[1, 6] and not red0[1, 9]      # w = 4: one column off each side; 0.5 * 2 = 1 row
    assert (R.control_strip([0.0, 0.0], 8, 4, np.float64) == 255).all()                            # after a reset nothing is drawn


def test_mixing_controls():
    assert R.mixing_controls(0) == [-1.0, 1.0, 0.0, 0.0]       # u_t, u_b, v_l, v_r over u_max (mixing.py:212-234)
    assert R.mixing_controls(1) == [1.0, -1.0, 0.0, 0.0]
    assert R.mixing_controls(2) == [0.0, 0.0, -1.0, 1.0]
    assert R.mixing_controls(3) == [0.0, 0.0, 1.0, -1.0]
    assert R.mixing_controls(4) == [0.0, 0.0, 0.0, 0.0]
    img = R.control_strip(R.mixing_controls(2), 16, 4, np.float32)
    assert (img[:, 0:8] == 255).all() and (img[2:, 9:11] == R.NEG).all() and (img[:2, 13:15] == R.RED).all()


def test_entry_points_through_the_host_layers():
    from beacon_amd import _lib, vec
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    declared = set(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert {"bcn_render", "bcn_render_shape"} <= declared and len(declared) == 78
    for doc in ("README.md", "INTEGRATION.md"):
        assert "78 entry points" in open(os.path.join(ROOT, doc)).read(), doc
    vp, ci = C.c_void_p, C.c_int
    assert _lib.SIGNATURES["bcn_render_shape"] == (ci, [vp, C.POINTER(_lib.RenderCfg), C.POINTER(ci), C.POINTER(ci)])
    assert _lib.SIGNATURES["bcn_render"] == (ci, [vp, C.POINTER(_lib.RenderCfg), vp, vp, ci, vp, vp])
    # the struct of the header, field by field
    body = re.search(r"typedef struct \{([^}]*)\} bcn_render_cfg;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.RenderCfg._fields_]
    assert C.sizeof(_lib.RenderCfg) == 6 * 4 + 3 * 8
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4     # no buffer changed size
    assert vec._RENDER_OPS == ("render",) and not set(vec._RENDER_OPS) & (set(vec._ALL_OPS) | set(vec._NORM_OPS) | set(vec._ROLLOUT_OPS))
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    assert src.count('m.def("render(') == 1 and src.count('m.impl("render"') == 2          # CUDA and Meta
    from beacon_amd import build
    assert build.FILE_FLAGS["render.hip"][0] == "-ffp-contract=off" and not any("fast-math" in f for f in build.FLAGS)


def _bare(cls, *a, **k):
    """an env of class `cls` without a handle and without a device: what the argument checks of renderer() may look at"""
    from beacon_amd import vec
    c = getattr(vec, cls)
    return c._derive(c.__new__(c), *a, **k)


def test_python_layer_errors_need_no_gpu():
    ray = _bare("VecRayleigh")
    with pytest.raises(ValueError, match="scale"):
        ray.renderer(scale=0)
    with pytest.raises(ValueError, match="no default range"):
        ray.renderer(field="u")
    with pytest.raises(ValueError, match="field"):
        ray.renderer(field="w")
    with pytest.raises(ValueError, match="vmax > vmin"):
        ray.renderer(vmin=1.0, vmax=1.0)
    with pytest.raises(ValueError, match="strip"):
        _bare("VecMixing").renderer(strip=-2)
    with pytest.raises(ValueError, match="width and height"):
        _bare("VecShkadov").renderer(width=0)
    for ode in ("VecLorenz", "VecVortex"):
        with pytest.raises(ValueError, match="nothing to draw"):
            _bare(ode).renderer()
        with pytest.raises(ValueError, match="nothing to draw"):
            _bare(ode).render_rgb()
    # the defaults are the reference's axes
    cfg = ray._render_cfg(2, 512, 128, None, "scalar", None, None, None)
    assert (cfg.plane, cfg.scale, cfg.strip, cfg.has_range, cfg.lo, cfg.hi) == (0, 2, -1, 1, -0.5, 0.5)
    cfg = _bare("VecMixing")._render_cfg(1, 512, 128, 0, "p", -1.0, 2.0, None)
    assert (cfg.plane, cfg.strip, cfg.lo, cfg.hi) == (3, 0, -1.0, 2.0)
    b = _bare("VecBurgers")
    cfg = b._render_cfg(1, 300, 64, None, "scalar", None, None, None)
    assert (cfg.width, cfg.height, cfg.lo, cfg.hi, cfg.ref) == (300, 64, 0.5 - 2 * 0.1, 0.5 + 2 * 0.1, 0.5)
    cfg = _bare("VecShkadov")._render_cfg(1, 512, 128, None, "scalar", None, None, None)
    assert (cfg.lo, cfg.hi, cfg.ref) == (0.0, 2.0, 1.0)
    cfg = _bare("VecSloshing")._render_cfg(1, 512, 128, None, "scalar", None, None, None)
    assert (cfg.lo, cfg.hi, cfg.ref) == (0.25, 1.75, 1.0)

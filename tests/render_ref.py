"""NumPy restatement of the device frames (bcn_render, include/beacon_hip.h), written from the pixel rules stated there and not from
the kernels: every function computes in the env's real type (np.float32 / np.float64) with exactly the operations the rules name --
one subtraction, one division, one product with a power of two or with H, truncation, integers -- so that the kernels can be held
to it byte for byte (tests/test_gpu_render.py)."""
import numpy as np

WHITE, GREY, BLUE, RED, NEG = (255, 255, 255), (160, 160, 160), (31, 119, 180), (255, 0, 0), (0, 0, 255)


def bin_of(t, n):
    """bin(t, n): 0 for t <= 0, n - 1 for t >= 1, else min(int(t n), n - 1); -1 for a NaN.  `t` keeps its dtype."""
    t = np.asarray(t)
    out = np.full(t.shape, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        lo, hi = t <= 0, t >= 1
    mid = ~(np.isnan(t) | lo | hi)
    out[lo] = 0
    out[hi] = n - 1
    out[mid] = np.minimum((t[mid] * t.dtype.type(n)).astype(np.int64), n - 1)
    return out


def color_index(v, vmin, vmax, dtype):
    """Index into the colour table of every value: bin((v - vmin) / (vmax - vmin), 256) in `dtype`; -1 for a NaN."""
    dt = np.dtype(dtype).type
    v = np.asarray(v, dtype=dt)
    lo = dt(vmin)
    den = dt(vmax) - lo
    with np.errstate(all="ignore"):
        t = (v - lo) / den
    return bin_of(t, 256)


def colorize(v, vmin, vmax, lut, dtype):
    """uint8 [..., 3]: lut[index], and (0, 0, 0) for a NaN."""
    idx = color_index(v, vmin, vmax, dtype)
    rgb = np.asarray(lut, dtype=np.uint8)[np.maximum(idx, 0)]
    rgb[idx < 0] = 0
    return rgb


def field_panel(plane, scale, vmin, vmax, lut, dtype):
    """plane: [ny + 2, nx + 2] (x fastest, ghost cells included) -> uint8 [ny scale, nx scale, 3]: pixel (r, c) shows cell
    i = 1 + c // scale, j = ny - r // scale."""
    ny, nx = plane.shape[0] - 2, plane.shape[1] - 2
    r, c = np.arange(ny * scale), np.arange(nx * scale)
    cells = np.asarray(plane)[(ny - r // scale)[:, None], (1 + c // scale)[None, :]]
    return colorize(cells, vmin, vmax, lut, dtype)


def row_of(y, ymin, ymax, H, dtype):
    dt = np.dtype(dtype).type
    hi = dt(ymax)
    den = hi - dt(ymin)
    with np.errstate(all="ignore"):
        t = (hi - np.asarray(y, dtype=dt)) / den
    return bin_of(t, H)


def line_panel(y, W, H, ymin, ymax, yref, dtype):
    """y: [n] samples -> uint8 [H, W, 3]."""
    y = np.asarray(y, dtype=dtype)
    n = y.shape[0]
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = WHITE
    img[int(row_of(yref, ymin, ymax, H, dtype))] = GREY
    for c in range(W):
        i0, i1 = (c * n) // W, min(((c + 1) * n) // W, n - 1)
        seg = y[i0:i1 + 1]
        if not np.all(np.isfinite(seg)):
            img[:, c] = RED
            continue
        rows = row_of(seg, ymin, ymax, H, dtype)
        img[rows.min():rows.max() + 1, c] = BLUE
    return img


def mixing_controls(a):
    """(u_t, u_b, v_l, v_r) / u_max of the action index a, as get_control assigns them."""
    u_t = u_b = v_l = v_r = 0.0
    if a == 0:
        u_b, u_t = 1.0, -1.0
    if a == 1:
        u_b, u_t = -1.0, 1.0
    if a == 2:
        v_r, v_l = 1.0, -1.0
    if a == 3:
        v_r, v_l = -1.0, 1.0
    return [u_t, u_b, v_l, v_r]


def bar_rows(c, strip, dtype):
    """Rows [top, bot) of the strip that the bar of the control value c takes, and its colour (None: no bar)."""
    dt = np.dtype(dtype).type
    c = dt(c)
    if np.isnan(c):
        c = dt(0)
    c = min(max(c, dt(-1)), dt(1))
    m = strip // 2
    nrow = (int(abs(c) * dt(2 * m)) + 1) // 2          # |c| m rounded half up
    if c > 0:
        return m - nrow, m, RED
    if c < 0:
        return m, m + nrow, NEG
    return m, m, None


def control_strip(ctrl, W, strip, dtype):
    """ctrl: the n_ctrl stored control values -> uint8 [strip, W, 3]."""
    img = np.empty((strip, W, 3), dtype=np.uint8)
    img[:] = WHITE
    n = len(ctrl)
    for k, c in enumerate(ctrl):
        c0, c1 = (k * W) // n, ((k + 1) * W) // n
        q = (c1 - c0) // 4
        top, bot, col = bar_rows(c, strip, dtype)
        if col is not None and bot > top:
            img[top:bot, c0 + q:c1 - q] = col
    return img


def field_frame(plane, ctrl, scale, vmin, vmax, lut, dtype, strip=None):
    panel = field_panel(plane, scale, vmin, vmax, lut, dtype)
    strip = panel.shape[0] // 8 if strip is None else strip
    return np.concatenate([panel, control_strip(ctrl, panel.shape[1], strip, dtype)], axis=0)


def line_frame(y, ctrl, W, H, ymin, ymax, yref, dtype, strip=None):
    strip = H // 8 if strip is None else strip
    return np.concatenate([line_panel(y, W, H, ymin, ymax, yref, dtype), control_strip(ctrl, W, strip, dtype)], axis=0)

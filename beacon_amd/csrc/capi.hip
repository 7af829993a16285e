// capi.hip -- extern "C" surface of libbeacon_hip.so (include/beacon_hip.h): handle
// management, argument-block construction (derived constants are computed here in double and
// narrowed once), state copies.  All device work is enqueued on the caller's stream.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>

#include <new>
#include <vector>

#include "env1d.h"
#include "ns2d.h"
#include "ns2d_builtin.h"
#include "ns2d_geom.h"
#include "ns2d_sched.h"
#include "ode_env.h"
#include "params.h"
#include "snapshot.h"
#include "episode.h"
#include "shkadov_jets.h"
#include "normalize.h"
#include "rollout.h"
#include "render.h"

static thread_local char g_err[512] = "";

// default visibility: the on-demand kernel plugins (csrc/jit/ns2d_jit.hip) report through the library's error buffer
__attribute__((visibility("default"))) void bcn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// The two internal queries of ns2d_geom.h (default visibility, like bcn_set_error: for beacon_amd/jit.py, not part of the ABI)
template <class G>
static int geometry_of(const G& g, size_t esz, long long out[5]) {
  if (!g.admissible(esz)) return 0;
  out[0] = g.nw(), out[1] = g.rl(), out[2] = g.threads(), out[3] = (long long)g.lds_bytes(esz), out[4] = (long long)g.scratch_elems();
  return 1;
}

__attribute__((visibility("default"))) int bcn_jit_geometry(int rows, int nx, int ny, int r, int g, int f64, long long out[5]) {
  const size_t esz = f64 ? 8 : 4;
  if (!out) return 0;
  if (rows == 1) return geometry_of(bcn_geom::Rows1{nx, ny, r, g}, esz, out);
  if (rows == 2) return geometry_of(bcn_geom::Rows2{nx, ny, r, g}, esz, out);
  if (rows == 4) return geometry_of(bcn_geom::Rows4{nx, ny, r, g}, esz, out);
  return 0;
}

__attribute__((visibility("default"))) int bcn_jit_builtin(int i, int out[7]) {
#define BCN_ROW1(REAL, NX, NY, R, KIND, GF) {sizeof(REAL) == 8, NX, NY, KIND, 1, R, GF},
#define BCN_ROW2(REAL, NX, NY, R, KIND, GF) {sizeof(REAL) == 8, NX, NY, KIND, 2, R, GF},
  static const int rows[][7] = {BCN_BUILTIN_FAST(BCN_ROW1) BCN_BUILTIN_FAST2(BCN_ROW2)};
#undef BCN_ROW1
#undef BCN_ROW2
  if (!out || i < 0 || i >= (int)(sizeof(rows) / sizeof(rows[0]))) return 0;
  for (int k = 0; k < 7; k++) out[k] = rows[i][k];
  return 1;
}

namespace {

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// F<float>(...) or F<double>(...) by a handle's (or a create call's) dtype
#define BCN_BY_DTYPE(dtype, F, ...) ((dtype) == BCN_F32 ? F<float>(__VA_ARGS__) : F<double>(__VA_ARGS__))

// The constructor skeleton of every env: allocate, fill the handle's header, let `fill` set the argument block from the cfg, init(),
// hand the handle out (or delete it when init() failed)
template <typename Env, typename Fill>
int make_env(int kind, int batch, int dtype, int device, uint64_t cfg_hash, bcn_env_t* out, Fill fill) {
  auto* e = new (std::nothrow) Env();
  if (!e) { bcn_set_error("out of host memory"); return BCN_ERR_ARG; }
  e->kind = kind; e->batch = batch; e->dtype = dtype; e->device = device; e->esz = dtype == BCN_F64 ? 8 : 4;
  e->cfg_hash = cfg_hash;
  fill(e);
  const int rc = e->init();
  if (rc) { delete e; return rc; }
  *out = e;
  return BCN_OK;
}

// bcn_get_state / bcn_set_state of the grid envs.  State buffer layout: [B][planes][row]; device layout: [planes][B][row]
int copy_planes(void* buf, void* dev, int planes, size_t row, int batch, int is_device, hipStream_t s, bool out) {
  const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : (out ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice);
  for (int k = 0; k < planes; k++) {
    char* e = static_cast<char*>(buf) + (size_t)k * row;
    char* d = static_cast<char*>(dev) + (size_t)k * batch * row;
    if (out) BCN_HIP(hipMemcpy2DAsync(e, planes * row, d, row, row, batch, kind, s));
    else BCN_HIP(hipMemcpy2DAsync(d, row, e, planes * row, row, batch, kind, s));
  }
  if (!is_device) BCN_HIP(hipStreamSynchronize(s));
  return BCN_OK;
}

// widest unit (bytes) in which the copy kernels move rows of `row` bytes (snapshot.h, episode.h)
inline unsigned copy_unit(size_t row) { return row % 16 == 0 ? 16 : row % 8 == 0 ? 8 : row % 4 == 0 ? 4 : 1; }

// FNV-1a over the values of a cfg struct (its int32 members, then its doubles: the layout of every bcn_*_cfg), without the padding
// between the two groups: the part of bcn_snapshot_signature that says "same constructor arguments"
uint64_t snap_fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
  return h;
}
template <typename Cfg, int NI, int ND>
uint64_t snap_cfg_hash(const Cfg* c) {
  constexpr size_t doubles_at = (NI * sizeof(int32_t) + 7) / 8 * 8;
  static_assert(sizeof(Cfg) == doubles_at + ND * sizeof(double), "cfg struct: NI int32 members followed by ND doubles");
  static_assert(offsetof(Cfg, ndt_act) < NI * sizeof(int32_t) && offsetof(Cfg, dt) >= doubles_at, "cfg struct: the int32 members come first");
  uint64_t h = snap_fnv(14695981039346656037ull, c, NI * sizeof(int32_t));
  return snap_fnv(h, reinterpret_cast<const char*>(c) + doubles_at, ND * sizeof(double));
}

// ------------------------------------------------------------------------------------------
// rayleigh / mixing
// ------------------------------------------------------------------------------------------
template <typename real>
struct NS2DEnv : bcn_env_s {
  NS2DArgs<real> a{};
  DevBuf fields;    // u,v,p,S,us,vs   [6][B][ncell]
  DevBuf work;      // g0,g1,g2        [3][B][ncell]  (only when the work arrays do not fit LDS)
  DevBuf obs_hist, a_last, ia_last, stpbuf, sweepbuf, orderbuf, schedbuf, fscrbuf, statusbuf;
  int32_t* status_int = nullptr;   // per-replica status words when the caller passes no status_dev
  bool fast_ok = false;
  bool guard_holds() const { return a.nx >= 48 && a.ny >= 48; }

  int init() {
    const size_t n = (size_t)batch * a.ncell, per = n * sizeof(real);
    int rc;
    real* f;
    if ((rc = fields.zalloc(6 * n, &f))) return rc;
    a.u = f; a.v = f + n; a.p = f + 2 * n; a.S = f + 3 * n; a.us = f + 4 * n; a.vs = f + 5 * n;
    const bool in_lds = ns2d_generic_lds_bytes(a.ncell, sizeof(real)) > (2 * 16 + 64) * sizeof(real);
    if (!in_lds) {
      if ((rc = work.alloc(3 * per))) return rc;
      real* w = static_cast<real*>(work.p);
      a.g0 = w; a.g1 = w + n; a.g2 = w + 2 * n;
    }
    if ((rc = obs_hist.zalloc((size_t)batch * a.n_obs, &a.obs_hist))) return rc;
    if ((rc = a_last.zalloc((size_t)batch * (a.n_sgts > 0 ? a.n_sgts : 1), &a.a_last))) return rc;
    if ((rc = ia_last.zalloc(batch, &a.ia_last))) return rc;
    if ((rc = stpbuf.zalloc(batch, &a.stp))) return rc;
    stp = a.stp;
    if ((rc = sweepbuf.zalloc((size_t)batch * (a.ndt_act > 0 ? a.ndt_act : 1), &a.sweeps_int))) return rc;
    if ((rc = statusbuf.zalloc(batch, &status_int))) return rc;
    if ((rc = orderbuf.zalloc(batch, &a.order_out))) return rc;
    const SchedLayout sl = ns2d_sched_layout(batch);   // zeroed by one memset per step
    char* sched;
    if ((rc = schedbuf.zalloc(sl.total, &sched))) return rc;
    a.sched_ctl = sched;
    a.sched_bytes = sl.total;
    a.cyc = reinterpret_cast<unsigned long long*>(sched + sl.cyc_offset);
    fast_ok = ns2d_fast_supported<real>(a);
    if (fast_ok && (a.fscr_stride = ns2d_fast_scratch_elems<real>(a)) > 0) {
      if ((rc = fscrbuf.zalloc((size_t)batch * a.fscr_stride, &a.fscr))) return rc;
    }
    variant = fast_ok ? 1 : 0;
    // both precisions: the extrapolating plan with PROVEN landings (plan 3: every stop sweep is the reference's, ns2d_fast_impl.h).
    // (Until round 5 float64 ran the lower-bound plan 1: plan 3's landings were not yet verified by a bound.)
    a.conv_plan = 3;
    // the landing test of plans 2 / 3 rests on a bound (BCN_CONV_GUARD, bcn_common.h) that holds for grids with no side below 48
    // cells -- every grid the reference can construct (nx = 50 L, ny = 50 H, L, H >= 1); smaller ones: the proven plan
    if (!guard_holds()) a.conv_plan = 1;
    // rayleigh float32: a solve opens with unevaluated double sweeps up to 15/16 of the previous timestep's count minus the stretch
    // in front of the stop where the residual is already below the landing guard (spec_start 17: ns2d_fast_impl.h); the landing
    // must find the residual above the guard or the solve is repeated without the guess.  Measured on the bench workload, repeats
    // per step of 102 400 solves / cycles per sweep -- with the global guard alone and a fixed fraction: 7/8 27 252 / 916,
    // 6/8 2 021 / 818, 5/8 205 / 827, 4/8 5 / 837, off 0 / 888; with the slow-mode guard: 6/8 789, the zone-aware opening 219 / 778
    // (the unverified rule of round 3 at 7/8: 750).  mixing's counts drop by up to 9x from one timestep to the next: off; the
    // float64 kernels are built without the opening
    a.spec_start = (a.kind == 0 && sizeof(real) == 4) ? 17 : 0;
    // mixing float32: the ordered part of the scalar transport as parallel passes while their count stays within 24 (12 at the
    // reference's u_max; ns2d_fast2_impl.h); float64 keeps the reference's ordered sweep
    a.transport_iter = (a.kind == 1 && sizeof(real) == 4) ? 24 : 0;
    // slow-mode landing guard: the constants of the grids the reference's defaults construct are built in (computed by
    // beacon_amd/stoprule.py, checked by tests/test_oracle.py); any other grid: bcn_set_slow_mode_bound, else BCN_CONV_GUARD alone
    static const struct { int nx, ny, kind; double cx, cut[2], cl[2]; } kBuiltin[] = {
        {128, 64, 0, 0.25, {0.9, 0.8}, {1.00020, 1.00568}},    // rayleigh L = 2.56, H = 1.28 (the bench workload)
        {50, 50, 0, 0.25, {0.9, 0.8}, {1.00020, 1.00020}},     // rayleigh.py:20-27 defaults L = H = 1
        {100, 100, 1, 0.25, {0.9, 0.8}, {1.00167, 1.00594}},   // mixing.py:20-28 defaults L = H = 1
    };
    for (const auto& e : kBuiltin)
      if (e.nx == a.nx && e.ny == a.ny && e.kind == a.kind && fabs((double)a.cx - e.cx) < 1e-6) set_slow_mode_bound(2, e.cut, e.cl);
    return BCN_OK;
  }
  int set_slow_mode_bound(int n, const double* cutoff, const double* bound) override {
    for (int k = 0; k < n; k++)
      if (!(cutoff[k] > 0.0 && cutoff[k] < 1.0) || !(bound[k] >= 1.0)) {
        bcn_set_error("bcn_set_slow_mode_bound: cutoff %g must lie in (0, 1), bound %g must be >= 1", cutoff[k], bound[k]);
        return BCN_ERR_ARG;
      }
    for (int k = 0; k < 2; k++) {
      a.slow_l2lc[k] = k < n ? (float)log2(cutoff[k]) : 0.f;
      // rounded UP to float: the kernels compare against it
      a.slow_cl[k] = k < n ? nextafterf((float)bound[k], INFINITY) : INFINITY;
      slow_cut[k] = k < n ? cutoff[k] : 0.0;
    }
    return BCN_OK;
  }
  int get_slow_mode_bound(double* cutoff, double* bound) const override {
    int n = 0;
    for (int k = 0; k < 2; k++)
      if (slow_cut[k] > 0.0) { cutoff[n] = slow_cut[k]; bound[n] = (double)a.slow_cl[k]; n++; }
    return n;
  }
  double slow_cut[2] = {0.0, 0.0};
  ~NS2DEnv() override {
    DeviceGuard g(device);
    fields.release(); work.release(); fscrbuf.release(); obs_hist.release(); a_last.release(); ia_last.release();
    stpbuf.release(); sweepbuf.release(); orderbuf.release(); schedbuf.release(); statusbuf.release();
  }
  size_t state_elems() const override { return 4 * (size_t)a.ncell; }
  int get_state(void* buf, int is_device, hipStream_t s) override {
    return copy_planes(buf, fields.p, 4, (size_t)a.ncell * sizeof(real), batch, is_device, s, true);
  }
  int set_state(const void* buf, int is_device, hipStream_t s) override {
    return copy_planes(const_cast<void*>(buf), fields.p, 4, (size_t)a.ncell * sizeof(real), batch, is_device, s, false);
  }
  int set_variant(int v) override { variant = (v == 1 && fast_ok) ? 1 : 0; host.launched = nullptr; return variant; }
  void set_mask(const uint8_t* m) override { a.mask = m; }
  int set_sched(int mode, int grid, int q, int lpt_min_batch) override {
    a.sched_mode = mode; a.sched_grid = grid; a.sched_q_user = q; a.lpt_min_batch = lpt_min_batch;
    return BCN_OK;
  }
  int set_option(const char* name, int value) override {
    if (!strcmp(name, "conv_plan") && value >= 0 && value <= 3) {
      if (value >= 2 && !guard_holds()) { bcn_set_error("conv_plan %d needs a grid with no side below 48 cells (%dx%d): plans 0, 1 only", value, a.nx, a.ny); return BCN_ERR_ARG; }
      a.conv_plan = value;
      return BCN_OK;
    }
    if (!strcmp(name, "plan_overshoot") && value >= 0 && value <= 64) { a.plan_overshoot = value; return BCN_OK; }
    if (!strcmp(name, "verify_conv")) { a.verify_conv = value ? 1 : 0; return BCN_OK; }
    if (!strcmp(name, "spec_start") && value >= 0 && value <= 17) { a.spec_start = value; return BCN_OK; }
    if (!strcmp(name, "transport_iter") && value >= 0 && value <= 64) { a.transport_iter = value; return BCN_OK; }
    if (!strcmp(name, "sched_tail") && value >= 0 && value <= 1024) { host.sched_tail = value; return BCN_OK; }
    if (!strcmp(name, "generic_threads") && (value == 0 || value == 256 || value == 1024)) { host.generic_nt = value; return BCN_OK; }
    if (!strcmp(name, "params_kernel") && (value == 0 || value == 1)) { params_kernel = value; host.launched = nullptr; return BCN_OK; }
    if (!strcmp(name, "cell_runs") && (value == 0 || value == 1)) { cell_runs = value; host.launched = nullptr; return BCN_OK; }
    return bcn_env_s::set_option(name, value);
  }
  int get_counters(uint64_t* host, hipStream_t s) override {
    BCN_HIP(hipMemcpyAsync(host, a.cyc, (size_t)batch * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    BCN_HIP(hipStreamSynchronize(s));
    return BCN_OK;
  }
  typedef int (*plugin_fn)(const void*, int, void*);
  plugin_fn plugin = nullptr;        // register-resident kernel of a grid that is not built in (bcn_set_fast_plugin)
  int set_fast_plugin(void* fn, size_t scratch_elems) override {
    plugin_prm = nullptr;   // (the table-reading launcher belongs to the plugin it was set behind)
    if (!fn) { plugin = nullptr; fast_ok = ns2d_fast_supported<real>(a); variant = fast_ok ? 1 : 0; return BCN_OK; }
    if (scratch_elems > 0) {
      DeviceGuard g(device);
      fscrbuf.release();
      int rc = fscrbuf.zalloc((size_t)batch * scratch_elems, &a.fscr);
      if (rc) return rc;
      a.fscr_stride = scratch_elems;
    }
    plugin = reinterpret_cast<plugin_fn>(fn);
    fast_ok = true; variant = 1; host.launched = nullptr;
    return BCN_OK;
  }
  // the plugin's launcher of its table-reading kernels (bcn_set_fast_plugin_params; a plugin built with -DBCN_JIT_PRM=1)
  typedef int (*plugin_prm_fn)(const void*, int, void*, const void*);
  plugin_prm_fn plugin_prm = nullptr;
  int set_fast_plugin_params(void* fn) override {
    if (fn && !plugin) { bcn_set_error("bcn_set_fast_plugin_params: the handle has no kernel plugin (bcn_set_fast_plugin comes first)"); return BCN_ERR_ARG; }
    plugin_prm = reinterpret_cast<plugin_prm_fn>(fn);
    host.launched = nullptr;
    return BCN_OK;
  }
  NS2DHost host;   // launcher-side state: kernel name of the last step, options that no kernel reads
  // per-replica parameters (bcn_set_params): the table is a kernel argument of its own.  The generic kernel takes it, and a handle
  // that has one steps through that kernel whatever its variant -- unless the option "params_kernel" is 1, the variant is 1 and
  // the handle has a register-resident kernel that takes the table too (built in: params.h; a plugin: plugin_prm).  Clearing
  // the table restores the previous dispatch.  A register-resident kernel that ignores the table is never launched while one is set.
  const real* prm = nullptr;
  int params_kernel = 0;
  void use_params(const void* table) override { prm = static_cast<const real*>(table); host.launched = nullptr; }
  bool prm_fast() const {
    return prm && params_kernel == 1 && variant == 1 && (plugin ? plugin_prm != nullptr : ns2d_fast_supported_prm<real>(a));
  }
  const char* kernel_name() const override {
    if (prm && !prm_fast()) return "ns2d_generic_step";
    return host.launched ? host.launched : (variant == 1 ? "ns2d_fast_step" : "ns2d_generic_step");
  }
  int launch(hipStream_t s) {
    a.host = &host;
    if (prm) {
      if (prm_fast()) {
        // BCN_ERR_UNSUPPORTED (as below: the hybrid's 32-bit addressing): the generic kernel takes the step, with the table
        const int rc = plugin ? plugin_prm(&a, batch, s, prm) : ns2d_launch_fast_prm<real>(a, batch, s, prm);
        if (rc != BCN_ERR_UNSUPPORTED) return rc;
      }
      return ns2d_launch_generic_prm<real>(a, batch, s, prm);
    }
    if (variant == 1 && plugin) {
      // BCN_ERR_UNSUPPORTED: the batch does not fit the plugin's addressing (ns2d_fast4_impl.h: 32-bit offsets from a
      // replica's u): the generic kernel takes the step
      const int rc = plugin(&a, batch, s);
      if (rc != BCN_ERR_UNSUPPORTED) return rc;
      return ns2d_launch_generic<real>(a, batch, s);
    }
    if constexpr (std::is_same<real, float>::value) {
      if (runs_unit()) return ns2d_launch_fast_runs(a, batch, s);
    }
    if (variant == 1) return ns2d_launch_fast<real>(a, batch, s);
    return ns2d_launch_generic<real>(a, batch, s);
  }
  // option "cell_runs" (default 1): 0 keeps a float32 handle on a built-in grid off ns2d_fast_runs.hip, so that its variant-1 steps go
  // to the cell-by-cell kernels of ns2d_fast.hip (the same bits: tests/test_gpu_jacobi_cells.py)
  int cell_runs = 1;
  // whether a variant-1 step of this handle without a parameter table goes through the kernels with cell runs: what launch() asks,
  // and what bcn_cell_runs_active answers
  bool runs_unit() const {
    if constexpr (std::is_same<real, float>::value) return variant == 1 && !plugin && cell_runs == 1 && ns2d_fast_runs_supported(a);
    return false;
  }
  int cell_runs_active() const override { return !prm && runs_unit() ? 1 : 0; }
};

template <typename real>
void ns2d_common(NS2DArgs<real>& a, int nx, int ny, double dx, double dy, double dt, double tol) {
  a.nx = nx; a.ny = ny; a.sx = nx + 2; a.ncell = (nx + 2) * (ny + 2);
  a.dt = (real)dt; a.rdx = (real)(1.0 / dx); a.rdy = (real)(1.0 / dy);
  a.rdx2 = (real)(1.0 / (dx * dx)); a.rdy2 = (real)(1.0 / (dy * dy));
  const double den = dx * dx + dy * dy;
  a.cx = (real)(0.5 * dy * dy / den);
  a.cy = (real)(0.5 * dx * dx / den);
  a.cb = (real)(0.5 * dx * dx * dy * dy / den / dt);
  a.tol = (real)tol;
}

template <typename real>
int make_rayleigh(const bcn_rayleigh_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<NS2DEnv<real>>(BCN_RAYLEIGH, batch, dtype, device, snap_cfg_hash<bcn_rayleigh_cfg, 12, 9>(c), out, [c](NS2DEnv<real>* e) {
    NS2DArgs<real>& a = e->a;
    ns2d_common(a, c->nx, c->ny, c->dx, c->dy, c->dt, c->tol);
    a.kind = 0; a.ndt_act = c->ndt_act; a.n_act = c->n_act; a.itmax = c->itmax;
    a.n_sgts = c->n_sgts; a.nx_sgts = c->nx_sgts;
    a.nxo = c->nx_obs_pts; a.nyo = c->ny_obs_pts; a.nx_obs = c->nx_obs; a.ny_obs = c->ny_obs;
    a.n_obs_steps = c->n_obs_steps; a.n_obs = 3 * c->n_obs_steps * c->nx_obs_pts * c->ny_obs_pts;
    a.kmom = (real)bcn_rayleigh_kmom(c->pr, c->ra);
    a.ksc = (real)bcn_rayleigh_ksc(c->pr, c->ra);
    e->prm_cfg[0] = c->ra; e->prm_aux[0] = c->pr;
    a.Tc = (real)c->Tc; a.Th = (real)c->Th; a.C = (real)c->C;
    a.rwd_scale = (real)(1.0 / (0.5 * c->dy * c->nx));
    e->n_obs = a.n_obs; e->n_act = c->n_sgts; e->ndt_act = a.ndt_act;
  });
}

template <typename real>
int make_mixing(const bcn_mixing_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<NS2DEnv<real>>(BCN_MIXING, batch, dtype, device, snap_cfg_hash<bcn_mixing_cfg, 14, 9>(c), out, [c](NS2DEnv<real>* e) {
    NS2DArgs<real>& a = e->a;
    ns2d_common(a, c->nx, c->ny, c->dx, c->dy, c->dt, c->tol);
    a.kind = 1; a.ndt_act = c->ndt_act; a.n_act = c->n_act; a.itmax = c->itmax;
    a.n_sgts = 0; a.nx_sgts = 1;
    a.nxo = c->nx_obs_pts; a.nyo = c->ny_obs_pts; a.nx_obs = c->nx_obs; a.ny_obs = c->ny_obs;
    a.n_obs_steps = c->n_obs_steps; a.n_obs = 3 * c->n_obs_steps * c->nx_obs_pts * c->ny_obs_pts;
    a.i_min = c->i_min; a.i_max = c->i_max; a.j_min = c->j_min; a.j_max = c->j_max;
    a.kmom = (real)bcn_mixing_kmom(c->re);
    a.ksc = (real)bcn_mixing_ksc(c->pe);
    e->prm_cfg[0] = c->re; e->prm_cfg[1] = c->pe; e->prm_aux[0] = c->re; e->prm_aux[1] = c->u_max;
    a.u_max = (real)bcn_mixing_u_max(c->re, c->re, c->u_max); a.ref_c = (real)c->ref_c; a.C0 = (real)c->C0;
    e->n_obs = a.n_obs; e->n_act = 1; e->ndt_act = a.ndt_act;
  });
}

// ------------------------------------------------------------------------------------------
// 1D envs
// ------------------------------------------------------------------------------------------
template <typename real>
struct Env1D : bcn_env_s {
  Env1DArgs<real> a{};
  int nfields = 4;
  int nact = 1;                    // columns of a_last / a_prev
  DevBuf fields, a_last, a_prev, stpbuf, nctrbuf;
  const char* general = "";        // name of the env's general step kernel
  Env1DLaunch last;                // what the last step launched (env1d_step_t); nothing before the first step and after a failed one

  int init() {
    int rc;
    const size_t n = (size_t)batch * a.n;
    real* f;
    if ((rc = fields.zalloc(4 * n, &f))) return rc;
    a.f0 = f; a.f1 = f + n; a.f2 = f + 2 * n; a.f3 = f + 3 * n;
    if ((rc = a_last.zalloc((size_t)batch * nact, &a.a_last))) return rc;
    if ((rc = a_prev.zalloc((size_t)batch * nact, &a.a_prev))) return rc;
    if ((rc = stpbuf.zalloc(batch, &a.stp))) return rc;
    stp = a.stp;
    if ((rc = nctrbuf.zalloc(batch, &a.nctr))) return rc;
    a.nsigma = 0; a.nseed_lo = 0; a.nseed_hi = 0; a.noff = 0;
    return BCN_OK;
  }
  ~Env1D() override {
    DeviceGuard g(device);
    fields.release(); a_last.release(); a_prev.release(); stpbuf.release(); nctrbuf.release();
  }
  int set_noise(double sigma, uint64_t seed, int64_t replica_offset) override {
    if (!(sigma >= 0) || replica_offset < 0) { bcn_set_error("bcn_set_noise: sigma >= 0 and replica_offset >= 0"); return BCN_ERR_ARG; }
    a.nsigma = (real)sigma; a.nseed_lo = (uint32_t)seed; a.nseed_hi = (uint32_t)(seed >> 32); a.noff = (int)replica_offset;
    DeviceGuard g(device);
    BCN_HIP(hipMemset(nctrbuf.p, 0, nctrbuf.bytes));
    return BCN_OK;
  }
  size_t state_elems() const override { return (size_t)nfields * a.n; }
  int get_state(void* buf, int is_device, hipStream_t s) override {
    return copy_planes(buf, fields.p, nfields, (size_t)a.n * sizeof(real), batch, is_device, s, true);
  }
  int set_state(const void* buf, int is_device, hipStream_t s) override {
    return copy_planes(const_cast<void*>(buf), fields.p, nfields, (size_t)a.n * sizeof(real), batch, is_device, s, false);
  }
  const char* kernel_name() const override { return last.name ? last.name : general; }
  void kernel_shape(int* k, int* nt) const override { *k = last.k; *nt = last.nt; }
  void set_mask(const uint8_t* m) override { a.mask = m; }
  void use_params(const void* table) override { a.prm = static_cast<const real*>(table); }
  int set_option(const char* name, int value) override {
    if (!strcmp(name, "cells_per_thread") && (value == 0 || value == 1 || value == 2 || value == 4 || value == 8)) { a.force_k = value; return BCN_OK; }
    if (!strcmp(name, "one_wave") && value >= 0 && value <= 2) { a.one_wave = value; return BCN_OK; }   // 2: without the packed float32 kernel
    return bcn_env_s::set_option(name, value);
  }
};

template <typename real>
int make_burgers(const bcn_burgers_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<Env1D<real>>(BCN_BURGERS, batch, dtype, device, snap_cfg_hash<bcn_burgers_cfg, 5, 4>(c), out, [c](Env1D<real>* e) {
    e->nfields = 3; e->nact = 1; e->general = "burgers_step_k";
    Env1DArgs<real>& a = e->a;
    a.n = a.nx = c->nx; a.ndt_act = c->ndt_act; a.n_act = c->n_act; a.n_obs = c->n_obs_pts;
    a.ctrl_pos = c->ctrl_pos; a.n_obs_pts = c->n_obs_pts;
    a.u_target = (real)c->u_target; a.amp = (real)c->amp;
    e->prm_cfg[0] = c->u_target; e->prm_cfg[1] = c->amp;
    a.dx = (real)c->dx; a.rdx = (real)(1.0 / c->dx); a.dt = (real)c->dt;
    e->n_obs = c->n_obs_pts; e->n_act = 1; e->ndt_act = a.ndt_act;
  });
}

template <typename real>
int make_shkadov(const bcn_shkadov_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<Env1D<real>>(BCN_SHKADOV, batch, dtype, device, snap_cfg_hash<bcn_shkadov_cfg, 12, 7>(c), out, [c](Env1D<real>* e) {
    e->nfields = 4; e->nact = c->n_jets; e->general = "shkadov_step_k";
    Env1DArgs<real>& a = e->a;
    a.n = a.nx = c->nx; a.ndt_act = c->ndt_act; a.n_act = c->n_act; a.n_obs = c->n_obs * c->n_jets;
    a.n_jets = c->n_jets; a.jet_pos = c->jet_pos; a.jet_hw = c->jet_hw; a.jet_space = c->jet_space;
    a.l_obs = c->l_obs; a.l_rwd = c->l_rwd; a.n_obs_jet = c->n_obs; a.obs_stride = c->obs_stride;
    a.n_interp = c->n_interp;
    a.delta_p = (real)bcn_shkadov_delta_p(c->delta);
    e->prm_cfg[0] = c->delta;
    a.jet_amp = (real)c->jet_amp; a.eps = (real)c->eps; a.h_blow = (real)c->h_blow;
    a.blowup_rwd = (real)c->blowup_rwd;
    a.dx = (real)c->dx; a.rdx = (real)(1.0 / c->dx); a.dt = (real)c->dt;
    e->n_obs = a.n_obs; e->n_act = c->n_jets; e->ndt_act = a.ndt_act;
  });
}

template <typename real>
int make_sloshing(const bcn_sloshing_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<Env1D<real>>(BCN_SLOSHING, batch, dtype, device, snap_cfg_hash<bcn_sloshing_cfg, 4, 5>(c), out, [c](Env1D<real>* e) {
    e->nfields = 4; e->nact = 1; e->general = "sloshing_step_k";
    Env1DArgs<real>& a = e->a;
    a.nx = c->nx; a.n = c->nx + 2; a.ndt_act = c->ndt_act; a.n_act = c->n_act;
    a.n_obs = c->nx / 2 + (c->nx % 2 ? 1 : 0);
    a.n_interp = c->n_interp;
    a.g = (real)c->g; a.amp = (real)c->amp; a.alpha = (real)c->alpha;
    e->prm_cfg[0] = c->amp; e->prm_cfg[1] = c->alpha; e->prm_cfg[2] = c->g;
    a.dx = (real)c->dx; a.rdx = (real)(1.0 / c->dx); a.dt = (real)c->dt;
    e->n_obs = a.n_obs; e->n_act = 1; e->ndt_act = a.ndt_act;
  });
}

// ------------------------------------------------------------------------------------------
// lorenz / vortex: one lane per replica (ode_env.h)
// ------------------------------------------------------------------------------------------
template <typename real>
struct OdeEnv : bcn_env_s {
  OdeArgs<real> a{};
  DevBuf st, iubuf, stpbuf, stage;   // stage: [B][n_state] rows of a host-side state copy
  int nreal = 0, nstate = 0;

  int init() {
    int rc;
    if ((rc = st.zalloc((size_t)batch * nreal, &a.st))) return rc;
    if ((rc = iubuf.zalloc(batch, &a.iu))) return rc;
    if ((rc = stpbuf.zalloc(batch, &a.stp))) return rc;
    stp = a.stp;
    a.batch = batch; a.n_obs = n_obs;
    // observation rows through LDS for float64 (48 / 64 B rows), direct per-lane stores for float32: measured A/B/A/B at B = 2^20
    // (DESIGN.md §10): lorenz float64 30.8 / 34.5 us per step staged / direct, float32 19.8 / 19.0; vortex float32 42.4 / 40.9,
    // float64 81.1 / 81.7
    a.obs_stage = sizeof(real) == 8 ? 1 : 0;
    return BCN_OK;
  }
  ~OdeEnv() override {
    DeviceGuard g(device);
    st.release(); iubuf.release(); stpbuf.release(); stage.release();
  }
  size_t state_elems() const override { return (size_t)nstate; }
  // caller layout [B][nstate]; device layout [field][B] (+ lorenz's int32 action index): one pack / unpack kernel, host copies
  // through a staging buffer
  int copy_state(void* buf, int is_device, hipStream_t s, bool out) {
    real* ext = static_cast<real*>(buf);
    const size_t bytes = (size_t)batch * nstate * sizeof(real);
    if (!is_device) {
      if (!stage.p) { int rc = stage.alloc(bytes); if (rc) return rc; }
      ext = static_cast<real*>(stage.p);
      if (!out) BCN_HIP(hipMemcpyAsync(ext, buf, bytes, hipMemcpyHostToDevice, s));
    }
    const int rc = out ? ode_launch_pack<real>(a, ext, s) : ode_launch_unpack<real>(a, ext, s);
    if (rc) return rc;
    if (!is_device) {
      if (out) BCN_HIP(hipMemcpyAsync(buf, ext, bytes, hipMemcpyDeviceToHost, s));
      BCN_HIP(hipStreamSynchronize(s));
    }
    return BCN_OK;
  }
  int get_state(void* buf, int is_device, hipStream_t s) override { return copy_state(buf, is_device, s, true); }
  int set_state(const void* buf, int is_device, hipStream_t s) override { return copy_state(const_cast<void*>(buf), is_device, s, false); }
  int set_variant(int) override { bcn_set_error("lorenz / vortex have one kernel and no variants"); return BCN_ERR_ARG; }
  int set_sched(int, int, int, int) override { bcn_set_error("lorenz / vortex step one replica per lane: nothing to schedule"); return BCN_ERR_ARG; }
  int set_option(const char* name, int value) override {
    if (!strcmp(name, "obs_stage") && (value == 0 || value == 1)) { a.obs_stage = value; return BCN_OK; }
    return bcn_env_s::set_option(name, value);
  }
  void set_mask(const uint8_t* m) override { a.mask = m; }
  void use_params(const void* table) override { a.prm = static_cast<const real*>(table); }
  const char* kernel_name() const override { return kind == BCN_LORENZ ? "lorenz_step_k" : "vortex_step_k"; }
};

template <typename real>
int make_lorenz(const bcn_lorenz_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<OdeEnv<real>>(BCN_LORENZ, batch, dtype, device, snap_cfg_hash<bcn_lorenz_cfg, 2, 4>(c), out, [c](OdeEnv<real>* e) {
    e->nreal = LZ_NREAL; e->nstate = LZ_NSTATE;
    OdeArgs<real>& a = e->a;
    a.kind = BCN_LORENZ; a.ndt_act = c->ndt_act; a.n_act = c->n_act;
    a.dt = (real)c->dt; a.sigma = (real)c->sigma; a.rho = (real)c->rho; a.beta = (real)c->beta;
    e->prm_cfg[0] = c->sigma; e->prm_cfg[1] = c->rho; e->prm_cfg[2] = c->beta;
    e->n_obs = 6; e->n_act = 1; e->ndt_act = c->ndt_act;
  });
}

template <typename real>
int make_vortex(const bcn_vortex_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  return make_env<OdeEnv<real>>(BCN_VORTEX, batch, dtype, device, snap_cfg_hash<bcn_vortex_cfg, 2, 19>(c), out, [c](OdeEnv<real>* e) {
    e->nreal = VX_NREAL; e->nstate = VX_NSTATE;
    OdeArgs<real>& a = e->a;
    a.kind = BCN_VORTEX; a.ndt_act = c->ndt_act; a.n_act = c->n_act;
    a.dt = (real)c->dt;
    a.lmbda_re = (real)c->lmbda_re; a.lmbda_cx = (real)c->lmbda_cx; a.mu_re = (real)c->mu_re; a.mu_cx = (real)c->mu_cx;
    a.alpha_re = (real)c->alpha_re; a.alpha_cx = (real)c->alpha_cx;
    // the derived constants of vortex.py:26-42, in double and in the reference's order
    a.ire = (real)bcn_vortex_ire(c->re_crit, c->re);
    e->prm_cfg[0] = c->re; e->prm_cfg[1] = c->weight; e->prm_aux[0] = c->re_crit;
    a.omega_f = (real)c->omega_f;
    a.m_omega_f_gamma = (real)(-c->omega_f * c->gamma);
    a.domega = (real)(c->omega_s - c->omega_f);
    a.beta_m = (real)(c->beta / (c->omega_f * c->mass));
    a.mod_min = (real)c->mod_min; a.dmod = (real)(c->mod_max - c->mod_min);
    a.phase_min = (real)c->phase_min; a.dphase = (real)(c->phase_max - c->phase_min);
    a.rwd_k = (real)(2.0 * c->omega_s * c->gamma);
    a.weight = (real)c->weight;
    e->n_obs = 8; e->n_act = 2; e->ndt_act = c->ndt_act;
  });
}

template <typename real>
static int ode_call(bcn_env_t h, bool reset, const void* actions, void* obs, void* rwd, uint8_t* done, uint8_t* trunc,
                    int32_t* status, void* stream) {
  auto* e = static_cast<OdeEnv<real>*>(h);
  DeviceGuard g(e->device);
  OdeArgs<real> a = e->a;
  a.actions = actions;
  a.obs_out = static_cast<real*>(obs);
  a.rwd_out = static_cast<real*>(rwd);
  a.done = done; a.trunc = trunc; a.status = status;
  return reset ? ode_launch_reset<real>(a, static_cast<hipStream_t>(stream)) : ode_launch_step<real>(a, static_cast<hipStream_t>(stream));
}

int check_create(const void* cfg, int batch, int dtype, int device, bcn_env_t* out) {
  if (!cfg || !out) { bcn_set_error("null cfg/out"); return BCN_ERR_ARG; }
  if (batch <= 0) { bcn_set_error("batch must be > 0"); return BCN_ERR_ARG; }
  if (dtype != BCN_F32 && dtype != BCN_F64) { bcn_set_error("dtype must be BCN_F32 or BCN_F64"); return BCN_ERR_ARG; }
  int ndev = 0;
  BCN_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { bcn_set_error("device %d out of range (%d visible)", device, ndev); return BCN_ERR_ARG; }
  return BCN_OK;
}

#define BCN_CHECK_KIND(h, K)                                                        \
  if (!(h) || (h)->kind != (K)) { bcn_set_error("handle is not a " #K " env"); return BCN_ERR_ARG; }

template <typename real>
static int ns2d_reset_t(bcn_env_t h, const void* init, void* obs, void* stream) {
  auto* e = static_cast<NS2DEnv<real>*>(h);
  DeviceGuard g(e->device);
  NS2DArgs<real> a = e->a;
  a.init_fields = static_cast<const real*>(init);
  a.obs_out = static_cast<real*>(obs);
  return ns2d_launch_reset<real>(a, e->batch, static_cast<hipStream_t>(stream));
}

template <typename real>
static int ns2d_step_t(bcn_env_t h, const void* actions, const int32_t* iactions, void* actions_norm, void* obs,
                       void* rwd, uint8_t* done, uint8_t* trunc, int32_t* status, int32_t* sweeps, void* stream) {
  auto* e = static_cast<NS2DEnv<real>*>(h);
  DeviceGuard g(e->device);
  NS2DArgs<real>& a = e->a;
  a.actions = static_cast<const real*>(actions);
  a.iactions = iactions;
  a.actions_norm = static_cast<real*>(actions_norm);
  a.obs_out = static_cast<real*>(obs);
  a.rwd_out = static_cast<real*>(rwd);
  a.done = done; a.trunc = trunc; a.sweeps = sweeps;
  a.status = status ? status : e->status_int;   // the chunk scheduler carries a replica's status across chunks
  return e->launch(static_cast<hipStream_t>(stream));
}

template <typename real>
static Env1DArgs<real>& env1d_io(bcn_env_t h, const void* actions, const void* noise, const void* init, void* obs,
                                 void* rwd, uint8_t* done, uint8_t* trunc, int32_t* status) {
  auto* e = static_cast<Env1D<real>*>(h);
  Env1DArgs<real>& a = e->a;
  a.actions = static_cast<const real*>(actions);
  a.noise = static_cast<const real*>(noise);
  a.init_fields = static_cast<const real*>(init);
  a.obs_out = static_cast<real*>(obs);
  a.rwd_out = static_cast<real*>(rwd);
  a.done = done; a.trunc = trunc; a.status = status;
  return a;
}

template <typename real>
static int env1d_reset_t(bcn_env_t h, int (*launch)(const Env1DArgs<real>&, int, hipStream_t), const void* init, void* obs, void* stream) {
  DeviceGuard g(h->device);
  return launch(env1d_io<real>(h, nullptr, nullptr, init, obs, nullptr, nullptr, nullptr, nullptr), h->batch, static_cast<hipStream_t>(stream));
}

// The step of a 1D env: the launcher says which kernel it dispatched through its return path (Env1DLaunch), and the handle keeps
// that for bcn_kernel_name / bcn_kernel_shape; a launcher that failed leaves the general name and (0, 0)
template <typename real>
static int env1d_step_t(bcn_env_t h, int (*launch)(const Env1DArgs<real>&, int, hipStream_t, Env1DLaunch*), const void* actions,
                        const void* noise, void* obs, void* rwd, uint8_t* done, uint8_t* trunc, int32_t* status, void* stream) {
  DeviceGuard g(h->device);
  Env1DLaunch note;
  const int rc = launch(env1d_io<real>(h, actions, noise, nullptr, obs, rwd, done, trunc, status), h->batch, static_cast<hipStream_t>(stream), &note);
  static_cast<Env1D<real>*>(h)->last = rc ? Env1DLaunch() : note;
  return rc;
}

// shkadov.reset with rand_init in one launch: the argument block of a reset (no actions, no noise tensor, no rwd / done / trunc / status),
// the warm launcher's three arguments behind it; the handle keeps what was dispatched, as after a step
template <typename real>
static int shkadov_reset_random_t(bcn_env_t h, const void* init, const int32_t* n_steps, int rand_steps, int32_t* n_out, void* obs, void* stream) {
  DeviceGuard g(h->device);
  Env1DLaunch note;
  const int rc = shkadov_launch_warm<real>(env1d_io<real>(h, nullptr, nullptr, init, obs, nullptr, nullptr, nullptr, nullptr), h->batch, n_steps,
                                           rand_steps, n_out, static_cast<hipStream_t>(stream), &note);
  static_cast<Env1D<real>*>(h)->last = rc ? Env1DLaunch() : note;
  return rc;
}

// ------------------------------------------------------------------------------------------
// snapshots (snapshot.h): which arrays of a handle are state, and where they sit in a snapshot of n replicas
// ------------------------------------------------------------------------------------------
// One named segment of a handle (SegDesc, snapshot.h) and where it lives there: plane stride = batch rows in the handle, n rows in the
// snapshot.
struct SnapDesc { SegDesc seg; void* dev; };

// What the next *_step reads of what an earlier call wrote ("Snapshots", has the reasoning for what is left out: us / vs,
// the work arrays, fscr, the sweep counts, the scheduler block and the cycle counters are rewritten or zeroed inside every step).
template <typename real>
int snap_desc(bcn_env_t h, SnapDesc* d) {
  int n = 0;
  if (h->kind == BCN_RAYLEIGH || h->kind == BCN_MIXING) {
    auto* e = static_cast<NS2DEnv<real>*>(h);
    d[n++] = {{"fields", BCN_SNAP_REAL, 4, (size_t)e->a.ncell}, e->fields.p};
    d[n++] = {{"obs_hist", BCN_SNAP_REAL, 1, (size_t)e->a.n_obs}, e->obs_hist.p};
    if (h->kind == BCN_RAYLEIGH) d[n++] = {{"a_last", BCN_SNAP_REAL, 1, (size_t)e->a.n_sgts}, e->a_last.p};
    else d[n++] = {{"ia_last", BCN_SNAP_I32, 1, 1}, e->ia_last.p};
    d[n++] = {{"stp", BCN_SNAP_I32, 1, 1}, e->stpbuf.p};
  } else if (h->kind == BCN_LORENZ || h->kind == BCN_VORTEX) {
    auto* e = static_cast<OdeEnv<real>*>(h);
    d[n++] = {{"fields", BCN_SNAP_REAL, e->nreal, 1}, e->st.p};
    if (h->kind == BCN_LORENZ) d[n++] = {{"iu", BCN_SNAP_I32, 1, 1}, e->iubuf.p};
    d[n++] = {{"stp", BCN_SNAP_I32, 1, 1}, e->stpbuf.p};
  } else {
    auto* e = static_cast<Env1D<real>*>(h);
    d[n++] = {{"fields", BCN_SNAP_REAL, e->nfields, (size_t)e->a.n}, e->fields.p};
    d[n++] = {{"a_last", BCN_SNAP_REAL, 1, (size_t)e->nact}, e->a_last.p};
    d[n++] = {{"a_prev", BCN_SNAP_REAL, 1, (size_t)e->nact}, e->a_prev.p};
    d[n++] = {{"stp", BCN_SNAP_I32, 1, 1}, e->stpbuf.p};
    d[n++] = {{"nctr", BCN_SNAP_U32, 1, 1}, e->nctrbuf.p};
  }
  return n;
}

inline size_t snap_up16(size_t x) { return (x + 15) / 16 * 16; }
inline size_t seg_elem_bytes(int elem, size_t esz) {
  return elem == BCN_SNAP_REAL ? esz : elem == BCN_SNAP_U8 ? 1 : elem == BCN_SNAP_F64 || elem == BCN_SNAP_I64 ? 8 : 4;
}

// THE layout of every packed buffer (snapshot, episode, per-jet, normaliser): the nd segments of `d` one behind the other for n
// replicas of an env whose reals take esz bytes, every start a multiple of 16 bytes; a segment takes (planes == 0 ? 1 : planes * n) *
// row_elems elements.  Fills the first max_lay entries of `lay` (NULL: none) and returns the bytes of the buffer.
size_t seg_layout(const SegDesc* d, int nd, size_t n, size_t esz, bcn_snapshot_seg* lay, int max_lay) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = snap_up16(off);
    if (lay && k < max_lay) {
      memset(&lay[k], 0, sizeof(lay[k]));
      strncpy(lay[k].name, d[k].name, sizeof(lay[k].name) - 1);
      lay[k].offset = off; lay[k].elem = d[k].elem; lay[k].planes = d[k].planes; lay[k].row_elems = (int64_t)d[k].row_elems;
    }
    off += (d[k].planes == 0 ? 1 : (size_t)d[k].planes * n) * d[k].row_elems * seg_elem_bytes(d[k].elem, esz);
  }
  return snap_up16(off);
}

// Lays out a snapshot of n replicas of this handle's configuration: the bytes it takes, optionally the named segments (`lay`, up to
// max_lay; the count is returned) and the kernels' table `t` (handle side: this handle's arrays and the packed output buffer
// `out_buf` of its `batch` replicas; NULL out_buf leaves the five output segments out of the copy).
int snap_build(bcn_env_t h, int n, char* out_buf, SnapTable* t, bcn_snapshot_seg* lay, int max_lay, size_t* bytes) {
  SnapDesc d[16];
  int nd = BCN_BY_DTYPE(h->dtype, snap_desc, h, d);
  const size_t B = (size_t)h->batch, esz = h->esz;
  const bcn_out_layout_t o = bcn_out_layout(B, (size_t)h->n_obs, esz);   // the callers' out_buf
  d[nd++] = {{"obs", BCN_SNAP_REAL, 1, (size_t)h->n_obs}, out_buf};
  d[nd++] = {{"rwd", BCN_SNAP_REAL, 1, 1}, out_buf ? out_buf + o.rwd : nullptr};
  d[nd++] = {{"status", BCN_SNAP_I32, 1, 1}, out_buf ? out_buf + o.status : nullptr};
  d[nd++] = {{"done", BCN_SNAP_U8, 1, 1}, out_buf ? out_buf + o.done : nullptr};
  d[nd++] = {{"trunc", BCN_SNAP_U8, 1, 1}, out_buf ? out_buf + o.trunc : nullptr};
  SegDesc sd[16];
  bcn_snapshot_seg sl[16];
  for (int k = 0; k < nd; k++) sd[k] = d[k].seg;
  const size_t total = seg_layout(sd, nd, (size_t)n, esz, sl, nd);
  size_t blk = 0;
  int ns = 0;
  for (int k = 0; k < nd; k++) {
    const size_t row = sd[k].row_elems * seg_elem_bytes(sd[k].elem, esz);
    if (lay && k < max_lay) lay[k] = sl[k];
    for (int pl = 0; t && d[k].dev && pl < sd[k].planes; pl++) {
      if (ns >= BCN_SNAP_MAX_SEG || row == 0 || row > 0xffffffffull) { bcn_set_error("snapshot: segment table overflow"); return -1; }
      SnapSeg& g = t->seg[ns++];
      g.dev = static_cast<char*>(d[k].dev) + (size_t)pl * B * row;
      g.snap_off = sl[k].offset + (size_t)pl * (size_t)n * row;
      g.row_bytes = (unsigned)row;
      g.blk0 = (unsigned)blk;
      if (row >= BCN_SNAP_LONG_ROW) {
        g.bpr = (unsigned)((row + BCN_SNAP_TILE - 1) / BCN_SNAP_TILE);
        g.unit = 16;
        blk += B * g.bpr;
      } else {
        g.bpr = 0;
        g.unit = copy_unit(row);
        blk += (B * (row / g.unit) + BCN_SNAP_NT * 4 - 1) / (BCN_SNAP_NT * 4);
      }
      if (blk > 0x7fffffffull) { bcn_set_error("snapshot: batch too large for one launch"); return -1; }
    }
  }
  if (bytes) *bytes = total;
  if (t) { t->nseg = ns; t->batch = h->batch; t->n_src = n; t->nblk = (unsigned)blk; }
  return nd;
}

// The three bookkeeping buffers of this handle's batch: their range check, their segment table (episode.h, normalize.h,
// shkadov_jets.h) and seg_layout -- the first max_lay segments into `lay` and / or the bytes the buffer takes; the segment count is
// returned, -1 with the message set when one launch cannot cover the batch.  Only batch, observation length (jets: the action
// length, which is the jet count) and dtype of the handle are used.
int episode_build(bcn_env_t h, bcn_snapshot_seg* lay, int max_lay, size_t* bytes) {
  const size_t B = (size_t)h->batch;
  if (h->batch < 1 || h->n_obs < 1 || B * (size_t)h->n_obs * h->esz / 4 > 0x7fffffffull) {
    bcn_set_error("episode: batch %d x %d observations is outside what one launch covers", h->batch, h->n_obs);
    return -1;
  }
  SegDesc d[BCN_EP_NSEG];
  episode_segs((size_t)h->n_obs, d);
  const size_t total = seg_layout(d, BCN_EP_NSEG, B, h->esz, lay, max_lay);
  if (bytes) *bytes = total;
  return BCN_EP_NSEG;
}
int normalize_build(bcn_env_t h, bcn_snapshot_seg* lay, int max_lay, size_t* bytes) {
  const size_t B = (size_t)h->batch, n = (size_t)h->n_obs;
  if (h->batch < 1 || h->n_obs < 1 || B * n > 0x7fffffffull) {
    bcn_set_error("normalize: batch %d x %d observations is outside what one launch covers", h->batch, h->n_obs);
    return -1;
  }
  SegDesc d[BCN_NRM_NSEG];
  normalize_segs(B, n, d);
  const size_t total = seg_layout(d, BCN_NRM_NSEG, B, h->esz, lay, max_lay);
  if (bytes) *bytes = total;
  return BCN_NRM_NSEG;
}
int jets_build(bcn_env_t h, bcn_snapshot_seg* lay, int max_lay, size_t* bytes) {
  const size_t B = (size_t)h->batch, nj = (size_t)h->n_act;
  if (h->batch < 1 || h->n_act < 1 || B * nj > 0x7fffffffull) {
    bcn_set_error("shkadov jets: batch %d x %d jets is outside what one launch covers", h->batch, h->n_act);
    return -1;
  }
  SegDesc d[BCN_JETS_NSEG];
  jets_segs(nj, d);
  const size_t total = seg_layout(d, BCN_JETS_NSEG, B, h->esz, lay, max_lay);
  if (bytes) *bytes = total;
  return BCN_JETS_NSEG;
}
// the bodies of the bcn_*_bytes / bcn_*_layout pairs of those three, behind each entry point's own argument checks
typedef int (*seg_build_fn)(bcn_env_t, bcn_snapshot_seg*, int, size_t*);
inline size_t built_bytes(seg_build_fn build, bcn_env_t h) {
  size_t bytes = 0;
  return build(h, nullptr, 0, &bytes) < 0 ? 0 : bytes;       // (the build function has set the message)
}
inline int built_layout(seg_build_fn build, bcn_env_t h, bcn_snapshot_seg* segs, int max_segs) {
  const int nd = build(h, segs, max_segs, nullptr);
  return nd < 0 ? 0 : nd;
}

// The rollout buffer of this handle for T steps (rollout.h): the same, with the two arguments the layout depends on besides the
// handle.  `who`: the entry point, for the message.  The actions are int32 [B] for the discrete envs and real [B][n_act] otherwise.
inline bool rollout_int_actions(bcn_env_t h) { return h->kind == BCN_MIXING || h->kind == BCN_LORENZ; }
int rollout_build(const char* who, bcn_env_t h, int T, int flags, bcn_snapshot_seg* lay, int max_lay, size_t* bytes) {
  if (T < 1 || T > 0x3fffffff) { bcn_set_error("%s: T = %d steps; at least 1", who, T); return -1; }
  if (flags & ~(BCN_RO_FINAL_OBS | BCN_RO_JETS)) { bcn_set_error("%s: unknown flags %#x", who, flags); return -1; }
  if ((flags & BCN_RO_JETS) && h->kind != BCN_SHKADOV) { bcn_set_error("%s: BCN_RO_JETS needs a BCN_SHKADOV env", who); return -1; }
  const size_t B = (size_t)h->batch;
  const size_t widest = (size_t)(h->n_obs > h->n_act ? h->n_obs : h->n_act);
  if (h->batch < 1 || h->n_obs < 1 || h->n_act < 1 || B * widest * h->esz / 4 > 0x7fffffffull) {
    bcn_set_error("%s: batch %d x %d observations is outside what one launch covers", who, h->batch, h->n_obs);
    return -1;
  }
  SegDesc d[BCN_RO_NSEG];
  const bool ia = rollout_int_actions(h);
  rollout_segs(T, (size_t)h->n_obs, ia ? BCN_SNAP_I32 : BCN_SNAP_REAL, ia ? 1 : (size_t)h->n_act, (size_t)h->n_act, flags, d);
  const size_t total = seg_layout(d, BCN_RO_NSEG, B, h->esz, lay, max_lay);
  if (bytes) *bytes = total;
  return BCN_RO_NSEG;
}
// one row copy of a record or a begin: rows of `row` bytes of B replicas, `blk` = the copy workgroups in front of it (advanced)
RolloutJob rollout_job(const char* src, char* dst, size_t B, size_t row, int when, int slot_off, unsigned* blk) {
  RolloutJob j;
  j.src = src; j.dst = dst; j.slot_bytes = (unsigned long long)(B * row);
  j.unit = copy_unit(row);      // rows are reals or int32: multiples of 4 bytes
  j.upr = (unsigned)(row / j.unit);
  j.total = (unsigned)(B * j.upr);
  j.blk0 = *blk;
  j.when = when; j.slot_off = slot_off;
  *blk += (j.total + BCN_RO_NT * BCN_RO_UPL - 1) / (BCN_RO_NT * BCN_RO_UPL);
  return j;
}

// bcn_shkadov_jet_rewards of a checked shkadov handle: the film and the jet layout come from the handle's argument block, the
// replica mask is the one bcn_set_mask left there, status / done / trunc are those of the step's packed outputs
template <typename real>
int shkadov_jets_t(bcn_env_t h, const char* out, char* jets, const bcn_snapshot_seg* lay, int with_stats, void* stream) {
  const Env1DArgs<real>& e = static_cast<Env1D<real>*>(h)->a;
  const bcn_out_layout_t o = bcn_out_layout((size_t)h->batch, (size_t)h->n_obs, h->esz);
  ShkadovJetsArgs<real> a;
  a.h = e.f0;
  a.status = reinterpret_cast<const int32_t*>(out + o.status);
  a.done = reinterpret_cast<const uint8_t*>(out + o.done); a.trunc = reinterpret_cast<const uint8_t*>(out + o.trunc);
  a.mask = e.mask;
  a.rwd_jets = reinterpret_cast<real*>(jets + lay[JETS_RWD_JETS].offset);
  a.ret = with_stats ? reinterpret_cast<real*>(jets + lay[JETS_RET].offset) : nullptr;
  a.last_ret = reinterpret_cast<real*>(jets + lay[JETS_LAST_RET].offset);
  a.sum_ret = reinterpret_cast<double*>(jets + lay[JETS_SUM_RET].offset);
  a.npairs = (unsigned)h->batch * (unsigned)e.n_jets;
  a.n = e.n; a.nx = e.nx;
  a.n_jets = e.n_jets; a.jet_pos = e.jet_pos; a.jet_space = e.jet_space; a.l_rwd = e.l_rwd;
  a.dx = e.dx; a.blowup_rwd = e.blowup_rwd;
  DeviceGuard g(h->device);
  return shkadov_jets_launch<real>(a, static_cast<hipStream_t>(stream));
}

// bcn_set_params: the table of derived constants of every replica, narrowed once to the handle's dtype, row k of replica b at
// [k * B + b]
template <typename real>
void params_table(bcn_env_t h, const double* values, std::vector<char>& out) {
  const BcnParamDesc* d = bcn_param_desc(h->kind);
  const size_t B = (size_t)h->batch;
  out.resize((size_t)d->n_derived * B * sizeof(real));
  real* t = reinterpret_cast<real*>(out.data());
  for (size_t b = 0; b < B; b++) {
    double p[BCN_MAX_PARAMS] = {0, 0, 0}, dv[BCN_MAX_PARAMS] = {0, 0, 0};
    for (int k = 0; k < d->n; k++) p[k] = values[(size_t)k * B + b];
    bcn_derive_params(h->kind, p, h->prm_aux, dv);
    for (int k = 0; k < d->n_derived; k++) t[(size_t)k * B + b] = (real)dv[k];
  }
}

// ------------------------------------------------------------------------------------------
// frames (render.h): what a frame of this handle shows, from the handle's own arrays and a bcn_render_cfg
// ------------------------------------------------------------------------------------------
// Checks the cfg against the handle and fills everything of the argument block but the caller's pointers.  The defaults are the
// reference's axes; the narrowed range must still be a range (the kernels divide by hi - lo in the env's type).
template <typename real>
int render_fill(const char* who, bcn_env_t h, const bcn_render_cfg* c, RenderArgs& a) {
  a = RenderArgs{};
  a.batch = h->batch; a.f64 = h->dtype == BCN_F64;
  double lo = c->lo, hi = c->hi, ref = c->ref;
  int panel_h = 0;
  if (h->kind == BCN_RAYLEIGH || h->kind == BCN_MIXING) {
    auto* e = static_cast<NS2DEnv<real>*>(h);
    if (c->plane < BCN_PLANE_SCALAR || c->plane > BCN_PLANE_P) { bcn_set_error("%s: plane %d; BCN_PLANE_SCALAR, _U, _V or _P", who, c->plane); return BCN_ERR_ARG; }
    if (c->scale < 1) { bcn_set_error("%s: scale %d; at least 1", who, c->scale); return BCN_ERR_ARG; }
    if ((long long)e->a.nx * c->scale > BCN_RENDER_MAX_W) { bcn_set_error("%s: %d cells x scale %d: a frame row holds at most %d pixels", who, e->a.nx, c->scale, BCN_RENDER_MAX_W); return BCN_ERR_ARG; }
    if ((long long)e->a.ny * c->scale > (1 << 20)) { bcn_set_error("%s: %d cells x scale %d pixel rows", who, e->a.ny, c->scale); return BCN_ERR_ARG; }
    if (!c->has_range) {
      if (c->plane != BCN_PLANE_SCALAR) { bcn_set_error("%s: the planes u, v, p have no default range: set has_range, lo, hi", who); return BCN_ERR_ARG; }
      lo = h->kind == BCN_RAYLEIGH ? (double)e->a.Tc : 0.0;          // rayleigh.py / mixing.py render(): vmin, vmax of imshow
      hi = h->kind == BCN_RAYLEIGH ? (double)e->a.Th : (double)e->a.C0;
    }
    const real* plane[4] = {e->a.S, e->a.u, e->a.v, e->a.p};
    a.field = plane[c->plane]; a.rep_stride = (size_t)e->a.ncell;
    a.nx = e->a.nx; a.ny = e->a.ny; a.scale = c->scale;
    a.W = a.nx * a.scale; panel_h = a.ny * a.scale;
    if (h->kind == BCN_RAYLEIGH) { a.ctrl = e->a.a_last; a.n_ctrl = e->a.n_sgts; }
    else { a.ctrl = e->a.ia_last; a.ctrl_int = 1; a.n_ctrl = 4; }
  } else if (h->kind == BCN_BURGERS || h->kind == BCN_SHKADOV || h->kind == BCN_SLOSHING) {
    auto* e = static_cast<Env1D<real>*>(h);
    const int W = c->width == 0 ? 512 : c->width, H = c->height == 0 ? 128 : c->height;
    if (W < 1 || W > BCN_RENDER_MAX_W || H < 1 || H > BCN_RENDER_MAX_H) {
      bcn_set_error("%s: %d x %d pixels; 1 .. %d wide, 1 .. %d high", who, W, H, BCN_RENDER_MAX_W, BCN_RENDER_MAX_H);
      return BCN_ERR_ARG;
    }
    if (!c->has_range) {
      if (h->kind == BCN_BURGERS) {       // burgers.py render(): u_target -+ 2 sigma; sigma is the noise setting of the handle
        if (!(e->a.nsigma > 0)) { bcn_set_error("%s: burgers has a default range only with inlet noise (bcn_set_noise): set has_range, lo, hi, ref", who); return BCN_ERR_ARG; }
        lo = (double)e->a.u_target - 2.0 * (double)e->a.nsigma; hi = (double)e->a.u_target + 2.0 * (double)e->a.nsigma; ref = (double)e->a.u_target;
      } else if (h->kind == BCN_SHKADOV) { lo = 0.0; hi = 2.0; ref = 1.0; }
      else { lo = 0.25; hi = 1.75; ref = 1.0; }
    }
    a.line = 1;
    a.field = e->a.f0 + (h->kind == BCN_SLOSHING ? 1 : 0);   // sloshing: h[1 .. nx] between the ghost cells
    a.rep_stride = (size_t)e->a.n; a.ns = e->a.nx;
    a.W = W; panel_h = H;
    a.ctrl = e->a.a_last; a.n_ctrl = e->nact;
    if (!isfinite(ref)) { bcn_set_error("%s: ref %g is not finite", who, ref); return BCN_ERR_ARG; }
  } else {
    bcn_set_error("%s: lorenz and vortex keep no trajectory on the device: nothing to draw", who);
    return BCN_ERR_UNSUPPORTED;
  }
  if (!isfinite(lo) || !isfinite(hi) || !(hi > lo) || !((real)hi > (real)lo)) { bcn_set_error("%s: range (%g, %g): hi must exceed lo, also in the handle's precision", who, lo, hi); return BCN_ERR_ARG; }
  const int strip = c->strip < 0 ? panel_h / 8 : c->strip;
  if (strip > BCN_RENDER_MAX_H) { bcn_set_error("%s: strip of %d rows; at most %d", who, strip, BCN_RENDER_MAX_H); return BCN_ERR_ARG; }
  if (a.n_ctrl < 1 || a.n_ctrl > BCN_RENDER_MAX_CTRL) { bcn_set_error("%s: %d controls; 1 .. %d", who, a.n_ctrl, BCN_RENDER_MAX_CTRL); return BCN_ERR_ARG; }
  a.H = panel_h; a.strip = strip;
  a.lo = lo; a.hi = hi; a.ref = ref;
  return BCN_OK;
}

}  // namespace

extern "C" {

// ---- rayleigh --------------------------------------------------------------------------------
int bcn_rayleigh_create(const bcn_rayleigh_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->nx < 2 || c->ny < 2 || c->n_sgts < 1 || c->n_sgts > 64 || c->nx_sgts < 1 || c->ndt_act < 0) {
    bcn_set_error("rayleigh cfg out of range (nx,ny >= 2; 1 <= n_sgts <= 64)");
    return BCN_ERR_ARG;
  }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_rayleigh, c, batch, dtype, device, out);
}

int bcn_rayleigh_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_RAYLEIGH);
  return BCN_BY_DTYPE(h->dtype, ns2d_reset_t, h, init_fields_dev, obs_dev, stream);
}

int bcn_rayleigh_step(bcn_env_t h, const void* actions_dev, void* actions_norm_dev, void* obs_dev, void* rwd_dev,
                      uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev, int32_t* sweeps_dev,
                      void* stream) {
  BCN_CHECK_KIND(h, BCN_RAYLEIGH);
  return BCN_BY_DTYPE(h->dtype, ns2d_step_t, h, actions_dev, nullptr, actions_norm_dev, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev,
                      sweeps_dev, stream);
}

// ---- mixing ----------------------------------------------------------------------------------
int bcn_mixing_create(const bcn_mixing_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->nx < 2 || c->ny < 2 || c->ndt_act < 0) { bcn_set_error("mixing cfg out of range"); return BCN_ERR_ARG; }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_mixing, c, batch, dtype, device, out);
}

int bcn_mixing_reset(bcn_env_t h, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_MIXING);
  return BCN_BY_DTYPE(h->dtype, ns2d_reset_t, h, nullptr, obs_dev, stream);
}

int bcn_mixing_step(bcn_env_t h, const int32_t* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev,
                    uint8_t* trunc_dev, int32_t* status_dev, int32_t* sweeps_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_MIXING);
  return BCN_BY_DTYPE(h->dtype, ns2d_step_t, h, nullptr, actions_dev, nullptr, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev, sweeps_dev,
                      stream);
}

// ---- 1D envs ---------------------------------------------------------------------------------
int bcn_burgers_create(const bcn_burgers_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->nx < 8 || c->nx > 8192 || c->ctrl_pos < c->n_obs_pts || c->ctrl_pos >= c->nx || c->n_obs_pts > 64) {
    bcn_set_error("burgers cfg out of range (8 <= nx <= 8192, n_obs_pts <= ctrl_pos < nx)");
    return BCN_ERR_ARG;
  }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_burgers, c, batch, dtype, device, out);
}
int bcn_burgers_reset(bcn_env_t h, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_BURGERS);
  return BCN_BY_DTYPE(h->dtype, env1d_reset_t, h, burgers_launch_reset, nullptr, obs_dev, stream);
}
int bcn_burgers_step(bcn_env_t h, const void* actions_dev, const void* noise_dev, void* obs_dev, void* rwd_dev,
                     uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_BURGERS);
  return BCN_BY_DTYPE(h->dtype, env1d_step_t, h, burgers_launch_step, actions_dev, noise_dev, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev,
                      stream);
}

int bcn_shkadov_create(const bcn_shkadov_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  const int last = c->jet_pos + (c->n_jets - 1) * c->jet_space;
  if (c->nx < 16 || c->nx > 8192 || c->n_jets < 1 || c->n_jets > 64 || 2 * c->jet_hw >= c->jet_space ||
      c->jet_pos - c->l_obs < 0 || c->jet_pos - c->jet_hw < 1 || last + c->l_rwd > c->nx ||
      last + c->jet_hw > c->nx - 2 || c->n_interp < 1) {
    bcn_set_error("shkadov cfg out of range (16 <= nx <= 8192, 1 <= n_jets <= 64, non-overlapping jets inside the domain)");
    return BCN_ERR_ARG;
  }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_shkadov, c, batch, dtype, device, out);
}
int bcn_shkadov_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_SHKADOV);
  return BCN_BY_DTYPE(h->dtype, env1d_reset_t, h, shkadov_launch_reset, init_fields_dev, obs_dev, stream);
}
int bcn_shkadov_reset_random(bcn_env_t h, const void* init_fields_dev, const int32_t* n_steps_dev, int rand_steps, int32_t* n_out_dev,
                             void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_SHKADOV);
  if (rand_steps < 0 || rand_steps > 65535) {
    bcn_set_error("bcn_shkadov_reset_random: rand_steps %d outside [0, 65535]", rand_steps);
    return BCN_ERR_ARG;
  }
  return BCN_BY_DTYPE(h->dtype, shkadov_reset_random_t, h, init_fields_dev, n_steps_dev, rand_steps, n_out_dev, obs_dev, stream);
}
int bcn_shkadov_step(bcn_env_t h, const void* actions_dev, const void* noise_dev, void* obs_dev, void* rwd_dev,
                     uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_SHKADOV);
  return BCN_BY_DTYPE(h->dtype, env1d_step_t, h, shkadov_launch_step, actions_dev, noise_dev, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev,
                      stream);
}

int bcn_sloshing_create(const bcn_sloshing_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->nx < 4 || c->nx + 2 > 8192 || c->n_interp < 1) { bcn_set_error("sloshing cfg out of range"); return BCN_ERR_ARG; }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_sloshing, c, batch, dtype, device, out);
}
int bcn_sloshing_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_SLOSHING);
  return BCN_BY_DTYPE(h->dtype, env1d_reset_t, h, sloshing_launch_reset, init_fields_dev, obs_dev, stream);
}
int bcn_sloshing_step(bcn_env_t h, const void* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev,
                      uint8_t* trunc_dev, int32_t* status_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_SLOSHING);
  return BCN_BY_DTYPE(h->dtype, env1d_step_t, h, sloshing_launch_step, actions_dev, nullptr, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev,
                      stream);
}

// ---- lorenz / vortex --------------------------------------------------------------------------
#define BCN_ODE_CALL(h, ...) BCN_BY_DTYPE(h->dtype, ode_call, h, __VA_ARGS__)

int bcn_lorenz_create(const bcn_lorenz_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->ndt_act < 1 || c->n_act < 1 || !(c->dt > 0)) { bcn_set_error("lorenz cfg out of range (ndt_act, n_act >= 1, dt > 0)"); return BCN_ERR_ARG; }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_lorenz, c, batch, dtype, device, out);
}
int bcn_lorenz_reset(bcn_env_t h, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_LORENZ);
  return BCN_ODE_CALL(h, true, nullptr, obs_dev, nullptr, nullptr, nullptr, nullptr, stream);
}
int bcn_lorenz_step(bcn_env_t h, const int32_t* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev, uint8_t* trunc_dev,
                    int32_t* status_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_LORENZ);
  return BCN_ODE_CALL(h, false, actions_dev, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev, stream);
}

int bcn_vortex_create(const bcn_vortex_cfg* c, int batch, int dtype, int device, bcn_env_t* out) {
  int rc = check_create(c, batch, dtype, device, out);
  if (rc) return rc;
  if (c->ndt_act < 1 || c->n_act < 1 || !(c->dt > 0) || !(c->omega_f != 0) || !(c->mass != 0) || !(c->re != 0) || !(c->re_crit != 0)) {
    bcn_set_error("vortex cfg out of range (ndt_act, n_act >= 1, dt > 0, omega_f, mass, re, re_crit nonzero)");
    return BCN_ERR_ARG;
  }
  DeviceGuard g(device);
  return BCN_BY_DTYPE(dtype, make_vortex, c, batch, dtype, device, out);
}
int bcn_vortex_reset(bcn_env_t h, void* obs_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_VORTEX);
  return BCN_ODE_CALL(h, true, nullptr, obs_dev, nullptr, nullptr, nullptr, nullptr, stream);
}
int bcn_vortex_step(bcn_env_t h, const void* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev, uint8_t* trunc_dev,
                    int32_t* status_dev, void* stream) {
  BCN_CHECK_KIND(h, BCN_VORTEX);
  return BCN_ODE_CALL(h, false, actions_dev, obs_dev, rwd_dev, done_dev, trunc_dev, status_dev, stream);
}

// ---- common ----------------------------------------------------------------------------------
int bcn_env_kind(bcn_env_t h) { return h ? h->kind : -1; }
int bcn_batch(bcn_env_t h) { return h ? h->batch : 0; }
int bcn_dtype(bcn_env_t h) { return h ? h->dtype : -1; }
int bcn_n_obs(bcn_env_t h) { return h ? h->n_obs : 0; }
int bcn_n_act(bcn_env_t h) { return h ? h->n_act : 0; }
int bcn_ndt_act(bcn_env_t h) { return h ? h->ndt_act : 0; }
int bcn_device(bcn_env_t h) { return h ? h->device : -1; }
size_t bcn_state_elems(bcn_env_t h) { return h ? h->state_elems() : 0; }

int bcn_get_state(bcn_env_t h, void* buf, int is_device, void* stream) {
  if (!h || !buf) { bcn_set_error("null handle/buffer"); return BCN_ERR_ARG; }
  DeviceGuard g(h->device);
  return h->get_state(buf, is_device, static_cast<hipStream_t>(stream));
}
int bcn_set_state(bcn_env_t h, const void* buf, int is_device, void* stream) {
  if (!h || !buf) { bcn_set_error("null handle/buffer"); return BCN_ERR_ARG; }
  DeviceGuard g(h->device);
  return h->set_state(buf, is_device, static_cast<hipStream_t>(stream));
}
int bcn_get_stp(bcn_env_t h, int32_t* buf_host, void* stream) {
  if (!h || !buf_host) { bcn_set_error("null handle/buffer"); return BCN_ERR_ARG; }
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BCN_HIP(hipMemcpyAsync(buf_host, h->stp, (size_t)h->batch * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  BCN_HIP(hipStreamSynchronize(s));
  return BCN_OK;
}
int bcn_set_stp(bcn_env_t h, const int32_t* buf_host, void* stream) {
  if (!h || !buf_host) { bcn_set_error("null handle/buffer"); return BCN_ERR_ARG; }
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BCN_HIP(hipMemcpyAsync(h->stp, buf_host, (size_t)h->batch * sizeof(int32_t), hipMemcpyHostToDevice, s));
  BCN_HIP(hipStreamSynchronize(s));
  return BCN_OK;
}
int bcn_set_mask(bcn_env_t h, const uint8_t* mask_dev) {
  if (!h) { bcn_set_error("null handle"); return BCN_ERR_ARG; }
  h->set_mask(mask_dev);
  return BCN_OK;
}
int bcn_set_variant(bcn_env_t h, int variant) { return h ? h->set_variant(variant) : 0; }
int bcn_get_counters(bcn_env_t h, uint64_t* buf_host, void* stream) {
  if (!h || !buf_host) { bcn_set_error("null handle/buffer"); return BCN_ERR_ARG; }
  DeviceGuard g(h->device);
  return h->get_counters(buf_host, static_cast<hipStream_t>(stream));
}
int bcn_get_counters_n(bcn_env_t h, uint64_t* buf_host, int words_per_replica, void* stream) {
  if (!h || !buf_host || words_per_replica < 1) { bcn_set_error("null handle/buffer or words_per_replica < 1"); return BCN_ERR_ARG; }
  if (words_per_replica == BCN_COUNTER_WORDS) return bcn_get_counters(h, buf_host, stream);
  std::vector<uint64_t> tmp((size_t)h->batch * BCN_COUNTER_WORDS);
  int rc = bcn_get_counters(h, tmp.data(), stream);
  if (rc) return rc;
  for (int b = 0; b < h->batch; b++)
    for (int k = 0; k < words_per_replica; k++)
      buf_host[(size_t)b * words_per_replica + k] = k < BCN_COUNTER_WORDS ? tmp[(size_t)b * BCN_COUNTER_WORDS + k] : 0;
  return BCN_OK;
}
int bcn_api_version(void) { return BCN_API_VERSION; }
int bcn_set_fast_plugin(bcn_env_t h, void* launch_fn, size_t scratch_elems) {
  if (!h) { bcn_set_error("null handle"); return BCN_ERR_ARG; }
  return h->set_fast_plugin(launch_fn, scratch_elems);
}
int bcn_set_fast_plugin_params(bcn_env_t h, void* launch_fn) {
  if (!h) { bcn_set_error("null handle"); return BCN_ERR_ARG; }
  return h->set_fast_plugin_params(launch_fn);
}
int bcn_set_noise(bcn_env_t h, double sigma, uint64_t seed, int64_t replica_offset) {
  if (!h) { bcn_set_error("null handle"); return BCN_ERR_ARG; }
  return h->set_noise(sigma, seed, replica_offset);
}
int bcn_set_option(bcn_env_t h, const char* name, int value) {
  if (!h || !name) { bcn_set_error("null handle/name"); return BCN_ERR_ARG; }
  return h->set_option(name, value);
}
int bcn_set_slow_mode_bound(bcn_env_t h, int n, const double* cutoff, const double* bound) {
  if (!h || n < 0 || n > 2 || (n > 0 && (!cutoff || !bound))) { bcn_set_error("bcn_set_slow_mode_bound: null handle/arrays or n outside 0..2"); return BCN_ERR_ARG; }
  return h->set_slow_mode_bound(n, cutoff, bound);
}
int bcn_get_slow_mode_bound(bcn_env_t h, double* cutoff, double* bound) {
  if (!h || !cutoff || !bound) { bcn_set_error("null handle/arrays"); return BCN_ERR_ARG; }
  return h->get_slow_mode_bound(cutoff, bound);
}
int bcn_set_sched(bcn_env_t h, int mode, int grid, int q, int lpt_min_batch) {
  if (!h) { bcn_set_error("null handle"); return BCN_ERR_ARG; }
  if (mode < -1 || mode > 2 || grid < 0 || q < 0 || lpt_min_batch < 0) { bcn_set_error("bcn_set_sched: argument out of range"); return BCN_ERR_ARG; }
  return h->set_sched(mode, grid, q, lpt_min_batch);
}
// ---- per-replica physical parameters ---------------------------------------------------------
int bcn_n_params(bcn_env_t h) {
  const BcnParamDesc* d = h ? bcn_param_desc(h->kind) : nullptr;
  return d ? d->n : 0;
}
const char* bcn_param_name(bcn_env_t h, int i) {
  const BcnParamDesc* d = h ? bcn_param_desc(h->kind) : nullptr;
  return d && i >= 0 && i < d->n ? d->name[i] : "";
}
int bcn_set_params(bcn_env_t h, const double* values_host, void* stream) {
  const BcnParamDesc* d = h ? bcn_param_desc(h->kind) : nullptr;
  if (!d) { bcn_set_error("bcn_set_params: null handle"); return BCN_ERR_ARG; }
  if (!values_host) {   // back to the cfg's values for every replica; the table stays allocated (a captured graph may hold its address)
    delete[] h->prm_host;
    h->prm_host = nullptr;
    h->use_params(nullptr);
    return BCN_OK;
  }
  const size_t B = (size_t)h->batch;
  // everything is checked before the device or the handle is touched
  for (int k = 0; k < d->n; k++)
    for (size_t b = 0; b < B; b++) {
      const double v = values_host[(size_t)k * B + b];
      if (!isfinite(v)) { bcn_set_error("bcn_set_params: %s of replica %zu is not finite (%g)", d->name[k], b, v); return BCN_ERR_ARG; }
      if (d->positive[k] && !(v > 0.0)) { bcn_set_error("bcn_set_params: %s of replica %zu must be > 0 (%g)", d->name[k], b, v); return BCN_ERR_ARG; }
    }
  std::vector<char> table;
  BCN_BY_DTYPE(h->dtype, params_table, h, values_host, table);
  double* keep = new (std::nothrow) double[(size_t)d->n * B];
  if (!keep) { bcn_set_error("out of host memory"); return BCN_ERR_ARG; }
  memcpy(keep, values_host, (size_t)d->n * B * sizeof(double));
  DeviceGuard g(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!h->prm_dev) {
    hipError_t e = hipMalloc(&h->prm_dev, table.size());
    if (e != hipSuccess) { delete[] keep; h->prm_dev = nullptr; bcn_set_error("hipMalloc(%zu): %s", table.size(), hipGetErrorString(e)); return BCN_ERR_HIP; }
  }
  // in place, in stream order: a graph captured after the first call reads the new values at its next replay
  hipError_t e = hipMemcpyAsync(h->prm_dev, table.data(), table.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // `table` is a temporary
  if (e != hipSuccess) { delete[] keep; bcn_set_error("bcn_set_params: copy to the device: %s", hipGetErrorString(e)); return BCN_ERR_HIP; }
  delete[] h->prm_host;
  h->prm_host = keep;
  h->use_params(h->prm_dev);
  return BCN_OK;
}
int bcn_get_params(bcn_env_t h, double* values_host) {
  const BcnParamDesc* d = h ? bcn_param_desc(h->kind) : nullptr;
  if (!d || !values_host) { bcn_set_error("bcn_get_params: null handle/buffer"); return BCN_ERR_ARG; }
  const size_t B = (size_t)h->batch;
  for (int k = 0; k < d->n; k++)
    for (size_t b = 0; b < B; b++) values_host[(size_t)k * B + b] = h->prm_host ? h->prm_host[(size_t)k * B + b] : h->prm_cfg[k];
  return BCN_OK;
}
int bcn_derive_params_host(int kind, const double* params, const double* aux, double* derived) {
  const BcnParamDesc* d = bcn_param_desc(kind);
  if (!d || !params || !aux || !derived) { bcn_set_error("bcn_derive_params_host: unknown kind or null array"); return -1; }
  bcn_derive_params(kind, params, aux, derived);
  return d->n_derived;
}
// ---- snapshots -------------------------------------------------------------------------------
size_t bcn_snapshot_bytes_n(bcn_env_t h, int n) {
  size_t bytes = 0;
  if (!h || n < 1 || snap_build(h, n, nullptr, nullptr, nullptr, 0, &bytes) < 0) return 0;
  return bytes;
}
size_t bcn_snapshot_bytes(bcn_env_t h) { return h ? bcn_snapshot_bytes_n(h, h->batch) : 0; }
int bcn_snapshot_layout(bcn_env_t h, int n, bcn_snapshot_seg* segs, int max_segs) {
  if (!h || n < 1 || (max_segs > 0 && !segs)) { bcn_set_error("bcn_snapshot_layout: null handle/array or n < 1"); return 0; }
  const int nd = snap_build(h, n, nullptr, nullptr, segs, max_segs, nullptr);
  return nd < 0 ? 0 : nd;
}
uint64_t bcn_snapshot_signature(bcn_env_t h) {
  if (!h) return 0;
  bcn_snapshot_seg lay[16];
  const int nd = snap_build(h, 1, nullptr, nullptr, lay, 16, nullptr);
  const int32_t head[2] = {h->kind, h->dtype};
  uint64_t sig = snap_fnv(14695981039346656037ull, head, sizeof(head));
  sig = snap_fnv(sig, &h->cfg_hash, sizeof(h->cfg_hash));
  for (int k = 0; k < nd && k < 16; k++) {
    sig = snap_fnv(sig, lay[k].name, sizeof(lay[k].name));
    sig = snap_fnv(sig, &lay[k].elem, sizeof(int32_t));
    sig = snap_fnv(sig, &lay[k].planes, sizeof(int32_t));
    sig = snap_fnv(sig, &lay[k].row_elems, sizeof(int64_t));
  }
  return sig;
}
static int snap_ptr_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int bcn_snapshot_save(bcn_env_t h, void* snap_dev, const void* out_buf_dev, void* stream) {
  if (!h || !snap_dev) { bcn_set_error("bcn_snapshot_save: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(snap_dev) || !snap_ptr_ok(out_buf_dev)) { bcn_set_error("bcn_snapshot_save: buffers must be 16-byte aligned"); return BCN_ERR_ARG; }
  SnapTable t;
  if (snap_build(h, h->batch, static_cast<char*>(const_cast<void*>(out_buf_dev)), &t, nullptr, 0, nullptr) < 0) return BCN_ERR_ARG;
  DeviceGuard g(h->device);
  return snapshot_launch(t, false, static_cast<char*>(snap_dev), nullptr, nullptr, static_cast<hipStream_t>(stream));
}
int bcn_snapshot_load(bcn_env_t h, const void* snap_dev, int n_src, const int32_t* src_dev, const uint8_t* mask_dev,
                      void* out_buf_dev, void* stream) {
  if (!h || !snap_dev) { bcn_set_error("bcn_snapshot_load: null handle/buffer"); return BCN_ERR_ARG; }
  if (n_src < 1 || (!src_dev && n_src != h->batch)) {
    bcn_set_error("bcn_snapshot_load: a snapshot of %d replicas into a batch of %d needs a source index per replica", n_src, h->batch);
    return BCN_ERR_ARG;
  }
  if (!snap_ptr_ok(snap_dev) || !snap_ptr_ok(out_buf_dev)) { bcn_set_error("bcn_snapshot_load: buffers must be 16-byte aligned"); return BCN_ERR_ARG; }
  SnapTable t;
  if (snap_build(h, n_src, static_cast<char*>(out_buf_dev), &t, nullptr, 0, nullptr) < 0) return BCN_ERR_ARG;
  DeviceGuard g(h->device);
  return snapshot_launch(t, true, static_cast<char*>(const_cast<void*>(snap_dev)), src_dev, mask_dev, static_cast<hipStream_t>(stream));
}
// ---- episode statistics (episode.h) ------------------------------------------------------------
size_t bcn_episode_bytes(bcn_env_t h) {
  if (!h) { bcn_set_error("bcn_episode_bytes: null handle"); return 0; }
  return built_bytes(episode_build, h);
}
int bcn_episode_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs) {
  if (!h || (max_segs > 0 && !segs)) { bcn_set_error("bcn_episode_layout: null handle/array"); return 0; }
  return built_layout(episode_build, h, segs, max_segs);
}
int bcn_episode_track(bcn_env_t h, const void* out_buf_dev, void* ep_buf_dev, const uint8_t* mask_dev, void* stream) {
  if (!h || !out_buf_dev || !ep_buf_dev) { bcn_set_error("bcn_episode_track: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(out_buf_dev) || !snap_ptr_ok(ep_buf_dev)) { bcn_set_error("bcn_episode_track: buffers must be 16-byte aligned"); return BCN_ERR_ARG; }
  bcn_snapshot_seg lay[BCN_EP_NSEG];
  if (episode_build(h, lay, BCN_EP_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  const size_t B = (size_t)h->batch, row = (size_t)h->n_obs * h->esz;
  const bcn_out_layout_t o = bcn_out_layout(B, (size_t)h->n_obs, h->esz);
  const char* out = static_cast<const char*>(out_buf_dev);
  char* ep = static_cast<char*>(ep_buf_dev);
  EpisodeArgs a;
  a.obs = out; a.rwd = out + o.rwd;
  a.done = reinterpret_cast<const uint8_t*>(out + o.done); a.trunc = reinterpret_cast<const uint8_t*>(out + o.trunc);
  a.mask = mask_dev;
  a.ret = ep + lay[EP_RET].offset; a.len = reinterpret_cast<int32_t*>(ep + lay[EP_LEN].offset);
  a.last_ret = ep + lay[EP_LAST_RET].offset; a.last_len = reinterpret_cast<int32_t*>(ep + lay[EP_LAST_LEN].offset);
  a.count = reinterpret_cast<int32_t*>(ep + lay[EP_COUNT].offset); a.sum_ret = reinterpret_cast<double*>(ep + lay[EP_SUM_RET].offset);
  a.sum_len = reinterpret_cast<long long*>(ep + lay[EP_SUM_LEN].offset); a.finished = reinterpret_cast<uint8_t*>(ep + lay[EP_FINISHED].offset);
  a.final_obs = ep + lay[EP_FINAL_OBS].offset;
  a.batch = (unsigned)B;
  a.nbk = (unsigned)((B + BCN_EP_NT - 1) / BCN_EP_NT);
  a.unit = copy_unit(row);      // rows are reals: multiples of 4 bytes
  a.upr = (unsigned)(row / a.unit);
  a.total = (unsigned)(B * a.upr);
  a.f64 = h->dtype == BCN_F64;
  DeviceGuard g(h->device);
  return episode_launch(a, static_cast<hipStream_t>(stream));
}
// ---- per-jet rewards and returns of shkadov (shkadov_jets.h) --------------------------------------
size_t bcn_shkadov_jets_bytes(bcn_env_t h) {
  if (!h) { bcn_set_error("bcn_shkadov_jets_bytes: null handle"); return 0; }
  if (h->kind != BCN_SHKADOV) { bcn_set_error("bcn_shkadov_jets_bytes: handle is not a BCN_SHKADOV env"); return 0; }
  return built_bytes(jets_build, h);
}
int bcn_shkadov_jets_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs) {
  if (!h || (max_segs > 0 && !segs)) { bcn_set_error("bcn_shkadov_jets_layout: null handle/array"); return 0; }
  if (h->kind != BCN_SHKADOV) { bcn_set_error("bcn_shkadov_jets_layout: handle is not a BCN_SHKADOV env"); return 0; }
  return built_layout(jets_build, h, segs, max_segs);
}
int bcn_shkadov_jet_rewards(bcn_env_t h, const void* out_buf_dev, void* jets_buf_dev, int with_stats, void* stream) {
  if (!h || !out_buf_dev || !jets_buf_dev) { bcn_set_error("bcn_shkadov_jet_rewards: null handle/buffer"); return BCN_ERR_ARG; }
  if (h->kind != BCN_SHKADOV) { bcn_set_error("bcn_shkadov_jet_rewards: handle is not a BCN_SHKADOV env"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(out_buf_dev) || !snap_ptr_ok(jets_buf_dev)) {
    bcn_set_error("bcn_shkadov_jet_rewards: buffers must be 16-byte aligned");
    return BCN_ERR_ARG;
  }
  bcn_snapshot_seg lay[BCN_JETS_NSEG];
  if (jets_build(h, lay, BCN_JETS_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  return BCN_BY_DTYPE(h->dtype, shkadov_jets_t, h, static_cast<const char*>(out_buf_dev), static_cast<char*>(jets_buf_dev), lay, with_stats, stream);
}
// ---- running normalisation of observations and rewards (normalize.h) ------------------------------
size_t bcn_normalize_bytes(bcn_env_t h) {
  if (!h) { bcn_set_error("bcn_normalize_bytes: null handle"); return 0; }
  return built_bytes(normalize_build, h);
}
int bcn_normalize_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs) {
  if (!h || (max_segs > 0 && !segs)) { bcn_set_error("bcn_normalize_layout: null handle/array"); return 0; }
  return built_layout(normalize_build, h, segs, max_segs);
}
int bcn_normalize(bcn_env_t h, const void* out_buf_dev, void* norm_buf_dev, const void* ep_buf_dev, const uint8_t* mask_dev, int kind,
                  int training, double gamma, double eps, double clip_obs, double clip_rwd, void* stream) {
  if (!h || !out_buf_dev || !norm_buf_dev) { bcn_set_error("bcn_normalize: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(out_buf_dev) || !snap_ptr_ok(norm_buf_dev) || !snap_ptr_ok(ep_buf_dev)) {
    bcn_set_error("bcn_normalize: buffers must be 16-byte aligned");
    return BCN_ERR_ARG;
  }
  if (kind != BCN_NORM_STEP && kind != BCN_NORM_RESET) { bcn_set_error("bcn_normalize: kind %d is neither BCN_NORM_STEP nor BCN_NORM_RESET", kind); return BCN_ERR_ARG; }
  if (!(gamma >= 0.0 && gamma <= 1.0) || !(eps > 0.0) || !(clip_obs > 0.0) || !(clip_rwd > 0.0)) {
    bcn_set_error("bcn_normalize: gamma %g must lie in [0, 1], eps %g, clip_obs %g and clip_rwd %g must be > 0", gamma, eps, clip_obs, clip_rwd);
    return BCN_ERR_ARG;
  }
  bcn_snapshot_seg lay[BCN_NRM_NSEG], el[BCN_EP_NSEG];
  if (normalize_build(h, lay, BCN_NRM_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  if (ep_buf_dev && episode_build(h, el, BCN_EP_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  const size_t B = (size_t)h->batch, n = (size_t)h->n_obs;
  const bcn_out_layout_t o = bcn_out_layout(B, n, h->esz);
  const NormalizeShape sh = normalize_shape(B, n);
  const char* out = static_cast<const char*>(out_buf_dev);
  const char* ep = static_cast<const char*>(ep_buf_dev);
  char* nb = static_cast<char*>(norm_buf_dev);
  NormalizeArgs a;
  a.obs = out + o.obs; a.rwd = out + o.rwd;
  a.status = reinterpret_cast<const int32_t*>(out + o.status);
  a.done = reinterpret_cast<const uint8_t*>(out + o.done); a.trunc = reinterpret_cast<const uint8_t*>(out + o.trunc);
  a.mask = mask_dev;
  a.finished = ep ? reinterpret_cast<const uint8_t*>(ep + el[EP_FINISHED].offset) : nullptr;
  a.final_obs = ep ? ep + el[EP_FINAL_OBS].offset : nullptr;
  a.obs_mean = reinterpret_cast<double*>(nb + lay[NRM_OBS_MEAN].offset); a.obs_var = reinterpret_cast<double*>(nb + lay[NRM_OBS_VAR].offset);
  a.obs_count = reinterpret_cast<double*>(nb + lay[NRM_OBS_COUNT].offset); a.ret_mean = reinterpret_cast<double*>(nb + lay[NRM_RET_MEAN].offset);
  a.ret_var = reinterpret_cast<double*>(nb + lay[NRM_RET_VAR].offset); a.ret_count = reinterpret_cast<double*>(nb + lay[NRM_RET_COUNT].offset);
  a.ret = reinterpret_cast<double*>(nb + lay[NRM_RET].offset);
  a.norm_obs = nb + lay[NRM_NORM_OBS].offset; a.norm_rwd = nb + lay[NRM_NORM_RWD].offset;
  a.norm_final_obs = nb + lay[NRM_NORM_FINAL_OBS].offset;
  a.prev = reinterpret_cast<double*>(nb + lay[NRM_SCRATCH].offset);
  a.part = a.prev + 2 * (n + 1) + 2;
  a.batch = (unsigned)B; a.n_obs = (unsigned)n;
  a.w = sh.w; a.R = sh.R; a.chunks = sh.chunks; a.S = sh.S; a.G = sh.G;
  a.f64 = h->dtype == BCN_F64;
  a.kind = kind == BCN_NORM_RESET ? BCN_NRM_RESET : BCN_NRM_STEP;
  a.training = training != 0;
  a.gamma = gamma; a.eps = eps; a.clip_obs = clip_obs; a.clip_rwd = clip_rwd;
  DeviceGuard g(h->device);
  return normalize_launch(a, static_cast<hipStream_t>(stream));
}
// ---- rollout storage and generalised advantage estimation (rollout.h) -----------------------------
size_t bcn_rollout_bytes(bcn_env_t h, int T, int flags) {
  if (!h) { bcn_set_error("bcn_rollout_bytes: null handle"); return 0; }
  size_t bytes = 0;
  return rollout_build("bcn_rollout_bytes", h, T, flags, nullptr, 0, &bytes) < 0 ? 0 : bytes;
}
int bcn_rollout_layout(bcn_env_t h, int T, int flags, bcn_snapshot_seg* segs, int max_segs) {
  if (!h || (max_segs > 0 && !segs)) { bcn_set_error("bcn_rollout_layout: null handle/array"); return 0; }
  const int nd = rollout_build("bcn_rollout_layout", h, T, flags, segs, max_segs, nullptr);
  return nd < 0 ? 0 : nd;
}
int bcn_rollout_begin(bcn_env_t h, void* ro_buf_dev, const void* out_buf_dev, const void* norm_buf_dev, void* stream) {
  if (!h || !ro_buf_dev || !out_buf_dev) { bcn_set_error("bcn_rollout_begin: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(ro_buf_dev) || !snap_ptr_ok(out_buf_dev) || !snap_ptr_ok(norm_buf_dev)) {
    bcn_set_error("bcn_rollout_begin: buffers must be 16-byte aligned");
    return BCN_ERR_ARG;
  }
  bcn_snapshot_seg lay[BCN_RO_NSEG], nl[BCN_NRM_NSEG];
  if (rollout_build("bcn_rollout_begin", h, 1, 0, lay, BCN_RO_NSEG, nullptr) < 0) return BCN_ERR_ARG;   // cursor and obs sit in front of whatever T scales
  if (norm_buf_dev && normalize_build(h, nl, BCN_NRM_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  const size_t B = (size_t)h->batch, row = (size_t)h->n_obs * h->esz;
  char* ro = static_cast<char*>(ro_buf_dev);
  const char* obs = norm_buf_dev ? static_cast<const char*>(norm_buf_dev) + nl[NRM_NORM_OBS].offset
                                 : static_cast<const char*>(out_buf_dev) + bcn_out_layout(B, (size_t)h->n_obs, h->esz).obs;
  unsigned blk = 0;
  const RolloutJob j = rollout_job(obs, ro + lay[RO_OBS].offset, B, row, RO_COPY_ALWAYS, 0, &blk);
  DeviceGuard g(h->device);
  return rollout_begin_launch(reinterpret_cast<int32_t*>(ro + lay[RO_CURSOR].offset), j, static_cast<hipStream_t>(stream));
}
int bcn_rollout_record(bcn_env_t h, const void* out_buf_dev, void* ro_buf_dev, const void* act_dev, const void* ep_buf_dev,
                       const void* norm_buf_dev, const void* jets_buf_dev, const uint8_t* mask_dev, int T, int flags, void* stream) {
  if (!h || !out_buf_dev || !ro_buf_dev) { bcn_set_error("bcn_rollout_record: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(out_buf_dev) || !snap_ptr_ok(ro_buf_dev) || !snap_ptr_ok(ep_buf_dev) || !snap_ptr_ok(norm_buf_dev) ||
      !snap_ptr_ok(jets_buf_dev)) {
    bcn_set_error("bcn_rollout_record: buffers must be 16-byte aligned");
    return BCN_ERR_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(act_dev) & 3) != 0) { bcn_set_error("bcn_rollout_record: actions must be 4-byte aligned"); return BCN_ERR_ARG; }
  bcn_snapshot_seg lay[BCN_RO_NSEG], el[BCN_EP_NSEG], nl[BCN_NRM_NSEG], jl[BCN_JETS_NSEG];
  if (rollout_build("bcn_rollout_record", h, T, flags, lay, BCN_RO_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  if (jets_buf_dev && !(flags & BCN_RO_JETS)) { bcn_set_error("bcn_rollout_record: a per-jet buffer without BCN_RO_JETS"); return BCN_ERR_ARG; }
  if (ep_buf_dev && episode_build(h, el, BCN_EP_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  if (norm_buf_dev && normalize_build(h, nl, BCN_NRM_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  if (jets_buf_dev && jets_build(h, jl, BCN_JETS_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  const size_t B = (size_t)h->batch, n = (size_t)h->n_obs, esz = h->esz;
  const bcn_out_layout_t o = bcn_out_layout(B, n, esz);
  const char* out = static_cast<const char*>(out_buf_dev);
  const char* ep = static_cast<const char*>(ep_buf_dev);
  const char* nb = static_cast<const char*>(norm_buf_dev);
  char* ro = static_cast<char*>(ro_buf_dev);
  RolloutRecordArgs a;
  a.cursor = reinterpret_cast<int32_t*>(ro + lay[RO_CURSOR].offset);
  a.rwd = nb ? nb + nl[NRM_NORM_RWD].offset : out + o.rwd;
  a.status = reinterpret_cast<const int32_t*>(out + o.status);
  a.done = reinterpret_cast<const uint8_t*>(out + o.done); a.trunc = reinterpret_cast<const uint8_t*>(out + o.trunc);
  a.mask = mask_dev;
  a.finished = ep ? reinterpret_cast<const uint8_t*>(ep + el[EP_FINISHED].offset) : nullptr;
  a.d_rwd = ro + lay[RO_RWD].offset; a.d_status = reinterpret_cast<int32_t*>(ro + lay[RO_STATUS].offset);
  a.d_done = reinterpret_cast<uint8_t*>(ro + lay[RO_DONE].offset); a.d_trunc = reinterpret_cast<uint8_t*>(ro + lay[RO_TRUNC].offset);
  a.d_valid = reinterpret_cast<uint8_t*>(ro + lay[RO_VALID].offset);
  unsigned blk = 0, nj = 0;
  const char* obs = nb ? nb + nl[NRM_NORM_OBS].offset : out + o.obs;
  a.job[nj++] = rollout_job(obs, ro + lay[RO_OBS].offset, B, n * esz, RO_COPY_ALWAYS, 1, &blk);
  if (ep && (flags & BCN_RO_FINAL_OBS)) {
    const char* fo = nb ? nb + nl[NRM_NORM_FINAL_OBS].offset : ep + el[EP_FINAL_OBS].offset;
    a.job[nj++] = rollout_job(fo, ro + lay[RO_FINAL_OBS].offset, B, n * esz, RO_COPY_FINISHED, 0, &blk);
  }
  const size_t act_row = rollout_int_actions(h) ? 4 : (size_t)h->n_act * esz;
  a.job[nj++] = rollout_job(static_cast<const char*>(act_dev), ro + lay[RO_ACT].offset, B, act_row, RO_COPY_STEPPED, 0, &blk);
  if (jets_buf_dev)
    a.job[nj++] = rollout_job(static_cast<const char*>(jets_buf_dev) + jl[JETS_RWD_JETS].offset, ro + lay[RO_RWD_JETS].offset, B,
                              (size_t)h->n_act * esz, RO_COPY_ALWAYS, 0, &blk);
  for (; nj < BCN_RO_NJOB; nj++) {               // off: no workgroup reaches it
    a.job[nj] = RolloutJob{};
    a.job[nj].blk0 = blk;
  }
  a.batch = (unsigned)B;
  a.nbk = (unsigned)((B + BCN_RO_NT - 1) / BCN_RO_NT);
  a.ncp = blk;
  a.T = T;
  a.f64 = h->dtype == BCN_F64;
  DeviceGuard g(h->device);
  return rollout_record_launch(a, static_cast<hipStream_t>(stream));
}
int bcn_rollout_gae(bcn_env_t h, void* ro_buf_dev, const void* values_dev, const void* last_value_dev, const void* final_values_dev,
                    int T, int flags, int cols, double gamma, double lam, void* stream) {
  if (!h || !ro_buf_dev || !values_dev || !last_value_dev) { bcn_set_error("bcn_rollout_gae: null handle/buffer"); return BCN_ERR_ARG; }
  if (!snap_ptr_ok(ro_buf_dev)) { bcn_set_error("bcn_rollout_gae: buffers must be 16-byte aligned"); return BCN_ERR_ARG; }
  bcn_snapshot_seg lay[BCN_RO_NSEG];
  if (rollout_build("bcn_rollout_gae", h, T, flags, lay, BCN_RO_NSEG, nullptr) < 0) return BCN_ERR_ARG;
  if (cols != 1 && !((flags & BCN_RO_JETS) && cols == h->n_act)) {
    bcn_set_error("bcn_rollout_gae: cols = %d; 1, or the jet count with BCN_RO_JETS", cols);
    return BCN_ERR_ARG;
  }
  if (!(gamma >= 0.0 && gamma <= 1.0) || !(lam >= 0.0 && lam <= 1.0)) {
    bcn_set_error("bcn_rollout_gae: gamma %g and lam %g must lie in [0, 1]", gamma, lam);
    return BCN_ERR_ARG;
  }
  char* ro = static_cast<char*>(ro_buf_dev);
  RolloutGaeArgs a;
  a.cursor = reinterpret_cast<const int32_t*>(ro + lay[RO_CURSOR].offset);
  a.rwd = ro + lay[cols == 1 ? RO_RWD : RO_RWD_JETS].offset;
  a.done = reinterpret_cast<const uint8_t*>(ro + lay[RO_DONE].offset); a.trunc = reinterpret_cast<const uint8_t*>(ro + lay[RO_TRUNC].offset);
  a.valid = reinterpret_cast<const uint8_t*>(ro + lay[RO_VALID].offset);
  a.values = values_dev; a.last_value = last_value_dev; a.final_values = final_values_dev;
  a.adv = ro + lay[RO_ADV].offset; a.ret = ro + lay[RO_RET].offset;
  a.batch = (unsigned)h->batch; a.cols = (unsigned)cols; a.ncols = a.batch * a.cols;
  a.T = T;
  a.f64 = h->dtype == BCN_F64;
  a.gamma = gamma; a.lam = lam;
  DeviceGuard g(h->device);
  return rollout_gae_launch(a, static_cast<hipStream_t>(stream));
}
// ---- frames (render.h) ------------------------------------------------------------------------------
int bcn_render_shape(bcn_env_t h, const bcn_render_cfg* cfg, int* H_px, int* W_px) {
  if (!h || !cfg || !H_px || !W_px) { bcn_set_error("bcn_render_shape: null handle/argument"); return BCN_ERR_ARG; }
  RenderArgs a;
  const int rc = BCN_BY_DTYPE(h->dtype, render_fill, "bcn_render_shape", h, cfg, a);
  if (rc) return rc;
  *H_px = a.H + a.strip; *W_px = a.W;
  return BCN_OK;
}
int bcn_render(bcn_env_t h, const bcn_render_cfg* cfg, const uint8_t* lut_dev, const int32_t* replicas_dev, int n, uint8_t* rgb_dev, void* stream) {
  if (!h || !cfg) { bcn_set_error("bcn_render: null handle/cfg"); return BCN_ERR_ARG; }
  RenderArgs a;
  const int rc = BCN_BY_DTYPE(h->dtype, render_fill, "bcn_render", h, cfg, a);
  if (rc) return rc;
  if (n < 0 || (!replicas_dev && n != h->batch)) { bcn_set_error("bcn_render: n = %d frames; n >= 0, and the batch (%d) without an index list", n, h->batch); return BCN_ERR_ARG; }
  if (n > 0 && !rgb_dev) { bcn_set_error("bcn_render: null frame buffer"); return BCN_ERR_ARG; }
  if (!a.line && (!lut_dev || (reinterpret_cast<uintptr_t>(lut_dev) & 3) != 0)) { bcn_set_error("bcn_render: the field panel needs a 4-byte aligned colour table"); return BCN_ERR_ARG; }
  if ((reinterpret_cast<uintptr_t>(replicas_dev) & 3) != 0) { bcn_set_error("bcn_render: the index list must be 4-byte aligned"); return BCN_ERR_ARG; }
  a.lut = lut_dev; a.replicas = replicas_dev; a.n = n; a.rgb = rgb_dev;
  DeviceGuard g(h->device);
  return render_launch(a, static_cast<hipStream_t>(stream));
}
const char* bcn_kernel_name(bcn_env_t h) { return h ? h->kernel_name() : ""; }
// 1 where the next variant-1 step of a 2D handle goes through the kernels of ns2d_fast_runs.hip (option "cell_runs"; for the tests: both
// units' kernels carry the same names).  Default visibility like bcn_jit_builtin: no part of the ABI of include/beacon_hip.h.
extern "C" __attribute__((visibility("default"))) int bcn_cell_runs_active(bcn_env_t h) { return h ? h->cell_runs_active() : 0; }
int bcn_kernel_shape(bcn_env_t h, int* cells_per_thread, int* threads) {
  if (!h || !cells_per_thread || !threads) { bcn_set_error("bcn_kernel_shape: null argument"); return BCN_ERR_ARG; }
  h->kernel_shape(cells_per_thread, threads);
  return BCN_OK;
}
int bcn_destroy(bcn_env_t h) {
  if (!h) return BCN_OK;
  {
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    if (h->prm_dev) (void)hipFree(h->prm_dev);
  }
  delete h;
  return BCN_OK;
}
const char* bcn_last_error(void) { return g_err; }
const char* bcn_version(void) { return "beacon_hip 0.1 (gfx950)"; }

}  // extern "C"

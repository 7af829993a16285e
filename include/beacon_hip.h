/*
 * beacon_hip.h -- C ABI of libbeacon_hip.so: the MI355X-native batched stepper that
 * replaces the per-env solver hot path of jviquerat/beacon.
 *
 * The reference has no FFI: its boundary is a duck-typed Gym env class, one instance
 * per env.  Each entry point below stands in for one method of that
 * class, batched over B independent replicas, and cites the reference method it
 * replaces (file:line into /root/reference/beacon/).  Plain C types only; every
 * pointer named *_dev is a DEVICE pointer in the handle's dtype (BCN_F32 -> float,
 * BCN_F64 -> double) unless a type is spelled out; `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Calls on one handle must be serialised by the caller
 * (the reference env is not thread-safe either).  No call blocks on the GPU except
 * bcn_get_state/bcn_set_state with host pointers, and *_destroy.
 *
 * Precision (measured on MI355X in round 4 against the float64 reference / its C restatement; the tests assert <= 10 x these
 * figures, tests/test_gpu_parity.py: table F32, EPISODE_TOL, shkadov_tol):
 *   BCN_F64: rayleigh / mixing fields and observations within 1e-9 with the reference's Jacobi sweep counts (measured 3e-15 ..
 *            6e-15 over 400 timesteps); burgers, shkadov, sloshing fields bit-identical (rewards, being reductions, 1e-13).
 *   BCN_F32, one action step: rayleigh 128x64 (200 timesteps, ~94 sweeps each) u, v 4e-7, T, p 1.3e-6, observations 1.2e-6,
 *            reward (Nusselt number) 4e-6, every sweep count equal; mixing 100x100 (250 timesteps) u, v, C 2.5e-6, p 1.1e-5,
 *            observations 1.2e-6, reward 2e-8; burgers observations 4e-6 on average (one step of a 200-step episode at 5e-5);
 *            sloshing observations 8e-6; shkadov observations 1e-6 .. 2e-6, growing 1.4 x per action step (the film is chaotic).
 *   BCN_F32, a whole 100-step episode against BCN_F64: rayleigh observations 2.3e-5 for the median replica, 2.5e-3 for the
 *            worst one in its most sensitive transient (the flow amplifies rounding-level differences ~3000 x there: two
 *            float64 kernels drift apart with the same profile), 7e-5 at the end of the episode; mixing 1.8e-4 (median) /
 *            8.5e-4 (worst probe), rewards 1e-5; shkadov: trajectories decorrelate after ~40 steps, episode-return statistics
 *            over 64 replicas agree to 3e-4 sigma.
 *
 * Return value: 0 = BCN_OK, otherwise a BCN_ERR_* code; bcn_last_error() gives text.
 * Solver failures never exit the process (the reference does: rayleigh.py:221-224);
 * they are reported per replica in status_dev (BCN_ST_* bits).
 */
#ifndef BEACON_HIP_H
#define BEACON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCN_API __attribute__((visibility("default")))

/* Bumped whenever the size of a caller-provided buffer or a struct layout changes; bcn_api_version() returns the value
 * the loaded library was built with, so a caller compiled against an older header can refuse to run.
 *   4: bcn_get_counters writes BCN_COUNTER_WORDS = 4 words per replica (2 before); bcn_get_counters_n takes the count. */
#define BCN_API_VERSION 4
#define BCN_COUNTER_WORDS 4

typedef struct bcn_env_s* bcn_env_t;

enum { BCN_F32 = 0, BCN_F64 = 1 };
enum { BCN_OK = 0, BCN_ERR_ARG = 1, BCN_ERR_HIP = 2, BCN_ERR_UNSUPPORTED = 3 };
/* per-replica status word written by *_step */
enum { BCN_ST_OK = 0, BCN_ST_ITMAX = 1, BCN_ST_BLOWUP = 2,
       BCN_ST_PLAN = 4 /* diagnostic (bcn_set_option "verify_conv"): a Jacobi sweep the residual-evaluation plan skips passed the test */ };
/* env kinds (bcn_env_kind) */
enum { BCN_RAYLEIGH = 0, BCN_MIXING = 1, BCN_BURGERS = 2, BCN_SHKADOV = 3, BCN_SLOSHING = 4, BCN_LORENZ = 5, BCN_VORTEX = 6 };

/* ---- rayleigh: rayleigh/rayleigh.py -------------------------------------------------- */
/* ctor kwargs + the derived quantities of rayleigh.__init__ (rayleigh.py:20-56) */
typedef struct {
  int32_t nx, ny;                 /* int(50 L), int(50 H) */
  int32_t ndt_act, n_act;         /* 200, 100 */
  int32_t n_sgts, nx_sgts;        /* 10, nx // n_sgts */
  int32_t nx_obs_pts, ny_obs_pts; /* 4 int(L), 4 int(H) */
  int32_t nx_obs, ny_obs;         /* nx // nx_obs_pts, ny // ny_obs_pts */
  int32_t n_obs_steps;            /* 4 */
  int32_t itmax;                  /* 300000 (rayleigh.py:417) */
  double dx, dy, dt;
  double pr, ra, Tc, Th, C;       /* 0.71, 1e4, -0.5, 0.5, 0.75 */
  double tol;                     /* 1e-8 (rayleigh.py:414) */
} bcn_rayleigh_cfg;

/* replaces rayleigh.__init__ (rayleigh.py:20-86); batch = number of replicas on this device */
BCN_API int bcn_rayleigh_create(const bcn_rayleigh_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces rayleigh.reset (rayleigh.py:89-128).  init_fields_dev: [4][ny+2][nx+2] (u,v,p,T; x fastest)
 * shared by all replicas, or NULL for all-zero fields (init=False).  obs_dev[B][n_obs] may be NULL. */
BCN_API int bcn_rayleigh_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream);
/* replaces rayleigh.step (rayleigh.py:138-157) incl. solve/get_obs/get_rwd (:160-275).
 * actions_dev[B][n_sgts] raw actions, NULL = repeat last (a=None, :162); on return
 * actions_norm_dev[B][n_sgts] (may be NULL) holds the conditioned actions the reference writes
 * back into the caller's list (:165-168).  obs_dev[B][n_obs], rwd_dev[B], done_dev/trunc_dev
 * uint8[B], status_dev int32[B], sweeps_dev int32[B][ndt_act] Jacobi sweeps per timestep (NULL ok). */
BCN_API int bcn_rayleigh_step(bcn_env_t h, const void* actions_dev, void* actions_norm_dev, void* obs_dev,
                      void* rwd_dev, uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev,
                      int32_t* sweeps_dev, void* stream);

/* ---- mixing: mixing/mixing.py -------------------------------------------------------- */
typedef struct {
  int32_t nx, ny;                 /* int(100 L), int(100 H) */
  int32_t ndt_act, n_act;         /* 250, 100 */
  int32_t nx_obs_pts, ny_obs_pts, nx_obs, ny_obs, n_obs_steps;
  int32_t itmax;                  /* 300000 (mixing.py:426) */
  int32_t i_min, i_max, j_min, j_max; /* initial patch, ARRAY indices (mixing.py:90-94) */
  double dx, dy, dt;
  double re, pe, u_max, C0, ref_c; /* ref_c = side^2/(L H) C0 (mixing.py:261) */
  double tol;                     /* 1e-4 (mixing.py:423) */
} bcn_mixing_cfg;

/* replaces mixing.__init__ (mixing.py:20-70) */
BCN_API int bcn_mixing_create(const bcn_mixing_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces mixing.reset / reset_fields (mixing.py:73-111) */
BCN_API int bcn_mixing_reset(bcn_env_t h, void* obs_dev, void* stream);
/* replaces mixing.step (mixing.py:114-135) incl. solve/get_control/get_obs/get_rwd (:138-264).
 * actions_dev int32[B] in {0,1,2,3} (anything else = walls at rest), NULL = repeat last. */
BCN_API int bcn_mixing_step(bcn_env_t h, const int32_t* actions_dev, void* obs_dev, void* rwd_dev,
                    uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev, int32_t* sweeps_dev,
                    void* stream);

/* ---- burgers: burgers/burgers.py ----------------------------------------------------- */
typedef struct {
  int32_t nx;                     /* 500 in the reference (burgers.py:26) */
  int32_t ndt_act, n_act;         /* 62, 200 */
  int32_t ctrl_pos, n_obs_pts;    /* 250, 5 */
  double dx, dt, amp, u_target;
} bcn_burgers_cfg;

/* replaces burgers.__init__ (burgers.py:21-65) */
BCN_API int bcn_burgers_create(const bcn_burgers_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces burgers.reset (burgers.py:68-94) */
BCN_API int bcn_burgers_reset(bcn_env_t h, void* obs_dev, void* stream);
/* replaces burgers.step (burgers.py:97-166).  actions_dev[B] (NULL = repeat last);
 * noise_dev[B]: the uniform(-sigma,sigma) inlet draw of this step (burgers.py:127), explicit. */
BCN_API int bcn_burgers_step(bcn_env_t h, const void* actions_dev, const void* noise_dev, void* obs_dev,
                     void* rwd_dev, uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev,
                     void* stream);

/* ---- shkadov: shkadov/shkadov.py ----------------------------------------------------- */
typedef struct {
  int32_t nx;                     /* int(5 (L0 + jet_space (n_jets+2))) */
  int32_t ndt_act, n_act;         /* 50, 400 */
  int32_t n_jets, jet_pos, jet_hw, jet_space; /* lattice units (shkadov.py:64-68) */
  int32_t l_obs, l_rwd, n_obs, obs_stride, n_interp; /* 50, 50, 10, 5, 20 */
  double dx, dt, delta, jet_amp, eps;
  double h_blow;                  /* 5 h_max = 25 (shkadov.py:176) */
  double blowup_rwd;              /* -1 */
} bcn_shkadov_cfg;

/* replaces shkadov.__init__ (shkadov.py:20-110) */
BCN_API int bcn_shkadov_create(const bcn_shkadov_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces shkadov.reset with rand_init = False (shkadov.py:113-146; bcn_shkadov_reset_random below is the reference's default,
 * rand_init = True): init_fields_dev [2][nx] (h_init, q_init) shared by all replicas, NULL = flat film h=q=1 (reset_fields only). */
BCN_API int bcn_shkadov_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream);
/* replaces shkadov.reset with rand_init = True (shkadov.py:113-146 with :119-123), in ONE launch and without host work: every replica
 * that bcn_set_mask leaves on is reset as by bcn_shkadov_reset and then takes n[b] action steps of the zero action under the
 * device's inlet noise (bcn_set_noise; sigma = 0: no noise) -- what n[b] calls of bcn_shkadov_step(actions NULL, noise NULL) compute
 * for it, bit for bit, with the fields kept in registers in between -- after which its episode counter is 0 again.
 *   n[b]: n_steps_dev[b] clamped to [0, rand_steps], or, with n_steps_dev NULL, uniform on {0 .. rand_steps} from the env's Philox
 *         stream: key = the noise seed, counter = (replica_offset + b, the replica's draw counter, 0, 1) -- the last word is 0 in every
 *         noise draw -- mapped by the high word of word0 * (rand_steps + 1).  0 <= rand_steps <= 65535 (the reference: 400).
 *   The count costs one tick of the replica's draw counter (a snapshot segment), with n_steps_dev and with sigma = 0 as well, and
 *   every warm-up step with noise one more, as a step does: two resets in a row draw different counts, a run restored from a
 *   snapshot redraws the same ones, and a sharded batch draws what the single one draws for the same global replica.
 *   Written: the fields, stp = 0, the stored actions (0), the observation rows obs_dev [B][n_obs] and n_out_dev [B] (NULL: not
 *   wanted) of the replicas that were reset.  There are no rwd / done / trunc / status arguments: a reset leaves those rows alone.
 *   A film that blows up during the warm-up is not flagged here (the reference prints and carries on); the first step reports it.
 * Per-replica delta (bcn_set_params) is honoured.  bcn_kernel_name / bcn_kernel_shape afterwards: "shkadov_warm_k" and the (K, NT)
 * the next bcn_shkadov_step will run with. */
BCN_API int bcn_shkadov_reset_random(bcn_env_t h, const void* init_fields_dev, const int32_t* n_steps_dev /* [B] or NULL: drawn */,
                             int rand_steps, int32_t* n_out_dev /* [B] or NULL */, void* obs_dev, void* stream);
/* replaces shkadov.step (shkadov.py:161-264).  actions_dev[B][n_jets] (NULL = repeat last);
 * noise_dev[B][ndt_act]: inlet draws, one per timestep (shkadov.py:204). */
BCN_API int bcn_shkadov_step(bcn_env_t h, const void* actions_dev, const void* noise_dev, void* obs_dev,
                     void* rwd_dev, uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev,
                     void* stream);

/* ---- sloshing: sloshing/sloshing.py -------------------------------------------------- */
typedef struct {
  int32_t nx;                     /* int(80 L) */
  int32_t ndt_act, n_act, n_interp; /* 50, 200, 10 */
  double dx, dt, g, amp, alpha;
} bcn_sloshing_cfg;

/* replaces sloshing.__init__ (sloshing.py:20-89) */
BCN_API int bcn_sloshing_create(const bcn_sloshing_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces sloshing.reset (sloshing.py:92-124): init_fields_dev [2][nx+2] (h_init, q_init) or NULL */
BCN_API int bcn_sloshing_reset(bcn_env_t h, const void* init_fields_dev, void* obs_dev, void* stream);
/* replaces sloshing.step (sloshing.py:141-244).  actions_dev[B] (NULL = repeat last) */
BCN_API int bcn_sloshing_step(bcn_env_t h, const void* actions_dev, void* obs_dev, void* rwd_dev,
                      uint8_t* done_dev, uint8_t* trunc_dev, int32_t* status_dev, void* stream);

/* ---- lorenz: lorenz/lorenz.py ------------------------------------------------------- */
/* The two ODE envs run one lane per replica with the whole state in registers (beacon_amd/csrc/ode_env.h).  Precision: BCN_F64
 * follows the reference's episodes bit for bit (lorenz) / to the last bits of the device cos / sin (vortex); BCN_F32 one action
 * step from the same state: tests/test_gpu_ode.py. */
typedef struct {
  int32_t ndt_act, n_act;         /* int(dt_act / dt) = 1, int(t_max / dt_act) = 500 */
  double dt;                      /* 0.05 */
  double sigma, rho, beta;        /* 10, 28, 8/3 (lorenz.py:22-25) */
} bcn_lorenz_cfg;

/* replaces lorenz.__init__ (lorenz.py:22-57) */
BCN_API int bcn_lorenz_create(const bcn_lorenz_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces lorenz.reset / reset_fields (lorenz.py:60-95): x = 10, fx = 0, t = 0, u = 1 (no force).  obs_dev[B][6] may be NULL. */
BCN_API int bcn_lorenz_reset(bcn_env_t h, void* obs_dev, void* stream);
/* replaces lorenz.step (lorenz.py:98-117) incl. solve/get_obs/get_rwd (:120-172).  actions_dev int32[B] in {0,1,2}
 * (force -1, 0, 1; anything else = no force), NULL = repeat last.  obs_dev[B][6] = (x, f(x) of the last RK stage). */
BCN_API int bcn_lorenz_step(bcn_env_t h, const int32_t* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev,
                    uint8_t* trunc_dev, int32_t* status_dev, void* stream);

/* ---- vortex: vortex/vortex.py ------------------------------------------------------- */
typedef struct {
  int32_t ndt_act, n_act;         /* int(dt_act / dt) = 5, int(t_max / dt_act) = 800 */
  double dt;                      /* 0.1 */
  double lmbda_re, lmbda_cx;      /* 9.153, 3.239 (vortex.py:26-48) */
  double mu_re, mu_cx;            /* 308.9, -1025 */
  double alpha_re, alpha_cx;      /* 0.03492, 0.01472 */
  double beta, re, re_crit;       /* 1, 50, 46.6 */
  double omega_s, omega_f;        /* 1.1, 0.74 */
  double gamma, mass, weight;     /* 0.023, 10, 50 */
  double mod_min, mod_max;        /* 0, 0.3 */
  double phase_min, phase_max;    /* -pi, pi */
} bcn_vortex_cfg;

/* replaces vortex.__init__ (vortex.py:21-79) */
BCN_API int bcn_vortex_create(const bcn_vortex_cfg* cfg, int batch, int dtype, int device, bcn_env_t* out);
/* replaces vortex.reset / reset_fields (vortex.py:82-125): the fixed start point, u = (0, 0), kmod = kphase = 0.  obs_dev[B][8] or NULL. */
BCN_API int bcn_vortex_reset(bcn_env_t h, void* obs_dev, void* stream);
/* replaces vortex.step (vortex.py:127-146) incl. solve/get_obs/get_rwd (:149-208).  actions_dev[B][2] = (modulus, phase) in
 * [-1, 1], NULL = repeat last.  obs_dev[B][8] = (x, f(x) of the last RK stage). */
BCN_API int bcn_vortex_step(bcn_env_t h, const void* actions_dev, void* obs_dev, void* rwd_dev, uint8_t* done_dev,
                    uint8_t* trunc_dev, int32_t* status_dev, void* stream);

/* ---- common -------------------------------------------------------------------------- */
BCN_API int bcn_env_kind(bcn_env_t h);
BCN_API int bcn_batch(bcn_env_t h);
BCN_API int bcn_dtype(bcn_env_t h);
BCN_API int bcn_n_obs(bcn_env_t h);       /* observation length per replica */
BCN_API int bcn_n_act(bcn_env_t h);       /* action length per replica */
BCN_API int bcn_ndt_act(bcn_env_t h);     /* timesteps per action step: rows of sweeps_dev [B][ndt_act] and of shkadov's noise_dev */
BCN_API int bcn_device(bcn_env_t h);      /* HIP device index the handle was created on (every *_dev pointer must live there) */
/* Solver state of all replicas, the equivalent of the env's field attributes (and of
 * dump()/load(), rayleigh.py:344-362): elements per replica, then copy out / in.  Layout per
 * replica: rayleigh/mixing [4][ny+2][nx+2] = u,v,p,S; burgers [3][nx] = u,up,upp;
 * shkadov [4][nx] = h,q,rhsh,rhsq; sloshing [4][nx+2] = h,q,rhsh,rhsq;
 * lorenz [8] = x0,x1,x2, fx0,fx1,fx2, t, u (the action index, as a value of the handle's dtype);
 * vortex [14] = ar,ai,yr,yi, fx0..fx3, t, y, kmod, kphase, u0,u1 (t accumulated as t += dt, y of the last get_rwd).
 * `buf` may be a host or a device pointer (is_device); host copies synchronise the stream. */
BCN_API size_t bcn_state_elems(bcn_env_t h);
BCN_API int bcn_get_state(bcn_env_t h, void* buf, int is_device, void* stream);
BCN_API int bcn_set_state(bcn_env_t h, const void* buf, int is_device, void* stream);
/* Replica mask for the calls that follow: *_reset and *_step skip every replica b with mask_dev[b] == 0
 * (state, stp and that replica's rows of the output buffers stay untouched); NULL = all replicas.  The
 * pointer is read at launch time of each later call, so it must stay valid.  Used for per-replica
 * resets at episode end (the reference's trainer calls reset() on one env) and for the per-env random
 * number of uncontrolled warm-up steps of shkadov.reset (shkadov.py:119-123). */
BCN_API int bcn_set_mask(bcn_env_t h, const uint8_t* mask_dev);
/* episode counter `stp` of every replica (rayleigh.py:126,155): int32[B] */
BCN_API int bcn_get_stp(bcn_env_t h, int32_t* buf_host, void* stream);
BCN_API int bcn_set_stp(bcn_env_t h, const int32_t* buf_host, void* stream);
/* Which kernel variant *_step uses: 0 = generic (any grid, fields in HBM/L2, Jacobi in LDS),
 * 1 = register-resident CDNA4 path where the grid has one (default there; falls back to 0 otherwise).  Built into the
 * library: rayleigh 128x64 f32/f64, 50x50 f32/f64, 100x50 / 150x50 / 200x50 f32 (one row per lane: ns2d_fast_impl.h);
 * rayleigh and mixing 100x100 f32/f64 (two rows per lane: ns2d_fast2_impl.h).  Every other grid gets its kernel through
 * bcn_set_fast_plugin (beacon_amd/jit.py compiles it on demand): one row per lane for rayleigh with ny <= 64, two rows per
 * lane for 64 < ny <= 128, and for everything else up to ny = 256 (tall grids, grids wider than the strips, mixing below
 * ny = 64) the hybrid of ns2d_fast4_impl.h (Poisson solve in registers, fields in HBM/L2).  Beyond that: variant 0 only.
 * Results of the two variants agree to rounding (float64: 1e-9).  Returns the variant actually selected; lorenz and vortex have
 * one kernel and no variants: BCN_ERR_ARG (as for bcn_set_noise, bcn_set_fast_plugin, bcn_set_sched, bcn_set_slow_mode_bound). */
BCN_API int bcn_set_variant(bcn_env_t h, int variant);
/* Measurement aid (no reference counterpart), uint64[B][4] on the host, per replica, of the last *_step (all chunks):
 *   [0] shader-clock cycles inside the Jacobi loop (rayleigh.py:419-454 / mixing.py:428-463), [1] in the whole replica,
 *   [2] solves whose LANDING -- the first evaluation of the residual behind sweeps the extrapolating plan (conv_plan 2 / 3) had
 *       skipped -- did not verify the skip: under plan 3 the residual was not above BCN_CONV_GUARD * tol there (so a skipped
 *       sweep may have passed the test); under plan 2 the landing itself passed,
 *   [3] timesteps (rayleigh) / solves (two-rows-per-lane and tall-grid kernels) that were repeated: a speculative opening whose
 *       landing did not verify it, or conv_plan 3 repeating an unverified solve under the proven plan.
 * Zeros for kernels that do not count (generic 2D kernel, 1D envs).
 * Under conv_plan 3 every stop sweep is the reference's BY PROOF (see "conv_plan"): zeros in [2] mean that no solve needed the
 * repeat, not that something went unnoticed.
 * buf_host must hold batch * BCN_COUNTER_WORDS words; bcn_get_counters_n writes `words_per_replica` words per replica instead
 * (the first min(words, BCN_COUNTER_WORDS) counters, zeros beyond) for callers built against another header. */
BCN_API int bcn_get_counters(bcn_env_t h, uint64_t* buf_host, void* stream);
BCN_API int bcn_get_counters_n(bcn_env_t h, uint64_t* buf_host, int words_per_replica, void* stream);
BCN_API int bcn_api_version(void);
/* Register-resident kernel for a grid that is not built into the library (up to ny = 256; above ny = 128 and for grids wider
 * than the all-in-registers kernels' strips only the Poisson solve is register-resident: csrc/ns2d_fast4_impl.h).  The reference takes any L, H
 * (rayleigh.py:20-27: nx = 50 L, ny = 50 H; mixing.py:20-28: 100 L, 100 H); csrc/jit/ns2d_jit.hip is compiled for ONE
 * grid into its own shared object (beacon_amd/jit.py does so on demand and caches it) whose
 *   int bcn_jit_launch(const void* step_args, int batch, void* stream)
 * is passed here together with bcn_jit_scratch_elems().  Selects variant 1; launch_fn = NULL restores the built-in
 * choice.  The plugin must outlive the handle. */
BCN_API int bcn_set_fast_plugin(bcn_env_t h, void* launch_fn, size_t scratch_elems);
/* The same plugin's kernels that read the per-replica parameter table (bcn_set_params; option "params_kernel").  A plugin compiled
 * with -DBCN_JIT_PRM=1 is a shared object of its own that exports, next to the symbols above,
 *   int bcn_jit_launch_prm(const void* step_args, int batch, void* stream, const void* params_table_dev)
 * Passed here AFTER bcn_set_fast_plugin (which clears it); launch_fn = NULL clears it.  Without it a plugin handle that has a
 * table steps through the generic kernel whatever "params_kernel" says.  BCN_ERR_ARG for a handle without a plugin and for envs
 * that take none. */
BCN_API int bcn_set_fast_plugin_params(bcn_env_t h, void* launch_fn);
/* Inlet noise on the device (burgers, shkadov).  The reference draws np.random.uniform(-sigma, sigma, 1) from numpy's global
 * stream -- once per action step (burgers.py:127), once per timestep (shkadov.py:204) -- and the *_step entry points take those
 * draws as noise_dev, so that a caller can reproduce the reference's stream.  A trainer that only needs noise of that law leaves
 * noise_dev NULL after this call: the step kernel then draws uniform(-sigma, sigma) itself (Philox4x32-10 keyed by `seed`, counter =
 * (replica_offset + replica index, the replica's own count of such steps, timestep, 0)) -- no extra launch, no host work, fresh values
 * when a captured graph replays.  sigma = 0 (the default) restores "NULL = no noise".  replica_offset: global index of this handle's
 * replica 0 (sharded batches).  Resets the replicas' draw counters.  BCN_ERR_ARG for envs without inlet noise.
 *   The value: key = (low, high 32-bit word of `seed`); with w0, w1 the first two output words, r = (w0 >> 8) 2^-24 (BCN_F32) or
 *   ((w0 << 21) ^ (w1 >> 11)) 2^-53 (BCN_F64), and the draw is (2 r - 1) sigma in the handle's precision.
 *   The draw counter: a step with noise_dev NULL and sigma > 0 advances the counter of every replica it steps by one; a replica
 *   that bcn_set_mask leaves out keeps its counter, and so does every step with an explicit noise_dev.  bcn_burgers_reset and
 *   bcn_shkadov_reset leave the counters alone, masked or not -- only this call sets them back to 0 -- so the episode after a reset
 *   goes on in the stream where the last one stopped (bcn_shkadov_reset_random ticks them as described there).
 *   tests/noise_ref.py restates the stream on the host; tests/test_gpu_noise.py holds the kernels to it bit for bit. */
BCN_API int bcn_set_noise(bcn_env_t h, double sigma, uint64_t seed, int64_t replica_offset);
/* Solver options of the 2D envs (no reference counterpart), by name:
 *   "conv_plan"   which Jacobi sweeps evaluate the residual err = sum((phi - phin)^2) of rayleigh.py:448-449 / mixing.py:457-458
 *                 in the register-resident kernels.  Every plan returns the reference's stop sweep -- the FIRST sweep with
 *                 err <= tol -- and differs only in how it knows that the sweeps it does not evaluate could not pass:
 *                 0 = every sweep evaluated, as the reference does;
 *                 1 = sweeps skipped while a PROVEN lower bound of err stays above tol: the increments obey d' = J d with J
 *                     symmetric, so the plain norm |d|^2 <= err is log-convex in the sweep count and its measured decay bounds
 *                     every later one (the default of BCN_F64 until round 5; what plan 3 repeats an unverified solve under);
 *                 3 = the decay of err itself extrapolated, landing where it is still expected above 1.035 tol, and every
 *                     landing -- the first evaluation behind skipped sweeps, the speculative opening's included -- VERIFIED:
 *                     err can grow from a sweep to a later one by at most max_m || W^1/2 J^m W^-1/2 ||^2 = 1.030 (W = I + G:
 *                     the ghost copies the reference's sum counts; scripts/weighted_norm_bound.py, every grid of the
 *                     reference's constructor space), so had a skipped sweep passed, the landing would find err <= 1.030 tol;
 *                     a landing above BCN_CONV_GUARD = 1.035 tol therefore proves that none did, and a landing below it is
 *                     counted ([2]) and the solve repeated under plan 1 (the default of both precisions; grids with a side below 48
 *                     cells, where the bound is larger, take plans 0 / 1 only).  With the grid's slow-mode constants in force
 *                     (bcn_set_slow_mode_bound below; built in for the default grids) the landing threshold drops from 1.035 tol
 *                     to a fraction of a percent above tol late in a solve -- still a proof, and far fewer evaluations.
 *                     What "proof" covers: the recurrence d' = J d in EXACT arithmetic, which BCN_F64 follows to 1e-16.  BCN_F32
 *                     adds rounding of ~eps |phi| per cell and sweep to the increments (0.05 - 0.3 % of tol = 1e-8 on 8192 cells),
 *                     the size of the slow-mode threshold's distance from tol; the kernels put a 0.1 % margin on that threshold
 *                     and the float32 default is VERIFIED EMPIRICALLY on top (option "verify_conv": every sweep evaluated next to
 *                     the plan over whole episodes of the bench workload, no BCN_ST_PLAN: tests/test_gpu_parity.py), not proven;
 *                     a caller who wants the float32 proof unconditional clears the slow-mode constants
 *                     (bcn_set_slow_mode_bound(h, 0, ...)): BCN_CONV_GUARD's 3.5 % dwarf the rounding;
 *                 2 = plan 3's extrapolation WITHOUT the verification (round 2's rule: it notices a landing only when the
 *                     landing itself passes, and then only counts it): kept for measurements, never a default
 *   "plan_overshoot" 0..64, TEST HOOK: lengthens every skip of plans 2 / 3 by that many sweeps, so that landings fall behind
 *                 the stop sweep (tests/test_gpu_parity.py: the adversarial right-hand side)
 *   "verify_conv" 1 = evaluate every sweep anyway and raise BCN_ST_PLAN if a sweep the plan skips passes the test
 *   "spec_start"  0..17: open a solve with unevaluated double sweeps up to spec_start/8 of the previous timestep's sweep
 *                 count (1..16), or -- 17, the default -- up to 15/16 of it minus 1.25 times the stretch in front of the stop in
 *                 which the residual is already below the landing guard (log2(1.035) / the previous solve's decay per sweep);
 *                 the landing behind them is verified like any other (plan 3: above 1.035 tol, else the solve is
 *                 repeated without the guess).  BCN_F32 rayleigh only; ignored by BCN_F64 handles, off for mixing
 *   "transport_iter" 0..64 (mixing, BCN_F32, 64 < ny <= 128): the ordered part of the scalar transport -- mixing.py:478-497 sweeps the
 *                 array in place, so a cell reads the NEW values of its west and south neighbours: S' = A + aW S'(i-1,j) + aS S'(i,j-1),
 *                 a lower-triangular system -- as the Neumann series sum_m L^m A, one parallel pass of every wave per term, M terms with
 *                 rho^(M+1) <= 2^-27, rho = max(|aW| + |aS|) measured in every timestep (0.2 at the reference's u_max: M = 12; 7e-9 of
 *                 a scalar in [0, 1], below the rounding of the sweep itself).  The option is the largest M allowed (default 24); where
 *                 the measured rho needs more, and with 0, the ordered sweep of the reference runs (one wave, nx + ny/2 dependent steps).
 *                 BCN_F64 always runs the ordered sweep
 *   "sched_tail"  short chunks that end a step of the ticket scheduler (0 = default 6; see bcn_set_sched)
 *   "generic_threads" 256 / 1024: workgroup size of the generic 2D kernel (0 = chosen by grid size)
 *   "params_kernel" 0 / 1: which kernel steps a handle that has a per-replica parameter table (bcn_set_params).  0 (default): the
 *                 generic kernel, whatever the variant.  1: with variant 1, the register-resident kernel of the grid in its
 *                 table-reading form (built in for every built-in grid; a plugin: bcn_set_fast_plugin_params) -- a replica computes,
 *                 bit for bit, what a handle created with its parameters computes on the plain register-resident kernel.  Where
 *                 there is no such kernel (a plugin without the second launcher, a batch beyond the hybrid's 32-bit addressing) and
 *                 with variant 0 the generic kernel takes the step; bcn_kernel_name says which one did.  Without a table: no effect
 *   "cell_runs"   0 / 1 (2D envs), TEST HOOK: which unit's one-row-per-lane kernels step a BCN_F32 rayleigh handle on a built-in grid
 *                 under variant 1.  1 (default): the kernels whose Jacobi cells are stated in runs (csrc/ns2d_fast_runs.hip), where
 *                 that unit has the grid; 0: the cell-by-cell kernels of csrc/ns2d_fast.hip, which compute the same bits
 *                 (tests/test_gpu_jacobi_cells.py holds the two to each other).  No effect on BCN_F64 handles, on handles with a kernel
 *                 plugin, on grids the runs unit does not have (100x50) and on steps with a parameter table.  Both units' kernels carry
 *                 the same names, so bcn_kernel_name cannot tell them apart; the library's internal query
 *                 int bcn_cell_runs_active(bcn_env_t) -- exported like bcn_jit_builtin, no part of this ABI -- answers 1 where the
 *                 next variant-1 step of the handle goes through the runs unit, from the predicate the dispatch itself uses
 *   "cells_per_thread" (1D envs) 1, 2, 4, 8 cells per thread (0 = chosen from grid and batch); "one_wave" (1D envs) 0 / 1:
 *                 grids up to 512 cells as one wave per replica with DPP halos (default 1)
 *   "obs_stage"   (lorenz, vortex) 1 = the observation rows [B][n_obs] go through LDS so that every store of a workgroup writes
 *                 contiguous bytes (default of BCN_F64), 0 = each lane stores its own row (default of BCN_F32)
 * No environment variable changes any of these (round 5: the library reads none).
 * Returns BCN_ERR_ARG for unknown names. */
BCN_API int bcn_set_option(bcn_env_t h, const char* name, int value);
/* Slow-mode landing guard of conv_plan 3 (no reference counterpart; beacon_amd/stoprule.py has the derivation).  Within the span of
 * the Jacobi matrix's eigenvectors with |lambda| >= cutoff[k], the reference norm can grow from a sweep to any later one by at most
 * bound[k] (>= 1: 1.0002 / 1.0057 for cutoffs 0.9 / 0.8 on the 128x64 grid, against 1.030 over all modes), and what lies outside that
 * span has decayed to cutoff^(j-1) |d_1| by sweep j.  With the constants set, a landing behind the last evaluated sweep i is verified
 * when it finds err > min(BCN_CONV_GUARD, min_k bound[k] (1 + 2 sqrt(3 |d_1|^2 / tol) cutoff[k]^i)^2 (1 + 0.001)) tol -- a fraction of
 * a percent above tol late in a solve instead of 3.5 %, i.e. a dozen sweeps fewer that must be evaluated one by one.  The constants
 * are properties of (nx, ny, boundary kind, cx): built in for the reference's default grids (rayleigh 50x50, mixing 100x100) and for
 * 128x64; for any other grid the host computes them (beacon_amd/stoprule.py, cached) and passes n <= 2 pairs here; n = 0 clears them
 * (the guard is then BCN_CONV_GUARD alone).  Used by the one-row and two-rows-per-lane kernels (ny <= 128); the hybrid kernel
 * (ny > 128) keeps BCN_CONV_GUARD.  bcn_get_slow_mode_bound returns the number of pairs in force and writes them (arrays of 2). */
BCN_API int bcn_set_slow_mode_bound(bcn_env_t h, int n, const double* cutoff, const double* bound);
BCN_API int bcn_get_slow_mode_bound(bcn_env_t h, double* cutoff, double* bound);
/* Work scheduling of the register-resident 2D kernels when replicas outnumber the CUs (no reference
 * counterpart: the reference steps one env per process, rayleigh.py:138-157).  mode: -1 = default
 * (2), 0 = one workgroup per replica in one launch, 1 = two launches with the
 * replicas re-ordered longest-first, 2 = persistent workgroups drawing (chunk of q timesteps, replica)
 * tickets; grid = persistent workgroups (0 = one per CU); q = timesteps per chunk (0 = kernel default);
 * lpt_min_batch = smallest batch that mode 1 splits (0 = CUs + 1).  Results do not depend on the mode.  BCN_ERR_ARG for lorenz
 * and vortex (one lane per replica, nothing to schedule). */
BCN_API int bcn_set_sched(bcn_env_t h, int mode, int grid, int q, int lpt_min_batch);
/* Snapshots: everything a handle needs to continue an episode bit for bit, for all its replicas, as ONE device byte buffer
 * (no reference counterpart beyond dump()/load() of the fields, rayleigh.py:344-362: SURVEY.md 5 lists resume as missing there).
 * bcn_get_state carries the solver fields only; a snapshot adds what the next *_step also reads -- the observation history, the
 * stored action that actions_dev = NULL repeats and the 1D envs' action ramp starts from, the episode counter, the draw counter
 * of the device noise -- and the packed outputs of the last call, so that a restored env also shows the observations a policy
 * needs for its next action.
 * Layout of a snapshot of n replicas: named segments in the order below, every segment start a multiple of 16 bytes; a segment
 * is [planes][n][row_elems] elements (no padding between planes or rows), `real` = the handle's dtype:
 *   rayleigh   fields real [4][n][(ny+2)(nx+2)] = u,v,p,S (per replica x fastest: bcn_get_state's [n][4][..] with the first two
 *              axes exchanged), obs_hist real [n][n_obs], a_last real [n][n_sgts] (the conditioned action), stp int32 [n]
 *   mixing     fields, obs_hist as rayleigh, ia_last int32 [n], stp int32 [n]
 *   burgers    fields real [3][n][nx] = u,up,upp, a_last real [n][1], a_prev real [n][1], stp int32 [n], nctr uint32 [n]
 *   shkadov    fields real [4][n][nx] = h,q,rhsh,rhsq, a_last / a_prev real [n][n_jets], stp, nctr
 *   sloshing   fields real [4][n][nx+2], a_last / a_prev real [n][1], stp, nctr
 *   lorenz     fields real [7][n][1] = x0,x1,x2, fx0,fx1,fx2, t, iu int32 [n] (the action index), stp
 *   vortex     fields real [14][n][1] (the columns of bcn_get_state), stp
 *   all        obs real [n][n_obs], rwd real [n], status int32 [n], done uint8 [n], trunc uint8 [n]
 * bcn_snapshot_layout writes these as (name, byte offset, element type, planes, row_elems) and returns their number (at most 16;
 * only the first max_segs are written); bcn_snapshot_bytes_n is the size (a multiple of 16) and bcn_snapshot_bytes that of the
 * handle's own batch.  What is NOT in it, because every *_step rewrites it before reading it: us / vs and the work arrays of the 2D
 * envs, their field scratch, sweep counts, scheduler block and cycle counters.  Kernel arguments are not state either: noise sigma,
 * seed and replica offset (bcn_set_noise), options, the kernel variant, the replica mask.
 * bcn_snapshot_signature: a hash of env kind, dtype, every value of the cfg struct the handle was CREATED from and the segment
 * shapes -- two handles exchange snapshots exactly when it is equal; the batch is not part of it.  What is set on a handle after
 * its creation (options, variant, noise, slow-mode bounds) is not hashed: none of it changes what the bytes mean.
 * out_buf_dev: the caller's packed output buffer of the handle's batch B, [obs | rwd | status | done | trunc] with every part
 * starting at a multiple of 16 bytes (obs at 0; B n_obs reals, B reals, B int32, B uint8, B uint8); NULL leaves the five output
 * segments out of the copy.  snap_dev and out_buf_dev must be 16-byte aligned.
 * bcn_snapshot_save: handle -> snap_dev (bcn_snapshot_bytes(h) bytes), every replica, the replica mask ignored.
 * bcn_snapshot_load: snap_dev holds n_src replicas; replica b of the handle takes replica src_dev[b] (int32[B] on the device; NULL =
 * b, which needs n_src == B) where mask_dev[b] != 0 (uint8[B], NULL = all; the mask of bcn_set_mask plays no part).  A replica whose
 * index lies outside [0, n_src) is left untouched like a masked one: no address is formed from it.  snap_dev must not alias the
 * handle's arrays or out_buf_dev (a gather inside one handle is a save followed by a load).
 * Both are ONE kernel launch on `stream` -- no host synchronisation, no host read, no allocation -- so they can be captured into a
 * graph next to *_step. */
enum { BCN_SNAP_REAL = 0, BCN_SNAP_I32 = 1, BCN_SNAP_U32 = 2, BCN_SNAP_U8 = 3 };
typedef struct {
  char name[16];
  uint64_t offset;                /* bytes from the start of the snapshot, a multiple of 16 */
  int32_t elem;                   /* BCN_SNAP_* */
  int32_t planes;
  int64_t row_elems;
} bcn_snapshot_seg;
BCN_API size_t bcn_snapshot_bytes(bcn_env_t h);
BCN_API size_t bcn_snapshot_bytes_n(bcn_env_t h, int n);
BCN_API int bcn_snapshot_layout(bcn_env_t h, int n, bcn_snapshot_seg* segs, int max_segs);
BCN_API uint64_t bcn_snapshot_signature(bcn_env_t h);
BCN_API int bcn_snapshot_save(bcn_env_t h, void* snap_dev, const void* out_buf_dev, void* stream);
BCN_API int bcn_snapshot_load(bcn_env_t h, const void* snap_dev, int n_src, const int32_t* src_dev, const uint8_t* mask_dev,
                              void* out_buf_dev, void* stream);
/* The packed output buffer (out_buf_dev above) of `batch` replicas with n_obs observations of esz bytes (4 or 8) each: byte offset
 * of every part and the size of the whole.  The one definition of that layout: the library, the torch extension and -- through a
 * test -- the Python side's allocation all follow it.  Header-only, not an exported symbol. */
typedef struct { size_t obs, rwd, status, done, trunc, bytes; } bcn_out_layout_t;
static inline bcn_out_layout_t bcn_out_layout(size_t batch, size_t n_obs, size_t esz) {
  const size_t len[5] = {batch * n_obs * esz, batch * esz, batch * 4, batch, batch};
  size_t off[6] = {0, 0, 0, 0, 0, 0};
  bcn_out_layout_t o;
  for (int k = 0; k < 5; k++) off[k + 1] = (off[k] + len[k] + 15) / 16 * 16;
  o.obs = off[0]; o.rwd = off[1]; o.status = off[2]; o.done = off[3]; o.trunc = off[4]; o.bytes = off[5];
  return o;
}
/* Per-replica physical parameters.  Every handle is created from ONE cfg; these calls give each replica of the batch its own values
 * of the reference's constructor arguments (everything else in a cfg -- grids, counts, segment and jet layout, dt, tolerances -- is
 * structural and stays per handle).  Parameters, in the order of bcn_param_name and of the value rows:
 *   lorenz    sigma, rho, beta        vortex   re, weight         burgers  u_target, amp      shkadov  delta
 *   sloshing  amp, alpha, g           rayleigh ra                 mixing   re, pe (the lid speed follows: u_max = re nu / L)
 * bcn_set_params: values_host is double [n_params][B] on the host (row k = parameter k of every replica); NULL clears them (every
 * replica has the cfg's values again).  Checked before the handle or the device is touched: every value finite, and ra, re, pe,
 * delta, g > 0 (divisors, arguments of roots); otherwise BCN_ERR_ARG, and bcn_last_error names the parameter and the replica.  The
 * constants the kernels read (rayleigh sqrt(pr / ra), 1 / sqrt(pr ra); mixing 1 / re, 1 / pe, u_max; shkadov 1 / (5 delta); vortex
 * 1 / re_crit - 1 / re) are computed on the host in double by the expressions *_create uses and narrowed once to the handle's dtype:
 * a replica whose parameters equal another handle's cfg computes what that handle computes, bit for bit.
 * The device table is allocated by the first call and never moves; later calls overwrite it in place on `stream` (and wait for the
 * copy: a set-up call like bcn_set_stp).  So a graph captured AFTER the first call reads whatever table is in force when it is
 * replayed -- also after a later NULL, which only stops new launches from reading it -- and a graph captured BEFORE it keeps the
 * uniform cfg.  Parameters are configuration, like the noise settings: they take effect at the next *_reset / *_step (burgers'
 * reset fills a replica with its own u_target), alter no state, are not part of a snapshot or of bcn_snapshot_signature, and
 * bcn_snapshot_load moves state between replicas while each replica keeps its physics.
 * rayleigh / mixing: the table is an argument of the generic kernel only; while it is set, *_step runs ns2d_generic_step whatever
 * bcn_set_variant selected (bcn_kernel_name says so), and NULL restores the previous dispatch.
 * bcn_get_params: the values in force, double [n_params][B]; the cfg's values broadcast when none are set.
 * bcn_derive_params_host (no device, no handle; for tests): the derived constants, in double, of one parameter set of env `kind`;
 * aux = what the expressions need of the cfg besides (rayleigh: pr; mixing: the cfg's re, u_max; vortex: re_crit; else unused but
 * not NULL).  Returns their number, -1 on a bad argument. */
BCN_API int bcn_n_params(bcn_env_t h);
BCN_API const char* bcn_param_name(bcn_env_t h, int i);
BCN_API int bcn_set_params(bcn_env_t h, const double* values_host, void* stream);
BCN_API int bcn_get_params(bcn_env_t h, double* values_host);
BCN_API int bcn_derive_params_host(int kind, const double* params, const double* aux, double* derived);
/* Episode statistics and the rescue of terminal observations: the bookkeeping a trainer does between a *_step and the masked
 * *_reset of the replicas whose episode ended, as ONE kernel launch on `stream` (no host synchronisation, no host read, no
 * allocation: it can be captured into a graph between the two).  The handle is used for batch B, observation length and dtype
 * only; the episode buffer belongs to the caller (bcn_episode_bytes(h) bytes -- 0 and bcn_last_error for a NULL handle --, 16-byte
 * aligned, zeroed before its first use).
 * Its segments, in this order, every start a multiple of 16 bytes (bcn_episode_layout writes them as bcn_snapshot_seg with
 * planes = 1 and returns their number, 9; only the first max_segs are written; 0 and bcn_last_error on a bad argument):
 *   ret real [B], len int32 [B]             return and length of the episode in progress
 *   last_ret real [B], last_len int32 [B]   those of the replica's last finished episode
 *   count int32 [B]                         finished episodes
 *   sum_ret float64 [B], sum_len int64 [B]  sums of the returns and lengths of the finished episodes
 *   finished uint8 [B]                      1 where the tracked step ended an episode -- the mask of the reset that follows
 *   final_obs real [B][n_obs]               the terminal observation, written for finished replicas only
 * bcn_episode_track: out_buf_dev is the packed output buffer of the step (bcn_snapshot_save: [obs | rwd | status | done | trunc]).
 * For every replica b with mask_dev[b] != 0 (uint8[B]; NULL = all; the mask of bcn_set_mask plays no part), fin = done[b] | trunc[b]:
 *   ret[b] += rwd[b] (one add in the handle's dtype); len[b] += 1;
 *   if fin: last_ret[b] = ret[b]; last_len[b] = len[b]; count[b] += 1; sum_ret[b] += (double)ret[b]; sum_len[b] += len[b];
 *           ret[b] = 0; len[b] = 0; final_obs[b][:] = obs[b][:];
 *   finished[b] = fin.
 * A replica with mask_dev[b] == 0 keeps every entry and gets finished[b] = 0 (its stale done byte must not start a reset).
 * Batch totals are the sums of the count / sum_ret / sum_len columns, taken by the reader. */
enum { BCN_SNAP_F64 = 4, BCN_SNAP_I64 = 5 };   /* element types of bcn_episode_layout besides BCN_SNAP_* above */
BCN_API size_t bcn_episode_bytes(bcn_env_t h);
BCN_API int bcn_episode_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs);
BCN_API int bcn_episode_track(bcn_env_t h, const void* out_buf_dev, void* ep_buf_dev, const uint8_t* mask_dev, void* stream);
/* Per-jet rewards and returns of shkadov: the multi-agent form of the env, shkadov_separable (shkadov.py:376-481), in which every
 * jet is an agent with its own reward, for all B replicas and without host work.  ONE kernel launch on `stream` behind
 * bcn_shkadov_step (no host synchronisation, no host read, no allocation, no atomics: it can be captured into a graph, and two runs
 * agree bit for bit).  The per-jet buffer belongs to the caller (bcn_shkadov_jets_bytes(h) bytes, 16-byte aligned, zeroed before
 * its first use); its segments, in this order, every start a multiple of 16 bytes, each [B][n_jets]:
 *   rwd_jets real     the reward of every jet after the step
 *   ret real          the return of every jet in the episode in progress
 *   last_ret real     that of the replica's last finished episode
 *   sum_ret float64   the sum of the finished returns
 * bcn_shkadov_jets_bytes replaces nothing in the reference (its rewards are host scalars); 0 and bcn_last_error for a NULL or
 * non-shkadov handle.  bcn_shkadov_jets_layout writes the segments as bcn_snapshot_seg with planes = 1 and row_elems = n_jets, as
 * bcn_episode_layout does, and returns their number, 4 (only the first max_segs are written; 0 and bcn_last_error on a bad argument).
 * bcn_shkadov_jet_rewards replaces shkadov_separable.get_rwd (shkadov.py:469-481) and the blow-up rule of shkadov_separable.step
 * (:441-445).  out_buf_dev is the packed output buffer the step wrote (bcn_snapshot_save: [obs | rwd | status | done | trunc]).
 * For every replica b that bcn_set_mask leaves on and every jet j, with s = jet_pos + j jet_space:
 *   rwd_jets[b][j] = -(sum_{c = s .. s + l_rwd - 1, c < nx} (h[b][c] - 1)^2 * dx) / (n_jets l_rwd)
 *                    or blowup_rwd where status[b] has BCN_ST_BLOWUP (the step's own flag: the film is not scanned again);
 *   with_stats != 0, fin = done[b] | trunc[b]:
 *     ret[b][j] += rwd_jets[b][j] (one add in the handle's dtype);
 *     if fin: last_ret[b][j] = ret[b][j]; sum_ret[b][j] += (double)ret[b][j]; ret[b][j] = 0.
 *   with_stats == 0 leaves ret, last_ret and sum_ret alone.  A replica the mask switches off keeps its rows of all four.
 * Episode lengths and counts are those of bcn_episode_track (one episode clock for all jets of a replica).  Call it after the step
 * and before the reset of the finished replicas, which overwrites the film.  BCN_ERR_ARG, and nothing dereferenced, for a NULL
 * handle or buffer and for a handle of another env. */
BCN_API size_t bcn_shkadov_jets_bytes(bcn_env_t h);
BCN_API int bcn_shkadov_jets_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs);
BCN_API int bcn_shkadov_jet_rewards(bcn_env_t h, const void* out_buf_dev, void* jets_buf_dev, int with_stats, void* stream);
/* Running normalisation of observations and rewards over the batch (what the VecNormalize wrapper of the common RL libraries
 * computes with a dozen tensor operations per step; the reference has no counterpart), on the device, behind a step or a reset:
 * at most TWO kernel launches on `stream`, ONE with training == 0 -- no host synchronisation, no host read, no allocation, no
 * atomics: it can be captured into a graph, and the same buffer and inputs give the same bits every time.  The normaliser buffer
 * belongs to the caller (bcn_normalize_bytes(h) bytes, 16-byte aligned, zeroed before its first use and then obs_var and ret_var
 * set to 1); its segments, in this order, every start a multiple of 16 bytes:
 *   obs_mean, obs_var float64 [n_obs]; obs_count float64 [1]       running mean, population variance and sample count per column
 *   ret_mean, ret_var, ret_count float64 [1]                       those of the discounted return
 *   ret float64 [B]                                                the discounted return of every replica
 *   norm_obs real [B][n_obs], norm_rwd real [B], norm_final_obs real [B][n_obs]   the outputs, in the handle's dtype
 *   scratch uint8                                                  private to the kernels; its contents mean nothing to a caller
 * bcn_normalize_layout writes them as bcn_snapshot_seg and returns their number, 11 (only the first max_segs are written; 0 and
 * bcn_last_error on a bad argument).  A segment that scales with the batch has planes = 1, as in bcn_episode_layout: B rows of
 * row_elems elements.  One that does NOT scale with the batch has planes = 0, and row_elems is the number of its elements.
 * bcn_normalize: out_buf_dev is the packed output buffer [obs | rwd | status | done | trunc] a step or reset wrote; ep_buf_dev
 * (NULL: none) the episode buffer of bcn_episode_track, of which `finished` and `final_obs` are read; mask_dev uint8[B] (NULL: all;
 * the mask of bcn_set_mask plays no part).  With S = { b : mask[b] != 0, and -- kind BCN_NORM_STEP only -- status[b] has neither
 * BCN_ST_ITMAX nor BCN_ST_BLOWUP }, n = |S|, and for a column x (all in float64):
 *   update (training != 0, n > 0):  m_b = mean_S x; M2_b = sum_S (x - m_b)^2, summed from deviations; d = m_b - mean; tot = count + n;
 *                                   mean' = mean + d n / tot; var' = (var count + M2_b + d^2 count n / tot) / tot; count' = tot
 *   apply:                          y = clip((x - mean') / sqrt(var' + eps), -clip, clip), rounded once to the handle's dtype
 * kind BCN_NORM_STEP: the columns of obs are updated and norm_obs[b] written for mask[b] != 0; ret[b] = gamma ret[b] + rwd[b] for
 *   mask[b] != 0, the return statistics updated from ret over S, norm_rwd[b] = clip(rwd[b] / sqrt(ret_var' + eps), +-clip_rwd), then
 *   ret[b] = 0 where done[b] | trunc[b]; with ep_buf_dev, norm_final_obs[b] = apply(final_obs[b]) where mask[b] != 0 and
 *   finished[b] != 0 (these rows are NOT counted: behind a masked reset obs already holds the reset observation, which is).
 * kind BCN_NORM_RESET: status is ignored (it is stale); observation statistics and norm_obs of the masked replicas only, and their
 *   ret becomes 0; norm_rwd and the return statistics stay.
 * training == 0: apply only, with the statistics as they are; nothing but the three outputs is written.
 * A replica the mask switches off keeps its rows of every output and its ret.  BCN_ERR_ARG, and nothing dereferenced, for a NULL
 * handle or buffer, a misaligned buffer, another kind, gamma outside [0, 1] or eps, clip_obs, clip_rwd <= 0. */
enum { BCN_NORM_STEP = 0, BCN_NORM_RESET = 1 };
BCN_API size_t bcn_normalize_bytes(bcn_env_t h);
BCN_API int bcn_normalize_layout(bcn_env_t h, bcn_snapshot_seg* segs, int max_segs);
BCN_API int bcn_normalize(bcn_env_t h, const void* out_buf_dev, void* norm_buf_dev, const void* ep_buf_dev, const uint8_t* mask_dev,
                          int kind, int training, double gamma, double eps, double clip_obs, double clip_rwd, void* stream);
/* Rollout storage and generalised advantage estimation: what an on-policy trainer keeps after every step and computes after every
 * rollout, on the device (the reference has no counterpart: its trainers keep Python lists).  No host synchronisation, no host read,
 * no allocation, no atomics: every call can be captured into a graph, and the same inputs give the same bits every time.  The
 * rollout buffer belongs to the caller (bcn_rollout_bytes(h, T, flags) bytes, 16-byte aligned, zeroed before its first use); its
 * segments, in this order, every start a multiple of 16 bytes, for T steps of the handle's B replicas:
 *   cursor int32 [4]                    [0] steps recorded so far, [1] sticky overflow flag; planes = 0
 *   obs real [T + 1][B][n_obs]          obs[0]: the observations bcn_rollout_begin found; obs[t + 1]: those step t returned
 *   act [T][B][n_act] real, or [T][B] int32 for the envs with discrete actions (mixing, lorenz)
 *   rwd real [T][B], status int32 [T][B], done, trunc, valid uint8 [T][B]
 *   final_obs real [T][B][n_obs]        with BCN_RO_FINAL_OBS: rows of the replicas that finished in step t
 *   rwd_jets real [T][B][n_jets]        with BCN_RO_JETS (shkadov): the per-jet rewards of step t
 *   adv, ret real [T][B cols]           written by bcn_rollout_gae; room for cols = n_jets with BCN_RO_JETS, else 1
 * bcn_rollout_layout writes them as bcn_snapshot_seg and returns their number, 12 (only the first max_segs are written; 0 and
 * bcn_last_error on a bad argument): planes = T (obs: T + 1) arrays of B rows of row_elems elements one behind the other; a segment
 * whose flag is off has row_elems = 0 and takes no bytes, so the names and their order are fixed.
 * bcn_rollout_begin: cursor = 0, overflow = 0, obs[0] = the obs of out_buf_dev, or norm_obs of norm_buf_dev (bcn_normalize) when one
 * is passed.  ONE launch.
 * bcn_rollout_record, behind a step (and behind bcn_episode_track, the masked reset and bcn_normalize when those run), with
 * t = cursor[0] read on the device: t >= T writes no slot and sets the overflow flag; otherwise, for every replica b,
 *   on = mask_dev == NULL || mask_dev[b] != 0 (uint8[B]; the mask of bcn_set_mask plays no part);
 *   rwd[t][b] = on ? rwd[b] : 0; done / trunc[t][b] = on ? done / trunc[b] : 0; valid[t][b] = on; status[t][b] = status[b];
 *   obs[t + 1][b] = obs[b] (a replica that was not stepped still holds its row);
 *   act[t][b] = act_dev[b] where on (act_dev: the element type and row length of the act segment; NULL records zeros);
 *   final_obs[t][b] = final_obs[b] of ep_buf_dev where its finished[b] != 0 (BCN_RO_FINAL_OBS and ep_buf_dev given);
 *   rwd_jets[t][b] = rwd_jets[b] of jets_buf_dev (bcn_shkadov_jet_rewards; needs BCN_RO_JETS);
 * and cursor[0] = t + 1.  With norm_buf_dev, obs, rwd and final_obs are norm_obs, norm_rwd and norm_final_obs of that buffer.  TWO
 * launches: the record, in which every workgroup reads the cursor and none writes it, and one lane that advances it.
 * bcn_rollout_gae: with n = min(cursor[0], T) read on the device, for every column c of [B cols] (cols = 1: rwd; cols = n_jets, which
 * needs BCN_RO_JETS: rwd_jets; the flags are those of replica c / cols), nv = last_value[c], gae = 0, and t = n - 1 ... 0:
 *   valid[t] == 0:  adv[t] = 0; ret[t] = values[t]; nv and gae pass through
 *   else            fin = done[t] | trunc[t]; boot = final_values_dev != NULL && trunc[t] ? final_values[t] : 0;
 *                   delta = rwd[t] + gamma (fin ? boot : nv) - values[t]; gae = delta + (fin ? 0 : gamma lam gae);
 *                   adv[t] = gae; ret[t] = gae + values[t]; nv = values[t]
 * in float64 whatever the handle's dtype, rounded once on store; rows t >= n of adv and ret are not written, and rows of
 * final_values without trunc are not used (they may hold anything).  values_dev, final_values_dev: real [T][B cols]; last_value_dev: real [B cols].  adv and
 * ret are [T][B cols] from the start of their segments.  ONE launch, a lane per column.
 * BCN_ERR_ARG (bcn_rollout_bytes / _layout: 0), and nothing dereferenced, for a NULL handle or buffer, a misaligned buffer, T < 1,
 * unknown flags, BCN_RO_JETS on another env than shkadov, another cols, gamma or lam outside [0, 1].  The size of the buffers is the
 * caller's to get right (the torch ops check it). */
enum { BCN_RO_FINAL_OBS = 1, BCN_RO_JETS = 2 };
BCN_API size_t bcn_rollout_bytes(bcn_env_t h, int T, int flags);
BCN_API int bcn_rollout_layout(bcn_env_t h, int T, int flags, bcn_snapshot_seg* segs, int max_segs);
BCN_API int bcn_rollout_begin(bcn_env_t h, void* ro_buf_dev, const void* out_buf_dev, const void* norm_buf_dev, void* stream);
BCN_API int bcn_rollout_record(bcn_env_t h, const void* out_buf_dev, void* ro_buf_dev, const void* act_dev, const void* ep_buf_dev,
                               const void* norm_buf_dev, const void* jets_buf_dev, const uint8_t* mask_dev, int T, int flags, void* stream);
BCN_API int bcn_rollout_gae(bcn_env_t h, void* ro_buf_dev, const void* values_dev, const void* last_value_dev, const void* final_values_dev,
                            int T, int flags, int cols, double gamma, double lam, void* stream);
/* Frames: what the reference's render() draws (rayleigh.py:278-341, mixing.py:267-359, burgers.py:169-213, shkadov.py:267-350,
 * sloshing.py:247-295), for any subset of the batch, as uint8 RGB frames [n][H_px][W_px][3] (HWC, contiguous) in a caller-owned
 * device buffer: ONE kernel launch on `stream` that reads the handle's persistent state -- one plane of the fields and the stored
 * action -- and writes nothing but the frames; no host synchronisation, no host read, no allocation, no atomics, so it can be
 * captured into a graph next to *_step.  Frame f shows replica replicas_dev[f] (int32 [n] on the device; an index outside [0, B)
 * leaves its frame untouched and forms no address), or replica f with replicas_dev NULL, which needs n == B.  lorenz and vortex keep
 * no trajectory on the device: BCN_ERR_UNSUPPORTED.
 * The rules below use only operations that round alike on host and device -- one subtraction, one IEEE division, one product with
 * a power of two or with H, truncation, integers -- in the handle's dtype, with lo, hi, ref narrowed to it first; tests/render_ref.py
 * restates them in NumPy and tests/test_gpu_render.py holds the kernels to it byte for byte.
 *   bin(t, n) = 0 for t <= 0, n - 1 for t >= 1, else min(int(t n), n - 1).
 * Field panel (rayleigh, mixing): W_px = nx scale, H = ny scale.  Panel pixel (r, c) shows cell i = 1 + c / scale, j = ny - r / scale
 *   (integer divisions) of the plane -- np.rot90(T[1:-1, 1:-1]) under imshow: the top pixel row is the top of the domain, nearest
 *   neighbour.  t = (value - lo) / (hi - lo); pixel = lut[bin(t, 256)], and (0, 0, 0) for a NaN t.  lut_dev: uint8 [256][3], 4-byte
 *   aligned (beacon_amd.render.colormap_lut() is RdBu_r, the reference's).  has_range == 0: (Tc, Th) for rayleigh and (0, C0) for
 *   mixing, the reference's vmin / vmax -- for BCN_PLANE_SCALAR only; u, v and p need a range.
 * Line panel (burgers u, shkadov h, sloshing h[1 .. nx]; n samples): W_px = width (0: 512), H = height (0: 128).
 *   row(y) = bin((hi - y) / (hi - lo), H).  Column c covers the samples (c n) / W .. min(((c + 1) n) / W, n - 1), the first sample of
 *   the next column included: that joins the curve.  Paint order: white; row(ref) in (160, 160, 160); then every row from the
 *   smallest to the largest row(y_i) of the column's samples in (31, 119, 180).  A column with a non-finite sample is (255, 0, 0)
 *   over the whole panel height: how a blown-up replica shows.  has_range == 0: the reference's axes -- burgers (u_target - 2 sigma,
 *   u_target + 2 sigma), ref u_target, with sigma the handle's noise setting (bcn_set_noise; without noise burgers needs a range);
 *   shkadov (0, 2), ref 1; sloshing (0.25, 1.75), ref 1.
 * Control strip: `strip` rows under the panel (negative: H / 8; 0: none), white, one cell per control: rayleigh's n_sgts segments,
 *   mixing's four wall speeds u_t, u_b, v_l, v_r over u_max as get_control assigns them to the stored action index (mixing.py:212-234),
 *   the one control of burgers and sloshing, shkadov's n_jets jets -- the value the last step stored (a_last; a NaN counts as 0),
 *   clamped to [-1, 1].  Control k owns the columns [(k W) / n_ctrl, ((k + 1) W) / n_ctrl), c0 to c1, and its bar the middle half of
 *   them, [c0 + (c1 - c0) / 4, c1 - (c1 - c0) / 4).  With m = strip / 2 and nrow = (int(|c| (2 m)) + 1) / 2 -- |c| m rounded half up --
 *   the bar takes the strip rows [m - nrow, m) in (255, 0, 0) for c > 0 and [m, m + nrow) in (0, 0, 255) for c < 0, the reference's
 *   bar colours.  A reset stores zero actions, so nothing is drawn after it -- except for mixing, whose reset stores action 1 as the
 *   reference's does (mixing.py:102).  Equal cells for shkadov's jets are a simplification: the reference draws each bar at its
 *   jet's position along the film.
 * Limits: W_px <= 4096, H <= 16384 for the line panel.  BCN_ERR_ARG, and nothing launched, for a null handle or cfg, an unknown plane,
 * scale < 1, hi <= lo (also after narrowing) or a non-finite lo, hi, ref, n < 0, n != B without an index list, a null or misaligned
 * table where one is needed.  bcn_render_shape: the frame's H_px = H + strip and W_px under the same checks. */
enum { BCN_PLANE_SCALAR = 0, BCN_PLANE_U = 1, BCN_PLANE_V = 2, BCN_PLANE_P = 3 };
typedef struct {
  int32_t plane;                  /* field panel: BCN_PLANE_*; line panel: unused */
  int32_t scale;                  /* field panel: pixels per cell side, >= 1 */
  int32_t width, height;          /* line panel: pixels; 0 = 512 / 128 */
  int32_t strip;                  /* rows of the control strip; negative = panel height / 8, 0 = none */
  int32_t has_range;              /* 0: the reference's range; else lo, hi (and ref) below */
  double lo, hi;                  /* vmin, vmax of the field panel / ymin, ymax of the line panel */
  double ref;                     /* line panel: the reference level drawn in grey */
} bcn_render_cfg;
BCN_API int bcn_render_shape(bcn_env_t h, const bcn_render_cfg* cfg, int* H_px, int* W_px);
BCN_API int bcn_render(bcn_env_t h, const bcn_render_cfg* cfg, const uint8_t* lut_dev, const int32_t* replicas_dev, int n, uint8_t* rgb_dev,
                       void* stream);
/* name of the kernel the last *_step dispatched, e.g. "ns2d_fast_sched" (before the first step: the
 * variant's plain kernel); for profiles */
BCN_API const char* bcn_kernel_name(bcn_env_t h);
/* shape of the 1D step kernel the last *_step dispatched (burgers, shkadov, sloshing): cells per thread K and threads per
 * replica NT of the instantiation, K * NT >= n.  The launcher picks them from the grid length, the batch and the options
 * "cells_per_thread" / "one_wave" -- and overrides a request that does not fit (K is raised while n > 1024 K; grids up to 512
 * cells run as one wave unless one_wave is 0) -- so this is how a caller learns what ran.  The packed and exact-fit one-wave
 * kernels report K = n / 64 or 4 / 8 with NT = 64.  Before the first step, and for envs without the notion: 0, 0. */
BCN_API int bcn_kernel_shape(bcn_env_t h, int* cells_per_thread, int* threads);
BCN_API int bcn_destroy(bcn_env_t h);
BCN_API const char* bcn_last_error(void);
BCN_API const char* bcn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BEACON_HIP_H */

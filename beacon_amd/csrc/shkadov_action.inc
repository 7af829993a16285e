// shkadov_action.inc -- the body shared by shkadov_step_k and shkadov_warm_k (env1d_impl.inc has the description).  Included inside a
// kernel, behind its mask return and shkadov_params(A); in scope: real, K, NT, the argument block A, constexpr bool WARM, and
// n_steps (const int32_t*), rand_steps (int), n_out (int32_t*) -- read only where WARM is true.
  constexpr int NB = (4 * NT * K * sizeof(real) <= 65536) ? 2 : 1;
  __shared__ __attribute__((aligned(8))) real lh[NB][NT * K + 8];   // + 8: guard words around the two halves of the interleaved layout (lidx
  __shared__ __attribute__((aligned(8))) real lq[NB][NT * K + 8];   //      below), one of them the slot holding 1 for reads outside the array
  // q^2 / (h + eps) of every cell, computed once by its owner (halo cells read it) -- where a third exchange array fits LDS
  constexpr bool XE2 = 3 * NB * (NT * K + 8) * sizeof(real) <= 150000;
  __shared__ __attribute__((aligned(8))) real le2[XE2 ? NB : 1][XE2 ? NT * K + 8 : 1];
  __shared__ real red[NT / BCN_WAVE];
  __shared__ real s_u[64], s_up[64];
  const int b = blockIdx.x, tid = threadIdx.x, i0 = tid * K, n = A.n;
  real* gh = A.f0 + (size_t)b * n;
  real* gq = A.f1 + (size_t)b * n;
  real* grh = A.f2 + (size_t)b * n;
  real* grq = A.f3 + (size_t)b * n;
  // float32 works on the DEVIATIONS from the flat film, h - 1 and q - 1 (DEVF; float64 keeps the reference's variables and
  // operation order: bit-identical fields).  One AB2 increment of a nearly flat film is 0.5 dt * 3 * rhs ~ 1e-7 -- an ulp of
  // 1.0f -- so with h itself in float32 the small waves that the inlet noise seeds (shkadov.py:204, sigma = 5e-4) stall
  // instead of growing: measured, the N = 4096 film stayed at max|h - 1| = 3e-4 through 2000 action steps where the
  // float64 kernel and the reference reach 1.0.  Every term of the scheme is a difference of neighbours or has the flat
  // state factored out exactly (below), so nothing is lost by subtracting it; the state arrays keep h, q (one rounding
  // per action step, 1e-4 of the noise amplitude).
  constexpr bool DEVF = std::is_same<real, float>::value;
  constexpr real FLAT = DEVF ? real(0) : real(1);     // the flat film in the kernel's variables
  real h[K], q[K], rh[K], rq[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    if constexpr (WARM) {   // shkadov_reset_k's values, as the step kernel would load them
      const real h0 = (c < n && A.init_fields) ? A.init_fields[c] : real(1), q0 = (c < n && A.init_fields) ? A.init_fields[n + c] : real(1);
      h[k] = c < n ? (DEVF ? h0 - real(1) : h0) : FLAT;
      q[k] = c < n ? (DEVF ? q0 - real(1) : q0) : FLAT;
      rh[k] = real(0);
      rq[k] = real(0);
    } else {
      h[k] = c < n ? (DEVF ? gh[c] - real(1) : gh[c]) : FLAT;
      q[k] = c < n ? (DEVF ? gq[c] - real(1) : gq[c]) : FLAT;
      rh[k] = c < n ? grh[c] : real(0);
      rq[k] = c < n ? grq[c] : real(0);
    }
  }
  // q^2 / (h + eps) (:213) -- float32: minus 1, exactly: ((1+q')^2 - (1+h') - eps) / (1 + h' + eps)
  auto e2of = [&](const real qv, const real hv) -> real {
    if constexpr (DEVF) return fdiv<real>(qv * (real(2) + qv) - (hv + A.eps), (real(1) + hv) + A.eps);
    else return fdiv<real>(qv * qv, hv + A.eps);
  };
  // action shift: up <- u, u <- new (shkadov.py:193-194)
  if (tid < A.n_jets) {
    const real uo = WARM ? real(0) : A.a_last[(size_t)b * A.n_jets + tid];   // WARM: a_last = a_prev = 0 (reset), and the stored action repeats
    const real un = (!WARM && A.actions) ? A.actions[(size_t)b * A.n_jets + tid] : uo;
    s_u[tid] = un;
    s_up[tid] = uo;
    A.a_last[(size_t)b * A.n_jets + tid] = un;
    A.a_prev[(size_t)b * A.n_jets + tid] = uo;
  }
  const real* nz = (!WARM && A.noise) ? A.noise + (size_t)b * A.ndt_act : nullptr;
  // the inlet noise of every timestep, staged once: a global load per timestep in wave 0 would sit in front of the
  // barrier that all 16 waves wait at
  constexpr int NZ = 128;
  __shared__ real s_nz[NZ];
  __shared__ real s_alpha[NZ];   // the jets' ramp of every timestep (:219-221): one division each, once, instead of in every thread and timestep
  const bool dev_noise = !nz && A.nsigma > real(0);   // drawn here, one value per timestep (shkadov.py:204; bcn_set_noise)
  const uint32_t ctr0 = (WARM || dev_noise) ? A.nctr[b] : 0u;
  uint32_t nctr = WARM ? ctr0 + 1u : ctr0;            // WARM: the count's tick; then one per action step with device noise
  int n_warm = 1;                                     // action steps taken here
  if constexpr (WARM) {
    if (n_steps) {
      n_warm = min(max(n_steps[b], 0), rand_steps);
    } else {
      uint32_t o[4];
      bcn_philox4x32((uint32_t)(b + A.noff), ctr0, 0u, 1u, A.nseed_lo, A.nseed_hi, o);
      n_warm = (int)__umulhi(o[0], (uint32_t)rand_steps + 1u);
    }
    n_warm = __builtin_amdgcn_readfirstlane(n_warm);   // one value per workgroup: the loop below holds barriers
  }
  for (int k = tid; k < NZ && k < A.ndt_act; k += NT) {
    s_nz[k] = nz ? nz[k] : (dev_noise ? bcn_device_noise<real>(A, b, nctr, k) : real(0));
    s_alpha[k] = fmin((real)k / (real)A.n_interp, real(1));
  }
  const real rdx3 = real(1) / (A.dx * A.dx * A.dx);
  __syncthreads();   // s_u / s_up / s_nz (and every read of nctr[b])
  if constexpr (!WARM) { if (dev_noise && tid == 0) A.nctr[b] = nctr + 1u; }
  // ---- everything that does not change over the action step is resolved once ----------------
  // halo cells i0-2, i0-1, i0+K, i0+K+1, i0+K+2: LDS index with the outflow copy BC
  // h[nx-1] = h[nx-2], q[nx-1] = q[nx-2] (shkadov.py:206-207) resolved on read; cells outside the
  // array read a slot that holds 1 (never used by a cell that is updated)
  constexpr int ONE = 0;
  // LDS layout: cell c = tid*K + k sits at k*NT + tid (consecutive lanes -> consecutive banks; the cell-major layout
  // c is a K-way bank conflict on every exchange access).  float32 with four cells per thread (IL, the packed step below):
  // cells 0, 2 of thread t at 2t, 2t + 1 and cells 1, 3 at RB + 2t, RB + 2t + 1 -- every PAIR of cells two apart, (c-2, c0),
  // (c0, c2), (c2, c4), (c-1, c1), ... is then two adjacent words: one 64-bit access (8 bytes per lane: conflict-free).  Word 0 is
  // the slot for reads outside the array; the words in front of and behind each half (RA - 1, RA + 2 NT .. + 1, RB - 1, RB + 2 NT ..
  // + 1) are what the first thread reads below and the last thread above the array in the packed step: they hold the flat film.
  constexpr bool IL = std::is_same<real, float>::value && K == 4;
  constexpr int RA = IL ? 2 : 1, RB = 2 * NT + 6;
  auto own = [&](int k) -> int { return IL ? ((k & 1) ? RB : RA) + 2 * tid + (k >> 1) : RA + k * NT + tid; };
  auto lidx = [&](int c) -> int { return IL ? (((c % K) & 1) ? RB : RA) + 2 * (c / K) + ((c % K) >> 1) : RA + (c % K) * NT + c / K; };
  auto hidx = [&](int c) -> int { return (c < 0 || c >= n) ? ONE : lidx(c == n - 1 ? n - 2 : c); };
  const int xm2 = hidx(i0 - 2), xm1 = hidx(i0 - 1), xp0 = hidx(i0 + K), xp1 = hidx(i0 + K + 1), xp2 = hidx(i0 + K + 2);
  const int xn2 = lidx(n >= 2 ? n - 2 : 0);
  const bool has_last = (i0 <= n - 1) && (n - 1 < i0 + K);   // this thread owns cell nx-1
  const bool has_tail = (i0 + K > n - 3) && (i0 <= n - 2);   // ... cells nx-3 / nx-2 (one-sided d3o2u)
  // jets (:223-232): parabolic profile on [s, e], s = jet_pos + j*space - hw, e = s + 2 hw
  real jvv[K], ju0[K], ju1[K];
  bool jon[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int rel = i0 + k - (A.jet_pos - A.jet_hw);
    const int j = rel >= 0 ? rel / A.jet_space : 0;
    const int ks = rel - j * A.jet_space;              // k - s
    jon[k] = rel >= 0 && j < A.n_jets && ks <= 2 * A.jet_hw;
    jvv[k] = (real)(ks * (2 * A.jet_hw - ks)) / (real(0.25) * (real)(4 * A.jet_hw * A.jet_hw));
    ju0[k] = jon[k] ? s_up[j] : real(0);
    ju1[k] = jon[k] ? s_u[j] : real(0);
  }
  if (tid < 8) {   // the slot for reads outside the array and (IL) the guard words of both halves
    const int gw[8] = {ONE, IL ? RA - 1 : ONE, IL ? RA + 2 * NT : ONE, IL ? RA + 2 * NT + 1 : ONE, IL ? RB - 1 : ONE, IL ? RB + 2 * NT : ONE,
                       IL ? RB + 2 * NT + 1 : ONE, ONE};
    const int g = gw[tid];
    lh[0][g] = FLAT; lq[0][g] = FLAT; lh[NB - 1][g] = FLAT; lq[NB - 1][g] = FLAT;
    if constexpr (XE2) { le2[0][g] = e2of(FLAT, FLAT); le2[NB - 1][g] = le2[0][g]; }
  }

  // Waves whose cells are all away from both ends of the array (all but the first and the last one on the
  // reference grids) run a body without edge cases; waves without jet cells skip the forcing.  Both flags are
  // wave-uniform, every variant executes the one barrier of the timestep.
  const bool t_int = (i0 >= 2) && (i0 + K + 2 <= n - 2);
  bool t_jet = false;
#pragma unroll
  for (int k = 0; k < K; k++) t_jet = t_jet || jon[k];
  const bool w_int = __builtin_amdgcn_ballot_w64(!t_int) == 0;
  const bool w_jet = __builtin_amdgcn_ballot_w64(t_jet) != 0;
#ifdef BCN_STAMP_1D
  unsigned long long st_sync = 0, st_read = 0, st_comp = 0;
#endif
  auto step = [&](const int it, auto int_tag, auto jet_tag) {
    constexpr bool INT = decltype(int_tag)::value, JET = decltype(jet_tag)::value;
    real* Lh = lh[it & (NB - 1)];
    real* Lq = lq[it & (NB - 1)];
    real* Le2 = le2[XE2 ? (it & (NB - 1)) : 0];
    if (!INT && tid == 0) {                           // inlet BC (:204-205)
      h[0] = FLAT + (it < NZ ? s_nz[it] : (nz ? nz[it] : (dev_noise ? bcn_device_noise<real>(A, b, nctr, it) : real(0))));
      q[0] = FLAT;
    }
#ifdef BCN_STAMP_1D
    const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
    real e2[K + 3];  // q^2/(h+eps) at cells i0-2 .. i0+K (:213): the thread's own cells here, the halo cells from their owners
#pragma unroll
    for (int k = 0; k < K; k++) {
      e2[k + 2] = e2of(q[k], h[k]);
      Lh[own(k)] = h[k]; Lq[own(k)] = q[k];
      if constexpr (XE2) Le2[own(k)] = e2[k + 2];
    }
    __syncthreads();
#ifdef BCN_STAMP_1D
    const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
    real eh[K + 5];  // cells i0-2 .. i0+K+2
    real eq[K + 3];  // cells i0-2 .. i0+K
    eh[0] = Lh[xm2]; eh[1] = Lh[xm1];
    eq[0] = Lq[xm2]; eq[1] = Lq[xm1];
    if (!INT && has_last) {
#pragma unroll
      for (int k = 0; k < K; k++)
        if (i0 + k == n - 1) {                                              // outflow copy (:206-207)
          h[k] = Lh[xn2]; q[k] = Lq[xn2];
          e2[k + 2] = XE2 ? Le2[xn2] : e2of(q[k], h[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      eh[k + 2] = h[k];
      eq[k + 2] = q[k];
    }
    eh[K + 2] = Lh[xp0]; eh[K + 3] = Lh[xp1]; eh[K + 4] = Lh[xp2];
    eq[K + 2] = Lq[xp0];
#ifdef BCN_STAMP_1D
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
#endif
    if constexpr (XE2) {
      e2[0] = Le2[xm2]; e2[1] = Le2[xm1]; e2[K + 2] = Le2[xp0];
    } else {
      e2[0] = e2of(eq[0], eh[0]);
      e2[1] = e2of(eq[1], eh[1]);
      e2[K + 2] = e2of(eq[K + 2], eh[K + 2]);
    }
    // minmod limiter at cells i0-1 .. i0+K-1 (zero at both array ends, :497-500), as the product mq = phi * (u[c+1] - u[c])
    // that d1tvd uses (:501-503).  float32: clip(a / (b + 1e-8), 0, 1) * b is med3(a, 0, b) -- minmod itself -- up to the
    // 1e-8 of the denominator: one v_med3_f32 instead of a reciprocal, two multiplications and the clip (10 of the 21
    // reciprocals of a thread's timestep; each v_rcp_f32 costs four plain instructions).  float64 keeps the reference's
    // operations (bit-identical fields).
    real mq[K + 1], m2[K + 1];
#pragma unroll
    for (int k = 0; k <= K; k++) {
      const int c = i0 - 1 + k;
      const bool edge = !INT && (c <= 0 || c >= n - 1);
      const real a1 = eq[k + 1] - eq[k], b1 = eq[k + 2] - eq[k + 1];
      const real a2 = e2[k + 1] - e2[k], b2 = e2[k + 2] - e2[k + 1];
      if constexpr (std::is_same<real, float>::value) {
        mq[k] = edge ? real(0) : __builtin_amdgcn_fmed3f(a1, 0.0f, b1);
        m2[k] = edge ? real(0) : __builtin_amdgcn_fmed3f(a2, 0.0f, b2);
      } else {
        const real r1 = fdiv<real>(a1, b1 + real(1.0e-8)), r2 = fdiv<real>(a2, b2 + real(1.0e-8));
        mq[k] = (edge ? real(0) : np_clip01(r1)) * b1;
        m2[k] = (edge ? real(0) : np_clip01(r2)) * b2;
      }
    }
    // d3o2u(h) (:485-491); eh index of cell c is k+2; the last two interior cells are one-sided
    real d3[K];
#pragma unroll
    for (int k = 0; k < K; k++)
      d3[k] = divc<real>(-eh[k + 5] + real(6) * eh[k + 4] - real(12) * eh[k + 3] + real(10) * eh[k + 2] -
                             real(3) * eh[k + 1], real(2) * A.dx * A.dx * A.dx, real(0.5) * rdx3);
    if (!INT && has_tail) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int c = i0 + k;
        if (c == n - 3) d3[k] = divc<real>(eh[k + 4] - real(3) * eh[k + 3] + real(3) * eh[k + 2] - eh[k + 1], A.dx * A.dx * A.dx, rdx3);
        if (c == n - 2) d3[k] = divc<real>(-eh[k] + real(3) * eh[k + 1] - real(3) * eh[k + 2] + eh[k + 3], A.dx * A.dx * A.dx, rdx3);
      }
    }
    const real alpha = JET ? (it < NZ ? s_alpha[it] : fmin((real)it / (real)A.n_interp, real(1))) : real(0);
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int c = i0 + k;
      const real rhp = rh[k], rqp = rq[k];            // rhs of the previous timestep (:200-201)
      // d1tvd(q) -> rhsh, d1tvd(q2h) -> dq2h (:494-504)
      real dq = eq[k + 2] + real(0.5) * mq[k + 1];
      dq -= eq[k + 1] + real(0.5) * mq[k];
      dq = divc<real>(dq, A.dx, A.rdx);
      real d2 = e2[k + 2] + real(0.5) * m2[k + 1];
      d2 -= e2[k + 1] + real(0.5) * m2[k];
      d2 = divc<real>(d2, A.dx, A.rdx);
      // rhsq (:507-512)
      real rqn;
      if constexpr (DEVF) {
        // h (dddh + 1) - q / (h^2 + eps) with h = 1 + h', q = 1 + q':  h dddh + (h^3 + h eps - q) / (h^2 + eps), and
        // h^3 - q = h' (3 + h' (3 + h')) - q'
        const real hh = real(1) + h[k];
        const real num = h[k] * (real(3) + h[k] * (real(3) + h[k])) + (hh * A.eps - q[k]);
        rqn = real(1.2) * d2 - A.delta_p * (hh * d3[k] + fdiv<real>(num, hh * hh + A.eps));
      } else {
        rqn = real(1.2) * d2 - A.delta_p * (h[k] * (d3[k] + real(1)) - fdiv<real>(q[k], h[k] * h[k] + A.eps));
      }
      if (JET) {
        const real uj = (real(1) - alpha) * ju0[k] + alpha * ju1[k];
        const real rqj = rqn + A.jet_amp * uj * jvv[k];
        rqn = jon[k] ? rqj : rqn;
      }
      if (INT || (c >= 1 && c <= n - 2)) {
        rh[k] = dq;
        rq[k] = rqn;
        h[k] += real(0.5) * A.dt * (real(-3) * dq + rhp);    // adams (:515-518)
        q[k] += real(0.5) * A.dt * (real(-3) * rqn + rqp);
      }
    }
    if (NB == 1) __syncthreads();
#ifdef BCN_STAMP_1D
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long ts3 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    st_sync += ts1 - ts0; st_read += ts2 - ts1; st_comp += ts3 - ts2;
#endif
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  // float32, four cells per thread (BASELINE configs[2]: N = 4096 on 1024 threads), interior waves: the PACKED timestep.  The
  // kernel is bound by vector-instruction throughput (four waves per SIMD, SQ_ACTIVE_INST_VALU 79 %), so two cells per
  // v_pk_{add,mul,fma}_f32 is what pays: a thread holds its cells as the pairs (c0, c2), (c1, c3), every stencil neighbour of a
  // pair is again a pair -- (c-1, c1), (c2, c4), ... -- and the pairs that reach into a neighbouring thread arrive from LDS as
  // one ds_read2st64_b32 each, both halves at once (the row shift of lidx), so none is assembled by v_mov.  Per cell the
  // operations are those of step() above.  162 -> ~100 vector instructions per timestep (interior wave with jets).
  // The waves that hold an end of the array run the same code plus the end conditions as selects on the TWO threads concerned
  // (EDGE; n a multiple of 4: the cells nx-4 .. nx-1 are one thread's): the inlet (:204-205) and the outflow copy (:206-207) set in
  // the registers before the exchange, the limiter zeroed at cells 0 and nx-1 (:497-500), the one-sided third derivatives of
  // cells nx-3, nx-2 (:488-491) in a two-cell branch, cells 0 and nx-1 restored behind the update.  It matters more than the
  // packing: every wave waits at the timestep's barrier for the slowest, and step()'s edge variant -- four exec-masked branches
  // per cell -- took 2.2 x an interior wave's time (measured with every wave on the interior path: 0.36 -> 0.265 ms).
  constexpr bool PK = DEVF && K == 4 && NB == 2 && XE2;
  int ia = 0;
  if (!WARM || n_warm > 0) do {   // !WARM: once, and no loop at all
  if constexpr (WARM) {
    if (ia > 0) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        if constexpr (DEVF) { h[k] = (real(1) + h[k]) - real(1); q[k] = (real(1) + q[k]) - real(1); }   // the state arrays keep h, q
        if (i0 + k >= n) { h[k] = FLAT; q[k] = FLAT; rh[k] = real(0); rq[k] = real(0); }
      }
      if (dev_noise) nctr += 1u;
      __syncthreads();   // every read of s_nz and of the exchange buffers by the action step before
      for (int k = tid; k < NZ && k < A.ndt_act; k += NT) s_nz[k] = dev_noise ? bcn_device_noise<real>(A, b, nctr, k) : real(0);
      __syncthreads();
    }
  }
    bool done_pk = false;
    if constexpr (PK) {
      const bool pk_ok = A.ndt_act <= NZ && A.one_wave != 2 && (n & 3) == 0 && n >= 16 && n <= NT * K;
      if (pk_ok) {
        typedef bcn_f2 f2;
        f2 hP[2] = {{h[0], h[2]}, {h[1], h[3]}}, qP[2] = {{q[0], q[2]}, {q[1], q[3]}};
        f2 rhP[2] = {{rh[0], rh[2]}, {rh[1], rh[3]}}, rqP[2] = {{rq[0], rq[2]}, {rq[1], rq[3]}};
        // jets: ju0 = ju1 = 0 outside a jet, so the forcing term is an exact + 0 there and needs no select
        const f2 jvP[2] = {{jvv[0], jvv[2]}, {jvv[1], jvv[3]}}, j0P[2] = {{ju0[0], ju0[2]}, {ju0[1], ju0[3]}},
                 j1P[2] = {{ju1[0], ju1[2]}, {ju1[1], ju1[3]}};
        const int o0 = own(0), o1 = own(1);   // cells c0 | c2 at o0, o0 + 1; c1 | c3 at o1, o1 + 1; the thread above's follow, the thread below's precede
        const f2 eps2 = A.eps, one2 = 1.f, two2 = 2.f, three2 = 3.f, half2 = 0.5f, rdx2 = A.rdx, hrdx3 = 0.5f * rdx3;
        const f2 c6 = 6.f, cm12 = -12.f, c10 = 10.f, cm3 = -3.f, c12 = 1.2f, mdp = -A.delta_p, hdt = 0.5f * A.dt, jamp = A.jet_amp;
        auto rcp2 = [](const f2 x) -> f2 { return (f2){__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)}; };
        auto med2 = [](const f2 a, const f2 b) -> f2 { return (f2){__builtin_amdgcn_fmed3f(a.x, 0.f, b.x), __builtin_amdgcn_fmed3f(a.y, 0.f, b.y)}; };
        auto FMA = [](const f2 a, const f2 b, const f2 c) -> f2 { return __builtin_elementwise_fma(a, b, c); };
        const bool isL = (tid == 0), isR = (tid == n / 4 - 1);   // the threads that hold cell 0 / cells nx-4 .. nx-1
        // EL / ER: the wave holds the first / the last thread of the array (wave-uniform; both only where the array is one wave)
        auto stepP = [&](const int it, auto jet_tag, auto el_tag, auto er_tag, float* __restrict__ Lh, float* __restrict__ Lq, float* __restrict__ Le2) {
          constexpr bool JET = decltype(jet_tag)::value, EL = decltype(el_tag)::value, ER = decltype(er_tag)::value;
          float h0k = 0.f, q0k = 0.f, rh0k = 0.f, rq0k = 0.f, h3k = 0.f, q3k = 0.f, rh3k = 0.f, rq3k = 0.f;
          if constexpr (EL) {
            hP[0].x = isL ? FLAT + s_nz[it] : hP[0].x;   // inlet BC (:204-205)
            qP[0].x = isL ? FLAT : qP[0].x;
            h0k = hP[0].x; q0k = qP[0].x; rh0k = rhP[0].x; rq0k = rqP[0].x;   // cells 0 and nx-1 are not updated (:515-518 write 1 .. nx-2)
          }
          if constexpr (ER) {
            hP[1].y = isR ? hP[0].y : hP[1].y;           // outflow copy h[nx-1] = h[nx-2] (:206-207): every reader sees it
            qP[1].y = isR ? qP[0].y : qP[1].y;
            h3k = hP[1].y; q3k = qP[1].y; rh3k = rhP[1].y; rq3k = rqP[1].y;
          }
          f2 E[5];   // E[j + 2] = q^2/(h + eps) - 1 of cells (j, j + 2), j = -2 .. 2; own: j = 0, 1
#pragma unroll
          for (int j = 0; j < 2; j++) E[j + 2] = FMA(qP[j], two2 + qP[j], -(hP[j] + eps2)) * rcp2((one2 + hP[j]) + eps2);   // e2of
          *(f2*)(Lh + o0) = hP[0]; *(f2*)(Lh + o1) = hP[1];
          *(f2*)(Lq + o0) = qP[0]; *(f2*)(Lq + o1) = qP[1];
          *(f2*)(Le2 + o0) = E[2]; *(f2*)(Le2 + o1) = E[3];
          __syncthreads();
          f2 Q[5], Hh[6];   // Q[j + 2]: cells (j, j + 2), j = -2 .. 2;  Hh[j + 1]: j = -1 .. 4
          Q[0] = (f2){Lq[o0 - 1], Lq[o0]}; Q[1] = (f2){Lq[o1 - 1], Lq[o1]}; Q[2] = qP[0]; Q[3] = qP[1]; Q[4] = (f2){Lq[o0 + 1], Lq[o0 + 2]};
          E[0] = (f2){Le2[o0 - 1], Le2[o0]}; E[1] = (f2){Le2[o1 - 1], Le2[o1]}; E[4] = (f2){Le2[o0 + 1], Le2[o0 + 2]};
          Hh[0] = (f2){Lh[o1 - 1], Lh[o1]}; Hh[1] = hP[0]; Hh[2] = hP[1]; Hh[3] = (f2){Lh[o0 + 1], Lh[o0 + 2]};
          Hh[4] = (f2){Lh[o1 + 1], Lh[o1 + 2]}; Hh[5] = (f2){Lh[o0 + 2], Lh[o0 + 3]};
          // d1tvd(q), d1tvd(q2h) (:494-504): face values T = x + 0.5 minmod(dx-, dx+) of cells (j, j + 2), j = -1, 0, 1
          f2 Dq[4], De[4], Tq[3], Te[3];
#pragma unroll
          for (int j = 0; j < 4; j++) { Dq[j] = Q[j + 1] - Q[j]; De[j] = E[j + 1] - E[j]; }
#pragma unroll
          for (int j = 0; j < 3; j++) { Tq[j] = med2(Dq[j], Dq[j + 1]); Te[j] = med2(De[j], De[j + 1]); }
          // the limiter is zero at both ends of the array (:497-500): cells 0 (pair 0, low) and nx-1 (pair 1, high)
          if constexpr (EL) { Tq[1].x = isL ? 0.f : Tq[1].x; Te[1].x = isL ? 0.f : Te[1].x; }
          if constexpr (ER) { Tq[2].y = isR ? 0.f : Tq[2].y; Te[2].y = isR ? 0.f : Te[2].y; }
#pragma unroll
          for (int j = 0; j < 3; j++) { Tq[j] = FMA(half2, Tq[j], Q[j + 1]); Te[j] = FMA(half2, Te[j], E[j + 1]); }
          f2 dq[2], d2[2], d3[2], rqn[2], hh[2], num[2], den[2];
#pragma unroll
          for (int j = 0; j < 2; j++) { dq[j] = Tq[j + 1] - Tq[j]; d2[j] = Te[j + 1] - Te[j]; }
#pragma unroll
          for (int j = 0; j < 2; j++) { dq[j] = dq[j] * rdx2; d2[j] = d2[j] * rdx2; }
          // d3o2u(h) (:485-491)
#pragma unroll
          for (int j = 0; j < 2; j++) d3[j] = FMA(c6, Hh[j + 3], -Hh[j + 4]);
#pragma unroll
          for (int j = 0; j < 2; j++) d3[j] = FMA(cm12, Hh[j + 2], d3[j]);
#pragma unroll
          for (int j = 0; j < 2; j++) d3[j] = FMA(c10, Hh[j + 1], d3[j]);
#pragma unroll
          for (int j = 0; j < 2; j++) d3[j] = FMA(cm3, Hh[j], d3[j]);
#pragma unroll
          for (int j = 0; j < 2; j++) d3[j] = d3[j] * hrdx3;
          if constexpr (ER) {
            if (isR) {   // one-sided at cells nx-3 = c1 and nx-2 = c2 of this thread (:488-491)
              const float a0 = hP[0].x, a1 = hP[1].x, a2 = hP[0].y, a3 = hP[1].y;
              d3[1].x = (a3 - 3.f * a2 + 3.f * a1 - a0) * rdx3;
              d3[0].y = (-a0 + 3.f * a1 - 3.f * a2 + a3) * rdx3;
            }
          }
          // rhsq (:507-512) in the deviation variables: 1.2 d2 - delta_p (hh dddh + (h'(3 + h'(3 + h')) + hh eps - q') / (hh^2 + eps))
#pragma unroll
          for (int j = 0; j < 2; j++) { hh[j] = one2 + hP[j]; num[j] = three2 + hP[j]; }
#pragma unroll
          for (int j = 0; j < 2; j++) { num[j] = FMA(hP[j], num[j], three2); den[j] = FMA(hh[j], hh[j], eps2); rqn[j] = FMA(hh[j], eps2, -qP[j]); }
#pragma unroll
          for (int j = 0; j < 2; j++) { num[j] = FMA(hP[j], num[j], rqn[j]); den[j] = rcp2(den[j]); }
#pragma unroll
          for (int j = 0; j < 2; j++) num[j] = FMA(hh[j], d3[j], num[j] * den[j]);
#pragma unroll
          for (int j = 0; j < 2; j++) rqn[j] = FMA(mdp, num[j], c12 * d2[j]);
          if constexpr (JET) {   // :223-232
            const float alpha = s_alpha[it];   // (ndt_act <= NZ: checked where this path is chosen)
            const f2 al = alpha, oma = 1.f - alpha;
#pragma unroll
            for (int j = 0; j < 2; j++) rqn[j] = FMA(jamp * FMA(al, j1P[j], oma * j0P[j]), jvP[j], rqn[j]);
          }
          // adams (:515-518)
#pragma unroll
          for (int j = 0; j < 2; j++) {
            hP[j] = FMA(hdt, FMA(cm3, dq[j], rhP[j]), hP[j]);
            qP[j] = FMA(hdt, FMA(cm3, rqn[j], rqP[j]), qP[j]);
            rhP[j] = dq[j]; rqP[j] = rqn[j];
          }
          if constexpr (EL) { hP[0].x = isL ? h0k : hP[0].x; qP[0].x = isL ? q0k : qP[0].x; rhP[0].x = isL ? rh0k : rhP[0].x; rqP[0].x = isL ? rq0k : rqP[0].x; }
          if constexpr (ER) { hP[1].y = isR ? h3k : hP[1].y; qP[1].y = isR ? q3k : qP[1].y; rhP[1].y = isR ? rh3k : rhP[1].y; rqP[1].y = isR ? rq3k : rqP[1].y; }
        };
        int it = 0;
#define BCN_SHK_LOOP(JT, LT, RT)                                                                                                    \
        {                                                                                                                             \
          for (; it + 2 <= A.ndt_act; it += 2) { stepP(it, JT{}, LT{}, RT{}, lh[0], lq[0], le2[0]); stepP(it + 1, JT{}, LT{}, RT{}, lh[1], lq[1], le2[1]); } \
          if (it < A.ndt_act) stepP(it, JT{}, LT{}, RT{}, lh[0], lq[0], le2[0]);                                                      \
        }
        const bool w_l = __builtin_amdgcn_ballot_w64(isL) != 0, w_r = __builtin_amdgcn_ballot_w64(isR) != 0;
        if (w_l && w_r) {
          if (w_jet) BCN_SHK_LOOP(T_, T_, T_) else BCN_SHK_LOOP(F_, T_, T_)
        } else if (w_l) {
          if (w_jet) BCN_SHK_LOOP(T_, T_, F_) else BCN_SHK_LOOP(F_, T_, F_)
        } else if (w_r) {
          if (w_jet) BCN_SHK_LOOP(T_, F_, T_) else BCN_SHK_LOOP(F_, F_, T_)
        } else {
          if (w_jet) BCN_SHK_LOOP(T_, F_, F_) else BCN_SHK_LOOP(F_, F_, F_)
        }
#undef BCN_SHK_LOOP
        h[0] = hP[0].x; h[1] = hP[1].x; h[2] = hP[0].y; h[3] = hP[1].y; q[0] = qP[0].x; q[1] = qP[1].x; q[2] = qP[0].y; q[3] = qP[1].y;
        rh[0] = rhP[0].x; rh[1] = rhP[1].x; rh[2] = rhP[0].y; rh[3] = rhP[1].y; rq[0] = rqP[0].x; rq[1] = rqP[1].x; rq[2] = rqP[0].y; rq[3] = rqP[1].y;
        done_pk = true;
      }
    }
    // one timestep loop per variant (the flags do not change over the action step; every loop executes the same barriers)
    if (done_pk) {
    } else if (w_int) {
      if (w_jet) { for (int it = 0; it < A.ndt_act; it++) step(it, T_{}, T_{}); }
      else { for (int it = 0; it < A.ndt_act; it++) step(it, T_{}, F_{}); }
    } else {
      if (w_jet) { for (int it = 0; it < A.ndt_act; it++) step(it, F_{}, T_{}); }
      else { for (int it = 0; it < A.ndt_act; it++) step(it, F_{}, F_{}); }
    }
  } while (WARM && ++ia < n_warm);
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    if (c < n) { gh[c] = DEVF ? real(1) + h[k] : h[k]; gq[c] = DEVF ? real(1) + q[k] : q[k]; grh[c] = rh[k]; grq[c] = rq[k]; }
    if constexpr (WARM) {   // no action step taken: the film as shkadov_reset_k stores it, not rounded through h - 1
      if (c < n && n_warm == 0 && A.init_fields) { gh[c] = A.init_fields[c]; gq[c] = A.init_fields[n + c]; }
    }
  }
  __syncthreads();
  bool blow;
  real rwd = shkadov_obs_rwd<real, NT>(A, b, red, &blow);
  if constexpr (WARM) {
    if (tid == 0) {
      A.stp[b] = 0;
      A.nctr[b] = ctr0 + 1u + (dev_noise ? (uint32_t)n_warm : 0u);
      if (n_out) n_out[b] = n_warm;
    }
  } else {
    finish<real, NT>(A, b, rwd, blow, A.blowup_rwd, true);   // shkadov.py:176-180
  }
#ifdef BCN_STAMP_1D   // diagnostic build only: cycles per timestep of three waves in obs[0..8]
  if ((tid & 63) == 0 && (tid >> 6) % 5 == 0 && A.obs_out) {
    real* o = A.obs_out + (size_t)b * A.n_obs + 3 * ((tid >> 6) / 5);
    o[0] = (real)st_sync / (real)A.ndt_act; o[1] = (real)st_read / (real)A.ndt_act; o[2] = (real)st_comp / (real)A.ndt_act;
  }
#endif

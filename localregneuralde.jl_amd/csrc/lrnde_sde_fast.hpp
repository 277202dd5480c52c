// lrnde_sde_fast.hpp — the Lamba Euler-Heun step (src/perform_step.jl:172-206) as ONE small-latency launch, for every
// NeuralDSDE whose drift is Chain(Dense(D => H, act), Dense(H => D)) without a time input and whose diffusion is
// Dense(D => D) (src/layers/neural_sde.jl:50-72; experiments/src/construct.jl:204-205 is D = 32, H = 64) with D <= 64 and
// H <= 128.  Included by lrnde_kernels.hip inside its anonymous namespace.
//
// k_sde_step (the generic kernel) runs the step's six field evaluations through feval_tile: per evaluation it restages
// the biases, reloads the resident weight fragments from L2, and passes every intermediate (du1, L, K, tmp, ...) through
// global memory between evaluations — 28 us for 15.7 MFLOP.  Here nothing leaves the CU between the first load of (u, dW) and
// the store of u_new: the weights are resident fragments of the workgroup frame (SdeFrame below, where the layout is described);
// a round = [drift Dense-1 + activation, and this wave's diffusion tile] barrier [drift Dense-2 of this wave's tile + the
// elementwise algebra] barrier; the step is three rounds: (f,g)(u) -> (f,g)(tmp) -> f(K), g(utilde).
// Arithmetic: the canonical dot products (k-ordered fma chains = v_mfma_f32_16x16x4_f32 chains over the k-groups in
// order, segments of 112 rows added left to right — H = 128 has two), the same activation polynomial and the same
// elementwise expressions as k_sde_step, so results are bit-identical to it and to the oracle
// (tests/test_gpu_parity.py::test_sde_*, tests/test_gpu_switches.py).  Rows beyond D / H are zero-padded fragments.
//
// The adaptive solve's controller (lrnde_sde_solve_adaptive, lrnde_sde_node_forward_record) runs in this kernel's footer
// (last workgroup to arrive): PI controller on EEst, position on the caller's Brownian grid, state buffer flip, and — for
// the layer's recorded forward — the dense record of the accepted steps (start index, length, end state) that the
// reverse sweep of lrnde_sde_node_backward_recorded walks.

constexpr int SF_NT = 256;
// -DLRNDE_SDE_STAMPS (tools/sde_persist_probe.hip): s_memtime of workgroup 0 at the phase boundaries of its first 32 steps
#ifdef LRNDE_SDE_STAMPS
__device__ unsigned long long g_sde_stamps[32][16];
#define SDE_STAMP(i) do { if (PERSIST && blockIdx.x == 0 && threadIdx.x == 0 && it < 32) g_sde_stamps[it][(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SDE_STAMP(i) do { } while (0)
#endif
constexpr int SF_MAXD = 64, SF_MAXH = 128;

struct SdeFastArgs {
  const f32x4* W1p; int KG1;         // drift Dense-1 fragments [MT1p][KG1][64]
  const f32x4* W2p; int KG2p;        // drift Dense-2 fragments [MT2][KG2p][64]
  const f32x4* Wgp; int KGgp;        // diffusion (second layer of the identity+Dense form) [MT2][KGgp][64]
  const float *b1, *b2, *bg;         // zero-padded to the tile sizes
  int act, D;
  const float* u; const float* dW; float* un;   // (B, D)
  int B;
  float dt, abstol, reltol, delta;
  const float* dt_dev;   // non-NULL: the single step's dt is read from here (a dt an earlier launch on the stream computed)
  float* dW_scaled;      // non-NULL: `dW` holds standard-normal draws z; the step uses sqrt(dt) * z and leaves it here (k_sde_scale's expression)
  // sde_determine_initdt on this kernel's tiles (idt_phase 1 / 2, lrnde_sde_node.hpp: sde_init_dt_dev): per-workgroup fp64
  // sums of the norms into idt_part (phase 1: d0, d1) / idt_part2 (phase 2: d2); phase 2 leaves {dt0, d1} in idt_scal
  int idt_phase; double* idt_part; double* idt_part2; float* idt_scal; float idt_dtmax;
  // fixed-grid solve as ONE launch (lrnde_sde_solve_fixed): march_n > 0 — the workgroup takes its columns through march_n steps,
  // step i with the increments dW + i * B * D, end state to un + i * B * D, and leaves its partial sum of step i in
  // march_part[(i * gridDim.x + workgroup) * PSTRIDE]: no step waits for another workgroup (nothing consumes EEst inside
  // the solve; k_sde_march_records forms every step's record afterwards, in the partial-vector order)
  int march_n; double* march_part;
  int dbg_stall;   // test hook (LRNDE_SDE_PERSIST_STALL): the persistent form waits for one workgroup more than there are — its barrier times out
  double* part;      // per-workgroup fp64 sums of the squared residual (PSTRIDE doubles each)
  int* arrive;       // fixed-grid solve: arrival counter of the step's footer, or NULL
  Ctrl* rec;         //   ... and the record slot the last workgroup fills (EEst, EEst*dt)
  double n_norm;     // elements of the norm (B * D)
  // adaptive solves: the controller lives on the device.  The launch reads the control block (grid position i, step
  // length m in grid intervals, which of the two state buffers is current), forms dW from the caller's path itself, and
  // its last workgroup runs the PI controller and writes the block for the next launch.
  SdeCtl* ctl; const float* Wpath; float* ua; float* ub; int nfine; float t0, h;
  float gamma, qmin, qmax, beta1, beta2; int maxiters;
  lrnde_trace_row* trace; int cap_trace;
  unsigned long long* prog;  // pinned host word: sde_report_pack(launches whose footer ran, status)
  int jlaunch;
  // the layer's recorded forward: end state of accepted step k -> rec_u[k] (slot = accepted steps so far; a rejected
  // attempt's slot is rewritten by the retry), its (i, m) -> rec_im[k]
  float* rec_u; int2* rec_im; int rec_cap;
  // persistent form (k_sde_eh_fast<DT, HT, true>, cooperative launch): the base of the TWO blocks of {partial sum, tag} slots the
  // steps alternate between (zero at launch: no slot carries a step's tag yet)
  double* part2;
  // the four-stage SRI step (k_sde_sri_fast, lrnde_sde_sri_fast.hpp): the second Brownian path on W's grid and the caller's
  // tableau, by value (last: the other kernels' argument offsets are what they were)
  const float* Zpath; lrnde_sri_tableau tab;
  // the path source of the TREE instantiations (lrnde_sde_tree.hpp): W (and SRI's Z) by descent instead of Wpath / Zpath, the
  // accepted step's increments recorded beside rec_u.  Behind everything else: no other field moves
  SdeTree tree;
};
// canonical dot product over NKG k-groups of 16 rows: fma chains over segments of SEGK k-groups, partials left to right
template <int NKG>
__device__ __forceinline__ f32x4 sf_chain(const f32x4 (&frag)[NKG], const f32x4* xb, int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kg = 0; kg < (NKG < SEGK ? NKG : SEGK); ++kg) acc = mfma4(frag[kg], xb[kg * 64 + lane], acc);
  if constexpr (NKG > SEGK) {
    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kg = SEGK; kg < NKG; ++kg) acc2 = mfma4(frag[kg], xb[kg * 64 + lane], acc2);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + acc2[r];
  }
  return acc;
}

// The controller of lrnde_sde_solve_adaptive's host loop on a copy of the control block: PI step factor from EEst
// (lrnde_stepctl.hpp, the caller's constants), the proposal kept as a real number, position on the caller's grid, buffer
// flip.  `writer` (one thread of the whole grid) also leaves the trace row and the accepted step's (start, length).
// qpow = fastpow(c.qold, a.beta2): does not depend on this step's EEst — the cooperative form computes it while the partial
// sums are still in flight.
// nfa: drift evaluations of one attempted step (Euler-Heun 3, Milstein 1, SRI 4): what SdeCtl::nf counts.
// (The same controller as sde_grid_update, lrnde_stepctl.hpp — the host loop's, and what tests/test_host_gridctl.py holds to the
// numpy loop.  It stays written out here: with the trace row and the pair written by the caller of the shared function the
// step kernels' footers compiled to other code than before — more SGPR spills in the persistent tree kernels.  A change to
// either statement goes into both; tests/test_gpu_switches.py holds the two loops to the same bits.)
__device__ __forceinline__ void sde_ctl_update(SdeCtl& c, float eest, float dt, const SdeFastArgs& a, bool writer, float qpow, int nfa) {
  c.nf += nfa; c.eest_last = eest;
  if (eest != eest) { c.status = LRNDE_DT_NAN; return; }
  const float q = pi_step({a.gamma, a.qmin, a.qmax, a.beta1, a.beta2}, 0, eest, qpow, 1.0f).q;
  const int accepted = eest <= 1.0f;
  const int ntr = c.naccept + c.nreject;
  if (writer && a.trace && ntr < a.cap_trace) {
    lrnde_trace_row r; r.t = a.t0 + (float)c.i * a.h; r.dt = dt; r.eest = eest; r.accepted = accepted;
    a.trace[ntr] = r;
  }
  c.dtc = (accepted ? fmaxf_(c.dtc, dt) : dt) / q;
  int mnew = (int)(c.dtc / a.h);
  if (mnew < 1) mnew = 1;
  if (accepted) {
    if (a.rec_im) {
      if (c.naccept < a.rec_cap) { if (writer) a.rec_im[c.naccept] = make_int2(c.i, c.m); }
      else c.status = LRNDE_CAPACITY;
    }
    c.naccept++;
    c.qold = pi_qold(eest);
    c.i += c.m;
    c.cur ^= 1;
    c.m = mnew;
    if (c.i >= a.nfine && c.status == ST_RUNNING) c.status = ST_DONE;
  } else {
    c.nreject++;
    if (c.m == 1) c.status = LRNDE_DT_LESS_THAN_MIN;  // the path's grid cannot be refined further
    else c.m = mnew < c.m ? mnew : c.m - 1;
  }
  if (c.status == ST_RUNNING) {
    if (c.m > a.nfine - c.i) c.m = a.nfine - c.i;
    if (++c.iters > a.maxiters) c.status = LRNDE_MAXITERS;
  }
}

// ---- the workgroup frame of the one-launch step kernels (k_sde_eh_fast, k_sde_mil_fast, k_sde_sri_fast) ----
// Layout: a workgroup is four waves on 16 columns (b0 .. b0 + 15; lane = 16 rq + n holds rows 4 rq .. 4 rq + 3 of column n of a
// 16-row tile).  The three weight matrices are v_mfma_f32_16x16x4_f32 A fragments in registers for the whole launch: wave w
// holds the hidden tiles w, w + 4 of Dense-1 (w1), Dense-2 tile t = w for w < DT (w2: `has_d2`) and at most one diffusion tile
// tg (wg: job j = wave + 4 r is diffusion tile j - DT for j in [DT, 2 DT)); tiles past D / H are zero fragments.  The waves with
// a Dense-2 tile own the elementwise algebra of their rows row0 .. row0 + 3 (C-fragment registers); `live` lanes are those whose
// rows and column exist, g is the lane's offset into a (B, D) array and nn = B D one such array.  D % 4 != 0 takes the scalar
// accesses of ld4s / st4s (rows past D stay zero / unwritten).  The kernel declares the LDS tiles — x tiles in B-operand layout
// ([kg][64 lanes] float4), the h tile hl, the diffusion results gl in C-fragment order — and constructs the frame after them.
template <int DT, int HT>
struct SdeFrame {
  static_assert(DT >= 1 && DT <= 4 && HT >= 1 && HT <= 8, "D <= 64, H <= 128");
  static constexpr int NJ = (HT + 3) / 4;   // hidden tiles per wave
  typedef __attribute__((address_space(3))) f32x4 lds4;
  lds4 *hl, *gl;   // (as LDS pointers: carried as generic ones, the persistent step loop measured 1.2 % slower)
  int lane, wave, n, rq, t, tg, act, D, row0;
  bool has_d2, vec, live;
  size_t g, nn;
  f32x4 w1[NJ][DT], w2[HT], wg[DT], b1v[NJ], b2v, bgv;   // resident A fragments and this lane's bias rows

  __device__ __forceinline__ SdeFrame(const SdeFastArgs& a, f32x4* hl_, f32x4* gl_) : hl((lds4*)hl_), gl((lds4*)gl_), act(a.act), D(a.D) {
    lane = threadIdx.x & 63;
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    n = lane & 15; rq = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const bool colok = b0 + n < a.B;
    // jobs of this wave: Dense-2 tile t (wave < DT), diffusion tile tg (job wave or wave + 4 in [DT, 2 DT))
    has_d2 = wave < DT;
    t = has_d2 ? wave : 0;
    tg = (wave >= DT && wave < 2 * DT) ? wave - DT : ((wave + 4 >= DT && wave + 4 < 2 * DT) ? wave + 4 - DT : -1);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ht = wave + 4 * j;
#pragma unroll
      for (int kg = 0; kg < DT; ++kg) w1[j][kg] = ht < HT ? a.W1p[((size_t)ht * a.KG1 + kg) * 64 + lane] : zero4;
      b1v[j] = ht < HT ? *reinterpret_cast<const f32x4*>(a.b1 + ht * 16 + rq * 4) : zero4;
    }
#pragma unroll
    for (int kg = 0; kg < HT; ++kg) w2[kg] = has_d2 ? a.W2p[((size_t)t * a.KG2p + kg) * 64 + lane] : zero4;
#pragma unroll
    for (int kg = 0; kg < DT; ++kg) wg[kg] = tg >= 0 ? a.Wgp[((size_t)tg * a.KGgp + kg) * 64 + lane] : zero4;
    b2v = has_d2 ? *reinterpret_cast<const f32x4*>(a.b2 + t * 16 + rq * 4) : zero4;
    bgv = tg >= 0 ? *reinterpret_cast<const f32x4*>(a.bg + tg * 16 + rq * 4) : zero4;
    row0 = t * 16 + rq * 4;
    vec = (D & 3) == 0;                 // rows in whole quads: one 16-byte access per lane
    live = has_d2 && colok && row0 < D;
    g = (size_t)(b0 + n) * D + row0;
    nn = (size_t)a.B * D;
  }
  // this lane's four rows of column n of the (B, D) array p (live lanes only)
  __device__ __forceinline__ f32x4 ld4s(const float* p) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) v = *reinterpret_cast<const f32x4*>(p + g);
    else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (row0 + r < D) v[r] = p[g + r];
    }
    return v;
  }
  __device__ __forceinline__ void st4s(float* p, const f32x4& v) const {
    if (vec) *reinterpret_cast<f32x4*>(p + g) = v;
    else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (row0 + r < D) p[g + r] = v[r];
    }
  }
  // the increment P[i + m] - P[i] of a path on the caller's grid (the expression of k_sde_dw)
  __device__ __forceinline__ f32x4 dpath(const float* P, int i, int m) const {
    const f32x4 lo = ld4s(P + (size_t)i * nn);
    const f32x4 hi = ld4s(P + (size_t)(i + m) * nn);
    f32x4 d;
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = hi[r] - lo[r];
    return d;
  }
  // this lane's four rows of W[k] of the virtual tree (stream 6: W, 7: Z; lrnde_sde_tree.hpp) — rows past D zero, as ld4s leaves them
  __device__ __forceinline__ f32x4 wtree(const SdeTree& T, uint32_t stream, int k) const {
    const uint32_t c[4] = {(uint32_t)g, (uint32_t)g + 1u, (uint32_t)g + 2u, (uint32_t)g + 3u};   // column b D + d
    float w[4];
    tree_query<4>(T, stream, c, k, w);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = row0 + r < D ? w[r] : 0.f;
    return v;
  }
  // ... and the increment W[i + m] - W[i] from it: dpath's subtraction on the tree's two values
  __device__ __forceinline__ f32x4 dtree(const SdeTree& T, uint32_t stream, int i, int m) const {
    const f32x4 hi = wtree(T, stream, i + m);
    const f32x4 lo = wtree(T, stream, i);
    f32x4 d;
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = hi[r] - lo[r];
    return d;
  }
  // The descent spread over the WHOLE workgroup (the live lanes above are the Dense-2 waves only: DT of four): thread x takes
  // column x & 15 and the rows (x >> 4) + 16 j, j < DT, of the 16 DT x 16 tile — DT elements instead of four on DT / 4 of the
  // waves — and leaves W[k] in wt ([row][16 columns], LDS; zero outside B / D).  Every thread of the workgroup calls it; after
  // a barrier the Dense-2 lanes read their four rows with wtree_rd.  Same normals, same operations: the bits of wtree.
  __device__ __forceinline__ void wtree_fill(const SdeTree& T, uint32_t stream, int k, int B, float* wt) const {
    const int ne = threadIdx.x & 15, r0 = threadIdx.x >> 4;
    const int be = blockIdx.x * 16 + ne;
    uint32_t c[DT];
    float w[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) c[j] = (uint32_t)be * (uint32_t)D + (uint32_t)(r0 + 16 * j);   // (outside B / D: some other column's value, discarded)
    tree_query<DT>(T, stream, c, k, w);
#pragma unroll
    for (int j = 0; j < DT; ++j) wt[(r0 + 16 * j) * 16 + ne] = (be < B && r0 + 16 * j < D) ? w[j] : 0.f;
  }
  __device__ __forceinline__ f32x4 wtree_rd(const float* wt) const {   // (live lanes: row0 + 3 < 16 DT)
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = wt[(row0 + r) * 16 + n];
    return v;
  }
  // B-operand image of rows 16 t + 4 rq + r, column n: float4 index t*64 + r*16 + n, component rq (Dense-2 waves)
  __device__ __forceinline__ void put(f32x4* x, const f32x4& v) const {
    float* p = reinterpret_cast<float*>(x) + ((t * 64 + n) << 2) + rq;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r * 64] = v[r];
  }
  // drift Dense-1 + activation of this wave's hidden tiles on the x tile xs -> hl
  __device__ __forceinline__ void dense1(const f32x4* xs) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ht = wave + 4 * j;
      if (ht < HT) {
        const f32x4 acc = sf_chain<DT>(w1[j], xs, lane);
        __attribute__((address_space(3))) float* p = (__attribute__((address_space(3))) float*)hl + ((ht * 64 + n) << 2) + rq;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r * 64] = act_apply_sel(act, acc[r] + b1v[j][r]);   // (four independent elements: the select form interleaves them)
      }
    }
  }
  __device__ __forceinline__ void diffusion(const f32x4* xs) const {  // tile tg of g(xs) -> gl (C-fragment order)
    if (tg < 0) return;
    f32x4 acc = sf_chain<DT>(wg, xs, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + bgv[r];
    gl[tg * 64 + lane] = acc;
  }
  __device__ __forceinline__ f32x4 dense2() const {  // tile t of f = W2 h + b2 (Dense-2 waves)
    f32x4 acc = sf_chain<HT>(w2, (const f32x4*)hl, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + b2v[r];
    return acc;
  }
};

// this workgroup's sum of the waves' partial sums red[] (Dense-2 waves, in wave order)
template <int DT> __device__ __forceinline__ double sde_wg_total(const double* red) {
  double tot = red[0];
#pragma unroll
  for (int w = 1; w < DT; ++w) tot += red[w];
  return tot;
}

// The footer of a launch that is one step (every thread calls it, after the barrier behind the red[] stores): the workgroup's
// total goes to its partial slot; the last workgroup to arrive adds the partials in partial-vector order and either fills the
// fixed-grid record (`adapt` false: EEst, EEst * dt) or runs the controller on the control block with nfa drift evaluations
// per attempt (trace row, the layer's (start, length) record) and reports through the pinned progress word.
template <int DT> __device__ __forceinline__ void sde_step_footer(const SdeFastArgs& a, const double* red, float dt, bool adapt, int nfa) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const double tot = sde_wg_total<DT>(red);
  int last = 0;
  if (lane == 0) {
    double* p = a.part + (size_t)blockIdx.x * PSTRIDE;
    __hip_atomic_store(p + 0, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + 1, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + 2, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = __hip_atomic_fetch_add(a.arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  }
  last = __shfl(last, 0, 64);
  if (!last) return;
  const Sum3 s = reduce_partials3(a.part, (int)gridDim.x);
  if (lane == 0) {
    const float eest = rms_from(s.a, a.n_norm);
    if (!adapt) {
      a.rec->eest_last = eest;
      a.rec->reg_error = eest * dt;
      a.rec->status = ST_DONE;
    } else {
      SdeCtl c = *a.ctl;
      sde_ctl_update(c, eest, dt, a, true, fastpow(c.qold, a.beta2), nfa);
      *a.ctl = c;
      __hip_atomic_store(a.prog, sde_report_pack((unsigned)(a.jlaunch + 1), (unsigned)c.status),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(a.arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// PERSIST: the whole adaptive solve in ONE cooperative launch.  The workgroups stay resident with their weight fragments and
// their columns' state in registers; a step ends in a grid barrier (tagged partial-sum slots + bounded polling) after which EVERY
// workgroup adds the partial sums in the same fixed order and runs the same controller on its own copy of the control
// block — the same decisions everywhere, no broadcast, and the arithmetic of a step is the code of the one-launch form.
// TREE: the adaptive solve's increments come from the virtual tree instead of a.Wpath, the descent spread over all four waves
// (F.wtree_fill -> 1 KB of LDS per 16 rows -> F.wtree_rd behind the step's first barrier).  W[i] is carried in registers: an
// accepted step's W[i + m] is the next step's W[i], a rejected step keeps it — one descent per attempt in the persistent form.
template <int DT, int HT, bool PERSIST = false, bool TREE = false>
__global__ __launch_bounds__(SF_NT) void k_sde_eh_fast(SdeFastArgs a) {
  const bool adapt = a.ctl != nullptr;
  int ad_i = 0, ad_m = 0, ad_slot = 0;
  SdeCtl cc{};
  if (adapt) {
    cc = *a.ctl;   // written by the previous launch's last workgroup (kernel boundary in between) / by k_sde_ctl_init
    if (cc.status != ST_RUNNING) return;
    ad_i = cc.i; ad_m = cc.m; ad_slot = cc.naccept;
    a.dt = (float)ad_m * a.h;
    a.u = cc.cur ? a.ub : a.ua;
    a.un = cc.cur ? a.ua : a.ub;
  } else if (a.dt_dev) a.dt = *a.dt_dev;
  __shared__ SdeCtl sh_cc;
  // LDS: three x tiles in B-operand layout (16 DT rows x 16 columns each: [kg][64 lanes] float4), the h tile, the
  // diffusion results in C-fragment order, the reduction scratch
  __shared__ f32x4 xA[DT * 64], xB[DT * 64], xC[DT * 64], hl[HT * 64], gl[DT * 64];
  __shared__ double red[4];
  const SdeFrame<DT, HT> F(a, hl, gl);
  const int lane = F.lane, wave = F.wave, t = F.t, row0 = F.row0, D = F.D;
  const bool has_d2 = F.has_d2, live = F.live;
  const size_t nn = F.nn;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 u4 = zero4, w4 = zero4;
  [[maybe_unused]] f32x4 wlo4 = zero4, whi4 = zero4;
  if (live) u4 = F.ld4s(a.u);
  [[maybe_unused]] float* wt = nullptr;   // TREE: W[k] of the workgroup's 16 DT x 16 tile
  if constexpr (TREE) {
    __shared__ float wt_[DT * 256];
    wt = wt_;
    if (adapt) {   // W[i] at the launch's position (zero without a descent at i = 0)
      F.wtree_fill(a.tree, TREE_STREAM_W, ad_i, a.B, wt);
      __syncthreads();
      if (live) wlo4 = F.wtree_rd(wt);
      __syncthreads();   // (wt is refilled below)
    }
  }
  for (int it = 0;; ++it) {   // (one trip unless PERSIST)
  SDE_STAMP(0);
  if constexpr (TREE) { if (adapt) F.wtree_fill(a.tree, TREE_STREAM_W, ad_i + ad_m, a.B, wt); }   // (every thread; read behind the barrier below)
  if (live) {
    if (adapt) {  // dW = W[i + m] - W[i], the path's own increment (the expression of k_sde_dw)
      if constexpr (!TREE) w4 = F.dpath(a.Wpath, ad_i, ad_m);
    } else {
      w4 = F.ld4s(a.dW);
      if (a.dW_scaled) {
        const float cz = __builtin_sqrtf(a.dt);
#pragma unroll
        for (int r = 0; r < 4; ++r) w4[r] = cz * w4[r];
        F.st4s(a.dW_scaled, w4);
      }
    }
  }
  if (has_d2) F.put(xA, u4);
  __syncthreads();
  if constexpr (TREE) {
    if (adapt && live) {   // (wt is next written at the top of the next step, barriers away)
      whi4 = F.wtree_rd(wt);
#pragma unroll
      for (int r = 0; r < 4; ++r) w4[r] = whi4[r] - wlo4[r];
    }
  }
  const float dt = a.dt, hdt = dt / 2.0f, sqdt = __builtin_sqrtf(dt);

  if constexpr (!PERSIST) {
    if (a.idt_phase) {
      // StochasticDiffEq.sde_determine_initdt's evaluations and norms (UPSTREAM-RECALL; the expressions of k_sde_initdt):
      // phase 1: f0 = f(u), g0 = g(u) -> sums of (u / sk)^2 and (max(|f0 + 3 g0|, |f0 - 3 g0|) / sk)^2;
      // phase 2: dt0 from phase 1's sums (every workgroup adds them in the same fixed order), u1 = u + dt0 f0, f1, g1 ->
      //          sum of (max(|df + dg|, |df - dg|) / sk)^2.  The launch ends here.
      __shared__ double red2[4];
      __shared__ float sh_dt0;
      F.dense1(xA);
      F.diffusion(xA);
      __syncthreads();
      f32x4 f0 = zero4, g0 = zero4;
      if (has_d2) { f0 = F.dense2(); g0 = gl[t * 64 + lane]; }
      double a0 = 0.0, a1 = 0.0;
      if (a.idt_phase == 1) {
        if (live) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (row0 + r >= D) continue;
            const float sk = a.abstol + __builtin_fabsf(u4[r]) * a.reltol;
            const float G0 = 3.0f * g0[r];
            const float r0 = u4[r] / sk;
            const float r1 = fmaxf_(__builtin_fabsf(f0[r] + G0), __builtin_fabsf(f0[r] - G0)) / sk;
            a0 += (double)(r0 * r0); a1 += (double)(r1 * r1);
          }
        }
      } else {
        if (threadIdx.x < 64) {
          const Sum3 s = reduce_partials3(a.idt_part, (int)gridDim.x);
          if (lane == 0) {
            const float d0 = (float)sqrt(s.a / a.n_norm), d1 = (float)sqrt(s.b / a.n_norm);
            const float dt0 = initdt_dt0(d0, d1, a.idt_dtmax);
            sh_dt0 = dt0;
            if (blockIdx.x == 0) { a.idt_scal[0] = dt0; a.idt_scal[1] = d1; }
          }
        }
        __syncthreads();
        const float dt0 = sh_dt0;
        if (has_d2) {
          f32x4 u1;
#pragma unroll
          for (int r = 0; r < 4; ++r) u1[r] = u4[r] + dt0 * f0[r];
          F.put(xB, u1);
        }
        __syncthreads();
        F.dense1(xB);
        F.diffusion(xB);
        __syncthreads();
        if (has_d2) {
          const f32x4 f1 = F.dense2();
          const f32x4 g1 = gl[t * 64 + lane];
          if (live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (row0 + r >= D) continue;
              const float sk = a.abstol + __builtin_fabsf(u4[r]) * a.reltol;
              const float G0 = 3.0f * g0[r], G1 = 3.0f * g1[r];
              const float dg = fmaxf_(__builtin_fabsf(G0 - G1), __builtin_fabsf(G0 + G1));
              const float df = f1[r] - f0[r];
              const float r2 = fmaxf_(__builtin_fabsf(df + dg), __builtin_fabsf(df - dg)) / sk;
              a0 += (double)(r2 * r2);
            }
          }
        }
      }
      if (has_d2) {
        a0 = wave_sum_dpp(a0); a1 = wave_sum_dpp(a1);
        if (lane == 0) { red[wave] = a0; red2[wave] = a1; }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        double t0s = red[0], t1s = red2[0];
#pragma unroll
        for (int w = 1; w < DT; ++w) { t0s += red[w]; t1s += red2[w]; }
        double* pp = (a.idt_phase == 1 ? a.idt_part : a.idt_part2) + (size_t)blockIdx.x * PSTRIDE;
        pp[0] = t0s; pp[1] = t1s; pp[2] = 0.0;
      }
      return;
    }
  }
  SDE_STAMP(1);
  // ---- round 1: du1 = f(u), L = g(u) (:174-176) ----
  F.dense1(xA);
  SDE_STAMP(8);
  F.diffusion(xA);
  SDE_STAMP(9);
  __syncthreads();
  SDE_STAMP(10);
  f32x4 du1 = zero4, L = zero4, Kv = zero4;
  if (has_d2) {
    du1 = F.dense2();
    SDE_STAMP(11);
    L = gl[t * 64 + lane];
    f32x4 tmp, ut;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Kv[r] = u4[r] + dt * du1[r];          // :175
      tmp[r] = Kv[r] + L[r] * w4[r];        // :179,183
      ut[r] = u4[r] + L[r] * sqdt;          // :196
    }
    F.put(xB, tmp); F.put(xC, ut);
  }
  SDE_STAMP(12);
  __syncthreads();
  SDE_STAMP(2);
  // ---- round 2: g(tmp), f(tmp) at t + dt (:184, :191) ----
  F.dense1(xB);
  F.diffusion(xB);
  __syncthreads();
  f32x4 un = zero4;
  if (has_d2) {
    const f32x4 f2 = F.dense2();
    const f32x4 g2 = gl[t * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gtmp2 = 0.5f * (L[r] + g2[r]);
      const float noise2 = gtmp2 * w4[r];
      un[r] = (u4[r] + hdt * (du1[r] + f2[r])) + noise2;   // :191
    }
    if (live) {
      if (!PERSIST) F.st4s(a.un, un);   // (PERSIST: the state lives in registers until the solve ends)
      if (a.rec_u && ad_slot < a.rec_cap) F.st4s(a.rec_u + (size_t)ad_slot * nn, un);
      if constexpr (TREE) { if (a.tree.rec_dw && ad_slot < a.rec_cap) F.st4s(a.tree.rec_dw + (size_t)ad_slot * nn, w4); }
    }
    F.put(xA, Kv);   // xA is free: every wave has read it (barrier above)
  }
  __syncthreads();
  SDE_STAMP(3);
  // ---- round 3: du2 = f(K, t + dt) (:193), g(utilde, t) (:197) ----
  F.dense1(xA);
  F.diffusion(xC);
  __syncthreads();
  double acc = 0.0;
  if (has_d2) {
    const f32x4 du2 = F.dense2();
    const f32x4 g3 = gl[t * 64 + lane];
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (row0 + r >= D) continue;
        const float Ed = (dt * (du2[r] - du1[r])) / 2.0f;                        // :194
        const float ggp = (g3[r] - L[r]) / sqdt;                                 // :197
        const float En = (ggp * (w4[r] * w4[r])) / 2.0f;                         // :198
        const float sc = a.abstol + fmaxf_(__builtin_fabsf(u4[r]), __builtin_fabsf(un[r])) * a.reltol;
        const float rr = (a.delta * Ed + En) / sc;                               // :214-216
        const float sq = rr * rr;
        acc += (double)sq;
      }
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) red[wave] = acc;
  }
  __syncthreads();
  SDE_STAMP(4);
  if constexpr (PERSIST) {
    const int nwg = (int)gridDim.x + a.dbg_stall;
    double* blk = a.part2 + (size_t)(it & 1) * nwg * PSTRIDE;   // (two blocks: a fast workgroup's next step must not overwrite what a slow one still reads)
    if (threadIdx.x < 64) {
      // The step's grid barrier IS the exchange of the partial sums: a workgroup publishes {sum, tag} as ONE 16-byte agent-scope
      // store — tag = step number and a checksum of the sum's bits, so that a reader can tell a slot of this step from a stale
      // or (should a 16-byte access ever be split) a torn one — and every workgroup polls all slots with 16-byte loads until
      // each carries this step's tag.  Two trips past the L2 per step (publish, poll) instead of four (store, arrive, poll,
      // read).  Bounded: 50 ms on the 100-MHz clock, then the solve ends with an error instead of hanging the queue.
      typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
      const unsigned step_tag = (unsigned)(it + 1);
      if (lane == 0) {
        const unsigned long long vb = __builtin_bit_cast(unsigned long long, sde_wg_total<DT>(red));
        const u32x4_ w = {(unsigned)vb, (unsigned)(vb >> 32), (unsigned)(vb >> 32) ^ (unsigned)vb, step_tag};
        double* p = blk + (size_t)blockIdx.x * PSTRIDE;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(w) : "memory");
      }
      float qpow = fastpow(cc.qold, a.beta2);   // (ahead of the wait: see sde_ctl_update)
      asm volatile("" : "+v"(qpow));              // (pinned here: the value is only used after the polling loop)
      PartLoads L;
      const unsigned long long t0c = __builtin_amdgcn_s_memrealtime();
      bool ok = true;
      for (;;) {
        u32x4_ v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = lane + 64 * u;
          const double* p = blk + (size_t)(i < nwg ? i : 0) * PSTRIDE;
          asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v[u]) : "v"(p) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool good = true;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          asm volatile("" : "+v"(v[u]));
          const bool mine = lane + 64 * u < nwg;
          good = good && (!mine || (v[u].w == step_tag && v[u].z == (v[u].x ^ v[u].y)));
          L.va[u] = __builtin_bit_cast(double, (unsigned long long)v[u].x | ((unsigned long long)v[u].y << 32));
        }
        if (__ballot(good) == ~0ull) break;
        if (__builtin_amdgcn_s_memrealtime() - t0c > 5000000ull) { ok = false; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      SDE_STAMP(5);
      SdeCtl c2 = cc;
      if (!ok) c2.status = LRNDE_HIP_ERROR;
      else {
        const Sum3 s3 = part_finish<false>(L, blk, nwg);   // (the fixed order of every reduction of these partials)
        const float eest = rms_from(s3.a, a.n_norm);
        sde_ctl_update(c2, eest, dt, a, blockIdx.x == 0 && lane == 0, qpow, 3);
      }
      if (lane == 0) sh_cc = c2;
    }
    __syncthreads();
    SDE_STAMP(6);
    const int nacc0 = cc.naccept;
    cc = sh_cc;
    if constexpr (TREE) { if (cc.naccept != nacc0) wlo4 = whi4; }
    if (cc.naccept != nacc0) u4 = un;   // accepted: the end state is the next step's start state (rows of the Dense-2 waves)
    if (cc.status != ST_RUNNING) {
      if (live) F.st4s(cc.cur ? a.ub : a.ua, u4);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.ctl = cc;
        __hip_atomic_store(a.prog, sde_report_pack((unsigned)(it + 1), (unsigned)cc.status),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      return;
    }
    ad_i = cc.i; ad_m = cc.m; ad_slot = cc.naccept;
    a.dt = (float)ad_m * a.h;
    continue;
  } else {
  if (a.march_n > 0) {
    if (threadIdx.x == 0) {
      double* p = a.march_part + ((size_t)it * gridDim.x + blockIdx.x) * PSTRIDE;
      p[0] = sde_wg_total<DT>(red); p[1] = 0.0; p[2] = 0.0;
    }
    if (it + 1 == a.march_n) return;
    u4 = un;                       // the end state is the next step's start state (rows of the Dense-2 waves)
    a.dW += nn; a.un += nn;
    __syncthreads();               // red and the tiles are rewritten by the next step
    continue;
  }
  if (!a.arrive) {   // (a single step whose caller reduces the partials)
    if (threadIdx.x == 0) { double* p = a.part + (size_t)blockIdx.x * PSTRIDE; p[0] = sde_wg_total<DT>(red); p[1] = 0.0; p[2] = 0.0; }
    return;
  }
  sde_step_footer<DT>(a, red, dt, adapt, 3);   // fills the fixed-grid record / runs the controller
  return;
  }
  }   // for (it)
}

// the gate of the one-launch kernels
inline bool sde_fast_shape(int D, int H) { return D >= 1 && D <= SF_MAXD && H >= 1 && H <= SF_MAXH; }
// launch by shape: fn(integral_constant DT, integral_constant HT) with DT = ceil(D / 16) in 1..4, HT = ceil(H / 16) in 1..8;
// false, and nothing called, for a shape outside sde_fast_shape (every caller checks the gate first)
template <class F, int... I> inline bool sde_fast_dispatch_(int k, F& fn, std::integer_sequence<int, I...>) {
  return ((k == I && (fn(std::integral_constant<int, I / 8 + 1>{}, std::integral_constant<int, I % 8 + 1>{}), true)) || ...);
}
template <class F> inline bool sde_fast_dispatch(int D, int H, F fn) {
  if (!sde_fast_shape(D, H)) return false;
  return sde_fast_dispatch_(((D + 15) / 16 - 1) * 8 + (H + 15) / 16 - 1, fn, std::make_integer_sequence<int, 32>{});
}
inline void sde_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    if (f.tree.on) hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, false, true>), dim3(nwg), dim3(SF_NT), 0, st, f);
    else hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value>), dim3(nwg), dim3(SF_NT), 0, st, f);
  });
}

// the persistent form.  coop: a cooperative launch (all workgroups resident, or the call fails and the caller takes the
// launch-per-step loop) — the API's guarantee costs 25-30 us per launch; !coop: a plain launch, for grids far smaller than the
// chip, whose barrier is bounded (a workgroup that waits 50 ms for the others ends the solve with an error and the caller runs
// the loop instead).  Returns the launch's hipError_t.
inline hipError_t sde_persist_launch(int D, int H, int nwg, hipStream_t st, SdeFastArgs& f, bool coop) {
  hipError_t e = hipErrorInvalidValue;   // (a shape outside the gate: nothing is launched)
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    void* args[] = {&f};
    if (f.tree.on) {
      if (!coop) { hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, true, true>), dim3(nwg), dim3(SF_NT), 0, st, f); e = hipGetLastError(); }
      else e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_sde_eh_fast<dt.value, ht.value, true, true>), dim3(nwg), dim3(SF_NT), args, 0, st);
    } else
    if (!coop) { hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), 0, st, f); e = hipGetLastError(); }
    else e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_sde_eh_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), args, 0, st);
  });
  return e;
}

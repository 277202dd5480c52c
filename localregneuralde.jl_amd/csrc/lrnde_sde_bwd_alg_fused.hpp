// lrnde_sde_bwd_alg_fused.hpp — the reverse sweep of a NeuralDSDE record made with the Milstein step (src/perform_step.jl:
// 108-170) or the four-stage SRI step (:49-106) as ONE launch, and the regulariser's local step of either kind as one more.
// Included by lrnde_kernels.hip after lrnde_sde_bwd_fused.hpp, whose general LDS form (SbfDev) these kernels are built on:
// a workgroup of 256 threads carries SBF_NS = 4 samples, one wave each, through all K recorded steps, newest first; the three
// weight matrices sit in LDS with odd leading dimensions; every product is SbfDev::mv — a plain fp32 fma chain over the input
// index in increasing order; the workgroup's parameter cotangent accumulates in LDS, each entry owned by one thread; each
// workgroup leaves one partial vector and k_sde_bwd_reduce adds them in workgroup order.  No float atomics, no grid barrier,
// no spin: the result does not depend on scheduling.
//
// What the per-step route (sde_node_backward_alg, lrnde_sde_node.hpp) enqueues per recorded step — for SRI the whole forward
// step again, three stage kernels, the seeds, four rounds of two VJPs + join + two accumulations, a copy and a host wait —
// is here a few hundred fma per lane.  The forward values are RECOMPUTED in the plain-chain order (the forward kernels'
// canonical MFMA chains differ in the last bits), exactly as the Euler-Heun sweep does; nothing but x, rec_u, the (i, m)
// pairs, the path(s) and the parameters is read.
//
// Milstein (the tape of k_sde_rkmil / k_sde_mil_fast; the dead du2 / En are not evaluated): one drift point and two
// diffusion points per step — evaluation point 1 = uprev (f and g), 0 = tmp (g only: its drift vectors stay zero).
//   K = u + dt f(u), L = g(u), tmp = K + sqrt(dt) L, u' = (K + L dW) + ((g(tmp) - L) / sqrt(dt)) (dW^2 / 2 - dt / 2)
// reversed by the expressions of k_mil_seed / k_mil_mid / k_sdeb_end.
// SRI: four drift points (uprev, H0_1..3) and four diffusion points (uprev, H1_1..3): evaluation point st holds H0_st as the
// drift's input and H1_st as the diffusion's (the own_xg layout of sbf_off).  chi1..3 by k_sri_chi's expressions, the stages
// by k_sri_stage's, the seeds by k_sri_bseed's, the joins by k_sri_bjoin's, the tableau passed by value.
//
// The regulariser's local step, d(EEst*dt)/dp at (u1, t1) with uprev, dW (SRI: dZ), dt constant: the same step function
// entered with the residual's seed instead of a state cotangent.  EEst and u' are the forward's record (the norm is the one
// thing that couples the batch; u' decides which side of max(|uprev|, |u'|) carries the scale — a tie stays with uprev, as
// fmaxf_ has it); there is no dx.  The partials are scaled by w_reg and ADDED by k_sde_bwd_reduce(..., add = 1).

namespace {

struct SdeAlgBwdArgs {
  SdeBwdFusedArgs a;        // (a.W: the path W; a.u1 / a.dW1 / a.un1 / a.dt1 / a.eest / tolerances: the local step's record)
  const float* Z;           // SRI: the second path
  const float* dZ1;         // SRI: the local step's second increment
  lrnde_sri_tableau T;      // SRI: the record's tableau
};

// evaluation points per sample and whether the diffusion's input has its own vector: Milstein 2 / no, SRI 4 / yes
__host__ __device__ constexpr int sba_nev(int kind) { return kind == 2 ? 4 : 2; }
__host__ __device__ constexpr bool sba_own_xg(int kind) { return kind == 2; }
inline size_t sba_smem_bytes(int D, int H, int kind) { return sbf_smem_bytes_xg(D, H, sba_nev(kind), sba_own_xg(kind)); }

// the residual's seed on u' and on the numerator: rb = d reg / d r with reg = dt sqrt(mean r^2), r = num / sc,
// sc = abstol + max(|up|, |un|) reltol.  Returns d reg / d num; unb gets the scale's term when u' carries the maximum.
__device__ __forceinline__ float sba_resid_seed(const SdeBwdFusedArgs& a, float up, float un, float num, float dt, float& unb) {
  if (!(a.eest > 0.f)) return 0.f;
  const float nf = (float)((size_t)a.B * a.D);
  const float sc = a.abstol + fmaxf_(__builtin_fabsf(up), __builtin_fabsf(un)) * a.reltol;
  const float r = num / sc;
  const float rb = dt * r / (nf * a.eest);
  const float scb = (-rb * num / (sc * sc)) * a.reltol;
  if (__builtin_fabsf(un) > __builtin_fabsf(up)) unb += scb * (un >= 0.f ? 1.f : -1.f);   // (else: uprev's side — a constant here)
  return rb / sc;
}

// One Milstein step backwards for this wave's sample.  ub: cotangent of u' (REG: none — the residual's seed takes its place,
// un = the recorded u').  Returns the cotangent of u.  Leaves the step's vectors in the two blocks for SbfDev::accumulate.
template <bool REG>
__device__ __forceinline__ float sba_mil_step(const SbfDev& c, const SdeBwdFusedArgs& a, bool live, float u, float dW, float dt, float ub, float un) {
  const SbfOff o = c.o;
  const int lane = c.lane;
  float* V0 = c.block(0);   // evaluation point tmp (diffusion only)
  float* V1 = c.block(1);   // evaluation point u
  const float sqdt = __builtin_sqrtf(dt), hdt = dt / 2.0f;
  // ---- forward pieces (:130-137): du1 = f(u), L = g(u), tmp = (u + dt du1) + sqdt L ----
  if (live) V1[o.X + lane] = u;
  float a1a, a1b;
  c.hidden(V1, a1a, a1b);
  const float du1 = c.f_out(V1);
  const float L = c.g_out(V1 + o.X);
  const float tmp = live ? (u + dt * du1) + sqdt * L : 0.f;
  if constexpr (REG) {   // (k_mil_reg_seed: r = (u' - u) / sc)
    ub = 0.f;
    if (live) { const float numb = sba_resid_seed(a, u, un, un - u, dt, ub); ub += numb; }
  }
  // ---- the seeds (k_mil_seed): cotangent of g(tmp), the direct part of L's ----
  const float J = (0.5f * dW) * dW - hdt;
  const float gb = (ub * J) / sqdt;
  const float Lb0 = ub * dW - gb;
  if (live) { V0[o.X + lane] = tmp; V0[o.LAMG + lane] = gb; }
  const float tb = c.wgt_x(V0 + o.LAMG);          // cotangent of tmp
  // ---- k_mil_mid ----
  const float kb = ub + tb;
  const float du1b = dt * kb;
  const float Lb = Lb0 + sqdt * tb;
  if (live) { V1[o.LAM + lane] = du1b; V1[o.LAMG + lane] = Lb; }
  const float duf = c.drift_vjp(V1, a1a, a1b);
  const float dug = c.wgt_x(V1 + o.LAMG);
  return live ? (kb + duf) + dug : 0.f;           // k_sdeb_end
}

// One four-stage SRI step backwards for this wave's sample (w = dW, z = dZ).  Same contract as sba_mil_step.
template <bool REG>
__device__ __forceinline__ float sba_sri_step(const SbfDev& c, const SdeBwdFusedArgs& a, const lrnde_sri_tableau& T, bool live, float up, float w,
                                              float z, float dt, float ub, float un) {
  const SbfOff o = c.o;
  const int lane = c.lane;
  float* V0 = c.block(0); float* V1 = c.block(1); float* V2 = c.block(2); float* V3 = c.block(3);
  const float sqdt = __builtin_sqrtf(__builtin_fabsf(dt));
  // chi1..3 (:57-59, k_sri_chi)
  const float sqrt3 = __builtin_sqrtf(3.0f), two_sqdt = 2.0f * sqdt, six_dt = 6.0f * dt, adt = __builtin_fabsf(dt);
  const float chi1 = (w * w - adt) / two_sqdt;
  const float chi2 = (w + z / sqrt3) / 2.0f;
  const float chi3 = ((w * w) * w - (3.0f * w) * dt) / six_dt;
  // ---- forward: the four evaluation points (k_sri_stage) ----
  float aa0, ab0, aa1, ab1, aa2, ab2, aa3, ab3;
  if (live) { V0[o.X + lane] = up; V0[o.XG + lane] = up; }
  c.hidden(V0, aa0, ab0);
  const float k1 = c.f_out(V0);
  const float g1 = c.g_out(V0 + o.XG);
  {
    const float da = dt * T.a021, db = dt * T.a121, sb = sqdt * T.b121;
    const float h0 = (up + da * k1) + (T.b021 * chi2) * g1;
    const float h1 = (up + db * k1) + sb * g1;
    if (live) { V1[o.X + lane] = h0; V1[o.XG + lane] = h1; }
  }
  c.hidden(V1, aa1, ab1);
  const float k2 = c.f_out(V1);
  const float g2 = c.g_out(V1 + o.XG);
  {
    const float h0 = (up + dt * (T.a031 * k1 + T.a032 * k2)) + chi2 * (T.b031 * g1 + T.b032 * g2);
    const float h1 = (up + dt * (T.a131 * k1 + T.a132 * k2)) + sqdt * (T.b131 * g1 + T.b132 * g2);
    if (live) { V2[o.X + lane] = h0; V2[o.XG + lane] = h1; }
  }
  c.hidden(V2, aa2, ab2);
  const float k3 = c.f_out(V2);
  const float g3 = c.g_out(V2 + o.XG);
  {
    const float h0 = (up + dt * ((T.a041 * k1 + T.a042 * k2) + T.a043 * k3)) + chi2 * ((T.b041 * g1 + T.b042 * g2) + T.b043 * g3);
    const float h1 = (up + dt * ((T.a141 * k1 + T.a142 * k2) + T.a143 * k3)) + sqdt * ((T.b141 * g1 + T.b142 * g2) + T.b143 * g3);
    if (live) { V3[o.X + lane] = h0; V3[o.XG + lane] = h1; }
  }
  c.hidden(V3, aa3, ab3);   // (k4, g4 themselves enter the residual only)
  // ---- seeds (k_sri_bseed): cotangents of k1..k4, g1..g4 and the direct part of uprev's ----
  float unb = ub, numb = 0.f;
  if constexpr (REG) {
    const float k4 = c.f_out(V3);
    const float g4 = c.g_out(V3 + o.XG);
    unb = 0.f;
    if (live) {
      const float s3 = ((T.beta31 * g1 + T.beta32 * g2) + T.beta33 * g3) + T.beta34 * g4;
      const float s4 = ((T.beta41 * g1 + T.beta42 * g2) + T.beta43 * g3) + T.beta44 * g4;
      const float E2 = chi2 * s3 + chi3 * s4;
      const float E1 = dt * (((k1 + k2) + k3) + k4);
      numb = sba_resid_seed(a, up, un, a.delta * E1 + E2, dt, unb);
    }
  }
  const float e1b = a.delta * numb;            // cotangent of E1
  const float e2b = unb + numb;                // cotangent of E2 (u' contains E2)
  const float kc = dt * unb, ke = dt * e1b;
  float kb0 = T.alpha1 * kc + ke, kb1 = T.alpha2 * kc + ke, kb2 = T.alpha3 * kc + ke, kb3 = T.alpha4 * kc + ke;
  const float w1 = unb * w, w2 = unb * chi1, w3 = e2b * chi2, w4 = e2b * chi3;
  float gb0 = ((T.beta11 * w1 + T.beta21 * w2) + T.beta31 * w3) + T.beta41 * w4;
  float gb1 = ((T.beta12 * w1 + T.beta22 * w2) + T.beta32 * w3) + T.beta42 * w4;
  float gb2 = ((T.beta13 * w1 + T.beta23 * w2) + T.beta33 * w3) + T.beta43 * w4;
  float gb3 = ((T.beta14 * w1 + T.beta24 * w2) + T.beta34 * w3) + T.beta44 * w4;
  float upb = unb;
  // ---- the stages backwards (k_sri_bjoin): x / y = cotangents of H0_st / H1_st ----
  {
    if (live) { V3[o.LAM + lane] = kb3; V3[o.LAMG + lane] = gb3; }
    const float x = c.drift_vjp(V3, aa3, ab3), y = c.wgt_x(V3 + o.LAMG);
    upb = (upb + x) + y;
    const float dx = dt * x, dy = dt * y, cx = chi2 * x, sy = sqdt * y;
    kb0 += T.a041 * dx + T.a141 * dy; gb0 += T.b041 * cx + T.b141 * sy;
    kb1 += T.a042 * dx + T.a142 * dy; gb1 += T.b042 * cx + T.b142 * sy;
    kb2 += T.a043 * dx + T.a143 * dy; gb2 += T.b043 * cx + T.b143 * sy;
  }
  {
    if (live) { V2[o.LAM + lane] = kb2; V2[o.LAMG + lane] = gb2; }
    const float x = c.drift_vjp(V2, aa2, ab2), y = c.wgt_x(V2 + o.LAMG);
    upb = (upb + x) + y;
    const float dx = dt * x, dy = dt * y, cx = chi2 * x, sy = sqdt * y;
    kb0 += T.a031 * dx + T.a131 * dy; gb0 += T.b031 * cx + T.b131 * sy;
    kb1 += T.a032 * dx + T.a132 * dy; gb1 += T.b032 * cx + T.b132 * sy;
  }
  {
    if (live) { V1[o.LAM + lane] = kb1; V1[o.LAMG + lane] = gb1; }
    const float x = c.drift_vjp(V1, aa1, ab1), y = c.wgt_x(V1 + o.LAMG);
    upb = (upb + x) + y;
    const float dx = dt * x, dy = dt * y, cx = chi2 * x, sy = sqdt * y;
    kb0 += T.a021 * dx + T.a121 * dy; gb0 += T.b021 * cx + T.b121 * sy;
  }
  {
    if (live) { V0[o.LAM + lane] = kb0; V0[o.LAMG + lane] = gb0; }
    const float x = c.drift_vjp(V0, aa0, ab0), y = c.wgt_x(V0 + o.LAMG);
    upb = (upb + x) + y;
  }
  return live ? upb : 0.f;
}

// The sweep.  KIND: 1 Milstein, 2 SRI.  DIRECT: a.W / q.Z hold the INCREMENTS of the recorded steps, step k's in slot k (a record
// made on the virtual path tree: lrnde_sde_node.hpp) — no path is read, (i, m) still gives dt.
template <int KIND, bool DIRECT = false>
__global__ __launch_bounds__(SBF_NT) void k_sde_alg_bwd_fused(SdeAlgBwdArgs q) {
  static_assert(KIND == 1 || KIND == 2, "1 Milstein, 2 SRI");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ int sk[SBF_MAXSER];
  __shared__ float sth[SBF_MAXSER];
  const SdeBwdFusedArgs& a = q.a;
  SbfDev c;
  c.setup(a, sm, sba_nev(KIND), sba_own_xg(KIND));
  for (int e = c.tid; e < a.nseries; e += SBF_NT) { sk[e] = a.ser_k[e]; sth[e] = a.ser_theta[e]; }
  __syncthreads();
  c.ones();
  const bool live = c.valid && c.row;
  const size_t nst = c.nst, g = c.g;
  float ub = 0.f;   // cotangent of the state at the end of the step being undone (row `lane` of this wave's sample)
  // the step's data: start state, the path values at its two ends, its length; the next (older) step's are requested while
  // this one is worked on
  auto step_src = [&](int k, float& u, float& wlo, float& whi, float& zlo, float& zhi, int& m) {
    const int2 im = a.im[k];
    const float* up = (k == 0) ? a.x : a.rec_u + (size_t)(k - 1) * nst;
    u = up[g]; m = im.y;
    if constexpr (DIRECT) {
      wlo = 0.f; whi = a.W[(size_t)k * nst + g];
      if constexpr (KIND == 2) { zlo = 0.f; zhi = q.Z[(size_t)k * nst + g]; }
    } else {
    wlo = a.W[(size_t)im.x * nst + g]; whi = a.W[(size_t)(im.x + im.y) * nst + g];
    if constexpr (KIND == 2) { zlo = q.Z[(size_t)im.x * nst + g]; zhi = q.Z[(size_t)(im.x + im.y) * nst + g]; }
    }
  };
  float u_n = 0.f, wlo_n = 0.f, whi_n = 0.f, zlo_n = 0.f, zhi_n = 0.f;
  int m_n = 0;
  if (a.K > 0) step_src(a.K - 1, u_n, wlo_n, whi_n, zlo_n, zhi_n, m_n);
  for (int k = a.K - 1; k >= 0; --k) {
    const float u = live ? u_n : 0.f;
    const float dW = live ? whi_n - wlo_n : 0.f;     // k_sde_dw's expression
    const float dZ = live ? zhi_n - zlo_n : 0.f;
    const float dt = (float)m_n * a.h;
    if (k > 0) step_src(k - 1, u_n, wlo_n, whi_n, zlo_n, zhi_n, m_n);
    // cotangents of the series values taken inside step k: theta of each onto the step's end state ...
    for (int j = 0; j < a.nseries; ++j)
      if (sk[j] == k) { const float th = sth[j]; if (th != 0.f && live) ub = ub + th * a.du_series[(size_t)j * nst + g]; }
    if constexpr (KIND == 1) ub = sba_mil_step<false>(c, a, live, u, dW, dt, ub, 0.f);
    else ub = sba_sri_step<false>(c, a, q.T, live, u, dW, dZ, dt, ub, 0.f);
    __syncthreads();
    c.accumulate();
    // ... and 1 - theta of the series values onto its start state
    for (int j = 0; j < a.nseries; ++j)
      if (sk[j] == k) { const float th = sth[j]; if (th != 1.0f && live) ub = ub + (1.0f - th) * a.du_series[(size_t)j * nst + g]; }
    __syncthreads();
  }
  for (int j = 0; j < a.nseries; ++j)   // a saved start value is the input itself
    if (sk[j] < 0 && live) ub = ub + a.du_series[(size_t)j * nst + g];
  if (live) a.dx[g] = ub;
  c.store_partial(a.part);
}

// d(EEst*dt)/dp of the recorded local step: the step function entered with the residual's seed.  No dx.
template <int KIND>
__global__ __launch_bounds__(SBF_NT) void k_sde_alg_reg_fused(SdeAlgBwdArgs q) {
  static_assert(KIND == 1 || KIND == 2, "1 Milstein, 2 SRI");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const SdeBwdFusedArgs& a = q.a;
  SbfDev c;
  c.setup(a, sm, sba_nev(KIND), sba_own_xg(KIND));
  __syncthreads();
  c.ones();
  const bool live = c.valid && c.row;
  const size_t g = c.g;
  const float u = live ? a.u1[g] : 0.f, dW = live ? a.dW1[g] : 0.f, un = live ? a.un1[g] : 0.f;
  if constexpr (KIND == 1) (void)sba_mil_step<true>(c, a, live, u, dW, a.dt1, 0.f, un);
  else {
    const float dZ = live ? q.dZ1[g] : 0.f;
    (void)sba_sri_step<true>(c, a, q.T, live, u, dW, dZ, a.dt1, 0.f, un);
  }
  __syncthreads();
  c.accumulate();
  c.store_partial(a.part);
}

}  // namespace

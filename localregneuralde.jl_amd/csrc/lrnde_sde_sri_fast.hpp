// lrnde_sde_sri_fast.hpp — one ATTEMPTED step of the adaptive four-stage SRI solve (FourStageSRIConstantCache, diagonal
// noise: src/perform_step.jl:49-106 — the step the reference's default solver SOSRI runs) as ONE launch with the step-size
// controller in its footer, for the shapes of lrnde_sde_fast.hpp (drift Chain(Dense(D => H, act), Dense(H => D)) without a
// time input, diffusion Dense(D => D), D <= 64, H <= 128).  Included by lrnde_kernels.hip inside its anonymous namespace,
// after lrnde_sde_mil_fast.hpp; argument struct (SdeFastArgs, whose `tab` is the caller's tableau by value), control block
// (SdeCtl), dot product (sf_chain) and controller (sde_ctl_update) are lrnde_sde_fast.hpp's.
//
// The layout is k_sde_mil_fast's: a workgroup is four waves on 16 columns; the three weight matrices are
// v_mfma_f32_16x16x4_f32 A fragments in registers (wave w: hidden tiles w, w + 4 of Dense-1; Dense-2 tile w for w < DT; the
// diffusion tiles round-robin); the step's algebra stays in the C-fragment registers of the wave that owns the Dense-2
// tile, and nothing goes through global memory between the loads of (u, W[i], W[i + m], Z[i], Z[i + m]) and the store of
// u_new.  The step is four rounds; round j = 1..4:
//   [drift Dense-1 + activation of H0_{j-1} on four waves | the diffusion tile of H1_{j-1}]  barrier
//   [drift Dense-2 -> k_j, g_j from the diffusion tile; H0_j, H1_j formed and put into the two x tiles]  barrier
// with H0_0 = H1_0 = uprev (:62-63), H0_j / H1_j the stage expressions (:65-66, :71-72, :77-82) and, after round 4, u_new
// (:84-97) and the residual of the seven-argument _calculate_residuals, (delta E1 + E2) / (abstol + max(|u|, |u_new|) reltol)
// (:99-104, :214-216).  The drift's and the diffusion's inputs differ from round 2 on: both x tiles are live in every round.
// Arithmetic: dW / dZ by k_sde_dw's expression, chi1..3 by k_sri_chi's, the stages by k_sri_stage's and the final
// combination by k_sri_final's, each in its own association order; every dot product is the canonical k-ordered chain — so
// u_new has the bits of lrnde_sde_sri_step and of the oracle's SRI step.  Squares of the residual are fp32, their sums fp64;
// padded rows and columns contribute nothing.
// Footer (the last workgroup to arrive, as in k_sde_mil_fast): the workgroups' fp64 partial sums added in partial-vector
// order, sde_ctl_update with four drift evaluations per attempt, trace row, the layer's dense record (rec_u / rec_im), the
// pinned progress word.  The host keeps launches enqueued (sde_adaptive_device); there is no persistent form of this kernel.

template <int DT, int HT>
__global__ __launch_bounds__(SF_NT) void k_sde_sri_fast(SdeFastArgs a) {
  static_assert(DT >= 1 && DT <= 4 && HT >= 1 && HT <= 8, "D <= 64, H <= 128");
  constexpr int NJ = (HT + 3) / 4;   // hidden tiles per wave
  if (!a.ctl) return;                // (the adaptive loop is this kernel's only caller)
  const SdeCtl cc = *a.ctl;          // written by the previous launch's last workgroup (kernel boundary in between) / by k_sde_ctl_init
  if (cc.status != ST_RUNNING) return;
  const int ad_i = cc.i, ad_m = cc.m, ad_slot = cc.naccept;
  const float dt = (float)ad_m * a.h;
  const float* up = cc.cur ? a.ub : a.ua;
  float* unp = cc.cur ? a.ua : a.ub;
  // LDS: two x tiles in B-operand layout ([kg][64 lanes] float4: the drift's input H0 and the diffusion's H1), the h tile, the
  // diffusion results in C-fragment order
  __shared__ f32x4 xA[DT * 64], xB[DT * 64], hl[HT * 64], gl[DT * 64];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, rq = lane >> 4;
  const int b0 = blockIdx.x * 16;
  const bool colok = b0 + n < a.B;
  const int D = a.D;
  const bool has_d2 = wave < DT;
  const int t = has_d2 ? wave : 0;
  const int tg = (wave >= DT && wave < 2 * DT) ? wave - DT : ((wave + 4 >= DT && wave + 4 < 2 * DT) ? wave + 4 - DT : -1);
  f32x4 w1[NJ][DT], w2[HT], wg[DT];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ht = wave + 4 * j;
#pragma unroll
    for (int kg = 0; kg < DT; ++kg) w1[j][kg] = ht < HT ? a.W1p[((size_t)ht * a.KG1 + kg) * 64 + lane] : zero4;
  }
#pragma unroll
  for (int kg = 0; kg < HT; ++kg) w2[kg] = has_d2 ? a.W2p[((size_t)t * a.KG2p + kg) * 64 + lane] : zero4;
#pragma unroll
  for (int kg = 0; kg < DT; ++kg) wg[kg] = tg >= 0 ? a.Wgp[((size_t)tg * a.KGgp + kg) * 64 + lane] : zero4;
  f32x4 b1v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) b1v[j] = (wave + 4 * j < HT) ? *reinterpret_cast<const f32x4*>(a.b1 + (wave + 4 * j) * 16 + rq * 4) : zero4;
  const f32x4 b2v = has_d2 ? *reinterpret_cast<const f32x4*>(a.b2 + t * 16 + rq * 4) : zero4;
  const f32x4 bgv = tg >= 0 ? *reinterpret_cast<const f32x4*>(a.bg + tg * 16 + rq * 4) : zero4;
  // this lane's four rows (16 t + 4 rq + r) of column n
  const int row0 = t * 16 + rq * 4;
  const bool vec = (D & 3) == 0;
  const bool live = has_d2 && colok && row0 < D;
  const size_t g = (size_t)(b0 + n) * D + row0;
  const size_t nn = (size_t)a.B * D;
  auto ld4s = [&](const float* p) {
    f32x4 v = zero4;
    if (vec) v = *reinterpret_cast<const f32x4*>(p + g);
    else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (row0 + r < D) v[r] = p[g + r];
    }
    return v;
  };
  auto st4s = [&](float* p, const f32x4& v) {
    if (vec) *reinterpret_cast<f32x4*>(p + g) = v;
    else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (row0 + r < D) p[g + r] = v[r];
    }
  };
  f32x4 u4 = zero4, w4 = zero4, z4 = zero4;
  if (live) {
    u4 = ld4s(up);
    const f32x4 wlo = ld4s(a.Wpath + (size_t)ad_i * nn);   // dW = W[i + m] - W[i], dZ = Z[i + m] - Z[i] (the expression of k_sde_dw)
    const f32x4 whi = ld4s(a.Wpath + (size_t)(ad_i + ad_m) * nn);
    const f32x4 zlo = ld4s(a.Zpath + (size_t)ad_i * nn);
    const f32x4 zhi = ld4s(a.Zpath + (size_t)(ad_i + ad_m) * nn);
#pragma unroll
    for (int r = 0; r < 4; ++r) { w4[r] = whi[r] - wlo[r]; z4[r] = zhi[r] - zlo[r]; }
  }
  // B-operand image of rows 16 t + 4 rq + r, column n: float4 index t*64 + r*16 + n, component rq
  auto put = [&](f32x4* x, const f32x4& v) {
    float* p = reinterpret_cast<float*>(x) + ((t * 64 + n) << 2) + rq;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r * 64] = v[r];
  };
  if (has_d2) put(xA, u4);
  __syncthreads();
  const lrnde_sri_tableau& T = a.tab;
  const float sqdt = __builtin_sqrtf(__builtin_fabsf(dt));
  // chi1, chi2, chi3 (:57-59; the expressions of k_sri_chi)
  f32x4 chi1, chi2, chi3;
  {
    const float sqrt3 = __builtin_sqrtf(3.0f), two_sqdt = 2.0f * sqdt, six_dt = 6.0f * dt, adt = __builtin_fabsf(dt);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = w4[r];
      chi1[r] = (w * w - adt) / two_sqdt;
      chi2[r] = (w + z4[r] / sqrt3) / 2.0f;
      chi3[r] = ((w * w) * w - (3.0f * w) * dt) / six_dt;
    }
  }
  // drift Dense-1 + activation of this wave's hidden tiles on the x tile xs -> hl
  auto dense1 = [&](const f32x4* xs) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ht = wave + 4 * j;
      if (ht < HT) {
        const f32x4 acc = sf_chain<DT>(w1[j], xs, lane);
        float* p = reinterpret_cast<float*>(hl) + ((ht * 64 + n) << 2) + rq;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r * 64] = act_apply_sel(a.act, acc[r] + b1v[j][r]);
      }
    }
  };
  auto diffusion = [&](const f32x4* xs) {  // tile tg of g(xs) -> gl (C-fragment order)
    if (tg < 0) return;
    f32x4 acc = sf_chain<DT>(wg, xs, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + bgv[r];
    gl[tg * 64 + lane] = acc;
  };
  auto dense2 = [&]() {  // tile t of f = W2 h + b2
    f32x4 acc = sf_chain<HT>(w2, hl, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + b2v[r];
    return acc;
  };
  f32x4 k1 = zero4, k2 = zero4, k3 = zero4, g1 = zero4, g2 = zero4, g3 = zero4;
  // ---- round 1: k1 = f(uprev), g1 = g(uprev) (:62-63); H0_1, H1_1 (:65-66) ----
  dense1(xA);
  diffusion(xA);
  __syncthreads();
  if (has_d2) {
    k1 = dense2();
    g1 = gl[t * 64 + lane];
    const float da = dt * T.a021, db = dt * T.a121, sb = sqdt * T.b121;
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + da * k1[r]) + (T.b021 * chi2[r]) * g1[r];
      h1[r] = (u4[r] + db * k1[r]) + sb * g1[r];
    }
    put(xA, h0); put(xB, h1);   // (xA is free: every wave has read it — barrier above)
  }
  __syncthreads();
  // ---- round 2: k2 = f(H0_1), g2 = g(H1_1) (:67-68); H0_2, H1_2 (:71-72) ----
  dense1(xA);
  diffusion(xB);
  __syncthreads();
  if (has_d2) {
    k2 = dense2();
    g2 = gl[t * 64 + lane];
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + dt * (T.a031 * k1[r] + T.a032 * k2[r])) + chi2[r] * (T.b031 * g1[r] + T.b032 * g2[r]);
      h1[r] = (u4[r] + dt * (T.a131 * k1[r] + T.a132 * k2[r])) + sqdt * (T.b131 * g1[r] + T.b132 * g2[r]);
    }
    put(xA, h0); put(xB, h1);
  }
  __syncthreads();
  // ---- round 3: k3 = f(H0_2), g3 = g(H1_2) (:73-74); H0_3, H1_3 (:77-82) ----
  dense1(xA);
  diffusion(xB);
  __syncthreads();
  if (has_d2) {
    k3 = dense2();
    g3 = gl[t * 64 + lane];
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + dt * ((T.a041 * k1[r] + T.a042 * k2[r]) + T.a043 * k3[r])) +
              chi2[r] * ((T.b041 * g1[r] + T.b042 * g2[r]) + T.b043 * g3[r]);
      h1[r] = (u4[r] + dt * ((T.a141 * k1[r] + T.a142 * k2[r]) + T.a143 * k3[r])) +
              sqdt * ((T.b141 * g1[r] + T.b142 * g2[r]) + T.b143 * g3[r]);
    }
    put(xA, h0); put(xB, h1);
  }
  __syncthreads();
  // ---- round 4: k4 = f(H0_3), g4 = g(H1_3) (:83-84); u_new and the residual (:86-104; the expressions of k_sri_final) ----
  dense1(xA);
  diffusion(xB);
  __syncthreads();
  if (has_d2) {
    const f32x4 k4 = dense2();
    const f32x4 g4 = gl[t * 64 + lane];
    f32x4 un;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s3 = ((T.beta31 * g1[r] + T.beta32 * g2[r]) + T.beta33 * g3[r]) + T.beta34 * g4[r];
      const float s4 = ((T.beta41 * g1[r] + T.beta42 * g2[r]) + T.beta43 * g3[r]) + T.beta44 * g4[r];
      const float E2 = chi2[r] * s3 + chi3[r] * s4;
      const float sa = ((T.alpha1 * k1[r] + T.alpha2 * k2[r]) + T.alpha3 * k3[r]) + T.alpha4 * k4[r];
      const float s1 = ((T.beta11 * g1[r] + T.beta12 * g2[r]) + T.beta13 * g3[r]) + T.beta14 * g4[r];
      const float s2 = ((T.beta21 * g1[r] + T.beta22 * g2[r]) + T.beta23 * g3[r]) + T.beta24 * g4[r];
      un[r] = (((u4[r] + dt * sa) + E2) + w4[r] * s1) + chi1[r] * s2;
      if (live && row0 + r < D) {
        const float E1 = dt * (((k1[r] + k2[r]) + k3[r]) + k4[r]);
        const float sc = a.abstol + fmaxf_(__builtin_fabsf(u4[r]), __builtin_fabsf(un[r])) * a.reltol;
        const float rr = (a.delta * E1 + E2) / sc;
        const float sq = rr * rr;
        acc += (double)sq;
      }
    }
    if (live) {
      st4s(unp, un);
      if (a.rec_u && ad_slot < a.rec_cap) st4s(a.rec_u + (size_t)ad_slot * nn, un);
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) red[wave] = acc;
  }
  __syncthreads();
  // ---- footer: the last workgroup to arrive reduces the partials and runs the controller ----
  if (threadIdx.x >= 64) return;
  double tot = red[0];
#pragma unroll
  for (int w = 1; w < DT; ++w) tot += red[w];
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
    SdeCtl c = *a.ctl;
    sde_ctl_update(c, eest, dt, a, true, fastpow(c.qold, a.beta2), 4);
    *a.ctl = c;
    __hip_atomic_store(a.prog, sde_report_pack((unsigned)(a.jlaunch + 1), (unsigned)c.status),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(a.arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int DT> inline void sde_sri_fast_launch_h(int HT, int nwg, hipStream_t st, const SdeFastArgs& f) {
  switch (HT) {
    case 1: hipLaunchKernelGGL((k_sde_sri_fast<DT, 1>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 2: hipLaunchKernelGGL((k_sde_sri_fast<DT, 2>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 3: hipLaunchKernelGGL((k_sde_sri_fast<DT, 3>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 4: hipLaunchKernelGGL((k_sde_sri_fast<DT, 4>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 5: hipLaunchKernelGGL((k_sde_sri_fast<DT, 5>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 6: hipLaunchKernelGGL((k_sde_sri_fast<DT, 6>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 7: hipLaunchKernelGGL((k_sde_sri_fast<DT, 7>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    default: hipLaunchKernelGGL((k_sde_sri_fast<DT, 8>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
  }
}
// launch by shape: DT = ceil(D / 16) in 1..4, HT = ceil(H / 16) in 1..8 (the caller has checked sde_fast_shape)
inline void sde_sri_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  const int DT = (D + 15) / 16, HT = (H + 15) / 16;
  switch (DT) {
    case 1: sde_sri_fast_launch_h<1>(HT, nwg, st, f); break;
    case 2: sde_sri_fast_launch_h<2>(HT, nwg, st, f); break;
    case 3: sde_sri_fast_launch_h<3>(HT, nwg, st, f); break;
    default: sde_sri_fast_launch_h<4>(HT, nwg, st, f); break;
  }
}

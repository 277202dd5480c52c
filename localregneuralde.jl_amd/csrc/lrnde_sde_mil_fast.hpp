// lrnde_sde_mil_fast.hpp — one ATTEMPTED step of the adaptive Milstein solve (RKMilCommute, diagonal noise, Ito:
// src/perform_step.jl:108-170) as ONE launch with the step-size controller in its footer, for the shapes of
// lrnde_sde_fast.hpp (drift Chain(Dense(D => H, act), Dense(H => D)) without a time input, diffusion Dense(D => D),
// D <= 64, H <= 128).  Included by lrnde_kernels.hip inside its anonymous namespace, after lrnde_sde_fast.hpp, whose
// argument struct (SdeFastArgs), control block (SdeCtl), dot product (sf_chain) and controller (sde_ctl_update) it uses.
//
// The layout is k_sde_eh_fast's non-persistent form: a workgroup is four waves on 16 columns; the three weight matrices are
// v_mfma_f32_16x16x4_f32 A fragments in registers (wave w: hidden tiles w, w + 4 of Dense-1; Dense-2 tile w for w < DT; the
// diffusion tiles round-robin); the step's algebra stays in the C-fragment registers of the wave that owns the Dense-2
// tile, and nothing goes through global memory between the first load of (u, W[i], W[i + m]) and the store of u_new.
// The step is two rounds instead of Euler-Heun's three:
//   1. du1 = f(u), L = g(u)                                  (:130-131)
//   2. gtmp = g(K + sqrt(dt) L),  K = u + dt du1             (:133-138; no drift evaluation: du2 / En are dead code in the
//                                                             reference, lrnde_sde_rkmil_step)
//   then  u_new = (K + L dW) + Dgj J,  Dgj = (gtmp - L) / sqrt(dt),  J = dW^2 / 2 - |dt| / 2          (:117-141)
//   and the residual of the four-argument _calculate_residuals, (u_new - u) / (abstol + max(|u|, |u_new|) reltol)
//   (:166-169, :218-220 — the reference's form, kept as it is).
// Arithmetic: the canonical k-ordered chains and the elementwise expressions of k_sde_rkmil, so u_new and EEst are the bits
// of k_sde_rkmil and of the oracle's rkmil_step.
// Footer (the last workgroup to arrive, as in k_sde_eh_fast): the workgroups' fp64 partial sums added in partial-vector
// order, sde_ctl_update with one drift evaluation per attempt, trace row, the layer's dense record (rec_u / rec_im), the
// pinned progress word.  The host keeps launches enqueued (sde_adaptive_device); there is no persistent form of this kernel.

template <int DT, int HT>
__global__ __launch_bounds__(SF_NT) void k_sde_mil_fast(SdeFastArgs a) {
  static_assert(DT >= 1 && DT <= 4 && HT >= 1 && HT <= 8, "D <= 64, H <= 128");
  constexpr int NJ = (HT + 3) / 4;   // hidden tiles per wave
  if (!a.ctl) return;                // (the adaptive loop is this kernel's only caller)
  const SdeCtl cc = *a.ctl;          // written by the previous launch's last workgroup (kernel boundary in between) / by k_sde_ctl_init
  if (cc.status != ST_RUNNING) return;
  const int ad_i = cc.i, ad_m = cc.m, ad_slot = cc.naccept;
  const float dt = (float)ad_m * a.h;
  const float* up = cc.cur ? a.ub : a.ua;
  float* unp = cc.cur ? a.ua : a.ub;
  // LDS: two x tiles in B-operand layout ([kg][64 lanes] float4), the h tile, the diffusion results in C-fragment order
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
  f32x4 u4 = zero4, w4 = zero4;
  if (live) {
    u4 = ld4s(up);
    const f32x4 lo = ld4s(a.Wpath + (size_t)ad_i * nn);   // dW = W[i + m] - W[i] (the expression of k_sde_dw)
    const f32x4 hi = ld4s(a.Wpath + (size_t)(ad_i + ad_m) * nn);
#pragma unroll
    for (int r = 0; r < 4; ++r) w4[r] = hi[r] - lo[r];
  }
  // B-operand image of rows 16 t + 4 rq + r, column n: float4 index t*64 + r*16 + n, component rq
  auto put = [&](f32x4* x, const f32x4& v) {
    float* p = reinterpret_cast<float*>(x) + ((t * 64 + n) << 2) + rq;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r * 64] = v[r];
  };
  if (has_d2) put(xA, u4);
  __syncthreads();
  const float sqdt = __builtin_sqrtf(dt), hdt = 0.5f * __builtin_fabsf(dt);
  auto diffusion = [&](const f32x4* xs) {  // tile tg of g(xs) -> gl (C-fragment order)
    if (tg < 0) return;
    f32x4 acc = sf_chain<DT>(wg, xs, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = acc[r] + bgv[r];
    gl[tg * 64 + lane] = acc;
  };
  // ---- round 1: du1 = f(u), L = g(u) (:130-131) ----
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ht = wave + 4 * j;
    if (ht < HT) {
      const f32x4 acc = sf_chain<DT>(w1[j], xA, lane);
      float* p = reinterpret_cast<float*>(hl) + ((ht * 64 + n) << 2) + rq;
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r * 64] = act_apply_sel(a.act, acc[r] + b1v[j][r]);
    }
  }
  diffusion(xA);
  __syncthreads();
  f32x4 L = zero4, Kv = zero4;
  if (has_d2) {
    f32x4 du1 = sf_chain<HT>(w2, hl, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) du1[r] = du1[r] + b2v[r];
    L = gl[t * 64 + lane];
    f32x4 tmp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Kv[r] = u4[r] + dt * du1[r];          // :133
      tmp[r] = Kv[r] + sqdt * L[r];         // :136-137 (Ito)
    }
    put(xB, tmp);
  }
  __syncthreads();
  // ---- round 2: gtmp = g(tmp) (:138) ----
  diffusion(xB);
  __syncthreads();
  if (has_d2) {
    const f32x4 gt = gl[t * 64 + lane];
    f32x4 un;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float J = (0.5f * w4[r]) * w4[r] - hdt;                         // :117, :122
      const float Dgj = (gt[r] - L[r]) / sqdt;                              // :139
      un[r] = (Kv[r] + L[r] * w4[r]) + Dgj * J;                             // :141
      if (live && row0 + r < D) {
        const float sc = a.abstol + fmaxf_(__builtin_fabsf(u4[r]), __builtin_fabsf(un[r])) * a.reltol;
        const float rr = (un[r] - u4[r]) / sc;                              // :166, :218-220
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
    sde_ctl_update(c, eest, dt, a, true, fastpow(c.qold, a.beta2), 1);
    *a.ctl = c;
    __hip_atomic_store(a.prog, sde_report_pack((unsigned)(a.jlaunch + 1), (unsigned)c.status),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(a.arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int DT> inline void sde_mil_fast_launch_h(int HT, int nwg, hipStream_t st, const SdeFastArgs& f) {
  switch (HT) {
    case 1: hipLaunchKernelGGL((k_sde_mil_fast<DT, 1>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 2: hipLaunchKernelGGL((k_sde_mil_fast<DT, 2>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 3: hipLaunchKernelGGL((k_sde_mil_fast<DT, 3>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 4: hipLaunchKernelGGL((k_sde_mil_fast<DT, 4>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 5: hipLaunchKernelGGL((k_sde_mil_fast<DT, 5>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 6: hipLaunchKernelGGL((k_sde_mil_fast<DT, 6>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    case 7: hipLaunchKernelGGL((k_sde_mil_fast<DT, 7>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
    default: hipLaunchKernelGGL((k_sde_mil_fast<DT, 8>), dim3(nwg), dim3(SF_NT), 0, st, f); break;
  }
}
// launch by shape: DT = ceil(D / 16) in 1..4, HT = ceil(H / 16) in 1..8 (the caller has checked sde_fast_shape)
inline void sde_mil_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  const int DT = (D + 15) / 16, HT = (H + 15) / 16;
  switch (DT) {
    case 1: sde_mil_fast_launch_h<1>(HT, nwg, st, f); break;
    case 2: sde_mil_fast_launch_h<2>(HT, nwg, st, f); break;
    case 3: sde_mil_fast_launch_h<3>(HT, nwg, st, f); break;
    default: sde_mil_fast_launch_h<4>(HT, nwg, st, f); break;
  }
}

// lrnde_sde_sri_fast.hip — one ATTEMPTED step of the adaptive four-stage SRI solve (FourStageSRIConstantCache, diagonal
// noise: src/perform_step.jl:49-106 — the step the reference's default solver SOSRI runs) as ONE launch with the step-size
// controller in its footer, for the shapes of lrnde_sde_fast.hpp (drift Chain(Dense(D => H, act), Dense(H => D)) without a
// time input, diffusion Dense(D => D), D <= 64, H <= 128).  A translation unit of its own: the library calls
// sde_sri_fast_launch (lrnde_sde_fast.hpp, with the argument struct SdeFastArgs, whose `tab` is the caller's tableau by value);
// the control block (SdeCtl) is lrnde_stepctl.hpp's, the workgroup frame (SdeFrame: the layout, the resident weight fragments,
// dense1 / diffusion / dense2), the footer (sde_step_footer) and the launch dispatch (sde_fast_dispatch) are lrnde_sde_frame.hpp's.
//
// Nothing goes through global memory between the loads of (u, W[i], W[i + m], Z[i], Z[i + m]) and the store of
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
// Footer: sde_step_footer with four drift evaluations per attempt.  The host keeps launches enqueued (sde_adaptive_device);
// there is no persistent form of this kernel.
#include <hip/hip_runtime.h>

#include "lrnde_sde_frame.hpp"

namespace {

using namespace lrnde;

// TREE: dW and dZ from the virtual trees of streams 6 and 7 (lrnde_sde_tree.hpp) instead of a.Wpath / a.Zpath, recorded beside rec_u.
template <int DT, int HT, bool TREE = false>
__global__ __launch_bounds__(SF_NT) void k_sde_sri_fast(SdeFastArgs a) {
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
  const SdeFrame<DT, HT> F(a, hl, gl);
  const int lane = F.lane, wave = F.wave, t = F.t, row0 = F.row0, D = F.D;
  const bool has_d2 = F.has_d2, live = F.live;
  const size_t nn = F.nn;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 u4 = zero4, w4 = zero4, z4 = zero4;
  if (live) {
    u4 = F.ld4s(up);
    if constexpr (TREE) { w4 = F.dtree(a.tree, TREE_STREAM_W, ad_i, ad_m); z4 = F.dtree(a.tree, TREE_STREAM_Z, ad_i, ad_m); }
    else { w4 = F.dpath(a.Wpath, ad_i, ad_m); z4 = F.dpath(a.Zpath, ad_i, ad_m); }
  }
  if (has_d2) F.put(xA, u4);
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
  f32x4 k1 = zero4, k2 = zero4, k3 = zero4, g1 = zero4, g2 = zero4, g3 = zero4;
  // ---- round 1: k1 = f(uprev), g1 = g(uprev) (:62-63); H0_1, H1_1 (:65-66) ----
  F.dense1(xA);
  F.diffusion(xA);
  __syncthreads();
  if (has_d2) {
    k1 = F.dense2();
    g1 = gl[t * 64 + lane];
    const float da = dt * T.a021, db = dt * T.a121, sb = sqdt * T.b121;
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + da * k1[r]) + (T.b021 * chi2[r]) * g1[r];
      h1[r] = (u4[r] + db * k1[r]) + sb * g1[r];
    }
    F.put(xA, h0); F.put(xB, h1);   // (xA is free: every wave has read it — barrier above)
  }
  __syncthreads();
  // ---- round 2: k2 = f(H0_1), g2 = g(H1_1) (:67-68); H0_2, H1_2 (:71-72) ----
  F.dense1(xA);
  F.diffusion(xB);
  __syncthreads();
  if (has_d2) {
    k2 = F.dense2();
    g2 = gl[t * 64 + lane];
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + dt * (T.a031 * k1[r] + T.a032 * k2[r])) + chi2[r] * (T.b031 * g1[r] + T.b032 * g2[r]);
      h1[r] = (u4[r] + dt * (T.a131 * k1[r] + T.a132 * k2[r])) + sqdt * (T.b131 * g1[r] + T.b132 * g2[r]);
    }
    F.put(xA, h0); F.put(xB, h1);
  }
  __syncthreads();
  // ---- round 3: k3 = f(H0_2), g3 = g(H1_2) (:73-74); H0_3, H1_3 (:77-82) ----
  F.dense1(xA);
  F.diffusion(xB);
  __syncthreads();
  if (has_d2) {
    k3 = F.dense2();
    g3 = gl[t * 64 + lane];
    f32x4 h0, h1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h0[r] = (u4[r] + dt * ((T.a041 * k1[r] + T.a042 * k2[r]) + T.a043 * k3[r])) +
              chi2[r] * ((T.b041 * g1[r] + T.b042 * g2[r]) + T.b043 * g3[r]);
      h1[r] = (u4[r] + dt * ((T.a141 * k1[r] + T.a142 * k2[r]) + T.a143 * k3[r])) +
              sqdt * ((T.b141 * g1[r] + T.b142 * g2[r]) + T.b143 * g3[r]);
    }
    F.put(xA, h0); F.put(xB, h1);
  }
  __syncthreads();
  // ---- round 4: k4 = f(H0_3), g4 = g(H1_3) (:83-84); u_new and the residual (:86-104; the expressions of k_sri_final) ----
  F.dense1(xA);
  F.diffusion(xB);
  __syncthreads();
  if (has_d2) {
    const f32x4 k4 = F.dense2();
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
      F.st4s(unp, un);
      if (a.rec_u && ad_slot < a.rec_cap) F.st4s(a.rec_u + (size_t)ad_slot * nn, un);
      if constexpr (TREE) {
        if (a.tree.rec_dw && ad_slot < a.rec_cap) { F.st4s(a.tree.rec_dw + (size_t)ad_slot * nn, w4); F.st4s(a.tree.rec_dz + (size_t)ad_slot * nn, z4); }
      }
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) red[wave] = acc;
  }
  __syncthreads();
  sde_step_footer<DT>(a, red, dt, true, 4);
}

}  // namespace

namespace lrnde {

void sde_sri_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    if (f.tree.on) hipLaunchKernelGGL((k_sde_sri_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), 0, st, f);
    else hipLaunchKernelGGL((k_sde_sri_fast<dt.value, ht.value>), dim3(nwg), dim3(SF_NT), 0, st, f);
  });
}

}  // namespace lrnde

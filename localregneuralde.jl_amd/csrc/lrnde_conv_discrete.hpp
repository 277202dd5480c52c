// lrnde_conv_discrete.hpp — the discrete adjoint of the conv handle's recorded Tsit5 solve: a reverse sweep over the step
// record instead of a reversed solve.  Included by lrnde_conv.hip inside its anonymous namespace,
// behind launch_vjp, lincomb and ensure_adj.
//
// Semantics: what lrnde_set_sensealg states for LRNDE_SENSE_DISCRETE (UPSTREAM-RECALL, frozen grid: a tape does not
// differentiate the step-size controller).  loss = <du_end, sol.u[end]> (+ w_reg * reg_val, whose gradient stays
// step_reg_grad's, added by the caller).  The record is lrnde_conv_node_forward_record's: accepted steps n = 0..N-1 with
// t_n, dt_n (dense_t, dense_dt) and [uprev, k1..k7] per step.  The gradient is the exact derivative of the discrete forward
// map with the times and step sizes constants; rejected attempts do not appear; first-same-as-last is differentiated
// (k1 of step n+1 is k7 of step n); u(t1) of the local step — and with it every saved state of `unbiased` and `biased`
// mode — stays a constant.
//
// Reverse sweep (ub: cotangent of u_{n+1}, kap: cotangent of this step's k7 = the k1 cotangent of step n+1):
//   ub = du_end, kap = 0.  For n = N-1 .. 0 (t = t_n, dt = dt_n, all times formed in fp32 as the forward forms them):
//     1. n < N-1:  (w, gp) = VJP(uprev_{n+1}, t + dt, kap);  ub = ub + w          (skipped for the last step: kap = 0)
//     2. i = 6..2: g_i   = uprev + dt * (((a_i1 k_1 + a_i2 k_2) + a_i3 k_3) ...)   (the forward's lincomb, same bits)
//                  lam_i = dt * (((a_7i ub + a_{i+1,i} gb_{i+1}) + ...) + a_6i gb_6)
//                  (gb_i, gp) = VJP(g_i, t + c_i dt, lam_i)
//     3. kap = dt * (((((a_71 ub + a_21 gb_2) + a_31 gb_3) + a_41 gb_4) + a_51 gb_5) + a_61 gb_6)
//        ub  = ((((ub + gb_2) + gb_3) + gb_4) + gb_5) + gb_6
//   (w, gp) = VJP(x, t_0, kap);  dx = ub + w.
// dp is the sum of every gp in the order the VJPs run (dp = dp + gp, one fp32 add per VJP), so two calls give the same
// bits.  6 N VJPs in all: N - 1 + 5 N + 1.  No norm is taken, so a sharded handle adds no exchange of its own to those of
// launch_vjp, whose gp is already summed over ranks: dx stays sharded, dp comes out replicated.
//
// Elementwise work: k_cdisc_stage<S> writes g_S and lam_S in one pass (S reads of the record slot, 7 - S of the kept
// cotangents, 2 writes) and k_cdisc_close writes kap and the next ub (6 reads, 2 writes); 16 bytes per load and store with
// every load of a thread issued before its first use, a scalar loop of the same arithmetic for n % 4 != 0 or a vector that is
// not 16-byte aligned (n is a multiple of 32 on this handle and every operand is a record slot or a workspace vector, so
// no call of today reaches the scalar loop; the caller's du_end is copied in and dx is written by lincomb, which has its
// own).  The three adds (ub + w, dx = ub + w, dp + gp) are lincomb's.
// Workspace (ensure_adj): ub, kap, gb_2..gb_6, g, lam, w — ten state vectors — and gp, dp — two parameter vectors; sized
// 11 n + 2 P so that the regulariser's sweep (11 n + P) behind this one does not grow it.

struct CdiscStageArgs {
  const float* rec;        // the step's record slot: row l of n floats = uprev (l = 0), k_l (l = 1..7)
  const float* ub;         // cotangent of u_{n+1}
  const float* gb;         // gb_j at gb + (j - 2) * n, j = 2..6
  float *g, *lam;          // out: stage input, stage cotangent
  float dt, c21;           // c21 = dt * a_21, formed on the host as the forward forms it
  float A[21];
  size_t n;
  int vec4;
};

// a_{r,c} of the strictly lower triangle, rows 2..7 (Tsit5F::A's layout)
__host__ __device__ constexpr int cdisc_a(int r, int c) { return (r - 2) * (r - 1) / 2 + (c - 1); }

template <int S> __device__ __forceinline__ void cdisc_stage_one(const CdiscStageArgs& a, const float* r, float ub, const float* gbv, float& g,
                                                                 float& lam) {
  // r[0] = uprev, r[l] = k_l, l < S; gbv[j - 2] = gb_j, j > S
  if constexpr (S == 2) g = r[0] + a.c21 * r[1];
  else {
    float s = a.A[cdisc_a(S, 1)] * r[1] + a.A[cdisc_a(S, 2)] * r[2];
#pragma unroll
    for (int l = 3; l < S; ++l) s = s + a.A[cdisc_a(S, l)] * r[l];
    g = r[0] + a.dt * s;
  }
  float q = a.A[cdisc_a(7, S)] * ub;
#pragma unroll
  for (int j = S + 1; j <= 6; ++j) q = q + a.A[cdisc_a(j, S)] * gbv[j - 2];
  lam = a.dt * q;
}

template <int S>
__global__ __launch_bounds__(256) void k_cdisc_stage(CdiscStageArgs a) {
  static_assert(S >= 2 && S <= 6, "stages 2..6");
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      f32x4 rv[S], gv[5];
#pragma unroll
      for (int l = 0; l < S; ++l) rv[l] = reinterpret_cast<const f32x4*>(a.rec + (size_t)l * a.n)[i];
      const f32x4 ub = reinterpret_cast<const f32x4*>(a.ub)[i];
#pragma unroll
      for (int j = S + 1; j <= 6; ++j) gv[j - 2] = reinterpret_cast<const f32x4*>(a.gb + (size_t)(j - 2) * a.n)[i];
      f32x4 g, lam;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        float r[S], gbv[5];
#pragma unroll
        for (int l = 0; l < S; ++l) r[l] = rv[l][h];
#pragma unroll
        for (int j = S + 1; j <= 6; ++j) gbv[j - 2] = gv[j - 2][h];
        float g1, l1;
        cdisc_stage_one<S>(a, r, ub[h], gbv, g1, l1);
        g[h] = g1; lam[h] = l1;
      }
      reinterpret_cast<f32x4*>(a.g)[i] = g;
      reinterpret_cast<f32x4*>(a.lam)[i] = lam;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      float r[S], gbv[5];
#pragma unroll
      for (int l = 0; l < S; ++l) r[l] = a.rec[(size_t)l * a.n + i];
#pragma unroll
      for (int j = S + 1; j <= 6; ++j) gbv[j - 2] = a.gb[(size_t)(j - 2) * a.n + i];
      float g1, l1;
      cdisc_stage_one<S>(a, r, a.ub[i], gbv, g1, l1);
      a.g[i] = g1; a.lam[i] = l1;
    }
  }
}

struct CdiscCloseArgs {
  float* ub;               // in: cotangent of u_{n+1}; out: cotangent of u_n (each element read and written by one thread)
  const float* gb;         // gb_2..gb_6
  float* kap;              // out: lam_1, the k7 cotangent of step n - 1
  float dt;
  float a1[6];             // a_71, a_21, a_31, a_41, a_51, a_61
  size_t n;
  int vec4;
};

__device__ __forceinline__ void cdisc_close_one(const CdiscCloseArgs& a, float& ub, const float* gbv, float& kap) {
  float q = a.a1[0] * ub;
#pragma unroll
  for (int j = 0; j < 5; ++j) q = q + a.a1[j + 1] * gbv[j];
  kap = a.dt * q;
  float s = ub;
#pragma unroll
  for (int j = 0; j < 5; ++j) s = s + gbv[j];
  ub = s;
}

__global__ __launch_bounds__(256) void k_cdisc_close(CdiscCloseArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      f32x4 gv[5];
      f32x4 ub = reinterpret_cast<const f32x4*>(a.ub)[i];
#pragma unroll
      for (int j = 0; j < 5; ++j) gv[j] = reinterpret_cast<const f32x4*>(a.gb + (size_t)j * a.n)[i];
      f32x4 kap;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        float gbv[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) gbv[j] = gv[j][h];
        float u1 = ub[h], k1;
        cdisc_close_one(a, u1, gbv, k1);
        ub[h] = u1; kap[h] = k1;
      }
      reinterpret_cast<f32x4*>(a.ub)[i] = ub;
      reinterpret_cast<f32x4*>(a.kap)[i] = kap;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      float gbv[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) gbv[j] = a.gb[(size_t)j * a.n + i];
      float u1 = a.ub[i], k1;
      cdisc_close_one(a, u1, gbv, k1);
      a.ub[i] = u1; a.kap[i] = k1;
    }
  }
}

inline bool cdisc_aligned(size_t n, std::initializer_list<const void*> ps) {
  bool ok = n % 4 == 0;
  for (const void* p : ps) ok = ok && ((uintptr_t)p % 16) == 0;
  return ok;
}
inline int cdisc_grid(size_t n, int vec4) {
  const size_t items = vec4 ? n / 4 : n;
  const size_t nb = (items + 255) / 256;
  return (int)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb));
}

template <int S> void cdisc_launch_stage(lrnde_conv* c, const CdiscStageArgs& a) {
  hipLaunchKernelGGL(k_cdisc_stage<S>, dim3(cdisc_grid(a.n, a.vec4)), dim3(256), 0, c->stream, a);
}

// the sweep over the record of the handle (R.valid, R.B == B and a Tsit5 record are the caller's checks): dx (n), dp (P)
int conv_discrete_sweep(lrnde_conv* c, int B, const float* du_end, float* dx, float* dp, lrnde_stats* st) {
  const size_t n = state_n(c, B), P = lrnde_conv_param_count(&c->d);
  const int N = (int)c->dense_t.size();
  int rc;
  if ((rc = ensure_adj(c, 11 * n + 2 * P))) return rc;   // (11 n + P is what the regulariser's sweep takes behind this one)
  float* W0 = c->adj;
  float *ub = W0, *kap = W0 + n, *gb = W0 + 2 * n, *g = W0 + 7 * n, *lam = W0 + 8 * n, *w = W0 + 9 * n;
  float *gtmp = W0 + 10 * n, *dpa = gtmp + P;
  const Tsit5F tb = tsit5_f32();
  const float one = 1.0f;
  int nvjp = 0;
  auto vjp = [&](const float* y, float t, const float* l, float* dy) -> int {   // dy = J^T l; dpa = dpa + gp
    int r;
    if ((r = launch_vjp(c, y, t, l, B, dy, gtmp))) return r;
    nvjp++;
    const float* g1[1] = {gtmp};
    return lincomb(c, dpa, dpa, 0.f, 1, g1, &one, P);
  };
  CHK(c, hipMemcpyAsync(ub, du_end, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  CHK(c, hipMemsetAsync(dpa, 0, sizeof(float) * P, c->stream));
  for (int s = N - 1; s >= 0; --s) {
    const float t = c->dense_t[s], dt = c->dense_dt[s];
    const float* rec = c->dense[s];
    if (s < N - 1) {   // 1. k7 of this step is k1 of the next: f(u_{n+1}, t + dt)
      if ((rc = vjp(c->dense[s + 1], t + tb.cs[5] * dt, kap, w))) return rc;
      const float* w1[1] = {w};
      if ((rc = lincomb(c, ub, ub, 0.f, 1, w1, &one, n))) return rc;
    }
    CdiscStageArgs a{};
    a.rec = rec; a.ub = ub; a.gb = gb; a.g = g; a.lam = lam; a.dt = dt; a.c21 = dt * tb.A[0]; a.n = n;
    for (int j = 0; j < 21; ++j) a.A[j] = tb.A[j];
    a.vec4 = cdisc_aligned(n, {rec, ub, gb, g, lam}) ? 1 : 0;
    for (int i = 6; i >= 2; --i) {   // 2.
      switch (i) {
        case 6: cdisc_launch_stage<6>(c, a); break;
        case 5: cdisc_launch_stage<5>(c, a); break;
        case 4: cdisc_launch_stage<4>(c, a); break;
        case 3: cdisc_launch_stage<3>(c, a); break;
        default: cdisc_launch_stage<2>(c, a); break;
      }
      CHK(c, hipGetLastError());
      if ((rc = vjp(g, t + tb.cs[i - 2] * dt, lam, gb + (size_t)(i - 2) * n))) return rc;
    }
    CdiscCloseArgs z{};   // 3.
    z.ub = ub; z.gb = gb; z.kap = kap; z.dt = dt; z.n = n;
    z.a1[0] = tb.A[cdisc_a(7, 1)];
    for (int j = 2; j <= 6; ++j) z.a1[j - 1] = tb.A[cdisc_a(j, 1)];
    z.vec4 = cdisc_aligned(n, {ub, gb, kap}) ? 1 : 0;
    hipLaunchKernelGGL(k_cdisc_close, dim3(cdisc_grid(n, z.vec4)), dim3(256), 0, c->stream, z);
    CHK(c, hipGetLastError());
  }
  // k1 of step 0 = f(x, t_0)
  if ((rc = vjp(c->dense[0], c->dense_t[0], kap, w))) return rc;
  { const float* w1[1] = {w}; if ((rc = lincomb(c, dx, ub, 0.f, 1, w1, &one, n))) return rc; }
  CHK(c, hipMemcpyAsync(dp, dpa, sizeof(float) * P, hipMemcpyDeviceToDevice, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));
  memset(st, 0, sizeof(*st));
  st->naccept = N; st->iters = N; st->nreject = 0; st->nf = nvjp;
  st->retcode = LRNDE_OK; st->t_final = c->dense_t[0];
  return LRNDE_OK;
}

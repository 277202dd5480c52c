// lrnde_conv_adams.hpp — VCAB3 / VCABM3 as the global solver of the NeuralODE layer over the conv field: the `solver`
// choices "vcab3" / "vcabm3" of experiments/src/construct.jl:154-164 (`_ode_solver`), which the reference hands to the
// CIFAR10 layer at :219-223.  Included by lrnde_conv.hip inside its anonymous namespace, behind launch_rhs, lincomb,
// fetch_sums and init_dt_g.
//
// UPSTREAM-RECALL, parity unpinned: OrdinaryDiffEq's Adams methods are not vendored by the reference; what is restated and
// what is recalled is said once, in lrnde_adams.hpp.  The algorithm is that file's adams_solve operation for operation (and
// so the oracle's adams_solve): ode_determine_initdt with order 3, two Bogacki-Shampine 3(2) start-up steps, the phi / phi* / g
// recurrences (lrnde_adams_math.hpp holds every per-element formula and the coefficient recurrence once), a rejected step
// changes nothing but dt, pi_order3() through the shared AttemptLoop, saveat by the cubic Hermite interpolant in the
// record's polynomial form [uprev, k1, P2, P3] evaluated with tsit5_rec_eval.  Deviation, stated there too: the reversed
// solve of a recorded Adams forward is the handle's Tsit5 adjoint.
//
// What is the conv handle's own is the elementwise work.  A conv state is large (2 097 152 floats at the CIFAR shape,
// B = 256) and every pass over it is memory-bound, so the kernels below move 16 bytes per load and store, issue every load of
// a thread before its first use, and fuse what the MLP loop does in several launches:
//   k_cadams_pred     phi*_1, phi*_2 and the predictor                                   4 reads, 3 writes
//   k_cadams_resid    phi(n+1), corrector (VCABM3), residual -> fp64 block partials      6 reads, VCABM3 1 write
//   k_cadams_bs3      the start-up step's residual (+ phi*_1 on the second one)          6 (+1) reads, (1 write)
//   k_cadams_record   an accepted step's record straight into its slot                   4 reads, 4 writes
//   k_cadams_eval     the Hermite interpolant at a saveat time, into the caller's slot   4 reads, 1 write
// Per attempted multistep step outside the f-eval: VCAB3 10 state-sized reads + 3 writes, VCABM3 10 + 4.
// (Writing VCAB3's P2 / P3 of every attempt into the next record slot from k_cadams_resid — kend is the new evaluation, so
// the operands are in registers — was built and measured: 14.0 + 7.8 us per accepted step against 10.3 + 12.4 us with the
// record kernel forming them, and 3.7 us more on every rejected attempt; a wash beside a 300 us f-eval, so it is not kept.)
// A vector that is not 16-byte aligned, or n % 4 != 0, takes the scalar loop of the same kernel (same arithmetic); n is a
// multiple of 8 on this handle, so only a caller's unaligned array reaches it.
// The residual kernels leave their block partials in c->sums in the triple layout of k_sums_err (other two slots zero), so
// fetch_sums serves the unsharded read-back and the sharded exchange unchanged.
// Every evaluation goes through launch_rhs: train-mode BatchNorm advances its running statistics once per evaluation, those
// of rejected attempts and of the start-up included, as in the Tsit5 solve; and every compute dtype of the handle works.

// (CAD_VECS state-sized work vectors in c->vec: lrnde_conv.hip's ensure_ws sizes it; the Tsit5 solve uses 11)

template <class... P> inline bool cad_vec4(size_t n, P... ps) {
  bool ok = n % 4 == 0;
  const void* v[] = {(const void*)ps...};
  for (const void* p : v) ok = ok && ((uintptr_t)p % 16) == 0;   // (a null optional pointer passes)
  return ok;
}
inline int cad_grid(size_t n, int vec4) {
  const size_t items = vec4 ? n / 4 : n;
  const size_t nb = (items + 255) / 256;
  return (int)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb));
}
#define CAD_V4(p) reinterpret_cast<const f32x4*>(p)[i]

struct CadPredArgs { const float *uprev, *k1, *kprev, *sp2; float *s2, *s3, *u; lrnde::AdamsCoef k; float dt; int three; size_t n; int vec4; };
__global__ __launch_bounds__(256) void k_cadams_pred(CadPredArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      const f32x4 up = CAD_V4(a.uprev), k1 = CAD_V4(a.k1), kp = CAD_V4(a.kprev), sp = CAD_V4(a.sp2);
      f32x4 v2, v3, un;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const lrnde::AdamsPred r = lrnde::adams_predict(up[h], k1[h], kp[h], sp[h], a.k, a.dt, a.three);
        v2[h] = r.v2; v3[h] = r.v3; un[h] = r.u;
      }
      reinterpret_cast<f32x4*>(a.s2)[i] = v2;
      reinterpret_cast<f32x4*>(a.s3)[i] = v3;
      reinterpret_cast<f32x4*>(a.u)[i] = un;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      const lrnde::AdamsPred r = lrnde::adams_predict(a.uprev[i], a.k1[i], a.kprev[i], a.sp2[i], a.k, a.dt, a.three);
      a.s2[i] = r.v2; a.s3[i] = r.v3; a.u[i] = r.u;
    }
  }
}

// du: the evaluation at the predicted state
struct CadResidArgs { const float *du, *k1, *s2, *s3, *uprev; float* u; float cu, ce, abstol, reltol; int moulton; size_t n; double* part; int vec4; };
__global__ __launch_bounds__(256) void k_cadams_resid(CadResidArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  double e0 = 0.0, z1 = 0.0, z2 = 0.0;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      const f32x4 du = CAD_V4(a.du), k1 = CAD_V4(a.k1), s2 = CAD_V4(a.s2), s3 = CAD_V4(a.s3), up = CAD_V4(a.uprev);
      f32x4 un = CAD_V4(a.u);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        float u = un[h];
        const float sq = lrnde::adams_correct(du[h], k1[h], s2[h], s3[h], up[h], u, a.cu, a.ce, a.moulton, a.abstol, a.reltol);
        un[h] = u;
        e0 += (double)sq;
      }
      if (a.moulton) reinterpret_cast<f32x4*>(a.u)[i] = un;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      float u = a.u[i];
      const float sq = lrnde::adams_correct(a.du[i], a.k1[i], a.s2[i], a.s3[i], a.uprev[i], u, a.cu, a.ce, a.moulton, a.abstol, a.reltol);
      e0 += (double)sq;
      if (a.moulton) a.u[i] = u;
    }
  }
  block_sum3(e0, z1, z2, a.part + (size_t)blockIdx.x * 3);
}

// Bogacki-Shampine 3(2) residual; s2 non-null (the second start-up step): phi*_1 for the first multistep step
struct CadBs3Args { const float *k1, *kb2, *kb3, *kend, *uprev, *u, *kprev; float* s2; float b2, dt, abstol, reltol; size_t n; double* part; int vec4; };
__global__ __launch_bounds__(256) void k_cadams_bs3(CadBs3Args a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  double e0 = 0.0, z1 = 0.0, z2 = 0.0;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      const f32x4 k1 = CAD_V4(a.k1), kb2 = CAD_V4(a.kb2), kb3 = CAD_V4(a.kb3), ke = CAD_V4(a.kend), up = CAD_V4(a.uprev), un = CAD_V4(a.u);
      f32x4 kp = {0.f, 0.f, 0.f, 0.f};
      if (a.s2) kp = CAD_V4(a.kprev);
      f32x4 v2;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        e0 += (double)lrnde::bs3_resid_sq(k1[h], kb2[h], kb3[h], ke[h], up[h], un[h], a.dt, a.abstol, a.reltol);
        v2[h] = lrnde::adams_phi1(k1[h], kp[h], a.b2);
      }
      if (a.s2) reinterpret_cast<f32x4*>(a.s2)[i] = v2;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      e0 += (double)lrnde::bs3_resid_sq(a.k1[i], a.kb2[i], a.kb3[i], a.kend[i], a.uprev[i], a.u[i], a.dt, a.abstol, a.reltol);
      if (a.s2) a.s2[i] = lrnde::adams_phi1(a.k1[i], a.kprev[i], a.b2);
    }
  }
  block_sum3(e0, z1, z2, a.part + (size_t)blockIdx.x * 3);
}

// An accepted step's record [uprev, k1, P2, P3] into its slot.  o0 / o1 null: no copy of uprev / k1 (a saveat point of a
// solve without a record reads them where they are).
struct CadRecArgs { const float *uprev, *u, *k1, *kend; float *o0, *o1, *P2, *P3; float dt; size_t n; int vec4; };
__global__ __launch_bounds__(256) void k_cadams_record(CadRecArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      const f32x4 up = CAD_V4(a.uprev), k1 = CAD_V4(a.k1), un = CAD_V4(a.u), ke = CAD_V4(a.kend);
      if (a.o0) { reinterpret_cast<f32x4*>(a.o0)[i] = up; reinterpret_cast<f32x4*>(a.o1)[i] = k1; }
      f32x4 p2, p3;
#pragma unroll
      for (int h = 0; h < 4; ++h) { float q2, q3; lrnde::adams_hermite(up[h], un[h], k1[h], ke[h], a.dt, q2, q3); p2[h] = q2; p3[h] = q3; }
      reinterpret_cast<f32x4*>(a.P2)[i] = p2; reinterpret_cast<f32x4*>(a.P3)[i] = p3;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) {
      const float up = a.uprev[i], k1 = a.k1[i];
      if (a.o0) { a.o0[i] = up; a.o1[i] = k1; }
      float q2, q3;
      lrnde::adams_hermite(up, a.u[i], k1, a.kend[i], a.dt, q2, q3);
      a.P2[i] = q2; a.P3[i] = q3;
    }
  }
}

// y(theta) of a Hermite record [y0, k1, P2, P3] (P4 = 0): tsit5_rec_eval's arithmetic
struct CadEvalArgs { const float *y0, *k1, *P2, *P3; float* out; float th, ddt; size_t n; int vec4; };
__global__ __launch_bounds__(256) void k_cadams_eval(CadEvalArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (a.vec4) {
    const size_t n4 = a.n / 4;
    for (size_t i = i0; i < n4; i += stride) {
      const f32x4 y0 = CAD_V4(a.y0), k1 = CAD_V4(a.k1), p2 = CAD_V4(a.P2), p3 = CAD_V4(a.P3);
      f32x4 r;
#pragma unroll
      for (int h = 0; h < 4; ++h) r[h] = lrnde::tsit5_rec_eval(y0[h], k1[h], p2[h], p3[h], 0.0f, a.th, a.ddt);
      reinterpret_cast<f32x4*>(a.out)[i] = r;
    }
  } else {
    for (size_t i = i0; i < a.n; i += stride) a.out[i] = lrnde::tsit5_rec_eval(a.y0[i], a.k1[i], a.P2[i], a.P3[i], 0.0f, a.th, a.ddt);
  }
}
#undef CAD_V4

// y(theta) of the Hermite slot d = [y0, k1, P2, P3] of n floats each (the recorded backward's state lookup)
int cad_eval(lrnde_conv* c, const float* d, size_t n, float th, float ddt, float* out) {
  CadEvalArgs e{};
  e.y0 = d; e.k1 = d + n; e.P2 = d + 2 * n; e.P3 = d + 3 * n; e.out = out; e.th = th; e.ddt = ddt; e.n = n;
  e.vec4 = cad_vec4(n, d, out) ? 1 : 0;
  hipLaunchKernelGGL(k_cadams_eval, dim3(cad_grid(n, e.vec4)), dim3(256), 0, c->stream, e);
  CHK(c, hipGetLastError());
  return LRNDE_OK;
}

// lrnde_conv_solve for c->solver_alg = 1 (VCAB3) | 2 (VCABM3), entered behind its argument checks and record bookkeeping:
// same arguments, same outputs, same side effects on the handle (save slots, rec.ts, trace rows, stats, the dense record when
// dense_on, stop codes through cfail)
int conv_adams_solve(lrnde_conv* c, const float* u0, int B, float t0, float t1, const lrnde_solve_opts* o, const float* saveat,
                     int nsave, float* u_saved, float* t_saved, int cap_saved, lrnde_stats* st, lrnde_trace_row* trace, int cap_trace) {
  int rc;
  const size_t n = state_n(c, B);
  const NormSpan sp = state_span(c, n);
  const bool moulton = c->solver_alg == LRNDE_ALG_VCABM3;
  const float abstol = o->abstol, reltol = o->reltol;
  float* V = c->vec;   // CAD_VECS vectors (ensure_ws)
  float *uprev = V, *u = V + n, *k1 = V + 2 * n, *kprev = V + 3 * n, *kend = V + 4 * n, *du = V + 5 * n, *sp2 = V + 6 * n, *s2 = V + 7 * n;
  float *s3 = V + 8 * n, *tmp = V + 9 * n, *kb2 = V + 10 * n, *kb3 = V + 11 * n, *P2s = V + 12 * n, *P3s = V + 13 * n;
  hipStream_t sq = c->stream;
  int nsaved = 0, isave = 0, ntrace = 0;
  // the next save slot (the Hermite evaluation writes into it directly); cap_saved is checked here
  auto slot = [&](float tt, float** dst) -> int {
    if (nsaved >= cap_saved || !u_saved) return cfail(c, LRNDE_CAPACITY, "u_saved capacity %d exhausted", cap_saved);
    *dst = u_saved + (size_t)nsaved * n;
    if (t_saved) t_saved[nsaved] = tt;
    c->rec.ts.push_back(tt);
    nsaved++;
    return LRNDE_OK;
  };
  auto push = [&](float tt, const float* uu) -> int {
    float* dst;
    const int r = slot(tt, &dst);
    if (r) return r;
    CHK(c, hipMemcpyAsync(dst, uu, sizeof(float) * n, hipMemcpyDeviceToDevice, sq));
    return LRNDE_OK;
  };
  // record slot idx of the forward record (8n floats, the Tsit5 record's size: a handle switched between solvers reuses it)
  auto dense_slot = [&](size_t idx, float** d) -> int {
    if (c->dense_n != n) { c->dense.clear(); c->dense_n = n; }
    while (idx >= c->dense.size()) { DevBuf<float> b; CHK(c, b.once(8 * n)); c->dense.push_back(std::move(b)); }
    *d = c->dense[idx];
    return LRNDE_OK;
  };
  auto rhs = [&](const float* x, float tt, float* k) { return launch_rhs(c, x, tt, B, k); };
  CHK(c, hipMemcpyAsync(uprev, u0, sizeof(float) * n, hipMemcpyDeviceToDevice, sq));
  float dt_init;
  if ((rc = init_dt_g(c, n, sp, rhs, uprev, t0, t1, abstol, reltol, k1, tmp, kb2, &dt_init, 3.0f))) return rc;   // k1 = f(u0, t0): fsalfirst
  st->nf = 3; st->dt_init = dt_init;
  AttemptLoop L = attempt_begin(pi_order3(), o->exact_pow, o->maxiters, 1, t0, t1, dt_init);
  const float &t = L.t, &dt = L.dt;
  float h1 = 0.0f, h2 = 0.0f;   // the last two accepted step sizes
  if (o->save_start && (rc = push(t0, uprev))) return rc;
  while (isave < nsave && saveat[isave] <= t0) ++isave;
  const float a21 = 0.5f, a32 = 0.75f;
  const float a4[3] = {(float)(2.0 / 9.0), (float)(1.0 / 3.0), (float)(4.0 / 9.0)};
  while (t < t1) {
    if (L.iter > 0 && L.accept) {
      std::swap(uprev, u);
      float* sw = kprev; kprev = k1; k1 = kend; kend = sw;   // phi*_0(n-1) <- f_n; fsalfirst <- fsallast
      std::swap(sp2, s2);                                    // phi*_1(n-1)
    }
    if (!attempt_header(L, t1)) break;
    const int nacc = st->naccept;
    const lrnde::AdamsCoef kc = lrnde::adams_coef(nacc, moulton ? 1 : 0, dt, h1, h2);
    double s[3];
    if (nacc < 2) {   // Bogacki-Shampine 3(2); lincomb's operation order is the oracle's for these sums
      const float c2s = dt * a21, c3s = dt * a32;
      const float* k_1[1] = {k1};
      if ((rc = lincomb(c, tmp, uprev, 0.f, 1, k_1, &c2s, n))) return rc;
      if ((rc = rhs(tmp, t + 0.5f * dt, kb2))) return rc;
      const float* k_2[1] = {kb2};
      if ((rc = lincomb(c, tmp, uprev, 0.f, 1, k_2, &c3s, n))) return rc;
      if ((rc = rhs(tmp, t + 0.75f * dt, kb3))) return rc;
      const float* k_3[3] = {k1, kb2, kb3};
      if ((rc = lincomb(c, u, uprev, dt, 3, k_3, a4, n))) return rc;
      if ((rc = rhs(u, t + dt, kend))) return rc;
      st->nf += 3;
      CadBs3Args e{};
      e.k1 = k1; e.kb2 = kb2; e.kb3 = kb3; e.kend = kend; e.uprev = uprev; e.u = u; e.kprev = kprev; e.s2 = nacc == 1 ? s2 : nullptr;
      e.b2 = kc.b2; e.dt = dt; e.abstol = abstol; e.reltol = reltol; e.n = sp.local; e.part = c->sums;
      e.vec4 = cad_vec4(n, k1, kb2, kb3, kend, uprev, u, kprev, s2) ? 1 : 0;
      hipLaunchKernelGGL(k_cadams_bs3, dim3(NSUMB), dim3(256), 0, sq, e);
      CHK(c, hipGetLastError());
    } else {
      CadPredArgs p{};
      p.uprev = uprev; p.k1 = k1; p.kprev = kprev; p.sp2 = sp2; p.s2 = s2; p.s3 = s3; p.u = u;
      p.k = kc; p.dt = dt; p.three = moulton ? 0 : 1; p.n = n;
      p.vec4 = cad_vec4(n, uprev, k1, kprev, sp2, s2, s3, u) ? 1 : 0;
      hipLaunchKernelGGL(k_cadams_pred, dim3(cad_grid(n, p.vec4)), dim3(256), 0, sq, p);
      CHK(c, hipGetLastError());
      float* dnew = moulton ? du : kend;   // VCAB3: the evaluation at the new state is fsallast itself
      if ((rc = rhs(u, t + dt, dnew))) return rc;
      st->nf += 1;
      CadResidArgs q{};
      q.du = dnew; q.k1 = k1; q.s2 = s2; q.s3 = s3; q.uprev = uprev; q.u = u;
      q.cu = kc.cu; q.ce = kc.ce; q.abstol = abstol; q.reltol = reltol; q.moulton = moulton ? 1 : 0;
      q.n = sp.local; q.part = c->sums;
      q.vec4 = cad_vec4(n, dnew, k1, s2, s3, uprev, u) ? 1 : 0;
      hipLaunchKernelGGL(k_cadams_resid, dim3(NSUMB), dim3(256), 0, sq, q);
      CHK(c, hipGetLastError());
      if (moulton) { if ((rc = rhs(u, t + dt, kend))) return rc; st->nf += 1; }   // fsallast at the corrected state
    }
    if ((rc = fetch_sums(c, s))) return rc;
    const float eest = (float)sqrt(s[0] / sp.global);
    st->eest_last = eest;
    const float tprev = t;
    const bool accept = attempt_judge(L, eest);
    if (L.status) break;  // a NaN estimate
    if (trace && ntrace < cap_trace) { trace[ntrace].t = tprev; trace[ntrace].dt = dt; trace[ntrace].eest = eest; trace[ntrace].accepted = accept; ++ntrace; }
    if (!accept) { st->nreject++; continue; }
    st->naccept++;
    h2 = h1; h1 = dt;
    bool need_poly = c->dense_on;
    for (int i = isave; i < nsave && saveat[i] <= t; ++i) if (saveat[i] != t) need_poly = true;
    const float *ry0 = uprev, *rk1 = k1, *rP2 = P2s, *rP3 = P3s;
    if (need_poly) {
      CadRecArgs r{};
      r.uprev = uprev; r.u = u; r.k1 = k1; r.kend = kend; r.P2 = P2s; r.P3 = P3s; r.dt = dt; r.n = n;
      if (c->dense_on) {
        float* d;
        if ((rc = dense_slot((size_t)nacc, &d))) return rc;
        r.o0 = d; r.o1 = d + n; r.P2 = d + 2 * n; r.P3 = d + 3 * n;
        ry0 = d; rk1 = d + n; rP2 = r.P2; rP3 = r.P3;
        c->dense_t.push_back(tprev); c->dense_dt.push_back(dt);
      }
      r.vec4 = cad_vec4(n, uprev, u, k1, kend, r.o0, r.P2) ? 1 : 0;
      hipLaunchKernelGGL(k_cadams_record, dim3(cad_grid(n, r.vec4)), dim3(256), 0, sq, r);
      CHK(c, hipGetLastError());
    }
    while (isave < nsave && saveat[isave] <= t) {  // savevalues!
      const float tsv = saveat[isave++];
      if (tsv != t) {
        float* dst;
        if ((rc = slot(tsv, &dst))) return rc;
        CadEvalArgs e{};
        e.y0 = ry0; e.k1 = rk1; e.P2 = rP2; e.P3 = rP3; e.out = dst; e.th = (tsv - tprev) / dt; e.ddt = dt; e.n = n;
        e.vec4 = cad_vec4(n, ry0, rk1, rP2, rP3, dst) ? 1 : 0;
        hipLaunchKernelGGL(k_cadams_eval, dim3(cad_grid(n, e.vec4)), dim3(256), 0, sq, e);
        CHK(c, hipGetLastError());
      } else if ((rc = push(t, u))) return rc;
    }
    if (o->save_everystep && (rc = push(t, u))) return rc;
  }
  CHK(c, hipStreamSynchronize(sq));
  rc = L.status;
  st->retcode = rc; st->iters = L.iter; st->nsaved = nsaved; st->t_final = t; st->dt_final = dt;
  if (rc) return cfail(c, rc, "solve stopped with retcode %d at t=%g (dt=%g, %d iterations)", rc, (double)t, (double)dt, L.iter);
  return LRNDE_OK;
}

// lrnde_chain_adams.hpp — VCAB3 / VCABM3 on the small Dense-chain handle as ONE launch per attempted step, the controller
// on the device.  Included by lrnde_kernels.hip inside its anonymous namespace, behind lrnde_chain.hpp (whose frame it
// uses: 8 columns per 512-thread workgroup, the forward weight image in LDS for the launch, chain_slots ownership,
// chain_feval, block_sum3 / publish_partial) and the step prologue's helpers (Bcast, CtrlHead, solve_progress).
//
// The algorithm, its constants and its operation order are adams_solve's (lrnde_adams.hpp: the host-driven loop, kept as the
// same-bits comparison path behind LRNDE_ADAMS_HOST=1, and the oracle's adams_solve).  What differs is where things live:
//
//   host loop                         this kernel (cur = parity of the accepted steps, as in k_step_chain)
//   uprev, u                          ubuf[cur], ubuf[cur^1]
//   k1, kend                          kfsal[cur], kfsal[cur^1]
//   kprev                             kfsal[cur^1] UNTIL this attempt's kend overwrites it: the first attempt after an accept
//                                     (AdamsBcast::fresh) forms p2 = k1 - kprev and keeps it in ks[0]; a retry reads ks[0]
//                                     (p2 does not depend on dt)
//   sp2, s2                           ks[1 + cur], ks[1 + (cur^1)]: an accept flips cur and s2 becomes sp2; a retry rewrites
//                                     its s2 and finds sp2 untouched
//   s3, du, kb2, kb3, tmp, P2, P3     registers of the thread that owns the element
//   h1, h2 (last two accepted dt)     AdamsChainArgs::hh, double-buffered by launch parity beside the control blocks
//
// A rejected attempt therefore leaves intact all the retry reads: uprev and k1 (never written), p2 (ks[0]), sp2.  Every
// array is read and written only at the elements the thread owns (chain_slots; the footer's loop visits the same elements),
// so the footer of the previous accepted step — which reads the arrays this attempt overwrites — needs no barrier.
//
// Launch j: wave 0 judges attempt j-1 from its partial sums (adams_prologue: lrnde_stepctl.hpp's pieces in attempt_header /
// attempt_judge's order, snap_magnitude, pi_order3), every thread then performs the accepted step's saves (cubic Hermite in
// the record's polynomial form, lrnde_adams.hpp) and dense record slot, then the attempt itself: a Bogacki-Shampine 3(2)
// step while fewer than two steps are accepted (three evaluations), else the multistep step (one evaluation, two for
// VCABM3).  It plugs into solve_impl's feed loop as k_step_chain does: same reports, same speculative launches.

struct AdamsChainArgs {
  float* hh;     // [2][2]: (h1, h2) per launch parity
  int moulton;   // 0 VCAB3, 1 VCABM3
};

struct AdamsBcast {
  Bcast b;       // do_step, cur, t, dt and the footer's fields (store_k / dense_slot are not used here)
  int phase;     // 0: start-up attempt (naccept == 0); 1: start-up attempt that leaves s2 (naccept == 1); 2: multistep
  int fresh;     // first attempt after an accept: p2 is formed from kfsal[cur^1] and stored; 0: a retry reads it
  float b2, b3, g2, g3, cu, ce;
};

static size_t adams_chain_smem_bytes(int wfloats) { return chain_smem_bytes(wfloats) + sizeof(AdamsBcast); }

// wave 0 of every workgroup, identical inputs; workgroup 0 publishes the next control block
__device__ __forceinline__ void adams_prologue(const StepArgs& a, const AdamsChainArgs& aa, int j, AdamsBcast* out) {
  const int lane = threadIdx.x & 63;
  CtrlHead c = *reinterpret_cast<const CtrlHead*>(a.ctrl + (j & 1));
  CtrlHead* cout = reinterpret_cast<CtrlHead*>(a.ctrl + ((j + 1) & 1));
  const double* ppart = a.part_recv + (size_t)(j & 1) * a.nwg_global * PSTRIDE;
  PartLoads pl;
  part_issue<false>(pl, ppart, a.nwg_global);
  AdamsBcast ab;
  Bcast& b = ab.b;
  memset(&ab, 0, sizeof(ab));
  b.dense_idx = -1; b.dense_slot = -1;
  if (c.status != ST_RUNNING) {
    if (blockIdx.x == 0 && lane == 0) { *cout = c; solve_progress(a, j, c, c.nsaved, 0.f); }
    if (lane == 0) *out = ab;
    return;
  }
  const PiConsts pi = pi_order3();
  const float dtmax = a.t1 - a.t0;
  const float dtmin = fmaxf_(eps_f(a.t1), eps_f(a.t0));
  float h1 = 0.f, h2 = 0.f;
  if (!c.first) { h1 = aa.hh[2 * (j & 1)]; h2 = aa.hh[2 * (j & 1) + 1]; }
  int accepted = 0, do_step = 0;
  float t = c.t, dt = c.dt;
  b.cur_prev = c.cur; b.isave0 = c.isave; b.isave1 = c.isave; b.nsaved0 = c.nsaved;
  b.t_new = c.t; b.tprev = c.t; b.dt_prev = c.dt;

  if (c.first) {
    // ode_determine_initdt with order 3 from the sums of k_init1_chain / k_init2_chain
    const Sum3 r1 = reduce_partials3(a.pinit_recv, a.nwg_global);
    const Sum3 r2 = reduce_partials3(a.pinit_recv + (size_t)a.nwg_global * PSTRIDE, a.nwg_global);
    dt = init_dt_final3(r1, r2, a.n_global, dtmax, 3.0f);
    c.nf = 3;
    c.dt_init = dt;
    c.dtpropose = dt;
  } else {
    const Sum3 sr = part_finish<false>(pl, ppart, a.nwg_global);
    const float eest = rms_from(sr.a, a.n_global);
    c.eest_last = eest;
    if (eest != eest) {  // attempt_judge: a NaN estimate stops the loop before the controller runs (no trace row)
      c.status = LRNDE_DT_NAN;
    } else {
      const PiStep ps = pi_step(pi, a.exact_pow, eest, pi_pow(a.exact_pow, c.qold, pi.beta2), c.q11);
      c.q11 = ps.q11;
      accepted = (eest <= 1.0f);
      const int ntr = c.naccept + c.nreject;
      if (blockIdx.x == 0 && lane == 0 && a.trace && ntr < a.cap_trace) {
        lrnde_trace_row r; r.t = c.t; r.dt = c.dt; r.eest = eest; r.accepted = accepted;
        a.trace[ntr] = r;
      }
      if (accepted) {
        c.naccept++;
        c.qold = pi_qold(eest);
        b.tprev = c.t; b.dt_prev = c.dt;
        t = snap_magnitude(c.t, c.dt, a.t1);
        c.dtpropose = pi_propose(c.dt, ps.q, dtmax, dt_floor(t, dtmin));
        h2 = h1; h1 = c.dt;
        b.accepted_prev = 1; b.t_new = t;
        if (a.dense) {
          b.dense_idx = c.naccept - 1;
          if (b.dense_idx >= a.dense_cap) { c.status = LRNDE_CAPACITY; b.accepted_prev = 0; b.dense_idx = -1; }
        }
        // savevalues!: count what this step saves (performed by all threads afterwards)
        int is = c.isave, ns = c.nsaved;
        while (is < a.nsave && a.saveat[is] <= t) { ++is; ++ns; }
        if (a.save_everystep) ++ns;
        if (ns > a.cap_saved) c.status = LRNDE_CAPACITY, b.accepted_prev = 0;
        else { c.isave = is; c.nsaved = ns; b.isave1 = is; }
      } else {
        c.nreject++;
      }
    }
  }

  if (c.status == ST_RUNNING) {
    if (!(t < a.t1)) {
      c.status = ST_DONE;
    } else {  // attempt_header
      if (!c.first) {
        if (accepted) { c.cur ^= 1; dt = c.dtpropose; }
        else dt = pi_reject_dt(pi, c.dt, c.q11);
      }
      c.iter++;
      dt = header_clamp(dt, dtmax, dtmin, t, a.t1);
      const int hs = header_status(c.iter, a.maxiters, dt, dtmin);
      if (hs != STEP_OK) c.status = hs;
      else { do_step = 1; c.nf += c.naccept < 2 ? 3 : (aa.moulton ? 2 : 1); }
    }
  }
  c.t = t; c.dt = dt; c.first = 0;
  b.do_step = do_step; b.cur = c.cur; b.t = t; b.dt = dt;
  // the attempt's scalars (adams_solve's recurrences: phi*_1, phi*_2 factors, g_2..g_4)
  const int nacc = c.naccept;
  ab.phase = nacc < 2 ? nacc : 2;
  ab.fresh = accepted;
  if (do_step) {
    const lrnde::AdamsCoef kc = lrnde::adams_coef(nacc, aa.moulton, dt, h1, h2);   // lrnde_adams_math.hpp
    ab.b2 = kc.b2; ab.b3 = kc.b3; ab.g2 = kc.g2; ab.g3 = kc.g3; ab.cu = kc.cu; ab.ce = kc.ce;
  }
  if (lane == 0) {
    *out = ab;
    if (blockIdx.x == 0) {
      *cout = c;
      aa.hh[2 * ((j + 1) & 1)] = h1; aa.hh[2 * ((j + 1) & 1) + 1] = h2;
      solve_progress(a, j, c, b.nsaved0, (do_step && dt > 0.f) ? (a.t1 - t) / dt : 0.f);
    }
  }
}

// SPEC only changes the kernel's name (a launch enqueued beyond what the last report makes certain)
template <bool SPEC> __global__ __launch_bounds__(NT) void k_adams_chain(StepArgs a, ChainDev cd, AdamsChainArgs aa, int j) {
  const ChainSmem s = chain_carve(cd);
  AdamsBcast* sbc = reinterpret_cast<AdamsBcast*>(s.bc);
  chain_load_weights(cd, s.w);
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const int D = cd.D;
  if (threadIdx.x < 64) adams_prologue(a, aa, j, sbc);
  __syncthreads();
  const AdamsBcast ab = *sbc;
  const Bcast& bc = ab.b;
  auto each = [&](auto fn) {  // every real element of the tile, as (global offset): the elements chain_slots gives this thread
    for (int e = threadIdx.x; e < nvalid * D; e += NT) fn((size_t)b0 * D + e);
  };

  // savevalues! of the step accepted by the prologue: the cubic Hermite interpolant on (uprev, k1, u, kend) in the record's
  // polynomial form (k_adams_hermite + k_adams_eval), a point at the new time as a copy of u; the dense record slot
  if (bc.accepted_prev) {
    const float* up = ubuf_at(a, bc.cur_prev);
    const float* un = ubuf_at(a, bc.cur_prev ^ 1);
    const float* k1p = kfsal_at(a, bc.cur_prev);
    const float* kep = kfsal_at(a, bc.cur_prev ^ 1);
    const float ddt = bc.dt_prev;
    auto poly = [&](size_t g, float& P2, float& P3) {
      const float d = (un[g] - up[g]) / ddt;
      const float k1 = k1p[g], ke = kep[g];
      P2 = (3.0f * d - 2.0f * k1) - ke;
      P3 = (k1 + ke) - 2.0f * d;
    };
    int slot = bc.nsaved0;
    for (int is = bc.isave0; is < bc.isave1; ++is, ++slot) {
      const float ts = a.saveat[is];
      float* dst = a.u_saved + (size_t)slot * a.B * D;
      float* dst2 = slot == a.also_slot ? a.also_dst : nullptr;
      if (ts != bc.t_new) {
        const float theta = (ts - bc.tprev) / ddt;
        each([&](size_t g) {
          float P2, P3;
          poly(g, P2, P3);
          const float o = tsit5_rec_eval(up[g], k1p[g], P2, P3, 0.0f, theta, ddt);
          dst[g] = o;
          if (dst2) dst2[g] = o;
        });
      } else {
        each([&](size_t g) { const float o = un[g]; dst[g] = o; if (dst2) dst2[g] = o; });
      }
      if (blockIdx.x == 0 && threadIdx.x == 0) a.t_saved[slot] = ts;
    }
    if (a.save_everystep) {
      float* dst = a.u_saved + (size_t)slot * a.B * D;
      each([&](size_t g) { dst[g] = un[g]; });
      if (blockIdx.x == 0 && threadIdx.x == 0) a.t_saved[slot] = bc.t_new;
    }
    if (bc.dense_idx >= 0) {  // [uprev, k1, P2, P3, 0]
      const size_t nst = (size_t)a.n_local;
      float* dd = a.dense + (size_t)bc.dense_idx * REC_ARRAYS * nst;
      each([&](size_t g) {
        float P2, P3;
        poly(g, P2, P3);
        dd[g] = up[g]; dd[nst + g] = k1p[g];
        dd[2 * nst + g] = P2; dd[3 * nst + g] = P3; dd[4 * nst + g] = 0.0f;
      });
      if (blockIdx.x == 0 && threadIdx.x == 0) { a.dense_t[bc.dense_idx] = bc.tprev; a.dense_dt[bc.dense_idx] = ddt; }
    }
  }
  if (!bc.do_step) return;

  const float t = bc.t, dt = bc.dt;
  const float* uprev = ubuf_at(a, bc.cur);
  float* unew = ubuf_at(a, bc.cur ^ 1);
  const float* k1g = kfsal_at(a, bc.cur);
  float* kendg = kfsal_at(a, bc.cur ^ 1);   // holds kprev until this attempt's last store
  float* p2g = a.ks[0];
  const float* sp2g = a.ks[1 + bc.cur];
  float* s2g = a.ks[1 + (bc.cur ^ 1)];
  const ChainSlots sl = chain_slots(D, b0, nvalid);
  float up[CEPT], k1[CEPT], un[CEPT], ke[CEPT];
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    up[i] = sl.valid[i] ? uprev[sl.g[i]] : 0.f;
    k1[i] = sl.valid[i] ? k1g[sl.g[i]] : 0.f;
    un[i] = 0.f; ke[i] = 0.f;
  }
  // f(x, ts) of the tile -> out[]: the input activation into xa, chain_feval (the bits of k_rhs_chain)
  auto feval = [&](const float* x, float ts, float* out) {
#pragma unroll
    for (int i = 0; i < CEPT; ++i)
      if (sl.in[i]) s.xa[sl.lidx[i]] = sl.valid[i] ? act_apply(cd.in_act, x[i]) : 0.f;
    __syncthreads();
    const float* r = chain_feval(cd, s.w, s.xa, s.xb, ts);
#pragma unroll
    for (int i = 0; i < CEPT; ++i) out[i] = sl.in[i] ? r[sl.lidx[i]] : 0.f;
  };
  // p2 = k1 - kprev of the owned elements (see the file head)
  auto load_p2 = [&](float* p2) {
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      p2[i] = 0.f;
      if (!sl.valid[i]) continue;
      if (ab.fresh) { p2[i] = k1[i] - kendg[sl.g[i]]; p2g[sl.g[i]] = p2[i]; }
      else p2[i] = p2g[sl.g[i]];
    }
  };

  double aerr = 0.0, az1 = 0.0, az2 = 0.0;
  if (ab.phase < 2) {
    // Bogacki-Shampine 3(2): k_axpy's order for the sums (one term: uprev + (dt*a)*k; several: uprev + dt*(left to right))
    const float a21 = 0.5f, a32 = 0.75f;
    const float a41 = (float)(2.0 / 9.0), a42 = (float)(1.0 / 3.0), a43 = (float)(4.0 / 9.0);
    const float bt1 = (float)(5.0 / 72.0), bt2 = (float)(-1.0 / 12.0), bt3 = (float)(-1.0 / 9.0), bt4 = 0.125f;
    float x[CEPT], kb2[CEPT], kb3[CEPT];
    const float c2s = dt * a21;
#pragma unroll
    for (int i = 0; i < CEPT; ++i) x[i] = up[i] + c2s * k1[i];
    feval(x, t + 0.5f * dt, kb2);
    const float c3s = dt * a32;
#pragma unroll
    for (int i = 0; i < CEPT; ++i) x[i] = up[i] + c3s * kb2[i];
    feval(x, t + 0.75f * dt, kb3);
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      float sm = a41 * k1[i] + a42 * kb2[i];
      sm = sm + a43 * kb3[i];
      un[i] = up[i] + dt * sm;
    }
    feval(un, t + dt, ke);
    if (ab.phase == 1) {  // phi*_1 for the first multistep step
      float p2[CEPT];
      load_p2(p2);
#pragma unroll
      for (int i = 0; i < CEPT; ++i)
        if (sl.valid[i]) s2g[sl.g[i]] = ab.b2 * p2[i];
    }
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      if (!sl.valid[i]) continue;
      float sm = bt1 * k1[i] + bt2 * kb2[i];
      sm = sm + bt3 * kb3[i];
      sm = sm + bt4 * ke[i];
      const float ut = dt * sm;
      const float sc = a.abstol + fmaxf_(__builtin_fabsf(up[i]), __builtin_fabsf(un[i])) * a.reltol;
      const float r = ut / sc;
      const float sq = r * r;
      aerr += (double)sq;
    }
  } else {
    // k_adams_pre: phi*_1, phi*_2 and the predictor
    float p2[CEPT], v2[CEPT], v3[CEPT], du[CEPT];
    load_p2(p2);
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      const float sp2 = sl.valid[i] ? sp2g[sl.g[i]] : 0.f;
      v2[i] = ab.b2 * p2[i];
      const float p3 = p2[i] - sp2;
      v3[i] = ab.b3 * p3;
      if (sl.valid[i]) s2g[sl.g[i]] = v2[i];
      float sm = k1[i] + ab.g2 * v2[i];
      if (!aa.moulton) sm = sm + ab.g3 * v3[i];
      un[i] = up[i] + dt * sm;
    }
    feval(un, t + dt, du);
    // k_adams_post: phi_j(n+1), the corrector (VCABM3), the residual
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      if (!sl.valid[i]) continue;
      const float q2 = du[i] - k1[i];
      const float q3 = q2 - v2[i];
      const float q4 = q3 - v3[i];
      if (aa.moulton) un[i] = un[i] + ab.cu * q3;
      const float ut = ab.ce * q4;
      const float sc = a.abstol + fmaxf_(__builtin_fabsf(up[i]), __builtin_fabsf(un[i])) * a.reltol;
      const float r = ut / sc;
      const float sq = r * r;
      aerr += (double)sq;
    }
    if (aa.moulton) {
      feval(un, t + dt, ke);   // fsallast at the corrected state
    } else {
#pragma unroll
      for (int i = 0; i < CEPT; ++i) ke[i] = du[i];   // VCAB3: the evaluation at the new state is fsallast itself
    }
  }
#pragma unroll
  for (int i = 0; i < CEPT; ++i)
    if (sl.valid[i]) { unew[sl.g[i]] = un[i]; kendg[sl.g[i]] = ke[i]; }
  block_sum3(s.red, aerr, az1, az2);
  publish_partial(a, (j + 1) & 1, aerr, 0.0, 0.0);
}

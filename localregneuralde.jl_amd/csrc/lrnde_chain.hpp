// lrnde_chain.hpp — the small Dense-chain vector field (lrnde_create_chain), included by lrnde_kernels.hip inside its
// anonymous namespace, behind the step prologue, the partial-sum protocol and the backward helpers it reuses.
//
//   Chain(act0.(u), Dense(d0 => d1, a1), ..., Dense(d(L-1) => dL, aL))  or  TDChain(Chain(Dense..)),  d0 = dL = D,
//   every width <= 128, L <= 16.
//
// Tile: CNB = 8 batch columns per workgroup of NT = 512 threads.  A column of the tile is its D contiguous floats of the
// (D x B) state, so the tile is the contiguous run [b0*D, (b0+nvalid)*D) and thread slot i holds element
// e = threadIdx.x + i*NT of it (row e % D, column e / D).  Activations live in LDS as [row][CNB].
//
// Layer arithmetic (the canonical order of this field, the same in every kernel here): thread (o-pair, n) computes
//   z[o][n] = ((fma chain over k = 0..in-1 of W[o][k] * x[k][n], from 0) (fma W[o][in] * t, TDChain)) + b[o],
// then h = act(z) (lrnde_math.hpp act_apply).  Nothing depends on which workgroup holds a column, or on B.
//
// Step kernel: the forward weight image (per layer rows k = 0..in-1, the t row, the bias row; outp = out rounded up to
// even floats per row) is copied to LDS once per launch and stays there; the six stage evaluations, the stage sums, the
// error / stiffness partials and the dense record run inside the launch; k1..k7 of a column stay in the registers of the
// threads that own its elements.  k2..k6 reach global memory only when the prologue asks for them (Bcast::store_k).
//
// VJP: the forward pass keeps every layer's input and act' in LDS, the backward pass reads W row-major from the
// backward image (global, L2-resident); the parameter cotangent of the tile (sum over its columns in column order) is
// a per-workgroup partial vector, summed over the workgroups in workgroup order by k_chain_pgsum.

constexpr int CNB = 8;                  // batch columns per workgroup
constexpr int CMAXW = 128;              // widest layer (LRNDE_CHAIN_MAX_WIDTH)
constexpr int CEPT = CMAXW * CNB / NT;  // state elements per thread
constexpr int CMETA = 10;               // ints per layer in the layer table
static_assert(CEPT * NT == CMAXW * CNB && CNB == 8 && NT == 512, "thread (o-pair, n) map: 64 row pairs x 8 columns");

// per layer: in, out, outp, act, woff (forward image), goff (backward image), poff (flat Lux vector), aoff (VJP: layer
// input in LDS), zoff (VJP: act' in LDS), 0
enum { CM_IN, CM_OUT, CM_OUTP, CM_ACT, CM_WOFF, CM_GOFF, CM_POFF, CM_AOFF, CM_ZOFF };

struct ChainDev {
  int L, td, in_act, D;
  int wfloats;       // floats of the forward image (a multiple of 4)
  int P;             // parameter count
  int uoff, gboff;   // VJP LDS: input act' [D][CNB], then the two cotangent buffers [CMAXW][CNB]
  const int* meta;   // [L][CMETA] (device)
  const float* wf;   // forward image
  const float* wg;   // backward image: per layer W[o][k] row-major (out x in), the state columns only
};

struct ChainSmem { float* w; float* xa; float* xb; double* red; Bcast* bc; };
__device__ __forceinline__ ChainSmem chain_carve(const ChainDev& cd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ChainSmem s;
  s.w = reinterpret_cast<float*>(smem);
  s.xa = s.w + cd.wfloats;
  s.xb = s.xa + CMAXW * CNB;
  s.red = reinterpret_cast<double*>(s.xb + CMAXW * CNB);
  s.bc = reinterpret_cast<Bcast*>(s.red + NW * 3);
  return s;
}
static size_t chain_smem_bytes(int wfloats) {
  return ((size_t)wfloats + 2 * (size_t)CMAXW * CNB) * sizeof(float) + NW * 3 * sizeof(double) + sizeof(Bcast) + 16;
}

__device__ __forceinline__ void chain_load_weights(const ChainDev& cd, float* w) {
  const f32x4* src = reinterpret_cast<const f32x4*>(cd.wf);
  f32x4* dst = reinterpret_cast<f32x4*>(w);
  for (int i = threadIdx.x; i < cd.wfloats / 4; i += NT) dst[i] = src[i];
}

// one Dense layer on the tile (see the file head for the order); dact (optional): act'(z) in the layout of xout
__device__ __forceinline__ void chain_layer(const float* W, int in, int out, int outp, int td, int act, const float* xin,
                                            float* xout, float* dact, float t) {
  const int n = threadIdx.x & (CNB - 1), o0 = (threadIdx.x >> 3) * 2;
  if (o0 >= out) return;
  const float* wp = W + o0;
  float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
  for (int k = 0; k < in; ++k) {
    const float x = xin[k * CNB + n];
    const float2 w = *reinterpret_cast<const float2*>(wp + (size_t)k * outp);
    a0 = fma_(w.x, x, a0);
    a1 = fma_(w.y, x, a1);
  }
  int kb = in;
  if (td) {
    const float2 w = *reinterpret_cast<const float2*>(wp + (size_t)in * outp);
    a0 = fma_(w.x, t, a0);
    a1 = fma_(w.y, t, a1);
    kb = in + 1;
  }
  const float2 b = *reinterpret_cast<const float2*>(wp + (size_t)kb * outp);
  a0 = a0 + b.x;
  a1 = a1 + b.y;
  const float h0 = act_apply(act, a0), h1 = act_apply(act, a1);
  xout[o0 * CNB + n] = h0;
  if (dact) dact[o0 * CNB + n] = act_deriv_c(act, a0, h0);
  if (o0 + 1 < out) {
    xout[(o0 + 1) * CNB + n] = h1;
    if (dact) dact[(o0 + 1) * CNB + n] = act_deriv_c(act, a1, h1);
  }
}

// the whole chain on the tile staged in xa (input activation already applied); returns the buffer holding f
__device__ __forceinline__ const float* chain_feval(const ChainDev& cd, const float* W, float* xa, float* xb, float t) {
  float* src = xa;
  float* dst = xb;
  for (int l = 0; l < cd.L; ++l) {
    const int* mt = cd.meta + l * CMETA;
    chain_layer(W + mt[CM_WOFF], mt[CM_IN], mt[CM_OUT], mt[CM_OUTP], cd.td, mt[CM_ACT], src, dst, nullptr, t);
    __syncthreads();
    float* tmp = src; src = dst; dst = tmp;
  }
  return src;
}

// the thread's element slots of the tile: LDS index, global offset, in the tile / in a real column
struct ChainSlots { int lidx[CEPT]; size_t g[CEPT]; bool in[CEPT], valid[CEPT]; };
__device__ __forceinline__ ChainSlots chain_slots(int D, int b0, int nvalid) {
  ChainSlots s;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    const int e = threadIdx.x + i * NT;
    s.in[i] = e < D * CNB;
    s.valid[i] = e < D * nvalid;
    s.lidx[i] = s.in[i] ? (e % D) * CNB + e / D : 0;
    s.g[i] = (size_t)b0 * D + e;
  }
  return s;
}

// f(u, t) -> out for the tile (xa receives act0.(u))
__device__ __forceinline__ void chain_eval_tile(const ChainDev& cd, const ChainSmem& s, const ChainSlots& sl, const float* u,
                                                float t, float* out, float* regs) {
#pragma unroll
  for (int i = 0; i < CEPT; ++i)
    if (sl.in[i]) s.xa[sl.lidx[i]] = sl.valid[i] ? act_apply(cd.in_act, u[sl.g[i]]) : 0.f;
  __syncthreads();
  const float* r = chain_feval(cd, s.w, s.xa, s.xb, t);
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    const float v = sl.in[i] ? r[sl.lidx[i]] : 0.f;
    if (regs) regs[i] = v;
    if (out && sl.valid[i]) out[sl.g[i]] = v;
  }
}

// du = f(u, t) for the whole batch (lrnde_rhs)
__global__ __launch_bounds__(NT) void k_rhs_chain(ChainDev cd, int B, const float* u, float t, float* du) {
  const ChainSmem s = chain_carve(cd);
  chain_load_weights(cd, s.w);
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, B - b0);
  const ChainSlots sl = chain_slots(cd.D, b0, nvalid);
  chain_eval_tile(cd, s, sl, u, t, du, nullptr);
}

// init phase 1 (k_init1's protocol): f0 = f(u0, t0) -> k1; partial sums of (u0/sk)^2 and (f0/sk)^2
__global__ __launch_bounds__(NT) void k_init1_chain(StepArgs a, ChainDev cd) {
  const ChainSmem s = chain_carve(cd);
  chain_load_weights(cd, s.w);
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const ChainSlots sl = chain_slots(cd.D, b0, nvalid);
  const Ctrl c = a.ctrl[0];
  const float* u0 = ubuf_at(a, c.cur);
  float* f0 = kfsal_at(a, c.cur);
  float f[CEPT];
  chain_eval_tile(cd, s, sl, u0, c.t, f0, f);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    if (!sl.valid[i]) continue;
    const float u = u0[sl.g[i]];
    const float sk = a.abstol + __builtin_fabsf(u) * a.reltol;
    const float r0 = u / sk, r1 = f[i] / sk;
    const float q0 = r0 * r0, q1 = r1 * r1;
    a0 += (double)q0; a1 += (double)q1;
  }
  block_sum3(s.red, a0, a1, a2);
  publish_partial(a, 2, a0, a1, 0.0);
}

// init phase 2: u1 = u0 + dt0*f0, f1 = f(u1, t0+dt0) -> ks[0]; partial sum of ((f1-f0)/sk)^2
__global__ __launch_bounds__(NT) void k_init2_chain(StepArgs a, ChainDev cd) {
  const ChainSmem s = chain_carve(cd);
  chain_load_weights(cd, s.w);
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const ChainSlots sl = chain_slots(cd.D, b0, nvalid);
  const Ctrl c = a.ctrl[0];
  if (threadIdx.x < 64) {
    double s1[3];
    reduce_partials(a.pinit_recv, a.nwg_global, s1);
    if (threadIdx.x == 0) s.bc->dt0 = init_dt0(s1, a.n_global, a.t1 - a.t0);
  }
  __syncthreads();
  const float dt0 = s.bc->dt0;
  const float* u0 = ubuf_at(a, c.cur);
  const float* f0 = kfsal_at(a, c.cur);
  float uu[CEPT], ff[CEPT];
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    uu[i] = sl.valid[i] ? u0[sl.g[i]] : 0.f;
    ff[i] = sl.valid[i] ? f0[sl.g[i]] : 0.f;
    if (sl.in[i]) s.xa[sl.lidx[i]] = sl.valid[i] ? act_apply(cd.in_act, uu[i] + dt0 * ff[i]) : 0.f;
  }
  __syncthreads();
  const float* r = chain_feval(cd, s.w, s.xa, s.xb, c.t + dt0);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    if (!sl.valid[i]) continue;
    const float f1 = r[sl.lidx[i]];
    a.ks[0][sl.g[i]] = f1;
    const float sk = a.abstol + __builtin_fabsf(uu[i]) * a.reltol;
    const float r2 = (f1 - ff[i]) / sk;
    const float q2 = r2 * r2;
    a0 += (double)q2;
  }
  block_sum3(s.red, a0, a1, a2);
  publish_partial(a, 3, a0, 0.0, 0.0);
}

// one attempted Tsit5 step (src/perform_step.jl:3-47) of the whole batch, preceded by the device-side footer of the
// previous attempt and header of this one (step_prologue, as k_step / k_step_q).  SPEC only changes the kernel's name.
template <bool SPEC> __global__ __launch_bounds__(NT) void k_step_chain(StepArgs a, ChainDev cd, int j) {
  const ChainSmem s = chain_carve(cd);
  chain_load_weights(cd, s.w);
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const int D = cd.D;
  if (threadIdx.x < 64) step_prologue(a, j, s.bc);
  __syncthreads();
  const Bcast bc = *s.bc;
  auto each = [&](auto fn) {  // every real element of the tile, as (global offset)
    for (int e = threadIdx.x; e < nvalid * D; e += NT) fn((size_t)b0 * D + e);
  };

  // savevalues! of the step accepted by the prologue (Tsit5 dense output / copy) and its dense record
  if (bc.accepted_prev) {
    const float* up = ubuf_at(a, bc.cur_prev);
    const float* un = ubuf_at(a, bc.cur_prev ^ 1);
    const float* k1p = kfsal_at(a, bc.cur_prev);
    const float* k7p = kfsal_at(a, bc.cur_prev ^ 1);
    int slot = bc.nsaved0;
    for (int is = bc.isave0; is < bc.isave1; ++is, ++slot) {
      const float ts = a.saveat[is];
      float* dst = a.u_saved + (size_t)slot * a.B * D;
      float* dst2 = slot == a.also_slot ? a.also_dst : nullptr;
      if (ts != bc.t_new) {
        const float theta = (ts - bc.tprev) / bc.dt_prev;
        float bw[7];
        tsit5_bweights(theta, bw);
        each([&](size_t g) {
          float sum = k1p[g] * bw[0] + a.ks[0][g] * bw[1];
          sum = sum + a.ks[1][g] * bw[2];
          sum = sum + a.ks[2][g] * bw[3];
          sum = sum + a.ks[3][g] * bw[4];
          sum = sum + a.ks[4][g] * bw[5];
          sum = sum + k7p[g] * bw[6];
          const float o = up[g] + bc.dt_prev * sum;
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
    if (bc.dense_idx >= 0) {  // dense record [uprev, k1, P2, P3, P4] of the accepted step (lrnde_math.hpp tsit5_rec_poly)
      const size_t nst = (size_t)a.n_local;
      float* dd = a.dense + (size_t)bc.dense_idx * REC_ARRAYS * nst;
      each([&](size_t g) {
        const float kk[6] = {a.ks[0][g], a.ks[1][g], a.ks[2][g], a.ks[3][g], a.ks[4][g], k7p[g]};
        float P[3];
        tsit5_rec_poly(k1p[g], kk, P);
        dd[g] = up[g]; dd[nst + g] = k1p[g];
        dd[2 * nst + g] = P[0]; dd[3 * nst + g] = P[1]; dd[4 * nst + g] = P[2];
      });
      if (blockIdx.x == 0 && threadIdx.x == 0) { a.dense_t[bc.dense_idx] = bc.tprev; a.dense_dt[bc.dense_idx] = bc.dt_prev; }
    }
  }
  if (!bc.do_step) return;

  const float t = bc.t, dt = bc.dt;
  const float* uprev = ubuf_at(a, bc.cur);
  float* unew = ubuf_at(a, bc.cur ^ 1);
  const float* k1 = kfsal_at(a, bc.cur);
  float* k7 = kfsal_at(a, bc.cur ^ 1);
  const ChainSlots sl = chain_slots(D, b0, nvalid);
  float up[CEPT], un[CEPT], g6[CEPT], kr[7][CEPT];
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    up[i] = sl.valid[i] ? uprev[sl.g[i]] : 0.f;
    kr[0][i] = sl.valid[i] ? k1[sl.g[i]] : 0.f;
    un[i] = 0.f; g6[i] = 0.f;
  }
  // stage S: its input from uprev and k1..k(S-1) (stage_value: src/perform_step.jl:11-18), f of it -> k_S
#define LRNDE_CHAIN_STAGE(S, TS)                                                                        \
  do {                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                                  \
      float kv[S - 1];                                                                                  \
      _Pragma("unroll") for (int q = 0; q < S - 1; ++q) kv[q] = kr[q][i];                               \
      const float x = stage_value<S>(up[i], kv, dt);                                                    \
      if (S == 6) g6[i] = x;                                                                            \
      if (S == 7) un[i] = x;                                                                            \
      if (sl.valid[i]) {                                                                                \
        if (S == 6 && a.want_stiff) a.g6[sl.g[i]] = x;                                                  \
        if (S == 7) unew[sl.g[i]] = x;                                                                  \
      }                                                                                                 \
      if (sl.in[i]) s.xa[sl.lidx[i]] = sl.valid[i] ? act_apply(cd.in_act, x) : 0.f;                     \
    }                                                                                                   \
    __syncthreads();                                                                                    \
    const float* r_ = chain_feval(cd, s.w, s.xa, s.xb, (TS));                                           \
    float* kout_ = (S == 7) ? k7 : a.ks[S < 7 ? S - 2 : 0];                                                       \
    const bool st_ = (S == 7) || bc.store_k;                                                            \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                                  \
      kr[S - 1][i] = sl.in[i] ? r_[sl.lidx[i]] : 0.f;                                                   \
      if (st_ && sl.valid[i]) kout_[sl.g[i]] = kr[S - 1][i];                                            \
    }                                                                                                   \
  } while (0)
  LRNDE_CHAIN_STAGE(2, t + (float)Tsit5::C[0] * dt);
  LRNDE_CHAIN_STAGE(3, t + (float)Tsit5::C[1] * dt);
  LRNDE_CHAIN_STAGE(4, t + (float)Tsit5::C[2] * dt);
  LRNDE_CHAIN_STAGE(5, t + (float)Tsit5::C[3] * dt);
  LRNDE_CHAIN_STAGE(6, t + dt);
  LRNDE_CHAIN_STAGE(7, t + dt);
#undef LRNDE_CHAIN_STAGE

  // utilde, scaled residual, regularisation residuals (src/perform_step.jl:21-47, 210-212): k_step's expressions
  double aerr = 0.0, anum = 0.0, aden = 0.0;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    if (!sl.valid[i]) continue;
    float sum = (float)Tsit5::BT[0] * kr[0][i] + (float)Tsit5::BT[1] * kr[1][i];
    sum = sum + (float)Tsit5::BT[2] * kr[2][i];
    sum = sum + (float)Tsit5::BT[3] * kr[3][i];
    sum = sum + (float)Tsit5::BT[4] * kr[4][i];
    sum = sum + (float)Tsit5::BT[5] * kr[5][i];
    sum = sum + (float)Tsit5::BT[6] * kr[6][i];
    const float utilde = dt * sum;
    const float sc = a.abstol + fmaxf_(__builtin_fabsf(up[i]), __builtin_fabsf(un[i])) * a.reltol;
    const float r = utilde / sc;
    const float sq = r * r;
    aerr += (double)sq;
    if (a.want_stiff) {
      const float d1 = un[i] - g6[i];
      const float d2 = kr[6][i] - kr[5][i];
      const float q1 = d1 * d1, q2 = d2 * d2;
      aden += (double)q1; anum += (double)q2;
    }
  }
  block_sum3(s.red, aerr, anum, aden);
  publish_partial(a, (j + 1) & 1, aerr, anum, aden);
}

// ---- vector-Jacobian product ----
struct VjpChainArgs {
  int B;
  float t;
  const float* y;      // (B,D) or NULL -> interpolate from the dense record
  const float* dense;  // [uprev, k1, P2, P3, P4] of one forward step (lrnde_math.hpp), REC_ARRAYS arrays of B*D
  float theta, dense_dt;
  const float* lam;    // (B,D)
  float* dy;           // (B,D)
  float* gpart;        // [nwg][P] per-workgroup parameter cotangents, or NULL
};

// dy = J^T lam; gpart[blockIdx.x] = (df/dp)^T lam summed over the tile's columns (in column order)
__global__ __launch_bounds__(NT) void k_vjp_chain(ChainDev cd, VjpChainArgs v) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int D = cd.D;
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, v.B - b0);
  const ChainSlots sl = chain_slots(D, b0, nvalid);
  float* du = lds + cd.uoff;        // act0'(u)
  float* ga = lds + cd.gboff;
  float* gb = ga + CMAXW * CNB;
  // ---- y (given, or the Tsit5 interpolant of the stored forward step) -> a_0 = act0.(y) ----
  {
    float* a0 = lds + cd.meta[CM_AOFF];
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      if (!sl.in[i]) continue;
      float y = 0.f;
      if (sl.valid[i]) {
        const size_t g = sl.g[i];
        if (v.y) {
          y = v.y[g];
        } else {
          const size_t nst = (size_t)v.B * D;
          y = tsit5_rec_eval(v.dense[g], v.dense[nst + g], v.dense[2 * nst + g], v.dense[3 * nst + g], v.dense[4 * nst + g],
                             v.theta, v.dense_dt);
        }
      }
      const float h = act_apply(cd.in_act, y);
      a0[sl.lidx[i]] = h;
      du[sl.lidx[i]] = act_deriv_c(cd.in_act, y, h);
    }
  }
  __syncthreads();
  // ---- forward: every layer's input and act' stay in LDS ----
  for (int l = 0; l < cd.L; ++l) {
    const int* mt = cd.meta + l * CMETA;
    float* xout = (l + 1 < cd.L) ? lds + mt[CMETA + CM_AOFF] : gb;
    chain_layer(cd.wf + mt[CM_WOFF], mt[CM_IN], mt[CM_OUT], mt[CM_OUTP], cd.td, mt[CM_ACT], lds + mt[CM_AOFF], xout,
                lds + mt[CM_ZOFF], v.t);
    __syncthreads();
  }
  // ---- backward ----
#pragma unroll
  for (int i = 0; i < CEPT; ++i)
    if (sl.in[i]) ga[sl.lidx[i]] = sl.valid[i] ? v.lam[sl.g[i]] : 0.f;
  __syncthreads();
  float* gc = ga;
  float* gn = gb;
  for (int l = cd.L - 1; l >= 0; --l) {
    const int* mt = cd.meta + l * CMETA;
    const int in = mt[CM_IN], out = mt[CM_OUT];
    const float* al = lds + mt[CM_AOFF];
    const float* zl = lds + mt[CM_ZOFF];
    for (int e = threadIdx.x; e < out * CNB; e += NT) gc[e] = gc[e] * zl[e];  // delta = g .* act'(z)
    __syncthreads();
    if (v.gpart) {  // this layer's block of the flat Lux vector: vec(W) (out x (in+td)), then b
      const int nw = out * (in + cd.td);
      float* gp = v.gpart + (size_t)blockIdx.x * cd.P + mt[CM_POFF];
      for (int q = threadIdx.x; q < nw + out; q += NT) {
        float acc = 0.f;
        if (q < nw) {
          const int o = q % out, k = q / out;
          if (k < in) {
#pragma unroll
            for (int n = 0; n < CNB; ++n) acc = fma_(gc[o * CNB + n], al[k * CNB + n], acc);
          } else {
#pragma unroll
            for (int n = 0; n < CNB; ++n) acc = fma_(gc[o * CNB + n], v.t, acc);
          }
        } else {
          const int o = q - nw;
#pragma unroll
          for (int n = 0; n < CNB; ++n) acc = acc + gc[o * CNB + n];
        }
        gp[q] = acc;
      }
    }
    // g_prev[k][n] = sum_o W[o][k] delta[o][n]  (o ascending)
    const float* wg = cd.wg + mt[CM_GOFF];
    for (int e = threadIdx.x; e < in * CNB; e += NT) {
      const int k = e >> 3, n = e & (CNB - 1);
      float acc = 0.f;
      for (int o = 0; o < out; ++o) acc = fma_(wg[(size_t)o * in + k], gc[o * CNB + n], acc);
      gn[e] = acc;
    }
    __syncthreads();
    float* tmp = gc; gc = gn; gn = tmp;
  }
#pragma unroll
  for (int i = 0; i < CEPT; ++i)
    if (sl.valid[i]) v.dy[sl.g[i]] = gc[sl.lidx[i]] * du[sl.lidx[i]];
}

// gp = (accumulate ? gp : 0) + sum over the workgroups of their partial, in workgroup order from 0.  A sum over several
// launches' partials (the wide chain's chunked VJP) is one chain all the same: it starts from carry_in instead of 0 and,
// but for the last launch, goes to carry_out instead of gp.
__global__ void k_chain_pgsum(const float* part, int nwg, int P, float* gp, int accumulate, const float* carry_in, float* carry_out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
    float acc = carry_in ? carry_in[i] : 0.f;
    for (int w = 0; w < nwg; ++w) acc = acc + part[(size_t)w * P + i];
    if (carry_out) carry_out[i] = acc;
    else gp[i] = accumulate ? gp[i] + acc : acc;
  }
}

// flat Lux vector -> the forward image (per layer rows k = 0..in+td of outp floats: W[:, k] then b, zero padded) and the
// backward image (W row-major, the state columns only).  In the Lux layout column k of layer l is p[poff + out*k + o]
// for k < in+td and the bias follows as column in+td: one formula for every row of the forward image.
__global__ void k_pack_chain(const float* p, ChainDev cd, int gfloats, float* wf, float* wg) {
  const int total = cd.wfloats + gfloats;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < cd.wfloats) {
      float val = 0.f;
      for (int l = 0; l < cd.L; ++l) {
        const int* mt = cd.meta + l * CMETA;
        const int in = mt[CM_IN], out = mt[CM_OUT], outp = mt[CM_OUTP], woff = mt[CM_WOFF];
        const int loc = i - woff;
        if (loc >= 0 && loc < (in + cd.td + 1) * outp) {
          const int k = loc / outp, o = loc % outp;
          if (o < out) val = p[(size_t)mt[CM_POFF] + (size_t)out * k + o];
        }
      }
      wf[i] = val;
    } else {
      const int gi = i - cd.wfloats;
      for (int l = 0; l < cd.L; ++l) {
        const int* mt = cd.meta + l * CMETA;
        const int in = mt[CM_IN], out = mt[CM_OUT], goff = mt[CM_GOFF];
        const int loc = gi - goff;
        if (loc >= 0 && loc < in * out) {
          const int o = loc / in, k = loc % in;
          wg[gi] = p[(size_t)mt[CM_POFF] + (size_t)out * k + o];
        }
      }
    }
  }
}

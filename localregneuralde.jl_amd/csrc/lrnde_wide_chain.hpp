// lrnde_wide_chain.hpp — the wide Dense-chain vector field (lrnde_create_wide_chain), included by lrnde_kernels.hip inside
// its anonymous namespace behind lrnde_chain.hpp (whose descriptor, parameter layout and partial-sum launch it shares).
//
//   Chain(act0.(u), Dense(d0 => d1, a1), ..., Dense(d(L-1) => dL, aL))  or  TDChain(Chain(Dense..)),  d0 = dL = D,
//   every width <= 1024, L <= 16.
//
// Tile: NB = 16 batch columns per workgroup of NT = 512 threads (8 waves), v_mfma_f32_16x16x4_f32 — the k_step<W> family's
// tile, so step_prologue, the fp64 partial protocol and the state workspace carry over unchanged.
//
// Weights: per layer an image in A-fragment order, [row tile][k-group][lane][4] (one 1-KiB wave-load per 16 rows x 16
// input rows, zero padded; row tiles padded to a multiple of WT), streamed from L2 with buffer loads, the next k-group in
// flight while the current one multiplies.  The t column and the bias are vectors beside it.  A transposed image (rows =
// the layer's inputs) serves g <- W^T delta of the backward pass through the same routine.
//
// Activations: two ping-pong LDS buffers in B-fragment order (lds_index), ceil16(widest layer) x 16 floats each.
//
// Canonical arithmetic, every layer: fp32 fma chains over consecutive segments of SEGK*16 = 112 input rows,
// each from 0 with k ascending (what a run of the MFMA computes), segment partials added left to right, the time column by
// fma, + bias, act_apply.  wide_gemm gives a wave WT row tiles of one segment (or of all segments in turn) as independent
// accumulator chains; when a layer has fewer row-tile groups than waves its segments are spread over the waves as well and
// the partials meet in LDS, where they are added in segment order.  Either way the sum of a row is the same expression: a
// column's result depends neither on B nor on the workgroup that holds it.
//
// Step kernel: one launch per attempted Tsit5 step: step_prologue, the savevalues / dense-record footer of the previous
// attempt, six stages, the fp64 partials.  The stage operands (uprev, k1..k7, g6, u) stay in global memory (L2): the lane
// that ends a row quad of the last layer stores k_S and builds the next stage input from operands it wrote itself.
//
// VJP: the forward pass writes every layer's input and act' to a per-workgroup record in global scratch; then per layer
// delta = g .* act', the tile's parameter cotangent (an MFMA over the tile's 16 columns: an fma chain in column order) goes
// to a per-workgroup partial vector, and g <- W^T delta.  k_chain_pgsum adds the partials in workgroup order.  No atomics.
// Stated exactly (tests/wide_chain_vjp_host.cpp restates it on the host, lrnde_vjp gives its bits): g <- W^T delta is
// wide_gemm on the transposed image, i.e. 112-row segments over the layer's OUTPUTS, o ascending, segment sums left to
// right; gW[o][k] is the fma chain from 0 over the tile's columns n = 0..15 (the columns past B are y = 0, lam = 0) of
// a[k][n] * delta[o][n]; the t column the fma chain over n of delta[o][n] * t; the bias 0 + delta[o][0] + ...; gp the
// partials added in workgroup order from 0, also when the batch takes several launches.

constexpr int WT = 4;                    // row tiles a wave runs as independent accumulator chains
constexpr int WMAXW = 1024;              // widest layer (LRNDE_WIDE_CHAIN_MAX_WIDTH)
constexpr int WMETA = 12;                // ints per layer in the layer table
// (WIDE_LDS_MAX, WIDE_SCRATCH_MAX: lrnde_adj_route.hpp.)  Scratch of one VJP launch (activation records + parameter-cotangent
// partials of the workgroups it runs) stays within WIDE_SCRATCH_MAX; a batch that needs more runs as several launches over
// consecutive workgroups (one workgroup's share always fits: lrnde_create_wide_chain)

// per layer: in, out, act, MT = row tiles, KG = k-groups, woff / goff (forward / transposed image, floats), voff (t column
// then bias, MT*16 floats each), poff (flat Lux vector), raoff / rzoff (VJP record: layer input, act'; [row][NB])
enum { WM_IN, WM_OUT, WM_ACT, WM_MT, WM_KG, WM_WOFF, WM_GOFF, WM_VOFF, WM_POFF, WM_RAOFF, WM_RZOFF };

struct WideDev {
  int L, td, in_act, D, P;
  int bufw;       // floats of one activation buffer: ceil16(widest layer) * NB
  int partcap;    // floats of the segment-partial region
  int recfloats;  // floats of one workgroup's VJP record
  int rduoff;     // record offset of act0'(y)
  const int* meta;   // [L][WMETA] (device)
  const float* wf;   // forward images
  const float* wg;   // transposed images
  const float* vec;  // t columns and biases
};

struct WideSmem { float* xa; float* xb; float* part; double* red; Bcast* bc; };
__device__ __forceinline__ WideSmem wide_carve(const WideDev& wd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  WideSmem s;
  s.xa = reinterpret_cast<float*>(smem);
  s.xb = s.xa + wd.bufw;
  s.part = s.xb + wd.bufw;
  s.red = reinterpret_cast<double*>(s.part + wd.partcap);
  s.bc = reinterpret_cast<Bcast*>(s.red + NW * 3);
  return s;
}
constexpr size_t WIDE_LDS_TAIL = NW * 3 * sizeof(double) + sizeof(Bcast) + 16;   // behind the buffers: red, bc, padding
static size_t wide_smem_bytes(int bufw, int partcap) { return wide_lds_bytes(bufw, partcap, WIDE_LDS_TAIL); }
// floats of segment partials a (MT row tiles) x (KG k-groups) product wants when its segments are spread over the waves
static int wide_part_want(int MT, int KG) {
  const int ngrp = (MT + WT - 1) / WT, nseg = (KG + SEGK - 1) / SEGK;
  return (ngrp < NW && nseg > 1) ? nseg * MT * 256 : 0;
}

// WT row tiles (tbase: their first 1-KiB block, KG blocks apart) over the k-groups [kg_lo, kg_hi): acc = the fma chains
// from 0.  The next k-group's A fragments and B fragment are in flight while the current one multiplies (feval_tile).
__device__ __forceinline__ void wide_seg(__amdgpu_buffer_rsrc_t rs, int voff, int tbase, int KG, int kg_lo, int kg_hi,
                                         const f32x4* xp, f32x4 (&acc)[WT]) {
  f32x4 aX[WT], aY[WT], bX, bY;
#pragma unroll
  for (int i = 0; i < WT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#define LRNDE_WLOAD(a, b, kg)                                                                                  \
  do {                                                                                                         \
    b = xp[(kg) * 64];                                                                                         \
    _Pragma("unroll") for (int i = 0; i < WT; ++i) a[i] = wload(rs, voff, (tbase + i * KG + (kg)) * 1024);      \
    __builtin_amdgcn_sched_barrier(0);                                                                         \
  } while (0)
#define LRNDE_WMMA(a, b)                                                                                       \
  do {                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < WT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b.x, acc[i], 0, 0, 0); \
    _Pragma("unroll") for (int i = 0; i < WT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b.y, acc[i], 0, 0, 0); \
    _Pragma("unroll") for (int i = 0; i < WT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b.z, acc[i], 0, 0, 0); \
    _Pragma("unroll") for (int i = 0; i < WT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b.w, acc[i], 0, 0, 0); \
    __builtin_amdgcn_sched_barrier(0);                                                                         \
  } while (0)
  int kg = kg_lo;
  LRNDE_WLOAD(aX, bX, kg_lo);
#pragma unroll 1
  for (; kg + 2 < kg_hi; kg += 2) {
    LRNDE_WLOAD(aY, bY, kg + 1);
    LRNDE_WMMA(aX, bX);
    LRNDE_WLOAD(aX, bX, kg + 2);
    LRNDE_WMMA(aY, bY);
  }
  if (kg + 1 < kg_hi) {
    LRNDE_WLOAD(aY, bY, kg + 1);
    LRNDE_WMMA(aX, bX);
    LRNDE_WMMA(aY, bY);
  } else {
    LRNDE_WMMA(aX, bX);
  }
#undef LRNDE_WLOAD
#undef LRNDE_WMMA
}

// [MT*16 x KG*16] (image img) times the B-fragment tile xin: fin(mt, v, l) is called once for every row tile mt and lane
// slot l with v = rows mt*16 + (l>>4)*4 .. +3 of column l&15, each the canonical sum (file head).  The caller synchronises
// before xin or the partial region is written again.
template <class Fin>
__device__ __forceinline__ void wide_gemm(const float* img, int MT, int KG, int partcap, const float* xin, float* part, Fin&& fin) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int voff = lane * 16;
  const int ngrp = (MT + WT - 1) / WT, nseg = (KG + SEGK - 1) / SEGK;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)img, 0, ngrp * WT * KG * 1024, 0x00020000);
  const f32x4* xp = reinterpret_cast<const f32x4*>(xin) + lane;
  const bool split = ngrp < NW && nseg > 1 && nseg * MT * 256 <= partcap;
  if (!split) {
#pragma unroll 1
    for (int g = wave; g < ngrp; g += NW) {
      f32x4 tot[WT];
#pragma unroll 1
      for (int seg = 0; seg < nseg; ++seg) {
        f32x4 acc[WT];
        wide_seg(rs, voff, g * WT * KG, KG, seg * SEGK, min(KG, seg * SEGK + SEGK), xp, acc);
        if (seg == 0) {
#pragma unroll
          for (int i = 0; i < WT; ++i) tot[i] = acc[i];
        } else {
#pragma unroll
          for (int i = 0; i < WT; ++i) { tot[i].x = tot[i].x + acc[i].x; tot[i].y = tot[i].y + acc[i].y; tot[i].z = tot[i].z + acc[i].z; tot[i].w = tot[i].w + acc[i].w; }
        }
      }
#pragma unroll
      for (int i = 0; i < WT; ++i)
        if (g * WT + i < MT) fin(g * WT + i, tot[i], lane);
    }
    return;
  }
  f32x4* pp = reinterpret_cast<f32x4*>(part);
#pragma unroll 1
  for (int it = wave; it < ngrp * nseg; it += NW) {
    const int g = it % ngrp, seg = it / ngrp;
    f32x4 acc[WT];
    wide_seg(rs, voff, g * WT * KG, KG, seg * SEGK, min(KG, seg * SEGK + SEGK), xp, acc);
#pragma unroll
    for (int i = 0; i < WT; ++i)
      if (g * WT + i < MT) pp[((size_t)seg * MT + g * WT + i) * 64 + lane] = acc[i];
  }
  __syncthreads();
  const int nquad = MT * 64;
  for (int q = threadIdx.x; q < nquad; q += NT) {
    f32x4 v = pp[q];
    for (int sgi = 1; sgi < nseg; ++sgi) {
      const f32x4 pv = pp[(size_t)sgi * nquad + q];
      v.x = v.x + pv.x; v.y = v.y + pv.y; v.z = v.z + pv.z; v.w = v.w + pv.w;
    }
    fin(q >> 6, v, q & 63);
  }
}

// rows row0..row0+3 of one column at global offset g: nrow of them are real (0: none); v4: D % 4 == 0, so the quad is
// one aligned 16-byte access
__device__ __forceinline__ f32x4 wide_ld4(const float* p, size_t g, int nrow, bool v4) {
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (v4) {
    if (nrow > 0) r = *reinterpret_cast<const f32x4*>(p + g);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i < nrow) r[i] = p[g + i];
  }
  return r;
}
__device__ __forceinline__ void wide_st4(float* p, size_t g, int nrow, bool v4, const f32x4& x) {
  if (v4) {
    if (nrow > 0) *reinterpret_cast<f32x4*>(p + g) = x;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i < nrow) p[g + i] = x[i];
  }
}

// the (row quad, column) a lane slot of a row tile ends: rows row0.., column n, global offset g, nrow real rows
struct WideQuad { int n, rq, row0, nrow; size_t g; };
__device__ __forceinline__ WideQuad wide_quad(int mt, int l, int D, int b0, int nvalid) {
  WideQuad q;
  q.n = l & 15; q.rq = l >> 4; q.row0 = mt * 16 + q.rq * 4;
  q.nrow = (q.n < nvalid) ? max(0, min(4, D - q.row0)) : 0;
  q.g = (size_t)(b0 + q.n) * D + q.row0;
  return q;
}
// x (rows of q) -> the B-fragment tile xl, zero where there is no real element
__device__ __forceinline__ void wide_put(float* xl, int mt, const WideQuad& q, int in_act, const f32x4& x) {
  float* dst = xl + ((mt * 64 + q.n) << 2) + q.rq;
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[r * 64] = (r < q.nrow) ? act_apply(in_act, x[r]) : 0.f;
}

// every element of the tile's B-fragment image (Dp = ceil16(D) rows): val(g, row, n) where it is real, else 0
template <class F> __device__ __forceinline__ void wide_stage(int D, int b0, int nvalid, float* xl, F&& val) {
  const int Dp = (D + 15) & ~15;
  for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
    const int n = idx / Dp, row = idx - n * Dp;
    const bool ok = n < nvalid && row < D;
    xl[lds_index(row, n)] = ok ? val((size_t)(b0 + n) * D + row, row, n) : 0.f;
  }
}

// the chain on the tile staged in src (input activation applied).  Hidden layers ping-pong src / dst; the last layer
// reads src and hands every row quad of f to out(mt, l, kv); dst is free for out to write (the next stage's input).
// rec: the workgroup's VJP record (every layer's input and act'), or NULL.  No barrier follows the last layer.
template <class Out>
__device__ __forceinline__ void wide_feval(const WideDev& wd, const WideSmem& s, float*& src, float*& dst, float t, float* rec,
                                           Out&& out) {
  for (int l = 0; l < wd.L; ++l) {
    const int* mt_ = wd.meta + l * WMETA;
    const int MT = mt_[WM_MT], KG = mt_[WM_KG], act = mt_[WM_ACT];
    const float* tv = wd.vec + mt_[WM_VOFF];
    const float* bv = tv + MT * 16;
    float* rz = rec ? rec + mt_[WM_RZOFF] : nullptr;
    const bool last = l + 1 == wd.L;
    float* ra = (rec && !last) ? rec + mt_[WMETA + WM_RAOFF] : nullptr;
    float* xout = dst;
    const int td = wd.td;
    wide_gemm(wd.wf + mt_[WM_WOFF], MT, KG, wd.partcap, src, s.part, [&](int mt, const f32x4& v, int ln) {
      const int n = ln & 15, rq = ln >> 4, o0 = mt * 16 + rq * 4;
      const f32x4 wt = *reinterpret_cast<const f32x4*>(tv + o0);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bv + o0);
      f32x4 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pre = td ? fma_(wt[r], t, v[r]) : v[r];
        pre = pre + bb[r];
        h[r] = act_apply(act, pre);
        if (rz) rz[(o0 + r) * NB + n] = act_deriv_c(act, pre, h[r]);
        if (ra) ra[(o0 + r) * NB + n] = h[r];
      }
      if (last) {
        out(mt, ln, h);
      } else {
        float* d = xout + ((mt * 64 + n) << 2) + rq;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r * 64] = h[r];
      }
    });
    if (!last) {
      __syncthreads();
      float* tmp = src; src = dst; dst = tmp;
    }
  }
}

// du = f(u, t) for the whole batch (lrnde_rhs)
__global__ __launch_bounds__(NT) void k_rhs_wide(WideDev wd, int B, const float* u, float t, float* du) {
  const WideSmem s = wide_carve(wd);
  const int b0 = blockIdx.x * NB, nvalid = min(NB, B - b0), D = wd.D;
  const bool v4 = (D & 3) == 0;
  float* src = s.xa;
  float* dst = s.xb;
  wide_stage(D, b0, nvalid, src, [&](size_t g, int, int) { return act_apply(wd.in_act, u[g]); });
  __syncthreads();
  wide_feval(wd, s, src, dst, t, nullptr, [&](int mt, int l, const f32x4& kv) {
    const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
    wide_st4(du, q.g, q.nrow, v4, kv);
  });
}

// init phase 1 (k_init1's protocol): f0 = f(u0, t0) -> k1; partial sums of (u0/sk)^2 and (f0/sk)^2
__global__ __launch_bounds__(NT) void k_init1_wide(StepArgs a, WideDev wd) {
  const WideSmem s = wide_carve(wd);
  const int b0 = blockIdx.x * NB, nvalid = min(NB, a.B - b0), D = wd.D;
  const bool v4 = (D & 3) == 0;
  const Ctrl c = a.ctrl[0];
  const float* u0 = ubuf_at(a, c.cur);
  float* f0 = kfsal_at(a, c.cur);
  float* src = s.xa;
  float* dst = s.xb;
  wide_stage(D, b0, nvalid, src, [&](size_t g, int, int) { return act_apply(wd.in_act, u0[g]); });
  __syncthreads();
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  wide_feval(wd, s, src, dst, c.t, nullptr, [&](int mt, int l, const f32x4& kv) {
    const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
    wide_st4(f0, q.g, q.nrow, v4, kv);
    const f32x4 u = wide_ld4(u0, q.g, q.nrow, v4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= q.nrow) continue;
      const float sk = a.abstol + __builtin_fabsf(u[r]) * a.reltol;
      const float r0 = u[r] / sk, r1 = kv[r] / sk;
      const float q0 = r0 * r0, q1 = r1 * r1;
      a0 += (double)q0; a1 += (double)q1;
    }
  });
  block_sum3(s.red, a0, a1, a2);
  publish_partial(a, 2, a0, a1, 0.0);
}

// init phase 2: u1 = u0 + dt0*f0, f1 = f(u1, t0+dt0) -> ks[0]; partial sum of ((f1-f0)/sk)^2
__global__ __launch_bounds__(NT) void k_init2_wide(StepArgs a, WideDev wd) {
  const WideSmem s = wide_carve(wd);
  const int b0 = blockIdx.x * NB, nvalid = min(NB, a.B - b0), D = wd.D;
  const bool v4 = (D & 3) == 0;
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
  float* f1 = a.ks[0];
  float* src = s.xa;
  float* dst = s.xb;
  wide_stage(D, b0, nvalid, src, [&](size_t g, int, int) { return act_apply(wd.in_act, u0[g] + dt0 * f0[g]); });
  __syncthreads();
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  wide_feval(wd, s, src, dst, c.t + dt0, nullptr, [&](int mt, int l, const f32x4& kv) {
    const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
    wide_st4(f1, q.g, q.nrow, v4, kv);
    const f32x4 u = wide_ld4(u0, q.g, q.nrow, v4), f = wide_ld4(f0, q.g, q.nrow, v4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= q.nrow) continue;
      const float sk = a.abstol + __builtin_fabsf(u[r]) * a.reltol;
      const float r2 = (kv[r] - f[r]) / sk;
      const float q2 = r2 * r2;
      a0 += (double)q2;
    }
  });
  block_sum3(s.red, a0, a1, a2);
  publish_partial(a, 3, a0, 0.0, 0.0);
}

// what the lane that ends a row quad of k_S does with it (k_step's EpiStage / EpiFinal expressions, operands from L2)
struct WideStepEpi {
  const float* uprev; float* unew; const float* k1; float* k7; float* ks0; float* g6;
  size_t nst;   // floats between ks[i] and ks[i+1]
  float dt, abstol, reltol;
  int want_stiff, in_act, D, b0, nvalid;
  bool v4;
  // after k_S (S = 2..6): store it, x_{S+1} = uprev + dt*(a_{S+1,1} k1 + ... + a_{S+1,S} k_S) left to right -> xl (and u / g6)
  template <int S> __device__ __forceinline__ void stage(int mt, int l, const f32x4& kv, float* xl) const {
    const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
    wide_put(xl, mt, q, in_act, stage_x<S>(q, kv));
  }
  // the same without the LDS store: x_{S+1} of the quad (k_wdisc_step also keeps act0 and act0' of it in its stage record)
  template <int S> __device__ __forceinline__ f32x4 stage_x(const WideQuad& q, const f32x4& kv) const {
    constexpr int off = (S - 1) * S / 2;
    wide_st4(ks0 + (size_t)(S - 2) * nst, q.g, q.nrow, v4, kv);
    const f32x4 up = wide_ld4(uprev, q.g, q.nrow, v4);
    f32x4 o[S];
    o[0] = wide_ld4(k1, q.g, q.nrow, v4);
#pragma unroll
    for (int j = 1; j < S - 1; ++j) o[j] = wide_ld4(ks0 + (size_t)(j - 1) * nst, q.g, q.nrow, v4);
    o[S - 1] = kv;
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sum = (float)Tsit5::A[off] * o[0][r] + (float)Tsit5::A[off + 1] * o[1][r];
#pragma unroll
      for (int j = 2; j < S; ++j) sum = sum + (float)Tsit5::A[off + j] * o[j][r];
      x[r] = up[r] + dt * sum;
    }
    if (S == 5 && want_stiff) wide_st4(g6, q.g, q.nrow, v4, x);
    if (S == 6) wide_st4(unew, q.g, q.nrow, v4, x);
    return x;
  }
  // after k7: store it; utilde, the scaled residual and the stiffness differences in fp64 per lane
  __device__ __forceinline__ void final(int mt, int l, const f32x4& kv, double& aerr, double& anum, double& aden) const {
    const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
    wide_st4(k7, q.g, q.nrow, v4, kv);
    if (q.nrow == 0) return;
    const f32x4 up = wide_ld4(uprev, q.g, q.nrow, v4), un = wide_ld4(unew, q.g, q.nrow, v4);
    f32x4 k[6];
    k[0] = wide_ld4(k1, q.g, q.nrow, v4);
#pragma unroll
    for (int j = 1; j < 6; ++j) k[j] = wide_ld4(ks0 + (size_t)(j - 1) * nst, q.g, q.nrow, v4);
    f32x4 gg = {0.f, 0.f, 0.f, 0.f};
    if (want_stiff) gg = wide_ld4(g6, q.g, q.nrow, v4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= q.nrow) continue;
      float sum = (float)Tsit5::BT[0] * k[0][r] + (float)Tsit5::BT[1] * k[1][r];
      sum = sum + (float)Tsit5::BT[2] * k[2][r];
      sum = sum + (float)Tsit5::BT[3] * k[3][r];
      sum = sum + (float)Tsit5::BT[4] * k[4][r];
      sum = sum + (float)Tsit5::BT[5] * k[5][r];
      sum = sum + (float)Tsit5::BT[6] * kv[r];
      const float utilde = dt * sum;
      const float sc = abstol + fmaxf_(__builtin_fabsf(up[r]), __builtin_fabsf(un[r])) * reltol;
      const float rr = utilde / sc;
      const float sq = rr * rr;
      aerr += (double)sq;
      if (want_stiff) {
        const float d1 = un[r] - gg[r];
        const float d2 = kv[r] - k[5][r];
        const float q1 = d1 * d1, q2 = d2 * d2;
        aden += (double)q1; anum += (double)q2;
      }
    }
  }
};

// one attempted Tsit5 step (src/perform_step.jl:3-47) of the whole batch, preceded by the device-side footer of the
// previous attempt and header of this one (step_prologue, as k_step / k_step_q).  SPEC only changes the kernel's name.
template <bool SPEC> __global__ __launch_bounds__(NT) void k_step_wide(StepArgs a, WideDev wd, int j) {
  const WideSmem s = wide_carve(wd);
  const int b0 = blockIdx.x * NB, nvalid = min(NB, a.B - b0);
  const int D = wd.D;
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
  WideStepEpi e;
  e.uprev = ubuf_at(a, bc.cur); e.unew = ubuf_at(a, bc.cur ^ 1);
  e.k1 = kfsal_at(a, bc.cur); e.k7 = kfsal_at(a, bc.cur ^ 1);
  e.ks0 = a.ks[0]; e.g6 = a.g6; e.nst = (size_t)a.n_local;
  e.dt = dt; e.abstol = a.abstol; e.reltol = a.reltol;
  e.want_stiff = a.want_stiff; e.in_act = wd.in_act; e.D = D; e.b0 = b0; e.nvalid = nvalid; e.v4 = (D & 3) == 0;
  float* src = s.xa;
  float* dst = s.xb;
  // the first stage input needs a pass of its own (stage_value<2>); every later one is built by the lanes that end k_S
  wide_stage(D, b0, nvalid, src, [&](size_t g, int, int) {
    const float kv = e.k1[g];
    return act_apply(wd.in_act, stage_value<2>(e.uprev[g], &kv, dt));
  });
  __syncthreads();
  double aerr = 0.0, anum = 0.0, aden = 0.0;
#pragma unroll 1
  for (int S = 2; S <= 7; ++S) {
    const float cS = S == 2 ? (float)Tsit5::C[0] : (S == 3 ? (float)Tsit5::C[1] : (S == 4 ? (float)Tsit5::C[2] : (float)Tsit5::C[3]));
    const float ts = S >= 6 ? t + dt : t + cS * dt;
    wide_feval(wd, s, src, dst, ts, nullptr, [&](int mt, int l, const f32x4& kv) {
      switch (S) {   // (uniform over the workgroup)
        case 2: e.stage<2>(mt, l, kv, dst); break;
        case 3: e.stage<3>(mt, l, kv, dst); break;
        case 4: e.stage<4>(mt, l, kv, dst); break;
        case 5: e.stage<5>(mt, l, kv, dst); break;
        case 6: e.stage<6>(mt, l, kv, dst); break;
        default: e.final(mt, l, kv, aerr, anum, aden); break;
      }
    });
    __syncthreads();   // the next stage input is complete in dst; src and the partial region are free
    float* tmp = src; src = dst; dst = tmp;
  }
  block_sum3(s.red, aerr, anum, aden);
  publish_partial(a, (j + 1) & 1, aerr, anum, aden);
}

// ---- vector-Jacobian product ----
struct VjpWideArgs {
  int B, wg0;          // this launch runs the workgroups wg0 .. wg0 + gridDim.x - 1 of the batch
  float t;
  const float* y;      // (B,D) or NULL -> interpolate from the dense record
  const float* dense;  // [uprev, k1, P2, P3, P4] of one forward step (lrnde_math.hpp), REC_ARRAYS arrays of B*D
  float theta, dense_dt;
  const float* lam;    // (B,D)
  float* dy;           // (B,D)
  float* gpart;        // [gridDim.x][P] per-workgroup parameter cotangents, or NULL
  float* rec;          // [gridDim.x][recfloats] activation records
};

// dy = J^T lam; gpart[blockIdx.x] = (df/dp)^T lam summed over the tile's columns (in column order)
__global__ __launch_bounds__(NT) void k_vjp_wide(WideDev wd, VjpWideArgs v) {
  const WideSmem s = wide_carve(wd);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int D = wd.D;
  const int b0 = (v.wg0 + (int)blockIdx.x) * NB, nvalid = min(NB, v.B - b0);
  float* rec = v.rec + (size_t)blockIdx.x * wd.recfloats;
  float* gp = v.gpart ? v.gpart + (size_t)blockIdx.x * wd.P : nullptr;
  float* src = s.xa;
  float* dst = s.xb;
  // ---- y (given, or the Tsit5 interpolant of the stored forward step) -> a_0 = act0.(y), act0'(y) ----
  {
    float* ra0 = rec + wd.meta[WM_RAOFF];
    float* rdu = rec + wd.rduoff;
    const int Dp = (D + 15) & ~15;
    for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
      const int n = idx / Dp, row = idx - n * Dp;
      float y = 0.f;
      if (n < nvalid && row < D) {
        const size_t g = (size_t)(b0 + n) * D + row;
        if (v.y) {
          y = v.y[g];
        } else {
          const size_t nst = (size_t)v.B * D;
          y = tsit5_rec_eval(v.dense[g], v.dense[nst + g], v.dense[2 * nst + g], v.dense[3 * nst + g], v.dense[4 * nst + g],
                             v.theta, v.dense_dt);
        }
      }
      const float h = act_apply(wd.in_act, y);
      src[lds_index(row, n)] = h;
      ra0[row * NB + n] = h;
      rdu[row * NB + n] = act_deriv_c(wd.in_act, y, h);
    }
  }
  __syncthreads();
  // ---- forward: every layer's input and act' go to the record ----
  wide_feval(wd, s, src, dst, v.t, rec, [&](int, int, const f32x4&) {});
  __syncthreads();
  // ---- backward ----
  float* gc = src;
  float* gn = dst;
  wide_stage(D, b0, nvalid, gc, [&](size_t g, int, int) { return v.lam[g]; });
  __syncthreads();
  for (int l = wd.L - 1; l >= 0; --l) {
    const int* mt_ = wd.meta + l * WMETA;
    const int in = mt_[WM_IN], out = mt_[WM_OUT], MT = mt_[WM_MT], KG = mt_[WM_KG];
    const float* ra = rec + mt_[WM_RAOFF];
    const float* rz = rec + mt_[WM_RZOFF];
    for (int idx = threadIdx.x; idx < MT * 16 * NB; idx += NT) {  // delta = g .* act'(z)
      const int row = idx >> 4, n = idx & 15;
      const int li = lds_index(row, n);
      gc[li] = gc[li] * rz[idx];
    }
    __syncthreads();
    if (gp) {  // this layer's block of the flat Lux vector: vec(W) (out x (in+td)), then b
      float* gl = gp + mt_[WM_POFF];
      // gW[o][k] = fma chain over the columns n = 0..15 of a[k][n] * delta[o][n]: one 16 (k) x 16 (o) block per four MFMAs
      // with the columns as their K dimension; a lane ends up with four k of one o, so the 16 lanes of a row quad store 64
      // contiguous bytes of the Lux vector.  WPG blocks per trip: their operand loads are in flight together.
      constexpr int WPG = 4;
      const int lr = lane & 15, lq = lane >> 4, ntile = MT * KG;
#pragma unroll 1
      for (int tile0 = wave; tile0 < ntile; tile0 += WPG * NW) {
        float av[WPG][4], bv[WPG][4];
#pragma unroll
        for (int u = 0; u < WPG; ++u) {
          const int tile = min(tile0 + u * NW, ntile - 1);
          const int ot = tile % MT, kt = tile / MT;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            av[u][q] = ra[(kt * 16 + lr) * NB + 4 * q + lq];
            bv[u][q] = gc[lds_index(ot * 16 + lr, 4 * q + lq)];
          }
        }
#pragma unroll
        for (int u = 0; u < WPG; ++u) {
          const int tile = tile0 + u * NW;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][q], bv[u][q], acc, 0, 0, 0);
          if (tile < ntile) {
            const int ot = tile % MT, kt = tile / MT;
            const int o = ot * 16 + lr, k0 = kt * 16 + lq * 4;
            if (o < out) {
#pragma unroll
              for (int r = 0; r < 4; ++r) if (k0 + r < in) gl[(size_t)out * (k0 + r) + o] = acc[r];
            }
          }
        }
      }
      // the t column (k = in) and the bias (k = in + td)
      for (int q = threadIdx.x; q < (wd.td + 1) * out; q += NT) {
        const int o = q % out, which = q / out;
        float acc = 0.f;
        if (wd.td && which == 0) {
#pragma unroll
          for (int n = 0; n < NB; ++n) acc = fma_(gc[lds_index(o, n)], v.t, acc);
        } else {
#pragma unroll
          for (int n = 0; n < NB; ++n) acc = acc + gc[lds_index(o, n)];
        }
        gl[(size_t)out * (in + which) + o] = acc;
      }
    }
    // g_prev = W^T delta: rows = the layer's inputs (KG row tiles), summed over its outputs (MT k-groups)
    wide_gemm(wd.wg + mt_[WM_GOFF], KG, MT, wd.partcap, gc, s.part, [&](int mt, const f32x4& vv, int ln) {
      float* d = gn + ((mt * 64 + (ln & 15)) << 2) + (ln >> 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r * 64] = vv[r];
    });
    __syncthreads();
    float* tmp = gc; gc = gn; gn = tmp;
  }
  {
    const float* rdu = rec + wd.rduoff;
    const int Dp = (D + 15) & ~15;
    for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
      const int n = idx / Dp, row = idx - n * Dp;
      if (n < nvalid && row < D) v.dy[(size_t)(b0 + n) * D + row] = gc[lds_index(row, n)] * rdu[row * NB + n];
    }
  }
}

// flat Lux vector -> the forward images, the transposed images and the t / bias vectors (zero padded).  In the Lux layout
// column k of layer l is p[poff + out*k + o] for k < in+td and the bias follows as column in+td.
__global__ void k_pack_wide(const float* p, WideDev wd, int ftot, int gtot, int vtot, float* wf, float* wg, float* vec) {
  const int total = ftot + gtot + vtot;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float val = 0.f;
    for (int l = 0; l < wd.L; ++l) {
      const int* mt_ = wd.meta + l * WMETA;
      const int in = mt_[WM_IN], out = mt_[WM_OUT], MT = mt_[WM_MT], KG = mt_[WM_KG];
      const size_t pl = (size_t)mt_[WM_POFF];
      if (i < ftot) {         // [row tile (of WT-padded MT)][k-group][lane][4]: row = an output, k = an input
        const int loc = i - mt_[WM_WOFF];
        if (loc >= 0 && loc < ((MT + WT - 1) / WT) * WT * KG * 256) {
          const int q = loc & 3, ln = (loc >> 2) & 63, blk = loc >> 8;
          const int o = (blk / KG) * 16 + (ln & 15), k = (blk % KG) * 16 + q * 4 + (ln >> 4);
          if (o < out && k < in) val = p[pl + (size_t)out * k + o];
        }
      } else if (i < ftot + gtot) {  // transposed: row = an input, k = an output
        const int loc = i - ftot - mt_[WM_GOFF];
        if (loc >= 0 && loc < ((KG + WT - 1) / WT) * WT * MT * 256) {
          const int q = loc & 3, ln = (loc >> 2) & 63, blk = loc >> 8;
          const int k = (blk / MT) * 16 + (ln & 15), o = (blk % MT) * 16 + q * 4 + (ln >> 4);
          if (o < out && k < in) val = p[pl + (size_t)out * k + o];
        }
      } else {
        const int loc = i - ftot - gtot - mt_[WM_VOFF];
        if (loc >= 0 && loc < 2 * MT * 16) {
          const int o = loc % (MT * 16), which = loc / (MT * 16);
          if (o < out && (which == 1 || wd.td)) val = p[pl + (size_t)out * (in + (which ? wd.td : 0)) + o];
        }
      }
    }
    (i < ftot ? wf[i] : (i < ftot + gtot ? wg[i - ftot] : vec[i - ftot - gtot])) = val;
  }
}

// lrnde_sde_frame.hpp — what the three one-launch SDE step kernels (lrnde_sde_eh_fast.hip, lrnde_sde_mil_fast.hip,
// lrnde_sde_sri_fast.hip; the seam to the library: lrnde_sde_fast.hpp) are written on: the canonical dot product over resident
// weight fragments, the workgroup frame (SdeFrame), the device controller of the adaptive solves and the footer that runs it,
// and the launch dispatch by shape.  Included by those three translation units only; everything is local to each.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "lrnde_math.hpp"
#include "lrnde_report.hpp"
#include "lrnde_sde_fast.hpp"

namespace {

using namespace lrnde;

// -DLRNDE_SDE_STAMPS (tools/sde_persist_probe.hip): s_memtime of workgroup 0 at the phase boundaries of its first 32 steps
#ifdef LRNDE_SDE_STAMPS
__device__ unsigned long long g_sde_stamps[32][16];
#define SDE_STAMP(i) do { if (PERSIST && blockIdx.x == 0 && threadIdx.x == 0 && it < 32) g_sde_stamps[it][(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SDE_STAMP(i) do { } while (0)
#endif
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

// launch by shape: fn(integral_constant DT, integral_constant HT) with DT = ceil(D / 16) in 1..4, HT = ceil(H / 16) in 1..8;
// false, and nothing called, for a shape outside sde_fast_shape (every caller checks the gate first)
template <class F, int... I> inline bool sde_fast_dispatch_(int k, F& fn, std::integer_sequence<int, I...>) {
  return ((k == I && (fn(std::integral_constant<int, I / 8 + 1>{}, std::integral_constant<int, I % 8 + 1>{}), true)) || ...);
}
template <class F> inline bool sde_fast_dispatch(int D, int H, F fn) {
  if (!sde_fast_shape(D, H)) return false;
  return sde_fast_dispatch_(((D + 15) / 16 - 1) * 8 + (H + 15) / 16 - 1, fn, std::make_integer_sequence<int, 32>{});
}

}  // namespace

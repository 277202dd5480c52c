// lrnde_sde_tree.hpp — the Brownian path of the adaptive SDE solves as a VIRTUAL tree: W at a grid index is a
// pure function of (seed, stream, column, index), so no (nfine + 1) x B x D array has to exist.  Included by every translation
// unit that queries the tree (lrnde_kernels.hip and the TREE instantiations of the one-launch step kernels); also the home of
// the Philox-4x32-10 block and the Box-Muller pair that lrnde_noise.hpp draws with (one definition for both).  The two kernels
// that only lrnde_kernels.hip launches are in lrnde_sde_tree_kernels.hpp.
//
// Definition (include/lrnde.h states it for callers; tests/brownian_tree_np.py restates it in numpy).  nfine = 2^L, L <= 20,
// span = t2 - t0 (float32), column c = b*D + d, z[n] = standard normal n of column c in the stream — counter (n >> 2, c, stream, 0),
// word n & 3, float64 Box-Muller rounded once: lrnde_sde_draw_noise's normals.  Every operation below is one float32 operation:
//   W[0] = 0,  W[nfine] = sT z[0],  sT = (float)sqrt((double)span);
//   level l = 1..L, node j = 0..2^(l-1)-1:  a = j 2^(L-l+1), b = a + 2^(L-l+1), mid = a + 2^(L-l), n = 2^(l-1) + j,
//   W[mid] = (0.5 (W[a] + W[b])) + (s_l z[n]),  s_l = (float)(0.5 sqrt((double)span 2^-(l-1))).
// A query descends from (0, nfine) and computes only the midpoints on its way: L - ctz(k) levels.
// s_l on the device: a power of four under the square root leaves it as a power of two, and a power of two commutes with both
// roundings, so s_l = s_1 2^-((l-1)/2) for odd l and s_2 2^-((l-2)/2) for even l, exactly (no span whose s_20 is subnormal is
// of interest: span > 2^-100).  The host computes sT, s_1 and s_2 in float64 and the kernels scale them.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace lrnde {

constexpr uint32_t TREE_STREAM_W = 6, TREE_STREAM_Z = 7;   // the trees of W and of SRI's second path Z (streams 0..5: lrnde.h)
constexpr int TREE_MAXL = 20;

// the path source of a launch, by value in its arguments.  rec_dw / rec_dz: the recording forward leaves the accepted step's
// increments in slot naccept (beside rec_u), which is all a backward route reads
struct SdeTree {
  int on;             // 0: the caller's array (every field below unused)
  uint32_t k0, k1;    // Philox key: (seed & 0xffffffff, seed >> 32)
  int L;              // nfine = 2^L
  float sT, s1, s2;   // sqrt(span), s_1, s_2 (host float64, rounded once)
  float* rec_dw; float* rec_dz;
};
inline void sde_tree_scales(SdeTree& T, float span) {
  T.sT = (float)sqrt((double)span);
  T.s1 = (float)(0.5 * sqrt((double)span));
  T.s2 = (float)(0.5 * sqrt((double)span * 0.5));
}

}  // namespace lrnde

namespace {

using namespace lrnde;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

__device__ __forceinline__ double noise_u01(uint32_t x) { return ((double)(x >> 8) + 0.5) * 0x1p-24; }

// (z0, z1) = sqrt(-2 ln u_a) (cos, sin)(2 pi u_b), float64, rounded once
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const double r = sqrt(-2.0 * log(noise_u01(a)));
  const double th = 6.283185307179586 * noise_u01(b);
  z0 = (float)(r * cos(th));
  z1 = (float)(r * sin(th));
}

// standard normal n of column c (lrnde_sde_draw_noise's normal n: the pair of its word, cos for even words and sin for odd)
__device__ __forceinline__ float tree_normal(const SdeTree& T, uint32_t stream, uint32_t c, uint32_t n) {
  uint32_t x[4];
  philox4x32_10(n >> 2, c, stream, 0u, T.k0, T.k1, x);
  const bool hi = (n & 2u) != 0;
  float z0, z1;
  box_muller(hi ? x[2] : x[0], hi ? x[3] : x[1], z0, z1);
  return (n & 1u) ? z1 : z0;
}

// W[k] of the columns c[0..R) (0 <= k <= nfine).  The descent's indices depend on k alone: uniform control flow when every
// lane asks for the same k, whatever its columns.
template <int R>
__device__ __forceinline__ void tree_query(const SdeTree& T, uint32_t stream, const uint32_t (&c)[R], int k, float (&w)[R]) {
  const int nfine = 1 << T.L;
  float wa[R], wb[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { wa[r] = 0.f; w[r] = 0.f; }
  if (k <= 0) return;
#pragma unroll
  for (int r = 0; r < R; ++r) wb[r] = __fmul_rn(T.sT, tree_normal(T, stream, c[r], 0u));
  int a = 0, b = nfine;
  bool found = k >= nfine;
#pragma unroll 1
  for (int l = 1; l <= T.L && !found; ++l) {
    const int mid = (a + b) >> 1;
    const uint32_t n = (1u << (l - 1)) + (uint32_t)(a >> (T.L - l + 1));
    const float sl = ldexpf((l & 1) ? T.s1 : T.s2, -((l - 1) >> 1));
    const bool left = k < mid;
    found = mid == k;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float wm = __fadd_rn(__fmul_rn(0.5f, __fadd_rn(wa[r], wb[r])), __fmul_rn(sl, tree_normal(T, stream, c[r], n)));
      if (left || found) wb[r] = wm; else wa[r] = wm;   // (found: the result leaves through wb)
    }
    if (left) b = mid; else a = mid;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) w[r] = wb[r];
}

}  // namespace

// float32 host restatement of the wide Dense-chain vector-Jacobian product in the canonical order of
// csrc/lrnde_wide_chain.hpp (file head, "VJP"), with the scalar functions of csrc/lrnde_math.hpp and its own copy of
// act' (lrnde_backward.hpp's act_deriv_c is device code).  lrnde_vjp of a wide-chain handle must return these bits
// (tests/test_gpu_wide_chain.py).  -ffp-contract=off; every loop below leaves each element's chain of operations as
// stated here, the loops are only ordered so that the weights are walked contiguously and the 16 columns of a tile (or the
// outputs of a weight row) are the inner, independent, accumulators.
//
//   tile      16 consecutive columns (one workgroup); the columns past B are y = 0, lam = 0 and run like the others
//   forward   wide_chain_host.cpp's: z[o] = (sum over consecutive 112-input segments, left to right, of the fma chain from
//             0 over the segment's k ascending of W[o][k] * a[k]) (fma W[o][in] * t, TDChain) + b[o];  h = act(z);
//             kept per layer: its input a and act'(z) from (z, h);  a_0 = act0(y), act0'(y)
//   backward  g = lam;  per layer, last to first:
//               delta[o]  = g[o] * act'[o]
//               gW[o][k]  = fma chain from 0 over the tile's columns n = 0..15 of a[k][n] * delta[o][n]
//               gW[o][in] = fma chain from 0 over n of delta[o][n] * t               (TDChain)
//               gb[o]     = 0 + delta[o][0] + ... + delta[o][15]
//               g_prev[k] = sum over consecutive 112-OUTPUT segments, left to right, of the fma chain from 0 over the
//                           segment's o ascending of W[o][k] * delta[o]
//             dy = g_0 * act0'(y)
//   gp        0 + (tile 0's partial) + (tile 1's) + ...   in tile order.  chunk > 0 states what a VJP split over launches
//             of `chunk` tiles did before its running sum was carried through the launches: the sum of each launch's
//             tiles from 0, the launches' sums added in launch order (kept so that the difference can be shown).
//
//   wide_chain_vjp_host in.bin out.bin
//   in:  int32 L, td, input_act, B, chunk, dims[L+1], act[L]; float32 t, params (the flat Lux vector), y (B, D), lam (B, D)
//   out: float32 dy (B, D), gp (P)
#include "lrnde_math.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using lrnde::act_apply;
using lrnde::expf_c;
using lrnde::fma_;

constexpr int SEG = 112;
constexpr int NB = 16;

static inline float act_deriv(int act, float pre, float h) {
  if (act == 1) return 1.0f - h * h;
  if (act == 2) {
    const float two_lambda = 1.5957691216057308f;
    const float x2 = pre * pre;
    const float a = (two_lambda * pre) * fma_(x2, 0.044715f, 1.0f);
    const float sg = 1.0f / (1.0f + expf_c(-a));
    const float da = two_lambda * fma_(x2, 3.0f * 0.044715f, 1.0f);
    return sg + pre * sg * (1.0f - sg) * da;
  }
  return 1.0f;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hd[5];
  if (fread(hd, 4, 5, fi) != 5) return 2;
  const int L = hd[0], td = hd[1], in_act = hd[2], B = hd[3], chunk = hd[4];
  if (L < 1 || L > 16 || B < 1 || chunk < 0) return 2;
  std::vector<int32_t> dims(L + 1), act(L);
  if (fread(dims.data(), 4, L + 1, fi) != (size_t)L + 1 || fread(act.data(), 4, L, fi) != (size_t)L) return 2;
  float t;
  if (fread(&t, 4, 1, fi) != 1) return 2;
  size_t P = 0;
  int maxw = 0;
  std::vector<size_t> poff(L);
  for (int l = 0; l < L; ++l) { poff[l] = P; P += (size_t)dims[l + 1] * (dims[l] + td) + dims[l + 1]; }
  for (int l = 0; l <= L; ++l) maxw = dims[l] > maxw ? dims[l] : maxw;
  const int D = dims[0];
  std::vector<float> p(P), y((size_t)B * D), lam((size_t)B * D), dy((size_t)B * D), gp(P), csum(P);
  if (fread(p.data(), 4, P, fi) != P || fread(y.data(), 4, y.size(), fi) != y.size() || fread(lam.data(), 4, lam.size(), fi) != lam.size())
    return 2;
  fclose(fi);

  // per layer l: its input a[l] ([in][NB]) and act' dz[l] ([out][NB]); du = act0'(y)
  std::vector<std::vector<float>> a(L + 1), dz(L);
  for (int l = 0; l <= L; ++l) a[l].resize((size_t)dims[l] * NB);
  for (int l = 0; l < L; ++l) dz[l].resize((size_t)dims[l + 1] * NB);
  std::vector<float> du((size_t)D * NB), tot((size_t)maxw * NB), acc((size_t)maxw * NB), g((size_t)maxw * NB), gn((size_t)maxw * NB),
      delta((size_t)maxw * NB), deltaT((size_t)maxw * NB), row(maxw);

  const int ntile = (B + NB - 1) / NB;
  bool gp_started = false;
  for (int w = 0; w < ntile; ++w) {
    const int b0 = w * NB;
    if (chunk ? w % chunk == 0 : w == 0)
      for (size_t i = 0; i < P; ++i) csum[i] = 0.f;
    // ---- forward ----
    for (int k = 0; k < D; ++k)
      for (int n = 0; n < NB; ++n) {
        const float yy = b0 + n < B ? y[(size_t)(b0 + n) * D + k] : 0.f;
        const float h = act_apply(in_act, yy);
        a[0][(size_t)k * NB + n] = h;
        du[(size_t)k * NB + n] = act_deriv(in_act, yy, h);
      }
    for (int l = 0; l < L; ++l) {
      const int in = dims[l], out = dims[l + 1];
      const float* W = p.data() + poff[l];   // W[o][k] = W[out * k + o]
      const float* b = W + (size_t)out * (in + td);
      const float* x = a[l].data();
      for (int k0 = 0; k0 < in; k0 += SEG) {
        const int k1 = k0 + SEG < in ? k0 + SEG : in;
        for (size_t i = 0; i < (size_t)out * NB; ++i) acc[i] = 0.f;
        for (int k = k0; k < k1; ++k) {
          const float* __restrict wk = W + (size_t)out * k;
          const float* __restrict xk = x + (size_t)k * NB;
          float* __restrict ac = acc.data();
          for (int o = 0; o < out; ++o)
            for (int n = 0; n < NB; ++n) ac[o * NB + n] = fma_(wk[o], xk[n], ac[o * NB + n]);
        }
        if (k0 == 0) for (size_t i = 0; i < (size_t)out * NB; ++i) tot[i] = acc[i];
        else for (size_t i = 0; i < (size_t)out * NB; ++i) tot[i] = tot[i] + acc[i];
      }
      for (int o = 0; o < out; ++o)
        for (int n = 0; n < NB; ++n) {
          float z = tot[(size_t)o * NB + n];
          if (td) z = fma_(W[(size_t)out * in + o], t, z);
          z = z + b[o];
          const float h = act_apply(act[l], z);
          dz[l][(size_t)o * NB + n] = act_deriv(act[l], z, h);
          a[l + 1][(size_t)o * NB + n] = h;
        }
    }
    // ---- backward ----
    for (int k = 0; k < D; ++k)
      for (int n = 0; n < NB; ++n) g[(size_t)k * NB + n] = b0 + n < B ? lam[(size_t)(b0 + n) * D + k] : 0.f;
    for (int l = L - 1; l >= 0; --l) {
      const int in = dims[l], out = dims[l + 1];
      const float* W = p.data() + poff[l];
      float* cs = csum.data() + poff[l];
      for (int o = 0; o < out; ++o)
        for (int n = 0; n < NB; ++n) {
          const float d = g[(size_t)o * NB + n] * dz[l][(size_t)o * NB + n];
          delta[(size_t)o * NB + n] = d;
          deltaT[(size_t)n * out + o] = d;
        }
      // the tile's parameter cotangent, added to the running sum of the tiles
      for (int k = 0; k < in; ++k) {
        float* __restrict r = row.data();
        for (int o = 0; o < out; ++o) r[o] = 0.f;
        for (int n = 0; n < NB; ++n) {
          const float ak = a[l][(size_t)k * NB + n];
          const float* __restrict dt_ = deltaT.data() + (size_t)n * out;
          for (int o = 0; o < out; ++o) r[o] = fma_(ak, dt_[o], r[o]);
        }
        for (int o = 0; o < out; ++o) cs[(size_t)out * k + o] = cs[(size_t)out * k + o] + r[o];
      }
      for (int o = 0; o < out; ++o) {
        if (td) {
          float s = 0.f;
          for (int n = 0; n < NB; ++n) s = fma_(delta[(size_t)o * NB + n], t, s);
          cs[(size_t)out * in + o] = cs[(size_t)out * in + o] + s;
        }
        float s = 0.f;
        for (int n = 0; n < NB; ++n) s = s + delta[(size_t)o * NB + n];
        cs[(size_t)out * (in + td) + o] = cs[(size_t)out * (in + td) + o] + s;
      }
      // g_prev = W^T delta
      for (int k = 0; k < in; ++k) {
        const float* __restrict wk = W + (size_t)out * k;
        float tt[NB];
        for (int o0 = 0; o0 < out; o0 += SEG) {
          const int o1 = o0 + SEG < out ? o0 + SEG : out;
          float ac[NB];
          for (int n = 0; n < NB; ++n) ac[n] = 0.f;
          for (int o = o0; o < o1; ++o) {
            const float* __restrict dl = delta.data() + (size_t)o * NB;
            for (int n = 0; n < NB; ++n) ac[n] = fma_(wk[o], dl[n], ac[n]);
          }
          if (o0 == 0) for (int n = 0; n < NB; ++n) tt[n] = ac[n];
          else for (int n = 0; n < NB; ++n) tt[n] = tt[n] + ac[n];
        }
        for (int n = 0; n < NB; ++n) gn[(size_t)k * NB + n] = tt[n];
      }
      g.swap(gn);
    }
    for (int k = 0; k < D; ++k)
      for (int n = 0; n < NB && b0 + n < B; ++n) dy[(size_t)(b0 + n) * D + k] = g[(size_t)k * NB + n] * du[(size_t)k * NB + n];
    // ---- the sum over the tiles ----
    const bool closes = w + 1 == ntile || (chunk && (w + 1) % chunk == 0);
    if (closes) {
      if (!gp_started) for (size_t i = 0; i < P; ++i) gp[i] = csum[i];
      else for (size_t i = 0; i < P; ++i) gp[i] = gp[i] + csum[i];
      gp_started = true;
    }
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  if (fwrite(dy.data(), 4, dy.size(), fo) != dy.size() || fwrite(gp.data(), 4, gp.size(), fo) != gp.size()) return 2;
  fclose(fo);
  return 0;
}

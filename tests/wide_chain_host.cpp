// float32 host restatement of the wide Dense-chain vector field in the canonical accumulation order of
// csrc/lrnde_wide_chain.hpp, with the scalar functions of csrc/lrnde_math.hpp.  lrnde_rhs of a wide-chain
// handle must return these bits (tests/test_gpu_wide_chain.py); compile with -O2 -ffp-contract=off.
//
//   every layer:  z[o] = (sum over consecutive 112-row segments, left to right, of the fma chain from 0 over the segment's
//                 k ascending of W[o][k] * x[k])  (fma W[o][in] * t, TDChain)  + b[o];   h = act(z)
//
//   wide_chain_host in.bin out.bin
//   in:  int32 L, td, input_act, B, dims[L+1], act[L]; float32 t, params (the flat Lux vector), x (B, D)
//   out: float32 f (B, D)
#include "lrnde_math.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using lrnde::act_apply;
using lrnde::fma_;

constexpr int SEG = 112;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hd[4];
  if (fread(hd, 4, 4, fi) != 4) return 2;
  const int L = hd[0], td = hd[1], in_act = hd[2], B = hd[3];
  if (L < 1 || L > 16 || B < 1) return 2;
  std::vector<int32_t> dims(L + 1), act(L);
  if (fread(dims.data(), 4, L + 1, fi) != (size_t)L + 1 || fread(act.data(), 4, L, fi) != (size_t)L) return 2;
  float t;
  if (fread(&t, 4, 1, fi) != 1) return 2;
  size_t P = 0;
  int maxw = 0;
  for (int l = 0; l < L; ++l) P += (size_t)dims[l + 1] * (dims[l] + td) + dims[l + 1];
  for (int l = 0; l <= L; ++l) maxw = dims[l] > maxw ? dims[l] : maxw;
  const int D = dims[0];
  std::vector<float> p(P), x((size_t)B * D), f((size_t)B * D), a(maxw), h(maxw);
  if (fread(p.data(), 4, P, fi) != P || fread(x.data(), 4, x.size(), fi) != x.size()) return 2;
  fclose(fi);
  for (int n = 0; n < B; ++n) {
    for (int k = 0; k < D; ++k) a[k] = act_apply(in_act, x[(size_t)n * D + k]);
    const float* w = p.data();
    for (int l = 0; l < L; ++l) {
      const int in = dims[l], out = dims[l + 1];
      const float* b = w + (size_t)out * (in + td);
      for (int o = 0; o < out; ++o) {
        float tot = 0.f;
        for (int k0 = 0; k0 < in; k0 += SEG) {
          float acc = 0.f;
          const int k1 = k0 + SEG < in ? k0 + SEG : in;
          for (int k = k0; k < k1; ++k) acc = fma_(w[o + (size_t)k * out], a[k], acc);
          tot = k0 == 0 ? acc : tot + acc;
        }
        if (td) tot = fma_(w[o + (size_t)in * out], t, tot);
        tot = tot + b[o];
        h[o] = act_apply(act[l], tot);
      }
      for (int o = 0; o < out; ++o) a[o] = h[o];
      w = b + out;
    }
    for (int k = 0; k < D; ++k) f[(size_t)n * D + k] = a[k];
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  if (fwrite(f.data(), 4, f.size(), fo) != f.size()) return 2;
  fclose(fo);
  return 0;
}

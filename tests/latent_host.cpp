// float32 host restatement of the Latent-ODE encoder forward (Recurrence(LatentGRUCell), rec_to_gen, reparameterisation)
// in the canonical accumulation order of csrc/lrnde_latent.hpp, with the scalar functions of csrc/lrnde_math.hpp.  The GPU
// kernel must return these bits (tests/test_gpu_latent.py); compile with -O2 -ffp-contract=off.
//
//   latent_host in.bin out.bin
//   in:  int32 I, H, L, N, B, T, training; float32 params (the flat Lux vector), x (B, T, 2I+1), eps (B, N)
//   out: float32 y (B, 2L), mu (B, N), logvar (B, N), z0 (B, N)
#include "lrnde_math.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using lrnde::fma_;

struct Dense {
  const float* W;   // column-major out x in
  const float* b;
  int out, in;
};

static const float* take(const float*& p, Dense& d, int out, int in) {
  d.W = p; d.b = p + (size_t)out * in; d.out = out; d.in = in;
  p += (size_t)out * in + out;
  return p;
}

// z[o] = (fma chain from 0 over k of W[o][k] * in[k]) + b[o]
static float plain(const Dense& d, int o, const float* in) {
  float acc = 0.f;
  for (int k = 0; k < d.in; ++k) acc = fma_(d.W[o + (size_t)k * d.out], in[k], acc);
  return acc + d.b[o];
}

// first layer of a gate: the x_t rows (input rows 2L..2L+F-1) first, then the carry rows 0..2L-1
static float gate1(const Dense& d, int o, const float* carry, const float* x, int L2, int F) {
  float acc = 0.f;
  for (int f = 0; f < F; ++f) acc = fma_(d.W[o + (size_t)(L2 + f) * d.out], x[f], acc);
  for (int k = 0; k < L2; ++k) acc = fma_(d.W[o + (size_t)k * d.out], carry[k], acc);
  return acc + d.b[o];
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hd[7];
  if (fread(hd, 4, 7, fi) != 7) return 2;
  const int I = hd[0], H = hd[1], L = hd[2], N = hd[3], B = hd[4], T = hd[5], training = hd[6];
  const int F = 2 * I + 1, K = 2 * L + F;
  const size_t P = (size_t)3 * (H * K + H) + 2 * (L * H + L) + (2 * L * H + 2 * L) + (L * 2 * L + L) + (2 * N * L + 2 * N) + (I * N + I);
  std::vector<float> ps(P), x((size_t)B * T * F), eps((size_t)B * N);
  if (fread(ps.data(), 4, P, fi) != P || fread(x.data(), 4, x.size(), fi) != x.size() || fread(eps.data(), 4, eps.size(), fi) != eps.size())
    return 2;
  fclose(fi);
  const float* p = ps.data();
  Dense u1, u2, r1, r2, n1, n2, e1, e2;
  take(p, u1, H, K); take(p, u2, L, H);
  take(p, r1, H, K); take(p, r2, L, H);
  take(p, n1, H, K); take(p, n2, 2 * L, H);
  take(p, e1, L, 2 * L); take(p, e2, 2 * N, L);
  std::vector<float> y((size_t)B * 2 * L), mu((size_t)B * N), lv((size_t)B * N), z0((size_t)B * N);
  std::vector<float> carry(2 * L), c(2 * L), hu(H), hr(H), hn(H), u(L), r(L), g1(L), o2(2 * N);
  for (int b = 0; b < B; ++b) {
    for (int l = 0; l < L; ++l) { carry[l] = 0.f; carry[L + l] = 1.f; }   // latent_ode.jl:20-21
    for (int t = 0; t < T; ++t) {
      const float* xt = x.data() + ((size_t)b * T + t) * F;
      float ms = 0.f;
      for (int f = F / 2; f < F; ++f) ms = ms + xt[f];                     // :40
      if (!(ms > 0.f)) continue;                                          // :42-43: the carry passes through
      for (int o = 0; o < H; ++o) { hu[o] = lrnde::tanhf_c(gate1(u1, o, carry.data(), xt, 2 * L, F)); hr[o] = lrnde::tanhf_c(gate1(r1, o, carry.data(), xt, 2 * L, F)); }
      for (int l = 0; l < L; ++l) { u[l] = lrnde::sigmoid_c(plain(u2, l, hu.data())); r[l] = lrnde::sigmoid_c(plain(r2, l, hr.data())); }
      for (int l = 0; l < L; ++l) { c[l] = carry[l] * r[l]; c[L + l] = carry[L + l] * r[l]; }   // :31
      for (int o = 0; o < H; ++o) hn[o] = lrnde::tanhf_c(gate1(n1, o, c.data(), xt, 2 * L, F));
      for (int l = 0; l < L; ++l) {
        const float s = lrnde::tanhf_c(plain(n2, L + l, hn.data()));      // new_state_std; rows 0..L-1 are never used (:37)
        const float om = 1.0f - u[l];
        const float nm = om * s + u[l] * carry[l];                        // :37
        const float ns = om * s + u[l] * carry[L + l];                    // :38
        carry[l] = nm; carry[L + l] = ns;
      }
    }
    for (int k = 0; k < 2 * L; ++k) y[(size_t)b * 2 * L + k] = carry[k];
    for (int l = 0; l < L; ++l) g1[l] = lrnde::tanhf_c(plain(e1, l, carry.data()));
    for (int o = 0; o < 2 * N; ++o) o2[o] = plain(e2, o, g1.data());
    for (int i = 0; i < N; ++i) {
      const size_t gi = (size_t)b * N + i;
      mu[gi] = o2[i];
      if (training) {                                                     // common.jl:61-71
        const float pe = lrnde::expf_c(o2[N + i] * 0.5f) * eps[gi];
        lv[gi] = o2[N + i];
        z0[gi] = o2[i] + pe;
      } else {                                                            // common.jl:73-77
        lv[gi] = o2[i];
        z0[gi] = o2[i];
      }
    }
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  fwrite(y.data(), 4, y.size(), fo); fwrite(mu.data(), 4, mu.size(), fo); fwrite(lv.data(), 4, lv.size(), fo); fwrite(z0.data(), 4, z0.size(), fo);
  fclose(fo);
  return 0;
}

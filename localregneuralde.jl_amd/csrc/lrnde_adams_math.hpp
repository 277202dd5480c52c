// lrnde_adams_math.hpp — the scalar arithmetic of VCAB3 / VCABM3, stated once (device + host): the coefficient
// recurrences of an attempt, the per-element predictor, corrector, residual, Bogacki-Shampine 3(2) residual and the
// Hermite record.  lrnde_adams.hpp (the MLP handle's host loop), lrnde_chain_adams.hpp (the coefficients of the small
// chain's one-launch loop) and lrnde_conv_adams.hpp (the conv handle) inline it; the oracle's adams_solve holds its own copy.
//
// Like lrnde_math.hpp: fixed sequences of IEEE-754 fp32 operations compiled with -ffp-contract=off, so an expression has
// the same bits wherever it is inlined.  UPSTREAM-RECALL, parity unpinned: lrnde_adams.hpp says what is recalled of
// OrdinaryDiffEq's Adams methods and what is restated from Hairer, Norsett, Wanner III.5.
#pragma once
#include "lrnde_math.hpp"

namespace lrnde {

// ---- the attempt's scalars: phi*_1, phi*_2 factors (b2, b3) and g_2 .. g_4 folded into what the kernels multiply by ----
// nacc: accepted steps so far; h1, h2: the last two accepted step sizes.  While nacc < 2 (a start-up attempt) only b2 is
// used (nacc == 1: phi*_1 for the first multistep step) and the g's stay zero.
struct AdamsCoef { float b2, b3, g2, g3, cu, ce; };
LRNDE_HD AdamsCoef adams_coef(int nacc, int moulton, float dt, float h1, float h2) {
  const float c21 = 0.5f, c22 = (float)(1.0 / 6.0), c23 = (float)(1.0 / 12.0);   // c_{1,q} = 1/(q(q+1))
  AdamsCoef k;
  k.b2 = nacc >= 1 ? dt / h1 : 0.0f;
  k.b3 = nacc >= 2 ? k.b2 * ((dt + h1) / (h1 + h2)) : 0.0f;
  k.g2 = k.g3 = k.cu = k.ce = 0.0f;
  if (nacc >= 2) {
    const float r1 = dt / (dt + h1);
    const float g3 = c21 - r1 * c22;
    const float c32 = c22 - r1 * c23;
    const float r2 = dt / ((dt + h1) + h2);
    const float g4 = g3 - r2 * c32;
    k.g2 = c21; k.g3 = g3;
    k.cu = dt * g3;                                   // VCABM3's corrector: u += cu * phi_2(n+1)
    k.ce = moulton ? dt * (g4 - g3) : dt * g4;        // the error estimate: ce * phi_3(n+1)
  }
  return k;
}

// ---- per element ----
// phi*_1(n) = b2 * (f_n - f_{n-1})
LRNDE_HD float adams_phi1(float k1, float kprev, float b2) { return b2 * (k1 - kprev); }
// phi*_1, phi*_2 and the predictor (VCAB3: three terms; VCABM3: two)
struct AdamsPred { float v2, v3, u; };
LRNDE_HD AdamsPred adams_predict(float uprev, float k1, float kprev, float sp2, const AdamsCoef& k, float dt, int three) {
  AdamsPred r;
  const float p2 = k1 - kprev;
  r.v2 = k.b2 * p2;
  const float p3 = p2 - sp2;
  r.v3 = k.b3 * p3;
  float sm = k1 + k.g2 * r.v2;
  if (three) sm = sm + k.g3 * r.v3;
  r.u = uprev + dt * sm;
  return r;
}
// phi_j(n+1) from the new evaluation, the corrector (VCABM3) and the squared scaled residual; u is updated in place
LRNDE_HD float adams_correct(float du, float k1, float v2, float v3, float uprev, float& u, float cu, float ce, int moulton,
                             float abstol, float reltol) {
  const float q2 = du - k1;
  const float q3 = q2 - v2;
  const float q4 = q3 - v3;
  if (moulton) u = u + cu * q3;
  const float ut = ce * q4;
  const float sc = abstol + fmaxf_(__builtin_fabsf(uprev), __builtin_fabsf(u)) * reltol;
  const float r = ut / sc;
  return r * r;
}
// Bogacki-Shampine 3(2): the squared scaled residual of the embedded pair
LRNDE_HD float bs3_resid_sq(float k1, float kb2, float kb3, float kend, float uprev, float u, float dt, float abstol, float reltol) {
  const float bt1 = (float)(5.0 / 72.0), bt2 = (float)(-1.0 / 12.0), bt3 = (float)(-1.0 / 9.0), bt4 = 0.125f;
  float sm = bt1 * k1 + bt2 * kb2;
  sm = sm + bt3 * kb3;
  sm = sm + bt4 * kend;
  const float ut = dt * sm;
  const float sc = abstol + fmaxf_(__builtin_fabsf(uprev), __builtin_fabsf(u)) * reltol;
  const float r = ut / sc;
  return r * r;
}
// the step's cubic Hermite interpolant in the record's polynomial form (lrnde_math.hpp: [uprev, k1, P2, P3], P4 = 0)
LRNDE_HD void adams_hermite(float uprev, float u, float k1, float kend, float dt, float& P2, float& P3) {
  const float d = (u - uprev) / dt;
  P2 = (3.0f * d - 2.0f * k1) - kend;
  P3 = (k1 + kend) - 2.0f * d;
}

}  // namespace lrnde

// k_lightcurve_ld: transit depths on the device, limb darkening per wavelength bin
#pragma once
#include "common.h"
#include "k_lightcurve.h"

namespace wayne {

// ---------------------------------------------------------------------------
// k_lightcurve_ld : depth[K][W] with four Claret coefficients PER wavelength bin
// ---------------------------------------------------------------------------
// I(mu) = c0 + sum_n a_n mu^(n/2), c0 = 1 - sum a_n, is linear in the coefficients, and so is the blocked flux:
//   B_n(z, p) = int_{occulted region} mu^(n/2) dA,  n = 0 .. 4           (B_0: the lens area)
//             = 2 pi (1 - mu_f^(n/2+2)) / (n/2+2)                          radii wholly inside the planet
//             + int_{|z-p|}^{min(1,z+p)} mu^(n/2) r theta(r) dr            k_lightcurve's 24-node rule, same nodes, same forms
//   deficit[k][w] = (c0(w) B_0 + sum_n a_n(w) B_n)(z_k, p_w) / (pi (1 - sum_n a_n(w) n/(n+4)))
// One pass over the nodes gives the five sums: float32 integrand, five float64 sums (as k_lightcurve: one).
struct LcLdArgs {
  int K, W;
  const double* z;        // [K]
  const double* hidden;   // [K] or null
  const double* rp;       // [W]
  const double* ld;       // [4][W]: four planes, a_n of bin w at ld[(n-1) * W + w] (a wave's loads coalesce)
  float x[kLcNodes], w[kLcNodes], d[kLcNodes];   // node, weight, distance to the nearer end
  double p_lo, p_hi;      // range of rp over the W wavelengths
  double* depth;          // [K*W]
};

struct LcBasis {
  double b0, b1, b2, b3, b4;   // (named members, not an array: they stay in registers)
};

// B_0 .. B_4 for one (z, p); all zero without a transit.
__device__ __forceinline__ LcBasis lc_basis(const LcLdArgs& a, double z, double p) {
  LcBasis B{0., 0., 0., 0., 0.};
  if (!(z < 1. + p)) return B;
  const double r_full = fmin(fmax(p - z, 0.), 1.);
  const double mu_f = sqrt(1. - r_full * r_full);
  {
    // int_{mu_f}^1 m^(n/2) 2 pi m dm
    const double s = sqrt(mu_f), m2 = mu_f * mu_f;
    B.b0 = 2. * kPi * (1. - m2) / 2.;
    B.b1 = 2. * kPi * (1. - m2 * s) / 2.5;
    B.b2 = 2. * kPi * (1. - m2 * mu_f) / 3.;
    B.b3 = 2. * kPi * (1. - m2 * mu_f * s) / 3.5;
    B.b4 = 2. * kPi * (1. - m2 * m2) / 4.;
  }
  const double ra = fabs(z - p), rb = fmin(1., z + p);
  if (rb > ra) {
    const float L = (float)(rb - ra), raf = (float)ra, zf = (float)z, pf = (float)p;
    const float gap = (float)(1. - rb);            // 1 - rb >= 0
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0.;
#pragma unroll 4
    for (int i = 0; i < kLcNodes; ++i) {
      const float x = a.x[i], dn = a.d[i];
      const float lo = L * (x < 0.5f ? dn : 1.f - dn);    // r - ra
      const float hi = L * (x < 0.5f ? 1.f - dn : dn);    // rb - r
      const float r = raf + lo;
      // the cancellation-free forms of k_lightcurve (lc_deficit)
      const float rmz = r - zf;
      const float num = fmaxf((pf - fabsf(rmz)) * (pf + fabsf(rmz)), 0.f);
      const float den = fmaxf((r + zf - pf) * (r + zf + pf), 0.f);
      const float theta = 4.f * atan2f(sqrtf(num), sqrtf(den));
      const float mu = sqrtf(fmaxf((gap + hi) * (1.f + r), 0.f));   // sqrt((1-r)(1+r))
      const float sm = sqrtf(mu);
      const float g = r * theta * a.w[i];
      s0 += (double)g;
      s1 += (double)(g * sm);
      s2 += (double)(g * mu);
      s3 += (double)(g * (mu * sm));
      s4 += (double)(g * (mu * mu));
    }
    const double Ld = (double)L;
    B.b0 += s0 * Ld; B.b1 += s1 * Ld; B.b2 += s2 * Ld; B.b3 += s3 * Ld; B.b4 += s4 * Ld;
  }
  return B;
}

// The grid and the decisions of k_lightcurve: one workgroup per sub-sample; the five B_n(z_k, .) are analytic in p
// wherever the deficit is, so outside a regime change they are evaluated at the kLcCheb Lobatto points of [p_lo, p_hi]
// only -- five interpolants -- and every wavelength evaluates five Clenshaw recurrences with its own p, combines them
// with its own four coefficients and divides by its own disk flux.
__global__ __launch_bounds__(256) void k_lightcurve_ld(LcLdArgs a) {
  static_assert(kLcCheb * kLcCheb == 256, "one thread per entry of the cosine table");
  static_assert(5 * kLcCheb <= 256, "one thread per Chebyshev coefficient");
  constexpr int n = kLcCheb - 1;
  const int k = blockIdx.x;
  __shared__ double s_f[5][kLcCheb];   // samples of B_0 .. B_4 at the Lobatto points
  __shared__ double s_c[5][kLcCheb];   // their Chebyshev coefficients (first and last halved)
  __shared__ double s_cos[kLcCheb][kLcCheb];
  const double z = a.z[k];
  const double p_lo = a.p_lo, p_hi = a.p_hi;
  const double width = p_hi - p_lo;
  const LcRoute route = lc_route(z, p_lo, p_hi);   // (k_lightcurve.h)
  const bool no_transit = route.no_transit, direct = route.direct, flat = route.flat;
  if (!direct && !no_transit) {
    const int tm = threadIdx.x / kLcCheb, tj = threadIdx.x % kLcCheb;
    s_cos[tm][tj] = cos((double)(tm * tj) * kPi / (double)n);
    if (threadIdx.x < kLcCheb) {
      const double t = cos((double)threadIdx.x * kPi / (double)n);
      const LcBasis B = lc_basis(a, z, 0.5 * (p_lo + p_hi) + 0.5 * width * t);
      s_f[0][threadIdx.x] = B.b0; s_f[1][threadIdx.x] = B.b1; s_f[2][threadIdx.x] = B.b2;
      s_f[3][threadIdx.x] = B.b3; s_f[4][threadIdx.x] = B.b4;
    }
    __syncthreads();
    if (threadIdx.x < 5 * kLcCheb) {
      const int q = threadIdx.x / kLcCheb, m = threadIdx.x % kLcCheb;
      double acc = 0.5 * (s_f[q][0] * s_cos[m][0] + s_f[q][n] * s_cos[m][n]);
      for (int j = 1; j < n; ++j) acc += s_f[q][j] * s_cos[m][j];
      acc *= 2. / (double)n;
      s_c[q][m] = (m == 0 || m == n) ? 0.5 * acc : acc;
    }
    __syncthreads();
  }
  const double hid = a.hidden ? a.hidden[k] : 0.;
  for (int w = threadIdx.x; w < a.W; w += blockDim.x) {
    const double p = a.rp[w];
    const bool sized = p == p;   // (a NaN radius ratio: no transit and no eclipse term, as in k_lightcurve)
    double deficit = 0.;   // 1 - transit
    if (!no_transit && sized) {
      LcBasis B;
      if (direct) {
        B = lc_basis(a, z, p);
      } else if (flat) {
        B.b0 = s_f[0][0]; B.b1 = s_f[1][0]; B.b2 = s_f[2][0]; B.b3 = s_f[3][0]; B.b4 = s_f[4][0];
      } else {
        const double t = (2. * p - (p_lo + p_hi)) / width;
        double u1[5] = {0., 0., 0., 0., 0.}, u2[5] = {0., 0., 0., 0., 0.};
#pragma unroll
        for (int m = n; m >= 1; --m) {
#pragma unroll
          for (int q = 0; q < 5; ++q) {
            const double u0 = s_c[q][m] + 2. * t * u1[q] - u2[q];
            u2[q] = u1[q];
            u1[q] = u0;
          }
        }
        B.b0 = s_c[0][0] + t * u1[0] - u2[0];
        B.b1 = s_c[1][0] + t * u1[1] - u2[1];
        B.b2 = s_c[2][0] + t * u1[2] - u2[2];
        B.b3 = s_c[3][0] + t * u1[3] - u2[3];
        B.b4 = s_c[4][0] + t * u1[4] - u2[4];
      }
      const double a1 = a.ld[w], a2 = a.ld[(size_t)a.W + w], a3 = a.ld[2 * (size_t)a.W + w], a4 = a.ld[3 * (size_t)a.W + w];
      const double c0 = 1. - a1 - a2 - a3 - a4;
      const double f0 = kPi * (1. - (a1 * (1. / 5.) + a2 * (2. / 6.) + a3 * (3. / 7.) + a4 * (4. / 8.)));
      deficit = (c0 * B.b0 + a1 * B.b1 + a2 * B.b2 + a3 * B.b3 + a4 * B.b4) / f0;
    }
    // eclipse term, unchanged (k_lightcurve)
    double ecl = 0.;
    if (a.hidden && sized) {
      const double f = p * p;
      ecl = f * hid / (1. + f);
    }
    a.depth[(size_t)k * a.W + w] = deficit + ecl;
  }
}

}  // namespace wayne

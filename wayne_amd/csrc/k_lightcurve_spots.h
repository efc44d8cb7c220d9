// k_lightcurve_spots: star spots in the device light curves, occulted and unocculted
#pragma once
#include "common.h"

namespace wayne {

// ---------------------------------------------------------------------------
// k_lightcurve_spots : depth[K][W] of a spotted star, in place, behind k_lightcurve / k_lightcurve_ld
// ---------------------------------------------------------------------------
// wayne_amd/spots.py states the law in numpy.  Spot i is a circle in projection (centre C_i, radius r_i, contrast c_{i,w});
// with I(mu) = c0 + sum_n a_n mu^(n/2), a'_0 = c0 = 1 - sum a_n, a'_n = a_n, F0_w = pi (1 - sum a_n n/(n+4)):
//   Q_n(P, C, p, r) = int_{planet disc n spot disc} mu^(n/2) dA            lens_basis: a fixed 2 x 10 x 10 Gauss-Legendre rule
//   S_{i,n} = Q_n(C_i, C_i, r_i, r_i)                                       the whole spot (host, the same function)
//   D_w     = sum_i (1 - c_{i,w}) sum_n a'_n(w) S_{i,n}
//   X_{k,w} = sum_i (1 - c_{i,w}) sum_n a'_n(w) Q_n(P_k, C_i, p_w, r_i)
//   depth'[k][w] = (depth[k][w] F0_w - X_{k,w}) / (F0_w - D_w)              rows with z_k < 10 and hidden_k = 0, sized columns
// float64 throughout, no contracted multiply-adds (the library's -ffp-contract=off): host and device run the same
// operations in the same order; they differ in sin / cos / acos alone.
constexpr int kSpotMax = 8;
constexpr int kSpotNodes = 10;

struct SpotRule {
  double g[kSpotNodes], w[kSpotNodes];   // numpy.polynomial.legendre.leggauss(10): the bits the numpy law uses
};

// One panel of the rule: phi in [lo, hi], t = cc - sg rad cos phi along u, half-chord h = rad sin phi along v.
__host__ __device__ inline void spot_panel(const SpotRule& gl, double px, double py, double ux, double uy, double cc,
                                           double rad, double sg, double lo, double hi, double& q0, double& q1, double& q2,
                                           double& q3, double& q4) {
  const double vx = -uy, vy = ux;
  const double mid = 0.5 * (lo + hi), half = 0.5 * (hi - lo);
  for (int a = 0; a < kSpotNodes; ++a) {
    const double phi = mid + half * gl.g[a];
    const double sn = sin(phi);
    const double t = cc - sg * rad * cos(phi);
    const double h = rad * sn;
    const double wa = gl.w[a] * half * rad * sn * h;
    const double bx = px + t * ux, by = py + t * uy;
    for (int b = 0; b < kSpotNodes; ++b) {
      const double s = h * gl.g[b];
      const double x = bx + s * vx, y = by + s * vy;
      const double mu = sqrt(fmax(1. - x * x - y * y, 0.));
      const double sm = sqrt(mu);
      const double wab = wa * gl.w[b];
      q0 += wab;
      q1 += wab * sm;
      q2 += wab * mu;
      q3 += wab * (mu * sm);
      q4 += wab * (mu * mu);
    }
  }
}

// Q_0 .. Q_4 over (disc of radius p at P) n (disc of radius r at C).  d >= p + r is decided before any node is touched.
__host__ __device__ inline void lens_basis(const SpotRule& gl, double px, double py, double cx, double cy, double p,
                                           double r, double& q0, double& q1, double& q2, double& q3, double& q4) {
  q0 = q1 = q2 = q3 = q4 = 0.;
  const double dx = cx - px, dy = cy - py;
  const double d = sqrt(dx * dx + dy * dy);
  if (!(d < p + r)) return;
  double ux = 1., uy = 0.;
  if (d > 0.) { ux = dx / d; uy = dy / d; }
  const double kHalfPi = 0.5 * kPi;
  if (d <= fabs(p - r)) {
    // the lens is the smaller circle
    const double rho = fmin(p, r), tc = r <= p ? d : 0.;
    spot_panel(gl, px, py, ux, uy, tc, rho, 1., 0., kHalfPi, q0, q1, q2, q3, q4);
    spot_panel(gl, px, py, ux, uy, tc, rho, 1., kHalfPi, kPi, q0, q1, q2, q3, q4);
    return;
  }
  const double ts = (d * d + p * p - r * r) / (2. * d);
  const double phi1 = acos(fmin(fmax((d - ts) / r, -1.), 1.));
  const double phi2 = acos(fmin(fmax(ts / p, -1.), 1.));
  spot_panel(gl, px, py, ux, uy, d, r, 1., 0., phi1, q0, q1, q2, q3, q4);     // bounded by the spot's circle
  spot_panel(gl, px, py, ux, uy, 0., p, -1., 0., phi2, q0, q1, q2, q3, q4);   // bounded by the planet's circle
}

struct SpotArgs {
  int K, W, n;
  const double* z;          // [K]
  const double* hidden;     // [K] or null
  const double* rp;         // [W]
  const double* px;         // [K] the planet's track
  const double* py;         // [K]
  const double* ld;         // a_n of bin w at ld[(n-1) * ld_plane + w * ld_step]: the table's planes (W, 1) or lc_ld (1, 0)
  size_t ld_plane, ld_step;
  const double* contrast;   // [n][W] (a wave's loads coalesce)
  double cx[kSpotMax], cy[kSpotMax], r[kSpotMax];
  double S[kSpotMax][5];    // the whole spots' integrals (host)
  SpotRule gl;
  double* depth;            // [K*W], rewritten in place
};

// Grid: K x (tiles of 256 wavelengths) -- the sub-sample on x, which has the wider range; a thread owns one (k, w) and
// walks the spots.  No atomics, no LDS.
__global__ __launch_bounds__(256) void k_lightcurve_spots(SpotArgs a) {
  const int k = blockIdx.x;
  const int w = blockIdx.y * 256 + threadIdx.x;
  if (k >= a.K || w >= a.W) return;
  if (!(a.z[k] < 10.)) return;                      // behind the star: the eclipse term alone, unchanged
  if (a.hidden && a.hidden[k] != 0.) return;
  const double p = a.rp[w];
  if (!(p == p)) return;                            // a planet of no size
  const double a1 = a.ld[w * a.ld_step], a2 = a.ld[a.ld_plane + w * a.ld_step];
  const double a3 = a.ld[2 * a.ld_plane + w * a.ld_step], a4 = a.ld[3 * a.ld_plane + w * a.ld_step];
  const double c0 = 1. - a1 - a2 - a3 - a4;
  const double f0 = kPi * (1. - (a1 * (1. / 5.) + a2 * (2. / 6.) + a3 * (3. / 7.) + a4 * (4. / 8.)));
  const double px = a.px[k], py = a.py[k];
  double D = 0., X = 0.;
  for (int i = 0; i < a.n; ++i) {
    const double dark = 1. - a.contrast[(size_t)i * a.W + w];
    D = D + dark * ((((c0 * a.S[i][0] + a1 * a.S[i][1]) + a2 * a.S[i][2]) + a3 * a.S[i][3]) + a4 * a.S[i][4]);
    double q0, q1, q2, q3, q4;
    lens_basis(a.gl, px, py, a.cx[i], a.cy[i], p, a.r[i], q0, q1, q2, q3, q4);
    X = X + dark * ((((c0 * q0 + a1 * q1) + a2 * q2) + a3 * q3) + a4 * q4);
  }
  const size_t at = (size_t)k * a.W + w;
  a.depth[at] = (a.depth[at] * f0 - X) / (f0 - D);
}

}  // namespace wayne

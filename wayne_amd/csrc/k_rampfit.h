// k_ramp_fit: the up-the-ramp fit of every pixel of an exposure's reads, on the device (wayne_exposure_set_rampfit;
// opt-in; no reference counterpart -- the law is the one tests/rampfit_law.py states in numpy, per pixel).
//
// All coordinates bordered, side S; everything in float64; a read of any stored type is promoted exactly.  For a
// light-sensitive pixel, with L_k, g and the step bits the extraction's (k_extract.h: extract_linear, the gain factor of
// extract_term; the gain step is required) and rn the read noise of a difference of two reads:
//   e_0 = 0, e_k = L_k g
//   K   = the largest K <= R with P_k < sat_dn for every 1 <= k <= K, and K = 0 if not P_0 < sat_dn
//         (a NaN read is not < sat_dn; a sample behind a saturated one is never used)
//   d_j = e_{j+1} - e_j,  r_j = d_j / dt_j,  j = 0 .. K-1;   G = {0 .. K-1}
//   med(G) = the element of rank floor((|G| - 1) / 2) of {r_j : j in G} ascending (the lower median; equal values in
//            order of j); 0 for an empty G
//   jump test (k_jump > 0), repeated while |G| >= 3:
//     m = med(G), f0 = max(m, 0),  z_j = (d_j - m dt_j) / sqrt(f0 dt_j + rn^2) for j in G,  j* = the lowest j with the largest z_j
//     z_j* > k_jump ? G <- G \ {j*}, bit j* of `jump` set : stop            (upward jumps only: a ray adds charge)
//   fit: f0 = max(med(G), 0);  a_j = f0 dt_j + rn^2;  o = -rn^2 / 2
//     the generalised least squares of d = f dt over j in G with cov(d_j, d_j) = a_j and cov(d_j, d_j+1) = o when both are
//     in G (two differences that share a read share its noise; a removed interval cuts the chain), solved as written:
//     ascending j:  j not in G: c_j = y_j = 0.  j in G: link = (j-1 in G); den = a_j - (link ? o c_{j-1} : 0);
//                   c_j = (j+1 in G) ? o / den : 0;   y_j = (dt_j - (link ? o y_{j-1} : 0)) / den
//     descending j: w_j = y_j - c_j w_{j+1}   (w_K = 0)
//     num = sum_{j in G, ascending} w_j d_j      den = sum_{j in G, ascending} w_j dt_j
//   rate = den > 0 ? num / den : 0  [e-/s]     var = den > 0 ? 1 / den : 0     word = K << 16 | jump
// Reference pixels (the 5-pixel border) get rate = var = word = 0 and are not loaded.
//
// One thread per pixel, 256-thread workgroups over S S.  A pixel's loads -- R + 1 reads, R dark values, four linearity
// coefficients, the pixel flat -- do not depend on each other and are all issued before the arithmetic.  d_j, r_j and the
// recurrence's c_j, y_j live in registers: every loop over the intervals is fully unrolled over kMaxReads with the
// interval count as a predicate, G and jump are bit masks, and no register array is indexed by a run-time value, so
// nothing goes to scratch (dt_j, uniform, comes from the kernel's arguments).  The median is a rank count (|G|^2
// comparisons) with a predicated select; the last jump pass's median is the fit's when that pass flagged nothing.  The
// jump loop is a divergent loop: a wave leaves it when none of its lanes has a hit.  No LDS, no atomics: the planes are a
// function of the reads alone -- the same bytes in any slot, on either stream, on every run.
//
// The file is compiled without FMA contraction (wayne_amd/build.py), and float64 divide and sqrt are correctly rounded,
// so a pixel's chain rounds as the numpy statement of it does.
#pragma once
#include "common.h"

namespace wayne {

constexpr int kRampFitThreads = 256;

struct RampFitArgs {
  int R, S;
  unsigned steps;                    // X_LINEARISE | X_DARK | X_GAIN (plan::rampfit_desc_error)
  double dt[kMaxReads];              // read intervals (s)
  double rn2, k_jump, sat_dn;        // rn^2; k_jump = 0: no jump test
  const void* reads;                 // [(R+1)*S*S] float, double or uint16_t
  const float* pfl;                  // [S*S] bordered (1 on the border) or null
  const float* lin[4];               // [S*S] or null
  const float* dark;                 // [R*S*S] or null
  double* rate;                      // [S*S] e-/s
  double* var;                       // [S*S] (e-/s)^2
  uint32_t* word;                    // [S*S] K << 16 | jump
};

// med(G) of the values r[] (a rank count: the member with exactly (|G| - 1) / 2 members in front of it)
__device__ __forceinline__ double rampfit_median(const double (&r)[kMaxReads], unsigned G) {
  const int target = (__popc(G) - 1) >> 1;
  double med = 0.;
#pragma unroll
  for (int j = 0; j < kMaxReads; ++j) {
    int rank = 0;
#pragma unroll
    for (int i = 0; i < kMaxReads; ++i) {
      if (i == j) continue;
      const bool front = i < j ? r[i] <= r[j] : r[i] < r[j];
      rank += (int)(((G >> i) & 1u) && front);
    }
    if (((G >> j) & 1u) && rank == target) med = r[j];
  }
  return med;
}

template <class T>
__global__ void __launch_bounds__(kRampFitThreads) k_ramp_fit(RampFitArgs a) {
  const int S = a.S, R = a.R;
  const size_t SS = (size_t)S * S;
  const size_t pix = (size_t)blockIdx.x * kRampFitThreads + threadIdx.x;
  if (pix >= SS) return;
  const int y = (int)(pix / (size_t)S), x = (int)(pix - (size_t)y * S);
  if (x < kBorder || x >= S - kBorder || y < kBorder || y >= S - kBorder) {
    a.rate[pix] = 0.;
    a.var[pix] = 0.;
    a.word[pix] = 0u;
    return;
  }
  const T* reads = (const T*)a.reads;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool dark = (a.steps & X_DARK) && a.dark;

  // every load of the pixel, then the arithmetic
  T P[kMaxReads + 1];
  float dk[kMaxReads];
  float cf[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k <= kMaxReads; ++k) P[k] = k <= R ? reads[(size_t)k * SS + pix] : (T)0;
#pragma unroll
  for (int k = 0; k < kMaxReads; ++k) dk[k] = (dark && k < R) ? a.dark[(size_t)k * SS + pix] : 0.f;
  if (lin) {
#pragma unroll
    for (int i = 0; i < 4; ++i) cf[i] = a.lin[i][pix];
  }
  const float pf = a.pfl ? a.pfl[pix] : 1.f;

  const double g = a.pfl ? 2.35 / (double)pf : 2.35;
  const double c0 = (double)cf[0], c1 = (double)cf[1], c2 = (double)cf[2], c3 = (double)cf[3];
  const double p0 = (double)P[0];

  // K, d_j, r_j
  int K = 0;
  bool good = p0 < a.sat_dn;
  double d[kMaxReads], r[kMaxReads];
  double e_lo = 0.;
#pragma unroll
  for (int j = 0; j < kMaxReads; ++j) {
    d[j] = 0.; r[j] = 0.;
    if (j < R) {
      const double Pk = (double)P[j + 1];
      good = good && Pk < a.sat_dn;
      K += (int)good;
      const double D = Pk - p0;
      double L = lin ? D * (1.0 + c0 + D * (c1 + D * (c2 + c3 * D))) : D;
      if (dark) L -= (double)dk[j];
      const double e = L * g;
      d[j] = e - e_lo;
      r[j] = d[j] / a.dt[j];
      e_lo = e;
    }
  }
  unsigned G = (1u << K) - 1u, jump = 0u;

  // the jump test
  double m = 0.;
  bool m_is_of_G = false;
  bool go = a.k_jump > 0. && K >= 3;
  while (go) {
    m = rampfit_median(r, G);
    const double f0 = fmax(m, 0.);
    double best = -__builtin_inf();
    int js = 0;
#pragma unroll
    for (int j = 0; j < kMaxReads; ++j) {
      if ((G >> j) & 1u) {
        const double z = (d[j] - m * a.dt[j]) / sqrt(f0 * a.dt[j] + a.rn2);
        if (z > best) { best = z; js = j; }
      }
    }
    if (best > a.k_jump) {
      G &= ~(1u << js);
      jump |= 1u << js;
      go = __popc(G) >= 3;
    } else {
      go = false;
      m_is_of_G = true;
    }
  }
  if (!m_is_of_G) m = rampfit_median(r, G);

  // the fit
  const double f0 = fmax(m, 0.);
  const double o = -a.rn2 / 2;
  double c[kMaxReads], yv[kMaxReads];
  double c_lo = 0., y_lo = 0.;
#pragma unroll
  for (int j = 0; j < kMaxReads; ++j) {
    c[j] = 0.; yv[j] = 0.;
    if ((G >> j) & 1u) {
      const bool link = j > 0 && ((G >> (j - 1)) & 1u);
      const bool next = j + 1 < kMaxReads && ((G >> (j + 1)) & 1u);
      const double aj = f0 * a.dt[j] + a.rn2;
      const double den = aj - (link ? o * c_lo : 0.);
      c[j] = next ? o / den : 0.;
      yv[j] = (a.dt[j] - (link ? o * y_lo : 0.)) / den;
    }
    c_lo = c[j]; y_lo = yv[j];
  }
  // descending: w_j into yv[j]
  double w_hi = 0.;
#pragma unroll
  for (int j = kMaxReads - 1; j >= 0; --j) {
    w_hi = yv[j] - c[j] * w_hi;
    yv[j] = w_hi;
  }
  double num = 0., den = 0.;
#pragma unroll
  for (int j = 0; j < kMaxReads; ++j) {
    if ((G >> j) & 1u) {
      num += yv[j] * d[j];
      den += yv[j] * a.dt[j];
    }
  }
  const bool ok = den > 0.;
  a.rate[pix] = ok ? num / den : 0.;
  a.var[pix] = ok ? 1. / den : 0.;
  a.word[pix] = ((unsigned)K << 16) | jump;
}

}  // namespace wayne

// k_extract: column spectra of an exposure from its reads, on the device (wayne_exposure_set_extraction; no reference
// counterpart -- the law is the observer's extraction that tests/visit_science.py states in numpy, per column).
//
// All coordinates bordered, side S; everything in float64; a read of any stored type is promoted exactly.
//   D_r = P_r - P_0,   L_r = D_r (1 + c1 + D_r (c2 + D_r (c3 + c4 D_r))) - dark_r,   L_0 = 0
//   I_r = (L_r - L_{r-1}) g,   g = 2.35 / pfl (a float64 divide; 2.35 on the border),   T = master sky (0 on the border)
//   product j < R (read interval j), rows [lo_j, hi_j):  A_j[x] = sum_y I_{j+1}[y, x],  B_j[x] = dt_j sum_y T[y, x]
//   product R (the last read alone), rows [lo_R, hi_R):  A_R[x] = sum_y L_R[y, x] g,    B_R[x] = (sum_j dt_j) sum_y T[y, x]
//   sky_j = sum_{x in [b0, b1)} A_j[x] / sum_{x in [b0, b1)} B_j[x]  (0 when the denominator is 0)
//   spectra_j[x] = A_j[x] - sky_j B_j[x]
//
// The result is a function of the exposure alone: no atomics, and every sum is taken in an order fixed by the constants
// below, never by the launch.  k_extract_rows: one workgroup per (64-column tile, chunk of kExtractRows rows of a
// product's window) -- the chunks of all products in one list, product by product, so that no workgroup is launched
// for nothing; wave w of its kExtractWaves takes rows w, w + kExtractWaves, ... of the chunk in ascending
// order -- a wave reads 64 consecutive pixels of a plane per row -- and the waves' sums are added in wave order.  The
// partial sums go to the slot's scratch [A | T][chunk][product][S]; k_extract_finish (one workgroup per product) adds
// the chunks in ascending order, forms sky_j and writes spectra and sky.
//
// The file is compiled without FMA contraction (wayne_amd/build.py), so a pixel's chain rounds as the numpy statement
// of it does; what differs from numpy is the order of the row sums alone.
#pragma once
#include "common.h"

namespace wayne {

// (kExtractRows, kExtractProducts and the step bits X_*: plan_consts.h, shared with the host's validator)
constexpr int kExtractWaves = 8;      // waves of a k_extract_rows workgroup: 4 rows of a chunk each
constexpr int kExtractThreads = 64 * kExtractWaves;

struct ExtractArgs {
  int R, S;
  unsigned steps;
  int bg_lo, bg_hi;
  int n_chunks;                      // chunks of the longest window: the scratch's leading dimension
  int first_chunk[kExtractProducts + 1];   // k_extract_rows: blockIdx.y in [first_chunk[p], first_chunk[p + 1]) works on product p
  int row_lo[kExtractProducts], row_hi[kExtractProducts];   // product j at j, the last read at R
  double scale[kExtractProducts];    // dt_j; at R: sum_j dt_j
  const void* reads;                 // [(R+1)*S*S] float, double or uint16_t
  const float* pfl;                  // [S*S] bordered (1 on the border) or null
  const float* sky;                  // [S*S] bordered (0 on the border) or null
  const float* lin[4];               // [S*S] or null
  const float* dark;                 // [R*S*S] or null
  double* part;                      // [2][n_chunks][R+1][S]: sums of A, then sums of T
  double* spectra;                   // [(R+1)*S]
  double* sky_out;                   // [R+1]
};

// L_r of one pixel (r >= 1); `lin`: the four coefficients are in c[]
template <class T>
__device__ __forceinline__ double extract_linear(const ExtractArgs& a, const T* reads, size_t SS, size_t pix, int r,
                                                 double p0, bool lin, const double* c) {
  const double D = (double)reads[(size_t)r * SS + pix] - p0;
  double L = lin ? D * (1.0 + c[0] + D * (c[1] + D * (c[2] + c[3] * D))) : D;
  if ((a.steps & X_DARK) && a.dark) L -= (double)a.dark[(size_t)(r - 1) * SS + pix];
  return L;
}

template <class T>
__global__ void __launch_bounds__(kExtractThreads) k_extract_rows(ExtractArgs a) {
  int p = 0;
  while (p < a.R && (int)blockIdx.y >= a.first_chunk[p + 1]) ++p;     // (wave-uniform: at most R steps)
  const int chunk = (int)blockIdx.y - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  if (lo >= hi) return;                                  // (never: the list holds a window's own chunks only)
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int x = (int)blockIdx.x * 64 + lane;
  const int S = a.S;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  // product p < R: reads p + 1 and p; the last read: R and nothing (L_0 = 0)
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  double sA = 0., sT = 0.;
  if (x < S) {
    for (int y = lo + wave; y < hi; y += kExtractWaves) {
      const size_t pix = (size_t)y * S + x;
      const double p0 = (double)reads[pix];
      double c[4] = {0., 0., 0., 0.};
      if (lin)
        for (int i = 0; i < 4; ++i) c[i] = (double)a.lin[i][pix];
      const double Lh = extract_linear<T>(a, reads, SS, pix, r_hi, p0, lin, c);
      const double Ll = r_lo > 0 ? extract_linear<T>(a, reads, SS, pix, r_lo, p0, lin, c) : 0.;
      const double g = (a.steps & X_GAIN) ? (gain ? 2.35 / (double)a.pfl[pix] : 2.35) : 1.0;
      sA += (Lh - Ll) * g;
      if (sky) sT += (double)a.sky[pix];
    }
  }
  __shared__ double sh[2][kExtractWaves][64];
  sh[0][wave][lane] = sA;
  sh[1][wave][lane] = sT;
  __syncthreads();
  if (wave == 0 && x < S) {
    double tA = sh[0][0][lane], tT = sh[1][0][lane];
    for (int w = 1; w < kExtractWaves; ++w) { tA += sh[0][w][lane]; tT += sh[1][w][lane]; }
    const int NP = a.R + 1;
    const size_t at = ((size_t)chunk * NP + p) * S + x;
    a.part[at] = tA;
    a.part[(size_t)a.n_chunks * NP * S + at] = tT;
  }
}

__global__ void __launch_bounds__(kExtractThreads) k_extract_finish(ExtractArgs a) {
  const int p = (int)blockIdx.x, S = a.S, NP = a.R + 1;
  const int tid = (int)threadIdx.x;
  if (p == a.R && !(a.steps & X_LAST_READ)) {            // the last-read product was not asked for: zeros
    for (int x = tid; x < S; x += kExtractThreads) a.spectra[(size_t)p * S + x] = 0.;
    if (tid == 0) a.sky_out[p] = 0.;
    return;
  }
  __shared__ double shA[kExtractMaxS], shB[kExtractMaxS];
  __shared__ double shR[2][64];
  __shared__ double sh_sky;
  const int rows = a.row_hi[p] - a.row_lo[p];
  const int chunks = (rows + kExtractRows - 1) / kExtractRows;
  const size_t half = (size_t)a.n_chunks * NP * S;
  for (int x = tid; x < S; x += kExtractThreads) {
    double A = 0., T = 0.;
    for (int c = 0; c < chunks; ++c) {                   // ascending chunks
      const size_t at = ((size_t)c * NP + p) * S + x;
      A += a.part[at];
      T += a.part[half + at];
    }
    shA[x] = A;
    shB[x] = a.scale[p] * T;
  }
  __syncthreads();
  if (tid < 64) {
    double sa = 0., sb = 0.;
    for (int x = a.bg_lo + tid; x < a.bg_hi; x += 64) { sa += shA[x]; sb += shB[x]; }
    shR[0][tid] = sa;
    shR[1][tid] = sb;
  }
  __syncthreads();
  if (tid == 0) {
    double sa = 0., sb = 0.;
    for (int l = 0; l < 64; ++l) { sa += shR[0][l]; sb += shR[1][l]; }
    sh_sky = ((a.steps & X_SKY) && sb != 0.) ? sa / sb : 0.;
    a.sky_out[p] = sh_sky;
  }
  __syncthreads();
  const double s = sh_sky;
  for (int x = tid; x < S; x += kExtractThreads) a.spectra[(size_t)p * S + x] = shA[x] - s * shB[x];
}

}  // namespace wayne

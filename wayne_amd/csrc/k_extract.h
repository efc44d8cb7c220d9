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
// Cosmic-ray rejection (wayne_exposure_set_crrej; off unless asked for -- the instantiations launched without it are
// those of the lines above).  For read interval j, I = I_{j+1}; a pixel is tested iff it lies kCrMargin pixels inside the
// frame and in the mask rows [min_p lo_p, max_p hi_p):
//   m8 = max of I[y+-1, x], I[y+-2, x], I[y, x+-1], I[y, x+-2],   d = I[y, x] - m8
//   flag_j[y, x] <=> d > 0 and d d > k^2 (rn^2 + max(m8, 0))
//   repl_j[y, x] = 0.5 (b + c), b <= c the middle two of I[y, x-2], I[y, x-1], I[y, x+1], I[y, x+2]
//   A_j sums flag_j ? repl_j : I_{j+1};   A_R sums L_R g - sum_j flag_j (I_{j+1} - repl_j)
// k_extract_crmask<T>: one workgroup per (64-column tile, 32-row chunk of the mask rows).  A thread keeps P_0, c1..c4, g
// and L_{r-1} of its (at most 5) pixels of the tile and its 2-pixel halo in registers over the loop on r; I_r of the tile
// goes to LDS (two buffers, so one barrier per read), then 4 pixels per thread are tested.  Every read plane is loaded
// once.  Bit j of the slot's uint16 plane is flag_j; every pixel of the mask rows is stored, so a second run rewrites the
// plane.  k_extract_rows<T, true> loads the pixel's mask word; a set bit is the rare, divergent path that forms repl_j
// from the row neighbours' I_{j+1}.  The flags of a chunk are counted per column beside the partial sums and
// k_extract_finish<true> adds them up: n_rejected[p], behind sky.
//
// Wavelength-binned channels (wayne_exposure_set_channels; off unless asked for -- the three kernels above are launched
// as before and are not touched by it).  With v the term A_p sums for a pixel, t = T[y, x], C channels with edges e[] (um)
// and the row's wavelength solution lambda_y(u) = wl_a[y] + wl_b[y] u:
//   ua_b(y) = (e[b] - wl_a[y]) / wl_b[y],   w_b(y, x) = min(max(min(x + 1, ua_{b+1}) - max(x, ua_b), 0), 1)
//   F(y, x) = the flat cube's cubic at lambda_y(x), rounded to float32 (1 without WAYNE_C_FLAT, on the border, where <= 0)
//   P_p[b] = sum_y sum_x w_b (v / F),   Q_p[b] = scale_p sum_y sum_x w_b (t / F),   channels_p[b] = P_p[b] - sky_p Q_p[b]
// k_extract_bins<T, CR>: one workgroup per (chunk of the list above, group of 8 consecutive rows of it) -- a chunk alone
// gives too few workgroups for the device (68 for the first order on the full array); wave w takes row w of the group,
// walks it over the column hull [u_lo, u_hi) of the plan in 64-column strips into LDS, then lane = channel gathers its
// columns in ascending x; the waves are added in wave order -> scratch [chunk][group][p][2][C].  k_extract_bins_finish,
// behind k_extract_finish for sky_p, adds the groups of a chunk and then the chunks in ascending order.
//
// Variances (wayne_exposure_set_variance; off unless asked for -- VAR = false gives the instantiations of the lines above,
// and those are the ones launched without it).  With v as above, g the gain factor, q = g / 2.35 and rn the read noise of
// a difference of two reads (every product is one):
//   var_p(y, x) = max(v, 0) + rn^2 (q q)
//   VA_p[x] = sum_y var_p,   sky_var_p = sum_{x in bg} VA_p[x] / (sum_{x in bg} B_p[x])^2  (0 where sky_p is 0 by its rule)
//   spectra_var_p[x] = VA_p[x] + (B_p[x] B_p[x]) sky_var_p
//   VP_p[b] = sum_y sum_x (w_b w_b) (var_p / (F F)),   channels_var_p[b] = VP_p[b] + (Q_p[b] Q_p[b]) sky_var_p
// No plane is read for them: a pixel's variance is formed from the v and g its flux was formed from, and summed in the
// order of the flux sums (k_extract_rows / _finish: a third sum beside A and T -> part_v [chunk][product][S]).
// k_extract_bins<.., true> keeps the 48 KB of LDS, and with them three workgroups per CU: a lane holds var / F^2 of its
// (at most 6) columns of the row in registers while the channels gather v / F and t / F, then the wave writes them over
// its v / F buffer and the channels gather them with w^2 -- one more pair of barriers and the weights formed twice, against
// a third 24 KB row buffer that would leave two workgroups per CU.  The waves' sums [wave][C] lie behind [wave][2][C].
// With rejection the row's chain is the register peak, so the VAR instantiations load the channel edges behind it: 117
// VGPRs, 4 waves / SIMD as without variances (loaded ahead of it: 137 and 3).  No instantiation uses scratch memory.
//
// Optimal (profile-weighted) extraction (wayne_exposure_set_optimal, on top of the variances; off unless asked for -- the
// kernels above are launched as before and are not touched by it).  With v, t, g and rn as above, bt = scale_p t,
// q = g / 2.35, H the profile's half width in columns (1 .. kOptMaxH) and sky_p, spectra_p, spectra_var_p, sky_var_p the
// values k_extract_finish wrote:
//   d(y, x)  = v - sky_p bt,   X(x) = [max(x - H, 0), min(x + H, S - 1)]
//   S1(y, x) = sum_{x' in X(x), ascending} d(y, x')
//   S0(x)    = sum_{x' in X(x), ascending} spectra_p[x'],   SV0(x) = the same sum of spectra_var_p
//   ok(x)   <=> S0 > 0 and S0 S0 > 9 SV0            (the source is detected at 3 sigma over the 2H + 1 columns)
//   Pr = S1 / S0,   P = max(Pr, 0)                  (sum_y S1 = S0 by construction: Pr sums to 1 over the window)
//   V(y, x)  = max(spectra_p[x] Pr + sky_p bt, 0) + rn^2 (q q)
//   U_p[x] = sum_y (P d) / V,   W_p[x] = sum_y (P P) / V,   G_p[x] = sum_y (P bt) / V
//   optimal_p[x]     = ok and W > 0 ? U / W                          : spectra_p[x]
//   optimal_var_p[x] = ok and W > 0 ? 1 / W + (G/W)(G/W) sky_var_p   : spectra_var_p[x]
// The profile of a column is the window's own light over 2H + 1 columns: a scan's profile changes slowly along the
// dispersion, and the sum beats the noise of a single column down.  Two choices, both measured on an ensemble of
// CPU-oracle exposures.  V is the variance of the model (the smoothed expectation spectra_p Pr), not of the pixel's own
// v: a data variance gives a downward fluctuation more weight and biased the mean flux by -0.09 %.  P is clamped at 0 but
// NOT renormalised to sum 1 over the window (Horne's P / sum_y P): after the clamp that division turns the positive noise
// of the dark margin rows into flux, +0.16 % on the last read and +9.5 % on a nearly unlit interval, against +0.05 % and
// +0.16 % without it.  A column that is not ok (no source, or a window of noise) keeps the box values to the bit.
// Limits: the profile's own noise is not in 1 / W, so on a nearly unlit interval the variance is underestimated (an
// ensemble showed 1.64 times the prediction); the intervals' correlation through shared reads is as for spectra_var;
// with rn = 0 a pixel whose model is <= 0 has V = 0 and its column falls back to the box values.
// k_extract_optimal<T, CR>, behind k_extract_finish: the grid of k_extract_rows.  The workgroup forms d of its 32 rows x
// (64 + 2 kOptMaxH) columns into LDS (24 KB) -- a thread its own four centre pixels (rows wave, wave + 8, ... at column
// lane, so that their bt and rn^2 q^2 stay in registers) and two of the halo's; columns outside the frame and rows past
// the chunk's end hold 0 and take part in nothing.  After one barrier a lane forms S0 of its column and S1 of its
// rows as literal left-to-right sums of 2H + 1 LDS reads (no sliding window: the numpy law must round identically), then
// U, W and G over its rows; the waves are added in wave order -> scratch [U | W | G][chunk][product][S].  A pixel of a
// column that is not ok runs all the same (uniform barriers; its sums are ignored).  k_extract_optimal_finish (one
// workgroup per product) adds the chunks in ascending order, forms ok(x) from the same ascending sums S0 and SV0 and writes
// optimal and optimal_var behind the variances.  No atomics.
//
// Profile planes and a supplied profile (wayne_exposure_deliver_profile, wayne_exposure_set_optimal_profile; off unless
// asked for -- the kernels above are launched as before).  The profile S1 / S0 carries the exposure's own noise, and
// neighbouring columns share 2H of their 2H + 1 profile columns: summed over the columns of a wavelength channel that noise
// adds coherently (measured: 1.8 times the predicted variance of a 13-column sum).  A visit therefore forms ONE profile
// from several exposures and extracts every exposure with it.  Both arrays hold the windows of all R + 1 products one
// behind the other, rows relative to the window (ProfileArgs).  k_extract_profile<T, CR>, on the grid of k_extract_optimal
// and in front of it: d into LDS in the same way, then S1(y, x) of every window pixel -- the same left-to-right sum -- to the
// plane; S1 and not S1 / S0, so that planes of several exposures are added and the sum normalised (a flux-weighted mean, no
// division by a noisy S0).  k_extract_optimal_fixed<T, CR>, in place of k_extract_optimal: the law above with Pr := the
// supplied profile at the pixel -- no halo, no tile; a thread's rows, the waves and the chunks are added in the order of
// k_extract_optimal into the same scratch, and k_extract_optimal_finish follows as it is (H enters through ok(x) alone).
//
// Optimal channels (wayne_exposure_set_optimal_channels; off unless asked for): the law and the kernels stand with them at
// the end of this file.  k_extract_bins_opt<T, CR, FIXED> keeps three row buffers per wave (e / F, k / F, ev / F^2: 72 KB)
// and W_p, S0 of the hull's columns (6 KB): 79.9 KB with a supplied profile, two workgroups per CU.  With the exposure's own
// profile a wave also keeps d of its row with the halo (26 KB more: 106.5 KB, one workgroup per CU) and walks the row's
// planes twice -- the variant whose variance is not to be trusted anyway (README), kept simple rather than fast.
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
  // cosmic-ray rejection (null / 0 without it)
  uint16_t* mask;                    // [S*S]: bit j = flag_j; written on the mask rows [m_lo, m_hi) only
  unsigned* part_n;                  // [n_chunks][R+1][S]: flags of a chunk's column
  unsigned* n_rej;                   // [R+1]
  int m_lo, m_hi;
  double k2, rn2;                    // k^2, rn^2
  // variances (null / 0 without them)
  double vrn2;                       // rn^2 of the variance law
  double* part_v;                    // [n_chunks][R+1][S]: sums of var
  double* spectra_var;               // [(R+1)*S]
  double* sky_var;                   // [R+1]
};

// var_p of one pixel from the term v its flux sums and its gain factor g
__device__ __forceinline__ double extract_var(double v, double g, double rn2) {
  const double q = g / 2.35;
  return fmax(v, 0.) + rn2 * (q * q);
}

// L_r of one pixel (r >= 1); `lin`: the four coefficients are in c[]
template <class T>
__device__ __forceinline__ double extract_linear(const ExtractArgs& a, const T* reads, size_t SS, size_t pix, int r,
                                                 double p0, bool lin, const double* c) {
  const double D = (double)reads[(size_t)r * SS + pix] - p0;
  double L = lin ? D * (1.0 + c[0] + D * (c[1] + D * (c[2] + c[3] * D))) : D;
  if ((a.steps & X_DARK) && a.dark) L -= (double)a.dark[(size_t)(r - 1) * SS + pix];
  return L;
}

// I_{j+1} of one pixel, everything loaded here (the rare path of a flagged pixel and of its row neighbours)
template <class T>
__device__ double extract_interval(const ExtractArgs& a, const T* reads, size_t SS, size_t pix, int j, bool lin, bool gain) {
  const double p0 = (double)reads[pix];
  double c[4] = {0., 0., 0., 0.};
  if (lin)
    for (int i = 0; i < 4; ++i) c[i] = (double)a.lin[i][pix];
  const double Lh = extract_linear<T>(a, reads, SS, pix, j + 1, p0, lin, c);
  const double Ll = j > 0 ? extract_linear<T>(a, reads, SS, pix, j, p0, lin, c) : 0.;
  const double g = (a.steps & X_GAIN) ? (gain ? 2.35 / (double)a.pfl[pix] : 2.35) : 1.0;
  return (Lh - Ll) * g;
}

// half the sum of the middle two of four values
__device__ __forceinline__ double middle_two_mean(double a0, double a1, double a2, double a3) {
  const double lo1 = fmin(a0, a1), hi1 = fmax(a0, a1), lo2 = fmin(a2, a3), hi2 = fmax(a2, a3);
  return 0.5 * (fmax(lo1, lo2) + fmin(hi1, hi2));
}

// repl_j of a flagged pixel (it is tested, so x -+ 2 lie inside the frame)
template <class T>
__device__ double extract_repl(const ExtractArgs& a, const T* reads, size_t SS, size_t pix, int j, bool lin, bool gain) {
  return middle_two_mean(extract_interval<T>(a, reads, SS, pix - 2, j, lin, gain), extract_interval<T>(a, reads, SS, pix - 1, j, lin, gain),
                         extract_interval<T>(a, reads, SS, pix + 1, j, lin, gain), extract_interval<T>(a, reads, SS, pix + 2, j, lin, gain));
}

constexpr int kCrW = kCrTileCols + 2 * kCrHalo, kCrH = kCrTileRows + 2 * kCrHalo;   // the tile and its halo: 68 x 36
constexpr int kCrOwn = (kCrW * kCrH + kExtractThreads - 1) / kExtractThreads;        // pixels a thread carries: 5
static_assert(kCrTileCols == 64 && kCrTileRows % kExtractWaves == 0, "k_extract_crmask: a wave tests rows of 64 pixels");

template <class T>
__global__ void __launch_bounds__(kExtractThreads) k_extract_crmask(ExtractArgs a) {
  const int S = a.S, R = a.R, tid = (int)threadIdx.x;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int x0 = (int)blockIdx.x * kCrTileCols - kCrHalo;
  const int y_lo = a.m_lo + (int)blockIdx.y * kCrTileRows, y_hi = min(y_lo + kCrTileRows, a.m_hi);   // the rows stored
  const int y0 = y_lo - kCrHalo;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool dark = (a.steps & X_DARK) && a.dark;
  __shared__ double sh[2][kCrH * kCrW];
  // the thread's pixels of tile + halo: element tid + i * kExtractThreads, row-major
  size_t pix[kCrOwn];
  bool in[kCrOwn];
  double p0[kCrOwn], g[kCrOwn], Lp[kCrOwn];
  float cf[kCrOwn][4];               // (float32 planes: promoted at use, exactly)
#pragma unroll
  for (int i = 0; i < kCrOwn; ++i) {
    const int e = tid + i * kExtractThreads, ty = e / kCrW, tx = e - ty * kCrW;
    const int y = y0 + ty, x = x0 + tx;
    in[i] = e < kCrW * kCrH && y >= 0 && y < min(y_hi + kCrHalo, S) && x >= 0 && x < S;
    pix[i] = in[i] ? (size_t)y * S + x : 0;
    p0[i] = 0.; g[i] = 2.35; Lp[i] = 0.;
    for (int q = 0; q < 4; ++q) cf[i][q] = 0.f;
    if (in[i]) {
      p0[i] = (double)reads[pix[i]];
      if (lin)
        for (int q = 0; q < 4; ++q) cf[i][q] = a.lin[q][pix[i]];
      if (a.pfl) g[i] = 2.35 / (double)a.pfl[pix[i]];
    }
  }
  // the thread's tested pixels: rows wave, wave + 8, ... of the tile, column lane
  const int wave = tid >> 6, lane = tid & 63;
  const int x = x0 + kCrHalo + lane;
  const bool x_tested = x >= kCrMargin && x < S - kCrMargin;
  constexpr int kTest = kCrTileRows / kExtractWaves;
  unsigned bits[kTest];
#pragma unroll
  for (int i = 0; i < kTest; ++i) bits[i] = 0u;
  for (int r = 1; r <= R; ++r) {
    double* I = sh[r & 1];
#pragma unroll
    for (int i = 0; i < kCrOwn; ++i) {
      const int e = tid + i * kExtractThreads;
      if (e < kCrW * kCrH) {
        double v = 0.;
        if (in[i]) {
          const double D = (double)reads[(size_t)r * SS + pix[i]] - p0[i];
          double L = lin ? D * (1.0 + (double)cf[i][0] + D * ((double)cf[i][1] + D * ((double)cf[i][2] + (double)cf[i][3] * D))) : D;
          if (dark) L -= (double)a.dark[(size_t)(r - 1) * SS + pix[i]];
          v = (L - Lp[i]) * g[i];
          Lp[i] = L;
        }
        I[e] = v;
      }
    }
    __syncthreads();       // (one barrier per read: the next read fills the other buffer)
#pragma unroll
    for (int i = 0; i < kTest; ++i) {
      const int ty = kCrHalo + wave + i * kExtractWaves, y = y0 + ty;
      if (x_tested && y < y_hi && y >= kCrMargin && y < S - kCrMargin) {
        const double* at = I + ty * kCrW + kCrHalo + lane;
        double m8 = fmax(fmax(at[-kCrW], at[kCrW]), fmax(at[-2 * kCrW], at[2 * kCrW]));
        m8 = fmax(m8, fmax(fmax(at[-1], at[1]), fmax(at[-2], at[2])));
        const double d = at[0] - m8;
        if (d > 0. && d * d > a.k2 * (a.rn2 + fmax(m8, 0.))) bits[i] |= 1u << (r - 1);
      }
    }
  }
  if (x < S) {
#pragma unroll
    for (int i = 0; i < kTest; ++i) {
      const int y = y_lo + wave + i * kExtractWaves;
      if (y < y_hi) a.mask[(size_t)y * S + x] = (uint16_t)bits[i];
    }
  }
}

template <class T, bool CR, bool VAR>
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
  [[maybe_unused]] double sV = 0.;
  unsigned n_flag = 0u;
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
      if constexpr (CR) {
        double v = (Lh - Ll) * g;
        const unsigned m = a.mask[pix];
        if (p < a.R) {
          if ((m >> p) & 1u) { v = extract_repl<T>(a, reads, SS, pix, p, lin, gain); ++n_flag; }
        } else if (m) {
          double corr = 0.;
          for (unsigned b = m; b; b &= b - 1u) {               // the set bits, ascending
            const int j = __ffs((int)b) - 1;
            corr += extract_interval<T>(a, reads, SS, pix, j, lin, gain) - extract_repl<T>(a, reads, SS, pix, j, lin, gain);
            ++n_flag;
          }
          v -= corr;
        }
        sA += v;
        if constexpr (VAR) sV += extract_var(v, g, a.vrn2);
      } else if constexpr (VAR) {
        const double v = (Lh - Ll) * g;
        sA += v;
        sV += extract_var(v, g, a.vrn2);
      } else {
        sA += (Lh - Ll) * g;
      }
      if (sky) sT += (double)a.sky[pix];
    }
  }
  __shared__ double sh[2][kExtractWaves][64];
  sh[0][wave][lane] = sA;
  sh[1][wave][lane] = sT;
  __shared__ unsigned sh_n[CR ? kExtractWaves : 1][64];
  if constexpr (CR) sh_n[wave][lane] = n_flag;
  __shared__ double sh_v[VAR ? kExtractWaves : 1][64];
  if constexpr (VAR) sh_v[wave][lane] = sV;
  __syncthreads();
  if (wave == 0 && x < S) {
    double tA = sh[0][0][lane], tT = sh[1][0][lane];
    for (int w = 1; w < kExtractWaves; ++w) { tA += sh[0][w][lane]; tT += sh[1][w][lane]; }
    const int NP = a.R + 1;
    const size_t at = ((size_t)chunk * NP + p) * S + x;
    a.part[at] = tA;
    a.part[(size_t)a.n_chunks * NP * S + at] = tT;
    if constexpr (CR) {
      unsigned n = 0u;
      for (int w = 0; w < kExtractWaves; ++w) n += sh_n[w][lane];
      a.part_n[at] = n;
    }
    if constexpr (VAR) {
      double tV = sh_v[0][lane];
      for (int w = 1; w < kExtractWaves; ++w) tV += sh_v[w][lane];
      a.part_v[at] = tV;
    }
  }
}

template <bool CR, bool VAR>
__global__ void __launch_bounds__(kExtractThreads) k_extract_finish(ExtractArgs a) {
  const int p = (int)blockIdx.x, S = a.S, NP = a.R + 1;
  const int tid = (int)threadIdx.x;
  if (p == a.R && !(a.steps & X_LAST_READ)) {            // the last-read product was not asked for: zeros
    for (int x = tid; x < S; x += kExtractThreads) a.spectra[(size_t)p * S + x] = 0.;
    if (tid == 0) a.sky_out[p] = 0.;
    if (CR && tid == 0) a.n_rej[p] = 0u;
    if constexpr (VAR) {
      for (int x = tid; x < S; x += kExtractThreads) a.spectra_var[(size_t)p * S + x] = 0.;
      if (tid == 0) a.sky_var[p] = 0.;
    }
    return;
  }
  __shared__ double shA[kExtractMaxS], shB[kExtractMaxS];
  __shared__ double shR[2][64];
  __shared__ double sh_sky;
  __shared__ double shV[VAR ? kExtractMaxS : 1], shRV[VAR ? 64 : 1];
  __shared__ double sh_skyvar;
  const int rows = a.row_hi[p] - a.row_lo[p];
  const int chunks = (rows + kExtractRows - 1) / kExtractRows;
  const size_t half = (size_t)a.n_chunks * NP * S;
  unsigned n_flag = 0u;
  for (int x = tid; x < S; x += kExtractThreads) {
    double A = 0., T = 0.;
    [[maybe_unused]] double V = 0.;
    for (int c = 0; c < chunks; ++c) {                   // ascending chunks
      const size_t at = ((size_t)c * NP + p) * S + x;
      A += a.part[at];
      T += a.part[half + at];
      if constexpr (CR) n_flag += a.part_n[at];
      if constexpr (VAR) V += a.part_v[at];
    }
    shA[x] = A;
    shB[x] = a.scale[p] * T;
    if constexpr (VAR) shV[x] = V;
  }
  __shared__ unsigned shN[CR ? kExtractThreads : 1];
  if constexpr (CR) shN[tid] = n_flag;
  __syncthreads();
  if (tid < 64) {
    double sa = 0., sb = 0.;
    for (int x = a.bg_lo + tid; x < a.bg_hi; x += 64) { sa += shA[x]; sb += shB[x]; }
    shR[0][tid] = sa;
    shR[1][tid] = sb;
    if constexpr (VAR) {
      double sv = 0.;
      for (int x = a.bg_lo + tid; x < a.bg_hi; x += 64) sv += shV[x];
      shRV[tid] = sv;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double sa = 0., sb = 0.;
    for (int l = 0; l < 64; ++l) { sa += shR[0][l]; sb += shR[1][l]; }
    sh_sky = ((a.steps & X_SKY) && sb != 0.) ? sa / sb : 0.;
    a.sky_out[p] = sh_sky;
    if constexpr (VAR) {
      double sv = 0.;
      for (int l = 0; l < 64; ++l) sv += shRV[l];
      sh_skyvar = ((a.steps & X_SKY) && sb != 0.) ? sv / (sb * sb) : 0.;
      a.sky_var[p] = sh_skyvar;
    }
    if constexpr (CR) {
      unsigned n = 0u;
      for (int t = 0; t < kExtractThreads; ++t) n += shN[t];
      a.n_rej[p] = n;
    }
  }
  __syncthreads();
  const double s = sh_sky;
  for (int x = tid; x < S; x += kExtractThreads) a.spectra[(size_t)p * S + x] = shA[x] - s * shB[x];
  if constexpr (VAR) {
    const double sv = sh_skyvar;
    for (int x = tid; x < S; x += kExtractThreads) a.spectra_var[(size_t)p * S + x] = shV[x] + (shB[x] * shB[x]) * sv;
  }
}

// ---- wavelength-binned channels (wayne_exposure_set_channels) ----

struct ChannelArgs {
  int C;                             // channels, 1 .. kChanMaxChannels
  int u_lo, u_hi;                    // the column hull (plan::channels_desc_error): u_hi - u_lo <= kChanMaxHull
  bool flat;                         // WAYNE_C_FLAT is set and the context holds a flat cube
  int N;                             // side of the flat planes: S - 2 kBorder
  double flat_wmin, flat_wmax;
  const double* edges;               // [C + 1] um
  const double* wl_a;                // [S]
  const double* wl_b;                // [S]
  const float* cube[4];              // [N*N] each, or null
  double* part;                      // [n_chunks][kChanGroups][R+1][2][C]: a row group's P, then its Q / scale
  double* channels;                  // [(R+1)*C]
  // variances (null without them)
  double* part_v;                    // [n_chunks][kChanGroups][R+1][C]: a row group's VP
  double* channels_var;              // [(R+1)*C]
};

// the term k_extract_rows adds to A_p[x] for pixel `pix` = y S + x (the same operations in the same order)
template <class T, bool CR>
__device__ __forceinline__ double extract_term(const ExtractArgs& a, const T* reads, size_t SS, size_t pix, int p, int r_hi,
                                               int r_lo, bool lin, bool gain, double* g_out = nullptr) {
  const double p0 = (double)reads[pix];
  double c[4] = {0., 0., 0., 0.};
  if (lin)
    for (int i = 0; i < 4; ++i) c[i] = (double)a.lin[i][pix];
  const double Lh = extract_linear<T>(a, reads, SS, pix, r_hi, p0, lin, c);
  const double Ll = r_lo > 0 ? extract_linear<T>(a, reads, SS, pix, r_lo, p0, lin, c) : 0.;
  const double g = (a.steps & X_GAIN) ? (gain ? 2.35 / (double)a.pfl[pix] : 2.35) : 1.0;
  if (g_out) *g_out = g;
  double v = (Lh - Ll) * g;
  if constexpr (CR) {
    const unsigned m = a.mask[pix];
    if (p < a.R) {
      if ((m >> p) & 1u) v = extract_repl<T>(a, reads, SS, pix, p, lin, gain);
    } else if (m) {
      double corr = 0.;
      for (unsigned b = m; b; b &= b - 1u) {                 // the set bits, ascending
        const int j = __ffs((int)b) - 1;
        corr += extract_interval<T>(a, reads, SS, pix, j, lin, gain) - extract_repl<T>(a, reads, SS, pix, j, lin, gain);
      }
      v -= corr;
    }
  }
  return v;
}

// F(y, x) of the channels' law (`y_in`: the row is no border row)
__device__ __forceinline__ double chan_flat(const ChannelArgs& ch, int y, int x, double wa, double wb, bool y_in, int S) {
  double F = 1.;
  if (ch.flat && y_in && x >= kBorder && x < S - kBorder) {
    const double tau = (1e4 * (wa + wb * (double)x) - ch.flat_wmin) / (ch.flat_wmax - ch.flat_wmin);
    const double t2 = tau * tau, t3 = t2 * tau;
    const size_t fi = (size_t)(y - kBorder) * ch.N + (x - kBorder);
    const double f = (double)ch.cube[0][fi] + ((double)ch.cube[1][fi] * tau) + ((double)ch.cube[2][fi] * t2) +
                     ((double)ch.cube[3][fi] * t3);
    F = (double)(float)f;
    if (!(F > 0.)) F = 1.;
  }
  return F;
}

constexpr int kChanPasses = (kChanMaxChannels + 63) / 64;             // channels a lane carries: 4
constexpr int kChanGroups = kExtractRows / kExtractWaves;            // groups of 8 rows (one per wave) in a chunk: 4
static_assert(kExtractRows % kExtractWaves == 0, "k_extract_bins: a chunk is a whole number of row groups");
// the waves' sums red[kExtractWaves][2][C] reuse the row buffers buf[kExtractWaves][2][kChanMaxHull]
static_assert(kExtractWaves * 2 * kChanMaxChannels <= kExtractWaves * 2 * kChanMaxHull,
              "k_extract_bins: the waves' sums of the widest channel plan must fit the row buffers they reuse");
constexpr int kChanStrips = kChanMaxHull / 64;                       // 64-column strips of the widest hull: 6
static_assert(kChanMaxHull % 64 == 0, "k_extract_bins: a lane keeps one value per 64-column strip of the hull");
// with variances the waves' sums are red[kExtractWaves][2][C], then redv[kExtractWaves][C]
static_assert(kExtractWaves * 3 * kChanMaxChannels <= kExtractWaves * 2 * kChanMaxHull,
              "k_extract_bins: the waves' sums with variances must fit the row buffers they reuse");

// One workgroup per (chunk of a product's window -- the chunk list of k_extract_rows -- , group blockIdx.y of 8 rows of
// it).  Wave w takes row w of the group: it writes v / F and t / F of the hull's columns into its row buffers, 64 columns
// at a time, then lane = channel (kChanPasses passes) gathers [ua_b, ua_{b+1}) from them in ascending x.  A row past
// the window's end adds nothing (its group still writes its zeros), so the barriers are uniform.  VAR: a lane keeps
// var / F^2 of its columns (one per strip) in registers meanwhile; the wave then writes them over its v / F buffer and the
// channels gather them with w^2.
template <class T, bool CR, bool VAR>
__global__ void __launch_bounds__(kExtractThreads) k_extract_bins(ExtractArgs a, ChannelArgs ch) {
  int p = 0;
  while (p < a.R && (int)blockIdx.x >= a.first_chunk[p + 1]) ++p;
  const int chunk = (int)blockIdx.x - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int S = a.S, C = ch.C, W = ch.u_hi - ch.u_lo;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  __shared__ double buf[kExtractWaves][2][kChanMaxHull];
  double* bv = buf[wave][0];
  double* bt = buf[wave][1];
  double P[kChanPasses], Q[kChanPasses], e0[kChanPasses], e1[kChanPasses];
#pragma unroll
  for (int k = 0; k < kChanPasses; ++k) {
    const int b = k * 64 + lane;
    P[k] = 0.; Q[k] = 0.;
    if constexpr (!VAR) {
      e0[k] = b < C ? ch.edges[b] : 0.;
      e1[k] = b < C ? ch.edges[b + 1] : 0.;
    }
  }
  const int group = (int)blockIdx.y;
  const int y = lo + wave + group * kExtractWaves;
  const bool row = y < hi;                                 // (wave-uniform)
  double wa = 0., wb = 1.;
  [[maybe_unused]] double vr[VAR ? kChanStrips : 1];           // var / F^2 of column lane + 64 s of the hull
  if (row) {
    wa = ch.wl_a[y]; wb = ch.wl_b[y];
    const bool y_in = y >= kBorder && y < S - kBorder;
    if constexpr (VAR) {
#pragma unroll
      for (int s = 0; s < kChanStrips; ++s) {
        const int o = lane + 64 * s;
        vr[s] = 0.;
        if (o < W) {
          const int x = ch.u_lo + o;
          const size_t pix = (size_t)y * S + x;
          double g;
          const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain, &g);
          const double t = sky ? (double)a.sky[pix] : 0.;
          const double F = chan_flat(ch, y, x, wa, wb, y_in, S);
          bv[o] = v / F;
          bt[o] = t / F;
          vr[s] = extract_var(v, g, a.vrn2) / (F * F);
        }
      }
    } else {
      for (int o = lane; o < W; o += 64) {
        const int x = ch.u_lo + o;
        const size_t pix = (size_t)y * S + x;
        const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain);
        const double t = sky ? (double)a.sky[pix] : 0.;
        const double F = chan_flat(ch, y, x, wa, wb, y_in, S);
        bv[o] = v / F;
        bt[o] = t / F;
      }
    }
  }
  if constexpr (VAR) {                                       // (the edges only now: the row's chain needs the registers)
#pragma unroll
    for (int k = 0; k < kChanPasses; ++k) {
      const int b = k * 64 + lane;
      e0[k] = b < C ? ch.edges[b] : 0.;
      e1[k] = b < C ? ch.edges[b + 1] : 0.;
    }
  }
  __syncthreads();
  if (row) {
#pragma unroll
    for (int k = 0; k < kChanPasses; ++k) {
      if (k * 64 + lane < C) {
        const double ua0 = (e0[k] - wa) / wb, ua1 = (e1[k] - wa) / wb;
        // the columns [floor(ua0), ceil(ua1)) of the hull (clamped as float64: an edge may lie far outside the frame)
        const int xs = (int)fmin(fmax(floor(ua0), (double)ch.u_lo), (double)ch.u_hi);
        const int xe = (int)fmin(fmax(ceil(ua1), (double)ch.u_lo), (double)ch.u_hi);
        for (int x = xs; x < xe; ++x) {
          const double w = fmin(fmax(fmin((double)x + 1.0, ua1) - fmax((double)x, ua0), 0.), 1.);
          P[k] += w * bv[x - ch.u_lo];
          Q[k] += w * bt[x - ch.u_lo];
        }
      }
    }
  }
  [[maybe_unused]] double V[VAR ? kChanPasses : 1];
  if constexpr (VAR) {
    __syncthreads();                                         // v / F has been gathered: the buffer takes var / F^2
    if (row) {
#pragma unroll
      for (int s = 0; s < kChanStrips; ++s) {
        const int o = lane + 64 * s;
        if (o < W) bv[o] = vr[s];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kChanPasses; ++k) {
      V[k] = 0.;
      if (row && k * 64 + lane < C) {
        const double ua0 = (e0[k] - wa) / wb, ua1 = (e1[k] - wa) / wb;
        const int xs = (int)fmin(fmax(floor(ua0), (double)ch.u_lo), (double)ch.u_hi);
        const int xe = (int)fmin(fmax(ceil(ua1), (double)ch.u_lo), (double)ch.u_hi);
        for (int x = xs; x < xe; ++x) {
          const double w = fmin(fmax(fmin((double)x + 1.0, ua1) - fmax((double)x, ua0), 0.), 1.);
          V[k] += (w * w) * bv[x - ch.u_lo];
        }
      }
    }
  }
  __syncthreads();
  // the waves' sums, added in wave order: the row buffers are free now (the barrier above)
  double* red = &buf[0][0][0];                               // [kExtractWaves][2][C]
  [[maybe_unused]] double* redv = red + (size_t)kExtractWaves * 2 * C;   // [kExtractWaves][C] (VAR)
#pragma unroll
  for (int k = 0; k < kChanPasses; ++k) {
    const int b = k * 64 + lane;
    if (b < C) {
      red[((size_t)wave * 2 + 0) * C + b] = P[k];
      red[((size_t)wave * 2 + 1) * C + b] = Q[k];
      if constexpr (VAR) redv[(size_t)wave * C + b] = V[k];
    }
  }
  __syncthreads();
  const int NP = a.R + 1;
  for (int i = (int)threadIdx.x; i < 2 * C; i += kExtractThreads) {
    double t = red[i];
    for (int w = 1; w < kExtractWaves; ++w) t += red[(size_t)w * 2 * C + i];
    ch.part[(((size_t)chunk * kChanGroups + group) * NP + p) * 2 * C + i] = t;
  }
  if constexpr (VAR) {
    for (int i = (int)threadIdx.x; i < C; i += kExtractThreads) {
      double t = redv[i];
      for (int w = 1; w < kExtractWaves; ++w) t += redv[(size_t)w * C + i];
      ch.part_v[(((size_t)chunk * kChanGroups + group) * NP + p) * C + i] = t;
    }
  }
}

// Behind k_extract_finish (it reads sky_p): one workgroup per product adds the row groups in ascending order and writes
// channels_p[b] = P_p[b] - sky_p (scale_p Q_p[b]); VAR: and channels_var_p[b] = VP_p[b] + (scale_p Q_p[b])^2 sky_var_p.
template <bool VAR>
__global__ void __launch_bounds__(kChanMaxChannels) k_extract_bins_finish(ExtractArgs a, ChannelArgs ch) {
  const int p = (int)blockIdx.x, b = (int)threadIdx.x, C = ch.C, NP = a.R + 1;
  if (b >= C) return;
  if (p == a.R && !(a.steps & X_LAST_READ)) {
    ch.channels[(size_t)p * C + b] = 0.;
    if constexpr (VAR) ch.channels_var[(size_t)p * C + b] = 0.;
    return;
  }
  const int rows = a.row_hi[p] - a.row_lo[p];
  const int chunks = (rows + kExtractRows - 1) / kExtractRows;
  double P = 0., Q = 0.;
  for (int c = 0; c < chunks * kChanGroups; ++c) {           // ascending chunks, ascending groups of a chunk
    const size_t at = ((size_t)c * NP + p) * 2 * C;
    P += ch.part[at + b];
    Q += ch.part[at + C + b];
  }
  ch.channels[(size_t)p * C + b] = P - a.sky_out[p] * (a.scale[p] * Q);
  if constexpr (VAR) {
    double V = 0.;
    for (int c = 0; c < chunks * kChanGroups; ++c) V += ch.part_v[((size_t)c * NP + p) * C + b];
    const double Qs = a.scale[p] * Q;
    ch.channels_var[(size_t)p * C + b] = V + (Qs * Qs) * a.sky_var[p];
  }
}

// ---- optimal extraction (wayne_exposure_set_optimal) ----

struct OptimalArgs {
  int H;                             // the profile's half width in columns, 1 .. kOptMaxH
  double* part;                      // [3][n_chunks][R+1][S]: a chunk's U, then W, then G
  double* optimal;                   // [(R+1)*S]
  double* optimal_var;               // [(R+1)*S]
};

constexpr int kOptW = 64 + 2 * kOptMaxH;                                  // columns of a tile and its halo: 96
constexpr int kOptOwn = kExtractRows / kExtractWaves;                     // centre pixels of a thread: 4
constexpr int kOptHalo = kExtractRows * 2 * kOptMaxH / kExtractThreads;   // halo pixels of a thread: 2
static_assert(kExtractRows % kExtractWaves == 0 && kExtractRows * 2 * kOptMaxH % kExtractThreads == 0,
              "k_extract_optimal: the tile and its halo are a whole number of entries per thread");
static_assert(kOptW <= kExtractThreads, "k_extract_optimal: one thread per staged value of spectra_p");

// One workgroup per (64-column tile, chunk of the list of k_extract_rows); LDS column c holds frame column xt + c.
template <class T, bool CR>
__global__ void __launch_bounds__(kExtractThreads) k_extract_optimal(ExtractArgs a, OptimalArgs o) {
  int p = 0;
  while (p < a.R && (int)blockIdx.y >= a.first_chunk[p + 1]) ++p;     // (wave-uniform: at most R steps)
  const int chunk = (int)blockIdx.y - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S, xt = (int)blockIdx.x * 64 - kOptMaxH;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  const double sky_p = a.sky_out[p], scale = a.scale[p];
  __shared__ double sd[kExtractRows][kOptW];                 // d of the chunk's rows
  __shared__ double ss[kOptW];                               // spectra_p of the tile's columns
  const int x = xt + kOptMaxH + lane;                        // the thread's own column
  double bt[kOptOwn], rq[kOptOwn];                           // bt and rn^2 (q q) of its centre pixels
#pragma unroll
  for (int i = 0; i < kOptOwn; ++i) {
    const int ty = wave + i * kExtractWaves, y = lo + ty;
    double d = 0.;
    bt[i] = 0.; rq[i] = 0.;
    if (y < hi && x < S) {
      const size_t pix = (size_t)y * S + x;
      double g;
      const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain, &g);
      const double t = sky ? (double)a.sky[pix] : 0.;
      const double q = g / 2.35;
      bt[i] = scale * t;
      rq[i] = a.vrn2 * (q * q);
      d = v - sky_p * bt[i];
    }
    sd[ty][kOptMaxH + lane] = d;
  }
#pragma unroll
  for (int k = 0; k < kOptHalo; ++k) {
    const int e = tid + k * kExtractThreads, ty = e / (2 * kOptMaxH), hc = e - ty * (2 * kOptMaxH);
    const int c = hc < kOptMaxH ? hc : 64 + hc, y = lo + ty, xh = xt + c;
    double d = 0.;
    if (y < hi && xh >= 0 && xh < S) {
      const size_t pix = (size_t)y * S + xh;
      const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain);
      const double t = sky ? (double)a.sky[pix] : 0.;
      d = v - sky_p * (scale * t);
    }
    sd[ty][c] = d;
  }
  if (tid < kOptW) {
    const int xs = xt + tid;
    ss[tid] = (xs >= 0 && xs < S) ? a.spectra[(size_t)p * S + xs] : 0.;
  }
  __syncthreads();
  double sU = 0., sW = 0., sG = 0.;
  if (x < S) {
    const int c0 = max(x - o.H, 0) - xt, c1 = min(x + o.H, S - 1) - xt;      // X(x), as LDS columns
    double S0 = 0.;
    for (int c = c0; c <= c1; ++c) S0 += ss[c];
    const double sp = ss[kOptMaxH + lane];
#pragma unroll
    for (int i = 0; i < kOptOwn; ++i) {
      const int ty = wave + i * kExtractWaves;
      if (lo + ty < hi) {
        const double* row = sd[ty];
        double S1 = 0.;
        for (int c = c0; c <= c1; ++c) S1 += row[c];
        const double d = row[kOptMaxH + lane];
        const double Pr = S1 / S0, P = fmax(Pr, 0.);
        const double V = fmax(sp * Pr + sky_p * bt[i], 0.) + rq[i];
        sU += (P * d) / V;
        sW += (P * P) / V;
        sG += (P * bt[i]) / V;
      }
    }
  }
  __shared__ double sh[3][kExtractWaves][64];
  sh[0][wave][lane] = sU;
  sh[1][wave][lane] = sW;
  sh[2][wave][lane] = sG;
  __syncthreads();
  if (wave == 0 && x < S) {
    const int NP = a.R + 1;
    const size_t at = ((size_t)chunk * NP + p) * S + x, third = (size_t)a.n_chunks * NP * S;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t = sh[k][0][lane];
      for (int w = 1; w < kExtractWaves; ++w) t += sh[k][w][lane];
      o.part[k * third + at] = t;
    }
  }
}

// Behind k_extract_optimal: one workgroup per product adds the chunks in ascending order and chooses, column by column,
// between the optimal values and the box values that are already there.
__global__ void __launch_bounds__(kExtractThreads) k_extract_optimal_finish(ExtractArgs a, OptimalArgs o) {
  const int p = (int)blockIdx.x, S = a.S, NP = a.R + 1, tid = (int)threadIdx.x;
  double* out = o.optimal + (size_t)p * S;
  double* out_var = o.optimal_var + (size_t)p * S;
  if (p == a.R && !(a.steps & X_LAST_READ)) {            // the last-read product was not asked for: zeros
    for (int x = tid; x < S; x += kExtractThreads) { out[x] = 0.; out_var[x] = 0.; }
    return;
  }
  __shared__ double shS[kExtractMaxS], shV[kExtractMaxS];
  for (int x = tid; x < S; x += kExtractThreads) {
    shS[x] = a.spectra[(size_t)p * S + x];
    shV[x] = a.spectra_var[(size_t)p * S + x];
  }
  __syncthreads();
  const int rows = a.row_hi[p] - a.row_lo[p];
  const int chunks = (rows + kExtractRows - 1) / kExtractRows;
  const size_t third = (size_t)a.n_chunks * NP * S;
  const double sky_var = a.sky_var[p];
  for (int x = tid; x < S; x += kExtractThreads) {
    const int x0 = max(x - o.H, 0), x1 = min(x + o.H, S - 1);
    double S0 = 0., SV0 = 0.;
    for (int c = x0; c <= x1; ++c) { S0 += shS[c]; SV0 += shV[c]; }
    double U = 0., W = 0., G = 0.;
    for (int c = 0; c < chunks; ++c) {                   // ascending chunks
      const size_t at = ((size_t)c * NP + p) * S + x;
      U += o.part[at];
      W += o.part[third + at];
      G += o.part[2 * third + at];
    }
    const bool ok = S0 > 0. && S0 * S0 > 9. * SV0 && W > 0.;
    const double GW = G / W;
    out[x] = ok ? U / W : shS[x];
    out_var[x] = ok ? 1. / W + (GW * GW) * sky_var : shV[x];
  }
}

// ---- profile planes and the supplied profile (wayne_exposure_deliver_profile, wayne_exposure_set_optimal_profile) ----

// Both lay a product's window out as [rows_p][S] float64, window-relative rows, the windows one behind the other:
// element row_off[p] + (y - row_lo[p]) S + x, row_off[p] = sum_{p' < p} rows_{p'} S over ALL R + 1 windows.
struct ProfileArgs {
  size_t row_off[kExtractProducts];
  double* planes;                    // k_extract_profile writes S1 here (null without delivery)
  const double* fixed;               // k_extract_optimal_fixed reads its profile here (null without one)
};

constexpr int kProfOwn = kExtractRows * kOptW / kExtractThreads;          // staged values of a thread: 6
static_assert(kExtractRows * kOptW % kExtractThreads == 0, "k_extract_profile: the tile and its halo are a whole number of entries per thread");

// One workgroup per (64-column tile, chunk of the list of k_extract_rows): d of the chunk's rows x (64 + 2 kOptMaxH)
// columns into LDS as k_extract_optimal forms it (0 outside the frame), then S1 of the thread's pixels -- the same
// literal left-to-right sums -- to the plane.  Every pixel of a formed window is written; nothing else is.
template <class T, bool CR>
__global__ void __launch_bounds__(kExtractThreads) k_extract_profile(ExtractArgs a, OptimalArgs o, ProfileArgs f) {
  int p = 0;
  while (p < a.R && (int)blockIdx.y >= a.first_chunk[p + 1]) ++p;     // (wave-uniform: at most R steps)
  const int chunk = (int)blockIdx.y - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S, xt = (int)blockIdx.x * 64 - kOptMaxH;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  const double sky_p = a.sky_out[p], scale = a.scale[p];
  __shared__ double sd[kExtractRows][kOptW];
#pragma unroll
  for (int k = 0; k < kProfOwn; ++k) {
    const int e = tid + k * kExtractThreads, ty = e / kOptW, c = e - ty * kOptW;
    const int y = lo + ty, xs = xt + c;
    double d = 0.;
    if (y < hi && xs >= 0 && xs < S) {
      const size_t pix = (size_t)y * S + xs;
      const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain);
      const double t = sky ? (double)a.sky[pix] : 0.;
      d = v - sky_p * (scale * t);
    }
    sd[ty][c] = d;
  }
  __syncthreads();
  const int x = xt + kOptMaxH + lane;
  if (x < S) {
    const int c0 = max(x - o.H, 0) - xt, c1 = min(x + o.H, S - 1) - xt;      // X(x), as LDS columns
    for (int ty = wave; lo + ty < hi; ty += kExtractWaves) {
      const double* row = sd[ty];
      double S1 = 0.;
      for (int c = c0; c <= c1; ++c) S1 += row[c];
      f.planes[f.row_off[p] + (size_t)(lo + ty - a.row_lo[p]) * S + x] = S1;
    }
  }
}

// The law of k_extract_optimal with Pr := the supplied profile at the pixel: no halo and no LDS tile.  The grid and the
// order of the row sums are k_extract_optimal's (a thread its rows wave, wave + 8, ... of the chunk, the waves in wave
// order -> the same scratch), so k_extract_optimal_finish follows as it is; H enters there alone, through ok(x).
template <class T, bool CR>
__global__ void __launch_bounds__(kExtractThreads) k_extract_optimal_fixed(ExtractArgs a, OptimalArgs o, ProfileArgs f) {
  int p = 0;
  while (p < a.R && (int)blockIdx.y >= a.first_chunk[p + 1]) ++p;     // (wave-uniform: at most R steps)
  const int chunk = (int)blockIdx.y - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int S = a.S, x = (int)blockIdx.x * 64 + lane;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  const double sky_p = a.sky_out[p], scale = a.scale[p];
  double sU = 0., sW = 0., sG = 0.;
  if (x < S) {
    const double sp = a.spectra[(size_t)p * S + x];
    const double* prof = f.fixed + f.row_off[p] + x;
    for (int y = lo + wave; y < hi; y += kExtractWaves) {
      const size_t pix = (size_t)y * S + x;
      const double Pr = prof[(size_t)(y - a.row_lo[p]) * S];
      double g;
      const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain, &g);
      const double t = sky ? (double)a.sky[pix] : 0.;
      const double q = g / 2.35;
      const double bt = scale * t;
      const double d = v - sky_p * bt;
      const double P = fmax(Pr, 0.);
      const double V = fmax(sp * Pr + sky_p * bt, 0.) + a.vrn2 * (q * q);
      sU += (P * d) / V;
      sW += (P * P) / V;
      sG += (P * bt) / V;
    }
  }
  __shared__ double sh[3][kExtractWaves][64];
  sh[0][wave][lane] = sU;
  sh[1][wave][lane] = sW;
  sh[2][wave][lane] = sG;
  __syncthreads();
  if (wave == 0 && x < S) {
    const int NP = a.R + 1;
    const size_t at = ((size_t)chunk * NP + p) * S + x, third = (size_t)a.n_chunks * NP * S;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t = sh[k][0][lane];
      for (int w = 1; w < kExtractWaves; ++w) t += sh[k][w][lane];
      o.part[k * third + at] = t;
    }
  }
}

// ---- optimal channels (wayne_exposure_set_optimal_channels) ----

struct OptChanArgs {
  double* part;                      // [n_chunks][kChanGroups][R+1][3][C]: a row group's E, K and EV
  double* channels_opt;              // [(R+1)*C]
  double* channels_opt_var;          // [(R+1)*C]
};

constexpr int kOptChanW = kChanMaxHull + 2 * kOptMaxH;               // a row of d with its halo: 416 columns
static_assert(kExtractWaves * 3 * kChanMaxChannels <= kExtractWaves * 3 * kChanMaxHull,
              "k_extract_bins_opt: the waves' sums of the widest channel plan must fit the row buffers they reuse");
static_assert(kChanMaxHull <= kExtractThreads, "k_extract_bins_opt: one thread per column of the hull forms W_p and ok");

// Behind k_extract_optimal_finish, shaped like k_extract_bins: one workgroup per (chunk of the list of k_extract_rows,
// group of 8 rows of it), wave w takes row w of the group, lane = channel gathers in ascending x, the waves are added in
// wave order.  First a thread per hull column forms W_p[x] from the optimal scratch -- the ascending chunk sum of
// k_extract_optimal_finish -- and ok(x) by its rule (shW holds W where ok, else 0; shS0 the sum S0).  FIXED: Pr is the
// supplied profile at the pixel.  Otherwise the wave first writes d of its row over the hull and kOptMaxH columns on either
// side into LDS (0 outside the frame) and Pr = S1 / S0 is the literal left-to-right sum k_extract_optimal takes.  Then
//   e = ok ? ((P d) / V) / W : d,   k = ok ? ((P bt) / V) / W : bt,   ev = ok ? ((P P) / V) / (W W) : max(v, 0) + rn^2 q^2
// go to the wave's three row buffers as e / F, k / F and ev / (F F), and channel b adds w_b, w_b and w_b^2 times them.
template <class T, bool CR, bool FIXED>
__global__ void __launch_bounds__(kExtractThreads) k_extract_bins_opt(ExtractArgs a, ChannelArgs ch, OptimalArgs o, ProfileArgs f,
                                                                      OptChanArgs oc) {
  int p = 0;
  while (p < a.R && (int)blockIdx.x >= a.first_chunk[p + 1]) ++p;
  const int chunk = (int)blockIdx.x - a.first_chunk[p];
  const int lo = a.row_lo[p] + chunk * kExtractRows, hi = min(lo + kExtractRows, a.row_hi[p]);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = a.S, C = ch.C, W = ch.u_hi - ch.u_lo, NP = a.R + 1;
  const size_t SS = (size_t)S * S;
  const T* reads = (const T*)a.reads;
  const int r_hi = p < a.R ? p + 1 : a.R, r_lo = p < a.R ? p : 0;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool gain = (a.steps & X_GAIN) && a.pfl, sky = (a.steps & X_SKY) && a.sky;
  const double sky_p = a.sky_out[p], scale = a.scale[p];
  __shared__ double buf[kExtractWaves][3][kChanMaxHull];
  __shared__ double shW[kChanMaxHull], shS0[kChanMaxHull];
  __shared__ double bd[FIXED ? 1 : kExtractWaves][FIXED ? 1 : kOptChanW];
  if (tid < W) {
    const int x = ch.u_lo + tid;
    const int x0 = max(x - o.H, 0), x1 = min(x + o.H, S - 1);
    double S0 = 0., SV0 = 0.;
    for (int c = x0; c <= x1; ++c) { S0 += a.spectra[(size_t)p * S + c]; SV0 += a.spectra_var[(size_t)p * S + c]; }
    const int rows = a.row_hi[p] - a.row_lo[p];
    const int chunks = (rows + kExtractRows - 1) / kExtractRows;
    const size_t third = (size_t)a.n_chunks * NP * S;
    double Ws = 0.;
    for (int c = 0; c < chunks; ++c) Ws += o.part[third + ((size_t)c * NP + p) * S + x];      // ascending chunks
    const bool ok = S0 > 0. && S0 * S0 > 9. * SV0 && Ws > 0.;
    shW[tid] = ok ? Ws : 0.;
    shS0[tid] = S0;
  }
  const int group = (int)blockIdx.y;
  const int y = lo + wave + group * kExtractWaves;
  const bool row = y < hi;                                   // (wave-uniform)
  const int xd = ch.u_lo - kOptMaxH;                         // frame column of bd's column 0
  if constexpr (!FIXED) {
    if (row) {
      for (int c = lane; c < W + 2 * kOptMaxH; c += 64) {
        const int xs = xd + c;
        double d = 0.;
        if (xs >= 0 && xs < S) {
          const size_t pix = (size_t)y * S + xs;
          const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain);
          const double t = sky ? (double)a.sky[pix] : 0.;
          d = v - sky_p * (scale * t);
        }
        bd[wave][c] = d;
      }
    }
  }
  __syncthreads();
  double* be = buf[wave][0];
  double* bk = buf[wave][1];
  double* bv = buf[wave][2];
  double wa = 0., wb = 1.;
  if (row) {
    wa = ch.wl_a[y]; wb = ch.wl_b[y];
    const bool y_in = y >= kBorder && y < S - kBorder;
    for (int oo = lane; oo < W; oo += 64) {
      const int x = ch.u_lo + oo;
      const size_t pix = (size_t)y * S + x;
      double g;
      const double v = extract_term<T, CR>(a, reads, SS, pix, p, r_hi, r_lo, lin, gain, &g);
      const double t = sky ? (double)a.sky[pix] : 0.;
      const double F = chan_flat(ch, y, x, wa, wb, y_in, S);
      const double q = g / 2.35;
      const double bt = scale * t, rq = a.vrn2 * (q * q);
      const double d = v - sky_p * bt;
      const double Wx = shW[oo];
      double e = d, k = bt, ev = fmax(v, 0.) + rq;
      if (Wx > 0.) {                                         // ok(x)
        double Pr;
        if constexpr (FIXED) {
          Pr = f.fixed[f.row_off[p] + (size_t)(y - a.row_lo[p]) * S + x];
        } else {
          const int c0 = max(x - o.H, 0) - xd, c1 = min(x + o.H, S - 1) - xd;      // X(x), as columns of bd
          double S1 = 0.;
          for (int c = c0; c <= c1; ++c) S1 += bd[wave][c];
          Pr = S1 / shS0[oo];
        }
        const double P = fmax(Pr, 0.);
        const double V = fmax(a.spectra[(size_t)p * S + x] * Pr + sky_p * bt, 0.) + rq;
        e = ((P * d) / V) / Wx;
        k = ((P * bt) / V) / Wx;
        ev = ((P * P) / V) / (Wx * Wx);
      }
      be[oo] = e / F;
      bk[oo] = k / F;
      bv[oo] = ev / (F * F);
    }
  }
  double e0[kChanPasses], e1[kChanPasses];
#pragma unroll
  for (int kk = 0; kk < kChanPasses; ++kk) {                 // (the edges only now: the row's chain needs the registers)
    const int b = kk * 64 + lane;
    e0[kk] = b < C ? ch.edges[b] : 0.;
    e1[kk] = b < C ? ch.edges[b + 1] : 0.;
  }
  __syncthreads();
  double E[kChanPasses], K[kChanPasses], EV[kChanPasses];
#pragma unroll
  for (int kk = 0; kk < kChanPasses; ++kk) {
    E[kk] = 0.; K[kk] = 0.; EV[kk] = 0.;
    if (row && kk * 64 + lane < C) {
      const double ua0 = (e0[kk] - wa) / wb, ua1 = (e1[kk] - wa) / wb;
      const int xs = (int)fmin(fmax(floor(ua0), (double)ch.u_lo), (double)ch.u_hi);
      const int xe = (int)fmin(fmax(ceil(ua1), (double)ch.u_lo), (double)ch.u_hi);
      for (int x = xs; x < xe; ++x) {
        const double w = fmin(fmax(fmin((double)x + 1.0, ua1) - fmax((double)x, ua0), 0.), 1.);
        E[kk] += w * be[x - ch.u_lo];
        K[kk] += w * bk[x - ch.u_lo];
        EV[kk] += (w * w) * bv[x - ch.u_lo];
      }
    }
  }
  __syncthreads();
  // the waves' sums, added in wave order: the row buffers are free now (the barrier above)
  double* red = &buf[0][0][0];                               // [kExtractWaves][3][C]
#pragma unroll
  for (int kk = 0; kk < kChanPasses; ++kk) {
    const int b = kk * 64 + lane;
    if (b < C) {
      red[((size_t)wave * 3 + 0) * C + b] = E[kk];
      red[((size_t)wave * 3 + 1) * C + b] = K[kk];
      red[((size_t)wave * 3 + 2) * C + b] = EV[kk];
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * C; i += kExtractThreads) {
    double t = red[i];
    for (int w = 1; w < kExtractWaves; ++w) t += red[(size_t)w * 3 * C + i];
    oc.part[(((size_t)chunk * kChanGroups + group) * NP + p) * 3 * C + i] = t;
  }
}

// Behind k_extract_bins_opt: one workgroup per product adds the row groups in ascending order and writes
// channels_opt_p[b] = E_p[b] and channels_opt_var_p[b] = EV_p[b] + K_p[b]^2 sky_var_p (zeros for a product not formed).
__global__ void __launch_bounds__(kChanMaxChannels) k_extract_bins_opt_finish(ExtractArgs a, ChannelArgs ch, OptChanArgs oc) {
  const int p = (int)blockIdx.x, b = (int)threadIdx.x, C = ch.C, NP = a.R + 1;
  if (b >= C) return;
  if (p == a.R && !(a.steps & X_LAST_READ)) {
    oc.channels_opt[(size_t)p * C + b] = 0.;
    oc.channels_opt_var[(size_t)p * C + b] = 0.;
    return;
  }
  const int rows = a.row_hi[p] - a.row_lo[p];
  const int chunks = (rows + kExtractRows - 1) / kExtractRows;
  double E = 0., K = 0., EV = 0.;
  for (int c = 0; c < chunks * kChanGroups; ++c) {           // ascending chunks, ascending groups of a chunk
    const size_t at = ((size_t)c * NP + p) * 3 * C;
    E += oc.part[at + b];
    K += oc.part[at + C + b];
    EV += oc.part[at + 2 * C + b];
  }
  oc.channels_opt[(size_t)p * C + b] = E;
  oc.channels_opt_var[(size_t)p * C + b] = EV + (K * K) * a.sky_var[p];
}

}  // namespace wayne

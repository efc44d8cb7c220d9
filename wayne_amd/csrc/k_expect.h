// k_expect: the noise-free expected image of an exposure's thrower stage, per read interval (opt-in; no reference counterpart)
#pragma once
#include "common.h"
#include "k_prep.h"
#include "k_throw.h"

namespace wayne {

// ---------------------------------------------------------------------------
// k_expect : what the Monte-Carlo throwers converge to
// ---------------------------------------------------------------------------
// A thrower keeps an electron of a bin at c = (xs, ys) iff 0 < floor(c + sigma z) < N on both axes (pyparallel_menu.c:
// 91-93; common.h, bin_local), so the chance that it lands in frame pixel (y, x) is a product of two normal-CDF
// differences,
//     a(p; c, sigma) = Phi((p + 1 - c) / sigma) - Phi((p - c) / sigma)   for 1 <= p <= N - 1, else 0,
// with the float32 sigma the production throwers use.  The expected accumulator of read interval r is then
//     E_r[y + 5, x + 5] = sum_s sum_{k: read(k) = r} f_{s,k}(y, x) sum_w (n_h a(x; xs, sigma_h) a(y; ys, sigma_h)
//                                                                      + n_l a(x; xs, sigma_l) a(y; ys, sigma_l)),
// f the flat of sub-sample k (flat_value of k_throw.h; 1 without it), and (n_h, n_l) the bin's wide and narrow electrons:
//   MODE 1 (WAYNE_EXPECT_COUNTS): those of plan_bin for this run -- the same Philox draws, so E is the conditional
//          expectation of the run's accumulators given its bin counts;
//   MODE 2 (WAYNE_EXPECT_MEAN): the counts chain before the draw / the rounding, shared out by the clamped ratio.
// A component whose position is not finite or beyond +-1e6, or whose sigma is not finite or <= 0, contributes nothing.
//
// A gather: for one sub-sample and one component the inner sum is a matrix product with the bins as the inner
// dimension.  A workgroup owns a tile of kExpectTW x kExpectTH pixels of the read interval's box (planned by the host:
// plan::expected_boxes), a thread kExpectRows pixels of one column.  Bins are planned 256 at a time (a thread a bin:
// position, then -- only for a bin whose 8 sigma square meets the tile -- the counts); a batch of kExpectBatch bins that
// meets the tile fills two LDS tables per component, a_x over the tile's columns and n a_y over its rows (two erfc per
// table entry, none per pixel), and the threads run FMAs from them: the column's entry is read once per bin, the rows'
// entries are wave-uniform (broadcast reads).  The sum of a sub-sample is multiplied by f once and added to the
// thread's totals; the totals are added to the plane at the end (several sources: sequential launches on one stream).
// No atomics: every term is added in an order the plan fixes (sub-samples, then bins, ascending), so the bytes are the
// same in any slot, on either stream and on every run.
//
// Culling: a component is dropped from a pixel whose nearer edge lies more than kExpectCull = 8 sigma of THAT component
// from the bin, in x or in y -- never closer -- and a batch none of whose bins reaches the tile is skipped by a
// workgroup-uniform branch.  What any pixel of interval r can lose is bounded by 2 Phi(-8) x (electrons of interval r).
constexpr int kExpectThreads = 256;
constexpr int kExpectTW = 64, kExpectTH = 32;                                   // tile (px)
constexpr int kExpectBatch = 32;                                                // bins per pair of LDS tables
constexpr int kExpectRows = kExpectTH / (kExpectThreads / kExpectTW);           // pixels of a thread: 8
constexpr double kExpectCull = 8.0;
constexpr int kExpectMaxReads = 16;

struct ExpectArgs {
  int R, S;
  int box[kExpectMaxReads][4];   // per read interval: x0, x1, y0, y1 (frame px, inside [1, N)); x0 >= x1: nothing to render
  double* plane;                 // [R][S][S]; the launch ADDS into it
};

// a(p; c, sigma), each difference formed on the tail side so that it keeps its relative accuracy far from the bin
__device__ __forceinline__ double expect_cell(int p, double c, double sigma, int N) {
  if (p < 1 || p > N - 1) return 0.;
  const double lo = (double)p - c, hi = (double)(p + 1) - c;
  if (lo > kExpectCull * sigma || -hi > kExpectCull * sigma) return 0.;
  const double s = 0.70710678118654752440;
  const double t0 = (lo / sigma) * s, t1 = (hi / sigma) * s;
  if (t0 >= 0.) return 0.5 * (erfc(t0) - erfc(t1));
  if (t1 <= 0.) return 0.5 * (erfc(-t1) - erfc(-t0));
  return 0.5 * (erf(t1) + erf(-t0));
}

// does the 8 sigma square of a component at (xs, ys) meet the tile [x0, x1) x [y0, y1)?
__device__ __forceinline__ bool expect_reaches(double xs, double ys, float sigma, int x0, int x1, int y0, int y1) {
  if (!(sigma > 0.f && sigma < 3e38f)) return false;
  const double c = kExpectCull * (double)sigma;
  return (double)x0 - xs <= c && xs - (double)x1 <= c && (double)y0 - ys <= c && ys - (double)y1 <= c;
}

template <int MODE>
__global__ __launch_bounds__(kExpectThreads) void k_expect(PrepArgs p, ThrowArgs t, ExpectArgs e) {
  static_assert(kExpectThreads == 256 && kExpectTW == 64 && kExpectBatch == 32, "the index arithmetic below assumes these");
  const int r = blockIdx.y;
  const int N = p.N, W = p.W;
  const int bx0 = max(e.box[r][0], 1), bx1 = min(e.box[r][1], N), by0 = max(e.box[r][2], 1), by1 = min(e.box[r][3], N);
  if (bx0 >= bx1 || by0 >= by1) return;
  const int ntx = (bx1 - bx0 + kExpectTW - 1) / kExpectTW, nty = (by1 - by0 + kExpectTH - 1) / kExpectTH;
  if ((int)blockIdx.x >= ntx * nty) return;
  const int tx0 = bx0 + ((int)blockIdx.x % ntx) * kExpectTW, ty0 = by0 + ((int)blockIdx.x / ntx) * kExpectTH;
  const int tx1 = min(tx0 + kExpectTW, bx1), ty1 = min(ty0 + kExpectTH, by1);
  const int tid = threadIdx.x, col = tid & 63, wave = tid >> 6;
  const int row0 = wave * kExpectRows;          // the thread's pixels: column tx0 + col, rows ty0 + row0 + j
  const bool flat_on = (t.flags & 1u) && t.flat[0];   // WAYNE_F_ADD_FLAT (deposit_global)

  __shared__ double s_ax[2][kExpectBatch][kExpectTW];     // [component: 0 wide, 1 narrow]
  __shared__ double s_nay[2][kExpectBatch][kExpectTH];
  __shared__ double s_x[kExpectThreads], s_y[kExpectThreads], s_n[2][kExpectThreads];
  __shared__ float s_sig[2][kExpectThreads];
  __shared__ unsigned long long s_rel[2][kExpectThreads / 64];

  double tot[kExpectRows];
#pragma unroll
  for (int j = 0; j < kExpectRows; ++j) tot[j] = 0.;

  for (int k = 0; k < p.K; ++k) {
    if (p.sample_read[k] != r) continue;
    const double x_ref = p.x_ref[k], y_ref = p.y_ref[k], dur = p.dur_ms[k];
    const double* tr = p.tr + kTrStride * (size_t)k;
    double sub[kExpectRows];
#pragma unroll
    for (int j = 0; j < kExpectRows; ++j) sub[j] = 0.;
    bool any = false;

    for (int w0 = 0; w0 < W; w0 += kExpectThreads) {
      // plan: a thread a bin
      const int w = w0 + tid;
      double xs = 0., ys = 0., nh = 0., nl = 0.;
      float sh = 0.f, sl = 0.f;
      bool rel_h = false, rel_l = false;
      if (w < W) {
        const double wl = p.wl[w];
        bin_position(p, wl, tr, x_ref, y_ref, &xs, &ys);
        sh = (float)p.wa.sigh[w]; sl = (float)p.wa.sigl[w];
        const bool pos_ok = fabs(xs) < 1e6 && fabs(ys) < 1e6;      // (false for a NaN)
        rel_h = pos_ok && expect_reaches(xs, ys, sh, tx0, tx1, ty0, ty1);
        rel_l = pos_ok && expect_reaches(xs, ys, sl, tx0, tx1, ty0, ty1);
        if (rel_h || rel_l) {
          const double depth = p.depth ? p.depth[(size_t)k * W + w] : 0.;
          const double ratio = p.wa.ratio[w];
          if (MODE == 1) {
            const BinPlan b = plan_bin(p, k, w, wl, p.flux[w], p.wa.sens[w], p.wa.dlam[w], ratio, p.wa.sigl[w], tr, x_ref,
                                       y_ref, dur, depth);
            const uint32_t wide = (uint32_t)min(max(b.nwide, 0), (int32_t)min(b.count, 0x7FFFFFFFu));
            nh = (double)wide;
            nl = (double)(b.count - wide);
          } else {
            const double lam = bin_mean_counts(p, p.flux[w], p.wa.sens[w], p.wa.dlam[w], dur, depth);
            const double lp = (lam > 0. && __builtin_isfinite(lam)) ? fmin(lam, 2147483647.) : 0.;
            const double rho = ratio > 0. ? (ratio < 1. ? ratio : 1.) : 0.;
            nh = rho * lp;
            nl = lp - nh;
          }
          rel_h = rel_h && nh > 0.;
          rel_l = rel_l && nl > 0.;
        }
      }
      s_x[tid] = xs; s_y[tid] = ys;
      s_n[0][tid] = nh; s_n[1][tid] = nl;
      s_sig[0][tid] = sh; s_sig[1][tid] = sl;
      const unsigned long long mh = __ballot(rel_h), ml = __ballot(rel_l);
      if (col == 0) { s_rel[0][wave] = mh; s_rel[1][wave] = ml; }
      __syncthreads();

      for (int sb = 0; sb < kExpectThreads / kExpectBatch; ++sb) {
        if (w0 + sb * kExpectBatch >= W) break;
        uint32_t mask[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
          mask[c] = __builtin_amdgcn_readfirstlane((uint32_t)(s_rel[c][sb >> 1] >> (32 * (sb & 1))));
        if (!(mask[0] | mask[1])) continue;       // no bin of the batch reaches the tile (workgroup-uniform)
        const int q0 = sb * kExpectBatch;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (!mask[c]) continue;
          for (int i = tid; i < kExpectBatch * kExpectTW; i += kExpectThreads) {
            const int b = i >> 6, x = i & 63;
            if (!((mask[c] >> b) & 1u)) continue;
            s_ax[c][b][x] = (tx0 + x < tx1) ? expect_cell(tx0 + x, s_x[q0 + b], (double)s_sig[c][q0 + b], N) : 0.;
          }
          for (int i = tid; i < kExpectBatch * kExpectTH; i += kExpectThreads) {
            const int b = i >> 5, y = i & 31;
            if (!((mask[c] >> b) & 1u)) continue;
            s_nay[c][b][y] = (ty0 + y < ty1) ? s_n[c][q0 + b] * expect_cell(ty0 + y, s_y[q0 + b], (double)s_sig[c][q0 + b], N) : 0.;
          }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (!mask[c]) continue;
          for (int b = 0; b < kExpectBatch; ++b) {
            if (!((mask[c] >> b) & 1u)) continue;
            const double ax = s_ax[c][b][col];
#pragma unroll
            for (int j = 0; j < kExpectRows; ++j) sub[j] = fma(ax, s_nay[c][b][row0 + j], sub[j]);
          }
        }
        any = true;
        __syncthreads();       // the tables are refilled by the next batch
      }
      __syncthreads();         // ... and the bins' records by the next 256 bins
    }

    if (any) {                 // (workgroup-uniform)
      if (flat_on) {
        const SubInfo si = make_sub_info(p, k, x_ref, y_ref, tr, 0u, 1e300, -1e300, 1e300, -1e300);
#pragma unroll
        for (int j = 0; j < kExpectRows; ++j) {
          const int x = tx0 + col, y = ty0 + row0 + j;
          if (x < tx1 && y < ty1) tot[j] += flat_value(t, si, x, y) * sub[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < kExpectRows; ++j) tot[j] += sub[j];
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kExpectRows; ++j) {
    const int x = tx0 + col, y = ty0 + row0 + j;
    if (x < tx1 && y < ty1) e.plane[((size_t)r * e.S + (size_t)(y + kBorder)) * e.S + (size_t)(x + kBorder)] += tot[j];
  }
}

}  // namespace wayne

// k_ima: the calibrated reads of an exposure -- the instrument pipeline's intermediate file, `_ima` -- as the data
// sections of a FITS file, on the device (wayne_exposure_set_ima; opt-in; no reference counterpart: the law is the one
// tests/ima_law.py states in numpy, per pixel).
//
// All coordinates bordered, side S, n = S*S; everything in float64; a read of any stored type is promoted exactly.  For
// a light-sensitive pixel, with L_k, g and the step bits the extraction's (k_extract.h: extract_linear, extract_var's q;
// the gain step is required), rn the read noise of a difference of two reads and t_k the time of read k:
//   e_0 = 0, e_k = L_k g
//   good_0 = P_0 < sat_dn, good_k = good_{k-1} and P_k < sat_dn      (a NaN is not <; good_k for k >= 1 is k <= K, the
//                                                                     ramp fit's K)
//   s_k = sqrt(max(e_k, 0) + rn^2 (q q)),  q = g / 2.35               (k >= 1; s_0 = 0)
//   counts: SCI_k = (float)e_k            ERR_k = (float)s_k
//   rate  : SCI_k = (float)(e_k / t_k)    ERR_k = (float)(s_k / t_k)  (k >= 1; read 0: both 0)
//   DQ_k  = (good_k ? 0 : 256) | (bits 0 .. k-1 of the ramp fit's `jump` hold a 1 ? 8192 : 0)
// Reference pixels (the 5-pixel border) get SCI = ERR = 0 and DQ = 0.  The jump bits are the low half of the word
// k_ramp_fit has just written for the same run (RampFitArgs::word), when the slot has a ramp fit.
//
// The payload, imset f = 0 .. R holding read k = R - f (the last read first: k_fits_words's convention):
//   [f imset_stride                ..)  SCI_k, n big-endian float32, zeros to sci_stride
//   [f imset_stride + sci_stride   ..)  ERR_k, the same
//   [f imset_stride + 2 sci_stride ..)  DQ_k,  n big-endian int16, zeros to dq_stride
// sci_stride = 4n and dq_stride = 2n rounded up to 2880 = 32 * 90, imset_stride = 2 sci_stride + dq_stride.
//
// A streaming kernel in the manner of k_fits_words.  A lane owns a UNIT of 8 consecutive pixels: 16 bytes of a DQ
// section, 32 of a SCI or ERR section, so every store is 16 bytes a lane, and a float read or dark value arrives in two
// 16-byte loads (a double read in four; a uint16 read in two 8-byte loads -- with n = 4 mod 8 every other plane of
// uint16 reads starts at 8 mod 16).  It loads P_0, the four linearity coefficients, pfl and the ramp-fit word of its
// pixels once and then walks k = 1 .. R with one read and one dark value a pixel per step, those of step k + 1 asked for
// before step k's arithmetic and none of them behind a branch; the byte reversal happens in registers.  Both strides are whole units and n is a
// multiple of 4, so a unit is 8 pixels, 4 pixels and padding (the last one when n = 4 mod 8: every sub-array but 1024),
// or padding alone; pixels beyond n are treated as reference pixels, whose zeros are the padding's.  dq_stride / 16 >=
// sci_stride / 32 units cover a section: the grid strides over the former and guards the SCI / ERR stores of a unit of
// padding with the latter.  The padding is written on every run.  No LDS, no atomics, no register array indexed at run time: the payload
// is a function of the reads (and the ramp fit's word) alone -- the same bytes in any slot, on either stream, on every run.
//
// The file is compiled without FMA contraction (wayne_amd/build.py); float64 divide and sqrt and the cast to float32
// are correctly rounded, so a pixel's chain rounds as the numpy statement of it does.
#pragma once
#include "common.h"
#include "k_fits.h"

namespace wayne {

constexpr int kImaThreads = 256;
constexpr int kImaMaxBlocks = 4096;     // workgroups of a launch (16 per CU: the grid strides over the rest)
constexpr int kImaUnit = 8;             // pixels of a lane's unit
constexpr unsigned kImaDqSaturated = 256u, kImaDqJump = 8192u;

struct ImaArgs {
  int R, S;
  unsigned n;                        // S*S: a multiple of 4
  unsigned steps;                    // X_LINEARISE | X_DARK | X_GAIN (plan::ima_desc_error)
  int rate;                          // WAYNE_IMA_RATE: SCI and ERR over t_k
  double t[kMaxReads + 1];           // t_k: the read intervals summed in ascending order (t_0 = 0)
  double rn2, sat_dn;                // rn^2
  const void* reads;                 // [(R+1)*n] float, double or uint16_t
  const float* pfl;                  // [n] bordered (1 on the border) or null
  const float* lin[4];               // [n] or null
  const float* dark;                 // [R*n] or null
  const uint32_t* word;              // [n] K << 16 | jump of the slot's ramp fit, written by this run; null without one
  unsigned char* payload;            // [(R+1) * imset_stride]
  unsigned long long sci_stride, dq_stride, imset_stride;
};

// four consecutive samples of a plane, promoted; `p` is 16-byte aligned for float and double, 8-byte for uint16
__device__ __forceinline__ void ima_load4(const float* p, float (&v)[4]) {
  const fits_f32x4 x = *(const fits_f32x4*)p;
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void ima_load4(const double* p, double (&v)[4]) {
  typedef double ima_f64x2 __attribute__((ext_vector_type(2)));
  const ima_f64x2 x = *(const ima_f64x2*)p, y = *(const ima_f64x2*)(p + 2);
  v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
}
__device__ __forceinline__ void ima_load4(const unsigned short* p, unsigned short (&v)[4]) {
  const fits_u32x2 x = *(const fits_u32x2*)p;
  v[0] = (unsigned short)(x.x & 0xFFFFu); v[1] = (unsigned short)(x.x >> 16);
  v[2] = (unsigned short)(x.y & 0xFFFFu); v[3] = (unsigned short)(x.y >> 16);
}
__device__ __forceinline__ void ima_load4(const uint32_t* p, uint32_t (&v)[4]) {
  const fits_u32x4 x = *(const fits_u32x4*)p;
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}

// a unit of 8 samples: its first half, and its second at p + hi4 -- 4 where those pixels exist; 0 in the plane's last,
// half unit, which so reads its first half twice and no sample beyond the plane (the copies are masked as reference
// pixels are).  No load hangs on a condition: a branch around one would make the compiler wait for every load in flight.
template <class V>
__device__ __forceinline__ void ima_load8(const V* p, unsigned hi4, V (&v)[kImaUnit]) {
  V a[4], b[4];
  ima_load4(p, a);
  ima_load4(p + hi4, b);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}

// the 4 bytes of a float, most significant first, as the dword a little-endian store writes in that order
__device__ __forceinline__ unsigned ima_word(float v) { return __builtin_bswap32(__float_as_uint(v)); }

// 8 float32 values as the 32 bytes of a SCI / ERR section at `out`
__device__ __forceinline__ void ima_store_f32(unsigned char* out, const float (&v)[kImaUnit]) {
  fits_u32x4* o = (fits_u32x4*)out;
  o[0] = fits_u32x4{ima_word(v[0]), ima_word(v[1]), ima_word(v[2]), ima_word(v[3])};
  o[1] = fits_u32x4{ima_word(v[4]), ima_word(v[5]), ima_word(v[6]), ima_word(v[7])};
}

// two int16 values in a dword -> their stored words: the bytes of each half swapped (k_fits.h, fits_pair, without the flip)
__device__ __forceinline__ unsigned ima_pair(unsigned w) { return __builtin_amdgcn_perm(w, w, 0x02030001u); }

// 8 data-quality values (< 2^15) as the 16 bytes of a DQ section at `out`: two to a dword, the bytes of each half swapped
__device__ __forceinline__ void ima_store_dq(unsigned char* out, const unsigned (&q)[kImaUnit]) {
  fits_u32x4 w;
  w.x = ima_pair(q[0] | (q[1] << 16));
  w.y = ima_pair(q[2] | (q[3] << 16));
  w.z = ima_pair(q[4] | (q[5] << 16));
  w.w = ima_pair(q[6] | (q[7] << 16));
  *(fits_u32x4*)out = w;
}

template <class T>
__global__ void __launch_bounds__(kImaThreads) k_ima(ImaArgs a) {
  const int S = a.S, R = a.R;
  const unsigned n = a.n;
  const T* reads = (const T*)a.reads;
  const bool lin = (a.steps & X_LINEARISE) && a.lin[0];
  const bool dark = (a.steps & X_DARK) && a.dark;
  const unsigned dq_units = (unsigned)(a.dq_stride / 16u), sci_units = (unsigned)(a.sci_stride / 32u);
  const fits_u32x4 zero = {0u, 0u, 0u, 0u};

  for (unsigned u = blockIdx.x * kImaThreads + threadIdx.x; u < dq_units; u += gridDim.x * kImaThreads) {
    const size_t first = (size_t)kImaUnit * u;
    unsigned char* sci_out = a.payload + 32u * (size_t)u;                       // of imset 0
    unsigned char* dq_out = a.payload + 2 * a.sci_stride + 16u * (size_t)u;     // of imset 0
    if (first >= n) {     // padding alone, of every imset; beyond sci_stride / 32 units only the DQ section's
      for (int f = 0; f <= R; ++f) {
        const size_t at = (size_t)f * a.imset_stride;
        if (u < sci_units) {
          fits_u32x4* s = (fits_u32x4*)(sci_out + at);
          fits_u32x4* e = (fits_u32x4*)(sci_out + at + a.sci_stride);
          s[0] = zero; s[1] = zero;
          e[0] = zero; e[1] = zero;
        }
        *(fits_u32x4*)(dq_out + at) = zero;
      }
      continue;
    }
    // a unit with pixels lies inside both sections (4 n <= sci_stride): its stores hang on no condition either, so that
    // the wait for a step's loads does not have to allow for stores that were never issued, and so wait for them all
    const bool hi = first + kImaUnit <= n;     // (n is a multiple of 4: else the unit's second half is padding)
    const unsigned hi4 = hi ? 4u : 0u;

    // what the walk keeps of a pixel: P_0, 1 + c1 and the other three coefficients, g, rn^2 q^2, the jump bits; `inner`
    // and `good` a bit a pixel
    T P0[kImaUnit];
    float cf[4][kImaUnit], pf[kImaUnit];
    uint32_t jump[kImaUnit];
    ima_load8(reads + first, hi4, P0);
    if (lin) {
#pragma unroll
      for (int i = 0; i < 4; ++i) ima_load8(a.lin[i] + first, hi4, cf[i]);
    }
    if (a.pfl) ima_load8(a.pfl + first, hi4, pf);
    if (a.word) {
      ima_load8(a.word + first, hi4, jump);
    } else {
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) jump[i] = 0u;
    }
    // the first step's read and dark value
    T Pk[kImaUnit];
    float dk[kImaUnit];
    ima_load8(reads + (size_t)n + first, hi4, Pk);
    if (dark) ima_load8(a.dark + first, hi4, dk);

    unsigned inner = 0u, good = 0u;
    double p0[kImaUnit], g[kImaUnit], rq[kImaUnit];
    {
      int y = (int)(first / (unsigned)S), x = (int)(first - (size_t)y * S);
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) {
        const bool in = (i < 4 || hi) && x >= kBorder && x < S - kBorder && y >= kBorder && y < S - kBorder;
        inner |= (unsigned)in << i;
        if (++x == S) { x = 0; ++y; }
        p0[i] = (double)P0[i];
        good |= (unsigned)(p0[i] < a.sat_dn) << i;
        g[i] = a.pfl ? 2.35 / (double)pf[i] : 2.35;
        const double q = g[i] / 2.35;
        rq[i] = a.rn2 * (q * q);
        jump[i] &= 0xFFFFu;
      }
    }

    // read 0: the last imset
    {
      const size_t at = (size_t)R * a.imset_stride;
      unsigned q[kImaUnit];
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) q[i] = ((inner >> i) & 1u) && !((good >> i) & 1u) ? kImaDqSaturated : 0u;
      fits_u32x4* s = (fits_u32x4*)(sci_out + at);
      fits_u32x4* e = (fits_u32x4*)(sci_out + at + a.sci_stride);
      s[0] = zero; s[1] = zero;
      e[0] = zero; e[1] = zero;
      ima_store_dq(dq_out + at, q);
    }

    // The coefficients and the first step's read and dark value are first used inside the walk.  Were their loads still
    // in flight at its head, every step would carry the waits that retire them -- counts that, from the second step on,
    // retire the previous step's stores instead.  An empty statement that takes them as operands settles them here.
#pragma unroll
    for (int i = 0; i < kImaUnit; ++i) {
      asm volatile("" ::"v"(Pk[i]));
      if (dark) asm volatile("" ::"v"(dk[i]));
      if (lin) {
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(cf[j][i]));
      }
    }

    for (int k = 1; k <= R; ++k) {
      // step k + 1's loads, in front of step k's arithmetic (the last step asks for its own planes once more)
      T Pn[kImaUnit];
      float dn[kImaUnit];
      const int kn = k < R ? k + 1 : R;
      ima_load8(reads + (size_t)kn * n + first, hi4, Pn);
      if (dark) ima_load8(a.dark + (size_t)(kn - 1) * n + first, hi4, dn);
      const double tk = a.t[k];
      // The unit's 8 chains are independent.  The uniform switches (linearise, dark, units) are taken once a step, around
      // all 8, and a reference pixel is a select at the end, so that the chains stand in one block and hide each other's
      // float64 latency.
      double e[kImaUnit], sg[kImaUnit];
      unsigned q[kImaUnit];
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) {
        const double P = (double)Pk[i];
        good &= ~((unsigned)!(P < a.sat_dn) << i);
        e[i] = P - p0[i];
        const bool in = (inner >> i) & 1u;
        q[i] = in ? (((good >> i) & 1u) ? 0u : kImaDqSaturated) | ((jump[i] & ((1u << k) - 1u)) ? kImaDqJump : 0u) : 0u;
      }
      if (lin) {
#pragma unroll
        for (int i = 0; i < kImaUnit; ++i) {
          const double D = e[i];
          e[i] = D * (1.0 + (double)cf[0][i] + D * ((double)cf[1][i] + D * ((double)cf[2][i] + (double)cf[3][i] * D)));
        }
      }
      if (dark) {
#pragma unroll
        for (int i = 0; i < kImaUnit; ++i) e[i] -= (double)dk[i];
      }
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) {
        e[i] *= g[i];
        sg[i] = sqrt((e[i] < 0. ? 0. : e[i]) + rq[i]);
      }
      if (a.rate) {
#pragma unroll
        for (int i = 0; i < kImaUnit; ++i) { e[i] /= tk; sg[i] /= tk; }
      }
      float sci[kImaUnit], err[kImaUnit];
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) {
        const bool in = (inner >> i) & 1u;
        sci[i] = in ? (float)e[i] : 0.f;
        err[i] = in ? (float)sg[i] : 0.f;
      }
      const size_t at = (size_t)(R - k) * a.imset_stride;
      ima_store_f32(sci_out + at, sci);
      ima_store_f32(sci_out + at + a.sci_stride, err);
      ima_store_dq(dq_out + at, q);
#pragma unroll
      for (int i = 0; i < kImaUnit; ++i) { Pk[i] = Pn[i]; dk[i] = dn[i]; }
    }
  }
}

}  // namespace wayne

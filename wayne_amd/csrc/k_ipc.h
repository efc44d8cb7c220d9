// k_ipc, k_ipc_clear: inter-pixel capacitance -- every read interval's collected charge coupled into the eight
// neighbours (wayne_exposure_set_ipc; opt-in; no reference counterpart: the law is the one tests/ipc_law.py states in
// numpy on int64).
//
// All coordinates bordered, side S, n = S*S.  q_r = acc[r] are the thrower's accumulators of read interval r (int64
// fixed point, 2^-28 e-), W the nine integer weights of wayne_ipc_weights (sum 65536):
//   q'_r[y, x] = floor((sum_{dy, dx in -1..1} W[dy+1][dx+1] q_r[y+dy, x+dx] + 32768) / 65536)   light-sensitive pixels
//   q'_r[y, x] = 0                                                                             the 5-pixel border
// W[1][2] is what a pixel receives from its right-hand neighbour.  A light-sensitive pixel's neighbours all lie inside
// the frame (the border is 5 wide), so "0 beyond the frame" needs no test.  The sum is exact for any int64 input: q is
// split into its arithmetic high half and unsigned low 32 bits, S_hi = sum W hi (|S_hi| <= 2^47), S_lo = sum W lo
// (<= 2^48), and q' = (S_hi << 16) + ((S_lo + 32768) >> 16) -- S_hi 2^32 is a multiple of 2^16, so the floor acts on the
// low sum alone.
//
// k_ipc is a gather: it reads A (the thrower's accumulators) and writes B, the accumulators k_ramp is then pointed at;
// no atomics, plain cached loads (nine 8-byte loads a pixel and interval, three rows of a wave's 64 consecutive pixels:
// each row is 66 consecutive int64 that the wave's lanes share through L1/L2 -- an LDS tile with a halo would add a
// barrier per interval and buys nothing a cache line does not already give: 34 VGPRs, no LDS, no scratch).
//
// Work only where something is live, by k_ramp's own rule and shape: a wave owns 64 consecutive flat pixels and handles
// read interval r only when they meet box[r] (here: the box dilated by one pixel, clamped to the frame) or a cosmic-ray
// hit's 3 x 3 neighbourhood touches them.  The second is a gather too: the wave ORs the segment words of A that hold
// flat indices [p0 + dy S - 1, p0 + dy S + 64], dy = -1, 0, 1 (up to three words a row), and writes the union as ITS
// word of the second bit array seg_b -- one writer per word, no atomics, so the bits do not depend on scheduling.  A
// word of seg_b may cover more than the hits' exact neighbourhoods (a whole segment of A counts as hit); k_ramp then
// loads a few zeros.  k_ipc writes B[r] exactly for the (wave, r) pairs k_ramp will load -- the same two tests on the
// same numbers -- so k_ramp, which clears what it loads, leaves B clean; outside them B stays at the zeros it holds.
//
// k_ipc_clear, behind it on the stream, leaves A and its segment bits clean: it zeroes A[r] on the UNDILATED live set
// (box[r] or the wave's own segment word: what k_ramp would have loaded and cleared without the option) and the word.
// Nothing else of A was ever written.  Two launches because a wave's neighbours read A until the first has finished.
#pragma once
#include "common.h"

namespace wayne {

constexpr int kIpcThreads = 256;

struct IpcArgs {
  int R, S;
  int use_box;               // 0: every (wave, r) is live (k_ramp loads everything)
  int box[16][4];            // {x0, x1, y0, y1} per read interval: dilated for k_ipc, the planner's own for k_ipc_clear
  int w[9];                  // W[dy+1][dx+1], row-major
  long long* a;              // [R*n] the thrower's accumulators: read by k_ipc, cleared by k_ipc_clear
  long long* b;              // [R*n] the coupled accumulators (k_ipc)
  uint32_t* seg_a;           // [ceil(n / 64)] bit r: a hit in read interval r among the segment's accumulators of A
  uint32_t* seg_b;           // [ceil(n / 64)] the same for B: written by k_ipc, read and cleared by k_ramp
};

// bit r: the wave at p0 handles read interval r -- k_ramp's test (acc_live) on `box` and the bits `cbits`
__device__ __forceinline__ unsigned long long ipc_live(const IpcArgs& a, int p0, uint32_t cbits) {
  if (!a.use_box) return ~0ull;
  const int S = a.S, lane = threadIdx.x & 63, lr = min(lane, 15);
  const int bx0 = a.box[lr][0], bx1 = a.box[lr][1], by0 = a.box[lr][2], by1 = a.box[lr][3];
  const int wy0 = p0 / S, wy1 = min(p0 + 63, S * S - 1) / S, wx0 = p0 - wy0 * S;
  const bool rows = wy0 < by1 && wy1 >= by0;
  const bool cols = (wy0 != wy1) || (wx0 < bx1 && wx0 + 64 > bx0);
  return __ballot(lane < 16 && ((rows && cols) || ((cbits >> lr) & 1u) != 0u));
}

__global__ __launch_bounds__(kIpcThreads) void k_ipc(IpcArgs a) {
  const int S = a.S, n = S * S;
  const int p = blockIdx.x * kIpcThreads + threadIdx.x;
  const int p0 = __builtin_amdgcn_readfirstlane(p) & ~63;
  if (p0 >= n) return;
  // the hits whose neighbourhood reaches this wave's pixels
  uint32_t cbits = 0u;
  if (a.use_box) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int lo = max(p0 + dy * S - 1, 0), hi = min(p0 + dy * S + 64, n - 1);
      if (lo > hi) continue;
      for (int w = lo >> 6; w <= (hi >> 6); ++w) cbits |= a.seg_a[w];
    }
    cbits = __builtin_amdgcn_readfirstlane(cbits);
    if (cbits != 0u && (threadIdx.x & 63) == 0) a.seg_b[p0 >> 6] = cbits;
  }
  const unsigned long long live = ipc_live(a, p0, cbits) & ((1ull << a.R) - 1ull);
  if (live == 0ull || p >= n) return;
  const int y = p / S, x = p - y * S;
  const bool interior = x >= kBorder && x < S - kBorder && y >= kBorder && y < S - kBorder;
  for (int r = 0; r < a.R; ++r) {
    if (((live >> r) & 1ull) == 0ull) continue;           // scalar
    const size_t plane = (size_t)r * (size_t)n;
    long long out = 0;
    if (interior) {
      const long long* q = a.a + plane + p;
      long long s_hi = 0;
      unsigned long long s_lo = 0ull;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const long long v = q[dy * S + dx];
          const int w = a.w[(dy + 1) * 3 + (dx + 1)];
          s_hi += (long long)w * (long long)(int)(v >> 32);
          s_lo += (unsigned long long)(unsigned)w * (unsigned long long)(unsigned)v;
        }
      }
      out = (long long)(((unsigned long long)s_hi << 16) + ((s_lo + 32768ull) >> 16));
    }
    a.b[plane + p] = out;
  }
}

__global__ __launch_bounds__(kIpcThreads) void k_ipc_clear(IpcArgs a) {
  const int S = a.S, n = S * S;
  const int p = blockIdx.x * kIpcThreads + threadIdx.x;
  const int p0 = __builtin_amdgcn_readfirstlane(p) & ~63;
  if (p0 >= n) return;
  uint32_t cbits = 0u;
  if (a.use_box) {
    cbits = __builtin_amdgcn_readfirstlane(a.seg_a[p0 >> 6]);
    if (cbits != 0u && (threadIdx.x & 63) == 0) a.seg_a[p0 >> 6] = 0u;
  }
  const unsigned long long live = ipc_live(a, p0, cbits) & ((1ull << a.R) - 1ull);
  if (live == 0ull || p >= n) return;
  for (int r = 0; r < a.R; ++r)
    if ((live >> r) & 1ull) a.a[(size_t)r * (size_t)n + p] = 0;
}

}  // namespace wayne

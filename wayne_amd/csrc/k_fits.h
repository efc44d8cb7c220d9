// k_fits_words: the reads of an exposure as the data sections of its FITS file (opt-in: wayne_exposure_set_fits).
//
// For the slot's reads P_0 .. P_R (each n = S*S samples of type T, read 0 first) the payload holds, plane f = 0 .. R,
//
//   payload[f*stride + i*B ...]                      = words(P_{R-f}[i])     the LAST read first: the file's HDU order
//   payload[f*stride + n*B .. (f + 1)*stride)        = 0                     the HDU's padding to the 2880-byte block
//
//   words(v)  float  : the 8 bytes of (double)v, most significant first  (BITPIX -64; the widening is exact)
//             double : the 8 bytes of v, most significant first          (BITPIX -64)
//             uint16 : the 2 bytes of v ^ 0x8000, most significant first (BITPIX 16, BZERO 32768: value - 32768 as int16)
//
// so that plane f is one contiguous piece of a file: an image HDU's data section and its padding.  No reference
// counterpart: the reference writes its files through astropy on the host (exposure.py:133-214).
//
// A streaming kernel: 16 bytes per lane per access on both sides, the byte reversal in registers, no LDS, no atomics.
// A lane takes a UNIT of the output -- float / double: 4 samples, one or two 16-byte loads and two 16-byte stores;
// uint16: 8 samples, one 16-byte load and one 16-byte store -- and the grid is (units of a plane, capped and strided
// over; plane).  stride is a multiple of 2880 = 32 * 90, so a plane is a whole number of units of either size and every
// plane of the payload starts 16-byte aligned; n is a multiple of 4 (S is even), so a float / double unit is all samples
// or all padding, and a uint16 unit all samples, its first half (n = 4 mod 8: every sub-array but 1024), or all padding.
// The padding is written on every run: the same buffer serves other strides (another sample type) between uploads.
#pragma once
#include "common.h"

namespace wayne {

constexpr int kFitsThreads = 256;
constexpr int kFitsBlock = 2880;        // the FITS block: a data section is padded to a multiple of it
constexpr int kFitsMaxBlocks = 4096;    // workgroups of a launch, all planes together (16 per CU: the grid strides over the rest)

struct FitsArgs {
  const void* reads;                 // [planes][n] samples, read 0 first (Slot::out)
  unsigned char* payload;            // [planes][stride] bytes
  int planes;                        // R + 1
  unsigned n;                        // samples of a plane, S*S: a multiple of 4
  unsigned long long stride;         // bytes of a plane of the payload: n * B rounded up to a multiple of kFitsBlock
};

typedef unsigned long long fits_u64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int fits_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int fits_u32x2 __attribute__((ext_vector_type(2)));
typedef float fits_f32x4 __attribute__((ext_vector_type(4)));

// the 8 bytes of a double, most significant first, as the u64 a little-endian store writes in that order
__device__ __forceinline__ unsigned long long fits_word(double v) {
  return __builtin_bswap64((unsigned long long)__double_as_longlong(v));
}

// two uint16 samples in a dword -> their stored words in a dword: the bytes of each half swapped (one v_perm_b32:
// selector byte k names the source byte that lands at byte k), then the top bit of each sample flipped -- after the
// swap it is bit 7 of bytes 0 and 2
__device__ __forceinline__ unsigned fits_pair(unsigned w) {
  return __builtin_amdgcn_perm(w, w, 0x02030001u) ^ 0x00800080u;
}

template <class T>
__device__ __forceinline__ void fits_unit(const T* __restrict__ in, unsigned char* __restrict__ out, unsigned u, unsigned n, bool in16);

// float: unit u = samples 4u .. 4u + 3 -> 32 bytes at 32u
template <>
__device__ __forceinline__ void fits_unit<float>(const float* __restrict__ in, unsigned char* __restrict__ out, unsigned u, unsigned n, bool) {
  fits_u64x2 a = {0ull, 0ull}, b = {0ull, 0ull};
  if (4u * u < n) {     // (n is a multiple of 4: the whole unit is samples)
    const fits_f32x4 v = *(const fits_f32x4*)(in + 4u * (size_t)u);
    a = fits_u64x2{fits_word((double)v.x), fits_word((double)v.y)};
    b = fits_u64x2{fits_word((double)v.z), fits_word((double)v.w)};
  }
  fits_u64x2* o = (fits_u64x2*)(out + 32u * (size_t)u);
  o[0] = a;
  o[1] = b;
}

// double: unit u = samples 4u .. 4u + 3 -> 32 bytes at 32u
template <>
__device__ __forceinline__ void fits_unit<double>(const double* __restrict__ in, unsigned char* __restrict__ out, unsigned u, unsigned n, bool) {
  fits_u64x2 a = {0ull, 0ull}, b = {0ull, 0ull};
  if (4u * u < n) {
    const fits_u64x2* p = (const fits_u64x2*)(in + 4u * (size_t)u);
    const fits_u64x2 x = p[0], y = p[1];
    a = fits_u64x2{__builtin_bswap64(x.x), __builtin_bswap64(x.y)};
    b = fits_u64x2{__builtin_bswap64(y.x), __builtin_bswap64(y.y)};
  }
  fits_u64x2* o = (fits_u64x2*)(out + 32u * (size_t)u);
  o[0] = a;
  o[1] = b;
}

// uint16: unit u = samples 8u .. 8u + 7 -> 16 bytes at 16u.  `in16`: the plane starts 16-byte aligned in `reads` (with
// n = 4 mod 8 every other plane starts at 8 mod 16: two 8-byte loads there)
template <>
__device__ __forceinline__ void fits_unit<unsigned short>(const unsigned short* __restrict__ in, unsigned char* __restrict__ out, unsigned u, unsigned n,
                                                          bool in16) {
  fits_u32x4 w = {0u, 0u, 0u, 0u};
  const unsigned first = 8u * u;
  if (first + 8u <= n) {
    const unsigned short* p = in + (size_t)first;
    if (in16) {
      w = *(const fits_u32x4*)p;
    } else {
      const fits_u32x2 lo = *(const fits_u32x2*)p, hi = *(const fits_u32x2*)(p + 4);
      w = fits_u32x4{lo.x, lo.y, hi.x, hi.y};
    }
    w = fits_u32x4{fits_pair(w.x), fits_pair(w.y), fits_pair(w.z), fits_pair(w.w)};
  } else if (first + 4u <= n) {     // the half vector left over: 4 samples, then 8 bytes of padding
    const fits_u32x2 lo = *(const fits_u32x2*)(in + (size_t)first);
    w = fits_u32x4{fits_pair(lo.x), fits_pair(lo.y), 0u, 0u};
  }
  *(fits_u32x4*)(out + 16u * (size_t)u) = w;
}

template <class T>
__global__ __launch_bounds__(kFitsThreads) void k_fits_words(FitsArgs a) {
  constexpr unsigned kUnitBytes = sizeof(T) == 2 ? 16u : 32u;
  const unsigned f = blockIdx.y;                                   // plane of the payload
  const unsigned units = (unsigned)(a.stride / kUnitBytes);        // of a plane, padding included
  const size_t in_plane = (size_t)(a.planes - 1 - (int)f) * a.n;   // the last read first
  const T* in = (const T*)a.reads + in_plane;
  unsigned char* out = a.payload + (size_t)f * a.stride;
  const bool in16 = ((in_plane * sizeof(T)) & 15u) == 0;
  for (unsigned u = blockIdx.x * kFitsThreads + threadIdx.x; u < units; u += gridDim.x * kFitsThreads) fits_unit<T>(in, out, u, a.n, in16);
}

}  // namespace wayne

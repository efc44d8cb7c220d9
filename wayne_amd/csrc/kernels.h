// HIP kernels (gfx950) of the WFC3-IR exposure-synthesis path, one header per stage:
//
//   k_lightcurve.h  k_lightcurve   transit depths depth[K][W] from z[K], rp[W], limb darkening
//   k_lightcurve_ld.h  k_lightcurve_ld   opt-in: the same matrix with four Claret coefficients per wavelength bin
//   k_lightcurve_spots.h  k_lightcurve_spots   opt-in: star spots -- rewrites that matrix in place (occulted and unocculted)
//   k_prep.h        k_prep_wl      per-wavelength arrays: PSF polynomials, sensitivity LUT, bin widths   (A8, A9) -- when a
//                                  source's grid is uploaded, not per run (k_prep_wl_run: the per-run form, knob prep_wl_per_run)
//                   k_prep_sub     per sub-sample: trace, bin positions, expected counts, Poisson/round,
//                                  sigma split, routing of the bins, prefix, electron count and clip rectangle
//                                  per sub-sample; cosmic-ray hits per read interval          (A6, A7, A9, A10, A13, cosmic_rays.py)
//   k_throw.h       k_throw        the electron thrower: LDS int32 tile per workgroup slice,
//                                  flushed x flat into the read-interval accumulator                     (A1-A4, A11, A12)
//   k_narrow.h      k_narrow       narrow PSF component as one multinomial per bin
//                   k_lane         a bin's one-by-one electrons (wide component, thin bins) thrown by its own lane
//                   k_lane_fused   thin exposures: k_lane planning its bins itself (plan_bin of k_prep.h), no k_prep_sub
//                   k_thrower      k_lane and k_narrow of the production pair as ONE grid (knob fuse_thrower)
//   k_ramp.h        k_ramp         fused up-the-ramp kernel: sky, gain, cumulative, dark, non-linearity,
//                                  clip, reference pixels, zero read, read noise                          (A13-A15)
//   k_extract.h     k_extract_rows / k_extract_finish   opt-in: column spectra per read interval from the reads
//                                  just written (linearise, dark, gain, row sums, sky level), no reference counterpart
//                   k_extract_crmask                    opt-in on top of it: the cosmic-ray flag plane of the difference images
//   k_fits.h        k_fits_words   opt-in: the reads as the big-endian data sections of their FITS file, in file order,
//                                  padding included (a streaming byte reversal), no reference counterpart
//   k_expect.h      k_expect       opt-in: the noise-free expected image of the thrower stage per read interval (the law
//                                  the Monte-Carlo throwers converge to, as a gather), no reference counterpart
//   k_rampfit.h     k_ramp_fit     opt-in: every pixel's up-the-ramp samples fitted with a line (saturated samples
//                                  dropped, jumps cut out): rate, variance and flag word planes, no reference counterpart
//   k_ima.h         k_ima          opt-in: the calibrated reads (electrons or e-/s, error, data quality) as the data sections
//                                  of an `_ima` FITS file (a streaming kernel over 8-pixel units), no reference counterpart
//   k_ipc.h         k_ipc / k_ipc_clear   opt-in: inter-pixel capacitance -- each read interval's accumulators coupled into
//                                  their eight neighbours in exact integer arithmetic, in front of k_ramp, no reference counterpart
//
// "A<n>" are the row ids of SURVEY.md section 8(a); reference file:line
// citations are next to each formula.
#pragma once
#include "common.h"
#include "k_lightcurve.h"
#include "k_lightcurve_ld.h"
#include "k_lightcurve_spots.h"
#include "k_prep.h"
#include "k_throw.h"
#include "k_narrow.h"
#include "k_ramp.h"
#include "k_extract.h"
#include "k_fits.h"
#include "k_expect.h"
#include "k_rampfit.h"
#include "k_ima.h"
#include "k_ipc.h"

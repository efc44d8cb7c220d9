/*
 * wayne_hip.h -- C ABI of libwayne_hip.so, the MI355X (gfx950) WFC3-IR
 * exposure-synthesis path.  Plain pointers and sizes only; bound from Python
 * with ctypes (wayne_amd/_lib.py) and from anything else that can call C.
 *
 * Each entry point names the reference interface it replaces
 * (file:line under the ucl-exoplanets/wayne tree).
 *
 * Conventions
 *   - every function returning int returns WAYNE_OK (0) or a negative
 *     WAYNE_E_* code; wayne_last_error(ctx) gives the message;
 *   - host pointers are borrowed for the duration of the call only;
 *   - the library owns all device memory; one wayne_ctx per GPU / stream;
 *     calls on distinct contexts are thread-safe, calls on one are not;
 *   - frames are row-major, y-major: pixel (y, x) at [y * side + x], exactly
 *     as the reference's `pixel_array[ypos*nc + xpos]` (pyparallel_menu.c:94).
 *   - N = light-sensitive side (SUBARRAY, or 1014 for SUBARRAY 1024),
 *     S = N + 10 = side with the 5-px reference border (detector.py:102-124).
 */
#ifndef WAYNE_HIP_H
#define WAYNE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAYNE_ABI_VERSION 7

/* status codes */
#define WAYNE_OK 0
#define WAYNE_E_INVALID (-1)   /* bad argument / shape                       */
#define WAYNE_E_NEGATIVE (-2)  /* negative electron count                     */
#define WAYNE_E_OVERFLOW (-3)  /* sum(counts)*threads >= 2^31 in replay mode   */
#define WAYNE_E_NOMEM (-4)     /* host or device allocation failed             */
#define WAYNE_E_HIP (-5)       /* a HIP runtime call failed                    */
#define WAYNE_E_NODEVICE (-6)  /* no usable gfx950 device                      */
#define WAYNE_E_STATE (-7)     /* grism / calibration / upload missing         */

/* rng_mode */
#define WAYNE_RNG_REPLAY 0 /* glibc rand_r streams + OpenMP partition of the reference: bit-exact */
#define WAYNE_RNG_PHILOX 1 /* Philox-keyed streams, every electron thrown individually */
#define WAYNE_RNG_SPLIT 2  /* production default: a bin with >= 32 narrow electrons has its narrow
                              component drawn as ONE multinomial (binomial chains, k_narrow); what is left
                              to throw one by one -- its wide electrons, or the whole of a bin that does
                              not qualify -- is thrown by the bin's own lane from the bin's own stream
                              (k_lane), or, beyond 4096 such electrons, shared out as in mode 1.
                              Same distribution of the frame, several times less work            */

/* wayne_exposure_desc.flags -- the keyword switches of
 * ExposureGenerator.scanning_frame (exposure_generator.py:178-192) */
#define WAYNE_F_ADD_FLAT (1u << 0)
#define WAYNE_F_ADD_GAIN_VARIATIONS (1u << 1)
#define WAYNE_F_ADD_NON_LINEAR (1u << 2)
#define WAYNE_F_CLIP_DET_LIMITS (1u << 3)
#define WAYNE_F_ADD_READ_NOISE (1u << 4)
#define WAYNE_F_ADD_STELLAR_NOISE (1u << 5)
#define WAYNE_F_ADD_DARK (1u << 6)
#define WAYNE_F_ADD_INITIAL_BIAS (1u << 7)
#define WAYNE_F_OUT_F64 (1u << 16) /* reads delivered as float64 (the reference's dtype) instead of float32 */
#define WAYNE_F_EXACT_SAMPLERS (1u << 17) /* IEEE divide/sqrt + libm-grade log/exp/sin/cos in the per-pixel
                                             Poisson / normal draws (parity runs) instead of the hardware
                                             approximations (production); same algorithm, same streams */
#define WAYNE_F_OUT_U16 (1u << 18) /* reads delivered as 16-bit unsigned DN, the ADC's sample type: the float32 read
                                      rounded half to even and saturated to 0 .. 65535 (NaN -> 0) in the ramp kernel's
                                      store.  Not together with WAYNE_F_OUT_F64: WAYNE_E_INVALID at upload */

typedef struct wayne_ctx wayne_ctx;

/* ---- context ---------------------------------------------------------- */

int wayne_abi_version(void);
const char *wayne_strerror(int status);
/* The compile-time switches (-DWAYNE_...) of this build that change what the library computes or launches, separated
 * by spaces: "" for the shipped library.  Negative-control and timing builds (tests/native, scripts/) name theirs
 * here, so that a measurement or a file can say which library produced it and refuse a defective one. */
const char *wayne_build_flags(void);

/* Number of HIP devices visible (0 when there is none / no driver). */
int wayne_device_count(void);

/* Create a context on `device` with its own HIP stream.  NULL on failure
 * (*status, if given, says why).  Fails -- never falls back to the CPU --
 * when no gfx950 GPU is present. */
wayne_ctx *wayne_ctx_create(int device, int *status);
void wayne_ctx_destroy(wayne_ctx *ctx);
const char *wayne_last_error(const wayne_ctx *ctx);
/* Wait for everything enqueued on the context AND settle it: the status word of every exposure run since the last
 * look is read (one copy for all slots); an exposure that met a bin beyond the reach of the short launch sequence
 * chosen from the host's electron estimate is run a second time with the general sequence (wayne_ctx_reruns counts
 * them), an overflow is reported as WAYNE_E_OVERFLOW.  After WAYNE_OK the reads of every slot are complete: this is
 * the call a throughput loop of wayne_exposure_run ends with. */
int wayne_ctx_synchronize(wayne_ctx *ctx);
/* Tuning and test knobs.  Each is read ONCE from the environment (WAYNE_<NAME IN CAPITALS>) by wayne_ctx_create; no
 * other entry point looks at the environment, so editing it from another thread cannot change what a live context
 * launches.  Afterwards only this call changes a knob (value < 0: back to the library's own choice).  Names:
 * tile_ints, batch, thin, no_acc_box, lane_reach, throw_wgs, keep_narrow, no_fuse, fork_narrow, streams,
 * upload_timing, narrow_compact, lane_tight_tile, fuse_thrower, prep_wl_per_run, ramp_reads (timing builds only).  None changes a frame (integer
 * accumulation commutes); they change launch shapes.  WAYNE_E_INVALID for an unknown name. */
int wayne_ctx_set_knob(wayne_ctx *ctx, const char *name, long long value);
int wayne_ctx_get_knob(const wayne_ctx *ctx, const char *name, long long *value);
/* The context's hipStream_t (as void*), for callers that interoperate. */
void *wayne_ctx_stream(wayne_ctx *ctx);

/* ---- inner boundary: the electron thrower ------------------------------ */

/*
 * Drop-in for  int *PSF(counts,size,x_pos,y_pos,psf_ratio,psf_sigmal,
 *                       psf_sigmah,nr,nc,test,threads)
 * (wayne/pyparallel_menu.h:1-3, pyparallel_menu.c:10-113) and therefore for
 * wayne.pyparallel.apply_psf (wayne/pyparallel.pyx:14-38), called once per
 * sub-sample at exposure_generator.py:636-639.
 *
 * Differences from the reference signature: the frame is written into the
 * caller's `out` (nr*nc int32) instead of a malloc'd buffer the caller must
 * free (pyparallel.pyx:36); `seed` is the reference's `test`;
 * `threads_compat` selects the reference's OpenMP partition in replay mode
 * (the result depends on it, pyparallel_menu.c:47-52) and never starts CPU
 * threads; in Philox mode `exposure`/`subsample` extend the counter.
 * WAYNE_RNG_REPLAY reproduces the reference frame bit for bit.
 */
int wayne_psf_apply(wayne_ctx *ctx, const int32_t *counts, int size,
                    const double *x_pos, const double *y_pos,
                    const double *psf_ratio, const double *psf_sigmal,
                    const double *psf_sigmah, int nr, int nc, uint32_t seed,
                    int threads_compat, int rng_mode, uint32_t exposure,
                    uint32_t subsample, int32_t *out);
/* The same with `flags`: WAYNE_F_EXACT_SAMPLERS runs the split mode's binomial chains (k_narrow) with IEEE
 * divide and libm-grade exp / log instead of the hardware approximations -- same algorithm, same streams; for
 * parity runs against oracle/split_oracle.c.  wayne_psf_apply is this call with flags = 0 (production math). */
int wayne_psf_apply_ex(wayne_ctx *ctx, const int32_t *counts, int size,
                       const double *x_pos, const double *y_pos,
                       const double *psf_ratio, const double *psf_sigmal,
                       const double *psf_sigmah, int nr, int nc, uint32_t seed,
                       int threads_compat, int rng_mode, uint32_t exposure,
                       uint32_t subsample, uint32_t flags, int32_t *out);

/* ---- grism and calibration (uploaded once per context) ----------------- */

/* What grism.G141 / grism.G102 hold (grism.py:24-118, 426-476, 756-776). */
typedef struct wayne_grism_desc {
  double trace_coeff[9];     /* aXe trace polynomial   (grism.py:756-764)   */
  double wl_solution[9];     /* aXe dispersion solution (grism.py:768-776)  */
  double psf_ratio_poly[4];  /* np.poly1d coefficients, highest power first */
  double psf_sigmal_poly[4]; /*   (grism.py:85-90)                          */
  double psf_sigmah_poly[4];
  int n_sens;                /* sensitivity table (grism.py:97-106)         */
  const double *sens_wl_um;  /* micron; finite and non-decreasing (np.interp's precondition), */
  const double *sens_val;    /* finite values: otherwise WAYNE_E_INVALID and nothing changes     */
  double flat_wmin, flat_wmax; /* WMIN / WMAX of the flat cube (grism.py:71-72), angstrom */
} wayne_grism_desc;

int wayne_ctx_set_grism(wayne_ctx *ctx, const wayne_grism_desc *g);

/*
 * Calibration planes for one (SUBARRAY, SAMPSEQ, NSAMP) mode, already
 * centre-cropped to the sub-array by the caller (tools.crop_central_box,
 * tools.py:317-324; detector.py:328-333).  float32 as in the CALWF3 files.
 * Any pointer may be NULL when the matching flag is never used.
 */
typedef struct wayne_calibration {
  int subarray;          /* 64, 128, 256, 512 or 1024                          */
  int n_reads;           /* R = NSAMP - 1 non-zero reads                       */
  const float *flat[4];  /* N*N each: flat cube planes f0..f3 (grism.py:73-76) */
  const float *pfl;      /* N*N: pixel flat; gain = 2.35 / pfl (detector.py:200-209) */
  const float *sky;      /* N*N: master sky (grism.py:411-423)                 */
  const float *lin[4];   /* S*S each: non-linearity c1..c4 (detector.py:58-67) */
  const float *dark_sci; /* R*S*S: super-dark SCI of non-zero read r (detector.py:185-188) */
  const float *dark_err; /* R*S*S: its ERR                                      */
  const double *zero_read; /* S*S initial bias or NULL (exposure_generator.py:446-466) */
} wayne_calibration;

int wayne_ctx_set_calibration(wayne_ctx *ctx, const wayne_calibration *c);

/* ---- outer boundary: one whole exposure -------------------------------- */

/*
 * Everything ExposureGenerator.scanning_frame / staring_frame
 * (exposure_generator.py:146-405) consumes for one exposure, as plain arrays.
 * The sample timing (A12), scan positions, jitter and SSV scaling are small
 * K-vectors prepared by the host (wayne_amd/exposure_generator.py); the
 * per-wavelength, per-electron and per-pixel work happens on the device:
 *   trace + counts chain   exposure_generator.py:581-634, grism.py:491-669, 779-803
 *   electron thrower       pyparallel_menu.c:10-113
 *   flat                   grism.py:349-409, exposure_generator.py:641-645
 *   per-read stage         exposure_generator.py:468-515, cosmic_rays.py:70-139
 *   post-ramp stage        exposure_generator.py:407-444, exposure.py:49-131,
 *                          detector.py:151-198, 318-350
 */
typedef struct wayne_exposure_desc {
  uint32_t seed;           /* visit seed (run_visit.py:68-77)                  */
  uint32_t exposure_index; /* extends every RNG counter                        */
  int rng_mode;            /* thrower RNG: WAYNE_RNG_*                         */
  int threads_compat;      /* replay mode only                                 */
  uint32_t flags;          /* WAYNE_F_*                                        */
  int sub_scale;           /* frame offset 507 - SUBARRAY/2 (exposure_generator.py:630) */

  int n_wl;                /* W: bins already cropped to grism.wl_limits       */
  const double *wl_um;     /* [W] increasing                                   */
  const double *flux;      /* [W] stellar flux                                 */
  const double *depth;     /* [K*W] transit depth per sub-sample, or NULL      */

  int n_samples;              /* K                                             */
  const double *x_ref;        /* [K] star x incl. jitter                       */
  const double *y_ref;        /* [K] star y incl. scan + jitter                */
  const double *dur_ms;       /* [K] sub-sample duration (after SSV)           */
  const int32_t *replay_seed; /* [K] s_rand_seeds (exposure_generator.py:327) */
  const int32_t *sample_read; /* [K] index 0..R-1 of the read that closes it   */

  int n_reads;              /* R                                               */
  const double *read_dt_s;  /* [R] interval since the previous read, seconds   */

  double sky_ct_s;     /* sky background counts/s; <= 0 disables               */
  double cosmic_rate;  /* hits/s per 1024^2; < 0 disables (None)               */
  double scale_factor; /* visit-trend scale (1 when None)                      */
  double noise_mean;   /* optional gaussian noise per second, both 0 disables  */
  double noise_std;

  int thrower_margin; /* LDS tile margin in px around the trace; 0 = default   */
  int thrower_splits; /* thrower workgroups launched per sub-sample (an upper bound: the kernel
                         shares the electrons it finds among as many as it needs); 0 = sized
                         from the host's estimate of the electron count           */

  /* Device light curves (replaces the W pylightcurve calls per exposure of
   * Observation.generate_lightcurves, observation.py:293-357).  When lc_z is
   * not NULL, `depth` must be NULL and the K x W transit-depth matrix is
   * computed on the device by k_lightcurve:
   *   depth[k][w] = (1 - transit(z_k, rp_w, ld)) + (1 - eclipse(rp_w^2, hidden_k))
   * A NaN rp_w (a negative element of the planet spectrum) is a planet of no size: depth[.][w] = 0,
   * and the bin takes no part in the range of radius ratios the kernel interpolates over.
   * Against the float64 law: 2e-8 for rp <= 0.2, growing in proportion to rp beyond (float32
   * integrand; DESIGN.md, k_lightcurve).                                                  */
  const double *lc_z;      /* [K] projected separation in stellar radii (>= 10: planet behind the star) */
  const double *lc_hidden; /* [K] fraction of the planet's disk hidden by the star (eclipse), or NULL   */
  const double *lc_rp;     /* [W] Rp/R* per bin = sqrt(planet_spectrum)                                  */
  double lc_ld[4];         /* Claret 4-coefficient limb darkening                                        */
} wayne_exposure_desc;

/* Stage an exposure's inputs in HBM slot `slot` (0 <= slot < wayne_ctx_slots). */
int wayne_ctx_slots(const wayne_ctx *ctx);
int wayne_exposure_upload(wayne_ctx *ctx, int slot, const wayne_exposure_desc *d);
/* Enqueue the whole synthesis of slot `slot` on the context stream
 * (asynchronous; inputs and outputs stay in HBM). */
int wayne_exposure_run(wayne_ctx *ctx, int slot);
/* wayne_exposure_run, then wait for the slot and settle it (see wayne_ctx_synchronize): when this returns WAYNE_OK the
 * slot's reads in HBM are complete.  The blocking form for callers that read wayne_exposure_device_reads directly. */
int wayne_exposure_run_checked(wayne_ctx *ctx, int slot);
/* The status word of the slot's last run (synchronises its stream): 0 = complete; bit 0 = a count overflowed (the
 * download / wait / synchronize calls report it as WAYNE_E_OVERFLOW); bit 1 = a bin held more electrons than the
 * launch sequence chosen from the host's estimate handles.  Every call that hands results over or ends a batch --
 * wayne_exposure_download / _wait / _run_checked / _debug_fetch and wayne_ctx_synchronize -- looks at the word itself
 * and runs such an exposure a second time with the general sequence; only a caller that waits on wayne_ctx_stream
 * with its own HIP calls bypasses that and must look here.  wayne_ctx_reruns: how many such second runs the context
 * has made (their electrons are counted twice in wayne_profile.electrons).  The word is that of the LAST run enqueued
 * on the slot: the library numbers a slot's runs and a flag raised by an earlier run does not show (nothing on the
 * device clears the block between runs, and no kernel runs in front of an exposure's k_prep_sub: the per-wavelength
 * arrays are worked out by wayne_exposure_upload / _set_sources and kept while the grid and the grism stay the same). */
int wayne_exposure_status(wayne_ctx *ctx, int slot, int *status);
unsigned long long wayne_ctx_reruns(const wayne_ctx *ctx);
/* Copy the NSAMP reads (read 0 = zero read) of `slot` to the host:
 * NSAMP*S*S float32, float64 when WAYNE_F_OUT_F64 was set, uint16 when WAYNE_F_OUT_U16 was.  Synchronises. */
int wayne_exposure_download(wayne_ctx *ctx, int slot, void *out_reads);
/* Pinned-host delivery for pipelines: wayne_exposure_fetch_async enqueues, on the
 * slot's stream (i.e. after its kernels), the copy of the reads into a pinned host
 * buffer owned by the library and returns at once; wayne_exposure_wait blocks until
 * that slot's work is done and returns the buffer (NSAMP*S*S float32 / float64 / uint16), which
 * stays valid until the slot is uploaded again.  With two slots on the two streams the
 * copy of one exposure overlaps the kernels of the next. */
int wayne_exposure_fetch_async(wayne_ctx *ctx, int slot);
int wayne_exposure_wait(wayne_ctx *ctx, int slot, void **host_reads);
/* Device pointer of that buffer (for zero-copy consumers). */
void *wayne_exposure_device_reads(wayne_ctx *ctx, int slot);
/* upload + run + download in one call: the batched drop-in for one
 * ExposureGenerator.scanning_frame call. */
int wayne_exposure_synthesize(wayne_ctx *ctx, const wayne_exposure_desc *d,
                              void *out_reads);

/* Intermediate products of the last run of `slot`, for parity tests
 * (any pointer may be NULL):
 *   counts  [K*W] int32  electrons per bin per sub-sample   (A9)
 *   x_pos   [K*W] double frame x of each bin                (A7, A10)
 *   y_pos   [K*W] double
 *   acc_e   [R*S*S] double  flat-weighted electrons accumulated per read
 *                    interval, before sky / gain (A11, A12); includes cosmic hits
 * `acc_e` is only meaningful between wayne_exposure_run_front and
 * wayne_exposure_run_back (the ramp kernel clears it). */
int wayne_exposure_debug_fetch(wayne_ctx *ctx, int slot, int32_t *counts,
                               double *x_pos, double *y_pos, double *acc_e);
/* The K*W transit-depth matrix of `slot` (as uploaded, or as computed by k_lightcurve
 * in the last run_front), for parity tests. */
int wayne_exposure_debug_depth(wayne_ctx *ctx, int slot, double *depth);
/* Which accumulators the ramp kernel of `slot` loads (for the byte accounting of bench.py): boxes[r*4 .. r*4+3] =
 * {x0, x1, y0, y1} of read interval r in bordered coordinates, the host's bound on where the thrower's electrons of
 * that interval can land (all zero: everything is loaded), and segments[r] = the number of 64-accumulator segments
 * (one per wave) that intersect it.  Segments with a cosmic-ray hit are loaded too and not counted here.  With
 * wayne_exposure_set_ipc the ramp kernel gets each non-empty box a pixel wider on every side, clamped to the frame
 * (coupled charge lies one pixel outside the thrower's bound): those are then the boxes reported and counted.
 * boxes: 16*4 ints, segments: 16 ints.  Returns WAYNE_OK, *use_box = 0 when the slot loads every accumulator. */
int wayne_exposure_debug_boxes(wayne_ctx *ctx, int slot, int32_t *boxes, int32_t *segments, int *use_box);
/* The two halves of wayne_exposure_run: front = prep + thrower + cosmic rays,
 * back = the fused up-the-ramp kernel. */
int wayne_exposure_run_front(wayne_ctx *ctx, int slot);
int wayne_exposure_run_back(wayne_ctx *ctx, int slot);
/* Which instantiation of the fused up-the-ramp kernel the back half of `slot` launches, written into buf (cap bytes,
 * NUL-terminated) in the form a kernel trace prints it, e.g. "k_ramp<float, true, 1, false, true>": <type of the reads,
 * production (hardware) math, sky sampler 0 direct / 1 alias tables / 2 tables + pieces, gaussian-noise stage, every
 * detector switch on>.  The arithmetic differs between them (float: exact integer sums + an all-float32 per-read
 * chain; double: fp64 cumulative sum; unsigned short: float's, quantised in the store), so a measurement names the one
 * it timed (bench.py `dtype`, `roofline.kernel`).
 * No reference counterpart: the reference has one float64 numpy path (exposure_generator.py:407-515). */
int wayne_exposure_ramp_variant(wayne_ctx *ctx, int slot, char *buf, int cap);

/* ---- contaminating field stars (no reference counterpart) --------------- */

/*
 * A second (third, ...) star whose first-order spectrum lands on the same exposure.  Its part of the exposure is
 * exactly the front half of the single-source exposure with x_ref + dx, y_ref + dy, its own wl_um / flux,
 * depth = NULL (contaminants do not transit), cosmic_rate < 0 and seed = wayne_source_seed(seed, tag); everything
 * else is the exposure's own.  Its electrons add into the same int64 accumulators as the target's; the stages that
 * belong to the exposure as a whole (sky, reads, noise, cosmic rays) run once, with the visit seed.
 * Not supported: zeroth / second orders, a contaminant in the direct image, a varying contaminant, per-sub-sample
 * offsets, WAYNE_RNG_REPLAY.
 */
typedef struct wayne_source_desc {
  uint32_t tag;          /* >= 1, unique within the exposure: selects the source's random streams */
  int n_wl;              /* 2 .. 32768 */
  const double *wl_um;   /* [W] */
  const double *flux;    /* [W] same units and scaling as wayne_exposure_desc.flux */
  double dx, dy;         /* detector-pixel offset from the target; added to x_ref[k] / y_ref[k] of every sub-sample */
} wayne_source_desc;

#define WAYNE_MAX_SOURCES 8 /* contaminants per exposure */

/* After wayne_exposure_upload, before run: extra sources of the slot's exposure (n = 0 clears).
 * wayne_exposure_upload clears the list, so callers that never call this get today's exposure.
 * WAYNE_E_INVALID (the slot stays usable, without contaminants) in replay mode, on a zero or duplicate tag, a
 * non-finite offset, n > WAYNE_MAX_SOURCES or a bad n_wl; WAYNE_E_STATE on a slot that is not uploaded. */
int wayne_exposure_set_sources(wayne_ctx *ctx, int slot, const wayne_source_desc *src, int n);
/* The visit seed a source's streams use: tag 0 -> seed; otherwise word 0 of
 * philox4x32_10(ctr = (tag, 0, 0, 0), key = (seed, STAGE_SOURCE)).  Pure host arithmetic. */
uint32_t wayne_source_seed(uint32_t seed, uint32_t tag);
/* debug_fetch for source i (0 = target, 1.. = list order): counts / x_pos / y_pos [K*W_i]. */
int wayne_exposure_debug_fetch_source(wayne_ctx *ctx, int slot, int source, int32_t *counts, double *x_pos,
                                      double *y_pos);

/* ---- charge trapping: the ramp effect per pixel (no reference counterpart) ---- */

/*
 * Two trap populations per pixel, p = 0 slow and 1 fast (the model of Zhou et al. 2017, AJ 153, 243): occupancy E_p
 * (e-) obeys dE/dt = eta f (1 - E/N) - E/tau for the pixel's collected-charge rate f (e-/s), stepped exactly read
 * interval by read interval on the device.  Read r shows what the pixel collected (its accumulators: thrower electrons
 * of every source and cosmic-ray hits, plus its sky draws; not the gaussian-noise stage) minus
 * (E_s + E_f)(r) - (E_s + E_f)(zero read).  Reference pixels are not trapped; nothing is drawn.
 * E_p at the zero read comes from start[p]: a table over the pixel's mean rate f_bar = (sum of its accumulators +
 * master sky x sum_r sky_ct_s read_dt[r]) / sum_r read_dt[r].  Point 0 is f = 0, points 1 .. n_rate-1 are log-spaced
 * from rate_lo to rate_hi; the device interpolates linearly in f below rate_lo, linearly in ln f above it, and clamps at
 * rate_hi.  The caller plans the table (wayne_amd/traps.py: the visit's history at f_bar), so exposures stay
 * independent of each other.
 */
typedef struct wayne_trap_desc {
  double n_traps[2];       /* capacity N_p (e-), > 0 */
  double efficiency[2];    /* trapping efficiency eta_p in [0, 1] */
  double lifetime_s[2];    /* lifetime tau_p (s), > 0 */
  int n_rate;              /* G: points of each start table, 2 .. WAYNE_MAX_TRAP_RATES */
  double rate_lo, rate_hi; /* e-/s, 0 < rate_lo < rate_hi (rate_lo <= rate_hi when G = 2) */
  const double *start[2];  /* [G] each: E_p at the zero read, every entry in [0, n_traps[p]] */
} wayne_trap_desc;

#define WAYNE_MAX_TRAP_RATES 4096

/* After wayne_exposure_upload, before run: trap the slot's exposure (t = NULL clears; upload clears too, so callers
 * that never call this get today's exposure).  The table is staged in the slot.  WAYNE_E_INVALID (the slot stays usable,
 * without traps) in replay mode, on non-finite values, n_traps <= 0, efficiency outside [0, 1], lifetime <= 0, n_rate
 * outside 2 .. WAYNE_MAX_TRAP_RATES, bad rates or a table entry outside [0, n_traps]; WAYNE_E_STATE on a slot that is
 * not uploaded.  The back half then launches k_ramp_trap<...> (wayne_exposure_ramp_variant names it). */
int wayne_exposure_set_traps(wayne_ctx *ctx, int slot, const wayne_trap_desc *t);

/* ---- a carried trap history: each pixel's trap state from exposure to exposure ----
 * (opt-in; without these calls every launch and every byte stay as they are.  Added within WAYNE_ABI_VERSION 7: new
 * symbols and a new struct only.)
 *
 * A context owns one trap state: [S*S][2] float32 in bordered coordinates, [pixel][0] slow and [pixel][1] fast.  A slot
 * with traps AND a history descriptor does not look at its start table: for every light-sensitive pixel and population p
 *     E_p <- state[pixel][p]
 *     E_p <- the exact step of E_p over gap_s seconds at rate (lit ? f_bar : 0)      (gap_s = 0 leaves E_p as it is)
 *     E_p <- min(E_p + fill[p], N_p)
 *     ... the read intervals as wayne_exposure_set_traps describes them, E_p(zero read) = the value above ...
 *     state[pixel][p] <- E_p after the last read, rounded to float32
 * (f_bar: the pixel's mean rate of THIS exposure, as above; float32 arithmetic in the production chain, float64 in the
 * others).  Reference pixels are neither read nor written.  The back half launches k_ramp_hist<...> with
 * k_ramp_trap's template list (wayne_exposure_ramp_variant names it).  The state belongs to the back half:
 * wayne_exposure_run_front does not touch it.
 *
 * Order: exposures run in the order of their wayne_exposure_run / _run_back calls, whatever their slots -- each
 * k_ramp_hist waits for the one enqueued before it (an event between the two streams); the front kernels of an exposure
 * still overlap the previous exposure.
 * Every run advances the state: wayne_exposure_run twice on such a slot steps the traps through the exposure twice.  For
 * the same reason the library never runs such an exposure a second time by itself: its slot is launched with the general
 * kernel sequence from the start (as a slot whose first run met a bin beyond the lanes' reach is on its second), so
 * status bit 1 is never raised.  The cost is the k_throw launch that finds nothing to do (~8 us) on configurations that
 * otherwise go without it.
 */
typedef struct wayne_trap_history_desc {
  double gap_s;            /* seconds since the previous exposure's last read, finite and >= 0 */
  int lit;                 /* != 0: the pixel collected at f_bar during the gap (staring); 0: a dark gap (a scan, an orbit's gap) */
  double fill[2];          /* added after the gap, in [0, n_traps[p]] (an orbit's start); the sum is clipped to n_traps[p] */
} wayne_trap_history_desc;

/* The trap state.  reset: every pixel := (initial[0], initial[1]), finite and >= 0 (allocated on first use).  upload /
 * download: the whole state, [S*S*2] float32.  Rare calls: each brings every stream to rest before and after.
 * WAYNE_E_STATE without calibration (S is not known), and for download before any reset or upload.  A calibration of
 * another frame size discards the state. */
int wayne_ctx_trap_state_reset(wayne_ctx *ctx, const double initial[2]);
int wayne_ctx_trap_state_upload(wayne_ctx *ctx, const float *state);
int wayne_ctx_trap_state_download(wayne_ctx *ctx, float *state);

/* After wayne_exposure_set_traps, before run: the slot's exposure carries the state (h = NULL clears; upload and
 * set_traps clear too).  WAYNE_E_INVALID (the slot stays usable, without a history: a plain k_ramp_trap exposure) on a
 * non-finite or negative gap or a fill outside [0, n_traps]; WAYNE_E_STATE without traps on the slot, before any
 * wayne_ctx_trap_state_reset / _upload, or between wayne_exposure_run_front and _run_back (the front half chooses the
 * launch sequence). */
int wayne_exposure_set_trap_history(wayne_ctx *ctx, int slot, const wayne_trap_history_desc *h);

/* ---- device-side spectral extraction (no reference counterpart) ---------- */

/*
 * Column spectra of the slot's exposure, formed on the device from the reads k_ramp has just written and the context's
 * calibration planes: what a light-curve consumer keeps of an exposure (~120 KB) instead of its reads (67 MB).
 * All coordinates bordered, side S; float64 throughout (a read of any stored type is promoted exactly); an absent
 * calibration plane counts as 0 (c1..c4, dark, master sky) or as a gain of 2.35 (pixel flat):
 *   D_r = P_r - P_0,  L_r = D_r (1 + c1 + D_r (c2 + D_r (c3 + c4 D_r))) - dark_r,  L_0 = 0
 *   I_r = (L_r - L_{r-1}) g,  g = 2.35 / pfl as a float64 divide (2.35 on the 5-px border),  T = master sky (0 on the border)
 *   product j = 0 .. R-1 (read interval j), rows [row_lo[j], row_hi[j]):  A_j[x] = sum_y I_{j+1}[y,x],  B_j[x] = read_dt_s[j] sum_y T[y,x]
 *   product R (the last read alone), rows [row_lo[R], row_hi[R]):       A_R[x] = sum_y L_R[y,x] g,   B_R[x] = (sum_j read_dt_s[j]) sum_y T[y,x]
 *   sky_j = sum_{x in [bg_col_lo, bg_col_hi)} A_j[x] / sum_{x in [bg_col_lo, bg_col_hi)} B_j[x]   (0 when the denominator is 0)
 *   spectra_j[x] = A_j[x] - sky_j B_j[x],  x = 0 .. S-1
 * Result: spectra [(R+1)*S] and sky [R+1], float64.  The sums are taken in an order fixed by the plan (chunks of 32
 * rows of a window, added in ascending order; no atomics): the same exposure gives the same bytes in any slot, on
 * either stream, in any process.  Cosmic-ray rejection and wavelength-binned channels are opt-in (below); fits stay
 * with the caller.
 */
#define WAYNE_X_LINEARISE (1u << 0) /* off: L_r = D_r - dark_r */
#define WAYNE_X_DARK (1u << 1)      /* off: dark_r = 0 */
#define WAYNE_X_GAIN (1u << 2)      /* off: g = 1, the result is in DN */
#define WAYNE_X_SKY (1u << 3)       /* off: sky_j = 0, spectra_j = A_j */
#define WAYNE_X_LAST_READ (1u << 4) /* off: product R is not formed (zeros); its window is ignored */
#define WAYNE_X_ALL 31u

typedef struct wayne_extract_desc {
  uint32_t steps;   /* WAYNE_X_* */
  int row_lo[17];   /* product j at index j, the last-read product at index R (= n_reads); the rest is ignored */
  int row_hi[17];
  int bg_col_lo;    /* columns the sky level is fitted on */
  int bg_col_hi;
} wayne_extract_desc;

/* After wayne_exposure_upload, before run: extract the slot's exposure (x = NULL clears; upload clears too, so callers
 * that never call this get today's exposure and today's launches).  WAYNE_E_INVALID (the slot stays usable, without
 * extraction) when a window or the background range is not within 0 <= lo < hi <= S or `steps` has unknown bits;
 * WAYNE_E_STATE on a slot that is not uploaded.  The back half of wayne_exposure_run then enqueues the extraction
 * behind the ramp kernel on the slot's stream, so every call that runs an exposure a second time re-extracts it. */
int wayne_exposure_set_extraction(wayne_ctx *ctx, int slot, const wayne_extract_desc *x);
/* The counterparts of wayne_exposure_fetch_async / _wait for the spectra: only the spectra block and the slot's status
 * block are copied to pinned memory, never the reads.  *spectra [(R+1)*S] and *sky [R+1] stay valid until the slot is
 * uploaded again.  The status word is handled as in wayne_exposure_wait (a bin beyond the lanes' reach: run again,
 * fetch again, look again).  WAYNE_E_STATE when no extraction is set.  wayne_exposure_fetch_async / _wait / _download
 * keep delivering the reads of the same slot. */
int wayne_exposure_fetch_spectra_async(wayne_ctx *ctx, int slot);
int wayne_exposure_wait_spectra(wayne_ctx *ctx, int slot, double **spectra, double **sky);
/* The blocking form: spectra [(R+1)*S] and sky [R+1] into the caller's arrays.  Synchronises. */
int wayne_exposure_download_spectra(wayne_ctx *ctx, int slot, double *spectra, double *sky);
/* The spectra block -- what one copy brings to pinned memory, and where the accessors below point into it -- holds, one
 * behind the other, float64 unless noted:
 *   spectra [(R+1)*S], sky [R+1]
 *   with rejection       n_rejected [R+1] (uint32); whatever follows begins on the next multiple of 8 bytes
 *   with channels        channels [(R+1)*C]
 *   with variances       spectra_var [(R+1)*S], sky_var [R+1] and, with channels, channels_var [(R+1)*C]
 *   with set_optimal     optimal [(R+1)*S], optimal_var [(R+1)*S] and, with the optimal channels, channels_opt and
 *                        channels_opt_var [(R+1)*C each]
 * Every setter of the extraction's options changes the layout: what was fetched before it is gone (WAYNE_E_STATE from
 * the accessors until the next wait_spectra / download_spectra). */
/*
 * Cosmic-ray rejection on the extraction's difference images (opt-in; without it nothing above changes).  I_r and g are
 * the extraction law's.  For read interval j = 0 .. R-1 let I = I_{j+1}.  A pixel (y, x) is TESTED iff 7 <= y < S-7,
 * 7 <= x < S-7 and y lies in the mask rows [min_p row_lo[p], max_p row_hi[p]) over the products that are formed:
 *   m8 = max of the eight stencil pixels I[y+-1,x], I[y+-2,x], I[y,x+-1], I[y,x+-2]
 *   d  = I[y,x] - m8
 *   flag_j[y,x]  <=>  d > 0  and  d d > k^2 (rn^2 + max(m8, 0))        (no square root, no division)
 *   repl_j[y,x]  =  0.5 (b + c),  b <= c the middle two of I[y,x-2], I[y,x-1], I[y,x+1], I[y,x+2]   (the same row)
 * A flag is a strict local maximum over the plus-shaped stencil by k sigma of a Poisson + read-noise model in electrons
 * (hence WAYNE_X_GAIN); the replacement is taken along the dispersion, never along the scan.
 *   product j < R:  A_j[x] sums  flag_j ? repl_j : I_{j+1}  over its window
 *   product R:      A_R[x] sums  L_R g - sum_j flag_j (I_{j+1} - repl_j)
 * B, the sky level and the spectra follow as above (the background columns are cleaned too).  n_rejected[p] is the
 * number of flags in product p's window; for p = R it counts (pixel, interval) pairs.  Defaults of the Python layer:
 * k = 8, read_noise_e = 20 (sqrt(2) x 14.1 e-, the noise of a difference of two reads as the ramp kernel adds it).
 * Not covered: hits on adjacent pixels of one interval (they shield each other) and the 7-pixel frame margin.
 */
typedef struct wayne_crrej_desc {
  double k;            /* threshold in sigma: finite, > 0 */
  double read_noise_e; /* rn (e-): finite, >= 0 */
} wayne_crrej_desc;

/* After wayne_exposure_set_extraction, before run: reject cosmic rays in the slot's extraction (r = NULL clears; upload
 * and set_extraction clear it too).  WAYNE_E_STATE when no extraction is set on the slot; WAYNE_E_INVALID (the slot stays
 * usable, extracting without rejection) for a bad k or read_noise_e or when WAYNE_X_GAIN is off. */
int wayne_exposure_set_crrej(wayne_ctx *ctx, int slot, const wayne_crrej_desc *r);
/* After wayne_exposure_wait_spectra / _download_spectra of a slot with rejection: *n_rejected [R+1], valid until the
 * slot's spectra are fetched or the slot is uploaded again.  WAYNE_E_STATE before any fetch or without rejection. */
int wayne_exposure_rejected(wayne_ctx *ctx, int slot, const uint32_t **n_rejected);
/* The flag plane of the slot's last run, blocking: mask [S*S], bit j = flag_j, 0 outside the mask rows. */
int wayne_exposure_download_crmask(wayne_ctx *ctx, int slot, uint16_t *mask);
/*
 * Wavelength-binned channel fluxes of the extraction, flat-fielded (opt-in; without it nothing above changes).  Added
 * within WAYNE_ABI_VERSION 7: new symbols and a new struct only, so a caller built against the earlier header runs
 * unchanged.  Conventions as above: bordered coordinates, side S, float64 throughout.  C channels with edges
 * e[0] < ... < e[C] (um); per bordered row y the wavelength at bordered column coordinate u (pixel x covers [x, x+1)) is
 *   lambda_y(u) = wl_a[y] + wl_b[y] u   (um)
 * For product p and pixel (y, x) of its window let v be the term A_p[x] sums for that pixel (I_{p+1}, or its cleaned
 * value under wayne_exposure_set_crrej; for p = R: L_R g minus the rejection's corrections), t = T[y, x] (0 on the
 * border, when the plane is absent or WAYNE_X_SKY is off), scale_p = read_dt_s[p] (sum_j read_dt_s[j] for p = R) and
 * sky_p the level of the column extraction, unchanged and not flat-fielded:
 *   ua_b(y)  = (e[b] - wl_a[y]) / wl_b[y]                         (one float64 subtract, one divide)
 *   w_b(y,x) = min(max(min(x+1, ua_{b+1}) - max(x, ua_b), 0), 1)
 *   F(y,x)   = 1, unless WAYNE_C_FLAT is set, the context holds a flat cube and (y, x) is not a border pixel; then, with
 *              tau = (1e4 (wl_a[y] + wl_b[y] x) - flat_wmin) / (flat_wmax - flat_wmin)  (lambda at the pixel's integer
 *              coordinate, as the thrower's flat evaluates it), F = (double)(float)(f0 + f1 tau + f2 tau^2 + f3 tau^3) on
 *              frame pixel (y-5, x-5), tau^2 = tau tau, tau^3 = tau^2 tau, the terms added left to right; F := 1 where
 *              that is not > 0
 *   P_p[b] = sum_y sum_x w_b(y,x) (v / F)        Q_p[b] = scale_p sum_y sum_x w_b(y,x) (t / F)
 *   channels_p[b] = P_p[b] - sky_p Q_p[b]        p = 0 .. R   (zeros for p = R when WAYNE_X_LAST_READ is off)
 * Result: channels [(R+1)*C], float64.  Every sum is taken in an order fixed by the plan (a row's columns ascending, then
 * the 8 rows of a group, the 4 groups of a 32-row chunk and the chunks of a window, each ascending; no atomics): the same exposure gives the same
 * bytes in any slot, on either stream, after a second run and in any process.  The work falls on the column hull
 * [min_y floor(ua_0(y)), max_y ceil(ua_C(y))) over the rows of the formed windows, clamped to [0, S].
 * Not covered: optimal extraction, resampling in y, other grism orders, the direct image, a flat-fielded sky fit.
 */
#define WAYNE_C_FLAT (1u << 0)   /* divide by the flat cube at the pixel's wavelength */
#define WAYNE_MAX_CHANNELS 256
#define WAYNE_MAX_CHANNEL_HULL 384 /* widest column hull a plan may have */

typedef struct wayne_channels_desc {
  int n_channels;         /* C: 1 .. WAYNE_MAX_CHANNELS */
  const double *edges_um; /* [C + 1], finite and increasing */
  const double *wl_a;     /* [S] um; finite on every row of a formed window */
  const double *wl_b;     /* [S] um / px; finite and > 0 on every row of a formed window */
  uint32_t flags;         /* WAYNE_C_* */
} wayne_channels_desc;

/* After wayne_exposure_set_extraction, before run: bin the slot's extraction into channels (d = NULL clears; upload and
 * set_extraction clear it too, set_crrej does not).  The arrays are copied before the call returns.  WAYNE_E_STATE when no
 * extraction is set on the slot; WAYNE_E_INVALID (the slot stays usable, extracting without channels) for n_channels
 * outside 1 .. 256, non-finite or non-increasing edges, a bad wl_a / wl_b on a row of a formed window, unknown flag bits
 * or a hull wider than WAYNE_MAX_CHANNEL_HULL.  The channels ride in the same copy as the spectra
 * (wayne_exposure_fetch_spectra_async / _wait_spectra / _download_spectra). */
int wayne_exposure_set_channels(wayne_ctx *ctx, int slot, const wayne_channels_desc *d);
/* After wayne_exposure_wait_spectra / _download_spectra of a slot with channels: *channels [(R+1)*C], valid until the
 * slot's spectra are fetched or the slot is uploaded again.  WAYNE_E_STATE before any fetch or without channels. */
int wayne_exposure_channels(wayne_ctx *ctx, int slot, const double **channels);
/*
 * Variances of the spectra, the sky levels and the channels (opt-in; without it nothing above changes: every launch and
 * every byte of the spectra block stay as they are).  Added within WAYNE_ABI_VERSION 7: new symbols and a new struct only.
 * Float64 throughout.  For product p and pixel (y, x) of its window let v be the term A_p[x] sums for that pixel (as
 * for the channels above), g the extraction's gain factor, q = g / 2.35 (1 / pfl; 1 on the border) and rn = read_noise,
 * the noise of a difference of two reads in electrons -- every product is one (wayne_crrej_desc.read_noise_e has the
 * same meaning and the same default, 20):
 *   var_p(y,x)        = max(v, 0) + rn^2 (q q)
 *   VA_p[x]           = sum_{y in window p} var_p(y,x)
 *   sky_var_p         = sum_{x in bg} VA_p[x] / (sum_{x in bg} B_p[x])^2       (0 where sky_p is 0 by its rule)
 *   spectra_var_p[x]  = VA_p[x] + (B_p[x] B_p[x]) sky_var_p
 *   VP_p[b]           = sum_y sum_x (w_b w_b) (var_p(y,x) / (F F))
 *   channels_var_p[b] = VP_p[b] + (Q_p[b] Q_p[b]) sky_var_p
 * with w_b, F, B_p, Q_p, the windows, the hull and the background columns of the laws above.  Zeros for p = R when
 * WAYNE_X_LAST_READ is off; sky_var = 0 when WAYNE_X_SKY is off.  The sums follow the order of the flux sums (no
 * atomics): the same exposure gives the same bytes in any slot, on either stream, after a second run.  No plane is read a
 * second time: a pixel's variance is formed beside its flux.
 * Left out: the covariance between a background column's own flux and the sky level (such a column's variance counts
 * its own pixels twice, once through sky_var_p); the correlation between neighbouring channels that share a pixel, and
 * through the common sky level; the correlation of read intervals through the read they share -- in a sum over
 * consecutive intervals the Poisson parts add, but the read noise is that of the first and the last read alone, i.e. of
 * the last-read product over the same rows, not R times it; the variance of a rejected pixel's replacement, which is
 * taken from the replacement's own value as if it were a measured pixel.
 */
typedef struct wayne_variance_desc {
  double read_noise; /* rn (e-) of a difference of two reads: finite, >= 0 */
} wayne_variance_desc;

/* After wayne_exposure_set_extraction, before run: deliver variances with the slot's extraction (v = NULL clears; upload
 * and set_extraction clear it too, set_crrej and set_channels do not -- with channels, before or after, channels_var is
 * delivered too).  WAYNE_E_STATE when no extraction is set on the slot; WAYNE_E_INVALID (the slot stays usable,
 * extracting without variances) for a negative or non-finite read_noise or when WAYNE_X_GAIN is off: a variance is in
 * electrons^2.  The variances ride in the same copy as the spectra, behind the channels. */
int wayne_exposure_set_variance(wayne_ctx *ctx, int slot, const wayne_variance_desc *v);
/* After wayne_exposure_wait_spectra / _download_spectra of a slot with variances: *spectra_var [(R+1)*S], *sky_var [R+1]
 * and *channels_var [(R+1)*C] (NULL without channels), valid until the slot's spectra are fetched or the slot is uploaded
 * again.  WAYNE_E_STATE before any fetch or without variances. */
int wayne_exposure_variances(wayne_ctx *ctx, int slot, const double **spectra_var, const double **sky_var,
                             const double **channels_var);
/*
 * Optimal (profile-weighted) extraction of the column spectra, on top of the variances (opt-in; without it nothing above
 * changes: every launch and every byte of the spectra block stay as they are).  Added within WAYNE_ABI_VERSION 7: new
 * symbols and a new struct only.  The box extraction above sums every row of a product's window, margin rows that hold
 * only read noise and sky included; this one weighs a pixel by the share of the column's light it is expected to hold.
 * Float64 throughout, bordered coordinates.  For product p with window [lo_p, hi_p), v the term A_p[x] sums for a pixel
 * (cleaned under rejection), t its master sky, bt = scale_p t (scale_p = dt_p; the sum of all dt for p = R), g the gain
 * factor, q = g / 2.35, rn the read noise of the slot's wayne_variance_desc, H = half_width and sky_p, spectra_p,
 * spectra_var_p, sky_var_p the values delivered above:
 *   d(y,x)  = v - sky_p bt                    X(x) = [max(x - H, 0), min(x + H, S - 1)]
 *   S1(y,x) = sum_{x' in X(x), ascending} d(y,x')
 *   S0(x)   = sum_{x' in X(x), ascending} spectra_p[x']       SV0(x) = the same sum of spectra_var_p
 *   ok(x)  <=> S0 > 0 and S0 S0 > 9 SV0       (the source is detected at 3 sigma over the 2H + 1 columns)
 *   Pr = S1 / S0,  P = max(Pr, 0)             (sum_y S1 = S0 by construction: Pr sums to 1 over the window)
 *   V(y,x)  = max(spectra_p[x] Pr + sky_p bt, 0) + rn^2 (q q)
 *   U_p[x]  = sum_y (P d) / V     W_p[x] = sum_y (P P) / V     G_p[x] = sum_y (P bt) / V
 *   optimal_p[x]     = ok and W > 0 ? U / W                         : spectra_p[x]
 *   optimal_var_p[x] = ok and W > 0 ? 1 / W + (G/W)(G/W) sky_var_p  : spectra_var_p[x]
 * Zeros for p = R when WAYNE_X_LAST_READ is off.  A column without a detected source keeps the box values to the bit.
 * Two choices, measured on an ensemble of 48 simulated exposures: V is the variance of the model, not of the pixel's own v
 * (a data variance weighs downward fluctuations up: -0.09 % on the mean flux); P is clamped at 0 but not renormalised to
 * sum 1 (that division turns the positive noise of dark margin rows into flux: +0.16 % on the last read, +9.5 % on a
 * nearly unlit interval, against +0.05 % and +0.16 % without it).  The sums have a fixed order (no atomics): the same
 * exposure gives the same bytes in any slot, on either stream, after a second run.
 * Limits: the profile's own noise is not in 1 / W -- on a nearly unlit read interval the ensemble variance was 1.64 times
 * optimal_var; the read intervals are correlated through the reads they share, as for spectra_var; with read_noise = 0
 * a pixel whose model is <= 0 has V = 0, and its column then falls back to the box values.
 * Optimal wavelength-binned channels and a profile supplied by the caller: below (wayne_exposure_set_optimal_channels,
 * wayne_exposure_set_optimal_profile).  Not covered: a profile from a PSF model or a polynomial fit along the dispersion; iterating the profile; rejecting on the optimal
 * residuals; the direct image.
 */
#define WAYNE_MAX_OPTIMAL_HALF_WIDTH 16
typedef struct wayne_optimal_desc {
  int half_width; /* H: 1 .. WAYNE_MAX_OPTIMAL_HALF_WIDTH columns on either side of a column form its profile */
} wayne_optimal_desc;

/* After wayne_exposure_set_variance, before run: deliver optimal and optimal_var with the slot's extraction (d = NULL
 * clears; whatever clears the variances -- upload, set_extraction, set_variance -- clears it too, set_crrej and
 * set_channels do not).  WAYNE_E_STATE when no variances are set on the slot; WAYNE_E_INVALID (the slot stays usable,
 * extracting with variances) for a half_width outside 1 .. WAYNE_MAX_OPTIMAL_HALF_WIDTH.  The two arrays ride in the same
 * copy as the spectra, behind the variances. */
int wayne_exposure_set_optimal(wayne_ctx *ctx, int slot, const wayne_optimal_desc *d);
/* After wayne_exposure_wait_spectra / _download_spectra of a slot with the optimal extraction: *optimal and *optimal_var
 * [(R+1)*S each], valid until the slot's spectra are fetched or the slot is uploaded again.  WAYNE_E_STATE before any
 * fetch or without wayne_exposure_set_optimal. */
int wayne_exposure_optimal(wayne_ctx *ctx, int slot, const double **optimal, const double **optimal_var);
/*
 * Profile planes, and the optimal extraction with a profile the caller supplies (opt-in on top of
 * wayne_exposure_set_optimal; without them nothing above changes.  Added within WAYNE_ABI_VERSION 7: new symbols only).
 * The profile S1 / S0 above is formed from the exposure's own light, so its noise enters the weights: a pipeline that
 * forms ONE profile per visit from several exposures and extracts every exposure with it has weights that do not depend
 * on the exposure's own noise.  With --spectra-only the reads never leave the device, so the profile's raw material is
 * formed there too.
 * Layout of both (float64): the windows of all R + 1 products one behind the other, rows relative to the window --
 *   element off_p + (y - lo_p) S + x,   off_p = sum_{p' < p} (hi_p' - lo_p') S.
 * Delivery: planes[...] = S1(y,x) of the law above, the same left-to-right sum; zeros for p = R when WAYNE_X_LAST_READ is
 * off (that window then counts with min(max(hi - lo, 0), S) rows).  It is S1 and not S1 / S0: the caller adds the planes of
 * several exposures and normalises the sum -- a flux-weighted mean, and no division by a noisy S0.
 * Supplied profile Pi: the law above with Pr := Pi(y,x); d, bt, q, rn, S0, SV0 and the box values are as above --
 *   P = max(Pi, 0)     V = max(spectra_p[x] Pi + sky_p bt, 0) + rn^2 (q q)
 *   U, W, G, ok(x), optimal_p and optimal_var_p as above (H enters through ok(x) alone; a column whose profile is 0 on
 *   every row has W = 0 and keeps the box values to the bit).  The row sums are taken in the order of the law above.
 * Limits: the profile is fixed on the detector -- a star that drifts by a fraction of a pixel between the profile's
 * exposures and the extracted one, and a forward scan extracted with a reverse scan's profile, are weighted by a shifted
 * profile (biased low where the profile is steep); a nearly unlit read interval has a profile of noise; the read intervals
 * are correlated through the reads they share.
 */
/* After wayne_exposure_set_optimal, before run: every run of the slot also writes the profile planes (on = 0 clears; whatever
 * clears the optimal extraction -- upload, set_extraction, set_variance, set_optimal -- clears it too).  WAYNE_E_STATE
 * without wayne_exposure_set_optimal. */
int wayne_exposure_deliver_profile(wayne_ctx *ctx, int slot, int on);
/* After wayne_exposure_set_optimal, before run: extract with `profile` (copied before the call returns; NULL clears, back to
 * the exposure's own profile; cleared by what clears the optimal extraction), laid out for windows of rows[0 .. R] rows.
 * WAYNE_E_STATE without wayne_exposure_set_optimal; WAYNE_E_INVALID for a height outside 1 .. S (0 .. S for the last read).
 * A run of a slot whose windows have other heights than rows[] returns WAYNE_E_INVALID and enqueues nothing; the slot stays
 * usable (set another profile or clear it). */
int wayne_exposure_set_optimal_profile(wayne_ctx *ctx, int slot, const double *profile, const int *rows);
/* The same, for a caller that hands a slot the same profile again and again (a visit does, with every exposure it uploads
 * there): `tag` != 0 identifies the CONTENT of `profile`.  The slot keeps its device copy across whatever clears the option,
 * and a call with the tag, the heights and the length of the profile it holds copies nothing, does not wait for the slot's
 * stream and does not read `profile`.  Equal tags are taken as equal content: a caller that reuses a tag for other values
 * extracts with the old ones.  tag = 0: always copied (wayne_exposure_set_optimal_profile). */
int wayne_exposure_set_optimal_profile_tagged(wayne_ctx *ctx, int slot, const double *profile, const int *rows, uint64_t tag);
/* Profiles the two calls above have copied to the device since the context was created. */
unsigned long long wayne_ctx_profile_uploads(const wayne_ctx *ctx);
/* After wayne_exposure_set_channels AND wayne_exposure_set_optimal (and a supplied profile, if any), before run: the
 * optimal channels (on = 0 clears; whatever clears the optimal extraction clears them, and so does set_channels).  With
 * w_b and F exactly those of the channels' law, d, bt, P, V, q, rn of the optimal law (either profile source), W_p[x] the
 * ascending chunk sum wayne_exposure_optimal's values were formed from and ok(x) its rule:
 *   e  = ok(x) ? ((P d) / V) / W_p[x] : d           k = ok(x) ? ((P bt) / V) / W_p[x] : bt
 *   ev = ok(x) ? ((P P) / V) / W_p[x]^2 : max(v, 0) + rn^2 q^2
 *   channels_opt_p[b]     = sum_y sum_x w_b e / F          K_p[b] = sum_y sum_x w_b k / F
 *   channels_opt_var_p[b] = sum_y sum_x w_b^2 ev / F^2 + K_p[b]^2 sky_var_p
 * both (R+1)*C, behind optimal_var in the spectra's copy; zeros for p = R when WAYNE_X_LAST_READ is off.  With edges on
 * whole columns, one solution for all rows and the flat off, channels_opt is `optimal` summed over a channel's columns and
 * channels_opt_var sum 1 / W plus the sky level's share taken ONCE for the channel -- where summing optimal_var is wrong.
 * With the exposure's own profile the profile's noise is common to a channel's columns and channels_opt_var is too small
 * (measured: README); it is meant for a supplied profile.  WAYNE_E_STATE without channels or the optimal extraction. */
int wayne_exposure_set_optimal_channels(wayne_ctx *ctx, int slot, int on);
/* After wayne_exposure_wait_spectra / _download_spectra of such a slot: *channels_opt and *channels_opt_var [(R+1)*C each],
 * valid as long as wayne_exposure_optimal's arrays.  WAYNE_E_STATE before any fetch or without the option. */
int wayne_exposure_optimal_channels(wayne_ctx *ctx, int slot, const double **channels_opt, const double **channels_opt_var);
/* After a run of a slot with profile delivery AND wayne_exposure_wait_spectra / _download_spectra of it (they settle the
 * run): enqueue the copy of the planes into pinned host memory -- a copy of its own, not part of the spectra's (tens of MB
 * on a full frame, wanted for a handful of exposures per visit).  Returns at once.  WAYNE_E_STATE otherwise. */
int wayne_exposure_fetch_profile(wayne_ctx *ctx, int slot);
/* Waits for wayne_exposure_fetch_profile's copy: *planes (valid until the next fetch_profile or upload of the slot) and
 * *count, its doubles.  WAYNE_E_STATE without a fetch. */
int wayne_exposure_profile(wayne_ctx *ctx, int slot, const double **planes, size_t *count);
/* HIP-event time of the extraction's kernels (the channels', the variances' and the optimal extraction's included) while wayne_profile_enable is on, since
 * wayne_profile_reset: launches (one per extracted exposure) and total milliseconds.  wayne_profile_select's bit 8
 * selects it.  Synchronises. */
int wayne_extract_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- device-side FITS words (no reference counterpart) ------------------- */

/*
 * The reads of an exposure as the data sections of its HST-style file, formed on the device (k_fits_words) and fetched
 * into pinned host memory, from which a file is written without a pass over the samples on the host.  For the slot's
 * reads P_0 .. P_R (each S*S samples of type T, bordered) the payload is (R + 1) * stride bytes:
 *
 *   payload[f*stride + i*B ...]                       = words(P_{R-f} flat [i])   f = 0 .. R: the last read first, the
 *                                                                                  order of the file's SCI images
 *   payload[f*stride + plane_bytes .. (f + 1)*stride) = 0                          the HDU's padding
 *   words(v):  float32 reads: the 8 bytes of (double)v, most significant first (BITPIX -64)
 *              float64 reads: the 8 bytes of v, most significant first          (BITPIX -64)
 *              uint16 reads : the 2 bytes of v ^ 0x8000, most significant first (BITPIX 16 with BZERO 32768)
 *   B = 8, 8, 2;  plane_bytes = S*S*B;  stride = plane_bytes rounded up to a multiple of 2880 (a multiple of 64)
 *
 * so plane f is one contiguous piece of a file: a data section with its padding.  The bit patterns of NaN reads are not
 * specified (the reads are clipped and finite).  Opt-in: without wayne_exposure_set_fits every launch and every byte stay
 * as they are.  Added within WAYNE_ABI_VERSION 7: new symbols only.
 */

/* The layout for bordered side S, R reads behind the zero read and the sample type of descriptor flags `out_flags`
 * (WAYNE_F_OUT_F64, WAYNE_F_OUT_U16 or neither; other bits are ignored): *plane_bytes, *stride, *bitpix (-64 or 16).
 * Any output pointer may be NULL.  Pure host arithmetic, callable without a device.  WAYNE_E_INVALID for S < 2, an odd
 * S, R < 1 or both type flags. */
int wayne_fits_layout(int S, int R, uint32_t out_flags, size_t *plane_bytes, size_t *stride, int *bitpix);
/* After wayne_exposure_upload, before run: the back half of every run of the slot also forms the payload, behind the
 * ramp kernel and the extraction's launches on the slot's stream (on = 0 clears).  wayne_exposure_upload clears it, so a
 * caller that never calls this gets today's exposure and today's launches.  WAYNE_E_STATE on a slot that is not uploaded. */
int wayne_exposure_set_fits(wayne_ctx *ctx, int slot, int on);
/* Pinned-host delivery of the payload, shaped like wayne_exposure_fetch_async / _wait: fetch enqueues the copy into a
 * pinned mirror of its own behind the slot's kernels and returns at once; wait blocks until the slot's work is done and
 * returns the mirror, (R + 1) * stride bytes, valid until the next fetch_fits_async or upload of the slot.  The status word rides behind
 * the payload: an exposure that met a bin beyond its launch sequence's reach is run a second time and fetched again
 * (spectra fetched beside it too), as wayne_exposure_wait does.  The reads themselves need not be fetched.
 * WAYNE_E_STATE on a slot without wayne_exposure_set_fits. */
int wayne_exposure_fetch_fits_async(wayne_ctx *ctx, int slot);
int wayne_exposure_wait_fits(wayne_ctx *ctx, int slot, void **host_payload);
/* The payload into the caller's (pageable) memory, (R + 1) * stride bytes.  Synchronises; for tests. */
int wayne_exposure_download_fits(wayne_ctx *ctx, int slot, void *out_payload);
/* HIP-event time of k_fits_words while wayne_profile_enable is on, since wayne_profile_reset: launches and total
 * milliseconds.  wayne_profile_select's bit 9 selects it.  Synchronises. */
int wayne_fits_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- the noise-free expected image (no reference counterpart) ------------- */

/*
 * The exposure without its noise: what the Monte-Carlo throwers converge to, rendered by a kernel of its own (k_expect)
 * beside the exposure.  Turning every noise flag off does not give it: the thrower still throws every electron at
 * random.  The law, in float64: a thrower keeps an electron of a bin at c iff 0 < floor(c + sigma z) < N on both axes,
 * so with Phi the standard normal CDF
 *
 *   a(p; c, sigma) = Phi((p + 1 - c) / sigma) - Phi((p - c) / sigma)   for 1 <= p <= N - 1, else 0
 *   E_r[y + 5, x + 5] = sum_s sum_{k: read(k) = r} f_{s,k}(y, x) sum_w ( n_h a(x; xs, sigma_h) a(y; ys, sigma_h)
 *                                                                    + n_l a(x; xs, sigma_l) a(y; ys, sigma_l) )
 *
 * over the sources s (the target, then the contaminants), the sub-samples k of read interval r and the bins w; (xs, ys)
 * the bin's frame position, sigma_h / sigma_l its float32 PSF widths (what the production throwers use), f the
 * wavelength-dependent flat of sub-sample k (1 with WAYNE_F_ADD_FLAT off or without a flat cube).  (n_h, n_l) by mode:
 *
 *   WAYNE_EXPECT_COUNTS  count, nwide = those of this run (the same Philox draws): n_h = min(max(nwide, 0), count),
 *                        n_l = count - n_h.  E is the exact conditional expectation of the slot's accumulators (acc_e
 *                        of wayne_exposure_debug_fetch) given the bin counts the run drew, for WAYNE_RNG_SPLIT and
 *                        WAYNE_RNG_PHILOX.
 *   WAYNE_EXPECT_MEAN    lambda = the counts chain before the draw / the rounding, lambda+ = lambda finite and > 0 ?
 *                        min(lambda, 2147483647) : 0; n_h = min(max(ratio, 0), 1) lambda+, n_l = lambda+ - n_h.  The
 *                        unconditional expectation, up to the truncation in nwide = (int)(count ratio) (< 1 electron per
 *                        bin and sub-sample, moved from the wide to the narrow component) and, with stellar noise off,
 *                        rint(lambda).
 *
 * A component contributes nothing if its position is not finite or beyond +-1e6, or if its sigma is not finite or <= 0.
 * The kernel drops a component from pixels more than 8 sigma of that component away from the bin: no pixel of interval
 * r loses more than 2 Phi(-8) = 1.3e-15 of the electrons thrown in r.  NOT in E: sky, cosmic rays, dark current, the
 * gaussian-noise stage, gain, non-linearity, charge traps -- E is the truth of the thrower stage in electrons, not a
 * noise-free read.  The plane is R * S * S doubles, its 5-pixel border zero, all of it written on every run; the same
 * bytes in any slot, on either stream and on every run (no floating-point atomics).  Opt-in: without
 * wayne_exposure_set_expected every launch and every byte stay as they are.  Added within WAYNE_ABI_VERSION 7: new
 * symbols only.
 */
#define WAYNE_EXPECT_COUNTS 1
#define WAYNE_EXPECT_MEAN 2

/* After wayne_exposure_upload, before run: every run of the slot also renders the plane, at the very end of its back
 * half (behind the extraction's launches and k_fits_words) on the slot's stream (mode 0 clears).  The plane's buffer is
 * reserved by this call, for slots that ask only.  wayne_exposure_upload clears it.  WAYNE_E_STATE on a slot that is not
 * uploaded; WAYNE_E_INVALID in replay mode (which reproduces the reference: it has no such product), for a mode that is
 * none of the above or with more than 16 reads -- the slot stays usable, without the option. */
int wayne_exposure_set_expected(wayne_ctx *ctx, int slot, int mode);
/* The plane into the caller's (pageable) memory, R * S * S doubles.  Synchronises and settles the run as
 * wayne_exposure_download does (an exposure run a second time renders again).  WAYNE_E_STATE without the option. */
int wayne_exposure_download_expected(wayne_ctx *ctx, int slot, double *out);
/* HIP-event time of k_expect (every source's launch and the clearing of the plane) while wayne_profile_enable is on,
 * since wayne_profile_reset: renderings and total milliseconds.  wayne_profile_select's bit 10 selects it.  Synchronises. */
int wayne_expected_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- the ramp fit: rate, error and flags per pixel (no reference counterpart) ---- */

/*
 * What an observer keeps of a STARING exposure: every pixel's up-the-ramp samples fitted with a line, samples behind
 * saturation dropped, a cosmic ray -- a jump in the ramp -- cut out of it (k_ramp_fit, behind the reads on the slot's
 * stream).  Three planes of S * S: rate (float64, e-/s), var (float64, (e-/s)^2) and word (uint32), 20 bytes a pixel.
 * The law, float64 throughout, bordered coordinates of side S.  For a light-sensitive pixel P_k (k = 0 .. R) are the
 * slot's reads, and L_k, g and dt_j exactly the extraction's (wayne_extract_desc above; the step bits WAYNE_X_LINEARISE,
 * WAYNE_X_DARK and WAYNE_X_GAIN with the same meaning; the gain step is required, as for the variances); rn =
 * read_noise_e is the read noise of a difference of two reads in electrons (wayne_variance_desc.read_noise):
 *
 *   e_0 = 0, e_k = L_k g                                  cumulative electrons
 *   K   = the largest K <= R with P_k < saturation_dn for every 1 <= k <= K, and K = 0 if not P_0 < saturation_dn
 *         (a NaN read is not < saturation_dn; a sample behind a saturated one is never used)
 *   d_j = e_{j+1} - e_j,  r_j = d_j / dt_j,  j = 0 .. K-1;   G = {0 .. K-1}
 *   med(G) = the element of rank floor((|G| - 1) / 2) of {r_j : j in G} in ascending order (the lower median; equal
 *            values in order of j); 0 for an empty G
 *   jump test (k_jump > 0), repeated while |G| >= 3:
 *     m = med(G), f0 = max(m, 0)
 *     z_j = (d_j - m dt_j) / sqrt(f0 dt_j + rn^2) for j in G;   j* = the lowest j with the largest z_j
 *     z_j* > k_jump ? G <- G \ {j*}, bit j* of `jump` set : stop          (upward jumps only: a ray adds charge)
 *   fit: f0 = max(med(G), 0);  a_j = f0 dt_j + rn^2;  o = -rn^2 / 2
 *     the generalised least squares of d = f dt over j in G with cov(d_j, d_j) = a_j and cov(d_j, d_j+1) = o when both
 *     are in G (two differences that share a read share its noise; a removed interval cuts the chain), solved as written:
 *     ascending j:  j not in G: c_j = y_j = 0.  j in G: link = (j-1 in G); den = a_j - (link ? o c_{j-1} : 0);
 *                   c_j = (j+1 in G) ? o / den : 0;   y_j = (dt_j - (link ? o y_{j-1} : 0)) / den
 *     descending j: w_j = y_j - c_j w_{j+1}   (w_K = 0)
 *     num = sum_{j in G, ascending} w_j d_j      den = sum_{j in G, ascending} w_j dt_j
 *   rate = den > 0 ? num / den : 0     var = den > 0 ? 1 / den : 0     word = K << 16 | jump
 *
 * Reference pixels (the 5-pixel border) get rate = var = word = 0.  The host derives nsamp = K - popcount(jump), the
 * time sum_{j in G} dt_j and a data-quality value from the word.  Limits: f0 is the median rate, not iterated on the
 * fitted one; max(med, 0) of pure noise is biased upward, so at rate 0 an ensemble's variance is ~0.83 of the predicted
 * one; downward jumps are not looked for.  A SCANNING exposure is not what this is for: the star crossing a pixel is a
 * jump, and with the jump test on a scan's trace is flagged as cosmic rays.  The planes are a function of the reads
 * alone: the same bytes in any slot, on either stream and on every run.  Works in every mode that produces reads
 * (replay mode, carried traps, any read type).  Opt-in: without wayne_exposure_set_rampfit every launch and every byte
 * stay as they are.  Added within WAYNE_ABI_VERSION 7: new symbols and a new struct only.
 */
typedef struct wayne_rampfit_desc {
  uint32_t steps;       /* WAYNE_X_LINEARISE | WAYNE_X_DARK | WAYNE_X_GAIN; WAYNE_X_GAIN is required */
  double read_noise_e;  /* rn: finite and > 0 (20 is the variances' default) */
  double k_jump;        /* finite and >= 0; 0 switches the jump test off (5 is a sensible value) */
  double saturation_dn; /* finite and > 0 (65000 lies below the 78000 DN clip and the uint16 ceiling) */
} wayne_rampfit_desc;

/* After wayne_exposure_upload, before run: every run of the slot also fits its ramps, at the end of its back half
 * (behind the extraction's launches and k_fits_words, in front of k_expect) on the slot's stream.  desc == NULL clears;
 * wayne_exposure_upload clears it too.  The planes' buffer (20 S^2 bytes) is reserved by this call, for slots that ask
 * only.  WAYNE_E_STATE on a slot that is not uploaded; WAYNE_E_INVALID for a bad slot, the gain step off, a steps bit
 * outside the three, a read_noise_e that is not finite and > 0, a k_jump or saturation_dn that is negative or not finite,
 * or saturation_dn = 0 -- the slot stays usable and runs without the fit. */
int wayne_exposure_set_rampfit(wayne_ctx *ctx, int slot, const wayne_rampfit_desc *desc);
/* The planes into the caller's (pageable) memory, S * S each.  Synchronises and settles the run as
 * wayne_exposure_download does (an exposure run a second time is fitted again).  WAYNE_E_STATE without the option or
 * before a run. */
int wayne_exposure_download_rampfit(wayne_ctx *ctx, int slot, double *rate, double *var, uint32_t *word);
/* HIP-event time of k_ramp_fit while wayne_profile_enable is on, since wayne_profile_reset: launches and total
 * milliseconds.  wayne_profile_select's bit 11 selects it.  Synchronises. */
int wayne_rampfit_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- the calibrated reads: an `_ima` file's SCI, ERR and DQ (no reference counterpart) ---- */

/*
 * What a SCAN observer with a reduction of their own starts from: the instrument pipeline's intermediate file, in which
 * every read has the zero read subtracted, is linearised, dark-subtracted and in electrons, with an error and a
 * data-quality plane beside it (k_ima, behind k_ramp_fit on the slot's stream, in front of k_expect).  The law, float64
 * throughout, bordered coordinates of side S, n = S * S.  For a light-sensitive pixel P_k (k = 0 .. R) are the slot's
 * reads, any read type, and L_k, g and dt_j exactly the extraction's (wayne_extract_desc above; the step bits
 * WAYNE_X_LINEARISE, WAYNE_X_DARK and WAYNE_X_GAIN with the same meaning; the gain step is required, as for the
 * variances); q = g / 2.35; rn = read_noise_e the read noise of a difference of two reads in electrons
 * (wayne_variance_desc.read_noise); sat = saturation_dn:
 *
 *   t_0 = 0, t_k = sum_{j<k} dt_j   (ascending j)
 *   e_0 = 0, e_k = L_k g
 *   K   = the ramp fit's: the largest K <= R with P_k < sat for every 1 <= k <= K, 0 if not P_0 < sat   (a NaN is not <)
 *   s_k = sqrt(max(e_k, 0) + rn^2 (q q))    (k >= 1; s_0 = 0)
 *   units WAYNE_IMA_COUNTS:  SCI_k = (float32) e_k            ERR_k = (float32) s_k
 *   units WAYNE_IMA_RATE  :  SCI_k = (float32)(e_k / t_k)     ERR_k = (float32)(s_k / t_k)     (k >= 1; read 0: both 0)
 *   DQ_k  = (k > K or (k = 0 and K = 0 and not P_0 < sat) ? 256 : 0)
 *         | (the slot also has a ramp fit and some bit j < k of its `jump` is set ? 8192 : 0)
 *   reference pixels (the 5-pixel border): SCI = ERR = 0, DQ = 0
 *
 * The cast to float32 rounds to nearest even.  A cosmic ray in interval j contaminates every cumulative e_k with k > j,
 * so those are the reads flagged; the jump bits are those of the word k_ramp_fit has just written for the same run (with
 * the ramp fit's own saturation_dn and k_jump; none without a ramp fit on the slot or with its k_jump = 0).  In a SCAN with
 * the jump test on the trace itself is flagged, as in the instrument's ima.  The bit patterns of a NaN are not specified.
 *
 * The payload, in file order -- the last read first, as in a raw file (wayne_exposure_set_fits's convention).  With
 * pad(b) = b rounded up to a multiple of 2880, sci_stride = pad(4 n), dq_stride = pad(2 n) and imset_stride =
 * 2 sci_stride + dq_stride (wayne_ima_layout), imset f = 0 .. R holds read k = R - f:
 *
 *   [f imset_stride                 ..)  SCI_k, n big-endian float32, then zeros to sci_stride
 *   [f imset_stride + sci_stride    ..)  ERR_k, the same
 *   [f imset_stride + 2 sci_stride  ..)  DQ_k,  n big-endian int16, then zeros to dq_stride
 *
 * so that every section is one contiguous piece of a file: an image HDU's data and its padding, which is written on every
 * run.  The payload is a function of the reads and the ramp fit's word alone: the same bytes in any slot, on either
 * stream and on every run.  Works in every mode that produces reads (replay mode, carried traps, any read type).  Not in
 * it: reference-pixel values and a bias-level correction, the zero-read signal correction, flat-fielding.  Opt-in:
 * without wayne_exposure_set_ima every launch and every byte stay as they are.  Added within WAYNE_ABI_VERSION 7: new
 * symbols and a new struct only.
 */
#define WAYNE_IMA_RATE 1
#define WAYNE_IMA_COUNTS 2
typedef struct wayne_ima_desc {
  uint32_t steps;       /* WAYNE_X_LINEARISE | WAYNE_X_DARK | WAYNE_X_GAIN; WAYNE_X_GAIN is required */
  int units;            /* WAYNE_IMA_RATE (e-/s) or WAYNE_IMA_COUNTS (e-) */
  double read_noise_e;  /* rn: finite and > 0 (20 is the variances' default) */
  double saturation_dn; /* finite and > 0 (65000 is the ramp fit's default) */
} wayne_ima_desc;

/* The strides of the payload for a frame of side S (even) with R read intervals (1 .. 15): host arithmetic, no device.
 * The payload is (R + 1) * imset_stride bytes.  WAYNE_E_INVALID otherwise. */
int wayne_ima_layout(int S, int R, size_t *sci_stride, size_t *dq_stride, size_t *imset_stride);
/* After wayne_exposure_upload, before run: every run of the slot also forms its calibrated reads.  desc == NULL clears;
 * wayne_exposure_upload clears it too.  The payload's buffer (168 MB at 1024^2 and NSAMP 16) is reserved by this call,
 * for slots that ask only.  WAYNE_E_STATE on a slot that is not uploaded; WAYNE_E_INVALID for a bad slot, the gain step
 * off, a steps bit outside the three, a unit that is neither of the two, a read_noise_e or saturation_dn that is not
 * finite and > 0, or more than 16 reads -- the slot stays usable and runs without the option. */
int wayne_exposure_set_ima(wayne_ctx *ctx, int slot, const wayne_ima_desc *desc);
/* The payload into the caller's (pageable) memory, (R + 1) * imset_stride bytes.  Synchronises and settles the run as
 * wayne_exposure_download_rampfit does (an exposure run a second time is calibrated again).  WAYNE_E_STATE without the
 * option or before a run. */
int wayne_exposure_download_ima(wayne_ctx *ctx, int slot, void *payload);
/* HIP-event time of k_ima while wayne_profile_enable is on, since wayne_profile_reset: launches and total milliseconds.
 * wayne_profile_select's bit 12 selects it.  Synchronises. */
int wayne_ima_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- inter-pixel capacitance ------------------------------------------- */

/* In a hybrid CMOS array a pixel's reading holds a few per cent of each neighbour's charge.  With the option, the
 * electrons each read interval collected (target, contaminants, cosmic rays: the thrower's int64 accumulators q_r,
 * 2^-28 e-, bordered S x S) are coupled before k_ramp reads them.  The law, in integers:
 *
 *   W[i][j] = (int64) rint(k[i][j] * 65536)   for the eight neighbours;   W[1][1] = 65536 - sum of them
 *   q'_r[y, x] = floor((sum_{dy, dx in -1..1} W[dy+1][dx+1] q_r[y+dy, x+dx] + 32768) / 65536)
 *
 * W[1][2] is the share a pixel receives from its right-hand neighbour; q is 0 beyond the frame; q' is 0 on the 5-pixel
 * reference border (charge coupled onto reference pixels is lost).  The sum is exact for every int64 input (k_ipc.h).
 * k_ramp, in whichever variant the slot selects, then reads q' instead of q: every cumulative read is coupled.  Not
 * coupled: the sky (drawn inside k_ramp), the expected image, reference pixels.  Stateless; works beside every other
 * option but replay mode.  Opt-in: without wayne_exposure_set_ipc every launch and every byte stay as they are.  Added
 * within WAYNE_ABI_VERSION 7: new symbols and a new struct only. */
typedef struct wayne_ipc_desc {
  double k[3][3]; /* the eight neighbour weights; k[1][1] is not looked at (the centre is what the neighbours leave) */
} wayne_ipc_desc;

/* The nine integer weights of a kernel, w[3 i + j] = W[i][j]: host arithmetic, no device.  WAYNE_E_INVALID for a
 * neighbour weight that is not finite or is negative, or when the rounded neighbours sum to more than 65536. */
int wayne_ipc_weights(const wayne_ipc_desc *desc, int32_t w[9]);
/* After wayne_exposure_upload, before run: every run of the slot couples its accumulators (k_ipc at the end of the front
 * half, so wayne_exposure_debug_fetch's acc_e between the halves returns what k_ramp will read).  desc == NULL clears;
 * wayne_exposure_upload clears it too.  The second accumulator array is reserved by this call, for slots that ask only.
 * WAYNE_E_STATE on a slot that is not uploaded; WAYNE_E_INVALID for a bad slot, in replay mode (the reference has no
 * coupling) and for what wayne_ipc_weights refuses -- the slot stays usable and runs without the option. */
int wayne_exposure_set_ipc(wayne_ctx *ctx, int slot, const wayne_ipc_desc *desc);
/* HIP-event time of k_ipc and k_ipc_clear (one interval spans both) while wayne_profile_enable is on, since
 * wayne_profile_reset: coupled exposures and total milliseconds.  wayne_profile_select's bit 13 selects it.  Synchronises. */
int wayne_ipc_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- limb darkening per wavelength bin ---------------------------------- */

/* A device light curve (lc_z of the descriptor) uses ONE set of Claret coefficients, lc_ld, for every wavelength bin.
 * With a table the slot's depth matrix is computed by k_lightcurve_ld with four coefficients per bin.  The law: with
 * I(mu) = c0 + sum_{n=1..4} a_n mu^(n/2), c0 = 1 - sum a_n, the blocked flux is linear in the coefficients,
 *
 *   B_n(z, p) = int_{occulted region} mu^(n/2) dA,  n = 0 .. 4                  (B_0: the lens area)
 *             = 2 pi (1 - mu_f^(n/2+2)) / (n/2+2)        radii wholly inside the planet, mu_f = sqrt(1 - clip(p - z, 0, 1)^2)
 *             + int_{|z-p|}^{min(1,z+p)} mu^(n/2) r theta(r) dr                 k_lightcurve's 24-node tanh-sinh rule
 *   deficit[k][w] = (c0(w) B_0 + sum_n a_n(w) B_n)(z_k, p_w) / (pi (1 - sum_n a_n(w) n/(n+4)))
 *   depth[k][w]   = deficit[k][w] + p_w^2 hidden_k / (1 + p_w^2)                the eclipse term, unchanged
 *
 * float32 integrand, float64 sums; grid, Chebyshev interpolation in p and the decisions between its paths are
 * k_lightcurve's (five interpolants, one per B_n).  A NaN radius ratio gives depth 0.  Not covered: limb darkening
 * in the eclipse term, a contaminant that eclipses, coefficients looked up from stellar parameters.  Counted under the
 * "k_lightcurve" slot of wayne_profile.  Opt-in: without a table every launch and every byte stay as they are.  Added
 * within WAYNE_ABI_VERSION 7: new symbols only.
 *
 * After wayne_exposure_upload, before run: Claret coefficients per wavelength bin, ld[w*4 + n-1], n_wl == the
 * descriptor's n_wl.  ld == NULL or n_wl == 0 clears; wayne_exposure_upload clears.  The slot then launches
 * k_lightcurve_ld in place of k_lightcurve; desc.lc_ld is ignored while a table is set.  The table is copied (into
 * pinned staging, four planes of n_wl on the device): the caller's array is free on return.  WAYNE_E_STATE on a slot that
 * is not uploaded; WAYNE_E_INVALID when the slot has no device light curve (lc_z was NULL), n_wl differs from the slot's,
 * a coefficient is not finite or 1 - sum a_n n/(n+4) <= 0 for some bin -- the slot stays usable and runs without a
 * table.  wayne_exposure_debug_depth serves the matrix as it is. */
int wayne_exposure_set_limb_darkening(wayne_ctx *ctx, int slot, const double *ld, int n_wl);

/* ---- star spots ---------------------------------------------------------- */

/* The star of a device light curve is a clean limb-darkened disc.  With spots, k_lightcurve_spots is enqueued directly
 * behind the slot's light-curve launch (k_lightcurve or k_lightcurve_ld) on the same stream and rewrites the depth
 * matrix in place, so k_prep_sub and wayne_exposure_debug_depth see the spotted matrix.  All quantities are float64,
 * lengths in stellar radii in the sky frame of the planet's track (px, py).  Spot i is a circle IN PROJECTION: centre
 * (cx, cy), radius, contrast c[i*W + w] >= 0 (spot over photosphere intensity in bin w; > 1: a facula); the
 * limb-darkening law inside a spot is the photosphere's.  With I(mu) = c0 + sum_n a_n mu^(n/2), a'_0 = c0 = 1 - sum a_n,
 * a'_n = a_n (the table's coefficients of bin w, or lc_ld) and F0_w = pi (1 - sum a_n n/(n+4)):
 *
 *   Q_n(P, C, p, r) = int over (disc of radius p at P) n (disc of radius r at C) of mu^(n/2) dA     wayne_spot_lens_basis
 *   S_{i,n} = Q_n(C_i, C_i, r_i, r_i)                                          the whole spot
 *   D_w     = sum_i (1 - c_{i,w}) sum_n a'_n(w) S_{i,n}
 *   X_{k,w} = sum_i (1 - c_{i,w}) sum_n a'_n(w) Q_n(P_k, C_i, p_w, r_i)        spots in list order, n ascending
 *   depth'[k][w] = (depth[k][w] F0_w - X_{k,w}) / (F0_w - D_w)                 rows with z_k < 10 and hidden_k = 0,
 *                                                                              columns with a radius ratio
 *   depth'[k][w] = depth[k][w]                                                 everywhere else
 *
 * An out-of-transit row stays exactly 0; without an overlap the depth is multiplied by F0 / (F0 - D), the bias of
 * unocculted spots; during a crossing it drops by the light the planet no longer blocks.  Q_n is a FIXED rule: with
 * d = |C - P|, u = (C - P) / d (or (1, 0)), v = (-u_y, u_x): zero for d >= p + r (decided before any node is touched);
 * for d <= |p - r| the smaller circle in two panels, phi in [0, pi/2] and [pi/2, pi]; otherwise the part bounded by
 * the spot's circle and the part bounded by the planet's, either side of the chord t* = (d^2 + p^2 - r^2) / (2 d).  A
 * panel (cc, rad, sg, phi range) takes the 10 Gauss-Legendre nodes g, omega of [-1, 1] in both directions:
 * phi_a = mid + half g_a, t = cc - sg rad cos phi_a, h = rad sin phi_a, s_b = h g_b, (x, y) = P + t u + s_b v,
 * Q_n += omega_a half rad sin phi_a h omega_b mu(x, y)^(n/2); panels in that order, a outer, b inner, ascending.  It is
 * within 1e-6 of the lens area of the converged integral for spots that stay inside radius 0.98.  float64 throughout,
 * no atomics, no LDS, no scratch.  Not covered: rotation or evolution within a visit, foreshortening, spots at or
 * across the limb, overlapping spots, spots in the eclipse term, a changed stellar spectrum, spotted contaminants,
 * interpolation in p.  Opt-in: without spots every launch and every byte stay as they are.  Added within
 * WAYNE_ABI_VERSION 7: new symbols and a new struct only. */
#define WAYNE_MAX_SPOTS 8
typedef struct wayne_spots_desc {
  int32_t n;                        /* spots, at most WAYNE_MAX_SPOTS; 0 clears */
  double cx[WAYNE_MAX_SPOTS], cy[WAYNE_MAX_SPOTS], radius[WAYNE_MAX_SPOTS];
  const double *contrast;           /* [n * n_wl], spot-major */
  const double *px, *py;            /* [n_sub]: the planet's centre at every sub-sample */
} wayne_spots_desc;
/* After wayne_exposure_upload (and after wayne_exposure_set_limb_darkening, which clears the spots: they are checked
 * against the coefficients in force), before run.  desc == NULL or n == 0 clears; wayne_exposure_upload clears.  The
 * arrays are copied: free on return.  WAYNE_E_STATE on a slot that is not uploaded; WAYNE_E_INVALID -- the slot stays
 * usable and runs unspotted -- for more than 8 spots, a radius that is not finite or <= 0, |C_i| + r_i > 0.98, two spots
 * with |C_i - C_j| < r_i + r_j, a contrast that is not finite or < 0, F0_w - D_w <= 0 in some bin, a slot without a
 * device light curve, n_wl or n_sub other than the slot's, a track value that is not finite on a transit row. */
int wayne_exposure_set_spots(wayne_ctx *ctx, int slot, const wayne_spots_desc *desc, int n_wl, int n_sub);
/* Q_0 .. Q_4 of the rule above: pure host arithmetic, the inline function the kernel compiles. */
void wayne_spot_lens_basis(double px, double py, double cx, double cy, double p, double r, double out[5]);
/* The rule's Gauss-Legendre nodes and weights (numpy.polynomial.legendre.leggauss(10), to the bit). */
void wayne_spot_rule(double nodes[10], double weights[10]);
/* HIP-event time of k_lightcurve_spots while wayne_profile_enable is on, since wayne_profile_reset: launches and total
 * milliseconds.  wayne_profile_select's bit 14 selects it.  Synchronises. */
int wayne_spots_profile(wayne_ctx *ctx, uint64_t *launches, double *ms);

/* ---- measurement ------------------------------------------------------- */

#define WAYNE_PROF_KERNELS 8
typedef struct wayne_profile {
  /* per kernel: launches and total milliseconds measured with HIP events on
   * the context stream since wayne_profile_reset */
  const char *name[WAYNE_PROF_KERNELS];
  uint64_t launches[WAYNE_PROF_KERNELS];
  double ms[WAYNE_PROF_KERNELS];
  uint64_t electrons; /* electrons thrown */
} wayne_profile;

int wayne_profile_enable(wayne_ctx *ctx, int on);
/* Restrict the HIP-event timing to the kernels whose bit (1 << index in `name`) is set; every event
 * pair costs a few microseconds of stream time, so a throughput measurement that only needs one
 * kernel's duration selects that kernel.  Default: all kernels. */
int wayne_profile_select(wayne_ctx *ctx, unsigned mask);
int wayne_profile_reset(wayne_ctx *ctx);
int wayne_profile_get(wayne_ctx *ctx, wayne_profile *out); /* synchronises */

/* ---- host helpers ------------------------------------------------------ */

/* Philox4x32-10 block (Random123), used by the host for the per-exposure
 * jitter / seed draws (exposure_generator.py:327-329). */
void wayne_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* The per-exposure host draws of scanning_frame (exposure_generator.py:327-329)
 * from the Philox HOST stage: for sub-sample k, block (k, 0, 0, exposure) gives
 * two standard normals (Box-Muller of words 0,1; the caller scales them by
 * x_jitter / y_jitter) and s_rand_seeds[k] = randint(0, 100000) from word 2.
 * Pure host arithmetic; any output pointer may be NULL. */
void wayne_host_sample_draws(uint32_t seed, uint32_t exposure, int n_samples,
                             double *z_x, double *z_y, int32_t *rand_seed);

#ifdef __cplusplus
}
#endif
#endif /* WAYNE_HIP_H */

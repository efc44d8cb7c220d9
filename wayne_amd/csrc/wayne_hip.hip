// libwayne_hip.so -- C ABI (include/wayne_hip.h) over the gfx950 kernels.
// Host side: context, HBM buffers, launch sequence, HIP-event profiling.
#include "../../include/wayne_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.h"
#include "host_plan.h"

using namespace wayne;

struct wayne_ctx;

namespace {

int fail(wayne_ctx* c, int code, const std::string& msg);   // (keeps `msg` as the context's last error: below, with the context)

#define HIP_TRY(ctx, expr)                                                                     \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess)                                                                     \
      return fail((ctx), WAYNE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
  } while (0)

inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

enum ProfKernel { PK_PREP_WL = 0, PK_PREP_SUB, PK_THROW, PK_COSMIC, PK_RAMP, PK_LIGHTCURVE, PK_NARROW, PK_LANE,
                  PK_EXTRACT, PK_FITS, PK_EXPECT, PK_RAMPFIT, PK_IMA, PK_IPC, PK_SPOTS };   // (PK_EXTRACT .. PK_SPOTS lie beyond wayne_profile's arrays, which the ABI fixes: wayne_extract_profile / wayne_fits_profile / wayne_expected_profile / wayne_rampfit_profile / wayne_ima_profile / wayne_ipc_profile / wayne_spots_profile report them)
constexpr int kProfKernels = WAYNE_PROF_KERNELS + 7;
const char* const kProfNames[WAYNE_PROF_KERNELS] = {"k_prep_wl", "k_prep_sub",   "k_throw",  "k_cosmic",   /* (cosmic rays ride in k_prep_sub: slot kept for the ABI) */
                                                    "k_ramp",    "k_lightcurve", "k_narrow", "k_lane"};

// A device buffer: an allocation of its own (freed with it), or a view into another one.  Not copied: slots and sources
// live in fixed arrays inside the context.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool owns = true;        // false: a view into another allocation (a staging arena's device mirror)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p && owns) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (!owns) { p = nullptr; cap = 0; owns = true; }
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (bytes == 0) return hipSuccess;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void view(void* at) {
    if (owns && p) (void)hipFree(p);
    p = at;
    cap = 0;
    owns = false;
  }
  template <class T> T* as() const { return (T*)p; }
};

// A grow-only block of pinned host memory.
struct PinnedBuf {
  char* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  bool reserve(size_t bytes) {      // false: no pinned memory (the block is then empty)
    if (bytes <= cap) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
    cap = bytes;
    return true;
  }
};

// A staging arena: a pinned block, its device mirror, and the event that tells when the last copy from the block into
// the mirror is done.  The arrays of a call are placed at 64-byte-aligned offsets of the block and DevBuf views pointed at
// the same offsets of the mirror: all of them reach the device in ONE copy, enqueued from pinned memory, so the call
// returns without waiting for the stream -- the next begin() waits instead, before the block is overwritten.
struct StageArena {
  PinnedBuf host;
  DevBuf dev;
  hipEvent_t ev = nullptr;
  bool pending = false;    // a copy out of `host` was enqueued that nobody has waited for yet
  size_t used = 0;
  ~StageArena() { if (ev) (void)hipEventDestroy(ev); }
  // Room for `bytes`, empty.  (with_event = false: for a caller that synchronises its stream before it returns.)
  int begin(wayne_ctx* c, size_t bytes, const char* nomem_msg, bool with_event = true) {
    if (pending) { HIP_TRY(c, hipEventSynchronize(ev)); pending = false; }
    if (!host.reserve(align64(bytes))) return fail(c, WAYNE_E_NOMEM, nomem_msg);
    if (with_event && !ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(c, dev.reserve(host.cap));
    used = 0;
    return WAYNE_OK;
  }
  // The next `bytes` of the block (null: they do not fit); `view` is pointed at the same offset of the mirror.
  char* place(DevBuf& view, size_t bytes) {
    bytes = std::max<size_t>(bytes, 1);
    if (used + bytes > host.cap) return nullptr;
    char* h = host.p + used;
    view.view((char*)dev.p + used);
    used += align64(bytes);
    return h;
  }
  bool put(DevBuf& view, const void* src, size_t bytes) {
    char* h = place(view, bytes);
    if (h && bytes) std::memcpy(h, src, bytes);
    return h != nullptr;
  }
  int commit(wayne_ctx* c, hipStream_t stream) {
    HIP_TRY(c, hipMemcpyAsync(dev.p, host.p, used, hipMemcpyHostToDevice, stream));   // one copy for all arrays
    if (ev) { HIP_TRY(c, hipEventRecord(ev, stream)); pending = true; }
    return WAYNE_OK;
  }
  // host copy of a placed array: the block still holds it (at the offset of the array's view in the mirror) until the
  // next begin()
  template <class T> const T* host_of(const DevBuf& view) const { return (const T*)(host.p + ((const char*)view.p - (const char*)dev.p)); }
};

// What one source (the target, or a contaminating field star: wayne_exposure_set_sources) of an exposure holds: its
// inputs, its per-bin and per-sub-sample scratch and its launch plan.  Each source has buffers of its own: with
// fork_narrow, k_narrow of one source still reads its counts / prefix on the side stream while the main stream moves on.
struct SourceState {
  bool fused_last = false;    // the last front half ran fused: positions / routing arrays were not written (debug_fetch)
  PrepArgs last_prep{};       // ... and k_prep_sub's arguments of that run
  int last_chunks = 0;
  int W = 0;
  uint32_t seed = 0;          // visit seed of the source's thrower-side streams (wayne_source_seed)
  DevBuf wl, flux, xref, yref;   // target: views into the slot's `stage`; contaminant: views into src_stage
  DevBuf ratio, sigl, sigh, sens, dlam;
  DevBuf counts, nwide, nsplit, nlane, prefix, xpos, ypos, sub, chunk_total, chunk_box;
  DevBuf tr;                  // trace coefficients of the K sub-samples (plan::trace_table): a view into the arena of xref / yref
  int kb = 1;             // sub-samples a workgroup of k_lane takes (k_lane, "BATCHES")
  bool thin = false;      // few electrons per (workgroup, sub-sample): k_lane flushes from its first-touch list
  double max_narrow = 0.;   // host estimate: most narrow electrons expected in a bin of the longest sub-sample
  double max_chunk_electrons = 0.;   // host estimate: electrons of the fullest k_lane chunk in the longest sub-sample
  double est_thrown = 0.;   // host estimate of the electrons k_throw handles in the longest sub-sample
  unsigned char chunk_order[kMaxChunks] = {0};   // chunks of kNarrowThreads bins, most electrons first (ThrowArgs::chunk_order)
  unsigned char lane_order[kMaxChunks] = {0};    // chunks of kLaneThreads bins, most electrons first
  StageArena src_stage;   // a contaminant's own inputs (wl, flux, offset positions, trace coefficients)
  plan::WlCache wl_cache;   // what ratio .. dlam on the device were worked out for (k_prep_wl at upload; host_plan.h)
};

constexpr int kMaxSources = WAYNE_MAX_SOURCES;   // contaminants per exposure

// the layout of a slot's status block `misc`, declared here only: [8] the last run that overflowed, [12] the last run
// that met a bin beyond its launch sequence (PrepArgs::status points at these two; the first word is spare)
struct SlotMisc {
  unsigned long long spare;
  uint32_t over_run, beyond_run;
  int bits(uint32_t run) const { return (run && over_run == run ? 1 : 0) | (run && beyond_run == run ? 2 : 0); }   // as wayne_exposure_status reports them
};

// The pinned host mirror of one of a slot's products (its reads, its spectra block, its FITS words), followed by a copy
// of the slot's status block -- inside the pinned block: a copy into pageable memory would block the caller -- and the
// number of the run the copies were enqueued behind.  `misc` is null until a fetch has succeeded.
struct PinnedMirror {
  PinnedBuf buf;
  SlotMisc* misc = nullptr;
  uint32_t run = 0;
  bool fetched() const { return buf.p && misc; }
  // What fetch_async / fetch_spectra_async / fetch_fits_async share, on c->stream: room for `bytes` and the status block
  // (refused as `nomem`), then the copies of `dev` and of the slot's status block, read against the slot's current run.
  // record_kdone: the exposure on the other stream waits for this one's KERNELS, not for its copy (wayne_ctx::ev_kdone)
  // -- the caller's choice: the reads always, FITS words unless this run's reads went in front of them, spectra never.
  int fetch(wayne_ctx* c, int slot, const void* dev, size_t bytes, bool record_kdone, const char* nomem);
};

// An exposure slot.  Its own SourceState is the target's (source 0); extra[0 .. n_extra) are the contaminants.
struct Slot : SourceState {
  bool uploaded = false;
  bool front_done = false;
  bool acc_dirty = false;
  bool acc_init = false;
  bool force_throw = false;   // the last run met a bin beyond a lane's reach: run with k_throw (set by look_at_status)
  bool ran = false;           // a whole run was enqueued whose status word nobody has looked at yet (settle)
  // The runs of the slot are numbered (from 1; counted on by wayne_exposure_run_front): a kernel raises a status word to
  // the number of its run and nothing clears the block on the device (k_prep.h, raise_status).  A copy of the block is
  // read against the number that was current when the copy was ENQUEUED: run_no for a read that waits for the stream,
  // PinnedMirror::run for the copies fetch_async / fetch_spectra_async / fetch_fits_async enqueue.
  uint32_t run_no = 0;
  wayne_exposure_desc d{};  // host copy (pointers are NOT valid after upload)
  int K = 0, R = 0;
  bool has_depth = false, has_replay_seed = false, has_lc = false, has_lc_hidden = false;
  DevBuf depth, dur, rseed, sread, read_dt, lc_z, lc_hidden, lc_rp;   // views into `stage` (depth: owned when computed by k_lightcurve)
  int n_extra = 0;                 // contaminants of this exposure (wayne_exposure_set_sources; cleared by upload)
  SourceState extra[kMaxSources];
  uint32_t extra_tag[kMaxSources] = {0};
  SourceState& source(int i) { return i == 0 ? *this : extra[i - 1]; }
  DevBuf acc, out, misc;  // misc: the slot's status block (Misc)
  DevBuf seg;             // cosmic-ray segments (CosmicArgs::seg): zeroed when allocated, k_ramp clears what it reads
  bool use_box = false;   // acc_box is valid: k_ramp loads the accumulators of a read only inside it (and where `seg` says)
  int acc_box[16][4] = {{0}};
  using Misc = SlotMisc;
  PinnedMirror pinned;    // pinned host copy of `out` (fetch_async / wait)
  // sky alias tables of this exposure (k_ramp): their arena, the view of the device copy, the lam_max they were built for
  StageArena sky_stage;
  DevBuf sky_tab;
  std::vector<uint32_t> sky_tab_keys;
  bool sky_alias_on = false, sky_pieces = false;
  uint32_t sky_mask = 0;
  int sky_L = 1;
  float sky_level[16] = {0};
  unsigned char sky_tab0[16] = {0};
  std::vector<double> read_dt_host;
  double lc_p_lo = 0., lc_p_hi = 0.;   // range of lc_rp
  // limb darkening per wavelength bin (wayne_exposure_set_limb_darkening; cleared by upload): four planes [4][W] in an
  // arena of their own; the slot then launches k_lightcurve_ld in place of k_lightcurve
  bool ld_on = false;
  StageArena ld_stage;
  DevBuf ld_tab;
  // star spots (wayne_exposure_set_spots; cleared by upload and by wayne_exposure_set_limb_darkening): k_lightcurve_spots
  // rewrites the depth matrix behind the light-curve launch.  One arena: contrast [n][W], the track px, py [K], lc_ld [4]
  bool spots_on = false;
  StageArena spot_stage;
  DevBuf spot_contrast, spot_px, spot_py, spot_ld;
  SpotArgs spot_args{};      // the geometry, the whole spots' integrals and the rule, filled when the spots are set
  // charge traps of this exposure (wayne_exposure_set_traps; cleared by upload): the parameters, and the start tables
  // in one arena -- [2][G] float64 (generic loop), then [2][G] float32 (production chain)
  bool traps_on = false;
  double trap_n[2] = {1., 1.}, trap_eta[2] = {0., 0.}, trap_tau[2] = {1., 1.}, trap_lo = 0., trap_hi = 0.;
  int trap_G = 0;
  StageArena trap_stage;
  DevBuf trap_d, trap_f;             // views of the float64 / float32 tables
  // a carried history on top of the traps (wayne_exposure_set_trap_history; cleared by upload and set_traps): the
  // exposure starts from the context's trap state and leaves its own behind (k_ramp_hist)
  bool hist_on = false;
  double hist_gap = 0., hist_fill[2] = {0., 0.};
  int hist_lit = 0;
  // spectral extraction of this exposure (wayne_exposure_set_extraction; cleared by upload): the plan, the partial sums
  // [2][chunks][R+1][S], and the result: the spectra block `ex_out`, laid out by `lay` (plan::spectra_layout; kept by
  // ex_relayout, which every setter below calls), with its pinned host copy followed by a copy of `misc`
  // (fetch_spectra_async / wait_spectra).  `ex_base`: the block as the last wait_spectra (in ex_pinned) or
  // download_spectra (in ex_host, which holds nothing in front of n_rejected) brought it back; null before any
  bool extract_on = false;
  wayne_extract_desc ex{};
  int ex_chunks = 0;
  DevBuf ex_part, ex_out;
  plan::SpectraLayout lay;
  PinnedMirror ex_pinned;
  const char* ex_base = nullptr;
  std::vector<double> ex_host;
  // cosmic-ray rejection of the extraction (wayne_exposure_set_crrej; cleared by upload and set_extraction): the flag
  // plane [S*S] uint16 and the chunks' flag counts [chunks][R+1][S]
  bool crrej_on = false;
  double cr_k = 0., cr_rn = 0.;
  int cr_lo = 0, cr_hi = 0;          // the mask rows
  DevBuf cr_mask, ex_part_n;
  // wavelength-binned channels of the extraction (wayne_exposure_set_channels; cleared by upload and set_extraction, not
  // by set_crrej): edges [C+1], wl_a [S], wl_b [S] in an arena of their own and the row groups' sums [chunks][4][R+1][2][C]
  bool chan_on = false;
  int ch_C = 0, ch_lo = 0, ch_hi = 0;
  uint32_t ch_flags = 0;
  StageArena ch_stage;
  DevBuf ch_edges, ch_wa, ch_wb, ch_part;
  // variances of the extraction (wayne_exposure_set_variance; cleared by upload and set_extraction, not by set_crrej or
  // set_channels): the chunks' sums [chunks][R+1][S] and, with channels, the row groups' [chunks][4][R+1][C]
  bool var_on = false;
  double var_rn = 0.;
  DevBuf ex_part_v, ch_part_v;
  // optimal extraction on top of the variances (wayne_exposure_set_optimal; cleared by what clears the variances): the
  // chunks' sums [3][chunks][R+1][S]
  bool opt_on = false;
  int opt_H = 0;
  DevBuf opt_part;
  // profile planes of the optimal extraction (cleared by what clears it).  Delivery (wayne_exposure_deliver_profile):
  // S1 of every window pixel [sum_p rows_p * S] and its pinned copy, fetched by a call of its own (`prof_fetched`: a copy
  // is enqueued or done).  A supplied profile (wayne_exposure_set_optimal_profile): the device copy in the same layout and
  // the window heights it was made for, checked against the plan's when the slot is run
  bool prof_deliver = false, prof_valid = false, prof_fetched = false;   // (prof_valid: a run has written the planes)
  DevBuf prof_planes;
  PinnedBuf prof_pinned;
  bool prof_fixed = false;
  int prof_rows[kExtractProducts] = {0};
  DevBuf prof_fix;
  // optimal channels (wayne_exposure_set_optimal_channels; needs the optimal extraction AND channels; cleared by what
  // clears either): the row groups' sums [chunks][4][R+1][3][C]
  bool optch_on = false;
  DevBuf optch_part;
  bool prof_fix_valid = false;       // prof_fix holds the profile of prof_rows / prof_fix_n and the caller's tag prof_fix_hash (kept across clears)
  size_t prof_fix_n = 0;
  uint64_t prof_fix_hash = 0;
  int prof_fix_R = 0;
  // FITS words of this exposure (wayne_exposure_set_fits; cleared by upload): the payload [(R+1)][fits_stride] bytes that
  // k_fits_words writes behind the ramp kernel and the extraction, and its pinned mirror (fetch_fits_async / wait_fits)
  bool fits_on = false;
  size_t fits_plane_bytes = 0, fits_stride = 0;
  DevBuf fits_dev;
  PinnedMirror fits_pinned;
  // the noise-free expected image of this exposure (wayne_exposure_set_expected; cleared by upload): the mode
  // (0: none) and the plane [R][S][S] float64 that k_expect renders at the very end of the back half
  int expect_mode = 0;
  DevBuf expect_plane;
  // the ramp fit of this exposure (wayne_exposure_set_rampfit; cleared by upload): its parameters and the planes
  // [rate S*S float64 | var S*S float64 | word S*S uint32] that k_ramp_fit writes near the end of the back half
  bool rampfit_on = false, rampfit_ran = false;
  wayne_rampfit_desc rampfit{};
  DevBuf rampfit_planes;
  // the calibrated reads of this exposure (wayne_exposure_set_ima; cleared by upload): their parameters, the strides of
  // the payload [(R+1)][SCI | ERR | DQ] that k_ima forms behind the ramp fit, and the payload
  bool ima_on = false, ima_ran = false;
  wayne_ima_desc ima{};
  size_t ima_sci_stride = 0, ima_dq_stride = 0, ima_imset_stride = 0;
  DevBuf ima_dev;
  // inter-pixel capacitance of this exposure (wayne_exposure_set_ipc; cleared by upload): the nine integer weights, the
  // coupled accumulators `acc_b` [R*S*S] that k_ipc writes and k_ramp then reads and clears, and their segment bits.
  // ipc_front: the front half that is waiting for its back half coupled; b_dirty: ... and no back half has cleared acc_b yet
  bool ipc_on = false, ipc_front = false, b_dirty = false;
  int ipc_w[9] = {0};
  DevBuf acc_b, seg_b;
  // staging arena of the descriptor's arrays: uploads are enqueued from here, so
  // wayne_exposure_upload returns without waiting for the slot's stream to drain
  StageArena stage;
};

struct ProfRec {
  int kernel;
  hipEvent_t a, b;
};

// HBM slots per context: every exposure of a batch keeps its inputs, scratch,
// accumulators and reads resident (~215 MB each at 1024^2 x 16 reads; buffers
// are allocated on first upload, so unused slots cost nothing).
constexpr int kSlots = 256;

}  // namespace

constexpr int kStreams = 2;   // exposures in even / odd slots run on different HIP streams

// Tuning and test knobs of a context.  Each is read ONCE from the environment (WAYNE_<NAME>) when the context is
// created; afterwards only wayne_ctx_set_knob changes it -- no entry point looks at the environment of a live context,
// so a thread that edits the environment cannot change what another thread's context launches (and getenv never races
// a setenv).  -1 = not set: the library's own choice.
struct Knobs {
  long long tile_ints = -1;      // LDS ints of a k_throw tile (thrower_lds_ints)
  long long batch = -1;          // sub-samples a k_lane workgroup takes (plan::lane_batches)
  long long thin = -1;           // k_lane's first-touch flush list on (1) / off (0)
  long long no_acc_box = -1;     // 1: k_ramp loads every accumulator (no boxes)
  long long lane_reach = -1;     // electrons a lane takes in an exposure launched without k_throw (lowers kLaneReach: exercises the re-run)
  long long throw_wgs = -1;      // k_throw workgroups per launch
  long long keep_narrow = -1;    // 1: k_narrow is launched even when no bin is expected to qualify
  long long no_fuse = -1;        // 1: never k_lane_fused
  long long fork_narrow = -1;    // 1: k_narrow on a side stream beside k_lane
  long long streams = -1;        // 1: every slot on one stream
  long long upload_timing = -1;  // 1: wayne_ctx_destroy prints the host time of wayne_exposure_upload by part
  long long narrow_compact = -1; // 0: k_narrow's pooled row chains stay on their groups' lanes (default: compacted across the workgroup)
  long long prep_wl_per_run = -1; // 1: k_prep_wl_run in front of every run (arrays, trace coefficients, status clear), as before the upload-time cache
  long long fuse_thrower = -1;   // 0: k_lane and k_narrow of the production pair as two launches (default: one grid, k_thrower)
  long long lane_tight_tile = -1; // 0: k_lane sizes its test-free tiles for the refined radius, 6.9 sigma (default: kLaneR16, the 16-bit radius)
  long long ramp_reads = -1;     // TIMING BUILDS (-DWAYNE_TIMING_KNOBS) only: k_ramp works through the first n reads
};
struct KnobName { const char* name; const char* env; long long Knobs::*field; };
const KnobName kKnobNames[] = {
    {"tile_ints", "WAYNE_TILE_INTS", &Knobs::tile_ints},       {"batch", "WAYNE_BATCH", &Knobs::batch},
    {"thin", "WAYNE_THIN", &Knobs::thin},                      {"no_acc_box", "WAYNE_NO_ACC_BOX", &Knobs::no_acc_box},
    {"lane_reach", "WAYNE_LANE_REACH", &Knobs::lane_reach},    {"throw_wgs", "WAYNE_THROW_WGS", &Knobs::throw_wgs},
    {"keep_narrow", "WAYNE_KEEP_NARROW", &Knobs::keep_narrow}, {"no_fuse", "WAYNE_NO_FUSE", &Knobs::no_fuse},
    {"fork_narrow", "WAYNE_FORK_NARROW", &Knobs::fork_narrow}, {"streams", "WAYNE_STREAMS", &Knobs::streams},
    {"upload_timing", "WAYNE_UPLOAD_TIMING", &Knobs::upload_timing}, {"ramp_reads", "WAYNE_RAMP_READS", &Knobs::ramp_reads},
    {"narrow_compact", "WAYNE_NARROW_COMPACT", &Knobs::narrow_compact},
    {"lane_tight_tile", "WAYNE_LANE_TIGHT_TILE", &Knobs::lane_tight_tile},
    {"fuse_thrower", "WAYNE_FUSE_THROWER", &Knobs::fuse_thrower},
    {"prep_wl_per_run", "WAYNE_PREP_WL_PER_RUN", &Knobs::prep_wl_per_run},
};
constexpr size_t kMiscBytes = 64;   // status block of a slot (Slot::Misc), zeroed when the context is created

constexpr size_t kCounterBytes = (size_t)kCounterStripes * kCounterStride * sizeof(unsigned long long);

// The streams and stream events of a context: a base of it, so that they are destroyed LAST -- a base goes after the
// members of the struct derived from it, i.e. after every buffer, arena and pinned block of the context has been freed.
struct CtxStreams {
  hipStream_t stream = nullptr;          // stream of the call in progress (one of streams[])
  hipStream_t streams[kStreams] = {nullptr, nullptr};
  // k_narrow of an exposure runs beside its k_throw (both only add into the accumulators): a side
  // stream per main stream, forked after the prep kernels and joined before the cosmic / ramp kernels
  hipStream_t side[kStreams] = {nullptr, nullptr};
  hipEvent_t ev_fork[kStreams] = {nullptr, nullptr}, ev_join[kStreams] = {nullptr, nullptr};
  bool fork_narrow = true;
  // Delivered pipeline (fetch_async): the kernels of the exposure that follows on the other stream wait for the
  // KERNELS of the fetched one (not for its copy).  Left alone, the two streams drift into phase -- both compute,
  // then both copy and share the PCIe link: 640 exposures/s -- instead of one copying while the other computes (810).
  hipEvent_t ev_kdone[kStreams] = {nullptr, nullptr};
  bool kdone_valid[kStreams] = {false, false};
  // Carried trap state (wayne_exposure_set_trap_history): exposures alternate over the streams and each k_ramp_hist reads
  // the state its predecessor wrote.  One event, recorded behind every k_ramp_hist launch and waited for in front of the
  // next one: the ramp kernels form a chain, the front kernels (prep, thrower) still overlap the previous exposure.
  // Created with the state (trap_state_reset / _upload).
  hipEvent_t ev_trap_chain = nullptr;
  bool trap_chain_valid = false;
  ~CtxStreams() {
    if (ev_trap_chain) (void)hipEventDestroy(ev_trap_chain);
    for (int i = 0; i < kStreams; ++i) {
      if (streams[i]) (void)hipStreamDestroy(streams[i]);
      if (side[i]) (void)hipStreamDestroy(side[i]);
      if (ev_fork[i]) (void)hipEventDestroy(ev_fork[i]);
      if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
      if (ev_kdone[i]) (void)hipEventDestroy(ev_kdone[i]);
    }
  }
};

struct wayne_ctx : CtxStreams {
  int device = 0;
  int n_streams = kStreams;              // knob `streams` = 1 serialises all exposures on one stream
  Knobs knobs;                           // frozen at creation (see Knobs)
  DevBuf status_all;                     // kSlots status blocks of kMiscBytes (Slot::misc views into it): ONE copy brings all of them back
  PinnedBuf status_host;                 // its pinned host mirror (settle)
  std::string err;
  // grism
  bool have_grism = false;
  unsigned long long grism_gen = 1;      // counts wayne_ctx_set_grism / wayne_ctx_set_calibration: what a source's per-wavelength arrays were worked out under (plan::WlCache)
  GrismDev g{};
  DevBuf sens_wl, sens_val;
  // what the upload keeps per spectrum (host_plan.h): per-bin count rates through this grism's sensitivity, the wide
  // fraction and sigma_l of a bin, the largest PSF sigma and the wavelength range -- cached on the spectrum's content
  plan::SpectrumEstimate est;
  plan::SpectrumEstimate src_est[kMaxSources];   // the same for the contaminants, one cache per list position
  // calibration
  bool have_cal = false;
  int subarray = 0, N = 0, S = 0, cal_R = 0;
  DevBuf flat[4], pfl, sky, lin[4], dark_sci, dark_err, zero_read;
  bool has_flat = false, has_pfl = false, has_sky = false, has_lin = false, has_dark = false,
       has_zero = false;
  float sky_max = 0.f, sky_min = 0.f;                            // range of the positive master sky pixels
  std::vector<float> sky_sorted;                                 // those pixels in ascending order (levels = quantiles)
  // host time of wayne_exposure_upload by part, microseconds (printed at destroy when WAYNE_UPLOAD_TIMING is set)
  double up_us[6] = {0, 0, 0, 0, 0, 0};
  long up_calls = 0;
  Slot slots[kSlots];
  // psf_apply scratch
  DevBuf pa_prefix, pa_nwide, pa_nsplit, pa_nlane, pa_x, pa_y, pa_sl, pa_sh, pa_sub, pa_frame;
  StageArena pa_stage;          // every input array of a call, copied to the device in one piece (the arrays above but pa_frame are views into it)
  // profiling
  bool prof_on = false;
  unsigned prof_mask = ~0u;   // kernels timed while prof_on (wayne_profile_select)
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  uint64_t prof_launches[kProfKernels] = {0};
  double prof_ms[kProfKernels] = {0};
  uint64_t electrons = 0;  // thrown through wayne_psf_apply (host-counted)
  uint64_t profile_uploads = 0;   // profiles wayne_exposure_set_optimal_profile copied to the device (not those a slot already held)
  DevBuf trap_state;       // [S*S][2] float32, (slow, fast) per bordered pixel: what k_ramp_hist carries from exposure to exposure
  bool trap_state_valid = false;   // reset or uploaded for this calibration's S
  uint64_t reruns = 0;     // exposures run a second time because a bin lay beyond what the first launch sequence handles
  DevBuf counters;         // kCounterStripes u64 words, 128 B apart: electrons thrown by exposures (device-counted,
                           // count_electrons); word [1]: a spare for debug_fetch's own k_prep_sub launch
};

namespace {

// k_lane's batches and its first-touch flush list of one source (knobs `batch` / `thin` applied)
void plan_lanes(const wayne_ctx* c, SourceState& ss, int K, int W) {
  int kb = 1;
  plan::lane_batches(K, W, ss.max_chunk_electrons, &kb, &ss.thin);
  {   // a knob that is set overrules the planner
    if (c->knobs.batch >= 0) kb = (int)std::min<long long>(std::max<long long>(c->knobs.batch, 1), kLaneBatchMax);
    if (c->knobs.thin >= 0) ss.thin = c->knobs.thin != 0;
  }
  ss.kb = kb;
}

// Scratch of one source for K sub-samples of W bins: per bin, per (sub-sample, bin), per sub-sample, per k_prep_sub chunk.
int reserve_source(wayne_ctx* c, SourceState& ss, int K, int W) {
  const size_t KW = (size_t)K * W, n_chunks = (size_t)(W + kPrepThreads - 1) / kPrepThreads;
  for (DevBuf* b : {&ss.ratio, &ss.sigl, &ss.sigh, &ss.sens, &ss.dlam}) HIP_TRY(c, b->reserve((size_t)W * sizeof(double)));
  for (DevBuf* b : {&ss.counts, &ss.nwide, &ss.nsplit, &ss.nlane}) HIP_TRY(c, b->reserve(KW * sizeof(int32_t)));
  HIP_TRY(c, ss.prefix.reserve((size_t)K * (W + 1) * sizeof(uint32_t)));
  HIP_TRY(c, ss.xpos.reserve(KW * sizeof(double)));
  HIP_TRY(c, ss.ypos.reserve(KW * sizeof(double)));
  HIP_TRY(c, ss.sub.reserve((size_t)K * sizeof(SubInfo)));
  HIP_TRY(c, ss.chunk_total.reserve(K * n_chunks * sizeof(uint32_t)));
  HIP_TRY(c, ss.chunk_box.reserve(K * n_chunks * 4 * sizeof(double)));
  return WAYNE_OK;
}

// ... and its launch plan: what plan::estimate_thrown worked out for its inputs, and k_lane's batches
void adopt_plan(const wayne_ctx* c, SourceState& ss, int K, int W, const plan::ThrowPlan& tp) {
  ss.est_thrown = tp.est_thrown; ss.max_chunk_electrons = tp.max_chunk_electrons; ss.max_narrow = tp.max_narrow;
  std::memcpy(ss.chunk_order, tp.chunk_order, sizeof ss.chunk_order);
  std::memcpy(ss.lane_order, tp.lane_order, sizeof ss.lane_order);
  plan_lanes(c, ss, K, W);
}

int fail(wayne_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

hipEvent_t get_event(wayne_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

struct ProfScope {
  wayne_ctx* c;
  ProfRec rec{};
  bool on;
  bool ext = false;
  // ext_launch: for a single launch through hipExtLaunchKernel: the events then carry the kernel's own start and stop
  // times (no marker packets before and after it in the stream).
  ProfScope(wayne_ctx* c_, int kernel, bool ext_launch = false) : c(c_), on(c_->prof_on && ((c_->prof_mask >> kernel) & 1u)) {
    if (!on) return;
    rec.kernel = kernel;
    rec.a = get_event(c);
    rec.b = get_event(c);
    if (!rec.a || !rec.b) { on = false; return; }
    ext = ext_launch;
    if (!ext) (void)hipEventRecord(rec.a, c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    if (!ext) (void)hipEventRecord(rec.b, c->stream);
    c->prof.push_back(rec);
  }
};

int sync_all(wayne_ctx* c) {
  for (int i = 0; i < kStreams; ++i) {
    HIP_TRY(c, hipStreamSynchronize(c->streams[i]));
    if (c->side[i]) HIP_TRY(c, hipStreamSynchronize(c->side[i]));
  }
  return WAYNE_OK;
}

// slot-based calls work on the slot's stream; everything else on stream 0
void use_slot_stream(wayne_ctx* c, int slot) { c->stream = c->streams[slot % c->n_streams]; }

int collect_profile(wayne_ctx* c) {
  int rc = sync_all(c);
  if (rc) return rc;
  for (ProfRec& r : c->prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->prof_ms[r.kernel] += ms;
      c->prof_launches[r.kernel] += 1;
    }
    c->ev_pool.push_back(r.a);
    c->ev_pool.push_back(r.b);
  }
  c->prof.clear();
  return WAYNE_OK;
}

template <class T>
int upload(wayne_ctx* c, DevBuf& b, const T* src, size_t n) {
  HIP_TRY(c, b.reserve(std::max<size_t>(n, 1) * sizeof(T)));
  if (n) HIP_TRY(c, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return WAYNE_OK;
}

// (the launch planner -- spectrum estimates, accumulator boxes, sky levels and alias tables -- is host_plan.h: host-only
// code that the CPU harness under tests/native builds with sanitizers)
using plan::build_sky_alias;

// Copy `n` elements of the descriptor into the slot's staging arena.
template <class T>
int upload_staged(wayne_ctx* c, Slot& s, DevBuf& b, const T* src, size_t n) {
  if (!s.stage.put(b, src, n * sizeof(T))) return fail(c, WAYNE_E_NOMEM, "upload: staging arena too small");
  return WAYNE_OK;
}

// The per-wavelength arrays of a source whose grid `wl_um` (W doubles, already on its way into ss.wl on the slot's stream)
// has just been uploaded: kept if they are the ones of this grid under this grism (plan::WlCache), else worked out now,
// on the slot's stream -- no run of the slot launches k_prep_wl.
int prepare_wl_arrays(wayne_ctx* c, SourceState& ss, int W, const double* wl_um) {
  if (ss.wl_cache.holds(W, wl_um, c->grism_gen)) return WAYNE_OK;
  ss.wl_cache.drop();
  WlArrays wa{ss.ratio.as<double>(), ss.sigl.as<double>(), ss.sigh.as<double>(), ss.sens.as<double>(), ss.dlam.as<double>()};
  {
    ProfScope ps(c, PK_PREP_WL);
    hipLaunchKernelGGL(k_prep_wl, dim3((W + 255) / 256), dim3(256), 0, c->stream, c->g, W, ss.wl.as<double>(), wa);
    HIP_TRY(c, hipGetLastError());
  }
  ss.wl_cache.adopt(W, wl_um, c->grism_gen);
  return WAYNE_OK;
}

// Plan the sky draws of an exposure (plan::plan_sky) and upload the alias tables it names on the slot's stream with
// the descriptor -- long before k_ramp needs them.
int prepare_sky_tables(wayne_ctx* c, Slot& s) {
  const wayne_exposure_desc& d = s.d;
  plan::SkyPlan sp;
  plan::plan_sky(d.sky_ct_s, s.R, s.read_dt_host.data(), c->has_sky, c->sky_min, c->sky_max, c->sky_sorted, &sp);
  s.sky_pieces = sp.pieces; s.sky_alias_on = false; s.sky_mask = 0; s.sky_L = 1;
  for (int l = 0; l < 16; ++l) { s.sky_level[l] = sp.level[l]; s.sky_tab0[l] = sp.tab0[l]; }
  if (!sp.alias_on) { s.sky_pieces = false; return WAYNE_OK; }    // (no sky, or a read whose rates fit no table: the direct sampler)
  if (sp.keys != s.sky_tab_keys || !s.sky_tab.p) {
    const size_t bytes = (size_t)kMaxReads * kSkyAlias * sizeof(uint32_t);
    int rc = s.sky_stage.begin(c, bytes, "upload: pinned allocation for the sky tables failed");
    if (rc) return rc;
    uint32_t* tab = (uint32_t*)s.sky_stage.place(s.sky_tab, bytes);
    std::memset(tab, 0, bytes);
    for (size_t t = 0; t < sp.keys.size() && t < (size_t)kMaxReads; ++t) {
      // (a table is ~1 us to build -- no cache: the sky level, and with it every rate, changes with the exposure)
      float lam;
      std::memcpy(&lam, &sp.keys[t], 4);
      build_sky_alias((double)lam, tab + t * kSkyAlias);
    }
    if ((rc = s.sky_stage.commit(c, c->stream))) return rc;
    s.sky_tab_keys = sp.keys;
  }
  s.sky_alias_on = true;
  s.sky_mask = sp.mask;
  s.sky_L = sp.L;
  return WAYNE_OK;
}

int side_of(int subarray) { return subarray == 1024 ? 1014 : subarray; }  // detector.py:116-119

// N*N plane -> S*S bordered layout (value `fill` on the 5-px border)
std::vector<float> embed(const float* src, int N, int S, float fill) {
  std::vector<float> v((size_t)S * S, fill);
  for (int y = 0; y < N; ++y)
    std::memcpy(&v[(size_t)(y + kBorder) * S + kBorder], src + (size_t)y * N, (size_t)N * sizeof(float));
  return v;
}

// LDS ints of a thrower workgroup's tile.  A workgroup covers 1/splits of a sub-sample's electrons,
// i.e. a slice of the trace (first-order spectra are < ~260 px long) plus the PSF margin on each
// side, by (margin on each side + the trace's small tilt) rows.  Knob `tile_ints` overrides.
int thrower_lds_ints(const wayne_ctx* c, int splits, int margin) {
  if (c->knobs.tile_ints >= 0) return (int)std::min<long long>(std::max<long long>(c->knobs.tile_ints, 256), 40000);
  const long long w = 260 / std::max(splits, 1) + 2 * margin + 4, h = 2 * margin + 12;
  return (int)std::min<long long>(std::max<long long>(w * h, 1024), 12288);   // <= 48 KiB
}

template <int RNG, int FLUSH>
int launch_throw(wayne_ctx* c, const ThrowArgs& a, int lds_ints) {
  const int groups = (a.K + 7) / 8;
  const dim3 grid((unsigned)(a.K < 8 ? a.K * a.splits : groups * 8 * a.splits));   // (k_throw: block -> (sub-sample, split))
  const size_t lds = (size_t)lds_ints * sizeof(int);
  HIP_TRY(c, hipFuncSetAttribute((const void*)k_throw<RNG, FLUSH>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_throw<RNG, FLUSH>), grid, dim3(kThrowThreads), lds, c->stream, a);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

template <int FLUSH>
int launch_narrow(wayne_ctx* c, const ThrowArgs& a, bool exact) {
  const dim3 grid((unsigned)a.K, (unsigned)((a.W + kNarrowThreads - 1) / kNarrowThreads));
  const bool compact = c->knobs.narrow_compact != 0;   // (knob narrow_compact: the same frames either way)
  void (*kern)(ThrowArgs) = exact ? (compact ? k_narrow<FLUSH, false, true> : k_narrow<FLUSH, false, false>)
                                  : (compact ? k_narrow<FLUSH, true, true> : k_narrow<FLUSH, true, false>);
  hipLaunchKernelGGL(kern, grid, dim3(kNarrowThreads), 0, c->stream, a);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

// The reads' sample type of a descriptor: 0 float32, 1 float64 (WAYNE_F_OUT_F64), 2 uint16 (WAYNE_F_OUT_U16), and its
// size -- the one place the read buffers are sized from
int out_kind(uint32_t flags) { return (flags & WAYNE_F_OUT_F64) ? 1 : (flags & WAYNE_F_OUT_U16) ? 2 : 0; }
size_t out_elem_size(uint32_t flags) {
  const int k = out_kind(flags);
  return k == 1 ? sizeof(double) : k == 2 ? sizeof(uint16_t) : sizeof(float);
}

// The ramp kernels are templates on <reads' type, production / exact math, sky sampler, gaussian-noise stage>, in three
// families: k_ramp / k_ramp_wide, k_ramp_trap for a slot with charge traps, k_ramp_hist for one with a carried history on
// top of them.  ramp_variant names one instantiation of a family; pick_ramp is the descent over the four switches,
// written once.  (The ALLON instantiations are not on the ladder: select_ramp, pick_ramp_trap and pick_ramp_hist name them.)
typedef void (*RampTrapKernel)(RampArgs, TrapArgs);
typedef void (*RampHistKernel)(RampArgs, TrapArgs, TrapHistArgs);
enum RampFamily { RAMP, RAMP_TRAP, RAMP_HIST };
template <RampFamily F, class OutT, bool FAST, int SKY, bool NOISE>
auto ramp_variant() {
  if constexpr (F == RAMP_TRAP) return RampTrapKernel(k_ramp_trap<OutT, FAST, SKY, NOISE, false>);
  else if constexpr (F == RAMP_HIST) return RampHistKernel(k_ramp_hist<OutT, FAST, SKY, NOISE, false>);
  // (pinned to 8 waves per SIMD where that does not spill: see k_ramp / k_ramp_wide)
  else if constexpr (FAST && SKY != 0 && !NOISE) return (void (*)(RampArgs))k_ramp<OutT, FAST, SKY, NOISE>;
  else return (void (*)(RampArgs))k_ramp_wide<OutT, FAST, SKY, NOISE>;
}
template <RampFamily F, class OutT, bool FAST, int SKY>
auto ramp_noise(bool noise) { return noise ? ramp_variant<F, OutT, FAST, SKY, true>() : ramp_variant<F, OutT, FAST, SKY, false>(); }
template <RampFamily F, class OutT, bool FAST>
auto ramp_sky(int sky, bool noise) {
  return sky == 1 ? ramp_noise<F, OutT, FAST, 1>(noise) : sky == 2 ? ramp_noise<F, OutT, FAST, 2>(noise) : ramp_noise<F, OutT, FAST, 0>(noise);
}
// (reads' type: 0 float, 1 double, 2 uint16_t -- out_kind())
template <RampFamily F>
auto pick_ramp(int out, bool exact, int sky, bool noise) {
  return out == 1 ? (exact ? ramp_sky<F, double, false>(sky, noise) : ramp_sky<F, double, true>(sky, noise))
       : out == 2 ? (exact ? ramp_sky<F, uint16_t, false>(sky, noise) : ramp_sky<F, uint16_t, true>(sky, noise))
                  : (exact ? ramp_sky<F, float, false>(sky, noise) : ramp_sky<F, float, true>(sky, noise));
}

// k_lane's tile reach in sigmas (knob lane_tight_tile: the same frames either way -- an electron beyond the tile takes
// the global path)
float lane_reach_sigmas(const wayne_ctx* c) { return c->knobs.lane_tight_tile != 0 ? kLaneR16 : kLaneR34; }

template <int FLUSH>
int launch_lane(wayne_ctx* c, const ThrowArgs& a, bool thin, const PrepArgs* fused_prep = nullptr, const CosmicArgs* fused_cosmic = nullptr) {
  const dim3 grid((unsigned)((a.K + a.kb - 1) / a.kb), (unsigned)((a.W + kLaneThreads - 1) / kLaneThreads));
  if (fused_prep) {
    hipLaunchKernelGGL((k_lane_fused<FLUSH>), grid, dim3(kLaneThreads), 0, c->stream, a, *fused_prep, *fused_cosmic);
  } else if (a.kb > 1) {
    if (thin) hipLaunchKernelGGL((k_lane<FLUSH, true, true>), grid, dim3(kLaneThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_lane<FLUSH, false, true>), grid, dim3(kLaneThreads), 0, c->stream, a);
  } else {
    if (thin) hipLaunchKernelGGL((k_lane<FLUSH, true, false>), grid, dim3(kLaneThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((k_lane<FLUSH, false, false>), grid, dim3(kLaneThreads), 0, c->stream, a);
  }
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}


// k_lane<FLUSH, false, false> and k_narrow<FLUSH, true, true> of one source as ONE grid (k_thrower): used when both
// kernels would be launched on the same stream in their production form -- one sub-sample per workgroup, no THIN list,
// fast samplers, compacted chains -- and knob fuse_thrower is not 0.  Any other combination launches the two kernels.
bool fuse_thrower(const wayne_ctx* c, const ThrowArgs& a, bool thin, bool exact) {
  return c->knobs.fuse_thrower != 0 && a.kb == 1 && !thin && !exact && c->knobs.narrow_compact != 0;
}
template <int FLUSH>
int launch_thrower(wayne_ctx* c, const ThrowArgs& a) {
  const int lane_chunks = (a.W + kLaneThreads - 1) / kLaneThreads, narrow_chunks = (a.W + kNarrowThreads - 1) / kNarrowThreads;
  const dim3 grid((unsigned)a.K, (unsigned)(lane_chunks + narrow_chunks));
  hipLaunchKernelGGL((k_thrower<FLUSH>), grid, dim3(kLaneThreads), 0, c->stream, a, lane_chunks);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

// k_ramp_trap<reads' type, production / exact math, sky sampler, gaussian-noise stage, every switch on>
RampTrapKernel pick_ramp_trap(int out, bool exact, int sky, bool noise, bool allon) {
  if (allon) return out == 2 ? k_ramp_trap<uint16_t, true, 1, false, true> : k_ramp_trap<float, true, 1, false, true>;
  return pick_ramp<RAMP_TRAP>(out, exact, sky, noise);
}
// k_ramp_hist<...>: k_ramp_trap's list again, for a slot with a carried history
RampHistKernel pick_ramp_hist(int out, bool exact, int sky, bool noise, bool allon) {
  if (allon) return out == 2 ? k_ramp_hist<uint16_t, true, 1, false, true> : k_ramp_hist<float, true, 1, false, true>;
  return pick_ramp<RAMP_HIST>(out, exact, sky, noise);
}

// The k_ramp instantiation the back half of slot `s` launches, and (if asked) its name as the kernel trace prints it.
// A slot with charge traps launches k_ramp_trap instead: *trap (when given) is then set, else left null; one with a
// carried history on top of them k_ramp_hist: *hist likewise.
void (*select_ramp(const wayne_ctx* c, const Slot& s, std::string* name, RampTrapKernel* trap = nullptr,
                   RampHistKernel* hist = nullptr))(RampArgs) {
  const wayne_exposure_desc& d = s.d;
  const int out = out_kind(d.flags);
  const bool f64 = out == 1, exact = (d.flags & WAYNE_F_EXACT_SAMPLERS) != 0;
  const char* out_name = out == 1 ? "double" : out == 2 ? "unsigned short" : "float";
  const int sky_mode = !s.sky_alias_on ? 0 : (s.sky_pieces ? 2 : 1);
  const bool noise = d.noise_mean != 0. && d.noise_std != 0.;
  void (*kern)(RampArgs) = pick_ramp<RAMP>(out, exact, sky_mode, noise);
  // the production variant with every detector switch on (the rule) has an instantiation of its own (k_ramp.h, ALLON)
  const uint32_t all_on = WAYNE_F_ADD_DARK | WAYNE_F_ADD_NON_LINEAR | WAYNE_F_CLIP_DET_LIMITS | WAYNE_F_ADD_READ_NOISE;
  const bool allon = !f64 && !exact && sky_mode == 1 && !noise && (d.flags & all_on) == all_on && c->has_dark && c->has_lin;
  if (allon) kern = out == 2 ? k_ramp<uint16_t, true, 1, false, true> : k_ramp<float, true, 1, false, true>;
  const bool with_hist = s.traps_on && s.hist_on;
  if (trap) *trap = s.traps_on && !with_hist ? pick_ramp_trap(out, exact, sky_mode, noise, allon) : nullptr;
  if (hist) *hist = with_hist ? pick_ramp_hist(out, exact, sky_mode, noise, allon) : nullptr;
  if (name) {
    const bool pinned = !exact && sky_mode != 0 && !noise;      // ramp_variant(): k_ramp where it fits 64 registers, else k_ramp_wide
    char buf[96];
    if (s.traps_on)
      std::snprintf(buf, sizeof buf, "%s<%s, %s, %d, %s, %s>", with_hist ? "k_ramp_hist" : "k_ramp_trap", out_name,
                    exact ? "false" : "true", sky_mode, noise ? "true" : "false", allon ? "true" : "false");
    else
      std::snprintf(buf, sizeof buf, "%s<%s, %s, %d, %s%s>", pinned ? "k_ramp" : "k_ramp_wide", out_name,
                    exact ? "false" : "true", sky_mode, noise ? "true" : "false", pinned ? (allon ? ", true" : ", false") : "");
    *name = buf;
  }
  return kern;
}

static_assert(WAYNE_MAX_CHANNELS == kChanMaxChannels && WAYNE_MAX_CHANNEL_HULL == kChanMaxHull && WAYNE_C_FLAT == C_FLAT,
              "include/wayne_hip.h and plan_consts.h must agree on the channels' caps and flag");

// The kernels of an exposure's reads are templates on the reads' type and on a few switches.  with_reads calls f with a
// tag of the type for out_kind(flags), with_flag with std::true_type / std::false_type: the branches are written here only.
template <class T> struct Reads { using type = T; };
template <class F> void with_reads(int out, F&& f) {
  if (out == 1) f(Reads<double>{});
  else if (out == 2) f(Reads<uint16_t>{});
  else f(Reads<float>{});
}
template <class F> auto with_flag(bool on, F&& f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

// A region of slot `s`'s spectra block on the device (s.lay: plan::spectra_layout).
double* ex_region(const Slot& s, size_t offset) { return (double*)((char*)s.ex_out.p + offset); }

// The channels of slot `s` (wayne_exposure_set_channels) behind k_extract_finish, from `a` as launch_extract filled it.
ChannelArgs channel_args(const wayne_ctx* c, const Slot& s) {
  ChannelArgs ch{};
  ch.C = s.ch_C; ch.u_lo = s.ch_lo; ch.u_hi = s.ch_hi;
  ch.flat = (s.ch_flags & C_FLAT) && c->has_flat;
  ch.N = c->S - 2 * kBorder;
  ch.flat_wmin = c->g.flat_wmin; ch.flat_wmax = c->g.flat_wmax;
  ch.edges = s.ch_edges.as<double>(); ch.wl_a = s.ch_wa.as<double>(); ch.wl_b = s.ch_wb.as<double>();
  for (int i = 0; i < 4; ++i) ch.cube[i] = c->has_flat ? c->flat[i].as<float>() : nullptr;
  return ch;
}

// The optimal channels of slot `s` (wayne_exposure_set_optimal_channels) behind k_extract_optimal_finish, from `a`, `o` and
// `f` as launch_optimal filled them.
template <bool CR>
int launch_optimal_channels(wayne_ctx* c, Slot& s, const ExtractArgs& a, const OptimalArgs& o, const ProfileArgs& f, int blocks, int out) {
  const ChannelArgs ch = channel_args(c, s);
  OptChanArgs oc{};
  oc.part = s.optch_part.as<double>();
  oc.channels_opt = ex_region(s, s.lay.channels_opt);
  oc.channels_opt_var = ex_region(s, s.lay.channels_opt_var);
  const dim3 grid((unsigned)blocks, (unsigned)kChanGroups), block(kExtractThreads);
  if (blocks > 0) {
    with_reads(out, [&](auto t) {
      with_flag(s.prof_fixed, [&](auto fixed) {
        hipLaunchKernelGGL((k_extract_bins_opt<typename decltype(t)::type, CR, decltype(fixed)::value>), grid, block, 0, c->stream,
                           a, ch, o, f, oc);
      });
    });
    HIP_TRY(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_extract_bins_opt_finish, dim3((unsigned)(a.R + 1)), dim3(kChanMaxChannels), 0, c->stream, a, ch, oc);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

template <bool CR, bool VAR>
int launch_channels(wayne_ctx* c, Slot& s, const ExtractArgs& a, int blocks, int out) {
  ChannelArgs ch = channel_args(c, s);
  ch.part = s.ch_part.as<double>();
  ch.channels = ex_region(s, s.lay.channels);
  if (VAR) {
    ch.part_v = s.ch_part_v.as<double>();
    ch.channels_var = ex_region(s, s.lay.channels_var);
  }
  const dim3 grid((unsigned)blocks, (unsigned)kChanGroups), block(kExtractThreads);
  if (blocks > 0) {
    with_reads(out, [&](auto t) {
      hipLaunchKernelGGL((k_extract_bins<typename decltype(t)::type, CR, VAR>), grid, block, 0, c->stream, a, ch);
    });
    HIP_TRY(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_extract_bins_finish<VAR>, dim3((unsigned)(a.R + 1)), dim3(kChanMaxChannels), 0, c->stream, a, ch);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

static_assert(WAYNE_MAX_OPTIMAL_HALF_WIDTH == kOptMaxH, "include/wayne_hip.h and plan_consts.h must agree on the widest profile");

// The optimal extraction of slot `s` (wayne_exposure_set_optimal) behind k_extract_finish, from `a` as launch_extract
// filled it: k_extract_optimal on the grid of k_extract_rows, then one workgroup per product.
template <bool CR>
int launch_optimal(wayne_ctx* c, Slot& s, const ExtractArgs& a, dim3 grid, int out) {
  OptimalArgs o{};
  o.H = s.opt_H;
  o.part = s.opt_part.as<double>();
  o.optimal = ex_region(s, s.lay.optimal);
  o.optimal_var = ex_region(s, s.lay.optimal_var);
  const dim3 block(kExtractThreads);
  ProfileArgs f{};
  const size_t planes_n = plan::profile_offsets(a.S, a.R, a.steps, a.row_lo, a.row_hi, f.row_off);
  f.planes = s.prof_deliver ? s.prof_planes.as<double>() : nullptr;
  f.fixed = s.prof_fixed ? s.prof_fix.as<double>() : nullptr;
  if (s.prof_deliver) {
    // S1 of every window pixel; a product that is not formed (the last read, switched off) delivers zeros
    if (!(a.steps & X_LAST_READ))
      HIP_TRY(c, hipMemsetAsync(f.planes + f.row_off[a.R], 0, (planes_n - f.row_off[a.R]) * sizeof(double), c->stream));
    if (grid.y > 0) {
      with_reads(out, [&](auto t) {
        hipLaunchKernelGGL((k_extract_profile<typename decltype(t)::type, CR>), grid, block, 0, c->stream, a, o, f);
      });
      HIP_TRY(c, hipGetLastError());
    }
    s.prof_valid = true;
    s.prof_fetched = false;          // (a copy fetched before this run holds the run before)
  }
  if (grid.y > 0) {
    with_reads(out, [&](auto t) {
      using T = typename decltype(t)::type;
      if (s.prof_fixed) hipLaunchKernelGGL((k_extract_optimal_fixed<T, CR>), grid, block, 0, c->stream, a, o, f);
      else hipLaunchKernelGGL((k_extract_optimal<T, CR>), grid, block, 0, c->stream, a, o);
    });
    HIP_TRY(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_extract_optimal_finish, dim3((unsigned)(a.R + 1)), block, 0, c->stream, a, o);
  HIP_TRY(c, hipGetLastError());
  return s.optch_on ? launch_optimal_channels<CR>(c, s, a, o, f, (int)grid.y, out) : WAYNE_OK;
}

// The launches of launch_extract, which filled `a`: with rejection the flag plane first, then the row sums of every
// product, the chunks added up, and behind them the optimal extraction and the channels.
template <bool CR, bool VAR>
int launch_extract_as(wayne_ctx* c, Slot& s, const ExtractArgs& a, int products, int out) {
  const dim3 grid((unsigned)((a.S + 63) / 64), (unsigned)a.first_chunk[products]);
  const dim3 block(kExtractThreads);
  if (CR) {
    // tiles of the mask rows
    const dim3 tiles((unsigned)((a.S + kCrTileCols - 1) / kCrTileCols), (unsigned)((a.m_hi - a.m_lo + kCrTileRows - 1) / kCrTileRows));
    with_reads(out, [&](auto t) { hipLaunchKernelGGL((k_extract_crmask<typename decltype(t)::type>), tiles, block, 0, c->stream, a); });
    HIP_TRY(c, hipGetLastError());
  }
  with_reads(out, [&](auto t) {
    hipLaunchKernelGGL((k_extract_rows<typename decltype(t)::type, CR, VAR>), grid, block, 0, c->stream, a);
  });
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL((k_extract_finish<CR, VAR>), dim3((unsigned)(a.R + 1)), block, 0, c->stream, a);
  HIP_TRY(c, hipGetLastError());
  if (s.opt_on)
    if (int rc = launch_optimal<CR>(c, s, a, grid, out)) return rc;
  return s.chan_on ? launch_channels<CR, VAR>(c, s, a, a.first_chunk[products], out) : WAYNE_OK;
}

// The extraction of slot `s` (wayne_exposure_set_extraction) behind its ramp kernel: the row sums of every product, then
// the chunks added up, the sky level and the spectra.  The grid follows from the plan alone.
int launch_extract(wayne_ctx* c, Slot& s) {
  const int S = c->S, R = s.R;
  ExtractArgs a{};
  a.R = R; a.S = S;
  a.steps = s.ex.steps;
  a.bg_lo = s.ex.bg_col_lo; a.bg_hi = s.ex.bg_col_hi;
  a.n_chunks = s.ex_chunks;
  double sum_dt = 0.;
  for (int j = 0; j < R; ++j) { a.scale[j] = s.read_dt_host[j]; sum_dt += s.read_dt_host[j]; }
  a.scale[R] = sum_dt;
  for (int j = 0; j <= R; ++j) { a.row_lo[j] = s.ex.row_lo[j]; a.row_hi[j] = s.ex.row_hi[j]; }
  a.reads = s.out.p;
  a.pfl = c->has_pfl ? c->pfl.as<float>() : nullptr;
  a.sky = c->has_sky ? c->sky.as<float>() : nullptr;
  for (int i = 0; i < 4; ++i) a.lin[i] = c->has_lin ? c->lin[i].as<float>() : nullptr;
  a.dark = c->has_dark ? c->dark_sci.as<float>() : nullptr;
  a.part = s.ex_part.as<double>();
  a.spectra = ex_region(s, s.lay.spectra);
  a.sky_out = ex_region(s, s.lay.sky);
  if (s.crrej_on) {
    a.mask = s.cr_mask.as<uint16_t>();
    a.part_n = s.ex_part_n.as<unsigned>();
    a.n_rej = (unsigned*)ex_region(s, s.lay.n_rejected);
    a.m_lo = s.cr_lo; a.m_hi = s.cr_hi;
    a.k2 = s.cr_k * s.cr_k; a.rn2 = s.cr_rn * s.cr_rn;
  }
  if (s.var_on) {
    a.vrn2 = s.var_rn * s.var_rn;
    a.part_v = s.ex_part_v.as<double>();
    a.spectra_var = ex_region(s, s.lay.spectra_var);
    a.sky_var = ex_region(s, s.lay.sky_var);
  }
  const int products = (a.steps & X_LAST_READ) ? R + 1 : R;
  for (int p = 0; p <= kExtractProducts; ++p) a.first_chunk[p] = 0;
  for (int p = 0; p < products; ++p)
    a.first_chunk[p + 1] = a.first_chunk[p] + (a.row_hi[p] - a.row_lo[p] + kExtractRows - 1) / kExtractRows;
  for (int p = products; p < kExtractProducts; ++p) a.first_chunk[p + 1] = a.first_chunk[p];
  ProfScope ps(c, PK_EXTRACT);
  const int out = out_kind(s.d.flags);
  return with_flag(s.crrej_on, [&](auto cr) {
    return with_flag(s.var_on, [&](auto var) {
      return launch_extract_as<decltype(cr)::value, decltype(var)::value>(c, s, a, products, out);
    });
  });
}

// The layout of a slot's FITS payload (wayne_fits_layout): false for a side or a flag word it is not defined for.
bool fits_layout(int S, int R, uint32_t flags, size_t* plane_bytes, size_t* stride, int* bitpix) {
  if (S < 2 || (S & 1) || R < 1 || ((flags & WAYNE_F_OUT_F64) && (flags & WAYNE_F_OUT_U16))) return false;
  const size_t B = (flags & WAYNE_F_OUT_U16) ? 2 : 8;
  const size_t pb = (size_t)S * S * B;
  if (plane_bytes) *plane_bytes = pb;
  if (stride) *stride = (pb + kFitsBlock - 1) / kFitsBlock * kFitsBlock;
  if (bitpix) *bitpix = (flags & WAYNE_F_OUT_U16) ? 16 : -64;
  return true;
}

// The FITS words of slot `s` (wayne_exposure_set_fits) behind its ramp kernel -- and behind the extraction's launches,
// which so stay where they are without the option, directly behind the kernel whose reads they take: one launch,
// grid (units of a plane, capped; R + 1 planes).
int launch_fits(wayne_ctx* c, Slot& s) {
  FitsArgs a{};
  a.reads = s.out.p;
  a.payload = s.fits_dev.as<unsigned char>();
  a.planes = s.R + 1;
  a.n = (unsigned)((size_t)c->S * c->S);
  a.stride = s.fits_stride;
  const int out = out_kind(s.d.flags);
  const size_t units = s.fits_stride / (out == 2 ? 16 : 32);
  const size_t cap = std::max<size_t>(1, (size_t)kFitsMaxBlocks / (size_t)a.planes);
  const dim3 grid((unsigned)std::min(cap, (units + kFitsThreads - 1) / kFitsThreads), (unsigned)a.planes), block(kFitsThreads);
  ProfScope ps(c, PK_FITS);
  with_reads(out, [&](auto t) { hipLaunchKernelGGL((k_fits_words<typename decltype(t)::type>), grid, block, 0, c->stream, a); });
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

// The expected image of slot `s` (wayne_exposure_set_expected), at the very end of the back half: the plane cleared, then
// one k_expect launch per source, each adding into it -- on the slot's stream, so in list order.  A source's launch takes
// k_prep_sub's arguments of THIS run (SourceState::last_prep, kept by front_source whether or not k_prep_sub was launched):
// the kernel plans its bins itself, with plan_bin, from the same inputs.  The boxes come from the host copies of the
// source's wavelengths, star positions and trace coefficients, which its staging arena holds until the next upload.
int launch_expected(wayne_ctx* c, Slot& s) {
  const int R = s.R, K = s.K, N = c->N, S = c->S;
  ProfScope ps(c, PK_EXPECT);
  HIP_TRY(c, hipMemsetAsync(s.expect_plane.p, 0, (size_t)R * S * S * sizeof(double), c->stream));
  const int32_t* sread = s.stage.host_of<int32_t>(s.sread);
  for (int i = 0; i <= s.n_extra; ++i) {
    SourceState& ss = s.source(i);
    const StageArena& st = i == 0 ? s.stage : ss.src_stage;
    ExpectArgs e{};
    e.R = R; e.S = S;
    e.plane = s.expect_plane.as<double>();
    plan::expected_boxes(c->g, ss.W, st.host_of<double>(ss.wl), K, R, N, s.d.sub_scale, st.host_of<double>(ss.xref),
                         st.host_of<double>(ss.yref), st.host_of<double>(ss.tr), sread, e.box);
    int tiles = 0;
    for (int r = 0; r < R; ++r) {
      const int* b = e.box[r];
      if (b[0] >= b[1] || b[2] >= b[3]) continue;
      tiles = std::max(tiles, ((b[1] - b[0] + kExpectTW - 1) / kExpectTW) * ((b[3] - b[2] + kExpectTH - 1) / kExpectTH));
    }
    if (tiles == 0) continue;      // the source reaches no pixel of the frame
    // what flat_value reads of a thrower's arguments (front_source)
    ThrowArgs t{};
    t.W = ss.W; t.K = K; t.N = N; t.S = S;
    t.flags = s.d.flags;
    t.flat_off = s.d.sub_scale;
    t.flat_wmin = c->g.flat_wmin; t.flat_wmax = c->g.flat_wmax;
    t.flat_inv_range = 1.0 / (c->g.flat_wmax - c->g.flat_wmin);
    for (int j = 0; j < 4; ++j) t.flat[j] = c->has_flat ? c->flat[j].as<float>() : nullptr;
    const dim3 grid((unsigned)tiles, (unsigned)R), block(kExpectThreads);
    if (s.expect_mode == WAYNE_EXPECT_COUNTS) hipLaunchKernelGGL(k_expect<1>, grid, block, 0, c->stream, ss.last_prep, t, e);
    else hipLaunchKernelGGL(k_expect<2>, grid, block, 0, c->stream, ss.last_prep, t, e);
    HIP_TRY(c, hipGetLastError());
  }
  return WAYNE_OK;
}

static_assert(WAYNE_X_LINEARISE == X_LINEARISE && WAYNE_X_DARK == X_DARK && WAYNE_X_GAIN == X_GAIN,
              "include/wayne_hip.h and plan_consts.h must agree on the step bits");

// The ramp fit of slot `s` (wayne_exposure_set_rampfit) behind its ramp kernel, the extraction's launches and
// k_fits_words: one launch, a thread a pixel of the bordered frame.
int launch_rampfit(wayne_ctx* c, Slot& s) {
  const size_t SS = (size_t)c->S * c->S;
  RampFitArgs a{};
  a.R = s.R; a.S = c->S;
  a.steps = s.rampfit.steps;
  for (int j = 0; j < kMaxReads; ++j) a.dt[j] = j < s.R ? s.read_dt_host[j] : 0.;
  a.rn2 = s.rampfit.read_noise_e * s.rampfit.read_noise_e;
  a.k_jump = s.rampfit.k_jump;
  a.sat_dn = s.rampfit.saturation_dn;
  a.reads = s.out.p;
  a.pfl = c->has_pfl ? c->pfl.as<float>() : nullptr;
  for (int i = 0; i < 4; ++i) a.lin[i] = c->has_lin ? c->lin[i].as<float>() : nullptr;
  a.dark = c->has_dark ? c->dark_sci.as<float>() : nullptr;
  a.rate = s.rampfit_planes.as<double>();
  a.var = a.rate + SS;
  a.word = (uint32_t*)(a.var + SS);
  const dim3 grid((unsigned)((SS + kRampFitThreads - 1) / kRampFitThreads)), block(kRampFitThreads);
  ProfScope ps(c, PK_RAMPFIT);
  with_reads(out_kind(s.d.flags), [&](auto t) { hipLaunchKernelGGL((k_ramp_fit<typename decltype(t)::type>), grid, block, 0, c->stream, a); });
  HIP_TRY(c, hipGetLastError());
  s.rampfit_ran = true;
  return WAYNE_OK;
}

// The calibrated reads of slot `s` (wayne_exposure_set_ima) behind its ramp fit, whose word of this run they read when
// the slot has one: one launch, a lane a unit of 8 pixels of every imset, the grid capped and strided over.
int launch_ima(wayne_ctx* c, Slot& s) {
  const size_t SS = (size_t)c->S * c->S;
  ImaArgs a{};
  a.R = s.R; a.S = c->S;
  a.n = (unsigned)SS;
  a.steps = s.ima.steps;
  a.rate = s.ima.units == WAYNE_IMA_RATE;
  a.t[0] = 0.;
  for (int k = 1; k <= kMaxReads; ++k) a.t[k] = k <= s.R ? a.t[k - 1] + s.read_dt_host[k - 1] : 0.;
  a.rn2 = s.ima.read_noise_e * s.ima.read_noise_e;
  a.sat_dn = s.ima.saturation_dn;
  a.reads = s.out.p;
  a.pfl = c->has_pfl ? c->pfl.as<float>() : nullptr;
  for (int i = 0; i < 4; ++i) a.lin[i] = c->has_lin ? c->lin[i].as<float>() : nullptr;
  a.dark = c->has_dark ? c->dark_sci.as<float>() : nullptr;
  a.word = s.rampfit_on ? (const uint32_t*)(s.rampfit_planes.as<double>() + 2 * SS) : nullptr;
  a.payload = s.ima_dev.as<unsigned char>();
  a.sci_stride = s.ima_sci_stride; a.dq_stride = s.ima_dq_stride; a.imset_stride = s.ima_imset_stride;
  const size_t units = s.ima_dq_stride / 16;
  const dim3 grid((unsigned)std::min((size_t)kImaMaxBlocks, (units + kImaThreads - 1) / kImaThreads)), block(kImaThreads);
  ProfScope ps(c, PK_IMA);
  with_reads(out_kind(s.d.flags), [&](auto t) { hipLaunchKernelGGL((k_ima<typename decltype(t)::type>), grid, block, 0, c->stream, a); });
  HIP_TRY(c, hipGetLastError());
  s.ima_ran = true;
  return WAYNE_OK;
}

// No extraction on slot `s` (upload, set_extraction): every switch of it off, nothing fetched.  The profile planes and
// the optimal channels go with the optimal extraction wherever that is cleared.
void ex_clear(Slot& s) {
  s.extract_on = s.crrej_on = s.chan_on = s.var_on = s.opt_on = s.optch_on = false;
  s.prof_deliver = s.prof_fetched = s.prof_valid = s.prof_fixed = false;
  s.ex_pinned.misc = nullptr;
  s.ex_base = nullptr;
}

// What every setter of the extraction calls once it has changed its switch: the spectra block's layout follows the
// switches, the device block has room for it, and what was fetched -- it has another layout -- is gone.  Nothing of the
// block is kept: the next run writes all of it.  The room always includes the rejection's counts, so that set_crrej,
// before or after the other setters, never moves the block: DevBuf::reserve frees and allocates when it grows.  Without
// room the slot is left without extraction (the block is gone).
int ex_relayout(wayne_ctx* c, Slot& s) {
  const int C = s.chan_on ? s.ch_C : 0;
  s.lay = plan::spectra_layout(c->S, s.R, s.crrej_on, C, s.var_on, s.opt_on, s.optch_on);
  s.ex_pinned.misc = nullptr;
  s.ex_base = nullptr;
  (void)hipSetDevice(c->device);
  const hipError_t e = s.ex_out.reserve(plan::spectra_layout(c->S, s.R, true, C, s.var_on, s.opt_on, s.optch_on).bytes);
  if (e != hipSuccess) s.extract_on = false;
  HIP_TRY(c, e);
  return WAYNE_OK;
}

// The head of an entry point that takes a slot: the context, the slot number ("<who>: slot") and the upload ("<who>: slot
// not uploaded").  *sp: the slot.  A head that says anything else -- run_back, wait, debug_depth, upload, which needs no
// upload, device_reads, which returns a pointer -- is written out where it stands.
int slot_gate(wayne_ctx* c, int slot, const char* who, Slot** sp) {
  if (!c) return WAYNE_E_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(c, WAYNE_E_INVALID, std::string(who) + ": slot");
  *sp = &c->slots[slot];
  if (!(*sp)->uploaded) return fail(c, WAYNE_E_STATE, std::string(who) + ": slot not uploaded");
  return WAYNE_OK;
}

// What the extraction's entry points may ask of a slot beyond an upload, and the head they share: slot_gate, then the
// switches `need` names, refused as `who`: `missing` -- the words for a slot that is not uploaded either.
enum : unsigned { EX_ON = 1, EX_CRREJ = 2, EX_CHAN = 4, EX_VAR = 8, EX_OPT = 16, EX_OPTCH = 32, EX_PROF = 64 };
int ex_gate(wayne_ctx* c, int slot, const char* who, unsigned need, const char* missing, Slot** sp) {
  const int rc = slot_gate(c, slot, who, sp);
  if (rc && rc != WAYNE_E_STATE) return rc;
  const Slot& s = **sp;
  const unsigned have = (s.extract_on ? EX_ON : 0) | (s.crrej_on ? EX_CRREJ : 0) | (s.chan_on ? EX_CHAN : 0) | (s.var_on ? EX_VAR : 0) |
                        (s.opt_on ? EX_OPT : 0) | (s.optch_on ? EX_OPTCH : 0) | (s.prof_deliver ? EX_PROF : 0);
  if (rc || (need & ~have)) return fail(c, WAYNE_E_STATE, std::string(who) + ": " + missing);
  return WAYNE_OK;
}

// launches and milliseconds of profiled kernel `pk` since wayne_profile_reset (either pointer may be null)
int kernel_profile(wayne_ctx* c, int pk, uint64_t* launches, double* ms) {
  if (!c) return WAYNE_E_INVALID;
  int rc = collect_profile(c);
  if (rc) return rc;
  if (launches) *launches = c->prof_launches[pk];
  if (ms) *ms = c->prof_ms[pk];
  return WAYNE_OK;
}

int PinnedMirror::fetch(wayne_ctx* c, int slot, const void* dev, size_t bytes, bool record_kdone, const char* nomem) {
  const Slot& s = c->slots[slot];
  const size_t tail = align64(bytes);
  misc = nullptr;
  if (!buf.reserve(tail + 64)) return fail(c, WAYNE_E_NOMEM, nomem);
  misc = (SlotMisc*)(buf.p + tail);
  if (record_kdone && c->n_streams == 2 && c->ev_kdone[slot % 2]) {
    HIP_TRY(c, hipEventRecord(c->ev_kdone[slot % 2], c->stream));
    c->kdone_valid[slot % 2] = true;
  }
  HIP_TRY(c, hipMemcpyAsync(buf.p, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(misc, s.misc.p, sizeof(SlotMisc), hipMemcpyDeviceToHost, c->stream));
  run = s.run_no;
  return WAYNE_OK;
}
constexpr const char* kNoExtraction = "no extraction set for the slot";
constexpr const char* kNoOptimal = "no optimal extraction set for the slot";
constexpr const char* kFetchFirst = "wait_spectra or download_spectra first";

}  // namespace

namespace {
bool box_empty(const int* b) { return b[0] >= b[1] || b[2] >= b[3]; }
}  // namespace

extern "C" {

int wayne_abi_version(void) { return WAYNE_ABI_VERSION; }

const char* wayne_strerror(int s) {
  switch (s) {
    case WAYNE_OK: return "ok";
    case WAYNE_E_INVALID: return "invalid argument";
    case WAYNE_E_NEGATIVE: return "negative electron count";
    case WAYNE_E_OVERFLOW: return "electron count overflows the reference's int arithmetic";
    case WAYNE_E_NOMEM: return "out of memory";
    case WAYNE_E_HIP: return "HIP runtime error";
    case WAYNE_E_NODEVICE: return "no gfx950 device";
    case WAYNE_E_STATE: return "grism / calibration / upload missing";
    default: return "unknown status";
  }
}

int wayne_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

wayne_ctx* wayne_ctx_create(int device, int* status) {
  auto set = [&](int s) { if (status) *status = s; };
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
    set(WAYNE_E_NODEVICE);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { set(WAYNE_E_HIP); return nullptr; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set(WAYNE_E_HIP); return nullptr; }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    // the code object holds gfx950 ISA only; there is no other path
    set(WAYNE_E_NODEVICE);
    return nullptr;
  }
  wayne_ctx* c = new (std::nothrow) wayne_ctx();
  if (!c) { set(WAYNE_E_NOMEM); return nullptr; }
  c->device = device;
  for (int i = 0; i < kStreams; ++i)
    if (hipStreamCreateWithFlags(&c->streams[i], hipStreamNonBlocking) != hipSuccess) {
      c->streams[i] = nullptr;
      delete c;
      set(WAYNE_E_HIP);
      return nullptr;
    }
  c->stream = c->streams[0];
  for (int i = 0; i < kStreams; ++i) {
    if (hipEventCreateWithFlags(&c->ev_kdone[i], hipEventDisableTiming) != hipSuccess) c->ev_kdone[i] = nullptr;
    if (hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) != hipSuccess)
      c->fork_narrow = false;     // not fatal: k_narrow then follows k_throw on the main stream
  }
  // k_narrow beside k_lane on a side stream: worth 10 % when the thrower still had idle issue slots
  // (round 1); now each of the two fills the VALU by itself and running them one after the other is as fast
  // (1860 vs 1846 exposures/s on one stream, 2212 vs 2224 on two) -- off unless WAYNE_FORK_NARROW=1
  // the one place the environment is read (see Knobs)
  for (const KnobName& k : kKnobNames)
    if (const char* e = std::getenv(k.env)) c->knobs.*(k.field) = std::max(std::atoll(e), -1LL);
  c->fork_narrow = c->fork_narrow && c->knobs.fork_narrow > 0;
  if (c->knobs.streams >= 0) c->n_streams = (int)std::min<long long>(std::max<long long>(c->knobs.streams, 1), kStreams);
  if (c->counters.reserve(kCounterBytes) != hipSuccess || hipMemset(c->counters.p, 0, kCounterBytes) != hipSuccess ||
      c->status_all.reserve(kSlots * kMiscBytes) != hipSuccess || hipMemset(c->status_all.p, 0, kSlots * kMiscBytes) != hipSuccess ||
      !c->status_host.reserve(kSlots * kMiscBytes)) {
    delete c;
    set(WAYNE_E_NOMEM);
    return nullptr;
  }
  set(WAYNE_OK);
  return c;
}

void wayne_ctx_destroy(wayne_ctx* c) {
  if (!c) return;
  if (c->knobs.upload_timing > 0 && c->up_calls > 0)
    std::fprintf(stderr, "wayne_exposure_upload: %ld calls; us per call: staging + copies %.1f, electron estimate %.1f, "
                 "accumulator boxes %.1f, sky tables %.1f\n", c->up_calls, c->up_us[0] / c->up_calls,
                 c->up_us[1] / c->up_calls, c->up_us[2] / c->up_calls, c->up_us[3] / c->up_calls);
  (void)hipSetDevice(c->device);
  (void)sync_all(c);
  for (ProfRec& r : c->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  delete c;     // the members free what they own; then ~CtxStreams: the streams and their events go last
}

const char* wayne_last_error(const wayne_ctx* c) { return c ? c->err.c_str() : "null context"; }

// The status block of a slot, from the device (the call waits for the slot's stream, c->stream)
static int read_status(wayne_ctx* c, const Slot& s, Slot::Misc* m) {
  HIP_TRY(c, hipMemcpyAsync(m, s.misc.p, sizeof *m, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WAYNE_OK;
}

// Look at the status word of the slot's last run -- in `host_copy` of its status block if the caller has brought one
// back already, else read from the device (read_status).  Bit 0 = overflow: WAYNE_E_OVERFLOW.  Bit 1 = a bin beyond the
// lanes' reach in an exposure launched without k_throw: if the caller names what to run `again` (wayne_exposure_run,
// or wayne_exposure_run_front between the two halves), that is enqueued, now with k_throw, and *reran set -- the caller
// then fetches what it needs a second time and looks again, without `again`.  The one place that re-runs an exposure.
// `run`: the slot's run number when the copy was enqueued (0: the current one -- a read from the device, which waits for
// the stream, or settle's copy, taken with every stream idle).
static int look_at_status(wayne_ctx* c, int slot, const Slot::Misc* host_copy, int (*again)(wayne_ctx*, int) = nullptr,
                          bool* reran = nullptr, uint32_t run = 0) {
  Slot& s = c->slots[slot];
  Slot::Misc m{};
  if (host_copy) m = *host_copy;
  else if (int rc = read_status(c, s, &m)) return rc;
  const uint32_t looked = run ? run : s.run_no;
  if (looked == s.run_no) s.ran = false;   // looked at (a copy that an earlier run left says nothing about the last one: settle still looks)
  const int status = m.bits(looked);
  if (status & 1) return fail(c, WAYNE_E_OVERFLOW, "exposure: a sub-sample holds >= 2^32 electrons (or a bin >= 2^31)");
  if (!(status & 2) || !again) return WAYNE_OK;
  s.force_throw = true;
  c->reruns += 1;
  *reran = true;
  return again(c, slot);
}

// Every slot whose last whole run nobody has looked at yet: read its status word (all of them in ONE copy) and run a
// slot that met a bin beyond its launch sequence's reach a second time, with the general sequence.  Called with all
// streams idle; leaves them idle.  An overflow (bit 0) is reported after the other slots have been settled.
static int settle(wayne_ctx* c) {
  int err = WAYNE_OK;
  for (int pass = 0; pass < 2; ++pass) {
    int hi = -1;
    for (int i = 0; i < kSlots; ++i)
      if (c->slots[i].ran && c->slots[i].uploaded) hi = i;
    if (hi < 0) break;
    HIP_TRY(c, hipMemcpy(c->status_host.p, c->status_all.p, (size_t)(hi + 1) * kMiscBytes, hipMemcpyDeviceToHost));
    const bool may_rerun = pass == 0;     // (the second pass takes a run as it is)
    bool again = false;
    for (int i = 0; i <= hi; ++i) {
      const Slot& s = c->slots[i];
      if (!s.ran || !s.uploaded) continue;
      const int rc = look_at_status(c, i, (const Slot::Misc*)(c->status_host.p + (size_t)i * kMiscBytes),
                                    may_rerun ? wayne_exposure_run : nullptr, &again);
      if (rc == WAYNE_E_OVERFLOW) err = rc;
      else if (rc) return rc;
    }
    if (!again) break;
    int rc = sync_all(c);
    if (rc) return rc;
  }
  return err;
}

}  // extern "C"

namespace {
// A blocking download of slot `slot`, settled: `copy` enqueues the caller's copies on c->stream (the slot's), the status
// word is read behind them, and an exposure that has to be run a second time is, with k_throw -- it is then extracted,
// fitted, calibrated and rendered again -- and copied and looked at once more.  What every wayne_exposure_download* runs,
// and wayne_exposure_run_checked with nothing to copy.  (Whether the slot has been run at all is the caller's to ask:
// download_rampfit and download_ima refuse before a run, download, download_spectra, download_fits and
// download_expected deliver what the buffer holds.)
template <class Copy>
int download_settled(wayne_ctx* c, int slot, Copy&& copy) {
  bool reran = false;
  int rc = copy();
  if (rc || (rc = look_at_status(c, slot, nullptr, wayne_exposure_run, &reran)) || !reran) return rc;
  if ((rc = copy())) return rc;
  return look_at_status(c, slot, nullptr);
}
// ... of one buffer
int download_settled(wayne_ctx* c, int slot, void* dst, const void* dev, size_t bytes) {
  return download_settled(c, slot, [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return WAYNE_OK;
  });
}
}  // namespace

extern "C" {

int wayne_ctx_synchronize(wayne_ctx* c) {
  if (!c) return WAYNE_E_INVALID;
  (void)hipSetDevice(c->device);
  int rc = sync_all(c);
  if (rc) return rc;
  return settle(c);
}

int wayne_ctx_set_knob(wayne_ctx* c, const char* name, long long value) {
  if (!c || !name) return WAYNE_E_INVALID;
  for (const KnobName& k : kKnobNames)
    if (std::strcmp(name, k.name) == 0) {
      if (k.field == &Knobs::streams || k.field == &Knobs::fork_narrow) {
        // (these two shape the context itself: no exposure may be in flight while they change)
        int rc = sync_all(c);
        if (rc) return rc;
      }
      c->knobs.*(k.field) = std::max(value, -1LL);
      if (k.field == &Knobs::streams)
        c->n_streams = value < 0 ? kStreams : (int)std::min<long long>(std::max<long long>(value, 1), kStreams);
      if (k.field == &Knobs::fork_narrow) c->fork_narrow = value > 0 && c->side[0] && c->side[1] && c->ev_fork[0] && c->ev_fork[1] && c->ev_join[0] && c->ev_join[1];
      return WAYNE_OK;
    }
  return fail(c, WAYNE_E_INVALID, std::string("set_knob: no knob named ") + name);
}

int wayne_ctx_get_knob(const wayne_ctx* c, const char* name, long long* value) {
  if (!c || !name || !value) return WAYNE_E_INVALID;
  for (const KnobName& k : kKnobNames)
    if (std::strcmp(name, k.name) == 0) { *value = c->knobs.*(k.field); return WAYNE_OK; }
  return WAYNE_E_INVALID;
}

const char* wayne_build_flags(void) {
  // every compile-time switch that changes what the library computes or launches; the shipped build has none
  return ""
#ifdef WAYNE_NEGCTL_SKY_RUNAWAY
         " WAYNE_NEGCTL_SKY_RUNAWAY"
#endif
#ifdef WAYNE_NEGCTL_ADDITIVE_KEY
         " WAYNE_NEGCTL_ADDITIVE_KEY"
#endif
#ifdef WAYNE_NEGCTL_DROP_FRACTION
         " WAYNE_NEGCTL_DROP_FRACTION"
#endif
#ifdef WAYNE_TIMING_KNOBS
         " WAYNE_TIMING_KNOBS"
#endif
#ifdef WAYNE_TIMING_COLPOOL
         " WAYNE_TIMING_COLPOOL"
#endif
#ifdef WAYNE_TIMING_RAMP_NO_DARK
         " WAYNE_TIMING_RAMP_NO_DARK"
#endif
#ifdef WAYNE_TIMING_RAMP_NO_ONCE
         " WAYNE_TIMING_RAMP_NO_ONCE"
#endif
#if WAYNE_PREP_THREADS != 512
         " WAYNE_PREP_THREADS"
#endif
#if WAYNE_RAMP_THREADS != 1024
         " WAYNE_RAMP_THREADS"
#endif
#if WAYNE_RAMP_PF != 2
         " WAYNE_RAMP_PF"
#endif
      ;
}

void* wayne_ctx_stream(wayne_ctx* c) { return c ? (void*)c->streams[0] : nullptr; }

int wayne_ctx_slots(const wayne_ctx*) { return kSlots; }

// ---------------------------------------------------------------------------
// wayne_psf_apply
// ---------------------------------------------------------------------------
int wayne_psf_apply(wayne_ctx* c, const int32_t* counts, int size, const double* x_pos,
                    const double* y_pos, const double* psf_ratio, const double* psf_sigmal,
                    const double* psf_sigmah, int nr, int nc, uint32_t seed, int threads_compat,
                    int rng_mode, uint32_t exposure, uint32_t subsample, int32_t* out) {
  return wayne_psf_apply_ex(c, counts, size, x_pos, y_pos, psf_ratio, psf_sigmal, psf_sigmah, nr, nc, seed, threads_compat,
                            rng_mode, exposure, subsample, 0u, out);
}

int wayne_psf_apply_ex(wayne_ctx* c, const int32_t* counts, int size, const double* x_pos,
                       const double* y_pos, const double* psf_ratio, const double* psf_sigmal,
                       const double* psf_sigmah, int nr, int nc, uint32_t seed, int threads_compat,
                       int rng_mode, uint32_t exposure, uint32_t subsample, uint32_t flags, int32_t* out) {
  if (!c) return WAYNE_E_INVALID;
  if (size < 0 || nr <= 0 || nc <= 0 || !out) return fail(c, WAYNE_E_INVALID, "psf_apply: bad size / frame");
  if (nr != nc)
    return fail(c, WAYNE_E_INVALID,
                "psf_apply: only square frames (the reference indexes ypos*nc+xpos but bounds xpos by nr)");
  if (size > 0 && (!counts || !x_pos || !y_pos || !psf_ratio || !psf_sigmal || !psf_sigmah))
    return fail(c, WAYNE_E_INVALID, "psf_apply: null input");
  if (rng_mode != WAYNE_RNG_REPLAY && rng_mode != WAYNE_RNG_PHILOX && rng_mode != WAYNE_RNG_SPLIT)
    return fail(c, WAYNE_E_INVALID, "psf_apply: rng_mode");
  if (rng_mode == WAYNE_RNG_REPLAY && threads_compat <= 0)
    return fail(c, WAYNE_E_INVALID, "psf_apply: threads_compat must be >= 1 in replay mode");
  const int N = nr;
  (void)hipSetDevice(c->device);
  c->stream = c->streams[0];

  // A1 (ssum, with the reference's silent int overflows turned into errors), N = (int)(counts * ratio), the split mode's
  // routing and the tiles' clip rectangle: plan::plan_psf_apply (host_plan.h: host-only code, under sanitizers in tests/native)
  const int margin = 30;
  plan::PsfPlan pp;
  switch (plan::plan_psf_apply(counts, size, x_pos, y_pos, psf_ratio, psf_sigmal, N, rng_mode, threads_compat, margin, &pp)) {
    case plan::PSF_NEGATIVE: return fail(c, WAYNE_E_NEGATIVE, "psf_apply: negative count");
    case plan::PSF_OVERFLOW_REPLAY: return fail(c, WAYNE_E_OVERFLOW, "psf_apply: sum(counts)*threads >= 2^31 (pyparallel_menu.c:12,48)");
    case plan::PSF_OVERFLOW_TOTAL: return fail(c, WAYNE_E_OVERFLOW, "psf_apply: more than 2^32-1 electrons");
    default: break;
  }
  const long long total = pp.total;

  HIP_TRY(c, c->pa_frame.reserve((size_t)N * N * sizeof(int32_t)));
  HIP_TRY(c, hipMemsetAsync(c->pa_frame.p, 0, (size_t)N * N * sizeof(int32_t), c->stream));  // A3

  if (total > 0) {
    const std::vector<uint32_t>& prefix = pp.prefix;
    const std::vector<int32_t>&nwide = pp.nwide, &nsplit = pp.nsplit, &nlane = pp.nlane;
    const uint32_t run = pp.run;
    const bool any_split = pp.any_split, any_lane = pp.any_lane;
    SubInfo si{};
    si.electrons = run;
    si.read = 0;
    si.replay_seed = (int)seed;
    si.tx0 = pp.tx0; si.ty0 = pp.ty0; si.tw = pp.tw; si.th = pp.th;   // clip region of the tiles
    int rc;
    {
      // one pinned arena, one host-to-device copy (nine pageable copies cost ~0.1 ms of a 0.35 ms call)
      const size_t n = (size_t)size;
      const size_t need = align64((n + 1) * 4) + 3 * align64(n * 4) + 4 * align64(n * 8) + align64(sizeof(SubInfo)) + 64;
      StageArena& st = c->pa_stage;       // (no event: this call synchronises the stream before it returns)
      if ((rc = st.begin(c, need, "psf_apply: pinned staging allocation failed", false))) return rc;
      const bool fits = st.put(c->pa_prefix, prefix.data(), (n + 1) * 4) && st.put(c->pa_nwide, nwide.data(), n * 4) &&
                        st.put(c->pa_nsplit, nsplit.data(), n * 4) && st.put(c->pa_nlane, nlane.data(), n * 4) &&
                        st.put(c->pa_x, x_pos, n * 8) && st.put(c->pa_y, y_pos, n * 8) && st.put(c->pa_sl, psf_sigmal, n * 8) &&
                        st.put(c->pa_sh, psf_sigmah, n * 8) && st.put(c->pa_sub, &si, sizeof si);
      if (!fits) return fail(c, WAYNE_E_NOMEM, "psf_apply: staging arena too small");
      if ((rc = st.commit(c, c->stream))) return rc;
    }

    ThrowArgs a{};
    a.W = size; a.K = 1; a.N = N; a.S = N + 2 * kBorder; a.kb = 1;
    a.off32 = offsets_fit_32(a.N, a.S) ? 1 : 0;
    a.lane_reach_sigmas = lane_reach_sigmas(c);
    // enough workgroups to fill the chip when the call is big, one when small
    a.splits = (int)std::min<long long>(512, std::max<long long>(1, total / (64LL * kThrowThreads)));
    a.min_wgs = a.splits;   // one call, one sub-sample: share the electrons among all launched workgroups
    a.threads_compat = threads_compat;
    a.margin = margin;
    const int lds_ints = thrower_lds_ints(c, a.splits, margin);
    a.lds_ints = lds_ints;
    a.seed = seed; a.exposure = exposure; a.subsample0 = subsample;
    a.flags = 0; a.flat_off = 0; a.flat_wmin = 0; a.flat_wmax = 1; a.flat_inv_range = 1;
    a.sub = c->pa_sub.as<SubInfo>();
    a.prefix = c->pa_prefix.as<uint32_t>();
    a.nwide = c->pa_nwide.as<int32_t>();
    a.nsplit = c->pa_nsplit.as<int32_t>();
    a.nlane = c->pa_nlane.as<int32_t>();
    a.xpos = c->pa_x.as<double>(); a.ypos = c->pa_y.as<double>();
    a.sigl = c->pa_sl.as<double>(); a.sigh = c->pa_sh.as<double>();
    for (int i = 0; i < 4; ++i) a.flat[i] = nullptr;
    a.acc = nullptr;
    a.frame = c->pa_frame.as<int32_t>();
    if ((size + kNarrowThreads - 1) / kNarrowThreads > kMaxChunks && (any_lane || any_split))
      return fail(c, WAYNE_E_INVALID, "psf_apply: more than 65536 bins in split mode");
    for (int i = 0; i < kMaxChunks; ++i) a.chunk_order[i] = a.lane_order[i] = (unsigned char)i;
    if (run > 0) {
      ProfScope ps(c, PK_THROW);
      rc = (rng_mode == WAYNE_RNG_REPLAY) ? launch_throw<0, 0>(c, a, lds_ints) : launch_throw<1, 0>(c, a, lds_ints);
      if (rc) return rc;
    }
    const bool exact = (flags & WAYNE_F_EXACT_SAMPLERS) != 0;
    if (any_lane && any_split && fuse_thrower(c, a, false, exact)) {
      // (one grid for both: PK_THROW and PK_LANE span it, PK_NARROW records nothing)
      ProfScope ps_throw(c, PK_THROW);
      ProfScope ps(c, PK_LANE);
      if ((rc = launch_thrower<0>(c, a))) return rc;
    } else {
      if (any_lane) {
        ProfScope ps(c, PK_LANE);
        if ((rc = launch_lane<0>(c, a, false))) return rc;
      }
      if (any_split) {
        ProfScope ps(c, PK_NARROW);
        if ((rc = launch_narrow<0>(c, a, exact))) return rc;
      }
    }
    c->electrons += (uint64_t)total;
  }
  // (the frame goes straight into the caller's pageable array: landing it in a pinned buffer first and copying it
  // from there was 0.1 ms slower per call)
  HIP_TRY(c, hipMemcpyAsync(out, c->pa_frame.p, (size_t)N * N * sizeof(int32_t), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// grism + calibration
// ---------------------------------------------------------------------------
int wayne_ctx_set_grism(wayne_ctx* c, const wayne_grism_desc* g) {
  if (!c || !g) return WAYNE_E_INVALID;
  if (g->n_sens < 0 || (g->n_sens > 0 && (!g->sens_wl_um || !g->sens_val)))
    return fail(c, WAYNE_E_INVALID, "set_grism: sensitivity table");
  if (!plan::sens_table_ok(g->sens_wl_um, g->sens_val, g->n_sens))
    return fail(c, WAYNE_E_INVALID, "set_grism: sensitivity table must have finite values at finite, non-decreasing wavelengths");
  (void)hipSetDevice(c->device);
  c->stream = c->streams[0];
  int rc;
  if ((rc = upload(c, c->sens_wl, g->sens_wl_um, (size_t)g->n_sens))) return rc;
  if ((rc = upload(c, c->sens_val, g->sens_val, (size_t)g->n_sens))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  GrismDev& d = c->g;
  std::memcpy(d.trace, g->trace_coeff, sizeof d.trace);
  std::memcpy(d.wlsol, g->wl_solution, sizeof d.wlsol);
  std::memcpy(d.p_ratio, g->psf_ratio_poly, sizeof d.p_ratio);
  std::memcpy(d.p_sigl, g->psf_sigmal_poly, sizeof d.p_sigl);
  std::memcpy(d.p_sigh, g->psf_sigmah_poly, sizeof d.p_sigh);
  d.flat_wmin = g->flat_wmin;
  d.flat_wmax = g->flat_wmax;
  d.n_sens = g->n_sens;
  d.sens_wl = c->sens_wl.as<double>();
  d.sens_val = c->sens_val.as<double>();
  c->have_grism = true;
  c->grism_gen += 1;       // per-wavelength arrays worked out under the previous grism serve no later upload (plan::WlCache)
  // (... which also forgets what the upload kept per spectrum: it was worked out with the previous grism)
  c->est.set_grism(d, g->sens_wl_um, g->sens_val, g->n_sens);
  for (plan::SpectrumEstimate& e : c->src_est) e.set_grism(d, g->sens_wl_um, g->sens_val, g->n_sens);
  return WAYNE_OK;
}

int wayne_ctx_set_calibration(wayne_ctx* c, const wayne_calibration* k) {
  if (!c || !k) return WAYNE_E_INVALID;
  const int sub = k->subarray;
  if (sub != 64 && sub != 128 && sub != 256 && sub != 512 && sub != 1024)
    return fail(c, WAYNE_E_INVALID, "set_calibration: SUBARRAY must be 64,128,256,512 or 1024");
  if (k->n_reads < 1 || k->n_reads > kMaxReads) return fail(c, WAYNE_E_INVALID, "set_calibration: n_reads must be 1..15");
  (void)hipSetDevice(c->device);
  { int rc0 = sync_all(c); if (rc0) return rc0; }   // no exposure may be in flight while planes change
  c->stream = c->streams[0];
  const int N = side_of(sub), S = N + 2 * kBorder;
  const size_t NN = (size_t)N * N, SS = (size_t)S * S;
  int rc;
  if (c->have_cal && S != c->S) c->trap_state_valid = false;   // a trap state belongs to its frame size
  c->has_flat = k->flat[0] && k->flat[1] && k->flat[2] && k->flat[3];
  if (c->has_flat)
    for (int i = 0; i < 4; ++i)
      if ((rc = upload(c, c->flat[i], k->flat[i], NN))) return rc;
  c->has_pfl = k->pfl != nullptr;
  if (c->has_pfl) {
    std::vector<float> v = embed(k->pfl, N, S, 1.0f);
    if ((rc = upload(c, c->pfl, v.data(), SS))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->has_sky = k->sky != nullptr;
  c->sky_max = 0.f;
  c->sky_min = 0.f;
  if (c->has_sky) {
    c->sky_sorted.clear();
    for (size_t i = 0; i < NN; ++i)
      if (k->sky[i] > 0.f) c->sky_sorted.push_back(k->sky[i]);
    std::sort(c->sky_sorted.begin(), c->sky_sorted.end());
    if (!c->sky_sorted.empty()) { c->sky_min = c->sky_sorted.front(); c->sky_max = c->sky_sorted.back(); }
    std::vector<float> v = embed(k->sky, N, S, 0.0f);
    if ((rc = upload(c, c->sky, v.data(), SS))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->has_lin = k->lin[0] && k->lin[1] && k->lin[2] && k->lin[3];
  if (c->has_lin)
    for (int i = 0; i < 4; ++i)
      if ((rc = upload(c, c->lin[i], k->lin[i], SS))) return rc;
  c->has_dark = k->dark_sci && k->dark_err;
  if (c->has_dark) {
    if ((rc = upload(c, c->dark_sci, k->dark_sci, SS * k->n_reads))) return rc;
    {
      // `err <= 0 -> 1e-5` (detector.py:189-190) once, here, instead of a compare and a select per pixel and read in
      // k_ramp: the plane in HBM already holds what the reference's np.where would hand to np.random.normal
      std::vector<float> e(k->dark_err, k->dark_err + SS * k->n_reads);
      for (float& x : e) if (!(x > 0.f)) x = 0.00001f;
      if ((rc = upload(c, c->dark_err, e.data(), e.size()))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the copy reads a local vector)
    }
  }
  c->has_zero = k->zero_read != nullptr;
  if (c->has_zero)
    if ((rc = upload(c, c->zero_read, k->zero_read, SS))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->subarray = sub; c->N = N; c->S = S; c->cal_R = k->n_reads;
  c->have_cal = true;
  c->grism_gen += 1;       // (every slot is uploaded afresh: so are its per-wavelength arrays)
  for (Slot& s : c->slots) { s.uploaded = false; s.acc_init = false; }
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// exposure
// ---------------------------------------------------------------------------
int wayne_exposure_upload(wayne_ctx* c, int slot, const wayne_exposure_desc* d) {
  if (!c || !d) return WAYNE_E_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(c, WAYNE_E_INVALID, "upload: slot");
  if (!c->have_grism || !c->have_cal) return fail(c, WAYNE_E_STATE, "upload: set grism and calibration first");
  const int W = d->n_wl, K = d->n_samples, R = d->n_reads;
  if (W < 2 || K < 1 || R < 1) return fail(c, WAYNE_E_INVALID, "upload: need n_wl >= 2, n_samples >= 1, n_reads >= 1");
  if (R != c->cal_R) return fail(c, WAYNE_E_INVALID, "upload: n_reads differs from the calibration's");
  if (!d->wl_um || !d->flux || !d->x_ref || !d->y_ref || !d->dur_ms || !d->sample_read || !d->read_dt_s)
    return fail(c, WAYNE_E_INVALID, "upload: null array");
  if (d->rng_mode != WAYNE_RNG_REPLAY && d->rng_mode != WAYNE_RNG_PHILOX && d->rng_mode != WAYNE_RNG_SPLIT)
    return fail(c, WAYNE_E_INVALID, "upload: rng_mode");
  if ((d->flags & WAYNE_F_OUT_F64) && (d->flags & WAYNE_F_OUT_U16))
    return fail(c, WAYNE_E_INVALID, "upload: WAYNE_F_OUT_F64 and WAYNE_F_OUT_U16 are mutually exclusive");
  if (d->rng_mode == WAYNE_RNG_REPLAY && (d->threads_compat <= 0 || !d->replay_seed))
    return fail(c, WAYNE_E_INVALID, "upload: replay mode needs threads_compat >= 1 and replay_seed");
  for (int k = 0; k < K; ++k)
    if (d->sample_read[k] < 0 || d->sample_read[k] >= R) return fail(c, WAYNE_E_INVALID, "upload: sample_read out of range");
  if ((long long)K * W > 0x7FFFFFFFLL) return fail(c, WAYNE_E_INVALID, "upload: K*W too large");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  Slot& s = c->slots[slot];
  const auto t_up0 = std::chrono::steady_clock::now();
  auto lap = [&](int part, std::chrono::steady_clock::time_point& t_) {
    const auto now = std::chrono::steady_clock::now();
    c->up_us[part] += std::chrono::duration<double, std::micro>(now - t_).count();
    t_ = now;
  };
  auto t_lap = t_up0;
  // the slot is unusable until this call has succeeded: a failure half way leaves re-pointed views behind
  s.uploaded = false;
  s.front_done = false;
  s.fused_last = false;      // (last_prep points into buffers this call may re-allocate)
  s.n_extra = 0;             // a new exposure has no contaminants until wayne_exposure_set_sources says so
  s.traps_on = false;        // ... and no charge traps until wayne_exposure_set_traps says so
  s.hist_on = false;         // ... nor a carried history (wayne_exposure_set_trap_history)
  ex_clear(s);               // ... and no spectral extraction, nor any option of it, until wayne_exposure_set_extraction says so
  s.fits_on = false;         // ... and no FITS words until wayne_exposure_set_fits says so
  s.fits_pinned.misc = nullptr;
  s.expect_mode = 0;         // ... and no expected image until wayne_exposure_set_expected says so
  s.rampfit_on = s.rampfit_ran = false;   // ... and no ramp fit until wayne_exposure_set_rampfit says so
  s.ima_on = s.ima_ran = false;           // ... and no calibrated reads until wayne_exposure_set_ima says so
  s.ld_on = false;           // ... and one set of limb-darkening coefficients until wayne_exposure_set_limb_darkening says so
  s.ipc_on = false;          // ... and no inter-pixel capacitance until wayne_exposure_set_ipc says so
  s.spots_on = false;        // ... and a clean star until wayne_exposure_set_spots says so
  int rc;
  const size_t KW = (size_t)K * W;
  {
    // staging arena: every array of the descriptor, 64-byte aligned
    size_t need = 2 * align64((size_t)W * 8) + 3 * align64((size_t)K * 8) + 2 * align64((size_t)K * 4) + align64((size_t)R * 8) +
                  align64((size_t)K * kTrStride * 8) + 1024;
    if (d->lc_z) need += 2 * align64((size_t)K * 8) + align64((size_t)W * 8);
    if (d->depth) need += align64(KW * 8);
    // (waits if the previous upload of this slot is still reading the arena)
    if ((rc = s.stage.begin(c, need, "upload: pinned staging allocation failed"))) return rc;
  }
  if ((rc = upload_staged(c, s, s.wl, d->wl_um, (size_t)W))) return rc;
  if ((rc = upload_staged(c, s, s.flux, d->flux, (size_t)W))) return rc;
  s.has_lc = d->lc_z != nullptr;
  if (s.has_lc) {
    if (d->depth) return fail(c, WAYNE_E_INVALID, "upload: give either depth or lc_z, not both");
    if (!d->lc_rp) return fail(c, WAYNE_E_INVALID, "upload: lc_z needs lc_rp");
    if ((rc = upload_staged(c, s, s.lc_z, d->lc_z, (size_t)K))) return rc;
    if ((rc = upload_staged(c, s, s.lc_rp, d->lc_rp, (size_t)W))) return rc;
    // the range of the finite radius ratios (a NaN one -- a negative element of the spectrum -- takes no part, wherever it
    // stands); with none at all both ends stay NaN and no column is in transit (lc_route)
    s.lc_p_lo = s.lc_p_hi = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < W; ++i) {
      const double v = d->lc_rp[i];
      if (!std::isfinite(v)) continue;
      if (!(s.lc_p_lo <= v)) s.lc_p_lo = v;
      if (!(s.lc_p_hi >= v)) s.lc_p_hi = v;
    }
    s.has_lc_hidden = d->lc_hidden != nullptr;
    if (s.has_lc_hidden && (rc = upload_staged(c, s, s.lc_hidden, d->lc_hidden, (size_t)K))) return rc;
    HIP_TRY(c, s.depth.reserve(KW * sizeof(double)));
  }
  s.has_depth = d->depth != nullptr || s.has_lc;
  if (d->depth && (rc = upload_staged(c, s, s.depth, d->depth, KW))) return rc;
  if ((rc = upload_staged(c, s, s.xref, d->x_ref, (size_t)K))) return rc;
  if ((rc = upload_staged(c, s, s.yref, d->y_ref, (size_t)K))) return rc;
  if ((rc = upload_staged(c, s, s.dur, d->dur_ms, (size_t)K))) return rc;
  {
    // the trace coefficients of the K sub-samples, worked out here (they were k_prep_wl's, per run)
    double* tr = (double*)s.stage.place(s.tr, (size_t)K * kTrStride * sizeof(double));
    if (!tr) return fail(c, WAYNE_E_NOMEM, "upload: staging arena too small");
    plan::trace_table(c->g, K, d->x_ref, d->y_ref, tr);
  }
  s.has_replay_seed = d->replay_seed != nullptr;
  if (s.has_replay_seed && (rc = upload_staged(c, s, s.rseed, d->replay_seed, (size_t)K))) return rc;
  if ((rc = upload_staged(c, s, s.sread, d->sample_read, (size_t)K))) return rc;
  if ((rc = upload_staged(c, s, s.read_dt, d->read_dt_s, (size_t)R))) return rc;
  if ((rc = s.stage.commit(c, c->stream))) return rc;
  if ((size_t)(W + kPrepThreads - 1) / kPrepThreads > (size_t)kMaxPrepChunks || W > 32768)
    return fail(c, WAYNE_E_INVALID, "upload: more than 32768 wavelength bins");
  if ((rc = reserve_source(c, s, K, W))) return rc;
  if ((rc = prepare_wl_arrays(c, s, W, d->wl_um))) return rc;
  s.misc.view((char*)c->status_all.p + (size_t)slot * kMiscBytes);
  s.ran = false;
  const size_t SS = (size_t)c->S * c->S;
  const size_t acc_bytes = (size_t)R * SS * sizeof(long long);
  if (s.acc.cap < acc_bytes) s.acc_init = false;
  HIP_TRY(c, s.acc.reserve(acc_bytes));
  if (!s.acc_init) {
    HIP_TRY(c, hipMemsetAsync(s.acc.p, 0, acc_bytes, c->stream));
    s.acc_init = true;
    s.acc_dirty = false;
  }
  const size_t out_elem = out_elem_size(d->flags);
  HIP_TRY(c, s.out.reserve((size_t)(R + 1) * SS * out_elem));
  // (no stream synchronisation: the host arrays were copied into the pinned arena above)
  s.d = *d;
  s.d.wl_um = s.d.flux = s.d.depth = s.d.x_ref = s.d.y_ref = s.d.dur_ms = s.d.read_dt_s = nullptr;
  s.d.replay_seed = s.d.sample_read = nullptr;
  s.d.lc_z = s.d.lc_hidden = s.d.lc_rp = nullptr;
  s.W = W; s.K = K; s.R = R;
  s.seed = d->seed;
  s.read_dt_host.assign(d->read_dt_s, d->read_dt_s + R);
  lap(0, t_lap);     // staging, copies, reservations
  {
    plan::ThrowPlan tp;
    plan::estimate_thrown(c->est, W, d->wl_um, d->flux, K, d->dur_ms, d->scale_factor, d->rng_mode, &tp);
    adopt_plan(c, s, K, W, tp);
  }
  lap(1, t_lap);
  s.use_box = plan::accumulator_boxes(c->est, W, d->wl_um, d->flux, K, R, c->S, d->sub_scale, d->x_ref, d->y_ref,
                                      d->sample_read, s.acc_box) && !(c->knobs.no_acc_box > 0);
  lap(2, t_lap);
  {
    const size_t seg_bytes = ((SS + 63) / 64) * sizeof(uint32_t);
    if (s.seg.cap < seg_bytes) {
      HIP_TRY(c, s.seg.reserve(seg_bytes));
      HIP_TRY(c, hipMemsetAsync(s.seg.p, 0, s.seg.cap, c->stream));
    }
  }
  if ((rc = prepare_sky_tables(c, s))) return rc;
  lap(3, t_lap);
  c->up_calls += 1;
  s.force_throw = false;
  s.uploaded = true;
  s.front_done = false;
  return WAYNE_OK;
}

// The front half of one source of slot `s` (src 0 = the target, 1.. = its contaminants): prep, thrower, and -- with the
// target only -- the cosmic rays.  A contaminant is planned and launched exactly as the single-source exposure of its
// inputs would be (its own estimates, batches, thin / fused choice, skip_narrow and splits).
static int front_source(wayne_ctx* c, int slot, Slot& s, SourceState& ss, int src) {
  const wayne_exposure_desc& d = s.d;
  const int W = ss.W, K = s.K, R = s.R, N = c->N, S = c->S;
  WlArrays wa{ss.ratio.as<double>(), ss.sigl.as<double>(), ss.sigh.as<double>(), ss.sens.as<double>(),
              ss.dlam.as<double>()};
  // Nothing runs in front of k_prep_sub: the per-wavelength arrays are the upload's (prepare_wl_arrays), the trace
  // coefficients came with the descriptor's arrays and the status block needs no clearing.  The launch as it was, per
  // run: knob prep_wl_per_run -- and the run after the grism changed under an uploaded slot, whose arrays and
  // coefficients are the old grism's (from then on they are this grism's, for the same grid).
  if (c->knobs.prep_wl_per_run > 0 || ss.wl_cache.gen != c->grism_gen) {
    ProfScope ps(c, PK_PREP_WL);
    hipLaunchKernelGGL(k_prep_wl_run, dim3((std::max(W, K) + 255) / 256), dim3(256), 0, c->stream, c->g, W,
                       ss.wl.as<double>(), wa, src == 0 ? s.misc.as<uint32_t>() : nullptr, K, ss.xref.as<double>(), ss.yref.as<double>(),
                       ss.tr.as<double>());
    HIP_TRY(c, hipGetLastError());
    if (ss.wl_cache.valid) ss.wl_cache.gen = c->grism_gen;
  }
  // margin of a thrower workgroup's tile around its slice of the trace: 5 sigma_h, so that practically no electron
  // takes the in-loop global-atomic path (see k_lane)
  bool skip_narrow = false;
  bool lane_unlimited = false;   // split mode without a k_throw launch: the lanes take every bin (up to kLaneReach)
  bool fused = false;            // ... and no k_prep_sub either: k_lane<.., FUSED> plans its bins itself
  // A slot with a carried trap history takes the general sequence from the start, like a slot that is being re-run:
  // its exposure must never be run a second time (later exposures may have consumed the state it left), so status bit 1
  // must not be raised.  The cost: the k_throw launch that finds nothing to do.
  const bool force_throw = s.force_throw || (s.traps_on && s.hist_on);
  const int margin = d.thrower_margin > 0 ? d.thrower_margin : 30;
  PrepArgs prep_args{};
  CosmicArgs cosmic_args{};
  {
    PrepArgs& a = prep_args;
    a.g = c->g;
    a.W = W; a.K = K; a.N = N;
    a.sub_scale = d.sub_scale;
    a.margin = margin;
    a.max_tile = 0x7FFFFFFF;      // the sub-sample rectangle is only the clip region of the workgroup tiles
    a.seed = ss.seed; a.exposure = d.exposure_index; a.flags = d.flags;
    a.scale_factor = d.scale_factor;
    a.wl = ss.wl.as<double>(); a.flux = ss.flux.as<double>();
    a.depth = (src == 0 && s.has_depth) ? s.depth.as<double>() : nullptr;   // (contaminants do not transit)
    a.x_ref = ss.xref.as<double>(); a.y_ref = ss.yref.as<double>(); a.dur_ms = s.dur.as<double>();
    a.replay_seed = s.has_replay_seed ? s.rseed.as<int32_t>() : nullptr;
    a.sample_read = s.sread.as<int32_t>();
    a.tr = ss.tr.as<double>();
    a.wa = wa;
    a.counts = ss.counts.as<int32_t>(); a.nwide = ss.nwide.as<int32_t>();
    a.nsplit = ss.nsplit.as<int32_t>();
    a.nlane = ss.nlane.as<int32_t>();
    a.split_min = (d.rng_mode == WAYNE_RNG_SPLIT) ? kSplitMin : 0;
    // no bin expected beyond a lane's cap (the rule on every BASELINE configuration): k_throw is not launched at
    // all -- an empty launch still costs ~8 us of the exposure's critical path -- and the lanes take what they
    // find up to kLaneReach electrons; a bin beyond that (the estimate carries no Poisson noise) sets status bit 1
    // and the exposure is run again with k_throw when its status is read (look_at_status; settle for a whole batch)
    // (knob `lane_reach`: a test knob that lowers the lanes' reach so that the re-run path can be exercised)
    int reach = kLaneReach;
    if (c->knobs.lane_reach >= 0) reach = (int)std::min<long long>(std::max<long long>(c->knobs.lane_reach, 1), kLaneReach);
    lane_unlimited = d.rng_mode == WAYNE_RNG_SPLIT && ss.est_thrown <= 0. && d.thrower_splits <= 0 && !force_throw &&
                     c->knobs.throw_wgs < 0;
    a.lane_max = lane_unlimited ? reach : kLaneMax;
    a.prefix = ss.prefix.as<uint32_t>(); a.xpos = ss.xpos.as<double>(); a.ypos = ss.ypos.as<double>();
    a.sub = ss.sub.as<SubInfo>();
    a.total_electrons = c->counters.as<unsigned long long>();
    a.status = (uint32_t*)(s.misc.as<char>() + 8);
    a.run = s.run_no;
    const int n_chunks = (W + kPrepThreads - 1) / kPrepThreads;
    a.chunk_total = ss.chunk_total.as<uint32_t>();
    a.chunk_box = ss.chunk_box.as<double>();
    a.fix_inline = lane_unlimited ? 1 : 0;
    // a finely sampled scan holds a few electrons per bin and sub-sample: no bin is expected to reach the
    // multinomial's threshold (mean <= 6 against kSplitMin = 32: 1e-13 per draw), k_narrow's launch would only find
    // that out workgroup by workgroup (0.04 ms at K = 2233) -- it is left out, and a bin that qualifies after all
    // flags the run, which is then repeated with every kernel (look_at_status)
    skip_narrow = lane_unlimited && ss.max_narrow <= 6. && !(c->knobs.keep_narrow > 0);
    a.no_narrow = skip_narrow ? 1 : 0;
    CosmicArgs& ca = cosmic_args;
    ca.R = R; ca.N = N; ca.S = S; ca.seed = ss.seed; ca.exposure = d.exposure_index;
    ca.rate = (src == 0 && d.cosmic_rate >= 0.) ? d.cosmic_rate : -1.;   // (cosmic rays: once, with the target)
    ca.read_dt = s.read_dt.as<double>(); ca.acc = s.acc.as<long long>();
    ca.seg = s.seg.as<uint32_t>();
    // thin exposure, nothing for k_throw or k_narrow expected: the lanes plan their bins themselves (k_lane, FUSED)
    fused = lane_unlimited && skip_narrow && ss.thin && !(c->knobs.no_fuse > 0);
    ss.fused_last = fused;
    ss.last_prep = a;
    ss.last_chunks = n_chunks;
    if (!fused) {
      ProfScope ps(c, PK_PREP_SUB);
      hipLaunchKernelGGL(k_prep_sub, dim3(K, n_chunks), dim3(kPrepThreads), 0, c->stream, a, ca);
      HIP_TRY(c, hipGetLastError());
      if (!a.fix_inline) {
        hipLaunchKernelGGL(k_prep_fix, dim3(K), dim3(kPrepThreads), 0, c->stream, a, n_chunks);
        HIP_TRY(c, hipGetLastError());
      }
    }
  }
  {
    ThrowArgs a{};
    a.W = W; a.K = K; a.N = N; a.S = S;
    a.off32 = offsets_fit_32(N, S) ? 1 : 0;
    a.kb = ss.kb;
    a.lane_reach_sigmas = lane_reach_sigmas(c);
    // grid: one unit (128 electrons; 1 in replay mode) per lane of the workgroups of a sub-sample, from
    // the host's estimate of the electrons + 8 %, but at least ~4 workgroups per CU over the launch
    // (knob `throw_wgs` / desc.thrower_splits override); k_throw shares out what it actually finds
    const int min_wgs = 1024;
    int splits = d.thrower_splits;
    if (splits <= 0) {
      if (c->knobs.throw_wgs >= 0) {
        splits = (int)std::max<long long>(1, (std::max<long long>(c->knobs.throw_wgs, 1) + K - 1) / K);
      } else {
        const double unit = (d.rng_mode == WAYNE_RNG_REPLAY) ? 1. : (double)kThrowBlock;
        const double lanes = 1.08 * ss.est_thrown / unit;
        splits = (int)std::min(4096., std::ceil(lanes / kThrowThreads));
        // split mode with no bin expected beyond a lane's cap: k_throw finds nothing to do (any stray bin is
        // handled by the one workgroup per sub-sample launched here)
        if (d.rng_mode == WAYNE_RNG_SPLIT && ss.est_thrown <= 0. && !force_throw) splits = -1;
        // a lane takes several units when the launch would exceed ~24 workgroups per CU: then ~12 per CU
        // (each lane a handful of units) is the measured optimum (scripts/sweep_throw.py)
        const int cap = std::max(1, (3072 + K - 1) / K);
        if (splits > 2 * cap) splits = cap;
        splits = splits < 0 ? 1 : std::max(splits, (min_wgs + K - 1) / K);
      }
    }
    a.min_wgs = min_wgs;
    a.splits = std::min(splits, 4096);
    a.margin = margin;
    const int lds_ints = thrower_lds_ints(c, a.splits, margin);
    a.lds_ints = lds_ints;
    a.threads_compat = d.threads_compat;
    a.seed = ss.seed; a.exposure = d.exposure_index; a.subsample0 = 0;
    a.flags = d.flags;
    // grism.py:363: indices + (1014 - size) / 2 -- the same number as the frame offset 507 - SUBARRAY / 2
    // (exposure_generator.py:630) for every sub-array, so the descriptor's sub_scale serves both: 0 for the
    // full array, or the reference's -5 there when the caller keeps its quirks (the host then uploads the
    // flat planes rolled by +5 px, numpy's wrap-around for the negative indices)
    a.flat_off = d.sub_scale;
    a.flat_wmin = c->g.flat_wmin; a.flat_wmax = c->g.flat_wmax;
    a.flat_inv_range = 1.0 / (c->g.flat_wmax - c->g.flat_wmin);
    a.sub = ss.sub.as<SubInfo>(); a.prefix = ss.prefix.as<uint32_t>(); a.nwide = ss.nwide.as<int32_t>();
    a.nsplit = ss.nsplit.as<int32_t>();
    a.nlane = ss.nlane.as<int32_t>();
    std::memcpy(a.chunk_order, ss.chunk_order, sizeof a.chunk_order);
    std::memcpy(a.lane_order, ss.lane_order, sizeof a.lane_order);
    a.xpos = ss.xpos.as<double>(); a.ypos = ss.ypos.as<double>();
    a.sigl = ss.sigl.as<double>(); a.sigh = ss.sigh.as<double>();
    for (int i = 0; i < 4; ++i) a.flat[i] = c->has_flat ? c->flat[i].as<float>() : nullptr;
    a.acc = s.acc.as<long long>();
    a.frame = nullptr;
    if ((d.flags & WAYNE_F_ADD_FLAT) && !c->has_flat) return fail(c, WAYNE_E_STATE, "run: add_flat without a flat cube");
    const int si_ = slot % c->n_streams;
    const bool fork = d.rng_mode == WAYNE_RNG_SPLIT && c->fork_narrow && !skip_narrow;
    // k_lane and k_narrow as one grid (k_thrower): both would follow each other on this stream in their production form
    const bool one_grid = d.rng_mode == WAYNE_RNG_SPLIT && !skip_narrow && !fork && !fused &&
                          fuse_thrower(c, a, ss.thin, (d.flags & WAYNE_F_EXACT_SAMPLERS) != 0);
    hipStream_t main_stream = c->stream;
    {
      // (with the fork, the PK_THROW interval spans all thrower kernels; PK_NARROW / PK_LANE are those kernels' own)
      ProfScope ps_throw(c, PK_THROW);
      if (fork) {
        HIP_TRY(c, hipEventRecord(c->ev_fork[si_], main_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->side[si_], c->ev_fork[si_], 0));
        c->stream = c->side[si_];
        int rc;
        {
          ProfScope ps(c, PK_NARROW);
          rc = launch_narrow<1>(c, a, (d.flags & WAYNE_F_EXACT_SAMPLERS) != 0);
        }
        if (rc == WAYNE_OK && hipEventRecord(c->ev_join[si_], c->side[si_]) != hipSuccess)
          rc = fail(c, WAYNE_E_HIP, "run: event record on the side stream");
        c->stream = main_stream;
        if (rc) return rc;
      }
      int rc = lane_unlimited ? (int)WAYNE_OK
               : (d.rng_mode == WAYNE_RNG_REPLAY) ? launch_throw<0, 1>(c, a, lds_ints) : launch_throw<1, 1>(c, a, lds_ints);
      if (rc) return rc;
      if (d.rng_mode == WAYNE_RNG_SPLIT) {
        // (one grid: the PK_THROW and PK_LANE intervals span the combined launch, PK_NARROW records nothing)
        ProfScope ps(c, PK_LANE);
        if ((rc = one_grid ? launch_thrower<1>(c, a)
                  : fused  ? launch_lane<1>(c, a, true, &prep_args, &cosmic_args) : launch_lane<1>(c, a, ss.thin))) return rc;
      }
      if (fork) HIP_TRY(c, hipStreamWaitEvent(main_stream, c->ev_join[si_], 0));
    }
    if (!fork && !one_grid && d.rng_mode == WAYNE_RNG_SPLIT && !skip_narrow) {
      ProfScope ps(c, PK_NARROW);
      int rc = launch_narrow<1>(c, a, (d.flags & WAYNE_F_EXACT_SAMPLERS) != 0);
      if (rc) return rc;
    }
  }
  return WAYNE_OK;
}

// The boxes of a coupled exposure: each non-empty one a pixel wider on every side, clamped to the frame.
static void ipc_dilate(const int (*box)[4], int S, int (*out)[4]) {
  for (int r = 0; r < 16; ++r) {
    const int* b = box[r];
    if (box_empty(b)) { std::memcpy(out[r], b, sizeof(int) * 4); continue; }
    out[r][0] = std::max(b[0] - 1, 0); out[r][1] = std::min(b[1] + 1, S);
    out[r][2] = std::max(b[2] - 1, 0); out[r][3] = std::min(b[3] + 1, S);
  }
}

// k_ipc and k_ipc_clear of a slot (k_ipc.h), at the very end of its front half
static int launch_ipc(wayne_ctx* c, Slot& s) {
  const int S = c->S;
  IpcArgs a{};
  a.R = s.R; a.S = S;
  a.use_box = s.use_box ? 1 : 0;
  std::memcpy(a.w, s.ipc_w, sizeof a.w);
  a.a = s.acc.as<long long>(); a.b = s.acc_b.as<long long>();
  a.seg_a = s.seg.as<uint32_t>(); a.seg_b = s.seg_b.as<uint32_t>();
  const unsigned blocks = (unsigned)(((size_t)S * S + kIpcThreads - 1) / kIpcThreads);
  ProfScope ps(c, PK_IPC);
  ipc_dilate(s.acc_box, S, a.box);
  hipLaunchKernelGGL(k_ipc, dim3(blocks), dim3(kIpcThreads), 0, c->stream, a);
  HIP_TRY(c, hipGetLastError());
  std::memcpy(a.box, s.acc_box, sizeof a.box);
  hipLaunchKernelGGL(k_ipc_clear, dim3(blocks), dim3(kIpcThreads), 0, c->stream, a);
  HIP_TRY(c, hipGetLastError());
  return WAYNE_OK;
}

// tanh-sinh rule on (0, 1) of the light-curve kernels: t in [-3, 3], u = pi/2 sinh t, x = (1 + tanh u)/2 (wayne_amd/lightcurve.py)
static void lc_rule(float* x, float* w, float* d) {
  const double h = 6.0 / (kLcNodes - 1);
  for (int i = 0; i < kLcNodes; ++i) {
    const double t = -3.0 + h * i, u = 0.5 * kPi * std::sinh(t);
    x[i] = (float)(0.5 * (1.0 + std::tanh(u)));
    w[i] = (float)(h * 0.25 * kPi * std::cosh(t) / (std::cosh(u) * std::cosh(u)));
    d[i] = (float)(0.5 * std::exp(-std::fabs(u)) / std::cosh(u));
  }
}

int wayne_exposure_run_front(wayne_ctx* c, int slot) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "run", &sp)) return rc;
  Slot& s = *sp;
  // a supplied profile is laid out for its own window heights: refused before anything is enqueued, the slot stays usable
  if (s.extract_on && s.opt_on && s.prof_fixed && !plan::profile_rows_match(c->S, s.R, s.ex.steps, s.ex.row_lo, s.ex.row_hi, s.prof_rows))
    return fail(c, WAYNE_E_INVALID, "run: the optimal profile was made for other window heights than the extraction's");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const wayne_exposure_desc& d = s.d;
  const int W = s.W, K = s.K, R = s.R, S = c->S;
  const size_t SS = (size_t)S * S;
  if (c->n_streams == 2) {
    const int other = 1 - slot % 2;
    if (c->kdone_valid[other]) {     // see wayne_ctx::ev_kdone
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_kdone[other], 0));
      c->kdone_valid[other] = false;
    }
  }
  if (s.acc_dirty) {     // a front half without its back half: start from clean accumulators (and segment bits)
    HIP_TRY(c, hipMemsetAsync(s.acc.p, 0, (size_t)R * SS * sizeof(long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(s.seg.p, 0, s.seg.cap, c->stream));
    s.acc_dirty = false;
  }
  if (s.b_dirty) {       // ... and one that was coupled: its coupled accumulators and their bits likewise
    HIP_TRY(c, hipMemsetAsync(s.acc_b.p, 0, s.acc_b.cap, c->stream));
    HIP_TRY(c, hipMemsetAsync(s.seg_b.p, 0, s.seg_b.cap, c->stream));
    s.b_dirty = false;
  }
  if (s.has_lc && s.ld_on) {
    LcLdArgs a{};
    a.K = K; a.W = W;
    a.z = s.lc_z.as<double>();
    a.hidden = s.has_lc_hidden ? s.lc_hidden.as<double>() : nullptr;
    a.rp = s.lc_rp.as<double>();
    a.ld = s.ld_tab.as<double>();
    lc_rule(a.x, a.w, a.d);
    a.p_lo = s.lc_p_lo; a.p_hi = s.lc_p_hi;
    a.depth = s.depth.as<double>();
    ProfScope ps(c, PK_LIGHTCURVE);
    hipLaunchKernelGGL(k_lightcurve_ld, dim3(K), dim3(256), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
  } else if (s.has_lc) {
    LcArgs a{};
    a.K = K; a.W = W;
    a.z = s.lc_z.as<double>();
    a.hidden = s.has_lc_hidden ? s.lc_hidden.as<double>() : nullptr;
    a.rp = s.lc_rp.as<double>();
    double sum = 0.;
    for (int i = 0; i < 4; ++i) { a.ld[i] = d.lc_ld[i]; sum += d.lc_ld[i] * (i + 1) / (i + 5.0); }
    a.f0 = kPi * (1.0 - sum);
    lc_rule(a.x, a.w, a.d);
    a.p_lo = s.lc_p_lo; a.p_hi = s.lc_p_hi;
    a.depth = s.depth.as<double>();
    ProfScope ps(c, PK_LIGHTCURVE);
    hipLaunchKernelGGL(k_lightcurve, dim3(K), dim3(256), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
  }
  if (s.has_lc && s.spots_on) {
    // star spots: the matrix just written, rewritten in place (k_prep_sub and wayne_exposure_debug_depth see the spotted one)
    SpotArgs a = s.spot_args;
    a.K = K; a.W = W;
    a.z = s.lc_z.as<double>();
    a.hidden = s.has_lc_hidden ? s.lc_hidden.as<double>() : nullptr;
    a.rp = s.lc_rp.as<double>();
    a.px = s.spot_px.as<double>(); a.py = s.spot_py.as<double>();
    a.contrast = s.spot_contrast.as<double>();
    if (s.ld_on) { a.ld = s.ld_tab.as<double>(); a.ld_plane = (size_t)W; a.ld_step = 1; }
    else         { a.ld = s.spot_ld.as<double>(); a.ld_plane = 1; a.ld_step = 0; }
    a.depth = s.depth.as<double>();
    ProfScope ps(c, PK_SPOTS);
    hipLaunchKernelGGL(k_lightcurve_spots, dim3(K, (W + 255) / 256), dim3(256), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
  }

  // the number of this run (Slot::run_no); after 2^32 - 1 runs the block is cleared once, on the stream, and the count starts over
  if (s.run_no == 0xFFFFFFFFu) {
    HIP_TRY(c, hipMemsetAsync(s.misc.p, 0, kMiscBytes, c->stream));
    s.run_no = 0;
  }
  s.run_no += 1;
  for (int i = 0; i <= s.n_extra; ++i) {
    int rc = front_source(c, slot, s, s.source(i), i);
    if (rc) return rc;
  }
  s.acc_dirty = true;
  // inter-pixel capacitance: behind every source's thrower and the cosmic rays, so that what lies between the halves is
  // what k_ramp will read
  s.ipc_front = s.ipc_on;
  if (s.ipc_on) {
    s.b_dirty = true;
    if (int rc = launch_ipc(c, s)) return rc;
  }
  s.front_done = true;
  return WAYNE_OK;
}

int wayne_exposure_run_back(wayne_ctx* c, int slot) {
  if (!c) return WAYNE_E_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(c, WAYNE_E_INVALID, "run: slot");
  Slot& s = c->slots[slot];
  if (!s.uploaded || !s.front_done) return fail(c, WAYNE_E_STATE, "run_back: run_front first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const wayne_exposure_desc& d = s.d;
  const int S = c->S;
  RampArgs a{};
  a.R = s.R; a.N = c->N; a.S = S;
#ifdef WAYNE_TIMING_KNOBS
  // measurement knob of TIMING BUILDS only (scripts/ramp_vs_reads.py builds its own library with -DWAYNE_TIMING_KNOBS):
  // the kernel works through the first n reads only -- the slot's other accumulators stay uncleared and the later
  // reads' planes stale, so the shipped library does not look at the knob at all
  bool ramp_reads_cut = false;
  if (c->knobs.ramp_reads >= 0) { a.R = (int)std::max<long long>(1, std::min<long long>(s.R, c->knobs.ramp_reads)); ramp_reads_cut = a.R < s.R; }
#endif
  a.seed = d.seed; a.exposure = d.exposure_index; a.flags = d.flags;
  a.sky_ct_s = d.sky_ct_s; a.noise_mean = d.noise_mean; a.noise_std = d.noise_std;
  a.read_dt = s.read_dt.as<double>();
  a.acc = s.acc.as<long long>();
  a.pfl = c->has_pfl ? c->pfl.as<float>() : nullptr;
  a.sky = c->has_sky ? c->sky.as<float>() : nullptr;
  for (int i = 0; i < 4; ++i) a.lin[i] = c->has_lin ? c->lin[i].as<float>() : nullptr;
  a.dark_sci = c->has_dark ? c->dark_sci.as<float>() : nullptr;
  a.dark_err = c->has_dark ? c->dark_err.as<float>() : nullptr;
  a.zero_read = c->has_zero ? c->zero_read.as<double>() : nullptr;
  a.out = s.out.p;
  if ((d.flags & WAYNE_F_ADD_GAIN_VARIATIONS) && !c->has_pfl) return fail(c, WAYNE_E_STATE, "run: add_gain_variations without a pixel flat");
  if ((d.flags & WAYNE_F_ADD_NON_LINEAR) && !c->has_lin) return fail(c, WAYNE_E_STATE, "run: add_non_linear without coefficient planes");
  if (d.sky_ct_s > 0. && !c->has_sky) return fail(c, WAYNE_E_STATE, "run: sky background without a master sky");
  // sky tables were planned and uploaded with the descriptor (prepare_sky_tables)
  a.sky_alias = s.sky_alias_on ? s.sky_tab.as<uint32_t>() : nullptr;
  a.alias_mask = s.sky_alias_on ? s.sky_mask : 0u;
  a.sky_levels = s.sky_L;
  for (int l = 0; l < 16; ++l) { a.sky_level[l] = s.sky_level[l]; a.sky_tab0[l] = s.sky_tab0[l]; a.tab0[l] = s.sky_tab0[l]; a.bg[l] = 0.f; }
  for (int r = 0; r < s.R && r < 16; ++r) a.bg[r] = (float)(d.sky_ct_s * s.read_dt_host[r]);
  a.use_box = s.use_box ? 1 : 0;
  std::memcpy(a.box, s.acc_box, sizeof a.box);
  a.seg = s.seg.as<uint32_t>();
  if (s.ipc_front) {     // the coupled accumulators, one pixel beyond the thrower's boxes, and their own segment bits
    a.acc = s.acc_b.as<long long>();
    ipc_dilate(s.acc_box, S, a.box);
    a.seg = s.seg_b.as<uint32_t>();
  }
  const int threads = kRampThreads;
  const unsigned blocks = (unsigned)(((size_t)S * S + threads - 1) / threads);
  if (s.traps_on && s.hist_on && (!c->trap_state_valid || !c->ev_trap_chain))
    return fail(c, WAYNE_E_STATE, "run: a trap history without a trap state (wayne_ctx_trap_state_reset / _upload first)");
  {
    ProfScope ps(c, PK_RAMP, true);
    RampTrapKernel trap = nullptr;
    RampHistKernel hist = nullptr;
    void (*kern)(RampArgs) = select_ramp(c, s, nullptr, &trap, &hist);
    if (trap || hist) {
      // charge traps (wayne_exposure_set_traps): the model, the per-read intervals and the staged start tables
      TrapArgs t{};
      t.G = s.trap_G;
      t.start_d = s.trap_d.as<double>();
      t.start_f = s.trap_f.as<float>();
      t.rate_lo = s.trap_lo;
      t.ln_lo = std::log(s.trap_lo);
      t.u_scale = s.trap_G > 2 ? (double)(s.trap_G - 2) / std::log(s.trap_hi / s.trap_lo) : 0.;
      for (int p = 0; p < 2; ++p) {
        t.eta[p] = s.trap_eta[p];
        t.eta_n[p] = s.trap_eta[p] / s.trap_n[p];
        t.inv_tau[p] = 1.0 / s.trap_tau[p];
        t.eta_f[p] = (float)t.eta[p]; t.eta_n_f[p] = (float)t.eta_n[p]; t.inv_tau_f[p] = (float)t.inv_tau[p];
      }
      for (int r = 0; r < s.R && r < 16; ++r) {
        t.sum_dt += s.read_dt_host[r];
        t.sum_bg += (double)a.bg[r];
        t.dt[r] = (float)s.read_dt_host[r];
        t.inv_dt[r] = (float)(1.0 / s.read_dt_host[r]);
      }
      t.inv_sum_dt_f = (float)(1.0 / t.sum_dt);
      t.sum_bg_f = (float)t.sum_bg;
      if (hist) {
        // a carried history: the state's read-after-write chain over the two streams (CtxStreams::ev_trap_chain)
        TrapHistArgs h{};
        h.state = c->trap_state.as<float2>();
        h.gap_s = s.hist_gap; h.gap_f = (float)s.hist_gap;
        h.lit = s.hist_lit;
        for (int p = 0; p < 2; ++p) {
          h.fill[p] = s.hist_fill[p]; h.fill_f[p] = (float)s.hist_fill[p];
          h.n[p] = s.trap_n[p]; h.n_f[p] = (float)s.trap_n[p];
        }
        if (c->trap_chain_valid) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_trap_chain, 0));
        if (ps.on) hipExtLaunchKernelGGL(hist, dim3(blocks), dim3(threads), 0, c->stream, ps.rec.a, ps.rec.b, 0, a, t, h);
        else hipLaunchKernelGGL(hist, dim3(blocks), dim3(threads), 0, c->stream, a, t, h);
        HIP_TRY(c, hipEventRecord(c->ev_trap_chain, c->stream));
        c->trap_chain_valid = true;
      } else if (ps.on) hipExtLaunchKernelGGL(trap, dim3(blocks), dim3(threads), 0, c->stream, ps.rec.a, ps.rec.b, 0, a, t);
      else hipLaunchKernelGGL(trap, dim3(blocks), dim3(threads), 0, c->stream, a, t);
    } else {
      if (ps.on) hipExtLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, c->stream, ps.rec.a, ps.rec.b, 0, a);
      else hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
  }
  if (s.extract_on)
    if (int rc = launch_extract(c, s)) return rc;   // the spectra of the reads just written, behind them on the stream
  if (s.fits_on)
    if (int rc = launch_fits(c, s)) return rc;      // ... and their FITS words
  if (s.rampfit_on)
    if (int rc = launch_rampfit(c, s)) return rc;   // ... and the fit of their ramps
  if (s.ima_on)
    if (int rc = launch_ima(c, s)) return rc;       // ... and the calibrated reads, which take the fit's jump bits
  if (s.expect_mode)
    if (int rc = launch_expected(c, s)) return rc;  // ... and, last of all, the expected image of the thrower stage
  s.acc_dirty = false;
  s.b_dirty = false;
#ifdef WAYNE_TIMING_KNOBS
  if (ramp_reads_cut) { s.acc_dirty = true; s.b_dirty = s.ipc_front; }     // the next front half starts from cleared accumulators
#endif
  s.front_done = false;
  s.ran = true;
  return WAYNE_OK;
}

int wayne_exposure_ramp_variant(wayne_ctx* c, int slot, char* buf, int cap) {
  if (!buf || cap <= 0) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "ramp_variant", &sp)) return rc;
  std::string name;
  (void)select_ramp(c, *sp, &name);
  std::snprintf(buf, (size_t)cap, "%s", name.c_str());
  return WAYNE_OK;
}

int wayne_exposure_run(wayne_ctx* c, int slot) {
  int rc = wayne_exposure_run_front(c, slot);
  if (rc) return rc;
  return wayne_exposure_run_back(c, slot);
}

int wayne_exposure_status(wayne_ctx* c, int slot, int* status) {
  if (!status) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "status", &sp)) return rc;
  Slot& s = *sp;
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  Slot::Misc m{};
  int rc = read_status(c, s, &m);
  if (rc) return rc;
  *status = m.bits(s.run_no);
  return WAYNE_OK;
}

unsigned long long wayne_ctx_reruns(const wayne_ctx* c) { return c ? (unsigned long long)c->reruns : 0ull; }

unsigned long long wayne_ctx_profile_uploads(const wayne_ctx* c) { return c ? (unsigned long long)c->profile_uploads : 0ull; }

int wayne_exposure_run_checked(wayne_ctx* c, int slot) {
  int rc = wayne_exposure_run(c, slot);
  if (rc) return rc;
  return download_settled(c, slot, [] { return WAYNE_OK; });
}

int wayne_exposure_download(wayne_ctx* c, int slot, void* out_reads) {
  if (!out_reads) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download", &sp)) return rc;
  Slot& s = *sp;
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  return download_settled(c, slot, out_reads, s.out.p, (size_t)(s.R + 1) * c->S * c->S * out_elem_size(s.d.flags));
}

int wayne_exposure_fetch_async(wayne_ctx* c, int slot) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "fetch_async", &sp)) return rc;
  Slot& s = *sp;
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // The copy follows the slot's kernels on the slot's own stream: while it runs (1.2 ms at 55 GB/s for a full
  // frame) the kernels of the exposure in the next slot run on the other stream.  (A separate copy stream fed by
  // events was measured: 660-700 exposures/s instead of 810-826 -- scripts/probe_pipeline.py.)
  return s.pinned.fetch(c, slot, s.out.p, (size_t)(s.R + 1) * c->S * c->S * out_elem_size(s.d.flags), true,
                        "fetch_async: pinned host allocation failed");
}

int wayne_exposure_wait(wayne_ctx* c, int slot, void** host_reads) {
  if (!c || !host_reads) return WAYNE_E_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(c, WAYNE_E_INVALID, "wait: slot");
  Slot& s = c->slots[slot];
  if (!s.uploaded || !s.pinned.fetched()) return fail(c, WAYNE_E_STATE, "wait: fetch_async first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *host_reads = s.pinned.buf.p;
  bool reran = false;                        // (the status word came with the reads)
  int rc = look_at_status(c, slot, s.pinned.misc, wayne_exposure_run, &reran, s.pinned.run);
  if (rc || !reran) return rc;
  if ((rc = wayne_exposure_fetch_async(c, slot))) return rc;     // a bin beyond the lanes' reach: once more, with k_throw
  // (spectra fetched beside the reads are those of the first run: fetched again too, with the second run's status word)
  if (s.extract_on && s.ex_pinned.misc && (rc = wayne_exposure_fetch_spectra_async(c, slot))) return rc;
  if (s.fits_on && s.fits_pinned.misc && (rc = wayne_exposure_fetch_fits_async(c, slot))) return rc;   // (... and FITS words likewise)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return look_at_status(c, slot, s.pinned.misc, nullptr, nullptr, s.pinned.run);
}

void* wayne_exposure_device_reads(wayne_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= kSlots) return nullptr;
  return c->slots[slot].out.p;
}

int wayne_exposure_synthesize(wayne_ctx* c, const wayne_exposure_desc* d, void* out_reads) {
  int rc = wayne_exposure_upload(c, 0, d);
  if (rc) return rc;
  if ((rc = wayne_exposure_run(c, 0))) return rc;
  return wayne_exposure_download(c, 0, out_reads);
}

// debug_fetch of source `src` of the slot (0 = the target; acc_e is the slot's, shared by all sources)
static int fetch_source(wayne_ctx* c, int slot, int src, int32_t* counts, double* x_pos, double* y_pos, double* acc_e) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "debug_fetch", &sp)) return rc;
  Slot& s = *sp;
  if (src < 0 || src > s.n_extra) return fail(c, WAYNE_E_INVALID, "debug_fetch: no such source in this slot");
  SourceState& ss = s.source(src);
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t KW = (size_t)s.K * ss.W;
  if (counts) HIP_TRY(c, hipMemcpyAsync(counts, ss.counts.p, KW * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (ss.fused_last && (x_pos || y_pos)) {
    // a fused front half kept no positions: k_prep_sub works them out now (same code, same inputs; its cosmic-ray
    // stage off and its electron count into a spare counter)
    PrepArgs a = ss.last_prep;
    a.total_electrons = c->counters.as<unsigned long long>() + 1;
    CosmicArgs off{};
    off.rate = -1.;
    hipLaunchKernelGGL(k_prep_sub, dim3(s.K, ss.last_chunks), dim3(kPrepThreads), 0, c->stream, a, off);
    HIP_TRY(c, hipGetLastError());
  }
  if (x_pos) HIP_TRY(c, hipMemcpyAsync(x_pos, ss.xpos.p, KW * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (y_pos) HIP_TRY(c, hipMemcpyAsync(y_pos, ss.ypos.p, KW * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  {
    // (between run_front and run_back: a run that met a bin beyond the lanes' reach is repeated with k_throw first)
    bool reran = false;
    int rc = look_at_status(c, slot, nullptr, s.front_done ? wayne_exposure_run_front : nullptr, &reran);
    if (rc) return rc;
    if (reran) return fetch_source(c, slot, src, counts, x_pos, y_pos, acc_e);
  }
  if (acc_e) {
    const size_t n = (size_t)s.R * c->S * c->S;
    std::vector<long long> tmp(n);
    // (a coupled front half: what k_ramp will read)
    const void* from = (s.front_done && s.ipc_front) ? s.acc_b.p : s.acc.p;
    HIP_TRY(c, hipMemcpyAsync(tmp.data(), from, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) acc_e[i] = (double)tmp[i] * kInvQ;
  }
  return look_at_status(c, slot, nullptr);
}

int wayne_exposure_debug_fetch(wayne_ctx* c, int slot, int32_t* counts, double* x_pos, double* y_pos,
                               double* acc_e) {
  return fetch_source(c, slot, 0, counts, x_pos, y_pos, acc_e);
}

int wayne_exposure_debug_fetch_source(wayne_ctx* c, int slot, int source, int32_t* counts, double* x_pos, double* y_pos) {
  return fetch_source(c, slot, source, counts, x_pos, y_pos, nullptr);
}

int wayne_exposure_debug_boxes(wayne_ctx* c, int slot, int32_t* boxes, int32_t* segments, int* use_box) {
  if (!boxes || !segments || !use_box) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "debug_boxes", &sp)) return rc;
  Slot& s = *sp;
  *use_box = s.use_box ? 1 : 0;
  const int S = c->S;
  // (a coupled slot: the boxes k_ramp gets, a pixel wider on every side)
  int box[16][4];
  std::memcpy(box, s.acc_box, sizeof box);
  if (s.ipc_on) ipc_dilate(s.acc_box, S, box);
  for (int r = 0; r < 16; ++r) {
    for (int i = 0; i < 4; ++i) boxes[4 * r + i] = s.use_box ? box[r][i] : 0;
    int n = 0;
    if (r < s.R) {
      // the wave test of k_ramp (acc_live) over the frame's 64-pixel segments
      for (int p0 = 0; p0 < S * S; p0 += 64) {
        const int wy0 = p0 / S, wy1 = std::min(p0 + 63, S * S - 1) / S, wx0 = p0 - wy0 * S;
        const int* b = box[r];
        const bool rows = wy0 < b[3] && wy1 >= b[2];
        const bool cols = (wy0 != wy1) || (wx0 < b[1] && wx0 + 64 > b[0]);
        n += (!s.use_box || (rows && cols)) ? 1 : 0;
      }
    }
    segments[r] = n;
  }
  return WAYNE_OK;
}

int wayne_exposure_debug_depth(wayne_ctx* c, int slot, double* depth) {
  if (!c || !depth) return WAYNE_E_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(c, WAYNE_E_INVALID, "debug_depth: slot");
  Slot& s = c->slots[slot];
  if (!s.uploaded || !s.has_depth) return fail(c, WAYNE_E_STATE, "debug_depth: no depth matrix in this slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  HIP_TRY(c, hipMemcpyAsync(depth, s.depth.p, (size_t)s.K * s.W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// contaminating field stars
// ---------------------------------------------------------------------------

int wayne_exposure_set_sources(wayne_ctx* c, int slot, const wayne_source_desc* src, int n) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_sources", &sp)) return rc;
  Slot& s = *sp;
  if (n < 0 || n > kMaxSources) return fail(c, WAYNE_E_INVALID, "set_sources: n must be 0 .. WAYNE_MAX_SOURCES");
  if (n > 0 && !src) return fail(c, WAYNE_E_INVALID, "set_sources: null list");
  if (n > 0 && s.d.rng_mode == WAYNE_RNG_REPLAY)
    return fail(c, WAYNE_E_INVALID, "set_sources: replay mode reproduces the reference, which has no second star");
  const int K = s.K, R = s.R;
  for (int i = 0; i < n; ++i) {
    const wayne_source_desc& q = src[i];
    if (q.tag == 0) return fail(c, WAYNE_E_INVALID, "set_sources: tag 0 is the target's");
    for (int j = 0; j < i; ++j)
      if (src[j].tag == q.tag) return fail(c, WAYNE_E_INVALID, "set_sources: duplicate tag");
    if (q.n_wl < 2 || q.n_wl > 32768) return fail(c, WAYNE_E_INVALID, "set_sources: n_wl must be 2 .. 32768");
    if ((long long)K * q.n_wl > 0x7FFFFFFFLL) return fail(c, WAYNE_E_INVALID, "set_sources: K*W too large");
    if (!q.wl_um || !q.flux) return fail(c, WAYNE_E_INVALID, "set_sources: null array");
    if (!std::isfinite(q.dx) || !std::isfinite(q.dy)) return fail(c, WAYNE_E_INVALID, "set_sources: offset not finite");
  }
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // from here on a failure leaves the slot as uploaded: the target alone, with the target's boxes
  s.n_extra = 0;
  s.front_done = false;
  // (the target's arrays, as the slot's arena still holds them)
  const double* x0 = s.stage.host_of<double>(s.xref);
  const double* y0 = s.stage.host_of<double>(s.yref);
  const double* dur = s.stage.host_of<double>(s.dur);
  const int32_t* sread = s.stage.host_of<int32_t>(s.sread);
  const bool no_box = c->knobs.no_acc_box > 0;
  s.use_box = plan::accumulator_boxes(c->est, s.W, s.stage.host_of<double>(s.wl), s.stage.host_of<double>(s.flux), K, R, c->S,
                                      s.d.sub_scale, x0, y0, sread, s.acc_box) && !no_box;
  if (n == 0) return WAYNE_OK;
  bool use_box = s.use_box;
  int box[16][4];
  std::memcpy(box, s.acc_box, sizeof box);
  for (int i = 0; i < n; ++i) {
    const wayne_source_desc& q = src[i];
    SourceState& e = s.extra[i];
    const int W = q.n_wl;
    StageArena& st = e.src_stage;
    int rc = st.begin(c, 2 * align64((size_t)W * 8) + 2 * align64((size_t)K * 8) + align64((size_t)K * kTrStride * 8) + 256,
                      "set_sources: pinned staging allocation failed");
    if (rc) return rc;
    const bool fits = st.put(e.wl, q.wl_um, (size_t)W * 8) && st.put(e.flux, q.flux, (size_t)W * 8);
    double* xs = (double*)st.place(e.xref, (size_t)K * 8);
    double* ys = (double*)st.place(e.yref, (size_t)K * 8);
    double* tr = (double*)st.place(e.tr, (size_t)K * kTrStride * sizeof(double));
    if (!fits || !xs || !ys || !tr) return fail(c, WAYNE_E_NOMEM, "set_sources: staging arena too small");
    for (int k = 0; k < K; ++k) { xs[k] = x0[k] + q.dx; ys[k] = y0[k] + q.dy; }
    plan::trace_table(c->g, K, xs, ys, tr);
    if ((rc = st.commit(c, c->stream))) return rc;
    if ((rc = reserve_source(c, e, K, W))) return rc;
    if ((rc = prepare_wl_arrays(c, e, W, q.wl_um))) return rc;
    e.W = W;
    e.seed = wayne_source_seed(s.d.seed, q.tag);
    e.fused_last = false;
    // the plan of the single-source exposure with these inputs (wayne_exposure_upload)
    plan::ThrowPlan tp;
    plan::estimate_thrown(c->src_est[i], W, q.wl_um, q.flux, K, dur, s.d.scale_factor, s.d.rng_mode, &tp);
    adopt_plan(c, e, K, W, tp);
    // k_ramp loads (and clears) an accumulator only inside its read's box: the box is the union over the sources, each
    // at its own positions -- a contaminant's electrons outside it would vanish from this exposure and reappear in the
    // next one of the slot
    int b[16][4];
    if (!plan::accumulator_boxes(c->src_est[i], W, q.wl_um, q.flux, K, R, c->S, s.d.sub_scale, xs, ys, sread, b)) {
      use_box = false;
    } else {
      for (int r = 0; r < 16; ++r) {
        if (box_empty(b[r])) continue;
        if (box_empty(box[r])) { std::memcpy(box[r], b[r], sizeof b[r]); continue; }
        box[r][0] = std::min(box[r][0], b[r][0]); box[r][1] = std::max(box[r][1], b[r][1]);
        box[r][2] = std::min(box[r][2], b[r][2]); box[r][3] = std::max(box[r][3], b[r][3]);
      }
    }
    s.extra_tag[i] = q.tag;
  }
  std::memcpy(s.acc_box, box, sizeof box);
  s.use_box = use_box && !no_box;
  s.n_extra = n;
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// limb darkening per wavelength bin
// ---------------------------------------------------------------------------

int wayne_exposure_set_limb_darkening(wayne_ctx* c, int slot, const double* ld, int n_wl) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_limb_darkening", &sp)) return rc;
  Slot& s = *sp;
  s.ld_on = false;                // from here on a refusal leaves the slot usable, without a table
  s.spots_on = false;             // (spots were checked against the coefficients they were set with: set them again)
  s.front_done = false;           // (the depth matrix of the last front half is not this setting's)
  if (!ld || n_wl == 0) return WAYNE_OK;
  if (!s.has_lc) return fail(c, WAYNE_E_INVALID, "set_limb_darkening: the slot has no device light curve (lc_z was NULL)");
  const int W = s.W;
  if (n_wl != W) return fail(c, WAYNE_E_INVALID, "set_limb_darkening: n_wl differs from the exposure's");
  for (int w = 0; w < W; ++w) {
    double sum = 0.;
    for (int i = 0; i < 4; ++i) {
      const double v = ld[(size_t)w * 4 + i];
      if (!std::isfinite(v)) return fail(c, WAYNE_E_INVALID, "set_limb_darkening: coefficient not finite");
      sum += v * (i + 1) / (i + 5.0);
    }
    if (!(1.0 - sum > 0.)) return fail(c, WAYNE_E_INVALID, "set_limb_darkening: the disk flux 1 - sum a_n n/(n+4) must be > 0 in every bin");
  }
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t bytes = (size_t)4 * W * sizeof(double);
  int rc = s.ld_stage.begin(c, bytes, "set_limb_darkening: pinned staging allocation failed");
  if (rc) return rc;
  double* h = (double*)s.ld_stage.place(s.ld_tab, bytes);
  if (!h) return fail(c, WAYNE_E_NOMEM, "set_limb_darkening: staging arena too small");
  for (int i = 0; i < 4; ++i)     // [W][4] -> four planes of W
    for (int w = 0; w < W; ++w) h[(size_t)i * W + w] = ld[(size_t)w * 4 + i];
  if ((rc = s.ld_stage.commit(c, c->stream))) return rc;
  s.ld_on = true;
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// star spots
// ---------------------------------------------------------------------------

// numpy.polynomial.legendre.leggauss(10), to the last bit (wayne_amd/spots.py hands the numpy law the same doubles)
static const SpotRule kSpotRule = {
    {-0.9739065285171717, -0.8650633666889845, -0.6794095682990244, -0.4333953941292472, -0.14887433898163122,
     0.14887433898163122, 0.4333953941292472, 0.6794095682990244, 0.8650633666889845, 0.9739065285171717},
    {0.06667134430868807, 0.14945134915058036, 0.219086362515982, 0.2692667193099965, 0.295524224714753,
     0.295524224714753, 0.2692667193099965, 0.219086362515982, 0.14945134915058036, 0.06667134430868807}};

void wayne_spot_lens_basis(double px, double py, double cx, double cy, double p, double r, double out[5]) {
  lens_basis(kSpotRule, px, py, cx, cy, p, r, out[0], out[1], out[2], out[3], out[4]);
}

void wayne_spot_rule(double nodes[10], double weights[10]) {
  for (int i = 0; i < kSpotNodes; ++i) { nodes[i] = kSpotRule.g[i]; weights[i] = kSpotRule.w[i]; }
}

int wayne_exposure_set_spots(wayne_ctx* c, int slot, const wayne_spots_desc* sp, int n_wl, int n_sub) {
  Slot* slotp;
  if (int rc = slot_gate(c, slot, "set_spots", &slotp)) return rc;
  Slot& s = *slotp;
  s.spots_on = false;             // from here on a refusal leaves the slot usable, with a clean star
  s.front_done = false;           // (the depth matrix of the last front half is not this setting's)
  if (!sp || sp->n == 0) return WAYNE_OK;
  if (!s.has_lc) return fail(c, WAYNE_E_INVALID, "set_spots: the slot has no device light curve (lc_z was NULL)");
  const int W = s.W, K = s.K, n = sp->n;
  if (n < 0 || n > kSpotMax) return fail(c, WAYNE_E_INVALID, "set_spots: at most 8 spots");
  if (n_wl != W) return fail(c, WAYNE_E_INVALID, "set_spots: n_wl differs from the exposure's");
  if (n_sub != K) return fail(c, WAYNE_E_INVALID, "set_spots: n_sub differs from the exposure's");
  if (!sp->contrast || !sp->px || !sp->py) return fail(c, WAYNE_E_INVALID, "set_spots: null array");
  SpotArgs a{};
  a.n = n;
  a.gl = kSpotRule;
  for (int i = 0; i < n; ++i) {
    const double x = sp->cx[i], y = sp->cy[i], r = sp->radius[i];
    if (!std::isfinite(r) || !(r > 0.)) return fail(c, WAYNE_E_INVALID, "set_spots: a radius must be finite and > 0");
    if (!std::isfinite(x) || !std::isfinite(y)) return fail(c, WAYNE_E_INVALID, "set_spots: a centre must be finite");
    if (!(std::sqrt(x * x + y * y) + r <= 0.98))
      return fail(c, WAYNE_E_INVALID, "set_spots: |centre| + radius must be <= 0.98 (a spot may not reach the limb)");
    for (int j = 0; j < i; ++j)
      if (std::hypot(x - sp->cx[j], y - sp->cy[j]) < r + sp->radius[j])
        return fail(c, WAYNE_E_INVALID, "set_spots: two spots overlap");
    a.cx[i] = x; a.cy[i] = y; a.r[i] = r;
    lens_basis(kSpotRule, x, y, x, y, r, r, a.S[i][0], a.S[i][1], a.S[i][2], a.S[i][3], a.S[i][4]);
  }
  for (size_t i = 0; i < (size_t)n * W; ++i)
    if (!std::isfinite(sp->contrast[i]) || sp->contrast[i] < 0.)
      return fail(c, WAYNE_E_INVALID, "set_spots: a contrast must be finite and >= 0");
  // the planet's track on the transit rows (the pinned copies of lc_z / lc_hidden hold until the next upload)
  const double* z = s.stage.host_of<double>(s.lc_z);
  const double* hid = s.has_lc_hidden ? s.stage.host_of<double>(s.lc_hidden) : nullptr;
  for (int k = 0; k < K; ++k) {
    if (!(z[k] < 10.) || (hid && hid[k] != 0.)) continue;
    if (!std::isfinite(sp->px[k]) || !std::isfinite(sp->py[k]))
      return fail(c, WAYNE_E_INVALID, "set_spots: the planet's track must be finite on every transit row");
  }
  // the spotted disc flux F0 - D, in the kernel's own arithmetic
  const double* tab = s.ld_on ? s.ld_stage.host_of<double>(s.ld_tab) : nullptr;
  for (int w = 0; w < W; ++w) {
    double l[4];
    for (int i = 0; i < 4; ++i) l[i] = tab ? tab[(size_t)i * W + w] : s.d.lc_ld[i];
    const double c0 = 1. - l[0] - l[1] - l[2] - l[3];
    const double f0 = kPi * (1. - (l[0] * (1. / 5.) + l[1] * (2. / 6.) + l[2] * (3. / 7.) + l[3] * (4. / 8.)));
    double D = 0.;
    for (int i = 0; i < n; ++i)
      D = D + (1. - sp->contrast[(size_t)i * W + w]) *
                  ((((c0 * a.S[i][0] + l[0] * a.S[i][1]) + l[1] * a.S[i][2]) + l[2] * a.S[i][3]) + l[3] * a.S[i][4]);
    if (!(f0 - D > 0.)) return fail(c, WAYNE_E_INVALID, "set_spots: the spotted disc flux F0 - D must be > 0 in every bin");
  }
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t cb = (size_t)n * W * sizeof(double), kb = (size_t)K * sizeof(double);
  int rc = s.spot_stage.begin(c, align64(cb) + 2 * align64(kb) + 64, "set_spots: pinned staging allocation failed");
  if (rc) return rc;
  if (!s.spot_stage.put(s.spot_contrast, sp->contrast, cb) || !s.spot_stage.put(s.spot_px, sp->px, kb) ||
      !s.spot_stage.put(s.spot_py, sp->py, kb) || !s.spot_stage.put(s.spot_ld, s.d.lc_ld, 4 * sizeof(double)))
    return fail(c, WAYNE_E_NOMEM, "set_spots: staging arena too small");
  if ((rc = s.spot_stage.commit(c, c->stream))) return rc;
  s.spot_args = a;
  s.spots_on = true;
  return WAYNE_OK;
}

int wayne_spots_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_SPOTS, launches, ms); }

// ---------------------------------------------------------------------------
// charge trapping
// ---------------------------------------------------------------------------

int wayne_exposure_set_traps(wayne_ctx* c, int slot, const wayne_trap_desc* t) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_traps", &sp)) return rc;
  Slot& s = *sp;
  s.traps_on = false;             // from here on a refusal leaves the slot usable, without traps
  s.hist_on = false;              // (a history belongs to the traps it was set after)
  if (!t) return WAYNE_OK;
  if (s.d.rng_mode == WAYNE_RNG_REPLAY)
    return fail(c, WAYNE_E_INVALID, "set_traps: replay mode reproduces the reference, which has no charge traps");
  const int G = t->n_rate;
  if (G < 2 || G > WAYNE_MAX_TRAP_RATES) return fail(c, WAYNE_E_INVALID, "set_traps: n_rate must be 2 .. WAYNE_MAX_TRAP_RATES");
  if (!std::isfinite(t->rate_lo) || !std::isfinite(t->rate_hi) || !(t->rate_lo > 0.) ||
      !(G > 2 ? t->rate_hi > t->rate_lo : t->rate_hi >= t->rate_lo))
    return fail(c, WAYNE_E_INVALID, "set_traps: need finite 0 < rate_lo < rate_hi");
  for (int p = 0; p < 2; ++p) {
    const double n = t->n_traps[p], eta = t->efficiency[p], tau = t->lifetime_s[p];
    if (!std::isfinite(n) || !(n > 0.)) return fail(c, WAYNE_E_INVALID, "set_traps: n_traps must be finite and > 0");
    if (!std::isfinite(eta) || !(eta >= 0. && eta <= 1.)) return fail(c, WAYNE_E_INVALID, "set_traps: efficiency must lie in [0, 1]");
    if (!std::isfinite(tau) || !(tau > 0.)) return fail(c, WAYNE_E_INVALID, "set_traps: lifetime_s must be finite and > 0");
    if (!t->start[p]) return fail(c, WAYNE_E_INVALID, "set_traps: null start table");
    for (int j = 0; j < G; ++j) {
      const double e = t->start[p][j];
      if (!std::isfinite(e) || !(e >= 0. && e <= n))
        return fail(c, WAYNE_E_INVALID, "set_traps: start table entries must lie in [0, n_traps]");
    }
  }
  for (int r = 0; r < s.R; ++r)
    if (!(s.read_dt_host[r] > 0.)) return fail(c, WAYNE_E_INVALID, "set_traps: every read interval must be > 0");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t bytes_d = (size_t)2 * G * sizeof(double), bytes_f = (size_t)2 * G * sizeof(float);
  int rc = s.trap_stage.begin(c, align64(bytes_d) + bytes_f, "set_traps: pinned staging allocation failed");
  if (rc) return rc;
  double* hd = (double*)s.trap_stage.place(s.trap_d, bytes_d);
  float* hf = (float*)s.trap_stage.place(s.trap_f, bytes_f);
  if (!hd || !hf) return fail(c, WAYNE_E_NOMEM, "set_traps: staging arena too small");
  for (int p = 0; p < 2; ++p)
    for (int j = 0; j < G; ++j) {
      hd[p * G + j] = t->start[p][j];
      hf[p * G + j] = (float)t->start[p][j];
    }
  if ((rc = s.trap_stage.commit(c, c->stream))) return rc;
  for (int p = 0; p < 2; ++p) {
    s.trap_n[p] = t->n_traps[p];
    s.trap_eta[p] = t->efficiency[p];
    s.trap_tau[p] = t->lifetime_s[p];
  }
  s.trap_lo = t->rate_lo;
  s.trap_hi = t->rate_hi;
  s.trap_G = G;
  s.traps_on = true;
  return WAYNE_OK;
}

// The context's trap state.  The three calls below are rare (a visit's start and end): every stream is brought to rest
// before and after, so no exposure is in flight while the state changes and the chain starts afresh.
static int trap_state_ready(wayne_ctx* c, const char* who) {
  if (!c->have_cal) return fail(c, WAYNE_E_STATE, std::string(who) + ": set the calibration first (the frame size is not known)");
  (void)hipSetDevice(c->device);
  int rc = sync_all(c);
  if (rc) return rc;
  c->stream = c->streams[0];
  c->trap_chain_valid = false;
  return WAYNE_OK;
}
static int trap_state_alloc(wayne_ctx* c) {
  if (!c->ev_trap_chain) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_trap_chain, hipEventDisableTiming));
  c->trap_state_valid = false;
  HIP_TRY(c, c->trap_state.reserve((size_t)c->S * c->S * sizeof(float2)));
  return WAYNE_OK;
}

int wayne_ctx_trap_state_reset(wayne_ctx* c, const double initial[2]) {
  if (!c || !initial) return WAYNE_E_INVALID;
  if (!std::isfinite(initial[0]) || !std::isfinite(initial[1]) || initial[0] < 0. || initial[1] < 0.)
    return fail(c, WAYNE_E_INVALID, "trap_state_reset: the initial occupancies must be finite and >= 0");
  int rc = trap_state_ready(c, "trap_state_reset");
  if (rc || (rc = trap_state_alloc(c))) return rc;
  const int n = c->S * c->S;
  hipLaunchKernelGGL(k_trap_state_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->trap_state.as<float2>(),
                     n, (float)initial[0], (float)initial[1]);
  HIP_TRY(c, hipGetLastError());
  if ((rc = sync_all(c))) return rc;
  c->trap_state_valid = true;
  return WAYNE_OK;
}

int wayne_ctx_trap_state_upload(wayne_ctx* c, const float* state) {
  if (!c || !state) return WAYNE_E_INVALID;
  int rc = trap_state_ready(c, "trap_state_upload");
  if (rc || (rc = trap_state_alloc(c))) return rc;
  HIP_TRY(c, hipMemcpy(c->trap_state.p, state, (size_t)c->S * c->S * sizeof(float2), hipMemcpyHostToDevice));
  if ((rc = sync_all(c))) return rc;
  c->trap_state_valid = true;
  return WAYNE_OK;
}

int wayne_ctx_trap_state_download(wayne_ctx* c, float* state) {
  if (!c || !state) return WAYNE_E_INVALID;
  if (c->have_cal && !c->trap_state_valid) return fail(c, WAYNE_E_STATE, "trap_state_download: no trap state (reset or upload first)");
  int rc = trap_state_ready(c, "trap_state_download");
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(state, c->trap_state.p, (size_t)c->S * c->S * sizeof(float2), hipMemcpyDeviceToHost));
  return sync_all(c);
}

int wayne_exposure_set_trap_history(wayne_ctx* c, int slot, const wayne_trap_history_desc* h) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_trap_history", &sp)) return rc;
  Slot& s = *sp;
  s.hist_on = false;              // from here on a refusal leaves the slot usable, without a history
  if (!h) return WAYNE_OK;
  if (!s.traps_on) return fail(c, WAYNE_E_STATE, "set_trap_history: wayne_exposure_set_traps first");
  // (the front half picks the launch sequence that can never ask for a second run: it has to know about the history)
  if (s.front_done) return fail(c, WAYNE_E_STATE, "set_trap_history: not between wayne_exposure_run_front and _run_back");
  if (!c->trap_state_valid) return fail(c, WAYNE_E_STATE, "set_trap_history: no trap state (wayne_ctx_trap_state_reset / _upload first)");
  if (!std::isfinite(h->gap_s) || !(h->gap_s >= 0.)) return fail(c, WAYNE_E_INVALID, "set_trap_history: gap_s must be finite and >= 0");
  for (int p = 0; p < 2; ++p)
    if (!std::isfinite(h->fill[p]) || !(h->fill[p] >= 0. && h->fill[p] <= s.trap_n[p]))
      return fail(c, WAYNE_E_INVALID, "set_trap_history: fill must lie in [0, n_traps]");
  s.hist_gap = h->gap_s;
  s.hist_lit = h->lit ? 1 : 0;
  s.hist_fill[0] = h->fill[0];
  s.hist_fill[1] = h->fill[1];
  s.hist_on = true;
  return WAYNE_OK;
}

// ---------------------------------------------------------------------------
// spectral extraction
// ---------------------------------------------------------------------------

int wayne_exposure_set_extraction(wayne_ctx* c, int slot, const wayne_extract_desc* x) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_extraction", &sp)) return rc;
  Slot& s = *sp;
  ex_clear(s);                    // from here on a refusal leaves the slot usable, without extraction
  if (!x) return WAYNE_OK;
  int chunks = 0;
  if (const char* why = plan::extract_desc_error(c->S, s.R, x->steps, x->row_lo, x->row_hi, x->bg_col_lo, x->bg_col_hi, &chunks))
    return fail(c, WAYNE_E_INVALID, std::string("set_extraction: ") + why);
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.ex_part.reserve((size_t)2 * chunks * ((size_t)s.R + 1) * c->S * sizeof(double)));
  s.ex = *x;
  s.ex_chunks = chunks;
  s.extract_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_set_crrej(wayne_ctx* c, int slot, const wayne_crrej_desc* r) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_crrej", EX_ON, kNoExtraction, &sp)) return rc;
  Slot& s = *sp;
  s.crrej_on = false;             // from here on a refusal leaves the slot extracting, without rejection
  if (int rc = ex_relayout(c, s)) return rc;
  if (!r) return WAYNE_OK;
  if (const char* why = plan::crrej_desc_error(s.ex.steps, r->k, r->read_noise_e))
    return fail(c, WAYNE_E_INVALID, std::string("set_crrej: ") + why);
  (void)hipSetDevice(c->device);
  const size_t NP = (size_t)s.R + 1, S = (size_t)c->S;
  HIP_TRY(c, s.cr_mask.reserve(S * S * sizeof(uint16_t)));
  HIP_TRY(c, s.ex_part_n.reserve((size_t)s.ex_chunks * NP * S * sizeof(unsigned)));
  plan::crrej_mask_rows(s.R, s.ex.steps, s.ex.row_lo, s.ex.row_hi, &s.cr_lo, &s.cr_hi);
  s.cr_k = r->k;
  s.cr_rn = r->read_noise_e;
  s.crrej_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_set_channels(wayne_ctx* c, int slot, const wayne_channels_desc* d) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_channels", EX_ON, kNoExtraction, &sp)) return rc;
  Slot& s = *sp;
  s.chan_on = false;              // from here on a refusal leaves the slot extracting, without channels
  s.optch_on = false;             // (the optimal channels are the channels': set_optimal_channels comes after this call)
  if (int rc = ex_relayout(c, s)) return rc;
  if (!d) return WAYNE_OK;
  int u_lo = 0, u_hi = 0;
  if (const char* why = plan::channels_desc_error(c->S, s.R, s.ex.steps, s.ex.row_lo, s.ex.row_hi, d->n_channels, d->edges_um,
                                                  d->wl_a, d->wl_b, d->flags, &u_lo, &u_hi))
    return fail(c, WAYNE_E_INVALID, std::string("set_channels: ") + why);
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t NP = (size_t)s.R + 1, S = (size_t)c->S, C = (size_t)d->n_channels;
  HIP_TRY(c, s.ch_part.reserve((size_t)s.ex_chunks * kChanGroups * NP * 2 * C * sizeof(double)));
  // (set_variance may have come first: the variances take on channels_var)
  if (s.var_on) HIP_TRY(c, s.ch_part_v.reserve((size_t)s.ex_chunks * kChanGroups * NP * C * sizeof(double)));
  if (int rc = s.ch_stage.begin(c, 3 * 64 + (2 * S + C + 1) * sizeof(double), "set_channels: pinned host allocation failed")) return rc;
  if (!s.ch_stage.put(s.ch_edges, d->edges_um, (C + 1) * sizeof(double)) || !s.ch_stage.put(s.ch_wa, d->wl_a, S * sizeof(double)) ||
      !s.ch_stage.put(s.ch_wb, d->wl_b, S * sizeof(double)))
    return fail(c, WAYNE_E_NOMEM, "set_channels: staging arena too small");
  if (int rc = s.ch_stage.commit(c, c->stream)) return rc;
  s.ch_C = d->n_channels;
  s.ch_lo = u_lo; s.ch_hi = u_hi;
  s.ch_flags = d->flags;
  s.chan_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_set_variance(wayne_ctx* c, int slot, const wayne_variance_desc* v) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_variance", EX_ON, kNoExtraction, &sp)) return rc;
  Slot& s = *sp;
  s.var_on = false;               // from here on a refusal leaves the slot extracting, without variances
  s.opt_on = false;               // (the optimal extraction stands on the variances: set_optimal comes after this call)
  s.prof_deliver = s.prof_fetched = s.prof_valid = s.prof_fixed = s.optch_on = false;   // (the profile planes and the optimal channels go with the optimal extraction)
  if (int rc = ex_relayout(c, s)) return rc;
  if (!v) return WAYNE_OK;
  if (const char* why = plan::variance_desc_error(s.ex.steps, v->read_noise))
    return fail(c, WAYNE_E_INVALID, std::string("set_variance: ") + why);
  (void)hipSetDevice(c->device);
  const size_t NP = (size_t)s.R + 1, S = (size_t)c->S, C = s.chan_on ? (size_t)s.ch_C : 0;
  HIP_TRY(c, s.ex_part_v.reserve((size_t)s.ex_chunks * NP * S * sizeof(double)));
  if (s.chan_on) HIP_TRY(c, s.ch_part_v.reserve((size_t)s.ex_chunks * kChanGroups * NP * C * sizeof(double)));
  s.var_rn = v->read_noise;
  s.var_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_set_optimal(wayne_ctx* c, int slot, const wayne_optimal_desc* d) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_optimal", EX_ON | EX_VAR, "no variances set for the slot", &sp)) return rc;
  Slot& s = *sp;
  s.opt_on = false;               // from here on a refusal leaves the slot extracting with variances, without the optimal values
  s.prof_deliver = s.prof_fetched = s.prof_valid = s.prof_fixed = s.optch_on = false;   // (the profile planes and the optimal channels go with the optimal extraction)
  if (int rc = ex_relayout(c, s)) return rc;
  if (!d) return WAYNE_OK;
  if (const char* why = plan::optimal_desc_error(d->half_width))
    return fail(c, WAYNE_E_INVALID, std::string("set_optimal: ") + why);
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.opt_part.reserve((size_t)3 * s.ex_chunks * ((size_t)s.R + 1) * c->S * sizeof(double)));
  s.opt_H = d->half_width;
  s.opt_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_fetch_spectra_async(wayne_ctx* c, int slot) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "fetch_spectra_async", &sp)) return rc;
  Slot& s = *sp;
  if (!s.extract_on) return fail(c, WAYNE_E_STATE, "fetch_spectra_async: no extraction set for the slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // (120 KB behind the slot's kernels on its own stream: nothing here for the other stream to keep out of phase with)
  return s.ex_pinned.fetch(c, slot, s.ex_out.p, s.lay.bytes, false, "fetch_spectra_async: pinned host allocation failed");
}

int wayne_exposure_wait_spectra(wayne_ctx* c, int slot, double** spectra, double** sky) {
  if (!spectra || !sky) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "wait_spectra", &sp)) return rc;
  Slot& s = *sp;
  if (!s.extract_on) return fail(c, WAYNE_E_STATE, "wait_spectra: no extraction set for the slot");
  if (!s.ex_pinned.fetched()) return fail(c, WAYNE_E_STATE, "wait_spectra: fetch_spectra_async first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  s.ex_base = s.ex_pinned.buf.p;
  *spectra = (double*)(s.ex_pinned.buf.p + s.lay.spectra);
  *sky = (double*)(s.ex_pinned.buf.p + s.lay.sky);
  bool reran = false;                        // (the status word came with the spectra)
  int rc = look_at_status(c, slot, s.ex_pinned.misc, wayne_exposure_run, &reran, s.ex_pinned.run);
  if (rc || !reran) return rc;
  if ((rc = wayne_exposure_fetch_spectra_async(c, slot))) return rc;     // a bin beyond the lanes' reach: once more, with k_throw
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return look_at_status(c, slot, s.ex_pinned.misc, nullptr, nullptr, s.ex_pinned.run);
}

int wayne_exposure_download_spectra(wayne_ctx* c, int slot, double* spectra, double* sky) {
  if (!spectra || !sky) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download_spectra", &sp)) return rc;
  Slot& s = *sp;
  if (!s.extract_on) return fail(c, WAYNE_E_STATE, "download_spectra: no extraction set for the slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // spectra and sky go straight to the caller's arrays; what lies behind them comes, in one copy, to its own offset of
  // ex_host, for the accessors below
  const plan::SpectraLayout& l = s.lay;
  const size_t head = l.sky + ((size_t)s.R + 1) * sizeof(double);
  s.ex_host.resize((l.bytes + 7) / 8);
  char* const host = (char*)s.ex_host.data();
  s.ex_base = host;
  return download_settled(c, slot, [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(spectra, (const char*)s.ex_out.p + l.spectra, l.sky - l.spectra, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sky, (const char*)s.ex_out.p + l.sky, head - l.sky, hipMemcpyDeviceToHost, c->stream));
    if (l.bytes > head)
      HIP_TRY(c, hipMemcpyAsync(host + head, (const char*)s.ex_out.p + head, l.bytes - head, hipMemcpyDeviceToHost, c->stream));
    return WAYNE_OK;
  });
}

// A region of the block the slot's last wait_spectra / download_spectra brought back (null: the region is off).
static const double* ex_fetched(const Slot& s, size_t offset) {
  return offset == plan::kNoRegion ? nullptr : (const double*)(s.ex_base + offset);
}

int wayne_exposure_rejected(wayne_ctx* c, int slot, const uint32_t** n_rejected) {
  if (!n_rejected) return WAYNE_E_INVALID;
  Slot* s;
  if (int rc = ex_gate(c, slot, "rejected", EX_ON | EX_CRREJ, "no rejection set for the slot", &s)) return rc;
  if (!s->ex_base) return fail(c, WAYNE_E_STATE, std::string("rejected: ") + kFetchFirst);
  *n_rejected = (const uint32_t*)ex_fetched(*s, s->lay.n_rejected);
  return WAYNE_OK;
}

int wayne_exposure_channels(wayne_ctx* c, int slot, const double** channels) {
  if (!channels) return WAYNE_E_INVALID;
  Slot* s;
  if (int rc = ex_gate(c, slot, "channels", EX_ON | EX_CHAN, "no channels set for the slot", &s)) return rc;
  if (!s->ex_base) return fail(c, WAYNE_E_STATE, std::string("channels: ") + kFetchFirst);
  *channels = ex_fetched(*s, s->lay.channels);
  return WAYNE_OK;
}

int wayne_exposure_variances(wayne_ctx* c, int slot, const double** spectra_var, const double** sky_var, const double** channels_var) {
  if (!spectra_var || !sky_var || !channels_var) return WAYNE_E_INVALID;
  Slot* s;
  if (int rc = ex_gate(c, slot, "variances", EX_ON | EX_VAR, "no variances set for the slot", &s)) return rc;
  if (!s->ex_base) return fail(c, WAYNE_E_STATE, std::string("variances: ") + kFetchFirst);
  *spectra_var = ex_fetched(*s, s->lay.spectra_var);
  *sky_var = ex_fetched(*s, s->lay.sky_var);
  *channels_var = ex_fetched(*s, s->lay.channels_var);
  return WAYNE_OK;
}

int wayne_exposure_optimal(wayne_ctx* c, int slot, const double** optimal, const double** optimal_var) {
  if (!optimal || !optimal_var) return WAYNE_E_INVALID;
  Slot* s;
  if (int rc = ex_gate(c, slot, "optimal", EX_ON | EX_VAR | EX_OPT, kNoOptimal, &s)) return rc;
  if (!s->ex_base) return fail(c, WAYNE_E_STATE, std::string("optimal: ") + kFetchFirst);
  *optimal = ex_fetched(*s, s->lay.optimal);
  *optimal_var = ex_fetched(*s, s->lay.optimal_var);
  return WAYNE_OK;
}

int wayne_exposure_set_optimal_channels(wayne_ctx* c, int slot, int on) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_optimal_channels", EX_ON | EX_VAR | EX_OPT | EX_CHAN, "the slot needs channels and the optimal extraction", &sp))
    return rc;
  Slot& s = *sp;
  s.optch_on = false;
  if (int rc = ex_relayout(c, s)) return rc;
  if (!on) return WAYNE_OK;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.optch_part.reserve((size_t)s.ex_chunks * kChanGroups * ((size_t)s.R + 1) * 3 * s.ch_C * sizeof(double)));
  s.optch_on = true;
  return ex_relayout(c, s);
}

int wayne_exposure_optimal_channels(wayne_ctx* c, int slot, const double** channels_opt, const double** channels_opt_var) {
  if (!channels_opt || !channels_opt_var) return WAYNE_E_INVALID;
  Slot* s;
  if (int rc = ex_gate(c, slot, "optimal_channels", EX_ON | EX_VAR | EX_OPT | EX_CHAN | EX_OPTCH, "no optimal channels set for the slot", &s))
    return rc;
  if (!s->ex_base) return fail(c, WAYNE_E_STATE, std::string("optimal_channels: ") + kFetchFirst);
  *channels_opt = ex_fetched(*s, s->lay.channels_opt);
  *channels_opt_var = ex_fetched(*s, s->lay.channels_opt_var);
  return WAYNE_OK;
}

// doubles of a slot's profile planes: every pixel of all R + 1 windows
static size_t profile_count(const wayne_ctx* c, const Slot& s) {
  return plan::profile_offsets(c->S, s.R, s.ex.steps, s.ex.row_lo, s.ex.row_hi, nullptr);
}

int wayne_exposure_deliver_profile(wayne_ctx* c, int slot, int on) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "deliver_profile", EX_ON | EX_VAR | EX_OPT, kNoOptimal, &sp)) return rc;
  Slot& s = *sp;
  s.prof_deliver = s.prof_fetched = s.prof_valid = false;
  if (!on) return WAYNE_OK;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.prof_planes.reserve(profile_count(c, s) * sizeof(double)));
  s.prof_deliver = true;
  return WAYNE_OK;
}


int wayne_exposure_set_optimal_profile(wayne_ctx* c, int slot, const double* profile, const int* rows) {
  return wayne_exposure_set_optimal_profile_tagged(c, slot, profile, rows, 0);
}

int wayne_exposure_set_optimal_profile_tagged(wayne_ctx* c, int slot, const double* profile, const int* rows, uint64_t tag) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "set_optimal_profile", EX_ON | EX_VAR | EX_OPT, kNoOptimal, &sp)) return rc;
  Slot& s = *sp;
  s.prof_fixed = false;           // from here on a refusal leaves the slot with the exposure's own profile
  if (!profile) return WAYNE_OK;
  size_t n = 0;
  if (const char* why = plan::profile_rows_error(c->S, s.R, rows, &n))
    return fail(c, WAYNE_E_INVALID, std::string("set_optimal_profile: ") + why);
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // A visit hands the same profile to a slot with every exposure it uploads there: the device copy outlives what clears
  // the option, and a profile the CALLER identifies by the same non-zero tag, with the same heights and length, is not
  // copied again -- no copy, no wait for the slot's stream, and the array is not looked at.
  const uint64_t h = tag;
  bool same = tag != 0 && s.prof_fix_valid && s.prof_fix_n == n && s.prof_fix_hash == h && s.prof_fix_R == s.R;
  for (int p = 0; same && p <= s.R; ++p) same = s.prof_rows[p] == rows[p];
  if (!same) {
    s.prof_fix_valid = false;
    HIP_TRY(c, s.prof_fix.reserve(n * sizeof(double)));
    // (from the caller's memory: the call returns when the array has been read)
    HIP_TRY(c, hipMemcpyAsync(s.prof_fix.p, profile, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p <= s.R; ++p) s.prof_rows[p] = rows[p];
    s.prof_fix_n = n; s.prof_fix_hash = h; s.prof_fix_R = s.R;
    s.prof_fix_valid = true;
    c->profile_uploads += 1;
  }
  s.prof_fixed = true;
  return WAYNE_OK;
}

int wayne_exposure_fetch_profile(wayne_ctx* c, int slot) {
  Slot* sp;
  if (int rc = ex_gate(c, slot, "fetch_profile", EX_ON | EX_VAR | EX_OPT | EX_PROF, "no profile delivery set for the slot", &sp)) return rc;
  Slot& s = *sp;
  if (!s.prof_valid || s.ran) return fail(c, WAYNE_E_STATE, "fetch_profile: run, then wait_spectra or download_spectra first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t bytes = profile_count(c, s) * sizeof(double);
  s.prof_fetched = false;
  if (!s.prof_pinned.reserve(std::max<size_t>(bytes, 8))) return fail(c, WAYNE_E_NOMEM, "fetch_profile: pinned host allocation failed");
  HIP_TRY(c, hipMemcpyAsync(s.prof_pinned.p, s.prof_planes.p, bytes, hipMemcpyDeviceToHost, c->stream));
  s.prof_fetched = true;
  return WAYNE_OK;
}

int wayne_exposure_profile(wayne_ctx* c, int slot, const double** planes, size_t* count) {
  if (!planes || !count) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = ex_gate(c, slot, "profile", EX_ON | EX_VAR | EX_OPT | EX_PROF, "no profile delivery set for the slot", &sp)) return rc;
  Slot& s = *sp;
  if (!s.prof_fetched) return fail(c, WAYNE_E_STATE, "profile: fetch_profile first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *planes = (const double*)s.prof_pinned.p;
  *count = profile_count(c, s);
  return WAYNE_OK;
}

int wayne_exposure_download_crmask(wayne_ctx* c, int slot, uint16_t* mask) {
  if (!mask) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = ex_gate(c, slot, "download_crmask", EX_ON | EX_CRREJ, "no rejection set for the slot", &sp)) return rc;
  Slot& s = *sp;
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t S = (size_t)c->S;
  std::memset(mask, 0, S * S * sizeof(uint16_t));
  HIP_TRY(c, hipMemcpyAsync(mask + (size_t)s.cr_lo * S, s.cr_mask.as<uint16_t>() + (size_t)s.cr_lo * S,
                            (size_t)(s.cr_hi - s.cr_lo) * S * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WAYNE_OK;
}

int wayne_extract_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_EXTRACT, launches, ms); }

// ---------------------------------------------------------------------------
// device-side FITS words
// ---------------------------------------------------------------------------
int wayne_fits_layout(int S, int R, uint32_t out_flags, size_t* plane_bytes, size_t* stride, int* bitpix) {
  return fits_layout(S, R, out_flags, plane_bytes, stride, bitpix) ? WAYNE_OK : WAYNE_E_INVALID;
}

int wayne_exposure_set_fits(wayne_ctx* c, int slot, int on) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_fits", &sp)) return rc;
  Slot& s = *sp;
  s.fits_on = false;           // from here on a refusal leaves the slot usable, without FITS words
  s.fits_pinned.misc = nullptr;
  if (!on) return WAYNE_OK;
  size_t pb = 0, stride = 0;
  if (!fits_layout(c->S, s.R, s.d.flags, &pb, &stride, nullptr)) return fail(c, WAYNE_E_INVALID, "set_fits: no layout for this side");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.fits_dev.reserve((size_t)(s.R + 1) * stride));
  s.fits_plane_bytes = pb;
  s.fits_stride = stride;
  s.fits_on = true;
  return WAYNE_OK;
}

int wayne_exposure_fetch_fits_async(wayne_ctx* c, int slot) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "fetch_fits_async", &sp)) return rc;
  Slot& s = *sp;
  if (!s.fits_on) return fail(c, WAYNE_E_STATE, "fetch_fits_async: no FITS words set for the slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  // (the record of the kernels' end, as wayne_exposure_fetch_async -- which has made it already when this run's reads
  // were fetched in front of the payload)
  return s.fits_pinned.fetch(c, slot, s.fits_dev.p, (size_t)(s.R + 1) * s.fits_stride, !(s.pinned.misc && s.pinned.run == s.run_no),
                             "fetch_fits_async: pinned host allocation failed");
}

int wayne_exposure_wait_fits(wayne_ctx* c, int slot, void** host_payload) {
  if (!host_payload) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "wait_fits", &sp)) return rc;
  Slot& s = *sp;
  if (!s.fits_on) return fail(c, WAYNE_E_STATE, "wait_fits: no FITS words set for the slot");
  if (!s.fits_pinned.fetched()) return fail(c, WAYNE_E_STATE, "wait_fits: fetch_fits_async first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *host_payload = s.fits_pinned.buf.p;
  const uint32_t first_run = s.fits_pinned.run;
  bool reran = false;                        // (the status word came with the payload)
  int rc = look_at_status(c, slot, s.fits_pinned.misc, wayne_exposure_run, &reran, s.fits_pinned.run);
  if (rc || !reran) return rc;
  if ((rc = wayne_exposure_fetch_fits_async(c, slot))) return rc;     // a bin beyond the lanes' reach: once more, with k_throw
  // (reads and spectra fetched beside the payload are those of the first run: fetched again too)
  if (s.pinned.misc && s.pinned.run == first_run && (rc = wayne_exposure_fetch_async(c, slot))) return rc;
  if (s.extract_on && s.ex_pinned.misc && (rc = wayne_exposure_fetch_spectra_async(c, slot))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *host_payload = s.fits_pinned.buf.p;
  return look_at_status(c, slot, s.fits_pinned.misc, nullptr, nullptr, s.fits_pinned.run);
}

int wayne_exposure_download_fits(wayne_ctx* c, int slot, void* out_payload) {
  if (!out_payload) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download_fits", &sp)) return rc;
  Slot& s = *sp;
  if (!s.fits_on) return fail(c, WAYNE_E_STATE, "download_fits: no FITS words set for the slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  return download_settled(c, slot, out_payload, s.fits_dev.p, (size_t)(s.R + 1) * s.fits_stride);
}

int wayne_fits_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_FITS, launches, ms); }

// ---------------------------------------------------------------------------
// the noise-free expected image
// ---------------------------------------------------------------------------
int wayne_exposure_set_expected(wayne_ctx* c, int slot, int mode) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_expected", &sp)) return rc;
  Slot& s = *sp;
  s.expect_mode = 0;           // from here on a refusal leaves the slot usable, without the expected image
  if (mode == 0) return WAYNE_OK;
  if (mode != WAYNE_EXPECT_COUNTS && mode != WAYNE_EXPECT_MEAN) return fail(c, WAYNE_E_INVALID, "set_expected: mode");
  if (s.d.rng_mode == WAYNE_RNG_REPLAY)
    return fail(c, WAYNE_E_INVALID, "set_expected: replay mode reproduces the reference, which has no expected image");
  if (s.R > kExpectMaxReads) return fail(c, WAYNE_E_INVALID, "set_expected: more than 16 reads");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.expect_plane.reserve((size_t)s.R * c->S * c->S * sizeof(double)));
  s.expect_mode = mode;
  return WAYNE_OK;
}

int wayne_exposure_download_expected(wayne_ctx* c, int slot, double* out) {
  if (!out) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download_expected", &sp)) return rc;
  Slot& s = *sp;
  if (!s.expect_mode) return fail(c, WAYNE_E_STATE, "download_expected: no expected image set for the slot");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  return download_settled(c, slot, out, s.expect_plane.p, (size_t)s.R * c->S * c->S * sizeof(double));
}

int wayne_expected_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_EXPECT, launches, ms); }

// ---------------------------------------------------------------------------
// the ramp fit
// ---------------------------------------------------------------------------
int wayne_exposure_set_rampfit(wayne_ctx* c, int slot, const wayne_rampfit_desc* desc) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_rampfit", &sp)) return rc;
  Slot& s = *sp;
  s.rampfit_on = s.rampfit_ran = false;   // from here on a refusal leaves the slot usable, without the fit
  if (!desc) return WAYNE_OK;
  if (const char* why = plan::rampfit_desc_error(desc->steps, desc->read_noise_e, desc->k_jump, desc->saturation_dn))
    return fail(c, WAYNE_E_INVALID, std::string("set_rampfit: ") + why);
  if (s.R < 1 || s.R > kMaxReads) return fail(c, WAYNE_E_INVALID, "set_rampfit: n_reads outside 1 .. 15");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.rampfit_planes.reserve((size_t)c->S * c->S * (2 * sizeof(double) + sizeof(uint32_t))));
  s.rampfit = *desc;
  s.rampfit_on = true;
  return WAYNE_OK;
}

int wayne_exposure_download_rampfit(wayne_ctx* c, int slot, double* rate, double* var, uint32_t* word) {
  if (!rate || !var || !word) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download_rampfit", &sp)) return rc;
  Slot& s = *sp;
  if (!s.rampfit_on) return fail(c, WAYNE_E_STATE, "download_rampfit: no ramp fit set for the slot");
  if (!s.rampfit_ran) return fail(c, WAYNE_E_STATE, "download_rampfit: run first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t SS = (size_t)c->S * c->S;
  const double* dev = s.rampfit_planes.as<double>();
  return download_settled(c, slot, [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(rate, dev, SS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(var, dev + SS, SS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(word, dev + 2 * SS, SS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return WAYNE_OK;
  });
}

int wayne_rampfit_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_RAMPFIT, launches, ms); }

// ---------------------------------------------------------------------------
// the calibrated reads
// ---------------------------------------------------------------------------
static_assert(WAYNE_IMA_RATE == 1 && WAYNE_IMA_COUNTS == 2, "plan::ima_desc_error takes the units as 1 and 2");

int wayne_ima_layout(int S, int R, size_t* sci_stride, size_t* dq_stride, size_t* imset_stride) {
  return plan::ima_layout(S, R, sci_stride, dq_stride, imset_stride) ? WAYNE_OK : WAYNE_E_INVALID;
}

int wayne_exposure_set_ima(wayne_ctx* c, int slot, const wayne_ima_desc* desc) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_ima", &sp)) return rc;
  Slot& s = *sp;
  s.ima_on = s.ima_ran = false;   // from here on a refusal leaves the slot usable, without the calibrated reads
  if (!desc) return WAYNE_OK;
  if (const char* why = plan::ima_desc_error(desc->steps, desc->units, desc->read_noise_e, desc->saturation_dn))
    return fail(c, WAYNE_E_INVALID, std::string("set_ima: ") + why);
  size_t sci = 0, dq = 0, imset = 0;
  if (!plan::ima_layout(c->S, s.R, &sci, &dq, &imset)) return fail(c, WAYNE_E_INVALID, "set_ima: more than 16 reads, or no layout for this side");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, s.ima_dev.reserve((size_t)(s.R + 1) * imset));
  s.ima_sci_stride = sci; s.ima_dq_stride = dq; s.ima_imset_stride = imset;
  s.ima = *desc;
  s.ima_on = true;
  return WAYNE_OK;
}

int wayne_exposure_download_ima(wayne_ctx* c, int slot, void* payload) {
  if (!payload) return WAYNE_E_INVALID;
  Slot* sp;
  if (int rc = slot_gate(c, slot, "download_ima", &sp)) return rc;
  Slot& s = *sp;
  if (!s.ima_on) return fail(c, WAYNE_E_STATE, "download_ima: no calibrated reads set for the slot");
  if (!s.ima_ran) return fail(c, WAYNE_E_STATE, "download_ima: run first");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  return download_settled(c, slot, payload, s.ima_dev.p, (size_t)(s.R + 1) * s.ima_imset_stride);
}

int wayne_ima_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_IMA, launches, ms); }

// ---------------------------------------------------------------------------
// inter-pixel capacitance
// ---------------------------------------------------------------------------
int wayne_ipc_weights(const wayne_ipc_desc* d, int32_t w[9]) {
  if (!d || !w) return WAYNE_E_INVALID;
  return plan::ipc_weights(&d->k[0][0], w) ? WAYNE_OK : WAYNE_E_INVALID;
}

int wayne_exposure_set_ipc(wayne_ctx* c, int slot, const wayne_ipc_desc* desc) {
  Slot* sp;
  if (int rc = slot_gate(c, slot, "set_ipc", &sp)) return rc;
  Slot& s = *sp;
  s.ipc_on = false;               // from here on a refusal leaves the slot usable, without the coupling
  if (!desc) return WAYNE_OK;
  if (s.d.rng_mode == WAYNE_RNG_REPLAY)
    return fail(c, WAYNE_E_INVALID, "set_ipc: replay mode reproduces the reference, which has no inter-pixel capacitance");
  int32_t w[9];
  if (!plan::ipc_weights(&desc->k[0][0], w))
    return fail(c, WAYNE_E_INVALID, "set_ipc: neighbour weights must be finite, >= 0 and sum to at most 1");
  (void)hipSetDevice(c->device);
  use_slot_stream(c, slot);
  const size_t SS = (size_t)c->S * c->S;
  const size_t acc_bytes = (size_t)s.R * SS * sizeof(long long), seg_bytes = ((SS + 63) / 64) * sizeof(uint32_t);
  // (zeroed when allocated, on the slot's stream; from then on k_ramp leaves both clean)
  if (s.acc_b.cap < acc_bytes) {
    HIP_TRY(c, s.acc_b.reserve(acc_bytes));
    HIP_TRY(c, hipMemsetAsync(s.acc_b.p, 0, s.acc_b.cap, c->stream));
  }
  if (s.seg_b.cap < seg_bytes) {
    HIP_TRY(c, s.seg_b.reserve(seg_bytes));
    HIP_TRY(c, hipMemsetAsync(s.seg_b.p, 0, s.seg_b.cap, c->stream));
  }
  for (int i = 0; i < 9; ++i) s.ipc_w[i] = w[i];
  s.ipc_on = true;
  return WAYNE_OK;
}

int wayne_ipc_profile(wayne_ctx* c, uint64_t* launches, double* ms) { return kernel_profile(c, PK_IPC, launches, ms); }

uint32_t wayne_source_seed(uint32_t seed, uint32_t tag) {
  if (tag == 0) return seed;
  return philox4x32_10(tag, 0u, 0u, 0u, seed, STAGE_SOURCE).v[0];
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
int wayne_profile_enable(wayne_ctx* c, int on) {
  if (!c) return WAYNE_E_INVALID;
  c->prof_on = on != 0;
  return WAYNE_OK;
}

int wayne_profile_select(wayne_ctx* c, unsigned mask) {
  if (!c) return WAYNE_E_INVALID;
  c->prof_mask = mask;
  return WAYNE_OK;
}

int wayne_profile_reset(wayne_ctx* c) {
  if (!c) return WAYNE_E_INVALID;
  int rc = collect_profile(c);
  if (rc) return rc;
  for (int i = 0; i < kProfKernels; ++i) { c->prof_launches[i] = 0; c->prof_ms[i] = 0; }
  c->electrons = 0;
  HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, kCounterBytes, c->streams[0]));
  return sync_all(c);
}

int wayne_profile_get(wayne_ctx* c, wayne_profile* out) {
  if (!c || !out) return WAYNE_E_INVALID;
  int rc = collect_profile(c);
  if (rc) return rc;
  for (int i = 0; i < WAYNE_PROF_KERNELS; ++i) {
    out->name[i] = kProfNames[i];
    out->launches[i] = c->prof_launches[i];
    out->ms[i] = c->prof_ms[i];
  }
  unsigned long long words[kCounterStripes * kCounterStride], dev = 0;
  HIP_TRY(c, hipMemcpy(words, c->counters.p, sizeof words, hipMemcpyDeviceToHost));
  for (int i = 0; i < kCounterStripes; ++i) dev += words[i * kCounterStride];
  out->electrons = c->electrons + dev;
  return WAYNE_OK;
}

void wayne_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const u32x4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}

void wayne_host_sample_draws(uint32_t seed, uint32_t exposure, int n_samples, double* z_x, double* z_y,
                             int32_t* rand_seed) {
  for (int k = 0; k < n_samples; ++k) {
    const u32x4 w = philox4x32_10((uint32_t)k, 0u, 0u, exposure, seed, STAGE_HOST);
    const double ua = u01d(w.v[0]), ub = u01d(w.v[1]);
    const double R = std::sqrt(-2.0 * std::log(ub));
    const double ang = 6.283185307179586476925 * ua;
    if (z_x) z_x[k] = R * std::cos(ang);
    if (z_y) z_y[k] = R * std::sin(ang);
    if (rand_seed) rand_seed[k] = (int32_t)uint_below(w.v[2], 100000u);
  }
}

}  // extern "C"

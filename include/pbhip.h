/* pbhip.h -- C ABI of libpbhip.so: MI355X (gfx950) kernels for the Pyrat Bay
 * line-by-line opacity + radiative-transfer hot path.
 *
 * Every entry point replaces one native function of the reference (pyratbay v2.0.1,
 * CPython extension modules under src_c/, file:line cited per function) or one
 * per-layer / per-impact-parameter Python loop around it.  The reference has no
 * C-level API of its own (each function parses a PyObject* tuple); this header is
 * the interface a binding (ctypes stub in INTEGRATION.md) attaches to.
 *
 * Conventions
 *   - `_d` pointers are DEVICE memory (hipMalloc / torch.cuda), `_h` pointers are
 *     HOST memory.  All arrays are C-contiguous; doubles are binary64; integer
 *     arrays are int32 (the reference reads/writes C `int` through the NumPy stride,
 *     src_c/include/ind.h:31-37).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous with respect to the host unless stated otherwise.
 *   - Return value: PB_OK (0) or a negative PB_ERR_* code; pb_last_error() returns a
 *     thread-local message.  The library never calls exit() and has no CPU fallback:
 *     without a usable GPU every compute entry fails with PB_ERR_HIP.
 *
 * The Python binding reads THIS FILE (pyratbay_amd/_capi.py): constants, struct layouts and
 * prototypes exist nowhere else, so a new entry point is declared here and nowhere in Python.  The
 * reader takes a subset of C and refuses everything else:
 *   - comments in this style only; #include <stdint.h>; #ifdef / #ifndef / #endif of PBHIP_H,
 *     __cplusplus (around the extern "C" braces only) and PB_EXPERIMENTS (entries bound only when
 *     the loaded library exports them); no #if, #else, line continuations or function-like macros;
 *   - #define NAME <integer>: decimal or hex, negative, with or without parentheses;
 *   - typedef struct pb_x pb_x; (a handle) and typedef struct pb_x { ... } pb_x; with fields of
 *     int, int16_t, int32_t, int64_t, uint64_t, uint8_t, double or a pointer to one of those, to void or
 *     to a struct declared above; several declarators per statement; arrays of one or two
 *     dimensions, of pointers too, whose bounds are integers or constants defined in this file;
 *   - functions that return int, int64_t, void or const char *, with named parameters of the
 *     scalar types above, `const char *` / `char *` (strings), or any other pointer, pointer to
 *     pointer or array parameter (`int64_t stats[3]`) of the types above.
 * No float, no unions, no nested or anonymous structs, no bit fields, no function pointers, no
 * struct passed or returned by value.  An entry that returns int returns a status unless
 * _capi.INT_QUERIES names it.
 */
#ifndef PBHIP_H
#define PBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PB_OK 0
#define PB_ERR_ARG (-1)         /* invalid argument / shape                      */
#define PB_ERR_HIP (-2)         /* HIP runtime error (message has the detail)    */
#define PB_ERR_UNSUPPORTED (-3) /* valid in the reference, not supported here    */
#define PB_ERR_NOMEM (-4)

const char *pb_last_error(void);
int pb_version(void);
int pb_device_count(int *count);
int pb_set_device(int device);

/* =========================================================================
 * Stage timers and profiler ranges  (Pyrat.timestamps['extinction'|'odepth'|'spectrum'],
 * pyratbay/pyrat/pyrat_obj.py:203-214 with the Timer of pyratbay/tools/tools.py:832-843)
 * ========================================================================= */
typedef struct pb_timer pb_timer;

/* A timer holds max_stages + 1 HIP events.  pb_timer_start records the first one on `stream`
 * (and opens a rocTX range `first_stage` when not NULL); pb_timer_mark records the END of the
 * stage `name` and opens the range of `next_stage` (NULL: none).  Entry points that fuse two of
 * the reference's stages (pb_transit_spectrum*: optical depth, then transmission) mark the
 * boundary themselves on the timer most recently started by the calling thread, under the
 * reference's stage name ("odepth").  Nothing synchronises until pb_timer_read, which waits for
 * the stage's closing event and returns its duration in seconds. */
int pb_timer_create(pb_timer **out, int max_stages);
int pb_timer_start(pb_timer *t, const char *first_stage, void *stream);
int pb_timer_mark(pb_timer *t, const char *name, const char *next_stage, void *stream);
int pb_timer_count(const pb_timer *t, int *nstages);
int pb_timer_read(pb_timer *t, int stage, char *name_out, int name_cap, double *seconds);
void pb_timer_destroy(pb_timer *t);
/* rocTX ranges for rocprofv3 --marker-trace (no-ops when the marker library is absent) */
int pb_range_push(const char *name);
int pb_range_pop(void);
int pb_roctx_available(void);

/* =========================================================================
 * Voigt profile table  (vprofile.grid, src_c/vprofile.c:42-114;
 *                       voigtn/voigtxy, src_c/include/voigt.h:147-359)
 * ========================================================================= */
typedef struct pb_voigt pb_voigt;

/* Build the table on the device from the width grids and the requested half-sizes
 * (psize_h[nlor*ndop]; 0 = alias the previous Doppler column, vprofile.c:100-104).
 * `dwn` is the fine-grid step (spec.ownstep), `osamp` the oversampling factor
 * (spec.wnosamp) that fixes the phase-major device layout used by the extinction
 * kernel.  keep_flat: 0 = phase-major layout only (constant-step plans), 1 = also the
 * reference layout (vprofile.grid's `profile`), 2 = the reference layout ONLY: what a plan of
 * the `resolution` / `wlstep` mode reads (utils.h:139-163) -- no second copy of the table.
 * Synchronous. */
int pb_voigt_create(pb_voigt **out, const double *lorentz_h, int nlor,
                    const double *doppler_h, int ndop, const int32_t *psize_h,
                    double dwn, int osamp, int keep_flat, void *stream);
/* Wrap an existing reference-layout table (what vprofile.grid returned) held on the
 * host: uploads it and derives the phase-major layout.  psize_h/pindex_h are the
 * arrays as left by vprofile.grid. */
int pb_voigt_from_flat(pb_voigt **out, const double *profile_h, int64_t nprofile,
                       const double *lorentz_h, int nlor, const double *doppler_h,
                       int ndop, const int32_t *psize_h, const int32_t *pindex_h,
                       int osamp, int keep_flat, void *stream);
/* Outputs of vprofile.grid: final half-sizes, start indices, number of samples. */
int pb_voigt_meta(const pb_voigt *v, int32_t *psize_h, int32_t *pindex_h,
                  int64_t *nprofile);
/* Reference-layout table (concatenated profiles) copied to host memory. */
int pb_voigt_flat_to_host(pb_voigt *v, double *profile_h, int64_t nprofile);
int64_t pb_voigt_device_bytes(const pb_voigt *v);
void pb_voigt_destroy(pb_voigt *v);

/* =========================================================================
 * Line list  (arrays read by _extcoeff.extinction, src_c/_extcoeff.c:87-123;
 *             TLI reader pyratbay/pyrat/line_by_line.py:298-482)
 * ========================================================================= */
typedef struct pb_lines pb_lines;

/* Upload a line list and pre-compute what depends only on (lwn, lID, own): the
 * in-range mask, the nearest fine-grid index of each line (_extcoeff.c:243-245) and
 * the greedy co-add groups (_extcoeff.c:248-262).  own_h may be NULL, in which case
 * own[i] = own0 + i*ownstep is generated exactly as NumPy does
 * (pyratbay/pyrat/spectrum.py:222). */
int pb_lines_create(pb_lines **out, const double *lwn_h, const double *elow_h,
                    const double *gf_h, const int32_t *lid_h, int64_t nlines, int niso,
                    const double *own_h, int64_t onwn, double own0, double ownstep);
/* stats[0]=lines in range, [1]=groups, [2]=co-added lines (nadd of _extcoeff.c:256) */
int pb_lines_stats(const pb_lines *l, int64_t stats[3]);
/* flag = 1 when the co-add groups were built on the device (lists in TLI order: isotope, then
 * wavenumber), 0 when the host loop did it (any other order, or PB_LINES_HOST=1). */
int pb_lines_grouped_on_device(const pb_lines *l, int *flag);
/* The co-add groups in (isotope, fine index) order: first line, number of lines, nearest
 * fine-grid index of the leader [ngroups each], and the first group of every isotope
 * [niso + 1].  Any pointer may be NULL. */
int pb_lines_groups(const pb_lines *l, int32_t *first_h, int32_t *count_h, int32_t *iown_h,
                    int64_t *iso_gstart_h);
void pb_lines_destroy(pb_lines *l);

/* =========================================================================
 * Line-by-line extinction for ALL layers in one call
 * (replaces the per-layer loop pyratbay/pyrat/extinction.py:170-213 around
 *  _extcoeff.extinction, src_c/_extcoeff.c:87-345)
 * ========================================================================= */
typedef struct pb_lbl pb_lbl;

int pb_lbl_create(pb_lbl **out, pb_voigt *voigt, pb_lines *lines,
                  const double *wn_h, int nwave,
                  const int32_t *divisors_h, int ndivs,
                  const double *molrad_h, const double *molmass_h, int nmol,
                  const int32_t *isoimol_h, const double *isomass_h,
                  const double *isoratio_h, const int32_t *isoiext_h, int niso,
                  double cutoff, double ethresh, int resolution, int max_layers);
/* Change the species-selection flags (isoiext < 0 = neglect; extinction.py:164-167) */
int pb_lbl_set_isoiext(pb_lbl *p, const int32_t *isoiext_h);
int pb_lbl_set_ethresh(pb_lbl *p, double ethresh);
/* Gather-kernel selection for constant-step grids.
 *   0 = automatic: layers whose phase-major profile blocks fit in LDS (narrow profiles) run
 *       the resident-profile kernel; the others run the LDS-staged kernel when several lines
 *       share a phase row of a tile, else the global gather;
 *   1 = global gather only, 2 = LDS-staged only (falls back to 1 when a phase row does not
 *       fit in LDS), 3 = resident-profile kernel where it applies + global gather,
 *   4, 5, 7 = measured dead ends (scatter, rounds, wave: see "Experiments" at the end of this
 *       header): refused by libpbhip.so, selectable in libpbhip_exp.so.
 * All sum the same terms; only the order differs (global, resident: isotope, position;
 * staged: isotope, phase, position).  In mode 0 the choice depends on the size of the launch
 * (layers x samples); with a fixed mode every tiling and sharding adds the same terms in the
 * same order, so shards concatenate bit-exactly.
 * Plans of the `resolution` mode (pb_lbl_create(resolution = 1)): any mode but 6 = the direct
 * gather (two reference-layout table reads per (line, output): no set-up, what a one-off call
 * wants); 6 = per-layer dynamic grids: the grid a layer's lines are summed on in the reference
 * (step = ofactor fine samples, _extcoeff.c:185-195, 281-307) is a constant-step grid, so one
 * constant-step sub-plan per factor in use (created on first use and kept, with the Lorentz rows
 * of the Voigt table its layers read re-cut into phase rows modulo the factor -- all factors
 * together about one more copy of the table) computes it with the staged kernels and the outputs
 * are interpolated from it as utils.h:139-163 does.  Same terms, summed in the staged order (~1e-16
 * of the direct gather).  Reads the layers' factors back: one stream synchronisation per call
 * (such a call cannot be captured into a HIP graph) and deals the runs of layers to side streams
 * of its own that join the caller's stream before the call returns.
 * Two-phase shard calls of such a plan use the direct gather.
 * last_gather_mode reports what the last call ran: 1 global, 2 staged, 3 resolution mode (direct
 * gather), 6 resolution mode through dynamic grids, plus 8 when the resident-profile kernel ran
 * as well. */
int pb_lbl_set_gather_mode(pb_lbl *p, int mode);
int pb_lbl_last_gather_mode(const pb_lbl *p, int *mode);
/* Hint: the caller keeps n independent calls in flight on n streams (the reference's callers
 * with independent spectra: the temperature loop of pyrat/extinction.py:100-122, the walkers of
 * a retrieval; here also the pipelined shards of a multi-GPU rank).  Changes only how a small
 * launch is tiled (fewer, longer workgroups: the other streams fill the chip), never a term. */
int pb_lbl_set_concurrency(pb_lbl *p, int n);
/* Out-of-core line lists.  The reference walks any number of lines sequentially
 * (src_c/_extcoeff.c:203-309; the "computer-intensive" opacity-table run,
 * pyratbay/pyrat/extinction.py:100-122, reads whole line databases).  Here a call keeps one
 * 16-byte record per (layer, co-add group); when those exceed `bytes` (default 96 GiB) the call
 * is made in chunks of the line list: one pass for the per-species maxima of all lines
 * (_extcoeff.c:203-226), then per chunk the records and a gather that continues the running
 * sums -- the same terms in the same order as an unchunked call with one workgroup per tile
 * (PB_STAGE_SPLIT=1), hence bit-identical to it.  last_chunks: chunks of the last call (0 = none). */
int pb_lbl_set_record_budget(pb_lbl *p, int64_t bytes);
int pb_lbl_last_chunks(const pb_lbl *p, int *chunks);
/* ext_d[nlayers, nrows, wcount] with nrows = 1 if add else (max isoiext)+1, for the
 * output samples [wbegin, wbegin+wcount) of the global grid (wavenumber shard).
 * temp_d[nlayers]; dens_d[nlayers, nmol]; isoz_d element (i,l) at
 * isoz_d[i*z_iso_stride + l*z_layer_stride].  Resample mode assigns, resolution
 * (linterp) mode accumulates into ext_d, like the reference. */
int pb_lbl_extinction(pb_lbl *p, double *ext_d, int64_t wbegin, int64_t wcount,
                      const double *temp_d, const double *dens_d, const double *isoz_d,
                      int64_t z_iso_stride, int64_t z_layer_stride, int nlayers, int add,
                      void *stream);
/* Diagnostics of the last call, copied to host (synchronises the stream):
 * ofactor_h[nlayers] (dynamic-sampling factor, _extcoeff.c:195) and
 * kmax_h[nlayers*nrows] (per-species maximum line strength, :225). */
int pb_lbl_last_state(pb_lbl *p, int32_t *ofactor_h, double *kmax_h, int nlayers,
                      int nrows, void *stream);
/* Which layers of the last call the resident-profile kernel computed (resident_h[nlayers],
 * 0/1; all 0 when that kernel was off) and the size in doubles of the largest phase-major
 * profile block each layer can select (block_h[nlayers]).  Synchronises the stream. */
int pb_lbl_last_layer_kinds(pb_lbl *p, int32_t *resident_h, int32_t *block_h, int nlayers,
                            void *stream);
/* Rows per barrier step of the LDS-staged gather.  Its row area holds two rows of `rowlds`
 * samples (the longest row of the table, at most 1024) between zero pads of 256; where the rows
 * of a (layer, isotope) are at most `rowlim` samples long and four or more slots of pitch
 * rowlim + 256 (rounded down to even) fit the same area, a step stages and walks R = min(2, slots / 2)
 * consecutive segments instead of one -- the same terms in the same order, fewer barriers.
 * rows_per_step returns R and, when `pitch` is not null, the slot pitch in samples; it makes no
 * HIP call.  last_rows_per_step: R of every (layer, isotope) of the last call
 * (rows_h[nlayers * niso]; all 1 when that call did not run the staged gather, or ran it with
 * PB_STAGE_ROWS=1, with rows via registers or with chunked long rows).  Synchronises the stream. */
int pb_lbl_rows_per_step(int rowlds, int rowlim, int *pitch);
int pb_lbl_last_rows_per_step(pb_lbl *p, int32_t *rows_h, int nlayers, int niso, void *stream);
/* The same call in two halves, for wavenumber shards on several GPUs. _begin derives the layer
 * state and the records of the groups within reach of the shard, with the per-row maxima
 * (_extcoeff.c:203-226) over THOSE groups only -- 1/N of the exp() work; the caller then
 * all-reduces (MAX) the buffer pb_lbl_kmax_buffer returns over the ranks -- count 64-bit words
 * holding the bit patterns of non-negative doubles, which order like integers -- and _end runs
 * the gather with the global maxima (ethresh * kmax is then the same threshold on every rank). */
int pb_lbl_extinction_begin(pb_lbl *p, double *ext_d, int64_t wbegin, int64_t wcount,
                            const double *temp_d, const double *dens_d, const double *isoz_d,
                            int64_t z_iso_stride, int64_t z_layer_stride, int nlayers, int add,
                            void *stream);
int pb_lbl_kmax_buffer(pb_lbl *p, void **kmax_d, int64_t *count);
int pb_lbl_extinction_end(pb_lbl *p, void *stream);
/* Work of the last pb_lbl_extinction call, counted on the device from its per-(layer, group)
 * records: work[0] = profile samples multiplied (the FMAs _extcoeff.c:302-307 keeps after
 * resampling), work[1] = lanes the LDS-staged kernels issue for them (256-sample spans),
 * work[2] = live records.  All -1 when the last launch kept no packed records. */
int pb_lbl_last_work(pb_lbl *p, int64_t work[3], void *stream);
/* Diagnostics: distinct Voigt-table samples the live records of the last extinction call select
 * (per (layer, isotope, Doppler column, phase) row the longest window taken from it) -- what any
 * evaluation of _extcoeff.c:302-307 must read of `profile` at least once.  -1 when the last
 * launch kept no packed one-piece records. */
int pb_lbl_last_table_samples(pb_lbl *p, int64_t *samples, void *stream);
/* Per-launch timing of the gather kernel with HIP events on the call's stream:
 * begin() arms up to max_launches start/stop pairs, every following
 * pb_lbl_extinction records one pair around its gather launch, end() returns the summed
 * kernel time and the number of launches (used by bench.py for the roofline figure). */
int pb_lbl_timing_begin(pb_lbl *p, int max_launches);
int pb_lbl_timing_end(pb_lbl *p, double *total_ms, int *launches);
void pb_lbl_destroy(pb_lbl *p);

/* =========================================================================
 * Cross-section table interpolation (_extcoeff.interp_ec / interp_ec_per_mol,
 * src_c/_extcoeff.c:367-472).  etable_d[nmol,ntemp,nlayers,nwave]; ttable_d[ntemp];
 * temperatures_d[nlayers];
 * density_d[nlayers,nmol]; accumulates into extinction_d[nlayers,nwave]
 * (per_mol: [nmol,nlayers,nwave]) for layers lay1 <= k < min(lay2,nlayers).
 * ========================================================================= */
int pb_interp_ec(double *extinction_d, const double *etable_d, const double *ttable_d,
                 const double *temperatures_d, const double *density_d, int nmol,
                 int ntemp, int nlayers, int nwave, int lay1, int lay2, int per_mol,
                 void *stream);
/* Same, but the rows lay1 <= k < min(lay2,nlayers) are ASSIGNED (= 0 + the sum) instead of
 * accumulated into: for callers that would zero the array first (the retrieval loop,
 * opacity/line_sampling.py:438-456 after `self.ec = np.zeros(...)`): saves that pass and
 * the read of `extinction`. */
int pb_interp_ec_set(double *extinction_d, const double *etable_d, const double *ttable_d,
                     const double *temperatures_d, const double *density_d, int nmol,
                     int ntemp, int nlayers, int nwave, int lay1, int lay2, int per_mol,
                     void *stream);

/* =========================================================================
 * Optical depth
 * ========================================================================= */
/* One impact parameter: _trapezoid.optdepth (src_c/_trapezoid.c:238-276).
 * data_d[(nint+1), nwave] rows row_stride elements apart. */
int pb_optdepth(double *tau_d, const double *data_d, int64_t row_stride,
                const double *intervals_d, int nint, double taumax, int32_t *ideep_d,
                int ilay, int nwave, void *stream);
/* All impact parameters in one launch: the loop of
 * pyratbay/opacity/optic_depth.py:103-112 including the final
 * `ideep[ideep<0] = r`.  raypath_d is the packed lower triangle of
 * atmosphere.transit_path(radius, itop): row r (itop<=r<nlayers) has r-itop
 * entries starting at ((r-itop)*(r-itop-1))/2.  depth_d[nlayers,nwave] is fully
 * written (rows outside [itop,ibottom) and below ideep are zero). */
int pb_optical_depth_transit(double *depth_d, int32_t *ideep_d, const double *ec_d,
                             const double *raypath_d, int itop, int ibottom,
                             double maxdepth, int nlayers, int nwave, void *stream);
/* Same loop fused with radiative_transfer.transmission (no cloud deck,
 * pyratbay/spectrum/radiative_transfer.py:57-71): depth_d and ideep_d as above, plus
 * spectrum_d[nwave] = (r_top^2 + 2*integral)/rstar^2 computed in the pass that resolves
 * the early exit. */
int pb_transit_spectrum(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                        const double *ec_d, const double *raypath_d, const double *radius_d,
                        double rstar, int itop, int ibottom, double maxdepth, int nlayers,
                        int nwave, void *stream);
/* _trapezoid.plane_parallel_optical_depth (src_c/_trapezoid.c:175-213); rows below
 * the stopping layer are left as passed in, like the reference. */
int pb_plane_parallel_optical_depth(double *depth_d, int32_t *ideep_d,
                                    const double *ec_d, const double *intervals_d,
                                    double maxdepth, int itop, int ibottom, int nlayers,
                                    int nwave, void *stream);

/* =========================================================================
 * Spectrum integrals
 * ========================================================================= */
/* _trapezoid.trapezoid2D (src_c/_trapezoid.c:70-90): data_d[nrows,nwave] */
int pb_trapezoid2D(double *out_d, const double *data_d, const double *intervals_d,
                   const int32_t *nint_d, int nrows, int nwave, void *stream);
/* Fused transmission spectrum = radiative_transfer.transmission without cloud deck
 * (pyratbay/spectrum/radiative_transfer.py:57-71): exp(-depth)*r, trapezoid2D over
 * ideep-itop intervals, (r_top^2 + 2*integral)/rstar^2. */
int pb_transmission(double *spectrum_d, const double *depth_d, const int32_t *ideep_d,
                    const double *radius_d, int itop, double rstar, int nlayers,
                    int nwave, void *stream);
/* _blackbody.blackbody_wn_2D / blackbody_wn (src_c/_blackbody.c:35-130);
 * last_d may be NULL. */
int pb_blackbody_wn_2D(double *B_d, const double *wn_d, int nwave, const double *temp_d,
                       int nlayers, const int32_t *last_d, void *stream);
int pb_blackbody_wn(double *B_d, const double *wn_d, int nwave, double temp, void *stream);
/* _trapezoid.intensity (src_c/_trapezoid.c:304-341): out_d[nmu,nwave] */
int pb_intensity(double *out_d, const double *tau_d, const int32_t *ideep_d,
                 const double *bbody_d, const double *mu_d, int nmu, int rtop,
                 int nlayers, int nwave, void *stream);
/* Fused emission: Planck evaluated in registers (never stored), intensity per mu and
 * flux = sum_k I_k * w_k (pyratbay/pyrat/spectrum.py:366-377).  intensity_d may be
 * NULL. */
int pb_emission_flux(double *flux_d, double *intensity_d, const double *tau_d,
                     const int32_t *ideep_d, const double *wn_d, const double *temp_d,
                     const double *mu_d, const double *weights_d, int nmu, int rtop,
                     int nlayers, int nwave, void *stream);
/* Radiative transfer with an opaque cloud deck (clouds/gray.py:92-150 Deck; the optical depth
 * is then computed with ibottom = deck_itop + 1, pyrat_obj.py:134-138):
 *  - transit (radiative_transfer.py:57-71): the interval that ends at layer deck_itop ends at
 *    the cloud top instead, h = deck_rsurf - radius[deck_itop-1], with the integrand
 *    interpolated linearly in radius; deck_itop <= itop or < 0 = no deck;
 *  - emission (radiative_transfer.py:121-131): the caller passes temp_d with the cloud-top
 *    temperature at index cloud_itop (Planck of that row) and ideep is clipped to cloud_itop;
 *    cloud_itop < 0 = no deck. */
int pb_transmission_deck(double *spectrum_d, const double *depth_d, const int32_t *ideep_d,
                         const double *radius_d, int itop, double rstar, int deck_itop,
                         double deck_rsurf, int nlayers, int nwave, void *stream);
int pb_transit_spectrum_deck(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                             const double *ec_d, const double *raypath_d,
                             const double *radius_d, double rstar, int itop, int ibottom,
                             double maxdepth, int deck_itop, double deck_rsurf, int nlayers,
                             int nwave, void *stream);
int pb_emission_flux_deck(double *flux_d, double *intensity_d, const double *tau_d,
                          const int32_t *ideep_d, const double *wn_d, const double *temp_d,
                          const double *mu_d, const double *weights_d, int nmu, int rtop,
                          int cloud_itop, int nlayers, int nwave, void *stream);

/* Continuum opacity terms, accumulated into ec_d[nlayers,nwave] in ONE pass:
 *  - nrank1 terms cs_d[m][nwave] * f_d[m][nlayers]: Rayleigh (rayleigh.py:85-107, f = number
 *    density of the scatterer), Lecavelier haze (lecavelier.py:73-100, f = p/kT) and
 *    constant-cross-section gray clouds (gray.py:63-75, cs = 1, f = cs[l]*p/kT);
 *  - ncia (<= 4) collision-induced-absorption tables cia_tab_d[c] -> [ntemp_c][nwave] on the
 *    model grid, already per (molecule cm-3)^2, linear in temperature between the nodes
 *    cia_temps_d[c] with the bracket rule of _spline.c:219-260 (lin_interp_2D), columns
 *    [cia_lo[c], cia_hi[c]) only, times cia_f_d[c][nlayers] = product of the pair's
 *    densities (cia.py:119-215).  A temperature off a table gives NaN there (the reference
 *    raises ValueError; the Python front-end checks before the call).  cia_tab_d and
 *    cia_temps_d are HOST arrays of device pointers;
 *  - H- bound-free + free-free (hydrogen_ion.py:157-276, John 1988) when hm_sigma_bf_d is not
 *    NULL: hm_sigma_bf_d[nwave] (Eq. 4), hm_ff_d[6][nwave] = 1e-29 * the wavelength
 *    polynomials of Eq. 6 as rows multiplying sqrt(5040/T)^(i+2) (zero rows where a branch
 *    does not use a power), hm_f_d[nlayers] = n_H * n_e. */
int pb_continuum(double *ec_d, const double *wn_d, const double *temp_d, int nlayers, int nwave,
                 int nrank1, const double *cs_d, const double *f_d, int ncia,
                 const double *const *cia_tab_d, const double *const *cia_temps_d,
                 const int32_t *cia_ntemp, const int32_t *cia_lo, const int32_t *cia_hi,
                 const double *cia_f_d, const double *hm_sigma_bf_d, const double *hm_ff_d,
                 const double *hm_f_d, void *stream);
/* Alkali resonance doublets, src_c/_alkali.c:30-106 (alkali_cross_section): adds the cross
 * section (cm2 molecule-1) of nlines (<= 8) lines to ec_d[nlayers,nwave] -- times
 * density_d[nlayers] when that is not NULL (alkali.py:239-262).  pressure_d in barye,
 * voigt_det_d[nlayers,nlines] = Voigt value at the detuning distance (alkali.py:56-89, host). */
int pb_alkali_cross_section(double *ec_d, const double *pressure_d, const double *wn_d,
                            const double *temp_d, const double *voigt_det_d, double detuning,
                            double mass, double lorentz_par, double part_func, double cutoff,
                            const double *wn0_h, const double *gf_h, int nlines,
                            const double *density_d, int nlayers, int nwave, void *stream);

/* Gaussian log-likelihood of band-integrated models (tools/retrieval_tools.py:98-104):
 * loglike_d[w] = -0.5*sum_b ((data_d[b] - bandflux_d[w,b]) / uncert_d[b])^2
 *                -0.5*sum_b log(2*pi*uncert_d[b]^2), or -1e98 when that is not finite
 * (the reference's reject value, retrieval_tools.py:101-103). */
int pb_loglike(double *loglike_d, const double *bandflux_d, const double *data_d,
               const double *uncert_d, int nwalkers, int nbands, void *stream);

/* Two-stream fluxes (pyratbay/pyrat/spectrum.py:454-522, Heng et al. 2014 Eqs. B5-B6) from
 * the plane-parallel optical depth depth_d[nlayers,nwave] (computed with maxdepth = inf,
 * opacity/optic_depth.py:124-125): flux_down_d, flux_up_d [nlayers,nwave]; the emission
 * spectrum is flux_up_d row 0.  f_int_d[nwave] = internal flux added at the bottom (NULL =
 * none), flux_top_d[nwave] = beta_irr*(rstar/smaxis)^2*starflux written into row rtop
 * before the downward sweep, exactly like the reference (NULL = no irradiation).  exp1 is
 * scipy.special.exp1 (SciPy 1.15.3 xsf/expint.h:22-52). */
int pb_two_stream(double *flux_down_d, double *flux_up_d, const double *depth_d,
                  const double *wn_d, const double *temp_d, const double *f_int_d,
                  const double *flux_top_d, int rtop, int nlayers, int nwave, void *stream);
/* The same for a batch of walkers in ONE pass (the retrieval loop in two-stream geometry):
 * per walker w the plane-parallel optical depth of ec_d[w] without a stop (maxdepth = inf,
 * itop = 0, opacity/optic_depth.py:124-126), the transmissions and both sweeps of pb_two_stream,
 * of which only flux_up row 0 is stored: flux_d[nwalkers,nwave].  ec_d[nwalkers,nlayers,nwave]
 * is DESTROYED (the downward sweep leaves each interval's optical depth in it for the upward
 * one); intervals_d[nwalkers,nlayers-1] = -diff(radius) (NULL allowed when nlayers == 1),
 * temps_d[nwalkers,nlayers]; wn_d, f_int_d, flux_top_d [nwave] are shared by the walkers
 * (NULL = no internal flux / no irradiation).  work_d: pb_two_stream_batch_work_doubles(...)
 * doubles of device scratch, written before it is read (NULL when that is 0).  nlayers == 1:
 * flux = flux_top + f_int.  Same operations in the same order as
 * pb_plane_parallel_optical_depth + pb_two_stream per walker: same bits.  nwalkers == 0 or
 * nwave == 0: nothing is launched. */
int pb_two_stream_batch(double *flux_d, double *ec_d, const double *intervals_d,
                        const double *wn_d, const double *temps_d, const double *f_int_d,
                        const double *flux_top_d, double *work_d, int nlayers, int nwave,
                        int nwalkers, void *stream);
int64_t pb_two_stream_batch_work_doubles(int nlayers, int nwave, int nwalkers);
/* pb_two_stream_batch with the irradiation of every walker's own stellar temperature (a retrieval
 * with a free T_eff: pyrat_obj.py:288-290 updates spec.starflux, the top boundary of the downward
 * sweep, pyrat/spectrum.py:498-500): in place of flux_top_d, star_grid_d[nt,nwave] (the SED grid on
 * the model's wavenumbers), sed_temps_d[nt] (strictly ascending, nt >= 2), tstar_d[nwalkers] and
 * factor = beta_irr*(rstar/smaxis)^2.  The bracket of tstar is found once per walker and per
 * column
 *   down = factor * (slope * (t - x_lo) + y_lo),   slope = (y_hi - y_lo) / (x_hi - x_lo)
 * -- interp1d's linear rule as SciPy states it, then the multiply, every operation rounded on its
 * own -- is formed in registers: no flux_top[nwalkers,nwave] exists.  Everything else is
 * pb_two_stream_batch's kernel (one template): the bits of that entry run one walker at a time with
 * the host-formed flux_top.  DEVIATION: a walker whose tstar is NaN or outside the grid reads no
 * grid row and gets +inf in its whole flux row (the reference's interp1d raises there); its ec and
 * work rows are left untouched.  At most 65535 walkers per call. */
int pb_two_stream_batch_star(double *flux_d, double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temps_d, const double *f_int_d,
                             const double *star_grid_d, const double *sed_temps_d,
                             const double *tstar_d, double factor, int nt, double *work_d,
                             int nlayers, int nwave, int nwalkers, void *stream);
/* f_int of spectrum.py:475-478: Planck at tint scaled to a bolometric sigma*tint^4. */
int pb_internal_flux(double *f_int_d, const double *wn_d, double tint, int nwave, void *stream);

/* ---- Radiative equilibrium (Pyrat.radiative_equilibrium, pyrat/pyrat_obj.py:559-646 ->
 * spectrum/radiative_transfer.py:141-272) for a batch of profiles, at fixed volume mixing ratios:
 * pb_radeq.hip.  One iteration is pb_interp_ec_batch[_cont], pb_two_stream_net_batch and
 * pb_radeq_update, or with convection pb_radeq_update_convective; nothing is read back.  With the
 * equilibrium chemistry of every iteration (pb_radeq_equilibrium, further down) an iteration is
 * five launches: the same two, the update with temps_only, pb_radeq_equilibrium at the new
 * temperatures, and pb_radeq_update(init_only = 1) for the atmosphere of the new VMRs.
 *
 * pb_two_stream_net_batch = pb_two_stream_batch (same arguments, same bits in flux_d, ec_d
 * DESTROYED) that also integrates flux_up and flux_down of EVERY layer over wavenumber with the
 * trapezoid weights trapz_weights_d[nwave] (half the neighbouring gaps of the grid, one-sided at
 * its ends; a single sample: 0): parts_d[nwalkers, nparts, 2, nlayers], nparts =
 * pb_two_stream_net_parts(nwave), holds the sums over the columns of one part (a workgroup of 256
 * columns), [.., 0, ..] of flux_up and [.., 1, ..] of flux_down; the parts added up are
 * Qup[nlayers] and Qdown[nlayers] (radiative_transfer.py:208-209).  No atomics: two runs give
 * the same bits.  At most 744 layers (LDS).  flux_down[0] is the irradiation, flux_up[nlayers-1] = flux_down[nlayers-1] +
 * f_int.  f_int_d / flux_top_d: [nwave] shared by the profiles (stride 0) or [nwalkers, nwave]
 * (stride nwave); NULL = none. */
int pb_two_stream_net_parts(int nwave);
int64_t pb_two_stream_net_work_doubles(int nlayers, int nwave, int nwalkers);
int pb_two_stream_net_batch(double *flux_d, double *parts_d, double *ec_d,
                            const double *intervals_d, const double *wn_d,
                            const double *trapz_weights_d, const double *temps_d,
                            const double *f_int_d, int f_int_stride, const double *flux_top_d,
                            int flux_top_stride, double *work_d, int nlayers, int nwave,
                            int nwalkers, void *stream);

/* The state of pb_radeq_update; every pointer is device memory.  Iteration k = iter_d[w] of
 * profile w reads temp_d[w] (= row k of temps_d[w]) and the parts of its fluxes, and writes row
 * k + 1, temp_d[w], dt_scale_d[w], row k % 4 of signs_d[w], q_up_d[w], q_down_d[w], iter_d[w] =
 * k + 1 and the atmosphere of the next evaluation.  A launch with k + 1 >= nrows does nothing. */
typedef struct pb_radeq {
    int nlayers, nwalkers;
    int nparts;                    /* pb_two_stream_net_parts(nwave) */
    int nrows;                     /* rows of temps_d per profile: 1 + nsamples */
    double tmin, tmax;             /* np.clip of the new temperatures */
    const double *parts_d;         /* [nwalkers, nparts, 2, nlayers] */
    const double *dpress_d;        /* [nlayers] ediff1d(log p), element 0 = element 1 */
    double *temps_d;               /* [nwalkers, nrows, nlayers] history */
    double *temp_d;                /* [nwalkers, nlayers] the profile to evaluate next */
    double *dt_scale_d;            /* [nwalkers, nlayers] */
    double *signs_d;               /* [nwalkers, 4, nlayers] sign(dF) of iteration k in row k % 4 */
    int32_t *iter_d;               /* [nwalkers] */
    double *q_up_d, *q_down_d;     /* [nwalkers, nlayers] bolometric fluxes of the evaluated profile */
    /* (diagnostics, for tests: nothing in the loop reads them) */
    int32_t *wobble_d;             /* [nwalkers, nlayers] the wobbling layers, or NULL */
    double *sigma_d;               /* [nwalkers] sigma of the temperature filter, or NULL */
    /* the atmosphere: n = vmr p / (k T) (atmosphere.ideal_gas_density, pyratbay.constants) */
    const double *pressure_d;      /* [nlayers] bar, ascending */
    const double *lnp_d;           /* [nlayers] log(pressure); radius models only */
    const double *vmr_d;           /* [nwalkers or 1, nlayers, nspecies] */
    int64_t vmr_stride;            /* 0 (shared) or nlayers * nspecies */
    int nspecies;
    const double *mm_d;            /* [nwalkers or 1, nlayers] mean molecular mass; radius models only */
    int mm_stride;                 /* 0 or nlayers */
    int ntab, ncont;               /* species of dens_d / cdens_d */
    const int32_t *tab_map_d, *cont_map_d;     /* their indices among the nspecies */
    double *dens_d;                /* [nwalkers, nlayers, ntab] */
    double *cdens_d;               /* [nwalkers, nlayers, ncont] (ncont > 0) */
    int rmodel;                    /* -1: radius_d, intervals_d are not touched; 0 hydro_m; 1 hydro_g */
    int has_ref;                   /* p0, r0 given (hydro_m: always; hydro_g without: radius[-1] = 0) */
    double mplanet, gplanet;       /* g (hydro_m), cm s-2 (hydro_g) */
    double p0, r0;                 /* bar within the pressure grid (the caller's check), cm */
    double *radius_d;              /* [nwalkers, nlayers] */
    double *intervals_d;           /* [nwalkers, nlayers - 1] radius[i] - radius[i + 1] */
    int temps_only;                /* != 0 (and init_only == 0): the update ends behind the new
                                      temperatures (and the convective half); dens_d, cdens_d,
                                      radius_d and intervals_d are not touched -- the caller forms
                                      them with init_only = 1 once vmr_d and mm_d are those of the
                                      new temperatures (pb_radeq_equilibrium) */
} pb_radeq;

/* One update of every profile (radiative_transfer.py:207-237, convection=False), one workgroup per
 * profile: Qup, Qdown from the parts in a fixed order (with G = max(1, min(256 / nlayers, nparts))
 * for nlayers <= 256, else 1: G groups of ceil(nparts / G) consecutive parts, each added left to
 * right, then the groups left to right); dF = ediff1d(Qup - Qdown, to_begin=0); wobble = a
 * sign of dF that differs from one of the up to four previous iterations; dt_scale * 0.5 / 1.15,
 * clipped to [1, 1e8], gaussian_filter1d(sigma = 1.5); dT = dt_scale sign(dF) |dF|**0.1 /
 * (pc.sigma T**3 dpress); isothermal top; gaussian_filter1d(sigma = clip(mean|dT| / 10, 0.75, 2))
 * of all but the last layer; clip to [tmin, tmax]; then the densities, radius and intervals of the
 * new profile.  gaussian_filter1d is SciPy's (radius int(4 sigma + 0.5), mode 'reflect').
 * init_only != 0: only the atmosphere of temp_d (before the first evaluation).  2 <= nlayers <=
 * PB_ATM_MAX_LAYERS. */
int pb_radeq_update(const pb_radeq *state, int init_only, void *stream);

/* What pb_radeq_update_convective takes beyond the state; every pointer is device memory. */
typedef struct pb_radeq_convection {
    const double *cp_temps_d;      /* [ntemps] ascending temperatures of the heat-capacity table */
    const double *cp_table_d;      /* [nwalkers or 1, ntemps, nspecies] cp / R of every species of vmr_d */
    int64_t cp_table_stride;       /* 0 (shared) or ntemps * nspecies */
    int ntemps;
    const double *mol_mass_d;      /* [nspecies] g mol-1 */
    const double *conv_dpress_d;   /* [nlayers] ediff1d(log p), element 0 = 1 (convection.py:49) */
    double mplanet;                /* g: gravity = pc.G mplanet / radius**2 whatever the radius model */
    double coeff;                  /* alpha**2 sqrt(beta) of the mixing length */
    double *conv_flux_d;           /* [nwalkers, nlayers] out: the convective flux (erg s-1 cm-2) */
    int32_t *convective_d;         /* [nwalkers] out: 1 where the second half ran */
} pb_radeq_convection;

/* pb_radeq_update(state, 0) with the convective half of the reference's loop
 * (radiative_transfer.py:239-272, spectrum/convection.py:13-67) behind the same radiative update:
 * cp = sum(np.interp(T', cp_temps, cp_table) vmr) k / amu at the temperatures T' that update
 * produced; gravity from radius_d AS IT IS ON ENTRY (the radius the fluxes were computed with;
 * required whatever rmodel is), rho = sum(n mol_mass) amu over ALL nspecies at temp_d on entry,
 * the mean mass mm_d (required); conv_flux = coeff cp / mu rho T' sqrt(g H) clip(grad_t -
 * grad_ad, 0, inf)**1.5.  A profile whose conv_flux is 0 in every layer (a NaN is not 0) keeps the
 * radiative update, bit for bit that of pb_radeq_update.  Any other: dF = ediff1d(Q_net +
 * conv_flux), row k % 4 of signs_d holds ITS signs, the wobbling layers are taken against the same
 * previous rows, the factors 0.5 / 1.15 apply to dt_scale_d as it is on entry, and row k + 1 is
 * T + dT of that update.  hydro_g needs has_ref (radius 0 at the bottom otherwise).  2 <= nlayers
 * <= 957 (two more vectors in LDS), nspecies <= 128. */
int pb_radeq_update_convective(const pb_radeq *state, const pb_radeq_convection *conv,
                               void *stream);

/* _simpson.simps2D (src_c/_simpson.c:167-203): y_d[ny,nwave] */
int pb_simps2D(double *out_d, const double *y_d, int ny, int nwave, const double *h_d,
               const int32_t *nint_d, const double *hsum_d, const double *hratio_d,
               const double *hfactor_d, void *stream);
/* cutils.ediff (src_c/cutils.c:27-42) */
int pb_ediff(double *out_d, const double *arr_d, int n, void *stream);

/* =========================================================================
 * Band integration (first "next" row after the path):
 * PassBand.integrate (pyratbay/spectrum/spec_tools.py:193-233) for nbands pass bands:
 * bandflux_d[b] = sum over the pairs (i,i+1) of band b's contiguous index range
 * [band_start, band_start+band_count) of 0.5*(wn[i+1]-wn[i])*(y_i+y_{i+1}),
 * y_i = spectrum[i]*response_b[i-band_start].  Only pairs whose left sample lies in
 * [wbegin, wbegin+wcount) are summed, so wavenumber shards can be all-reduced;
 * spectrum_d and wn_d are indexed on the global grid.  The caller applies the band's
 * `height` (and the wl factor of photon counting through the response).
 * ========================================================================= */
int pb_band_integrate(double *bandflux_d, const double *spectrum_d, const double *wn_d,
                      const int32_t *band_start_d, const int32_t *band_count_d,
                      const double *response_d, const int64_t *response_offset_d,
                      int nbands, int64_t wbegin, int64_t wcount, void *stream);

/* =========================================================================
 * Walker-batched retrieval path (BASELINE config 5): one launch per stage for nwalkers models,
 * no per-walker host work.  Reference inner loop: pyratbay/pyrat/pyrat_obj.py:225-385.
 * ========================================================================= */
/* atmosphere.transit_path (pyratbay/atmosphere/atmosphere.py:782-802) on the device:
 * radius_d[nwalkers,nlayers] -> raypath_d[nwalkers, n(n-1)/2], n = nlayers - itop, the packed
 * lower triangle pb_optical_depth_transit takes. */
int pb_transit_path(double *raypath_d, const double *radius_d, int itop, int nlayers,
                    int nwalkers, void *stream);
/* Partition functions of the isotopes of ONE TLI database at ntemp temperatures (the layers of
 * one atmosphere, or of a batch of walkers): what Line_By_Line.__init__ prepares with
 * scipy.interpolate.interp1d(db.temp, db.iso_pf[j], kind='slinear')
 * (pyratbay/pyrat/line_by_line.py:156-158) and calc_extinction_coefficient evaluates at the
 * temperature profile on EVERY call (:219-222).  ttab_d[ntab] ascending, pf_d[niso, ntab];
 * z_d[i*z_iso_stride + t*z_t_stride] (the isoz operand of pb_lbl_extinction takes the same two
 * strides).  Bit-equal to SciPy's first-order spline (its de Boor recurrence, restated).  A
 * temperature outside [ttab[0], ttab[ntab-1]] makes interp1d raise; here NaN is written and,
 * when nbad_d is not NULL, counted there (int32, zeroed by the caller). */
int pb_iso_partition(double *z_d, int64_t z_iso_stride, int64_t z_t_stride,
                     const double *temp_d, int64_t ntemp, const double *ttab_d, int ntab,
                     const double *pf_d, int niso, int32_t *nbad_d, void *stream);
/* Loader of sampled cross sections: one species' table of one opacity file
 * (in_d[ntemp_in, nlay_in, nwave_in], cm2 molecule-1) brought onto the run's grid
 * (out_d[ntemp_out, nlay_out, nwave_out]) -- tools.interpolate_opacity
 * (pyratbay/tools/tools.py:1026-1107) as Line_Sample.__init__ calls it
 * (pyratbay/opacity/line_sampling.py:245-275).  wsel_d[nwave_out]: the kept wavenumber samples
 * of the file (window + thinning).  Per output temperature / pressure the lower bracket node
 * (tlo_d, plo_d) and the weight of the upper one (tweight_d, pweight_d; 0 = on or beyond a
 * node: constant extrapolation), prepared on the host.  resample = 0: the file's own grid,
 * values pass untouched (brackets = the nodes, weights ignored); else linear in log(cs), zeros
 * entering as exp(-230).  accumulate != 0 adds to out_d (a species spread over several files). */
int pb_resample_cross_section(double *out_d, const double *in_d, const int32_t *wsel_d,
                              const int32_t *tlo_d, const double *tweight_d,
                              const int32_t *plo_d, const double *pweight_d, int ntemp_in,
                              int nlay_in, int nwave_in, int ntemp_out, int nlay_out,
                              int nwave_out, int resample, int accumulate, void *stream);
/* interp_ec (src_c/_extcoeff.c:367-418), assigning form, for a batch: temps_d[nwalkers,nlayers],
 * density_d[nwalkers,nlayers,nmol] -> ec_d[nwalkers,nlayers,nwave].  The table is read once per
 * chunk of walkers.  work_d: pb_interp_ec_batch_work_doubles(...) doubles of device scratch (-1
 * for a negative argument).  nmol <= 8. */
int64_t pb_interp_ec_batch_work_doubles(int nlayers, int nwalkers);
/* What a call of that shape would launch, with the PB_INTERP_* variables as they are now:
 * out[6] (host) = walkers per chunk, two samples per thread (0/1), pair slots per thread, species
 * held in registers (4 or 8), unpredicated species loop (0/1), grid.x.  aligned16: ec_d and
 * etable_d both on 16 bytes; kcont: 0 no continuum, 1 continuum, 2 with H-; kalk: alkali lines.
 * No device is touched: for tests of the launch decision, not a tuning interface. */
int pb_interp_ec_batch_plan(int32_t *out, int nmol, int nlayers, int nwave, int nwalkers,
                            int aligned16, int kcont, int kalk);
int pb_interp_ec_batch(double *ec_d, const double *etable_d, const double *ttable_d,
                       const double *temps_d, const double *density_d, void *work_d, int nmol,
                       int ntemp, int nlayers, int nwave, int nwalkers, void *stream);
/* optic_depth.py:103-112 + radiative_transfer.py:57-71 (no cloud deck) for a batch:
 * ec_d[nwalkers,nlayers,nwave], raypath_d[nwalkers, n(n-1)/2], radius_d[nwalkers,nlayers] ->
 * spectrum_d[nwalkers,nwave]; depth_d[nwalkers,nlayers,nwave] and ideep_d[nwalkers,nwave] are
 * optional (NULL: not stored).  work_d: pb_transit_work_doubles(...) doubles of device scratch
 * (the ray paths re-laid for scalar loads), or NULL (ray paths staged in LDS: slower). */
int64_t pb_transit_work_doubles(int nlayers, int itop, int ibottom, int nwave, int nwalkers);
int pb_transit_spectrum_batch(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                              const double *ec_d, const double *raypath_d,
                              const double *radius_d, double rstar, int itop, int ibottom,
                              double maxdepth, int nlayers, int nwave, int nwalkers,
                              void *work_d, void *stream);
/* The same batch with its columns in an order of the caller's choosing (retrieval batches:
 * columns sorted by the row at which a typical model crosses maxdepth).  ec_d[nwalkers,nlayers,
 * nwave] holds the columns IN THAT ORDER; column_d[nwave] gives the grid index of each, and
 * spectrum_d[nwalkers,nwave] is written in grid order.  The optical depths are formed row tile by
 * row tile and a wavefront stops at the tile in which its 32 columns have all crossed maxdepth --
 * the reference's per-column exit (_trapezoid.c:259-273) at tile granularity: neither the
 * remaining products nor the deeper layers of ec are touched.  Per column the arithmetic does not
 * depend on the order: spectra equal those of pb_transit_spectrum_batch bit for bit.  2 ... 128
 * impact parameters, nwave >= 2, no cloud deck; work_d as above (required). */
int pb_transit_spectrum_ordered(double *spectrum_d, const double *ec_d, const double *raypath_d,
                                const double *radius_d, const int32_t *column_d, double rstar,
                                int itop, int ibottom, double maxdepth, int nlayers, int nwave,
                                int nwalkers, void *work_d, void *stream);
/* The same two passes without the layers nobody reads.  With the columns in the depth order of a
 * base model, tile_limit_d[ceil(nwave / 256)] names for every block of 256 (ordered) columns the
 * last ROW TILE (16 impact parameters; tile m = layers itop + 16 m ... itop + 16 m + 15) any of
 * its columns is expected to need (the base model's deepest first crossing of maxdepth in the
 * block, _trapezoid.c:259-273, plus a margin):
 *   pb_interp_ec_batch_limited writes ec only for the layers row0 ... row0 + 16 (tile + 1) - 1 of
 *     a block (row0 = itop; the other elements of ec_d are left as they are);
 *   pb_transit_spectrum_limited stops a wavefront whose columns are still open beyond their
 *     block's tile, leaves their spectrum samples unwritten and sets flags_d[walker] = 1 and
 *     flags_d[nwalkers] = 1 (int32[nwalkers + 1], zeroed by the caller).
 * Repair without a host round trip: the same two calls again with tile_limit_d = NULL and
 *   gate_d = flags_d + nwalkers (interpolation: every workgroup returns at once unless *gate_d != 0;
 *     the per-walker weights in work_d are those of the first call) resp.
 *   gate_d = flags_d (transit: walker w is computed only if gate_d[w] != 0; the Q blocks in work_d
 *     are those of the first call).
 * The spectra are then bit-identical to pb_interp_ec_batch + pb_transit_spectrum_ordered whatever
 * the limits were (tests/test_gpu_batch.py::test_tile_limited_batch). */
int pb_interp_ec_batch_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                               const double *temps_d, const double *density_d, void *work_d,
                               int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                               const int32_t *tile_limit_d, int row0, const int32_t *gate_d,
                               void *stream);
int pb_transit_spectrum_limited(double *spectrum_d, const double *ec_d, const double *raypath_d,
                                const double *radius_d, const int32_t *column_d, double rstar,
                                int itop, int ibottom, double maxdepth, int nlayers, int nwave,
                                int nwalkers, void *work_d, const int32_t *tile_limit_d,
                                int32_t *flags_d, const int32_t *gate_d, void *stream);
/* The emission counterpart (pb_emission_flux_ordered with the same limits: a column stops at the
 * first layer whose plane-parallel depth reaches maxdepth, _trapezoid.c:199-209; one still open at
 * layer itop + 16 (tile + 1) of its block is left unwritten and its walker flagged; gate_d as for
 * the transit call). */
int pb_emission_flux_limited(double *flux_d, const double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temp_d, const double *mu_d,
                             const double *weights_d, const int32_t *column_d, int nmu,
                             double maxdepth, int itop, int ibottom, int nlayers, int nwave,
                             int nwalkers, const int32_t *tile_limit_d, int32_t *flags_d,
                             const int32_t *gate_d, void *stream);
/* Emission geometry for a batch: plane_parallel_optical_depth (src_c/_trapezoid.c:175-213) +
 * blackbody + intensity + quadrature sum (pyrat/spectrum.py:366-377) in one pass, no cloud deck:
 * ec_d[nwalkers,nlayers,nwave], intervals_d[nwalkers,nlayers-1], temp_d[nwalkers,nlayers] ->
 * flux_d[nwalkers,nwave]. */
int pb_emission_flux_batch(double *flux_d, const double *ec_d, const double *intervals_d,
                           const double *wn_d, const double *temp_d, const double *mu_d,
                           const double *weights_d, int nmu, double maxdepth, int itop,
                           int ibottom, int nlayers, int nwave, int nwalkers, void *stream);
/* The same batch with its columns in an order of the caller's choosing (columns that become
 * optically thick at similar layers side by side: a wavefront walks the layers until its LAST lane
 * has reached maxdepth, _trapezoid.c:190-200).  ec_d and wn_d hold the columns in that order,
 * column_d[nwave] the grid index of each; flux_d[nwalkers,nwave] is written in grid order.  Per
 * column the arithmetic does not depend on the order: same bits as pb_emission_flux_batch. */
int pb_emission_flux_ordered(double *flux_d, const double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temp_d, const double *mu_d,
                             const double *weights_d, const int32_t *column_d, int nmu,
                             double maxdepth, int itop, int ibottom, int nlayers, int nwave,
                             int nwalkers, void *stream);
/* PassBand.integrate for a batch of full-grid spectra: bandflux_d[nwalkers,nbands]
 * (x heights_d[b] when given). */
int pb_band_integrate_batch(double *bandflux_d, const double *spectrum_d, const double *wn_d,
                            const int32_t *band_start_d, const int32_t *band_count_d,
                            const double *response_d, const int64_t *response_offset_d,
                            const double *heights_d, int nbands, int nwave, int nwalkers,
                            void *stream);
/* What the reference makes of a plane-parallel flux after the radiative transfer
 * (pyrat/spectrum.py:394-405; eval()'s f_lambda conversion, pyrat_obj.py:323-329), per sample:
 *   fplanet = flux_d [* f_dilution when dilute != 0]
 *   mode 0 emission: spectrum = fplanet
 *   mode 1 eclipse : spectrum = fplanet * (1/starflux_d * scale), scale = (rplanet/rstar)^2
 *   mode 2 f_lambda: spectrum = 10 * fplanet * (scale * wn_d * 1e-4)^2, scale = rplanet/distance
 * -- the NumPy expressions' products in their order (bit-equal).  fplanet_d may be NULL; spectrum_d
 * and fplanet_d may alias flux_d. */
int pb_emission_observables(double *spectrum_d, double *fplanet_d, const double *flux_d,
                            const double *starflux_d, const double *wn_d, int64_t nwave, int mode,
                            int dilute, double f_dilution, double scale, void *stream);
/* bandflux_d[w,b] *= walker_scale_d[w] (f_dilution of walker w, pyrat_obj.py:296-297) and
 * *= band_scale_d[b] (eclipse: rprs^2 / bandflux_star, pyrat_obj.py:662-665), in that order;
 * either pointer may be NULL. */
int pb_band_scale(double *bandflux_d, const double *band_scale_d, const double *walker_scale_d,
                  int nbands, int nwalkers, void *stream);
/* eval()'s reject path (pyrat_obj.py:302-320, 378-380): walkers with a temperature outside
 * [tmin, tmax] get bandflux = +inf. */
int pb_reject_walkers(double *bandflux_d, const double *temps_d, double tmin, double tmax,
                      int nlayers, int nbands, int nwalkers, void *stream);

/* ---- The exit towards the sampler (pb_observation.hip).
 * The eclipse factor of a batch whose walkers have a stellar temperature of their own (eval()'s
 * tstar branch, pyrat_obj.py:288-294, then Pyrat.band_integrate, pyrat_obj.py:662-665):
 *   bandflux_d[w,b] *= f_dilution_d[w] (when given), then *= rprs2_w / bandflux_star[w,b]
 * bandflux_star[w,b] = the band integral (x heights_d[b] when given, like PassBand.integrate) of
 * star_grid_d[nt,nwave], the SED grid on the model's wavenumbers, interpolated at tstar_d[w]
 * along sed_temps_d[nt] (strictly ascending, nt >= 2) by interp1d's linear rule:
 *   i = searchsorted_left(sed_temps, tstar) clipped to [1, nt-1], lo = i-1,
 *   s = ((y_hi - y_lo) / (x_hi - x_lo)) * (tstar - x_lo) + y_lo   (every operation rounded)
 * and summed in the order of pb_band_integrate_batch; the interpolated spectra are never stored.
 * rprs2_w = rprs2 when rplanet_d is NULL, else t * t with t = rplanet_d[w] / rstar.
 * The bands are the arrays of pb_band_integrate_batch.
 * DEVIATION: a walker whose tstar is NaN or outside [sed_temps[0], sed_temps[nt-1]] gets +inf in
 * every band (the reference's interp1d raises there): rejected like a walker outside the table's
 * temperatures.  nwalkers == 0 or nbands == 0: PB_OK, nothing launched. */
int pb_star_band_scale_batch(double *bandflux_d, const double *star_grid_d,
                             const double *sed_temps_d, const double *tstar_d, double rprs2,
                             const double *rplanet_d, double rstar, const double *f_dilution_d,
                             const double *wn_d, const int32_t *band_start_d,
                             const int32_t *band_count_d, const double *response_d,
                             const int64_t *response_offset_d, const double *heights_d, int nt,
                             int nbands, int nwave, int nwalkers, void *stream);
/* pb_loglike with the data and the uncertainties of each walker (Data.offset_data /
 * Data.scale_errors, tools/data.py:210-270): per band b of walker w
 *   d = data_d[b] + offset_vals_d[w,g] * offset_unit      g = offset_group_d[b] (-1: none)
 *   e = pow(10, err_vals_d[w,g])                          g = err_group_d[b]    (-1: none)
 *   err_mode_d[g] == 0 (scale):      u = uncert_d[b] * e
 *   err_mode_d[g] == 1 (quadrature): e *= err_unit; u = sqrt(uncert_d[b]^2 + e^2)
 * and pb_loglike's sums of d, u and bandflux_d[w,b] in its order; not finite: -1e98.
 * offset_vals_d[nwalkers,noff], err_vals_d[nwalkers,nerr]; with noff == nerr == 0 (their pointers
 * may then be NULL) the result has the bits of pb_loglike. */
int pb_loglike_obs(double *loglike_d, const double *bandflux_d, const double *data_d,
                   const double *uncert_d, const int32_t *offset_group_d,
                   const double *offset_vals_d, double offset_unit, int noff,
                   const int32_t *err_group_d, const int32_t *err_mode_d,
                   const double *err_vals_d, double err_unit, int nerr, int nwalkers, int nbands,
                   void *stream);

/* ---- The front end towards the sampler (pb_retrieval.hip): theta_d[nwalkers,nfree], the free
 * parameters a sampler holds, -> every per-walker tensor of the batched loop, the log-prior and the
 * bounds flag, in one launch.  The map is nmap entries (device arrays, built once per retrieval);
 * entry e writes ONE element of one destination:
 *   v = src_d[e] >= 0 ? theta[w, src_d[e]] : const_d[e];   if (factor_d[e] != 1) v = v * factor_d[e]
 *   dest_ptrs[dest_d[e]][w * dest_ncols[dest_d[e]] + col_d[e]] = v
 * (a fixed parameter is a constant; a shared one has the src of the parameter it follows: Loglike's
 * rule, tools/retrieval_tools.py:91-93; values are copies and at most one multiply).  dest_ptrs /
 * dest_ncols: HOST arrays of ndest device pointers [nwalkers,ncols] and their column counts,
 * passed to the kernel by value.  Per free parameter f: pmin_d, pmax_d, prior_d, priorlow_d,
 * priorup_d and value_d [nfree].  The bounds test comes first:
 *   inside_d[w] = every theta[w,f] is finite and pmin[f] <= theta[w,f] <= pmax[f]
 * and a walker that fails it is mapped from value_d instead of its own row (DEVIATION: so that no
 * later kernel sees NaN or out-of-range input); its log_prior_d[w] is -inf.  Otherwise
 *   log_prior_d[w] = sum_f (priorlow[f] == 0 && priorup[f] == 0 ? 0
 *                           : -0.5 ((p - prior[f]) / s)^2,  s = p < prior[f] ? priorlow[f] : priorup[f])
 * without a normalisation term, summed in a fixed order (two terms per lane, then a butterfly):
 * the same bits in every run.  One wavefront per walker.  An entry whose dest, col or src is out
 * of range writes nothing.  More than PB_RETRIEVAL_MAX_PARAMS entries or free parameters, or
 * more than PB_RETRIEVAL_MAX_DESTS destinations: PB_ERR_ARG.  nwalkers == 0: nothing launched. */
#define PB_RETRIEVAL_MAX_PARAMS 128
#define PB_RETRIEVAL_MAX_DESTS 16
int pb_retrieval_map(double *const *dest_ptrs, const int32_t *dest_ncols, int ndest,
                     double *log_prior_d, int32_t *inside_d, const double *theta_d,
                     const int32_t *src_d, const double *const_d, const double *factor_d,
                     const int32_t *dest_d, const int32_t *col_d, const double *value_d,
                     const double *pmin_d, const double *pmax_d, const double *prior_d,
                     const double *priorlow_d, const double *priorup_d, int nmap, int nfree,
                     int nwalkers, void *stream);
/* The prior transform of a nested sampler: cube_d[nwalkers,nfree] in (0, 1) -> theta_d, per free
 * parameter: uniform (priorlow == priorup == 0): pmin + u (pmax - pmin); two-sided Gaussian, with
 * lo = priorlow and up = priorup:
 *   u <  lo / (lo + up):  prior + lo * ndtri(0.5 u (lo + up) / lo)
 *   otherwise:            prior + up * ndtri(1 - 0.5 (1 - u) (1 + lo / up))
 * with the device library's inverse normal CDF; not truncated to [pmin, pmax]. */
int pb_prior_transform(double *theta_d, const double *cube_d, const double *pmin_d,
                       const double *pmax_d, const double *prior_d, const double *priorlow_d,
                       const double *priorup_d, int nfree, int nwalkers, void *stream);
/* out_d[w] = inside_d[w] ? (add_prior ? loglike_d[w] + log_prior_d[w] : loglike_d[w])
 *                        : outside_value     (log_prior_d may be NULL when add_prior == 0). */
int pb_log_posterior(double *out_d, const double *loglike_d, const double *log_prior_d,
                     const int32_t *inside_d, double outside_value, int add_prior, int nwalkers,
                     void *stream);

/* ---- The sampler (pb_sampler.hip): DEMC-zs (ter Braak & Vrugt 2008, Stat. Comput. 18, 435).  A
 * generation is pb_demc_propose -> the caller's log-posterior of prop_d -> pb_demc_accept, with
 * nothing read back; pyratbay_amd/sampler.py states every kernel in NumPy (the specification).
 * Random numbers: Philox4x32-10 (pb_philox.h), key = seed (low word, high word), counter =
 * (block, chain w, generation g, tag), tags 0 propose, 1 accept, 2 initial draw; a block's words
 * (0, 1) and (2, 3) give two uniforms u = (n + 0.5) 2^-52, n = ((x_a >> 6) << 26) + (x_b >> 6), in
 * [2^-53, 1 - 2^-53], and two normals sqrt(-2 ln u_a) cos(2 pi u_b), ... sin(2 pi u_b); an index
 * into n rows is idx(u, n) = min(floor(u n), n - 1).  One wavefront per chain, two parameters per
 * lane, nfree <= PB_RETRIEVAL_MAX_PARAMS; sums in a fixed order (the lane's two terms, then a
 * butterfly).  0 <= g < 2^32, else PB_ERR_ARG.  nwalkers == 0: nothing launched.
 *
 * pb_demc_propose: theta_d[nwalkers,nfree], the history z_d[., nfree] whose first M >= 3 rows exist
 * (fewer: PB_ERR_ARG), pstep_d[nfree] -> prop_d[nwalkers,nfree], log_jac_d[nwalkers],
 * kind_d[nwalkers] (0 parallel, 1 snooker).  Block 0: r1 = idx(u, M), r2 = idx(u', M - 1),
 * r2 += (r2 >= r1); block 1: u_s, rz = idx(u', M); block 2: u_g; block 3 + f / 2: the normals n_f
 * (even f the cosine, odd f the sine).
 *   u_s >= p_snooker:  prop = (theta + gamma (Z[r1] - Z[r2])) + (fepsilon pstep) n,
 *                      gamma = fgamma 2.38 / sqrt(2 nfree); log_jac = 0
 *   otherwise:         d = theta - Z[rz], D2 = d.d,
 *                      prop = theta + ((1.2 + u_g) ((Z[r1] - Z[r2]).d / D2)) d,
 *                      log_jac = 0.5 (nfree - 1) (ln |prop - Z[rz]|^2 - ln D2);
 *                      D2 not > 0 or log_jac not finite: prop = theta, log_jac = 0. */
int pb_demc_propose(double *prop_d, double *log_jac_d, int32_t *kind_d, const double *theta_d,
                    const double *z_d, const double *pstep_d, int64_t g, uint64_t seed, int64_t M,
                    double fgamma, double fepsilon, double p_snooker, int nfree, int nwalkers,
                    void *stream);
/* The rest of a generation.  With u the first uniform of block 0, tag 1, chain w accepts iff
 *   ln u < (logp_prop_d[w] - logp_d[w]) + log_jac_d[w]
 * (a NaN on either side rejects; so does a proposal at -inf).  On accept theta_d[w] and logp_d[w]
 * are overwritten in place and row nrows_d[w] of the chain store is opened: rows_d[w,.,nfree],
 * row_logp_d[w,.], row_gen_d[w,.] = g, counts_d[w,.] = 1 (cap rows per chain), nrows_d[w] += 1; on
 * reject counts_d[w, nrows_d[w] - 1] += 1.  An accept at nrows_d[w] == cap sets overflow_d[w]
 * instead; from then on (and while nrows_d[w] is outside 1 .. cap) the chain records nothing but
 * goes on sampling.  Per chain and parameter Welford's running mean and M2 of the state after the
 * decision: nstat_d[w] += 1, delta = x - mean, mean += delta / nstat, M2 += delta (x - mean).
 * append != 0: the state after the decision is written to z_d[M + w] (M + nwalkers <= Mcap, else
 * PB_ERR_ARG; g must also fit row_gen_d).  accepted_d[w] = 1 or 0. */
int pb_demc_accept(double *theta_d, double *logp_d, const double *prop_d,
                   const double *logp_prop_d, const double *log_jac_d, double *rows_d,
                   double *row_logp_d, int32_t *row_gen_d, int64_t *counts_d, int32_t *nrows_d,
                   int32_t *overflow_d, double *mean_d, double *m2_d, int64_t *nstat_d,
                   double *z_d, int32_t *accepted_d, int64_t g, uint64_t seed, int64_t M,
                   int64_t Mcap, int append, int cap, int nfree, int nwalkers, void *stream);
/* rhat_d[nfree] of nwalkers chains of n states each from their Welford sums: W = the mean over
 * chains of M2 / (n - 1), B / n = the ddof = 1 variance of the chain means,
 * R = sqrt(((n - 1) / n W + B / n) / W); NaN where W == 0, n < 2 or nwalkers < 2. */
int pb_gelman_rubin(double *rhat_d, const double *mean_d, const double *m2_d, int64_t n,
                    int nfree, int nwalkers, void *stream);
/* out_d[n,ncol]: the uniforms of tag 2 -- row = chain slot, g = 0, block col / 2, even columns
 * from words (0, 1), odd ones from words (2, 3).  For the initial draw. */
int pb_philox_uniform(double *out_d, uint64_t seed, int64_t n, int ncol, void *stream);

/* ---- Nested sampling (pb_nested.hip; Skilling 2006, Bayesian Anal. 1, 833): the evidence ln Z and
 * the weighted dead points, in the unit cube, on nlive <= PB_NESTED_MAX_LIVE live points
 * live_u_d[nlive,nfree], live_logl_d[nlive].  An iteration `it` (from 1) is pb_nested_select ->
 * nsteps x (pb_nested_propose -> the caller's prior transform and log-likelihood of point_d ->
 * pb_nested_accept), with nothing read back; pyratbay_amd/nested.py states every kernel in NumPy
 * (the specification).  Random numbers, idx(u, n) and the conventions are the sampler's above,
 * with the tags 3 (start), 4 (walk step), 5 (resample); the walk's kernels run one wavefront per
 * slot, two parameters per lane, nfree <= PB_RETRIEVAL_MAX_PARAMS.  state_d[4]: ln X (starts at
 * 0), ln Z (starts at -inf), Lstar, remain.  Refused with PB_ERR_ARG and a message: a null pointer,
 * a batch K outside 1 .. nlive - 2, nlive > PB_NESTED_MAX_LIVE, nfree too large, `it` or `q`
 * outside 0 .. 2^32 - 1.
 *
 * pb_nested_select: the live points ranked by logl ascending -- ties to the lower index, NaN the
 * lowest -- by counting over the values held in LDS (one thread per point; the result depends on
 * the values alone).  The K lowest die in rank order: dead_idx_d[K]; the others are
 * surv_idx_d[nlive - K] in rank order.  Dead point j, n = nlive - j, one after the other:
 *   ln w = (logl + ln X) + ln(-expm1(-1 / n))   (-inf for a NaN logl)
 *   ln X = ln X - 1 / n;   ln Z = logaddexp(ln Z, ln w)         (NumPy's logaddexp)
 * Its cube row, logl and ln w go to row dead_base + j of dead_u_d[dead_cap,nfree], dead_logl_d,
 * dead_logw_d (dead_base + K > dead_cap: PB_ERR_ARG).  Lstar = logl of the last dead point;
 * remain = logaddexp(ln Z, Ltop + ln X) - ln Z with Ltop the logl of the last survivor. */
#define PB_NESTED_MAX_LIVE 4096
int pb_nested_select(int32_t *dead_idx_d, int32_t *surv_idx_d, double *dead_u_d,
                     double *dead_logl_d, double *dead_logw_d, double *state_d,
                     const double *live_u_d, const double *live_logl_d, int64_t dead_base,
                     int64_t dead_cap, int K, int nlive, int nfree, void *stream);
/* One walk step of the K slots, nsurv = nlive - K.  start != 0 (the first step of an iteration):
 * slot k first takes cur_d[k] = live_u[pick], cur_logl_d[k] = live_logl[pick], pick =
 * surv_idx[idx(u, nsurv)], u the first uniform of block 0 at (0, k, it, tag 3), and acc_it_d[k] = 0.
 * Then, at (block, k, q, tag 4): block 0: a = idx(u, nsurv), b = idx(u', nsurv - 1), b += (b >= a);
 * block 1: gamma = u_m < p_unit ? 1 : fgamma 2.38 / sqrt(2 nfree);
 *   prop = cur + gamma (U[surv a] - U[surv b])     (product and sum rounded separately)
 *   inside_d[k] = every 0 < prop_f < 1;   point_d[k] = inside ? prop : cur
 * a_d, b_d, gamma_d [K]: the draw.  An entry of surv_idx_d outside the live set is clamped into
 * it.  K == 0: nothing launched. */
int pb_nested_propose(double *point_d, int32_t *inside_d, int32_t *a_d, int32_t *b_d,
                      double *gamma_d, double *cur_d, double *cur_logl_d, int32_t *acc_it_d,
                      const double *live_u_d, const double *live_logl_d,
                      const int32_t *surv_idx_d, int64_t it, int64_t q, uint64_t seed,
                      double fgamma, double p_unit, int start, int nlive, int nfree, int K,
                      void *stream);
/* The rest of a walk step.  Slot k accepts iff inside_d[k] != 0 and logl_prop_d[k] > Lstar
 * (state_d[2]; strict, and a NaN on either side rejects): cur_d[k], cur_logl_d[k] overwritten in
 * place, naccept_d[k] (int64) and acc_it_d[k] raised; accepted_d[k] = 1 or 0.  last != 0 (the last
 * step of an iteration): live_u[dead_idx_d[k]] = cur[k], live_logl[dead_idx_d[k]] = cur_logl[k]
 * (an index outside the live set writes nothing), and stuck_d[k] += 1 where acc_it_d[k] == 0: the
 * replacement duplicates a survivor.  K == 0: nothing launched. */
int pb_nested_accept(double *cur_d, double *cur_logl_d, const double *point_d,
                     const double *logl_prop_d, const int32_t *inside_d, const double *state_d,
                     int64_t *naccept_d, int32_t *acc_it_d, int64_t *stuck_d, int32_t *accepted_d,
                     double *live_u_d, double *live_logl_d, const int32_t *dead_idx_d, int last,
                     int nlive, int nfree, int K, void *stream);
/* The result so far; changes nothing of the run.  n = ndead + nlive rows: the dead points, then
 * the live ones at ln w = (logl + ln X) - ln(nlive) (-inf for a NaN logl) -> logl_d[n], logw_d[n].
 * m = max ln w, e = exp(ln w - m) (0 where ln w = -inf), S = sum e:
 *   out_d[0] = ln Z = m + ln S;   out_d[2] = H = (sum of e ln L over e > 0) / S - ln Z;
 *   out_d[1] = ln Z_err = sqrt(max(H, 0) / nlive);   cdf_d[i] = (e_0 + ... + e_i) / S
 * The sums run over 256 chunks of ceil(n / 256) consecutive rows: each chunk from 0 in index
 * order, the chunk sums in chunk order, the running sum of a chunk from the sum of the chunks
 * before it.  One block. */
int pb_nested_finish(double *out_d, double *logw_d, double *logl_d, double *cdf_d,
                     const double *dead_logl_d, const double *dead_logw_d,
                     const double *live_logl_d, const double *state_d, int64_t ndead, int nlive,
                     void *stream);
/* The equal-weight posterior as a histogram: counts_d[n] (int64, zeroed here, integer atomics) of
 * nsamples <= 2^32 draws; sample s takes uniform s % 2 of block 0 at (0, s / 2, 0, tag 5) and
 * falls on the first row i with cdf_d[i] > u (bisection; cdf_d must not decrease), clipped to
 * n - 1. */
int pb_nested_resample(int64_t *counts_d, const double *cdf_d, int64_t n, int64_t nsamples,
                       uint64_t seed, void *stream);

/* ---- The posterior modes of a finished nested-sampling run (pb_modes.hip): the run does not
 * cluster; its stored points are decomposed afterwards.  pyratbay_amd/modes.py states every kernel
 * in NumPy (the specification), and the kernels have the statements' bits.  All rows are rows of
 * the unit cube, finite by construction: there is no rule for NaN.  FP64 vector arithmetic, every
 * product and sum rounded separately, no atomics on doubles.  Refused with PB_ERR_ARG and a
 * message: a null pointer, nfree outside 1 .. PB_RETRIEVAL_MAX_PARAMS, more than
 * PB_NESTED_MAX_LIVE rows, knn outside 1 .. PB_MODES_MAX_KNN, max_modes < 1.
 *
 * pb_modes_sqdist: d2_d[na,nb] of a_d[na,nfree] and b_d[nb,nfree]: d2 = 0, then for p = 0 ..
 * nfree - 1 in order t = a[i,p] - b[j,p]; d2 = d2 + t * t.  A thread owns a point; tiles of 32
 * rows of b are staged in LDS in chunks of 16 parameters, visited in ascending order, with the 32
 * partial sums in registers.  Every kernel below takes its distances from the same sweep. */
#define PB_MODES_MAX_KNN 32
int pb_modes_sqdist(double *d2_d, const double *a_d, const double *b_d, int64_t na, int nb,
                    int nfree, void *stream);
/* Single linkage of r_d[n,nfree], 2 <= n <= PB_NESTED_MAX_LIVE, at the scale of the rows' own
 * spacing.  k = min(knn, n - 1); dk_d[n]: the k-th smallest squared distance from row i to another
 * row (a running list per row; duplicates count); ell2_d[0] = (link * link) * max dk.  Rows
 * i != j are linked iff d2 <= ell2: bits_d[n, ceil(n / 32)] (32-bit words; bit j % 32 of word
 * j / 32 of row i).  The components of the links come from one block with the labels in LDS:
 * minimum-label propagation with pointer jumping until a pass changes nothing, which leaves every
 * row the smallest row index of its component whatever the order of the updates.  In the canonical
 * order -- size descending, ties to the component with the smallest row -- the first max_modes
 * components of at least min_mode rows get the labels 0, 1, ... in labels_d[n]; every other row
 * gets -1; the largest component is mode 0 whatever its size.  nmodes_d[0] >= 1.  The rule is
 * conservative: a far outlier raises ell2 and merges modes, it never splits one.  dk_d and bits_d
 * are the caller's work space. */
int pb_modes_link(int32_t *labels_d, int32_t *nmodes_d, double *ell2_d, double *dk_d,
                  int32_t *bits_d, const double *r_d, int n, int nfree, int knn, double link,
                  int min_mode, int max_modes, void *stream);
/* mode_d[np]: every point of p_d[np,nfree] takes the label of the row of r_d[n,nfree] with the
 * smallest squared distance among the rows with labels_d >= 0, ties to the lower row (the minimum
 * over (d2, row): no tiling changes it); -1 where no row has a label. */
int pb_modes_assign(int32_t *mode_d, const double *p_d, const double *r_d,
                    const int32_t *labels_d, int64_t np, int n, int nfree, void *stream);
/* rows_d[cap] (int64): the indices i < n with counts_d[i] > 0, ascending, the first cap of them;
 * nrows_d[0] (int64): how many there are.  One block. */
int pb_modes_rows(int64_t *rows_d, int64_t *nrows_d, const int64_t *counts_d, int64_t n,
                  int64_t cap, void *stream);
/* pb_nested_finish's formulae per mode c < nmodes, one block each: m = the largest ln w with
 * mode_d[i] == c, e = exp(ln w - m) there where ln w > -inf and 0 elsewhere, S = sum e,
 *   ln_z_m_d[c] = m + ln S;   info_m_d[c] = (sum of e ln L over e > 0) / S - ln Z_m;
 *   fraction_m_d[c] = exp(ln Z_m - ln_z_d[0])
 * with the sums over all n rows in pb_nested_finish's 256 chunks and order.  A mode without
 * weight: -inf, NaN, 0. */
int pb_modes_evidence(double *ln_z_m_d, double *info_m_d, double *fraction_m_d,
                      const double *logw_d, const double *logl_d, const int32_t *mode_d,
                      const double *ln_z_d, int64_t n, int nmodes, void *stream);

/* ---- Batched multi-start Levenberg-Marquardt (pb_optimize.hip): the maximum of the posterior and
 * its Laplace covariance for nstarts starts at once, theta_d[nstarts,nfree], on residual vectors of
 * m columns.  An iteration is pb_lm_probe -> the caller's residuals of probe_d -> pb_lm_normal ->
 * pb_lm_step -> the caller's residuals of trial_d -> pb_lm_update, with nothing read back;
 * pyratbay_amd/optimize.py states every kernel in NumPy (the specification).  Products and sums
 * round separately; no atomics on doubles; every sum has one fixed order (below).  Refused with
 * PB_ERR_ARG and a message: a null pointer, nfree outside 1 .. PB_RETRIEVAL_MAX_PARAMS, m < 1,
 * ntrial outside 1 .. PB_LM_MAX_TRIALS, nu <= 1.  nstarts == 0: nothing launched.
 *
 * pb_lm_residuals: residuals_d[nw, ndata + ngauss] of a walker batch.  Column i < ndata is
 * (data_i + offset - bandflux[w,i]) / uncert_i with the walker's offsets and uncertainty scaling
 * exactly as pb_loglike_obs applies them; column ndata + j is (theta[w,k] - prior_k) / s_k,
 * k = gauss_index_d[j] (an index outside 0 .. nfree - 1 gives +inf), s_k = priorlow_k for
 * theta < prior_k, else priorup_k (prior_d, priorlow_d, priorup_d: [nfree]).  A walker with
 * inside_d[w] == 0 or a non-finite band flux gets a row of +inf. */
int pb_lm_residuals(double *residuals_d, const double *bandflux_d, const double *data_d,
                    const double *uncert_d, const int32_t *offset_group_d,
                    const double *offset_vals_d, double offset_unit, int noff,
                    const int32_t *err_group_d, const int32_t *err_mode_d,
                    const double *err_vals_d, double err_unit, int nerr, const double *theta_d,
                    const int32_t *inside_d, const int32_t *gauss_index_d, const double *prior_d,
                    const double *priorlow_d, const double *priorup_d, int ngauss, int nfree,
                    int nwalkers, int ndata, void *stream);
/* probe_d[nstarts, nfree + 1, nfree]: row 0 = theta, row k + 1 = theta + hs_k e_k with
 * hs_k = h_k = fd_step scale_k, or -h_k where theta_k + h_k > pmax_k; step_d[nstarts, nfree] = hs. */
int pb_lm_probe(double *probe_d, double *step_d, const double *theta_d, const double *pmax_d,
                const double *scale_d, double fd_step, int nfree, int64_t nstarts, void *stream);
/* The normal equations of every start from R_d[nstarts, nfree + 1, m], the residuals of probe_d:
 * D_ik = R[s,k+1,i] - R[s,0,i]; S_kl = sum_i D_ik D_il, summed in index order by one thread;
 *   A_d[s,k,l] = (S_kl / hs_min(k,l)) / hs_max(k,l)   (full, symmetric in bits)
 *   g_d[s,k] = (sum_i D_ik R[s,0,i]) / hs_k           (index order)
 *   cost_d[s] = 0.5 sum_i R[s,0,i]^2                  (64 lane-strided partial sums -- lane j takes
 *               i = j, j + 64, ... -- then the xor butterfly 32, 16, .., 1)
 * A column k with a non-finite D_ik is frozen: row and column k of A and g_k are 0.  Block =
 * (start, 32 x 32 tile of the upper triangle), the m loop inside, PB_LM_CHUNK points of the tile's
 * columns staged through LDS per step. */
#define PB_LM_CHUNK 64
#define PB_LM_MAX_TRIALS 16
int pb_lm_normal(double *A_d, double *g_d, double *cost_d, const double *R_d, const double *step_d,
                 int nfree, int m, int64_t nstarts, void *stream);
/* doubles of work_d for pb_lm_step with ntrial trials and for pb_lm_covariance:
 * nstarts nfree^2 max(ntrial, 2) (the Cholesky factors live there, one per block: a 128 x 128
 * factor does not fit the 64 KiB of LDS a block gets). */
int64_t pb_lm_work_doubles(int nfree, int ntrial, int64_t nstarts);
/* The trial points trial_d[nstarts, ntrial, nfree].  Active set: k is active if theta_k <= pmin_k
 * and g_k > 0, or theta_k >= pmax_k and g_k < 0, or A_kk == 0.  On the others (f), for
 * lam_j = lam_d[s] nu^(j-1), j = 0 .. ntrial - 1 (lam / nu, then times nu per trial):
 *   (A_ff + lam_j diag(A_ff)) delta = -g_f   by Cholesky (right-looking; column-oriented solves)
 *   trial = min(max(theta + delta, pmin), pmax), active parameters unchanged.
 * A pivot that is <= 0 or not finite, or a non-finite delta: trial = theta.
 * pgrad_d[s] = max over f of |g_k| scale_k (0 without a free parameter). */
int pb_lm_step(double *trial_d, double *pgrad_d, double *work_d, const double *A_d,
               const double *g_d, const double *theta_d, const double *lam_d,
               const double *pmin_d, const double *pmax_d, const double *scale_d, double nu,
               int ntrial, int nfree, int64_t nstarts, void *stream);
/* The decision of every start with status_d[s] == 0 (running) from Rt_d[nstarts, ntrial, m], the
 * residuals of trial_d; a finished start is left untouched.  Status: 1 GTOL, 2 FTOL, 3 XTOL,
 * 4 STALL, 5 MAXIT.  A non-finite cost_d[s]: STALL; else pgrad_d[s] <= gtol: GTOL (both without a
 * step: picked_d[s] = -1, niter_d unchanged).  Otherwise the trial costs 0.5 |Rt|^2 in cost_d's
 * order; the lowest finite one wins, ties to the lowest index.  Below cost_d[s]: accepted --
 * theta_d[s] = that trial, cost_d[s] = its cost, lam = max(lam_j / nu, lam_min), picked_d[s] = j;
 * FTOL if the decrease <= ftol max(cost, 1), else XTOL if max_k |dtheta_k| / scale_k <= xtol.
 * Otherwise lam = lam nu^ntrial and picked_d[s] = -1.  Then niter_d[s] += 1; still running and
 * lam > lam_max: STALL; still running and niter_d[s] >= max_iter: MAXIT.
 * unfinished_d[0] = the number of starts still running (int32, always written). */
int pb_lm_update(double *theta_d, double *cost_d, double *lam_d, int32_t *status_d,
                 int32_t *niter_d, int32_t *picked_d, int32_t *unfinished_d,
                 const double *trial_d, const double *Rt_d, const double *pgrad_d,
                 const double *scale_d, double nu, double lam_min, double lam_max, double gtol,
                 double ftol, double xtol, int max_iter, int ntrial, int nfree, int m,
                 int64_t nstarts, void *stream);
/* The Laplace covariance cov_d[nstarts, nfree, nfree] = (A_ff)^-1 on the parameters that are not
 * active (pb_lm_step's rule; active_d[nstarts, nfree] = 1 / 0), 0 in the active rows and columns.
 * Cholesky, one solve per column, the upper triangle mirrored: symmetric in bits.  Numerically
 * singular -- a pivot that is not finite or not above nf eps A_pp, nf the free parameters, A_pp
 * the diagonal before the factorisation --: NaN in the free block and singular_d[s] = 1 (else 0).
 * work_d: pb_lm_work_doubles. */
int pb_lm_covariance(double *cov_d, int32_t *active_d, int32_t *singular_d, double *work_d,
                     const double *A_d, const double *g_d, const double *theta_d,
                     const double *pmin_d, const double *pmax_d, int nfree, int64_t nstarts,
                     void *stream);

/* High-resolution data (eval()'s second exit, pyrat/pyrat_obj.py:331-356).
 * ps.inst_convolution's last step (spectrum/spec_tools.py:879) for a batch:
 *   out_d[w] = convolve(spectra_d[w] * sample_scale_d, taps_d, mode='same')
 * -- the full convolution cut to the grid, zeros beyond both ends; ntaps odd, at most 1025 (a
 * larger kernel is refused: PB_ERR_ARG, the message names the limit).  sample_scale_d[nwave]
 * (or NULL) multiplies every sample as it is loaded: the eclipse ratio and the f_lambda factor are
 * applied before the convolution in the reference.  Not in place. */
int pb_inst_convolve_batch(double *out_d, const double *spectra_d, const double *taps_d,
                           const double *sample_scale_d, int ntaps, int nwave, int nwalkers,
                           void *stream);
/* Convolution, radial-velocity shift and sampling at the data in one launch, the convolved
 * spectra never stored: per walker w
 *   s = spectra_d[w] [* walker_scale_d[w]] [* sample_scale_d]
 *   c = convolve(s, taps_d, mode='same')                       (only where a data point needs it)
 *   x = wn_d * sqrt((1 - v/c) / (1 + v/c)), v = rv_kms_d[w] km/s  (spec_tools.py:883-907; NULL: 0)
 *   out_d[w, data_slot_d[j]] = interp1d(x, c)(data_wn_sorted_d[j]):  idx = searchsorted(x, d,
 *     'left') clipped to [1, nwave - 1], lo = idx - 1, (c[idx] - c[lo]) / (x[idx] - x[lo]) * (d -
 *     x[lo]) + c[lo]
 * data_wn_sorted_d[ndata] ascending, data_slot_d[ndata] a permutation of 0 .. ndata - 1 (the
 * caller's order).  A walker with |rv| > rv_max (or NaN), or with a data point off its shifted
 * grid (interp1d raises there), gets +inf in every output.  Same limit on ntaps. */
int pb_hires_observe_batch(double *out_d, const double *spectra_d, const double *wn_d,
                           const double *taps_d, const double *sample_scale_d,
                           const double *data_wn_sorted_d, const int32_t *data_slot_d,
                           const double *rv_kms_d, const double *walker_scale_d, double rv_max,
                           int ntaps, int nwave, int ndata, int nwalkers, void *stream);

/* The retrieval batch with continuum terms (pyrat/opacity.py:206-257: every model adds to the
 * one ec), added in registers before pb_interp_ec_batch[_limited] store a sample -- no second
 * pass over ec.  Per walker and layer the terms of Continuum.add / pb_continuum, in its order, on
 * top of the interpolated value:
 *   rank-1 models in list order: kind 0 Rayleigh (Kurucz): rank1_cs_d[m][nwave] x the density of
 *     species rank1_species[m]; kind 1 Lecavelier: 10^p[par] s0 (wn l0)^-p[par+1] x p BAR/T/K
 *     (lecavelier.py:73-100); kind 2 CCSgray: 10^p[par] s0 where 10^p[par+1] <= p <= 10^p[par+2],
 *     else 0, x p BAR/T/K (gray.py:63-75) -- p = rank1_pressure_d[m][nlayers] (bar), p[] = the
 *     walker's row of pars_d;
 *   CIA tables in order (pb_continuum's bracket rule; a temperature off a table is clamped to its
 *     ends: finite, and the caller rejects the walker) x the product of the densities of its
 *     cia_nspec[c] species, only where bit c of cia_mask_d[w] is set;
 *   H- bound-free + free-free when hminus != 0 (n_H x n_e: species hm_species[0], [1]).
 * density_d[nwalkers][nlayers][ncs]; pars_d[.][npars] with pars_stride = npars (per walker) or 0
 * (one row for all).  Every per-sample operand (rank1_cs_d, cia_tab_d rows, cia_mask_d, wn_d,
 * hm_sigma_bf_d, hm_ff_d rows) is in the column order of etable_d / ec_d.  At most
 * PB_CONT_MAX_RANK1 rank-1 models, PB_CONT_MAX_CIA tables of at most PB_CONT_MAX_CIA species,
 * one H- model.
 *   Alkali resonance doublets (alkali.py:28-262, _alkali.c:58-104) after H-, nalkali models in
 *     order, the lines of a model in order: per sample inside |wn - wn0| <= cutoff the power-law
 *     wing voigt_det (|dwn|/dsigma)^-1.5 C3 gf/Z exp(-C2 (|dwn| - dsigma)/T) where |dwn| >=
 *     dsigma, else the Lorentz core; the sum over a model's lines x alkali_density_d[w][l][model].
 *     lorentz, dsigma and voigt_det are formed per (walker, layer) on the device
 *     (pb_alkali_voigt_det_batch's arithmetic) from alkali_pressure_d[nlayers] (barye).  At most
 *     PB_CONT_MAX_ALKALI models with PB_CONT_MAX_ALKALI_LINES lines in all; nalkali = 0: none,
 *     the alkali fields are not read. */
#define PB_CONT_MAX_RANK1 8
#define PB_CONT_MAX_CIA 4
#define PB_CONT_MAX_ALKALI 2
#define PB_CONT_MAX_ALKALI_LINES 4
typedef struct pb_cont_batch {
    int nrank1;
    int rank1_kind[PB_CONT_MAX_RANK1];
    int rank1_species[PB_CONT_MAX_RANK1];
    int rank1_par[PB_CONT_MAX_RANK1];
    double rank1_s0[PB_CONT_MAX_RANK1];
    double rank1_l0[PB_CONT_MAX_RANK1];
    const double *rank1_cs_d[PB_CONT_MAX_RANK1];
    const double *rank1_pressure_d[PB_CONT_MAX_RANK1];
    int ncia;
    int cia_ntemp[PB_CONT_MAX_CIA];
    int cia_nspec[PB_CONT_MAX_CIA];
    int cia_species[PB_CONT_MAX_CIA][PB_CONT_MAX_CIA];
    const double *cia_tab_d[PB_CONT_MAX_CIA];
    const double *cia_temps_d[PB_CONT_MAX_CIA];
    const uint8_t *cia_mask_d;
    int hminus;
    int hm_species[2];
    const double *hm_sigma_bf_d;
    const double *hm_ff_d;
    const double *wn_d;
    const double *density_d;
    int ncs;
    const double *pars_d;
    int npars;
    int pars_stride;
    /* alkali doublets (appended: the layout above is unchanged) */
    int nalkali;
    int alkali_nlines[PB_CONT_MAX_ALKALI];
    double alkali_wn0[PB_CONT_MAX_ALKALI][PB_CONT_MAX_ALKALI_LINES];
    double alkali_gf[PB_CONT_MAX_ALKALI][PB_CONT_MAX_ALKALI_LINES];
    double alkali_detuning[PB_CONT_MAX_ALKALI];
    double alkali_mass[PB_CONT_MAX_ALKALI];
    double alkali_lpar[PB_CONT_MAX_ALKALI];
    double alkali_part_func[PB_CONT_MAX_ALKALI];
    double alkali_cutoff[PB_CONT_MAX_ALKALI];
    const double *alkali_pressure_d;
    const double *alkali_density_d;
} pb_cont_batch;
/* Device scratch (doubles) of the two calls below: the interpolation weights, the per-(walker,
 * layer) continuum scalars and the per-walker Lecavelier rows [nlec][nwalkers][nwave]; -1 when
 * cont is invalid. */
int64_t pb_interp_ec_batch_cont_work_doubles(const pb_cont_batch *cont, int nlayers, int nwave,
                                             int nwalkers);
/* pb_interp_ec_batch / pb_interp_ec_batch_limited + the continuum terms of `cont` (a host
 * struct).  A gated repair call (gate_d != NULL) reuses the scalars and rows its first call left
 * in work_d.  Arguments are checked before any HIP call. */
int pb_interp_ec_batch_cont(double *ec_d, const double *etable_d, const double *ttable_d,
                            const double *temps_d, const double *density_d, void *work_d,
                            int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                            const pb_cont_batch *cont, void *stream);
int pb_interp_ec_batch_cont_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                                    const double *temps_d, const double *density_d, void *work_d,
                                    int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                                    const pb_cont_batch *cont, const int32_t *tile_limit_d,
                                    int row0, const int32_t *gate_d, void *stream);

/* The Voigt value of every line of an alkali model at the detuning distance, for a batch of
 * walkers (VanderWaals.voigt_det, alkali.py:48-82 -> broadening.py:231-260), one launch:
 *   dsigma = detuning (T/500)^0.6, lorentz = lpar (T/2000)^-0.7 p/1.01e6, hwhm_G of `mass` at T
 *   out_d[w][l][j] = Voigt(wn0[j] + dsigma): Re w(z)/(sigma sqrt(pi)), z = (dsigma + i lorentz)/sigma
 *     where lorentz/hwhm_G < 0.1, else the four-term rational approximation.
 * Re w(z) is the Laplace continued fraction with 6 levels: exact to 8e-15 for Re z >= 20 (the
 * shipped models: 570 ... 1069); the caller keeps a model out whose Re z is smaller.
 * temps_d[nwalkers][nlayers], pressure_d[nlayers] (barye), wn0_h[nlines] (host, at most
 * PB_CONT_MAX_ALKALI_LINES). */
int pb_alkali_voigt_det_batch(double *out_d, const double *temps_d, const double *pressure_d,
                              double detuning, double mass, double lpar, const double *wn0_h,
                              int nlines, int nlayers, int nwalkers, void *stream);

/* The retrieval batch with clouds: an opaque deck at a per-walker pressure (opacity/clouds/
 * gray.py:95-154; pyrat_obj.py:135-139; spectrum/radiative_transfer.py:63-67, 125-127) and patchy
 * clouds (pyrat_obj.py:285-286, opacity/optic_depth.py:94-136, pyrat/spectrum.py:357-384).
 *
 * Deck state of every walker, p = 10^logp_d[w] bar on pressure_d[nlayers] (bar, ascending):
 *   itop  = first layer with pressure >= p; nlayers - 1 if p >= pressure[nlayers-1] (or NaN);
 *           1 (at most nlayers - 1) if p < pressure[0]
 *   rsurf, tsurf = radius and temperature at p, linear in pressure, CLAMPED to the end values
 *           outside the grid (the reference's interp1d raises there)
 * radius_d[w * radius_stride + l] (radius_stride = 0: one profile for all), temps_d[nwalkers,
 * nlayers].  One launch, nothing read back. */
int pb_deck_state_batch(int32_t *itop_d, double *rsurf_d, double *tsurf_d,
                        const double *pressure_d, const double *logp_d, const double *radius_d,
                        int64_t radius_stride, const double *temps_d, int nlayers, int nwalkers,
                        void *stream);
/* ec_cloud = sum_m cs_m[sample] f_m[walker, layer], m in model order, is never stored: the
 * kernels below add it to ec as they walk a column.  cs_d[m]: NULL (a row of ones: gray) or the
 * cross sections in ec's column order at cs_d[m][w * cs_stride[m] + sample] (cs_stride 0: one row
 * for all walkers; nwave: a row per walker); f_d[nwalkers][nlayers][nr]. */
#define PB_CLOUD_MAX 8
typedef struct pb_cloud_terms {
    int nr;
    const double *cs_d[PB_CLOUD_MAX];
    int64_t cs_stride[PB_CLOUD_MAX];
    const double *f_d;
} pb_cloud_terms;
/* The factors of the cloud-type models of a Continuum from the walkers' parameters, as
 * pb_interp_ec_batch_cont forms them for the same models in ec (kind 1 Lecavelier: f = p BAR/T/K,
 * cross sections 10^p[par] s0 (wn l0)^-p[par+1] into rows_d[j][nwalkers][nwave], j counting the
 * Lecavelier models; kind 2 CCSgray: f = 10^p[par] s0 p BAR/T/K between 10^p[par+1] and
 * 10^p[par+2] bar, else 0).  f_d[nwalkers][nlayers][nr]; pars_stride 0: one row for all. */
typedef struct pb_cloud_models {
    int nr;
    int kind[PB_CLOUD_MAX];
    int par[PB_CLOUD_MAX];
    double s0[PB_CLOUD_MAX];
    double l0[PB_CLOUD_MAX];
    const double *pressure_d[PB_CLOUD_MAX];
} pb_cloud_models;
int pb_cloud_plan(double *f_d, double *rows_d, const pb_cloud_models *models,
                  const double *temps_d, const double *pars_d, int pars_stride,
                  const double *wn_d, int nlayers, int nwave, int nwalkers, void *stream);
/* Transit geometry, one pass over ec_d[nwalkers,nlayers,nwave] for both columns of a walker:
 *   clear : ec over [itop, nlayers), no deck
 *   cloudy: ec + ec_cloud over [itop, deck_itop + 1); the interval that ends at the deck ends at
 *           deck_rsurf with the integrand interpolated linearly in radius (nothing is replaced
 *           when deck_itop <= itop); no deck (deck_itop_d NULL): down to the last layer
 *   spectrum = f cloudy + (1 - f) clear, f = f_patchy_d[w] clamped to [0, 1] (NaN stays NaN);
 *           f_patchy_d NULL: spectrum = cloudy, and the clear column is not walked
 * With cloud == NULL (or nr = 0) the two optical depths are equal row for row down to the deck and
 * are summed once.  raypath_d[w * path_stride + .] = pb_transit_path's packed triangle,
 * radius_d[w * radius_stride + l] (stride 0: shared).  column_d (or NULL): ec_d's columns are in
 * that order (grid index of each), the outputs in grid order; per column the arithmetic does not
 * depend on the order.  clear_d / cloudy_d (or NULL): the two parts.  At most 1024 impact
 * parameters. */
int pb_cloudy_transit_batch(double *spectrum_d, double *clear_d, double *cloudy_d,
                            const double *ec_d, const double *raypath_d, int64_t path_stride,
                            const double *radius_d, int64_t radius_stride,
                            const int32_t *column_d, double rstar, int itop, double maxdepth,
                            int nlayers, int nwave, int nwalkers, const int32_t *deck_itop_d,
                            const double *deck_rsurf_d, const pb_cloud_terms *cloud,
                            const double *f_patchy_d, void *stream);
/* Emission geometry (pb_emission_flux_batch's pass): the cloudy column stops at deck_itop (the
 * reference clips ideep to it), layer deck_itop radiates at deck_tsurf_d[w] -- in the CLEAR
 * column too: the reference's cloudy pass overwrites that row of its Planck array and the clear
 * pass reads it (spectrum/radiative_transfer.py:125-126, pyrat/spectrum.py:380-383).  wn_d in
 * ec_d's column order. */
int pb_cloudy_emission_batch(double *flux_d, double *clear_d, double *cloudy_d, const double *ec_d,
                             const double *intervals_d, const double *wn_d, const double *temp_d,
                             const double *mu_d, const double *weights_d, const int32_t *column_d,
                             int nmu, double maxdepth, int itop, int nlayers, int nwave,
                             int nwalkers, const int32_t *deck_itop_d, const double *deck_tsurf_d,
                             const pb_cloud_terms *cloud, const double *f_patchy_d, void *stream);

/* The walkers' atmospheres from their parameter vectors: what Atmosphere.calc_profiles
 * (pyratbay/pyrat/atmosphere.py:399-526) makes of the parameters eval() maps (pyrat_obj.py:258-275),
 * for a batch, in ONE launch with no host read-back and no allocation (graph-capturable):
 *   temperature  tmodel 0 isothermal, 1 guillot (src_c/_pt.c:11-15, 88-109; E2 by power series
 *                for x <= 1 and continued fraction above, 0 for x > log(2^127) like the reference),
 *                2 madhu (tmodels.py:301-325; the smoothing of gaussian_filter1d(mode='nearest')
 *                as a clamped-index correlation with the 2 madhu_radius + 1 host-made weights)
 *   abundances   nvmr models on species vmr_species[i]: kind 0 IsoVMR, 1 ScaleVMR (its vmr0 in row
 *                i of vmr0_d[nvmr][nlayers]), 2 SlantVMR (vmr_models.py:129-347), parameters from
 *                column vmr_par[i]; then the bulk balance of vmr_scale (vmr_scaling.py:69-126,
 *                259-278, qsat = None) with bulk_ratio_d[nlayers][nbulk], invsrat_d[nlayers]
 *   density      ((vmr (p / T)) bar) / k (atmosphere.py:664), mean mass sum(vmr mass) (:626, in
 *                NumPy's pairwise order)
 *   radius       rmodel 0 hydro_m (:467-485), 1 hydro_g (:397-415): cumulative trapezoid over ln p
 *                summed left to right, the value at the reference pressure by SciPy's first-order
 *                spline, radius(p0) = r0
 * Free scalars: column par_rplanet (cm), par_log_refpressure (log10 bar), par_mplanet (g) of
 * params_d, or -1: the struct's constant.  All arithmetic in binary64.
 * CONSTANTS: this kernel uses those of pyratbay.constants, which the reference's Python code runs
 * with (CODATA 2018: k = 1.380649e-23 * 1e7 erg/K, G = 6.67430e-11 * 1e3, N_A = 6.02214076e23;
 * bar = 1e6) -- NOT the legacy values of the C extensions (pb_common.h), which every other kernel
 * of this library keeps.
 * Outputs, each written once: temps_d[nw][L], dens_d[nw][L][ntab] (species tab_map_d[j]),
 * radius_d[nw][L], mm_d[nw][L], cont_dens_d[nw][L][ncont] and alk_dens_d[nw][L][nalk] (or NULL with
 * a count of 0), reject_d[nw]: a bit mask, 0 = accepted.  A rejected walker gets temps = 0 (which
 * pb_reject_walkers turns into +inf band fluxes), densities and mean masses of 0 and
 * base_radius_d[L] as its radius.  The divergent hydro_m case deviates from the reference, which
 * would carry on above the layer where the profile turns over. */
#define PB_ATM_MAX_SPECIES 32
#define PB_ATM_MAX_VMR 16
#define PB_ATM_MAX_BULK 4
#define PB_ATM_MAX_LAYERS 1024
#define PB_ATM_REJECT_TEMP 1        /* a temperature <= 0 or not finite                     */
#define PB_ATM_REJECT_MADHU 2       /* madhu: log_p1 > log_p3                               */
#define PB_ATM_REJECT_QCAP 4        /* trace VMRs sum above qcap in a layer (:52-66)        */
#define PB_ATM_REJECT_REFPRESSURE 8 /* reference pressure outside the grid (interp1d raises) */
#define PB_ATM_REJECT_DIVERGENT 16  /* hydro_m: the radius does not decrease with index; either
                                       model: a radius <= 0 or not finite (a free rplanet or
                                       mplanet that is NaN, zero or negative)              */
typedef struct pb_atm_model {
    int nlayers, nspecies, npar;
    int tmodel;
    double guillot_gravity;             /* 1.0 for gravity = None */
    int madhu_radius;
    double madhu_logp0, madhu_loge;
    const double *madhu_weights_d;
    int nvmr;
    int vmr_kind[PB_ATM_MAX_VMR];
    int vmr_species[PB_ATM_MAX_VMR];
    int vmr_par[PB_ATM_MAX_VMR];
    const double *vmr0_d;
    int nbulk;
    int bulk_species[PB_ATM_MAX_BULK];
    const double *bulk_ratio_d, *invsrat_d;
    const double *base_vmr_d;           /* [nlayers][nspecies] */
    const double *pressure_d;           /* [nlayers] bar, ascending */
    const double *log10p_d, *lnp_d;     /* NumPy's log10 and log of it */
    const double *mass_d;               /* [nspecies] g mol-1 */
    int rmodel;
    int base_vmr_stride;                /* doubles from one walker's base_vmr_d to the next's;
                                           0: one base VMR shared by all walkers */
    double mplanet, gplanet, rplanet, refpressure;
    int par_rplanet, par_log_refpressure, par_mplanet;
    int has_qcap;
    double qcap;
    const double *base_radius_d;
    int ntab, ncont, nalk;
    const int32_t *tab_map_d, *cont_map_d, *alk_map_d;
} pb_atm_model;
/* The model struct (a host struct) is checked before any HIP call. */
int pb_walker_atmosphere(const pb_atm_model *model, const double *params_d, int nwalkers,
                         double *temps_d, double *dens_d, double *radius_d, double *mm_d,
                         double *cont_dens_d, double *alk_dens_d, int32_t *reject_d, void *stream);

/* ---- Equilibrium chemistry per walker (pb_chemistry.hip, pb_atmosphere.hip): the VMRs of every
 * (walker, layer) cell from the walkers' [M/H], [X/H] and X/Y, where the reference calls chemcat
 * (pyrat/atmosphere.py:445-473).  Three launches, nothing read back, no allocation:
 *   pb_walker_temperature     temps_d[nw][L]: the T(p) model of pb_walker_atmosphere (the same
 *                             statements, the same bits), as formed: no reject contract
 *   pb_equilibrium_vmr        vmr_d[nw][L][S], status_d[nw][L]
 *   pb_walker_atmosphere_chem pb_walker_atmosphere with model->base_vmr_d[nw][L][S] read per walker
 *                             (base_vmr_stride = L * S), nvmr = 0 and nbulk = 0 allowed (the
 *                             reference balances no bulk in equilibrium), and chem_status_d[nw][L]
 *                             folded into reject_d under PB_ATM_REJECT_CHEMISTRY: a status below 0
 *                             other than PB_CHEM_REJECTED, which is the temperature's own reject.
 *
 * pb_equilibrium_vmr: one wavefront per cell, lane i = species i, the gas-phase reduced Newton
 * iteration of Gordon & McBride (NASA RP-1311, section 2.3) on ln n_i and ln n from the cold start
 * n_i = 0.1 / S, n = 0.1, with mu_i = g_i + ln n_i - ln n + ln p (p in bar), g_i = np.interp of
 * column i of gibbs_d[ntemps][S] (G°/RT at 1 bar) at the cell's temperature; the symmetric system
 * of order E + 1 is summed by butterfly reductions and solved in every lane by Gaussian elimination
 * with partial pivoting; damping lambda = min(1, l1, l2) of RP-1311 eqs. 3.1-3.3; converged when
 * lambda == 1, n_i |dln n_i| / sum n < tolerance for every species and |dln n| < tolerance.
 * The elemental abundances b[E] come from the walker's parameters: dex = base_dex; elements with
 * is_metal get + params[par_metal] (par_metal -1: 0); [X/H] k sets dex[scale_element[k]] =
 * base_dex + params[scale_par[k]]; then X/Y k, in order, sets dex[ratio_num[k]] =
 * dex[ratio_den[k]] + log10(params[ratio_par[k]]); b_j = pow(10, dex_j - dex[ihydrogen]).
 * Hybrid k (a free log10 VMR on top of the equilibrium, the reference's hybrid_vmr): the column of
 * species hybrid_species[k] becomes clip(pow(10, params[hybrid_par[k]]), 0, max_vmr), max_vmr the
 * minimum over the species' elements j of (sum_i vmr_i a_ij) / a_kj, from the equilibrium VMRs;
 * nothing is renormalised.
 * status: the iteration count of a converged cell, or PB_CHEM_*; a cell with a negative status has
 * zeros in vmr_d and (but for PB_CHEM_NOT_CONVERGED) iterated nothing.  params_d may be NULL when
 * npar == 0.  The model struct (a host struct) is checked before any HIP call.
 *
 * Ions and electrons: charge_d[nspecies] (NULL: a neutral network, the solver above unchanged)
 * holds a species' charge; the electron is a species with an all-zero stoich row and charge -1.
 * The charge never enters stoich_d.  The charge balance sum_i q_i n_i = 0 takes one more row of the
 * system, so nelements + 1 <= PB_CHEM_MAX_ELEMENTS, and the cold solve has three steps:
 *   1. the neutral species alone, from the cold start of their sub-network (n_i = 0.1 / their
 *      count): the iteration above on the lanes with charge 0, the others adding 0 to every sum;
 *   2. every charged species is seeded from the potentials pi of that solve:
 *      ln n_i = t_i + q_i pi_q, t_i = ln n - g_i - ln p + sum_j a_ij pi_j, pi_q = (LSE- - LSE+) / 2
 *      with LSE the log-sum-exp of t_i over the species of one sign -- the neutral gas exactly for
 *      charges +-1 while the ions are trace, and in logarithms, so nothing underflows;
 *   3. the system of order nelements + 2 from there: the balance matrix is [stoich | charge], the
 *      right-hand side of the charge row 0, damping as above.
 * (From the cold start alone an ion would move by about one unit of ln n per iteration.)
 * Step 3 has converged when the test above holds AND |dln n_i| < 1e-9 for every charged species:
 * the test above weighs a step by n_i, and ions are trace species, so alone it does not see the
 * charge balance.  Where sum_i q_i^2 n_i == 0 (every ion has underflowed) the charge row and column
 * of that iteration are replaced by an identity row with right-hand side 0 and the charged species
 * keep their ln n_i.  Steps 1 and 3 are each capped at max_iterations; status is the sum of their
 * iteration counts; a failure of either gives PB_CHEM_NOT_CONVERGED.  A hybrid on a charged
 * species is for the caller to refuse (charge_d is device memory). */
#define PB_ATM_REJECT_CHEMISTRY 64  /* an equilibrium cell that did not converge, a temperature
                                       outside the Gibbs table, a bad element ratio (32 is
                                       PB_ISO_REJECT) */
#define PB_CHEM_MAX_SPECIES 64
#define PB_CHEM_MAX_ELEMENTS 8
#define PB_CHEM_MAX_HYBRID 16
#define PB_CHEM_REJECTED (-1)       /* temperature <= 0 or NaN: rejected before the chemistry */
#define PB_CHEM_TEMPERATURE (-2)    /* temperature outside gibbs_temps                        */
#define PB_CHEM_RATIO (-3)          /* an X/Y <= 0, an abundance not finite and positive      */
#define PB_CHEM_NOT_CONVERGED (-4)  /* max_iterations without a converged full step           */
typedef struct pb_chem_model {
    int nspecies, nelements, ntemps, nlayers, npar;
    int ihydrogen;
    double base_dex[PB_CHEM_MAX_ELEMENTS];
    int is_metal[PB_CHEM_MAX_ELEMENTS];
    int par_metal;
    int nscale;
    int scale_element[PB_CHEM_MAX_ELEMENTS];
    int scale_par[PB_CHEM_MAX_ELEMENTS];
    int nratio;
    int ratio_num[PB_CHEM_MAX_ELEMENTS];
    int ratio_den[PB_CHEM_MAX_ELEMENTS];
    int ratio_par[PB_CHEM_MAX_ELEMENTS];
    int nhybrid;
    int hybrid_species[PB_CHEM_MAX_HYBRID];
    int hybrid_par[PB_CHEM_MAX_HYBRID];
    int max_iterations;
    double tolerance;
    const double *gibbs_temps_d;        /* [ntemps] K, ascending */
    const double *gibbs_d;              /* [ntemps][nspecies] */
    const int32_t *stoich_d;            /* [nspecies][nelements] */
    const double *pressure_d;           /* [nlayers] bar */
    const int32_t *charge_d;            /* [nspecies], or NULL: a neutral network */
} pb_chem_model;
int pb_equilibrium_vmr(const pb_chem_model *model, const double *temps_d, const double *params_d,
                       int nwalkers, double *vmr_d, int32_t *status_d, void *stream);
/* The equilibrium inside the radiative-equilibrium loop (RadiativeEquilibrium(chemistry=...), the
 * reference's chem_model.thermochemical_equilibrium(temp) at the top of every iteration,
 * spectrum/radiative_transfer.py:202-203): pb_equilibrium_vmr's solver on temps_d[nw][L] with the
 * iterate of every cell carried from launch to launch, and the mean molecular mass.  Every pointer
 * is device memory. */
typedef struct pb_radeq_chem {
    double *ln_ni_d;                    /* [nw][L][S] the iterate ln n_i, carried */
    double *ln_n_d;                     /* [nw][L] its ln n, carried */
    double *vmr_d;                      /* [nw][L][S] out */
    double *mm_d;                       /* [nw][L] out: sum_i vmr_i mol_mass_i (xor butterfly over
                                           the 64 lanes, lanes past S adding 0) */
    const double *mol_mass_d;           /* [S] g mol-1 */
    int32_t *status_d;                  /* [nw][L] out: iteration count or PB_CHEM_* */
    int32_t *failures_d;                /* [nw][L] + 1 for every launch that left the cell with a
                                           negative status (the caller zeroes it) */
    double tol_all;                     /* > 0: a warm solve has converged once max_i |dln n_i|
                                           is below it (and the cold test holds) */
} pb_radeq_chem;
/* warm == 0: every cell from the cold start with the test of pb_equilibrium_vmr; vmr_d and
 * status_d are bit for bit its output; the converged iterate is stored.  warm != 0: a cell starts
 * from its stored iterate and has converged when that test holds AND |dln n_i| < tol_all for every
 * species (the test alone weighs a step by n_i and passes trace species that are still a factor
 * off after one step from a neighbouring solution); a stored iterate that is not finite, or
 * max_iterations without convergence, and the cell is solved from the cold start in the same
 * launch, its output then bit for bit the cold one.  status: the iteration count of the solve that
 * converged.  A cell that converges neither way, or whose temperature or abundances are refused
 * (PB_CHEM_*), keeps vmr_d, mm_d and its iterate AS THEY WERE (unlike pb_equilibrium_vmr, which
 * writes zeros: zeros would empty a layer of the next evaluation), gets the negative status and
 * + 1 in failures_d.  model->nhybrid must be 0.  No LDS, no barrier, no atomic.
 * With model->charge_d a warm cell goes straight to step 3 of the solve with charges (the full
 * system from its stored iterate, both tests above and that of the charged species), the cold
 * solve is the three steps, and mm_d includes the electrons through mol_mass_d. */
int pb_radeq_equilibrium(const pb_chem_model *model, const double *temps_d,
                         const double *params_d, int nwalkers, int warm,
                         const pb_radeq_chem *state, void *stream);
int pb_walker_temperature(const pb_atm_model *model, const double *params_d, int nwalkers,
                          double *temps_d, void *stream);
int pb_walker_atmosphere_chem(const pb_atm_model *model, const double *params_d, int nwalkers,
                              const int32_t *chem_status_d, double *temps_d, double *dens_d,
                              double *radius_d, double *mm_d, double *cont_dens_d,
                              double *alk_dens_d, int32_t *reject_d, void *stream);

/* ---- Isotope ratios of the table's slots (pb_isotopes.hip): Line_Sample's isotope_ratios
 * (pyratbay/opacity/line_sampling.py:282-298, 451-456: density * iso_ratios before interp_ec) for
 * a batch, in ONE launch with no host read-back and no allocation (graph-capturable).  The table
 * has nspec slots; nlabelled <= PB_ISO_MAX_SLOTS of them carry an isotope label, the others have
 * the ratio 1.0.  Labelled slot i is table slot slot[i] and has
 *   kind PB_ISO_CONST  ratio = constant[i]
 *   kind PB_ISO_FREE   ratio = pow(10.0, pars_d[w][par[i]])
 *   kind PB_ISO_FILL   ratio = 1 - (r_a + r_b + ...), the ratios of the labelled slots
 *                      fill[i][0 .. nfill[i]-1] (1 ... PB_ISO_MAX_FILLERS of them, none a fill slot
 *                      itself), summed left to right, every operation rounded on its own
 * dens_out_d[nw][L][nspec] = dens_in_d * ratio (one multiply), temps_out_d[nw][L] = temps_in_d,
 * ratios_out_d[nw][nspec] (or NULL), reject_out_d[nw].  A walker with a ratio that is negative or
 * not finite gets 0 in every element of dens_out_d and temps_out_d (pb_walker_atmosphere's reject
 * contract: pb_reject_walkers turns it into +inf band fluxes) and reject PB_ISO_REJECT, else 0;
 * its ratios_out row holds the ratios as formed.  pars_d[nw][npars] may be NULL when no slot is
 * PB_ISO_FREE.  Limits (PB_ERR_ARG beyond them): nspec <= 4096 (a walker's ratios are held in LDS),
 * nlayers * nspec <= INT32_MAX (a walker's slab is indexed in 32 bits).  The outputs may not
 * overlap the inputs.  The model struct (a host struct) is
 * checked before any HIP call.  nwalkers == 0: nothing launched. */
#define PB_ISO_MAX_SLOTS 32
#define PB_ISO_MAX_FILLERS 7
#define PB_ISO_CONST 0
#define PB_ISO_FREE 1
#define PB_ISO_FILL 2
#define PB_ISO_REJECT 32            /* continues the PB_ATM_REJECT_* bits */
typedef struct pb_iso_model {
    int nspec, npars, nlabelled;
    int slot[PB_ISO_MAX_SLOTS];
    int kind[PB_ISO_MAX_SLOTS];
    int par[PB_ISO_MAX_SLOTS];
    int nfill[PB_ISO_MAX_SLOTS];
    int fill[PB_ISO_MAX_SLOTS][PB_ISO_MAX_FILLERS];
    double constant[PB_ISO_MAX_SLOTS];
} pb_iso_model;
int pb_iso_density(double *dens_out_d, double *temps_out_d, double *ratios_out_d,
                   int32_t *reject_out_d, const double *dens_in_d, const double *temps_in_d,
                   const double *pars_d, const pb_iso_model *model, int nlayers, int nwalkers,
                   void *stream);

/* ---- Posterior summary: weighted column quantiles (pb_quantiles.hip).  The reduction of
 * posterior_post_processing (pyratbay/tools/retrieval_tools.py:384-503: np.percentile of
 * models[uinv] along the samples, per wavenumber / band / layer) on the UNIQUE samples and their
 * multiplicities; the expansion is never formed.
 *
 * values_d[ncol][ld] (sample-minor: a column's n samples are contiguous, ld >= n, the padding is
 * never read), counts_d[n] >= 0 (how often the chain visited sample i; shared by the columns; a
 * row with count 0 does not exist; the counts may sum past 2^31).  With a_k = the element of rank
 * k of column c's samples, each repeated counts[i] times and sorted (N = sum of counts elements):
 *   out_d[q][c] = lerp(a_{rank_lo[q]}, a_{rank_hi[q]}, gamma[q])
 * with NumPy's lerp, every operation rounded on its own: d = b - a; a + d t, and b - d (1 - t)
 * where t >= 0.5.  The caller forms rank_lo_d[nq], rank_hi_d[nq] (0 <= rank < N), gamma_d[nq]
 * (device memory) the way np.percentile(method='linear') does; the result then has np.percentile's
 * bits (pyratbay_amd/posterior.py: weighted_quantiles_host is the NumPy statement).  Exact
 * selection (a weighted radix select on the order-preserving key of the double, integer
 * histograms in LDS), no floating-point atomics: two runs give the same bits.  Values order by
 * that key: -0.0 before +0.0, NaNs of positive sign last.  A column whose counts are all zero
 * (the caller's error), and a quantile with a rank outside [0, N), get NaN.
 * n <= pb_weighted_quantiles_resident_rows(): the column is read once and kept in LDS; above, every
 * pass re-reads it.  work_d: pb_weighted_quantiles_work_doubles(n, ncol, nq) doubles of device
 * scratch (0 today: NULL is then accepted).  Refused before any launch (PB_ERR_ARG): n < 1,
 * nq < 1, ncol < 0, ld < n, a null pointer; ncol == 0 succeeds and launches nothing. */
int pb_weighted_quantiles(double *out_d, const double *values_d, int64_t ld,
                          const int64_t *counts_d, int n, int ncol, const int64_t *rank_lo_d,
                          const int64_t *rank_hi_d, const double *gamma_d, int nq, double *work_d,
                          void *stream);
int64_t pb_weighted_quantiles_work_doubles(int n, int ncol, int nq);
int pb_weighted_quantiles_resident_rows(void);

/* ---- Band contribution functions per walker (pb_contribution.hip): Pyrat.band_contribution
 * (pyrat/pyrat_obj.py:671-696 -> spectrum/contribution_funcs.py) for a batch: first without
 * clouds, then -- the two *_cloudy_batch entries at the end -- with them.
 * The bands are the four arrays of pb_band_integrate_batch (the heights cancel and are not taken)
 * plus max_band_count >= every band_count_d[b]; a band's samples are wn_d[start .. start + count),
 * clipped to the grid.  At a clip the band's end weight is one-sided (the trapezoid of the retained
 * samples; response_d stays indexed by the unclipped position) and wn_d is never read outside
 * [0, nwave); a clipped band has the bits of the in-grid band of its retained samples.  out_d[nwalkers,nlayers,nbands] = the band integrals (np.trapezoid of
 * value x response over the band's samples), each band divided by its maximum over the layers: a
 * band of one sample (or none) is 0 / 0 = NaN in every layer, like the reference.
 * work_d: pb_band_contribution_work_doubles(nlayers, nbands, max_band_count, nwalkers) doubles of
 * device scratch, written before it is read.  FP64, no atomics, fixed summation order: two runs
 * give the same bits.  Refused before any launch (PB_ERR_ARG): bad sizes, itop outside the
 * layers, ibottom > nlayers, more than 65535 bands or walkers, more layers than the LDS of a
 * workgroup holds (1024 emission, 2048 transit), a null pointer; nbands == 0 or nwalkers == 0
 * succeed and launch nothing.
 *
 * Emission and two-stream geometry: contribution_function from ec_d[nwalkers,nlayers,nwave]
 * directly -- per column the plane-parallel depth with pb_emission_flux_batch's stop rule
 * (maxdepth = inf in two-stream geometry: no stop; the rows up to itop and below the stop are 0),
 * detau = diff(exp(-depth)) with the elements > 0.1 set to 0, B = Planck at every layer of
 * temps_d[nwalkers,nlayers], cf = B detau / dlogp_d[nlayers-1] (= diff(log(pressure)), shared by
 * the walkers), a zero last row, each column divided by its sum.  Neither depth nor B is stored.
 * intervals_d[nwalkers,nlayers-1] = -diff(radius).  nlayers >= 2. */
int pb_band_contribution_emission_batch(double *out_d, const double *ec_d,
                                        const double *intervals_d, const double *dlogp_d,
                                        const double *wn_d, const double *temps_d,
                                        const int32_t *band_start_d, const int32_t *band_count_d,
                                        const double *response_d,
                                        const int64_t *response_offset_d, int max_band_count,
                                        double maxdepth, int itop, int ibottom, int nlayers,
                                        int nwave, int nbands, int nwalkers, double *work_d,
                                        void *stream);
/* Transit geometry: transmittance from depth_d[nwalkers,nlayers,nwave] and ideep_d[nwalkers,nwave]
 * as pb_transit_spectrum_batch(..., depth_d, ideep_d) leaves them: exp(-depth[r]) for r < ideep,
 * 0 from row ideep on; the rows above itop are 1 and are not read.  ideep_d values outside
 * [0, nlayers] are taken as the nearer end. */
int pb_band_transmittance_batch(double *out_d, const double *depth_d, const int32_t *ideep_d,
                                const double *wn_d, const int32_t *band_start_d,
                                const int32_t *band_count_d, const double *response_d,
                                const int64_t *response_offset_d, int max_band_count, int itop,
                                int nlayers, int nwave, int nbands, int nwalkers, double *work_d,
                                void *stream);
int64_t pb_band_contribution_work_doubles(int nlayers, int nbands, int max_band_count,
                                          int nwalkers);
/* The same with clouds (pyrat_obj.py:129-164, 671-696; opacity/optic_depth.py:91-136): per walker
 * an opaque deck at layer deck_itop_d[w] (pb_deck_state_batch; NULL: no deck), cloud-type opacity
 * ec_cloud from `cloud` (pb_cloud_terms in ec_d's column order, i.e. grid order; NULL or nr = 0:
 * none), which is added to ec_d as a column is walked and never stored, and in transit geometry a
 * patchy fraction.  Bands, out_d, work_d (the same pb_band_contribution_work_doubles), the
 * summation order and the refusals are those of the two entries above; also refused: more than
 * PB_CLOUD_MAX cloud terms, null cloud factors.  Neither entry stores a depth.
 *
 * Emission: pb_band_contribution_emission_batch on the CLOUDY column only, as the reference --
 * the clear column of a patchy model is not mixed in and a patchy fraction does not enter:
 *   the column is ec + ec_cloud; with a deck the stop rule's ibottom is deck_itop_d[w] + 1 (the
 *   ibottom argument otherwise), so the depth runs through the row past the deck, as the
 *   reference's loop stores row ibottom before it stops; row deck_itop_d[w] of B is the Planck
 *   function at deck_tsurf_d[w] (spectrum/radiative_transfer.py:125-127 writes it in place).
 * deck_itop_d and deck_tsurf_d go together; deck_itop_d values outside [0, nlayers) are taken as
 * the nearer end. */
int pb_band_contribution_emission_cloudy_batch(
    double *out_d, const double *ec_d, const double *intervals_d, const double *dlogp_d,
    const double *wn_d, const double *temps_d, const int32_t *band_start_d,
    const int32_t *band_count_d, const double *response_d, const int64_t *response_offset_d,
    int max_band_count, double maxdepth, int itop, int ibottom, int nlayers, int nwave, int nbands,
    int nwalkers, const int32_t *deck_itop_d, const double *deck_tsurf_d,
    const pb_cloud_terms *cloud, double *work_d, void *stream);
/* Transit: from ec_d[nwalkers,nlayers,nwave] and the ray paths of pb_cloudy_transit_batch
 * (raypath_d[w * path_stride + .] = pb_transit_path's packed triangle from itop; stride 0:
 * shared), with that entry's walk.  Two columns per walker:
 *   clear : ec over the rows itop .. nlayers-1
 *   cloudy: ec + ec_cloud over the rows itop .. deck_itop (no deck: nlayers-1)
 * In each, ideep = the first row whose depth exceeds maxdepth, else the column's last row
 * (deck_itop <= itop: itop, the cloudy column has no row), and the transmittance is 1 above itop,
 * exp(-depth[r]) for itop <= r < ideep and 0 from row ideep on.  A layer's value is
 * f T_cloudy + (1 - f) T_clear, f = f_patchy_d[w] clamped to [0, 1] (NaN stays NaN), formed per
 * sample BEFORE the band integral; f_patchy_d NULL: T_cloudy, and the clear column is not walked.
 * The deck's radius does not enter.  With cloud == NULL (or nr = 0) one running sum serves both
 * columns.  A sum of two layers' opacities is capped at the largest finite double, as in
 * pb_cloudy_transit_batch.
 * LDS of a workgroup: 4 nlayers doubles of wavefront sums + 16 (nlayers - itop) doubles of staged
 * ray-path segments; 64 KiB hold that for nlayers <= PB_BAND_CLOUDY_MAX_LAYERS, more is refused. */
#define PB_BAND_CLOUDY_MAX_LAYERS 400
int pb_band_transmittance_cloudy_batch(double *out_d, const double *ec_d, const double *raypath_d,
                                       int64_t path_stride, const double *wn_d,
                                       const int32_t *band_start_d, const int32_t *band_count_d,
                                       const double *response_d,
                                       const int64_t *response_offset_d, int max_band_count,
                                       int itop, double maxdepth, int nlayers, int nwave,
                                       int nbands, int nwalkers, const int32_t *deck_itop_d,
                                       const pb_cloud_terms *cloud, const double *f_patchy_d,
                                       double *work_d, void *stream);

/* =========================================================================
 * Line lists to TLI columns  (the reference's `runmode = tli`: Hitran.dbread,
 * pyratbay/opacity/linelist/hitran.py:173-203; Exomol.dbread, exomol.py:177-204)
 * ========================================================================= */
/* flag bits of a record (flags_d): a field whose text is not on the fast path of the conversion
 * (pb_linelist.hip: an integer of at most 2^53 times or over a power of ten up to 1e22) or not in
 * its grammar, which the host reads with float() / int() instead; an isotope character that the
 * map does not have; a record with fewer than three tokens; a state id outside [0, nstates) */
#define PB_LL_HITRAN_ISO 1
#define PB_LL_HITRAN_WN 2
#define PB_LL_HITRAN_A21 4
#define PB_LL_HITRAN_ELOW 8
#define PB_LL_HITRAN_G2 16
#define PB_LL_EXOMOL_UP 1
#define PB_LL_EXOMOL_LOW 2
#define PB_LL_EXOMOL_A21 4
#define PB_LL_EXOMOL_TOKEN 8
#define PB_LL_EXOMOL_STATE 16
/* text_d[nrec * recsize]: nrec whole records of recsize bytes (153 ... 255 for HITRAN, 5 ... 255
 * for ExoMol), at any byte alignment -> wn_d, elow_d, a21_d, g2_d [nrec] doubles, iso_d [nrec]
 * int16 (HITRAN: the index of the record's isotope character, '1'..'9' -> 0..8, '0' -> 9,
 * 'A' -> 10, 'B' -> 11; ExoMol: `iso`), flags_d [nrec].  A flagged field is written as NaN (the
 * isotope as -1) and *nflagged_d, which the caller zeroes, grows by one per flagged record.
 * ExoMol: energy_d, degeneracy_d [nstates] doubles, dense in the state id; wn = E[up] - E[low],
 * elow = E[low], g2 = g[up]. */
int pb_parse_hitran(const uint8_t *text_d, int64_t nrec, int recsize, double *wn_d, double *elow_d,
                    double *a21_d, double *g2_d, int16_t *iso_d, uint8_t *flags_d,
                    int32_t *nflagged_d, void *stream);
int pb_parse_exomol(const uint8_t *text_d, int64_t nrec, int recsize, const double *energy_d,
                    const double *degeneracy_d, int64_t nstates, int iso, double *wn_d,
                    double *elow_d, double *a21_d, double *g2_d, int16_t *iso_d, uint8_t *flags_d,
                    int32_t *nflagged_d, void *stream);
/* gf_d[n] = g2 * a21 * c1 / divisor / (wn * wn), every operation rounded on its own, in this
 * order (NumPy's of hitran.py:199) */
int pb_linelist_gf(const double *wn_d, const double *a21_d, const double *g2_d, int64_t n,
                   double c1, double divisor, double *gf_d, void *stream);

/* =========================================================================
 * Partition functions from ExoMol states  (the reference's `pf` step: exomol_states,
 * pyratbay/opacity/partitions/partitions.py:329-427)
 * ========================================================================= */
/* flag bits of a `.states` record (flags_d): the id, the energy or the degeneracy token is off
 * the fast path or outside its grammar (id: an optional '+' and 1 ... 18 digits; degeneracy: an
 * optional '+' and 1 ... 15 digits; energy: the decimal rule of the line-list kernels); fewer than
 * three blank-separated tokens end within bytes 0 ... 32, or a white-space byte other than the
 * blank lies there; the record's layout: byte recsize - 1 is no line feed, a line feed lies
 * earlier, or the energy and degeneracy tokens do not lie wholly inside bytes 12 ... 31 */
#define PB_LL_STATES_ID 1
#define PB_LL_STATES_ENERGY 2
#define PB_LL_STATES_G 4
#define PB_LL_STATES_TOKEN 8
#define PB_LL_STATES_LAYOUT 16
/* records of one workgroup of pb_parse_states; temperatures of one tile and the smallest number
 * of states of one chunk of pb_pf_states */
#define PB_STATES_RECORDS_PER_BLOCK 128
#define PB_PF_TEMPS_PER_TILE 1024
#define PB_PF_MIN_CHUNK 1024
#define PB_PF_MAX_CHUNKS 4096
/* text_d[nrec * recsize]: nrec whole records of recsize bytes (33 ... 255, the line feed
 * included), at any byte alignment -> id_d [nrec] int64, energy_d, degeneracy_d [nrec] doubles,
 * flags_d [nrec]: the first three blank-separated tokens as integer, decimal, integer.  A flagged
 * token is written as -1 (id) or NaN, all three of a record with a token or layout flag, and
 * *nflagged_d, which the caller zeroes, grows by one per flagged record. */
int pb_parse_states(const uint8_t *text_d, int64_t nrec, int recsize, int64_t *id_d,
                    double *energy_d, double *degeneracy_d, uint8_t *flags_d, int32_t *nflagged_d,
                    void *stream);
/* q_d[ntemp] = sum_j degeneracy_d[j] * exp((-c2 * energy_d[j]) * (1 / temp_d[t])) over the nstates
 * states (0 ... 2^31-1; ntemp 0 ... 65536).  The states are cut into chunks of a size that is
 * a function of (nstates, ntemp) alone; one partial per (chunk, temperature)
 * goes to work_d [pb_pf_states_work(nstates, ntemp) doubles] and the partials of a temperature
 * are added in ascending chunk order: no atomics, the same bits on every call and stream.  q_d and
 * work_d may hold anything on entry.  nstates = 0 gives zeros; ntemp = 0 launches nothing.
 * pb_pf_states_work writes the two sizes to host memory: sizes_h[0] the doubles of work_d (0 when
 * there is nothing to launch: work_d may then be null), sizes_h[1] the states per chunk. */
int pb_pf_states_work(int64_t nstates, int ntemp, int64_t sizes_h[2]);
int pb_pf_states(const double *energy_d, const double *degeneracy_d, int64_t nstates,
                 const double *temp_d, int ntemp, double c2, double *q_d, double *work_d,
                 void *stream);

/* =========================================================================
 * Experiments -- NOT in libpbhip.so.  `make -C pyratbay_amd/csrc EXPERIMENTS=1` builds
 * libpbhip_exp.so (compiled with -DPB_EXPERIMENTS) = the product library + the variants that were
 * built, verified and measured SLOWER than the default path (profiles/notes_r0*.md): gather modes
 * 4 (scatter), 5 (rounds), 7 (wave) of pb_lbl_set_gather_mode, the layers-outer and the one-pass
 * matrix transit kernels, the LDS-tile transit kernel, predicted run plans of the `resolution`
 * mode.  Their entry points:
 * ========================================================================= */
#ifdef PB_EXPERIMENTS
/* Which layers of the last call the wave-autonomous kernel computed (wave_h[nlayers], 0/1: the
 * layers whose longest phase row is at most 384 samples; all 0 when that kernel was off).
 * Synchronises the stream. */
int pb_lbl_last_wave_layers(pb_lbl *p, int32_t *wave_h, int nlayers, void *stream);
/* `resolution` plans in gather mode 6 (per-layer dynamic grids, _extcoeff.c:185-195, 320-326): the
 * run plan of a call -- which layers share an oversampling factor, which Lorentz rows of the re-cut
 * tables they read -- needs the layers' factors on the host: one stream synchronisation per call.
 * pb_lbl_set_dyn_predict(plan, 1) removes it: from the second call on the plan is taken from the
 * last read-back (asynchronous), a device check marks the layers it fits and the direct gather
 * computes the others, so the result is right whatever the prediction (to the direct gather's
 * 1e-12 of the dynamic grids; bit for bit while the prediction fits, i.e. always for a steady
 * atmosphere), and such calls can be captured into a HIP graph.  A read-back that contradicts its
 * prediction makes the next 8 calls synchronous.  Default off (PB_RES_DYN_PREDICT=1: on).
 * stats = {calls planned from a prediction, synchronous calls, read-backs that contradicted their
 * prediction}. */
int pb_lbl_set_dyn_predict(pb_lbl *p, int on);
int pb_lbl_dyn_stats(pb_lbl *p, int64_t stats[3]);
/* interp_ec + optical depth + transmission of a batch in ONE pass (the retrieval inner loop,
 * pyrat_obj.py:225-385: opacity/line_sampling.py:394-463 -> _extcoeff.c:367-418, then
 * opacity/optic_depth.py:103-112 and spectrum/radiative_transfer.py:57-71, no cloud deck):
 * etable_d[nmol,ntemp,nlayers,nwave], temps_d[nwalkers,nlayers], density_d[nwalkers,nlayers,nmol],
 * raypath_d[nwalkers, n(n-1)/2], radius_d[nwalkers,nlayers] -> spectrum_d[nwalkers,nwave].
 * The interpolated extinction is formed in registers as the operand of the FP64 matrix products
 * and never stored.  From two walkers on, neighbours in an order of the walkers by their table
 * brackets share a wavefront and one set of table loads (decided on the device; a batch whose
 * pairs bracket different temperatures in more than a fifth of the layers runs one walker per
 * wavefront).  pb_table_transit_supported(...) != 0 says whether the shape has this form
 * (2..128 impact parameters, nwave >= 2, one species' block of the table below 4 GiB); work_d: pb_table_transit_work_doubles(...) doubles. */
int pb_table_transit_supported(int nmol, int ntemp, int nlayers, int itop, int ibottom,
                               int nwave);
int64_t pb_table_transit_work_doubles(int nmol, int nlayers, int itop, int ibottom, int nwalkers);
int pb_table_transit_batch(double *spectrum_d, const double *etable_d, const double *ttable_d,
                           const double *temps_d, const double *density_d,
                           const double *raypath_d, const double *radius_d, double rstar,
                           int itop, int ibottom, double maxdepth, int nmol, int ntemp,
                           int nlayers, int nwave, int nwalkers, void *work_d, void *stream);
#endif /* PB_EXPERIMENTS */

#ifdef __cplusplus
}
#endif
#endif /* PBHIP_H */

/*
 * fcx.h -- C ABI of the MI355X exchange-grid flux engine (libfcx.so).
 *
 * This is the drop-in boundary for the per-coupling-step flux path of the IOW-ESM
 * flux_calculator.  It replaces the compute of module flux_calculator_calculate
 * (/root/reference/src/flux_calculator_calculate.F90) and do_regridding
 * (flux_calculator_basic.F90:463-522); the Fortran host keeps its data model, OASIS
 * put/get and namcouple surface.  The iso_c_binding shim that binds these entry points
 * under the reference subroutine names is
 * components.flux_calculator_amd/fortran/flux_calculator_calculate.F90.
 *
 * Plain C: integers, doubles and opaque handles only.  Every entry point returns an int
 * status (FCX_OK == 0); on failure fcx_last_error() returns a message (thread-local).
 * The reference calc_* never fail at run time (validation happens in
 * flux_calculator_prepare.F90); here validation happens in fcx_commit and later calls
 * only fail on HIP errors or misuse.  Not re-entrant per engine (one engine per rank and
 * GPU, calls serialised by the host loop, as in the reference).
 */
#ifndef FCX_H
#define FCX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCX_VERSION 1
#define FCX_MAX_SURFACE_TYPES 10 /* flux_calculator_basic.F90:28 */
#define FCX_NUM_VARS 35          /* flux_calculator_basic.F90:42 */

/* Variable ids: identical to the reference idx_* values (flux_calculator_basic.F90:526-568). */
enum fcx_var {
  FCX_ALBE = 1, FCX_ALBA, FCX_AMOI, FCX_AMOM, FCX_FARE, FCX_FICE, FCX_PATM, FCX_PSUR,
  FCX_QATM, FCX_TATM, FCX_TSUR, FCX_UATM, FCX_VATM, FCX_U10M, FCX_V10M,
  FCX_CMOM, FCX_CMOI, FCX_CHEA, FCX_QSUR, FCX_HLAT, FCX_HSEN,
  FCX_MEVA, FCX_MPRE, FCX_MRAI, FCX_MSNO,
  FCX_RBBR, FCX_RLWD, FCX_RLWU, FCX_RSID, FCX_RSIU, FCX_RSIN, FCX_RSDD, FCX_RSDR,
  FCX_UMOM, FCX_VMOM
};

/* which_grid: 1 = t_grid, 2 = u_grid, 3 = v_grid (flux_calculator_basic.F90:64) */
enum fcx_grid { FCX_T_GRID = 1, FCX_U_GRID = 2, FCX_V_GRID = 3 };

/* Method strings of the namelist which_* tables (flux_calculator.F90:99-107). */
enum fcx_method {
  FCX_NONE = 0, FCX_ZERO, FCX_COPY, FCX_CCLM, FCX_MOM5, FCX_RCO, FCX_WATER, FCX_ICE, FCX_STBO
};

/* The which_* tables, in the order of the namelist (flux_calculator.F90:99-107). */
enum fcx_flux {
  FCX_SPEC_VAPOR_SURFACE_T = 0, FCX_SPEC_VAPOR_SURFACE_U, FCX_SPEC_VAPOR_SURFACE_V,
  FCX_FLUX_MASS_EVAP, FCX_FLUX_HEAT_LATENT, FCX_FLUX_HEAT_SENSIBLE, FCX_FLUX_MOMENTUM,
  FCX_FLUX_RADIATION_BLACKBODY, FCX_NUM_FLUXES
};

/* Coupling-step phases (flux_calculator.F90:872-936 early, :942-1026 normal). */
enum fcx_phase { FCX_PHASE_EARLY = 1, FCX_PHASE_NORMAL = 2, FCX_PHASE_ALL = 3 };

/* Regridding matrices (flux_calculator.F90:330-337). */
enum fcx_regrid { FCX_U_TO_T = 0, FCX_V_TO_T, FCX_T_TO_U, FCX_T_TO_V };

enum fcx_status {
  FCX_OK = 0, FCX_E_ARG = 1, FCX_E_STATE = 2, FCX_E_UNSUPPORTED = 3, FCX_E_HIP = 4,
  FCX_E_MISSING = 5, FCX_E_NOMEM = 6,
  FCX_E_NONFINITE = 7 /* FCX_OPT_CHECK_FINITE found a NaN or an Inf (fcx_check_result) */
};

/* fcx_bind_field flags */
#define FCX_MEM_HOST   0x0 /* ptr is a host array owned by the caller (Fortran)       */
#define FCX_MEM_DEVICE 0x1 /* ptr is device memory owned by the caller (zero copy)     */
#define FCX_ALLOCATED  0x2 /* realarray%allocated (basic:88): an own array, not alias */

/* fcx_set_corrections layouts */
#define FCX_CORR_CELL_MAJOR  0 /* Fortran corrections(1,12,grid_size(1)) (bias:29-30,191) */
#define FCX_CORR_MONTH_MAJOR 1 /* [12][grid_size(1)] (the device layout)                 */

typedef struct fcx_engine fcx_engine;

const char *fcx_last_error(void);
int fcx_version(void);

/* The host's abort routine for errors that must end the coupled run, not just this rank:
 * the reference turns them into oasis_abort(comp_id, comp_name, msg)
 * (flux_calculator.F90:883-887, 930-934, 960-964).  The Fortran drop-in module calls
 * fcx_abort(message) on a failed call or a contract violation before its own ERROR STOP, so
 * a host that registers a routine calling oasis_abort (or MPI_Abort) takes the other
 * components down with it instead of leaving them waiting in their next exchange.
 * Process-wide; NULL unregisters.  fcx_abort returns FCX_E_STATE when none is registered,
 * FCX_OK when the handler returned. */
typedef void (*fcx_abort_handler)(const char *message);
int fcx_set_abort_handler(fcx_abort_handler handler);
int fcx_abort(const char *message);

/* trim(method)=='CCLM' etc. on a blank-padded Fortran CHARACTER(len=20); -1 if unknown */
int fcx_method_from_string(const char *s, size_t len);

/* datetime_helpers.get_current_date (pyfort/datetime_helpers.py:4-13): calendar month of
 * init_date (YYYYMMDD) + seconds.  Replaces the Fortran->C->CPython round trip of
 * calc:66-73. */
int fcx_current_month(int32_t init_date, int64_t seconds, int32_t *month);

/* ---- engine set-up (after flux_calculator.F90:761, when allocations are final) ---- */
int fcx_create(int device, int num_surface_types, const int32_t grid_size[3], fcx_engine **out);
int fcx_destroy(fcx_engine *e);
/* hipStream_t to run on (default: a stream owned by the engine) */
int fcx_set_stream(fcx_engine *e, void *hip_stream);
/* methods(my_bottom_model, surface_type) of one which_* table */
int fcx_set_method(fcx_engine *e, int flux, int surface_type, int method);
/* local_field(surface_type, grid)%var(var)%field => ptr(1:n).  Identical pointers in
 * several slots are aliases (basic:334-358, prepare:36-38) and share one device buffer.
 * n >= grid_size(grid) (FCX_E_ARG otherwise).  An array may be longer than its grid: cells
 * past the slot's grid size -- for a pointer bound on several grids, past the largest of them
 * -- are never read and never written, by a kernel or by a transfer, whatever the memory
 * (device arrays in place, caller heap arrays, fcx_host_malloc arrays as spans or in place). */
int fcx_bind_field(fcx_engine *e, int surface_type, int grid, int var, double *ptr, int64_t n,
                   int flags);
/* A namelist-constant input field (val_bottom_var_* / val_atmos_var_*, flux_calculator.F90:
 * 444-549: filled once by init_localvar, never received, never written): the slot holds
 * `value` in every cell.  Call before fcx_commit.  An unbound slot becomes bound, with no
 * caller array at all; a slot bound to an array turns constant together with EVERY slot bound
 * to the same address (the aliases of distribute_input_field, basic:334-358), and from then on
 * the engine neither reads nor writes that array: it is not uploaded, staged, mapped or given
 * a span.  Where only the flux pass reads the field, the fp64 generic and CCLM kernels without
 * register averages take it as a wave-uniform value out of the parameter block: no device
 * array, no vector load, and fcx_algorithmic_bytes does not count it.  Every other reader --
 * the fp32, MOM5, RCO and register-average kernels (no registers to spare for it, or a slower
 * step with it), a regridding, an average's FARE or field, the atmosphere
 * accumulation, a remap, fcx_device_ptr -- reads a device array of the engine's own, filled
 * once (in an fp32 engine with the value rounded to float once, as a bound float array holds
 * it).  Either way a constant costs no host-link traffic and no place in the staging arena,
 * and results are those of a bound array holding `value`, bit for bit.  fcx_upload_field of a
 * constant slot is a no-op.  `value` must be finite (FCX_E_ARG).  A constant slot that some plan would write --
 * a computed flux, a 'copy' target, a regrid destination, an average's type-0 output, RSDR --
 * is a named FCX_E_STATE error of fcx_plan_check / fcx_commit. */
int fcx_bind_constant(fcx_engine *e, int surface_type, int grid, int var, double value);
/* after fcx_commit: *kind = 0 the slot is not a constant; 1 a constant no device array has
 * been filled for (so far only launches that take it as a wave-uniform value read it); 2 a
 * constant in a device array the engine filled itself, at commit for a reader outside the flux
 * pass, later when the first launch that streams it is planned or fcx_device_ptr asks for it */
int fcx_constant_info(const fcx_engine *e, int surface_type, int grid, int var, int32_t *kind);
/* ---- receive side: model-grid inputs gathered to the exchange grid ----
 * What OASIS3-MCT does inside oasis_get of a received field (remap files
 * mappings/remap_<grid>_<model>_to_exchangegrid.nc): the host receives the field on the MODEL's
 * grid and the engine expands it on the device, so the 4-9 copies an intersection grid holds of
 * every atmosphere value never cross the host link.
 *
 * fcx_add_receive_map: a model grid -> exchange grid map: out[d] = sum over the links k with
 * dst[k] == d, in link order from 0.0, of w[k] * src_field[src[k]]; an exchange cell without a
 * link gets 0.0.  src: 0-based cell of the model-grid array on this rank (n_src cells), dst:
 * 0-based exchange cell of `grid`.  Before fcx_commit only.  Checked on the host, so that no
 * kernel ever indexes outside an array: n_src >= 1, every src in [0, n_src), every dst in
 * [0, grid_size(grid)), every weight finite; a violation is FCX_E_ARG naming the link.  The link
 * arrays are copied.  At fcx_commit every map in use is classified once: the injection form
 * where no exchange cell has two links (one source index per exchange cell, a weight per cell
 * only when some weight is not exactly 1.0), else the general form (CSR by exchange cell in
 * stable link order).
 *
 * fcx_bind_received: slot (surface_type, grid, var) is received through map `map_id` into `src`
 * before `phase` -- FCX_PHASE_EARLY or FCX_PHASE_NORMAL (FCX_PHASE_ALL is FCX_E_ARG).  Before
 * fcx_commit only.  src holds at least n_src elements (n >= n_src; double in an fp64 engine, float
 * in an fp32 engine); flags is FCX_MEM_HOST (heap or fcx_host_malloc memory) or FCX_MEM_DEVICE.
 * The declaration belongs to the buffer, as a constant's does: a slot bound to an exchange-grid
 * array turns received together with EVERY slot bound to that address (the aliases of
 * distribute_input_field, so one declaration of an atmosphere field covers every surface type),
 * and from then on that exchange-grid array is neither read nor written: it is not uploaded,
 * staged, mapped or given a span.  An unbound slot becomes bound.  The exchange-grid values live
 * in a device array of the engine's own, in the pool of arrays the whole-step launch reads (next
 * to the filled constants, tile-blocked where the layout applies); fcx_device_ptr returns it.
 * Cells of it past the grid size are never written.  The source array is an ordinary input
 * mirror of n_src elements that every transport takes: the staging arena for heap arrays; direct
 * DMA, a span or in-place use for fcx_host_malloc arrays; nothing for FCX_MEM_DEVICE; the upload
 * thread for fcx_upload_field (of a received slot: it hands over the source).  One source array
 * may serve several declarations of maps with the same n_src.
 * Named FCX_E_STATE errors of fcx_plan_check / fcx_commit: the buffer is also a constant; some
 * plan writes it (a computed flux, a 'copy' target, a regrid destination, an average's type-0
 * output, RSDR); the map's grid differs from the declared slot's grid (an alias of the buffer on
 * another grid must have the map's grid size: the u / v grids that ARE the t grid); two
 * declarations of one buffer disagree (map, phase or source).
 * When values move: fcx_upload(phase), and the upload half of fcx_step / fcx_step_async, move the
 * phase's host sources; fcx_run(phase) begins with the phase's gather launches, before any
 * regridding or flux pass (fcx_run_group: per member, before the merged launch; membership does
 * not change); a host-bound step cut into pipeline chunks uploads whole sources and gathers the
 * whole grid before its first chunk.  fcx_receive(phase) is upload plus gather alone, for hosts
 * of the per-call face: fcx_calc_* and fcx_do_regridding read the device array as last gathered
 * and never gather themselves.
 * Gather launches: all received fields of one (map, phase) in one launch, at most 16 per launch.
 * Arithmetic: fp64 engine: products and sum in double, in link order from 0.0, no contraction
 * (a one-link cell of weight 1.0 yields 0.0 + x, so -0.0 becomes +0.0); fp32 engine:
 * w * (double)x32 summed in double and rounded to float once, the rule of the remaps.
 * fcx_algorithmic_bytes(phase) adds, per gather launch, the map (injection: 4 B per exchange
 * cell, + 8 B with weights; general: 4 (grid_size + 1) + 12 n_links), n_src elements read and
 * grid_size elements written per field, and drops nothing else; fcx_staging_bytes,
 * fcx_zero_copy_bytes and fcx_span_runs count the sources instead of the exchange-grid arrays. */
int fcx_add_receive_map(fcx_engine *e, int grid, int64_t n_src, int64_t n_links,
                        const int32_t *src_cell, const int32_t *dst_cell, const double *weight,
                        int32_t *map_id);
int fcx_bind_received(fcx_engine *e, int32_t map_id, int phase, int surface_type, int grid,
                      int var, double *src, int64_t n, int flags);
int fcx_receive(fcx_engine *e, int phase);
/* after fcx_commit: *kind = 0 the slot is not received (*map_id = -1); 1 it is gathered into a
 * device array by a gather launch of map *map_id.  (Further kinds are reserved: a gather inside
 * the flux pass.) */
int fcx_received_info(const fcx_engine *e, int surface_type, int grid, int var,
                      int32_t *kind, int32_t *map_id);
/* What the host does with a computed output (a flux of surface types 1..T, a type-0 average, a
 * regrid destination).  The reference host sends only the fields its send_to_* / name_send_* tables
 * select (output_field, flux_calculator.F90:668-768, basic:170-284); an output it never sends
 * need not cross the host link, and one nobody reads at all need not be stored.  Call before
 * fcx_commit.  The declaration belongs to the buffer, as a constant's does: it covers EVERY slot
 * bound to the same address ('copy' aliases, uniform type-0 aliases, a T = 1 type-0 slot pointing at
 * type 1); where slots of one address are declared differently, FCX_OUT_DEVICE wins.
 *   FCX_OUT_HOST (default): the output is downloaded into the caller's array, as ever.
 *   FCX_OUT_DEVICE: the kernels store it into a device array of the engine's own -- valid after
 *     every run, readable through fcx_device_ptr and by every later engine call -- and it never
 *     crosses the host link.  From fcx_commit on the caller's array is neither written nor read:
 *     it is not staged, mapped, given a span or used in place (under zero-copy the buffer is an
 *     engine device array, not the host array), it has no place in the staging arena, and
 *     fcx_upload_field of the slot is a no-op; fcx_staging_bytes, fcx_zero_copy_bytes and
 *     fcx_span_runs count the smaller set.  (A slot bound as FCX_MEM_DEVICE keeps the caller's
 *     device array: it crosses no link as it is.)
 *   FCX_OUT_UNREAD: FCX_OUT_DEVICE, plus permission not to store it at all.  A whole-phase launch
 *     (fcx_run / fcx_step / fcx_run_group of a phase, per pipelined chunk too) whose own registers
 *     are the output's only consumer gets a null store pointer for it; the flux is still computed
 *     wherever a later flux of the launch needs it (QSUR -> MEVA / momentum, MEVA -> HLAT, a
 *     register average, the fused accumulation).  The buffer stays FCX_OUT_DEVICE for good when
 *     anything outside such a launch reads the array: any regridding of the engine, an average
 *     that re-reads its fields, the separate accumulation kernel or the crossing-record fix-up
 *     (a fused launch without halo tiles on a map with crossings keeps its accumulated fields;
 *     so does every launch of an engine whose host arrays fcx_step could cut into pipeline
 *     chunks -- set FCX_OPT_PIPELINE_CHUNKS to 1 where the engine only runs whole grids),
 *     a remap, a 'copy' consumer, a whole-phase launch that reads it without producing it; so
 *     does a type-0 average.  The per-call subroutines (fcx_calc_*) always store.  A skipped
 *     store leaves the device array STALE until a launch stores it again: a call that would read
 *     a stale buffer -- a per-call subroutine, fcx_run_atmos, fcx_device_ptr -- returns
 *     FCX_E_STATE naming the slot before anything is launched.  The array keeps its reserved
 *     slot in the device pool, as a constant's does.  fcx_algorithmic_bytes drops the skipped
 *     stores' bytes and nothing else.
 * Results in every output the host still reads are those of an engine without declarations, bit
 * for bit.  A declared slot that is unbound, is a constant, or that no plan writes is a named
 * FCX_E_STATE error of fcx_plan_check / fcx_commit.  Atmosphere outputs (fcx_add_atmos_field) and
 * remap outputs are always wanted. */
enum fcx_output_use { FCX_OUT_HOST = 0, FCX_OUT_DEVICE = 1, FCX_OUT_UNREAD = 2 };
int fcx_set_output_use(fcx_engine *e, int surface_type, int grid, int var, int use);
/* after fcx_commit: *kind = 0 the host reads the slot's output; 1 it is kept in a device array;
 * 2 the last whole-phase plan built for it left its store out */
int fcx_output_info(const fcx_engine *e, int surface_type, int grid, int var, int32_t *kind);
/* bias_corrections: lcorrections(E_MASS_EVAP_CORRECTION), init_date, corrections(1,:,:) */
int fcx_set_corrections(fcx_engine *e, int enabled, int32_t init_date, const double *corr,
                        int64_t n, int layout);
/* sparse_regridding_matrix (basic:117-122): 1-based, rank-local, offset-corrected links */
int fcx_set_regrid_matrix(fcx_engine *e, int which, int64_t num_elements, const int32_t *src_index,
                          const int32_t *dst_index, const double *weight);
/* realarray%put_to_{t,u,v}_grid of (surface_type, grid, var): bit0 t, bit1 u, bit2 v.  A
 * regridding reads one array and writes another: a destination slot bound to the source's own
 * array (u / v grids that ARE the t grid) is a named FCX_E_STATE error of fcx_plan_check /
 * fcx_commit -- the launch would read the cells it is overwriting. */
int fcx_set_put_to(fcx_engine *e, int surface_type, int grid, int var, int mask);
/* register a type-0 output that is averaged before its oasis_put (flux_calculator.F90:
 * 911-918 early, 1001-1008 normal).  Follows the P7 trigger: only applied when the type-0
 * array is FCX_ALLOCATED and surface type 2 exists. */
int fcx_add_average(fcx_engine *e, int phase, int grid, int var);
/* arithmetic/storage type of the engine's fields.  FCX_PRECISION_F64 (default) is the
 * reference's -r8 build (build_hlrnb.sh:26).  FCX_PRECISION_F32: every pointer given to
 * fcx_bind_field / fcx_add_atmos_field / returned by fcx_device_ptr addresses float arrays
 * (the double* parameter type then only carries the address) and the kernels compute in
 * fp32 -- the SURVEY.md 8d config-5 variant, half the HBM bytes per cell.  Corrections are
 * still passed as double and rounded once at commit.  do_regridding runs in fp32 with the
 * matrix weights rounded once (the single-precision build's REAL(wp) arithmetic,
 * basic:117-122, 463-522).  The atmosphere accumulation and the remaps read the fp32 fields
 * and write fp32 outputs (fcx_add_atmos_field / fcx_add_remap_field then take float arrays)
 * but weigh and sum in fp64, as OASIS maps in double; the shared boundary buffer of
 * fcx_set_atmos_shared stays double.  Call before fcx_commit. */
enum fcx_precision { FCX_PRECISION_F64 = 0, FCX_PRECISION_F32 = 1 };
int fcx_set_precision(fcx_engine *e, int precision);
/* validate (flux_calculator_prepare.F90 rules), allocate device mirrors, build plans */
int fcx_commit(fcx_engine *e);
/* before fcx_commit, host only (no GPU): validate, then build every launch plan the engine can
 * take -- the whole phases, the per-call subroutines, the regridding sequence, the explicit
 * averages -- and audit each against the kernels' load predicates: a computed flux whose input
 * the planner did not bind is a named FCX_E_STATE error (the same audit runs on every plan
 * fcx_commit and the later calls build, before its first launch) */
int fcx_plan_check(fcx_engine *e);

/* ---- per coupling step: fused path ---- */
int fcx_upload(fcx_engine *e, int phase);   /* H2D of host-bound inputs of the phase  */
int fcx_run(fcx_engine *e, int phase, int32_t current_step_time); /* device compute  */
int fcx_download(fcx_engine *e, int phase); /* D2H of host-bound outputs of the phase */
/* fcx_run of several engines on one device (e.g. one per bottom-model variant), in the order
 * given: the flux passes of those whose phase is one fused launch of the same shape: one
 * surface type, or several with the type-0 averages in registers, in any precision (engines of
 * one precision and arithmetic merge with each other, single-type ones with single-type ones)
 * on the same stream go out as ONE launch (at most 4 engines; the others run as fcx_run), so a
 * step pays the launch ramp and drain once.  Results are those of fcx_run of each, bit for
 * bit. */
int fcx_run_group(fcx_engine *const *engines, int n_engines, int phase, int32_t current_step_time);
/* engines in the merged launch of the engine's last fcx_run_group (0: it ran as fcx_run).
 * Every engine's work after its launch (fix-up, accumulation, the boundary exchange of an
 * attached communicator, remaps) runs in LIST order whichever engines were merged, so the
 * per-engine collectives of fcx_set_comm keep the same order on every rank. */
int fcx_last_group_size(fcx_engine *e, int32_t *members);
/* after fcx_commit: 1 when the engine keeps its atmosphere outputs as per-cell records
 * (FCX_OPT_ATM_RECORDS), 0 when as plain arrays */
int fcx_atm_records(const fcx_engine *e, int32_t *on);
/* 1 when the engine is an fp32 engine whose fluxes are computed in double (FCX_OPT_F32_MATH, by
 * the option or the environment's default), 0 otherwise; before fcx_commit: what it would apply */
int fcx_f32_math(const fcx_engine *e, int32_t *on);
/* 1 when the engine is a committed fp64 engine that runs the correctly rounded kernels
 * (FCX_OPT_CR_MATH, by the option or the environment's default); 0 before fcx_commit, on an
 * fp32 engine and with the option off */
int fcx_cr_math(const fcx_engine *e, int32_t *on);
/* after fcx_commit: 1 when the phase's exchange -> atmosphere accumulation rides inside the flux
 * launch (no second pass over the fields), 0 when atmos_kernel runs it; FCX_E_STATE before commit,
 * FCX_E_ARG for a phase outside 1..3 or a NULL pointer.  It may build the phase's plan (as the
 * first fcx_run of the phase would) and changes nothing else */
int fcx_fused_accumulation(fcx_engine *e, int phase, int32_t *on);
/* the three above; with host-bound fields pipelined over cell chunks (FCX_OPT_PIPELINE_CHUNKS) */
int fcx_step(fcx_engine *e, int phase, int32_t current_step_time);
/* waits for the engine's stream; the caller's host arrays hold the downloaded outputs once it
 * returns.  fcx_download fills caller heap arrays itself (it waits for the stream); with
 * FCX_OPT_DEFERRED_SCATTER they are filled from the staging arena here.  fcx_step and the
 * per-call subroutines end with it. */
int fcx_synchronize(fcx_engine *e);
/* fcx_step without its final wait (the asynchronous phase): when it returns the engine holds
 * the inputs (caller heap arrays are copied into the staging arena inside the call, so the
 * host may overwrite them), the launch and the output DMAs are queued, and the caller's
 * output arrays are filled by the next fcx_synchronize.  Inputs in fcx_host_malloc memory
 * are read in place until then.  A host starts several engines this way from one thread (each
 * on its own stream), or overlaps its own work -- another component's exchange -- with the
 * step.  Host-bound grids of at least two pipeline chunks complete inside the call. */
int fcx_step_async(fcx_engine *e, int phase, int32_t current_step_time);
/* One input field handed over as the host receives it (oasis_get of field j, then
 * fcx_upload_field): its host array is copied into the staging arena and DMAed to its
 * mirror by the engine's upload thread while the host goes on to receive the next field
 * (flux_calculator.F90:872-897, 938-966: the reference gets the fields one by one).  The
 * upload thread copies the array at some point before the next engine call (any but
 * fcx_upload_field) returns, so the array must not change until that call returns; from
 * then on the host may overwrite it -- every call first waits for the handed-over fields.
 * fcx_upload / fcx_step / fcx_step_async then move only the phase's remaining inputs.
 * Aliases (one array in several slots) are handed over once.  If a hand-over fails, the
 * next call returns its error and no field counts as handed over, so a retried step moves
 * every input again. */
int fcx_upload_field(fcx_engine *e, int surface_type, int grid, int var);

/* ---- per call: the reference subroutines one by one (exact drop-in semantics; each
 * call uploads what it reads, computes, downloads what it writes, and synchronises) ---- */
int fcx_calc_spec_vapor_surface(fcx_engine *e, int which_grid);            /* calc:25  */
int fcx_calc_flux_mass_evap(fcx_engine *e, int32_t current_step_time);     /* calc:54  */
int fcx_calc_flux_heat_latent(fcx_engine *e);                              /* calc:124 */
int fcx_calc_flux_heat_sensible(fcx_engine *e);                            /* calc:156 */
int fcx_calc_flux_momentum_east(fcx_engine *e, int which_grid);            /* calc:212 */
int fcx_calc_flux_momentum_north(fcx_engine *e, int which_grid);           /* calc:265 */
int fcx_calc_flux_radiation_blackbody(fcx_engine *e);                      /* calc:320 */
int fcx_distribute_shortwave_radiation_flux(fcx_engine *e);                /* calc:347 */
int fcx_average_across_surface_types(fcx_engine *e, int which_grid, int var); /* calc:368 */
int fcx_do_regridding(fcx_engine *e, int var, int surface_type);           /* basic:463 */

/* ---- device-resident use and measurement ---- */
/* device buffer behind a slot (NULL if unbound).  Cell j of it sits at element
 * (j / tile) * tile_stride + j % tile (fcx_device_layout); tile_stride == tile means the
 * buffer is one contiguous array. */
int fcx_device_ptr(fcx_engine *e, int surface_type, int grid, int var, double **dptr);
/* layout of the engine-owned field mirrors (after fcx_commit): cells in tiles of `tile`
 * elements, consecutive tiles of one array `tile_stride` elements apart (FCX_OPT_TILED_LAYOUT) */
int fcx_device_layout(fcx_engine *e, int64_t *tile, int64_t *tile_stride);
/* device time (hipEvents on the engine stream) of the kernels of the last fcx_run;
   needs FCX_OPT_TIMING = 1 */
int fcx_last_kernel_ms(fcx_engine *e, float *ms);
/* bytes of the engine's page-locked staging arena for caller heap arrays (0: none): one host
 * image per device pool that holds a heap array's mirror, allocated at fcx_commit (the
 * pinned footprint: ~the mirrors' size, e.g. 2.2-2.6 GB per 10M-cell CCLM engine).  A pool
 * whose image cannot be page-locked takes the direct path instead and is not counted. */
int fcx_staging_bytes(fcx_engine *e, int64_t *bytes);
/* retired in version 3, kept for one release: always 0 (nothing of the caller's memory is
 * page-locked; the in-launch carry hand-off is gone) */
int fcx_pinned_bytes(fcx_engine *e, int64_t *bytes);
int fcx_handoff_recoveries(fcx_engine *e, int64_t *count);
/* bytes of host arrays the kernels use in place (FCX_OPT_ZERO_COPY) */
int fcx_zero_copy_bytes(fcx_engine *e, int64_t *bytes);
/* copies one fcx_step(phase) makes of the engine's fcx_host_malloc arrays with the span
 * transport (FCX_OPT_LIB_SPANS): uploads, downloads (0 / 0 when no array takes it) */
int fcx_span_runs(fcx_engine *e, int phase, int32_t *h2d_copies, int32_t *d2h_copies);
/* algorithmic HBM bytes of one fcx_run(phase) (each distinct array read once, written once) */
int fcx_algorithmic_bytes(fcx_engine *e, int phase, int64_t *bytes);

/* ---- field ranges and the non-finite guard ----
 * At verbosity_level DEBUG the reference host logs MINVAL and MAXVAL of every field it receives
 * and sends (flux_calculator.F90:879-881, 921-924, 949-951, 1011-1013).  Here most of those fields
 * never reach host memory (constants, outputs kept on the device, received fields, atmosphere
 * records, device-resident hosts), so the reduction runs on the device: one streaming launch over
 * at most 16 fields plus a one-wave-per-field finishing launch, on the engine's stream.
 *   min, max:  over the cells that are not NaN; +-Inf takes part; both NaN when every cell is NaN
 *              or the grid is empty.  Exact, independent of order; -0.0 and +0.0 compare equal and
 *              either may be returned.  A float field's values are widened to double.
 *   n_nan, n_inf: cells holding a NaN / an Inf of either sign.
 *   first_bad: the lowest cell holding a NaN or an Inf, -1 when there is none.
 * Cells at or past the slot's grid size never enter a result. */
typedef struct fcx_field_range {
  double min, max;
  int64_t n_nan, n_inf, first_bad;
} fcx_field_range;
/* The ranges of n slots, slots[3 k .. 3 k + 2] = (surface_type, grid, var), into out[k], in request
 * order (any n; launches of at most 16 fields).  After fcx_commit (FCX_E_STATE before).  It waits
 * for the engine's stream; the results travel through a small page-locked buffer of the engine's
 * own, 40 B per field.  A slot is read where fcx_device_ptr of it would point after a step: the
 * engine's mirror (contiguous or tile-blocked), the caller's device array, the host array used in
 * place under zero-copy (read through the link, as the flux kernel reads it), an engine-filled
 * constant, a received field's exchange-grid array, an FCX_OUT_DEVICE array.  A constant no device
 * array was filled for (fcx_constant_info 1) is answered from its value, without a launch and
 * without filling one: min = max = the value as the kernels see it (rounded to float in an fp32
 * engine).  A slot whose store was skipped (FCX_OUT_UNREAD, stale) is the named FCX_E_STATE error
 * of fcx_device_ptr, before any launch; an unbound slot is FCX_E_ARG naming it. */
int fcx_field_ranges(fcx_engine *e, int32_t n, const int32_t *slots, fcx_field_range *out);
/* The ranges of the atmosphere outputs of `phase`, in fcx_add_atmos_field order, over the n_atmos
 * local cells; *n_fields = their number (more than cap: FCX_E_ARG).  Read from the device arrays
 * or per-cell records as they are: no unpack launch, no download pool.  With several ranks the
 * values are this rank's, complete after fcx_atmos_finish (flux_calculator.F90:1011-1013). */
int fcx_atmos_ranges(fcx_engine *e, int phase, int32_t cap, fcx_field_range *out, int32_t *n_fields);
/* What FCX_OPT_CHECK_FINITE checks after a whole-phase run of `phase`, with the option's current
 * value: slots[3 k .. 3 k + 2], first the inputs (bit 1), then the outputs (bit 0), each in slot
 * order (surface type, grid, variable; a buffer under its first slot); *n = their number (more
 * than cap: FCX_E_ARG, *n set).  The phase's atmosphere outputs are checked too and are not
 * listed.  Host only: answered after fcx_plan_check or fcx_commit (FCX_E_STATE before either);
 * before fcx_commit the answer is that of the plan without a fused accumulation. */
int fcx_check_fields(fcx_engine *e, int phase, int32_t cap, int32_t *slots, int32_t *n);
/* The last FCX_E_NONFINITE of the engine as numbers: *is_atmos 1 for an atmosphere output (then
 * the slot is the accumulated field's), the slot, the cell (first_bad) and the value stored
 * there.  *cell = -1 when the last checked run was clean or none has run.  NULL pointers are
 * skipped. */
int fcx_check_result(const fcx_engine *e, int32_t *is_atmos, int32_t *surface_type, int32_t *grid,
                     int32_t *var, int64_t *cell, double *value);

/* ---- exact (area-weighted) field integrals: flux budgets ----
 * How much heat, water or momentum crossed the surface in a step is sum_j A_j F_j over a grid, and
 * a step is conservative when that sum over the exchange grid equals the one over the atmosphere
 * grid.  Most fields never reach host memory, so the sum runs on the device; and because a budget
 * is a cancelling sum that must not depend on block counts, tile order or the number of ranks, it
 * is EXACT: a fixed-point long accumulator whose partial results add associatively, rounded once
 * when a double is asked for.  The same bits for 1 rank or 8, for tile-blocked or contiguous
 * mirrors, for any grid.
 *
 * The terms of field x over the cells j < n (n: the slot's grid size), fp64 arithmetic, no FMA:
 *   unweighted  t_j = x_j;   weighted  t_j = fl(a_j * x_j), one IEEE double multiply.
 * An fp32 engine's x_j is widened to double first (exactly); areas are always fp64.  The integral
 * is sum_j t_j without any rounding.  A non-finite term (a NaN, +-Inf, a product that overflowed)
 * never enters the limbs; it is counted.  Zeros of either sign contribute nothing; an empty or
 * fully cancelling sum has the value +0.0.
 *
 *   value = sum_k limb[k] * 2^(32 k - 1088).  A finite double +-m * 2^q (m < 2^53, q >= -1074) lands
 *   at bit p = q + 1088, in limbs p >> 5 .. (p >> 5) + 2, as the three 32-bit digits of
 *   m << (p & 31).  Limbs 0..66 cover every double (DBL_MAX: limbs 64, 65; the smallest denormal:
 *   limb[0] = 16384), limb 67 is carry headroom.
 *   n_terms: the finite terms (zeros included); n_nan, n_pinf, n_ninf: the terms left out.  The
 *   four counts add up to the cells summed.
 * CANONICAL FORM -- what every entry point returns: limbs 0..66 in [0, 2^32), limb 67 signed (a
 * negative value is the two's complement over the 68 limbs).  Every value has exactly one
 * representation: two sums are equal iff their 576 bytes are.  Canonical sums of up to 2^30 ranks
 * may be added limb by limb and count by count -- MPI_SUM on INTEGER(8), 72 of them -- and
 * fcx_sum_merge(into, raw) of the result, once, gives the global sum.  No limb reaches 2^62 in
 * magnitude at any point, on the device or the host (csrc/fcx_exactsum.h says where carries are
 * propagated). */
#define FCX_SUM_LIMBS 68
typedef struct fcx_exact_sum {          /* 576 B */
  int64_t limb[FCX_SUM_LIMBS];          /* value = sum_k limb[k] * 2^(32 k - 1088) */
  int64_t n_terms, n_nan, n_pinf, n_ninf;
} fcx_exact_sum;
/* Host arithmetic (no GPU, no engine; the device kernels compile the same code).
 * fcx_sum_clear: the empty sum.  fcx_sum_add_terms / _f32: the CPU twin of the kernel -- the terms
 * of x[0..n) (a NULL: unweighted) added to *s, which is left canonical.  fcx_sum_merge: limbs and
 * counts of `other` added to `into`, then normalised; `other` may be a raw limb-wise sum of up to
 * 2^30 canonical sums, and other == NULL only normalises `into`.  fcx_sum_value: the sum rounded
 * once, to nearest even; NaN when n_nan > 0 or both infinity counts are non-zero, +-Inf when one
 * is, +-Inf when the exact value rounds beyond DBL_MAX (the limbs stay exact: a later merge can
 * bring the value back). */
int fcx_sum_clear(fcx_exact_sum *s);
int fcx_sum_add_terms(fcx_exact_sum *s, const double *x, const double *a, int64_t n);
int fcx_sum_add_terms_f32(fcx_exact_sum *s, const float *x, const double *a, int64_t n);
int fcx_sum_merge(fcx_exact_sum *into, const fcx_exact_sum *other);
int fcx_sum_value(const fcx_exact_sum *s, double *value);
/* The cell areas of exchange grid `grid` (1..3: t, u, v), a host array of n >= grid_size doubles --
 * the areas the reference hands to OASIS (flux_calculator.F90:791-793, oasis_write_area).  The
 * engine keeps a contiguous device copy of the first grid_size values (never tile-blocked),
 * uploaded once: the step's transports never see it and fcx_algorithmic_bytes does not count it.
 * Before or after fcx_commit, and again to replace the array.  A non-finite area is FCX_E_ARG
 * naming the cell; negative and zero areas are allowed. */
int fcx_set_areas(fcx_engine *e, int grid, const double *area, int64_t n);
/* ... and of the n_atmos local atmosphere cells (after fcx_set_atmos_map).  A rank passes 0.0 for
 * an atmosphere cell it shares with a neighbour but does not own, so that a shared cell counts
 * once across the ranks (fcx.parallel.owned_atmos_mask gives the rule: the lower rank owns). */
int fcx_set_atmos_areas(fcx_engine *e, const double *area, int64_t n_atmos);
/* The integrals of n slots, as fcx_field_ranges reads them (the same slot triples, argument checks,
 * FCX_E_STATE before fcx_commit, stale FCX_OUT_UNREAD error; a slot is read where fcx_device_ptr
 * points after a step), into out[k], canonical.  weighted 1: by the areas of the slot's grid
 * (FCX_E_STATE naming the grid when none were set); 0: plain sums.  A wave-uniform constant has no
 * array and gets none: the launch carries its value, and the result is that of an array holding
 * it.  One streaming launch per 16 fields plus a one-block-per-field finishing launch, on the
 * engine's stream, which the call waits for; the results travel through a page-locked buffer of
 * the engine's own, 576 B per field. */
int fcx_field_integrals(fcx_engine *e, int32_t n, const int32_t *slots, int weighted, fcx_exact_sum *out);
/* ... of the atmosphere outputs of `phase`, as fcx_atmos_ranges reads them (pool slot, plain array
 * or record column; no unpack launch), weighted by fcx_set_atmos_areas. */
int fcx_atmos_integrals(fcx_engine *e, int phase, int weighted, int32_t cap, fcx_exact_sum *out,
                        int32_t *n_fields);

/* ---- exchange-grid -> atmosphere accumulation ----
 * What OASIS3-MCT does on oasis_put of the type-0 fields ('S A xxxx 00',
 * create_namcouple.F90:92-98): out[a] = sum_x weight[x] * field[x] over the local t-grid
 * exchange cells x of atmosphere cell a, summed in increasing x.  Ranks own contiguous
 * exchange ranges, so only the first and last local atmosphere cells can be shared with a
 * neighbour rank; their partial sums go to `shared` slots that ONE all-reduce (sum) over
 * all ranks completes, after which fcx_atmos_finish writes them back. */
/* atmos_index[x]: 0-based local atmosphere cell of exchange cell x (grid_size(1) entries) */
int fcx_set_atmos_map(fcx_engine *e, int64_t n_atmos, const int32_t *atmos_index,
                      const double *weight);
/* accumulate slot (surface_type, grid, var) into out[n_atmos] at the end of `phase` */
int fcx_add_atmos_field(fcx_engine *e, int phase, int surface_type, int grid, int var,
                        double *out, int flags);
/* shared: device buffer [n_boundaries][stride] (zero on entry, re-zeroed by finish); the
 * rank's first local atmosphere cell is boundary `left` (-1: not shared), its last one
 * boundary `right`; field f of the accumulation uses column f (f < stride).  Boundary m - 1
 * is the one just before rank m's cells: left = rank - 1, right = (next rank with cells) - 1
 * (a rank with an empty task, io:101-104, sits between two slots' owners without one).
 * Every rank that holds part of one atmosphere cell uses ONE slot for it, the slot of the
 * first rank boundary inside the cell: a rank whose cells all lie in one atmosphere cell
 * shared with both neighbours has left == right (fcx.parallel.boundary_slots).  The slots
 * are written, never added to, so left == right is safe. */
int fcx_set_atmos_shared(fcx_engine *e, double *shared, int32_t n_boundaries, int32_t stride,
                         int32_t left, int32_t right);
/* instead of fcx_set_atmos_shared: the engine allocates the [n_boundaries][fields] slots
 * itself (device memory, zeroed; stride = number of fcx_add_atmos_field fields).  Before
 * fcx_commit. */
int fcx_set_atmos_boundaries(fcx_engine *e, int32_t n_boundaries, int32_t left, int32_t right);
/* FCX_OPT_ATMOS_INVARIANT: the term columns of the boundary slots.  Before fcx_commit.
 * max_terms (K): the largest number of exchange cells of any atmosphere cell shared between
 * ranks, the SAME number on every rank of the run (1 .. 4096).  left_pos: how many exchange
 * cells of this rank's FIRST local atmosphere cell lie on lower ranks (0 when left < 0).  The
 * last local atmosphere cell needs no number: where it is another cell than the first it
 * begins on this rank, at position 0; where it is the same cell (n_atmos == 1) its position is
 * left_pos.  (fcx.parallel.boundary_terms gives both numbers; INTEGRATION.md section 3 shows
 * the two MPI calls that do.)
 * Slot layout with the option on, per boundary: the columns f < fields of the partial sums stay
 * (the accumulation kernels still write them; nothing reads them), and fields x K term columns
 * follow: column fields + f * K + p holds fl(w[x] * field_f[x]) of the exchange cell x at link
 * position p of the shared atmosphere cell, written by the one rank that owns x and +0.0 on
 * every other rank, so the fp64 sum all-reduce delivers it exactly (x + 0 + ... + 0 = x; a
 * -0.0 term arrives as +0.0, which the sum from +0.0 does not notice).  fcx_atmos_finish adds
 * the K positions in order.  After fcx_run / fcx_run_atmos / fcx_run_group return, the region
 * holds the terms (stream-ordered).  fcx_set_atmos_boundaries allocates stride = fields x
 * (1 + K); fcx_set_atmos_shared needs a stride of at least that.  Named FCX_E_ARG errors of
 * fcx_plan_check and fcx_commit: left_pos + the rank's own cells of that atmosphere cell >
 * max_terms; a stride that is too small; an unsorted atmosphere map; max_terms outside 1..4096;
 * boundary slots without this call.  Ranks that disagree on K disagree on the stride, which the
 * signature agreement of the exchange reports on every rank. */
int fcx_set_atmos_terms(fcx_engine *e, int32_t max_terms, int32_t left_pos);
/* the doubles per boundary slot: the number of fcx_add_atmos_field fields, times 1 + max_terms
 * with FCX_OPT_ATMOS_INVARIANT on and fcx_set_atmos_terms called -- for a host that owns the
 * buffer of fcx_set_atmos_shared.  At any time; the answer follows the calls made so far. */
int fcx_atmos_columns(const fcx_engine *e, int32_t *columns);
/* the engines whose terms went out in ONE launch with this engine's after its last accumulation:
 * 1 a launch of its own (fcx_run, fcx_run_atmos, an engine that exchanges by itself), n the
 * launch shared by n engines of an fcx_run_group, 0 none (the option off, no shared cell) */
int fcx_last_terms_group(const fcx_engine *e, int32_t *engines);
/* 1 when FCX_OPT_ATMOS_INVARIANT is on */
int fcx_atmos_invariant(const fcx_engine *e, int32_t *on);
/* after the all-reduce of `shared`: boundary values -> out arrays, slots re-zeroed */
int fcx_atmos_finish(fcx_engine *e);
/* the accumulation of `phase` on its own (fcx_run runs it unless FCX_OPT_ATMOS_IN_RUN=0) */
int fcx_run_atmos(fcx_engine *e, int phase);

/* ---- the one collective: RCCL over xGMI ----
 * The boundary slots of all ranks are summed by ONE ncclAllReduce(sum, ncclFloat64) per
 * step, the exchange OASIS3-MCT performs on the oasis_put of the type-0 fields
 * (flux_calculator.F90:1015, create_namcouple.F90:92-98).  One communicator per rank (one
 * rank per GPU): rank 0 creates the unique id, the host broadcasts its
 * FCX_COMM_ID_BYTES bytes (MPI_Bcast in the Fortran host) and every rank creates its
 * communicator.  RCCL is loaded at run time (the process's own librccl.so if one is
 * already loaded, e.g. PyTorch's, else /opt/rocm's). */
#define FCX_COMM_ID_BYTES 128
typedef struct fcx_comm fcx_comm;
int fcx_comm_unique_id(void *id /* FCX_COMM_ID_BYTES */);
int fcx_comm_create(int device, int nranks, int rank, const void *id, fcx_comm **out);
int fcx_comm_destroy(fcx_comm *c);
/* sum-all-reduce of count doubles in place on a HIP stream (generic) */
int fcx_comm_allreduce_sum(fcx_comm *c, double *buf, size_t count, void *hip_stream);
/* attach: from now on fcx_run / fcx_step / fcx_run_atmos of the engine complete its
 * boundary slots themselves (all-reduce on the engine's stream, then fcx_atmos_finish);
 * every rank's engine must then run the same steps.  fcx_run_atmos after an fcx_run that
 * already exchanged issues no collective.  NULL detaches. */
int fcx_set_comm(fcx_engine *e, fcx_comm *c);
/* several engines of this rank (e.g. one per bottom-model variant) in ONE all-reduce of
 * sum(n_boundaries * stride) doubles over their slots in list order, on the first engine's
 * stream, then fcx_atmos_finish of each.  Regions that follow each other in list order in
 * one buffer are reduced in place, others through the communicator's scratch; the collective
 * is the same either way.  Call after their accumulation (fcx_run, or fcx_run_atmos).
 * Collective contract: every rank passes its engines in the same order with the same
 * n_boundaries and strides.  What is checked: by default, the FIRST exchange of each
 * signature a rank has not exchanged before on this communicator is preceded by a blocking
 * max-all-reduce of the signature, and ranks that disagree all return FCX_E_ARG -- this
 * catches a decomposition the ranks disagree on from the start, without a host wait per
 * step.  It cannot catch a rank that switches to a new engine list after exchanging while
 * another keeps an already agreed one (that rank skips the check, the collectives differ);
 * fcx_comm_verify(c, 1) runs the check before EVERY exchange (one 6-double all-reduce and a
 * host wait per exchange) for hosts that change their engine lists at run time.  An engine
 * already completed in this run (fcx_set_comm) takes part with zeros and is skipped; one
 * with no accumulation since its last exchange takes part with zeros and the call returns
 * FCX_E_STATE after the collective, so no rank is left waiting. */
int fcx_atmos_allreduce(fcx_comm *c, fcx_engine *const *engines, int n_engines);
/* 1: the signature agreement before every exchange of the communicator; 0 (default): before
 * the first exchange of each signature */
int fcx_comm_verify(fcx_comm *c, int every_exchange);

/* ---- exchange-grid -> model remaps ----
 * The SCRIP weight application OASIS3-MCT performs on the 'S' fields sent to a model
 * (remap files mappings/remap_<grid>_exchangegrid_to_<model>.nc): out[d] = sum over the
 * links k with dst[k] == d, in link order from 0.0, of w[k] * field[src[k]].  src: 0-based
 * cell of the field's grid on this rank; dst: 0-based cell of the target grid (n_dst cells,
 * e.g. the whole ocean grid).  With several ranks, every rank writes its partial sums of
 * all n_dst cells (0 where it has no link); an all-reduce (sum) of the output arrays over
 * the ranks completes them.  Run by fcx_run / fcx_step after the fluxes. */
int fcx_add_remap(fcx_engine *e, int64_t n_dst, int64_t n_links, const int32_t *src_cell,
                  const int32_t *dst_cell, const double *weight, int32_t *remap_id);
int fcx_add_remap_field(fcx_engine *e, int32_t remap_id, int phase, int surface_type, int grid,
                        int var, double *out, int flags);
/* after fcx_commit: the map's gather scatter (distinct 64-B field segments per link over a
 * sample of 256-destination blocks) and whether its launches gather packed records
 * (FCX_OPT_REMAP_PACK): 0 no, 1 packed by a packing pass, 2 the flux launch of the last
 * fcx_run / fcx_step wrote the records of one launch group of this remap (T=1 fluxes of
 * surface type 1; that group needs no packing pass -- a remap of more than 16 fields has
 * further groups, which pack their own).  Per-call runs do not change the answer. */
int fcx_remap_info(const fcx_engine *e, int32_t remap_id, double *scatter, int32_t *packed);

/* launch tuning of the fused cells kernel (defaults are the measured best on MI355X) */
enum fcx_option {
  FCX_OPT_CELLS_PER_THREAD = 1, /* 1 or 2 cells per lane (2: 16-B loads; default 2)       */
  FCX_OPT_MAX_BLOCKS = 2,       /* grid-stride cap in 256-thread blocks; 0 = no cap;
                                   -1 (default) = per kernel: 8192 for the flux pass, no
                                   cap for the T=1 pass with the fused accumulation       */
  FCX_OPT_NONTEMPORAL = 3,      /* non-temporal hint on streamed loads/stores (default 1) */
  FCX_OPT_SPECIALIZE = 4,       /* T=1 CCLM/MOM5/RCO specialised kernels (default 1)      */
  FCX_OPT_ATMOS_IN_RUN = 5,     /* fcx_run also runs the atmosphere accumulation (def. 1) */
  FCX_OPT_PIPELINE_CHUNKS = 7,  /* fcx_step of host-bound fields: H2D/compute/D2H overlap
                                   over this many cell chunks (default 8; 1 = sequential) */
  FCX_OPT_PIPELINE_MIN_CHUNK = 8, /* ... of at least this many cells (multiple of 1024;
                                   default 262144: smaller grids take the sequential step) */
  FCX_OPT_ZERO_COPY = 9,        /* fields used by the kernels in place through the host link:
                                   no mirrors, no copy calls (fcx_host_malloc arrays directly,
                                   caller heap arrays through the mapped staging arena).
                                   2 auto (default): when every grid is below
                                   2 x PIPELINE_MIN_CHUNK cells; 1: at any size; 0: never */
  FCX_OPT_LIB_SPANS = 19,       /* fcx_host_malloc arrays not used in place: device mirrors
                                   laid out like the host memory (one buffer per slab span), so
                                   arrays adjacent in host memory move as ONE copy per
                                   direction -- a host allocating its inputs, then its outputs,
                                   in the reference's order makes
                                   one or two uploads and one download per phase.  1 (default);
                                   0: one copy per array.  Applied at fcx_commit           */
  FCX_OPT_TIMING = 10,          /* record the events behind fcx_last_kernel_ms (default 0:
                                   two event records per run cost ~8 us on small grids) */
  FCX_OPT_HOST_STAGING = 15,    /* caller heap arrays (not fcx_host_malloc memory) reach
                                   their device mirrors through an engine-owned page-locked
                                   staging arena laid out like the mirrors: host threads copy
                                   the arrays into it, then ONE DMA per pool and direction
                                   (per chunk when pipelined), and back.  1 (default); 0:
                                   one runtime copy per array (pageable, staged by HIP).
                                   Nothing of the caller's memory is ever page-locked or
                                   mapped.  Applied at fcx_commit                          */
  FCX_OPT_HOST_THREADS = 16,    /* host threads of those copies (the calling thread
                                   included); 0 (default): min(16, OMP_NUM_THREADS if set,
                                   else the CPUs of the process affinity set -- divided by
                                   the node's local rank count when the rank is not pinned
                                   (OMPI_COMM_WORLD_LOCAL_SIZE, MPI_LOCALNRANKS,
                                   SLURM_NTASKS_PER_NODE or LOCAL_WORLD_SIZE)).  Under MPI,
                                   pin ranks or set this to each rank's core share        */
  FCX_OPT_DEFERRED_SCATTER = 18, /* staged downloads: 0 (default) fcx_download waits for the
                                   stream and fills the caller's heap arrays before it
                                   returns; 1: the host copies wait for the next
                                   fcx_synchronize (a host that overlaps engines)         */
  FCX_OPT_RETIRED_PIN_HOST = 6, /* retired options (version 3): accepted and ignored      */
  FCX_OPT_RETIRED_12 = 12,
  FCX_OPT_RETIRED_CARRY_HANDOFF = 14,
  FCX_OPT_ATMOS_HALO = 17,      /* fused accumulation of one surface type, launched over the
                                   whole grid, on a map whose segments are at most 9 cells:
                                   1 (default) halo tiles -- each wave also computes the
                                   head cells of the next tile for their products, so every
                                   segment completes inside the launch (no crossing records,
                                   no fix-up launch); 0: crossing records + fix-up launch  */
  FCX_OPT_REMAP_PACK = 13,      /* exchange -> model remaps: the fields of a launch packed
                                   cell-major into one record per exchange cell before the
                                   gather, so a link reads one record instead of nf
                                   scattered values.  2 auto (default): launches of >= 2
                                   fields; 1: always; 0: never (gather from the arrays).
                                   Applied at fcx_commit (scratch of cells x record)      */
  FCX_OPT_ATM_RECORDS = 21,     /* engine-owned atmosphere outputs on the device as one record
                                   per atmosphere cell ([cell][field]) instead of one array
                                   per field: a wave of the fused flux launch then stores its
                                   segment sums as one contiguous run.  The host arrays are
                                   plain arrays as ever: fcx_download unpacks the records on
                                   the device first (one more launch per download).  2 auto
                                   (default): exchange grids of >= 2 x PIPELINE_MIN_CHUNK
                                   cells whose whole-grid launch is the halo launch of one
                                   surface type and the six fluxes (FCX_OPT_ATMOS_HALO; any
                                   other launch stores the records value by value, slower
                                   than arrays); 1: wherever the layout applies; 0: never.  It
                                   applies to fp64 engines with tile-blocked mirrors and >= 2
                                   atmosphere fields, none of them the caller's device
                                   memory or used in place.  Applied at fcx_commit; the
                                   environment variable FCX_ATM_RECORDS (0, 1, 2) sets the
                                   default                                                  */
  FCX_OPT_F32_MATH = 22,        /* arithmetic of an FCX_PRECISION_F32 engine.  0 (default):
                                   float, as ever.  1: every flux is computed in double from
                                   its float inputs and rounded to float once where it is
                                   stored; arrays, layout, transports, constants, output-use
                                   rules and fcx_algorithmic_bytes are the fp32 engine's.  One
                                   rule: a value consumed inside the launch that produced it is
                                   consumed in double, unrounded (QSUR -> MEVA and momentum,
                                   MEVA (+ bias) -> HLAT, T_a * EF and the exchange-rate
                                   numerators formed once per cell, a type-0 average formed in
                                   registers / LDS from the types' fluxes, with or without the
                                   fused accumulation riding in the launch: its accumulators
                                   are doubles either way); a value read back
                                   from an array is the stored float, widened (a per-call
                                   subroutine, a regridded field, an average that re-reads its
                                   fields).  Unchanged: the bias slice (rounded to float at
                                   commit, widened when read), everything outside the flux
                                   pass (do_regridding in REAL(4), the accumulation kernel,
                                   fix-up, remaps, record packing, constant fills) and the
                                   fused accumulation's products w * (double)x32 of the
                                   float-rounded flux (several surface types: of the
                                   float-rounded type-0 average), so an atmosphere output stays
                                   the sequential fp64 sum of the engine's own stored values,
                                   rounded once.  No flux is computed in float with it on.
                                   Accepted and without effect on an fp64 engine.  Applied at
                                   fcx_commit (FCX_E_STATE afterwards); other values are
                                   FCX_E_ARG; the environment variable FCX_F32_MATH (0, 1)
                                   sets the default                                         */
  FCX_OPT_CHECK_FINITE = 23,    /* the non-finite guard (a debug mode).  0 off (default); bit 0:
                                   the phase's outputs; bit 1: its inputs too (values 0..3).
                                   With it on, every whole-phase run -- fcx_run, fcx_step,
                                   fcx_step_async, fcx_run_group per member in list order, a
                                   pipelined host step once after its last chunk, over the whole
                                   arrays -- queues range launches (fcx_field_ranges) behind the
                                   phase's work: fix-up, accumulation, the boundary exchange of
                                   an attached communicator, fcx_atmos_finish, remaps.  Bit 1:
                                   every buffer a plan of the phase reads (the received fields'
                                   exchange-grid arrays and engine-filled constants included).
                                   Bit 0: every buffer a plan of the phase writes and stores
                                   (per-type fluxes, type-0 averages, regrid destinations,
                                   RSDR) and the phase's atmosphere outputs.  Left out: outputs
                                   whose store the plan dropped and wave-uniform constants
                                   (nothing to read; constants are finite by fcx_bind_constant's
                                   rule).  fcx_check_fields lists the slots.  The verdict is
                                   read at the call's final wait: fcx_run and fcx_run_group then
                                   end with a wait; fcx_step still downloads first, so the host
                                   has the arrays to look at; after fcx_step_async the next
                                   fcx_synchronize returns it.  Every collective of the call is
                                   queued before the verdict is read, so a rank that finds a bad
                                   value never leaves its neighbours inside the all-reduce.  A
                                   hit returns FCX_E_NONFINITE; fcx_last_error names the first
                                   offender -- inputs before outputs before atmosphere outputs,
                                   then by slot -- e.g. "phase 2: TATM(1,t) cell 4097 = nan
                                   (1 NaN, 0 Inf of 8200 cells)", and fcx_check_result gives the
                                   same as numbers (the value: one 8-B or 4-B copy from the
                                   device, made only on a hit).  The per-call subroutines
                                   (fcx_calc_*, fcx_do_regridding) do not check.
                                   fcx_algorithmic_bytes describes fcx_run's own work and does
                                   not count the check.  Applied at fcx_commit (FCX_E_STATE
                                   afterwards); other values are FCX_E_ARG; the environment
                                   variable FCX_CHECK_FINITE (0..3) sets the default         */
  FCX_OPT_CR_MATH = 24,         /* the transcendental functions of an fp64 engine.  0 (default):
                                   the device library's exp and log, as ever.  1: the three
                                   places where a flux formula leaves IEEE arithmetic -- the
                                   exp of QSUR (CCLM), the exp of RCO's MEVA and the Exner
                                   power (p_s / p_a)**(R_d / c_p) of the CCLM / MOM5 HSEN --
                                   return the CORRECTLY ROUNDED value: the double nearest the
                                   exact exp(a) or x**y, ties to even, for the argument the
                                   formula forms in double.  Every other operation already is
                                   one IEEE operation in the reference's order, so with the
                                   option on every flux is a function of the input bits alone:
                                   it does not move with the ROCm release, and it differs from
                                   a host's result only where that host's libm misrounds.
                                   Domain: exp for 2^-30 <= |a| <= 690; the power for 0.5 <=
                                   x <= 2, x != 1 and 1/16 <= y <= 1.  Outside it (NaN, Inf,
                                   zero or negative pressure ratios, overflow, TSUR within
                                   1e-8 K of the formula's reference temperature) the site
                                   returns what the default build returns.  The evaluation's
                                   error bound is 2^-100 relative (csrc/fcx_crmath.h): an
                                   expected 4e-5 misrounded values in 2.5e9.  Every fp64 launch
                                   has its sibling (T = 1 specialised and generic, several
                                   types, register averages, fused accumulation with records or
                                   halo tiles, remap records, the group launch, the per-call
                                   subroutines); no plan falls back and none is refused.
                                   fcx_run_group merges engines that agree on the option.
                                   Unchanged: arrays, layout, transports, constants, output-use
                                   rules, received fields, the non-finite guard,
                                   fcx_algorithmic_bytes.  A visibly slower step.
                                   Accepted and without effect on an fp32 engine, with or
                                   without FCX_OPT_F32_MATH.  Applied at fcx_commit
                                   (FCX_E_STATE afterwards); other values are FCX_E_ARG; the
                                   environment variable FCX_CR_MATH (0, 1) sets the default  */
  FCX_OPT_SUM_BASELINE = 25,    /* measurement: 1 = the integral launches add every term through
                                   the block's LDS accumulator, without the lanes' register
                                   windows (default 0).  The results are the same bits; only
                                   the time differs (bench/integrals_ab.py).  At any time.   */
  FCX_OPT_ATMOS_INVARIANT = 26, /* atmosphere sums that do not depend on the number of ranks.
                                   0 (default): an atmosphere cell whose exchange cells lie on
                                   several ranks is completed by adding the ranks' partial sums
                                   (launches, slot layout, collective and results as ever).  1:
                                   the ranks exchange the TERMS w[x] * field[x] of such a cell,
                                   each at its link position, and every rank adds them in
                                   increasing x from 0.0 -- the definition above
                                   fcx_set_atmos_map, and the bits of a one-rank engine over the
                                   global grid, for any number of ranks.  Needs
                                   fcx_set_atmos_terms and a sorted atmosphere map; the slots
                                   grow to fcx_atmos_columns doubles per boundary (see
                                   fcx_set_atmos_terms); one more launch per step (the terms,
                                   one for all engines of an fcx_run_group), the same single
                                   all-reduce.  On an engine with boundary slots and a shared
                                   first or last cell, an accumulated field declared
                                   FCX_OUT_UNREAD keeps its store (fcx_output_info says so):
                                   the terms are formed from the stored values.  Applied at fcx_commit
                                   (FCX_E_STATE afterwards); other values are FCX_E_ARG      */
  FCX_OPT_TILED_LAYOUT = 11   /* engine-owned mirrors tile-blocked (default 1): tiles of
                                   4096 cells, the read-only arrays' tiles interleaved in
                                   one pool and the written arrays' in another, so a wave's
                                   accesses fall in one contiguous region (+8-10 % streaming
                                   rate, components.flux_calculator_amd/bench/layout_probe.hip).
                                   Applied at fcx_commit when no field array is the caller's
                                   device memory or used in place (zero-copy) */
};
int fcx_set_option(fcx_engine *e, int option, int64_t value);

/* page-locked host memory owned by the library, mapped for the device at allocation: a
 * host that allocates its local_field arrays here (c_f_pointer in Fortran) gets the
 * zero-copy step on small grids (FCX_OPT_ZERO_COPY auto) and direct DMA on large ones,
 * without any registration of its own memory.  Free only after every engine using the
 * memory is destroyed.  No GPU work; callable before any engine exists. */
int fcx_host_malloc(size_t bytes, void **ptr);
int fcx_host_free(void *ptr);

/* device memory for hosts that keep fields resident in HBM (bind with FCX_MEM_DEVICE) */
int fcx_device_malloc(int device, size_t bytes, void **ptr);
int fcx_device_free(void *ptr);
/* synchronous copy; kind: 1 host->device, 2 device->host, 3 device->device */
int fcx_memcpy(void *dst, const void *src, size_t bytes, int kind);

#ifdef __cplusplus
}
#endif
#endif /* FCX_H */

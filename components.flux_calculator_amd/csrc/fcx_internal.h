// fcx_internal.h -- engine <-> kernel contract (device parameter block) of libfcx.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/fcx.h"

// Measurement switches that make the kernels compute WRONG results (they take work out to
// time what is left).  They exist for the A/B builds of tools/build_variant.sh only, which
// define FCX_AB_BUILD; a product build that sets one of them does not compile.
#if !defined(FCX_AB_BUILD)
#if defined(FCX_TRIVIAL_MATH) || defined(FCX_DBG_ATM_NOLDS) || defined(FCX_DBG_ATM_NOSTORE) || \
    defined(FCX_DBG_NO_HEAD)
#error "FCX_TRIVIAL_MATH / FCX_DBG_*: wrong-result measurement builds need FCX_AB_BUILD"
#endif
#endif
#ifndef FCX_TRIVIAL_MATH  // every formula returns a plain sum of its inputs
#define FCX_TRIVIAL_MATH 0
#endif
#ifndef FCX_DBG_ATM_NOLDS  // no LDS products in the fused accumulation (sums of garbage)
#define FCX_DBG_ATM_NOLDS 0
#endif
#ifndef FCX_DBG_ATM_NOSTORE  // no atmosphere-output stores
#define FCX_DBG_ATM_NOSTORE 0
#endif
#ifndef FCX_DBG_NO_HEAD  // no crossing-record head stores
#define FCX_DBG_NO_HEAD 0
#endif
// Wave timestamps of the fused kernel (measurement builds only: correct results, but an extra
// kernel argument and a store per wave; fcx_debug_wave_trace, bench/wave_trace.py)
#if !defined(FCX_AB_BUILD) && defined(FCX_WAVE_TRACE)
#error "FCX_WAVE_TRACE is a measurement build (FCX_AB_BUILD)"
#endif
#ifndef FCX_WAVE_TRACE
#define FCX_WAVE_TRACE 0
#endif
// Rules of the fused kernels that are stated where they apply, with their evidence:
//  - halo tiles are for the single-type (T = 1) launches only; the multi-type kernel with
//    register averages keeps crossing records (with halo tiles its T = 2 step took +3.9 %,
//    DESIGN.md section 3, profiles/r06/probes/halo_t2_ab.json)
//  - the single-type (TM = 1) kernels wait once, s_waitcnt vmcnt(0), after a type's input loads,
//    in straight-line code before the first flux block, so that no flux block waits for the
//    stores of the blocks before it (fcx_kernels.hip, process / wait_inputs; profiles/r09/isa/)
//  - the compacted map's dependent load of the segments' atmosphere cells follows the flux pass
//    (fcx_kernels.hip, atmos_tile; issued right behind that wait it gained nothing: DESIGN.md
//    section 3, "Current numbers")
//  - which fused launches read the compacted exchange -> atmosphere map: compact_map() below

namespace fcx {

constexpr int kMaxTypes = FCX_MAX_SURFACE_TYPES;
constexpr int kNumVars = FCX_NUM_VARS;
constexpr int kMaxAvg = 24;

// Stage bits of one launch, in the reference call order (flux_calculator.F90:902-991).
enum Stage : uint32_t {
  S_RBBR = 1u << 0,    // calc_flux_radiation_blackbody          (early phase)
  S_QSUR_T = 1u << 1,  // calc_spec_vapor_surface(t)
  S_QSUR_U = 1u << 2,  // calc_spec_vapor_surface(u)
  S_QSUR_V = 1u << 3,  // calc_spec_vapor_surface(v)
  S_MEVA = 1u << 4,    // calc_flux_mass_evap (+ bias)
  S_HLAT = 1u << 5,    // calc_flux_heat_latent
  S_HSEN = 1u << 6,    // calc_flux_heat_sensible
  S_UMOM = 1u << 7,    // calc_flux_momentum_east  (u grid)
  S_VMOM = 1u << 8,    // calc_flux_momentum_north (v grid)
  S_RSDR = 1u << 9,    // distribute_shortwave_radiation_flux
  S_AVG = 1u << 10,    // average_across_surface_types of the registered type-0 outputs
};

// Per surface type, per launch.  A nullptr input means "not needed by this launch"; a
// nullptr output means "not stored" (method none/copy, or stage not in this launch).
struct TGridPtrs {
  const double *tsur, *fice, *psur, *patm, *qatm, *tatm, *uatm, *vatm;
  const double *amoi, *cmoi, *chea;
  const double *qsur_in;  // QSUR(s,t) when not produced in-register (none/copy/not run)
  const double *meva_in;  // MEVA(s,t) when MEVA is not produced in this launch
  double *qsur, *meva, *hlat, *hsen, *rbbr, *rsdr;
};
struct UVGridPtrs {
  const double *tsur, *fice, *psur, *uatm, *vatm, *amom, *cmom;
  const double *qsur_in;
  double *qsur, *mom;  // mom = UMOM on the u grid, VMOM on the v grid
};
struct TypeParams {
  TGridPtrs t;
  UVGridPtrs uv[2];
  int8_t m_qsur[3], m_meva, m_hlat, m_hsen, m_mom, m_rbbr;
  int8_t bias_adds;  // how many times corr(month) is added to MEVA (1 + #'copy' aliases)
  // Outputs computed though not stored (fcx_set_output_use, FCX_OUT_UNREAD): bit WantBit of a flux
  // set = its store pointer is null, but a consumer inside the launch (a later flux, a register
  // average, the fused accumulation, remap records) needs the value, so the block runs and only
  // its store is left out.  The byte behind bias_adds: it arrives with the same scalar load.
  uint8_t want;
  int8_t pad[2];
  // Wave-uniform inputs (fcx_bind_constant): bit ConstBit of an input of t / uv[0] / uv[1] set =
  // that member's 8 bytes hold the VALUE (the double's bits; in an fp32 engine the float's bits
  // in the low word), not an address, and the flux pass issues no vector load for it.  The
  // high half of the bias_adds word, so it arrives with the same scalar load.
  uint32_t cmask;
};
enum ConstBit : int {  // TGridPtrs inputs 0..10, UVGridPtrs inputs of uv[k] at kUvBit0 + 7 k
  K_TSUR = 0, K_FICE, K_PSUR, K_PATM, K_QATM, K_TATM, K_UATM, K_VATM, K_AMOI, K_CMOI, K_CHEA,
  kUvBit0 = 11, KU_TSUR = 0, KU_FICE, KU_PSUR, KU_UATM, KU_VATM, KU_AMOM, KU_CMOM, kUvBits = 7
};
static_assert(kUvBit0 + 2 * kUvBits <= 32, "TypeParams::cmask: 25 bits");
// TypeParams::want.  QSUR(t) and MEVA need no bit: their blocks compute whatever the pointer says.
enum WantBit : uint32_t {
  W_RBBR = 1u << 0, W_HLAT = 1u << 1, W_HSEN = 1u << 2, W_UMOM = 1u << 3, W_VMOM = 1u << 4,
  W_QSUR_U = 1u << 5, W_QSUR_V = 1u << 6
};
// Which kernel family may leave out the store of a wanted output (TypeParams::want) -- ONE rule
// for the kernels (process: elsewhere the byte is a compile-time zero and the code is the stored
// path's) and for the planner (build_plan: elsewhere an FCX_OUT_UNREAD output with a consumer in
// the launch keeps a stored device array).  An output nothing in the launch consumes is a null
// pointer without a want bit, which every family skips as it always has.  Three families do
// not take the path (profiles/r12/): the fp64 CCLM single-type kernel with
// halo tiles (20 B of scratch per lane with it), the fp64 generic multi-type kernel of merged
// grids without register averages (a wave per SIMD at one cell per lane; nothing in that kernel
// consumes a flux but its store, so it never wants one), and the register-average kernels (they
// kept their registers, but the T = 2 bench step was slower with it in every process pair; the
// rule covers the register-average kernels of every precision, the fp32 and wide ones with the
// fused accumulation included: there an unread output that an average or the accumulation
// consumes keeps a stored device array).
// tm1: one surface type fixed at compile time; halo: a launch with halo tiles.
// (f32: the storage type; an fp32 engine computing in double, FCX_OPT_F32_MATH, goes by the fp32
// engine's rule: at its two cells per lane the halo kernels hold no scratch with the path.)
constexpr bool skip_family(bool f32, int variant, bool ravg, bool tm1, bool merged, bool halo) {
  if (ravg) return false;
  if (!f32 && variant == 1 && tm1 && halo) return false;
  if (!f32 && variant == 0 && !tm1 && !ravg && merged) return false;
  return true;
}
// Which kernel family takes wave-uniform inputs -- ONE rule for the kernels (uniform_inputs<>,
// the template arguments of process) and for the planner (build_plan, with the variant and
// register-average mode its launch will be instantiated with): a set cmask bit in a launch of
// any other family would be a value's bits read as an address.  fp64 generic (variant 0) and
// CCLM (1) kernels without register averages; why not the others: DESIGN.md section 3.  (No
// register-average kernel takes them, in any precision: a namelist constant of a multi-type
// launch, fused or not, is an engine-filled array.)
constexpr bool uniform_family(bool f32, int variant, bool ravg) {
  return !f32 && !ravg && (variant == 0 || variant == 1);
}
// The kernels read a type's method bytes as ONE aligned 64-bit word (m_qsur[0] in the low
// byte ... m_rbbr in the high one) and bias_adds with its padding as the next 64-bit word
// (fcx_kernels.hip, type_methods): wave-uniform scalar loads, where a byte member is a
// vector load and a round trip (gfx950 has no byte-sized scalar load).  The layout they rely on:
static_assert(offsetof(TypeParams, m_qsur) % 8 == 0 && offsetof(TypeParams, m_meva) == offsetof(TypeParams, m_qsur) + 3 &&
                  offsetof(TypeParams, m_hlat) == offsetof(TypeParams, m_qsur) + 4 &&
                  offsetof(TypeParams, m_hsen) == offsetof(TypeParams, m_qsur) + 5 &&
                  offsetof(TypeParams, m_mom) == offsetof(TypeParams, m_qsur) + 6 &&
                  offsetof(TypeParams, m_rbbr) == offsetof(TypeParams, m_qsur) + 7,
              "TypeParams: the eight method bytes are one aligned 64-bit word");
static_assert(offsetof(TypeParams, bias_adds) == offsetof(TypeParams, m_qsur) + 8 &&
                  sizeof(TypeParams) == offsetof(TypeParams, bias_adds) + 8,
              "TypeParams: bias_adds and its padding are the next aligned 64-bit word");
static_assert(offsetof(TypeParams, want) == offsetof(TypeParams, bias_adds) + 1 && sizeof(TypeParams::want) == 1,
              "TypeParams: want is byte 1 of the bias_adds word");
static_assert(offsetof(TypeParams, cmask) == offsetof(TypeParams, bias_adds) + 4,
              "TypeParams: cmask is the high half of the bias_adds word");
static_assert(sizeof(TypeParams) % 8 == 0 && alignof(TypeParams) == 8, "TypeParams: 8-B aligned in Params::type[]");
// type-0 average: X0 = sum_{s=1..T} X_s * FARE_s, in order (calc:376-383)
struct AvgEntry {
  double *x0;
  int32_t grid;  // 0,1,2
  int32_t pad;
  const double *x[kMaxTypes];
  const double *fare[kMaxTypes];
};
// Type-0 averages accumulated in registers while the surface types are processed (the
// kernel produces X_s, adds X_s * FARE_s to an accumulator, in type order from 0.0: the
// sum of calc:377-383 without re-reading X_s or FARE_s).  One slot per value the cells
// kernel holds in registers; slots 0..5 are also the fused accumulation fields.
enum AvgSlot : int { A_MEVA = 0, A_HLAT = 1, A_HSEN = 2, A_RBBR = 3, A_UMOM = 4, A_VMOM = 5, A_TSUR = 6 };
constexpr int kAvgSlots = 7;
struct AvgRegs {
  double *out[kAvgSlots];          // type-0 array of the slot, nullptr = not averaged in registers
  const double *fare[kMaxTypes];   // FARE(s) of the t grid (shared by every register slot)
};

// Tile-blocked field layout (FCX_OPT_TILED_LAYOUT).  Cell j of a field array lives at
// element (j >> kLayoutShift) * tile_stride + (j & (kLayoutTile - 1)) of its buffer; the
// kernels get tpad = tile_stride - kLayoutTile and address base + j + (j >> kLayoutShift) * tpad
// (tpad = 0: plain contiguous arrays).  Chunk boundaries of a tiled engine are whole tiles.
constexpr int kLayoutShift = 12;  // tiles of 2^shift cells (4096 measured best)
constexpr int64_t kLayoutTile = int64_t(1) << kLayoutShift;
__host__ __device__ inline int64_t tiled(int64_t j, int64_t tpad) { return j + (j >> kLayoutShift) * tpad; }
// Element of atmosphere cell a in an atmosphere output array.  Two layouts: the arrays of
// their own or the tile-blocked pool (stride 1, tpad), and per-cell records
// (FCX_OPT_ATM_RECORDS: field k's array starts at pool + k, the cells are `stride` = fields
// per record elements apart, tpad 0).
__host__ __device__ inline int64_t atm_at(int64_t a, int64_t stride, int64_t tpad) { return tiled(a, tpad) * stride; }

struct Params {
  int64_t n[3];          // cells per grid
  int64_t n_max;         // max of the grids in this launch
  int32_t num_types;
  uint32_t stages;
  const double *rsdd0;   // RSDD of type 0 (t grid), for S_RSDR
  int32_t merged_uv;     // u/v grids are the t grid (same buffers, same sizes)
  int32_t num_avg;
  TypeParams type[kMaxTypes];
  AvgEntry avg[kMaxAvg];  // averages done by re-reading X_s (the rest)
  AvgRegs ravg;
  int32_t ravg_on;        // any ravg.out set (selects the RAVG kernel instantiation)
  int32_t pad2;
  int64_t tpad;           // tile-blocked layout of every field pointer above (0: contiguous)
  // remap records written by the T=1 specialised launch (the fields of one remap launch
  // group, fcx_engine.hip plan_fused_records): cell j's record at rec + j * rec_p, the value
  // of register slot k (AvgSlot 0..5) at position rec_pos[k] (-1 = not in the record)
  double *rec;
  int32_t rec_p;
  int8_t rec_pos[6];
  int8_t pad3[2];
};
static_assert(offsetof(Params, type) % 8 == 0, "Params::type: the method words are 8-B aligned");
// rec_pos and its padding are read as two aligned 32-bit words too (RecEmit)
static_assert(offsetof(Params, rec_pos) % 4 == 0 && sizeof(Params) >= offsetof(Params, rec_pos) + 8 &&
                  sizeof(Params::rec_pos) == 6,
              "Params: rec_pos[6] + pad3[2] are two aligned 32-bit words");

// launchers (fcx_kernels.hip); return hipError_t as int
// how one cells_kernel launch is instantiated
struct LaunchConfig {
  int cells_per_thread = 2;  // 1 or 2 (2 needs 16-B aligned arrays)
  int max_blocks = -1;       // grid-stride cap; 0 = one unit per thread; -1 = per-kernel
                             // default (cells_kernel: 8192, fused accumulation: one trip)
  bool nontemporal = true;   // non-temporal hint on the streamed loads/stores
  bool merged = false;       // u/v grids are the t grid
  int variant = 0;           // 0 generic, 1 CCLM, 2 MOM5, 3 RCO (T=1 specialisations)
  bool f32 = false;          // fp32 fields (FCX_PRECISION_F32): 4 cells per lane
  bool wide = false;         // ... computed in double (FCX_OPT_F32_MATH; needs f32): the same
                             // launch shapes, tiles and maps, the F32Wide instantiations
  bool cr = false;           // fp64 fields, the transcendental sites correctly rounded
                             // (FCX_OPT_CR_MATH; never with f32): the fp64 launch shapes, the
                             // F64Cr instantiations
  bool ravg = false;         // register averages in this plan (Params::ravg_on)
  int64_t lo = 0, hi = -1;   // cell range of this launch (lo a multiple of kChunkAlign;
                             // hi < 0: to n_max) -- the pipelined host-bound step
  bool rec = false;          // Params::rec set: the launch also writes remap records
                             // (T=1 specialised fp64 kernels, 2 cells per lane)
  int halo = 0;              // fused accumulation with halo tiles (AtmosFused::halo lanes)
};
constexpr int64_t kChunkAlign = 1024;  // chunk boundaries: whole wave tiles and vectors

struct AtmosFused;
// corr_m: month slice [n_t] of the bias corrections (device), or nullptr
int launch_cells(const Params *host_params, const Params *dev_params, const double *corr_m,
                 const LaunchConfig &lc, void *stream, const AtmosFused *atm = nullptr);
constexpr int kMaxAtmosFields = 16;
struct AtmosArgs {
  const int32_t *row_ptr;  // [n_atmos + 1] into the exchange cells (CSR by atmosphere cell)
  const int32_t *col;      // exchange cell of each link, or nullptr when col[k] == k
  const double *w;         // [links]
  int64_t n_atmos;
  int32_t nf;
  int32_t stride;
  int32_t left, right;     // boundary slot of the first / last atmosphere cell, -1 = none
  double *shared;
  const double *x[kMaxAtmosFields];
  double *out[kMaxAtmosFields];
  int32_t f32;             // fields and outputs are float arrays (fp32 engine); the weights,
                           // products and sums stay fp64 (OASIS maps in double)
  int64_t tpad;            // layout of the x fields (engine buffers)
  int64_t out_tpad;        // layout of out: the engine's tiled atmosphere pool, or 0
  int64_t out_stride = 1;  // ... elements between atmosphere cells (atm_at): 1, or the record length
  int32_t vec;             // col == nullptr and every x 16-B aligned: vector staging loads
  int32_t rec_p;           // elements per record of rec (nf rounded up to a 16-B multiple)
  const void *rec;         // remap gather: the x fields packed cell-major (pack_records),
                           // record of exchange cell j at rec + j * rec_p; nullptr = SoA gather
  int32_t scol[kMaxAtmosFields];  // column of field f in the shared boundary slots: the
                                  // field's registration index (fcx_add_atmos_field order),
                                  // the same for every phase and for the fused kernel
  // FCX_OPT_ATMOS_INVARIANT (0 everywhere with the option off): terms_k = K > 0 says the slots
  // carry, behind the term0 partial-sum columns (term0: the registered fields), K term columns
  // per registered field -- column term0 + scol[f] * K + p holds the term at link position p --
  // and left_pos is the position of this rank's first exchange cell within its first
  // atmosphere cell (fcx_set_atmos_terms)
  int32_t terms_k;
  int32_t term0;
  int32_t left_pos;
};
int launch_atmos(const AtmosArgs &a, void *stream);
// FCX_OPT_ATMOS_INVARIANT: the terms w[x] * field[x] of the first and last local atmosphere
// cells of n engines (same precision, one stream; n <= kMaxGroup) into the term columns of their
// boundary slots, ONE launch (fcx_atmos_terms.hip).  max_items: the largest (cells x fields) of
// any boundary cell, which sizes the grid.  Engines without a slot or with terms_k == 0 are
// passed over.
// The largest K fcx_set_atmos_terms takes: the ordered finish adds a slot's K terms in one
// thread, and a region row is fields * (1 + K) doubles
constexpr int32_t kMaxAtmosTerms = 4096;
int launch_atmos_terms(const AtmosArgs *as, int n, int64_t max_items, void *stream);
// atmos_finish of several engines (same precision, one stream) in one launch
struct FinishGroup;
int launch_atmos_finish_group(const AtmosArgs *as, const int32_t *n_boundaries, int n, void *stream);
// remap records: rec[j * P + f] = x[f][tiled(j)] for f < nf, 0 for nf <= f < P, cells
// j < n (P a multiple of the 16-B vector length); aligned16: every x is 16-B aligned;
// nontemporal: streaming hint on the field loads (off for host-mapped fields)
int launch_pack_records(const AtmosArgs &a, int64_t n, bool aligned16, bool nontemporal, void *rec, void *stream);

// Exchange -> atmosphere accumulation fused into the T=1 cells kernel (or, with several types,
// into the register-average kernel: the type-0 averages instead of the fluxes; fp64, fp32 and
// fp32 computing in double alike).  The six fluxes it
// can take from registers, in this order: MEVA HLAT HSEN RBBR UMOM VMOM (out[k] nullptr =
// not accumulated).  Every 128-cell wave tile sums the segments that start in it; a
// segment running past the tile end leaves its prefix sum in the next tile's crossing
// record, whose head cells atmos_fixup_kernel adds after the launch in link order (no wave
// ever waits on another).
constexpr int kFusedFields = 6;
constexpr int kRecHead = 4;     // head products kept per crossing record (longer heads: recomputed)
constexpr int kXRec = 32;       // doubles per crossing record (256 B, two lines)
constexpr int kTile = 128;  // cells per wave iteration (64 lanes x 2)
// the fused launches that read the compacted map (AtmosFused::seg_*) rather than idx: the fp32
// launches and the fp64 halo launches; fp64 launches with crossing records read the 4-B index per
// cell (the compacted map there lost: T = 2 +1.1 %, T = 1 on the periodic map +2.1 %,
// profiles/r05/f64seg2/; an index in the halo launches too lost 0.1 - 0.7 %, profiles/r05/f64seg/)
constexpr bool compact_map(bool f32, bool halo) { return f32 || halo; }
struct AtmosFused {
  // the exchange -> atmosphere map of a contiguous (sorted) map, compacted (round 5): bit x of
  // seg_bits[x / 32] is set where exchange cell x starts a segment (its atmosphere cell
  // differs from cell x-1's); seg_pre[w] counts the starts in cells < 32 w; seg_atm[s] is the
  // atmosphere cell of segment s.  1/8 + 1/8 + 4/(cells per segment) bytes per cell instead
  // of a 4-B index per cell.  Which launches read it and which read idx: compact_map().
  const uint32_t *seg_bits;
  const int32_t *seg_pre;
  const int32_t *seg_atm;
  const int32_t *tile_a0;  // compacted map: the atmosphere cell of each wave tile's first cell
                           // (crossing records; a load that depends on nothing)
  const int32_t *idx;  // the local atmosphere cell of every exchange cell
  const double *w;
  double *out[kFusedFields];
  const double *x[kFusedFields];  // the stored outputs (read by the fix-up only)
  double *xrec;        // [n_tiles][kXRec] crossing records (atmos_fixup_kernel):
                       // record t = the carry of tile t-1's last segment (doubles 0..5), the
                       // products w * x of tile t's first kRecHead head cells (6..29, cell-major)
                       // and {head cells, their atmosphere cell} of tile t (int2 at double 30);
                       // fp32 engines index the records by their 256-cell tiles
  int32_t xrec_on;     // some segment crosses a tile boundary: the launch fills the records
  int32_t halo;        // > 0: halo tiles (no records, no fix-up): a wave owns the cells of its
                       // first 64 - halo lanes and computes the fluxes of the last `halo`
                       // lanes' cells -- the head of the next tile -- for its products only,
                       // so every segment that starts in its own cells ends inside the wave
                       // (needs halo * C >= the longest segment - 1; full-range launches)
  int64_t n_atmos;
  double *shared;
  int32_t stride, left, right;
  int64_t tpad;        // layout of x (engine buffers); idx, w are contiguous
  int64_t out_tpad;    // layout of out (tiled atmosphere pool, or 0)
  int32_t out_stride = 1;  // ... elements between atmosphere cells (atm_at): 1, or the record length
  int32_t rec_dense;   // out is one record of exactly the kFusedFields fluxes per cell, in slot
                       // order (out[k] == out[0] + k, out_stride == kFusedFields, 16-B aligned):
                       // the halo launch stores a wave's run of records densely
  int32_t scol[kFusedFields];  // shared-slot column of fused field k (AtmosArgs::scol)
  int64_t n_tiles;     // tiles [lo / tile cells, n_tiles) of one launch (set per launch, so no
                       // wave divides by the halo-dependent tile size)
#if FCX_WAVE_TRACE
  uint64_t *trace;     // per wave (dispatch order): {start, end, HW_ID, XCC_ID}, or nullptr
#endif
};
// Several engines' fused launches (T = 1, or several types with register averages) in ONE launch
// (fcx_run_group): member k's wave tiles
// are tiles [tile0, tile0 + af.n_tiles) of the grid.  Passed by value (kernel arguments).
constexpr int kMaxGroup = 4;
struct FinishGroup {
  int32_t n;
  int32_t nb[kMaxGroup];
  AtmosArgs a[kMaxGroup];
};
// cells per lane of the fp32 engine's fused kernels (16-B lanes of 4 floats; 2, 8-B lanes of
// 2 floats in 128-cell tiles like the fp64 kernels and half the registers per lane, took the
// group step from 0.441 to 0.460 ms: profiles/README.md, round-4 index, profiles/r04/f32c2/)
constexpr int kF32Cpl = 4;
// ... and of the wide fused kernels (FCX_OPT_F32_MATH): 2, 8-B lanes of 2 floats in 128-cell
// tiles.  Their step is bound by the fp64 arithmetic, not by memory: four cells per lane hold
// 172-197 VGPRs (2 waves per SIMD) and ran the T = 1 group launch in 0.811 ms, two cells per
// lane fit the 128 of 4 waves and ran it in 0.688 ms (profiles/r13/f32_math/ab/).  The tile
// size is all that differs from the fp32 engine's launches: the compacted map, the crossing
// records (indexed by this tile), halo lanes and the fix-up go by it.
constexpr int kWideCpl = 2;
// cells per lane of a fused launch: fp64 2, fp32 kF32Cpl, fp32 computing in double kWideCpl
constexpr int fused_cpl(bool f32, bool wide) { return !f32 ? 2 : wide ? kWideCpl : kF32Cpl; }
struct GroupMember {
  const Params *P;        // the member's device parameter block
  const double *corr_m;   // its month slice, or nullptr
  int64_t tile0;          // its first tile in the group's grid
  int32_t var;            // 1 CCLM, 2 MOM5, 3 RCO (the T = 1 specialisation)
  int32_t pad;
  AtmosFused af;          // its accumulation (af.n_tiles: its tile count)
};
// The grid's tiles in ranges: grid tiles [t0, next range's t0) are tiles [first, ...) of member
// `member`; a group launch has one range per member (all its tiles).  (Round 5 also launched
// the boundary-slot tiles apart, as ranges of the same members, to overlap the exchange; it
// measured slower and was removed in round 6.)
constexpr int kMaxGroupRanges = kMaxGroup;
struct GroupRange {
  int64_t t0;
  int64_t first;
  int32_t member;
  int32_t pad;
};
struct GroupArgs {
  int32_t n;
  int32_t n_ranges;
  int64_t total_tiles;
  GroupMember m[kMaxGroup];
  GroupRange r[kMaxGroupRanges];
};
// lc: the members' common launch shape (nontemporal, f32, halo > 0 or not); af.n_tiles of
// every member is set by the caller.  hipError_t as int.
int launch_cells_group(GroupMember *members, int n, const LaunchConfig &lc, void *stream);

// the segments carried over a tile boundary: carry of tile t-1 + the head cells of tile t,
// for every tile of a launch of n_cells (fp32: 256-cell tiles of float fields)
// (wide: an fp32 engine computing in double, whose tiles are 64 * kWideCpl cells)
int launch_atmos_fixup(const AtmosFused &af, int64_t n_cells, bool f32, void *stream, bool wide = false);
// atmosphere records -> the tile-blocked pool the downloads read: soa[f][tiled(a, tpad)] =
// rec[a * nf + f], a < n_atmos (fp64; rec and soa 16-B aligned)
int launch_atm_unpack(const double *rec, double *soa, int64_t n_atmos, int nf, int64_t tpad, void *stream);
// zero the fused outputs of the n atmosphere cells in cells[] (cells without exchange cells)
int launch_atmos_zero(const AtmosFused &af, const int32_t *cells, int64_t n, bool f32, void *stream);
// the fix-ups of several engines' fused launches (fcx_run_group members) as one launch
struct FixupGroup {
  int32_t n;
  int32_t pad;
  int64_t first[kMaxGroup + 1];  // member m's (tile boundary, field) threads: [first[m], first[m+1])
  AtmosFused af[kMaxGroup];
};
int launch_atmos_fixup_group(const AtmosFused *afs, const int64_t *n_cells, int n, bool f32, void *stream,
                             bool wide = false);
int launch_atmos_finish(const AtmosArgs &a, int32_t n_boundaries, void *stream);

// f32: w, src and dst are float arrays (the reference's single-precision build, where the
// matrix weights and the fields are REAL(wp) = REAL(4), basic:117-122, and so is the sum)
// src and dst: engine buffers in the layout tpad
int launch_regrid_csr(const int32_t *row_ptr, const int32_t *col, const double *w,
                      const double *src, double *dst, int64_t n_dst, void *stream, bool f32 = false,
                      int64_t tpad = 0);
// x[tiled(j, tpad)] = value for the cells j < n of an engine buffer in the layout tpad (the
// mirror of a constant field, fcx_bind_constant); f32: x is a float array and value is
// rounded to float once
int launch_fill(double *x, int64_t n, double value, bool f32, int64_t tpad, void *stream);

// Model grid -> exchange grid gather of received fields (fcx_bind_received): the fields of one
// (map, phase), at most kMaxReceiveFields per launch, by value.  dst[f][tiled(j, tpad)] = sum over
// the links of exchange cell j < n, in link order from 0.0, of w * src[f][source cell]; a cell
// without a link gets 0.0; cells past n are not written.  Injection form (idx set): idx[j] is the
// one source cell of exchange cell j or -1, padded with -1 to a multiple of 4 entries and 16-B
// aligned; w is one weight per exchange cell, or nullptr when every weight is 1.0.  General form
// (idx == nullptr): CSR by exchange cell (row_ptr [n + 1], col and w per link).  Sources are
// engine buffers in the layout tpad, or (bit f of src_plain) contiguous arrays; the engine has
// checked every source cell against the sources' length.  f32: float fields, double arithmetic.
constexpr int kMaxReceiveFields = 16;
struct ReceiveArgs {
  const int32_t *idx;
  const double *w;
  const int32_t *row_ptr, *col;
  int64_t n;
  int64_t tpad;
  int32_t nf;
  int32_t f32;
  uint32_t src_plain;
  uint32_t pad;
  const void *src[kMaxReceiveFields];
  void *dst[kMaxReceiveFields];
};
int launch_receive(const ReceiveArgs &a, void *stream);

// Field ranges (fcx_field_ranges, fcx_atmos_ranges, FCX_OPT_CHECK_FINITE): min / max over the
// cells that are not NaN, the NaN and Inf counts and the lowest cell holding either, of at most
// kMaxRangeFields fields per launch, by value.  Cell j < n of field f is element
// tiled(j, tpad) * stride of p: stride 1 for every field buffer (contiguous, tpad 0, or
// tile-blocked), the record length for an atmosphere output kept as per-cell records (atm_at).
// Cells at or past n are never read.  field_range_kernel stores one partial per (field, block)
// into `partial` ([nf][blocks], the engine's scratch of kRangePartials entries) and
// field_range_finish_kernel, the next launch on the stream, folds them into out[f]: no wave
// waits for another, nothing is added to atomically, and the result does not depend on the grid.
constexpr int kMaxRangeFields = 16;
constexpr int kRangePartials = 2048;  // 80 KiB of scratch
struct RangeField {
  const void *p;
  int64_t n;
  int64_t tpad;
  int32_t stride;
  int32_t vec;  // set by launch_field_ranges: stride 1 and a 16-B aligned array, read with 16-B loads
};
struct RangeArgs {
  int32_t nf;
  int32_t f32;  // float fields (min / max widened to double, exactly)
  RangeField f[kMaxRangeFields];
  fcx_field_range *partial;
  fcx_field_range *out;  // [nf], device memory
};
int launch_field_ranges(RangeArgs a, void *stream);

// Exact field sums (fcx_field_integrals, fcx_atmos_integrals; fcx_integrals.hip, fcx_exactsum.h):
// the range launches' descriptor and addressing rule, plus per field the areas (cell j's weight
// is area[j]: contiguous, never tile-blocked, a 16-B aligned allocation of the engine's; nullptr
// when the launch is unweighted) and, for a wave-uniform constant, the value in place of an
// array (uniform: r.p is not read, every cell j < r.n holds cval).  field_sum_kernel stores one
// canonical 72-word partial (68 limbs, 4 counts: an fcx_exact_sum) per (field, block) into
// `partial` ([nf][blocks] of kRangePartials, 1.1 MiB of scratch), field_sum_finish_kernel folds
// them into out[f].
constexpr int kSumWords = FCX_SUM_LIMBS + 4;
struct SumField {
  RangeField r;
  const double *area;
  double cval;
  int32_t uniform;
  int32_t pad;
};
struct SumArgs {
  int32_t nf;
  int32_t f32;       // float fields (widened to double, exactly)
  int32_t weighted;  // every field's area is set
  int32_t baseline;  // measurement: every term through the LDS accumulator, no register window
  SumField f[kMaxRangeFields];
  int64_t *partial;
  fcx_exact_sum *out;  // [nf], device memory
};
int launch_field_sums(SumArgs a, void *stream);

}  // namespace fcx

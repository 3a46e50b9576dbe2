// Host side of the line-by-line extinction, shared by its translation units: the plan handle, what
// a call asks for (Call), the PB_* variables it consults (Tuning), what it will launch (GatherPlan)
// and the functions that cross files.  Kernel-side definitions are in pb_ext_args.h.
#pragma once

#include <vector>

#include "pb_ext_args.h"

// ===========================================================================
// handles
// ===========================================================================
struct pb_lbl {
    pb_voigt *voigt = nullptr;
    pb_lines *lines = nullptr;
    int nwave = 0, nmol = 0, niso = 0, ndivs = 0, max_layers = 0, resolution = 0;
    int nrows_sep = 1;       // rows when add == 0
    double cutoff = 0, ethresh = 0, wnstep = 0, wn0 = 0;
    std::vector<int32_t> isoiext;
    double *d_wn = nullptr, *d_molrad = nullptr, *d_molmass = nullptr, *d_isomass = nullptr,
           *d_isoratio = nullptr;
    int32_t *d_divisors = nullptr, *d_isoimol = nullptr, *d_isoiext = nullptr;
    // workspace
    int32_t *ls_ofactor = nullptr, *ls_scale = nullptr, *li_ilor = nullptr, *li_hmax = nullptr;
    int32_t *li_rowmax = nullptr, *li_hlo = nullptr, *li_hhi = nullptr;
    int64_t *ls_dnwn = nullptr;
    double *ls_dwnstep = nullptr, *li_alphad = nullptr, *li_dens = nullptr, *li_z = nullptr;
    double *ls_quot = nullptr;        // [5][max_layers]: cutsteps, 1/ofactor, 1/scale, 1/temp, 1/dwnstep
    double *li_invz = nullptr;        // [max_layers][niso] 1 / partition function
    unsigned long long *kmax_bits = nullptr;
    int kmax_rows = 0;
    // phase-sorted copy of the groups for the LDS-staged kernel
    int32_t *ph_first = nullptr, *ph_count = nullptr, *ph_iown = nullptr;
    int64_t *ph_start = nullptr;
    int32_t *ph_iso = nullptr;
    int32_t *ph_bin = nullptr;
    int ph_nbins = 0;
    double *ph_lead = nullptr;       // leader lwn, elow, gf of the phase-sorted groups [3][G]
    double *g_lead = nullptr;        // same for the position-sorted groups
    double *rec_k = nullptr;
    int32_t *rec_i32 = nullptr;      // 5 arrays of max_layers*ngroups
    int rowcap = 0;
    int32_t *ls_resident = nullptr;   // [max_layers]
    int32_t *ls_block = nullptr;      // [max_layers]
    int32_t *ls_wave = nullptr;       // [max_layers] layers of the wave-autonomous kernel
    pbx::Rec32 *rec32 = nullptr;           // [max_layers][ngroups], scatter kernel
    size_t rec32_bytes = 0;
    pbx::Rec16 *rec16 = nullptr;           // [layers of the largest call][ngroups][nch_max], staged kernel
    size_t rec16_alloc = 0;
    double *part = nullptr;           // partial sums of a phase-split staged launch
    size_t part_bytes = 0;
    // window map of two-phase shard calls (LblArgs::wm_*): host copies of the phase-sorted group
    // positions, the cached map and the window / order it was built for
    std::vector<int32_t> h_ph_iown;
    std::vector<int64_t> h_ph_start;
    std::vector<int32_t> h_wm;
    int32_t *d_wm = nullptr;
    size_t wm_bytes = 0;
    int64_t wm_flo = 0, wm_fhi = -1;
    int wm_staged = -1, wm_n0 = 0, wm_n1 = 0;
    int64_t wm_total0 = 0, wm_total1 = 0;
    int32_t *gs_start = nullptr;      // [niso][nwave+1]
    int res_cap = 0;                  // LDS doubles of one resident profile block (0 = none fits)
    // Which layers are resident is decided on the device, per call; a plan none of whose layers
    // ever qualifies (C2: the smallest block a layer selects is 53 820 doubles) still paid an
    // empty launch of the resident kernel on every spectrum (7.5 us).  The host looks at the
    // decision of the first automatic call and of every 256th one (one small synchronous copy
    // each): while no layer qualified the resident kernel is left out (res_cap = 0 for the whole
    // call: the staged / global kernel computes every layer).
    int res_seen = -1;                // -1 not looked yet, 0 no resident layer, 1 some
    uint64_t res_calls = 0;
    bool res_on_pending = false;      // decision of a two-phase call's first half
    bool res_look_pending = false;
    // packed (layer, group) records above this many bytes are produced and consumed in chunks of
    // the line list (pb_lbl_set_record_budget; PB_RECORD_BUDGET overrides)
    size_t record_budget = (size_t)96 << 30;
    int last_chunks = 0;     // chunks of the last call (0 = records of every group at once)
    // per-layer phase split of the staged kernel: device tables and the configuration they hold
    int32_t *d_unit_tab = nullptr, *d_lsplit = nullptr;
    size_t ut_bytes = 0, ls_bytes = 0;
    // per-tile phase split (uneven line density): device table and what it was made for
    int32_t *d_tsplit = nullptr;
    int32_t *pos2ph = nullptr;                        // [ngroups] (LblArgs::pos2ph)
    bool ts_sparse = false;                           // some tile of the table is the global gather's
    int64_t ts_key[4] = {-1, -1, -1, -1};            // wbegin, wcount, tile, base split
    int ts_max = 0;
    size_t ts_bytes = 0;
    int ut_key[4] = {-1, -1, -1, -1};                 // nlayers, base split, deep layers, deep split
    int ut_units = 0;
    int concurrency = 1;     // independent calls the caller keeps in flight beside this plan's
    int gather_mode = 0;     // 0 = choose, 1 = global gather, 2 = LDS-staged, 3 = resident+global
    // a constant-step sub-plan of a `resolution` plan's dynamic grids (pb_ext_resolution.hip): its
    // staged launches keep one row per barrier step (measured slower with two: profiles/rows_per_step.md)
    bool dyn_child = false;
    int last_gather = 0;     // last call: 1 global, 2 staged, 3 linterp; +8 = resident kernel too
    double stage_threshold = 8.0;   // groups per (2048-sample tile, phase) to go staged
    // optional per-launch timing of the gather kernel (bench.py's roofline figure)
    std::vector<hipEvent_t> ev;      // start/stop pairs
    int ev_used = 0;
    // round-staged gather (pb_rounds.hip): per-unit capacities (cached per launch geometry)
    // and the visit-record / segment / header lists
    int64_t *unit_cap = nullptr;
    size_t unit_cap_bytes = 0;
    int64_t cap_key[5] = {-1, -1, -1, -1, -1};   // wbegin, wcount, tile, nsplit, total
    pbx::VRec *vrec = nullptr;
    pbx::VSeg *vseg = nullptr;
    int32_t *vrnd = nullptr;
    size_t vrec_alloc = 0;            // entries
    pbx::UnitHdr *uhdr = nullptr;
    size_t uhdr_bytes = 0;
    struct Pending {                 // call begun with pb_lbl_extinction_begin
        double *ext;
        int64_t wbegin, wcount;
        const double *temp, *dens, *isoz;
        int64_t zs0, zs1;
        int nlayers, add;
        bool open;
    } pending = {nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0, false};
    pbx::LblArgs last_args;               // arguments of the last launch (pb_lbl_last_work)
    bool last_packed = false;        // ... whose records are packed, one per (layer, group)
    // `resolution` plans, gather mode 6: one constant-step plan per oversampling factor in use
    // (the layer's dynamic grid IS a constant-step grid of step ofactor fine samples), with the
    // Voigt table cut into phase rows modulo that factor (pb_voigt_rephase: kept by the table)
    struct DynSub {
        int f;
        pb_voigt *voigt;
        pb_lbl *plan;
        double *ktmp;                // dynamic-grid sums of one run of layers
        size_t ktmp_bytes;
        uint64_t call;               // last call that used it, and on which side stream
        int lane;
    };
    std::vector<DynSub> dyn;
    // Host-free calls (opt-in, pb_lbl_set_dyn_predict): the run plan comes from the factors /
    // Lorentz rows the layers had when they were last read back (pred_*), a device check marks the
    // layers it fits (d_ok), the direct gather computes the others; this call's state is read back
    // asynchronously (rb_*) and adopted by a later call.  A read-back that contradicts the
    // prediction makes the next dyn_hold calls synchronous (one stream synchronisation each, the
    // default form): atmospheres that change from call to call are not worth predicting.  Opt-in
    // because a layer that takes the direct gather differs from the same layer on its dynamic grid
    // in the last bits (the same terms in another order): with the prediction on, a result can
    // depend on the plan's history at the 1e-13 level; with a steady atmosphere it never does.
    std::vector<int32_t> pred_f, pred_ilor, used_f;
    int pred_layers = 0, pred_cap = 0, dyn_hold = 0;
    bool pred_dirty = false, rb_pending = false, dyn_fallback = false;
    int dyn_predict = 0;             // pb_lbl_set_dyn_predict
    int32_t *d_pred_f = nullptr, *d_ok = nullptr, *rb_host = nullptr;
    const uint8_t **d_pred_mask = nullptr;
    size_t rb_cap = 0;
    int rb_layers = 0;
    hipEvent_t rb_ev = nullptr;
    int64_t dyn_spec_calls = 0, dyn_sync_calls = 0, dyn_mispredicted = 0;
    uint64_t dyn_call = 0;
    int dyn_runs = 0;                // runs of equal-factor layers of the last call
    // the runs of a call are independent until ext: dealt to side streams (deep layers have
    // short dynamic grids and factors of their own: launches of one layer that leave the chip idle)
    std::vector<hipStream_t> dyn_streams;
    std::vector<hipEvent_t> dyn_join;
    hipEvent_t dyn_fork = nullptr;
    std::vector<int32_t> h_ofactor, h_ilor, h_divisors, h_isoimol, h_isoiext0;   // (isoiext at creation)
    std::vector<double> h_wn, h_molrad, h_molmass, h_isomass, h_isoratio;
};

namespace pbx {

using Call = pb_lbl::Pending;        // what the caller asked for
using GatherKernel = void (*)(LblArgs);

// The PB_* variables a call consults.  Read once at the top of EVERY call, never kept in the
// handle or in a static: the tests change them between calls of one process.
struct Tuning {
    int experiment = 0;            // PB_EXPERIMENT
    bool dma = true;               // PB_STAGE_DMA=0: rows via registers
    bool no_long_rows = false;     // PB_NO_LONG_ROWS (set at all)
    int stage_s = 0;               // PB_STAGE_S as 1, 2 or 4; 0 = not set
    int stage_split = 0;           // PB_STAGE_SPLIT as 1..8; 0 = not set
    int stage_rows = 0;            // PB_STAGE_ROWS as 1..kStageRowsMax; 0 = not set
    bool poison = false;           // PB_POISON_RECORDS (set and not 0)
    bool budget_set = false;       // PB_RECORD_BUDGET
    size_t budget = 0;
    bool rec_soa = false;          // PB_REC_SOA (set at all)
    int wave = -1;                 // PB_WAVE: 0 / 1; -1 = not set
    bool res_dyn_off = false;      // PB_RES_DYN=0
    bool rec_layers_1 = false;     // PB_REC_LAYERS=1
    bool no_window_map = false;    // PB_NO_WINDOW_MAP (set at all)
    size_t wm_lds_cap = 48 * 1024; // PB_WM_LDS_CAP
    int scatter_t = 512;           // PB_SCATTER_T as 512, 1024 or 2048
    int rounds_geom = 2;           // PB_ROUNDS_GEOM as 0..7
    bool deep_set = false;         // PB_STAGE_DEEP=frac[,factor]
    double deep_frac = 0.0;
    int deep_factor = 2;
    bool tile_split_off = false;   // PB_TILE_SPLIT=0
    int tile_min = 1;              // PB_TILE_MIN
    bool tile_debug = false;       // PB_TILE_DEBUG (set at all)
    bool tile_global_off = false;  // PB_TILE_GLOBAL=0
    int stage_probe = 0;           // PB_STAGE_PROBE
    int rsplit = 0;                // PB_RSPLIT as 1, 2, 4 or 16; 0 = not set
    int dyn_streams = 4;           // PB_RES_DYN_STREAMS as 1..8
    int dyn_big = 1;               // PB_RES_DYN_BIG as 1..7
};

// What a call will launch, decided from the plan, the arguments and the environment alone.
struct Chunk {
    int key_lo, key_hi;
    int64_t g_lo, g_hi;
};

struct GatherPlan {
    int rc = PB_OK;                  // the call cannot be planned (pb_last_error says why)
    bool staged = false, rounds = false, scatter = false;
    bool use_records = false, packable = false;
    // resident-profile kernel.  plan_gather() says whether the plan and the mode allow it
    // (resident) and whether the layers' own decision counts too (res_auto); resident_probe()
    // then settles `resident` and `res_look` (read the layers' decision back after this call)
    bool resident = false, res_auto = false, res_look = false;
    bool dma = true;                 // rows by LDS-DMA (k_ext_staged); PB_STAGE_DMA=0: via registers
    bool shared_chip = false;
    int S = 2, nsplit = 1;
    int nch_max = 1, rowlds = 0;     // LblArgs::nch_max, rowlds
    size_t lds = 0;                  // dynamic LDS of the staged kernel
    double per_phase = 0.0;          // groups per (2048-sample tile, phase)
    // out-of-core line lists: the chunks of the phase-sorted group list (empty: one piece), the
    // bytes of packed records the call needs, whether it uses packed records at all, and the
    // format k_records writes (launch_records)
    std::vector<Chunk> chunks;
    size_t rec16_need = 0;
    bool packed = false;
    int fmt = 0;
};

// pb_extinction.hip
int64_t group_reach(const pb_voigt *v, double cutoff, double ownstep);
int64_t groups_in_reach(const pb_lines *l, int niso, int64_t flo, int64_t fhi);
int ensure_bytes(void **ptr, size_t *have, size_t need, hipStream_t s, bool sync_first,
                 const char *what);
int64_t plane_bytes(const LblArgs &a);
int cap_split_to_planes(int n, int64_t plane, int least = 1);
int ensure_part(pb_lbl *p, LblArgs &a, int nplanes, hipStream_t s);
int lbl_extinction(pb_lbl *p, const Call &c, void *stream, int phase);
// pb_ext_records.hip
int launch_layer_state(const LblArgs &a, hipStream_t s);
int launch_kmax(const LblArgs &a, hipStream_t s);
size_t records_lds(const LblArgs &a, int per);
int launch_records(const LblArgs &a, int fmt, int per, dim3 grid, size_t lds, hipStream_t s);
// pb_ext_gather.hip
GatherKernel staged_kernel(int S, bool dma, int rows);   // rows: LblArgs::rows_cap
int allow_lds(const void *kern, size_t lds);
int launch_staged(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn, hipStream_t s);
int launch_global(LblArgs &a, const Tuning &tn, hipStream_t s);
int launch_resident(LblArgs &a, hipStream_t s);
// pb_ext_resolution.hip
int launch_linterp(LblArgs &a, hipStream_t s);
int lbl_resolution_dyn(pb_lbl *p, LblArgs &a, const Call &c, const Tuning &tn, hipStream_t s);

// the measured dead ends that cross files (`make EXPERIMENTS=1`): the scatter and round gathers
// (pb_ext_gather.hip) and the wave kernel (pb_extinction.hip); the default library has the stand-ins
#ifdef PB_EXPERIMENTS
int exp_launch_scatter(LblArgs &a, const Tuning &tn, hipStream_t s);
int exp_launch_rounds(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn, hipStream_t s);
int exp_launch_wave(const LblArgs &a, int nunits, hipStream_t s);
#else
static inline int exp_launch_scatter(LblArgs &, const Tuning &, hipStream_t) { return PB_OK; }
static inline int exp_launch_rounds(pb_lbl *, LblArgs &, const GatherPlan &, const Tuning &,
                                    hipStream_t) { return PB_OK; }
static inline int exp_launch_wave(const LblArgs &, int, hipStream_t) { return PB_OK; }
#endif  // PB_EXPERIMENTS

}  // namespace pbx

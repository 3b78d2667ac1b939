// The library's context: owned HIP resources, creation and teardown.
//
// Every device buffer, pinned host buffer, stream and event sits in a move-only handle that
// releases it in its destructor, so a context (and a slab's communicator) is torn down by
// deleting it, and creation returns on the first failure without a cleanup list of its own.
#pragma once

#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "cell_build.h"
#include "common_kernels.h"
#include "full_kernels.h"
#include "full_tiled.h"
#include "ref_kernels.h"
#include "sample_kernels.h"
#include "surface_kernels.h"
#include "render_kernels.h"
#include "scene_kernels.h"
#include "tint_kernels.h"
#include "tracer_kernels.h"
#include "gauge_kernels.h"
#include "pressure_kernels.h"
#include "scalar_kernels.h"
#include "buoyancy_kernels.h"
#include "cohesion_kernels.h"
#include "xsph_kernels.h"
#include "viscous_implicit_kernels.h"
#include "viscous_kernels.h"
#include "monitor_kernels.h"
#include "velgrad_kernels.h"
#include "port_kernels.h"
#include "slab_kernels.h"
#include "slab_rccl.h"

namespace {

std::string g_create_error;

inline int div_up(int a, int b) { return (a + b - 1) / b; }

// environment switch "NAME=1"
bool getenv_flag(const char* name)
{
   const char* v = getenv(name);
   return v && v[0] == '1';
}

// ---- owned resources -------------------------------------------------------------------------
template <class P> hipError_t release_device(P p) { return hipFree((void*)p); }
template <class P> hipError_t release_pinned(P p) { return hipHostFree((void*)p); }
hipError_t release_stream(hipStream_t s) { return hipStreamDestroy(s); }
hipError_t release_event(hipEvent_t e) { return hipEventDestroy(e); }

// One resource and its release.  Converts to the raw handle; out() lends its address to the
// call that creates it (after releasing what it held).
template <class T, hipError_t (*Release)(T)>
class Owned {
   T h_ = nullptr;

 public:
   Owned() = default;
   Owned(const Owned&) = delete;
   Owned& operator=(const Owned&) = delete;
   Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
   Owned& operator=(Owned&& o) noexcept
   {
      if (this != &o) {
         reset();
         h_ = std::exchange(o.h_, nullptr);
      }
      return *this;
   }
   ~Owned() { reset(); }
   void reset()
   {
      if (h_) (void)Release(h_);
      h_ = nullptr;
   }
   T* out()
   {
      reset();
      return &h_;
   }
   T get() const { return h_; }
   operator T() const { return h_; }
};

template <class T> using DevBuf = Owned<T*, release_device<T*>>;
template <class T> using PinnedBuf = Owned<T*, release_pinned<T*>>;
using Stream = Owned<hipStream_t, release_stream>;
using Event = Owned<hipEvent_t, release_event>;

template <class T>
hipError_t dev_alloc(DevBuf<T>& buf, size_t count)
{
   return hipMalloc(reinterpret_cast<void**>(buf.out()), count * sizeof(T));
}

template <class T>
hipError_t pinned_alloc(PinnedBuf<T>& buf, size_t count)
{
   return hipHostMalloc((void**)buf.out(), count * sizeof(T), hipHostMallocDefault);
}

hipError_t event_create(Event& ev, unsigned flags = hipEventDisableTiming)
{
   return hipEventCreateWithFlags(ev.out(), flags);
}

// Device scratch of one call, grown on demand; what it held is not kept.  reserve() makes room for
// `count` elements: a larger buffer replaces the old one only once the context's stream is idle
// (launches on it may still use the old one).  A failed wait is SPH_HIP_ERR_DEVICE; a failed
// allocation is SPH_HIP_ERR_CAPACITY with the message `capacity_err` where one is given,
// SPH_HIP_ERR_DEVICE otherwise.
template <class T>
struct Scratch {
   DevBuf<T> buf;
   size_t cap = 0;   // elements

   int reserve(sph_hip_context* ctx, size_t count, const char* capacity_err = nullptr);
   T* get() const { return buf.get(); }
   operator T*() const { return buf.get(); }
};

} // namespace

// One slab's communicator, exchange stream and message buffers (native RCCL exchange).
struct SlabComm {
   ncclComm_t comm = nullptr;
   int rank = 0, nranks = 1;
   Stream stream;                     // exchange stream (high priority)
   Event packed;                      // main stream -> exchange stream (serial exchange only)
   Event arrived;                     // exchange stream -> main stream
   DevBuf<void> send_left, send_right, recv_left, recv_right;
   int capacity_records = 0;          // what the buffers hold
   int active_records = 0;            // what messages are packed for and transferred with (<= capacity)
   size_t bytes = 0;                  // bytes of a message of active_records
   DevBuf<int32_t> trim_word;         // device int: this rank's wish, then the maximum over the ranks
   bool primed = false;               // the first ghosts have been delivered
   // trimmed messages grow BEFORE they overflow: every GROW_EVERY steps of sph_hip_slab_comm_run the
   // ranks reduce (max) the record counts of the messages they packed last, the result travels to
   // pinned host memory behind the exchange, and the look at it - GROW_EVERY steps later, at the same
   // step on every rank, because every rank holds the same number - decides for all of them alike
   long long steps_run = 0;           // steps enqueued by sph_hip_slab_comm_run so far
   DevBuf<int32_t> fill_word;         // device int: max records of this rank's two messages, then over the ranks
   PinnedBuf<int32_t> fill_host;      // pinned copy of it
   Event fill_arrived;
   bool fill_pending = false;
   int growths = 0;                   // times the messages went back to capacity_records

   // (the exchange stream has been drained: sph_hip_destroy)
   ~SlabComm()
   {
      const RcclApi* api = comm ? rccl_api(nullptr) : nullptr;
      if (api) (void)api->CommDestroy(comm);
   }
};
#define SLAB_GROW_EVERY 16

struct sph_hip_context {
   sph_hip_params prm;
   int mode = 0;
   int device = 0;
   int capacity = 0;
   int n = 0;       // host upper bound of resident entries (owned + ghosts + dead)
   int n_owned = 0; // owned particles at the last upload / count query
   DevBuf<int32_t> meta; // META_* (device)
   // slab (FULL mode): owned global z-planes [plane_lo, plane_hi), halo planes on each side
   int plane_lo = 0, plane_hi = 0, halo = 0;
   hipStream_t stream = nullptr;     // the stream every launch goes to
   Stream own_stream;                // created with the context; `stream` may be redirected
   // per-phase event ring: EV_RING steps x 7 events; `ev_steps` counts timed steps since the
   // last reset (phase totals cover the last min(ev_steps, EV_RING) of them)
   Event ev[EV_RING][7];
   long long ev_steps = 0;
   std::string err;

   CellGrid grid;

   // particle state: {x,y,z,m} and {vx,vy,vz,id-bits}.  FULL mode keeps it cell-sorted and
   // ping-pongs between the two buffers at every cell build; REF mode keeps it in index order
   // in buffer 0.
   DevBuf<float4> posm[2];
   DevBuf<float4> velp[2];
   int cur = 0;

   // cell build
   DevBuf<uint32_t> key;        // cell id per particle
   DevBuf<uint32_t> slot;       // arrival rank inside the cell (from the counting atomic)
   DevBuf<uint32_t> perm;       // cell-sorted, arbitrary order inside a cell
   DevBuf<uint32_t> order;      // REF: cell-sorted, ascending index inside a cell
   DevBuf<uint32_t> cell_count; // ncells
   DevBuf<uint32_t> cell_start; // ncells + 1
   DevBuf<uint32_t> scan_part;  // per-tile partial sums of the scan
   DevBuf<uint32_t> big_cells;  // [0] = count, then the cells with more than RANK_BIG members
   int scan_tiles = 0;

   // sums
   DevBuf<float> rho;
   DevBuf<float4> velB; // per particle {vx, vy, vz, B = p_j * rhojInv^2}: the acceleration gather
   DevBuf<float> auxc;  // per particle C = (rhojInv * m_j) * k3 (FAST: m_j * B): staged in the acceleration tile
   DevBuf<float4> acc;  // {ax, ay, az, unused}
   DevBuf<int32_t> ncount;
   DevBuf<TileDesc> tile_desc;          // per 256-particle workgroup: LDS tile layout
   DevBuf<uint32_t> nlist;              // neighbour lists density pass -> acceleration pass
   DevBuf<uint32_t> nlist_overflow;     // per workgroup: LISTS_ALL / LISTS_NONE / LISTS_SOME (neighbor_lists.h)
   int fast = 0;                   // tolerance-mode pair arithmetic (SPH_HIP_MODE_FULL_FAST / sph_hip_set_arithmetic)
   // what velB / auxc were last formed with (launch_density, k_neighbor_terms): the acceleration pass
   // of a phase call whose constants differ (a setter in between) forms them again first
   struct {
      int valid = 0;               // 0: none formed yet, or the particles have moved since (keep_sums build)
      int fast = 0;
      float rho0 = 0.0f, stiffness = 0.0f, kernel3 = 0.0f;
   } terms;
   int uniform_mass = 0;           // every resident particle has bit-identical mass
   int use_tiled = 1;              // FULL mode: LDS-tiled kernels (0 = untiled everywhere)
   int prehashed = 0;              // the last integrate also did the next build's cell hash + counts
                                   // (2: a slab's fused step - owned entries only, see k_hash_tail)
   int no_prehash = 0, no_fused_integrate = 0, no_fused_slab = 0;   // SPH_HIP_NO_* switches, read at creation
   Stream chunk_stream;            // k_full_density_chunked runs beside the tiled density pass (created on first use)
   Event ev_chunk_fork, ev_chunk_join;
   int chunked_giveups = -1;       // SPH_HIP_CHUNKED: 1 always / 0 never launch k_full_density_chunked (-1: by count)
   int slab_fused = 0;             // the step in progress (step_begin .. step_end) is fused
   void* slab_msgs[2] = {nullptr, nullptr};   // its message buffers
   int slab_msg_capacity = 0;
   int had_exchange = 0;           // pack/unpack/step_begin were used on this context: never prehash
   int may_hold_dead = 0;          // sph_hip_slab_pack has marked entries dead since the last cell build
   int early_exchange = 0;         // the last step packed its messages early (sph_hip_slab_step_begin)
   std::unique_ptr<SlabComm> comm;      // native RCCL exchange (slab_comm.h), or null
   hipStream_t border_stream = nullptr; // stream the last step_begin put the border work on
   Event ev_density;               // early exchange: density done (main stream) -> border work may start
   Event ev_border;                //                 border acceleration done (exchange stream) -> integrate may run
   Event ev_pace[2];               // recorded every PACE_STEPS steps (see pace_host)
   long long steps_enqueued = 0;
   int timing_level = 2;           // SPH_HIP_TIMING_*: which events sph_hip_step() records
   int timing_stride = 1;          // ... on every timing_stride-th step only (sph_hip_set_timing_stride)
   long long timing_seen = 0;      // timed steps since the stride was set
   int slab_step_level = 0;        // level sph_hip_slab_step_begin chose for the step in progress
   // LDS tile capacity of the two tiled kernels: chosen per launch among the largest tiles that
   // still allow B workgroups per CU (levels, ascending), from the tile size recent steps needed
   // (tile_feedback: pinned host word the density kernel stores into; 0 = nothing known yet)
   PinnedBuf<int> tile_feedback;   // TSTAT_COUNT ints, pinned host memory
   DevBuf<int32_t> tile_stats;     // TSTAT_* of the current step (device)
   DevBuf<uint32_t> giveup_density; // workgroups whose tile exceeds the density capacity
   DevBuf<uint32_t> giveup_accel;   // ... or the acceleration capacity
   int tile_cap_forced = 0;        // SPH_HIP_TILE_CAP: fixed capacity for both kernels (tests)
   int tile_cap_accel = 0, tile_cap_density = 0;   // SPH_HIP_TILE_CAP_ACCEL / _DENSITY: smaller for one pass
   int list_cap = 0;               // neighbours per particle the lists hold (even)
   int list_cap_max = 0;           // how far the host may enlarge them (SPH_HIP_LIST_CAP pins both)
   size_t list_blocks = 0;         // workgroup blocks the list allocation covers
   TileLevels density_levels = {}, accel_levels = {};
   TileCaps caps = {};             // candidate capacities + the two chosen for the current step
   int cand_kept[TILE_CANDS] = {0}, n_cand_kept = 0;   // the candidate list tile_feedback's counts belong to

   // REF-mode lists
   DevBuf<int32_t> vox; // 3 ints per particle
   DevBuf<uint32_t> nb;
   DevBuf<float> nd;

   // reductions
   DevBuf<double> epart; // 2 * blocks partial sums, then [0],[1] totals
   int eblocks = 0;
   int energy_blocks = 0;   // partials written by the last integrate (0 = none yet)
   DevBuf<int32_t> stats; // sum(lo,hi), max, min

   // error word of the slab exchange as last copied to the host (pinned; sph_hip_slab_poll_errors)
   PinnedBuf<volatile int32_t> err_watch;
   Event watch_event;                 // behind the last requested copy of the error word
   int watch_pending = 0;

   // asynchronous host mirror (sph_hip_download_async): its own device staging, copy stream and
   // events, created on first use
   DevBuf<float> mirror_stage;        // capacity * 11 floats + voxel counts
   Stream copy_stream;
   Event ev_exported;                 // compute stream: the mirror staging is complete
   Event ev_copied;                   // copy stream: it has reached the host
   int mirror_busy = 0;               // a copy has been started and not yet been seen complete

   // staging for host <-> device in the reference's interleaved layouts
   DevBuf<float> stage; // capacity * 11 floats

   // field sampler (sph_hip_sample_points / _lattice): probes and outputs of one chunk
   Scratch<float> sample_buf;
   int sample_route = 0;           // SAMPLE_ROUTE_*: SPH_HIP_SAMPLE_UNTILED=1 / SPH_HIP_SAMPLE_TILED=1 (tests, A/B runs)
   int sample_lds_set = 0;         // the tiled lattice kernels may take their dynamic LDS on this device
   int sample_chunk_forced = 0;    // SPH_HIP_SAMPLE_CHUNK=n (tests): probes per chunk, clamped (sample_chunk_forced)

   // iso-surface extractor (sph_hip_extract_surface): one slab's scratch, the running totals per
   // slab, and the kept mesh (grown on demand, kept until the next extraction or destroy)
   Scratch<unsigned char> surf_scratch;
   Scratch<unsigned long long> surf_totals;   // 4 per slab boundary (k_surf_scan)
   PinnedBuf<unsigned long long> surf_totals_host;   // 4
   DevBuf<float> surf_vtx, surf_nrm, surf_vel;
   DevBuf<int32_t> surf_tri;
   long long surf_vtx_cap = 0, surf_nrm_cap = 0, surf_vel_cap = 0, surf_tri_cap = 0;
   long long surf_nv = 0, surf_nt = 0;
   int surf_flags = 0;
   int surf_kept = 0;
   int surf_planes_forced = 0;   // SPH_HIP_SURFACE_PLANES=n (tests): planes per slab

   // renderer (sph_hip_render): one row chunk's scratch and the occupancy map (a byte per FULL cell)
   Scratch<unsigned char> render_scratch;
   Scratch<unsigned char> render_occ;
   int render_noskip = 0;   // SPH_HIP_RENDER_NOSKIP=1 (tests, A/B runs): every sample walks
   // scene renderer (sph_hip_render_scene): a chunk's solid_id, and the solids as they stand at the call
   Scratch<int32_t> scene_id;
   Scratch<SceneSolid> scene_list;
   SceneSolid scene_list_host[SPH_HIP_MAX_OBSTACLES];
   // scalar renderer (sph_hip_render_scalars): a chunk's scalar, and the colour table of the call
   Scratch<float> tint_scalar;
   Scratch<float> tint_table;
   float tint_table_host[TINT_TABLE_FLOATS];

   // static obstacles (sph_hip_set_obstacles): the list the next enqueued steps use, its device copy,
   // and the pinned staging of that copy (reused only after the event behind the last copy)
   sph_hip_obstacle obst_host[SPH_HIP_MAX_OBSTACLES];
   int n_obst = 0;
   DevBuf<sph_hip_obstacle> obst_dev;
   PinnedBuf<sph_hip_obstacle> obst_stage;
   Event ev_obst_copied;
   int obst_copy_pending = 0;
   int slab_step_open = 0;         // between sph_hip_slab_step_begin and _end (the list must not change)

   // moving obstacles (sph_hip_set_obstacle_motion): one motion per obstacle (n_motion = 0 or n_obst),
   // n_moving of them with a velocity, staged and copied like the obstacle list; the motion clock, and
   // the pair a slab's early pack took for its step (the integrate behind it uses the same)
   sph_hip_obstacle_motion motion_host[SPH_HIP_MAX_OBSTACLES];
   int n_motion = 0, n_moving = 0;
   DevBuf<sph_hip_obstacle_motion> motion_dev;
   PinnedBuf<sph_hip_obstacle_motion> motion_stage;
   Event ev_motion_copied;
   int motion_copy_pending = 0;
   float motion_tau = 0.0f;
   float step_tau[2] = {0.0f, 0.0f};
   int step_tau_taken = 0;

   // motion paths (sph_hip_set_obstacle_paths): one path per obstacle (n_path_entries = 0 or n_obst),
   // n_paths of them with keys; paths and keys are staged and copied like the motion list, their buffers
   // allocated with the context's first set.  path_shift_dev: the shifts k_paths_eval writes in front
   // of every integrate, single-buffered - the next eval is behind this step's integrate on the stream
   sph_hip_motion_path paths_host[SPH_HIP_MAX_OBSTACLES];
   std::vector<sph_hip_motion_key> path_keys_host;
   int n_path_entries = 0, n_paths = 0;
   DevBuf<sph_hip_motion_path> paths_dev;
   PinnedBuf<sph_hip_motion_path> paths_stage;
   Event ev_paths_copied;
   int paths_copy_pending = 0;
   DevBuf<sph_hip_motion_key> path_keys_dev;
   PinnedBuf<sph_hip_motion_key> path_keys_stage;
   Event ev_path_keys_copied;
   int path_keys_copy_pending = 0;
   DevBuf<PathShift> path_shift_dev;

   // load recording (sph_hip_record_loads): loads_rows rows of LOAD_ROW_WORDS int64, the next integrate
   // enqueued fills row loads_next (load_row below)
   DevBuf<unsigned long long> loads_dev;
   int loads_rows = 0, loads_next = 0;
   int loads_quantum = LOAD_QUANTUM_DEFAULT;

   // free bodies (sph_hip_set_bodies): one entry per obstacle (n_body_entries = 0 or n_obst), n_bodies of
   // them with a mass; the list and the initial state are staged and copied like the obstacle list.  The
   // state lives on the device (k_bodies_advance).  body_rows: the two internal load rows, used alternately
   // when no recording has rows left (body_flip: the one last filled); body_last_row: the row the last
   // integrate enqueued filled - the caller's or an internal one - or null before the first
   sph_hip_body bodies_host[SPH_HIP_MAX_OBSTACLES];
   int n_body_entries = 0, n_bodies = 0;
   int body_quantum = LOAD_QUANTUM_DEFAULT;
   DevBuf<sph_hip_body> bodies_dev;
   PinnedBuf<sph_hip_body> bodies_stage;
   Event ev_bodies_copied;
   int bodies_copy_pending = 0;
   DevBuf<BodyState> body_state_dev;
   PinnedBuf<BodyState> body_state_stage;
   Event ev_body_state_copied;
   int body_state_copy_pending = 0;
   DevBuf<unsigned long long> body_rows;
   int body_flip = 0;
   const unsigned long long* body_last_row = nullptr;

   // tracers (sph_hip_set_tracers): n_tracers slots {x, y, z, id} and {wet, dry} in pair tr_cur of two (the
   // sort moves them to the other pair); the sort's scratch - per-slot key and rank, the cells' counts padded
   // to whole scan tiles, the tiles' totals - allocated with the set when it is kept sorted; advances since
   // the last sort, counted here so that nothing is read back
   int n_tracers = 0;
   DevBuf<float4> tr_xi[2];
   DevBuf<int2> tr_cnt[2];
   int tr_cur = 0;
   DevBuf<uint32_t> tr_key, tr_rank, tr_cells, tr_part;
   int tracer_sort_switch = -1;    // SPH_HIP_TRACER_SORT (tracer_policy.h: tracer_sort_switch), read at creation
   long long tr_since_sort = 0;
   // recording (sph_hip_record_tracers): trec_rows rows of 3 * n_tracers floats; trec_step = steps advanced
   // since the call, trec_filled = rows those steps have filled
   DevBuf<float> trec_dev;
   int trec_rows = 0, trec_every = 1, trec_filled = 0;
   long long trec_step = 0;

   // gauges (sph_hip_set_gauges): the descriptors as given (gauges_host) and on the device, and the row
   // sph_hip_read_gauges evaluates into
   int n_gauges = 0;
   std::unique_ptr<sph_hip_gauge[]> gauges_host;
   DevBuf<sph_hip_gauge> gauges_dev;
   DevBuf<sph_hip_gauge_reading> gauge_now;
   // how many of them each kernel reads (gauge_policy.h: gauge_set_counts)
   int n_gauges_field = 0, n_gauges_pressure = 0;
   // the pressure kinds and samplers outside a step: the densities of the current sorted state, f32[capacity]
   // (k_particle_density), allocated at the first use
   DevBuf<float> rho_own;
   // recording (sph_hip_record_gauges): grec_rows rows of one reading per gauge; grec_step = steps enqueued
   // since the call, grec_filled = rows those steps have filled
   DevBuf<sph_hip_gauge_reading> grec_dev;
   int grec_rows = 0, grec_every = 1, grec_filled = 0;
   long long grec_step = 0;
   int grec_row_now = -1;   // the row the step being enqueued fills (its pressure kinds follow its density pass)

   // carried scalars (sph_hip_set_scalars): n_scalars rows of four channels by particle ID (scalar_T), and the
   // stage of a step or a sampler call by sorted slot - the channels (scalar_Ts) and the volumes m / rho
   // (scalar_Vs); all three hold the capacity and are allocated at the first set.  The diffusivities and the
   // sources go to a pass by value.
   int n_scalars = 0;
   DevBuf<float4> scalar_T, scalar_Ts;
   DevBuf<float> scalar_Vs;
   float scalar_kappa[SPH_HIP_SCALAR_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f};
   int n_scalar_sources = 0;
   sph_hip_scalar_source scalar_sources[SPH_HIP_MAX_SCALAR_SOURCES];
   int scalar_force_rows = 0;      // SPH_HIP_SCALAR_ROWS=1, read at creation: every workgroup of the pass walks the rows

   // buoyancy (sph_hip_set_buoyancy): the setting the next enqueued steps take by value; dropped with the scalars
   int have_buoyancy = 0;
   sph_hip_buoyancy buoyancy = {};

   // cohesion (sph_hip_set_cohesion): the gamma the next enqueued steps take by value; dropped by an upload
   int have_cohesion = 0;
   float cohesion_gamma = 0.0f;

   // xsph (sph_hip_set_xsph): the eps the next enqueued steps take by value, dropped by an upload; the staged rows
   // {v, 1 / rho} by sorted slot (xsph_R) hold the capacity and are allocated at the first non-zero setting
   int have_xsph = 0;
   float xsph_eps = 0.0f;
   DevBuf<float4> xsph_R;

   // viscous stress (sph_hip_set_viscous_stress): the mu and the law the next enqueued steps take by value, dropped
   // by an upload (the law also with the scalars); the staged rows {v, m / rho} by sorted slot (viscous_R) and, with a
   // law, the staged viscosities (viscous_M) hold the capacity: allocated at the first non-zero mu and the first law
   int have_viscous = 0, have_viscous_law = 0;
   float viscous_mu = 0.0f;
   sph_hip_viscosity_law viscous_law = {};
   DevBuf<float4> viscous_R;
   DevBuf<float> viscous_M;

   // implicit viscous stress (sph_hip_set_viscous_implicit): the Jacobi sweeps the next enqueued steps take in the
   // place of the explicit term while mu != 0 (0: the explicit term), dropped by an upload; the second row set of the
   // ping-pong (viscous_R2) holds the capacity and is allocated by the first count of 2 or more
   int viscous_sweeps = 0;
   DevBuf<float4> viscous_R2;

   // step monitor (sph_hip_record_monitor): mon_rows rows; mon_step = steps enqueued since the call, mon_filled =
   // rows those steps have filled, mon_row_now = the row the step being enqueued fills (-1: none).  The partial
   // rows of the particle kernel's bounded grid and of the pair pass's workgroups (one per 256 particles of the
   // capacity) are allocated with the recording; queued steps reuse them in stream order.
   DevBuf<sph_hip_monitor_row> mon_dev;
   DevBuf<MonitorAcc> mon_part;
   DevBuf<MonitorPairAcc> mon_pair_part;
   int mon_rows = 0, mon_every = 1, mon_filled = 0, mon_quantum = LOAD_QUANTUM_DEFAULT;
   long long mon_step = 0;
   int mon_row_now = -1;

   // velocity gradients (sph_hip_get_velocity_gradients and its samplers and renderer): the two rows of every sorted
   // slot, (w_x, w_y, w_z, div) and (strain, Q, |w|, valid); both hold the capacity and are allocated at the first
   // call.  Nothing is cached: every call forms them anew behind its cell build.
   DevBuf<float4> velgrad_A, velgrad_B;

   // ports (sph_hip_set_ports): the lists the next enqueued steps use, staged and copied like the obstacle
   // list; the schedule (port steps taken, layers fired per emitter), the id the next new particle gets, the
   // emitted totals (host-known) and the removed totals (device, one int64 per sink)
   sph_hip_emitter emit_host[SPH_HIP_MAX_EMITTERS];
   sph_hip_sink sink_host[SPH_HIP_MAX_SINKS];
   int n_emit = 0, n_sink = 0;
   DevBuf<sph_hip_emitter> emit_dev;
   PinnedBuf<sph_hip_emitter> emit_stage;
   Event ev_emit_copied;
   int emit_copy_pending = 0;
   DevBuf<sph_hip_sink> sink_dev;
   PinnedBuf<sph_hip_sink> sink_stage;
   Event ev_sink_copied;
   int sink_copy_pending = 0;
   DevBuf<unsigned long long> removed_dev;   // SPH_HIP_MAX_SINKS
   long long port_step = 0;
   long long port_fired[SPH_HIP_MAX_EMITTERS] = {0};
   long long port_emitted[SPH_HIP_MAX_EMITTERS] = {0};
   uint32_t next_id = 0;
   int ports_seen = 0;        // ports have been set since the creation: counts are read from the device
   int ids_changed = 0;       // a step with a sink or a firing emitter since the last upload: ids are not 0..n-1
   int n_in_stale = 0;        // meta[META_N_IN] is what the last port step's build read, not n_live
   // the uploaded masses, for the uniform-mass rule with emitters: known (host masses were given), and the
   // first one - the value of them all while uniform_mass holds
   int upload_mass_known = 0;
   float upload_mass = 0.0f;
};

namespace {

template <class T>
int Scratch<T>::reserve(sph_hip_context* ctx, size_t count, const char* capacity_err)
{
   if (count <= cap) return SPH_HIP_OK;
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   buf.reset();
   cap = 0;
   if (!capacity_err) {
      SPH_TRY(dev_alloc(buf, count));
   } else if (dev_alloc(buf, count) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = capacity_err;
      return SPH_HIP_ERR_CAPACITY;
   }
   cap = count;
   return SPH_HIP_OK;
}

// whether the next integrate enqueued fills a row of the load recording
bool loads_pending(const sph_hip_context* ctx) { return ctx->loads_next < ctx->loads_rows; }

int check_ctx(sph_hip_context* ctx)
{
   if (!ctx) return SPH_HIP_ERR_INVALID;
   hipError_t e = hipSetDevice(ctx->device);
   if (e != hipSuccess) {
      ctx->err = std::string("hipSetDevice: ") + hipGetErrorString(e);
      return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}

int create_impl(sph_hip_context** out, const sph_hip_params* params, int capacity, int mode,
                int device, int plane_lo, int plane_hi, int halo)
{
   if (!out || !params || capacity < 1 ||
       (mode != SPH_HIP_MODE_REF && mode != SPH_HIP_MODE_FULL && mode != SPH_HIP_MODE_FULL_FAST)) {
      g_create_error = "sph_hip_create: invalid argument";
      return SPH_HIP_ERR_INVALID;
   }
   // REF mode: the search stores up to 4 neighbours per chunk and stops once more than
   // examine_count - 8 are stored (ref_kernels.h), so a list of fewer than 4 entries overflows in
   // its first chunk
   if (mode == SPH_HIP_MODE_REF && params->examine_count < SPH_HIP_MIN_EXAMINE_COUNT) {
      g_create_error = "sph_hip_create: examine_count must be at least " +
                       std::to_string(SPH_HIP_MIN_EXAMINE_COUNT) + " in REF mode (the search's largest chunk)";
      return SPH_HIP_ERR_INVALID;
   }
   // FULL with the tolerance-mode pair arithmetic (SPH_HIP_ARITH=fast: experiments run the tools
   // that create plain FULL contexts - A/B, ablation, slab cost - in that mode)
   // - only together with SPH_HIP_ALLOW_DIAGNOSTIC=1, which those tools set: a variable left over
   // in a shell must not turn the bit-exact gates and bench.py's exact record into FAST runs)
   const char* arith_env = getenv_flag("SPH_HIP_ALLOW_DIAGNOSTIC") ? getenv("SPH_HIP_ARITH") : nullptr;
   const bool fast = mode == SPH_HIP_MODE_FULL_FAST ||
                     (mode == SPH_HIP_MODE_FULL && arith_env && strcmp(arith_env, "fast") == 0);
   if (fast) mode = SPH_HIP_MODE_FULL;
   *out = nullptr;
   int ndev = 0;
   hipError_t e = hipGetDeviceCount(&ndev);
   if (e != hipSuccess || ndev == 0 || device < 0 || device >= ndev) {
      g_create_error = "sph_hip_create: no usable HIP device (" +
                       std::string(e != hipSuccess ? hipGetErrorString(e) : "device index out of range") + ")";
      return SPH_HIP_ERR_NO_DEVICE;
   }
   std::unique_ptr<sph_hip_context> ctx(new (std::nothrow) sph_hip_context());
   if (!ctx) return SPH_HIP_ERR_INVALID;
   ctx->prm = *params;
   ctx->mode = mode;
   ctx->fast = fast ? 1 : 0;
   // diagnostic switches, read once per context (not once per step)
   ctx->no_prehash = getenv_flag("SPH_HIP_NO_PREHASH");
   ctx->no_fused_integrate = getenv_flag("SPH_HIP_NO_FUSED_INTEGRATE");
   ctx->no_fused_slab = getenv_flag("SPH_HIP_NO_FUSED_SLAB");
   if (const char* v = getenv("SPH_HIP_CHUNKED")) ctx->chunked_giveups = v[0] == '1' ? 1 : 0;   // default: by count
   ctx->sample_route = getenv_flag("SPH_HIP_SAMPLE_UNTILED") ? SAMPLE_ROUTE_UNTILED
                       : getenv_flag("SPH_HIP_SAMPLE_TILED")  ? SAMPLE_ROUTE_TILED
                                                              : SAMPLE_ROUTE_DEFAULT;
   if (const char* v = getenv("SPH_HIP_SAMPLE_CHUNK")) ctx->sample_chunk_forced = sample_chunk_forced(atoll(v));
   if (const char* v = getenv("SPH_HIP_SURFACE_PLANES")) ctx->surf_planes_forced = atoi(v) > 0 ? atoi(v) : 0;
   ctx->render_noskip = getenv_flag("SPH_HIP_RENDER_NOSKIP");
   ctx->tracer_sort_switch = tracer_sort_switch(getenv("SPH_HIP_TRACER_SORT"));
   ctx->scalar_force_rows = getenv_flag("SPH_HIP_SCALAR_ROWS");
   ctx->device = device;
   ctx->capacity = capacity;

   CellGrid& g = ctx->grid;
   if (mode == SPH_HIP_MODE_REF) {
      g.nx = params->cells_x; g.ny = params->cells_y; g.nz_global = params->cells_z;
      g.inv = params->htimes2inv;
   } else {
      g.nx = params->full_cells_x; g.ny = params->full_cells_y; g.nz_global = params->full_cells_z;
      g.inv = params->full_cell_inv;
   }
   if (plane_hi < 0) plane_hi = g.nz_global;  // whole grid
   if (g.nx < 1 || g.ny < 1 || g.nz_global < 1 || plane_lo < 0 || plane_hi > g.nz_global ||
       plane_lo >= plane_hi || (mode == SPH_HIP_MODE_REF && (plane_lo != 0 || plane_hi != g.nz_global))) {
      g_create_error = "sph_hip_create: bad grid shape or slab range";
      return SPH_HIP_ERR_INVALID;
   }
   // A slab with a neighbour feeds that neighbour's `halo` ghost planes from its own planes, and
   // the ghost planes of the two sides must not overlap in what they send: 2 * halo planes at
   // least (slab.plan_cuts plans with the same minimum).  A thinner slab would leave its
   // neighbour's ghosts incomplete without any error bit being raised.
   if (halo > 0 && (plane_lo > 0 || plane_hi < g.nz_global) && plane_hi - plane_lo < 2 * halo) {
      g_create_error = "sph_hip_create_slab: a slab next to another needs at least 2 * SPH_HIP_SLAB_HALO planes";
      return SPH_HIP_ERR_INVALID;
   }
   ctx->plane_lo = plane_lo;
   ctx->plane_hi = plane_hi;
   ctx->halo = halo;
   // planes held: the owned ones plus `halo` ghost planes on each side, clipped to the grid
   g.z0 = plane_lo - halo < 0 ? 0 : plane_lo - halo;
   const int z1 = plane_hi + halo > g.nz_global ? g.nz_global : plane_hi + halo;
   g.nz = z1 - g.z0;
   const long long ncells = (long long)g.nx * g.ny * g.nz;
   if (ncells > 0x7fff0000ll) {
      g_create_error = "sph_hip_create: grid too large";
      return SPH_HIP_ERR_INVALID;
   }
   g.ncells = (int)ncells;
   ctx->scan_tiles = div_up(g.ncells + 1, SCAN_TILE);
   ctx->eblocks = div_up(capacity, RED_THREADS);

#define CREATE_TRY(expr)                                                     \
   do {                                                                      \
      hipError_t e_ = (expr);                                                \
      if (e_ != hipSuccess) {                                                \
         g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_); \
         return SPH_HIP_ERR_DEVICE;                                          \
      }                                                                      \
   } while (0)

   CREATE_TRY(hipSetDevice(device));
   CREATE_TRY(hipStreamCreateWithFlags(ctx->own_stream.out(), hipStreamNonBlocking));
   ctx->stream = ctx->own_stream;
   for (auto& slot : ctx->ev)
      for (Event& ev : slot) CREATE_TRY(hipEventCreate(ev.out()));
   for (int k = 0; k < 2; k++) CREATE_TRY(event_create(ctx->ev_pace[k]));
   const size_t cap = (size_t)capacity;
   const int nbuf = (mode == SPH_HIP_MODE_FULL) ? 2 : 1;
   for (int b = 0; b < nbuf; b++) {
      CREATE_TRY(dev_alloc(ctx->posm[b], cap));
      CREATE_TRY(dev_alloc(ctx->velp[b], cap));
   }
   CREATE_TRY(dev_alloc(ctx->key, cap));
   CREATE_TRY(dev_alloc(ctx->slot, cap));
   CREATE_TRY(dev_alloc(ctx->perm, cap));
   // cell arrays padded to whole scan tiles so vector accesses never run off the end
   const size_t cells_padded = (size_t)ctx->scan_tiles * SCAN_TILE + 16;
   CREATE_TRY(dev_alloc(ctx->cell_count, cells_padded));
   CREATE_TRY(dev_alloc(ctx->cell_start, cells_padded));
   CREATE_TRY(dev_alloc(ctx->scan_part, (size_t)ctx->scan_tiles + 1));
   CREATE_TRY(dev_alloc(ctx->big_cells, cap / RANK_BIG + 2));
   CREATE_TRY(hipMemsetAsync(ctx->big_cells, 0, sizeof(uint32_t), ctx->stream));
   CREATE_TRY(hipMemsetAsync(ctx->cell_count, 0, cells_padded * sizeof(uint32_t), ctx->stream));
   CREATE_TRY(hipMemsetAsync(ctx->cell_start, 0, cells_padded * sizeof(uint32_t), ctx->stream));
   CREATE_TRY(dev_alloc(ctx->rho, cap));
   CREATE_TRY(dev_alloc(ctx->acc, cap));
   CREATE_TRY(dev_alloc(ctx->ncount, cap));
   CREATE_TRY(hipMemsetAsync(ctx->rho, 0, cap * sizeof(float), ctx->stream));
   CREATE_TRY(hipMemsetAsync(ctx->acc, 0, cap * sizeof(float4), ctx->stream));
   CREATE_TRY(hipMemsetAsync(ctx->ncount, 0, cap * sizeof(int32_t), ctx->stream));
   CREATE_TRY(dev_alloc(ctx->meta, META_COUNT));
   CREATE_TRY(hipMemsetAsync(ctx->meta, 0, META_COUNT * sizeof(int32_t), ctx->stream));
   if (mode == SPH_HIP_MODE_FULL) {
      CREATE_TRY(dev_alloc(ctx->velB, cap));
      CREATE_TRY(dev_alloc(ctx->auxc, cap));
      CREATE_TRY(dev_alloc(ctx->tile_desc, (size_t)div_up(capacity, TILE_THREADS) + 1));
      ctx->list_cap = NLIST_CAP;
      ctx->list_cap_max = NLIST_CAP_MAX;
      if (const char* v = getenv("SPH_HIP_LIST_CAP")) {
         const int c = atoi(v) / 2 * 2;
         if (c > 0) ctx->list_cap = ctx->list_cap_max = c < 2 ? 2 : (c > NLIST_CAP_MAX ? NLIST_CAP_MAX : c);
      }
      ctx->list_blocks = (size_t)div_up(capacity, TILE_THREADS) + 1;
      const size_t nlist_words = ctx->list_blocks * list_rows(ctx->list_cap) * TILE_THREADS;
      CREATE_TRY(dev_alloc(ctx->nlist, nlist_words));
      // touched once here, so that the first step does not pay for mapping the pages
      CREATE_TRY(hipMemsetAsync(ctx->nlist, 0, nlist_words * sizeof(uint32_t), ctx->stream));
      CREATE_TRY(dev_alloc(ctx->nlist_overflow, (size_t)div_up(capacity, TILE_THREADS) + 1));
      if (const char* v = getenv("SPH_HIP_UNTILED")) ctx->use_tiled = (v[0] == '1') ? 0 : 1;
      CREATE_TRY(pinned_alloc(ctx->tile_feedback, TSTAT_COUNT));
      memset(ctx->tile_feedback, 0, TSTAT_COUNT * sizeof(int));
      CREATE_TRY(dev_alloc(ctx->tile_stats, TSTAT_COUNT));
      CREATE_TRY(hipMemsetAsync(ctx->tile_stats, 0, TSTAT_COUNT * sizeof(int32_t), ctx->stream));
      CREATE_TRY(dev_alloc(ctx->giveup_density, (size_t)div_up(capacity, TILE_THREADS) + 1));
      CREATE_TRY(dev_alloc(ctx->giveup_accel, (size_t)div_up(capacity, TILE_THREADS) + 1));
      CREATE_TRY(event_create(ctx->ev_density));
      CREATE_TRY(event_create(ctx->ev_border));
      if (const char* v = getenv("SPH_HIP_TILE_CAP")) {
         const int c = atoi(v);
         if (c > 0) ctx->tile_cap_forced = c < 256 ? 256 : (c > 8000 ? 8000 : c / 32 * 32);  // 128 KiB at most
      }
      // (a smaller forced capacity for one pass alone: launch_policy.h, choose_caps)
      if (const char* v = getenv("SPH_HIP_TILE_CAP_ACCEL")) ctx->tile_cap_accel = atoi(v) / 32 * 32;
      if (const char* v = getenv("SPH_HIP_TILE_CAP_DENSITY")) ctx->tile_cap_density = atoi(v) / 32 * 32;
   } else {
      CREATE_TRY(dev_alloc(ctx->order, cap));
      CREATE_TRY(dev_alloc(ctx->vox, cap * 3));
      CREATE_TRY(dev_alloc(ctx->nb, cap * (size_t)params->examine_count));
      CREATE_TRY(dev_alloc(ctx->nd, cap * (size_t)params->examine_count));
   }
   CREATE_TRY(dev_alloc(ctx->epart, (size_t)2 * ctx->eblocks + 2));
   CREATE_TRY(hipMemsetAsync(ctx->epart, 0, sizeof(double) * 2, ctx->stream));
   CREATE_TRY(dev_alloc(ctx->stats, 4));
   CREATE_TRY(pinned_alloc(ctx->err_watch, 4));
   for (int i = 0; i < 4; i++) ctx->err_watch[i] = 0;
   CREATE_TRY(event_create(ctx->watch_event));
   CREATE_TRY(dev_alloc(ctx->stage, cap * 12));
   CREATE_TRY(dev_alloc(ctx->obst_dev, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(pinned_alloc(ctx->obst_stage, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(event_create(ctx->ev_obst_copied));
   CREATE_TRY(dev_alloc(ctx->motion_dev, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(pinned_alloc(ctx->motion_stage, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(event_create(ctx->ev_motion_copied));
   CREATE_TRY(dev_alloc(ctx->bodies_dev, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(pinned_alloc(ctx->bodies_stage, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(event_create(ctx->ev_bodies_copied));
   CREATE_TRY(dev_alloc(ctx->body_state_dev, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(pinned_alloc(ctx->body_state_stage, SPH_HIP_MAX_OBSTACLES));
   CREATE_TRY(event_create(ctx->ev_body_state_copied));
   CREATE_TRY(dev_alloc(ctx->body_rows, 2 * LOAD_ROW_WORDS));
   CREATE_TRY(dev_alloc(ctx->emit_dev, SPH_HIP_MAX_EMITTERS));
   CREATE_TRY(pinned_alloc(ctx->emit_stage, SPH_HIP_MAX_EMITTERS));
   CREATE_TRY(event_create(ctx->ev_emit_copied));
   CREATE_TRY(dev_alloc(ctx->sink_dev, SPH_HIP_MAX_SINKS));
   CREATE_TRY(pinned_alloc(ctx->sink_stage, SPH_HIP_MAX_SINKS));
   CREATE_TRY(event_create(ctx->ev_sink_copied));
   CREATE_TRY(dev_alloc(ctx->removed_dev, SPH_HIP_MAX_SINKS));
   CREATE_TRY(hipMemsetAsync(ctx->removed_dev, 0, SPH_HIP_MAX_SINKS * sizeof(unsigned long long), ctx->stream));
   CREATE_TRY(hipStreamSynchronize(ctx->stream));
#undef CREATE_TRY
   *out = ctx.release();
   return SPH_HIP_OK;
}

// Drain every stream the context's resources are used on, then release them all (the
// handles): the comm stream before the communicator goes, the chunk and copy streams before
// the buffers they read and write.
void destroy_impl(sph_hip_context* ctx)
{
   (void)hipSetDevice(ctx->device);
   if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
   if (ctx->comm && ctx->comm->stream) (void)hipStreamSynchronize(ctx->comm->stream);
   if (ctx->chunk_stream) (void)hipStreamSynchronize(ctx->chunk_stream);
   if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
   delete ctx;
}

} // namespace

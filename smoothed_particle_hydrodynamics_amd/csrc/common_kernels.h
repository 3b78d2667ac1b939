// Kernels shared by both modes: integrate (+ energy totals), host-layout import/export,
// neighbour-count statistics.
#pragma once

#include "body_policy.h"
#include "cell_build.h"
#include "load_policy.h"
#include "obstacle_policy.h"
#include "pair_math.h"

#define RED_THREADS 256

// The wall response of the kernels without a hook, the integrate fused into k_full_accel_lists among
// them: load_walls_respond (load_policy.h) with LoadNoRecorder operation for operation, kept as written
// because calling that function here changed k_full_accel_lists' code (tools/kernel_isa_diff.py).
// SPH::applyBoundary (reference src/sph.cpp:1124-1148): reflect at a wall with unit normal
// along `axis` (sign sgn), continue for the rest of the step scaled by mDamping.  vec3
// operators of the reference are component-wise fp32 operations.
__device__ __forceinline__ void apply_boundary(const PairConsts& k, const float pos[3], float dt,
                                               float np[3], float dist, int axis, float sgn,
                                               float nv[3])
{
   float normal[3] = {0.0f, 0.0f, 0.0f};
   normal[axis] = sgn;
   float inter[3], refl[3];
#pragma unroll
   for (int c = 0; c < 3; c++) inter[c] = pos[c] + (nv[c] * dist);
   const float dot = nv[0] * normal[0] + nv[1] * normal[1] + nv[2] * normal[2];
#pragma unroll
   for (int c = 0; c < 3; c++) refl[c] = nv[c] - ((normal[c] * dot) * 2.0f);
   const float remaining = dt - dist;
#pragma unroll
   for (int c = 0; c < 3; c++) {
      nv[c] = refl[c];
      np[c] = inter[c] + refl[c] * (remaining * k.damping);
   }
}

// SPH::handleBoundaryConditions (reference src/sph.cpp:1025-1121): x, then y, then z.
__device__ __forceinline__ void handle_boundaries(const PairConsts& k, const float pos[3],
                                                  float nv[3], float dt, float np[3])
{
   const float maxv[3] = {k.max_x, k.max_y, k.max_z};
#pragma unroll
   for (int axis = 0; axis < 3; axis++) {
      if (np[axis] < 0.0f)
         apply_boundary(k, pos, dt, np, -pos[axis] / nv[axis], axis, 1.0f, nv);
      else if (np[axis] > maxv[axis])
         apply_boundary(k, pos, dt, np, (maxv[axis] - pos[axis]) / nv[axis], axis, -1.0f, nv);
   }
}

// ---- integrate (reference src/sph.cpp:937-1022) -------------------------------------------------
// "KDK as coded": half kick with the SPH acceleration, drift, then a FULL-dt kick with the
// point-mass gravity only, evaluated at the new position (reference src/sph.cpp:937-1022).
// Updates x (position, mass kept) and v (velocity, id kept); ke/pe = the particle's energy terms.
// A hook is what a context adds to the step of one particle of mass m, two calls:
//   walls(k, pos, nv, dt, np, m)   the wall handling (only where k.apply_walls),
//   after(pos, nv, np, m)          on (old position, new velocity, new position) after the walls and
//                                  before the energy terms.
// Hook::active: after() does something.  Hook::records: every lane of the wave must make both calls,
// the lanes without a particle too (integrate_block).
struct NoHook {
   static constexpr bool active = false;
   static constexpr bool records = false;
   __device__ void walls(const PairConsts& k, const float* pos, float* nv, float dt, float* np, float) const { handle_boundaries(k, pos, nv, dt, np); }
   __device__ void after(const float*, float*, float*, float) const {}
};
template <bool UNIT_SCALE, class Hook>
__device__ __forceinline__ void integrate_particle_hooked(const PairConsts& k, float4& x, float4& v,
                                                   const float4 a, double& ke, double& pe,
                                                   const Hook hook)
{
   const float dt = k.dt;
   const float pos_dt = dt * k.sim_scale_inv;

   const float vhx = v.x + (a.x * dt * 0.5f);
   const float vhy = v.y + (a.y * dt * 0.5f);
   const float vhz = v.z + (a.z * dt * 0.5f);
   const float nx0 = x.x + (vhx * pos_dt);
   const float ny0 = x.y + (vhy * pos_dt);
   const float nz0 = x.z + (vhz * pos_dt);

   // (k.skip_point_mass: tolerance mode without a point mass - the term is +-0 or NaN, see
   // point_mass_nan; d3 then only divides a potential energy of exactly zero, or one of a particle
   // whose new velocity is NaN and whose energy terms are not summed)
   float agx = 0.0f, agy = 0.0f, agz = 0.0f, d3 = 1.0f;
   if (!k.skip_point_mass) {
      float rsx = (nx0 - k.cx), rsy = (ny0 - k.cy), rsz = (nz0 - k.cz);
      if (!UNIT_SCALE) {
         rsx *= k.sim_scale;
         rsy *= k.sim_scale;
         rsz *= k.sim_scale;
      }
      float dot = rsx * rsx + rsy * rsy + rsz * rsz;
      dot = sqrtf(dot);
      const float ds = dot + k.softening;
      d3 = ds * ds * ds;
      const float gm = -k.grav_const * k.central_mass;
      agx = gm * (rsx / d3);
      agy = gm * (rsy / d3);
      agz = gm * (rsz / d3);
   } else {
      float rsx = (nx0 - k.cx), rsy = (ny0 - k.cy), rsz = (nz0 - k.cz);
      if (!UNIT_SCALE) {
         rsx *= k.sim_scale;
         rsy *= k.sim_scale;
         rsz *= k.sim_scale;
      }
      const float nan_any = point_mass_nan(rsx, rsy, rsz);   // 0, or NaN where the term is
      agx = (rsx - rsx) + nan_any;
      agy = (rsy - rsy) + nan_any;
      agz = (rsz - rsz) + nan_any;
   }
   if (k.apply_gravity) { // extension, as in accel_end
      agx += k.gx;
      agy += k.gy;
      agz += k.gz;
   }
   float nvx = vhx + (agx * dt);
   float nvy = vhy + (agy * dt);
   float nvz = vhz + (agz * dt);
   float nx = nx0, ny = ny0, nz = nz0;
   if (k.apply_walls || Hook::active) {
      const float pos[3] = {x.x, x.y, x.z};
      float nv[3] = {nvx, nvy, nvz}, np[3] = {nx, ny, nz};
      if (k.apply_walls) hook.walls(k, pos, nv, dt, np, x.w); // extension: the reference's own (unwired) wall handling
      hook.after(pos, nv, np, x.w);
      nvx = nv[0]; nvy = nv[1]; nvz = nv[2];
      nx = np[0]; ny = np[1]; nz = np[2];
   }

   const float dot = nvx * nvx + nvy * nvy + nvz * nvz;
   ke = 0.0;
   pe = 0.0;
   if (dot > 0) {
      ke = (double)(0.5f * x.w * dot);
      pe = -(double)(k.grav_const * k.central_mass * x.w / d3);
   }
   x.x = nx; x.y = ny; x.z = nz;
   v.x = nvx; v.y = nvy; v.z = nvz;
}

// Static obstacles (obstacle_policy.h) from a device list: every lane reads the same entries, field
// by field where the kind needs them.  (Copying each entry whole first - one batch of scalar loads per
// obstacle - measured slower: 2.03x instead of 1.30x the obstacle-free step with 64 obstacles.)
struct ObstacleHook {
   static constexpr bool active = true;
   static constexpr bool records = false;
   const sph_hip_obstacle* list;
   int n;
   float dt, damping;
   __device__ void walls(const PairConsts& k, const float* pos, float* nv, float dt_, float* np, float m) const
   {
      const float maxv[3] = {k.max_x, k.max_y, k.max_z};
      load_walls_respond(maxv, k.damping, pos, nv, dt_, np, m, LoadNoRecorder());
   }
   __device__ void after(const float* p, float* v, float* q, float) const
   {
      obstacles_respond(list, n, p, v, q, dt, damping);
   }
};

// Load recording (load_policy.h; sph_hip_record_loads): the wall and obstacle responses of
// load_policy.h with this hook as their recorder.  Every lane of the wave calls the recorder for every
// solid in turn (integrate_block keeps the lanes without a particle in step, live = false), so
// the solid is wave-uniform: one vote, and only where some lane was hit a wave reduction of the three
// terms and the two counters and one 64-bit atomic add per non-zero sum into the step's row.
struct LoadHook {
   static constexpr bool active = true;
   static constexpr bool records = true;
   const sph_hip_obstacle* list;
   int n;
   float dt, damping;
   unsigned long long* row;   // LOAD_ROW_WORDS words of this step
   double scale;              // load_scale(quantum_log2)
   bool live;
   __device__ void operator()(int s, bool hit, float m, const float* vb, const float* va) const
   {
      hit = hit && live;
      if (!__any(hit)) return;
      long long sum[5] = {0, 0, 0, 0, 0};   // the term, count, skipped
      if (hit) {
         if (load_term(m, vb, va, scale, sum)) sum[3] = 1;
         else sum[4] = 1;
      }
#pragma unroll
      for (int d = SPH_WAVE / 2; d > 0; d >>= 1) {
#pragma unroll
         for (int i = 0; i < 5; i++) sum[i] += __shfl_down(sum[i], d);
      }
      if ((threadIdx.x & (SPH_WAVE - 1)) == 0) {
#pragma unroll
         for (int c = 0; c < 3; c++)
            if (sum[c] != 0) atomicAdd(row + 3 * s + c, (unsigned long long)sum[c]);
         if (sum[3] != 0) atomicAdd(row + LOAD_ROW_COUNT + s, (unsigned long long)sum[3]);
         if (sum[4] != 0) atomicAdd(row + LOAD_ROW_SKIPPED + s, (unsigned long long)sum[4]);
      }
   }
   __device__ void walls(const PairConsts& k, const float* pos, float* nv, float dt_, float* np, float m) const
   {
      const float maxv[3] = {k.max_x, k.max_y, k.max_z};
      load_walls_respond(maxv, k.damping, pos, nv, dt_, np, m, *this);
   }
   __device__ void after(const float* p, float* v, float* q, float m) const
   {
      load_obstacles_respond(list, n, p, v, q, dt, damping, m, *this);
   }
};

// The two hooks above for a list in which some entry moves (obstacle_policy.h: moving obstacles): the
// motion list is a second device buffer read wave-uniformly, tau0 and tau1 - the motion clock at the
// start and the end of this step - are kernel arguments, and every lane forms the same shifts from them
// (9 adds per moving obstacle); no device state is written for it.  Only after() differs.
struct MovingObstacleHook : ObstacleHook {
   const sph_hip_obstacle_motion* motion;
   float tau0, tau1;
   __device__ void after(const float* p, float* v, float* q, float) const
   {
      obstacles_respond_moving(list, motion, n, p, v, q, dt, damping, tau0, tau1);
   }
};

struct MovingLoadHook : LoadHook {
   const sph_hip_obstacle_motion* motion;
   float tau0, tau1;
   __device__ void after(const float* p, float* v, float* q, float m) const
   {
      load_obstacles_respond_moving(list, motion, n, p, v, q, dt, damping, tau0, tau1, m,
                                    static_cast<const LoadHook&>(*this));
   }
};

// MovingLoadHook for a list with free bodies (body_policy.h): an entry takes the body turn with the
// shifts its BodyState holds (written by k_bodies_advance earlier on the stream, read wave-uniformly), the
// turn of its motion (`motion` is null when no motions are set), or the static turn.  Only after() differs.
struct BodyLoadHook : LoadHook {
   const sph_hip_obstacle_motion* motion;
   float tau0, tau1;
   const sph_hip_body* bodies;
   const BodyState* state;
   __device__ void after(const float* p, float* v, float* q, float m) const
   {
      body_obstacles_respond(list, motion, bodies, state, n, p, v, q, dt, damping, tau0, tau1, m,
                             static_cast<const LoadHook&>(*this));
   }
};

// The obstacle and load hooks for a list with motion paths (obstacle_policy.h, fourth part): an entry
// takes the path turn with the two shifts its PathShift holds (written by k_paths_eval earlier on the
// stream, read wave-uniformly), the turn of its motion (`motion` is null when no motions are set), or the
// static turn.  Only after() differs.
struct PathObstacleHook : ObstacleHook {
   const sph_hip_obstacle_motion* motion;
   float tau0, tau1;
   const PathShift* shift;
   __device__ void after(const float* p, float* v, float* q, float) const
   {
      obstacles_respond_path(list, motion, shift, n, p, v, q, dt, damping, tau0, tau1);
   }
};

struct PathLoadHook : LoadHook {
   const sph_hip_obstacle_motion* motion;
   float tau0, tau1;
   const PathShift* shift;
   __device__ void after(const float* p, float* v, float* q, float m) const
   {
      load_obstacles_respond_path(list, motion, shift, n, p, v, q, dt, damping, tau0, tau1, m,
                                  static_cast<const LoadHook&>(*this));
   }
};

// The call the tuned kernels make, with the signature they always had (a hook parameter with a
// default changed the code of k_full_accel_lists: tools/kernel_isa_diff.py).
template <bool UNIT_SCALE>
__device__ __forceinline__ void integrate_particle(const PairConsts& k, float4& x, float4& v,
                                                   const float4 a, double& ke, double& pe)
{
   integrate_particle_hooked<UNIT_SCALE>(k, x, v, a, ke, pe, NoHook());
}

// The body of the three integrate kernels: particle p (live: an owned one) stepped with `hook`.
// KE/PE contributions are reduced per block in double (the reference's serial fp32 running sum
// is order dependent).
// HASH: the context holds the whole grid and exchanges with nobody, so the sorted state this
// kernel leaves is exactly the input of the next cell build: the build's first step (cell id,
// counting atomics - k_hash_count) is done here, on the position just computed, and the next
// build starts at its scan.  One launch and one read of the positions less per step.
// Under a hook that records, the lanes without a particle integrate a particle of zeros, so that the
// whole wave takes part in the hook's votes and reductions; nothing of it is stored or summed.
template <bool UNIT_SCALE, bool HASH, class Hook>
__device__ __forceinline__ void integrate_block(float4* __restrict__ posm, float4* __restrict__ velp,
                                                const float4* __restrict__ acc, const PairConsts& k,
                                                double* __restrict__ epart, const CellGrid& g,
                                                uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                                                uint32_t* __restrict__ cell_count, int p, bool live,
                                                const Hook& hook)
{
   double ke = 0.0, pe = 0.0;
   uint32_t c = 0xffffffffu;
   if (live || Hook::records) {
      float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = x, a = x;
      if (live) {
         x = posm[p];
         v = velp[p];
         a = acc[p];
      }
      integrate_particle_hooked<UNIT_SCALE>(k, x, v, a, ke, pe, hook);
      if (live) {
         posm[p] = x;
         velp[p] = v;
         if (HASH) {
            int cx, cy, cz;
            c = cell_of(g, x.x, x.y, x.z, cx, cy, cz);
            key[p] = c;
         }
      } else {
         ke = 0.0;
         pe = 0.0;
      }
   }
   if (HASH) count_cell_runs(c, live, p, cell_count, slot, (uint32_t)g.ncells);
   // block reduction, fixed order
   __shared__ double s_ke[RED_THREADS / SPH_WAVE], s_pe[RED_THREADS / SPH_WAVE];
#pragma unroll
   for (int d = SPH_WAVE / 2; d > 0; d >>= 1) {
      ke += __shfl_down(ke, d);
      pe += __shfl_down(pe, d);
   }
   const int lane = threadIdx.x & (SPH_WAVE - 1), w = threadIdx.x / SPH_WAVE;
   if (lane == 0) {
      s_ke[w] = ke;
      s_pe[w] = pe;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int q = 0; q < RED_THREADS / SPH_WAVE; q++) {
         a += s_ke[q];
         b += s_pe[q];
      }
      epart[2 * blockIdx.x + 0] = a;
      epart[2 * blockIdx.x + 1] = b;
   }
}

// Owned particles only: ghosts are integrated by the slab that owns them.
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
            const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
            uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
            uint32_t* __restrict__ cell_count)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, p < meta[META_OWN_END], NoHook());
}

// k_integrate followed by the response to the `n_obst` static obstacles of `obst` (a context with
// obstacles takes this kernel instead of the fused routes: launch_policy.h, fuse_integrate).
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_obst(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                 const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                 uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                 uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const ObstacleHook hook = {obst, n_obst, k.dt, k.damping};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, p < meta[META_OWN_END], hook);
}

// k_integrate_obst (n_obst may be 0: k_integrate) that also adds every wall and obstacle response to
// `row`, this step's row of the context's load recording (LoadHook above).
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_loads(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                  const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                  uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                  uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                  unsigned long long* __restrict__ row, int quantum_log2)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const bool live = p < meta[META_OWN_END];
   const LoadHook hook = {obst, n_obst, k.dt, k.damping, row, load_scale(quantum_log2), live};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, live, hook);
}

// k_integrate_obst and k_integrate_loads for a list in which some entry moves (launch_policy.h:
// use_moving_kernels): `motion` holds one entry per obstacle, tau0 / tau1 the motion clock of this step.
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_obst_moving(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                        const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                        uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                        uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                        const sph_hip_obstacle_motion* __restrict__ motion, float tau0, float tau1)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const MovingObstacleHook hook = {{obst, n_obst, k.dt, k.damping}, motion, tau0, tau1};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, p < meta[META_OWN_END], hook);
}

template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_loads_moving(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                         const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                         uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                         uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                         unsigned long long* __restrict__ row, int quantum_log2,
                         const sph_hip_obstacle_motion* __restrict__ motion, float tau0, float tau1)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const bool live = p < meta[META_OWN_END];
   const MovingLoadHook hook = {{obst, n_obst, k.dt, k.damping, row, load_scale(quantum_log2), live}, motion, tau0, tau1};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, live, hook);
}

// Free bodies (body_policy.h; launch_policy.h: use_body_kernels).  One wave in front of every integrate of
// a context with bodies: lane i advances the body of obstacle i from `row`, the load row the previous
// integrate filled (null: none yet), and the wave zeroes `clear`, the internal row the coming integrate
// fills (null: it fills a row of the caller's recording).  Every lane loads and stores its own words.
__global__ void __launch_bounds__(SPH_WAVE)
k_bodies_advance(const sph_hip_body* __restrict__ bodies, BodyState* __restrict__ state, int n_obst,
                 const unsigned long long* row, int quantum_log2, float dt, unsigned long long* clear)
{
   const int lane = threadIdx.x;
   if (clear)
      for (int w = lane; w < LOAD_ROW_WORDS; w += SPH_WAVE) clear[w] = 0ull;
   if (lane >= n_obst) return;
   const sph_hip_body b = bodies[lane];
   BodyState s = state[lane];
   body_advance(b, s, reinterpret_cast<const long long*>(row), lane, quantum_log2, dt);
   state[lane] = s;
}

// k_integrate_loads_moving for a list with bodies: `bodies` and `state` hold one entry per obstacle,
// `motion` too or is null; always records into `row`.
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_bodies(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                   const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                   uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                   uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                   unsigned long long* __restrict__ row, int quantum_log2,
                   const sph_hip_obstacle_motion* __restrict__ motion, float tau0, float tau1,
                   const sph_hip_body* __restrict__ bodies, const BodyState* __restrict__ state)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const bool live = p < meta[META_OWN_END];
   const BodyLoadHook hook = {{obst, n_obst, k.dt, k.damping, row, load_scale(quantum_log2), live}, motion, tau0, tau1,
                              bodies, state};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, live, hook);
}

// Motion paths (obstacle_policy.h, fourth part; launch_policy.h: use_path_kernels).  One wave in front of
// every integrate of a context with paths: lane i forms the shifts of obstacle i at the step's clock pair
// (path_shift_of_step: two searches of its own keys by value) and stores its own 32 bytes of `shift`.
// The host has checked every key range against the key list (path_check).
__global__ void __launch_bounds__(SPH_WAVE)
k_paths_eval(const sph_hip_motion_path* __restrict__ paths, const sph_hip_motion_key* __restrict__ keys, int n_obst,
             float tau0, float tau1, PathShift* __restrict__ shift)
{
   const int lane = threadIdx.x;
   if (lane >= n_obst) return;
   const sph_hip_motion_path P = paths[lane];
   shift[lane] = path_shift_of_step(P, keys, tau0, tau1);
}

// k_integrate_obst_moving and k_integrate_loads_moving for a list with paths: `shift` holds one entry per
// obstacle, `motion` too or is null.
template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_obst_path(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                      const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                      uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                      uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                      const sph_hip_obstacle_motion* __restrict__ motion, float tau0, float tau1,
                      const PathShift* __restrict__ shift)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const PathObstacleHook hook = {{obst, n_obst, k.dt, k.damping}, motion, tau0, tau1, shift};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, p < meta[META_OWN_END], hook);
}

template <bool UNIT_SCALE, bool HASH>
__global__ void __launch_bounds__(RED_THREADS)
k_integrate_loads_path(float4* __restrict__ posm, float4* __restrict__ velp, const float4* __restrict__ acc,
                       const int32_t* __restrict__ meta, PairConsts k, double* __restrict__ epart, CellGrid g,
                       uint32_t* __restrict__ key, uint32_t* __restrict__ slot,
                       uint32_t* __restrict__ cell_count, const sph_hip_obstacle* __restrict__ obst, int n_obst,
                       unsigned long long* __restrict__ row, int quantum_log2,
                       const sph_hip_obstacle_motion* __restrict__ motion, float tau0, float tau1,
                       const PathShift* __restrict__ shift)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   const bool live = p < meta[META_OWN_END];
   const PathLoadHook hook = {{obst, n_obst, k.dt, k.damping, row, load_scale(quantum_log2), live}, motion, tau0, tau1,
                              shift};
   integrate_block<UNIT_SCALE, HASH>(posm, velp, acc, k, epart, g, key, slot, cell_count, p, live, hook);
}

// one block: totals of the per-block partials, written to out[0..1]
__global__ void __launch_bounds__(RED_THREADS)
k_energy_total(const double* __restrict__ epart, int nblocks, double* __restrict__ out)
{
   double ke = 0.0, pe = 0.0;
   for (int b = threadIdx.x; b < nblocks; b += RED_THREADS) {
      ke += epart[2 * b + 0];
      pe += epart[2 * b + 1];
   }
   __shared__ double s_ke[RED_THREADS], s_pe[RED_THREADS];
   s_ke[threadIdx.x] = ke;
   s_pe[threadIdx.x] = pe;
   __syncthreads();
   for (int d = RED_THREADS / 2; d > 0; d >>= 1) {
      if ((int)threadIdx.x < d) {
         s_ke[threadIdx.x] += s_ke[threadIdx.x + d];
         s_pe[threadIdx.x] += s_pe[threadIdx.x + d];
      }
      __syncthreads();
   }
   if (threadIdx.x == 0) {
      out[0] = s_ke[0];
      out[1] = s_pe[0];
   }
}

// ---- host layout <-> device layout --------------------------------------------------------------
// stage holds the reference's arrays back to back: pos[3n] vel[3n] mass[n]
__global__ void __launch_bounds__(256)
k_import(const float* __restrict__ pos, const float* __restrict__ vel,
         const float* __restrict__ mass, const uint32_t* __restrict__ ids, int n,
         float4* __restrict__ posm, float4* __restrict__ velp)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   const uint32_t id = ids ? ids[i] : (uint32_t)i;
   posm[i] = make_float4(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], mass[i]);
   velp[i] = make_float4(vel[3 * i + 0], vel[3 * i + 1], vel[3 * i + 2], __uint_as_float(id));
}

// scatter by persistent id into pos[3n] vel[3n] rho[n] acc[3n] ncount[n] (any may be null)
// `compact`: write row (p - own_begin) instead of row id, and the ids to oid (slab download)
__global__ void __launch_bounds__(256)
k_export(const float4* __restrict__ posm, const float4* __restrict__ velp,
         const float* __restrict__ rho, const float4* __restrict__ acc,
         const int32_t* __restrict__ ncount, const int32_t* __restrict__ meta, int compact,
         float* __restrict__ pos, float* __restrict__ vel, float* __restrict__ orho,
         float* __restrict__ oacc, int32_t* __restrict__ ocount, uint32_t* __restrict__ oid)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_OWN_END]) return;
   const float4 v = velp[p];
   uint32_t id = __float_as_uint(v.w);
   if (compact) {
      if (oid) oid[p - meta[META_OWN_BEGIN]] = id;
      id = (uint32_t)(p - meta[META_OWN_BEGIN]);
   }
   if (pos) {
      const float4 x = posm[p];
      pos[3 * id + 0] = x.x;
      pos[3 * id + 1] = x.y;
      pos[3 * id + 2] = x.z;
   }
   if (vel) {
      vel[3 * id + 0] = v.x;
      vel[3 * id + 1] = v.y;
      vel[3 * id + 2] = v.z;
   }
   if (orho) orho[id] = rho[p];
   if (oacc) {
      const float4 a = acc[p];
      oacc[3 * id + 0] = a.x;
      oacc[3 * id + 1] = a.y;
      oacc[3 * id + 2] = a.z;
   }
   if (ocount) ocount[id] = ncount[p];
}

// masses of the owned particles, row p - own_begin (the row order of a compact k_export)
__global__ void __launch_bounds__(256)
k_export_mass(const float4* __restrict__ posm, const int32_t* __restrict__ meta, float* __restrict__ mass)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_OWN_END]) return;
   mass[p - meta[META_OWN_BEGIN]] = posm[p].w;
}

// per-voxel occupancy on the REFERENCE voxel grid (edge mCellSize = 2h, reference
// src/sph.cpp:438-481) whatever grid the context sorts by: what getGrid()[i].count() readers get
__global__ void __launch_bounds__(256)
k_voxel_counts(const float4* __restrict__ posm, const int32_t* __restrict__ meta, float inv, int nx,
               int ny, int nz, int32_t* __restrict__ counts)
{
   const int p = meta[META_OWN_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_OWN_END]) return;
   const float4 x = posm[p];
   const int cx = cell_coord(x.x, inv, nx), cy = cell_coord(x.y, inv, ny), cz = cell_coord(x.z, inv, nz);
   atomicAdd(&counts[(cz * ny + cy) * nx + cx], 1);
}

// ---- neighbour statistics (reference src/sph.cpp:204-232) -----------------------------------------
// out: [0] = sum low 32, [1] = sum high 32 (as one 64-bit add), [2] = max, [3] = min (from 34)
__global__ void __launch_bounds__(RED_THREADS)
k_neighbor_stats(const int32_t* __restrict__ ncount, const int32_t* __restrict__ meta,
                 int32_t* __restrict__ out)
{
   long long sum = 0;
   int mx = -1, mn = 34;
   const int begin = meta[META_OWN_BEGIN], end = meta[META_OWN_END];
   for (int i = begin + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
      const int c = ncount[i];
      sum += c;
      mx = c > mx ? c : mx;
      mn = c < mn ? c : mn;
   }
#pragma unroll
   for (int d = SPH_WAVE / 2; d > 0; d >>= 1) {
      sum += __shfl_down(sum, d);
      const int omx = __shfl_down(mx, d), omn = __shfl_down(mn, d);
      mx = omx > mx ? omx : mx;
      mn = omn < mn ? omn : mn;
   }
   if ((threadIdx.x & (SPH_WAVE - 1)) == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)sum);
      atomicMax(out + 2, mx);
      atomicMin(out + 3, mn);
   }
}

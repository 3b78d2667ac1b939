/* sph_hip.h — C ABI of the MI355X (gfx950) SPH step.
 *
 * This is the drop-in boundary for the hot path of
 * DanielaCourel/smoothed_particle_hydrodynamics: everything SPH::step()
 * (reference src/sph.cpp:190-304) does between "particles in" and "particles out".
 * The reference has no FFI layer; its seam is the C++ class `SPH` (reference
 * src/sph.h:15-216).  Each entry point below names the member(s) of that class it
 * replaces, so a maintainer can keep sph.h unchanged and forward the bodies in sph.cpp
 * to this library.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary;
 *   - every call returns SPH_HIP_OK (0) or a negative sph_hip_status; the message for the
 *     last failure on a context is available from sph_hip_last_error();
 *   - host arrays use the reference's layouts: positions / velocities / accelerations
 *     interleaved xyz (`mPosition[3*i+c]`, reference src/particle.h:13-18), one float or
 *     int per particle otherwise, all indexed by the particle's persistent index;
 *   - device memory, streams and events are owned by the context.
 */
#ifndef SPH_HIP_H
#define SPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_HIP_ABI_VERSION 7
/* The ABI version the loaded library was built with (compare with SPH_HIP_ABI_VERSION of the
 * header the host was compiled against before calling anything else).  A library built with
 * profiling hooks that cut pieces out of the kernels (diagnostic builds: results are garbage by
 * design) ORs SPH_HIP_ABI_DIAGNOSTIC into the value, so that no host takes it for the product. */
#define SPH_HIP_ABI_DIAGNOSTIC 0x4000
int sph_hip_abi_version(void);

typedef enum sph_hip_status {
   SPH_HIP_OK = 0,
   SPH_HIP_ERR_INVALID = -1,   /* bad argument / bad state */
   SPH_HIP_ERR_DEVICE = -2,    /* a HIP runtime call failed */
   SPH_HIP_ERR_CAPACITY = -3,  /* more particles than the context was created for */
   SPH_HIP_ERR_NO_DEVICE = -4, /* no usable gfx950 device */
   SPH_HIP_ERR_EXCHANGE = -5   /* a slab exchange lost particles (sph_hip_slab_status bits) */
} sph_hip_status;

/* Neighbour semantics of a context.
 *   REF  — the shipped search: octant of 2h-voxels, LCG-sampled chunks of 8 of which 4 are
 *          tested, at most 28 stored neighbours (reference src/sph.cpp:484-692), then the
 *          list-driven sums.  Integer outputs are identical to the reference's.
 *   FULL — every neighbour inside the interaction radius, found on a grid of cell edge
 *          >= h (27 cells), visited in ascending (cell id, particle index); per-pair
 *          arithmetic is the reference's (src/sph.cpp:737-761, 825-884).
 *   FULL_FAST — FULL with tolerance-mode pair arithmetic (SPH_HIP_ARITH_FAST below): the same
 *          neighbour sets (the exact fp32 test (dx*dx + dy*dy) + dz*dz < h^2 of
 *          src/sph.cpp:641,653), the same canonical order and the viscous rescale inside the
 *          neighbour loop (src/sph.cpp:880-882) - but the per-pair arithmetic evaluated the way
 *          the reference's own shipped build may evaluate it (reference CMakeLists.txt:21:
 *          -O3 -ffast-math -funsafe-math-optimizations -mfma), in the ACCELERATION sum only: an
 *          fp32 reciprocal in place of the fp64 quotient of src/sph.cpp:854-856, fused
 *          accumulation, and a viscous sum that leaves out the neighbours whose weight - the
 *          rescale of src/sph.cpp:880-882 applied once per later neighbour - is below 1e-20;
 *          both sums on the reference's stored distance.  Neighbour counts AND densities are
 *          identical to FULL; the acceleration of EVERY particle agrees with the IEEE evaluation of
 *          src/sph.cpp to 1e-4 relative, |a - a_ref| <= 1e-4 * max(|a|, |a_ref|) (vector norm) -
 *          asserted as written, without escape clauses, on every BASELINE configuration and every
 *          committed scene (tests/test_gpu_full_fast.py, test_gpu_full_size.py, test_gpu_c4_c5.py;
 *          measured: 1.4e-5 at worst on the 4M column at rest, 6e-6 moving; bench.py re-checks the
 *          state it timed: `parity` in its JSON line).  ONE clause exists, for adversarial inputs only
 *          (tests/test_gpu_random_scenes.py, which prints every particle that takes it): where a
 *          particle's ~30 pair terms cancel to less than a hundredth of their magnitude sum T, any
 *          evaluation that is not the reference's bit for bit - its own -ffast-math build included -
 *          differs by rounding errors of the terms, and such a particle is held to 1e-6 * T instead
 *          (at most 0.5 % of a scene's particles).  Deterministic, the same for any route and slab
 *          count, not bit-reproducible against the CPU. */
typedef enum sph_hip_mode {
   SPH_HIP_MODE_REF = 0,
   SPH_HIP_MODE_FULL = 1,
   SPH_HIP_MODE_FULL_FAST = 2
} sph_hip_mode;

/* The constants the hot path reads — the protected members SPH::SPH() initialises
 * (reference src/sph.h:149-210, src/sph.cpp:46-98).  Field order is ABI. */
typedef struct sph_hip_params {
   int32_t cells_x, cells_y, cells_z; /* mGridCellsX/Y/Z   (voxel grid, edge 2h)        */
   float cell_size;                   /* mCellSize                                      */
   float max_x, max_y, max_z;         /* mMaxX/Y/Z                                      */
   float h;                           /* mH                                             */
   float h2;                          /* mH2                                            */
   float hscaled;                     /* mHScaled                                       */
   float hscaled2;                    /* mHScaled2                                      */
   float hscaled6;                    /* mHScaled6                                      */
   float hscaled9;                    /* mHScaled9                                      */
   float htimes2;                     /* mHTimes2                                       */
   float htimes2inv;                  /* mHTimes2Inv                                    */
   float sim_scale;                   /* mSimulationScale                               */
   float sim_scale_inv;               /* mSimulationScaleInverse                        */
   float kernel1, kernel2, kernel3;   /* mKernel1Scaled, mKernel2Scaled, mKernel3Scaled */
   float rho0;                        /* mRho0                                          */
   float stiffness;                   /* mStiffness        (SPH::setStiffness)          */
   float viscosity;                   /* mViscosityScalar  (SPH::setViscosityScalar)    */
   float time_step;                   /* mTimeStep         (SPH::setTimeStep)           */
   float damping;                     /* mDamping          (SPH::setDamping)            */
   float cfl_limit, cfl_limit2;       /* mCflLimit, mCflLimit2 (SPH::setCflLimit)       */
   float gravity[3];                  /* mGravity          (SPH::setGravity)            */
   float grav_const;                  /* mGravConstant                                  */
   float central_mass;                /* mCentralMass                                   */
   float central_pos[3];              /* mCentralPos                                    */
   float softening;                   /* mSoftening                                     */
   int32_t examine_count;             /* mExamineCount (32); REF mode: >= SPH_HIP_MIN_EXAMINE_COUNT */
   /* FULL-mode grid (no reference counterpart): cell edge >= h */
   int32_t full_cells_x, full_cells_y, full_cells_z;
   float full_cell_inv;
   /* Dam-break physics the reference defines but never wires; both 0 =
    * shipped behaviour.
    *   apply_gravity: mGravity is added wherever the reference adds its point-mass gravity
    *                  (computeAcceleration src/sph.cpp:913-915 and integrate :987-989).
    *   apply_walls:   integrate passes (old position, new velocity, dt, new position) through
    *                  SPH::handleBoundaryConditions / applyBoundary (src/sph.cpp:1025-1148):
    *                  per-axis reflection at 0 / mMax*, remaining path scaled by mDamping. */
   int32_t apply_gravity;
   int32_t apply_walls;
} sph_hip_params;

typedef struct sph_hip_context sph_hip_context;

/* ---- construction -------------------------------------------------------------------- */

/* Constants for smoothing length h and a voxel grid of the given shape, derived exactly as
 * SPH::SPH() derives them (reference src/sph.cpp:46-98: double pow() narrowed to float,
 * float kernel normalisations).  h = 0.1f, cells = 32^3 gives the reference's defaults. */
int sph_hip_params_default(sph_hip_params* out, float h, int cells_x, int cells_y, int cells_z);

/* Replaces the allocations in SPH::SPH() (reference src/sph.cpp:100-113): device storage for
 * up to `capacity` particles on HIP device `device`.  A REF-mode context needs examine_count >=
 * SPH_HIP_MIN_EXAMINE_COUNT (else SPH_HIP_ERR_INVALID, with a last_error text): the search
 * (reference src/sph.cpp:598-679) stores up to 4 neighbours per chunk of 8 candidates and stops
 * once more than examine_count - 8 are stored, so it stores at most max(4, examine_count - 4)
 * entries - past the end of a list of fewer than 4.  The reference does not check this. */
#define SPH_HIP_MIN_EXAMINE_COUNT 4
int sph_hip_create(sph_hip_context** out, const sph_hip_params* params, int capacity, int mode,
                   int device);
void sph_hip_destroy(sph_hip_context* ctx);

/* Last error text for ctx (or for the failed create when ctx is NULL). Never NULL. */
const char* sph_hip_last_error(const sph_hip_context* ctx);

/* Replaces the six GUI setters + the constructor constants (reference src/sph.cpp:1219-1289).
 * Takes effect at the start of the next phase call; grid shape, h and examine_count may not
 * change.  Like the reference, which forms every pressure inside computeAcceleration
 * (src/sph.cpp:785, 829-834), an acceleration phase uses the constants set when it is called for
 * the neighbours' pressure terms too: a FULL-mode context forms those terms in its density pass
 * and, when rho0, stiffness, kernel3 or the arithmetic have changed since, forms them again
 * before the acceleration pass (sph_hip_step never changes constants in the middle of a step). */
int sph_hip_set_params(sph_hip_context* ctx, const sph_hip_params* params);
int sph_hip_get_params(const sph_hip_context* ctx, sph_hip_params* out);

/* Pair arithmetic of a FULL-mode context (sph_hip_create with SPH_HIP_MODE_FULL_FAST starts in
 * SPH_HIP_ARITH_FAST; slab contexts start exact).  May be changed between steps (synchronises);
 * takes effect with the next cell build.  No counterpart in the reference's API: its counterpart
 * is the compiler flags the reference is built with (CMakeLists.txt:21). */
#define SPH_HIP_ARITH_EXACT 0
#define SPH_HIP_ARITH_FAST 1
int sph_hip_set_arithmetic(sph_hip_context* ctx, int arithmetic);
int sph_hip_get_arithmetic(const sph_hip_context* ctx);

/* ---- particle state ------------------------------------------------------------------- */

/* Host -> device.  Replaces the fill of Particle::mPosition/mVelocity/mMass done by
 * initParticlePolitionsSphere() and the constructor (reference src/sph.cpp:105-108,
 * 361-425).  pos/vel: 3*n floats interleaved; mass: n floats.  Sets the live count. */
int sph_hip_upload(sph_hip_context* ctx, int n, const float* pos, const float* vel,
                   const float* mass);

/* Device -> host mirror of `Particle` (reference src/particle.h:13-18), any pointer may be
 * NULL: mPosition, mVelocity, mDensity, mAcceleration, mNeighborCount, indexed by the
 * particle's persistent index.  This is what SPH::getParticles() consumers read
 * (reference src/visualization.cpp:144-158). */
int sph_hip_download(sph_hip_context* ctx, float* pos, float* vel, float* density, float* acc,
                     int32_t* neighbor_count);

/* The same mirror without stopping the solver thread - what the reference's GUI gets when it
 * reads SPH::getParticles() / getGrid() at 60 Hz from another thread, without locks
 * (reference src/visualization.cpp:144-158, 178-193).
 *   sph_hip_download_async  enqueues, behind the work queued so far, a snapshot of the
 *       per-particle arrays (any pointer may be NULL) and of the per-voxel occupancy on the
 *       REFERENCE voxel grid (cells_x*cells_y*cells_z ints, edge mCellSize - in FULL mode too),
 *       and their copy to the host on a separate low-priority stream; returns at once.  The
 *       later steps' kernels do not wait for the copy.  *started = 0 (nothing done) while the
 *       previous request is still on its way: a mirror is a picture, not a queue.
 *   sph_hip_download_done   1 = the last request has arrived in the host arrays, 0 = not yet
 *       (wait != 0: blocks until it has).  Negative = error.
 *   sph_hip_host_register   page-locks host memory (e.g. the storage of Particle's vectors) so
 *       that the copy really is asynchronous; pageable memory works, slower and less overlapped.
 * Double-buffer on the host: request into the back set, swap when done (integration/). */
int sph_hip_download_async(sph_hip_context* ctx, float* pos, float* vel, float* density, float* acc,
                           int32_t* neighbor_count, int32_t* voxel_counts, int* started);
int sph_hip_download_done(sph_hip_context* ctx, int wait);
int sph_hip_host_register(void* ptr, size_t bytes);
int sph_hip_host_unregister(void* ptr);

int sph_hip_particle_count(const sph_hip_context* ctx);

/* ---- the step -------------------------------------------------------------------------- */

/* SPH::step() (reference src/sph.cpp:190-304): the five phases below, in order. */
int sph_hip_step(sph_hip_context* ctx);
/* `steps` back-to-back steps with no host synchronisation in between. */
int sph_hip_run(sph_hip_context* ctx, int steps);

/* SPH::voxelizeParticles() + clearGrid() (reference src/sph.cpp:429-481): cell ids, per-cell
 * counts, cell-sorted order (ascending particle index inside a cell). */
int sph_hip_voxelize(sph_hip_context* ctx);
/* The findNeighbors() loop (reference src/sph.cpp:216-231, 484-692).  REF: builds
 * mNeighbors / mNeighborDistancesScaled / mNeighborCount.  FULL: no stored lists — the
 * neighbour walk is fused into the two sums; this call is a no-op kept for phase timing. */
int sph_hip_find_neighbors(sph_hip_context* ctx);
/* The computeDensity() loop (reference src/sph.cpp:242-249, 721-766). */
int sph_hip_compute_density(sph_hip_context* ctx);
/* The computeAcceleration() loop (reference src/sph.cpp:270-277, 778-934). */
int sph_hip_compute_acceleration(sph_hip_context* ctx);
/* The integrate() loop (reference src/sph.cpp:285-289, 937-1022) incl. KE/PE totals. */
int sph_hip_integrate(sph_hip_context* ctx);

/* Wait for all queued work of ctx. */
int sph_hip_synchronize(sph_hip_context* ctx);

/* ---- diagnostics ------------------------------------------------------------------------ */

/* Milliseconds (fractional, unlike the reference's truncated ints) spent in the six phases of
 * the last sph_hip_step(): voxelize, findNeighbors, density, pressure(=0), acceleration,
 * integrate — the arguments of SPH::updateElapsed (reference src/sph.cpp:292-299). */
int sph_hip_get_timings(sph_hip_context* ctx, float ms[6]);
/* Sums of the same six phase times over the sph_hip_step() calls since the last
 * sph_hip_reset_timings() (at most the most recent 128 steps are kept); *steps = how many
 * steps the sums cover.  Measured with HIP events on the context's own stream. */
int sph_hip_get_phase_totals(sph_hip_context* ctx, double ms[6], int32_t* steps);
int sph_hip_reset_timings(sph_hip_context* ctx);
/* What sph_hip_step() times (an event record is a barrier packet: ~10 us each on the stream).
 * SPH_HIP_TIMING_PHASES (default): every phase boundary, as SPH::updateElapsed wants.
 * SPH_HIP_TIMING_SUMS: only the density + acceleration pair, as one interval - reported in
 * slot 2 (density) of the two calls above, the other slots 0.  SPH_HIP_TIMING_OFF: nothing
 * (sph_hip_get_timings fails, the totals cover 0 steps).  Resets the collected timings. */
#define SPH_HIP_TIMING_OFF 0
#define SPH_HIP_TIMING_SUMS 1
#define SPH_HIP_TIMING_PHASES 2
int sph_hip_set_timing(sph_hip_context* ctx, int level);
/* Record the events of the chosen level on every `every`-th timed step only (default 1 = every
 * step); the totals and their step count then cover the sampled steps.  For measurements that
 * must not weigh on what they measure (bench.py).  Resets the collected timings. */
int sph_hip_set_timing_stride(sph_hip_context* ctx, int every);

/* FULL mode, tiled kernels: statistics of the LDS tiles of the last step (synchronises).
 * out[0..11]: workgroups whose tile exceeds capacity level i (the levels are the largest tiles
 * that allow a given number of workgroups per CU), out[12]: workgroups, out[13]: largest tile
 * (entries), out[14], out[15]: workgroups computed untiled in the density / acceleration pass,
 * out[16], out[17]: tile capacities the two passes were launched with, out[18]: 1 if the list
 * entries were in their wide format (a capacity above 4064), out[19]: neighbours per particle the
 * lists currently hold (starts at 254; enlarged to 1022 - or to 510, if that is all the device has
 * room for - when a step reports particles with more: those are computed without a list, slower,
 * same results). */
int sph_hip_get_tile_stats(sph_hip_context* ctx, int32_t out[20]);

/* mKineticEnergyTotal / mPotentialEnergyTotal of the last integrate
 * (reference src/sph.cpp:1001-1013).  Summed in double in a fixed tree order; the
 * reference's serial fp32 sum is order-dependent, so compare with a tolerance. */
int sph_hip_get_energy(sph_hip_context* ctx, float* kinetic, float* potential);

/* The three numbers the reference appends to out/neighbors.txt each step
 * (reference src/sph.cpp:204-232): sum/N (integer division), max, min(<=34). */
int sph_hip_get_neighbor_stats(sph_hip_context* ctx, int32_t* avg, int32_t* max, int32_t* min);

/* mVoxelCoords / mVoxelIds (reference src/sph.cpp:466-472); coords: 3*n ints. */
int sph_hip_download_voxels(sph_hip_context* ctx, int32_t* coords_xyz, int32_t* ids);
/* Per-voxel occupancy, what callers get from SPH::getGrid()[i].count()
 * (reference src/visualization.cpp:178-193). `counts` has cells_x*cells_y*cells_z entries
 * (REF) or full_cells_x*full_cells_y*full_cells_z (FULL). */
int sph_hip_download_grid_counts(sph_hip_context* ctx, int32_t* counts);
/* REF mode only: mNeighbors / mNeighborDistancesScaled, n*examine_count entries each
 * (reference src/sph.cpp:112-113). */
int sph_hip_download_neighbor_lists(sph_hip_context* ctx, uint32_t* neighbors, float* distances);

/* ---- field sampler ----------------------------------------------------------------------- */

/* SPH interpolation of the CURRENT state (positions, masses, velocities; never the densities of
 * the last step) at probe points, FULL and FULL_FAST contexts that hold the whole grid (identical
 * results in both arithmetics).  For a probe x, over every live particle j:
 *   member  d2 = (dx*dx + dy*dy) + dz*dz < h2 in fp32, dx = x.x - x_j.x etc. - the density
 *           pass's test, but NO particle is excluded: a probe placed on a particle includes that
 *           particle's own term (unlike computeDensity, reference src/sph.cpp:737);
 *   term    t_j = m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrtf(d2) * sim_scale - the density
 *           pass's arithmetic, including its range test on d where the scale is not unit;
 *   density sum of t_j in fp32, in canonical order: ascending FULL cell id, then ascending index;
 *   velocity (sum of t_j * v_j, per component, unfused, same order) / density if density > 0,
 *           else 0 (Shepard-normalised);
 *   count   the number of members.
 * A non-finite or out-of-box probe needs no special case: its cell is the cell build's clamped
 * one, and a NaN or infinite d2 is never a member - such a probe gives density 0, count 0 and
 * velocity 0.
 * Each call first brings the cell structure up to date (the build sph_hip_voxelize runs).  A call
 * does not change the simulation: sph_hip_download returns the same bytes before and after it,
 * and every later step is bit-identical to one without it.  Any output may be NULL (with all of
 * them NULL the probes are still evaluated: timing); arrays are host memory; the call
 * synchronises.  SPH_HIP_ERR_INVALID for a REF context, a slab context (sph_hip_create_slab with
 * neighbours, or one that has exchanged), n < 0, dims <= 0, a non-finite origin, a non-finite or
 * non-positive spacing, and a lattice of more than 2^31 - 1 points.  n == 0 does nothing.
 * These two calls return density, velocity and count; the pressure at a probe is
 * sph_hip_sample_pressure_points / _lattice (below: pressure readings). */
/* n probes, xyz interleaved; density[n], velocity_xyz[3n], count[n] */
int sph_hip_sample_points(sph_hip_context* ctx, int n, const float* xyz,
                          float* density, float* velocity_xyz, int32_t* count);
/* The lattice origin + (float)i * spacing per axis (fp32, unfused), i in [0, dims).
 * Out index (k*dims[1] + j)*dims[0] + i, x fastest like the cell ids. */
int sph_hip_sample_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                           const int32_t dims[3], float* density, float* velocity_xyz, int32_t* count);

/* ---- iso-surface extractor ---------------------------------------------------------------- *
 *
 * An indexed triangle mesh of the fluid's surface {f > iso} over the density lattice f that
 * sph_hip_sample_lattice(ctx, origin, spacing, dims, ...) would return at that moment (hence the
 * same mesh in FULL and FULL_FAST).  All arithmetic is fp32, unfused, in the order written.
 *   inside     a lattice point is inside when f > iso (strictly); NaN is outside.
 *   cells      the cube with lower corner (i, j, k), i < nx-1, j < ny-1, k < nz-1; its corner
 *              c = x + 2y + 4z is lattice point (i+x, j+y, k+z).  It splits into six tetrahedra
 *              {0, a, a|b, 7}, (a, b) in the order (1,2), (1,4), (2,1), (2,4), (4,1), (4,2).
 *   edges      every tetrahedron edge is one of the seven positive-direction edges of a lattice
 *              point p, in the order +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z; an edge exists only
 *              where its far end is on the lattice.  An edge with exactly one inside endpoint
 *              carries one vertex.  Vertex ids are ranks in canonical order: first by p's lattice
 *              index (k*ny + j)*nx + i, then by the edge's place in that list.
 *   position   a = p (the owning end), b = the far end: t = (iso - f_a) / (f_b - f_a), then
 *              t = fminf(fmaxf(t, 0), 1) (IEEE: NaN becomes 0); per component
 *              x = x_a + t * (x_b - x_a), lattice coordinates origin + (float)i * spacing.
 *   normal     the lattice gradient at a and at b, per axis of spacing s: central
 *              (f[+1] - f[-1]) / (2 * s) inside, (f[+1] - f) / s on the lower face, (f - f[-1]) / s
 *              on the upper face, 0 along an axis of one point; g = g_a + t * (g_b - g_a) per
 *              component; len = sqrtf((gx*gx + gy*gy) + gz*gz); the normal is -(g / len) per
 *              component when len is finite and > 0, else 0 (it points toward lower density).
 *   velocity   v = v_a + t * (v_b - v_a) per component, of the sampler's Shepard velocity.
 *   triangles  in canonical cube order, then tetrahedron order.  A tetrahedron with its four
 *              corners all inside or all outside emits none; one corner apart from the other three:
 *              one triangle of the three edges at that corner; two and two: the quad of the four
 *              crossing edges, cycle (q0, q1, q2, q3) with consecutive edges sharing a corner, as
 *              (q0, q1, q2), (q0, q2, q3).  Every cycle starts at its smallest vertex id and is
 *              oriented so that, with its vertices at the edge midpoints (t = 0.5),
 *              (v1 - v0) x (v2 - v0) points from the inside corners toward the outside ones -
 *              combinatorial: degenerate positions (t of 0 or 1) cannot flip it.
 *   guarantee  when no point on the lattice's outer faces is inside, the mesh is closed and
 *              consistently oriented: every undirected edge is used by exactly two triangles, once
 *              in each direction.  (The sampler gives zeros outside the box: a lattice reaching
 *              past it yields a closed surface.)  Vertices on edges that no cube uses (a lattice of
 *              one point along x or y) are counted and emitted all the same.
 * The mesh is kept in the context until the next extraction or sph_hip_destroy; steps do not
 * touch it.  Both calls synchronise; neither changes the simulation (extraction first runs the
 * cell build sph_hip_voxelize runs, as the sampler does).
 * sph_hip_extract_surface: SPH_HIP_ERR_INVALID for everything sph_hip_sample_lattice refuses, for
 * an iso that is not finite or not > 0, and for unknown flag bits; SPH_HIP_ERR_CAPACITY when V or T
 * would exceed 2^31 - 1 or the mesh cannot be allocated.  Either way no mesh is kept.
 * sph_hip_download_surface: SPH_HIP_ERR_INVALID when no mesh is kept, or when an output is asked
 * for that the extraction's flags did not compute. */
#define SPH_HIP_SURFACE_NORMALS  1
#define SPH_HIP_SURFACE_VELOCITY 2
/* meshes the lattice, keeps the mesh in the context; counts[0] = vertices, counts[1] = triangles */
int sph_hip_extract_surface(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                            const int32_t dims[3], float iso, int flags, int32_t counts[2]);
/* copies the kept mesh out: vertices_xyz[3V], normals_xyz[3V], velocity_xyz[3V], triangles[3T]; any may be NULL */
int sph_hip_download_surface(sph_hip_context* ctx, float* vertices_xyz, float* normals_xyz,
                             float* velocity_xyz, int32_t* triangles);

/* ---- renderer ----------------------------------------------------------------------------- *
 *
 * A ray-marched image of the fluid's surface {f > iso}, where f(p) is the density
 * sph_hip_sample_points would return at p at that moment (hence the same image in FULL and
 * FULL_FAST, and one that agrees with the sampler and the extractor).  All arithmetic is fp32,
 * unfused, in the order written; fminf / fmaxf follow C99 (a NaN operand yields the other one).
 *   pixel ray  pixel (px, py) of a W x H image, row 0 at the top:
 *              a = (float)(2*px + 1 - W) / (float)W, b = (float)(H - 2*py - 1) / (float)H;
 *              d_c = (forward_c + a * right_c) + b * up_c per component;
 *              len = sqrtf((dx*dx + dy*dy) + dz*dz); the direction is d_c / len per component.
 *              A pixel whose len is 0 or not finite misses.
 *   box        per axis: inv = 1.0f / d, t0 = (lo - eye) * inv, t1 = (hi - eye) * inv,
 *              near = fminf(t0, t1), far = fmaxf(t0, t1);
 *              tnear = fmaxf(fmaxf(fmaxf(near_x, near_y), near_z), 0.0f),
 *              tfar = fminf(fminf(far_x, far_y), far_z).  The ray misses unless tnear <= tfar.
 *   march      t_k = tnear + (float)k * step, p_k = eye + t_k * d per component, for k = 0, 1, ...
 *              while t_k <= tfar and k < max_samples.  The first k with f(p_k) > iso (strictly;
 *              NaN is outside) is first_inside; if no sample is inside, the ray misses.
 *   refine     k = 0: t_hit = tnear.  Otherwise ta = t_(k-1), tb = t_k, and `refine` times:
 *              tm = 0.5f * (ta + tb); tb = tm if f(eye + tm * d) > iso, else ta = tm.
 *              t_hit = tb; p_hit = eye + t_hit * d per component.
 *   normal     g_a = (f(p_hit + e_a) - f(p_hit - e_a)) / (2.0f * grad_step) per axis, where
 *              p_hit + e_a moves coordinate a alone by grad_step;
 *              len = sqrtf((gx*gx + gy*gy) + gz*gz); the normal is -(g / len) per component
 *              when len is finite and > 0, else 0 (it points toward lower density).
 *   shade      l = light / sqrtf((lx*lx + ly*ly) + lz*lz) per component;
 *              ndl = (nx*lx + ny*ly) + nz*lz; w = ambient + diffuse * fmaxf(ndl, 0.0f);
 *              channel c = (uint8_t)(fminf(fmaxf(albedo_c * w, 0.0f), 1.0f) * 255.0f + 0.5f);
 *              alpha 255.  A miss is `background`.
 *   outputs    one entry per pixel, row-major (index py * W + px), host memory, each may be NULL
 *              (with all of them NULL the frame is still computed: timing):
 *              rgba[4], depth (t_hit; +inf on a miss), normal_xyz[3] (0 on a miss),
 *              velocity_xyz[3] (the sampler's Shepard velocity at p_hit with
 *              SPH_HIP_RENDER_VELOCITY; 0 on a miss, and everywhere without the flag),
 *              first_inside (k; -1 on a miss).
 * Each call first brings the cell structure up to date (the build sph_hip_voxelize runs) and
 * synchronises before it returns; it does not change the simulation (sph_hip_download returns the
 * same bytes before and after it, and every later step is bit-identical to one without it).
 * SPH_HIP_ERR_INVALID, with a last_error text, for a REF or slab context (as the sampler), null
 * camera or params, width or height outside [1, 16384], a non-finite camera or params field, a
 * step or grad_step that is not > 0, an iso that is not > 0, refine outside [0, 30],
 * box_lo >= box_hi on an axis, a zero light vector, max_samples outside [1, 2^24], and unknown
 * flag bits. */
typedef struct sph_hip_camera {          /* field order is ABI */
   float eye[3];
   float forward[3];   /* toward the image centre, any length */
   float right[3];     /* image-plane half-width at unit forward distance */
   float up[3];        /* image-plane half-height at unit forward distance */
} sph_hip_camera;

typedef struct sph_hip_render_params {   /* field order is ABI */
   float box_lo[3], box_hi[3];   /* the volume that is marched */
   float step;                   /* march step, world units */
   float iso;                    /* surface level */
   int32_t refine;               /* bisection iterations */
   float grad_step;              /* offset of the central differences */
   float light[3];               /* direction toward the light */
   float albedo[3], ambient, diffuse;
   uint8_t background[4];        /* RGBA of a pixel whose ray misses */
   int32_t max_samples;          /* march samples per ray at most */
} sph_hip_render_params;

#define SPH_HIP_RENDER_VELOCITY 1
int sph_hip_render(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                   int width, int height, int flags, uint8_t* rgba, float* depth,
                   float* normal_xyz, float* velocity_xyz, int32_t* first_inside);

/* ---- scene renderer ------------------------------------------------------------------------ *
 *
 * sph_hip_render's frame with the context's solids drawn into it: the obstacles as they stand now
 * (what sph_hip_get_obstacles_now returns: motions at the current clock, bodies where the device has
 * moved them), met analytically by each pixel's ray and composited with the fluid by depth.  The
 * fluid pass is sph_hip_render's, unchanged; a pass of its own (k_scene_solids) then overwrites the
 * pixels a solid takes.  csrc/scene_policy.h holds the functions, one set for the device and the
 * host.  All arithmetic is fp32, unfused, in the order written ("a + b + c" is (a + b) + c); sqrtf and
 * "/" are correctly rounded; fminf / fmaxf follow C99.  eye, d: the camera's eye and the pixel's
 * normalised direction exactly as the renderer forms it (a pixel whose len is 0 or not finite meets no
 * solid); the ray is eye + t * d.
 *   slab       of one axis a with bounds lo, hi: inv = 1.0f / d_a, u0 = (lo - eye_a) * inv,
 *              u1 = (hi - eye_a) * inv, near_a = fminf(u0, u1), far_a = fmaxf(u0, u1) - the renderer's
 *              box, with its NaN behaviour: d_a == 0 with eye_a on a plane makes that u NaN, and
 *              near_a = far_a = the other u.
 *   interval   every kind gives [t0, t1].  A miss unless t0 <= t1 and t1 >= 0 (NaN misses).
 *              t0 < 0: the eye is inside; t = 0 and the normal is -d per component.  Otherwise
 *              t = fmaxf(t0, 0.0f) + 0.0f (the sum makes a -0 a +0) and the normal is the kind's.
 *   sphere     o = eye - center; b = (ox*dx + oy*dy) + oz*dz; c = ((ox*ox + oy*oy) + oz*oz) - r*r;
 *              disc = b*b - c; a miss unless disc >= 0; s = sqrtf(disc); t0 = -b - s, t1 = -b + s.
 *              normal_a = ((eye_a + t * d_a) - center_a) / r.
 *   box        t0 = fmaxf(fmaxf(near_x, near_y), near_z), t1 = fminf(fminf(far_x, far_y), far_z).
 *              The normal lies on the first axis a of x, y, z with near_a == t0:
 *              normal_a = d_a > 0 ? -1 : 1, the other two components 0.
 *   cylinder   axis a, u = (a+1)%3, w = (a+2)%3; ou = eye_u - center_u, ow = eye_w - center_w;
 *              A = du*du + dw*dw.  A == 0 (the ray is parallel to the axis): a miss unless
 *              ou*ou + ow*ow < r*r, else s0 = -inf, s1 = +inf.  Otherwise B = ou*du + ow*dw,
 *              C = (ou*ou + ow*ow) - r*r, disc = B*B - A*C, a miss unless disc >= 0, s = sqrtf(disc),
 *              s0 = (-B - s) / A, s1 = (-B + s) / A.  Cap slab on a: near_a, far_a.
 *              side = s0 >= near_a (on equal bounds the side wins); t0 = side ? s0 : near_a;
 *              t1 = fminf(s1, far_a).  Side: normal_u = ((eye_u + t * d_u) - center_u) / r, normal_w
 *              likewise, normal_a = 0.  Cap: normal_a = d_a > 0 ? -1 : 1, the other two 0.
 *   wedge      n = center, off = radius.  The box's b0 = fmaxf(fmaxf(near_x, near_y), near_z) and
 *              b1 = fminf(fminf(far_x, far_y), far_z); g = (n0*d0 + n1*d1) + n2*d2,
 *              f = ((n0*eye0 + n1*eye1) + n2*eye2) - off.  g < 0: near_p = (-f) / g, far_p = +inf.
 *              g > 0: near_p = -inf, far_p = (-f) / g.  Otherwise a miss unless f < 0, else
 *              near_p = -inf, far_p = +inf.  t0 = fmaxf(b0, near_p), t1 = fminf(b1, far_p).  The normal
 *              is the box's (first axis with near_a == t0) when t0 == b0 - a box face wins a tie with
 *              the cut face -, else n as stored.
 *   nearest    the solids in list order; solid i replaces the best so far when it is hit with
 *              t_i < t_best (strictly; t_best starts at +inf): the lower index wins a tie.
 *   composite  the nearest solid takes the pixel when t_solid < depth_fluid, strictly; depth_fluid is
 *              sph_hip_render's depth, +inf on a miss.  The marched box does not clip solids.  Such a
 *              pixel gets: rgba by the renderer's shade formula with the solid's normal, rp->light, the
 *              solid's albedo (solid_albedo_rgb[3 * i ..], or sp->albedo for every solid when
 *              n_albedo == 0) and sp->ambient / sp->diffuse, alpha 255; depth = t_solid; normal_xyz =
 *              the solid's normal; velocity_xyz = the solid's velocity with SPH_HIP_RENDER_VELOCITY,
 *              else 0; first_inside = -1; solid_id = i.  Every other pixel keeps sph_hip_render's
 *              outputs bit for bit and gets solid_id = -1.
 *   velocity   of solid i: its motion's velocity while start <= tau < stop on the motion clock (and
 *              the motion moves); a body's velocity V of its device state; otherwise 0.
 * Without obstacles every output equals sph_hip_render's byte for byte and solid_id is -1 everywhere.
 * With obstacles and no particle resident the solids are drawn over `background`.  The call
 * synchronises (it reads the bodies' state when bodies are set) and does not change the simulation:
 * sph_hip_download returns the same bytes before and after it, later steps are bit-identical, the
 * motion clock and the bodies' state are untouched.
 * SPH_HIP_ERR_INVALID, with a last_error text that names sph_hip_render_scene, for everything
 * sph_hip_render refuses, null scene params, a scene params field or a solid's albedo that is not
 * finite, an n_albedo that is neither 0 nor the obstacle count (or a null array with n_albedo > 0),
 * and flag bits other than SPH_HIP_RENDER_VELOCITY.
 * This entry point was added without a change of SPH_HIP_ABI_VERSION: no existing struct and no
 * existing prototype changed.  A host that must run with older libraries looks the symbol up. */
typedef struct sph_hip_scene_params {   /* field order is ABI: 20 bytes */
   float albedo[3];       /* of every solid without an entry in solid_albedo */
   float ambient, diffuse;
} sph_hip_scene_params;

int sph_hip_render_scene(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                         const sph_hip_scene_params* sp, const float* solid_albedo_rgb /* 3n or NULL */,
                         int n_albedo, int width, int height, int flags,
                         uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz,
                         int32_t* first_inside, int32_t* solid_id);

/* ---- scalar renderer ----------------------------------------------------------------------- *
 *
 * The frame of sph_hip_render_scene - of sph_hip_render when sp is NULL - in which every pixel that
 * shows fluid is coloured by one carried channel (carried scalars, below) through a colour table.
 * The fluid pass and the solids pass are the two renderers', unchanged; a pass of its own (k_tint_surface
 * or k_tint_column) then overwrites rgba on the fluid pixels and writes `scalar`.  csrc/tint_policy.h
 * holds the functions, one set for the device and the host.  All arithmetic is fp32, unfused, in the
 * order written; fminf / fmaxf follow C99.
 *   pixels     a pixel whose first_inside >= 0 after the fluid pass and the solids pass is a fluid hit
 *              that no solid took: it is tinted.  Every other pixel keeps the bits of
 *              sph_hip_render_scene (with sp NULL: of sph_hip_render, and solid_id is -1 everywhere) and
 *              its scalar is 0.
 *   ray        d, tnear, tfar and t_k = tnear + (float)k * step exactly as the renderer forms them;
 *              t_hit is the depth output; p_hit = eye + t_hit * d per component.
 *   walk       walk(p) is the scalar sampler's walk over the sampler's members in canonical order:
 *              rho = sum of t_j, a_c = sum of t_j * T_j,c, count - what sph_hip_sample_scalars_points
 *              forms at p, on the channels staged by sorted slot once per call.
 *   SURFACE    v = rho > 0 ? a_channel / rho : 0 at p_hit: the value sph_hip_sample_scalars_points
 *              returns there.
 *   COLUMN     A = 0.0f; for k = first_inside, first_inside + 1, ... while t_k <= tfar and
 *              k < max_samples: (rho, a) = walk(eye + t_k * d); if rho > iso (strictly; NaN is outside)
 *              A = A + (rho > 0 ? a_channel / rho : 0) * step.  v = A: the channel integrated along the
 *              ray through the fluid; with a channel that is 1 everywhere, the fluid's thickness.
 *              The marched box clips the column.  Solids do NOT: particles do not stand inside solids,
 *              so a solid contributes nothing, but the fluid behind a solid that the ray passes through
 *              after its fluid hit is added.  (A sample in a cell the renderer's occupancy map leaves
 *              unmarked has rho exactly +0 and is outside: its walk is skipped, which changes no bit;
 *              SPH_HIP_RENDER_NOSKIP=1 walks every sample.)
 *   map        u = (v - lo) / (hi - lo); u = fminf(fmaxf(u, 0.0f), 1.0f) (a NaN value lands on row 0);
 *              x = u * (float)(n_colors - 1); i = (int)x, lowered to n_colors - 2 where larger;
 *              fr = x - (float)i; col_c = t[i][c] + fr * (t[i+1][c] - t[i][c]), t = table_rgb.
 *   shade      w = 1.0f with SPH_HIP_TINT_FLAT, else the renderer's w = ambient + diffuse * fmaxf(ndl, 0.0f)
 *              from normal_xyz as stored and rp->light; channel c = the renderer's byte of col_c * w,
 *              alpha 255.  scalar = v.  FLAT exists for cut views: clipping `box` to half the tank makes
 *              rays enter inside the fluid (first_inside == 0), where the density gradient is no surface
 *              normal.
 * The call synchronises and changes nothing: sph_hip_download, sph_hip_get_scalars, the motion clock, the
 * bodies' state and every later step are bit-identical to a run without it.  With no particle resident
 * the frame is the scene's and scalar is 0.
 * SPH_HIP_ERR_INVALID, with a last_error text that names sph_hip_render_scalars, for everything
 * sph_hip_render_scene refuses (but sp may be NULL), a non-null albedo array or n_albedo != 0 with a
 * null sp, a context that carries no scalars, null tp or table_rgb, a channel outside 0 .. 3, an unknown
 * mode, unknown tint flag bits, n_colors outside [2, 256], a lo, hi or table entry that is not finite,
 * and lo >= hi.
 * This entry point was added without a change of SPH_HIP_ABI_VERSION: no existing struct and no
 * existing prototype changed. */
#define SPH_HIP_TINT_SURFACE 0
#define SPH_HIP_TINT_COLUMN  1
#define SPH_HIP_TINT_FLAT    1          /* flag: no Lambert factor */
#define SPH_HIP_TINT_MAX_COLORS 256
typedef struct sph_hip_tint_params {    /* field order is ABI: 24 bytes */
   int32_t channel;     /* 0 .. 3 */
   int32_t mode;        /* SPH_HIP_TINT_SURFACE or SPH_HIP_TINT_COLUMN */
   float lo, hi;        /* the values mapped onto the table's ends; lo < hi */
   int32_t n_colors;    /* 2 .. 256 rows of table_rgb */
   int32_t flags;       /* SPH_HIP_TINT_FLAT or 0 */
} sph_hip_tint_params;

int sph_hip_render_scalars(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                           const sph_hip_scene_params* sp /* NULL: fluid only */,
                           const float* solid_albedo_rgb /* 3n or NULL */, int n_albedo,
                           const sph_hip_tint_params* tp, const float* table_rgb /* 3 * n_colors */,
                           int width, int height, int flags, uint8_t* rgba, float* depth, float* normal_xyz,
                           float* velocity_xyz, int32_t* first_inside, int32_t* solid_id,
                           float* scalar /* one per pixel, may be NULL */);

/* ---- static obstacles --------------------------------------------------------------------- *
 *
 * Analytic solids inside the domain: spheres, axis-aligned boxes, axis-aligned capped
 * cylinders and wedges (an axis-aligned box cut by one plane: ramps, beaches, weirs), in position
 * units (those of mPosition and max_x/y/z).  No counterpart in the reference's step: the response
 * generalises SPH::applyBoundary (src/sph.cpp:1124-1148), which the reference applies to the six
 * walls only.  Inside integrate, after the drift, the kick and the wall
 * handling (apply_walls), every obstacle in list order tests the particle's new position strictly
 * (on the surface is outside) and, when it is inside, reflects the particle where the line from its
 * old position along its new velocity enters the obstacle and moves it on for the rest of the step
 * scaled by mDamping (the time left is clamped at 0), or, when that line gives no valid entry,
 * moves it to the nearest surface point and reflects an inward velocity component only.  The
 * operation-by-operation contract is in csrc/obstacle_policy.h.  The KE term of sph_hip_get_energy
 * uses the final velocity.  Obstacles carry no density or pressure (the walls do not either); they
 * stand still unless sph_hip_set_obstacle_motion gives them a velocity (moving obstacles, below).
 *   sphere    center, radius.
 *   box       lo, hi.
 *   cylinder  axis (0 x, 1 y, 2 z), center (its axis component is ignored), radius, and its caps at
 *             lo[axis], hi[axis].
 *   wedge     the box lo < x < hi intersected with the half-space n.x < d: the unit normal n of the
 *             cut face, pointing out of the solid, in center[0..2]; d in radius; axis is ignored.
 *             n.x is always (n0*x0 + n1*x1) + n2*x2.  A plane that cuts nothing off is allowed (the
 *             solid is the box); one that leaves nothing is refused.  Moved by a motion or as a body,
 *             lo and hi get the shift D, n stays and d = d + ((n0*D0 + n1*D1) + n2*D2).
 * sph_hip_set_obstacles replaces the whole list (n = 0 clears it), ordered on the context's stream:
 * steps enqueued before the call keep the old list; `list` may be reused as soon as it returns.  It
 * is refused with SPH_HIP_ERR_INVALID, and the previous list kept, for an unknown kind, a field that
 * is not finite (unused fields included), a radius that is not > 0, lo >= hi on a used axis, a
 * cylinder axis outside 0..2, a wedge normal with | |n|^2 - 1 | > 2^-20 (in double from the float
 * fields), a wedge none of whose box's eight corners c has n.c < d (in double), n < 0,
 * n > SPH_HIP_MAX_OBSTACLES, a null list with n > 0, and on a slab between
 * sph_hip_slab_step_begin and sph_hip_slab_step_end.  Valid in REF, FULL and FULL_FAST and on slab
 * contexts; without obstacles every step is bit-identical to one on a context that never had any.
 * sph_hip_get_obstacles copies up to `capacity` entries to `out` (NULL with capacity 0) and returns
 * how many the context holds (or a negative status).
 * SPH_HIP_OBSTACLE_WEDGE was added without a change of SPH_HIP_ABI_VERSION: no struct and no prototype
 * changed; a library without it refuses the kind as unknown. */
#define SPH_HIP_OBSTACLE_SPHERE   0
#define SPH_HIP_OBSTACLE_BOX      1
#define SPH_HIP_OBSTACLE_CYLINDER 2
#define SPH_HIP_OBSTACLE_WEDGE    3
#define SPH_HIP_MAX_OBSTACLES     64
typedef struct sph_hip_obstacle {   /* field order is ABI: 48 bytes */
   int32_t kind;                    /* SPH_HIP_OBSTACLE_* */
   int32_t axis;                    /* cylinder only */
   float center[3];                 /* sphere, cylinder; wedge: the cut face's unit normal */
   float radius;                    /* sphere, cylinder; wedge: the plane's offset d */
   float lo[3], hi[3];              /* box, wedge; cylinder: its caps on `axis` */
} sph_hip_obstacle;
int sph_hip_set_obstacles(sph_hip_context* ctx, const sph_hip_obstacle* list, int n);
int sph_hip_get_obstacles(sph_hip_context* ctx, sph_hip_obstacle* out, int capacity);

/* ---- moving obstacles ---------------------------------------------------------------------- *
 *
 * Pistons, gates and paddles: obstacle i of the list translates at motion i's constant velocity
 * while the context's motion clock tau is between `start` and `stop`, and rests before and after.
 * The fluid does not act back on it.  The operation-by-operation contract is in
 * csrc/obstacle_policy.h: the obstacle at tau is the list entry shifted by
 * velocity * (clamp(tau, start, stop) - start), and a particle that ends its step inside the obstacle
 * as it stands at the end of the step gets the static response in the frame that moves with the solid
 * during the step - a piston moving at u into fluid at rest leaves it at 2u along its normal.  An
 * entry whose velocity is zero is used exactly as without motions.  The loads (below) record a moving
 * obstacle's turn with the world velocities before and after it.
 *   motion clock  one fp32 value per context, kept on the host.  A successful
 *                 sph_hip_set_obstacle_motion sets it to 0.  Every integrate enqueued while some entry
 *                 moves - sph_hip_step, sph_hip_run, sph_hip_integrate, sph_hip_slab_step_end,
 *                 sph_hip_slab_comm_run - takes tau0 = tau and tau1 = tau + time_step (fp32 add, the
 *                 time step in force) and leaves tau = tau1; both launches of a slab's early-exchange
 *                 step get the same pair.  The pair reaches the kernels by value: nothing synchronises
 *                 for it, and steps already queued keep theirs.  Slab contexts given the same motions
 *                 advance in lock-step and agree.
 * sph_hip_set_obstacle_motion: n is the current obstacle count, or 0 to clear all motions; ordered on
 * the context's stream like sph_hip_set_obstacles.  Refused with SPH_HIP_ERR_INVALID, the previous
 * motions and clock kept, for a velocity that is not finite, a start that is not finite or not >= 0,
 * stop < start or a NaN stop (stop may be +INFINITY), an n that is neither 0 nor the obstacle count,
 * a null list with n > 0, and on a slab between sph_hip_slab_step_begin and sph_hip_slab_step_end.
 * sph_hip_set_obstacles clears all motions and the clock.
 * sph_hip_get_obstacle_motion copies up to `capacity` motions to `out`, the clock to *clock (either
 * may be NULL) and returns how many motions are set (0 or the obstacle count).
 * sph_hip_get_obstacles keeps returning the list as it was set; sph_hip_get_obstacles_now returns it
 * displaced to the current clock (computed on the host by the function the device uses).
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no existing
 * prototype changed. */
typedef struct sph_hip_obstacle_motion {   /* field order is ABI: 20 bytes */
   float velocity[3];               /* position units per unit of time_step */
   float start, stop;               /* on the motion clock; stop may be +INFINITY */
} sph_hip_obstacle_motion;
int sph_hip_set_obstacle_motion(sph_hip_context* ctx, const sph_hip_obstacle_motion* list, int n);
int sph_hip_get_obstacle_motion(sph_hip_context* ctx, sph_hip_obstacle_motion* out, int capacity, float* clock);
int sph_hip_get_obstacles_now(sph_hip_context* ctx, sph_hip_obstacle* out, int capacity);

/* ---- motion paths -------------------------------------------------------------------------- *
 *
 * Wavemakers, lifted gates, sloshing walls, paddles driven by a measured record: obstacle i of the list
 * follows path i, a piecewise linear displacement given by keys (t, d) on the motion clock.  The fluid
 * does not act back on it.  The operation-by-operation contract is in csrc/obstacle_policy.h (fourth
 * part), all of it fp32, unfused, in the order written:
 *   ownership  path i belongs to obstacle i; count == 0: no path, the entry takes exactly the turn it
 *              takes without this call (static, or its motion's).  Otherwise its keys are
 *              keys[first .. first + count), t[0] == 0 and t strictly increasing.
 *   path time  T = t[count-1]; u = tau - start, u < 0 becomes 0.  cycle == 0: u > T becomes T.
 *              cycle != 0: if u >= T then k = floorf(u / T), u = u - k * T; after that u < 0 becomes 0
 *              and u >= T becomes 0 (the path repeats with period T).
 *   segment    j: the largest index in [0, count-2] with t[j] <= u.
 *   shift      w = (u - t[j]) / (t[j+1] - t[j]); D_c(tau) = d[j][c] + w * (d[j+1][c] - d[j][c]).  The
 *              obstacle at tau is the list entry shifted by D as a moving obstacle is (a wedge's plane
 *              offset moves with it).  An entry with a path is always shifted, also by D == 0.
 *   turn       D0 = D(tau0), D1 = D(tau1) for the step's clock pair; the moving obstacle's response
 *              with these two shifts: a particle that ends the step inside the obstacle as it stands at
 *              tau1 gets the static response in the frame that moves with the solid during the step.
 *              The loads record the turn as they record a moving entry's.
 *   velocity   (scene renderer) (d[j+1] - d[j]) / (t[j+1] - t[j]) per component of the segment in force
 *              at the clock; 0 before `start` and after the end of a path that does not cycle.
 *   clock      the motion clock of the moving obstacles.  A successful sph_hip_set_obstacle_paths sets it
 *              to 0; it advances with every integrate enqueued while some entry moves or has a path.
 * The shifts of a step are formed on the device by one single-wave launch in front of the step's
 * integrate (lane i = obstacle i), from the clock pair it gets by value: queued steps stay queued and
 * nothing synchronises.  It runs also when the context holds no particle.
 * sph_hip_set_obstacle_paths: n is the obstacle count, or 0 to clear all paths; `keys` holds the n_keys
 * keys of all paths, at most SPH_HIP_MAX_PATH_KEYS; ordered on the context's stream like
 * sph_hip_set_obstacles.  Refused with SPH_HIP_ERR_INVALID, the previous paths and clock kept: an n that
 * is neither 0 nor the obstacle count; null lists with counts > 0; n_keys outside
 * [0, SPH_HIP_MAX_PATH_KEYS]; count == 1 or count < 0; a range that leaves [0, n_keys); t[0] != 0; t not
 * strictly increasing or not finite; a d that is not finite; a start that is not finite or < 0; a
 * cyclic path whose last d differs from its first in any component; a path on an obstacle whose motion
 * moves (and sph_hip_set_obstacle_motion then refuses a moving motion on an obstacle with a path); any
 * path in a list that holds a free body (and sph_hip_set_bodies then refuses a body in a list with
 * paths); any slab context - paths on slabs are not built -; between sph_hip_slab_step_begin and _end.
 * A context with paths refuses sph_hip_slab_pack, _unpack and _step_begin.  Rotations are not built.
 * sph_hip_set_obstacles clears the paths as it clears the motions.
 * sph_hip_get_obstacle_paths copies up to `capacity` paths and `key_capacity` keys (either array may be
 * NULL) and returns how many paths are set (0 or the obstacle count).  With `shifts` non-null it
 * synchronises and copies, for every obstacle of the list, the D0 and D1 the device used in the last
 * enqueued step (six floats per obstacle; zeros for an entry without a path, and before the first step
 * after a set).  sph_hip_get_obstacles_now shifts an entry with a path to the current clock on the host,
 * by the function the device uses.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no
 * existing prototype changed. */
#define SPH_HIP_MAX_PATH_KEYS 16384     /* over all paths of a context */
typedef struct sph_hip_motion_key {     /* field order is ABI: 16 bytes */
   float t;                         /* on the path's own time: t[0] == 0, strictly increasing */
   float d[3];                      /* the displacement at t, position units */
} sph_hip_motion_key;
typedef struct sph_hip_motion_path {    /* field order is ABI: 16 bytes */
   int32_t first, count;            /* keys[first .. first + count); count == 0: no path */
   float start;                     /* the motion clock at which the path begins */
   int32_t cycle;                   /* != 0: repeat with period t[count-1] */
} sph_hip_motion_path;
int sph_hip_set_obstacle_paths(sph_hip_context* ctx, const sph_hip_motion_path* paths, int n,
                               const sph_hip_motion_key* keys, int n_keys);
int sph_hip_get_obstacle_paths(sph_hip_context* ctx, sph_hip_motion_path* paths, int capacity,
                               sph_hip_motion_key* keys, int key_capacity, float* shifts);

/* ---- loads on walls and obstacles --------------------------------------------------------- *
 *
 * The impulse the fluid gives to each domain wall and each obstacle, step by step, summed on the
 * device.  No counterpart in the reference.  The operation-by-operation contract is in
 * csrc/load_policy.h.
 *   solids     column s of a row: 0..5 the walls x-lo, x-hi, y-lo, y-hi, z-lo, z-hi; 6 + i obstacle i
 *              of the list in force when the step was enqueued.  A row always has
 *              SPH_HIP_LOAD_SOLIDS columns; unused ones stay zero.
 *   response   one wall reflection of integrate (apply_walls), or one obstacle's turn at a particle
 *              whose new position is inside it.  With vb / va the particle's velocity just before /
 *              after it and m its mass: j_c = m * (vb_c - va_c) per component in fp32, the impulse
 *              given to the solid.
 *   sum        s_c = (double)j_c * 2^(-quantum_log2).  If the three s_c are finite and below 2^38 in
 *              magnitude, llrint(s_c) (ties to even) is added to impulse[s][c] and 1 to count[s];
 *              otherwise nothing is added and skipped[s] grows by 1.  All accumulators are int64:
 *              a row is the same for every thread order, every route (sph_hip_step, sph_hip_run, the
 *              phase calls) and every number of slabs (add the slabs' rows), and REF, FULL and
 *              FULL_FAST differ only by what their velocities differ by.  impulse * 2^quantum_log2 is
 *              the impulse in mass * velocity units; divided by time_step, the mean force of the step.
 *              The default quantum_log2 = -24 suits unit masses: terms up to 16384 are kept.
 * sph_hip_record_loads allocates and zeroes `rows` rows on the context's stream and restarts at row
 * 0; rows = 0 stops recording and frees them.  Row r belongs to the r-th integrate enqueued after the
 * call, whichever way (sph_hip_step, sph_hip_run, sph_hip_integrate, sph_hip_slab_step_end,
 * sph_hip_slab_comm_run); no step synchronises for it.  Only owned particles are recorded, once.  While
 * rows are left the context integrates in a kernel of its own behind the acceleration pass
 * (k_integrate_loads); once they are used up, steps are not recorded and take their usual routes.  A
 * recording changes no particle: positions, velocities and energies are bit-identical to a run
 * without it.  SPH_HIP_ERR_INVALID, the previous recording kept, for rows < 0, quantum_log2 outside
 * [-64, 32], and on a slab between sph_hip_slab_step_begin and sph_hip_slab_step_end;
 * SPH_HIP_ERR_CAPACITY when the rows cannot be allocated.
 * sph_hip_get_loads synchronises and copies rows [first_row, first_row + n_rows) to host arrays, any of
 * which may be NULL; *rows_recorded = rows filled so far.  SPH_HIP_ERR_INVALID when nothing is being
 * recorded or the range leaves the allocated rows.
 * These two entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no
 * existing prototype changed.  A host that must run with older libraries looks the symbols up. */
#define SPH_HIP_LOAD_SOLIDS (6 + SPH_HIP_MAX_OBSTACLES)
int sph_hip_record_loads(sph_hip_context* ctx, int rows, int quantum_log2);
/* impulse[n_rows][SPH_HIP_LOAD_SOLIDS][3], count[n_rows][SPH_HIP_LOAD_SOLIDS], skipped likewise */
int sph_hip_get_loads(sph_hip_context* ctx, int first_row, int n_rows, int64_t* impulse, int64_t* count,
                      int64_t* skipped, int32_t* rows_recorded);

/* ---- free bodies ---------------------------------------------------------------------------- *
 *
 * Obstacles that the fluid's own loads set in motion: debris, a float, a gate the water opens.  Body
 * i of the list belongs to obstacle i; an entry with mass == 0 is not a body and behaves exactly as
 * without this call, at rest or under its motion.  A body translates (no rotation, no contact between
 * bodies); its state lives on the device and is advanced by one single-wave launch per step, so queued
 * steps stay queued.  The operation-by-operation contract is in csrc/body_policy.h:
 *   state      per obstacle: the displacement D at the end of the last enqueued step, Dprev at its
 *              start, the velocity V, and two int64 counters, skipped and steps.  All zero when bodies
 *              are set, except V = velocity on the free components.
 *   advance    once per step, before that step's integrate, from the load row the previous integrate
 *              filled (column 6 + i; the first step after sph_hip_set_bodies has no such row and takes a
 *              zero impulse).  Dprev = D; per free component c, in fp32, unfused:
 *              J = (float)((double)impulse_q[6 + i][c] * 2^quantum_log2); V_c = V_c + J / mass;
 *              V_c = V_c + accel_c * time_step; D_c = D_c + V_c * time_step; D_c < travel_lo[c]:
 *              D_c = travel_lo[c], V_c = 0; D_c > travel_hi[c]: D_c = travel_hi[c], V_c = 0.  A
 *              component that is not free keeps V_c = 0 and D_c = 0.  skipped grows by the row's skipped
 *              count of that column, steps by 1.
 *   response   inside integrate, the body's turn is the moving obstacle's with the shifts Dprev and D
 *              (obstacle_respond_moved), and the loads record it as they record a moving entry.
 *   lag        the coupling is explicit: the impulse received in step k changes the velocity used in
 *              step k + 1.  Within a step the response treats the solid as infinitely heavy, so a body
 *              much lighter than the fluid that touches it in one step oscillates: use heavy bodies.
 *   quantum    sph_hip_set_bodies fixes the quantum of the rows the bodies consume.  A context with
 *              bodies always records: into the caller's row while a recording has rows left, otherwise
 *              into one of two internal rows.  While bodies are set, sph_hip_record_loads with rows > 0
 *              and another quantum is refused; sph_hip_set_bodies is refused while a recording with
 *              another quantum has rows left.  A recording therefore still changes no particle and no
 *              body.
 * sph_hip_set_bodies: n is the obstacle count, or 0 to clear the bodies; ordered on the context's stream
 * like sph_hip_set_obstacles.  Refused with SPH_HIP_ERR_INVALID, the previous bodies and their state
 * kept: an n that is neither; a null list with n > 0; quantum_log2 outside [-64, 32]; for an entry with
 * mass != 0, a mass that is not finite and > 0, a velocity or accel that is not finite, free_axes with
 * a bit above bit 2, travel_lo[c] <= 0 <= travel_hi[c] not holding (infinities are allowed); a body on
 * an entry whose motion moves (and sph_hip_set_obstacle_motion refuses a moving motion on a body); the
 * quantum rule above; any slab context (a body needs the sum of all slabs' rows before any slab may
 * advance it: one all-reduce per step, which is not built); between sph_hip_slab_step_begin and _end.
 * A context with bodies refuses sph_hip_slab_pack, _unpack and _step_begin.
 * sph_hip_set_obstacles clears the bodies, as it clears the motions.
 * sph_hip_get_bodies synchronises, copies up to `capacity` entries to `list` and `state` (either may be
 * NULL) and returns how many entries are set (0 or the obstacle count).  sph_hip_get_obstacles_now adds
 * a body's displacement to its obstacle and synchronises only when bodies are set.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no
 * existing prototype changed. */
typedef struct sph_hip_body {       /* field order is ABI: 56 bytes */
   float mass;                      /* 0: not a body */
   float velocity[3];               /* initial velocity, position units per unit of time_step */
   float accel[3];                  /* body force per unit mass (gravity, say); the caller states it */
   uint32_t free_axes;              /* bit c: component c may move */
   float travel_lo[3], travel_hi[3];/* limits of the displacement: the stops */
} sph_hip_body;
typedef struct sph_hip_body_state { /* field order is ABI: 40 bytes */
   float displacement[3];
   float velocity[3];
   int64_t skipped;                 /* responses the rows it consumed had left out */
   int64_t steps;                   /* advances so far */
} sph_hip_body_state;
int sph_hip_set_bodies(sph_hip_context* ctx, const sph_hip_body* list, int n, int quantum_log2);
int sph_hip_get_bodies(sph_hip_context* ctx, sph_hip_body* list, sph_hip_body_state* state, int capacity);

/* ---- tracers --------------------------------------------------------------------------------- *
 *
 * Massless markers the fluid carries: pathlines, a dye front, residence times.  FULL mode keeps the
 * particles cell-sorted, so a particle's place in memory says nothing about its path; a tracer is a point
 * of its own - x[3], int32 wet_steps, int32 dry_steps - that lives on the device and is advanced inside
 * every step, so that queued steps stay queued.  No counterpart in the reference.  The operation-by-
 * operation contract is in csrc/tracer_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   contexts   FULL and FULL_FAST contexts that hold the whole grid: what the field sampler accepts, with
 *              the sampler's refusals for REF and slab contexts.
 *   advance    step k advances every tracer once, after that step's cell build and before anything moves
 *              the particles, in the state S_k the sampler would see at that moment, with the particles'
 *              displacement step pos_dt = time_step * sim_scale_inv (the integrate moves a particle by
 *              vh * pos_dt; at unit scale pos_dt is time_step itself) - one fp32 product of the parameters
 *              in force when the step is enqueued (by value: a later setter does not reach queued steps).
 *              sample(S, p) is sph_hip_sample_points at p: Shepard velocity u and member count c.
 *                1  (u1, c1) = sample(S_k, x)
 *                2  c1 == 0: the tracer is dry this step - x unchanged, dry_steps += 1, done
 *                3  half = 0.5f * pos_dt; xm_c = x_c + u1_c * half; (u2, c2) = sample(S_k, xm);
 *                   u = c2 > 0 ? u2 : u1
 *                4  y_c = x_c + u_c * pos_dt; if any y_c is not finite the tracer is dry as in 2
 *                5  apply_walls: y_c < 0 gives y_c = 0, y_c > max_c gives y_c = max_c - a clamp, not the
 *                   particles' reflection: a marker has no momentum
 *                6  x = y; wet_steps += 1
 *              The midpoint rule in the velocity field frozen at the start of the step.  Tracers read
 *              positions, masses and velocities of S_k only and never write anything a particle kernel
 *              reads: every particle, density, acceleration and energy is bit-identical to a run without
 *              tracers.  sph_hip_step, sph_hip_run and the phase calls give the same tracer bits: the
 *              stand-alone sph_hip_integrate advances the tracers first, after bringing the cell structure
 *              up to date as the sampler does.  With no particle resident every tracer is dry.
 *   order      the device keeps the tracers in slots that carry their ids and re-sorts the slots by FULL
 *              cell id now and then (SPH_HIP_TRACER_SORT=n, read at creation: every n steps, 0 never); no
 *              result depends on the slot order, and every array below is in the order given to
 *              sph_hip_set_tracers.
 *   not done   solids do not stop a tracer: one that ends inside an obstacle finds no members there and
 *              stays dry.  Slab contexts and REF mode are refused.  Tracers do not interact.
 * sph_hip_set_tracers replaces the set (n = 0 clears it) with zeroed counts, ends a recording and waits
 * for the steps already queued.  SPH_HIP_ERR_INVALID, the old set kept, for n < 0, a null array with
 * n > 0, a coordinate that is not finite, and a REF or slab context.  The set survives sph_hip_upload,
 * sph_hip_set_params and sph_hip_set_arithmetic.
 * sph_hip_get_tracers synchronises and copies tracers [first, first + n); any output may be NULL.
 * sph_hip_tracer_count returns how many tracers are set.
 * sph_hip_record_tracers keeps the positions after recorded steps on the device: steps are numbered
 * 1, 2, ... from this call, row r holds the positions after step 1 + r * every, for r < rows - the next
 * step, then every every-th.  rows = 0 stops and frees the recording.  SPH_HIP_ERR_INVALID, the previous
 * recording kept, for rows < 0, every < 1, and rows * count * 12 bytes above the 64 MiB scratch budget of
 * the sampler and the extractor.
 * sph_hip_get_tracer_path synchronises, copies rows [first_row, first_row + n_rows) of the rows filled so
 * far - xyz[n_rows][count][3] by tracer id, step_index[n_rows] the step numbers; either may be NULL - and
 * returns how many rows are filled (n_rows = 0 asks just that).  SPH_HIP_ERR_INVALID for a range that
 * leaves the filled rows.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no existing
 * prototype changed. */
int sph_hip_set_tracers(sph_hip_context* ctx, int n, const float* xyz);
int sph_hip_get_tracers(sph_hip_context* ctx, int first, int n, float* xyz, int32_t* wet_steps, int32_t* dry_steps);
int sph_hip_tracer_count(const sph_hip_context* ctx);
int sph_hip_record_tracers(sph_hip_context* ctx, int rows, int every);
int sph_hip_get_tracer_path(sph_hip_context* ctx, int first_row, int n_rows, float* xyz, int32_t* step_index);

/* ---- gauges ---------------------------------------------------------------------------------- *
 *
 * Fixed instruments that read the field inside the step: the water level at a station, the velocity at a
 * point, the discharge through an opening - the time series a dam-break experiment publishes - without a
 * host that samples once per step and drains the queue.  A gauge lives in the context; one wave of 64
 * lanes evaluates its probe points on the device and reduces them to one reading, and a recording keeps
 * one device row of readings per recorded step.  No counterpart in the reference.  The operation-by-
 * operation contract is in csrc/gauge_policy.h; all arithmetic is fp32, unfused, in the order written.
 * walk(S, p) is the field sampler's walk at p over the state S: the raw sums rho, vx, vy, vz (each member's
 * term t_j and t_j * v_j, in canonical order) and the member count, before any normalisation.
 *   kinds      POINT    one probe at origin.  v = {rho, ux, uy, uz} with the sampler's normalisation
 *                       (rho > 0 ? vx / rho : 0), n = count, k = 0: sph_hip_sample_points there, bit for bit.
 *              COLUMN   count[0] = m probes up `axis` from the base: probe k is the origin with coordinate
 *                       `axis` replaced by p_k = origin[axis] + (float)k * spacing[0].  A probe is wet when
 *                       rho > iso (strictly; NaN is dry).  n = the wet probes, k = the largest wet index or
 *                       -1, v[1] = (float)n * spacing[0] (the wet depth), v[0] the level:
 *                         k == -1:    v[0] = origin[axis], v[2] = 0, v[3] = rho_0
 *                         k == m - 1: v[0] = p_k, v[2] = rho_k, v[3] = 0
 *                         otherwise   fa = rho_k, fb = rho_(k+1), t = (iso - fa) / (fb - fa) clamped to
 *                                     [0, 1] by fminf(fmaxf(t, 0), 1) (NaN becomes 0, the extractor's rule),
 *                                     v[0] = p_k + t * (p_(k+1) - p_k), v[2] = fa, v[3] = fb
 *              SECTION  count = {nu, nv} probes on the rectangle with normal `axis` through origin: probe
 *                       q = j * nu + i has the first other axis (ascending axis order) at origin[u] +
 *                       (float)i * spacing[0] and the second at origin[v] + (float)j * spacing[1].  Lane l of
 *                       the wave takes the probes l, l + 64, ... in order into two accumulators that start
 *                       at 0.0f: a = a + (the raw velocity sum of the normal axis, the momentum density
 *                       sum of t_j v_j), r = r + rho; the 64 lane values are summed by the butterfly
 *                       x = x + x[lane ^ d], d = 1, 2, 4, 8, 16, 32.  area = spacing[0] * spacing[1];
 *                       v = {a_sum * area (the mass flow along the normal), (float)n * area (the wetted
 *                       area), r_sum, 0}, n = the wet probes, k = 0.
 *   contexts   FULL and FULL_FAST contexts that hold the whole grid, with the sampler's refusals for REF
 *              and slab contexts.  With no particle resident every walk gives zeros: columns are dry.
 *   when       while a recording is set, step k evaluates the gauges once, after that step's cell build and
 *              before anything moves the particles, in the state S_k the sampler would see.  Gauges read
 *              positions, masses and velocities only and write nothing a particle kernel reads: every
 *              particle, density, acceleration and energy is bit-identical to a run without gauges.
 *              sph_hip_step, sph_hip_run and the phase calls give the same bits: the stand-alone
 *              sph_hip_integrate reads the gauges first, after bringing the cell structure up to date as
 *              the sampler does.  With no recording a step launches nothing for gauges.
 *   pressure   PRESSURE and PRESSURE_PATCH read the pressure field (below: pressure readings); they take the
 *              values 4 and 5 - 3 stays refused as an unknown kind, which callers and tests rely on.
 *   not done   slab contexts and REF mode are refused; pressures are not clamped or density-corrected; gauges
 *              do not move with an obstacle or a body, and solids do not shade a probe.
 * sph_hip_set_gauges replaces the set (n = 0 clears it), ends a recording and waits for the steps already
 * queued.  SPH_HIP_ERR_INVALID, the previous set and recording kept, for a REF or slab context, n < 0,
 * n > SPH_HIP_MAX_GAUGES, a null list with n > 0, an unknown kind, an axis outside 0..2, any float field
 * that is not finite (unused fields included), a used spacing that is not > 0, a used count < 1, more than
 * SPH_HIP_MAX_GAUGE_PROBES probes in one gauge, and an iso that is not > 0 for COLUMN, SECTION and
 * PRESSURE_PATCH.  The
 * set survives sph_hip_upload, sph_hip_set_params and sph_hip_set_arithmetic, and a recording goes on
 * across them.
 * sph_hip_get_gauges copies up to `capacity` gauges and returns how many are set.
 * sph_hip_read_gauges evaluates the gauges now, in the current state, into out[count]: the sampler's kind
 * of call - it brings the cell structure up to date, synchronises and changes nothing a caller can read or
 * a later step computes.  With no gauges set it does nothing.
 * sph_hip_record_gauges keeps `rows` rows of readings on the device: steps are numbered 1, 2, ... from this
 * call, and step s fills row (s - 1) / every when every divides s - 1 and that row exists.  Row r is the
 * state after r * every steps; row 0 is the state at the call.  rows = 0 stops and frees the recording.
 * SPH_HIP_ERR_INVALID, the previous recording kept, for rows < 0, every < 1, rows * gauges * 24 bytes above
 * the 64 MiB scratch budget of the sampler and the extractor, and rows > 0 with no gauges set.
 * sph_hip_get_gauge_record synchronises, copies rows [first_row, first_row + n_rows) of the rows filled so
 * far - out[n_rows][gauges], steps_done[n_rows] = row * every; either may be NULL - and returns how many
 * rows are filled (n_rows = 0 asks just that).  SPH_HIP_ERR_INVALID for a range that leaves the filled rows.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no existing
 * prototype changed. */
#define SPH_HIP_GAUGE_POINT   0
#define SPH_HIP_GAUGE_COLUMN  1
#define SPH_HIP_GAUGE_SECTION 2
#define SPH_HIP_GAUGE_PRESSURE       4  /* (3 is not a kind: it stays "unknown gauge kind") */
#define SPH_HIP_GAUGE_PRESSURE_PATCH 5
#define SPH_HIP_MAX_GAUGES        4096
#define SPH_HIP_MAX_GAUGE_PROBES  4096
typedef struct sph_hip_gauge {      /* field order is ABI: 40 bytes */
   int32_t kind;
   int32_t axis;        /* COLUMN: the axis it climbs; SECTION, PRESSURE_PATCH: its normal; POINT, PRESSURE: 0 */
   float origin[3];     /* POINT, PRESSURE: the point; COLUMN: the base; SECTION, PRESSURE_PATCH: the corner,
                           origin[axis] = the plane */
   float spacing[2];    /* COLUMN: [0]; SECTION, PRESSURE_PATCH: along the two other axes, ascending axis order */
   int32_t count[2];    /* COLUMN: count[0] = m; SECTION, PRESSURE_PATCH: nu, nv */
   float iso;           /* COLUMN, SECTION, PRESSURE_PATCH: a probe is wet when rho > iso (strictly; NaN is dry) */
} sph_hip_gauge;
typedef struct sph_hip_gauge_reading {   /* 24 bytes */
   float v[4];
   int32_t n;
   int32_t k;
} sph_hip_gauge_reading;
int sph_hip_set_gauges(sph_hip_context* ctx, const sph_hip_gauge* list, int n);
int sph_hip_get_gauges(sph_hip_context* ctx, sph_hip_gauge* out, int capacity);
int sph_hip_read_gauges(sph_hip_context* ctx, sph_hip_gauge_reading* out);
int sph_hip_record_gauges(sph_hip_context* ctx, int rows, int every);
int sph_hip_get_gauge_record(sph_hip_context* ctx, int first_row, int n_rows, sph_hip_gauge_reading* out,
                             int32_t* steps_done);

/* ---- pressure readings ------------------------------------------------------------------------ *
 *
 * The pressure at sensors on a wall or an obstacle - the second time series of a dam-break experiment -
 * read on the device: at points and lattices (the two calls below) and by two gauge kinds that are set,
 * read and recorded like the others.  No counterpart in the reference.  The operation-by-operation
 * contract is in csrc/gauge_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   particle   rho_j is the FULL density pass's density of particle j in the state S: the particle itself
 *              excluded, canonical order, the same bits in FULL and FULL_FAST and on every route (tiled,
 *              give-up, SPH_HIP_UNTILED=1).  P_j = (rho_j - rho0) * stiffness, the pressure the
 *              acceleration pass forms, with the context's constants at the time of the call or at the time
 *              the step is enqueued.  P is NOT clamped: it is negative wherever rho_j < rho0, as in the
 *              reference.
 *   probe      over the sampler's members of x with the sampler's terms t_j (a particle at x included):
 *              pw = sum of t_j * P_j in canonical order beside the sampler's rho and count;
 *              pressure = rho > 0 ? pw / rho : 0 - Shepard normalisation, the velocity's rule.  A probe at a
 *              wall has half its support empty: the normalisation is what makes that reading a pressure.
 *              A non-finite or out-of-box probe gives 0, 0, 0 as in the sampler.
 *   kinds      PRESSURE        one probe at origin: v = {pressure, rho, pw, 0}, n = count, k = 0:
 *                              sph_hip_sample_pressure_points there, bit for bit.
 *              PRESSURE_PATCH  a sensor face or wall panel: SECTION's rectangle of probes, the same fields
 *                              and probe order, lane l taking probes l, l + 64, ...  A probe is wet when
 *                              rho > iso (strictly; NaN is dry).  A wet probe adds its pressure (the quotient
 *                              of that probe) to the lane's a and its rho to r, both from 0.0f; a dry or
 *                              missing probe adds nothing; the lanes are summed by SECTION's butterfly.
 *                              area = spacing[0] * spacing[1]; v = {a_sum * area (the force along the normal
 *                              by the pressure integral), (float)n * area (the wetted area),
 *                              n > 0 ? a_sum / (float)n : 0 (the mean pressure over the wet probes), r_sum},
 *                              n = the wet probes, k = 0.
 *   when       in a step that fills a record row the pressure kinds are read after that step's density pass
 *              and before its acceleration pass, from the densities that pass has just formed for the state
 *              S_k the other gauges saw, into the same row; the other kinds are read where they were.
 *              sph_hip_read_gauges, the two calls below and the stand-alone sph_hip_integrate form the
 *              densities of the current state themselves, into a buffer of the context's own (4 bytes per
 *              particle of the capacity, allocated at the first use), and trust no earlier
 *              sph_hip_compute_density: both routes give the same bits.  Queued steps stay queued; no
 *              particle, density, acceleration, count or energy changes by a bit.  A context without a
 *              pressure kind launches what it launched before.
 *   contexts   REF and slab contexts are refused.  With ports or obstacles the pressure kinds do what the
 *              other gauges do: they read the fluid particles resident in that state and nothing else -
 *              solids carry no density and do not shade a probe.
 * sph_hip_sample_pressure_points / _lattice follow sph_hip_sample_points / _lattice: their refusals, any
 * output may be NULL, the lattice's index order, the call synchronises and does not change the simulation.
 * These entry points and kinds were added without a change of SPH_HIP_ABI_VERSION: no struct and no
 * existing prototype changed. */
/* n probes, xyz interleaved; pressure[n], density[n], count[n] */
int sph_hip_sample_pressure_points(sph_hip_context* ctx, int n, const float* xyz, float* pressure, float* density,
                                   int32_t* count);
int sph_hip_sample_pressure_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                    const int32_t dims[3], float* pressure, float* density, int32_t* count);

/* ---- carried scalars ---------------------------------------------------------------------------- *
 *
 * Four channels per particle - a temperature, a dye concentration, a salinity - that move with the fluid,
 * diffuse between neighbours and are read back or sampled.  No counterpart in the reference.  The
 * operation-by-operation contract is in csrc/scalar_policy.h; all arithmetic is fp32, unfused, in the order
 * written.
 *   storage    one row {T0, T1, T2, T3} per particle ID (the upload row), not per sorted slot: the rows never
 *              move, a channel with diffusivity 0 keeps its bits for as long as it is carried.
 *   a step     every sph_hip_step and every queued step of sph_hip_run advances the scalars once, in that
 *              step's state S_k, behind the step's density pass and before anything moves.  For particle i and
 *              every channel c with kappa[c] > 0: sum = over i's neighbours j (the acceleration pass's pairs, in
 *              canonical order) of V_j * (T_j,c - T_i,c) * L(d_ij), T_i,c' = T_i,c + (dt * kappa[c]) * sum, with
 *              V_j = m_j / rho_j (rho_j the density pass's value; a neighbour whose rho_j is not > 0 contributes
 *              nothing) and L(d) = kernel3 * (hscaled - d), the reference's viscosity Laplacian.  A channel with
 *              kappa[c] == 0 is only carried.  The same bits in FULL and FULL_FAST and on every route.
 *   stability  the scheme is explicit: per channel the update is a convex combination of T_i and its
 *              neighbours while dt * kappa[c] * (sum over j of V_j * L(d_ij)) <= 1.  Nothing polices that.
 *              rho_j does not include j itself, so a particle of the spray - its few neighbours all near its
 *              rim - has next to no density and a volume without bound: V_j * L(d) grows like (h - d)^-2
 *              there, no kappa > 0 keeps the step convex next to it, and a diffusing channel can overflow and
 *              spread NaN from there.  A carried channel (kappa 0) is not touched by any of this.
 *   sources    at most SPH_HIP_MAX_SCALAR_SOURCES boxes.  After the update, in list order, a particle whose S_k
 *              position is STRICTLY inside [lo, hi] gets T_channel = value (HOLD: a heated plate, a dye
 *              injector) or T_channel = T_channel + value * dt (ADD: a heater of a given power).
 *   coupling   one way: no particle, density, acceleration, count or energy changes by a bit - unless a
 *              buoyancy is set (buoyancy, below), which is the coupling back and off by default.
 *              Queued steps stay queued.  A context without scalars launches what it launched before.
 *   not done   the stand-alone phase calls (sph_hip_compute_density .. sph_hip_integrate) do NOT advance the
 *              scalars.  REF and slab contexts are refused.  Ports are refused both ways - sph_hip_set_ports
 *              with an emitter or a sink on a context that carries scalars, sph_hip_set_scalars on a context
 *              with ports - an emitter would need a value per layer.
 * sph_hip_set_scalars gives every particle its row (values4: n rows of 4 floats, in ID order) and the
 * channels their diffusivities kappa4[4]; it waits for the steps already queued.  values4 == NULL or n == 0
 * switches the scalars off and drops the sources.  SPH_HIP_ERR_INVALID, the previous state kept, for a REF
 * or slab context, ports, n < 0, n other than the particle count, a value that is not finite, a
 * diffusivity that is not finite and >= 0.  The buffers (36 bytes per particle of the capacity) are
 * allocated at the first call.  A new sph_hip_upload drops the scalars and the sources.
 * sph_hip_get_scalars copies rows first .. first + n - 1, in ID order, after the steps queued so far.
 * sph_hip_set_scalar_sources replaces the sources for the steps enqueued from now on (n = 0 clears them):
 * SPH_HIP_ERR_INVALID for a context that carries no scalars, n < 0, n > SPH_HIP_MAX_SCALAR_SOURCES, a
 * channel outside 0..3, an unknown kind, a box that is not finite or not lo < hi on every axis, a value
 * that is not finite.  sph_hip_get_scalar_sources copies up to `capacity` of them and returns how many are set.
 * sph_hip_sample_scalars_points / _lattice follow sph_hip_sample_points / _lattice - their refusals, any
 * output may be NULL, the lattice's index order, the call synchronises and changes nothing - and return the
 * Shepard-normalised channels, (sum of t_j * T_j,c) / rho where rho > 0, else 0, over the sampler's members
 * and terms, beside the sampler's density and count: channels4 holds 4 floats per probe.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no existing
 * prototype changed. */
#define SPH_HIP_SCALAR_CHANNELS     4
#define SPH_HIP_MAX_SCALAR_SOURCES  8
#define SPH_HIP_SCALAR_HOLD 0
#define SPH_HIP_SCALAR_ADD  1
typedef struct sph_hip_scalar_source {   /* field order is ABI: 36 bytes */
   float lo[3];
   float hi[3];
   int32_t channel;
   int32_t kind;
   float value;
} sph_hip_scalar_source;
int sph_hip_set_scalars(sph_hip_context* ctx, int n, const float* values4, const float* kappa4);
int sph_hip_get_scalars(sph_hip_context* ctx, int first, int n, float* out4);
int sph_hip_set_scalar_sources(sph_hip_context* ctx, const sph_hip_scalar_source* list, int n);
int sph_hip_get_scalar_sources(sph_hip_context* ctx, sph_hip_scalar_source* out, int capacity);
/* n probes, xyz interleaved; channels4[4n], density[n], count[n] */
int sph_hip_sample_scalars_points(sph_hip_context* ctx, int n, const float* xyz, float* channels4, float* density,
                                  int32_t* count);
int sph_hip_sample_scalars_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                   const int32_t dims[3], float* channels4, float* density, int32_t* count);

/* ---- buoyancy ----------------------------------------------------------------------------------- *
 *
 * The carried scalars change a particle's weight: warm water rises over a heated plate, a salinity front
 * slumps.  No counterpart in the reference.  The operation-by-operation contract is in
 * csrc/buoyancy_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   excess     for particle i of a step's state S_k, with T_i its channels as they stood BEFORE that step's
 *              scalar update: s = 0; for c = 0 .. 3: s = s + beta[c] * (T_i,c - reference[c]).
 *   force      b = (-s) * gravity per component: with gravity pointing down a positive beta lifts warm fluid,
 *              a negative one (a salinity) sinks it.  `gravity` is the setting's own vector, not read from the
 *              parameters: it says which way is down, whatever apply_gravity is.
 *   guard      a particle with s == 0, or with s not finite (a diffusing channel can go NaN next to the spray,
 *              see stability above), is left alone: not a bit of it changes, -0.0f included.
 *   a step     behind the step's acceleration pass and before its integrate: a' = clamp(a + b), the
 *              acceleration pass's own cfl_limit rule applied again, and v' = v + b * dt; the step's usual
 *              integrate then runs from (x, v', a').  The acceleration read back after the step is a'.
 *   two terms  the integrate gives a particle's acceleration half a time step of velocity (vh = v + a*dt/2) and
 *              gravity a whole one more (nv = vh + g*dt).  b enters both ways, so that a particle's weight
 *              changes by exactly the factor 1 - s in velocity: with s = 1 and a = gravity, a' = 0 exactly and
 *              nv = (v - g*dt) + g*dt.  The position sees b*dt one step early, an offset of the size of one
 *              step's velocity change, constant over a run.
 *   route      a buoyant context gives up the fused integrate (it keeps the prehash) and launches one more
 *              kernel per step.  Obstacles, motions, paths, bodies, load recordings, gauges and tracers work
 *              beside it unchanged.  A context without buoyancy enqueues exactly what it always did.
 *   not done   the stand-alone phase calls (sph_hip_compute_density .. sph_hip_integrate) do NOT apply
 *              buoyancy, as they do not advance the scalars.
 * sph_hip_set_buoyancy sets it for the steps enqueued from now on; it does not wait, and steps already queued
 * keep the setting they were enqueued with.  b == NULL or a beta of four zeros switches buoyancy off.
 * SPH_HIP_ERR_INVALID, the previous setting kept, for a context that carries no scalars, a beta, a reference
 * or a gravity that is not finite.  Switching the scalars off, and a new sph_hip_upload, drop the setting.
 * sph_hip_get_buoyancy returns 1 and copies the setting, or returns 0 when none is set.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
typedef struct sph_hip_buoyancy {   /* field order is ABI: 44 bytes */
   float beta[4];        /* per channel: weight change per unit of (T - reference) */
   float reference[4];   /* per channel: the value at which a particle has its own weight */
   float gravity[3];     /* the acceleration that -s scales */
} sph_hip_buoyancy;
int sph_hip_set_buoyancy(sph_hip_context* ctx, const sph_hip_buoyancy* b);
int sph_hip_get_buoyancy(sph_hip_context* ctx, sph_hip_buoyancy* out);

/* ---- cohesion ----------------------------------------------------------------------------------- *
 *
 * A pairwise surface tension that holds the fluid together (Becker and Teschner 2007): with rho0 below every
 * density the pressure only ever pushes the fluid apart; cohesion pulls every particle towards its neighbours,
 * which cancels inside the fluid and points inward at a free surface.  No counterpart in the reference.  The
 * operation-by-operation contract is in csrc/cohesion_policy.h; all arithmetic is fp32, unfused, in the order
 * written.
 *   sum        for particle i of a step's state S_k, over its neighbours j (the acceleration pass's pairs, in
 *              canonical order): s = s + t_j * (r_i - r_j) per component from 0, t_j the density pass's pair term
 *              m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrtf(d2) * sim_scale (the field sampler's term, above),
 *              the separation times sim_scale too.
 *   force      c = (-gamma) * s per component.  The terms of (i, j) and (j, i) are each other's negation: with equal
 *              masses momentum is conserved.  A negative gamma is a repulsion and is allowed.
 *   guard      a particle whose c is zero in every component, or not finite in any, is left alone: not a bit of
 *              it changes, -0.0f included.
 *   a step     behind the step's acceleration pass, before buoyancy and the integrate: a' = clamp(a + c), the
 *              acceleration pass's own cfl_limit rule applied again.  The velocity is not touched.  The
 *              acceleration read back after the step is a' (with buoyancy: what buoyancy made of a').
 *   modes      FULL and FULL_FAST give the same c bits.
 *   route      a cohesive context gives up the fused integrate (it keeps the prehash) and launches one more
 *              kernel per step.  Obstacles, motions, paths, bodies, load recordings, gauges, tracers, carried
 *              scalars and buoyancy work beside it unchanged.  A context without cohesion enqueues exactly what
 *              it always did.
 *   not done   the stand-alone phase calls (sph_hip_compute_density .. sph_hip_integrate) and the slab steps do
 *              NOT apply cohesion.
 * sph_hip_set_cohesion sets gamma for the steps enqueued from now on; it does not wait, and steps already queued
 * keep the gamma they were enqueued with.  gamma == 0 switches cohesion off and is never refused.
 * SPH_HIP_ERR_INVALID, the previous setting kept, for a gamma that is not finite, a REF or a slab context, and a
 * context with ports; sph_hip_set_ports refuses ports on a context with cohesion.  A new sph_hip_upload drops the
 * setting.  sph_hip_get_cohesion stores the gamma in force, 0 when none is.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
int sph_hip_set_cohesion(sph_hip_context* ctx, float gamma);
int sph_hip_get_cohesion(sph_hip_context* ctx, float* gamma);

/* ---- xsph --------------------------------------------------------------------------------------- *
 *
 * Velocity smoothing after Monaghan (1989): each step every particle's velocity is drawn towards a kernel-weighted
 * mean of its neighbours' velocities.  Particle-scale velocity noise decays and the flow stays coherent; a uniform
 * motion is not changed, and with equal masses neither is the total momentum.  No counterpart in the reference.
 * The operation-by-operation contract is in csrc/xsph_policy.h; all arithmetic is fp32, unfused, in the order
 * written.
 *   stage      for every particle p of a step's state S_k: R_p = {v_p, 1.0f / rho_p}, rho_p the density the step's
 *              density pass formed.
 *   sum        for particle i over its neighbours j (the acceleration pass's pairs, in canonical order):
 *              s = s + g_ij * (v_j - v_i) per component from 0, g_ij = t_j * (0.5f * (R_i.w + R_j.w)), t_j the
 *              density pass's pair term m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrtf(d2) * sim_scale (the field
 *              sampler's term, above): Monaghan's 2 m_j W / (rho_i + rho_j) with the mean of the inverse densities.
 *   change     dv = eps * s per component; every sum reads S_k's velocities, never a smoothed one.
 *   guard      a particle whose dv is zero in every component, or not finite in any, is left alone: not a bit of
 *              it changes.  A particle without a neighbour and a uniform velocity field are left alone.
 *   a step     behind the step's acceleration pass and cohesion, before buoyancy and the integrate: v' = v + dv.
 *              There is no clamp, and the acceleration is not touched.  Buoyancy adds its b*dt to v'.
 *   modes      FULL and FULL_FAST give the same dv bits from the same state.
 *   range      the smoothing is a convex combination while eps * sum_j g_ij <= 1 - about eps at the fluid's own
 *              density; nothing polices the sum.
 *   route      a context with the smoothing gives up the fused integrate (it keeps the prehash) and launches two
 *              more kernels per step.  Obstacles, motions, paths, bodies, load recordings, gauges, tracers, carried
 *              scalars, buoyancy, cohesion and the step monitor work beside it unchanged.  A context without it
 *              enqueues exactly what it always did, and allocates nothing for it.
 *   not done   the stand-alone phase calls (sph_hip_compute_density .. sph_hip_integrate) and the slab steps do
 *              NOT apply the smoothing.
 * sph_hip_set_xsph sets eps for the steps enqueued from now on; it does not wait, and steps already queued keep the
 * eps they were enqueued with.  eps == 0 switches the smoothing off and is never refused.  SPH_HIP_ERR_INVALID, the
 * previous setting kept, for an eps that is not finite or lies outside [0, 1], a REF or a slab context, and a
 * context with ports; sph_hip_set_ports refuses ports on a context with the smoothing.  A new sph_hip_upload drops
 * the setting.  sph_hip_get_xsph stores the eps in force, 0 when none is.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
int sph_hip_set_xsph(sph_hip_context* ctx, float eps);
int sph_hip_get_xsph(sph_hip_context* ctx, float* eps);

/* ---- viscous stress ----------------------------------------------------------------------------- *
 *
 * A pairwise, momentum-conserving viscous force of a stated dynamic viscosity mu: oil, honey, mud, a sloshing tank
 * that comes to rest - and, with a law, a viscosity that follows a carried channel through a table: lava that
 * stiffens as it cools.  params.viscosity is not this term: the reference rescales its viscous sum inside the
 * neighbour loop by a factor derived from the pressure, and the bit-exact port keeps that.  The
 * operation-by-operation contract is in csrc/viscous_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   law        factor(x) of a channel value x over K keys (value[k] strictly ascending, factor[k] >= 0): factor[0]
 *              where !(x > value[0]) (NaN too), factor[K-1] where x >= value[K-1], else linear between the two keys
 *              around x: f_k + u * (f_{k+1} - f_k), u = (x - x_k) / (x_{k+1} - x_k).
 *   stage      for every particle p of a step's state S_k: R_p = {v_p, V_p}, V_p = m_p / rho_p (0 where rho_p is not
 *              > 0), rho_p the density the step's density pass formed; with a law M_p = mu * factor(T_p,channel), T
 *              the channels as they stood before this step (what buoyancy reads).
 *   sum        for particle i over its neighbours j (the acceleration pass's pairs, in canonical order) with
 *              V_j != 0: s = s + g_ij * (v_j - v_i) per component from 0, g_ij = (m_ij * (V_i * V_j)) * L,
 *              L = kernel3 * (hscaled - d) the reference's viscosity Laplacian, d = sqrtf(d2) * sim_scale,
 *              m_ij = 0.5f * (M_i + M_j) with a law, else mu.  g_ij == g_ji by bits: the force addends of a pair
 *              negate each other for any masses.
 *   accel      c = s / m_i per component.
 *   guard      a particle with V_i == 0, a mass that is not > 0, a c that is zero in every component or not finite
 *              in any, is left alone: not a bit of it changes.  A uniform velocity field stores nothing.
 *   a step     behind the step's acceleration pass and cohesion, before XSPH, buoyancy and the integrate:
 *              a' = clamp(a + c), the acceleration pass's clamp.  The velocity is not touched; every sum reads
 *              S_k's velocities.
 *   modes      FULL and FULL_FAST give the same c bits from the same state.
 *   range      the scheme is explicit: a velocity stays a convex combination of itself and its neighbours' while
 *              N_i = dt * (1 / m_i) * sum_j m_ij V_i V_j L <= 1.  NOTHING polices this, on the device or here.
 *   route      a context with the term gives up the fused integrate (it keeps the prehash) and launches two more
 *              kernels per step.  Obstacles, motions, paths, bodies, load recordings, gauges, tracers, carried
 *              scalars, buoyancy, cohesion, XSPH and the step monitor work beside it unchanged.  A context without
 *              it enqueues exactly what it always did, and allocates nothing for it: the first non-zero mu
 *              allocates 16 bytes per particle of capacity, the first law 4 more.
 *   not done   the stand-alone phase calls (sph_hip_compute_density .. sph_hip_integrate) and the slab steps do
 *              NOT apply the viscous stress.
 * sph_hip_set_viscous_stress sets mu and the law (null: a constant mu) for the steps enqueued from now on; it does
 * not wait, and steps already queued keep what they were enqueued with.  mu == 0 switches the term off and is never
 * refused.  SPH_HIP_ERR_INVALID, the previous setting kept, for a mu that is not finite or negative, a law whose
 * channel, key count, key values or key factors break the rules above, a law on a context without scalars, a REF or
 * a slab context, and a context with ports; sph_hip_set_ports refuses ports on a context with the term.
 * sph_hip_set_scalars without rows drops the law and keeps mu.  A new sph_hip_upload drops the whole setting.
 * sph_hip_get_viscous_stress stores the mu in force (0 when none is), the law (zeroed when none is) and whether there
 * is one; each output may be null.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
#define SPH_HIP_MAX_VISCOSITY_KEYS 16

typedef struct sph_hip_viscosity_law {
   int32_t channel;                            /* 0 .. SPH_HIP_SCALAR_CHANNELS - 1 */
   int32_t n_keys;                             /* 2 .. SPH_HIP_MAX_VISCOSITY_KEYS */
   float value[SPH_HIP_MAX_VISCOSITY_KEYS];    /* strictly ascending */
   float factor[SPH_HIP_MAX_VISCOSITY_KEYS];   /* >= 0: mu is multiplied by it */
} sph_hip_viscosity_law;

int sph_hip_set_viscous_stress(sph_hip_context* ctx, float mu, const sph_hip_viscosity_law* law_or_null);
int sph_hip_get_viscous_stress(sph_hip_context* ctx, float* mu, sph_hip_viscosity_law* law, int* have_law);

/* ---- implicit viscous stress -------------------------------------------------------------------- *
 *
 * A solver mode of the viscous setting above, for a mu beyond the explicit range: the same symmetric pair operator
 * taken by backward Euler, m_i (v_i' - v_i) = dt * sum_j g_ij (v_j' - v_i'), and solved by a fixed number of Jacobi
 * sweeps on the device.  mu and the law stay sph_hip_set_viscous_stress's.  The operation-by-operation contract is in
 * csrc/viscous_implicit_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   sweeps     0 .. SPH_HIP_MAX_VISCOUS_SWEEPS.  0 is the explicit term above, bit for bit.  The count takes effect
 *              only while mu != 0.
 *   stage      the explicit term's: X0_p = R_p = {v_p, V_p}, M_p with a law.
 *   a sweep    for particle i with its own velocity v0 of the step's state, over the explicit term's neighbours in
 *              its order, with V_j != 0 and the rows X of the sweep before: s = s + g_ij * (X_j - v0) per component
 *              and D = D + g_ij, both from 0, g_ij the explicit term's by bits; den = m_i + dt * D;
 *              dv = (dt * s) / den per component; x_i = v0 + dv.  The last sweep stores x_i as the velocity.
 *   guard      a particle with V_i == 0, a mass that is not > 0, a den that is not > 0, a dv that is zero in every
 *              component or not finite in any, keeps v0.  A uniform velocity field stores nothing at any count.
 *   a step     where the explicit term stands: behind the acceleration pass and cohesion, before XSPH, buoyancy and
 *              the integrate.  The splitting is sequential: XSPH smooths, and buoyancy adds to, the velocities the
 *              last sweep left.  The acceleration is never read or written, so no clamp applies and FULL and
 *              FULL_FAST give the same velocities by bits.
 *   range      every iterate is a convex combination of the particle's own velocity and its neighbours' iterates
 *              (weights m / den and dt g / den) for ANY dt and mu >= 0, PROVIDED every g_ij >= 0: no component
 *              leaves the range of the step's velocities by more than rounding, and nothing has to police N_i.
 *              g >= 0 holds where no neighbour stands beyond hscaled (L >= 0); parameters with hscaled < h * sim_scale
 *              have neighbours with L < 0, and for those the claim is not made.
 *   the price  convergence is slow where N_i >> 1: the error contracts like N / (1 + N) per sweep, K sweeps reach K
 *              rings of neighbours, and an under-swept solve acts like a smaller mu.  And a truncated solve does not
 *              conserve momentum pair by pair: the defect sum_i m_i (x_i - v0_i) is the sum of the residuals; it
 *              falls with the sweeps and vanishes at convergence.  Measured on a 3 000-particle shear layer (momentum
 *              749.5; N is 5.9 in the bulk and up to 44 at the rim at 5 times the bulk's explicit limit, ten times
 *              that at 50 times): the defect is 1.07 after 2 sweeps and 0.064 after 16 at 5 times the limit, 1.85 and
 *              1.79 at 50 times; at a tenth of the limit 1.4e-3 and 1e-6, and 8 sweeps are within 1e-7 of 16
 *              (implicit viscous stress).
 *   route      K sweeps are K + 1 launches per step in the place of the explicit term's two, without a
 *              synchronisation.  The first count of 2 or more allocates 16 more bytes per particle of capacity; a
 *              count of 1 needs none.  A context without the mode enqueues and allocates exactly what it did.
 * sph_hip_set_viscous_implicit sets the count for the steps enqueued from now on; it does not wait, and steps already
 * queued keep what they were enqueued with.  0 is never refused.  SPH_HIP_ERR_INVALID, the previous count kept, for a
 * count outside the range, a REF or a slab context, and a context with ports; sph_hip_set_ports refuses ports on a
 * context with the mode.  A new sph_hip_upload drops the count with the rest of the viscous setting;
 * sph_hip_set_scalars without rows keeps it.  sph_hip_get_viscous_implicit stores the count in force.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
#define SPH_HIP_MAX_VISCOUS_SWEEPS 64

int sph_hip_set_viscous_implicit(sph_hip_context* ctx, int sweeps);
int sph_hip_get_viscous_implicit(sph_hip_context* ctx, int* sweeps);

/* ---- step monitor ------------------------------------------------------------------------------- *
 *
 * Per-step stability and conservation rows, filled on the device while the steps stay queued: at which step a run
 * left its limits, and what time step it should have had.  No counterpart in the reference.  The
 * operation-by-operation contract is in csrc/monitor_policy.h; all arithmetic is fp32, unfused, in the order
 * written, and everything a row holds is a maximum, a minimum, a count or an integer sum: its bits do not depend
 * on the route a context takes (tiled or not, fused integrate or not, list capacities) nor on the run.
 *   a row      describes one step: the step's densities, neighbour counts and final accelerations (behind cohesion
 *              and buoyancy), and the positions, velocities and carried channels the step PRODUCED.
 *   bad        a particle whose position, velocity, acceleration (x, y, z each) or density is not finite, or whose
 *              density is negative: counted in `bad`, its id offered to bad_id_min (0xffffffff: none), and left
 *              out of every other field but live, s_max and pair_bad.
 *   ranges     v2 = (vx*vx + vy*vy) + vz*vz and a2 likewise; v2_max, a2_max, rho_max, rho_min, ncount_max, and
 *              lone = the particles without a neighbour.  Floats are compared by the ordered integer key of their
 *              bits: -0.0f < +0.0f, and the winner's bits do not depend on the order of comparison.  A range over
 *              no value is 0.
 *   sums       momentum[c] = sum llrint(m*v_c * 2^-q), kinetic = sum llrint(((0.5f*m)*v2) * 2^-q), mass =
 *              sum llrint(m * 2^-q), q = quantum_log2, the rule of sph_hip_record_loads; a particle with a term
 *              that is not finite or reaches 2^38 quanta adds to none of them and counts in `skipped`.
 *   scalars    (flags bit 0) scalar_min / scalar_max over the finite values of each channel as the step left
 *              them; scalar_bad = the particles with a channel that is not finite.
 *   diffusion  (flags bit 1) s_max = the maximum over the particles of S_p = sum_j V_j * kernel3 * (hscaled -
 *              d_ij), the scalar pass's own weights in its own order: dt * kappa[c] * s_max <= 1 is the condition
 *              under which the pass is a convex combination.  pair_bad counts the S_p that are not finite.
 * Fields that are not valid (a context without scalars) hold zeros.
 * sph_hip_record_monitor keeps `rows` rows on the device: steps are numbered 1, 2, ... from the call, and step s
 * fills row (s - 1) / every when every divides s - 1 and the row exists; only such steps launch anything new.
 * rows = 0 stops and frees the recording.  The call does not wait unless it replaces a recording.
 * SPH_HIP_ERR_INVALID, the previous recording kept, for rows < 0, every < 1, a quantum_log2 outside [-64, 32], a
 * REF or a slab context, and a context with ports; sph_hip_set_ports and the slab exchange refuse a context with a
 * recording.  The recording survives sph_hip_set_params, sph_hip_set_arithmetic and uploads.  The stand-alone phase
 * calls do not record.
 * sph_hip_get_monitor_record synchronises, copies rows [first_row, first_row + n_rows) of the rows filled so far
 * into out (may be null with n_rows 0) and the number of the step each describes into steps (may be null);
 * returns the number of filled rows, SPH_HIP_ERR_INVALID for a range that leaves them.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
#define SPH_HIP_MONITOR_SCALARS_VALID 1u
#define SPH_HIP_MONITOR_DIFFUSION_VALID 2u
typedef struct sph_hip_monitor_row {   /* field order is ABI: 128 bytes */
   int64_t momentum[3];    /* quanta of 2^quantum_log2 */
   int64_t kinetic;
   int64_t mass;
   int32_t live;           /* slots visited */
   int32_t bad;
   int32_t skipped;
   int32_t lone;
   int32_t ncount_max;
   int32_t scalar_bad;
   int32_t pair_bad;
   uint32_t bad_id_min;
   float v2_max, a2_max, rho_max, rho_min, s_max;
   float scalar_min[4];
   float scalar_max[4];
   uint32_t flags;
} sph_hip_monitor_row;
int sph_hip_record_monitor(sph_hip_context* ctx, int rows, int every, int quantum_log2);
int sph_hip_get_monitor_record(sph_hip_context* ctx, int first_row, int n_rows, sph_hip_monitor_row* out,
                               int32_t* steps);

/* ---- velocity gradients --------------------------------------------------------------------------- *
 *
 * Where the flow rotates, compresses and shears: the vorticity, the divergence, the strain rate and the Q criterion
 * of every particle, at particles, at probes, on lattices and in a frame.  No counterpart in the reference.  The
 * gradient is a weighted least-squares fit over the particle's neighbours (the renormalised gradient of Randles and
 * Libersky 1996), G = B * inverse(M) with B = sum_j w_j (v_i - v_j) (x) (r_i - r_j), M = sum_j w_j (r_i - r_j) (x)
 * (r_i - r_j) and w_j the density pass's pair term: it reads no density and is exact on a linear velocity field for
 * any neighbourhood whose M can be inverted, one-sided ones at a free surface or a wall included.  The
 * operation-by-operation contract is in csrc/velgrad_policy.h; all arithmetic is fp32, unfused, in the order written.
 *   members    the acceleration pass's pairs of the current state, in canonical order; at least 3 are needed
 *   valid      det M > 2^-10 * (tr M / 3)^3: 1 for an isotropic neighbourhood, 0 for a coplanar one
 *   rows       rotation   = (w_x, w_y, w_z, div), w = curl v, div = div v
 *              invariants = (strain, Q, |w|, valid): strain = sqrt(2 S:S), Q = (|O|^2 - |S|^2) / 2 with S and O the
 *              symmetric and antisymmetric parts of G, valid = 1.0f
 *              A particle that is not valid, or with a value that is not finite, holds +0.0f in all eight.
 *   units      the separations are taken times sim_scale, as the density pass takes its distances: G is the gradient
 *              per unit of scaled length, and a field v = A x gives G = A / sim_scale.
 *   modes      FULL and FULL_FAST give the same bits.
 *   no cache  every call below runs a cell build of the current state and forms the rows anew; no particle,
 *              density, neighbour list or clock changes by a bit, and a context that never calls them enqueues
 *              exactly what it always did.
 * sph_hip_get_velocity_gradients synchronises and copies rows [first, first + n) in particle-id order (either
 * output may be null).  SPH_HIP_ERR_INVALID for a range that leaves the particles, a REF or a slab context, and a
 * context whose ids ports have changed, until its next upload (sph_hip_download's rule).
 * sph_hip_sample_velocity_gradients_points / _lattice are sph_hip_sample_scalars_points / _lattice with the rows in
 * the place of the channels: group 0 samples `rotation`, group 1 `invariants`; a probe's value is the
 * Shepard-normalised sum over its members, so a sampled `valid` is the weighted share of valid particles around
 * it.  Allowed on a context with ports.
 * sph_hip_render_velocity_gradients is sph_hip_render_scalars with tp->channel carrying a quantity
 * SPH_HIP_VELGRAD_* in the place of a channel; the context needs no carried scalars.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no existing struct and no existing
 * prototype changed. */
#define SPH_HIP_VELGRAD_VORTICITY_X 0
#define SPH_HIP_VELGRAD_VORTICITY_Y 1
#define SPH_HIP_VELGRAD_VORTICITY_Z 2
#define SPH_HIP_VELGRAD_DIVERGENCE 3
#define SPH_HIP_VELGRAD_STRAIN_RATE 4
#define SPH_HIP_VELGRAD_Q 5
#define SPH_HIP_VELGRAD_VORTICITY_MAGNITUDE 6
#define SPH_HIP_VELGRAD_VALID 7
int sph_hip_get_velocity_gradients(sph_hip_context* ctx, int first, int n, float* rotation4, float* invariants4);
int sph_hip_sample_velocity_gradients_points(sph_hip_context* ctx, int n, const float* xyz, int group, float* channels4,
                                             float* density, int32_t* count);
int sph_hip_sample_velocity_gradients_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                              const int32_t dims[3], int group, float* channels4, float* density,
                                              int32_t* count);
int sph_hip_render_velocity_gradients(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                                      const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo,
                                      const sph_hip_tint_params* tp, const float* table_rgb, int width, int height,
                                      int flags, uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz,
                                      int32_t* first_inside, int32_t* solid_id, float* scalar);

/* ---- ports: inflow emitters and outflow sinks ------------------------------------------------- *
 *
 * A particle count that changes while the steps stay queued: emitters append whole lattice layers
 * of new particles, sinks remove the particles that stand inside a box.  No counterpart in the
 * reference.  The operation-by-operation contract is in csrc/port_policy.h; all arithmetic is fp32,
 * unfused, in the order written.
 *   emitter   a = axis, u = (a + 1) % 3, w = (a + 2) % 3.  A layer is count = {nu, nw} points on the
 *             plane x_a = origin[a]: point k has i = k % nu, j = k / nu, x_u = origin[u] +
 *             (float)i * spacing, x_w = origin[w] + (float)j * spacing.  Every point enters with the
 *             emitter's velocity and mass.  Emitter e fires in port step s when s >= first,
 *             (s - first) % every == 0 and it has fired fewer than `layers` times (layers = -1: no
 *             limit).  s counts the steps of sph_hip_step / sph_hip_run since the ports were set or
 *             the state was uploaded, from 0.
 *   ids       the context keeps next_id: an upload sets it to n, an upload with ids to the largest
 *             id + 1.  The emitters that fire in a step take ids in list order, point k of emitter e
 *             gets id_base_e + k.  A step whose ids would reach 0xffffffff is refused.
 *   sink      the box lo <= x < hi on all three axes (NaN is never inside).  A particle inside several
 *             sinks counts for the one with the lowest index.
 *   order     at the start of a step, before its cell build: the sinks look at the particles the last
 *             step left and remove those inside; then the firing emitters' layers are appended.  A
 *             layer is never caught in the step it enters, and it takes part in that whole step: cell
 *             build, sums, integrate.  Sinks act at the START of a step only: whatever stands inside a
 *             sink after the last step of a run is still there and is read back.
 *   capacity  a layer that does not fit the context's capacity is never emitted in part: the step is
 *             refused with SPH_HIP_ERR_CAPACITY before anything of it is enqueued (the call first
 *             waits for the queued steps and counts what the sinks have freed).  sph_hip_run returns
 *             at that step, the earlier steps stand, and the schedule does not advance.
 *   route     a context with ports gives up the prehash and the fused integrate: its steps take the
 *             separate integrate kernel and hash in the cell build, plus one launch of
 *             k_ports_apply in front of the build.  Results are bit-identical to the default route.
 *             A context without ports enqueues exactly what it always did.
 *   with      obstacles, motions, bodies, load recordings, tracers, gauges, the sampler, the surface
 *             extractor and both renderers work on a port context unchanged.  The stand-alone phase
 *             calls (sph_hip_voxelize ... sph_hip_integrate) apply no ports.
 *   not done  REF contexts, slab contexts and contexts that have exchanged are refused.  From the first
 *             step with a sink or a firing emitter until the next upload the ids are no longer 0..n-1:
 *             sph_hip_download and sph_hip_download_async are refused and name sph_hip_download_live.
 * sph_hip_set_ports replaces both lists (ne = ns = 0 clears them) and restarts the schedule, the totals
 * and the port step count at 0; an upload does the same and keeps the lists.  SPH_HIP_ERR_INVALID, the
 * previous lists kept, for everything port_check (csrc/port_policy.h) refuses.
 * sph_hip_get_ports synchronises; copies up to capacity_e emitters and capacity_s sinks; emitted[e] =
 * particles emitter e has added, removed[s] = particles sink s has caught (arrays of
 * SPH_HIP_MAX_EMITTERS / SPH_HIP_MAX_SINKS entries, each may be NULL); *live = the resident particles,
 * *next_id.  Returns ne | ns << 8.
 * sph_hip_download_live is the compact read-back: synchronises, *rows = the live count, and - when that
 * is at most max_rows - the particles in device order with their ids; every array may be NULL.
 * These entry points were added without a change of SPH_HIP_ABI_VERSION: no struct and no existing
 * prototype changed. */
#define SPH_HIP_MAX_EMITTERS 8
#define SPH_HIP_MAX_SINKS    8
#define SPH_HIP_MAX_EMITTER_POINTS 65536
typedef struct sph_hip_emitter {   /* field order is ABI: 56 bytes */
   int32_t axis;          /* normal of the lattice plane, 0..2 */
   float origin[3];
   int32_t count[2];      /* nu, nw; nu * nw <= SPH_HIP_MAX_EMITTER_POINTS */
   float spacing;
   float velocity[3];
   float mass;
   int32_t first;         /* first port step that fires */
   int32_t every;         /* then every every-th */
   int32_t layers;        /* at most this many layers; -1 = no limit */
} sph_hip_emitter;
typedef struct sph_hip_sink {      /* 24 bytes */
   float lo[3];
   float hi[3];
} sph_hip_sink;
int sph_hip_set_ports(sph_hip_context* ctx, const sph_hip_emitter* emitters, int ne, const sph_hip_sink* sinks,
                      int ns);
int sph_hip_get_ports(sph_hip_context* ctx, sph_hip_emitter* emitters, sph_hip_sink* sinks, int capacity_e,
                      int capacity_s, int64_t* emitted, int64_t* removed, int32_t* live, uint32_t* next_id);
int sph_hip_download_live(sph_hip_context* ctx, int max_rows, int32_t* rows, uint32_t* ids, float* pos, float* vel,
                          float* density, float* acc, int32_t* neighbor_count);

/* ---- multi-GPU: 1-D slab decomposition of the FULL-mode cell grid ------------------------- *
 *
 * No counterpart in the reference (one process, one thread).  One context per GPU owns the
 * global z-planes [plane_lo, plane_hi) of the FULL grid and additionally holds
 * SPH_HIP_SLAB_HALO (= 2) ghost planes on each side: with two planes the densities of the
 * ghosts next to the slab are recomputed locally from complete neighbourhoods, in the same
 * canonical order (cell id, particle id) as on their owner, so ONE exchange per step is enough
 * and results do not depend on the number of slabs.
 *
 * Per step, on every rank:
 *     sph_hip_slab_pack   -> two device messages (left / right neighbour)
 *     <transport>            RCCL send/recv over xGMI (torch.distributed), or a device copy
 *     sph_hip_slab_unpack <- the two messages received
 *     sph_hip_step
 * A message is sph_hip_slab_message_bytes(capacity) bytes of DEVICE memory owned by the
 * caller: 8 int32 header words (word 0 = record count) + 32-byte records
 * {x,y,z,m,vx,vy,vz,id}.  Every step a slab re-sends each owned particle that lies within the
 * halo width of (or beyond) a neighbour's border: the receiver treats records inside its own
 * planes as migrants (now owned) and the rest as ghosts; ghosts are dropped and re-sent every
 * step.  All counts stay on the device — none of these calls synchronises with the host.
 * sph_hip_create() is the special case plane_lo = 0, plane_hi = all planes, no neighbours.
 *
 * Exchange overlapped with the interior's force computation (after one pack/transport/unpack
 * round has delivered the first ghosts), per step:
 *     sph_hip_slab_step_begin   cell build, density, acceleration of the owned planes next to a
 *                               neighbour (halo + 1 planes), and the two messages: those
 *                               particles are integrated on the fly, the state is not touched
 *     <transport>               on the exchange stream handed to step_begin
 *     sph_hip_slab_step_end     acceleration of all other workgroups, integrate - concurrent
 *                               with the transport
 *     sph_hip_slab_unpack       after the context's stream has waited for the transport
 * Same results as the serial sequence.  Last step's ghosts and departed particles are recognised
 * by the next cell build from their position in the sorted order; error bit 8 reports an
 * interior particle that crossed more than one cell plane in a step and so missed its message. */
#define SPH_HIP_SLAB_HALO 2

int sph_hip_create_slab(sph_hip_context** out, const sph_hip_params* params, int capacity,
                        int device, int plane_lo, int plane_hi);
/* Owned particles of this slab with their GLOBAL persistent ids (the canonical order inside
 * a cell is by id).  all_masses_equal: non-zero iff every particle of the WHOLE system has
 * the same mass (enables the same fast path as sph_hip_upload detects by itself). */
int sph_hip_slab_upload(sph_hip_context* ctx, int n, const float* pos, const float* vel,
                        const float* mass, const uint32_t* ids, int all_masses_equal);
/* Owned particles in cell-sorted order: *rows receives their number (synchronises). */
int sph_hip_slab_download(sph_hip_context* ctx, int max_rows, int32_t* rows, uint32_t* ids,
                          float* pos, float* vel, float* density, float* acc,
                          int32_t* neighbor_count);
/* Masses of the owned particles in the row order of sph_hip_slab_download (what a host needs,
 * with that call's arrays, to move particles to another slab: slab.py rebalance()). */
int sph_hip_slab_download_mass(sph_hip_context* ctx, int max_rows, int32_t* rows, float* mass);
/* Device-to-device re-partitioning (no counterpart in the reference): the owned particles as the
 * 32-byte records of a halo message, {x,y,z,m | vx,vy,vz,id}, in cell-sorted order, written to
 * DEVICE memory of the caller (*rows = their number; synchronises) - and a slab's owned particles
 * from n such records in device memory (what sph_hip_slab_upload does from host arrays).  The rows
 * that change owner when the cut planes move (slab.py rebalance()) can then travel over RCCL
 * without touching the host. */
int sph_hip_slab_export_records(sph_hip_context* ctx, void* device_records, int max_records,
                                int32_t* rows);
int sph_hip_slab_upload_records(sph_hip_context* ctx, const void* device_records, int n,
                                int all_masses_equal);
size_t sph_hip_slab_message_bytes(int capacity_records);
/* NULL for a side without neighbour.  Call after sph_hip_step()/upload, before the transport. */
int sph_hip_slab_pack(sph_hip_context* ctx, void* left_device, void* right_device,
                      int capacity_records);
int sph_hip_slab_unpack(sph_hip_context* ctx, const void* left_device, const void* right_device,
                        int capacity_records);
/* See above.  Message buffers: exactly one per existing neighbour (NULL otherwise).
 * exchange_stream: the HIP stream the transport will be issued on (NULL = the context's stream,
 * no overlap).  The border planes' acceleration and the packing are enqueued on it, behind the
 * density pass, so the messages are complete in that stream's order and the work runs next to
 * the interior's acceleration; sph_hip_slab_step_end makes the integrate wait for it. */
int sph_hip_slab_step_begin(sph_hip_context* ctx, void* left_device, void* right_device,
                            int capacity_records, void* exchange_stream);
int sph_hip_slab_step_end(sph_hip_context* ctx);
/* ---- native RCCL exchange (no Python, no torch) ----
 * librccl is opened with dlopen on first use.  One rank (any) calls sph_hip_rccl_unique_id and
 * hands the 128 bytes to every rank (MPI, a file, a socket, torch.distributed ...); every rank
 * then calls sph_hip_slab_comm_init on its slab context - ranks are ordered along z, rank r's
 * neighbours are r - 1 and r + 1 - which creates the communicator, a high-priority exchange
 * stream and the four message buffers (capacity_records must be the same on all ranks).
 * sph_hip_slab_comm_run(steps) is then the whole loop: a first serial exchange, and per step
 * sph_hip_slab_step_begin -> ncclSend/ncclRecv of both directions in one group on the exchange
 * stream -> sph_hip_slab_step_end -> sph_hip_slab_unpack.  Asynchronous like sph_hip_run.
 * sph_hip_slab_comm_selftest sends a message to itself through the same calls (synchronises). */
int sph_hip_rccl_unique_id(void* id_out, int id_bytes);
int sph_hip_slab_comm_init(sph_hip_context* ctx, const void* id, int id_bytes, int rank, int nranks,
                           int capacity_records);
int sph_hip_slab_comm_run(sph_hip_context* ctx, int steps);
/* Only the used part of a message needs to cross the link.  Collective over the communicator
 * (synchronises): every rank looks at the record counts of the messages it packed last, the
 * largest count * slack + extra_records (at most the capacity given to sph_hip_slab_comm_init)
 * becomes the size every message is packed for, sent and received with from now on
 * (*active_records).  sph_hip_slab_comm_run puts the messages back to the allocated size before
 * they overflow (sph_hip_slab_comm_stats); a message that outgrows even that - or grows by more
 * than a quarter within 32 steps - raises error bit 2, which stops the run.  Call after a few
 * steps, and now and then in a long run. */
int sph_hip_slab_comm_trim(sph_hip_context* ctx, float slack, int extra_records,
                           int32_t* active_records);
int sph_hip_slab_comm_selftest(sph_hip_context* ctx);
/* One checked message to and from each neighbour through the same calls (after
 * sph_hip_slab_comm_init, before the first step; collective over the neighbours; synchronises): a
 * pre-flight of the device-to-device path that a launcher can run in a helper process with a time
 * limit before it commits a run to it (bench.py does). */
int sph_hip_slab_comm_exchange_check(sph_hip_context* ctx);
/* out[0]: records the messages are currently packed for and transferred with, out[1]: records the
 * buffers hold, out[2]: how often sph_hip_slab_comm_run put trimmed messages back to the allocated
 * size (they grow BEFORE they overflow: every 16 steps the ranks reduce the record counts of the
 * messages they packed last - ncclAllReduce(max) behind the exchange, result read 16 steps later,
 * at the same step on every rank - and all of them switch together when any message was more than
 * 4/5 full), out[3]: steps enqueued by sph_hip_slab_comm_run so far. */
int sph_hip_slab_comm_stats(sph_hip_context* ctx, int32_t out[4]);
/* Diagnostics (synchronises): live entries, owned particles, error bits (1: a received entry
 * lies outside the slab and its halo, 2: a message overflowed, 4: context capacity exceeded - by
 * received records or by the cell counts of a build: the build clamps its ranges to the capacity
 * and drops what does not fit instead of writing past its arrays, 8: a particle missed the early
 * exchange, 16: one cell holds a persistent id twice - a record delivered twice, a particle owned
 * by two slabs). */
int sph_hip_slab_status(sph_hip_context* ctx, int32_t* live, int32_t* owned, int32_t* errors);
/* The same error bits without draining the stream: reports what the copy requested by the
 * PREVIOUS call brought (*errors, may be NULL; waits for that one copy if the host has run more
 * than one polling interval ahead of the device) and requests the next copy of the device's
 * error word into pinned host memory.  Returns SPH_HIP_ERR_EXCHANGE (message in
 * sph_hip_last_error) once a non-zero word has arrived, so a loop that calls this every K steps
 * stops within 2 K steps of the exchange going wrong instead of running on with missing particles.
 * sph_hip_slab_comm_run polls every 16 steps itself; sph_hip_synchronize and
 * sph_hip_slab_download check after waiting and return the same status. */
int sph_hip_slab_poll_errors(sph_hip_context* ctx, int32_t* errors);

/* ---- self tests -------------------------------------------------------------------------- */

/* The pair loops take square roots with a shorter instruction sequence than the compiler's
 * sqrtf (csrc/sph_device.h: sqrt_rn).  This compares the two for EVERY non-negative finite
 * float on `device` (2^31 inputs, well under a second): *mismatches = how many differ,
 * *first_bad = bit pattern of the smallest one that does (0xffffffff if none). */
int sph_hip_selftest_sqrt(int device, uint64_t* mismatches, uint32_t* first_bad);

/* ---- streams ----------------------------------------------------------------------------- */

/* Run all of ctx's work on the caller's HIP stream (e.g. the stream torch.distributed orders
 * its RCCL calls against); NULL returns to the context's own stream. */
int sph_hip_set_stream(sph_hip_context* ctx, void* hip_stream);
/* The HIP stream all of ctx's kernels currently run on. */
void* sph_hip_stream(sph_hip_context* ctx);

#ifdef __cplusplus
}
#endif

#endif /* SPH_HIP_H */

// Shared device-side helpers and types of the gfx950 SPH step (the context: context.h).
// Written for MI355X only: wave = 64 lanes, no other targets, no compatibility paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/sph_hip.h"
#include "launch_policy.h"

#define SPH_WAVE 64
#define EV_RING 128
#define PACE_STEPS 16   // the host enqueues at most 2 * PACE_STEPS steps ahead of the device

// ---- error plumbing -------------------------------------------------------------------
#define SPH_TRY(expr)                                                                \
   do {                                                                              \
      hipError_t e_ = (expr);                                                        \
      if (e_ != hipSuccess) {                                                        \
         ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
         return SPH_HIP_ERR_DEVICE;                                                  \
      }                                                                              \
   } while (0)

// Grid description handed to kernels by value.
struct CellGrid {
   int nx, ny, nz;  // cells held by this context (nz = local planes for a slab)
   float inv;       // cells per unit length
   int ncells;      // nx*ny*nz; cell id `ncells` is the trash cell (dead / out-of-slab entries)
   int z0;          // global z-plane of local plane 0
   int nz_global;   // planes of the whole grid (positions are clamped against this)
};

// Device-side counts and ranges of a context (int32 each); kernels read them so that a step
// never needs a host round trip.
enum {
   META_N_IN = 0,      // entries in the input arrays of the next cell build
   META_N_LIVE = 1,    // entries in real cells after the build (sorted order [0, n_live))
   META_OWN_BEGIN = 2, // sorted range of owned particles (planes [lo, hi))
   META_OWN_END = 3,
   META_SUM_BEGIN = 4, // sorted range whose density is needed (planes [lo-1, hi+1))
   META_SUM_END = 5,
   META_ERRORS = 6,    // bit 0: entry outside slab+halo, bit 1: message overflow, bit 2: capacity
   // early exchange (sph_hip_slab_step_begin): sorted ranges [OWN_BEGIN, BND_LO_END) and
   // [BND_HI_BEGIN, OWN_END) hold the owned planes next to a neighbouring slab, whose particles are
   // integrated and packed before the interior's acceleration runs
   META_BND_LO_END = 7,
   META_BND_HI_BEGIN = 8,
   META_COUNT = 12
};

// What a slab's cell build needs to know about the exchange (by value in kernarg).
struct SlabZone {
   int lo, hi;          // owned global planes [lo, hi)
   int halo;            // planes sent to / held from a neighbour
   int have_left, have_right;
   int drop_ghosts;     // FULL mode: entries of the previous sorted order outside its owned range
                        // are last step's ghosts - dropped, their owner re-sends them
   int early;           // the previous step packed its messages early: check nothing was missed
};

// density pass: widening of h2 for the fused screening test (csrc/full_tiled.h, "TEST screens")
#define TEST_SCREEN_FACTOR 1.000002f
// The rest of the step, done by the acceleration pass itself (a context that holds the whole
// grid and exchanges with nobody): every particle is integrated where its acceleration was just
// computed - into the state buffers the cell build left free, the neighbours still read the old
// ones - and hashed and counted for the next cell build; no k_integrate launch, no second trip of
// positions, velocities and accelerations through HBM.
struct SlabMsg;
struct FusedStep {
   int on;
   const float4* velp_in;   // velocity + id of the state the sums read
   float4* posm_out;        // the other pair of state buffers
   float4* velp_out;
   double* epart;           // energy partial sums, one pair per workgroup (as k_integrate)
   uint32_t* key;           // next build: cell id, slot inside the cell, the cells' counts
   uint32_t* slot;
   uint32_t* cell_count;
   // A slab that exchanges early (sph_hip_slab_step_begin / _end): the two parts of the
   // acceleration launch do the rest of the step for the particles they own - integrate, hash for
   // the next build, and, in the border part, the halo messages (what k_slab_pack_early did from
   // a second read of the state).  The next build only has to hash what arrives from the
   // neighbours (k_hash_tail).
   int slab;
   SlabZone zone;
   SlabMsg* left;
   SlabMsg* right;
   int msg_capacity;
   int32_t* meta;           // error bits
};
#define SPH_DEAD_ID 0xffffffffu

// Constants of the per-pair arithmetic, by value in kernarg (scalar registers).
struct PairConsts {
   float h2, hscaled, hscaled2, sim_scale;
   float h2_screen;   // h2 widened for the density pass's fused-multiply-add screening test
   // FAST pressure sum: kernel2 * sim_scale times a power of two 2^-s chosen from ITS exponent so that
   // the product is a normal number of magnitude [2^-8, 2^-7) whatever h and sim_scale are (a fixed
   // 2^-64 went subnormal for h_scaled ~ 1e3 and up), and 2^s, which takes it out of the finished sum
   float fast_k2s, fast_unscale;
   float kernel1, kernel2, kernel3;
   float rho0, stiffness, viscosity;
   float grav_const, central_mass, cx, cy, cz, softening;
   float cfl_limit, cfl_limit2;
   float dt, sim_scale_inv;
   // dam-break extensions (0 = shipped behaviour)
   float gx, gy, gz;         // mGravity
   float damping;            // mDamping
   float max_x, max_y, max_z; // mMaxX/Y/Z
   int apply_gravity, apply_walls;
   // tolerance mode, no point mass (central_mass == 0, softening > 0): the point-mass terms of
   // computeAcceleration / integrate (src/sph.cpp:892-915, 966-989) are +-0 and are skipped
   int skip_point_mass;
};

// ---- arithmetic helpers -----------------------------------------------------------------

// (int)floor(x) the way the x86-64 reference build does it (cvttsd2si): out-of-range and NaN
// give INT_MIN, which the clamp that follows turns into cell 0.
__device__ __forceinline__ int floor_to_int_x86(float f)
{
   float fl = floorf(f);
   return (fl >= -2147483648.0f && fl < 2147483648.0f) ? (int)fl : (int)0x80000000;
}

__device__ __forceinline__ int cell_coord(float x, float inv, int ncell)
{
   int c = floor_to_int_x86(x * inv);
   c = c < 0 ? 0 : c;
   c = c >= ncell ? ncell - 1 : c;
   return c;
}

// Cell of a position.  cz is the LOCAL plane (global plane - g.z0); a position whose plane lies
// outside the planes this context holds gets the trash cell id g.ncells.
__device__ __forceinline__ uint32_t cell_of(const CellGrid& g, float x, float y, float z, int& cx,
                                           int& cy, int& cz)
{
   cx = cell_coord(x, g.inv, g.nx);
   cy = cell_coord(y, g.inv, g.ny);
   cz = cell_coord(z, g.inv, g.nz_global) - g.z0;
   if (cz < 0 || cz >= g.nz) return (uint32_t)g.ncells;
   return (uint32_t)((cz * g.ny + cy) * g.nx + cx);
}

// Correctly rounded fp32 square root for the hot pair loops: the same value sqrtf() returns
// (IEEE round-to-nearest-even; checked against it for EVERY non-negative finite float by
// sph_hip_selftest_sqrt / tests/test_gpu_full_mode.py), in 10 instructions instead of the 15 of
// the compiler's expansion (v_sqrt_f32 + two +-1 ulp residual checks + denormal rescaling).
// Reciprocal-square-root seed, one coupled Goldschmidt step for g ~ sqrt(x) and h ~ 1/(2 sqrt(x)),
// then Markstein's correction g + (x - g*g) * h, whose fused residual makes the last rounding the
// only one that matters.  x = 0 gives 0 (the seed is taken of max(x, FLT_MIN), so g = 0 * finite).
// Below 2^-102 the residual x - g*g leaves the normal range and the sweep finds 1.8 million
// inputs that round the other way (none above): those, and denormals, take sqrtf() - a squared
// distance that small needs two fp32 positions 2^-51 apart, so the branch is there for
// correctness, not for speed.
// Non-finite inputs are outside the sweep on purpose: sqrt_rn(+inf) would be NaN (inf * rsq(inf) =
// inf * 0) where sqrtf gives inf, but every call site takes the root of a squared distance that
// has just passed "d2 < h2" - the membership test of src/sph.cpp:641,653, repeated bit for bit by
// the acceleration pass on the same positions - and neither +inf nor NaN passes that test.
#ifndef SPH_SQRT_GENERIC
__device__ __forceinline__ float sqrt_rn(float x)
{
   // bits in [1, 0x0c7fffff]  <=>  0 < x < 2^-102  (x is never negative here; -0 and 0 pass)
   if (__builtin_expect(__any(__float_as_uint(x) - 1u < 0x0c7fffffu), 0)) return sqrtf(x);
   // (seed of x + FLT_MIN, one plain addition, instead of max(x, FLT_MIN), which costs two wide-class
   // v_max_f32 - profiles/r4_valu_prices_more.txt: here x is 0 or at least 2^-102, so the sum is
   // FLT_MIN for 0 and x itself otherwise - except for odd mantissas in [2^-102, 2^-101), a tie that
   // moves the SEED's argument by one ulp; the result is checked for every float all the same:
   // sph_hip_selftest_sqrt)
   const float y = __builtin_amdgcn_rsqf(x + 1.17549435e-38f);
   float g = x * y;
   float h = 0.5f * y;
   const float r = __builtin_fmaf(-h, g, 0.5f);
   g = __builtin_fmaf(g, r, g);
   h = __builtin_fmaf(h, r, h);
   const float d = __builtin_fmaf(-g, g, x);
   return __builtin_fmaf(d, h, g);
}

// The same root for N values at once, with ONE uniform branch for the lot: a pair loop that takes
// the roots of the N neighbours of a trip one by one gets a scalar branch per neighbour from
// sqrt_rn's test for tiny arguments, which fences every neighbour's dependent chain (reciprocal
// square root, three fused steps, the pair arithmetic behind them) off from the next one's; taken
// together the N chains are one basic block and overlap.  Same values as sqrt_rn, bit for bit.
template <int N>
__device__ __forceinline__ void sqrt_rn_batch(float (&x)[N])
{
   bool tiny = false;
#pragma unroll
   for (int u = 0; u < N; u++) tiny |= __float_as_uint(x[u]) - 1u < 0x0c7fffffu;
   if (__builtin_expect(__any(tiny), 0)) {
#pragma unroll
      for (int u = 0; u < N; u++) x[u] = sqrtf(x[u]);
      return;
   }
#pragma unroll
   for (int u = 0; u < N; u++) {
      const float y = __builtin_amdgcn_rsqf(x[u] + 1.17549435e-38f);      // (as in sqrt_rn)
      float g = x[u] * y;
      float h = 0.5f * y;
      const float r = __builtin_fmaf(-h, g, 0.5f);
      g = __builtin_fmaf(g, r, g);
      h = __builtin_fmaf(h, r, h);
      const float d = __builtin_fmaf(-g, g, x[u]);
      x[u] = __builtin_fmaf(d, h, g);
   }
}
#else
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }
template <int N>
__device__ __forceinline__ void sqrt_rn_batch(float (&x)[N])
{
#pragma unroll
   for (int u = 0; u < N; u++) x[u] = sqrtf(x[u]);
}
#endif

// fp32 squared distance with the reference's association: (dx*dx + dy*dy) + dz*dz, no FMA
// (the translation unit is compiled with -ffp-contract=off).
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz,
                                       float& dx, float& dy, float& dz)
{
   dx = ax - bx;
   dy = ay - by;
   dz = az - bz;
   return dx * dx + dy * dy + dz * dz;
}

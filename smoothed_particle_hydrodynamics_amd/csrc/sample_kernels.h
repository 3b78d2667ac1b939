// Field sampler: SPH interpolation of the current state at probe points (sph_hip_sample_points)
// and on regular lattices (sph_hip_sample_lattice), over the cell-sorted FULL-mode state that a
// cell build has just produced.  The walk of a probe and the per-probe kernels take the accumulator
// as a parameter: with PressureSum (pressure_kernels.h) and ScalarSum (scalar_kernels.h) they are the
// samplers of the pressure and of the carried scalars.
//
// What a probe at x computes (include/sph_hip.h promises it, tests/test_gpu_sample.py pins it):
//   members   every live particle j with d2 = (dx*dx + dy*dy) + dz*dz < h2 in fp32 (dist2), the
//             density pass's membership test - and no particle is excluded: a probe placed on a
//             particle includes that particle's own term;
//   term      t_j = density_term(k, m_j, d), d = sqrtf(d2) (times sim_scale unless unit scale),
//             the FULL density pass's arithmetic, identical in both arithmetics;
//   density   rho = sum of t_j in fp32, in canonical order: ascending FULL cell id, then ascending
//             sorted index (= persistent id inside a cell);
//   velocity  v_c = (sum of t_j * v_j,c, unfused, same order) / rho if rho > 0, else 0;
//   count     the number of members.
// Only positions, masses and velocities of the current state are read, never the densities of
// the last step.  A non-finite or out-of-box probe needs no special case: its cell is the build's
// own clamped cell_coord (NaN and +-inf clamp to cell 0), and a NaN or infinite d2 is never a
// member, so such a probe gives density 0, count 0 and velocity 0.
//
// The walk of one probe is density_untiled's (full_kernels.h) without the self-skip: 9 cell rows
// (cz-1..cz+1, cy-1..cy+1), each the contiguous sorted range of cells cx-1..cx+1.  The tiled lattice
// kernel stages those rows once per brick of points (sample_policy.h) in LDS and
// every lane walks its own 9 row segments from there, in the same order: the same bits.
#pragma once

#include "full_kernels.h"
#include "sample_policy.h"

// What a lattice launch covers: a chunk of points (sample_lattice_chunk) of the caller's lattice.
struct SampleLattice {
   float ox, oy, oz;   // lattice origin
   float sx, sy, sz;   // spacing per axis (> 0)
   int i0, j0, k0;     // lattice index of the chunk's first point
   int ex, ey, ez;     // points of the chunk per axis
   int bx, by, bz;     // brick shape (sample_policy.h: sample_brick), bx * by * bz = SAMPLE_THREADS
   int bricks_x, bricks_y;   // bricks per chunk along x and y
};

// Accumulator of one probe.  What sample_walk and the per-probe kernels ask of an accumulator (this one,
// PressureSum: pressure_kernels.h, ScalarSum: scalar_kernels.h): Payload, the per-particle array in sorted
// order that a member contributes besides its position and mass; member(), which loads payload[q] - for
// members only, behind the d2 < h2 test - and adds the term; Out, the output arrays, and store().
template <bool VEL>
struct SampleSum {
   float rho = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;
   int count = 0;

   using Payload = float4;   // velp: the velocities (not read, and may be null, unless VEL)
   struct Out {
      float* rho;
      float* vel;
      int32_t* cnt;
   };

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void member(const PairConsts& k, float d2, float m, const float4* __restrict__ velp,
                                          uint32_t q)
   {
      float4 vj = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (VEL) vj = velp[q];
      add<UNIT_SCALE>(k, d2, m, vj.x, vj.y, vj.z);
   }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const PairConsts& k, float d2, float m, float ux, float uy, float uz)
   {
      // d2 < h2 passed: the root is finite; sqrt_rn == sqrtf for every such argument
      float d = sqrt_rn(d2);
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float t = density_term<UNIT_SCALE>(k, m, d);
      rho += t;
      if (VEL) {
         vx += t * ux;
         vy += t * uy;
         vz += t * uz;
      }
      count++;
   }

   __device__ __forceinline__ void store(int o, const Out& out) const { store(o, out.rho, out.vel, out.cnt); }

   __device__ __forceinline__ void store(int o, float* __restrict__ rho_out, float* __restrict__ vel_out,
                                         int32_t* __restrict__ cnt_out) const
   {
      rho_out[o] = rho;
      cnt_out[o] = count;
      if (VEL) {
         const bool pos = rho > 0.0f;
         vel_out[3 * o + 0] = pos ? vx / rho : 0.0f;
         vel_out[3 * o + 1] = pos ? vy / rho : 0.0f;
         vel_out[3 * o + 2] = pos ? vz / rho : 0.0f;
      }
   }
};

// cell of a probe on a grid that holds every plane (sampled contexts hold the whole grid)
__device__ __forceinline__ void probe_cell(const CellGrid& g, float x, float y, float z, int& cx, int& cy, int& cz)
{
   cx = cell_coord(x, g.inv, g.nx);
   cy = cell_coord(y, g.inv, g.ny);
   cz = cell_coord(z, g.inv, g.nz);
}

// one probe, candidates read from global memory (through L1/L2), for any accumulator
template <bool UNIT_SCALE, class Sum>
__device__ __forceinline__ void sample_walk(float px, float py, float pz, const float4* __restrict__ posm,
                                            const typename Sum::Payload* __restrict__ payload,
                                            const uint32_t* __restrict__ cell_start, const CellGrid& g,
                                            const PairConsts& k, Sum& s)
{
   int cx, cy, cz;
   probe_cell(g, px, py, pz, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      uint32_t b, e;
      row_range(r, row, b, e);
      for (uint32_t q = b; q < e; q++) {
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(px, py, pz, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < k.h2) s.template member<UNIT_SCALE>(k, d2, pj.w, payload, q);
      }
   }
}

// ---- point probes: one lane per probe ---------------------------------------------------------
template <bool UNIT_SCALE, class Sum>
__global__ void __launch_bounds__(256)
k_sample_points(const float* __restrict__ xyz, int n, const float4* __restrict__ posm,
                const typename Sum::Payload* __restrict__ payload, const uint32_t* __restrict__ cell_start, CellGrid g,
                PairConsts k, typename Sum::Out out)
{
   const int p = blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= n) return;
   Sum s;
   sample_walk<UNIT_SCALE>(xyz[3 * p + 0], xyz[3 * p + 1], xyz[3 * p + 2], posm, payload, cell_start, g, k, s);
   s.store(p, out);
}

// ---- lattice probes: one workgroup per brick --------------------------------------------------
// Outputs are indexed by the point's place in the chunk: ((kl * ey) + jl) * ex + il.
// Every lane walks per probe (the default route: sample_policy.h); no LDS.
template <bool UNIT_SCALE, class Sum>
__global__ void __launch_bounds__(SAMPLE_THREADS)
k_sample_lattice_walk(SampleLattice L, const float4* __restrict__ posm, const typename Sum::Payload* __restrict__ payload,
                      const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k, typename Sum::Out out)
{
   const int t = threadIdx.x;
   const int b = blockIdx.x;
   const int bx = b % L.bricks_x, by = (b / L.bricks_x) % L.bricks_y, bz = b / (L.bricks_x * L.bricks_y);
   const int il = bx * L.bx + t % L.bx;
   const int jl = by * L.by + (t / L.bx) % L.by;
   const int kl = bz * L.bz + t / (L.bx * L.by);
   if (!(il < L.ex && jl < L.ey && kl < L.ez)) return;
   // the lattice point, origin + (float)i * spacing per axis (unfused: -ffp-contract=off)
   const float px = L.ox + (float)(L.i0 + il) * L.sx;
   const float py = L.oy + (float)(L.j0 + jl) * L.sy;
   const float pz = L.oz + (float)(L.k0 + kl) * L.sz;
   const int o = (kl * L.ey + jl) * L.ex + il;
   Sum s;
   sample_walk<UNIT_SCALE>(px, py, pz, posm, payload, cell_start, g, k, s);
   s.store(o, out);
}

// The tiled route of the density and velocity sampler (SPH_HIP_SAMPLE_TILED=1): the tile of sample_policy.h,
// in dynamic LDS of tile_cap * (16 or 28) bytes, SoA: x[cap], y[cap], z[cap], m[cap] (, vx[cap], vy[cap], vz[cap]).
template <bool UNIT_SCALE, bool VEL>
__global__ void __launch_bounds__(SAMPLE_THREADS)
k_sample_lattice(SampleLattice L, const float4* __restrict__ posm, const float4* __restrict__ velp,
                 const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k, int tile_cap,
                 float* __restrict__ rho_out, float* __restrict__ vel_out, int32_t* __restrict__ cnt_out)
{
   const int t = threadIdx.x;
   const int b = blockIdx.x;
   const int bx = b % L.bricks_x, by = (b / L.bricks_x) % L.bricks_y, bz = b / (L.bricks_x * L.bricks_y);
   const int il = bx * L.bx + t % L.bx;
   const int jl = by * L.by + (t / L.bx) % L.by;
   const int kl = bz * L.bz + t / (L.bx * L.by);
   const bool valid = il < L.ex && jl < L.ey && kl < L.ez;
   // (the lattice point and its place in the chunk: k_sample_lattice_walk's)
   const float px = L.ox + (float)(L.i0 + il) * L.sx;
   const float py = L.oy + (float)(L.j0 + jl) * L.sy;
   const float pz = L.oz + (float)(L.k0 + kl) * L.sz;
   const int o = (kl * L.ey + jl) * L.ex + il;
   SampleSum<VEL> s;

   __shared__ uint32_t row_s[SAMPLE_MAX_ROWS];       // global start of each tile row
   __shared__ uint32_t row_b[SAMPLE_MAX_ROWS + 1];   // its LDS base; [nrows] = entries
   extern __shared__ float tile[];

   int cx, cy, cz;
   probe_cell(g, px, py, pz, cx, cy, cz);
   // The brick's cell box, from its first and last point per axis (the same values in every lane):
   // a point's coordinate grows with its index and so does its cell - as long as x * inv stays below
   // 2^31, past which (and at +inf) cell_coord gives cell 0; such a brick walks per probe.
   int c0[3], c1[3];
   bool box_ok = true;
   {
      const float o[3] = {L.ox, L.oy, L.oz}, sp[3] = {L.sx, L.sy, L.sz};
      const int first[3] = {L.i0 + bx * L.bx, L.j0 + by * L.by, L.k0 + bz * L.bz};
      const int last[3] = {L.i0 + min(L.ex, (bx + 1) * L.bx) - 1, L.j0 + min(L.ey, (by + 1) * L.by) - 1,
                           L.k0 + min(L.ez, (bz + 1) * L.bz) - 1};
      const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
      for (int a = 0; a < 3; a++) {
         const float x0 = o[a] + (float)first[a] * sp[a], x1 = o[a] + (float)last[a] * sp[a];
         box_ok = box_ok && floorf(x1 * g.inv) < 2147483648.0f;
         c0[a] = cell_coord(x0, g.inv, n[a]);
         c1[a] = cell_coord(x1, g.inv, n[a]);
      }
   }
   const int X0 = c0[0] - 1 < 0 ? 0 : c0[0] - 1, X1 = c1[0] + 1 >= g.nx ? g.nx - 1 : c1[0] + 1;
   const int Y0 = c0[1] - 1 < 0 ? 0 : c0[1] - 1, Y1 = c1[1] + 1 >= g.ny ? g.ny - 1 : c1[1] + 1;
   const int Z0 = c0[2] - 1 < 0 ? 0 : c0[2] - 1, Z1 = c1[2] + 1 >= g.nz ? g.nz - 1 : c1[2] + 1;
   const int ny_t = Y1 - Y0 + 1;
   const int nrows = ny_t * (Z1 - Z0 + 1);
   if (!box_ok || nrows > SAMPLE_MAX_ROWS) {
      // (uniform) more rows than the table holds, or a box that cannot be bounded: walk per probe
      if (!valid) return;
      sample_walk<UNIT_SCALE>(px, py, pz, posm, velp, cell_start, g, k, s);
      s.store(o, rho_out, vel_out, cnt_out);
      return;
   }
   // row table: wave 0 reads the rows' ranges and scans their lengths in registers
   if (t < SPH_WAVE) {
      uint32_t s0 = 0, len = 0;
      if (t < nrows) {
         const int row = ((Z0 + t / ny_t) * g.ny + Y0 + t % ny_t) * g.nx;
         s0 = cell_start[row + X0];
         len = cell_start[row + X1 + 1] - s0;
      }
      uint32_t inc = len;
#pragma unroll
      for (int d = 1; d < SPH_WAVE; d <<= 1) {
         const uint32_t v = __shfl_up(inc, d);
         if (t >= d) inc += v;
      }
      if (t < nrows) {
         row_s[t] = s0;
         row_b[t] = inc - len;
      }
      if (t == nrows - 1) row_b[nrows] = inc;
   }
   __syncthreads();
   const uint32_t total = row_b[nrows];
   if (total == 0) {
      // no particle anywhere in the bricks' neighbourhoods: nothing to stage, every sum is zero
      if (valid) s.store(o, rho_out, vel_out, cnt_out);
      return;
   }
   if (total > (uint32_t)tile_cap) {
      // a denser region than the capacity is sized for: this brick walks per probe, with the same bits
      if (!valid) return;
      sample_walk<UNIT_SCALE>(px, py, pz, posm, velp, cell_start, g, k, s);
      s.store(o, rho_out, vel_out, cnt_out);
      return;
   }
   float* tx = tile;
   float* ty = tx + tile_cap;
   float* tz = ty + tile_cap;
   float* tm = tz + tile_cap;
   float* tvx = tm + tile_cap;
   float* tvy = tvx + tile_cap;
   float* tvz = tvy + tile_cap;
   // stage: wave w copies rows w, w + 4, ..., 64 entries at a time
   const int wave = t / SPH_WAVE, lane = t % SPH_WAVE;
   for (int r = wave; r < nrows; r += SAMPLE_THREADS / SPH_WAVE) {
      const uint32_t base = row_b[r], len = row_b[r + 1] - base, src = row_s[r];
      for (uint32_t e = lane; e < len; e += SPH_WAVE) {
         const float4 pj = posm[src + e];
         tx[base + e] = pj.x;
         ty[base + e] = pj.y;
         tz[base + e] = pj.z;
         tm[base + e] = pj.w;
         if (VEL) {
            const float4 vj = velp[src + e];
            tvx[base + e] = vj.x;
            tvy[base + e] = vj.y;
            tvz[base + e] = vj.z;
         }
      }
   }
   __syncthreads();
   if (!valid) return;
   // the lane's 9 row segments, in canonical order: row (z, y) of the tile, cells x0..x1 of it
   const int x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
#pragma unroll 1
   for (int rr = 0; rr < 9; rr++) {
      const int z = cz + rr / 3 - 1, y = cy + rr % 3 - 1;
      if (z < 0 || z >= g.nz || y < 0 || y >= g.ny) continue;
      const int r = (z - Z0) * ny_t + (y - Y0);
      const int row = (z * g.ny + y) * g.nx;
      const uint32_t a = row_b[r] + (cell_start[row + x0] - row_s[r]);
      const uint32_t e = row_b[r] + (cell_start[row + x1 + 1] - row_s[r]);
      for (uint32_t q = a; q < e; q++) {
         float dx, dy, dz;
         const float d2 = dist2(px, py, pz, tx[q], ty[q], tz[q], dx, dy, dz);
         if (d2 < k.h2) {
            if (VEL) s.template add<UNIT_SCALE>(k, d2, tm[q], tvx[q], tvy[q], tvz[q]);
            else s.template add<UNIT_SCALE>(k, d2, tm[q], 0.0f, 0.0f, 0.0f);
         }
      }
   }
   s.store(o, rho_out, vel_out, cnt_out);
}

// Launch decisions of the field sampler (sample_kernels.h, sph_hip_sample_points / _lattice) as
// functions of plain values: the brick of lattice points one workgroup covers, the LDS tile
// capacity of a brick, the choice between the tiled and the per-probe walk, and the chunking that
// bounds the device scratch of large probe sets.
// The lattice argument checks, the scratch budget and the 256-byte rounding are shared with the
// iso-surface extractor (surface_policy.h) and the renderer (render_policy.h).
// Pure C++17 without HIP (tests/test_sample_cpu.py compiles it with g++); the environment switches
// (SPH_HIP_SAMPLE_UNTILED, SPH_HIP_SAMPLE_TILED, SPH_HIP_SAMPLE_CHUNK) are read by the caller and passed in.
#pragma once

#include <math.h>
#include <stdint.h>

// Why the lattice origin + i * spacing, dims points per axis, is refused, or nullptr.
inline const char* lattice_check(const float origin[3], const float spacing[3], const int32_t dims[3])
{
   if (!origin || !spacing || !dims) return "null origin, spacing or dims";
   long long total = 1;
   for (int a = 0; a < 3; a++) {
      if (dims[a] <= 0 || !isfinite(origin[a]) || !isfinite(spacing[a]) || !(spacing[a] > 0.0f))
         return "dims must be positive, the origin finite, the spacing finite and positive";
      total *= dims[a];
      if (total > 0x7fffffffll) return "more than 2^31 - 1 lattice points";
   }
   return nullptr;
}

// the lattice spacing in cell edges (inv: cells per unit length)
inline void sample_spacing_cells(const float spacing[3], float inv, double cells[3])
{
   for (int a = 0; a < 3; a++) cells[a] = spacing[a] * (double)inv;
}

// One workgroup = one brick of lattice points, SAMPLE_THREADS of them, x fastest.  Its shape is
// chosen per lattice from SAMPLE_BRICKS (sample_brick): lattices that span a scene's bounding box are
// far from cubic in cell units (a 256^3 lattice over the 4M dam column is 0.08 x 0.56 x 0.75 cell
// edges apart), and the shape that stages the fewest cells per point follows the spacing.
#define SAMPLE_THREADS 256
struct SampleBrick {
   int bx, by, bz;
};
#define SAMPLE_N_BRICKS 10
static const SampleBrick SAMPLE_BRICKS[SAMPLE_N_BRICKS] = {
    {8, 8, 4}, {16, 8, 2}, {16, 4, 4}, {8, 4, 8}, {4, 8, 8}, {32, 4, 2}, {32, 8, 1}, {16, 16, 1},
    {64, 2, 2}, {64, 4, 1}};

// The brick's tile: the particle ranges of the cell rows (one (cy, cz) row of cells = one contiguous
// range of the sorted state) that the 27-cell neighbourhoods of its points touch, as SoA in dynamic
// LDS: x, y, z, m (16 B per entry), + vx, vy, vz when velocity is sampled (28 B).
// Priced against the MI355X's 160 KiB of LDS per CU: 2560 entries are 40 KiB (density only: 3
// workgroups per CU, the row table's static LDS keeps a 4th out) or 70 KiB (with velocity: 2 per CU,
// 8 waves).  Halving the capacity would buy 5 / 4 workgroups per CU, but then a 128^3 lattice over
// the 4M dam column (264 cells per brick at best, sample_brick) would not fit it, and all its bricks
// would walk from global memory.
#define SAMPLE_TILE_CAP 2560
#define SAMPLE_TILE_BYTES_DENSITY 16
#define SAMPLE_TILE_BYTES_VELOCITY 28
// cell rows a tile may hold (static LDS: global start and LDS base per row); more -> per-probe walk
#define SAMPLE_MAX_ROWS 64

// At a spacing of a cell or more on every axis, each point is alone in its cell neighbourhood and a
// brick's tile is its 256 neighbourhoods side by side: staging reads every candidate once more than
// the walk does.  Such lattices always walk per probe.
#define SAMPLE_TILED_MIN_CELLS 1.0
// Entries per cell a tile is budgeted for: the 32-neighbour scenes hold about 7.6 per cell
// (32 / (4/3 pi) with a cell edge of h).  A brick in a denser region than that whose tile exceeds the
// capacity walks per probe, with the same bits.
#define SAMPLE_CELL_BUDGET 8

// Probes per chunk of a large probe set: the scratch holds a chunk's probes (3 floats per point
// probe) and outputs (density, count, 3 velocity floats): 8 words per point probe, 5 per lattice
// point, so 64 MiB / 40 MiB at most, whatever the caller asks for.  That 64 MiB is the device scratch
// budget the extractor's slabs and the renderer's row chunks are sized to as well.
#define SAMPLE_CHUNK_POINTS (1 << 21)
#define SAMPLE_SCRATCH_BUDGET (64ll << 20)

// SPH_HIP_SAMPLE_CHUNK=n (tests; read at context creation): the chunk limit of every sampler call, so
// that a small probe set takes several chunks.  0 or less: off, the compiled limits hold.  Otherwise
// clamped to [SAMPLE_THREADS, SAMPLE_CHUNK_POINTS]: below one brick sample_lattice_chunk would return
// an empty run of bricks, above the limit the scratch would exceed its budget.
inline int sample_chunk_forced(long long value)
{
   if (value <= 0) return 0;
   return (int)(value < SAMPLE_THREADS ? SAMPLE_THREADS : value > SAMPLE_CHUNK_POINTS ? SAMPLE_CHUNK_POINTS : value);
}

// the chunk limit of a call whose own limit is `limit`: the smaller of it and a forced one
inline int sample_chunk_limit(int limit, int forced) { return forced > 0 && forced < limit ? forced : limit; }

// scratch arrays start on 256-byte boundaries
inline long long round256(long long b) { return (b + 255) / 256 * 256; }

// Cells a brick's tile spans along one axis at the worst alignment: `points` points `spacing`
// cell edges apart touch floor((points - 1) * spacing) + 2 cells, and their neighbourhoods one
// more on each side.
inline int sample_tile_cells_axis(int points, double spacing_cells)
{
   if (points <= 1) return 3;
   return (int)((points - 1) * spacing_cells) + 4;
}

// the brick's points along each axis: fewer than the brick where the lattice is thinner
inline int sample_brick_points(int brick, int dim) { return dim < brick ? dim : brick; }

// Worst-case cells of the tile of brick b on the lattice (dims, spacing in cell edges).
inline long long sample_tile_cells(const SampleBrick& b, const int dims[3], const double spacing_cells[3])
{
   const int brick[3] = {b.bx, b.by, b.bz};
   long long cells = 1;
   for (int a = 0; a < 3; a++)
      cells *= sample_tile_cells_axis(sample_brick_points(brick[a], dims[a]), spacing_cells[a]);
   return cells;
}

// The brick shape that stages the fewest cells per lattice point of a brick (the first such in
// SAMPLE_BRICKS on a tie).
inline SampleBrick sample_brick(const int dims[3], const double spacing_cells[3])
{
   SampleBrick best = SAMPLE_BRICKS[0];
   double best_cost = 0.0;
   for (int i = 0; i < SAMPLE_N_BRICKS; i++) {
      const SampleBrick& b = SAMPLE_BRICKS[i];
      const double points = (double)sample_brick_points(b.bx, dims[0]) * sample_brick_points(b.by, dims[1]) *
                            sample_brick_points(b.bz, dims[2]);
      const double cost = (double)sample_tile_cells(b, dims, spacing_cells) / points;
      if (i == 0 || cost < best_cost) {
         best = b;
         best_cost = cost;
      }
   }
   return best;
}

// Whether the tile of brick b fits: the spacing decides (every axis of more than one point a cell
// or more apart: no), then the capacity: the brick's worst-case tile at SAMPLE_CELL_BUDGET entries
// per cell.  Bricks whose tile still exceeds the capacity (a denser region than budgeted) walk per
// probe inside the tiled kernel, with the same bits.
inline bool sample_tile_fits(const SampleBrick& b, const int dims[3], const double spacing_cells[3], int tile_cap)
{
   bool fine = false;
   for (int a = 0; a < 3; a++)
      if (dims[a] > 1 && !(spacing_cells[a] >= SAMPLE_TILED_MIN_CELLS)) fine = true;
   if (!fine) return false;
   return sample_tile_cells(b, dims, spacing_cells) * SAMPLE_CELL_BUDGET <= tile_cap;
}

// The route of a lattice: the switches SPH_HIP_SAMPLE_UNTILED=1 / SPH_HIP_SAMPLE_TILED=1 (read at
// context creation) or the default.  Measured on the 4M dam column (DESIGN.md section 11,
// profiles/sample_cost.txt), the tiled route cost 1.16 - 1.45 times the per-probe walk at every
// spacing tried, 0.08 to 0.76 cell edges, isotropic h/4 and h/2 included: the per-probe walk's
// neighbouring lanes read the same cells through L1, at full occupancy, while the tile holds the
// workgroups to 3 (2 with velocity) per CU.  So the default never tiles; SPH_HIP_SAMPLE_TILED=1 takes
// the tiled route wherever the tile fits (tests, A/B runs).
enum { SAMPLE_ROUTE_DEFAULT = 0, SAMPLE_ROUTE_UNTILED = 1, SAMPLE_ROUTE_TILED = 2 };
inline bool sample_use_tiled(const SampleBrick& b, const int dims[3], const double spacing_cells[3], int tile_cap,
                             int route_switch)
{
   if (route_switch != SAMPLE_ROUTE_TILED) return false;
   return sample_tile_fits(b, dims, spacing_cells, tile_cap);
}

// One chunk of a lattice: a box of points, as large as SAMPLE_CHUNK_POINTS allows, made of whole
// bricks wherever the lattice has more points than the chunk can hold: whole z-slabs of bricks
// first, then whole rows of bricks along y, then runs of bricks along x.
struct SampleChunk {
   int ex, ey, ez;   // points per chunk along each axis (the last chunk along an axis may be shorter)
};

inline SampleChunk sample_lattice_chunk(const int dims[3], const SampleBrick& b, long long max_points)
{
   SampleChunk c = {dims[0], dims[1], dims[2]};
   const long long plane = (long long)dims[0] * dims[1];
   if (plane * dims[2] <= max_points) return c;
   if (plane * b.bz <= max_points) {
      c.ez = (int)(max_points / plane / b.bz * b.bz);
      return c;
   }
   c.ez = dims[2] < b.bz ? dims[2] : b.bz;
   const long long row = (long long)dims[0] * c.ez;
   if (row * b.by <= max_points) {
      c.ey = (int)(max_points / row / b.by * b.by);
      return c;
   }
   c.ey = dims[1] < b.by ? dims[1] : b.by;
   const long long run = (long long)b.bx * c.ey * c.ez;
   c.ex = (int)(max_points / run * b.bx);
   return c;
}

// points of a point-probe set handled per chunk
inline int sample_points_chunk(int n, int max_points) { return n < max_points ? n : max_points; }

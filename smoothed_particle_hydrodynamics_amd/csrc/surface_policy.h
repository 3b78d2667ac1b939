// Decisions of the iso-surface extractor (surface_kernels.h, sph_hip_extract_surface) that need no
// GPU: the iso and flag checks, the Kuhn split of a lattice cube into six tetrahedra, the seven edges
// a lattice point owns, the oriented triangles of every tetrahedron case, and the z-slabs the lattice
// is meshed in.
// Pure C++17 without HIP (tests/test_surface_cpu.py compiles it with g++); the environment switch
// (SPH_HIP_SURFACE_PLANES) is read by the caller at context creation and passed in.
#pragma once

#include <stdint.h>

#include "../../include/sph_hip.h"
#include "sample_policy.h"

// Why the extractor's iso and flags are refused, or nullptr (the lattice: sample_policy.h, lattice_check).
inline const char* surf_check(float iso, int flags)
{
   if (!isfinite(iso) || !(iso > 0.0f)) return "iso must be finite and positive";
   if (flags & ~(SPH_HIP_SURFACE_NORMALS | SPH_HIP_SURFACE_VELOCITY)) return "unknown flag bits";
   return nullptr;
}

// corners of a lattice cube are numbered by bits: c = x + 2y + 4z (corner c is lattice point p + c)
// The seven positive-direction edges of a lattice point, in the canonical order of vertex ids:
// +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z, as corner bit masks.
#define SURF_EDGES 7
constexpr int surf_edge_dir(int e) { return e < 3 ? 1 << e : e == 3 ? 3 : e == 4 ? 5 : e == 5 ? 6 : 7; }

// the place of direction d (1..7) in that order
constexpr int surf_edge_index(int d) { return d == 1 ? 0 : d == 2 ? 1 : d == 4 ? 2 : d == 3 ? 3 : d == 5 ? 4 : d == 6 ? 5 : 6; }

// Kuhn (Freudenthal) split: tetrahedron {0, a, a|b, 7} for (a, b) = (1,2), (1,4), (2,1), (2,4), (4,1), (4,2).
#define SURF_TETS 6
constexpr int surf_tet_a(int t) { return t < 2 ? 1 : t < 4 ? 2 : 4; }
constexpr int surf_tet_b(int t) { return t == 0 ? 2 : t == 1 ? 4 : t == 2 ? 1 : t == 3 ? 4 : t == 4 ? 1 : 2; }

// A cube edge used by the split runs from corner lo to corner hi with lo a subset of hi: it is the
// edge of lattice point p + lo in direction hi ^ lo.  Its key, lo * 7 + surf_edge_index(hi ^ lo),
// orders the vertices of one cube as their ids do (ids grow with the owner's lattice index, which
// grows with lo as long as the lattice has a cube, then with the edge's place).
constexpr int surf_edge_key(int lo, int hi) { return lo * SURF_EDGES + surf_edge_index(hi ^ lo); }
constexpr int surf_key_corner(int key) { return key / SURF_EDGES; }
constexpr int surf_key_edge(int key) { return key % SURF_EDGES; }

// Tetrahedron t's corners in path order: 0, a, a|b, 7.
constexpr int surf_tet_corner(int t, int i)
{
   return i == 0 ? 0 : i == 1 ? surf_tet_a(t) : i == 2 ? (surf_tet_a(t) | surf_tet_b(t)) : 7;
}

// The triangles of tetrahedron t in case m (bit i of m: corner i of the path is inside, f > iso):
// n = 0, 1 or 2; key[0..2] one triangle, key[0..3] the quad (key0, key1, key2), (key0, key2, key3).
// Each cycle starts at its smallest key (= smallest vertex id) and is oriented so that, with its
// vertices at the edge midpoints, (v1 - v0) x (v2 - v0) points from the inside corners toward the
// outside ones.
struct SurfCase {
   int n;
   int key[4];
};
struct SurfCases {
   SurfCase c[SURF_TETS][16];
};

namespace surf_detail {
struct V3 {
   int x, y, z;
};
constexpr V3 corner_pos(int c) { return {c & 1, (c >> 1) & 1, (c >> 2) & 1}; }
// twice the midpoint of the edge between corners a and b
constexpr V3 mid2(int a, int b)
{
   return {corner_pos(a).x + corner_pos(b).x, corner_pos(a).y + corner_pos(b).y, corner_pos(a).z + corner_pos(b).z};
}
constexpr V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
constexpr V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
constexpr int dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// orient the cycle of (lo, hi) corner pairs, then start it at its smallest key
constexpr SurfCase make_cycle(const int (&ends)[4][2], int n, V3 toward_out)
{
   SurfCase s = {n == 3 ? 1 : 2, {0, 0, 0, 0}};
   int lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
   for (int i = 0; i < n; i++) {
      lo[i] = ends[i][0] < ends[i][1] ? ends[i][0] : ends[i][1];
      hi[i] = ends[i][0] < ends[i][1] ? ends[i][1] : ends[i][0];
   }
   const V3 p0 = mid2(lo[0], hi[0]), p1 = mid2(lo[1], hi[1]), p2 = mid2(lo[2], hi[2]);
   const bool flip = dot(cross(sub(p1, p0), sub(p2, p0)), toward_out) < 0;
   int key[4] = {0, 0, 0, 0};
   for (int i = 0; i < n; i++) {
      const int j = flip ? (n - i) % n : i;   // reversed cycle, same start
      key[i] = surf_edge_key(lo[j], hi[j]);
   }
   int first = 0;
   for (int i = 1; i < n; i++)
      if (key[i] < key[first]) first = i;
   for (int i = 0; i < n; i++) s.key[i] = key[(first + i) % n];
   return s;
}

constexpr SurfCases make_cases()
{
   SurfCases out = {};
   for (int t = 0; t < SURF_TETS; t++)
      for (int m = 0; m < 16; m++) {
         int in[4] = {0, 0, 0, 0}, ni = 0, ou[4] = {0, 0, 0, 0}, no = 0;
         for (int i = 0; i < 4; i++) {
            if ((m >> i) & 1) in[ni++] = surf_tet_corner(t, i);
            else ou[no++] = surf_tet_corner(t, i);
         }
         out.c[t][m] = SurfCase{0, {0, 0, 0, 0}};
         if (ni == 0 || no == 0) continue;
         // from the inside corners' centroid toward the outside corners' (times ni * no)
         V3 si = {0, 0, 0}, so = {0, 0, 0};
         for (int i = 0; i < ni; i++) {
            si.x += corner_pos(in[i]).x; si.y += corner_pos(in[i]).y; si.z += corner_pos(in[i]).z;
         }
         for (int i = 0; i < no; i++) {
            so.x += corner_pos(ou[i]).x; so.y += corner_pos(ou[i]).y; so.z += corner_pos(ou[i]).z;
         }
         const V3 toward_out = {ni * so.x - no * si.x, ni * so.y - no * si.y, ni * so.z - no * si.z};
         int ends[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
         if (ni == 1) {
            for (int i = 0; i < 3; i++) { ends[i][0] = in[0]; ends[i][1] = ou[i]; }
            out.c[t][m] = make_cycle(ends, 3, toward_out);
         } else if (no == 1) {
            for (int i = 0; i < 3; i++) { ends[i][0] = in[i]; ends[i][1] = ou[0]; }
            out.c[t][m] = make_cycle(ends, 3, toward_out);
         } else {
            // the quad I0O0, I0O1, I1O1, I1O0: consecutive edges share a corner
            ends[0][0] = in[0]; ends[0][1] = ou[0];
            ends[1][0] = in[0]; ends[1][1] = ou[1];
            ends[2][0] = in[1]; ends[2][1] = ou[1];
            ends[3][0] = in[1]; ends[3][1] = ou[0];
            out.c[t][m] = make_cycle(ends, 4, toward_out);
         }
      }
   return out;
}
} // namespace surf_detail

static constexpr SurfCases SURF_CASES = surf_detail::make_cases();

// triangles a tetrahedron emits for k of its 4 corners inside
constexpr int surf_tet_triangles(int k) { return k == 1 || k == 3 ? 1 : k == 2 ? 2 : 0; }

// The inside bits (bit i: path corner i) of tetrahedron t in a cube whose corner c is inside
// where bit c of cube_in is set.
constexpr int surf_tet_case(int t, int cube_in)
{
   return ((cube_in >> surf_tet_corner(t, 0)) & 1) | (((cube_in >> surf_tet_corner(t, 1)) & 1) << 1) |
          (((cube_in >> surf_tet_corner(t, 2)) & 1) << 2) | (((cube_in >> surf_tet_corner(t, 3)) & 1) << 3);
}

// ---- slabs -------------------------------------------------------------------------------------
// The lattice is meshed in z-slabs of P planes.  A slab samples its planes plus 1 below and 2 above
// (the normals' central differences), classifies P + 1 planes (the plane above holds the seam's
// vertices: their ids are needed before the next slab emits them) and emits the vertices and cubes
// of its own P planes.  Device scratch, in bytes:
//   per sampled point     density + count (8), + velocity (12) when it is asked for;
//   per classified point  crossing code (1) + vertex offset (4);
//   per own point         active-cube entry (8: cube index, triangle offset);
//   per 256 points        block sums and offsets (20).
#define SURF_THREADS 256
#define SURF_SCRATCH_BUDGET SAMPLE_SCRATCH_BUDGET   // the sampler's chunk budget (sample_policy.h)
#define SURF_HALO_BELOW 1
#define SURF_HALO_ABOVE 2

struct SurfScratch {
   long long sampled, classified, own, blocks;   // points of each kind, workgroups of a slab
   long long bytes;                              // total, each array rounded up to 256 bytes
};

inline SurfScratch surf_scratch(const int dims[3], int planes, bool velocity)
{
   const long long plane = (long long)dims[0] * dims[1];
   const int sampled = planes + SURF_HALO_BELOW + SURF_HALO_ABOVE;
   SurfScratch s;
   s.sampled = plane * (sampled < dims[2] ? sampled : dims[2]);
   s.classified = plane * (planes + 1 < dims[2] ? planes + 1 : dims[2]);
   s.own = plane * (planes < dims[2] ? planes : dims[2]);
   s.blocks = (s.classified + SURF_THREADS - 1) / SURF_THREADS;
   s.bytes = round256(s.sampled * 4) * (velocity ? 5 : 2) + round256(s.classified) +
             round256(s.classified * 4) + round256(s.own * 8) + 5 * round256(s.blocks * 4);
   return s;
}

// Planes per slab: the most that keep the scratch within the budget (at least 1), or `forced`
// (SPH_HIP_SURFACE_PLANES=n, tests) when it is > 0; never more than the lattice has.
inline int surf_planes(const int dims[3], bool velocity, int forced)
{
   if (forced > 0) return forced < dims[2] ? forced : dims[2];
   int lo = 1, hi = dims[2];
   while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (surf_scratch(dims, mid, velocity).bytes <= SURF_SCRATCH_BUDGET) lo = mid;
      else hi = mid - 1;
   }
   return lo;
}

// Classified points of one slab must keep every in-slab count below 2^32 (7 vertices and 12
// triangles per point at most); larger planes are refused (SPH_HIP_ERR_CAPACITY).
#define SURF_MAX_SLAB_POINTS (1ll << 28)

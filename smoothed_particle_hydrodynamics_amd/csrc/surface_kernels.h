// Iso-surface extractor (sph_hip_extract_surface): an indexed triangle mesh of {f > iso} over the
// field sampler's density lattice, by the Kuhn split of every lattice cube into six tetrahedra.
// include/sph_hip.h states the contract (which edges carry vertices, their ids, positions, normals
// and velocities, the triangles and their order); surface_policy.h holds the tables and the slab
// sizing; tests/surface_emulation.py restates the contract in numpy, bit for bit.
//
// One z-slab of the lattice (surface_policy.h) takes five launches, in this order:
//   k_sample_lattice    (sample_kernels.h) the slab's planes plus its halo: density (+ velocity);
//   k_surf_classify     one lane per classified point: crossing code (7 edge bits + inside bit),
//                       block sums of the packed counts (vertices | triangles << 11 | active << 23)
//                       and of the vertices of the slab's own planes;
//   k_surf_scan         one workgroup: block offsets, and the running totals of the slab after
//                       this one (device, 64-bit), the carry across slabs;
//   k_surf_vertices     one lane per classified point: its vertex id base (stored for the seam and
//                       the triangles), the compacted active cubes, and the vertices of its crossing
//                       edges (own planes only) - a wave without any skips the field reads;
//   k_surf_triangles    one lane per active cube: the triangles of its six tetrahedra.
// Every output place is a scanned offset: nothing depends on arrival order.
#pragma once

#include "cell_build.h"
#include "surface_policy.h"

// the case table in constant memory (surface_policy.h builds it at compile time)
__constant__ SurfCases c_surf_cases = SURF_CASES;

// One slab of the caller's lattice (nx, ny, nz points).  Local index of a classified point:
// (kz - k0) * plane + j * nx + i; of a sampled one: (kz - ks0) * plane + j * nx + i.
struct SurfSlab {
   int nx, ny, nz, plane;
   int k0;        // first own plane
   int own;       // own planes (vertices and cubes emitted here)
   int cls;       // classified planes: own + the next slab's first plane where it exists
   int ks0;       // first sampled plane (k0 - 1 where it exists)
   float ox, oy, oz, sx, sy, sz;   // lattice origin and spacing
   float iso;
};

// packed per-lane counts: block totals stay below each field's width (256 lanes: 1792, 3072, 256)
#define SURF_PACK_T 11
#define SURF_PACK_A 23
#define SURF_PACK_VMASK 0x7ffu
#define SURF_PACK_TMASK 0xfffu

__device__ __forceinline__ bool surf_inside(float f, float iso) { return f > iso; }   // NaN: outside

// inside bits of the cube at a point whose code is `code` (valid where the cube exists)
__device__ __forceinline__ int surf_cube_in(int code)
{
   const int in0 = code >> 7;
   int cin = in0;
#pragma unroll
   for (int c = 1; c < 8; c++) cin |= (in0 ^ ((code >> surf_edge_index(c)) & 1)) << c;
   return cin;
}

__device__ __forceinline__ int surf_cube_triangles(int cin)
{
   int n = 0;
#pragma unroll
   for (int t = 0; t < SURF_TETS; t++) n += surf_tet_triangles(__popc(surf_tet_case(t, cin)));
   return n;
}

// crossing code of a lattice point (bits 0..6: crossing edges in surf_edge_dir order; bit 7: inside)
// and the inside bits of its cube (-1 where the cube does not exist)
__device__ __forceinline__ int surf_code(const SurfSlab& S, const float* __restrict__ rho, int i, int j, int kz, int& cin)
{
   const int base = (kz - S.ks0) * S.plane + j * S.nx + i;
   const bool hx = i + 1 < S.nx, hy = j + 1 < S.ny, hz = kz + 1 < S.nz;
   int in = 0;
#pragma unroll
   for (int c = 0; c < 8; c++) {
      const bool ex = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
      if (ex) {
         const float f = rho[base + ((c & 1) ? 1 : 0) + ((c & 2) ? S.nx : 0) + ((c & 4) ? S.plane : 0)];
         in |= (surf_inside(f, S.iso) ? 1 : 0) << c;
      }
   }
   const int in0 = in & 1;
   int code = in0 << 7;
#pragma unroll
   for (int e = 0; e < SURF_EDGES; e++) {
      const int d = surf_edge_dir(e);
      const bool ex = (!(d & 1) || hx) && (!(d & 2) || hy) && (!(d & 4) || hz);
      if (ex && (((in >> d) & 1) != in0)) code |= 1 << e;
   }
   cin = hx && hy && hz ? in : -1;
   return code;
}

__global__ void __launch_bounds__(SURF_THREADS)
k_surf_classify(SurfSlab S, const float* __restrict__ rho, uint8_t* __restrict__ code_out,
                uint32_t* __restrict__ bsum_pack, uint32_t* __restrict__ bsum_vown)
{
   const int q = blockIdx.x * SURF_THREADS + threadIdx.x;
   uint32_t pack = 0, vown = 0;
   if (q < S.cls * S.plane) {
      const int kl = q / S.plane, r = q - kl * S.plane;
      const int j = r / S.nx, i = r - j * S.nx;
      int cin;
      const int code = surf_code(S, rho, i, j, S.k0 + kl, cin);
      code_out[q] = (uint8_t)code;
      const uint32_t nv = __popc(code & 0x7f);
      pack = nv;
      if (kl < S.own) {
         vown = nv;
         if (cin > 0 && cin < 255) pack |= ((uint32_t)surf_cube_triangles(cin) << SURF_PACK_T) | (1u << SURF_PACK_A);
      }
   }
   uint32_t total;
   block_exclusive_scan(pack, &total);
   if (threadIdx.x == 0) bsum_pack[blockIdx.x] = total;
   block_exclusive_scan(vown, &total);
   if (threadIdx.x == 0) bsum_vown[blockIdx.x] = total;
}

// One workgroup: exclusive offsets of the blocks' vertices, triangles and active cubes inside the
// slab, and the totals: base[0..1] = vertex and triangle ids before this slab (in), next[0..3] =
// the same before the next slab, this slab's active cubes, its classified points' vertices (out).
__global__ void __launch_bounds__(SURF_THREADS)
k_surf_scan(int nb, const uint32_t* __restrict__ bsum_pack, const uint32_t* __restrict__ bsum_vown,
            uint32_t* __restrict__ boff_v, uint32_t* __restrict__ boff_t, uint32_t* __restrict__ boff_a,
            const unsigned long long* __restrict__ base, unsigned long long* __restrict__ next)
{
   const int per = (nb + SURF_THREADS - 1) / SURF_THREADS;
   const int b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
   uint32_t sv = 0, st = 0, sa = 0, so = 0;
   for (int b = b0; b < b1; b++) {
      const uint32_t p = bsum_pack[b];
      sv += p & SURF_PACK_VMASK;
      st += (p >> SURF_PACK_T) & SURF_PACK_TMASK;
      sa += p >> SURF_PACK_A;
      so += bsum_vown[b];
   }
   uint32_t tv, tt, ta, to;
   uint32_t ov = block_exclusive_scan(sv, &tv);
   uint32_t ot = block_exclusive_scan(st, &tt);
   uint32_t oa = block_exclusive_scan(sa, &ta);
   block_exclusive_scan(so, &to);
   for (int b = b0; b < b1; b++) {
      const uint32_t p = bsum_pack[b];
      boff_v[b] = ov;
      boff_t[b] = ot;
      boff_a[b] = oa;
      ov += p & SURF_PACK_VMASK;
      ot += (p >> SURF_PACK_T) & SURF_PACK_TMASK;
      oa += p >> SURF_PACK_A;
   }
   if (threadIdx.x == 0) {
      next[0] = base[0] + to;
      next[1] = base[1] + tt;
      next[2] = ta;
      next[3] = tv;
   }
}

// Lattice gradient of the sampled density at (i, j, kz), include/sph_hip.h: central differences
// (f[+1] - f[-1]) / (2 * s), one-sided (f[+1] - f) / s and (f - f[-1]) / s on the faces, 0 along
// an axis of one point.
__device__ __forceinline__ void surf_gradient(const SurfSlab& S, const float* __restrict__ rho, int i, int j, int kz,
                                              float g[3])
{
   const int o = (kz - S.ks0) * S.plane + j * S.nx + i;
   const int n[3] = {S.nx, S.ny, S.nz}, at[3] = {i, j, kz}, step[3] = {1, S.nx, S.plane};
   const float s[3] = {S.sx, S.sy, S.sz};
#pragma unroll
   for (int a = 0; a < 3; a++) {
      if (n[a] == 1) g[a] = 0.0f;
      else if (at[a] == 0) g[a] = (rho[o + step[a]] - rho[o]) / s[a];
      else if (at[a] == n[a] - 1) g[a] = (rho[o] - rho[o - step[a]]) / s[a];
      else g[a] = (rho[o + step[a]] - rho[o - step[a]]) / (2.0f * s[a]);
   }
}

template <bool NORMALS, bool VEL>
__global__ void __launch_bounds__(SURF_THREADS)
k_surf_vertices(SurfSlab S, const float* __restrict__ rho, const float* __restrict__ vel,
                const uint8_t* __restrict__ codes, const uint32_t* __restrict__ boff_v,
                const uint32_t* __restrict__ boff_t, const uint32_t* __restrict__ boff_a,
                const unsigned long long* __restrict__ base, int32_t* __restrict__ vbase, int2* __restrict__ active,
                float* __restrict__ vtx, float* __restrict__ nrm, float* __restrict__ vout)
{
   const int q = blockIdx.x * SURF_THREADS + threadIdx.x;
   const bool valid = q < S.cls * S.plane;
   int kl = 0, i = 0, j = 0, code = 0;
   uint32_t pack = 0;
   bool own = false, act = false;
   if (valid) {
      kl = q / S.plane;
      const int r = q - kl * S.plane;
      j = r / S.nx;
      i = r - j * S.nx;
      code = codes[q];
      own = kl < S.own;
      pack = __popc(code & 0x7f);
      if (own && i + 1 < S.nx && j + 1 < S.ny && S.k0 + kl + 1 < S.nz) {
         const int cin = surf_cube_in(code);
         if (cin > 0 && cin < 255) {
            act = true;
            pack |= ((uint32_t)surf_cube_triangles(cin) << SURF_PACK_T) | (1u << SURF_PACK_A);
         }
      }
   }
   uint32_t total;
   const uint32_t ex = block_exclusive_scan(pack, &total);
   if (!valid) return;
   const long long vid = (long long)base[0] + boff_v[blockIdx.x] + (ex & SURF_PACK_VMASK);
   vbase[q] = (int32_t)vid;
   if (act)
      active[boff_a[blockIdx.x] + (ex >> SURF_PACK_A)] =
          make_int2(q, (int)((long long)base[1] + boff_t[blockIdx.x] + ((ex >> SURF_PACK_T) & SURF_PACK_TMASK)));
   const bool emit = own && (code & 0x7f) != 0;
   if (__ballot(emit) == 0ull) return;   // (wave-uniform) most waves meet no surface
   if (!emit) return;
   const int kz = S.k0 + kl;
   const int oa = (kz - S.ks0) * S.plane + j * S.nx + i;
   const float fa = rho[oa];
   const float xa = S.ox + (float)i * S.sx, ya = S.oy + (float)j * S.sy, za = S.oz + (float)kz * S.sz;
   float ga[3] = {0.0f, 0.0f, 0.0f};
   if (NORMALS) surf_gradient(S, rho, i, j, kz, ga);
   int v = (int)vid;
#pragma unroll
   for (int e = 0; e < SURF_EDGES; e++) {
      if (!((code >> e) & 1)) continue;
      const int d = surf_edge_dir(e);
      const int ib = i + (d & 1), jb = j + ((d >> 1) & 1), kb = kz + ((d >> 2) & 1);
      const int ob = oa + (d & 1) + ((d & 2) ? S.nx : 0) + ((d & 4) ? S.plane : 0);
      const float fb = rho[ob];
      float t = (S.iso - fa) / (fb - fa);
      t = fminf(fmaxf(t, 0.0f), 1.0f);
      const float xb = S.ox + (float)ib * S.sx, yb = S.oy + (float)jb * S.sy, zb = S.oz + (float)kb * S.sz;
      vtx[3 * (size_t)v + 0] = xa + t * (xb - xa);
      vtx[3 * (size_t)v + 1] = ya + t * (yb - ya);
      vtx[3 * (size_t)v + 2] = za + t * (zb - za);
      if (NORMALS) {
         float gb[3];
         surf_gradient(S, rho, ib, jb, kb, gb);
         const float gx = ga[0] + t * (gb[0] - ga[0]);
         const float gy = ga[1] + t * (gb[1] - ga[1]);
         const float gz = ga[2] + t * (gb[2] - ga[2]);
         const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
         const bool ok = isfinite(len) && len > 0.0f;
         nrm[3 * (size_t)v + 0] = ok ? -(gx / len) : 0.0f;
         nrm[3 * (size_t)v + 1] = ok ? -(gy / len) : 0.0f;
         nrm[3 * (size_t)v + 2] = ok ? -(gz / len) : 0.0f;
      }
      if (VEL) {
         for (int c = 0; c < 3; c++) {
            const float va = vel[3 * (size_t)oa + c], vb = vel[3 * (size_t)ob + c];
            vout[3 * (size_t)v + c] = va + t * (vb - va);
         }
      }
      v++;
   }
}

// one lane per active cube: vertex ids of the cube's edges from the stored bases and codes
__global__ void __launch_bounds__(SURF_THREADS)
k_surf_triangles(SurfSlab S, const uint8_t* __restrict__ codes, const int32_t* __restrict__ vbase,
                 const int2* __restrict__ active, int nactive, int32_t* __restrict__ tri)
{
   const int a = blockIdx.x * SURF_THREADS + threadIdx.x;
   if (a >= nactive) return;
   const int2 e = active[a];
   const int q = e.x;
   int out = e.y;
   const int cin = surf_cube_in(codes[q]);
#pragma unroll
   for (int t = 0; t < SURF_TETS; t++) {
      const SurfCase& sc = c_surf_cases.c[t][surf_tet_case(t, cin)];
      if (sc.n == 0) continue;
      int id[4];
      for (int k = 0; k < 2 + sc.n; k++) {
         const int c = surf_key_corner(sc.key[k]), ed = surf_key_edge(sc.key[k]);
         const int qc = q + (c & 1) + ((c & 2) ? S.nx : 0) + ((c & 4) ? S.plane : 0);
         id[k] = vbase[qc] + __popc(codes[qc] & ((1u << ed) - 1u));
      }
      tri[3 * (size_t)out + 0] = id[0];
      tri[3 * (size_t)out + 1] = id[1];
      tri[3 * (size_t)out + 2] = id[2];
      out++;
      if (sc.n == 2) {
         tri[3 * (size_t)out + 0] = id[0];
         tri[3 * (size_t)out + 1] = id[2];
         tri[3 * (size_t)out + 2] = id[3];
         out++;
      }
   }
}

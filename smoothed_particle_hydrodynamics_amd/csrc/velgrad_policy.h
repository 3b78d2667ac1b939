// Velocity gradients (include/sph_hip.h: velocity gradients): vorticity, divergence, strain rate and the Q criterion of
// every particle, from a weighted least-squares fit of the velocity over its neighbours - the renormalised gradient of
// Randles and Libersky (1996), G = B * inverse(M) with B = sum_j w_j (v_i - v_j) (x) (r_i - r_j) and
// M = sum_j w_j (r_i - r_j) (x) (r_i - r_j).  It reads no density, and it is exact on a linear velocity field for any
// arrangement of neighbours whose M can be inverted - at a free surface and at a wall too, where the plain SPH gradient
// sum falls apart.  The arithmetic of one particle and every check: one set of inline functions for the device
// (velgrad_kernels.h) and for g++ (tests/test_velgrad_cpu.py, against the numpy restatement tests/velgrad_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written here.  For particle i of the sorted state a cell
// build of the current state has just produced:
//   members   cohesion's: j with d2 = (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i itself excluded, in
//             canonical order (ascending FULL cell id, then ascending sorted index)
//   weight    w_j = the density pass's pair term m_j * (kernel1 * (hscaled2 - d*d)^3) of d = sqrt(d2), correctly
//             rounded, times sim_scale unless the context runs at unit scale: density_term of pair_math.h, which only
//             the device compiles.  The kernel calls it and hands w_j to velgrad_pair; a member with d > hscaled off
//             unit scale therefore adds w_j = +0.0f terms (and counts as a member).
//   r, u      r = (dx, dy, dz), times sim_scale first unless unit scale; u = v_i - v_j
//   sums      fifteen named accumulators from 0.0f.  Per member q_a = w * r_a and p_a = w * u_a, then
//             M_ab = M_ab + q_a * r_b for xx, xy, xz, yy, yz, zz and B_ab = B_ab + p_a * r_b for all nine (velgrad_pair)
//   inverse   the six cofactors of the symmetric M:
//                c00 = m11*m22 - m12*m12   c01 = m02*m12 - m01*m22   c02 = m01*m12 - m02*m11
//                c11 = m00*m22 - m02*m02   c12 = m01*m02 - m00*m12   c22 = m00*m11 - m01*m01
//             det = (m00*c00 + m01*c01) + m02*c02, t = ((m00 + m11) + m22) * (1.0f / 3.0f)
//   valid     at least VELGRAD_MIN_MEMBERS members and det > VELGRAD_MIN_DET_RATIO * ((t*t)*t); a NaN fails the
//             comparison.  det / t^3 is 1 for an isotropic neighbourhood and 0 for a coplanar one: the constant is a
//             condition on the fit, not a measurement.
//   gradient  G_ab = ((B_a0*c_0b + B_a1*c_1b) + B_a2*c_2b) / det = dv_a / dx_b
//   outputs   A  = (w_x, w_y, w_z, div): w = (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy), div = (G_xx + G_yy) + G_zz
//             B' = (strain, Q, |w|, valid) with S = (G + G^T)/2, O = (G - G^T)/2:
//                s_ab = 0.5f * (G_ab + G_ba) off the diagonal,
//                ss = ((G_xx*G_xx + G_yy*G_yy) + G_zz*G_zz) + 2.0f * ((s_xy*s_xy + s_xz*s_xz) + s_yz*s_yz)   (S:S)
//                ww = (w_x*w_x + w_y*w_y) + w_z*w_z, oo = 0.5f * ww                                        (O:O)
//                strain = sqrt(2.0f * ss), Q = 0.5f * (oo - ss), |w| = sqrt(ww), valid = 1.0f
//             with sqrtf and "/" correctly rounded, on the device as under g++.
//   guard     a particle that is not valid, or whose eight values are not all finite, stores +0.0f in all eight.
//   units     r is the scaled separation, so G is the gradient per unit of scaled length, dv_a / d(sim_scale * x_b): off
//             unit scale a field v = A x gives G = A / sim_scale, and every output scales with it.
// Range.  M's entries and t are of the order 0.4 * (members / 32) * m / hscaled, det and t^3 of its cube and a cofactor
// of its square.  On the particles of droplet(3000) (h = 0.0576, unit masses) with 20 or more members det and t^3 lie
// in [27, 1.4e4] at unit scale and under SHELL and in [1.3e3, 7.9e4] at sim_scale = 0.5; tests/param_cases.py's
// h = 0.1 gives a fifth of the first.  They would leave fp32's normal range only for m / hscaled beyond 1e12 or below
// 1e-12, so no power-of-two rescaling of M is applied.
// FULL and FULL_FAST share the arithmetic: positions, masses and velocities are all the pass reads, and the two modes
// form none of them differently.  It writes its own two arrays only.
#pragma once

#include <math.h>

#include "scalar_policy.h"

#define VELGRAD_MIN_MEMBERS 3
#define VELGRAD_MIN_DET_RATIO 0.0009765625f   // 2^-10

// the running sums of one particle (every component written out: no array, which on the device could live in
// scratch memory)
struct VelgradSums {
   float mxx, mxy, mxz, myy, myz, mzz;
   float bxx, bxy, bxz, byx, byy, byz, bzx, bzy, bzz;   // b_ab: velocity component a, direction b
   int count;
};

SCALAR_HD SCALAR_INLINE inline VelgradSums velgrad_zero()
{
   return VelgradSums{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0};
}

// the eight values of one particle, in the order of SPH_HIP_VELGRAD_*
struct VelgradRows {
   float wx, wy, wz, div;
   float strain, q, wmag, valid;
};

// one member into the sums: w = its weight, (dx, dy, dz) = r_i - r_j, (ux, uy, uz) = v_i - v_j
SCALAR_HD SCALAR_INLINE inline void velgrad_pair(VelgradSums& s, float w, float dx, float dy, float dz, float ux, float uy,
                                                 float uz, float sim_scale, bool unit_scale)
{
   const float rx = unit_scale ? dx : dx * sim_scale;
   const float ry = unit_scale ? dy : dy * sim_scale;
   const float rz = unit_scale ? dz : dz * sim_scale;
   const float qx = w * rx, qy = w * ry, qz = w * rz;
   const float px = w * ux, py = w * uy, pz = w * uz;
   s.mxx = s.mxx + qx * rx;
   s.mxy = s.mxy + qx * ry;
   s.mxz = s.mxz + qx * rz;
   s.myy = s.myy + qy * ry;
   s.myz = s.myz + qy * rz;
   s.mzz = s.mzz + qz * rz;
   s.bxx = s.bxx + px * rx;
   s.bxy = s.bxy + px * ry;
   s.bxz = s.bxz + px * rz;
   s.byx = s.byx + py * rx;
   s.byy = s.byy + py * ry;
   s.byz = s.byz + py * rz;
   s.bzx = s.bzx + pz * rx;
   s.bzy = s.bzy + pz * ry;
   s.bzz = s.bzz + pz * rz;
   s.count = s.count + 1;
}

// the particle's eight values from its sums
SCALAR_HD SCALAR_INLINE inline VelgradRows velgrad_finish(const VelgradSums& s)
{
   const VelgradRows none = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
   const float c00 = s.myy * s.mzz - s.myz * s.myz;
   const float c01 = s.mxz * s.myz - s.mxy * s.mzz;
   const float c02 = s.mxy * s.myz - s.mxz * s.myy;
   const float c11 = s.mxx * s.mzz - s.mxz * s.mxz;
   const float c12 = s.mxy * s.mxz - s.mxx * s.myz;
   const float c22 = s.mxx * s.myy - s.mxy * s.mxy;
   const float det = (s.mxx * c00 + s.mxy * c01) + s.mxz * c02;
   const float t = ((s.mxx + s.myy) + s.mzz) * (1.0f / 3.0f);
   const bool valid = s.count >= VELGRAD_MIN_MEMBERS && det > VELGRAD_MIN_DET_RATIO * ((t * t) * t);
   if (!valid) return none;
   const float gxx = ((s.bxx * c00 + s.bxy * c01) + s.bxz * c02) / det;
   const float gxy = ((s.bxx * c01 + s.bxy * c11) + s.bxz * c12) / det;
   const float gxz = ((s.bxx * c02 + s.bxy * c12) + s.bxz * c22) / det;
   const float gyx = ((s.byx * c00 + s.byy * c01) + s.byz * c02) / det;
   const float gyy = ((s.byx * c01 + s.byy * c11) + s.byz * c12) / det;
   const float gyz = ((s.byx * c02 + s.byy * c12) + s.byz * c22) / det;
   const float gzx = ((s.bzx * c00 + s.bzy * c01) + s.bzz * c02) / det;
   const float gzy = ((s.bzx * c01 + s.bzy * c11) + s.bzz * c12) / det;
   const float gzz = ((s.bzx * c02 + s.bzy * c12) + s.bzz * c22) / det;
   VelgradRows r;
   r.wx = gzy - gyz;
   r.wy = gxz - gzx;
   r.wz = gyx - gxy;
   r.div = (gxx + gyy) + gzz;
   const float sxy = 0.5f * (gxy + gyx), sxz = 0.5f * (gxz + gzx), syz = 0.5f * (gyz + gzy);
   const float ss = ((gxx * gxx + gyy * gyy) + gzz * gzz) + 2.0f * ((sxy * sxy + sxz * sxz) + syz * syz);
   const float ww = (r.wx * r.wx + r.wy * r.wy) + r.wz * r.wz;
   const float oo = 0.5f * ww;
   r.strain = sqrtf(2.0f * ss);
   r.q = 0.5f * (oo - ss);
   r.wmag = sqrtf(ww);
   r.valid = 1.0f;
   const bool finite = scalar_finite(r.wx) && scalar_finite(r.wy) && scalar_finite(r.wz) && scalar_finite(r.div) &&
                       scalar_finite(r.strain) && scalar_finite(r.q) && scalar_finite(r.wmag);
   return finite ? r : none;
}

// the nine entries of G themselves (row a, column b: dv_a / dx_b), for the checks of the fit; false: not valid
inline bool velgrad_gradient(const VelgradSums& s, float g[9])
{
   const float c00 = s.myy * s.mzz - s.myz * s.myz;
   const float c01 = s.mxz * s.myz - s.mxy * s.mzz;
   const float c02 = s.mxy * s.myz - s.mxz * s.myy;
   const float c11 = s.mxx * s.mzz - s.mxz * s.mxz;
   const float c12 = s.mxy * s.mxz - s.mxx * s.myz;
   const float c22 = s.mxx * s.myy - s.mxy * s.mxy;
   const float det = (s.mxx * c00 + s.mxy * c01) + s.mxz * c02;
   const float t = ((s.mxx + s.myy) + s.mzz) * (1.0f / 3.0f);
   for (int e = 0; e < 9; e++) g[e] = 0.0f;
   if (!(s.count >= VELGRAD_MIN_MEMBERS && det > VELGRAD_MIN_DET_RATIO * ((t * t) * t))) return false;
   const float b[9] = {s.bxx, s.bxy, s.bxz, s.byx, s.byy, s.byz, s.bzx, s.bzy, s.bzz};
   const float c[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
   for (int a = 0; a < 3; a++)
      for (int e = 0; e < 3; e++) g[3 * a + e] = ((b[3 * a] * c[e] + b[3 * a + 1] * c[3 + e]) + b[3 * a + 2] * c[6 + e]) / det;
   return true;
}

// ---- checks ---------------------------------------------------------------------------------------------
#define VELGRAD_QUANTITIES 8

// Why a context cannot give velocity gradients, or nullptr: the kernel walks the FULL-mode cell rows of a context
// that holds the whole grid.  full_mode: FULL or FULL_FAST; whole_grid: every plane, never exchanged.
inline const char* velgrad_context_check(bool full_mode, bool whole_grid)
{
   if (!full_mode) return "FULL and FULL_FAST contexts only";
   if (!whole_grid) return "slab contexts (with neighbours, or that have exchanged) have no velocity gradients";
   return nullptr;
}

// sph_hip_get_velocity_gradients copies rows by particle id: sph_hip_download's rule for a context that has had ports
inline const char* velgrad_ids_check(bool ids_changed)
{
   return ids_changed ? "ports have changed the particle set, the ids are no longer 0..n-1 until the next upload: "
                        "use the samplers"
                      : nullptr;
}

inline const char* velgrad_range_check(int first, int n, int have)
{
   if (first < 0 || n < 0 || (long long)first + n > have) return "the range leaves what the context holds";
   return nullptr;
}

// the samplers' group: 0 samples A = (w_x, w_y, w_z, div), 1 samples B' = (strain, Q, |w|, valid)
inline const char* velgrad_group_check(int group) { return group == 0 || group == 1 ? nullptr : "group must be 0 or 1"; }

// the renderer's quantity, carried by sph_hip_tint_params.channel
inline const char* velgrad_quantity_check(int quantity)
{
   return quantity >= 0 && quantity < VELGRAD_QUANTITIES ? nullptr : "quantity must be 0 .. 7";
}

// which of the two arrays holds a quantity, and its component there
inline int velgrad_quantity_group(int quantity) { return quantity >> 2; }
inline int velgrad_quantity_component(int quantity) { return quantity & 3; }

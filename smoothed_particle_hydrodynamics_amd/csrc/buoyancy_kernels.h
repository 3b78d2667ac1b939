// Buoyancy (include/sph_hip.h: buoyancy; the contract and the check: buoyancy_policy.h; the decision:
// launch_policy.h, step_launches_buoyancy): one kernel between a step's acceleration pass and its integrate.
// No existing kernel changes: the integrate of the context, whichever form launch_integrate picks, runs behind it
// from the rows it leaves.
#pragma once

#include "buoyancy_policy.h"
#include "scalar_kernels.h"

static_assert(sizeof(sph_hip_buoyancy) == 44, "sph_hip_buoyancy is ABI: 44 bytes");

// One lane per sorted slot below the live count (k_scalars_stage's bound, which filled Ts for exactly these
// slots earlier in the step): three 16-byte loads, and for a particle the guard lets through two 16-byte stores.
// The setting and the constants arrive by value; no LDS, no atomics.
__global__ void __launch_bounds__(256)
k_buoyancy_apply(const float4* __restrict__ Ts, const int32_t* __restrict__ meta, sph_hip_buoyancy b, float dt,
                 float cfl_limit, float cfl_limit2, float4* __restrict__ acc, float4* __restrict__ velp)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const float4 t = Ts[p];
   float4 a = acc[p];
   float4 v = velp[p];
   const float s = buoyancy_excess(b, scalar4_of(t));
   if (!buoyancy_acts(s)) return;
   buoyancy_apply(b, s, dt, cfl_limit, cfl_limit2, a.x, a.y, a.z, v.x, v.y, v.z);
   acc[p] = a;
   velp[p] = v;
}

// Ports on the device (the contract: port_policy.h): one launch per step, in front of the cell build.
#pragma once

#include "port_policy.h"
#include "sph_device.h"

#define PORT_THREADS 256

// The first `sink_blocks` workgroups cover the entries [0, n_live) the last build left: one 16-byte load of
// the position, the sink list read uniformly (scalar loads, as the obstacle list), a 4-byte store of the dead
// id into the caught entries' id word - the next build (k_hash_count<false, true>) drops them - and the
// per-sink counts by wave ballot and popcount, one 64-bit atomic per wave and sink.  The workgroups behind
// them append the step's m new points at n_live + j; an entry past the capacity raises error bit 4 and is
// not written (the k_slab_unpack guard; the host refuses such a step before it is enqueued).  Thread 0 sets
// the entry count of the build that follows.  The host sizes sink_blocks by its upper bound of n_live.
__global__ void __launch_bounds__(PORT_THREADS)
k_ports_apply(float4* __restrict__ posm, float4* __restrict__ velp, int32_t* __restrict__ meta,
              const sph_hip_sink* __restrict__ sinks, int ns, const sph_hip_emitter* __restrict__ emitters,
              PortFiring f, int sink_blocks, int capacity, unsigned long long* __restrict__ removed)
{
   const int n_live = meta[META_N_LIVE];
   if ((int)blockIdx.x < sink_blocks) {
      const int i = blockIdx.x * PORT_THREADS + threadIdx.x;
      if (i == 0) meta[META_N_IN] = min(n_live + f.m, capacity);
      if (ns == 0) return;
      int hit = -1;
      if (i < n_live) {
         const float4 p = posm[i];
         hit = port_first_sink(sinks, ns, p.x, p.y, p.z);
         if (hit >= 0) reinterpret_cast<uint32_t*>(&velp[i])[3] = SPH_DEAD_ID;
      }
      if (__ballot(hit >= 0) == 0ull) return;
      const int lane = threadIdx.x & (SPH_WAVE - 1);
      for (int s = 0; s < ns; s++) {
         const unsigned long long caught = __ballot(hit == s);
         if (caught != 0ull && lane == 0) atomicAdd(&removed[s], (unsigned long long)__popcll(caught));
      }
      return;
   }
   const int j = ((int)blockIdx.x - sink_blocks) * PORT_THREADS + threadIdx.x;
   if (j >= f.m) return;
   // the firing emitter whose layer holds point j: the last one whose offset is not above j
   // (selects over the whole table, so that it stays in scalar registers)
   int em = f.emitter[0], off = f.offset[0];
   uint32_t id_base = f.id_base[0];
#pragma unroll
   for (int q = 1; q < SPH_HIP_MAX_EMITTERS; q++) {
      const bool here = q < f.n && j >= f.offset[q];
      em = here ? f.emitter[q] : em;
      off = here ? f.offset[q] : off;
      id_base = here ? f.id_base[q] : id_base;
   }
   const int k = j - off;
   const sph_hip_emitter& e = emitters[em];   // (fields loaded as used: a private copy would be staged in LDS)
   const int at = n_live + j;
   if (at >= capacity) {
      atomicOr(&meta[META_ERRORS], 4);
      return;
   }
   float x, y, z;
   port_point(e, k, x, y, z);
   posm[at] = make_float4(x, y, z, e.mass);
   velp[at] = make_float4(e.velocity[0], e.velocity[1], e.velocity[2], __uint_as_float(id_base + (uint32_t)k));
}

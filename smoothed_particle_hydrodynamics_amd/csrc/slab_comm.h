// A slab's side of the neighbour exchange: pack / unpack, the step split around an early
// exchange (step_begin / step_end), and the native RCCL loop that drives them (slab_rccl.h).
// The C entry points (sph_hip.hip) check the context and call these.
#pragma once

#include "launch.h"

// record count of the fuller of a slab's two send messages (their headers' first word)
extern "C" __global__ void k_msg_fill(const SlabMsg* __restrict__ left, const SlabMsg* __restrict__ right,
                           int32_t* __restrict__ out)
{
   const int a = left ? left->header[0] : 0, b = right ? right->header[0] : 0;
   out[0] = a > b ? a : b;
}

namespace {

// ports (port_policy.h) change one context's count between its own steps: a context that holds some cannot be a slab
int refuse_ports(sph_hip_context* ctx)
{
   ctx->err = "a context with ports (sph_hip_set_ports) cannot exchange with neighbouring slabs";
   return SPH_HIP_ERR_INVALID;
}

// free bodies (body_policy.h) are advanced from one context's rows: a context that holds some cannot be a slab
int refuse_bodies(sph_hip_context* ctx)
{
   ctx->err = "a context with bodies (sph_hip_set_bodies) cannot exchange with neighbouring slabs";
   return SPH_HIP_ERR_INVALID;
}

// motion paths (obstacle_policy.h, fourth part) are evaluated in front of launch_integrate only, not in
// front of a slab's early pack: a context that holds some cannot be a slab
int refuse_paths(sph_hip_context* ctx)
{
   ctx->err = "a context with paths (sph_hip_set_obstacle_paths) cannot exchange with neighbouring slabs";
   return SPH_HIP_ERR_INVALID;
}

// a step monitor (monitor_policy.h) reads the whole-grid arrays of one context: a context that records one cannot be a slab
int refuse_monitor(sph_hip_context* ctx)
{
   ctx->err = monitor_exchange_check(ctx->mon_rows);
   return SPH_HIP_ERR_INVALID;
}

int slab_pack(sph_hip_context* ctx, void* left_device, void* right_device,
                      int capacity_records)
{
   int rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || capacity_records < 0) return SPH_HIP_ERR_INVALID;
   if (ctx->n_bodies > 0) return refuse_bodies(ctx);
   if (ctx->n_paths > 0) return refuse_paths(ctx);
   if (ports_active(ctx->n_emit, ctx->n_sink)) return refuse_ports(ctx);
   if (monitor_exchange_check(ctx->mon_rows)) return refuse_monitor(ctx);
   hipStream_t st = ctx->stream;
   ctx->had_exchange = 1;
   if ((rc = drop_prehash(ctx))) return rc;
   ctx->early_exchange = 0;  // this pack sees every particle after the integrate
   ctx->may_hold_dead = 1;   // ... and marks the ones to drop with the dead id
   if (left_device) SPH_TRY(hipMemsetAsync(left_device, 0, sizeof(int32_t) * SLAB_HEADER_INTS, st));
   if (right_device) SPH_TRY(hipMemsetAsync(right_device, 0, sizeof(int32_t) * SLAB_HEADER_INTS, st));
   hipLaunchKernelGGL(k_slab_pack, dim3(div_up(ctx->n, 256)), dim3(256), 0, st, ctx->posm[ctx->cur],
                      ctx->velp[ctx->cur], ctx->meta, ctx->grid, ctx->plane_lo, ctx->plane_hi,
                      ctx->halo, left_device ? 1 : 0, right_device ? 1 : 0,
                      (SlabMsg*)left_device, (SlabMsg*)right_device, capacity_records);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

int slab_unpack(sph_hip_context* ctx, const void* left_device, const void* right_device,
                        int capacity_records)
{
   int rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || capacity_records < 0) return SPH_HIP_ERR_INVALID;
   if (ctx->n_bodies > 0) return refuse_bodies(ctx);
   if (ctx->n_paths > 0) return refuse_paths(ctx);
   if (ports_active(ctx->n_emit, ctx->n_sink)) return refuse_ports(ctx);
   if (monitor_exchange_check(ctx->mon_rows)) return refuse_monitor(ctx);
   ctx->had_exchange = 1;
   // (a slab's fused step has hashed its owned entries for the next build, which hashes what is
   // unpacked here: that stays; a whole-grid prehash knows nothing of new entries)
   if (ctx->prehashed != 2 && (rc = drop_prehash(ctx))) return rc;
   // entries behind the live ones; n_in = n_live + what the messages hold
   hipLaunchKernelGGL(k_slab_unpack, dim3(div_up(2 * capacity_records, 256) + 1), dim3(256), 0,
                      ctx->stream, (const SlabMsg*)left_device, (const SlabMsg*)right_device,
                      ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->meta, ctx->capacity,
                      capacity_records);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

int slab_step_begin(sph_hip_context* ctx, void* left_device, void* right_device,
                            int capacity_records, void* exchange_stream)
{
   int rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || capacity_records < 0) return SPH_HIP_ERR_INVALID;
   if (ctx->n_bodies > 0) return refuse_bodies(ctx);
   if (ctx->n_paths > 0) return refuse_paths(ctx);
   if (ports_active(ctx->n_emit, ctx->n_sink)) return refuse_ports(ctx);
   if (monitor_exchange_check(ctx->mon_rows)) return refuse_monitor(ctx);
   if (!ctx->use_tiled) {
      ctx->err = "sph_hip_slab_step_begin: needs the tiled kernels (SPH_HIP_UNTILED is set)";
      return SPH_HIP_ERR_INVALID;
   }
   if ((left_device != nullptr) != (ctx->plane_lo > 0) ||
       (right_device != nullptr) != (ctx->plane_hi < ctx->grid.nz_global)) {
      ctx->err = "sph_hip_slab_step_begin: one message buffer per existing neighbour, no other";
      return SPH_HIP_ERR_INVALID;
   }
   ctx->had_exchange = 1;
   if (ctx->prehashed != 2 && (rc = drop_prehash(ctx))) return rc;
   hipStream_t st = ctx->stream;
   hipStream_t side = exchange_stream ? (hipStream_t)exchange_stream : st;
   StepEvents se;
   if ((rc = open_step(ctx, true, se))) return rc;
   ctx->slab_step_level = se.level;
   if ((rc = mark_phase(ctx, se, 0, st))) return rc;
   if ((rc = launch_cell_build(ctx, left_device, right_device))) return rc;
   if ((rc = mark_phase(ctx, se, 1, st))) return rc;
   if ((rc = launch_density(ctx))) return rc;
   if ((rc = mark_phase(ctx, se, 3, st))) return rc;
   ctx->early_exchange = 1;
   if (ctx->n == 0) return SPH_HIP_OK;
   // border work on the exchange stream, behind the density pass: it runs next to the interior's
   // acceleration (sph_hip_slab_step_end, main stream) and is short, so the messages leave early
   if (side != st) {
      SPH_TRY(hipEventRecord(ctx->ev_density, st));
      SPH_TRY(hipStreamWaitEvent(side, ctx->ev_density, 0));
   }
   // The two parts of the acceleration launch do the rest of the step themselves (FusedStep):
   // integrate into the other pair of state buffers, hash for the next build, and - the border
   // part - the messages.  SPH_HIP_NO_FUSED_SLAB=1, or static obstacles, keep k_slab_pack_early +
   // k_integrate (their _obst forms); so does a load recording with rows left (k_slab_pack_early
   // records nothing: the border particles are counted once, by k_integrate_loads).
   ctx->slab_fused = fuse_slab_step(ctx->no_fused_slab != 0, ctx->n_obst, loads_pending(ctx)) ? 1 : 0;
   ctx->slab_step_open = 1;
   ctx->slab_msgs[0] = left_device;
   ctx->slab_msgs[1] = right_device;
   ctx->slab_msg_capacity = capacity_records;
   const SlabFused sf = {left_device, right_device, capacity_records};
   if ((rc = launch_accel(ctx, 1, side, ctx->slab_fused, ctx->slab_fused ? &sf : nullptr))) return rc;
   if (!ctx->slab_fused) {
      const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
      const SlabZone zone = slab_zone(ctx);
      // the pack integrates with the motion clock of this step; the integrate of sph_hip_slab_step_end
      // uses the same pair (launch_integrate)
      const bool moving = use_moving_kernels(ctx->n_obst, ctx->n_moving);
      if (moving) {
         motion_tick(ctx, ctx->step_tau);
         ctx->step_tau_taken = 1;
      }
      bind_flags([&](auto U) {
         if (moving)
            hipLaunchKernelGGL(k_slab_pack_early_obst_moving<U.value>, dim3(SLAB_PACK_BLOCKS), dim3(256), 0, side,
                               ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->grid,
                               zone, (SlabMsg*)left_device, (SlabMsg*)right_device, capacity_records,
                               ctx->obst_dev, ctx->n_obst, ctx->motion_dev, ctx->step_tau[0], ctx->step_tau[1]);
         else if (ctx->n_obst > 0)
            hipLaunchKernelGGL(k_slab_pack_early_obst<U.value>, dim3(SLAB_PACK_BLOCKS), dim3(256), 0, side,
                               ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->grid,
                               zone, (SlabMsg*)left_device, (SlabMsg*)right_device, capacity_records,
                               ctx->obst_dev, ctx->n_obst);
         else
            hipLaunchKernelGGL(k_slab_pack_early<U.value>, dim3(SLAB_PACK_BLOCKS), dim3(256), 0, side,
                               ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->grid,
                               zone, (SlabMsg*)left_device, (SlabMsg*)right_device, capacity_records);
      }, unit_scale(ctx->prm));
      SPH_TRY(hipGetLastError());
   }
   if (side != st) SPH_TRY(hipEventRecord(ctx->ev_border, side));
   ctx->border_stream = side;
   return SPH_HIP_OK;
}

int slab_step_end(sph_hip_context* ctx)
{
   int rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || !ctx->early_exchange) {
      ctx->err = "sph_hip_slab_step_end: no sph_hip_slab_step_begin before it";
      return SPH_HIP_ERR_INVALID;
   }
   hipStream_t st = ctx->stream;
   ctx->slab_step_open = 0;
   const StepEvents se = step_events(ctx, ctx->slab_step_level);
   const bool fused = ctx->slab_fused && ctx->n > 0;
   const SlabFused sf = {ctx->slab_msgs[0], ctx->slab_msgs[1], ctx->slab_msg_capacity};
   if ((rc = launch_accel(ctx, 2, st, fused, fused ? &sf : nullptr))) return rc;
   if ((rc = mark_phase(ctx, se, 5, st))) return rc;
   // the integrate needs the border planes' acceleration (and must not move them under the pack);
   // fused, what follows on this stream (unpack, the next build) reads what the border part wrote
   if (ctx->n > 0 && ctx->border_stream != st) SPH_TRY(hipStreamWaitEvent(st, ctx->ev_border, 0));
   if (fused) fused_step_done(ctx, 2);
   else if ((rc = launch_integrate(ctx))) return rc;
   return mark_phase(ctx, se, 6, st);
}

// ---- native RCCL exchange -------------------------------------------------------------------

#define SPH_NCCL_TRY(call)                                                                    \
   do {                                                                                       \
      const ncclResult_t r_ = (call);                                                         \
      if (r_ != ncclSuccess) {                                                                \
         ctx->err = std::string(#call " failed: ") + api->GetErrorString(r_);                 \
         return SPH_HIP_ERR_DEVICE;                                                          \
      }                                                                                       \
   } while (0)

int slab_comm_init(sph_hip_context* ctx, const void* id, int id_bytes, int rank, int nranks,
                           int capacity_records)
{
   if (ctx->mode != SPH_HIP_MODE_FULL || !id || id_bytes < (int)sizeof(ncclUniqueId) || rank < 0 ||
       rank >= nranks || capacity_records < 1) {
      ctx->err = "sph_hip_slab_comm_init: bad arguments";
      return SPH_HIP_ERR_INVALID;
   }
   // slabs are ordered by rank along z: the neighbours of rank r are r - 1 and r + 1
   if ((rank > 0) != (ctx->plane_lo > 0) || (rank + 1 < nranks) != (ctx->plane_hi < ctx->grid.nz_global)) {
      ctx->err = "sph_hip_slab_comm_init: the slab's planes do not match its rank (rank 0 owns "
                 "plane 0, the last rank the last plane)";
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->comm) {
      ctx->err = "sph_hip_slab_comm_init: already initialised";
      return SPH_HIP_ERR_INVALID;
   }
   std::string why;
   const RcclApi* api = rccl_api(&why);
   if (!api) {
      ctx->err = why;
      return SPH_HIP_ERR_DEVICE;
   }
   SPH_TRY(hipSetDevice(ctx->device));
   ctx->comm.reset(new (std::nothrow) SlabComm());   // (a failure below leaves it to sph_hip_destroy)
   SlabComm* c = ctx->comm.get();
   if (!c) return SPH_HIP_ERR_DEVICE;
   c->rank = rank;
   c->nranks = nranks;
   c->capacity_records = c->active_records = capacity_records;
   c->bytes = sph_hip_slab_message_bytes(capacity_records);
   int least = 0, greatest = 0;
   SPH_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
   SPH_TRY(hipStreamCreateWithPriority(c->stream.out(), hipStreamNonBlocking, greatest));
   SPH_TRY(event_create(c->packed));
   SPH_TRY(event_create(c->arrived));
   DevBuf<void>* bufs[4] = {&c->send_left, &c->recv_left, &c->send_right, &c->recv_right};
   for (int b = 0; b < 4; b++) {
      if (b < 2 ? rank == 0 : rank + 1 == nranks) continue;   // no neighbour on that side
      SPH_TRY(hipMalloc(bufs[b]->out(), c->bytes));
      SPH_TRY(hipMemsetAsync(*bufs[b], 0, c->bytes, ctx->stream));
   }
   SPH_TRY(dev_alloc(c->trim_word, 1));
   SPH_TRY(dev_alloc(c->fill_word, 1));
   SPH_TRY(pinned_alloc(c->fill_host, 1));
   c->fill_host[0] = 0;
   SPH_TRY(event_create(c->fill_arrived));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   ncclUniqueId uid;
   memcpy(&uid, id, sizeof(uid));
   SPH_NCCL_TRY(api->CommInitRank(&c->comm, nranks, uid, rank));
   return SPH_HIP_OK;
}

// Trimmed messages (sph_hip_slab_comm_trim) grow before they overflow - an overflow drops records
// and the run is lost.  Called by every rank at the same steps (every SLAB_GROW_EVERY-th of
// sph_hip_slab_comm_run, while active < capacity - the same on every rank): look at the reduced
// fill the PREVIOUS call requested (it waits for that one copy: the exchange it rode behind is
// SLAB_GROW_EVERY steps old), go back to the allocated size when any rank's message was more than
// 4/5 full, and request the next one: max over the two send headers -> ncclAllReduce(max) on the
// exchange stream -> asynchronous copy to pinned memory.  Every rank sees the same number at the
// same step, so all of them switch together and sender and receiver keep agreeing on the size.
int comm_grow_if_needed(sph_hip_context* ctx)
{
   SlabComm* c = ctx->comm.get();
   const RcclApi* api = rccl_api(nullptr);
   if (c->fill_pending) {
      SPH_TRY(hipEventSynchronize(c->fill_arrived));
      c->fill_pending = false;
      const int active = grown_active_records(c->fill_host[0], c->active_records, c->capacity_records);
      if (active != c->active_records) {
         c->active_records = active;
         c->bytes = sph_hip_slab_message_bytes(active);
         c->growths++;
      }
   }
   if (c->active_records >= c->capacity_records || c->nranks < 2) return SPH_HIP_OK;
   // (the headers are read on the context's stream, where this step's cell build will zero them;
   // the reduction rides on the exchange stream, in the same place between two exchanges on every rank)
   hipLaunchKernelGGL(k_msg_fill, dim3(1), dim3(1), 0, ctx->stream, (const SlabMsg*)c->send_left.get(),
                      (const SlabMsg*)c->send_right.get(), c->fill_word);
   SPH_TRY(hipGetLastError());
   SPH_TRY(hipEventRecord(c->packed, ctx->stream));
   SPH_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
   SPH_NCCL_TRY(api->AllReduce(c->fill_word, c->fill_word, 1, ncclInt32, ncclMax, c->comm, c->stream));
   SPH_TRY(hipMemcpyAsync(c->fill_host, c->fill_word, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
   SPH_TRY(hipEventRecord(c->fill_arrived, c->stream));
   c->fill_pending = true;
   return SPH_HIP_OK;
}

// both directions in one group on the exchange stream
int comm_send_recv(sph_hip_context* ctx)
{
   SlabComm* c = ctx->comm.get();
   const RcclApi* api = rccl_api(nullptr);
   if (c->rank == 0 && c->rank + 1 == c->nranks) return SPH_HIP_OK;
   SPH_NCCL_TRY(api->GroupStart());
   if (c->rank > 0) {
      SPH_NCCL_TRY(api->Send(c->send_left, c->bytes, ncclChar, c->rank - 1, c->comm, c->stream));
      SPH_NCCL_TRY(api->Recv(c->recv_left, c->bytes, ncclChar, c->rank - 1, c->comm, c->stream));
   }
   if (c->rank + 1 < c->nranks) {
      SPH_NCCL_TRY(api->Send(c->send_right, c->bytes, ncclChar, c->rank + 1, c->comm, c->stream));
      SPH_NCCL_TRY(api->Recv(c->recv_right, c->bytes, ncclChar, c->rank + 1, c->comm, c->stream));
   }
   SPH_NCCL_TRY(api->GroupEnd());
   return SPH_HIP_OK;
}

int slab_comm_run(sph_hip_context* ctx, int steps)
{
   int rc;
   SlabComm* c = ctx->comm.get();
   if (!c || !c->comm || steps < 0) {
      ctx->err = "sph_hip_slab_comm_run: sph_hip_slab_comm_init first";
      return SPH_HIP_ERR_INVALID;
   }
   hipStream_t st = ctx->stream;
   if (!c->primed) {
      // the first ghosts: pack -> send/recv -> unpack, serially
      if ((rc = slab_pack(ctx, c->send_left, c->send_right, c->active_records))) return rc;
      SPH_TRY(hipEventRecord(c->packed, st));
      SPH_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
      if ((rc = comm_send_recv(ctx))) return rc;
      SPH_TRY(hipEventRecord(c->arrived, c->stream));
      SPH_TRY(hipStreamWaitEvent(st, c->arrived, 0));
      if ((rc = slab_unpack(ctx, c->recv_left, c->recv_right, c->active_records))) return rc;
      c->primed = true;
   }
   for (int s = 0; s < steps; s++) {
      // every 16 steps: ask for the device's error word (asynchronous copy) and look at what the
      // previous request brought - a run that lost particles stops within 32 steps, with no
      // synchronisation anywhere
      // (counted over all calls: a caller that steps one at a time does not wait for a copy per step)
      if (c->steps_run % 16 == 0) {
         if (ctx->watch_pending) SPH_TRY(hipEventSynchronize(ctx->watch_event));
         ctx->watch_pending = 0;
         if ((rc = watch_check(ctx, "sph_hip_slab_comm_run"))) return rc;
         if ((rc = watch_enqueue(ctx))) return rc;
      }
      // (the messages packed by the previous step have been sent: their counts decide about growth)
      if (c->steps_run % SLAB_GROW_EVERY == 0 && (rc = comm_grow_if_needed(ctx))) return rc;
      c->steps_run++;
      // border planes + messages on the exchange stream, transfer behind them; the interior's
      // acceleration and the integrate meanwhile on the context's stream
      if ((rc = slab_step_begin(ctx, c->send_left, c->send_right, c->active_records, c->stream)))
         return rc;
      if ((rc = comm_send_recv(ctx))) return rc;
      SPH_TRY(hipEventRecord(c->arrived, c->stream));
      if ((rc = slab_step_end(ctx))) return rc;
      SPH_TRY(hipStreamWaitEvent(st, c->arrived, 0));
      if ((rc = slab_unpack(ctx, c->recv_left, c->recv_right, c->active_records))) return rc;
   }
   // the word as it stands after the last step travels behind the loop - unless a copy is on its
   // way already (a caller stepping one at a time): the caller's sph_hip_synchronize, or the next
   // call of this function, reports it
   return (steps > 1 || !ctx->watch_pending) ? watch_enqueue(ctx) : SPH_HIP_OK;
}

int slab_comm_trim(sph_hip_context* ctx, float slack, int extra_records, int32_t* active_records)
{
   SlabComm* c = ctx->comm.get();
   if (!c || !c->comm || !(slack >= 1.0f) || extra_records < 0) {
      ctx->err = "sph_hip_slab_comm_trim: sph_hip_slab_comm_init first; slack >= 1, extra >= 0";
      return SPH_HIP_ERR_INVALID;
   }
   const RcclApi* api = rccl_api(nullptr);
   // what this rank packed last (the headers' record counts), with head room
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   SPH_TRY(hipStreamSynchronize(c->stream));
   int32_t most = 0;
   for (void* msg : {c->send_left.get(), c->send_right.get()}) {
      if (!msg) continue;
      int32_t n = 0;
      SPH_TRY(hipMemcpy(&n, msg, sizeof(n), hipMemcpyDeviceToHost));
      most = n > most ? n : most;
   }
   int32_t want = trim_records(most, slack, extra_records, c->capacity_records);
   // every message of the run has one size: the largest wish of any rank
   SPH_TRY(hipMemcpy(c->trim_word, &want, sizeof(want), hipMemcpyHostToDevice));
   SPH_NCCL_TRY(api->AllReduce(c->trim_word, c->trim_word, 1, ncclInt32, ncclMax, c->comm, c->stream));
   SPH_TRY(hipStreamSynchronize(c->stream));
   SPH_TRY(hipMemcpy(&want, c->trim_word, sizeof(want), hipMemcpyDeviceToHost));
   c->active_records = want;
   c->bytes = sph_hip_slab_message_bytes(want);
   c->fill_pending = false;      // (both streams were drained above: a request made for the old size is void)
   if (active_records) *active_records = want;
   return SPH_HIP_OK;
}

int slab_comm_stats(sph_hip_context* ctx, int32_t out[4])
{
   SlabComm* c = ctx->comm.get();
   if (!c || !out) {
      ctx->err = "sph_hip_slab_comm_stats: sph_hip_slab_comm_init first";
      return SPH_HIP_ERR_INVALID;
   }
   out[0] = c->active_records;
   out[1] = c->capacity_records;
   out[2] = c->growths;
   out[3] = (int32_t)(c->steps_run > 0x7fffffffLL ? 0x7fffffffLL : c->steps_run);
   return SPH_HIP_OK;
}

// One checked message to and from each neighbour through the calls, the stream and the group shape
// the exchange uses (before the first step: the message buffers serve as scratch).  Rank r sends
// bytes of value r + 1 and expects r from the left, r + 2 from the right.
int slab_comm_exchange_check(sph_hip_context* ctx)
{
   int rc;
   SlabComm* c = ctx->comm.get();
   if (!c || !c->comm || c->primed) {
      ctx->err = "sph_hip_slab_comm_exchange_check: after sph_hip_slab_comm_init, before the first step";
      return SPH_HIP_ERR_INVALID;
   }
   for (void* q : {c->send_left.get(), c->send_right.get()}) if (q) SPH_TRY(hipMemsetAsync(q, (c->rank + 1) & 0xff, c->bytes, c->stream));
   for (void* q : {c->recv_left.get(), c->recv_right.get()}) if (q) SPH_TRY(hipMemsetAsync(q, 0, c->bytes, c->stream));
   if ((rc = comm_send_recv(ctx))) return rc;
   SPH_TRY(hipStreamSynchronize(c->stream));
   std::string got(c->bytes, '\0');
   bool ok = true;
   for (int side = 0; side < 2; side++) {
      void* q = side == 0 ? c->recv_left.get() : c->recv_right.get();
      if (!q) continue;
      SPH_TRY(hipMemcpy(&got[0], q, c->bytes, hipMemcpyDeviceToHost));
      const char want = (char)((side == 0 ? c->rank : c->rank + 2) & 0xff);
      for (size_t i = 0; i < c->bytes; i++) ok = ok && got[i] == want;
   }
   // leave the buffers as sph_hip_slab_comm_init left them
   for (void* q : {c->send_left.get(), c->send_right.get(), c->recv_left.get(), c->recv_right.get()}) if (q) SPH_TRY(hipMemsetAsync(q, 0, c->bytes, c->stream));
   SPH_TRY(hipStreamSynchronize(c->stream));
   if (!ok) {
      ctx->err = "sph_hip_slab_comm_exchange_check: a neighbour's message arrived with the wrong content";
      return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}

int slab_comm_selftest(sph_hip_context* ctx)
{
   SlabComm* c = ctx->comm.get();
   if (!c || !c->comm) {
      ctx->err = "sph_hip_slab_comm_selftest: sph_hip_slab_comm_init first";
      return SPH_HIP_ERR_INVALID;
   }
   const RcclApi* api = rccl_api(nullptr);
   // a message to oneself through the same calls, stream and group shape the exchange uses
   const size_t n = 1 << 20;
   DevBuf<unsigned char> a, b;
   SPH_TRY(dev_alloc(a, n));
   SPH_TRY(dev_alloc(b, n));
   std::string host(n, '\0'), back(n, '\0');
   for (size_t i = 0; i < n; i++) host[i] = (char)((i * 2654435761u) >> 13);
   SPH_TRY(hipMemcpy(a, host.data(), n, hipMemcpyHostToDevice));
   SPH_TRY(hipMemset(b, 0, n));
   SPH_NCCL_TRY(api->GroupStart());
   SPH_NCCL_TRY(api->Send(a, n, ncclChar, c->rank, c->comm, c->stream));
   SPH_NCCL_TRY(api->Recv(b, n, ncclChar, c->rank, c->comm, c->stream));
   SPH_NCCL_TRY(api->GroupEnd());
   SPH_TRY(hipStreamSynchronize(c->stream));
   SPH_TRY(hipMemcpy(&back[0], b, n, hipMemcpyDeviceToHost));
   if (back != host) {
      ctx->err = "sph_hip_slab_comm_selftest: the message came back different";
      return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}

} // namespace

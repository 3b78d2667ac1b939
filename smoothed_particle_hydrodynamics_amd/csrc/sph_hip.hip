// C ABI of the gfx950 SPH step (include/sph_hip.h): the entry points.  One translation unit, so
// that every kernel is instantiated in one device code object: the context and its resources
// (context.h), the phase launches and the step sequence (launch.h), a slab's exchange
// (slab_comm.h), the launch decisions (launch_policy.h).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see build.py).

#include "slab_comm.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace {

__global__ void k_selftest_sqrt(unsigned long long* __restrict__ out)
{
   // every non-negative finite float: bit patterns 0 .. 0x7f7fffff
   unsigned long long bad = 0;
   uint32_t first = 0xffffffffu, last = 0u;
   const uint32_t stride = gridDim.x * blockDim.x;
   for (uint64_t b = blockIdx.x * blockDim.x + threadIdx.x; b <= 0x7f7fffffull; b += stride) {
      const float x = __uint_as_float((uint32_t)b);
      const float want = sqrtf(x), got = sqrt_rn(x);
      if (__float_as_uint(want) != __float_as_uint(got)) {
         bad++;
         first = min(first, (uint32_t)b);
         last = max(last, (uint32_t)b);
      }
   }
   if (bad) {
      atomicAdd(&out[0], bad);
      atomicMin(&out[1], (unsigned long long)first);
      atomicMax(&out[2], (unsigned long long)last);
   }
}


// ---- field sampler (sample_kernels.h; decisions: sample_policy.h) ---------------------------------

// ctx->err = "who: why"; the call is refused
int refuse(sph_hip_context* ctx, const char* who, const char* why)
{
   ctx->err = std::string(who) + ": " + why;
   return SPH_HIP_ERR_INVALID;
}

// Sampling reads a whole-grid FULL-mode state; a slab holds part of the grid and ghosts besides.
int sample_check(sph_hip_context* ctx, const char* who)
{
   if (ctx->mode != SPH_HIP_MODE_FULL) return refuse(ctx, who, "FULL and FULL_FAST contexts only");
   if (ctx->plane_lo != 0 || ctx->plane_hi != ctx->grid.nz_global || ctx->had_exchange)
      return refuse(ctx, who, "slab contexts (with neighbours, or that have exchanged) cannot be sampled");
   return SPH_HIP_OK;
}

// Bring the cell structure up to date with the current positions: the build sph_hip_voxelize runs,
// which consumes a pending prehash and moves the last sums with the particles, so that nothing a
// caller can read or a later step computes changes.
int sample_prepare(sph_hip_context* ctx) { return launch_cell_build(ctx, nullptr, nullptr, true); }

// A lattice launch's origin, spacing and brick; the chunk it covers is the caller's to fill in.
SampleLattice lattice_of(const float origin[3], const float spacing[3], const SampleBrick& brick)
{
   SampleLattice L = {};
   L.ox = origin[0];
   L.oy = origin[1];
   L.oz = origin[2];
   L.sx = spacing[0];
   L.sy = spacing[1];
   L.sz = spacing[2];
   L.bx = brick.bx;
   L.by = brick.by;
   L.bz = brick.bz;
   return L;
}

// Consecutive arrays of a scratch buffer, each rounded up to 256 bytes (surface_policy.h: surf_scratch,
// render_policy.h: render_scratch_bytes).
struct Carver {
   unsigned char* p;
   template <class T> T* take(long long bytes)
   {
      T* q = reinterpret_cast<T*>(p);
      p += round256(bytes);
      return q;
   }
};

// ---- the samplers' host driver ---------------------------------------------------------------------
// What the calls that sample a field at points or on a lattice share (density and velocity, the
// pressure, the carried scalars): the checks in the order the header promises them, the cell build, the
// chunks that bound the device scratch, the copies out.  A call says what it returns and what it needs;
// its kernel launch for one chunk is a callable.

// one output: the caller's array (null: not wanted) and its bytes per probe
struct SampleOut {
   void* host;
   size_t bytes;
};

struct SampleCall {
   const char* who;                                  // the entry point, for error text
   SampleOut out[3];                                 // in the order of the entry point's arguments
   const char* (*refusal)(const sph_hip_context*);   // a precondition of the call's own: why not, or nullptr
   int (*stage)(sph_hip_context*);                   // what the kernel reads besides the sorted state: launched
                                                     // behind the cell build
};

// The refusals every sampler shares, behind check_ctx and `args` (why the probes or the lattice are
// refused, or nullptr), then the call's own.
int sample_refusals(sph_hip_context* ctx, const SampleCall& c, const char* args)
{
   if (args) return refuse(ctx, c.who, args);
   if (int rc = sample_check(ctx, c.who)) return rc;
   if (c.refusal)
      if (const char* why = c.refusal(ctx)) return refuse(ctx, c.who, why);
   return SPH_HIP_OK;
}

// nothing resident (the cell arrays may still describe an earlier upload): n samples of 0
int sample_zero(const SampleCall& c, size_t n)
{
   for (const SampleOut& o : c.out)
      if (o.host) memset(o.host, 0, o.bytes * n);
   return SPH_HIP_OK;
}

// the cell build, then the call's stage
int sample_ready(sph_hip_context* ctx, const SampleCall& c)
{
   if (int rc = sample_prepare(ctx)) return rc;
   return c.stage ? c.stage(ctx) : SPH_HIP_OK;
}

// A chunk's arrays in ctx->sample_buf: the outputs of 16-byte elements first (their stores are 16 bytes
// wide), then the probes of a point set (3 floats each), then the other outputs in the call's order.
struct SampleScratch {
   float* xyz;
   void* dev[3];
};

int sample_carve(sph_hip_context* ctx, const SampleCall& c, size_t chunk, bool probes, SampleScratch& s)
{
   size_t words = probes ? 3 : 0;
   for (const SampleOut& o : c.out) words += o.bytes / sizeof(float);
   if (int rc = ctx->sample_buf.reserve(ctx, chunk * words)) return rc;
   float* p = ctx->sample_buf;
   auto take = [&](size_t words_each) {
      float* q = p;
      p += chunk * words_each;
      return q;
   };
   for (int i = 0; i < 3; i++)
      if (c.out[i].bytes % 16 == 0) s.dev[i] = take(c.out[i].bytes / sizeof(float));
   s.xyz = probes ? take(3) : nullptr;
   for (int i = 0; i < 3; i++)
      if (c.out[i].bytes % 16 != 0) s.dev[i] = take(c.out[i].bytes / sizeof(float));
   return SPH_HIP_OK;
}

// n probes, at most chunk_limit per chunk; launch(probes on the device, their count, the outputs' arrays)
template <class Launch>
int sample_points_run(sph_hip_context* ctx, const SampleCall& c, int n, const float* xyz, int chunk_limit,
                      Launch launch)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = sample_refusals(ctx, c, n < 0 || (n > 0 && !xyz) ? "negative count or null probe array" : nullptr)))
      return rc;
   if (n == 0) return SPH_HIP_OK;
   if (ctx->n == 0) return sample_zero(c, (size_t)n);
   if ((rc = sample_ready(ctx, c))) return rc;
   const int chunk = sample_points_chunk(n, sample_chunk_limit(chunk_limit, ctx->sample_chunk_forced));
   SampleScratch s;
   if ((rc = sample_carve(ctx, c, (size_t)chunk, true, s))) return rc;
   hipStream_t st = ctx->stream;
   for (int p0 = 0; p0 < n; p0 += chunk) {
      const int m = n - p0 < chunk ? n - p0 : chunk;
      SPH_TRY(hipMemcpyAsync(s.xyz, xyz + 3 * (size_t)p0, sizeof(float) * 3 * m, hipMemcpyHostToDevice, st));
      launch(s.xyz, m, s.dev);
      SPH_TRY(hipGetLastError());
      for (int i = 0; i < 3; i++)
         if (c.out[i].host)
            SPH_TRY(hipMemcpyAsync((char*)c.out[i].host + c.out[i].bytes * (size_t)p0, s.dev[i], c.out[i].bytes * m,
                                   hipMemcpyDeviceToHost, st));
   }
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

// A chunk's outputs are a box of the caller's arrays (elem bytes a point); a chunk that spans whole planes is
// one contiguous piece of them.  Any other chunk is brought over contiguous as well, into `src` on the host,
// and its x-rows are dealt out to their places in the box here.
void sample_deal_box(void* dst, const void* src, size_t elem, const SampleLattice& L, const int32_t dims[3])
{
   char* d = (char*)dst;
   const char* s = (const char*)src;
   const size_t row = (size_t)L.ex * elem;
   for (int z = 0; z < L.ez; z++)
      for (int y = 0; y < L.ey; y++)
         memcpy(d + (((size_t)(L.k0 + z) * dims[1] + L.j0 + y) * dims[0] + L.i0) * elem,
                s + ((size_t)z * L.ey + y) * row, row);
}

// a lattice, in chunks of whole bricks (sample_lattice_chunk); launch(the chunk, its bricks, the outputs' arrays)
template <class Launch>
int sample_lattice_run(sph_hip_context* ctx, const SampleCall& c, const float origin[3], const float spacing[3],
                       const int32_t dims[3], Launch launch)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = sample_refusals(ctx, c, lattice_check(origin, spacing, dims)))) return rc;
   if (ctx->n == 0) return sample_zero(c, (size_t)dims[0] * dims[1] * dims[2]);
   if ((rc = sample_ready(ctx, c))) return rc;
   double cells[3];
   sample_spacing_cells(spacing, ctx->grid.inv, cells);
   const SampleBrick brick = sample_brick(dims, cells);
   const SampleChunk ch =
       sample_lattice_chunk(dims, brick, sample_chunk_limit(SAMPLE_CHUNK_POINTS, ctx->sample_chunk_forced));
   SampleScratch s;
   if ((rc = sample_carve(ctx, c, (size_t)ch.ex * ch.ey * ch.ez, false, s))) return rc;
   hipStream_t st = ctx->stream;
   SampleLattice L = lattice_of(origin, spacing, brick);
   // Chunks of whole planes are copied straight into the caller's arrays, every copy behind its kernel on the
   // stream.  A chunk cut along x or y comes over contiguous too, into a host buffer of this call, and its rows
   // are dealt out here once the stream has drained.  (One strided hipMemcpy2DAsync per z-plane into the
   // caller's arrays stood here; a whole-suite run ended in one of them with "an illegal memory access", as
   // three had in sph_hip_get_loads' strided copies before: DESIGN.md sections 29 and 30.)
   const bool whole_planes = ch.ex == dims[0] && ch.ey == dims[1];
   std::vector<char> stage[3];
   if (!whole_planes) {
      try {
         for (int i = 0; i < 3; i++)
            if (c.out[i].host) stage[i].resize((size_t)ch.ex * ch.ey * ch.ez * c.out[i].bytes);
      } catch (const std::bad_alloc&) {
         ctx->err = std::string(c.who) + ": no host memory for a chunk of the lattice";
         return SPH_HIP_ERR_CAPACITY;
      }
   }
   const size_t plane = (size_t)dims[0] * dims[1];
   for (L.k0 = 0; L.k0 < dims[2]; L.k0 += ch.ez)
      for (L.j0 = 0; L.j0 < dims[1]; L.j0 += ch.ey)
         for (L.i0 = 0; L.i0 < dims[0]; L.i0 += ch.ex) {
            L.ex = dims[0] - L.i0 < ch.ex ? dims[0] - L.i0 : ch.ex;
            L.ey = dims[1] - L.j0 < ch.ey ? dims[1] - L.j0 : ch.ey;
            L.ez = dims[2] - L.k0 < ch.ez ? dims[2] - L.k0 : ch.ez;
            L.bricks_x = div_up(L.ex, L.bx);
            L.bricks_y = div_up(L.ey, L.by);
            launch(L, L.bricks_x * L.bricks_y * div_up(L.ez, L.bz), s.dev);
            SPH_TRY(hipGetLastError());
            const size_t points = (size_t)L.ex * L.ey * L.ez;
            for (int i = 0; i < 3; i++) {
               if (!c.out[i].host) continue;
               void* to = whole_planes ? (char*)c.out[i].host + (size_t)L.k0 * plane * c.out[i].bytes : stage[i].data();
               SPH_TRY(hipMemcpyAsync(to, s.dev[i], points * c.out[i].bytes, hipMemcpyDeviceToHost, st));
            }
            if (whole_planes) continue;
            SPH_TRY(hipStreamSynchronize(st));
            for (int i = 0; i < 3; i++)
               if (c.out[i].host) sample_deal_box(c.out[i].host, stage[i].data(), c.out[i].bytes, L, dims);
         }
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

// the launches of the per-probe kernels (sample_kernels.h), for any accumulator
template <bool UNIT_SCALE, class Sum>
void sample_points_launch(sph_hip_context* ctx, const float* xyz, int m, const typename Sum::Payload* payload,
                          typename Sum::Out out)
{
   hipLaunchKernelGGL((k_sample_points<UNIT_SCALE, Sum>), dim3(div_up(m, 256)), dim3(256), 0, ctx->stream, xyz, m,
                      ctx->posm[ctx->cur], payload, ctx->cell_start, ctx->grid, pair_consts(ctx->prm, ctx->fast != 0), out);
}

template <bool UNIT_SCALE, class Sum>
void sample_lattice_launch(sph_hip_context* ctx, const SampleLattice& L, int bricks, const typename Sum::Payload* payload,
                           typename Sum::Out out)
{
   hipLaunchKernelGGL((k_sample_lattice_walk<UNIT_SCALE, Sum>), dim3(bricks), dim3(SAMPLE_THREADS), 0, ctx->stream, L,
                      ctx->posm[ctx->cur], payload, ctx->cell_start, ctx->grid, pair_consts(ctx->prm, ctx->fast != 0), out);
}


// ---- iso-surface extractor (surface_kernels.h; decisions: surface_policy.h) ------------------------

// Grow a mesh array to hold `need` elements, keeping its first `keep` (the stream is idle).
template <class T>
int surf_grow(sph_hip_context* ctx, DevBuf<T>& buf, long long& cap, long long need, long long keep)
{
   if (need <= cap) return SPH_HIP_OK;
   long long n = cap + cap / 2;
   if (n < need) n = need;
   if (n < 4096) n = 4096;
   DevBuf<T> fresh;
   if (dev_alloc(fresh, (size_t)n) != hipSuccess) {
      (void)hipGetLastError();
      return SPH_HIP_ERR_CAPACITY;
   }
   if (keep > 0) SPH_TRY(hipMemcpy(fresh.get(), buf.get(), sizeof(T) * (size_t)keep, hipMemcpyDeviceToDevice));
   buf = std::move(fresh);
   cap = n;
   return SPH_HIP_OK;
}

} // namespace

extern "C" {

// (a diagnostic build - SPH_ABLATE hooks compiled in, garbage by design - says so here: the
// Python binding refuses it unless SPH_HIP_ALLOW_DIAGNOSTIC=1)
#ifdef SPH_DIAGNOSTIC_BUILD
int sph_hip_abi_version(void) { return SPH_HIP_ABI_VERSION | SPH_HIP_ABI_DIAGNOSTIC; }
#else
int sph_hip_abi_version(void) { return SPH_HIP_ABI_VERSION; }
#endif

#ifdef SPH_TRIPCOUNT
// diagnostic builds with -DSPH_TRIPCOUNT only (tools/trip_counts.py): the loop trip counters of the
// pair kernels (csrc/full_tiled.h: TRIP_*), accumulated since the last reset
extern "C" int sph_hip_diag_trips(unsigned long long* out, int n, int reset)
{
   unsigned long long h[TRIP_COUNT];
   if (hipDeviceSynchronize() != hipSuccess ||
       hipMemcpyFromSymbol(h, HIP_SYMBOL(g_trip), sizeof(h)) != hipSuccess) return SPH_HIP_ERR_DEVICE;
   for (int i = 0; i < n && i < TRIP_COUNT; i++) out[i] = h[i];
   if (reset) {
      memset(h, 0, sizeof(h));
      if (hipMemcpyToSymbol(HIP_SYMBOL(g_trip), h, sizeof(h)) != hipSuccess) return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}
#endif

#ifdef SPH_PHASECLOCK
// diagnostic builds with -DSPH_PHASECLOCK only (tools/phase_clock.py): csrc/full_tiled.h, g_phase
extern "C" int sph_hip_diag_phases(unsigned long long* out, int n, int reset)
{
   // out[0..7] / out[16..23]: sums over the workgroups that wrote (density / acceleration), [7] / [23] their number
   static unsigned int h[2][PHASE_WGS][8];
   if (hipDeviceSynchronize() != hipSuccess ||
       hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)) != hipSuccess) return SPH_HIP_ERR_DEVICE;
   for (int i = 0; i < n && i < 32; i++) out[i] = 0;
   for (int kq = 0; kq < 2; kq++)
      for (int w = 0; w < PHASE_WGS; w++)
         if (h[kq][w][7])
            for (int i = 0; i < 8; i++)
               if (16 * kq + i < n) out[16 * kq + i] += h[kq][w][i];
   if (reset) {
      memset(h, 0, sizeof(h));
      if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h, sizeof(h)) != hipSuccess) return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}
#endif

int sph_hip_selftest_sqrt(int device, uint64_t* mismatches, uint32_t* first_bad)
{
   if (hipSetDevice(device) != hipSuccess) {
      g_create_error = "sph_hip_selftest_sqrt: no such device";
      return SPH_HIP_ERR_NO_DEVICE;
   }
   DevBuf<unsigned long long> d;
   unsigned long long h[3] = {0ull, 0xffffffffull, 0ull};
   if (dev_alloc(d, 3) != hipSuccess ||
       hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) {
      g_create_error = "sph_hip_selftest_sqrt: device memory";
      return SPH_HIP_ERR_DEVICE;
   }
   hipLaunchKernelGGL(k_selftest_sqrt, dim3(256 * 16), dim3(256), 0, 0, d);
   const hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
   if (e != hipSuccess) {
      g_create_error = std::string("sph_hip_selftest_sqrt: ") + hipGetErrorString(e);
      return SPH_HIP_ERR_DEVICE;
   }
   if (mismatches) *mismatches = h[0];
   if (first_bad) *first_bad = (uint32_t)h[1];
   if (getenv("SPH_HIP_DEBUG")) fprintf(stderr, "sph_hip_selftest_sqrt: %llu differ, bits 0x%08llx .. 0x%08llx\n", h[0], h[1], h[2]);
   return SPH_HIP_OK;
}

int sph_hip_params_default(sph_hip_params* p, float h, int cells_x, int cells_y, int cells_z)
{
   if (!p || !(h > 0.0f) || cells_x < 1 || cells_y < 1 || cells_z < 1) return SPH_HIP_ERR_INVALID;
   memset(p, 0, sizeof(*p));
   // reference src/sph.cpp:46-98, same order, same rounding points
   p->sim_scale = 1.0f;
   p->sim_scale_inv = 1.0f / p->sim_scale;
   p->h = h;
   p->h2 = (float)pow((double)h, 2.0);
   p->htimes2 = h * 2.0f;
   p->htimes2inv = 1.0f / p->htimes2;
   p->hscaled = h * p->sim_scale;
   p->hscaled2 = (float)pow((double)(h * p->sim_scale), 2.0);
   p->hscaled6 = (float)pow((double)(h * p->sim_scale), 6.0);
   p->hscaled9 = (float)pow((double)(h * p->sim_scale), 9.0);
   p->cells_x = cells_x;
   p->cells_y = cells_y;
   p->cells_z = cells_z;
   p->cell_size = 2.0f * h;
   p->max_x = p->cell_size * (float)cells_x;
   p->max_y = p->cell_size * (float)cells_y;
   p->max_z = p->cell_size * (float)cells_z;
   p->time_step = 0.001f;
   p->rho0 = 0.1f;
   p->stiffness = 0.001f;
   p->viscosity = 0.01f;
   p->damping = 0.001f;
   p->grav_const = 4.3009e-3f;
   p->central_mass = 1e+5f;
   p->central_pos[0] = p->max_x * 0.5f;
   p->central_pos[1] = p->max_y * 0.5f;
   p->central_pos[2] = p->max_z * 0.5f;
   p->softening = p->hscaled;
   p->cfl_limit = 10000.0f;
   p->cfl_limit2 = p->cfl_limit * p->cfl_limit;
   p->kernel1 = 315.0f / (64.0f * (float)(M_PI)*p->hscaled9);
   p->kernel2 = -45.0f / ((float)(M_PI)*p->hscaled6);
   p->kernel3 = -p->kernel2;
   p->examine_count = 32;
   // FULL grid: cell edge h*(1+1e-4) >= h, covering the same box
   const double edge = (double)h * 1.0001;
   p->full_cell_inv = (float)(1.0 / edge);
   p->full_cells_x = (int)ceil((double)p->max_x / edge);
   p->full_cells_y = (int)ceil((double)p->max_y / edge);
   p->full_cells_z = (int)ceil((double)p->max_z / edge);
   return SPH_HIP_OK;
}

int sph_hip_create(sph_hip_context** out, const sph_hip_params* params, int capacity, int mode,
                   int device)
{
   return create_impl(out, params, capacity, mode, device, 0, -1, 0);
}

int sph_hip_create_slab(sph_hip_context** out, const sph_hip_params* params, int capacity,
                        int device, int plane_lo, int plane_hi)
{
   return create_impl(out, params, capacity, SPH_HIP_MODE_FULL, device, plane_lo, plane_hi,
                      SPH_HIP_SLAB_HALO);
}

void sph_hip_destroy(sph_hip_context* ctx)
{
   if (!ctx) return;
   destroy_impl(ctx);
}

const char* sph_hip_last_error(const sph_hip_context* ctx)
{
   return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int sph_hip_set_stream(sph_hip_context* ctx, void* hip_stream)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
   return SPH_HIP_OK;
}

int sph_hip_set_params(sph_hip_context* ctx, const sph_hip_params* p)
{
   if (!ctx || !p) return SPH_HIP_ERR_INVALID;
   const sph_hip_params& o = ctx->prm;
   if (p->cells_x != o.cells_x || p->cells_y != o.cells_y || p->cells_z != o.cells_z ||
       p->full_cells_x != o.full_cells_x || p->full_cells_y != o.full_cells_y ||
       p->full_cells_z != o.full_cells_z || p->h != o.h || p->htimes2inv != o.htimes2inv ||
       p->full_cell_inv != o.full_cell_inv || p->examine_count != o.examine_count) {
      ctx->err = "sph_hip_set_params: grid shape, h and examine_count are fixed at creation";
      return SPH_HIP_ERR_INVALID;
   }
   ctx->prm = *p;
   return SPH_HIP_OK;
}

int sph_hip_set_arithmetic(sph_hip_context* ctx, int arithmetic)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || (arithmetic != SPH_HIP_ARITH_EXACT && arithmetic != SPH_HIP_ARITH_FAST)) {
      ctx->err = "sph_hip_set_arithmetic: FULL-mode contexts; SPH_HIP_ARITH_EXACT or SPH_HIP_ARITH_FAST";
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->fast == arithmetic) return SPH_HIP_OK;
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   ctx->fast = arithmetic;
   // the capacity levels belong to the kernels that run: worked out again at the next cell build,
   // and what the old kernels' levels reported means nothing for the new ones
   ctx->caps.n_cand = 0;
   return SPH_HIP_OK;
}

int sph_hip_get_arithmetic(const sph_hip_context* ctx) { return ctx ? ctx->fast : SPH_HIP_ERR_INVALID; }

int sph_hip_get_params(const sph_hip_context* ctx, sph_hip_params* out)
{
   if (!ctx || !out) return SPH_HIP_ERR_INVALID;
   *out = ctx->prm;
   return SPH_HIP_OK;
}

// The uniform-mass rule with emitters (port_policy.h: port_mass_rule, which decides): a context whose resident
// particles all have one mass keeps skipping the mass gather only while every emitter's mass equals it in bits.
// nothing_resident: an upload of no particles that nothing has been emitted into - the emitters' own agreement
// decides, and their mass becomes the resident one.  Results are bit-identical either way.
static void ports_mass_rule(sph_hip_context* ctx, bool nothing_resident)
{
   const PortMassRule r = port_mass_rule(ctx->uniform_mass, ctx->upload_mass_known, ctx->upload_mass,
                                         ctx->emit_host, ctx->n_emit, nothing_resident);
   ctx->uniform_mass = r.uniform;
   ctx->upload_mass_known = r.known;
   ctx->upload_mass = r.mass;
}

// the port schedule, the totals and the id bookkeeping start over (sph_hip_set_ports, every upload)
static int ports_restart(sph_hip_context* ctx)
{
   ctx->port_step = 0;
   for (int e = 0; e < SPH_HIP_MAX_EMITTERS; e++) ctx->port_fired[e] = ctx->port_emitted[e] = 0;
   SPH_TRY(hipMemsetAsync(ctx->removed_dev, 0, SPH_HIP_MAX_SINKS * sizeof(unsigned long long), ctx->stream));
   return SPH_HIP_OK;
}

// shared by sph_hip_upload (ids = 0..n-1) and sph_hip_slab_upload (caller's global ids)
static int upload_impl(sph_hip_context* ctx, int n, const float* pos, const float* vel,
                       const float* mass, const uint32_t* ids, int uniform_mass,
                       const void* device_records = nullptr)
{
   if (n < 0 || (n > 0 && !device_records && (!pos || !vel || !mass))) {
      ctx->err = "upload: null array or negative count";
      return SPH_HIP_ERR_INVALID;
   }
   if (n > ctx->capacity) {
      ctx->err = "upload: more particles than the context capacity";
      return SPH_HIP_ERR_CAPACITY;
   }
   int rc_prehash = drop_prehash(ctx);
   if (rc_prehash) return rc_prehash;
   // a slab's entry count changes every step, so its launches are sized by the capacity
   const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global;
   ctx->n = whole ? n : ctx->capacity;
   ctx->n_owned = n;
   ctx->cur = 0;
   ctx->uniform_mass = uniform_mass;
   // ports: the ids start over behind the uploaded ones, the schedule at step 0, with the lists kept
   ctx->next_id = (uint32_t)n;
   if (ids && n > 0) {
      uint32_t most = 0;
      for (int i = 0; i < n; i++) most = ids[i] > most ? ids[i] : most;
      ctx->next_id = most + 1u;
   }
   ctx->ids_changed = 0;
   ctx->n_in_stale = 0;
   // carried scalars belong to the rows of the upload they were set for: dropped with their sources
   ctx->n_scalars = 0;
   ctx->n_scalar_sources = 0;
   ctx->have_buoyancy = 0;   // (buoyancy reads the scalars: it goes with them)
   ctx->have_cohesion = 0;   // cohesion is a setting of the upload it was made for
   ctx->have_xsph = 0;       // and so is the velocity smoothing
   ctx->have_viscous = 0;    // and the viscous stress, with its law
   ctx->have_viscous_law = 0;
   ctx->viscous_sweeps = 0;   // and its solver mode
   ctx->upload_mass_known = (n > 0 && mass) ? 1 : 0;
   ctx->upload_mass = (n > 0 && mass) ? mass[0] : 0.0f;
   ports_mass_rule(ctx, n == 0);
   if (ctx->ports_seen) {
      int rc_ports = ports_restart(ctx);
      if (rc_ports) return rc_ports;
   }
   ctx->ev_steps = 0;
   ctx->err_watch[0] = 0;   // (the upload clears the device's error word below)
   ctx->watch_pending = 0;
   // before the first cell build everything uploaded is live and owned, in upload order
   const int32_t meta[META_COUNT] = {n, n, 0, n, 0, n, 0, 0};
   SPH_TRY(hipMemcpyAsync(ctx->meta, meta, sizeof(meta), hipMemcpyHostToDevice, ctx->stream));
   if (n > 0 && device_records) {
      // the state is on the device already, as message records (sph_hip_slab_export_records)
      hipLaunchKernelGGL(k_import_records, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                         (const float4*)device_records, n, ctx->posm[0], ctx->velp[0]);
      SPH_TRY(hipGetLastError());
   } else if (n > 0) {
      float* spos = ctx->stage;
      float* svel = spos + 3 * (size_t)n;
      float* smass = svel + 3 * (size_t)n;
      uint32_t* sids = reinterpret_cast<uint32_t*>(smass + (size_t)n);
      hipStream_t st = ctx->stream;
      SPH_TRY(hipMemcpyAsync(spos, pos, sizeof(float) * 3 * n, hipMemcpyHostToDevice, st));
      SPH_TRY(hipMemcpyAsync(svel, vel, sizeof(float) * 3 * n, hipMemcpyHostToDevice, st));
      SPH_TRY(hipMemcpyAsync(smass, mass, sizeof(float) * n, hipMemcpyHostToDevice, st));
      if (ids) SPH_TRY(hipMemcpyAsync(sids, ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_import, dim3(div_up(n, 256)), dim3(256), 0, st, spos, svel, smass,
                         ids ? sids : (const uint32_t*)nullptr, n, ctx->posm[0], ctx->velp[0]);
      SPH_TRY(hipGetLastError());
   }
   if (ctx->tile_feedback) {
      // Tile capacity of the first steps: nothing has run yet to report what the scene needs,
      // and the host may enqueue many steps before the first one finishes, so sort the upload
      // once here (the first step's cell build then finds it already in canonical order) and
      // read the largest tile back.
      memset(ctx->tile_feedback, 0, TSTAT_COUNT * sizeof(int));
      if (n > 0 && ctx->use_tiled) {
         int rc = launch_cell_build(ctx);
         if (rc) return rc;
         int stats[TSTAT_COUNT];
         SPH_TRY(hipMemcpyAsync(stats, ctx->tile_stats, sizeof(stats), hipMemcpyDeviceToHost,
                                ctx->stream));
         SPH_TRY(hipStreamSynchronize(ctx->stream));
         memcpy(ctx->tile_feedback, stats, sizeof(stats));
      }
   }
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

static int all_same_mass(int n, const float* mass)
{
   for (int i = 1; i < n; i++)
      if (memcmp(&mass[i], &mass[0], sizeof(float)) != 0) return 0;
   return 1;
}

int sph_hip_upload(sph_hip_context* ctx, int n, const float* pos, const float* vel,
                   const float* mass)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   // the reference gives every particle the same mass (src/sph.cpp:105-108); when the upload
   // does too, the tiled kernels skip the per-neighbour mass gather (bit-identical results)
   return upload_impl(ctx, n, pos, vel, mass, nullptr, (n > 0 && mass) ? all_same_mass(n, mass) : 0);
}

int sph_hip_slab_upload(sph_hip_context* ctx, int n, const float* pos, const float* vel,
                        const float* mass, const uint32_t* ids, int all_masses_equal)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || (n > 0 && !ids)) {
      ctx->err = "sph_hip_slab_upload: FULL-mode contexts only, ids required";
      return SPH_HIP_ERR_INVALID;
   }
   return upload_impl(ctx, n, pos, vel, mass, ids, all_masses_equal ? 1 : 0);
}

// owned count right now (device value); synchronises the stream
static int owned_count(sph_hip_context* ctx, int32_t* meta_out)
{
   int32_t meta[META_COUNT];
   SPH_TRY(hipMemcpyAsync(meta, ctx->meta, sizeof(meta), hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (meta_out) memcpy(meta_out, meta, sizeof(meta));
   ctx->n_owned = meta[META_OWN_END] - meta[META_OWN_BEGIN];
   return SPH_HIP_OK;
}

static int download_impl(sph_hip_context* ctx, int compact, int n, uint32_t* ids, float* pos,
                         float* vel, float* density, float* acc, int32_t* neighbor_count)
{
   if (n == 0) return SPH_HIP_OK;
   float* spos = ctx->stage;
   float* svel = spos + 3 * (size_t)n;
   float* srho = svel + 3 * (size_t)n;
   float* sacc = srho + (size_t)n;
   int32_t* scnt = reinterpret_cast<int32_t*>(sacc + 3 * (size_t)n);
   uint32_t* sids = reinterpret_cast<uint32_t*>(scnt + (size_t)n);
   hipStream_t st = ctx->stream;
   hipLaunchKernelGGL(k_export, dim3(div_up(ctx->n, 256)), dim3(256), 0, st, ctx->posm[ctx->cur],
                      ctx->velp[ctx->cur], ctx->rho, ctx->acc, ctx->ncount, ctx->meta, compact,
                      pos ? spos : nullptr, vel ? svel : nullptr, density ? srho : nullptr,
                      acc ? sacc : nullptr, neighbor_count ? scnt : nullptr, ids ? sids : nullptr);
   SPH_TRY(hipGetLastError());
   if (pos) SPH_TRY(hipMemcpyAsync(pos, spos, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
   if (vel) SPH_TRY(hipMemcpyAsync(vel, svel, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
   if (density) SPH_TRY(hipMemcpyAsync(density, srho, sizeof(float) * n, hipMemcpyDeviceToHost, st));
   if (acc) SPH_TRY(hipMemcpyAsync(acc, sacc, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
   if (neighbor_count)
      SPH_TRY(hipMemcpyAsync(neighbor_count, scnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
   if (ids) SPH_TRY(hipMemcpyAsync(ids, sids, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

int sph_hip_download(sph_hip_context* ctx, float* pos, float* vel, float* density, float* acc,
                     int32_t* neighbor_count)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!(ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global)) {
      ctx->err = "sph_hip_download: slab contexts use sph_hip_slab_download";
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->ids_changed)
      return refuse(ctx, "sph_hip_download", "ports have changed the particle set, the ids are no longer 0..n-1 until "
                                             "the next upload: use sph_hip_download_live");
   return download_impl(ctx, 0, ctx->n_owned, nullptr, pos, vel, density, acc, neighbor_count);
}

int sph_hip_download_live(sph_hip_context* ctx, int max_rows, int32_t* rows, uint32_t* ids, float* pos, float* vel,
                          float* density, float* acc, int32_t* neighbor_count)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || !(ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global))
      return refuse(ctx, "sph_hip_download_live", "FULL and FULL_FAST contexts that hold the whole grid only");
   if (max_rows < 0) return refuse(ctx, "sph_hip_download_live", "negative max_rows");
   // the device's count, and the host bound with it (launch.h: ports_tighten)
   if ((rc = ports_tighten(ctx))) return rc;
   if (rows) *rows = ctx->n_owned;
   if (ctx->n_owned > max_rows) {
      ctx->err = "sph_hip_download_live: caller's arrays are too small";
      return SPH_HIP_ERR_CAPACITY;
   }
   return download_impl(ctx, 1, ctx->n_owned, ids, pos, vel, density, acc, neighbor_count);
}

// ---- asynchronous host mirror ---------------------------------------------------------------

int sph_hip_host_register(void* ptr, size_t bytes)
{
   if (!ptr || bytes == 0) return SPH_HIP_ERR_INVALID;
   const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
   if (e != hipSuccess) {
      (void)hipGetLastError();
      g_create_error = std::string("sph_hip_host_register: ") + hipGetErrorString(e);
      return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}

int sph_hip_host_unregister(void* ptr)
{
   if (!ptr) return SPH_HIP_ERR_INVALID;
   if (hipHostUnregister(ptr) != hipSuccess) {
      (void)hipGetLastError();
      return SPH_HIP_ERR_DEVICE;
   }
   return SPH_HIP_OK;
}

int sph_hip_download_done(sph_hip_context* ctx, int wait)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ctx->mirror_busy) return 1;
   if (wait) {
      SPH_TRY(hipEventSynchronize(ctx->ev_copied));
   } else {
      const hipError_t e = hipEventQuery(ctx->ev_copied);
      if (e == hipErrorNotReady) {
         (void)hipGetLastError();
         return 0;
      }
      SPH_TRY(e);
   }
   ctx->mirror_busy = 0;
   return 1;
}

int sph_hip_download_async(sph_hip_context* ctx, float* pos, float* vel, float* density, float* acc,
                           int32_t* neighbor_count, int32_t* voxel_counts, int* started)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (started) *started = 0;
   if (!(ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global)) {
      ctx->err = "sph_hip_download_async: whole-grid contexts only";
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->ids_changed)
      return refuse(ctx, "sph_hip_download_async", "ports have changed the particle set, the ids are no longer 0..n-1 "
                                                   "until the next upload: use sph_hip_download_live");
   // the previous mirror is still on its way: this request is dropped (a mirror is a picture of
   // the latest state, not a queue) - its staging must not be overwritten under the copy
   rc = sph_hip_download_done(ctx, 0);
   if (rc < 0) return rc;
   if (rc == 0) return SPH_HIP_OK;
   const int n = ctx->n_owned;
   const sph_hip_params& prm = ctx->prm;
   const size_t cells = (size_t)prm.cells_x * prm.cells_y * prm.cells_z;
   if (!ctx->mirror_stage) {
      SPH_TRY(dev_alloc(ctx->mirror_stage, (size_t)ctx->capacity * 11 + cells));
      int least = 0, greatest = 0;
      SPH_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
      SPH_TRY(hipStreamCreateWithPriority(ctx->copy_stream.out(), hipStreamNonBlocking, least));
      SPH_TRY(event_create(ctx->ev_exported));
      SPH_TRY(event_create(ctx->ev_copied));
   }
   float* spos = ctx->mirror_stage;
   float* svel = spos + 3 * (size_t)n;
   float* srho = svel + 3 * (size_t)n;
   float* sacc = srho + (size_t)n;
   int32_t* scnt = reinterpret_cast<int32_t*>(sacc + 3 * (size_t)n);
   int32_t* svox = reinterpret_cast<int32_t*>(ctx->mirror_stage + (size_t)ctx->capacity * 11);
   hipStream_t st = ctx->stream;
   if (n > 0)
      hipLaunchKernelGGL(k_export, dim3(div_up(ctx->n, 256)), dim3(256), 0, st, ctx->posm[ctx->cur],
                         ctx->velp[ctx->cur], ctx->rho, ctx->acc, ctx->ncount, ctx->meta, 0,
                         pos ? spos : nullptr, vel ? svel : nullptr, density ? srho : nullptr,
                         acc ? sacc : nullptr, neighbor_count ? scnt : nullptr, (uint32_t*)nullptr);
   if (voxel_counts) {
      SPH_TRY(hipMemsetAsync(svox, 0, cells * sizeof(int32_t), st));
      if (n > 0)
         hipLaunchKernelGGL(k_voxel_counts, dim3(div_up(ctx->n, 256)), dim3(256), 0, st,
                            ctx->posm[ctx->cur], ctx->meta, prm.htimes2inv, prm.cells_x, prm.cells_y,
                            prm.cells_z, svox);
   }
   SPH_TRY(hipGetLastError());
   // the copies run on their own low-priority stream: the next steps' kernels do not wait for PCIe
   SPH_TRY(hipEventRecord(ctx->ev_exported, st));
   hipStream_t cs = ctx->copy_stream;
   SPH_TRY(hipStreamWaitEvent(cs, ctx->ev_exported, 0));
   if (pos) SPH_TRY(hipMemcpyAsync(pos, spos, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, cs));
   if (vel) SPH_TRY(hipMemcpyAsync(vel, svel, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, cs));
   if (density) SPH_TRY(hipMemcpyAsync(density, srho, sizeof(float) * n, hipMemcpyDeviceToHost, cs));
   if (acc) SPH_TRY(hipMemcpyAsync(acc, sacc, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, cs));
   if (neighbor_count)
      SPH_TRY(hipMemcpyAsync(neighbor_count, scnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, cs));
   if (voxel_counts)
      SPH_TRY(hipMemcpyAsync(voxel_counts, svox, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, cs));
   SPH_TRY(hipEventRecord(ctx->ev_copied, cs));
   ctx->mirror_busy = 1;
   if (started) *started = 1;
   return SPH_HIP_OK;
}

int sph_hip_slab_download(sph_hip_context* ctx, int max_rows, int32_t* rows, uint32_t* ids,
                          float* pos, float* vel, float* density, float* acc,
                          int32_t* neighbor_count)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   int32_t meta[META_COUNT];
   if ((rc = owned_count(ctx, meta))) return rc;
   ctx->err_watch[0] = meta[META_ERRORS];
   if ((rc = watch_check(ctx, "sph_hip_slab_download"))) return rc;
   if (rows) *rows = ctx->n_owned;
   if (ctx->n_owned > max_rows) {
      ctx->err = "sph_hip_slab_download: caller's arrays are too small";
      return SPH_HIP_ERR_CAPACITY;
   }
   return download_impl(ctx, 1, ctx->n_owned, ids, pos, vel, density, acc, neighbor_count);
}

int sph_hip_slab_download_mass(sph_hip_context* ctx, int max_rows, int32_t* rows, float* mass)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = owned_count(ctx, nullptr))) return rc;
   if (rows) *rows = ctx->n_owned;
   if (!mass || ctx->n_owned > max_rows) {
      ctx->err = "sph_hip_slab_download_mass: caller's array is missing or too small";
      return SPH_HIP_ERR_CAPACITY;
   }
   if (ctx->n_owned == 0) return SPH_HIP_OK;
   hipLaunchKernelGGL(k_export_mass, dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream,
                      ctx->posm[ctx->cur], ctx->meta, ctx->stage);
   SPH_TRY(hipGetLastError());
   SPH_TRY(hipMemcpyAsync(mass, ctx->stage, sizeof(float) * ctx->n_owned, hipMemcpyDeviceToHost,
                          ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

int sph_hip_slab_export_records(sph_hip_context* ctx, void* device_records, int max_records, int32_t* rows)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   int32_t meta[META_COUNT];
   if ((rc = owned_count(ctx, meta))) return rc;
   ctx->err_watch[0] = meta[META_ERRORS];
   if ((rc = watch_check(ctx, "sph_hip_slab_export_records"))) return rc;
   if (rows) *rows = ctx->n_owned;
   if (!device_records || ctx->n_owned > max_records) {
      ctx->err = "sph_hip_slab_export_records: caller's buffer is missing or too small";
      return SPH_HIP_ERR_CAPACITY;
   }
   if (ctx->n_owned == 0) return SPH_HIP_OK;
   hipLaunchKernelGGL(k_export_records, dim3(div_up(ctx->n_owned, 256)), dim3(256), 0, ctx->stream,
                      ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->meta, (float4*)device_records);
   SPH_TRY(hipGetLastError());
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

int sph_hip_slab_upload_records(sph_hip_context* ctx, const void* device_records, int n, int all_masses_equal)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_FULL || n < 0 || (n > 0 && !device_records)) {
      ctx->err = "sph_hip_slab_upload_records: FULL-mode contexts only, records required";
      return SPH_HIP_ERR_INVALID;
   }
   return upload_impl(ctx, n, nullptr, nullptr, nullptr, nullptr, all_masses_equal ? 1 : 0, device_records);
}

int sph_hip_slab_status(sph_hip_context* ctx, int32_t* live, int32_t* owned, int32_t* errors)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   int32_t meta[META_COUNT];
   if ((rc = owned_count(ctx, meta))) return rc;
   if (live) *live = meta[META_N_LIVE];
   if (owned) *owned = meta[META_OWN_END] - meta[META_OWN_BEGIN];
   if (errors) *errors = meta[META_ERRORS];
   return SPH_HIP_OK;
}

int sph_hip_slab_poll_errors(sph_hip_context* ctx, int32_t* errors)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->watch_pending) SPH_TRY(hipEventSynchronize(ctx->watch_event));
   ctx->watch_pending = 0;
   if (errors) *errors = ctx->err_watch[0];
   if ((rc = watch_check(ctx, "sph_hip_slab_poll_errors"))) return rc;
   return watch_enqueue(ctx);
}

size_t sph_hip_slab_message_bytes(int capacity_records)
{
   return sizeof(int32_t) * SLAB_HEADER_INTS + (size_t)capacity_records * 2 * sizeof(float4);
}

int sph_hip_slab_pack(sph_hip_context* ctx, void* left_device, void* right_device, int capacity_records)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_pack(ctx, left_device, right_device, capacity_records);
}

int sph_hip_slab_unpack(sph_hip_context* ctx, const void* left_device, const void* right_device,
                        int capacity_records)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_unpack(ctx, left_device, right_device, capacity_records);
}

int sph_hip_slab_step_begin(sph_hip_context* ctx, void* left_device, void* right_device,
                            int capacity_records, void* exchange_stream)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_step_begin(ctx, left_device, right_device, capacity_records, exchange_stream);
}

int sph_hip_slab_step_end(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_step_end(ctx);
}

// ---- native RCCL exchange (slab_comm.h) ------------------------------------------------------

int sph_hip_rccl_unique_id(void* id_out, int id_bytes)
{
   std::string why;
   const RcclApi* api = rccl_api(&why);
   if (!api || !id_out || id_bytes < (int)sizeof(ncclUniqueId)) {
      g_create_error = api ? "sph_hip_rccl_unique_id: buffer too small (128 bytes needed)" : why;
      return SPH_HIP_ERR_INVALID;
   }
   ncclUniqueId id;
   if (api->GetUniqueId(&id) != ncclSuccess) {
      g_create_error = "ncclGetUniqueId failed";
      return SPH_HIP_ERR_DEVICE;
   }
   memcpy(id_out, &id, sizeof(id));
   return SPH_HIP_OK;
}

int sph_hip_slab_comm_init(sph_hip_context* ctx, const void* id, int id_bytes, int rank, int nranks,
                           int capacity_records)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_init(ctx, id, id_bytes, rank, nranks, capacity_records);
}

int sph_hip_slab_comm_run(sph_hip_context* ctx, int steps)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_run(ctx, steps);
}

int sph_hip_slab_comm_trim(sph_hip_context* ctx, float slack, int extra_records, int32_t* active_records)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_trim(ctx, slack, extra_records, active_records);
}

int sph_hip_slab_comm_stats(sph_hip_context* ctx, int32_t out[4])
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_stats(ctx, out);
}

int sph_hip_slab_comm_exchange_check(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_exchange_check(ctx);
}

int sph_hip_slab_comm_selftest(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : slab_comm_selftest(ctx);
}

int sph_hip_particle_count(const sph_hip_context* ctx) { return ctx ? ctx->n_owned : 0; }

int sph_hip_step(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   return step_impl(ctx, true);
}

int sph_hip_run(sph_hip_context* ctx, int steps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   for (int s = 0; s < steps; s++)
      if ((rc = step_impl(ctx, false))) return rc;
   return SPH_HIP_OK;
}

int sph_hip_voxelize(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   // FULL mode keeps the state cell-sorted, so this call moves the particles in device memory:
   // density, acceleration and neighbour counts of the last sums move with them
   return rc ? rc : launch_cell_build(ctx, nullptr, nullptr, true);
}

int sph_hip_find_neighbors(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : launch_find_neighbors(ctx);
}

int sph_hip_compute_density(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : launch_density(ctx);
}

int sph_hip_compute_acceleration(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   return rc ? rc : launch_accel(ctx);
}

int sph_hip_integrate(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   // tracers advance first, in the state the integrate is about to move: the cell structure is brought up to
   // date the way the sampler does it (the build consumes a pending prehash and moves the sums along)
   // and a gauge recording reads the same state behind the same build
   if (ctx->n_tracers > 0 || ctx->grec_rows > 0) {
      if (ctx->n > 0 && (rc = sample_prepare(ctx))) return rc;
      if (ctx->n_tracers > 0 && (rc = launch_tracers(ctx))) return rc;
      if (ctx->grec_rows > 0 && (rc = launch_gauges(ctx))) return rc;
      // the pressure kinds, with densities formed here: whatever the caller's last sph_hip_compute_density left
      // in the context is not trusted
      if (ctx->grec_row_now >= 0 && (rc = launch_gauges_pressure(ctx, gauge_density_source(false)))) return rc;
   }
   if ((rc = drop_prehash(ctx))) return rc;   // the state moves on without a new hash
   return launch_integrate(ctx);
}

// ---- tracers (tracer_kernels.h; contract and decisions: tracer_policy.h) ----------------------------

namespace {
void stop_tracer_recording(sph_hip_context* ctx)
{
   ctx->trec_dev.reset();
   ctx->trec_rows = ctx->trec_filled = 0;
   ctx->trec_every = 1;
   ctx->trec_step = 0;
}
} // namespace

int sph_hip_set_tracers(sph_hip_context* ctx, int n, const float* xyz)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = tracer_check(n, xyz)) return refuse(ctx, "sph_hip_set_tracers", why);
   if ((rc = sample_check(ctx, "sph_hip_set_tracers"))) return rc;
   // the new set's arrays first: a failure keeps the old set
   DevBuf<float4> xi[2];
   DevBuf<int2> cnt[2];
   DevBuf<uint32_t> key, rank, cells, part;
   const bool sorted = tracer_use_sort(n, ctx->tracer_sort_switch);
   std::unique_ptr<float4[]> host;
   if (n > 0) {
      host.reset(new (std::nothrow) float4[(size_t)n]);
      bool ok = host != nullptr;
      for (int b = 0; ok && b < (sorted ? 2 : 1); b++)
         ok = dev_alloc(xi[b], (size_t)n) == hipSuccess && dev_alloc(cnt[b], (size_t)n) == hipSuccess;
      if (ok && sorted)
         ok = dev_alloc(key, (size_t)n) == hipSuccess && dev_alloc(rank, (size_t)n) == hipSuccess &&
              dev_alloc(cells, (size_t)ctx->scan_tiles * SCAN_TILE + 16) == hipSuccess &&
              dev_alloc(part, (size_t)ctx->scan_tiles + 1) == hipSuccess;
      if (!ok) {
         (void)hipGetLastError();
         ctx->err = "sph_hip_set_tracers: cannot allocate " + std::to_string(n) + " tracers";
         return SPH_HIP_ERR_CAPACITY;
      }
      for (int i = 0; i < n; i++) {
         const uint32_t id = (uint32_t)i;
         float w;
         memcpy(&w, &id, sizeof(w));
         host[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], w);
      }
   }
   // steps already queued advance the old set: wait for them before it goes
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (n > 0) {
      SPH_TRY(hipMemcpy(xi[0], host.get(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
      SPH_TRY(hipMemset(cnt[0], 0, sizeof(int2) * (size_t)n));
   }
   for (int b = 0; b < 2; b++) {
      ctx->tr_xi[b] = std::move(xi[b]);
      ctx->tr_cnt[b] = std::move(cnt[b]);
   }
   ctx->tr_key = std::move(key);
   ctx->tr_rank = std::move(rank);
   ctx->tr_cells = std::move(cells);
   ctx->tr_part = std::move(part);
   ctx->n_tracers = n;
   ctx->tr_cur = 0;
   ctx->tr_since_sort = 0;
   stop_tracer_recording(ctx);
   if (sorted && (rc = launch_tracer_sort(ctx))) return rc;
   return SPH_HIP_OK;
}

int sph_hip_tracer_count(const sph_hip_context* ctx) { return ctx ? ctx->n_tracers : SPH_HIP_ERR_INVALID; }

int sph_hip_get_tracers(sph_hip_context* ctx, int first, int n, float* xyz, int32_t* wet_steps, int32_t* dry_steps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = tracer_range_check(first, n, ctx->n_tracers)) return refuse(ctx, "sph_hip_get_tracers", why);
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   const int total = ctx->n_tracers;
   if (n == 0 || total == 0) return SPH_HIP_OK;
   std::unique_ptr<float4[]> x(new (std::nothrow) float4[(size_t)total]);
   std::unique_ptr<int2[]> c(new (std::nothrow) int2[(size_t)total]);
   if (!x || !c) {
      ctx->err = "sph_hip_get_tracers: out of host memory";
      return SPH_HIP_ERR_CAPACITY;
   }
   SPH_TRY(hipMemcpy(x.get(), ctx->tr_xi[ctx->tr_cur], sizeof(float4) * (size_t)total, hipMemcpyDeviceToHost));
   SPH_TRY(hipMemcpy(c.get(), ctx->tr_cnt[ctx->tr_cur], sizeof(int2) * (size_t)total, hipMemcpyDeviceToHost));
   // slots -> the caller's rows: by id
   for (int s = 0; s < total; s++) {
      uint32_t id;
      memcpy(&id, &x[s].w, sizeof(id));
      if (id < (uint32_t)first || id >= (uint32_t)(first + n)) continue;
      const size_t o = (size_t)id - (size_t)first;
      if (xyz) {
         xyz[3 * o + 0] = x[s].x;
         xyz[3 * o + 1] = x[s].y;
         xyz[3 * o + 2] = x[s].z;
      }
      if (wet_steps) wet_steps[o] = c[s].x;
      if (dry_steps) dry_steps[o] = c[s].y;
   }
   return SPH_HIP_OK;
}

int sph_hip_record_tracers(sph_hip_context* ctx, int rows, int every)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = tracer_record_check(rows, every, ctx->n_tracers)) return refuse(ctx, "sph_hip_record_tracers", why);
   DevBuf<float> fresh;
   const size_t words = (size_t)rows * 3 * (size_t)ctx->n_tracers;
   if (words > 0 && dev_alloc(fresh, words) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "sph_hip_record_tracers: cannot allocate " + std::to_string(rows) + " rows";
      return SPH_HIP_ERR_CAPACITY;
   }
   // steps already queued may still be writing the rows this call replaces
   if (ctx->trec_dev) SPH_TRY(hipStreamSynchronize(ctx->stream));
   stop_tracer_recording(ctx);
   if (words > 0) {
      ctx->trec_dev = std::move(fresh);
      ctx->trec_rows = rows;
      ctx->trec_every = every;
   }
   return SPH_HIP_OK;
}

int sph_hip_get_tracer_path(sph_hip_context* ctx, int first_row, int n_rows, float* xyz, int32_t* step_index)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = tracer_range_check(first_row, n_rows, ctx->trec_filled))
      return refuse(ctx, "sph_hip_get_tracer_path", why);
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   const size_t row = 3 * (size_t)ctx->n_tracers;
   if (xyz && n_rows > 0)
      SPH_TRY(hipMemcpy(xyz, ctx->trec_dev.get() + (size_t)first_row * row, sizeof(float) * row * (size_t)n_rows,
                        hipMemcpyDeviceToHost));
   for (int r = 0; step_index && r < n_rows; r++) step_index[r] = tracer_record_step(first_row + r, ctx->trec_every);
   return ctx->trec_filled;
}

// ---- gauges (gauge_kernels.h; contract and decisions: gauge_policy.h) --------------------------------

namespace {
void stop_gauge_recording(sph_hip_context* ctx)
{
   ctx->grec_dev.reset();
   ctx->grec_rows = ctx->grec_filled = 0;
   ctx->grec_every = 1;
   ctx->grec_step = 0;
   ctx->grec_row_now = -1;
}
} // namespace

int sph_hip_set_gauges(sph_hip_context* ctx, const sph_hip_gauge* list, int n)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = sample_check(ctx, "sph_hip_set_gauges"))) return rc;
   if (const char* why = gauge_check(list, n)) return refuse(ctx, "sph_hip_set_gauges", why);
   // the new set's arrays first: a failure keeps the old set
   std::unique_ptr<sph_hip_gauge[]> host;
   DevBuf<sph_hip_gauge> dev;
   DevBuf<sph_hip_gauge_reading> now;
   if (n > 0) {
      host.reset(new (std::nothrow) sph_hip_gauge[(size_t)n]);
      if (!host || dev_alloc(dev, (size_t)n) != hipSuccess || dev_alloc(now, (size_t)n) != hipSuccess) {
         (void)hipGetLastError();
         ctx->err = "sph_hip_set_gauges: cannot allocate " + std::to_string(n) + " gauges";
         return SPH_HIP_ERR_CAPACITY;
      }
      memcpy(host.get(), list, sizeof(sph_hip_gauge) * (size_t)n);
   }
   // steps already queued read the old set: wait for them before it goes
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (n > 0) SPH_TRY(hipMemcpy(dev, host.get(), sizeof(sph_hip_gauge) * (size_t)n, hipMemcpyHostToDevice));
   ctx->gauges_host = std::move(host);
   ctx->gauges_dev = std::move(dev);
   ctx->gauge_now = std::move(now);
   ctx->n_gauges = n;
   int reads[2];
   gauge_set_counts(ctx->gauges_host.get(), n, reads);
   ctx->n_gauges_field = reads[GAUGE_LAUNCH_FIELD];
   ctx->n_gauges_pressure = reads[GAUGE_LAUNCH_PRESSURE];
   stop_gauge_recording(ctx);
   return SPH_HIP_OK;
}

int sph_hip_get_gauges(sph_hip_context* ctx, sph_hip_gauge* out, int capacity)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (capacity < 0 || (capacity > 0 && !out)) return refuse(ctx, "sph_hip_get_gauges", "negative capacity or null array");
   const int m = ctx->n_gauges < capacity ? ctx->n_gauges : capacity;
   if (m > 0) memcpy(out, ctx->gauges_host.get(), sizeof(sph_hip_gauge) * (size_t)m);
   return ctx->n_gauges;
}

int sph_hip_read_gauges(sph_hip_context* ctx, sph_hip_gauge_reading* out)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const int n = ctx->n_gauges;
   if (n == 0) return SPH_HIP_OK;
   if (!out) return refuse(ctx, "sph_hip_read_gauges", "null output array");
   if (ctx->n > 0 && (rc = sample_prepare(ctx))) return rc;
   if ((rc = launch_gauges_into(ctx, ctx->gauge_now))) return rc;
   if ((rc = launch_gauges_pressure_into(ctx, ctx->gauge_now, gauge_density_source(false)))) return rc;
   SPH_TRY(hipMemcpyAsync(out, ctx->gauge_now, sizeof(sph_hip_gauge_reading) * (size_t)n, hipMemcpyDeviceToHost,
                          ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

int sph_hip_record_gauges(sph_hip_context* ctx, int rows, int every)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = gauge_record_check(rows, every, ctx->n_gauges)) return refuse(ctx, "sph_hip_record_gauges", why);
   DevBuf<sph_hip_gauge_reading> fresh;
   const size_t cells = (size_t)rows * (size_t)ctx->n_gauges;
   if (cells > 0 && dev_alloc(fresh, cells) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "sph_hip_record_gauges: cannot allocate " + std::to_string(rows) + " rows";
      return SPH_HIP_ERR_CAPACITY;
   }
   // steps already queued may still be writing the rows this call replaces
   if (ctx->grec_dev) SPH_TRY(hipStreamSynchronize(ctx->stream));
   stop_gauge_recording(ctx);
   if (cells > 0) {
      ctx->grec_dev = std::move(fresh);
      ctx->grec_rows = rows;
      ctx->grec_every = every;
   }
   return SPH_HIP_OK;
}

int sph_hip_get_gauge_record(sph_hip_context* ctx, int first_row, int n_rows, sph_hip_gauge_reading* out,
                             int32_t* steps_done)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = gauge_range_check(first_row, n_rows, ctx->grec_filled))
      return refuse(ctx, "sph_hip_get_gauge_record", why);
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   const size_t row = (size_t)ctx->n_gauges;
   if (out && n_rows > 0)
      SPH_TRY(hipMemcpy(out, ctx->grec_dev.get() + (size_t)first_row * row,
                        sizeof(sph_hip_gauge_reading) * row * (size_t)n_rows, hipMemcpyDeviceToHost));
   for (int r = 0; steps_done && r < n_rows; r++) steps_done[r] = gauge_record_steps_done(first_row + r, ctx->grec_every);
   return ctx->grec_filled;
}

// ---- ports (port_kernels.h; contract: port_policy.h; routes: launch_policy.h ports_active) -----------
int sph_hip_set_ports(sph_hip_context* ctx, const sph_hip_emitter* emitters, int ne, const sph_hip_sink* sinks, int ns)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_ports";
   if (ctx->mode != SPH_HIP_MODE_FULL) return refuse(ctx, who, "FULL and FULL_FAST contexts only");
   if (ctx->plane_lo != 0 || ctx->plane_hi != ctx->grid.nz_global || ctx->had_exchange)
      return refuse(ctx, who, "slab contexts (with neighbours, or that have exchanged) cannot have ports");
   if (const char* why = port_check(emitters, ne, sinks, ns, port_grid(ctx))) return refuse(ctx, who, why);
   if (const char* why = scalar_ports_check(ctx->n_scalars, ne, ns)) return refuse(ctx, who, why);
   if (const char* why = cohesion_ports_check(ctx->have_cohesion != 0, ne, ns)) return refuse(ctx, who, why);
   if (const char* why = xsph_ports_check(ctx->have_xsph != 0, ne, ns)) return refuse(ctx, who, why);
   if (const char* why = viscous_ports_check(ctx->have_viscous != 0, ne, ns)) return refuse(ctx, who, why);
   if (const char* why = viscous_implicit_ports_check(ctx->viscous_sweeps, ne, ns)) return refuse(ctx, who, why);
   if (const char* why = monitor_ports_check(ctx->mon_rows, ne, ns)) return refuse(ctx, who, why);
   // a pending prehash counted for a build whose entries the ports may change first
   if ((rc = drop_prehash(ctx))) return rc;
   // steps already queued keep the lists they were enqueued with: the copies go behind them
   if (ne > 0 && (rc = stage_list(ctx, emitters, ne, ctx->emit_stage, ctx->emit_dev, ctx->ev_emit_copied,
                                  ctx->emit_copy_pending)))
      return rc;
   if (ns > 0 && (rc = stage_list(ctx, sinks, ns, ctx->sink_stage, ctx->sink_dev, ctx->ev_sink_copied,
                                  ctx->sink_copy_pending)))
      return rc;
   if (ne > 0) memcpy(ctx->emit_host, emitters, sizeof(sph_hip_emitter) * (size_t)ne);
   if (ns > 0) memcpy(ctx->sink_host, sinks, sizeof(sph_hip_sink) * (size_t)ns);
   ctx->n_emit = ne;
   ctx->n_sink = ns;
   if (ports_active(ne, ns)) ctx->ports_seen = 1;
   if ((rc = ports_restart(ctx))) return rc;
   ports_mass_rule(ctx, ctx->n == 0 && !ctx->ids_changed);
   return SPH_HIP_OK;
}

int sph_hip_get_ports(sph_hip_context* ctx, sph_hip_emitter* emitters, sph_hip_sink* sinks, int capacity_e,
                      int capacity_s, int64_t* emitted, int64_t* removed, int32_t* live, uint32_t* next_id)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (capacity_e < 0 || capacity_s < 0 || (capacity_e > 0 && !emitters) || (capacity_s > 0 && !sinks))
      return refuse(ctx, "sph_hip_get_ports", "negative capacity or null array");
   int32_t meta[META_COUNT];
   if ((rc = ports_tighten(ctx, meta))) return rc;
   const int me = ctx->n_emit < capacity_e ? ctx->n_emit : capacity_e;
   const int ms = ctx->n_sink < capacity_s ? ctx->n_sink : capacity_s;
   if (me > 0) memcpy(emitters, ctx->emit_host, sizeof(sph_hip_emitter) * (size_t)me);
   if (ms > 0) memcpy(sinks, ctx->sink_host, sizeof(sph_hip_sink) * (size_t)ms);
   if (emitted)
      for (int e = 0; e < SPH_HIP_MAX_EMITTERS; e++) emitted[e] = (int64_t)ctx->port_emitted[e];
   if (removed) {
      static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the removed totals are int64");
      SPH_TRY(hipMemcpy(removed, ctx->removed_dev, SPH_HIP_MAX_SINKS * sizeof(int64_t), hipMemcpyDeviceToHost));
   }
   if (live) *live = meta[META_N_LIVE];
   if (next_id) *next_id = ctx->next_id;
   return ctx->n_emit | (ctx->n_sink << 8);
}

// ---- static obstacles (obstacle_policy.h; routes: launch_policy.h fuse_integrate / fuse_slab_step) ----

namespace {
void clear_bodies(sph_hip_context* ctx)
{
   ctx->n_body_entries = ctx->n_bodies = 0;
   ctx->body_last_row = nullptr;
}

// the device state of every body entry, after everything enqueued so far (synchronises)
int read_body_states(sph_hip_context* ctx, BodyState* out)
{
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (ctx->n_body_entries > 0)
      SPH_TRY(hipMemcpy(out, ctx->body_state_dev, sizeof(BodyState) * (size_t)ctx->n_body_entries, hipMemcpyDeviceToHost));
   return SPH_HIP_OK;
}
} // namespace

int sph_hip_set_obstacles(sph_hip_context* ctx, const sph_hip_obstacle* list, int n)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = obstacle_check(list, n)) {
      ctx->err = std::string("sph_hip_set_obstacles: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->slab_step_open) {
      ctx->err = "sph_hip_set_obstacles: not between sph_hip_slab_step_begin and sph_hip_slab_step_end";
      return SPH_HIP_ERR_INVALID;
   }
   if (n > 0) {
      if ((rc = stage_list(ctx, list, n, ctx->obst_stage, ctx->obst_dev, ctx->ev_obst_copied, ctx->obst_copy_pending)))
         return rc;
      memcpy(ctx->obst_host, list, sizeof(sph_hip_obstacle) * (size_t)n);
   }
   ctx->n_obst = n;   // the steps enqueued from here on take the routes of this count
   ctx->n_motion = ctx->n_moving = 0;   // a new list stands still
   ctx->motion_tau = 0.0f;
   clear_bodies(ctx);                   // ... and is nobody's body
   ctx->n_path_entries = ctx->n_paths = 0;   // ... and follows no path
   return SPH_HIP_OK;
}

int sph_hip_get_obstacles(sph_hip_context* ctx, sph_hip_obstacle* out, int capacity)
{
   if (!ctx) return SPH_HIP_ERR_INVALID;
   if (capacity < 0 || (capacity > 0 && !out)) {
      ctx->err = "sph_hip_get_obstacles: capacity must be >= 0, out non-null when it is > 0";
      return SPH_HIP_ERR_INVALID;
   }
   const int k = capacity < ctx->n_obst ? capacity : ctx->n_obst;
   if (k > 0) memcpy(out, ctx->obst_host, sizeof(sph_hip_obstacle) * (size_t)k);
   return ctx->n_obst;
}

// ---- moving obstacles (obstacle_policy.h; routes: launch_policy.h use_moving_kernels) --------------

int sph_hip_set_obstacle_motion(sph_hip_context* ctx, const sph_hip_obstacle_motion* list, int n)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = obstacle_motion_check(list, n, ctx->n_obst)) {
      ctx->err = std::string("sph_hip_set_obstacle_motion: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (const char* why = body_motion_check(list, n, ctx->bodies_host, ctx->n_body_entries)) {
      ctx->err = std::string("sph_hip_set_obstacle_motion: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (const char* why = path_motion_check(ctx->paths_host, ctx->n_path_entries, list, n))
      return refuse(ctx, "sph_hip_set_obstacle_motion", why);
   if (ctx->slab_step_open) {
      ctx->err = "sph_hip_set_obstacle_motion: not between sph_hip_slab_step_begin and sph_hip_slab_step_end";
      return SPH_HIP_ERR_INVALID;
   }
   if (n > 0) {
      if ((rc = stage_list(ctx, list, n, ctx->motion_stage, ctx->motion_dev, ctx->ev_motion_copied,
                           ctx->motion_copy_pending)))
         return rc;
      memcpy(ctx->motion_host, list, sizeof(sph_hip_obstacle_motion) * (size_t)n);
   }
   ctx->n_motion = n;   // the steps enqueued from here on take the routes of these motions
   ctx->n_moving = obstacles_moving(ctx->motion_host, n);
   ctx->motion_tau = 0.0f;
   return SPH_HIP_OK;
}

int sph_hip_get_obstacle_motion(sph_hip_context* ctx, sph_hip_obstacle_motion* out, int capacity, float* clock)
{
   if (!ctx) return SPH_HIP_ERR_INVALID;
   if (capacity < 0 || (capacity > 0 && !out)) {
      ctx->err = "sph_hip_get_obstacle_motion: capacity must be >= 0, out non-null when it is > 0";
      return SPH_HIP_ERR_INVALID;
   }
   const int k = capacity < ctx->n_motion ? capacity : ctx->n_motion;
   if (k > 0) memcpy(out, ctx->motion_host, sizeof(sph_hip_obstacle_motion) * (size_t)k);
   if (clock) *clock = ctx->motion_tau;
   return ctx->n_motion;
}

namespace {
// The first k obstacles as they stand now: displaced to the motion clock, bodies to where the device
// has moved them (which synchronises; `st`, when given, receives the bodies' device state then).
int obstacles_now(sph_hip_context* ctx, sph_hip_obstacle* out, int k, BodyState* st)
{
   for (int i = 0; i < k; i++)
      out[i] = path_obstacle_at(ctx->obst_host[i], i < ctx->n_path_entries ? &ctx->paths_host[i] : nullptr,
                                ctx->path_keys_host.data(), i < ctx->n_motion ? &ctx->motion_host[i] : nullptr,
                                ctx->motion_tau);
   if (ctx->n_bodies > 0 && k > 0) {   // a body stands where the device has moved it to
      BodyState mine[SPH_HIP_MAX_OBSTACLES];
      if (!st) st = mine;
      int rc = check_ctx(ctx);
      if (rc) return rc;
      if ((rc = read_body_states(ctx, st))) return rc;
      for (int i = 0; i < k; i++)
         if (body_is(ctx->bodies_host[i])) out[i] = obstacle_shifted(ctx->obst_host[i], st[i].D);
   }
   return SPH_HIP_OK;
}
} // namespace

int sph_hip_get_obstacles_now(sph_hip_context* ctx, sph_hip_obstacle* out, int capacity)
{
   if (!ctx) return SPH_HIP_ERR_INVALID;
   if (capacity < 0 || (capacity > 0 && !out)) {
      ctx->err = "sph_hip_get_obstacles_now: capacity must be >= 0, out non-null when it is > 0";
      return SPH_HIP_ERR_INVALID;
   }
   const int k = capacity < ctx->n_obst ? capacity : ctx->n_obst;
   if (int rc = obstacles_now(ctx, out, k, nullptr)) return rc;
   return ctx->n_obst;
}

// ---- motion paths (obstacle_policy.h, fourth part; routes: launch_policy.h use_path_kernels) ---------

int sph_hip_set_obstacle_paths(sph_hip_context* ctx, const sph_hip_motion_path* paths, int n,
                               const sph_hip_motion_key* keys, int n_keys)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_obstacle_paths";
   if (ctx->plane_lo != 0 || ctx->plane_hi != ctx->grid.nz_global || ctx->had_exchange || ctx->comm)
      return refuse(ctx, who, "slab contexts (with neighbours, or that have exchanged) cannot have paths");
   if (const char* why = path_check(paths, n, keys, n_keys, ctx->n_obst)) return refuse(ctx, who, why);
   if (const char* why = path_motion_check(paths, n, ctx->motion_host, ctx->n_motion)) return refuse(ctx, who, why);
   if (const char* why = path_body_check(paths, n, ctx->bodies_host, ctx->n_body_entries)) return refuse(ctx, who, why);
   if (ctx->slab_step_open) return refuse(ctx, who, "not between sph_hip_slab_step_begin and sph_hip_slab_step_end");
   if (n > 0) {
      if (!ctx->path_shift_dev) {   // the first set of this context: the buffers of every later one
         DevBuf<sph_hip_motion_path> pd;
         PinnedBuf<sph_hip_motion_path> ps;
         DevBuf<sph_hip_motion_key> kd;
         PinnedBuf<sph_hip_motion_key> ks;
         DevBuf<PathShift> sd;
         Event ep, ek;
         if (dev_alloc(pd, SPH_HIP_MAX_OBSTACLES) != hipSuccess || pinned_alloc(ps, SPH_HIP_MAX_OBSTACLES) != hipSuccess ||
             dev_alloc(kd, SPH_HIP_MAX_PATH_KEYS) != hipSuccess || pinned_alloc(ks, SPH_HIP_MAX_PATH_KEYS) != hipSuccess ||
             dev_alloc(sd, SPH_HIP_MAX_OBSTACLES) != hipSuccess || event_create(ep) != hipSuccess ||
             event_create(ek) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = std::string(who) + ": cannot allocate the path buffers";
            return SPH_HIP_ERR_CAPACITY;
         }
         ctx->paths_dev = std::move(pd);
         ctx->paths_stage = std::move(ps);
         ctx->path_keys_dev = std::move(kd);
         ctx->path_keys_stage = std::move(ks);
         ctx->ev_paths_copied = std::move(ep);
         ctx->ev_path_keys_copied = std::move(ek);
         ctx->path_shift_dev = std::move(sd);
      }
      // steps already queued keep the lists they were enqueued with: the copies go behind them
      if ((rc = stage_list(ctx, paths, n, ctx->paths_stage, ctx->paths_dev, ctx->ev_paths_copied, ctx->paths_copy_pending)))
         return rc;
      if (n_keys > 0 && (rc = stage_list(ctx, keys, n_keys, ctx->path_keys_stage, ctx->path_keys_dev,
                                         ctx->ev_path_keys_copied, ctx->path_keys_copy_pending)))
         return rc;
      SPH_TRY(hipMemsetAsync(ctx->path_shift_dev, 0, sizeof(PathShift) * SPH_HIP_MAX_OBSTACLES, ctx->stream));
      memcpy(ctx->paths_host, paths, sizeof(sph_hip_motion_path) * (size_t)n);
      ctx->path_keys_host.assign(keys, keys + n_keys);
   } else {
      ctx->path_keys_host.clear();
   }
   ctx->n_path_entries = n;   // the steps enqueued from here on take the routes of these paths
   ctx->n_paths = paths_count(ctx->paths_host, n);
   ctx->motion_tau = 0.0f;
   return SPH_HIP_OK;
}

int sph_hip_get_obstacle_paths(sph_hip_context* ctx, sph_hip_motion_path* paths, int capacity,
                               sph_hip_motion_key* keys, int key_capacity, float* shifts)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (capacity < 0 || key_capacity < 0)
      return refuse(ctx, "sph_hip_get_obstacle_paths", "capacity and key_capacity must be >= 0");
   const int k = capacity < ctx->n_path_entries ? capacity : ctx->n_path_entries;
   const int n_keys = (int)ctx->path_keys_host.size();
   const int kk = key_capacity < n_keys ? key_capacity : n_keys;
   if (paths && k > 0) memcpy(paths, ctx->paths_host, sizeof(sph_hip_motion_path) * (size_t)k);
   if (keys && kk > 0) memcpy(keys, ctx->path_keys_host.data(), sizeof(sph_hip_motion_key) * (size_t)kk);
   if (shifts) {
      PathShift st[SPH_HIP_MAX_OBSTACLES];
      memset(st, 0, sizeof(st));
      if (ctx->n_paths > 0) {
         SPH_TRY(hipStreamSynchronize(ctx->stream));
         SPH_TRY(hipMemcpy(st, ctx->path_shift_dev, sizeof(PathShift) * (size_t)ctx->n_obst, hipMemcpyDeviceToHost));
      }
      for (int i = 0; i < ctx->n_obst; i++)
         for (int c = 0; c < 3; c++) {
            shifts[6 * i + c] = st[i].D0[c];
            shifts[6 * i + 3 + c] = st[i].D1[c];
         }
   }
   return ctx->n_path_entries;
}

// ---- free bodies (body_policy.h; routes: launch_policy.h use_body_kernels) --------------------------

int sph_hip_set_bodies(sph_hip_context* ctx, const sph_hip_body* list, int n, int quantum_log2)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* why = body_check(list, n, ctx->n_obst, ctx->motion_host, ctx->n_motion, quantum_log2);
   const int n_bodies = why ? 0 : bodies_count(list, n);
   if (!why)
      why = recording_refuses_bodies(ctx->loads_rows - ctx->loads_next, ctx->loads_quantum, n_bodies, quantum_log2);
   if (!why && n_bodies > 0 &&
       (ctx->plane_lo != 0 || ctx->plane_hi != ctx->grid.nz_global || ctx->had_exchange || ctx->comm))
      why = "slab contexts (with neighbours, or that have exchanged) cannot hold bodies";
   if (!why) why = path_body_check(ctx->paths_host, ctx->n_path_entries, list, n);
   if (!why && ctx->slab_step_open) why = "not between sph_hip_slab_step_begin and sph_hip_slab_step_end";
   if (why) {
      ctx->err = std::string("sph_hip_set_bodies: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (n > 0) {
      BodyState initial[SPH_HIP_MAX_OBSTACLES];
      for (int i = 0; i < n; i++) initial[i] = body_initial(list[i]);
      if ((rc = stage_list(ctx, list, n, ctx->bodies_stage, ctx->bodies_dev, ctx->ev_bodies_copied,
                           ctx->bodies_copy_pending)))
         return rc;
      if ((rc = stage_list(ctx, initial, n, ctx->body_state_stage, ctx->body_state_dev, ctx->ev_body_state_copied,
                           ctx->body_state_copy_pending)))
         return rc;
      memcpy(ctx->bodies_host, list, sizeof(sph_hip_body) * (size_t)n);
   }
   ctx->n_body_entries = n;   // the steps enqueued from here on take the routes of these bodies
   ctx->n_bodies = n_bodies;
   ctx->body_quantum = quantum_log2;
   ctx->body_last_row = nullptr;   // the first advance takes a zero impulse
   return SPH_HIP_OK;
}

int sph_hip_get_bodies(sph_hip_context* ctx, sph_hip_body* list, sph_hip_body_state* state, int capacity)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (capacity < 0) {
      ctx->err = "sph_hip_get_bodies: capacity must be >= 0";
      return SPH_HIP_ERR_INVALID;
   }
   const int k = capacity < ctx->n_body_entries ? capacity : ctx->n_body_entries;
   BodyState st[SPH_HIP_MAX_OBSTACLES];
   if ((rc = read_body_states(ctx, st))) return rc;
   if (list && k > 0) memcpy(list, ctx->bodies_host, sizeof(sph_hip_body) * (size_t)k);
   for (int i = 0; state && i < k; i++) {
      for (int c = 0; c < 3; c++) {
         state[i].displacement[c] = st[i].D[c];
         state[i].velocity[c] = st[i].V[c];
      }
      state[i].skipped = st[i].skipped;
      state[i].steps = st[i].steps;
   }
   return ctx->n_body_entries;
}

// ---- loads on walls and obstacles (load_policy.h; kernel: k_integrate_loads) ----------------------

int sph_hip_record_loads(sph_hip_context* ctx, int rows, int quantum_log2)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = load_check(rows, quantum_log2)) {
      ctx->err = std::string("sph_hip_record_loads: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (const char* why = body_refuses_recording(ctx->n_bodies, ctx->body_quantum, rows, quantum_log2)) {
      ctx->err = std::string("sph_hip_record_loads: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   if (ctx->slab_step_open) {
      ctx->err = "sph_hip_record_loads: not between sph_hip_slab_step_begin and sph_hip_slab_step_end";
      return SPH_HIP_ERR_INVALID;
   }
   DevBuf<unsigned long long> fresh;
   if (rows > 0) {
      const size_t words = (size_t)rows * LOAD_ROW_WORDS;
      if (dev_alloc(fresh, words) != hipSuccess) {
         (void)hipGetLastError();
         ctx->err = "sph_hip_record_loads: cannot allocate " + std::to_string(rows) + " rows";
         return SPH_HIP_ERR_CAPACITY;
      }
      SPH_TRY(hipMemsetAsync(fresh, 0, words * sizeof(unsigned long long), ctx->stream));
   }
   // the bodies' next advance reads the row the last integrate filled: when that is a row of the recording
   // this call replaces, it moves to the internal row that is free
   if (ctx->n_bodies > 0 && ctx->loads_dev && ctx->body_last_row >= ctx->loads_dev.get() &&
       ctx->body_last_row < ctx->loads_dev.get() + (size_t)ctx->loads_rows * LOAD_ROW_WORDS) {
      ctx->body_flip ^= 1;
      unsigned long long* keep = ctx->body_rows.get() + (size_t)ctx->body_flip * LOAD_ROW_WORDS;
      SPH_TRY(hipMemcpyAsync(keep, ctx->body_last_row, LOAD_ROW_WORDS * sizeof(unsigned long long),
                             hipMemcpyDeviceToDevice, ctx->stream));
      ctx->body_last_row = keep;
   }
   // steps already queued may still be adding to the rows this call replaces
   if (ctx->loads_dev) SPH_TRY(hipStreamSynchronize(ctx->stream));
   ctx->loads_dev = std::move(fresh);
   ctx->loads_rows = rows;
   ctx->loads_next = 0;
   ctx->loads_quantum = quantum_log2;
   return SPH_HIP_OK;
}

int sph_hip_get_loads(sph_hip_context* ctx, int first_row, int n_rows, int64_t* impulse, int64_t* count,
                      int64_t* skipped, int32_t* rows_recorded)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ctx->loads_dev) {
      ctx->err = "sph_hip_get_loads: nothing is being recorded (sph_hip_record_loads)";
      return SPH_HIP_ERR_INVALID;
   }
   if (const char* why = load_range_check(first_row, n_rows, ctx->loads_rows)) {
      ctx->err = std::string("sph_hip_get_loads: ") + why;
      return SPH_HIP_ERR_INVALID;
   }
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (rows_recorded) *rows_recorded = ctx->loads_next;
   if (n_rows == 0) return SPH_HIP_OK;
   // A device row is impulse | count | skipped.  The rows come over whole, in one contiguous copy, and are
   // dealt out to the caller's arrays here.  (Three strided hipMemcpy2D calls into the caller's arrays stood
   // here.  Three times a whole-suite run ended in one of them with "an illegal memory access", each time
   // behind a stream synchronise that had succeeded, a different one of the three each time: DESIGN.md
   // sections 20, 27 and 29.  A strided copy to pageable memory makes the runtime map the caller's pages for
   // the device; a contiguous one goes through the runtime's own staging, as every other download here.)
   const size_t word = sizeof(int64_t), S = SPH_HIP_LOAD_SOLIDS;
   const unsigned long long* first = ctx->loads_dev.get() + (size_t)first_row * LOAD_ROW_WORDS;
   std::vector<unsigned long long> rows;
   try {
      rows.resize((size_t)n_rows * LOAD_ROW_WORDS);
   } catch (const std::bad_alloc&) {
      ctx->err = "sph_hip_get_loads: no host memory for " + std::to_string(n_rows) + " rows";
      return SPH_HIP_ERR_CAPACITY;
   }
   SPH_TRY(hipMemcpy(rows.data(), first, rows.size() * word, hipMemcpyDeviceToHost));
   for (size_t r = 0; r < (size_t)n_rows; r++) {
      const unsigned long long* row = rows.data() + r * LOAD_ROW_WORDS;
      if (impulse) memcpy(impulse + r * 3 * S, row, 3 * S * word);
      if (count) memcpy(count + r * S, row + LOAD_ROW_COUNT, S * word);
      if (skipped) memcpy(skipped + r * S, row + LOAD_ROW_SKIPPED, S * word);
   }
   return SPH_HIP_OK;
}

int sph_hip_synchronize(sph_hip_context* ctx)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (ctx->mode == SPH_HIP_MODE_FULL) {
      // say so here, where every host waits before it reads results: a slab whose exchange lost or
      // duplicated particles, and any context whose cell build found more entries than it has room
      // for (bit 4) or an id twice in one cell (bit 16)
      int32_t bits = 0;
      SPH_TRY(hipMemcpy(&bits, ctx->meta + META_ERRORS, sizeof(bits), hipMemcpyDeviceToHost));
      ctx->err_watch[0] = bits;
      return watch_check(ctx, "sph_hip_synchronize");
   }
   return SPH_HIP_OK;
}

int sph_hip_get_timings(sph_hip_context* ctx, float ms[6])
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ms) return SPH_HIP_ERR_INVALID;
   if (ctx->ev_steps == 0) {
      ctx->err = "sph_hip_get_timings: no sph_hip_step() has run since the last upload/reset";
      return SPH_HIP_ERR_INVALID;
   }
   return read_phases(ctx, ctx->ev[(ctx->ev_steps - 1) % EV_RING], ms);
}

int sph_hip_set_timing(sph_hip_context* ctx, int level)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (level < SPH_HIP_TIMING_OFF || level > SPH_HIP_TIMING_PHASES) {
      ctx->err = "sph_hip_set_timing: level must be SPH_HIP_TIMING_OFF, _SUMS or _PHASES";
      return SPH_HIP_ERR_INVALID;
   }
   SPH_TRY(hipStreamSynchronize(ctx->stream));  // events of the old level are not read any more
   ctx->timing_level = level;
   ctx->ev_steps = 0;
   ctx->timing_seen = 0;
   return SPH_HIP_OK;
}

int sph_hip_set_timing_stride(sph_hip_context* ctx, int every)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (every < 1) {
      ctx->err = "sph_hip_set_timing_stride: every >= 1";
      return SPH_HIP_ERR_INVALID;
   }
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   ctx->timing_stride = every;
   ctx->ev_steps = 0;
   ctx->timing_seen = 0;
   return SPH_HIP_OK;
}

int sph_hip_reset_timings(sph_hip_context* ctx)
{
   if (!ctx) return SPH_HIP_ERR_INVALID;
   ctx->ev_steps = 0;
   return SPH_HIP_OK;
}

int sph_hip_get_phase_totals(sph_hip_context* ctx, double ms[6], int32_t* steps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ms || !steps) return SPH_HIP_ERR_INVALID;
   const long long have = ctx->ev_steps < EV_RING ? ctx->ev_steps : EV_RING;
   for (int k = 0; k < 6; k++) ms[k] = 0.0;
   for (long long s = ctx->ev_steps - have; s < ctx->ev_steps; s++) {
      float one[6];
      if ((rc = read_phases(ctx, ctx->ev[s % EV_RING], one))) return rc;
      for (int k = 0; k < 6; k++) ms[k] += (double)one[k];
   }
   *steps = (int32_t)have;
   return SPH_HIP_OK;
}

int sph_hip_get_energy(sph_hip_context* ctx, float* kinetic, float* potential)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   double e[2] = {0.0, 0.0};
   if (ctx->energy_blocks > 0) {
      // per-workgroup partial sums of the last integrate -> totals, fixed order
      hipLaunchKernelGGL(k_energy_total, dim3(1), dim3(RED_THREADS), 0, ctx->stream,
                         ctx->epart + 2, ctx->energy_blocks, ctx->epart);
      SPH_TRY(hipGetLastError());
   }
   SPH_TRY(hipMemcpyAsync(e, ctx->epart, sizeof(e), hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (kinetic) *kinetic = (float)e[0];
   if (potential) *potential = (float)e[1];
   return SPH_HIP_OK;
}

int sph_hip_get_tile_stats(sph_hip_context* ctx, int32_t out[20])
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!out || !ctx->tile_feedback) return SPH_HIP_ERR_INVALID;
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   for (int i = 0; i < 16; i++) out[i] = ctx->tile_feedback[i];
   out[16] = ctx->caps.cap_density;
   out[17] = ctx->caps.cap_accel;
   out[18] = ctx->caps.wide;
   out[19] = ctx->list_cap;
   return SPH_HIP_OK;
}

int sph_hip_get_neighbor_stats(sph_hip_context* ctx, int32_t* avg, int32_t* mx, int32_t* mn)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = owned_count(ctx, nullptr))) return rc;
   const int n = ctx->n_owned;
   if (n == 0) return SPH_HIP_ERR_INVALID;
   const int32_t init[4] = {0, 0, -1, 34};
   SPH_TRY(hipMemcpyAsync(ctx->stats, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
   int blocks = div_up(n, RED_THREADS);
   if (blocks > 1024) blocks = 1024;
   hipLaunchKernelGGL(k_neighbor_stats, dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                      ctx->ncount, ctx->meta, ctx->stats);
   SPH_TRY(hipGetLastError());
   int32_t out[4];
   SPH_TRY(hipMemcpyAsync(out, ctx->stats, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   const long long sum = ((long long)(uint32_t)out[1] << 32) | (uint32_t)out[0];
   if (avg) *avg = (int32_t)(sum / n);
   if (mx) *mx = out[2];
   if (mn) *mn = out[3];
   return SPH_HIP_OK;
}

int sph_hip_download_voxels(sph_hip_context* ctx, int32_t* coords_xyz, int32_t* ids)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_REF) {
      ctx->err = "sph_hip_download_voxels: REF-mode contexts only";
      return SPH_HIP_ERR_INVALID;
   }
   const int n = ctx->n_owned;
   if (coords_xyz)
      SPH_TRY(hipMemcpyAsync(coords_xyz, ctx->vox, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost,
                             ctx->stream));
   if (ids)
      SPH_TRY(hipMemcpyAsync(ids, ctx->key, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

int sph_hip_download_grid_counts(sph_hip_context* ctx, int32_t* counts)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!counts) return SPH_HIP_ERR_INVALID;
   const int nc = ctx->grid.ncells;
   // counts are kept as the exclusive scan; difference them on the host
   uint32_t* tmp = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)nc + 1));
   if (!tmp) return SPH_HIP_ERR_INVALID;
   hipError_t e = hipMemcpyAsync(tmp, ctx->cell_start, sizeof(uint32_t) * ((size_t)nc + 1),
                                 hipMemcpyDeviceToHost, ctx->stream);
   if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
   if (e != hipSuccess) {
      free(tmp);
      ctx->err = std::string("sph_hip_download_grid_counts: ") + hipGetErrorString(e);
      return SPH_HIP_ERR_DEVICE;
   }
   for (int c = 0; c < nc; c++) counts[c] = (int32_t)(tmp[c + 1] - tmp[c]);
   free(tmp);
   return SPH_HIP_OK;
}

int sph_hip_download_neighbor_lists(sph_hip_context* ctx, uint32_t* neighbors, float* distances)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (ctx->mode != SPH_HIP_MODE_REF) {
      ctx->err = "sph_hip_download_neighbor_lists: REF-mode contexts only (FULL mode stores no lists)";
      return SPH_HIP_ERR_INVALID;
   }
   const size_t m = (size_t)ctx->n_owned * ctx->prm.examine_count;
   if (neighbors)
      SPH_TRY(hipMemcpyAsync(neighbors, ctx->nb, sizeof(uint32_t) * m, hipMemcpyDeviceToHost,
                             ctx->stream));
   if (distances)
      SPH_TRY(hipMemcpyAsync(distances, ctx->nd, sizeof(float) * m, hipMemcpyDeviceToHost,
                             ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   return SPH_HIP_OK;
}

// ---- field sampler --------------------------------------------------------------------------------

int sph_hip_sample_points(sph_hip_context* ctx, int n, const float* xyz, float* density, float* velocity_xyz,
                          int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_points", {{density, 4}, {velocity_xyz, 12}, {count, 4}}, nullptr, nullptr};
   return sample_points_run(ctx, call, n, xyz, SAMPLE_CHUNK_POINTS, [&](const float* sxyz, int m, void* const dev[3]) {
      bind_flags([&](auto U, auto V) {
         sample_points_launch<U.value, SampleSum<V.value>>(ctx, sxyz, m, ctx->velp[ctx->cur],
                                                           {(float*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm), velocity_xyz != nullptr);
   });
}

int sph_hip_sample_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3], const int32_t dims[3],
                           float* density, float* velocity_xyz, int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_lattice", {{density, 4}, {velocity_xyz, 12}, {count, 4}}, nullptr, nullptr};
   const bool vel = velocity_xyz != nullptr;
   return sample_lattice_run(ctx, call, origin, spacing, dims, [&](const SampleLattice& L, int bricks, void* const dev[3]) {
      float* srho = (float*)dev[0];
      float* svel = (float*)dev[1];
      int32_t* scnt = (int32_t*)dev[2];
      // the tiled route (SPH_HIP_SAMPLE_TILED=1: sample_policy.h) is this call's alone
      double cells[3];
      sample_spacing_cells(spacing, ctx->grid.inv, cells);
      if (!sample_use_tiled(SampleBrick{L.bx, L.by, L.bz}, dims, cells, SAMPLE_TILE_CAP, ctx->sample_route)) {
         bind_flags([&](auto U, auto V) {
            sample_lattice_launch<U.value, SampleSum<V.value>>(ctx, L, bricks, ctx->velp[ctx->cur], {srho, svel, scnt});
         }, unit_scale(ctx->prm), vel);
         return;
      }
      if (!ctx->sample_lds_set) {
         // (the attribute belongs to the function on the current device: set once per context)
         for (int m = 0; m < 4; m++)
            bind_flags([&](auto U, auto V) {
               (void)hipFuncSetAttribute((const void*)(k_sample_lattice<U.value, V.value>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         SAMPLE_TILE_CAP * SAMPLE_TILE_BYTES_VELOCITY);
            }, (m & 1) != 0, (m & 2) != 0);
         (void)hipGetLastError();
         ctx->sample_lds_set = 1;
      }
      const size_t lds = (size_t)SAMPLE_TILE_CAP * (vel ? SAMPLE_TILE_BYTES_VELOCITY : SAMPLE_TILE_BYTES_DENSITY);
      bind_flags([&](auto U, auto V) {
         hipLaunchKernelGGL((k_sample_lattice<U.value, V.value>), dim3(bricks), dim3(SAMPLE_THREADS), lds, ctx->stream, L,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->cell_start, ctx->grid,
                            pair_consts(ctx->prm, ctx->fast != 0), SAMPLE_TILE_CAP, srho, svel, scnt);
      }, unit_scale(ctx->prm), vel);
   });
}

// ---- pressure samplers (pressure_kernels.h; contract: gauge_policy.h) ------------------------------
// The sampler's calls with the pressure sums: behind the cell build the densities of the current state
// are formed into the context's own buffer (launch_particle_density), then the probes are walked.

int sph_hip_sample_pressure_points(sph_hip_context* ctx, int n, const float* xyz, float* pressure, float* density,
                                   int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_pressure_points", {{pressure, 4}, {density, 4}, {count, 4}}, nullptr,
                            launch_particle_density};
   return sample_points_run(ctx, call, n, xyz, SAMPLE_CHUNK_POINTS, [&](const float* sxyz, int m, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_points_launch<U.value, PressureSum>(ctx, sxyz, m, ctx->rho_own,
                                                    {(float*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

int sph_hip_sample_pressure_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                    const int32_t dims[3], float* pressure, float* density, int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_pressure_lattice", {{pressure, 4}, {density, 4}, {count, 4}}, nullptr,
                            launch_particle_density};
   return sample_lattice_run(ctx, call, origin, spacing, dims, [&](const SampleLattice& L, int bricks, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_lattice_launch<U.value, PressureSum>(ctx, L, bricks, ctx->rho_own,
                                                     {(float*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

// ---- carried scalars (scalar_kernels.h; contract and checks: scalar_policy.h) -----------------------

int sph_hip_set_scalars(sph_hip_context* ctx, int n, const float* values4, const float* kappa4)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_scalars";
   if ((rc = sample_check(ctx, who))) return rc;
   if (const char* why = scalar_context_check(ports_active(ctx->n_emit, ctx->n_sink), ctx->ids_changed != 0))
      return refuse(ctx, who, why);
   if (const char* why = scalar_set_check(n, values4, kappa4, ctx->n_owned)) return refuse(ctx, who, why);
   // steps already queued advance the old rows: wait for them before they go
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (!values4 || n == 0) {
      ctx->n_scalars = 0;
      ctx->n_scalar_sources = 0;
      ctx->have_buoyancy = 0;
      ctx->have_viscous_law = 0;   // (a viscosity law reads the scalars: it goes with them, its mu stays)
      return SPH_HIP_OK;
   }
   if (!ctx->scalar_T) {
      DevBuf<float4> rows, staged;
      DevBuf<float> volumes;
      if (dev_alloc(rows, (size_t)ctx->capacity) != hipSuccess || dev_alloc(staged, (size_t)ctx->capacity) != hipSuccess ||
          dev_alloc(volumes, (size_t)ctx->capacity) != hipSuccess) {
         (void)hipGetLastError();
         ctx->err = "sph_hip_set_scalars: cannot allocate the scalars of " + std::to_string(ctx->capacity) + " particles";
         return SPH_HIP_ERR_CAPACITY;
      }
      ctx->scalar_T = std::move(rows);
      ctx->scalar_Ts = std::move(staged);
      ctx->scalar_Vs = std::move(volumes);
   }
   SPH_TRY(hipMemcpy(ctx->scalar_T, values4, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++) ctx->scalar_kappa[c] = kappa4[c];
   ctx->n_scalars = n;
   return SPH_HIP_OK;
}

int sph_hip_get_scalars(sph_hip_context* ctx, int first, int n, float* out4)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_get_scalars";
   if (const char* why = scalar_have_check(ctx->n_scalars)) return refuse(ctx, who, why);
   if (const char* why = scalar_range_check(first, n, ctx->n_scalars)) return refuse(ctx, who, why);
   if (n > 0 && !out4) return refuse(ctx, who, "null output array");
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (n > 0)
      SPH_TRY(hipMemcpy(out4, ctx->scalar_T.get() + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
   return SPH_HIP_OK;
}

int sph_hip_set_scalar_sources(sph_hip_context* ctx, const sph_hip_scalar_source* list, int n)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_scalar_sources";
   if (const char* why = scalar_have_check(ctx->n_scalars)) return refuse(ctx, who, why);
   if (const char* why = scalar_source_check(list, n)) return refuse(ctx, who, why);
   // (a pass takes its sources by value: the steps already queued keep theirs)
   for (int q = 0; q < n; q++) ctx->scalar_sources[q] = list[q];
   ctx->n_scalar_sources = n;
   return SPH_HIP_OK;
}

int sph_hip_get_scalar_sources(sph_hip_context* ctx, sph_hip_scalar_source* out, int capacity)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (capacity < 0 || (capacity > 0 && !out))
      return refuse(ctx, "sph_hip_get_scalar_sources", "negative capacity or null array");
   const int m = ctx->n_scalar_sources < capacity ? ctx->n_scalar_sources : capacity;
   for (int q = 0; q < m; q++) out[q] = ctx->scalar_sources[q];
   return ctx->n_scalar_sources;
}

// ---- buoyancy (buoyancy_kernels.h; contract and check: buoyancy_policy.h) -------------------------------

int sph_hip_set_buoyancy(sph_hip_context* ctx, const sph_hip_buoyancy* b)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = buoyancy_set_check(b, ctx->n_scalars)) return refuse(ctx, "sph_hip_set_buoyancy", why);
   // (a step takes the setting by value: the steps already queued keep theirs)
   ctx->have_buoyancy = buoyancy_is_off(b) ? 0 : 1;
   if (ctx->have_buoyancy) ctx->buoyancy = *b;
   return SPH_HIP_OK;
}

int sph_hip_get_buoyancy(sph_hip_context* ctx, sph_hip_buoyancy* out)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ctx->have_buoyancy) return 0;
   if (!out) return refuse(ctx, "sph_hip_get_buoyancy", "null output");
   *out = ctx->buoyancy;
   return 1;
}

// ---- cohesion (cohesion_kernels.h; contract and checks: cohesion_policy.h) -------------------------------

int sph_hip_set_cohesion(sph_hip_context* ctx, float gamma)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_cohesion";
   if (const char* why = cohesion_gamma_check(gamma)) return refuse(ctx, who, why);
   if (!cohesion_is_off(gamma)) {   // (switching it off is never refused)
      const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
      if (const char* why = cohesion_context_check(ctx->mode == SPH_HIP_MODE_FULL, whole)) return refuse(ctx, who, why);
      if (const char* why = cohesion_ports_set_check(ports_active(ctx->n_emit, ctx->n_sink))) return refuse(ctx, who, why);
   }
   // (a step takes gamma by value: the steps already queued keep theirs)
   ctx->have_cohesion = cohesion_is_off(gamma) ? 0 : 1;
   ctx->cohesion_gamma = ctx->have_cohesion ? gamma : 0.0f;
   return SPH_HIP_OK;
}

int sph_hip_get_cohesion(sph_hip_context* ctx, float* gamma)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!gamma) return refuse(ctx, "sph_hip_get_cohesion", "null output");
   *gamma = ctx->have_cohesion ? ctx->cohesion_gamma : 0.0f;
   return SPH_HIP_OK;
}

// ---- step monitor (monitor_kernels.h; contract and checks: monitor_policy.h) ------------------------------

static void stop_monitor_recording(sph_hip_context* ctx)
{
   ctx->mon_dev.reset();
   ctx->mon_part.reset();
   ctx->mon_pair_part.reset();
   ctx->mon_rows = ctx->mon_filled = 0;
   ctx->mon_every = 1;
   ctx->mon_quantum = LOAD_QUANTUM_DEFAULT;
   ctx->mon_step = 0;
   ctx->mon_row_now = -1;
}

int sph_hip_record_monitor(sph_hip_context* ctx, int rows, int every, int quantum_log2)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_record_monitor";
   if (const char* why = monitor_rows_check(rows)) return refuse(ctx, who, why);
   if (const char* why = monitor_every_check(every)) return refuse(ctx, who, why);
   if (const char* why = monitor_quantum_check(quantum_log2)) return refuse(ctx, who, why);
   if (rows > 0) {   // (stopping a recording is never refused)
      const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
      if (const char* why = monitor_mode_check(ctx->mode == SPH_HIP_MODE_FULL)) return refuse(ctx, who, why);
      if (const char* why = monitor_slab_check(whole)) return refuse(ctx, who, why);
      if (const char* why = monitor_ports_set_check(ports_active(ctx->n_emit, ctx->n_sink))) return refuse(ctx, who, why);
   }
   DevBuf<sph_hip_monitor_row> fresh;
   DevBuf<MonitorAcc> part;
   DevBuf<MonitorPairAcc> pair_part;
   const size_t pair_blocks = (size_t)div_up(ctx->capacity > 0 ? ctx->capacity : 1, TILE_THREADS);
   if (rows > 0 && (dev_alloc(fresh, (size_t)rows) != hipSuccess || dev_alloc(part, (size_t)MONITOR_MAX_BLOCKS) != hipSuccess ||
                    dev_alloc(pair_part, pair_blocks) != hipSuccess)) {
      (void)hipGetLastError();
      ctx->err = "sph_hip_record_monitor: cannot allocate " + std::to_string(rows) + " rows";
      return SPH_HIP_ERR_CAPACITY;
   }
   // steps already queued may still be writing the rows this call replaces
   if (ctx->mon_dev) SPH_TRY(hipStreamSynchronize(ctx->stream));
   stop_monitor_recording(ctx);
   if (rows > 0) {
      ctx->mon_dev = std::move(fresh);
      ctx->mon_part = std::move(part);
      ctx->mon_pair_part = std::move(pair_part);
      ctx->mon_rows = rows;
      ctx->mon_every = every;
      ctx->mon_quantum = quantum_log2;
   }
   return SPH_HIP_OK;
}

int sph_hip_get_monitor_record(sph_hip_context* ctx, int first_row, int n_rows, sph_hip_monitor_row* out, int32_t* steps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = monitor_range_check(first_row, n_rows, ctx->mon_filled))
      return refuse(ctx, "sph_hip_get_monitor_record", why);
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   if (out && n_rows > 0)
      SPH_TRY(hipMemcpy(out, ctx->mon_dev.get() + (size_t)first_row, sizeof(sph_hip_monitor_row) * (size_t)n_rows,
                        hipMemcpyDeviceToHost));
   for (int r = 0; steps && r < n_rows; r++) steps[r] = monitor_record_step(first_row + r, ctx->mon_every);
   return ctx->mon_filled;
}

// ---- xsph (xsph_kernels.h; contract and checks: xsph_policy.h) -------------------------------------------

int sph_hip_set_xsph(sph_hip_context* ctx, float eps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_xsph";
   if (const char* why = xsph_eps_check(eps)) return refuse(ctx, who, why);
   if (!xsph_is_off(eps)) {   // (switching it off is never refused)
      const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
      if (const char* why = xsph_context_check(ctx->mode == SPH_HIP_MODE_FULL, whole)) return refuse(ctx, who, why);
      if (const char* why = xsph_ports_set_check(ports_active(ctx->n_emit, ctx->n_sink))) return refuse(ctx, who, why);
      if (!ctx->xsph_R) {   // the staged rows: at the first setting, so a context that never asks keeps its footprint
         DevBuf<float4> rows;
         if (dev_alloc(rows, (size_t)ctx->capacity) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = "sph_hip_set_xsph: cannot allocate the staged rows of " + std::to_string(ctx->capacity) + " particles";
            return SPH_HIP_ERR_CAPACITY;
         }
         ctx->xsph_R = std::move(rows);
      }
   }
   // (a step takes eps by value: the steps already queued keep theirs)
   ctx->have_xsph = xsph_is_off(eps) ? 0 : 1;
   ctx->xsph_eps = ctx->have_xsph ? eps : 0.0f;
   return SPH_HIP_OK;
}

int sph_hip_get_xsph(sph_hip_context* ctx, float* eps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!eps) return refuse(ctx, "sph_hip_get_xsph", "null output");
   *eps = ctx->have_xsph ? ctx->xsph_eps : 0.0f;
   return SPH_HIP_OK;
}

// ---- viscous stress (viscous_kernels.h; contract and checks: viscous_policy.h) ---------------------------------

int sph_hip_set_viscous_stress(sph_hip_context* ctx, float mu, const sph_hip_viscosity_law* law)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_viscous_stress";
   if (const char* why = viscous_mu_finite_check(mu)) return refuse(ctx, who, why);
   if (const char* why = viscous_mu_sign_check(mu)) return refuse(ctx, who, why);
   const bool with_law = law && !viscous_is_off(mu);
   if (!viscous_is_off(mu)) {   // (switching it off is never refused)
      if (law) {
         if (const char* why = viscous_law_channel_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_keys_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_values_finite_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_ascending_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_factors_finite_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_factors_sign_check(*law)) return refuse(ctx, who, why);
         if (const char* why = viscous_law_scalars_check(ctx->n_scalars)) return refuse(ctx, who, why);
      }
      const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
      if (const char* why = viscous_mode_check(ctx->mode == SPH_HIP_MODE_FULL)) return refuse(ctx, who, why);
      if (const char* why = viscous_slab_check(whole)) return refuse(ctx, who, why);
      if (const char* why = viscous_ports_set_check(ports_active(ctx->n_emit, ctx->n_sink))) return refuse(ctx, who, why);
      // the staged rows: at the first setting that needs them, so a context that never asks keeps its footprint
      DevBuf<float4> rows;
      DevBuf<float> mus;
      if ((!ctx->viscous_R && dev_alloc(rows, (size_t)ctx->capacity) != hipSuccess) ||
          (with_law && !ctx->viscous_M && dev_alloc(mus, (size_t)ctx->capacity) != hipSuccess)) {
         (void)hipGetLastError();
         ctx->err = "sph_hip_set_viscous_stress: cannot allocate the staged rows of " + std::to_string(ctx->capacity) +
                    " particles";
         return SPH_HIP_ERR_CAPACITY;
      }
      if (!ctx->viscous_R) ctx->viscous_R = std::move(rows);
      if (with_law && !ctx->viscous_M) ctx->viscous_M = std::move(mus);
   }
   // (a step takes mu and the law by value: the steps already queued keep theirs)
   ctx->have_viscous = viscous_is_off(mu) ? 0 : 1;
   ctx->viscous_mu = ctx->have_viscous ? mu : 0.0f;
   ctx->have_viscous_law = with_law ? 1 : 0;
   ctx->viscous_law = viscous_law_clean(with_law ? law : nullptr);
   return SPH_HIP_OK;
}

// The solver mode of the setting above (viscous_implicit_kernels.h; contract and checks: viscous_implicit_policy.h).
// It stands in front of the getter because it allocates the second row set of the sweeps' ping-pong.
int sph_hip_set_viscous_implicit(sph_hip_context* ctx, int sweeps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_set_viscous_implicit";
   if (const char* why = viscous_implicit_sweeps_check(sweeps)) return refuse(ctx, who, why);
   if (!viscous_implicit_is_off(sweeps)) {   // (switching to the explicit term is never refused)
      const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
      if (const char* why = viscous_implicit_mode_check(ctx->mode == SPH_HIP_MODE_FULL)) return refuse(ctx, who, why);
      if (const char* why = viscous_implicit_slab_check(whole)) return refuse(ctx, who, why);
      if (const char* why = viscous_implicit_ports_set_check(ports_active(ctx->n_emit, ctx->n_sink)))
         return refuse(ctx, who, why);
      // the second row set: at the first count that needs it, so a context that never asks keeps its footprint
      if (viscous_implicit_needs_second(sweeps) && !ctx->viscous_R2) {
         DevBuf<float4> second;
         if (dev_alloc(second, (size_t)ctx->capacity) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = "sph_hip_set_viscous_implicit: cannot allocate the second row set of " +
                       std::to_string(ctx->capacity) + " particles";
            return SPH_HIP_ERR_CAPACITY;
         }
         ctx->viscous_R2 = std::move(second);
      }
   }
   // (a step takes the count by value: the steps already queued keep theirs)
   ctx->viscous_sweeps = sweeps;
   return SPH_HIP_OK;
}

int sph_hip_get_viscous_implicit(sph_hip_context* ctx, int* sweeps)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!sweeps) return refuse(ctx, "sph_hip_get_viscous_implicit", "null output");
   *sweeps = ctx->viscous_sweeps;
   return SPH_HIP_OK;
}

int sph_hip_get_viscous_stress(sph_hip_context* ctx, float* mu, sph_hip_viscosity_law* law, int* have_law)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const bool with_law = ctx->have_viscous && ctx->have_viscous_law;
   if (mu) *mu = ctx->have_viscous ? ctx->viscous_mu : 0.0f;
   if (law) *law = viscous_law_clean(with_law ? &ctx->viscous_law : nullptr);
   if (have_law) *have_law = with_law ? 1 : 0;
   return SPH_HIP_OK;
}

// The sampler's calls with the channel sums: behind the cell build the scalars are staged by sorted slot
// (launch_scalars_stage, channels only), then the probes are walked.

static const char* scalars_refusal(const sph_hip_context* ctx) { return scalar_have_check(ctx->n_scalars); }
static int scalars_stage_channels(sph_hip_context* ctx) { return launch_scalars_stage(ctx, false); }

int sph_hip_sample_scalars_points(sph_hip_context* ctx, int n, const float* xyz, float* channels4, float* density,
                                  int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_scalars_points", {{channels4, 16}, {density, 4}, {count, 4}}, scalars_refusal,
                            scalars_stage_channels};
   // (36 bytes a probe against the sampler's 32: half its chunk keeps the scratch inside the 64 MiB budget)
   return sample_points_run(ctx, call, n, xyz, SAMPLE_CHUNK_POINTS / 2, [&](const float* sxyz, int m, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_points_launch<U.value, ScalarSum>(ctx, sxyz, m, ctx->scalar_Ts,
                                                  {(float4*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

int sph_hip_sample_scalars_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                   const int32_t dims[3], float* channels4, float* density, int32_t* count)
{
   const SampleCall call = {"sph_hip_sample_scalars_lattice", {{channels4, 16}, {density, 4}, {count, 4}}, scalars_refusal,
                            scalars_stage_channels};
   return sample_lattice_run(ctx, call, origin, spacing, dims, [&](const SampleLattice& L, int bricks, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_lattice_launch<U.value, ScalarSum>(ctx, L, bricks, ctx->scalar_Ts,
                                                   {(float4*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

// ---- velocity gradients (velgrad_kernels.h; contract and checks: velgrad_policy.h) -------------------------

static const char* velgrad_refusal(const sph_hip_context* ctx)
{
   const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global && !ctx->had_exchange;
   return velgrad_context_check(ctx->mode == SPH_HIP_MODE_FULL, whole);
}

int sph_hip_get_velocity_gradients(sph_hip_context* ctx, int first, int n, float* rotation4, float* invariants4)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_get_velocity_gradients";
   if (const char* why = velgrad_refusal(ctx)) return refuse(ctx, who, why);
   if (const char* why = velgrad_ids_check(ctx->ids_changed != 0)) return refuse(ctx, who, why);
   if (const char* why = velgrad_range_check(first, n, ctx->n_owned)) return refuse(ctx, who, why);
   if (n == 0 || ctx->n == 0) {
      SPH_TRY(hipStreamSynchronize(ctx->stream));
      return SPH_HIP_OK;
   }
   if ((rc = sample_prepare(ctx))) return rc;
   if ((rc = launch_velgrad(ctx))) return rc;
   // both rows into id order, in the staging buffer (idle outside a step: 12 floats a particle, 8 used here); an id
   // no sorted slot holds keeps zeros
   const int rows = ctx->n_owned;
   float4* outA = reinterpret_cast<float4*>(ctx->stage.get());
   float4* outB = outA + (size_t)rows;
   hipStream_t st = ctx->stream;
   SPH_TRY(hipMemsetAsync(outA, 0, sizeof(float4) * 2 * (size_t)rows, st));
   hipLaunchKernelGGL(k_velgrad_unsort, dim3(div_up(ctx->n, 256)), dim3(256), 0, st, ctx->velp[ctx->cur], ctx->meta,
                      ctx->velgrad_A.get(), ctx->velgrad_B.get(), rows, outA, outB);
   SPH_TRY(hipGetLastError());
   if (rotation4)
      SPH_TRY(hipMemcpyAsync(rotation4, outA + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
   if (invariants4)
      SPH_TRY(hipMemcpyAsync(invariants4, outB + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

// The sampler's calls with the rows as the payload of the channel sums: behind the cell build the rows are formed
// (launch_velgrad), then the probes are walked.  (36 bytes a probe, as the scalars' calls.)

int sph_hip_sample_velocity_gradients_points(sph_hip_context* ctx, int n, const float* xyz, int group, float* channels4,
                                             float* density, int32_t* count)
{
   const char* who = "sph_hip_sample_velocity_gradients_points";
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = velgrad_group_check(group)) return refuse(ctx, who, why);
   const SampleCall call = {who, {{channels4, 16}, {density, 4}, {count, 4}}, velgrad_refusal, launch_velgrad};
   return sample_points_run(ctx, call, n, xyz, SAMPLE_CHUNK_POINTS / 2, [&](const float* sxyz, int m, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_points_launch<U.value, ScalarSum>(ctx, sxyz, m, group == 0 ? ctx->velgrad_A.get() : ctx->velgrad_B.get(),
                                                  {(float4*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

int sph_hip_sample_velocity_gradients_lattice(sph_hip_context* ctx, const float origin[3], const float spacing[3],
                                              const int32_t dims[3], int group, float* channels4, float* density,
                                              int32_t* count)
{
   const char* who = "sph_hip_sample_velocity_gradients_lattice";
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (const char* why = velgrad_group_check(group)) return refuse(ctx, who, why);
   const SampleCall call = {who, {{channels4, 16}, {density, 4}, {count, 4}}, velgrad_refusal, launch_velgrad};
   return sample_lattice_run(ctx, call, origin, spacing, dims, [&](const SampleLattice& L, int bricks, void* const dev[3]) {
      bind_flags([&](auto U) {
         sample_lattice_launch<U.value, ScalarSum>(ctx, L, bricks, group == 0 ? ctx->velgrad_A.get() : ctx->velgrad_B.get(),
                                                   {(float4*)dev[0], (float*)dev[1], (int32_t*)dev[2]});
      }, unit_scale(ctx->prm));
   });
}

// ---- iso-surface extractor ------------------------------------------------------------------------

int sph_hip_extract_surface(sph_hip_context* ctx, const float origin[3], const float spacing[3], const int32_t dims[3],
                            float iso, int flags, int32_t counts[2])
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   // the old mesh goes first: a refused or failed extraction keeps nothing
   ctx->surf_kept = 0;
   ctx->surf_nv = ctx->surf_nt = 0;
   if (const char* why = lattice_check(origin, spacing, dims)) return refuse(ctx, "sph_hip_extract_surface", why);
   if (const char* why = surf_check(iso, flags)) return refuse(ctx, "sph_hip_extract_surface", why);
   if ((rc = sample_check(ctx, "sph_hip_extract_surface"))) return rc;
   ctx->surf_flags = flags;
   const bool normals = (flags & SPH_HIP_SURFACE_NORMALS) != 0, vel = (flags & SPH_HIP_SURFACE_VELOCITY) != 0;
   if (ctx->n == 0) {
      // nothing resident: the density is 0 everywhere, nothing is inside (iso > 0)
      ctx->surf_kept = 1;
      if (counts) counts[0] = counts[1] = 0;
      return SPH_HIP_OK;
   }
   if ((rc = sample_prepare(ctx))) return rc;

   const int nx = dims[0], ny = dims[1], nz = dims[2];
   const int P = surf_planes(dims, vel, ctx->surf_planes_forced);
   const SurfScratch sz = surf_scratch(dims, P, vel);
   if (sz.classified > SURF_MAX_SLAB_POINTS) {
      ctx->err = "sph_hip_extract_surface: lattice planes too large to mesh";
      return SPH_HIP_ERR_CAPACITY;
   }
   const int nslabs = div_up(nz, P);
   if ((rc = ctx->surf_scratch.reserve(ctx, (size_t)sz.bytes,
                                       "sph_hip_extract_surface: cannot allocate the slab scratch")))
      return rc;
   if ((rc = ctx->surf_totals.reserve(ctx, 4 * (size_t)(nslabs + 1)))) return rc;
   if (!ctx->surf_totals_host) SPH_TRY(pinned_alloc(ctx->surf_totals_host, 4));
   Carver carve{ctx->surf_scratch};
   float* srho = carve.take<float>(sz.sampled * 4);
   int32_t* scnt = carve.take<int32_t>(sz.sampled * 4);
   float* svel = vel ? carve.take<float>(sz.sampled * 12) : nullptr;
   uint8_t* codes = carve.take<uint8_t>(sz.classified);
   int32_t* vbase = carve.take<int32_t>(sz.classified * 4);
   int2* active = carve.take<int2>(sz.own * 8);
   uint32_t* bsum_pack = carve.take<uint32_t>(sz.blocks * 4);
   uint32_t* bsum_vown = carve.take<uint32_t>(sz.blocks * 4);
   uint32_t* boff_v = carve.take<uint32_t>(sz.blocks * 4);
   uint32_t* boff_t = carve.take<uint32_t>(sz.blocks * 4);
   uint32_t* boff_a = carve.take<uint32_t>(sz.blocks * 4);
   unsigned long long* totals = ctx->surf_totals;
   unsigned long long* host = ctx->surf_totals_host;

   double cells[3];
   sample_spacing_cells(spacing, ctx->grid.inv, cells);
   const SampleBrick brick = sample_brick(dims, cells);
   const bool unit = unit_scale(ctx->prm);
   hipStream_t st = ctx->stream;
   SPH_TRY(hipMemsetAsync(totals, 0, 4 * sizeof(unsigned long long), st));

   SurfSlab S;
   S.nx = nx;
   S.ny = ny;
   S.nz = nz;
   S.plane = nx * ny;
   S.ox = origin[0];
   S.oy = origin[1];
   S.oz = origin[2];
   S.sx = spacing[0];
   S.sy = spacing[1];
   S.sz = spacing[2];
   S.iso = iso;
   SampleLattice L = lattice_of(origin, spacing, brick);
   L.ex = nx;
   L.ey = ny;
   L.bricks_x = div_up(nx, L.bx);
   L.bricks_y = div_up(ny, L.by);
   long long nv = 0, nt = 0;   // vertices and triangles before the slab
   for (int s = 0; s < nslabs; s++) {
      S.k0 = s * P;
      S.own = nz - S.k0 < P ? nz - S.k0 : P;
      S.cls = nz - S.k0 < P + 1 ? nz - S.k0 : P + 1;
      S.ks0 = S.k0 - SURF_HALO_BELOW < 0 ? 0 : S.k0 - SURF_HALO_BELOW;
      const int ks1 = S.k0 + P + SURF_HALO_ABOVE < nz ? S.k0 + P + SURF_HALO_ABOVE : nz;
      // 1. density (+ velocity) of the slab's planes and halo: the sampler's kernel and bits
      L.k0 = S.ks0;
      L.ez = ks1 - S.ks0;
      const int bricks = L.bricks_x * L.bricks_y * div_up(L.ez, L.bz);
      bind_flags([&](auto U, auto V) {
         sample_lattice_launch<U.value, SampleSum<V.value>>(ctx, L, bricks, ctx->velp[ctx->cur], {srho, svel, scnt});
      }, unit, vel);
      SPH_TRY(hipGetLastError());
      // 2. classify, 3. scan
      const int pts = S.cls * S.plane;
      const int nb = div_up(pts, SURF_THREADS);
      hipLaunchKernelGGL(k_surf_classify, dim3(nb), dim3(SURF_THREADS), 0, st, S, srho, codes, bsum_pack, bsum_vown);
      SPH_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_surf_scan, dim3(1), dim3(SURF_THREADS), 0, st, nb, bsum_pack, bsum_vown, boff_v, boff_t,
                         boff_a, totals + 4 * (size_t)s, totals + 4 * (size_t)(s + 1));
      SPH_TRY(hipGetLastError());
      // the slab's totals: the mesh arrays must hold them before anything is emitted
      SPH_TRY(hipMemcpyAsync(host, totals + 4 * (size_t)(s + 1), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             st));
      SPH_TRY(hipStreamSynchronize(st));
      const long long nv_next = (long long)host[0], nt_next = (long long)host[1];
      const int nactive = (int)host[2];
      if (nv + (long long)host[3] > 0x7fffffffll || nt_next > 0x7fffffffll) {
         ctx->err = "sph_hip_extract_surface: more than 2^31 - 1 vertices or triangles";
         return SPH_HIP_ERR_CAPACITY;
      }
      rc = surf_grow(ctx, ctx->surf_vtx, ctx->surf_vtx_cap, 3 * nv_next, 3 * nv);
      if (!rc && normals) rc = surf_grow(ctx, ctx->surf_nrm, ctx->surf_nrm_cap, 3 * nv_next, 3 * nv);
      if (!rc && vel) rc = surf_grow(ctx, ctx->surf_vel, ctx->surf_vel_cap, 3 * nv_next, 3 * nv);
      if (!rc) rc = surf_grow(ctx, ctx->surf_tri, ctx->surf_tri_cap, 3 * nt_next, 3 * nt);
      if (rc) {
         if (rc == SPH_HIP_ERR_CAPACITY) ctx->err = "sph_hip_extract_surface: cannot allocate the mesh";
         return rc;
      }
      // 4. vertex bases, active cubes, vertices, 5. triangles
      bind_flags([&](auto N, auto V) {
         hipLaunchKernelGGL((k_surf_vertices<N.value, V.value>), dim3(nb), dim3(SURF_THREADS), 0, st, S, srho, svel,
                            codes, boff_v, boff_t, boff_a, totals + 4 * (size_t)s, vbase, active, ctx->surf_vtx.get(),
                            ctx->surf_nrm.get(), ctx->surf_vel.get());
      }, normals, vel);
      SPH_TRY(hipGetLastError());
      if (nactive > 0) {
         hipLaunchKernelGGL(k_surf_triangles, dim3(div_up(nactive, SURF_THREADS)), dim3(SURF_THREADS), 0, st, S, codes,
                            vbase, active, nactive, ctx->surf_tri.get());
         SPH_TRY(hipGetLastError());
      }
      nv = nv_next;
      nt = nt_next;
   }
   SPH_TRY(hipStreamSynchronize(st));
   ctx->surf_nv = nv;
   ctx->surf_nt = nt;
   ctx->surf_kept = 1;
   if (counts) {
      counts[0] = (int32_t)nv;
      counts[1] = (int32_t)nt;
   }
   return SPH_HIP_OK;
}

int sph_hip_download_surface(sph_hip_context* ctx, float* vertices_xyz, float* normals_xyz, float* velocity_xyz,
                             int32_t* triangles)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if (!ctx->surf_kept) {
      ctx->err = "sph_hip_download_surface: no mesh is kept (extract one first)";
      return SPH_HIP_ERR_INVALID;
   }
   if ((normals_xyz && !(ctx->surf_flags & SPH_HIP_SURFACE_NORMALS)) ||
       (velocity_xyz && !(ctx->surf_flags & SPH_HIP_SURFACE_VELOCITY))) {
      ctx->err = "sph_hip_download_surface: the extraction did not compute normals / velocity";
      return SPH_HIP_ERR_INVALID;
   }
   hipStream_t st = ctx->stream;
   const size_t v3 = 3 * (size_t)ctx->surf_nv, t3 = 3 * (size_t)ctx->surf_nt;
   if (vertices_xyz && v3) SPH_TRY(hipMemcpyAsync(vertices_xyz, ctx->surf_vtx.get(), sizeof(float) * v3, hipMemcpyDeviceToHost, st));
   if (normals_xyz && v3) SPH_TRY(hipMemcpyAsync(normals_xyz, ctx->surf_nrm.get(), sizeof(float) * v3, hipMemcpyDeviceToHost, st));
   if (velocity_xyz && v3) SPH_TRY(hipMemcpyAsync(velocity_xyz, ctx->surf_vel.get(), sizeof(float) * v3, hipMemcpyDeviceToHost, st));
   if (triangles && t3) SPH_TRY(hipMemcpyAsync(triangles, ctx->surf_tri.get(), sizeof(int32_t) * t3, hipMemcpyDeviceToHost, st));
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

// ---- renderer -------------------------------------------------------------------------------------

namespace {

// the solids a scene frame draws (null: sph_hip_render's frame)
struct SceneDraw {
   sph_hip_scene_params sp;
   int n;               // solids in ctx->scene_list_host
   int32_t* solid_id;   // host output, may be null
};

// the tint of a scalar frame (null: no pixel is tinted)
struct TintDraw {
   sph_hip_tint_params tp;
   const float* table;   // host, 3 * n_colors floats
   float* scalar;        // host output, may be null
   int velgrad = 0;      // tp.channel is a velocity-gradient quantity 0 .. 7 (sph_hip_render_velocity_gradients)
};

// The frame of the three entry points, arguments checked: the row chunks, their scratch, the launches and the
// copies.  `who` names the caller in an error text.
int render_frame(sph_hip_context* ctx, const char* who, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                 int width, int height, int flags, uint8_t* rgba, float* depth, float* normal_xyz,
                 float* velocity_xyz, int32_t* first_inside, const SceneDraw* scene, const TintDraw* tint = nullptr)
{
   int rc;
   const size_t pixels = (size_t)width * height;
   const bool vel = (flags & SPH_HIP_RENDER_VELOCITY) != 0;
   const bool solids = scene && scene->n > 0;
   const bool tinted = frame_launches_tint(tint != nullptr, ctx->n);
   if (tint && !tinted && tint->scalar) memset(tint->scalar, 0, sizeof(float) * pixels);
   if (velocity_xyz && !vel) memset(velocity_xyz, 0, sizeof(float) * 3 * pixels);
   if (scene && !solids && scene->solid_id) memset(scene->solid_id, 0xff, sizeof(int32_t) * pixels);
   if (ctx->n == 0 && !solids) {
      // nothing resident (the cell arrays may still describe an earlier upload): every ray misses
      for (size_t i = 0; i < pixels; i++) {
         if (rgba) memcpy(rgba + 4 * i, rp->background, 4);
         if (depth) depth[i] = INFINITY;
         if (first_inside) first_inside[i] = -1;
      }
      if (normal_xyz) memset(normal_xyz, 0, sizeof(float) * 3 * pixels);
      if (velocity_xyz) memset(velocity_xyz, 0, sizeof(float) * 3 * pixels);
      return SPH_HIP_OK;
   }
   const bool fluid = ctx->n > 0;   // without a particle the solids are drawn over a background frame
   if (fluid && (rc = sample_prepare(ctx))) return rc;
   // the channels by sorted slot, once: the carried scalars staged, or the velocity-gradient rows formed
   if (tinted && (rc = tint->velgrad ? launch_velgrad(ctx) : launch_scalars_stage(ctx, false))) return rc;
   hipStream_t st = ctx->stream;
   const CellGrid& g = ctx->grid;
   const bool skip = !ctx->render_noskip;
   if (fluid && skip) {
      if ((rc = ctx->render_occ.reserve(ctx, (size_t)g.ncells))) return rc;
      hipLaunchKernelGGL(k_render_occupancy, dim3(div_up(g.ncells, RENDER_THREADS)), dim3(RENDER_THREADS), 0, st,
                         ctx->cell_start, g, ctx->render_occ.get());
      SPH_TRY(hipGetLastError());
   }
   // scratch of one row chunk (render_policy.h)
   const int rows = render_chunk_rows(width, height);
   const std::string no_scratch = std::string(who) + ": cannot allocate the chunk scratch";
   if ((rc = ctx->render_scratch.reserve(ctx, (size_t)render_scratch_bytes(width, rows), no_scratch.c_str())))
      return rc;
   const long long cp = (long long)width * rows;
   Carver carve{ctx->render_scratch};
   uint32_t* s_rgba = carve.take<uint32_t>(cp * 4);
   float* s_depth = carve.take<float>(cp * 4);
   float* s_nrm = carve.take<float>(cp * 12);
   float* s_vel = carve.take<float>(cp * 12);
   int32_t* s_first = carve.take<int32_t>(cp * 4);
   int32_t* s_hits = carve.take<int32_t>(cp * 4);
   uint32_t* s_count = carve.take<uint32_t>(256);
   int32_t* s_id = nullptr;
   if (solids) {
      // the scene pass's own scratch (scene_policy.h) and the list, on the device before the first chunk
      if ((rc = ctx->scene_id.reserve(ctx, (size_t)(scene_id_bytes(width, rows) / 4), no_scratch.c_str()))) return rc;
      if ((rc = ctx->scene_list.reserve(ctx, SPH_HIP_MAX_OBSTACLES))) return rc;
      s_id = ctx->scene_id.get();
      SPH_TRY(hipMemcpyAsync(ctx->scene_list.get(), ctx->scene_list_host, sizeof(SceneSolid) * (size_t)scene->n,
                             hipMemcpyHostToDevice, st));
   }
   float* s_scalar = nullptr;
   TintArgs T = {};
   if (tinted) {
      // the tint pass's own scratch (tint_policy.h) and the table, on the device before the first chunk
      if ((rc = ctx->tint_scalar.reserve(ctx, (size_t)(tint_scalar_bytes(width, rows) / 4), no_scratch.c_str()))) return rc;
      if ((rc = ctx->tint_table.reserve(ctx, TINT_TABLE_FLOATS))) return rc;
      s_scalar = ctx->tint_scalar.get();
      const size_t table_bytes = sizeof(float) * 3 * (size_t)tint->tp.n_colors;
      memcpy(ctx->tint_table_host, tint->table, table_bytes);
      SPH_TRY(hipMemcpyAsync(ctx->tint_table.get(), ctx->tint_table_host, table_bytes, hipMemcpyHostToDevice, st));
      T.tp = tint->tp;
      T.table = ctx->tint_table.get();
      if (tint->velgrad) T.tp.channel = velgrad_quantity_component(tint->tp.channel);
   }
   // what the tint kernels walk: the staged scalars, or the array that holds the quantity
   const float4* tint_rows = !tinted          ? nullptr
                             : !tint->velgrad ? ctx->scalar_Ts.get()
                             : velgrad_quantity_group(tint->tp.channel) == 0 ? ctx->velgrad_A.get() : ctx->velgrad_B.get();
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   const bool unit = unit_scale(ctx->prm);
   const unsigned char* occ = skip ? ctx->render_occ.get() : nullptr;
   RenderFrame F;
   F.cam = *cam;
   F.rp = *rp;
   F.width = width;
   F.height = height;
   F.tiles_x = div_up(width, RENDER_TILE);
   for (F.row0 = 0; F.row0 < height; F.row0 += rows) {
      F.rows = height - F.row0 < rows ? height - F.row0 : rows;
      const int chunk = width * F.rows;
      const int tiles = F.tiles_x * div_up(F.rows, RENDER_TILE);
      if (fluid) {
         SPH_TRY(hipMemsetAsync(s_count, 0, sizeof(uint32_t), st));
         bind_flags([&](auto U, auto S) {
            hipLaunchKernelGGL((k_render_march<U.value, S.value>), dim3(div_up(tiles, RENDER_THREADS / SPH_WAVE)),
                               dim3(RENDER_THREADS), 0, st, F, ctx->posm[ctx->cur], ctx->cell_start, g, k, occ, s_rgba,
                               s_depth, s_nrm, s_vel, s_first, s_hits, s_count);
         }, unit, skip);
         SPH_TRY(hipGetLastError());
         bind_flags([&](auto U, auto S, auto V) {
            hipLaunchKernelGGL((k_render_shade<U.value, S.value, V.value>), dim3(div_up(chunk, RENDER_THREADS)),
                               dim3(RENDER_THREADS), 0, st, F, ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->cell_start,
                               g, k, occ, s_hits, s_count, s_first, s_rgba, s_depth, s_nrm, s_vel);
         }, unit, skip, vel);
         SPH_TRY(hipGetLastError());
      }
      if (solids) {
         bind_flags([&](auto FILL) {
            hipLaunchKernelGGL((k_scene_solids<FILL.value>), dim3(div_up(tiles, RENDER_THREADS / SPH_WAVE)),
                               dim3(RENDER_THREADS), 0, st, F, scene->sp,
                               reinterpret_cast<const uint32_t*>(ctx->scene_list.get()), scene->n, vel ? 1 : 0, s_rgba,
                               s_depth, s_nrm, s_vel, s_first, s_id);
         }, !fluid);
         SPH_TRY(hipGetLastError());
      }
      if (tinted) {
         // untinted pixels keep this 0; the hit list and its count are the march's, still in the scratch
         SPH_TRY(hipMemsetAsync(s_scalar, 0, sizeof(float) * (size_t)chunk, st));
         const bool flat = (tint->tp.flags & SPH_HIP_TINT_FLAT) != 0;
         if (tint->tp.mode == SPH_HIP_TINT_SURFACE)
            bind_flags([&](auto U, auto FL) {
               hipLaunchKernelGGL((k_tint_surface<U.value, FL.value>), dim3(div_up(chunk, RENDER_THREADS)),
                                  dim3(RENDER_THREADS), 0, st, F, T, ctx->posm[ctx->cur], tint_rows, ctx->cell_start,
                                  g, k, s_hits, s_count, s_first, s_depth, s_nrm, s_rgba, s_scalar);
            }, unit, flat);
         else
            bind_flags([&](auto U, auto S, auto FL) {
               hipLaunchKernelGGL((k_tint_column<U.value, S.value, FL.value>), dim3(div_up(chunk, RENDER_THREADS)),
                                  dim3(RENDER_THREADS), 0, st, F, T, ctx->posm[ctx->cur], tint_rows, ctx->cell_start,
                                  g, k, occ, s_hits, s_count, s_first, s_nrm, s_rgba, s_scalar);
            }, unit, skip, flat);
         SPH_TRY(hipGetLastError());
      }
      const size_t o = (size_t)F.row0 * width;
      if (rgba) SPH_TRY(hipMemcpyAsync(rgba + 4 * o, s_rgba, (size_t)chunk * 4, hipMemcpyDeviceToHost, st));
      if (depth) SPH_TRY(hipMemcpyAsync(depth + o, s_depth, (size_t)chunk * 4, hipMemcpyDeviceToHost, st));
      if (normal_xyz) SPH_TRY(hipMemcpyAsync(normal_xyz + 3 * o, s_nrm, (size_t)chunk * 12, hipMemcpyDeviceToHost, st));
      if (velocity_xyz && vel)
         SPH_TRY(hipMemcpyAsync(velocity_xyz + 3 * o, s_vel, (size_t)chunk * 12, hipMemcpyDeviceToHost, st));
      if (first_inside) SPH_TRY(hipMemcpyAsync(first_inside + o, s_first, (size_t)chunk * 4, hipMemcpyDeviceToHost, st));
      if (solids && scene->solid_id)
         SPH_TRY(hipMemcpyAsync(scene->solid_id + o, s_id, (size_t)chunk * 4, hipMemcpyDeviceToHost, st));
      if (tinted && tint->scalar)
         SPH_TRY(hipMemcpyAsync(tint->scalar + o, s_scalar, (size_t)chunk * 4, hipMemcpyDeviceToHost, st));
   }
   SPH_TRY(hipStreamSynchronize(st));
   return SPH_HIP_OK;
}

// the solids as they stand now (sph_hip_get_obstacles_now's list), their velocities and albedos, into
// ctx->scene_list_host
int scene_solids_now(sph_hip_context* ctx, const SceneDraw& scene, const sph_hip_scene_params* sp,
                     const float* solid_albedo_rgb, int n_albedo)
{
   int rc;
   sph_hip_obstacle now[SPH_HIP_MAX_OBSTACLES];
   BodyState st[SPH_HIP_MAX_OBSTACLES];
   if ((rc = obstacles_now(ctx, now, scene.n, st))) return rc;
   for (int i = 0; i < scene.n; i++) {
      SceneSolid& s = ctx->scene_list_host[i];
      s.o = now[i];
      if (ctx->n_bodies > 0 && body_is(ctx->bodies_host[i]))
         for (int c = 0; c < 3; c++) s.vel[c] = st[i].V[c];
      else if (i < ctx->n_path_entries && path_is(ctx->paths_host[i]))
         path_velocity(ctx->paths_host[i], ctx->path_keys_host.data(), ctx->motion_tau, s.vel);
      else if (i < ctx->n_motion)
         scene_motion_velocity(ctx->motion_host[i], ctx->motion_tau, s.vel);
      else
         for (int c = 0; c < 3; c++) s.vel[c] = 0.0f;
      for (int c = 0; c < 3; c++) s.alb[c] = n_albedo > 0 ? solid_albedo_rgb[3 * i + c] : sp->albedo[c];
   }
   return SPH_HIP_OK;
}

} // namespace

int sph_hip_render(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp, int width,
                   int height, int flags, uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz,
                   int32_t* first_inside)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = sample_check(ctx, "sph_hip_render"))) return rc;
   if (const char* why = render_check(cam, rp, width, height, flags)) return refuse(ctx, "sph_hip_render", why);
   return render_frame(ctx, "sph_hip_render", cam, rp, width, height, flags, rgba, depth, normal_xyz, velocity_xyz,
                       first_inside, nullptr);
}

// ---- scene renderer (scene_kernels.h; decisions: scene_policy.h) ---------------------------------------

int sph_hip_render_scene(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                         const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo, int width,
                         int height, int flags, uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz,
                         int32_t* first_inside, int32_t* solid_id)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   if ((rc = sample_check(ctx, "sph_hip_render_scene"))) return rc;
   if (const char* why = scene_check(cam, rp, sp, solid_albedo_rgb, n_albedo, ctx->n_obst, width, height, flags))
      return refuse(ctx, "sph_hip_render_scene", why);
   SceneDraw scene = {*sp, ctx->n_obst, solid_id};
   if ((rc = scene_solids_now(ctx, scene, sp, solid_albedo_rgb, n_albedo))) return rc;
   return render_frame(ctx, "sph_hip_render_scene", cam, rp, width, height, flags, rgba, depth, normal_xyz,
                       velocity_xyz, first_inside, &scene);
}

// ---- scalar renderer (tint_kernels.h; decisions: tint_policy.h) -----------------------------------------

int sph_hip_render_scalars(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                           const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo,
                           const sph_hip_tint_params* tp, const float* table_rgb, int width, int height, int flags,
                           uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz, int32_t* first_inside,
                           int32_t* solid_id, float* scalar)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_render_scalars";
   if ((rc = sample_check(ctx, who))) return rc;
   if (const char* why = tint_check(cam, rp, sp, solid_albedo_rgb, n_albedo, ctx->n_obst, ctx->n_scalars, tp, table_rgb,
                                    width, height, flags))
      return refuse(ctx, who, why);
   const TintDraw tint = {*tp, table_rgb, scalar, 0};
   if (!sp) {
      // fluid only: sph_hip_render's frame, solid_id -1 everywhere
      if (solid_id) memset(solid_id, 0xff, sizeof(int32_t) * (size_t)width * height);
      return render_frame(ctx, who, cam, rp, width, height, flags, rgba, depth, normal_xyz, velocity_xyz, first_inside,
                          nullptr, &tint);
   }
   SceneDraw scene = {*sp, ctx->n_obst, solid_id};
   if ((rc = scene_solids_now(ctx, scene, sp, solid_albedo_rgb, n_albedo))) return rc;
   return render_frame(ctx, who, cam, rp, width, height, flags, rgba, depth, normal_xyz, velocity_xyz, first_inside,
                       &scene, &tint);
}

// ---- velocity-gradient renderer: the scalar renderer's frame tinted by one of the eight quantities -----------

int sph_hip_render_velocity_gradients(sph_hip_context* ctx, const sph_hip_camera* cam, const sph_hip_render_params* rp,
                                      const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo,
                                      const sph_hip_tint_params* tp, const float* table_rgb, int width, int height,
                                      int flags, uint8_t* rgba, float* depth, float* normal_xyz, float* velocity_xyz,
                                      int32_t* first_inside, int32_t* solid_id, float* scalar)
{
   int rc = check_ctx(ctx);
   if (rc) return rc;
   const char* who = "sph_hip_render_velocity_gradients";
   if ((rc = sample_check(ctx, who))) return rc;
   // tp->channel carries the quantity: checked here, and the scalar renderer's checks see a channel of their own
   if (!tp) return refuse(ctx, who, "null tint params or colour table");
   if (const char* why = velgrad_quantity_check(tp->channel)) return refuse(ctx, who, why);
   sph_hip_tint_params as_channel = *tp;
   as_channel.channel = velgrad_quantity_component(tp->channel);
   if (const char* why = tint_check(cam, rp, sp, solid_albedo_rgb, n_albedo, ctx->n_obst, 1, &as_channel, table_rgb, width,
                                    height, flags))
      return refuse(ctx, who, why);
   TintDraw tint = {*tp, table_rgb, scalar};
   tint.velgrad = 1;
   if (!sp) {
      if (solid_id) memset(solid_id, 0xff, sizeof(int32_t) * (size_t)width * height);
      return render_frame(ctx, who, cam, rp, width, height, flags, rgba, depth, normal_xyz, velocity_xyz, first_inside,
                          nullptr, &tint);
   }
   SceneDraw scene = {*sp, ctx->n_obst, solid_id};
   if ((rc = scene_solids_now(ctx, scene, sp, solid_albedo_rgb, n_albedo))) return rc;
   return render_frame(ctx, who, cam, rp, width, height, flags, rgba, depth, normal_xyz, velocity_xyz, first_inside,
                       &scene, &tint);
}

void* sph_hip_stream(sph_hip_context* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

} // extern "C"

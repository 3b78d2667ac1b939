// FULL mode: the neighbour lists the density pass hands to the acceleration pass, and the flag per
// workgroup that says which of its particles have one.  This header owns their format; the two
// density kernels write them through ListWriter, the acceleration routes read them through ListReader.
//
// 16-bit entries (ListEntry), per workgroup a block of list_rows(list_cap) * TILE_THREADS 32-bit
// words laid out in BLOCKS OF EIGHT ENTRIES: entries 8b .. 8b+7 of lane t are the 16 bytes at
// b * LIST_BLOCK_BYTES + 16 t.  A consumer fetches a trip's eight entries with one 16-byte load per
// lane (a wave: 1 KB contiguous); the producer fills a 16-byte slot with eight consecutive 2-byte
// stores of ONE lane, so a 128-byte line is complete after eight lanes have taken eight pops each and
// leaves the L2 whole.  (Until round 4 entry j sat in half (j & 1) of word (j >> 1) * TILE_THREADS + t:
// a line was shared by 32 lanes x 2 entries and stayed open until the slowest of them got there - in a
// compressed scene, 150 entries per particle and three workgroups per CU, the open lines outgrew the L2
// several times over and the density pass WROTE 9 GB for 1.3 GB of entries: profiles/r4_notes.md.)
// Only blocks in use are ever touched.  list_cap - the neighbours per particle the lists hold - is a
// launch argument: a context starts with NLIST_CAP and the host enlarges it (up to NLIST_CAP_MAX,
// memory permitting) when the density pass reports particles that went without a list.
#pragma once

#include "launch_policy.h"
#include "sph_device.h"

constexpr int NLIST_CAP = 254;
#define NLIST_CAP_MAX 1022
#define LIST_BLOCK_ENTRIES 8
#define LIST_BLOCK_BYTES (16 * TILE_THREADS)
static_assert(NLIST_CAP <= NLIST_CAP_MAX, "initial list capacity");

// rows of TILE_THREADS words a workgroup's list block takes: whole blocks for entries 0 .. list_cap
__host__ __device__ __forceinline__ constexpr int list_rows(int list_cap)
{
   return 4 * ((list_cap + LIST_BLOCK_ENTRIES) / LIST_BLOCK_ENTRIES);
}

// The flag per workgroup (nlist_overflow[wg]), written by the density pass.
constexpr uint32_t LISTS_ALL = 0u;    // every particle of the workgroup has its list
constexpr uint32_t LISTS_NONE = 1u;   // no lists: the tile did not fit (or its indices do not fit an entry)
constexpr uint32_t LISTS_SOME = 2u;   // some particle has more neighbours than list_cap: NLIST_NO_LIST
// first list word of a particle that has no list (more neighbours than list_cap): no valid
// entry has segment id 15
#define NLIST_NO_LIST 0xffffffffu

// byte offset of entry j of the lane whose slots start at lane_off (= 16 * lane) in the block
__device__ __forceinline__ uint32_t list_entry_off(uint32_t j, uint32_t lane_off)
{
   return (j >> 3) * (uint32_t)LIST_BLOCK_BYTES + lane_off + (j & 7u) * 2u;
}
// The append's running position.  pos holds block and slot of the next entry with the lane field
// (bits 4 .. 4 + log2(TILE_THREADS)) ALL ONES: pos += 2 then carries from the slot field straight
// into the block field when a 16-byte slot is full (and leaves the lane field zero: or it back).
// The address puts the lane in: one v_bfi.  Three instructions per entry, none of them a shift.
#define LIST_LANE_FIELD ((uint32_t)(LIST_BLOCK_BYTES - 16))
#define LIST_SLOT_FIELD 14u   // the entry's two bytes inside its 16-byte slot
__device__ __forceinline__ uint32_t list_pos_of(uint32_t j)
{
   return ((j >> 3) * (uint32_t)LIST_BLOCK_BYTES + (j & 7u) * 2u) | LIST_LANE_FIELD;
}
__device__ __forceinline__ uint32_t list_pos_off(uint32_t pos, uint32_t lane_off)
{
   return (LIST_LANE_FIELD & lane_off) | (~LIST_LANE_FIELD & pos);      // v_bfi_b32
}
__device__ __forceinline__ uint32_t list_pos_next(uint32_t pos) { return (pos + 2u) | LIST_LANE_FIELD; }
__device__ __forceinline__ uint32_t list_entry_load(const char* __restrict__ lists, uint32_t j, uint32_t lane_off)
{
   return *reinterpret_cast<const uint16_t*>(lists + list_entry_off(j, lane_off));
}
// the eight entries of block b of that lane
__device__ __forceinline__ uint4 list_block_load(const char* __restrict__ lists, int b, uint32_t lane_off)
{
   return *reinterpret_cast<const uint4*>(lists + (uint32_t)b * (uint32_t)LIST_BLOCK_BYTES + lane_off);
}
__device__ __forceinline__ void list_block_entries(const uint4& blk, uint32_t (&entry)[8])
{
   entry[0] = blk.x & 0xffffu; entry[1] = blk.x >> 16;
   entry[2] = blk.y & 0xffffu; entry[3] = blk.y >> 16;
   entry[4] = blk.z & 0xffffu; entry[5] = blk.z >> 16;
   entry[6] = blk.w & 0xffffu; entry[7] = blk.w >> 16;
}
// Four consecutive entries that start at slot `first` (0 .. 7) of block `a` and run on into block `b`
// (the block after it): a run of entries that begins anywhere in a list, taken out of two 16-byte
// loads without a register array indexed per lane (which would live in scratch) - three 4-way word
// selects and two funnel shifts.  (first + 3 <= 10: of `b` only its first two words can be needed.)
__device__ __forceinline__ void list_entries_from(const uint4& a, const uint4& b, uint32_t first, uint32_t (&entry)[4])
{
   const uint32_t w = first >> 1;
   const uint32_t w0 = w == 0u ? a.x : w == 1u ? a.y : w == 2u ? a.z : a.w;
   const uint32_t w1 = w == 0u ? a.y : w == 1u ? a.z : w == 2u ? a.w : b.x;
   const uint32_t w2 = w == 0u ? a.z : w == 1u ? a.w : w == 2u ? b.x : b.y;
   const uint32_t sh = (first & 1u) * 16u;
   const uint32_t lo = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
   const uint32_t hi = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
   entry[0] = lo & 0xffffu; entry[1] = lo >> 16;
   entry[2] = hi & 0xffffu; entry[3] = hi >> 16;
}
// Zeroes the entries between a list's end and the end of its last block (0 is a valid tile index):
// the bit-exact acceleration loop gathers by every entry of a fetched block before it looks at the
// count, and what an earlier step left there need not be an index of this step's tile.
__device__ __forceinline__ void list_pad(char* __restrict__ lists, uint32_t lane_off, int count, int list_cap)
{
   if (count >= list_cap + 1) return;
   uint32_t c = (uint32_t)count;
   if (c & 1u) { *reinterpret_cast<uint16_t*>(lists + list_entry_off(c, lane_off)) = (uint16_t)0; c += 1u; }
   if (c & 2u) { *reinterpret_cast<uint32_t*>(lists + list_entry_off(c, lane_off)) = 0u; c += 2u; }
   if (c & 4u) { *reinterpret_cast<uint2*>(lists + list_entry_off(c, lane_off)) = make_uint2(0u, 0u); }
}

// A 16-bit list entry is a tile index plus what it takes to get back from it to the neighbour's
// sorted position (tile index - D[segment]).  Narrow (tiles up to 4064 entries): segment id << 12 |
// 12-bit index.  Wide (scenes several times denser, tiles up to 16352 entries, chosen per step by
// the host): plane dz + 1 << 14 | 14-bit index; the row inside the plane follows from the index
// and the descriptor's segment starts B - two more LDS reads and compares per neighbour, which is
// why it is not the only format.
template <bool WIDE>
struct ListEntry {
   static constexpr int TBITS = WIDE ? 14 : 12;
   static constexpr uint32_t TMASK = (1u << TBITS) - 1u;
   __device__ static __forceinline__ uint32_t tag(int segment)
   {
      return (uint32_t)(WIDE ? segment / 3 : segment) << TBITS;
   }
   __device__ static __forceinline__ int tile(uint32_t e) { return (int)(e & TMASK); }
   // D of the entry's segment.  Segments of a plane that share storage have equal D, and an
   // empty segment starts where the next begins, so comparing with the starts finds a valid one.
   template <class Desc>
   __device__ static __forceinline__ int shift(const Desc& d, uint32_t e)
   {
      if (!WIDE) return d.D[e >> TBITS];
      const int z = (int)(e >> TBITS), t = (int)(e & TMASK);
      const int k = 3 * z + (t >= d.B[3 * z + 1] ? 1 : 0) + (t >= d.B[3 * z + 2] ? 1 : 0);
      return d.D[k];
   }
};
static_assert(TILE_CAP_MAX + TILE_PAD <= (1 << ListEntry<false>::TBITS) &&
                 TILE_CAP_MAX_WIDE + TILE_PAD <= (1 << ListEntry<true>::TBITS),
              "tile index must fit the list entry");

// uniform base of workgroup wg's list block; lanes address it with 32-bit offsets
template <class Word>
__device__ __forceinline__ Word* list_block_of(Word* nlist, int wg, int list_cap)
{
   return nlist + (size_t)wg * (size_t)(list_rows(list_cap) * TILE_THREADS);
}

// The consumer's side: one lane's list in its workgroup's block.
struct ListReader {
   const char* lists;
   uint32_t lane_off;
   __device__ __forceinline__ ListReader(const uint32_t* nlist, int wg, int list_cap, int lane)
      : lists(reinterpret_cast<const char*>(list_block_of(nlist, wg, list_cap))), lane_off(16u * (uint32_t)lane)
   {
   }
   __device__ __forceinline__ uint4 block(int b) const { return list_block_load(lists, b, lane_off); }
   __device__ __forceinline__ uint32_t entry(uint32_t j) const { return list_entry_load(lists, j, lane_off); }
   // (only in a workgroup flagged LISTS_SOME, and only for a lane with neighbours, does the first word
   // mean anything else than entries)
   __device__ __forceinline__ bool no_list() const
   {
      return *reinterpret_cast<const uint32_t*>(lists + lane_off) == NLIST_NO_LIST;
   }
};

// The producer's side: one lane appends its neighbours in canonical order; pos (list_pos_of(entries
// appended)) is the caller's own variable - kept in the writer, it changed the tiled density kernel's
// code.  A STAGED append collects
// the entries of the current block in the lane's 16-byte slot in LDS (list_stage_clear first) and
// writes the block with ONE 16-byte store when it is full; an unstaged one writes every entry with a
// 2-byte store.  (The texture addresser was busy 80 % of the density pass with the 2-byte stores - one
// per accepted neighbour, each to a 16-byte slot of its own, 13 L2 requests per wave-instruction - and
// every other load of the CU queued behind them: with seven stores in eight left out (a probe, lists
// wrong) a workgroup's life went from 55 to 45 us, its prologue from 13 to 9 us: tools/phase_clock.py,
// tools/pmc_latency.sh, profiles/r4_notes.md 4c.)
__device__ __forceinline__ void list_stage_clear(char* stage_lane)
{
   *reinterpret_cast<uint4*>(stage_lane) = make_uint4(0u, 0u, 0u, 0u);
}

struct ListWriter {
   char* lists;
   uint32_t lane_off;
   char* stage;     // the lane's staging slot in LDS (staged appends only)
   __device__ __forceinline__ ListWriter(uint32_t* nlist, int wg, int list_cap, int lane, char* stage_lane)
      : lists(reinterpret_cast<char*>(list_block_of(nlist, wg, list_cap))), lane_off(16u * (uint32_t)lane),
        stage(stage_lane)
   {
   }
   template <bool STAGED>
   __device__ __forceinline__ void append(uint32_t& pos, uint32_t e)
   {
      const uint32_t in_block = pos & LIST_SLOT_FIELD;
      if constexpr (STAGED) {
         *reinterpret_cast<uint16_t*>(stage + in_block) = (uint16_t)e;
         if (in_block == LIST_SLOT_FIELD)   // the block is complete: one 16-byte store
            *reinterpret_cast<uint4*>(lists + list_pos_off(pos & ~LIST_SLOT_FIELD, lane_off)) =
               *reinterpret_cast<const uint4*>(stage);
      } else {
         *reinterpret_cast<uint16_t*>(lists + list_pos_off(pos, lane_off)) = (uint16_t)e;
      }
      pos = list_pos_next(pos);
   }
   // the list read back (the density pass's SUM)
   __device__ __forceinline__ uint4 block(int b) const { return list_block_load(lists, b, lane_off); }
   // SUM's compaction: entry `kept` of the list becomes e (kept never passes the read position)
   __device__ __forceinline__ void keep(int kept, uint32_t e)
   {
      *reinterpret_cast<uint16_t*>(lists + list_entry_off((uint32_t)kept, lane_off)) = (uint16_t)e;
   }
   __device__ __forceinline__ void pad(int count, int list_cap) { list_pad(lists, lane_off, count, list_cap); }
   // After the last append: the rest of the last block, and the marker of a lane without a list
   // (count > list_cap), which also sets the workgroup's wg_no_list (in LDS).  Unstaged, the rest is
   // list_pad's zeros; staged, the last, partly filled block (or block 0 of a lane without neighbours)
   // is the slot as it is - what lies behind the list's end are entries of the lane's previous block or
   // the zeros the slot started with, valid indices of this tile either way, which is all list_pad's
   // zeros are there for.  Returns whether the lane went without a list.
   __device__ __forceinline__ bool finish(uint32_t pos, int count, int list_cap, bool staged, int& wg_no_list)
   {
      if (!staged)
         list_pad(lists, lane_off, count, list_cap);
      else if (count <= list_cap && ((count & 7) != 0 || count == 0))
         *reinterpret_cast<uint4*>(lists + list_pos_off(pos & ~LIST_SLOT_FIELD, lane_off)) =
            *reinterpret_cast<const uint4*>(stage);
      const bool none = count > list_cap;
      if (none) {
         wg_no_list = 1;
         *reinterpret_cast<uint32_t*>(lists + lane_off) = NLIST_NO_LIST;
      }
      return none;
   }
};

// The workgroup's step after every lane's finish(): the lanes without a list are counted for the host
// (TSTAT_NO_LIST, which then enlarges the lists) and the workgroup's flag is written.
__device__ __forceinline__ void lists_publish(bool no_list, const int& wg_no_list, int32_t* tile_stats,
                                              uint32_t* nlist_overflow, int wg)
{
   if (__any(no_list)) {
      const int without = __popcll(__ballot(no_list));
      if ((threadIdx.x & (SPH_WAVE - 1)) == 0) atomicAdd(&tile_stats[TSTAT_NO_LIST], without);
   }
   __syncthreads();
   if (threadIdx.x == 0) nlist_overflow[wg] = wg_no_list ? LISTS_SOME : LISTS_ALL;
}

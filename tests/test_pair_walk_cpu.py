"""CPU checks of the shared neighbour walk (csrc/pair_walk.h), read from the sources: the header is a dependency of
the build, the pair passes that moved onto it include it and keep no walk of their own, the two that kept a copy
(viscous_kernels.h, velgrad_kernels.h: DESIGN.md, the pair walk) say so, and every kernel's signature is the one the
launches, the C API and the Python layer were written against."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# the passes on the shared walk, and the two that keep a copy of it
SHARED = ("scalar_kernels.h", "monitor_kernels.h", "cohesion_kernels.h", "xsph_kernels.h")
OWN_WALK = ("viscous_kernels.h", "velgrad_kernels.h")
# what only the walk does: the list blocks, the cell rows, the lane's route
WALK_TEXT = ("lr.block(", "list_block_entries(", "row_ranges(", "scalar_lane_route(")

SIGNATURES = {
    "scalar_kernels.h": """template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_scalars_step(const float4* __restrict__ posm, const float4* __restrict__ velp, const float4* __restrict__ Ts,
               const float* __restrict__ Vs, const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
               const int32_t* __restrict__ meta, CellGrid g, float h2, ScalarStep st, const TileDesc* __restrict__ desc,
               const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
               int force_rows, float4* __restrict__ T, int n_rows)
{""",
    "monitor_kernels.h": """template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_monitor_pairs(const float4* __restrict__ posm, const float* __restrict__ Vs, const int32_t* __restrict__ ncount,
                const uint32_t* __restrict__ cell_start, const int32_t* __restrict__ meta, CellGrid g, PairConsts k,
                const TileDesc* __restrict__ desc, const uint32_t* __restrict__ nlist,
                const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled, int force_rows,
                MonitorPairAcc* __restrict__ part)
{""",
    "cohesion_kernels.h": """template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_cohesion_apply(const float4* __restrict__ posm, const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
                 const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float gamma, const TileDesc* __restrict__ desc,
                 const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
                 float4* __restrict__ acc)
{""",
    "xsph_kernels.h": """template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_xsph_apply(const float4* __restrict__ posm, const float4* __restrict__ R, const int32_t* __restrict__ ncount,
             const uint32_t* __restrict__ cell_start, const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float eps,
             const TileDesc* __restrict__ desc, const uint32_t* __restrict__ nlist,
             const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled, float4* __restrict__ velp)
{""",
    "viscous_kernels.h": """template <bool UNIT_SCALE, bool WIDE, bool LAW>
__global__ void __launch_bounds__(TILE_THREADS)
k_viscous_apply(const float4* __restrict__ posm, const float4* __restrict__ R, const float* __restrict__ M,
                const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
                const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float mu, const TileDesc* __restrict__ desc,
                const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
                float4* __restrict__ acc)
{""",
    "velgrad_kernels.h": """template <bool UNIT_SCALE>
__global__ void __launch_bounds__(TILE_THREADS)
k_velgrad_particles(const float4* __restrict__ posm, const float4* __restrict__ velp, const uint32_t* __restrict__ cell_start,
                    const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float4* __restrict__ rowA,
                    float4* __restrict__ rowB)
{""",
}


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def code_of(text):
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_the_header_is_a_dependency_of_the_build():
    from smoothed_particle_hydrodynamics_amd import build
    assert "pair_walk.h" in build.HEADERS
    assert os.path.exists(os.path.join(CSRC, "pair_walk.h"))


def test_the_walk_lives_in_one_place():
    walk = read("pair_walk.h")
    for text in WALK_TEXT:
        assert text in code_of(walk), text
    for name in SHARED:
        mine = read(name)
        assert '#include "pair_walk.h"' in mine, name
        for text in WALK_TEXT:
            assert text not in mine, (name, text)
        assert not re.search(r"\w+_from_(lists|rows)\b", mine), name
        assert "pair_workgroup(meta, tiled, " in mine and "pair_walk<UNIT_SCALE, WIDE>(" in mine, name
    # the two that keep a copy: each points at the header and at why
    for name in OWN_WALK:
        mine = read(name)
        assert "pair_walk.h" in mine and "DESIGN.md: the pair walk" in mine, name
        assert "row_ranges(" in code_of(mine), name
    # one TileDesc in LDS per kernel, declared by the kernel; the header itself declares nothing there
    assert "__shared__" not in code_of(walk)
    for name in SHARED + ("viscous_kernels.h",):
        assert read(name).count("__shared__ TileDesc sd;") == 1, name
    assert "__shared__" not in read("velgrad_kernels.h")
    assert "atomic" not in code_of(walk)


def test_what_the_walk_keeps():
    """The pieces the passes were copied from, as they were: the next block requested before this block's gathers,
    the stand-in for a short last block, posm[q] in front of the payload, eight gathers then eight guarded adds;
    the row loop that is not unrolled, the self-skip and the membership test in front of the payload's gather."""
    code = code_of(read("pair_walk.h"))
    lists = code[code.index("void pair_walk_lists("):code.index("void pair_walk_rows(")]
    assert lists.index("list_block_entries(blk, entry);") < lists.index("blk = lr.block(min((j0 >> 3) + 1, lastb));") \
        < lists.index("pj[u] = posm[q];") < lists.index("pay[u] = a.gather(q);") \
        < lists.index("if (j0 + u < cnt) a.template add<UNIT_SCALE>(pi, pj[u], pay[u]);")
    assert "const uint32_t e = j0 + u < cnt ? entry[u] : entry[0];" in lists
    assert "const int q = ListEntry<WIDE>::tile(e) - ListEntry<WIDE>::shift(d, e);" in lists
    assert lists.count("#pragma unroll\n") == 2
    rows = code[code.index("void pair_walk_rows("):code.index("void pair_walk(")]
    assert "#pragma unroll 1\n   for (int row = 0; row < 9; row++)" in rows
    assert rows.index("if (q == (uint32_t)p) continue;") < rows.index("const float4 pj = posm[q];") \
        < rows.index("if (d2 < h2) a.template add<UNIT_SCALE>(pi, pj, a.gather(q));")
    # the routes are decided in one place each
    assert code.count("scalar_workgroup_route(") == 1 and code.count("scalar_lane_route(") == 1
    assert code.count("tile_desc_load(") == 1 and code.count("xcd_workgroup(blockIdx.x, gridDim.x)") == 1
    # a workgroup past the live range reads neither its flag nor its descriptor, and no lane returns inside the step
    step = code[code.index("PairLane pair_workgroup("):code.index("void pair_walk_lists(")]
    assert "(tiled && w.any) ? nlist_overflow[w.wg] : LISTS_NONE" in step
    assert "if (w.any && w.wg_route == SCALAR_ROUTE_LISTS) tile_desc_load(desc, w.wg, sd);" in step
    assert step.count("return") == 1 and "return w;" in step


def test_the_kernels_signatures_are_the_ones_the_launches_were_written_against():
    for name, sig in SIGNATURES.items():
        assert sig in read(name), name
    # k_monitor_pairs stores a partial for every workgroup of its grid: nothing returns before the fold
    mon = read("monitor_kernels.h")
    body = mon[mon.index("k_monitor_pairs(const float4*"):mon.index("// ---- the fold: one workgroup")]
    assert "return" not in code_of(body) and "if (w.tid == 0) part[blockIdx.x] = a;" in body
    # the other three return as whole lanes behind the workgroup step
    for name in ("scalar_kernels.h", "cohesion_kernels.h", "xsph_kernels.h"):
        assert "desc, sd);\n   if (!w.live) return;" in read(name), name

// Host-computable geometry of the strip DP (sdp.h): strip and chunk counts, LDS sizes, the ONE description of the
// workspace (a table of sections, from which both its size and its carve come) and the launch plan.  Integer
// arithmetic, no HIP headers, so tests/sanitize/sdp_plan_driver.cpp runs it stand-alone; sdp.h includes it, and the
// functions the kernels call are __host__ __device__ there.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define RTS_SDP_HD __host__ __device__
#else
#define RTS_SDP_HD
#endif

namespace rts {
namespace sdp {

constexpr int kSteps = 16;     // steps of a chunk = step codes of a packed word (sdp.h states it as kChunk)
constexpr int kYRec = 14;      // doubles per prepared column record: 12 features, norm, pad (112 bytes)
constexpr int kRing = 96;      // steps of the LDS cost ring: a helper runs one chunk ahead and a column spans 64 steps
constexpr int kStageLd = 65;   // leading dimension of the [16][64] output tiles
constexpr int kTiles = 3;      // output tiles per strip: written in chunk m, read in chunks m+1 and m+2
constexpr int kBtChunks = 8;   // chunks of a strip the backtrack stages in LDS at once (sdp.h, walk_strip)

RTS_SDP_HD inline int n_strips(int M) { return (M + 63) / 64; }
RTS_SDP_HD inline int n_chunks(int N) { return (N + 63 + kSteps - 1) / kSteps; }  // per strip
RTS_SDP_HD inline size_t lds_core_bytes(int NS) {
    return sizeof(double) * (size_t)NS * ((size_t)kRing * 64 + (size_t)kTiles * kSteps * kStageLd + 2 * kSteps * kYRec + 64 + 2 * kSteps);
}
// + 16 bytes behind the strips' buffers: the workgroup's current ticket (for_each_rowgroup).  All of it is dynamic LDS --
// the kernels declare no static LDS, so that the dynamic limit can be raised to the full 160 KB.
RTS_SDP_HD inline size_t lds_bytes(int NS) { return lds_core_bytes(NS) + 16; }
RTS_SDP_HD inline size_t codes_words(int M, int N) { return (size_t)n_strips(M) * n_chunks(N) * 64; }
RTS_SDP_HD inline size_t scratch_pairs(int M, int N) { return (size_t)64 * n_strips(M) + N; }  // sdp.h, path_segment
RTS_SDP_HD inline size_t tail_lds_bytes(int S) { return sizeof(uint32_t) * 2 * kBtChunks * 64 * (size_t)S; }  // path_tail

// ---- the workspace -----------------------------------------------------------------------------------------------
// One allocation: a 256-byte header whose first word is `err` (the kernels' fault flag; the 16 bytes the host clears),
// then the sections of the table in workspace_layout(), each rounded up to 256 bytes.  A problem (a DTW pair, a WTW
// stream's window) of at most M_cap x N_cap cells owns slice [problem] of every section.
constexpr size_t kWsHeader = 256;
enum Section { kBnd, kEntb, kCross, kLens, kYrecs, kCodes, kScratch, kTicket, kSections };
struct WorkspaceLayout {
    size_t off[kSections], len[kSections], total;  // byte offset from the base, bytes in use (the section ends 256-aligned)
};
inline WorkspaceLayout workspace_layout(int M_cap, int N_cap, int B) {
    const size_t S = (size_t)n_strips(M_cap), N = (size_t)N_cap;
    const size_t table[kSections][2] = {
        // bytes per element, elements per problem
        {sizeof(unsigned long long), S * N},               // kBnd     [n_strips][N] rows handed between row groups
        {sizeof(int32_t), S * N},                          // kEntb    [n_strips][N] entry columns of the bottom rows
        {sizeof(int32_t), S},                              // kCross   [n_strips] strip-boundary crossings of the path
        {sizeof(int32_t), S},                              // kLens    [n_strips] lengths of the path's segments
        {sizeof(double), N * kYRec},                       // kYrecs   [N][kYRec] prepared column records
        {sizeof(uint32_t), codes_words(M_cap, N_cap)},     // kCodes   packed step codes
        {2 * sizeof(int32_t), scratch_pairs(M_cap, N_cap)},  // kScratch path segments as walked, (i, j) pairs
        {sizeof(int32_t), 1},                              // kTicket  next row group (for_each_rowgroup)
    };
    WorkspaceLayout w;
    w.total = kWsHeader;
    for (int s = 0; s < kSections; s++) {
        w.off[s] = w.total;
        w.len[s] = table[s][0] * table[s][1] * (size_t)B;
        w.total += (w.len[s] + 255) & ~(size_t)255;
    }
    return w;
}
inline size_t workspace_bytes(int M_cap, int N_cap, int B) { return workspace_layout(M_cap, N_cap, B).total; }
// The carve: points the workspace fields of an argument struct (DtwArgs and WtwArgs name them alike: err, bnd, entb,
// cross, lens, yrec, codes, ticket) and `*scratch` into the workspace at `base`; returns the layout it walked.
template <class Args>
inline WorkspaceLayout workspace_carve(void *base, int M_cap, int N_cap, int B, Args *g, int32_t **scratch) {
    const WorkspaceLayout w = workspace_layout(M_cap, N_cap, B);
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    g->err = reinterpret_cast<int32_t *>(p);
    g->bnd = reinterpret_cast<unsigned long long *>(p + w.off[kBnd]);
    g->entb = reinterpret_cast<int32_t *>(p + w.off[kEntb]);
    g->cross = reinterpret_cast<int32_t *>(p + w.off[kCross]);
    g->lens = reinterpret_cast<int32_t *>(p + w.off[kLens]);
    g->yrec = reinterpret_cast<double *>(p + w.off[kYrecs]);
    g->codes = reinterpret_cast<uint32_t *>(p + w.off[kCodes]);
    *scratch = reinterpret_cast<int32_t *>(p + w.off[kScratch]);
    g->ticket = reinterpret_cast<int32_t *>(p + w.off[kTicket]);
    return w;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------
// Strips per workgroup / helper waves per strip / workgroups of one problem's pipeline.  One strip per workgroup
// (3 helpers; the DP wave, which sets the pace, has a SIMD to itself; 77 KB of LDS, so two workgroups share a CU) when
// every strip of every problem can have a resident workgroup of its own; otherwise two strips per workgroup (2 helpers
// each), which halves the number of passes a workgroup makes over the columns.
//
// Residency.  A problem's row groups wait for one another inside the launch (run_rowgroup polls the bottom row of the
// row group above).  That is deadlock-free WHATEVER the residency, because row groups are not bound to workgroups:
// a workgroup takes the next row group of its problem from a ticket counter when it starts and whenever it finishes
// one (for_each_rowgroup), so row group r - 1 was always taken by a workgroup that is already running -- by induction it
// finishes, and r with it.  `resident1` / `resident2` (workgroups of the one-strip / two-strip kernel the device holds
// at once: compute units x hipOccupancyMaxActiveBlocksPerMultiprocessor, queried by the caller for the instantiation
// it launches) only size the grid: workgroups beyond residency would just queue behind the running ones.
// RTS_SDP_CONFIG=1|2 forces the strips per workgroup, RTS_SDP_GRID=n the workgroups per problem (tuning and tests;
// results do not depend on either).
inline int helpers(int NS) { return NS == 1 ? 3 : 2; }
inline int block_threads(int NS) { return 64 * NS * (1 + helpers(NS)); }  // NS strips of one DP wave and H helpers each
struct Plan {
    int NS, H, n_rg;  // strips per workgroup, helper waves per strip, row groups of a problem of `strips` strips
    int grid, block;  // workgroups per problem, threads per workgroup
    size_t smem;      // dynamic LDS per workgroup, the test knob's padding included
};
inline Plan pick_config(int strips, int B, int resident1, int resident2, size_t pad) {
    Plan p;
    if (resident1 < 1) resident1 = 1;
    if (resident2 < 1) resident2 = 1;
    p.NS = ((long long)strips * B <= resident1) ? 1 : 2;
    if (const char *e = getenv("RTS_SDP_CONFIG")) p.NS = (atoi(e) == 1) ? 1 : 2;
    if (p.NS > strips) p.NS = strips;
    p.H = helpers(p.NS);
    p.n_rg = (strips + p.NS - 1) / p.NS;
    const int resident = (p.NS == 1) ? resident1 : resident2;
    p.grid = resident / B;
    if (p.grid < 1) p.grid = 1;
    if (p.grid > p.n_rg) p.grid = p.n_rg;
    if (const char *e = getenv("RTS_SDP_GRID")) p.grid = atoi(e) > 0 ? atoi(e) : p.grid;
    p.block = block_threads(p.NS);
    p.smem = lds_bytes(p.NS) + pad;
    return p;
}
// Test knob: extra bytes of dynamic LDS per workgroup (lowers the residency the occupancy query reports and the
// hardware grants, e.g. 80000 -> one workgroup per CU); 0 in production.
inline size_t lds_pad() {
    const char *e = getenv("RTS_SDP_LDS_PAD");
    const long v = e ? atol(e) : 0;
    return v > 0 && v < 80 * 1024 ? (size_t)v : 0;
}

}  // namespace sdp
}  // namespace rts

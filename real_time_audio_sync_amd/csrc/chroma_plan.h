// Everything about a chroma launch (chroma.hip) that the host can compute: which kernel runs, the ONE statement of each
// kernel's LDS layout (the kernels carve their dynamic LDS from the functions create sizes it from) and the grid.
// Integer arithmetic, no HIP headers, so tests/sanitize/chroma_plan_driver.cpp runs it stand-alone.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define RTS_CH_HD __host__ __device__
#else
#define RTS_CH_HD
#endif

namespace rts {

constexpr int kCh = 12;         // pitch classes
constexpr int kChromaNT = 256;  // threads of a team: one frame's FFT and projection

namespace chroma_plan {

// ---- which kernel ----------------------------------------------------------------------------------------------------
// fft_len 4096 whose sample indices fit 32 bits: the specialised kernel (`span`: n_samples of a single call,
// sample_stride of a batched one).  fft_len 8192: the big kernel.  Anything else: the generic one.  kProject is
// rts_chroma_project's kernel, no flavour of the others: listed so that every launch goes through one table.
enum Kernel { kGeneric, k4096, kBig, kProject, kKernels };
inline Kernel flavour(int L, int hop, long long span, int n_frames) {
    if (L == 4096 && span + 2LL * L + (long long)n_frames * hop < 0x7fffffffLL) return k4096;
    return L > 4096 ? kBig : kGeneric;
}
// Teams of kChromaNT threads per workgroup (one frame in flight each), frames of a group (chroma.hip states them as
// kChromaFR and kBigFR), and the frames of a group that one team projects in a single pass over the filterbank
// (project_normalize's kProjMax).
RTS_CH_HD constexpr int teams(Kernel k) { return k == kGeneric || k == k4096 ? 2 : 1; }
RTS_CH_HD constexpr int group(Kernel k) { return k == kBig ? 2 : 4; }
RTS_CH_HD constexpr int proj_frames(Kernel k) { return group(k) / teams(k); }

// ---- LDS -------------------------------------------------------------------------------------------------------------
// A workgroup's dynamic LDS: four sections one behind the other, each starting on a 16-byte slot (one double2).
//   z    [teams][z_team] double2   FFT work buffer of each team
//   tw   [tw_slots] double2        quarter-circle twiddles exp(-2 pi i n / L), n < L/4
//   spec [frames][sstride] double  power spectra of a group, L/2 + 1 bins each (frames and sstride are even)
//   red  [teams][red_team] double  project_normalize's scratch: the [12][16] row totals of each frame a team projects
//                                  in one pass.  A team's FFT buffer is free by then, so the scratch lives there
//                                  (red_in_z) when the buffer is at least that large; otherwise behind the spectra.
// The kernels chain their pointers through the sections from these shapes (chroma.hip, lds_carve); the offsets and the
// total, in slots, are the same walk for the host.
struct Lds {
    int teams, z_team, tw_slots, frames, sstride, red_team;  // the shapes above
    RTS_CH_HD constexpr bool red_in_z() const { return 2 * z_team >= red_team; }
    // slots from the base: team t's FFT buffer, the twiddles, the spectra, team t's scratch, the end
    RTS_CH_HD constexpr int z(int t) const { return t * z_team; }
    RTS_CH_HD constexpr int tw() const { return teams * z_team; }
    RTS_CH_HD constexpr int spec() const { return tw() + tw_slots; }
    RTS_CH_HD constexpr int red(int t) const { return red_in_z() ? z(t) : spec() + (frames * sstride + t * red_team) / 2; }
    RTS_CH_HD constexpr int total() const { return red_in_z() ? spec() + frames * sstride / 2 : red(teams); }
    RTS_CH_HD constexpr size_t bytes() const { return (size_t)16 * total(); }
};
RTS_CH_HD constexpr Lds lds_sections(int teams, int z_slots, int tw_slots, int frames, int sstride) {
    return Lds{teams, z_slots, tw_slots, frames, sstride, frames / teams * kCh * 16};
}
// fft_len 4096, specialised: the work buffer is padded by one slot per 8 (chroma.hip, c4k::zi)
constexpr int k4096Slots = 2048 + 2048 / 8;
RTS_CH_HD constexpr Lds lds_layout(Kernel k, int L) {
    const int N2 = L / 2;  // packed complex points of a frame; L/2 + 1 rfft bins
    return k == kGeneric ? lds_sections(teams(k), N2, N2 / 2, group(k), N2 + 2)
           : k == k4096  ? lds_sections(teams(k), k4096Slots, 1024, group(k), 2048 + 2)
           : k == kBig   ? lds_sections(teams(k), N2, 0, group(k), N2 + 2)  // twiddles from the table in L2: no room
                         : lds_sections(teams(k), 0, 0, group(k), N2 + 2);
}

// ---- grid ------------------------------------------------------------------------------------------------------------
// Workgroups are persistent over groups of frames.  Single launches: one workgroup per compute unit (155 KB of LDS each
// at fft_len 4096; 41.7 M frames/s against 40.7 M with four short-lived ones per CU, each loading the twiddle table and
// its window registers first), four of the big kernel's one-team workgroups; batched launches (gridDim.y = streams):
// at most 64 per stream; project: at most 1024.
constexpr int kBatchGrid = 64, kProjectGrid = 1024;
inline int grid_x(Kernel k, int n_frames, int cus, bool batched) {
    const int groups = (n_frames + group(k) - 1) / group(k);
    const int cap = k == kProject ? kProjectGrid : batched ? kBatchGrid : k == kBig ? 4 * cus : cus;
    return groups < cap ? groups : cap;
}

}  // namespace chroma_plan
}  // namespace rts

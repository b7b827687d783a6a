// Device-side live ingestion for many microphones: the batched form of the reference's audio loops
//   livenote_live.py:161-209  receive_audio -> _process_input: while len(data) >= 4096: wav_to_chroma_col(data[:4096]);
//                              OnlineTimeWarping.insert(col); data = data[2048:]
//   wtw.py:71-93              WTW.insert: self.buf += list; while len(buf) >= fft_len: column of buf[:fft_len]; buf = buf[hop:]
// for B independent streams per call ("feed").  The host side of a feed (rts_live_submit) is plan, chain, commit.
//
// Plan (csrc/live_plan.h, no HIP in it).  The producer has written counts[B] and the packed new samples of all streams
// into a pinned staging slot (rts_live_staging hands the slot out, so it can write there directly).  Nothing is ever read
// back: the host mirrors the pending counts, the carry flags of diff mode and a resampling handle's input / output totals,
// and live_plan_feed derives from mirror and counts whether the feed is refused, the launch geometry (n_max and its
// kin) and the mirror after the feed, which it leaves in scratch.
//
// Chain (live_enqueue: ONE host-to-device copy and a fixed sequence of launches on the caller's stream, no synchronisation)
//   copy                  of the used part of the slot by one hipMemcpyAsync on the handle's copy stream; the compute
//                         stream waits for it by event, so the copy of feed k+1 overlaps the kernels of feed k (a ring
//                         of kSlots pinned + device slots)
//   resample_live_kernel  rts_live_create_resampled only (csrc/resample.hip): the staged samples are at the microphones' own
//                         rate; (carried tail + staged samples) of every stream are resampled into a second device
//                         buffer laid out like a staging slot, which the append below reads instead of the slot
//   live_append_kernel    per stream (16 slices each): append the new samples (float32, or PCM16 scaled by 1/32768 like librosa.load)
//                         behind the pending ones in a per-stream device buffer; pending -> n_samples, complete hops ->
//                         n_frames  ((pending - fft_len) / hop + 1 once pending >= fft_len).
//   rts_chroma_frames_batch   un-padded framing of every stream's pending samples -> chroma columns [B][n_max][12]
//   live_diff_kernel      RTS_FEATURE_CHROMA_DIFF only: the columns become max(chroma[m+1] - chroma[m], 0)
//                         (np.clip(np.diff(chroma), 0, inf), chroma.py:85-90) in a second buffer; the last chroma
//                         column of every stream is carried on the device from feed to feed
//   live_level_kernel, live_gate_kernel   only after rts_live_gate(min_level > 0) (csrc/live_gate.h): the mean square of
//                         every column's frame, then per stream the decision which columns its tracker gets, those
//                         packed into a second buffer with their counts, and the meter words of rts_live_levels into a
//                         host-mapped block of its own; the push below then takes that buffer and those counts
//   rts_otw_push | rts_wtw_push   the columns into the alignment state (insert semantics, column by column)
//   the publishers        (live_publishers_launch) each only after its enabling call, each into a host-mapped block of its own
//                         that a non-blocking reader copies out like rts_live_poll the status words:
//     rts_otw_path_cost     rts_live_watch(K > 0): the tracker's mean cell cost over its last K path points -- rts_live_confidence
//     annot_live_kernel     rts_live_annotate with tables (csrc/annot.hip): beat and label of the reference frame of every
//                           tracker's last path point -- rts_live_beats
//     tempo_tail_kernel     rts_live_follow_tempo(K > 0) (csrc/tempo.hip): slope, position and beats per minute of the last K
//                           points of every tracker's path -- rts_live_tempo
//     ensemble_fuse_kernel  rts_live_follow_consensus with an ensemble, while annotations are on (csrc/ensemble.hip): the median
//                           beat of every group of streams, each member's deviation, strikes and out -- rts_live_consensus
//     accomp_steer_kernel, rts_warp_run   rts_live_accompany with a plan (csrc/accomp.hip): the next anchor of every armed
//                           stream's time map from the tail of its tracker's path, and the blocks that made due rendered into
//                           this feed's chunk of a host-mapped ring, their words into a block that accomp.hip keeps --
//                           rts_live_accompaniment reads both
//   live_compact_kernel   drop hop * n_frames consumed samples per stream (data = data[2048:], livenote_live.py:208),
//                         and publish {status, live position, ref position, feed number} of every stream into
//                         host-mapped memory -- rts_live_poll reads those words without touching the stream.
//
// Commit (live_commit).  Once the last step has been enqueued the planned values become the mirror, and the slot ring
// and the feed counter move on.  A chain that fails part-way commits nothing and marks the handle failed -- the device
// may have run a part of it -- and every feed and restart is refused until rts_live_reset has zeroed both sides.
//
// The host-mapped blocks.  ONE table (csrc/live_pub.h) says where every word of the status, gate, confidence, beats, tempo
// and consensus blocks lies and what an empty word holds; sizes, the kernels' and readers' pointers, the clears of
// allocation, rts_live_reset, live_restart_kernel and live_import_kernel all come from it.  A new publisher adds a table
// entry, an enabling call that ends in live_pub_alloc, a launch in live_publishers_launch and a reader made of live_word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "accomp_plan.h"
#include "common.h"
#include "live_plan.h"
#include "live_pub.h"

namespace rts {

constexpr int kLiveSlots = 4;
constexpr int kLiveF = 12;     // pitch classes of a column (96 B in float64)

struct LiveArgs {
    const unsigned char *stage;  // device copy of the staging slot: int32 counts[B], int32 offs[B], then samples at samples_off
    size_t samples_off;
    int sample_kind;             // RTS_F32 or RTS_I16
    float *buf;                  // [B][cap] pending samples
    int32_t *pending;            // [B]
    int32_t *n_samples, *n_frames;  // [B] inputs of rts_chroma_frames_batch
    int B, cap, L, hop;
    const int32_t *state;        // alignment state of the streams, state_len ints each
    int state_len, st_status, st_live, st_ref;
    int feed_no;                 // (with state and the st_* words in one 64-byte line of the kernel arguments: measured)
    PubSet pubs;                 // the host-mapped blocks (csrc/live_pub.h): status from create, the others when enabled
    // RTS_FEATURE_CHROMA_DIFF (all NULL in chroma mode)
    double *cols;                // [B][cols_stride][12] chroma columns of this feed
    double *dcols;               // [B][cols_stride][12] difference columns handed to the tracker
    double *carry;               // [B][12] last chroma column of every stream
    int32_t *has_carry, *n_cols; // [B]
    int cols_stride;             // rows per stream in cols / dcols: n_max of this feed
    int32_t *ens_state;          // strikes[B], out[B] of the bound ensemble (NULL while consensus is off): a restart or an
                                 // import clears the stream's
};

// Status and positions of stream b from the tracker's state into the status block: every feed, restart and import.
__device__ __forceinline__ void live_publish_status(const LiveArgs &g, int b) {
    const int32_t *st = g.state + (size_t)b * g.state_len;
    unsigned char *blk = g.pubs.dev[kPubStatus];
    *(volatile int32_t *)pub_ptr<kPubStatus, kStatusStatus>(blk, g.B, b) = st[g.st_status];
    *(volatile int32_t *)pub_ptr<kPubStatus, kStatusLive>(blk, g.B, b) = st[g.st_live];
    *(volatile int32_t *)pub_ptr<kPubStatus, kStatusRef>(blk, g.B, b) = st[g.st_ref];
}

__device__ __forceinline__ void live_publish(const LiveArgs &g, int b) {
    live_publish_status(g, b);
    __threadfence_system();
    // written last: a reader that sees feed k sees the three words of feed >= k
    *(volatile int32_t *)pub_ptr<kPubStatus, kStatusFeed>(g.pubs.dev[kPubStatus], g.B, b) = g.feed_no;
}

// A restarted or imported stream: the per-stream words of the allocated blocks among `blocks` (bit k: PubBlock k) hold
// their empty values until the next feed.
__device__ __forceinline__ void live_clear_published(const PubSet &s, unsigned blocks, int B, int b) {
    RTS_PUB_UNROLL
    for (int k = 0; k < kPubBlocks; k++)
        if ((blocks >> k & 1) && s.dev[k]) pub_clear_stream((PubBlock)k, s.dev[k], B, b);
}

constexpr int kAppendSlices = 16;  // workgroups per stream in the append kernel (a 1-second buffer is 88 KB)

// grid (B, kAppendSlices): slice y of stream b copies its share of the new samples behind the pending ones.  `pending`
// is only read here (every slice needs the same base); the compact kernel, which always follows, writes it.
__global__ void __launch_bounds__(256) live_append_kernel(LiveArgs g) {
    const int b = blockIdx.x;
    const int32_t *counts = reinterpret_cast<const int32_t *>(g.stage);
    const int32_t *offs = counts + g.B;
    const int p = g.pending[b];
    int n = counts[b];
    if (n < 0) n = 0;
    if (p + n > g.cap) n = g.cap - p;  // (the host refuses such a feed before it gets here)
    const long long off = offs[b];
    float *dst = g.buf + (size_t)b * g.cap + p;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int lo = blockIdx.y * per, hi = (lo + per < n) ? lo + per : n;
    if (g.sample_kind == RTS_F32) {
        const float *src = reinterpret_cast<const float *>(g.stage + g.samples_off) + off;
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) dst[i] = src[i];
    } else {
        const int16_t *src = reinterpret_cast<const int16_t *>(g.stage + g.samples_off) + off;
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) dst[i] = (float)src[i] * (1.0f / 32768.0f);  // exact
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const int q = p + n;
        g.n_samples[b] = q;
        g.n_frames[b] = q >= g.L ? (q - g.L) / g.hop + 1 : 0;
    }
}

// One workgroup per stream, after the tracker has taken the columns (or right after the append when no stream completed
// a hop): drops the consumed samples and publishes.
__global__ void __launch_bounds__(1024) live_compact_kernel(LiveArgs g) {
    const int b = blockIdx.x;
    const int p = g.n_samples[b];
    const int used = g.n_frames[b] * g.hop;
    // hop > fft_len: the last column's hop may reach past what is pending; `buf = buf[hop:]` then leaves an empty
    // list (wtw.py:83, livenote_live.py:208), and the next column starts at the next sample delivered
    const int rem = p > used ? p - used : 0;
    float *buf = g.buf + (size_t)b * g.cap;
    if (used > 0 && rem > 0) {
        // forward move of possibly overlapping ranges: every round reads its elements before any of them is written,
        // and a later round reads only above what earlier rounds wrote
        for (int base = 0; base < rem; base += blockDim.x) {
            const int i = base + threadIdx.x;
            const float v = i < rem ? buf[used + i] : 0.0f;
            __syncthreads();
            if (i < rem) buf[i] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        g.pending[b] = rem;
        live_publish(g, b);
    }
}

// RTS_FEATURE_CHROMA_DIFF, one workgroup per stream, between the chroma kernel and the tracker push.  With n =
// n_frames[b] new chroma columns: difference column i - skip = max(cols[i] - prev_i, 0), prev_i = cols[i - 1], or the
// carried column for i = 0; a stream without a carry (fresh, restarted, reset) skips i = 0, so its tracker gets its
// first frame with its second chroma column.  A NaN difference stays NaN, like chroma_diff_kernel.  Lanes run over the
// flat (column, pitch class) index: loads and stores are contiguous 8-byte accesses.  n_frames is left as it is (the
// compaction drops n_frames * hop samples); the tracker push takes n_cols.  Every lane reads the carry and its flag
// before the barrier, the new carry is written behind it.
__global__ void __launch_bounds__(256) live_diff_kernel(LiveArgs g) {
    const int b = blockIdx.x;
    int n = g.n_frames[b];
    if (n > g.cols_stride) n = g.cols_stride;  // (the host mirror sizes cols_stride as the largest n_frames)
    const int skip = g.has_carry[b] ? 0 : 1;
    const double *in = g.cols + (size_t)b * g.cols_stride * kLiveF;
    double *out = g.dcols + (size_t)b * g.cols_stride * kLiveF;
    double *carry = g.carry + (size_t)b * kLiveF;
    for (int e = skip * kLiveF + threadIdx.x; e < n * kLiveF; e += blockDim.x) {
        const double prev = e >= kLiveF ? in[e - kLiveF] : carry[e];
        const double d = in[e] - prev;
        out[e - skip * kLiveF] = d < 0.0 ? 0.0 : d;
    }
    __syncthreads();
    if (n > 0 && threadIdx.x < kLiveF) carry[threadIdx.x] = in[(n - 1) * kLiveF + threadIdx.x];
    if (threadIdx.x == 0) {
        g.n_cols[b] = n > skip ? n - skip : 0;
        if (n > 0) g.has_carry[b] = 1;
    }
}

}  // namespace rts

#include "live_gate.h"

namespace rts {

// rts_live_restart, after the bound tracker's own restart: the selected streams' pending samples are dropped and their
// status / position words republished from the (now fresh) tracker state.  The feed number is left alone: the words
// still reflect every feed submitted before the restart.  Every other block that exists holds the stream's empty words
// until the next feed (the gate's meter words among them), and the bound ensemble forgets the member's strikes.  In diff
// mode the carried chroma column goes with the samples, and once rts_live_gate has made its buffers (t.q != NULL) the
// stream's gate closes.
__global__ void live_restart_kernel(RestartSel sel, LiveArgs g, GateArgs t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sel.n) return;
    const int b = sel.idx[i];
    g.pending[b] = 0;
    if (g.has_carry) g.has_carry[b] = 0;
    live_publish_status(g, b);
    if (g.ens_state) g.ens_state[b] = g.ens_state[g.B + b] = 0;  // a fresh member: no strikes, heard again
    live_clear_published(g.pubs, kPubRestartBlocks, g.B, b);
    if (t.q) live_gate_restart(t, b);
    __threadfence_system();
}

}  // namespace rts

struct rts_live {
    rts_chroma *plan;
    rts_otw *otw;
    rts_wtw *wtw;
    rts::LiveGeom geo;   // B, fft_len, hop, max_pending, diff mode, the resampler's ratio and in_cap
    // what every launch takes, from create and the enabling calls; a feed adds stage, sample_kind, feed_no, cols_stride to a
    // copy.  Every kernel gets every field: none may take a NULL field for the mode (live_restart_kernel's tests are of buffers)
    rts::LiveArgs args;
    int cols_cap, device;
    unsigned char *stage_host[rts::kLiveSlots];  // pinned
    unsigned char *stage_dev[rts::kLiveSlots];
    hipEvent_t copied[rts::kLiveSlots], done[rts::kLiveSlots];
    int used[rts::kLiveSlots];
    int slot;            // the slot rts_live_staging handed out last (-1: none outstanding)
    int next;
    hipStream_t copy_stream;
    // the host mirror, and the plan of the feed being submitted with its scratch (the next mirror, rs_nout, offs): the arrays
    // follow the handle in its own allocation (kMirrorBytes per stream), whatever the mode
    rts::LiveMirror cur;
    rts::FeedPlan fp;
    int last_stride;     // rows per stream in the layout of the last submitted feed (rts_live_columns_view)
    // the host-mapped blocks as the host sees them, by PubBlock (csrc/live_pub.h has their layouts); NULL: never allocated.
    // args.pubs holds the same blocks as the device sees them
    unsigned char *pub_host[rts::kPubBlocks];
    int feeds;
    int failed;          // a feed's chain was enqueued in part: the mirror no longer describes the device (rts_live_reset)
    // rts_live_watch: K path points per stream (0 = off); the confidence block comes with the first rts_live_watch(K > 0)
    int watch_k;
    // rts_live_create_resampled (rs NULL otherwise): the plan, the input samples a stream carries (rs_T), the second
    // staging-layout device buffer the resampling launch writes and the append reads, tail [B][rs_T] and totals [B][2]
    // (input samples taken, output samples made) on the device
    rts_resample *rs;
    int rs_T;
    unsigned char *rs_stage;
    float *rs_tail;  // [2][B][rs_T]: the copy feed k reads and the one it writes, alternating (rs_cur)
    int rs_cur;
    long long *rs_tot;
    // rts_live_gate: on / off and what its two launches take; the buffers and the gate block come with the first
    // rts_live_gate(min_level > 0)
    int gate_on;
    rts::GateArgs gate;
    // rts_live_annotate: the tables in use (NULL = off) and the two [B] device tables, which come with the beats block in the
    // first call with tables
    rts_annot *annot;
    int32_t *ann_tables;  // piece[B] then frame0[B] on the device
    // rts_live_follow_tempo: K points per stream (0 = off) and how far ahead; the tempo block comes with the first call with K > 0
    int tempo_k;
    double tempo_ahead;
    // rts_live_follow_consensus: the ensemble in use (NULL = off) and the groups of the one bound last; the consensus block,
    // whose group words use the first n_groups entries of theirs, comes with the first call with an ensemble
    rts_ensemble *ens;
    int ens_groups;
    // rts_live_accompany: on / off, and everything it owns (csrc/accomp.hip), made by the first call with a plan: the streams'
    // steering state on the device, a host-mapped block of its own and the ring of chunks
    int acc_on;
    rts::Accomp *acc;
};

namespace rts {

constexpr size_t kMirrorBytes = 6 * sizeof(long long) + 2 * sizeof(int32_t) + 2;  // per stream: two mirrors, rs_nout, offs

static int live_usable(const rts_live *h) {
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (h->failed)
        return set_error(RTS_ERR_INVALID, "an earlier feed failed while it was being enqueued: the handle needs rts_live_reset");
    return RTS_OK;
}

// Stream b's word of plane P of block K as the host reads it.
template <PubBlock K, int P>
static auto live_word(const rts_live *h, int b) {
    auto *p = pub_ptr<K, P>(h->pub_host[K], h->geo.B, b);
    return *const_cast<const volatile std::remove_pointer_t<decltype(p)> *>(p);
}

// Block k of the handle: nothing to do if it exists; else, with the handle's device current, mapped coherent host memory of
// the table's size, every word empty, entered on both sides.  `who` names the public call in the one error message there is.
static int live_pub_alloc(rts_live *h, PubBlock k, const char *who) {
    if (h->pub_host[k]) return RTS_OK;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    void *host = nullptr, *dev = nullptr;
    if (hipError_t e = mapped_alloc(pub_block_bytes(k, h->geo.B), &host, &dev); e != hipSuccess)
        return set_error(RTS_ERR_HIP, "%s: host-mapped block %d: %s", who, (int)k, hipGetErrorString(e));
    pub_clear_all(k, host, h->geo.B);
    h->pub_host[k] = static_cast<unsigned char *>(host);
    h->args.pubs.dev[k] = static_cast<unsigned char *>(dev);
    return RTS_OK;
}

// The tracker as the publishers' kernels see it (state, path, reference lengths), fetched on every use and never kept in
// the handle: nothing here rests on which of those pointers a restart may move.  Returns the tracker's longest reference.
static int live_tracker_view(const rts_live *h, TempoTail *t) {
    *t = TempoTail{};
    return h->otw ? otw_tempo_view(h->otw, t) : wtw_tempo_view(h->wtw, t);
}

// The publishers of a feed, between the tracker push and live_compact_kernel: each reads what the push left in the tracker
// and writes its own host-mapped block, and the compaction writes the feed number last, so a reader that sees feed k sees
// every block's words of a feed >= k.  The order is watch (rts_otw_path_cost), beats, tempo, consensus, accompaniment (the
// steering launch and one rts_warp_run; in the first feed after streams were armed also the launch that arms them); each is
// skipped while it is off.  Tempo and consensus need the piece / frame0 tables of rts_live_annotate: the tempo launch
// publishes NaN beats per minute without them or while annotations are off, the consensus launch is skipped while
// annotations are off (rts_live_follow_consensus refuses a session that never had them).
static int live_publishers_launch(rts_live *h, int feed_no, hipStream_t s) {
    const int B = h->geo.B;
    const PubSet &d = h->args.pubs;
    const int32_t *piece = h->ann_tables, *frame0 = piece ? piece + B : nullptr;
    TempoTail view;
    (void)live_tracker_view(h, &view);
    if (h->watch_k >= 1) {
        if (int rc = rts_otw_path_cost(h->otw, h->watch_k, pub_ptr<kPubConf, kConfMean>(d.dev[kPubConf], B),
                                       pub_ptr<kPubConf, kConfN>(d.dev[kPubConf], B), nullptr, s);
            rc != RTS_OK)
            return rc;
    }
    if (h->annot) {
        unsigned char *blk = d.dev[kPubBeats];
        const AnnotLive a = {view.state, view.state_len, view.st_n_path, view.path, view.path_cap, piece, frame0,
                             pub_ptr<kPubBeats, kBeatsBeat>(blk, B), pub_ptr<kPubBeats, kBeatsLabel>(blk, B),
                             pub_ptr<kPubBeats, kBeatsRef>(blk, B), B};
        if (int rc = annot_live_enqueue(h->annot, a, s); rc != RTS_OK) return rc;
    }
    if (h->tempo_k >= 1) {
        unsigned char *blk = d.dev[kPubTempo];
        TempoTail t = view;
        t.K = h->tempo_k;
        t.ahead = h->tempo_ahead;
        t.slope = pub_ptr<kPubTempo, kTempoSlope>(blk, B);
        t.pos = pub_ptr<kPubTempo, kTempoPos>(blk, B);
        t.bpm = pub_ptr<kPubTempo, kTempoBpm>(blk, B);
        t.n_out = pub_ptr<kPubTempo, kTempoN>(blk, B);
        t.piece = piece;
        t.frame0 = frame0;
        if (int rc = tempo_tail_enqueue(t, h->annot, s); rc != RTS_OK) return rc;
    }
    if (h->ens && h->annot) {
        unsigned char *blk = d.dev[kPubEns];
        const EnsembleOut o = {pub_ptr<kPubEns, kEnsConsensus>(blk, B), pub_ptr<kPubEns, kEnsSpread>(blk, B),
                               pub_ptr<kPubEns, kEnsNIn>(blk, B),       pub_ptr<kPubEns, kEnsNValid>(blk, B),
                               pub_ptr<kPubEns, kEnsDev>(blk, B),       pub_ptr<kPubEns, kEnsStrikes>(blk, B),
                               pub_ptr<kPubEns, kEnsOut>(blk, B)};
        if (int rc = ensemble_fuse_enqueue(h->ens, h->annot, view, piece, frame0, o, s); rc != RTS_OK) return rc;
    }
    if (h->acc_on) return accomp_enqueue(h->acc, view, h->args.n_samples, h->args.pending, feed_no, s);
    return RTS_OK;
}

// With the gate on, two more launches per feed between the chroma (and difference) step and the tracker push, in a feed
// without a column the second alone (it writes the feed's zero counts).  `g` is the feed's copy of the arguments.
static int live_gate_launch(rts_live *h, const LiveArgs &g, int n_max, hipStream_t s) {
    if (n_max > 0) {
        hipLaunchKernelGGL(live_level_kernel, dim3(n_max, h->geo.B), dim3(256), 0, s, g, h->gate);
        RTS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(live_gate_kernel, dim3(h->geo.B), dim3(256), 0, s, g, h->gate);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

static int live_refuse(const rts_live *h, LiveRefusal why, const FeedPlan &p, const int32_t *counts) {
    const int b = p.stream;
    if (why == kLiveNegativeCount) return set_error(RTS_ERR_INVALID, "stream %d: negative sample count", b);
    if (why == kLiveOverStaging)
        return set_error(RTS_ERR_INVALID, "stream %d: %d new input samples exceed the staging capacity of %lld per stream", b,
                         counts[b], h->geo.in_cap);
    if (h->rs)
        return set_error(RTS_ERR_INVALID, "stream %d: %lld pending + %lld resampled samples (of %d new input samples) "
                         "exceed max_pending = %d", b, h->cur.pending[b], p.n_new, counts[b], h->geo.cap);
    return set_error(RTS_ERR_INVALID, "stream %d: %lld pending + %d new samples exceed max_pending = %d", b,
                     h->cur.pending[b], counts[b], h->geo.cap);
}

// The chain of feed h->feeds + 1 from staging slot k, as `p` plans it.  Every feed enqueues every step, except: the
// resampling launch exists on a resampling handle only, live_diff_kernel in diff mode only (there in a feed without a
// chroma column too: it writes the feed's n_cols); rts_chroma_frames_batch and rts_otw_push return at once when their
// n_max is 0, rts_wtw_push after its entry check, which wtw.py:76-77 runs on every insert(), new column or not; in diff
// mode the tracker is pushed only when some stream hands it a column (n_max_diff > 0; the rows still lie n_max apart);
// the two gate launches follow rts_live_gate: with the gate on the push takes the gated buffer and its counts, and nothing
// else moves; live_publishers_launch has the launches behind the push.  The compaction and the publication end every feed.
static int live_enqueue(rts_live *h, const FeedPlan &p, int k, int sample_kind, void *stream) {
    const int B = h->geo.B;
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = h->args.samples_off + (size_t)p.total * (sample_kind == RTS_F32 ? sizeof(float) : sizeof(int16_t));
    RTS_HIP(hipMemcpyAsync(h->stage_dev[k], h->stage_host[k], bytes, hipMemcpyHostToDevice, h->copy_stream));
    RTS_HIP(hipEventRecord(h->copied[k], h->copy_stream));
    RTS_HIP(hipStreamWaitEvent(s, h->copied[k], 0));
    LiveArgs g = h->args;
    g.stage = h->stage_dev[k];
    g.sample_kind = sample_kind;
    g.feed_no = h->feeds + 1;
    g.cols_stride = p.n_max;
    if (h->rs) {  // input-rate samples: resampled into the second staging-layout buffer, which the chain goes on from
        const int cur = h->rs_cur, nxt = cur ^ 1;
        const size_t tail_n = (size_t)B * h->rs_T, tot_n = 2 * (size_t)B;
        if (int rc = resample_live_enqueue(h->rs, h->stage_dev[k], h->args.samples_off, sample_kind, B, h->geo.cap, h->rs_stage,
                                           h->rs_tail + cur * tail_n, h->rs_tot + cur * tot_n, h->rs_tail + nxt * tail_n,
                                           h->rs_tot + nxt * tot_n, p.n_out_max, s);
            rc != RTS_OK)
            return rc;
        g.stage = h->rs_stage;
        g.sample_kind = RTS_F32;
    }
    hipLaunchKernelGGL(live_append_kernel, dim3(B, kAppendSlices), dim3(256), 0, s, g);
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipEventRecord(h->done[k], s));  // the staging slot (host and device side) is free again after this point
    if (int rc = rts_chroma_frames_batch(h->plan, h->args.buf, RTS_F32, h->geo.cap, h->args.n_samples, 0, B, p.n_max, h->args.n_frames, 1,
                                         h->args.cols, RTS_F64, stream);
        rc != RTS_OK)
        return rc;
    if (h->geo.diff) {
        hipLaunchKernelGGL(live_diff_kernel, dim3(B), dim3(256), 0, s, g);
        RTS_HIP(hipGetLastError());
    }
    const double *cols = h->geo.diff ? h->args.dcols : h->args.cols;
    const int32_t *n_new = h->geo.diff ? h->args.n_cols : h->args.n_frames;
    if (h->gate_on) {
        if (int rc = live_gate_launch(h, g, p.n_max, s); rc != RTS_OK) return rc;
        cols = h->gate.gcols;
        n_new = h->gate.n_gated;
    }
    const int n_push = h->geo.diff && p.n_max_diff == 0 ? 0 : p.n_max;
    if (int rc = h->otw ? rts_otw_push(h->otw, cols, RTS_F64, n_push, n_new, stream)
                        : rts_wtw_push(h->wtw, cols, RTS_F64, n_push, n_new, 1, stream);
        rc != RTS_OK)
        return rc;
    if (int rc = live_publishers_launch(h, g.feed_no, s); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(live_compact_kernel, dim3(B), dim3(1024), 0, s, g);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

static void live_commit(rts_live *h, const FeedPlan &p, int k) {
    live_mirror_commit(h->geo, h->cur, p.next);
    if (h->rs) h->rs_cur ^= 1;
    h->feeds += 1;
    h->slot = -1;
    h->next = (k + 1) % kLiveSlots;
    h->used[k] = 1;
    h->last_stride = p.n_max;
}

// Every reader: `read(b)` under stream b's sequence word.  Returns the feeds whose results the
// words read reflect for every stream.
template <class Read>
static int live_read_published(const rts_live *h, Read read) {
    int fd = h->feeds;
    for (int b = 0; b < h->geo.B; b++) {
        const int seq = live_word<kPubStatus, kStatusFeed>(h, b);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        read(b);
        if (seq < fd) fd = seq;
    }
    return fd;
}

// hipMalloc of n zeroed elements, once everything before it has succeeded.
template <class T>
static hipError_t live_dev_zeroed(hipError_t e, T **p, size_t n) {
    if (e == hipSuccess) e = hipMalloc((void **)p, sizeof(T) * n);
    if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * n);
    return e;
}

}  // namespace rts

extern "C" {

int rts_live_destroy(rts_live *h) {
    if (!h) return RTS_OK;
    for (int k = 0; k < rts::kLiveSlots; k++) {
        if (h->stage_host[k]) (void)hipHostFree(h->stage_host[k]);
        if (h->stage_dev[k]) (void)hipFree(h->stage_dev[k]);
        if (h->copied[k]) (void)hipEventDestroy(h->copied[k]);
        if (h->done[k]) (void)hipEventDestroy(h->done[k]);
    }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    void *dev[] = {h->args.buf,   h->args.pending,   h->args.n_samples, h->args.n_frames, h->args.cols,    h->args.dcols,
                   h->args.carry, h->args.has_carry, h->args.n_cols,    h->rs_stage, h->rs_tail, h->rs_tot,
                   h->gate.lev,   h->gate.gcols,     h->gate.n_gated,   h->gate.q,   h->gate.prev, h->gate.seen,
                   h->gate.passed, h->gate.ord, h->ann_tables};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    for (unsigned char *p : h->pub_host)
        if (p) (void)hipHostFree(p);
    accomp_destroy(h->acc);
    free(h);  // the mirrors with it
    return RTS_OK;
}

int rts_live_create(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, rts_live **out) {
    return rts_live_create_features(plan, otw, wtw, B, max_pending, RTS_FEATURE_CHROMA, out);
}

// rts_live_create_features (rs NULL) and rts_live_create_resampled
static int live_create(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, int feature_kind,
                       rts_resample *rs, rts_live **out) {
    using namespace rts;
    if (feature_kind != RTS_FEATURE_CHROMA && feature_kind != RTS_FEATURE_CHROMA_DIFF)
        return set_error(RTS_ERR_INVALID, "feature_kind must be RTS_FEATURE_CHROMA or RTS_FEATURE_CHROMA_DIFF, not %d", feature_kind);
    if (feature_kind == RTS_FEATURE_CHROMA_DIFF && wtw)
        return set_error(RTS_ERR_UNSUPPORTED, "chroma-difference features with a WTW tracker: the reference never runs WTW on "
                                              "them, and its cosine cost is NaN on the zero columns they contain");
    if (!plan) return set_error(RTS_ERR_INVALID, "plan is NULL");
    if ((otw == nullptr) == (wtw == nullptr)) return set_error(RTS_ERR_INVALID, "exactly one of otw / wtw must be given");
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1");
    if ((otw ? otw_batch(otw) : wtw_batch(wtw)) != B)
        return set_error(RTS_ERR_INVALID, "the tracker was created for %d streams, not B = %d",
                         otw ? otw_batch(otw) : wtw_batch(wtw), B);
    LiveGeom geo = {B, 0, 0, max_pending, feature_kind == RTS_FEATURE_CHROMA_DIFF};  // no resampler so far
    if (int rc = rts_chroma_plan_info(plan, &geo.L, &geo.hop); rc != RTS_OK) return rc;
    if (max_pending < geo.L + geo.hop || (long long)max_pending * B > 0x7fffffffLL)
        return set_error(RTS_ERR_INVALID, "max_pending must be at least fft_len + hop samples (and B * max_pending < 2^31)");
    int rs_T = 0, rs_device = -1;
    if (rs) {
        (void)resample_info(rs, &geo.rs_L, &geo.rs_M, &geo.rs_half, &rs_T, &rs_device);
        if (int rc = check_device(rs_device, "resample_plan"); rc != RTS_OK) return rc;
        // the most input samples whose output fits max_pending: n_out >= n L / M - 1 once a stream's first output exists,
        // n_out >= (n L - half) / M before
        geo.in_cap = ((long long)(max_pending + 1) * geo.rs_M + geo.rs_L - 1) / geo.rs_L + rs_T + 2;
        if (geo.in_cap * B > 0x7fffffffLL)
            return set_error(RTS_ERR_INVALID, "max_pending: B * %lld input-rate samples per staging slot must stay below 2^31", geo.in_cap);
    }
    const size_t nB = (size_t)B;
    rts_live *h = (rts_live *)calloc(1, sizeof(rts_live) + kMirrorBytes * nB);
    if (!h) return set_error(RTS_ERR_INVALID, "out of host memory");
    h->plan = plan;
    h->otw = otw;
    h->wtw = wtw;
    h->geo = geo;
    h->args.B = B;
    h->args.cap = max_pending;
    h->args.L = geo.L;
    h->args.hop = geo.hop;
    h->cols_cap = (max_pending - geo.L) / geo.hop + 1;
    h->slot = -1;
    h->args.samples_off = (2 * sizeof(int32_t) * nB + 255) & ~(size_t)255;
    const size_t slot_bytes = h->args.samples_off + sizeof(float) * nB * (size_t)(rs ? geo.in_cap : max_pending);
    h->rs = rs;
    h->rs_T = rs_T;
    long long *ll = reinterpret_cast<long long *>(h + 1);  // 8-byte values first
    h->cur.pending = ll;
    h->cur.rs_tot = ll + nB;
    h->fp.next.pending = ll + 3 * nB;
    h->fp.next.rs_tot = ll + 4 * nB;
    h->fp.rs_nout = reinterpret_cast<int32_t *>(ll + 6 * nB);
    h->fp.offs = h->fp.rs_nout + nB;
    h->cur.has_carry = reinterpret_cast<uint8_t *>(h->fp.offs + nB);
    h->fp.next.has_carry = h->cur.has_carry + nB;
    hipError_t e = hipGetDevice(&h->device);
    for (int k = 0; k < kLiveSlots && e == hipSuccess; k++) {
        if ((e = hipHostMalloc((void **)&h->stage_host[k], slot_bytes, hipHostMallocDefault)) != hipSuccess) break;
        if ((e = hipMalloc((void **)&h->stage_dev[k], slot_bytes)) != hipSuccess) break;
        if ((e = hipEventCreateWithFlags(&h->copied[k], hipEventDisableTiming)) != hipSuccess) break;
        if ((e = hipEventCreateWithFlags(&h->done[k], hipEventDisableTiming)) != hipSuccess) break;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    e = live_dev_zeroed(e, &h->args.buf, nB * max_pending);
    e = live_dev_zeroed(e, &h->args.pending, nB);
    e = live_dev_zeroed(e, &h->args.n_frames, nB);
    if (e == hipSuccess) e = hipMalloc((void **)&h->args.n_samples, sizeof(int32_t) * nB);  // written by every feed before it is read
    if (e == hipSuccess) e = hipMalloc((void **)&h->args.cols, sizeof(double) * 12 * nB * h->cols_cap);
    if (geo.diff) {
        if (e == hipSuccess) e = hipMalloc((void **)&h->args.dcols, sizeof(double) * 12 * nB * h->cols_cap);
        e = live_dev_zeroed(e, &h->args.carry, 12 * nB);
        e = live_dev_zeroed(e, &h->args.has_carry, nB);
        e = live_dev_zeroed(e, &h->args.n_cols, nB);
    }
    if (rs) {
        e = live_dev_zeroed(e, &h->rs_stage, h->args.samples_off + sizeof(float) * nB * max_pending);
        e = live_dev_zeroed(e, &h->rs_tail, 2 * nB * rs_T);
        e = live_dev_zeroed(e, &h->rs_tot, 4 * nB);
    }
    if (e != hipSuccess) {
        rts_live_destroy(h);
        return set_error(RTS_ERR_HIP, "rts_live_create: %s", hipGetErrorString(e));
    }
    if (int rc = live_pub_alloc(h, kPubStatus, "rts_live_create"); rc != RTS_OK) {
        rts_live_destroy(h);
        return rc;
    }
    int32_t *st = nullptr;
    const int rc = otw ? rts_otw_device_views(otw, nullptr, nullptr, &st) : rts_wtw_state_view(wtw, &st);
    h->args.state = st;
    h->args.state_len = otw ? RTS_STATE_LEN : RTS_WTW_STATE_LEN;
    h->args.st_status = otw ? RTS_ST_STATUS : RTS_WTW_ST_STATUS;
    h->args.st_live = otw ? RTS_ST_T : RTS_WTW_ST_LIVE_PTR;
    h->args.st_ref = otw ? RTS_ST_J : RTS_WTW_ST_REF_PTR;
    if (rc != RTS_OK) {
        rts_live_destroy(h);
        return rc;
    }
    *out = h;
    return RTS_OK;
}

int rts_live_create_features(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, int feature_kind,
                             rts_live **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    return live_create(plan, otw, wtw, B, max_pending, feature_kind, nullptr, out);
}

int rts_live_create_resampled(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, int feature_kind,
                              rts_resample *resample_plan, rts_live **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!resample_plan)
        return set_error(RTS_ERR_INVALID, "resample_plan is NULL (equal rates build no resampler: rts_live_create_features)");
    return live_create(plan, otw, wtw, B, max_pending, feature_kind, resample_plan, out);
}

int rts_live_reset(rts_live *h, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    const size_t nB = (size_t)h->geo.B;
    RTS_HIP(hipStreamSynchronize((hipStream_t)stream));
    RTS_HIP(hipStreamSynchronize(h->copy_stream));
    RTS_HIP(hipMemsetAsync(h->args.pending, 0, sizeof(int32_t) * nB, (hipStream_t)stream));
    if (h->args.has_carry) RTS_HIP(hipMemsetAsync(h->args.has_carry, 0, sizeof(int32_t) * nB, (hipStream_t)stream));
    if (h->rs) {
        RTS_HIP(hipMemsetAsync(h->rs_tail, 0, sizeof(float) * 2 * nB * h->rs_T, (hipStream_t)stream));
        RTS_HIP(hipMemsetAsync(h->rs_tot, 0, sizeof(long long) * 4 * nB, (hipStream_t)stream));
    }
    if (h->gate.q) {  // every stream closed and at ordinal 0 again; the setting stays
        RTS_HIP(hipMemsetD32Async((hipDeviceptr_t)h->gate.q, kGateClosed, nB, (hipStream_t)stream));
        for (int32_t *w : {h->gate.prev, h->gate.seen, h->gate.passed})
            RTS_HIP(hipMemsetAsync(w, 0, sizeof(int32_t) * nB, (hipStream_t)stream));
    }
    memset(h + 1, 0, kMirrorBytes * nB);
    for (int k = 0; k < kPubBlocks; k++)  // every block that exists: every word empty, the group words too
        if (h->pub_host[k]) pub_clear_all((PubBlock)k, h->pub_host[k], h->geo.B);
    if (h->ens) {
        if (int rc = rts_ensemble_reset(h->ens, nullptr, stream); rc != RTS_OK) return rc;
    }
    if (h->acc) {  // every stream disarmed; on / off stays
        if (int rc = accomp_reset(h->acc, (hipStream_t)stream); rc != RTS_OK) return rc;
    }
    memset(h->used, 0, sizeof(h->used));
    h->slot = -1;
    h->feeds = 0;
    h->last_stride = 0;
    const int rc = h->otw ? rts_otw_reset(h->otw, stream) : rts_wtw_reset(h->wtw, stream);
    if (rc == RTS_OK) h->failed = 0;  // everything a half-enqueued chain may have touched is as at create again
    return rc;
}

int rts_live_restart(rts_live *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                     void *stream) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (!mask_host) return set_error(RTS_ERR_INVALID, "mask_host is NULL");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    // the tracker makes every check before it enqueues anything; behind the feeds already submitted on `stream`
    if (int rc = h->otw ? rts_otw_restart(h->otw, mask_host, first_host, len_host, stream)
                        : rts_wtw_restart(h->wtw, mask_host, first_host, len_host, stream);
        rc != RTS_OK)
        return rc;
    RestartSel sel;
    for (int pos = 0; restart_next_chunk(h->geo.B, mask_host, nullptr, nullptr, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(live_restart_kernel, dim3((sel.n + 63) / 64), dim3(64), 0, (hipStream_t)stream, sel, h->args, h->gate);
        RTS_HIP(hipGetLastError());
        if (h->rs) {
            if (int rc = resample_live_restart_enqueue(h->rs, sel, h->geo.B, h->rs_tail, h->rs_tot, (hipStream_t)stream); rc != RTS_OK)
                return rc;
        }
        if (h->acc) {  // a restarted stream is disarmed until rts_live_accompany arms it again
            if (int rc = accomp_restart(h->acc, sel, (hipStream_t)stream); rc != RTS_OK) return rc;
        }
    }
    for (int b = 0; b < h->geo.B; b++)
        if (mask_host[b]) {  // the mirror: samples submitted from here on belong to the new run
            h->cur.pending[b] = 0;
            h->cur.has_carry[b] = 0;
            h->cur.rs_tot[2 * b] = h->cur.rs_tot[2 * b + 1] = 0;
        }
    return RTS_OK;
}

int rts_live_staging(rts_live *h, int32_t **counts_host, void **samples_host, long long *capacity_samples) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (h->slot < 0) {
        const int k = h->next;
        if (h->used[k]) RTS_HIP(hipEventSynchronize(h->done[k]));  // the feed that used this slot kSlots feeds ago
        h->used[k] = 0;
        h->slot = k;
    }
    if (counts_host) *counts_host = reinterpret_cast<int32_t *>(h->stage_host[h->slot]);
    if (samples_host) *samples_host = h->stage_host[h->slot] + h->args.samples_off;
    if (capacity_samples) *capacity_samples = (long long)h->geo.B * (h->rs ? h->geo.in_cap : h->geo.cap);
    return RTS_OK;
}

int rts_live_submit(rts_live *h, int sample_kind, void *stream) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (h->slot < 0) return set_error(RTS_ERR_INVALID, "rts_live_submit without rts_live_staging");
    if (sample_kind != RTS_F32 && sample_kind != RTS_I16) return set_error(RTS_ERR_INVALID, "samples must be RTS_F32 or RTS_I16");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    const int k = h->slot;
    int32_t *counts = reinterpret_cast<int32_t *>(h->stage_host[k]);
    const FeedPlan &p = h->fp;
    if (const LiveRefusal why = live_plan_feed(h->geo, h->cur, counts, &h->fp); why != kLiveFeedOk)
        return live_refuse(h, why, p, counts);
    memcpy(counts + h->geo.B, p.offs, sizeof(int32_t) * (size_t)h->geo.B);  // the second table of the slot
    if (int rc = live_enqueue(h, p, k, sample_kind, stream); rc != RTS_OK) {
        h->failed = 1;
        return rc;
    }
    live_commit(h, p, k);
    return RTS_OK;
}

int rts_live_feed(rts_live *h, const void *samples_host, int sample_kind, const int32_t *counts_host, void *stream) {
    using namespace rts;
    if (!h || !counts_host) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (sample_kind != RTS_F32 && sample_kind != RTS_I16) return set_error(RTS_ERR_INVALID, "samples must be RTS_F32 or RTS_I16");
    int32_t *counts = nullptr;
    void *samples = nullptr;
    long long capacity = 0;
    if (int rc = rts_live_staging(h, &counts, &samples, &capacity); rc != RTS_OK) return rc;
    long long total = 0;
    for (int b = 0; b < h->geo.B; b++) {
        if (counts_host[b] < 0) return set_error(RTS_ERR_INVALID, "stream %d: negative sample count", b);
        total += counts_host[b];
    }
    if (total > capacity)
        return set_error(RTS_ERR_INVALID, h->rs ? "%lld samples in one feed exceed the staging capacity of %lld input-rate samples"
                                                : "%lld samples in one feed exceed B * max_pending = %lld", total, capacity);
    if (total > 0 && !samples_host) return set_error(RTS_ERR_INVALID, "samples_host is NULL");
    memcpy(counts, counts_host, sizeof(int32_t) * (size_t)h->geo.B);
    if (total > 0) memcpy(samples, samples_host, (size_t)total * (sample_kind == RTS_F32 ? sizeof(float) : sizeof(int16_t)));
    return rts_live_submit(h, sample_kind, stream);
}

int rts_live_poll(rts_live *h, int32_t *status, int32_t *positions, int *feeds_done, int *feeds_submitted) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    const int fd = live_read_published(h, [=](int b) {
        if (status) status[b] = live_word<kPubStatus, kStatusStatus>(h, b);
        if (positions) {
            positions[2 * b] = live_word<kPubStatus, kStatusLive>(h, b);
            positions[2 * b + 1] = live_word<kPubStatus, kStatusRef>(h, b);
        }
    });
    if (feeds_done) *feeds_done = fd;
    if (feeds_submitted) *feeds_submitted = h->feeds;
    return RTS_OK;
}

int rts_live_watch(rts_live *h, int K) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (K < 0 || K > 256) return set_error(RTS_ERR_INVALID, "K must be in [0, 256] (got %d)", K);
    if (!h->otw)
        return set_error(RTS_ERR_UNSUPPORTED, "rts_live_watch on a WTW tracker: there is no WTW path cost (its cosine cost is NaN "
                                              "on silent frames and its windows re-decide the path)");
    if (K > 0) {
        if (int rc = live_pub_alloc(h, kPubConf, "rts_live_watch"); rc != RTS_OK) return rc;
    }
    h->watch_k = K;
    return RTS_OK;
}

int rts_live_confidence(rts_live *h, double *mean_cost, int32_t *n_points, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->pub_host[kPubConf]) return set_error(RTS_ERR_INVALID, "rts_live_confidence before any rts_live_watch(K > 0)");
    const int fd = live_read_published(h, [=](int b) {
        if (mean_cost) mean_cost[b] = live_word<kPubConf, kConfMean>(h, b);
        if (n_points) n_points[b] = live_word<kPubConf, kConfN>(h, b);
    });
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_annotate(rts_live *h, rts_annot *annot, const uint8_t *mask_host, const int32_t *piece_host,
                      const int32_t *frame0_host, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!annot) {  // off: the words stay as they are
        h->annot = nullptr;
        return RTS_OK;
    }
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (!mask_host || !piece_host) return set_error(RTS_ERR_INVALID, "mask_host and piece_host must be given with tables");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (annot_device(annot) != h->device)
        return set_error(RTS_ERR_INVALID, "the tables live on device %d, the handle on device %d", annot_device(annot), h->device);
    const int B = h->geo.B, P = annot_pieces(annot);
    for (int b = 0; b < B; b++) {
        if (!mask_host[b]) continue;
        if (piece_host[b] < 0 || piece_host[b] >= P)
            return set_error(RTS_ERR_INVALID, "stream %d: piece %d outside [0, %d)", b, piece_host[b], P);
        if (frame0_host && frame0_host[b] < 0) return set_error(RTS_ERR_INVALID, "stream %d: negative frame0 %d", b, frame0_host[b]);
    }
    if (!h->ann_tables) {
        const size_t nB = (size_t)B;
        int32_t *tables = nullptr;
        hipError_t e = hipMalloc((void **)&tables, sizeof(int32_t) * 2 * nB);
        if (e == hipSuccess) e = hipMemset(tables, 0xff, sizeof(int32_t) * nB);  // no piece
        if (e == hipSuccess) e = hipMemset(tables + nB, 0, sizeof(int32_t) * nB);
        if (int rc = e == hipSuccess ? live_pub_alloc(h, kPubBeats, "rts_live_annotate")
                                     : set_error(RTS_ERR_HIP, "rts_live_annotate: %s", hipGetErrorString(e));
            rc != RTS_OK) {
            if (tables) (void)hipFree(tables);  // nothing is left behind
            return rc;
        }
        h->ann_tables = tables;
    }
    if (int rc = annot_select_enqueue(B, mask_host, piece_host, frame0_host, h->ann_tables, h->ann_tables + B, (hipStream_t)stream);
        rc != RTS_OK)
        return rc;
    h->annot = annot;
    return RTS_OK;
}

int rts_live_beats(rts_live *h, double *beat, int32_t *label, int32_t *ref_frame, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->pub_host[kPubBeats]) return set_error(RTS_ERR_INVALID, "rts_live_beats before any rts_live_annotate with tables");
    const int fd = live_read_published(h, [=](int b) {
        if (beat) beat[b] = live_word<kPubBeats, kBeatsBeat>(h, b);
        if (label) label[b] = live_word<kPubBeats, kBeatsLabel>(h, b);
        if (ref_frame) ref_frame[b] = live_word<kPubBeats, kBeatsRef>(h, b);
    });
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_follow_tempo(rts_live *h, int K, double ahead) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (K == 0) {  // off: the words stay as they are
        h->tempo_k = 0;
        return RTS_OK;
    }
    TempoTail view;
    if (int rc = tempo_tail_check(K, ahead, live_tracker_view(h, &view)); rc != RTS_OK) return rc;
    if (int rc = live_pub_alloc(h, kPubTempo, "rts_live_follow_tempo"); rc != RTS_OK) return rc;
    h->tempo_ahead = ahead;
    h->tempo_k = K;
    return RTS_OK;
}

int rts_live_tempo(rts_live *h, double *slope, double *pos, double *bpm, int32_t *n, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->pub_host[kPubTempo]) return set_error(RTS_ERR_INVALID, "rts_live_tempo before any rts_live_follow_tempo(K > 0)");
    const int fd = live_read_published(h, [=](int b) {
        if (slope) slope[b] = live_word<kPubTempo, kTempoSlope>(h, b);
        if (pos) pos[b] = live_word<kPubTempo, kTempoPos>(h, b);
        if (bpm) bpm[b] = live_word<kPubTempo, kTempoBpm>(h, b);
        if (n) n[b] = live_word<kPubTempo, kTempoN>(h, b);
    });
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_follow_consensus(rts_live *h, rts_ensemble *e) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (!e) {  // off: the words stay as they are
        h->ens = nullptr;
        h->args.ens_state = nullptr;
        return RTS_OK;
    }
    if (!h->ann_tables)
        return set_error(RTS_ERR_INVALID, "rts_live_follow_consensus before any rts_live_annotate with tables: the member beat "
                                          "needs every stream's piece and frame0");
    if (ensemble_batch(e) != h->geo.B)
        return set_error(RTS_ERR_INVALID, "the ensemble e was created for B = %d streams, the handle has %d", ensemble_batch(e),
                         h->geo.B);
    if (ensemble_device(e) != h->device)
        return set_error(RTS_ERR_INVALID, "the ensemble e lives on device %d, the handle on device %d", ensemble_device(e),
                         h->device);
    if (int rc = live_pub_alloc(h, kPubEns, "rts_live_follow_consensus"); rc != RTS_OK) return rc;
    h->ens = e;
    h->ens_groups = ensemble_groups(e);
    h->args.ens_state = ensemble_state(e);
    return RTS_OK;
}

int rts_live_consensus(rts_live *h, double *consensus, double *spread, int32_t *n_in, int32_t *n_valid, double *dev,
                       int32_t *strikes, int32_t *out, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->pub_host[kPubEns])
        return set_error(RTS_ERR_INVALID, "rts_live_consensus before any rts_live_follow_consensus with an ensemble");
    const int G = h->ens_groups;
    const int fd = live_read_published(h, [=](int b) {
        if (b < G) {  // the group words ride under the sequence words of the first G streams: every stream's is written last
            if (consensus) consensus[b] = live_word<kPubEns, kEnsConsensus>(h, b);
            if (spread) spread[b] = live_word<kPubEns, kEnsSpread>(h, b);
            if (n_in) n_in[b] = live_word<kPubEns, kEnsNIn>(h, b);
            if (n_valid) n_valid[b] = live_word<kPubEns, kEnsNValid>(h, b);
        }
        if (dev) dev[b] = live_word<kPubEns, kEnsDev>(h, b);
        if (strikes) strikes[b] = live_word<kPubEns, kEnsStrikes>(h, b);
        if (out) out[b] = live_word<kPubEns, kEnsOut>(h, b);
    });
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_gate(rts_live *h, double min_level, int hold) {
    using namespace rts;
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (!(min_level >= 0.0) || min_level > 1.7976931348623157e308)
        return set_error(RTS_ERR_INVALID, "min_level must be a finite mean square >= 0 (0 = gate off)");
    if (hold < 0 || hold > kGateMaxHold) return set_error(RTS_ERR_INVALID, "hold must be in [0, %d] (got %d)", kGateMaxHold, hold);
    if (min_level > 0.0 && h->acc_on)
        return set_error(RTS_ERR_UNSUPPORTED, "rts_live_gate with the accompaniment on: with a gate live indices are not microphone time");
    if (h->feeds != 0)
        return set_error(RTS_ERR_INVALID, "rts_live_gate after %d feeds: the gate is set before the first feed after create or "
                                          "rts_live_reset, so that every ordinal counts from a closed stream", h->feeds);
    if (min_level > 0.0 && !h->gate.q) {
        if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
        const size_t nB = (size_t)h->geo.B;
        GateArgs t = {};
        t.ord_len = h->otw ? otw_history(h->otw) : wtw_history(h->wtw);
        hipError_t e = hipMalloc((void **)&t.lev, sizeof(double) * nB * h->cols_cap);
        if (e == hipSuccess) e = hipMalloc((void **)&t.gcols, sizeof(double) * kLiveF * nB * h->cols_cap);
        e = live_dev_zeroed(e, &t.n_gated, nB);
        if (e == hipSuccess) e = hipMalloc((void **)&t.q, sizeof(int32_t) * nB);
        if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)t.q, kGateClosed, nB);
        e = live_dev_zeroed(e, &t.prev, nB);
        e = live_dev_zeroed(e, &t.seen, nB);
        e = live_dev_zeroed(e, &t.passed, nB);
        e = live_dev_zeroed(e, &t.ord, nB * (size_t)t.ord_len);
        if (int rc = e == hipSuccess ? live_pub_alloc(h, kPubGate, "rts_live_gate")
                                     : set_error(RTS_ERR_HIP, "rts_live_gate: %s", hipGetErrorString(e));
            rc != RTS_OK) {
            for (void *p : {(void *)t.lev, (void *)t.gcols, (void *)t.n_gated, (void *)t.q, (void *)t.prev, (void *)t.seen,
                            (void *)t.passed, (void *)t.ord})
                if (p) (void)hipFree(p);  // nothing is left behind
            return rc;
        }
        t.pub_level = pub_ptr<kPubGate, kGateLevel>(h->args.pubs.dev[kPubGate], h->geo.B);
        t.pub_words = pub_ptr<kPubGate, kGateOpen>(h->args.pubs.dev[kPubGate], h->geo.B);  // open, seen, passed interleaved
        h->gate = t;
    }
    h->gate.min_level = min_level;
    h->gate.hold = hold;
    h->gate.diff = h->geo.diff;
    h->gate_on = min_level > 0.0;
    return RTS_OK;
}

int rts_live_levels(rts_live *h, double *level, int32_t *open, int32_t *seen, int32_t *passed, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->gate.q) return set_error(RTS_ERR_INVALID, "rts_live_levels before any rts_live_gate(min_level > 0)");
    const int fd = live_read_published(h, [=](int b) {
        if (level) level[b] = live_word<kPubGate, kGateLevel>(h, b);
        if (open) open[b] = live_word<kPubGate, kGateOpen>(h, b);
        if (seen) seen[b] = live_word<kPubGate, kGateSeen>(h, b);
        if (passed) passed[b] = live_word<kPubGate, kGatePassed>(h, b);
    });
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_gate_columns(rts_live *h, int b, int32_t *ordinals_host, int cap, int *n, void *stream) {
    using namespace rts;
    if (!h || !n) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (!h->gate.q) return set_error(RTS_ERR_INVALID, "rts_live_gate_columns before any rts_live_gate(min_level > 0)");
    if (b < 0 || b >= h->geo.B) return set_error(RTS_ERR_INVALID, "stream %d out of range [0, %d)", b, h->geo.B);
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    int32_t passed = 0;
    RTS_HIP(hipMemcpyAsync(&passed, h->gate.passed + b, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    *n = passed;
    int k = passed < h->gate.ord_len ? passed : h->gate.ord_len;
    if (k > cap) k = cap;
    if (k > 0 && ordinals_host) {
        RTS_HIP(hipMemcpyAsync(ordinals_host, h->gate.ord + (size_t)b * h->gate.ord_len, sizeof(int32_t) * (size_t)k,
                               hipMemcpyDeviceToHost, s));
        RTS_HIP(hipStreamSynchronize(s));
    }
    return RTS_OK;
}

int rts_live_columns_view(rts_live *h, double **cols_dev, int *cols_cap, int *cols_stride, int32_t **n_cols_dev) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (cols_dev) *cols_dev = h->gate_on ? h->gate.gcols : h->geo.diff ? h->args.dcols : h->args.cols;
    if (cols_cap) *cols_cap = h->cols_cap;
    if (cols_stride) *cols_stride = h->last_stride;
    if (n_cols_dev) *n_cols_dev = h->gate_on ? h->gate.n_gated : h->geo.diff ? h->args.n_cols : h->args.n_frames;
    return RTS_OK;
}

int rts_live_pending(rts_live *h, long long *pending_host /* [B] */) {
    using namespace rts;
    if (!h || !pending_host) return set_error(RTS_ERR_INVALID, "NULL argument");
    memcpy(pending_host, h->cur.pending, sizeof(long long) * (size_t)h->geo.B);
    return RTS_OK;
}

int rts_live_accompany(rts_live *h, rts_warp *warp_plan, const void *tracks_dev, int track_dtype, const uint8_t *mask_host,
                       const long long *first_host, const long long *len_host, const long long *origin_host,
                       const rts_accomp_params *params) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!warp_plan) {  // off: the words and chunks stay as they are
        h->acc_on = 0;
        if (h->acc) accomp_off(h->acc);
        return RTS_OK;
    }
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (h->gate_on)
        return set_error(RTS_ERR_UNSUPPORTED, "rts_live_accompany with the level gate on: live indices count the columns the "
                                              "tracker received, not microphone time");
    if (h->rs)
        return set_error(RTS_ERR_UNSUPPORTED, "rts_live_accompany on a session that resamples its input: live indices are not "
                                              "in samples of the microphones' clock");
    if (!tracks_dev) return set_error(RTS_ERR_INVALID, "tracks_dev is NULL");
    if (track_dtype != RTS_F32 && track_dtype != RTS_I16) return set_error(RTS_ERR_INVALID, "track_dtype must be RTS_F32 or RTS_I16");
    if (!mask_host || !first_host || !len_host) return set_error(RTS_ERR_INVALID, "mask_host, first_host and len_host must be given");
    if (h->geo.B > 65535) return set_error(RTS_ERR_INVALID, "B = %d: the renderer takes at most 65535 streams", h->geo.B);
    AccompGeom p;
    if (int rc = accomp_check(params, warp_plan, h->geo.hop, h->device, &p); rc != RTS_OK) return rc;
    TempoTail view;
    if (int rc = tempo_tail_check(p.K, 0.0, live_tracker_view(h, &view)); rc != RTS_OK) return rc;
    if (int rc = accomp_tracks_check(h->geo.B, mask_host, first_host, len_host, origin_host); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (h->acc && !accomp_same(h->acc, p, warp_plan, tracks_dev, track_dtype)) {
        // another plan, pool or law: everything is rebuilt once the device has finished with what there is
        h->acc_on = 0;
        RTS_HIP(hipDeviceSynchronize());
        accomp_destroy(h->acc);
        h->acc = nullptr;
    }
    if (!h->acc) {
        if (int rc = accomp_create(p, warp_plan, tracks_dev, track_dtype, h->geo.B, h->device, &h->acc); rc != RTS_OK) return rc;
    }
    accomp_arm(h->acc, mask_host, first_host, len_host, origin_host);
    h->acc_on = 1;
    return RTS_OK;
}

int rts_live_accompaniment(rts_live *h, const float **chunk_host, long long *row_stride, int32_t *blocks, long long *out_total,
                           long long *in_pos, double *rate, int32_t *status, int32_t *warp_status, int *feeds_done) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!h->acc) return set_error(RTS_ERR_INVALID, "rts_live_accompaniment before any rts_live_accompany with a plan");
    const int fd = live_read_published(h, [](int) {});
    accomp_look(h->acc, fd, chunk_host, row_stride, blocks, out_total, in_pos, rate, status, warp_status);
    if (feeds_done) *feeds_done = fd;
    return RTS_OK;
}

int rts_live_accomp_map(rts_live *h, int b, long long *anchors_host, int cap, int *n, long long state[2], void *stream) {
    using namespace rts;
    if (!h || !n) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (!h->acc) return set_error(RTS_ERR_INVALID, "rts_live_accomp_map before any rts_live_accompany with a plan");
    if (b < 0 || b >= h->geo.B) return set_error(RTS_ERR_INVALID, "stream %d out of range [0, %d)", b, h->geo.B);
    if (cap < 0) return set_error(RTS_ERR_INVALID, "cap must be >= 0");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    return accomp_map(h->acc, b, anchors_host, cap, n, state, (hipStream_t)stream);
}

}  // extern "C"

#include "snapshot_live.h"  // rts_live_export / rts_live_import: single streams move between sessions

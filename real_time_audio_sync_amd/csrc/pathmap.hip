// The time map of a path: where a moment of one recording lies on the other (include/rtsync.h, rts_path_map, has the
// definition; csrc/pathmap_device.h the verdict on a path and the image of one position; csrc/pathmap_plan.h the host's
// checks and the geometry).  The reference takes error statistics of a path and stops there (tests.py:59-137).
//   rts_path_map        float64 positions of column `from`, in frames      -> positions on the other column
//   rts_annot_transfer  the rows of an annotation table, in seconds         -> the table of the other recording
//
// Both kernels: one workgroup of 256 lanes per pair.  The workgroup walks the pair's path once, 256 points per turn, and
// reduces the status word; after the barrier of that reduction every lane knows the verdict.  The lanes then take entries
// tid, tid + 256, ..: a usable path costs an entry at most three bisections of column `from`, dependent global loads log2
// P deep (16 at 40 000 points), a refused one a NaN.  The path stays in global memory: 40 000 points are 320 KB, twice a
// CU's LDS, and an entry reads about 3 * 16 of them; the 4 LDS words are the reduction's.  No atomics, nothing handed from
// one workgroup to another, no workspace.
//
// Every index is bounded: points inside min(len, P_max), entries inside min(n, n_max), a table's rows inside its own
// length and rows_max, a piece outside [0, P) has no rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "annot_device.h"
#include "common.h"
#include "pathmap_device.h"
#include "pathmap_plan.h"

#pragma clang fp contract(off)

namespace rts {

__global__ void __launch_bounds__(kPathmapThreads)
path_map_kernel(const int32_t *path, int P_max, const int32_t *len, const int32_t *off, int from, const double *x, int n_max,
                const int32_t *n_dev, double *y, int32_t *status) {
    __shared__ int32_t red[kPathmapWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const PathSide s = pathmap_side(path, P_max, len, off, from, b);
    const int st = pathmap_status(s, red);
    if (tid == 0) status[b] = st;
    const int n = pathmap_entries(n_dev != nullptr, n_dev ? n_dev[b] : 0, n_max);
    const size_t row = pathmap_entry_offset(b, n_max);
    for (int e = tid; e < n; e += kPathmapThreads) y[row + e] = st ? pathmap_nan() : pathmap_at(s, x[row + e]);
}

__global__ void __launch_bounds__(kPathmapThreads)
annot_transfer_kernel(AnnotTables t, const int32_t *path, int P_max, const int32_t *len, const int32_t *off, int from,
                      const int32_t *piece_dev, int rows_max, double *times, int32_t *n_rows, int32_t *status) {
    __shared__ int32_t red[kPathmapWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const AnnotPiece p = annot_piece(t, piece_dev[b]);
    if (p.n < 1) {  // no such piece: uniform over the workgroup
        if (tid == 0) {
            n_rows[b] = 0;
            status[b] = RTS_PATHMAP_EMPTY;
        }
        return;
    }
    const PathSide s = pathmap_side(path, P_max, len, off, from, b);
    const int st = pathmap_status(s, red);
    const int n = pathmap_entries(true, p.n, rows_max);  // the host refused a rows_max below the longest table
    if (tid == 0) {
        n_rows[b] = n;
        status[b] = st;
    }
    const size_t row = pathmap_entry_offset(b, rows_max);
    for (int r = tid; r < n; r += kPathmapThreads) {
        double out = pathmap_nan();
        if (!st) {
            const double yy = pathmap_at(s, p.times[r] / t.frame_seconds);
            if (yy == yy) out = yy * t.frame_seconds;
        }
        times[row + r] = out;
    }
}

}  // namespace rts

extern "C" {

int rts_path_map(const int32_t *path_dev, int P_max, const int32_t *len_dev, const int32_t *off_dev, int from,
                 const double *x_dev, int n_max, const int32_t *n_dev, int B, double *y_dev, int32_t *status_dev, void *stream) {
    using namespace rts;
    if (const PathmapRefusal why = pathmap_check(path_dev, P_max, len_dev, from, x_dev, false, n_max, B, y_dev, status_dev);
        why != kPathmapOk)
        return set_error(RTS_ERR_INVALID, "rts_path_map: %s", pathmap_message(why, false));
    hipLaunchKernelGGL(path_map_kernel, dim3(pathmap_grid(B)), dim3(kPathmapThreads), 0, (hipStream_t)stream, path_dev, P_max,
                       len_dev, off_dev, from, x_dev, n_max, n_dev, y_dev, status_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_annot_transfer(rts_annot *h, const int32_t *path_dev, int P_max, const int32_t *len_dev, const int32_t *off_dev, int from,
                       const int32_t *piece_dev, int B, int rows_max, double *times_dev, int32_t *n_rows_dev, int32_t *status_dev,
                       void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (const PathmapRefusal why = pathmap_check(path_dev, P_max, len_dev, from, piece_dev, true, rows_max, B, times_dev, status_dev);
        why != kPathmapOk)
        return set_error(RTS_ERR_INVALID, "rts_annot_transfer: %s", pathmap_message(why, true));
    if (!n_rows_dev) return set_error(RTS_ERR_INVALID, "rts_annot_transfer: n_rows_dev is NULL");
    if (rows_max < annot_longest(h))
        return set_error(RTS_ERR_INVALID, "rts_annot_transfer: rows_max (%d) is below the longest table of the handle (%d rows)",
                         rows_max, annot_longest(h));
    if (int rc = check_device(annot_device(h), "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(annot_transfer_kernel, dim3(pathmap_grid(B)), dim3(kPathmapThreads), 0, (hipStream_t)stream,
                       *annot_tables(h), path_dev, P_max, len_dev, off_dev, from, piece_dev, rows_max, times_dev, n_rows_dev,
                       status_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"

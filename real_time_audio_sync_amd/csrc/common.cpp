// librtsync.so: error reporting, device discovery (rts_last_error, rts_version, rts_device_count) and the host-side rules
// the handles share (device check, host-mapped blocks, reference ranges and tables, path read-back, restart selection).
#include "common.h"

#include <string.h>

namespace rts {

char *last_error_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int check_device(int handle_device, const char *noun) {
    int d = -1;
    RTS_HIP(hipGetDevice(&d));
    if (d != handle_device)
        return set_error(RTS_ERR_INVALID, "%s was created on device %d but device %d is current "
                                          "(one process per GPU, or hipSetDevice before the call)", noun, handle_device, d);
    return RTS_OK;
}

hipError_t mapped_alloc(size_t bytes, void **host, void **dev) {
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess && (e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) (void)hipHostFree(h);
    *host = e == hipSuccess ? h : nullptr;
    *dev = e == hipSuccess ? d : nullptr;
    return e;
}

int ref_ranges_check(int B, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                     long long n_ref_frames, int len_max, const char *len_name) {
    int longest = 0;
    for (int b = 0; b < B; b++) {
        if (mask_host && !mask_host[b]) continue;
        if (len_host[b] < 1) return set_error(RTS_ERR_INVALID, "stream %d: len must be >= 1 (got %d)", b, len_host[b]);
        if (first_host[b] < 0) return set_error(RTS_ERR_INVALID, "stream %d: first must be >= 0 (got %lld)", b, first_host[b]);
        if (first_host[b] > n_ref_frames - len_host[b])
            return set_error(RTS_ERR_INVALID, "stream %d: frames [%lld, %lld) lie outside the %lld reference frames", b,
                             first_host[b], first_host[b] + len_host[b], n_ref_frames);
        if (len_name && len_host[b] > len_max)
            return set_error(RTS_ERR_INVALID, "stream %d: len %d exceeds the handle's %s = %d (its buffers were sized by it)", b,
                             len_host[b], len_name, len_max);
        if (len_host[b] > longest) longest = len_host[b];
    }
    return longest;
}

hipError_t ref_table_upload(RefTable *t, const long long *first_host, const int32_t *len_host, int B) {
    hipError_t e;
    if ((e = hipMalloc((void **)&t->first, sizeof(long long) * (size_t)B)) != hipSuccess ||
        (e = hipMalloc((void **)&t->len, sizeof(int32_t) * (size_t)B)) != hipSuccess ||
        (e = hipMemcpy(t->first, first_host, sizeof(long long) * (size_t)B, hipMemcpyHostToDevice)) != hipSuccess)
        return e;
    return hipMemcpy(t->len, len_host, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice);
}

void ref_table_free(RefTable *t) {
    if (t->first) (void)hipFree(t->first);
    if (t->len) (void)hipFree(t->len);
    t->first = nullptr;
    t->len = nullptr;
}

int read_path(const int32_t *state, int state_len, int n_path_slot, const int32_t *path, int path_cap, int b, int B,
              int32_t *pairs, int cap_pairs, int *n, hipStream_t s) {
    if (b < 0 || b >= B) return set_error(RTS_ERR_INVALID, "stream index %d out of range [0, %d)", b, B);
    int32_t np = 0;
    RTS_HIP(hipMemcpyAsync(&np, state + (size_t)b * state_len + n_path_slot, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    *n = np;
    int m = np < path_cap ? np : path_cap;
    if (m > cap_pairs) m = cap_pairs;
    if (m > 0 && pairs) {
        RTS_HIP(hipMemcpyAsync(pairs, path + (size_t)b * path_cap * 2, sizeof(int32_t) * 2 * (size_t)m, hipMemcpyDeviceToHost, s));
        RTS_HIP(hipStreamSynchronize(s));
    }
    return RTS_OK;
}

int restart_check(int B, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                  long long n_ref_frames, int len_max, const char *len_name) {
    if (!mask_host) return set_error(RTS_ERR_INVALID, "mask_host is NULL");
    if ((first_host == nullptr) != (len_host == nullptr))
        return set_error(RTS_ERR_INVALID, "first_host and len_host must both be given or both be NULL");
    if (!first_host) return RTS_OK;
    if (n_ref_frames < 0)
        return set_error(RTS_ERR_INVALID, "new reference ranges need a handle with per-stream references (rts_*_create_refs)");
    const int rc = ref_ranges_check(B, mask_host, first_host, len_host, n_ref_frames, len_max, len_name);
    return rc < 0 ? rc : RTS_OK;
}

int restart_next_chunk(int B, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host, int *pos,
                       RestartSel *sel) {
    int n = 0, b = *pos;
    sel->set_ref = first_host != nullptr;
    for (; b < B && n < kRestartChunk; b++) {
        if (!mask_host[b]) continue;
        sel->idx[n] = b;
        sel->first[n] = first_host ? first_host[b] : 0;
        sel->len[n] = len_host ? len_host[b] : 0;
        n++;
    }
    *pos = b;
    sel->n = n;
    return n;
}

}  // namespace rts

extern "C" {

const char *rts_last_error(void) { return rts::last_error_buf(); }

int rts_version(void) { return 101; }

int rts_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        rts::set_error(RTS_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return e == hipErrorNoDevice ? 0 : RTS_ERR_HIP;
    }
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

}  // extern "C"

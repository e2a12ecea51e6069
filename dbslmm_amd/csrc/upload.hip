// upload.hip -- the panel on the device (included by plan.hip): staged host -> device uploads of a
// .bed through pinned buffers, from memory or a file descriptor, and the resident panel image made
// from the verbatim bytes, shared between a context's cache and its plans.

// An image cached from a file descriptor has no host bytes behind its key: once the verbatim
// upload has become the panel image of one n_ref, a call that passes the key with another n_ref
// cannot be served (the host-array cache uploads again from its pointer, panel_image()).
static bool key_of_other_n_ref(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref) {
    if (!ctx->bed_from_fd || bed != ctx->bed_host || bed_len != ctx->bed_host_len || ctx->bed_cache ||
        !ctx->img_cache.mem || ctx->img_cache.n_ref == n_ref)
        return false;
    ctx->err = "the image cached from a file descriptor was built for n_ref = " +
               std::to_string(ctx->img_cache.n_ref) + "; cache it again to use n_ref = " + std::to_string(n_ref);
    return true;
}
#define KEY_CHECK(ctx, bed, bed_len, nref)                                              \
    do {                                                                                \
        if (key_of_other_n_ref(ctx, bed, bed_len, nref)) return DBSLMM_E_STATE;         \
    } while (0)

// Host -> device copy of a large buffer through pinned staging buffers: a pool of host threads
// fills the chunks (memcpy from the caller's memory, or pread from a file) as far ahead as free
// buffers allow while earlier chunks' DMAs run; kStageBufs buffers, each reused once its copy's
// event has completed.  The threads live for the whole copy and hand chunks over through atomic
// counters (a condition variable notified by every part woke the whole pool 16 times per chunk:
// 11 GB/s end to end on the box, against 47 GB/s for pread into pinned memory and 48 GB/s for
// the DMA alone -- tools/micro/upload_probe).  Small buffers take a plain hipMemcpy.  Ends
// synchronised.  fill(dst, offset, len) -> false on error.
template <class Fill>
static hipError_t upload_pipelined(void* dst, size_t n, hipStream_t st, Fill fill) {
    // 4 x 16 MiB: pinning costs ~0.25 ms per MiB on the box (3 x 64 MiB took 47 ms), while 16 MiB
    // DMAs still run at ~45 GB/s (tools/micro/upload_probe)
    constexpr size_t kChunk = size_t(16) << 20;
    constexpr int kStageBufs = 4;
    PinnedBuf stage[kStageBufs];   // (freed, like the events, when the copy has ended)
    EventList done;
    hipError_t e = hipSuccess;
    for (int b = 0; b < kStageBufs && e == hipSuccess; ++b) {
        e = stage[b].reserve(kChunk);
        if (e == hipSuccess) e = done.grow(b + 1);
    }
    const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nchunk = (n + kChunk - 1) / kChunk;
    std::atomic<int64_t> go{-1};          // chunks 0 .. go may be filled (their buffer is free)
    std::atomic<bool> bad{false}, stop{false};
    std::unique_ptr<std::atomic<unsigned>[]> parts(new std::atomic<unsigned>[nchunk]);
    for (size_t k = 0; k < nchunk; ++k) parts[k].store(0, std::memory_order_relaxed);
    std::vector<std::thread> th;
    if (e == hipSuccess)
        for (unsigned t = 0; t < T; ++t)
            th.emplace_back([&, t] {
                for (size_t k = 0; k < nchunk; ++k) {
                    backoff_wait([&] {
                        return go.load(std::memory_order_acquire) >= static_cast<int64_t>(k) ||
                               stop.load(std::memory_order_relaxed);
                    });
                    if (go.load(std::memory_order_acquire) < static_cast<int64_t>(k)) return;   // stopped
                    const size_t off = k * kChunk, len = std::min(kChunk, n - off);
                    const size_t part = (len + T - 1) / T, a0 = std::min(len, t * part), z = std::min(len, a0 + part);
                    if (!(a0 >= z || fill(stage[k % kStageBufs].get<char>() + a0, off + a0, z - a0)))
                        bad.store(true, std::memory_order_relaxed);
                    parts[k].fetch_add(1, std::memory_order_release);
                }
            });
    int64_t released = -1;                // highest chunk whose buffer was handed to the pool
    auto release_free = [&](size_t k) {   // chunks k .. k + kStageBufs - 1 whose buffers are free
        for (size_t k2 = std::max<int64_t>(released + 1, k); k2 < std::min(nchunk, k + kStageBufs); ++k2) {
            if (k2 >= static_cast<size_t>(kStageBufs) && k2 != k &&
                hipEventQuery(done[k2 % kStageBufs]) != hipSuccess)
                break;                    // chunk k2 - kStageBufs's DMA still runs
            released = static_cast<int64_t>(k2);
        }
        go.store(released, std::memory_order_release);
    };
    for (size_t k = 0; k < nchunk && e == hipSuccess; ++k) {
        const int b = static_cast<int>(k % kStageBufs);
        if (released < static_cast<int64_t>(k)) {
            if (k >= static_cast<size_t>(kStageBufs) && (e = hipEventSynchronize(done[b])) != hipSuccess) break;
            released = static_cast<int64_t>(k) - 1;
        }
        release_free(k);
        backoff_wait([&] { return parts[k].load(std::memory_order_acquire) == T; });
        if (bad.load(std::memory_order_relaxed)) { e = hipErrorInvalidValue; break; }
        const size_t off = k * kChunk, len = std::min(kChunk, n - off);
        e = hipMemcpyAsync(static_cast<char*>(dst) + off, stage[b].get(), len, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(done[b], st);
    }
    stop.store(true, std::memory_order_relaxed);
    for (auto& t : th) t.join();
    const hipError_t e2 = hipStreamSynchronize(st);
    return e != hipSuccess ? e : e2;
}

static hipError_t upload_staged(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n <= (size_t(128) << 20)) {   // (stream-ordered: a pageable hipMemcpy may return before its
                                      // DMA lands, ordered only on the null stream)
        const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    }
    return upload_pipelined(dst, n, st, [src](char* d, size_t off, size_t len) {
        memcpy(d, static_cast<const char*>(src) + off, len);
        return true;
    });
}

// len bytes of the file at offset off (short reads continued); false on an error or the file's end
static bool read_fully(int fd, char* d, size_t off, size_t len) {
    for (size_t got = 0; got < len;) {
        const ssize_t r = pread(fd, d + got, len - got, static_cast<off_t>(off + got));
        if (r <= 0) return false;
        got += static_cast<size_t>(r);
    }
    return true;
}

// The same reading the bytes from a file descriptor (pread straight into the pinned staging
// buffers): the caller's pages of the file are never faulted in, so neither the copy nor the
// process's exit pays for hundreds of thousands of page-table entries.
static hipError_t upload_staged_fd(void* dst, int fd, size_t n, hipStream_t st) {
    if (n <= (size_t(32) << 20)) {   // small images (the reference's example: 72 KB): one read and one
                                     // pageable copy -- pinning the staging buffers would cost ~20 ms
        std::vector<char> h(n);
        if (!read_fully(fd, h.data(), 0, n)) return hipErrorInvalidValue;
        const hipError_t e = hipMemcpyAsync(dst, h.data(), n, hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    }
    return upload_pipelined(dst, n, st, [fd](char* d, size_t off, size_t len) { return read_fully(fd, d, off, len); });
}

// The verbatim .bed on the device by a staged upload.  dst holds bed_len + kBedPad bytes (zero pad).
static hipError_t bed_to_device(dbslmm_ctx* ctx, uint8_t* dst, const uint8_t* bed, int64_t bed_len) {
    hipError_t e = hipMemsetAsync(dst + bed_len, 0, kBedPad, ctx->stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(ctx->stream);
    return e != hipSuccess ? e : upload_staged(dst, bed, bed_len, ctx->stream);
}

static std::shared_ptr<uint8_t> dev_shared(uint8_t* d, int dev) {
    return std::shared_ptr<uint8_t>(d, [dev](uint8_t* q) {
        (void)hipSetDevice(dev);
        (void)hipFree(q);
    });
}

// The panel image of a verbatim device upload d_bed (bed_len + kBedPad bytes) for n_ref
// individuals; complete on return.
static hipError_t image_from_verbatim(dbslmm_ctx* ctx, const uint8_t* d_bed, int64_t bed_len, int32_t n_ref,
                                      PanelImage* out) {
    const int64_t bps = bed_row_bytes(n_ref);
    const int64_t n_rows = (bed_len - 3) / bps;
    if (n_rows >= INT32_MAX) return hipErrorInvalidValue;
    const int64_t pitch = round_up(n_ref, gram::kKpadAlign) / 4;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc(&d, static_cast<size_t>(n_rows + 1) * (pitch + sizeof(v4i)));   // image | row table
    if (e != hipSuccess) return e;
    PanelImage im;
    im.mem = dev_shared(d, ctx->device);
    im.pitch = pitch;
    im.n_rows = static_cast<int32_t>(n_rows);
    im.n_ref = n_ref;
    hipLaunchKernelGGL(dbslmm_bed_repitch, dim3(static_cast<unsigned>((n_rows + 1 + 3) / 4)), dim3(256), 0,
                       ctx->stream, d_bed, n_ref, bps, im.n_rows, d, pitch, const_cast<v4i*>(im.rows()));
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return e;
    *out = std::move(im);
    return hipSuccess;
}

// The panel image of the host .bed range (bed, bed_len) for n_ref individuals: the context's
// cached one when the caller passes the cached host range (built from the cached verbatim upload
// on the first such call, which then releases the verbatim bytes: one resident copy per panel),
// else an upload of its own.
static hipError_t panel_image(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                              PanelImage* out) {
    if (bed == ctx->bed_host && bed_len == ctx->bed_host_len) {
        if (ctx->img_cache.mem && ctx->img_cache.n_ref == n_ref) {
            *out = ctx->img_cache;
            return hipSuccess;
        }
        if (ctx->bed_cache) {
            const hipError_t e = image_from_verbatim(ctx, ctx->bed_cache.get(), bed_len, n_ref, &ctx->img_cache);
            if (e != hipSuccess) return e;
            ctx->bed_cache.reset();
            *out = ctx->img_cache;
            return hipSuccess;
        }
        // (cached for another n_ref and the verbatim bytes are gone: upload again below -- a host
        // array; the entry points turn a file-descriptor key away before this, KEY_CHECK)
    }
    DevBufs B(ctx->device);   // the verbatim upload lives until the image is made
    uint8_t* d_bed = nullptr;
    hipError_t e = B.alloc(&d_bed, bed_len + kBedPad);
    if (e != hipSuccess) return e;
    if ((e = bed_to_device(ctx, d_bed, bed, bed_len)) == hipSuccess) e = image_from_verbatim(ctx, d_bed, bed_len, n_ref, out);
    return e;
}

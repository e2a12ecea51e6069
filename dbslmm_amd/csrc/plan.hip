// plan.hip -- host side of libdbslmm_hip.so: contexts, plans (HBM layout + work lists), the route
// dispatch and the extern "C" entry points of include/dbslmm_hip.h; its parts are included below.
//
// HBM layout of a plan (one context = one GPU):
//   image     the resident panel image (dbslmm_bed_repitch, made once per uploaded panel): the
//             .bed rows without the magic bytes at a pitch of kpad / 4 bytes (64-B aligned rows),
//             bits past individual n_ref - 1 set (PLINK 11 = dosage 0), one all-0xFF zero-dosage
//             row at the end; raw PLINK codes in file order, shared by every plan on the panel;
//             behind it, in the same allocation, the row table: per row the exact integers
//             {sum, sumsq, nmiss} the per-slot statistics are gathered from (dbslmm_slot_stats)
//   slots     non-empty blocks, in block order, each padded to ld = roundup(m + 1, 32) slots:
//             [small SNPs | large SNPs | padding]; per slot: bed row (-1 = pad), block,
//             z-score, output index (>= 0 small, -1-i large); slot m of a block doubles as
//             the row that carries z through the bordered Cholesky
//             (kpad = roundup(n_ref, 256); the Gram kernels gather their operand rows from the
//             image by the slots' bed rows and decode them in registers: no operand buffer)
//   M         fp64 per block ld x ld row-major, lower triangle; row m = z (written by the solve)
//   stats     S, mu, 1/sd per slot; y (solve scratch) per slot; flags/status per block
// The whole problem stays resident; plan_run re-executes stats -> gram -> chol from the
// packed genotypes (nothing cached between runs except the uploaded inputs).
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <numeric>
#include <string>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/dbslmm_hip.h"
#include "dev_bufs.hpp"
#include "ldsc_fit.hpp"
#include "out_ranges.hpp"
#include "plan_layout.hpp"
#include "host_copy.hpp"

// The kernels are compiled in this translation unit (no relocatable device code needed).
#include "kernels.hip"
#include "chol.hip"
#include "chol_tiled.hip"
#include "variance.hip"
#include "score.hip"
#include "trsv.hip"
#include "pcg.hip"
#include "clump.hip"
#include "ldscore.hip"
#include "assoc.hip"

#include "plan_state.hpp"

namespace {
// every instant after the Gram, in stream order: what a run that ends there (no blocks, debug_stop) records
constexpr std::initializer_list<Ev> kEvAfterGram = {kEvLargeEnd, kEvSmallBegin, kEvSmallEnd, kEvTiledBegin,
                                                    kEvTiledEnd, kEvRestEnd, kEvEnd};
constexpr size_t kCholLargeLds = sizeof(double) * chol::kLargeDoubles;
constexpr size_t kCholChebLds = sizeof(double) * chol::kChebLdsDoubles;
constexpr size_t kTiledLds = sizeof(double) * chol::kTiledDoubles;
constexpr size_t kRegionLds = sizeof(double) * chol::kRegionDoubles;
constexpr size_t kTrail3Lds = sizeof(double) * chol::kTrail3k16Doubles;   // the K = 16 variant (2 per CU)
constexpr int kBedPad = 64;            // zero bytes after a verbatim .bed upload (dbslmm_bed_repitch reads whole 16-B chunks)
constexpr int kEpochsPerRun = 1 << 14;  // substitution epochs one run may take (next_epoch)
}  // namespace

#include "upload.hip"

// the dynamic LDS a kernel may ask for
static bool set_lds(const void* kernel, size_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)) == hipSuccess;
}
template <int NR>
static bool set_trsv_lds() {
    return set_lds(reinterpret_cast<const void*>(dbslmm_trsv_fwd<NR>), trsv::kLdsBytes) &&
           set_lds(reinterpret_cast<const void*>(dbslmm_trsv_cheb<NR>), trsv::kLdsBytes) &&
           set_lds(reinterpret_cast<const void*>(dbslmm_tcheb<NR>), (NR * kTChebMaxM + trsv::kT * NR) * sizeof(double)) &&
           set_lds(reinterpret_cast<const void*>(dbslmm_trsv_bwd<NR>), trsv::kLdsBytes);
}

// the deferred part of dbslmm_ctx_create (streams 2-5, events, kernel attributes) is done
static int ctx_ready(dbslmm_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->setup_mu);
    if (ctx->setup.joinable()) ctx->setup.join();
    if (!ctx->setup_ok) {
        ctx->err = "context set-up (streams / events / kernel attributes) failed";
        return DBSLMM_E_HIP;
    }
    return DBSLMM_OK;
}

// Forget the context's cached panel (plans created from its image keep their reference) and, for
// bed_len > 0, allocate the verbatim buffer of a new one at *d with its zero pad enqueued.
static int cache_begin(dbslmm_ctx* ctx, int64_t bed_len, uint8_t** d) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bed_cache.reset();
    ctx->img_cache = PanelImage{};
    ctx->bed_host = nullptr;
    ctx->bed_host_len = 0;
    ctx->bed_from_fd = false;
    if (bed_len == 0) return DBSLMM_OK;
    HIP_TRY(ctx, hipMalloc(d, bed_len + kBedPad));
    ctx->bed_cache = dev_shared(*d, ctx->device);
    HIP_TRY(ctx, hipMemsetAsync(*d + bed_len, 0, kBedPad, ctx->stream));
    return DBSLMM_OK;
}

extern "C" {

int dbslmm_abi_version(void) { return DBSLMM_ABI_VERSION; }

int dbslmm_ctx_create(int device, dbslmm_ctx** out) {
    if (!out) return DBSLMM_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DBSLMM_E_HIP;
    if (device < 0 || device >= n) return DBSLMM_E_ARG;
    auto* c = new dbslmm_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        dbslmm_ctx_destroy(c);
        return DBSLMM_E_HIP;
    }
    c->setup = std::thread([c, device] {
        int prio_lo = 0, prio_hi = 0;   // the tiled sequence is the critical path: high priority
        c->setup_ok =
            hipSetDevice(device) == hipSuccess &&
            hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess &&
            hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_hi) == hipSuccess &&
            // the lead (or only) sequence's bulk trailing stream high too: its far updates pace the
            // lead chain (normal priority left config 5 bimodal, 34 / 39 ms per step)
            hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio_hi) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream5, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->fork2, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->join4, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->join, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->join3, hipEventDisableTiming) == hipSuccess &&
            set_lds(reinterpret_cast<const void*>(dbslmm_chol_large), kCholLargeLds) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_chol_cheb), kCholChebLds) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_gram_big), gram::kLdsBytes) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_l2_tiles), gram::kLdsBytes) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_gram_huge), gram::kHLdsBytes) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_pcg_block), pcg::block_lds_bytes(pcg::kMaxNC)) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_tchol_region), kRegionLds) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_tchol_panel), kTiledLds) &&
            set_lds(reinterpret_cast<const void*>(dbslmm_tchol_trailing3k16), kTrail3Lds) &&
            set_trsv_lds<1>() && set_trsv_lds<2>();
        // The first kernel launch of the process loads the library's code object (~30 ms on the
        // box): done here, beside the caller's .bed upload, instead of inside its first MAF pass
        DevBufs B(device);
        double* d_warm = nullptr;
        if (c->setup_ok && B.alloc(&d_warm, 1) == hipSuccess) {
            hipLaunchKernelGGL(dbslmm_set_scalar, dim3(1), dim3(1), 0, c->stream2, d_warm, 0.0);
            c->setup_ok = hipStreamSynchronize(c->stream2) == hipSuccess;
        }
    });
    *out = c;
    return DBSLMM_OK;
}

void dbslmm_ctx_destroy(dbslmm_ctx* ctx) {
    if (!ctx) return;
    if (ctx->setup.joinable()) ctx->setup.join();
    for (dbslmm_ctx* s : ctx->subs) dbslmm_ctx_destroy(s);
    if (ctx->device < 0) {
        delete ctx;
        return;
    }
    (void)hipSetDevice(ctx->device);
    ctx->bed_cache.reset();
    ctx->img_cache = PanelImage{};
    for (hipStream_t s : {ctx->stream, ctx->stream2, ctx->stream3, ctx->stream4, ctx->stream5})
        if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : {ctx->fork2, ctx->join4, ctx->fork, ctx->join, ctx->join3})
        if (e) (void)hipEventDestroy(e);
    delete ctx;
}

const char* dbslmm_last_error(const dbslmm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dbslmm_ctx_cache_bed(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len) {
    if (!ctx) return DBSLMM_E_ARG;
    if (!ctx->subs.empty()) return DBSLMM_OK;   // multi-device: each device gets its own rows
    ARG_CHECK(ctx, (bed == nullptr) == (bed_len == 0) && bed_len >= 0, "bed / bed_len");
    uint8_t* d = nullptr;
    if (const int rc = cache_begin(ctx, bed_len, &d)) return rc;
    if (!bed) return DBSLMM_OK;
    HIP_TRY(ctx, upload_staged(d, bed, bed_len, ctx->stream));
    ctx->bed_host = bed;
    ctx->bed_host_len = bed_len;
    return DBSLMM_OK;
}

int dbslmm_ctx_cache_bed_fd(dbslmm_ctx* ctx, int fd, int64_t bed_len, const uint8_t* key) {
    if (!ctx) return DBSLMM_E_ARG;
    if (!ctx->subs.empty()) return DBSLMM_OK;   // multi-device: each device gets its own rows
    ARG_CHECK(ctx, fd >= 0 && key && bed_len > 0, "fd / bed_len / key");
    uint8_t* d = nullptr;
    if (const int rc = cache_begin(ctx, bed_len, &d)) return rc;
    if (upload_staged_fd(d, fd, static_cast<size_t>(bed_len), ctx->stream) != hipSuccess) {
        ctx->bed_cache.reset();
        ctx->err = "reading / uploading the .bed from its file descriptor failed";
        return DBSLMM_E_HIP;
    }
    ctx->bed_host = key;
    ctx->bed_host_len = bed_len;
    ctx->bed_from_fd = true;
    return DBSLMM_OK;
}

}  // extern "C"

static int collect_timing(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    for (int r = 0; p->tm.timing && r < p->tm.runs_pending; ++r) {
        hipEvent_t* e = &p->tm.ev.ev[kEvCount * r];
        // event times from the run's start; with split substitutions the tiled factorisation +
        // backward of the two groups ends on two streams (kEvTiledEnd: lead, kEvRestEnd: rest) and
        // the Chebyshev passes start there: tiled = kEvTiledBegin -> the later of the two, trsv =
        // the earlier of the two -> kEvEnd (the spans overlap)
        float t[kEvCount] = {0.f};
        if (r < static_cast<int>(p->tm.run_route.size()) && p->tm.run_route[r]) {
            // PCG: statistics, Gram, iterations; the only instants this route records
            for (Ev k : {kEvStatsEnd, kEvGramEnd, kEvPcgBlockBegin, kEvPcgBlockEnd, kEvEnd})
                HIP_TRY(ctx, hipEventElapsedTime(&t[k], e[kEvStart], e[k]));
            p->tm.ms_acc[DBSLMM_K_UNPACK] += t[kEvStatsEnd];
            p->tm.ms_acc[DBSLMM_K_GRAM] += t[kEvGramEnd] - t[kEvStatsEnd];
            p->tm.ms_acc[DBSLMM_K_PCG] += t[kEvEnd] - t[kEvGramEnd];
            p->tm.ms_acc[DBSLMM_K_PCG_BLOCK] += t[kEvPcgBlockEnd] - t[kEvPcgBlockBegin];   // (inside the PCG span, on the second stream)
            p->tm.ms_runs++;
            continue;
        }
        for (int k = 1; k < kEvCount; ++k) HIP_TRY(ctx, hipEventElapsedTime(&t[k], e[kEvStart], e[k]));
        const float fend = std::max(t[kEvTiledEnd], t[kEvRestEnd]), cstart = std::min(t[kEvTiledEnd], t[kEvRestEnd]);
        float span[DBSLMM_K_COUNT] = {t[kEvStatsEnd], t[kEvGramEnd] - t[kEvStatsEnd], t[kEvLargeEnd] - t[kEvGramEnd],
                                      t[kEvSmallEnd] - t[kEvSmallBegin], fend - t[kEvTiledBegin], t[kEvEnd] - cstart, 0.f, 0.f};
        for (int k = 0; k < DBSLMM_K_COUNT; ++k) p->tm.ms_acc[k] += span[k];
        // the lead group's Gram sits inside the statistics span (kEvStart -> kEvStatsEnd)
        float lg = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&lg, e[kEvLeadGramBegin], e[kEvLeadGramEnd]));
        p->tm.ms_acc[0] -= lg;
        p->tm.ms_acc[1] += lg;
        p->tm.ms_runs++;
    }
    p->tm.runs_pending = 0;
    p->tm.run_route.clear();
    return DBSLMM_OK;
}

// Grow the per-copy buffers to n solve copies (betas, status, sigma scalars, scratch) and mc
// block-matrix copies (the factorisation route factors mc = n copies of the Gram; the PCG route
// reads one Sigma, copy 0).  Contents are rebuilt by the next run.
static int ensure_copies(dbslmm_plan* p, int n, int mc) {
    dbslmm_ctx* ctx = p->ctx;
    if (n <= p->n_copies && mc <= p->m_copies) return DBSLMM_OK;
    n = std::max(n, p->n_copies);
    mc = std::max(mc, p->m_copies);
    std::lock_guard<std::mutex> lk(g_capture_mu);   // device-wide sync + synchronous memset
    HIP_TRY(ctx, hipDeviceSynchronize());
    DevBufs& B = p->bufs;
    B.release_all(p->d_M, p->d_dshift, p->d_y, p->d_beta_s, p->d_beta_l, p->d_status);
    const size_t nn = static_cast<size_t>(n), nm = static_cast<size_t>(mc);
    // (+ 256 elements: the PCG product's masked row segments may run past the last block's rows)
    HIP_TRY(ctx, B.zeroed(&p->d_M, std::max<size_t>(1, nm * p->M_elems) + 256, ctx->stream));
    HIP_TRY(ctx, B.alloc(&p->d_dshift, nn));
    HIP_TRY(ctx, B.alloc(&p->d_y, nn * std::max<int64_t>(1, p->n_slots)));
    HIP_TRY(ctx, B.alloc(&p->d_beta_s, nn * std::max<int64_t>(1, p->n_s)));
    HIP_TRY(ctx, B.alloc(&p->d_beta_l, nn * std::max<int64_t>(1, p->n_l)));
    HIP_TRY(ctx, B.alloc(&p->d_status, nn * p->nbk));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    p->n_copies = n;
    p->m_copies = mc;
    p->fac.drop_graphs();   // (they hold the old pointers)
    return DBSLMM_OK;
}

// Open a timed run (dbslmm_plan_enable_timing): *ev = its kEvCount events, created on first use, and
// its route noted for collect_timing.  An untimed run leaves *ev null.
static int open_timed_run(dbslmm_plan* p, bool pcg, hipEvent_t** ev) {
    *ev = nullptr;
    if (!p->tm.timing) return DBSLMM_OK;
    const size_t need = kEvCount * static_cast<size_t>(p->tm.runs_pending + 1);
    HIP_TRY(p->ctx, p->tm.ev.grow(need));
    *ev = &p->tm.ev.ev[kEvCount * p->tm.runs_pending];
    p->tm.runs_pending++;
    p->tm.run_route.resize(p->tm.runs_pending);
    p->tm.run_route.back() = pcg ? 1 : 0;
    return DBSLMM_OK;
}

// Record the instants `ks` of a timed run on stream st, in that order: the phases a run does not
// have, so that its event set is complete (collect_timing).  Nothing for an untimed run.
static int record_instants(dbslmm_ctx* ctx, hipEvent_t* ev, std::initializer_list<Ev> ks, hipStream_t st) {
    if (!ev) return DBSLMM_OK;
    for (Ev k : ks) HIP_TRY(ctx, hipEventRecord(ev[k], st));
    return DBSLMM_OK;
}

// What a Gram launch writes: copies [0, ncopy) of every block's matrix, except that blocks with
// m >= tmin_copy write copy tcopy only (tcopy < 0: all); the PCG route also stores the integer
// Gram as uint16 (g16 with its per-block offsets and strides; null on the factorisation route).
struct GramOut {
    int32_t ncopy, tmin_copy, tcopy;
    uint16_t* g16;
    const int64_t* off16;
    const int32_t* ld16;
};
enum GramKernel { kGramI8, kGramBig, kGramHuge };
// One Gram launch on stream st: the `nt` tiles at `tiles` by kernel `which` (nt = 0: nothing).
static hipError_t launch_gram(const dbslmm_plan* p, hipStream_t st, GramKernel which, const GramTile* tiles,
                              int32_t nt, const GramOut& o) {
    if (nt <= 0) return hipSuccess;
    struct Shape {
        decltype(&dbslmm_gram_i8) kernel;
        int tiles_per_wg, threads;
        size_t lds;
    };
    static const Shape shapes[] = {{dbslmm_gram_i8, 4, 256, 0},
                                   {dbslmm_gram_big, 1, 256, gram::kLdsBytes},
                                   {dbslmm_gram_huge, 1, 512, gram::kHLdsBytes}};
    const Shape& k = shapes[which];
    hipLaunchKernelGGL(k.kernel, dim3((nt + k.tiles_per_wg - 1) / k.tiles_per_wg), dim3(k.threads), k.lds, st,
                       p->d_img, p->kpad, p->d_slot_pos, p->img.n_rows, tiles, nt, p->d_row0, p->d_m, p->d_ld,
                       p->d_matoff, p->d_flags, p->d_S, p->d_mu, p->d_rsd, static_cast<double>(p->n_ref),
                       static_cast<double>(p->kpad - p->n_ref), p->tau, p->d_M, o.ncopy, p->M_elems, o.tmin_copy,
                       o.tcopy, o.g16, o.off16, o.ld16);
    return hipGetLastError();
}

// The one writer of p->last: whoever ends a run states everything it leaves behind (a caller that
// keeps a member starts from the previous record and says so).
static void close_run(dbslmm_plan* p, const LastRun& r) { p->last = r; }

#include "route_factor.hip"
#include "route_pcg.hip"

// One run: a PCG run still pending is finished first (plan_run without sync), then the route the
// sigmas pick enqueues the whole run (pcg_route).
static int run_impl(dbslmm_plan* p, const double* sigmas, int n) {
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    if (pcg_route(p, sigmas, n)) return run_pcg(p, sigmas, n);
    // A run kept off the PCG route by its number of copies alone keeps that route's accuracy: its
    // iterated h2f copies stop at pcg_tol (relative error per block and copy, as run_pcg), so a
    // fifth h2f factor does not move the results of the others from 1e-12 to cheb_tol.
    p->fac.h2f_tol = n > pcg::kMaxNC && pcg_eligible(p, sigmas, n) ? std::min(p->opt.cheb_tol, p->opt.pcg_tol) : p->opt.cheb_tol;
    return run_factor(p, sigmas, n);
}

// The plan's enqueued work is done: a pending PCG run closed, the main stream drained and the
// substitutions' error word read.
static int drain(dbslmm_plan* p) {
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    HIP_TRY(p->ctx, hipStreamSynchronize(p->ctx->stream));
    return check_trsv(p);
}

// Results of factorisation copies c0 .. c0 + n - 1 (each copy's betas / status contiguous on the
// device and in the caller's arrays): one asynchronous copy per array into the plan's pinned
// buffer, then a threaded copy out (pageable hipMemcpy of 8 MB arrays cost ~0.3 ms each).
static int download_copies(dbslmm_plan* p, int c0, int n, double* beta_s, double* beta_l, int32_t* block_status) {
    dbslmm_ctx* ctx = p->ctx;
    if (!p->last.ran) { ctx->err = "plan_download before plan_run"; return DBSLMM_E_STATE; }
    if (p->last.stopped) { ctx->err = "plan_download after a run stopped at the Gram (debug_stop)"; return DBSLMM_E_STATE; }
    if (const int rc = drain(p)) return rc;
    const size_t nbs = beta_s ? static_cast<size_t>(n) * p->n_s : 0;
    const size_t nbl = beta_l ? static_cast<size_t>(n) * p->n_l : 0;
    const size_t nst = block_status && p->num_block ? static_cast<size_t>(n) * p->nbk : 0;
    const size_t bytes = (nbs + nbl) * sizeof(double) + nst * sizeof(int32_t);
    if (bytes == 0) return DBSLMM_OK;
    HIP_TRY(ctx, p->pin.reserve(bytes));
    double* ps = p->pin.get<double>();
    double* pl = ps + nbs;
    int32_t* pt = reinterpret_cast<int32_t*>(pl + nbl);
    // per copy: its DMA into the pinned buffer, an event, then (below) its host copy-out while the
    // next copy's DMA runs
    HIP_TRY(ctx, p->dl_ev.grow(n));
    if (nst) HIP_TRY(ctx, hipMemcpyAsync(pt, p->d_status + c0 * p->nbk, nst * sizeof(int32_t),
                                         hipMemcpyDeviceToHost, ctx->stream));
    const size_t cs = nbs / n, cl = nbl / n;   // per copy
    for (int c = 0; c < n; ++c) {
        if (cs) HIP_TRY(ctx, hipMemcpyAsync(ps + c * cs, p->d_beta_s + static_cast<int64_t>(c0 + c) * p->n_s,
                                            cs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (cl) HIP_TRY(ctx, hipMemcpyAsync(pl + c * cl, p->d_beta_l + static_cast<int64_t>(c0 + c) * p->n_l,
                                            cl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(p->dl_ev[c], ctx->stream));
    }
    for (int c = 0; c < n; ++c) {
        HIP_TRY(ctx, hipEventSynchronize(p->dl_ev[c]));
        if (cs) par_memcpy(beta_s + c * cs, ps + c * cs, cs * sizeof(double));
        if (cl) par_memcpy(beta_l + c * cl, pl + c * cl, cl * sizeof(double));
    }
    for (int c = 0; c < n && nst; ++c) {
        int32_t* out = block_status + static_cast<int64_t>(c) * p->num_block;
        memcpy(out, pt + c * p->nbk, p->num_block * sizeof(int32_t));
        for (int32_t b : p->h_empty) out[b] = DBSLMM_BLOCK_EMPTY;
    }
    return DBSLMM_OK;
}

extern "C" {

void dbslmm_plan_destroy(dbslmm_plan* p) {
    if (!p) return;
    if (p->mp) {
        mp_destroy(p);
        delete p;
        return;
    }
    (void)hipSetDevice(p->ctx->device);
    p->img = PanelImage{};   // (shared with the context when it came from its cache)
    delete p;                // (its members free what they own: dev_bufs.hpp)
}

int dbslmm_plan_create(dbslmm_ctx* ctx, const dbslmm_problem* pr, dbslmm_plan** out) {
    if (!ctx) return DBSLMM_E_ARG;
    if (!ctx->subs.empty()) return mp_create(ctx, pr, out);
    ARG_CHECK(ctx, pr && out, "null problem/out");
    *out = nullptr;
    if (const int rc = ctx_ready(ctx)) return rc;
    ARG_CHECK(ctx, pr->bed && pr->n_ref > 1 && pr->n_obs > 0 && pr->num_block >= 0, "bad sizes");
    // the FP4 Gram accumulates the raw-form sums, integers up to 9 kpad, in fp32 (exact below 2^24)
    ARG_CHECK(ctx, 9 * round_up(pr->n_ref, gram::kKpadAlign) < (int64_t(1) << 24),
              "n_ref must be at most 1,863,936 (exact FP4 Gram accumulation)");
    ARG_CHECK(ctx, pr->s_ptr && (pr->s_ptr[pr->num_block] == 0 || (pr->s_pos && pr->z_s)), "bad small CSR");
    ARG_CHECK(ctx, pr->sigma_s > 0.0 && std::isfinite(pr->sigma_s), "sigma_s must be > 0");
    ARG_CHECK(ctx, pr->bed_len >= 3 + bed_row_bytes(pr->n_ref), "bed image shorter than one SNP row");
    KEY_CHECK(ctx, pr->bed, pr->bed_len, pr->n_ref);
    const bool has_l = pr->l_ptr != nullptr;
    if (has_l) ARG_CHECK(ctx, pr->l_ptr[pr->num_block] == 0 || (pr->l_pos && pr->z_l), "bad large CSR");
    const dbslmm_options op = pr->opts ? *pr->opts : dbslmm_options{};
    // ---- host-side layout (plan_layout.hpp); its upload-only lists go with L
    PlanLayout L;
    if (const int rc = build_plan_layout(*pr, op, ctx->n_cu, L, ctx->err)) return rc;

    auto* p = new dbslmm_plan();
    static_cast<PlanLayout::Kept&>(*p) = std::move(L.keep);
    p->ctx = ctx;
    p->bufs.device = ctx->device;
    p->n_ref = pr->n_ref;
    p->n_obs = pr->n_obs;
    p->num_block = pr->num_block;
    p->sigma_s = pr->sigma_s;
    p->tau = pr->tau;
    p->bed_len = pr->bed_len;
    p->pcg.g16 = 4 * static_cast<int64_t>(pr->n_ref) <= 65535;
    PlanOptions& o = p->opt;   // frozen from here on
    o.solver = op.solver;
    o.pcg_fused = op.pcg_whole >= 0;
    o.stream_out = op.stream_out >= 0;
    o.pcg_block_wgs = op.pcg_block_wgs;
    if (op.pcg_tol > 0.0) o.pcg_tol = std::max(1e-15, op.pcg_tol);
    if (op.pcg_maxit > 0) o.pcg_maxit = op.pcg_maxit;
    o.h2f_mode = op.h2f_mode;
    o.cheb_fused = op.cheb_fused == 1;
    o.h2f_cg = op.h2f_iter != 1;
    o.debug_delay_us = op.debug_delay_us;
    o.debug_stop = op.debug_stop;
    if (op.cheb_tol > 0.0) o.cheb_tol = std::max(1e-16, op.cheb_tol);

    // ---- device allocations
    hipError_t e = hipSetDevice(ctx->device);
    auto fail = [&](const char* what) {
        ctx->err = std::string(what) + ": " + hipGetErrorString(e);
        dbslmm_plan_destroy(p);
        return DBSLMM_E_HIP;
    };
    if (e != hipSuccess) return fail("hipSetDevice");
    // the panel image: the context's cached one (read-only, shared: no copy) or an upload of our own
    if ((e = panel_image(ctx, pr->bed, pr->bed_len, pr->n_ref, &p->img)) != hipSuccess) return fail("upload bed");
    p->d_img = p->img.mem.get();
    // (every memset of the plan's buffers is ordered on the main stream, which every run starts
    // on: a null-stream hipMemset is not ordered against the context's non-blocking streams, and
    // one still running under the first run's Gram would zero matrix entries behind it)
    const char* what = nullptr;   // the step that failed
    auto up = [&](const char* w, auto** d, const auto& h) {
        if (!what && (e = p->bufs.upload(d, h, ctx->stream)) != hipSuccess) what = w;
    };
    up("upload slots", &p->d_slot_pos, L.slot_pos);
    up("upload slots", &p->d_slot_block, L.slot_block);
    up("upload slots", &p->d_slot_out, p->h_slot_out);
    up("upload z", &p->d_z, L.z);
    up("upload blocks", &p->d_row0, p->h_row0);
    up("upload blocks", &p->d_m, p->h_m);
    up("upload blocks", &p->d_ms, p->h_ms);
    up("upload blocks", &p->d_ld, p->h_ld);
    up("upload blocks", &p->d_matoff, p->h_matoff);
    up("upload blocks", &p->d_blk_id, p->h_blk_id);
    up("upload order", &p->d_order, L.order);
    up("upload tiles", &p->d_tiles, L.tiles);
    up("upload tiles", &p->d_btiles, L.btiles);
    up("upload tiles", &p->d_htiles, L.htiles);
    up("upload tiled lists", &p->fac.d_tlist, L.tlist);
    up("upload trsv lists", &p->fac.d_tri_f, L.tri_f);
    up("upload trsv lists", &p->fac.d_tri_b, L.tri_b);
    up("upload trsv lists", &p->fac.d_foff, L.foff);
    up("upload trsv lists", &p->fac.d_tb, p->h_tb);
    if (!L.tcheb_list.empty()) up("upload trsv lists", &p->fac.d_tcheb_blocks, L.tcheb_list);
    if (what) return fail(what);
    // [tile flags | ticket counter | error word | spare]
    if ((e = p->bufs.zeroed(&p->fac.d_tflags, p->n_tflags + 3, ctx->stream)) != hipSuccess ||
        (e = p->bufs.zeroed(&p->fac.d_tepi, p->n_tflags, ctx->stream)) != hipSuccess)
        return fail("hipMalloc trsv flags");
    if ((e = p->bufs.alloc(&p->d_S, p->n_slots)) != hipSuccess || (e = p->bufs.alloc(&p->d_mu, p->n_slots)) != hipSuccess ||
        (e = p->bufs.alloc(&p->d_rsd, p->n_slots)) != hipSuccess)
        return fail("hipMalloc stats");
    const size_t nbk = std::max<int32_t>(1, std::max(p->n_nonempty, p->num_block));
    p->nbk = static_cast<int64_t>(nbk);
    // (zeroed here for the PCG route, whose front kernel only sets bits: run_pcg)
    if ((e = p->bufs.zeroed(&p->d_flags, nbk, ctx->stream)) != hipSuccess) return fail("hipMalloc flags");
    // (the block matrices, betas, status and sigma scalars are allocated by the first run, for as
    // many factorisation copies as it solves: ensure_copies -- an h2f plan is not sized twice)
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail("plan set-up");
    *out = p;
    return DBSLMM_OK;
}

int dbslmm_plan_set_sigma(dbslmm_plan* p, double sigma_s) {
    if (!p) return DBSLMM_E_ARG;
    ARG_CHECK(p->ctx, sigma_s > 0.0 && std::isfinite(sigma_s), "sigma_s must be > 0");
    p->sigma_s = sigma_s;
    if (p->mp)
        for (auto& sh : p->mp->shards) sh.plan->sigma_s = sigma_s;
    return DBSLMM_OK;
}

int dbslmm_plan_enable_timing(dbslmm_plan* p, int enable) {
    if (!p) return DBSLMM_E_ARG;
    p->tm.timing = enable != 0;
    for (double& v : p->tm.ms_acc) v = 0.0;
    p->tm.ms_runs = 0;
    if (p->mp)
        for (auto& sh : p->mp->shards) dbslmm_plan_enable_timing(sh.plan, enable);
    return DBSLMM_OK;
}

int dbslmm_plan_run(dbslmm_plan* p) {
    if (!p) return DBSLMM_E_ARG;
    if (p->mp) return mp_run(p, &p->sigma_s, 1, false);
    return run_impl(p, &p->sigma_s, 1);
}

// h2f tuning (software/DBSLMM.R:204-219 runs dbslmm once per h2 factor): one statistics pass + Gram, then
// n_sigma factorisations + solves of device copies of it, all in one merged launch sequence.
int dbslmm_plan_run_multi(dbslmm_plan* p, const double* sigmas, int32_t n_sigma, double* beta_s,
                          double* beta_l, int32_t* block_status) {
    if (!p) return DBSLMM_E_ARG;
    dbslmm_ctx* ctx = p->ctx;
    ARG_CHECK(ctx, sigmas && n_sigma > 0 && n_sigma <= 64, "sigmas / n_sigma (1..64)");
    for (int i = 0; i < n_sigma; ++i)
        ARG_CHECK(ctx, sigmas[i] > 0.0 && std::isfinite(sigmas[i]), "sigma_s must be > 0");
    if (p->mp) {
        for (auto& sh : p->mp->shards)
            ARG_CHECK(ctx, static_cast<int64_t>(sh.plan->n_nonempty) * n_sigma < 32768,
                      "blocks x sigmas per device must stay below 32768 (packed work items)");
        int rc = mp_run(p, sigmas, n_sigma, true);
        if (rc == DBSLMM_OK) rc = mp_download_all(p, n_sigma, beta_s, beta_l, block_status);
        return rc;
    }
    ARG_CHECK(ctx, static_cast<int64_t>(p->n_nonempty) * n_sigma < 32768,
              "blocks x sigmas must stay below 32768 (packed work items)");
    p->so.want = true;                       // (the PCG route may stream its results: stream_out)
    int rc = run_impl(p, sigmas, n_sigma);
    p->so.want = false;
    if (!rc && p->last.pcg_ran && p->so.active) return stream_results(p, beta_s, beta_l, block_status);
    if (!rc) rc = dbslmm_plan_sync(p);
    if (!rc) rc = download_copies(p, 0, n_sigma, beta_s, beta_l, block_status);
    return rc;
}

int dbslmm_plan_sync(dbslmm_plan* p) {
    if (!p) return DBSLMM_E_ARG;
    if (p->mp) return mp_sync(p);
    if (const int rc = drain(p)) return rc;
    return collect_timing(p);
}

int dbslmm_plan_kernel_ms(dbslmm_plan* p, double* ms_out, int32_t* launches_out) {
    if (!p || !ms_out) return DBSLMM_E_ARG;
    if (p->mp) {   // per kernel class the slowest device (the critical path of the node)
        int32_t runs = INT32_MAX;
        for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = 0.0;
        for (auto& sh : p->mp->shards) {
            if (p->last.ran && sh.run_copies.empty()) continue;   // a job the latest run skipped (stale)
            double ms[DBSLMM_K_COUNT];
            int32_t n = 0;
            dbslmm_plan_kernel_ms(sh.plan, ms, &n);
            for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = std::max(ms_out[k], ms[k]);
            runs = std::min(runs, n);
        }
        if (launches_out) *launches_out = runs == INT32_MAX ? 0 : runs;
        return DBSLMM_OK;
    }
    for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = p->tm.ms_runs ? p->tm.ms_acc[k] / p->tm.ms_runs : 0.0;
    if (launches_out) *launches_out = p->tm.ms_runs;
    return DBSLMM_OK;
}

#ifdef DBSLMM_DIAG
// diagnostic build only (not in the public header): the substitution stamps of the last forward launch
extern "C" int dbslmm_diag_trsv_stamps(dbslmm_plan* p, unsigned long long* out, int n) {
    if (!p || !p->fac.d_stamps) return DBSLMM_E_STATE;
    if (hipDeviceSynchronize() != hipSuccess) return DBSLMM_E_HIP;
    return hipMemcpy(out, p->fac.d_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess
               ? DBSLMM_OK : DBSLMM_E_HIP;
}
#endif

int dbslmm_plan_block_iters(dbslmm_plan* p, int32_t* iters) {
    if (!p || !iters) return DBSLMM_E_ARG;
    if (p->mp) return mp_block_iters(p, iters);
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    HIP_TRY(p->ctx, hipStreamSynchronize(p->ctx->stream));
    std::fill(iters, iters + p->num_block, 0);
    if (!p->last.pcg_ran) return DBSLMM_OK;
    for (int b = 0; b < p->pcg.n_pblk; ++b) iters[p->h_blk_id[b]] = p->pcg.h_mon()[1 + b];
    return DBSLMM_OK;
}

int dbslmm_out_ranges(int32_t num_block, const int64_t* s_ptr, const int64_t* l_ptr, int64_t* ranges,
                      int32_t* n_ranges) {
    if (num_block < 0 || !s_ptr || !ranges || !n_ranges) return DBSLMM_E_ARG;
    std::vector<OutRange> t;
    if (!build_out_ranges(num_block, s_ptr, l_ptr, t)) return DBSLMM_E_ARG;
    for (size_t i = 0; i < t.size(); ++i) {
        const int64_t row[5] = {t[i].blk, t[i].s0, t[i].s1, t[i].l0, t[i].l1};
        std::copy(row, row + 5, ranges + 5 * i);
    }
    *n_ranges = static_cast<int32_t>(t.size());
    return DBSLMM_OK;
}

int dbslmm_plan_workload(const dbslmm_plan* p, double* out) {
    if (!p || !out) return DBSLMM_E_ARG;
    if (p->mp) {   // sums over the jobs; [12] launches, [14] iterations: the max; [15] job 0's;
                   // SNPs [0] and blocks [6] once per block (not per split h2f copy)
        for (int i = 0; i < DBSLMM_WORKLOAD_LEN; ++i) out[i] = 0.0;
        out[15] = -1;
        if (p->mp->shards.empty()) return DBSLMM_OK;   // a units plan whose device owns no unit
        for (auto& sh : p->mp->shards) {
            if (p->last.ran && sh.run_copies.empty()) continue;   // a job the latest run skipped (stale)
            double w[DBSLMM_WORKLOAD_LEN];
            dbslmm_plan_workload(sh.plan, w);
            for (int i = 0; i < DBSLMM_WORKLOAD_LEN; ++i)
                out[i] = (i == 12 || i == 14 || i == 17 || i == 18) ? std::max(out[i], w[i])
                         : ((i == 0 || i == 6) && sh.copy > 0) ? out[i] : out[i] + w[i];
        }
        double w0[DBSLMM_WORKLOAD_LEN];
        dbslmm_plan_workload(p->mp->shards[0].plan, w0);
        out[15] = w0[15];
        return DBSLMM_OK;
    }
    for (int i = 0; i < DBSLMM_WORKLOAD_LEN; ++i) out[i] = p->wl[i];
    out[14] = p->last.cheb_iters;
    out[15] = p->last.cheb_base;
    out[16] = p->last.cheb_bytes;
    out[17] = p->last.pcg_ran ? 1.0 : 0.0;
    out[18] = p->last.pcg_ran ? p->pcg.iters_max : 0.0;
    out[19] = p->last.pcg_ran ? p->pcg.cbytes : 0.0;
    out[20] = p->last.pcg_ran ? p->pcg.pbytes : 0.0;
    out[21] = p->last.pcg_ran ? p->pcg.fbytes : 0.0;
    if (p->last.cg_ran && p->fac.d_cgit) {   // the passes each tiled block ran before it converged (run_multi is synchronous)
        std::vector<int32_t> it(std::max(1, p->n_nonempty));
        if (hipSetDevice(p->ctx->device) != hipSuccess ||
            hipMemcpy(it.data(), p->fac.d_cgit, it.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return DBSLMM_E_HIP;
        double bytes = 0.0;
        for (int32_t b : p->h_tb) {
            const double T = (p->h_m[b] + trsv::kT - 1) / trsv::kT;
            bytes += 2.0 * it[b] * T * (T + 1) / 2 * trsv::kT * trsv::kT * sizeof(double);
        }
        out[16] = bytes;
    }
    return DBSLMM_OK;
}

int dbslmm_plan_block_matrix(dbslmm_plan* p, int32_t block, int32_t copy, double* out, int32_t* ld_out) {
    if (!p) return DBSLMM_E_ARG;
    dbslmm_ctx* ctx = p->ctx;
    ARG_CHECK(ctx, block >= 0 && block < p->num_block, "block out of range");
    if (p->mp) {   // the shard that solves the block (sub-plan block id = its position in the shard)
        for (auto& sh : p->mp->shards)
            for (size_t j = 0; j < sh.blocks.size(); ++j)
                if (sh.blocks[j] == block) {
                    const int rc = dbslmm_plan_block_matrix(sh.plan, static_cast<int32_t>(j), copy, out, ld_out);
                    if (rc != DBSLMM_OK) ctx->err = sh.plan->ctx->err;
                    return rc;
                }
        ARG_CHECK(ctx, false, "block has no SNPs");
    }
    ARG_CHECK(ctx, copy >= 0 && copy < p->m_copies, "copy out of range");
    const auto it = std::find(p->h_blk_id.begin(), p->h_blk_id.end(), block);
    ARG_CHECK(ctx, it != p->h_blk_id.end(), "block has no SNPs");
    const size_t nb = static_cast<size_t>(it - p->h_blk_id.begin());
    const int64_t ld = p->h_ld[nb];
    if (ld_out) *ld_out = static_cast<int32_t>(ld);
    if (!out) return DBSLMM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    std::lock_guard<std::mutex> lk(g_capture_mu);   // device-wide sync + synchronous copy
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, p->d_M + static_cast<int64_t>(copy) * p->M_elems + p->h_matoff[nb],
                           ld * ld * sizeof(double), hipMemcpyDeviceToHost));
    return DBSLMM_OK;
}

int dbslmm_plan_download(dbslmm_plan* p, double* beta_s, double* beta_l, int32_t* block_status) {
    if (!p) return DBSLMM_E_ARG;
    if (p->mp) {
        if (!p->last.ran) { p->ctx->err = "plan_download before plan_run"; return DBSLMM_E_STATE; }
        return mp_download(p, p->last.var_copy, beta_s, beta_l, block_status);
    }
    return download_copies(p, p->last.var_copy, 1, beta_s, beta_l, block_status);
}

int dbslmm_est(dbslmm_ctx* ctx, const dbslmm_problem* pr, double* beta_s, double* beta_l,
               int32_t* block_status) {
    if (!ctx) return DBSLMM_E_ARG;
    dbslmm_plan* p = nullptr;
    int rc = dbslmm_plan_create(ctx, pr, &p);
    if (rc) return rc;
    rc = dbslmm_plan_run(p);
    if (!rc) rc = dbslmm_plan_sync(p);
    if (!rc) rc = dbslmm_plan_download(p, beta_s, beta_l, block_status);
    dbslmm_plan_destroy(p);
    return rc;
}

#include "panel_api.hip"   // the test-panel and .bed entry points (variance, score, MAF, row lists, clumping)

#ifdef DBSLMM_STAMPS
// diagnostic build only (libdbslmm_hip_stamps.so): read + clear the per-phase tick counters
// (16 counters: the region kernel's first-of-super-step regions count at 8..15)
int dbslmm_debug_stamps(double* out8) {
    unsigned long long h[16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(chol::g_stamp), sizeof(h)) != hipSuccess) return -2;
    for (int i = 0; i < 16; ++i) out8[i] = static_cast<double>(h[i]) * 10.0;  // ns (100 MHz clock)
    unsigned long long z[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(chol::g_stamp), z, sizeof(z)) == hipSuccess ? 0 : -2;
}
#endif

}  // extern "C"

#include "multi.hip"

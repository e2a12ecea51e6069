// plan.hip -- host side of libdbslmm_hip.so: contexts, plans (HBM layout + work lists),
// launches and the extern "C" entry points declared in include/dbslmm_hip.h.
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
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <numeric>
#include <string>
#include <memory>
#include <mutex>
#include <chrono>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/dbslmm_hip.h"
#include "dev_bufs.hpp"
#include "ldsc_fit.hpp"
#include "out_ranges.hpp"
#include "plan_layout.hpp"

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

namespace {
// the instants of a timed run, one event each (collect_timing turns them into kernel spans)
enum Ev {
    kEvStart,           // the run's start
    kEvStatsEnd,        // after the statistics gather (slot name: unpack) and the lead group's Gram
    kEvGramEnd,         // after the Gram
    kEvLargeEnd,        // after chol_large
    kEvSmallBegin,      // around chol_small (the main stream, or stream2 without a tiled sequence)
    kEvSmallEnd,
    kEvTiledBegin,      // the tiled factorisation sequence starts (stream2)
    kEvEnd,             // the h2f Chebyshev iterations are done (stream2); PCG: its iterations
    kEvTiledEnd,        // the tiled factorisation + backward are done and the h2f Chebyshev iterations
                        // start (stream2; split substitutions: the lead group's)
    kEvLeadGramBegin,   // around the lead group's Gram (between the statistics and kEvStatsEnd)
    kEvLeadGramEnd,
    kEvRestEnd,         // the rest group's factorisation + backward done (its own stream, split
                        // substitutions; else recorded with kEvTiledEnd)
    kEvCount,           // events per timed run
    kEvPcgBlockBegin = kEvLargeEnd,   // PCG route: around dbslmm_pcg_block (stream2)
    kEvPcgBlockEnd = kEvSmallBegin,
};
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

static_assert(sizeof(v4i) == kRowEntryBytes, "one row-table entry");
// The resident panel image (kernels.hip: dbslmm_bed_repitch): n_rows rows of `pitch` bytes and the
// zero-dosage row n_rows, made for n_ref individuals, followed IN THE SAME ALLOCATION by the row
// table: one 16-byte entry {sum, sumsq, nmiss, 0} per row (the zero-dosage row's all zero), the
// exact integers every per-row statistic derives from (dbslmm_slot_stats).  One allocation, so the
// table lives exactly as long as the image bytes: shared by the context's cache and every plan
// created from it, released with them.
struct PanelImage {
    std::shared_ptr<uint8_t> mem;
    int64_t pitch = 0;
    int32_t n_rows = 0, n_ref = 0;
    int64_t image_bytes() const { return (static_cast<int64_t>(n_rows) + 1) * pitch; }   // a multiple of 64
    const v4i* rows() const { return reinterpret_cast<const v4i*>(mem.get() + image_bytes()); }
};
// Graph capture (launch_graph) vs the device-synchronising setup calls of another host thread
// (multi-device plans run one thread per shard; several shards may share a device): a
// hipDeviceSynchronize / synchronous memset or copy while another thread's stream is capturing
// invalidates that capture.  Both sides hold this lock.
std::mutex g_capture_mu;
}  // namespace

struct dbslmm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // main stream (statistics, gram, large-block Cholesky)
    hipStream_t stream2 = nullptr;   // tiled (multi-workgroup) Cholesky sequence, forked/joined
    hipStream_t stream3 = nullptr;   // its bulk trailing updates (lookahead), forked/joined
    // a plan with a lead group (dbslmm_options.lead_min) factors it on stream2 / stream3 and the
    // other tiled blocks on stream4 / stream5 (chain / bulk trailing), concurrently
    hipStream_t stream4 = nullptr, stream5 = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, join3 = nullptr, fork2 = nullptr, join4 = nullptr;
    int n_cu = 256;                  // compute units (persistent substitution grid)
    std::string err;
    // device copy of a caller's .bed (dbslmm_ctx_cache_bed): bed_maf and plan_create on the same
    // host range (pointer and length) read it instead of uploading again.  The upload is verbatim
    // (bed_cache: the cache calls do not know n_ref); the first use that supplies n_ref turns it
    // into the panel image (img_cache, panel_image()) and releases the verbatim bytes.  A plan
    // created from it shares the image (freed when the context and every such plan have released it)
    const uint8_t* bed_host = nullptr;
    int64_t bed_host_len = 0;
    std::shared_ptr<uint8_t> bed_cache;
    PanelImage img_cache;
    bool bed_from_fd = false;        // cached by dbslmm_ctx_cache_bed_fd: bed_host is a key, never read
    std::vector<dbslmm_ctx*> subs;   // multi-device context (multi.hip): one context per device,
                                     // device = -1 and no streams of its own
    // dbslmm_ctx_create returns once the main stream exists; the other streams, the events and the
    // kernel attributes are set up on this thread meanwhile (each stream costs ~15-30 ms of HIP
    // runtime time), joined by ctx_ready() before anything uses them.  dbslmm_ctx_cache_bed and
    // dbslmm_bed_maf need only the main stream, so a .bed upload overlaps the rest of the set-up.
    std::thread setup;
    std::mutex setup_mu;
    bool setup_ok = true;
};
struct dbslmm_plan;
// the jobs of a multi-device (or units) plan (multi.hip): one plan each
struct DeviceShard {
    dbslmm_plan* plan = nullptr;
    dbslmm_ctx* ctx = nullptr;          // the context the job's plan runs on
    dbslmm_ctx* own_ctx = nullptr;      // ... created for a split unit (owned by the job)
    int device_index = 0;               // in the shard plan's device numbering
    int copy = -1;                      // -1: every h2f copy of its blocks; c: that copy of one block
    std::vector<int32_t> blocks;        // original block ids, in sub-problem order
    std::vector<int64_t> s_idx, l_idx;  // sub small / large SNP -> original beta position
    std::vector<int> run_copies;        // the caller's h2f copy of each of the plan's copies (last run)
    std::vector<double> dl_s, dl_l;     // download staging of every run copy, reused across runs
    std::vector<int32_t> dl_st;         //   (fresh vectors page-faulted ~1 ms per step on a big shard)
};
struct dbslmm_mplan {
    std::vector<DeviceShard> shards;
    int32_t n_copies = 1;               // h2f copies per run the units were planned for
    bool partial = false;               // one device's units (dbslmm_plan_create_units): outputs of
                                        // the other units are left untouched
    std::vector<int32_t> unit_device;   // [block * n_copies + copy] -> device index, -1 empty
};

// (the host layout plan_create computed lives in the base: plan_layout.hpp)
struct dbslmm_plan : PlanLayout::Kept {
    dbslmm_ctx* ctx = nullptr;
    dbslmm_mplan* mp = nullptr;        // multi-device plan: every call fans out over its shards
    int32_t n_ref = 0, n_obs = 0, num_block = 0;
    double sigma_s = 0.0, tau = 0.8;
    int64_t bed_len = 0;
    // device
    DevBufs bufs;                      // owns every d_* member below (freed with the plan)
    PanelImage img;                    // own upload, or the context's cached image (shared)
    const uint8_t* d_img = nullptr;    // img.mem.get(): pitch kpad / 4, zero-dosage row img.n_rows
    int32_t *d_slot_pos = nullptr, *d_slot_block = nullptr, *d_slot_out = nullptr;
    double *d_z = nullptr, *d_S = nullptr, *d_mu = nullptr, *d_rsd = nullptr, *d_y = nullptr;
    int32_t *d_flags = nullptr, *d_status = nullptr, *d_order = nullptr, *d_blk_id = nullptr;
    int32_t* d_tlist = nullptr;         // work lists of the tiled sequence (tl, tl_rest)
    hipGraphExec_t graph_exec = nullptr;   // captured tiled sequence
    int32_t *d_row0 = nullptr, *d_m = nullptr, *d_ms = nullptr, *d_ld = nullptr;
    int64_t* d_matoff = nullptr;
    GramTile* d_tiles = nullptr;       // 32 x 32 tiles of the small blocks (dbslmm_gram_i8)
    GramTile* d_btiles = nullptr;      // 128 x 128 tiles of the mid blocks, per-XCD queues
    GramTile* d_htiles = nullptr;      // 256 x 256 tiles of the big blocks, per-XCD queues
    double* d_M = nullptr;
    double *d_beta_s = nullptr, *d_beta_l = nullptr;
    double* d_dshift = nullptr;        // 1/(sigma_s n), read by the solve kernels
    // h2f tuning: n_copies independent factorisations of the same Gram, copy c at
    // d_M + c M_elems (and the per-copy sigma scalar, scratch, betas, status); one merged tiled
    // sequence factors all copies (tl_multi, built for multi_n copies)
    int32_t n_copies = 0;              // allocated on the first run (ensure_copies), sized for it
    int64_t nbk = 1;                   // status entries per copy
    std::vector<TLaunch> tl_multi;
    int32_t* d_tlist_multi = nullptr;
    int32_t multi_n = 0;
    hipGraphExec_t graph_multi = nullptr;
    int32_t var_copy = 0;              // copy holding the latest factorisation (variance)
    int32_t score_copies = 0;          // copies of the latest user run (dbslmm_plan_score)
    bool score_stale = false;          // the variance's re-solve has overwritten copy 0 of its results
    void* h_pin = nullptr;         // pinned landing buffer of the result downloads
    size_t h_pin_bytes = 0;
    double sigma_run = 0.0;        // sigma_s of the factorisation held in d_M
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;  // kEvCount per run
    std::vector<hipEvent_t> dl_ev;   // result download: one per factorisation copy
    std::vector<hipEvent_t> tev; // dependencies between the tiled sequence's two streams
    std::vector<hipEvent_t> tev_rest;   // ... of the rest sequence
    // h2f tuning by Chebyshev on one factor (trsv.hip): tile work lists of the tiled blocks in
    // forward / backward dependency order, tile flags (+ ticket counter, error word) and the
    // iteration vectors [Y, Z, X, R, D, S] x kMaxR x n_slots
    int32_t *d_tri_f = nullptr, *d_tri_b = nullptr, *d_foff = nullptr, *d_tflags = nullptr, *d_tb = nullptr;
    int32_t* d_tepi = nullptr;                 // per tile: epoch of its last stored Chebyshev update
    int32_t* d_cheb_items = nullptr;           // work list of the fused Chebyshev launch (K iterations)
    int32_t n_cheb_items = 0, cheb_items_K = -1;
    int32_t trsv_epoch = 0;                  // tile-flag value of the latest substitution launch
    int32_t h2f_mode = 0;                    // dbslmm_options.h2f_mode
    double cheb_tol = 1e-9;                  // dbslmm_options.cheb_tol
    double h2f_tol = 1e-9;                   // the current run's target for its iterated copies (run_impl)
    bool cheb_fused = false;                 // dbslmm_options.cheb_fused
    bool h2f_cg = false;                     // dbslmm_options.h2f_iter: the tiled blocks' copies by CG
    double* d_cgrec = nullptr;               // CG: per non-empty block and copy {gamma, alpha}
    int32_t* d_cgconv = nullptr;             // CG: per non-empty block, its copies have converged
    int32_t* d_cgit = nullptr;               // CG: per non-empty block, iterations of the latest run
    bool cg_ran = false;                     // the latest run_multi iterated by CG
    int32_t debug_delay_us = 0;              // dbslmm_options.debug_delay_us (tests)
    int32_t debug_stop = 0;                  // dbslmm_options.debug_stop (tests)
    int64_t n_runs = 0;                      // completed run enqueues (graphs are captured from the second)
    int32_t* d_tcheb_blocks = nullptr;       // sub_block: the rest group's blocks, largest first
    bool trsv_pending = false;               // a persistent substitution ran since the last error check
    bool trsv_failed = false;                // ... and one of its hand-off waits gave up (sticky until the next run)
    unsigned long long* d_stamps = nullptr;  // diagnostic builds (DBSLMM_DIAG) only
    double* d_cheb = nullptr;
    double* d_coef = nullptr;
    int32_t coef_cap = 0;
    std::vector<double> h_coef;              // the coefficients in d_coef
    std::vector<hipGraphExec_t> graph_copy;  // the single-copy tiled sequence on copy c
    std::vector<hipGraphExec_t> graph_rest;  // ... and the rest sequence (lead group)
    int32_t cheb_base = -1;                  // base copy of the last Chebyshev run (-1: none)
    bool cheb_pending_var = false;           // copy var_copy's tiled blocks are not factored yet
    int runs_pending = 0;
    double ms_acc[DBSLMM_K_COUNT] = {0, 0, 0, 0, 0, 0};
    int32_t ms_runs = 0;
    bool ran = false;
    bool stopped = false;          // the last run stopped after the Gram (debug_stop = 1): no betas
    int32_t m_copies = 0;          // block-matrix copies allocated in d_M (<= n_copies)
    // ---- PCG route (dbslmm_options.solver, pcg.hip)
    int32_t solver = 0;            // 0 auto, 1 factorisation, 2 PCG
    double pcg_tol = 1e-12;
    int32_t pcg_maxit = 1000;
    bool force_factor = false;     // the variance's re-solve
    bool pcg_g16 = false;          // n_ref <= 16383: the integer Gram fits uint16
    int32_t pcg_m_blocks = -1;     // blocks with missing calls (fp64 Sigma products); -1 unknown
    uint16_t* d_G16 = nullptr;     // integer Gram: per block Tb*128 x Tb*128 (zero past m)
    int64_t* d_off16 = nullptr;    // ... its offset per block
    int32_t* d_ld16 = nullptr;     // ... its row stride per block (Tb * 128)
    std::vector<int64_t> h_off16;
    int32_t pcg_n = 0;             // copies the PCG buffers are laid out for
    PcgBlk* d_pblk = nullptr;
    int4* d_pitem = nullptr;
    int2* d_prow = nullptr;
    int32_t n_pblk = 0, n_pitem = 0, n_prow = 0;
    int32_t n_pitem_chip = 0, n_prow_chip = 0;   // ... of them, those of the chip-wide blocks (listed first)
    int32_t n_phead = 0;           // d_prow's tail past n_prow: one (block, -1) per block solved whole
    bool pcg_trim = false;         // launch only those: no block dbslmm_pcg_block takes has missing calls
    int32_t pcg_run = pcg::kRunMax;  // tiles per product item (pcg_layout)
    bool pcg_fused = true;         // small one-column blocks solved whole by dbslmm_pcg_block
    int2* d_pflist = nullptr;      // ... their (PcgBlk, copy) sequences (biggest first)
    int32_t* d_pfnext = nullptr;   // ... the next list index to take (16 B, zeroed per run)
    int32_t n_pflist = 0;
    int32_t pcg_block_wgs = 0;     // dbslmm_options.pcg_block_wgs: a cap on dbslmm_pcg_block's workgroups (0: none)
    std::vector<char> h_pfused;    // per PcgBlk: 1 = in that list
    std::vector<int32_t> h_pnseq;  // ... its sequences there (1, or the copies with large SNPs)
    bool pcg_join = false;         // the main stream still has to wait for dbslmm_pcg_block
    double *d_pvec = nullptr, *d_ppart = nullptr, *d_pdot = nullptr, *d_pqs = nullptr;
    int32_t *d_pcnv = nullptr, *d_pitb = nullptr, *d_pdone = nullptr, *d_pact = nullptr, *d_pfin = nullptr;
    int64_t pcg_vstride = 0;
    int32_t* h_pmon = nullptr;     // pinned: [active | itb per block] after a chunk
    int32_t pcg_it = 0;            // iterations enqueued by the current run
    int32_t pcg_need = -1;         // chip-wide iterations the latest finished run needed (-1: no run yet)
    int32_t pcg_iters_max = 0;     // ... and the iterations of its slowest block (any path)
    bool pcg_pending = false;      // a PCG run whose convergence has not been checked yet
    bool pcg_ran = false;          // the latest run took the PCG route
    bool pcg_pending_var = false;  // ... so the variance needs a factorisation first
    std::vector<char> run_route;   // per pending timed run: 1 = PCG
    std::vector<double> h_pmat, h_ppart;   // per PcgBlk: lower-triangle bytes (uint16) / partial-sum bytes per iteration
    std::vector<char> h_pmiss;     // per PcgBlk: missing calls (fp64 Sigma, 4x the matrix bytes)
    double pcg_cbytes = 0.0, pcg_pbytes = 0.0, pcg_fbytes = 0.0;   // the latest run (workload [19]-[21])
    PcgArgs pcg_args{};            // the arguments of the latest PCG run (continuation chunks)
    hipEvent_t pcg_ev_end = nullptr;   // its timing end event (re-recorded by a continuation)
    // ---- streamed results (dbslmm_options.stream_out): on the PCG route of dbslmm_plan_run_multi the
    // kernels write every result to a host-visible mirror as well and flag each (route block, copy)
    // they finish (dbslmm_pcg_block, dbslmm_pcg_update), and the calling thread copies flagged
    // blocks into the caller's arrays while the GPU still iterates (stream_results)
    bool stream_out = true;        // the option
    bool so_want = false;          // the call in progress may stream (dbslmm_plan_run_multi)
    bool so_active = false;        // the latest PCG run writes the mirror
    void* h_mir = nullptr;         // pinned, mapped, coherent: [beta_s | beta_l | status], copy-major
    size_t h_mir_bytes = 0;        //   (the layout and strides of the device arrays, so_n copies)
    int32_t* h_mflag = nullptr;    // ... and [route block * so_n + copy] = so_run once finished
    int32_t so_n = 0;              // copies of the latest streamed run
    int32_t so_run = 0;            // its number (per plan; flags of earlier runs never match)
    hipEvent_t so_ev = nullptr;    // after the last work a chunk enqueued
    std::vector<int2> h_pfpairs;   // the host's scan order: dbslmm_pcg_block's (route block, copy) pairs in its
                                   // list order, then the chip-wide blocks' 
    std::vector<int32_t> so_done;  // [route block * so_n + copy] = so_run once copied out
};

#define HIP_TRY(ctx, expr)                                                               \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (ctx)->err = std::string(#expr) + " (" __FILE_NAME__ ":" + std::to_string(__LINE__) + "): " + \
                         hipGetErrorString(e_);                                          \
            return DBSLMM_E_HIP;                                                         \
        }                                                                                \
    } while (0)

#define ARG_CHECK(ctx, cond, msg)                   \
    do {                                            \
        if (!(cond)) {                              \
            (ctx)->err = msg;                       \
            return DBSLMM_E_ARG;                    \
        }                                           \
    } while (0)

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

// multi-device plans (multi.hip)
static int mp_create(dbslmm_ctx* ctx, const dbslmm_problem* pr, dbslmm_plan** out);
static void mp_destroy(dbslmm_plan* p);
static int mp_download(dbslmm_plan* p, int copy, double* beta_s, double* beta_l, int32_t* block_status);
static int mp_download_all(dbslmm_plan* p, int n, double* beta_s, double* beta_l, int32_t* block_status);
static int mp_run(dbslmm_plan* p, const double* sigmas, int n, bool wait);
static int mp_sync(dbslmm_plan* p);
static int mp_block_iters(dbslmm_plan* p, int32_t* iters);
static int mp_variance(dbslmm_plan* p, const dbslmm_test_panel* tp, double* diags, int32_t* n_test_out);
static int mp_score(dbslmm_plan* p, const dbslmm_test_panel* tp, const dbslmm_score_args* args, int32_t n_copies,
                    double* scores, int32_t* dropped, int32_t* n_test_out, double* gpu_ms);
static int mp_bed_maf(dbslmm_ctx* ctx, const uint8_t* bed, int32_t n_ref, int64_t n_snp, double* maf);
// context-level tools on a multi-device context run on its first device
#define ON_FIRST_DEVICE(ctx, call)                                       \
    do {                                                                 \
        if (!(ctx)->subs.empty()) {                                      \
            dbslmm_ctx* ctx0_ = (ctx)->subs[0];                          \
            const int rc_ = call;                                        \
            if (rc_ != DBSLMM_OK) (ctx)->err = ctx0_->err;               \
            return rc_;                                                  \
        }                                                                \
    } while (0)

// wait until pred(): a short spin (a chunk is ~0.35 ms of work), then 20 us sleeps, so waiting
// threads do not take the cores of the host threads the caller runs meanwhile (the CLI parses
// its text files during the upload) on a machine with fewer cores than the pool
template <class P>
static void backoff_wait(P pred) {
    for (int i = 0; !pred(); ++i) {
        if (i < 256) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

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
    void* stage[kStageBufs] = {};
    hipEvent_t done[kStageBufs] = {};
    hipError_t e = hipSuccess;
    for (int b = 0; b < kStageBufs && e == hipSuccess; ++b) {
        e = hipHostMalloc(&stage[b], kChunk, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[b], hipEventDisableTiming);
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
                    if (!(a0 >= z || fill(static_cast<char*>(stage[k % kStageBufs]) + a0, off + a0, z - a0)))
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
        e = hipMemcpyAsync(static_cast<char*>(dst) + off, stage[b], len, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(done[b], st);
    }
    stop.store(true, std::memory_order_relaxed);
    for (auto& t : th) t.join();
    const hipError_t e2 = hipStreamSynchronize(st);
    for (int b = 0; b < kStageBufs; ++b) {
        if (done[b]) (void)hipEventDestroy(done[b]);
        if (stage[b]) (void)hipHostFree(stage[b]);
    }
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

// The same reading the bytes from a file descriptor (pread straight into the pinned staging
// buffers): the caller's pages of the file are never faulted in, so neither the copy nor the
// process's exit pays for hundreds of thousands of page-table entries.
static hipError_t upload_staged_fd(void* dst, int fd, size_t n, hipStream_t st) {
    if (n <= (size_t(32) << 20)) {   // small images (the reference's example: 72 KB): one read and one
                                     // pageable copy -- pinning the staging buffers would cost ~20 ms
        std::vector<char> h(n);
        size_t got = 0;
        while (got < n) {
            const ssize_t r = pread(fd, h.data() + got, n - got, static_cast<off_t>(got));
            if (r <= 0) return hipErrorInvalidValue;
            got += static_cast<size_t>(r);
        }
        const hipError_t e = hipMemcpyAsync(dst, h.data(), n, hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    }
    return upload_pipelined(dst, n, st, [fd](char* d, size_t off, size_t len) {
        size_t got = 0;
        while (got < len) {
            const ssize_t r = pread(fd, d + got, len - got, static_cast<off_t>(off + got));
            if (r <= 0) return false;
            got += static_cast<size_t>(r);
        }
        return true;
    });
}

// memcpy on up to 8 host threads (a result download lands in pinned memory; the caller's arrays
// are often fresh pages, so the page faults of the copy are spread over the threads too)
static void par_memcpy(void* dst, const void* src, size_t n) {
    constexpr size_t kMin = size_t(2) << 20;
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const unsigned nt = static_cast<unsigned>(std::min<size_t>(hw, std::max<size_t>(1, n / kMin)));
    if (nt <= 1) { if (n) memcpy(dst, src, n); return; }
    const size_t part = (n + nt - 1) / nt;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) {
        const size_t a = t * part, z = std::min(n, a + part);
        if (a < z) th.emplace_back([=] { memcpy(static_cast<char*>(dst) + a, static_cast<const char*>(src) + a, z - a); });
    }
    memcpy(dst, src, std::min(n, part));
    for (auto& t : th) t.join();
}

// The same for a list of copies (a streamed run's remainder: scattered block ranges), the bytes of
// the concatenation split evenly over the threads.
struct CopySeg {
    void* dst;
    const void* src;
    size_t n;
};
static void par_memcpy_list(const std::vector<CopySeg>& segs) {
    constexpr size_t kMin = size_t(512) << 10;
    size_t total = 0;
    for (const CopySeg& s : segs) total += s.n;
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const unsigned nt = static_cast<unsigned>(std::min<size_t>(hw, std::max<size_t>(1, total / kMin)));
    const size_t part = (total + nt - 1) / nt;
    auto work = [&segs, part](unsigned t) {   // bytes [t part, (t + 1) part) of the concatenation
        const size_t lo = t * part, hi = lo + part;
        size_t off = 0;
        for (const CopySeg& s : segs) {
            const size_t a = std::max(lo, off), z = std::min(hi, off + s.n);
            if (a < z) memcpy(static_cast<char*>(s.dst) + (a - off), static_cast<const char*>(s.src) + (a - off), z - a);
            off += s.n;
            if (off >= hi) break;
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
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

template <int NR>
static hipError_t set_trsv_lds() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_trsv_fwd<NR>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(trsv::kLdsBytes));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_trsv_cheb<NR>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(trsv::kLdsBytes));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_tcheb<NR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>((NR * kTChebMaxM + trsv::kT * NR) * sizeof(double)));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_trsv_bwd<NR>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(trsv::kLdsBytes));
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
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_chol_large),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kCholLargeLds)) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_chol_cheb),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kCholChebLds)) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_gram_big),
                                hipFuncAttributeMaxDynamicSharedMemorySize, gram::kLdsBytes) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_l2_tiles),
                                hipFuncAttributeMaxDynamicSharedMemorySize, gram::kLdsBytes) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_gram_huge),
                                hipFuncAttributeMaxDynamicSharedMemorySize, gram::kHLdsBytes) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_pcg_block),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(pcg::block_lds_bytes(pcg::kMaxNC))) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_tchol_region),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kRegionLds)) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_tchol_panel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kTiledLds)) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(dbslmm_tchol_trailing3k16),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(kTrail3Lds)) == hipSuccess &&
            set_trsv_lds<1>() == hipSuccess && set_trsv_lds<2>() == hipSuccess;
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
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream4) (void)hipStreamDestroy(ctx->stream4);
    if (ctx->stream5) (void)hipStreamDestroy(ctx->stream5);
    if (ctx->fork2) (void)hipEventDestroy(ctx->fork2);
    if (ctx->join4) (void)hipEventDestroy(ctx->join4);
    if (ctx->fork) (void)hipEventDestroy(ctx->fork);
    if (ctx->join) (void)hipEventDestroy(ctx->join);
    if (ctx->join3) (void)hipEventDestroy(ctx->join3);
    delete ctx;
}

const char* dbslmm_last_error(const dbslmm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dbslmm_ctx_cache_bed(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len) {
    if (!ctx) return DBSLMM_E_ARG;
    if (!ctx->subs.empty()) return DBSLMM_OK;   // multi-device: each device gets its own rows
    ARG_CHECK(ctx, (bed == nullptr) == (bed_len == 0) && bed_len >= 0, "bed / bed_len");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bed_cache.reset();
    ctx->img_cache = PanelImage{};   // plans created from the old image keep their reference
    ctx->bed_host = nullptr;
    ctx->bed_host_len = 0;
    ctx->bed_from_fd = false;
    if (!bed) return DBSLMM_OK;
    uint8_t* d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, bed_len + kBedPad));
    ctx->bed_cache = dev_shared(d, ctx->device);
    HIP_TRY(ctx, hipMemsetAsync(d + bed_len, 0, kBedPad, ctx->stream));
    HIP_TRY(ctx, upload_staged(d, bed, bed_len, ctx->stream));
    ctx->bed_host = bed;
    ctx->bed_host_len = bed_len;
    return DBSLMM_OK;
}

int dbslmm_ctx_cache_bed_fd(dbslmm_ctx* ctx, int fd, int64_t bed_len, const uint8_t* key) {
    if (!ctx) return DBSLMM_E_ARG;
    if (!ctx->subs.empty()) return DBSLMM_OK;   // multi-device: each device gets its own rows
    ARG_CHECK(ctx, fd >= 0 && key && bed_len > 0, "fd / bed_len / key");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bed_cache.reset();
    ctx->img_cache = PanelImage{};
    ctx->bed_host = nullptr;
    ctx->bed_host_len = 0;
    ctx->bed_from_fd = false;
    uint8_t* d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, bed_len + kBedPad));
    ctx->bed_cache = dev_shared(d, ctx->device);
    HIP_TRY(ctx, hipMemsetAsync(d + bed_len, 0, kBedPad, ctx->stream));
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

void dbslmm_plan_destroy(dbslmm_plan* p) {
    if (!p) return;
    if (p->mp) {
        mp_destroy(p);
        delete p;
        return;
    }
    (void)hipSetDevice(p->ctx->device);
    if (p->h_pin) (void)hipHostFree(p->h_pin);
    if (p->h_pmon) (void)hipHostFree(p->h_pmon);
    if (p->h_mir) (void)hipHostFree(p->h_mir);
    if (p->h_mflag) (void)hipHostFree(p->h_mflag);
    if (p->so_ev) (void)hipEventDestroy(p->so_ev);
    p->img = PanelImage{};                      // (shared with the context when it came from its cache)
    for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->dl_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->tev) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->tev_rest) (void)hipEventDestroy(e);
    if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
    if (p->graph_multi) (void)hipGraphExecDestroy(p->graph_multi);
    for (hipGraphExec_t g : p->graph_copy)
        if (g) (void)hipGraphExecDestroy(g);
    for (hipGraphExec_t g : p->graph_rest)
        if (g) (void)hipGraphExecDestroy(g);
    delete p;                                   // (its DevBufs frees the device buffers)
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
    p->solver = op.solver;
    p->pcg_fused = op.pcg_whole >= 0;
    p->stream_out = op.stream_out >= 0;
    p->pcg_block_wgs = op.pcg_block_wgs;
    if (op.pcg_tol > 0.0) p->pcg_tol = std::max(1e-15, op.pcg_tol);
    if (op.pcg_maxit > 0) p->pcg_maxit = op.pcg_maxit;
    p->pcg_g16 = 4 * static_cast<int64_t>(pr->n_ref) <= 65535;
    p->h2f_mode = op.h2f_mode;
    p->cheb_fused = op.cheb_fused == 1;
    p->h2f_cg = op.h2f_iter != 1;
    p->debug_delay_us = op.debug_delay_us;
    p->debug_stop = op.debug_stop;
    if (op.cheb_tol > 0.0) p->cheb_tol = std::max(1e-16, op.cheb_tol);

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
    if ((e = p->bufs.upload(&p->d_slot_pos, L.slot_pos, ctx->stream)) != hipSuccess) return fail("upload slots");
    if ((e = p->bufs.upload(&p->d_slot_block, L.slot_block, ctx->stream)) != hipSuccess) return fail("upload slots");
    if ((e = p->bufs.upload(&p->d_slot_out, p->h_slot_out, ctx->stream)) != hipSuccess) return fail("upload slots");
    if ((e = p->bufs.upload(&p->d_z, L.z, ctx->stream)) != hipSuccess) return fail("upload z");
    if ((e = p->bufs.upload(&p->d_row0, p->h_row0, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_m, p->h_m, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_ms, p->h_ms, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_ld, p->h_ld, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_matoff, p->h_matoff, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_blk_id, p->h_blk_id, ctx->stream)) != hipSuccess) return fail("upload blocks");
    if ((e = p->bufs.upload(&p->d_order, L.order, ctx->stream)) != hipSuccess) return fail("upload order");
    if ((e = p->bufs.upload(&p->d_tiles, L.tiles, ctx->stream)) != hipSuccess) return fail("upload tiles");
    if ((e = p->bufs.upload(&p->d_btiles, L.btiles, ctx->stream)) != hipSuccess) return fail("upload tiles");
    if ((e = p->bufs.upload(&p->d_htiles, L.htiles, ctx->stream)) != hipSuccess) return fail("upload tiles");
    if ((e = p->bufs.upload(&p->d_tlist, L.tlist, ctx->stream)) != hipSuccess) return fail("upload tiled lists");
    if ((e = p->bufs.upload(&p->d_tri_f, L.tri_f, ctx->stream)) != hipSuccess) return fail("upload trsv lists");
    if ((e = p->bufs.upload(&p->d_tri_b, L.tri_b, ctx->stream)) != hipSuccess) return fail("upload trsv lists");
    if ((e = p->bufs.upload(&p->d_foff, L.foff, ctx->stream)) != hipSuccess) return fail("upload trsv lists");
    if ((e = p->bufs.upload(&p->d_tb, p->h_tb, ctx->stream)) != hipSuccess) return fail("upload trsv lists");
    if (!L.tcheb_list.empty() && (e = p->bufs.upload(&p->d_tcheb_blocks, L.tcheb_list, ctx->stream)) != hipSuccess)
        return fail("upload trsv lists");
    // [tile flags | ticket counter | error word | spare]
    if ((e = p->bufs.zeroed(&p->d_tflags, p->n_tflags + 3, ctx->stream)) != hipSuccess) return fail("hipMalloc trsv flags");
    if ((e = p->bufs.zeroed(&p->d_tepi, p->n_tflags, ctx->stream)) != hipSuccess) return fail("hipMalloc trsv flags");
    if ((e = p->bufs.alloc(&p->d_S, p->n_slots)) != hipSuccess) return fail("hipMalloc stats");
    if ((e = p->bufs.alloc(&p->d_mu, p->n_slots)) != hipSuccess) return fail("hipMalloc stats");
    if ((e = p->bufs.alloc(&p->d_rsd, p->n_slots)) != hipSuccess) return fail("hipMalloc stats");
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
    p->timing = enable != 0;
    for (double& v : p->ms_acc) v = 0.0;
    p->ms_runs = 0;
    if (p->mp)
        for (auto& sh : p->mp->shards) dbslmm_plan_enable_timing(sh.plan, enable);
    return DBSLMM_OK;
}

static int collect_timing(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    for (int r = 0; r < p->runs_pending; ++r) {
        hipEvent_t* e = &p->ev[kEvCount * r];
        // event times from the run's start; with split substitutions the tiled factorisation +
        // backward of the two groups ends on two streams (kEvTiledEnd: lead, kEvRestEnd: rest) and
        // the Chebyshev passes start there: tiled = kEvTiledBegin -> the later of the two, trsv =
        // the earlier of the two -> kEvEnd (the spans overlap)
        float t[kEvCount] = {0.f};
        if (r < static_cast<int>(p->run_route.size()) && p->run_route[r]) {
            // PCG: statistics, Gram, iterations; the only instants this route records
            for (Ev k : {kEvStatsEnd, kEvGramEnd, kEvPcgBlockBegin, kEvPcgBlockEnd, kEvEnd})
                HIP_TRY(ctx, hipEventElapsedTime(&t[k], e[kEvStart], e[k]));
            float span[DBSLMM_K_COUNT] = {0.f};
            span[DBSLMM_K_UNPACK] = t[kEvStatsEnd];
            span[DBSLMM_K_GRAM] = t[kEvGramEnd] - t[kEvStatsEnd];
            span[DBSLMM_K_PCG] = t[kEvEnd] - t[kEvGramEnd];
            span[DBSLMM_K_PCG_BLOCK] = t[kEvPcgBlockEnd] - t[kEvPcgBlockBegin];   // (inside the PCG span, on the second stream)
            for (int k = 0; k < DBSLMM_K_COUNT; ++k) p->ms_acc[k] += span[k];
            p->ms_runs++;
            continue;
        }
        for (int k = 1; k < kEvCount; ++k) HIP_TRY(ctx, hipEventElapsedTime(&t[k], e[kEvStart], e[k]));
        const float fend = std::max(t[kEvTiledEnd], t[kEvRestEnd]), cstart = std::min(t[kEvTiledEnd], t[kEvRestEnd]);
        float span[DBSLMM_K_COUNT] = {t[kEvStatsEnd], t[kEvGramEnd] - t[kEvStatsEnd], t[kEvLargeEnd] - t[kEvGramEnd],
                                      t[kEvSmallEnd] - t[kEvSmallBegin], fend - t[kEvTiledBegin], t[kEvEnd] - cstart, 0.f, 0.f};
        for (int k = 0; k < DBSLMM_K_COUNT; ++k) p->ms_acc[k] += span[k];
        // the lead group's Gram sits inside the statistics span (kEvStart -> kEvStatsEnd)
        float lg = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&lg, e[kEvLeadGramBegin], e[kEvLeadGramEnd]));
        p->ms_acc[0] -= lg;
        p->ms_acc[1] += lg;
        p->ms_runs++;
    }
    p->runs_pending = 0;
    p->run_route.clear();
    return DBSLMM_OK;
}

// The stream pair and event set of a tiled sequence: the lead / only sequence runs on stream2
// (chain, high priority) + stream3 (bulk trailing), the rest sequence on stream4 + stream5.
struct TSeq {
    hipStream_t chain, bulk;
    std::vector<hipEvent_t>* tev;
};
static TSeq seq_main(dbslmm_plan* p) { return TSeq{p->ctx->stream2, p->ctx->stream3, &p->tev}; }
static TSeq seq_rest(dbslmm_plan* p) { return TSeq{p->ctx->stream4, p->ctx->stream5, &p->tev_rest}; }

// dbslmm_options.debug_delay_us (tests): a spin kernel at the head of a stream segment.  side > 0:
// the concurrent side (bulk trailing launches, the rest sequence, the main stream after the lead
// fork) runs late; side < 0: the critical side (chain launches, the lead sequence).
static void debug_spin(const dbslmm_plan* p, hipStream_t st, int side) {
    const int32_t d = p->debug_delay_us;
    if (d == 0 || (d > 0) != (side > 0)) return;
    const int64_t ticks = 100 * static_cast<int64_t>(d > 0 ? d : -d);   // 100 MHz counter
    hipLaunchKernelGGL(dbslmm_debug_spin, dim3(1), dim3(64), 0, st, ticks);
}

// Enqueue a tiled launch list on its stream pair.
// copy: the list is a single-copy list applied to factorisation copy `copy` (its matrix, sigma
// scalar, scratch, betas and status); multi-copy lists address the copies themselves (copy 0).
static int enqueue_tiled(dbslmm_plan* p, double isn, const std::vector<TLaunch>& tl, const int32_t* d_tlist,
                         int copy, const TSeq& sq) {
    dbslmm_ctx* ctx = p->ctx;
    const int64_t c = copy;
    const chol::TiledArgs ta{p->d_M + c * p->M_elems, p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff,
                             p->d_blk_id, p->d_z, p->d_slot_out, p->d_rsd, p->d_dshift + c, isn,
                             p->d_y + c * p->n_slots, p->d_beta_s + c * p->n_s, p->d_beta_l + c * p->n_l,
                             p->d_status + c * p->nbk, p->n_nonempty,
                             p->M_elems, p->n_slots, p->n_s, p->n_l, p->nbk};
    int nev = 0;
    for (const TLaunch& L : tl)
        if (L.kind == kTlRecord) nev = std::max(nev, L.step + 1);
    std::vector<hipEvent_t>& tev = *sq.tev;
    while (static_cast<int>(tev.size()) < nev) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        tev.push_back(e);
    }
    for (const TLaunch& L : tl) {
        hipStream_t st = L.strm ? sq.bulk : sq.chain;
        if (L.kind == kTlRecord) { HIP_TRY(ctx, hipEventRecord(tev[L.step], st)); continue; }
        if (L.kind == kTlWait) { HIP_TRY(ctx, hipStreamWaitEvent(st, tev[L.step], 0)); continue; }
        if (L.items == 0) continue;
        const int32_t* act = d_tlist + L.off;
        const dim3 g(static_cast<unsigned>(L.items)), blk(chol::kLargeThreads);
        if (p->debug_delay_us) debug_spin(p, st, L.strm ? 1 : -1);
        switch (L.kind) {
        case 4: hipLaunchKernelGGL(dbslmm_tchol_region, g, blk, kRegionLds, st, ta, act, L.items); break;
        case 1: hipLaunchKernelGGL(dbslmm_tchol_panel, g, blk, kTiledLds, st, ta, act, L.items); break;
        default: hipLaunchKernelGGL(dbslmm_tchol_trailing3k16, g, dim3(512), kTrail3Lds, st, ta, L.n, act, L.items); break;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
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
    // captured graphs hold the old pointers
    if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
    if (p->graph_multi) (void)hipGraphExecDestroy(p->graph_multi);
    p->graph_exec = p->graph_multi = nullptr;
    for (hipGraphExec_t& g : p->graph_copy)
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (hipGraphExec_t& g : p->graph_rest)
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    return DBSLMM_OK;
}

extern "C++" {
template <int NR>
static void launch_trsv(bool fwd, int grid, hipStream_t st, const trsv::Args& a) {
    if (fwd) hipLaunchKernelGGL(dbslmm_trsv_fwd<NR>, dim3(grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
    else hipLaunchKernelGGL(dbslmm_trsv_bwd<NR>, dim3(grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
}
}

// Backward substitution of factorisation copy `copy`'s tiled blocks in one persistent launch
// (trsv.hip, plain mode): y = the bordered z row, x -> y scratch of the copy, beta of the copy.
// A set of tiled blocks whose substitutions run as one launch sequence: items [item_off,
// item_off + n_items) of d_tri_f / d_tri_b, blocks [tb_off, tb_off + n_tb) of d_tb, on stream st
// with ticket counter ctr
struct TGroup {
    int32_t item_off, n_items, tb_off, n_tb;
    hipStream_t st;
    int32_t* ctr;
    int grid;
};
static TGroup tgroup_all(const dbslmm_plan* p) {
    return TGroup{0, p->n_titems, 0, p->n_tiled, p->ctx->stream2, p->d_tflags + p->n_tflags,
                  std::max(1, std::min(p->ctx->n_cu, p->n_titems))};
}
// split substitutions: the lead group on stream2 (ticket counter after the flags), the rest group
// on the rest sequence's stream (its own counter: the spare word after the error word)
static TGroup tgroup_lead(const dbslmm_plan* p) {
    const int g = p->sub_grid_lead;
    return TGroup{0, p->n_titems_lead, 0, p->n_tb_lead, p->ctx->stream2, p->d_tflags + p->n_tflags,
                  std::max(1, std::min(g, p->n_titems_lead))};
}
static TGroup tgroup_rest(const dbslmm_plan* p) {
    const int g = p->sub_grid_rest;
    const int32_t ni = p->n_titems - p->n_titems_lead;
    return TGroup{p->n_titems_lead, ni, p->n_tb_lead, p->n_tiled - p->n_tb_lead, p->ctx->stream4,
                  p->d_tflags + p->n_tflags + 2, std::max(1, std::min(g, ni))};
}
// The substitution epochs of one run (tile-flag values, trsv.hip): run_impl resets the flags ahead
// of the fork whenever the counter is within kEpochsPerRun of wrapping, so inside a run the counter
// only grows.  Bound: 64 copies' backward solves + 2 groups x 32 copy groups x 2 x 60 passes.
static int next_epoch(dbslmm_plan* p, int k) {
    if (p->trsv_epoch > INT32_MAX - k) {   // unreachable unless a run exceeds kEpochsPerRun
        p->ctx->err = "substitution epoch counter overflow within one run";
        return DBSLMM_E_STATE;
    }
    p->trsv_epoch += k;
    return DBSLMM_OK;
}

static int run_pbwd(dbslmm_plan* p, double isn, int copy, const TGroup& grp) {
    dbslmm_ctx* ctx = p->ctx;
    hipStream_t st = grp.st;
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    if (!p->d_cheb) {
        std::lock_guard<std::mutex> lk(g_capture_mu);
        HIP_TRY(ctx, p->bufs.alloc(&p->d_cheb, 6 * trsv::kMaxR * vs));
    }
    const int64_t c = copy;
    trsv::Args a{};
    a.M = p->d_M + c * p->M_elems;
    a.matoff = p->d_matoff;
    a.ld = p->d_ld;
    a.m = p->d_m;
    a.ms = p->d_ms;
    a.row0 = p->d_row0;
    a.blk_id = p->d_blk_id;
    a.slot_out = p->d_slot_out;
    a.items = p->d_tri_b + 2 * grp.item_off;
    a.n_items = grp.n_items;
    a.grid = grp.grid;
    a.foff = p->d_foff;
    a.flags = p->d_tflags;
    a.ctr = grp.ctr;
    a.err = p->d_tflags + p->n_tflags + 1;
    a.vs = vs;
    a.dst = p->d_cheb + trsv::kMaxR * vs;          // the Z hand-off buffer
    a.X = p->d_y + c * p->n_slots;
    a.inv_sqrt_n = isn;
    a.beta_s = p->d_beta_s;
    a.beta_l = p->d_beta_l;
    a.ns_stride = p->n_s;
    a.nl_stride = p->n_l;
    a.cix[0] = copy;
    a.status = p->d_status + c * p->nbk;
    a.mode = 1;
    if (const int rc = next_epoch(p, 1)) return rc;
    a.epoch = p->trsv_epoch;
    if (a.n_items > 0) {
        launch_trsv<1>(false, a.grid, st, a);
        p->trsv_pending = true;
    }
    HIP_TRY(ctx, hipGetLastError());
    return DBSLMM_OK;
}

// Capture a launch list into a graph on its chain stream (once; sigma is read from device scalars,
// so the graph stays valid) and replay it.  A plan's first run enqueues the list launch by launch:
// a plan solved once (the dbslmm CLI) never pays the capture and instantiation of the few-hundred-
// node graphs; repeated runs replay from the second on (the same launches: bit-identical).
static int launch_graph(dbslmm_plan* p, double isn, const std::vector<TLaunch>& tl, const int32_t* d_tlist,
                        int copy, hipGraphExec_t& gx, const TSeq& sq) {
    dbslmm_ctx* ctx = p->ctx;
    if (!gx && p->n_runs == 0) return enqueue_tiled(p, isn, tl, d_tlist, copy, sq);
    if (!gx) {
        std::lock_guard<std::mutex> lk(g_capture_mu);
        hipGraph_t gr = nullptr;
        HIP_TRY(ctx, hipStreamBeginCapture(sq.chain, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_tiled(p, isn, tl, d_tlist, copy, sq);
        hipError_t ce = hipStreamEndCapture(sq.chain, &gr);
        if (rc != DBSLMM_OK) {
            if (gr) (void)hipGraphDestroy(gr);
            return rc;
        }
        HIP_TRY(ctx, ce);
        hipError_t ie = hipGraphInstantiate(&gx, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        HIP_TRY(ctx, ie);
    }
    HIP_TRY(ctx, hipGraphLaunch(gx, sq.chain));
    return DBSLMM_OK;
}

// The single-copy tiled sequence on factorisation copy `copy` (stream2, one graph per copy).
// With a lead group this is the lead group's sequence; the rest sequence (run_rest_copy) runs on
// stream4 and stream2 waits for it before the backward substitution (run_pbwd).
static int run_tiled_copy(dbslmm_plan* p, double isn, int copy) {
    if (static_cast<int>(p->graph_copy.size()) <= copy) p->graph_copy.resize(copy + 1, nullptr);
    return launch_graph(p, isn, p->tl, p->d_tlist, copy, p->graph_copy[copy], seq_main(p));
}
static int run_rest_copy(dbslmm_plan* p, double isn, int copy) {
    if (static_cast<int>(p->graph_rest.size()) <= copy) p->graph_rest.resize(copy + 1, nullptr);
    return launch_graph(p, isn, p->tl_rest, p->d_tlist, copy, p->graph_rest[copy], seq_rest(p));
}

// ---- h2f tuning by Chebyshev on one factor (trsv.hip)
struct ChebPlan {
    int base = -1;
    double db = 0.0;                  // the base copy's shift d_b = 1 / (sigma_b n)
    std::vector<int> others;          // copies solved by iteration, in launch groups of kMaxR
    std::vector<int> iters;           // per group
    std::vector<char> capped;         // per group: pcg_maxit cut CG's cap below the a priori count
    std::vector<double> coef;         // per group: [iters][nr][3] {alpha, beta, delta}
    std::vector<size_t> coef_off;
};

// Base = the median of the shifts d_c = 1/(sigma_c n); per other copy the spectrum of
// M_b^{-1} M_c lies in [1, 1 + delta / (d_b + 1 - tau)] (delta > 0) or its mirror (delta < 0).
// Not applicable (false): tau outside (0, 1], or more than 60 iterations needed.
static bool cheb_plan(const dbslmm_plan* p, const double* sigmas, int n, ChebPlan& cp) {
    if (p->h2f_mode != 0 || n < 2 || (p->n_tiled == 0 && p->n_large == 0) || !(p->tau > 0.0 && p->tau <= 1.0))
        return false;
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return sigmas[a] < sigmas[b]; });
    cp.base = idx[n / 2];
    const double nobs = static_cast<double>(p->n_obs);
    const double db = 1.0 / (sigmas[cp.base] * nobs);
    cp.db = db;
    const double floor_ = db + 1.0 - p->tau;
    const double tol = p->h2f_tol;
    for (int c = 0; c < n; ++c)
        if (c != cp.base) cp.others.push_back(c);
    for (size_t g0 = 0; g0 < cp.others.size(); g0 += trsv::kMaxR) {
        const int nr = static_cast<int>(std::min<size_t>(trsv::kMaxR, cp.others.size() - g0));
        std::vector<double> lo(nr), hi(nr), dl(nr);
        int K = 1;
        for (int j = 0; j < nr; ++j) {
            const double dc = 1.0 / (sigmas[cp.others[g0 + j]] * nobs);
            dl[j] = dc - db;
            const double ext = dl[j] / floor_;
            lo[j] = std::min(1.0, 1.0 + ext) * (1.0 - 1e-6);
            hi[j] = std::max(1.0, 1.0 + ext) * (1.0 + 1e-6);
            if (!(lo[j] > 0.0)) return false;
            // Chebyshev: error <= 2 q^K x the initial error x_c - x_b, itself <= |ext| relative
            // (the same bound); K so that the final error is cheb_tol of the solution (default
            // 1e-9: the parity bar on beta is 1e-5 relative, the reference's own PCG -- absolute
            // residual 1e-7 -- deviates from the exact solution by ~1e-8 normwise, so the
            // iteration adds at most a tenth of the reference's own solver error; 7 iterations
            // at h2f 0.8 / 1 / 1.2, measured error ~0.2 x the target)
            const double kap = hi[j] / lo[j], q = (std::sqrt(kap) - 1.0) / (std::sqrt(kap) + 1.0);
            const double e0 = std::max(std::fabs(ext), 1e-300);
            // (2 q^K e0 <= tol, the 2 included: without it the count came out one short wherever
            // log(tol / e0) / log q fell within log 2 / |log q| below an integer, and the copies of
            // h2f 0.5 on a base of 1.0 / 1.3 measured 1.2e-9 / 1.35e-9 per block -- the bound's own
            // value at that count -- against the target of 1e-9)
            const int k = q < 1e-300 ? 1
                                     : std::max(1, static_cast<int>(std::ceil(std::log(tol / (2.0 * e0)) / std::log(q))));
            K = std::max(K, k);
        }
        if (K > 60) return false;
        // CG (h2f_iter 2) iterates adaptively with the Chebyshev count as its cap.  A copy that ran
        // all K iterations is within the target whatever its stopping test says: 2 q^K e_0 <=
        // cheb_tol holds on an interval that does not depend on the data, and CG's energy-norm
        // error is at most Chebyshev's.  (The stopping test cannot say so at tau = 1: its
        // lambda_min bound of a block with large SNPs, 1 - tau, is 0.)  Only a cap that pcg_maxit
        // cut below K can leave a copy short of the target: DBSLMM_BLOCK_NOT_CONVERGED
        const bool capped = p->h2f_cg && !p->cheb_fused && p->pcg_maxit < K;
        if (capped) K = p->pcg_maxit;
        cp.iters.push_back(K);
        cp.capped.push_back(capped);
        cp.coef_off.push_back(cp.coef.size());
        std::vector<double> rho(nr);
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < nr; ++j) {
                const double th = 0.5 * (hi[j] + lo[j]), de = 0.5 * (hi[j] - lo[j]), sg = th / de;
                double al, be;
                if (k == 0) {
                    rho[j] = 1.0 / sg;
                    al = 0.0;
                    be = 1.0 / th;
                } else {
                    const double rn = 1.0 / (2.0 * sg - rho[j]);
                    al = rn * rho[j];
                    be = 2.0 * rn / de;
                    rho[j] = rn;
                }
                cp.coef.push_back(al);
                cp.coef.push_back(be);
                cp.coef.push_back(dl[j]);
            }
    }
    return true;
}


// Chebyshev iterations of the non-base copies on the base copy's factor (stream2, after the
// base copy's tiled sequence): every tiled block of copy c gets its beta and status.

// Chebyshev coefficients and iteration vectors: uploaded / allocated on stream st before any
// group's iterations (run_impl: on the main stream ahead of the fork)
static int cheb_prepare(dbslmm_plan* p, const ChebPlan& cp, hipStream_t st) {
    dbslmm_ctx* ctx = p->ctx;
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    if (!p->d_cheb) {
        std::lock_guard<std::mutex> lk(g_capture_mu);
        HIP_TRY(ctx, p->bufs.alloc(&p->d_cheb, 6 * trsv::kMaxR * vs));
    }
    if (p->h2f_cg && !p->d_cgconv) {
        std::lock_guard<std::mutex> lk(g_capture_mu);
        const size_t nb = std::max(1, p->n_nonempty);
        HIP_TRY(ctx, p->bufs.alloc(&p->d_cgrec, nb * trsv::kMaxR * 2));
        HIP_TRY(ctx, p->bufs.alloc(&p->d_cgconv, nb));
        HIP_TRY(ctx, p->bufs.alloc(&p->d_cgit, nb));
    }
    // every block's CG pass count starts at 0 each run (the rest group of sub_split = 2 iterates by
    // Chebyshev and never writes it; workload[16] sums it over every tiled block: ADVICE r05)
    if (p->d_cgit) HIP_TRY(ctx, hipMemsetAsync(p->d_cgit, 0, std::max(1, p->n_nonempty) * sizeof(int32_t), st));
    // the coefficients depend only on the sigmas: uploaded when they change, synchronously (the
    // host vector is a temporary of the run; an asynchronous copy from pageable memory may still
    // be pending when it is freed) after every earlier run that reads d_coef has finished
    if (cp.coef == p->h_coef) return DBSLMM_OK;
    std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous copy below
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
    if (p->coef_cap < static_cast<int32_t>(cp.coef.size())) {
        (void)p->bufs.release(p->d_coef);
        HIP_TRY(ctx, p->bufs.alloc(&p->d_coef, cp.coef.size()));
        p->coef_cap = static_cast<int32_t>(cp.coef.size());
    }
    HIP_TRY(ctx, hipMemcpyAsync(p->d_coef, cp.coef.data(), cp.coef.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    p->h_coef = cp.coef;
    return DBSLMM_OK;
}

// Work list of the fused Chebyshev launch (dbslmm_trsv_cheb) for K iterations: every (tiled
// block, pass p < 2K, tile) item, the passes alternating forward (tiles 0 .. T-1) and backward
// (T-1 .. 0).  Keys model when an item can run: a block's chain needs (p T + pos) steps of
// kChainStep, and the bulk of the substitutions streams at kStreamBw, so a block cannot usefully
// run ahead of its share of the bytes either: key = max(chain time, bulk time).  Both grow along
// each block's own order, so every dependency has a smaller ticket (deadlock-free for any
// residency); across blocks the small ones finish their iterations early at the memory bandwidth
// while the largest blocks' chains go on beside them and then alone.
static void build_cheb_items(const dbslmm_plan* p, int K, std::vector<int32_t>& items) {
    constexpr double kChainStep = 4.0e-6, kStreamBw = 5.5e12;
    struct It { double key; int T; int32_t w, I; };
    std::vector<It> v;
    double tb = 0.0;
    for (int32_t b : p->h_tb) {
        const double T = (p->h_m[b] + trsv::kT - 1) / trsv::kT;
        tb += T * (T + 1) / 2 * trsv::kT * trsv::kT * sizeof(double);
    }
    const double t_bw = 2.0 * K * tb / kStreamBw;
    for (int32_t b : p->h_tb) {
        const int T = (p->h_m[b] + trsv::kT - 1) / trsv::kT;
        for (int ps = 0; ps < 2 * K; ++ps)
            for (int pos = 0; pos < T; ++pos) {
                const double chain = (static_cast<double>(ps) * T + pos) * kChainStep;
                const double bulk = (ps + static_cast<double>(pos) / T) / (2.0 * K) * t_bw;
                v.push_back({std::max(chain, bulk), T, b | (ps << 16), (ps & 1) ? T - 1 - pos : pos});
            }
    }
    std::stable_sort(v.begin(), v.end(), [](const It& x, const It& y) {
        return x.key != y.key ? x.key < y.key : x.T > y.T;
    });
    items.clear();
    items.reserve(2 * v.size());
    for (const It& x : v) {
        items.push_back(x.w);
        items.push_back(x.I);
    }
}

// Passes: one launch per forward / backward pass (default), or, with dbslmm_options.cheb_fused = 1
// (experimental: measured slower at config 4, 15.9 vs 13.9 ms -- every pass there is
// bound by the largest block's 150-tile chain and by the streaming bandwidth alike, and the fused
// items' own-input waits and update hand-offs cost more than the launch boundaries they remove),
// all 2K passes of a group in one dbslmm_trsv_cheb launch over the whole plan (grp = tgroup_all).
static int run_cheb(dbslmm_plan* p, double isn, const ChebPlan& cp, const TGroup& grp) {
    dbslmm_ctx* ctx = p->ctx;
    hipStream_t st = grp.st;
    if (grp.n_items == 0) return DBSLMM_OK;
    const bool fused = p->cheb_fused && grp.item_off == 0 && grp.n_items == p->n_titems;
    const bool cg = p->h2f_cg && !fused;   // (the fused launch iterates by Chebyshev)
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    const int64_t blk = trsv::kMaxR * vs;
    double *Y = p->d_cheb, *Z = Y + blk, *X = Z + blk, *R = X + blk, *D = R + blk, *S = D + blk;
    for (size_t g = 0; g < cp.iters.size(); ++g) {
        const size_t g0 = g * trsv::kMaxR;
        const int nr = static_cast<int>(std::min<size_t>(trsv::kMaxR, cp.others.size() - g0));
        const int K = cp.iters[g];
        int cix[trsv::kMaxR] = {0, 0};
        for (int j = 0; j < nr; ++j) cix[j] = cp.others[g0 + j];
        const double* coef = p->d_coef + cp.coef_off[g];
        if (fused && p->cheb_items_K != K) {   // the work list of K iterations (cached: K depends on the sigmas)
            std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous upload below
            std::vector<int32_t> items;
            build_cheb_items(p, K, items);
            HIP_TRY(ctx, hipStreamSynchronize(st));
            (void)p->bufs.release(p->d_cheb_items);
            HIP_TRY(ctx, p->bufs.upload(&p->d_cheb_items, items, ctx->stream));
            p->n_cheb_items = static_cast<int32_t>(items.size() / 2);
            p->cheb_items_K = K;
        }
        hipLaunchKernelGGL(dbslmm_cheb_init, dim3(grp.n_tb), dim3(256), 0, st, p->d_tb + grp.tb_off, p->d_row0, p->d_m,
                           p->d_ms, p->d_blk_id, p->d_y + static_cast<int64_t>(cp.base) * p->n_slots, coef,
                           nr, vs, X, R, D, S, p->d_status + cp.base * p->nbk, p->d_status, p->nbk,
                           cix[0], cix[1], cg ? p->d_cgconv : nullptr, cg && g == 0 ? p->d_cgit : nullptr);
        HIP_TRY(ctx, hipGetLastError());
        trsv::Args a{};
        a.M = p->d_M + static_cast<int64_t>(cp.base) * p->M_elems;
        a.matoff = p->d_matoff;
        a.ld = p->d_ld;
        a.m = p->d_m;
        a.ms = p->d_ms;
        a.row0 = p->d_row0;
        a.blk_id = p->d_blk_id;
        a.slot_out = p->d_slot_out;
        a.grid = grp.grid;
        a.foff = p->d_foff;
        a.flags = p->d_tflags;
        a.epi = p->d_tepi;
        a.ctr = grp.ctr;
        a.err = p->d_tflags + p->n_tflags + 1;
        a.vs = vs;
        a.X = X;
        a.R = R;
        a.D = D;
        a.S = S;
        a.Y = Y;
        a.Z = Z;
        a.coef = coef;
        a.iters = K;
        a.inv_sqrt_n = isn;
        a.beta_s = p->d_beta_s;
        a.beta_l = p->d_beta_l;
        a.ns_stride = p->n_s;
        a.nl_stride = p->n_l;
        for (int j = 0; j < trsv::kMaxR; ++j) a.cix[j] = cix[j];
        a.status = p->d_status + cp.base * p->nbk;
#ifdef DBSLMM_DIAG   // diagnostic build: per-tile stamps of the largest tiled block
        if (getenv("DBSLMM_TRSV_STAMPS")) {
            int bmax = p->h_tb[0];
            for (int32_t b : p->h_tb) if (p->h_m[b] > p->h_m[bmax]) bmax = b;
            if (!p->d_stamps) HIP_TRY(ctx, p->bufs.alloc(&p->d_stamps, 8 * 4096));
            a.stamps = p->d_stamps;
            a.stamp_b = bmax;
        }
#endif
        if (!fused) {   // one launch per pass (the launch boundary orders the passes)
            a.n_items = grp.n_items;
            trsv::CGArgs ca{};
            if (cg) {   // K (the a priori Chebyshev count) caps the iterations
                a.mode = 2;
                a.conv = p->d_cgconv;
                ca.tb = p->d_tb + grp.tb_off;
                ca.row0 = p->d_row0;
                ca.m = p->d_m;
                ca.ms = p->d_ms;
                ca.blk_id = p->d_blk_id;
                ca.slot_out = p->d_slot_out;
                ca.st_base = a.status;
                ca.nr = nr;
                ca.vs = vs;
                ca.Z = Z;
                ca.X = X;
                ca.R = R;
                ca.D = D;
                ca.S = S;
                for (int j = 0; j < nr; ++j) {
                    ca.delta[j] = cp.coef[cp.coef_off[g] + 3 * j + 2];
                    ca.floor_s[j] = cp.db + ca.delta[j] + 1.0 - p->tau;
                    ca.cix[j] = cix[j];
                }
                ca.floor_l = 1.0 - p->tau;
                ca.tol = p->h2f_tol;
                ca.capped = cp.capped[g];
                ca.rec = p->d_cgrec;
                ca.conv = p->d_cgconv;
                ca.iters = p->d_cgit;
                ca.inv_sqrt_n = isn;
                ca.beta_s = p->d_beta_s;
                ca.beta_l = p->d_beta_l;
                ca.ns_stride = p->n_s;
                ca.nl_stride = p->n_l;
                ca.status = p->d_status;
                ca.st_stride = p->nbk;
            }
            for (int k = 0; k < K; ++k) {
                for (int pass = 0; pass < 2; ++pass) {
                    const bool fwd = pass == 0;
                    if (const int rc = next_epoch(p, 1)) return rc;
                    a.epoch = p->trsv_epoch;
                    a.items = (fwd ? p->d_tri_f : p->d_tri_b) + 2 * grp.item_off;
                    a.src = fwd ? R : Y;
                    a.dst = fwd ? Y : Z;
                    a.coef = coef + static_cast<int64_t>(k) * nr * 3;
                    a.last = k == K - 1;
                    if (nr == 1) launch_trsv<1>(fwd, a.grid, st, a);
                    else launch_trsv<2>(fwd, a.grid, st, a);
                    HIP_TRY(ctx, hipGetLastError());
                    p->trsv_pending = true;
                }
                if (cg) {
                    ca.k = k;
                    ca.last = k == K - 1;
                    hipLaunchKernelGGL(dbslmm_cg_update, dim3(grp.n_tb), dim3(trsv::kCGThreads), 0, st, ca);
                    HIP_TRY(ctx, hipGetLastError());
                }
            }
            continue;
        }
        a.fused = 1;
        a.items = p->d_cheb_items;
        a.n_items = p->n_cheb_items;
        a.grid = std::max(1, std::min(ctx->n_cu, p->n_cheb_items));
        // passes 0 .. 2K-1 run at epochs epoch .. epoch + 2K - 1 (flags and update flags only grow)
        a.epoch = p->trsv_epoch + 1;
        if (const int rc = next_epoch(p, 2 * K)) return rc;
        if (nr == 1) hipLaunchKernelGGL(dbslmm_trsv_cheb<1>, dim3(a.grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
        else hipLaunchKernelGGL(dbslmm_trsv_cheb<2>, dim3(a.grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
        HIP_TRY(ctx, hipGetLastError());
        p->trsv_pending = true;
    }
    return DBSLMM_OK;
}

// The rest group's Chebyshev copies as whole-block launches (sub_split = 2, trsv.hip dbslmm_tcheb):
// per copy group one launch, one workgroup per block, every iteration inside; same state vectors,
// coefficients and outputs as run_cheb's passes.
static int run_tcheb(dbslmm_plan* p, double isn, const ChebPlan& cp, hipStream_t st) {
    dbslmm_ctx* ctx = p->ctx;
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    const int64_t blk = trsv::kMaxR * vs;
    double *X = p->d_cheb + 2 * blk, *R = X + blk, *D = R + blk, *S = D + blk;
    for (size_t g = 0; g < cp.iters.size(); ++g) {
        const size_t g0 = g * trsv::kMaxR;
        const int nr = static_cast<int>(std::min<size_t>(trsv::kMaxR, cp.others.size() - g0));
        TChebArgs a{};
        a.M = p->d_M + static_cast<int64_t>(cp.base) * p->M_elems;
        a.matoff = p->d_matoff;
        a.ld = p->d_ld;
        a.m = p->d_m;
        a.ms = p->d_ms;
        a.row0 = p->d_row0;
        a.blk_id = p->d_blk_id;
        a.slot_out = p->d_slot_out;
        a.blocks = p->d_tcheb_blocks;
        a.n_blocks = p->n_tcheb;
        a.iters = cp.iters[g];
        a.vld = p->tcheb_vld;
        a.vs = vs;
        a.x_base = p->d_y + static_cast<int64_t>(cp.base) * p->n_slots;
        a.X = X;
        a.R = R;
        a.D = D;
        a.S = S;
        a.coef = p->d_coef + cp.coef_off[g];
        a.inv_sqrt_n = isn;
        a.beta_s = p->d_beta_s;
        a.beta_l = p->d_beta_l;
        a.ns_stride = p->n_s;
        a.nl_stride = p->n_l;
        for (int j = 0; j < trsv::kMaxR; ++j) a.cix[j] = j < nr ? cp.others[g0 + j] : cp.others[g0];
        a.st_base = p->d_status + cp.base * p->nbk;
        a.status = p->d_status;
        a.st_stride = p->nbk;
        const size_t lds = (static_cast<size_t>(nr) * a.vld + trsv::kT * nr) * sizeof(double);
        if (nr == 1) hipLaunchKernelGGL(dbslmm_tcheb<1>, dim3(p->n_tcheb), dim3(trsv::kBThreads), lds, st, a);
        else hipLaunchKernelGGL(dbslmm_tcheb<2>, dim3(p->n_tcheb), dim3(trsv::kBThreads), lds, st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    return DBSLMM_OK;
}

// ---------------------------------------------------------------- PCG route (pcg.hip)
// Does this run take the PCG route?  solver 2 forces it and 0 (auto) picks it when every copy's
// prior shift d_c = 1/(sigma_c n) keeps the system well conditioned (d_c >= kPcgDmin: kappa <=
// 1 + lambda_LD / (d + 1 - tau) ~ 6 at lambda_LD ~ 10, tools/cg_gate.py); both need a data-free
// lower bound on lambda_min (tau < 1, or no large SNPs: then d_c + 1 - tau), at most
// pcg::kMaxNC copies and no debug stop after the Gram.
constexpr double kPcgDmin = 2.0;
// ... every condition but the number of copies
static bool pcg_eligible(const dbslmm_plan* p, const double* sigmas, int n) {
    if (p->force_factor || p->solver == 1 || p->n_nonempty == 0 || p->debug_stop) return false;
    if (!(p->tau > 0.0 && p->tau <= 1.0) || (p->tau >= 1.0 && p->has_large)) return false;
    if (p->solver == 2) return true;
    for (int c = 0; c < n; ++c)
        if (1.0 / (sigmas[c] * static_cast<double>(p->n_obs)) < kPcgDmin) return false;
    return true;
}
static bool pcg_route(const dbslmm_plan* p, const double* sigmas, int n) {
    return n <= pcg::kMaxNC && pcg_eligible(p, sigmas, n);
}

// Lay the PCG buffers out for n copies: per block its tile rows (128 slots), the product's work
// items (runs of up to kRunMax tiles along a tile row, biggest blocks first), vectors [6][copy][slots],
// partial slots, dots and the recurrence state.
static int pcg_layout(dbslmm_plan* p, int n) {
    dbslmm_ctx* ctx = p->ctx;
    if (p->pcg_g16 && !p->d_G16) {
        // the integer Gram: block b at off16, Tb 128 x Tb 128, zero past m (set once: the Gram
        // writes only rows and columns < m), so the product reads whole 16-B row segments unmasked
        std::vector<int64_t> off;
        std::vector<int32_t> ldv;
        int64_t o = 0;
        for (int b = 0; b < p->n_nonempty; ++b) {
            const int64_t l = (p->h_m[b] + pcg::kT - 1) / pcg::kT * pcg::kT;
            off.push_back(o);
            ldv.push_back(static_cast<int32_t>(l));
            o += l * l;
        }
        const size_t e = static_cast<size_t>(o) + 256;
        HIP_TRY(ctx, p->bufs.zeroed(&p->d_G16, e, ctx->stream));
        HIP_TRY(ctx, p->bufs.upload(&p->d_off16, off, ctx->stream));
        HIP_TRY(ctx, p->bufs.upload(&p->d_ld16, ldv, ctx->stream));
        p->h_off16 = off;
    }
    if (!p->h_pmon) HIP_TRY(ctx, hipHostMalloc(&p->h_pmon, (1 + std::max(1, p->n_nonempty)) * sizeof(int32_t),
                                               hipHostMallocDefault));
    if (p->pcg_n == n) return DBSLMM_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the old layout's buffers go, each member null from here on: a failure below leaves nothing dangling
    // (d_pflist is uploaded again only when some block is solved whole)
    DevBufs& B = p->bufs;
    B.release_all(p->d_pblk, p->d_pitem, p->d_prow, p->d_pvec, p->d_ppart, p->d_pdot, p->d_pqs, p->d_pcnv,
                  p->d_pitb, p->d_pdone, p->d_pact, p->d_pflist, p->d_pfin);
    p->pcg_n = 0;                        // (no layout until the new one is complete)
    p->pcg_trim = false;                 // (until a run of this layout has read the flags)
    using namespace pcg;
    std::vector<PcgBlk> blk;
    std::vector<int2> flist;             // (block, copy) sequences solved whole by dbslmm_pcg_block
    std::vector<double> mat, part;
    std::vector<int4> items;
    std::vector<int2> rows;
    int64_t vo = 0, po = 0, dof = 0;
    int32_t sco = 0;
    const double esz = p->pcg_g16 ? 2.0 : 8.0;
    // tiles per product item: one (measured at config 4: 10.65 / 10.90 / 11.13 / 11.34 ms per step
    // at 1 / 2 / 4 / 8, and the N = 8 shards' product 114 -> ~45 us: many short items keep more
    // row segments in flight than a few long ones)
    int run = 1;
    p->pcg_run = run;
    for (int b = 0; b < p->n_nonempty; ++b) {
        const int32_t m = p->h_m[b], Tb = (m + kT - 1) / kT, nrun = (Tb + run - 1) / run;
        // a block without large SNPs solves n scalar shifts of one matrix: one Krylov sequence
        // (multi-shift CG, one product column); with large SNPs each copy iterates on its own
        const bool msh = n > 1 && p->h_ms[b] == m;
        const int32_t nc = msh ? 1 : n;
        const bool fused = p->pcg_fused && Tb <= kFTb && !p->h_off16.empty();
        PcgBlk k{b, p->h_row0[b], m, p->h_ms[b], p->h_ld[b], Tb, Tb + nrun, sco, p->h_matoff[b], vo, po, dof,
                 p->h_off16.empty() ? 0 : p->h_off16[b], nc, msh ? 1 : 0, fused ? 1 : 0, 0};
        if (fused) {   // one entry per Krylov sequence: copy -1 = every copy (multi-shift, or one copy)
            const int32_t bi = static_cast<int32_t>(blk.size());
            if (nc == 1) flist.push_back(int2{bi, msh ? -1 : 0});
            else for (int c = 0; c < nc; ++c) flist.push_back(int2{bi, c});
        }
        const int bi = static_cast<int>(blk.size());
        blk.push_back(k);
        vo += static_cast<int64_t>(Tb) * kT;
        po += static_cast<int64_t>(Tb) * k.Ns * nc * kT;
        dof += static_cast<int64_t>(Tb) * kNDot * n;
        sco += n;
        for (int I = 0; I < Tb; ++I) {
            rows.push_back(int2{bi, I});
            for (int J0 = 0; J0 <= I; J0 += run) items.push_back(int4{bi, I, J0, std::min(I, J0 + run - 1)});
        }
        // per iteration: the lower triangle in its storage; partials written and read once (a column
        // slot per tile (I, J <= I), a row slot per run; none for a block solved whole)
        mat.push_back(0.5 * m * (m + 1.0) * esz);
        double runs = 0.0;
        for (int I = 0; I < Tb; ++I) runs += I / run + 1;
        part.push_back(fused ? 0.0 : 2.0 * 8.0 * nc * kT * (0.5 * Tb * (Tb + 1.0) + runs));
    }
    // biggest blocks' items first (their tile rows are the longest runs of work); the items of the
    // blocks dbslmm_pcg_block solves last (they return at once unless the block has missing calls)
    std::stable_sort(items.begin(), items.end(), [&](const int4& x, const int4& y) {
        return blk[x.x].fused != blk[y.x].fused ? blk[x.x].fused < blk[y.x].fused : blk[x.x].Tb > blk[y.x].Tb;
    });
    std::stable_sort(flist.begin(), flist.end(), [&](const int2& x, const int2& y) { return blk[x.x].Tb > blk[y.x].Tb; });
    // tile rows of those blocks last too: once no such block turns out to have missing calls, the
    // chip-wide launches stop short of them (pcg_iters)
    std::stable_sort(rows.begin(), rows.end(), [&](const int2& x, const int2& y) { return blk[x.x].fused < blk[y.x].fused; });
    p->n_prow_chip = p->n_pitem_chip = 0;
    for (const int2& r : rows) p->n_prow_chip += blk[r.x].fused ? 0 : 1;
    for (const int4& e : items) p->n_pitem_chip += blk[e.x].fused ? 0 : 1;
    p->h_pfused.assign(blk.size(), 0);
    p->h_pnseq.assign(blk.size(), 0);
    for (const int2& f : flist) {
        p->h_pfused[f.x] = 1;
        p->h_pnseq[f.x] += 1;
    }
    p->n_pflist = static_cast<int32_t>(flist.size());
    // a streamed run's host scan: the (block, copy) pairs in the order dbslmm_pcg_block takes them,
    // then those of the chip-wide blocks (flagged by dbslmm_pcg_update as each block converges)
    p->h_pfpairs.clear();
    for (const int2& f : flist)
        for (int c = f.y < 0 ? 0 : f.y; c < (f.y < 0 ? n : f.y + 1); ++c) p->h_pfpairs.push_back(int2{f.x, c});
    for (int b = 0; b < static_cast<int>(blk.size()); ++b)
        if (!blk[b].fused)
            for (int c = 0; c < n; ++c) p->h_pfpairs.push_back(int2{b, c});
    if (!flist.empty()) HIP_TRY(ctx, B.upload(&p->d_pflist, flist, ctx->stream));
    if (!flist.empty() && !p->d_pfnext) HIP_TRY(ctx, B.alloc(&p->d_pfnext, 4));   // (16 B)
    p->n_pblk = static_cast<int32_t>(blk.size());
    p->n_pitem = static_cast<int32_t>(items.size());
    p->n_prow = static_cast<int32_t>(rows.size());
    // past the tile rows, one header entry per block solved whole: a trimmed dbslmm_pcg_init (run_pcg)
    // runs the chip-wide blocks' tile rows and these
    for (int b = 0; b < static_cast<int>(blk.size()); ++b)
        if (blk[b].fused) rows.push_back(int2{b, -1});
    p->n_phead = static_cast<int32_t>(rows.size()) - p->n_prow;
    p->pcg_vstride = vo;
    p->h_pmat = mat;
    p->h_ppart = part;
    HIP_TRY(ctx, B.upload(&p->d_pblk, blk, ctx->stream));
    HIP_TRY(ctx, B.upload(&p->d_pitem, items, ctx->stream));
    HIP_TRY(ctx, B.upload(&p->d_prow, rows, ctx->stream));
    HIP_TRY(ctx, B.alloc(&p->d_pvec, 6 * n * vo));
    HIP_TRY(ctx, B.alloc(&p->d_ppart, po));
    HIP_TRY(ctx, B.alloc(&p->d_pdot, dof));
    HIP_TRY(ctx, B.alloc(&p->d_pqs, static_cast<size_t>(std::max<int32_t>(1, sco)) * pcg::kQS));
    HIP_TRY(ctx, B.alloc(&p->d_pcnv, sco));
    HIP_TRY(ctx, B.alloc(&p->d_pitb, p->n_pblk));
    HIP_TRY(ctx, B.alloc(&p->d_pdone, p->n_pblk));
    HIP_TRY(ctx, B.alloc(&p->d_pact, 1));
    HIP_TRY(ctx, B.alloc(&p->d_pfin, p->n_pblk));
    p->pcg_n = n;
    return DBSLMM_OK;
}

// Iterations the first chunk of a run enqueues: the previous run's count (same data), else the
// Chebyshev bound of the well-conditioned case, kappa = 1 + 12 / (d_min + 1 - tau), + 2, + 4 when
// large SNPs add outlying eigenvalues (tools/cg_gate.py: +4 at 10 large SNPs in a block).
static int pcg_first_chunk(const dbslmm_plan* p, const double* sigmas, int n) {
    if (p->pcg_need >= 0) return std::min(p->pcg_need, p->pcg_maxit);   // (0: every block solved whole)
    double dmin = INFINITY;
    for (int c = 0; c < n; ++c) dmin = std::min(dmin, 1.0 / (sigmas[c] * static_cast<double>(p->n_obs)));
    const double kap = 1.0 + 12.0 / std::max(1e-3, dmin + 1.0 - p->tau);
    const double q = (std::sqrt(kap) - 1.0) / (std::sqrt(kap) + 1.0);
    const int k = static_cast<int>(std::ceil(std::log(2.0 / p->pcg_tol) / -std::log(q))) + 2 + (p->has_large ? 4 : 0);
    return std::clamp(k, 1, p->pcg_maxit);
}

// K iterations (product, rows, update) and the tail (betas, status, convergence read-back).
static int pcg_iters(dbslmm_plan* p, int K) {
    dbslmm_ctx* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    for (int k = 0; k < K; ++k) {
        const int32_t ni = p->pcg_trim ? p->n_pitem_chip : p->n_pitem, nr = p->pcg_trim ? p->n_prow_chip : p->n_prow;
        if (ni == 0 && nr == 0) continue;
        const dim3 g((std::max(1, ni) + pcg::kWaves - 1) / pcg::kWaves);
        if (p->pcg_g16)
            hipLaunchKernelGGL(dbslmm_pcg_symv16, g, dim3(pcg::kThreads), pcg::lds_bytes(p->pcg_n), s, p->pcg_args,
                               p->d_pitem, ni);
        if (!p->pcg_g16 || p->pcg_m_blocks != 0)   // (-1: not known yet)
            hipLaunchKernelGGL(dbslmm_pcg_symv64, g, dim3(pcg::kThreads), pcg::lds_bytes(p->pcg_n), s, p->pcg_args,
                               p->d_pitem, ni);
        hipLaunchKernelGGL(dbslmm_pcg_rows, dim3(std::max(1, nr)), dim3(pcg::kThreads), 0, s, p->pcg_args, p->d_prow);
        hipLaunchKernelGGL(dbslmm_pcg_update, dim3(std::max(1, nr)), dim3(pcg::kThreads), 0, s, p->pcg_args, p->d_prow);
    }
    HIP_TRY(ctx, hipGetLastError());
    p->pcg_it += K;
    if (p->pcg_join) {   // dbslmm_pcg_block's x / cnv / itb before the betas and the read-back
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->join, 0));
        p->pcg_join = false;
    }
    hipLaunchKernelGGL(dbslmm_pcg_final, dim3(p->n_prow), dim3(pcg::kThreads), 0, s, p->pcg_args, p->d_prow);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(p->h_pmon, p->d_pact, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(p->h_pmon + 1, p->d_pitb, p->n_pblk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (p->pcg_ev_end) HIP_TRY(ctx, hipEventRecord(p->pcg_ev_end, s));
    if (p->so_active) HIP_TRY(ctx, hipEventRecord(p->so_ev, s));   // (a streamed run polls it: stream_results)
    return DBSLMM_OK;
}

// Wait for the latest chunk of a pending PCG run; while blocks still iterate (and the cap allows),
// enqueue a further chunk (the run stays pending), else close the run.
static int pcg_check(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    if (p->pcg_pending) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        int32_t need = 0;
        for (int b = 0; b < p->n_pblk; ++b)   // (the chip-wide blocks: the chunk sizes are theirs)
            if (p->h_pfused.empty() || !p->h_pfused[b]) need = std::max(need, p->h_pmon[1 + b]);
        if (p->h_pmon[0] <= 0 || p->pcg_it >= p->pcg_maxit) {
            p->pcg_pending = false;
            p->pcg_need = p->h_pmon[0] <= 0 ? need : p->pcg_maxit;
            p->pcg_iters_max = 0;
            for (int b = 0; b < p->n_pblk; ++b) p->pcg_iters_max = std::max(p->pcg_iters_max, p->h_pmon[1 + b]);
            if (p->pcg_m_blocks < 0) {   // missing-call flags are data: read once, after the first run
                std::vector<int32_t> fl(std::max(1, p->n_nonempty));
                HIP_TRY(ctx, hipMemcpy(fl.data(), p->d_flags, fl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
                p->pcg_m_blocks = 0;
                p->h_pmiss.assign(p->n_pblk, 0);
                for (int b = 0; b < p->n_nonempty; ++b) {
                    p->pcg_m_blocks += fl[b] & 1;
                    if (b < p->n_pblk) p->h_pmiss[b] = fl[b] & 1;
                }
            }
            p->pcg_trim = true;   // (the fused flags are those of the current layout)
            for (int b = 0; b < p->n_pblk && b < static_cast<int>(p->h_pfused.size()); ++b)
                if (p->h_pfused[b] && p->h_pmiss[b]) p->pcg_trim = false;
            // bytes the run streamed: every block its own iteration count
            p->pcg_cbytes = p->pcg_pbytes = p->pcg_fbytes = 0.0;
            for (int b = 0; b < p->n_pblk && b < static_cast<int>(p->h_pmat.size()); ++b) {
                const double it = p->h_pmon[1 + b];
                const bool miss = !p->h_pmiss.empty() && p->h_pmiss[b];
                const double mb = p->h_pmat[b] * (miss && p->pcg_g16 ? 4.0 : 1.0);
                if (!p->h_pfused.empty() && p->h_pfused[b] && !miss) {
                    p->pcg_fbytes += it * mb * p->h_pnseq[b];
                } else {
                    p->pcg_cbytes += it * mb;
                    p->pcg_pbytes += it * p->h_ppart[b];
                }
            }
            return DBSLMM_OK;
        }
        const int K = std::min(std::max(4, p->pcg_it / 4), p->pcg_maxit - p->pcg_it);
        if (const int rc = pcg_iters(p, K)) return rc;
    }
    return DBSLMM_OK;
}

// Wait for a PCG run, continuation chunks included.
static int pcg_finish(dbslmm_plan* p) {
    while (p->pcg_pending)
        if (const int rc = pcg_check(p)) return rc;
    return DBSLMM_OK;
}

// The mirror and flags of a streamed run of n copies, and its run number.
static int so_prepare(dbslmm_plan* p, int n) {
    dbslmm_ctx* ctx = p->ctx;
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    const size_t bytes = static_cast<size_t>(n) * (p->n_s + p->n_l) * sizeof(double) +
                         static_cast<size_t>(n) * p->nbk * sizeof(int32_t);
    if (bytes > p->h_mir_bytes) {
        if (p->h_mir) HIP_TRY(ctx, hipHostFree(p->h_mir));
        p->h_mir = nullptr;
        p->h_mir_bytes = 0;
        HIP_TRY(ctx, hipHostMalloc(&p->h_mir, bytes, fl));
        p->h_mir_bytes = bytes;
    }
    const size_t nf = static_cast<size_t>(std::max(1, p->n_nonempty)) * pcg::kMaxNC;
    if (!p->h_mflag) {
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&p->h_mflag), nf * sizeof(int32_t), fl));
        memset(p->h_mflag, 0, nf * sizeof(int32_t));
        p->so_done.assign(nf, 0);
    }
    if (!p->so_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&p->so_ev, hipEventDisableTiming));
    if (p->so_run == INT32_MAX) {   // (no run in flight here: flags and marks restart with the numbers)
        memset(p->h_mflag, 0, nf * sizeof(int32_t));
        p->so_done.assign(nf, 0);
        p->so_run = 0;
    }
    p->so_run++;
    p->so_n = n;
    return DBSLMM_OK;
}

// Open a timed run (dbslmm_plan_enable_timing): *ev = its kEvCount events, created on first use, and
// its route noted for collect_timing.  An untimed run leaves *ev null.
static int open_timed_run(dbslmm_plan* p, bool pcg, hipEvent_t** ev) {
    *ev = nullptr;
    if (!p->timing) return DBSLMM_OK;
    const size_t need = kEvCount * static_cast<size_t>(p->runs_pending + 1);
    while (p->ev.size() < need) {
        hipEvent_t e;
        HIP_TRY(p->ctx, hipEventCreate(&e));
        p->ev.push_back(e);
    }
    *ev = &p->ev[kEvCount * p->runs_pending];
    p->runs_pending++;
    p->run_route.resize(p->runs_pending);
    p->run_route.back() = pcg ? 1 : 0;
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

// One run on the PCG route: statistics + Gram (the integer Gram as uint16 where it fits, Sigma in fp64
// for the other blocks), then the iterations of every block and copy together.
static int run_pcg(dbslmm_plan* p, const double* sigmas, int n) {
    dbslmm_ctx* ctx = p->ctx;
#ifdef DBSLMM_DIAG
    auto diag_error = [](const char* when) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) fprintf(stderr, "run_pcg: %s: %s\n", when, hipGetErrorString(e));
    };
#else
    auto diag_error = [](const char*) {};
#endif
    diag_error("stale error on entry");
    if (const int rc = ensure_copies(p, n, 1)) return rc;
    diag_error("error after ensure_copies");
    if (const int rc = pcg_layout(p, n)) return rc;
    diag_error("error after pcg_layout");
    // results streamed to the host while the run iterates: dbslmm_plan_run_multi on one device
    p->so_active = p->so_want && p->stream_out;
    if (p->so_active)
        if (const int rc = so_prepare(p, n)) return rc;
    hipStream_t s = ctx->stream;
    hipEvent_t* ev = nullptr;
    if (const int rc = open_timed_run(p, true, &ev)) return rc;
    p->pcg_ev_end = ev ? ev[kEvEnd] : nullptr;
    p->trsv_failed = false;
    p->stopped = false;
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvStart], s));
    // One launch in front of the Gram: the statistics, and with them the run's resets (status,
    // the count of iterating blocks, dbslmm_pcg_block's sequence counter) and the copies' shifts.
    // The timed instants of this route: kEvStart, kEvStatsEnd, kEvGramEnd, kEvPcgBlockBegin / End and
    // kEvEnd (collect_timing).
    static_assert(pcg::kMaxNC <= kFrontCopies, "PcgFront carries every copy's shift");
    PcgFront fr{};
    for (int c = 0; c < n; ++c) fr.shift[c] = 1.0 / (sigmas[c] * static_cast<double>(p->n_obs));
    fr.dshift = p->d_dshift;
    fr.n = n;
    fr.n_status = static_cast<int32_t>(n * p->nbk);
    fr.status = p->d_status;
    fr.active = p->d_pact;
    fr.next = p->n_pflist > 0 ? p->d_pfnext : nullptr;
    hipLaunchKernelGGL(dbslmm_pcg_front, dim3(std::max(1, (p->n_slots + 255) / 256)), dim3(256), 0, s, p->img.rows(),
                       p->n_ref, p->d_slot_pos, p->d_slot_block, p->n_slots, p->d_S, p->d_mu, p->d_rsd, p->d_flags, fr);
    HIP_TRY(ctx, hipGetLastError());
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvStatsEnd], s));
    uint16_t* g16 = p->pcg_g16 ? p->d_G16 : nullptr;
    const double nrd = static_cast<double>(p->n_ref);
    // one copy of Sigma, and the integer Gram as uint16 where it fits
    const GramOut go{1, INT32_MAX, -1, g16, p->d_off16, p->d_ld16};
    // (Measured and dropped: the Gram of the blocks dbslmm_pcg_block solves on the second stream
    // beside the chip-wide iterations -- its 256-tile workgroups hold 128 KiB of LDS, so the product
    // items cannot run beside them: config 4 8.8 -> 9.6 ms.)
    HIP_TRY(ctx, launch_gram(p, s, kGramHuge, p->d_htiles, p->n_htiles, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramI8, p->d_tiles, p->n_tiles, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramBig, p->d_btiles, p->n_btiles, go));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvGramEnd], s));
    PcgArgs a{};
    a.blk = p->d_pblk;
    a.G16 = g16;
    a.M = p->d_M;
    a.flags = p->d_flags;
    a.S = p->d_S;
    a.rsd = p->d_rsd;
    a.z = p->d_z;
    a.slot_out = p->d_slot_out;
    a.blk_id = p->d_blk_id;
    a.dshift = p->d_dshift;
    const int64_t vs = static_cast<int64_t>(n) * p->pcg_vstride;
    a.X = p->d_pvec;
    a.R = a.X + vs;
    a.P = a.R + vs;
    a.Sv = a.P + vs;
    a.W = a.Sv + vs;
    a.U = a.W + vs;
    a.part = p->d_ppart;
    a.dot = p->d_pdot;
    a.qs = p->d_pqs;
    a.cnv = p->d_pcnv;
    a.itb = p->d_pitb;
    a.done = p->d_pdone;
    a.active = p->d_pact;
    a.fin = p->d_pfin;
    a.beta_s = p->d_beta_s;
    a.beta_l = p->d_beta_l;
    a.status = p->d_status;
    if (p->so_active) {   // the mirror through its device addresses: [beta_s | beta_l | status]
        void *dm = nullptr, *df = nullptr;
        HIP_TRY(ctx, hipHostGetDevicePointer(&dm, p->h_mir, 0));
        HIP_TRY(ctx, hipHostGetDevicePointer(&df, p->h_mflag, 0));
        a.mir_s = static_cast<double*>(dm);
        a.mir_l = a.mir_s + static_cast<int64_t>(n) * p->n_s;
        a.mir_st = reinterpret_cast<int32_t*>(a.mir_l + static_cast<int64_t>(n) * p->n_l);
        a.mir_flag = static_cast<int32_t*>(df);
        a.run_no = p->so_run;
    }
    a.vstride = p->pcg_vstride;
    a.ns = p->n_s;
    a.nl = p->n_l;
    a.nbk = p->nbk;
    a.tau = p->tau;
    a.rn = 1.0 / nrd;
    a.c0 = p->tau * (nrd - 1.0) / nrd + 1.0 - p->tau;
    a.tol = p->pcg_tol;
    a.inv_sqrt_n = 1.0 / std::sqrt(static_cast<double>(p->n_obs));
    a.ncopy = n;
    a.run = p->pcg_run;
                         // the multi-shift seed: the smallest shift (largest sigma)
    for (int c = 1; c < n; ++c)
        if (sigmas[c] > sigmas[a.seed]) a.seed = c;
    p->pcg_args = a;
    // Once a run has read the missing-call flags and none of the blocks dbslmm_pcg_block takes has
    // any (pcg_trim), those blocks keep their whole state in LDS: their tile rows' vectors are
    // neither written nor read, and one header workgroup each does what their tile row 0 did.
    if (p->pcg_trim)
        hipLaunchKernelGGL(dbslmm_pcg_init, dim3(std::max(1, p->n_prow_chip + p->n_phead)), dim3(pcg::kThreads), 0, s, a,
                           p->d_prow, p->n_prow_chip, p->n_prow - p->n_prow_chip);
    else
        hipLaunchKernelGGL(dbslmm_pcg_init, dim3(p->n_prow), dim3(pcg::kThreads), 0, s, a, p->d_prow, p->n_prow, 0);
    HIP_TRY(ctx, hipGetLastError());
    p->pcg_join = false;
    if (p->n_pflist > 0) {   // the small blocks' whole solves beside the chip-wide iterations
        HIP_TRY(ctx, hipEventRecord(ctx->fork, s));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->fork, 0));
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvPcgBlockBegin], ctx->stream2));
        // one workgroup per CU (its LDS holds x and p: one fits): the chip-wide kernels of the
        // other blocks keep the rest of every CU
        // (two per CU at one copy, where their LDS fits: configs 3 / 5 6.02 -> 6.27 / 2.35 -> 2.51 ms)
        int grid = std::max(1, std::min(p->n_pflist, ctx->n_cu));
        if (p->pcg_block_wgs > 0) grid = std::min(grid, p->pcg_block_wgs);
        hipLaunchKernelGGL(dbslmm_pcg_block, dim3(grid), dim3(pcg::kThreads), pcg::block_lds_bytes(n), ctx->stream2, a,
                           p->d_pflist, p->n_pflist, p->d_pfnext, p->pcg_maxit);
        HIP_TRY(ctx, hipGetLastError());
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvPcgBlockEnd], ctx->stream2));
        HIP_TRY(ctx, hipEventRecord(ctx->join, ctx->stream2));
        p->pcg_join = true;
    } else if (const int rc = record_instants(ctx, ev, {kEvPcgBlockBegin, kEvPcgBlockEnd}, s)) {
        return rc;
    }
    p->pcg_it = 0;
    p->pcg_pending = true;
    if (const int rc = pcg_iters(p, pcg_first_chunk(p, sigmas, n))) return rc;
    p->ran = true;
    p->n_runs++;
    p->sigma_run = sigmas[n - 1];
    p->var_copy = n - 1;
    p->score_copies = n;
    p->score_stale = false;
    p->pcg_ran = true;
    p->pcg_pending_var = true;
    p->cheb_base = -1;
    p->cg_ran = false;
    p->cheb_pending_var = false;
    p->wl[14] = 0;
    p->wl[15] = -1;
    p->wl[16] = 0;
    return DBSLMM_OK;
}

// One run: statistics + Gram, then n factorisations + solves of it, copy c with
// sigma_s = sigmas[c] (n > 1: h2f tuning; copies 1.. are device copies of the Gram, all factored
// by one merged tiled sequence).
static int run_impl(dbslmm_plan* p, const double* sigmas, int n) {
    dbslmm_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = pcg_finish(p)) return rc;   // a PCG run still pending (plan_run without sync)
    if (pcg_route(p, sigmas, n)) return run_pcg(p, sigmas, n);
    // A run kept off the PCG route by its number of copies alone keeps that route's accuracy: its
    // iterated h2f copies stop at pcg_tol (relative error per block and copy, as run_pcg), so a
    // fifth h2f factor does not move the results of the others from 1e-12 to cheb_tol.
    p->h2f_tol = n > pcg::kMaxNC && pcg_eligible(p, sigmas, n) ? std::min(p->cheb_tol, p->pcg_tol) : p->cheb_tol;
    if (const int rc = ensure_copies(p, n, n)) return rc;
    if (n > 1) {
        if (p->multi_n != n) {
            std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous upload below
            std::vector<int32_t> tlist;
            p->tl_multi.clear();
            build_tiled(p->h_m, p->h_tb, n, p->n_nonempty, p->tl_multi, tlist);
            (void)p->bufs.release(p->d_tlist_multi);
            HIP_TRY(ctx, p->bufs.upload(&p->d_tlist_multi, tlist, ctx->stream));
            if (p->graph_multi) (void)hipGraphExecDestroy(p->graph_multi);
            p->graph_multi = nullptr;
            p->multi_n = n;
        }
    }
    // h2f: the tiled blocks are factored once (copy cp.base) and the other copies iterate on it
    p->trsv_failed = false;
    ChebPlan cp;
    const bool cheb = p->n_nonempty > 0 && cheb_plan(p, sigmas, n, cp);
    const int32_t tcopy = cheb ? cp.base : -1;   // Gram epilogues: iterated blocks write this copy only
    // ... the blocks with m >= tmin_copy: the tiled ones and the single-workgroup ones (ld > 64),
    // whose other h2f copies iterate on the base factor too (dbslmm_chol_cheb)
    const bool large_cheb = cheb && p->large_cheb_ok;
    const int32_t tmin_copy = large_cheb ? chol::kSmallLd : p->tiled_min;
    hipStream_t s = ctx->stream;
    hipEvent_t* ev = nullptr;
    if (const int rc = open_timed_run(p, false, &ev)) return rc;
    p->pcg_ran = false;
    p->pcg_pending_var = false;
    const size_t nbk = static_cast<size_t>(p->nbk);
    // Substitution tile flags are epochs (trsv.hip): a run takes at most kEpochsPerRun of them
    // (backward solves and Chebyshev passes of every group and copy).  When the counter could wrap
    // during this run, the flags restart from a clean slate HERE, on the main stream: every stream
    // of the run forks from it after this point and every stream of the previous run has joined
    // it, so no substitution launch of either group can still be running (a reset inside a group
    // would race the other group's launch on its own stream).
    if (p->n_tflags > 0 && p->trsv_epoch > INT32_MAX - kEpochsPerRun) {
        HIP_TRY(ctx, hipMemsetAsync(p->d_tflags, 0, p->n_tflags * sizeof(int32_t), s));
        HIP_TRY(ctx, hipMemsetAsync(p->d_tepi, 0, p->n_tflags * sizeof(int32_t), s));
        p->trsv_epoch = 0;
    }
    p->stopped = false;
    HIP_TRY(ctx, hipMemsetAsync(p->d_flags, 0, nbk * sizeof(int32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(p->d_status, 0, n * nbk * sizeof(int32_t), s));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvStart], s));
    // the statistics of every slot in one launch (a gather from the image's row table: microseconds,
    // so a lead group's Gram right behind it starts at once)
    if (p->n_slots > 0) {
        hipLaunchKernelGGL(dbslmm_slot_stats, dim3((p->n_slots + 255) / 256), dim3(256), 0, s, p->img.rows(),
                           p->n_ref, p->d_slot_pos, p->d_slot_block, p->n_slots, p->d_S, p->d_mu, p->d_rsd,
                           p->d_flags);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvLeadGramBegin], s));
    const std::vector<TLaunch>& tl = n > 1 && !cheb ? p->tl_multi : p->tl;
    // lead group (plan_layout.hpp): the single-copy sequence is split in two -- the lead blocks'
    // sequence starts on stream2 right after their Gram tiles, the rest on stream4 after the
    // whole Gram; stream2 waits for the rest before the substitutions
    const bool lead = !p->tl_rest.empty() && (n == 1 || cheb);
    const int fcopy = cheb ? cp.base : 0;   // the copy the single-copy sequence factors
    const double isn = 1.0 / std::sqrt(static_cast<double>(p->n_obs));
    if (p->n_nonempty > 0) {
        for (int c = 0; c < n; ++c) {
            const double dshift = 1.0 / (sigmas[c] * static_cast<double>(p->n_obs));
            hipLaunchKernelGGL(dbslmm_set_scalar, dim3(1), dim3(1), 0, s, p->d_dshift + c, dshift);
        }
        if (cheb) {
            const int rc = cheb_prepare(p, cp, s);
            if (rc != DBSLMM_OK) return rc;
        }
    }
    // (the factorisation overwrites its matrix: the Gram epilogues write all n copies)
    const GramOut go{n, tmin_copy, tcopy, nullptr, nullptr, nullptr};
    HIP_TRY(ctx, launch_gram(p, s, kGramHuge, p->d_htiles, p->n_htiles_lead, go));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvLeadGramEnd], s));
    // the lead sequence (stream2, high priority: the critical path) waits for this point of the
    // main stream; its graph is launched after every main-stream kernel is enqueued (a graph
    // launch of a few hundred nodes keeps the host busy for milliseconds)
    if (lead) {
        HIP_TRY(ctx, hipEventRecord(ctx->fork, s));
        debug_spin(p, s, 1);
    }
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvStatsEnd], s));   // (the statistics span less the lead Gram's)
    // the other tiled blocks' Gram tiles next: with early_fork their sequence (and the single
    // sequence without a lead group) forks here, before the non-tiled blocks' Gram
    HIP_TRY(ctx, launch_gram(p, s, kGramHuge, p->d_htiles + p->n_htiles_lead, p->n_htiles_tiled - p->n_htiles_lead, go));
    const bool early = p->early_fork && p->n_nonempty > 0;
    if (early) {
        HIP_TRY(ctx, hipEventRecord(ctx->fork2, s));
        HIP_TRY(ctx, hipStreamWaitEvent(lead ? ctx->stream4 : ctx->stream2, ctx->fork2, 0));
    }
    HIP_TRY(ctx, launch_gram(p, s, kGramI8, p->d_tiles, p->n_tiles, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramHuge, p->d_htiles + p->n_htiles_tiled, p->n_htiles - p->n_htiles_tiled, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramBig, p->d_btiles, p->n_btiles, go));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvGramEnd], s));
    if (p->debug_stop == 1) {   // tests: the block matrices hold Sigma (dbslmm_plan_block_matrix)
        if (const int rc = record_instants(ctx, ev, kEvAfterGram, s)) return rc;
        p->ran = true;
        p->stopped = true;      // download / variance refuse: the betas of this run were never computed
        return DBSLMM_OK;
    }
    if (p->n_nonempty > 0) {
        // fork: the tiled sequence (or, with a lead group, the rest sequence on stream4) runs
        // beside the single-workgroup and single-wave kernels of the main stream
        if (!early) {
            HIP_TRY(ctx, hipEventRecord(ctx->fork2, s));
            HIP_TRY(ctx, hipStreamWaitEvent(lead ? ctx->stream4 : ctx->stream2, ctx->fork2, 0));
        }
        if (p->n_large > 0 && !large_cheb) {   // every copy in one launch
            hipLaunchKernelGGL(dbslmm_chol_large, dim3(p->n_large * n), dim3(chol::kLargeThreads),
                               kCholLargeLds, s, p->d_M, p->d_order, p->n_large,
                               p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff, p->d_blk_id, p->d_z,
                               p->d_slot_out, p->d_rsd, p->d_dshift, isn, p->d_y, p->d_beta_s, p->d_beta_l,
                               p->d_status, n, p->M_elems, static_cast<int64_t>(p->n_slots), p->n_s, p->n_l,
                               p->nbk);
            HIP_TRY(ctx, hipGetLastError());
        } else if (p->n_large > 0) {
            // h2f by Chebyshev: the base copy is factored, the others iterate on its factor
            const int64_t bc = cp.base;
            hipLaunchKernelGGL(dbslmm_chol_large, dim3(p->n_large), dim3(chol::kLargeThreads), kCholLargeLds, s,
                               p->d_M + bc * p->M_elems, p->d_order, p->n_large, p->d_row0, p->d_m, p->d_ms,
                               p->d_ld, p->d_matoff, p->d_blk_id, p->d_z, p->d_slot_out, p->d_rsd,
                               p->d_dshift + bc, isn, p->d_y + bc * p->n_slots, p->d_beta_s + bc * p->n_s,
                               p->d_beta_l + bc * p->n_l, p->d_status + bc * p->nbk, 1, p->M_elems,
                               static_cast<int64_t>(p->n_slots), p->n_s, p->n_l, p->nbk);
            HIP_TRY(ctx, hipGetLastError());
            for (size_t g = 0; g < cp.iters.size(); ++g) {
                const size_t g0 = g * chol::kChebR;
                const int nr = static_cast<int>(std::min<size_t>(chol::kChebR, cp.others.size() - g0));
                chol::CgStop cgs{};   // h2f by CG (the default): stopping bounds per copy
                cgs.on = p->h2f_cg ? 1 : 0;
                for (int j = 0; j < nr; ++j) cgs.fs[j] = cp.db + cp.coef[cp.coef_off[g] + 3 * j + 2] + 1.0 - p->tau;
                cgs.fl = 1.0 - p->tau;
                cgs.tol = p->h2f_tol;
                cgs.capped = cp.capped[g];
                hipLaunchKernelGGL(dbslmm_chol_cheb, dim3(p->n_large), dim3(chol::kChebThreads), kCholChebLds, s,
                                   p->d_M + bc * p->M_elems, p->d_order, p->n_large, p->d_row0, p->d_m, p->d_ms,
                                   p->d_ld, p->d_matoff, p->d_blk_id, p->d_slot_out, p->d_y + bc * p->n_slots,
                                   p->d_coef + cp.coef_off[g], nr, cp.iters[g], isn, p->d_beta_s, p->d_beta_l,
                                   p->n_s, p->n_l, p->d_status + bc * p->nbk, p->d_status,
                                   static_cast<int64_t>(p->nbk), cp.others[g0], nr > 1 ? cp.others[g0 + 1] : 0, cgs);
                HIP_TRY(ctx, hipGetLastError());
            }
        }
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvLargeEnd], s));
        // single-wave blocks: concurrently on stream2 when there is no tiled sequence, else
        // behind the single-workgroup kernel (each stream keeps its own hardware queue)
        hipStream_t ss = tl.empty() ? ctx->stream2 : s;
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvSmallBegin], ss));
        for (int c = 0; c < n && p->n_small > 0; ++c) {
            const unsigned g = static_cast<unsigned>((p->n_small + chol::kSmallWaves - 1) / chol::kSmallWaves);
            hipLaunchKernelGGL(dbslmm_chol_small, dim3(g), dim3(chol::kSmallWaves * chol::kWave), 0,
                               ss, p->d_M + c * p->M_elems, p->d_order + p->n_large, p->n_small, p->d_row0,
                               p->d_m, p->d_ms, p->d_ld, p->d_matoff, p->d_blk_id, p->d_z,
                               p->d_slot_out, p->d_rsd, p->d_dshift + c, isn, p->d_beta_s + c * p->n_s,
                               p->d_beta_l + c * p->n_l, p->d_status + c * p->nbk);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvSmallEnd], ss));
        if (ss != s) HIP_TRY(ctx, hipEventRecord(ctx->join, ss));
        if (lead) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->fork, 0));
            if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvTiledBegin], ctx->stream2));
            debug_spin(p, ctx->stream2, -1);
            debug_spin(p, ctx->stream4, 1);
            int rc = run_tiled_copy(p, isn, fcopy);
            if (rc == DBSLMM_OK) rc = run_rest_copy(p, isn, fcopy);
            if (rc != DBSLMM_OK) return rc;
        } else if (ev) {
            HIP_TRY(ctx, hipEventRecord(ev[kEvTiledBegin], ctx->stream2));
        }
        if (!tl.empty()) {
            // the tiled sequence (~2.5 launches per 128 columns) is replayed from a graph
            // captured on first use (sigma is read from device scalars, so it stays valid)
            if (n == 1 || cheb) {
                // h2f: factor only the base copy, iterate the others on its factor
                int rc = lead ? DBSLMM_OK : run_tiled_copy(p, isn, fcopy);
                if (lead && p->sub_split) {
                    // per-group substitutions: the rest group's on its own stream right after its
                    // factorisation, the lead group's on stream2 after the lead factorisation
                    const TGroup gr = tgroup_rest(p), gl = tgroup_lead(p);
                    if (rc == DBSLMM_OK && gr.n_items > 0) rc = run_pbwd(p, isn, fcopy, gr);
                    if (ev && cheb) HIP_TRY(ctx, hipEventRecord(ev[kEvRestEnd], gr.st));
                    if (rc == DBSLMM_OK && cheb && gr.n_items > 0)
                        rc = p->sub_block ? run_tcheb(p, isn, cp, gr.st) : run_cheb(p, isn, cp, gr);
                    if (rc == DBSLMM_OK) rc = run_pbwd(p, isn, fcopy, gl);
                    if (rc != DBSLMM_OK) return rc;
                    if (cheb) {
                        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvTiledEnd], ctx->stream2));
                        rc = run_cheb(p, isn, cp, gl);
                        if (rc != DBSLMM_OK) return rc;
                    }
                    HIP_TRY(ctx, hipEventRecord(ctx->join4, ctx->stream4));
                    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->join4, 0));
                } else {
                    if (lead) {   // the rest sequence is done before the substitutions (one launch
                                  // sequence over all tiled blocks)
                        HIP_TRY(ctx, hipEventRecord(ctx->join4, ctx->stream4));
                        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->join4, 0));
                    }
                    if (rc == DBSLMM_OK) rc = run_pbwd(p, isn, fcopy, tgroup_all(p));
                    if (rc != DBSLMM_OK) return rc;
                    if (cheb) {
                        if (const int rce = record_instants(ctx, ev, {kEvTiledEnd, kEvRestEnd}, ctx->stream2)) return rce;
                        rc = run_cheb(p, isn, cp, tgroup_all(p));
                        if (rc != DBSLMM_OK) return rc;
                    }
                }
            } else {
                // merged copies: one sequence factors every copy, then one backward launch each
                int rc = launch_graph(p, isn, tl, p->d_tlist_multi, 0, p->graph_multi, seq_main(p));
                for (int c = 0; c < n && rc == DBSLMM_OK; ++c) rc = run_pbwd(p, isn, c, tgroup_all(p));
                if (rc != DBSLMM_OK) return rc;
            }
        }
        if (!cheb)
            if (const int rc = record_instants(ctx, ev, {kEvTiledEnd, kEvRestEnd}, ctx->stream2)) return rc;
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvEnd], ctx->stream2));
        HIP_TRY(ctx, hipEventRecord(ctx->join3, ctx->stream2));
        if (ss != s) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->join, 0));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->join3, 0));
    }
    else if (const int rc = record_instants(ctx, ev, kEvAfterGram, s)) {   // no blocks
        return rc;
    }
    p->ran = true;
    p->n_runs++;
    p->sigma_run = sigmas[n - 1];
    p->var_copy = n - 1;
    if (p->force_factor) {
        p->score_stale = true;   // the variance's re-solve: copy 0 of the device results is overwritten
    } else {
        p->score_copies = n;
        p->score_stale = false;
    }
    {
        p->cheb_base = cheb ? cp.base : -1;
        int iters = 0;
        for (int k : cp.iters) iters += k;
        p->wl[14] = cheb ? iters : 0;
        p->wl[15] = p->cheb_base;
        p->cg_ran = cheb && p->h2f_cg && !p->cheb_fused;
        p->wl[16] = cheb ? 2.0 * iters * p->wl[13] : 0.0;   // (CG: counted from d_cgit on query)
        p->cheb_pending_var = cheb && cp.base != n - 1;   // no factor of the last copy's tiled blocks
    }
    return DBSLMM_OK;
}

// After the main stream has drained: the error word of the persistent substitutions (trsv.hip:
// a bounded hand-off wait that gave up means the tiled blocks' betas of that run are invalid).
// Read and cleared after every run that launched one; the failure stays reported until the next run.
static int check_trsv(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    if (p->trsv_pending) {
        std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous copy / memset below
        int32_t werr = 0;
        HIP_TRY(ctx, hipMemcpy(&werr, p->d_tflags + p->n_tflags + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (werr) {
            HIP_TRY(ctx, hipMemsetAsync(p->d_tflags + p->n_tflags + 1, 0, sizeof(int32_t), ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        p->trsv_pending = false;
        p->trsv_failed = p->trsv_failed || werr != 0;
    }
    if (p->trsv_failed) {
        ctx->err = "substitution hand-off wait gave up (trsv): the tiled blocks' betas of this run are invalid";
        return DBSLMM_E_HIP;
    }
    return DBSLMM_OK;
}

// Results of factorisation copies c0 .. c0 + n - 1 (each copy's betas / status contiguous on the
// device and in the caller's arrays): one asynchronous copy per array into the plan's pinned
// buffer, then a threaded copy out (pageable hipMemcpy of 8 MB arrays cost ~0.3 ms each).
static int download_copies(dbslmm_plan* p, int c0, int n, double* beta_s, double* beta_l, int32_t* block_status) {
    dbslmm_ctx* ctx = p->ctx;
    if (!p->ran) { ctx->err = "plan_download before plan_run"; return DBSLMM_E_STATE; }
    if (p->stopped) { ctx->err = "plan_download after a run stopped at the Gram (debug_stop)"; return DBSLMM_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (const int rc = check_trsv(p)) return rc;
    const size_t nbs = beta_s ? static_cast<size_t>(n) * p->n_s : 0;
    const size_t nbl = beta_l ? static_cast<size_t>(n) * p->n_l : 0;
    const size_t nst = block_status && p->num_block ? static_cast<size_t>(n) * p->nbk : 0;
    const size_t bytes = (nbs + nbl) * sizeof(double) + nst * sizeof(int32_t);
    if (bytes == 0) return DBSLMM_OK;
    if (bytes > p->h_pin_bytes) {
        if (p->h_pin) HIP_TRY(ctx, hipHostFree(p->h_pin));
        p->h_pin = nullptr;
        p->h_pin_bytes = 0;
        HIP_TRY(ctx, hipHostMalloc(&p->h_pin, bytes, hipHostMallocDefault));
        p->h_pin_bytes = bytes;
    }
    double* ps = static_cast<double*>(p->h_pin);
    double* pl = ps + nbs;
    int32_t* pt = reinterpret_cast<int32_t*>(pl + nbl);
    // per copy: its DMA into the pinned buffer, an event, then (below) its host copy-out while the
    // next copy's DMA runs
    while (static_cast<int>(p->dl_ev.size()) < n) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        p->dl_ev.push_back(e);
    }
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

// The results of a streamed PCG run (run_pcg with so_active) into the caller's arrays, from the
// plan's host-visible mirror and without a download: while the run's latest chunk is on the GPU
// the calling thread polls its end event and copies out every (route block, copy) flagged since
// the last look (by dbslmm_pcg_block at the end of a sequence, by dbslmm_pcg_update when a
// chip-wide block has converged) -- that block's range of beta_s, its few beta_l entries and its
// status -- so nearly all the bytes have left before the last kernel ends.  The flags only say
// what may be copied early; once the run is over, whatever was not copied (monomorphic blocks and
// blocks at the iteration cap, which dbslmm_pcg_final writes, and any block whose flag was not
// seen in time) is copied regardless of them, so no result can be missed and nothing waits on a
// flag.  Timing events are collected after the copy-out.
static int stream_results(dbslmm_plan* p, double* beta_s, double* beta_l, int32_t* block_status) {
    dbslmm_ctx* ctx = p->ctx;
    const int n = p->so_n;
    const int32_t run = p->so_run;
    const double* ms = static_cast<const double*>(p->h_mir);
    const double* ml = ms + static_cast<int64_t>(n) * p->n_s;
    const int32_t* mst = reinterpret_cast<const int32_t*>(ml + static_cast<int64_t>(n) * p->n_l);
    if (!p->num_block) block_status = nullptr;
    auto copy_out = [&](int b, int c) {
        const OutRange& r = p->h_orange[b];
        if (beta_s && r.s1 > r.s0)
            memcpy(beta_s + c * p->n_s + r.s0, ms + c * p->n_s + r.s0, (r.s1 - r.s0) * sizeof(double));
        if (beta_l && r.l1 > r.l0)
            memcpy(beta_l + c * p->n_l + r.l0, ml + c * p->n_l + r.l0, (r.l1 - r.l0) * sizeof(double));
        if (block_status) block_status[static_cast<int64_t>(c) * p->num_block + r.blk] = mst[c * p->nbk + r.blk];
        p->so_done[static_cast<size_t>(b) * n + c] = run;
    };
    const std::vector<int2>& pairs = p->h_pfpairs;
    size_t head = 0;                         // every pair before it is copied
    bool polled = false;
    while (p->pcg_pending) {
        for (;;) {
            const hipError_t q = hipEventQuery(p->so_ev);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIP_TRY(ctx, q);
            polled = true;
            for (size_t e = head; e < pairs.size(); ++e) {
                const size_t f = static_cast<size_t>(pairs[e].x) * n + pairs[e].y;
                if (p->so_done[f] != run && __atomic_load_n(p->h_mflag + f, __ATOMIC_ACQUIRE) == run)
                    copy_out(pairs[e].x, pairs[e].y);
            }
            while (head < pairs.size() && p->so_done[static_cast<size_t>(pairs[head].x) * n + pairs[head].y] == run)
                ++head;
        }
        if (const int rc = pcg_check(p)) return rc;   // (may enqueue another chunk: poll again)
    }
    if (polled) (void)hipGetLastError();     // (hipErrorNotReady of the polls is no error)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (const int rc = check_trsv(p)) return rc;
    // the rest: runs of neighbouring blocks not copied yet are one range of beta_s / beta_l each
    std::vector<CopySeg> rest;
    for (int c = 0; c < n; ++c)
        for (int b = 0; b < p->n_pblk;) {
            if (p->so_done[static_cast<size_t>(b) * n + c] == run) { ++b; continue; }
            int e = b;
            while (e + 1 < p->n_pblk && p->so_done[static_cast<size_t>(e + 1) * n + c] != run) ++e;
            const OutRange &r0 = p->h_orange[b], &r1 = p->h_orange[e];
            if (beta_s && r1.s1 > r0.s0)
                rest.push_back({beta_s + c * p->n_s + r0.s0, ms + c * p->n_s + r0.s0, (r1.s1 - r0.s0) * sizeof(double)});
            if (beta_l && r1.l1 > r0.l0)
                rest.push_back({beta_l + c * p->n_l + r0.l0, ml + c * p->n_l + r0.l0, (r1.l1 - r0.l0) * sizeof(double)});
            for (int k = b; k <= e; ++k) {
                const int32_t id = p->h_orange[k].blk;
                if (block_status) block_status[static_cast<int64_t>(c) * p->num_block + id] = mst[c * p->nbk + id];
                p->so_done[static_cast<size_t>(k) * n + c] = run;
            }
            b = e + 1;
        }
    par_memcpy_list(rest);
    for (int c = 0; c < n && block_status; ++c)
        for (int32_t b : p->h_empty) block_status[static_cast<int64_t>(c) * p->num_block + b] = DBSLMM_BLOCK_EMPTY;
    if (p->timing) return collect_timing(p);
    p->runs_pending = 0;
    p->run_route.clear();
    return DBSLMM_OK;
}

static int download_copy(dbslmm_plan* p, int c, double* beta_s, double* beta_l, int32_t* block_status) {
    return download_copies(p, c, 1, beta_s, beta_l, block_status);
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
    p->so_want = true;                       // (the PCG route may stream its results: stream_out)
    int rc = run_impl(p, sigmas, n_sigma);
    p->so_want = false;
    if (!rc && p->pcg_ran && p->so_active) return stream_results(p, beta_s, beta_l, block_status);
    if (!rc) rc = dbslmm_plan_sync(p);
    if (!rc) rc = download_copies(p, 0, n_sigma, beta_s, beta_l, block_status);
    return rc;
}

int dbslmm_plan_sync(dbslmm_plan* p) {
    if (!p) return DBSLMM_E_ARG;
    if (p->mp) return mp_sync(p);
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (const int rc = pcg_finish(p)) return rc;
    HIP_TRY(p->ctx, hipStreamSynchronize(p->ctx->stream));
    if (const int rc = check_trsv(p)) return rc;
    if (p->timing) return collect_timing(p);
    p->runs_pending = 0;
    p->run_route.clear();
    return DBSLMM_OK;
}

int dbslmm_plan_kernel_ms(dbslmm_plan* p, double* ms_out, int32_t* launches_out) {
    if (!p || !ms_out) return DBSLMM_E_ARG;
    if (p->mp) {   // per kernel class the slowest device (the critical path of the node)
        int32_t runs = INT32_MAX;
        for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = 0.0;
        for (auto& sh : p->mp->shards) {
            if (p->ran && sh.run_copies.empty()) continue;   // a job the latest run skipped (stale)
            double ms[DBSLMM_K_COUNT];
            int32_t n = 0;
            dbslmm_plan_kernel_ms(sh.plan, ms, &n);
            for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = std::max(ms_out[k], ms[k]);
            runs = std::min(runs, n);
        }
        if (launches_out) *launches_out = runs == INT32_MAX ? 0 : runs;
        return DBSLMM_OK;
    }
    for (int k = 0; k < DBSLMM_K_COUNT; ++k) ms_out[k] = p->ms_runs ? p->ms_acc[k] / p->ms_runs : 0.0;
    if (launches_out) *launches_out = p->ms_runs;
    return DBSLMM_OK;
}

#ifdef DBSLMM_DIAG
// diagnostic build only (not in the public header): the substitution stamps of the last forward launch
extern "C" int dbslmm_diag_trsv_stamps(dbslmm_plan* p, unsigned long long* out, int n) {
    if (!p || !p->d_stamps) return DBSLMM_E_STATE;
    if (hipDeviceSynchronize() != hipSuccess) return DBSLMM_E_HIP;
    return hipMemcpy(out, p->d_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess
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
    if (!p->pcg_ran) return DBSLMM_OK;
    for (int b = 0; b < p->n_pblk; ++b) iters[p->h_blk_id[b]] = p->h_pmon[1 + b];
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
            if (p->ran && sh.run_copies.empty()) continue;   // a job the latest run skipped (stale)
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
    out[17] = p->pcg_ran ? 1.0 : 0.0;
    out[18] = p->pcg_ran ? p->pcg_iters_max : 0.0;
    out[19] = p->pcg_ran ? p->pcg_cbytes : 0.0;
    out[20] = p->pcg_ran ? p->pcg_pbytes : 0.0;
    out[21] = p->pcg_ran ? p->pcg_fbytes : 0.0;
    if (p->cg_ran && p->d_cgit) {   // the passes each tiled block ran before it converged (run_multi is synchronous)
        std::vector<int32_t> it(std::max(1, p->n_nonempty));
        if (hipSetDevice(p->ctx->device) != hipSuccess ||
            hipMemcpy(it.data(), p->d_cgit, it.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
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
        if (!p->ran) { p->ctx->err = "plan_download before plan_run"; return DBSLMM_E_STATE; }
        return mp_download(p, p->var_copy, beta_s, beta_l, block_status);
    }
    return download_copy(p, p->var_copy, beta_s, beta_l, block_status);
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

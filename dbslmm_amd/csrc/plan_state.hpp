// plan_state.hpp -- what a context and a plan hold between calls (included by plan.hip ahead of the
// host parts: upload.hip, route_factor.hip, route_pcg.hip, panel_api.hip, multi.hip), and the macros
// every entry point reports errors with.
#pragma once

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

// The options plan_create copied from dbslmm_options: never written afterwards.
struct PlanOptions {
    int32_t solver = 0;            // 0 auto, 1 factorisation, 2 PCG
    double pcg_tol = 1e-12;
    int32_t pcg_maxit = 1000;
    bool pcg_fused = true;         // small one-column blocks solved whole by dbslmm_pcg_block
    int32_t pcg_block_wgs = 0;     // a cap on dbslmm_pcg_block's workgroups (0: none)
    bool stream_out = true;        // a PCG run of dbslmm_plan_run_multi streams its results (StreamOut)
    int32_t h2f_mode = 0;
    double cheb_tol = 1e-9;
    bool cheb_fused = false;
    bool h2f_cg = false;           // h2f_iter: the tiled blocks' copies by CG
    int32_t debug_delay_us = 0;    // (tests)
    int32_t debug_stop = 0;        // (tests)
};

// What the latest run left behind.  Written by close_run (plan.hip) alone: each route, the debug_stop
// exit, the variance's re-solve and mp_run (multi.hip) spell out the whole record there.
struct LastRun {
    bool ran = false;
    bool stopped = false;          // it stopped after the Gram (debug_stop = 1): no betas
    double sigma_run = 0.0;        // sigma_s of the factorisation held in d_M
    int32_t var_copy = 0;          // copy holding the latest factorisation (variance)
    int32_t score_copies = 0;      // copies of the latest user run (dbslmm_plan_score)
    bool score_stale = false;      // the variance's re-solve has overwritten copy 0 of its results
    bool pcg_ran = false;          // it took the PCG route
    bool pcg_pending_var = false;  // ... so the variance needs a factorisation first
    int32_t cheb_base = -1;        // base copy of its h2f iterations (-1: none); workload [15]
    bool cheb_pending_var = false; // copy var_copy's tiled blocks are not factored yet
    bool cg_ran = false;           // it iterated by CG (workload [16] is counted from d_cgit on query)
    double cheb_iters = 0;         // workload [14]: a priori h2f iterations, summed over the copy groups
    double cheb_bytes = 0;         // workload [16]: the bytes their substitutions stream
};

// The PCG route's layout and run state (route_pcg.hip, pcg.hip).
struct PcgState {
    bool g16 = false;              // n_ref <= 16383: the integer Gram fits uint16
    int32_t m_blocks = -1;         // blocks with missing calls (fp64 Sigma products); -1 unknown
    uint16_t* d_G16 = nullptr;     // integer Gram: per block Tb*128 x Tb*128 (zero past m)
    int64_t* d_off16 = nullptr;    // ... its offset per block
    int32_t* d_ld16 = nullptr;     // ... its row stride per block (Tb * 128)
    std::vector<int64_t> h_off16;
    int32_t n = 0;                 // copies the PCG buffers are laid out for
    PcgBlk* d_pblk = nullptr;
    int4* d_pitem = nullptr;
    int2* d_prow = nullptr;
    int32_t n_pblk = 0, n_pitem = 0, n_prow = 0;
    int32_t n_pitem_chip = 0, n_prow_chip = 0;   // ... of them, those of the chip-wide blocks (listed first)
    int32_t n_phead = 0;           // d_prow's tail past n_prow: one (block, -1) per block solved whole
    bool trim = false;             // launch only those: no block dbslmm_pcg_block takes has missing calls
    int32_t run = pcg::kRunMax;    // tiles per product item (pcg_layout)
    int2* d_pflist = nullptr;      // the blocks solved whole: their (PcgBlk, copy) sequences (biggest first)
    int32_t* d_pfnext = nullptr;   // ... the next list index to take (16 B, zeroed per run)
    int32_t n_pflist = 0;
    std::vector<char> h_pfused;    // per PcgBlk: 1 = in that list
    std::vector<int32_t> h_pnseq;  // ... its sequences there (1, or the copies with large SNPs)
    bool join = false;             // the main stream still has to wait for dbslmm_pcg_block
    double *d_pvec = nullptr, *d_ppart = nullptr, *d_pdot = nullptr, *d_pqs = nullptr;
    int32_t *d_pcnv = nullptr, *d_pitb = nullptr, *d_pdone = nullptr, *d_pact = nullptr, *d_pfin = nullptr;
    int64_t vstride = 0;
    PinnedBuf mon;                 // int32: [active | itb per block] after a chunk
    int32_t it = 0;                // iterations enqueued by the current run
    int32_t need = -1;             // chip-wide iterations the latest finished run needed (-1: no run yet)
    int32_t iters_max = 0;         // ... and the iterations of its slowest block (any path)
    bool pending = false;          // a PCG run whose convergence has not been checked yet
    std::vector<double> h_pmat, h_ppart;   // per PcgBlk: lower-triangle bytes (uint16) / partial-sum bytes per iteration
    std::vector<char> h_pmiss;     // per PcgBlk: missing calls (fp64 Sigma, 4x the matrix bytes)
    double cbytes = 0.0, pbytes = 0.0, fbytes = 0.0;   // the latest run (workload [19]-[21])
    PcgArgs args{};                // the arguments of the latest PCG run (continuation chunks)
    int32_t* h_mon() const { return mon.get<int32_t>(); }
};

// Streamed results (dbslmm_options.stream_out, route_pcg.hip): on the PCG route of
// dbslmm_plan_run_multi the kernels write every result to a host-visible mirror as well and flag
// each (route block, copy) they finish (dbslmm_pcg_block, dbslmm_pcg_update), and the calling thread
// copies flagged blocks into the caller's arrays while the GPU still iterates (stream_results).
struct StreamOut {
    bool want = false;             // the call in progress may stream (dbslmm_plan_run_multi)
    bool active = false;           // the latest PCG run writes the mirror
    // mapped, coherent: [beta_s | beta_l | status], copy-major (the layout and strides of the device
    // arrays, n copies), and int32 [route block * n + copy] = run once finished
    PinnedBuf mir{hipHostMallocMapped | hipHostMallocCoherent}, mflag{hipHostMallocMapped | hipHostMallocCoherent};
    int32_t n = 0;                 // copies of the latest streamed run
    int32_t run = 0;               // its number (per plan; flags of earlier runs never match)
    EventList ev;                  // [0]: after the last work a chunk enqueued
    std::vector<int2> h_pfpairs;   // the host's scan order: dbslmm_pcg_block's (route block, copy) pairs in its
                                   // list order, then the chip-wide blocks'
    std::vector<int32_t> done;     // [route block * n + copy] = run once copied out
};

// The factorisation route's state (route_factor.hip): the tiled sequences and their graphs, the
// persistent substitutions (trsv.hip: tile work lists of the tiled blocks in forward / backward
// dependency order, tile flags + ticket counter + error word) and the h2f copies iterated on one
// factor (Chebyshev / CG; iteration vectors [Y, Z, X, R, D, S] x kMaxR x n_slots).
struct FactorState {
    int32_t* d_tlist = nullptr;         // work lists of the tiled sequence (tl, tl_rest)
    // h2f without iteration: one merged tiled sequence factors all copies (built for multi_n copies)
    std::vector<TLaunch> tl_multi;
    int32_t* d_tlist_multi = nullptr;
    int32_t multi_n = 0;
    GraphExecs graph_multi;             // [0]: that sequence, captured
    GraphExecs graph_copy;              // [c]: the single-copy tiled sequence on copy c
    GraphExecs graph_rest;              // ... and the rest sequence (lead group)
    EventList tev, tev_rest;            // dependencies between a tiled sequence's two streams (main / rest)
    int32_t *d_tri_f = nullptr, *d_tri_b = nullptr, *d_foff = nullptr, *d_tflags = nullptr, *d_tb = nullptr;
    int32_t* d_tepi = nullptr;          // per tile: epoch of its last stored Chebyshev update
    int32_t* d_cheb_items = nullptr;    // work list of the fused Chebyshev launch (K iterations)
    int32_t n_cheb_items = 0, cheb_items_K = -1;
    int32_t trsv_epoch = 0;             // tile-flag value of the latest substitution launch
    double h2f_tol = 1e-9;              // the current run's target for its iterated copies (run_impl)
    double* d_cgrec = nullptr;          // CG: per non-empty block and copy {gamma, alpha}
    int32_t* d_cgconv = nullptr;        // CG: per non-empty block, its copies have converged
    int32_t* d_cgit = nullptr;          // CG: per non-empty block, iterations of the latest run
    int32_t* d_tcheb_blocks = nullptr;  // sub_block: the rest group's blocks, largest first
    bool trsv_pending = false;          // a persistent substitution ran since the last error check
    bool trsv_failed = false;           // ... and one of its hand-off waits gave up (sticky until the next run)
    unsigned long long* d_stamps = nullptr;  // diagnostic builds (DBSLMM_DIAG) only
    double* d_cheb = nullptr;
    double* d_coef = nullptr;
    int32_t coef_cap = 0;
    std::vector<double> h_coef;         // the coefficients in d_coef
    void drop_graphs() {                // captured graphs hold device pointers: gone when those move
        graph_multi.reset();
        graph_copy.reset();
        graph_rest.reset();
    }
};

// Timing (dbslmm_plan_enable_timing; plan.hip: open_timed_run, record_instants, collect_timing).
struct Timing {
    bool timing = false;
    EventList ev{hipEventDefault};  // kEvCount per run
    std::vector<char> run_route;    // per pending timed run: 1 = PCG
    int runs_pending = 0;
    double ms_acc[DBSLMM_K_COUNT] = {0, 0, 0, 0, 0, 0};
    int32_t ms_runs = 0;
    hipEvent_t pcg_ev_end = nullptr;   // the pending PCG run's end event (one of ev; re-recorded by a continuation)
};

// (the host layout plan_create computed lives in the base: plan_layout.hpp)
struct dbslmm_plan : PlanLayout::Kept {
    dbslmm_ctx* ctx = nullptr;
    dbslmm_mplan* mp = nullptr;        // multi-device plan: every call fans out over its shards
    int32_t n_ref = 0, n_obs = 0, num_block = 0;
    double sigma_s = 0.0, tau = 0.8;
    int64_t bed_len = 0;
    PlanOptions opt;
    LastRun last;
    int64_t n_runs = 0;                // completed run enqueues (graphs are captured from the second)
    bool force_factor = false;         // the call in progress is the variance's re-solve
    // device arrays shared by the routes and the panel entry points
    DevBufs bufs;                      // owns every d_* member of the plan and its groups (freed with it)
    PanelImage img;                    // own upload, or the context's cached image (shared)
    const uint8_t* d_img = nullptr;    // img.mem.get(): pitch kpad / 4, zero-dosage row img.n_rows
    int32_t *d_slot_pos = nullptr, *d_slot_block = nullptr, *d_slot_out = nullptr;
    double *d_z = nullptr, *d_S = nullptr, *d_mu = nullptr, *d_rsd = nullptr, *d_y = nullptr;
    int32_t *d_flags = nullptr, *d_status = nullptr, *d_order = nullptr, *d_blk_id = nullptr;
    int32_t *d_row0 = nullptr, *d_m = nullptr, *d_ms = nullptr, *d_ld = nullptr;
    int64_t* d_matoff = nullptr;
    GramTile* d_tiles = nullptr;       // 32 x 32 tiles of the small blocks (dbslmm_gram_i8)
    GramTile* d_btiles = nullptr;      // 128 x 128 tiles of the mid blocks, per-XCD queues
    GramTile* d_htiles = nullptr;      // 256 x 256 tiles of the big blocks, per-XCD queues
    double* d_M = nullptr;
    double *d_beta_s = nullptr, *d_beta_l = nullptr;
    double* d_dshift = nullptr;        // 1/(sigma_s n), read by the solve kernels
    // per-copy arrays: n_copies independent solves, copy c at d_M + c M_elems (and the per-copy sigma
    // scalar, scratch, betas, status: copy_view); allocated on the first run (ensure_copies)
    int32_t n_copies = 0;
    int32_t m_copies = 0;              // block-matrix copies allocated in d_M (<= n_copies)
    int64_t nbk = 1;                   // status entries per copy
    PinnedBuf pin;                     // landing buffer of the result downloads
    EventList dl_ev;                   // ... one event per downloaded copy
    PcgState pcg;
    StreamOut so;
    FactorState fac;
    Timing tm;
};

// Copy c's part of the per-copy arrays.
struct CopyView {
    double *M, *dshift, *y, *beta_s, *beta_l;
    int32_t* status;
};
static CopyView copy_view(const dbslmm_plan* p, int64_t c) {
    return {p->d_M + c * p->M_elems,   p->d_dshift + c,           p->d_y + c * p->n_slots,
            p->d_beta_s + c * p->n_s,  p->d_beta_l + c * p->n_l,  p->d_status + c * p->nbk};
}
// What the substitution and iteration kernels' argument structs share (trsv::Args, TChebArgs,
// trsv::CGArgs, which has no ld / matoff): the per-plan block table, and every copy's betas with
// their strides.
template <class A, class = void>
struct HasLd : std::false_type {};
template <class A>
struct HasLd<A, std::void_t<decltype(std::declval<A&>().ld)>> : std::true_type {};
template <class A>
static void set_plan_args(A& a, const dbslmm_plan* p, double inv_sqrt_n) {
    a.row0 = p->d_row0;
    a.m = p->d_m;
    a.ms = p->d_ms;
    a.blk_id = p->d_blk_id;
    a.slot_out = p->d_slot_out;
    if constexpr (HasLd<A>::value) {
        a.ld = p->d_ld;
        a.matoff = p->d_matoff;
    }
    a.inv_sqrt_n = inv_sqrt_n;
    a.beta_s = p->d_beta_s;
    a.beta_l = p->d_beta_l;
    a.ns_stride = p->n_s;
    a.nl_stride = p->n_l;
}

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

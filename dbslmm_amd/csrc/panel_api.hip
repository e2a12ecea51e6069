// panel_api.hip -- the entry points that read a panel beside the solve (included by plan.hip, inside
// its extern "C" block: same translation unit): the test-set variance and polygenic scores of a
// plan, and the context-level tools on a .bed (MAF, row statistics, standardised rows, the `valid`
// terms, LD r2, clumping, LD scores and the association scan; the host-only LD score regression,
// scan finish and t tail).  Each allocates for one call on a local DevBufs (dev_bufs.hpp).

// "<what>: <HIP error>" as the context's error
static int hip_fail(dbslmm_ctx* ctx, const char* what, hipError_t e) {
    ctx->err = std::string(what) + hipGetErrorString(e);
    return DBSLMM_E_HIP;
}

// The last h2f run iterated the last sigma's tiled blocks on another copy's factor and wrote no
// matrix for them: re-run that sigma alone (Gram + factorisation) so the variance has its factor.
// A multi-device plan does this for every shard (and waits) before any shard's variance starts,
// so no shard captures a graph while another runs the variance's synchronous calls.
static int variance_factor(dbslmm_plan* p) {
    if (const int rc = pcg_finish(p)) return rc;
    if (!p->last.cheb_pending_var && !p->last.pcg_pending_var) return DBSLMM_OK;
    const double sg = p->last.sigma_run;
    LastRun r = p->last;   // (cleared even if the re-solve below fails: it is not tried twice)
    r.cheb_pending_var = false;
    r.pcg_pending_var = false;
    close_run(p, r);
    p->force_factor = true;          // the variance needs the factor of this sigma
    const int rc = run_impl(p, &sg, 1);
    p->force_factor = false;
    return rc;
}

// What the variance and the scores both derive from a test panel on the host: the selected
// individuals (the constructor: nothing can fail) and the plan's slots in the test .bed (test_rows_map).
struct TestRows {
    std::vector<int32_t> sel;    // the individuals with indicator != 0 (readSNPIm skips only 0 entries)
    bool all = true;             // every individual is selected (no indicator, or no 0 in it)
    int32_t n_test = 0;
    int64_t tbps = 0;            // bytes per row of the test .bed
    int64_t n_rows = 0;          // its rows
    std::vector<int32_t> tpos;   // per slot: its test .bed row (-1: a padding slot)
    std::vector<int32_t> cpos;   // per slot: its row of the compacted rows (the slot itself; -1: padding)
    explicit TestRows(const dbslmm_test_panel* tp)
        : tbps((tp->n_total + 3) / 4), n_rows((tp->bed_len - 3) / tbps) {
        if (tp->indicator)
            for (int32_t i = 0; i < tp->n_total; ++i) {
                if (tp->indicator[i] != 0) sel.push_back(i);
                else all = false;
            }
        n_test = tp->indicator ? static_cast<int32_t>(sel.size()) : tp->n_total;
    }
};
static int test_rows_map(dbslmm_plan* p, const dbslmm_test_panel* tp, TestRows& T) {
    dbslmm_ctx* ctx = p->ctx;
    ARG_CHECK(ctx, tp->bed_len >= 3 + T.tbps, "test bed image shorter than one SNP row");
    T.tpos.resize(p->n_slots);
    T.cpos.resize(p->n_slots);
    for (int32_t s = 0; s < p->n_slots; ++s) {
        const int32_t o = p->h_slot_out[s];
        int32_t r = -1;
        if (o >= 0) r = tp->s_pos[o];
        else if (o != INT32_MIN) r = tp->l_pos[-1 - o];
        ARG_CHECK(ctx, o == INT32_MIN || (r >= 0 && r < T.n_rows), "test SNP bed row out of range");
        T.tpos[s] = r;
        T.cpos[s] = r >= 0 ? s : -1;
    }
    return DBSLMM_OK;
}

// The test .bed verbatim on the device (bed_len + kBedPad bytes, zeroed first); complete on return.
static hipError_t upload_test_bed(DevBufs& B, uint8_t** out, const dbslmm_test_panel* tp, hipStream_t st) {
    const hipError_t e = B.zeroed(out, tp->bed_len + kBedPad, st);
    return e != hipSuccess ? e : upload_staged(*out, tp->bed, tp->bed_len, st);
}

// Test-set variance: compact the test panel to the plan's slots and the
// indicator-1 individuals, standardise (readSNPIm + nomalizeVec over n_test), then one
// forward-substitution pass per block against the factor the solve left in d_M.
int dbslmm_plan_variance(dbslmm_plan* p, const dbslmm_test_panel* tp, double* diags,
                         int32_t* n_test_out) {
    if (!p) return DBSLMM_E_ARG;
    dbslmm_ctx* ctx = p->ctx;
    if (!p->last.ran) { ctx->err = "plan_variance before plan_run"; return DBSLMM_E_STATE; }
    if (p->last.stopped) { ctx->err = "plan_variance after a run stopped at the Gram (debug_stop)"; return DBSLMM_E_STATE; }
    if (p->mp) return mp_variance(p, tp, diags, n_test_out);
    ARG_CHECK(ctx, tp && tp->bed && tp->indicator && tp->n_total > 0, "bad test panel");
    if (const int rc = variance_factor(p)) return rc;
    ARG_CHECK(ctx, p->n_s == 0 || tp->s_pos, "test panel s_pos missing");
    ARG_CHECK(ctx, p->n_l == 0 || tp->l_pos, "test panel l_pos missing");
    TestRows T(tp);
    const int32_t n_test = T.n_test;
    if (n_test_out) *n_test_out = n_test;
    if (n_test == 0 || p->num_block == 0) return DBSLMM_OK;   // (before the row checks, unlike the scores)
    ARG_CHECK(ctx, diags, "null diags");
    if (const int rc = test_rows_map(p, tp, T)) return rc;
    const int64_t nt_pad = round_up(n_test, 64);
    const int64_t cpitch = nt_pad / 4;          // the compacted rows in the panel image's format
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint8_t *d_tbed = nullptr, *d_cbed = nullptr;
    int32_t *d_tpos = nullptr, *d_sel = nullptr, *d_cpos = nullptr;
    double *d_mu = nullptr, *d_rsd = nullptr, *d_Y = nullptr, *d_diags = nullptr;
    const size_t nsl = static_cast<size_t>(p->n_slots);
    const size_t ndiag = static_cast<size_t>(n_test) * p->num_block;
    // synchronous allocations and copies: ordered against other host threads' graph captures
    // (several shards of a multi-device plan on one device)
    std::lock_guard<std::mutex> lk(g_capture_mu);
    DevBufs B(ctx->device);
    hipError_t e;
    if ((e = upload_test_bed(B, &d_tbed, tp, st)) != hipSuccess ||
        (e = B.upload(&d_tpos, T.tpos, st)) != hipSuccess || (e = B.upload(&d_sel, T.sel, st)) != hipSuccess ||
        (e = B.upload(&d_cpos, T.cpos, st)) != hipSuccess ||
        (e = B.alloc(&d_cbed, nsl * cpitch)) != hipSuccess ||   // (dbslmm_test_compact writes every byte)
        (e = B.alloc(&d_mu, nsl)) != hipSuccess || (e = B.alloc(&d_rsd, nsl)) != hipSuccess ||
        (e = B.alloc(&d_Y, nsl * nt_pad)) != hipSuccess || (e = B.zeroed(&d_diags, ndiag, st)) != hipSuccess)
        return hip_fail(ctx, "variance alloc/upload: ", e);
    if (p->n_slots > 0 && p->n_nonempty > 0) {
        hipLaunchKernelGGL(dbslmm_test_compact, dim3(static_cast<unsigned>((cpitch + 255) / 256), p->n_slots),
                           dim3(256), 0, st, d_tbed, T.tbps, d_tpos, p->n_slots, d_sel, n_test, cpitch, d_cbed);
        hipLaunchKernelGGL(dbslmm_snp_stats, dim3(static_cast<unsigned>((p->n_slots + 3) / 4)), dim3(256), 0,
                           st, d_cbed, n_test, cpitch, d_cpos, p->n_slots, d_mu, d_rsd);
        const CopyView fv = copy_view(p, p->last.var_copy);   // the copy holding the latest factorisation
        hipLaunchKernelGGL(dbslmm_variance, dim3(static_cast<unsigned>(nt_pad / 64), p->n_nonempty),
                           dim3(256), 0, st, fv.M, p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff, p->d_blk_id, fv.status,
                           d_cbed, cpitch, d_mu, d_rsd, n_test,
                           p->last.sigma_run, static_cast<double>(p->n_obs), d_Y, nt_pad, d_diags);
    }
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess ||
        (e = hipMemcpy(diags, d_diags, ndiag * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(ctx, "variance run: ", e);
    return DBSLMM_OK;
}

// Polygenic scores of the test panel for every copy of the latest run (score.hip).  Two feeders of
// one kernel: all individuals selected -> the test .bed as a panel image (repitch + row table; the
// per-slot statistics gathered from the table, rows gathered by the slots' test rows); a subset ->
// the variance path's compaction + statistics, rows in slot order.
int dbslmm_plan_score(dbslmm_plan* p, const dbslmm_test_panel* tp, const dbslmm_score_args* args,
                      int32_t n_copies, double* scores, int32_t* dropped, int32_t* n_test_out,
                      double* gpu_ms) {
    if (!p) return DBSLMM_E_ARG;
    dbslmm_ctx* ctx = p->ctx;
    if (!p->last.ran) { ctx->err = "plan_score before plan_run"; return DBSLMM_E_STATE; }
    if (p->last.stopped) { ctx->err = "plan_score after a run stopped at the Gram (debug_stop)"; return DBSLMM_E_STATE; }
    ARG_CHECK(ctx, tp && tp->bed && tp->n_total > 0, "bad test panel");
    const int32_t mode = args ? args->mode : DBSLMM_SCORE_COUNTS;
    ARG_CHECK(ctx, mode == DBSLMM_SCORE_COUNTS || mode == DBSLMM_SCORE_STD, "score mode");
    ARG_CHECK(ctx, !args || args->chunk_slots >= 0, "chunk_slots must be >= 0");
    ARG_CHECK(ctx, n_copies == p->last.score_copies, "n_copies must equal the copies of the latest run");
    ARG_CHECK(ctx, p->n_s == 0 || tp->s_pos, "test panel s_pos missing");
    ARG_CHECK(ctx, p->n_l == 0 || tp->l_pos, "test panel l_pos missing");
    if (p->mp) return mp_score(p, tp, args, n_copies, scores, dropped, n_test_out, gpu_ms);
    if (p->last.score_stale) {
        ctx->err = "plan_score after plan_variance re-solved the latest sigma (the device results of copy 0 are "
                   "overwritten): score before the variance, or run again";
        return DBSLMM_E_STATE;
    }
    if (const int rc = drain(p)) return rc;            // a run still pending
    TestRows T(tp);
    const bool all = T.all;
    const int32_t n_test = T.n_test;
    if (n_test_out) *n_test_out = n_test;
    if (gpu_ms) *gpu_ms = 0.0;
    // (the all-selected feeder makes a panel image of the test .bed: int32 rows.  A .bed shorter than
    // one row has no rows, so this check never hides test_rows_map's own)
    ARG_CHECK(ctx, T.n_rows < INT32_MAX, "test bed image has too many rows");
    if (const int rc = test_rows_map(p, tp, T)) return rc;   // (before the n_test == 0 return, unlike the variance)
    const int64_t tbps = T.tbps, n_rows = T.n_rows;
    const std::vector<int32_t>& tpos = T.tpos;
    if (n_test == 0) {
        if (dropped) std::fill(dropped, dropped + n_copies, 0);
        return DBSLMM_OK;
    }
    ARG_CHECK(ctx, scores, "null scores");
    const size_t n_out = static_cast<size_t>(n_copies) * n_test;
    if (p->n_slots == 0 || p->n_nonempty == 0) {       // no SNP: every score is the empty sum
        std::fill(scores, scores + n_out, 0.0);
        if (dropped) std::fill(dropped, dropped + n_copies, 0);
        return DBSLMM_OK;
    }
    // (a multiple of the kernel's prefetch depth: a chunk_slots between two multiples acts as the next one)
    const int32_t chunk_slots = static_cast<int32_t>(std::min<int64_t>(
        round_up(args && args->chunk_slots > 0 ? args->chunk_slots : score::kChunkSlots, score::kDepth), 1 << 30));
    const int32_t n_chunks = (p->n_slots + chunk_slots - 1) / chunk_slots;
    const int64_t stride64 = static_cast<int64_t>(n_chunks) * chunk_slots;   // slots incl. the last chunk's tail
    ARG_CHECK(ctx, stride64 + score::kDepth < INT32_MAX, "chunk_slots too large");
    const int32_t stride = static_cast<int32_t>(stride64);
    const int32_t n_words = (n_test + 15) / 16;
    const int64_t n_pad = 16 * static_cast<int64_t>(n_words);
    ARG_CHECK(ctx, n_chunks <= 65535, "chunk_slots too small for this plan (more than 65535 chunks)");
    const int64_t cpitch = round_up(n_test, 256) / 4;   // the compacted rows in the panel image's format
    // the row the product kernel loads for every slot it may touch (a chunk's tail and the
    // prefetch past it included): a padding slot and the tail read a valid row with a = 0 --
    // image feeder: the image's zero-dosage row; compaction feeder: the slot's own row (all 11), row 0
    std::vector<int32_t> srow(static_cast<size_t>(stride) + score::kDepth);
    for (size_t s = 0; s < srow.size(); ++s) {
        const bool real = s < static_cast<size_t>(p->n_slots);
        if (all) srow[s] = real && tpos[s] >= 0 ? tpos[s] : static_cast<int32_t>(n_rows);
        else srow[s] = real ? static_cast<int32_t>(s) : 0;
    }
    std::vector<double> hw_s, hw_l;
    std::vector<uint8_t> hf_s, hf_l;
    if (args && args->w_s) hw_s.assign(args->w_s, args->w_s + p->n_s);
    if (args && args->w_l) hw_l.assign(args->w_l, args->w_l + p->n_l);
    if (args && args->flip_s) hf_s.assign(args->flip_s, args->flip_s + p->n_s);
    if (args && args->flip_l) hf_l.assign(args->flip_l, args->flip_l + p->n_l);
    hipStream_t st = ctx->stream;
    uint8_t *d_tbed = nullptr, *d_cbed = nullptr, *d_fs = nullptr, *d_fl = nullptr;
    int32_t *d_tpos = nullptr, *d_sel = nullptr, *d_cpos = nullptr, *d_drop = nullptr, *d_srow = nullptr;
    double *d_mu = nullptr, *d_rsd = nullptr, *d_ws = nullptr, *d_wl = nullptr, *d_coef = nullptr, *d_kc = nullptr,
           *d_part = nullptr, *d_scores = nullptr;
    PanelImage im;
    const size_t nsl = static_cast<size_t>(p->n_slots);
    const size_t ncoef = static_cast<size_t>(n_copies) * stride;
    const int pass_max = std::min<int>(score::kMaxPass, n_copies);
    // synchronous allocations: ordered against other host threads' graph captures
    std::lock_guard<std::mutex> lk(g_capture_mu);
    EventList ev{hipEventDefault};   // [0], [1]: around the call's kernels
    DevBufs B(ctx->device);
    hipError_t e;
    if ((e = upload_test_bed(B, &d_tbed, tp, st)) != hipSuccess ||
        (e = B.upload(&d_tpos, tpos, st)) != hipSuccess || (e = B.upload(&d_srow, srow, st)) != hipSuccess ||
        (e = B.alloc(&d_mu, nsl)) != hipSuccess || (e = B.alloc(&d_rsd, nsl)) != hipSuccess ||
        (e = B.alloc(&d_coef, 3 * ncoef)) != hipSuccess ||
        (e = B.alloc(&d_kc, static_cast<size_t>(n_copies) * (1 + n_chunks))) != hipSuccess ||   // K_c | per chunk
        (e = B.zeroed(&d_drop, n_copies, st)) != hipSuccess ||
        (e = B.alloc(&d_part, static_cast<size_t>(n_chunks) * pass_max * n_pad)) != hipSuccess ||
        (e = B.alloc(&d_scores, n_out)) != hipSuccess ||
        (!hw_s.empty() && (e = B.upload(&d_ws, hw_s, st)) != hipSuccess) ||
        (!hw_l.empty() && (e = B.upload(&d_wl, hw_l, st)) != hipSuccess) ||
        (!hf_s.empty() && (e = B.upload(&d_fs, hf_s, st)) != hipSuccess) ||
        (!hf_l.empty() && (e = B.upload(&d_fl, hf_l, st)) != hipSuccess) || (e = ev.grow(2)) != hipSuccess)
        return hip_fail(ctx, "score alloc/upload: ", e);
    const uint8_t* rows = nullptr;    // the 2-bit rows the product reads and their pitch
    int64_t pitch = 0;
    if (all) {
        if ((e = image_from_verbatim(ctx, d_tbed, tp->bed_len, tp->n_total, &im)) != hipSuccess)
            return hip_fail(ctx, "score panel image: ", e);
        hipLaunchKernelGGL(dbslmm_slot_stats, dim3((p->n_slots + 255) / 256), dim3(256), 0, st, im.rows(),
                           tp->n_total, d_tpos, nullptr, p->n_slots, nullptr, d_mu, d_rsd, nullptr);
        rows = im.mem.get();
        pitch = im.pitch;
    } else {
        if ((e = B.upload(&d_sel, T.sel, st)) != hipSuccess || (e = B.upload(&d_cpos, T.cpos, st)) != hipSuccess ||
            (e = B.alloc(&d_cbed, nsl * cpitch)) != hipSuccess)   // (dbslmm_test_compact writes every byte)
            return hip_fail(ctx, "score alloc/upload: ", e);
        for (int32_t q0 = 0; q0 < p->n_slots; q0 += 32768) {   // (one grid row per slot)
            const int32_t nq = std::min<int32_t>(32768, p->n_slots - q0);
            hipLaunchKernelGGL(dbslmm_test_compact, dim3(static_cast<unsigned>((cpitch + 255) / 256), nq),
                               dim3(256), 0, st, d_tbed, tbps, d_tpos + q0, nq, d_sel, n_test, cpitch,
                               d_cbed + static_cast<int64_t>(q0) * cpitch);
        }
        hipLaunchKernelGGL(dbslmm_snp_stats, dim3(static_cast<unsigned>((p->n_slots + 3) / 4)), dim3(256), 0,
                           st, d_cbed, n_test, cpitch, d_cpos, p->n_slots, d_mu, d_rsd);
        rows = d_cbed;
        pitch = cpitch;
    }
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[0], st)) != hipSuccess)
        return hip_fail(ctx, "score statistics: ", e);
    double *d_a = d_coef, *d_am = d_coef + ncoef, *d_k = d_coef + 2 * ncoef;
    hipLaunchKernelGGL(dbslmm_score_coef, dim3((stride + 255) / 256, n_copies), dim3(256), 0, st,
                       p->d_slot_out, p->d_slot_block, p->d_blk_id, p->d_status, p->nbk, p->d_beta_s,
                       p->d_beta_l, p->n_s, p->n_l, d_ws, d_wl, d_fs, d_fl, d_mu, d_rsd, p->n_slots, stride,
                       n_copies, mode, n_test, d_a, d_am, d_k, d_drop);
    hipLaunchKernelGGL(dbslmm_score_const, dim3(n_chunks, n_copies), dim3(256), 0, st, d_k, stride, chunk_slots,
                       static_cast<int64_t>(stride), d_kc + n_copies);
    hipLaunchKernelGGL(dbslmm_score_const, dim3(1, n_copies), dim3(256), 0, st, d_kc + n_copies, n_chunks, n_chunks,
                       static_cast<int64_t>(n_chunks), d_kc);
    const dim3 pgrid((n_words + 255) / 256, n_chunks);
    for (int c0 = 0; c0 < n_copies; c0 += score::kMaxPass) {   // at most kMaxPass copies per pass
        const int nc = std::min<int>(score::kMaxPass, n_copies - c0);
        const double* pa = d_a + static_cast<size_t>(c0) * stride;
        const double* pam = d_am + static_cast<size_t>(c0) * stride;
#define DBSLMM_SCORE_PASS(NC)                                                                                   \
    hipLaunchKernelGGL(dbslmm_score_partial<NC>, pgrid, dim3(256), 0, st, rows, pitch, d_srow, pa, pam, stride, \
                       chunk_slots, n_words, d_part)
        if (nc == 1) DBSLMM_SCORE_PASS(1);
        else if (nc == 2) DBSLMM_SCORE_PASS(2);
        else if (nc == 3) DBSLMM_SCORE_PASS(3);
        else DBSLMM_SCORE_PASS(4);
#undef DBSLMM_SCORE_PASS
        hipLaunchKernelGGL(dbslmm_score_reduce, dim3((n_test + 255) / 256, nc), dim3(256), 0, st, d_part, n_chunks,
                           nc, n_pad, d_kc + c0, n_test, d_scores + static_cast<size_t>(c0) * n_test);
    }
    float ms = 0.0f;
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[1], st)) != hipSuccess ||
        (e = hipMemcpyAsync(scores, d_scores, n_out * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (dropped && (e = hipMemcpyAsync(dropped, d_drop, n_copies * sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) ||
        (e = hipStreamSynchronize(st)) != hipSuccess || (e = hipEventElapsedTime(&ms, ev[0], ev[1])) != hipSuccess)
        return hip_fail(ctx, "score run: ", e);
    if (gpu_ms) *gpu_ms = ms;
    return DBSLMM_OK;
}

// MAF pass over the first n_snp rows (IO::readBim, dtpr.cpp:93-102).
int dbslmm_bed_maf(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                   int64_t n_snp, double* maf) {
    if (!ctx) return DBSLMM_E_ARG;
    ARG_CHECK(ctx, bed && maf && n_ref > 1 && n_snp >= 0 && n_snp < INT32_MAX, "bad arguments");
    ARG_CHECK(ctx, bed_len >= 3 + n_snp * bed_row_bytes(n_ref), "bed image shorter than n_snp rows");
    if (n_snp == 0) return DBSLMM_OK;
    if (!ctx->subs.empty()) return mp_bed_maf(ctx, bed, n_ref, n_snp, maf);
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PanelImage im;            // the context's cached image of this host range, or an upload of our own
    DevBufs B(ctx->device);
    char* d_work = nullptr;   // one allocation: mu | S | maf (doubles), then the per-row missing flags
    hipError_t e;
    const size_t nd = static_cast<size_t>(n_snp) * sizeof(double);
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess ||
        (e = B.alloc(&d_work, 3 * nd + n_snp * sizeof(int32_t))) != hipSuccess ||
        (e = hipMemsetAsync(d_work + 3 * nd, 0, n_snp * sizeof(int32_t), ctx->stream)) != hipSuccess)
        return hip_fail(ctx, "bed_maf alloc/upload: ", e);
    double* d_mu = reinterpret_cast<double*>(d_work);
    double* d_S = d_mu + n_snp;
    double* d_maf = d_S + n_snp;
    int32_t* d_miss = reinterpret_cast<int32_t*>(d_maf + n_snp);
    const uint8_t* db = im.mem.get();
    // from the image's row table: row k = image row k (null row lists); per-row missing-call
    // flags (row k's "block" is k)
    hipLaunchKernelGGL(dbslmm_slot_stats, dim3(static_cast<unsigned>((n_snp + 255) / 256)), dim3(256), 0,
                       ctx->stream, im.rows(), n_ref, nullptr, nullptr, static_cast<int32_t>(n_snp),
                       d_S, d_mu, nullptr, d_miss);
    hipLaunchKernelGGL(dbslmm_maf_arma, dim3(static_cast<unsigned>((n_snp + 255) / 256)), dim3(256), 0,
                       ctx->stream, db, n_ref, im.pitch, nullptr, static_cast<int32_t>(n_snp), d_mu, d_maf,
                       d_S, d_miss);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(maf, d_maf, nd, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return hip_fail(ctx, "bed_maf run: ", e);
    return DBSLMM_OK;
}

// The row table of the panel's image, rows [0, n_rows): the exact integers {sum, sumsq, nmiss}.
int dbslmm_bed_row_stats(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                         int64_t n_rows, int32_t* out) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_bed_row_stats(ctx0_, bed, bed_len, n_ref, n_rows, out));
    ARG_CHECK(ctx, bed && out && n_ref > 1 && n_rows >= 0 && n_rows < INT32_MAX, "bad arguments");
    ARG_CHECK(ctx, bed_len >= 3 + n_rows * bed_row_bytes(n_ref), "bed image shorter than n_rows rows");
    if (n_rows == 0) return DBSLMM_OK;
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PanelImage im;
    std::vector<int32_t> h(static_cast<size_t>(n_rows) * 4);
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess ||
        (e = hipMemcpyAsync(h.data(), im.rows(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        return hip_fail(ctx, "bed_row_stats: ", e);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int k = 0; k < 3; ++k) out[3 * r + k] = h[4 * r + k];
    return DBSLMM_OK;
}

// The single row-range check of the row-list entry points: every listed row lies inside the .bed.
static int rows_in_bed(dbslmm_ctx* ctx, int64_t bed_len, int32_t n_ref, const int32_t* pos, int64_t n_rows) {
    const int64_t bps = bed_row_bytes(n_ref);
    for (int64_t j = 0; j < n_rows; ++j)
        ARG_CHECK(ctx, pos[j] >= 0 && 3 + (static_cast<int64_t>(pos[j]) + 1) * bps <= bed_len, "row out of range");
    return DBSLMM_OK;
}

int dbslmm_read_snp_std(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                        const int32_t* pos, int32_t n_rows, double* out, double* maf) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_read_snp_std(ctx0_, bed, bed_len, n_ref, pos, n_rows, out, maf));
    if (const int rc = ctx_ready(ctx)) return rc;
    ARG_CHECK(ctx, bed && pos && out && n_ref > 1 && n_rows >= 0, "bad arguments");
    if (const int rc = rows_in_bed(ctx, bed_len, n_ref, pos, n_rows)) return rc;
    if (n_rows == 0) return DBSLMM_OK;
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PanelImage im;
    DevBufs B(ctx->device);
    int32_t* d_pos = nullptr;
    double *d_mu = nullptr, *d_rsd = nullptr, *d_maf = nullptr, *d_out = nullptr;
    const std::vector<int32_t> hp(pos, pos + n_rows);
    const int64_t n_out = static_cast<int64_t>(n_rows) * n_ref;
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess ||
        (e = B.upload(&d_pos, hp, ctx->stream)) != hipSuccess ||
        (e = B.alloc(&d_mu, n_rows)) != hipSuccess || (e = B.alloc(&d_rsd, n_rows)) != hipSuccess ||
        (e = B.alloc(&d_maf, n_rows)) != hipSuccess || (e = B.alloc(&d_out, n_out)) != hipSuccess)
        return hip_fail(ctx, "read_snp_std alloc/upload: ", e);
    const uint8_t* db = im.mem.get();
    hipLaunchKernelGGL(dbslmm_slot_stats, dim3((n_rows + 255) / 256), dim3(256), 0, ctx->stream,
                       im.rows(), n_ref, d_pos, nullptr, n_rows, nullptr, d_mu, d_rsd, nullptr);
    hipLaunchKernelGGL(dbslmm_maf_arma, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0,
                       ctx->stream, db, n_ref, im.pitch, d_pos, n_rows, d_mu, d_maf, nullptr, nullptr);
    hipLaunchKernelGGL(dbslmm_std_columns, dim3(static_cast<unsigned>((n_out + 255) / 256)),
                       dim3(256), 0, ctx->stream, db, n_ref, im.pitch, d_pos, n_rows, d_mu, d_rsd,
                       d_out);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess ||
        (e = hipMemcpy(out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess ||
        (maf && (e = hipMemcpy(maf, d_maf, n_rows * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess))
        return hip_fail(ctx, "read_snp_std run: ", e);
    return DBSLMM_OK;
}

// External-validation terms of the `valid` tool (scr/validate.cpp:221-257).
int dbslmm_valid_blocks(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                        int32_t num_block, const int64_t* ptr, const int32_t* pos,
                        const double* z1, const double* z2, double* nume, double* deno) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_valid_blocks(ctx0_, bed, bed_len, n_ref, num_block, ptr, pos, z1, z2, nume, deno));
    if (const int rc = ctx_ready(ctx)) return rc;
    ARG_CHECK(ctx, bed && ptr && nume && deno && n_ref > 1 && num_block >= 0, "bad arguments");
    const int64_t n_rows = ptr[num_block];
    ARG_CHECK(ctx, n_rows >= 0 && n_rows < INT32_MAX && (n_rows == 0 || (pos && z1 && z2)), "bad CSR");
    for (int b = 0; b < num_block; ++b) ARG_CHECK(ctx, ptr[b + 1] >= ptr[b], "CSR offsets not monotone");
    if (const int rc = rows_in_bed(ctx, bed_len, n_ref, pos, n_rows)) return rc;
    // nume = z1 . z2 per block (host: O(m), in the reference's accumulation order)
    for (int b = 0; b < num_block; ++b) {
        double t = 0.0;
        for (int64_t j = ptr[b]; j < ptr[b + 1]; ++j) t += z1[j] * z2[j];
        nume[b] = t;
    }
    if (num_block == 0) return DBSLMM_OK;
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_words = (n_ref + 15) / 16;
    const int32_t n_chunks = static_cast<int32_t>((n_words + 255) / 256);
    PanelImage im;
    DevBufs B(ctx->device);
    int32_t* d_pos = nullptr;
    int64_t* d_ptr = nullptr;
    double *d_z1 = nullptr, *d_mu = nullptr, *d_rsd = nullptr, *d_part = nullptr, *d_deno = nullptr;
    const std::vector<int32_t> hp(pos, pos + n_rows);
    const std::vector<int64_t> hptr(ptr, ptr + num_block + 1);
    const std::vector<double> hz(z1, z1 + n_rows);
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess ||
        (e = B.upload(&d_pos, hp, ctx->stream)) != hipSuccess || (e = B.upload(&d_ptr, hptr, ctx->stream)) != hipSuccess ||
        (e = B.upload(&d_z1, hz, ctx->stream)) != hipSuccess ||
        (e = B.alloc(&d_mu, n_rows)) != hipSuccess || (e = B.alloc(&d_rsd, n_rows)) != hipSuccess ||
        (e = B.alloc(&d_part, static_cast<size_t>(num_block) * n_chunks)) != hipSuccess ||
        (e = B.alloc(&d_deno, num_block)) != hipSuccess)
        return hip_fail(ctx, "valid alloc/upload: ", e);
    const uint8_t* db = im.mem.get();
    if (n_rows > 0)
        hipLaunchKernelGGL(dbslmm_slot_stats, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0,
                           ctx->stream, im.rows(), n_ref, d_pos, nullptr, static_cast<int32_t>(n_rows),
                           nullptr, d_mu, d_rsd, nullptr);
    // grid rows stride over the blocks, so num_block is not bound by the grid-row limit
    constexpr int32_t kValidGridY = 65535;
    hipLaunchKernelGGL(dbslmm_valid_partial, dim3(n_chunks, std::min(num_block, kValidGridY)), dim3(256), 0,
                       ctx->stream, db, n_ref, im.pitch, d_ptr, d_pos, d_z1, d_mu, d_rsd, d_part, n_chunks,
                       num_block);
    hipLaunchKernelGGL(dbslmm_valid_reduce, dim3((num_block + 255) / 256), dim3(256), 0, ctx->stream,
                       d_part, n_chunks, num_block, static_cast<double>(n_ref), d_deno);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess ||
        (e = hipMemcpy(deno, d_deno, num_block * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(ctx, "valid run: ", e);
    return DBSLMM_OK;
}

// dbslmm_r2_tiles over the tiles of L on the panel's image: mask mode (h_masks: kClumpMaskWords words
// per tile; chr / bp in position order) or value mode (h_r2: n x n doubles).  pos = the bed rows in
// position order.  Every transfer on the context's stream; complete on return.
static int r2_tiles_run(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, const ClumpLayout& L,
                        const std::vector<int32_t>& pos, const std::vector<int32_t>* chr,
                        const std::vector<int64_t>* bp, double thr, int64_t window, uint32_t* h_masks,
                        double* h_r2, double* gpu_ms) {
    PanelImage im;
    EventList ev{hipEventDefault};   // [0], [1]: around the call's kernels
    DevBufs B(ctx->device);
    int32_t *d_pos = nullptr, *d_chr = nullptr;
    int64_t* d_bp = nullptr;
    ClumpTile* d_tiles = nullptr;
    uint32_t* d_masks = nullptr;
    double* d_r2 = nullptr;
    const int32_t n_tiles = static_cast<int32_t>(L.tiles.size());
    const size_t n_mask = static_cast<size_t>(n_tiles) * kClumpMaskWords;
    const size_t n_r2 = static_cast<size_t>(L.n) * L.n;
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess ||
        (e = B.upload(&d_pos, pos, ctx->stream)) != hipSuccess ||
        (e = B.upload(&d_tiles, L.tiles, ctx->stream)) != hipSuccess ||
        (chr && (e = B.upload(&d_chr, *chr, ctx->stream)) != hipSuccess) ||
        (bp && (e = B.upload(&d_bp, *bp, ctx->stream)) != hipSuccess) ||
        (h_masks && (e = B.alloc(&d_masks, n_mask)) != hipSuccess) ||
        (h_r2 && (e = B.alloc(&d_r2, n_r2)) != hipSuccess) ||
        (e = ev.grow(2)) != hipSuccess || (e = hipEventRecord(ev[0], ctx->stream)) != hipSuccess)
        return hip_fail(ctx, "r2 tiles alloc/upload: ", e);
    const int64_t kpad = im.pitch * 4;
    const dim3 grid(static_cast<unsigned>((n_tiles + 3) / 4));
    if (h_masks)
        hipLaunchKernelGGL(dbslmm_r2_tiles<true>, grid, dim3(256), 0, ctx->stream, im.mem.get(), kpad, im.rows(),
                           im.n_rows, n_ref, d_pos, L.n, d_tiles, n_tiles, d_chr, d_bp, thr, window, d_masks,
                           static_cast<double*>(nullptr));
    else
        hipLaunchKernelGGL(dbslmm_r2_tiles<false>, grid, dim3(256), 0, ctx->stream, im.mem.get(), kpad, im.rows(),
                           im.n_rows, n_ref, d_pos, L.n, d_tiles, n_tiles, static_cast<const int32_t*>(nullptr),
                           static_cast<const int64_t*>(nullptr), 0.0, int64_t(0), static_cast<uint32_t*>(nullptr),
                           d_r2);
    float ms = 0.0f;
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[1], ctx->stream)) != hipSuccess ||
        (h_masks && (e = hipMemcpyAsync(h_masks, d_masks, n_mask * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) ||
        (h_r2 && (e = hipMemcpyAsync(h_r2, d_r2, n_r2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess || (e = hipEventElapsedTime(&ms, ev[0], ev[1])) != hipSuccess)
        return hip_fail(ctx, "r2 tiles run: ", e);
    if (gpu_ms) *gpu_ms = ms;
    return DBSLMM_OK;
}

// the row-list checks shared by dbslmm_ld_r2 and dbslmm_clump: the FP4 Gram's range, then the rows
static int r2_rows_check(dbslmm_ctx* ctx, int64_t bed_len, int32_t n_ref, const int32_t* pos, int32_t n_rows) {
    ARG_CHECK(ctx, 9 * round_up(n_ref, gram::kKpadAlign) < (int64_t(1) << 24),
              "n_ref past the FP4 Gram's exact range (9 * roundup(n_ref, 256) < 2^24)");
    return rows_in_bed(ctx, bed_len, n_ref, pos, n_rows);
}

// LD r2 of every pair of the listed rows (clump.hip, value mode).
int dbslmm_ld_r2(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, const int32_t* pos,
                 int32_t n_rows, double* r2) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_ld_r2(ctx0_, bed, bed_len, n_ref, pos, n_rows, r2));
    ARG_CHECK(ctx, bed && n_ref > 1 && n_rows >= 0 && n_rows <= 8192 && (n_rows == 0 || (pos && r2)), "bad arguments");
    if (const int rc = r2_rows_check(ctx, bed_len, n_ref, pos, n_rows)) return rc;
    if (n_rows == 0) return DBSLMM_OK;
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ClumpLayout L = build_dense_layout(n_rows);
    return r2_tiles_run(ctx, bed, bed_len, n_ref, L, std::vector<int32_t>(pos, pos + n_rows), nullptr, nullptr, 0.0, 0,
                        nullptr, r2, nullptr);
}

// Clumping (software/DBSLMM.R:139-145, `plink --clump`): the index SNPs of the candidates.
int dbslmm_clump(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, int32_t n_cand,
                 const int32_t* pos, const int32_t* chr, const int64_t* bp, const dbslmm_clump_args* args,
                 int32_t* index_of, int32_t* n_index, double* gpu_ms) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_clump(ctx0_, bed, bed_len, n_ref, n_cand, pos, chr, bp, args, index_of, n_index, gpu_ms));
    ARG_CHECK(ctx, bed && args && n_ref > 1 && n_cand >= 0 && (n_cand == 0 || (pos && chr && bp && index_of)),
              "bad arguments");
    ARG_CHECK(ctx, args->r2 > 0.0 && args->r2 <= 1.0, "clump r2 threshold outside (0, 1]");
    ARG_CHECK(ctx, args->window_bp >= 0, "clump window below 0");
    if (const int rc = r2_rows_check(ctx, bed_len, n_ref, pos, n_cand)) return rc;
    if (n_index) *n_index = 0;
    if (gpu_ms) *gpu_ms = 0.0;
    if (n_cand == 0) return DBSLMM_OK;
    ClumpLayout L = build_clump_layout(n_cand, chr, bp, args->window_bp);
    clump_index_columns(L);
    std::vector<uint32_t> masks(L.tiles.size() * kClumpMaskWords);
    if (!L.tiles.empty()) {
        KEY_CHECK(ctx, bed, bed_len, n_ref);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<int32_t> spos(static_cast<size_t>(n_cand)), schr(static_cast<size_t>(n_cand));
        std::vector<int64_t> sbp(static_cast<size_t>(n_cand));
        for (int32_t p = 0; p < n_cand; ++p) {
            const int32_t k = L.order[static_cast<size_t>(p)];
            spos[static_cast<size_t>(p)] = pos[k];
            schr[static_cast<size_t>(p)] = chr[k];
            sbp[static_cast<size_t>(p)] = bp[k];
        }
        if (const int rc = r2_tiles_run(ctx, bed, bed_len, n_ref, L, spos, &schr, &sbp, args->r2, args->window_bp,
                                        masks.data(), nullptr, gpu_ms))
            return rc;
    }
    const int32_t ni = clump_greedy(L, masks.data(), index_of);
    if (n_index) *n_index = ni;
    return DBSLMM_OK;
}

// LD scores of the listed rows (ldscore.hip): the band of 128 x 128 tiles of ldsc_layout.hpp in
// slices of at most max_tiles_per_launch tiles, dbslmm_l2_reduce after every slice.
int dbslmm_ld_scores(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, int32_t n_rows,
                     const int32_t* pos, const int32_t* chr, const int64_t* bp, const dbslmm_l2_args* args,
                     double* l2, int32_t* n_window, double* gpu_ms) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_ld_scores(ctx0_, bed, bed_len, n_ref, n_rows, pos, chr, bp, args, l2, n_window, gpu_ms));
    if (const int rc = ctx_ready(ctx)) return rc;
    const dbslmm_l2_args a = args ? *args : dbslmm_l2_args{1000000, 1, 0};
    ARG_CHECK(ctx, bed && n_ref > 1 && n_rows >= 0 && (n_rows == 0 || (pos && chr && bp && l2)), "bad arguments");
    ARG_CHECK(ctx, a.window_bp >= 0, "LD score window below 0");
    ARG_CHECK(ctx, a.max_tiles_per_launch >= 0, "max_tiles_per_launch below 0");
    ARG_CHECK(ctx, !a.unbiased || n_ref > 2, "the unbiased LD score needs n_ref > 2");
    if (const int rc = r2_rows_check(ctx, bed_len, n_ref, pos, n_rows)) return rc;
    if (gpu_ms) *gpu_ms = 0.0;
    if (n_rows == 0) return DBSLMM_OK;
    KEY_CHECK(ctx, bed, bed_len, n_ref);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PanelImage im;
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_ref, &im)) != hipSuccess) return hip_fail(ctx, "ld_scores panel image: ", e);
    // the missing-call flags of the listed rows, from the image's row table
    std::vector<int32_t> h_tab(static_cast<size_t>(im.n_rows) * 4);
    if ((e = hipMemcpyAsync(h_tab.data(), im.rows(), h_tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(ctx, "ld_scores row table: ", e);
    std::vector<uint8_t> miss(static_cast<size_t>(n_rows));
    for (int32_t k = 0; k < n_rows; ++k) miss[static_cast<size_t>(k)] = h_tab[4 * static_cast<size_t>(pos[k]) + 2] > 0;
    const LdscLayout L = build_ldsc_layout(n_rows, chr, bp, a.window_bp, miss.data());
    if (n_window) ldsc_window_counts(L, n_window);
    std::vector<int32_t> spos(static_cast<size_t>(n_rows)), schr(static_cast<size_t>(n_rows));
    std::vector<int64_t> sbp(static_cast<size_t>(n_rows));
    for (int32_t p = 0; p < n_rows; ++p) {
        const int32_t k = L.order[static_cast<size_t>(p)];
        spos[static_cast<size_t>(p)] = pos[k];
        schr[static_cast<size_t>(p)] = chr[k];
        sbp[static_cast<size_t>(p)] = bp[k];
    }
    const int32_t n_tiles = static_cast<int32_t>(L.tiles.size());
    constexpr int32_t kDefaultSlice = (256 << 20) / (kL2SlotWords * static_cast<int32_t>(sizeof(double)));   // 131072 tiles
    const int32_t slice = std::min(n_tiles, a.max_tiles_per_launch > 0 ? a.max_tiles_per_launch : kDefaultSlice);
    EventList ev{hipEventDefault};   // [0], [1]: around the call's kernels
    DevBufs B(ctx->device);
    int32_t *d_pos = nullptr, *d_chr = nullptr, *d_order = nullptr, *d_row_ptr = nullptr, *d_col_lo = nullptr;
    int64_t* d_bp = nullptr;
    L2Tile* d_tiles = nullptr;
    double *d_slots = nullptr, *d_run = nullptr, *d_out = nullptr;
    if ((e = B.upload(&d_pos, spos, st)) != hipSuccess || (e = B.upload(&d_chr, schr, st)) != hipSuccess ||
        (e = B.upload(&d_bp, sbp, st)) != hipSuccess || (e = B.upload(&d_order, L.order, st)) != hipSuccess ||
        (e = B.upload(&d_row_ptr, L.row_ptr, st)) != hipSuccess || (e = B.upload(&d_col_lo, L.col_lo, st)) != hipSuccess ||
        (e = B.upload(&d_tiles, L.tiles, st)) != hipSuccess ||
        (e = B.alloc(&d_slots, static_cast<size_t>(slice) * kL2SlotWords)) != hipSuccess ||
        (e = B.zeroed(&d_run, static_cast<size_t>(n_rows), st)) != hipSuccess ||
        (e = B.alloc(&d_out, static_cast<size_t>(n_rows))) != hipSuccess ||
        (e = ev.grow(2)) != hipSuccess || (e = hipEventRecord(ev[0], st)) != hipSuccess)
        return hip_fail(ctx, "ld_scores alloc/upload: ", e);
    const int64_t kpad = im.pitch * 4;
    for (int32_t t0 = 0; t0 < n_tiles; t0 += slice) {
        const int32_t t1 = std::min(n_tiles, t0 + slice);
        hipLaunchKernelGGL(dbslmm_l2_tiles, dim3(static_cast<unsigned>(t1 - t0)), dim3(256), gram::kLdsBytes, st,
                           im.mem.get(), kpad, im.rows(), im.n_rows, n_ref, d_pos, n_rows, d_tiles + t0, t1 - t0, d_chr,
                           d_bp, a.window_bp, a.unbiased, d_slots);
        hipLaunchKernelGGL(dbslmm_l2_reduce, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, st, d_slots,
                           t0, t1, d_row_ptr, d_col_lo, n_rows, d_run, t1 == n_tiles ? 1 : 0, im.rows(), d_pos, n_ref,
                           d_order, d_out);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, "ld_scores launch: ", e);
    }
    float ms = 0.0f;
    if ((e = hipEventRecord(ev[1], st)) != hipSuccess ||
        (e = hipMemcpyAsync(l2, d_out, static_cast<size_t>(n_rows) * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess || (e = hipEventElapsedTime(&ms, ev[0], ev[1])) != hipSuccess)
        return hip_fail(ctx, "ld_scores run: ", e);
    if (gpu_ms) *gpu_ms = ms;
    return DBSLMM_OK;
}

// LD score regression (ldsc_fit.hpp): host only.
int dbslmm_ldsc_fit(int64_t n, const double* chi2, const double* n_obs, const double* l2, double m,
                    const dbslmm_ldsc_args* args, dbslmm_ldsc_result* out) {
    const dbslmm_ldsc_args a = args ? *args : dbslmm_ldsc_args{1.0, 0.0, 0, 0};
    if (!out || n < 0 || (n > 0 && (!chi2 || !n_obs || !l2)) || !(m > 0.0) || a.n_blocks < 0 || a.n_blocks == 1 ||
        !(a.chisq_max >= 0.0))
        return DBSLMM_E_ARG;
    const ldsc::Result r = ldsc::fit(n, chi2, n_obs, l2, m, a.fixed_intercept != 0, a.intercept,
                                     a.n_blocks > 0 ? a.n_blocks : 200, a.chisq_max);
    *out = dbslmm_ldsc_result{r.h2, r.h2_se, r.intercept, r.intercept_se, r.mean_chi2, r.n_used, r.status};
    return DBSLMM_OK;
}

// Association scan (assoc.hip): the design on the host (assoc_layout.hpp), then the counts, one
// product launch per group of 16 columns of V, and the finish.
int dbslmm_assoc(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_total, int32_t n_rows,
                 const int32_t* rows, const dbslmm_assoc_args* args, int32_t* n_mis, int32_t* n_obs, double* af,
                 double* beta, double* se, double* tstat, double* p, int32_t* status, double* prod_d,
                 double* prod_m, double* gpu_ms) {
    if (!ctx) return DBSLMM_E_ARG;
    ON_FIRST_DEVICE(ctx, dbslmm_assoc(ctx0_, bed, bed_len, n_total, n_rows, rows, args, n_mis, n_obs, af, beta, se,
                                      tstat, p, status, prod_d, prod_m, gpu_ms));
    if (const int rc = ctx_ready(ctx)) return rc;
    ARG_CHECK(ctx, bed && args && n_total >= 1 && n_rows >= 0, "bad arguments");
    ARG_CHECK(ctx, n_rows == 0 || (n_mis && n_obs && af && beta && se && tstat && p && status), "null outputs");
    ARG_CHECK(ctx, (prod_d == nullptr) == (prod_m == nullptr), "prod_d and prod_m: both or neither");
    ARG_CHECK(ctx, args->chunk_indiv >= 0 && args->chunk_indiv % kAssocStage == 0,
              "chunk_indiv must be a multiple of 64 (0: the default)");
    if (rows) {
        if (const int rc = rows_in_bed(ctx, bed_len, n_total, rows, n_rows)) return rc;
    } else {
        ARG_CHECK(ctx, bed_len >= 3 + n_rows * bed_row_bytes(n_total), "bed image shorter than n_rows rows");
    }
    const int64_t n_pad = round_up(n_total, gram::kKpadAlign);     // the individuals of an image row
    assoc::Design D;
    if (!assoc::build_design(n_total, n_pad, args->keep, args->pheno, args->n_pheno, args->covar, args->n_covar, D)) {
        ctx->err = "assoc: " + D.err;
        return DBSLMM_E_ARG;
    }
    if (gpu_ms) *gpu_ms = 0.0;
    if (n_rows == 0) return DBSLMM_OK;
    const int32_t n_stages = static_cast<int32_t>(n_pad / kAssocStage);
    const int32_t spc = (args->chunk_indiv > 0 ? args->chunk_indiv : kAssocChunkIndiv) / kAssocStage;
    const int32_t n_chunks = (n_stages + spc - 1) / spc;
    ARG_CHECK(ctx, n_chunks <= 65535, "chunk_indiv too small for this panel (more than 65535 chunks)");
    const int32_t n_tiles = (n_rows + kAssocRows - 1) / kAssocRows;
    KEY_CHECK(ctx, bed, bed_len, n_total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PanelImage im;
    hipError_t e;
    if ((e = panel_image(ctx, bed, bed_len, n_total, &im)) != hipSuccess) return hip_fail(ctx, "assoc panel image: ", e);
    // the image row of every tile row: the zero-dosage row past the list
    std::vector<int32_t> rows16(static_cast<size_t>(n_tiles) * kAssocRows, im.n_rows);
    for (int32_t j = 0; j < n_rows; ++j) rows16[static_cast<size_t>(j)] = rows ? rows[j] : j;
    const int32_t P = D.P, c1 = D.c1, n_cols = D.n_cols;
    const size_t n_part = static_cast<size_t>(D.n_groups) * n_chunks * n_tiles * assoc::kTileWords;
    const size_t n_prod = static_cast<size_t>(n_rows) * n_cols, n_stat = static_cast<size_t>(n_rows) * P;
    EventList ev{hipEventDefault};   // [0], [1]: around the call's kernels
    DevBufs B(ctx->device);
    int32_t *d_rows = nullptr, *d_int = nullptr;   // d_int: n_mis | n_obs | status
    uint32_t* d_mask = nullptr;
    v4i* d_counts = nullptr;
    double *d_V = nullptr, *d_yy = nullptr, *d_part = nullptr, *d_prod = nullptr, *d_out = nullptr;   // d_out: af | beta | se | T | p
    if ((e = B.upload(&d_rows, rows16, st)) != hipSuccess || (e = B.upload(&d_mask, D.mask, st)) != hipSuccess ||
        (e = B.upload(&d_V, D.V, st)) != hipSuccess || (e = B.upload(&d_yy, D.yy, st)) != hipSuccess ||
        (e = B.alloc(&d_counts, static_cast<size_t>(n_rows))) != hipSuccess ||
        (e = B.alloc(&d_part, 2 * n_part)) != hipSuccess || (e = B.alloc(&d_prod, 2 * n_prod)) != hipSuccess ||
        (e = B.alloc(&d_int, 3 * static_cast<size_t>(n_rows))) != hipSuccess ||
        (e = B.alloc(&d_out, static_cast<size_t>(n_rows) + 4 * n_stat)) != hipSuccess ||
        (e = ev.grow(2)) != hipSuccess || (e = hipEventRecord(ev[0], st)) != hipSuccess)
        return hip_fail(ctx, "assoc alloc/upload: ", e);
    hipLaunchKernelGGL(dbslmm_assoc_counts, dim3(static_cast<unsigned>((n_rows + 3) / 4)), dim3(256), 0, st,
                       im.mem.get(), im.pitch, d_rows, n_rows, d_mask, d_counts);
    const size_t group_part = n_part / D.n_groups;
    for (int32_t g = 0; g < D.n_groups; ++g)
        hipLaunchKernelGGL(dbslmm_assoc_tiles, dim3(static_cast<unsigned>((n_tiles + assoc::kTileWaves - 1) / assoc::kTileWaves), n_chunks),
                           dim3(256), 0, st, im.mem.get(), im.pitch, d_rows, n_tiles,
                           d_V + static_cast<size_t>(g) * n_pad * kAssocCols, n_stages, spc, d_part + g * group_part,
                           d_part + n_part + g * group_part);
    double* d_af = d_out;
    double *d_beta = d_af + n_rows, *d_se = d_beta + n_stat, *d_t = d_se + n_stat, *d_p = d_t + n_stat;
    hipLaunchKernelGGL(dbslmm_assoc_finish, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, st, d_part,
                       d_part + n_part, D.n_groups, n_chunks, n_tiles, n_rows, c1, P, D.n, d_counts, d_yy, d_prod,
                       d_prod + n_prod, d_int, d_int + n_rows, d_af, d_beta, d_se, d_t, d_p, d_int + 2 * static_cast<size_t>(n_rows));
    float ms = 0.0f;
    const size_t ni = static_cast<size_t>(n_rows) * sizeof(int32_t), nd = static_cast<size_t>(n_rows) * sizeof(double);
    auto down = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[1], st)) != hipSuccess ||
        (e = down(n_mis, d_int, ni)) != hipSuccess || (e = down(n_obs, d_int + n_rows, ni)) != hipSuccess ||
        (e = down(status, d_int + 2 * static_cast<size_t>(n_rows), ni)) != hipSuccess || (e = down(af, d_af, nd)) != hipSuccess ||
        (e = down(beta, d_beta, nd * P)) != hipSuccess || (e = down(se, d_se, nd * P)) != hipSuccess ||
        (e = down(tstat, d_t, nd * P)) != hipSuccess || (e = down(p, d_p, nd * P)) != hipSuccess ||
        (prod_d && ((e = down(prod_d, d_prod, n_prod * sizeof(double))) != hipSuccess ||
                    (e = down(prod_m, d_prod + n_prod, n_prod * sizeof(double))) != hipSuccess)) ||
        (e = hipStreamSynchronize(st)) != hipSuccess || (e = hipEventElapsedTime(&ms, ev[0], ev[1])) != hipSuccess)
        return hip_fail(ctx, "assoc run: ", e);
    if (gpu_ms) *gpu_ms = ms;
    return DBSLMM_OK;
}

// The finish of the scan on caller-supplied counts and products (assoc_fit.hpp): host only.
int dbslmm_assoc_stat_host(int64_t n, int32_t n_covar, int32_t n_pheno, int32_t n_rows, const int32_t* n1,
                           const int32_t* n2, const int32_t* nm, const double* t, const double* yy,
                           int32_t* n_obs, double* af, double* beta, double* se, double* tstat, double* p,
                           int32_t* status) {
    if (n_pheno < 1 || n_covar < 0 || n_rows < 0 || n - n_covar - 2 < 1 || !yy) return DBSLMM_E_ARG;
    if (n_rows > 0 && !(n1 && n2 && nm && t && n_obs && af && beta && se && tstat && p && status)) return DBSLMM_E_ARG;
    const int64_t n_cols = static_cast<int64_t>(n_covar) + n_pheno;
    for (int32_t j = 0; j < n_rows; ++j)
        status[j] = assoc::finish_row(n, n_covar, n_pheno, n1[j], n2[j], nm[j], t + j * n_cols, nullptr, yy, n_obs + j,
                                      af + j, beta + j, se + j, tstat + j, p + j, n_rows);
    return DBSLMM_OK;
}

int dbslmm_student_t_two_sided(double t, double df, double* p_out) {
    if (!p_out) return DBSLMM_E_ARG;
    *p_out = assoc::student_t_two_sided(t, df);
    return DBSLMM_OK;
}

// route_factor.hip -- the factorisation route of a run (included by plan.hip): the tiled Cholesky
// sequences and their graphs, the persistent substitutions, the h2f copies iterated on one factor
// (Chebyshev / CG), and run_factor, which enqueues a whole run of it.

// The stream pair and event set of a tiled sequence: the lead / only sequence runs on stream2
// (chain, high priority) + stream3 (bulk trailing), the rest sequence on stream4 + stream5.
struct TSeq {
    hipStream_t chain, bulk;
    EventList* tev;
};
static TSeq seq_main(dbslmm_plan* p) { return TSeq{p->ctx->stream2, p->ctx->stream3, &p->fac.tev}; }
static TSeq seq_rest(dbslmm_plan* p) { return TSeq{p->ctx->stream4, p->ctx->stream5, &p->fac.tev_rest}; }

// dbslmm_options.debug_delay_us (tests): a spin kernel at the head of a stream segment.  side > 0:
// the concurrent side (bulk trailing launches, the rest sequence, the main stream after the lead
// fork) runs late; side < 0: the critical side (chain launches, the lead sequence).
static void debug_spin(const dbslmm_plan* p, hipStream_t st, int side) {
    const int32_t d = p->opt.debug_delay_us;
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
    const CopyView v = copy_view(p, copy);
    const chol::TiledArgs ta{v.M, p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff, p->d_blk_id, p->d_z,
                             p->d_slot_out, p->d_rsd, v.dshift, isn, v.y, v.beta_s, v.beta_l, v.status,
                             p->n_nonempty, p->M_elems, p->n_slots, p->n_s, p->n_l, p->nbk};
    int nev = 0;
    for (const TLaunch& L : tl)
        if (L.kind == kTlRecord) nev = std::max(nev, L.step + 1);
    EventList& tev = *sq.tev;
    HIP_TRY(ctx, tev.grow(nev));
    for (const TLaunch& L : tl) {
        hipStream_t st = L.strm ? sq.bulk : sq.chain;
        if (L.kind == kTlRecord) { HIP_TRY(ctx, hipEventRecord(tev[L.step], st)); continue; }
        if (L.kind == kTlWait) { HIP_TRY(ctx, hipStreamWaitEvent(st, tev[L.step], 0)); continue; }
        if (L.items == 0) continue;
        const int32_t* act = d_tlist + L.off;
        const dim3 g(static_cast<unsigned>(L.items)), blk(chol::kLargeThreads);
        if (p->opt.debug_delay_us) debug_spin(p, st, L.strm ? 1 : -1);
        switch (L.kind) {
        case 4: hipLaunchKernelGGL(dbslmm_tchol_region, g, blk, kRegionLds, st, ta, act, L.items); break;
        case 1: hipLaunchKernelGGL(dbslmm_tchol_panel, g, blk, kTiledLds, st, ta, act, L.items); break;
        default: hipLaunchKernelGGL(dbslmm_tchol_trailing3k16, g, dim3(512), kTrail3Lds, st, ta, L.n, act, L.items); break;
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return DBSLMM_OK;
}

template <int NR>
static void launch_trsv(bool fwd, int grid, hipStream_t st, const trsv::Args& a) {
    if (fwd) hipLaunchKernelGGL(dbslmm_trsv_fwd<NR>, dim3(grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
    else hipLaunchKernelGGL(dbslmm_trsv_bwd<NR>, dim3(grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
}

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
    return TGroup{0, p->n_titems, 0, p->n_tiled, p->ctx->stream2, p->fac.d_tflags + p->n_tflags,
                  std::max(1, std::min(p->ctx->n_cu, p->n_titems))};
}
// split substitutions: the lead group on stream2 (ticket counter after the flags), the rest group
// on the rest sequence's stream (its own counter: the spare word after the error word)
static TGroup tgroup_lead(const dbslmm_plan* p) {
    return TGroup{0, p->n_titems_lead, 0, p->n_tb_lead, p->ctx->stream2, p->fac.d_tflags + p->n_tflags,
                  std::max(1, std::min(p->sub_grid_lead, p->n_titems_lead))};
}
static TGroup tgroup_rest(const dbslmm_plan* p) {
    const int32_t ni = p->n_titems - p->n_titems_lead;
    return TGroup{p->n_titems_lead, ni, p->n_tb_lead, p->n_tiled - p->n_tb_lead, p->ctx->stream4,
                  p->fac.d_tflags + p->n_tflags + 2, std::max(1, std::min(p->sub_grid_rest, ni))};
}
// The substitution epochs of one run (tile-flag values, trsv.hip): run_impl resets the flags ahead
// of the fork whenever the counter is within kEpochsPerRun of wrapping, so inside a run the counter
// only grows.  Bound: 64 copies' backward solves + 2 groups x 32 copy groups x 2 x 60 passes.
static int next_epoch(dbslmm_plan* p, int k) {
    if (p->fac.trsv_epoch > INT32_MAX - k) {   // unreachable unless a run exceeds kEpochsPerRun
        p->ctx->err = "substitution epoch counter overflow within one run";
        return DBSLMM_E_STATE;
    }
    p->fac.trsv_epoch += k;
    return DBSLMM_OK;
}

// the substitutions' vectors [Y, Z, X, R, D, S] x kMaxR x n_slots, allocated on first use
static int ensure_vectors(dbslmm_plan* p) {
    if (p->fac.d_cheb) return DBSLMM_OK;
    std::lock_guard<std::mutex> lk(g_capture_mu);
    HIP_TRY(p->ctx, p->bufs.alloc(&p->fac.d_cheb, 6 * trsv::kMaxR * std::max<int64_t>(1, p->n_slots)));
    return DBSLMM_OK;
}
// What every substitution launch of group grp on the factor of copy view f shares.
static trsv::Args trsv_args(const dbslmm_plan* p, const TGroup& grp, const CopyView& f, double isn) {
    trsv::Args a{};
    set_plan_args(a, p, isn);
    a.M = f.M;
    a.status = f.status;
    a.grid = grp.grid;
    a.foff = p->fac.d_foff;
    a.flags = p->fac.d_tflags;
    a.ctr = grp.ctr;
    a.err = p->fac.d_tflags + p->n_tflags + 1;
    a.vs = std::max<int64_t>(1, p->n_slots);
    return a;
}

// Backward substitution of factorisation copy `copy`'s tiled blocks in one persistent launch
// (trsv.hip, plain mode): y = the bordered z row, x -> y scratch of the copy, beta of the copy.
static int run_pbwd(dbslmm_plan* p, double isn, int copy, const TGroup& grp) {
    dbslmm_ctx* ctx = p->ctx;
    hipStream_t st = grp.st;
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    if (const int rc = ensure_vectors(p)) return rc;
    const CopyView v = copy_view(p, copy);
    trsv::Args a = trsv_args(p, grp, v, isn);
    a.items = p->fac.d_tri_b + 2 * grp.item_off;
    a.n_items = grp.n_items;
    a.dst = p->fac.d_cheb + trsv::kMaxR * vs;          // the Z hand-off buffer
    a.X = v.y;
    a.cix[0] = copy;
    a.mode = 1;
    if (const int rc = next_epoch(p, 1)) return rc;
    a.epoch = p->fac.trsv_epoch;
    if (a.n_items > 0) {
        launch_trsv<1>(false, a.grid, st, a);
        p->fac.trsv_pending = true;
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
    return launch_graph(p, isn, p->tl, p->fac.d_tlist, copy, p->fac.graph_copy.at(copy), seq_main(p));
}
static int run_rest_copy(dbslmm_plan* p, double isn, int copy) {
    return launch_graph(p, isn, p->tl_rest, p->fac.d_tlist, copy, p->fac.graph_rest.at(copy), seq_rest(p));
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
    if (p->opt.h2f_mode != 0 || n < 2 || (p->n_tiled == 0 && p->n_large == 0) || !(p->tau > 0.0 && p->tau <= 1.0))
        return false;
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return sigmas[a] < sigmas[b]; });
    cp.base = idx[n / 2];
    const double nobs = static_cast<double>(p->n_obs);
    const double db = 1.0 / (sigmas[cp.base] * nobs);
    cp.db = db;
    const double floor_ = db + 1.0 - p->tau;
    const double tol = p->fac.h2f_tol;
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
        const bool capped = p->opt.h2f_cg && !p->opt.cheb_fused && p->opt.pcg_maxit < K;
        if (capped) K = p->opt.pcg_maxit;
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

// Chebyshev coefficients and iteration vectors: uploaded / allocated on stream st before any
// group's iterations (run_impl: on the main stream ahead of the fork)
static int cheb_prepare(dbslmm_plan* p, const ChebPlan& cp, hipStream_t st) {
    dbslmm_ctx* ctx = p->ctx;
    if (const int rc = ensure_vectors(p)) return rc;
    if (p->opt.h2f_cg && !p->fac.d_cgconv) {
        std::lock_guard<std::mutex> lk(g_capture_mu);
        const size_t nb = std::max(1, p->n_nonempty);
        HIP_TRY(ctx, p->bufs.alloc(&p->fac.d_cgrec, nb * trsv::kMaxR * 2));
        HIP_TRY(ctx, p->bufs.alloc(&p->fac.d_cgconv, nb));
        HIP_TRY(ctx, p->bufs.alloc(&p->fac.d_cgit, nb));
    }
    // every block's CG pass count starts at 0 each run (the rest group of sub_split = 2 iterates by
    // Chebyshev and never writes it; workload[16] sums it over every tiled block: ADVICE r05)
    if (p->fac.d_cgit) HIP_TRY(ctx, hipMemsetAsync(p->fac.d_cgit, 0, std::max(1, p->n_nonempty) * sizeof(int32_t), st));
    // the coefficients depend only on the sigmas: uploaded when they change, synchronously (the
    // host vector is a temporary of the run; an asynchronous copy from pageable memory may still
    // be pending when it is freed) after every earlier run that reads d_coef has finished
    if (cp.coef == p->fac.h_coef) return DBSLMM_OK;
    std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous copy below
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
    if (p->fac.coef_cap < static_cast<int32_t>(cp.coef.size())) {
        (void)p->bufs.release(p->fac.d_coef);
        HIP_TRY(ctx, p->bufs.alloc(&p->fac.d_coef, cp.coef.size()));
        p->fac.coef_cap = static_cast<int32_t>(cp.coef.size());
    }
    HIP_TRY(ctx, hipMemcpyAsync(p->fac.d_coef, cp.coef.data(), cp.coef.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    p->fac.h_coef = cp.coef;
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
    const bool fused = p->opt.cheb_fused && grp.item_off == 0 && grp.n_items == p->n_titems;
    const bool cg = p->opt.h2f_cg && !fused;   // (the fused launch iterates by Chebyshev)
    const int64_t vs = std::max<int64_t>(1, p->n_slots);
    const int64_t blk = trsv::kMaxR * vs;
    double *Y = p->fac.d_cheb, *Z = Y + blk, *X = Z + blk, *R = X + blk, *D = R + blk, *S = D + blk;
    const CopyView base = copy_view(p, cp.base);
    for (size_t g = 0; g < cp.iters.size(); ++g) {
        const size_t g0 = g * trsv::kMaxR;
        const int nr = static_cast<int>(std::min<size_t>(trsv::kMaxR, cp.others.size() - g0));
        const int K = cp.iters[g];
        int cix[trsv::kMaxR] = {0, 0};
        for (int j = 0; j < nr; ++j) cix[j] = cp.others[g0 + j];
        const double* coef = p->fac.d_coef + cp.coef_off[g];
        if (fused && p->fac.cheb_items_K != K) {   // the work list of K iterations (cached: K depends on the sigmas)
            std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous upload below
            std::vector<int32_t> items;
            build_cheb_items(p, K, items);
            HIP_TRY(ctx, hipStreamSynchronize(st));
            (void)p->bufs.release(p->fac.d_cheb_items);
            HIP_TRY(ctx, p->bufs.upload(&p->fac.d_cheb_items, items, ctx->stream));
            p->fac.n_cheb_items = static_cast<int32_t>(items.size() / 2);
            p->fac.cheb_items_K = K;
        }
        hipLaunchKernelGGL(dbslmm_cheb_init, dim3(grp.n_tb), dim3(256), 0, st, p->fac.d_tb + grp.tb_off, p->d_row0, p->d_m,
                           p->d_ms, p->d_blk_id, base.y, coef, nr, vs, X, R, D, S, base.status, p->d_status, p->nbk,
                           cix[0], cix[1], cg ? p->fac.d_cgconv : nullptr, cg && g == 0 ? p->fac.d_cgit : nullptr);
        HIP_TRY(ctx, hipGetLastError());
        trsv::Args a = trsv_args(p, grp, base, isn);
        a.epi = p->fac.d_tepi;
        a.X = X;
        a.R = R;
        a.D = D;
        a.S = S;
        a.Y = Y;
        a.Z = Z;
        a.coef = coef;
        a.iters = K;
        for (int j = 0; j < trsv::kMaxR; ++j) a.cix[j] = cix[j];
#ifdef DBSLMM_DIAG   // diagnostic build: per-tile stamps of the largest tiled block
        if (getenv("DBSLMM_TRSV_STAMPS")) {
            int bmax = p->h_tb[0];
            for (int32_t b : p->h_tb) if (p->h_m[b] > p->h_m[bmax]) bmax = b;
            if (!p->fac.d_stamps) HIP_TRY(ctx, p->bufs.alloc(&p->fac.d_stamps, 8 * 4096));
            a.stamps = p->fac.d_stamps;
            a.stamp_b = bmax;
        }
#endif
        if (!fused) {   // one launch per pass (the launch boundary orders the passes)
            a.n_items = grp.n_items;
            trsv::CGArgs ca{};
            if (cg) {   // K (the a priori Chebyshev count) caps the iterations
                a.mode = 2;
                a.conv = p->fac.d_cgconv;
                set_plan_args(ca, p, isn);
                ca.tb = p->fac.d_tb + grp.tb_off;
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
                ca.tol = p->fac.h2f_tol;
                ca.capped = cp.capped[g];
                ca.rec = p->fac.d_cgrec;
                ca.conv = p->fac.d_cgconv;
                ca.iters = p->fac.d_cgit;
                ca.status = p->d_status;
                ca.st_stride = p->nbk;
            }
            for (int k = 0; k < K; ++k) {
                for (int pass = 0; pass < 2; ++pass) {
                    const bool fwd = pass == 0;
                    if (const int rc = next_epoch(p, 1)) return rc;
                    a.epoch = p->fac.trsv_epoch;
                    a.items = (fwd ? p->fac.d_tri_f : p->fac.d_tri_b) + 2 * grp.item_off;
                    a.src = fwd ? R : Y;
                    a.dst = fwd ? Y : Z;
                    a.coef = coef + static_cast<int64_t>(k) * nr * 3;
                    a.last = k == K - 1;
                    if (nr == 1) launch_trsv<1>(fwd, a.grid, st, a);
                    else launch_trsv<2>(fwd, a.grid, st, a);
                    HIP_TRY(ctx, hipGetLastError());
                    p->fac.trsv_pending = true;
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
        a.items = p->fac.d_cheb_items;
        a.n_items = p->fac.n_cheb_items;
        a.grid = std::max(1, std::min(ctx->n_cu, p->fac.n_cheb_items));
        // passes 0 .. 2K-1 run at epochs epoch .. epoch + 2K - 1 (flags and update flags only grow)
        a.epoch = p->fac.trsv_epoch + 1;
        if (const int rc = next_epoch(p, 2 * K)) return rc;
        if (nr == 1) hipLaunchKernelGGL(dbslmm_trsv_cheb<1>, dim3(a.grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
        else hipLaunchKernelGGL(dbslmm_trsv_cheb<2>, dim3(a.grid), dim3(trsv::kThreads), trsv::kLdsBytes, st, a);
        HIP_TRY(ctx, hipGetLastError());
        p->fac.trsv_pending = true;
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
    double *X = p->fac.d_cheb + 2 * blk, *R = X + blk, *D = R + blk, *S = D + blk;
    const CopyView base = copy_view(p, cp.base);
    for (size_t g = 0; g < cp.iters.size(); ++g) {
        const size_t g0 = g * trsv::kMaxR;
        const int nr = static_cast<int>(std::min<size_t>(trsv::kMaxR, cp.others.size() - g0));
        TChebArgs a{};
        set_plan_args(a, p, isn);
        a.M = base.M;
        a.blocks = p->fac.d_tcheb_blocks;
        a.n_blocks = p->n_tcheb;
        a.iters = cp.iters[g];
        a.vld = p->tcheb_vld;
        a.vs = vs;
        a.x_base = base.y;
        a.X = X;
        a.R = R;
        a.D = D;
        a.S = S;
        a.coef = p->fac.d_coef + cp.coef_off[g];
        for (int j = 0; j < trsv::kMaxR; ++j) a.cix[j] = j < nr ? cp.others[g0 + j] : cp.others[g0];
        a.st_base = base.status;
        a.status = p->d_status;
        a.st_stride = p->nbk;
        const size_t lds = (static_cast<size_t>(nr) * a.vld + trsv::kT * nr) * sizeof(double);
        if (nr == 1) hipLaunchKernelGGL(dbslmm_tcheb<1>, dim3(p->n_tcheb), dim3(trsv::kBThreads), lds, st, a);
        else hipLaunchKernelGGL(dbslmm_tcheb<2>, dim3(p->n_tcheb), dim3(trsv::kBThreads), lds, st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    return DBSLMM_OK;
}

// One run on the factorisation route: statistics + Gram, then n factorisations + solves of it, copy c
// with sigma_s = sigmas[c] (n > 1: h2f tuning; copies 1.. are device copies of the Gram, all factored
// by one merged tiled sequence).
static int run_factor(dbslmm_plan* p, const double* sigmas, int n) {
    dbslmm_ctx* ctx = p->ctx;
    if (const int rc = ensure_copies(p, n, n)) return rc;
    if (n > 1 && p->fac.multi_n != n) {   // the merged sequence of n copies
        std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous upload below
        std::vector<int32_t> tlist;
        p->fac.tl_multi.clear();
        build_tiled(p->h_m, p->h_tb, n, p->n_nonempty, p->fac.tl_multi, tlist);
        (void)p->bufs.release(p->fac.d_tlist_multi);
        HIP_TRY(ctx, p->bufs.upload(&p->fac.d_tlist_multi, tlist, ctx->stream));
        p->fac.graph_multi.reset();
        p->fac.multi_n = n;
    }
    // h2f: the tiled blocks are factored once (copy cp.base) and the other copies iterate on it
    p->fac.trsv_failed = false;
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
    const size_t nbk = static_cast<size_t>(p->nbk);
    // Substitution tile flags are epochs (trsv.hip): a run takes at most kEpochsPerRun of them
    // (backward solves and Chebyshev passes of every group and copy).  When the counter could wrap
    // during this run, the flags restart from a clean slate HERE, on the main stream: every stream
    // of the run forks from it after this point and every stream of the previous run has joined
    // it, so no substitution launch of either group can still be running (a reset inside a group
    // would race the other group's launch on its own stream).
    if (p->n_tflags > 0 && p->fac.trsv_epoch > INT32_MAX - kEpochsPerRun) {
        HIP_TRY(ctx, hipMemsetAsync(p->fac.d_tflags, 0, p->n_tflags * sizeof(int32_t), s));
        HIP_TRY(ctx, hipMemsetAsync(p->fac.d_tepi, 0, p->n_tflags * sizeof(int32_t), s));
        p->fac.trsv_epoch = 0;
    }
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
    const std::vector<TLaunch>& tl = n > 1 && !cheb ? p->fac.tl_multi : p->tl;
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
    if (p->opt.debug_stop == 1) {   // tests: the block matrices hold Sigma (dbslmm_plan_block_matrix)
        if (const int rc = record_instants(ctx, ev, kEvAfterGram, s)) return rc;
        LastRun r = p->last;   // no results: what the previous run left for the variance and the scores stays
                               // (sigma_run, var_copy, score_*, cheb_*, cg_ran), and n_runs does not count it
        r.ran = true;
        r.stopped = true;      // download / variance refuse: the betas of this run were never computed
        r.pcg_ran = false;
        r.pcg_pending_var = false;
        close_run(p, r);
        return DBSLMM_OK;
    }
    if (p->n_nonempty > 0) {
        // fork: the tiled sequence (or, with a lead group, the rest sequence on stream4) runs
        // beside the single-workgroup and single-wave kernels of the main stream
        if (!early) {
            HIP_TRY(ctx, hipEventRecord(ctx->fork2, s));
            HIP_TRY(ctx, hipStreamWaitEvent(lead ? ctx->stream4 : ctx->stream2, ctx->fork2, 0));
        }
        if (p->n_large > 0) {
            // every copy in one launch; h2f by iteration: the base copy alone is factored, and the
            // others iterate on its factor (below)
            const int nc = large_cheb ? 1 : n;
            const CopyView b = copy_view(p, large_cheb ? cp.base : 0);
            hipLaunchKernelGGL(dbslmm_chol_large, dim3(p->n_large * nc), dim3(chol::kLargeThreads), kCholLargeLds, s,
                               b.M, p->d_order, p->n_large, p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff,
                               p->d_blk_id, p->d_z, p->d_slot_out, p->d_rsd, b.dshift, isn, b.y, b.beta_s,
                               b.beta_l, b.status, nc, p->M_elems, static_cast<int64_t>(p->n_slots), p->n_s,
                               p->n_l, p->nbk);
            HIP_TRY(ctx, hipGetLastError());
            for (size_t g = 0; large_cheb && g < cp.iters.size(); ++g) {
                const size_t g0 = g * chol::kChebR;
                const int nr = static_cast<int>(std::min<size_t>(chol::kChebR, cp.others.size() - g0));
                chol::CgStop cgs{};   // h2f by CG (the default): stopping bounds per copy
                cgs.on = p->opt.h2f_cg ? 1 : 0;
                for (int j = 0; j < nr; ++j) cgs.fs[j] = cp.db + cp.coef[cp.coef_off[g] + 3 * j + 2] + 1.0 - p->tau;
                cgs.fl = 1.0 - p->tau;
                cgs.tol = p->fac.h2f_tol;
                cgs.capped = cp.capped[g];
                hipLaunchKernelGGL(dbslmm_chol_cheb, dim3(p->n_large), dim3(chol::kChebThreads), kCholChebLds, s,
                                   b.M, p->d_order, p->n_large, p->d_row0, p->d_m, p->d_ms, p->d_ld, p->d_matoff,
                                   p->d_blk_id, p->d_slot_out, b.y, p->fac.d_coef + cp.coef_off[g], nr,
                                   cp.iters[g], isn, p->d_beta_s, p->d_beta_l, p->n_s, p->n_l, b.status, p->d_status,
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
            const CopyView v = copy_view(p, c);
            hipLaunchKernelGGL(dbslmm_chol_small, dim3(g), dim3(chol::kSmallWaves * chol::kWave), 0, ss, v.M,
                               p->d_order + p->n_large, p->n_small, p->d_row0, p->d_m, p->d_ms, p->d_ld,
                               p->d_matoff, p->d_blk_id, p->d_z, p->d_slot_out, p->d_rsd, v.dshift, isn, v.beta_s,
                               v.beta_l, v.status);
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
                int rc = launch_graph(p, isn, tl, p->fac.d_tlist_multi, 0, p->fac.graph_multi.at(0), seq_main(p));
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
    p->n_runs++;
    const int iters = std::accumulate(cp.iters.begin(), cp.iters.end(), 0);
    LastRun r;
    r.ran = true;
    r.stopped = false;
    r.sigma_run = sigmas[n - 1];
    r.var_copy = n - 1;
    // the variance's re-solve (force_factor) overwrites copy 0 of the device results: the user run's
    // copies stay on record, stale
    r.score_copies = p->force_factor ? p->last.score_copies : n;
    r.score_stale = p->force_factor;
    r.pcg_ran = false;
    r.pcg_pending_var = false;
    r.cheb_base = cheb ? cp.base : -1;
    r.cheb_pending_var = cheb && cp.base != n - 1;   // no factor of the last copy's tiled blocks
    r.cg_ran = cheb && p->opt.h2f_cg && !p->opt.cheb_fused;
    r.cheb_iters = cheb ? iters : 0;
    r.cheb_bytes = cheb ? 2.0 * iters * p->wl[13] : 0.0;   // (CG: counted from d_cgit on query)
    close_run(p, r);
    return DBSLMM_OK;
}

// After the main stream has drained: the error word of the persistent substitutions (trsv.hip:
// a bounded hand-off wait that gave up means the tiled blocks' betas of that run are invalid).
// Read and cleared after every run that launched one; the failure stays reported until the next run.
static int check_trsv(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    if (p->fac.trsv_pending) {
        std::lock_guard<std::mutex> lk(g_capture_mu);   // synchronous copy / memset below
        int32_t werr = 0;
        HIP_TRY(ctx, hipMemcpy(&werr, p->fac.d_tflags + p->n_tflags + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (werr) {
            HIP_TRY(ctx, hipMemsetAsync(p->fac.d_tflags + p->n_tflags + 1, 0, sizeof(int32_t), ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        p->fac.trsv_pending = false;
        p->fac.trsv_failed = p->fac.trsv_failed || werr != 0;
    }
    if (p->fac.trsv_failed) {
        ctx->err = "substitution hand-off wait gave up (trsv): the tiled blocks' betas of this run are invalid";
        return DBSLMM_E_HIP;
    }
    return DBSLMM_OK;
}

// route_pcg.hip -- the PCG route of a run (included by plan.hip): its layout, the chunked iterations
// and their continuation, and the results streamed to the host while the run iterates.

// ---------------------------------------------------------------- PCG route (pcg.hip)
// Does this run take the PCG route?  solver 2 forces it and 0 (auto) picks it when every copy's
// prior shift d_c = 1/(sigma_c n) keeps the system well conditioned (d_c >= kPcgDmin: kappa <=
// 1 + lambda_LD / (d + 1 - tau) ~ 6 at lambda_LD ~ 10, tools/cg_gate.py); both need a data-free
// lower bound on lambda_min (tau < 1, or no large SNPs: then d_c + 1 - tau), at most
// pcg::kMaxNC copies and no debug stop after the Gram.
constexpr double kPcgDmin = 2.0;
// ... every condition but the number of copies
static bool pcg_eligible(const dbslmm_plan* p, const double* sigmas, int n) {
    if (p->force_factor || p->opt.solver == 1 || p->n_nonempty == 0 || p->opt.debug_stop) return false;
    if (!(p->tau > 0.0 && p->tau <= 1.0) || (p->tau >= 1.0 && p->has_large)) return false;
    if (p->opt.solver == 2) return true;
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
    if (p->pcg.g16 && !p->pcg.d_G16) {
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
        HIP_TRY(ctx, p->bufs.zeroed(&p->pcg.d_G16, e, ctx->stream));
        HIP_TRY(ctx, p->bufs.upload(&p->pcg.d_off16, off, ctx->stream));
        HIP_TRY(ctx, p->bufs.upload(&p->pcg.d_ld16, ldv, ctx->stream));
        p->pcg.h_off16 = off;
    }
    HIP_TRY(ctx, p->pcg.mon.reserve((1 + std::max(1, p->n_nonempty)) * sizeof(int32_t)));
    if (p->pcg.n == n) return DBSLMM_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the old layout's buffers go, each member null from here on: a failure below leaves nothing dangling
    // (d_pflist is uploaded again only when some block is solved whole)
    DevBufs& B = p->bufs;
    B.release_all(p->pcg.d_pblk, p->pcg.d_pitem, p->pcg.d_prow, p->pcg.d_pvec, p->pcg.d_ppart, p->pcg.d_pdot, p->pcg.d_pqs, p->pcg.d_pcnv,
                  p->pcg.d_pitb, p->pcg.d_pdone, p->pcg.d_pact, p->pcg.d_pflist, p->pcg.d_pfin);
    p->pcg.n = 0;                        // (no layout until the new one is complete)
    p->pcg.trim = false;                 // (until a run of this layout has read the flags)
    using namespace pcg;
    std::vector<PcgBlk> blk;
    std::vector<int2> flist;             // (block, copy) sequences solved whole by dbslmm_pcg_block
    std::vector<double> mat, part;
    std::vector<int4> items;
    std::vector<int2> rows;
    int64_t vo = 0, po = 0, dof = 0;
    int32_t sco = 0;
    const double esz = p->pcg.g16 ? 2.0 : 8.0;
    // tiles per product item: one (measured at config 4: 10.65 / 10.90 / 11.13 / 11.34 ms per step
    // at 1 / 2 / 4 / 8, and the N = 8 shards' product 114 -> ~45 us: many short items keep more
    // row segments in flight than a few long ones)
    int run = 1;
    p->pcg.run = run;
    for (int b = 0; b < p->n_nonempty; ++b) {
        const int32_t m = p->h_m[b], Tb = (m + kT - 1) / kT, nrun = (Tb + run - 1) / run;
        // a block without large SNPs solves n scalar shifts of one matrix: one Krylov sequence
        // (multi-shift CG, one product column); with large SNPs each copy iterates on its own
        const bool msh = n > 1 && p->h_ms[b] == m;
        const int32_t nc = msh ? 1 : n;
        const bool fused = p->opt.pcg_fused && Tb <= kFTb && !p->pcg.h_off16.empty();
        PcgBlk k{b, p->h_row0[b], m, p->h_ms[b], p->h_ld[b], Tb, Tb + nrun, sco, p->h_matoff[b], vo, po, dof,
                 p->pcg.h_off16.empty() ? 0 : p->pcg.h_off16[b], nc, msh ? 1 : 0, fused ? 1 : 0, 0};
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
    p->pcg.n_prow_chip = p->pcg.n_pitem_chip = 0;
    for (const int2& r : rows) p->pcg.n_prow_chip += blk[r.x].fused ? 0 : 1;
    for (const int4& e : items) p->pcg.n_pitem_chip += blk[e.x].fused ? 0 : 1;
    p->pcg.h_pfused.assign(blk.size(), 0);
    p->pcg.h_pnseq.assign(blk.size(), 0);
    for (const int2& f : flist) {
        p->pcg.h_pfused[f.x] = 1;
        p->pcg.h_pnseq[f.x] += 1;
    }
    p->pcg.n_pflist = static_cast<int32_t>(flist.size());
    // a streamed run's host scan: the (block, copy) pairs in the order dbslmm_pcg_block takes them,
    // then those of the chip-wide blocks (flagged by dbslmm_pcg_update as each block converges)
    p->so.h_pfpairs.clear();
    for (const int2& f : flist)
        for (int c = f.y < 0 ? 0 : f.y; c < (f.y < 0 ? n : f.y + 1); ++c) p->so.h_pfpairs.push_back(int2{f.x, c});
    for (int b = 0; b < static_cast<int>(blk.size()); ++b)
        if (!blk[b].fused)
            for (int c = 0; c < n; ++c) p->so.h_pfpairs.push_back(int2{b, c});
    if (!flist.empty()) HIP_TRY(ctx, B.upload(&p->pcg.d_pflist, flist, ctx->stream));
    if (!flist.empty() && !p->pcg.d_pfnext) HIP_TRY(ctx, B.alloc(&p->pcg.d_pfnext, 4));   // (16 B)
    p->pcg.n_pblk = static_cast<int32_t>(blk.size());
    p->pcg.n_pitem = static_cast<int32_t>(items.size());
    p->pcg.n_prow = static_cast<int32_t>(rows.size());
    // past the tile rows, one header entry per block solved whole: a trimmed dbslmm_pcg_init (run_pcg)
    // runs the chip-wide blocks' tile rows and these
    for (int b = 0; b < static_cast<int>(blk.size()); ++b)
        if (blk[b].fused) rows.push_back(int2{b, -1});
    p->pcg.n_phead = static_cast<int32_t>(rows.size()) - p->pcg.n_prow;
    p->pcg.vstride = vo;
    p->pcg.h_pmat = mat;
    p->pcg.h_ppart = part;
    HIP_TRY(ctx, B.upload(&p->pcg.d_pblk, blk, ctx->stream));
    HIP_TRY(ctx, B.upload(&p->pcg.d_pitem, items, ctx->stream));
    HIP_TRY(ctx, B.upload(&p->pcg.d_prow, rows, ctx->stream));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pvec, 6 * n * vo));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_ppart, po));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pdot, dof));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pqs, static_cast<size_t>(std::max<int32_t>(1, sco)) * pcg::kQS));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pcnv, sco));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pitb, p->pcg.n_pblk));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pdone, p->pcg.n_pblk));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pact, 1));
    HIP_TRY(ctx, B.alloc(&p->pcg.d_pfin, p->pcg.n_pblk));
    p->pcg.n = n;
    return DBSLMM_OK;
}

// Iterations the first chunk of a run enqueues: the previous run's count (same data), else the
// Chebyshev bound of the well-conditioned case, kappa = 1 + 12 / (d_min + 1 - tau), + 2, + 4 when
// large SNPs add outlying eigenvalues (tools/cg_gate.py: +4 at 10 large SNPs in a block).
static int pcg_first_chunk(const dbslmm_plan* p, const double* sigmas, int n) {
    if (p->pcg.need >= 0) return std::min(p->pcg.need, p->opt.pcg_maxit);   // (0: every block solved whole)
    double dmin = INFINITY;
    for (int c = 0; c < n; ++c) dmin = std::min(dmin, 1.0 / (sigmas[c] * static_cast<double>(p->n_obs)));
    const double kap = 1.0 + 12.0 / std::max(1e-3, dmin + 1.0 - p->tau);
    const double q = (std::sqrt(kap) - 1.0) / (std::sqrt(kap) + 1.0);
    const int k = static_cast<int>(std::ceil(std::log(2.0 / p->opt.pcg_tol) / -std::log(q))) + 2 + (p->has_large ? 4 : 0);
    return std::clamp(k, 1, p->opt.pcg_maxit);
}

// K iterations (product, rows, update) and the tail (betas, status, convergence read-back).
static int pcg_iters(dbslmm_plan* p, int K) {
    dbslmm_ctx* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    for (int k = 0; k < K; ++k) {
        const int32_t ni = p->pcg.trim ? p->pcg.n_pitem_chip : p->pcg.n_pitem, nr = p->pcg.trim ? p->pcg.n_prow_chip : p->pcg.n_prow;
        if (ni == 0 && nr == 0) continue;
        const dim3 g((std::max(1, ni) + pcg::kWaves - 1) / pcg::kWaves);
        if (p->pcg.g16)
            hipLaunchKernelGGL(dbslmm_pcg_symv16, g, dim3(pcg::kThreads), pcg::lds_bytes(p->pcg.n), s, p->pcg.args,
                               p->pcg.d_pitem, ni);
        if (!p->pcg.g16 || p->pcg.m_blocks != 0)   // (-1: not known yet)
            hipLaunchKernelGGL(dbslmm_pcg_symv64, g, dim3(pcg::kThreads), pcg::lds_bytes(p->pcg.n), s, p->pcg.args,
                               p->pcg.d_pitem, ni);
        hipLaunchKernelGGL(dbslmm_pcg_rows, dim3(std::max(1, nr)), dim3(pcg::kThreads), 0, s, p->pcg.args, p->pcg.d_prow);
        hipLaunchKernelGGL(dbslmm_pcg_update, dim3(std::max(1, nr)), dim3(pcg::kThreads), 0, s, p->pcg.args, p->pcg.d_prow);
    }
    HIP_TRY(ctx, hipGetLastError());
    p->pcg.it += K;
    if (p->pcg.join) {   // dbslmm_pcg_block's x / cnv / itb before the betas and the read-back
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->join, 0));
        p->pcg.join = false;
    }
    hipLaunchKernelGGL(dbslmm_pcg_final, dim3(p->pcg.n_prow), dim3(pcg::kThreads), 0, s, p->pcg.args, p->pcg.d_prow);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(p->pcg.h_mon(), p->pcg.d_pact, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(p->pcg.h_mon() + 1, p->pcg.d_pitb, p->pcg.n_pblk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (p->tm.pcg_ev_end) HIP_TRY(ctx, hipEventRecord(p->tm.pcg_ev_end, s));
    if (p->so.active) HIP_TRY(ctx, hipEventRecord(p->so.ev[0], s));   // (a streamed run polls it: stream_results)
    return DBSLMM_OK;
}

// Wait for the latest chunk of a pending PCG run; while blocks still iterate (and the cap allows),
// enqueue a further chunk (the run stays pending), else close the run.
static int pcg_check(dbslmm_plan* p) {
    dbslmm_ctx* ctx = p->ctx;
    if (p->pcg.pending) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        int32_t need = 0;
        for (int b = 0; b < p->pcg.n_pblk; ++b)   // (the chip-wide blocks: the chunk sizes are theirs)
            if (p->pcg.h_pfused.empty() || !p->pcg.h_pfused[b]) need = std::max(need, p->pcg.h_mon()[1 + b]);
        if (p->pcg.h_mon()[0] <= 0 || p->pcg.it >= p->opt.pcg_maxit) {
            p->pcg.pending = false;
            p->pcg.need = p->pcg.h_mon()[0] <= 0 ? need : p->opt.pcg_maxit;
            p->pcg.iters_max = 0;
            for (int b = 0; b < p->pcg.n_pblk; ++b) p->pcg.iters_max = std::max(p->pcg.iters_max, p->pcg.h_mon()[1 + b]);
            if (p->pcg.m_blocks < 0) {   // missing-call flags are data: read once, after the first run
                std::vector<int32_t> fl(std::max(1, p->n_nonempty));
                HIP_TRY(ctx, hipMemcpy(fl.data(), p->d_flags, fl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
                p->pcg.m_blocks = 0;
                p->pcg.h_pmiss.assign(p->pcg.n_pblk, 0);
                for (int b = 0; b < p->n_nonempty; ++b) {
                    p->pcg.m_blocks += fl[b] & 1;
                    if (b < p->pcg.n_pblk) p->pcg.h_pmiss[b] = fl[b] & 1;
                }
            }
            p->pcg.trim = true;   // (the fused flags are those of the current layout)
            for (int b = 0; b < p->pcg.n_pblk && b < static_cast<int>(p->pcg.h_pfused.size()); ++b)
                if (p->pcg.h_pfused[b] && p->pcg.h_pmiss[b]) p->pcg.trim = false;
            // bytes the run streamed: every block its own iteration count
            p->pcg.cbytes = p->pcg.pbytes = p->pcg.fbytes = 0.0;
            for (int b = 0; b < p->pcg.n_pblk && b < static_cast<int>(p->pcg.h_pmat.size()); ++b) {
                const double it = p->pcg.h_mon()[1 + b];
                const bool miss = !p->pcg.h_pmiss.empty() && p->pcg.h_pmiss[b];
                const double mb = p->pcg.h_pmat[b] * (miss && p->pcg.g16 ? 4.0 : 1.0);
                if (!p->pcg.h_pfused.empty() && p->pcg.h_pfused[b] && !miss) {
                    p->pcg.fbytes += it * mb * p->pcg.h_pnseq[b];
                } else {
                    p->pcg.cbytes += it * mb;
                    p->pcg.pbytes += it * p->pcg.h_ppart[b];
                }
            }
            return DBSLMM_OK;
        }
        const int K = std::min(std::max(4, p->pcg.it / 4), p->opt.pcg_maxit - p->pcg.it);
        if (const int rc = pcg_iters(p, K)) return rc;
    }
    return DBSLMM_OK;
}

// Wait for a PCG run, continuation chunks included.
static int pcg_finish(dbslmm_plan* p) {
    while (p->pcg.pending)
        if (const int rc = pcg_check(p)) return rc;
    return DBSLMM_OK;
}

// The mirror and flags of a streamed run of n copies, and its run number.
static int so_prepare(dbslmm_plan* p, int n) {
    dbslmm_ctx* ctx = p->ctx;
    const size_t bytes = static_cast<size_t>(n) * (p->n_s + p->n_l) * sizeof(double) +
                         static_cast<size_t>(n) * p->nbk * sizeof(int32_t);
    HIP_TRY(ctx, p->so.mir.reserve(bytes));
    const size_t nf = static_cast<size_t>(std::max(1, p->n_nonempty)) * pcg::kMaxNC;
    const bool fresh = !p->so.mflag.get();
    HIP_TRY(ctx, p->so.mflag.reserve(nf * sizeof(int32_t)));
    HIP_TRY(ctx, p->so.ev.grow(1));
    // a new mirror, or the run numbers wrap (no run in flight here): flags and marks restart with the numbers
    if (fresh || p->so.run == INT32_MAX) {
        memset(p->so.mflag.get(), 0, nf * sizeof(int32_t));
        p->so.done.assign(nf, 0);
        p->so.run = 0;
    }
    p->so.run++;
    p->so.n = n;
    return DBSLMM_OK;
}

// One run on the PCG route: statistics + Gram (the integer Gram as uint16 where it fits, Sigma in fp64
// for the other blocks), then the iterations of every block and copy together.
static int run_pcg(dbslmm_plan* p, const double* sigmas, int n) {
    dbslmm_ctx* ctx = p->ctx;
    auto diag_error = [](const char* when) {   // (diagnostic builds only)
#ifdef DBSLMM_DIAG
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) fprintf(stderr, "run_pcg: %s: %s\n", when, hipGetErrorString(e));
#endif
    };
    diag_error("stale error on entry");
    if (const int rc = ensure_copies(p, n, 1)) return rc;
    diag_error("error after ensure_copies");
    if (const int rc = pcg_layout(p, n)) return rc;
    diag_error("error after pcg_layout");
    // results streamed to the host while the run iterates: dbslmm_plan_run_multi on one device
    p->so.active = p->so.want && p->opt.stream_out;
    if (p->so.active)
        if (const int rc = so_prepare(p, n)) return rc;
    hipStream_t s = ctx->stream;
    hipEvent_t* ev = nullptr;
    if (const int rc = open_timed_run(p, true, &ev)) return rc;
    p->tm.pcg_ev_end = ev ? ev[kEvEnd] : nullptr;
    p->fac.trsv_failed = false;
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
    fr.active = p->pcg.d_pact;
    fr.next = p->pcg.n_pflist > 0 ? p->pcg.d_pfnext : nullptr;
    hipLaunchKernelGGL(dbslmm_pcg_front, dim3(std::max(1, (p->n_slots + 255) / 256)), dim3(256), 0, s, p->img.rows(),
                       p->n_ref, p->d_slot_pos, p->d_slot_block, p->n_slots, p->d_S, p->d_mu, p->d_rsd, p->d_flags, fr);
    HIP_TRY(ctx, hipGetLastError());
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvStatsEnd], s));
    uint16_t* g16 = p->pcg.g16 ? p->pcg.d_G16 : nullptr;
    const double nrd = static_cast<double>(p->n_ref);
    // one copy of Sigma, and the integer Gram as uint16 where it fits
    const GramOut go{1, INT32_MAX, -1, g16, p->pcg.d_off16, p->pcg.d_ld16};
    // (Measured and dropped: the Gram of the blocks dbslmm_pcg_block solves on the second stream
    // beside the chip-wide iterations -- its 256-tile workgroups hold 128 KiB of LDS, so the product
    // items cannot run beside them: config 4 8.8 -> 9.6 ms.)
    HIP_TRY(ctx, launch_gram(p, s, kGramHuge, p->d_htiles, p->n_htiles, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramI8, p->d_tiles, p->n_tiles, go));
    HIP_TRY(ctx, launch_gram(p, s, kGramBig, p->d_btiles, p->n_btiles, go));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvGramEnd], s));
    PcgArgs a{};
    a.blk = p->pcg.d_pblk;
    a.G16 = g16;
    a.M = p->d_M;
    a.flags = p->d_flags;
    a.S = p->d_S;
    a.rsd = p->d_rsd;
    a.z = p->d_z;
    a.slot_out = p->d_slot_out;
    a.blk_id = p->d_blk_id;
    a.dshift = p->d_dshift;
    const int64_t vs = static_cast<int64_t>(n) * p->pcg.vstride;
    a.X = p->pcg.d_pvec;
    a.R = a.X + vs;
    a.P = a.R + vs;
    a.Sv = a.P + vs;
    a.W = a.Sv + vs;
    a.U = a.W + vs;
    a.part = p->pcg.d_ppart;
    a.dot = p->pcg.d_pdot;
    a.qs = p->pcg.d_pqs;
    a.cnv = p->pcg.d_pcnv;
    a.itb = p->pcg.d_pitb;
    a.done = p->pcg.d_pdone;
    a.active = p->pcg.d_pact;
    a.fin = p->pcg.d_pfin;
    a.beta_s = p->d_beta_s;
    a.beta_l = p->d_beta_l;
    a.status = p->d_status;
    if (p->so.active) {   // the mirror through its device addresses: [beta_s | beta_l | status]
        void *dm = nullptr, *df = nullptr;
        HIP_TRY(ctx, hipHostGetDevicePointer(&dm, p->so.mir.get(), 0));
        HIP_TRY(ctx, hipHostGetDevicePointer(&df, p->so.mflag.get<int32_t>(), 0));
        a.mir_s = static_cast<double*>(dm);
        a.mir_l = a.mir_s + static_cast<int64_t>(n) * p->n_s;
        a.mir_st = reinterpret_cast<int32_t*>(a.mir_l + static_cast<int64_t>(n) * p->n_l);
        a.mir_flag = static_cast<int32_t*>(df);
        a.run_no = p->so.run;
    }
    a.vstride = p->pcg.vstride;
    a.ns = p->n_s;
    a.nl = p->n_l;
    a.nbk = p->nbk;
    a.tau = p->tau;
    a.rn = 1.0 / nrd;
    a.c0 = p->tau * (nrd - 1.0) / nrd + 1.0 - p->tau;
    a.tol = p->opt.pcg_tol;
    a.inv_sqrt_n = 1.0 / std::sqrt(static_cast<double>(p->n_obs));
    a.ncopy = n;
    a.run = p->pcg.run;
                         // the multi-shift seed: the smallest shift (largest sigma)
    for (int c = 1; c < n; ++c)
        if (sigmas[c] > sigmas[a.seed]) a.seed = c;
    p->pcg.args = a;
    // Once a run has read the missing-call flags and none of the blocks dbslmm_pcg_block takes has
    // any (pcg_trim), those blocks keep their whole state in LDS: their tile rows' vectors are
    // neither written nor read, and one header workgroup each does what their tile row 0 did.
    if (p->pcg.trim)
        hipLaunchKernelGGL(dbslmm_pcg_init, dim3(std::max(1, p->pcg.n_prow_chip + p->pcg.n_phead)), dim3(pcg::kThreads), 0, s, a,
                           p->pcg.d_prow, p->pcg.n_prow_chip, p->pcg.n_prow - p->pcg.n_prow_chip);
    else
        hipLaunchKernelGGL(dbslmm_pcg_init, dim3(p->pcg.n_prow), dim3(pcg::kThreads), 0, s, a, p->pcg.d_prow, p->pcg.n_prow, 0);
    HIP_TRY(ctx, hipGetLastError());
    p->pcg.join = false;
    if (p->pcg.n_pflist > 0) {   // the small blocks' whole solves beside the chip-wide iterations
        HIP_TRY(ctx, hipEventRecord(ctx->fork, s));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->fork, 0));
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvPcgBlockBegin], ctx->stream2));
        // one workgroup per CU (its LDS holds x and p: one fits): the chip-wide kernels of the
        // other blocks keep the rest of every CU
        // (two per CU at one copy, where their LDS fits: configs 3 / 5 6.02 -> 6.27 / 2.35 -> 2.51 ms)
        int grid = std::max(1, std::min(p->pcg.n_pflist, ctx->n_cu));
        if (p->opt.pcg_block_wgs > 0) grid = std::min(grid, p->opt.pcg_block_wgs);
        hipLaunchKernelGGL(dbslmm_pcg_block, dim3(grid), dim3(pcg::kThreads), pcg::block_lds_bytes(n), ctx->stream2, a,
                           p->pcg.d_pflist, p->pcg.n_pflist, p->pcg.d_pfnext, p->opt.pcg_maxit);
        HIP_TRY(ctx, hipGetLastError());
        if (ev) HIP_TRY(ctx, hipEventRecord(ev[kEvPcgBlockEnd], ctx->stream2));
        HIP_TRY(ctx, hipEventRecord(ctx->join, ctx->stream2));
        p->pcg.join = true;
    } else if (const int rc = record_instants(ctx, ev, {kEvPcgBlockBegin, kEvPcgBlockEnd}, s)) {
        return rc;
    }
    p->pcg.it = 0;
    p->pcg.pending = true;
    if (const int rc = pcg_iters(p, pcg_first_chunk(p, sigmas, n))) return rc;
    p->n_runs++;
    LastRun r;   // (no h2f iterations on this route: cheb_base -1, cheb_* / cg_ran at their zeros)
    r.ran = true;
    r.stopped = false;
    r.sigma_run = sigmas[n - 1];
    r.var_copy = n - 1;
    r.score_copies = n;
    r.score_stale = false;
    r.pcg_ran = true;
    r.pcg_pending_var = true;   // Sigma is not factored: the variance factors it first
    r.cheb_base = -1;
    r.cheb_pending_var = false;
    r.cg_ran = false;
    r.cheb_iters = r.cheb_bytes = 0;
    close_run(p, r);
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
    const int n = p->so.n;
    const int32_t run = p->so.run;
    const double* ms = p->so.mir.get<double>();
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
        p->so.done[static_cast<size_t>(b) * n + c] = run;
    };
    const std::vector<int2>& pairs = p->so.h_pfpairs;
    size_t head = 0;                         // every pair before it is copied
    bool polled = false;
    while (p->pcg.pending) {
        for (;;) {
            const hipError_t q = hipEventQuery(p->so.ev[0]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIP_TRY(ctx, q);
            polled = true;
            for (size_t e = head; e < pairs.size(); ++e) {
                const size_t f = static_cast<size_t>(pairs[e].x) * n + pairs[e].y;
                if (p->so.done[f] != run && __atomic_load_n(p->so.mflag.get<int32_t>() + f, __ATOMIC_ACQUIRE) == run)
                    copy_out(pairs[e].x, pairs[e].y);
            }
            while (head < pairs.size() && p->so.done[static_cast<size_t>(pairs[head].x) * n + pairs[head].y] == run)
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
        for (int b = 0; b < p->pcg.n_pblk;) {
            if (p->so.done[static_cast<size_t>(b) * n + c] == run) { ++b; continue; }
            int e = b;
            while (e + 1 < p->pcg.n_pblk && p->so.done[static_cast<size_t>(e + 1) * n + c] != run) ++e;
            const OutRange &r0 = p->h_orange[b], &r1 = p->h_orange[e];
            if (beta_s && r1.s1 > r0.s0)
                rest.push_back({beta_s + c * p->n_s + r0.s0, ms + c * p->n_s + r0.s0, (r1.s1 - r0.s0) * sizeof(double)});
            if (beta_l && r1.l1 > r0.l0)
                rest.push_back({beta_l + c * p->n_l + r0.l0, ml + c * p->n_l + r0.l0, (r1.l1 - r0.l0) * sizeof(double)});
            for (int k = b; k <= e; ++k) {
                const int32_t id = p->h_orange[k].blk;
                if (block_status) block_status[static_cast<int64_t>(c) * p->num_block + id] = mst[c * p->nbk + id];
                p->so.done[static_cast<size_t>(k) * n + c] = run;
            }
            b = e + 1;
        }
    par_memcpy_list(rest);
    for (int c = 0; c < n && block_status; ++c)
        for (int32_t b : p->h_empty) block_status[static_cast<int64_t>(c) * p->num_block + b] = DBSLMM_BLOCK_EMPTY;
    return collect_timing(p);
}

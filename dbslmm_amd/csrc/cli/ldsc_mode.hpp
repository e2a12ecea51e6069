// ldsc_mode.hpp -- the --ldsc mode of the dbslmm CLI (included by dbslmm_main.cpp after its
// parsers): LD scores of every row of the reference panels (dbslmm_ld_scores) and the LD score
// regression of the summary statistics on them (dbslmm_ldsc_fit) -- the heritability the
// reference's manual takes from an LDSC run (Rmd/Manual.Rmd:170, -h of the solve).
//
//   dbslmm --ldsc --summary F1[,F2,...] -r P1[,P2,...] --out PREFIX [--ld-wind-kb 1000]
//          [--intercept free|X] [--chisq-max X] [--gpu G] [--dry-run]
//
// Panels and summaries pair up in order (one per chromosome, or one whole-genome pair).
//   M                the rows with a finite LD score and MAF > 0.05 (dbslmm_bed_maf), over all panels
//   regression SNPs  per panel in .bim order: the rows a summary SNP names (the first summary line of
//                    a SNP id), with a finite LD score, z = beta / se as read_summ forms it and
//                    N = the summary's n_obs field (column 5) > 0
// Writes PREFIX.l2.ldscore (CHR SNP BP L2), PREFIX.l2.M_5_50 and PREFIX.h2.txt.

// n_obs (field 5) of the lines read_summ keeps (at least 11 fields), in file order
inline vector<double> read_summ_nobs(const MappedText& f) {
    vector<double> out;
    for (string_view line : lines_of(f.text)) {
        string_view fl[11];
        if (tab_fields(line, fl, 11) < 11) continue;
        out.push_back(field_atof(fl[4]));
    }
    return out;
}

struct LdscPanel {
    string prefix;
    int n_ref = 0;
    MappedText bim_txt, summ_txt;
    Bim bim;
    vector<int32_t> summ_of;        // per .bim row: its regression summary line (-1: none)
    vector<double> z, n_obs;        // per summary line
};

inline int ldsc_mode(const Param& p) {
    if (!p.s.empty() || !p.l.empty() || !p.b.empty())
        return fail("--ldsc takes --summary and -r only: no -s / -l / -b");
    if (p.out.empty()) return fail("--ldsc needs --out (the prefix of its output files)");
    if (p.summary.empty() || p.r.empty()) return fail("--ldsc needs --summary and -r");
    const vector<string> refs = split(p.r, ','), summs = split(p.summary, ',');
    if (refs.size() != summs.size() || refs.empty())
        return fail("--ldsc: -r and --summary must list the same number of files");
    if (!(p.ld_wind_kb >= 0)) return fail("--ld-wind-kb must not be negative");
    if (!(p.chisq_max >= 0)) return fail("--chisq-max must not be negative");
    bool fixed = false;
    double a0 = 1.0;
    if (p.intercept != "free") {
        char* end = nullptr;
        a0 = strtod(p.intercept.c_str(), &end);
        if (p.intercept.empty() || *end != 0 || !std::isfinite(a0)) return fail("--intercept must be `free` or a number");
        fixed = true;
    }
    vector<LdscPanel> panels(refs.size());
    int64_t n_rows_all = 0, n_reg = 0;
    for (size_t i = 0; i < refs.size(); ++i) {
        LdscPanel& P = panels[i];
        P.prefix = refs[i];
        for (const char* ext : {".fam", ".bim", ".bed"})
            if (!std::ifstream(P.prefix + ext)) return fail(P.prefix + ext + " dose not exist!");
        if (!std::ifstream(summs[i])) return fail(summs[i] + " dose not exist!");
        P.n_ref = get_row(P.prefix + ".fam");
        P.bim_txt.open(P.prefix + ".bim");
        read_bim(P.bim_txt, P.bim);
        P.summ_txt.open(summs[i]);
        const vector<Summ> summ = read_summ(P.summ_txt);
        P.n_obs = read_summ_nobs(P.summ_txt);
        if (P.n_obs.size() != summ.size()) return fail(summs[i] + ": inconsistent line count");
        const vector<int32_t> rows = lookup_ref(summ, P.bim);
        P.z.resize(summ.size());
        P.summ_of.assign(P.bim.snp.size(), -1);
        for (size_t s = 0; s < summ.size(); ++s) {
            P.z[s] = summ[s].z;
            if (rows[s] >= 0 && P.n_obs[s] > 0 && P.summ_of[rows[s]] < 0) P.summ_of[rows[s]] = static_cast<int32_t>(s);
        }
        for (int32_t s : P.summ_of) n_reg += s >= 0;
        n_rows_all += static_cast<int64_t>(P.bim.snp.size());
        std::cout << P.prefix << ": " << P.n_ref << " individuals, " << P.bim.snp.size() << " rows\n";
    }
    if (p.dry_run) {
        std::cout << "dry-run: " << n_rows_all << " rows, " << n_reg << " regression SNPs; stops before the LD scores\n";
        return 0;
    }
    dbslmm_ctx* ctx = nullptr;
    if (dbslmm_ctx_create(p.gpu, &ctx) != DBSLMM_OK) return fail("no usable HIP device (dbslmm_ctx_create)");
    struct CtxGuard { dbslmm_ctx* c; ~CtxGuard() { dbslmm_ctx_destroy(c); } } guard{ctx};
    const dbslmm_l2_args la{static_cast<int64_t>(std::llround(p.ld_wind_kb * 1000.0)), 1, 0};
    string ld_out = "CHR\tSNP\tBP\tL2\n";
    vector<double> chi2, nn, ll;
    int64_t M = 0;
    double gpu_ms = 0.0;
    for (LdscPanel& P : panels) {
        const int32_t n = static_cast<int32_t>(P.bim.snp.size());
        Mapped bed;
        if (!bed.open(P.prefix + ".bed")) return fail(P.prefix + ".bed cannot be opened");
        if (static_cast<int64_t>(bed.n) < 3 + static_cast<int64_t>(n) * ((P.n_ref + 3) / 4))
            return fail(P.prefix + ".bed is shorter than its .bim and .fam say");
        if (dbslmm_ctx_cache_bed_fd(ctx, bed.fd, static_cast<int64_t>(bed.n), bed.p) != DBSLMM_OK)
            return fail(string("uploading the .bed: ") + dbslmm_last_error(ctx));
        vector<int32_t> pos(n), chr(n);
        vector<int64_t> bp(n);
        std::unordered_map<string_view, int32_t> chr_code;
        for (int32_t r = 0; r < n; ++r) {
            pos[r] = r;
            chr[r] = chr_code.emplace(P.bim.chr[r], static_cast<int32_t>(chr_code.size())).first->second;
            bp[r] = P.bim.bp[r];
        }
        vector<double> l2(n), maf(n);
        double ms = 0.0;
        if (dbslmm_ld_scores(ctx, bed.p, static_cast<int64_t>(bed.n), P.n_ref, n, pos.data(), chr.data(), bp.data(), &la,
                             l2.data(), nullptr, &ms) != DBSLMM_OK)
            return fail(string("dbslmm_ld_scores: ") + dbslmm_last_error(ctx));
        if (dbslmm_bed_maf(ctx, bed.p, static_cast<int64_t>(bed.n), P.n_ref, n, maf.data()) != DBSLMM_OK)
            return fail(string("MAF pass: ") + dbslmm_last_error(ctx));
        gpu_ms += ms;
        char num[64];
        for (int32_t r = 0; r < n; ++r) {
            const bool ok = std::isfinite(l2[r]);
            if (ok && maf[r] > 0.05) ++M;
            ld_out.append(P.bim.chr[r].data(), P.bim.chr[r].size());
            ld_out += '\t';
            ld_out.append(P.bim.snp[r].data(), P.bim.snp[r].size());
            ld_out += '\t' + std::to_string(bp[r]) + '\t';
            if (ok) snprintf(num, sizeof(num), "%.10g", l2[r]);
            else snprintf(num, sizeof(num), "nan");
            ld_out += num;
            ld_out += '\n';
            const int32_t s = P.summ_of[r];
            if (s >= 0 && ok) {
                chi2.push_back(P.z[s] * P.z[s]);
                nn.push_back(P.n_obs[s]);
                ll.push_back(l2[r]);
            }
        }
    }
    auto write = [](const string& path, const string& text) {
        std::ofstream f(path, std::ios::binary);
        f.write(text.data(), static_cast<std::streamsize>(text.size()));
        f.close();
        return static_cast<bool>(f);
    };
    if (!write(p.out + ".l2.ldscore", ld_out)) return fail(p.out + ".l2.ldscore cannot be written");
    if (!write(p.out + ".l2.M_5_50", std::to_string(M) + "\n")) return fail(p.out + ".l2.M_5_50 cannot be written");
    std::cout << "LD scores of " << n_rows_all << " rows within " << p.ld_wind_kb << " kb (" << gpu_ms
              << " ms on the GPU); M_5_50 = " << M << "\n";
    if (M <= 0) return fail("no row with a finite LD score and MAF > 0.05");
    const dbslmm_ldsc_args fa{a0, p.chisq_max, fixed ? 1 : 0, 0};
    dbslmm_ldsc_result res;
    if (dbslmm_ldsc_fit(static_cast<int64_t>(chi2.size()), chi2.data(), nn.data(), ll.data(), static_cast<double>(M), &fa,
                        &res) != DBSLMM_OK)
        return fail("dbslmm_ldsc_fit: bad arguments");
    if (res.status == DBSLMM_LDSC_TOO_FEW)
        return fail("LD score regression: too few SNPs (" + std::to_string(res.n_used) + ")");
    if (res.status != DBSLMM_LDSC_OK) return fail("LD score regression: singular normal equations");
    char buf[512];
    string h;
    snprintf(buf, sizeof(buf), "h2 %.10g %.10g\n", res.h2, res.h2_se);
    h += buf;
    if (fixed) snprintf(buf, sizeof(buf), "intercept %.10g fixed\n", a0);
    else snprintf(buf, sizeof(buf), "intercept %.10g %.10g\n", res.intercept, res.intercept_se);
    h += buf;
    snprintf(buf, sizeof(buf), "M %lld\nn_snp %lld\nmean_chi2 %.10g\n", static_cast<long long>(M),
             static_cast<long long>(res.n_used), res.mean_chi2);
    h += buf;
    if (!write(p.out + ".h2.txt", h)) return fail(p.out + ".h2.txt cannot be written");
    std::cout << h;
    return 0;
}

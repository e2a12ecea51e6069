// assoc_mode.hpp -- the --assoc mode of the dbslmm CLI (included by dbslmm_main.cpp after its
// parsers): the association scan of training panels (dbslmm_assoc), written as the 11-column GEMMA
// *.assoc.txt that --ldsc, --summary / --pth and -s / -l read -- the summary statistics the
// reference's workflow takes from a GEMMA run (Rmd/Manual.Rmd).
//
//   dbslmm --assoc -r TRAIN[,TRAIN2,...] --out PREFIX [--pheno FILE] [--pheno-col K[,K2,...]]
//          [--covar FILE] [--keep FILE] [--maf-min X] [--miss-max X] [--assoc-header] [--precise-out]
//          [--gpu G] [--dry-run]
//
// The panels of a comma list hold the same individuals (their .fam files name the same FID / IID in
// the same order) and are written one after the other.  Phenotypes: column 6 of the first .fam
// (-9, NA and absent are missing, as --score reads it), or the value columns K, K2, ... (1-based) of
// --pheno, a file of `FID IID v1 v2 ...` lines matched to the .fam by FID and IID; --covar likewise,
// all of its value columns (the intercept is added by the library).  NA or a non-number is missing
// (in --pheno also -9); an individual without a line, or with a missing value, is left out of the
// sample.  --keep is an indicator file in the format of -test_indicator_file (one line per .fam
// line, first field non-zero = kept).
// One file per trait: PREFIX.assoc.txt (one trait) or PREFIX.<k>.assoc.txt, k = 1 .. P; columns
//   chr rs ps n_mis n_obs allele1 allele0 af beta se p_wald
// tab-separated, af as %.3f and beta, se, p_wald as %e (GEMMA's formats), or 17 significant digits
// with --precise-out; no header line unless --assoc-header.  A row whose status is not OK, whose
// folded af is below --maf-min (default 0) or whose missing fraction n_mis / n is above --miss-max
// (default 1) is left out and listed with the reason in PREFIX.assoc.skipped.
// --dry-run stops before any GPU work, after the parsing, the matching and the QR of the covariates.
#include "../assoc_layout.hpp"

// `FID IID v1 v2 ...` lines -> per key "FID\tIID" the values (NaN for NA / a non-number; minus9: also -9)
inline bool read_value_file(const string& path, bool minus9, std::unordered_map<string, vector<double>>& out,
                            size_t& n_values) {
    std::ifstream f(path);
    if (!f) return false;
    string line;
    n_values = 0;
    bool first = true;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        vector<string> t;
        for (string w; is >> w;) t.push_back(w);
        if (t.size() < 2) continue;
        vector<double> v;
        for (size_t k = 2; k < t.size(); ++k) {
            double y = std::nan("");
            if (t[k] != "NA" && !(minus9 && t[k] == "-9")) {
                char* end = nullptr;
                const double x = strtod(t[k].c_str(), &end);
                if (end != t[k].c_str() && *end == 0) y = x;
            }
            v.push_back(y);
        }
        if (first || v.size() < n_values) n_values = v.size();   // the columns every line has
        first = false;
        out.emplace(t[0] + "\t" + t[1], std::move(v));             // (the first line of an individual wins)
    }
    return true;
}

inline int assoc_mode(const Param& p) {
    if (!p.s.empty() || !p.l.empty() || !p.b.empty() || !p.summary.empty())
        return fail("--assoc takes -r and its own options only: no -s / -l / -b / --summary");
    if (p.out.empty()) return fail("--assoc needs --out (the prefix of its output files)");
    if (p.r.empty()) return fail("--assoc needs -r (the training panels)");
    if (!(p.maf_min >= 0.0 && p.maf_min <= 0.5)) return fail("--maf-min must lie in [0, 0.5]");
    if (!(p.miss_max >= 0.0 && p.miss_max <= 1.0)) return fail("--miss-max must lie in [0, 1]");
    const vector<string> refs = split(p.r, ',');
    if (refs.empty()) return fail("--assoc needs -r (the training panels)");
    struct Panel { string prefix; MappedText bim_txt; Bim bim; };
    vector<Panel> panels(refs.size());
    Fam fam;
    int64_t n_rows_all = 0;
    for (size_t i = 0; i < refs.size(); ++i) {
        Panel& Pn = panels[i];
        Pn.prefix = refs[i];
        for (const char* ext : {".fam", ".bim", ".bed"})
            if (!std::ifstream(Pn.prefix + ext)) return fail(Pn.prefix + ext + " dose not exist!");
        const Fam f = read_fam(Pn.prefix + ".fam");
        if (i == 0) fam = f;
        else if (f.fid != fam.fid || f.iid != fam.iid)
            return fail(Pn.prefix + ".fam does not list the individuals of " + refs[0] + ".fam");
        Pn.bim_txt.open(Pn.prefix + ".bim");
        read_bim(Pn.bim_txt, Pn.bim);
        n_rows_all += static_cast<int64_t>(Pn.bim.snp.size());
    }
    const int32_t n_total = static_cast<int32_t>(fam.fid.size());
    if (n_total < 1) return fail(refs[0] + ".fam is empty");
    // phenotypes
    vector<int> cols;
    for (const string& c : split(p.pheno_col, ',')) {
        char* end = nullptr;
        const long k = strtol(c.c_str(), &end, 10);
        if (c.empty() || *end != 0 || k < 1 || k > 1000000) return fail("--pheno-col must list column numbers from 1");
        cols.push_back(static_cast<int>(k));
    }
    if (cols.empty()) cols.push_back(1);
    const int32_t P = static_cast<int32_t>(cols.size());
    vector<double> pheno(static_cast<size_t>(n_total) * P, std::nan(""));
    if (p.pheno.empty()) {
        if (P != 1 || cols[0] != 1) return fail("--pheno-col " + p.pheno_col + ": the .fam holds one phenotype (column 1)");
        pheno = fam.pheno;
    } else {
        std::unordered_map<string, vector<double>> tab;
        size_t nv = 0;
        if (!read_value_file(p.pheno, true, tab, nv)) return fail(p.pheno + " dose not exist!");
        for (int k : cols)
            if (static_cast<size_t>(k) > nv) return fail("--pheno-col " + std::to_string(k) + ": " + p.pheno + " has " + std::to_string(nv) + " value columns");
        for (int32_t i = 0; i < n_total; ++i) {
            const auto it = tab.find(fam.fid[i] + "\t" + fam.iid[i]);
            if (it == tab.end()) continue;
            for (int32_t q = 0; q < P; ++q) pheno[static_cast<size_t>(i) * P + q] = it->second[cols[q] - 1];
        }
    }
    // covariates
    int32_t c1 = 0;
    vector<double> covar;
    if (!p.covar.empty()) {
        std::unordered_map<string, vector<double>> tab;
        size_t nv = 0;
        if (!read_value_file(p.covar, false, tab, nv)) return fail(p.covar + " dose not exist!");
        if (nv < 1) return fail(p.covar + " has no value column");
        c1 = static_cast<int32_t>(nv);
        covar.assign(static_cast<size_t>(n_total) * c1, std::nan(""));
        for (int32_t i = 0; i < n_total; ++i) {
            const auto it = tab.find(fam.fid[i] + "\t" + fam.iid[i]);
            if (it == tab.end()) continue;
            for (int32_t k = 0; k < c1; ++k) covar[static_cast<size_t>(i) * c1 + k] = it->second[k];
        }
    }
    vector<uint8_t> keep;
    if (!p.keep.empty()) {
        if (!std::ifstream(p.keep)) return fail(p.keep + " dose not exist!");
        const vector<int32_t> ind = read_indicator(p.keep);
        if (ind.size() != static_cast<size_t>(n_total))
            return fail("--keep: " + std::to_string(ind.size()) + " lines for " + std::to_string(n_total) + " individuals");
        keep.resize(ind.size());
        for (size_t i = 0; i < ind.size(); ++i) keep[i] = ind[i] != 0;
    }
    // the sample and the QR, as dbslmm_assoc will form them
    assoc::Design D;
    const int64_t n_pad = (static_cast<int64_t>(n_total) + 255) / 256 * 256;
    if (!assoc::build_design(n_total, n_pad, keep.empty() ? nullptr : keep.data(), pheno.data(), P,
                             c1 ? covar.data() : nullptr, c1, D))
        return fail("--assoc: " + D.err);
    const int64_t n = D.n;
    std::cout << "assoc: n " << n << " of " << n_total << " individuals, c " << c1 + 1 << ", P " << P << ", "
              << n_rows_all << " rows\n";
    if (p.dry_run) {
        std::cout << "dry-run: n " << n << " c " << c1 + 1 << " P " << P << "; stops before the scan\n";
        return 0;
    }
    dbslmm_ctx* ctx = nullptr;
    if (dbslmm_ctx_create(p.gpu, &ctx) != DBSLMM_OK) return fail("no usable HIP device (dbslmm_ctx_create)");
    struct CtxGuard { dbslmm_ctx* c; ~CtxGuard() { dbslmm_ctx_destroy(c); } } guard{ctx};
    const dbslmm_assoc_args aa{keep.empty() ? nullptr : keep.data(), pheno.data(), c1 ? covar.data() : nullptr, P, c1, 0};
    vector<string> text(static_cast<size_t>(P));
    if (p.assoc_header)
        for (string& t : text) t = "chr\trs\tps\tn_mis\tn_obs\tallele1\tallele0\taf\tbeta\tse\tp_wald\n";
    string skipped;
    int64_t n_written = 0, n_skipped = 0;
    double gpu_ms = 0.0;
    for (Panel& Pn : panels) {
        const int32_t m = static_cast<int32_t>(Pn.bim.snp.size());
        Mapped bed;
        if (!bed.open(Pn.prefix + ".bed")) return fail(Pn.prefix + ".bed cannot be opened");
        if (static_cast<int64_t>(bed.n) < 3 + static_cast<int64_t>(m) * ((n_total + 3) / 4))
            return fail(Pn.prefix + ".bed is shorter than its .bim and .fam say");
        if (dbslmm_ctx_cache_bed_fd(ctx, bed.fd, static_cast<int64_t>(bed.n), bed.p) != DBSLMM_OK)
            return fail(string("uploading the .bed: ") + dbslmm_last_error(ctx));
        const size_t mm = static_cast<size_t>(std::max(m, 1));
        vector<int32_t> n_mis(mm), n_obs(mm), status(mm);
        vector<double> af(mm), beta(mm * P), se(mm * P), ts(mm * P), pv(mm * P);
        double ms = 0.0;
        if (dbslmm_assoc(ctx, bed.p, static_cast<int64_t>(bed.n), n_total, m, nullptr, &aa, n_mis.data(), n_obs.data(),
                         af.data(), beta.data(), se.data(), ts.data(), pv.data(), status.data(), nullptr, nullptr,
                         &ms) != DBSLMM_OK)
            return fail(string("dbslmm_assoc: ") + dbslmm_last_error(ctx));
        gpu_ms += ms;
        char num[256];
        for (int32_t r = 0; r < m; ++r) {
            const char* why = nullptr;
            if (status[r] == DBSLMM_ASSOC_NO_CALL) why = "no_call";
            else if (status[r] == DBSLMM_ASSOC_MONOMORPHIC) why = "monomorphic";
            else if (status[r] == DBSLMM_ASSOC_COLLINEAR) why = "collinear";
            else if (std::min(af[r], 1.0 - af[r]) < p.maf_min) why = "maf";
            else if (static_cast<double>(n_mis[r]) / static_cast<double>(n) > p.miss_max) why = "missing";
            if (why) {
                skipped.append(Pn.bim.snp[r].data(), Pn.bim.snp[r].size());
                skipped += '\t';
                skipped += why;
                skipped += '\n';
                ++n_skipped;
                continue;
            }
            string head;
            head.append(Pn.bim.chr[r].data(), Pn.bim.chr[r].size());
            head += '\t';
            head.append(Pn.bim.snp[r].data(), Pn.bim.snp[r].size());
            head += '\t' + std::to_string(Pn.bim.bp[r]) + '\t' + std::to_string(n_mis[r]) + '\t' + std::to_string(n_obs[r]) + '\t';
            head.append(Pn.bim.a1[r].data(), Pn.bim.a1[r].size());
            head += '\t';
            head.append(Pn.bim.a2[r].data(), Pn.bim.a2[r].size());
            for (int32_t q = 0; q < P; ++q) {
                const size_t o = static_cast<size_t>(q) * m + r;
                snprintf(num, sizeof(num), p.precise ? "\t%.17g\t%.17g\t%.17g\t%.17g\n" : "\t%.3f\t%e\t%e\t%e\n", af[r],
                         beta[o], se[o], pv[o]);
                text[q] += head;
                text[q] += num;
            }
            ++n_written;
        }
    }
    auto write = [](const string& path, const string& t) {
        std::ofstream f(path, std::ios::binary);
        f.write(t.data(), static_cast<std::streamsize>(t.size()));
        f.close();
        return static_cast<bool>(f);
    };
    for (int32_t q = 0; q < P; ++q) {
        const string path = P == 1 ? p.out + ".assoc.txt" : p.out + "." + std::to_string(q + 1) + ".assoc.txt";
        if (!write(path, text[q])) return fail(path + " cannot be written");
    }
    if (!write(p.out + ".assoc.skipped", skipped)) return fail(p.out + ".assoc.skipped cannot be written");
    std::cout << "assoc: " << n_written << " rows written, " << n_skipped << " skipped (" << gpu_ms << " ms on the GPU)\n";
    return 0;
}

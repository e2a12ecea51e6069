/*
 * dbslmm_hip.h -- C-ABI of the MI355X (gfx950) per-LD-block effect-size solver.
 *
 * Drop-in boundary for the hot path of fboehm/DBSLMM.  Every entry point below replaces one
 * reference interface (paths relative to the reference's scr/):
 *
 *   dbslmm_est            DBSLMMFIT::est (large+small, dbslmmfit.hpp:38-53, dbslmmfit.cpp:56-244)
 *                         and DBSLMMFIT::est (small only, dbslmmfit.hpp:55-66, :247-363):
 *                         l_ptr == NULL selects the LMM-only overload.  Called where
 *                         DBSLMM::BatchRun calls est (dbslmm.cpp:334-348, 375-386).
 *   dbslmm_plan_*         the same call split into upload / run / download so the solve can be
 *                         repeated with inputs resident in HBM (bench, h2f tuning).
 *   dbslmm_bed_maf        the MAF pass of IO::readBim (dtpr.cpp:93-102) = readSNPIm over every
 *                         reference SNP, maf only.
 *   dbslmm_clump          the large-effect clumping of software/DBSLMM.R:139-145 (`plink --clump` on
 *                         the reference panel): the index SNPs of a candidate list.
 *   dbslmm_ld_scores,     the heritability the reference takes from an LDSC run (Rmd/Manual.Rmd:170):
 *   dbslmm_ldsc_fit       LD scores of the reference panel and the LD score regression.
 *   dbslmm_assoc          the association scan that makes the summary statistics the reference reads
 *                         (a GEMMA *.assoc.txt, Rmd/Manual.Rmd): per-SNP linear model, Wald test.
 *   dbslmm_read_snp_std   IO::readSNPIm + SNPPROC::nomalizeVec (dtpr.cpp:285-364, 375-380) for a
 *                         list of bed rows: standardised fp64 columns (parity / diagnostics).
 *
 * Conventions: plain pointers and sizes, no C++ types, no exceptions across the boundary.
 * Every call returns 0 on success or a negative DBSLMM_E* code; dbslmm_last_error(ctx) then
 * holds a message.  The caller owns every buffer; inputs are read-only for the call.  One call
 * at a time per context; distinct contexts are independent.  A context drives one GPU
 * (dbslmm_ctx_create) or several (dbslmm_ctx_create_multi: the LD blocks of every plan are
 * sharded over the devices).
 */
#ifndef DBSLMM_HIP_H_
#define DBSLMM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBSLMM_ABI_VERSION 22

enum {
    DBSLMM_OK = 0,
    DBSLMM_E_ARG = -1,      /* invalid argument (sizes, NULL, ranges) */
    DBSLMM_E_HIP = -2,      /* HIP runtime error (no device, OOM, launch failure) */
    DBSLMM_E_STATE = -3     /* call sequence error (plan not run, ...) */
};

/* Per-block status written by dbslmm_est / dbslmm_plan_download. */
enum {
    DBSLMM_BLOCK_OK = 0,
    DBSLMM_BLOCK_EMPTY = 1,        /* no SNP in this block */
    DBSLMM_BLOCK_NOT_PD = 2,       /* joint LD matrix not positive definite -> beta = NaN
                                      (reference: PCG "Matrix is Singular!", dbslmmfit.cpp:664) */
    DBSLMM_BLOCK_MONOMORPHIC = 3,  /* a SNP with zero variance -> NaN column in the reference
                                      (dtpr.cpp:375-380); beta = NaN for the whole block */
    DBSLMM_BLOCK_NOT_CONVERGED = 4 /* an iterative solve stopped at its iteration cap without
                                      meeting its error bound: beta = the last iterate (the
                                      reference's PCG prints "Matrix is Singular!" at maxiter and
                                      returns its iterate, dbslmmfit.cpp:664-666).  The PCG route
                                      (solver, pcg_maxit) reports it, and so does an h2f copy
                                      iterated by CG on a base factor (h2f_iter) when pcg_maxit
                                      cut its cap below the a priori count and the copy was still
                                      above its bound there.  A copy that ran the whole a priori
                                      count is OK: the count itself bounds its error by cheb_tol
                                      (at tau = 1 the stopping test of a block with large SNPs,
                                      |r| <= cheb_tol (1 - tau) |x|, can never pass). */
};
/* A non-finite z (NaN, +Inf or -Inf in one z_s / z_l entry: a summary row whose beta is `nan` or
 * `inf`) is data, not an error.  It makes EVERY beta of its block non-finite in every copy, as the
 * reference's algebra does, and touches no other block: their betas, statuses and iteration counts
 * are bit for bit those of the run without it.  The status of such a block:
 *
 *   route                                            status              betas        iterations
 *   PCG (every kernel, 1 .. 4 copies)                NOT_CONVERGED (4)   non-finite   pcg_maxit
 *   factorisation, a factored copy (base, merged,    OK (0)              non-finite   -
 *     copy-split units, blocks of <= 63 SNPs)
 *   factorisation, an h2f copy iterated on the base  OK (0): it ran its  non-finite   the a priori
 *     factor (Chebyshev, CG, dbslmm_tcheb, fused)    a priori count                   count
 *     ... CG under a pcg_maxit below that count      NOT_CONVERGED (4)   non-finite   pcg_maxit
 *
 * (a NaN never passes a stopping test; the factorisation has no test to fail: the matrix is sound).
 * So a status of OK does not promise finite betas; dbslmm_plan_score drops such SNPs by its
 * !isfinite rule, dbslmm_plan_variance reads the matrix alone and is unchanged.
 *
 * Every stopping rule is relative, so the solve is exactly homogeneous in z: z -> c z with c = +-2^k
 * gives c beta bit for bit, the same statuses and the same iteration counts, as long as no z^2,
 * (c z)^2 or squared residual leaves the normal fp64 range (tests/test_z_edges.py). */

typedef struct dbslmm_ctx dbslmm_ctx;
typedef struct dbslmm_plan dbslmm_plan;

/* Path selection of a plan (the product has ONE numerical path per block size class; these
 * fields only move the size thresholds, e.g. so tests can drive every kernel class at small
 * sizes).  Zero-initialise for the defaults; every field's 0 means "default".
 *
 * tiled_min      blocks with m >= tiled_min take the multi-workgroup tiled factorisation
 *                (default 384, or 256 when no block reaches 512; minimum 64)
 * gram_big_min   blocks with m >= this use the 128 x 128-tile Gram kernel (default 96)
 * gram_huge_min  ... and the 256 x 256-tile one from here (default 384, 768 when n_ref < 4096)
 * h2f_mode       plan_run_multi: 0 = tiled blocks factored once, the other sigmas solved by
 *                Chebyshev iteration on that factor when the bound allows (tau in (0, 1],
 *                <= 60 iterations); 1 = one factorisation per sigma (the merged sequence)
 * cheb_tol       relative error target of the h2f copies iterated on the base copy's factor (default
 *                1e-9: four orders below the 1e-5 parity bar on beta, one below the reference PCG's
 *                own deviation from the exact solution (~1e-8)).  CG (the default h2f_iter) stops a
 *                block once |r| <= cheb_tol lambda_min(M_c) |x| (5.03 iterations per tiled block at
 *                config 4); Chebyshev runs its a priori count (7 at h2f 0.8 / 1 / 1.2), which is
 *                also CG's cap.  A run that only its number of sigmas (more than 4) keeps off the PCG
 *                route (solver 2, or solver 0 with every 1/(sigma n) >= 2) uses pcg_tol instead, so
 *                its results stay as accurate as those of a run of up to 4 sigmas
 * lead_min       tiled blocks with m >= lead_min form the lead group: their Gram tiles run first
 *                and their factorisation (the longest dependency chains) starts right after
 *                them, beside the rest of the Gram and the other blocks' factorisation (default
 *                max(1536, m_max / 8) when tiled blocks lie on both sides of it; < 0: no lead
 *                group, and the tiled sequence starts after the whole Gram instead of right
 *                after the tiled blocks' Gram tiles).  Scheduling only: the results are
 *                bit-identical either way.
 * large_cheb     plan_run_multi with Chebyshev h2f: the single-workgroup blocks (64 <= m+1, m
 *                below tiled_min) iterate on the base copy's factor too (0 = on when every such
 *                block fits the iteration kernel, ld <= 512; -1 = off: every copy factored)
 * cheb_fused     1 = all Chebyshev passes of a copy group in one persistent launch over every tiled
 *                block (experimental, bit-identical, slower at config 4; turns sub_split off);
 *                0 = one launch per pass
 * debug_delay_us testing only: a spin kernel of this many microseconds at the head of every
 *                concurrently running stream segment (the bulk trailing launches of each tiled
 *                sequence, the rest sequence, the main stream after the lead fork, the lead
 *                sequence), so a missing cross-stream dependency fails deterministically
 *                instead of by timing.  Results must be bit-identical to a run without it.
 * debug_stop     testing only: 1 = stop every run after the Gram (the block matrices then hold
 *                Sigma, dbslmm_plan_block_matrix); 0 = the full solve
 * sub_split      scheduling, plans with a lead group: 0 / 1 = the substitutions (backward solve and
 *                h2f Chebyshev passes) run per group -- the rest group's right after its own
 *                factorisation, beside the lead group's, on sub_grid_rest / sub_grid_lead
 *                persistent workgroups (default); -1 = one launch sequence over all tiled blocks
 *                after both factorisations.  Scheduling only: bit-identical results.
 *                2 = as 0 / 1, but the rest group's h2f copies iterate with one workgroup per
 *                block (every Chebyshev pass in one launch, dbslmm_tcheb; blocks up to 4096 SNPs,
 *                otherwise as 0): results within cheb_tol, not bit-identical to 0 / 1.
 * sub_grid_lead, sub_grid_rest   their persistent grids (0 = default: 5/16 of the CUs for
 *                the lead group, the other three quarters for the rest)
 * shard_copies   multi-device plans (dbslmm_ctx_create_multi): the number of h2f solves each
 *                run_multi call will request (0 / 1: single solves).  With K >= 2 and at least K
 *                devices the shard plan may split the K copies of the blocks whose dependency chain
 *                exceeds the fair share of the step into K (block, copy) units on distinct devices
 *                (dbslmm_shard_plan).  Any n_sigma still works: with n_sigma != K a split block is
 *                solved whole on the device of its copy 0.  Ignored by single-device plans.
 * h2f_iter       h2f_mode 0, the iterated copies (tiled and single-workgroup blocks): 1 = Chebyshev
 *                (a priori coefficients and iteration count), 2 = preconditioned CG on the same
 *                factor (Chronopoulos-Gear form, dbslmm_cg_update / dbslmm_chol_cheb): stops per
 *                block once |r| <= cheb_tol lambda_min(M_c) |x|,
 *                capped at the Chebyshev count K (2 q^K e_0 <= cheb_tol on an interval that does
 *                not depend on the data; CG's energy-norm error is at most Chebyshev's, so a copy
 *                that ran all K iterations is within the target and OK whether or not the stopping
 *                test passed -- with large SNPs and tau = 1 its bound is 0 and the block always
 *                runs K).  Only when pcg_maxit lowered the cap below K is a copy still above the
 *                bound there reported DBSLMM_BLOCK_NOT_CONVERGED; 0 = the default (2).  Both
 *                within cheb_tol; the base copy is bit-identical either way.  (cheb_fused = 1 and the whole-block rest
 *                group of sub_split = 2 iterate by Chebyshev.)
 * solver         how a run solves its blocks (ABI 12): 1 = factorisation (fp64 Cholesky of every
 *                block, the paths above); 2 = PCG: the reference's own algorithm (Jacobi-PCG,
 *                dbslmmfit.cpp:629-678) on the joint matrix of every block, all h2f copies as
 *                right-hand sides of one iteration, the LD matrix streamed from the Gram as exact
 *                integers (uint16; fp64 Sigma for blocks with missing calls or n_ref > 16383);
 *                0 = auto: PCG when every copy is well conditioned by its prior shift
 *                (1/(sigma_s n) >= 2, so that kappa <= ~6 and <= ~35 iterations), 0 < tau < 1
 *                (or no large SNPs), at most 4 copies and no debug_stop; the factorisation
 *                otherwise.  dbslmm_plan_variance needs the factor: after a PCG run it
 *                re-solves the latest sigma by factorisation first.
 * pcg_tol        PCG: relative error bound per block and copy, |x - x*| <= pcg_tol |x*| in the
 *                2-norm, enforced as |r| <= pcg_tol lambda |x| with lambda = 1/(sigma_s n) + 1 - tau
 *                (blocks without large SNPs) or 1 - tau, lower bounds of lambda_min that hold for
 *                any data (0 = default 1e-12)
 * pcg_maxit      PCG: iteration cap (0 = default 1000, the reference's maxiter); a copy still
 *                above its bound there is reported DBSLMM_BLOCK_NOT_CONVERGED with its iterate.
 *                Also lowers the cap of the factorisation route's h2f CG (h2f_iter 2) below its
 *                default, the Chebyshev count.
 * pcg_whole      PCG (ABI 15): blocks of at most 8 tile rows (1024 SNPs) on the uint16 Gram are
 *                solved whole by one workgroup per Krylov sequence (dbslmm_pcg_block) beside the
 *                chip-wide iterations of the others; 0 = default (on), -1 = off (every block on
 *                the chip-wide kernels: A/B and parity tests).  Results agree within pcg_tol.
 * stream_out     PCG route of dbslmm_plan_run_multi on one device (ABI 17): 1 (and 0, the default)
 *                = the kernels write every result to a host-visible pinned mirror as well as the
 *                device arrays and flag each block they finish (dbslmm_pcg_block at the end of a
 *                sequence, dbslmm_pcg_update when a chip-wide block has converged), and the calling
 *                thread copies finished blocks into the caller's arrays while the GPU still
 *                iterates (no device-to-host copy after the last kernel); -1 = off: the run is
 *                waited for and downloaded through the pinned staging buffer, as the
 *                factorisation route, plan_run + plan_download and multi-device contexts always
 *                are.  Bit-identical results either way.  (The Python binding passes an explicit
 *                stream_out = 0 as -1, so there 1 / 0 read on / off.)
 * pcg_block_wgs  PCG (ABI 19): at most this many workgroups of dbslmm_pcg_block (each takes its
 *                sequences from one counter, so the results are bit-identical for any value); 0 =
 *                default, one per compute unit (never more than there are sequences or compute
 *                units).
 */
typedef struct dbslmm_options {
    int32_t tiled_min;
    int32_t gram_big_min;
    int32_t gram_huge_min;
    int32_t h2f_mode;
    double cheb_tol;
    int32_t lead_min;
    int32_t large_cheb;
    int32_t cheb_fused;
    int32_t debug_delay_us;
    int32_t debug_stop;
    int32_t sub_split;
    int32_t sub_grid_lead;
    int32_t sub_grid_rest;
    int32_t shard_copies;
    int32_t h2f_iter;
    int32_t solver;
    double pcg_tol;
    int32_t pcg_maxit;
    int32_t pcg_whole;
    int32_t stream_out;
    int32_t pcg_block_wgs;
} dbslmm_options;

/* One LD-block problem set, the arguments of DBSLMMFIT::est in flat form.
 *
 * bed       the whole PLINK .bed image INCLUDING its 3 magic bytes (host memory); row r of
 *           SNP-major data starts at byte 3 + r*ceil(n_ref/4) (dtpr.cpp:302).
 * n_ref     individuals in the reference .fam (getRow, dbslmm.cpp:232).
 * n_obs     GWAS sample size (-n).
 * sigma_s   h / nsnp (dbslmm.cpp:332).
 * tau       LD shrinkage; the reference hard-codes 0.8 (dbslmmfit.cpp:697,751).
 * num_block number of LD blocks (addBlock's return, dtpr.cpp:455-481).
 * s_ptr     num_block+1 offsets; small SNPs of block b are s_pos[s_ptr[b]..s_ptr[b+1]) (bed
 *           rows, INFO::pos) with z-scores z_s[...] (INFO::z); order = the reference's
 *           info_s order.
 * l_ptr     same for large SNPs, or NULL for the LMM-only path.
 * opts      path-selection thresholds (dbslmm_options), or NULL for the defaults.
 */
typedef struct dbslmm_problem {
    const uint8_t* bed;
    int64_t bed_len;
    int32_t n_ref;
    int32_t n_obs;
    double sigma_s;
    double tau;
    int32_t num_block;
    const int64_t* s_ptr;
    const int32_t* s_pos;
    const double* z_s;
    const int64_t* l_ptr;
    const int32_t* l_pos;
    const double* z_l;
    const dbslmm_options* opts;
} dbslmm_problem;

/* Kernel timing slots reported by dbslmm_plan_kernel_ms. */
enum {
    DBSLMM_K_UNPACK = 0,      /* dbslmm_slot_stats: per-SNP statistics of the slots, gathered from
                                 the panel image's row table
                                 (the slot keeps the name of the unpack that used to run here) */
    DBSLMM_K_GRAM = 1,        /* dbslmm_gram_i8 / _big / _huge: FP4-MFMA grouped syrk of the exact
                                 integer dosages (raw 2-bit panel rows gathered, decoded and
                                 expanded on the fly) + fp64
                                 standardising epilogue (PCG route: the integer Gram as uint16) */
    DBSLMM_K_CHOL_LARGE = 2,  /* dbslmm_chol_large: blocks with 64 <= m+1 and m below the tiled
                                 threshold, one workgroup each */
    DBSLMM_K_CHOL_SMALL = 3,  /* dbslmm_chol_small: blocks with <= 63 SNPs, one wave each
                                 (concurrent with CHOL_LARGE when there are no tiled blocks) */
    DBSLMM_K_CHOL_TILED = 4,  /* dbslmm_tchol_*: blocks with m >= the tiled threshold
                                 (dbslmm_options.tiled_min; default 384, or 256 when no block
                                 reaches 512), many workgroups per block,
                                 one launch per panel phase (third stream); the whole sequence */
    DBSLMM_K_TRSV = 5,        /* dbslmm_trsv_fwd/bwd: h2f tuning's CG / Chebyshev iterations of the
                                 tiled blocks on the base copy's factor (run_multi; 0 otherwise) */
    DBSLMM_K_PCG = 6,         /* dbslmm_pcg_*: the PCG route's iterations (init to final; 0 on the
                                 factorisation route) */
    DBSLMM_K_PCG_BLOCK = 7,   /* dbslmm_pcg_block: the small blocks solved whole (ABI 14; runs on a
                                 second stream inside the K_PCG span) */
    DBSLMM_K_COUNT = 8
};

int dbslmm_abi_version(void);

/* Create a context on HIP device `device` (ordinal as seen by this process). */
int dbslmm_ctx_create(int device, dbslmm_ctx** out);

/* Create a context over n_dev HIP devices (ordinals; a device may repeat: several shards on one
 * GPU).  Replaces the reference's only parallelism, OpenMP over LD blocks
 * (scr/dbslmmfit.cpp:191-220), with one GPU per shard: plan_create assigns the work units --
 * (LD block, h2f copy) pairs, dbslmm_shard_plan with dbslmm_options.shard_copies -- to the devices,
 * uploads to each device only the .bed rows of its blocks, and every plan / est call then drives
 * all devices concurrently (one host thread per job) and returns beta, status and variance columns
 * in the caller's original order.  dbslmm_bed_maf splits its rows over the devices; read_snp_std
 * and valid_blocks run on the first device.  n_dev == 1 is dbslmm_ctx_create(device_ids[0]). */
int dbslmm_ctx_create_multi(int32_t n_dev, const int32_t* device_ids, dbslmm_ctx** out);
/* Shard plan (ABI 10): assign the work units of a problem -- (LD block, h2f copy) pairs -- to n_dev
 * devices.  m[b] = SNPs of block b (small + large), n_copies = h2f solves per run (1: single solves).
 * A block's copies stay on one device (one Gram, one factorisation, the other copies iterated on
 * it) unless the block's dependency chain exceeds the fair share of the step and n_dev >= n_copies:
 * then each copy is a unit of its own, factored directly, copy c on device c of a group of n_copies
 * devices (several split blocks may share a group: a device's split units are all of one copy and
 * are solved as one job, their chains together).  Whole blocks go to devices
 * longest-first by a time model of one MI355X (per-block chip time of each kernel class and the
 * block's chain alone).  Out: unit_device[b * n_copies + c] = the device index
 * of copy c of block b (-1: empty block); dev_ms (optional, n_dev entries) = the model's predicted
 * step of each device in ms.  Host-only (no GPU needed); deterministic.  Replaces the reference's
 * OpenMP schedule(dynamic) over blocks (scr/dbslmmfit.cpp:189-220). */
int dbslmm_shard_plan(int32_t num_block, const int32_t* m, int32_t n_ref, int32_t n_dev, int32_t n_copies,
                      int32_t* unit_device, double* dev_ms);
/* Shard plan of a problem (ABI 13): as dbslmm_shard_plan, for the route the problem's plans take
 * with these n_sigma sigmas (dbslmm_options.solver and the prior shift, as dbslmm_plan_run_multi
 * decides).  Factorisation route: dbslmm_shard_plan's model and units.  PCG route: whole blocks
 * only (every copy of a block on one device: one Krylov sequence serves the copies of a block
 * without large SNPs), longest first onto the least-loaded device by the PCG model (unpack + Gram
 * at the measured kernel rates, then per iteration the block's tiles and tile rows; a priori
 * iteration counts).  Outputs as dbslmm_shard_plan, n_copies = n_sigma.
 * Host-only; deterministic. */
int dbslmm_shard_plan_problem(const dbslmm_problem* p, const double* sigma_s, int32_t n_sigma, int32_t n_dev,
                              int32_t* unit_device, double* dev_ms);
/* A plan over ONE device's units of a shard plan (ABI 10), on a single-device context: the same
 * problem as dbslmm_plan_create (the whole .bed image and CSR arrays), solving only the units with
 * unit_device[b * n_copies + c] == device_index (its split units -- all of one h2f copy -- as one
 * job on a context of its own on the same GPU, so they run beside the device's whole blocks).  run_multi / download / variance write only
 * those units' entries of the caller's full-size arrays; everything else is left untouched, so
 * one process per GPU (bench.py under torch.distributed) solves its part and gathers the rest.
 * Run it with n_sigma == n_copies (otherwise a split block is solved whole by the device of its
 * copy 0). */
int dbslmm_plan_create_units(dbslmm_ctx* ctx, const dbslmm_problem* p, int32_t n_copies,
                             const int32_t* unit_device, int32_t device_index, dbslmm_plan** out);
/* Devices a context drives (1 for dbslmm_ctx_create). */
int dbslmm_ctx_num_devices(const dbslmm_ctx* ctx);
/* block_device[b] (num_block entries) = the device index (0 .. n_dev-1, in device_ids order) that
 * solves block b (its h2f copy 0 when the shard plan split its copies), -1 for an empty block (or,
 * on a units plan, a block none of whose units it solves); all 0 on a single-device context. */
int dbslmm_plan_shard_info(const dbslmm_plan* plan, int32_t* block_device);
void dbslmm_ctx_destroy(dbslmm_ctx* ctx);
const char* dbslmm_last_error(const dbslmm_ctx* ctx);
/* Keep a device copy of the caller's .bed image on the context (staged upload through pinned
 * buffers): dbslmm_bed_maf and dbslmm_plan_create calls that pass the same host range (bed,
 * bed_len) then read it instead of uploading again -- the reference reads the .bed once for the
 * MAF pass (IO::readBim, dtpr.cpp:93-102) and again per block in calcBlock (dbslmmfit.cpp:
 * 384-387).  The cached image is matched by host pointer and length only: the caller must not
 * modify the buffer, or free it and pass a new one at the same address, while it is cached
 * (call this again, or with bed == NULL, after any change).  The upload is kept verbatim until the
 * first call that supplies n_ref, which turns it into the row-aligned panel image the kernels read
 * (one resident copy either way; a later call with another n_ref uploads for itself).  A plan
 * created from the cached image reads it in place (no second device copy) and keeps it alive until
 * the plan is destroyed, even if the context releases or replaces it.  bed == NULL releases the context's reference.  A
 * multi-device context ignores the call (each device holds only its shard's rows). */
int dbslmm_ctx_cache_bed(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len);
/* dbslmm_ctx_cache_bed with the image read from an open file descriptor (pread straight into the
 * pinned staging buffers: the caller's pages of the file are never touched, so a caller that maps
 * the file pays no page faults and no page-table teardown for it).  `key` -- typically the
 * caller's mmap of the same file, never dereferenced here -- identifies the image: dbslmm_bed_maf
 * and dbslmm_plan_create calls that pass (key, bed_len) as their .bed read the cached copy.  The
 * cached copy serves ONE n_ref, that of the first such call (which turns the verbatim bytes into
 * the panel image and releases them): a later call that passes (key, bed_len) with another n_ref
 * returns DBSLMM_E_STATE -- dbslmm_last_error names the cached n_ref -- and does not read through
 * key; call this again (or dbslmm_ctx_cache_bed) to use the other n_ref.  The file must not change
 * while cached.  (ABI 8; the dbslmm CLI uses it.) */
int dbslmm_ctx_cache_bed_fd(dbslmm_ctx* ctx, int fd, int64_t bed_len, const uint8_t* key);

/* DBSLMMFIT::est replacement: upload, solve, download, free.  beta_s has s_ptr[num_block]
 * entries, beta_l l_ptr[num_block] (ignored when l_ptr == NULL); block_status (optional) has
 * num_block entries.  Blocking. */
int dbslmm_est(dbslmm_ctx* ctx, const dbslmm_problem* p, double* beta_s, double* beta_l,
               int32_t* block_status);

/* Split form.  plan_create copies the .bed image and block metadata into HBM and sizes the
 * workspace; plan_run enqueues the three kernels on the context's stream (asynchronous);
 * plan_sync waits; plan_download copies beta / status to the caller. */
int dbslmm_plan_create(dbslmm_ctx* ctx, const dbslmm_problem* p, dbslmm_plan** out);
int dbslmm_plan_run(dbslmm_plan* plan);
int dbslmm_plan_sync(dbslmm_plan* plan);
int dbslmm_plan_download(dbslmm_plan* plan, double* beta_s, double* beta_l, int32_t* block_status);
/* h2f tuning (replaces the three dbslmm runs of software/DBSLMM.R:204-219, -h = h2 * h2f):
 * one unpack + Gram, then for each sigma_s[i] one factorisation + solve; outputs are
 * n_sigma consecutive slices: beta_s[i * n_s ..], beta_l[i * n_l ..], block_status[i * num_block ..]
 * (NULL skips).  Synchronous.  The plan's own sigma_s is unchanged. */
int dbslmm_plan_run_multi(dbslmm_plan* plan, const double* sigma_s, int32_t n_sigma,
                          double* beta_s, double* beta_l, int32_t* block_status);

/* Change sigma_s (h2f tuning, software/DBSLMM.R:205-219) without re-uploading. */
int dbslmm_plan_set_sigma(dbslmm_plan* plan, double sigma_s);
void dbslmm_plan_destroy(dbslmm_plan* plan);

/* Kernel timing (HIP events recorded around each launch on the plan's stream).  Enable before
 * plan_run; after plan_sync, ms_out[k] = average duration in ms of kernel k over the runs since
 * enabling, launches_out = number of runs averaged. */
int dbslmm_plan_enable_timing(dbslmm_plan* plan, int enable);
int dbslmm_plan_kernel_ms(dbslmm_plan* plan, double* ms_out /*[DBSLMM_K_COUNT]*/, int32_t* launches_out);

/* Workload figures of the plan (for rooflines): [0] SNPs, [1] bytes read by the statistics
 * gather (per slot: its row position, the row's 16-byte table entry, its block id), [2] bytes it
 * writes (S, mean, 1/sd per slot and the blocks' missing-call flags), [3] Gram ops (2 per MAC, algorithmic
 * sum_b n_ref*m_b*(m_b+1)), [4] Gram ops as executed on padded tiles, [5] Cholesky+solve fp64
 * flops of the large blocks (sum_b m_b^3/3 + 2 m_b^2), [6] non-empty blocks, [7] gram tiles,
 * [8] the same fp64 flops for the small blocks, [9] large blocks, [10] the same fp64 flops for
 * the tiled blocks, [11] tiled blocks, [12] launches of the tiled sequence per run, [13] bytes of
 * the factor read by one substitution launch over the tiled blocks (64-row tiles), [14] Chebyshev
 * iterations of the latest run_multi (0: none; with CG their cap), [15] its base copy (-1: none),
 * [16] factor bytes its h2f passes read (CG: each tiled block's own iteration count),
 * [17] 1 when the latest run took the PCG route, [18] its iterations (the slowest block),
 * [19] the lower-triangle LD matrix bytes the chip-wide PCG kernels streamed in that run (in their
 * storage: uint16 integer Gram / fp64 Sigma; every block times its own iterations), [20] their
 * partial-sum bytes (written + read once), [21] the same matrix bytes of the blocks
 * dbslmm_pcg_block solved whole (ABI 14; before: per-iteration figures). */
#define DBSLMM_WORKLOAD_LEN 22
int dbslmm_plan_workload(const dbslmm_plan* plan, double* out /*[DBSLMM_WORKLOAD_LEN]*/);
/* PCG iterations of each block in the latest run (ABI 13): iters[b] (num_block entries) = the
 * iterations block b ran before its every copy met the stopping rule (pcg_maxit at the cap), 0 for
 * empty blocks and after a run on the factorisation route.  Waits for the run. */
int dbslmm_plan_block_iters(dbslmm_plan* plan, int32_t* iters);

/* Where each block's results lie in the caller's arrays (ABI 17; tests and diagnostics, host only:
 * no context, no GPU): the table a streamed run (dbslmm_options.stream_out) copies finished blocks
 * out by.  ranges receives one row of 5 per non-empty block, in block order -- {block, s0, s1, l0,
 * l1}: beta_s[s0 .. s1), beta_l[l0 .. l1) and status entry `block` -- and has room for num_block
 * rows; *n_ranges their number.  l_ptr NULL: no large SNPs.  DBSLMM_E_ARG when the offsets are not
 * monotone. */
int dbslmm_out_ranges(int32_t num_block, const int64_t* s_ptr, const int64_t* l_ptr, int64_t* ranges,
                      int32_t* n_ranges);

/* Diagnostics (parity tests): after plan_sync, the working matrix of block `block` (original
 * block id) in factorisation copy `copy`: ld x ld fp64, row-major, ld = *ld_out (out == NULL:
 * only ld).  Layout: rows / columns [small | large | z row m | padding];
 * after a debug_stop = 1 run the lower triangle (i < m, j <= i) holds Sigma (no 1/(sigma_s n)
 * shift); after a full run of a block on the multi-workgroup path (m >= tiled_min) the strict
 * lower triangle holds L (M = L L^T), row m holds y = L^{-1} z, and each 64 x 64 diagonal tile's
 * diagonal and upper triangle hold its inverse transposed.  Synchronous.  (ABI 9) */
int dbslmm_plan_block_matrix(dbslmm_plan* plan, int32_t block, int32_t copy, double* out,
                             int32_t* ld_out);

/* Test-set variance (the `diags` matrix DBSLMMFIT::est saves to variance.txt,
 * scr/dbslmmfit.cpp:116,191-214,242; calcBlock :366-626 with calc_nt_by_nt_matrix,
 * scr/calc_asymptotic_variance.cpp:22-137).  The test panel is a PLINK .bed image of n_total
 * individuals; indicator[0..n_total) selects the test individuals (nonzero; readSNPIm,
 * dtpr.cpp:285-364); s_pos / l_pos give each small / large SNP of the plan (same order and
 * length as the problem's s_pos / l_pos, l_pos NULL when the plan has no large SNPs) its row
 * in the test .bed (calcBlock's positional test_info_s_block[i].pos).
 */
typedef struct dbslmm_test_panel {
    const uint8_t* bed;
    int64_t bed_len;
    int32_t n_total;
    const int32_t* indicator;
    const int32_t* s_pos;
    const int32_t* l_pos;
} dbslmm_test_panel;

/* After plan_run / plan_run_multi (uses the factorisation of the most recent sigma_s):
 * diags is n_test x num_block column-major, n_test = number of indicator entries equal to 1;
 * column b = diag(X_l var_bl X_l^T + X_s var_bs X_s^T) of block b, zeros for a block without
 * SNPs (a block of large SNPs only: x_l^T Sigma_ll^-1 x_l / n), NaN for a block whose status is
 * NOT_PD / MONOMORPHIC and, as in the reference, for a block with a test SNP that has no variance
 * or no observed call among the selected individuals.  Synchronous; host buffers.
 * n_test_out (optional) receives n_test. */
int dbslmm_plan_variance(dbslmm_plan* plan, const dbslmm_test_panel* test, double* diags,
                         int32_t* n_test_out);

/* Polygenic scores of a target panel from the betas of the latest run (ABI 18): what the reference
 * leaves to `plink --score <eff>.txt 1 2 4 sum` (Rmd/Manual.Rmd:176-188), once per h2f factor
 * (software/DBSLMM.R:204-219, software/TUNE.R), computed on the device for every copy of the run in
 * one pass over the 2-bit panel (score.hip).
 *
 * The panel is a dbslmm_test_panel; indicator == NULL selects all n_total individuals.  Per SNP j
 * of the plan, over the selected individuals: dosage 00 -> 2, 10 -> 1, 11 -> 0, 01 -> missing; mu_j
 * = mean of the observed dosages; a missing call takes mu_j (readSNPIm, scr/dtpr.cpp:358-360 =
 * PLINK's mean imputation); sd_j = N-1 standard deviation of the imputed dosages (nomalizeVec).
 * A flip flag replaces g by 2 - g (a panel whose A1 is the other allele); w defaults to 1.
 *   DBSLMM_SCORE_COUNTS  score[c][t] = sum_j beta_jc w_j g'_tj          (w_j = 1/sqrt(2 maf (1-maf)):
 *                        column 4 of the effect file times allele counts, `--score 1 2 4 sum`)
 *   DBSLMM_SCORE_STD     score[c][t] = sum_j beta_jc w_j (g'_tj - mu'_j) / sd_j  (the predicted value
 *                        whose variance dbslmm_plan_variance returns)
 * A SNP contributes 0 to copy c and is counted in dropped[c] when its block's status for that copy
 * is NOT_PD / MONOMORPHIC, beta_jc w_j is not finite, no selected call is observed, or (STD) sd_j
 * is 0 or n_test < 2.  NOT_CONVERGED blocks contribute their iterate, as the effect file does.
 *
 * chunk_slots  the plan's slots are summed in runs of this many (0 = the library's constant, 512; a
 *              value between two multiples of 4 acts as the next multiple), the runs then in order: results are bit-identical from run to run and from device to
 *              device for a given plan and chunk_slots.  A multi-device context adds its shards'
 *              scores on the host in shard order, so across device counts scores agree to rounding
 *              (2 (M + 64) 2^-53 sum_j |a_j| (|g_tj| + |mu_j|), M SNPs), not bit for bit; a units
 *              plan returns its own units' contribution (zeros elsewhere): the caller adds the ranks.
 */
enum { DBSLMM_SCORE_COUNTS = 0, DBSLMM_SCORE_STD = 1 };
typedef struct dbslmm_score_args {
    int32_t mode;            /* DBSLMM_SCORE_COUNTS / DBSLMM_SCORE_STD */
    int32_t chunk_slots;     /* 0 = the library's constant; tests and A/B runs set it */
    const double* w_s;       /* per small SNP, NULL = 1 */
    const double* w_l;       /* per large SNP, NULL = 1 */
    const uint8_t* flip_s;   /* per small SNP, NULL = none */
    const uint8_t* flip_l;   /* per large SNP, NULL = none */
} dbslmm_score_args;
/* args NULL: counts, defaults.  n_copies must equal the copies of the latest run (1 after plan_run,
 * n_sigma after plan_run_multi); scores = n_copies slices of n_test (n_test_out, the selected
 * individuals in .fam order); dropped (optional) n_copies entries; gpu_ms (optional) = the event
 * time of the scoring kernels (a multi-device context: its slowest shard).  Finishes a pending run
 * first; reads the device betas and statuses and changes neither.  DBSLMM_E_STATE before any run,
 * after a debug_stop run, and after dbslmm_plan_variance had to re-solve the latest sigma (its
 * re-solve overwrites the device results of copy 0): score before the variance, or run again. */
int dbslmm_plan_score(dbslmm_plan* plan, const dbslmm_test_panel* test, const dbslmm_score_args* args,
                      int32_t n_copies, double* scores, int32_t* dropped, int32_t* n_test_out,
                      double* gpu_ms);

/* MAF pass: maf[r] for every bed row r < n_snp (readSNPIm with an all-ones indicator). */
int dbslmm_bed_maf(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                   int64_t n_snp, double* maf);

/* The row table of the panel image (ABI 16; tests and diagnostics): out[3 r .. 3 r + 2] = the exact
 * integers {dosage sum, sum of squared dosages, missing calls} of bed row r < n_rows over the
 * n_ref individuals -- what the image keeps per row and every per-row statistic (the plans' S, mean
 * and 1/sd, bed_maf, read_snp_std, valid_blocks) derives from.  Pad bits of a row's last byte never
 * count.  Same panel-key rules as dbslmm_bed_maf (the context's cached image when (bed, bed_len)
 * is its key, else an upload of its own); a multi-device context answers from its first device. */
int dbslmm_bed_row_stats(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                         int64_t n_rows, int32_t* out /* n_rows x 3: sum, sumsq, nmiss */);

/* LD r2 between rows of the reference panel (ABI 20; clump.hip).  r_ij is the Pearson correlation
 * of the dosages of bed rows i and j over the n_ref individuals, missing calls at the row mean
 * (readSNPIm's convention; the correlation of the standardised columns dbslmm_read_snp_std returns).
 * Pairs of rows without a missing call are computed from exact integers: r2 = N^2 / (D_i D_j) with
 * N = n G_ij - S_i S_j and D_i = n sq_i - S_i^2 formed in int64 and three fp64 roundings.  A row
 * without variance or without an observed call has r2 = NaN with every row, itself included.
 * Both entries follow the panel-key rules of dbslmm_bed_maf (the context's cached image when
 * (bed, bed_len) is its key, else an upload of their own); a multi-device context answers from its
 * first device.  DBSLMM_E_ARG for a pos outside the panel or n_ref past the FP4 Gram's exact range
 * (9 * roundup(n_ref, 256) < 2^24: n_ref <= 1 863 936).
 *
 * r2 of every pair of bed rows pos[0..n_rows): n_rows x n_rows fp64, row-major, symmetric; NaN in
 * the row and column of a row without variance or observed call.  n_rows <= 8192. */
int dbslmm_ld_r2(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                 const int32_t* pos, int32_t n_rows, double* r2);

/* Clumping: PLINK's greedy rule (`--clump-p1` candidates only; DBSLMM uses nothing but the index
 * SNPs, which `--clump-p2` cannot change).  The candidates -- bed row pos[k], chromosome code chr[k]
 * (any integer per chromosome), base pair bp[k] -- come in priority order, most significant first.
 * Walking them in that order, a candidate not yet absorbed becomes an index SNP and absorbs every
 * not yet absorbed candidate j on its chromosome with |bp_j - bp_k| <= window_bp and r2_kj >= r2.
 * Absorption is not transitive: if A absorbs B and C is linked only to B, C becomes an index SNP of
 * its own.  NaN compares false: a row without variance or observed call neither absorbs nor is
 * absorbed.  r2 is the dosage correlation above, not PLINK's haplotype-frequency estimate, and PLINK
 * documents neither its treatment of r2 exactly at the threshold nor of p-value ties: the index set
 * is this rule's, not a replay of a PLINK run.
 * r2 in (0, 1], window_bp >= 0, else DBSLMM_E_ARG. */
typedef struct dbslmm_clump_args { double r2; int64_t window_bp; } dbslmm_clump_args;
/* Candidates in priority order (most significant first).  index_of[k] = the candidate that
 * absorbed k (k itself for an index SNP); n_index (optional); gpu_ms (optional) = event time of
 * the tile kernel.  n_cand == 0 is valid.  Rows may repeat (a repeat has r2 = 1 with its twin). */
int dbslmm_clump(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, int32_t n_cand,
                 const int32_t* pos, const int32_t* chr, const int64_t* bp,
                 const dbslmm_clump_args* args, int32_t* index_of, int32_t* n_index, double* gpu_ms);

/* LD scores (ABI 21; ldscore.hip): what the reference's manual leaves to LDSC (Rmd/Manual.Rmd:170).
 * The listed rows -- bed row pos[k], chromosome code chr[k] (any integer per chromosome), base pair
 * bp[k] -- come in any order and may repeat.  window_bp >= 0.
 *   l2[k] = sum over the listed j with chr[j] == chr[k] and |bp[j] - bp[k]| <= window_bp (j = k
 *           included) of t_kj
 * r2_kj is exactly dbslmm_ld_r2's quantity (missing calls at the row mean, n = n_ref).  With
 * unbiased != 0 (args == NULL: unbiased, window 1 Mb) t = r2 - (1 - r2) / (n_ref - 2), ldsc's
 * adjustment, which needs n_ref > 2 (else DBSLMM_E_ARG); with unbiased == 0 t = r2.  A row whose r2
 * is NaN (no variance or no observed call) gets l2 = NaN and contributes nothing to any other row.
 * n_window[k] (optional) = the number of listed j inside the window of k, k itself and NaN rows
 * included: a pure position count.  gpu_ms (optional) = event time of the tile and reduce kernels.
 * The tile list is processed in slices of at most max_tiles_per_launch 128 x 128 tiles (0 = the
 * default, which keeps the partial-sum buffer at 256 MiB); l2 is bit-identical for every slice
 * size and from run to run (no atomics; the order is fixed, ldscore.hip).  The n_ref cap is the FP4
 * Gram's (dbslmm_ld_r2); n_rows == 0 is valid and n_rows has no 8192 limit.  Panel-key rules of
 * dbslmm_bed_maf; a multi-device context answers from its first device. */
typedef struct dbslmm_l2_args { int64_t window_bp; int32_t unbiased; int32_t max_tiles_per_launch; } dbslmm_l2_args;
int dbslmm_ld_scores(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref, int32_t n_rows,
                     const int32_t* pos, const int32_t* chr, const int64_t* bp, const dbslmm_l2_args* args,
                     double* l2, int32_t* n_window, double* gpu_ms);

/* LD score regression (ABI 21; ldsc_fit.hpp, which states the rule in full).  Host-only: no context,
 * no GPU.  chi2[j] = z_j^2, n_obs[j] = N_j, l2[j] the LD score of SNP j < n (all finite), m = the
 * number of SNPs the LD scores stand for.  fixed_intercept != 0 holds the intercept at `intercept`;
 * n_blocks = jackknife blocks (0 = 200; else >= 2); chisq_max > 0 drops the SNPs with chi2 above it
 * first (0 = off: no filter by default).  args == NULL: free intercept and the defaults.
 * Returns DBSLMM_E_ARG for null arrays, m <= 0 or n_blocks == 1 or < 0; else DBSLMM_OK with
 * out->status: DBSLMM_LDSC_OK, DBSLMM_LDSC_TOO_FEW (fewer SNPs than twice the parameters) or
 * DBSLMM_LDSC_SINGULAR (normal equations of the fit or of a delete-one block; e.g. every x equal
 * with a free intercept); the estimates are NaN unless OK.  intercept_se is 0 when fixed. */
enum { DBSLMM_LDSC_OK = 0, DBSLMM_LDSC_TOO_FEW = 1, DBSLMM_LDSC_SINGULAR = 2 };
typedef struct dbslmm_ldsc_args { double intercept; double chisq_max; int32_t fixed_intercept; int32_t n_blocks; } dbslmm_ldsc_args;
typedef struct dbslmm_ldsc_result {
    double h2, h2_se, intercept, intercept_se, mean_chi2;
    int64_t n_used;
    int32_t status;
} dbslmm_ldsc_result;
int dbslmm_ldsc_fit(int64_t n, const double* chi2, const double* n_obs, const double* l2, double m,
                    const dbslmm_ldsc_args* args, dbslmm_ldsc_result* out);

/* Association scan (ABI 22; assoc.hip, assoc_fit.hpp states the model in full): the summary
 * statistics of a training panel -- per SNP row a linear model of each phenotype on the row's
 * mean-imputed dosage, the intercept and the covariates, with a Wald test: the 11-column GEMMA
 * *.assoc.txt the reference's workflow starts from.
 *   keep    n_total flags (null: all); an individual is in the sample S when its flag is non-zero and
 *           all of its phenotypes and covariates are finite.  n = |S|, c = n_covar + 1 (the intercept
 *           is added by the library), df = n - c - 1 >= 1.
 *   pheno   n_total x n_pheno, covar n_total x n_covar (null when n_covar = 0), row-major fp64.
 *   chunk_indiv   individuals per chunk of the fixed-order reduction: a multiple of 64; 0 = the
 *           library's constant (4096).  The same call with the same chunk_indiv gives the same bits on
 *           every run; a row's result does not depend on the other rows of the call.
 * rows (null: 0 .. n_rows - 1) lists bed rows in any order, repeats allowed.  Outputs: n_mis, n_obs,
 * status [n_rows] int32; af [n_rows]; beta, se, tstat, p [n_pheno x n_rows] fp64.  For a status other
 * than DBSLMM_ASSOC_OK beta, se, tstat and p are NaN (af too without an observed call); the integers are
 * always reported.  prod_d / prod_m (optional, both or neither) [n_rows x (n_covar + n_pheno)]: the raw
 * products of the row's observed dosages / missing-call mask with the columns [Q_1 .. | Yr] of the
 * residualised design (tests, diagnostics).  gpu_ms (optional) = event time of the kernels.
 * DBSLMM_E_ARG for n_pheno < 1, df < 1, a rank-deficient covariate matrix, a chunk_indiv that is
 * negative or no multiple of 64, or a row outside the panel.  Mixed models, logistic models and
 * per-trait sample masks are out of scope.  Panel-key rules of dbslmm_bed_maf; a multi-device context
 * runs the scan on its first device. */
enum { DBSLMM_ASSOC_OK = 0, DBSLMM_ASSOC_NO_CALL = 1, DBSLMM_ASSOC_MONOMORPHIC = 2, DBSLMM_ASSOC_COLLINEAR = 3 };
typedef struct dbslmm_assoc_args {
    const uint8_t* keep;
    const double* pheno;
    const double* covar;
    int32_t n_pheno;
    int32_t n_covar;
    int32_t chunk_indiv;
} dbslmm_assoc_args;
int dbslmm_assoc(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_total, int32_t n_rows,
                 const int32_t* rows, const dbslmm_assoc_args* args, int32_t* n_mis, int32_t* n_obs, double* af,
                 double* beta, double* se, double* tstat, double* p, int32_t* status, double* prod_d,
                 double* prod_m, double* gpu_ms);

/* The finish of dbslmm_assoc on the host (no context, no GPU): row j has the counts n1[j], n2[j],
 * nm[j] over n individuals and the products t[j x (n_covar + n_pheno) ..] of its mean-imputed dosages
 * with [Q_1 .. | Yr]; yy [n_pheno] = |Yr_p|^2.  Outputs as dbslmm_assoc's.  DBSLMM_E_ARG for null
 * arrays, n_pheno < 1, n_covar < 0 or n - n_covar - 2 < 1. */
int dbslmm_assoc_stat_host(int64_t n, int32_t n_covar, int32_t n_pheno, int32_t n_rows, const int32_t* n1,
                           const int32_t* n2, const int32_t* nm, const double* t, const double* yy,
                           int32_t* n_obs, double* af, double* beta, double* se, double* tstat, double* p,
                           int32_t* status);

/* 2 P(t_df <= -|t|) through the regularised incomplete beta function (host only).  *p_out = NaN for a
 * non-finite t or df or df <= 0; DBSLMM_E_ARG for a null p_out. */
int dbslmm_student_t_two_sided(double t, double df, double* p_out);

/* readSNPIm + nomalizeVec for rows pos[0..n_rows): out is n_ref x n_rows column-major fp64
 * (column j = standardised dosages of bed row pos[j]); maf (optional) n_rows entries. */
int dbslmm_read_snp_std(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                        const int32_t* pos, int32_t n_rows, double* out, double* maf);

/* External-validation R^2 terms: the per-block loop of the `valid` tool (replaces the
 * Armadillo products of scr/validate.cpp:221-257).  Block b owns .bed rows pos[ptr[b]..ptr[b+1])
 * with weights z1 (DBSLMM beta) and z2 (external z):
 *   nume[b] = z1 . z2,   deno[b] = z1^T (X^T X / n_ref) z1 = |X z1|^2 / n_ref
 * X = the nomalizeVec-standardised reference genotypes (N-1 sd, missing calls at the mean);
 * a monomorphic SNP gives NaN, as the reference's 0/0 column.  Any num_block >= 0 (not bound by
 * the device's grid limits); rows may repeat, in any order.  Synchronous; host buffers. */
int dbslmm_valid_blocks(dbslmm_ctx* ctx, const uint8_t* bed, int64_t bed_len, int32_t n_ref,
                        int32_t num_block, const int64_t* ptr, const int32_t* pos,
                        const double* z1, const double* z2, double* nume, double* deno);

#ifdef __cplusplus
}
#endif
#endif /* DBSLMM_HIP_H_ */

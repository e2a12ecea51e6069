"""dbslmm_amd -- MI355X-native per-LD-block effect-size solver of DBSLMM.

Python front-end over the C-ABI library ``libdbslmm_hip.so`` (include/dbslmm_hip.h).  The
entry points mirror the reference operator interface (fboehm/DBSLMM, scr/dbslmmfit.hpp):

* ``DBSLMMFIT.est(...)``  -- DBSLMMFIT::est, both overloads (dbslmmfit.hpp:38-66): large +
  small effects, or LMM-only when no large SNPs are given.
* ``Plan``                -- the same problem kept resident in HBM for repeated solves.
* ``bed_maf``             -- the MAF pass of IO::readBim (dtpr.cpp:93-102).
* ``read_snp_std``        -- IO::readSNPIm + SNPPROC::nomalizeVec for a list of rows.
* ``clump``               -- the index SNPs of a candidate list by PLINK's greedy clumping rule on the
  reference panel (software/DBSLMM.R:139-145), ``ld_r2`` the dense r2 matrix of a list of rows.
* ``ld_scores``           -- the LD scores of listed panel rows, ``ldsc_h2`` the LD score regression on
  them: the heritability the reference takes from an LDSC run (Rmd/Manual.Rmd:170).
* ``assoc``               -- the association scan of a training panel: the per-SNP linear model with
  a Wald test whose output (a GEMMA ``*.assoc.txt``) the reference's workflow starts from.
* ``Plan.score``          -- the polygenic scores of a target panel for every h2f copy of the latest
  run (what the reference leaves to ``plink --score``), ``tune_r2`` the R2 index of TUNE.R on them.
* ``Context.row_stats``   -- the exact per-row integers (sum, sum of squares, missing calls) the
  resident panel image keeps and every per-row statistic derives from (tests, diagnostics).

All compute runs on the GPU through the HIP library; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (WORKLOAD_LEN, BLOCK_EMPTY, BLOCK_MONOMORPHIC, BLOCK_NOT_CONVERGED, BLOCK_NOT_PD,
                   BLOCK_OK, KERNEL_NAMES, SOLVER_AUTO, SOLVER_FACTOR, SOLVER_PCG, DbslmmError)

__all__ = ["Context", "Plan", "DBSLMMFIT", "BlockProblem", "bed_maf", "read_snp_std", "valid_blocks", "tune_r2", "ld_r2", "clump", "ld_scores", "ldsc_h2", "assoc", "assoc_stat_host", "student_t_two_sided",
           "DbslmmError", "BLOCK_OK", "BLOCK_EMPTY", "BLOCK_NOT_PD", "BLOCK_MONOMORPHIC",
           "BLOCK_NOT_CONVERGED", "KERNEL_NAMES", "SOLVER_AUTO", "SOLVER_FACTOR", "SOLVER_PCG"]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One HIP device (dbslmm_ctx_create), or several (a list of ordinals, repeats allowed:
    dbslmm_ctx_create_multi -- every plan's LD blocks are sharded over the devices)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = np.ascontiguousarray(device, dtype=np.int32)
            rc = self.lib.dbslmm_ctx_create_multi(len(ids), _ptr(ids), C.byref(h))
        else:
            rc = self.lib.dbslmm_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise DbslmmError(f"dbslmm_ctx_create(device={device}) failed rc={rc}")
        self.h = h
        self.device = device

    @property
    def num_devices(self) -> int:
        return int(self.lib.dbslmm_ctx_num_devices(self.h))

    def cache_bed(self, bed):
        """Keep a device copy of this .bed image (dbslmm_ctx_cache_bed); bed_maf / plan_create on
        the same array then skip their upload (a plan reads the cached image in place).  The
        array is matched by address and length only: do not modify it while it is cached (call
        cache_bed again after a change).  None releases it."""
        if bed is None:
            self._cached_bed = None
            self.check(self.lib.dbslmm_ctx_cache_bed(self.h, None, 0), "ctx_cache_bed")
            return
        b = np.ascontiguousarray(bed, dtype=np.uint8)
        self.check(self.lib.dbslmm_ctx_cache_bed(self.h, _ptr(b), b.size), "ctx_cache_bed")
        self._cached_bed = b       # the host range must stay alive and unchanged

    def row_stats(self, bed, n_ref: int, n_rows: int) -> np.ndarray:
        """The panel image's row table (dbslmm_bed_row_stats): an (n_rows, 3) int32 array of the
        exact per-row dosage sum, sum of squares and missing-call count."""
        b = np.ascontiguousarray(bed, dtype=np.uint8)
        out = np.zeros((n_rows, 3), dtype=np.int32)
        self.check(self.lib.dbslmm_bed_row_stats(self.h, _ptr(b), b.size, n_ref, n_rows, _ptr(out)),
                   "bed_row_stats")
        return out

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.dbslmm_last_error(self.h).decode(errors="replace")
            raise DbslmmError(f"{what} failed rc={rc}: {msg}")

    def close(self):
        if self.h:
            self.lib.dbslmm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class BlockProblem:
    """Flat form of DBSLMMFIT::est's arguments (see include/dbslmm_hip.h dbslmm_problem)."""
    bed: np.ndarray            # uint8 .bed image incl. magic
    n_ref: int
    n_obs: int
    sigma_s: float
    s_ptr: np.ndarray          # int64 [num_block+1]
    s_pos: np.ndarray          # int32 bed rows
    z_s: np.ndarray            # float64
    l_ptr: np.ndarray | None = None
    l_pos: np.ndarray | None = None
    z_l: np.ndarray | None = None
    tau: float = 0.8
    # dbslmm_options (path-selection thresholds; missing keys = the library defaults):
    # tiled_min, gram_big_min, gram_huge_min, h2f_mode (0 auto / 1 merged), cheb_tol, lead_min,
    # ..., solver (0 auto / 1 factorisation / 2 PCG), pcg_tol, pcg_maxit, stream_out (PCG route of
    # run_multi: 1 = results copied out block by block while the GPU iterates, the default; 0 = the
    # download after the run)
    opts: dict = field(default_factory=dict)

    def __post_init__(self):
        self.bed = np.ascontiguousarray(self.bed, dtype=np.uint8)
        self.s_ptr = np.ascontiguousarray(self.s_ptr, dtype=np.int64)
        self.s_pos = np.ascontiguousarray(self.s_pos, dtype=np.int32)
        self.z_s = np.ascontiguousarray(self.z_s, dtype=np.float64)
        if self.l_ptr is not None:
            self.l_ptr = np.ascontiguousarray(self.l_ptr, dtype=np.int64)
            self.l_pos = np.ascontiguousarray(self.l_pos, dtype=np.int32)
            self.z_l = np.ascontiguousarray(self.z_l, dtype=np.float64)
        nb = len(self.s_ptr) - 1
        if self.l_ptr is not None and len(self.l_ptr) != nb + 1:
            raise ValueError("s_ptr and l_ptr must have the same number of blocks")

    @property
    def num_block(self) -> int:
        return len(self.s_ptr) - 1

    @property
    def n_s(self) -> int:
        return int(self.s_ptr[-1])

    @property
    def n_l(self) -> int:
        return 0 if self.l_ptr is None else int(self.l_ptr[-1])

    def c_struct(self) -> _lib.Problem:
        unknown = set(self.opts) - {f[0] for f in _lib.Options._fields_}
        if unknown:
            raise ValueError(f"unknown dbslmm_options fields: {sorted(unknown)}")
        o = dict(self.opts)
        if "stream_out" in o and int(o["stream_out"]) == 0:
            o["stream_out"] = -1                   # here 1 / 0 read on / off (the struct's 0 is "default": on)
        self._opts = _lib.Options(**o)             # kept alive with the problem
        return _lib.Problem(
            _ptr(self.bed), self.bed.size, self.n_ref, self.n_obs, self.sigma_s, self.tau,
            self.num_block, _ptr(self.s_ptr), _ptr(self.s_pos), _ptr(self.z_s),
            _ptr(self.l_ptr), _ptr(self.l_pos), _ptr(self.z_l), C.pointer(self._opts))


class Plan:
    """A BlockProblem resident in HBM (dbslmm_plan_*)."""

    def __init__(self, ctx: Context, prob: BlockProblem):
        self.ctx, self.prob = ctx, prob
        self._cs = prob.c_struct()          # keep the struct (and arrays) alive
        h = C.c_void_p()
        ctx.check(ctx.lib.dbslmm_plan_create(ctx.h, C.byref(self._cs), C.byref(h)), "plan_create")
        self.h = h

    @classmethod
    def units(cls, ctx: Context, prob: BlockProblem, unit_device, device_index: int):
        """dbslmm_plan_create_units: the (block, h2f copy) units of `prob` that a shard plan
        (dist.shard_units -> unit_device [num_block, n_copies]) gives device `device_index`, on
        this single-device context.  run_multi(sigmas) with len(sigmas) == n_copies writes only
        those units' entries of the full-size outputs."""
        self = cls.__new__(cls)
        self.ctx, self.prob = ctx, prob
        ud = np.ascontiguousarray(unit_device, dtype=np.int32)
        if ud.ndim != 2 or ud.shape[0] != prob.num_block:
            raise ValueError("unit_device: [num_block, n_copies]")
        self._cs = prob.c_struct()
        self._ud = ud
        h = C.c_void_p()
        ctx.check(ctx.lib.dbslmm_plan_create_units(ctx.h, C.byref(self._cs), ud.shape[1], _ptr(ud),
                                                   int(device_index), C.byref(h)), "plan_create_units")
        self.h = h
        return self

    def run(self):
        self.ctx.check(self.ctx.lib.dbslmm_plan_run(self.h), "plan_run")
        self._run_copies = 1

    def sync(self):
        self.ctx.check(self.ctx.lib.dbslmm_plan_sync(self.h), "plan_sync")

    def set_sigma(self, sigma_s: float):
        self.ctx.check(self.ctx.lib.dbslmm_plan_set_sigma(self.h, float(sigma_s)), "plan_set_sigma")

    def run_multi(self, sigmas, out=None):
        """h2f tuning: one unpack + Gram, one solve per sigma_s -> [(beta_s, beta_l, status)].
        out: optional (beta_s, beta_l, status) arrays of shapes (n, n_s), (n, n_l), (n, num_block)
        to write into (a caller that solves repeatedly reuses its buffers)."""
        p = self.prob
        sig = np.ascontiguousarray(sigmas, dtype=np.float64)
        n = len(sig)
        if out is not None:
            bs, bl, st = out
            if (bs.shape != (n, p.n_s) or bl.shape != (n, p.n_l) or st.shape != (n, p.num_block)
                    or bs.dtype != np.float64 or bl.dtype != np.float64 or st.dtype != np.int32
                    or not all(a.flags.c_contiguous for a in out)):
                raise ValueError("out: C-contiguous float64 (n, n_s), (n, n_l) and int32 (n, num_block)")
        else:
            bs = np.zeros((n, p.n_s))
            bl = np.zeros((n, p.n_l))
            st = np.zeros((n, p.num_block), dtype=np.int32)
        self.ctx.check(self.ctx.lib.dbslmm_plan_run_multi(self.h, _ptr(sig), n, _ptr(bs), _ptr(bl),
                                                          _ptr(st)), "plan_run_multi")
        self._run_copies = n
        return [(bs[i], bl[i], st[i]) for i in range(n)]

    def enable_timing(self, on: bool = True):
        self.ctx.check(self.ctx.lib.dbslmm_plan_enable_timing(self.h, int(on)), "plan_enable_timing")

    def kernel_ms(self):
        out = np.zeros(len(KERNEL_NAMES))
        n = np.zeros(1, dtype=np.int32)
        self.ctx.check(self.ctx.lib.dbslmm_plan_kernel_ms(self.h, _ptr(out), _ptr(n)), "plan_kernel_ms")
        return out, int(n[0])

    def workload(self) -> dict:
        w = np.zeros(WORKLOAD_LEN)
        self.ctx.check(self.ctx.lib.dbslmm_plan_workload(self.h, _ptr(w)), "plan_workload")
        keys = ("snps", "unpack_read_bytes", "unpack_write_bytes", "gram_ops_alg",
                "gram_ops_exec", "chol_flops_large", "blocks", "gram_tiles", "chol_flops_small",
                "blocks_large", "chol_flops_tiled", "blocks_tiled", "tiled_launches", "trsv_bytes",
                "cheb_iters", "cheb_base", "h2f_pass_bytes", "pcg_route", "pcg_iters", "pcg_chip_bytes",
                "pcg_partial_bytes", "pcg_block_bytes")
        return dict(zip(keys, w.tolist()))

    def block_iters(self) -> np.ndarray:
        """PCG iterations of each block in the latest run (dbslmm_plan_block_iters; 0: empty block
        or the factorisation route)."""
        out = np.zeros(max(1, self.prob.num_block), dtype=np.int32)
        self.ctx.check(self.ctx.lib.dbslmm_plan_block_iters(self.h, _ptr(out)), "plan_block_iters")
        return out[:self.prob.num_block]

    def shard_info(self) -> np.ndarray:
        """Device index (in the context's device order) solving each block; -1 = empty block."""
        out = np.zeros(self.prob.num_block, dtype=np.int32)
        self.ctx.check(self.ctx.lib.dbslmm_plan_shard_info(self.h, _ptr(out)), "plan_shard_info")
        return out

    def block_matrix(self, block: int, copy: int = 0) -> np.ndarray:
        """Diagnostics (dbslmm_plan_block_matrix): block `block`'s ld x ld working matrix of
        factorisation copy `copy` after the last run -- Sigma after a debug_stop = 1 run, the
        factor (strict lower L, row m = L^-1 z) after a full run of a tiled block."""
        ld = C.c_int32()
        self.ctx.check(self.ctx.lib.dbslmm_plan_block_matrix(self.h, int(block), int(copy), None,
                                                             C.byref(ld)), "plan_block_matrix")
        out = np.empty((ld.value, ld.value))
        self.ctx.check(self.ctx.lib.dbslmm_plan_block_matrix(self.h, int(block), int(copy), _ptr(out),
                                                             None), "plan_block_matrix")
        return out

    def download(self):
        p = self.prob
        bs = np.zeros(p.n_s)
        bl = np.zeros(p.n_l)
        st = np.zeros(p.num_block, dtype=np.int32)
        self.ctx.check(self.ctx.lib.dbslmm_plan_download(self.h, _ptr(bs), _ptr(bl), _ptr(st)),
                       "plan_download")
        return bs, bl, st

    def variance(self, test_bed: np.ndarray, indicator, s_pos, l_pos=None) -> np.ndarray:
        """Test-set variance diags (the variance.txt matrix of DBSLMMFIT::est,
        scr/dbslmmfit.cpp:116,242) of the last run: n_test x num_block.  s_pos / l_pos = each
        small / large SNP's row in the test .bed (calcBlock's test_info_*_block[i].pos)."""
        tb = np.ascontiguousarray(test_bed, dtype=np.uint8)
        ind = np.ascontiguousarray(indicator, dtype=np.int32)
        sp = np.ascontiguousarray(s_pos, dtype=np.int32)
        lp = None if l_pos is None else np.ascontiguousarray(l_pos, dtype=np.int32)
        if sp.size != self.prob.n_s or (self.prob.n_l and (lp is None or lp.size != self.prob.n_l)):
            raise ValueError("test s_pos / l_pos must align with the plan's small / large SNPs")
        n_test = int((ind != 0).sum())
        out = np.zeros(n_test * self.prob.num_block)
        nt = np.zeros(1, dtype=np.int32)
        tp = _lib.TestPanel(_ptr(tb), tb.size, ind.size, _ptr(ind), _ptr(sp), _ptr(lp))
        self.ctx.check(self.ctx.lib.dbslmm_plan_variance(self.h, C.byref(tp), _ptr(out), _ptr(nt)),
                       "plan_variance")
        return out.reshape(self.prob.num_block, n_test).T

    def score(self, test_bed: np.ndarray, indicator, s_pos, l_pos=None, *, mode="counts", w_s=None, w_l=None,
              flip_s=None, flip_l=None, chunk_slots=0, n_total=None, n_copies=None):
        """Polygenic scores of a target panel from the betas of the latest run (dbslmm_plan_score),
        one row per copy of that run (1 after run(), len(sigmas) after run_multi()): returns
        (scores[n_copies, n_test], dropped[n_copies]).  indicator: nonzero = selected, or None for
        every individual of the panel (then n_total = the individuals in its .fam is required);
        s_pos / l_pos as in variance().  mode "counts": sum beta w g (with w = 1/sqrt(2 maf (1 - maf))
        the `plink --score 1 2 4 sum` of the effect file); "std": sum beta w (g - mu) / sd over the
        selected individuals.  flip_*: nonzero = the panel's A1 is the other allele.  dropped[c] =
        SNPs that contribute nothing to copy c (NaN betas, no observed call, zero variance in "std").
        The event time of the scoring kernels is kept in self.score_gpu_ms."""
        p = self.prob
        modes = {"counts": _lib.SCORE_COUNTS, "std": _lib.SCORE_STD}
        if mode not in modes:
            raise ValueError('mode: "counts" or "std"')
        tb = np.ascontiguousarray(test_bed, dtype=np.uint8)
        ind = None if indicator is None else np.ascontiguousarray(indicator, dtype=np.int32)
        if ind is None and n_total is None:
            raise ValueError("indicator None (all individuals) needs n_total")
        if ind is not None and n_total is not None and int(n_total) != ind.size:
            raise ValueError("n_total differs from len(indicator)")
        nt_all = ind.size if ind is not None else int(n_total)
        sp = np.ascontiguousarray(s_pos, dtype=np.int32)
        lp = None if l_pos is None else np.ascontiguousarray(l_pos, dtype=np.int32)
        if sp.size != p.n_s or (p.n_l and (lp is None or lp.size != p.n_l)):
            raise ValueError("test s_pos / l_pos must align with the plan's small / large SNPs")

        def per_snp(a, n, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != (n,):
                raise ValueError(f"{what}: one entry per SNP ({n})")
            return a
        ws, wl = per_snp(w_s, p.n_s, np.float64, "w_s"), per_snp(w_l, p.n_l, np.float64, "w_l")
        fs, fl = per_snp(flip_s, p.n_s, np.uint8, "flip_s"), per_snp(flip_l, p.n_l, np.uint8, "flip_l")
        if n_copies is None:                       # the copies of the latest run (anything else is refused)
            n_copies = getattr(self, "_run_copies", 0)
        n_copies = int(n_copies)
        n_test = nt_all if ind is None else int((ind != 0).sum())
        scores = np.zeros((max(1, n_copies), n_test))
        dropped = np.zeros(max(1, n_copies), dtype=np.int32)
        nt = np.zeros(1, dtype=np.int32)
        ms = np.zeros(1)
        args = _lib.ScoreArgs(modes[mode], int(chunk_slots), _ptr(ws), _ptr(wl), _ptr(fs), _ptr(fl))
        tp = _lib.TestPanel(_ptr(tb), tb.size, nt_all, _ptr(ind), _ptr(sp), _ptr(lp))
        self.ctx.check(self.ctx.lib.dbslmm_plan_score(self.h, C.byref(tp), C.byref(args), n_copies, _ptr(scores),
                                                      _ptr(dropped), _ptr(nt), _ptr(ms)), "plan_score")
        self.score_gpu_ms = float(ms[0])
        return scores[:n_copies], dropped[:n_copies]

    def close(self):
        if self.h:
            self.ctx.lib.dbslmm_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DBSLMMFIT:
    """Mirror of the reference's DBSLMMFIT::est (scr/dbslmmfit.hpp:35-66) on one GPU, or on
    several (device = a list of ordinals: the LD blocks sharded over them)."""

    def __init__(self, device=0):
        self.ctx = Context(device)

    def est(self, prob: BlockProblem):
        """Return (beta_s, beta_l, block_status).  LMM-only when prob.l_ptr is None."""
        bs = np.zeros(prob.n_s)
        bl = np.zeros(prob.n_l)
        st = np.zeros(prob.num_block, dtype=np.int32)
        cs = prob.c_struct()
        self.ctx.check(self.ctx.lib.dbslmm_est(self.ctx.h, C.byref(cs), _ptr(bs), _ptr(bl), _ptr(st)),
                       "dbslmm_est")
        return bs, bl, st


def out_ranges(s_ptr, l_ptr=None) -> np.ndarray:
    """The table a streamed run copies finished blocks out by (dbslmm_out_ranges; host only, no
    GPU): one row {block, s0, s1, l0, l1} per non-empty block, in block order."""
    lib = _lib.load()
    sp = np.ascontiguousarray(s_ptr, dtype=np.int64)
    lp = None if l_ptr is None else np.ascontiguousarray(l_ptr, dtype=np.int64)
    nb = len(sp) - 1
    out = np.zeros((max(1, nb), 5), dtype=np.int64)
    n = np.zeros(1, dtype=np.int32)
    rc = lib.dbslmm_out_ranges(nb, _ptr(sp), _ptr(lp), _ptr(out), _ptr(n))
    if rc != 0:
        raise DbslmmError(f"dbslmm_out_ranges failed rc={rc}")
    return out[:int(n[0])]


def bed_maf(ctx: Context, bed: np.ndarray, n_ref: int, n_snp: int) -> np.ndarray:
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    maf = np.zeros(n_snp)
    ctx.check(ctx.lib.dbslmm_bed_maf(ctx.h, _ptr(bed), bed.size, n_ref, n_snp, _ptr(maf)), "bed_maf")
    return maf


def read_snp_std(ctx: Context, bed: np.ndarray, n_ref: int, rows) -> tuple[np.ndarray, np.ndarray]:
    """Standardised genotype columns (n_ref x len(rows), Fortran order) and MAFs."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros(n_ref * len(rows))
    maf = np.zeros(len(rows))
    ctx.check(ctx.lib.dbslmm_read_snp_std(ctx.h, _ptr(bed), bed.size, n_ref, _ptr(rows), len(rows),
                                          _ptr(out), _ptr(maf)), "read_snp_std")
    return out.reshape(len(rows), n_ref).T, maf


def valid_blocks(ctx: Context, bed: np.ndarray, n_ref: int, ptr, pos, z1, z2):
    """External-validation terms of the `valid` tool (scr/validate.cpp:221-257) on the GPU:
    per block nume = z1.z2 and deno = z1^T (X^T X / n_ref) z1."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    z1 = np.ascontiguousarray(z1, dtype=np.float64)
    z2 = np.ascontiguousarray(z2, dtype=np.float64)
    nb = len(ptr) - 1
    nume = np.zeros(nb)
    deno = np.zeros(nb)
    ctx.check(ctx.lib.dbslmm_valid_blocks(ctx.h, _ptr(bed), bed.size, n_ref, nb, _ptr(ptr), _ptr(pos),
                                          _ptr(z1), _ptr(z2), _ptr(nume), _ptr(deno)), "valid_blocks")
    return nume, deno


def ld_r2(ctx: Context, bed: np.ndarray, n_ref: int, rows) -> np.ndarray:
    """r2 of every pair of the bed rows `rows` (dbslmm_ld_r2): the squared Pearson correlation of the
    dosages, missing calls at the row mean; NaN in the row and column of a row without variance."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((len(rows), len(rows)))
    ctx.check(ctx.lib.dbslmm_ld_r2(ctx.h, _ptr(bed), bed.size, n_ref, _ptr(rows), len(rows), _ptr(out)), "ld_r2")
    return out


def clump(ctx: Context, bed: np.ndarray, n_ref: int, rows, chrom, bp, r2: float = 0.2, kb: float = 1000) -> np.ndarray:
    """PLINK's greedy clumping (dbslmm_clump) of the candidates `rows` (bed rows, most significant
    first) with chromosome codes `chrom` and base pairs `bp`: index_of[k] = the candidate that
    absorbed k, k itself for an index SNP.  The event time of the tile kernel is kept in
    ctx.clump_gpu_ms."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    chrom = np.ascontiguousarray(chrom, dtype=np.int32)
    bp = np.ascontiguousarray(bp, dtype=np.int64)
    if not (rows.shape == chrom.shape == bp.shape and rows.ndim == 1):
        raise ValueError("rows, chrom, bp: one entry per candidate")
    out = np.zeros(max(1, len(rows)), dtype=np.int32)
    ms = np.zeros(1)
    args = _lib.ClumpArgs(float(r2), int(round(float(kb) * 1000)))
    ctx.check(ctx.lib.dbslmm_clump(ctx.h, _ptr(bed), bed.size, n_ref, len(rows), _ptr(rows), _ptr(chrom), _ptr(bp),
                                   C.byref(args), _ptr(out), None, _ptr(ms)), "clump")
    ctx.clump_gpu_ms = float(ms[0])
    return out[:len(rows)]


def ld_scores(ctx: Context, bed: np.ndarray, n_ref: int, rows, chrom, bp, kb: float = 1000, unbiased: bool = True,
              max_tiles: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """LD scores (dbslmm_ld_scores) of the bed rows `rows` with chromosome codes `chrom` and base pairs
    `bp`, in any order: (l2, n_window).  l2[k] = the sum over the listed rows within `kb` of row k on
    its chromosome (k included) of r2, with ldsc's adjustment r2 - (1 - r2) / (n_ref - 2) unless
    unbiased is false; NaN for a row without variance or observed call.  n_window[k] counts those
    rows.  max_tiles: 128 x 128 tiles per launch (0 = default; any value gives the same bits).  The
    event time of the kernels is kept in ctx.l2_gpu_ms."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    chrom = np.ascontiguousarray(chrom, dtype=np.int32)
    bp = np.ascontiguousarray(bp, dtype=np.int64)
    if not (rows.shape == chrom.shape == bp.shape and rows.ndim == 1):
        raise ValueError("rows, chrom, bp: one entry per row")
    l2 = np.zeros(max(1, len(rows)))
    nw = np.zeros(max(1, len(rows)), dtype=np.int32)
    ms = np.zeros(1)
    args = _lib.L2Args(int(round(float(kb) * 1000)), 1 if unbiased else 0, int(max_tiles))
    ctx.check(ctx.lib.dbslmm_ld_scores(ctx.h, _ptr(bed), bed.size, n_ref, len(rows), _ptr(rows), _ptr(chrom), _ptr(bp),
                                       C.byref(args), _ptr(l2), _ptr(nw), _ptr(ms)), "ld_scores")
    ctx.l2_gpu_ms = float(ms[0])
    return l2[:len(rows)], nw[:len(rows)]


def ldsc_h2(chi2, n, l2, m, intercept=None, n_blocks: int = 200, chisq_max: float = 0) -> dict:
    """LD score regression (dbslmm_ldsc_fit; host only, no GPU): chi2 = z^2, n = the sample size per
    SNP (or one number), l2 the LD scores, m the number of SNPs the scores stand for.  intercept None
    = free, else fixed at that value.  Returns a dict: h2, h2_se, intercept, intercept_se, mean_chi2,
    n (SNPs used), status (0 ok, 1 too few SNPs, 2 singular; the estimates are NaN unless 0)."""
    chi2 = np.ascontiguousarray(chi2, dtype=np.float64)
    l2 = np.ascontiguousarray(l2, dtype=np.float64)
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, dtype=np.float64), chi2.shape))
    if not (chi2.shape == l2.shape and chi2.ndim == 1):
        raise ValueError("chi2, n, l2: one entry per SNP")
    args = _lib.LdscArgs(1.0 if intercept is None else float(intercept), float(chisq_max),
                         0 if intercept is None else 1, int(n_blocks))
    res = _lib.LdscResult()
    rc = _lib.load().dbslmm_ldsc_fit(len(chi2), _ptr(chi2), _ptr(n), _ptr(l2), float(m), C.byref(args), C.byref(res))
    if rc != 0:
        raise DbslmmError(f"ldsc_fit failed (rc={rc}): bad arguments")
    return dict(h2=res.h2, h2_se=res.h2_se, intercept=res.intercept, intercept_se=res.intercept_se,
                mean_chi2=res.mean_chi2, n=int(res.n_used), status=int(res.status))


def assoc(ctx: Context, bed: np.ndarray, n_total: int, pheno, covar=None, keep=None, rows=None,
          chunk_indiv: int = 0, products: bool = False) -> dict:
    """The association scan (dbslmm_assoc): per bed row a linear model of every phenotype on the row's
    mean-imputed dosage, the intercept and the covariates, with a Wald test.  pheno: n_total or
    n_total x P; covar: n_total x (c - 1) or None; keep: n_total flags or None.  The sample is the kept
    individuals with finite phenotypes and covariates.  rows: bed rows in any order (None: all).
    Returns a dict: n_mis, n_obs, status [rows]; af [rows]; beta, se, tstat, p [P, rows] (NaN unless
    status is 0); with products also prod_d, prod_m [rows, c - 1 + P], the raw products.  chunk_indiv:
    individuals per chunk of the fixed-order sum (a multiple of 64; 0 = the library's constant).  The
    event time of the kernels is kept in ctx.assoc_gpu_ms."""
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    y = np.ascontiguousarray(pheno, dtype=np.float64)
    if y.ndim == 1:
        y = np.ascontiguousarray(y[:, None])
    if y.ndim != 2 or y.shape[0] != n_total:
        raise ValueError("pheno: n_total or n_total x P")
    w = None
    if covar is not None:
        w = np.ascontiguousarray(covar, dtype=np.float64)
        if w.ndim == 1:
            w = np.ascontiguousarray(w[:, None])
        if w.ndim != 2 or w.shape[0] != n_total:
            raise ValueError("covar: n_total x (c - 1)")
        if w.shape[1] == 0:
            w = None
    k = None
    if keep is not None:
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if k.shape != (n_total,):
            raise ValueError("keep: n_total flags")
    if rows is None:
        n_rows = (bed.size - 3) // ((n_total + 3) // 4)
        r = None
    else:
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 1:
            raise ValueError("rows: a list of bed rows")
        n_rows = len(r)
    P, c1 = y.shape[1], 0 if w is None else w.shape[1]
    m = max(1, n_rows)
    n_mis, n_obs, status = (np.zeros(m, dtype=np.int32) for _ in range(3))
    af = np.zeros(m)
    beta, se, tstat, p = (np.zeros((P, m)) for _ in range(4))
    pd = np.zeros((m, c1 + P)) if products else None
    pm = np.zeros((m, c1 + P)) if products else None
    ms = np.zeros(1)
    args = _lib.AssocArgs(_ptr(k), _ptr(y), _ptr(w), P, c1, int(chunk_indiv))
    ctx.check(ctx.lib.dbslmm_assoc(ctx.h, _ptr(bed), bed.size, n_total, n_rows, _ptr(r), C.byref(args), _ptr(n_mis),
                                   _ptr(n_obs), _ptr(af), _ptr(beta), _ptr(se), _ptr(tstat), _ptr(p), _ptr(status),
                                   _ptr(pd), _ptr(pm), _ptr(ms)), "assoc")
    ctx.assoc_gpu_ms = float(ms[0])
    out = dict(n_mis=n_mis[:n_rows], n_obs=n_obs[:n_rows], status=status[:n_rows], af=af[:n_rows],
               beta=beta[:, :n_rows], se=se[:, :n_rows], tstat=tstat[:, :n_rows], p=p[:, :n_rows])
    if products:
        out.update(prod_d=pd[:n_rows], prod_m=pm[:n_rows])
    return out


def assoc_stat_host(n: int, c: int, n1, n2, nm, t, yy) -> dict:
    """The finish of the scan on the host (dbslmm_assoc_stat_host; no GPU): rows with the counts n1, n2,
    nm over n individuals and the products t [rows, c - 1 + P] of their mean-imputed dosages with
    [Q_1 .. | Yr]; yy [P] = |Yr_p|^2; c counts the intercept.  Returns the dict of `assoc` without n_mis."""
    n1, n2, nm = (np.ascontiguousarray(a, dtype=np.int32) for a in (n1, n2, nm))
    yy = np.ascontiguousarray(np.atleast_1d(yy), dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    n_rows, P, c1 = len(n1), len(yy), int(c) - 1
    if not (n1.shape == n2.shape == nm.shape and n1.ndim == 1 and t.shape == (n_rows, c1 + P)):
        raise ValueError("n1, n2, nm: one entry per row; t: rows x (c - 1 + P)")
    m = max(1, n_rows)
    n_obs, status = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    af = np.zeros(m)
    beta, se, tstat, p = (np.zeros((P, m)) for _ in range(4))
    rc = _lib.load().dbslmm_assoc_stat_host(int(n), c1, P, n_rows, _ptr(n1), _ptr(n2), _ptr(nm), _ptr(t), _ptr(yy),
                                            _ptr(n_obs), _ptr(af), _ptr(beta), _ptr(se), _ptr(tstat), _ptr(p),
                                            _ptr(status))
    if rc != 0:
        raise DbslmmError(f"assoc_stat_host failed (rc={rc}): bad arguments")
    return dict(n_obs=n_obs[:n_rows], status=status[:n_rows], af=af[:n_rows], beta=beta[:, :n_rows],
                se=se[:, :n_rows], tstat=tstat[:, :n_rows], p=p[:, :n_rows])


def student_t_two_sided(t: float, df: float) -> float:
    """2 P(t_df <= -|t|) (dbslmm_student_t_two_sided; host only): NaN for a non-finite argument."""
    out = C.c_double()
    rc = _lib.load().dbslmm_student_t_two_sided(float(t), float(df), C.byref(out))
    if rc != 0:
        raise DbslmmError(f"student_t_two_sided failed (rc={rc})")
    return float(out.value)


def tune_r2(scores, pheno) -> tuple[np.ndarray, int]:
    """The r2 index of software/TUNE.R on the scores of Plan.score: per copy the squared Pearson
    correlation of its scores with the phenotype over the individuals whose phenotype is not NaN,
    and the index of the best copy (the first among equals; a copy without variance has r2 NaN and
    never wins)."""
    sc = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    y = np.asarray(pheno, dtype=np.float64)
    if sc.shape[1] != y.size:
        raise ValueError("scores: [n_copies, n_test]; pheno: n_test")
    ok = ~np.isnan(y)
    yc = y[ok] - y[ok].mean() if ok.any() else y[ok]
    r2 = np.full(sc.shape[0], np.nan)
    for c in range(sc.shape[0]):
        x = sc[c, ok]
        xc = x - x.mean() if x.size else x
        den = float(xc @ xc) * float(yc @ yc)
        if x.size >= 2 and den > 0.0 and np.isfinite(den):
            r2[c] = float(xc @ yc) ** 2 / den
    best = int(np.nanargmax(r2)) if np.any(~np.isnan(r2)) else 0
    return r2, best

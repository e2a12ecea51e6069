"""The factorisation route at its size edges and on failed pivots (dbslmm_chol_small,
dbslmm_chol_large, the dbslmm_tchol_* sequence, dbslmm_trsv_bwd).

Part A -- healthy blocks of 1 .. 127 SNPs (tau = 0.8, n_ref = 301, missing calls): the one-wave /
one-workgroup hand-over (63 / 64), the Gram class edge (95 / 96), the z row alone in its 32-row tile
(m % 32 == 0), an odd number of one-wave blocks, and the extreme SNP splits (no large SNP, one, all
but one, all), each block against the oracle's direct solve on its own scale.

Part B -- DBSLMM_BLOCK_NOT_PD.  For tau <= 1 the joint matrix M = Sigma + d P_s is >= (1 - tau) I
and a pivot can only fail through rounding.  tau > 1 is the lever: with
Sigma = tau R (n - 1) / n + (1 - tau) I two identical SNP rows i, j give M (e_i - e_j) =
(1 - tau + d) (e_i - e_j) (d only when both are small SNPs), so with tau = 1.05 and d = 0.02 the
block is indefinite by 0.03 (0.05 for two large SNPs) while every healthy block keeps
lambda_min >= 0.05.  The pivot of column j given any leading part that contains i is at most
e (2a - e) / a < 0 (a = M_ii, e = 1 - tau + d), and the leading j x j part is positive definite, so
the factorisation fails exactly at the copy's column: the test chooses the tile, the step and the
region in which each kernel meets it.  test_preconditions_from_the_reference_alone checks all of
this on the CPU from the oracle and NumPy longdouble, with margins ten orders of magnitude above
fp64 rounding.

Contract under test: status 2 = every beta of that block and copy is NaN; every other block and
copy is what it would be without the failing block, bit for bit; the status is cleared per run.

Reference: oracle.est(method="direct") (its per-block return code is non-zero exactly when its
Cholesky of A or of the Schur complement fails) and NumPy.  Bars: 1e-10 per block for a direct
solve (kappa <= 28 in part A, <= 130 for part B's healthy blocks: m eps kappa <= 1e-11), CHEB_TOL
for the iterated h2f copies, 1e-11 between the single-workgroup and the tiled path
(tests/test_tiled.py).  Measured on the MI355X: part A 6.7e-14 per block at worst (2.4e-10 for an
iterated h2f copy, 4.1e-16 between the two paths), part B's healthy blocks 1.4e-13.
"""
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import ref_numpy as R
from _common import BLOCKS_EUR1, CHEB_TOL, ROOT, TD, blockwise, td_problem

LD = np.longdouble
N_OBS = 100000


# ----------------------------------------------------------------------------- the builder
@functools.lru_cache(maxsize=None)
def _panel_rows(rows, n_ref, miss_rate, seed):
    """The packed rows [m, ceil(n_ref / 4)] of a synthetic panel with at least `rows` SNPs."""
    from dbslmm_amd import synth
    p = synth.simulate(rows + 50, n_ref, pop="EUR", chroms=[1, 2], seed=seed, miss_rate=miss_rate, large_every=0)
    out = p.bed[3:].reshape(-1, (n_ref + 3) // 4)
    assert out.shape[0] >= rows
    out.setflags(write=False)
    return p.bed[:3].copy(), out


class Case:
    """prob (a BlockProblem; copy it with `variant` before changing options or sigma), blocks (the
    builder's list), first (panel row of each block's slot 0), fail (indices of the blocks with a
    duplicated row), keep (the blocks present in the CSR)."""

    def kind(self, b):
        """None (healthy), "s" (the duplicate gets the prior shift) or "l" (it does not)."""
        m, ml, dup = self.blocks[b]
        if dup is None:
            return None
        in_l = [k >= m - ml for k in dup]
        assert in_l[0] == in_l[1], "a duplicate pair lies among the small or among the large SNPs"
        return "l" if in_l[0] and not self.lmm else "s"

    def fails(self, b, sigma):
        """The plan: does block b fail at sigma?  (lambda = 1 - tau + d for "s", 1 - tau for "l")"""
        k = self.kind(b)
        if k is None or b not in self.keep:
            return False
        return 1.0 - self.prob.tau + (1.0 / (sigma * self.prob.n_obs) if k == "s" else 0.0) < 0.0

    def column(self, b):
        return max(self.blocks[b][2])

    def rows(self, b):
        """(small slice, large slice or None) of block b in the output vectors."""
        p = self.prob
        return (slice(int(p.s_ptr[b]), int(p.s_ptr[b + 1])),
                None if p.l_ptr is None else slice(int(p.l_ptr[b]), int(p.l_ptr[b + 1])))

    def of(self, res, b):
        """[beta_s | beta_l] of block b from (beta_s, beta_l, ...)."""
        s, l = self.rows(b)
        return res[0][s] if l is None else np.concatenate([res[0][s], res[1][l]])

    def variant(self, sigma_s=None, **opts):
        return dataclasses.replace(self.prob, sigma_s=self.prob.sigma_s if sigma_s is None else sigma_s,
                                   opts=dict(opts))

    def oracle(self, sigma_s=None):
        """(beta_s, beta_l, status) of the oracle's direct solve, once per sigma."""
        sg = float(self.prob.sigma_s if sigma_s is None else sigma_s)
        if sg not in self._oracle:
            # (no oracle.use_blas here: the switch is process-wide and would move other modules' references)
            p = self.prob
            bs, bl, st, _ = O.est(p.bed, p.n_ref, p.n_obs, sg, p.s_ptr, p.s_pos, p.z_s, p.l_ptr, p.l_pos, p.z_l,
                                  tau=p.tau, method="direct", threads=8)
            for a in (bs, bl, st):
                a.setflags(write=False)
            self._oracle[sg] = (bs, bl, st)
        return self._oracle[sg]

    def sigma_block(self, b):
        """Block b's unshifted joint Sigma in slot order [small | large] (fp64), once."""
        if b not in self._sigma:
            p = self.prob
            s, l = self.rows(b)
            Xs = O.read_block_std(p.bed, p.n_ref, p.s_pos[s], threads=4)
            Xl = O.read_block_std(p.bed, p.n_ref, p.l_pos[l], threads=4) if l is not None and l.stop > l.start else None
            ss, ls, ll = R.block_sigmas_tau(Xs, Xl, p.n_ref, p.tau)
            ms, m = ss.shape[0], ss.shape[0] + (0 if ls is None else ls.shape[0])
            S = np.zeros((m, m))
            S[:ms, :ms] = ss
            if ls is not None:
                S[ms:, :ms], S[:ms, ms:], S[ms:, ms:] = ls, ls.T, ll
            self._sigma[b] = (S, ms)
        return self._sigma[b]

    def joint(self, b, sigma):
        S, ms = self.sigma_block(b)
        M = S.copy()
        M[np.arange(ms), np.arange(ms)] += 1.0 / (sigma * self.prob.n_obs)
        return M


def build_case(blocks, *, n_ref, tau, sigma_s, miss_rate=0.0, seed=11, panel_rows=None, lmm=False, empty=()):
    """blocks: [(m, m_l, dup)], block b on the panel rows first[b] .. first[b] + m in slot order
    [small | large]: the large SNPs are the LAST m_l SNPs of the block, z = +-6; dup = None or
    (i, j) = "the .bed row of slot j := the row of slot i".  lmm: the large SNPs stay small ones
    (no l_ptr); empty: these blocks keep their panel rows but have no SNP in the CSR (so every
    other block reads the rows it reads in the full problem)."""
    from dbslmm_amd import BlockProblem
    sizes = np.array([b[0] for b in blocks], dtype=np.int64)
    n_large = np.array([b[1] for b in blocks], dtype=np.int64)
    assert np.all(n_large <= sizes)
    total = int(sizes.sum())
    magic, panel = _panel_rows(int(panel_rows or total), n_ref, miss_rate, seed)
    rows = panel[:total].copy()
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    for b, (m, _, dup) in enumerate(blocks):
        if dup is not None:
            i, j = dup
            assert 0 <= i < m and 0 <= j < m and i != j
            rows[first[b] + j] = rows[first[b] + i]
    bed = np.concatenate([magic, rows.reshape(-1)])
    bid = np.repeat(np.arange(len(blocks)), sizes)
    slot = np.arange(total) - first[bid]
    large = slot >= (sizes - n_large)[bid]
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(total)
    z[large] = 6.0 * np.sign(z[large])
    if lmm:
        large[:] = False
    keep = ~np.isin(bid, list(empty))

    def csr(mask):
        idx = np.flatnonzero(mask & keep)
        ptr = np.zeros(len(blocks) + 1, dtype=np.int64)
        np.add.at(ptr, bid[idx] + 1, 1)
        return np.cumsum(ptr), idx.astype(np.int32), z[idx]
    s_ptr, s_pos, z_s = csr(~large)
    kw = {}
    if not lmm:
        l_ptr, l_pos, z_l = csr(large)
        kw = dict(l_ptr=l_ptr, l_pos=l_pos, z_l=z_l)
    c = Case()
    c.prob = BlockProblem(bed=bed, n_ref=n_ref, n_obs=N_OBS, sigma_s=sigma_s, tau=tau, s_ptr=s_ptr, s_pos=s_pos,
                          z_s=z_s, **kw)
    c.blocks, c.first, c.lmm = list(blocks), first, lmm
    c.keep = [b for b in range(len(blocks)) if blocks[b][0] > 0 and b not in empty]
    c.fail = [b for b in c.keep if blocks[b][2] is not None]
    c.healthy = [b for b in c.keep if blocks[b][2] is None]
    c._oracle, c._sigma = {}, {}
    return c


def expected_status(c, sigma):
    from dbslmm_amd import BLOCK_EMPTY, BLOCK_NOT_PD, BLOCK_OK
    return np.array([BLOCK_EMPTY if b not in c.keep else BLOCK_NOT_PD if c.fails(b, sigma) else BLOCK_OK
                     for b in range(len(c.blocks))], dtype=np.int32)


def check_failed_blocks_nan_rest_finite(c, res, sigma, what):
    bad = [b for b in c.keep if c.fails(b, sigma)]
    for b in c.keep:
        v = c.of(res, b)
        if b in bad:
            assert np.all(np.isnan(v)), (what, b, c.blocks[b])
        else:
            assert np.all(np.isfinite(v)), (what, b, c.blocks[b])
    return bad


# ----------------------------------------------------------------------------- part A: the cases
LADDER = [1, 2, 3, 31, 32, 33, 40, 62, 63, 64, 65, 95, 96, 97, 127]
PATTERNS = ["none", "one", "all_but_one", "all"]
PATHS = {"default": {}, "tiled64": {"tiled_min": 64}}
A_NREF, A_TAU = 301, 0.8
H2F = (0.8, 1.0, 1.2)


@functools.lru_cache(maxsize=None)
def case_a(pattern):
    ml = {"none": lambda m: 0, "one": lambda m: 1 if m >= 2 else 0, "all_but_one": lambda m: m - 1,
          "all": lambda m: m}[pattern]
    return build_case([(m, ml(m), None) for m in LADDER], n_ref=A_NREF, tau=A_TAU, sigma_s=0.5 / sum(LADDER),
                      miss_rate=0.002, lmm=pattern == "none")


# ----------------------------------------------------------------------------- part B: the cases
B_NREF, B_TAU = 2048, 1.05
B_SIGMA = 5e-4                   # d = 1 / (sigma n) = 0.02
B_ROWS = 2050                    # one panel for the three problems (the largest needs 2044 rows)
B_FACTORS = (0.25, 1.0, 2.0)     # d_c = 0.08 / 0.02 / 0.01
B_RECOVER = B_SIGMA / 10         # d = 0.2: every duplicate among small SNPs turns to +0.15
B_BLOCKS = {
    # one-wave kernel (default dispatch; nine one-wave blocks: the last workgroup's second wave idles)
    "B1": [(1, 0, None), (2, 0, (0, 1)), (40, 1, None), (40, 0, (0, 1)), (63, 2, None), (63, 0, (30, 62)),
           (63, 2, (61, 62)), (0, 0, None), (2, 1, None), (31, 0, None)],
    # one-workgroup kernel: tile 0 (the factor_diag in front of the loop), a lookahead tile, the last
    # column, two large SNPs, a late tile of a 330-SNP block, and 600 SNPs (the panel does not fit LDS)
    "B2": [(64, 1, None), (64, 0, (10, 63)), (100, 2, None), (65, 0, None), (330, 3, None), (100, 0, (2, 5)),
           (100, 0, (7, 40)), (0, 0, None), (100, 0, (50, 99)), (100, 2, (98, 99)), (330, 0, (100, 200)),
           (600, 0, (1, 5))],
    # tiled sequence: region 0 first / fourth 32-column step, region 1 with its pending update,
    # the last column, region 2 (reported by the branch of the later regions), two large SNPs
    "B3": [(128, 2, None), (330, 3, None), (200, 0, None), (70, 1, None), (128, 0, (0, 3)), (128, 0, (50, 100)),
           (0, 0, None), (200, 0, (20, 130)), (200, 0, (100, 199)), (330, 0, (150, 300)), (330, 2, (328, 329))],
}
B_OPTS = {"B1": {"tiled_min": 256},            # (the default of a problem without a block of 512 SNPs)
          "B2": {"tiled_min": 2 ** 31 - 1},
          "B3": {"tiled_min": 64}}
B_NAMES = ["B1", "B2", "B3"]


@functools.lru_cache(maxsize=None)
def case_b(name, lmm=False, emptied=False):
    blocks = B_BLOCKS[name]
    empty = tuple(b for b, x in enumerate(blocks) if x[2] is not None) if emptied else ()
    return build_case(blocks, n_ref=B_NREF, tau=B_TAU, sigma_s=B_SIGMA, panel_rows=B_ROWS, lmm=lmm, empty=empty)


# ----------------------------------------------------------------------------- CPU tests
def test_builder_self_checks():
    for c in [case_a(p) for p in PATTERNS] + [case_b(n) for n in B_NAMES] + [case_b("B3", lmm=True),
                                                                            case_b("B2", emptied=True)]:
        p = c.prob
        nbytes = (p.n_ref + 3) // 4
        rows = p.bed[3:].reshape(-1, nbytes)
        assert rows.shape[0] == sum(b[0] for b in c.blocks)
        seen = []
        for b, (m, ml, dup) in enumerate(c.blocks):
            s, l = c.rows(b)
            if b not in c.keep:
                assert s.stop == s.start and (l is None or l.stop == l.start)
                continue
            ms = m if c.lmm else m - ml
            pos = p.s_pos[s] if l is None else np.concatenate([p.s_pos[s], p.l_pos[l]])
            # slot order [small | large] = consecutive panel rows: the large SNPs are the last m_l
            assert pos.tolist() == list(range(int(c.first[b]), int(c.first[b]) + m)), b
            assert s.stop - s.start == ms
            if l is not None:
                assert np.all(np.abs(p.z_l[l]) == 6.0)
            seen += pos.tolist()
            if dup is not None:
                i, j = dup
                assert np.array_equal(rows[c.first[b] + j], rows[c.first[b] + i])
                assert sum(np.array_equal(rows[c.first[b] + j], rows[c.first[b] + k]) for k in range(m)) == 2
        assert len(set(seen)) == len(seen)
    a = case_a("all")
    assert a.prob.n_s == 0 and a.prob.n_l == sum(LADDER)
    assert case_a("all_but_one").prob.n_s == len(LADDER)
    assert case_a("none").prob.l_ptr is None
    assert sum(1 for m in LADDER if m <= 63) % 2 == 1
    # the emptied problem keeps every healthy block's rows and z
    full, emp = case_b("B2"), case_b("B2", emptied=True)
    assert emp.fail == [] and emp.healthy == full.healthy
    for b in full.healthy:
        assert np.array_equal(full.prob.s_pos[full.rows(b)[0]], emp.prob.s_pos[emp.rows(b)[0]])
        assert np.array_equal(full.prob.z_s[full.rows(b)[0]], emp.prob.z_s[emp.rows(b)[0]])


def first_bad_pivot(M):
    """Column of the first non-positive pivot of an LDL^T of M in longdouble (None: none)."""
    M = np.asarray(M, dtype=LD)
    m = M.shape[0]
    L = np.zeros((m, m), dtype=LD)
    d = np.zeros(m, dtype=LD)
    for j in range(m):
        w = L[j, :j] * d[:j]
        d[j] = M[j, j] - L[j, :j] @ w
        if not d[j] > 0:
            return j
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ w) / d[j]
    return None


# (copies, per problem variant) used on the GPU: d = 1 / (sigma n)
B_SIGMAS_MIXED = sorted({B_SIGMA * f for f in B_FACTORS} | {B_SIGMA})
B_SIGMAS_LMM = [B_SIGMA, B_RECOVER]


@pytest.mark.parametrize("name", B_NAMES)
def test_preconditions_from_the_reference_alone(name):
    """Part B's margins, from the oracle and NumPy only (see the module docstring): healthy blocks
    lambda_min(M_c) >= 0.05 for every sigma_c used, failing blocks <= -0.02 in the copies meant to
    fail and >= 0.02 in those meant to succeed, the first non-positive longdouble pivot at the
    planned column, and the oracle's direct status non-zero on exactly the planned pairs."""
    worst = dict(healthy=np.inf, fail=-np.inf, ok=np.inf, lam_max=0.0)
    for c, sigmas in ((case_b(name), B_SIGMAS_MIXED), (case_b(name, lmm=True), B_SIGMAS_LMM)):
        for sg in sigmas:
            d = 1.0 / (sg * N_OBS)
            planned = []
            for b in c.keep:
                ev = np.linalg.eigvalsh(c.joint(b, sg))
                worst["lam_max"] = max(worst["lam_max"], float(ev[-1]))
                if c.kind(b) is None:
                    worst["healthy"] = min(worst["healthy"], float(ev[0]))
                    assert ev[0] >= 0.05, (name, c.lmm, b, c.blocks[b], d, ev[0])
                elif c.fails(b, sg):
                    planned.append(b)
                    worst["fail"] = max(worst["fail"], float(ev[0]))
                    assert ev[0] <= -0.02, (name, c.lmm, b, c.blocks[b], d, ev[0])
                    assert first_bad_pivot(c.joint(b, sg)) == c.column(b), (name, b, c.blocks[b], d)
                else:
                    worst["ok"] = min(worst["ok"], float(ev[0]))
                    assert ev[0] >= 0.02, (name, c.lmm, b, c.blocks[b], d, ev[0])
            st = c.oracle(sg)[2]
            assert np.flatnonzero(st != 0).tolist() == planned, (name, c.lmm, d, st)
        assert [b for b in c.keep if c.fails(b, B_SIGMA)] == c.fail       # the base copy: every F block fails
    print(f"{name}: healthy lambda_min >= {worst['healthy']:.4f}, failing <= {worst['fail']:.4f}, "
          f"succeeding copies of F blocks >= {worst['ok']:.4f}, lambda_max <= {worst['lam_max']:.2f}")


def test_cli_block_is_indefinite_by_construction():
    """The CLI case of test_cli_reports_the_singular_block: LMM-only test_dat has one non-empty
    block of 716 small SNPs over 400 reference individuals, so Sigma's smallest eigenvalue is
    1 - tau exactly and lambda_min(M) = 1 - tau + d = -0.05 + 996 / (0.5 * 240000) = -0.0417."""
    d = td_problem(lmm_only=True, nsnp=CLI_NSNP, tau=CLI_TAU)
    m_b = np.diff(d["s_ptr"])
    (b,) = np.flatnonzero(m_b)
    assert m_b[b] == 716 > d["n_ref"] == 400
    X = R.read_block_matrix(d["bed"], d["s_pos"], d["n_ref"])
    S, _, _ = R.block_sigmas_tau(X, None, d["n_ref"], CLI_TAU)
    shift = CLI_NSNP / (CLI_H * CLI_N)
    lam = np.linalg.eigvalsh(S + shift * np.eye(716))[0]
    assert abs(lam - (1.0 - CLI_TAU + shift)) < 1e-12 and lam < -0.04


# ----------------------------------------------------------------------------- GPU plumbing
_CTX = {}


def ctx(devices=0):
    from dbslmm_amd import Context
    key = tuple(devices) if isinstance(devices, list) else devices
    if key not in _CTX:
        _CTX[key] = Context(devices)
    return _CTX[key]


def gpu_run(prob, devices=0):
    """(beta_s, beta_l, status, workload) of one run on a fresh plan."""
    from dbslmm_amd import Plan
    plan = Plan(ctx(devices), prob)
    plan.run()
    out = plan.download()
    wl = plan.workload()
    plan.close()
    return out + (wl,)


def gpu_multi(prob, sigmas, devices=0):
    from dbslmm_amd import Plan
    plan = Plan(ctx(devices), prob)
    out = plan.run_multi(sigmas)
    wl = plan.workload()
    plan.close()
    return out, wl


def same(x, y, what=""):
    """Bit for bit (NaNs at the same places)."""
    for a, b in zip(x[:3], y[:3]):
        np.testing.assert_array_equal(a, b, err_msg=str(what))


_A_RUNS = {}


def run_a(pattern, path):
    if (pattern, path) not in _A_RUNS:
        _A_RUNS[pattern, path] = gpu_run(case_a(pattern).variant(**PATHS[path]))
    return _A_RUNS[pattern, path]


# ----------------------------------------------------------------------------- part A on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_ladder_matches_oracle_per_block(pattern, path):
    c = case_a(pattern)
    bs, bl, st, wl = run_a(pattern, path)
    assert wl["pcg_route"] == 0
    n_tiled = sum(1 for m in LADDER if m >= 64) if path == "tiled64" else 0
    assert wl["blocks_tiled"] == n_tiled and wl["blocks_large"] == sum(1 for m in LADDER if m >= 64) - n_tiled
    assert np.all(st == 0), st
    assert np.all(c.oracle()[2] == 0)
    err = blockwise(c.prob, (bs, bl), c.oracle()[:2])
    print(f"ladder {pattern} {path}: worst per-block error vs the direct solve {err:.3e}")
    assert err < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_ladder_tiled_equals_single_workgroup(pattern):
    c = case_a(pattern)
    err = blockwise(c.prob, run_a(pattern, "tiled64")[:2], run_a(pattern, "default")[:2])
    print(f"ladder {pattern}: tiled_min = 64 vs the default dispatch, worst per block {err:.3e}")
    assert err < 1e-11
    for b, m in enumerate(LADDER):     # below 64 SNPs the option changes nothing
        if m < 64:
            np.testing.assert_array_equal(c.of(run_a(pattern, "tiled64"), b), c.of(run_a(pattern, "default"), b))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_ladder_h2f_copies(pattern):
    """run_multi on the default dispatch: dbslmm_chol_small factors every copy, the blocks of
    >= 64 SNPs factor the base copy (the median sigma) and iterate the others on it."""
    c = case_a(pattern)
    sig = [c.prob.sigma_s * f for f in H2F]
    multi, wl = gpu_multi(c.variant(), sig)
    assert wl["pcg_route"] == 0 and wl["cheb_base"] == 1
    for k, sg in enumerate(sig):
        assert np.all(multi[k][2] == 0), (k, multi[k][2])
        err = blockwise(c.prob, multi[k][:2], c.oracle(sg)[:2])
        print(f"ladder {pattern} h2f {H2F[k]}: worst per-block error {err:.3e}")
        assert err < CHEB_TOL, (k, err)
    same(multi[1], run_a(pattern, "default"), "the base copy")
    assert blockwise(c.prob, multi[1][:2], c.oracle()[:2]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("m,tiled_min,keeps", [(63, 0, "no_y"), (95, 0, "full"), (96, 0, "full"), (127, 64, "full")],
                         ids=["small63", "large95", "large96", "tiled127"])
def test_ladder_stored_factor(m, tiled_min, keeps):
    """The factor dbslmm_variance reads back (strict lower L, diagonal 1 / L_ii) and the y row, per
    kernel: dbslmm_chol_small (63; its y row stays in LDS), dbslmm_chol_large with the z row
    inside its last SNP tile (95) and alone in a tile of its own (96), the region kernel with the
    z row in the last row of the region (127, ld = 128)."""
    from test_fullscale import _diagnose
    c = case_a("one")
    prob = c.variant(**({"tiled_min": tiled_min} if tiled_min else {}))
    d = _diagnose(prob, LADDER.index(m), prob.sigma_s, 4, factor=keeps)
    print(f"stored factor m = {m}: {d}")
    assert set(d) == {"sigma", "L", "L_diag", "beta"} | ({"y"} if keeps == "full" else set()), d
    assert max(d.values()) < 1e-10, d


# ----------------------------------------------------------------------------- part B on the GPU
def healthy_error(c, res, sigma):
    skip = [b for b in range(len(c.blocks)) if c.fails(b, sigma)]
    return blockwise(c.prob, res[:2], c.oracle(sigma)[:2], skip=skip)


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_NAMES)
def test_failed_pivot_single_run(name):
    c = case_b(name)
    res = gpu_run(c.variant(**B_OPTS[name]))
    assert res[3]["pcg_route"] == 0
    assert res[2].tolist() == expected_status(c, B_SIGMA).tolist()
    assert check_failed_blocks_nan_rest_finite(c, res, B_SIGMA, name) == c.fail
    err = healthy_error(c, res, B_SIGMA)
    print(f"{name}: healthy blocks beside failing ones, worst per-block error {err:.3e}")
    assert err < 1e-10
    # a block is factored identically whatever it is batched with
    e = case_b(name, emptied=True)
    alone = gpu_run(e.variant(**B_OPTS[name]))
    assert alone[2].tolist() == expected_status(e, B_SIGMA).tolist()
    for b in c.healthy:
        np.testing.assert_array_equal(c.of(res, b), e.of(alone, b), err_msg=f"{name} block {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_NAMES)
def test_failed_pivot_repeat_and_recover(name):
    from dbslmm_amd import Plan
    c = case_b(name, lmm=True)
    assert all(c.kind(b) == "s" for b in c.fail)
    plan = Plan(ctx(), c.variant(**B_OPTS[name]))
    runs = []
    for _ in range(3):                       # (the tiled sequence: direct, then captured and replayed)
        plan.run()
        runs.append(plan.download())
    assert runs[0][2].tolist() == expected_status(c, B_SIGMA).tolist()
    assert check_failed_blocks_nan_rest_finite(c, runs[0], B_SIGMA, name) == c.fail
    for r in runs[1:]:
        same(r, runs[0], "repeat at the failing sigma")
    plan.set_sigma(B_RECOVER)
    plan.run()
    good = plan.download()
    assert good[2].tolist() == expected_status(c, B_RECOVER).tolist()
    assert set(good[2].tolist()) <= {0, 1} and np.all(np.isfinite(good[0]))
    same(good, gpu_run(c.variant(sigma_s=B_RECOVER, **B_OPTS[name])), "recovered plan vs a fresh one")
    err = blockwise(c.prob, good[:2], c.oracle(B_RECOVER)[:2])
    print(f"{name}: after set_sigma (d = 0.2), worst per-block error {err:.3e}")
    assert err < 1e-10
    plan.set_sigma(B_SIGMA)
    plan.run()
    same(plan.download(), runs[0], "back at the failing sigma")
    plan.close()


_B_MULTI = {}


def multi_b(name):
    """Part B's run_multi on the mixed problem, once: (copies, workload)."""
    if name not in _B_MULTI:
        _B_MULTI[name] = gpu_multi(case_b(name).variant(**B_OPTS[name]), [B_SIGMA * f for f in B_FACTORS])
    return _B_MULTI[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_NAMES)
def test_failed_pivot_per_copy_verdicts(name):
    from dbslmm_amd import BLOCK_EMPTY, BLOCK_NOT_PD, BLOCK_OK
    c = case_b(name)
    multi, wl = multi_b(name)
    assert wl["pcg_route"] == 0 and wl["cheb_iters"] == 0          # tau > 1: the merged factorisation
    n_fail = []
    for k, f in enumerate(B_FACTORS):
        sg = B_SIGMA * f
        ost = c.oracle(sg)[2]
        want = np.where(ost != 0, BLOCK_NOT_PD, BLOCK_OK)
        want[[b for b in range(len(c.blocks)) if b not in c.keep]] = BLOCK_EMPTY
        assert multi[k][2].tolist() == want.tolist(), (name, k)
        assert want.tolist() == expected_status(c, sg).tolist()
        n_fail.append(len(check_failed_blocks_nan_rest_finite(c, multi[k], sg, (name, k))))
        err = healthy_error(c, multi[k], sg)
        print(f"{name} copy {k} (d = {0.02 / f:.3g}): worst per-block error of the succeeding blocks {err:.3e}")
        assert err < 1e-10
        same(multi[k], gpu_run(c.variant(sigma_s=sg, **B_OPTS[name])), f"{name} copy {k} vs a fresh plan")
    n_l = sum(1 for b in c.fail if c.kind(b) == "l")
    assert n_fail == [n_l, len(c.fail), len(c.fail)]


@functools.lru_cache(maxsize=None)
def target_panel(n_total=150, seed=111):
    """A target panel for B3's SNPs at permuted rows, 75 % of its individuals selected."""
    c = case_b("B3")
    magic, t = _panel_rows(B_ROWS, n_total, 0.0, seed)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(t.shape[0]).astype(np.int32)          # SNP r sits at target row perm[r]
    rows = np.zeros_like(t)
    rows[perm] = t
    tbed = np.concatenate([magic, rows.reshape(-1)])
    ind = (rng.random(n_total) < 0.75).astype(np.int32)
    return tbed, ind, perm[c.prob.s_pos], perm[c.prob.l_pos], n_total


@pytest.mark.gpu
def test_failed_pivot_consumers():
    """dbslmm_variance and dbslmm_score_* behind a run with failed (block, copy) pairs (B3)."""
    from dbslmm_amd import Plan
    from test_score import Panel, check
    from test_variance import TOL, _colwise, synth_oracle
    c = case_b("B3")
    prob = c.variant(**B_OPTS["B3"])
    sig = [B_SIGMA * f for f in B_FACTORS]
    tbed, ind, ts_pos, tl_pos, n_total = target_panel()
    plan = Plan(ctx(), prob)
    multi = plan.run_multi(sig)
    same_as = multi_b("B3")[0]
    for k in range(len(sig)):
        same(multi[k], same_as[k])
    # variance: the factor of the last copy
    got = plan.variance(tbed, ind, ts_pos, tl_pos)
    last_bad = [b for b in c.keep if c.fails(b, sig[-1])]
    assert last_bad == c.fail
    assert np.all(np.isnan(got[:, last_bad]))
    rest = [b for b in range(len(c.blocks)) if b not in last_bad]
    ref = synth_oracle(prob, tbed, ind, ts_pos, tl_pos, sigma=sig[-1])
    assert np.all(np.isfinite(got[:, rest]))
    err = _colwise(got[:, rest], ref[:, rest])
    print(f"B3 variance beside failed blocks: worst column {err:.3e}")
    assert err < TOL
    # scores: ok from the ORACLE's verdicts
    m_b = np.array([b[0] for b in c.blocks])
    P = Panel(tbed, n_total, ind, np.concatenate([ts_pos, tl_pos]))
    beta = np.stack([np.concatenate([r[0], r[1]]) for r in multi])
    blk = np.concatenate([np.repeat(np.arange(len(m_b)), np.diff(prob.s_ptr)),
                          np.repeat(np.arange(len(m_b)), np.diff(prob.l_ptr))])
    ok = np.stack([c.oracle(sg)[2][blk] == 0 for sg in sig])
    want_dropped = [int(sum(m_b[b] for b in c.keep if c.fails(b, sg))) for sg in sig]
    for mode in ("counts", "std"):
        sc, dropped = plan.score(tbed, ind, ts_pos, tl_pos, mode=mode)
        assert dropped.tolist() == want_dropped, (mode, dropped)
        check(sc, dropped, P, beta, ok, mode, what="B3 beside failed blocks", useful=False)
    plan.close()


@pytest.mark.gpu
def test_failed_pivot_three_shards_on_one_device():
    c = case_b("B3")
    prob = c.variant(**B_OPTS["B3"])
    one = gpu_run(prob)
    assert one[2].tolist() == expected_status(c, B_SIGMA).tolist()
    same(gpu_run(prob, [0, 0, 0]), one, "run on three shards")
    sig = [B_SIGMA * f for f in B_FACTORS]
    multi, _ = gpu_multi(prob, sig, [0, 0, 0])
    for k in range(len(sig)):
        same(multi[k], multi_b("B3")[0][k], f"run_multi copy {k} on three shards")


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_NAMES)
def test_failed_pivot_pcg_gate(name):
    """tau > 1 has no data-free lower bound on lambda_min: the PCG route is refused whether it is
    forced (solver = 2) or its prior-shift rule would pick it (every d_c >= 2)."""
    c = case_b(name)
    sig = [B_SIGMA * f for f in B_FACTORS]
    forced, wl = gpu_multi(c.variant(solver=2, **B_OPTS[name]), sig)
    assert wl["pcg_route"] == 0
    for k in range(len(sig)):
        same(forced[k], multi_b(name)[0][k], f"{name} solver = 2, copy {k}")
    one = gpu_run(c.variant(solver=2, **B_OPTS[name]))
    assert one[3]["pcg_route"] == 0
    same(one, gpu_run(c.variant(solver=1, **B_OPTS[name])), f"{name} solver = 2, one run")
    big = [s / 400.0 for s in sig]                       # d_c = 32 / 8 / 4
    assert min(1.0 / (s * N_OBS) for s in big) >= 2.0
    auto, wl = gpu_multi(c.variant(sigma_s=big[1], **B_OPTS[name]), big)
    assert wl["pcg_route"] == 0
    fact, _ = gpu_multi(c.variant(sigma_s=big[1], solver=1, **B_OPTS[name]), big)
    for k in range(len(big)):
        same(auto[k], fact[k], f"{name} auto rule at d >= 2, copy {k}")
        assert auto[k][2].tolist() == expected_status(c, big[k]).tolist()   # ("l" duplicates still fail)


# ----------------------------------------------------------------------------- the CLI
CLI = os.path.join(ROOT, "dbslmm_amd", "bin", "dbslmm")
CLI_TAU, CLI_N, CLI_H, CLI_NSNP = 1.05, 240000, 0.5, 996


@pytest.mark.gpu
def test_cli_reports_the_singular_block(tmp_path):
    """test_cli_block_is_indefinite_by_construction's block through the CLI: the reference's
    "Matrix is Singular!" line with the block count, every effect of the block written as nan, and
    exit code 0 (the reference prints the error and goes on, and so does the CLI)."""
    eff = str(tmp_path / "out")
    r = subprocess.run([CLI, "-s", os.path.join(TD, "summary_gemma_chr1.assoc.txt"), "-r", os.path.join(TD, "ref_chr1"),
                        "-b", BLOCKS_EUR1, "-n", str(CLI_N), "-nsnp", str(CLI_NSNP), "-h", str(CLI_H), "-mafMax", "0.2",
                        "-eff", eff, "--tau", str(CLI_TAU), "--precise-out"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert "Matrix is Singular! (1 LD blocks" in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = [l.split() for l in open(eff + ".txt").read().splitlines() if l.strip()]
    assert len(rows) == 716
    assert all(x[2] == "nan" and x[3] == "nan" for x in rows), rows[:3]

"""The test-set variance at its shape edges (dbslmm_test_compact, dbslmm_snp_stats,
dbslmm_variance; dbslmm_plan_variance / mp_variance).

Reference: the factor form of DESIGN 3.5 evaluated per block in NumPy longdouble from the two .bed
images alone (factor_form: the joint matrix M at the problem's tau and d = 1 / (n sigma), a
hand-written Cholesky and forward substitution, readSNPIm + nomalizeVec over the selected
individuals with mean imputation and the N - 1 sd).  test_reference_equals_literal_formulas holds
it to the literal formulas of calc_nt_by_nt_matrix (ref_numpy.nt_diag_ls / nt_diag_s, explicit
fp64 inverses) on every block of the ladder, so it stands on the reference's mathematics.

The all-large block (no small SNP): calcBlock's formulas with empty small-SNP matrices give
x_l^T Sigma_ll^-1 x_l / n, which is what the kernel returns (|L_ll^-1 x_l|^2 / n); only a block
without any SNP is a zero column.  ref_numpy.variance_diags and test_variance.synth_oracle used to
skip such a block (column 0) and follow the literal formulas now.

Bars: per case, the same factor form in plain fp64 NumPy; its worst column-wise max-norm distance
to the longdouble reference is the floor fp64 leaves on that input (d |x_s|^2 - d^2 (q1 - w2)
cancels by about (d + 1 - tau) / (1 - tau)).  The GPU bar of a case is min(10 x floor, 1e-8), each
column on its own scale (Ref.bar).  A column is NaN exactly where the reference's is (a SNP
without variance among the selected individuals: 0/0 in nomalizeVec; no observed call: 0/0 in
readSNPIm; a block whose factorisation failed).

Cases: (1) the ladder LADDER of block sizes and small / large splits around the 32-row chunks and
8-row wave groups of the substitution, with tiled_min 64 and 100000; (2) n_test around the 64-wide
workgroups and the 4-per-byte compaction, n_total = 4k / 4k + 1 / 4k + 3 with the last individual
selected, the first or the last alone (n_test = 1: every non-empty column NaN), everyone; (3) two
row layouts of one test panel (rows 0 and the last needed), missing calls, a SNP without any
observed call; (4) the factor behind run, run_multi (last copy factored, iterated by Chebyshev and
by CG) and a PCG-route run; (5) a NOT_PD block (tau = 1.05, a duplicated row) beside healthy ones;
(6) more than 65 536 slots; (7) three shards on one device.

tau = 1: test_preconditions_from_the_reference_alone measures the reference's own floor on the
ladder at tau = 1: 1.2e-14, far below 1e-8, so the tau = 1 ladder is held to the relative bar like
every other case (the floor of every case is asserted below 1e-9 there: the 1e-8 cap never binds).

Measured on the MI355X: the worst column of each group, with the floor and the bar of the case it
occurred in (fp64 NumPy is usually the further of the two from the longdouble reference):
  group                                                     GPU worst   floor     bar
  ladder tau 0.8: both paths, run, run_multi, shards        1.4e-15     4.9e-15   4.9e-14
  ladder tau 1, both paths                                  2.5e-15     1.2e-14   1.2e-13
  after a PCG-route run, d = 20                             4.3e-14     1.4e-14   1.4e-13
  after a PCG-route run_multi, d = 16.7                     1.3e-14     1.2e-14   1.2e-13
  test individuals, worst (64 of 197)                       9.8e-16     1.1e-15   1.1e-14
  test individuals, closest to its bar (2 of 197)           2.1e-16     2.1e-16   2.1e-15
  test-panel rows, missing calls                            4.8e-16     1.0e-15   1.0e-14
  beside NOT_PD blocks, tau = 1.05                          5.1e-16     5.4e-16   5.4e-15
  89 600 slots (four sampled blocks)                        5.2e-16     4.1e-16   4.1e-15
The launch with grid.y = 89 600 (dbslmm_test_compact, one grid row per slot) is accepted and its
results are right in the first and last block and on both sides of slot 65 536: nothing was
changed for it (the score path's subset feeder launches the same kernel 32 768 slots at a time).

One defect found: a test SNP's missing call was standardised to 0 without the division by the sd,
so a SNP without any observed call among the selected individuals left its block's column finite
(seen: 3.0e-3 where the reference's readSNPIm mean is 0/0), and a SNP without variance left the
entries of the individuals with a missing call finite.  var::xval now returns 0 x (1 / sd) for a
missing call: NaN in both cases, +0 otherwise (every other result keeps its bits).

Mutants of variance.hip, failing tests of this module's 33 GPU tests (each built and run once):
r <= ms in the q1 / w2 split 28; the chunk's row count one short 30; pass 2 from ms + 1 30; w2
dropped 28; t <= n_test in dbslmm_test_compact (the extra code read from the last selected
individual) 26; the last selected individual read from sel[t] - 1 28.
"""
import dataclasses
import functools

import numpy as np
import pytest

import ref_numpy as R
from test_chol_edges import N_OBS, build_case, ctx

LD = np.longdouble
TOL_MAX = 1e-8                   # the bar of tests/test_variance.py: no case is held looser

# ----------------------------------------------------------------------------- the reference
_DOSE = (2.0, np.nan, 1.0, 0.0)  # PLINK code -> dosage (01 = missing)


def std_columns(bed, rows, n_total, sel, dt):
    """readSNPIm + nomalizeVec in dtype dt: the standardised columns [len(sel), len(rows)] of the
    .bed rows `rows` over the individuals `sel` (missing -> the mean of the observed selected calls,
    then centred and divided by the N - 1 sd; 0/0 = NaN where the reference divides 0 by 0)."""
    nbytes = (n_total + 3) // 4
    lut = np.array(_DOSE, dtype=dt)
    X = np.zeros((len(sel), len(rows)), dtype=dt)
    with np.errstate(all="ignore"):
        for c, r in enumerate(rows):
            r = int(r)
            code = R.decode_codes(bed[3 + r * nbytes: 3 + (r + 1) * nbytes], n_total)[sel]
            g = lut[code]
            miss = code == 1
            g[miss] = g[~miss].sum() / dt(g.size - miss.sum())
            x = g - g.sum() / dt(g.size)
            X[:, c] = x / np.sqrt((x * x).sum() / dt(g.size - 1))
    return X


def cholesky(M):
    """Hand-written (column by column, in M's dtype); LinAlgError at a non-positive pivot."""
    m = M.shape[0]
    L = np.zeros_like(M)
    for j in range(m):
        s = M[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0:
            raise np.linalg.LinAlgError(f"pivot {j}")
        L[j, j] = np.sqrt(s)
        if j + 1 < m:
            L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward(L, B):
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def factor_form(S, ms, Ts, Tl, n_obs, sigma, dt):
    """DESIGN 3.5 in dtype dt.  S: the block's unshifted joint Sigma [small | large], Ts / Tl the
    standardised test columns [n_test, ms] / [n_test, m - ms].
    diag_t = |L_ll^-1 x_l|^2 / n + n sigma^2 (d |x_s|^2 - d^2 (|y_s|^2 - |y_l|^2)), y = L^-1 [x_s; 0]."""
    m, nt = S.shape[0], Ts.shape[0]
    n, sg = dt(n_obs), dt(sigma)
    d = dt(1) / (n * sg)
    M = S.copy()
    M[np.arange(ms), np.arange(ms)] += d
    try:
        L = cholesky(M)
    except np.linalg.LinAlgError:
        return np.full(nt, np.nan, dtype=dt)
    U = np.zeros((m, nt), dtype=dt)
    U[:ms] = Ts.T
    Y = forward(L, U)
    q1, w2 = (Y[:ms] ** 2).sum(0), (Y[ms:] ** 2).sum(0)
    q3 = (forward(L[ms:, ms:], np.ascontiguousarray(Tl.T)) ** 2).sum(0)
    xs2 = (Ts ** 2).sum(1)
    return q3 / n + n * sg * sg * (d * xs2 - d * d * (q1 - w2))


class Panel:
    """A test panel: tbed, n_total, and the test row of each small / large SNP (ts_pos / tl_pos)."""

    def __init__(self, dos, perm, prob):
        from dbslmm_amd.synth import BED_MAGIC, pack_dosages
        rows = np.zeros((dos.shape[0], (dos.shape[1] + 3) // 4), dtype=np.uint8)
        rows[perm] = pack_dosages(dos)                       # SNP (reference row) r sits at test row perm[r]
        self.tbed = np.concatenate([np.frombuffer(BED_MAGIC, dtype=np.uint8), rows.reshape(-1)])
        self.n_total = dos.shape[1]
        self.ts_pos = perm[prob.s_pos].astype(np.int32)
        self.tl_pos = perm[prob.l_pos].astype(np.int32)


def random_dosages(n_rows, n_total, seed, miss=0.01):
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.2, 0.5, size=(n_rows, 1))
    dos = ((rng.random((n_rows, n_total)) < af).astype(np.int8) + (rng.random((n_rows, n_total)) < af).astype(np.int8))
    dos[rng.random(dos.shape) < miss] = -1
    return dos


class Ref:
    """The reference of one (problem, test panel, selection): per sigma the n_test x num_block
    matrix in longdouble, its fp64 floor and the bar; Sigma and the test columns are kept per block."""

    def __init__(self, c, panel, ind, blocks=None):
        self.c, self.p, self.panel = c, c.prob, panel
        self.ind = np.asarray(ind, dtype=np.int32)
        self.sel = np.flatnonzero(self.ind != 0)
        self.blocks = list(range(self.p.num_block)) if blocks is None else list(blocks)
        self._parts, self._out = {}, {}

    def rows(self, b):
        p = self.p
        s, l = slice(int(p.s_ptr[b]), int(p.s_ptr[b + 1])), slice(int(p.l_ptr[b]), int(p.l_ptr[b + 1]))
        return p.s_pos[s], p.l_pos[l], self.panel.ts_pos[s], self.panel.tl_pos[l]

    def parts(self, b, dt):
        if (b, dt) not in self._parts:
            p = self.p
            rs, rl, ts, tl = self.rows(b)
            X = std_columns(p.bed, np.concatenate([rs, rl]), p.n_ref, np.arange(p.n_ref), dt)
            m = X.shape[1]
            S = dt(p.tau) * (X.T @ X) / dt(p.n_ref) + (dt(1) - dt(p.tau)) * np.eye(m, dtype=dt)
            Ts = std_columns(self.panel.tbed, ts, self.panel.n_total, self.sel, dt)
            Tl = std_columns(self.panel.tbed, tl, self.panel.n_total, self.sel, dt)
            self._parts[b, dt] = (S, rs.size, Ts, Tl)
        return self._parts[b, dt]

    def diags(self, sigma=None, dt=LD):
        sg = float(self.p.sigma_s if sigma is None else sigma)
        if (sg, dt) not in self._out:
            D = np.zeros((self.sel.size, self.p.num_block), dtype=dt)
            with np.errstate(all="ignore"):
                for b in self.blocks:
                    S, ms, Ts, Tl = self.parts(b, dt)
                    if S.shape[0]:
                        D[:, b] = factor_form(S, ms, Ts, Tl, self.p.n_obs, sg, dt)
            D.setflags(write=False)
            self._out[sg, dt] = D
        return self._out[sg, dt]

    def floor(self, sigma=None):
        """The worst column of the fp64 evaluation against the longdouble one."""
        return worst_column(self.diags(sigma, np.float64), self.diags(sigma), self.blocks)

    def bar(self, sigma=None):
        return min(10.0 * self.floor(sigma), TOL_MAX)


def column_errors(got, ref, blocks=None):
    """Per column max |got - ref| / max |ref| (longdouble).  A reference column is all NaN or all
    finite, and got is NaN in exactly the same columns; a zero reference column is exactly zero."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = {}
    for b in range(ref.shape[1]) if blocks is None else blocks:
        g, r = np.asarray(got[:, b], dtype=LD), np.asarray(ref[:, b], dtype=LD)
        if np.any(np.isnan(r)):
            assert np.all(np.isnan(r)), b
            assert np.all(np.isnan(g)), ("the reference's column is NaN", b, g)
            continue
        assert np.all(np.isfinite(g)), ("the reference's column is finite", b, g)
        s = np.max(np.abs(r)) if r.size else LD(0)
        if s == 0:
            assert np.all(g == 0), b
            continue
        out[b] = float(np.max(np.abs(g - r)) / s)
    return out


def worst_column(got, ref, blocks=None):
    e = column_errors(got, ref, blocks)
    return max(e.values()) if e else 0.0


def held(got, ref, sigma=None, what=""):
    """The case's check: got against ref.diags(sigma) at the case's bar; prints floor, bar, worst."""
    floor, bar = ref.floor(sigma), ref.bar(sigma)
    err = column_errors(got, ref.diags(sigma), ref.blocks)
    b = max(err, key=err.get) if err else None
    worst = err[b] if err else 0.0
    print(f"{what}: floor {floor:.2e}, bar {bar:.2e}, GPU worst column {worst:.2e} "
          f"(block {b}{'' if b is None else ' ' + str(ref.c.blocks[b][:2])})")
    assert worst <= bar, (what, b, worst, bar)
    return worst


# ----------------------------------------------------------------------------- the cases
V_NREF, V_MISS, V_SIGMA = 301, 0.002, 1e-4          # d = 1 / (1e-4 x 100000) = 0.1
PCG_SIGMA = 0.5 / 1e6                                # d = 20: the prior shift of the flagship runs
# (m, m_large): the large SNPs are the last m_large slots of a block, so the small ones end at
# ms = m - m_large.  32-row chunks, 8 rows per wave.
LADDER = (
    # no large SNP: m % 32 in {0, 1, 31}, one row, one chunk + 1, four chunks + 1
    [(m, 0) for m in (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)]
    # one large SNP: the last row of a chunk (32, 64, 128), alone in a new chunk (33, 65, 129: ms % 32 == 0)
    + [(2, 1), (32, 1), (33, 1), (64, 1), (65, 1), (127, 1), (128, 1), (129, 1)]
    # ms a multiple of 32 and nine large SNPs: the large rows open a chunk and cross a wave's rows
    + [(41, 9), (73, 9), (105, 9), (128, 96)]
    # ms % 8 == 1 (57, 73, 33) and == 7 (55, 31, 127, 63)
    + [(64, 7), (96, 23), (63, 8), (33, 2), (129, 2), (65, 32), (96, 33)]
    # ms = 1, the rest large
    + [(32, 31), (65, 64), (128, 127)]
    # no small SNP at all; an empty block among them
    + [(1, 1), (31, 31), (0, 0), (32, 32), (64, 64), (129, 129)]
)
PATHS = {"tiled64": {"tiled_min": 64}, "single": {"tiled_min": 100000}}
EMPTY = LADDER.index((0, 0))


@functools.lru_cache(maxsize=None)
def case_ladder(tau=0.8):
    return build_case([(m, ml, None) for m, ml in LADDER], n_ref=V_NREF, tau=tau, sigma_s=V_SIGMA,
                      miss_rate=V_MISS, seed=23)


@functools.lru_cache(maxsize=None)
def ladder(tau=0.8):
    """(case, panel, indicator, Ref): 150 test individuals, about three quarters selected (two
    workgroups of 64), the SNPs at permuted test rows, missing calls."""
    c = case_ladder(tau)
    rows, n_total = sum(m for m, _ in LADDER) + 10, 150
    rng = np.random.default_rng(5)
    panel = Panel(random_dosages(rows, n_total, seed=6), rng.permutation(rows), c.prob)
    ind = (rng.random(n_total) < 0.75).astype(np.int32)
    return c, panel, ind, Ref(c, panel, ind)


SMALL = [(40, 3), (33, 1), (5, 0), (0, 0), (7, 7)]       # 40 and 33 span a chunk seam
SMALL_ROWS = sum(m for m, _ in SMALL) + 3


@functools.lru_cache(maxsize=None)
def case_small():
    return build_case([(m, ml, None) for m, ml in SMALL], n_ref=V_NREF, tau=0.8, sigma_s=V_SIGMA,
                      miss_rate=V_MISS, seed=29)


def selection(n_total, n_test, mode, seed):
    """mode "last": n_test individuals with the last one among them; "first_only" / "last_only" /
    "all"."""
    ind = np.zeros(n_total, dtype=np.int32)
    if mode == "all":
        ind[:] = 1
    elif mode == "first_only":
        ind[0] = 1
    elif mode == "last_only":
        ind[-1] = 1
    else:
        rng = np.random.default_rng(seed)
        ind[rng.choice(n_total - 1, size=n_test - 1, replace=False)] = 1
        ind[-1] = 1
    return ind


def small_panel(n_total, ind, seed=31):
    """Random dosages; every SNP of block 0 differs between the first and the last selected
    individual (both observed), so block 0 is finite from n_test = 2 on."""
    c = case_small()
    dos = random_dosages(SMALL_ROWS, n_total, seed)
    sel = np.flatnonzero(ind)
    if sel.size >= 2:
        m0 = SMALL[0][0]
        a = np.where(dos[:m0, sel[0]] < 0, 0, dos[:m0, sel[0]])
        dos[:m0, sel[0]] = a
        dos[:m0, sel[-1]] = (a + 1 + np.arange(m0) % 2) % 3
    perm = np.random.default_rng(seed + 1).permutation(SMALL_ROWS)
    return Panel(dos, perm, c.prob)


# (n_total, n_test, mode): every n_test around the 64-wide workgroups and the bytes of 4, with
# n_total = 4k + 1 / 4k + 3 / 4k and the last individual selected; then the selections of one,
# and everyone at each n_total % 4
SELECTIONS = ([(nt_all, n, "last") for n, nt_all in zip((2, 3, 63, 64, 65, 127, 128, 129),
                                                        (197, 199, 200, 197, 199, 200, 197, 199))]
              + [(197, 1, "first_only"), (199, 1, "last_only"), (200, 1, "last_only")]
              + [(132, 132, "all"), (129, 129, "all"), (131, 131, "all")])


@functools.lru_cache(maxsize=None)
def small(n_total, n_test, mode):
    ind = selection(n_total, n_test, mode, seed=n_total + n_test)
    assert int(ind.sum()) == n_test
    panel = small_panel(n_total, ind)
    return case_small(), panel, ind, Ref(case_small(), panel, ind)


# NOT_PD: tau = 1.05 and a duplicated row (test_chol_edges.py part B, its panel and margins)
D_NREF, D_TAU, D_SIGMA, D_ROWS = 2048, 1.05, 5e-4, 2050
D_BLOCKS = [(40, 1, None), (64, 0, (10, 63)), (70, 2, None), (0, 0, None), (33, 3, (31, 32)), (65, 1, None),
            (5, 0, (0, 1)), (96, 0, None)]


@functools.lru_cache(maxsize=None)
def dup(emptied=False):
    empty = tuple(b for b, x in enumerate(D_BLOCKS) if x[2] is not None) if emptied else ()
    c = build_case(D_BLOCKS, n_ref=D_NREF, tau=D_TAU, sigma_s=D_SIGMA, panel_rows=D_ROWS, empty=empty)
    rows, n_total = sum(b[0] for b in D_BLOCKS), 90
    rng = np.random.default_rng(41)
    perm = rng.permutation(rows)
    ind = (rng.random(n_total) < 0.8).astype(np.int32)
    dos = random_dosages(rows, n_total, seed=42)
    panel = Panel(dos, perm, c.prob)
    return c, panel, ind, Ref(c, panel, ind)


# more than 65 536 slots: 700 blocks of 100 SNPs, each padded to ld = roundup(m + 1, 32) = 128 slots
B_M, B_NB, B_NREF, B_NTOTAL = 100, 700, 64, 7
B_SLOTS = B_NB * 128
B_SAMPLE = [0, 65536 // 128 - 1, 65536 // 128, B_NB - 1]   # first, around slot 65 536, last


@functools.lru_cache(maxsize=None)
def big():
    from dbslmm_amd import BlockProblem
    from dbslmm_amd.synth import BED_MAGIC, pack_dosages
    rng = np.random.default_rng(51)
    total = B_M * B_NB
    dos = rng.integers(0, 3, size=(total, B_NREF), dtype=np.int8)
    dos[rng.random(dos.shape) < 0.002] = -1
    bed = np.concatenate([np.frombuffer(BED_MAGIC, dtype=np.uint8), pack_dosages(dos).reshape(-1)])
    bid = np.repeat(np.arange(B_NB), B_M)
    large = (np.arange(total) % B_M) >= B_M - (bid % 3)        # 0, 1 or 2 large SNPs, the last of the block
    z = rng.standard_normal(total)

    def csr(mask):
        idx = np.flatnonzero(mask)
        ptr = np.zeros(B_NB + 1, dtype=np.int64)
        np.add.at(ptr, bid[idx] + 1, 1)
        return np.cumsum(ptr), idx.astype(np.int32), z[idx]
    s_ptr, s_pos, z_s = csr(~large)
    l_ptr, l_pos, z_l = csr(large)
    prob = BlockProblem(bed=bed, n_ref=B_NREF, n_obs=N_OBS, sigma_s=V_SIGMA, tau=0.8, s_ptr=s_ptr, s_pos=s_pos,
                        z_s=z_s, l_ptr=l_ptr, l_pos=l_pos, z_l=z_l)

    class C:
        pass
    c = C()
    c.prob, c.blocks = prob, [(B_M, int(b % 3), None) for b in range(B_NB)]
    ind = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)          # n_test = 5, the last selected
    tdos = rng.integers(0, 3, size=(total, B_NTOTAL), dtype=np.int8)
    tdos[:, 0], tdos[:, 2] = 0, 2                                  # no SNP without variance among the selected
    panel = Panel(tdos, rng.permutation(total), prob)
    return c, panel, ind, Ref(c, panel, ind, blocks=B_SAMPLE)


# ----------------------------------------------------------------------------- CPU tests
def test_builder_self_checks():
    c, panel, ind, _ = ladder()
    p = c.prob
    assert [(m, ml) for m, ml, _ in c.blocks] == list(LADDER) and EMPTY not in c.keep
    ms = [m - ml for m, ml in LADDER]
    sizes = {m for m, _ in LADDER}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129} <= sizes
    assert {m % 32 for m in sizes if m} >= {0, 1, 31}
    with_large = [(m, ml) for m, ml in LADDER if 0 < ml < m]
    assert {ml for m, ml in with_large if (m - ml) % 32 == 0} >= {1, 9}
    assert {(m - ml) % 8 for m, ml in with_large} >= {0, 1, 7}
    assert sum(1 for m, ml in LADDER if m - ml == 1 and ml >= 31) >= 3
    assert sum(1 for m, ml in LADDER if m and ml == m) >= 4
    for b, (m, ml) in enumerate(LADDER):
        assert p.s_ptr[b + 1] - p.s_ptr[b] == ms[b] and p.l_ptr[b + 1] - p.l_ptr[b] == ml
    assert int(ind.sum()) > 64 and panel.n_total == 150
    # every SNP's test row is its own
    assert len(set(panel.ts_pos.tolist()) | set(panel.tl_pos.tolist())) == p.n_s + p.n_l
    for n_total, n_test, mode in SELECTIONS:
        _, pn, sel, _ = small(n_total, n_test, mode)
        assert pn.n_total == n_total and int(sel.sum()) == n_test
        assert mode == "first_only" or sel[-1] == 1
    assert {n for _, n, _ in SELECTIONS} >= {1, 2, 3, 63, 64, 65, 127, 128, 129}
    assert {t % 4 for t, _, m in SELECTIONS if m == "last"} == {0, 1, 3}
    assert {t % 4 for t, _, m in SELECTIONS if m == "all"} == {0, 1, 3}
    assert B_SLOTS > 65536 and B_SAMPLE[2] * 128 == 65536


def test_reference_equals_literal_formulas():
    """The longdouble factor form against calc_nt_by_nt_matrix's literal formulas (fp64, explicit
    inverses) on every block of the ladder, the blocks of large SNPs only through nt_diag_ls with
    empty small-SNP matrices.  Bar 1e-10 per column: the literal side inverts A and the Schur
    complement in fp64 (kappa <= 5 x 130 / 0.3, m <= 129: m eps kappa <= 4e-11)."""
    c, panel, ind, ref = ladder()
    p = c.prob
    D = ref.diags()
    lit = np.zeros(D.shape)
    for b in c.keep:
        rs, rl, ts, tl = ref.rows(b)
        Xs, Xl = R.read_block_matrix(p.bed, rs, p.n_ref), R.read_block_matrix(p.bed, rl, p.n_ref)
        Ts, Tl = R.read_test_block_matrix(panel.tbed, ts, ind), R.read_test_block_matrix(panel.tbed, tl, ind)
        ss, sl, ll = R.block_sigmas(Xs, Xl, p.n_ref, p.tau)
        if rl.size:
            lit[:, b] = R.nt_diag_ls(ll, sl, ss, p.sigma_s, p.n_obs, Tl, Ts)
        else:
            lit[:, b] = R.nt_diag_s(ss, p.sigma_s, p.n_obs, Ts)
    assert np.all(np.isfinite(lit)) and np.all(lit >= 0) and np.all(lit[:, EMPTY] == 0)
    assert np.all(lit[:, c.keep].max(0) > 0)          # (an imputed call of a one-SNP block is x = 0: a zero entry)
    err = column_errors(lit, D)
    print(f"longdouble factor form vs the literal formulas: worst column {max(err.values()):.2e}")
    assert max(err.values()) < 1e-10
    # the all-large blocks: x_l^T Sigma_ll^-1 x_l / n, not 0
    for b in c.keep:
        if LADDER[b][0] == LADDER[b][1]:
            _, rl, _, tl = ref.rows(b)
            Xl = R.read_block_matrix(p.bed, rl, p.n_ref)
            Tl = R.read_test_block_matrix(panel.tbed, tl, ind)
            ll = R.block_sigmas(Xl, None, p.n_ref, p.tau)[0]
            want = np.einsum("ti,ij,tj->t", Tl, np.linalg.inv(ll), Tl) / p.n_obs
            assert np.max(np.abs(lit[:, b] - want)) < 1e-12 * np.max(want) and np.max(want) > 0


def test_restatements_follow_the_literal_formulas_on_all_large_blocks():
    """ref_numpy.variance_diags and test_variance.synth_oracle on a problem with an all-large and
    an empty block: the longdouble reference's columns, the empty block's zero."""
    from test_variance import synth_oracle
    c, panel, ind, ref = small(132, 132, "all")
    p = c.prob
    D = ref.diags()
    got = synth_oracle(p, panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    bid_s = np.repeat(np.arange(p.num_block), np.diff(p.s_ptr))
    bid_l = np.repeat(np.arange(p.num_block), np.diff(p.l_ptr))
    info = lambda pos, bid: [dict(pos=int(r), block=int(b)) for r, b in zip(pos, bid)]
    got2 = R.variance_diags(p.bed, p.n_ref, p.n_obs, p.sigma_s, p.num_block, info(p.s_pos, bid_s), info(p.l_pos, bid_l),
                            panel.tbed, ind, info(panel.ts_pos, bid_s), info(panel.tl_pos, bid_l), tau=p.tau)
    all_large = [b for b, (m, ml) in enumerate(SMALL) if m and m == ml]
    assert all_large and np.all(D[:, all_large].max(0) > 0)
    for g in (got, got2):
        assert np.all(g[:, SMALL.index((0, 0))] == 0)
        assert worst_column(g, D) < 1e-10


CPU_CASES = {
    "ladder": lambda: (ladder()[3], [None, 1.2 * V_SIGMA, PCG_SIGMA, 1.2 * PCG_SIGMA]),
    "ladder_tau1": lambda: (ladder(1.0)[3], [None]),
    "dup": lambda: (dup()[3], [None]),
    "dup_emptied": lambda: (dup(True)[3], [None]),
    "big": lambda: (big()[3], [None]),
}


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_preconditions_from_the_reference_alone(name):
    """From the two evaluations of the reference alone: every block meant to be healthy has a finite,
    positive longdouble column and the fp64 floor of every case stays below 1e-9, so 10 x floor is
    the bar and the 1e-8 cap never binds; the blocks with a duplicated row fail the longdouble
    Cholesky (NaN column).  tau = 1: the floor is printed and held to the same 1e-9."""
    ref, sigmas = CPU_CASES[name]()
    c = ref.c
    for sg in sigmas:
        D = ref.diags(sg)
        for b in ref.blocks:
            m, _, dupl = c.blocks[b]
            if m == 0 or (name == "dup_emptied" and dupl is not None):
                assert np.all(D[:, b] == 0), b
            elif dupl is not None:
                assert np.all(np.isnan(D[:, b])), b
            else:
                assert np.all(np.isfinite(D[:, b])) and np.all(D[:, b] >= 0) and D[:, b].max() > 0, (b, c.blocks[b])
        floor = ref.floor(sg)
        print(f"{name} sigma {ref.p.sigma_s if sg is None else sg:.3g} (d = "
              f"{1.0 / ((ref.p.sigma_s if sg is None else sg) * ref.p.n_obs):.3g}): fp64 floor {floor:.2e}, "
              f"bar {ref.bar(sg):.2e}")
        assert 0.0 < floor < 1e-9, (name, sg, floor)


def test_preconditions_of_the_small_cases():
    """Every selection: block 0 is finite from n_test = 2 on, n_test = 1 makes every non-empty
    column NaN (0/0 in the N - 1 sd), the empty block is zero; floors below 1e-9."""
    worst = 0.0
    for n_total, n_test, mode in SELECTIONS:
        c, _, _, ref = small(n_total, n_test, mode)
        D = ref.diags()
        assert np.all(D[:, SMALL.index((0, 0))] == 0)
        if n_test == 1:
            assert np.all(np.isnan(D[:, c.keep]))
            continue
        assert np.all(np.isfinite(D[:, 0])) and np.all(D[:, 0] > 0), (n_total, n_test, mode)
        if n_test >= 63:
            assert np.all(np.isfinite(D)), (n_total, n_test, mode)
        worst = max(worst, ref.floor())
        assert 0.0 < ref.floor() < 1e-9, (n_total, n_test, mode, ref.floor())
    print(f"small cases: worst fp64 floor {worst:.2e}")


# ----------------------------------------------------------------------------- GPU plumbing
def variant(c, sigma_s=None, **opts):
    return dataclasses.replace(c.prob, sigma_s=c.prob.sigma_s if sigma_s is None else sigma_s, opts=dict(opts))


def gpu_variance(c, panel, ind, devices=0, sigmas=None, **opts):
    """The variance after run() (sigmas None) or run_multi(sigmas) on a fresh plan, with the
    run's results and workload."""
    from dbslmm_amd import Plan
    plan = Plan(ctx(devices), variant(c, **opts))
    if sigmas is None:
        plan.run()
        res = plan.download()
    else:
        res = plan.run_multi(sigmas)
    wl = plan.workload()
    got = plan.variance(panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    plan.close()
    return got, res, wl


_LADDER_RUNS = {}


def ladder_run(path, tau=0.8):
    if (path, tau) not in _LADDER_RUNS:
        c, panel, ind, _ = ladder(tau)
        _LADDER_RUNS[path, tau] = gpu_variance(c, panel, ind, **PATHS[path])
    return _LADDER_RUNS[path, tau]


# ----------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.8, 1.0])
@pytest.mark.parametrize("path", list(PATHS))
def test_ladder_against_longdouble(path, tau):
    """Case 1: every block of the ladder on its own scale; blocks of >= 64 SNPs on the tiled
    factor path (tiled_min = 64) and on the one-workgroup path, the others on the one-wave path."""
    c, _, _, ref = ladder(tau)
    got, res, wl = ladder_run(path, tau)
    n_big = sum(1 for m, _ in LADDER if m >= 64)
    assert wl["pcg_route"] == 0
    assert (wl["blocks_tiled"], wl["blocks_large"]) == ((n_big, 0) if path == "tiled64" else (0, n_big))
    assert np.all(res[2][c.keep] == 0) and res[2][EMPTY] == 1
    assert np.all(got[:, EMPTY] == 0)
    held(got, ref, what=f"ladder tau {tau} {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_total,n_test,mode", SELECTIONS, ids=[f"{m}-{n}of{t}" for t, n, m in SELECTIONS])
def test_test_individuals(n_total, n_test, mode):
    """Case 2."""
    c, panel, ind, ref = small(n_total, n_test, mode)
    got, _, _ = gpu_variance(c, panel, ind)
    assert got.shape == (n_test, len(SMALL))
    assert np.all(got[:, SMALL.index((0, 0))] == 0)
    if n_test == 1:
        assert np.all(np.isnan(got[:, c.keep])), got
        return
    held(got, ref, what=f"{mode} {n_test} of {n_total}")


@pytest.mark.gpu
def test_test_panel_rows():
    """Case 3: the panel's rows in two layouts (a permutation; identity with the needed rows
    reaching row 0 and the last row of the .bed) give the same bits; missing calls among the
    selected; a SNP without any observed call among the selected: its column NaN, the others
    bit for bit those of the panel where it is observed."""
    c = case_small()
    n_total = 131
    ind = selection(n_total, 70, "last", seed=7)
    sel = np.flatnonzero(ind)
    total = sum(m for m, _ in SMALL)
    dos = random_dosages(total, n_total, seed=61)
    j = SMALL[0][0] + 2                                   # a small SNP of block 1: 9 missing among the selected
    dos[j, sel[:9]] = -1
    dos[j, sel[9]], dos[j, sel[10]] = 0, 2
    ident = Panel(dos, np.arange(total), c.prob)
    assert {0, total - 1} <= set(ident.ts_pos.tolist()) | set(ident.tl_pos.tolist())
    assert ident.tbed.size == 3 + total * ((n_total + 3) // 4)
    shuffled = Panel(np.concatenate([dos, random_dosages(5, n_total, seed=62)]),
                     np.random.default_rng(63).permutation(total + 5), c.prob)
    ref = Ref(c, ident, ind)
    assert np.all(np.isfinite(ref.diags()))
    a, _, _ = gpu_variance(c, ident, ind)
    b, _, _ = gpu_variance(c, shuffled, ind)
    np.testing.assert_array_equal(a, b)
    held(a, ref, what="panel rows, 9 missing calls in one SNP")
    gone = dos.copy()
    gone[j, sel] = -1                                      # (the unselected keep their calls)
    assert np.any(gone[j] >= 0)
    pg = Panel(gone, np.arange(total), c.prob)
    rg = Ref(c, pg, ind)
    assert np.all(np.isnan(rg.diags()[:, 1])) and np.all(np.isfinite(rg.diags()[:, [0, 2, 3, 4]]))
    g, _, _ = gpu_variance(c, pg, ind)
    assert np.all(np.isnan(g[:, 1]))
    np.testing.assert_array_equal(g[:, [0, 2, 3, 4]], a[:, [0, 2, 3, 4]])
    # no variance among the observed selected calls and three missing ones: nomalizeVec's 0/0 for
    # every individual, the imputed ones included
    mono = dos.copy()
    mono[j, sel] = 1
    mono[j, sel[:3]] = -1
    pm = Panel(mono, np.arange(total), c.prob)
    assert np.all(np.isnan(Ref(c, pm, ind).diags()[:, 1]))
    g, _, _ = gpu_variance(c, pm, ind)
    assert np.all(np.isnan(g[:, 1])), g[:, 1]
    np.testing.assert_array_equal(g[:, [0, 2, 3, 4]], a[:, [0, 2, 3, 4]])


H2F = (0.8, 1.0, 1.2)
ITER = {"cheb": dict(h2f_iter=1), "cg": dict(h2f_iter=2)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_factor_after_run_is_stable(path):
    """Case 4, run(): two variance() calls in a row give the same bits, and so does a fresh plan."""
    from dbslmm_amd import Plan
    c, panel, ind, ref = ladder()
    plan = Plan(ctx(), variant(c, **PATHS[path]))
    plan.run()
    one = plan.variance(panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    two = plan.variance(panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    plan.close()
    np.testing.assert_array_equal(one, two)
    np.testing.assert_array_equal(one, ladder_run(path)[0])
    held(one, ref, what=f"after run() {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_factor_after_run_multi_last_copy_factored(path):
    """Case 4: two copies, the base (the factored copy) is the last one."""
    c, panel, ind, ref = ladder()
    sig = [0.8 * V_SIGMA, 1.2 * V_SIGMA]
    got, _, wl = gpu_variance(c, panel, ind, sigmas=sig, **PATHS[path])
    assert wl["cheb_base"] == 1 and wl["cheb_iters"] > 0
    held(got, ref, sigma=sig[-1], what=f"run_multi, last copy factored, {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("it", list(ITER))
@pytest.mark.parametrize("path", list(PATHS))
def test_factor_after_run_multi_last_copy_iterated(path, it):
    """Case 4: three copies, the base is the middle one and the last was iterated on its factor:
    the variance re-solves the last sigma; twice the same bits; a run_multi after the variance
    gives the betas of one without, bit for bit."""
    from dbslmm_amd import Plan
    c, panel, ind, ref = ladder()
    sig = [V_SIGMA * f for f in H2F]
    plan = Plan(ctx(), variant(c, **PATHS[path], **ITER[it]))
    first = plan.run_multi(sig)
    first = [tuple(a.copy() for a in r) for r in first]
    wl = plan.workload()
    assert wl["cheb_base"] == 1 and wl["cheb_iters"] > 0 and wl["pcg_route"] == 0
    one = plan.variance(panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    two = plan.variance(panel.tbed, ind, panel.ts_pos, panel.tl_pos)
    again = plan.run_multi(sig)
    plan.close()
    np.testing.assert_array_equal(one, two)
    held(one, ref, sigma=sig[-1], what=f"run_multi, last copy iterated ({it}), {path}")
    for k in range(len(sig)):
        for x, y in zip(first[k], again[k]):
            np.testing.assert_array_equal(x, y, err_msg=f"copy {k} after a variance")


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True], ids=["run", "run_multi"])
def test_factor_after_pcg_route(multi):
    """Case 4: a PCG-route run (solver = 2) at the flagship's prior shift d = 20 leaves no factor:
    the variance factors the last sigma first."""
    c, panel, ind, ref = ladder()
    sig = [PCG_SIGMA * f for f in H2F] if multi else None
    got, _, wl = gpu_variance(c, panel, ind, sigmas=sig, sigma_s=PCG_SIGMA, solver=2)
    assert wl["pcg_route"] == 1
    last = sig[-1] if multi else PCG_SIGMA
    assert 0.0 < ref.floor(last) < 1e-9
    held(got, ref, sigma=last, what=f"after a PCG-route {'run_multi' if multi else 'run'}")


@pytest.mark.gpu
def test_not_pd_block_beside_healthy_blocks():
    """Case 5: the blocks with a duplicated row fail (status 2) and their columns are NaN; every
    other column is, bit for bit, that of the problem without them, and within its bar."""
    c, panel, ind, ref = dup()
    e, epanel, eind, _ = dup(True)
    np.testing.assert_array_equal(panel.tbed, epanel.tbed)
    got, res, _ = gpu_variance(c, panel, ind, tiled_min=64)
    alone, eres, _ = gpu_variance(e, epanel, eind, tiled_min=64)
    assert c.fail == [1, 4, 6]
    assert res[2].tolist() == [0, 2, 0, 1, 2, 0, 2, 0] and eres[2].tolist() == [0, 1, 0, 1, 1, 0, 1, 0]
    assert np.all(np.isnan(got[:, c.fail]))
    assert np.all(alone[:, c.fail] == 0)
    np.testing.assert_array_equal(got[:, c.healthy], alone[:, c.healthy])
    held(got, ref, what="beside NOT_PD blocks")


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_three_shards_on_one_device(path):
    """Case 7."""
    c, panel, ind, _ = ladder()
    got, res, _ = gpu_variance(c, panel, ind, devices=[0, 0, 0], **PATHS[path])
    one, one_res, _ = ladder_run(path)
    np.testing.assert_array_equal(got, one)
    for x, y in zip(res, one_res):
        np.testing.assert_array_equal(x, y)
    all_large = [b for b, (m, ml) in enumerate(LADDER) if m and m == ml]
    assert np.all(got[:, all_large].max(0) > 0) and np.all(got[:, EMPTY] == 0)


@pytest.mark.gpu
def test_more_than_65536_slots():
    """Case 6: 700 blocks of 100 SNPs = 89 600 slots; the first and the last block and the two
    around slot 65 536 against the reference, every column finite and positive."""
    c, panel, ind, ref = big()
    got, res, _ = gpu_variance(c, panel, ind)
    assert np.all(res[2] == 0)
    assert got.shape == (5, B_NB)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    held(got, ref, what="89 600 slots")

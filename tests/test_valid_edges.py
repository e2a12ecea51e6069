"""`valid_blocks` (dbslmm_valid_partial / dbslmm_valid_reduce, the whole numeric result of the `valid`
tool), `read_snp_std` and the `valid` CLI at their shape edges: more than one 4096-individual
chunk, pad bits, CSR shapes, degenerate rows, more blocks than a grid has rows, major-allele rows.

Reference: exact_valid() in this module, np.longdouble from exact integers.  Per panel row the
observed-call count, the dosage sum S and the sum of squares sq are integers; mu = S / count,
css = (count sq - S^2) / count with the numerator formed as an exact integer, sd = sqrt(css / (n - 1)),
y_i = sum_j z1_j (g_ij - mu_j) / sd_j (a missing call contributes 0), deno_b = sum_i y_i^2 / n.
A block with a row that has count == 0 or css == 0 is NaN; an empty block is exactly 0.
nume_b = sum_j z1_j z2_j is host arithmetic: it must equal the same sequential fp64 loop.

The bar (derived from kernels.hip, not measured), per block, u = 2^-53, m_b = rows of the block:

  |got - ref| <= 2 [ (1/n) sum_i (2 |y_i| E_i + E_i^2) + c_red u deno ]
  E_i = sum_j |z1_j| / sd_j ( |g_ij - mu_j| ((m_b + c_row) u + rho_j) + u mu_j [g_ij observed, g_ij != 0] )

* rho_j, the relative error of the fp64 1/sd_j of row_moments: count, S, sq convert exactly and
  S S is exact (S^2 < 2^53).  t = S^2 / count rounds once (u S^2 / count absolute) and the
  subtraction sq - t rounds once more: css carries u (1 + q_j), q_j = S_j^2 / (count_j css_j).  The
  division by n - 1 (u), the sqrt (halves what came before, adds u) and the reciprocal (u) follow:
  rho_j <= u (3 + q_j / 2).  The bar uses rho_j = u (c + q_j), c = 3, the form without the half.
* c_row = 3: of one term (g - mu_j) (z1_j rsd_j), the subtraction rounds (u), the weight z1_j rsd_j
  rounds (u, beside rho_j) and the product rounds (u); the term is then added into y_i, a chain of
  m_b additions ((m_b) u on the sum of the |terms|).
* u mu_j: the subtraction takes the ROUNDED mean, off by u mu_j.  For g = 0 the difference is the
  rounded mean itself (already the u of the subtraction); for an observed g = 1 or 2 it is an
  absolute error that |g - mu_j| does not scale (mu_j = 2 - 1/n against g = 2), so it stands by
  itself.  A missing call is mu - mu = 0 exactly.
* c_red = 28 + n_chunks: sum_i y_i^2 adds non-negative terms only -- the square (1), 16 additions per
  lane, 6 shuffle steps, 4 waves, n_chunks partials, the division by n (1).
* the leading 2 is the factor test_score.py allows itself (second-order terms, and the reference's
  own 2^-64 roundings).

The bar must still say something: every parity block checks bound <= 1e-9 deno on the CPU, from the
reference alone.  Exempt: the block built to cancel (two identical rows, z1 = (+a, -a): deno == 0.0
exactly, the kernel rounds each term once and only adds).  The major-allele case (q_j ~ 4 n) also
states its own limit, 16 max_j rho_j.

Observed on the MI355X, worst |got - ref| / bound (and the worst bound / deno) per case:
  ladder n_ref <= 65      0.0004 .. 0.008   (5e-14 .. 3e-13)
  ladder 4095             0.0045            (1.3e-13)
  ladder 4096, 4097       0.0001 .. 0.0007  (3.9e-13 .. 5.2e-13)
  ladder 8200             0.024             (2.2e-12)
  csr                     0.024             (9.3e-13)
  degenerate              0.022             (1.5e-14)
  300 blocks              0.064             (7.1e-12)
  65 835 blocks           0.11              (1.3e-13)
  major allele            0.058             (1.2e-11)
The bar is a worst case over every rounding, so a healthy kernel sits one to three decimal orders
below it; the wrong kernels this module was tried against (the reduce summing chunk 0 only, the
tail mask dropped, a missing call taken as dosage 0) miss it by many orders.  With the y
accumulation fused (an FMA of the unrounded product) the cancelling block returned 3.3e-33, not 0.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import ref_numpy as R
from _common import ROOT
from test_row_stats import C_MISS, C_ONE, C_TWO, C_ZERO, FILLS, _bed

LD = np.longdouble
U = LD(2.0) ** -53
C_ROW, C_RHO = 3, 3
N_ROWS = 37
VALID = os.path.join(ROOT, "dbslmm_amd", "bin", "valid")

# rows of _vcodes (0..15 random and polymorphic by construction, 16..25 random)
R_MAJOR = range(26, 30)          # all 00 but one or two heterozygotes (S ~ 2 n)
R_TWO, R_ZERO, R_MISS, R_SINGLE, R_HET, R_LASTMISS, R_FIRSTMISS = 30, 31, 32, 33, 34, 35, 36


def n_chunks_of(n_ref):
    return ((n_ref + 15) // 16 + 255) // 256


@functools.lru_cache(maxsize=None)
def _vcodes(n_ref, miss):
    """(N_ROWS, n_ref) 2-bit codes, a sibling of test_row_stats._codes that holds for n_ref >= 2 and
    carries the rows this module needs: 16 random rows made polymorphic by a dosage 2 at individual
    0 and a dosage 0 at individual 1 (never missing), 10 random rows, 4 major-allele rows (all 00
    but 1, 2, 1, 2 heterozygotes; the last two with a missing call as well), then all 00, all 11,
    all missing, one observed call, all heterozygous, and rows 0 / 1 again with the last / the first
    call missing."""
    rng = np.random.default_rng(7000 * n_ref + int(1000 * miss))
    c = rng.choice(np.array([C_TWO, C_ONE, C_ZERO], dtype=np.uint8), size=(N_ROWS, n_ref), p=[0.2, 0.4, 0.4])
    c[:26][rng.random((26, n_ref)) < miss] = C_MISS
    c[:16, 0] = C_TWO
    c[:16, 1] = C_ZERO
    c[26:30] = C_TWO
    c[26, n_ref // 2] = C_ONE
    c[27, [n_ref // 3, n_ref - 1]] = C_ONE
    c[28, 0] = C_ONE
    c[28, n_ref - 1] = C_MISS
    c[29, [1, n_ref - 2]] = C_ONE
    c[29, n_ref // 2] = C_MISS
    c[R_TWO] = C_TWO
    c[R_ZERO] = C_ZERO
    c[R_MISS] = C_MISS
    c[R_SINGLE] = C_MISS
    c[R_SINGLE, n_ref // 2] = C_ONE
    c[R_HET] = C_ONE
    c[R_LASTMISS] = c[0]
    c[R_LASTMISS, n_ref - 1] = C_MISS
    c[R_FIRSTMISS] = c[1]
    c[R_FIRSTMISS, 0] = C_MISS
    c.setflags(write=False)
    return c


# ----------------------------------------------------------------------------- the reference
def row_table(codes):
    """exact integers per row: count of observed calls, S, sq, and count sq - S^2"""
    c = np.asarray(codes)
    two, one, mis = (c == C_TWO).sum(1).astype(np.int64), (c == C_ONE).sum(1).astype(np.int64), \
        (c == C_MISS).sum(1).astype(np.int64)
    count = c.shape[1] - mis
    S, sq = 2 * two + one, 4 * two + one
    assert int(S.max(initial=0)) ** 2 < 2 ** 53
    return count, S, sq, count * sq - S * S


def finite_rows(codes):
    """rows with a finite standard deviation, from the exact integers"""
    count, _, _, num = row_table(codes)
    return [int(r) for r in np.flatnonzero((count > 0) & (num > 0))]


class Ref:
    """deno, bound, use (bound / deno, NaN where that says nothing) in longdouble; nume in fp64"""


def seq_dot(z1, z2):
    t = 0.0
    for a, b in zip(z1.tolist(), z2.tolist()):
        t += a * b
    return t


def exact_valid(codes, n_ref, ptr, pos, z1, z2=None):
    codes = np.asarray(codes)
    assert codes.shape[1] == n_ref
    ptr, pos = np.asarray(ptr, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    z1 = np.asarray(z1, dtype=np.float64)
    count, S, sq, num = row_table(codes)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = S.astype(LD) / count.astype(LD)
        css = num.astype(LD) / count.astype(LD)
        sd = np.sqrt(css / LD(n_ref - 1))
        rho = U * (C_RHO + (S * S).astype(LD) / num.astype(LD))
    dose = np.array([2, 0, 1, 0], dtype=LD)                    # by PLINK code (01, missing: unused)
    nb = len(ptr) - 1
    c_red = 28 + n_chunks_of(n_ref)
    out = Ref()
    out.deno, out.bound, out.nume = np.zeros(nb, dtype=LD), np.zeros(nb, dtype=LD), np.zeros(nb)
    for b in range(nb):
        sl = slice(int(ptr[b]), int(ptr[b + 1]))
        r = pos[sl]
        if z2 is not None:
            out.nume[b] = seq_dot(z1[sl], np.asarray(z2, dtype=np.float64)[sl])
        if r.size == 0:
            continue
        if np.any((count[r] == 0) | (num[r] == 0)):
            out.deno[b] = out.bound[b] = np.nan
            continue
        c = codes[r]
        obs = c != C_MISS
        dev = np.where(obs, dose[c] - mu[r, None], LD(0))
        a = z1[sl].astype(LD) / sd[r]
        y = (a[:, None] * dev).sum(axis=0)
        k = (r.size + C_ROW) * U + rho[r]
        E = (np.abs(a)[:, None] * (np.abs(dev) * k[:, None] + U * mu[r, None] * (obs & (c != C_ZERO)))).sum(axis=0)
        out.deno[b] = (y * y).sum() / LD(n_ref)
        out.bound[b] = 2 * ((2 * np.abs(y) * E + E * E).sum() / LD(n_ref) + c_red * U * out.deno[b])
    with np.errstate(divide="ignore", invalid="ignore"):
        out.use = out.bound / out.deno
    out.rho = rho
    return out


# ----------------------------------------------------------------------------- the cases
class Case:
    """codes, n_ref, the CSR (ptr, pos, z1, z2), the reference, nan = the blocks that must be NaN,
    exempt = the blocks whose bar need not be useful (built to cancel), zero = blocks that are 0.0"""

    def __init__(self, name, codes, blocks, seed, z1_of=None, nan=(), exempt=(), zero=(), ref_blocks=None):
        self.name, self.codes, self.n_ref = name, codes, codes.shape[1]
        self.ptr = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
        self.pos = np.array([r for b in blocks for r in b], dtype=np.int32)
        rng = np.random.default_rng(seed)
        self.z1, self.z2 = rng.standard_normal(self.pos.size), rng.standard_normal(self.pos.size)
        if z1_of is not None:
            z1_of(self)
        self.nan, self.exempt, self.zero = set(nan), set(exempt), set(zero)
        # the blocks held to the reference (all of them unless the case has too many)
        self.ref_blocks = np.arange(len(blocks)) if ref_blocks is None else np.asarray(ref_blocks)
        sub_ptr = np.concatenate([[0], np.cumsum(np.diff(self.ptr)[self.ref_blocks])]).astype(np.int64)
        idx = np.concatenate([np.arange(self.ptr[b], self.ptr[b + 1]) for b in self.ref_blocks] +
                             [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        self.ref = exact_valid(codes, self.n_ref, sub_ptr, self.pos[idx], self.z1[idx], self.z2[idx])

    def bed(self, fill=FILLS[0]):
        return _bed(self.codes, fill)

    def precheck(self):
        """on the CPU, from the reference alone: NaN exactly where the case says, empty blocks 0,
        and a bar that still says something on every other block"""
        sizes = np.diff(self.ptr)[self.ref_blocks]
        for k, b in enumerate(self.ref_blocks):
            d, use = self.ref.deno[k], self.ref.use[k]
            if int(b) in self.nan:
                assert np.isnan(d), (self.name, b)
            elif sizes[k] == 0 or int(b) in self.zero:
                assert d == 0, (self.name, b)
            else:
                assert np.isfinite(d) and d > 0, (self.name, b)
                if int(b) not in self.exempt:
                    assert use <= 1e-9, (self.name, b, float(use))

    def check(self, gn, gd, what=""):
        """the GPU's (nume, deno) against the reference: returns the worst |got - ref| / bound"""
        assert gn.shape == gd.shape == (len(self.ptr) - 1,)
        np.testing.assert_array_equal(gn[self.ref_blocks], self.ref.nume)          # host arithmetic: ==
        sizes = np.diff(self.ptr)
        worst = 0.0
        for k, b in enumerate(self.ref_blocks):
            d, bound = self.ref.deno[k], self.ref.bound[k]
            if np.isnan(d):
                assert np.isnan(gd[b]), (self.name, what, b, gd[b])
            elif sizes[b] == 0 or int(b) in self.zero:
                assert gd[b] == 0.0, (self.name, what, b, gd[b])
            else:
                assert np.isfinite(gd[b]), (self.name, what, b)
                err = abs(LD(gd[b]) - d)
                worst = max(worst, float(err / bound))
                assert err <= bound, (self.name, what, int(b), float(err), float(bound))
        use = self.ref.use[np.isfinite(self.ref.use)]
        print(f"valid {self.name} {what}: worst |got - ref| / bound = {worst:.3g}, "
              f"worst bound / deno = {float(use.max(initial=0)):.3g}")
        return worst


LADDER = [2, 5, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8200]
MISS = [0.0, 0.07]


@functools.lru_cache(maxsize=None)
def ladder_case(n_ref, miss):
    """one block of all finite-sd rows, in a shuffled order"""
    codes = _vcodes(n_ref, miss)
    rows = finite_rows(codes)
    rows = [rows[i] for i in np.random.default_rng(n_ref).permutation(len(rows))]
    return Case(f"ladder n={n_ref} miss={miss}", codes, [rows], seed=n_ref)


@functools.lru_cache(maxsize=None)
def csr_case():
    """n_ref = 4097: empty first / middle / last blocks, a one-row block, a row twice in a block and
    in two blocks, a descending block, twelve rows as one block and split in two"""
    codes = _vcodes(4097, 0.07)
    F = finite_rows(codes)
    assert len(F) >= 24
    blocks = [[], [], F[:5], [], [F[7]], [F[3], F[3], F[8]], F[2:6], sorted(F, reverse=True), F[:12], F[:6], F[6:12],
              [], []]
    def z1_of(c):                                              # the split halves carry the joint block's weights
        joint, halves = slice(c.ptr[8], c.ptr[9]), slice(c.ptr[9], c.ptr[11])
        c.z1[halves], c.z2[halves] = c.z1[joint], c.z2[joint]
    return Case("csr", codes, blocks, seed=41, z1_of=z1_of)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """n_ref = 4097: degenerate rows in blocks of their own between healthy ones; block 10 is built
    to cancel (exempt from the usefulness check)"""
    codes = _vcodes(4097, 0.07)
    F = [r for r in finite_rows(codes) if r not in R_MAJOR]
    blocks = [F[:4], [F[4], R_TWO, F[5]], F[4:9], [R_MISS, F[9]], F[9:12], [R_SINGLE], F[12:15],
              [F[15], R_HET, F[16]], F[15:19], [R_ZERO], [F[2], F[2]], F[1:3]]

    def z1_of(c):
        c.z1[c.ptr[7] + 1] = 0.0                               # the monomorphic row with z1 = 0: still NaN
        c.z1[c.ptr[10] + 1] = -c.z1[c.ptr[10]]
    return Case("degenerate", codes, blocks, seed=43, z1_of=z1_of, nan=(1, 3, 5, 7, 9), exempt=(10,), zero=(10,))


@functools.lru_cache(maxsize=None)
def many_case():
    """300 blocks of 0 to 3 rows at n_ref = 4097: the second workgroup of dbslmm_valid_reduce"""
    codes = _vcodes(4097, 0.0)
    F = finite_rows(codes)
    blocks = [[F[(5 * b + k) % len(F)] for k in range(b % 4)] for b in range(300)]
    return Case("300 blocks", codes, blocks, seed=47)


GRID_ROWS = 65535
N_HUGE = GRID_ROWS + 300


@functools.lru_cache(maxsize=None)
def huge_case():
    """65 835 blocks at n_ref = 65, one row or (every 7th) none per block: more blocks than a grid
    has rows.  The first, the last and the blocks around 65 535 are held to the reference."""
    codes = _vcodes(65, 0.07)
    F = finite_rows(codes)
    blocks = [[] if b % 7 == 3 else [F[b % len(F)]] for b in range(N_HUGE)]
    near = np.concatenate([np.arange(0, 16), np.arange(GRID_ROWS - 16, GRID_ROWS + 16), np.arange(N_HUGE - 16, N_HUGE)])
    return Case("65835 blocks", codes, blocks, seed=53, ref_blocks=near)


@functools.lru_cache(maxsize=None)
def major_case():
    """n_ref = 8200: the major-allele rows (S ~ 2 n, css ~ 1 or 2 against sq ~ 4 n) drive z1, the
    other rows of the block are scaled down by 1e-3"""
    codes = _vcodes(8200, 0.07)
    quiet = [r for r in finite_rows(codes) if r not in R_MAJOR][:8]

    def z1_of(c):
        c.z1[:] = np.abs(c.z1) + 0.5
        c.z1[np.isin(c.pos, quiet)] *= 1e-3
    return Case("major allele", codes, [list(R_MAJOR), list(R_MAJOR) + quiet, quiet[:3] + [26, 27]], seed=59, z1_of=z1_of)


ALL_CASES = [lambda n=n, m=m: ladder_case(n, m) for n in LADDER for m in MISS] + \
    [csr_case, degenerate_case, many_case, huge_case, major_case]


# ----------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("n_ref,miss", [(250, 0.0), (257, 0.07)])
def test_exact_valid_equals_the_restatement(n_ref, miss):
    """exact_valid against z1^T (X^T X / n) z1 of ref_numpy.read_block_matrix (what test_valid.py
    holds the GPU to), 1e-12 relative"""
    codes = _vcodes(n_ref, miss)
    F = [r for r in finite_rows(codes) if r < 28]           # (rows 28 and up have a missing call of their own)
    assert len(F) >= 24 and (miss == 0) == (not (codes[F] == C_MISS).any())
    c = Case("restatement", codes, [F[:9], [], F[9:10], F[5:24]], seed=n_ref)
    bed = c.bed()
    for b in range(4):
        sl = slice(c.ptr[b], c.ptr[b + 1])
        if b == 1:
            assert c.ref.deno[b] == 0 and c.ref.nume[b] == 0
            continue
        X = R.read_block_matrix(bed, c.pos[sl], n_ref)
        want = c.z1[sl] @ (X.T @ X / n_ref) @ c.z1[sl]
        assert abs(float(c.ref.deno[b]) - want) <= 1e-12 * abs(want)
        assert abs(c.ref.nume[b] - c.z1[sl] @ c.z2[sl]) <= 1e-12 * np.abs(c.z1[sl] * c.z2[sl]).sum()
    # a degenerate row makes its block NaN in both, whatever its weight
    for r in (R_TWO, R_MISS, R_SINGLE, R_HET, R_ZERO):
        ref = exact_valid(codes, n_ref, [0, 2], [F[0], r], [1.0, 0.0])
        X = R.read_block_matrix(bed, [F[0], r], n_ref)
        assert np.isnan(ref.deno[0]) and np.isnan(np.array([1.0, 0.0]) @ (X.T @ X / n_ref) @ np.array([1.0, 0.0]))


def test_preconditions_from_the_reference_alone():
    """Every GPU case reaches what it is built for, and its bar still says something."""
    assert np.finfo(LD).eps <= 2.0 ** -63                              # the reference is wider than fp64
    assert [n_chunks_of(n) for n in (2, 4096, 4097, 8192, 8200)] == [1, 1, 2, 2, 3]
    assert (8200 + 15) // 16 - 2 * 256 == 1 and 8200 % 16 == 8           # third chunk: one half-valid word
    for make in ALL_CASES:
        c = make()
        c.precheck()
        assert c.pos.size == 0 or set(c.pos.tolist()) <= set(range(N_ROWS))
    for n in LADDER:
        for m in MISS:
            c = ladder_case(n, m)
            assert c.ptr.tolist() == [0, c.pos.size] and c.pos.size >= (16 if n > 2 else 2)
            assert sorted(c.pos.tolist()) == finite_rows(c.codes)
            if m > 0 and n >= 63:
                assert (c.codes[c.pos] == C_MISS).any()
            if n % 4:                                           # the three pad fills differ in the image
                beds = [c.bed(f).reshape(-1)[3:].reshape(N_ROWS, -1)[:, -1] >> (2 * (n % 4)) for f in FILLS]
                assert not np.array_equal(beds[0], beds[1]) and not np.array_equal(beds[1], beds[2])
    c = csr_case()
    sizes = np.diff(c.ptr).tolist()
    assert sizes[:2] == [0, 0] and sizes[3] == 0 and sizes[-2:] == [0, 0] and sizes[4] == 1
    assert c.pos[c.ptr[5]] == c.pos[c.ptr[5] + 1] and set(c.pos[c.ptr[2]:c.ptr[3]]) & set(c.pos[c.ptr[6]:c.ptr[7]])
    assert np.all(np.diff(c.pos[c.ptr[7]:c.ptr[8]]) < 0)
    j = slice(c.ptr[8], c.ptr[9])
    assert np.array_equal(c.z1[j], c.z1[c.ptr[9]:c.ptr[11]]) and np.array_equal(c.pos[j], c.pos[c.ptr[9]:c.ptr[11]])
    d = degenerate_case()
    assert d.z1[d.ptr[7] + 1] == 0.0 and d.ref.deno[10] == 0 and d.ref.bound[10] > 0
    assert np.isnan(d.ref.deno).sum() == 5
    h = huge_case()
    assert len(h.ptr) - 1 == N_HUGE > GRID_ROWS and np.diff(h.ptr).max() == 1 and (np.diff(h.ptr) == 0).sum() > 9000
    assert len(many_case().ptr) - 1 > 256
    # major-allele rows: css is small against sq, and the case's own limit is what rho gives
    m = major_case()
    count, S, sq, num = row_table(m.codes)
    for r in R_MAJOR:
        assert S[r] >= 2 * count[r] - 2 and num[r] / count[r] < 2.01 and sq[r] > 4 * 8000
    rho = float(m.ref.rho[list(R_MAJOR)].max())
    assert 2.0 ** -53 * 3e4 < rho < 2.0 ** -53 * 4e4
    assert np.all(m.ref.use <= 16 * rho) and 16 * rho < 1e-9
    assert np.all(m.ref.use[:2] > 1e3 * float(U))           # ... and rho is what it consists of


# ----------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def ctx():
    from dbslmm_amd import Context
    c = Context(0)
    yield c
    c.close()


def run(ctx, case, fill=FILLS[0], bed=None):
    from dbslmm_amd import valid_blocks
    return valid_blocks(ctx, case.bed(fill) if bed is None else bed, case.n_ref, case.ptr, case.pos, case.z1, case.z2)


@pytest.mark.gpu
@pytest.mark.parametrize("miss", MISS)
@pytest.mark.parametrize("n_ref", LADDER)
def test_individuals_ladder(ctx, n_ref, miss):
    """1, 2 and 3 chunks, both sides of the chunk edge, a last chunk of one half-valid word; the pad
    fills 01 / 00 / 11 agree bit for bit."""
    c = ladder_case(n_ref, miss)
    outs = [run(ctx, c, fill) for fill in FILLS]
    c.check(*outs[0])
    for o in outs[1:]:
        np.testing.assert_array_equal(o[0], outs[0][0])
        np.testing.assert_array_equal(o[1], outs[0][1])


@pytest.mark.gpu
def test_csr_shapes(ctx):
    c = csr_case()
    gn, gd = run(ctx, c)
    c.check(gn, gd)
    # the same rows as one block and split in two: nume adds up in fp64 order per block
    j, h1, h2 = (slice(c.ptr[b], c.ptr[b + 1]) for b in (8, 9, 10))
    assert gn[8] == seq_dot(c.z1[j], c.z2[j]) and gn[9] == seq_dot(c.z1[h1], c.z2[h1]) and gn[10] == seq_dot(c.z1[h2], c.z2[h2])


@pytest.mark.gpu
def test_all_blocks_empty_and_no_block(ctx):
    from dbslmm_amd import valid_blocks
    bed = csr_case().bed()
    e = np.zeros(0)
    gn, gd = valid_blocks(ctx, bed, 4097, np.zeros(7, dtype=np.int64), e, e, e)
    assert gn.tolist() == [0.0] * 6 and gd.tolist() == [0.0] * 6
    gn, gd = valid_blocks(ctx, bed, 4097, np.zeros(1, dtype=np.int64), e, e, e)
    assert gn.shape == gd.shape == (0,)


@pytest.mark.gpu
def test_degenerate_rows_stay_in_their_block(ctx):
    """all 00, all missing, one observed call, a monomorphic row with z1 = 0, all 11: NaN exactly
    where the reference is NaN, every other block within the bar; two identical rows with weights
    (+a, -a) give 0.0 exactly."""
    c = degenerate_case()
    gn, gd = run(ctx, c)
    c.check(gn, gd)
    assert np.isnan(gd).tolist() == [b in c.nan for b in range(len(gd))]
    assert gd[10] == 0.0


@pytest.mark.gpu
def test_300_blocks(ctx):
    c = many_case()
    c.check(*run(ctx, c))


@pytest.mark.gpu
def test_more_blocks_than_grid_rows(ctx):
    """65 835 blocks: the launch does not depend on the grid-row limit."""
    c = huge_case()
    gn, gd = run(ctx, c)
    c.check(gn, gd)
    sizes = np.diff(c.ptr)
    assert np.all(gd[sizes == 0] == 0.0) and np.all(gn[sizes == 0] == 0.0)
    assert np.all(np.isfinite(gd[sizes == 1])) and np.all(gd[sizes == 1] > 0.0)
    np.testing.assert_array_equal(gn[sizes == 1], c.z1 * c.z2)
    # one finite row alone: deno = z1^2 (n - 1) / n, whichever row (the bar of a one-row block is a few
    # hundred u at n = 65: 1e-11 is far above it and far below a wrong block)
    want = c.z1 ** 2 * (64.0 / 65.0)
    assert np.all(np.abs(gd[sizes == 1] - want) <= 1e-11 * want)


@pytest.mark.gpu
def test_contexts(ctx):
    """uncached vs cached, one device vs Context([0, 0]), and a repeat: bit for bit"""
    from dbslmm_amd import Context
    c = csr_case()
    bed = c.bed()
    base = run(ctx, c, bed=bed)
    outs = [run(ctx, c, bed=bed)]
    c1 = Context(0)
    c1.cache_bed(bed)
    outs.append(run(c1, c, bed=bed))
    outs.append(run(c1, c, bed=bed))
    c1.close()
    c2 = Context([0, 0])
    outs.append(run(c2, c, bed=bed))
    c2.close()
    for o in outs:
        np.testing.assert_array_equal(o[0], base[0])
        np.testing.assert_array_equal(o[1], base[1])


@pytest.mark.gpu
def test_major_allele_rows(ctx):
    """css = sq - S^2 / count loses q ~ 4 n ulps on these rows; the bar carries that through rho."""
    c = major_case()
    c.check(*run(ctx, c))


# rows test_row_stats.py::test_consumers leaves out, mixed with finite ones: descending, one twice
STD_LIST = [R_FIRSTMISS, R_LASTMISS, R_HET, R_SINGLE, R_SINGLE, R_MISS, R_ZERO, R_TWO, 27, 26, 20, 7, 3, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_ref", [65, 4097])
def test_read_snp_std_on_degenerate_rows(ctx, n_ref):
    """NaN pattern of the oracle's normalize(read_snp_im(...)) column by column, finite columns
    within the bounds of test_consumers (1e-12, MAF 1e-14); bed_maf bit for bit the oracle's."""
    import oracle as O
    from dbslmm_amd import bed_maf, read_snp_std
    assert np.all(np.diff(STD_LIST) <= 0) and STD_LIST.count(R_SINGLE) == 2
    codes = _vcodes(n_ref, 0.07)
    idv = np.ones(n_ref, dtype=np.int32)
    fin = set(finite_rows(codes))
    for fill in FILLS:
        bed = _bed(codes, fill)
        np.testing.assert_array_equal(bed_maf(ctx, bed, n_ref, N_ROWS), O.bed_maf(bed, n_ref, N_ROWS))
        X, maf = read_snp_std(ctx, bed, n_ref, STD_LIST)
        for j, r in enumerate(STD_LIST):
            g, m = O.read_snp_im(bed, r, idv)
            with np.errstate(divide="ignore", invalid="ignore"):
                want = O.normalize(g)
            np.testing.assert_array_equal(np.isnan(X[:, j]), np.isnan(want))
            assert np.isnan(want).all() == (r not in fin) and np.isnan(want).any() == (r not in fin)
            if r in fin:
                np.testing.assert_allclose(X[:, j], want, rtol=0, atol=1e-12)
            assert abs(maf[j] - m) < 1e-14 or (np.isnan(m) and np.isnan(maf[j]))


# ----------------------------------------------------------------------------- the CLI
def _write_valid_inputs(tmp):
    """A bfile of 4100 individuals (two chunks), 400 SNPs on two chromosomes, a blocks file with a
    gap that one matched SNP falls into (the scan stalls there: every later block is empty), a
    DBSLMM result and an external summary with swapped A1, a duplicate id, short lines, SNPs absent
    from the .bim and MAFs outside -mafMax 0.2.  (The layouts of test_cli.py are synthetic panels
    for `dbslmm`'s GEMMA inputs; `valid` reads other files, so this writes its own.)"""
    n_ref, m = 4100, 400
    rng = np.random.default_rng(77)
    f = rng.uniform(0.05, 0.5, m)                             # allele frequency of the dosage-2 allele
    u = rng.random((m, n_ref))
    codes = np.where(u < (f * f)[:, None], C_TWO, np.where(u < (f * (2 - f))[:, None], C_ONE, C_ZERO)).astype(np.uint8)
    codes[rng.random((m, n_ref)) < 0.01] = C_MISS
    codes[57] = C_TWO                                          # a monomorphic SNP: its block is nan
    ref = os.path.join(tmp, "ref")
    _bed(codes, 1).tofile(ref + ".bed")
    chrom = np.where(np.arange(m) < 230, 1, 2)
    ps = np.where(chrom == 1, 1000 + 100 * np.arange(m), 1050 + 100 * (np.arange(m) - 230))
    with open(ref + ".bim", "w") as o:
        for k in range(m):
            o.write(f"{chrom[k]}\trs{k}\t0\t{ps[k]}\tA\tG\n")
    with open(ref + ".fam", "w") as o:
        for i in range(n_ref):
            o.write(f"f{i} i{i} 0 0 0 -9\n")
    maf = np.array([R.read_snp_im(_bed(codes, 1), k, np.ones(n_ref, dtype=np.int32))[1] for k in range(m)])
    d_path, s_path, s_clean, b_path = (os.path.join(tmp, x) for x in ("d.txt", "ext.txt", "ext_clean.txt", "blocks.bed"))
    with open(d_path, "w") as o:
        for k in range(m):
            if k % 13 == 6:
                continue                                       # not in the DBSLMM result
            a1 = "G" if k % 17 == 4 else "A"                   # A1 other than the .bim's: dropped by matchAll
            o.write(f"rs{k} {a1} {rng.standard_normal() * 0.01:.6g} {rng.standard_normal():.6g} 0\n")
        o.write("rs_nowhere A 0.01 0.01 0\n")
    lines = []
    for k in range(m):
        if k % 19 == 7:
            continue                                           # not in the external summary
        a1 = "G" if k % 5 == 2 else "A"                        # swapped A1: z2 changes sign
        mf = maf[k] + (0.3 if k % 23 == 9 else 0.01)           # outside -mafMax 0.2
        lines.append(f"rs{k} {a1} {mf:.6g} {rng.standard_normal() * 3:.6g}")
        if k % 29 == 3:
            lines.append(f"rs{k} A 0.9 99")                    # a duplicate id: the first line wins
        if k % 31 == 5:
            lines.append(f"rs{k}_short A 0.25")                # fewer than 4 fields
    lines += ["rs_absent1 A 0.2 1.5", "rs_absent2 G 0.3 -0.5", "onlyone"]
    open(s_path, "w").write("\n".join(lines) + "\n")
    # the reference indexes past the end of a short line (undefined); the CLI skips the line, and
    # the restatement is given the file without them
    open(s_clean, "w").write("\n".join(x for x in lines if len(x.split(" ")) >= 4) + "\n")
    top = int(ps.max()) + 1
    edges = [(0, 4000), (4000, 9000), (9000, 13000), (13100, 17000), (17000, 21000), (21000, top)]
    with open(b_path, "w") as o:
        for k, (s, e) in enumerate(edges):
            o.write(f"chr{1 if k < 4 else 2}\t{s}\t{e}\n")
    return ref, d_path, s_path, s_clean, b_path, ps


def test_cli_inputs_reach_their_edges(tmp_path):
    """CPU: the restatement on the CLI case -- a SNP in the gap is matched, blocks after it are
    empty, the monomorphic SNP's block is nan, the MAF filter and the A1 rules all bite."""
    ref, d_path, s_path, s_clean, b_path, ps = _write_valid_inputs(str(tmp_path))
    with np.errstate(divide="ignore", invalid="ignore"):
        lines1, nume1, deno1 = R.valid(d_path, s_clean, ref, 1.0, b_path)
        lines2, nume2, deno2 = R.valid(d_path, s_clean, ref, 0.2, b_path)
    summc = R.match_summ(R.read_dbslmm(d_path), R.read_ext(s_clean))
    bim = R.read_bim_b(ref, 4100, False)
    summp = R.match_all(summc, bim, 1.0)
    assert any(13000 <= x[4] < 13100 for x in summp)                       # the SNP the scan stalls on
    assert sum(x[4] >= 13100 for x in summp) > 100
    assert "nan" in lines1[1] and lines1[3:] == ["0 0"] * 3 and lines2[3:] == ["0 0"] * 3
    assert all(np.isfinite(deno1[[0, 2]])) and all(deno1[[0, 2]] > 0) and not np.array_equal(deno1[[0, 2]], deno2[[0, 2]])
    assert any(a[4] != b[3] for a, b in zip(summc, (R.read_ext(s_clean)[x[0]] for x in summc)))   # flipped z2
    assert len(summp) < len([x for x in summc if x[0] in bim])              # A1 rule of matchAll


@pytest.mark.gpu
@pytest.mark.parametrize("maf_max", [0.2, 1.0])
def test_valid_cli_two_chromosomes_and_a_stalled_scan(tmp_path, maf_max):
    ref, d_path, s_path, s_clean, b_path, ps = _write_valid_inputs(str(tmp_path))
    out = str(tmp_path / "r2")
    r = subprocess.run([VALID, "-d", d_path, "-s", s_path, "-r", ref, "-mafMax", str(maf_max), "-b", b_path,
                        "-r2", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with np.errstate(divide="ignore", invalid="ignore"):
        lines, nume, deno = R.valid(d_path, s_clean, ref, maf_max, b_path)
    got = open(out + ".txt").read().strip("\n").split("\n")
    assert len(got) == len(lines) == 6
    for a, b in zip(got, lines):
        if a != b:   # 6 significant digits: allow one unit in the last place; nan matches nan
            x, y = np.array(a.split(), float), np.array(b.split(), float)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (a, b)
            ok = ~np.isnan(y)
            assert np.all(np.abs(x[ok] - y[ok]) <= 1e-5 * np.abs(y[ok]) + 1e-300), (a, b)
    assert got[3:] == ["0 0"] * 3

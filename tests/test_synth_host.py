"""The restatement of the GPU panel generator (tests/_synth_ref.py) is the model dbslmm_amd/synth.py
documents: two haplotypes per individual, an AR(1) latent Gaussian with rho along the SNPs of a block
restarted at each block, a threshold at Phi^-1(p), independent missing calls, PLINK codes.  No GPU:
tests/test_synth.py then holds the kernel to the restatement call by call.

The bands.  Every statistic below is held to 5 standard errors of its own sampling distribution under
the model (two-sided 5.7e-7); a maximum over n statistics is held to Z(n) = Phi^-1(1 - Phi(-5) / n)
standard errors each, the Bonferroni bound that keeps the whole family at the level of one 5-SE test
(Z(400) = 6.1).  Standard errors:

* a frequency or a count of N independent calls of probability p: binomial, sqrt(p (1 - p) / N);
* a correlation r of N independent pairs against a value r0: Fisher, atanh(r) - atanh(r0) has standard
  error 1 / sqrt(N - 3); against 0 with large N this is 1 / sqrt(N);
* pooled over SNPs the latent values are not independent (they are an AR(1)), so the pooled tests use
  the innovations e_s = (u_s - rho u_{s-1}) / a (e = u at the first SNP of a block), which the model
  makes independent N(0, 1) across SNPs, haplotypes and individuals: N is then the plain count;
* the pooled lag-k test: y = u_s - rho^k u_{s-k} is a sum of the k innovations after s - k, so it is
  independent of x = u_{s-k} and corr(x, y) = 0 exactly when the lag-k correlation is rho^k.  The
  products x y of two SNPs at least k apart are uncorrelated (the later y is independent of everything
  before it), and the at most 2 k - 1 others are bounded by Cauchy-Schwarz, so the pooled correlation
  has standard error at most sqrt((2 k - 1) / N).

The panel: 400 SNPs x 2000 individuals, blocks [0, 150, 150, 151, 400], rho 0.9, missing rate 0.01,
seed 1, allele frequencies U(0.05, 0.5) from a fixed generator.  Measured on it (printed by the tests):
latent mean 4e-4 and variance 0.9996, lag-1 correlation inside a block 0.90006, across the block
boundaries 0.003 and 0.02, worst |freq - af| / SE 2.8, missing rate 0.0101."""
import math

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import norm, t as student_t

import _synth_ref as SR

P5 = norm.sf(5.0)
RHO, MISS, N_REF, M = 0.9, 0.01, 2000, 400
BLOCKS = (0, 150, 150, 151, 400)
STARTS = (0, 150, 151)


def Z(n):
    """Bonferroni: standard errors for each of n statistics at the family level of one 5-SE test"""
    return float(norm.isf(P5 / n))


def corr(x, y):
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    x, y = x - x.mean(), y - y.mean()
    return float(x @ y / math.sqrt((x @ x) * (y @ y)))


class Big:
    pass


@pytest.fixture(scope="module")
def big():
    b = Big()
    b.af = np.random.default_rng(1).uniform(0.05, 0.5, size=M)
    b.p = SR.panel(BLOCKS, ndtri(b.af).astype(np.float32), N_REF, 1, RHO, MISS)
    assert b.p.real.all()                                          # 2000 = 4 * 500: no pad individual
    b.u = b.p.u.astype(np.float64)                                 # [M, 2000, 2]
    b.U = b.u.reshape(M, 2 * N_REF)                                # [M, 4000 haplotypes]
    rho, a = float(np.float32(RHO)), float(np.sqrt(np.float32(1) - np.float32(RHO) * np.float32(RHO)))
    b.e = b.u.copy()
    inner = np.array([s for s in range(M) if s not in STARTS])
    b.e[inner] = (b.u[inner] - rho * b.u[inner - 1]) / a
    b.inside = [(0, 150), (151, 400)]                              # blocks with more than one SNP
    for x in (b.u, b.U, b.e, b.p.u, b.p.hap, b.p.dosage, b.p.miss, b.p.rows):
        x.setflags(write=False)
    return b


# ------------------------------------------------------------------------------------------------
# the hash and the Box-Muller step
# ------------------------------------------------------------------------------------------------
def test_mix64_is_splitmix64():
    """the first SplitMix64 output from state 0, and the second (state = the increment)"""
    assert int(SR.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(SR.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert SR.mix64(np.arange(3)).dtype == np.uint64


def test_box_muller_edges():
    """top 24 bits all ones: k + 0.5 rounds up to 2^24, u1 == 1.0f, log 0, the pair is (0, 0) and
    finite; u1 at its minimum 2^-25: |e| = sqrt(50 log 2) = 5.887; no uniform is 0 or above 1"""
    top = np.uint64(0xFFFFFF) << np.uint64(40)
    u1, u2 = SR.uniforms(top)
    assert u1.dtype == np.float32 and float(u1) == 1.0 and float(u2) == 2.0 ** -25
    a, b = SR.normal2(top)
    assert float(a) == 0.0 and float(b) == 0.0
    u1, _ = SR.uniforms(np.uint64(0))
    assert float(u1) == 2.0 ** -25
    a, b = SR.normal2(np.uint64(0))
    assert abs(math.hypot(float(a), float(b)) - math.sqrt(50 * math.log(2))) < 1e-5
    assert abs(float(a) - 5.887) < 1e-3                            # the angle is pi 2^-24: all cosine
    h = SR.mix64(np.arange(1 << 16))
    h[:2] = (0, 0xFFFFFFFFFFFFFFFF)
    for u in SR.uniforms(h):
        assert u.min() > 0.0 and u.max() <= 1.0
    for e in SR.normal2(h):
        assert np.all(np.isfinite(e)) and np.abs(e).max() < 5.89


def test_rows_are_the_plink_packing():
    """the restatement's bytes are synth.pack_dosages of its dosages and mask, pads 00 (n_ref = 5)"""
    from dbslmm_amd.synth import pack_dosages
    p = SR.case_ref("n5")
    d = p.dosage[:, :5].copy()
    d[p.miss[:, :5]] = -1
    assert p.miss.any() and not p.miss[:, 5:].any()
    assert np.array_equal(p.rows, pack_dosages(d))
    assert np.array_equal(SR.DOSAGE_OF_CODE[SR.decode(p.rows, 5)][:, :5], d)
    assert not np.any(SR.decode(p.rows, 5)[:, 5:])


def test_compare_sees_what_it_must():
    """the rule of test_synth.py on doctored rows: the restatement's own rows pass with no mismatch; a
    flipped call outside the band, a dosage off by 2 with one haplotype in the band, a moved missing
    code and a non-zero pad are errors; a flipped call inside the band is counted and allowed"""
    p = SR.case_ref("n1025")
    assert SR.compare(p.rows, p) == ([], 0, 0.0)
    code = SR.decode(p.rows, p.n_ref)
    lo = np.sort(p.margin, axis=2)
    live = p.real[None, :] & ~p.miss

    def doctored(s, i, new):
        rows = p.rows.copy()
        sh = 2 * (int(i) % 4)
        rows[s, i // 4] = (int(rows[s, i // 4]) & (0xFF ^ (3 << sh))) | (int(new) << sh)
        return SR.compare(rows, p)

    step = {0: 2, 2: 0, 3: 2}                                       # a dosage one away: code -> code
    s, i = np.argwhere(live & (lo[:, :, 0] > SR.EPS))[0]
    assert len(doctored(s, i, step[code[s, i]])[0]) == 1
    s, i = np.argwhere(live & (lo[:, :, 0] <= SR.EPS))[0]
    errors, n_bad, worst = doctored(s, i, step[code[s, i]])
    assert errors == [] and n_bad == 1 and worst == lo[s, i, 0] <= SR.EPS
    s, i = np.argwhere(live & (lo[:, :, 0] <= SR.EPS) & (lo[:, :, 1] > SR.EPS) & (code != 2))[0]
    assert len(doctored(s, i, 3 - code[s, i])[0]) == 1              # 00 <-> 11: off by 2, one in band
    s, i = np.argwhere(live)[0]
    assert len(doctored(s, i, 1)[0]) == 1                           # a missing code the mask lacks
    s, i = np.argwhere(p.miss)[0]
    assert len(doctored(s, i, int(SR.CODE_OF_DOSAGE[p.dosage[s, i]]))[0]) == 1   # a missing code lost
    assert len(doctored(0, p.n_ref, 3)[0]) == 1                     # a pad individual with a call


# ------------------------------------------------------------------------------------------------
# the latent AR(1)
# ------------------------------------------------------------------------------------------------
def test_latent_moments(big):
    """innovations pooled: mean 0 +- 5 / sqrt(N), variance 1 +- 5 sqrt(2 / N); the latent of every
    SNP (4000 independent haplotypes) mean 0 and variance 1 at Z(2 M) standard errors: a wrong
    a = sqrt(1 - rho^2) would let the variance drift along a block"""
    n = big.e.size
    print(f"latent mean {big.u.mean():.1e} variance {big.u.var():.4f}; innovations mean {big.e.mean():.1e} "
          f"variance {big.e.var():.4f}")
    assert abs(big.e.mean()) <= 5 / math.sqrt(n)
    assert abs(big.e.var() - 1) <= 5 * math.sqrt(2 / n)
    h = big.U.shape[1]
    z = Z(2 * M)
    assert np.abs(big.U.mean(axis=1)).max() <= z / math.sqrt(h)
    assert np.abs(big.U.var(axis=1) - 1).max() <= z * math.sqrt(2 / h)
    # the tails are Gaussian: P(|u| > 3) = 2.70e-3, binomial over the first SNPs of the blocks and
    # every innovation (independent draws)
    p3 = 2 * norm.sf(3.0)
    assert abs(np.mean(np.abs(big.e) > 3) - p3) <= 5 * math.sqrt(p3 * (1 - p3) / n)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_lag_k_correlation_is_rho_k(big, k):
    """every pair of SNPs k apart inside a block: Fisher z over the 4000 haplotypes against rho^k,
    Z(pairs) / sqrt(N - 3); and pooled, corr(u_s - rho^k u_{s-k}, u_{s-k}) = 0 +- 5 sqrt((2k - 1) / N)"""
    Zs = (big.U - big.U.mean(axis=1, keepdims=True)) / big.U.std(axis=1, keepdims=True)
    lo = np.concatenate([np.arange(s0, s1 - k) for s0, s1 in big.inside])
    r = np.mean(Zs[lo] * Zs[lo + k], axis=1)
    h = big.U.shape[1]
    x, y = big.U[lo], big.U[lo + k] - RHO ** k * big.U[lo]
    c = corr(x, y)
    print(f"lag {k}: mean r {r.mean():.5f} (rho^k {RHO ** k:.5f}), worst Fisher z "
          f"{np.abs(np.arctanh(r) - math.atanh(RHO ** k)).max() * math.sqrt(h - 3):.2f} SE of {len(lo)} pairs; "
          f"pooled residual correlation {c:.2e}")
    assert np.abs(np.arctanh(r) - math.atanh(RHO ** k)).max() <= Z(len(lo)) / math.sqrt(h - 3)
    assert abs(c) <= 5 * math.sqrt((2 * k - 1) / x.size)


def test_blocks_restart(big):
    """across a block boundary the latent correlation is 0: SNPs 149 | 150 | 151 (the one-SNP block
    between two long ones), Fisher z at Z(3) / sqrt(N - 3); and the innovations have no serial
    correlation anywhere (the restart is a draw like any other)"""
    h = big.U.shape[1]
    r = [corr(big.U[a], big.U[b]) for a, b in ((149, 150), (150, 151), (149, 151))]
    print("across the boundaries:", " ".join(f"{x:.3f}" for x in r))
    assert np.abs(np.arctanh(r)).max() <= Z(3) / math.sqrt(h - 3)
    c = corr(big.e[:-1], big.e[1:])
    assert abs(c) <= 5 / math.sqrt(big.e[1:].size)


# ------------------------------------------------------------------------------------------------
# thresholds: frequencies, Hardy-Weinberg, independence of haplotypes and individuals
# ------------------------------------------------------------------------------------------------
def test_haplotype_frequency_is_af(big):
    """per SNP the 4000 haplotype calls are Bernoulli(af): Z(M) binomial standard errors"""
    h = big.U.shape[1]
    f = big.p.hap.reshape(M, h).mean(axis=1)
    se = np.sqrt(big.af * (1 - big.af) / h)
    print(f"worst |freq - af| / SE {(np.abs(f - big.af) / se).max():.2f}")
    assert np.all(np.abs(f - big.af) <= Z(M) * se)


def test_hardy_weinberg_counts(big):
    """per SNP the dosage counts of the 2000 individuals are multinomial ((1 - p)^2, 2 p (1 - p), p^2):
    each count within Z(3 M) binomial standard errors of its expectation"""
    p = big.af
    for d, q in ((0, (1 - p) ** 2), (1, 2 * p * (1 - p)), (2, p ** 2)):
        n = np.count_nonzero(big.p.dosage == d, axis=1)
        assert np.all(np.abs(n - N_REF * q) <= Z(3 * M) * np.sqrt(N_REF * q * (1 - q))), d


def test_haplotypes_and_individuals_are_uncorrelated(big):
    """innovations pooled over SNPs: the two haplotypes of an individual (N = M n_ref); individuals
    j < j' of one byte, each of the four haplotype pairings (24 statistics, N = M nb each); the same
    slot one byte and 256 bytes on (a second workgroup column that repeated the first would give 1).
    Per SNP, the latent values of an individual's two haplotypes: Fisher z, Z(M) / sqrt(n_ref - 3)."""
    e = big.e
    c = corr(e[:, :, 0], e[:, :, 1])
    print(f"haplotype 1 against 2: {c:.2e}")
    assert abs(c) <= 5 / math.sqrt(e[:, :, 0].size)
    r = np.array([corr(big.u[s, :, 0], big.u[s, :, 1]) for s in range(M)])
    assert np.abs(np.arctanh(r)).max() <= Z(M) / math.sqrt(N_REF - 3)
    e4 = e.reshape(M, N_REF // 4, 4, 2)
    worst = 0.0
    for j in range(4):
        for jj in range(j):
            for a in range(2):
                for b in range(2):
                    worst = max(worst, abs(corr(e4[:, :, j, a], e4[:, :, jj, b])))
    print(f"individuals of one byte: worst |r| {worst:.2e}")
    assert worst <= Z(24) / math.sqrt(M * (N_REF // 4))
    for lag in (1, 256):
        c = corr(e4[:, lag:], e4[:, :-lag])
        assert abs(c) <= Z(2) / math.sqrt(e4[:, lag:].size), lag


# ------------------------------------------------------------------------------------------------
# missing calls
# ------------------------------------------------------------------------------------------------
def test_missing_calls_are_independent(big):
    """the mask is Bernoulli(q), q = the share of 16-bit values k with (k + 0.5) / 2^16 < miss_rate:
    the pooled rate at 5 binomial SE and every SNP's at Z(M); uncorrelated with the dosage and with
    either latent value (the mask is independent of both whatever their distribution, so r has
    standard error 1 / sqrt(N)), between the individuals of a byte (6 pairs) and along the SNPs"""
    m = big.p.miss
    q = math.ceil(float(np.float32(MISS)) * 65536 - 0.5) / 65536
    assert abs(q - MISS) < 2.0 ** -16
    print(f"missing rate {m.mean():.5f} (q {q:.5f})")
    assert abs(m.mean() - q) <= 5 * math.sqrt(q * (1 - q) / m.size)
    assert np.abs(m.mean(axis=1) - q).max() <= Z(M) * math.sqrt(q * (1 - q) / N_REF)
    z = Z(3 + 6 + 1) / math.sqrt(m.size)
    assert abs(corr(m, big.p.dosage)) <= z
    assert abs(corr(m, big.u[:, :, 0])) <= z and abs(corr(m, big.u[:, :, 1])) <= z
    m4 = m.reshape(M, N_REF // 4, 4)
    for j in range(4):
        for jj in range(j):
            assert abs(corr(m4[:, :, j], m4[:, :, jj])) <= Z(10) / math.sqrt(m4[:, :, 0].size), (j, jj)
    assert abs(corr(m[1:], m[:-1])) <= Z(10) / math.sqrt(m[1:].size)


def test_missing_rate_edges():
    """miss_rate 0 forms no mask, 1.0 masks every call (the largest uniform is below 1), 0.5 half"""
    assert not SR.case_ref("miss0.0").miss.any()
    p = SR.case_ref("miss1.0")
    assert p.miss[:, p.real].all() and not p.miss[:, ~p.real].any()
    assert np.all(SR.decode(p.rows, p.n_ref)[:, p.real] == 1)
    p = SR.case_ref("miss0.5")
    m = p.miss[:, p.real]
    assert abs(m.mean() - 0.5) <= 5 * math.sqrt(0.25 / m.size)
    # the mask does not move the genotypes: the three panels share their latent values
    assert np.array_equal(p.u, SR.case_ref("miss0.0").u)


# ------------------------------------------------------------------------------------------------
# the NumPy engine draws the same LD
# ------------------------------------------------------------------------------------------------
def _adjacent_r2(dos):
    """dosage r^2 of adjacent SNPs, [m - 1]"""
    x = dos.astype(np.float64)
    x = x - x.mean(axis=1, keepdims=True)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.sum(x[1:] * x[:-1], axis=1) ** 2


def test_adjacent_ld_matches_the_numpy_engine():
    """One block of 400 SNPs x 2000 individuals from synth.simulate(engine="numpy") and the
    restatement at the same af and rho: the mean dosage r^2 over the 399 adjacent pairs agree.
    Sampling error of the difference: the individuals are independent, so the 2000 are cut into 10
    groups of 200 and D_g = mean r^2 (restatement) - mean r^2 (NumPy engine) is computed in each (the
    O(1 / n) bias of a sample r^2 is the same on both sides).  Under a common model the D_g are 10
    independent draws of mean 0, so their mean is held to the Student-t (9 degrees of freedom)
    quantile of a 5-SE test times their standard error.  A restatement at rho 0.8 is outside that
    band by far (the band can see a wrong rho)."""
    from dbslmm_amd import synth
    ref = synth.simulate(M, N_REF, block_limit=1, seed=11, rho=RHO, engine="numpy", large_every=0)
    assert ref.m == M and np.all(ref.block == 0)
    d_np = SR.DOSAGE_OF_CODE[SR.decode(ref.bed[3:].reshape(M, -1), N_REF)]
    thr = ndtri(ref.af).astype(np.float32)
    groups = np.arange(N_REF).reshape(10, -1)
    tq = float(student_t.isf(P5, len(groups) - 1))

    def t_stat(rho):
        d = SR.panel((0, M), thr, N_REF, 1, rho, 0.0).dosage
        D = np.array([_adjacent_r2(d[:, g]).mean() - _adjacent_r2(d_np[:, g]).mean() for g in groups])
        se = D.std(ddof=1) / math.sqrt(len(D))
        print(f"rho {rho}: mean r^2 {_adjacent_r2(d).mean():.4f} against {_adjacent_r2(d_np).mean():.4f}; "
              f"D {D.mean():.2e}, SE {se:.2e}, band {tq:.1f} SE")
        return abs(D.mean()) / se

    assert t_stat(RHO) <= tq
    assert t_stat(0.8) > 2 * tq


# ------------------------------------------------------------------------------------------------
# the GPU cases' precondition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.CASES) + ["simulate"])
def test_gpu_cases_keep_the_band_thin(name):
    """at most 1e-3 of a case's haplotypes lie within EPS of their threshold (P(|u - t| <= eps) is
    2 eps phi(t) <= 7.8e-4), so the band rule of tests/test_synth.py excuses next to nothing; the
    thresholds of the cases come from a fixed generator, and the small cases (600 haplotypes at
    n_ref = 1) have none in the band"""
    p = SR.sim_case()[3] if name == "simulate" else SR.case_ref(name)
    share = SR.band_share(p)
    print(f"{name}: {share:.2e} of {p.margin[:, p.real].size} haplotypes in the band")
    assert share <= SR.BAND_MAX


def test_seeds_and_splits_of_the_restatement():
    """what tests/test_synth.py asserts of the GPU holds for the restatement: four seeds, four panels;
    a boundary at 100 leaves rows 0..99 alone and changes what follows; the tail alone is the tail"""
    rows = [SR.case_ref(n).rows for n in SR.SEED_CASES]
    for i in range(4):
        for j in range(i):
            assert not np.any(np.all(rows[i] == rows[j], axis=1))
    whole, split, tail = (SR.case_ref(n) for n in ("whole", "split", "tail"))
    assert np.array_equal(whole.rows[:100], split.rows[:100])
    assert np.any(whole.rows[100] != split.rows[100])
    assert tail.first == 100 and np.array_equal(tail.rows, split.rows[100:])

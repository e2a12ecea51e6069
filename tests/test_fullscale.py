"""Full-size parity of the HIP path on BASELINE.json configs[2..4].

The HIP solve of the whole synthetic panel (GPU generator, the bench's own workloads) is compared
block by block with the oracle's direct fp64 solve of the reference equations
(scr/dbslmmfit.cpp:680-770; oracle/ref_numpy.py est_block_*_sigma, Cholesky on all host cores):

* every block with m >= 2000 SNPs -- this includes the largest EUR block (~9.6k SNPs at 1M) and
  the largest AFR block (~11.7k): normwise max|dbeta| / max|beta| <= 1e-10 per block and h2f
  copy.  By default these configs take the PCG route (dbslmm_options.solver = 0: the prior shift
  d = 1/(sigma_s n) >= 2 keeps every block well conditioned), whose stopping rule bounds each
  copy's relative error by pcg_tol = 1e-12; "4-factor" forces the factorisation route (the tiled
  sequence's long-chain regime, >= 37 super steps, ~150-tile substitution chains, and the h2f
  copies iterated on the base factor: those copies <= cheb_tol, CHEB_TOL);
* the same blocks against the reference-faithful Jacobi-PCG (abs. tol 1e-7, :629-678): <= 1e-5;
* a random sample of the smaller blocks through the C oracle (direct): <= 1e-10;
* every block: status OK and beta finite.

These tests take ~0.5-1 min each on the GPU box (most of it the CPU reference)."""
import numpy as np
import pytest

import oracle as O
import ref_numpy as R
from _common import CHEB_TOL, normwise

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# config -> (SNPs, n_ref, pop, LMM-only, h2f factors); BASELINE.json configs[i - 1]
CONFIGS = {
    3: (500_000, 5_000, "EUR", False, (1.0,)),
    4: (1_000_000, 10_000, "EUR", False, (0.8, 1.0, 1.2)),
    5: (1_000_000, 10_000, "AFR", True, (1.0,)),
}
BIG = 2000           # blocks at least this large are all checked
SAMPLE = 64          # plus this many random smaller blocks


def _threads():
    import os
    return int(os.environ.get("OMP_NUM_THREADS") or min(16, os.cpu_count() or 1))


def _gpu_solve(prob, factors, devices=0):
    from dbslmm_amd import Context, Plan
    if isinstance(devices, list):    # the shard plan may split the largest blocks' h2f copies
        prob.opts["shard_copies"] = len(factors)
    plan = Plan(Context(devices), prob)
    sig = [prob.sigma_s * f for f in factors]
    if len(sig) > 1:
        out = plan.run_multi(sig)
    else:
        plan.run()
        out = [plan.download()]
    wl = plan.workload()
    plan.close()
    return sig, out, wl


def _block_ref(prob, b, sig, thr, pcg=True):
    """Direct (Cholesky) and PCG betas of block b for every sigma, sharing one Gram."""
    s0, s1 = int(prob.s_ptr[b]), int(prob.s_ptr[b + 1])
    Xs = O.read_block_std(prob.bed, prob.n_ref, prob.s_pos[s0:s1], threads=thr)
    Xl = None
    if prob.l_ptr is not None and prob.l_ptr[b + 1] > prob.l_ptr[b]:
        l0, l1 = int(prob.l_ptr[b]), int(prob.l_ptr[b + 1])
        Xl = O.read_block_std(prob.bed, prob.n_ref, prob.l_pos[l0:l1], threads=thr)
    Sss, Sls, Sll = R.block_sigmas_tau(Xs, Xl, prob.n_ref, prob.tau)
    del Xs, Xl
    out = {}
    for method in ("chol", "pcg") if pcg else ("chol",):
        res = []
        for sg in sig:
            if Sls is None:
                res.append(R.est_block_s_sigma(Sss, prob.n_obs, sg, prob.z_s[s0:s1], method))
            else:
                bs, bl = R.est_block_ls_sigma(Sss, Sls, Sll, prob.n_obs, sg, prob.z_s[s0:s1],
                                              prob.z_l[l0:l1], method)
                res.append(np.concatenate([bs, bl]))
        out[method] = res
    return out


def _diagnose(prob, b, sg, thr, devices=0, factor=None):
    """Per-phase differences of block b (a full-size mismatch must name its phase):
    Sigma after the Gram (a debug_stop = 1 run, dbslmm_plan_block_matrix) against the oracle's
    standardised Gram, then -- from a fresh full run -- the factor L (strict lower triangle and the
    stored 1 / L_ii), y = L^-1 z (row m) and beta, each against NumPy's Cholesky of the reference
    matrix (scr/dbslmmfit.cpp:697-729 restated as one joint solve).  Returns a dict
    of normwise differences (phases of a block below the tiled threshold: Sigma and beta only,
    unless factor names what the block's kernel leaves in its matrix: "full" = L, 1 / L_ii and the
    y row, as the tiled layout -- dbslmm_chol_large keeps the same; "no_y" = L and 1 / L_ii only --
    dbslmm_chol_small keeps y in LDS).
    Runs the factorisation route (solver = 1): its beta is that route's, beside the failing one."""
    from scipy.linalg import solve_triangular
    from dbslmm_amd import Context, Plan
    s0, s1 = int(prob.s_ptr[b]), int(prob.s_ptr[b + 1])
    Xs = O.read_block_std(prob.bed, prob.n_ref, prob.s_pos[s0:s1], threads=thr)
    Xl, zl = None, np.zeros(0)
    if prob.l_ptr is not None and prob.l_ptr[b + 1] > prob.l_ptr[b]:
        l0, l1 = int(prob.l_ptr[b]), int(prob.l_ptr[b + 1])
        Xl = O.read_block_std(prob.bed, prob.n_ref, prob.l_pos[l0:l1], threads=thr)
        zl = prob.z_l[l0:l1]
    Sss, Sls, Sll = R.block_sigmas_tau(Xs, Xl, prob.n_ref, prob.tau)
    del Xs, Xl
    ms = s1 - s0
    m = ms + zl.size
    S = np.zeros((m, m))
    S[:ms, :ms] = Sss
    if zl.size:
        S[ms:, :ms] = Sls
        S[:ms, ms:] = Sls.T
        S[ms:, ms:] = Sll
    z = np.concatenate([prob.z_s[s0:s1], zl])
    opts0 = dict(prob.opts)
    sigma0 = prob.sigma_s
    out = {}
    try:
        prob.opts = dict(opts0, debug_stop=1, solver=1)
        plan = Plan(Context(devices), prob)
        plan.run()
        A = plan.block_matrix(b)
        plan.close()
        lo = np.tril_indices(m)
        out["sigma"] = float(np.max(np.abs(A[:m, :m][lo] - S[lo])) / np.max(np.abs(S)))
        prob.opts = dict(opts0, solver=1)
        prob.sigma_s = sg
        plan = Plan(Context(devices), prob)
        plan.run()
        A = plan.block_matrix(b)
        got = _got(prob, plan.download(), b)
        plan.close()
    finally:
        prob.opts = opts0
        prob.sigma_s = sigma0
    M = S
    M[np.arange(ms), np.arange(ms)] += 1.0 / (sg * prob.n_obs)
    L = np.linalg.cholesky(M)
    del M, S
    y = solve_triangular(L, z, lower=True)
    x = solve_triangular(L.T, y, lower=False) / np.sqrt(prob.n_obs)
    if factor is None:
        factor = "full" if m >= 384 else ""     # the tiled layout (default tiled_min at full scale)
    if factor:
        st = np.tril_indices(m, -1)
        out["L"] = float(np.max(np.abs(A[:m, :m][st] - L[st])) / np.max(np.abs(L)))
        out["L_diag"] = normwise(1.0 / np.diag(A)[:m], np.diag(L))
        if factor == "full":
            out["y"] = normwise(A[m, :m], y)
    out["beta"] = normwise(got, x)
    return out


def _got(prob, res, b):
    bs, bl, _ = res
    s = bs[prob.s_ptr[b]:prob.s_ptr[b + 1]]
    if prob.l_ptr is None:
        return s
    return np.concatenate([s, bl[prob.l_ptr[b]:prob.l_ptr[b + 1]]])


@pytest.mark.parametrize("cfg,devices,solver", [(3, 0, 0), (4, 0, 0), (5, 0, 0), (4, 0, 1), (3, [0, 0], 0),
                                                (4, [0, 0, 0, 0], 0), (4, [0, 0, 0, 0], 1)],
                         ids=["3", "4", "5", "4-factor", "3-multi", "4-multi", "4-multi-factor"])
def test_fullscale_blocks_match_oracle(cfg, devices, solver):
    """devices = [0, 0] / [0] * 4: the product's multi-device context (dbslmm_ctx_create_multi: the
    shard plan's units, compact per-device .bed images, one host thread per job) on the test GPU.
    Its betas must equal the one-device solve bit for bit -- on the PCG route every block is whole
    on one device and iterates independently of the others; on the factorisation route
    (solver = 1) except the non-base h2f copies of the block whose copies the shard plan splits
    over devices at config 4: those are factored directly there (the one-device run iterates them),
    so they agree to cheb_tol.  The oracle comparison below holds every copy to its bar either way."""
    from dbslmm_amd import synth
    from dbslmm_amd.dist import shard_units_problem
    snps, n_ref, pop, lmm, factors = CONFIGS[cfg]
    panel = synth.simulate(snps, n_ref, pop=pop, seed=1, engine="gpu")
    prob = synth.make_problem(panel, lmm_only=lmm)
    del panel
    if solver:
        prob.opts["solver"] = solver
    sig, out, wl = _gpu_solve(prob, factors, devices)
    pcg = bool(wl["pcg_route"])
    assert pcg == (solver == 0), wl["pcg_route"]
    m_b = np.diff(prob.s_ptr) + (np.diff(prob.l_ptr) if prob.l_ptr is not None else 0)
    if isinstance(devices, list):
        prob.opts.pop("shard_copies", None)
        _, one, _ = _gpu_solve(prob, factors, 0)
        ud, _ = shard_units_problem(prob, [prob.sigma_s] * len(factors), len(devices))
        split = np.flatnonzero(~np.all(ud == ud[:, :1], axis=1))
        if pcg:
            assert split.size == 0                                              # whole blocks
        elif cfg == 4:
            assert split.size >= 1 and m_b[split].max() == m_b.max(), split   # the 9.7k block
        ms = np.zeros(prob.n_s, dtype=bool)
        ml = np.zeros(prob.n_l, dtype=bool)
        for b in split:
            ms[prob.s_ptr[b]:prob.s_ptr[b + 1]] = True
            if prob.l_ptr is not None:
                ml[prob.l_ptr[b]:prob.l_ptr[b + 1]] = True
        base0 = int(np.argsort(sig, kind="stable")[len(sig) // 2])
        for c, ((bs, bl, st), (bs1, bl1, st1)) in enumerate(zip(out, one)):
            assert np.array_equal(st, st1)
            assert np.array_equal(bs[~ms], bs1[~ms]) and np.array_equal(bl[~ml], bl1[~ml]), c
            if split.size:
                g, o = np.concatenate([bs[ms], bl[ml]]), np.concatenate([bs1[ms], bl1[ml]])
                if c == base0:
                    assert np.array_equal(g, o), c
                else:
                    assert normwise(g, o) <= CHEB_TOL, (c, normwise(g, o))
    for bs, bl, st in out:
        assert np.all((st == 0) | ((st == 1) & (m_b == 0))), np.flatnonzero((st != 0) & (m_b > 0))
        assert np.all(np.isfinite(bs)) and np.all(np.isfinite(bl))
    if len(factors) > 1 and not pcg:
        assert wl["cheb_iters"] > 0          # the h2f iterations on the base factor are under test
    # factorisation route: the base copy (median sigma) is solved directly, the others iterated on
    # its factor to cheb_tol; PCG route: every copy to pcg_tol
    base = int(np.argsort(sig, kind="stable")[len(sig) // 2])
    tol_c = [1e-10 if (pcg or len(sig) == 1 or c == base) else CHEB_TOL for c in range(len(sig))]
    thr = _threads()
    O.use_blas(True)
    O.blas_threads(thr)
    try:
        big = np.flatnonzero(m_b >= BIG)
        assert m_b.max() >= {3: 4000, 4: 9000, 5: 11000}[cfg]
        worst_d, worst_p = 0.0, 0.0
        for b in big:
            ref = _block_ref(prob, int(b), sig, thr)
            for c in range(len(sig)):
                got = _got(prob, out[c], int(b))
                d = normwise(got, ref["chol"][c])
                p = normwise(got, ref["pcg"][c])
                worst_d, worst_p = max(worst_d, d), max(worst_p, p)
                if d > tol_c[c]:   # name the phase before failing
                    diag = _diagnose(prob, int(b), sig[c], thr, devices)
                    pytest.fail(f"config {cfg} block {int(b)} (m = {int(m_b[b])}) copy {c}: normwise "
                                f"{d:.3e} vs direct; per phase (fresh plans): {diag}")
                assert p <= 1e-5, (cfg, int(b), int(m_b[b]), c, p)
        print(f"config {cfg}: {len(big)} blocks >= {BIG} SNPs (max {int(m_b.max())}), "
              f"worst normwise vs direct {worst_d:.2e}, vs PCG {worst_p:.2e}")
    finally:
        O.blas_threads(1)
    # random sample of the other blocks through the C oracle (block-parallel, direct)
    rng = np.random.default_rng(cfg)
    rest = np.flatnonzero((m_b > 0) & (m_b < BIG))
    pick = np.sort(rng.choice(rest, size=min(SAMPLE, rest.size), replace=False))
    from dbslmm_amd.dist import sub_problem
    sub, s_idx, l_idx = sub_problem(prob, pick)
    for c, sg in enumerate(sig):
        rs, rl, rst, rc = O.est(sub.bed, sub.n_ref, sub.n_obs, sg, sub.s_ptr, sub.s_pos, sub.z_s,
                                sub.l_ptr, sub.l_pos, sub.z_l, tau=prob.tau, method="direct",
                                threads=thr)
        assert rc == 0
        got = np.concatenate([out[c][0][s_idx], out[c][1][l_idx]])
        ref = np.concatenate([rs, rl])
        assert normwise(got, ref) <= tol_c[c], (cfg, c)

"""dbslmm_assoc (assoc.hip: dbslmm_assoc_counts, dbslmm_assoc_tiles, dbslmm_assoc_finish) on the GPU
against tests/_assoc_ref.py.

Exact: n_mis, n_obs, af and status equal the restatement bit for bit; two identical calls, a row
alone / in a permuted list / in the full call, and a column in the first or the second pass of 16
columns give the same bits.

Raw products (bounded, derived): |D - D_ref| <= n_total 2^-52 sum_i |g_ij V_ik| and |Mm - Mm_ref| <=
n_total 2^-52 sum_{i missing} |V_ik| per entry, the order-independent bound of a dot product of at most
n_total terms.  D_ref is summed in longdouble over the library's own fp64 V, which the test reads
through the public interface: the scan of an identity panel (row i: dosage 1 for individual i, else
0) returns D = V exactly.  That V is also held to the restatement's to 1e-10 of its largest entry.

beta, se, T (measured, against the reference alone): beta normwise, max |d beta| / max |beta|; se and T
elementwise relative over all OK rows.  The yardstick of a case is the larger of the fp64
restatement's deviation from its longdouble run and the deviation between its two orders of summation
(sequential; 4-wide groups in 64-individual chunks); the allowance is 32 x the yardstick and never
below 2^-48.  Every case asserts from the reference, before the GPU runs, that every non-degenerate
row has xPx / ssx >= 1e-3 and n_obs >= c + 2, so no row sits near the COLLINEAR threshold and the
comparison leaves out no OK row.  Each case prints its yardsticks and deviations (DESIGN.md records
them).

p_wald: the finish kernel runs the host's student_t_two_sided source with the device's lgamma, log,
log1p and exp, which are not the host library's bit for bit; it is held to the host function of the
returned T and df, and to scipy at that T, to 1e-10 relative, the bar of the host test."""
import functools

import numpy as np
import pytest
import scipy.stats

import _assoc_ref as AR

gpu = pytest.mark.gpu
LD = np.longdouble
FLOOR = 2.0 ** -48


@functools.lru_cache(maxsize=None)
def _ctx():
    from dbslmm_amd import Context
    return Context(0)


# (n_total, n_rows, c - 1, P, chunk_indiv, missing rate, rows list)
CASES = {
    "n7_r1_c1": (7, 1, 0, 1, 0, 0.05, None),
    "n64_r15_c4_nomiss": (64, 15, 2, 2, 64, 0.0, None),
    "n65_r17_c17_ch64": (65, 17, 3, 14, 64, 0.05, None),
    "n257_r16_c16_ch64": (257, 16, 15, 1, 64, 0.05, None),
    "n257_r33_c1_rows": (257, 33, 0, 1, 0, 0.05, "shuffled"),
    "n1031_r33_c16": (1031, 33, 15, 1, 0, 0.05, None),
    "n1031_r33_c17_ch64": (1031, 33, 3, 14, 64, 0.05, None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case and its references (computed once, read only)."""
    n_total, n_rows, c1, P, chunk, miss, rows_kind = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    n_bed = n_rows + 3 if rows_kind else n_rows               # a list may skip rows of the panel
    freq = rng.uniform(0.15, 0.5, size=(n_bed, 1))
    g = rng.binomial(2, freq, size=(n_bed, n_total)).astype(np.int8)
    m = rng.random((n_bed, n_total)) < miss
    keep = np.ones(n_total, dtype=np.uint8)
    holes = [i for i in (3, 4, 15, 16, 63, 64, 65, 127, 128, 255, 256) if i < n_total and n_total > 7]
    keep[holes] = 0                                           # straddle byte, dword and 64-individual edges
    y = rng.standard_normal((n_total, P)) + 0.4 * g[0][:, None] * rng.standard_normal(P)
    w = rng.standard_normal((n_total, c1)) if c1 else None
    if n_total > 7:
        y[min(20, n_total - 1), P - 1] = np.nan               # a NaN phenotype drops the individual
    planted = {}
    if n_rows >= 15 and miss > 0:
        in_s = (keep != 0) & np.all(np.isfinite(y), axis=1)
        planted = dict(no_call=5, miss_outside=6, mono=7)
        m[5] = in_s                                           # every kept call missing, the others called
        m[6] = ~in_s                                          # missing calls outside S only
        g[7], m[7] = 2, rng.random(n_total) < 0.2             # monomorphic among its calls
        if c1:
            planted["collinear"] = 8
            m[8] = False
            w[:, c1 - 1] = g[8]                               # row 8 is a covariate
    bed = AR.encode(g, m)
    if rows_kind == "shuffled":
        rows = rng.permutation(n_bed)[:n_rows].astype(np.int32)
        rows[3], rows[10] = rows[20], rows[20]                # out of order, with repeats
        for r in planted.values():
            if r not in rows:
                rows[np.flatnonzero(~np.isin(rows, list(planted.values())))[0]] = r
    else:
        rows = None
    lst = np.arange(n_rows) if rows is None else rows
    ref = AR.scan(bed, n_total, y, w, keep, lst)
    ref_g = AR.scan(bed, n_total, y, w, keep, lst, grouped=True)
    ref_l = AR.scan(bed, n_total, y, w, keep, lst, dtype=LD)
    ok = ref["status"] == AR.OK
    # the preconditions of the measured comparison, from the reference alone
    c = c1 + 1
    assert np.array_equal(ref_l["status"], ref["status"]) and np.array_equal(ref_g["status"], ref["status"])
    assert ok.sum() >= 1 and np.all(ref["n_obs"][ok] >= c + 2)
    assert np.all(ref["xPx"][ok] / ref["ssx"][ok] >= 1e-3)
    for k, r in planted.items():
        want = dict(no_call=AR.NO_CALL, miss_outside=AR.OK, mono=AR.MONOMORPHIC, collinear=AR.COLLINEAR)[k]
        assert np.all(ref["status"][lst == r] == want), (k, ref["status"][lst == r])
    if "miss_outside" in planted:
        assert np.all(ref["n_mis"][lst == 6] == 0)
    if planted:
        assert ref["n_mis"].max() > 0 and {0, 1, 2, 3} <= set(np.unique((bed[3:, None] >> [0, 2, 4, 6]) & 3))
    yard = {}
    for k in ("beta", "se", "tstat"):
        a, b, l = (np.asarray(r[k][:, ok], dtype=LD) for r in (ref, ref_g, ref_l))
        if k == "beta":
            sc = np.max(np.abs(l), axis=1, keepdims=True)
            yard[k] = max(float(np.max(np.abs(a - l) / sc)), float(np.max(np.abs(a - b) / sc)))
        else:
            yard[k] = max(float(np.max(np.abs(a / l - 1))), float(np.max(np.abs(a / b - 1))))
    return dict(n_total=n_total, n_rows=n_rows, c1=c1, P=P, chunk=chunk, bed=bed, y=y, w=w, keep=keep, rows=rows,
                lst=lst, ref=ref, ok=ok, yard=yard, g=g, m=m, planted=planted)


@functools.lru_cache(maxsize=None)
def run(name):
    from dbslmm_amd import assoc
    c = case(name)
    return assoc(_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"], c["rows"], c["chunk"], products=True)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in a)


def take(out, idx):
    """The listed rows of every output of `assoc`."""
    return {k: v[:, idx] if k in ("beta", "se", "tstat", "p") else v[idx] for k, v in out.items()}


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_integers_af_and_status_are_exact(name):
    c, got = case(name), run(name)
    ref = c["ref"]
    for k in ("n_mis", "n_obs", "status"):
        assert np.array_equal(got[k], ref[k]), k
    fin = np.isfinite(ref["af"])                               # (NaN without an observed call, on both sides)
    assert np.array_equal(np.isnan(got["af"]), ~fin) and np.array_equal(got["af"][fin].view(np.uint64), ref["af"][fin].view(np.uint64))
    bad = ~c["ok"]
    for k in ("beta", "se", "tstat", "p"):
        assert np.all(np.isnan(got[k][:, bad])) and np.all(np.isfinite(got[k][:, c["ok"]])), k


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_raw_products_within_the_dot_product_bound(name):
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    n_total = c["n_total"]
    eye = AR.encode(np.eye(n_total, dtype=np.int8))
    V = assoc(_ctx(), eye, n_total, c["y"], c["w"], c["keep"], None, c["chunk"], products=True)
    assert not V["prod_m"].any()
    V = V["prod_d"]                                            # the library's V: 1 * V_ik + zeros, exact
    Vr = c["ref"]["design"]["V"]
    assert V.shape == Vr.shape and np.max(np.abs(V - Vr)) <= 1e-10 * np.max(np.abs(Vr))
    assert not V[~c["ref"]["design"]["in_s"]].any()
    gl, ml = AR.decode(c["bed"], n_total, c["lst"])
    D, Mm, aD, aM = AR.products(gl, ml, V, LD)
    bound = LD(n_total) * LD(2.0) ** -52
    eD = np.abs(got["prod_d"].astype(LD) - D)
    eM = np.abs(got["prod_m"].astype(LD) - Mm)
    print(f"assoc products {name}: max |dD| / bound {float(np.max(eD / np.maximum(bound * aD, LD(1e-300)))):.3f}, "
          f"max |dMm| / bound {float(np.max(eM / np.maximum(bound * aM, LD(1e-300)))):.3f}")
    assert np.all(eD <= bound * aD) and np.all(eM <= bound * aM)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_beta_se_t_within_32_yardsticks(name):
    c, got = case(name), run(name)
    ref, ok = c["ref"], c["ok"]
    dev = {}
    for k in ("beta", "se", "tstat"):
        a, r = got[k][:, ok], ref[k][:, ok]
        if k == "beta":
            dev[k] = float(np.max(np.max(np.abs(a - r), axis=1) / np.max(np.abs(r), axis=1)))
        else:
            dev[k] = float(np.max(np.abs(a / r - 1)))
    print(f"assoc {name}: yardstick beta {c['yard']['beta']:.2e} se {c['yard']['se']:.2e} T {c['yard']['tstat']:.2e}; "
          f"GPU beta {dev['beta']:.2e} se {dev['se']:.2e} T {dev['tstat']:.2e}; OK rows {int(ok.sum())}")
    for k in dev:
        assert dev[k] <= max(32 * c["yard"][k], FLOOR), (k, dev[k], c["yard"][k])


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_p_wald_is_the_t_tail_of_the_returned_t(name):
    from dbslmm_amd import student_t_two_sided
    c, got = case(name), run(name)
    df = c["ref"]["df"]
    T, p = got["tstat"][:, c["ok"]].ravel(), got["p"][:, c["ok"]].ravel()
    host = np.array([student_t_two_sided(t, df) for t in T])
    sp = 2 * scipy.stats.t.sf(np.abs(T), df)
    print(f"assoc p {name}: max rel to the host function {float(np.max(np.abs(p / host - 1))):.2e}, "
          f"to scipy {float(np.max(np.abs(p / sp - 1))):.2e}; bit-equal to the host {int(np.sum(p == host))} of {p.size}")
    assert np.all(np.abs(p - host) <= 1e-10 * host) and np.all(np.abs(p - sp) <= 1e-10 * sp)


@gpu
@pytest.mark.parametrize("name", ["n65_r17_c17_ch64", "n257_r33_c1_rows", "n1031_r33_c16"])
def test_runs_rows_and_lists_give_the_same_bits(name):
    """Twice the same call; every row alone; the list permuted (tiles regrouped)."""
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    args = (_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"])
    again = assoc(*args, c["rows"], c["chunk"], products=True)
    assert same_bits(got, again)
    lst = c["lst"].astype(np.int32)
    perm = np.random.default_rng(7).permutation(len(lst))
    shuf = assoc(*args, lst[perm], c["chunk"], products=True)
    assert same_bits(take(got, perm), shuf)
    for j in (0, 5, 6, 7, 8, len(lst) - 1):
        one = assoc(*args, lst[j:j + 1], c["chunk"], products=True)
        assert same_bits(take(got, [j]), one), j


@gpu
def test_a_column_has_the_same_bits_in_either_pass():
    """17 columns: with the traits reversed the one column of the second pass moves into the first (and
    another takes its place); every trait's outputs and raw products keep their bits."""
    from dbslmm_amd import assoc
    name = "n65_r17_c17_ch64"
    c, got = case(name), run(name)
    P, c1 = c["P"], c["c1"]
    rev = assoc(_ctx(), c["bed"], c["n_total"], np.ascontiguousarray(c["y"][:, ::-1]), c["w"], c["keep"], c["rows"],
                c["chunk"], products=True)
    for k in ("beta", "se", "tstat", "p"):
        assert np.array_equal(got[k].view(np.uint64), rev[k][::-1].view(np.uint64)), k
    for k in ("prod_d", "prod_m"):
        assert np.array_equal(got[k][:, :c1].view(np.uint64), rev[k][:, :c1].view(np.uint64))
        assert np.array_equal(got[k][:, c1:].view(np.uint64), np.ascontiguousarray(rev[k][:, c1:][:, ::-1]).view(np.uint64))
    for k in ("n_mis", "n_obs", "status"):
        assert np.array_equal(got[k], rev[k])
    assert P == 14 and c1 + P == 17


@gpu
def test_chunking_changes_the_order_not_the_answer():
    """chunk_indiv 64 against the default on 1031 individuals: seventeen chunks against one -- the same
    integers and status, beta within the same allowance."""
    from dbslmm_amd import assoc
    c, got = case("n1031_r33_c17_ch64"), run("n1031_r33_c17_ch64")
    one = assoc(_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"], c["rows"], 0)
    for k in ("n_mis", "n_obs", "status"):
        assert np.array_equal(got[k], one[k])
    ok = c["ok"]
    dev = float(np.max(np.abs(got["beta"][:, ok] - one["beta"][:, ok]).max(axis=1) / np.abs(one["beta"][:, ok]).max(axis=1)))
    assert dev <= max(32 * c["yard"]["beta"], FLOOR)


@gpu
def test_argument_errors():
    from dbslmm_amd import DbslmmError, assoc
    c = case("n64_r15_c4_nomiss")
    args = (_ctx(), c["bed"], c["n_total"], c["y"])
    with pytest.raises(DbslmmError, match="chunk_indiv"):
        assoc(*args, c["w"], c["keep"], None, 100)
    with pytest.raises(DbslmmError, match="rank"):
        assoc(*args, np.column_stack([c["w"], 2 * c["w"][:, 0] + 1]), c["keep"])
    with pytest.raises(DbslmmError, match="n - c - 1"):
        assoc(*args, c["w"], (np.arange(64) < 4).astype(np.uint8))
    with pytest.raises(DbslmmError, match="row out of range"):
        assoc(*args, c["w"], c["keep"], [0, 99])
    with pytest.raises(DbslmmError):
        assoc(_ctx(), c["bed"], c["n_total"], np.zeros((64, 0)))

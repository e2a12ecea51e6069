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
returned T and df, and to scipy at that T, to 1e-10 relative, the bar of the host test.

The launch geometry the cases cover (test_cases_reach_the_claimed_geometry recomputes it from the
inputs, without a GPU; 16 rows per tile, 4 tiles per workgroup, 64 individuals per stage, rows padded to
256 individuals, 4096 individuals per default chunk, 16 columns per group, 256 rows per finish block):
  n7 .. n1031_r33_c17_ch64     one workgroup in x, one finish block; one chunk, or one stage per chunk;
                               at most 17 columns (the second group holds one)
  n257_r63 / r64 / r65 _ch128  four tiles, the last a row short; four live waves and no padding row; a
                               second workgroup with one live wave and three dead; chunks of two stages
  n300_r257_c3, n300_r600_c3   17 tiles in 5 workgroups and two finish blocks; 38 tiles and three finish
                               blocks under a shuffled list with repeats
  n1031_r70_c33_ch192_rows     33 columns in three groups; chunks of three stages over 20: seven chunks,
                               odd first stages, a last chunk of two
  n1031_r33_c32_ch192          32 columns: two full groups
  n4097_r17_c2 (_ch1088)       two chunks (64 + 4 stages) under the default chunk; four chunks of 17
  n1031_r33_c3_ch192_sparse    0.4 % missing calls: skipped and executed Mm steps inside one tile
  n3_r4_c1, n5_r6_c3           df = 1, without and with covariates

Exact relations, no tolerance: a trait scaled by a power of two; the same individuals dropped through
keep, a NaN phenotype or a NaN covariate; random calls outside the sample; a multi-device context and a
cached image; an empty row list."""
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
    # past one workgroup, one finish block, two column groups and one stage per chunk
    "n257_r63_c2_ch128": (257, 63, 1, 1, 128, 0.05, None),
    "n257_r64_c2_ch128": (257, 64, 1, 1, 128, 0.05, None),
    "n257_r65_c2_ch128": (257, 65, 1, 1, 128, 0.05, None),
    "n300_r257_c3": (300, 257, 1, 2, 0, 0.05, None),
    "n300_r600_c3_ch64_rows": (300, 600, 1, 2, 64, 0.05, "shuffled"),
    "n1031_r70_c33_ch192_rows": (1031, 70, 16, 17, 192, 0.05, "shuffled"),
    "n1031_r33_c32_ch192": (1031, 33, 15, 17, 192, 0.05, None),
    "n4097_r17_c2": (4097, 17, 1, 1, 0, 0.05, None),
    "n4097_r17_c2_ch1088": (4097, 17, 1, 1, 1088, 0.05, None),
    "n1031_r33_c3_ch192_sparse": (1031, 33, 1, 2, 192, 0.004, None),
    "n3_r4_c1_nomiss": (3, 4, 0, 1, 0, 0.0, None),
    "n5_r6_c3_nomiss": (5, 6, 2, 1, 0, 0.0, None),
}
EXACT_CASES = ["n1031_r70_c33_ch192_rows", "n300_r257_c3"]      # the exact relations run on these two

# the constants of assoc_layout.hpp, assoc.hip and the image's padding, restated
ROWS_PER_TILE, TILES_PER_WG, STAGE, PAD, DEFAULT_CHUNK, COLS_PER_GROUP, FINISH_BLOCK = 16, 4, 64, 256, 4096, 16, 256


def geometry(name):
    """The launch geometry of a case, from its inputs alone."""
    n_total, n_rows, c1, P, chunk, _, _ = CASES[name]
    n_pad = -(-n_total // PAD) * PAD
    n_stages = n_pad // STAGE
    spc = (chunk if chunk else DEFAULT_CHUNK) // STAGE
    n_chunks = -(-n_stages // spc)
    held = [min(n_stages, (ch + 1) * spc) - ch * spc for ch in range(n_chunks)]     # stages of every chunk
    n_tiles = -(-n_rows // ROWS_PER_TILE)
    wgs = -(-n_tiles // TILES_PER_WG)
    live_last = n_tiles - TILES_PER_WG * (wgs - 1)
    return dict(n_pad=n_pad, n_stages=n_stages, spc=spc, n_chunks=n_chunks, last_chunk=held[-1], n_tiles=n_tiles,
                wgs=wgs, live_last=live_last, dead_last=TILES_PER_WG - live_last,
                full_wg=n_rows // (ROWS_PER_TILE * TILES_PER_WG) >= 1,     # some workgroup: 4 live waves, 64 listed rows
                pad_rows=n_tiles * ROWS_PER_TILE - n_rows, finish_blocks=-(-n_rows // FINISH_BLOCK),
                n_cols=c1 + P, groups=-(-(c1 + P) // COLS_PER_GROUP),
                odd_start=any((ch * spc) % 2 == 1 and held[ch] > 1 for ch in range(n_chunks)), default_chunk=chunk == 0)


# what the table of the cases claims: (n_pad, stages per chunk, chunks, stages of the last chunk, tiles,
# workgroups in x, dead waves of the last workgroup, finish blocks, column groups)
CLAIMED = {
    "n257_r63_c2_ch128": (512, 2, 4, 2, 4, 1, 0, 1, 1),
    "n257_r64_c2_ch128": (512, 2, 4, 2, 4, 1, 0, 1, 1),
    "n257_r65_c2_ch128": (512, 2, 4, 2, 5, 2, 3, 1, 1),
    "n300_r257_c3": (512, 64, 1, 8, 17, 5, 3, 2, 1),
    "n300_r600_c3_ch64_rows": (512, 1, 8, 1, 38, 10, 2, 3, 1),
    "n1031_r70_c33_ch192_rows": (1280, 3, 7, 2, 5, 2, 3, 1, 3),
    "n1031_r33_c32_ch192": (1280, 3, 7, 2, 3, 1, 1, 1, 2),
    "n4097_r17_c2": (4352, 64, 2, 4, 2, 1, 2, 1, 1),
    "n4097_r17_c2_ch1088": (4352, 17, 4, 17, 2, 1, 2, 1, 1),
    "n1031_r33_c3_ch192_sparse": (1280, 3, 7, 2, 3, 1, 1, 1, 1),
    "n3_r4_c1_nomiss": (256, 64, 1, 4, 1, 1, 3, 1, 1),
    "n5_r6_c3_nomiss": (256, 64, 1, 4, 1, 1, 3, 1, 1),
}


def test_cases_reach_the_claimed_geometry():
    """No GPU.  Every new case has the geometry its table line claims, and the union of CASES holds
    every launch shape the suite is meant to reach."""
    geo = {name: geometry(name) for name in CASES}
    for name, want in CLAIMED.items():
        g = geo[name]
        got = (g["n_pad"], g["spc"], g["n_chunks"], g["last_chunk"], g["n_tiles"], g["wgs"], g["dead_last"],
               g["finish_blocks"], g["groups"])
        assert got == want, (name, got, want)

    def some(pred):
        return any(pred(g) for g in geo.values())
    assert some(lambda g: g["wgs"] >= 2 and g["live_last"] == 1)           # a second workgroup: one live wave, three dead
    assert some(lambda g: g["full_wg"])                                    # four live waves of listed rows
    assert some(lambda g: g["full_wg"] and g["pad_rows"] == 0)             # ... and no padding row in the launch
    assert some(lambda g: g["n_tiles"] % TILES_PER_WG == 0 and g["pad_rows"] == 1)    # the last tile a row short
    assert some(lambda g: g["finish_blocks"] == 2) and some(lambda g: g["finish_blocks"] >= 3)
    assert some(lambda g: g["groups"] == 3) and some(lambda g: g["n_cols"] == 32)
    assert some(lambda g: g["n_chunks"] >= 2 and g["spc"] >= 2 and g["odd_start"] and g["last_chunk"] < g["spc"])
    assert some(lambda g: g["n_chunks"] >= 2 and g["spc"] >= 2 and g["odd_start"] and g["last_chunk"] == g["spc"])
    assert some(lambda g: g["default_chunk"] and g["n_chunks"] == 2)
    for name in ("n3_r4_c1_nomiss", "n5_r6_c3_nomiss"):                    # df = n - c - 1 = 1 (nobody is dropped)
        assert CASES[name][0] - (CASES[name][2] + 1) - 1 == 1 and case(name)["ref"]["df"] == 1


def test_the_sparse_case_mixes_skipped_and_executed_steps():
    """No GPU.  From the decoded missing mask of the sparse case: some tile holds a missing call in
    between 10 % and 90 % of its (16 rows x 4 individuals) steps and of its (16 rows x 16 individuals)
    dwords, so the per-step and the per-dword ballot are each true and false inside that tile."""
    name = "n1031_r33_c3_ch192_sparse"
    c, g = case(name), geometry(name)
    _, miss = AR.decode(c["bed"], c["n_total"], c["lst"])
    m = np.zeros((g["n_tiles"] * ROWS_PER_TILE, g["n_pad"]), dtype=bool)      # padding rows and individuals: called
    m[:miss.shape[0], :miss.shape[1]] = miss
    m = m.reshape(g["n_tiles"], ROWS_PER_TILE, g["n_pad"]).any(axis=1)        # [tile, individual]
    steps = m.reshape(g["n_tiles"], -1, 4).any(axis=2).mean(axis=1)
    dwords = m.reshape(g["n_tiles"], -1, 16).any(axis=2).mean(axis=1)
    print(f"assoc {name}: share of steps / dwords with a missing call per tile {np.round(steps, 3)} / {np.round(dwords, 3)}")
    assert np.any((steps >= 0.1) & (steps <= 0.9) & (dwords >= 0.1) & (dwords <= 0.9))


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
    # the references, the yardsticks and the preconditions of the measured comparison (n_obs >= c + 2 and
    # xPx / ssx >= 1e-3 on every OK row), from the reference alone
    ref, ok, yard = AR.measured(bed, n_total, y, w, keep, lst)
    assert ref["design"]["c"] == c1 + 1
    for k, r in planted.items():
        want = dict(no_call=AR.NO_CALL, miss_outside=AR.OK, mono=AR.MONOMORPHIC, collinear=AR.COLLINEAR)[k]
        assert np.all(ref["status"][lst == r] == want), (k, ref["status"][lst == r])
    if "miss_outside" in planted:
        assert np.all(ref["n_mis"][lst == 6] == 0)
    if planted:
        assert ref["n_mis"].max() > 0 and {0, 1, 2, 3} <= set(np.unique((bed[3:, None] >> [0, 2, 4, 6]) & 3))
    return dict(n_total=n_total, n_rows=n_rows, c1=c1, P=P, chunk=chunk, bed=bed, y=y, w=w, keep=keep, rows=rows,
                lst=lst, ref=ref, ok=ok, yard=yard, g=g, m=m, planted=planted)


@pytest.mark.parametrize("name", list(CASES))
def test_case_preconditions_hold_on_the_reference(name):
    """No GPU.  case() asserts, from the restatement alone, that every planted status holds and that every
    OK row has n_obs >= c + 2 and xPx / ssx >= 1e-3; the measured comparison then leaves out no OK row."""
    c = case(name)
    assert c["ok"].sum() >= 1 and len(c["lst"]) == c["n_rows"]
    print(f"assoc {name}: OK rows {int(c['ok'].sum())} of {c['n_rows']}, smallest xPx / ssx "
          f"{float(np.min(c['ref']['xPx'][c['ok']] / c['ref']['ssx'][c['ok']])):.3g}, yardstick beta {c['yard']['beta']:.1e} "
          f"T {c['yard']['tstat']:.1e}")


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
    ok = c["ok"]
    dev = AR.deviation(got, c["ref"], ok)
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
@pytest.mark.parametrize("name", ["n65_r17_c17_ch64", "n257_r33_c1_rows", "n1031_r33_c16", "n300_r257_c3"])
def test_runs_rows_and_lists_give_the_same_bits(name):
    """Twice the same call; rows alone (the planted ones, and the first and last row of a tile and of a
    workgroup); the list permuted (tiles regrouped: with 257 rows a row changes tile, wave and workgroup)."""
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    args = (_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"])
    again = assoc(*args, c["rows"], c["chunk"], products=True)
    assert same_bits(got, again)
    lst = c["lst"].astype(np.int32)
    perm = np.random.default_rng(7).permutation(len(lst))
    if len(lst) > ROWS_PER_TILE * TILES_PER_WG:
        was, now = perm, np.arange(len(lst))                   # row perm[i] of the full call is row i of the permuted one
        assert np.any((was // 64 != now // 64) & (was // 16 % 4 != now // 16 % 4) & (was % 16 != now % 16))
    shuf = assoc(*args, lst[perm], c["chunk"], products=True)
    assert same_bits(take(got, perm), shuf)
    for j in sorted({j for j in (0, 5, 6, 7, 8, 15, 16, 63, 64) if j < len(lst)} | {len(lst) - 1}):
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
    """chunk_indiv 64, 128, 192 and 1088 against the default on 1031 individuals (20 stages): twenty chunks
    of one stage, ten of two, seven of three (the last of two) and two of 17 and 3 against one chunk -- the
    same integers and status, beta within the same allowance."""
    from dbslmm_amd import assoc
    c, got = case("n1031_r33_c17_ch64"), run("n1031_r33_c17_ch64")
    args = (_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"], c["rows"])
    one = assoc(*args, 0)
    ok = c["ok"]
    for chunk in (64, 128, 192, 1088):
        other = got if chunk == c["chunk"] else assoc(*args, chunk)
        for k in ("n_mis", "n_obs", "status"):
            assert np.array_equal(other[k], one[k]), (chunk, k)
        dev = float(np.max(np.abs(other["beta"][:, ok] - one["beta"][:, ok]).max(axis=1) / np.abs(one["beta"][:, ok]).max(axis=1)))
        print(f"assoc chunk_indiv {chunk} against 0: beta {dev:.2e}")
        assert dev <= max(32 * c["yard"]["beta"], FLOOR), chunk


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@gpu
@pytest.mark.parametrize("factor", [-1.0, 2.0 ** 40, 2.0 ** -40, -2.0 ** 100])
@pytest.mark.parametrize("name", EXACT_CASES)
def test_scaling_a_trait_by_a_power_of_two_is_exact(name, factor):
    """One phenotype column times c = -1, 2^40, 2^-40, -2^100: that trait's beta and raw-product column are c
    times the clean run's under ==, its se |c| times, its T sign(c) times, its p the same bits; status,
    n_mis, n_obs, af, every other trait and every other column of prod_d / prod_m keep their bits.  No
    tolerance applies: the host QR does not see the traits; Yr, yy, the fp64 MFMA chain, the sum over the
    chunks and finish_row are linear in the trait (yy and s2 quadratic, se their square root) with one
    rounding per operation, and a product with a power of two commutes with every such rounding while
    nothing overflows or goes subnormal -- contracted into an FMA or not."""
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    P, c1, ok = c["P"], c["c1"], c["ok"]
    q = P - 1 if abs(factor) > 1 else 0                        # (column P - 1 is the last group's, and holds the NaN)
    y = c["y"].copy()
    y[:, q] *= factor
    sc = assoc(_ctx(), c["bed"], c["n_total"], y, c["w"], c["keep"], c["rows"], c["chunk"], products=True)
    col = c1 + q
    rest = [k for k in range(c1 + P) if k != col]
    for k in ("prod_d", "prod_m"):
        assert np.all(sc[k][:, col] == factor * got[k][:, col]), k
        assert np.array_equal(_bits(sc[k][:, rest]), _bits(got[k][:, rest])), k
    assert np.any(got["prod_d"][:, col] != 0) and np.any(got["prod_m"][:, col] != 0)
    assert np.all(sc["beta"][q, ok] == factor * got["beta"][q, ok])
    assert np.all(sc["se"][q, ok] == abs(factor) * got["se"][q, ok])
    assert np.all(sc["tstat"][q, ok] == np.sign(factor) * got["tstat"][q, ok])
    assert np.array_equal(_bits(sc["p"][q, ok]), _bits(got["p"][q, ok]))
    others = [t for t in range(P) if t != q]
    for k in ("beta", "se", "tstat", "p"):
        assert np.all(np.isnan(sc[k][:, ~ok]))
        assert np.array_equal(_bits(sc[k][others][:, ok]), _bits(got[k][others][:, ok])), k
    for k in ("status", "n_mis", "n_obs"):
        assert np.array_equal(sc[k], got[k]), k
    assert np.array_equal(_bits(sc["af"]), _bits(got["af"]))


@gpu
@pytest.mark.parametrize("name", EXACT_CASES)
def test_three_ways_out_of_the_sample_give_the_same_bits(name):
    """The same five individuals dropped through keep = 0, through a NaN phenotype and through a NaN
    covariate: the same S, so every output and both raw products are identical bit for bit; and the
    integers are the restatement's for that S."""
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    n_total, P, c1 = c["n_total"], c["P"], c["c1"]
    extra = np.array([1, 17, 66, 129, 299])
    assert np.all(c["ref"]["design"]["in_s"][extra]) and c1 >= 1
    keep, y, w = c["keep"].copy(), c["y"].copy(), c["w"].copy()
    keep[extra] = 0
    y[extra, np.arange(len(extra)) % P] = np.nan
    w[extra, np.arange(len(extra)) % c1] = np.nan
    tail = (c["rows"], c["chunk"])
    by_keep = assoc(_ctx(), c["bed"], n_total, c["y"], c["w"], keep, *tail, products=True)
    by_pheno = assoc(_ctx(), c["bed"], n_total, y, c["w"], c["keep"], *tail, products=True)
    by_covar = assoc(_ctx(), c["bed"], n_total, c["y"], w, c["keep"], *tail, products=True)
    assert same_bits(by_keep, by_pheno) and same_bits(by_keep, by_covar)
    assert not np.array_equal(by_keep["n_obs"], got["n_obs"])
    ref = AR.scan(c["bed"], n_total, c["y"], c["w"], keep, c["lst"])
    for k in ("n_mis", "n_obs", "status"):
        assert np.array_equal(by_keep[k], ref[k]), k


@gpu
@pytest.mark.parametrize("name", EXACT_CASES)
def test_calls_outside_the_sample_do_not_matter(name):
    """Every individual outside S gets random codes (40 % of them missing) in every row: the per-dword and
    per-step ballots change, V is zero there, and every output and both raw products keep their bits."""
    from dbslmm_amd import assoc
    c, got = case(name), run(name)
    out = ~c["ref"]["design"]["in_s"]
    rng = np.random.default_rng(5)
    g, m = c["g"].copy(), c["m"].copy()
    g[:, out] = rng.integers(0, 3, size=(g.shape[0], int(out.sum())))
    m[:, out] = rng.random((g.shape[0], int(out.sum()))) < 0.4
    bed = AR.encode(g, m)
    assert out.sum() >= 10 and np.any(m[:, out] != c["m"][:, out]) and bed.shape == c["bed"].shape
    other = assoc(_ctx(), bed, c["n_total"], c["y"], c["w"], c["keep"], c["rows"], c["chunk"], products=True)
    assert same_bits(got, other)


@gpu
def test_other_contexts_give_the_bytes_of_a_plain_one():
    """A context over [0, 0] runs the scan on its first device, and a context's cached image serves the
    same answer: the bytes of a plain one-device context."""
    from dbslmm_amd import Context, assoc
    name = "n300_r257_c3"
    c, got = case(name), run(name)
    args = (c["bed"], c["n_total"], c["y"], c["w"], c["keep"], c["rows"], c["chunk"])
    assert same_bits(got, assoc(Context([0, 0]), *args, products=True))
    ctx = Context(0)
    ctx.cache_bed(c["bed"])
    assert same_bits(got, assoc(ctx, *args, products=True))


@gpu
def test_an_empty_row_list():
    """rows = []: empty arrays and no error; a bad design is still refused."""
    from dbslmm_amd import DbslmmError, assoc
    c = case("n64_r15_c4_nomiss")
    out = assoc(_ctx(), c["bed"], c["n_total"], c["y"], c["w"], c["keep"], [], products=True)
    P, c1 = c["P"], c["c1"]
    for k in ("n_mis", "n_obs", "status", "af"):
        assert out[k].shape == (0,), k
    for k in ("beta", "se", "tstat", "p"):
        assert out[k].shape == (P, 0), k
    assert out["prod_d"].shape == (0, c1 + P) and out["prod_m"].shape == (0, c1 + P)
    with pytest.raises(DbslmmError, match="rank"):
        assoc(_ctx(), c["bed"], c["n_total"], c["y"], np.column_stack([c["w"], 2 * c["w"][:, 0] + 1]), c["keep"], [])


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

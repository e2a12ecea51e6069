// ldscore.hip -- LD scores of listed panel rows (dbslmm_ld_scores): what the reference's manual
// leaves to LDSC (Rmd/Manual.Rmd:170), the dense case of clump.hip.
//
//   dbslmm_l2_tiles    one 256-thread workgroup per 128 x 128 tile of the band of ldsc_layout.hpp
//                      (rows in position order; rows past the list read the zero-dosage row).  A tile
//                      without a missing call runs dbslmm_gram_big's K loop: stages of 256
//                      individuals through double-buffered LDS at the 144-B row stride, raw-form
//                      FP4 expansion on the way in, global loads two stages ahead, wave w the 64 x 64
//                      quadrant (w >> 1, w & 1) = 2 x 2 MFMA sub-tiles of 32 x 32; a diagonal tile
//                      stages one operand and skips the quadrant (0, 1).  A tile with a missing call
//                      in any of its up to 256 rows (flag from the host layout) takes the four
//                      products of the observed-call expansion per 32 x 32 sub-tile, operands
//                      straight from the image rows, sub-tile q on wave q & 3 -- dbslmm_r2_tiles' loop.
//   dbslmm_l2_reduce   one thread per position: the sequential sum of its slots.
//
// Per element the epilogue forms r2 exactly as dbslmm_r2_tiles does (raw: the exact integers N and
// D, three roundings; four products: the fp64 form, NaN unless css_i css_j > 0).  What depends on
// one row only -- S, D = n sq - S^2 (int64), gram_exact's term, the moments -- is formed once per
// position and staged in LDS (l2::Meta); N = n G - S_i S_j is formed in fp64, where it is exact (both
// products are integers below 2^45), instead of 64-bit integer multiplies per element.  Then
//     t = r2                               (unbiased == 0)
//     t = fma(r2, n - 1, -1) / (n - 2)     (= r2 - (1 - r2) / (n - 2), ldsc's adjustment: one
//                                           rounding of (n - 2) t, one of the quotient)
// and counts the element when both positions are listed, lie on one chromosome with |bp_i - bp_j|
// <= window and r2 is not NaN.  An off-diagonal tile (ti < tj) counts every element: t goes to the
// row sum of i and the column sum of j.  A diagonal tile counts the elements with i >= j (r2 is
// symmetric; the quadrant above is the one skipped): t goes to the row sum of i and, when i != j,
// to the column sum of j, so the self term is added once.  A NaN pair adds to neither side.
//
// Reduction order (fixed: ℓ is bit-identical from run to run and for every slice size).
//   1. In a 32 x 32 sub-tile (MFMA C/D layout: lane l holds column l & 31, rows (r & 3) + 8 (r >> 2)
//      + 4 (l >> 5), r = 0 .. 15) a column's sum is the lane's 16 terms added in r order, then the
//      sum of the two lane halves (one xor-32 exchange); a row's sum is a halving butterfly over its
//      32 lanes (sub_epilogue): exchanges at xor 16, 8, 4, 2, each lane adding what it receives to
//      what it kept, then xor 1.
//   2. The sub-tile stores its 32 row sums and 32 column sums to LDS, part[row][sj] and
//      part[128 + column][si] ((si, sj) the sub-tile of the 4 x 4); skipped sub-tiles leave 0.
//   3. Thread k < 128 adds row k's four parts in sj order, thread 128 + k column k's in si order,
//      and stores the sum to the tile's slot: 128 row sums, then 128 column sums.  No atomics.
//   4. dbslmm_l2_reduce adds, for position p of tile row P, the column slots of the tiles (I, P) in
//      ascending I and then the row slots of the tiles (P, J) in ascending J: ascending tile index,
//      a tile's column slot before its row slot.  Slices of the tile list continue the same
//      sequence in the running sum.  The last slice writes ℓ in the caller's order, NaN for a row
//      without variance or without an observed call (from the row table's integers).
#include "ldsc_layout.hpp"

namespace l2 {

// the per-position inputs of a tile's epilogue, formed once per position (thread) from the row table
// entry {sum, sumsq, nmiss} and staged in LDS: [0, 128) the tile's rows, [128, 256) its columns
struct Meta {
    double dS[2 * kL2Tile];             // dosage sum S
    double D[2 * kL2Tile];              // n sq - S^2, formed in int64 (< 2^45: exact as a double)
    double mu[2 * kL2Tile];             // clump::moments of the row (the four-product form)
    double css[2 * kL2Tile];
    int64_t bp[2 * kL2Tile];
    int32_t chr[2 * kL2Tile];
    int32_t gterm[2 * kL2Tile];         // gram_exact's term: gram_row of a row, gram_col of a column
    double part[2 * kL2Tile][4];        // step 2 of the reduction order
};
static_assert(sizeof(Meta) <= gram::kLdsBytes, "the epilogue reuses the K loop's LDS");
static_assert(kL2Tile == gram::kGT, "dbslmm_gram_big's tile");

// t of one pair from its r2
__device__ __forceinline__ double adjust(double r2, int32_t unbiased, double nm1, double nm2) {
    return unbiased ? __builtin_fma(r2, nm1, -1.0) / nm2 : r2;
}

// Epilogue of the 32 x 32 sub-tile (si, sj) of a tile held by one wave in the MFMA C/D layout: steps
// 1 and 2 of the reduction order.  missing: the four-product form (acc = GG; go, og, oo).
__device__ __forceinline__ void sub_epilogue(const v16f& acc, const v16f& go, const v16f& og, const v16f& oo,
                                             bool missing, int si, int sj, bool diag, int r0, int c0, int32_t n,
                                             int32_t n_ref, int64_t kpad, int64_t window, int32_t unbiased,
                                             Meta* M, int lane) {
    const int sub = lane & 31, half = lane >> 5;
    const int jl = kL2Tile + 32 * sj + sub;                     // this lane's column in Meta
    const int pj = c0 + 32 * sj + sub;
    const double dnn = static_cast<double>(n_ref);
    const double dSj = M->dS[jl], Dj = M->D[jl], muj = M->mu[jl], cssj = M->css[jl];
    const int cj = M->gterm[jl];
    const double pad_k = static_cast<double>(kpad - n_ref);
    const double nm1 = static_cast<double>(n_ref - 1), nm2 = static_cast<double>(n_ref - 2);
    const int32_t chrj = M->chr[jl];
    const int64_t bpj = M->bp[jl];
    double colsum = 0.0;
    double t[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int il = 32 * si + i;
        const int pi = r0 + il;
        double r2;
        if (!missing) {
            // dbslmm_r2_tiles' N = n G - S_i S_j in fp64: both products are integers below 2^45 and so
            // is their difference, so dn is (double)N exactly and r2 has the same three roundings
            const double dG = static_cast<double>(gram_exact(acc[r], M->gterm[il], cj));
            const double dn = dnn * dG - M->dS[il] * dSj;
            r2 = dn * dn / (M->D[il] * Dj);
        } else {
            const double mui = M->mu[il];
            const double c = ((static_cast<double>(acc[r]) - muj * static_cast<double>(go[r])) -
                              mui * static_cast<double>(og[r])) +
                             (mui * muj) * (static_cast<double>(oo[r]) - pad_k);   // padding counts as observed
            const double den = M->css[il] * cssj;
            r2 = den > 0.0 ? c * c / den : __builtin_nan("");
        }
        const int64_t d = M->bp[il] - bpj;
        const bool in = pi < n && pj < n && (!diag || pi >= pj) && M->chr[il] == chrj &&
                        (d < 0 ? -d : d) <= window && r2 == r2;
        t[r] = in ? adjust(r2, unbiased, nm1, nm2) : 0.0;
        if (!diag || pi != pj) colsum += t[r];
    }
    // row sums: the halving butterfly over a row's 32 lanes (one lane half) -- 16 exchanges for the 16
    // rows of a lane instead of 80.  At the step of lane bit b a lane keeps the half of its values
    // whose register-index bit matches its own bit b, sends the other half to lane ^ b and adds what
    // it receives to what it kept (bit 16 <-> register bit 3, 8 <-> 2, 4 <-> 1, 2 <-> 0); after four
    // steps it holds register r = bits 1 .. 4 of its lane number summed over the 16 lanes of its
    // parity, and the xor-1 exchange adds the other 16.
    double v8[8], v4[4], v2[2];
    const bool b16 = (sub & 16) != 0, b8 = (sub & 8) != 0, b4 = (sub & 4) != 0, b2 = (sub & 2) != 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v8[k] = (b16 ? t[k + 8] : t[k]) + __shfl_xor(b16 ? t[k] : t[k + 8], 16, kWave);
#pragma unroll
    for (int k = 0; k < 4; ++k) v4[k] = (b8 ? v8[k + 4] : v8[k]) + __shfl_xor(b8 ? v8[k] : v8[k + 4], 8, kWave);
#pragma unroll
    for (int k = 0; k < 2; ++k) v2[k] = (b4 ? v4[k + 2] : v4[k]) + __shfl_xor(b4 ? v4[k] : v4[k + 2], 4, kWave);
    double rowsum = (b2 ? v2[1] : v2[0]) + __shfl_xor(b2 ? v2[0] : v2[1], 2, kWave);
    rowsum += __shfl_xor(rowsum, 1, kWave);
    {
        const int r = sub >> 1;             // the register this lane pair holds
        if ((sub & 1) == 0) M->part[32 * si + (r & 3) + 8 * (r >> 2) + 4 * half][sj] = rowsum;
    }
    colsum += __shfl_xor(colsum, 32, kWave);
    if (half == 0) M->part[jl][si] = colsum;
}

}  // namespace l2

// (two workgroups per compute unit, as dbslmm_gram_big runs: two waves per SIMD bound the registers)
__global__ __launch_bounds__(256, 2) void dbslmm_l2_tiles(
    const uint8_t* __restrict__ img, int64_t kpad, const v4i* __restrict__ tab, int32_t zrow, int32_t n_ref,
    const int32_t* __restrict__ pos, int32_t n, const L2Tile* __restrict__ tiles, int32_t n_tiles,
    const int32_t* __restrict__ chr, const int64_t* __restrict__ bp, int64_t window, int32_t unbiased,
    double* __restrict__ slots) {
    using namespace gram;
    extern __shared__ __attribute__((aligned(16))) int8_t glds[];
    if (static_cast<int>(blockIdx.x) >= n_tiles) return;
    const L2Tile tile = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = kL2Tile * tile.ti, c0 = kL2Tile * tile.tj;
    const bool diag = tile.ti == tile.tj;
    const bool missing = tile.missing != 0;
    const int64_t kw = kpad / 16;           // image dwords per row (kpad: a multiple of 256)
    l2::Meta* M = reinterpret_cast<l2::Meta*>(glds);
    // thread tid stages position (tid < 128: row r0 + tid; else column c0 + tid - 128) for the epilogue
    auto stage_meta = [&]() {
        const int p = tid < kL2Tile ? r0 + tid : c0 + tid - kL2Tile;
        const v4i e = tab[clump::row_of(pos, p, n, zrow)];
        const int64_t nn = n_ref, S = e[0];
        M->dS[tid] = static_cast<double>(e[0]);
        M->D[tid] = static_cast<double>(nn * e[1] - S * S);
        clump::moments(n_ref, e, M->mu[tid], M->css[tid]);
        M->gterm[tid] = tid < kL2Tile ? gram_row(static_cast<double>(e[0]), kpad) : gram_col(static_cast<double>(e[0]));
        M->chr[tid] = p < n ? chr[p] : 0;
        M->bp[tid] = p < n ? bp[p] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) M->part[tid][k] = 0.0;
    };
    const v16f zero = {0.0f};
    if (missing) {   // four-product form, 4 x 4 sub-tiles of 32, 4 per wave: dbslmm_r2_tiles' K loop
        stage_meta();
        __syncthreads();
        const int sub = lane & 31, half = lane >> 5;
        for (int q = wave; q < 16; q += 4) {
            const int si = q >> 2, sj = q & 3;
            if (diag && sj > si) continue;
            if (r0 + 32 * si >= n || c0 + 32 * sj >= n) continue;       // wholly past the list
            const uint32_t* pa = reinterpret_cast<const uint32_t*>(img) +
                                 clump::row_of(pos, r0 + 32 * si + sub, n, zrow) * kw + 4 * half;
            const uint32_t* pb = reinterpret_cast<const uint32_t*>(img) +
                                 clump::row_of(pos, c0 + 32 * sj + sub, n, zrow) * kw + 4 * half;
            v16f acc = zero, acc_go = zero, acc_og = zero, acc_oo = zero;
            for (int64_t w = 0; w < kw; w += 8) {
                const v4i wa = *reinterpret_cast<const v4i*>(pa + w);
                const v4i wb = *reinterpret_cast<const v4i*>(pb + w);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    uint32_t ga0, oa0, ga1, oa1, gb0, ob0, gb1, ob1;
                    split_missing(static_cast<uint32_t>(wa[2 * h]), ga0, oa0);
                    split_missing(static_cast<uint32_t>(wa[2 * h + 1]), ga1, oa1);
                    split_missing(static_cast<uint32_t>(wb[2 * h]), gb0, ob0);
                    split_missing(static_cast<uint32_t>(wb[2 * h + 1]), gb1, ob1);
                    const v4i ga = fp4_chunk(ga0, ga1), oa = fp4_chunk(oa0, oa1);
                    const v4i gb = fp4_chunk(gb0, gb1), ob = fp4_chunk(ob0, ob1);
                    acc = mfma_fp4(ga, gb, acc);
                    acc_go = mfma_fp4(ga, ob, acc_go);
                    acc_og = mfma_fp4(oa, gb, acc_og);
                    acc_oo = mfma_fp4(oa, ob, acc_oo);
                }
            }
            l2::sub_epilogue(acc, acc_go, acc_og, acc_oo, true, si, sj, diag, r0, c0, n, n_ref, kpad, window,
                             unbiased, M, lane);
        }
    } else {
        // dbslmm_gram_big's staging map: 128 rows x 16 image dwords per operand and stage; thread t moves
        // dword pairs e = t + 256 q (row e >> 3, pair e & 7) and expands each pair to one 16-B FP4
        // chunk (raw form) on the way into LDS.  Two register sets: the global loads of stage s + 2
        // are issued before stage s's MFMAs.
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        const uint32_t *ga[4], *gb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = q * 256 + tid, r = e >> 3, c = e & 7;
            ga[q] = reinterpret_cast<const uint32_t*>(img) + clump::row_of(pos, r0 + r, n, zrow) * kw + 2 * c;
            gb[q] = diag ? ga[q]
                         : reinterpret_cast<const uint32_t*>(img) + clump::row_of(pos, c0 + r, n, zrow) * kw + 2 * c;
        }
        const uint32_t k44 = raw_k44();
        u2 ra0[4], rb0[4], ra1[4], rb1[4];
        auto gload = [&](u2 (&ra)[4], u2 (&rb)[4], int st) {
            const int64_t w0 = static_cast<int64_t>(st) * (kKS / 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = *reinterpret_cast<const u2*>(ga[q] + w0);
                if (!diag) rb[q] = *reinterpret_cast<const u2*>(gb[q] + w0);
            }
        };
        auto lstore = [&](const u2 (&ra)[4], const u2 (&rb)[4], int buf) {
            int8_t* A = glds + buf * 2 * kOpBytes;
            int8_t* B = A + kOpBytes;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = q * 256 + tid, r = e >> 3, c = e & 7;
                *reinterpret_cast<v4i*>(A + r * kRS + 16 * c) = fp4_chunk_raw(ra[q][0], ra[q][1], k44);
                if (!diag) *reinterpret_cast<v4i*>(B + r * kRS + 16 * c) = fp4_chunk_raw(rb[q][0], rb[q][1], k44);
            }
        };
        const int wr = wave >> 1, wc = wave & 1;
        const bool idle = diag && wc > wr;            // strictly-upper quadrant of a diagonal tile
        v16f acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = zero;
        const int rsub = lane & 31, ksub = 16 * (lane >> 5);
        auto compute = [&](int buf) {
            if (idle) return;
            const int8_t* A = glds + buf * 2 * kOpBytes;
            const int8_t* B = diag ? A : A + kOpBytes;
            const int8_t* pa = A + (64 * wr + rsub) * kRS + ksub;
            const int8_t* pb = B + (64 * wc + rsub) * kRS + ksub;
#pragma unroll
            for (int kk = 0; kk < kKS / 2; kk += 32) {
                const v4i a0 = *reinterpret_cast<const v4i*>(pa + kk);
                const v4i a1 = *reinterpret_cast<const v4i*>(pa + 32 * kRS + kk);
                const v4i b0 = *reinterpret_cast<const v4i*>(pb + kk);
                const v4i b1 = *reinterpret_cast<const v4i*>(pb + 32 * kRS + kk);
                acc[0][0] = mfma_fp4_raw(a0, b0, acc[0][0]);
                acc[0][1] = mfma_fp4_raw(a0, b1, acc[0][1]);
                acc[1][0] = mfma_fp4_raw(a1, b0, acc[1][0]);
                acc[1][1] = mfma_fp4_raw(a1, b1, acc[1][1]);
            }
        };
        const int nst = static_cast<int>(kpad / kKS);
        gload(ra0, rb0, 0);
        lstore(ra0, rb0, 0);
        if (nst > 1) gload(ra1, rb1, 1);
        __syncthreads();
        for (int st = 0; st < nst; st += 2) {
            if (st + 2 < nst) gload(ra0, rb0, st + 2);
            compute(0);
            if (st + 1 < nst) lstore(ra1, rb1, 1);
            __syncthreads();
            if (st + 1 >= nst) break;
            if (st + 3 < nst) gload(ra1, rb1, st + 3);
            compute(1);
            if (st + 2 < nst) lstore(ra0, rb0, 0);
            __syncthreads();
        }
        // the K loop's last barrier has passed: no wave reads the stages any more
        stage_meta();
        __syncthreads();
        if (!idle) {
#pragma unroll
            for (int si = 0; si < 2; ++si)
#pragma unroll
                for (int sj = 0; sj < 2; ++sj)
                    l2::sub_epilogue(acc[si][sj], zero, zero, zero, false, 2 * wr + si, 2 * wc + sj, diag, r0, c0, n,
                                     n_ref, kpad, window, unbiased, M, lane);
        }
    }
    __syncthreads();
    // step 3: thread k < 128 row k, thread 128 + k column k
    slots[static_cast<int64_t>(blockIdx.x) * kL2SlotWords + tid] =
        ((M->part[tid][0] + M->part[tid][1]) + M->part[tid][2]) + M->part[tid][3];
}

// Step 4 of the reduction order for the tiles [t0, t1) of the list (their slots at slots[0 ..)):
// run[p] continues the sequential sum of position p.  last: ℓ in the caller's order.
__global__ __launch_bounds__(256) void dbslmm_l2_reduce(
    const double* __restrict__ slots, int32_t t0, int32_t t1, const int32_t* __restrict__ row_ptr,
    const int32_t* __restrict__ col_lo, int32_t n, double* __restrict__ run, int32_t last,
    const v4i* __restrict__ tab, const int32_t* __restrict__ pos, int32_t n_ref, const int32_t* __restrict__ order,
    double* __restrict__ out) {
    const int32_t p = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
    if (p >= n) return;
    const int32_t P = p / kL2Tile, e = p % kL2Tile;
    double s = run[p];
    for (int32_t I = col_lo[P]; I <= P; ++I) {
        const int32_t t = row_ptr[I] + (P - I);
        if (t >= t0 && t < t1) s += slots[static_cast<int64_t>(t - t0) * kL2SlotWords + kL2Tile + e];
    }
    const int32_t ta = row_ptr[P] > t0 ? row_ptr[P] : t0, tb = row_ptr[P + 1] < t1 ? row_ptr[P + 1] : t1;
    for (int32_t t = ta; t < tb; ++t) s += slots[static_cast<int64_t>(t - t0) * kL2SlotWords + e];
    run[p] = s;
    if (last) {
        const v4i en = tab[pos[p]];
        const int64_t m = static_cast<int64_t>(n_ref) - en[2], S = en[0];
        const bool nan_row = m <= 0 || m * en[1] - S * S == 0;   // no observed call, or no variance
        out[order[p]] = nan_row ? __builtin_nan("") : s;
    }
}

// clump.hip -- LD r2 between rows of the reference panel, for clumping (what software/DBSLMM.R:
// 139-145 leaves to `plink --clump`) and as a dense matrix (dbslmm_ld_r2).
//
//   dbslmm_r2_tiles   one wave per 32 x 32 tile of row pairs (clump_layout.hpp: the band of a
//                     candidate list in position order, or every tile of a dense list), like
//                     dbslmm_gram_i8: operands straight from the panel image rows (L2), FP4 MFMAs
//                     from the shared helpers of kernels.hip, K over all kpad individuals.  Tile
//                     rows and columns past the list read the zero-dosage row.  The per-row integers
//                     {sum, sumsq, nmiss} are gathered from the image's row table by bed row: no
//                     statistics pass, no slot arrays.
//
// r_ij is the Pearson correlation of the two rows' dosages over the n_ref individuals, missing calls
// at the row mean (readSNPIm's convention, the centred sums of row_moments and the Gram's
// missing-call form).  A tile whose 64 rows hold no missing call takes the raw form and EXACT
// numerators: with the integer Gram G_ij (gram_exact), N = n G_ij - S_i S_j and D_i = n sq_i - S_i^2
// in int64 (n G <= 4 n^2 < 1.4e13 under the cap 9 kpad < 2^24), then
//     r2 = (double)N (double)N / ((double)D_i (double)D_j):
// exact conversions and three roundings, so r2 is within 3 * 2^-53 (relative) of the true quotient
// and the comparison with the threshold can differ from the exact one only that close to it.  A tile
// with a missing call in any of its rows (wave-uniform, from the table entries) takes the four
// products of the observed-call expansion and the fp64 form of the Gram's missing-call epilogue,
//     c = GG - mu_j GO - mu_i OG + mu_i mu_j (OO - pad_k),   r2 = c c / (css_i css_j),
// css the centred sum of squares as row_moments forms it.  A row without variance or without an
// observed call gives 0 / 0 = NaN on both paths; NaN compares false, so such a row is never linked.
//
// Two outputs (template flag):
//   mask mode   per tile 64 words: word r = the tile columns c linked to tile row r, word 32 + c =
//               the tile rows linked to tile column c, where "linked" = both inside the list, row
//               position < column position, same chr, |bp_i - bp_j| <= window and r2 >= thr.  In the
//               MFMA C/D layout a tile row's 32 columns sit in one lane half, so one __ballot per
//               accumulator register gives two row masks; the column masks are the OR of the two
//               lane halves' bits.  Each lane then picks one word: one 256-byte vector store.
//   value mode  r2 as fp64 into a dense n x n array, both (i, j) and (j, i) from the one value
//               computed for i <= j (symmetric bit for bit).
#include "clump_layout.hpp"

namespace clump {

// mean over the observed calls and centred sum of squares of a row from its table entry: the
// expressions of row_moments (kernels.hip)
__device__ __forceinline__ void moments(int32_t n_ref, v4i e, double& mu, double& css) {
    const double dc = static_cast<double>(n_ref - e[2]);
    const double ds = static_cast<double>(e[0]);
    mu = ds / dc;
    css = static_cast<double>(e[1]) - ds * ds / dc;
}

// image row of list position p (past the list: the zero-dosage row)
__device__ __forceinline__ int32_t row_of(const int32_t* __restrict__ pos, int32_t p, int32_t n, int32_t zrow) {
    return p < n ? pos[p] : zrow;
}

}  // namespace clump

template <bool kMask>
__global__ __launch_bounds__(256) void dbslmm_r2_tiles(
    const uint8_t* __restrict__ img, int64_t kpad, const v4i* __restrict__ tab, int32_t zrow, int32_t n_ref,
    const int32_t* __restrict__ pos, int32_t n, const ClumpTile* __restrict__ tiles, int32_t n_tiles,
    const int32_t* __restrict__ chr, const int64_t* __restrict__ bp, double thr, int64_t window,
    uint32_t* __restrict__ masks, double* __restrict__ r2_out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int t = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (t >= n_tiles) return;
    const ClumpTile tile = tiles[t];
    const int r0 = kClumpTile * tile.ti, c0 = kClumpTile * tile.tj;
    const int sub = lane & 31, half = lane >> 5;
    const int32_t rowa = clump::row_of(pos, r0 + sub, n, zrow), rowb = clump::row_of(pos, c0 + sub, n, zrow);
    const v4i eb = tab[rowb];               // this lane's column
    const bool missing = __ballot(tab[rowa][2] > 0 || eb[2] > 0) != 0;   // any of the tile's 64 rows

    const int64_t kw = kpad / 16;           // image dwords per row (kpad: a multiple of 256, kw of 16)
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(img) + rowa * kw + 4 * half;
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(img) + rowb * kw + 4 * half;
    // K loop: per 128 individuals (8 image dwords) lane (row, half) loads dwords 4 half .. 4 half + 3
    // of its row per operand and feeds two MFMAs (the individual -> k map of gram_tile32: the same on
    // both operands, so every product sums each individual once); two such steps per trip
    v16f acc = {0.0f};
    v16f acc_go = {0.0f}, acc_og = {0.0f}, acc_oo = {0.0f};
    if (!missing) {                         // raw form: acc = T (gram_exact in the epilogue)
        const uint32_t k44 = raw_k44();
        for (int64_t w = 0; w < kw; w += 16) {
            const v4i wa0 = *reinterpret_cast<const v4i*>(pa + w), wa1 = *reinterpret_cast<const v4i*>(pa + w + 8);
            const v4i wb0 = *reinterpret_cast<const v4i*>(pb + w), wb1 = *reinterpret_cast<const v4i*>(pb + w + 8);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                acc = mfma_fp4_raw(fp4_chunk_raw(static_cast<uint32_t>(wa0[2 * q]), static_cast<uint32_t>(wa0[2 * q + 1]), k44),
                                   fp4_chunk_raw(static_cast<uint32_t>(wb0[2 * q]), static_cast<uint32_t>(wb0[2 * q + 1]), k44), acc);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                acc = mfma_fp4_raw(fp4_chunk_raw(static_cast<uint32_t>(wa1[2 * q]), static_cast<uint32_t>(wa1[2 * q + 1]), k44),
                                   fp4_chunk_raw(static_cast<uint32_t>(wb1[2 * q]), static_cast<uint32_t>(wb1[2 * q + 1]), k44), acc);
        }
    } else {
        for (int64_t w = 0; w < kw; w += 8) {
            const v4i wa = *reinterpret_cast<const v4i*>(pa + w);
            const v4i wb = *reinterpret_cast<const v4i*>(pb + w);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                uint32_t ga0, oa0, ga1, oa1, gb0, ob0, gb1, ob1;
                split_missing(static_cast<uint32_t>(wa[2 * q]), ga0, oa0);
                split_missing(static_cast<uint32_t>(wa[2 * q + 1]), ga1, oa1);
                split_missing(static_cast<uint32_t>(wb[2 * q]), gb0, ob0);
                split_missing(static_cast<uint32_t>(wb[2 * q + 1]), gb1, ob1);
                const v4i ga = fp4_chunk(ga0, ga1), oa = fp4_chunk(oa0, oa1);
                const v4i gb = fp4_chunk(gb0, gb1), ob = fp4_chunk(ob0, ob1);
                acc = mfma_fp4(ga, gb, acc);
                acc_go = mfma_fp4(ga, ob, acc_go);
                acc_og = mfma_fp4(oa, gb, acc_og);
                acc_oo = mfma_fp4(oa, ob, acc_oo);
            }
        }
    }

    // epilogue.  C/D map of the 32 x 32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int pj = c0 + sub;                                    // this lane's column position
    const int64_t nn = n_ref;
    const int64_t Sj = eb[0], Dj = nn * eb[1] - Sj * Sj;
    const int cj = gram_col(static_cast<double>(eb[0]));
    double muj, cssj;
    clump::moments(n_ref, eb, muj, cssj);
    const double pad_k = static_cast<double>(kpad - n_ref);
    int32_t chrj = 0;
    int64_t bpj = 0;
    if (kMask && pj < n) {
        chrj = chr[pj];
        bpj = bp[pj];
    }
    uint64_t rowbits[16];                   // mask mode: the ballots (two row masks each)
    uint32_t colbits = 0;                   // ... and this lane's rows of its column
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int pi = r0 + i;
        const v4i ea = tab[clump::row_of(pos, pi, n, zrow)];
        double r2;
        if (!missing) {
            const int64_t Si = ea[0];
            const int64_t G = gram_exact(acc[r], gram_row(static_cast<double>(ea[0]), kpad), cj);
            const int64_t N = nn * G - Si * Sj, Di = nn * ea[1] - Si * Si;
            const double dn = static_cast<double>(N);
            r2 = dn * dn / (static_cast<double>(Di) * static_cast<double>(Dj));
        } else {
            double mui, cssi;
            clump::moments(n_ref, ea, mui, cssi);
            const double c = ((static_cast<double>(acc[r]) - muj * static_cast<double>(acc_go[r])) -
                              mui * static_cast<double>(acc_og[r])) +
                             (mui * muj) * (static_cast<double>(acc_oo[r]) - pad_k);   // padding counts as observed
            // (css is exactly 0 for a row without variance, where rounding may leave c != 0; NaN
            // where a mean is 0 / 0)
            const double den = cssi * cssj;
            r2 = den > 0.0 ? c * c / den : __builtin_nan("");
        }
        if (kMask) {
            bool link = false;
            if (pi < pj && pj < n) {
                const int64_t d = bp[pi] - bpj;
                link = chr[pi] == chrj && (d < 0 ? -d : d) <= window && r2 >= thr;
            }
            rowbits[r] = __ballot(link);
            colbits |= link ? 1u << i : 0u;
        } else if (pi <= pj && pj < n) {
            r2_out[static_cast<int64_t>(pi) * n + pj] = r2;
            r2_out[static_cast<int64_t>(pj) * n + pi] = r2;
        }
    }
    if (kMask) {
        colbits |= static_cast<uint32_t>(__shfl_xor(static_cast<int>(colbits), 32, kWave));
        // lane l < 32 takes row mask l = register (l & 3) + 4 (l >> 3), lane half (l >> 2) & 1
        uint32_t word = colbits;            // lanes 32 .. 63: column mask l - 32
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i0 = (r & 3) + 8 * (r >> 2);
            if (lane == i0) word = static_cast<uint32_t>(rowbits[r]);
            if (lane == i0 + 4) word = static_cast<uint32_t>(rowbits[r] >> 32);
        }
        masks[static_cast<int64_t>(t) * kClumpMaskWords + lane] = word;
    }
}

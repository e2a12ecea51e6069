// assoc.hip -- the association scan over the resident panel image (dbslmm_assoc): per SNP row the
// Wald test of a linear model with covariates, the transpose of score.hip's product -- there
// (individuals x SNPs) beta, here (SNPs x individuals) [covariates | phenotypes].
//
//   dbslmm_assoc_counts   one wave per listed row: n1, n2, nm over the kept individuals, popcounts of
//                         the image dwords ANDed with the keep mask of assoc_layout.hpp.
//   dbslmm_assoc_tiles    the hot path.  Workgroup (x, y) = 4 waves: wave w the 16 listed rows of tile
//                         4 x + w, all on chunk y of the individuals; one launch per group of 16
//                         columns of V.  Per stage of 64 individuals the workgroup stages the 64 x 16
//                         block of V through LDS (double-buffered: the next stage's block is fetched
//                         before this stage's MFMAs and stored after them, one barrier per stage) and
//                         every lane loads the 16-B image chunk of its row.  A wave forms the 16 x 16
//                         tile of D with 16 v_mfma_f64_16x16x4_f64 per stage: lane l holds
//                         A[row l & 15][k = l >> 4] = the dosage of individual 4 s + (l >> 4) of step s,
//                         expanded from the dword's 2-bit field (score.hip's bit tricks; the dword is
//                         shifted by 2 (l >> 4) once, step s then reads bits 8 (s & 3)), and
//                         B[k][column l & 15] from LDS (64 consecutive doubles per step: no bank
//                         conflict).  Mm is a second MFMA with the missing mask as A; a step whose
//                         16 x 4 codes hold no missing call (one ballot per dword, one per step) skips
//                         it -- the skipped product is exactly +0 and the accumulator is never -0, so
//                         the bits do not depend on the tile's other rows.  Rows past the list read the
//                         image's zero-dosage row.  C/D layout: column l & 15, row (l >> 4) + 4 reg.
//                         Each (group, chunk, tile) writes its 16 x 16 partial tiles of D and Mm.
//   dbslmm_assoc_finish   one thread per listed row: adds the chunks' partials in index order per
//                         column (the raw products prod_d / prod_m), then assoc::finish_row
//                         (assoc_fit.hpp).
//
// Determinism: a chunk is chunk_indiv consecutive individuals (an argument of the call, a multiple of
// 64; 0 = kAssocChunkIndiv, never derived from the machine).  Inside a chunk an element of D is one
// chain of MFMAs over the steps in individual order; the chunks are added in index order.  No
// floating-point atomics.  A column's chain does not depend on its group, a row's not on its tile.
#include "assoc_fit.hpp"
#include "assoc_layout.hpp"

static_assert(assoc::kOk == DBSLMM_ASSOC_OK && assoc::kNoCall == DBSLMM_ASSOC_NO_CALL &&
              assoc::kMonomorphic == DBSLMM_ASSOC_MONOMORPHIC && assoc::kCollinear == DBSLMM_ASSOC_COLLINEAR,
              "assoc_fit.hpp's status codes are the header's");

namespace assoc {
constexpr int kTileWaves = 4;                                    // tiles (waves) per workgroup
constexpr int kTileWords = kAssocRows * kAssocCols;              // doubles of one partial tile
constexpr int kStageWords = kAssocStage * kAssocCols;            // doubles of one LDS stage of V
static_assert(kStageWords == 4 * kTileWaves * kWave, "four doubles of a stage per thread");
typedef double v2d_t __attribute__((ext_vector_type(2)));
typedef double acc4_t __attribute__((ext_vector_type(4)));   // the f64 MFMA's C/D registers of a lane
}  // namespace assoc

// rows: the image row of each listed row.  mask: one dword per image dword.  counts: {n1, n2, nm, 0}.
extern "C" __global__ __launch_bounds__(256) void dbslmm_assoc_counts(
    const uint8_t* __restrict__ img, int64_t pitch, const int32_t* __restrict__ rows, int32_t n_rows,
    const uint32_t* __restrict__ mask, v4i* __restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int j = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (j >= n_rows) return;
    const uint32_t* row = reinterpret_cast<const uint32_t*>(img + static_cast<int64_t>(rows[j]) * pitch);
    const int nw = static_cast<int>(pitch / 4);
    int n1 = 0, n2 = 0, nm = 0;
    for (int w = lane; w < nw; w += kWave) {
        const uint32_t word = row[w], keep = mask[w] & 0x55555555u;
        const uint32_t lo = word & 0x55555555u, hi = (word >> 1) & 0x55555555u;
        nm += __builtin_popcount(lo & ~hi & keep);        // 01
        n2 += __builtin_popcount(~lo & ~hi & keep);       // 00
        n1 += __builtin_popcount(~lo & hi & keep);        // 10
    }
    n1 = wave_sum_i32(n1);
    n2 = wave_sum_i32(n2);
    nm = wave_sum_i32(nm);
    if (lane == 0) counts[j] = v4i{n1, n2, nm, 0};
}

// rows16: n_tiles x 16 image rows (the zero-dosage row past the list).  V: this group's
// [n_pad][16] block.  stages_per_chunk = chunk_indiv / 64, n_stages = n_pad / 64.  part_d / part_m:
// this group's [n_chunks][n_tiles][16][16] partial tiles.
__global__ __launch_bounds__(256) void dbslmm_assoc_tiles(
    const uint8_t* __restrict__ img, int64_t pitch, const int32_t* __restrict__ rows16, int32_t n_tiles,
    const double* __restrict__ V, int32_t n_stages, int32_t stages_per_chunk, double* __restrict__ part_d,
    double* __restrict__ part_m) {
    using namespace assoc;
    __shared__ __attribute__((aligned(16))) double lds[2][kStageWords];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int r = lane & 15, kq = lane >> 4;
    const int32_t tile = static_cast<int32_t>(blockIdx.x) * kTileWaves + wave;
    const bool live = tile < n_tiles;                      // (a dead wave still stages V and meets the barriers)
    const int32_t st0 = static_cast<int32_t>(blockIdx.y) * stages_per_chunk;
    const int32_t st1 = min(n_stages, st0 + stages_per_chunk);
    const uint8_t* row = img + static_cast<int64_t>(live ? rows16[static_cast<int64_t>(tile) * kAssocRows + r] : 0) * pitch;
    const double* vsrc = V + 4 * tid;
    acc4_t acc_d = {0.0, 0.0, 0.0, 0.0}, acc_m = {0.0, 0.0, 0.0, 0.0};
    auto vload = [&](int32_t st, v2d_t& lo, v2d_t& hi) {
        const double* p = vsrc + static_cast<int64_t>(st) * kStageWords;
        lo = *reinterpret_cast<const v2d_t*>(p);
        hi = *reinterpret_cast<const v2d_t*>(p + 2);
    };
    auto vstore = [&](int buf, const v2d_t& lo, const v2d_t& hi) {
        *reinterpret_cast<v2d_t*>(&lds[buf][4 * tid]) = lo;
        *reinterpret_cast<v2d_t*>(&lds[buf][4 * tid + 2]) = hi;
    };
    auto aload = [&](int32_t st) -> v4i {
        return live ? *reinterpret_cast<const v4i*>(row + 16 * static_cast<int64_t>(st)) : v4i{-1, -1, -1, -1};
    };
    if (st0 < st1) {
        v2d_t vlo, vhi;
        vload(st0, vlo, vhi);
        vstore(0, vlo, vhi);
        v4i words = aload(st0);
        __syncthreads();
        for (int32_t st = st0; st < st1; ++st) {
            const int buf = (st - st0) & 1;
            const bool more = st + 1 < st1;
            v4i next = words;
            if (more) {
                vload(st + 1, vlo, vhi);
                next = aload(st + 1);
            }
            const double* B = &lds[buf][kq * kAssocCols + r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t word = static_cast<uint32_t>(words[j]);
                const uint32_t nlo = ~word & 0x55555555u;             // low bit clear: codes 00, 10
                const uint32_t hi = (word >> 1) & 0x55555555u;        // high bit set: codes 10, 11
                const uint32_t field = (((nlo & ~hi) << 1) | (nlo & hi)) >> (2 * kq);   // the dosage, 2 bits
                const uint32_t miss = (word & 0x55555555u & ~hi) >> (2 * kq);           // code 01
                const bool any = __ballot(miss != 0u) != 0ull;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double b = B[(16 * j + 4 * u) * kAssocCols];
                    const double g = static_cast<double>((field >> (8 * u)) & 3u);
                    acc_d = __builtin_amdgcn_mfma_f64_16x16x4f64(g, b, acc_d, 0, 0, 0);
                    if (any) {
                        const uint32_t mb = (miss >> (8 * u)) & 1u;
                        if (__ballot(mb != 0u) != 0ull)
                            acc_m = __builtin_amdgcn_mfma_f64_16x16x4f64(static_cast<double>(mb), b, acc_m, 0, 0, 0);
                    }
                }
            }
            if (more) vstore(buf ^ 1, vlo, vhi);
            words = next;
            __syncthreads();
        }
    }
    if (!live) return;
    const int64_t o = (static_cast<int64_t>(blockIdx.y) * n_tiles + tile) * kTileWords + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        part_d[o + (kq + 4 * i) * kAssocCols] = acc_d[i];
        part_m[o + (kq + 4 * i) * kAssocCols] = acc_m[i];
    }
}

// part_d / part_m: [n_groups][n_chunks][n_tiles][16][16].  prod_d / prod_m: [n_rows][n_cols].  yy: P.
// Outputs: n_obs, af, status [n_rows]; beta / se / tstat / p [P][n_rows].
extern "C" __global__ __launch_bounds__(256) void dbslmm_assoc_finish(
    const double* __restrict__ part_d, const double* __restrict__ part_m, int32_t n_groups, int32_t n_chunks,
    int32_t n_tiles, int32_t n_rows, int32_t c1, int32_t P, int64_t n, const v4i* __restrict__ counts,
    const double* __restrict__ yy, double* __restrict__ prod_d, double* __restrict__ prod_m,
    int32_t* __restrict__ n_mis, int32_t* __restrict__ n_obs, double* __restrict__ af, double* __restrict__ beta,
    double* __restrict__ se, double* __restrict__ tstat, double* __restrict__ p, int32_t* __restrict__ status) {
    using namespace assoc;
    const int32_t j = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
    if (j >= n_rows) return;
    const int32_t n_cols = c1 + P;
    const int64_t in_tile = static_cast<int64_t>(j / kAssocRows) * kTileWords + (j % kAssocRows) * kAssocCols;
    double* pd = prod_d + static_cast<int64_t>(j) * n_cols;
    double* pm = prod_m + static_cast<int64_t>(j) * n_cols;
    for (int32_t k = 0; k < n_cols; ++k) {
        const int64_t g = k / kAssocCols;
        double d = 0.0, m = 0.0;
        for (int32_t ch = 0; ch < n_chunks; ++ch) {
            const int64_t o = (g * n_chunks + ch) * n_tiles * kTileWords + in_tile + k % kAssocCols;
            d += part_d[o];
            m += part_m[o];
        }
        pd[k] = d;
        pm[k] = m;
    }
    const v4i cn = counts[j];
    n_mis[j] = cn[2];
    status[j] = finish_row(n, c1, P, cn[0], cn[1], cn[2], pd, pm, yy, n_obs + j, af + j, beta + j, se + j,
                           tstat + j, p + j, n_rows);
}

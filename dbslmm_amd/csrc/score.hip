// score.hip -- polygenic scores of a target panel from the solved betas (included by plan.hip).
//
// Reference: the manual ends each fit with `plink --score <eff>.txt 1 2 4 sum` on a test panel
// (Rmd/Manual.Rmd:176-188) and the h2f tuning scores one effect file per factor
// (software/DBSLMM.R:204-219, software/TUNE.R).  Here every h2f copy is scored in one streaming
// pass over the 2-bit test panel, from the betas resident on the device.
//
// Per SNP j (plan slot s) with imputed dosage g (observed call, else the mean mu_j over the
// selected individuals: readSNPIm, scr/dtpr.cpp:358-360) every mode is
//   score[c][t] = K_c + sum_s a[c][s] * g_ts,      K_c = sum_s k[c][s]
// with per-slot coefficients (dbslmm_score_coef):
//   COUNTS  a = beta w,        k = 0;               flipped: a = -beta w,       k = 2 beta w
//   STD     a = beta w rsd,    k = -a mu;           flipped: a = -beta w rsd,   k = -a mu
// (a flip replaces g by 2 - g and mu by 2 - mu).  A missing call adds am = a mu instead of a * g.
// Dropped SNPs (block NOT_PD / MONOMORPHIC for that copy, beta w not finite, no observed call,
// STD: sd = 0 or fewer than two individuals) have a = am = k = 0 and are counted per copy.
//
// Determinism: chunks are runs of chunk_slots consecutive slots (a constant of the call, never of
// the machine); a chunk's partial is one sequential fp64 FMA chain per individual and copy; the
// chunks are added in index order (dbslmm_score_reduce) after K_c, itself a fixed-shape reduction
// (dbslmm_score_const: per chunk, then over the chunks).  No floating-point atomics anywhere.

namespace score {
constexpr int kChunkSlots = 512;    // slots per chunk (dbslmm_score_args.chunk_slots = 0): 500k SNPs x 10k
                                    // individuals, 3 copies: 1.30 ms at 512, 1.44 at 1024, 1.69 at 2048
constexpr int kMaxPass = 4;         // copies per pass of dbslmm_score_partial
constexpr int kDepth = 4;           // rows whose loads are in flight ahead of the one in use
}  // namespace score

// One thread per (slot, copy).  slot_out: >= 0 small SNP, -1 - l large SNP, INT32_MIN padding;
// slot_block: the slot's non-empty block, blk_id its original id (status index); beta_s / beta_l /
// status: copy c at c * n_s / c * n_l / c * nbk.  mu / rsd: the slot's mean over the observed
// selected calls (NaN: none observed) and 1 / sd (row_moments).  Writes a, am, k at
// [c * stride + s] for every s < stride (zeros from n_slots on: the tail of the last chunk) and
// adds the dropped SNPs of copy c to dropped[c] (integer atomics).
extern "C" __global__ __launch_bounds__(256) void dbslmm_score_coef(
    const int32_t* __restrict__ slot_out, const int32_t* __restrict__ slot_block,
    const int32_t* __restrict__ blk_id, const int32_t* __restrict__ status, int64_t nbk,
    const double* __restrict__ beta_s, const double* __restrict__ beta_l, int64_t n_s, int64_t n_l,
    const double* __restrict__ w_s, const double* __restrict__ w_l,
    const uint8_t* __restrict__ flip_s, const uint8_t* __restrict__ flip_l,
    const double* __restrict__ mu, const double* __restrict__ rsd, int32_t n_slots, int32_t stride,
    int32_t n_copies, int32_t mode, int32_t n_test, double* __restrict__ a_out, double* __restrict__ am_out,
    double* __restrict__ k_out, int32_t* __restrict__ dropped) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (s >= stride || c >= n_copies) return;
    const int64_t o = static_cast<int64_t>(c) * stride + s;
    const int32_t so = s < n_slots ? slot_out[s] : INT32_MIN;
    double a = 0.0, am = 0.0, k = 0.0;
    if (so != INT32_MIN) {
        const bool small = so >= 0;
        const int64_t j = small ? so : -1 - static_cast<int64_t>(so);
        const double beta = small ? beta_s[c * n_s + j] : beta_l[c * n_l + j];
        const double* w = small ? w_s : w_l;
        const uint8_t* fl = small ? flip_s : flip_l;
        const double bw = w ? beta * w[j] : beta;
        const bool flip = fl && fl[j] != 0;
        const int32_t st = status[c * nbk + blk_id[slot_block[s]]];
        const double m = mu[s], r = rsd[s];
        bool drop = st == DBSLMM_BLOCK_NOT_PD || st == DBSLMM_BLOCK_MONOMORPHIC || !isfinite(bw) || isnan(m);
        if (mode == DBSLMM_SCORE_STD) drop = drop || n_test < 2 || !isfinite(r) || !(r > 0.0);
        if (drop) {
            atomicAdd(dropped + c, 1);
        } else {
            const double a0 = mode == DBSLMM_SCORE_STD ? bw * r : bw;
            a = flip ? -a0 : a0;
            am = a * m;
            if (mode == DBSLMM_SCORE_STD) k = -am;
            else if (flip) k = 2.0 * a0;
        }
    }
    a_out[o] = a;
    am_out[o] = am;
    k_out[o] = k;
}

// K_c = sum_s k[c][s] in two launches of one fixed-shape reduction (a single workgroup walking all
// slots is latency-bound: 1.4 ms at 500k SNPs): workgroup (x, y) sums in[y * in_stride + x * seg ..
// min(n, (x + 1) seg)) -- thread i its elements i, i + 256, ... in order, then a binary tree over
// the 256 partial sums -- into out[y * gridDim.x + x].  First the chunks (seg = chunk_slots), then
// the chunk sums of each copy (one segment).
extern "C" __global__ __launch_bounds__(256) void dbslmm_score_const(
    const double* __restrict__ in, int32_t n, int32_t seg, int64_t in_stride, double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t lo = static_cast<int64_t>(blockIdx.x) * seg;
    const int64_t hi = min(static_cast<int64_t>(n), lo + seg);
    const double* v = in + static_cast<int64_t>(blockIdx.y) * in_stride;
    double t = 0.0;
    for (int64_t s = lo + threadIdx.x; s < hi; s += 256) t += v[s];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

namespace score {
// One image dword (16 PLINK codes) of a slot into the lane's accumulators: 00 -> 2, 10 -> 1,
// 11 -> 0, 01 -> missing (dosage field 0, then am once per missing code).  a / am wave-uniform.
template <int NC>
__device__ __forceinline__ void accumulate(uint32_t word, const double (&a)[NC], const double (&am)[NC],
                                           double (&acc)[NC][16]) {
    const uint32_t nlo = ~word & 0x55555555u;            // low bit clear: codes 00, 10
    const uint32_t hi = (word >> 1) & 0x55555555u;       // high bit set: codes 10, 11
    const uint32_t field = ((nlo & ~hi) << 1) | (nlo & hi);   // the dosage as a 2-bit field
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double g = static_cast<double>((field >> (2 * i)) & 3u);
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c][i] = __builtin_fma(a[c], g, acc[c][i]);
    }
    const uint32_t miss = word & 0x55555555u & ~hi;      // code 01
    if (miss != 0u) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if ((miss >> (2 * i)) & 1u) {
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c][i] += am[c];
            }
        }
    }
}
}  // namespace score

// The hot path.  Workgroup (x, y): dword columns [256 x, 256 x + 256) of chunk y = slots
// [y chunk_slots, (y + 1) chunk_slots); a lane owns one dword column (16 individuals) of every row.
// srow[s] = the slot's row in img (pitch bytes per row, 64-B aligned, pad codes 11) for every
// s < n_chunks chunk_slots + kDepth -- padding slots and the tail name any valid row and have
// a = am = 0 -- so the loop is straight-line code: chunk_slots is a multiple of kDepth, the slot
// loop is unrolled kDepth times over a ring of words with a static index, and the load of slot
// s + kDepth is issued before slot s's word is used (each use waits for its own load only).
// a / am: copy c of this pass at c * stride.  part: the chunk's partial sums
// [chunk][copy of the pass][n_pad], n_pad = 16 n_words.
template <int NC>
__global__ __launch_bounds__(256) void dbslmm_score_partial(
    const uint8_t* __restrict__ img, int64_t pitch, const int32_t* __restrict__ srow,
    const double* __restrict__ a, const double* __restrict__ am, int32_t stride, int32_t chunk_slots,
    int32_t n_words, double* __restrict__ part) {
    using namespace score;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    const int32_t s0 = static_cast<int32_t>(blockIdx.y) * chunk_slots;
    const uint8_t* col = img + 4 * static_cast<int64_t>(w);
    double acc[NC][16];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.0;
    auto fetch = [&](int32_t s) -> uint32_t {
        return *reinterpret_cast<const uint32_t*>(col + static_cast<int64_t>(srow[s]) * pitch);
    };
    uint32_t ring[kDepth];
#pragma unroll
    for (int u = 0; u < kDepth; ++u) ring[u] = fetch(s0 + u);
#pragma clang loop unroll(disable)
    for (int32_t sg = s0; sg < s0 + chunk_slots; sg += kDepth) {
#pragma unroll
        for (int u = 0; u < kDepth; ++u) {
            const int32_t s = sg + u;
            const uint32_t word = ring[u];
            ring[u] = fetch(s + kDepth);
            double ac[NC], amc[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                ac[c] = a[static_cast<int64_t>(c) * stride + s];
                amc[c] = am[static_cast<int64_t>(c) * stride + s];
            }
            accumulate<NC>(word, ac, amc, acc);
        }
    }
    const int64_t n_pad = 16 * static_cast<int64_t>(n_words);
    double* out = part + static_cast<int64_t>(blockIdx.y) * NC * n_pad + 16 * static_cast<int64_t>(w);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) out[c * n_pad + i] = acc[c][i];
}

// scores[c][t] = K_c + the chunks' partials in index order.  One thread per (individual, copy of the
// pass); nc copies in this pass, kc / scores already offset to its first copy.
extern "C" __global__ __launch_bounds__(256) void dbslmm_score_reduce(
    const double* __restrict__ part, int32_t n_chunks, int32_t nc, int64_t n_pad,
    const double* __restrict__ kc, int32_t n_test, double* __restrict__ scores) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (t >= n_test || c >= nc) return;
    double v = kc[c];
#pragma unroll 8
    for (int ch = 0; ch < n_chunks; ++ch) v += part[(static_cast<int64_t>(ch) * nc + c) * n_pad + t];
    scores[static_cast<int64_t>(c) * n_test + t] = v;
}

// lm_head with a log-softmax / argmax / gather epilogue: scores given target tokens without the [M][N] logits ever leaving the chip.
//   logit[m][n] = sum_k X[m][k] * W[n][k]   (bf16 operands in the packed fragment-tile format, fp32 accumulate on the matrix cores)
//   lse[m]    = log sum_{n < N} exp(logit[m][n])
//   tok_lp[m] = logit[m][targets[m]] - lse[m]        (targets[m] < 0: 0.0, stock's ignore_index; >= N: 0.0 and counted in the error word)
//   arg_id[m] = argmax_n logit[m][n] (ties: the lowest index, as greedy_select),   arg_lp[m] = logit[m][arg_id[m]] - lse[m]
//
// LAYOUT (the choice the 32x32 MFMA output forces): the operand roles are SWAPPED - A = W fragment, B = X fragment, as the packed
// epilogues of k_gemm.hip do - so that a lane holds ONE token (column lane % 32 of the accumulator) and sixteen vocabulary columns in its
// registers.  The reduction over the vocabulary then runs down a lane's own registers (no DPP / LDS traffic per tile); only the two
// half-waves (vocabulary rows 4 * half + ... of a tile) and the two column waves of a workgroup meet, once per slab, through LDS.
// The other form (lane = vocabulary column, cross-lane tree per row and tile) costs five exchange steps per row group and tile.
//
// PARTITION (compile-time): the vocabulary is cut into slabs of SC_SLAB = 1024 columns; a workgroup (4 waves as 2 x 2, 128 tokens x
// 128 columns per step, the main loop of gemm_big_kernel) walks the 8 column tiles of ONE slab for its 128 tokens with the running
// (max, sum of exp(x - max), lowest index of the max, target logit) of every token in registers, and leaves one 16-byte partial per
// (slab, token) in the caller's scratch: ceil(N / 1024) * 16 bytes per token instead of 4 * N.
// MERGE ORDER (fixed): inside a lane, column tiles ascending; inside a workgroup, the four (column wave, half-wave) contributors
// 0 .. 3 of a token; across slabs (score_merge_kernel), slab 0, 1, 2, ...  No float atomics.  A token's four results depend on its own
// X row and W only: every accumulator element is the same k-ascending chain of MFMAs wherever the token sits in the call.
// Pad columns (n >= N: zero rows of W_pk, logit 0.0) are masked before anything looks at them; pad rows (m >= M) are never written.
#include "mg_kernels.h"
#include "mg_dispatch.h"

namespace mg {

constexpr int SC_M = 128, SC_N = 128, SC_K = 64;
constexpr int SC_STAGE_BYTES = (SC_M + SC_N) / 32 * (SC_K / 16) * TILE_BYTES;   // 32 KiB
constexpr int SC_SLAB = 1024;                                                    // vocabulary columns per slab
constexpr int SC_TILES = SC_SLAB / SC_N;
constexpr int SC_HEADER = 256;                                                   // scratch: [0] error word, then the partials
constexpr float SC_NEG = -1.0e30f;                                               // "no column yet": finite, and so is SC_NEG * log2(e) (no Inf - Inf)
constexpr float SC_LOG2E = 1.44269504088896340736f;

MG_HD int score_slabs(int N) { return (N + SC_SLAB - 1) / SC_SLAB; }
size_t score_scratch_bytes(int M, int N) { return (size_t)SC_HEADER + (size_t)score_slabs(N) * (size_t)((M + 31) / 32 * 32) * sizeof(float4); }

struct ScoreState { float bv, sum, tv; int bi; };      // running max, sum of exp(x - bv), target logit, lowest index of the max

// (b, s) merged into (a, s_a) in that order: a's max wins ties, so the caller merges in ascending column order
MG_DEV void score_merge(float& bv, float& sum, int& bi, float obv, float osum, int obi) {
    const float nm = fmaxf(bv, obv);
    sum = sum * fast_exp2((bv - nm) * SC_LOG2E) + osum * fast_exp2((obv - nm) * SC_LOG2E);
    if (obv > bv || (obv == bv && obi < bi)) bi = obi;
    bv = nm;
}

template <int TGT>
__global__ __launch_bounds__(256) void score_slab_kernel(ScoreArgs a, float4* part, int Mp) {
    MG_DYN_SMEM(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5;
    const int nbm = (a.M + SC_M - 1) / SC_M;
    const int slab = blockIdx.x / nbm, bm = blockIdx.x - slab * nbm;      // consecutive workgroups share a W slab (L2)
    const int mt32 = (a.M + 31) >> 5, nt32 = (a.N + 31) >> 5;
    const int nks = a.K / SC_K;
    const int n_slab0 = slab * SC_SLAB;
    int ntiles = (a.N - n_slab0 + SC_N - 1) / SC_N;                        // column tiles of this slab with at least one real column
    ntiles = ntiles < SC_TILES ? ntiles : SC_TILES;
    const int nsteps = ntiles * nks;

    // loader: wave w stages fragments f = 8w .. 8w+7 of a stage; f < 16: X row-tile f/4, k-tile f%4 (waves 0, 1); else W (waves 2, 3)
    const bool isW = w >= 2;
    auto stage = [&](int buf, int ct, int ks) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ff = (w * 8 + i) & 15, rt = ff >> 2, kt = ff & 3;
            int trow = isW ? ((n_slab0 + ct * SC_N) >> 5) + rt : bm * 4 + rt;
            const int tmax = isW ? nt32 - 1 : mt32 - 1;
            trow = trow < tmax ? trow : tmax;   // clamp: tiles past the edge re-read the last tile, their results are masked / not written
            const char* src = (const char*)((isW ? a.W : a.X) + pk_tile_off(trow, ks * 4 + kt, a.K)) + lane * 16;
            glds16(src, smem + buf * SC_STAGE_BYTES + (w * 8 + i) * TILE_BYTES);
        }
    };

    const int wr = w >> 1, wc = w & 1;
    int tg[2];                                        // the lane's tokens' targets (-1: none in range)
    ScoreState st[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = bm * SC_M + wr * 64 + 32 * i + (lane & 31);
        tg[i] = -1;
        if (TGT && m < a.M) {
            const int64_t t = a.targets[m];
            if (t >= 0 && t < (int64_t)a.N) tg[i] = (int)t;
        }
        st[i].bv = SC_NEG; st[i].sum = 0.f; st[i].tv = 0.f; st[i].bi = 0x7fffffff;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = acc_zero();

    stage(0, 0, 0);
    __syncthreads();
    int ct = 0, ks = 0;
    for (int s = 0; s < nsteps; ++s) {
        const int cur = s & 1;
        const bool last_k = ks + 1 == nks;
        if (s + 1 < nsteps) stage(cur ^ 1, last_k ? ct + 1 : ct, last_k ? 0 : ks + 1);
        const char* xb = smem + cur * SC_STAGE_BYTES + lane * 16;
        const char* wb = xb + 16 * TILE_BYTES;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            uint4 xf[2], wf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                xf[i] = ld16(xb + ((wr * 2 + i) * 4 + kt) * TILE_BYTES);
                wf[i] = ld16(wb + ((wc * 2 + i) * 4 + kt) * TILE_BYTES);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(wf[j], xf[i], acc[i][j]);      // lane: token lane % 32, 16 columns
        }
        if (last_k) {
            // the wave's 64 columns of this tile: n0w + 32 j + acc_row(r, half); lim = how many of them are real (wave-uniform)
            const int n0w = n_slab0 + ct * SC_N + wc * 64;
            const int lim = a.N - n0w;
            if (lim > 0) {
                const bool full = lim >= 64;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float v[32];
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            v[16 * j + r] = (full || 32 * j + acc_row(r, half) < lim) ? acc[i][j][r] : SC_NEG;
                    float tmx = v[0];
#pragma unroll
                    for (int q = 1; q < 32; ++q) tmx = fmaxf(tmx, v[q]);
                    const bool up = tmx > st[i].bv;          // strictly: an equal maximum of a later tile keeps the earlier (lower) index
                    if (wave_any(up)) {
                        int cand = 0x7fffffff;
#pragma unroll
                        for (int q = 31; q >= 0; --q)
                            if (v[q] == tmx) cand = n0w + 32 * (q >> 4) + acc_row(q & 15, half);      // descending: the lowest index stays
                        if (up) st[i].bi = cand;
                    }
                    if (TGT) {
                        const int rel = tg[i] - n0w;
                        if (wave_any(rel >= 0 && rel < 64)) {
#pragma unroll
                            for (int q = 0; q < 32; ++q)
                                if (rel == 32 * (q >> 4) + acc_row(q & 15, half)) st[i].tv = v[q];
                        }
                    }
                    const float nm = fmaxf(st[i].bv, tmx);
                    const float nms = -nm * SC_LOG2E;
                    float e = 0.f;
                    if (nm > SC_NEG) {                       // (a lane whose 16 + 16 columns are all pad keeps sum 0)
#pragma unroll
                        for (int q = 0; q < 32; ++q) e += fast_exp2(v[q] * SC_LOG2E + nms);      // masked: exp2(-huge) = 0
                    }
                    st[i].sum = st[i].sum * fast_exp2(st[i].bv * SC_LOG2E + nms) + e;
                    st[i].bv = nm;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = acc_zero();
        }
        __syncthreads();
        if (last_k) { ks = 0; ++ct; } else ++ks;
    }

    // the four contributors of a token - (column wave wc, half-wave) = 0 .. 3 - meet in LDS (the stages are idle: barrier above)
    float4* red = (float4*)smem;                      // [128 tokens][4]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int tl = wr * 64 + 32 * i + (lane & 31);
        red[tl * 4 + wc * 2 + half] = make_float4(st[i].bv, st[i].sum, __int_as_float(st[i].bi), st[i].tv);
    }
    __syncthreads();
    if (tid < SC_M) {
        const int m = bm * SC_M + tid;
        if (m < a.M) {
            float bv = SC_NEG, sum = 0.f, tv = 0.f;
            int bi = 0x7fffffff;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 p = red[tid * 4 + c];
                score_merge(bv, sum, bi, p.x, p.y, __float_as_int(p.z));
            }
            if (TGT) {
                const int64_t t = a.targets[m];
                if (t >= (int64_t)n_slab0 && t < (int64_t)n_slab0 + SC_SLAB && t < (int64_t)a.N) {
                    const int rel = (int)t - n_slab0;
                    tv = red[tid * 4 + ((rel >> 6) & 1) * 2 + ((rel >> 2) & 1)].w;
                }
            }
            part[(size_t)slab * Mp + m] = make_float4(bv, sum, __int_as_float(bi), tv);
        }
    }
}

// one thread per token: the slabs' partials in ascending order -> the four results
__global__ __launch_bounds__(256) void score_merge_kernel(ScoreArgs a, const float4* part, int Mp, int nslab, int* err) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.M) return;
    float bv = SC_NEG, sum = 0.f;
    int bi = 0x7fffffff;
    for (int s = 0; s < nslab; ++s) {
        const float4 p = part[(size_t)s * Mp + m];
        score_merge(bv, sum, bi, p.x, p.y, __float_as_int(p.z));
    }
    const float lse = bv + logf(sum);
    if (a.lse) a.lse[m] = lse;
    if (a.arg_id) a.arg_id[m] = (int64_t)bi;
    if (a.arg_lp) a.arg_lp[m] = bv - lse;
    if (a.targets) {
        const int64_t t = a.targets[m];
        float lp = 0.f;
        if (t >= (int64_t)a.N) atomicAdd(err, 1);
        else if (t >= 0) lp = part[(size_t)((int)t / SC_SLAB) * Mp + m].w - lse;
        if (a.tok_lp) a.tok_lp[m] = lp;
    }
}

void score_lm_head(const ScoreArgs& a, mgStream_t stream) {
    const int Mp = (a.M + 31) / 32 * 32, nslab = score_slabs(a.N);
    int* err = (int*)a.scratch;
    float4* part = (float4*)((char*)a.scratch + SC_HEADER);
    mg_memset_async(err, 0, SC_HEADER, stream);
    // M = 16384, N = 33201: 128 x 33 = 4224 workgroups of 64 KiB LDS (two per CU); M = 1: one per slab
    const dim3 grid(((a.M + SC_M - 1) / SC_M) * nslab), block(256);
    const size_t sh = 2 * SC_STAGE_BYTES;                // 64 KiB: within the default dynamic-LDS limit (no MG_SET_MAX_SMEM_ONCE needed)
    dispatch_int<0, 1>(a.targets ? 1 : 0, [&](auto T) {
        MG_LAUNCH((score_slab_kernel<decltype(T)::value>), grid, block, sh, stream, a, part, Mp);
    });
    MG_LAUNCH(score_merge_kernel, dim3((a.M + 255) / 256), dim3(256), 0, stream, a, (const float4*)part, Mp, nslab, err);
}

}  // namespace mg

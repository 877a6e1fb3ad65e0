// Cross-attention attribution maps: the fp32 softmax of the teacher-forced cross-attention, summed over heads in registers and over
// layers in one scratch buffer, without the [B][H][T][S] probabilities ever being stored.
//   p[h][q][k] = exp(s - m) / l,   s = Q[h][q] . K[h][k] (no scale, no bias: stock UDOP cross-attention), masked keys excluded,
//   m = max over the attended keys, l = sum over them of exp(s - m)
//   acc[q][k]  = sum_h p[h][q][k]  (h ascending);  scratch = acc (first selected layer) or scratch + acc (later layers), times `scale`
//   in the last selected layer's launch (1 / (layers * H)).
// Operands: the packed bf16 Q / K of the cross-attention launch itself (HF_PK_ROWS), read straight from memory as MFMA fragments - a
// 32 x 32 score tile is four v_mfma_f32_32x32x16_bf16 over the head dimension, A = K fragment, B = Q fragment as in attention_kernel, so a
// lane holds ONE query (column lane % 32) and sixteen keys (acc_row(r, half)) of a tile.  No LDS re-layout.
//
// PARTITION: a workgroup (8 waves) owns one (image, 32-query tile) and ALL keys; wave w owns the NT consecutive 32-key tiles
// w * NT .. w * NT + NT - 1 and keeps their 16 * NT head sums per lane in registers (NT <= 6: 1536 keys, 96 accumulators).  Every scratch
// element has exactly one owning lane, layers follow each other on one stream: plain loads and stores, no float atomics.
// PER HEAD: pass one computes, per key tile, (m_t, l_t) = (max, sum of exp(s - m_t)) over the tile's attended keys and leaves them in LDS
// [tile][query]; after ONE barrier every lane merges the tiles of its query in ASCENDING TILE ORDER - m = max_t m_t,
// l = sum_t l_t * exp(m_t - m) - and pass two recomputes its tiles' scores and adds exp(s - m) * (1 / l) to the accumulators.  (The LDS
// slots alternate between two buffers by head parity, which is what makes one barrier per head enough.)
// ORDER: l_t is the lane's sixteen keys in register order, then half-wave 0 + half-wave 1; l is the tiles in ascending order.  Neither
// depends on which wave owns a tile, so a row's bits depend on its own Q row, the image's K and mask only: not on B, Sq, NT or Sk_cap.
// A fully masked tile has m_t = XA_NEG and contributes l_t * exp2(-huge) = +0.0.
// The key-mask test happens on the score before the maximum (as ATT_CROSS); a masked key adds exactly 0.0.
//
// SCRATCH LAYOUT (accumulator order, so that a wave's loads and stores are 256 contiguous bytes per register):
//   [image][query tile][key tile][register r (16)][lane (64)] fp32,  key tiles = ceil(Sk / 32), query tiles = ceil(Sq / 32).
// xattn_map_gather turns it into the caller's [B][T][M_e1 + L + P] rows: e1 columns first (the M_pad - M_e1 pad slots dropped), then the
// encoder positions in the documented [text | patches] order through the per-image padding map; rows with qmask == 0 are 0.0.
#include "mg_kernels.h"
#include "mg_dispatch.h"

namespace mg {

constexpr int XA_WAVES = 8;
constexpr int XA_MAX_NT = 6;
constexpr float XA_NEG = -1.0e30f;                      // finite, and so is XA_NEG * log2(e)
constexpr float XA_LOG2E = 1.44269504088896340736f;

MG_HD int xa_tiles(int n) { return (n + 31) >> 5; }
size_t xattn_map_scratch_bytes(int B, int Sq, int Sk) { return (size_t)B * xa_tiles(Sq) * xa_tiles(Sk) * 1024 * sizeof(float); }
bool xattn_map_supported(int Sk) { return Sk >= 1 && xa_tiles(Sk) <= XA_WAVES * XA_MAX_NT; }

template <int NT>
__global__ __launch_bounds__(XA_WAVES * 64) void xattn_map_kernel(XattnMapArgs a) {
    MG_DYN_SMEM(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l32 = lane & 31;
    const int nqt = xa_tiles(a.Sq), nkt = xa_tiles(a.Sk);
    const int b = blockIdx.x / nqt, qt = blockIdx.x - b * nqt;
    float2* ml = (float2*)smem;                          // [2][nkt][32 queries] (m_t, l_t)

    // this lane's sixteen keys of each of its tiles: attended bits in register order (once per workgroup, every head reads them)
    uint32_t okb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int kt = w * NT + t;
        okb[t] = 0;
        if (kt < nkt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + acc_row(r, half);
                if (key < a.Sk && (!a.kmask || a.kmask[(size_t)b * a.Sk_cap + key] != 0)) okb[t] |= 1u << r;
            }
        }
    }

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = acc_zero();

    auto scores = [&](const uint16_t* Kb, const uint4 (&qf)[4], int kt) {
        f32x16 s = acc_zero();
        const char* kp = (const char*)(Kb + (size_t)kt * (4 * TILE_ELEMS)) + lane * 16;
#pragma unroll
        for (int dk = 0; dk < 4; ++dk) s = mfma32(ld16(kp + dk * TILE_BYTES), qf[dk], s);
        return s;
    };

    for (int h = 0; h < a.H; ++h) {
        const size_t bh = (size_t)b * a.H + h;
        const uint16_t* Qb = a.Q + (bh * (size_t)(a.Sq_cap >> 5) + (size_t)qt) * (4 * TILE_ELEMS);
        const uint16_t* Kb = a.K + bh * (size_t)(a.Sk_cap >> 5) * (4 * TILE_ELEMS);
        uint4 qf[4];
#pragma unroll
        for (int dk = 0; dk < 4; ++dk) qf[dk] = ld16((const char*)(Qb + dk * TILE_ELEMS) + lane * 16);
        float2* mlh = ml + (size_t)(h & 1) * nkt * 32;

        // pass one: (m_t, l_t) of this wave's tiles
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int kt = w * NT + t;
            if (kt < nkt) {
                const f32x16 s = scores(Kb, qf, kt);
                float v[16];
                float mt = XA_NEG;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    v[r] = ((okb[t] >> r) & 1u) ? s[r] : XA_NEG;
                    mt = fmaxf(mt, v[r]);
                }
                mt = fmaxf(mt, __shfl_xor(mt, 32));
                // (the difference first: XA_NEG - XA_NEG is exactly 0, whereas v * log2(e) - m * log2(e) contracted into one fused
                // multiply-add leaves the rounding error of 1.4e30 as the exponent)
                float lt = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) lt += fast_exp2((v[r] - mt) * XA_LOG2E);
                const float other = __shfl_xor(lt, 32);
                lt = half ? other + lt : lt + other;     // half-wave 0 first
                if (half == 0) mlh[kt * 32 + l32] = make_float2(mt, lt);
            }
        }
        __syncthreads();
        // merge: tiles ascending
        float m = XA_NEG;
        for (int kt = 0; kt < nkt; ++kt) m = fmaxf(m, mlh[kt * 32 + l32].x);
        float l = 0.f;
        for (int kt = 0; kt < nkt; ++kt) {
            const float2 p = mlh[kt * 32 + l32];
            l += p.y * fast_exp2((p.x - m) * XA_LOG2E);
        }
        const float inv = 1.0f / l;
        // pass two: the same scores again, normalised, into the head sum
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int kt = w * NT + t;
            if (kt < nkt) {
                const f32x16 s = scores(Kb, qf, kt);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    acc[t][r] += ((okb[t] >> r) & 1u) ? fast_exp2((s[r] - m) * XA_LOG2E) * inv : 0.f;
            }
        }
    }

    float* out = a.scratch + ((size_t)blockIdx.x * nkt) * 1024 + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int kt = w * NT + t;
        if (kt < nkt) {
            float* o = out + (size_t)kt * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[t][r];
                if (a.accumulate) v += o[r * 64];
                o[r * 64] = v * a.scale;
            }
        }
    }
}

int xattn_map(const XattnMapArgs& a, mgStream_t stream) {
    const int nkt = xa_tiles(a.Sk);
    if (!xattn_map_supported(a.Sk)) return -1;
    const int nt = (nkt + XA_WAVES - 1) / XA_WAVES;
    const dim3 grid(a.B * xa_tiles(a.Sq)), block(XA_WAVES * 64);
    const size_t sh = (size_t)2 * nkt * 32 * sizeof(float2);      // <= 24 KiB
    dispatch_int<1, 2, 3, 4, 5, 6>(nt, [&](auto N) {
        MG_LAUNCH((xattn_map_kernel<decltype(N)::value>), grid, block, sh, stream, a);
    });
    return 0;
}

// scratch (accumulator order) -> map [B][Sq][M_e1 + L + P]; one thread per output element, consecutive threads = consecutive columns
__global__ __launch_bounds__(256) void xattn_map_gather_kernel(XattnGatherArgs g) {
    const int No = g.M_e1 + g.L + g.P;
    const int nqt = xa_tiles(g.Sq), nkt = xa_tiles(g.Sk);
    const size_t n = (size_t)g.B * g.Sq * No;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / No;
        const int c = (int)(i - row * No), b = (int)(row / g.Sq), q = (int)(row - (size_t)b * g.Sq);
        float v = 0.f;
        if (!g.qmask || g.qmask[(size_t)b * g.qmask_ld + q] != 0) {
            int key;
            if (c < g.M_e1) key = c;
            else {
                const int s = c - g.M_e1, Lb = g.text_len ? g.text_len[b] : g.L;      // (enc_src_row of engine.hip)
                key = g.M_pad + (s < Lb ? s : (s < g.L ? Lb + g.P + (s - Lb) : Lb + (s - g.L)));
            }
            const int kr = key & 31, r = (kr & 3) + 4 * (kr >> 3), ln = ((kr >> 2) & 1) * 32 + (q & 31);
            v = g.scratch[((((size_t)b * nqt + (q >> 5)) * nkt + (key >> 5)) * 16 + r) * 64 + ln];
        }
        g.out[i] = v;
    }
}

void xattn_map_gather(const XattnGatherArgs& g, mgStream_t stream) {
    const size_t n = (size_t)g.B * g.Sq * (g.M_e1 + g.L + g.P);
    size_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    MG_LAUNCH(xattn_map_gather_kernel, dim3((unsigned)(blocks ? blocks : 1)), dim3(256), 0, stream, g);
}

}  // namespace mg

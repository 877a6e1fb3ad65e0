// C-ABI operator entry points (kernel-level): what the parity tests call to compare each HIP kernel with the
// oracle.  Plain pointers and sizes only; all pointers are device pointers; work is enqueued on `stream`.
#include "mg_kernels.h"
#include "mg_swin.h"
#include "mg_ocr.h"
#include <stdlib.h>
#include "../../include/mgrapher.h"

using namespace mg;

extern "C" {

int mgk_pack_weight(void* stream, const void* src, int src_is_bf16, int N, int K, void* dst_pk, int Npad) {
    if ((K & 15) || (Npad & 31) || Npad < N) return MG_E_SHAPE;
    pack_weight(src, src_is_bf16, N, K, (uint16_t*)dst_pk, Npad, (mgStream_t)stream);
    return MG_OK;
}

int mgk_rmsnorm_pack(void* stream, const float* h, const float* gain, void* x_pk, float* out_f32, int M, int d,
                     float eps, float scale) {
    if (d & 15) return MG_E_SHAPE;
    rmsnorm_pack(h, gain, (uint16_t*)x_pk, out_f32, M, d, eps, scale, (mgStream_t)stream);
    return MG_OK;
}

int mgk_im2col_pack(void* stream, const float* pix, void* x_pk, int B, int C, int I, int ps) {
    if ((ps & 7) || (I % ps)) return MG_E_SHAPE;
    im2col_pack(pix, (uint16_t*)x_pk, B, C, I, ps, (mgStream_t)stream);
    return MG_OK;
}

// mode: 0 = tiled (large M), 1 = row-streaming (decode step)
int mgk_set_rows_split(int mode) { gemm_rows_set_split(mode); return MG_OK; }
int mgk_set_resid_f16(int on) { gemm_rows_set_resid_f16(on); return MG_OK; }
int mgk_set_rows_ft2(int mode) { gemm_rows_set_ft2(mode); return MG_OK; }
int mgk_gemm(void* stream, int mode, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* out_f32,
             int ldo, const float* bias, void* out_pk) {
    const bool swin_epi = epi == EPI_PK_BIAS || epi == EPI_PK_GELU_ERF;      // (the Swin branch's: every tile kernel family has them)
    if ((K & 63) || epi < 0 || (epi > EPI_PK && epi != EPI_PK_GELU && !swin_epi)) return MG_E_SHAPE;
    if (epi == EPI_PK_GELU && !(mode == 0 && gemm_has_gelu_epilogue(M, N))) return MG_E_UNSUPPORTED;
    if (swin_epi && mode != 0) return MG_E_UNSUPPORTED;
    if (swin_epi && ((N & 15) || !out_pk)) return MG_E_SHAPE;
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    a.out_f32 = out_f32; a.ldo = ldo; a.bias = bias; a.out_pk = (uint16_t*)out_pk;
    if (mode == 0) gemm(a, epi, (mgStream_t)stream); else gemm_rows(a, epi, (mgStream_t)stream);
    return MG_OK;
}

// Deferred-RMSNorm pair of the encoder (test entry):
//   epi = EPI_RESID_NORM (5): h_tiled (fp32, layout ht_off) += X W^T, x_out_pk = pack(bf16(h * gain)), part[M][part_ld] partial sums
//   epi = EPI_PK / EPI_PK_RELU (3 / 2): out_pk = pack(bf16(relu?(X W^T * r(m)))) with r from rs_part[M][rs_nparts] (null: r = 1)
int mgk_gemm_norm(void* stream, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* h_tiled, const float* gain,
                  void* out_pk, float* part, int part_ld, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps) {
    // (a ragged M only in the form the Swin branch issues: the plain tiled residual update without gain / packed output / partial sums)
    const bool plain_resid = epi == EPI_RESID_NORM && !gain && !out_pk && !part && !rs_part;
    if ((K & 63) || (N & 31) || ((M & 31) && !plain_resid) || M < 1) return MG_E_SHAPE;
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    a.out_f32 = h_tiled; a.gain = gain; a.out_pk = (uint16_t*)out_pk; a.part = part; a.ldo = part_ld;
    a.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps};
    gemm(a, epi, (mgStream_t)stream);
    return MG_OK;
}

// Large-M GEMM restricted to the 32-row tiles with a non-zero entry in row_mask [M] (M a multiple of 32): the row-tile list form
// the encoder uses.  list_scratch: M/32 + 1 ints.  epi as mgk_gemm_norm (5: tiled residual + packed x + partial sums; 2 / 3: packed
// outputs, rows scaled by rs_*) or 0 / 1 (fp32 store / accumulate, row-major ldo = N).
int mgk_gemm_row_tiles(void* stream, int epi, const void* X_pk, const void* W_pk, int M, int N, int K, float* out_f32, const float* gain,
                       void* out_pk, float* part, int part_ld, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps,
                       const uint8_t* row_mask, int* list_scratch) {
    if ((K & 63) || (N & 31) || (M & 31) || !row_mask || !list_scratch) return MG_E_SHAPE;
    row_tile_list(row_mask, M, list_scratch + 1, list_scratch, (mgStream_t)stream);
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    a.out_f32 = out_f32; a.gain = gain; a.out_pk = (uint16_t*)out_pk; a.part = part; a.ldo = (epi == EPI_RESID_NORM) ? part_ld : N;
    a.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps};
    a.row_tiles = list_scratch + 1; a.n_row_tiles = list_scratch;
    gemm(a, epi, (mgStream_t)stream);
    return MG_OK;
}

int mgk_gemm_heads(void* stream, int mode, const void* X_pk, const void* W_pk, int M, int N, int K, void* p0, void* p1,
                   void* p2, int f0, int f1, int f2, int H, int S_in, int S_cap, const int* row_map, int pos) {
    if ((K & 63) || (N % (H * 64))) return MG_E_SHAPE;
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    a.heads.ptr[0] = (uint16_t*)p0; a.heads.ptr[1] = (uint16_t*)p1; a.heads.ptr[2] = (uint16_t*)p2;
    a.heads.fmt[0] = f0; a.heads.fmt[1] = f1; a.heads.fmt[2] = f2;
    a.heads.inner = H * 64; a.heads.H = H; a.heads.S_in = S_in; a.heads.S_cap = S_cap; a.heads.row_map = row_map;
    a.heads.pos = pos;
    if (mode == 0) gemm(a, EPI_HEADS, (mgStream_t)stream); else gemm_rows(a, EPI_HEADS, (mgStream_t)stream);
    return MG_OK;
}

int mgk_gemm_heads_step(void* stream, const void* X_pk, int x_kts, int x_k0, const void* W_pk, int M, int N, int K, void* p0, void* p1, void* p2,
                        int f0, int f1, int f2, int H, int S_cap, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, int pos,
                        const int* pos_dev, const int* pos_rows, int both_halves) {
    if (!X_pk || !W_pk) return MG_E_ARG;
    if (K < 64 || (K & 63) || H < 1 || N < H * 64 || (N % (H * 64)) || N > 3 * H * 64 || M < 1 || M > 256 || S_cap < 1) return MG_E_SHAPE;
    if (x_kts ? (x_k0 < 0 || x_k0 + (K >> 4) > x_kts) : x_k0 != 0) return MG_E_SHAPE;
    if (rs_part && (rs_nparts < 8 || (rs_nparts & 7))) return MG_E_SHAPE;
    void* const ptr[3] = {p0, p1, p2};
    const int fmt[3] = {f0, f1, f2};
    bool kv = false;
    for (int i = 0; i < 3; ++i) {
        if (fmt[i] != HF_NONE && fmt[i] != HF_STEP_Q && fmt[i] != HF_STEP_KV) return MG_E_UNSUPPORTED;
        if (i < N / (H * 64) && fmt[i] != HF_NONE && !ptr[i]) return MG_E_ARG;
        kv = kv || fmt[i] == HF_STEP_KV;
    }
    if (kv && !pos_dev && !pos_rows && (pos < 0 || pos >= S_cap)) return MG_E_SHAPE;
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.x_kts = x_kts; a.x_k0 = x_k0; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    for (int i = 0; i < 3; ++i) { a.heads.ptr[i] = (uint16_t*)ptr[i]; a.heads.fmt[i] = fmt[i]; }
    a.heads.inner = H * 64; a.heads.H = H; a.heads.S_in = M; a.heads.S_cap = S_cap;
    a.heads.pos = pos; a.heads.pos_dev = pos_dev; a.heads.pos_rows = pos_rows;
    a.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps};
    a.both_halves = both_halves;
    gemm_rows(a, EPI_HEADS, (mgStream_t)stream);
    return MG_OK;
}

int mgk_attention(void* stream, int mode, const void* Q, const void* K, const void* Vt, void* ctx_pk, int B, int H,
                  int Sq, int Sk, int Sq_cap, int Sk_cap, const uint8_t* kmask, const float* tab1, int tab1_len,
                  const float* tabh, const float* tabv, const double* cx, const double* cy, const int* bk1, const int* bkhv,
                  void* bidx_scratch) {
    if ((Sq_cap & 31) || (Sk_cap & 63) || Sk > Sk_cap || Sq > Sq_cap || mode < 0 || mode > 2) return MG_E_SHAPE;
    AttnArgs a{};
    a.Q = (const uint16_t*)Q; a.K = (const uint16_t*)K; a.Vt = (const uint16_t*)Vt; a.ctx = (uint16_t*)ctx_pk;
    a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.Sq_cap = Sq_cap; a.Sk_cap = Sk_cap; a.mode = mode; a.kmask = kmask;
    a.tab1 = tab1; a.tab1_len = tab1_len; a.tabh = tabh; a.tabv = tabv;
    if (mode == ATT_ENC) {
        if (!bidx_scratch || !bk1 || !bkhv || !cx || !cy || Sq_cap != Sk_cap) return MG_E_ARG;
        bias_index((uint16_t*)bidx_scratch, cx, cy, kmask, bk1, bkhv, B, Sk, Sk_cap, (mgStream_t)stream);
        a.bidx = (const uint16_t*)bidx_scratch;
        a.bk1 = bk1;
    }
    attention(a, (mgStream_t)stream);
    return MG_OK;
}

// encoder attention with the padded-stage / padded-block skip lists built from the key mask (as mg_encode runs it)
int mgk_attention_enc_skip(void* stream, const void* Q, const void* K, const void* Vt, void* ctx_pk, int B, int H, int S, int S_cap,
                           const uint8_t* kmask, const float* tab1, const float* tabh, const float* tabv, const double* cx,
                           const double* cy, const int* bk1, const int* bkhv, void* bidx_scratch, int* kst_scratch,
                           uint8_t* qbv_scratch) {
    if ((S_cap & 63) || S > S_cap || !kmask || !bidx_scratch || !kst_scratch || !qbv_scratch) return MG_E_ARG;
    AttnArgs a{};
    a.Q = (const uint16_t*)Q; a.K = (const uint16_t*)K; a.Vt = (const uint16_t*)Vt; a.ctx = (uint16_t*)ctx_pk;
    a.B = B; a.H = H; a.Sq = S; a.Sk = S; a.Sq_cap = S_cap; a.Sk_cap = S_cap; a.mode = ATT_ENC; a.kmask = kmask;
    a.tab1 = tab1; a.tab1_len = 32; a.tabh = tabh; a.tabv = tabv;
    bias_index((uint16_t*)bidx_scratch, cx, cy, kmask, bk1, bkhv, B, S, S_cap, (mgStream_t)stream);
    attn_lists(kmask, B, S, S_cap, kst_scratch, qbv_scratch, (mgStream_t)stream);
    a.bidx = (const uint16_t*)bidx_scratch; a.bk1 = bk1; a.kst = kst_scratch; a.qbv = qbv_scratch;
    attention(a, (mgStream_t)stream);
    return MG_OK;
}

int mgk_attention_step(void* stream, const void* q, const void* Kc, const void* Vc, void* ctx_pk, int rows, int H,
                       int group, int cap, const int* len, int n_keys, const float* bias, const int* anc, int t) {
    if (group < 1 || group > 8) return MG_E_SHAPE;
    AttnStepArgs a{};
    a.q = (const uint16_t*)q; a.Kc = (const uint16_t*)Kc; a.Vc = (const uint16_t*)Vc; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H; a.group = group; a.cap = cap; a.len = len; a.n_keys = n_keys; a.bias = bias; a.anc = anc;
    a.t = t;
    attention_step(a, (mgStream_t)stream);
    return MG_OK;
}

// mgk_attention_step with the AttnStepArgs fields the engine sets on every decode step (test entry; nullable pointers = not used, as in
// AttnStepArgs): the position from device memory (t_dev + t_off) or per row (pos_rows), the K/V pool indirection (kv_owner: per row for
// group 1, per owner = image slot otherwise), dead rows (live), the deferred RMSNorm scale of the queries (qrs_*), the context as a
// column window [ctx_col0, ctx_col0 + H*64) of a packed buffer of ctx_ld columns, and the one-workgroup-per-CU residency of the cross form.
int mgk_attention_step_ex(void* stream, const void* q, const void* Kc, const void* Vc, void* ctx_pk, int rows, int H, int group, int cap,
                          const int* len, int n_keys, const float* bias, const int* anc, int t, const int* t_dev, int t_off,
                          const int* pos_rows, const int* kv_owner, const int* live, const float* qrs_part, int qrs_nparts, float qrs_inv_d,
                          float qrs_eps, int ctx_ld, int ctx_col0, int one_wg_per_cu) {
    if (group < 1 || group > 8 || rows < 1) return MG_E_SHAPE;
    if (ctx_ld ? ((ctx_ld & 15) || ctx_col0 < 0 || ctx_col0 + H * 64 > ctx_ld) : ctx_col0 != 0) return MG_E_SHAPE;
    if (one_wg_per_cu) attention_step_allow_shared();
    AttnStepArgs a{};
    a.q = (const uint16_t*)q; a.Kc = (const uint16_t*)Kc; a.Vc = (const uint16_t*)Vc; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H; a.group = group; a.cap = cap; a.len = len; a.n_keys = n_keys; a.bias = bias; a.anc = anc;
    a.t = t; a.t_dev = t_dev; a.t_off = t_off; a.pos_rows = pos_rows; a.kv_owner = kv_owner; a.live = live;
    a.qrs = RowScale{qrs_part, qrs_nparts, qrs_inv_d, qrs_eps};
    a.ctx_ld = ctx_ld; a.ctx_col0 = ctx_col0; a.one_wg_per_cu = one_wg_per_cu;
    attention_step(a, (mgStream_t)stream);
    return MG_OK;
}

// The rotary grouped-query form (every layer of the ChemicalOCR text model; test entry): qkv fp32 [rows][ld] = [H_kv*group q heads |
// H_kv k heads | H_kv v heads] x 64 un-normalised, cs [positions][cos 32 | sin 32], rs_* the deferred RMSNorm scale of the rows
// (rs_part null: none), Kc / Vc [pages][H_kv][cap][64] bf16 - read over [0, position) and appended to at the position.  Position of a
// row: pos_rows ? pos_rows[row] + t_off : (t_dev ? *t_dev + t_off : t), plus t_off_rows[page] where given; page = kv_owner ? kv_owner[row]
// : row.  ctx_pk packed [rows padded to 32][ctx_ld ? ctx_ld : H_kv*group*64], written at columns ctx_col0 on.
int mgk_attention_step_rope(void* stream, const float* qkv, int ld, const float* cs, const float* rs_part, int rs_nparts, float rs_inv_d,
                            float rs_eps, float qscale, void* Kc, void* Vc, void* ctx_pk, int rows, int H_kv, int group, int cap, int t,
                            const int* t_dev, int t_off, const int* pos_rows, const int* t_off_rows, const int* kv_owner, const int* live,
                            int ctx_ld, int ctx_col0) {
    if (group < 1 || group > 8 || group == 5 || group == 7 || rows < 1) return MG_E_SHAPE;      // (attention_step has no rotary case for 5 and 7)
    if (!qkv || !cs || ld < (group + 2) * H_kv * 64 || (ld & 3)) return MG_E_ARG;
    if (ctx_ld ? ((ctx_ld & 15) || ctx_col0 < 0 || ctx_col0 + H_kv * group * 64 > ctx_ld) : ctx_col0 != 0) return MG_E_SHAPE;
    AttnStepArgs a{};
    a.Kc = (const uint16_t*)Kc; a.Vc = (const uint16_t*)Vc; a.Kc_w = (uint16_t*)Kc; a.Vc_w = (uint16_t*)Vc; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H_kv; a.group = group; a.cap = cap; a.n_keys = t + 1; a.t = t; a.t_dev = t_dev; a.t_off = t_off;
    a.pos_rows = pos_rows; a.t_off_rows = t_off_rows; a.kv_owner = kv_owner; a.live = live;
    a.rope.qkv = qkv; a.rope.ld = ld; a.rope.cs = cs; a.rope.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps}; a.rope.qscale = qscale;
    a.ctx_ld = ctx_ld; a.ctx_col0 = ctx_col0;
    attention_step(a, (mgStream_t)stream);
    return MG_OK;
}

#ifdef MG_TOOLS
int mgk_attention_step_trace(void* stream, const void* q, const void* Kc, const void* Vc, void* ctx_pk, int rows, int H, int cap,
                             const int* len, long long* trace) {
    AttnStepArgs a{};
    a.q = (const uint16_t*)q; a.Kc = (const uint16_t*)Kc; a.Vc = (const uint16_t*)Vc; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H; a.group = 1; a.cap = cap; a.len = len;
    attention_step_trace(a, trace, (mgStream_t)stream);
    return MG_OK;
}
#endif

// Weight-absorbed cross-attention of the greedy decode step (k_xattn.hip), the three launches of a layer + the weight re-ordering:
// q [rows][H][64] bf16, wkv fp32 [2*H*64][d] (K rows first), enc [owners][cap][d] bf16 natural rows, len [owners], kv_owner [rows]
// (nullable).  Scratch: wk, wv [H*d*64] bf16 each, qx [rows][H][d] bf16, part [rows][nsplit][H][d] bf16, ml [rows][nsplit][H][2] fp32.
// Result: ctx_pk packed [rows padded to 32][H*64] bf16.
int mgk_xattn(void* stream, const void* q, const float* wkv, const void* enc, const int* len, const int* kv_owner, int rows, int H, int d,
              int cap, int nsplit, int nstg, void* wk, void* wv, void* qx, void* part, float* ml, void* ctx_pk) {
    if (!xattn_supported(d, H) || nsplit < 1 || nsplit > 4 || (nstg != 3 && nstg != 4)) return MG_E_UNSUPPORTED;
    mgStream_t st = (mgStream_t)stream;
    xattn_pack_weights(wkv, (uint16_t*)wk, (uint16_t*)wv, H, d, st);
    xattn_stream_prepare(d, nstg);
    XAttnArgs a{};
    a.q = (const uint16_t*)q; a.qx = (uint16_t*)qx; a.wk = (const uint16_t*)wk; a.wv = (const uint16_t*)wv; a.enc = (const uint16_t*)enc;
    a.len = len; a.kv_owner = kv_owner; a.part = (uint16_t*)part; a.ml = ml; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H; a.d = d; a.cap = cap; a.nsplit = nsplit; a.nstg = nstg;
    { const char* e = getenv("MG_XATTN_NT"); a.nt = e ? atoi(e) : 1; }
    xattn_expand(a, st);
    xattn_stream(a, st);
    xattn_contract(a, st);
    return MG_OK;
}
// The same for beam search (xattn_stream_beams): `group` rows per owner, kv_owner indexed by image, live [rows] nullable; beams_per_wg 0 =
// the engine's choice; nt: cache policy of the stream's copies.
int mgk_xattn_beams(void* stream, const void* q, const float* wkv, const void* enc, const int* len, const int* kv_owner, const int* live,
                    int rows, int H, int d, int cap, int group, int nsplit, int nstg, int beams_per_wg, int nt, void* wk, void* wv, void* qx,
                    void* part, float* ml, void* ctx_pk) {
    if (!xattn_supported(d, H) || nsplit < 1 || nsplit > 4 || (nstg != 3 && nstg != 4)) return MG_E_UNSUPPORTED;
    if (group < 1 || rows < group || rows % group != 0 || beams_per_wg < 0 || !xattn_beams_bp(d, nstg, beams_per_wg)) return MG_E_UNSUPPORTED;
    mgStream_t st = (mgStream_t)stream;
    xattn_pack_weights(wkv, (uint16_t*)wk, (uint16_t*)wv, H, d, st);
    xattn_beams_prepare(d);
    XAttnArgs a{};
    a.q = (const uint16_t*)q; a.qx = (uint16_t*)qx; a.wk = (const uint16_t*)wk; a.wv = (const uint16_t*)wv; a.enc = (const uint16_t*)enc;
    a.len = len; a.kv_owner = kv_owner; a.live = live; a.part = (uint16_t*)part; a.ml = ml; a.ctx = (uint16_t*)ctx_pk;
    a.rows = rows; a.H = H; a.d = d; a.cap = cap; a.nsplit = nsplit; a.nstg = nstg; a.nt = nt ? 1 : 0; a.group = group; a.bpw = beams_per_wg;
    xattn_expand(a, st);
    xattn_stream_beams(a, st);
    xattn_contract(a, st);
    return MG_OK;
}
// rows of a packed [B*rows_per_image][d] bf16 operand -> natural rows dst[b][row_map[r]][d] (k_xattn.hip enc_rows)
int mgk_enc_rows(void* stream, const void* src_pk, const int* row_map, void* dst, int B, int rows_per_image, int cap, int d) {
    enc_rows((const uint16_t*)src_pk, row_map, (uint16_t*)dst, B, rows_per_image, cap, d, (mgStream_t)stream);
    return MG_OK;
}

size_t mgk_embed_meta_bytes(int B, int S_cap) { return embed_meta_bytes(B, S_cap); }

int mgk_embed_assemble(void* stream, void* meta_ws, const int64_t* input_ids, const float* bbox,
                       const uint8_t* attention_mask, const float* patch_emb, const void* tok_emb, const void* x_emb,
                       const void* y_emb, int B, int L, int P, int d, int n_side, int M2, int V, int S_cap,
                       float* hidden, double* cx, double* cy, uint8_t* mask, int* xrow, int* xlen, int* err) {
    if (S_cap < L + P || (d & 3) || P != n_side * n_side) return MG_E_SHAPE;
    EmbedArgs a{};
    a.input_ids = input_ids; a.bbox = bbox; a.attn_mask = attention_mask; a.patch_emb = patch_emb;
    a.tok_emb = (const uint16_t*)tok_emb; a.x_emb = (const uint16_t*)x_emb; a.y_emb = (const uint16_t*)y_emb;
    a.B = B; a.L = L; a.P = P; a.d = d; a.n_side = n_side; a.M2 = M2; a.V = V; a.S_cap = S_cap;
    a.hidden = hidden; a.cx = cx; a.cy = cy; a.mask = mask; a.xrow = xrow; a.xlen = xlen; a.err = err;
    embed_assemble(a, meta_ws, (mgStream_t)stream);
    return MG_OK;
}

int mgk_greedy_select(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len,
                      int64_t* next_ids, int64_t* out_ids, int max_len, int pos, int* unfinished, int* n_unfinished,
                      float* top2) {
    ArgmaxArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.top2 = top2;
    mg_memset_async(n_unfinished, 0, sizeof(int), (mgStream_t)stream);   // the kernel accumulates
    greedy_select(a, (mgStream_t)stream);
    return MG_OK;
}

// greedy_select with token scores (ArgmaxArgs::token_scores [rows][ts_ld], written at column pos - 1)
int mgk_greedy_select_scored(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len,
                             int64_t* next_ids, int64_t* out_ids, int max_len, int pos, int* unfinished, int* n_unfinished,
                             float* token_scores, int ts_ld) {
    ArgmaxArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.token_scores = token_scores; a.ts_ld = ts_ld;
    mg_memset_async(n_unfinished, 0, sizeof(int), (mgStream_t)stream);
    greedy_select(a, (mgStream_t)stream);
    return MG_OK;
}

// sample_select at operator level (k_sample.hip): one launch over `rows` rows at column `pos`; token_scores [rows][ts_ld] nullable
int mgk_sample_select(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                      int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                      int pos, int* unfinished, int* n_unfinished, float* token_scores, int ts_ld) {
    if (!logits || !next_ids || !out_ids || !unfinished || !n_unfinished || rows < 1 || ldl < V || (ldl & 3)) return MG_E_ARG;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return MG_E_ARG;
    if (!sample_select_supported(V)) return MG_E_UNSUPPORTED;
    SampleArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.stream_ids = stream_ids;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.token_scores = token_scores; a.ts_ld = ts_ld;
    mg_memset_async(n_unfinished, 0, sizeof(int), (mgStream_t)stream);   // the kernel accumulates
    sample_select(a, (mgStream_t)stream);
    return MG_OK;
}

// The selection step in every form the decode loops launch it in (greedy_select batch / queue, greedy_select_fused, sample_select queue,
// slot_refill): descriptors as mgk_gemm_resid_ex.  None of them clears n_unfinished (the engine does not either: the step_ctr path does).
static SlotTable slot_table(const mgk_slot_table* t) {
    SlotTable s{};
    if (!t) return s;
    s.pos = t->pos; s.img = t->img; s.pool = t->pool; s.ctr = t->ctr; s.out_len = t->out_len; s.pool_cap = t->pool_cap; s.start_id = t->start_id;
    s.first_tok = t->first_tok; s.n_stop = t->n_stop; s.max_len = t->max_len; s.nsamp = t->nsamp;
    for (int k = 0; k < 4; ++k) s.stop[k] = t->stop[k];
    return s;
}
// the operator entries' constraint -> DecConstraint; MG_E_ARG before any device work (sizes as mg_generate_constrained checks them)
static int dec_constraint(const mgk_constraint* c, DecConstraint* out) {
    if (!c || !c->cls || !c->table || !c->state || !c->empty) return MG_E_ARG;
    if (c->n_classes < 1 || c->n_classes > DEC_CON_MAX_CLASSES || c->n_states < 2) return MG_E_ARG;
    if ((long long)c->n_states * c->n_classes > (1ll << 24)) return MG_E_ARG;
    *out = DecConstraint{c->cls, c->table, c->n_states, c->n_classes, c->state, c->empty};
    return MG_OK;
}
static int select_impl(void* stream, const mgk_select_desc* s, const DecPrompt& prompt, const DecConstraint& con = DecConstraint{},
                       bool queue_ex = false) {
    if (!s || !s->next_ids || !s->out_ids || !s->unfinished) return MG_E_ARG;
    const bool queue = s->slots.pos != nullptr;
    if (queue_ex && !queue) return MG_E_ARG;
    // (the operators from before the queue forms took a prompt and a constraint keep refusing them with a slot table: mgk_select_queue_ex takes those)
    if (con.cls && ((queue && !queue_ex) || s->fused || s->ptop)) return MG_E_ARG;      // (a constraint belongs to the scan: no fused tail, no ptop)
    if (prompt.ids && ((queue && !queue_ex) || !prompt.len || prompt.ld < 1 || prompt.group < 0)) return MG_E_ARG;
    if (s->fused && queue) return MG_E_ARG;                              // (the fused tail has no queue form)
    if (queue ? (!s->slots.img || !s->slots.ctr || !s->slots.out_len) : !s->n_unfinished) return MG_E_ARG;
    if (s->n_eos_more < 0 || s->n_eos_more > 3) return MG_E_ARG;
    if (s->rows < 1 || s->rows > 256 || s->V < 1 || s->max_len < 1 || s->pos < 0) return MG_E_SHAPE;
    if (s->token_scores && (s->ts_ld < s->max_len - 1 || (!queue && !s->pos_dev && s->pos < 1))) return MG_E_SHAPE;
    if (s->fused) {
        if (!s->ptop || !s->stopv || !s->tok_emb || !s->gain || !s->h || !s->x_pk) return MG_E_ARG;
        if (s->d < 16 || s->d > 2048 || (s->d & 15) || s->ntiles != (s->V + 31) / 32) return MG_E_SHAPE;
        if (s->pad < 0 || s->pad >= s->V) return MG_E_ARG;               // (a finished row embeds pad)
        if (s->x2_pk && ((s->x2_ld & 15) || s->x2_col0 < 0 || (s->x2_col0 & 7) || s->x2_col0 + s->d > s->x2_ld)) return MG_E_SHAPE;
    } else {
        if (!s->logits) return MG_E_ARG;
        if (s->ldl < s->V || (s->ldl & 3)) return MG_E_SHAPE;
    }
    ArgmaxArgs a{};
    a.logits = s->logits; a.rows = s->rows; a.V = s->V; a.ldl = s->ldl; a.eos = s->eos; a.pad = s->pad; a.suppress_eos = s->suppress_eos;
    a.n_eos_more = s->n_eos_more;
    for (int k = 0; k < 3; ++k) a.eos_more[k] = s->eos_more[k];
    a.next_ids = s->next_ids; a.out_ids = s->out_ids; a.max_len = s->max_len; a.pos = s->pos; a.pos_dev = s->pos_dev; a.min_len = s->min_len;
    a.unfinished = s->unfinished; a.n_unfinished = s->n_unfinished; a.top2 = s->top2; a.step_ctr = s->step_ctr;
    if (queue) a.slots = slot_table(&s->slots);
    a.ptop = (const float4*)s->ptop; a.stopv = s->stopv; a.ntiles = s->ntiles; a.tok_emb = (const uint16_t*)s->tok_emb; a.h = s->h;
    a.gain = s->gain; a.x_pk = (uint16_t*)s->x_pk; a.x2_pk = (uint16_t*)s->x2_pk; a.x2_ld = s->x2_ld; a.x2_col0 = s->x2_col0; a.d = s->d;
    a.eps = s->eps; a.token_scores = s->token_scores; a.ts_ld = s->ts_ld;
    a.prompt = prompt;
    a.con = con;
    if (s->fused) greedy_select_fused(a, (mgStream_t)stream); else greedy_select(a, (mgStream_t)stream);
    return MG_OK;
}
int mgk_select_ex(void* stream, const mgk_select_desc* s) { return select_impl(stream, s, DecPrompt{}); }
// mgk_select_ex under a decoder prompt (DecPrompt, mg_kernels.h): batch forms only
int mgk_select_prompted(void* stream, const mgk_select_desc* s, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int group,
                        int* bad) {
    if (!prompt_ids) return MG_E_ARG;
    return select_impl(stream, s, DecPrompt{prompt_ids, prompt_len, prompt_ld, group, bad});
}
// mgk_sample_select under a decoder prompt, with the step bookkeeping of the engine's launch (pos_dev / step_ctr nullable)
int mgk_sample_select_prompted(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                               int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                               int pos, const int* pos_dev, int* unfinished, int* n_unfinished, int* step_ctr, float* token_scores, int ts_ld,
                               const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int group, int* bad) {
    if (!logits || !next_ids || !out_ids || !unfinished || !n_unfinished || rows < 1 || ldl < V || (ldl & 3)) return MG_E_ARG;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return MG_E_ARG;
    if (!prompt_ids || !prompt_len || prompt_ld < 1 || group < 0) return MG_E_ARG;
    if (rows > 256 || max_len < 1 || (token_scores && ts_ld < max_len - 1)) return MG_E_SHAPE;
    if (!sample_select_supported(V)) return MG_E_UNSUPPORTED;
    SampleArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.stream_ids = stream_ids;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.pos_dev = pos_dev; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.step_ctr = step_ctr; a.token_scores = token_scores; a.ts_ld = ts_ld;
    a.prompt = DecPrompt{prompt_ids, prompt_len, prompt_ld, group, bad};
    sample_select(a, (mgStream_t)stream);      // (n_unfinished is not cleared: the caller sets it, the step_ctr path clears it)
    return MG_OK;
}
// mgk_select_ex under a constraint (DecConstraint, mg_kernels.h), with an optional decoder prompt (prompt_ids null: none)
int mgk_select_constrained(void* stream, const mgk_select_desc* s, const mgk_constraint* con, const int64_t* prompt_ids, const int* prompt_len,
                           int prompt_ld, int group, int* bad) {
    DecConstraint dc{};
    const int rc = dec_constraint(con, &dc);
    if (rc != MG_OK) return rc;
    return select_impl(stream, s, prompt_ids ? DecPrompt{prompt_ids, prompt_len, prompt_ld, group, bad} : DecPrompt{}, dc);
}
// mgk_sample_select_prompted under a constraint (prompt_ids null: no prompt), top2 [rows][2] nullable as the engine's launch has it
int mgk_sample_select_constrained(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                                  int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids,
                                  int max_len, int pos, const int* pos_dev, int* unfinished, int* n_unfinished, int* step_ctr, float* token_scores,
                                  int ts_ld, float* top2, const mgk_constraint* con, const int64_t* prompt_ids, const int* prompt_len,
                                  int prompt_ld, int group, int* bad) {
    if (!logits || !next_ids || !out_ids || !unfinished || !n_unfinished || rows < 1 || ldl < V || (ldl & 3)) return MG_E_ARG;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return MG_E_ARG;
    if (prompt_ids && (!prompt_len || prompt_ld < 1 || group < 0)) return MG_E_ARG;
    DecConstraint dc{};
    const int rc = dec_constraint(con, &dc);
    if (rc != MG_OK) return rc;
    if (rows > 256 || max_len < 1 || (token_scores && ts_ld < max_len - 1)) return MG_E_SHAPE;
    if (!sample_select_supported(V)) return MG_E_UNSUPPORTED;
    SampleArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.stream_ids = stream_ids;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.pos_dev = pos_dev; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.step_ctr = step_ctr; a.token_scores = token_scores; a.ts_ld = ts_ld; a.top2 = top2;
    if (prompt_ids) a.prompt = DecPrompt{prompt_ids, prompt_len, prompt_ld, group, bad};
    a.con = dc;
    sample_select(a, (mgStream_t)stream);      // (n_unfinished is not cleared, as in mgk_sample_select_prompted)
    return MG_OK;
}
int mgk_sample_select_queue(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                            int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                            int pos, int* unfinished, int* n_unfinished, float* token_scores, int ts_ld, const mgk_slot_table* slots) {
    if (!logits || !next_ids || !out_ids || !unfinished || !n_unfinished || rows < 1 || ldl < V || (ldl & 3)) return MG_E_ARG;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return MG_E_ARG;
    if (!slots || !slots->pos || !slots->img || !slots->ctr || !slots->out_len) return MG_E_ARG;
    if (rows > 256 || max_len < 1 || (token_scores && ts_ld < max_len - 1)) return MG_E_SHAPE;
    if (!sample_select_supported(V)) return MG_E_UNSUPPORTED;
    SampleArgs a{};
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.stream_ids = stream_ids;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.token_scores = token_scores; a.ts_ld = ts_ld; a.slots = slot_table(slots);
    sample_select(a, (mgStream_t)stream);
    return MG_OK;
}
// The queue forms under a decoder prompt and / or a constraint (mg_generate_stream_constrained): the prompt and the start states are per
// image of the queue, the states per slot
static int queue_con(const mgk_queue_con* q, DecPrompt* dp, DecConstraint* dc) {
    if (!q) return MG_OK;
    if (q->prompt_ids) {
        if (!q->prompt_len || q->prompt_ld < 1 || q->V < 1) return MG_E_ARG;
        *dp = DecPrompt{q->prompt_ids, q->prompt_len, q->prompt_ld, 1, q->bad};
    }
    if (q->con) return dec_constraint(q->con, dc);
    return MG_OK;
}
int mgk_select_queue_ex(void* stream, const mgk_select_desc* s, const mgk_queue_con* q) {
    DecPrompt dp{};
    DecConstraint dc{};
    const int rc = queue_con(q, &dp, &dc);
    if (rc != MG_OK) return rc;
    return select_impl(stream, s, dp, dc, true);
}
int mgk_sample_select_queue_ex(void* stream, const float* logits, int rows, int V, int ldl, int eos, int pad, int min_len, float temperature,
                               int top_k, float top_p, uint64_t seed, const uint64_t* stream_ids, int64_t* next_ids, int64_t* out_ids, int max_len,
                               int* unfinished, float* token_scores, int ts_ld, const mgk_slot_table* slots, const mgk_queue_con* q) {
    if (!logits || !next_ids || !out_ids || !unfinished || rows < 1 || ldl < V || (ldl & 3)) return MG_E_ARG;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return MG_E_ARG;
    if (!slots || !slots->pos || !slots->img || !slots->ctr || !slots->out_len) return MG_E_ARG;
    if (rows > 256 || max_len < 1 || (token_scores && ts_ld < max_len - 1)) return MG_E_SHAPE;
    if (!sample_select_supported(V)) return MG_E_UNSUPPORTED;
    SampleArgs a{};
    const int rc = queue_con(q, &a.prompt, &a.con);
    if (rc != MG_OK) return rc;
    a.logits = logits; a.rows = rows; a.V = V; a.ldl = ldl; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.stream_ids = stream_ids;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.unfinished = unfinished;
    a.token_scores = token_scores; a.ts_ld = ts_ld; a.slots = slot_table(slots);
    sample_select(a, (mgStream_t)stream);
    return MG_OK;
}
int mgk_slot_refill_ex(void* stream, const mgk_slot_table* slots, int64_t* next_ids, int* unfinished, int rows, const mgk_queue_con* q,
                       int64_t* out_ids, int out_ld) {
    if (!slots || !slots->pos || !slots->img || !slots->pool || !slots->ctr || !slots->out_len || !next_ids || !unfinished) return MG_E_ARG;
    if (slots->nsamp < 1 || slots->pool_cap < 1 || slots->n_stop < 0 || slots->n_stop > 4) return MG_E_ARG;
    if (rows < 1 || rows > 256) return MG_E_SHAPE;
    SlotTable t = slot_table(slots);
    DecPrompt dp{};
    DecConstraint dc{};
    const int rc = queue_con(q, &dp, &dc);
    if (rc != MG_OK) return rc;
    if (dp.ids) {
        if (out_ids && out_ld < 1) return MG_E_ARG;
        t.q_prompt_ids = dp.ids; t.q_prompt_ld = dp.ld; t.q_V = q->V; t.q_bad = dp.bad; t.q_out_ids = out_ids; t.q_out_ld = out_ld;
    }
    if (dc.cls) {
        if (!q->con_start) return MG_E_ARG;
        t.q_con_start = q->con_start; t.q_con_state = dc.state;
    }
    slot_refill(t, next_ids, unfinished, rows, (mgStream_t)stream);
    return MG_OK;
}
int mgk_slot_refill(void* stream, const mgk_slot_table* slots, int64_t* next_ids, int* unfinished, int rows) {
    if (!slots || !slots->pos || !slots->img || !slots->pool || !slots->ctr || !slots->out_len || !next_ids || !unfinished) return MG_E_ARG;
    if (slots->nsamp < 1 || slots->pool_cap < 1 || slots->n_stop < 0 || slots->n_stop > 4) return MG_E_ARG;
    if (rows < 1 || rows > 256) return MG_E_SHAPE;                       // (the kernel keeps the slots' state in two LDS arrays of 256)
    slot_refill(slot_table(slots), next_ids, unfinished, rows, (mgStream_t)stream);
    return MG_OK;
}

// the generator of sample_select on the host: out_host[4] = Philox4x32-10(key = seed, counter = (stream_id lo, stream_id hi, pos, 0))
int mgk_philox(uint64_t seed, uint64_t stream_id, uint32_t pos, uint32_t* out_host) {
    if (!out_host) return MG_E_ARG;
    philox4x32_10(seed, stream_id, pos, out_host);
    return MG_OK;
}

// The lm_head form of the fused greedy tail (gemm_rows_splitk with TopOut, KS = 1): P [M][ldp] logits (nullable: not written),
// ptop [M][ceil(N/32)] float4 partials, stopv [M][4]; stop token `eos` kept apart; lse = TopOut::lse
int mgk_lm_head_top(void* stream, const void* X_pk, const void* W_pk, float* P, int M, int N, int K, int ldp, void* ptop, float* stopv,
                    int eos, int lse) {
    if ((K & 63) || M > 256 || M < 1) return MG_E_SHAPE;
    RowScale rs{};
    TopOut top{(float4*)ptop, stopv, {eos, -1, -1, -1}, P ? 1 : 0, lse ? 1 : 0};
    gemm_rows_splitk((const uint16_t*)X_pk, (const uint16_t*)W_pk, P, M, N, K, ldp, 0, 1, rs, (mgStream_t)stream, &top);
    return MG_OK;
}

// lm_head with the log-softmax / argmax / gather epilogue (score_lm_head, k_score.hip): no logits; every output and `targets` nullable.
// The first int of scratch counts the targets >= N of the call.
size_t mgk_score_scratch_bytes(int M, int N) { return (M < 1 || N < 1) ? 0 : score_scratch_bytes(M, N); }
int mgk_score(void* stream, const void* X_pk, const void* W_pk, int M, int N, int K, const int64_t* targets, float* tok_lp, int64_t* arg_id,
              float* arg_lp, float* lse, void* scratch, size_t scratch_bytes) {
    if (!X_pk || !W_pk || !scratch) return MG_E_ARG;
    if (K < 64 || (K & 63) || M < 1 || N < 1) return MG_E_SHAPE;
    if (scratch_bytes < score_scratch_bytes(M, N)) return MG_E_WORKSPACE;
    const ScoreArgs a{(const uint16_t*)X_pk, (const uint16_t*)W_pk, M, N, K, targets, tok_lp, arg_id, arg_lp, lse, scratch};
    score_lm_head(a, (mgStream_t)stream);
    return MG_OK;
}

// Cross-attention attribution (xattn_map + xattn_map_gather, k_attrib.hip): one call = one layer's launch, then the gather into `map`
// [B][Sq][M_e1 + L + P] when map is non-null.  Sk = M_pad + L + P keys per image; scratch keeps the running sums between calls.
size_t mgk_xattn_map_scratch_bytes(int B, int Sq, int Sk) { return (B < 1 || Sq < 1 || Sk < 1) ? 0 : xattn_map_scratch_bytes(B, Sq, Sk); }
int mgk_xattn_map(void* stream, const void* Q, const void* K, int B, int H, int Sq, int Sq_cap, int Sk_cap, const uint8_t* kmask, int accumulate,
                  float scale, void* scratch, size_t scratch_bytes, int M_e1, int M_pad, int L, int P, const int* text_len, const uint8_t* qmask,
                  float* map) {
    if (!Q || !K || !scratch) return MG_E_ARG;
    if (B < 1 || H < 1 || Sq < 1 || M_e1 < 0 || M_pad < M_e1 || (M_pad & 63) || L < 0 || P < 0) return MG_E_SHAPE;
    const int Sk = M_pad + L + P;
    if (Sk < 1 || (Sq_cap & 31) || (Sk_cap & 63) || Sk > Sk_cap || Sq > Sq_cap) return MG_E_SHAPE;
    if (!xattn_map_supported(Sk)) return MG_E_UNSUPPORTED;
    if (scratch_bytes < xattn_map_scratch_bytes(B, Sq, Sk)) return MG_E_WORKSPACE;
    const XattnMapArgs a{(const uint16_t*)Q, (const uint16_t*)K, B, H, Sq, Sk, Sq_cap, Sk_cap, kmask, accumulate, scale, (float*)scratch};
    if (xattn_map(a, (mgStream_t)stream) != 0) return MG_E_UNSUPPORTED;
    if (map) xattn_map_gather(XattnGatherArgs{(const float*)scratch, map, B, Sq, Sk, M_e1, M_pad, L, P, text_len, qmask, Sq}, (mgStream_t)stream);
    return MG_OK;
}

// mgk_lm_head_top as the decode step launches it: the deferred row scale of the final norm and up to four stop tokens (host array, -1 = unused);
// ptop null: the plain projection (the unfused tail's launch)
int mgk_lm_head_step(void* stream, const void* X_pk, const void* W_pk, float* P, int M, int N, int K, int ldp, const float* rs_part, int rs_nparts,
                     float rs_inv_d, float rs_eps, void* ptop, float* stopv, const int* stop4_host, int write_logits, int lse) {
    if (!X_pk || !W_pk) return MG_E_ARG;
    if (K < 64 || (K & 63) || M > 256 || M < 1 || N < 1) return MG_E_SHAPE;
    if (rs_part && (rs_nparts < 8 || (rs_nparts & 7))) return MG_E_SHAPE;
    const bool writes = !ptop || write_logits;
    if (writes && (!P || ldp < N)) return MG_E_ARG;
    if (ptop && (!stopv || !stop4_host)) return MG_E_ARG;
    const RowScale rs{rs_part, rs_nparts, rs_inv_d, rs_eps};
    if (!ptop) {
        gemm_rows_splitk((const uint16_t*)X_pk, (const uint16_t*)W_pk, P, M, N, K, ldp, 0, 1, rs, (mgStream_t)stream);
        return MG_OK;
    }
    TopOut top{(float4*)ptop, stopv, {stop4_host[0], stop4_host[1], stop4_host[2], stop4_host[3]}, write_logits ? 1 : 0, lse ? 1 : 0};
    gemm_rows_splitk((const uint16_t*)X_pk, (const uint16_t*)W_pk, P, M, N, K, ldp, 0, 1, rs, (mgStream_t)stream, &top);
    return MG_OK;
}

// greedy_select_fused on lm_head partials (mgk_lm_head_top): selection, bookkeeping, optional token scores, and the next step's embedding
// + first RMSNorm of the selected token (tok_emb [V][d] bf16, gain [d], h [rows][d] fp32, x_pk packed bf16 [rows padded to 32][d])
int mgk_greedy_select_fused(void* stream, const void* ptop, const float* stopv, int rows, int V, int eos, int pad, int min_len,
                            int64_t* next_ids, int64_t* out_ids, int max_len, int pos, int* unfinished, int* n_unfinished, float* token_scores,
                            int ts_ld, const void* tok_emb, const float* gain, float* h, void* x_pk, int d, float eps) {
    if (d > 2048 || (d & 7)) return MG_E_SHAPE;
    ArgmaxArgs a{};
    a.rows = rows; a.V = V; a.ldl = (V + 31) / 32 * 32; a.eos = eos; a.pad = pad; a.min_len = min_len;
    a.next_ids = next_ids; a.out_ids = out_ids; a.max_len = max_len; a.pos = pos; a.unfinished = unfinished;
    a.n_unfinished = n_unfinished; a.token_scores = token_scores; a.ts_ld = ts_ld;
    a.ptop = (const float4*)ptop; a.stopv = stopv; a.ntiles = (V + 31) / 32;
    a.tok_emb = (const uint16_t*)tok_emb; a.gain = gain; a.h = h; a.x_pk = (uint16_t*)x_pk; a.d = d; a.eps = eps;
    mg_memset_async(n_unfinished, 0, sizeof(int), (mgStream_t)stream);
    greedy_select_fused(a, (mgStream_t)stream);
    return MG_OK;
}

// Beam-search step kernels (k_beam.hip) on caller-owned buffers, one launch sequence per call as decode_step (engine.hip) enqueues it.
// slot_pos / slot_live both null: batch form; both given: queue form (BeamSlots).
static bool beam_geometry_ok(int B, int K, int max_len) { return B >= 1 && K >= 2 && K <= 8 && B * K <= 1024 && max_len >= 2; }
size_t mgk_beam_state_bytes(int B, int K, int max_len) { return beam_geometry_ok(B, K, max_len) ? beam_state_bytes(B, K, max_len) : 0; }
float mgk_beam_length_divisor(int cur_len, float length_penalty) { return beam_length_divisor(cur_len, length_penalty); }
int mgk_beam_init(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc, int T_cap,
                  int* counters) {
    if (!beam_geometry_ok(B, K, max_len) || T_cap < max_len - 1) return MG_E_SHAPE;
    beam_init(state, B, K, max_len, pad, eos, start, next_ids, anc, T_cap, counters, (mgStream_t)stream);
    return MG_OK;
}
int mgk_beam_step(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len, const int* tdev,
                  const float* div_table, int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids, int* beam_idx,
                  int* counters, const int* slot_pos, const int* slot_live) {
    if (!beam_geometry_ok(B, K, max_len) || V < 2 * K || ldl < V || (!slot_pos != !slot_live)) return MG_E_SHAPE;
    if ((tdev || slot_pos) && !div_table) return MG_E_ARG;
    const BeamSlots bs{slot_pos, slot_live};
    beam_step(state, logits, ldl, V, B, K, max_len, cur_len, tdev, div_table, eos, min_len, length_penalty, early_stopping, next_ids, beam_idx,
              counters, (mgStream_t)stream, slot_pos ? &bs : nullptr);
    return MG_OK;
}
// mgk_beam_init / mgk_beam_step (batch form) under a decoder prompt: prompt_ids [B][prompt_ld], prompt_len [B] device; div_table
// [max_len + 1] is required (the per-image divisor index lives on the device)
int mgk_beam_init_prompted(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc,
                           int T_cap, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int V, int* bad) {
    if (!beam_geometry_ok(B, K, max_len) || T_cap < max_len - 1 || V < 2 * K) return MG_E_SHAPE;
    if (!prompt_ids || !prompt_len || prompt_ld < 1) return MG_E_ARG;
    const DecPrompt pr{prompt_ids, prompt_len, prompt_ld, 1, bad};
    beam_init(state, B, K, max_len, pad, eos, start, next_ids, anc, T_cap, counters, (mgStream_t)stream, &pr, V);
    return MG_OK;
}
int mgk_beam_step_prompted(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len, const int* tdev,
                           const float* div_table, int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids,
                           int* beam_idx, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld) {
    if (!beam_geometry_ok(B, K, max_len) || V < 2 * K || ldl < V) return MG_E_SHAPE;
    if (!div_table || !prompt_ids || !prompt_len || prompt_ld < 1) return MG_E_ARG;
    const DecPrompt pr{prompt_ids, prompt_len, prompt_ld, 1, nullptr};
    beam_step(state, logits, ldl, V, B, K, max_len, cur_len, tdev, div_table, eos, min_len, length_penalty, early_stopping, next_ids, beam_idx,
              counters, (mgStream_t)stream, nullptr, &pr);
    return MG_OK;
}
// mgk_beam_init_prompted / mgk_beam_step_prompted under a constraint (the prompt is optional: prompt_ids null).  start [B] device: the
// images' states at their first free columns; con->state [B * K] takes them at init and is reordered and advanced by every free step
int mgk_beam_init_constrained(void* stream, void* state, int B, int K, int max_len, int pad, int eos, int start, int64_t* next_ids, int* anc,
                              int T_cap, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld, int V, int* bad,
                              const mgk_constraint* con, const int* con_start) {
    if (!beam_geometry_ok(B, K, max_len) || T_cap < max_len - 1 || V < 2 * K) return MG_E_SHAPE;
    if (prompt_ids && (!prompt_len || prompt_ld < 1)) return MG_E_ARG;
    DecConstraint dc{};
    const int rc = dec_constraint(con, &dc);
    if (rc != MG_OK) return rc;
    if (!con_start) return MG_E_ARG;
    const DecPrompt pr{prompt_ids, prompt_len, prompt_ld, 1, bad};
    beam_init(state, B, K, max_len, pad, eos, start, next_ids, anc, T_cap, counters, (mgStream_t)stream, prompt_ids ? &pr : nullptr, V, dc.state,
              con_start);
    return MG_OK;
}
int mgk_beam_step_constrained(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, int cur_len,
                              const int* tdev, const float* div_table, int eos, int min_len, float length_penalty, int early_stopping,
                              int64_t* next_ids, int* beam_idx, int* counters, const int64_t* prompt_ids, const int* prompt_len, int prompt_ld,
                              const mgk_constraint* con) {
    if (!beam_geometry_ok(B, K, max_len) || V < 2 * K || ldl < V) return MG_E_SHAPE;
    if (!div_table || (prompt_ids && (!prompt_len || prompt_ld < 1))) return MG_E_ARG;
    DecConstraint dc{};
    const int rc = dec_constraint(con, &dc);
    if (rc != MG_OK) return rc;
    const DecPrompt pr{prompt_ids, prompt_len, prompt_ld, 1, nullptr};
    beam_step(state, logits, ldl, V, B, K, max_len, cur_len, tdev, div_table, eos, min_len, length_penalty, early_stopping, next_ids, beam_idx,
              counters, (mgStream_t)stream, nullptr, prompt_ids ? &pr : nullptr, &dc);
    return MG_OK;
}
// The beam queue under a decoder prompt and / or a constraint (mg_generate_stream_beam_constrained): mgk_beam_step in the queue form and
// mgk_beam_slots_step with mgk_queue_con - prompt and start state per image of the queue (slot_img [slots * K] names the image in a row's
// slot), con->state [slots * K] per slot row.  q NULL or empty: the plain operators.
int mgk_beam_step_queue_ex(void* stream, void* state, const float* logits, int ldl, int V, int B, int K, int max_len, const float* div_table,
                           int eos, int min_len, float length_penalty, int early_stopping, int64_t* next_ids, int* beam_idx, int* counters,
                           const int* slot_pos, const int* slot_live, const int* slot_img, const mgk_queue_con* q) {
    if (!beam_geometry_ok(B, K, max_len) || V < 2 * K || ldl < V) return MG_E_SHAPE;
    if (!slot_pos || !slot_live || !div_table) return MG_E_ARG;
    DecPrompt dp{};
    DecConstraint dc{};
    const int rc = queue_con(q, &dp, &dc);
    if (rc != MG_OK) return rc;
    if (dp.ids && !slot_img) return MG_E_ARG;
    const BeamSlots bs{slot_pos, slot_live, slot_img};
    beam_step(state, logits, ldl, V, B, K, max_len, 0, nullptr, div_table, eos, min_len, length_penalty, early_stopping, next_ids, beam_idx,
              counters, (mgStream_t)stream, &bs, dp.ids ? &dp : nullptr, dc.cls ? &dc : nullptr);
    return MG_OK;
}
int mgk_beam_slots_step_ex(void* stream, void* state, int slots, int K, int max_len, int pad, int eos, int start, int early_stopping, int* pos,
                           int* img, int* pool, int* bpool, int* live, int* assign, int64_t* next_ids, int* anc, int T_cap, int pool_cap,
                           int64_t* out_ids, int* out_len, float* out_scores, int* ctr, int end_first, int num_return, int* beam_indices,
                           float* token_scores, const mgk_queue_con* q) {
    if (!beam_geometry_ok(slots, K, max_len) || T_cap < max_len - 1 || pool_cap < 1 || num_return < 1 || num_return > K) return MG_E_SHAPE;
    DecPrompt dp{};
    DecConstraint dc{};
    const int rc = queue_con(q, &dp, &dc);
    if (rc != MG_OK) return rc;
    if (dc.cls && !q->con_start) return MG_E_ARG;
    const BeamOut nb{num_return, beam_indices, token_scores};
    beam_slots_step(state, slots, K, max_len, pad, eos, start, early_stopping, pos, img, pool, bpool, live, assign, next_ids, anc, T_cap, pool_cap,
                    out_ids, out_len, out_scores, ctr, end_first != 0, (mgStream_t)stream, &nb, dp.ids ? &dp : nullptr, q ? q->V : 0,
                    dc.cls ? dc.state : nullptr, dc.cls ? q->con_start : nullptr);
    return MG_OK;
}
int mgk_beam_reorder_anc(void* stream, int* anc, const int* beam_idx, int rows, int t_written, const int* tdev, const int* counters,
                         const int* slot_pos, const int* slot_live) {
    if (rows < 1 || rows > 1024 || t_written < 1 || (!slot_pos != !slot_live)) return MG_E_SHAPE;
    const BeamSlots bs{slot_pos, slot_live};
    beam_reorder_anc(anc, beam_idx, rows, t_written, tdev, counters, (mgStream_t)stream, slot_pos ? &bs : nullptr);
    return MG_OK;
}
int mgk_beam_finalize(void* stream, void* state, int B, int K, int max_len, int64_t* out_ids, int* out_cols, float* out_scores, int num_return,
                      int* beam_indices, float* token_scores) {
    if (!beam_geometry_ok(B, K, max_len) || num_return < 1 || num_return > K) return MG_E_SHAPE;
    const BeamOut nb{num_return, beam_indices, token_scores};
    beam_finalize(state, B, K, max_len, out_ids, out_cols, out_scores, (mgStream_t)stream, &nb);
    return MG_OK;
}
int mgk_beam_slots_step(void* stream, void* state, int slots, int K, int max_len, int pad, int eos, int start, int early_stopping, int* pos,
                        int* img, int* pool, int* bpool, int* live, int* assign, int64_t* next_ids, int* anc, int T_cap, int pool_cap,
                        int64_t* out_ids, int* out_len, float* out_scores, int* ctr, int end_first, int num_return, int* beam_indices,
                        float* token_scores) {
    if (!beam_geometry_ok(slots, K, max_len) || T_cap < max_len - 1 || pool_cap < 1 || num_return < 1 || num_return > K) return MG_E_SHAPE;
    const BeamOut nb{num_return, beam_indices, token_scores};
    beam_slots_step(state, slots, K, max_len, pad, eos, start, early_stopping, pos, img, pool, bpool, live, assign, next_ids, anc, T_cap, pool_cap,
                    out_ids, out_len, out_scores, ctr, end_first != 0, (mgStream_t)stream, &nb);
    return MG_OK;
}

int mgk_gemm_splitk(void* stream, const void* X_pk, const void* W_pk, float* P, int M, int N, int K, int ldp,
                    size_t slab_stride, int KS) {
    if ((K & 63) || KS < 1 || KS > 16 || M > 256) return MG_E_SHAPE;
    RowScale rs{};
    gemm_rows_splitk((const uint16_t*)X_pk, (const uint16_t*)W_pk, P, M, N, K, ldp, slab_stride, KS, rs, (mgStream_t)stream);
    return MG_OK;
}
int mgk_splitk_factor(int N, int K) { return splitk_factor(N, K); }
int mgk_gemm_set_variant(int v) { gemm_set_variant(v); return MG_OK; }

// true when a row scale / a column window / a k-tile window is one the decode-step kernels can take
static bool rs_ok(const float* part, int nparts) { return !part || (nparts >= 8 && (nparts & 7) == 0); }      // (8 threads share a row's partial sums)
static bool kwin_ok(int x_kts, int x_k0, int K) { return x_kts ? (x_k0 >= 0 && x_k0 + (K >> 4) <= x_kts) : x_k0 == 0; }
static bool cwin_ok(int ld, int col0, int N) { return ld ? ((ld & 15) == 0 && col0 >= 0 && (col0 & 7) == 0 && col0 + N <= ld) : col0 == 0; }
static int resid_args(const mgk_resid_desc* d, ResidArgs& r) {
    if (!d || !d->X || !d->W || !d->h || !d->part) return MG_E_ARG;
    if (d->K < 64 || (d->K & 63) || d->N < 32 || (d->N & 31) || d->M < 1 || d->M > 256) return MG_E_SHAPE;
    if (d->x_pk && !d->gain) return MG_E_ARG;
    if (!kwin_ok(d->x_kts, d->x_k0, d->K) || !cwin_ok(d->x_ld, d->x_col0, d->N) || !cwin_ok(d->x2_ld, d->x2_col0, d->N)) return MG_E_SHAPE;
    if (!rs_ok(d->rs_part, d->rs_nparts) || d->wide_tiles < 0 || d->wide_tiles > 8 || (!d->kpart != !d->ticket)) return MG_E_SHAPE;
    r.X = (const uint16_t*)d->X; r.x_kts = d->x_kts; r.x_k0 = d->x_k0; r.W = (const uint16_t*)d->W; r.h = d->h; r.gain = d->gain; r.gscale = d->gscale;
    r.x_pk = (uint16_t*)d->x_pk; r.x_ld = d->x_ld; r.x_col0 = d->x_col0; r.x2_pk = (uint16_t*)d->x2_pk; r.x2_ld = d->x2_ld; r.x2_col0 = d->x2_col0;
    r.part = d->part; r.M = d->M; r.N = d->N; r.K = d->K; r.rs = RowScale{d->rs_part, d->rs_nparts, d->rs_inv_d, d->rs_eps};
    r.alone = d->alone; r.wide_tiles = d->wide_tiles; r.kpart = d->kpart; r.ticket = d->ticket;
    return MG_OK;
}
int mgk_gemm_resid_ex(void* stream, const mgk_resid_desc* d) {
    ResidArgs r{};
    if (const int rc = resid_args(d, r)) return rc;
    gemm_rows_resid(r, (mgStream_t)stream);
    return MG_OK;
}
int mgk_gemm_pair_ex(void* stream, const mgk_resid_desc* d, const mgk_proj_desc* p, int epi) {
    ResidArgs r{};
    if (const int rc = resid_args(d, r)) return rc;
    if (!p || !p->X || !p->W) return MG_E_ARG;
    if (epi != EPI_HEADS && epi != EPI_PK_RELU && epi != EPI_F32_STORE) return MG_E_UNSUPPORTED;
    if (r.kpart) return MG_E_ARG;                                        // (the pair launch has no K-slab form)
    if (p->K < 64 || (p->K & 63) || p->N < 16 || (p->N & 15) || !kwin_ok(p->x_kts, p->x_k0, p->K) || !rs_ok(p->rs_part, p->rs_nparts)) return MG_E_SHAPE;
    GemmArgs g{};
    g.X = (const uint16_t*)p->X; g.x_kts = p->x_kts; g.x_k0 = p->x_k0; g.W = (const uint16_t*)p->W; g.M = r.M; g.N = p->N; g.K = p->K;
    g.rs = RowScale{p->rs_part, p->rs_nparts, p->rs_inv_d, p->rs_eps}; g.both_halves = p->both_halves;
    if (epi == EPI_HEADS) {
        if (!p->q) return MG_E_ARG;
        if (p->N & 63) return MG_E_SHAPE;
        g.heads.ptr[0] = (uint16_t*)p->q; g.heads.fmt[0] = HF_STEP_Q; g.heads.inner = p->N; g.heads.H = p->N >> 6; g.heads.S_in = r.M;
    } else if (epi == EPI_PK_RELU) {
        if (!p->out_pk) return MG_E_ARG;
        g.out_pk = (uint16_t*)p->out_pk;
    } else {
        if (!p->out_f32) return MG_E_ARG;
        if (p->ldo < p->N || (p->ldo & 3)) return MG_E_SHAPE;
        g.out_f32 = p->out_f32; g.ldo = p->ldo;
    }
    gemm_rows_pair(r, g, epi, (mgStream_t)stream);
    return MG_OK;
}

int mgk_gemm_resid(void* stream, const void* X_pk, const void* W_pk, float* h, const float* gain, float gscale, void* x_pk,
                   float* part, int M, int N, int K, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps) {
    return mgk_gemm_resid_mt(stream, X_pk, W_pk, h, gain, gscale, x_pk, part, M, N, K, rs_part, rs_nparts, rs_inv_d, rs_eps, 0, nullptr, nullptr);
}

int mgk_gemm_resid_mt(void* stream, const void* X_pk, const void* W_pk, float* h, const float* gain, float gscale, void* x_pk,
                      float* part, int M, int N, int K, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, int wide_tiles,
                      float* kpart, int* ticket) {
    if ((K & 63) || (N & 31) || M > 256) return MG_E_SHAPE;
    ResidArgs r{};
    r.X = (const uint16_t*)X_pk; r.W = (const uint16_t*)W_pk; r.h = h; r.gain = gain; r.gscale = gscale; r.x_pk = (uint16_t*)x_pk;
    r.part = part; r.M = M; r.N = N; r.K = K; r.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps};
    r.wide_tiles = wide_tiles; r.kpart = kpart; r.ticket = ticket;
    gemm_rows_resid(r, (mgStream_t)stream);
    return MG_OK;
}
int mgk_set_rows_mt(int on) { gemm_rows_set_mt(on); return MG_OK; }
int mgk_set_attention_qt(int qt) { attention_set_qt(qt); return MG_OK; }
int mgk_set_pp_parts(int mode) { gemm_pp_set_parts(mode); return MG_OK; }
int mgk_set_pp_groups(int cap) { gemm_pp_set_groups(cap); return MG_OK; }

// The tiled gemm() with everything its call sites set (test entry; include/mgrapher.h).  Every check comes before any device work.
int mgk_gemm_ex(void* stream, const mgk_gemm_desc* d, int epi) {
    if (!d || !d->X || !d->W) return MG_E_ARG;
    if (d->M < 1 || d->N < 1 || d->K < 64 || (d->K & 63)) return MG_E_SHAPE;
    if (epi != EPI_F32_STORE && epi != EPI_F32_RESID && epi != EPI_PK_RELU && epi != EPI_PK && epi != EPI_HEADS && epi != EPI_RESID_NORM)
        return MG_E_UNSUPPORTED;
    const bool scaled = epi == EPI_PK_RELU || epi == EPI_PK || epi == EPI_HEADS;
    if (d->rs_part && !scaled) return MG_E_UNSUPPORTED;
    if (d->rs_part && (d->rs_nparts < 4 || (d->rs_nparts & 3))) return MG_E_SHAPE;
    if ((d->row_mask && !d->list_scratch) || ((uintptr_t)d->row_mask & 15)) return MG_E_ARG;
    if (d->list_scratch && (d->M & 31)) return MG_E_SHAPE;
    GemmArgs a{};
    a.X = (const uint16_t*)d->X; a.W = (const uint16_t*)d->W; a.M = d->M; a.N = d->N; a.K = d->K;
    a.rs = RowScale{d->rs_part, d->rs_nparts, d->rs_inv_d, d->rs_eps};
    if (epi == EPI_F32_STORE || epi == EPI_F32_RESID) {
        if (!d->out_f32) return MG_E_ARG;
        if (d->ldo < d->N) return MG_E_SHAPE;
        a.out_f32 = d->out_f32; a.ldo = d->ldo; a.bias = d->bias;
    } else if (epi == EPI_PK_RELU || epi == EPI_PK) {
        if (!d->out_pk) return MG_E_ARG;
        if (d->N & 15) return MG_E_SHAPE;
        a.out_pk = (uint16_t*)d->out_pk;
    } else if (epi == EPI_RESID_NORM) {
        if (!d->out_f32 || (d->gain && !d->out_pk)) return MG_E_ARG;
        if ((d->N & 31) || ((d->M & 31) && (d->gain || d->out_pk || d->part)) || (d->part && d->ldo < (d->N + 63) / 64)) return MG_E_SHAPE;
        a.out_f32 = d->out_f32; a.gain = d->gain; a.out_pk = (uint16_t*)d->out_pk; a.part = d->part; a.ldo = d->ldo;
    } else {
        if (d->H < 1 || (d->N % (d->H * 64)) || d->N > 3 * d->H * 64 || d->S_in < 1 || d->S_cap < 1) return MG_E_SHAPE;
        if (d->s_off < 0 || (d->s_off & 31) || d->s_off + d->S_in > d->S_cap) return MG_E_SHAPE;
        for (int i = 0; i < 3; ++i) {
            const int f = d->head_fmt[i];
            if (f != HF_NONE && f != HF_PK_ROWS && f != HF_PK_T && f != HF_NATURAL) return MG_E_UNSUPPORTED;
            if (i < d->N / (d->H * 64) && f != HF_NONE && !d->head_ptr[i]) return MG_E_ARG;
            if ((f == HF_PK_ROWS || f == HF_PK_T) && ((d->S_cap & 31) || (d->S_in & 31))) return MG_E_SHAPE;
            if (f == HF_NATURAL && d->s_off) return MG_E_SHAPE;
            a.heads.ptr[i] = (uint16_t*)d->head_ptr[i]; a.heads.fmt[i] = f;
        }
        a.heads.inner = d->H * 64; a.heads.H = d->H; a.heads.S_in = d->S_in; a.heads.S_cap = d->S_cap; a.heads.s_off = d->s_off;
        a.heads.row_map = d->row_map;
    }
    if (d->row_mask) row_tile_list(d->row_mask, d->M, d->list_scratch + 1, d->list_scratch, (mgStream_t)stream);
    if (d->list_scratch) { a.row_tiles = d->list_scratch + 1; a.n_row_tiles = d->list_scratch; }      // (row_mask null: the caller's own list)
    gemm(a, epi, (mgStream_t)stream);
    return MG_OK;
}

#ifdef MG_TOOLS
int mgk_gemm_resid_trace(void* stream, const void* X_pk, const void* W_pk, float* h, const float* gain, void* x_pk, float* part, int N,
                         int K, const float* rs_part, long long* trace) {
    ResidArgs r{};
    r.X = (const uint16_t*)X_pk; r.W = (const uint16_t*)W_pk; r.h = h; r.gain = gain; r.gscale = 1.0f; r.x_pk = (uint16_t*)x_pk;
    r.part = part; r.M = 32; r.N = N; r.K = K; r.rs = RowScale{rs_part, N / 8, 1.0f / (float)N, 1e-6f};
    gemm_rows_resid_trace(r, trace, (mgStream_t)stream);
    return MG_OK;
}
#endif

int mgk_gemm_pair(void* stream, const void* Wn_pk, const void* Wr_pk, const float* gain, int N2, int d, int inner, void* W2_pk,
                  float* scratch_f32, const void* xwin_pk, float* h, void* hb_out_pk, float* part, void* out2_pk, int M, int relu) {
    if ((d & 63) || (inner & 63) || (N2 & 31) || M > 256) return MG_E_SHAPE;
    mgStream_t st = (mgStream_t)stream;
    const int K2 = d + inner;
    float *A = scratch_f32, *Bm = A + (size_t)N2 * d, *Cm = Bm + (size_t)d * inner;
    unpack_weight((const uint16_t*)Wr_pk, Bm, d, inner, st);
    unpack_weight((const uint16_t*)Wn_pk, A, N2, d, st);
    scale_cols_f32(A, gain, Cm, N2, d, K2, st);
    gemm_f32_scaled(A, gain, Bm, Cm + d, N2, d, inner, K2, st);
    pack_weight(Cm, 0, N2, K2, (uint16_t*)W2_pk, N2, st);
    ResidArgs r{};
    r.X = (const uint16_t*)xwin_pk; r.x_kts = K2 >> 4; r.x_k0 = d >> 4; r.W = (const uint16_t*)Wr_pk; r.h = h;
    r.x2_pk = (uint16_t*)hb_out_pk; r.part = part; r.M = M; r.N = d; r.K = inner;
    GemmArgs g{};
    g.X = (const uint16_t*)xwin_pk; g.W = (const uint16_t*)W2_pk; g.M = M; g.N = N2; g.K = K2; g.out_pk = (uint16_t*)out2_pk;
    if (!relu) {                             // the per-head form: out2_pk = q [M][N2 / 64][64] bf16 (N2 = H * 64)
        if (N2 & 63) return MG_E_SHAPE;
        g.out_pk = nullptr;
        g.heads.ptr[0] = (uint16_t*)out2_pk; g.heads.fmt[0] = HF_STEP_Q; g.heads.inner = N2; g.heads.H = N2 >> 6; g.heads.S_in = M;
    }
    gemm_rows_pair(r, g, relu ? EPI_PK_RELU : EPI_HEADS, st);
    return MG_OK;
}

int mgk_add_norm_pack(void* stream, float* h, const float* P, int KS, int ldp, size_t slab_stride, const float* gain,
                      void* x_pk, int M, int d, float eps, float scale) {
    if ((d & 15) || d > 4096 || KS < 0 || KS > 16) return MG_E_SHAPE;
    Slabs sl; sl.P = P; sl.KS = KS; sl.ldp = ldp; sl.stride = slab_stride;
    add_norm_pack(h, sl, gain, (uint16_t*)x_pk, M, d, eps, scale, (mgStream_t)stream);
    return MG_OK;
}

int mgk_relu_pack(void* stream, const float* P, int KS, int ldp, size_t slab_stride, void* y_pk, int M, int N) {
    if ((N & 15) || KS < 1 || KS > 16) return MG_E_SHAPE;
    Slabs sl; sl.P = P; sl.KS = KS; sl.ldp = ldp; sl.stride = slab_stride;
    relu_pack(sl, (uint16_t*)y_pk, M, N, (mgStream_t)stream);
    return MG_OK;
}

// ---- kernels of the OCSR vision branch (k_swin.hip; test entries) ----
int mgk_swin_attention(void* stream, const void* qkv_pk, void* ctx_pk, const float* table_HT, int B, int R, int C, int H, int w, int shift) {
    if (B < 1 || R < 1 || H < 1 || !qkv_pk || !ctx_pk || !table_HT) return MG_E_SHAPE;
    if (!swin_attention_supported(w, R, C, H)) return MG_E_UNSUPPORTED;
    if (shift < 0 || shift >= w) return MG_E_SHAPE;
    SwinAttnArgs a{};
    a.qkv = (const uint16_t*)qkv_pk; a.ctx = (uint16_t*)ctx_pk; a.table = table_HT;
    a.B = B; a.R = R; a.C = C; a.H = H; a.w = w; a.shift = shift;
    swin_attention(a, (mgStream_t)stream);
    return MG_OK;
}

int mgk_swin_layernorm(void* stream, const float* h_in, int in_tiled, float* h_out, int h_out_norm, const float* w, const float* b,
                       const float* add_bias, void* x_pk, float* out_f32, int M, int C, int merge_R, float eps, int kaug) {
    if (!(swin_ln_supported(C) || C == 768)) return MG_E_UNSUPPORTED;      // (the launcher has no case of its own for any other width)
    if (M < 1 || !h_in || !w || !b || merge_R < 0 || (merge_R & 1)) return MG_E_SHAPE;
    if (kaug && ((kaug & 15) || kaug < C)) return MG_E_SHAPE;
    if (merge_R) {                     // the gather reads the TILED map of width C / 4; whole images; not in place
        const int P = (merge_R >> 1) * (merge_R >> 1);
        if (!in_tiled || (C & 15) || M % P || h_out == h_in) return MG_E_SHAPE;
    }
    if (h_out == h_in && !in_tiled) return MG_E_SHAPE;
    SwinLnArgs a{};
    a.h_in = h_in; a.in_tiled = in_tiled; a.h_out = h_out; a.h_out_norm = h_out_norm; a.w = w; a.b = b; a.add_bias = add_bias;
    a.x_pk = (uint16_t*)x_pk; a.out_f32 = out_f32; a.M = M; a.C = C; a.merge_R = merge_R; a.eps = eps; a.kaug = kaug;
    swin_layernorm(a, (mgStream_t)stream);
    return MG_OK;
}

int mgk_swin_resize(void* stream, const float* src, float* dst, int B, int C, int S, int I, const float* scale_host, const float* shift_host) {
    if (B < 1 || C < 1 || C > 4 || S < 1 || I < 1 || !src || !dst || !scale_host || !shift_host) return MG_E_SHAPE;
    SwinPixAffine af{};
    for (int c = 0; c < 4; ++c) { af.scale[c] = c < C ? scale_host[c] : 1.0f; af.shift[c] = c < C ? shift_host[c] : 0.0f; }
    swin_resize(src, dst, B, C, S, I, af, (mgStream_t)stream);
    return MG_OK;
}

int mgk_swin_im2col_pack(void* stream, const float* pix, void* x_pk, int B, int C, int I, int ps, int Kp) {
    if (B < 1 || C < 1 || ps < 1 || I < ps || (I % ps) || (Kp & 15) || Kp < C * ps * ps || !pix || !x_pk) return MG_E_SHAPE;
    swin_im2col_pack(pix, (uint16_t*)x_pk, B, C, I, ps, Kp, (mgStream_t)stream);
    return MG_OK;
}

int mgk_swin_transpose(void* stream, const float* src, float* dst, int n, int H) {
    if (n < 1 || H < 1 || !src || !dst || src == dst) return MG_E_SHAPE;
    swin_transpose_f32(src, dst, n, H, (mgStream_t)stream);
    return MG_OK;
}

// ---- kernels of the ChemicalOCR stage (k_ocr.hip and the decode-step kernels it starts from; test entries) ----
// The launchers check nothing: what each assumes about its arguments is refused here.
int mgk_ocr_layernorm_pack(void* stream, float* h, const float* w, const float* b, const float* add_bias, void* x_pk, float* out_f32, int M,
                           int d, int Kaug, float eps) {
    if (M < 1 || d < 1 || !h || !w || !b || (!x_pk && !out_f32 && !add_bias)) return MG_E_SHAPE;
    if (Kaug < d || (x_pk && (Kaug & 15))) return MG_E_SHAPE;
    ocr_layernorm_pack(h, w, b, add_bias, (uint16_t*)x_pk, out_f32, M, d, Kaug, eps, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_gelu_pack(void* stream, const float* in, void* y_pk, int M, int N, int Kaug) {
    if (M < 1 || N < 1 || !in || !y_pk || (Kaug & 15) || Kaug < N) return MG_E_SHAPE;
    ocr_gelu_pack(in, (uint16_t*)y_pk, M, N, Kaug, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_silu_mul_pack(void* stream, const float* in, void* y_pk, int M, int I) {
    if (M < 1 || I < 16 || (I & 15) || !in || !y_pk) return MG_E_SHAPE;
    ocr_silu_mul_pack(in, (uint16_t*)y_pk, M, I, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_silu_mul_rows(void* stream, const float* in, const float* rs_part, int rs_nparts, float rs_inv_d, float rs_eps, void* y_pk, int M,
                          int I) {
    if (M < 1 || I < 16 || (I & 15) || !in || !y_pk || (rs_part && rs_nparts < 1)) return MG_E_SHAPE;
    ocr_silu_mul_rows(in, RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps}, (uint16_t*)y_pk, M, I, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_add_pos(void* stream, const float* patch, const void* pos, const int* pos_ids, const uint8_t* patch_mask, uint8_t* vmask,
                    float* hidden, int N, int P, int P_cap, int d) {
    if (N < 1 || P < 1 || P > P_cap || d < 1 || !patch || !pos || !hidden) return MG_E_SHAPE;
    ocr_add_pos(patch, (const uint16_t*)pos, pos_ids, patch_mask, vmask, hidden, N, P, P_cap, d, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_pixel_shuffle_pack(void* stream, const float* vis, void* x_pk, int N, int g, int P_cap, int e, int sf) {
    if (N < 1 || sf < 1 || g < sf || (g % sf) || e < 1 || !vis || !x_pk) return MG_E_SHAPE;
    if (P_cap < g * g || ((e * sf * sf) & 15)) return MG_E_SHAPE;
    ocr_pixel_shuffle_pack(vis, (uint16_t*)x_pk, N, g, P_cap, e, sf, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_merge_embed(void* stream, const int64_t* ids, const void* tok_emb, const float* feats, float* h, int B, int L, int T_cap, int d,
                        int V, int image_token, int per_seq, int* err) {
    if (B < 1 || L < 1 || T_cap < L || d < 1 || V < 1 || per_seq < 0 || !ids || !tok_emb || !h || !err) return MG_E_SHAPE;
    if (L > 2048) return MG_E_UNSUPPORTED;       // the kernel's rank table
    ocr_merge_embed(ids, (const uint16_t*)tok_emb, feats, h, B, L, T_cap, d, V, image_token, per_seq, err, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_rope_heads(void* stream, const float* qkv, int B, int T, int T_cap, int H, int KV, float theta, void* Q, void* K, void* Vt, void* Kc,
                       void* Vc, int cap) {
    if (B < 1 || T < 1 || T > T_cap || (T_cap & 31) || H < 1 || KV < 1 || cap < T || !(theta > 0.f)) return MG_E_SHAPE;
    if (!qkv || !Q || !K || !Vt || !Kc || !Vc) return MG_E_SHAPE;
    if (H % KV) return MG_E_UNSUPPORTED;         // whole groups of query heads per key/value head
    ocr_rope_heads(qkv, B, T, T_cap, H, KV, theta, (uint16_t*)Q, (uint16_t*)K, (uint16_t*)Vt, (uint16_t*)Kc, (uint16_t*)Vc, cap, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_rope_table(void* stream, float* cs, int positions, float theta) {
    if (positions < 1 || !cs || !(theta > 0.f)) return MG_E_SHAPE;
    ocr_rope_table(cs, positions, theta, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_pack_aug(void* stream, const float* W, const float* bias, float scale, void* dst_pk, int row0, int N, int K, int Kaug, int Nfill,
                     int rstride) {
    if (N < 1 || K < 1 || Nfill < N || row0 < 0 || rstride < 1 || !W || !dst_pk) return MG_E_SHAPE;
    if ((Kaug & 15) || Kaug < K + (bias ? 1 : 0)) return MG_E_SHAPE;
    ocr_pack_aug(W, bias, scale, (uint16_t*)dst_pk, row0, N, K, Kaug, Nfill, rstride, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_tile_f32(void* stream, const float* src, float* dst, int M, int d, int to_tiled) {
    if (M < 32 || (M & 31) || d < 4 || (d & 3) || !src || !dst || src == dst) return MG_E_SHAPE;
    ocr_tile_f32(src, dst, M, d, to_tiled, (mgStream_t)stream);
    return MG_OK;
}
int mgk_ocr_row_maps(void* stream, int* last_rows, int* all_rows, uint8_t* key_mask, int B, int T, int T_cap, const int* lens) {
    if (B < 1 || T < 1 || T > T_cap || !last_rows || !all_rows || !key_mask) return MG_E_SHAPE;
    ocr_row_maps(last_rows, all_rows, key_mask, B, T, T_cap, (mgStream_t)stream, lens);
    return MG_OK;
}
int mgk_ocr_len_delta(void* stream, const int* lens, int* delta, int N, int L, int* err) {
    if (N < 1 || L < 1 || !lens || !delta || !err) return MG_E_SHAPE;
    ocr_len_delta(lens, delta, N, L, err, (mgStream_t)stream);
    return MG_OK;
}
// The gate / up projection of the ChemicalOCR decode step: gemm_rows with EPI_PK_SWIGLU.  W_pk packed [N padded to 32][K], rows gate_0, up_0,
// gate_1, ...; X_pk a packed buffer of x_kts 16-wide k-tiles per row tile read from k-tile x_k0 on (x_kts = 0: K / 16 and x_k0 = 0); the row
// scale as in mgk_gemm_norm; out_pk packed [M padded to 32][out_ld], written at columns [out_col0, out_col0 + N / 2) (out_ld = 0: N / 2 wide)
int mgk_gemm_swiglu(void* stream, const void* X_pk, int x_kts, int x_k0, const void* W_pk, int M, int N, int K, const float* rs_part,
                    int rs_nparts, float rs_inv_d, float rs_eps, void* out_pk, int out_ld, int out_col0) {
    if (!X_pk || !W_pk || !out_pk || K < 64 || (K & 63) || N < 16 || (N & 15) || M < 1) return MG_E_SHAPE;
    if (M > 256) return MG_E_UNSUPPORTED;        // 8 row tiles: beyond them gemm_rows hands over to the tiled kernel, which has no such epilogue
    if (x_kts ? (x_k0 < 0 || x_k0 + (K >> 4) > x_kts) : x_k0 != 0) return MG_E_SHAPE;
    if (out_ld ? ((out_ld & 15) || out_col0 < 0 || (out_col0 & 3) || out_col0 + (N >> 1) > out_ld) : (out_col0 != 0 || (N & 31))) return MG_E_SHAPE;
    if (rs_part && (rs_nparts < 8 || (rs_nparts & 7))) return MG_E_SHAPE;      // (8 threads of the kernel share a row's partial sums)
    GemmArgs a{};
    a.X = (const uint16_t*)X_pk; a.x_kts = x_kts; a.x_k0 = x_k0; a.W = (const uint16_t*)W_pk; a.M = M; a.N = N; a.K = K;
    a.rs = RowScale{rs_part, rs_nparts, rs_inv_d, rs_eps};
    a.out_pk = (uint16_t*)out_pk; a.out_ld = out_ld; a.out_col0 = out_col0;
    gemm_rows(a, EPI_PK_SWIGLU, (mgStream_t)stream);
    return MG_OK;
}
int mgk_rmsnorm_pack_tiled(void* stream, const float* h_tiled, const float* gain, void* x_pk, float* out_f32, int M, int d, float eps) {
    if (M < 32 || (M & 31) || d < 16 || (d & 15) || !h_tiled || !gain || (!x_pk && !out_f32)) return MG_E_SHAPE;
    rmsnorm_pack_tiled(h_tiled, gain, (uint16_t*)x_pk, out_f32, M, d, eps, (mgStream_t)stream);
    return MG_OK;
}
int mgk_embed_norm_rows(void* stream, const int64_t* ids, const void* tok_emb, float* h, const float* gain, void* x_pk, void* x2_pk, int x2_ld,
                        int x2_col0, int rows, int d, int V, int* err, float eps) {
    if (rows < 1 || d < 16 || (d & 15) || V < 1 || !ids || !tok_emb || !h || !gain || !x_pk || !err) return MG_E_SHAPE;
    if (x2_pk && ((x2_ld & 15) || x2_col0 < 0 || (x2_col0 & 7) || x2_col0 + d > x2_ld)) return MG_E_SHAPE;
    embed_norm_rows(ids, (const uint16_t*)tok_emb, h, gain, (uint16_t*)x_pk, (uint16_t*)x2_pk, x2_ld, x2_col0, rows, d, V, err, eps,
                    (mgStream_t)stream);
    return MG_OK;
}

// ---- the encoder's input assembly, index tables and output copies in every form mg_encode runs them (test entries; include/mgrapher.h) ----
// The launchers check nothing: what each assumes about its arguments is refused here, before any device work.
int mgk_embed_assemble_ex(void* stream, const mgk_embed_desc* e) {
    if (!e || !e->meta_ws || !e->input_ids || !e->bbox || !e->patch_emb || !e->tok_emb || !e->x_emb || !e->y_emb) return MG_E_ARG;
    if (!e->hidden || !e->cx || !e->cy || !e->mask || !e->xrow || !e->xlen || !e->err) return MG_E_ARG;
    if (e->B < 1 || e->L < 1 || e->n_side < 1 || e->n_side > 256 || e->M2 < 1 || e->V < 1 || e->d < 4) return MG_E_SHAPE;
    if (e->P != e->n_side * e->n_side || e->S_cap < e->L + e->P || (e->d & 3) || e->x_row0 < 0) return MG_E_SHAPE;
    if (e->hidden_tiled && (e->S_cap & 31)) return MG_E_SHAPE;
    EmbedArgs a{};
    a.input_ids = e->input_ids; a.bbox = e->bbox; a.attn_mask = e->attention_mask; a.patch_emb = e->patch_emb;
    a.tok_emb = (const uint16_t*)e->tok_emb; a.x_emb = (const uint16_t*)e->x_emb; a.y_emb = (const uint16_t*)e->y_emb;
    a.B = e->B; a.L = e->L; a.P = e->P; a.d = e->d; a.n_side = e->n_side; a.M2 = e->M2; a.V = e->V; a.S_cap = e->S_cap;
    a.hidden = e->hidden; a.hidden_tiled = e->hidden_tiled ? 1 : 0; a.cx = e->cx; a.cy = e->cy; a.mask = e->mask; a.xrow = e->xrow;
    a.xlen = e->xlen; a.x_row0 = e->x_row0; a.trim_padding = e->trim_padding ? 1 : 0; a.text_len = e->text_len; a.err = e->err;
    embed_assemble(a, e->meta_ws, (mgStream_t)stream);
    return MG_OK;
}
int mgk_bias_index(void* stream, void* out, const double* cx, const double* cy, const uint8_t* kmask, const int* bk1, const int* bkhv, int B,
                   int Sk, int S_cap) {
    if (!out || !cx || !cy || !bkhv) return MG_E_ARG;                    // (bk1 belongs to the launcher's signature; the kernel does not read it)
    if (B < 1 || S_cap < 64 || (S_cap & 63) || Sk < 0 || Sk > S_cap) return MG_E_SHAPE;
    bias_index((uint16_t*)out, cx, cy, kmask, bk1, bkhv, B, Sk, S_cap, (mgStream_t)stream);
    return MG_OK;
}
int mgk_attn_lists(void* stream, const uint8_t* kmask, int B, int Sk, int S_cap, int* kst, uint8_t* qbv) {
    if (!kmask || !kst || !qbv) return MG_E_ARG;
    if (B < 1 || S_cap < 64 || (S_cap & 63) || Sk < 0 || Sk > S_cap) return MG_E_SHAPE;
    attn_lists(kmask, B, Sk, S_cap, kst, qbv, (mgStream_t)stream);
    return MG_OK;
}
int mgk_row_tile_list(void* stream, const uint8_t* kmask, int rows, int* list, int* count) {
    if (!kmask || !list || !count || ((uintptr_t)kmask & 15)) return MG_E_ARG;
    if (rows < 32 || (rows & 31)) return MG_E_SHAPE;
    row_tile_list(kmask, rows, list, count, (mgStream_t)stream);
    return MG_OK;
}
int mgk_pack_e1(void* stream, const float* e1, int B, int M, int M_pad, int d, void* e1_pk, int* row_map, const uint8_t* enc_mask, int S_cap,
                uint8_t* xmask) {
    if (!e1 || !e1_pk || !row_map || (xmask && !enc_mask)) return MG_E_ARG;
    if (B < 1 || M < 1 || M_pad < M || (M_pad & 31) || d < 16 || (d & 15)) return MG_E_SHAPE;
    if (S_cap < 0 || (S_cap & 63) || (xmask && S_cap < 64)) return MG_E_SHAPE;
    pack_e1(e1, B, M, M_pad, d, (uint16_t*)e1_pk, row_map, enc_mask, S_cap, xmask, (mgStream_t)stream);
    return MG_OK;
}
int mgk_enc_copy_out(void* stream, const float* enc_f32, const uint8_t* mask, float* enc_out, uint8_t* enc_mask, int B, int S, int S_cap, int d,
                     int L, const int* text_len) {
    if ((!enc_out && !enc_mask) || (enc_out && !enc_f32) || (enc_mask && !mask)) return MG_E_ARG;
    if (B < 1 || L < 0 || S < 1 || L > S || S > S_cap || d < 4 || (d & 3)) return MG_E_SHAPE;
    enc_copy_out(enc_f32, mask, enc_out, enc_mask, B, S, S_cap, d, L, text_len, (mgStream_t)stream);
    return MG_OK;
}
int mgk_embed_rows(void* stream, const int64_t* ids, const void* tok_emb, float* h, int rows, int d, int V, int* err, void* x_pk, int x_ld,
                   int x_col0) {
    if (!ids || !tok_emb || !h || !err) return MG_E_ARG;
    if (rows < 1 || d < 4 || (d & 3) || V < 1) return MG_E_SHAPE;
    if (x_pk && ((x_ld & 15) || x_col0 < 0 || (x_col0 & 3) || x_col0 + d > x_ld)) return MG_E_SHAPE;
    embed_rows(ids, (const uint16_t*)tok_emb, h, rows, d, V, err, (mgStream_t)stream, (uint16_t*)x_pk, x_ld, x_col0);
    return MG_OK;
}
int mgk_rmsnorm_pack_rows(void* stream, const float* h, const float* gain, void* x_pk, const int* dst_row, int M, int d, float eps, float scale) {
    if (!h || !gain || !x_pk) return MG_E_ARG;
    if (M < 1 || d < 16 || (d & 15)) return MG_E_SHAPE;
    rmsnorm_pack_rows(h, gain, (uint16_t*)x_pk, dst_row, M, d, eps, scale, (mgStream_t)stream);
    return MG_OK;
}

size_t mg_preprocess_scratch_bytes(int B, int Hs, int Ws, int out_size) {
    if (B < 1 || Hs < 1 || Ws < 1 || out_size < 1) return 0;
    return preprocess_scratch_bytes(B, Hs, Ws, out_size);
}

int mg_preprocess_pages(void* stream, const uint8_t* pages_u8, int B, int Hs, int Ws, int out_size, float* pixel_values,
                        void* scratch, size_t scratch_bytes) {
    if (!pages_u8 || !pixel_values || !scratch || B < 1 || Hs < 1 || Ws < 1 || out_size < 1) return MG_E_ARG;
    if (scratch_bytes < preprocess_scratch_bytes(B, Hs, Ws, out_size)) return MG_E_WORKSPACE;
    preprocess_pages(pages_u8, B, Hs, Ws, out_size, pixel_values, scratch, (mgStream_t)stream);
    return MG_OK;
}

}  // extern "C"

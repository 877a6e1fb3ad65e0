// Sampled selection of the decode step (stock generation/utils.py::_sample with do_sample = True): MinLength -> temperature -> top-k ->
// top-p -> one draw per live row, with greedy_select_kernel's bookkeeping (finished rows emit pad, a row stops at EOS, step counters).
//
// One workgroup per decode row: NT = 1024 threads with NQ = 1 or 3 loads each for V <= 4096 / 12 288, and NT = 512 threads with
// NQ = 18 loads for V <= 36 864 (the large shape's 33 201).  The row is read from memory ONCE (16-byte loads, one batch of NQ independent
// loads per thread) and stays in registers as (integer key, integer mass) pairs: wave w holds the NQ * 256 consecutive tokens from
// w * NQ * 256 on, load u of lane l being tokens 4 * (w * NQ * 64 + u * 64 + l) .. + 3 - coalesced, and token-index order is
// (wave, load, lane, element).  There is no re-reading form for larger vocabularies (sample_select_supported).
// Registers: 72 values per thread do not fit the 128 VGPRs of a 1024-thread workgroup (9 loads: 75 dwords spilled, 88 us per launch at
// 160 rows); 512 threads have 256 and hold 144 values (38 dwords still spilled by the compiler, none in the histogram loops; 79 us).
//
// Everything that decides the token is integer arithmetic, so a row's draw is the same run to run and whatever else its call holds:
//   mass     m_i = min(rint(expf((x_i - max) / T) * 2^32), 2^32 - 1)  (u32; the clamp moves the maximum's own mass by one unit of the
//            fixed-point step, which every other mass is uncertain by anyway; the row's sum stays below V * 2^32 < 2^48)
//   top-k    the k-th largest value by radix select on the order-preserving integer image of the floats: 4 passes of 8-bit digits,
//            counts in an LDS histogram; every token >= that value survives (ties kept, stock's `scores < kth`)
//   top-p    the smallest value v whose ascending cumulative mass over the survivors (ties at v included) exceeds
//            (u64)((1 - top_p) * total): the same radix select with u64 masses in the histogram; tokens >= v survive
//   draw     r = 64 bits of Philox4x32-10 (key = seed, counter = (stream id lo, stream id hi, position, 0)); the token whose interval
//            of the survivors' running mass IN TOKEN-INDEX ORDER holds __umul64hi(r, total_kept): wave totals through LDS, then the
//            wave that holds the target finds the load, the lane and the element
// The histograms are [256 bins][4 copies] (lane & 3 picks the copy): logits cluster in a few exponent bins, and same-address LDS
// atomics serialise.  Integer adds are order-independent, so the copies change nothing but the contention.  LDS: 8.5 KB.
#include "mg_kernels.h"

namespace mg {

namespace {
constexpr int SS_COPIES = 4;
typedef unsigned long long u64;

MG_DEV float ss_neg_inf() { return -__builtin_inff(); }
// order-preserving image of a float (no NaN): a < b  <=>  key(a) < key(b)
MG_DEV uint32_t ss_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MG_DEV float ss_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
MG_DEV uint32_t ss_mass(float v, float mx, float T) {
    const float r = rintf(expf((v - mx) / T) * 4294967296.f);
    return r >= 4294967296.f ? 0xFFFFFFFFu : (r > 0.f ? (uint32_t)r : 0u);      // (a NaN gives 0)
}
MG_DEV u64 ss_shfl64(u64 v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
MG_DEV u64 ss_wave_sum64(u64 v, int lane) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += ss_shfl64(v, lane ^ m);
    return v;
}
MG_DEV u64 ss_wave_scan64(u64 v, int lane) {      // inclusive, lane order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = ss_shfl64(v, (lane - off) & 63);
        if (lane >= off) v += o;
    }
    return v;
}
MG_DEV void ss_top2_merge(float& b1, float& b2, int& i1, float o1, float o2, int oi) {
    if (o1 > b1 || (o1 == b1 && oi < i1)) { b2 = fmaxf(b1, o2); b1 = o1; i1 = oi; }
    else b2 = fmaxf(b2, o1);
}

// Radix select over the row held in registers.  MASS = false: the key of the (limit + 1)-th largest token (descending, counts).
// MASS = true: the smallest key whose ascending cumulative mass over the tokens with key >= floor_key exceeds `limit`.  The caller
// guarantees that such a key exists (limit < number of tokens / < total mass).  Every thread returns the key.
template <int NQ, bool MASS, int NT>
MG_DEV uint32_t ss_radix_select(const uint32_t (&keys)[NQ * 4], const uint32_t (&m)[NQ * 4], u64* hist, u64* sel, uint32_t floor_key, u64 limit,
                                int tid) {
    uint32_t prefix = 0, pmask = 0;
    u64 base = 0;       // tokens (mass) in front of the prefix' range in scan order
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256 * SS_COPIES; i += NT) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NQ * 4; ++i) {
            const uint32_t key = keys[i];
            const u64 val = MASS ? (u64)m[i] : (u64)1;
            if ((key & pmask) == prefix && key >= floor_key && val != 0)
                atomicAdd(hist + ((key >> shift) & 255u) * SS_COPIES + (tid & (SS_COPIES - 1)), val);
            if ((i & 3) == 3) MG_SCHED_FENCE();      // (keeps the unrolled body from being interleaved across the whole row: register pressure)
        }
        __syncthreads();
        if (tid < 64) {                      // the 256-bin scan: lane l takes 4 bins in scan order, the lanes are combined by shuffles
            u64 t[4], lt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 4 * tid + j, bin = MASS ? s : 255 - s;
                t[j] = hist[bin * SS_COPIES] + hist[bin * SS_COPIES + 1] + hist[bin * SS_COPIES + 2] + hist[bin * SS_COPIES + 3];
                lt += t[j];
            }
            u64 excl = base + ss_wave_scan64(lt, tid) - lt;
            if (excl <= limit && limit < excl + lt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = 4 * tid + j, bin = MASS ? s : 255 - s;
                    if (excl <= limit && limit < excl + t[j]) { sel[0] = (u64)bin; sel[1] = excl; }
                    excl += t[j];
                }
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sel[0] << shift;
        pmask |= 255u << shift;
        base = sel[1];
    }
    return prefix;
}

// QUEUE: the continuous decoder's form (SampleArgs::slots, mg_kernels.h) - the row's column, output row and random stream are those of
// the sequence in the slot (three wave-uniform scalars); everything that decides the token is the batch form's code.
// QUEUE under a prompt / constraint: the owner of a live row is the image of its sequence, seq / slots.nsamp; a forced column and the
// empty-set rule are the batch form's, and a row that ends frees its slot as ever.
// CON (DecConstraint in mg_kernels.h): the tokens the row's state does not allow become -inf where MinLength's EOS does, in
// the registers that hold the row, before temperature, top-k, top-p and the draw; the draw's counter and stream are unchanged.
template <int NQ, int NT, bool QUEUE, bool CON = false>
__global__ __launch_bounds__(NT) void sample_select_kernel(SampleArgs a) {
    MG_DYN_SMEM(smem);
    u64* hist = (u64*)smem;                  // [256][SS_COPIES]
    u64* wtot = hist + 256 * SS_COPIES;      // [16] the waves' surviving mass
    u64* sel = wtot + 16;                    // [2] digit and running base of a radix pass
    float* rv = (float*)(sel + 2);           // [16][2]
    int* ri = (int*)(rv + 32);               // [16]
    int* trow = ri + 16;                     // CON: [n_classes] the table row of the row's state
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int unf = a.unfinished[row];       // (queue form: 0 = idle slot, computed on stale inputs - nothing is written, nothing is drawn)
    // Queue form: both slot-table loads stay HERE, in front of the first barrier.  The lane that holds the draw later stores slots.pos[row]
    // and clears slots.img[row] while other waves may still be computing the target from them (their first use, the Philox call, comes
    // after the last barrier): a load moved down towards that use would race with those stores.
    const int pos = QUEUE ? a.slots.pos[row] + 1 : (a.pos_dev ? *a.pos_dev + a.pos : a.pos);      // column written
    const int seq = QUEUE ? a.slots.img[row] : row;              // row of out_ids / token_scores / stream_ids
    int64_t tok = (int64_t)a.pad;
    float score = 0.f, b1 = 0.f, b2 = 0.f;
    bool writer = tid == 0;                  // the thread that does the row's bookkeeping: thread 0 of a finished or forced row, else the one that holds the draw
    // decoder prompt (batch form): a row in a forced column neither scans nor draws - thread 0 writes the prompt's token with score 0 and
    // the row stays live; it takes part in the step's counters exactly as a free row does
    bool forced = false;
    const int owner = QUEUE ? (a.slots.nsamp > 1 ? seq / a.slots.nsamp : seq) : (a.prompt.group > 1 ? row / a.prompt.group : row);
    if (a.prompt.ids && (!QUEUE || unf)) forced = pos < a.prompt.len[owner];      // (queue form: an idle slot has no owner)
    if (forced) {
        // Every thread has read the step counter (pos) before thread 0 may advance it: the last workgroup to arrive increments *pos_dev in
        // its bookkeeping below, and a thread of this workgroup that read it afterwards would no longer see a forced column.  (A free row
        // has its scan's barriers between the two; a finished row never looks at pos again.)
        __syncthreads();
        if (tid == 0) prompt_forced_owner(a.prompt, owner, pos, a.V, tok);
    } else if (unf) {
        const float* lg = a.logits + (size_t)row * a.ldl;
        const bool no_eos = pos < a.min_len;
        const int nq = (a.V + 3) >> 2;       // rows are padded to a multiple of 32 floats, so the last float4 is readable
        const int c0 = w * 64 * NQ + lane;
        float4 q[NQ];
        uint2 kc[CON ? NQ : 1];              // CON: the classes of a load's four tokens, 16 bits each
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int c = c0 + u * 64;
            q[u] = c < nq ? *(const float4*)(lg + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (CON) kc[u] = c < nq ? *(const uint2*)(a.con.cls + c * 4) : make_uint2(0u, 0u);
        }
        if (CON) {                           // (the branch is uniform over the workgroup: unf and forced are the row's)
            const int* src = a.con.table + (size_t)a.con.state[row] * a.con.n_classes;
            for (int c = tid; c < a.con.n_classes; c += NT) trow[c] = src[c];
            __syncthreads();
        }
        uint32_t m[NQ * 4], keys[NQ * 4];     // the row is kept as (key, mass) pairs; a key gives its float back (ss_unkey)
        b1 = -3.0e38f; b2 = -3.0e38f;
        int i1 = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const float vv[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = (c0 + u * 64) * 4 + j;
                // tokens past V and a suppressed EOS leave the distribution: -inf has mass 0 and sorts below every logit (-0 -> +0: one key per value)
                bool out = i >= a.V || (no_eos && i == a.eos);
                if (CON && !out) out = trow[((j < 2 ? kc[u].x : kc[u].y) >> ((j & 1) * 16)) & 0xffffu] < 0;
                const float x = out ? ss_neg_inf() : vv[j] + 0.0f;
                keys[u * 4 + j] = ss_key(x);
                if (x > b1 || (x == b1 && i < i1)) { b2 = b1; b1 = x; i1 = i; }
                else if (x > b2) b2 = x;
            }
        }
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const float o1 = __shfl_xor(b1, step), o2 = __shfl_xor(b2, step);
            const int oi = __shfl_xor(i1, step);
            ss_top2_merge(b1, b2, i1, o1, o2, oi);
        }
        if (lane == 0) { rv[w * 2] = b1; rv[w * 2 + 1] = b2; ri[w] = i1; }
        __syncthreads();
        b1 = rv[0]; b2 = rv[1]; i1 = ri[0];
        for (int ww = 1; ww < NT / 64; ++ww) ss_top2_merge(b1, b2, i1, rv[ww * 2], rv[ww * 2 + 1], ri[ww]);
        const float mx = b1, T = a.temperature;
#pragma unroll
        for (int i = 0; i < NQ * 4; ++i) {
            m[i] = ss_mass(ss_unkey(keys[i]), mx, T);
            if ((i & 3) == 3) MG_SCHED_FENCE();
        }
        // top-k: k clamped to the tokens in the distribution
        uint32_t kmin = 0;
        // (CON: n_alive does not count the masked tokens.  A top_k above the allowed count then selects a -inf key as the k-th largest: every
        // finite token survives and the -inf ones carry mass 0 - what the unconstrained kernel does on host-masked logits, bit for bit.)
        int n_alive = a.V - ((no_eos && a.eos >= 0 && a.eos < a.V) ? 1 : 0);
        if (a.top_k > 0 && a.top_k < n_alive) kmin = ss_radix_select<NQ, false, NT>(keys, m, hist, sel, 0u, (u64)(a.top_k - 1), tid);
        // top-p over the top-k survivors
        if (a.top_p < 1.0f) {
            u64 s1 = 0;
#pragma unroll
            for (int i = 0; i < NQ * 4; ++i) s1 += keys[i] >= kmin ? (u64)m[i] : (u64)0;
            s1 = ss_wave_sum64(s1, lane);
            __syncthreads();                 // (wtot may still be read by nobody; sel / hist of the top-k passes are done with)
            if (lane == 0) wtot[w] = s1;
            __syncthreads();
            u64 total1 = 0;
            for (int ww = 0; ww < NT / 64; ++ww) total1 += wtot[ww];
            u64 thr = (u64)((1.0 - (double)a.top_p) * (double)total1);
            if (thr >= total1) thr = total1 > 0 ? total1 - 1 : 0;        // at least the maximum survives
            if (total1 > 0) {
                const uint32_t qmin = ss_radix_select<NQ, true, NT>(keys, m, hist, sel, kmin, thr, tid);
                kmin = qmin > kmin ? qmin : kmin;
            }
        }
        // the draw: wave totals of the survivors' masses -> target -> wave -> load -> lane -> element
        u64 mine = 0;
#pragma unroll
        for (int i = 0; i < NQ * 4; ++i) {
            if (keys[i] < kmin) m[i] = 0;
            mine += m[i];
        }
        mine = ss_wave_sum64(mine, lane);
        __syncthreads();
        if (lane == 0) wtot[w] = mine;
        __syncthreads();
        u64 total = 0, before = 0;
        for (int ww = 0; ww < NT / 64; ++ww) { if (ww == w) before = total; total += wtot[ww]; }
        uint32_t rnd[4];
        philox4x32_10(a.seed, a.stream_ids ? a.stream_ids[seq] : (uint64_t)seq, (uint32_t)pos, rnd);
        const u64 r = ((u64)rnd[1] << 32) | rnd[0];
        const u64 target = __umul64hi(r, total);             // in [0, total)
        writer = false;
        if (total == 0) {                    // no finite logit in the row (never with a model's logits): emit the arg-max slot, keep the protocol
            writer = tid == 0;
            tok = (int64_t)(i1 < a.V ? i1 : 0);
            // CON: no mass at all counts as the empty allowed set - also when the allowed tokens' logits are all -inf or not finite, which a
            // model's logits never are.  EOS ends the row in the sink, score 0.0, no draw
            if (CON && tid == 0) {
                tok = (int64_t)a.eos;
                a.con.state[row] = a.con.n_states - 1;
                atomicAdd(a.con.empty, 1);
            }
        } else if (target >= before && target < before + mine) {      // wave-uniform: this wave holds the target
            u64 t = target - before;
            bool found = false;
            u64 su_sel = 0;
            uint32_t ms[4] = {0, 0, 0, 0};
            uint32_t ks[4] = {0, 0, 0, 0};
            int u_sel = 0;
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const u64 su = (u64)m[u * 4] + m[u * 4 + 1] + m[u * 4 + 2] + m[u * 4 + 3];
                const u64 tot = ss_wave_sum64(su, lane);
                if (!found) {
                    if (t < tot) {
                        found = true; u_sel = u; su_sel = su;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { ms[j] = m[u * 4 + j]; ks[j] = keys[u * 4 + j]; }
                    } else {
                        t -= tot;
                    }
                }
            }
            u64 excl = ss_wave_scan64(su_sel, lane) - su_sel;
            if (t >= excl && t < excl + su_sel) {
                writer = true;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (t >= excl && t < excl + ms[j]) {
                        tok = (int64_t)((c0 + u_sel * 64) * 4 + j);
                        // log-probability under the warped distribution: the token's own exponent (not its rounded mass) over the integer total
                        score = (ss_unkey(ks[j]) - mx) / T - logf((float)((double)total * (1.0 / 4294967296.0)));
                    }
                    excl += ms[j];
                }
                if (CON) a.con.state[row] = trow[a.con.cls[tok]];      // the row's state advances with the drawn token
            }
        }
    }
    if (writer) {
        if (QUEUE) {
            // greedy_select_kernel's stream branch, store for store: a row that ends frees its slot (slot_refill hands it the next sequence)
            if (!unf) return;
            a.next_ids[row] = tok;
            a.slots.pos[row] = pos;
            if (pos < a.max_len) a.out_ids[(size_t)seq * a.max_len + pos] = tok;
            if (a.token_scores && pos < a.max_len) a.token_scores[(size_t)seq * a.ts_ld + pos - 1] = score;
            if ((!forced && tok == (int64_t)a.eos) || pos + 1 >= a.max_len) {      // (a forced EOS does not end the row)
                a.unfinished[row] = 0;
                a.slots.img[row] = -1;
                a.slots.out_len[seq] = pos + 1 < a.max_len ? pos + 1 : a.max_len;
                atomicAdd(a.slots.ctr + 1, 1);
            }
            return;
        }
        a.next_ids[row] = tok;
        if (pos < a.max_len) a.out_ids[(size_t)row * a.max_len + pos] = tok;
        if (a.token_scores && pos < a.max_len) a.token_scores[(size_t)row * a.ts_ld + pos - 1] = unf ? score : 0.f;
        const int still = forced ? 1 : (unf && tok != (int64_t)a.eos);
        a.unfinished[row] = still;
        if (still) atomicAdd(a.n_unfinished, 1);
        if (a.top2) {
            float* tp = a.top2 + (a.pos_dev ? (size_t)pos * a.rows * 2 : 0);
            tp[row * 2] = b1; tp[row * 2 + 1] = b2;
        }
        if (a.step_ctr) {                    // greedy_select_kernel's step bookkeeping (counters layout: engine.hip)
            int* c = a.step_ctr;
            __threadfence();
            if (atomicAdd(c + 6, 1) == a.rows - 1) {
                const int unf_total = atomicAdd(a.n_unfinished, 0);
                *a.n_unfinished = 0;
                c[0] = unf_total;
                if (unf_total == 0 && c[1] < 0) c[1] = c[2];
                c[2] += 1;
                c[6] = 0;
            }
        }
    }
}
}  // namespace

bool sample_select_supported(int V) { return V >= 1 && V <= 4096 * 9; }

void sample_select(const SampleArgs& a, mgStream_t stream) {
    const size_t lds = (256 * SS_COPIES + 16 + 2) * sizeof(u64) + 32 * sizeof(float) + 16 * sizeof(int);
    if (a.slots.pos && a.con.cls) {
        const size_t ldc = lds + (size_t)a.con.n_classes * sizeof(int);
        if (a.V <= 4096) MG_LAUNCH((sample_select_kernel<1, 1024, true, true>), dim3(a.rows), dim3(1024), ldc, stream, a);
        else if (a.V <= 4096 * 3) MG_LAUNCH((sample_select_kernel<3, 1024, true, true>), dim3(a.rows), dim3(1024), ldc, stream, a);
        else MG_LAUNCH((sample_select_kernel<18, 512, true, true>), dim3(a.rows), dim3(512), ldc, stream, a);
        return;
    }
    if (a.slots.pos) {
        if (a.V <= 4096) MG_LAUNCH((sample_select_kernel<1, 1024, true>), dim3(a.rows), dim3(1024), lds, stream, a);
        else if (a.V <= 4096 * 3) MG_LAUNCH((sample_select_kernel<3, 1024, true>), dim3(a.rows), dim3(1024), lds, stream, a);
        else MG_LAUNCH((sample_select_kernel<18, 512, true>), dim3(a.rows), dim3(512), lds, stream, a);
        return;
    }
    if (a.con.cls) {
        const size_t ldc = lds + (size_t)a.con.n_classes * sizeof(int);
        if (a.V <= 4096) MG_LAUNCH((sample_select_kernel<1, 1024, false, true>), dim3(a.rows), dim3(1024), ldc, stream, a);
        else if (a.V <= 4096 * 3) MG_LAUNCH((sample_select_kernel<3, 1024, false, true>), dim3(a.rows), dim3(1024), ldc, stream, a);
        else MG_LAUNCH((sample_select_kernel<18, 512, false, true>), dim3(a.rows), dim3(512), ldc, stream, a);
        return;
    }
    if (a.V <= 4096) MG_LAUNCH((sample_select_kernel<1, 1024, false>), dim3(a.rows), dim3(1024), lds, stream, a);
    else if (a.V <= 4096 * 3) MG_LAUNCH((sample_select_kernel<3, 1024, false>), dim3(a.rows), dim3(1024), lds, stream, a);
    else MG_LAUNCH((sample_select_kernel<18, 512, false>), dim3(a.rows), dim3(512), lds, stream, a);
}

}  // namespace mg

// BERT embeddings of the HIP text encoder (gfx950): HF `BertEmbeddings` -- word + token-type + position gather,
// LayerNorm, dropout -- as one forward kernel that writes the layer stack's first input in time-major rows
// (row = t*B + b), and the scatter of the pre-LayerNorm gradient into the three table gradients WITHOUT float
// atomics: every destination row has one owner that adds its contributions in one fixed order (bitwise reproducible).
//
// Forward: one wave per row, 16-byte accesses (d % 32 == 0, d <= 1024), two rows (six gathered table rows) in flight
// per wave: the kernel is bound by gather latency, not by bytes.  Inputs, the sum s and every output are fp32; the
// LayerNorm of a row is evaluated in fp64 registers and rounded once.
// Backward (after bpm_ln_bwd_ws has produced ds): two launches.
//   stage 1  word table: the ids arrive SORTED (stable) with their permutation; the sorted list is cut where the id changes
//            and at every SC_CH-th position, one wave sums each piece in sorted order.  A piece that is a whole run is
//            stored to its table row; the others go to a workspace (two slots per SC_CH positions: the piece that starts
//            the chunk, the piece that ends it).
//            position table: dpos[t] = sum_b ds[t*B + b] (B adjacent rows), one wave per t.
//            type table: per-block partial rows (SC_TROWS rows of ds each) for every type id.
//   stage 2  word table: the wave of the chunk in which a split run STARTS adds the run's pieces in chunk order.
//            type table: one thread per (type id, four columns) adds the partial rows in block order.
#include "rows_common.h"      // NT, put4

namespace {

constexpr int WPB = NT / 64;
constexpr int SC_CH = 32;        // sorted positions per chunk of the word-table sum (<= 64: one ballot finds a piece's end)
constexpr int SC_TROWS = 32;     // rows of ds per partial row of the type-table sum

BPM_DEV double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct EmbFwdP {
    const int64_t* ids; const int64_t* seg;
    const float* word; const float* pos; const float* type;
    const float* gamma; const float* beta;
    float* x; void* xc; float* s; float* mean; float* rstd; unsigned* bad;
    int V, Tt, B, L, ldc;
    float eps;
    DropCfg drop;
};

template <typename CT, int NV>
__global__ __launch_bounds__(NT) void bert_embed_fwd_kernel(const EmbFwdP P, int d, const uint64_t* seedp) {
    const DropCfg drop = bpm_resolve_drop(P.drop, seedp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nch = d >> 2;
    const int R = P.L * P.B;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 gam[NV], bet[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        gam[e] = *(const f32x4*)(P.gamma + 4 * (q < nch ? q : 0));
        bet[e] = *(const f32x4*)(P.beta + 4 * (q < nch ? q : 0));
    }
    constexpr int U = 2;                             // rows in flight per wave
    for (int row0 = (blockIdx.x * WPB + wv) * U; row0 < R; row0 += gridDim.x * WPB * U) {
        f32x4 wr[U][NV], ty[U][NV], po[U][NV];
        bool okw[U], okt[U];
        // phase 1: the ids, then every gather of the U rows (clamped rows / chunks / ids: never outside a table)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            const int rc = row < R ? row : row0;
            const int t = rc / P.B, b = rc - t * P.B;
            const int64_t id = P.ids[(size_t)b * P.L + t];
            const int64_t sg = P.seg ? P.seg[(size_t)b * P.L + t] : 0;
            okw[u] = id >= 0 && id < P.V;
            okt[u] = sg >= 0 && sg < P.Tt;
            const float* w = P.word + (size_t)(okw[u] ? id : 0) * d;
            const float* y = P.type + (size_t)(okt[u] ? sg : 0) * d;
            const float* p = P.pos + (size_t)t * d;  // t < L <= P (host)
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const int qc = q < nch ? q : 0;
                wr[u][e] = *(const f32x4*)(w + 4 * qc);
                ty[u][e] = *(const f32x4*)(y + 4 * qc);
                po[u][e] = *(const f32x4*)(p + 4 * qc);
            }
            if (lane == 0 && row < R) {
                const unsigned nbad = (okw[u] ? 0u : 1u) + (okt[u] ? 0u : 1u);
                if (nbad) atomicAdd(P.bad, nbad);    // an id outside its table: a zero row and a count, no fault
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            if (row >= R) continue;                  // wave-uniform
            // s itself is fp32 (HF's own two fp32 adds, bit for bit); the row statistics and the normalisation are carried
            // in fp64 registers and rounded ONCE: x is the correctly rounded LayerNorm of s, so against another fp32
            // evaluation of the same embeddings only that evaluation's rounding noise is left
            f32x4 v[NV];
            double sm = 0.0;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const f32x4 a = okw[u] ? wr[u][e] : zero;
                const f32x4 c = okt[u] ? ty[u][e] : zero;
                const f32x4 sv = (a + c) + po[u][e];              // HF: (inputs_embeds + token_type_embeddings) + position_embeddings
                v[e] = q < nch ? sv : zero;
                if (q < nch) *(f32x4*)(P.s + (size_t)row * d + 4 * q) = sv;
                sm += ((double)v[e][0] + (double)v[e][1]) + ((double)v[e][2] + (double)v[e][3]);
            }
            const double mu = wave_sum_d(sm) / d;
            double qq = 0.0;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                if (lane + 64 * e < nch) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const double t = (double)v[e][j] - mu; qq += t * t; }
                }
            }
            const double rs = 1.0 / sqrt(wave_sum_d(qq) / d + (double)P.eps);
            if (lane == 0) { P.mean[row] = (float)mu; P.rstd[row] = (float)rs; }
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                if (q < nch) {
                    f32x4 y;
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[j] = (float)(((double)v[e][j] - mu) * rs * (double)gam[e][j] + (double)bet[e][j]);
                    if (drop.thresh != 0) {          // row*d + 4q is a multiple of 4: one hash quad
                        float d0, d1, d2, d3;
                        bpm_drop_mult4(drop, (uint32_t)row * (uint32_t)d + 4u * (uint32_t)q, d0, d1, d2, d3);
                        y[0] *= d0; y[1] *= d1; y[2] *= d2; y[3] *= d3;
                    }
                    *(f32x4*)(P.x + (size_t)row * d + 4 * q) = y;
                    if (P.xc) put4<CT>(P.xc, (size_t)row * P.ldc + 4 * q, y);
                } else if (P.xc && 4 * q < P.ldc) {
                    put4<CT>(P.xc, (size_t)row * P.ldc + 4 * q, zero);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct EmbScP {
    const float* ds; const int64_t* sid; const int64_t* perm; const int64_t* seg;
    float* dword; float* dpos; float* dtype;
    float* ws_word; float* ws_type;
    int V, Tt, B, L;
    long long pad_idx;
    unsigned nb_word, nb_pos, nb_type;   // block ranges of a launch, in this order
};

BPM_DEV bool word_ok(const EmbScP& P, long long id) { return id >= 0 && id < P.V && id != P.pad_idx; }

// acc = sum of n rows of `src`; row k starts at src + rowoff(k) floats; fixed order, four rows in flight
template <int NV, typename F>
BPM_DEV void sum_rows(f32x4 (&acc)[NV], const float* src, int n, int nch, int lane, F rowoff) {
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = zero;
    for (int k0 = 0; k0 < n; k0 += 4) {
        f32x4 v[4][NV];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t off = rowoff(k0 + j < n ? k0 + j : k0);
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                v[j][e] = *(const f32x4*)(src + off + 4 * (q < nch ? q : 0));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k0 + j < n) {
#pragma unroll
                for (int e = 0; e < NV; ++e) acc[e] += v[j][e];
            }
    }
}

template <int NV>
BPM_DEV void store_row(float* dst, const f32x4 (&acc)[NV], int nch, int lane) {
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        if (q < nch) *(f32x4*)(dst + 4 * q) = acc[e];
    }
}

template <int NV>
__global__ __launch_bounds__(NT) void bert_scatter1_kernel(const EmbScP P, int d) {
    __shared__ float red[WPB][NV * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nch = d >> 2;
    const int R = P.L * P.B;
    unsigned bid = blockIdx.x;
    if (bid < P.nb_word) {
        // ---- word table: one wave per sorted position; only the first position of a piece works
        const int i = (int)bid * WPB + wv;
        if (i >= R) return;
        const long long id = P.sid[i];
        const bool run_start = i == 0 || P.sid[i - 1] != id;
        if (!(run_start || i % SC_CH == 0) || !word_ok(P, id)) return;          // wave-uniform
        const int lim = min(R, (i / SC_CH + 1) * SC_CH);                        // the piece ends at the chunk's end at the latest
        const int k = i + 1 + lane;
        const bool diff = k < lim ? P.sid[k] != id : true;                      // lane lim - i - 1 <= 63 is always set
        const int len = __ffsll((unsigned long long)__ballot(diff));
        const int j = i + len;
        const bool run_end = j == R || P.sid[j] != id;
        // time-major row of sorted position i + lane (perm indexes the batch-major [B, L] ids)
        long long p = lane < len ? P.perm[i + lane] : 0;
        p = p < 0 ? 0 : (p >= R ? R - 1 : p);
        const int myrow = (int)(p % P.L) * P.B + (int)(p / P.L);
        f32x4 acc[NV];
        sum_rows<NV>(acc, P.ds, len, nch, lane, [&](int kk) { return (size_t)__shfl(myrow, kk) * d; });
        float* dst = (run_start && run_end) ? P.dword + (size_t)id * d
                                            : P.ws_word + (size_t)(2 * (i / SC_CH) + (i % SC_CH == 0 ? 0 : 1)) * d;
        store_row<NV>(dst, acc, nch, lane);
        return;
    }
    bid -= P.nb_word;
    if (bid < P.nb_pos) {
        // ---- position table: B adjacent rows per time step
        const int t = (int)bid * WPB + wv;
        if (t >= P.L) return;
        f32x4 acc[NV];
        sum_rows<NV>(acc, P.ds + (size_t)t * P.B * d, P.B, nch, lane, [&](int kk) { return (size_t)kk * d; });
        store_row<NV>(P.dpos + (size_t)t * d, acc, nch, lane);
        return;
    }
    bid -= P.nb_pos;
    // ---- type table, stage 1: this block's SC_TROWS rows, one partial row per type id
    const int r0 = (int)bid * SC_TROWS, r1 = min(R, r0 + SC_TROWS);
    constexpr int RPW = SC_TROWS / WPB;
    long long sg[RPW];
#pragma unroll
    for (int a = 0; a < RPW; ++a) {
        const int r = r0 + wv + WPB * a;
        const int rc = r < r1 ? r : r0;
        const int t = rc / P.B, b = rc - t * P.B;
        sg[a] = r < r1 ? (P.seg ? P.seg[(size_t)b * P.L + t] : 0) : -1;
    }
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tt = 0; tt < P.Tt; ++tt) {
        f32x4 acc[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[e] = zero;
#pragma unroll
        for (int a = 0; a < RPW; ++a) {
            if (sg[a] != tt) continue;               // wave-uniform
            const float* src = P.ds + (size_t)(r0 + wv + WPB * a) * d;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const f32x4 v = *(const f32x4*)(src + 4 * (q < nch ? q : 0));
                acc[e] += q < nch ? v : zero;
            }
        }
#pragma unroll
        for (int e = 0; e < NV; ++e) *(f32x4*)(&red[wv][4 * (lane + 64 * e)]) = acc[e];
        __syncthreads();
        float* dst = P.ws_type + ((size_t)bid * P.Tt + tt) * d;
        for (int q = threadIdx.x; q < nch; q += NT) {
            f32x4 s4 = *(const f32x4*)(&red[0][4 * q]);
#pragma unroll
            for (int w = 1; w < WPB; ++w) s4 += *(const f32x4*)(&red[w][4 * q]);
            *(f32x4*)(dst + 4 * q) = s4;
        }
        __syncthreads();
    }
}

template <int NV>
__global__ __launch_bounds__(NT) void bert_scatter2_kernel(const EmbScP P, int d) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nch = d >> 2;
    const int R = P.L * P.B;
    unsigned bid = blockIdx.x;
    if (bid < P.nb_word) {
        // ---- word table: the chunk in which a run that crosses a chunk boundary STARTS owns that run
        const int nchunk = (R + SC_CH - 1) / SC_CH;
        const int c = (int)bid * WPB + wv;
        if (c >= nchunk - 1) return;                                            // the last chunk has no successor
        const int last = (c + 1) * SC_CH - 1;                                   // < R: c is not the last chunk
        const long long id = P.sid[last];
        if (P.sid[last + 1] != id || !word_ok(P, id)) return;                  // the run ends with this chunk: stage 1 finished it
        const bool eq = lane < SC_CH ? P.sid[c * SC_CH + lane] == id : false;
        const int first = __ffsll((unsigned long long)__ballot(eq)) - 1;       // >= 0: position `last` matches
        if (first == 0 && c > 0 && P.sid[c * SC_CH - 1] == id) return;         // started earlier: an earlier chunk owns it
        // the following chunks that START with this id (their first piece sits in slot 2 c')
        int n = 0;
        for (int base = c + 1;; base += 64) {
            const int kc = base + lane;
            const bool same = kc < nchunk && P.sid[(size_t)kc * SC_CH] == id;
            const unsigned long long m = ~(unsigned long long)__ballot(same);
            const int cnt = m == 0 ? 64 : __ffsll(m) - 1;
            n += cnt;
            if (cnt < 64) break;
        }
        const size_t own = (size_t)(2 * c + (first == 0 ? 0 : 1)) * d;
        f32x4 acc[NV];
        sum_rows<NV>(acc, P.ws_word, n + 1, nch, lane, [&](int kk) { return kk == 0 ? own : (size_t)(2 * (c + kk)) * d; });
        store_row<NV>(P.dword + (size_t)id * d, acc, nch, lane);
        return;
    }
    bid -= P.nb_word;
    // ---- type table, stage 2: one owner per (type id, four columns), partial rows in block order
    const int nblk = (R + SC_TROWS - 1) / SC_TROWS;
    const int v = (int)bid * NT + threadIdx.x;
    if (v >= P.Tt * nch) return;
    const int tt = v / nch, q = v - tt * nch;
    const float* src = P.ws_type + (size_t)tt * d + 4 * q;
    f32x4 acc4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) acc4 += *(const f32x4*)(src + (size_t)b * P.Tt * d);
    *(f32x4*)(P.dtype + (size_t)tt * d + 4 * q) = acc4;
}

inline bool al(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int bpm_bert_embed_fwd(int dtype, const bpm_bert_embed_problem* q, int d, float eps, uint64_t seed, void* stream) {
    if (!q || (dtype != BPM_F32 && dtype != BPM_BF16)) return BPM_ERR_ARG;
    if (d < 32 || d % 32 || d > 1024) return BPM_ERR_ARG;
    if (!q->ids || !q->word || !q->pos || !q->type || !q->gamma || !q->beta || !q->x || !q->s || !q->mean || !q->rstd || !q->bad)
        return BPM_ERR_ARG;
    if (q->B < 1 || q->L < 1 || q->V < 1 || q->P < 1 || q->Tt < 1 || q->L > q->P) return BPM_ERR_ARG;
    if ((size_t)q->B * q->L * d > 0xFFFFFFFFull) return BPM_ERR_ARG;            // 32-bit element counter of the dropout hash
    if (q->xc && (q->ldc < d || q->ldc % 4 || q->ldc > 1024)) return BPM_ERR_ARG;
    if (!(q->drop_p >= 0.f && q->drop_p < 1.f)) return BPM_ERR_ARG;
    const unsigned csz = dtype == BPM_BF16 ? 2 : 4;
    if (!al(q->word, 16) || !al(q->pos, 16) || !al(q->type, 16) || !al(q->gamma, 16) || !al(q->beta, 16) || !al(q->x, 16) ||
        !al(q->s, 16) || !al(q->xc, 4 * csz) || !al(q->ids, 8) || !al(q->seg, 8) || !al(q->mean, 4) || !al(q->rstd, 4) || !al(q->bad, 4))
        return BPM_ERR_ALIGN;
    EmbFwdP p;
    p.ids = q->ids; p.seg = q->seg; p.word = q->word; p.pos = q->pos; p.type = q->type; p.gamma = q->gamma; p.beta = q->beta;
    p.x = q->x; p.xc = q->xc; p.s = q->s; p.mean = q->mean; p.rstd = q->rstd; p.bad = q->bad;
    p.V = q->V; p.Tt = q->Tt; p.B = q->B; p.L = q->L; p.ldc = q->xc ? q->ldc : 0; p.eps = eps;
    p.drop = bpm_make_drop(q->drop_p, seed, q->drop_site);
    const int R = q->B * q->L;
    const int span = p.ldc > d ? p.ldc : d;
    const unsigned grid = (unsigned)((R + 2 * WPB - 1) / (2 * WPB));
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* seedp = bpm_seed_ptr(seed);
#define BPM_EMB_FWD(NV)                                                                                              \
    if (span <= 256 * NV) {                                                                                          \
        if (dtype == BPM_BF16) hipLaunchKernelGGL((bert_embed_fwd_kernel<bf16_t, NV>), dim3(grid), dim3(NT), 0, s, p, d, seedp); \
        else hipLaunchKernelGGL((bert_embed_fwd_kernel<float, NV>), dim3(grid), dim3(NT), 0, s, p, d, seedp);        \
        BPM_CHECK_LAUNCH();                                                                                          \
        return 0;                                                                                                    \
    }
    BPM_EMB_FWD(1) BPM_EMB_FWD(2) BPM_EMB_FWD(3) BPM_EMB_FWD(4)
#undef BPM_EMB_FWD
    return BPM_ERR_ARG;
}

extern "C" size_t bpm_bert_embed_scatter_ws_bytes(int rows, int d, int type_rows) {
    if (rows < 1 || d < 1 || type_rows < 0) return 0;
    const size_t nchunk = ((size_t)rows + SC_CH - 1) / SC_CH, nblk = ((size_t)rows + SC_TROWS - 1) / SC_TROWS;
    return (2 * nchunk + nblk * (size_t)type_rows) * (size_t)d * sizeof(float);
}

extern "C" int bpm_bert_embed_scatter(const bpm_bert_scatter_problem* q, int d, void* stream) {
    if (!q || d < 32 || d % 32 || d > 1024) return BPM_ERR_ARG;
    if (!q->ds || q->B < 1 || q->L < 1) return BPM_ERR_ARG;
    if (!q->dword && !q->dpos && !q->dtype) return BPM_ERR_ARG;
    if (q->dword && (!q->sorted_ids || !q->perm || q->V < 1)) return BPM_ERR_ARG;
    if (q->dtype && q->Tt < 1) return BPM_ERR_ARG;
    const int R = q->B * q->L;
    if ((size_t)q->B * q->L > 0x7FFFFFFFull / 1024) return BPM_ERR_ARG;
    const size_t need = bpm_bert_embed_scatter_ws_bytes(R, d, q->dtype ? q->Tt : 0);
    if ((q->dword || q->dtype) && (!q->ws || q->ws_bytes < need)) return BPM_ERR_ARG;
    if (!al(q->ds, 16) || !al(q->dword, 16) || !al(q->dpos, 16) || !al(q->dtype, 16) || !al(q->ws, 16) || !al(q->sorted_ids, 8) ||
        !al(q->perm, 8) || !al(q->seg, 8))
        return BPM_ERR_ALIGN;
    EmbScP p;
    p.ds = q->ds; p.sid = q->sorted_ids; p.perm = q->perm; p.seg = q->seg;
    p.dword = q->dword; p.dpos = q->dpos; p.dtype = q->dtype;
    const int nchunk = (R + SC_CH - 1) / SC_CH, nblk = (R + SC_TROWS - 1) / SC_TROWS;
    p.ws_word = q->ws; p.ws_type = q->ws ? q->ws + (size_t)2 * nchunk * d : nullptr;
    p.V = q->V; p.Tt = q->Tt; p.B = q->B; p.L = q->L;
    p.pad_idx = q->padding_idx;
    hipStream_t s = (hipStream_t)stream;
    const int nch = d / 4;
#define BPM_EMB_SC(KERNEL, GRID)                                                                                     \
    do {                                                                                                             \
        if (d <= 256) hipLaunchKernelGGL((KERNEL<1>), dim3(GRID), dim3(NT), 0, s, p, d);                            \
        else if (d <= 512) hipLaunchKernelGGL((KERNEL<2>), dim3(GRID), dim3(NT), 0, s, p, d);                       \
        else if (d <= 768) hipLaunchKernelGGL((KERNEL<3>), dim3(GRID), dim3(NT), 0, s, p, d);                       \
        else hipLaunchKernelGGL((KERNEL<4>), dim3(GRID), dim3(NT), 0, s, p, d);                                     \
        BPM_CHECK_LAUNCH();                                                                                          \
    } while (0)
    p.nb_word = q->dword ? (unsigned)((R + WPB - 1) / WPB) : 0;
    p.nb_pos = q->dpos ? (unsigned)((q->L + WPB - 1) / WPB) : 0;
    p.nb_type = q->dtype ? (unsigned)nblk : 0;
    BPM_EMB_SC(bert_scatter1_kernel, p.nb_word + p.nb_pos + p.nb_type);
    // stage 2: runs that cross a chunk boundary (none when every chunk boundary separates two ids: still one tiny launch --
    // whether there are any is only known on the device) and the type table's partial rows
    p.nb_word = q->dword && nchunk > 1 ? (unsigned)((nchunk - 1 + WPB - 1) / WPB) : 0;
    p.nb_pos = 0;
    p.nb_type = q->dtype ? (unsigned)((q->Tt * nch + NT - 1) / NT) : 0;
    if (p.nb_word + p.nb_type) BPM_EMB_SC(bert_scatter2_kernel, p.nb_word + p.nb_type);
#undef BPM_EMB_SC
    return 0;
}

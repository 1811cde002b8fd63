// Embedding prologue, LayerNorm and the fused key / value source built from the two (gfx950).  HBM-bound row kernels,
// one wave per row; rows are [(t*B + b), d] fp32 on the residual stream and CT (f32 / bf16, leading dim padded to 32
// with zeros) where the consumer is an MFMA GEMM.  Per operation: problem struct, kernel(s), fill, choose, entry point.
#include "rows_common.h"

namespace {
// ---------------------------------------------------------------------------
// embedding prologue (reference transformer.py:66-79, position_embedding.py:62-76)
//   out = dropout(scale * x + table[pos]),  pos = t+1 if x[t,b,0] != 0 else 0
// backward: dx (+)= scale * drop_mult * dy   (the positional term is detached)
// ---------------------------------------------------------------------------
struct EmbP { const float* x; float* out; int T, B; int accumulate; int pos0, pstride; DropCfg drop; };

// four consecutive channels per lane (d % 4 == 0, 16-byte aligned tensors, < 2^32 elements): 32-bit index arithmetic, one
// dropout hash per quad, 16-byte accesses; the element-wise loops below are the general path
BPM_DEV bool emb_wide(const EmbP& P, const float* table, int d, size_t total) {
    return (d & 3) == 0 && total < (1ull << 32) && (((uintptr_t)P.x | (uintptr_t)P.out | (uintptr_t)table) & 15) == 0;
}

__global__ void embed_pos_fwd_kernel(const Grp<EmbP> grp, const float* __restrict__ table, int d, float scale) {
    unsigned bid = blockIdx.x, nblk;
    const EmbP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const size_t total = (size_t)P.T * P.B * d;
    if (emb_wide(P, table, d, total)) {
        const uint32_t total4 = (uint32_t)(total >> 2), ud = (uint32_t)d;
        for (uint32_t q = bid * NT + threadIdx.x; q < total4; q += nblk * NT) {
            const uint32_t i = 4u * q, row = i / ud, c = i - row * ud;
            const int t = (int)(row / (uint32_t)P.B);
            const int pos = (P.x[(size_t)row * ud] != 0.f) ? P.pos0 + t * P.pstride + 1 : 0;
            f32x4 v = scale * *(const f32x4*)(P.x + i) + *(const f32x4*)(table + (size_t)pos * ud + c);
            if (drop.thresh != 0) {
                float d0, d1, d2, d3;
                bpm_drop_mult4(drop, i, d0, d1, d2, d3);
                v *= f32x4{d0, d1, d2, d3};
            }
            *(f32x4*)(P.out + i) = v;
        }
        return;
    }
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const int c = (int)(i % d);
        const size_t row = i / d;
        const int t = (int)(row / P.B);
        const int pos = (P.x[row * d] != 0.f) ? P.pos0 + t * P.pstride + 1 : 0;     // row t sits at time pos0 + t*pstride
        P.out[i] = (scale * P.x[i] + table[(size_t)pos * d + c]) * bpm_drop_mult(drop, (uint32_t)i);
    }
}

__global__ void embed_pos_bwd_kernel(const Grp<EmbP> grp, int d, float scale) {
    unsigned bid = blockIdx.x, nblk;
    const EmbP& P = pick(grp, bid, nblk);      // x = dy, out = dx
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const size_t total = (size_t)P.T * P.B * d;
    if (emb_wide(P, nullptr, d, total)) {
        const uint32_t total4 = (uint32_t)(total >> 2);
        for (uint32_t q = bid * NT + threadIdx.x; q < total4; q += nblk * NT) {
            const uint32_t i = 4u * q;
            f32x4 v = scale * *(const f32x4*)(P.x + i);
            if (drop.thresh != 0) {
                float d0, d1, d2, d3;
                bpm_drop_mult4(drop, i, d0, d1, d2, d3);
                v *= f32x4{d0, d1, d2, d3};
            }
            f32x4* o = (f32x4*)(P.out + i);
            *o = P.accumulate ? *o + v : v;
        }
        return;
    }
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const float v = scale * P.x[i] * bpm_drop_mult(drop, (uint32_t)i);
        P.out[i] = P.accumulate ? P.out[i] + v : v;
    }
}
}  // namespace

static int fill_embed(Grp<EmbP>& g, const bpm_embed_problem* q, int n, int d, uint64_t seed) {
    if (!grp_begin(g, q, n, seed) || d < 1) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!q[i].x || !q[i].out || q[i].T < 1 || q[i].B < 1) return BPM_ERR_ARG;
        EmbP& p = g.p[i];
        p.x = q[i].x; p.out = q[i].out; p.T = q[i].T; p.B = q[i].B; p.accumulate = q[i].accumulate;
        if (q[i].pos0 < 0 || q[i].pos_stride < 0) return BPM_ERR_ARG;
        p.pos0 = q[i].pos0; p.pstride = q[i].pos_stride > 0 ? q[i].pos_stride : 1;
        p.drop = bpm_make_drop(q[i].drop_p, seed, q[i].drop_site);
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)p.T * p.B * d, NT * 4, CAP);
    }
    return 0;
}

extern "C" int bpm_embed_pos_fwd(const bpm_embed_problem* q, int n, const float* table, int table_rows, int d,
                                 float scale, uint64_t seed, void* stream) {
    Grp<EmbP> g;
    int rc = fill_embed(g, q, n, d, seed);
    if (rc) return rc;
    if (!table) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (table_rows < q[i].pos0 + (q[i].T - 1) * (q[i].pos_stride > 0 ? q[i].pos_stride : 1) + 2) return BPM_ERR_ARG;
    return launch<embed_pos_fwd_kernel>(g.blk0[n], NT, stream, g, table, d, scale);
}

extern "C" int bpm_embed_pos_bwd(const bpm_embed_problem* q, int n, int d, float scale, uint64_t seed, void* stream) {
    Grp<EmbP> g;
    int rc = fill_embed(g, q, n, d, seed);
    if (rc) return rc;
    return launch<embed_pos_bwd_kernel>(g.blk0[n], NT, stream, g, d, scale);
}

namespace {
// ---------------------------------------------------------------------------
// LayerNorm, eps inside the sqrt, biased variance (nn.LayerNorm).  One wave
// per row, row held in registers (NE = ceil(span/64) elements per lane).
// ---------------------------------------------------------------------------
constexpr int MAXE = 32;
constexpr int LN_WS_HEAD = 64;             // floats in front of the partial rows of a bpm_ln_bwd_ws workspace (ticket words)

struct LnP {
    const float* x; const float* gamma; const float* beta; void* out; int ldo; int out_f32;
    float* mean; float* rstd; int R;
    const float* dy; int ldy; const float* add; float* dx; float* dgamma; float* dbeta;
    void* cast; int ldc; float* csum; DropCfg drop;
};

template <typename CT, int NE>
__global__ __launch_bounds__(NT) void ln_fwd_kernel(const Grp<LnP> grp, int d, float eps) {
    unsigned bid = blockIdx.x, nblk;
    const LnP& P = pick(grp, bid, nblk);
    const int lane = threadIdx.x & 63;
    const int wpb = NT / 64;
    for (int row = bid * wpb + (threadIdx.x >> 6); row < P.R; row += nblk * wpb) {
        const float* xr = P.x + (size_t)row * d;
        float v[NE];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            v[e] = c < d ? xr[c] : 0.f;
            s += v[e];
        }
        const float mu = wave_sum(s) / d;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            const float t = c < d ? v[e] - mu : 0.f;
            q += t * t;
        }
        const float rs = rsqrtf(wave_sum(q) / d + eps);
        if (lane == 0) { P.mean[row] = mu; P.rstd[row] = rs; }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const float y = (v[e] - mu) * rs * P.gamma[c] + P.beta[c];
                if (P.out_f32) ((float*)P.out)[(size_t)row * P.ldo + c] = y;
                else put<CT>(P.out, (size_t)row * P.ldo + c, y);
            } else if (!P.out_f32 && c < P.ldo) {
                put<CT>(P.out, (size_t)row * P.ldo + c, 0.f);
            }
        }
    }
}

// dx = add + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma
// dgamma += sum_rows dy * xhat,  dbeta += sum_rows dy   (atomics, one per column per block)
// optional: cast[row, c] = CT(dx * dropout_mult(row*d + c)) (pad columns zeroed), csum += its column sums
// ln_bwd_kernel (below) with the atomics replaced by plain stores of the block's three partial rows, part[(block * 3 + a)
// * d .. + d) (a: dgamma, dbeta, cast sums), for col_finish_kernel (bpm_ln_bwd_det).  A copy of that kernel's body, kept
// expression for expression so that dx and the cast output are the same bits; the default kernel is left as it was, so
// that it compiles to the instructions it always did.
template <typename CT, int NE>
__global__ __launch_bounds__(NT) void ln_bwd_part_kernel(const Grp<LnP> grp, int d, float* part) {
    __shared__ float red[3][NT / 64][512];   // 512 columns per pass
    unsigned bid = blockIdx.x, nblk;
    const LnP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wpb = NT / 64;
    const bool fused = P.cast != nullptr;          // uniform per block
    float ag[NE], ab[NE], ac[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) { ag[e] = 0.f; ab[e] = 0.f; ac[e] = 0.f; }
    for (int row = bid * wpb + wv; row < P.R; row += nblk * wpb) {
        const float mu = P.mean[row], rs = P.rstd[row];
        const float* xr = P.x + (size_t)row * d;
        const float* gr = P.dy + (size_t)row * P.ldy;
        float xh[NE], gg[NE], av[NE];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const float dyv = gr[c];
                av[e] = P.add ? P.add[(size_t)row * d + c] : 0.f;
                xh[e] = (xr[c] - mu) * rs;
                gg[e] = dyv * P.gamma[c];
                ag[e] += dyv * xh[e];
                ab[e] += dyv;
                s1 += gg[e];
                s2 += gg[e] * xh[e];
            } else { xh[e] = 0.f; gg[e] = 0.f; av[e] = 0.f; }
        }
        s1 = wave_sum(s1) / d;
        s2 = wave_sum(s2) / d;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const float v = av[e] + rs * (gg[e] - s1 - xh[e] * s2);
                P.dx[(size_t)row * d + c] = v;
                if (fused) {
                    const float m = v * bpm_drop_mult(drop, (uint32_t)row * (uint32_t)d + (uint32_t)c);
                    put<CT>(P.cast, (size_t)row * P.ldc + c, m);
                    ac[e] += m;
                }
            } else if (fused && c < P.ldc) {
                put<CT>(P.cast, (size_t)row * P.ldc + c, 0.f);
            }
        }
    }
    const bool want_g = P.dgamma != nullptr, want_c = fused && P.csum != nullptr;
    if (!want_g && !want_c) return;     // uniform per block
#pragma unroll
    for (int e0 = 0; e0 < NE; e0 += 8) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool in = e0 + e < NE;
            const int ei = in ? e0 + e : 0;
            red[0][wv][lane + 64 * e] = in ? ag[ei] : 0.f;
            red[1][wv][lane + 64 * e] = in ? ab[ei] : 0.f;
            red[2][wv][lane + 64 * e] = in ? ac[ei] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 512; i += NT) {
            const int c = e0 * 64 + i;
            if (c < d) {
                float sg = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
                for (int w = 0; w < NT / 64; ++w) { sg += red[0][w][i]; sb += red[1][w][i]; sc += red[2][w][i]; }
                float* row = part + (size_t)blockIdx.x * 3 * d + c;
                row[0] = sg; row[d] = sb; row[2 * d] = sc;
            }
        }
    }
}

template <typename CT, int NE>
__global__ __launch_bounds__(NT) void ln_bwd_kernel(const Grp<LnP> grp, int d) {
    __shared__ float red[3][NT / 64][512];   // 512 columns per pass
    unsigned bid = blockIdx.x, nblk;
    const LnP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wpb = NT / 64;
    const bool fused = P.cast != nullptr;          // uniform per block
    float ag[NE], ab[NE], ac[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) { ag[e] = 0.f; ab[e] = 0.f; ac[e] = 0.f; }
    for (int row = bid * wpb + wv; row < P.R; row += nblk * wpb) {
        const float mu = P.mean[row], rs = P.rstd[row];
        const float* xr = P.x + (size_t)row * d;
        const float* gr = P.dy + (size_t)row * P.ldy;
        float xh[NE], gg[NE], av[NE];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const float dyv = gr[c];
                av[e] = P.add ? P.add[(size_t)row * d + c] : 0.f;
                xh[e] = (xr[c] - mu) * rs;
                gg[e] = dyv * P.gamma[c];
                ag[e] += dyv * xh[e];
                ab[e] += dyv;
                s1 += gg[e];
                s2 += gg[e] * xh[e];
            } else { xh[e] = 0.f; gg[e] = 0.f; av[e] = 0.f; }
        }
        s1 = wave_sum(s1) / d;
        s2 = wave_sum(s2) / d;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const float v = av[e] + rs * (gg[e] - s1 - xh[e] * s2);
                P.dx[(size_t)row * d + c] = v;
                if (fused) {
                    const float m = v * bpm_drop_mult(drop, (uint32_t)row * (uint32_t)d + (uint32_t)c);
                    put<CT>(P.cast, (size_t)row * P.ldc + c, m);
                    ac[e] += m;
                }
            } else if (fused && c < P.ldc) {
                put<CT>(P.cast, (size_t)row * P.ldc + c, 0.f);
            }
        }
    }
    const bool want_g = P.dgamma != nullptr, want_c = fused && P.csum != nullptr;
    if (!want_g && !want_c) return;     // uniform per block
#pragma unroll
    for (int e0 = 0; e0 < NE; e0 += 8) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool in = e0 + e < NE;
            const int ei = in ? e0 + e : 0;
            red[0][wv][lane + 64 * e] = in ? ag[ei] : 0.f;
            red[1][wv][lane + 64 * e] = in ? ab[ei] : 0.f;
            red[2][wv][lane + 64 * e] = in ? ac[ei] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 512; i += NT) {
            const int c = e0 * 64 + i;
            if (c < d) {
                float sg = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
                for (int w = 0; w < NT / 64; ++w) { sg += red[0][w][i]; sb += red[1][w][i]; sc += red[2][w][i]; }
                if (want_g) { atomicAdd(P.dgamma + c, sg); atomicAdd(P.dbeta + c, sb); }
                if (want_c) atomicAdd(P.csum + c, sc);
            }
        }
    }
}


// ---------------------------------------------------------------------------
// Vector forms (d % 4 == 0, 16-byte aligned rows): a lane owns 4-column chunks lane, lane+64, ... (NV of them),
// moved as one 16-byte (f32) / 8-byte (bf16) access each; the backward keeps TWO rows in flight per wave.
// ---------------------------------------------------------------------------
BPM_DEV float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

template <typename CT, int NV>
__global__ __launch_bounds__(NT) void ln_fwd_vec_kernel(const Grp<LnP> grp, int d, float eps) {
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    unsigned bid = blockIdx.x, nblk;
    const LnP& P = pick(grp, bid, nblk);
    const int lane = threadIdx.x & 63;
    const int wpb = NT / 64;
    const int nch = d >> 2;
    f32x4 gam[NV], bet[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        const bool in = q < nch;
        gam[e] = *(const f32x4*)(P.gamma + 4 * (in ? q : 0));
        bet[e] = *(const f32x4*)(P.beta + 4 * (in ? q : 0));
    }
    const float inv_d = 1.f / d;
    for (int row = bid * wpb + (threadIdx.x >> 6); row < P.R; row += nblk * wpb) {
        const float* xr = P.x + (size_t)row * d;
        f32x4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = lane + 64 * e;
            const f32x4 t = *(const f32x4*)(xr + 4 * (q < nch ? q : 0));
            v[e] = q < nch ? t : f32x4{0.f, 0.f, 0.f, 0.f};
            s += sum4(v[e]);
        }
        const float mu = wave_sum(s) * inv_d;
        float qq = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = lane + 64 * e;
            f32x4 t = v[e] - mu;
            if (q >= nch) t = f32x4{0.f, 0.f, 0.f, 0.f};
            v[e] = t;
            qq += sum4(t * t);
        }
        const float rs = rsqrtf(wave_sum(qq) * inv_d + eps);
        if (lane == 0) { P.mean[row] = mu; P.rstd[row] = rs; }
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = lane + 64 * e;
            if (q < nch) {
                const f32x4 y = v[e] * rs * gam[e] + bet[e];
                if (P.out_f32) *(f32x4*)((float*)P.out + (size_t)row * P.ldo + 4 * q) = y;
                else put4<CT>(P.out, (size_t)row * P.ldo + 4 * q, y);
            } else if (!P.out_f32 && 4 * q < P.ldo) {
                put4<CT>(P.out, (size_t)row * P.ldo + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});
            }
        }
    }
}

template <typename CT, int NV>
__global__ __launch_bounds__(NT) void ln_bwd_vec_kernel(const Grp<LnP> grp, int d, float* __restrict__ ws) {
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    __shared__ float red[3][NT / 64][NV * 256];
    unsigned bid = blockIdx.x, nblk;
    const LnP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wpb = NT / 64;
    const int nch = d >> 2;
    const bool fused = P.cast != nullptr;          // uniform per block
    const bool has_add = P.add != nullptr;
    const float inv_d = 1.f / d;
    f32x4 gam[NV], ag[NV], ab[NV], ac[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        gam[e] = *(const f32x4*)(P.gamma + 4 * (q < nch ? q : 0));
        ag[e] = ab[e] = ac[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    constexpr int U = 2;                             // rows in flight per wave
    for (int row0 = (bid * wpb + wv) * U; row0 < P.R; row0 += nblk * wpb * U) {
        f32x4 xv[U][NV], gv[U][NV], av[U][NV];
        float mu[U], rs[U];
        // phase 1: every load of the U rows (clamped rows / chunks, zeroed by selects)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            const int rc = row < P.R ? row : row0;
            mu[u] = P.mean[rc]; rs[u] = P.rstd[rc];
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const int qc = q < nch ? q : 0;
                xv[u][e] = *(const f32x4*)(P.x + (size_t)rc * d + 4 * qc);
                gv[u][e] = *(const f32x4*)(P.dy + (size_t)rc * P.ldy + 4 * qc);
                av[u][e] = has_add ? *(const f32x4*)(P.add + (size_t)rc * d + 4 * qc) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            const bool rok = row < P.R;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const bool ok = rok && q < nch;
                const f32x4 dyv = ok ? gv[u][e] : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 xh = ok ? (xv[u][e] - mu[u]) * rs[u] : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 g = dyv * gam[e];
                ag[e] += dyv * xh;
                ab[e] += dyv;
                s1 += sum4(g);
                s2 += sum4(g * xh);
                xv[u][e] = xh; gv[u][e] = g;
            }
            s1 = wave_sum(s1) * inv_d;
            s2 = wave_sum(s2) * inv_d;
            if (!rok) continue;                      // wave-uniform
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                if (q < nch) {
                    const f32x4 v = av[u][e] + rs[u] * (gv[u][e] - s1 - xv[u][e] * s2);
                    *(f32x4*)(P.dx + (size_t)row * d + 4 * q) = v;
                    if (fused) {
                        f32x4 m = v;
                        if (drop.thresh != 0) {   // row*d + 4q is a multiple of 4 (d % 4 == 0): one hash quad
                            float d0, d1, d2, d3;
                            const uint32_t i0 = (uint32_t)row * (uint32_t)d + 4u * (uint32_t)q;
                            bpm_drop_mult4(drop, i0, d0, d1, d2, d3);
                            m[0] *= d0; m[1] *= d1; m[2] *= d2; m[3] *= d3;
                        }
                        put4<CT>(P.cast, (size_t)row * P.ldc + 4 * q, m);
                        ac[e] += m;
                    }
                } else if (fused && 4 * q < P.ldc) {
                    put4<CT>(P.cast, (size_t)row * P.ldc + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});
                }
            }
        }
    }
    const bool want_g = P.dgamma != nullptr, want_c = fused && P.csum != nullptr;
    if (!want_g && !want_c) return;                  // uniform per block
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        *(f32x4*)(&red[0][wv][4 * (lane + 64 * e)]) = ag[e];
        *(f32x4*)(&red[1][wv][4 * (lane + 64 * e)]) = ab[e];
        *(f32x4*)(&red[2][wv][4 * (lane + 64 * e)]) = ac[e];
    }
    __syncthreads();
    // Per-block column sums.  With a workspace every block stores its three rows and the LAST block of the problem to
    // finish adds them up (one owner per column, fixed order: bitwise reproducible) -- no second launch: a tiny dependent
    // kernel behind this one waited ~45 us for CU slots beside the side stream's GEMMs.  Without a workspace they go out
    // as float atomics -- up to 128 blocks per problem adding into the same three 3 KB rows, which runs an order of
    // magnitude below the atomic rate (MI355X_MICROARCH, global float atomics, contention row).
    // Hand-off (cdna_hip_programming.md Guideline 16 R1, counter form): partial rows stored write-through -> every wave's
    // stores drained -> workgroup barrier -> ticket by one lane; the block that draws the last ticket acquires (agent
    // scope: invalidates this CU's L1) and reads the other blocks' rows.  The ticket word is reset by its last
    // user, so the workspace only has to be zero when it is created.
    if (ws) {
        __shared__ int s_last;
        unsigned* cnt = (unsigned*)ws;                       // BPM_MAX_GROUP tickets, then the partial rows
        float* rows = ws + LN_WS_HEAD;
        // partial rows go out WRITE-THROUGH (sc1, 16 bytes per lane): no release fence is needed then -- an agent-scope
        // release (buffer_wbl2) per block would write back the whole L2's dirty dx lines, measured +50 us per launch
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(rows + (size_t)blockIdx.x * 3 * d), 0, 3 * d * 4, 0x00020000);
        for (int v = threadIdx.x; v < 3 * nch; v += NT) {
            const int a = v / nch, c = 4 * (v - a * nch);
            f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) s4 += *(const f32x4*)(&red[a][w][c]);
            __builtin_amdgcn_raw_buffer_store_b128((u32x4&)s4, rw, (a * d + c) * 4, 0, 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int pi = 0;                                          // (not &P - grp.p: taking that address sends the kernel arguments to scratch)
#pragma unroll 1
        for (int i = 1; i < grp.n; ++i)
            if (blockIdx.x >= grp.blk0[i]) pi = i;
        if (threadIdx.x == 0) {
            const unsigned ticket = __hip_atomic_fetch_add(cnt + pi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = ticket == nblk - 1;
            if (s_last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(cnt + pi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (!s_last) return;
        // 3 d / 4 four-column slots (array a, columns 4 c4 ..), 16 partial rows in flight per thread
        const float* first = rows + (size_t)grp.blk0[pi] * 3 * d;
        const int nslot = 3 * nch;
        for (int v = threadIdx.x; v < nslot; v += NT) {
            const int a = v / nch, c4 = v - a * nch;
            if ((a < 2 && !want_g) || (a == 2 && !want_c)) continue;
            const float* src = first + a * d + 4 * c4;
            f32x4 acc4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
            for (unsigned b = 0; b < nblk; ++b) acc4 += *(const f32x4*)(src + (size_t)b * 3 * d);
            float* dst = (a == 0 ? P.dgamma : a == 1 ? P.dbeta : P.csum) + 4 * c4;
            *(f32x4*)dst = *(const f32x4*)dst + acc4;
        }
        return;
    }
    for (int c = threadIdx.x; c < d; c += NT) {
        float sg = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) { sg += red[0][w][c]; sb += red[1][w][c]; sc += red[2][w][c]; }
        if (want_g) { atomicAdd(P.dgamma + c, sg); atomicAdd(P.dbeta + c, sb); }
        if (want_c) atomicAdd(P.csum + c, sc);
    }
}
}  // namespace

// checks and copies the problems; their block counts follow from the choice (ln_blocks)
static int fill_ln(Grp<LnP>& g, const bpm_ln_problem* q, int n, int d, bool bwd, uint64_t seed = 0) {
    if (!grp_begin(g, q, n, seed) || d < 1 || d > 64 * MAXE) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_ln_problem& s = q[i];
        LnP& p = g.p[i];
        if (!s.x || !s.gamma || !s.mean || !s.rstd || s.R < 1) return BPM_ERR_ARG;
        if (bwd) {
            if (!s.dy || !s.dx || s.ldy < d || ((s.dgamma == nullptr) != (s.dbeta == nullptr))) return BPM_ERR_ARG;
            if (s.cast && (s.ldc < d || s.ldc > 64 * ((d + 63) / 64))) return BPM_ERR_ARG;
            if (!s.cast && s.cast_colsum) return BPM_ERR_ARG;
        } else {
            if (!s.beta || !s.out || s.ldo < d || s.ldo > 64 * MAXE) return BPM_ERR_ARG;
        }
        p.x = s.x; p.gamma = s.gamma; p.beta = s.beta; p.out = s.out; p.ldo = s.ldo; p.out_f32 = s.out_f32;
        p.mean = s.mean; p.rstd = s.rstd; p.R = s.R;
        p.dy = s.dy; p.ldy = s.ldy; p.add = s.add; p.dx = s.dx; p.dgamma = s.dgamma; p.dbeta = s.dbeta;
        p.cast = bwd ? s.cast : nullptr; p.ldc = s.ldc; p.csum = s.cast_colsum;
        p.drop = bpm_make_drop(bwd && s.cast ? s.drop_p : 0.f, seed, s.drop_site);
    }
    return 0;
}

// vector kernels: d % 4 == 0, every row 16-byte (CT outputs: 8-byte) aligned
static bool ln_vec_ok(const bpm_ln_problem* q, int n, int d, bool bwd, int ct_size) {
    if (d % 4 || d > 4 * 64 * 4) return false;
    for (int i = 0; i < n; ++i) {
        const bpm_ln_problem& s = q[i];
        uintptr_t a = (uintptr_t)s.x | (uintptr_t)s.gamma;
        if (bwd) {
            a |= (uintptr_t)s.dy | (uintptr_t)s.add | (uintptr_t)s.dx;
            if (s.ldy % 4) return false;
            if (s.cast && (((uintptr_t)s.cast % (4 * ct_size)) || s.ldc % 4)) return false;
        } else {
            a |= (uintptr_t)s.beta;
            if (s.ldo % 4 || ((uintptr_t)s.out % (4 * (s.out_f32 ? 4 : ct_size)))) return false;
        }
        if (a & 15) return false;
    }
    return true;
}

// What is decided before a LayerNorm launch.
struct LnChoice {
    bool vec;         // ln_*_vec_kernel<CT, NV> (VecWidths) or ln_*_kernel<CT, NE> (RowWidths)
    int span;         // columns a wave has to cover: the first width of the family's list that does is launched
    int rows; unsigned cap;     // a problem of R rows gets ceil(R / rows) blocks, at most cap
    float* ws;        // backward: the partial-row workspace, or null: column sums by float atomics
};

static void ln_blocks(Grp<LnP>& g, const LnChoice& c) {
    for (int i = 0; i < g.n; ++i) g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)g.p[i].R, c.rows, c.cap);
}

static LnChoice choose_ln_fwd(const bpm_ln_problem* q, int n, int d, int ct_size) {
    int span = d;                                    // a CT row is written up to its zero pad: the wave covers ldo columns
    for (int i = 0; i < n; ++i)
        if (!q[i].out_f32 && q[i].ldo > span) span = q[i].ldo;
    return LnChoice{ln_vec_ok(q, n, d, false, ct_size) && span <= 4 * 64 * 4, span, 4, 4096, nullptr};
}

extern "C" int bpm_ln_fwd(int dtype, const bpm_ln_problem* q, int n, int d, float eps, void* stream) {
    Grp<LnP> g;
    if (const int rc = fill_ln(g, q, n, d, false)) return rc;
    const LnChoice c = choose_ln_fwd(q, n, d, dtype == BPM_BF16 ? 2 : 4);
    ln_blocks(g, c);
    return with_ct(dtype, [&](auto ct) {
        using CT = decltype(ct);
        if (c.vec) return with_width(VecWidths(), c.span, [&](auto w) {
            return launch<ln_fwd_vec_kernel<CT, decltype(w)::value>>(g.blk0[n], NT, stream, g, d, eps);
        });
        return with_width(RowWidths(), c.span, [&](auto w) {
            return launch<ln_fwd_kernel<CT, decltype(w)::value>>(g.blk0[n], NT, stream, g, d, eps);
        });
    });
}

extern "C" size_t bpm_ln_bwd_ws_bytes(int n, int d) {
    return ((size_t)(n > 0 ? n : 0) * 128 * 3 * (size_t)(d > 0 ? d : 0) + LN_WS_HEAD) * sizeof(float);
}

// BPM_ERR_ARG: the workspace route is taken and the workspace is misaligned or too small.
static int choose_ln_bwd(const bpm_ln_problem* q, int n, int d, int ct_size, void* ws, size_t ws_bytes, LnChoice& c) {
    c = LnChoice{false, d, 4, 256, nullptr};
    if (!ln_vec_ok(q, n, d, true, ct_size)) return 0;
    // two rows per wave and iteration: half the blocks of the scalar kernel
    // at most 64 blocks per problem (= partial rows the last block sums): 128 took 78 / 98 us stand-alone at hidden 768,
    // six problems (with parameter gradients / with the fused cast), 64 takes 72 / 88
    c = LnChoice{true, d, 8, 64, nullptr};
    bool sums = false;
    for (int i = 0; i < n; ++i) {
        if (q[i].cast && q[i].ldc > c.span) c.span = q[i].ldc;
        sums = sums || q[i].dgamma || (q[i].cast && q[i].cast_colsum);
        if (((uintptr_t)q[i].dgamma | (uintptr_t)q[i].dbeta | (uintptr_t)q[i].cast_colsum) & 15) ws = nullptr;   // 16-byte row sums
    }
    // the last block of a problem adds its partial rows to dgamma / dbeta / cast_colsum with a plain read-modify-write:
    // exact only while no other problem of this launch owns the same row (and, host contract, no other stream
    // accumulates into it while this launch runs: include/bpmult_hip.h).  Shared rows go out as float atomics.
    if (ws && sums) {
        const float* rows[3 * BPM_MAX_GROUP];
        int nr = 0;
        for (int i = 0; i < n; ++i) {
            if (q[i].dgamma) { rows[nr++] = q[i].dgamma; rows[nr++] = q[i].dbeta; }
            if (q[i].cast && q[i].cast_colsum) rows[nr++] = q[i].cast_colsum;
        }
        for (int a = 0; a < nr && ws; ++a)
            for (int b = a + 1; b < nr; ++b)
                if (rows[a] && rows[a] == rows[b]) { ws = nullptr; break; }
    }
    if (ws && sums) {
        size_t blocks = 0;
        for (int i = 0; i < n; ++i) blocks += blocks_for((size_t)q[i].R, c.rows, c.cap);
        if (((uintptr_t)ws & 15) || ws_bytes < (blocks * 3 * d + LN_WS_HEAD) * sizeof(float)) return BPM_ERR_ARG;
        c.ws = (float*)ws;
    }
    return 0;
}

// strict (bpm_ln_bwd_det): a launch whose column sums would go out as float atomics is refused
static int ln_bwd_entry(int dtype, const bpm_ln_problem* q, int n, int d, uint64_t seed, void* ws, size_t ws_bytes, bool strict,
                        void* stream) {
    if (dtype != BPM_F32 && dtype != BPM_BF16) return BPM_ERR_ARG;
    Grp<LnP> g;
    if (const int rc = fill_ln(g, q, n, d, true, seed)) return rc;
    LnChoice c;
    if (const int rc = choose_ln_bwd(q, n, d, dtype == BPM_BF16 ? 2 : 4, ws, ws_bytes, c)) return rc;
    bool sums = false;
    for (int i = 0; i < n; ++i) sums = sums || q[i].dgamma || (q[i].cast && q[i].cast_colsum);
    if (strict && sums && !c.ws) {
        // what bpm_ln_bwd_ws sends to float atomics -- the scalar family (d % 4 != 0, d > 1024), a misaligned row, problems
        // that share a gradient row: the scalar kernel with partial rows, then col_finish_kernel (problem order, block order)
        c = LnChoice{false, d, 4, 256, nullptr};
        ln_blocks(g, c);
        if (!ws || ((uintptr_t)ws & 15) || ws_bytes < ((size_t)g.blk0[n] * 3 * d + LN_WS_HEAD) * sizeof(float)) return BPM_ERR_ARG;
        float* part = (float*)ws + LN_WS_HEAD;
        ColFin f;
        fin_begin(f, n, d, g.blk0);
        for (int i = 0; i < n; ++i) {
            fin_add(f, i, 0, q[i].dgamma);
            fin_add(f, i, 1, q[i].dbeta);
            fin_add(f, i, 2, q[i].cast ? q[i].cast_colsum : nullptr);
        }
        const int rc = with_ct(dtype, [&](auto ct) {
            using CT = decltype(ct);
            return with_width(RowWidths(), c.span, [&](auto w) {
                return launch<ln_bwd_part_kernel<CT, decltype(w)::value>>(g.blk0[n], NT, stream, g, d, part);
            });
        });
        return rc ? rc : launch<col_finish_kernel<FIN_ARR>>((unsigned)f.nown, NT, stream, f, (const float*)part);
    }
    ln_blocks(g, c);
    return with_ct(dtype, [&](auto ct) {
        using CT = decltype(ct);
        if (c.vec) return with_width(VecWidths(), c.span, [&](auto w) {
            return launch<ln_bwd_vec_kernel<CT, decltype(w)::value>>(g.blk0[n], NT, stream, g, d, c.ws);
        });
        return with_width(RowWidths(), c.span, [&](auto w) {
            return launch<ln_bwd_kernel<CT, decltype(w)::value>>(g.blk0[n], NT, stream, g, d);
        });
    });
}

extern "C" int bpm_ln_bwd_ws(int dtype, const bpm_ln_problem* q, int n, int d, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    return ln_bwd_entry(dtype, q, n, d, seed, ws, ws_bytes, false, stream);
}

// what either route of bpm_ln_bwd_det needs at most: 256 blocks per problem (the scalar kernel's cap), three rows each
extern "C" size_t bpm_ln_bwd_det_ws_bytes(int n, int d) {
    return ((size_t)(n > 0 ? n : 0) * 256 * 3 * (size_t)(d > 0 ? d : 0) + LN_WS_HEAD) * sizeof(float);
}

extern "C" int bpm_ln_bwd_det(int dtype, const bpm_ln_problem* q, int n, int d, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    return ln_bwd_entry(dtype, q, n, d, seed, ws, ws_bytes, true, stream);
}

extern "C" int bpm_ln_bwd(int dtype, const bpm_ln_problem* q, int n, int d, uint64_t seed, void* stream) {
    return bpm_ln_bwd_ws(dtype, q, n, d, seed, nullptr, 0, stream);
}

namespace {
// ---------------------------------------------------------------------------
// Key / value source of a crossmodal encoder in ONE pass per direction: embed_pos_fwd -> affine-free ln_fwd, and
// ln_bwd -> embed_pos_bwd (-> the dxk + dxv sum), without the fp32 [S B, d] tensors ke / ve / dke / dve in between.
// The source is the same tensor for K and V at every call site of the model: it is read once, embedded with the two
// sites' dropout masks, and both rows are normalised from registers; the backward recomputes the embedded rows from
// the source (the dropout hash per quad is the one the embedding backward draws anyway).
// One wave per row, a lane owns the 4-column chunks lane + 64 e as in the vector LayerNorm kernels.  Every value that
// the two-kernel route rounds to fp32 in memory is kept from being contracted into a neighbouring operation here
// (kv_opaque), and the expressions are those of embed_pos_*_kernel / ln_*_vec_kernel: the results are the same bits.
// ---------------------------------------------------------------------------
struct KvP {
    const float* xk; const float* xv; int T, B, pos0, pstride; DropCfg dk, dv;
    void* khat; void* vhat; int ld; float* mk; float* rk; float* mv; float* rv;
    const float* gk; const float* gv; float* dxk; float* dxv;
};

BPM_DEV f32x4 kv_opaque(f32x4 v) {
    asm("" : "+v"(v));
    return v;
}

BPM_DEV float kv_opaque1(float v) {
    asm("" : "+v"(v));
    return v;
}
BPM_DEV f32x4 kv_fma4(f32x4 a, f32x4 b, f32x4 c) {
    return f32x4{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1]), __builtin_fmaf(a[2], b[2], c[2]), __builtin_fmaf(a[3], b[3], c[3])};
}

// dropout(scale * x + table[pos]) of the quad at element index i0 (embed_pos_fwd_kernel, wide path); mult: its dropout factors
BPM_DEV f32x4 kv_embed4(f32x4 x, f32x4 tab, float scale, const DropCfg& drop, uint32_t i0, f32x4& mult) {
    f32x4 v = scale * x + tab;
    mult = f32x4{1.f, 1.f, 1.f, 1.f};
    if (drop.thresh != 0) {
        float d0, d1, d2, d3;
        bpm_drop_mult4(drop, i0, d0, d1, d2, d3);
        mult = f32x4{d0, d1, d2, d3};
        v *= mult;
    }
    return kv_opaque(v);
}

// ln_fwd_vec_kernel's row body with gamma = 1, beta = 0
template <typename CT, int NV>
BPM_DEV void kv_norm_store(f32x4 (&v)[NV], int lane, int nch, float inv_d, float eps, int row, void* out, int ld, float* mean, float* rstd) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) s += sum4(v[e]);
    const float mu = wave_sum(s) * inv_d;
    float qq = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        f32x4 t = v[e] - mu;
        if (q >= nch) t = f32x4{0.f, 0.f, 0.f, 0.f};
        v[e] = t;
        qq += sum4(t * t);
    }
    const float rs = rsqrtf(wave_sum(qq) * inv_d + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int q = lane + 64 * e;
        if (q < nch) put4<CT>(out, (size_t)row * ld + 4 * q, v[e] * rs + 0.f);
        else if (4 * q < ld) put4<CT>(out, (size_t)row * ld + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});
    }
}

template <typename CT, int NV>
__global__ __launch_bounds__(NT) void kv_source_fwd_kernel(const Grp<KvP> grp, const float* __restrict__ table, int d, float scale, float eps) {
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    unsigned bid = blockIdx.x, nblk;
    const KvP& P = pick(grp, bid, nblk);
    const DropCfg dk = bpm_resolve_drop(P.dk, grp.seedp), dv = bpm_resolve_drop(P.dv, grp.seedp);
    const int lane = threadIdx.x & 63;
    const int wpb = NT / 64;
    const int nch = d >> 2, R = P.T * P.B;
    const bool same = P.xk == P.xv;                  // uniform per block
    const float inv_d = 1.f / d;
    for (int row = bid * wpb + (threadIdx.x >> 6); row < R; row += nblk * wpb) {
        const int t = row / P.B;
        const uint32_t r0 = (uint32_t)row * (uint32_t)d;
        const float* xkr = P.xk + r0;
        const float* xvr = P.xv + r0;
        const int posk = xkr[0] != 0.f ? P.pos0 + t * P.pstride + 1 : 0;
        const int posv = same ? posk : xvr[0] != 0.f ? P.pos0 + t * P.pstride + 1 : 0;
        const float* tk = table + (size_t)posk * d;
        const float* tv = table + (size_t)posv * d;
        f32x4 ek[NV], ev[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = lane + 64 * e;
            const int qc = q < nch ? q : 0;
            const f32x4 xk4 = *(const f32x4*)(xkr + 4 * qc), tk4 = *(const f32x4*)(tk + 4 * qc);
            f32x4 xv4 = xk4, tv4 = tk4, m;
            if (!same) { xv4 = *(const f32x4*)(xvr + 4 * qc); tv4 = *(const f32x4*)(tv + 4 * qc); }
            const f32x4 a = kv_embed4(xk4, tk4, scale, dk, r0 + 4u * (uint32_t)qc, m);
            const f32x4 b = kv_embed4(xv4, tv4, scale, dv, r0 + 4u * (uint32_t)qc, m);
            ek[e] = q < nch ? a : f32x4{0.f, 0.f, 0.f, 0.f};
            ev[e] = q < nch ? b : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        kv_norm_store<CT, NV>(ek, lane, nch, inv_d, eps, row, P.khat, P.ld, P.mk, P.rk);
        kv_norm_store<CT, NV>(ev, lane, nch, inv_d, eps, row, P.vhat, P.ld, P.mv, P.rv);
    }
}

// dx = scale * drop * rstd * (g - mean(g) - xhat * mean(g * xhat)) for the K and the V side of each row (ln_bwd_vec_kernel
// without affine, add or column sums, then embed_pos_bwd_kernel); merged: their fp32 sum goes to dxk.  SAME: every problem
// of the launch has xk == xv -- one source row serves both sides and two rows are in flight per wave; otherwise the two
// rows in flight are the K and the V source row.
template <int NV, bool SAME>
__global__ __launch_bounds__(NT) void kv_source_bwd_kernel(const Grp<KvP> grp, const float* __restrict__ table, int d, float scale) {
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    constexpr int U = SAME ? 2 : 1;                  // rows in flight per wave
    constexpr int NS = SAME ? 1 : 2;                 // source rows loaded per row
    unsigned bid = blockIdx.x, nblk;
    const KvP& P = pick(grp, bid, nblk);
    const DropCfg dk = bpm_resolve_drop(P.dk, grp.seedp), dv = bpm_resolve_drop(P.dv, grp.seedp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wpb = NT / 64;
    const int nch = d >> 2, R = P.T * P.B;
    const bool merge = P.dxv == nullptr || P.dxv == P.dxk;       // uniform per block
    const float inv_d = 1.f / d;
    for (int row0 = (bid * wpb + wv) * U; row0 < R; row0 += nblk * wpb * U) {
        f32x4 xs[U][NS][NV], tb[U][NS][NV], g[U][2][NV];
        float mu[U][2], rs[U][2];
        // phase 1: every load of the rows in flight (clamped rows / chunks, zeroed by selects)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            const int rc = row < R ? row : row0;
            const int t = rc / P.B;
            const uint32_t r0 = (uint32_t)rc * (uint32_t)d;
            mu[u][0] = P.mk[rc]; rs[u][0] = P.rk[rc];
            mu[u][1] = P.mv[rc]; rs[u][1] = P.rv[rc];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float* xr = (s ? P.xv : P.xk) + r0;
                const int pos = xr[0] != 0.f ? P.pos0 + t * P.pstride + 1 : 0;
                const float* tr = table + (size_t)pos * d;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int q = lane + 64 * e;
                    const int qc = q < nch ? q : 0;
                    xs[u][s][e] = *(const f32x4*)(xr + 4 * qc);
                    tb[u][s][e] = *(const f32x4*)(tr + 4 * qc);
                }
            }
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                const int qc = q < nch ? q : 0;
                g[u][0][e] = *(const f32x4*)(P.gk + r0 + 4 * qc);
                g[u][1][e] = *(const f32x4*)(P.gv + r0 + 4 * qc);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            const bool rok = row < R;
            const uint32_t r0 = (uint32_t)(rok ? row : row0) * (uint32_t)d;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int s = SAME ? 0 : side;
                const DropCfg& drop = side ? dv : dk;
                f32x4 xh[NV], mult[NV];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int q = lane + 64 * e;
                    const bool ok = rok && q < nch;
                    const f32x4 emb = kv_embed4(xs[u][s][e], tb[u][s][e], scale, drop, r0 + 4u * (uint32_t)(q < nch ? q : 0), mult[e]);
                    const f32x4 dyv = ok ? g[u][side][e] : f32x4{0.f, 0.f, 0.f, 0.f};
                    xh[e] = ok ? (emb - mu[u][side]) * rs[u][side] : f32x4{0.f, 0.f, 0.f, 0.f};
                    s1 += sum4(dyv);
                    s2 += sum4(dyv * xh[e]);
                    g[u][side][e] = dyv;
                }
                // The roundings of g - mean(g) - xhat * mean(g xhat) are spelled out as ln_bwd_vec_kernel<., NV> is compiled:
                // xhat * mean(g xhat) and the product with rstd are fused everywhere; mean(g) = sum / d is rounded before it
                // is subtracted, except at NV == 1, where the division is fused into the subtraction.
                s1 = wave_sum(s1);
                if constexpr (NV != 1) s1 = kv_opaque1(s1 * inv_d);
                s2 = kv_opaque1(wave_sum(s2) * inv_d);
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    f32x4 t = NV == 1 ? kv_fma4(f32x4{-inv_d, -inv_d, -inv_d, -inv_d}, f32x4{s1, s1, s1, s1}, g[u][side][e]) : g[u][side][e] - s1;
                    t = kv_fma4(-xh[e], f32x4{s2, s2, s2, s2}, kv_opaque(t));
                    const f32x4 rs4 = f32x4{rs[u][side], rs[u][side], rs[u][side], rs[u][side]};
                    const f32x4 dl = kv_opaque(kv_fma4(rs4, t, f32x4{0.f, 0.f, 0.f, 0.f}));                  // = dke / dve
                    f32x4 v = scale * dl;
                    if (drop.thresh != 0) v *= mult[e];
                    g[u][side][e] = kv_opaque(v);
                }
            }
            if (!rok) continue;                      // wave-uniform
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int q = lane + 64 * e;
                if (q < nch) {
                    if (merge) {
                        *(f32x4*)(P.dxk + r0 + 4 * q) = g[u][0][e] + g[u][1][e];
                    } else {
                        *(f32x4*)(P.dxk + r0 + 4 * q) = g[u][0][e];
                        *(f32x4*)(P.dxv + r0 + 4 * q) = g[u][1][e];
                    }
                }
            }
        }
    }
}
}  // namespace

// Domain of the fused key / value source kernels (the wide paths of the kernels they replace): d % 4 == 0, d <= 1024,
// 16-byte aligned fp32 tensors, fewer than 2^32 elements per tensor.
static int fill_kv(Grp<KvP>& g, const bpm_kv_source_problem* q, int n, const float* table, int table_rows, int d, uint64_t seed,
                   bool bwd, int ct_size) {
    if (!grp_begin(g, q, n, seed) || !table || d < 4 || d % 4 || d > 4 * 64 * 4 || ((uintptr_t)table & 15)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_kv_source_problem& s = q[i];
        if (!s.xk || !s.xv || s.T < 1 || s.B < 1 || s.pos0 < 0 || s.pos_stride < 0) return BPM_ERR_ARG;
        if (!s.mean_k || !s.rstd_k || !s.mean_v || !s.rstd_v) return BPM_ERR_ARG;
        const int pstride = s.pos_stride > 0 ? s.pos_stride : 1;
        if ((long long)table_rows < (long long)s.pos0 + (long long)(s.T - 1) * pstride + 2) return BPM_ERR_ARG;
        if ((unsigned long long)s.T * (unsigned long long)s.B * (unsigned long long)d >= (1ull << 32)) return BPM_ERR_ARG;
        uintptr_t a = (uintptr_t)s.xk | (uintptr_t)s.xv;
        if (bwd) {
            if (!s.gk || !s.gv || !s.dxk) return BPM_ERR_ARG;
            a |= (uintptr_t)s.gk | (uintptr_t)s.gv | (uintptr_t)s.dxk | (uintptr_t)s.dxv;
        } else {
            if (!s.khat || !s.vhat || s.ld < d || s.ld % 4 || s.ld > 4 * 64 * 4) return BPM_ERR_ARG;
            if (((uintptr_t)s.khat | (uintptr_t)s.vhat) % (4 * ct_size)) return BPM_ERR_ARG;
        }
        if (a & 15) return BPM_ERR_ARG;
        KvP& p = g.p[i];
        p.xk = s.xk; p.xv = s.xv; p.T = s.T; p.B = s.B; p.pos0 = s.pos0; p.pstride = pstride;
        p.dk = bpm_make_drop(s.drop_p_k, seed, s.drop_site_k);
        p.dv = bpm_make_drop(s.drop_p_v, seed, s.drop_site_v);
        p.khat = s.khat; p.vhat = s.vhat; p.ld = s.ld;
        p.mk = s.mean_k; p.rk = s.rstd_k; p.mv = s.mean_v; p.rv = s.rstd_v;
        p.gk = s.gk; p.gv = s.gv; p.dxk = s.dxk; p.dxv = s.dxv;
    }
    return 0;
}

// What is decided before a key / value source launch.
struct KvChoice {
    int span;             // columns a wave covers (forward: up to the zero pad of the widest khat / vhat row): NV from VecWidths
    bool same;            // xk == xv in every problem (backward: the SAME instantiation, one source row for both sides)
    int rows_per_wave;    // 2 in the SAME backward kernel, else 1: a block of four waves takes 4 * rows_per_wave rows
};

static KvChoice choose_kv(const bpm_kv_source_problem* q, int n, int d, bool bwd) {
    KvChoice c = {d, true, 1};
    for (int i = 0; i < n; ++i) {
        if (!bwd && q[i].ld > c.span) c.span = q[i].ld;
        if (q[i].xk != q[i].xv) c.same = false;
    }
    if (bwd && c.same) c.rows_per_wave = 2;
    return c;
}

static void kv_blocks(Grp<KvP>& g, const KvChoice& c) {
    for (int i = 0; i < g.n; ++i) {
        const size_t waves = ((size_t)g.p[i].T * g.p[i].B + c.rows_per_wave - 1) / c.rows_per_wave;
        g.blk0[i + 1] = g.blk0[i] + blocks_for(waves, 4, 4096);
    }
}

extern "C" int bpm_kv_source_fwd(int dtype, const bpm_kv_source_problem* q, int n, const float* table, int table_rows, int d,
                                 float scale, float eps, uint64_t seed, void* stream) {
    if (dtype != BPM_F32 && dtype != BPM_BF16) return BPM_ERR_ARG;
    Grp<KvP> g;
    if (const int rc = fill_kv(g, q, n, table, table_rows, d, seed, false, dtype == BPM_BF16 ? 2 : 4)) return rc;
    const KvChoice c = choose_kv(q, n, d, false);
    kv_blocks(g, c);
    return with_ct(dtype, [&](auto ct) {
        return with_width(VecWidths(), c.span, [&](auto w) {
            return launch<kv_source_fwd_kernel<decltype(ct), decltype(w)::value>>(g.blk0[n], NT, stream, g, table, d, scale, eps);
        });
    });
}

extern "C" int bpm_kv_source_bwd(const bpm_kv_source_problem* q, int n, const float* table, int table_rows, int d, float scale,
                                 uint64_t seed, void* stream) {
    Grp<KvP> g;
    if (const int rc = fill_kv(g, q, n, table, table_rows, d, seed, true, 4)) return rc;
    const KvChoice c = choose_kv(q, n, d, true);
    kv_blocks(g, c);
    return with_width(VecWidths(), c.span, [&](auto w) {
        constexpr int NV = decltype(w)::value;
        return c.same ? launch<kv_source_bwd_kernel<NV, true>>(g.blk0[n], NT, stream, g, table, d, scale)
                      : launch<kv_source_bwd_kernel<NV, false>>(g.blk0[n], NT, stream, g, table, d, scale);
    });
}

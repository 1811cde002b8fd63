// Element-wise row kernels (gfx950): casts with bias reduction and column sums, exact GELU, Fusion-GMU gating, sums of
// gradient contributions, the head expansion of the low-rank key side.  HBM-bound streaming kernels.  Per operation:
// problem struct, kernel(s), fill, choose, entry point.
#include "rows_common.h"

namespace {
// ---------------------------------------------------------------------------
// rows_cast: y = (a [+ b]) * drop_mult ; a is fp32 or CT; written as CT
// (padded) and/or fp32; optional column sums (bias gradient) by atomics.
// Block = 32 rows x 256 columns.
// ---------------------------------------------------------------------------
constexpr int CAST_ROWS = 32;

struct CastP {
    const void* a; int lda; int a_is_ct; const float* b; int ldb;
    void* dct; int ldd; int ctw; float* df32; int ldf; float* colsum;
    int R, C; int cblk;   // column blocks
    DropCfg drop;
};

// The partial rows of the workspace entry (bpm_rows_cast_ws, deterministic mode): row block rb of problem i stores its
// column sums at part[(rb0[i] + rb) * FIN_ARR * ncol .. + C) for col_finish_kernel, instead of the atomics
struct CastPart { float* part; int ncol; unsigned rb0[BPM_MAX_GROUP]; };

BPM_DEV float* cast_part_row(const Grp<CastP>& grp, const CastPart& cp, unsigned rb) {
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.n; ++i)
        if (blockIdx.x >= grp.blk0[i]) pi = i;
    return cp.part + (size_t)(cp.rb0[pi] + rb) * FIN_ARR * cp.ncol;
}

// rows_cast_kernel (below) storing its column sums as partial rows: a copy of its body, expression for expression
template <typename CT>
__global__ __launch_bounds__(NT) void rows_cast_part_kernel(const Grp<CastP> grp, const CastPart cp) {
    unsigned bid = blockIdx.x, nblk;
    const CastP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int c = (bid % P.cblk) * NT + threadIdx.x;
    const int r0 = (bid / P.cblk) * CAST_ROWS;
    const int r1 = min(P.R, r0 + CAST_ROWS);
    const int cmax = P.dct ? P.ctw : P.C;
    if (c >= cmax) return;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) {
        float v = 0.f;
        if (c < P.C) {
            v = P.a_is_ct ? Tr<CT>::to_f(((const CT*)P.a)[(size_t)r * P.lda + c]) : ((const float*)P.a)[(size_t)r * P.lda + c];
            if (P.b) v += P.b[(size_t)r * P.ldb + c];
            v *= bpm_drop_mult(drop, (uint32_t)r * (uint32_t)P.C + (uint32_t)c);
            if (P.df32) P.df32[(size_t)r * P.ldf + c] = v;
            s += v;
        }
        if (P.dct) put<CT>(P.dct, (size_t)r * P.ldd + c, v);
    }
    if (P.colsum && c < P.C) cast_part_row(grp, cp, bid / P.cblk)[c] = s;
}

// (the default kernel keeps its own copy of the body, so that it compiles to the instructions it always did)
template <typename CT>
__global__ __launch_bounds__(NT) void rows_cast_kernel(const Grp<CastP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const CastP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int c = (bid % P.cblk) * NT + threadIdx.x;
    const int r0 = (bid / P.cblk) * CAST_ROWS;
    const int r1 = min(P.R, r0 + CAST_ROWS);
    const int cmax = P.dct ? P.ctw : P.C;
    if (c >= cmax) return;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) {
        float v = 0.f;
        if (c < P.C) {
            v = P.a_is_ct ? Tr<CT>::to_f(((const CT*)P.a)[(size_t)r * P.lda + c]) : ((const float*)P.a)[(size_t)r * P.lda + c];
            if (P.b) v += P.b[(size_t)r * P.ldb + c];
            v *= bpm_drop_mult(drop, (uint32_t)r * (uint32_t)P.C + (uint32_t)c);
            if (P.df32) P.df32[(size_t)r * P.ldf + c] = v;
            s += v;
        }
        if (P.dct) put<CT>(P.dct, (size_t)r * P.ldd + c, v);
    }
    if (P.colsum && c < P.C) atomicAdd(P.colsum + c, s);
}


// Column sums only (bias gradients from a gradient matrix already in HBM): 4-column vector loads, several rows
// per pass and four passes in flight per thread, LDS reduction, one atomic per column and workgroup.
constexpr int CSUM_ROWS = 128;

// colsum_kernel (below) storing its column sums as partial rows: a copy of its body, expression for expression
template <typename CT>
__global__ __launch_bounds__(NT) void colsum_part_kernel(const Grp<CastP> grp, const CastPart cp) {
    __shared__ float red[NT * 4];
    unsigned bid = blockIdx.x, nblk;
    const CastP& P = pick(grp, bid, nblk);
    const int CH = (P.C + 3) >> 2;                  // 4-column chunks per row (host: CH <= NT, rows padded to 4*CH)
    const int rpp = NT / CH;                        // rows per pass
    const int rr = threadIdx.x / CH, ch = threadIdx.x - rr * CH;
    const int r0 = bid * CSUM_ROWS, r1 = min(P.R, r0 + CSUM_ROWS);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rr < rpp) {
        auto ld = [&](int r) -> f32x4 {
            const int rc = r < r1 ? r : r0;         // clamped, unconditional load; zeroed below
            f32x4 v;
            if (P.a_is_ct && sizeof(CT) == 2) {
                const bf16x4 t = *(const bf16x4*)((const bf16_t*)P.a + (size_t)rc * P.lda + 4 * ch);
                v = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
            } else {
                v = *(const f32x4*)((const float*)P.a + (size_t)rc * P.lda + 4 * ch);
            }
            return r < r1 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        for (int r = r0 + rr; r < r1; r += 4 * rpp) {
            const f32x4 a0 = ld(r), a1 = ld(r + rpp), a2 = ld(r + 2 * rpp), a3 = ld(r + 3 * rpp);
            acc += (a0 + a1) + (a2 + a3);
        }
    }
    *(f32x4*)(red + 4 * threadIdx.x) = acc;
    __syncthreads();
    for (int c = threadIdx.x; c < P.C; c += NT) {
        float sum = 0.f;
        for (int q = 0; q < rpp; ++q) sum += red[4 * (q * CH) + c];
        cast_part_row(grp, cp, bid)[c] = sum;
    }
}

// (as rows_cast_kernel: its own copy of the body)
template <typename CT>
__global__ __launch_bounds__(NT) void colsum_kernel(const Grp<CastP> grp) {
    __shared__ float red[NT * 4];
    unsigned bid = blockIdx.x, nblk;
    const CastP& P = pick(grp, bid, nblk);
    const int CH = (P.C + 3) >> 2;                  // 4-column chunks per row (host: CH <= NT, rows padded to 4*CH)
    const int rpp = NT / CH;                        // rows per pass
    const int rr = threadIdx.x / CH, ch = threadIdx.x - rr * CH;
    const int r0 = bid * CSUM_ROWS, r1 = min(P.R, r0 + CSUM_ROWS);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rr < rpp) {
        auto ld = [&](int r) -> f32x4 {
            const int rc = r < r1 ? r : r0;         // clamped, unconditional load; zeroed below
            f32x4 v;
            if (P.a_is_ct && sizeof(CT) == 2) {
                const bf16x4 t = *(const bf16x4*)((const bf16_t*)P.a + (size_t)rc * P.lda + 4 * ch);
                v = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
            } else {
                v = *(const f32x4*)((const float*)P.a + (size_t)rc * P.lda + 4 * ch);
            }
            return r < r1 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        for (int r = r0 + rr; r < r1; r += 4 * rpp) {
            const f32x4 a0 = ld(r), a1 = ld(r + rpp), a2 = ld(r + 2 * rpp), a3 = ld(r + 3 * rpp);
            acc += (a0 + a1) + (a2 + a3);
        }
    }
    *(f32x4*)(red + 4 * threadIdx.x) = acc;
    __syncthreads();
    for (int c = threadIdx.x; c < P.C; c += NT) {
        float sum = 0.f;
        for (int q = 0; q < rpp; ++q) sum += red[4 * (q * CH) + c];
        atomicAdd(P.colsum + c, sum);
    }
}

}  // namespace

// Column sums only, of aligned matrices, in every problem: the vectorised reduction kernel (else rows_cast_kernel)
static bool choose_colsum(int dtype, const bpm_cast_problem* q, int n) {
    bool only_sums = true;
    for (int i = 0; i < n; ++i) {
        const bpm_cast_problem& s = q[i];
        const int ch = (s.C + 3) / 4;
        const size_t esz = (s.a_is_ct && dtype == BPM_BF16) ? 2 : 4;
        only_sums = only_sums && !s.dst_ct && !s.dst_f32 && !s.b && s.colsum && !(s.drop_p > 0.f) && ch <= NT &&
                    s.lda >= 4 * ch && (s.lda % 4) == 0 && ((uintptr_t)s.a % (4 * esz)) == 0;
    }
    return only_sums;
}

// part: null (bpm_rows_cast: column sums by float atomics) or the workspace of bpm_rows_cast_ws
static int rows_cast_entry(int dtype, const bpm_cast_problem* q, int n, uint64_t seed, float* part, size_t part_bytes, void* stream) {
    Grp<CastP> g;
    if (!grp_begin(g, q, n, seed)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_cast_problem& s = q[i];
        if (!s.a || s.R < 1 || s.C < 1 || s.lda < s.C || (s.b && s.ldb < s.C) || (s.dst_ct && s.ldd < s.C) ||
            (s.dst_f32 && s.ldf < s.C) || (!s.dst_ct && !s.dst_f32 && !s.colsum))
            return BPM_ERR_ARG;
        CastP& p = g.p[i];
        p.a = s.a; p.lda = s.lda; p.a_is_ct = s.a_is_ct; p.b = s.b; p.ldb = s.ldb;
        p.dct = s.dst_ct; p.ldd = s.ldd; p.ctw = s.ct_cols > 0 ? s.ct_cols : s.ldd; p.df32 = s.dst_f32; p.ldf = s.ldf; p.colsum = s.colsum;
        p.R = s.R; p.C = s.C;
        if (s.dst_ct && (p.ctw < s.C || p.ctw > s.ldd)) return BPM_ERR_ARG;
        const int cols = s.dst_ct ? p.ctw : s.C;
        p.cblk = (cols + NT - 1) / NT;
        p.drop = bpm_make_drop(s.drop_p, seed, s.drop_site);
    }
    const bool colsum = choose_colsum(dtype, q, n);
    for (int i = 0; i < n; ++i)
        g.blk0[i + 1] = g.blk0[i] + (colsum ? (unsigned)((q[i].R + CSUM_ROWS - 1) / CSUM_ROWS)
                                            : (unsigned)g.p[i].cblk * ((q[i].R + CAST_ROWS - 1) / CAST_ROWS));
    if (part) {
        // row blocks of each problem (a block of rows_cast_kernel is one of its cblk column blocks), the widest problem
        CastPart cp;
        unsigned rb0[BPM_MAX_GROUP + 1] = {0};
        bool any = false;
        cp.part = part; cp.ncol = 0;
        for (int i = 0; i < n; ++i) {
            const unsigned rb = (unsigned)((q[i].R + (colsum ? CSUM_ROWS : CAST_ROWS) - 1) / (colsum ? CSUM_ROWS : CAST_ROWS));
            cp.rb0[i] = rb0[i];
            rb0[i + 1] = rb0[i] + rb;
            if (q[i].colsum) { any = true; if (q[i].C > cp.ncol) cp.ncol = q[i].C; }
        }
        if (any) {
            if (((uintptr_t)part & 15) || part_bytes < (size_t)rb0[n] * FIN_ARR * cp.ncol * sizeof(float)) return BPM_ERR_ARG;
            ColFin f;
            fin_begin(f, n, cp.ncol, rb0);
            for (int i = 0; i < n; ++i) { f.cols[i] = q[i].C; fin_add(f, i, 0, q[i].colsum); }
            const int rc = with_ct(dtype, [&](auto ct) {
                using CT = decltype(ct);
                return colsum ? launch<colsum_part_kernel<CT>>(g.blk0[n], NT, stream, g, cp) : launch<rows_cast_part_kernel<CT>>(g.blk0[n], NT, stream, g, cp);
            });
            return rc ? rc : launch<col_finish_kernel<FIN_ARR>>((unsigned)f.nown, NT, stream, f, (const float*)part);
        }
    }
    return with_ct(dtype, [&](auto ct) {
        using CT = decltype(ct);
        return colsum ? launch<colsum_kernel<CT>>(g.blk0[n], NT, stream, g) : launch<rows_cast_kernel<CT>>(g.blk0[n], NT, stream, g);
    });
}

extern "C" int bpm_rows_cast(int dtype, const bpm_cast_problem* q, int n, uint64_t seed, void* stream) {
    return rows_cast_entry(dtype, q, n, seed, nullptr, 0, stream);
}

extern "C" size_t bpm_rows_cast_ws_bytes(const bpm_cast_problem* q, int n) {
    if (!q || n < 1 || n > BPM_MAX_GROUP) return 0;
    size_t rb = 0, ncol = 0;
    for (int i = 0; i < n; ++i) {
        rb += (size_t)((q[i].R > 0 ? q[i].R : 0) + CAST_ROWS - 1) / CAST_ROWS;          // the finer of the two kernels' row blocks
        if (q[i].colsum && q[i].C > 0 && (size_t)q[i].C > ncol) ncol = q[i].C;
    }
    return (rb * FIN_ARR * ncol + 4) * sizeof(float);
}

extern "C" int bpm_rows_cast_ws(int dtype, const bpm_cast_problem* q, int n, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (!ws) return BPM_ERR_ARG;
    return rows_cast_entry(dtype, q, n, seed, (float*)ws, ws_bytes, stream);
}

namespace {
// ---------------------------------------------------------------------------
// exact (erf) GELU between the two FFN products of a BERT layer (HF BertIntermediate, hidden_act = "gelu")
//   forward   g  = u Phi(u)                      Phi(u) = 0.5 (1 + erf(u / sqrt 2))
//   backward  du = dg (Phi(u) + u phi(u))        phi(u) = exp(-u^2 / 2) / sqrt(2 pi)
// Phi(u) is taken as 0.5 erfc(|u| / sqrt 2) for u < 0: 1 + erf cancels there (at u = -6 nothing of it is left in fp32).
// One thread per 4-column chunk, grid-stride over the [R, ld / 4] chunks of the output (chunks at or past C are the zero
// pad the next GEMM reads under BPM_GEMM_KPAD_ZERO).  Vector loads and stores only: every leading dimension is a multiple
// of 4, so a row's last chunk may read up to 3 pad elements of its own row (ignored).
// ---------------------------------------------------------------------------
struct GeluP { const void* u; int ldu; int u_is_ct; void* g; int ldg; const float* dg; int lddg; void* du; int lddu; int R, C; };

BPM_DEV float gelu_cdf(float u) {
    const float a = fabsf(u) * 0.70710678118654752f;
    return u < 0.f ? 0.5f * erfcf(a) : 0.5f + 0.5f * erff(a);
}

template <typename CT>
BPM_DEV f32x4 gelu_load_u(const GeluP& P, int r, int c) {
    if (P.u_is_ct && sizeof(CT) == 2) {
        const bf16x4 t = *(const bf16x4*)((const bf16_t*)P.u + (size_t)r * P.ldu + c);
        return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    }
    return *(const f32x4*)((const float*)P.u + (size_t)r * P.ldu + c);
}

template <typename CT, bool BWD>
__global__ __launch_bounds__(NT) void gelu_kernel(const Grp<GeluP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const GeluP& P = pick(grp, bid, nblk);
    const int ldo = BWD ? P.lddu : P.ldg;
    void* out = BWD ? P.du : P.g;
    const unsigned cpr = (unsigned)ldo >> 2;                   // chunks per output row
    const size_t total = (size_t)P.R * cpr;
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const int r = (int)(i / cpr), c = 4 * (int)(i - (size_t)r * cpr);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < P.C) {
            const f32x4 u = gelu_load_u<CT>(P, r, c);
            if constexpr (BWD) {
                const f32x4 d = *(const f32x4*)(P.dg + (size_t)r * P.lddg + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = d[k] * (gelu_cdf(u[k]) + u[k] * (0.3989422804014327f * __expf(-0.5f * u[k] * u[k])));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = u[k] * gelu_cdf(u[k]);
            }
            if (c + 3 >= P.C) {                                // the row's last, partial chunk: what was read past C is pad
#pragma unroll
                for (int k = 1; k < 4; ++k) v[k] = c + k < P.C ? v[k] : 0.f;
            }
        }
        put4<CT>(out, (size_t)r * ldo + c, v);
    }
}
}  // namespace

static int gelu_launch(int dtype, const bpm_gelu_problem* q, int n, bool bwd, void* stream) {
    Grp<GeluP> g;
    if (!grp_begin(g, q, n) || (dtype != BPM_BF16 && dtype != BPM_F32)) return BPM_ERR_ARG;
    const size_t csz = dtype == BPM_BF16 ? 2 : 4;
    for (int i = 0; i < n; ++i) {
        const bpm_gelu_problem& s = q[i];
        const int ldo = bwd ? s.lddu : s.ldg;
        const void* out = bwd ? s.du : s.g;
        if (!s.u || !out || (bwd && !s.dg) || s.R < 1 || s.C < 1 || s.ldu < s.C || ldo < s.C || (bwd && s.lddg < s.C)) return BPM_ERR_ARG;
        if ((long)s.R * (ldo > s.ldu ? ldo : s.ldu) > (1l << 40)) return BPM_ERR_ARG;
        const size_t usz = s.u_is_ct ? csz : 4;
        // whole 4-element chunks: 16 bytes of fp32, 8 bytes of bf16
        if ((s.ldu & 3) || (ldo & 3) || (bwd && (s.lddg & 3))) return BPM_ERR_ALIGN;
        if (((uintptr_t)s.u % (4 * usz)) || ((uintptr_t)out % (4 * csz)) || (bwd && ((uintptr_t)s.dg & 15))) return BPM_ERR_ALIGN;
        GeluP& p = g.p[i];
        p.u = s.u; p.ldu = s.ldu; p.u_is_ct = s.u_is_ct; p.g = s.g; p.ldg = s.ldg; p.dg = s.dg; p.lddg = s.lddg; p.du = s.du; p.lddu = s.lddu;
        p.R = s.R; p.C = s.C;
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)s.R * (ldo >> 2), NT * 4, CAP);
    }
    return with_ct(dtype, [&](auto ct) {
        using CT = decltype(ct);
        return bwd ? launch<gelu_kernel<CT, true>>(g.blk0[n], NT, stream, g) : launch<gelu_kernel<CT, false>>(g.blk0[n], NT, stream, g);
    });
}

extern "C" int bpm_gelu_fwd(int dtype, const bpm_gelu_problem* q, int n, void* stream) { return gelu_launch(dtype, q, n, false, stream); }
extern "C" int bpm_gelu_bwd(int dtype, const bpm_gelu_problem* q, int n, void* stream) { return gelu_launch(dtype, q, n, true, stream); }

namespace {
// ---------------------------------------------------------------------------
// Fusion-GMU gating (reference mmtr.py:189-195)
//   out = z*tanh(a1)*x1 + (1-z)*tanh(a2)*x2,  z = sigmoid(ag)
// a1,a2,ag are the three bias-free linear maps produced by the GEMM kernel.
// ---------------------------------------------------------------------------
struct GmuP {
    const float* a1; const float* a2; const float* ag; const float* x1; const float* x2; float* out;
    const float* dout; void* da1; void* da2; void* dag; int ldg; float* dx1; float* dx2; int R;
};

BPM_DEV float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

__global__ void gmu2_fwd_kernel(const Grp<GmuP> grp, int d) {
    unsigned bid = blockIdx.x, nblk;
    const GmuP& P = pick(grp, bid, nblk);
    const size_t total = (size_t)P.R * d;
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const float z = sigmoidf_(P.ag[i]);
        P.out[i] = z * tanhf(P.a1[i]) * P.x1[i] + (1.f - z) * tanhf(P.a2[i]) * P.x2[i];
    }
}

// da1, da2, dag -> CT [R, ldg] (GEMM operands, pad zeroed); dx1, dx2 (direct terms) -> fp32 [R, d]
template <typename CT>
__global__ void gmu2_bwd_kernel(const Grp<GmuP> grp, int d) {
    unsigned bid = blockIdx.x, nblk;
    const GmuP& P = pick(grp, bid, nblk);
    const size_t total = (size_t)P.R * P.ldg;
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const int c = (int)(i % P.ldg);
        const size_t r = i / P.ldg;
        float g1 = 0.f, g2 = 0.f, gz = 0.f;
        if (c < d) {
            const size_t k = r * d + c;
            const float go = P.dout[k];
            const float z = sigmoidf_(P.ag[k]);
            const float h1 = tanhf(P.a1[k]), h2 = tanhf(P.a2[k]);
            const float u1 = P.x1[k], u2 = P.x2[k];
            g1 = go * z * u1 * (1.f - h1 * h1);
            g2 = go * (1.f - z) * u2 * (1.f - h2 * h2);
            gz = go * (h1 * u1 - h2 * u2) * z * (1.f - z);
            P.dx1[k] = go * z * h1;
            P.dx2[k] = go * (1.f - z) * h2;
        }
        put<CT>(P.da1, i, g1);
        put<CT>(P.da2, i, g2);
        put<CT>(P.dag, i, gz);
    }
}
}  // namespace

static int fill_gmu(Grp<GmuP>& g, const bpm_gmu_problem* q, int n, int d, bool bwd) {
    if (!grp_begin(g, q, n) || d < 1) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_gmu_problem& s = q[i];
        if (!s.a1 || !s.a2 || !s.ag || !s.x1 || !s.x2 || s.R < 1) return BPM_ERR_ARG;
        if (bwd ? (!s.dout || !s.da1 || !s.da2 || !s.dag || !s.dx1 || !s.dx2 || s.ldg < d) : !s.out) return BPM_ERR_ARG;
        GmuP& p = g.p[i];
        p.a1 = s.a1; p.a2 = s.a2; p.ag = s.ag; p.x1 = s.x1; p.x2 = s.x2; p.out = s.out;
        p.dout = s.dout; p.da1 = s.da1; p.da2 = s.da2; p.dag = s.dag; p.ldg = s.ldg; p.dx1 = s.dx1; p.dx2 = s.dx2; p.R = s.R;
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)s.R * (bwd ? s.ldg : d), NT * 4, CAP);
    }
    return 0;
}

extern "C" int bpm_gmu2_fwd(const bpm_gmu_problem* q, int n, int d, void* stream) {
    Grp<GmuP> g;
    int rc = fill_gmu(g, q, n, d, false);
    if (rc) return rc;
    return launch<gmu2_fwd_kernel>(g.blk0[n], NT, stream, g, d);
}

extern "C" int bpm_gmu2_bwd(int dtype, const bpm_gmu_problem* q, int n, int d, void* stream) {
    Grp<GmuP> g;
    int rc = fill_gmu(g, q, n, d, true);
    if (rc) return rc;
    return with_ct(dtype, [&](auto ct) { return launch<gmu2_bwd_kernel<decltype(ct)>>(g.blk0[n], NT, stream, g, d); });
}

namespace {
// ---------------------------------------------------------------------------
// out = sum_j in[j] over `count` fp32 elements (count % 4 == 0, 16-byte aligned; out may be one of the inputs).
// The sums of gradient contributions that meet at a tensor several consumers read: a level-1 output feeds a Fusion-GMU
// twice and a level-2 encoder as key and value source; a projected input feeds up to eight encoders.
// ---------------------------------------------------------------------------
struct AddP { float* out; const float* in[BPM_ADDN_MAX]; int n_in; unsigned count4, tail; };

__global__ __launch_bounds__(NT) void add_n_kernel(const Grp<AddP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const AddP& P = pick(grp, bid, nblk);
    for (unsigned q = bid * NT + threadIdx.x; q < P.count4; q += nblk * NT) {
        f32x4 acc = *(const f32x4*)(P.in[0] + 4 * (size_t)q);
#pragma unroll
        for (int j = 1; j < BPM_ADDN_MAX; ++j)
            if (j < P.n_in) acc += *(const f32x4*)(P.in[j] + 4 * (size_t)q);
        *(f32x4*)(P.out + 4 * (size_t)q) = acc;
    }
    if (bid == 0 && threadIdx.x < P.tail) {            // count % 4 trailing elements
        const size_t i = 4 * (size_t)P.count4 + threadIdx.x;
        float a = P.in[0][i];
        for (int j = 1; j < P.n_in; ++j) a += P.in[j][i];
        P.out[i] = a;
    }
}
}  // namespace

extern "C" int bpm_add_n(const bpm_addn_problem* q, int n, void* stream) {
    Grp<AddP> g;
    if (!grp_begin(g, q, n)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_addn_problem& s = q[i];
        if (!s.out || s.n_in < 1 || s.n_in > BPM_ADDN_MAX || s.count < 1 || s.count > (size_t)1 << 33) return BPM_ERR_ARG;
        AddP& p = g.p[i];
        uintptr_t al = (uintptr_t)s.out;
        for (int j = 0; j < BPM_ADDN_MAX; ++j) {
            p.in[j] = j < s.n_in ? s.src[j] : s.src[0];
            if (j < s.n_in && !s.src[j]) return BPM_ERR_ARG;
            al |= (uintptr_t)p.in[j];
        }
        if (al & 15) return BPM_ERR_ALIGN;
        p.out = s.out; p.n_in = s.n_in; p.count4 = (unsigned)(s.count >> 2); p.tail = (unsigned)(s.count & 3);
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)p.count4, NT * 4, CAP);
    }
    return launch<add_n_kernel>(g.blk0[n], NT, stream, g);
}

// ---------------------------------------------------------------------------
// expand_heads: head-major q / dO [B, H, T, dhp] -> block rows [(h*T + t)*B + b, ld] whose columns [h dh, (h+1) dh) hold
// the head's vector and all others zero.  With these the per-head products of the low-rank key side (a handful of query
// rows: engine.EncoderGroupPlan) are plain grouped GEMMs over all heads at once: Qexp W_k' = every head's query through
// its block of W_k', Qexp^T U = every head's block of the weight gradient.  Also the value-projection bias gradient,
// sum_{b,t} rowsum(Pd[b,h,t,:]) dO[b,h,t,:] (the column sums of dV = Pd^T dO; rowsum(Pd) != 1 under attention dropout).
// One workgroup per (problem, head); its four waves take the head's T*B rows in turn, the bias sums are combined in a
// fixed order (no atomics: bitwise reproducible) and WRITTEN (the launch owns dbias).
// ---------------------------------------------------------------------------
struct ExpP { const void* q; const void* dO; void* qexp; void* dOexp; const void* Pd; float* dbias; int B, H, T, S, dh, dhp, ld; };

constexpr int EXP_NT = 1024;      // 16 waves, one row each per pass (T*B = 16 rows at the headline: one pass)
constexpr int EXP_MAXDH = 256;    // head_dim limit: bias sums of columns lane + 64 k, k < EXP_MAXDH / 64, per lane

template <typename CT>
__global__ __launch_bounds__(EXP_NT) void expand_heads_kernel(const Grp<ExpP> grp) {
    __shared__ float red[EXP_NT / 64][EXP_MAXDH];
    unsigned bid = blockIdx.x, nblk;
    const ExpP& P = pick(grp, bid, nblk);
    const int h = (int)bid, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = h * P.dh;
    float acc[EXP_MAXDH / 64] = {};                       // bias sums of columns lane + 64 k of this head
    for (int tb = wv; tb < P.T * P.B; tb += EXP_NT / 64) {
        const int t = tb / P.B, b = tb - t * P.B;
        const size_t r = (size_t)(h * P.T + t) * P.B + b;
        const CT* qrow = (const CT*)P.q + ((size_t)(b * P.H + h) * P.T + t) * P.dhp;
        const CT* drow = (const CT*)P.dO + ((size_t)(b * P.H + h) * P.T + t) * P.dhp;
        for (int c = lane; c < P.ld; c += 64) {
            const bool in = c >= c0 && c < c0 + P.dh;
            put<CT>(P.qexp, r * P.ld + c, in ? Tr<CT>::to_f(qrow[c - c0]) : 0.f);
            put<CT>(P.dOexp, r * P.ld + c, in ? Tr<CT>::to_f(drow[c - c0]) : 0.f);
        }
        if (P.dbias) {
            float rs = 0.f;
            const CT* prow = (const CT*)P.Pd + r * P.S;
            for (int j = lane; j < P.S; j += 64) rs += Tr<CT>::to_f(prow[j]);
            rs = wave_sum(rs);
#pragma unroll
            for (int k = 0; k < EXP_MAXDH / 64; ++k)
                if (lane + 64 * k < P.dh) acc[k] += rs * Tr<CT>::to_f(drow[lane + 64 * k]);
        }
    }
    if (!P.dbias) return;                                 // uniform per block
#pragma unroll
    for (int k = 0; k < EXP_MAXDH / 64; ++k) red[wv][lane + 64 * k] = acc[k];
    __syncthreads();
    for (int j = threadIdx.x; j < P.dh; j += EXP_NT) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < EXP_NT / 64; ++w) s += red[w][j];
        P.dbias[c0 + j] = s;
    }
}

extern "C" int bpm_expand_heads(int dtype, const bpm_expand_problem* q, int n, void* stream) {
    Grp<ExpP> g;
    if (!grp_begin(g, q, n) || (dtype != BPM_F32 && dtype != BPM_BF16)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_expand_problem& s = q[i];
        if (!s.q || !s.dO || !s.qexp || !s.dOexp || s.B < 1 || s.H < 1 || s.T < 1 || s.dh < 1 || s.dh > s.dhp || s.dh > EXP_MAXDH ||
            s.ld < s.H * s.dh || (s.dbias && (!s.Pd || s.S < 1)))
            return BPM_ERR_ARG;
        ExpP& p = g.p[i];
        p.q = s.q; p.dO = s.dO; p.qexp = s.qexp; p.dOexp = s.dOexp; p.Pd = s.Pd; p.dbias = s.dbias;
        p.B = s.B; p.H = s.H; p.T = s.T; p.S = s.S; p.dh = s.dh; p.dhp = s.dhp; p.ld = s.ld;
        g.blk0[i + 1] = g.blk0[i] + (unsigned)s.H;
    }
    return with_ct(dtype, [&](auto ct) { return launch<expand_heads_kernel<decltype(ct)>>(g.blk0[n], EXP_NT, stream, g); });
}

// Input staging and the parameter-side row kernels (gfx950): packed CT inputs, CT weight shadows, the folded bias and the
// gradients unfolded from it, zeroing of gradient segments, bf16x3 split images.  HBM-bound streaming kernels; rows are
// [(t*B + b), d] fp32 on the residual stream and CT (f32 / bf16, leading dim padded to 32 with zeros) where the consumer
// is an MFMA GEMM.  Per operation: problem struct, kernel(s), entry point.
#include "rows_common.h"

namespace {
// ---------------------------------------------------------------------------
// input staging: src fp32 [B,T,C]  <->  packed CT [(t*B+b), ld]
// (reference mmtr.py:741-753: dropout on the raw text features, transpose,
//  permute(2,0,1); the permutation is done here on the read side)
// ---------------------------------------------------------------------------
struct PackP { const float* src; void* dst; float* dsrc; const float* g; int ldg; int B, T, C, ld; DropCfg drop; };

template <typename CT>
__global__ void pack_rows_fwd_kernel(const Grp<PackP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const PackP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const size_t total = (size_t)P.T * P.B * P.ld;
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const int c = (int)(i % P.ld);
        const size_t row = i / P.ld;
        const int b = (int)(row % P.B), t = (int)(row / P.B);
        float v = 0.f;
        if (c < P.C) {
            const size_t si = ((size_t)b * P.T + t) * P.C + c;
            v = P.src[si] * bpm_drop_mult(drop, (uint32_t)si);
        }
        put<CT>(P.dst, i, v);
    }
}

// d(src)[b,t,c] = drop_mult * g[(t*B+b), c]   (g fp32, leading dim ldg)
__global__ void pack_rows_bwd_kernel(const Grp<PackP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const PackP& P = pick(grp, bid, nblk);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const size_t total = (size_t)P.T * P.B * P.C;
    for (size_t si = (size_t)bid * NT + threadIdx.x; si < total; si += (size_t)nblk * NT) {
        const int c = (int)(si % P.C);
        const size_t bt = si / P.C;
        const int t = (int)(bt % P.T), b = (int)(bt / P.T);
        P.dsrc[si] = P.g[((size_t)t * P.B + b) * P.ldg + c] * bpm_drop_mult(drop, (uint32_t)si);
    }
}
}  // namespace

extern "C" int bpm_pack_rows_fwd(int dtype, const bpm_pack_problem* q, int n, uint64_t seed, void* stream) {
    Grp<PackP> g;
    if (!grp_begin(g, q, n, seed)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!q[i].src || !q[i].dst || q[i].B < 1 || q[i].T < 1 || q[i].C < 1 || q[i].ld < q[i].C) return BPM_ERR_ARG;
        PackP& p = g.p[i];
        p.src = q[i].src; p.dst = q[i].dst; p.dsrc = nullptr; p.g = nullptr; p.ldg = 0;
        p.B = q[i].B; p.T = q[i].T; p.C = q[i].C; p.ld = q[i].ld;
        p.drop = bpm_make_drop(q[i].drop_p, seed, q[i].drop_site);
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)p.T * p.B * p.ld, NT * 4, CAP);
    }
    return with_ct(dtype, [&](auto ct) { return launch<pack_rows_fwd_kernel<decltype(ct)>>(g.blk0[n], NT, stream, g); });
}

extern "C" int bpm_pack_rows_bwd(const bpm_pack_problem* q, int n, uint64_t seed, void* stream) {
    Grp<PackP> g;
    if (!grp_begin(g, q, n, seed)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!q[i].g || !q[i].dsrc || q[i].B < 1 || q[i].T < 1 || q[i].C < 1 || q[i].ldg < q[i].C) return BPM_ERR_ARG;
        PackP& p = g.p[i];
        p.src = nullptr; p.dst = nullptr; p.dsrc = q[i].dsrc; p.g = q[i].g; p.ldg = q[i].ldg;
        p.B = q[i].B; p.T = q[i].T; p.C = q[i].C; p.ld = 0;
        p.drop = bpm_make_drop(q[i].drop_p, seed, q[i].drop_site);
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)p.T * p.B * p.C, NT * 4, CAP);
    }
    return launch<pack_rows_bwd_kernel>(g.blk0[n], NT, stream, g);
}

namespace {
// ---------------------------------------------------------------------------
// weight shadows: every fp32 master [rows, cols] (row stride src_ld) -> CT
// [rows, ld] (zero pad), one launch over a device-resident table
// ---------------------------------------------------------------------------
template <typename CT>
__global__ void pack_weights_kernel(const bpm_pack_desc* __restrict__ tab, int ndesc) {
    int lo = 0, hi = ndesc - 1;
    const unsigned bid = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= bid) lo = mid; else hi = mid - 1;
    }
    const bpm_pack_desc d = tab[lo];
    const size_t total = (size_t)d.rows * d.ld;
    const size_t i0 = ((size_t)(bid - d.blk0) * NT + threadIdx.x) * 4;
    if (i0 >= total) return;
    const float* src = (const float*)d.src;
    // ld % 4 == 0: the thread's 4 elements share a row
    const size_t r = i0 / d.ld;
    const int c = (int)(i0 - r * d.ld);
    const float* sp = src + r * d.src_ld + c;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((d.ld & 3) == 0 && c + 3 < d.cols && (((uintptr_t)sp) & 15) == 0) {
        v = *(const f32x4*)sp;
        if (d.colscale) v *= *(const f32x4*)(d.colscale + c);     // colscale is 64-byte aligned and c % 4 == 0
        if ((((uintptr_t)d.dst) & 15) == 0 && (d.dst_ld & 3) == 0) { put4<CT>(d.dst, r * d.dst_ld + c, v); return; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t i = i0 + e;
            if (i >= total) break;
            const int ce = (int)(i % d.ld);
            const size_t re = i / d.ld;
            float x = 0.f;
            if (ce < d.cols) {
                x = src[re * d.src_ld + ce];
                if (d.colscale) x *= d.colscale[ce];
            }
            put<CT>(d.dst, re * d.dst_ld + ce, x);
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) put<CT>(d.dst, r * d.dst_ld + c + e, v[e]);
}
}  // namespace

extern "C" int bpm_pack_weights(int dtype, const bpm_pack_desc* table_dev, int ndesc, unsigned total_blocks, void* stream) {
    if (!table_dev || ndesc < 1 || total_blocks < 1) return BPM_ERR_ARG;
    return with_ct(dtype, [&](auto ct) { return launch<pack_weights_kernel<decltype(ct)>>(total_blocks, NT, stream, table_dev, ndesc); });
}

namespace {
// folded bias: out[n] = b[n] + W[n,:] . beta   (one wave per row)
__global__ __launch_bounds__(NT) void fold_bias_kernel(const bpm_fold_desc* __restrict__ tab, int ndesc) {
    const bpm_fold_desc d = find_desc(tab, ndesc, blockIdx.x);
    const int row = (int)(blockIdx.x - d.blk0) * (NT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= d.rows) return;
    float s = 0.f;
    for (int c = lane; c < d.cols; c += 64) s += d.W[(size_t)row * d.ldw + c] * d.beta[c];
    s = wave_sum(s);
    if (lane == 0) d.out[row] = s + (d.b ? d.b[row] : 0.f);
}
}  // namespace

extern "C" int bpm_fold_bias(const bpm_fold_desc* table_dev, int ndesc, unsigned total_blocks, void* stream) {
    if (!table_dev || ndesc < 1 || total_blocks < 1) return BPM_ERR_ARG;
    return launch<fold_bias_kernel>(total_blocks, NT, stream, table_dev, ndesc);
}

namespace {
// gradients of the real parameters from the folded ones (see bpm_unfold_desc)
// (Measured in round 3 and not kept: per-block partial rows through a workspace + last-block sum instead of the float
// atomics on dgamma / dbeta -- 72 us against 42 stand-alone at hidden 768: the 4-byte write-through stores cost more
// than the contended atomics.)
//
// A block owns 16 rows.  Wide path (cols and ldw multiples of 4, every matrix and vector 16-byte aligned): a thread owns
// four consecutive columns and walks its rows in batches of UNF_BATCH, the 16-byte loads of dWf, W and (when it is
// accumulated into) dW of a whole batch issued before the first use -- the one-column loop below keeps a single 4-byte
// load per operand in flight, because the store into dW may alias the next row's loads.  The per-column sums run over
// r ascending with the expressions of the one-column loop, so both paths give the same dW, dbias and partial sums.  The
// sums of a pass go through LDS to be added as the one-column loop adds them: consecutive lanes on consecutive columns
// (one 256-byte atomic instruction per wave, not 64 dwords 16 bytes apart).
constexpr int UNF_ROWS = 16;
constexpr int UNF_BATCH = 8;

// the descriptor's pointers come out of a device table, which makes them generic (flat_*) to the compiler: the wide path
// says that they are global memory, so its loads take a uniform row base and count their own waits
typedef f32x4 __attribute__((address_space(1))) g_f32x4;
BPM_DEV f32x4 gload4(const float* p) { return *(const g_f32x4*)p; }
BPM_DEV void gstore4(float* p, f32x4 v) { *(g_f32x4*)p = v; }
BPM_DEV float gload1(const float* p) { return *(const float __attribute__((address_space(1)))*)p; }

// one element of dW's update, written once so that both paths round it alike: two rounded products, then their sum (left
// to the compiler, the wide path fused db * bt into the sum and the one-column loop neither); the column sums are fused
BPM_DEV float unf_dw(float f, float g, float db, float bt) {
#pragma clang fp contract(off)
    return f * g + db * bt;
}

BPM_DEV bool unf_wide(const bpm_unfold_desc& d) {
    const uintptr_t a = (uintptr_t)d.dWf | (uintptr_t)d.W | (uintptr_t)d.dW | (uintptr_t)d.gamma | (uintptr_t)d.beta |
                        (uintptr_t)d.dgamma | (uintptr_t)d.dbeta;
    return ((d.cols | d.ldw) & 3) == 0 && (a & 15) == 0;
}

// PART (bpm_unfold_grads_ws): the block's column sums go to its partial rows part[0 .. cols) (dgamma) and
// part[pstride .. pstride + cols) (dbeta), 16 bytes per lane write-through, instead of LDS and the float atomics
template <bool STORE, bool PART = false>
BPM_DEV void unfold_wide(const bpm_unfold_desc& d, int r0, int r1, float* sums, float* part = nullptr, int pstride = 0) {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < d.cols; c0 += 4 * NT) {         // (block-uniform trip count: the barriers below)
        const int c = c0 + 4 * tid;
        f32x4 ag = f32x4{0.f, 0.f, 0.f, 0.f}, ab = ag;
        if (c < d.cols) {
            const f32x4 g = gload4(d.gamma + c), bt = gload4(d.beta + c);
            for (int rb = r0; rb < r1; rb += UNF_BATCH) {
                f32x4 f[UNF_BATCH], w[UNF_BATCH], o[UNF_BATCH];
                float db[UNF_BATCH];
#pragma unroll
                for (int j = 0; j < UNF_BATCH; ++j) {
                    const int r = min(rb + j, r1 - 1);    // a dead row of the last batch re-reads the last live one
                    f[j] = gload4(d.dWf + (size_t)r * d.cols + c);
                    w[j] = gload4(d.W + (size_t)r * d.ldw + c);
                    if (!STORE) o[j] = gload4(d.dW + (size_t)r * d.ldw + c);
                    db[j] = gload1(d.dbf + r);
                }
                __builtin_amdgcn_sched_barrier(0);        // the whole batch is issued before the first row is used
#pragma unroll
                for (int j = 0; j < UNF_BATCH; ++j) {
                    if (rb + j >= r1) break;
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = unf_dw(f[j][e], g[e], db[j], bt[e]);
                        if (!STORE) v[e] = o[j][e] + v[e];
                        ag[e] = fmaf(f[j][e], w[j][e], ag[e]);
                        ab[e] = fmaf(db[j], w[j][e], ab[e]);
                    }
                    gstore4(d.dW + (size_t)(rb + j) * d.ldw + c, v);
                }
            }
        }
        if constexpr (PART) {
            if (c < d.cols) {                                 // (cols % 4 == 0: the thread's four columns are all live)
                const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)part, 0, 2 * pstride * 4, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128((u32x4&)ag, rw, c * 4, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128((u32x4&)ab, rw, (pstride + c) * 4, 0, 16);
            }
        } else {
            *(f32x4*)(sums + 4 * tid) = ag;
            *(f32x4*)(sums + 4 * NT + 4 * tid) = ab;
            __syncthreads();
            for (int k = tid; k < 4 * NT && c0 + k < d.cols; k += NT) {
                atomicAdd(d.dgamma + c0 + k, sums[k]);
                atomicAdd(d.dbeta + c0 + k, sums[4 * NT + k]);
            }
            __syncthreads();
        }
    }
}

// one column of unfold_grads_kernel's one-column loop, expression for expression (the same dW and partial sums), for
// unfold_grads_ws_kernel: dW's update over the block's rows, the two column sums returned
BPM_DEV void unfold_column(const bpm_unfold_desc& d, int r0, int r1, int c, int store_dw, float& ag, float& ab) {
    const float g = d.gamma[c], bt = d.beta[c];
    ag = 0.f; ab = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float f = d.dWf[(size_t)r * d.cols + c], w = d.W[(size_t)r * d.ldw + c], db = d.dbf[r];
        const float v = unf_dw(f, g, db, bt);
        float* o = d.dW + (size_t)r * d.ldw + c;
        *o = store_dw ? v : *o + v;                   // store_dw: this launch is the first writer of dW this step
        ag = fmaf(f, w, ag);
        ab = fmaf(db, w, ab);
    }
}

__global__ __launch_bounds__(NT) void unfold_grads_kernel(const bpm_unfold_desc* __restrict__ tab, int ndesc, int store_dw) {
    const bpm_unfold_desc d = find_desc(tab, ndesc, blockIdx.x);
    const int r0 = (int)(blockIdx.x - d.blk0) * UNF_ROWS, r1 = min(d.rows, r0 + UNF_ROWS);
    __shared__ __attribute__((aligned(16))) float sums[2 * 4 * NT];
    if (unf_wide(d)) {
        if (store_dw) unfold_wide<true>(d, r0, r1, sums);
        else unfold_wide<false>(d, r0, r1, sums);
    } else for (int c = threadIdx.x; c < d.cols; c += NT) {
        const float g = d.gamma[c], bt = d.beta[c];
        float ag = 0.f, ab = 0.f;
        for (int r = r0; r < r1; ++r) {
            const float f = d.dWf[(size_t)r * d.cols + c], w = d.W[(size_t)r * d.ldw + c], db = d.dbf[r];
            const float v = unf_dw(f, g, db, bt);
            float* o = d.dW + (size_t)r * d.ldw + c;
            *o = store_dw ? v : *o + v;                   // store_dw: this launch is the first writer of dW this step
            ag = fmaf(f, w, ag);
            ab = fmaf(db, w, ab);
        }
        atomicAdd(d.dgamma + c, ag);
        atomicAdd(d.dbeta + c, ab);
    }
    if ((int)threadIdx.x < r1 - r0) d.dbias[r0 + threadIdx.x] += d.dbf[r0 + threadIdx.x];
}

// The same launch without float atomics (bpm_unfold_grads_ws): dW and dbias as above, bit for bit; the column sums of a
// block go to its two partial rows in the workspace, and the block of a descriptor that draws the last ticket adds the
// partial rows in block order and makes one plain read-modify-write into dgamma / dbeta -- one owner per column, a
// fixed order, and nothing that depends on the other descriptors of the launch.  Hand-off as in ln_bwd_vec_kernel
// (rows_norm.hip): partial rows stored write-through, every wave's stores drained, workgroup barrier, ticket by one lane
// (agent scope); the last block acquires and reads with plain vector loads.  The ticket words are zeroed by the entry
// ahead of every launch.  ws: UNF_WS_HEAD-padded ticket words (one per descriptor), then 2 * pstride floats per block.
constexpr int UNF_WS_HEAD = 64;
inline size_t unf_ws_head(int ndesc) { return ((size_t)ndesc + UNF_WS_HEAD - 1) / UNF_WS_HEAD * UNF_WS_HEAD; }

__global__ __launch_bounds__(NT) void unfold_grads_ws_kernel(const bpm_unfold_desc* __restrict__ tab, int ndesc, int store_dw,
                                                              unsigned* cnt, float* rows, int pstride) {
    int di = 0, hi = ndesc - 1;
    while (di < hi) {                                     // find_desc, keeping the index: the descriptor's ticket word
        const int mid = (di + hi + 1) >> 1;
        if (tab[mid].blk0 <= blockIdx.x) di = mid; else hi = mid - 1;
    }
    const bpm_unfold_desc d = tab[di];
    const unsigned nblk = (unsigned)(d.rows + UNF_ROWS - 1) / UNF_ROWS;
    const int r0 = (int)(blockIdx.x - d.blk0) * UNF_ROWS, r1 = min(d.rows, r0 + UNF_ROWS);
    // host contract, checked so that nothing is ever read or written past the workspace: a partial row holds the
    // descriptor's columns, its nblk blocks lie inside the grid, and a block beyond them draws no ticket
    if (d.cols > pstride || d.blk0 + nblk > gridDim.x || r0 >= d.rows) return;
    float* part = rows + (size_t)blockIdx.x * 2 * pstride;
    // 16-byte partial rows: pstride % 4 == 0 and rows 16-byte aligned (entry), so the wide path's stores are aligned
    const bool wide = unf_wide(d);
    if (wide) {
        if (store_dw) unfold_wide<true, true>(d, r0, r1, nullptr, part, pstride);
        else unfold_wide<false, true>(d, r0, r1, nullptr, part, pstride);
    } else for (int c = threadIdx.x; c < d.cols; c += NT) {
        float ag, ab;
        unfold_column(d, r0, r1, c, store_dw, ag, ab);
        __hip_atomic_store(part + c, ag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + pstride + c, ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if ((int)threadIdx.x < r1 - r0) d.dbias[r0 + threadIdx.x] += d.dbf[r0 + threadIdx.x];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(cnt + di, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == nblk - 1;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    const float* first = rows + (size_t)d.blk0 * 2 * pstride;
    for (int c = threadIdx.x; c < d.cols; c += NT) {      // block order, one column per thread: the same sum on both paths
        float sg = 0.f, sb = 0.f;
#pragma unroll 8
        for (unsigned b = 0; b < nblk; ++b) {
            sg += gload1(first + (size_t)b * 2 * pstride + c);
            sb += gload1(first + (size_t)b * 2 * pstride + pstride + c);
        }
        d.dgamma[c] += sg;
        d.dbeta[c] += sb;
    }
}
}  // namespace

extern "C" int bpm_unfold_grads(const bpm_unfold_desc* table_dev, int ndesc, unsigned total_blocks, int store_dw, void* stream) {
    if (!table_dev || ndesc < 1 || total_blocks < 1) return BPM_ERR_ARG;
    return launch<unfold_grads_kernel>(total_blocks, NT, stream, table_dev, ndesc, store_dw);
}

extern "C" size_t bpm_unfold_grads_ws_bytes(int ndesc, unsigned total_blocks, int max_cols) {
    if (ndesc < 1 || max_cols < 1) return 0;
    const size_t pstride = ((size_t)max_cols + 3) / 4 * 4;
    return (unf_ws_head(ndesc) + (size_t)total_blocks * 2 * pstride) * sizeof(float);
}

extern "C" int bpm_unfold_grads_ws(const bpm_unfold_desc* table_dev, int ndesc, unsigned total_blocks, int store_dw, int max_cols,
                                   void* ws, size_t ws_bytes, void* stream) {
    if (!table_dev || ndesc < 1 || total_blocks < 1 || max_cols < 1 || !ws) return BPM_ERR_ARG;
    if (((uintptr_t)ws & 15) || ws_bytes < bpm_unfold_grads_ws_bytes(ndesc, total_blocks, max_cols)) return BPM_ERR_ARG;
    const size_t head = unf_ws_head(ndesc);
#ifdef BPM_LAB
    if (!g_bpm_rows_dry)          // (the dry mode of the lab build touches no device)
#endif
    if (const hipError_t e = hipMemsetAsync(ws, 0, head * sizeof(float), (hipStream_t)stream); e != hipSuccess) return (int)e;
    return launch<unfold_grads_ws_kernel>(total_blocks, NT, stream, table_dev, ndesc, store_dw, (unsigned*)ws, (float*)ws + head,
                                          (max_cols + 3) / 4 * 4);
}

namespace {
// zero a list of fp32 segments (device-resident table): the small tensors of a flat gradient buffer whose large ones are
// written by plain stores (see bpm_zero_segments)
constexpr unsigned ZSEG = NT * 16;          // elements per block
__global__ __launch_bounds__(NT) void zero_segments_kernel(const bpm_zero_desc* __restrict__ tab, int ndesc) {
    const bpm_zero_desc d = find_desc(tab, ndesc, blockIdx.x);
    const unsigned i0 = (blockIdx.x - d.blk0) * ZSEG, i1 = min(d.n, i0 + ZSEG);
    if ((((uintptr_t)d.p) & 15) == 0) {
        for (unsigned i = i0 + 4 * threadIdx.x; i + 3 < i1; i += 4 * NT) *(f32x4*)(d.p + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        for (unsigned i = i0 + ((i1 - i0) & ~3u) + threadIdx.x; i < i1; i += NT) d.p[i] = 0.f;
    } else {
        for (unsigned i = i0 + threadIdx.x; i < i1; i += NT) d.p[i] = 0.f;
    }
}
}  // namespace

extern "C" int bpm_zero_segment_blocks(unsigned n) { return (int)((n + ZSEG - 1) / ZSEG); }

extern "C" int bpm_zero_segments(const bpm_zero_desc* table_dev, int ndesc, unsigned total_blocks, void* stream) {
    if (!table_dev || ndesc < 1 || total_blocks < 1) return BPM_ERR_ARG;
    return launch<zero_segments_kernel>(total_blocks, NT, stream, table_dev, ndesc);
}

namespace {
// ---------------------------------------------------------------------------
// split: fp32 [R, C] (row stride ld) -> bf16 [R, 2 ldp]: columns [0, ldp) hold hi = bf16(x), columns [ldp, 2 ldp) hold
// lo = bf16(x - hi), pad columns [C, ldp) of both planes zero.  Operands of the "bf16x3" products (bpm_gemm_grouped with
// dtype BPM_BF16X3: x y ~ hi hi + hi lo + lo hi on the bf16 MFMA with f32 accumulation: ~2^-16 relative per product).
// ---------------------------------------------------------------------------
struct SplitP { const float* src; bf16_t* dst; int R, C, ld, ldp; };

__global__ __launch_bounds__(NT) void split_rows_kernel(const Grp<SplitP> grp) {
    unsigned bid = blockIdx.x, nblk;
    const SplitP& P = pick(grp, bid, nblk);
    const unsigned cpr = (unsigned)P.ldp >> 2;                     // 4-column chunks per row (ldp % 4 == 0)
    const size_t total = (size_t)P.R * cpr;
    const bool vec = ((P.ld & 3) == 0) && ((((uintptr_t)P.src) & 15) == 0);
    for (size_t i = (size_t)bid * NT + threadIdx.x; i < total; i += (size_t)nblk * NT) {
        const size_t r = i / cpr;
        const int c = 4 * (int)(i - r * cpr);
        f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* sp = P.src + r * P.ld + c;
        if (vec && c + 3 < P.C) x = *(const f32x4*)sp;
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (c + q < P.C) x[q] = sp[q];
        }
        bf16x4 hi, lo;
#pragma unroll
        for (int q = 0; q < 4; ++q) { hi[q] = (bf16_t)x[q]; lo[q] = (bf16_t)(x[q] - (float)hi[q]); }
        bf16_t* dp = P.dst + r * 2 * (size_t)P.ldp + c;
        *(bf16x4*)dp = hi;
        *(bf16x4*)(dp + P.ldp) = lo;
    }
}
}  // namespace

extern "C" int bpm_split_rows(const bpm_split_problem* q, int n, void* stream) {
    Grp<SplitP> g;
    if (!grp_begin(g, q, n)) return BPM_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bpm_split_problem& s = q[i];
        if (!s.src || !s.dst || s.R < 1 || s.C < 1 || s.ld < s.C || s.ldp < s.C || (s.ldp & 3)) return BPM_ERR_ARG;
        if (((uintptr_t)s.dst & 7) || ((uintptr_t)s.src & 3)) return BPM_ERR_ALIGN;
        SplitP& p = g.p[i];
        p.src = s.src; p.dst = (bf16_t*)s.dst; p.R = s.R; p.C = s.C; p.ld = s.ld; p.ldp = s.ldp;
        g.blk0[i + 1] = g.blk0[i] + blocks_for((size_t)s.R * (s.ldp >> 2), NT * 4, CAP);
    }
    return launch<split_rows_kernel>(g.blk0[n], NT, stream, g);
}

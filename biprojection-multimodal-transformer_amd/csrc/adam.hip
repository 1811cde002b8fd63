// The optimizer step and the global gradient norm in front of it (gfx950): fused Adam over flat fp32 buffers and the sum
// of squares with torch's clip coefficient, streaming over device-resident segment tables.  Per operation: kernel(s), fill, entry.
#include "rows_common.h"

namespace {
// ---------------------------------------------------------------------------
// Global gradient norm: sum of squares over a list of fp32 segments (device-resident table), then the norm and torch's
// clip coefficient, all left on the device (see bpm_grad_sumsq).  Bitwise reproducible: no float atomics, a fixed shape.
//   block   : one 4096-element window of ONE segment.  Windows start at the 16-byte boundary at or below the segment's
//             first element, so every quad of a window is aligned whatever the segment's start; a lane owns 4 quads
//             (f32x4 loads, all issued before the first use).  The at most two quads that straddle the segment's ends
//             (scalar head and tail) are read element-wise by the lane that owns them, elements outside count as 0.
//   lane    : <= 16 squares, one fp32 fma chain;   block: 6 shuffle levels + 2 levels over the four waves (fp32);
//   partial : one float per block into the workspace;  final launch (one block): the partials in fp64, every thread a
//             fixed strided subset in index order, then a fixed tree.
// Relative error of the sum of squares <= (1 + 16 + 8) * 2^-24 = 1.5e-6 (square, chain, tree; fp64 above adds nothing
// visible), half of that under the root, plus the norm's own rounding to fp32.
// ---------------------------------------------------------------------------
constexpr int SSQ_ITER = 4;
constexpr int SSQ_CHUNK = NT * 4 * SSQ_ITER;            // elements per block
constexpr int SSQ_FINAL_NT = 1024;

BPM_DEV unsigned ssq_lead(const float* p) { return (unsigned)(((uintptr_t)p >> 2) & 3); }      // elements past the 16-byte boundary

__global__ __launch_bounds__(NT) void grad_sumsq_kernel(const bpm_sumsq_seg* __restrict__ tab, int nseg, float* __restrict__ partial) {
    const bpm_sumsq_seg S = find_desc(tab, nseg, blockIdx.x);
    const long long n = (long long)S.n;
    const long long e0 = (long long)(blockIdx.x - S.blk0) * SSQ_CHUNK - ssq_lead(S.p);   // window start, as a segment index
    f32x4 x[SSQ_ITER];
#pragma unroll
    for (int j = 0; j < SSQ_ITER; ++j) {
        const long long e = e0 + 4 * (j * NT + (int)threadIdx.x);
        x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e >= 0 && e + 4 <= n) {
            x[j] = *(const f32x4*)(S.p + e);
        } else if (e > -4 && e < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q >= 0 && e + q < n) x[j][q] = S.p[e + q];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < SSQ_ITER; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) s = fmaf(x[j][q], x[j][q], s);
    s = wave_sum(s);
    __shared__ float red[NT / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = grad_scale * sqrt(sum of the partials + *extra),  out[1] = min(1, max_norm / (out[0] + 1e-6))  (1 when !clip)
__global__ __launch_bounds__(SSQ_FINAL_NT) void grad_sumsq_final_kernel(const float* partial, unsigned nblk, float grad_scale,
                                                                        float max_norm, int clip, const float* extra, float* out) {
    __shared__ double red[SSQ_FINAL_NT];
    const unsigned nq = (nblk + 3) / 4;                    // the workspace is 16-byte aligned and sized in whole quads
    double acc = 0.0;
    for (unsigned q0 = threadIdx.x; q0 < nq; q0 += SSQ_FINAL_NT * 4) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = q0 + j * SSQ_FINAL_NT;
            v[j] = q < nq ? ((const f32x4*)partial)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = 4 * (q0 + j * SSQ_FINAL_NT);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < nblk) acc += (double)v[j][e];  // (past nblk: the quad's unwritten remainder, or a quad not loaded)
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = SSQ_FINAL_NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double tot = red[0] + (extra ? (double)*extra : 0.0);
        const float norm = (float)((double)grad_scale * sqrt(tot));
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = !clip ? 1.f : c > 1.f ? 1.f : c;          // a NaN coefficient passes through, as torch's clamp lets it
    }
}
}  // namespace

extern "C" int bpm_grad_sumsq_blocks(const float* p, size_t n) { return (int)(((((uintptr_t)p >> 2) & 3) + n + SSQ_CHUNK - 1) / SSQ_CHUNK); }

extern "C" size_t bpm_grad_sumsq_ws_bytes(unsigned total_blocks) { return ((size_t)total_blocks + 3) / 4 * 16; }

extern "C" int bpm_grad_sumsq(const bpm_sumsq_seg* table_dev, int nseg, unsigned total_blocks, float grad_scale, float max_norm,
                              const float* extra_sumsq, void* ws, size_t ws_bytes, float* out, void* stream) {
    if (!table_dev || nseg < 1 || total_blocks < 1 || !ws || !out) return BPM_ERR_ARG;
    if (ws_bytes < bpm_grad_sumsq_ws_bytes(total_blocks)) return BPM_ERR_ARG;
    if (((uintptr_t)ws & 15) || ((uintptr_t)out & 7) || ((uintptr_t)extra_sumsq & 3)) return BPM_ERR_ALIGN;
    const int clip = max_norm > 0.f && max_norm < INFINITY;          // <= 0, +inf (and NaN): the norm only
    if (const int rc = launch<grad_sumsq_kernel>(total_blocks, NT, stream, table_dev, nseg, (float*)ws)) return rc;
    return launch<grad_sumsq_final_kernel>(1, SSQ_FINAL_NT, stream, (const float*)ws, total_blocks, grad_scale, max_norm, clip, extra_sumsq, out);
}

// ---------------------------------------------------------------------------
// Fused Adam over one flat fp32 buffer (torch.optim.Adam semantics, no amsgrad):
//   g = grad * grad_scale + wd * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc_i = 1 - b_i^t  (passed in)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, size_t n4, float lr_c, float b1, float b2, float eps,
                                                 float wd, float rsq_bc2, float gscale, int zero_grad) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
        f32x4 pp = ((f32x4*)p)[i], gg = ((f32x4*)g)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        gg = gg * gscale + wd * pp;
        mm = b1 * mm + (1.f - b1) * gg;
        vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
        for (int q = 0; q < 4; ++q) pp[q] -= lr_c * mm[q] / (sqrtf(vv[q]) * rsq_bc2 + eps);
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
        if (zero_grad) ((f32x4*)g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

extern "C" int bpm_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n == 0 || (n & 3) || step < 1) return BPM_ERR_ARG;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return BPM_ERR_ALIGN;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const size_t n4 = n / 4;
    const unsigned blocks = blocks_for(n4, NT, 256 * 16);
    return launch<adam_kernel>(blocks, NT, stream, param, grad, exp_avg, exp_avg_sq, n4, (float)(lr / bc1), beta1, beta2, eps, weight_decay,
                               (float)(1.0 / sqrt(bc2)), grad_scale, zero_grad);
}

// ---------------------------------------------------------------------------
// The same step, table driven and with PARAMETER GROUPS, writing the CT weight shadows as it stores the updated masters
// (no second pass over the flat master for the shadow refresh: 2.7 GB read + 1.35 GB written per optimizer step at
// hidden 768).  The flat buffer
// is cut into segments (device-resident table, built once): runs of parameters without a plain shadow, and one segment per
// parameter that has one -- a whole [rows, cols] matrix whose shadow is [rows, dst_ld], pad columns left as they are
// (zero since allocation).  A block covers ADAM_CHUNK consecutive f32x4 of ONE segment, so the segment is looked up once
// per block; every thread has its 4 x 4 loads in flight before the first use, and the shadow is stored from the updated
// value.  ONE kernel behind bpm_adam_step_groups, bpm_adam_step_table and bpm_adam_step_table_clip.
// A segment carries the index of its group (or -1: not stepped), the groups' constants ride in the kernel arguments, and
// group, skip decision and step number are uniform per block.
//   L2 group        : g = grad * scale + wd * p                                    (wd_l2 = wd, decay = 1: adam_kernel's arithmetic)
//   decoupled group : p *= 1 - lr * wd, then the update on g = grad * scale       (wd_l2 = 0, decay = 1 - lr * wd)
// One expression serves both.  ngroups == 0 (the two table entries): one group, G.g[0], and the segments' group words are
// not looked at.  A block that is not stepped (group -1, or *norm_dev not finite) loads nothing and stores nothing but
// zeros to its gradients when zero_grad is set.  scale_dev: the gradient scale is gscale * (*scale_dev), one uniform read
// per block of a value an earlier launch on the stream left on the device (the clip coefficient of bpm_grad_sumsq).
// steps_dev: the bias corrections come from steps_dev[group] + 1, in double.
// ---------------------------------------------------------------------------
constexpr int ADAM_ITER = 4;
constexpr int ADAM_CHUNK = NT * ADAM_ITER;             // f32x4 per block

extern "C" int bpm_adam_blocks(size_t n4) { return (int)((n4 + ADAM_CHUNK - 1) / ADAM_CHUNK); }

struct AdamGroupK { float lr, b1, b2, eps, wd_l2, decay, lr_c, rsq_bc2; };
struct AdamGroupsK { AdamGroupK g[BPM_ADAM_MAX_GROUPS]; };

BPM_DEV double adam_ipow(double b, int e) {              // b^e, e >= 1, by squaring
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

BPM_DEV bool adam_norm_finite(const float* norm_dev) { return fabsf(*norm_dev) <= 3.402823466e+38f; }   // NaN, +-inf: false

// One block's work: segment S of the buffers p / g / m / v, group grp (block-uniform).  Shared by the two kernels below.
template <typename CT>
BPM_DEV void adam_block(const bpm_adam_seg& S, const int grp, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                        float* __restrict__ v, const AdamGroupsK& G, int ngroups, float gscale, int zero_grad,
                        const float* __restrict__ scale_dev, const float* __restrict__ norm_dev, const int* __restrict__ steps_dev) {
    const size_t base = S.off4 + (size_t)(blockIdx.x - S.blk0) * ADAM_CHUNK;
    const size_t end = S.off4 + S.n4;
    bool live = grp >= 0 && grp < (ngroups ? ngroups : 1);
    if (live && norm_dev) live = adam_norm_finite(norm_dev);
    if (!live) {
        if (zero_grad) {
#pragma unroll
            for (int j = 0; j < ADAM_ITER; ++j) {
                const size_t i = base + j * NT + threadIdx.x;
                if (i < end) ((f32x4*)g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        return;
    }
    f32x4 pp[ADAM_ITER], gg[ADAM_ITER], mm[ADAM_ITER], vv[ADAM_ITER];
#pragma unroll
    for (int j = 0; j < ADAM_ITER; ++j) {
        const size_t i = base + j * NT + threadIdx.x;
        const size_t ic = i < end ? i : S.off4;             // clamped, unconditional loads
        pp[j] = ((const f32x4*)p)[ic]; gg[j] = ((const f32x4*)g)[ic]; mm[j] = ((const f32x4*)m)[ic]; vv[j] = ((const f32x4*)v)[ic];
    }
    if (scale_dev) gscale *= *scale_dev;
    const AdamGroupK H = G.g[grp];
    const float b1 = H.b1, b2 = H.b2, eps = H.eps, wd = H.wd_l2, decay = H.decay;
    float lr_c = H.lr_c, rsq_bc2 = H.rsq_bc2;
    if (steps_dev) {
        const int t = steps_dev[grp] + 1;
        const double bc1 = 1.0 - adam_ipow((double)b1, t), bc2 = 1.0 - adam_ipow((double)b2, t);
        lr_c = (float)((double)H.lr / bc1);
        rsq_bc2 = (float)(1.0 / sqrt(bc2));
    }
#pragma unroll
    for (int j = 0; j < ADAM_ITER; ++j) {
        const size_t i = base + j * NT + threadIdx.x;
        if (i >= end) continue;
        f32x4 x = pp[j] * decay, gr = gg[j] * gscale + wd * pp[j];
        const f32x4 mo = b1 * mm[j] + (1.f - b1) * gr;
        const f32x4 vo = b2 * vv[j] + (1.f - b2) * gr * gr;
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] -= lr_c * mo[q] / (sqrtf(vo[q]) * rsq_bc2 + eps);
        ((f32x4*)p)[i] = x; ((f32x4*)m)[i] = mo; ((f32x4*)v)[i] = vo;
        if (zero_grad) ((f32x4*)g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (S.dst) {
            const size_t e = 4 * (i - S.off4);               // element index inside the [rows, cols] matrix; cols % 4 == 0
            if (e < (size_t)S.rows * S.cols) {               // (the segment's 64-element alignment tail has no shadow)
                size_t o = e;
                if (S.cols != S.dst_ld) { const size_t r = e / (unsigned)S.cols; o = r * S.dst_ld + (e - r * S.cols); }
                put4<CT>(S.dst, o, x);
            }
        }
    }
}

template <typename CT>
__global__ __launch_bounds__(NT) void adam_groups_kernel(const bpm_adam_seg* __restrict__ tab, int nseg, float* __restrict__ p,
                                                        float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        const AdamGroupsK G, int ngroups, float gscale, int zero_grad,
                                                        const float* __restrict__ scale_dev, const float* __restrict__ norm_dev,
                                                        const int* __restrict__ steps_dev) {
    const bpm_adam_seg S = find_desc(tab, nseg, blockIdx.x);
    // block-uniform; ngroups == 0: whatever the word holds, group 0
    adam_block<CT>(S, ngroups ? S.group : 0, p, g, m, v, G, ngroups, gscale, zero_grad, scale_dev, norm_dev, steps_dev);
}

// The same block over SEVERAL buffer sets (bpm_adam_step_sets): the segment's group word names its set (BPM_ADAM_SET_SHIFT)
// beside its group (the low byte, signed), and off4 is relative to that set.  The sets are a device-resident array: one
// block-uniform 32-byte load after find_desc -- a by-value argument indexed by a loaded value would be copied to scratch.
template <typename CT>
__global__ __launch_bounds__(NT) void adam_sets_kernel(const bpm_adam_seg* __restrict__ tab, int nseg,
                                                      const bpm_adam_set* __restrict__ sets, int nsets, const AdamGroupsK G,
                                                      int ngroups, float gscale, int zero_grad, const float* __restrict__ scale_dev,
                                                      const float* __restrict__ norm_dev, const int* __restrict__ steps_dev) {
    const bpm_adam_seg S = find_desc(tab, nseg, blockIdx.x);
    const unsigned set = (unsigned)S.group >> BPM_ADAM_SET_SHIFT;
    if (set >= (unsigned)nsets) return;                  // (the entry has checked the host copy of the table: never taken)
    const bpm_adam_set B = sets[set];
    adam_block<CT>(S, (int)(signed char)(S.group & 0xff), B.param, B.grad, B.exp_avg, B.exp_avg_sq, G, ngroups, gscale, zero_grad,
                   scale_dev, norm_dev, steps_dev);
}

// After the step, one tiny launch: every group's counter of applied steps goes up by one, or, when the step was skipped,
// the skip counter does.  Plain stores from one wave; the stream orders it behind the kernel that read the counters.
__global__ __launch_bounds__(64) void adam_counters_kernel(const float* norm_dev, int* steps_dev, int ngroups, int* skipped_dev) {
    const bool skipped = norm_dev && !adam_norm_finite(norm_dev);
    if (skipped) {
        if (threadIdx.x == 0 && skipped_dev) skipped_dev[0] += 1;
    } else if (steps_dev && (int)threadIdx.x < ngroups) {
        steps_dev[threadIdx.x] += 1;
    }
}

// Fills the launch's copy of the groups.
static int adam_fill_groups(AdamGroupsK& G, const bpm_adam_group* groups, int ngroups, bool host_steps) {
    for (int i = 0; i < ngroups; ++i) {
        const bpm_adam_group& h = groups[i];
        if (host_steps && h.step < 1) return BPM_ERR_ARG;
        AdamGroupK& k = G.g[i];
        k.lr = h.lr; k.b1 = h.beta1; k.b2 = h.beta2; k.eps = h.eps;
        k.wd_l2 = h.decoupled ? 0.f : h.weight_decay;
        k.decay = h.decoupled ? (float)(1.0 - (double)h.lr * (double)h.weight_decay) : 1.f;
        if (host_steps) {
            const double bc1 = 1.0 - pow((double)h.beta1, h.step), bc2 = 1.0 - pow((double)h.beta2, h.step);
            k.lr_c = (float)(h.lr / bc1); k.rsq_bc2 = (float)(1.0 / sqrt(bc2));
        }
    }
    return 0;
}

static int adam_count(int ngroups, const float* norm_dev, int* steps_dev, int* skipped_dev, void* stream) {
    if (!steps_dev && !(skipped_dev && norm_dev)) return 0;
    return launch<adam_counters_kernel>(1, 64, stream, norm_dev, steps_dev, ngroups, skipped_dev);
}

// Fills the launch's copy of the groups and launches.  ngroups_k: what the kernel takes (0: ignore the group words).
static int adam_launch(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param, float* grad,
                       float* exp_avg, float* exp_avg_sq, const bpm_adam_group* groups, int ngroups, int ngroups_k, float grad_scale,
                       const float* scale_dev, const float* norm_dev, int* steps_dev, int* skipped_dev, int zero_grad, void* stream) {
    AdamGroupsK G = {};
    if (const int rc = adam_fill_groups(G, groups, ngroups, !steps_dev)) return rc;
    const int rc = with_ct(dtype, [&](auto ct) {
        return launch<adam_groups_kernel<decltype(ct)>>(total_blocks, NT, stream, table_dev, nseg, param, grad, exp_avg, exp_avg_sq, G,
                                                        ngroups_k, grad_scale, zero_grad, scale_dev, norm_dev, (const int*)steps_dev);
    });
    return rc ? rc : adam_count(ngroups, norm_dev, steps_dev, skipped_dev, stream);
}

extern "C" int bpm_adam_step_groups(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param,
                                    float* grad, float* exp_avg, float* exp_avg_sq, const bpm_adam_group* groups, int ngroups,
                                    float grad_scale, const float* scale_dev, const float* norm_dev, int* steps_dev,
                                    int* skipped_dev, int zero_grad, void* stream) {
    if (!table_dev || nseg < 1 || total_blocks < 1 || !param || !grad || !exp_avg || !exp_avg_sq || !groups) return BPM_ERR_ARG;
    if (ngroups < 1 || ngroups > BPM_ADAM_MAX_GROUPS) return BPM_ERR_ARG;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return BPM_ERR_ALIGN;
    if (((uintptr_t)scale_dev | (uintptr_t)norm_dev | (uintptr_t)steps_dev | (uintptr_t)skipped_dev) & 3) return BPM_ERR_ALIGN;
    return adam_launch(dtype, table_dev, nseg, total_blocks, param, grad, exp_avg, exp_avg_sq, groups, ngroups, ngroups, grad_scale,
                       scale_dev, norm_dev, steps_dev, skipped_dev, zero_grad, stream);
}

// Several buffer sets, one launch and one counter launch.  Every check reads the HOST copies of the table and the sets (the
// arrays the device ones were uploaded from); nothing is launched unless the whole table is sound: sorted and gap-free in
// blocks, every segment inside its set.
extern "C" int bpm_adam_step_sets(int dtype, const bpm_adam_seg* table_dev, const bpm_adam_seg* table_host, int nseg,
                                  unsigned total_blocks, const bpm_adam_set* sets_dev, const bpm_adam_set* sets_host, int nsets,
                                  const bpm_adam_group* groups, int ngroups, float grad_scale, const float* scale_dev,
                                  const float* norm_dev, int* steps_dev, int* skipped_dev, int zero_grad, void* stream) {
    if (!table_dev || !table_host || nseg < 1 || total_blocks < 1 || !sets_dev || !sets_host || !groups) return BPM_ERR_ARG;
    if (nsets < 1 || nsets > BPM_ADAM_MAX_SETS || ngroups < 1 || ngroups > BPM_ADAM_MAX_GROUPS) return BPM_ERR_ARG;
    for (int i = 0; i < nsets; ++i) {
        const bpm_adam_set& b = sets_host[i];
        if (!b.param || !b.grad || !b.exp_avg || !b.exp_avg_sq || b.n == 0 || (b.n & 3)) return BPM_ERR_ARG;
        if (((uintptr_t)b.param | (uintptr_t)b.grad | (uintptr_t)b.exp_avg | (uintptr_t)b.exp_avg_sq) & 15) return BPM_ERR_ALIGN;
    }
    if (((uintptr_t)scale_dev | (uintptr_t)norm_dev | (uintptr_t)steps_dev | (uintptr_t)skipped_dev) & 3) return BPM_ERR_ALIGN;
    unsigned blk = 0;
    for (int i = 0; i < nseg; ++i) {
        const bpm_adam_seg& s = table_host[i];
        const unsigned set = (unsigned)s.group >> BPM_ADAM_SET_SHIFT;
        if (set >= (unsigned)nsets || s.n4 == 0 || s.blk0 != blk) return BPM_ERR_ARG;
        if (s.off4 > sets_host[set].n / 4 || s.n4 > sets_host[set].n / 4 - s.off4) return BPM_ERR_ARG;
        if (s.dst && (s.rows < 1 || s.cols < 4 || (s.cols & 3) || s.dst_ld < s.cols || (size_t)s.rows * s.cols > 4 * (size_t)s.n4))
            return BPM_ERR_ARG;
        blk += (unsigned)bpm_adam_blocks(s.n4);
    }
    if (blk != total_blocks) return BPM_ERR_ARG;
    AdamGroupsK G = {};
    if (const int rc = adam_fill_groups(G, groups, ngroups, !steps_dev)) return rc;
    const int rc = with_ct(dtype, [&](auto ct) {
        return launch<adam_sets_kernel<decltype(ct)>>(total_blocks, NT, stream, table_dev, nseg, sets_dev, nsets, G, ngroups, grad_scale,
                                                      zero_grad, scale_dev, norm_dev, (const int*)steps_dev);
    });
    return rc ? rc : adam_count(ngroups, norm_dev, steps_dev, skipped_dev, stream);
}

// The one-group entries: one L2 group at the host's `step`, no skip, no counters, the segments' group words ignored.
extern "C" int bpm_adam_step_table_clip(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param,
                                        float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, int step, float grad_scale, const float* scale_dev, int zero_grad,
                                        void* stream) {
    if (!table_dev || nseg < 1 || total_blocks < 1 || !param || !grad || !exp_avg || !exp_avg_sq || step < 1) return BPM_ERR_ARG;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return BPM_ERR_ALIGN;
    if ((uintptr_t)scale_dev & 3) return BPM_ERR_ALIGN;
    const bpm_adam_group one = {lr, beta1, beta2, eps, weight_decay, 0, step, 0};
    return adam_launch(dtype, table_dev, nseg, total_blocks, param, grad, exp_avg, exp_avg_sq, &one, 1, 0, grad_scale, scale_dev,
                       nullptr, nullptr, nullptr, zero_grad, stream);
}

extern "C" int bpm_adam_step_table(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param, float* grad,
                                   float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, float grad_scale, int zero_grad, void* stream) {
    return bpm_adam_step_table_clip(dtype, table_dev, nseg, total_blocks, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                                    weight_decay, step, grad_scale, nullptr, zero_grad, stream);
}

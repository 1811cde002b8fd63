// Training criterion of the step (gfx950): BCE-with-logits, cross-entropy and L1 over fp32 logits [B, C], forward with
// the derivative for an upstream gradient of 1, and the scaling of that derivative by the upstream gradient read on the
// device (see bpm_loss_fwd / bpm_loss_bwd).  The tensors are [batch, classes]: a few thousand elements, so arithmetic is
// free -- every element is carried in fp64 and rounded to fp32 once, sums are fp64 in one fixed order (no float atomics:
// loss and gradient are bitwise reproducible).
//
// BCE / L1 (element kinds), N = B*C elements in row-major order:
//   launch 1  block k owns elements [k*EL_CH, (k+1)*EL_CH): a thread takes EL_IT of them, stride NT, writes their
//             derivative (and, reduction none, their loss) and sums their loss in index order; the block's sum (6 shuffle
//             levels, then the four waves in order) goes to ws[k] as one double.  Reduction none: this is all.
//   launch 2  one block: thread t adds partials t, t + NT, ... in index order, then a fixed tree; / N for mean.
// Cross-entropy (row kind):
//   launch 1  block b < B owns row b: maximum, S = sum exp(x - max) (thread-strided, then the fixed tree), the row's
//             loss w (max + log S - x[t]); ws row b = {max, S, loss}.  Block B: W = sum of w[t] over the kept rows in the
//             same fixed order -> ws[3B], and the count of class indices outside [0, C) (one vector atomic add).
//   launch 2  block b < B: gradient row b = (exp(x - max) / S - onehot) w / W;  block B: loss = sum_b loss_b (/ W).
// A class index is compared against [0, C) BEFORE it indexes anything; an index outside is an ignored row.
#include "bpm_common.h"
#include "../../include/bpmult_hip.h"

namespace {

constexpr int NT = 256;
constexpr int EL_IT = 4;
constexpr int EL_CH = NT * EL_IT;       // elements per block of the element kinds

BPM_DEV double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the block's sum in every thread: one fixed shape whatever the values
BPM_DEV double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();                    // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
BPM_DEV float block_max_f(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

struct LossP {
    const float* x; const float* y; const int64_t* t; const float* w;
    float* loss; float* du; double* ws; int* bad;
    long long N; int B, C, ld, ldt, ldd;
    int kind, red;
    int64_t ignore;
};

// kept row: its class index; -1: ignore_index; -2: outside [0, C) (counted, then treated as ignored)
BPM_DEV int ce_class(int64_t t, int64_t ignore, int C) {
    if (t == ignore) return -1;
    if (t < 0 || t >= (int64_t)C) return -2;
    return (int)t;
}

__global__ __launch_bounds__(NT) void loss_elem_kernel(LossP P) {
    __shared__ double red[NT / 64];
    const long long e0 = (long long)blockIdx.x * EL_CH + threadIdx.x;
    const double scale = P.red == BPM_LOSS_MEAN ? 1.0 / (double)P.N : 1.0;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < EL_IT; ++j) {
        const long long e = e0 + (long long)j * NT;
        if (e >= P.N) break;
        const long long b = e / P.C;
        const int c = (int)(e - b * P.C);
        const double x = (double)P.x[b * P.ld + c], y = (double)P.y[b * P.ldt + c];
        double l, d;
        if (P.kind == BPM_LOSS_BCE) {
            const double w = P.w ? 1.0 + ((double)P.w[c] - 1.0) * y : 1.0;
            const double en = exp(-fabs(x));                          // in (0, 1]: never overflows
            const double sneg = (x >= 0.0 ? en : 1.0) / (1.0 + en);    // sigmoid(-x) = 1 - sigmoid(x), no subtraction
            l = (1.0 - y) * x + w * (fmax(-x, 0.0) + log1p(en));
            d = (1.0 - y) - w * sneg;
        } else {
            const double r = x - y;
            l = fabs(r);
            d = (double)(r > 0.0) - (double)(r < 0.0);                // exactly 0 where x == y
        }
        acc += l;
        if (P.red == BPM_LOSS_NONE) P.loss[e] = (float)l;
        if (P.du) P.du[b * P.ldd + c] = (float)(d * scale);
    }
    if (P.red == BPM_LOSS_NONE) return;
    const double s = block_sum_d(acc, red);
    if (threadIdx.x == 0) P.ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void loss_elem_final_kernel(const double* __restrict__ partial, unsigned nblk, double scale,
                                                             float* __restrict__ loss) {
    __shared__ double red[NT / 64];
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < nblk; i += NT) acc += partial[i];
    const double s = block_sum_d(acc, red);
    if (threadIdx.x == 0) loss[0] = (float)(s * scale);
}

__global__ __launch_bounds__(NT) void loss_ce_rows_kernel(LossP P) {
    __shared__ double red[NT / 64];
    __shared__ float redf[NT / 64];
    const int b = blockIdx.x;
    if (b == P.B) {                     // the denominator of `mean` and the count of class indices outside [0, C)
        double acc = 0.0;
        int nbad = 0;
        for (int i = threadIdx.x; i < P.B; i += NT) {
            const int k = ce_class(P.t[i], P.ignore, P.C);
            if (k >= 0) acc += P.w ? (double)P.w[k] : 1.0;
            nbad += k == -2;
        }
        const double W = block_sum_d(acc, red);
        if (threadIdx.x == 0) P.ws[3 * (size_t)P.B] = W;
        if (nbad && P.bad) atomicAdd(P.bad, nbad);
        return;
    }
    const float* x = P.x + (size_t)b * P.ld;
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < P.C; c += NT) mx = fmaxf(mx, x[c]);
    const double m = (double)block_max_f(mx, redf);
    double acc = 0.0;
    for (int c = threadIdx.x; c < P.C; c += NT) acc += exp((double)x[c] - m);
    const double S = block_sum_d(acc, red);
    if (threadIdx.x == 0) {
        const int k = ce_class(P.t[b], P.ignore, P.C);
        double l = 0.0;
        if (k >= 0) l = (P.w ? (double)P.w[k] : 1.0) * ((m - (double)x[k]) + log(S));
        double* r = P.ws + 3 * (size_t)b;
        r[0] = m; r[1] = S; r[2] = l;
        if (P.red == BPM_LOSS_NONE) P.loss[b] = (float)l;
    }
}

__global__ __launch_bounds__(NT) void loss_ce_grad_kernel(LossP P) {
    __shared__ double red[NT / 64];
    const int b = blockIdx.x;
    const double W = P.ws[3 * (size_t)P.B];
    if (b == P.B) {                     // the reduced loss
        double acc = 0.0;
        for (int i = threadIdx.x; i < P.B; i += NT) acc += P.ws[3 * (size_t)i + 2];
        const double s = block_sum_d(acc, red);
        if (threadIdx.x == 0) P.loss[0] = (float)(P.red == BPM_LOSS_MEAN ? s / W : s);
        return;
    }
    if (!P.du) return;
    const int k = ce_class(P.t[b], P.ignore, P.C);
    float* du = P.du + (size_t)b * P.ldd;
    if (k < 0) {                        // ignored row: exactly zero, whatever W is
        for (int c = threadIdx.x; c < P.C; c += NT) du[c] = 0.f;
        return;
    }
    const float* x = P.x + (size_t)b * P.ld;
    const double m = P.ws[3 * (size_t)b], S = P.ws[3 * (size_t)b + 1];
    double f = P.w ? (double)P.w[k] : 1.0;
    if (P.red == BPM_LOSS_MEAN) f /= W;                               // 0 / 0 = NaN, as torch
    for (int c = threadIdx.x; c < P.C; c += NT) {
        const double p = exp((double)x[c] - m) / S;
        du[c] = (float)((c == k ? p - 1.0 : p) * f);
    }
}

// dl = du * g;  gmode 0: one scalar, 1: g[b*ldg + c], 2: g[b]
__global__ __launch_bounds__(NT) void loss_bwd_kernel(const float* __restrict__ du, int ldd, const float* __restrict__ g, int ldg,
                                                      int gmode, float* __restrict__ dl, int lddl, int C, long long N) {
    const long long e0 = (long long)blockIdx.x * EL_CH + threadIdx.x;
#pragma unroll
    for (int j = 0; j < EL_IT; ++j) {
        const long long e = e0 + (long long)j * NT;
        if (e >= N) break;
        const long long b = e / C;
        const int c = (int)(e - b * C);
        const float gv = gmode == 0 ? g[0] : gmode == 1 ? g[b * ldg + c] : g[b];
        dl[b * lddl + c] = du[b * ldd + c] * gv;
    }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool known(const bpm_loss_desc* d) {
    return (d->kind == BPM_LOSS_BCE || d->kind == BPM_LOSS_CE || d->kind == BPM_LOSS_L1) &&
           (d->reduction == BPM_LOSS_MEAN || d->reduction == BPM_LOSS_SUM || d->reduction == BPM_LOSS_NONE);
}
inline long long elem_blocks(long long N) { return (N + EL_CH - 1) / EL_CH; }

}  // namespace

extern "C" size_t bpm_loss_ws_bytes(int kind, int reduction, int B, int C) {
    if (B < 1 || C < 1) return 0;
    if (kind == BPM_LOSS_CE) return (3 * (size_t)B + 1) * sizeof(double);
    if (reduction == BPM_LOSS_NONE) return 0;
    return (size_t)elem_blocks((long long)B * C) * sizeof(double);
}

extern "C" int bpm_loss_fwd(const bpm_loss_desc* d, void* stream) {
    if (!d || !known(d)) return BPM_ERR_ARG;
    if (!d->logits || !d->target || !d->loss || d->B < 1 || d->C < 1 || d->ld < d->C) return BPM_ERR_ARG;
    const bool ce = d->kind == BPM_LOSS_CE;
    if (!ce && d->ldt < d->C) return BPM_ERR_ARG;
    if (d->dlogits_unit && d->ldd < d->C) return BPM_ERR_ARG;
    if (d->kind == BPM_LOSS_L1 && d->weight) return BPM_ERR_ARG;
    const long long N = (long long)d->B * d->C;
    if (elem_blocks(N) > 0x7FFFFFFFll || (ce && d->B == 0x7FFFFFFF)) return BPM_ERR_ARG;
    const size_t need = bpm_loss_ws_bytes(d->kind, d->reduction, d->B, d->C);
    if (need && (!d->ws || d->ws_bytes < need)) return BPM_ERR_ARG;
    if (!al(d->logits, 4) || !al(d->target, ce ? 8 : 4) || !al(d->weight, 4) || !al(d->loss, 4) || !al(d->dlogits_unit, 4) ||
        !al(d->bad, 4) || !al(d->ws, 8))
        return BPM_ERR_ALIGN;
    LossP p;
    p.x = d->logits; p.y = ce ? nullptr : (const float*)d->target; p.t = ce ? (const int64_t*)d->target : nullptr; p.w = d->weight;
    p.loss = d->loss; p.du = d->dlogits_unit; p.ws = (double*)d->ws; p.bad = d->bad;
    p.N = N; p.B = d->B; p.C = d->C; p.ld = d->ld; p.ldt = d->ldt; p.ldd = d->ldd;
    p.kind = d->kind; p.red = d->reduction; p.ignore = d->ignore_index;
    hipStream_t s = (hipStream_t)stream;
    if (ce) {
        hipLaunchKernelGGL(loss_ce_rows_kernel, dim3(d->B + 1), dim3(NT), 0, s, p);
        BPM_CHECK_LAUNCH();
        if (d->reduction != BPM_LOSS_NONE || d->dlogits_unit) {
            // reduction none: no block B (nothing to reduce); its gradient rows do not use W
            hipLaunchKernelGGL(loss_ce_grad_kernel, dim3(d->B + (d->reduction != BPM_LOSS_NONE ? 1 : 0)), dim3(NT), 0, s, p);
            BPM_CHECK_LAUNCH();
        }
        return 0;
    }
    const unsigned nblk = (unsigned)elem_blocks(N);
    hipLaunchKernelGGL(loss_elem_kernel, dim3(nblk), dim3(NT), 0, s, p);
    BPM_CHECK_LAUNCH();
    if (d->reduction != BPM_LOSS_NONE) {
        hipLaunchKernelGGL(loss_elem_final_kernel, dim3(1), dim3(NT), 0, s, (const double*)d->ws, nblk,
                           d->reduction == BPM_LOSS_MEAN ? 1.0 / (double)N : 1.0, d->loss);
        BPM_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int bpm_loss_bwd(const bpm_loss_desc* d, const float* g, int ldg, float* dlogits, int lddl, void* stream) {
    if (!d || !known(d)) return BPM_ERR_ARG;
    if (!d->dlogits_unit || !g || !dlogits || d->B < 1 || d->C < 1 || d->ldd < d->C || lddl < d->C) return BPM_ERR_ARG;
    const int gmode = d->reduction != BPM_LOSS_NONE ? 0 : d->kind == BPM_LOSS_CE ? 2 : 1;
    if (gmode == 1 && ldg < d->C) return BPM_ERR_ARG;
    const long long N = (long long)d->B * d->C;
    if (elem_blocks(N) > 0x7FFFFFFFll) return BPM_ERR_ARG;
    if (!al(d->dlogits_unit, 4) || !al(g, 4) || !al(dlogits, 4)) return BPM_ERR_ALIGN;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)elem_blocks(N)), dim3(NT), 0, (hipStream_t)stream, (const float*)d->dlogits_unit,
                       d->ldd, g, ldg, gmode, dlogits, lddl, d->C, N);
    BPM_CHECK_LAUNCH();
    return 0;
}

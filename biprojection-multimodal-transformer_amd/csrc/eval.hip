// Evaluation of an epoch on the device (gfx950): model_eval of the reference (train.py:165-280) without its four host
// syncs per batch and without scikit-learn.  bpm_eval_update appends one batch to a store the caller owns (one launch,
// no reduction); bpm_eval_finalize turns the N stored rows into counts and fp64 metrics (a few launches); the caller reads
// the result once.  In the style of loss.hip: elements carried in fp64 and rounded once, every floating-point sum fp64
// through one fixed tree, every other combination in integers (integer atomics commute) -- two runs give identical bits.
//
// Average precision of a list (scores s, labels y, P positives) without a sort:
//     AP = (1 / P) sum_{i : y_i = 1} TP>=(s_i) / N>=(s_i)
// N>=(s): elements with score >= s, TP>=(s): the positives among them.  Scores are sigmoids, so non-negative floats, whose
// bit patterns order as unsigned integers: key = bits << 1 | label, and key_j >= (key_i & ~1) <=> s_j >= s_i.
//   ap_count   block = (list, 256 query elements in registers, one split of the list): the split streams through LDS in
//              chunks of AP_CH keys, every lane reads the same address (a broadcast), two integer counters per lane;
//              the splits meet in uint32 counters by vector atomic adds.  Lists: micro (all N C elements) and one per class.
//   ap_quot    block = 1024 elements of a list: the quotients of its positives summed in index order, then the fixed tree.
//   ml_rows    thread = row: the row's own list (C elements: O(C^2) from L1), its F1 and whether every class is right.
//   ml_final   block per list / per class: the partial sums in index order, the class's tp / fp / fn / tn, the loss mean.
// Regression / classes: eval_rows_kernel (1024 rows per block) and eval_rows_final_kernel.
//
// Sharded evaluation: bpm_eval_pack copies a shard's rows, losses and bad counter into one image of 32-bit words,
// bpm_eval_merge lays W such images into a store in rank order (one launch each, bit patterns only): the merged store is
// the store of an unsharded evaluation, so finalize gives the same bits.
#include "bpm_common.h"
#include "../../include/bpmult_hip.h"

namespace {

constexpr int NT = 256;
constexpr int AP_CH = 1024;             // keys per LDS chunk
constexpr int AP_SPLIT = 8192;          // keys of a list that one block of ap_count streams
constexpr int Q_CH = 1024;              // elements per block of ap_quot and of the row kernels
constexpr int REG_D = 6, REG_I = 8;     // doubles / integers a block of eval_rows_kernel leaves

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
BPM_DEV long long block_sum_i(long long v, long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// (float) sigmoid((double) x): one rounding
BPM_DEV float sigmoid_once(float x) {
    const double e = exp(-fabs((double)x));                 // in (0, 1]: never overflows
    return (float)((x >= 0.f ? 1.0 : e) / (1.0 + e));
}

// s * 6 - 3 in two separately rounded fp32 operations, as numpy evaluates preds * 6 - 3 on a float32 array (train.py:261).
// hipcc contracts a * b - c into one fused multiply-add by default (and __fmul_rn / __fsub_rn are plain operators to it):
// contraction is switched off for this function.
BPM_DEV float times6_minus3(float s) {
#pragma clang fp contract(off)
    const float m = s * 6.f;
    return m - 3.f;
}

struct UpdP {
    const float* x; const float* y; const int64_t* t; const float* loss;
    float* score; float* predict; float* raw; float* target; unsigned char* pred; unsigned char* label; float* losses; int* bad;
    int B, C, ld, ldt, n0, batch_index, kind;
};

__global__ __launch_bounds__(NT) void eval_update_kernel(UpdP P) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && P.loss) P.losses[P.batch_index] = P.loss[0];
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    int isbad = 0;
    if (P.kind == BPM_EVAL_MULTILABEL) {
        if (e < (long long)P.B * P.C) {
            const int b = (int)(e / P.C), c = (int)(e - (long long)b * P.C);
            const float s = sigmoid_once(P.x[(size_t)b * P.ld + c]);
            const float y = P.y[(size_t)b * P.ldt + c];
            isbad = !(y == 0.f || y == 1.f);                // NaN is neither
            const size_t o = ((size_t)P.n0 + b) * P.C + c;
            P.score[o] = s;
            P.pred[o] = s > 0.5f;                            // on the fp32 score, as torch.sigmoid(out) > 0.5
            P.label[o] = y == 1.f;
        }
    } else if (e < P.B) {
        const size_t o = (size_t)P.n0 + e;
        if (P.kind == BPM_EVAL_REGRESSION) {
            const float x = P.x[(size_t)e * P.ld];
            const float s = sigmoid_once(x);
            P.score[o] = s;
            P.predict[o] = times6_minus3(s);
            P.raw[o] = x;
            P.target[o] = P.y[e];
        } else {
            const float* x = P.x + (size_t)e * P.ld;
            int k = 0;
            float m = x[0];
            for (int c = 1; c < P.C; ++c)
                if (x[c] > m) { m = x[c]; k = c; }           // first index on ties
            const int64_t t = P.t[e];
            isbad = t < 0 || t >= (int64_t)P.C;
            P.predict[o] = (float)k;
            P.target[o] = isbad ? 0.f : (float)t;
            P.label[o] = !isbad;                             // 1: the row takes part
        }
    }
    const int nbad = __syncthreads_count(isbad);
    if (threadIdx.x == 0 && nbad && P.bad) atomicAdd(P.bad, nbad);
}

// ---------------------------------------------------------------------------------------------------------------------
struct MlP {
    const float* score; const unsigned char* pred; const unsigned char* label; const float* losses;
    uint32_t* cnt_micro; uint32_t* cnt_class;       // [N C][2]: N>=, TP>= of element (n, c) in the micro / its class list
    double* dpart; long long* ppart;                // [nq0 + C nq1]: quotient sums and positives per ap_quot block
    double* rpart; long long* rint;                 // [2 nr], [nr]: row AP / row F1 sums and all-right rows per ml_rows block
    double* result; long long* counts;
    long long NC;
    int N, C, nbatches;
    unsigned t0, s0, t1, s1, nq0, nq1, nr;          // tiles and splits of the micro list / of a class list; block counts
};

BPM_DEV uint32_t ap_key(const MlP& P, size_t idx) { return (__float_as_uint(P.score[idx]) << 1) | (uint32_t)(P.label[idx] != 0); }

__global__ __launch_bounds__(NT) void ap_count_kernel(MlP P) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[AP_CH];
    // which list, tile and split
    unsigned b = blockIdx.x;
    size_t base, stride;
    long long n;
    unsigned tile, split;
    uint32_t* cnt;
    const unsigned micro_blocks = P.t0 * P.s0;
    if (b < micro_blocks) {
        tile = b / P.s0; split = b - tile * P.s0;
        base = 0; stride = 1; n = P.NC; cnt = P.cnt_micro;
    } else {
        b -= micro_blocks;
        const unsigned per = P.t1 * P.s1, c = b / per;
        b -= c * per;
        tile = b / P.s1; split = b - tile * P.s1;
        base = c; stride = (size_t)P.C; n = P.N; cnt = P.cnt_class;
    }
    const long long qi = (long long)tile * NT + threadIdx.x;
    const bool live = qi < n;
    const size_t qidx = base + (size_t)(live ? qi : 0) * stride;
    const uint32_t q = live ? (ap_key(P, qidx) & ~1u) : 0xFFFFFFFFu;
    uint32_t a = 0, p = 0;
    const long long lo = (long long)split * AP_SPLIT, hi = lo + AP_SPLIT < n ? lo + AP_SPLIT : n;
    for (long long c0 = lo; c0 < hi; c0 += AP_CH) {
        const int cn = (int)(hi - c0 < AP_CH ? hi - c0 : AP_CH);
        __syncthreads();                                    // the previous chunk is read
        for (int j = threadIdx.x; j < cn; j += NT) keys[j] = ap_key(P, base + (size_t)(c0 + j) * stride);
        __syncthreads();
        int j = 0;
        for (; j + 4 <= cn; j += 4) {
            const uint4 k = *(const uint4*)&keys[j];        // one address for the wave: broadcast
            a += (k.x >= q) + (k.y >= q) + (k.z >= q) + (k.w >= q);
            p += (k.x >= q ? k.x & 1u : 0u) + (k.y >= q ? k.y & 1u : 0u) + (k.z >= q ? k.z & 1u : 0u) + (k.w >= q ? k.w & 1u : 0u);
        }
        for (; j < cn; ++j) {
            const uint32_t k = keys[j];
            a += k >= q;
            p += k >= q ? k & 1u : 0u;
        }
    }
    if (live) {
        atomicAdd(&cnt[2 * qidx], a);
        atomicAdd(&cnt[2 * qidx + 1], p);
    }
}

__global__ __launch_bounds__(NT) void ap_quot_kernel(MlP P) {
    __shared__ double red[NT / 64];
    __shared__ long long redi[NT / 64];
    unsigned b = blockIdx.x;
    size_t base, stride;
    long long n;
    const uint32_t* cnt;
    unsigned chunk;
    if (b < P.nq0) {
        chunk = b; base = 0; stride = 1; n = P.NC; cnt = P.cnt_micro;
    } else {
        const unsigned c = (b - P.nq0) / P.nq1;
        chunk = (b - P.nq0) - c * P.nq1; base = c; stride = (size_t)P.C; n = P.N; cnt = P.cnt_class;
    }
    double acc = 0.0;
    long long pos = 0;
#pragma unroll
    for (int j = 0; j < Q_CH / NT; ++j) {
        const long long i = (long long)chunk * Q_CH + j * NT + threadIdx.x;
        if (i >= n) break;
        const size_t idx = base + (size_t)i * stride;
        if (P.label[idx]) {
            acc += (double)cnt[2 * idx + 1] / (double)cnt[2 * idx];      // N>= counts the element itself: never 0
            ++pos;
        }
    }
    const double s = block_sum_d(acc, red);
    const long long np = block_sum_i(pos, redi);
    if (threadIdx.x == 0) { P.dpart[blockIdx.x] = s; P.ppart[blockIdx.x] = np; }
}

__global__ __launch_bounds__(NT) void ml_rows_kernel(MlP P) {
    __shared__ double red[NT / 64];
    __shared__ long long redi[NT / 64];
    const long long r = (long long)blockIdx.x * NT + threadIdx.x;
    double ap = 0.0, f1 = 0.0;
    long long right = 0;
    if (r < P.N) {
        const float* s = P.score + (size_t)r * P.C;
        const unsigned char* y = P.label + (size_t)r * P.C;
        const unsigned char* pr = P.pred + (size_t)r * P.C;
        int ny = 0, np = 0, both = 0, same = 0;
        double acc = 0.0;
        for (int i = 0; i < P.C; ++i) {
            ny += y[i] != 0; np += pr[i] != 0; both += y[i] && pr[i]; same += (y[i] != 0) == (pr[i] != 0);
            if (!y[i]) continue;
            const uint32_t q = __float_as_uint(s[i]);
            int a = 0, tp = 0;
            for (int j = 0; j < P.C; ++j) {
                const bool ge = __float_as_uint(s[j]) >= q;
                a += ge; tp += ge && y[j];
            }
            acc += (double)tp / (double)a;
        }
        ap = ny ? acc / (double)ny : 0.0;                    // a row without a positive counts as 0
        f1 = ny + np ? 2.0 * (double)both / (double)(ny + np) : 0.0;
        right = same == P.C;
    }
    const double sa = block_sum_d(ap, red), sf = block_sum_d(f1, red);
    const long long nr = block_sum_i(right, redi);
    if (threadIdx.x == 0) { P.rpart[2 * blockIdx.x] = sa; P.rpart[2 * blockIdx.x + 1] = sf; P.rint[blockIdx.x] = nr; }
}

// thread-strided in index order, then the fixed tree
BPM_DEV double strided_sum_d(const double* v, unsigned n, unsigned step, double* red) {
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < n; i += NT) acc += v[(size_t)i * step];
    return block_sum_d(acc, red);
}
BPM_DEV long long strided_sum_i(const long long* v, unsigned n, long long* redi) {
    long long acc = 0;
    for (unsigned i = threadIdx.x; i < n; i += NT) acc += v[i];
    return block_sum_i(acc, redi);
}
BPM_DEV double loss_mean(const float* losses, int nb, double* red) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) acc += (double)losses[i];
    const double s = block_sum_d(acc, red);
    return nb > 0 ? s / (double)nb : NAN;
}

// result: [0] loss, [1, C] AP per class, [1 + C] AP micro, [2 + C] AP samples, [3 + C] F1 samples
// counts: [4 c + {0, 1, 2, 3}] tp, fp, fn, tn of class c, [4 C] rows with every class right
__global__ __launch_bounds__(NT) void ml_final_kernel(MlP P) {
    __shared__ double red[NT / 64];
    __shared__ long long redi[NT / 64];
    const int b = blockIdx.x;
    if (b == 0) {                                            // micro
        const double s = strided_sum_d(P.dpart, P.nq0, 1, red);
        const long long np = strided_sum_i(P.ppart, P.nq0, redi);
        if (threadIdx.x == 0) P.result[1 + P.C] = np ? s / (double)np : 0.0;
    } else if (b <= P.C) {                                   // class b - 1
        const int c = b - 1;
        const size_t o = (size_t)P.nq0 + (size_t)c * P.nq1;
        const double s = strided_sum_d(P.dpart + o, P.nq1, 1, red);
        const long long np = strided_sum_i(P.ppart + o, P.nq1, redi);
        long long tp = 0, fp = 0, fn = 0, tn = 0;
        for (int r = threadIdx.x; r < P.N; r += NT) {
            const bool y = P.label[(size_t)r * P.C + c], p = P.pred[(size_t)r * P.C + c];
            tp += y && p; fp += !y && p; fn += y && !p; tn += !y && !p;
        }
        tp = block_sum_i(tp, redi); fp = block_sum_i(fp, redi); fn = block_sum_i(fn, redi); tn = block_sum_i(tn, redi);
        if (threadIdx.x == 0) {
            P.result[1 + c] = np ? s / (double)np : 0.0;    // no positive: 0, scikit-learn's answer under its warning
            long long* k = P.counts + 4 * (size_t)c;
            k[0] = tp; k[1] = fp; k[2] = fn; k[3] = tn;
        }
    } else if (b == P.C + 1) {                               // the row means
        const double sa = strided_sum_d(P.rpart, P.nr, 2, red), sf = strided_sum_d(P.rpart + 1, P.nr, 2, red);
        const long long nr = strided_sum_i(P.rint, P.nr, redi);
        if (threadIdx.x == 0) {
            P.result[2 + P.C] = sa / (double)P.N;
            P.result[3 + P.C] = sf / (double)P.N;
            P.counts[4 * (size_t)P.C] = nr;
        }
    } else {
        const double l = loss_mean(P.losses, P.nbatches, red);
        if (threadIdx.x == 0) P.result[0] = l;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct RowP {
    const float* predict; const float* target; const unsigned char* label; const float* losses;
    double* dpart; long long* ipart; double* result; long long* counts;
    int N, nbatches, kind;
    unsigned nblk;
};

// dpart [blk][6]: sum |p - t|, p, t, p p, t t, p t;  ipart [blk][8]: rint(p) == rint(t), then over t != 0 the 2 x 2 of p > 0 against
// t > 0 (both, p only, t only, neither), p == t, rows that take part, rows with t != 0
__global__ __launch_bounds__(NT) void eval_rows_kernel(RowP P) {
    __shared__ double red[NT / 64];
    __shared__ long long redi[NT / 64];
    double d[REG_D] = {0, 0, 0, 0, 0, 0};
    long long k[REG_I] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < Q_CH / NT; ++j) {
        const long long i = (long long)blockIdx.x * Q_CH + j * NT + threadIdx.x;
        if (i >= P.N) break;
        if (P.kind == BPM_EVAL_CLASSES && !P.label[i]) continue;
        const float pf = P.kind == BPM_EVAL_CLASSES ? times6_minus3(P.predict[i]) : P.predict[i];
        const float tf = P.target[i];
        const double p = (double)pf, t = (double)tf;
        d[0] += fabs(p - t); d[1] += p; d[2] += t; d[3] += p * p; d[4] += t * t; d[5] += p * t;
        k[0] += rintf(pf) == rintf(tf);                      // round-half-even, as np.round
        if (tf != 0.f) {
            const bool pp = pf > 0.f, tp = tf > 0.f;
            k[1] += pp && tp; k[2] += pp && !tp; k[3] += !pp && tp; k[4] += !pp && !tp;
            ++k[7];
        }
        k[5] += P.predict[i] == tf;
        ++k[6];
    }
#pragma unroll
    for (int j = 0; j < REG_D; ++j) {
        const double s = block_sum_d(d[j], red);
        if (threadIdx.x == 0) P.dpart[(size_t)blockIdx.x * REG_D + j] = s;
    }
#pragma unroll
    for (int j = 0; j < REG_I; ++j) {
        const long long s = block_sum_i(k[j], redi);
        if (threadIdx.x == 0) P.ipart[(size_t)blockIdx.x * REG_I + j] = s;
    }
}

// result: [0] loss, [1 + j] the sums above; counts: the integers above
__global__ __launch_bounds__(NT) void eval_rows_final_kernel(RowP P) {
    __shared__ double red[NT / 64];
    __shared__ long long redi[NT / 64];
    for (int j = 0; j < REG_D; ++j) {
        const double s = strided_sum_d(P.dpart + j, P.nblk, REG_D, red);
        if (threadIdx.x == 0) P.result[1 + j] = s;
    }
    for (int j = 0; j < REG_I; ++j) {
        long long acc = 0;
        for (unsigned i = threadIdx.x; i < P.nblk; i += NT) acc += P.ipart[(size_t)i * REG_I + j];
        const long long s = block_sum_i(acc, redi);
        if (threadIdx.x == 0) P.counts[j] = s;
    }
    const double l = loss_mean(P.losses, P.nbatches, red);
    if (threadIdx.x == 0) P.result[0] = l;
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool known(int kind) { return kind == BPM_EVAL_MULTILABEL || kind == BPM_EVAL_REGRESSION || kind == BPM_EVAL_CLASSES; }
inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
// the store a kind uses, all present
inline bool store_ok(const bpm_eval_desc* d) {
    if (d->kind == BPM_EVAL_MULTILABEL) return d->score && d->pred && d->label;
    if (d->kind == BPM_EVAL_REGRESSION) return d->score && d->predict && d->raw && d->target;
    return d->predict && d->target && d->label;
}
inline bool store_aligned(const bpm_eval_desc* d) {
    return al(d->score, 4) && al(d->predict, 4) && al(d->raw, 4) && al(d->target, 4) && al(d->losses, 4) && al(d->bad, 4);
}
// elements of the store at `rows` rows must be addressable with the 32-bit block counts used here
inline bool sizes_ok(int kind, long long rows, int C) {
    if (kind != BPM_EVAL_MULTILABEL) return true;
    return rows * C <= 0x7FFFFFFFll;
}

struct MlLayout { size_t cnt_micro, cnt_class, dpart, ppart, rpart, rint, total; unsigned nq0, nq1, nr; };
inline MlLayout ml_layout(size_t N, size_t C) {
    MlLayout L;
    const size_t NC = N * C;
    L.nq0 = (unsigned)cdiv(NC, Q_CH); L.nq1 = (unsigned)cdiv(N, Q_CH); L.nr = (unsigned)cdiv(N, NT);
    const size_t nq = L.nq0 + C * L.nq1;
    size_t o = 0;
    L.cnt_micro = o; o += NC * 8;
    L.cnt_class = o; o += NC * 8;
    L.dpart = o; o += nq * 8;
    L.ppart = o; o += nq * 8;
    L.rpart = o; o += (size_t)L.nr * 16;
    L.rint = o; o += (size_t)L.nr * 8;
    L.total = o;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------------
// The exchange image of a shard: 32-bit words, every field as its bit pattern.  For an image of `rows` rows and `batches`
// losses (E = rows C elements for BPM_EVAL_MULTILABEL, rows otherwise):
//     [0] bad   [1] void mark   [2, 2 + batches) losses   then the 32-bit fields, E words each, then the byte fields,
//     ceil(E / 4) words each, byte i of a field in bits 8 (i & 3) of its word i >> 2.
// The void mark is 0 from pack; a rank that finds its shard is not what the ranks agreed on sets it in its slot instead of
// packing, and a merge that meets one leaves bad = -1 for the one host read to find.
// Fields in order -- multilabel: score | pred, label; regression: score, predict, raw, target; classes: predict, target |
// label.  Words past the shard's own n rows / nb losses are zero.
struct ImgLayout { size_t losses, w[4], b[2], total; int nw, nb; };
inline ImgLayout img_layout(int kind, size_t rows, size_t batches, size_t C) {
    ImgLayout L = {};
    const size_t E = kind == BPM_EVAL_MULTILABEL ? rows * C : rows;
    L.nw = kind == BPM_EVAL_MULTILABEL ? 1 : kind == BPM_EVAL_REGRESSION ? 4 : 2;
    L.nb = kind == BPM_EVAL_MULTILABEL ? 2 : kind == BPM_EVAL_REGRESSION ? 0 : 1;
    size_t o = 2;
    L.losses = o; o += batches;
    for (int k = 0; k < L.nw; ++k) { L.w[k] = o; o += E; }
    for (int k = 0; k < L.nb; ++k) { L.b[k] = o; o += cdiv(E, 4); }
    L.total = o;
    return L;
}

struct ImgFields { uint32_t* w[4]; unsigned char* b[2]; };
inline ImgFields img_fields(const bpm_eval_desc* d) {
    ImgFields f = {};
    if (d->kind == BPM_EVAL_MULTILABEL) {
        f.w[0] = (uint32_t*)d->score; f.b[0] = d->pred; f.b[1] = d->label;
    } else if (d->kind == BPM_EVAL_REGRESSION) {
        f.w[0] = (uint32_t*)d->score; f.w[1] = (uint32_t*)d->predict; f.w[2] = (uint32_t*)d->raw; f.w[3] = (uint32_t*)d->target;
    } else {
        f.w[0] = (uint32_t*)d->predict; f.w[1] = (uint32_t*)d->target; f.b[0] = d->label;
    }
    return f;
}

struct PackP {
    ImgFields f; ImgLayout L;
    const uint32_t* losses; const int* bad;
    uint32_t* image;
    size_t words, E;                    // words of the image (all written), elements the shard holds
    int nb;
};

// thread = one word of the image
__global__ __launch_bounds__(NT) void eval_pack_kernel(PackP P) {
    const size_t w = (size_t)blockIdx.x * NT + threadIdx.x;
    if (w >= P.words) return;
    uint32_t v = 0;
    if (w == 0) {
        v = P.bad ? (uint32_t)P.bad[0] : 0u;
    } else if (w < P.L.losses) {                            // the void mark: 0
    } else if (w < P.L.w[0]) {
        const size_t i = w - P.L.losses;
        if (i < (size_t)P.nb) v = P.losses[i];
    } else if (w < P.L.total) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < P.L.nw && w >= P.L.w[k] && w - P.L.w[k] < P.E) v = P.f.w[k][w - P.L.w[k]];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < P.L.nb && w >= P.L.b[k]) {
                const size_t i = (w - P.L.b[k]) * 4;       // a later byte field's words start past this one's: i >= E there
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j < P.E) v |= (uint32_t)P.f.b[k][i + j] << (8 * j);
            }
    }
    P.image[w] = v;
}

struct MergeP {
    ImgFields f; ImgLayout L;
    const uint32_t* images; size_t stride;      // words from one rank's image to the next
    uint32_t* losses; int* bad;
    int W, C;                                   // C: elements per row (1 unless multilabel)
    int row0[BPM_EVAL_MAX_RANKS + 1], b0[BPM_EVAL_MAX_RANKS + 1];
};

// block = (256 elements, rank): thread = one element of that rank's shard, every field of it.  The byte fields land at
// (row0 C + e), any residue mod 4: byte stores.
__global__ __launch_bounds__(NT) void eval_merge_kernel(MergeP P) {
    const int r = blockIdx.y;
    const uint32_t* img = P.images + (size_t)r * P.stride;
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (r == 0 && e == 0 && P.bad) {
        int s = 0;
        uint32_t mark = 0;
        for (int q = 0; q < P.W; ++q) { s += (int)P.images[(size_t)q * P.stride]; mark |= P.images[(size_t)q * P.stride + 1]; }
        P.bad[0] = mark ? -1 : s;
    }
    const size_t nb = (size_t)(P.b0[r + 1] - P.b0[r]);
    if (e < nb) P.losses[(size_t)P.b0[r] + e] = img[P.L.losses + e];
    const size_t E = (size_t)(P.row0[r + 1] - P.row0[r]) * P.C;
    if (e >= E) return;
    const size_t o = (size_t)P.row0[r] * P.C + e;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < P.L.nw) P.f.w[k][o] = img[P.L.w[k] + e];
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (k < P.L.nb) P.f.b[k][o] = (unsigned char)(img[P.L.b[k] + (e >> 2)] >> (8 * (e & 3)));
}

}  // namespace

extern "C" size_t bpm_eval_ws_bytes(int kind, int capacity, int C) {
    if (!known(kind) || capacity < 1 || C < 1 || !sizes_ok(kind, capacity, C)) return 0;
    if (kind == BPM_EVAL_MULTILABEL) return ml_layout((size_t)capacity, (size_t)C).total;
    return cdiv((size_t)capacity, Q_CH) * (REG_D + REG_I) * 8;
}

extern "C" int bpm_eval_update(const bpm_eval_desc* d, void* stream) {
    if (!d || !known(d->kind)) return BPM_ERR_ARG;
    if (!d->logits || !d->targets || !store_ok(d) || d->B < 1 || d->C < 1 || d->capacity < 1 || d->n0 < 0 ||
        (long long)d->n0 + d->B > d->capacity || d->ld < d->C)
        return BPM_ERR_ARG;
    if (d->kind == BPM_EVAL_MULTILABEL && d->ldt < d->C) return BPM_ERR_ARG;
    if (d->kind == BPM_EVAL_REGRESSION && d->C != 1) return BPM_ERR_ARG;
    if (d->loss && (!d->losses || d->batch_index < 0 || d->batch_index >= d->max_batches)) return BPM_ERR_ARG;
    if (!sizes_ok(d->kind, d->capacity, d->C)) return BPM_ERR_ARG;
    if (!store_aligned(d) || !al(d->logits, 4) || !al(d->loss, 4) || !al(d->targets, d->kind == BPM_EVAL_CLASSES ? 8 : 4))
        return BPM_ERR_ALIGN;
    UpdP p;
    p.x = d->logits;
    p.y = d->kind == BPM_EVAL_CLASSES ? nullptr : (const float*)d->targets;
    p.t = d->kind == BPM_EVAL_CLASSES ? (const int64_t*)d->targets : nullptr;
    p.loss = d->loss;
    p.score = d->score; p.predict = d->predict; p.raw = d->raw; p.target = d->target; p.pred = d->pred; p.label = d->label;
    p.losses = d->losses; p.bad = d->bad;
    p.B = d->B; p.C = d->C; p.ld = d->ld; p.ldt = d->ldt; p.n0 = d->n0; p.batch_index = d->batch_index; p.kind = d->kind;
    const size_t work = d->kind == BPM_EVAL_MULTILABEL ? (size_t)d->B * d->C : (size_t)d->B;
    hipLaunchKernelGGL(eval_update_kernel, dim3((unsigned)cdiv(work, NT)), dim3(NT), 0, (hipStream_t)stream, p);
    BPM_CHECK_LAUNCH();
    return 0;
}

extern "C" int bpm_eval_finalize(const bpm_eval_desc* d, void* stream) {
    if (!d || !known(d->kind)) return BPM_ERR_ARG;
    if (!store_ok(d) || !d->result || !d->counts || d->C < 1 || d->capacity < 1 || d->N < 1 || d->N > d->capacity ||
        d->nbatches < 0 || d->nbatches > d->max_batches || (d->nbatches && !d->losses))
        return BPM_ERR_ARG;
    if (d->kind == BPM_EVAL_REGRESSION && d->C != 1) return BPM_ERR_ARG;
    if (!sizes_ok(d->kind, d->capacity, d->C)) return BPM_ERR_ARG;
    const size_t need = d->kind == BPM_EVAL_MULTILABEL ? ml_layout((size_t)d->N, (size_t)d->C).total
                                                       : cdiv((size_t)d->N, Q_CH) * (REG_D + REG_I) * 8;
    if (!d->ws || d->ws_bytes < need) return BPM_ERR_ARG;
    if (!store_aligned(d) || !al(d->result, 8) || !al(d->counts, 8) || !al(d->ws, 8)) return BPM_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->ws;
    if (d->kind != BPM_EVAL_MULTILABEL) {
        RowP p;
        p.predict = d->predict; p.target = d->target; p.label = d->label; p.losses = d->losses;
        p.nblk = (unsigned)cdiv((size_t)d->N, Q_CH);
        p.dpart = (double*)ws; p.ipart = (long long*)(ws + (size_t)p.nblk * REG_D * 8);
        p.result = d->result; p.counts = (long long*)d->counts;
        p.N = d->N; p.nbatches = d->nbatches; p.kind = d->kind;
        hipLaunchKernelGGL(eval_rows_kernel, dim3(p.nblk), dim3(NT), 0, s, p);
        BPM_CHECK_LAUNCH();
        hipLaunchKernelGGL(eval_rows_final_kernel, dim3(1), dim3(NT), 0, s, p);
        BPM_CHECK_LAUNCH();
        return 0;
    }
    const MlLayout L = ml_layout((size_t)d->N, (size_t)d->C);
    MlP p;
    p.score = d->score; p.pred = d->pred; p.label = d->label; p.losses = d->losses;
    p.cnt_micro = (uint32_t*)(ws + L.cnt_micro); p.cnt_class = (uint32_t*)(ws + L.cnt_class);
    p.dpart = (double*)(ws + L.dpart); p.ppart = (long long*)(ws + L.ppart);
    p.rpart = (double*)(ws + L.rpart); p.rint = (long long*)(ws + L.rint);
    p.result = d->result; p.counts = (long long*)d->counts;
    p.N = d->N; p.C = d->C; p.NC = (long long)d->N * d->C; p.nbatches = d->nbatches;
    p.t0 = (unsigned)cdiv((size_t)p.NC, NT); p.s0 = (unsigned)cdiv((size_t)p.NC, AP_SPLIT);
    p.t1 = (unsigned)cdiv((size_t)d->N, NT); p.s1 = (unsigned)cdiv((size_t)d->N, AP_SPLIT);
    p.nq0 = L.nq0; p.nq1 = L.nq1; p.nr = L.nr;
    const unsigned long long count_blocks = (unsigned long long)p.t0 * p.s0 + (unsigned long long)d->C * p.t1 * p.s1;
    if (count_blocks > 0x7FFFFFFFull) return BPM_ERR_ARG;
    hipError_t e = hipMemsetAsync(ws + L.cnt_micro, 0, (size_t)p.NC * 16, s);     // both counter arrays, adjacent
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ap_count_kernel, dim3((unsigned)count_blocks), dim3(NT), 0, s, p);
    BPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ap_quot_kernel, dim3(p.nq0 + (unsigned)d->C * p.nq1), dim3(NT), 0, s, p);
    BPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ml_rows_kernel, dim3(p.nr), dim3(NT), 0, s, p);
    BPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ml_final_kernel, dim3((unsigned)d->C + 3), dim3(NT), 0, s, p);
    BPM_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t bpm_eval_image_bytes(int kind, int rows, int batches, int C) {
    if (!known(kind) || rows < 0 || batches < 0 || C < 1 || (kind == BPM_EVAL_REGRESSION && C != 1) || !sizes_ok(kind, rows, C)) return 0;
    return img_layout(kind, (size_t)rows, (size_t)batches, (size_t)C).total * 4;
}

extern "C" int bpm_eval_pack(const bpm_eval_desc* d, int n, int nb, int rows, int batches, void* image, size_t image_bytes,
                             void* stream) {
    if (!d || !known(d->kind)) return BPM_ERR_ARG;
    if (!store_ok(d) || !image || d->C < 1 || d->capacity < 1 || n < 0 || n > d->capacity || n > rows || nb < 0 ||
        nb > d->max_batches || nb > batches || (nb && !d->losses))
        return BPM_ERR_ARG;
    if (d->kind == BPM_EVAL_REGRESSION && d->C != 1) return BPM_ERR_ARG;
    if (!sizes_ok(d->kind, d->capacity, d->C) || !sizes_ok(d->kind, rows, d->C)) return BPM_ERR_ARG;
    PackP p;
    p.L = img_layout(d->kind, (size_t)rows, (size_t)batches, (size_t)d->C);
    if ((image_bytes & 3) || image_bytes / 4 < p.L.total) return BPM_ERR_ARG;
    if (!store_aligned(d) || !al(image, 4)) return BPM_ERR_ALIGN;
    p.f = img_fields(d);
    p.losses = (const uint32_t*)d->losses; p.bad = d->bad;
    p.image = (uint32_t*)image;
    p.words = image_bytes / 4;
    p.E = (size_t)n * (d->kind == BPM_EVAL_MULTILABEL ? d->C : 1);
    p.nb = nb;
    const size_t blocks = cdiv(p.words, NT);
    if (blocks > 0x7FFFFFFFull) return BPM_ERR_ARG;
    hipLaunchKernelGGL(eval_pack_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, p);
    BPM_CHECK_LAUNCH();
    return 0;
}

extern "C" int bpm_eval_merge(const bpm_eval_desc* d, const void* images, size_t image_bytes, int W, const int* rows,
                              const int* batches, void* stream) {
    if (!d || !known(d->kind)) return BPM_ERR_ARG;
    if (!store_ok(d) || !images || !rows || !batches || W < 1 || W > BPM_EVAL_MAX_RANKS || d->C < 1 || d->capacity < 1)
        return BPM_ERR_ARG;
    if (d->kind == BPM_EVAL_REGRESSION && d->C != 1) return BPM_ERR_ARG;
    if (!sizes_ok(d->kind, d->capacity, d->C)) return BPM_ERR_ARG;
    MergeP p;
    long long nrows = 0, nbat = 0;
    int rmax = 0, bmax = 0;
    for (int r = 0; r < W; ++r) {
        if (rows[r] < 0 || batches[r] < 0) return BPM_ERR_ARG;
        p.row0[r] = (int)nrows; p.b0[r] = (int)nbat;
        nrows += rows[r]; nbat += batches[r];
        if (nrows > d->capacity || nbat > d->max_batches) return BPM_ERR_ARG;
        rmax = rows[r] > rmax ? rows[r] : rmax; bmax = batches[r] > bmax ? batches[r] : bmax;
    }
    for (int r = W; r <= BPM_EVAL_MAX_RANKS; ++r) { p.row0[r] = (int)nrows; p.b0[r] = (int)nbat; }
    if (nbat && !d->losses) return BPM_ERR_ARG;
    p.L = img_layout(d->kind, (size_t)rmax, (size_t)bmax, (size_t)d->C);       // the common size: that of the largest shard
    if ((image_bytes & 3) || image_bytes / 4 < p.L.total) return BPM_ERR_ARG;
    if (!store_aligned(d) || !al(images, 4)) return BPM_ERR_ALIGN;
    p.f = img_fields(d);
    p.images = (const uint32_t*)images; p.stride = image_bytes / 4;
    p.losses = (uint32_t*)d->losses; p.bad = d->bad;
    p.W = W; p.C = d->kind == BPM_EVAL_MULTILABEL ? d->C : 1;
    size_t work = (size_t)rmax * p.C;
    work = work > (size_t)bmax ? work : (size_t)bmax;
    const size_t blocks = cdiv(work > 0 ? work : 1, NT);                        // an all-empty merge still writes bad
    hipLaunchKernelGGL(eval_merge_kernel, dim3((unsigned)blocks, (unsigned)W), dim3(NT), 0, (hipStream_t)stream, p);
    BPM_CHECK_LAUNCH();
    return 0;
}

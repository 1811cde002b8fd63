// Head-averaged attention maps for BPMulT on gfx950 (bpm_attn_maps / _amask / _hmask / _kmask / _kamask): the kernel and its
// five entries; below them the per-head maps (bpm_attn_head_maps / ...): a kernel of their own and five entries.
// What it shares with the forward / backward kernels of attention.hip is in attn_common.h.
#include "attn_common.h"

namespace {

// ---------------------------------------------------------------------------
// head-averaged attention maps: W[b][i][j] = (1/H) sum_h exp(S_h[i][j] - LSE_h[i])  (0 for a masked key)
// ---------------------------------------------------------------------------
// The probabilities before dropout, recomputed from the Q / K images and the LSE a forward pass left (what the backward
// kernels do), summed over the heads in registers and written once as fp32 [B, T, ldw]: the reference's second return
// value (multihead_attention.py:132-135).  dK / dV orientation, S = Qs K^T (rows = queries, lane = key): the 16 lanes of
// an MFMA column group hold 16 consecutive keys of one query row, so every store instruction writes four 64-byte row
// segments.  One workgroup owns a (batch element, 64-query tile, 64-key tile) of one problem -- a wave 16 of its keys --
// and loops over the heads: the head's 64 Q rows pass through the LDS image (RowStage, loaded one head ahead), its 16 K
// rows stay in registers as the B operand (also loaded one head ahead), the LSE of the tile's rows sits beside the image.
// Neighbouring workgroups (key tiles of one query tile) read the same Q rows: they meet in L2 (xcd_remap).
// Fully masked tiles are skipped block-uniformly and written as zeros; a masked element is exp2(-inf) = 0 in every
// head, so it is stored as exactly 0.0f.
//
// Waves per SIMD each instantiation is compiled for (register budget 512 / waves; the kernel holds 16 accumulators, 16
// scores, two sets of K fragments and the Q staging registers), bf16 / f32 registers used at head_dim 32, 64, 128, 256:
//   bf16  74 / 88 / 116 / 166  ->  4, 4, 4, 3 waves        f32  92 / 116 / 168 / 296  ->  4, 4, 3, 1 waves
// (f32 at 256: 64 + 64 K-fragment and 64 staging registers; 14 registers spill at two waves, none at one -- the
// parity-mode corner).  No instantiation spills: scratch size 0 in the gfx950 assembly of all eight.
// With an additive mask (am) the tile's 16 mask registers spill at three waves (bf16 at 256: 60 bytes, f32 at 128: 52): two.
template <typename CT>
constexpr int map_waves(int dhp, bool am = false) {
    const bool bf = sizeof(CT) == 2;
    if (dhp <= 64 || (bf && dhp <= 128)) return 4;
    if (dhp <= 128 || bf) return am ? 2 : 3;
    return 1;
}
constexpr int MQT = 64;     // queries per tile of the maps kernel

struct MProb {
    const char* Q; const char* K;
    const float* lse;
    float* W; int ldw;
    int B, H, T, S;
    int mask_off, qpos0, qstride;
    int blk0, nqt, nkt;     // block prefix / query tiles / key tiles
};
struct MGroup {
    int nprob;
    MProb p[BPM_MAX_GROUP];
};

// AM (bpm_attn_maps_amask): the additive mask through its transpose, as in the dK / dV kernel (lane = key, four queries
// per register group).  With one image for all heads the tile's mask values are loaded once, before the head loop.
// PH (taken when a mask of the launch has a head stride): they are loaded inside the loop, from the head's image -- an
// instantiation of its own, so the one above keeps its registers (bf16 at 128 and f32 at 64 would spill 12 / 28 bytes at
// four waves with both paths in one kernel).
struct MGroupA {
    MGroup g;
    AAdd m[BPM_MAX_GROUP];
};
// KB (bpm_attn_maps_kmask / _kamask): the per-key byte mask of the *_kmask entries, as in the dK / dV kernel: the lane
// reads the byte of its key once (never at j >= S); a hidden key sees no query row, so every probability of its column is
// exp2(-inf) = 0 in every head and the map holds exactly 0.0f there.  A tile without a visible key is skipped
// block-uniformly.  The descriptors sit behind the additive ones in an argument block of their own (MGroupK), so the
// instantiations without KB keep their argument layout.  The switch rides in the compute-type argument (WithBytes).  One more live register (ilo is per lane either way); no
// instantiation needs another occupancy than its sibling without KB.
struct MGroupK {
    MGroupA a;              // a.m: used with AM only
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(MGroupA) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(sizeof(MGroupK) <= 4096, "kernel arguments are limited to 4 KiB");
BPM_DEV const MGroup& map_group(const MGroup& g) { return g; }
BPM_DEV const MGroup& map_group(const MGroupA& g) { return g.g; }
BPM_DEV const MGroup& map_group(const MGroupK& g) { return g.a.g; }
BPM_DEV const AAdd& map_add(const MGroupA& g, int pi) { return g.m[pi]; }
BPM_DEV const AAdd& map_add(const MGroupK& g, int pi) { return g.a.m[pi]; }

// CTX: the compute type, or WithBytes<compute type> for KB
template <typename CTX, int DHP, bool AM = false, bool PH = false>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(map_waves<typename CtOf<CTX>::type>(DHP, AM), map_waves<typename CtOf<CTX>::type>(DHP, AM)))) void attn_maps_kernel(const std::conditional_t<CtOf<CTX>::bytes, MGroupK, std::conditional_t<AM, MGroupA, MGroup>> ga) {
    static_assert(AM || !PH, "a head stride belongs to an additive mask");
    typedef typename CtOf<CTX>::type CT;
    constexpr bool KB = CtOf<CTX>::bytes;
    const MGroup& grp = map_group(ga);
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    __shared__ __attribute__((aligned(16))) char smem[MQT * C::STRIDE + MQT * 4];
    char* qimg = smem;
    float* s_lse = (float*)(smem + MQT * C::STRIDE);            // -lse * log2(e) of the tile's query rows

    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const MProb& P = grp.p[pi];
    bid -= P.blk0;
    const int kb = bid % P.nkt, qt = (bid / P.nkt) % P.nqt, b = bid / (P.nkt * P.nqt);     // key tiles of a query tile are neighbours

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int j0 = kb * 64 + wave * 16;                 // wave-uniform first key
    const int j = j0 + c;                               // this lane's key
    const int i0 = qt * MQT;                            // first query row of the tile
    float* Wb = P.W + ((size_t)b * P.T + i0) * P.ldw;   // row i0 of this batch element's map

    // query row i (time qpos0 + i*qstride) sees key j iff i >= first_row(j - mask_off + 1)   (the dK / dV kernel's rule)
    auto first_row = [&](int tmin) { const int a = tmin - P.qpos0; return a <= 0 ? 0 : (a + P.qstride - 1) / P.qstride; };
    int ilo = (j < P.S) ? first_row(j - P.mask_off + 1) : (1 << 30);
    int ilo_max = (j0 + 15 < P.S) ? first_row(j0 + 15 - P.mask_off + 1) : (1 << 30);         // wave-uniform: rows at or above it need no test
    bool any_key = true;                                // KB: the tile has a visible key (block-uniform)
    if constexpr (KB) {
        bool kvis = false;
        if (j < P.S) kvis = ga.k[pi].mask[(size_t)b * ga.k[pi].ldm + j] != 0;
        if (!kvis) ilo = 1 << 30;
        if (__builtin_amdgcn_ballot_w64(!kvis) != 0) ilo_max = 1 << 30;                          // a hidden key in the wave: every row tests
        any_key = __syncthreads_or(kvis);
    }
    const int i_first = first_row(kb * 64 - P.mask_off + 1);                                   // first query row that sees any key of the tile
    const int i_end = min(P.T, i0 + MQT);

    f32x4 acc[MQT / 16];
#pragma unroll
    for (int u = 0; u < MQT / 16; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (i_first < i_end && any_key) {                   // block-uniform: a fully masked tile keeps its zeros
        f32x4 am4[MQT / 16];                            // AM: mask of queries i0 + 16u + 4g + (0..3) against key j
        AAdd am = AAdd{nullptr, 0, 0};
        if constexpr (AM) am = map_add(ga, pi);
        auto load_mask = [&](int h) {
            const float* acol = am.m + (size_t)h * am.hs + (size_t)min(j, P.S - 1) * am.ld;
#pragma unroll
            for (int u = 0; u < MQT / 16; ++u) {
                const int ic = i0 + 16 * u + 4 * g;     // ic % 4 == 0 and ldt % 4 == 0: ic < T implies ic + 3 < ldt
                am4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (j < P.S && ic < P.T) am4[u] = *(const f32x4*)(acol + ic);
            }
        };
        if constexpr (AM && !PH) load_mask(0);
        RowStage<CT, DHP, MQT> qst;
        frag kn[C::NKS];
        float n_lse = 0.f;
        auto stage = [&](int h) {
            const size_t bh = (size_t)b * P.H + h;
            qst.load(P.Q + bh * P.T * C::ROWB, i0, P.T, tid);
            const char* Kh = P.K + bh * P.S * C::ROWB;
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) kn[s] = load_frag<CT, DHP>(Kh, j, P.S, s, g);
            const int i = i0 + (tid & (MQT - 1));
            const bool ok = i < P.T;
            const float l = P.lse[bh * P.T + (ok ? i : 0)];
            n_lse = ok ? -l * LOG2E : 0.f;
        };
        stage(0);
        const bool edge = (i0 < ilo_max) || (i0 + MQT > P.T);
#pragma unroll 1
        for (int h = 0; h < P.H; ++h) {
            __syncthreads();
            qst.store(qimg, tid);
            if (tid < MQT) s_lse[tid] = n_lse;
            frag kf[C::NKS];
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) kf[s] = kn[s];
            __syncthreads();
            if (h + 1 < P.H) stage(h + 1);
            if constexpr (PH) load_mask(h);
#pragma unroll
            for (int u = 0; u < MQT / 16; ++u) {
                f32x4 s_ = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < C::NKS; ++s) s_ = Tr<CT>::mma(read_rowfrag<CT>(qimg, C::STRIDE, 16 * u, s, lane), kf[s], s_);
                if constexpr (AM) s_ += am4[u];
                const f32x4 l4 = *(const f32x4*)(s_lse + 16 * u + 4 * g);
                const int ib = i0 + 16 * u + 4 * g;                 // query row of element r is ib + r
                f32x4 e4 = s_ * LOG2E + l4;
                if (edge) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e4[r] = (ib + r >= ilo && ib + r < P.T) ? e4[r] : -INFINITY;   // exp2(-inf) = 0
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u][r] += fast_exp2(e4[r]);
            }
        }
    }
    if (j < P.S) {
        const float inv = 1.f / (float)P.H;
#pragma unroll
        for (int u = 0; u < MQT / 16; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * u + 4 * g + r;
                if (i0 + row < P.T) Wb[(size_t)row * P.ldw + j] = acc[u][r] * inv;
            }
    }
}

// ---- bpm_attn_maps / _amask / _hmask / _kmask / _kamask: check / fill / choose / launch ---------------------------------------------------
// check: the pointers, geometry and alignment of one problem
int maps_check(const bpm_attn_map_problem& q, int dhp0) {
    if (!q.Q || !q.K || !q.lse || !q.W) return BPM_ERR_ARG;
    if (!geometry_ok(q, dhp0) || q.ldw < q.S) return BPM_ERR_ARG;
    if ((((uintptr_t)q.Q | (uintptr_t)q.K) & 15) != 0 || (((uintptr_t)q.lse | (uintptr_t)q.W) & 3) != 0) return BPM_ERR_ALIGN;
    return 0;
}

// fill: the argument block and the grid; masks: the additive masks (read through their transposes), or nullptr; kmasks:
// the per-key byte masks, or nullptr.  Problem by problem: check, the mask_off rule, the block limit, the mask descriptors.
int maps_fill(MGroupK& gk, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, const bpm_attn_kmask* kmasks, int nprob, long* total) {
    MGroupA& ga = gk.a;
    MGroup& g = ga.g;
    g.nprob = nprob;
    long blk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_map_problem& q = probs[i];
        MProb& p = g.p[i];
        int rc = maps_check(q, probs[0].dhp);
        if (rc) return rc;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.lse = q.lse; p.W = q.W; p.ldw = q.ldw;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        if (!positions(q, p)) return BPM_ERR_ARG;
        p.nqt = (q.T + MQT - 1) / MQT; p.nkt = (q.S + 63) / 64;
        p.blk0 = (int)blk;
        blk += (long)p.nqt * p.nkt * q.B;
        if (blk > (1l << 30)) return BPM_ERR_ARG;
        if (kmasks && (rc = kmask_desc(gk.k[i], kmasks[i], q.S)) != 0) return rc;
        if (masks && (rc = amask_desc(ga.m[i], masks[i], q.T, q.S, true)) != 0) return rc;
    }
    for (int i = masks ? nprob : 0; i < BPM_MAX_GROUP; ++i) ga.m[i] = AAdd{nullptr, 0, 0};
    for (int i = kmasks ? nprob : 0; i < BPM_MAX_GROUP; ++i) gk.k[i] = AMask{nullptr, 0};
    *total = blk;
    return 0;
}

// choose: the per-head instantiation when a mask of the launch has a head stride
bool maps_per_head(const MGroupA& ga, int nprob, bool with_masks) {
    bool per_head = false;
    for (int i = 0; with_masks && i < nprob; ++i) per_head = per_head || ga.m[i].hs != 0;
    return per_head;
}

int maps_launch(int dtype, int dhp, bool with_masks, bool per_head, bool with_kmasks, const MGroupK& gk, long total, void* stream) {
    const MGroupA& ga = gk.a;
    return with_ct(dtype, [&](auto ct) {
        return with_dhp(dhp, [&](auto d) {
            typedef decltype(ct) CT;
            constexpr int D = decltype(d)::value;
            if (with_kmasks) {
                if (per_head) return launch<attn_maps_kernel<WithBytes<CT>, D, true, true>>((unsigned)total, NTHREADS, stream, gk);
                if (with_masks) return launch<attn_maps_kernel<WithBytes<CT>, D, true>>((unsigned)total, NTHREADS, stream, gk);
                return launch<attn_maps_kernel<WithBytes<CT>, D, false>>((unsigned)total, NTHREADS, stream, gk);
            }
            if (per_head) return launch<attn_maps_kernel<CT, D, true, true>>((unsigned)total, NTHREADS, stream, ga);
            if (with_masks) return launch<attn_maps_kernel<CT, D, true>>((unsigned)total, NTHREADS, stream, ga);
            return launch<attn_maps_kernel<CT, D, false>>((unsigned)total, NTHREADS, stream, ga.g);
        });
    });
}

// Head-averaged attention probabilities of finished forward passes (see attn_maps_kernel); masks: the additive masks of
// bpm_attn_maps_amask (read through their transposes), or nullptr; kmasks: the byte masks of bpm_attn_maps_kmask, or nullptr.
int attn_maps_impl(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, bool with_masks,
                   const bpm_attn_kmask* kmasks, bool with_kmasks, int nprob, void* stream) {
    if (!group_ok(probs, nprob)) return BPM_ERR_ARG;
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if ((with_masks && !masks) || (with_kmasks && !kmasks)) return BPM_ERR_ARG;
    MGroupK gk;
    const MGroupA& ga = gk.a;
    long total = 0;
    int rc = maps_fill(gk, probs, masks, kmasks, nprob, &total);
    if (rc) return rc;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double flops = 0, bytes = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_map_problem& q = probs[i];
        const double ts = (double)q.B * q.T * q.S;
        flops += 2.0 * ts * q.H * q.dh;
        bytes += (double)q.B * q.H * ((double)(q.T + q.S) * q.dh * sz + q.T * 4.0) + ts * 4.0;      // Q, K, lse in; W out
        if (with_masks) bytes += 4.0 * q.T * q.S;
    }
    BpmProfScope prof(BPM_K_ATTN_MAPS, (hipStream_t)stream, flops, bytes);
    return maps_launch(dtype, probs[0].dhp, with_masks, maps_per_head(ga, nprob, with_masks), with_kmasks, gk, total, stream);
}


// ---------------------------------------------------------------------------
// per-head attention maps: W[b][h][i][j] = exp(S_h[i][j] - LSE_h[i])  (0 for a hidden pair)
// ---------------------------------------------------------------------------
// The addend attn_maps_kernel sums over the heads, written head by head as fp32 [B, H, T, ldw] (bpm_attn_head_maps and its
// four masked siblings): the same orientation (rows = queries, lane = key), the same fragment order into the MFMA, the same
// -lse * log2(e), visibility tests and fast_exp2, so a value here is bit for bit what that kernel adds for its head.
// There is no head loop to carry: one workgroup owns a (batch element, head, 64-query tile, 64-key tile) of one problem,
// stages the head's 64 Q rows through the LDS image once, holds a wave's 16 K rows as the B operand, and keeps nothing
// across heads -- no accumulators, no second set of K fragments, no loads in flight behind arithmetic (occupancy hides
// them).  The finished 64 x 64 tile goes through LDS (the Q image's bytes, reused behind a barrier; rows HM_LD floats apart:
// the four query groups of a wave land on banks 16 apart) and leaves row-contiguously: a wave writes whole 256-byte row
// segments, lane = key, sixteen rows each -- one store instruction per row segment instead of attn_maps_kernel's four 64-byte
// pieces.  A tile the future rule hides, or whose key bytes are all zero, is skipped block-uniformly and written as zeros
// the same way.  (An all -inf additive tile is not known without reading it: it runs, and comes out as zeros.)
// Only W[b][h][i][0 .. S) is written.
//
// Waves per SIMD each instantiation is compiled for (register budget 512 / waves), bf16 / f32 registers used at head_dim
// 32, 64, 128, 256 by the plain instantiation, and by the one with both masks in brackets:
//   bf16  32 / 40 / 52 / 83 (50 / 52 / 76 / 103)  ->  4 waves      f32  40 / 54 / 83 / 153 (56 / 68 / 103 / 173)  ->  4, 4, 4, 2 waves
// (f32 at 256: 64 K-fragment and 64 staging registers).  No instantiation spills: scratch size 0 in the gfx950 assembly of
// all 32.  LDS per workgroup is the larger of the Q image and the 17 KiB output tile: four workgroups fit a CU up to 35 KiB
// (f32 at 128, bf16 at 256), two at 67 KiB (f32 at 256).
template <typename CT>
constexpr int head_map_waves(int dhp) {
    return sizeof(CT) == 4 && dhp > 128 ? 2 : 4;
}
constexpr int HM_LD = 68;   // floats per row of the LDS tile the store reads

struct HProb {
    const char* Q; const char* K;
    const float* lse;
    float* W; int ldw;
    int B, H, T, S;
    int mask_off, qpos0, qstride;
    int blk0, nqt, nkt;     // block prefix / query tiles / key tiles
    int64_t hs, bs;         // elements between the maps of consecutive heads / samples
};
struct HGroup {
    int nprob;
    HProb p[BPM_MAX_GROUP];
};
// the masked entries: the additive descriptors (m: used with AM only) and the byte masks (k: used with KB only) behind the
// problems, in an argument block of their own, so the unmasked instantiations carry neither
struct HGroupM {
    HGroup g;
    AAdd m[BPM_MAX_GROUP];
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(HGroupM) <= 4096, "kernel arguments are limited to 4 KiB");
BPM_DEV const HGroup& head_group(const HGroup& g) { return g; }
BPM_DEV const HGroup& head_group(const HGroupM& g) { return g.g; }

// CTX: the compute type, or WithBytes<compute type> for the byte mask (KB); AM: an additive image, read through its
// transpose from the head's image (head stride 0: the one image)
template <typename CTX, int DHP, bool AM = false>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(head_map_waves<typename CtOf<CTX>::type>(DHP), head_map_waves<typename CtOf<CTX>::type>(DHP)))) void attn_head_maps_kernel(const std::conditional_t<CtOf<CTX>::bytes || AM, HGroupM, HGroup> ga) {
    typedef typename CtOf<CTX>::type CT;
    constexpr bool KB = CtOf<CTX>::bytes;
    const HGroup& grp = head_group(ga);
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    constexpr int QBYTES = MQT * C::STRIDE + MQT * 4, TBYTES = MQT * HM_LD * 4;
    __shared__ __attribute__((aligned(16))) char smem[QBYTES > TBYTES ? QBYTES : TBYTES];
    char* qimg = smem;
    float* s_lse = (float*)(smem + MQT * C::STRIDE);            // -lse * log2(e) of the tile's query rows
    float* tile = (float*)smem;                                 // the finished tile, once the image has been read

    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const HProb& P = grp.p[pi];
    bid -= P.blk0;
    const int per = P.nkt * P.nqt;
    const int kb = bid % P.nkt, qt = (bid / P.nkt) % P.nqt, bh = bid / per;     // key tiles of a query tile are neighbours
    const int h = bh % P.H, b = bh / P.H;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int j0 = kb * 64 + wave * 16;                 // wave-uniform first key
    const int j = j0 + c;                               // this lane's key
    const int i0 = qt * MQT;                            // first query row of the tile
    float* Wt = P.W + (size_t)b * P.bs + (size_t)h * P.hs + (size_t)i0 * P.ldw + kb * 64;     // the tile's first element

    // query row i (time qpos0 + i*qstride) sees key j iff i >= first_row(j - mask_off + 1)   (attn_maps_kernel's rule)
    auto first_row = [&](int tmin) { const int a = tmin - P.qpos0; return a <= 0 ? 0 : (a + P.qstride - 1) / P.qstride; };
    int ilo = (j < P.S) ? first_row(j - P.mask_off + 1) : (1 << 30);
    int ilo_max = (j0 + 15 < P.S) ? first_row(j0 + 15 - P.mask_off + 1) : (1 << 30);         // wave-uniform: rows at or above it need no test
    bool any_key = true;                                // KB: the tile has a visible key (block-uniform)
    if constexpr (KB) {
        bool kvis = false;
        if (j < P.S) kvis = ga.k[pi].mask[(size_t)b * ga.k[pi].ldm + j] != 0;
        if (!kvis) ilo = 1 << 30;
        if (__builtin_amdgcn_ballot_w64(!kvis) != 0) ilo_max = 1 << 30;                          // a hidden key in the wave: every row tests
        any_key = __syncthreads_or(kvis);
    }
    const int i_first = first_row(kb * 64 - P.mask_off + 1);                                   // first query row that sees any key of the tile
    const int i_end = min(P.T, i0 + MQT);
    const int nrow = i_end - i0, ncol = min(64, P.S - kb * 64);                                // the part of the tile inside [T, S)
    const int r0 = wave * (MQT / 4);                    // the store: this wave's sixteen rows, lane = key

    if (i_first < i_end && any_key) {                   // block-uniform
        f32x4 am4[MQT / 16];                            // AM: mask of queries i0 + 16u + 4g + (0..3) against key j
        if constexpr (AM) {
            const AAdd am = ga.m[pi];
            const float* acol = am.m + (size_t)h * am.hs + (size_t)min(j, P.S - 1) * am.ld;
#pragma unroll
            for (int u = 0; u < MQT / 16; ++u) {
                const int ic = i0 + 16 * u + 4 * g;     // ic % 4 == 0 and ldt % 4 == 0: ic < T implies ic + 3 < ldt
                am4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (j < P.S && ic < P.T) am4[u] = *(const f32x4*)(acol + ic);
            }
        }
        frag kf[C::NKS];
        {
            RowStage<CT, DHP, MQT> qst;
            qst.load(P.Q + (size_t)bh * P.T * C::ROWB, i0, P.T, tid);
            const char* Kh = P.K + (size_t)bh * P.S * C::ROWB;
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) kf[s] = load_frag<CT, DHP>(Kh, j, P.S, s, g);
            const int i = i0 + (tid & (MQT - 1));
            const bool ok = i < P.T;
            const float l = P.lse[(size_t)bh * P.T + (ok ? i : 0)];
            qst.store(qimg, tid);
            if (tid < MQT) s_lse[tid] = ok ? -l * LOG2E : 0.f;
        }
        __syncthreads();
        const bool edge = (i0 < ilo_max) || (i0 + MQT > P.T);
        f32x4 p4[MQT / 16];
#pragma unroll
        for (int u = 0; u < MQT / 16; ++u) {
            f32x4 s_ = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) s_ = Tr<CT>::mma(read_rowfrag<CT>(qimg, C::STRIDE, 16 * u, s, lane), kf[s], s_);
            if constexpr (AM) s_ += am4[u];
            const f32x4 l4 = *(const f32x4*)(s_lse + 16 * u + 4 * g);
            const int ib = i0 + 16 * u + 4 * g;                 // query row of element r is ib + r
            f32x4 e4 = s_ * LOG2E + l4;
            if (edge) {
#pragma unroll
                for (int r = 0; r < 4; ++r) e4[r] = (ib + r >= ilo && ib + r < P.T) ? e4[r] : -INFINITY;   // exp2(-inf) = 0
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) p4[u][r] = fast_exp2(e4[r]);
        }
        __syncthreads();                                // every wave has read the image and the LSE: the tile takes their place
#pragma unroll
        for (int u = 0; u < MQT / 16; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[(16 * u + 4 * g + r) * HM_LD + wave * 16 + c] = p4[u][r];
        __syncthreads();
        if (lane < ncol) {
#pragma unroll 4
            for (int r = r0; r < min(r0 + MQT / 4, nrow); ++r) Wt[(size_t)r * P.ldw + lane] = tile[r * HM_LD + lane];
        }
    } else if (lane < ncol) {                           // a fully hidden tile: zeros, row by row
        for (int r = r0; r < min(r0 + MQT / 4, nrow); ++r) Wt[(size_t)r * P.ldw + lane] = 0.f;
    }
}

// ---- bpm_attn_head_maps / _amask / _hmask / _kmask / _kamask: check / fill / choose / launch -------------------------------
// check: the pointers, geometry, strides and alignment of one problem
int head_maps_check(const bpm_attn_head_map_problem& q, int dhp0) {
    if (!q.Q || !q.K || !q.lse || !q.W) return BPM_ERR_ARG;
    if (!geometry_ok(q, dhp0) || q.ldw < q.S) return BPM_ERR_ARG;
    if (q.head_stride < (int64_t)q.T * q.ldw || q.head_stride > INT64_MAX / q.H || q.batch_stride < (int64_t)q.H * q.head_stride) return BPM_ERR_ARG;
    if (q.batch_stride > INT64_MAX / q.B) return BPM_ERR_ARG;
    if ((((uintptr_t)q.Q | (uintptr_t)q.K) & 15) != 0 || (((uintptr_t)q.lse | (uintptr_t)q.W) & 3) != 0) return BPM_ERR_ALIGN;
    return 0;
}

// fill: the argument block and the grid, as maps_fill; one workgroup per (sample, head, query tile, key tile)
int head_maps_fill(HGroupM& gm, const bpm_attn_head_map_problem* probs, const bpm_attn_hmask* masks, const bpm_attn_kmask* kmasks, int nprob, long* total) {
    HGroup& g = gm.g;
    g.nprob = nprob;
    long blk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_head_map_problem& q = probs[i];
        HProb& p = g.p[i];
        int rc = head_maps_check(q, probs[0].dhp);
        if (rc) return rc;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.lse = q.lse; p.W = q.W; p.ldw = q.ldw;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        p.hs = q.head_stride; p.bs = q.batch_stride;
        if (!positions(q, p)) return BPM_ERR_ARG;
        p.nqt = (q.T + MQT - 1) / MQT; p.nkt = (q.S + 63) / 64;
        p.blk0 = (int)blk;
        const long tiles = (long)p.nqt * p.nkt;
        if (tiles > (1l << 30) || (long)q.B * q.H > (1l << 30) || tiles * q.B * q.H > (1l << 30)) return BPM_ERR_ARG;
        blk += tiles * q.B * q.H;
        if (blk > (1l << 30)) return BPM_ERR_ARG;
        if (kmasks && (rc = kmask_desc(gm.k[i], kmasks[i], q.S)) != 0) return rc;
        if (masks && (rc = amask_desc(gm.m[i], masks[i], q.T, q.S, true)) != 0) return rc;
    }
    for (int i = masks ? nprob : 0; i < BPM_MAX_GROUP; ++i) gm.m[i] = AAdd{nullptr, 0, 0};
    for (int i = kmasks ? nprob : 0; i < BPM_MAX_GROUP; ++i) gm.k[i] = AMask{nullptr, 0};
    *total = blk;
    return 0;
}

// choose / launch: the instantiation is the entry's family (byte mask, additive image) at the compute type and head_dim
int head_maps_launch(int dtype, int dhp, bool with_masks, bool with_kmasks, const HGroupM& gm, long total, void* stream) {
    return with_ct(dtype, [&](auto ct) {
        return with_dhp(dhp, [&](auto d) {
            typedef decltype(ct) CT;
            constexpr int D = decltype(d)::value;
            if (with_kmasks) {
                if (with_masks) return launch<attn_head_maps_kernel<WithBytes<CT>, D, true>>((unsigned)total, NTHREADS, stream, gm);
                return launch<attn_head_maps_kernel<WithBytes<CT>, D, false>>((unsigned)total, NTHREADS, stream, gm);
            }
            if (with_masks) return launch<attn_head_maps_kernel<CT, D, true>>((unsigned)total, NTHREADS, stream, gm);
            return launch<attn_head_maps_kernel<CT, D, false>>((unsigned)total, NTHREADS, stream, gm.g);
        });
    });
}

// Per-head attention probabilities of finished forward passes (see attn_head_maps_kernel); masks / kmasks as attn_maps_impl
int attn_head_maps_impl(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_hmask* masks, bool with_masks,
                        const bpm_attn_kmask* kmasks, bool with_kmasks, int nprob, void* stream) {
    if (!group_ok(probs, nprob)) return BPM_ERR_ARG;
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if ((with_masks && !masks) || (with_kmasks && !kmasks)) return BPM_ERR_ARG;
    HGroupM gm;
    long total = 0;
    int rc = head_maps_fill(gm, probs, masks, kmasks, nprob, &total);
    if (rc) return rc;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double flops = 0, bytes = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_head_map_problem& q = probs[i];
        const double ts = (double)q.B * q.H * q.T * q.S;
        flops += 2.0 * ts * q.dh;
        bytes += (double)q.B * q.H * ((double)(q.T + q.S) * q.dh * sz + q.T * 4.0) + ts * 4.0;      // Q, K, lse in; W out
        if (with_masks) bytes += 4.0 * q.T * q.S * (masks[i].head_strideT != 0 ? q.H : 1);
    }
    BpmProfScope prof(BPM_K_ATTN_MAPS, (hipStream_t)stream, flops, bytes);
    return head_maps_launch(dtype, probs[0].dhp, with_masks, with_kmasks, gm, total, stream);
}

}  // namespace

extern "C" int bpm_attn_maps(int dtype, const bpm_attn_map_problem* probs, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, nullptr, false, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_amask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_amask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, HMasks(masks, nprob).p, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_hmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
// ... with a per-key byte mask (lse from bpm_attn_fwd_kmask), and with both masks (lse from bpm_attn_fwd_kamask)
extern "C" int bpm_attn_maps_kmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_kmask* kmasks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, nullptr, false, kmasks, true, nprob, stream);
}
extern "C" int bpm_attn_maps_kamask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks, int nprob,
                                    void* stream) {
    return attn_maps_impl(dtype, probs, masks, true, kmasks, true, nprob, stream);
}

// ---- the per-head maps: the five entries above, one map per head -----------------------------------------------------------
extern "C" int bpm_attn_head_maps(int dtype, const bpm_attn_head_map_problem* probs, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, nullptr, false, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_amask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_amask* masks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, HMasks(masks, nprob).p, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_hmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_hmask* masks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_kmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_kmask* kmasks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, nullptr, false, kmasks, true, nprob, stream);
}
extern "C" int bpm_attn_head_maps_kamask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks,
                                         int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, masks, true, kmasks, true, nprob, stream);
}

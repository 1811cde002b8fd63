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
// Per-sample images (bpm_attn_maps_bmask / _kbmask): the descriptors are AAddB, in argument blocks of their own behind the
// same MGroup, so the kernels above keep theirs.  The image of (b, h) is loaded inside the head loop (the PH path) whatever
// the head stride is: with one image per sample the heads re-read it from L2.
struct MGroupB {
    MGroup g;
    AAddB m[BPM_MAX_GROUP];
};
struct MGroupKB {
    MGroupB a;
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(MGroupKB) <= 4096, "kernel arguments are limited to 4 KiB");
BPM_DEV const MGroup& map_group(const MGroupB& g) { return g.g; }
BPM_DEV const MGroup& map_group(const MGroupKB& g) { return g.a.g; }
BPM_DEV const AAddB& map_add(const MGroupB& g, int pi) { return g.m[pi]; }
BPM_DEV const AAddB& map_add(const MGroupKB& g, int pi) { return g.a.m[pi]; }
template <typename G> constexpr bool per_sample_group = std::is_same_v<G, MGroupB> || std::is_same_v<G, MGroupKB>;

template <typename CTX, int DHP, bool AM = false, bool PH = false>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(map_waves<typename CtOf<CTX>::type>(DHP, AM), map_waves<typename CtOf<CTX>::type>(DHP, AM)))) void attn_maps_kernel(const std::conditional_t<CtOf<CTX>::bytes, MGroupK, std::conditional_t<AM, MGroupA, MGroup>> ga) {
#include "attn_maps_body.inc"
}
// ... with one image per sample (bpm_attn_maps_bmask / _kbmask), at the occupancy of the per-head instantiation above
template <typename CTX, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(map_waves<typename CtOf<CTX>::type>(DHP, true), map_waves<typename CtOf<CTX>::type>(DHP, true)))) void attn_maps_bmask_kernel(const std::conditional_t<CtOf<CTX>::bytes, MGroupKB, MGroupB> ga) {
    constexpr bool AM = true, PH = true;
#include "attn_maps_body.inc"
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
// GK / HM: MGroupK with bpm_attn_hmask masks, or MGroupKB with bpm_attn_bmask masks (one image per sample).
template <typename GK, typename HM>
int maps_fill(GK& gk, const bpm_attn_map_problem* probs, const HM* masks, const bpm_attn_kmask* kmasks, int nprob, long* total) {
    auto& ga = gk.a;
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
        if (masks && (rc = image_desc(ga.m[i], masks[i], q.H, q.T, q.S, true)) != 0) return rc;
    }
    for (int i = masks ? nprob : 0; i < BPM_MAX_GROUP; ++i) ga.m[i] = {};
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

// the per-sample family: one instantiation per compute type, head_dim and byte-mask switch
bool maps_per_head(const MGroupB&, int, bool) { return true; }
int maps_launch(int dtype, int dhp, bool, bool, bool with_kmasks, const MGroupKB& gk, long total, void* stream) {
    return with_ct(dtype, [&](auto ct) {
        return with_dhp(dhp, [&](auto d) {
            typedef decltype(ct) CT;
            constexpr int D = decltype(d)::value;
            if (with_kmasks) return launch<attn_maps_bmask_kernel<WithBytes<CT>, D>>((unsigned)total, NTHREADS, stream, gk);
            return launch<attn_maps_bmask_kernel<CT, D>>((unsigned)total, NTHREADS, stream, gk.a);
        });
    });
}

// Head-averaged attention probabilities of finished forward passes (see attn_maps_kernel); masks: the additive masks of
// bpm_attn_maps_amask (read through their transposes), or nullptr; kmasks: the byte masks of bpm_attn_maps_kmask, or nullptr.
// GK: MGroupK (masks: bpm_attn_hmask), or MGroupKB (masks: bpm_attn_bmask, one image per sample).
template <typename GK = MGroupK, typename HM = bpm_attn_hmask>
int attn_maps_impl(int dtype, const bpm_attn_map_problem* probs, const HM* masks, bool with_masks,
                   const bpm_attn_kmask* kmasks, bool with_kmasks, int nprob, void* stream) {
    if (!group_ok(probs, nprob)) return BPM_ERR_ARG;
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if ((with_masks && !masks) || (with_kmasks && !kmasks)) return BPM_ERR_ARG;
    GK gk;
    const auto& ga = gk.a;
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
// per-sample images (bpm_attn_head_maps_bmask / _kbmask): HGroupM with AAddB descriptors, an argument block of its own
struct HGroupB {
    HGroup g;
    AAddB m[BPM_MAX_GROUP];
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(HGroupB) <= 4096, "kernel arguments are limited to 4 KiB");
BPM_DEV const HGroup& head_group(const HGroupB& g) { return g.g; }

// CTX: the compute type, or WithBytes<compute type> for the byte mask (KB); AM: an additive image, read through its
// transpose from the head's image (head stride 0: the one image)
template <typename CTX, int DHP, bool AM = false>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(head_map_waves<typename CtOf<CTX>::type>(DHP), head_map_waves<typename CtOf<CTX>::type>(DHP)))) void attn_head_maps_kernel(const std::conditional_t<CtOf<CTX>::bytes || AM, HGroupM, HGroup> ga) {
#include "attn_head_maps_body.inc"
}
// ... with one image per sample (bpm_attn_head_maps_bmask / _kbmask)
template <typename CTX, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(head_map_waves<typename CtOf<CTX>::type>(DHP), head_map_waves<typename CtOf<CTX>::type>(DHP)))) void attn_head_maps_bmask_kernel(const HGroupB ga) {
    constexpr bool AM = true;
#include "attn_head_maps_body.inc"
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
// GM / HM: HGroupM with bpm_attn_hmask masks, or HGroupB with bpm_attn_bmask masks (one image per sample).
template <typename GM, typename HM>
int head_maps_fill(GM& gm, const bpm_attn_head_map_problem* probs, const HM* masks, const bpm_attn_kmask* kmasks, int nprob, long* total) {
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
        if (masks && (rc = image_desc(gm.m[i], masks[i], q.H, q.T, q.S, true)) != 0) return rc;
    }
    for (int i = masks ? nprob : 0; i < BPM_MAX_GROUP; ++i) gm.m[i] = {};
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

int head_maps_launch(int dtype, int dhp, bool, bool with_kmasks, const HGroupB& gm, long total, void* stream) {
    return with_ct(dtype, [&](auto ct) {
        return with_dhp(dhp, [&](auto d) {
            typedef decltype(ct) CT;
            constexpr int D = decltype(d)::value;
            if (with_kmasks) return launch<attn_head_maps_bmask_kernel<WithBytes<CT>, D>>((unsigned)total, NTHREADS, stream, gm);
            return launch<attn_head_maps_bmask_kernel<CT, D>>((unsigned)total, NTHREADS, stream, gm);
        });
    });
}

// Per-head attention probabilities of finished forward passes (see attn_head_maps_kernel); masks / kmasks / the template
// arguments as attn_maps_impl
template <typename GM = HGroupM, typename HM = bpm_attn_hmask>
int attn_head_maps_impl(int dtype, const bpm_attn_head_map_problem* probs, const HM* masks, bool with_masks,
                        const bpm_attn_kmask* kmasks, bool with_kmasks, int nprob, void* stream) {
    if (!group_ok(probs, nprob)) return BPM_ERR_ARG;
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if ((with_masks && !masks) || (with_kmasks && !kmasks)) return BPM_ERR_ARG;
    GM gm;
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
    return attn_maps_impl(dtype, probs, (const bpm_attn_hmask*)nullptr, false, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_amask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_amask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, HMasks(masks, nprob).p, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_hmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
// ... with a per-key byte mask (lse from bpm_attn_fwd_kmask), and with both masks (lse from bpm_attn_fwd_kamask)
extern "C" int bpm_attn_maps_kmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_kmask* kmasks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, (const bpm_attn_hmask*)nullptr, false, kmasks, true, nprob, stream);
}
extern "C" int bpm_attn_maps_kamask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks, int nprob,
                                    void* stream) {
    return attn_maps_impl(dtype, probs, masks, true, kmasks, true, nprob, stream);
}

// ---- the per-head maps: the five entries above, one map per head -----------------------------------------------------------
extern "C" int bpm_attn_head_maps(int dtype, const bpm_attn_head_map_problem* probs, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, (const bpm_attn_hmask*)nullptr, false, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_amask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_amask* masks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, HMasks(masks, nprob).p, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_hmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_hmask* masks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_kmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_kmask* kmasks, int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, (const bpm_attn_hmask*)nullptr, false, kmasks, true, nprob, stream);
}
extern "C" int bpm_attn_head_maps_kamask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks,
                                         int nprob, void* stream) {
    return attn_head_maps_impl(dtype, probs, masks, true, kmasks, true, nprob, stream);
}

// ---- both kinds of maps under one additive image per sample (see bpm_attn_bmask), alone or beside key bytes ----------------
extern "C" int bpm_attn_maps_bmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_bmask* masks, int nprob, void* stream) {
    return attn_maps_impl<MGroupKB>(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_kbmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_bmask* masks, int nprob,
                                    void* stream) {
    return attn_maps_impl<MGroupKB>(dtype, probs, masks, true, kmasks, true, nprob, stream);
}
extern "C" int bpm_attn_head_maps_bmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_bmask* masks, int nprob, void* stream) {
    return attn_head_maps_impl<HGroupB>(dtype, probs, masks, true, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_head_maps_kbmask(int dtype, const bpm_attn_head_map_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_bmask* masks,
                                         int nprob, void* stream) {
    return attn_head_maps_impl<HGroupB>(dtype, probs, masks, true, kmasks, true, nprob, stream);
}

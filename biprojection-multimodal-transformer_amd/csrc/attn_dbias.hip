// Gradient of an additive attention mask (a learned bias) for BPMulT on gfx950: bpm_attn_bwd_dbias[_kmask] and the workspace
// query.
// What it shares with the forward / backward kernels of attention.hip is in attn_common.h.
#include "attn_common.h"

namespace {

// ---------------------------------------------------------------------------
// gradient of the additive mask: dB[img][i][j] = sum over the heads that read image img of dS[b,h,i,j]
// ---------------------------------------------------------------------------
// The dQ block body's first two products without the third: S^T = K Qs^T and dP^T = V dO^T, keys on the register rows, one
// query per lane (the forward orientation: the lane's 4 consecutive keys of a register group are one float4 of its mask
// row, and one float4 of the result).  A workgroup owns a 64-query x 64-key tile of one output image -- a wave 16 of its
// queries -- and loops over a range of the heads that feed the image (every (b, h) for the shared form, every b of head
// h for the per-head form): the head's 64 K / V rows pass through the LDS images (RowStage, loaded one head ahead), the
// lane's Q / dO fragments, lse and delta come straight from global memory.  The dS tile stays in 16 fp32 accumulators per
// lane and is stored once.  A pair the mask_off rule or a -inf entry hides has probability exp2(-inf) = 0 in every head:
// its sum is exactly 0.0f.  Dropout: the hash, element index and site of the dQ pass.
//
// Filling the chip (dbias_choose): with fewer tiles than the chip holds workgroups at once (compute units x the waves per
// SIMD the kernel is compiled for: a workgroup is one wave per SIMD), the head range of a tile is split over `nsplit`
// workgroups; each writes its partial tile to the workspace image [split][img][T][ldp] and attn_dbias_sum_kernel adds the
// splits in index order -- a fixed order of fp32 additions in both kernels, so the result is bit-reproducible.
//
// Waves per SIMD (dbias_waves): the largest occupancy at which no instantiation spills
// (profiles/attn_dbias_resource_usage.txt).  bf16 / f32 registers at head_dim 32, 64, 128, 256 when compiled for the dQ
// pass's occupancies: 96 (+ 84 bytes of scratch at five waves) / 128 (+ 20 at four) / 167 / 244 and 128 (+ 20 at four) /
// 168 / 250 / 256 + 134 -- so one wave fewer than dQ at bf16 32 and 64 and at f32 32.
template <typename CT>
constexpr int dbias_waves(int dhp) {
    const bool bf = sizeof(CT) == 2;
    if (dhp <= 32) return bf ? 4 : 3;
    if (dhp <= 64) return 3;
    if (dhp <= 128) return bf ? 3 : 2;
    return bf ? 2 : 1;
}
constexpr int DB_CUS = 256;          // split until the launch has DB_CUS x dbias_waves workgroups (the MI355X's compute units x residency) ...
constexpr int DB_MIN_TERMS = 4;      // ... but keep at least this many heads per workgroup: below that the partial images cost more than they spread

struct DProb {
    const char* Q; const char* K; const char* V; const char* dO;
    const float* lse; const float* delta;
    const float* m; int ldm; int mhs;       // the additive mask, forward orientation, and its head stride
    float* out; int ldo; int wlim;          // dB (nsplit == 1) or the partial images; columns < wlim of a row may be written
    long ohs, osplit;                       // elements between images / between splits of `out`
    int B, H, T, S;
    int mask_off, qpos0, qstride;
    int per_head;                           // image = head (terms: samples) instead of one image (terms: all B*H heads)
    int nterm, nsplit, chunk;               // heads that feed an image; workgroups that share them; heads per workgroup
    int blk0, nqt, nkt;
    DropCfg drop;
};
struct DGroup {
    const uint64_t* seedp;
    int nprob;
    DProb p[BPM_MAX_GROUP];
};
static_assert(sizeof(DGroup) <= 4096, "kernel arguments are limited to 4 KiB");

// KB (bpm_attn_bwd_dbias_kmask): the per-key byte masks of the forward pass, in an argument block of their own behind
// DGroup (the kernel without KB keeps its arguments); the switch rides in the compute-type argument (WithBytes).  The head's sample decides the bytes: the tile's KT of them are
// fetched one head ahead by the first KT threads (never at j >= S), pass through KT bytes of LDS behind the K / V images as
// 0 / 1 and hide a key before the exponential, as the mask_off rule does: sample b adds exactly nothing at its hidden
// keys.  A head whose sample hides the whole tile is skipped.  The order of the additions does not change.
struct DGroupK {
    DGroup g;
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(DGroupK) <= 4096, "kernel arguments are limited to 4 KiB");

// Waves per SIMD with KB: the staging costs registers; one wave fewer where the kernel would spill at dbias_waves (bf16 at
// head_dim 32 / 128 / 256: 12 / 76 / 12 bytes per lane, f32 at 64: 52).  dbias_choose keeps the bf16 target of the kernel
// without KB: the workspace query does not know of the byte masks, and a launch split a little further is still correct.
template <typename CT>
constexpr int dbias_waves_kb(int dhp) {
    const bool bf = sizeof(CT) == 2;
    const bool lower = bf ? (dhp <= 32 || dhp == 128 || dhp == 256) : (dhp == 64);
    return dbias_waves<CT>(dhp) - (lower ? 1 : 0);
}

// PS (bpm_attn_bwd_dbias_bmask): per-sample masks and the per-sample result forms.  DProb plus the sample stride of the
// mask, the map (image, term) -> head that replaces per_head, and the second stride of the result -- in an argument
// block of its own (the byte masks ride in it; KB stays the switch), so the kernels above keep their arguments and code:
//   result    images     terms of an image      head b*H + h of (img, t)      imul, tmul     image img is written at
//   [T,S]     1          the B*H heads          t                             0, 1           0
//   [H,T,S]   H          the B samples          t*H + img                     1, H           img*ohs
//   [B,1,T,S] B          the H heads            img*H + t                     H, 1           img*obs
//   [B,H,T,S] B*H        1                      img                           1, 0           (img / H)*obs + (img % H)*ohs
// The terms of an image are added in ascending t, as in the kernel without PS: at batch strides 0 the same bits.
struct DProbB : DProb {
    int mbs;                                // elements between the mask images of consecutive samples
    int imul, tmul;                         // head of (img, t) = img * imul + t * tmul
    int odiv; long obs;                     // image img at out + (img / odiv) * obs + (img % odiv) * ohs
};
struct DGroupB {
    const uint64_t* seedp;
    int nprob;
    DProbB p[BPM_MAX_GROUP];
    AMask k[BPM_MAX_GROUP];
};
static_assert(sizeof(DGroupB) <= 4096, "kernel arguments are limited to 4 KiB");

BPM_DEV const DGroup& dbias_group(const DGroup& g) { return g; }
BPM_DEV const DGroup& dbias_group(const DGroupK& g) { return g.g; }
BPM_DEV const DGroupB& dbias_group(const DGroupB& g) { return g; }
template <typename CTX>
constexpr int dbias_waves_x(int dhp) {
    return CtOf<CTX>::bytes ? dbias_waves_kb<typename CtOf<CTX>::type>(dhp) : dbias_waves<typename CtOf<CTX>::type>(dhp);
}

template <typename CTX, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(dbias_waves_x<CTX>(DHP), dbias_waves_x<CTX>(DHP)))) void attn_dbias_kernel(const std::conditional_t<CtOf<CTX>::bytes, DGroupK, DGroup> ga) {
#include "attn_dbias_body.inc"
}
// ... with per-sample masks and results (bpm_attn_bwd_dbias_bmask), at the occupancy of the sibling above
template <typename CTX, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(dbias_waves_x<CTX>(DHP), dbias_waves_x<CTX>(DHP)))) void attn_dbias_bmask_kernel(const DGroupB ga) {
#include "attn_dbias_body.inc"
}

// dB = the partial images of a split launch, added in split order.  One thread per 4 consecutive keys of a row.
struct DSumProb {
    const float* part; int ldp; long phs, psplit;
    float* dB; int lddb; long ohs;
    int nimg, T, S, nsplit;
    int c4;                 // float4 groups per row: (S + 3) / 4
    unsigned blk0;
};
struct DSumGroup {
    int nprob;
    DSumProb p[BPM_MAX_GROUP];
};
static_assert(sizeof(DSumGroup) <= 4096, "kernel arguments are limited to 4 KiB");

// ... and into a result with a sample stride (DProbB's rule for where image img goes)
struct DSumProbB : DSumProb { int odiv; long obs; };
struct DSumGroupB {
    int nprob;
    DSumProbB p[BPM_MAX_GROUP];
};
static_assert(sizeof(DSumGroupB) <= 4096, "kernel arguments are limited to 4 KiB");

template <typename G>
BPM_DEV void attn_dbias_sum_body(const G& grp) {
    unsigned bid = blockIdx.x;
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const auto& P = grp.p[pi];
    bid -= P.blk0;
    const size_t idx = (size_t)bid * NTHREADS + threadIdx.x;
    const size_t per_img = (size_t)P.T * P.c4;
    if (idx >= per_img * P.nimg) return;
    const int img = (int)(idx / per_img);
    const size_t rem = idx - (size_t)img * per_img;
    const int i = (int)(rem / P.c4), j = 4 * (int)(rem % P.c4);
    const float* src = P.part + (size_t)img * P.phs + (size_t)i * P.ldp + j;      // ldp = 4 c4: whole groups
    f32x4 v = *(const f32x4*)src;
#pragma unroll 1
    for (int s = 1; s < P.nsplit; ++s) v += *(const f32x4*)(src + (size_t)s * P.psplit);
    float* dst;
    if constexpr (std::is_same_v<G, DSumGroupB>) dst = P.dB + (size_t)(img / P.odiv) * P.obs + (size_t)(img % P.odiv) * P.ohs + (size_t)i * P.lddb + j;
    else dst = P.dB + (size_t)img * P.ohs + (size_t)i * P.lddb + j;
    if (j + 4 <= P.S) *(f32x4*)dst = v;
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j + r < P.S) dst[r] = v[r];
    }
}
__global__ __launch_bounds__(NTHREADS) void attn_dbias_sum_kernel(const DSumGroup grp) { attn_dbias_sum_body(grp); }
__global__ __launch_bounds__(NTHREADS) void attn_dbias_sum_bmask_kernel(const DSumGroupB grp) { attn_dbias_sum_body(grp); }

// ---- bpm_attn_bwd_dbias: check / choose / fill / launch -----------------------------------------------------------------
// check: everything about the problems and the outputs that can be refused on the host; nothing is dereferenced
int dbias_check(const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    if (!group_ok(probs, nprob) || !outs) return BPM_ERR_ARG;
    if (with_dhp(probs[0].dhp, [](auto) { return 0; }) != 0) return BPM_ERR_ARG;      // here up front: the workspace query chooses by it
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const bpm_attn_dbias& o = outs[i];
        if (!geometry_ok(q, probs[0].dhp)) return BPM_ERR_ARG;
        if (q.dS || q.Pd) return BPM_ERR_ARG;
        if (!o.dB || o.lddb < q.S || (o.lddb & 3) || ((uintptr_t)o.dB & 15)) return BPM_ERR_ARG;
        if (o.head_stride != 0 && (o.head_stride < (int64_t)q.T * o.lddb || (o.head_stride & 3))) return BPM_ERR_ARG;
    }
    return 0;
}

// choose: how many workgroups share the heads of one tile (1: no split, the tile goes straight to dB).  The launch's
// tiles are counted over all problems; the head range is split until the launch has DB_CUS workgroups, while a workgroup
// keeps at least DB_MIN_TERMS heads.  The target is DB_CUS x the bf16 kernel's waves per SIMD at this head_dim (the
// workspace query does not know the compute type; the f32 kernels hold fewer workgroups at once and are merely split a
// little further than they need).  Measured at B 8, H 12 x 64, T = S = 512: a target of DB_CUS
// alone (4 splits, 256 workgroups of 24 heads) took 67 us against the per-head form's 36.  Returns the workspace the
// splits need, in bytes (16-byte granules).
struct DChoice { int nimg, nterm, nsplit, chunk, ldp; size_t ws_off; };
// (dbias_split: the choice itself, from the images and terms the result's form implies -- ch[i].nimg / nterm are set)
size_t dbias_split(DChoice* ch, const bpm_attn_problem* probs, int nprob) {
    long tiles = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        tiles += (long)ch[i].nimg * ((q.T + 63) / 64) * ((q.S + KT - 1) / KT);
    }
    const long target = (long)DB_CUS * dbias_waves<bf16_t>(probs[0].dhp);
    const long want = tiles >= target ? 1 : (target + tiles - 1) / tiles;
    size_t bytes = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        DChoice& c = ch[i];
        long ns = (c.nterm + DB_MIN_TERMS - 1) / DB_MIN_TERMS;
        if (ns > want) ns = want;
        c.chunk = (int)((c.nterm + ns - 1) / ns);
        c.nsplit = (c.nterm + c.chunk - 1) / c.chunk;           // no empty split: nsplit <= ns, and 1 only when ns is
        c.ldp = (q.S + 3) / 4 * 4;
        c.ws_off = bytes;
        if (ns > 1) bytes += (size_t)ns * c.nimg * q.T * c.ldp * sizeof(float);      // by ns: monotone in the number of heads
    }
    return bytes;
}
size_t dbias_choose(DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        ch[i].nimg = outs[i].head_stride != 0 ? q.H : 1;
        ch[i].nterm = outs[i].head_stride != 0 ? q.B : q.B * q.H;
    }
    return dbias_split(ch, probs, nprob);
}

// fill: the two argument blocks (the mask descriptors are checked here, by the rule of the other *_amask entries; the
// byte masks, when there are any, by the rule of the *_kmask entries)
int dbias_fill(DGroupK& gk, DSumGroup& sg, const DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_hmask* masks,
               const bpm_attn_kmask* kmasks, const bpm_attn_dbias* outs, int nprob, uint64_t seed, void* ws, long* total, long* sum_blocks) {
    DGroup& g = gk.g;
    g.nprob = nprob;
    g.seedp = bpm_seed_ptr(seed);
    sg.nprob = 0;
    long blk = 0, sblk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const DChoice& c = ch[i];
        DProb& p = g.p[i];
        if (!q.Q || !q.K || !q.V || !q.dO || !q.lse || !q.delta) return BPM_ERR_ARG;
        if (((uintptr_t)q.Q | (uintptr_t)q.K | (uintptr_t)q.V | (uintptr_t)q.dO) & 15) return BPM_ERR_ALIGN;
        AAdd a;
        int rc = amask_desc(a, masks[i], q.T, q.S, false);
        if (rc) return rc;
        gk.k[i] = AMask{nullptr, 0};
        if (kmasks && (rc = kmask_desc(gk.k[i], kmasks[i], q.S)) != 0) return rc;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.V = (const char*)q.V; p.dO = (const char*)q.dO;
        p.lse = q.lse; p.delta = q.delta;
        p.m = a.m; p.ldm = a.ld; p.mhs = a.hs;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        if (!positions(q, p)) return BPM_ERR_ARG;
        p.per_head = outs[i].head_stride != 0;
        p.nterm = c.nterm; p.nsplit = c.nsplit; p.chunk = c.chunk;
        p.drop = bpm_make_drop(q.drop_p, seed, q.drop_site);
        p.nqt = (q.T + 63) / 64; p.nkt = (q.S + KT - 1) / KT;
        p.blk0 = (int)blk;
        blk += (long)c.nimg * c.nsplit * p.nqt * p.nkt;
        if (blk > (1l << 30)) return BPM_ERR_ARG;
        if (c.nsplit == 1) {
            p.out = outs[i].dB; p.ldo = outs[i].lddb; p.wlim = q.S; p.ohs = (long)outs[i].head_stride; p.osplit = 0;
        } else {
            p.out = (float*)((char*)ws + c.ws_off); p.ldo = c.ldp; p.wlim = c.ldp;
            p.ohs = (long)q.T * c.ldp; p.osplit = (long)c.nimg * q.T * c.ldp;
            DSumProb& s = sg.p[sg.nprob++];
            s.part = p.out; s.ldp = c.ldp; s.phs = p.ohs; s.psplit = p.osplit;
            s.dB = outs[i].dB; s.lddb = outs[i].lddb; s.ohs = (long)outs[i].head_stride;
            s.nimg = c.nimg; s.T = q.T; s.S = q.S; s.nsplit = c.nsplit; s.c4 = c.ldp / 4;
            s.blk0 = (unsigned)sblk;
            sblk += ((long)c.nimg * q.T * s.c4 + NTHREADS - 1) / NTHREADS;
        }
    }
    for (int i = nprob; i < BPM_MAX_GROUP; ++i) gk.k[i] = AMask{nullptr, 0};
    *total = blk; *sum_blocks = sblk;
    return 0;
}

template <typename CT>
int dbias_launch(int dhp, bool with_kmasks, const DGroupK& gk, long total, const DSumGroup& sg, long sum_blocks, void* stream) {
    const int rc = with_dhp(dhp, [&](auto d) {
        if (with_kmasks) return launch<attn_dbias_kernel<WithBytes<CT>, decltype(d)::value>>((unsigned)total, NTHREADS, stream, gk);
        return launch<attn_dbias_kernel<CT, decltype(d)::value>>((unsigned)total, NTHREADS, stream, gk.g);
    });
    if (rc || sum_blocks <= 0) return rc;
    return launch<attn_dbias_sum_kernel>((unsigned)sum_blocks, NTHREADS, stream, sg);
}

}  // namespace

extern "C" size_t bpm_attn_bwd_dbias_ws_bytes(const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    DChoice ch[BPM_MAX_GROUP];
    if (dbias_check(probs, outs, nprob)) return 0;
    return dbias_choose(ch, probs, outs, nprob);
}

// The gradient of an additive mask (a learned attention bias): see bpm_attn_dbias in include/bpmult_hip.h.  kmasks: the
// per-key byte masks of a forward pass through bpm_attn_fwd_kamask, or NULL (bpm_attn_bwd_dbias).
extern "C" int bpm_attn_bwd_dbias_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, const bpm_attn_kmask* kmasks,
                                        const bpm_attn_dbias* outs, int nprob, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if (!masks) return BPM_ERR_ARG;
    int rc = dbias_check(probs, outs, nprob);
    if (rc) return rc;
    DChoice ch[BPM_MAX_GROUP];
    const size_t need = dbias_choose(ch, probs, outs, nprob);
    if (need > 0 && (!ws || ws_bytes < need || ((uintptr_t)ws & 15))) return BPM_ERR_ARG;
    DGroupK g;
    DSumGroup sg;
    long total = 0, sum_blocks = 0;
    rc = dbias_fill(g, sg, ch, probs, masks, kmasks, outs, nprob, seed, ws, &total, &sum_blocks);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double bytes = 0;                                            // Q, K, V, dO, lse, delta in; the mask in, dB out (partials: overhead)
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        bytes += (double)q.B * q.H * ((2.0 * q.T + 2.0 * q.S) * q.dh * sz + 2.0 * q.T * 4) + 4.0 * q.T * q.S * ch[i].nimg * 2;
    }
    BpmProfScope prof(BPM_K_ATTN_BWD_DBIAS, s, 4.0 * useful_pair_flops(probs, nprob), bytes);      // S and dP: two products
    return with_ct(dtype, [&](auto ct) { return dbias_launch<decltype(ct)>(probs[0].dhp, kmasks != nullptr, g, total, sg, sum_blocks, stream); });
}
extern "C" int bpm_attn_bwd_dbias(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, const bpm_attn_dbias* outs,
                                  int nprob, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    return bpm_attn_bwd_dbias_kmask(dtype, probs, masks, nullptr, outs, nprob, seed, ws, ws_bytes, stream);
}

// ---- bpm_attn_bwd_dbias_bmask: the same four steps with per-sample masks and the four result forms ----------------------------
namespace {

int dbias_b_check(const bpm_attn_problem* probs, const bpm_attn_dbias_b* outs, int nprob) {
    if (!group_ok(probs, nprob) || !outs) return BPM_ERR_ARG;
    if (with_dhp(probs[0].dhp, [](auto) { return 0; }) != 0) return BPM_ERR_ARG;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const bpm_attn_dbias_b& o = outs[i];
        if (!geometry_ok(q, probs[0].dhp)) return BPM_ERR_ARG;
        if (q.dS || q.Pd) return BPM_ERR_ARG;
        if (!o.dB || o.lddb < q.S || (o.lddb & 3) || ((uintptr_t)o.dB & 15)) return BPM_ERR_ARG;
        if (o.head_stride != 0 && (o.head_stride < (int64_t)q.T * o.lddb || (o.head_stride & 3))) return BPM_ERR_ARG;
        const int64_t sample = o.head_stride != 0 ? (int64_t)q.H * o.head_stride : (int64_t)q.T * o.lddb;
        if (o.batch_stride != 0 && (o.batch_stride < sample || (o.batch_stride & 3) || o.batch_stride > 0x7fffffff)) return BPM_ERR_ARG;
    }
    return 0;
}

// choose: the images and terms of each result form (the table at DProbB), then the split of bpm_attn_bwd_dbias
size_t dbias_b_choose(DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_dbias_b* outs, int nprob) {
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const bool ph = outs[i].head_stride != 0, ps = outs[i].batch_stride != 0;
        ch[i].nimg = (ph ? q.H : 1) * (ps ? q.B : 1);
        ch[i].nterm = (ph ? 1 : q.H) * (ps ? 1 : q.B);
    }
    return dbias_split(ch, probs, nprob);
}

int dbias_b_fill(DGroupB& g, DSumGroupB& sg, const DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_bmask* masks,
                 const bpm_attn_kmask* kmasks, const bpm_attn_dbias_b* outs, int nprob, uint64_t seed, void* ws, long* total, long* sum_blocks) {
    g.nprob = nprob;
    g.seedp = bpm_seed_ptr(seed);
    sg.nprob = 0;
    long blk = 0, sblk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const bpm_attn_dbias_b& o = outs[i];
        const DChoice& c = ch[i];
        DProbB& p = g.p[i];
        if (!q.Q || !q.K || !q.V || !q.dO || !q.lse || !q.delta) return BPM_ERR_ARG;
        if (((uintptr_t)q.Q | (uintptr_t)q.K | (uintptr_t)q.V | (uintptr_t)q.dO) & 15) return BPM_ERR_ALIGN;
        AAddB a;
        int rc = bmask_desc(a, masks[i], q.H, q.T, q.S, false);
        if (rc) return rc;
        g.k[i] = AMask{nullptr, 0};
        if (kmasks && (rc = kmask_desc(g.k[i], kmasks[i], q.S)) != 0) return rc;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.V = (const char*)q.V; p.dO = (const char*)q.dO;
        p.lse = q.lse; p.delta = q.delta;
        p.m = a.m; p.ldm = a.ld; p.mhs = a.hs; p.mbs = a.bs;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        if (!positions(q, p)) return BPM_ERR_ARG;
        const bool ph = o.head_stride != 0, ps = o.batch_stride != 0;
        p.per_head = ph;
        p.imul = ps ? (ph ? 1 : q.H) : (ph ? 1 : 0);
        p.tmul = ps ? (ph ? 0 : 1) : (ph ? q.H : 1);
        // where image img of the RESULT goes; the partial images of a split are dense, one after the other
        const int odiv = ps && ph ? q.H : 1;
        const long obs = ps ? (long)o.batch_stride : (long)o.head_stride;
        p.nterm = c.nterm; p.nsplit = c.nsplit; p.chunk = c.chunk;
        p.drop = bpm_make_drop(q.drop_p, seed, q.drop_site);
        p.nqt = (q.T + 63) / 64; p.nkt = (q.S + KT - 1) / KT;
        p.blk0 = (int)blk;
        blk += (long)c.nimg * c.nsplit * p.nqt * p.nkt;
        if (blk > (1l << 30)) return BPM_ERR_ARG;
        if (c.nsplit == 1) {
            p.out = o.dB; p.ldo = o.lddb; p.wlim = q.S; p.osplit = 0;
            p.odiv = odiv; p.obs = obs; p.ohs = (long)o.head_stride;
        } else {
            p.out = (float*)((char*)ws + c.ws_off); p.ldo = c.ldp; p.wlim = c.ldp;
            p.odiv = 1; p.obs = (long)q.T * c.ldp; p.ohs = 0; p.osplit = (long)c.nimg * q.T * c.ldp;
            DSumProbB& s = sg.p[sg.nprob++];
            s.part = p.out; s.ldp = c.ldp; s.phs = p.obs; s.psplit = p.osplit;
            s.dB = o.dB; s.lddb = o.lddb; s.ohs = (long)o.head_stride; s.odiv = odiv; s.obs = obs;
            s.nimg = c.nimg; s.T = q.T; s.S = q.S; s.nsplit = c.nsplit; s.c4 = c.ldp / 4;
            s.blk0 = (unsigned)sblk;
            sblk += ((long)c.nimg * q.T * s.c4 + NTHREADS - 1) / NTHREADS;
        }
    }
    for (int i = nprob; i < BPM_MAX_GROUP; ++i) g.k[i] = AMask{nullptr, 0};
    *total = blk; *sum_blocks = sblk;
    return 0;
}

template <typename CT>
int dbias_b_launch(int dhp, bool with_kmasks, const DGroupB& g, long total, const DSumGroupB& sg, long sum_blocks, void* stream) {
    const int rc = with_dhp(dhp, [&](auto d) {
        if (with_kmasks) return launch<attn_dbias_bmask_kernel<WithBytes<CT>, decltype(d)::value>>((unsigned)total, NTHREADS, stream, g);
        return launch<attn_dbias_bmask_kernel<CT, decltype(d)::value>>((unsigned)total, NTHREADS, stream, g);
    });
    if (rc || sum_blocks <= 0) return rc;
    return launch<attn_dbias_sum_bmask_kernel>((unsigned)sum_blocks, NTHREADS, stream, sg);
}

}  // namespace

extern "C" size_t bpm_attn_bwd_dbias_bmask_ws_bytes(const bpm_attn_problem* probs, const bpm_attn_dbias_b* outs, int nprob) {
    DChoice ch[BPM_MAX_GROUP];
    if (dbias_b_check(probs, outs, nprob)) return 0;
    return dbias_b_choose(ch, probs, outs, nprob);
}

// The bias gradient under per-sample masks, in any of the four result forms: see bpm_attn_dbias_b in include/bpmult_hip.h.
extern "C" int bpm_attn_bwd_dbias_bmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_bmask* masks, const bpm_attn_kmask* kmasks,
                                        const bpm_attn_dbias_b* outs, int nprob, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if (!masks) return BPM_ERR_ARG;
    int rc = dbias_b_check(probs, outs, nprob);
    if (rc) return rc;
    DChoice ch[BPM_MAX_GROUP];
    const size_t need = dbias_b_choose(ch, probs, outs, nprob);
    if (need > 0 && (!ws || ws_bytes < need || ((uintptr_t)ws & 15))) return BPM_ERR_ARG;
    DGroupB g;
    DSumGroupB sg;
    long total = 0, sum_blocks = 0;
    rc = dbias_b_fill(g, sg, ch, probs, masks, kmasks, outs, nprob, seed, ws, &total, &sum_blocks);
    if (rc) return rc;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double bytes = 0;                                            // as bpm_attn_bwd_dbias: every image of the mask in, every image of dB out
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const double mimg = (double)(masks[i].head_stride ? q.H : 1) * (masks[i].batch_stride ? q.B : 1);
        bytes += (double)q.B * q.H * ((2.0 * q.T + 2.0 * q.S) * q.dh * sz + 2.0 * q.T * 4) + 4.0 * q.T * q.S * (mimg + ch[i].nimg);
    }
    BpmProfScope prof(BPM_K_ATTN_BWD_DBIAS, (hipStream_t)stream, 4.0 * useful_pair_flops(probs, nprob), bytes);
    return with_ct(dtype, [&](auto ct) { return dbias_b_launch<decltype(ct)>(probs[0].dhp, kmasks != nullptr, g, total, sg, sum_blocks, stream); });
}

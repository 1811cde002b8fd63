// What more than one family of attention kernels uses (attention.hip: forward / dQ / dK,dV with and without masks;
// attn_maps.hip: head-averaged and per-head maps; attn_dbias.hip: the gradient of an additive mask): tile constants and occupancies,
// the kernel-argument structs, the LDS staging and store helpers, and the shared pieces of the ONE shape of an entry
// point -- check, fill, choose, launch (launch / with_ct come from bpm_launch.h; with_dhp is here).
// Everything sits in the unnamed namespace, as the kernels of those files do: their symbols carry it.
#pragma once
#include <type_traits>

#include "bpm_common.h"
#include "bpm_launch.h"
#include "bpm_prof.h"
#include "../../include/bpmult_hip.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int KT = 64;      // keys per tile (forward / dQ)
constexpr int BPM_ATTN_W128 = 2;    // waves per SIMD at head_dim 128 (unified 256-register budget: no AGPR copies)
constexpr int BPM_ATTN_WF = 5;      // waves per SIMD of the forward kernel at head_dim <= 32 (90 VGPRs; dQ / dKdV spill at 5)
constexpr int BPM_ATTN_SETPRIO = 1;
constexpr int BPM_ATTN_QT = 64;
constexpr int BPM_ATTN_DKV_W32 = 4;
constexpr int BPM_ATTN_DKV_W64 = 3;
constexpr int BPM_ATTN_DQ_W32 = 5;
constexpr int BPM_ATTN_DQ_W128 = 3;
constexpr int BPM_ATTN_DQ_W64 = 4;
constexpr int QT = BPM_ATTN_QT;      // queries per tile (dK/dV): a multiple of 32
// head_dim 256 tiles: the dQ pass stages 32 keys per tile (K / V staging registers 32 instead of 64 in bf16: 228
// registers, 2 waves per SIMD without spills); the f32 dK / dV pass stages 32 queries per tile (64 keys spill even at
// one wave: 128 registers of K / V fragments, 128 of dK / dV accumulators and 128 of Q / dO staging).
constexpr int BPM_ATTN_KT256_DQ = 32;
constexpr int BPM_ATTN_QT256_F32 = 32;

// Waves per SIMD each kernel is compiled for (register budget 512 / waves), per kernel (0 forward, 1 dQ, 2 dK/dV),
// compute type and padded head_dim: the largest occupancy at which the kernel does not spill inside its tile loop.
// Measured on MI355X (tools/attn_lab.py, six encoders, B*H = 96 heads each, T = S = 512, masked), bf16: dQ at head_dim 64
// 110 us at 4 waves (12 registers spilled) -> 98 at 3.  Both backward kernels now compute one k-step of their second
// product at a time (dQ: 112 registers at head_dim 64, 89 at 25, 166 at 128; dK/dV: 154 / 114 / 222), which fits one more
// wave per SIMD without spills.  The f32 (parity-mode) kernels need
// one wave fewer.  Head_dim 256 (bf16 / f32): forward 2 / 1 (244 registers in bf16; the f32 K / V images take 130 KiB of
// LDS, one workgroup per CU anyway), dQ 2 / 1, dK / dV 1 / 1 (bf16: 256 accumulator + fragment registers spill at 2).
template <typename CT>
constexpr int attn_waves(int kernel, int dhp) {
    const bool bf = sizeof(CT) == 2;
    if (dhp <= 32) return kernel == 0 ? (bf ? BPM_ATTN_WF : 4) : (kernel == 2 ? (bf ? BPM_ATTN_DKV_W32 : 3) : (bf ? BPM_ATTN_DQ_W32 : 4));
    if (dhp <= 64) return kernel == 0 ? (bf ? 4 : 3) : kernel == 1 ? (bf ? BPM_ATTN_DQ_W64 : 3) : (bf ? BPM_ATTN_DKV_W64 : 2);
    if (dhp <= 128) return kernel == 0 ? (bf ? 3 : 2) : (kernel == 1 && bf ? BPM_ATTN_DQ_W128 : BPM_ATTN_W128);
    return kernel == 2 || !bf ? 1 : 2;
}
constexpr float LOG2E = 1.4426950408889634f;

struct AProb {
    const char* Q; const char* K; const char* V;
    char* O; int ldo;
    float* lse;
    const char* dO;
    float* delta;
    char* dQ; int lddq;
    char* dK; int lddk;
    char* dV; int lddv;
    int B, H, T, S, dh;
    int mask_off;
    int qpos0, qstride;   // query row i sits at time qpos0 + i*qstride (mask rule only)
    float dq_scale;
    DropCfg drop;
    char* dS; char* Pd;       // dQ pass, optional: dS and the dropped probabilities, element (b, h, i, j) at b xs_b + h xs_h + i xs_q + j
    int xs_b, xs_h, xs_q;
    int blk0, nblk;     // block prefix / blocks per (b,h)
    int pair;           // workgroups take two blocks (b, nblk - 1 - b) instead of one
};
struct AGroup {
    const uint64_t* seedp;     // dropout seed read at execution time (BPM_SEED_INDIRECT), or nullptr
    int nprob;
    AProb p[BPM_MAX_GROUP];
};

// Per-key padding mask of the *_kmask entries (HF's attention_mask): bytes [B, ldm], key j of sample b is visible iff
// mask[b * ldm + j] != 0, ANDed with the mask_off rule.  A second argument block beside AGroup, so the unmasked kernels
// keep their argument layout (and their code: the block bodies of attention.hip take the mask as a compile-time switch).
struct AMask { const uint8_t* mask; int ldm; };
struct NoMask {};           // the mask argument of the block bodies when there is none

// Additive mask of the *_amask entries (the reference's attn_mask argument, multihead_attention.py:113-115): fp32 [T, ldm],
// added to the score of (query i, key j) in every head of the problem; -inf hides the pair.  The forward and dQ kernels
// hold one query per lane and 4 consecutive keys per register group: they read `mask` rows as float4.  The dK / dV and
// maps kernels hold one key per lane and 4 consecutive queries per register group: they read the TRANSPOSE [S, ldt] the
// caller supplies, again as float4 (reading `mask` down a column would be 16 scalar loads per lane and tile).  One
// descriptor per kernel: m / ld are (mask, ldm) or (maskT, ldt).  A third argument block beside AGroup / AGroupK: without
// AM none of this is compiled.  hs: elements between the images of consecutive heads (head h of every sample reads
// m + h * hs); 0: one image for all heads.
struct AAdd { const float* m; int ld; int hs; };

// Both at once (the *_kamask entries: a key_padding_mask beside an attn_mask / attn_bias): pair (b, h, i, j) is visible iff
// the mask_off rule, the byte k.mask[b * k.ldm + j] != 0 and a.m[h * a.hs + i * a.ld + j] > -inf all say so.  The block
// bodies compile their byte-mask part for AMask and AKAdd and their additive part for AAdd and AKAdd; the two parts do not
// know of each other.  byte_of / add_of: the part of a descriptor a body reads (a reference to the descriptor itself for
// the two single types, so their instantiations see the same value they always did).
struct AKAdd { AMask k; AAdd a; };

// Per-sample additive images (the *_bmask / *_kbmask entries: torch's 3-D attn_mask [B*H, T, S], a time-distance bias): AAdd
// plus bs, the elements between the images of consecutive samples -- (sample b, head h) reads m + b * bs + h * hs; the four
// combinations of zero and non-zero strides are the images [T, S], [H, T, S], [B, 1, T, S] and [B, H, T, S].  A descriptor
// type of its own with its own instantiations: the kernels that take AAdd keep their arguments and their code.
struct AAddB { const float* m; int ld; int hs; int bs; };
struct AKAddB { AMask k; AAddB a; };
template <typename M> constexpr bool has_bytes = std::is_same_v<M, AMask> || std::is_same_v<M, AKAdd> || std::is_same_v<M, AKAddB>;
template <typename M> constexpr bool has_add = std::is_same_v<M, AAdd> || std::is_same_v<M, AKAdd> || std::is_same_v<M, AAddB> || std::is_same_v<M, AKAddB>;
BPM_DEV const AMask& byte_of(const AMask& m) { return m; }
BPM_DEV const AMask& byte_of(const AKAdd& m) { return m.k; }
BPM_DEV const AMask& byte_of(const AKAddB& m) { return m.k; }
BPM_DEV const AAdd& add_of(const AAdd& m) { return m; }
BPM_DEV const AAdd& add_of(const AKAdd& m) { return m.a; }
BPM_DEV const AAddB& add_of(const AAddB& m) { return m; }
BPM_DEV const AAddB& add_of(const AKAddB& m) { return m.a; }
// the image (sample b, head h) reads: its first element (offsets in 64 bits)
BPM_DEV const float* image_of(const AAdd& a, int, int h) { return a.m + (size_t)h * a.hs; }
BPM_DEV const float* image_of(const AAddB& a, int b, int h) { return a.m + (size_t)b * a.bs + (size_t)h * a.hs; }

// The byte-mask switch of the maps and bias-gradient kernels (attn_maps.hip, attn_dbias.hip): it rides in the compute-type
// argument -- attn_maps_kernel<WithBytes<bf16_t>, 64, ...> -- so the instantiations without it keep their template
// arguments, which is what launch records and profiles spell them by.
template <typename T> struct WithBytes {};
template <typename T> struct CtOf { typedef T type; static constexpr bool bytes = false; };
template <typename T> struct CtOf<WithBytes<T>> { typedef T type; static constexpr bool bytes = true; };

template <typename CT, int DHP> struct Cfg {
    static constexpr int SZ = sizeof(CT);
    static constexpr int NKS = DHP / Tr<CT>::KSTEP;        // k-steps over head_dim
    static constexpr int ND = DHP / 16;                     // 16-wide head_dim tiles
    static constexpr int ROWB = DHP * SZ;                   // bytes per head row
    static constexpr int STRIDE = ROWB + Tr<CT>::TR_PAD_B;  // LDS image row stride
    static constexpr int CPR = ROWB / 16;                   // chunks per row
    static constexpr int KTQ = DHP <= 128 ? KT : BPM_ATTN_KT256_DQ;   // keys per tile of the dQ pass
    static constexpr int QTK = DHP <= 128 || SZ == 2 ? QT : BPM_ATTN_QT256_F32;   // queries per tile of the dK / dV pass
};

// cooperative copy of `rows` head rows (global row index row0.., bound nrows) into an LDS image
template <typename CT, int DHP, int ROWS>
BPM_DEV void load_rows(char* img, const char* src, int row0, int nrows, int tid) {
    typedef Cfg<CT, DHP> C;
    constexpr int N = ROWS * C::CPR;
#pragma unroll
    for (int c = tid; c < N; c += NTHREADS) {
        const int row = c / C::CPR, cc = c % C::CPR;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (row0 + row < nrows) v = *(const u32x4*)(src + (size_t)(row0 + row) * C::ROWB + cc * 16);
        *(u32x4*)(img + row * C::STRIDE + cc * 16) = v;
    }
}

// the same copy split in two: global -> registers (issued one tile ahead, behind the current tile's arithmetic)
// and registers -> LDS image.  Loads are unconditional from a clamped row (row 0 always exists) and zeroed by
// a select, so no branch sits between the load and its use.
template <typename CT, int DHP, int ROWS>
struct RowStage {
    typedef Cfg<CT, DHP> C;
    static constexpr int N = ROWS * C::CPR;
    static constexpr int PT = (N + NTHREADS - 1) / NTHREADS;
    u32x4 r[PT];
    // `src` is wave-uniform (a head's first row): buffer loads through a descriptor of nrows rows, so rows past the end
    // come back as zeros from the range check instead of a clamp + select per dword (16 v_cndmask per tile and wave)
    BPM_DEV void load(const char* src, int row0, int nrows, int tid) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, nrows * C::ROWB, 0x00020000);
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int c = tid + i * NTHREADS;
            const int row = c / C::CPR, cc = c % C::CPR;
            int voff = (row0 + row) * C::ROWB + cc * 16;
            if (N % NTHREADS != 0 && c >= N) voff = 0x7fffffff;
            r[i] = (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
        }
    }
    BPM_DEV void store(char* img, int tid) const {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int c = tid + i * NTHREADS;
            if (N % NTHREADS != 0 && c >= N) continue;
            *(u32x4*)(img + (c / C::CPR) * C::STRIDE + (c % C::CPR) * 16) = r[i];
        }
    }
};

// operand chunk straight from a head-major global row (zero beyond nrows)
template <typename CT, int DHP>
BPM_DEV typename Tr<CT>::frag load_frag(const char* src, int row, int nrows, int ks, int g) {
    typedef Cfg<CT, DHP> C;
    if (row >= nrows) return Tr<CT>::zero();
    return *(const typename Tr<CT>::frag*)(src + (size_t)row * C::ROWB + ks * 64 + g * 16);
}

BPM_DEV const AProb& pick(const AGroup& grp, int& bid) {
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    bid -= grp.p[pi].blk0;
    return grp.p[pi];
}

BPM_DEV int pick_index(const AGroup& grp, int& bid) {      // the *_kmask kernels: the problem's index also selects its mask
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    bid -= grp.p[pi].blk0;
    return pi;
}

// ---------------------------------------------------------------------------
// Row-contiguous store of one wave's 16 x dh result tile.  The MFMA leaves lane (c = lane & 15, g = lane >> 4) with
// columns 16n + 4g + r of row c; written from there, every element is its own 2-byte request to L2 (64 lanes x 16
// instructions per wave): measured on MI355X at B*H = 576 heads of 64, T = S = 512, the forward launch spent 54 of its
// 105 us in those stores, the dQ pass 98 of 144 (plus the same pattern reading O for delta) and dK/dV 95 of 167 --
// 19 M requests per output tensor at ~300 G requests/s.  Instead the wave passes the tile through a private LDS block
// (rows padded by 16 bytes: conflict-free for the 8-byte writes and the 16-byte reads) and stores whole 16-byte chunks
// with consecutive lanes on consecutive chunks of a row (a 64-wide head row is one 128-byte line per 8 lanes).
// Head dims that are not whole 16-byte chunks (25 at hidden 300) go element-wise, lanes along the row.
// Row i of the tile lives at base + i * rstride (elements); rows >= nvalid are not written.
// ---------------------------------------------------------------------------
template <typename CT, int DHP>
BPM_DEV void store_rows16(char* blk, CT* base, size_t rstride, int nvalid, int dh, const f32x4 (&acc)[DHP / 16], float scale, int lane) {
    constexpr int SZ = sizeof(CT), RS = DHP * SZ + 16, EPC = 16 / SZ;
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int n = 0; n < DHP / 16; ++n) {
        const f32x4 v = acc[n] * scale;
        char* dst = blk + c * RS + (16 * n + 4 * g) * SZ;
        if constexpr (SZ == 4) *(f32x4*)dst = v;
        else { bf16x4 o; o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3]; *(bf16x4*)dst = o; }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave: its LDS accesses execute in order; this also pins the compiler
    const bool wide = (dh % EPC) == 0 && (((uintptr_t)base | (uintptr_t)(rstride * SZ)) & 15) == 0;
    if (wide && dh == DHP) {                                // the usual case (head_dim 64 / 128): row / chunk by shifts, no
        constexpr int cpr = DHP / EPC, total = 16 * cpr;    // run-time division (that was ~60 VALU instructions per tile)
#pragma unroll
        for (int idx0 = 0; idx0 < total; idx0 += 64) {
            const int idx = idx0 + lane;
            const int row = idx / cpr, ch = idx % cpr;
            if (row < nvalid) *(u32x4*)(base + (size_t)row * rstride + ch * EPC) = *(const u32x4*)(blk + row * RS + ch * 16);
        }
    } else if (wide) {
        const int cpr = dh / EPC, total = 16 * cpr;
        for (int idx = lane; idx < total; idx += 64) {
            const int row = idx / cpr, ch = idx - row * cpr;
            if (row < nvalid) *(u32x4*)(base + (size_t)row * rstride + ch * EPC) = *(const u32x4*)(blk + row * RS + ch * 16);
        }
    } else {
        const int total = 16 * dh;
        for (int idx = lane; idx < total; idx += 64) {
            const int row = idx / dh, col = idx - row * dh;
            if (row < nvalid) base[(size_t)row * rstride + col] = *(const CT*)(blk + row * RS + col * SZ);
        }
    }
}
template <typename CT, int DHP> constexpr int store_rows16_bytes() { return 16 * (DHP * (int)sizeof(CT) + 16); }

BPM_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32: exp2(-inf) = 0, no denormal fix-up

// ---------------------------------------------------------------------------
// host side: the pieces every attention entry is built from
// ---------------------------------------------------------------------------
// launch: f(std::integral_constant<int, D>()) with the padded head_dim the kernels are instantiated at
template <typename F> inline int with_dhp(int dhp, F&& f) {
    switch (dhp) {
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
        case 128: return f(std::integral_constant<int, 128>());
        case 256: return f(std::integral_constant<int, 256>());
        default: return BPM_ERR_ARG;
    }
}

// check: what can be refused without touching the device, each rule written once.  All of them are BPM_ERR_ARG; the
// entries keep the ORDER in which they test them (it decides the code of a call with an argument and an alignment fault).
inline bool dtype_ok(int dtype) { return dtype == BPM_BF16 || dtype == BPM_F32; }
inline bool group_ok(const void* probs, int nprob) { return nprob >= 1 && nprob <= BPM_MAX_GROUP && probs; }

// the geometry of one problem (bpm_attn_problem or bpm_attn_map_problem) of a group whose first problem has dhp0
template <typename Q> inline bool geometry_ok(const Q& q, int dhp0) {
    if (q.B < 1 || q.H < 1 || q.T < 1 || q.S < 1 || q.dh < 1 || q.dh > q.dhp) return false;
    if (q.T > (1 << 22) || q.S > (1 << 22)) return false;      // index arithmetic is 32-bit (rows * 512 B per head fits 31 bits)
    if ((long)(q.T > q.S ? q.T : q.S) * q.dhp * 4 > (1l << 31)) return false;   // ... and rows * 1 KiB at head_dim 256 in f32
    return q.dhp == dhp0;
}

// the mask_off rule of problem q as the kernels take it (p: AProb, MProb or DProb): the clamped offset and the query
// positions; false for a q_pos0 / q_stride out of range or a last position past 2^28
template <typename Q, typename P> inline bool positions(const Q& q, P& p) {
    if (q.q_pos0 < 0 || q.q_stride < 0 || q.q_pos0 > (1 << 24) || q.q_stride > (1 << 24)) return false;
    p.mask_off = (q.mask_off > 0 && q.mask_off < (1 << 29)) ? q.mask_off : (1 << 29);
    p.qpos0 = q.q_pos0; p.qstride = q.q_stride > 0 ? q.q_stride : 1;
    return (long)p.qpos0 + (long)(q.T - 1) * p.qstride <= (1l << 28);
}

// the pointers a launch needs.  parts: 0 forward; backward: bit 0 dQ (+ delta), bit 1 dK / dV -- a masked entry's
// `which` (0 forward, 1 dQ, 2 dK / dV) reads the same way
inline bool pointers_ok(const bpm_attn_problem* probs, int nprob, int parts) {
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        if (!q.Q || !q.K || !q.V || !q.O || !q.lse) return false;
        if (parts != 0 && (!q.dO || !q.delta)) return false;
        if ((parts & 1) && !q.dQ) return false;
        if ((parts & 2) && (!q.dK || !q.dV)) return false;
    }
    return true;
}

// sum over problems of B*H*dh * (number of visible (query, key) pairs): the useful
// multiply-adds of ONE attention product (P(T,S) = sum_i min(S, i + mask_off))
inline double useful_pair_flops(const bpm_attn_problem* probs, int nprob) {
    double tot = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        double pairs = 0;
        if (q.mask_off <= 0) pairs = (double)q.T * q.S;
        else
            for (int t = 0; t < q.T; ++t) {
                const long tt = (long)q.q_pos0 + (long)t * (q.q_stride > 0 ? q.q_stride : 1);
                pairs += (double)(tt + q.mask_off < (long)q.S ? tt + q.mask_off : q.S);
            }
        tot += pairs * q.dh * q.B * q.H;
    }
    return tot;
}

// One additive mask as a kernel reads it: `transposed` false: (mask, ldm) against [T, S]; true: (maskT, ldt) against [S, T].
// The forward-oriented array must be there in every entry (it is the mask; maskT only restates it).  float4 reads: the
// base 16-byte aligned, the leading dimension a multiple of 4.
// A head stride (0: one image for all heads) keeps every head image under the same rules: a multiple of 4 elements, at
// least one image long, and within 31 bits (the kernels carry it as an int).
inline int amask_desc(AAdd& a, const bpm_attn_hmask& m, int T, int S, bool transposed) {
    if (!m.mask || m.ldm < S || (m.ldm & 3) || ((uintptr_t)m.mask & 15)) return BPM_ERR_ARG;
    if (transposed && (!m.maskT || m.ldt < T || (m.ldt & 3) || ((uintptr_t)m.maskT & 15))) return BPM_ERR_ARG;
    const int64_t hs = transposed ? m.head_strideT : m.head_stride;
    const int64_t image = transposed ? (int64_t)S * m.ldt : (int64_t)T * m.ldm;
    if (hs != 0 && (hs < image || (hs & 3) || hs > 0x7fffffff)) return BPM_ERR_ARG;
    if (m.head_stride != 0 && (m.head_stride < (int64_t)T * m.ldm || (m.head_stride & 3) || m.head_stride > 0x7fffffff)) return BPM_ERR_ARG;
    a.m = transposed ? m.maskT : m.mask;
    a.ld = transposed ? m.ldt : m.ldm;
    a.hs = (int)hs;
    return 0;
}

// One per-sample mask (bpm_attn_bmask): the rules of amask_desc for the image(s) of one sample, and for a non-zero batch
// stride those of a head stride one level up: a multiple of 4 elements, at least the images of one sample long (H head
// strides, or one image when the head stride is 0), and within 31 bits.
inline int bmask_desc(AAddB& a, const bpm_attn_bmask& m, int H, int T, int S, bool transposed) {
    AAdd one;
    const bpm_attn_hmask hm{m.mask, m.ldm, m.maskT, m.ldt, m.head_stride, m.head_strideT};
    const int rc = amask_desc(one, hm, T, S, transposed);
    if (rc) return rc;
    auto stride_ok = [&](int64_t bs, int64_t hs, int64_t image) {
        return bs == 0 || (!(bs & 3) && bs <= 0x7fffffff && bs >= (hs != 0 ? (int64_t)H * hs : image));
    };
    if (!stride_ok(m.batch_stride, m.head_stride, (int64_t)T * m.ldm)) return BPM_ERR_ARG;
    if (transposed && !stride_ok(m.batch_strideT, m.head_strideT, (int64_t)S * m.ldt)) return BPM_ERR_ARG;
    a = AAddB{one.m, one.ld, one.hs, (int)(transposed ? m.batch_strideT : m.batch_stride)};
    return 0;
}

// either of the two, by the descriptor's type (the fills that serve both families)
inline int image_desc(AAdd& a, const bpm_attn_hmask& m, int, int T, int S, bool transposed) { return amask_desc(a, m, T, S, transposed); }
inline int image_desc(AAddB& a, const bpm_attn_bmask& m, int H, int T, int S, bool transposed) { return bmask_desc(a, m, H, T, S, transposed); }

// One byte mask as the kernels read it: bytes [B, ldm], ldm >= S (the kernels never read at j >= S: a tight [B, S] is legal).
inline int kmask_desc(AMask& k, const bpm_attn_kmask& m, int S) {
    if (!m.mask || m.ldm < S) return BPM_ERR_ARG;
    k = AMask{m.mask, m.ldm};
    return 0;
}

// The *_amask entries are the *_hmask entries at head stride 0: their masks are restated as bpm_attn_hmask on the host.
struct HMasks {
    bpm_attn_hmask m[BPM_MAX_GROUP];
    const bpm_attn_hmask* p = nullptr;      // stays NULL for arguments the callee refuses (no array, nprob out of range)
    HMasks(const bpm_attn_amask* masks, int nprob) {
        if (!masks || nprob < 1 || nprob > BPM_MAX_GROUP) return;
        for (int i = 0; i < nprob; ++i) m[i] = bpm_attn_hmask{masks[i].mask, masks[i].ldm, masks[i].maskT, masks[i].ldt, 0, 0};
        p = m;
    }
};
}  // namespace
